// Fused per-channel softmax aggregation for the kgx engine (gfx950, wave64): the learnable
// aggregation of DeeperGCN (PyG's SoftmaxAggregation, the aggregation of GENConv),
//   r_t = x[j] + edge[e_t]      m_t = r_t  or  max(r_t, 0) + eps      s_t = temp[c] * m_t
//   out[i] = sum_t softmax_t(s_t) * m_t                (every channel its own softmax over the row)
// and its backward.  No [E, F] tensor exists in either direction: the backward recomputes
// every weight from x, edge, temp, out and the per-row stats (M | S) of the forward.
//
// Row-owned lanes over the hub-split schedule (the walk of kgx_attn.h) in the float4-piece
// layout of gated.hip: a group of G = 2^lgG lanes owns a work item, lane l holds NP float4
// pieces of the row, piece p at columns 4 (l + p G); NP = 1 up to F = 256, 2 above.  The
// softmax state is per channel, so it lives in the lane that holds the channel: running
// max M (fp32), denominator S, numerator N = sum w m and second moment Q = sum w m^2
// (fp64).  Nothing crosses lanes: no LDS tile, no reduction.  (The attention core keeps one
// (max, denominator) per head and reduces a score across lanes; here that would be F
// reductions per edge.)
//
// The state moves once per block of U slots, not per slot: the block's max per channel, one
// rescale exponential for the block, then U weight exponentials -- (1 + 1/U) expf per
// channel and edge, where a slot-by-slot online softmax takes two.  The terms are fp32
// (expf, the products' operands); S, N, Q and the source pass's gradient sums are carried in
// fp64, which holds a 1000-slot row at a few percent of 1e-5 max(1, A) where sequential fp32
// sums reach the bound itself.  The fp64 FMAs hide under the row gathers.
//
// Hub chunks store (M | S | N | Q) partials, merged in chunk order by a fix-up; the source
// pass stores [F] partials added in chunk order.  One writer per element, no atomics: the
// same bits from run to run, in split and in exact mode alike.
//
// Backward, with g = grad_out and p_t = exp(s_t - M) / S:
//   d m_t = g p_t (1 + temp (m_t - out))  =  (g / S) exp(temp m_t - M) ((1 - temp out) + temp m_t)
// A prologue packs each destination into one row (g / S | M | 1 - temp out) of a [n_dst, 3F]
// workspace, so the source pass gathers one contiguous 12F-byte run per slot instead of rows
// of four tables.  The destination pass (grad_edge, one writer per row, no sums) owns the
// destination and forms the same three values in registers.
#include "kgx_attn.h"

namespace kgx {
namespace {

template <int NP>
constexpr int unroll() {
  return NP == 1 ? 4 : 2;
}

// This thread's pieces of a row (the layout of gated.hip).
template <int NP>
struct RowLanes {
  int c[NP];
  bool ok[NP];
  __device__ __forceinline__ RowLanes(int lgG, int F) {
    const int lane = threadIdx.x & ((1 << lgG) - 1);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int col = 4 * (lane + (p << lgG));
      ok[p] = col < F;
      c[p] = ok[p] ? col : 0;  // a piece past F loads column 0 (a valid address) and stores nothing
    }
  }
};

template <int NP>
__device__ __forceinline__ void load_row(float (&d)[NP][4], const float* __restrict__ row, const RowLanes<NP>& L) {
#pragma unroll
  for (int p = 0; p < NP; ++p) vload<4>(d[p], row + L.c[p]);
}

template <int NP>
__device__ __forceinline__ void store_row(float* __restrict__ row, const float (&d)[NP][4], const RowLanes<NP>& L) {
#pragma unroll
  for (int p = 0; p < NP; ++p)
    if (L.ok[p]) vstore<4>(row + L.c[p], d[p]);
}

template <int NP>
__device__ __forceinline__ void store_row(float* __restrict__ row, const double (&d)[NP][4], const RowLanes<NP>& L) {
  float f[NP][4];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int i = 0; i < 4; ++i) f[p][i] = float(d[p][i]);
  store_row<NP>(row, f, L);
}

template <int NP, typename T>
__device__ __forceinline__ void fill_row(T (&d)[NP][4], T v) {
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int i = 0; i < 4; ++i) d[p][i] = v;
}

// The message operands of all kernels: x rows (null: by-edge messages) and the edge table
// (null: none).  Not both null.
struct Msg {
  const float* x;
  int64_t ld_x;
  const float* edge;
  int64_t ld_e;
  int32_t n_e;
  const float* temp;
  int gen;  // 0: m = r; 1: m = max(r, 0) + eps
  float eps;
  // the edge row of slot t under idx, clamped to a row that exists; has: it is the slot's own
  __device__ __forceinline__ int32_t row(const int32_t* idx, int32_t t, bool& has) const {
    int32_t r;
    has = edge_row(idx, n_e, t, r);
    return has ? r : 0;
  }
  // r = x + edge by this one rounded add in every kernel, so the backward sees the forward's r
  template <bool kX, bool kEdge>
  __device__ __forceinline__ float r(float xv, float ev, bool has) const {
    const float e = (kEdge && has) ? ev : 0.0f;
    return kX ? (kEdge ? xv + e : xv) : e;
  }
  __device__ __forceinline__ float m(float rv) const { return gen ? fmaxf(rv, 0.0f) + eps : rv; }
};

// The per-channel softmax state of one lane.
template <int NP>
struct State {
  float M[NP][4];
  double S[NP][4], N[NP][4], Q[NP][4];
  __device__ __forceinline__ State() {
    fill_row<NP>(M, -__builtin_inff());
    fill_row<NP>(S, 0.0);
    fill_row<NP>(N, 0.0);
    fill_row<NP>(Q, 0.0);
  }
  // moves channel (p, i) to a max of at least mb: one exponential (M = -inf: the sums are still 0)
  __device__ __forceinline__ void raise(int p, int i, float mb) {
    const float m_new = fmaxf(M[p][i], mb);
    const double f = m_new > M[p][i] ? double(expf(M[p][i] - m_new)) : 1.0;
    S[p][i] *= f;
    N[p][i] *= f;
    Q[p][i] *= f;
    M[p][i] = m_new;
  }
  // adds the slot of message m whose weight under M is w
  __device__ __forceinline__ void add(int p, int i, double w, double m) {
    S[p][i] += w;
    const double wm = w * m;
    N[p][i] += wm;
    Q[p][i] = fma(wm, m, Q[p][i]);
  }
};

struct FwdArgs {
  Sched sched;
  const int32_t* col;
  const int32_t* e_idx;
  Msg msg;
  int F, lgG;
  float* out;
  int64_t ld_o;
  float* stats;  // [n_rows, ld_s]: M | S (| Q when stats_q), null: not kept
  int64_t ld_s;
  int stats_q;
  float* partials;  // [n_slots, 4F]: M | S | N | Q
};

// A whole row's state into out and stats.  A row without slots stores zeros.
template <int NP>
__device__ __forceinline__ void finish_row(const FwdArgs& a, const RowLanes<NP>& L, int32_t row, const State<NP>& st,
                                           bool empty) {
  float o[NP][4], s[NP][4], q[NP][4], mx[NP][4];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      o[p][i] = empty ? 0.0f : float(st.N[p][i] / st.S[p][i]);
      q[p][i] = empty ? 0.0f : float(st.Q[p][i] / st.S[p][i]);
      s[p][i] = float(st.S[p][i]);
      mx[p][i] = empty ? 0.0f : st.M[p][i];
    }
  store_row<NP>(a.out + int64_t(row) * a.ld_o, o, L);
  if (a.stats) {
    float* sp = a.stats + int64_t(row) * a.ld_s;
    store_row<NP>(sp, mx, L);
    store_row<NP>(sp + a.F, s, L);
    if (a.stats_q) store_row<NP>(sp + 2 * a.F, q, L);
  }
}

template <int NP, bool kX, bool kEdge>
__global__ __launch_bounds__(kBlock) void softmax_aggr_kernel(FwdArgs a) {
  constexpr int U = unroll<NP>();
  const RowLanes<NP> L(a.lgG, a.F);
  const int64_t ngroups = group_count(a.lgG);
  const int64_t n_work = a.sched.n_work();
  float temp[NP][4];
  load_row<NP>(temp, a.msg.temp, L);
  for (int64_t it = first_group(a.lgG); it < n_work; it += ngroups) {
    int32_t row, beg, end, slot;
    work_item(a.sched, it, row, beg, end, slot);
    State<NP> st;
    for (int32_t e = beg; e < end; e += U) {
      int32_t c[U], r[U];
      bool has[U];
      float xv[U][NP][4], ev[U][NP][4];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t ee = e + u < end ? e + u : end - 1;  // slots past the end re-read the last one
        c[u] = kX ? a.col[ee] : 0;
        has[u] = false;
        r[u] = kEdge ? a.msg.row(a.e_idx, ee, has[u]) : 0;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if constexpr (kX) load_row<NP>(xv[u], a.msg.x + row_off(c[u], a.msg.ld_x), L);
        if constexpr (kEdge) load_row<NP>(ev[u], a.msg.edge + row_off(r[u], a.msg.ld_e), L);
      }
      const int n = end - e;  // the block's slots (U or more: a full block)
#pragma unroll
      for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float m[U], s[U], mb = -__builtin_inff();
#pragma unroll
          for (int u = 0; u < U; ++u) {
            m[u] = a.msg.m(a.msg.r<kX, kEdge>(kX ? xv[u][p][i] : 0.0f, kEdge ? ev[u][p][i] : 0.0f, has[u]));
            s[u] = temp[p][i] * m[u];
            mb = u < n ? fmaxf(mb, s[u]) : mb;
          }
          st.raise(p, i, mb);
#pragma unroll
          for (int u = 0; u < U; ++u)
            if (u < n) st.add(p, i, double(expf(s[u] - st.M[p][i])), double(m[u]));
        }
    }
    if (slot >= 0) {
      float* pp = a.partials + int64_t(slot) * 4 * a.F;
      store_row<NP>(pp, st.M, L);
      store_row<NP>(pp + a.F, st.S, L);
      store_row<NP>(pp + 2 * a.F, st.N, L);
      store_row<NP>(pp + 3 * a.F, st.Q, L);
    } else {
      finish_row<NP>(a, L, row, st, beg == end);
    }
  }
}

// Split rows: the chunk partials merged in chunk order, B chunks' loads in flight and one
// rescale exponential per batch, as the main kernel's blocks.
template <int NP>
__global__ __launch_bounds__(kBlock) void softmax_aggr_fixup_kernel(FwdArgs a) {
  constexpr int B = 4 / NP;
  const RowLanes<NP> L(a.lgG, a.F);
  const int64_t ngroups = group_count(a.lgG);
  for (int64_t it = first_group(a.lgG); it < a.sched.n_split; it += ngroups) {
    const int4 sp = a.sched.split[it];
    State<NP> st;
    for (int32_t c0 = 0; c0 < sp.z; c0 += B) {
      float pm[B][NP][4], ps[B][NP][4], pn[B][NP][4], pq[B][NP][4];
#pragma unroll
      for (int u = 0; u < B; ++u) {
        const float* pp = a.partials + int64_t(sp.y + (c0 + u < sp.z ? c0 + u : sp.z - 1)) * 4 * a.F;
        load_row<NP>(pm[u], pp, L);
        load_row<NP>(ps[u], pp + a.F, L);
        load_row<NP>(pn[u], pp + 2 * a.F, L);
        load_row<NP>(pq[u], pp + 3 * a.F, L);
      }
      const int n = sp.z - c0;
#pragma unroll
      for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float mb = -__builtin_inff();
#pragma unroll
          for (int u = 0; u < B; ++u) mb = u < n ? fmaxf(mb, pm[u][p][i]) : mb;
          st.raise(p, i, mb);
#pragma unroll
          for (int u = 0; u < B; ++u)
            if (u < n) {
              const double w = double(expf(pm[u][p][i] - st.M[p][i]));
              st.S[p][i] = fma(w, double(ps[u][p][i]), st.S[p][i]);
              st.N[p][i] = fma(w, double(pn[u][p][i]), st.N[p][i]);
              st.Q[p][i] = fma(w, double(pq[u][p][i]), st.Q[p][i]);
            }
        }
    }
    finish_row<NP>(a, L, sp.x, st, false);
  }
}

// ===========================================================================
// Backward
// ===========================================================================
// d r of one channel from the destination's packed values A = g / S, M, C = 1 - temp out.
// A weight of exactly 0 gives exactly 0; under the GEN message r <= 0 is selected to 0.
__device__ __forceinline__ float dr_of(const Msg& mg, float rv, float temp, float A, float M, float C) {
  const float m = mg.m(rv);
  const float s = temp * m;
  const float d = (A * expf(s - M)) * (C + s);
  return (mg.gen && !(rv > 0.0f)) ? 0.0f : d;
}

struct PackArgs {
  const float *grad, *out, *stats, *temp;
  int64_t ld_g, ld_o, ld_s;
  int64_t n_rows;
  int F;
  float* packed;  // [n_rows, 3F]: g / S | M | 1 - temp out
};

// One destination's packed values in this lane's pieces; a row without slots (S = 0) packs A = 0.
template <int NP>
__device__ __forceinline__ void pack_row(const float* g, const float* out, const float* stats, int F,
                                         const float (&temp)[NP][4], const RowLanes<NP>& L, float (&A)[NP][4],
                                         float (&M)[NP][4], float (&C)[NP][4]) {
  float gv[NP][4], ov[NP][4], sv[NP][4];
  load_row<NP>(gv, g, L);
  load_row<NP>(ov, out, L);
  load_row<NP>(M, stats, L);
  load_row<NP>(sv, stats + F, L);
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      A[p][i] = sv[p][i] > 0.0f ? __fdiv_rn(gv[p][i], sv[p][i]) : 0.0f;
      C[p][i] = 1.0f - temp[p][i] * ov[p][i];
    }
}

template <int NP>
__global__ __launch_bounds__(kBlock) void softmax_aggr_pack_kernel(PackArgs a, int lgG) {
  const RowLanes<NP> L(lgG, a.F);
  const int64_t ngroups = group_count(lgG);
  float temp[NP][4];
  load_row<NP>(temp, a.temp, L);
  for (int64_t row = first_group(lgG); row < a.n_rows; row += ngroups) {
    float A[NP][4], M[NP][4], C[NP][4];
    pack_row<NP>(a.grad + row * a.ld_g, a.out + row * a.ld_o, a.stats + row * a.ld_s, a.F, temp, L, A, M, C);
    float* w = a.packed + row * 3 * a.F;
    store_row<NP>(w, A, L);
    store_row<NP>(w + a.F, M, L);
    store_row<NP>(w + 2 * a.F, C, L);
  }
}

struct BwdArgs {
  Sched sched;
  const int32_t* idx;    // per slot: the node at its other end
  const int32_t* e_idx;  // per slot: its edge row (null: the slot itself)
  Msg msg;
  int F, lgG;
  // destination pass: the destination's own rows
  const float *grad, *out, *stats;
  int64_t ld_g, ld_o, ld_s;
  float* grad_edge;
  int64_t ld_ge;
  // source pass: the packed destination rows, chunk partials [t_n_slots, F], grad_x
  const float* packed;
  float* partials;
  float* grad_x;
  int64_t ld_gx;
};

// Destination pass over the CSR (launched with an edge table only): grad_edge[e_t] = d r_t.
template <int NP, bool kX>
__global__ __launch_bounds__(kBlock) void softmax_aggr_bwd_dst_kernel(BwdArgs a) {
  constexpr int U = unroll<NP>();
  const RowLanes<NP> L(a.lgG, a.F);
  const int64_t ngroups = group_count(a.lgG);
  const int64_t n_work = a.sched.n_work();
  float temp[NP][4];
  load_row<NP>(temp, a.msg.temp, L);
  for (int64_t it = first_group(a.lgG); it < n_work; it += ngroups) {
    int32_t row, beg, end, slot;
    work_item(a.sched, it, row, beg, end, slot);
    if (beg == end) continue;
    float A[NP][4], M[NP][4], C[NP][4];
    pack_row<NP>(a.grad + int64_t(row) * a.ld_g, a.out + int64_t(row) * a.ld_o, a.stats + int64_t(row) * a.ld_s, a.F,
                 temp, L, A, M, C);
    for (int32_t e = beg; e < end; e += U) {
      int32_t c[U], r[U];
      bool has[U];
      float xv[U][NP][4], ev[U][NP][4];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t ee = e + u < end ? e + u : end - 1;
        c[u] = kX ? a.idx[ee] : 0;
        r[u] = a.msg.row(a.e_idx, ee, has[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if constexpr (kX) load_row<NP>(xv[u], a.msg.x + row_off(c[u], a.msg.ld_x), L);
        load_row<NP>(ev[u], a.msg.edge + row_off(r[u], a.msg.ld_e), L);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (e + u < end && has[u]) {
          float d[NP][4];
#pragma unroll
          for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int i = 0; i < 4; ++i)
              d[p][i] = dr_of(a.msg, a.msg.r<kX, true>(kX ? xv[u][p][i] : 0.0f, ev[u][p][i], true), temp[p][i],
                              A[p][i], M[p][i], C[p][i]);
          store_row<NP>(a.grad_edge + row_off(r[u], a.ld_ge), d, L);
        }
      }
    }
  }
}

// Source pass over the transposed CSR (launched with an x only): grad_x[j] = sum over j's
// out-slots of d r_t.  The group keeps x[j] for all its slots and gathers one packed
// destination row (and the edge row) per slot; the sum is fp64.
template <int NP, bool kEdge>
__global__ __launch_bounds__(kBlock) void softmax_aggr_bwd_src_kernel(BwdArgs a) {
  constexpr int U = unroll<NP>();
  const RowLanes<NP> L(a.lgG, a.F);
  const int64_t ngroups = group_count(a.lgG);
  const int64_t n_work = a.sched.n_work();
  float temp[NP][4];
  load_row<NP>(temp, a.msg.temp, L);
  for (int64_t it = first_group(a.lgG); it < n_work; it += ngroups) {
    int32_t row, beg, end, slot;
    work_item(a.sched, it, row, beg, end, slot);
    float xv[NP][4];
    double acc[NP][4];
    load_row<NP>(xv, a.msg.x + int64_t(row) * a.msg.ld_x, L);
    fill_row<NP>(acc, 0.0);
    for (int32_t e = beg; e < end; e += U) {
      int32_t c[U], r[U];
      bool has[U];
      float A[U][NP][4], M[U][NP][4], C[U][NP][4], ev[U][NP][4];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t ee = e + u < end ? e + u : end - 1;
        c[u] = a.idx[ee];
        has[u] = false;
        r[u] = kEdge ? a.msg.row(a.e_idx, ee, has[u]) : 0;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float* w = a.packed + row_off(c[u], 3 * int64_t(a.F));
        load_row<NP>(A[u], w, L);
        load_row<NP>(M[u], w + a.F, L);
        load_row<NP>(C[u], w + 2 * a.F, L);
        if constexpr (kEdge) load_row<NP>(ev[u], a.msg.edge + row_off(r[u], a.msg.ld_e), L);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (e + u < end) {
#pragma unroll
          for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int i = 0; i < 4; ++i)
              acc[p][i] += double(dr_of(a.msg, a.msg.r<true, kEdge>(xv[p][i], kEdge ? ev[u][p][i] : 0.0f, has[u]),
                                        temp[p][i], A[u][p][i], M[u][p][i], C[u][p][i]));
        }
      }
    }
    store_row<NP>(slot >= 0 ? a.partials + int64_t(slot) * a.F : a.grad_x + int64_t(row) * a.ld_gx, acc, L);
  }
}

constexpr int64_t kLim = int64_t(1) << 31;

// Pieces per lane and lanes per group of an F-wide row.
inline int pieces_of(int64_t F) { return F > 256 ? 2 : 1; }
inline int lg_group(int64_t F) { return log2i(next_pow2(int((F / 4 + pieces_of(F) - 1) / pieces_of(F)))); }

template <int NP>
int launch_fwd(const FwdArgs& a, bool x, bool edge, hipStream_t s) {
  const int G = 1 << a.lgG;
  const int64_t n = a.sched.n_work();
  const int rc = !x     ? launch_resident(softmax_aggr_kernel<NP, false, true>, n, G, a, s)
                 : edge ? launch_resident(softmax_aggr_kernel<NP, true, true>, n, G, a, s)
                        : launch_resident(softmax_aggr_kernel<NP, true, false>, n, G, a, s);
  if (rc) return rc;
  return launch_resident(softmax_aggr_fixup_kernel<NP>, a.sched.n_split, G, a, s);
}

template <int NP>
int launch_pack(const PackArgs& a, int lgG, hipStream_t s) {
  auto kernel = softmax_aggr_pack_kernel<NP>;
  hipLaunchKernelGGL(kernel, dim3(resident_grid(kernel, a.n_rows, 1 << lgG)), dim3(kBlock), 0, s, a, lgG);
  KGX_CHECK_LAUNCH();
  return KGX_OK;
}

template <int NP>
int launch_dst(const BwdArgs& a, bool x, hipStream_t s) {
  const int G = 1 << a.lgG;
  return x ? launch_resident(softmax_aggr_bwd_dst_kernel<NP, true>, a.sched.n_work(), G, a, s)
           : launch_resident(softmax_aggr_bwd_dst_kernel<NP, false>, a.sched.n_work(), G, a, s);
}

template <int NP>
int launch_src(const BwdArgs& a, bool edge, hipStream_t s) {
  const int G = 1 << a.lgG;
  const int rc = edge ? launch_resident(softmax_aggr_bwd_src_kernel<NP, true>, a.sched.n_work(), G, a, s)
                      : launch_resident(softmax_aggr_bwd_src_kernel<NP, false>, a.sched.n_work(), G, a, s);
  if (rc) return rc;
  return launch_chunk_sum(a.sched, a.partials, a.F, a.F, a.F, a.grad_x, a.ld_gx, a.grad_x, a.ld_gx, s);
}

struct BwdCarve {
  float *packed, *t_partials;
  size_t bytes;
};
inline BwdCarve carve_bwd(void* ws, size_t cap, int64_t n_rows, int64_t t_n_slots, int64_t F) {
  Carve c(ws, cap);
  BwdCarve b;
  b.packed = c.take<float>(size_t(n_rows) * 3 * size_t(F));
  b.t_partials = c.take<float>(size_t(t_n_slots) * size_t(F));
  b.bytes = c.used();
  return b;
}

// A table read four floats at a time: present, wide enough, below 2^31, aligned.
int check_table(const char* fn, const char* what, const void* p, int64_t ld, int64_t W, bool required) {
  KGX_REQUIRE(p || !required, KGX_ERR_ARG, "%s: %s is null", fn, what);
  if (!p) return KGX_OK;
  KGX_REQUIRE(ld >= W && ld < kLim, KGX_ERR_ARG, "%s: leading dimension of %s (%lld) below its width %lld or >= 2^31",
              fn, what, (long long)ld, (long long)W);
  KGX_REQUIRE(attn_vec_ok(16, {p}, {ld}), KGX_ERR_UNSUPPORTED,
              "%s: %s is read four floats at a time: a 16-byte aligned address and a leading dimension that is a "
              "multiple of 4 (got ld %lld)", fn, what, (long long)ld);
  return KGX_OK;
}

int check_shape(const char* fn, int64_t F, const float* x, const float* edge, int64_t n_e, const float* temp,
                int message, float eps) {
  KGX_REQUIRE(F >= 1, KGX_ERR_ARG, "%s: F = %lld", fn, (long long)F);
  KGX_REQUIRE(!edge || (n_e >= 0 && n_e < kLim), KGX_ERR_ARG, "%s: edge table rows n_e = %lld outside [0, 2^31)", fn,
              (long long)n_e);
  KGX_REQUIRE(x || (edge && n_e > 0), KGX_ERR_ARG, "%s: x and edge are both absent: no message", fn);
  KGX_REQUIRE(temp, KGX_ERR_ARG, "%s: temp is null", fn);
  KGX_REQUIRE(message == KGX_SOFTMAX_MSG_IDENTITY || message == KGX_SOFTMAX_MSG_GEN, KGX_ERR_ARG,
              "%s: message %d (0 identity, 1 gen)", fn, message);
  KGX_REQUIRE(eps == eps, KGX_ERR_ARG, "%s: eps is NaN", fn);
  KGX_REQUIRE(F % 4 == 0 && F <= 512, KGX_ERR_UNSUPPORTED, "%s: F = %lld (F a multiple of 4 in [4, 512])", fn,
              (long long)F);
  return KGX_OK;
}

}  // namespace
}  // namespace kgx

using namespace kgx;

#define KGX_TRY(expr)                      \
  do {                                     \
    const int kgx_rc_ = (expr);            \
    if (kgx_rc_ != KGX_OK) return kgx_rc_; \
  } while (0)

extern "C" int kgx_softmax_aggr(const kgx_softmax_aggr_args* p, kgx_stream_t stream_) {
  const char* fn = "kgx_softmax_aggr";
  KGX_REQUIRE(p && p->struct_size == sizeof(kgx_softmax_aggr_args), KGX_ERR_ARG,
              "kgx_softmax_aggr: struct_size %llu is not this header's %zu",
              p ? (unsigned long long)p->struct_size : 0ull, sizeof(kgx_softmax_aggr_args));
  KGX_REQUIRE(p->n_rows >= 0 && p->n_rows < kLim && p->n_items >= 0 && p->n_split >= 0, KGX_ERR_ARG,
              "kgx_softmax_aggr: bad sizes");
  KGX_TRY(check_shape(fn, p->F, p->x, p->edge, p->n_e, p->temp, p->message, p->eps));
  const bool edge = p->edge && p->n_e > 0;  // no row to read: every slot is without a feature
  const int64_t stats_w = (p->stats_q ? 3 : 2) * p->F;
  KGX_TRY(check_table(fn, "x", p->x, p->ld_x, p->F, false));
  KGX_TRY(check_table(fn, "edge", edge ? p->edge : nullptr, p->ld_e, p->F, false));
  KGX_TRY(check_table(fn, "temp", p->temp, p->F, p->F, true));
  KGX_TRY(check_table(fn, "out", p->out, p->ld_out, p->F, true));
  KGX_TRY(check_table(fn, "stats", p->stats, p->ld_stats, stats_w, false));
  KGX_TRY(check_table(fn, "partials", p->partials, 4 * p->F, 4 * p->F, false));
  if (p->n_rows == 0) return KGX_OK;
  KGX_REQUIRE(p->rowptr && p->rows && (p->col || !p->x), KGX_ERR_ARG, "kgx_softmax_aggr: null rowptr / rows / col");
  KGX_REQUIRE(!p->items || p->n_split == 0 || (p->split && p->partials), KGX_ERR_ARG,
              "kgx_softmax_aggr: split rows need split list and partials");
  FwdArgs a{};
  a.sched = make_sched(p->rowptr, p->rows, p->n_rows, p->items, p->n_items, p->split, p->n_split);
  a.col = p->col, a.e_idx = p->e_idx;
  a.msg = {p->x, p->ld_x, edge ? p->edge : nullptr, p->ld_e, int32_t(edge ? p->n_e : 0), p->temp, p->message, p->eps};
  a.F = int(p->F), a.lgG = lg_group(p->F);
  a.out = p->out, a.ld_o = p->ld_out;
  a.stats = p->stats, a.ld_s = p->ld_stats, a.stats_q = p->stats_q != 0;
  a.partials = p->partials;
  hipStream_t stream = as_stream(stream_);
  return pieces_of(p->F) == 2 ? launch_fwd<2>(a, p->x, edge, stream) : launch_fwd<1>(a, p->x, edge, stream);
}

extern "C" int kgx_softmax_aggr_backward_workspace_bytes(int64_t n_rows, int64_t t_n_slots, int64_t F, size_t* bytes) {
  KGX_REQUIRE(bytes && n_rows >= 0 && t_n_slots >= 0 && F >= 1 && F <= 512, KGX_ERR_ARG,
              "kgx_softmax_aggr_backward_workspace_bytes: n_rows %lld, t_n_slots %lld, F %lld", (long long)n_rows,
              (long long)t_n_slots, (long long)F);
  *bytes = carve_bwd(nullptr, 0, n_rows, t_n_slots, F).bytes;
  return KGX_OK;
}

extern "C" int kgx_softmax_aggr_backward(const kgx_softmax_aggr_backward_args* p, kgx_stream_t stream_) {
  const char* fn = "kgx_softmax_aggr_backward";
  KGX_REQUIRE(p && p->struct_size == sizeof(kgx_softmax_aggr_backward_args), KGX_ERR_ARG,
              "kgx_softmax_aggr_backward: struct_size %llu is not this header's %zu",
              p ? (unsigned long long)p->struct_size : 0ull, sizeof(kgx_softmax_aggr_backward_args));
  KGX_REQUIRE(p->n_rows >= 0 && p->n_rows < kLim && p->n_src >= 0 && p->n_src < kLim && p->n_items >= 0 &&
                  p->n_split >= 0 && p->t_n_items >= 0 && p->t_n_split >= 0 && p->t_n_slots >= 0,
              KGX_ERR_ARG, "kgx_softmax_aggr_backward: bad sizes");
  KGX_TRY(check_shape(fn, p->F, p->x, p->edge, p->n_e, p->temp, p->message, p->eps));
  const bool edge = p->edge && p->n_e > 0;  // no row to read or write
  KGX_REQUIRE(!edge || p->grad_edge, KGX_ERR_ARG, "kgx_softmax_aggr_backward: an edge table needs grad_edge");
  KGX_REQUIRE(!(edge && p->x) || p->t_e_idx, KGX_ERR_ARG,
              "kgx_softmax_aggr_backward: an edge table next to x needs t_e_idx");
  KGX_REQUIRE(!p->x || p->grad_x, KGX_ERR_ARG, "kgx_softmax_aggr_backward: x needs grad_x");
  KGX_TRY(check_table(fn, "x", p->x, p->ld_x, p->F, false));
  KGX_TRY(check_table(fn, "edge", edge ? p->edge : nullptr, p->ld_e, p->F, false));
  KGX_TRY(check_table(fn, "temp", p->temp, p->F, p->F, true));
  KGX_TRY(check_table(fn, "out", p->out, p->ld_out, p->F, true));
  KGX_TRY(check_table(fn, "stats", p->stats, p->ld_stats, 2 * p->F, true));
  KGX_TRY(check_table(fn, "grad_out", p->grad_out, p->ld_grad, p->F, true));
  KGX_TRY(check_table(fn, "grad_x", p->x ? p->grad_x : nullptr, p->ld_gx, p->F, false));
  KGX_TRY(check_table(fn, "grad_edge", edge ? p->grad_edge : nullptr, p->ld_ge, p->F, false));
  if (p->n_rows == 0) return KGX_OK;  // no destination: no slot, and the caller's gradients stay as they are
  KGX_REQUIRE(p->rowptr && p->rows, KGX_ERR_ARG, "kgx_softmax_aggr_backward: null rowptr / rows");
  const int64_t t_n_slots = p->t_items ? p->t_n_slots : 0;
  const BwdCarve ws = carve_bwd(p->workspace, size_t(p->workspace_bytes), p->n_rows, t_n_slots, p->F);
  KGX_REQUIRE(p->workspace && p->workspace_bytes >= ws.bytes, KGX_ERR_ARG,
              "kgx_softmax_aggr_backward: workspace of %llu bytes, %zu needed", (unsigned long long)p->workspace_bytes,
              ws.bytes);
  KGX_TRY(check_table(fn, "workspace", p->workspace, p->F, p->F, true));
  hipStream_t stream = as_stream(stream_);
  const bool two = pieces_of(p->F) == 2;
  BwdArgs d{};
  d.msg = {p->x, p->ld_x, edge ? p->edge : nullptr, p->ld_e, int32_t(edge ? p->n_e : 0), p->temp, p->message, p->eps};
  d.F = int(p->F), d.lgG = lg_group(p->F);
  BwdArgs t = d;
  if (edge) {
    KGX_REQUIRE(p->col || !p->x, KGX_ERR_ARG, "kgx_softmax_aggr_backward: null col");
    d.sched = make_sched(p->rowptr, p->rows, p->n_rows, p->items, p->n_items, p->split, p->n_split);
    d.idx = p->col, d.e_idx = p->e_idx;
    d.grad = p->grad_out, d.ld_g = p->ld_grad, d.out = p->out, d.ld_o = p->ld_out;
    d.stats = p->stats, d.ld_s = p->ld_stats;
    d.grad_edge = p->grad_edge, d.ld_ge = p->ld_ge;
    KGX_TRY(two ? launch_dst<2>(d, p->x, stream) : launch_dst<1>(d, p->x, stream));
  }
  if (p->x && p->n_src > 0) {
    KGX_REQUIRE(p->t_rowptr && p->t_rows && p->t_col, KGX_ERR_ARG,
                "kgx_softmax_aggr_backward: null t_rowptr / t_rows / t_col");
    const PackArgs pk{p->grad_out, p->out, p->stats, p->temp, p->ld_grad, p->ld_out, p->ld_stats,
                      p->n_rows,   int(p->F), ws.packed};
    KGX_TRY(two ? launch_pack<2>(pk, d.lgG, stream) : launch_pack<1>(pk, d.lgG, stream));
    t.sched = make_sched(p->t_rowptr, p->t_rows, p->n_src, p->t_items, p->t_n_items, p->t_split, p->t_n_split);
    t.idx = p->t_col, t.e_idx = p->t_e_idx;
    t.packed = ws.packed, t.partials = ws.t_partials;
    t.grad_x = p->grad_x, t.ld_gx = p->ld_gx;
    KGX_TRY(two ? launch_src<2>(t, edge, stream) : launch_src<1>(t, edge, stream));
  }
  return KGX_OK;
}
