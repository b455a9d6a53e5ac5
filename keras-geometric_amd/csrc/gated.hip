// Fused per-channel edge gate for the kgx engine (gfx950, wave64): the aggregation of
// the residual gated graph convolution (PyG's ResGatedGraphConv after its linear maps),
//   z_t = (k[i] + q[j]) + edge[e_t]      s_t = 1 / (1 + expf(-z_t))      (every channel its own gate)
//   out[i] = (sum_{t into i} s_t * v[j] + root[i]) + bias
// and its backward.  No [E, F] tensor exists in either direction: the backward
// recomputes s from k, q and edge in both of its passes.
//
// Row-owned lanes over the hub-split schedule (the walk of kgx_attn.h), not GINE's
// slot-parallel spans: the gate needs the destination's k row next to every gathered
// row, which a lane group that owns the row keeps in registers for all of its slots
// (the backward keeps two rows, k and grad_out, or q and v); a span of 64 slots would
// gather that row again per slot, a third (forward) or two more (backward) row reads
// per edge in a kernel that is bound by exactly those reads.  Nothing here crosses
// lanes (the gate is per channel), so there is no LDS tile and no reduction.
//
// Lane layout: a group of G = 2^lgG lanes owns a work item; lane l holds NP float4
// pieces of the row, piece p at columns 4 (l + p G): a group's piece is one contiguous
// run of the row.  NP = 1 up to F = 256 (G = next_pow2(F / 4) <= 64), NP = 2 above
// (G = 64).  A piece past F loads column 0 (a valid address) and stores nothing.
// U slots' rows (2 or 3 gathered rows each) are in flight per lane group, as the U-edge
// blocks of gat.hip; slots past the item's end re-read its last slot and are dropped.
//
// z is formed by exactly the two rounded adds above, in that order, in all three
// kernels (the file is compiled with -ffp-contract=off), and the products of dz in one
// order, so both backward passes see the forward's gate.  expf(-z) saturates to 0 and to
// +inf, where the correctly rounded divide gives exactly 1 and exactly 0.
//
// Hub chunks store [F] partials (the source pass [2F]: d q | d v) that a fix-up adds in
// chunk order; rows are sequential fp32 sums in CSR order.  One writer per element, no
// atomics: the same bits from run to run.
#include "kgx_attn.h"
#include "kgx_red.h"

namespace kgx {
namespace {

using Sum = RowRed<KGX_SUM>;  // sequential round-to-nearest adds

template <int NP>
constexpr int unroll() {
  return NP == 1 ? 4 : 2;
}

// This thread's pieces of a row.
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
      c[p] = ok[p] ? col : 0;
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
__device__ __forceinline__ void zero_row(float (&d)[NP][4]) {
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int i = 0; i < 4; ++i) d[p][i] = Sum::init();
}

// The gate of one channel: the two rounded adds, then the logistic function.
__device__ __forceinline__ float gate(float k, float q, float e, bool edge) {
  float z = k + q;
  if (edge) z = z + e;
  return __fdiv_rn(1.0f, 1.0f + expf(-z));
}
// d loss / d z of one channel: s = 1 and s = 0 give exactly 0
__device__ __forceinline__ float dz_of(float g, float v, float s) { return (g * v) * (s * (1.0f - s)); }

// The edge table of all three kernels.  p null: no edge term.
struct EdgeTab {
  const float* p;
  int64_t ld;
  int32_t n_e;
  // the row of slot t under index array idx, clamped to a row that exists; has: it is the slot's own
  __device__ __forceinline__ int32_t row(const int32_t* idx, int32_t t, bool& has) const {
    int32_t r;
    has = edge_row(idx, n_e, t, r);
    return has ? r : 0;
  }
};

struct GatedFwdArgs {
  Sched sched;
  const int32_t* col;
  const int32_t* e_idx;
  const float *k, *q, *v;
  int64_t ld_k, ld_q, ld_v;
  EdgeTab edge;
  const float* root;
  int64_t ld_r;
  const float* bias;
  int F, lgG;
  float* out;
  int64_t ld_o;
  float* partials;  // [n_slots, F]
};

// (acc + root[row]) + bias into out[row]
template <int NP>
__device__ __forceinline__ void finish_row(const GatedFwdArgs& a, const RowLanes<NP>& L, int32_t row,
                                           float (&acc)[NP][4]) {
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    if (!L.ok[p]) continue;
    if (a.root) {
      float r[4];
      vload<4>(r, a.root + int64_t(row) * a.ld_r + L.c[p]);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[p][i] = acc[p][i] + r[i];
    }
    if (a.bias) {
      float b[4];
      vload<4>(b, a.bias + L.c[p]);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[p][i] = acc[p][i] + b[i];
    }
    vstore<4>(a.out + int64_t(row) * a.ld_o + L.c[p], acc[p]);
  }
}

template <int NP, bool kEdge>
__global__ __launch_bounds__(kBlock) void gated_kernel(GatedFwdArgs a) {
  constexpr int U = unroll<NP>();
  const RowLanes<NP> L(a.lgG, a.F);
  const int64_t ngroups = group_count(a.lgG);
  const int64_t n_work = a.sched.n_work();
  for (int64_t it = first_group(a.lgG); it < n_work; it += ngroups) {
    int32_t row, beg, end, slot;
    work_item(a.sched, it, row, beg, end, slot);
    float k[NP][4], acc[NP][4];
    load_row<NP>(k, a.k + int64_t(row) * a.ld_k, L);
    zero_row<NP>(acc);
    for (int32_t e = beg; e < end; e += U) {
      int32_t c[U], r[U];
      bool has[U];
      float q[U][NP][4], v[U][NP][4], ev[U][NP][4];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t ee = e + u < end ? e + u : end - 1;  // slots past the end re-read the last one
        c[u] = a.col[ee];
        has[u] = false;
        r[u] = kEdge ? a.edge.row(a.e_idx, ee, has[u]) : 0;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        load_row<NP>(q[u], a.q + row_off(c[u], a.ld_q), L);
        load_row<NP>(v[u], a.v + row_off(c[u], a.ld_v), L);
        if constexpr (kEdge) load_row<NP>(ev[u], a.edge.p + row_off(r[u], a.edge.ld), L);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (e + u < end) {
#pragma unroll
          for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const float s = gate(k[p][i], q[u][p][i], (kEdge && has[u]) ? ev[u][p][i] : 0.0f, kEdge);
              acc[p][i] = Sum::combine(acc[p][i], s * v[u][p][i]);
            }
        }
      }
    }
    if (slot >= 0) store_row<NP>(a.partials + int64_t(slot) * a.F, acc, L);
    else finish_row<NP>(a, L, row, acc);
  }
}

// The chunk partials of lane group `it`'s split row, added in chunk order, B loads in flight.
template <int NP, int B>
__device__ __forceinline__ void sum_chunks(const float* __restrict__ partials, int64_t ld_p, int32_t slot0,
                                           int32_t nc, const RowLanes<NP>& L, float (&acc)[NP][4]) {
  zero_row<NP>(acc);
  for (int32_t c0 = 0; c0 < nc; c0 += B) {
    float pv[B][NP][4];
#pragma unroll
    for (int u = 0; u < B; ++u)
      load_row<NP>(pv[u], partials + int64_t(slot0 + (c0 + u < nc ? c0 + u : nc - 1)) * ld_p, L);
#pragma unroll
    for (int u = 0; u < B; ++u) {
      if (c0 + u < nc) {
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[p][i] = Sum::combine(acc[p][i], pv[u][p][i]);
      }
    }
  }
}

template <int NP>
__global__ __launch_bounds__(kBlock) void gated_fixup_kernel(GatedFwdArgs a) {
  const RowLanes<NP> L(a.lgG, a.F);
  const int64_t ngroups = group_count(a.lgG);
  for (int64_t it = first_group(a.lgG); it < a.sched.n_split; it += ngroups) {
    const int4 sp = a.sched.split[it];
    float acc[NP][4];
    sum_chunks<NP, 8 / NP>(a.partials, a.F, sp.y, sp.z, L, acc);
    finish_row<NP>(a, L, sp.x, acc);
  }
}

// ===========================================================================
// Backward.  One kernel serves both passes; a work item's lanes keep two rows of
// the item's own node and gather two rows of the node at the slot's other end:
//   destination pass (kSrc false): own k[i], G[i]; gathered q[j], v[j]
//       acc0 = sum dz -> grad_k[i]          grad_edge[e_t] = dz_t
//   source pass (kSrc true, transposed CSR): own q[j], v[j]; gathered k[i], G[i]
//       acc0 = sum dz -> grad_q[j]          acc1 = sum s * G[i] -> grad_v[j]
// ===========================================================================
struct GatedBwdArgs {
  Sched sched;
  const int32_t* idx;    // per slot: the node at its other end
  const int32_t* e_idx;  // per slot: its edge row (null: the slot itself)
  const float *own0, *own1, *oth0, *oth1;
  int64_t ld_own0, ld_own1, ld_oth0, ld_oth1;
  EdgeTab edge;
  int F, lgG;
  float* partials;  // [slots, ld_p]: [F] (destination pass) or [F d q | F d v]
  int64_t ld_p;
  float *out0, *out1, *grad_edge;
  int64_t ld_o0, ld_o1, ld_ge;
};

template <int NP, bool kEdge, bool kSrc>
__global__ __launch_bounds__(kBlock) void gated_bwd_kernel(GatedBwdArgs a) {
  constexpr int U = unroll<NP>();
  const RowLanes<NP> L(a.lgG, a.F);
  const int64_t ngroups = group_count(a.lgG);
  const int64_t n_work = a.sched.n_work();
  for (int64_t it = first_group(a.lgG); it < n_work; it += ngroups) {
    int32_t row, beg, end, slot;
    work_item(a.sched, it, row, beg, end, slot);
    float o0[NP][4], o1[NP][4], acc0[NP][4], acc1[NP][4];
    load_row<NP>(o0, a.own0 + int64_t(row) * a.ld_own0, L);
    load_row<NP>(o1, a.own1 + int64_t(row) * a.ld_own1, L);
    zero_row<NP>(acc0);
    zero_row<NP>(acc1);
    for (int32_t e = beg; e < end; e += U) {
      int32_t c[U], r[U];
      bool has[U];
      float g0[U][NP][4], g1[U][NP][4], ev[U][NP][4];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t ee = e + u < end ? e + u : end - 1;
        c[u] = a.idx[ee];
        has[u] = false;
        r[u] = kEdge ? a.edge.row(a.e_idx, ee, has[u]) : 0;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        load_row<NP>(g0[u], a.oth0 + row_off(c[u], a.ld_oth0), L);
        load_row<NP>(g1[u], a.oth1 + row_off(c[u], a.ld_oth1), L);
        if constexpr (kEdge) load_row<NP>(ev[u], a.edge.p + row_off(r[u], a.edge.ld), L);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (e + u < end) {
          float dz[NP][4];
#pragma unroll
          for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const float ee = (kEdge && has[u]) ? ev[u][p][i] : 0.0f;
              // k + q in the forward's operand order: own0 is k in the destination pass, q in the source pass
              const float s = kSrc ? gate(g0[u][p][i], o0[p][i], ee, kEdge) : gate(o0[p][i], g0[u][p][i], ee, kEdge);
              const float G = kSrc ? g1[u][p][i] : o1[p][i], v = kSrc ? o1[p][i] : g1[u][p][i];
              dz[p][i] = dz_of(G, v, s);
              acc0[p][i] = Sum::combine(acc0[p][i], dz[p][i]);
              if constexpr (kSrc) acc1[p][i] = Sum::combine(acc1[p][i], s * G);
            }
          if constexpr (kEdge && !kSrc) {
            if (has[u]) store_row<NP>(a.grad_edge + row_off(r[u], a.ld_ge), dz, L);
          }
        }
      }
    }
    if (slot >= 0) {
      float* p = a.partials + int64_t(slot) * a.ld_p;
      store_row<NP>(p, acc0, L);
      if constexpr (kSrc) store_row<NP>(p + a.F, acc1, L);
    } else {
      store_row<NP>(a.out0 + int64_t(row) * a.ld_o0, acc0, L);
      if constexpr (kSrc) store_row<NP>(a.out1 + int64_t(row) * a.ld_o1, acc1, L);
    }
  }
}

constexpr int64_t kLim = int64_t(1) << 31;

// Pieces per lane and lanes per group of an F-wide row.
inline int pieces_of(int64_t F) { return F > 256 ? 2 : 1; }
inline int lg_group(int64_t F) { return log2i(next_pow2(int((F / 4 + pieces_of(F) - 1) / pieces_of(F)))); }

template <int NP>
int launch_fwd(const GatedFwdArgs& a, hipStream_t s) {
  const int G = 1 << a.lgG;
  const int rc = a.edge.p ? launch_resident(gated_kernel<NP, true>, a.sched.n_work(), G, a, s)
                          : launch_resident(gated_kernel<NP, false>, a.sched.n_work(), G, a, s);
  if (rc) return rc;
  return launch_resident(gated_fixup_kernel<NP>, a.sched.n_split, G, a, s);
}

template <int NP, bool kSrc>
int launch_bwd(const GatedBwdArgs& a, hipStream_t s) {
  const int G = 1 << a.lgG;
  const int rc = a.edge.p ? launch_resident(gated_bwd_kernel<NP, true, kSrc>, a.sched.n_work(), G, a, s)
                          : launch_resident(gated_bwd_kernel<NP, false, kSrc>, a.sched.n_work(), G, a, s);
  if (rc) return rc;
  // the shared in-order chunk sum: columns [0, F) of a slot into out0, [F, 2F) into out1
  return launch_chunk_sum(a.sched, a.partials, a.ld_p, a.F, int(a.ld_p), a.out0, a.ld_o0, kSrc ? a.out1 : a.out0,
                          kSrc ? a.ld_o1 : a.ld_o0, s);
}

struct BwdCarve {
  float *d_partials, *t_partials;
  size_t bytes;
};
inline BwdCarve carve_bwd(void* ws, size_t cap, int64_t n_slots, int64_t t_n_slots, int64_t F) {
  Carve c(ws, cap);
  BwdCarve b;
  b.d_partials = c.take<float>(size_t(n_slots) * size_t(F));
  b.t_partials = c.take<float>(size_t(t_n_slots) * 2 * size_t(F));
  b.bytes = c.used();
  return b;
}

// A table read four floats at a time: present, wide enough, below 2^31, aligned.
int check_table(const char* fn, const char* what, const void* p, int64_t ld, int64_t F, bool required) {
  KGX_REQUIRE(p || !required, KGX_ERR_ARG, "%s: %s is null", fn, what);
  if (!p) return KGX_OK;
  KGX_REQUIRE(ld >= F && ld < kLim, KGX_ERR_ARG, "%s: leading dimension of %s (%lld) below F = %lld or >= 2^31", fn,
              what, (long long)ld, (long long)F);
  KGX_REQUIRE(attn_vec_ok(16, {p}, {ld}), KGX_ERR_UNSUPPORTED,
              "%s: %s is read four floats at a time: a 16-byte aligned address and a leading dimension that is a "
              "multiple of 4 (got ld %lld)", fn, what, (long long)ld);
  return KGX_OK;
}

int check_shape(const char* fn, int64_t F, const float* edge, int64_t n_e) {
  KGX_REQUIRE(F >= 1, KGX_ERR_ARG, "%s: F = %lld", fn, (long long)F);
  KGX_REQUIRE(!edge || (n_e >= 0 && n_e < kLim), KGX_ERR_ARG, "%s: edge table rows n_e = %lld outside [0, 2^31)", fn,
              (long long)n_e);
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

extern "C" int kgx_gated(const kgx_gated_args* p, kgx_stream_t stream_) {
  const char* fn = "kgx_gated";
  KGX_REQUIRE(p && p->struct_size == sizeof(kgx_gated_args), KGX_ERR_ARG,
              "kgx_gated: struct_size %llu is not this header's %zu", p ? (unsigned long long)p->struct_size : 0ull,
              sizeof(kgx_gated_args));
  KGX_REQUIRE(p->n_rows >= 0 && p->n_rows < kLim && p->n_items >= 0 && p->n_split >= 0, KGX_ERR_ARG,
              "kgx_gated: bad sizes");
  KGX_TRY(check_shape(fn, p->F, p->edge, p->n_e));
  if (p->n_rows == 0) return KGX_OK;
  KGX_REQUIRE(p->rowptr && p->rows && p->col, KGX_ERR_ARG, "kgx_gated: null rowptr / rows / col");
  KGX_REQUIRE(!p->items || p->n_split == 0 || (p->split && p->partials), KGX_ERR_ARG,
              "kgx_gated: split rows need split list and partials");
  const bool edge = p->edge && p->n_e > 0;  // no row to read: every slot is without a feature
  KGX_TRY(check_table(fn, "k", p->k, p->ld_k, p->F, true));
  KGX_TRY(check_table(fn, "q", p->q, p->ld_q, p->F, true));
  KGX_TRY(check_table(fn, "v", p->v, p->ld_v, p->F, true));
  KGX_TRY(check_table(fn, "out", p->out, p->ld_out, p->F, true));
  KGX_TRY(check_table(fn, "edge", edge ? p->edge : nullptr, p->ld_e, p->F, false));
  KGX_TRY(check_table(fn, "root", p->root, p->ld_root, p->F, false));
  KGX_TRY(check_table(fn, "bias", p->bias, p->F, p->F, false));
  KGX_TRY(check_table(fn, "partials", p->partials, p->F, p->F, false));
  GatedFwdArgs a{};
  a.sched = make_sched(p->rowptr, p->rows, p->n_rows, p->items, p->n_items, p->split, p->n_split);
  a.col = p->col;
  a.e_idx = p->e_idx;
  a.k = p->k, a.q = p->q, a.v = p->v;
  a.ld_k = p->ld_k, a.ld_q = p->ld_q, a.ld_v = p->ld_v;
  a.edge = {edge ? p->edge : nullptr, p->ld_e, int32_t(edge ? p->n_e : 0)};
  a.root = p->root, a.ld_r = p->ld_root, a.bias = p->bias;
  a.F = int(p->F), a.lgG = lg_group(p->F);
  a.out = p->out, a.ld_o = p->ld_out, a.partials = p->partials;
  hipStream_t stream = as_stream(stream_);
  return pieces_of(p->F) == 2 ? launch_fwd<2>(a, stream) : launch_fwd<1>(a, stream);
}

extern "C" int kgx_gated_backward_workspace_bytes(int64_t n_slots, int64_t t_n_slots, int64_t F, size_t* bytes) {
  KGX_REQUIRE(bytes && n_slots >= 0 && t_n_slots >= 0 && F >= 1 && F <= 512, KGX_ERR_ARG,
              "kgx_gated_backward_workspace_bytes: n_slots %lld, t_n_slots %lld, F %lld", (long long)n_slots,
              (long long)t_n_slots, (long long)F);
  *bytes = carve_bwd(nullptr, 0, n_slots, t_n_slots, F).bytes;
  return KGX_OK;
}

extern "C" int kgx_gated_backward(const kgx_gated_backward_args* p, kgx_stream_t stream_) {
  const char* fn = "kgx_gated_backward";
  KGX_REQUIRE(p && p->struct_size == sizeof(kgx_gated_backward_args), KGX_ERR_ARG,
              "kgx_gated_backward: struct_size %llu is not this header's %zu",
              p ? (unsigned long long)p->struct_size : 0ull, sizeof(kgx_gated_backward_args));
  KGX_REQUIRE(p->n_rows >= 0 && p->n_rows < kLim && p->n_src >= 0 && p->n_src < kLim && p->n_items >= 0 &&
                  p->n_split >= 0 && p->t_n_items >= 0 && p->t_n_split >= 0 && p->n_slots >= 0 && p->t_n_slots >= 0,
              KGX_ERR_ARG, "kgx_gated_backward: bad sizes");
  KGX_TRY(check_shape(fn, p->F, p->edge, p->n_e));
  KGX_REQUIRE(!p->edge || (p->grad_edge && p->t_e_idx), KGX_ERR_ARG,
              "kgx_gated_backward: an edge table needs grad_edge and t_e_idx");
  if (p->n_rows == 0 && p->n_src == 0) return KGX_OK;
  KGX_REQUIRE(p->rowptr && p->rows && p->t_rowptr && p->t_rows, KGX_ERR_ARG,
              "kgx_gated_backward: null rowptr / rows / t_rowptr / t_rows");
  const bool edge = p->edge && p->n_e > 0;  // no row to read or write
  KGX_TRY(check_table(fn, "k", p->k, p->ld_k, p->F, true));
  KGX_TRY(check_table(fn, "q", p->q, p->ld_q, p->F, true));
  KGX_TRY(check_table(fn, "v", p->v, p->ld_v, p->F, true));
  KGX_TRY(check_table(fn, "grad_out", p->grad_out, p->ld_grad, p->F, true));
  KGX_TRY(check_table(fn, "grad_k", p->grad_k, p->ld_gk, p->F, true));
  KGX_TRY(check_table(fn, "grad_q", p->grad_q, p->ld_gq, p->F, true));
  KGX_TRY(check_table(fn, "grad_v", p->grad_v, p->ld_gv, p->F, true));
  KGX_TRY(check_table(fn, "edge", edge ? p->edge : nullptr, p->ld_e, p->F, false));
  KGX_TRY(check_table(fn, "grad_edge", edge ? p->grad_edge : nullptr, p->ld_ge, p->F, false));
  const int64_t n_slots = p->items ? p->n_slots : 0, t_n_slots = p->t_items ? p->t_n_slots : 0;
  const BwdCarve ws = carve_bwd(p->workspace, size_t(p->workspace_bytes), n_slots, t_n_slots, p->F);
  KGX_REQUIRE(p->workspace && p->workspace_bytes >= ws.bytes, KGX_ERR_ARG,
              "kgx_gated_backward: workspace of %llu bytes, %zu needed", (unsigned long long)p->workspace_bytes,
              ws.bytes);
  KGX_TRY(check_table(fn, "workspace", p->workspace, p->F, p->F, true));
  hipStream_t stream = as_stream(stream_);
  GatedBwdArgs d{};
  d.edge = {edge ? p->edge : nullptr, p->ld_e, int32_t(edge ? p->n_e : 0)};
  d.F = int(p->F), d.lgG = lg_group(p->F);
  GatedBwdArgs t = d;
  const bool two = pieces_of(p->F) == 2;
  if (p->n_rows > 0) {
    KGX_REQUIRE(p->col, KGX_ERR_ARG, "kgx_gated_backward: null col");
    d.sched = make_sched(p->rowptr, p->rows, p->n_rows, p->items, p->n_items, p->split, p->n_split);
    d.idx = p->col, d.e_idx = p->e_idx;
    d.own0 = p->k, d.ld_own0 = p->ld_k, d.own1 = p->grad_out, d.ld_own1 = p->ld_grad;
    d.oth0 = p->q, d.ld_oth0 = p->ld_q, d.oth1 = p->v, d.ld_oth1 = p->ld_v;
    d.partials = ws.d_partials, d.ld_p = p->F;
    d.out0 = p->grad_k, d.ld_o0 = p->ld_gk, d.grad_edge = p->grad_edge, d.ld_ge = p->ld_ge;
    KGX_TRY(two ? (launch_bwd<2, false>(d, stream)) : (launch_bwd<1, false>(d, stream)));
  }
  if (p->n_src > 0) {
    KGX_REQUIRE(p->t_col, KGX_ERR_ARG, "kgx_gated_backward: null t_col");
    t.sched = make_sched(p->t_rowptr, p->t_rows, p->n_src, p->t_items, p->t_n_items, p->t_split, p->t_n_split);
    t.idx = p->t_col, t.e_idx = p->t_e_idx;
    t.own0 = p->q, t.ld_own0 = p->ld_q, t.own1 = p->v, t.ld_own1 = p->ld_v;
    t.oth0 = p->k, t.ld_oth0 = p->ld_k, t.oth1 = p->grad_out, t.ld_oth1 = p->ld_grad;
    t.partials = ws.t_partials, t.ld_p = 2 * p->F;
    t.out0 = p->grad_q, t.ld_o0 = p->ld_gq, t.out1 = p->grad_v, t.ld_o1 = p->ld_gv;
    KGX_TRY(two ? (launch_bwd<2, true>(t, stream)) : (launch_bwd<1, true>(t, stream)));
  }
  return KGX_OK;
}
