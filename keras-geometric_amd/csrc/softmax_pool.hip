// Fused segment softmax + weighted sum for the attention readouts (gfx950, wave64).
//
//   out[g,:] = sum_{i in g} softmax_g(s)_i * x[i,:]
//
// Reference (src/keras_geometric/layers/pooling/attention_pooling.py): both
// AttentionPooling (:409-412) and every Set2Set processing step (:175-180,
// :206-211) run ops.softmax(scores, axis=0) and ops.sum(weights * inputs,
// axis=0): a max pass, an exp/sum pass and an [N,F] product that is summed
// again.  Here one group of G lanes owns a segment (or one chunk of a large
// one), lane l holds R vectors of V consecutive features, each row of x is
// read ONCE and the softmax is computed online (running max m, running sum l,
// rescaled accumulator), U rows per rescale, as gatv2.hip does per edge.
// Set2Set's score tanh(x_i . u + c_g) is computed from the row already in
// registers (one cross-lane dot product), so a processing step is one pass
// over x instead of two.
//
// Numerics: algebraically the reference's softmax / sum; the summation order,
// exp and the place of the division differ at the ulp level, so the result is
// tolerance-checked (|a-b| <= 1e-5*max(1,|b|)).  Numerator and denominator
// are accumulated in fp64 (a single-graph segment sums 10^7 terms); the kernel
// is bound by the read of x.  No atomics: chunk partials [acc | m | l] are
// merged in chunk order by a fix-up, so results are the same bits every run.
// There is no epsilon in the denominator (the reference's softmax has none):
// an empty segment is a zero row, an all -inf segment is NaN, as torch.softmax.
#include "kgx_attn.h"

namespace kgx {
namespace {

constexpr int kPoolMaxF = KGX_POOL_MAX_F;

struct PoolArgs {
  Sched sched;
  const int32_t* idx;  // node per segment slot, or null: identity
  const float* x;
  int64_t ld_x;
  int F;
  const float* s;  // given scores [N], or null:
  const float* u;  //   s_i = act(x_i . u + c[g]), stored to s_out
  const float* c;
  int tanh_act;
  float* s_out;
  float* out;
  int64_t ld_o;
  float* stats;     // optional [n_seg, 2]: max, denominator
  float* partials;  // per slot: [F acc | m | l]
  int G, lgG;
};

// The shift of the online softmax: the running max, or 0 while it is still
// -inf (nothing but -inf scores seen: every weight so far is exp(-inf) = 0,
// not exp(-inf - -inf) = NaN).  A +inf max stays: exp(inf - inf) = NaN is the
// reference's result for a segment holding +inf.
__device__ __forceinline__ float shift_of(float m) { return m == -__builtin_inff() ? 0.0f : m; }

template <int V, int R>
struct Lanes {
  int off[R];  // feature offset of vector r (0 where the vector is padding)
  bool ok[R];
  __device__ __forceinline__ Lanes(int lane, int G, int F) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int f = (r * G + lane) * V;
      ok[r] = f < F;  // V == 4 only with F % 4 == 0: a vector is whole or padding
      off[r] = ok[r] ? f : 0;
    }
  }
  // unconditional loads from clamped offsets (padding lanes re-read column 0), masked to 0
  __device__ __forceinline__ void load(float (&d)[V * R], const float* __restrict__ row) const {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float t[V];
      vload<V>(t, row + off[r]);
#pragma unroll
      for (int k = 0; k < V; ++k) d[r * V + k] = ok[r] ? t[k] : 0.0f;
    }
  }
  __device__ __forceinline__ void store(float* __restrict__ row, const float (&d)[V * R]) const {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (!ok[r]) continue;
      float t[V];
#pragma unroll
      for (int k = 0; k < V; ++k) t[k] = d[r * V + k];
      vstore<V>(row + off[r], t);
    }
  }
};

template <int V, int R>
__global__ __launch_bounds__(kBlock) void softmax_pool_kernel(PoolArgs a) {
  constexpr int U = 4;  // rows per online-softmax block
  constexpr int W = V * R;
  const int G = a.G;
  const int lane = threadIdx.x & (G - 1);
  const Lanes<V, R> L(lane, G, a.F);
  const int64_t ngroups = group_count(a.lgG);
  const int64_t n_work = a.sched.n_work();

  float su[W];
#pragma unroll
  for (int k = 0; k < W; ++k) su[k] = 0.0f;
  if (a.u) L.load(su, a.u);

  for (int64_t it = first_group(a.lgG); it < n_work; it += ngroups) {
    int32_t row, beg, end, slot;
    work_item(a.sched, it, row, beg, end, slot);
    const float cg = a.u ? a.c[row] : 0.0f;
    double acc[W];
#pragma unroll
    for (int k = 0; k < W; ++k) acc[k] = 0.0;
    float m = -__builtin_inff();
    double l = 0.0;

    for (int32_t e = beg; e < end; e += U) {
      const int n = (end - e) < U ? (end - e) : U;
      int32_t node[U];
#pragma unroll
      for (int j = 0; j < U; ++j) {
        const int32_t ee = j < n ? e + j : end - 1;  // rows past the end re-read the last one
        node[j] = a.idx ? a.idx[ee] : ee;
      }
      float xs[U][W];
#pragma unroll
      for (int j = 0; j < U; ++j) L.load(xs[j], a.x + row_off(node[j], a.ld_x));
      float sc[U];
      if (a.u) {
#pragma unroll
        for (int j = 0; j < U; ++j) {
          float p = 0.0f;
#pragma unroll
          for (int k = 0; k < W; ++k) p += xs[j][k] * su[k];
          const float z = group_reduce(p, G) + cg;
          sc[j] = a.tanh_act ? tanhf(z) : z;
          if (lane == 0 && j < n) a.s_out[node[j]] = sc[j];
        }
      } else {
#pragma unroll
        for (int j = 0; j < U; ++j) sc[j] = a.s[node[j]];
      }
      float mc = -__builtin_inff();
#pragma unroll
      for (int j = 0; j < U; ++j)
        if (j < n) mc = fmaxf(mc, sc[j]);  // a NaN score is skipped here and poisons l below
      const float m_new = fmaxf(m, mc);
      const float ref = shift_of(m_new);
      const double scale = double(expf(m - ref));
      l *= scale;
#pragma unroll
      for (int k = 0; k < W; ++k) acc[k] *= scale;
#pragma unroll
      for (int j = 0; j < U; ++j) {
        if (j < n) {
          const double p = double(expf(sc[j] - ref));
          l += p;
#pragma unroll
          for (int k = 0; k < W; ++k) acc[k] = fma(p, double(xs[j][k]), acc[k]);
        }
      }
      m = m_new;
    }

    if (slot >= 0) {
      float* p = a.partials + int64_t(slot) * (a.F + 2);
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int k = 0; k < V; ++k)
          if (L.ok[r]) p[L.off[r] + k] = float(acc[r * V + k]);
      if (lane == 0) {
        p[a.F] = m;
        p[a.F + 1] = float(l);
      }
    } else {
      if (a.stats && lane == 0) {
        a.stats[int64_t(row) * 2] = m;
        a.stats[int64_t(row) * 2 + 1] = float(l);
      }
      float r[W];
#pragma unroll
      for (int k = 0; k < W; ++k) r[k] = end > beg ? float(acc[k] / l) : 0.0f;  // no rows: the empty sum
      L.store(a.out + int64_t(row) * a.ld_o, r);
    }
  }
}

// Merge chunk partials [c_beg, c_end) of a split segment, in chunk order, into
// (M, Lsum, acc): m = max m_c, l and acc rescaled by exp(m_c - m), B chunks'
// loads in flight per step, the running max rescaled online as in the main
// kernel.  An empty range leaves (-inf, 0, 0).
template <int V, int R>
__device__ __forceinline__ void merge_chunks(const PoolArgs& a, const Lanes<V, R>& L, int32_t slot0, int32_t c_beg,
                                             int32_t c_end, float& M, double& Lsum, double (&acc)[V * R]) {
  constexpr int B = 8;
  constexpr int W = V * R;
  const int64_t ld_p = a.F + 2;
  for (int32_t c0 = c_beg; c0 < c_end; c0 += B) {
    float mv[B], lv[B], v[B][W];
#pragma unroll
    for (int j = 0; j < B; ++j) {
      const float* p = a.partials + int64_t(slot0 + (c0 + j < c_end ? c0 + j : c_end - 1)) * ld_p;
      mv[j] = p[a.F];
      lv[j] = p[a.F + 1];
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int k = 0; k < V; ++k) v[j][r * V + k] = p[L.off[r] + k];
    }
    float mb = M;
#pragma unroll
    for (int j = 0; j < B; ++j) mb = fmaxf(mb, mv[j]);  // clamped repeats leave the max unchanged
    if (mb > M) {
      const double r = double(expf(M - shift_of(mb)));
      Lsum *= r;
#pragma unroll
      for (int k = 0; k < W; ++k) acc[k] *= r;
      M = mb;
    }
    // every chunk max still -inf: the shift is 0 and each chunk weighs exp(-inf) = 0, so l stays 0
    // and the row ends as 0 / 0 = NaN, the reference's all -inf softmax
    const float ref = shift_of(M);
#pragma unroll
    for (int j = 0; j < B; ++j) {
      const bool in = c0 + j < c_end;  // clamped repeats add nothing (selected, not multiplied by 0)
      const double sc = double(expf(mv[j] - ref));
      Lsum = in ? Lsum + double(lv[j]) * sc : Lsum;
#pragma unroll
      for (int k = 0; k < W; ++k) acc[k] = in ? acc[k] + double(v[j][k]) * sc : acc[k];
    }
  }
}

template <int V, int R>
__device__ __forceinline__ void finish_row(const PoolArgs& a, const Lanes<V, R>& L, int lane, int32_t row, float M,
                                           double Lsum, const double (&acc)[V * R]) {
  if (a.stats && lane == 0) {
    a.stats[int64_t(row) * 2] = M;
    a.stats[int64_t(row) * 2 + 1] = float(Lsum);
  }
  float r[V * R];
#pragma unroll
  for (int k = 0; k < V * R; ++k) r[k] = float(acc[k] / Lsum);
  L.store(a.out + int64_t(row) * a.ld_o, r);
}

// Fix-up, one lane group per split segment: batches whose larger graphs are a few chunks each.
template <int V, int R>
__global__ __launch_bounds__(kBlock) void softmax_pool_fixup_kernel(PoolArgs a) {
  constexpr int W = V * R;
  const int G = a.G;
  const int lane = threadIdx.x & (G - 1);
  const Lanes<V, R> L(lane, G, a.F);
  const int64_t ngroups = group_count(a.lgG);
  for (int64_t it = first_group(a.lgG); it < a.sched.n_split; it += ngroups) {
    const int4 sp = a.sched.split[it];
    float M = -__builtin_inff();
    double Lsum = 0.0, acc[W];
#pragma unroll
    for (int k = 0; k < W; ++k) acc[k] = 0.0;
    merge_chunks<V, R>(a, L, sp.y, 0, sp.z, M, Lsum, acc);
    finish_row<V, R>(a, L, lane, sp.x, M, Lsum, acc);
  }
}

// Fix-up, one block per split segment: the single graph's thousands of chunks.
// Each of the block's kBlock / G lane groups merges a contiguous range of
// chunks in order; group 0 then merges the groups' results in group order
// through LDS.  The grouping depends on the shapes alone: the same bits every run.
template <int V, int R>
__global__ __launch_bounds__(kBlock) void softmax_pool_fixup_block_kernel(PoolArgs a) {
  constexpr int W = V * R;
  __shared__ double sh_acc[kBlock * W];
  __shared__ double sh_l[kBlock];
  __shared__ float sh_m[kBlock];
  const int G = a.G;
  const int lane = threadIdx.x & (G - 1);
  const int grp = threadIdx.x >> a.lgG;
  const int n_grp = kBlock >> a.lgG;
  const Lanes<V, R> L(lane, G, a.F);
  for (int64_t it = blockIdx.x; it < a.sched.n_split; it += gridDim.x) {
    const int4 sp = a.sched.split[it];
    const int32_t nc = sp.z;
    const int32_t per = (nc + n_grp - 1) / n_grp;
    const int32_t c_beg = grp * per < nc ? grp * per : nc;
    const int32_t c_end = c_beg + per < nc ? c_beg + per : nc;
    float M = -__builtin_inff();
    double Lsum = 0.0, acc[W];
#pragma unroll
    for (int k = 0; k < W; ++k) acc[k] = 0.0;
    merge_chunks<V, R>(a, L, sp.y, c_beg, c_end, M, Lsum, acc);
#pragma unroll
    for (int k = 0; k < W; ++k) sh_acc[threadIdx.x * W + k] = acc[k];
    if (lane == 0) {
      sh_m[grp] = M;
      sh_l[grp] = Lsum;
    }
    __syncthreads();
    if (grp == 0) {
      float M2 = -__builtin_inff();
      for (int j = 0; j < n_grp; ++j) M2 = fmaxf(M2, sh_m[j]);
      const float ref = shift_of(M2);
      double L2 = 0.0, acc2[W];
#pragma unroll
      for (int k = 0; k < W; ++k) acc2[k] = 0.0;
      for (int j = 0; j < n_grp; ++j) {  // groups past the last chunk hold (-inf, 0, 0): weight exp(-inf) = 0
        const double sc = double(expf(sh_m[j] - ref));
        L2 += sh_l[j] * sc;
#pragma unroll
        for (int k = 0; k < W; ++k) acc2[k] += sh_acc[(j * G + lane) * W + k] * sc;
      }
      finish_row<V, R>(a, L, lane, sp.x, M2, L2, acc2);
    }
    __syncthreads();  // sh_* are rewritten by the block's next segment
  }
}

template <int V, int R>
int launch(const PoolArgs& a, hipStream_t s) {
  if (const int rc = launch_resident(softmax_pool_kernel<V, R>, a.sched.n_work(), a.G, a, s)) return rc;
  if (a.sched.n_split > 0) {
    // a block per segment once the split segments average (at most n_items / n_split chunks each)
    // four merge steps per lane group of a block; a lane group per segment below that
    const int64_t n_grp = kBlock / a.G;
    if (a.sched.n_items / a.sched.n_split >= 4 * n_grp) {
      auto k = softmax_pool_fixup_block_kernel<V, R>;
      hipLaunchKernelGGL(k, dim3(resident_grid(k, a.sched.n_split, kBlock)), dim3(kBlock), 0, s, a);
    } else {
      auto k = softmax_pool_fixup_kernel<V, R>;
      hipLaunchKernelGGL(k, dim3(resident_grid(k, a.sched.n_split, a.G)), dim3(kBlock), 0, s, a);
    }
    KGX_CHECK_LAUNCH();
  }
  return KGX_OK;
}

// Lane layout of an F-wide row: V floats per vector (4 when every operand is
// 16-byte aligned with F % 4 == 0, else 1), R vectors per lane so that a group
// of at most 64 lanes covers the row (F <= 256).
struct Layout {
  int V, R, G;
};
inline Layout layout_for(int64_t F, bool vec4) {
  Layout y;
  y.V = vec4 ? 4 : 1;
  const int vecs = int((F + y.V - 1) / y.V);
  y.R = vecs <= 64 ? 1 : (vecs <= 128 ? 2 : 4);
  y.G = next_pow2((vecs + y.R - 1) / y.R);
  return y;
}

}  // namespace
}  // namespace kgx

using namespace kgx;

extern "C" int kgx_softmax_pool(const int32_t* rowptr, const int32_t* rows, int64_t n_seg, const int32_t* items,
                                int64_t n_items, const int32_t* split, int64_t n_split, const int32_t* idx,
                                const float* x, int64_t ld_x, int64_t F, const float* s, const float* score_u,
                                const float* score_c, int flags, float* s_out, float* out, int64_t ld_out,
                                float* stats, float* partials, kgx_stream_t stream_) {
  hipStream_t stream = as_stream(stream_);
  KGX_REQUIRE(F > 0 && n_seg >= 0 && n_items >= 0 && n_split >= 0, KGX_ERR_ARG, "kgx_softmax_pool: bad sizes");
  KGX_REQUIRE((flags & ~KGX_POOL_SCORE_TANH) == 0, KGX_ERR_ARG, "kgx_softmax_pool: unknown flags %d", flags);
  if (n_seg == 0) return KGX_OK;
  KGX_REQUIRE(rowptr && (rows || items) && x && out, KGX_ERR_ARG, "kgx_softmax_pool: null pointer");
  KGX_REQUIRE((s != nullptr) != (score_u != nullptr), KGX_ERR_ARG,
              "kgx_softmax_pool: exactly one score source (s, or score_u with score_c)");
  KGX_REQUIRE(!score_u || (score_c && s_out), KGX_ERR_ARG,
              "kgx_softmax_pool: fused scores need score_c and s_out");
  KGX_REQUIRE(score_u || !(flags & KGX_POOL_SCORE_TANH), KGX_ERR_ARG,
              "kgx_softmax_pool: KGX_POOL_SCORE_TANH applies to fused scores only");
  KGX_REQUIRE(ld_x >= F && ld_out >= F, KGX_ERR_ARG, "kgx_softmax_pool: leading dimension < F");
  KGX_REQUIRE(ld_x < (int64_t(1) << 31), KGX_ERR_ARG, "kgx_softmax_pool: leading dimension >= 2^31");
  KGX_REQUIRE(!items || n_split == 0 || (split && partials), KGX_ERR_ARG,
              "kgx_softmax_pool: split rows need split list and partials");
  KGX_REQUIRE(F <= kPoolMaxF, KGX_ERR_UNSUPPORTED, "kgx_softmax_pool: F=%lld above the maximum %d (unsupported)",
              (long long)F, kPoolMaxF);
  const bool vec4 = attn_vec_ok(16, {x, out, score_u}, {F, ld_x, ld_out});
  const Layout y = layout_for(F, vec4);
  PoolArgs a{};
  a.sched = make_sched(rowptr, rows, n_seg, items, n_items, split, n_split);
  a.idx = idx;
  a.x = x;
  a.ld_x = ld_x;
  a.F = int(F);
  a.s = s;
  a.u = score_u;
  a.c = score_c;
  a.tanh_act = (flags & KGX_POOL_SCORE_TANH) ? 1 : 0;
  a.s_out = s_out;
  a.out = out;
  a.ld_o = ld_out;
  a.stats = stats;
  a.partials = partials;
  a.G = y.G;
  a.lgG = log2i(y.G);
  if (y.V == 4) return launch<4, 1>(a, stream);
  switch (y.R) {
    case 1: return launch<1, 1>(a, stream);
    case 2: return launch<1, 2>(a, stream);
    default: return launch<1, 4>(a, stream);
  }
}

// ===========================================================================
// Backward (kgx_softmax_pool_backward).  With G = d loss / d out and the
// forward's (m_g, l_g) = stats, out and scores s:
//   alpha_i     = exp(s_i - m_g) / l_g
//   grad_x[i,:] = alpha_i * G[g,:]
//   grad_s[i]   = alpha_i * (x_i . G_g - out_g . G_g)   (= alpha_i * (x_i - out_g) . G_g)
// Every node is independent once its segment's constants are known: one pass
// over x, no schedule, no partials, no atomics.
// ===========================================================================

namespace kgx {
namespace {

struct PoolBwdArgs {
  int64_t N, n_seg;
  const int32_t* seg;
  const float* x;
  int64_t ld_x;
  int F;
  const float* s;
  const float* stats;
  const float* out;
  int64_t ld_o;
  const float* grad;
  int64_t ld_g;
  float* grad_x;
  int64_t ld_gx;
  float* grad_s;
  int G, lgG;
};

template <int V, int R>
__global__ __launch_bounds__(kBlock) void softmax_pool_bwd_kernel(PoolBwdArgs a) {
  constexpr int W = V * R;
  const int G = a.G;
  const int lane = threadIdx.x & (G - 1);
  const Lanes<V, R> L(lane, G, a.F);
  const int64_t ngroups = group_count(a.lgG);
  for (int64_t i = first_group(a.lgG); i < a.N; i += ngroups) {
    const int32_t g = a.seg ? a.seg[i] : 0;
    const bool in = g >= 0 && g < a.n_seg;  // ids outside the segments pool nowhere: zero gradient
    const int64_t gc = in ? g : 0;
    const float m = a.stats[gc * 2], den = a.stats[gc * 2 + 1];
    float xs[W], gr[W], o[W];
    L.load(xs, a.x + i * a.ld_x);
    L.load(gr, a.grad + gc * a.ld_g);
    L.load(o, a.out + gc * a.ld_o);
    // (x_i - out_g) . G_g: the difference first, so a one-node segment (x_i = out_g) gives exactly 0
    float p = 0.0f;
#pragma unroll
    for (int k = 0; k < W; ++k) p += (xs[k] - o[k]) * gr[k];
    p = group_reduce(p, G);
    const float al = __fdiv_rn(expf(a.s[i] - shift_of(m)), den);
    float r[W];
#pragma unroll
    for (int k = 0; k < W; ++k) r[k] = in ? al * gr[k] : 0.0f;
    L.store(a.grad_x + i * a.ld_gx, r);
    if (lane == 0) a.grad_s[i] = in ? al * p : 0.0f;
  }
}

template <int V, int R>
int launch_bwd(const PoolBwdArgs& a, hipStream_t s) {
  return launch_resident(softmax_pool_bwd_kernel<V, R>, a.N, a.G, a, s);
}

}  // namespace
}  // namespace kgx

extern "C" int kgx_softmax_pool_backward(int64_t N, int64_t n_seg, const int32_t* seg, const float* x, int64_t ld_x,
                                         int64_t F, const float* s, const float* stats, const float* out,
                                         int64_t ld_out, const float* grad_out, int64_t ld_grad, float* grad_x,
                                         int64_t ld_grad_x, float* grad_s, kgx_stream_t stream_) {
  hipStream_t stream = as_stream(stream_);
  KGX_REQUIRE(F > 0 && N >= 0 && n_seg >= 0, KGX_ERR_ARG, "kgx_softmax_pool_backward: bad sizes");
  if (N == 0) return KGX_OK;
  KGX_REQUIRE(n_seg > 0, KGX_ERR_ARG, "kgx_softmax_pool_backward: nodes but no segments");
  KGX_REQUIRE(x && s && stats && out && grad_out && grad_x && grad_s, KGX_ERR_ARG,
              "kgx_softmax_pool_backward: null pointer");
  KGX_REQUIRE(ld_x >= F && ld_out >= F && ld_grad >= F && ld_grad_x >= F, KGX_ERR_ARG,
              "kgx_softmax_pool_backward: leading dimension < F");
  KGX_REQUIRE(F <= kPoolMaxF, KGX_ERR_UNSUPPORTED,
              "kgx_softmax_pool_backward: F=%lld above the maximum %d (unsupported)", (long long)F, kPoolMaxF);
  const bool vec4 = attn_vec_ok(16, {x, out, grad_out, grad_x}, {F, ld_x, ld_out, ld_grad, ld_grad_x});
  const Layout y = layout_for(F, vec4);
  PoolBwdArgs a{};
  a.N = N;
  a.n_seg = n_seg;
  a.seg = seg;
  a.x = x;
  a.ld_x = ld_x;
  a.F = int(F);
  a.s = s;
  a.stats = stats;
  a.out = out;
  a.ld_o = ld_out;
  a.grad = grad_out;
  a.ld_g = ld_grad;
  a.grad_x = grad_x;
  a.ld_gx = ld_grad_x;
  a.grad_s = grad_s;
  a.G = y.G;
  a.lgG = log2i(y.G);
  if (y.V == 4) return launch_bwd<4, 1>(a, stream);
  switch (y.R) {
    case 1: return launch_bwd<1, 1>(a, stream);
    case 2: return launch_bwd<1, 2>(a, stream);
    default: return launch_bwd<1, 4>(a, stream);
  }
}
