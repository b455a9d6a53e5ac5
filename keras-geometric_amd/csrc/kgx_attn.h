// The core the segment-softmax kernels share (gatv2.hip, dot_attention.hip and,
// for the reduction and the schedule only, softmax_pool.hip): the DPP group
// reduction, the row / chunk schedule, the attention dropout mask, the head /
// sub-lane prologue, the fp64 online-softmax block update, the chunk-order
// fix-ups of split rows and the launch helpers.
//
// What differs between the attention ops is a Policy (see GatSoftmax in
// gatv2.hip and DotSoftmax in dot_attention.hip; DESIGN.md §12 lists them):
//   kBias, kZeroEmptyRow     bias added in the store; a row without edges stores zeros
//   fixup_batch<K>()         chunk loads in flight per step of the forward fix-up
//   den(l)                   the denominator, which is also what stats keep
//   rescale(m, m_new)        factor of the running sums when the max moves
//   weight(s, m)             weight of a score (and of a chunk max) under max m
#pragma once

#include <cstdlib>
#include <type_traits>

#include "kgx_internal.h"
#include "kgx_vec.h"

namespace kgx {
namespace {

// Sum over a group of n (power of two) adjacent lanes, result in every lane.
// Within 16 lanes the exchanges are DPP moves (VALU, no LDS round trip):
// quad_perm xor 1 and xor 2, then row_half_mirror (lane i <-> 7-i) and
// row_mirror (i <-> 15-i) pair each lane with one holding the other half's sum.
template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float group_reduce(float p, int n) {
  if (n > 1) p += dpp<0xB1>(p);   // quad_perm [1,0,3,2]
  if (n > 2) p += dpp<0x4E>(p);   // quad_perm [2,3,0,1]
  if (n > 4) p += dpp<0x141>(p);  // row_half_mirror
  if (n > 8) p += dpp<0x140>(p);  // row_mirror
  if (n > 16) p += __shfl_xor(p, 16, 64);
  if (n > 32) p += __shfl_xor(p, 32, 64);
  return p;
}

// Lane groups of 1 << lgG lanes stride over work items: this thread's first
// item, and the grid's group count.
__device__ __forceinline__ int64_t first_group(int lgG) {
  return (int64_t(blockIdx.x) * kBlock + threadIdx.x) >> lgG;
}
__device__ __forceinline__ int64_t group_count(int lgG) { return (int64_t(gridDim.x) * kBlock) >> lgG; }

// A CSR's schedule: `items` (row, beg, end, slot) with hub rows cut into
// chunks (slot >= 0: the chunk's partial; `split` lists (row, first slot,
// chunks) of the cut rows), or, without items, whole rows in `rows` order.
struct Sched {
  const int32_t* rowptr;
  const int32_t* rows;
  int64_t n_rows;
  const int4* items;
  int64_t n_items;
  const int4* split;
  int64_t n_split;
  __host__ __device__ int64_t n_work() const { return items ? n_items : n_rows; }
};

__device__ __forceinline__ void work_item(const Sched& s, int64_t it, int32_t& row, int32_t& beg, int32_t& end,
                                          int32_t& slot) {
  if (s.items) {
    const int4 v = s.items[it];
    row = v.x;
    beg = v.y;
    end = v.z;
    slot = v.w;
  } else {
    row = s.rows[it];
    beg = s.rowptr[row];
    end = s.rowptr[row + 1];
    slot = -1;
  }
}

// Without an item list there are no chunks: n_items and n_split are 0 then.
inline Sched make_sched(const int32_t* rowptr, const int32_t* rows, int64_t n_rows, const int32_t* items,
                        int64_t n_items, const int32_t* split, int64_t n_split) {
  Sched s{};
  s.rowptr = rowptr;
  s.rows = rows;
  s.n_rows = n_rows;
  s.items = reinterpret_cast<const int4*>(items);
  s.n_items = items ? n_items : 0;
  s.split = reinterpret_cast<const int4*>(split);
  s.n_split = items ? n_split : 0;
  return s;
}

// Attention dropout (training): alpha_e *= keep(seed, key[e], head) / (1 - p).
// key == null: no dropout.
struct Drop {
  const int32_t* key;
  uint64_t seed;
  uint32_t thresh;
  float scale;
  __device__ __forceinline__ float multiplier(int32_t e, int head) const {
    return key ? drop_scale(seed, uint32_t(key[e]), uint32_t(head), thresh, scale) : 1.0f;
  }
};

inline Drop make_drop(const int32_t* key, float p, uint64_t seed) {
  Drop d{};
  if (key && p > 0.0f) {
    d.key = key;
    d.seed = seed;
    d.thresh = uint32_t(double(p) * 4294967296.0);
    d.scale = 1.0f / (1.0f - p);
  }
  return d;
}

#define KGX_REQUIRE_DROP_P(p, fn) \
  KGX_REQUIRE((p) >= 0.0f && (p) < 1.0f, KGX_ERR_ARG, fn ": dropout p must be in [0, 1)")

// Edge tables (kgx_dot_attention_edge, kgx_gatv2_edge): the edge row of slot t
// (idx null: the slot itself) and whether it has one (a row inside [0, n_e)).
__device__ __forceinline__ bool edge_row(const int32_t* idx, int32_t n_e, int32_t t, int32_t& r) {
  r = idx ? idx[t] : t;
  return uint32_t(r) < uint32_t(n_e);
}

// This thread's place in its row's lane group: K channels from `f` of `head`.
// Padding lanes (head >= H, or a sub-lane past C) are not valid; their f is 0,
// so they can load from a valid address and use nothing.
template <int K>
struct HeadLanes {
  int head, sub, f;
  bool valid;
  __device__ __forceinline__ HeadLanes(const AttnLayout& y, int H, int C) {
    const int lane = threadIdx.x & (y.G - 1);
    head = lane >> y.lgLH;
    sub = lane & (y.LH - 1);
    valid = head < H && sub * K < C;
    f = valid ? head * C + sub * K : 0;
  }
  __device__ __forceinline__ int head0() const { return valid ? head : 0; }
};

// Where the forward kernels write: rows of `out`, chunk partials per slot
// [H*C acc | H m | H l] ld_p floats apart, and optionally stats [n, 2H], per
// row and head the softmax max m and the policy's denominator.
struct AttnOut {
  float* out;
  int64_t ld_o;
  float* partials;
  int64_t ld_p;
  float* stats;
  const float* bias;  // policies with kBias only
};

// One block of the online softmax: U scores s (the first n count) of this
// lane's head, their dropout multipliers and value rows update the running max
// m, denominator l and numerator acc.  Both sums are fp64: a hub row sums 10^5
// terms, whose fp32 rounding (~sqrt(n) ulp) would exceed 1e-5, and the fp64
// FMAs are free in these HBM-bound kernels.
template <int K, int U, typename P>
__device__ __forceinline__ void softmax_block(const float (&s)[U], int n, const float (&dm)[U],
                                              const float (&v)[U][K], float& m, double& l, double (&acc)[K]) {
  float mc = -__builtin_inff();
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (u < n) mc = fmaxf(mc, s[u]);
  const float m_new = fmaxf(m, mc);
  const double r = P::rescale(m, m_new);
  l *= r;
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] *= r;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (u < n) {
      const double pu = double(P::weight(s[u], m_new));
      l += pu;  // the denominator sees every edge; dropout masks the normalised weight
      const double pd = pu * double(dm[u]);
#pragma unroll
      for (int k = 0; k < K; ++k) acc[k] = fma(pd, double(v[u][k]), acc[k]);
    }
  }
  m = m_new;
}

// A chunk's running state into its partial slot (valid lanes only).
template <int K>
__device__ __forceinline__ void store_partial(const AttnOut& o, int H, int HC, const HeadLanes<K>& L, int32_t slot,
                                              float m, double l, const double (&acc)[K]) {
  float* p = o.partials + int64_t(slot) * o.ld_p;
  float accf[K];
#pragma unroll
  for (int k = 0; k < K; ++k) accf[k] = float(acc[k]);
  vstore<K>(p + L.f, accf);
  if (L.sub == 0) {
    p[HC + L.head] = m;
    p[HC + H + L.head] = float(l);
  }
}

// A whole row's (m, l, acc) into stats and out (valid lanes only).
template <int K, typename P>
__device__ __forceinline__ void finish_row(const AttnOut& o, int H, const HeadLanes<K>& L, int32_t row, float m,
                                           double l, const double (&acc)[K], bool empty) {
  const double den = P::den(l);
  if (o.stats && L.sub == 0) {
    o.stats[int64_t(row) * 2 * H + L.head] = m;
    o.stats[int64_t(row) * 2 * H + H + L.head] = float(den);
  }
  float r[K];
#pragma unroll
  for (int k = 0; k < K; ++k) r[k] = (P::kZeroEmptyRow && empty) ? 0.0f : float(acc[k] / den);
  if (P::kBias && o.bias) {
    float b[K];
    vload<K>(b, o.bias + L.f);
#pragma unroll
    for (int k = 0; k < K; ++k) r[k] += b[k];
  }
  vstore<K>(o.out + int64_t(row) * o.ld_o + L.f, r);
}

// Merges the nc chunk partials from slot0 on, in chunk order, into (M, Lsum,
// acc).  One pass, B chunks' loads in flight per step (clamped, unconditional),
// the running max rescaled online as in the main kernels: a hub row's ~160
// partials cost ~10 load latencies, not ~320.
template <int K, int B, typename P>
__device__ __forceinline__ void merge_partials(const AttnOut& o, int H, int HC, const HeadLanes<K>& L,
                                               int32_t slot0, int32_t nc, float& M, double& Lsum,
                                               double (&acc)[K]) {
  const int64_t ld_p = o.ld_p;
  for (int32_t c0 = 0; c0 < nc; c0 += B) {
    float mv[B], lv[B], v[B][K];
#pragma unroll
    for (int u = 0; u < B; ++u) {
      const float* p = o.partials + int64_t(slot0 + (c0 + u < nc ? c0 + u : nc - 1)) * ld_p;
      mv[u] = p[HC + L.head];
      lv[u] = p[HC + H + L.head];
      vload<K>(v[u], p + L.f);
    }
    float mb = M;
#pragma unroll
    for (int u = 0; u < B; ++u) mb = fmaxf(mb, mv[u]);  // clamped repeats leave the max unchanged
    if (__builtin_expect(mb > M, false)) {  // after a row's first chunks the max seldom moves: keep it a branch
      const double r = double(expf(M - mb));  // M = -inf: 0, and Lsum and acc are still 0
      Lsum *= r;
#pragma unroll
      for (int k = 0; k < K; ++k) acc[k] *= r;
      M = mb;
    }
#pragma unroll
    for (int u = 0; u < B; ++u) {
      const bool in = c0 + u < nc;  // clamped repeats add nothing (selected, not multiplied by 0: inf rows stay inf)
      const double sc = double(P::weight(mv[u], M));
      Lsum = in ? Lsum + double(lv[u]) * sc : Lsum;
#pragma unroll
      for (int k = 0; k < K; ++k) acc[k] = in ? acc[k] + double(v[u][k]) * sc : acc[k];
    }
  }
}

// The forward fix-up's body: one lane group per split row.
template <int K, typename P>
__device__ __forceinline__ void fixup_rows(const Sched& s, const AttnLayout& y, int H, int C, const AttnOut& o) {
  const HeadLanes<K> L(y, H, C);
  if (!L.valid) return;  // no cross-lane work here
  const int64_t ngroups = group_count(y.lgG);
  for (int64_t it = first_group(y.lgG); it < s.n_split; it += ngroups) {
    const int4 sp = s.split[it];
    float M = -__builtin_inff();
    double Lsum = 0.0, acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    merge_partials<K, P::template fixup_batch<K>(), P>(o, H, H * C, L, sp.y, sp.z, M, Lsum, acc);
    finish_row<K, P>(o, H, L, sp.x, M, Lsum, acc, false);
  }
}

// The backward fix-up: sums the chunk partials of split rows in chunk order,
// columns [0, HC) of a slot into out0, columns [HC, W) (W = HC or 2 HC) into
// out1.  One 64-lane group per split row.  (A template, so that a translation
// unit without a backward fix-up gets no copy of it.)
template <int B>  // chunk loads in flight, then the in-order sum
__global__ __launch_bounds__(kBlock) void chunk_sum_fixup_kernel(const int4* __restrict__ split, int64_t n_split,
                                                                 const float* __restrict__ partials, int64_t ld_p,
                                                                 int HC, int W, float* __restrict__ out0,
                                                                 int64_t ld0, float* __restrict__ out1,
                                                                 int64_t ld1) {
  const int lane = threadIdx.x & 63;
  const int64_t ngroups = group_count(6);
  for (int64_t it = first_group(6); it < n_split; it += ngroups) {
    const int4 sp = split[it];
    for (int f = lane; f < W; f += 64) {
      float acc = 0.0f;
      for (int32_t c0 = 0; c0 < sp.z; c0 += B) {
        float pv[B];
#pragma unroll
        for (int u = 0; u < B; ++u) pv[u] = partials[int64_t(sp.y + (c0 + u < sp.z ? c0 + u : sp.z - 1)) * ld_p + f];
#pragma unroll
        for (int u = 0; u < B; ++u) acc = c0 + u < sp.z ? acc + pv[u] : acc;
      }
      if (f < HC) out0[int64_t(sp.x) * ld0 + f] = acc;
      else out1[int64_t(sp.x) * ld1 + (f - HC)] = acc;
    }
  }
}

// A persistent grid of lane groups of G lanes over `work` items (none: no launch).
template <typename Kern, typename Args>
int launch_resident(Kern kernel, int64_t work, int G, const Args& a, hipStream_t s) {
  if (work <= 0) return KGX_OK;
  hipLaunchKernelGGL(kernel, dim3(resident_grid(kernel, work, G)), dim3(kBlock), 0, s, a);
  KGX_CHECK_LAUNCH();
  return KGX_OK;
}

// The forward pair: a resident grid over the work items of a.sched, then one
// over its split rows.
template <typename Main, typename Fix, typename Args>
int launch_with_fixup(Main main_kernel, Fix fixup_kernel, const Args& a, hipStream_t s) {
  if (const int rc = launch_resident(main_kernel, a.sched.n_work(), a.lay.G, a, s)) return rc;
  return launch_resident(fixup_kernel, a.sched.n_split, a.lay.G, a, s);
}

template <int B = 8>
int launch_chunk_sum(const Sched& sc, const float* partials, int64_t ld_p, int HC, int W, float* out0,
                            int64_t ld0, float* out1, int64_t ld1, hipStream_t s) {
  if (sc.n_split <= 0) return KGX_OK;
  hipLaunchKernelGGL(chunk_sum_fixup_kernel<B>, dim3(grid_for(sc.n_split * 64, 4096)), dim3(kBlock), 0, s, sc.split,
                     sc.n_split, partials, ld_p, HC, W, out0, ld0, out1, ld1);
  KGX_CHECK_LAUNCH();
  return KGX_OK;
}

// f(std::integral_constant<int, K>) for the K channels per lane a layout chose.
template <typename F>
int dispatch_k(int K, F&& f) {
  switch (K) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    default: return f(std::integral_constant<int, 16>{});
  }
}

// An experiment knob's integer value (0: unset); callers cache it in a function-local static.
inline int env_int(const char* name) {
  const char* h = getenv(name);
  return h ? atoi(h) : 0;
}

}  // namespace
}  // namespace kgx
