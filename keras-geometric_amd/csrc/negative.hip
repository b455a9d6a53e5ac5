// Negative sampling for link prediction (gfx950): Q corrupted sources for
// every positive edge (source -> destination a[p]), rejected against the
// destination's own in-neighbours (kgx_negative_edges).
//
// No reference counterpart.  Counter based, like kgx_sample_neighbors: every
// output is a pure function of (seed, the positive's key, q, the destination's
// sorted CSR row), so a positive draws the same negatives in every batch, at
// every position, for every grid size and on every device, and
// tests/negative_ref.py restates it bit for bit.
//
// Key derivation (all arithmetic uint64 modulo 2^64; splitmix64 as below):
//   ks   = splitmix64(seed ^ splitmix64(uint64(uint32(keys[p]))))
//   rs   = splitmix64(ks + q)
//   try t: r = splitmix64(rs + t), cand = ((r >> 32) * n_src) >> 32  in [0, n_src)
// The first candidate that is neither a[p] itself (KGX_NEG_NO_SELF) nor a
// source of a[p]'s row (KGX_NEG_REJECT_EDGES, binary search of the sorted row)
// is the output; after max_tries rejections the last candidate is, and the
// fallback counter says so.
//
// This file carries its own copy of splitmix64, as sampler.hip does.
#include "kgx_internal.h"

namespace kgx {
namespace {

__device__ __host__ __forceinline__ uint64_t splitmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ int32_t wave_sum(int32_t v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// is v in the ascending col[beg, end)?
__device__ __forceinline__ bool row_has(const int32_t* __restrict__ col, int32_t beg, int32_t end, int32_t v) {
  int32_t lo = beg, hi = end;
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (col[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo < end && col[lo] == v;
}

// one lane per output (p, q): coalesced stores for ld_out == Q
__global__ void negative_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                int64_t n_dst, uint64_t n_src, const int32_t* __restrict__ a,
                                const int32_t* __restrict__ keys, int64_t total, uint32_t Q, uint64_t seed,
                                int max_tries, int flags, int32_t* __restrict__ out, int64_t ld_out,
                                int32_t* __restrict__ stats) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  int32_t fell = 0, bad = 0;
  for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < total; e += stride) {
    const uint32_t p = uint32_t(e) / Q;  // total < 2^31
    const uint32_t q = uint32_t(e) - p * Q;
    const int32_t r = a[p];
    int32_t res = -1;
    if (r < 0 || r >= n_dst) {
      bad += q == 0;  // once per positive
    } else {
      int32_t beg = 0, end = 0;
      if (flags & KGX_NEG_REJECT_EDGES) {
        beg = rowptr[r];
        end = rowptr[r + 1];
      }
      const uint64_t ks = splitmix64(seed ^ splitmix64(uint64_t(uint32_t(keys[p]))));
      const uint64_t rs = splitmix64(ks + uint64_t(q));
      bool found = false;
      for (int t = 0; t < max_tries && !found; ++t) {
        res = int32_t(((splitmix64(rs + uint64_t(t)) >> 32) * n_src) >> 32);
        found = !(((flags & KGX_NEG_NO_SELF) && res == r) || row_has(col, beg, end, res));
      }
      fell += !found;
    }
    out[int64_t(p) * ld_out + q] = res;
  }
  fell = wave_sum(fell);
  bad = wave_sum(bad);
  if ((threadIdx.x & 63) == 0) {  // status only: no output value depends on an atomic
    if (fell) atomicAdd(stats, fell);
    if (bad) atomicAdd(stats + 1, bad);
  }
}

constexpr int64_t kInt32Limit = int64_t(1) << 31;

}  // namespace
}  // namespace kgx

using namespace kgx;

extern "C" int kgx_negative_edges(const int32_t* rowptr, const int32_t* col_sorted, int64_t n_dst, int64_t n_src,
                                  const int32_t* a, const int32_t* keys, int64_t P, int Q, uint64_t seed,
                                  int max_tries, int flags, int32_t* out, int64_t ld_out, int32_t* stats,
                                  kgx_stream_t stream_) {
  hipStream_t stream = as_stream(stream_);
  KGX_REQUIRE(Q >= 1, KGX_ERR_ARG, "kgx_negative_edges: Q must be >= 1 (got %d)", Q);
  KGX_REQUIRE(max_tries >= 1 && max_tries <= 64, KGX_ERR_ARG, "kgx_negative_edges: max_tries %d outside 1..64",
              max_tries);
  KGX_REQUIRE(n_src >= 1 && n_src < kInt32Limit, KGX_ERR_ARG, "kgx_negative_edges: n_src %lld outside [1, 2^31)",
              (long long)n_src);
  KGX_REQUIRE(P >= 0 && n_dst >= 0 && n_dst < kInt32Limit, KGX_ERR_ARG,
              "kgx_negative_edges: bad size (P=%lld, n_dst=%lld)", (long long)P, (long long)n_dst);
  KGX_REQUIRE((flags & ~(KGX_NEG_NO_SELF | KGX_NEG_REJECT_EDGES)) == 0, KGX_ERR_ARG,
              "kgx_negative_edges: unknown flags %d", flags);
  KGX_REQUIRE(ld_out >= Q, KGX_ERR_ARG, "kgx_negative_edges: ld_out %lld < Q %d", (long long)ld_out, Q);
  KGX_REQUIRE(P < kInt32Limit && P * int64_t(Q) < kInt32Limit, KGX_ERR_ARG,
              "kgx_negative_edges: P * Q = %lld * %d does not fit int32", (long long)P, Q);
  if (P == 0) return KGX_OK;
  KGX_REQUIRE(a && keys && out && stats, KGX_ERR_ARG, "kgx_negative_edges: null pointer");
  KGX_REQUIRE(!(flags & KGX_NEG_REJECT_EDGES) || (rowptr && col_sorted), KGX_ERR_ARG,
              "kgx_negative_edges: KGX_NEG_REJECT_EDGES needs rowptr and col_sorted");
  const int64_t total = P * int64_t(Q);
  hipLaunchKernelGGL(negative_kernel, dim3(grid_for(total)), dim3(kBlock), 0, stream, rowptr, col_sorted, n_dst,
                     uint64_t(n_src), a, keys, total, uint32_t(Q), seed, max_tries, flags, out, ld_out, stats);
  KGX_CHECK_LAUNCH();
  return KGX_OK;
}
