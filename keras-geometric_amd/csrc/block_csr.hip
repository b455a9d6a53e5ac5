// The CSR pair of one sampled bipartite block (gfx950): kgx_block_csr.
//
// NeighborSampler assigns local ids seeds first, then hop by hop, and emits the
// hops' edges in that order, so the merged edge list is sorted by destination
// already: it IS the destination CSR (col = src, eid = the edge's position), and
// the block a layer needs is a prefix of it.  What is left to compute is rowptr /
// deg over the sorted destinations and the transposed (source-major) CSR the
// backward pass gathers through.
//
//   block_check_kernel   one lane per edge: counts order and range violations,
//                        writes the sort keys (src) and values (edge position)
//   rocprim radix sort   stable, keyed on src over ceil_log2(n_src) bits
//   block_emit_kernel    rowptr / t_rowptr by binary search of the sorted dst /
//                        sorted src, deg by difference, t_eid = the sorted edge
//                        positions, t_col = their destinations
//
// Every output is an integer and a pure function of the inputs: the stable sort
// places the edges of one source in ascending position, the searches read sorted
// arrays, and the only atomics count violations and fold the two maximum degrees
// (a maximum does not depend on the order it is folded in).  block_emit_kernel
// returns before its first store when a violation was counted, so a rejected
// call writes none of the caller's arrays.  No reference counterpart: the
// reference trains full-batch.
#include <rocprim/device/device_radix_sort.hpp>

#include "kgx_internal.h"

namespace kgx {
namespace {

struct BlockStatus {
  unsigned long long order_bad;  // edges with dst[e] < dst[e - 1]
  unsigned long long range_bad;  // ids outside [0, n_src) / [0, n_dst), each edge end once
  unsigned int max_in;           // largest in-degree (rows of dst)
  unsigned int max_out;          // largest out-degree (rows of src)
};

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ unsigned int wave_max(unsigned int v) {
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned int u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  return v;
}

// the number of entries of the non-decreasing a[0, n) that are < v
template <typename T>
__device__ __forceinline__ int32_t lower_bound(const T* __restrict__ a, int64_t n, int64_t v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (int64_t(a[mid]) < v) lo = mid + 1; else hi = mid;
  }
  return int32_t(lo);
}

__global__ void block_check_kernel(const int32_t* __restrict__ src, const int32_t* __restrict__ dst, int64_t E,
                                   int64_t n_src, int64_t n_dst, uint32_t* __restrict__ keys,
                                   int32_t* __restrict__ pos, BlockStatus* __restrict__ st) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  unsigned long long order_bad = 0, range_bad = 0;
  for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < E; e += stride) {
    const int64_t s = src[e], d = dst[e];
    range_bad += (s < 0 || s >= n_src) + (d < 0 || d >= n_dst);
    order_bad += (e > 0 && d < int64_t(dst[e - 1]));
    keys[e] = uint32_t(s);  // a bad id is only ever a sort key: the emit kernel does not run past it
    pos[e] = int32_t(e);
  }
  order_bad = wave_sum(order_bad);
  range_bad = wave_sum(range_bad);
  if ((threadIdx.x & 63) == 0) {  // status only
    if (order_bad) atomicAdd(&st->order_bad, order_bad);
    if (range_bad) atomicAdd(&st->range_bad, range_bad);
  }
}

// One grid-stride pass over max(E, n_src + 1, n_dst + 1) indices.  sorted_src / sorted_pos: the
// radix sort's output (dst itself is the sorted key array of the forward side).
__global__ void block_emit_kernel(const int32_t* __restrict__ dst, int64_t E, int64_t n_src, int64_t n_dst,
                                  const uint32_t* __restrict__ sorted_src, const int32_t* __restrict__ sorted_pos,
                                  int32_t* __restrict__ rowptr, int32_t* __restrict__ deg,
                                  int32_t* __restrict__ t_rowptr, int32_t* __restrict__ t_deg,
                                  int32_t* __restrict__ t_col, int32_t* __restrict__ t_eid,
                                  BlockStatus* __restrict__ st) {
  if (st->order_bad | st->range_bad) return;  // final: block_check_kernel has finished
  const int64_t n = max(E, max(n_src, n_dst) + 1);
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  unsigned int max_in = 0, max_out = 0;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
    if (i < E) {
      const int32_t p = sorted_pos[i];  // a permutation of [0, E)
      t_eid[i] = p;
      t_col[i] = dst[p];
    }
    if (i <= n_dst) {
      const int32_t b = lower_bound(dst, E, i);
      if (rowptr) rowptr[i] = b;
      if (i < n_dst) {
        const int32_t d = lower_bound(dst, E, i + 1) - b;
        if (deg) deg[i] = d;
        max_in = max(max_in, (unsigned int)d);
      }
    }
    if (i <= n_src) {
      const int32_t b = lower_bound(sorted_src, E, i);
      t_rowptr[i] = b;
      if (i < n_src) {
        const int32_t d = lower_bound(sorted_src, E, i + 1) - b;
        t_deg[i] = d;
        max_out = max(max_out, (unsigned int)d);
      }
    }
  }
  max_in = wave_max(max_in);
  max_out = wave_max(max_out);
  if ((threadIdx.x & 63) == 0) {  // status only, and a maximum is the same in any order
    if (max_in) atomicMax(&st->max_in, max_in);
    if (max_out) atomicMax(&st->max_out, max_out);
  }
}

int sort_end_bit(int64_t n_src) {
  const int b = ceil_log2_u64(uint64_t(n_src > 1 ? n_src : 1));
  return b > 0 ? b : 1;
}

struct BlockLayout {
  uint32_t* keys;
  uint32_t* sorted_src;
  int32_t* pos;
  int32_t* sorted_pos;
  BlockStatus* st;
  void* tmp;
  size_t tmp_bytes;
  size_t total;
};

BlockLayout block_layout(void* ws, int64_t E, int64_t n_src) {
  Carve c(ws, ~size_t(0));
  BlockLayout L;
  L.keys = c.take<uint32_t>(E);
  L.sorted_src = c.take<uint32_t>(E);
  L.pos = c.take<int32_t>(E);
  L.sorted_pos = c.take<int32_t>(E);
  L.st = c.take<BlockStatus>(1);
  L.tmp_bytes = 0;
  uint32_t* k = nullptr;
  int32_t* v = nullptr;
  (void)rocprim::radix_sort_pairs(nullptr, L.tmp_bytes, k, k, v, v, (unsigned)(E > 0 ? E : 1), 0,
                                  sort_end_bit(n_src), 0, false);
  L.tmp = c.take<char>(L.tmp_bytes);
  L.total = c.used();
  return L;
}

constexpr int64_t kInt32Limit = int64_t(1) << 31;

}  // namespace
}  // namespace kgx

using namespace kgx;

extern "C" int kgx_block_workspace_bytes(int64_t E, int64_t n_src, size_t* bytes) {
  KGX_REQUIRE(bytes && E >= 0 && E < kInt32Limit && n_src >= 0 && n_src < kInt32Limit - 1, KGX_ERR_ARG,
              "kgx_block_workspace_bytes: bad arguments");
  *bytes = block_layout(nullptr, E, n_src).total;
  return KGX_OK;
}

extern "C" int kgx_block_csr(const int32_t* src, const int32_t* dst, int64_t E, int64_t n_src, int64_t n_dst,
                             int32_t* rowptr, int32_t* deg, int32_t* t_rowptr, int32_t* t_deg, int32_t* t_col,
                             int32_t* t_eid, void* workspace, size_t workspace_bytes, int64_t* info,
                             kgx_stream_t stream_) {
  hipStream_t stream = as_stream(stream_);
  KGX_REQUIRE(E >= 0 && n_src >= 0 && n_dst >= 0, KGX_ERR_ARG,
              "kgx_block_csr: negative size (E=%lld, n_src=%lld, n_dst=%lld)", (long long)E, (long long)n_src,
              (long long)n_dst);
  KGX_REQUIRE(E < kInt32Limit && n_src < kInt32Limit - 1 && n_dst < kInt32Limit - 1, KGX_ERR_ARG,
              "kgx_block_csr: E=%lld, n_src=%lld, n_dst=%lld do not fit int32 offsets", (long long)E,
              (long long)n_src, (long long)n_dst);
  KGX_REQUIRE(info && t_rowptr && (n_src == 0 || t_deg) && (E == 0 || (src && dst && t_col && t_eid)), KGX_ERR_ARG,
              "kgx_block_csr: null pointer");
  KGX_REQUIRE((rowptr == nullptr) == (deg == nullptr), KGX_ERR_ARG,
              "kgx_block_csr: rowptr and deg are given together, or both NULL");
  BlockLayout L = block_layout(workspace, E, n_src);
  KGX_REQUIRE(workspace && workspace_bytes >= L.total, KGX_ERR_ARG, "kgx_block_csr: workspace %zu < %zu bytes",
              workspace_bytes, L.total);

  KGX_CHECK_HIP(hipMemsetAsync(L.st, 0, sizeof(BlockStatus), stream));
  if (E > 0) {
    hipLaunchKernelGGL(block_check_kernel, dim3(grid_for(E)), dim3(kBlock), 0, stream, src, dst, E, n_src, n_dst,
                       L.keys, L.pos, L.st);
    KGX_CHECK_LAUNCH();
    size_t tb = L.tmp_bytes;
    KGX_CHECK_HIP(rocprim::radix_sort_pairs(L.tmp, tb, L.keys, L.sorted_src, L.pos, L.sorted_pos, (unsigned)E, 0,
                                            sort_end_bit(n_src), stream, false));
  }
  const int64_t n_rows = (n_src > n_dst ? n_src : n_dst) + 1;
  hipLaunchKernelGGL(block_emit_kernel, dim3(grid_for(E > n_rows ? E : n_rows)), dim3(kBlock), 0, stream, dst, E,
                     n_src, n_dst, (const uint32_t*)L.sorted_src, (const int32_t*)L.sorted_pos, rowptr, deg, t_rowptr,
                     t_deg, t_col, t_eid, L.st);
  KGX_CHECK_LAUNCH();
  BlockStatus hs;
  KGX_CHECK_HIP(hipMemcpyAsync(&hs, L.st, sizeof(BlockStatus), hipMemcpyDeviceToHost, stream));
  KGX_CHECK_HIP(hipStreamSynchronize(stream));
  info[0] = int64_t(hs.max_in);
  info[1] = int64_t(hs.max_out);
  info[2] = int64_t(hs.order_bad);
  info[3] = int64_t(hs.range_bad);
  KGX_REQUIRE(hs.range_bad == 0, KGX_ERR_INDEX,
              "kgx_block_csr: %llu id(s) outside [0, %lld) / [0, %lld) (nothing was written)", hs.range_bad,
              (long long)n_src, (long long)n_dst);
  KGX_REQUIRE(hs.order_bad == 0, KGX_ERR_ARG,
              "kgx_block_csr: dst is not sorted: %llu edge(s) with dst[e] < dst[e - 1] (nothing was written)",
              hs.order_bad);
  return KGX_OK;
}
