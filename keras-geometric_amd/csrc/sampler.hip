// Neighbour sampling for mini-batch GraphSAGE training (gfx950).
//
//   one hop of fan-out sampling over a destination CSR  (kgx_sample_neighbors)
//   compaction of a hop's sources into local ids         (kgx_relabel_frontier)
//
// No reference counterpart: the reference trains full-batch.  The sample is
// counter based, like kgx_rmat_edges: every output is a pure function of
// (seed, hop, the row's global id, the row's CSR slots), so a node draws the
// same neighbours in every batch, at every position in `seeds`, for every grid
// size and on every device, and tests/sampling_ref.py restates it bit for bit.
//
// Key derivation (all arithmetic uint64 modulo 2^64; splitmix64 as below):
//   hs     = splitmix64(seed ^ splitmix64(uint64(uint32(hop))))
//   rs     = splitmix64(hs ^ uint64(row))           row = the seed's global id
//   key[i] = splitmix64(rs + i)                     i = 0..3
//   rot    = ((splitmix64(rs + 4) >> 32) * d) >> 32 in [0, d)
// A row of degree d > k takes the CSR slots pi(0), ..., pi(k-1) in that order,
// pi(t) = (phi(t) + rot) mod d, phi = the 4-round Feistel permutation with those
// keys on 2*hb bits, hb = ceil(ceil_log2(d) / 2), cycle-walked into [0, d) (the
// walked superset 2^(2 hb) is smaller than 4 d).  The row-keyed rotation is
// there because four rounds on halves of one or two bits are measurably biased
// even under ideal keys (d = 10, k = 3: slots 0-3 drawn with frequency 0.315,
// slots 4-7 with 0.288); rotated, every slot of a row is drawn with probability
// k / d.  A row of degree d <= k (or fanout -1) is taken whole, in CSR order.
// Sampling is over CSR slots: an edge the input lists twice has two slots and
// can be drawn once per copy.
//
// This file carries its own copy of the splitmix64 / Feistel helpers of
// graph_build.hip, so that neither that file nor a header it includes changes.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "kgx_internal.h"

namespace kgx {
namespace {

__device__ __host__ __forceinline__ uint64_t splitmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

struct Feistel {
  uint64_t keys[4];
  int hb;          // half width in bits
  uint64_t mask;   // (1 << hb) - 1
};

__device__ __forceinline__ uint64_t feistel_once(const Feistel& f, uint64_t x) {
  uint64_t L = x >> f.hb, R = x & f.mask;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint64_t nl = R;
    R = L ^ (splitmix64(f.keys[i] ^ R) & f.mask);
    L = nl;
  }
  return (L << f.hb) | R;
}

// pi(t) for the row's keys: a bijection of [0, d) (cycle walking terminates: feistel_once is
// a bijection of the superset [0, 2^(2 hb)), d >= 2)
__device__ __forceinline__ uint32_t row_perm(uint64_t hs, uint32_t row, uint32_t d, uint32_t t) {
  Feistel f;
  const uint64_t rs = splitmix64(hs ^ uint64_t(row));
#pragma unroll
  for (int i = 0; i < 4; ++i) f.keys[i] = splitmix64(rs + uint64_t(i));
  const int lg = 32 - __clz(int(d - 1));  // ceil_log2(d), d >= 2
  f.hb = (lg + 1) >> 1;
  f.mask = (uint64_t(1) << f.hb) - 1;
  uint64_t y = feistel_once(f, t);
  while (y >= d) y = feistel_once(f, y);
  const uint64_t rot = ((splitmix64(rs + 4) >> 32) * uint64_t(d)) >> 32;  // in [0, d)
  y += rot;
  return uint32_t(y >= d ? y - d : y);
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the row of output slot e: the largest i in [0, n) with off[i] <= e (off[n] > e)
__device__ __forceinline__ int64_t row_of(const int32_t* __restrict__ off, int64_t n, int64_t e) {
  int64_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (off[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

// --------------------------------------------------------------------------
// one hop
// --------------------------------------------------------------------------
struct SampleStatus {
  unsigned long long total;  // sum of the rows' sample counts, in 64 bits
  unsigned long long bad;    // seeds outside [0, n_rows)
};

// cnt[i] = min(deg(seeds[i]), k) (deg with fanout -1; 0 for a seed out of range), cnt[n_seeds] = 0
__global__ void sample_count_kernel(const int32_t* __restrict__ rowptr, int64_t n_rows,
                                    const int32_t* __restrict__ seeds, int64_t n_seeds, int fanout,
                                    int32_t* __restrict__ cnt, SampleStatus* __restrict__ st) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  unsigned long long total = 0, bad = 0;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i <= n_seeds; i += stride) {
    int32_t c = 0;
    if (i < n_seeds) {
      const int64_t r = seeds[i];
      if (r < 0 || r >= n_rows) {
        ++bad;
      } else {
        const int32_t d = rowptr[r + 1] - rowptr[r];
        c = (fanout < 0 || d < fanout) ? d : fanout;
        if (c < 0) c = 0;
      }
    }
    cnt[i] = c;
    total += (unsigned long long)c;
  }
  total = wave_sum(total);
  bad = wave_sum(bad);
  if ((threadIdx.x & 63) == 0) {  // status only: no output value depends on an atomic
    if (total) atomicAdd(&st->total, total);
    if (bad) atomicAdd(&st->bad, bad);
  }
}

// one lane per output slot e = (seed i, draw t): coalesced out_* stores, one random dword
// per lane from col and eid
__global__ void sample_emit_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                   const int32_t* __restrict__ eid, const int32_t* __restrict__ seeds,
                                   int64_t n_seeds, int fanout, uint64_t hs,
                                   const int32_t* __restrict__ out_rowptr, const SampleStatus* __restrict__ st,
                                   int64_t cap, int32_t* __restrict__ out_src, int32_t* __restrict__ out_eid) {
  // more samples than the caller's buffers hold (this also covers an int32 overflow of the
  // scan): nothing is written, the host reports it after the sync
  if (st->total > (unsigned long long)cap) return;
  const int64_t total = out_rowptr[n_seeds];
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < total; e += stride) {
    const int64_t i = row_of(out_rowptr, n_seeds, e);
    const uint32_t t = uint32_t(e - out_rowptr[i]);
    const int32_t r = seeds[i];  // in range: rows of bad seeds are empty
    const int32_t b = rowptr[r];
    const int32_t d = rowptr[r + 1] - b;
    const uint32_t slot = (fanout < 0 || d <= fanout) ? t : row_perm(hs, uint32_t(r), uint32_t(d), t);
    out_src[e] = col[int64_t(b) + slot];
    out_eid[e] = eid[int64_t(b) + slot];
  }
}

size_t scan_temp_bytes(int64_t n) {
  size_t bytes = 0;
  const int32_t* si = nullptr;
  int32_t* so = nullptr;
  (void)rocprim::exclusive_scan(nullptr, bytes, si, so, 0, (size_t)(n > 0 ? n : 1), rocprim::plus<int32_t>(), 0,
                                false);
  return bytes;
}

struct SampleLayout {
  int32_t* cnt;
  SampleStatus* st;
  void* tmp;
  size_t tmp_bytes;
  size_t total;
};

SampleLayout sample_layout(void* ws, int64_t n_seeds) {
  Carve c(ws, ~size_t(0));
  SampleLayout L;
  L.cnt = c.take<int32_t>(n_seeds + 1);
  L.st = c.take<SampleStatus>(1);
  L.tmp_bytes = scan_temp_bytes(n_seeds + 1);
  L.tmp = c.take<char>(L.tmp_bytes);
  L.total = c.used();
  return L;
}

// --------------------------------------------------------------------------
// relabel
// --------------------------------------------------------------------------
struct RelabelStatus {
  unsigned long long n_new;  // sampled sources not yet in `nodes`, each once
  unsigned long long dup;    // entries of `nodes` whose id another entry also holds
  unsigned long long bad;    // ids outside [0, n_nodes)
};

__global__ void map_write_kernel(const int32_t* __restrict__ nodes, int64_t n_known, int64_t n_nodes,
                                 int32_t* __restrict__ map, RelabelStatus* __restrict__ st) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  unsigned long long bad = 0;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n_known; i += stride) {
    const int64_t v = nodes[i];
    if (v < 0 || v >= n_nodes) ++bad; else map[v] = int32_t(i);
  }
  bad = wave_sum(bad);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(&st->bad, bad);
}

// after map_write_kernel has finished: an entry that does not read its own index back shares
// its id with another entry
__global__ void map_check_kernel(const int32_t* __restrict__ nodes, int64_t n_known, int64_t n_nodes,
                                 const int32_t* __restrict__ map, RelabelStatus* __restrict__ st) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  unsigned long long dup = 0;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n_known; i += stride) {
    const int64_t v = nodes[i];
    if (v >= 0 && v < n_nodes && map[v] != int32_t(i)) ++dup;
  }
  dup = wave_sum(dup);
  if ((threadIdx.x & 63) == 0 && dup) atomicAdd(&st->dup, dup);
}

// sort key of sampled source e: its id when it is not in `nodes` yet, n_nodes (sorts last) otherwise
__global__ void new_keys_kernel(const int32_t* __restrict__ out_src, int64_t n_edges, int64_t n_nodes,
                                const int32_t* __restrict__ map, uint32_t* __restrict__ keys,
                                RelabelStatus* __restrict__ st) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  unsigned long long bad = 0;
  for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < n_edges; e += stride) {
    const int64_t s = out_src[e];
    const bool in = s >= 0 && s < n_nodes;
    bad += !in;
    keys[e] = (in && map[s] < 0) ? uint32_t(s) : uint32_t(n_nodes);
  }
  bad = wave_sum(bad);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(&st->bad, bad);
}

__global__ void unique_flags_kernel(const uint32_t* __restrict__ sorted, int64_t n_edges, int64_t n_nodes,
                                    int32_t* __restrict__ flags) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; j < n_edges; j += stride) {
    const uint32_t v = sorted[j];
    flags[j] = (v != uint32_t(n_nodes) && (j == 0 || sorted[j - 1] != v)) ? 1 : 0;
  }
}

// new_nodes[rank] = id, map[id] = n_known + rank (ranks from the scan: ascending id)
__global__ void select_new_kernel(const uint32_t* __restrict__ sorted, const int32_t* __restrict__ flags,
                                  const int32_t* __restrict__ pos, int64_t n_edges, int64_t n_known,
                                  int32_t* __restrict__ new_nodes, int32_t* __restrict__ map,
                                  RelabelStatus* __restrict__ st) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; j < n_edges; j += stride) {
    if (flags[j]) {  // pos[j] < n_edges: new_nodes holds n_edges entries
      new_nodes[pos[j]] = int32_t(sorted[j]);
      map[sorted[j]] = int32_t(n_known + pos[j]);
    }
    if (j == n_edges - 1) st->n_new = (unsigned long long)(pos[j] + flags[j]);
  }
}

__global__ void local_ids_kernel(const int32_t* __restrict__ out_rowptr, const int32_t* __restrict__ out_src,
                                 const int32_t* __restrict__ frontier, int64_t n_f, int64_t n_edges,
                                 int64_t n_nodes, const int32_t* __restrict__ map,
                                 int32_t* __restrict__ src_local, int32_t* __restrict__ dst_local,
                                 RelabelStatus* __restrict__ st) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  unsigned long long bad = 0;
  for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < n_edges; e += stride) {
    const int64_t s = out_src[e];
    const int64_t f = frontier[row_of(out_rowptr, n_f, e)];
    const bool f_in = f >= 0 && f < n_nodes;
    bad += !f_in;  // a bad source was counted by new_keys_kernel
    src_local[e] = (s >= 0 && s < n_nodes) ? map[s] : -1;
    dst_local[e] = f_in ? map[f] : -1;
  }
  bad = wave_sum(bad);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(&st->bad, bad);
}

// map back to all -1: the entries of `nodes` and of the new nodes (their count is on the device)
__global__ void map_reset_kernel(const int32_t* __restrict__ nodes, int64_t n_known,
                                 const int32_t* __restrict__ new_nodes, const RelabelStatus* __restrict__ st,
                                 int64_t n_nodes, int32_t* __restrict__ map) {
  const int64_t n_new = int64_t(st->n_new);
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n_known + n_new; i += stride) {
    const int64_t v = i < n_known ? nodes[i] : new_nodes[i - n_known];
    if (v >= 0 && v < n_nodes) map[v] = -1;
  }
}

struct RelabelLayout {
  uint32_t* keys;
  uint32_t* sorted;
  int32_t* flags;
  int32_t* pos;
  RelabelStatus* st;
  void* tmp;
  size_t tmp_bytes;
  size_t total;
};

RelabelLayout relabel_layout(void* ws, int64_t n_edges, int64_t n_nodes) {
  Carve c(ws, ~size_t(0));
  RelabelLayout L;
  L.keys = c.take<uint32_t>(n_edges);
  L.sorted = c.take<uint32_t>(n_edges);
  L.flags = c.take<int32_t>(n_edges);
  L.pos = c.take<int32_t>(n_edges);
  L.st = c.take<RelabelStatus>(1);
  size_t sb = 0;
  uint32_t* k = nullptr;
  const int end_bit = ceil_log2_u64(uint64_t(n_nodes) + 1);
  (void)rocprim::radix_sort_keys(nullptr, sb, k, k, (unsigned)(n_edges > 0 ? n_edges : 1), 0,
                                 end_bit > 0 ? end_bit : 1, 0, false);
  const size_t scb = scan_temp_bytes(n_edges);
  L.tmp_bytes = sb > scb ? sb : scb;
  L.tmp = c.take<char>(L.tmp_bytes);
  L.total = c.used();
  return L;
}

constexpr int64_t kInt32Limit = int64_t(1) << 31;

}  // namespace
}  // namespace kgx

using namespace kgx;

extern "C" int kgx_sample_workspace_bytes(int64_t n_seeds, size_t* bytes) {
  KGX_REQUIRE(bytes && n_seeds >= 0 && n_seeds < kInt32Limit - 1, KGX_ERR_ARG,
              "kgx_sample_workspace_bytes: bad arguments");
  *bytes = sample_layout(nullptr, n_seeds).total;
  return KGX_OK;
}

extern "C" int kgx_sample_neighbors(const int32_t* rowptr, const int32_t* col, const int32_t* eid, int64_t n_rows,
                                    const int32_t* seeds, int64_t n_seeds, int fanout, uint64_t seed, int hop,
                                    int32_t* out_rowptr, int32_t* out_src, int32_t* out_eid, int64_t cap,
                                    void* workspace, size_t workspace_bytes, int64_t* info,
                                    kgx_stream_t stream_) {
  hipStream_t stream = as_stream(stream_);
  KGX_REQUIRE(fanout >= 1 || fanout == -1, KGX_ERR_ARG,
              "kgx_sample_neighbors: fanout must be >= 1, or -1 for all neighbours (got %d)", fanout);
  KGX_REQUIRE(n_seeds >= 0 && n_rows >= 0 && cap >= 0, KGX_ERR_ARG,
              "kgx_sample_neighbors: negative size (n_seeds=%lld, n_rows=%lld, cap=%lld)", (long long)n_seeds,
              (long long)n_rows, (long long)cap);
  KGX_REQUIRE(n_seeds < kInt32Limit - 1 && n_rows < kInt32Limit - 1 && cap < kInt32Limit &&
                  (fanout < 0 || n_seeds * int64_t(fanout) < kInt32Limit),
              KGX_ERR_ARG, "kgx_sample_neighbors: n_seeds * fanout = %lld * %d does not fit int32 offsets",
              (long long)n_seeds, fanout);
  if (n_seeds == 0) {
    if (info) info[0] = info[1] = info[2] = info[3] = 0;
    return KGX_OK;
  }
  KGX_REQUIRE(rowptr && col && eid && seeds && out_rowptr && out_src && out_eid && info, KGX_ERR_ARG,
              "kgx_sample_neighbors: null pointer");
  KGX_REQUIRE(fanout < 0 || cap >= n_seeds * int64_t(fanout), KGX_ERR_ARG,
              "kgx_sample_neighbors: cap %lld < n_seeds * fanout = %lld", (long long)cap,
              (long long)(n_seeds * int64_t(fanout)));
  SampleLayout L = sample_layout(workspace, n_seeds);
  KGX_REQUIRE(workspace && workspace_bytes >= L.total, KGX_ERR_ARG,
              "kgx_sample_neighbors: workspace %zu < %zu bytes", workspace_bytes, L.total);

  KGX_CHECK_HIP(hipMemsetAsync(L.st, 0, sizeof(SampleStatus), stream));
  hipLaunchKernelGGL(sample_count_kernel, dim3(grid_for(n_seeds + 1)), dim3(kBlock), 0, stream, rowptr, n_rows,
                     seeds, n_seeds, fanout, L.cnt, L.st);
  KGX_CHECK_LAUNCH();
  size_t tb = L.tmp_bytes;
  KGX_CHECK_HIP(rocprim::exclusive_scan(L.tmp, tb, (const int32_t*)L.cnt, out_rowptr, 0, (size_t)(n_seeds + 1),
                                        rocprim::plus<int32_t>(), stream, false));
  const int64_t bound = fanout < 0 ? cap : n_seeds * int64_t(fanout);  // the most slots the emit can have
  if (bound > 0) {
    const uint64_t hs = splitmix64(seed ^ splitmix64(uint64_t(uint32_t(hop))));
    hipLaunchKernelGGL(sample_emit_kernel, dim3(grid_for(bound)), dim3(kBlock), 0, stream, rowptr, col, eid, seeds,
                       n_seeds, fanout, hs, (const int32_t*)out_rowptr, (const SampleStatus*)L.st, cap, out_src,
                       out_eid);
    KGX_CHECK_LAUNCH();
  }
  SampleStatus hs_;
  KGX_CHECK_HIP(hipMemcpyAsync(&hs_, L.st, sizeof(SampleStatus), hipMemcpyDeviceToHost, stream));
  KGX_CHECK_HIP(hipStreamSynchronize(stream));
  info[0] = int64_t(hs_.total);
  info[1] = int64_t(hs_.bad);
  info[2] = info[3] = 0;
  KGX_REQUIRE(hs_.bad == 0, KGX_ERR_INDEX, "kgx_sample_neighbors: %llu seed(s) outside [0, %lld)", hs_.bad,
              (long long)n_rows);
  KGX_REQUIRE(hs_.total <= (unsigned long long)cap, KGX_ERR_ARG,
              "kgx_sample_neighbors: %llu sampled edges do not fit cap %lld (nothing was written)", hs_.total,
              (long long)cap);
  return KGX_OK;
}

extern "C" int kgx_relabel_workspace_bytes(int64_t n_edges, int64_t n_nodes, size_t* bytes) {
  KGX_REQUIRE(bytes && n_edges >= 0 && n_edges < kInt32Limit && n_nodes >= 0 && n_nodes < kInt32Limit - 1,
              KGX_ERR_ARG, "kgx_relabel_workspace_bytes: bad arguments");
  *bytes = relabel_layout(nullptr, n_edges, n_nodes).total;
  return KGX_OK;
}

extern "C" int kgx_relabel_frontier(const int32_t* nodes, int64_t n_known, const int32_t* frontier, int64_t n_f,
                                    const int32_t* out_rowptr, const int32_t* out_src, int64_t n_edges,
                                    int32_t* map, int64_t n_nodes, int32_t* new_nodes, int32_t* src_local,
                                    int32_t* dst_local, void* workspace, size_t workspace_bytes, int64_t* info,
                                    kgx_stream_t stream_) {
  hipStream_t stream = as_stream(stream_);
  KGX_REQUIRE(n_known >= 0 && n_f >= 0 && n_edges >= 0 && n_nodes >= 0, KGX_ERR_ARG,
              "kgx_relabel_frontier: negative size");
  KGX_REQUIRE(n_nodes < kInt32Limit - 1 && n_known + n_edges < kInt32Limit, KGX_ERR_ARG,
              "kgx_relabel_frontier: n_known + n_edges = %lld does not fit int32 local ids",
              (long long)(n_known + n_edges));
  KGX_REQUIRE(n_edges == 0 || n_f > 0, KGX_ERR_ARG, "kgx_relabel_frontier: edges without a frontier row");
  if (n_known == 0 && n_edges == 0) {
    if (info) info[0] = info[1] = info[2] = info[3] = 0;
    return KGX_OK;
  }
  KGX_REQUIRE(map && info && (n_known == 0 || nodes), KGX_ERR_ARG, "kgx_relabel_frontier: null pointer");
  KGX_REQUIRE(n_edges == 0 || (frontier && out_rowptr && out_src && new_nodes && src_local && dst_local),
              KGX_ERR_ARG, "kgx_relabel_frontier: null pointer");
  RelabelLayout L = relabel_layout(workspace, n_edges, n_nodes);
  KGX_REQUIRE(workspace && workspace_bytes >= L.total, KGX_ERR_ARG,
              "kgx_relabel_frontier: workspace %zu < %zu bytes", workspace_bytes, L.total);

  KGX_CHECK_HIP(hipMemsetAsync(L.st, 0, sizeof(RelabelStatus), stream));
  const unsigned gk = grid_for(n_known), ge = grid_for(n_edges);
  if (n_known > 0) {
    hipLaunchKernelGGL(map_write_kernel, dim3(gk), dim3(kBlock), 0, stream, nodes, n_known, n_nodes, map, L.st);
    KGX_CHECK_LAUNCH();
    hipLaunchKernelGGL(map_check_kernel, dim3(gk), dim3(kBlock), 0, stream, nodes, n_known, n_nodes,
                       (const int32_t*)map, L.st);
    KGX_CHECK_LAUNCH();
  }
  if (n_edges > 0) {
    hipLaunchKernelGGL(new_keys_kernel, dim3(ge), dim3(kBlock), 0, stream, out_src, n_edges, n_nodes,
                       (const int32_t*)map, L.keys, L.st);
    KGX_CHECK_LAUNCH();
    const int end_bit = ceil_log2_u64(uint64_t(n_nodes) + 1);
    size_t tb = L.tmp_bytes;
    KGX_CHECK_HIP(rocprim::radix_sort_keys(L.tmp, tb, L.keys, L.sorted, (unsigned)n_edges, 0,
                                           end_bit > 0 ? end_bit : 1, stream, false));
    hipLaunchKernelGGL(unique_flags_kernel, dim3(ge), dim3(kBlock), 0, stream, (const uint32_t*)L.sorted, n_edges,
                       n_nodes, L.flags);
    KGX_CHECK_LAUNCH();
    tb = L.tmp_bytes;
    KGX_CHECK_HIP(rocprim::exclusive_scan(L.tmp, tb, (const int32_t*)L.flags, L.pos, 0, (size_t)n_edges,
                                          rocprim::plus<int32_t>(), stream, false));
    hipLaunchKernelGGL(select_new_kernel, dim3(ge), dim3(kBlock), 0, stream, (const uint32_t*)L.sorted,
                       (const int32_t*)L.flags, (const int32_t*)L.pos, n_edges, n_known, new_nodes, map, L.st);
    KGX_CHECK_LAUNCH();
    hipLaunchKernelGGL(local_ids_kernel, dim3(ge), dim3(kBlock), 0, stream, out_rowptr, out_src, frontier, n_f,
                       n_edges, n_nodes, (const int32_t*)map, src_local, dst_local, L.st);
    KGX_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(map_reset_kernel, dim3(grid_for(n_known + n_edges)), dim3(kBlock), 0, stream, nodes, n_known,
                     (const int32_t*)new_nodes, (const RelabelStatus*)L.st, n_nodes, map);
  KGX_CHECK_LAUNCH();
  RelabelStatus hs;
  KGX_CHECK_HIP(hipMemcpyAsync(&hs, L.st, sizeof(RelabelStatus), hipMemcpyDeviceToHost, stream));
  KGX_CHECK_HIP(hipStreamSynchronize(stream));
  info[0] = int64_t(hs.n_new);
  info[1] = int64_t(hs.dup);
  info[2] = int64_t(hs.bad);
  info[3] = 0;
  KGX_REQUIRE(hs.bad == 0, KGX_ERR_INDEX, "kgx_relabel_frontier: %llu node id(s) outside [0, %lld)", hs.bad,
              (long long)n_nodes);
  KGX_REQUIRE(hs.dup == 0, KGX_ERR_ARG, "kgx_relabel_frontier: %llu duplicate id(s) in the node list", hs.dup);
  return KGX_OK;
}
