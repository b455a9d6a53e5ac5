// k nearest neighbours within segments, without a distance table (gfx950, wave64).  No reference
// counterpart (PyG's knn / knn_graph, the graph build of DGCNN's DynamicEdgeConv).
//
//   for every query row y[i] of segment s: the k rows x[c], seg_x[s] <= c < seg_x[s + 1] (c != i with
//   exclude_self), of smallest (d2, c), ascending;  d2 NaN or +inf is never selected.
//
// Work split.  A block owns kTQ = 64 consecutive queries, wave w the 16 queries 16 w .. 16 w + 15, and
// walks the candidate range of the segments its queries lie in (seg_x[s(first)] .. seg_x[s(last) + 1]) in
// tiles that go through LDS once for all four waves.  Within a wave the scores of 16 candidates against
// 16 queries sit in the MFMA accumulator layout: lane (n, q) = (lane & 15, lane >> 4) holds query n and
// the candidates 4 q .. 4 q + 3 of the group.  Both distance paths produce that layout, so one
// selection serves both.
//
// Selection.  Every query keeps its k best (d2, index) sorted in LDS ([64][k | 1] floats and ints, owned
// by the query's wave: no barrier is needed around an insertion) and its k-th best d2 in a register of
// each of its four lanes.  The common case is one compare per score.  When any lane of the wave has a
// score below its threshold, the four q-groups take turns (the lanes of a group own distinct queries)
// and insert by shifting; then every lane rereads its threshold.  Candidates meet a query in ascending
// index order (groups ascending, q ascending, r ascending) and the compare is strict, so ties go to the
// lower index and the result is a pure function of the inputs.  No atomics.
//
// Direct path, D <= 8: acc = 0; for d ascending: t = y_d - x_d; acc = acc + t * t, every operation a
// separately rounded fp32 one (-ffp-contract=off).  The query is in registers, padded with zeros to DP =
// 4 or 8 coordinates (a zero coordinate adds +0 to a non-negative sum: the same bits); a tile is 128
// candidates [128][DP] in LDS, filled from registers that were loaded one tile ahead.
//
// MFMA path, 8 < D <= 256: d2 = max(0, (|y|^2 + |x|^2) - 2 c).  A preparation launch per operand
// writes the norms (accumulated as in the direct path) and the rows split three ways into bf16, in
// v_mfma_f32_16x16x32_bf16 fragment order: fragment (row block b, k chunk kc, plane) is 64 lanes x 16
// bytes, lane (m, q) holding row 16 b + m, k = 32 kc + 8 q .. + 7, zero outside the matrix.  The cross
// term is the six significant products (kgx_bf16x3.h), in two independent accumulator chains.  The
// wave's query fragments stay in registers (KC x 3 x 4 VGPRs); a tile is 8 / KC candidate groups = 24 KB
// of ready A operands copied linearly global -> registers -> LDS, two LDS buffers, one lds_barrier per
// tile, the next tile's loads in flight across it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "kgx_bf16x3.h"
#include "kgx_internal.h"
#include "kgx_mfma.h"

namespace kgx {
namespace {

constexpr int kTQ = 64;                 // queries per block
constexpr int kFrag = 512;              // bf16 per fragment plane (64 lanes x 8)
constexpr int kTileGroupsKC = 8;        // MFMA path: candidate groups x k chunks per tile
constexpr int kTileUnits = kTileGroupsKC * 3 * kFrag * 2 / 16;  // 16-byte units per tile (1536)
constexpr int kUnitsPerThread = kTileUnits / kBlock;            // 6
constexpr int kDirectGroups = 8;        // direct path: 16-candidate groups per tile
constexpr int kMaxK = 64, kMaxD = 256, kDirectD = 8;

struct KnnArgs {
  const float* x;
  const float* y;
  uint32_t ld_x, ld_y;
  int32_t P, Q;
  int D, k, S, exclude_self;
  const int32_t* seg_x;  // device copies, [S + 1]
  const int32_t* seg_y;
  int32_t* nbr;
  uint32_t ld_nbr;
  float* dist2;  // or null
  uint32_t ld_d;
  const short* xf;  // MFMA path: fragments [row blocks][KC][3][kFrag] and norms [16 row blocks]
  const short* yf;
  const float* nx;
  const float* ny;
};

// The segment of row i: the last s with seg[s] <= i (empty segments before it are passed over).
__device__ __forceinline__ int seg_of(const int32_t* seg, int S, int32_t i) {
  int lo = 0, hi = S;  // invariant: seg[lo] <= i < seg[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (seg[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// One thread per (row block, k chunk, lane): the norms of the block's rows (kc == 0, lanes 0..15) and the
// lane's eight values split into the three planes.
__global__ __launch_bounds__(kBlock) void knn_prep_kernel(const float* src, uint32_t ld, int32_t n, int D, int KC,
                                                           int64_t n_frag, short* frag, float* norm) {
  const int64_t idx = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  const int64_t f = idx >> 6;
  if (f >= n_frag) return;
  const int lane = int(idx & 63), m = lane & 15, q = lane >> 4;
  const int kc = int(f % KC);
  const int32_t row = int32_t(f / KC) * 16 + m;
  const float* r = src + row_off(row < n ? row : 0, ld);
  if (kc == 0 && q == 0) {
    float acc = 0.0f;
    if (row < n)
      for (int d = 0; d < D; ++d) acc = __fadd_rn(acc, __fmul_rn(r[d], r[d]));
    norm[row] = acc;
  }
  uint32_t h[4], mi[4], l[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k0 = kc * 32 + 8 * q + 2 * i;
    const float v0 = (row < n && k0 < D) ? r[k0] : 0.0f;
    const float v1 = (row < n && k0 + 1 < D) ? r[k0 + 1] : 0.0f;
    split3_pair(v0, v1, h[i], mi[i], l[i]);
  }
  short* o = frag + f * 3 * kFrag + lane * 8;
  *reinterpret_cast<u32x4_t*>(o) = u32x4_t{h[0], h[1], h[2], h[3]};
  *reinterpret_cast<u32x4_t*>(o + kFrag) = u32x4_t{mi[0], mi[1], mi[2], mi[3]};
  *reinterpret_cast<u32x4_t*>(o + 2 * kFrag) = u32x4_t{l[0], l[1], l[2], l[3]};
}

// What a lane knows about its query, and the wave-uniform ranges that let a candidate group skip the masks.
struct Sel {
  float* ld;    // the query's sorted d2 [k]
  int32_t* li;  // and indices
  float thr;    // the k-th best d2 (ld[k - 1])
  int32_t lo, hi, self;     // the query's candidate range; its own index with exclude_self, else -1
  int32_t in_lo, in_hi;     // wave-uniform: a group inside [in_lo, in_hi) is inside every query's range
  int32_t w_lo, w_hi;       // wave-uniform: the union of the wave's ranges
  int32_t self_lo, self_hi; // wave-uniform: the wave's own query indices with exclude_self, else empty
  int k, q;
};

// LDS operations of one wave execute in order; this keeps the compiler from moving them across.
__device__ __forceinline__ void wave_lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// The scores s[r] of candidates c0 + r (r < 4) against this lane's query.
__device__ __forceinline__ void select4(Sel& z, float (&s)[4], int32_t g0, int32_t c0) {
  const bool plain = g0 >= z.in_lo && g0 + 16 <= z.in_hi && (g0 + 16 <= z.self_lo || g0 >= z.self_hi);
  if (!plain) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int32_t c = c0 + r;
      if (c < z.lo || c >= z.hi || c == z.self) s[r] = __builtin_inff();
    }
  }
  const bool hit = s[0] < z.thr || s[1] < z.thr || s[2] < z.thr || s[3] < z.thr;
  if (__builtin_amdgcn_ballot_w64(hit) == 0) return;
  for (int qq = 0; qq < 4; ++qq) {
    if (z.q == qq && hit) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = s[r];
        if (v < z.ld[z.k - 1]) {  // false for NaN and +inf
          int j = z.k - 1;
          while (j > 0 && z.ld[j - 1] > v) {
            z.ld[j] = z.ld[j - 1];
            z.li[j] = z.li[j - 1];
            --j;
          }
          z.ld[j] = v;
          z.li[j] = c0 + r;
        }
      }
    }
    wave_lds_fence();
  }
  z.thr = z.ld[z.k - 1];
}

// KC > 0: the MFMA path with KC k chunks (D <= 32 KC).  KC == 0: the direct path with DP coordinates.
template <int KC, int DP>
__global__ __launch_bounds__(kBlock, 2) void knn_kernel(KnnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr bool kMfma = KC > 0;
  constexpr int TCB = kMfma ? kTileGroupsKC / (kMfma ? KC : 1) : kDirectGroups;  // 16-candidate groups per tile
  constexpr int kBufBytes = kMfma ? kTileUnits * 16 + TCB * 16 * 4 : TCB * 16 * DP * 4;
  constexpr int NPRE = kMfma ? kUnitsPerThread : TCB * 16 * DP / kBlock;

  const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, q = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ks = a.k | 1;  // list stride: odd, so the 16 queries of a group fall on distinct banks
  float* list_d = reinterpret_cast<float*>(smem);
  int32_t* list_i = reinterpret_cast<int32_t*>(smem) + kTQ * ks;
  char* bufs = smem + size_t(2) * kTQ * ks * 4;  // 2 x kBufBytes (kTQ * ks * 8 is a multiple of 16: kTQ = 64)

  for (int j = tid; j < kTQ * ks; j += kBlock) {
    list_d[j] = __builtin_inff();
    list_i[j] = -1;
  }

  // ranges: the block's, the wave's and the lane's
  const int32_t q0 = int32_t(blockIdx.x) * kTQ;
  const int32_t qlast = min(q0 + kTQ - 1, a.Q - 1);
  const int32_t wfirst = q0 + 16 * wave, wlast = min(wfirst + 15, a.Q - 1);
  const bool wave_ok = wfirst < a.Q;
  const int32_t qi = wfirst + n;
  const int32_t c_lo = a.seg_x[seg_of(a.seg_y, a.S, q0)], c_hi = a.seg_x[seg_of(a.seg_y, a.S, qlast) + 1];

  Sel z;
  z.ld = list_d + (16 * wave + n) * ks;
  z.li = list_i + (16 * wave + n) * ks;
  z.thr = __builtin_inff();
  z.k = a.k, z.q = q;
  z.lo = z.hi = 0, z.self = -1;
  z.in_lo = z.in_hi = z.w_lo = z.w_hi = 0;
  z.self_lo = z.self_hi = -1;
  if (wave_ok) {
    const int sf = seg_of(a.seg_y, a.S, wfirst), sl = seg_of(a.seg_y, a.S, wlast);
    z.w_lo = a.seg_x[sf], z.in_hi = a.seg_x[sf + 1];
    z.in_lo = a.seg_x[sl], z.w_hi = a.seg_x[sl + 1];
    if (a.exclude_self) z.self_lo = wfirst, z.self_hi = wfirst + 16;
    if (qi < a.Q) {
      const int s = seg_of(a.seg_y, a.S, qi);
      z.lo = a.seg_x[s], z.hi = a.seg_x[s + 1];
      if (a.exclude_self) z.self = qi;
    }
  }

  // tiles: groups of 16 candidates from g_base on (the MFMA path's groups are the fragments' row blocks)
  const int32_t g_base = kMfma ? (c_lo & ~15) : c_lo;
  const int32_t n_groups = c_hi > g_base ? (c_hi - g_base + 15) / 16 : 0;
  const int n_tiles = (n_groups + TCB - 1) / TCB;

  // the query: fragments and norm (MFMA), coordinates (direct)
  [[maybe_unused]] bf16x8_t yh[kMfma ? KC : 1], ym[kMfma ? KC : 1], yl[kMfma ? KC : 1];
  [[maybe_unused]] float ynorm = 0.0f;
  [[maybe_unused]] float yv[DP];
  if constexpr (kMfma) {
    const int64_t qb = int64_t(blockIdx.x) * (kTQ / 16) + wave;
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) {
      if (wave_ok) {
        const short* f = a.yf + ((qb * KC + kc) * 3) * kFrag + lane * 8;
        yh[kc] = *reinterpret_cast<const bf16x8_t*>(f);
        ym[kc] = *reinterpret_cast<const bf16x8_t*>(f + kFrag);
        yl[kc] = *reinterpret_cast<const bf16x8_t*>(f + 2 * kFrag);
      } else {
        yh[kc] = ym[kc] = yl[kc] = bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0};
      }
    }
    if (wave_ok) ynorm = a.ny[qb * 16 + n];
  } else {
#pragma unroll
    for (int d = 0; d < DP; ++d) yv[d] = (qi < a.Q && d < a.D) ? a.y[row_off(qi, a.ld_y) + d] : 0.0f;
  }

  // a tile's global loads into registers; rows and groups past the block's range load nothing (zeros)
  [[maybe_unused]] u32x4_t pre[kMfma ? NPRE : 1];
  [[maybe_unused]] f32x4_t pre_n = {0.0f, 0.0f, 0.0f, 0.0f};
  [[maybe_unused]] float pre_c[kMfma ? 1 : NPRE];
  auto load_tile = [&](int t) {
    if constexpr (kMfma) {
      const int64_t gb = int64_t(g_base >> 4) + int64_t(t) * TCB;  // the tile's first row block
      const int32_t left = n_groups - t * TCB;                     // groups of the tile that exist
      const u32x4_t* src = reinterpret_cast<const u32x4_t*>(a.xf + gb * KC * 3 * kFrag);
#pragma unroll
      for (int j = 0; j < NPRE; ++j) {
        const int u = j * kBlock + tid;
        pre[j] = (u / (KC * 192) < left) ? src[u] : u32x4_t{0, 0, 0, 0};  // 192 units per (group, k chunk)
      }
      if (tid < TCB * 4 && (tid >> 2) < left) pre_n = *reinterpret_cast<const f32x4_t*>(a.nx + gb * 16 + 4 * tid);
    } else {
      const int32_t c_t = g_base + t * TCB * 16;
#pragma unroll
      for (int j = 0; j < NPRE; ++j) {
        const int e = j * kBlock + tid;
        const int32_t c = c_t + e / DP;
        const int d = e % DP;
        pre_c[j] = (c < c_hi && d < a.D) ? a.x[row_off(c, a.ld_x) + d] : 0.0f;
      }
    }
  };
  auto store_tile = [&](int t) {
    char* b = bufs + (t & 1) * kBufBytes;
    if constexpr (kMfma) {
#pragma unroll
      for (int j = 0; j < NPRE; ++j) reinterpret_cast<u32x4_t*>(b)[j * kBlock + tid] = pre[j];
      if (tid < TCB * 4) reinterpret_cast<f32x4_t*>(b + kTileUnits * 16)[tid] = pre_n;
    } else {
#pragma unroll
      for (int j = 0; j < NPRE; ++j) reinterpret_cast<float*>(b)[j * kBlock + tid] = pre_c[j];
    }
  };

  if (n_tiles > 0) {
    load_tile(0);
    store_tile(0);
  }
  for (int t = 0; t < n_tiles; ++t) {
    if (t + 1 < n_tiles) load_tile(t + 1);  // in flight across the barrier and the scoring
    lds_barrier();  // tile t is in LDS (and, at t == 0, the lists are initialised); tile t - 1 has been read
    const char* b = bufs + (t & 1) * kBufBytes;
#pragma unroll 1
    for (int g = 0; g < TCB; ++g) {
      const int32_t gi = t * TCB + g, g0 = g_base + gi * 16;
      if (gi >= n_groups || !wave_ok || g0 + 16 <= z.w_lo || g0 >= z.w_hi) continue;  // wave-uniform
      float s[4];
      if constexpr (kMfma) {
        f32x4_t c1 = {0.0f, 0.0f, 0.0f, 0.0f}, c2 = {0.0f, 0.0f, 0.0f, 0.0f};
        const short* xa = reinterpret_cast<const short*>(b) + g * KC * 3 * kFrag + lane * 8;
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) {
          const bf16x8_t xh = *reinterpret_cast<const bf16x8_t*>(xa + kc * 3 * kFrag);
          const bf16x8_t xm = *reinterpret_cast<const bf16x8_t*>(xa + kc * 3 * kFrag + kFrag);
          const bf16x8_t xl = *reinterpret_cast<const bf16x8_t*>(xa + kc * 3 * kFrag + 2 * kFrag);
          c1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, yl[kc], c1, 0, 0, 0);  // the small terms
          c2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, ym[kc], c2, 0, 0, 0);
          c1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xl, yh[kc], c1, 0, 0, 0);
          c2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xm, yh[kc], c2, 0, 0, 0);
          c1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xm, ym[kc], c1, 0, 0, 0);
          c2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, yh[kc], c2, 0, 0, 0);
        }
        const f32x4_t xn = reinterpret_cast<const f32x4_t*>(b + kTileUnits * 16)[g * 4 + q];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float c = __fadd_rn(c1[r], c2[r]);
          const float d = __fsub_rn(__fadd_rn(ynorm, xn[r]), __fmul_rn(2.0f, c));
          s[r] = d < 0.0f ? 0.0f : d;  // NaN stays NaN
        }
      } else {
        const f32x4_t* xr = reinterpret_cast<const f32x4_t*>(b) + (g * 16 + 4 * q) * (DP / 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float acc = 0.0f;
#pragma unroll
          for (int v = 0; v < DP / 4; ++v) {
            const f32x4_t xc = xr[r * (DP / 4) + v];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float df = __fsub_rn(yv[4 * v + e], xc[e]);
              acc = __fadd_rn(acc, __fmul_rn(df, df));
            }
          }
          s[r] = acc;
        }
      }
      select4(z, s, g0, g0 + 4 * q);
    }
    if (t + 1 < n_tiles) store_tile(t + 1);  // into the buffer tile t - 1 was read from, before barrier t
  }
  if (n_tiles == 0) lds_barrier();  // the lists' initial values
  wave_lds_fence();

  // the wave's 16 lists, k entries each
  if (!wave_ok) return;
  for (int j = lane; j < 16 * a.k; j += 64) {
    const int qq = j / a.k, jj = j - qq * a.k;
    const int32_t row = wfirst + qq;
    if (row >= a.Q) break;
    const int src = (16 * wave + qq) * ks + jj;
    a.nbr[row_off(row, a.ld_nbr) + jj] = list_i[src];
    if (a.dist2) a.dist2[row_off(row, a.ld_d) + jj] = list_d[src];
  }
}

constexpr int64_t kInt32Limit = int64_t(1) << 31;
constexpr int64_t kRowLimit = kInt32Limit - 64;  // row indices plus a tile stay in int32

inline int k_chunks(int64_t D) { return D <= 32 ? 1 : (D <= 64 ? 2 : (D <= 128 ? 4 : 8)); }
inline int64_t row_blocks(int64_t n) { return (n + 15) / 16; }
inline size_t frag_bytes(int64_t n, int64_t D) {
  return align_up(size_t(row_blocks(n)) * k_chunks(D) * 3 * kFrag * sizeof(short), 256);
}
inline size_t norm_bytes(int64_t n) { return align_up(size_t(row_blocks(n)) * 16 * sizeof(float), 256); }
inline size_t seg_bytes(int64_t S) { return align_up(size_t(S + 1) * sizeof(int32_t), 256); }

size_t workspace_bytes(int64_t P, int64_t Q, int64_t D, int64_t S) {
  size_t b = 2 * seg_bytes(S);
  if (D > kDirectD) b += frag_bytes(P, D) + frag_bytes(Q, D) + norm_bytes(P) + norm_bytes(Q);
  return b;
}

bool offsets_ok(const int32_t* seg, int64_t S, int64_t n) {
  if (seg[0] != 0 || seg[S] != n) return false;
  for (int64_t s = 0; s < S; ++s)
    if (seg[s] > seg[s + 1]) return false;
  return true;
}

template <int KC, int DP>
int launch(const KnnArgs& a, hipStream_t s) {
  constexpr int TCB = KC > 0 ? kTileGroupsKC / (KC > 0 ? KC : 1) : kDirectGroups;
  constexpr size_t buf = KC > 0 ? kTileUnits * 16 + TCB * 16 * 4 : TCB * 16 * DP * 4;
  const size_t lds = size_t(2) * kTQ * (a.k | 1) * 4 + 2 * buf;  // at most 33 + 50 KB
  if (lds > 48 * 1024)
    KGX_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&knn_kernel<KC, DP>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
  hipLaunchKernelGGL((knn_kernel<KC, DP>), dim3(unsigned((a.Q + kTQ - 1) / kTQ)), dim3(kBlock), lds, s, a);
  KGX_CHECK_LAUNCH();
  return KGX_OK;
}

int launch_prep(const float* src, uint32_t ld, int32_t n, int D, short* frag, float* norm, hipStream_t s) {
  const int KC = k_chunks(D);
  const int64_t n_frag = row_blocks(n) * KC;
  hipLaunchKernelGGL(knn_prep_kernel, dim3(unsigned((n_frag * 64 + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, src, ld, n,
                     D, KC, n_frag, frag, norm);
  KGX_CHECK_LAUNCH();
  return KGX_OK;
}

}  // namespace
}  // namespace kgx

using namespace kgx;

extern "C" int kgx_knn_workspace_bytes(int64_t P, int64_t Q, int64_t D, int64_t S, size_t* bytes) {
  KGX_REQUIRE(bytes && P >= 0 && P < kRowLimit && Q >= 0 && Q < kRowLimit && S >= 1 && S < kInt32Limit, KGX_ERR_ARG,
              "kgx_knn_workspace_bytes: P = %lld, Q = %lld (each in [0, 2^31 - 64)), S = %lld (>= 1)", (long long)P,
              (long long)Q, (long long)S);
  KGX_REQUIRE(D >= 1 && D <= kMaxD, KGX_ERR_ARG, "kgx_knn_workspace_bytes: D = %lld outside [1, %d]", (long long)D, kMaxD);
  *bytes = workspace_bytes(P, Q, D, S);
  return KGX_OK;
}

extern "C" int kgx_knn(const kgx_knn_args* p, kgx_stream_t stream_) {
  KGX_REQUIRE(p && p->struct_size == sizeof(kgx_knn_args), KGX_ERR_ARG, "kgx_knn: struct_size %llu is not this header's %zu",
              p ? (unsigned long long)p->struct_size : 0ull, sizeof(kgx_knn_args));
  const char* fn = "kgx_knn";
  KGX_REQUIRE(p->k >= 1 && p->k <= kMaxK, KGX_ERR_ARG, "%s: k = %lld outside [1, %d]", fn, (long long)p->k, kMaxK);
  KGX_REQUIRE(p->D >= 1 && p->D <= kMaxD, KGX_ERR_ARG, "%s: D = %lld outside [1, %d]", fn, (long long)p->D, kMaxD);
  KGX_REQUIRE(p->P >= 0 && p->P < kRowLimit && p->Q >= 0 && p->Q < kRowLimit && p->S >= 1 && p->S < kInt32Limit,
              KGX_ERR_ARG, "%s: P = %lld, Q = %lld (each in [0, 2^31 - 64)), S = %lld (>= 1)", fn, (long long)p->P,
              (long long)p->Q, (long long)p->S);
  KGX_REQUIRE(p->Q * p->k < kInt32Limit, KGX_ERR_ARG, "%s: Q k = %lld >= 2^31", fn, (long long)(p->Q * p->k));
  KGX_REQUIRE(p->ld_x >= p->D && p->ld_y >= p->D && p->ld_nbr >= p->k && (!p->dist2 || p->ld_dist2 >= p->k) &&
                  p->ld_x < kInt32Limit && p->ld_y < kInt32Limit && p->ld_nbr < kInt32Limit && p->ld_dist2 < kInt32Limit,
              KGX_ERR_ARG, "%s: a leading dimension below its width or >= 2^31 (ld_x %lld, ld_y %lld, ld_nbr %lld, ld_dist2 %lld)",
              fn, (long long)p->ld_x, (long long)p->ld_y, (long long)p->ld_nbr, (long long)p->ld_dist2);
  KGX_REQUIRE(p->seg_x && p->seg_y, KGX_ERR_ARG, "%s: null pointer (seg_x, seg_y)", fn);
  KGX_REQUIRE(offsets_ok(p->seg_x, p->S, p->P) && offsets_ok(p->seg_y, p->S, p->Q), KGX_ERR_ARG,
              "%s: seg_x / seg_y must ascend from 0 to P / Q", fn);
  KGX_REQUIRE(!p->exclude_self || p->Q <= p->P, KGX_ERR_ARG, "%s: exclude_self with more queries than points", fn);
  if (p->Q == 0) return KGX_OK;  // nothing to write: x, y and nbr may be null
  KGX_REQUIRE(p->nbr && p->y && (p->x || p->P == 0), KGX_ERR_ARG, "%s: null pointer (x, y, nbr)", fn);
  const size_t need = workspace_bytes(p->P, p->Q, p->D, p->S);
  KGX_REQUIRE(p->workspace && reinterpret_cast<uintptr_t>(p->workspace) % 16 == 0 && p->workspace_bytes >= need, KGX_ERR_ARG,
              "%s: workspace of %llu bytes, needs %zu (16-byte aligned)", fn, (unsigned long long)p->workspace_bytes, need);
  hipStream_t stream = as_stream(stream_);

  KnnArgs a{};
  a.x = p->x, a.y = p->y, a.ld_x = uint32_t(p->ld_x), a.ld_y = uint32_t(p->ld_y);
  a.P = int32_t(p->P), a.Q = int32_t(p->Q), a.D = int(p->D), a.k = int(p->k), a.S = int(p->S);
  a.exclude_self = p->exclude_self != 0;
  a.nbr = p->nbr, a.ld_nbr = uint32_t(p->ld_nbr), a.dist2 = p->dist2, a.ld_d = uint32_t(p->ld_dist2);

  char* w = static_cast<char*>(p->workspace);
  const size_t sb = size_t(p->S + 1) * sizeof(int32_t);
  // One copy for both arrays.  Its source is pageable, so the runtime has consumed it when the call returns (and
  // has waited for the stream: kgx.h says so); knn_graph's shared array goes as it is, two arrays are packed first.
  a.seg_x = reinterpret_cast<const int32_t*>(w);
  if (p->seg_y == p->seg_x) {
    KGX_CHECK_HIP(hipMemcpyAsync(w, p->seg_x, sb, hipMemcpyHostToDevice, stream));
    a.seg_y = a.seg_x;
  } else {
    const size_t n = size_t(p->S + 1);
    std::vector<int32_t> both(2 * n);
    std::copy(p->seg_x, p->seg_x + n, both.begin());
    std::copy(p->seg_y, p->seg_y + n, both.begin() + n);
    KGX_CHECK_HIP(hipMemcpyAsync(w, both.data(), 2 * sb, hipMemcpyHostToDevice, stream));
    a.seg_y = a.seg_x + n;
  }
  w += 2 * seg_bytes(p->S);

  if (a.D <= kDirectD) return a.D <= 4 ? launch<0, 4>(a, stream) : launch<0, 8>(a, stream);

  short* xf = reinterpret_cast<short*>(w);
  float* nx = reinterpret_cast<float*>(w + frag_bytes(p->P, p->D));
  w += frag_bytes(p->P, p->D) + norm_bytes(p->P);
  if (p->P > 0)
    if (const int rc = launch_prep(a.x, a.ld_x, a.P, a.D, xf, nx, stream); rc != KGX_OK) return rc;
  a.xf = xf, a.nx = nx;
  if (p->y == p->x && p->ld_y == p->ld_x && p->Q == p->P) {
    a.yf = xf, a.ny = nx;  // knn_graph: one preparation serves both operands
  } else {
    short* yf = reinterpret_cast<short*>(w);
    float* ny = reinterpret_cast<float*>(w + frag_bytes(p->Q, p->D));
    if (const int rc = launch_prep(a.y, a.ld_y, a.Q, a.D, yf, ny, stream); rc != KGX_OK) return rc;
    a.yf = yf, a.ny = ny;
  }
  switch (k_chunks(a.D)) {
    case 1: return launch<1, 4>(a, stream);
    case 2: return launch<2, 4>(a, stream);
    case 4: return launch<4, 4>(a, stream);
    default: return launch<8, 4>(a, stream);
  }
}
