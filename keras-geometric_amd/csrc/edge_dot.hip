// Edge scores from node rows (gfx950, wave64): the SDDMM-shaped counterpart
// of spmm.hip, for link prediction.
//
//   out[p, k] = sum_f xa[a_idx[p], f] * xb[b_idx[p, k], f]        (kgx_edge_dot)
//
// No reference counterpart.  One group of G lanes (G = pow2 >= F/VEC, <= 64)
// owns one p, as one spmm group owns one row: lane l holds columns
// (t*G + l)*VEC .. +VEC of column tile t.  The group loads its xa row into
// registers once and walks the K candidates U at a time: the U candidate
// indices are loaded, the U candidate rows are gathered with VEC-wide loads
// (all U in flight), each lane adds its products in column order with
// separately rounded multiplies and adds, and the G lane sums are folded by a
// fixed xor butterfly; lane 0 stores the U scores.  A positive with K
// candidates therefore moves (1 + K) * 4F bytes, not 2K * 4F.
//
// The lane layout (VEC, G) is chosen from F alone; rows whose address or
// leading dimension is not VEC-aligned are read with scalar loads in the same
// layout (AL = false).  So a score is a function of its two rows and F: not of
// p, k, K, P, perm, the grid size or the alignment of the tables.
//
// Every global load is unconditional on a clamped index / offset and masked
// work is skipped in the fold by a select (never by a multiply, so inf and NaN
// stay in their own pair): no load sits under a lane-dependent branch, and the
// U gathers stay in flight together (see spmm.hip's edge_block).
#include "kgx_internal.h"
#include "kgx_vec.h"

namespace kgx {
namespace {

struct DotArgs {
  const float* xa;
  const float* xb;
  int64_t ld_a, ld_b;
  int32_t n_a, n_b;
  int F;
  const int32_t* a_idx;
  const int32_t* b_idx;
  const int32_t* perm;
  int64_t P;
  int32_t K;
  float* out;
  int64_t ld_out;
  int32_t* bad;
  int G, lgG;
};

// VEC consecutive floats of a row: one VEC-wide load where the row is aligned
// for it, VEC scalar loads (same lane layout, same values) where it is not
template <int VEC, bool AL>
__device__ __forceinline__ void rload(float (&d)[VEC], const float* __restrict__ p) {
  if constexpr (AL) {
    vload<VEC>(d, p);
  } else {
#pragma unroll
    for (int k = 0; k < VEC; ++k) d[k] = p[k];
  }
}

__device__ __forceinline__ int32_t clamp_idx(int32_t v, int32_t n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// acc[u] += sum_k va[k] * vb[u][k] in column order, where the lane's columns exist
template <int U, int VEC>
__device__ __forceinline__ void fold(float (&acc)[U], const float (&va)[VEC], const float (&vb)[U][VEC], bool valid) {
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const float s = __fadd_rn(acc[u], __fmul_rn(va[k], vb[u][k]));
      acc[u] = valid ? s : acc[u];
    }
}

// WIDE: F is not exactly one column tile (G * VEC): the tiles are looped over
// into the same lane accumulators and the xa tile is re-read per candidate
// block (an L1 / L2 hit).  F == 0 takes this path with no tile and no load.
template <int VEC, bool AL, bool WIDE, int U>
__global__ __launch_bounds__(kBlock) void edge_dot_kernel(DotArgs a) {
  const int G = a.G;
  const int lane = threadIdx.x & (G - 1);
  const int64_t ngroups = (int64_t(gridDim.x) * kBlock) >> a.lgG;
  const int tile = G * VEC;
  const int fo0 = lane * VEC;
  for (int64_t p = (int64_t(blockIdx.x) * kBlock + threadIdx.x) >> a.lgG; p < a.P; p += ngroups) {
    const int32_t ia_raw = a.a_idx[p];
    const bool a_bad = ia_raw < 0 || ia_raw >= a.n_a;
    const float* ra = a.xa + row_off(clamp_idx(ia_raw, a.n_a), a.ld_a);
    int64_t orow = p;
    bool row_ok = true;
    if (a.perm) {  // group-uniform
      const int32_t q = a.perm[p];
      row_ok = q >= 0 && q < a.P;
      orow = q;
    }
    int32_t n_bad = int32_t(a_bad) + int32_t(!row_ok);

    float va[VEC];
    if constexpr (!WIDE) rload<VEC, AL>(va, ra + (fo0 < a.F ? fo0 : a.F - VEC));  // one tile: F >= VEC

    for (int32_t k0 = 0; k0 < a.K; k0 += U) {
      int32_t ib[U];
      bool bb[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {  // candidates past K: the last one again (its row is being fetched anyway)
        const int32_t kk = k0 + u < a.K ? k0 + u : a.K - 1;
        const int32_t raw = a.b_idx[p * a.K + kk];
        bb[u] = raw < 0 || raw >= a.n_b;
        ib[u] = clamp_idx(raw, a.n_b);
      }
      float acc[U];
#pragma unroll
      for (int u = 0; u < U; ++u) acc[u] = 0.0f;
      if constexpr (!WIDE) {
        const int fl = fo0 < a.F ? fo0 : a.F - VEC;
        float vb[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) rload<VEC, AL>(vb[u], a.xb + row_off(ib[u], a.ld_b) + fl);
        fold<U, VEC>(acc, va, vb, fo0 < a.F);
      } else {
        for (int c0 = 0; c0 < a.F; c0 += tile) {
          const int fo = c0 + fo0;
          const bool valid = fo < a.F;
          const int fl = valid ? fo : a.F - VEC;  // load offset, always in range (F >= VEC here)
          float vb[U][VEC];
          rload<VEC, AL>(va, ra + fl);
#pragma unroll
          for (int u = 0; u < U; ++u) rload<VEC, AL>(vb[u], a.xb + row_off(ib[u], a.ld_b) + fl);
          fold<U, VEC>(acc, va, vb, valid);
        }
      }
      // fixed xor butterfly: every lane of the group ends with the same bits
      for (int o = G >> 1; o > 0; o >>= 1) {
#pragma unroll
        for (int u = 0; u < U; ++u) acc[u] = __fadd_rn(acc[u], __shfl_xor(acc[u], o, 64));
      }
      if (lane == 0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (k0 + u < a.K) {
            n_bad += int32_t(bb[u]);
            if (row_ok) a.out[orow * a.ld_out + k0 + u] = (a_bad || bb[u]) ? __builtin_nanf("") : acc[u];
          }
        }
      }
    }
    if (lane == 0 && n_bad && a.bad) atomicAdd(a.bad, n_bad);  // status only: no score depends on it
  }
}

template <int VEC, bool AL, bool WIDE, int U>
int launch(const DotArgs& a, hipStream_t s) {
  auto kern = edge_dot_kernel<VEC, AL, WIDE, U>;
  hipLaunchKernelGGL(kern, dim3(resident_grid(kern, a.P, a.G)), dim3(kBlock), 0, s, a);
  KGX_CHECK_LAUNCH();
  return KGX_OK;
}

template <int VEC, bool AL, bool WIDE>
int launch_u(const DotArgs& a, hipStream_t s) {
  static_assert(KGX_EDGE_DOT_U == 8, "U is picked from {1, 2, 4, 8}");
  if (a.K == 1) return launch<VEC, AL, WIDE, 1>(a, s);
  if (a.K == 2) return launch<VEC, AL, WIDE, 2>(a, s);
  if (a.K <= 4) return launch<VEC, AL, WIDE, 4>(a, s);
  return launch<VEC, AL, WIDE, 8>(a, s);
}

template <int VEC, bool AL>
int launch_w(bool wide, const DotArgs& a, hipStream_t s) {
  return wide ? launch_u<VEC, AL, true>(a, s) : launch_u<VEC, AL, false>(a, s);
}

bool aligned(const void* p, int bytes) { return reinterpret_cast<uintptr_t>(p) % bytes == 0; }

constexpr int64_t kInt32Limit = int64_t(1) << 31;

}  // namespace
}  // namespace kgx

using namespace kgx;

extern "C" int kgx_edge_dot(const float* xa, int64_t n_a, int64_t ld_a, const float* xb, int64_t n_b, int64_t ld_b,
                            int64_t F, const int32_t* a_idx, const int32_t* b_idx, int64_t P, int64_t K,
                            const int32_t* perm, float* out, int64_t ld_out, int32_t* bad, kgx_stream_t stream_) {
  hipStream_t stream = as_stream(stream_);
  KGX_REQUIRE(P >= 0 && F >= 0 && n_a >= 0 && n_b >= 0, KGX_ERR_ARG,
              "kgx_edge_dot: negative size (P=%lld, F=%lld, n_a=%lld, n_b=%lld)", (long long)P, (long long)F,
              (long long)n_a, (long long)n_b);
  KGX_REQUIRE(K >= 1, KGX_ERR_ARG, "kgx_edge_dot: K must be >= 1 (got %lld)", (long long)K);
  KGX_REQUIRE(ld_a >= F && ld_b >= F, KGX_ERR_ARG, "kgx_edge_dot: leading dimension < F (ld_a=%lld, ld_b=%lld, F=%lld)",
              (long long)ld_a, (long long)ld_b, (long long)F);
  KGX_REQUIRE(ld_out >= K, KGX_ERR_ARG, "kgx_edge_dot: ld_out %lld < K %lld", (long long)ld_out, (long long)K);
  KGX_REQUIRE(K < kInt32Limit && P < kInt32Limit && P * K < kInt32Limit, KGX_ERR_ARG,
              "kgx_edge_dot: P * K = %lld * %lld does not fit int32", (long long)P, (long long)K);
  KGX_REQUIRE(ld_a < kInt32Limit && ld_b < kInt32Limit && n_a < kInt32Limit && n_b < kInt32Limit && F < kInt32Limit,
              KGX_ERR_ARG, "kgx_edge_dot: a table size or leading dimension >= 2^31");
  if (P == 0) return KGX_OK;
  // F == 0: the tables hold no bytes and are never read
  KGX_REQUIRE((F == 0 || (xa && xb)) && a_idx && b_idx && out, KGX_ERR_ARG, "kgx_edge_dot: null pointer");
  KGX_REQUIRE(n_a >= 1 && n_b >= 1, KGX_ERR_ARG, "kgx_edge_dot: an empty table cannot be indexed (n_a=%lld, n_b=%lld)",
              (long long)n_a, (long long)n_b);

  // the lane layout is a function of F alone; AL: may the rows be read VEC floats at a time?
  const int VEC = (F > 0 && F % 4 == 0) ? 4 : ((F > 0 && F % 2 == 0) ? 2 : 1);
  const bool al = ld_a % VEC == 0 && ld_b % VEC == 0 && aligned(xa, 4 * VEC) && aligned(xb, 4 * VEC);
  const int64_t fvec = F / VEC;
  const int G = int(fvec >= 64 ? 64 : next_pow2(int(fvec > 0 ? fvec : 1)));
  DotArgs a{};
  a.xa = xa;
  a.xb = xb;
  a.ld_a = ld_a;
  a.ld_b = ld_b;
  a.n_a = int32_t(n_a);
  a.n_b = int32_t(n_b);
  a.F = int(F);
  a.a_idx = a_idx;
  a.b_idx = b_idx;
  a.perm = perm;
  a.P = P;
  a.K = int32_t(K);
  a.out = out;
  a.ld_out = ld_out;
  a.bad = bad;
  a.G = G;
  a.lgG = log2i(G);
  const bool wide = F == 0 || F > int64_t(G) * VEC;
  if (VEC == 4) return al ? launch_w<4, true>(wide, a, stream) : launch_w<4, false>(wide, a, stream);
  if (VEC == 2) return al ? launch_w<2, true>(wide, a, stream) : launch_w<2, false>(wide, a, stream);
  return launch_w<1, true>(wide, a, stream);
}
