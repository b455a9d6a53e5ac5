// Shared by the aggregate-then-transform tile kernels (rgcn.hip, nnconv.hip): the weight planes split
// three ways into bf16 and stored in MFMA fragment order, the six-product MFMA, the split of gathered
// sums, and the fix-up that adds the partial rows of a node cut into several pieces.
//
// Fragment (p, kc, cb, plane) of a stack of [F_in, F_out] weight planes is 64 lanes x 16 bytes, lane
// (m, q) holding column 16 cb + m, k = 32 kc + 8 q .. + 7 (zero outside the matrix), so a tile reads
// ready A operands of v_mfma_f32_16x16x32_bf16 and never splits a weight.
#pragma once

#include <hip/hip_runtime.h>

#include "kgx_bf16x3.h"
#include "kgx_internal.h"
#include "kgx_mfma.h"

namespace kgx {
namespace wfrag {

constexpr int kFrag = 512;  // bf16 per fragment plane (64 lanes x 8)
constexpr int kFixB = 8;    // partial rows loaded together by the fix-up

struct Planes {
  bf16x8_t h, m, l;
};

__device__ __forceinline__ Planes split8(const float (&v)[8]) {
  uint32_t h[4], m[4], l[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) split3_pair(v[2 * i], v[2 * i + 1], h[i], m[i], l[i]);
  Planes p;
  p.h = __builtin_bit_cast(bf16x8_t, (u32x4_t{h[0], h[1], h[2], h[3]}));
  p.m = __builtin_bit_cast(bf16x8_t, (u32x4_t{m[0], m[1], m[2], m[3]}));
  p.l = __builtin_bit_cast(bf16x8_t, (u32x4_t{l[0], l[1], l[2], l[3]}));
  return p;
}

// the six significant products, small terms first; W (split3_a) is the A operand, the sums (split3_a_lo on
// the rare path: a non-finite value sits in the lo plane) the B operand, so lo meets only W's hi plane
__device__ __forceinline__ f32x4_t mfma6(const Planes& W, const Planes& S, f32x4_t d) {
  d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(W.h, S.l, d, 0, 0, 0);
  d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(W.l, S.h, d, 0, 0, 0);
  d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(W.m, S.m, d, 0, 0, 0);
  d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(W.h, S.m, d, 0, 0, 0);
  d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(W.m, S.h, d, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(W.h, S.h, d, 0, 0, 0);
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ bf16x8_t ld8(const short* p) { return *reinterpret_cast<const bf16x8_t*>(p); }

// four sums -> three packed planes (two words each); the fast split unless a value is non-finite or huge
__device__ __forceinline__ void split4(float4 s, uint32_t (&h)[2], uint32_t (&m)[2], uint32_t (&l)[2]) {
  if (split_fast_ok(s.x, s.y, s.z, s.w)) {
    split3_pair(s.x, s.y, h[0], m[0], l[0]);
    split3_pair(s.z, s.w, h[1], m[1], l[1]);
  } else {
    const float v[4] = {s.x, s.y, s.z, s.w};
    short hh[4], mm[4], ll[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) split3_a_lo(v[i], hh[i], mm[i], ll[i]);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      h[i] = uint32_t(uint16_t(hh[2 * i])) | (uint32_t(uint16_t(hh[2 * i + 1])) << 16);
      m[i] = uint32_t(uint16_t(mm[2 * i])) | (uint32_t(uint16_t(mm[2 * i + 1])) << 16);
      l[i] = uint32_t(uint16_t(ll[2 * i])) | (uint32_t(uint16_t(ll[2 * i + 1])) << 16);
    }
  }
}

// R stacked planes W [R][F_in][F_out] (contiguous), then up to two single planes; a null plane keeps its
// fragment slot, which is then never read.
struct PrepArgs {
  const float* W;
  const float* extra[2];
  int R, n_extra, F_in, F_out, KC, NCB;
  short* wf;  // [(R + n_extra) KC NCB][3][kFrag]
};

// One thread per (plane, k chunk, column block, lane): its 8 weights, split, 16 bytes into each bf16 plane.
static __global__ __launch_bounds__(kBlock) void prep_kernel(PrepArgs a) {
  const int64_t idx = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  const int64_t n_frag = int64_t(a.R + a.n_extra) * a.KC * a.NCB;
  const int64_t frag = idx >> 6;
  if (frag >= n_frag) return;
  const int lane = int(idx & 63), m = lane & 15, q = lane >> 4;
  const int cb = int(frag % a.NCB), kc = int((frag / a.NCB) % a.KC), r = int(frag / (int64_t(a.NCB) * a.KC));
  const float* W = r < a.R ? a.W + int64_t(r) * a.F_in * a.F_out : a.extra[r - a.R];
  if (!W) return;
  const int c = cb * 16 + m;
  float v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int k = kc * 32 + 8 * q + i;
    v[i] = (c < a.F_out && k < a.F_in) ? W[int64_t(k) * a.F_out + c] : 0.0f;
  }
  const Planes p = split8(v);
  short* f = a.wf + frag * 3 * kFrag + lane * 8;
  *reinterpret_cast<bf16x8_t*>(f) = p.h;
  *reinterpret_cast<bf16x8_t*>(f + kFrag) = p.m;
  *reinterpret_cast<bf16x8_t*>(f + 2 * kFrag) = p.l;
}

// A wave per split piece that is its node's first: the node's partial rows, added in piece order.
static __global__ __launch_bounds__(kBlock) void fixup_kernel(const int32_t* pieces, int64_t n_split, int F_out,
                                                              const float* part, float* out, uint32_t ld_o) {
  const int lane = threadIdx.x & 63;
  const int64_t wid = (int64_t(blockIdx.x) * kBlock + threadIdx.x) >> 6, n_waves = (int64_t(gridDim.x) * kBlock) >> 6;
  for (int64_t p = wid; p < n_split; p += n_waves) {  // wave-uniform
    const int32_t node = pieces[p * 3];
    if (p > 0 && pieces[(p - 1) * 3] == node) continue;
    int64_t k = 1;
    while (p + k < n_split && pieces[(p + k) * 3] == node) ++k;
    for (int c = 4 * lane; c < F_out; c += 256) {
      float4 s = ld4(part + p * F_out + c);
      for (int64_t k0 = 1; k0 < k; k0 += kFixB) {
        float4 v[kFixB];
#pragma unroll
        for (int u = 0; u < kFixB; ++u) {  // clamped, unconditional: all in flight together
          const int64_t t = k0 + u < k ? k0 + u : k - 1;
          v[u] = ld4(part + (p + t) * F_out + c);
        }
#pragma unroll
        for (int u = 0; u < kFixB; ++u) {
          const bool ok = k0 + u < k;
          s.x = ok ? __fadd_rn(s.x, v[u].x) : s.x;
          s.y = ok ? __fadd_rn(s.y, v[u].y) : s.y;
          s.z = ok ? __fadd_rn(s.z, v[u].z) : s.z;
          s.w = ok ? __fadd_rn(s.w, v[u].w) : s.w;
        }
      }
      *reinterpret_cast<float4*>(out + row_off(node, ld_o) + c) = s;
    }
  }
}

inline int k_chunks(int64_t F_in) { return int((F_in + 31) / 32); }
inline int col_blocks(int64_t F_out) { return int((F_out + 15) / 16); }
inline size_t frag_bytes(int64_t n_planes, int64_t F_in, int64_t F_out) {
  return align_up(size_t(n_planes) * k_chunks(F_in) * col_blocks(F_out) * 3 * kFrag * sizeof(short), 256);
}
inline bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

inline int launch_prep(const PrepArgs& w, hipStream_t stream) {
  const int64_t threads = int64_t(w.R + w.n_extra) * w.KC * w.NCB * 64;
  hipLaunchKernelGGL(prep_kernel, dim3(unsigned((threads + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, w);
  KGX_CHECK_LAUNCH();
  return KGX_OK;
}

inline int launch_fixup(const int32_t* pieces, int64_t n_split, int F_out, const float* part, float* out, uint32_t ld_o,
                        hipStream_t stream) {
  hipLaunchKernelGGL(fixup_kernel, dim3(grid_for(n_split * 64)), dim3(kBlock), 0, stream, pieces, n_split, F_out, part,
                     out, ld_o);
  KGX_CHECK_LAUNCH();
  return KGX_OK;
}

}  // namespace wfrag
}  // namespace kgx
