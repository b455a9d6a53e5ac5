// Device helpers shared by the MFMA kernels (the fused aggregate -> transform
// family, dense, gemm_tn): the vector types of the bf16 MFMA operands, the
// LDS-only barrier, the gathered-row address and the output epilogue.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kgx_vec.h"

namespace kgx {

// f32x4_t (accumulators) is kgx_vec.h's
typedef short bf16x8_t __attribute__((ext_vector_type(8)));
typedef short bf16x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

// Workgroup barrier for LDS hand-offs only: waits for this wave's LDS ops
// (lgkmcnt) but NOT for its outstanding global loads / stores (vmcnt), unlike
// __syncthreads(), so gathers prefetched for the next tile stay in flight.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// Source row of column c: x[c], or with TWO x2[c - n_x1] (x2b = x2 - n_x1 *
// ld_x, host address math: one 64-bit select per gathered row; a separate
// instantiation, so the one-table kernels keep their register budget).  Root
// rows (pre_gin's x_i) are always rows of x.
template <bool TWO, class Args>
__device__ __forceinline__ const float* gather_src(const Args& a, int32_t c) {
  if constexpr (TWO) return (c >= a.n_x1 ? a.x2b : a.x) + row_off(c, a.ld_x);
  return a.x + row_off(c, a.ld_x);
}

// The fused kernels' epilogue on four output columns: out (+)= v, then ReLU.
__device__ __forceinline__ void store_out4(float4* dst, float4 v, int accumulate, int relu) {
  if (accumulate) {
    const float4 p = *dst;
    v = make_float4(__fadd_rn(p.x, v.x), __fadd_rn(p.y, v.y), __fadd_rn(p.z, v.z), __fadd_rn(p.w, v.w));
  }
  if (relu) v = make_float4(fmaxf(v.x, 0.0f), fmaxf(v.y, 0.0f), fmaxf(v.z, 0.0f), fmaxf(v.w, 0.0f));
  *dst = v;
}

}  // namespace kgx
