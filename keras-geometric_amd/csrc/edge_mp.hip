// Edge-feature messages summed per row (gfx950, wave64): GINE's
//
//   out[i] = sum_{t in row i} relu(x[col t] + eps_t)  (+ gin_scale * xroot[i])
//   eps_t  = a[eid t] W_e + b_e   (PROJ: a [n_e, D <= 32], projected in the kernel)
//          = a[eid t]             (plain: a [n_e, F])
//
// and its backward over the transposed CSR.  No reference counterpart.
//
// Slot-parallel, unlike spmm.hip's row-owned lanes: a wave owns SPANS of 64
// consecutive CSR slots (four tiles of 16) of one 64-column group (blockIdx.y),
// so its load never depends on a degree.  Per tile and 16-column block:
//   * eps^T = W_e^T a^T on v_mfma_f32_16x16x32_bf16 (K = D padded to 32), both
//     operands split into three bf16 planes and the six significant products
//     taken (kgx_bf16x3.h): A = W_e's fragment of the block, split once per
//     wave and kept in registers, B = the tile's 16 attribute rows.  In the
//     transposed product lane (m, q) holds slot m, columns 4q..4q+3: it adds
//     b_e and ONE float4 of x[col] (the four q lanes of a slot read 64
//     contiguous bytes of the row), applies relu and writes its float4 to a
//     wave-local LDS tile [16 slots][64 columns].
//   * lane l then owns column l and walks the 16 slots in CSR order (the row of
//     every slot comes from the graph's row-of-slot array, wave-uniform), one
//     sequential sum per row, carried across tiles in a register.
// A row wholly inside a span is stored with its epilogue.  A row shared with
// the previous span leaves its partial in part[span][0], one shared with the
// next span in part[span][1]; gine_fixup_kernel finds those rows (and the empty
// ones) from rowptr alone and adds a row's partials in span order.  One writer
// per element, no atomics.
//
// Backward (BWD): the same walk over the transposed CSR (row = source j).  A
// slot recomputes z = x[j] + eps exactly as the forward did, gathers gout[dst],
// forms dz = gout * [z > 0] and segment-sums grad_x[j].  Plain: the slot's dz row
// is grad_a[eid].  PROJ: the tile's dz (from the LDS tile) and attribute rows,
// both split, feed dW_e^T += dz^T a (K = the 16 slots padded to 32) into
// per-wave accumulators, the column sums of dz ride along in the walk, every
// wave stores its partial and gine_finish_kernel adds them in wave order.
//
// LDS is wave-local (no s_barrier anywhere): a wave's LDS ops retire in order,
// so a wait on lgkmcnt after the tile is written is the whole hand-off, and
// global loads stay in flight across it.
#include <hip/hip_runtime.h>

// No packed f32 VALU (v_pk_add_f32 and kin) in this file: the feature is taken off every function of the
// device pass, the shared helpers included (a helper without it is not inlined into a kernel with it), so
// the host pass never sees it.  The Makefile adds -fno-slp-vectorize, as for gatv2 and dense.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#include "kgx_bf16x3.h"
#include "kgx_internal.h"
#include "kgx_mfma.h"

namespace kgx {
namespace {

constexpr int kSpan = 64;        // slots per span
constexpr int kTile = 16;        // slots per MFMA tile
constexpr int kCols = 64;        // columns per wave (blockIdx.y)
constexpr int kCB = kCols / 16;  // 16-column blocks per wave
constexpr int kLd = kCols + 4;   // LDS tile row stride (floats): 16-byte aligned rows, 4 banks apart
constexpr int kWaves = kBlock / 64;
constexpr int kFixB = 8;         // span partials loaded together by the fix-up
constexpr int kGridCap = 1024;   // blocks of the span kernel (x * y): 4 per CU
constexpr int kFinJ = 16;        // the finish kernel cuts the wave list into 16 runs,
constexpr int kFinU = 8;         // each added with 8 loads in flight

struct SpanArgs {
  const float* x;
  uint32_t ld_x;  // < 2^31 (checked at the entry points)
  const int32_t* xidx;   // per slot: row of x
  const int32_t* rowid;  // per slot: the row it is summed into
  const int32_t* eidx;   // per slot: row of a (null: the slot itself)
  const float* a;
  uint32_t ld_a;  // < 2^31 (checked at the entry points)
  const float* W;
  uint32_t ld_w;  // < 2^31 (checked at the entry points)
  const float* b;
  int D, F;
  int64_t E, n_spans;
  float* out;
  uint32_t ld_o;  // < 2^31 (checked at the entry points)
  const float* xroot;
  uint32_t ld_r;  // < 2^31 (checked at the entry points)
  float gin_scale;
  float* part;  // [n_spans][2][F]
  const float* gout;
  uint32_t ld_g;  // < 2^31 (checked at the entry points)
  const int32_t* gidx;
  float* grad_a;
  uint32_t ld_ga;  // < 2^31 (checked at the entry points)
  float* wpart;  // [waves][D + 1][F]
};

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

// the six significant products of two split operands, small terms first
__device__ __forceinline__ f32x4_t mfma6(const Planes& A, const Planes& B, f32x4_t d) {
  d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A.h, B.l, d, 0, 0, 0);
  d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A.l, B.h, d, 0, 0, 0);
  d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A.m, B.m, d, 0, 0, 0);
  d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A.h, B.m, d, 0, 0, 0);
  d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A.m, B.h, d, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(A.h, B.h, d, 0, 0, 0);
}

// this wave's LDS ops are done and the compiler moves no memory access across
__device__ __forceinline__ void wave_lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// NB: attribute blocks of 16 in the dW_e product (2 for D > 16; 1 otherwise and wherever there is no such product)
template <bool PROJ, bool BWD, int NB>
// waves per SIMD asked of the register allocator: the dW_e accumulators leave room for 2, the rest for 4
__global__ __launch_bounds__(kBlock, (PROJ && BWD) ? 2 : 4) void gine_span_kernel(SpanArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[kWaves][kTile][kLd];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int m = lane & 15, q = lane >> 4;
  float(*tile)[kLd] = lds[wave];
  const int cg0 = blockIdx.y * kCols;  // first column of this wave's group
  const int cw = cg0 + lane;           // the column this lane owns in the walk
  const bool cw_ok = cw < a.F;
  const int64_t wid = int64_t(blockIdx.x) * kWaves + wave, n_waves = int64_t(gridDim.x) * kWaves;

  // W_e's fragments (A = W_e^T: lane (m, q) holds column c0 + m, k = 8q..8q+7), once per wave
  Planes wf[kCB];
  float4 be[kCB];  // b_e: held by the backward (registers to spare at 2 waves), re-read per tile by the forward
  if constexpr (PROJ) {
#pragma unroll
    for (int cb = 0; cb < kCB; ++cb) {
      const int c = cg0 + cb * 16 + m;
      float v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int k = 8 * q + i;
        v[i] = (c < a.F && k < a.D) ? a.W[uint64_t(k) * a.ld_w + c] : 0.0f;
      }
      wf[cb] = split8(v);
      const int c4 = cg0 + cb * 16 + 4 * q;
      if constexpr (BWD) be[cb] = (a.b && c4 < a.F) ? ld4(a.b + c4) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
  }
  // dW_e^T accumulators: [column block][attribute block of 16], and the column sum of dz
  f32x4_t dw[kCB][NB];
  float dbias = 0.0f;
  if constexpr (PROJ && BWD) {
#pragma unroll
    for (int cb = 0; cb < kCB; ++cb)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) dw[cb][nb] = f32x4_t{0.0f, 0.0f, 0.0f, 0.0f};
  }

  for (int64_t span = wid; span < a.n_spans; span += n_waves) {
    const int64_t s0 = span * kSpan;
    const int64_t slot = s0 + lane;
    const bool live = slot < a.E;
    const int32_t xi = live ? a.xidx[slot] : 0;
    const int32_t rid = live ? a.rowid[slot] : -1;
    const int32_t ei = live ? (a.eidx ? a.eidx[slot] : int32_t(slot)) : 0;
    int32_t gi = 0;
    if constexpr (BWD) gi = live ? a.gidx[slot] : 0;
    // the rows this span shares with its neighbours (wave-uniform)
    const int32_t prev_row = s0 > 0 ? a.rowid[s0 - 1] : -1;
    const int32_t next_row = s0 + kSpan < a.E ? a.rowid[s0 + kSpan] : -1;

    int32_t cur = -1;  // the running row and this lane's sum of it
    float acc = 0.0f;
    auto flush = [&]() {
      if (cur < 0 || !cw_ok) return;
      if (cur == prev_row) {
        a.part[(span * 2 + 0) * a.F + cw] = acc;
      } else if (cur == next_row) {
        a.part[(span * 2 + 1) * a.F + cw] = acc;
      } else {
        float v = acc;
        if (!BWD && a.xroot) v = __fadd_rn(__fmul_rn(a.gin_scale, a.xroot[row_off(cur, a.ld_r) + cw]), v);
        a.out[row_off(cur, a.ld_o) + cw] = v;
      }
    };

#pragma unroll 1
    for (int t = 0; t < kSpan / kTile; ++t) {
      if (s0 + t * kTile >= a.E) break;  // wave-uniform
      const int src = t * kTile + m;     // the lane of the span that holds this lane's slot
      const bool ok = s0 + src < a.E;
      const int32_t e_m = __shfl(ei, src, 64);
      const int32_t x_m = __shfl(xi, src, 64);
      const int32_t g_m = __shfl(gi, src, 64);

      Planes ap;  // B = a^T: lane (m, q) holds slot m, k = 8q..8q+7
      if constexpr (PROJ) {
        const float* arow = a.a + row_off(e_m, a.ld_a);
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int k = 8 * q + i;
          v[i] = (ok && k < a.D) ? arow[k] : 0.0f;
        }
        ap = split8(v);
      }

#pragma unroll
      for (int cb = 0; cb < kCB; ++cb) {
        const int c4 = cg0 + cb * 16 + 4 * q;
        const bool in = ok && c4 < a.F;
        const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const float4 xv = in ? ld4(a.x + row_off(x_m, a.ld_x) + c4) : zero4;
        float ev[4];
        if constexpr (PROJ) {
          const f32x4_t d = mfma6(wf[cb], ap, f32x4_t{0.0f, 0.0f, 0.0f, 0.0f});
          float4 b4;
          if constexpr (BWD)
            b4 = be[cb];
          else
            b4 = (a.b && c4 < a.F) ? ld4(a.b + c4) : zero4;  // an L1 hit: not worth 16 registers at 4 waves
          ev[0] = __fadd_rn(d[0], b4.x);
          ev[1] = __fadd_rn(d[1], b4.y);
          ev[2] = __fadd_rn(d[2], b4.z);
          ev[3] = __fadd_rn(d[3], b4.w);
        } else {
          const float4 e4 = in ? ld4(a.a + row_off(e_m, a.ld_a) + c4) : zero4;
          ev[0] = e4.x, ev[1] = e4.y, ev[2] = e4.z, ev[3] = e4.w;
        }
        const float z[4] = {__fadd_rn(xv.x, ev[0]), __fadd_rn(xv.y, ev[1]), __fadd_rn(xv.z, ev[2]),
                            __fadd_rn(xv.w, ev[3])};
        float v[4];
        if constexpr (BWD) {
          const float4 gv = in ? ld4(a.gout + row_off(g_m, a.ld_g) + c4) : zero4;
          const float gg[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = (in && z[k] > 0.0f) ? gg[k] : 0.0f;
          if constexpr (!PROJ) {
            if (in) *reinterpret_cast<float4*>(a.grad_a + row_off(e_m, a.ld_ga) + c4) = make_float4(v[0], v[1], v[2], v[3]);
          }
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = !in ? 0.0f : (z[k] <= 0.0f ? 0.0f : z[k]);  // NaN stays NaN
        }
        *reinterpret_cast<float4*>(&tile[m][cb * 16 + 4 * q]) = make_float4(v[0], v[1], v[2], v[3]);
      }
      wave_lds_fence();

      if constexpr (PROJ && BWD) {
        // dW_e^T += dz^T a: A = dz^T (lane (m, q): column c0 + m, slots 8q..8q+7), B = a (lane (m, q):
        // attribute m (+16), slots 8q..8q+7); the 16 slots are K, padded to 32 (q >= 2: zeros)
        const bool kq = q < 2;
        Planes bp[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          const int d = 16 * nb + m;
          float v[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const int sl = t * kTile + ((8 * q + i) & 15);
            const int32_t e = __shfl(ei, sl, 64);
            v[i] = (kq && d < a.D && s0 + sl < a.E) ? a.a[row_off(e, a.ld_a) + d] : 0.0f;
          }
          bp[nb] = split8(v);
        }
#pragma unroll
        for (int cb = 0; cb < kCB; ++cb) {
          float v[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const float r = tile[(8 * q + i) & 15][cb * 16 + m];
            v[i] = kq ? r : 0.0f;
          }
          const Planes dp = split8(v);
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) dw[cb][nb] = mfma6(dp, bp[nb], dw[cb][nb]);
        }
      }

      // the walk: lane l sums column l over the tile's slots in CSR order
      for (int i = 0; i < kTile; ++i) {
        const int32_t r = __builtin_amdgcn_readlane(rid, t * kTile + i);
        if (r < 0) break;  // past the last slot (wave-uniform)
        const float v = tile[i][lane];
        if constexpr (PROJ && BWD) dbias = __fadd_rn(dbias, v);
        if (r != cur) {
          flush();
          cur = r;
          acc = v;
        } else {
          acc = __fadd_rn(acc, v);
        }
      }
      wave_lds_fence();  // the tile is read before the next one is written
    }
    flush();
  }

  if constexpr (PROJ && BWD) {  // every wave stores its partial (zeros where it had no span)
    float* wp = a.wpart + wid * (a.D + 1) * a.F;
#pragma unroll
    for (int cb = 0; cb < kCB; ++cb) {
      const int c4 = cg0 + cb * 16 + 4 * q;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const int d = 16 * nb + m;  // D^T block: lane (m, q) holds attribute d, columns c4..c4+3
        if (d < a.D && c4 < a.F)
          *reinterpret_cast<float4*>(wp + int64_t(d) * a.F + c4) =
              make_float4(dw[cb][nb][0], dw[cb][nb][1], dw[cb][nb][2], dw[cb][nb][3]);
      }
    }
    if (cw_ok) wp[int64_t(a.D) * a.F + cw] = dbias;
  }
}

struct FixArgs {
  const int32_t* rowptr;
  int64_t n_rows;
  int F;
  const float* part;
  float* out;
  int64_t ld_o;
  const float* xroot;
  int64_t ld_r;
  float gin_scale;
};

// Rows the span kernel did not store: the empty ones (epilogue alone) and those that
// straddle a span boundary, whose partials are part[first span][1], then
// part[span][0] of every later span, added in that order.
__global__ __launch_bounds__(kBlock) void gine_fixup_kernel(FixArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wid = (int64_t(blockIdx.x) * kBlock + threadIdx.x) >> 6, n_waves = (int64_t(gridDim.x) * kBlock) >> 6;
  for (int64_t r0 = wid * 64; r0 < a.n_rows; r0 += n_waves * 64) {
    const int64_t r = r0 + lane;
    int32_t b = 0, e = 0;
    if (r < a.n_rows) {
      b = a.rowptr[r];
      e = a.rowptr[r + 1];
    }
    const bool need = r < a.n_rows && (b == e || (b / kSpan) != ((e - 1) / kSpan));
    uint64_t todo = __ballot(need);
    while (todo) {  // wave-uniform
      const int l = __builtin_ctzll(todo);
      todo &= todo - 1;
      const int32_t rb = __shfl(b, l, 64), re = __shfl(e, l, 64);
      const int64_t row = r0 + l;
      const int64_t sb = rb / kSpan;
      const int32_t n = rb == re ? 0 : int32_t((re - 1) / kSpan - sb + 1);
      for (int c = 4 * lane; c < a.F; c += 256) {
        float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int32_t k0 = 0; k0 < n; k0 += kFixB) {
          float4 p[kFixB];
#pragma unroll
          for (int u = 0; u < kFixB; ++u) {  // clamped, unconditional: all in flight together
            const int32_t k = k0 + u < n ? k0 + u : n - 1;
            p[u] = ld4(a.part + ((sb + k) * 2 + (k == 0 ? 1 : 0)) * a.F + c);
          }
#pragma unroll
          for (int u = 0; u < kFixB; ++u) {
            if (k0 + u < n) {
              const bool first = k0 + u == 0;  // the first partial is the sum so far (no 0 + p: keeps -0)
              s.x = first ? p[u].x : __fadd_rn(s.x, p[u].x);
              s.y = first ? p[u].y : __fadd_rn(s.y, p[u].y);
              s.z = first ? p[u].z : __fadd_rn(s.z, p[u].z);
              s.w = first ? p[u].w : __fadd_rn(s.w, p[u].w);
            }
          }
        }
        if (a.xroot) {
          const float4 xr = ld4(a.xroot + row * a.ld_r + c);
          s.x = __fadd_rn(__fmul_rn(a.gin_scale, xr.x), s.x);
          s.y = __fadd_rn(__fmul_rn(a.gin_scale, xr.y), s.y);
          s.z = __fadd_rn(__fmul_rn(a.gin_scale, xr.z), s.z);
          s.w = __fadd_rn(__fmul_rn(a.gin_scale, xr.w), s.w);
        }
        *reinterpret_cast<float4*>(a.out + row * a.ld_o + c) = s;
      }
    }
  }
}

// dW_e [D, F] and db_e [F] from the waves' partials [n_waves][D + 1][F], in wave order.  A block owns 64
// consecutive elements (one per lane: 256-byte rows of every partial) and cuts the wave list into kFinJ
// runs, one per wave of the block; each run is added in order, kFinU loads in flight, and thread (e, 0)
// adds the kFinJ run sums in order.
__global__ __launch_bounds__(64 * kFinJ) void gine_finish_kernel(const float* wpart, int64_t n_waves,
                                                                              int D, int F, float* gW, float* gb) {
  __shared__ float runs[kFinJ][64];
  const int ex = threadIdx.x & 63, j = threadIdx.x >> 6;
  const int64_t n_el = int64_t(D + 1) * F;
  const int64_t el = int64_t(blockIdx.x) * 64 + ex;
  const int64_t per = (n_waves + kFinJ - 1) / kFinJ;
  const int64_t w0 = j * per, w1 = w0 + per < n_waves ? w0 + per : n_waves;
  float s = 0.0f;
  if (el < n_el) {
    for (int64_t w = w0; w < w1; w += kFinU) {
      float v[kFinU];
#pragma unroll
      for (int u = 0; u < kFinU; ++u) v[u] = w + u < w1 ? wpart[(w + u) * n_el + el] : 0.0f;
#pragma unroll
      for (int u = 0; u < kFinU; ++u) s = w + u < w1 ? __fadd_rn(s, v[u]) : s;
    }
  }
  runs[j][ex] = s;
  __syncthreads();
  if (j == 0 && el < n_el) {
    float v = runs[0][ex];
    for (int k = 1; k < kFinJ; ++k) v = __fadd_rn(v, runs[k][ex]);
    if (el < int64_t(D) * F) {
      gW[el] = v;
    } else if (gb) {
      gb[el - int64_t(D) * F] = v;
    }
  }
}

constexpr int64_t kInt32Limit = int64_t(1) << 31;

int64_t span_count(int64_t n_slots) { return (n_slots + kSpan - 1) / kSpan; }
int col_groups(int64_t F) { return int((F + kCols - 1) / kCols); }
// blocks along x: four spans per block, at most kGridCap blocks in all
int64_t grid_x(int64_t n_slots, int64_t F) {
  const int64_t need = (span_count(n_slots) + kWaves - 1) / kWaves, cap = kGridCap / col_groups(F);
  const int64_t g = need < cap ? need : cap;
  return g < 1 ? 1 : g;
}
size_t part_floats(int64_t n_slots, int64_t F) { return size_t(span_count(n_slots)) * 2 * size_t(F); }
size_t wpart_floats(int64_t n_slots, int64_t F, int64_t D) {
  return size_t(grid_x(n_slots, F)) * kWaves * size_t(D + 1) * size_t(F);
}
size_t workspace_bytes(int64_t n_slots, int64_t F, int64_t D, bool backward) {
  size_t n = align_up(part_floats(n_slots, F) * sizeof(float), 256);
  if (backward && D > 0) n += align_up(wpart_floats(n_slots, F, D) * sizeof(float), 256);
  return n;
}

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// the shape rules both entry points share; D = 0 is the plain variant
int check_shape(const char* fn, int64_t F, int64_t D, int64_t n_rows, int64_t n_slots, int64_t n_e, int64_t ld_x,
                int64_t ld_edge, int64_t ld_w) {
  KGX_REQUIRE(n_rows >= 0 && n_rows < kInt32Limit && n_slots >= 0 && n_slots < kInt32Limit, KGX_ERR_ARG,
              "%s: n_rows %lld / n_slots %lld outside [0, 2^31)", fn, (long long)n_rows, (long long)n_slots);
  KGX_REQUIRE(n_e >= 0 && n_e < kInt32Limit, KGX_ERR_ARG, "%s: edge table rows n_e = %lld outside [0, 2^31)", fn,
              (long long)n_e);
  KGX_REQUIRE(F >= 1 && D >= 0, KGX_ERR_ARG, "%s: F %lld, D %lld", fn, (long long)F, (long long)D);
  const int64_t we = D > 0 ? D : F;
  KGX_REQUIRE(ld_x >= F && ld_edge >= we && (D == 0 || ld_w >= F), KGX_ERR_ARG,
              "%s: leading dimension below the width (ld_x %lld, ld_edge %lld, ld_w %lld; F %lld, edge width %lld)", fn,
              (long long)ld_x, (long long)ld_edge, (long long)ld_w, (long long)F, (long long)we);
  KGX_REQUIRE(ld_x < kInt32Limit && ld_edge < kInt32Limit && ld_w < kInt32Limit, KGX_ERR_ARG,
              "%s: a leading dimension >= 2^31", fn);
  KGX_REQUIRE(F % 4 == 0 && F <= 512 && D <= 32, KGX_ERR_UNSUPPORTED,
              "%s: F = %lld, D = %lld (F a multiple of 4 in [4, 512], D in [1, 32])", fn, (long long)F, (long long)D);
  return KGX_OK;
}

// float4 access: 16-byte aligned base and a leading dimension that keeps every row so
int check_vec(const char* fn, const char* what, const void* p, int64_t ld) {
  KGX_REQUIRE(p == nullptr || (aligned16(p) && ld % 4 == 0), KGX_ERR_UNSUPPORTED,
              "%s: %s is read four floats at a time: a 16-byte aligned address and a leading dimension that is a "
              "multiple of 4 (got ld %lld)", fn, what, (long long)ld);
  return KGX_OK;
}

// One launch of the span kernel on a grid that is resident at once: the waves stride over the spans, so
// blocks beyond the kernel's occupancy would only queue behind the first round.  grid_x caps the blocks at
// kGridCap (the wave partials of the projected backward are sized by it); *n_waves: the waves along x.
template <class Kern>
int launch_one(Kern kern, const SpanArgs& a, hipStream_t s, int64_t* n_waves) {
  const int ncg = col_groups(a.F);
  const int64_t resident = occupancy_blocks(kern, kBlock, 2) / ncg;
  int64_t gx = grid_x(a.E, a.F);
  if (gx > resident) gx = resident > 0 ? resident : 1;
  *n_waves = gx * kWaves;
  hipLaunchKernelGGL(kern, dim3(unsigned(gx), unsigned(ncg)), dim3(kBlock), 0, s, a);
  KGX_CHECK_LAUNCH();
  return KGX_OK;
}

template <bool BWD>
int launch_span(bool proj, const SpanArgs& a, hipStream_t s, int64_t* n_waves) {
  if constexpr (BWD) {
    if (proj && a.D > 16) return launch_one(gine_span_kernel<true, true, 2>, a, s, n_waves);
  }
  if (proj) return launch_one(gine_span_kernel<true, BWD, 1>, a, s, n_waves);
  return launch_one(gine_span_kernel<false, BWD, 1>, a, s, n_waves);
}

int launch_fixup(const FixArgs& f, hipStream_t s) {
  hipLaunchKernelGGL(gine_fixup_kernel, dim3(grid_for(f.n_rows)), dim3(kBlock), 0, s, f);
  KGX_CHECK_LAUNCH();
  return KGX_OK;
}

}  // namespace
}  // namespace kgx

using namespace kgx;

#define KGX_TRY(expr)                 \
  do {                                \
    const int kgx_rc_ = (expr);       \
    if (kgx_rc_ != KGX_OK) return kgx_rc_; \
  } while (0)

extern "C" int kgx_gine_workspace_bytes(int64_t n_slots, int64_t F, int64_t D, int backward, size_t* bytes) {
  KGX_REQUIRE(bytes && n_slots >= 0 && n_slots < kInt32Limit && F >= 1 && F <= 512 && D >= 0 && D <= 32, KGX_ERR_ARG,
              "kgx_gine_workspace_bytes: n_slots %lld, F %lld, D %lld", (long long)n_slots, (long long)F, (long long)D);
  *bytes = workspace_bytes(n_slots, F, D, backward != 0);
  return KGX_OK;
}

extern "C" int kgx_gine_run(const kgx_gine_args* p, kgx_stream_t stream_) {
  KGX_REQUIRE(p && p->struct_size == sizeof(kgx_gine_args), KGX_ERR_ARG,
              "kgx_gine_run: struct_size %llu is not this header's %zu", p ? (unsigned long long)p->struct_size : 0ull,
              sizeof(kgx_gine_args));
  const char* fn = "kgx_gine_run";
  KGX_TRY(check_shape(fn, p->F, p->D, p->n_rows, p->n_slots, p->n_e, p->ld_x, p->ld_edge, p->ld_w));
  KGX_REQUIRE(p->ld_out >= p->F && p->ld_out < kInt32Limit && (!p->xroot || (p->ld_xroot >= p->F && p->ld_xroot < kInt32Limit)),
              KGX_ERR_ARG, "%s: leading dimension of out / xroot below F or >= 2^31", fn);
  if (p->n_rows == 0) return KGX_OK;
  KGX_REQUIRE(p->rowptr && p->out && p->x && (p->n_slots == 0 || (p->col && p->row_of_slot && p->edge)), KGX_ERR_ARG,
              "%s: null pointer", fn);
  KGX_REQUIRE(p->D == 0 || p->W, KGX_ERR_ARG, "%s: D = %lld needs W", fn, (long long)p->D);
  KGX_REQUIRE(p->n_slots == 0 || p->eid || p->n_e == p->n_slots, KGX_ERR_ARG, "%s: an edge table in CSR order has n_slots = %lld rows, got %lld",
              fn, (long long)p->n_slots, (long long)p->n_e);
  KGX_TRY(check_vec(fn, "x", p->x, p->ld_x));
  KGX_TRY(check_vec(fn, "out", p->out, p->ld_out));
  KGX_TRY(check_vec(fn, "xroot", p->xroot, p->ld_xroot));
  KGX_TRY(check_vec(fn, "bias", p->bias, 4));
  if (p->D == 0) KGX_TRY(check_vec(fn, "edge", p->edge, p->ld_edge));
  KGX_REQUIRE(p->workspace && p->workspace_bytes >= workspace_bytes(p->n_slots, p->F, p->D, false), KGX_ERR_ARG,
              "%s: workspace of %llu bytes, needs %zu", fn, (unsigned long long)p->workspace_bytes,
              workspace_bytes(p->n_slots, p->F, p->D, false));
  hipStream_t stream = as_stream(stream_);
  SpanArgs a{};
  a.x = p->x, a.ld_x = uint32_t(p->ld_x), a.xidx = p->col, a.rowid = p->row_of_slot, a.eidx = p->eid;
  a.a = p->edge, a.ld_a = uint32_t(p->ld_edge), a.W = p->W, a.ld_w = uint32_t(p->ld_w), a.b = p->bias;
  a.D = int(p->D), a.F = int(p->F), a.E = p->n_slots, a.n_spans = span_count(p->n_slots);
  a.out = p->out, a.ld_o = uint32_t(p->ld_out), a.xroot = p->xroot, a.ld_r = uint32_t(p->ld_xroot), a.gin_scale = p->gin_scale;
  a.part = static_cast<float*>(p->workspace);
  int64_t n_waves = 0;
  if (p->n_slots > 0) KGX_TRY(launch_span<false>(p->D > 0, a, stream, &n_waves));
  return launch_fixup(FixArgs{p->rowptr, p->n_rows, a.F, a.part, a.out, a.ld_o, a.xroot, a.ld_r, a.gin_scale}, stream);
}

extern "C" int kgx_gine_backward_run(const kgx_gine_backward_args* p, kgx_stream_t stream_) {
  KGX_REQUIRE(p && p->struct_size == sizeof(kgx_gine_backward_args), KGX_ERR_ARG,
              "kgx_gine_backward_run: struct_size %llu is not this header's %zu",
              p ? (unsigned long long)p->struct_size : 0ull, sizeof(kgx_gine_backward_args));
  const char* fn = "kgx_gine_backward_run";
  KGX_TRY(check_shape(fn, p->F, p->D, p->n_rows, p->n_slots, p->n_e, p->ld_x, p->ld_edge, p->ld_w));
  KGX_REQUIRE(p->ld_gout >= p->F && p->ld_gout < kInt32Limit && p->ld_gx >= p->F && p->ld_gx < kInt32Limit, KGX_ERR_ARG,
              "%s: leading dimension of gout / grad_x below F or >= 2^31", fn);
  KGX_REQUIRE(p->grad_x, KGX_ERR_ARG, "%s: grad_x is missing", fn);
  if (p->D == 0) {
    KGX_REQUIRE(p->grad_edge, KGX_ERR_ARG, "%s: grad_edge is missing (plain variant)", fn);
    KGX_REQUIRE(p->ld_ge >= p->F && p->ld_ge < kInt32Limit, KGX_ERR_ARG,
                "%s: leading dimension of grad_edge %lld below F or >= 2^31", fn, (long long)p->ld_ge);
  } else {
    KGX_REQUIRE(p->grad_W && (p->grad_bias || !p->bias), KGX_ERR_ARG, "%s: grad_W / grad_bias is missing", fn);
  }
  if (p->n_rows == 0) return KGX_OK;
  KGX_REQUIRE(p->t_rowptr && p->x && p->gout && (p->n_slots == 0 || (p->t_col && p->t_row_of_slot && p->t_eid && p->edge)),
              KGX_ERR_ARG, "%s: null pointer", fn);
  KGX_REQUIRE(p->D == 0 || p->W, KGX_ERR_ARG, "%s: D = %lld needs W", fn, (long long)p->D);
  KGX_TRY(check_vec(fn, "x", p->x, p->ld_x));
  KGX_TRY(check_vec(fn, "gout", p->gout, p->ld_gout));
  KGX_TRY(check_vec(fn, "grad_x", p->grad_x, p->ld_gx));
  KGX_TRY(check_vec(fn, "bias", p->bias, 4));
  if (p->D == 0) {
    KGX_TRY(check_vec(fn, "edge", p->edge, p->ld_edge));
    KGX_TRY(check_vec(fn, "grad_edge", p->grad_edge, p->ld_ge));
  }
  KGX_REQUIRE(p->workspace && p->workspace_bytes >= workspace_bytes(p->n_slots, p->F, p->D, true), KGX_ERR_ARG,
              "%s: workspace of %llu bytes, needs %zu", fn, (unsigned long long)p->workspace_bytes,
              workspace_bytes(p->n_slots, p->F, p->D, true));
  hipStream_t stream = as_stream(stream_);
  SpanArgs a{};
  a.x = p->x, a.ld_x = uint32_t(p->ld_x), a.xidx = p->t_row_of_slot, a.rowid = p->t_row_of_slot, a.eidx = p->t_eid;
  a.a = p->edge, a.ld_a = uint32_t(p->ld_edge), a.W = p->W, a.ld_w = uint32_t(p->ld_w), a.b = p->bias;
  a.D = int(p->D), a.F = int(p->F), a.E = p->n_slots, a.n_spans = span_count(p->n_slots);
  a.out = p->grad_x, a.ld_o = uint32_t(p->ld_gx);
  a.gout = p->gout, a.ld_g = uint32_t(p->ld_gout), a.gidx = p->t_col, a.grad_a = p->grad_edge, a.ld_ga = uint32_t(p->ld_ge);
  a.part = static_cast<float*>(p->workspace);
  a.wpart = reinterpret_cast<float*>(static_cast<char*>(p->workspace) +
                                     align_up(part_floats(p->n_slots, p->F) * sizeof(float), 256));
  int64_t n_waves = 0;  // no slot: the span kernel does not run, and the finish adds no partial
  if (p->n_slots > 0) KGX_TRY(launch_span<true>(p->D > 0, a, stream, &n_waves));
  KGX_TRY(launch_fixup(FixArgs{p->t_rowptr, p->n_rows, a.F, a.part, a.out, a.ld_o, nullptr, 0, 0.0f}, stream));
  if (p->D > 0) {
    const int64_t n_el = (p->D + 1) * p->F;
    hipLaunchKernelGGL(gine_finish_kernel, dim3(unsigned((n_el + 63) / 64)), dim3(64 * kFinJ), 0, stream, a.wpart, n_waves,
                       a.D, a.F, p->grad_W, p->grad_bias);
    KGX_CHECK_LAUNCH();
  }
  return KGX_OK;
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
