// Fused dot-product (query / key / value) graph attention for the kgx engine
// (gfx950, wave64): PyG's TransformerConv message passing without edge
// features, DGL's SDDMM -> edge_softmax -> SpMM chain in one kernel.
//
// Forward, destination row i, head h, edges e of the row (j_e = col[e]):
//   s_e = scale * <q[i,h,:], k[j_e,h,:]>,  m = max_e s_e,  l = sum_e exp(s_e - m)
//   out[i,h,:] = sum_e exp(s_e - m) / l * mask_e * v[j_e,h,:]
// The lane layout, the online softmax with fp64 numerator / denominator, the
// hub-split schedule with a chunk-order fix-up and the (seed, edge id, head)
// dropout mask are kgx_gatv2's (gatv2.hip).  Two rows are gathered per edge
// (k_j and v_j), both unconditionally from clamped addresses, masked on use.
//
// The score is bilinear, so both backward passes recompute p_e from q, k and
// the saved (m, l): no E x H workspace, and no atomics -- every output element
// has one writer and a fixed summation order, so a run gives the same bits
// every time.
#include <cstdlib>

#include "kgx_internal.h"
#include "kgx_vec.h"

namespace kgx {
namespace {

struct DotArgs {
  // forward CSR + its schedule
  const int32_t* rowptr;
  const int32_t* rows;
  int64_t n_rows;
  const int4* items;
  int64_t n_items;
  const int4* split;
  int64_t n_split;
  const int32_t* col;
  const float* q;
  int64_t ld_q;
  const float* k;
  int64_t ld_k;
  const float* v;
  int64_t ld_v;
  int H, C;
  float scale;
  float* out;  // forward: written; backward: the forward's output
  int64_t ld_o;
  float* partials;  // forward, per slot: [H*C acc | H m | H l], slots ld_p floats apart
  int64_t ld_p;     // forward: H*C + 2H rounded up to a multiple of 4; backward: 2*H*C
  float* stats;     // [n_dst, 2H]: per row and head the softmax max m and denominator l (no epsilon)
  const int32_t* drop_key;
  uint64_t drop_seed;
  uint32_t drop_thresh;
  float drop_scale;
  // backward only
  const float* grad;
  int64_t ld_g;
  float* dsum;  // [n_dst, H]: D = <G, out>_h
  float* grad_q;
  int64_t ld_gq;
  float* grad_k;
  int64_t ld_gk;
  float* grad_v;
  int64_t ld_gv;
  const int32_t* t_rowptr;
  const int32_t* t_rows;
  int64_t t_n_rows;
  const int4* t_items;
  int64_t t_n_items;
  const int4* t_split;
  int64_t t_n_split;
  const int32_t* t_col;  // destination row of each transposed slot
  const int32_t* t_key;  // input edge id of each transposed slot (dropout key)
  int G, lgG, LH, lgLH;
};

// Sum over the LH (power of two) lanes of a head, result in every lane: DPP
// moves within 16 lanes (quad_perm xor 1, xor 2, row_half_mirror, row_mirror),
// shuffles above.  This file's own copy (gatv2.hip keeps its own).
template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float head_reduce(float p, int LH) {
  if (LH > 1) p += dpp<0xB1>(p);   // quad_perm [1,0,3,2]
  if (LH > 2) p += dpp<0x4E>(p);   // quad_perm [2,3,0,1]
  if (LH > 4) p += dpp<0x141>(p);  // row_half_mirror
  if (LH > 8) p += dpp<0x140>(p);  // row_mirror
  if (LH > 16) p += __shfl_xor(p, 16, 64);
  if (LH > 32) p += __shfl_xor(p, 32, 64);
  return p;
}

__device__ __forceinline__ void work_item(const int4* items, const int32_t* rows, const int32_t* rowptr, int64_t it,
                                          int32_t& row, int32_t& beg, int32_t& end, int32_t& slot) {
  if (items) {
    const int4 w = items[it];
    row = w.x;
    beg = w.y;
    end = w.z;
    slot = w.w;
  } else {
    row = rows[it];
    beg = rowptr[row];
    end = rowptr[row + 1];
    slot = -1;
  }
}

// exp(s - m) with a -inf score weighing 0 whatever m is (-inf - -inf is NaN);
// +inf and NaN scores give NaN, which poisons their (row, head) only.
__device__ __forceinline__ float weight(float s, float m) { return s == -__builtin_inff() ? 0.0f : expf(s - m); }

template <int K, int U>
__global__ __launch_bounds__(kBlock) void dot_attention_kernel(DotArgs a) {
  const int G = a.G;
  const int lane = threadIdx.x & (G - 1);
  const int head = lane >> a.lgLH;
  const int sub = lane & (a.LH - 1);
  const bool valid = head < a.H && sub * K < a.C;
  const int f = valid ? head * a.C + sub * K : 0;  // padding lanes read columns [0, K) and use nothing
  const int HC = a.H * a.C;
  const int64_t ngroups = (int64_t(gridDim.x) * kBlock) >> a.lgG;
  const int64_t n_work = a.items ? a.n_items : a.n_rows;

  for (int64_t it = (int64_t(blockIdx.x) * kBlock + threadIdx.x) >> a.lgG; it < n_work; it += ngroups) {
    int32_t row, beg, end, slot;
    work_item(a.items, a.rows, a.rowptr, it, row, beg, end, slot);
    float qd[K];
    double acc[K];
    vload<K>(qd, a.q + int64_t(row) * a.ld_q + f);
#pragma unroll
    for (int c = 0; c < K; ++c) acc[c] = 0.0;
    float m = -__builtin_inff();
    double l = 0.0;

    for (int32_t e = beg; e < end; e += U) {
      const int n = (end - e) < U ? (end - e) : U;
      int32_t j[U];
#pragma unroll
      for (int u = 0; u < U; ++u) j[u] = a.col[u < n ? e + u : end - 1];
      float dm[U];  // attention dropout multiplier per edge (this lane's head)
#pragma unroll
      for (int u = 0; u < U; ++u)
        dm[u] = a.drop_key ? drop_scale(a.drop_seed, uint32_t(a.drop_key[u < n ? e + u : end - 1]), uint32_t(head),
                                        a.drop_thresh, a.drop_scale)
                           : 1.0f;
      // unconditional loads from clamped addresses (edges past the end re-read the last one), masked on use
      float ks[U][K], vs[U][K];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        vload<K>(ks[u], a.k + row_off(j[u], a.ld_k) + f);
        vload<K>(vs[u], a.v + row_off(j[u], a.ld_v) + f);
      }
      float s[U];
      float mc = -__builtin_inff();
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float p = 0.0f;
#pragma unroll
        for (int c = 0; c < K; ++c) p += qd[c] * ks[u][c];
        // a padding lane's partial is dropped here, whatever it read (an inf of another head included)
        s[u] = a.scale * head_reduce(valid ? p : 0.0f, a.LH);
        if (u < n) mc = fmaxf(mc, s[u]);
      }
      const float m_new = fmaxf(m, mc);
      const double r = m == m_new ? 1.0 : double(expf(m - m_new));  // -inf == -inf: nothing weighed yet
      l *= r;
#pragma unroll
      for (int c = 0; c < K; ++c) acc[c] *= r;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (u < n) {
          const double pu = double(weight(s[u], m_new));
          l += pu;  // the denominator sees every edge; dropout masks the normalised weight
          const double pd = pu * double(dm[u]);
#pragma unroll
          for (int c = 0; c < K; ++c) acc[c] = fma(pd, double(vs[u][c]), acc[c]);
        }
      }
      m = m_new;
    }

    if (!valid) continue;
    if (slot >= 0) {
      float* p = a.partials + int64_t(slot) * a.ld_p;
      float accf[K];
#pragma unroll
      for (int c = 0; c < K; ++c) accf[c] = float(acc[c]);
      vstore<K>(p + f, accf);
      if (sub == 0) {
        p[HC + head] = m;
        p[HC + a.H + head] = float(l);
      }
    } else {
      if (a.stats && sub == 0) {
        a.stats[int64_t(row) * 2 * a.H + head] = m;
        a.stats[int64_t(row) * 2 * a.H + a.H + head] = float(l);
      }
      float o[K];
#pragma unroll
      for (int c = 0; c < K; ++c) o[c] = end > beg ? float(acc[c] / l) : 0.0f;  // a row without edges is a zero row
      vstore<K>(a.out + int64_t(row) * a.ld_o + f, o);
    }
  }
}

// Merges the chunk partials of split rows in chunk order.
template <int K>
__global__ __launch_bounds__(kBlock) void dot_attention_fixup_kernel(DotArgs a) {
  const int G = a.G;
  const int lane = threadIdx.x & (G - 1);
  const int head = lane >> a.lgLH;
  const int sub = lane & (a.LH - 1);
  const bool valid = head < a.H && sub * K < a.C;
  const int f = head * a.C + sub * K;
  const int HC = a.H * a.C;
  const int64_t ngroups = (int64_t(gridDim.x) * kBlock) >> a.lgG;
  for (int64_t it = (int64_t(blockIdx.x) * kBlock + threadIdx.x) >> a.lgG; it < a.n_split; it += ngroups) {
    if (!valid) continue;
    const int4 sp = a.split[it];
    const int32_t row = sp.x, slot0 = sp.y, nc = sp.z;
    constexpr int B = K >= 16 ? 8 : 16;  // chunk loads in flight per step (clamped, unconditional); B*K <= 128 registers
    const int64_t ld_p = a.ld_p;
    float M = -__builtin_inff();
    double L = 0.0, acc[K];
#pragma unroll
    for (int c = 0; c < K; ++c) acc[c] = 0.0;
    for (int32_t c0 = 0; c0 < nc; c0 += B) {
      float mv[B], lv[B], pv[B][K];
#pragma unroll
      for (int u = 0; u < B; ++u) {
        const float* p = a.partials + int64_t(slot0 + (c0 + u < nc ? c0 + u : nc - 1)) * ld_p;
        mv[u] = p[HC + head];
        lv[u] = p[HC + a.H + head];
        vload<K>(pv[u], p + f);
      }
      float mb = M;
#pragma unroll
      for (int u = 0; u < B; ++u) mb = fmaxf(mb, mv[u]);  // clamped repeats leave the max unchanged
      if (mb > M) {
        const double r = double(expf(M - mb));  // M = -inf: 0, and L and acc are still 0
        L *= r;
#pragma unroll
        for (int c = 0; c < K; ++c) acc[c] *= r;
        M = mb;
      }
#pragma unroll
      for (int u = 0; u < B; ++u) {
        const bool in = c0 + u < nc;  // clamped repeats add nothing (selected, not multiplied by 0)
        const double sc = double(weight(mv[u], M));  // a chunk of -inf scores holds zeros and weighs 0
        L = in ? L + double(lv[u]) * sc : L;
#pragma unroll
        for (int c = 0; c < K; ++c) acc[c] = in ? acc[c] + double(pv[u][c]) * sc : acc[c];
      }
    }
    if (a.stats && sub == 0) {
      a.stats[int64_t(row) * 2 * a.H + head] = M;
      a.stats[int64_t(row) * 2 * a.H + a.H + head] = float(L);
    }
    float o[K];
#pragma unroll
    for (int c = 0; c < K; ++c) o[c] = float(acc[c] / L);
    vstore<K>(a.out + int64_t(row) * a.ld_o + f, o);
  }
}

// ---------------------------------------------------------------------------
// Backward.  With G = d loss / d out, D[i,h] = <G[i,h,:], out[i,h,:]> (holds
// under dropout: out contains the mask), p_e = exp(s_e - m) / l:
//   ds_e      = p_e (mask_e <G_i, v_j>_h - D[i,h])
//   grad_q[i] = scale sum_e ds_e k[j_e]                 destination pass
//   grad_v[j] = sum_{e: j_e = j} p_e mask_e G_i          source pass
//   grad_k[j] = scale sum_{e: j_e = j} ds_e q_i          source pass
// Both passes recompute s_e from q and k with the forward's operation order.
// ---------------------------------------------------------------------------
template <int K>
constexpr int bwd_unroll() {
  return K <= 4 ? 8 : (K == 8 ? 4 : 2);  // two K-wide rows per edge in flight: 64 registers
}

template <int K>
__global__ __launch_bounds__(kBlock) void dot_attention_bwd_dst_kernel(DotArgs a) {
  constexpr int U = bwd_unroll<K>();
  const int G = a.G;
  const int lane = threadIdx.x & (G - 1);
  const int head = lane >> a.lgLH;
  const int sub = lane & (a.LH - 1);
  const bool valid = head < a.H && sub * K < a.C;
  const int f = valid ? head * a.C + sub * K : 0;
  const int hh = valid ? head : 0;
  const int64_t ngroups = (int64_t(gridDim.x) * kBlock) >> a.lgG;
  const int64_t n_work = a.items ? a.n_items : a.n_rows;
  for (int64_t it = (int64_t(blockIdx.x) * kBlock + threadIdx.x) >> a.lgG; it < n_work; it += ngroups) {
    int32_t row, beg, end, slot;
    work_item(a.items, a.rows, a.rowptr, it, row, beg, end, slot);
    float qd[K], gr[K], o[K], gq[K];
    vload<K>(qd, a.q + int64_t(row) * a.ld_q + f);
    vload<K>(gr, a.grad + int64_t(row) * a.ld_g + f);
    vload<K>(o, a.out + int64_t(row) * a.ld_o + f);
    float dp = 0.0f;
#pragma unroll
    for (int c = 0; c < K; ++c) {
      gq[c] = 0.0f;
      dp += gr[c] * o[c];
    }
    const float D = head_reduce(valid ? dp : 0.0f, a.LH);  // padding lanes' partials are dropped
    // every chunk of a split row computes the same D; the row's first chunk stores it
    if (valid && sub == 0 && (slot < 0 || beg == a.rowptr[row])) a.dsum[int64_t(row) * a.H + head] = D;
    const float m = a.stats[int64_t(row) * 2 * a.H + hh];
    const float l = a.stats[int64_t(row) * 2 * a.H + a.H + hh];
    for (int32_t e = beg; e < end; e += U) {
      float ks[U][K], vs[U][K];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t j = a.col[e + u < end ? e + u : end - 1];
        vload<K>(ks[u], a.k + row_off(j, a.ld_k) + f);
        vload<K>(vs[u], a.v + row_off(j, a.ld_v) + f);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float ps = 0.0f, pa = 0.0f;
#pragma unroll
        for (int c = 0; c < K; ++c) {
          ps += qd[c] * ks[u][c];
          pa += gr[c] * vs[u][c];
        }
        const float s = a.scale * head_reduce(valid ? ps : 0.0f, a.LH);
        const float da = head_reduce(valid ? pa : 0.0f, a.LH);
        if (e + u < end) {
          const float p = __fdiv_rn(weight(s, m), l);
          const float dmu = a.drop_key ? drop_scale(a.drop_seed, uint32_t(a.drop_key[e + u]), uint32_t(head),
                                                    a.drop_thresh, a.drop_scale)
                                       : 1.0f;
          const float ds = p * (dmu * da - D);
#pragma unroll
          for (int c = 0; c < K; ++c) gq[c] += ds * ks[u][c];
        }
      }
    }
    if (!valid) continue;
#pragma unroll
    for (int c = 0; c < K; ++c) gq[c] *= a.scale;
    if (slot >= 0) vstore<K>(a.partials + int64_t(slot) * a.ld_p + f, gq);
    else vstore<K>(a.grad_q + int64_t(row) * a.ld_gq + f, gq);
  }
}

template <int K>
__global__ __launch_bounds__(kBlock) void dot_attention_bwd_src_kernel(DotArgs a) {
  constexpr int U = bwd_unroll<K>();
  const int G = a.G;
  const int lane = threadIdx.x & (G - 1);
  const int head = lane >> a.lgLH;
  const int sub = lane & (a.LH - 1);
  const bool valid = head < a.H && sub * K < a.C;
  const int f = valid ? head * a.C + sub * K : 0;
  const int hh = valid ? head : 0;
  const int HC = a.H * a.C;
  const int64_t ngroups = (int64_t(gridDim.x) * kBlock) >> a.lgG;
  const int64_t n_work = a.t_items ? a.t_n_items : a.t_n_rows;
  for (int64_t it = (int64_t(blockIdx.x) * kBlock + threadIdx.x) >> a.lgG; it < n_work; it += ngroups) {
    int32_t j, beg, end, slot;
    work_item(a.t_items, a.t_rows, a.t_rowptr, it, j, beg, end, slot);
    float kj[K], vj[K], gk[K], gv[K];
    vload<K>(kj, a.k + int64_t(j) * a.ld_k + f);
    vload<K>(vj, a.v + int64_t(j) * a.ld_v + f);
#pragma unroll
    for (int c = 0; c < K; ++c) {
      gk[c] = 0.0f;
      gv[c] = 0.0f;
    }
    for (int32_t e = beg; e < end; e += U) {
      float qi[U][K], gi[U][K], mv[U], lv[U], Dv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t i = a.t_col[e + u < end ? e + u : end - 1];
        mv[u] = a.stats[row_off(i, 2 * a.H) + hh];
        lv[u] = a.stats[row_off(i, 2 * a.H) + a.H + hh];
        Dv[u] = a.dsum[row_off(i, a.H) + hh];
        vload<K>(qi[u], a.q + row_off(i, a.ld_q) + f);
        vload<K>(gi[u], a.grad + row_off(i, a.ld_g) + f);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float ps = 0.0f, pa = 0.0f;
#pragma unroll
        for (int c = 0; c < K; ++c) {
          ps += qi[u][c] * kj[c];
          pa += gi[u][c] * vj[c];
        }
        const float s = a.scale * head_reduce(valid ? ps : 0.0f, a.LH);
        const float da = head_reduce(valid ? pa : 0.0f, a.LH);
        if (e + u < end) {
          const float p = __fdiv_rn(weight(s, mv[u]), lv[u]);
          const float dmu = a.drop_key ? drop_scale(a.drop_seed, uint32_t(a.t_key[e + u]), uint32_t(head),
                                                    a.drop_thresh, a.drop_scale)
                                       : 1.0f;
          const float pm = p * dmu;
          const float ds = p * (dmu * da - Dv[u]);
#pragma unroll
          for (int c = 0; c < K; ++c) {
            gv[c] += pm * gi[u][c];
            gk[c] += ds * qi[u][c];
          }
        }
      }
    }
    if (!valid) continue;
#pragma unroll
    for (int c = 0; c < K; ++c) gk[c] *= a.scale;
    if (slot >= 0) {
      float* p = a.partials + int64_t(slot) * a.ld_p;
      vstore<K>(p + f, gv);
      vstore<K>(p + HC + f, gk);
    } else {
      vstore<K>(a.grad_v + int64_t(j) * a.ld_gv + f, gv);
      vstore<K>(a.grad_k + int64_t(j) * a.ld_gk + f, gk);
    }
  }
}

// Sums the chunk partials of split rows in chunk order: columns [0, HC) of a
// slot into out0, columns [HC, W) (W = HC or 2 HC) into out1.
__global__ __launch_bounds__(kBlock) void dot_attention_bwd_fixup_kernel(const int4* __restrict__ split,
                                                                         int64_t n_split,
                                                                         const float* __restrict__ partials,
                                                                         int64_t ld_p, int HC, int W,
                                                                         float* __restrict__ out0, int64_t ld0,
                                                                         float* __restrict__ out1, int64_t ld1) {
  const int lane = threadIdx.x & 63;
  const int64_t ngroups = (int64_t(gridDim.x) * kBlock) >> 6;
  for (int64_t it = (int64_t(blockIdx.x) * kBlock + threadIdx.x) >> 6; it < n_split; it += ngroups) {
    const int4 sp = split[it];
    for (int f = lane; f < W; f += 64) {
      float acc = 0.0f;
      constexpr int B = 8;  // chunk loads in flight, then the in-order sum
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

template <int K, int U>
int launch_fwd(const DotArgs& a, hipStream_t s) {
  const int64_t work = a.items ? a.n_items : a.n_rows;
  if (work > 0) {
    auto kern = dot_attention_kernel<K, U>;
    hipLaunchKernelGGL(kern, dim3(resident_grid(kern, work, a.G)), dim3(kBlock), 0, s, a);
    KGX_CHECK_LAUNCH();
  }
  if (a.items && a.n_split > 0) {
    auto kern = dot_attention_fixup_kernel<K>;
    hipLaunchKernelGGL(kern, dim3(resident_grid(kern, a.n_split, a.G)), dim3(kBlock), 0, s, a);
    KGX_CHECK_LAUNCH();
  }
  return KGX_OK;
}

// Edges per online-softmax rescale: 2 for K >= 4, measured at C3 (8 heads x 16,
// R-MAT 1M / 10M, forward medians of 20): K = 8: 1.43 ms at 2, 1.44 at 3, 1.51
// at 4; K = 4: 1.38 / 1.51 / 1.47; K = 16: 1.55 / 1.53 / not run.  Two rows per
// edge are already in flight, and 2 leaves K = 8 at 94 registers (5 waves per
// SIMD against 4 at 3).  K <= 2 (float2 / scalar fallback) keeps 4 and was not
// swept.  KGX_DOT_U overrides it for A/B runs (DESIGN.md §12 has the table).
template <int K>
int launch_fwd_u(const DotArgs& a, hipStream_t s) {
  static const int uf = [] {
    const char* h = getenv("KGX_DOT_U");
    return h ? atoi(h) : 0;
  }();
  const int U = (uf >= 2 && uf <= 4) ? uf : (K <= 2 ? 4 : 2);
  switch (U) {
    case 2: return launch_fwd<K, 2>(a, s);
    case 3: return launch_fwd<K, 3>(a, s);
    default: return launch_fwd<K, 4>(a, s);
  }
}

template <int K>
int launch_bwd(const DotArgs& a, hipStream_t s) {
  const int HC = a.H * a.C;
  const int64_t work = a.items ? a.n_items : a.n_rows;
  if (work > 0) {
    auto kern = dot_attention_bwd_dst_kernel<K>;
    hipLaunchKernelGGL(kern, dim3(resident_grid(kern, work, a.G)), dim3(kBlock), 0, s, a);
    KGX_CHECK_LAUNCH();
  }
  if (a.items && a.n_split > 0) {
    hipLaunchKernelGGL(dot_attention_bwd_fixup_kernel, dim3(grid_for(a.n_split * 64, 4096)), dim3(kBlock), 0, s,
                       a.split, a.n_split, a.partials, a.ld_p, HC, HC, a.grad_q, a.ld_gq, a.grad_q, a.ld_gq);
    KGX_CHECK_LAUNCH();
  }
  const int64_t t_work = a.t_items ? a.t_n_items : a.t_n_rows;
  if (t_work > 0) {
    auto kern = dot_attention_bwd_src_kernel<K>;
    hipLaunchKernelGGL(kern, dim3(resident_grid(kern, t_work, a.G)), dim3(kBlock), 0, s, a);
    KGX_CHECK_LAUNCH();
  }
  if (a.t_items && a.t_n_split > 0) {
    hipLaunchKernelGGL(dot_attention_bwd_fixup_kernel, dim3(grid_for(a.t_n_split * 64, 4096)), dim3(kBlock), 0, s,
                       a.t_split, a.t_n_split, a.partials, a.ld_p, HC, 2 * HC, a.grad_v, a.ld_gv, a.grad_k, a.ld_gk);
    KGX_CHECK_LAUNCH();
  }
  return KGX_OK;
}

bool aligned(const void* p, int bytes) { return p == nullptr || reinterpret_cast<uintptr_t>(p) % bytes == 0; }

// Channels per lane, shared by the forward and both backward passes: float4
// pieces when every pointer is 16-byte aligned and every leading dimension a
// multiple of 4 -- 8 first, then 4, 16, the first that divides C and fits a
// row's heads into 64 lanes -- else float2 or scalar loads.  0: the shape
// needs more than 64 lanes per row.  Measured at C3 (medians, forward /
// forward + backward): K = 8: 1.43 / 5.09 ms, K = 4: 1.38 / 5.13, K = 16:
// 1.55 / 5.43 -- 4 wins the forward by 3 % and gives it back in the backward
// (ranges overlap there), so one rule serves all three kernels.
int pick_k(int heads, int channels, bool vec4, bool vec2) {
  if (vec4) {
    const int cands[3] = {8, 4, 16};
    for (int k : cands)
      if (channels % k == 0 && heads * next_pow2(channels / k) <= 64) return k;
  }
  const int k = (vec2 && channels % 2 == 0) ? 2 : 1;
  return heads * next_pow2((channels + k - 1) / k) <= 64 ? k : 0;
}

// experiment knob (A/B only): KGX_DOT_K = channels per lane, if the shape and alignment allow it
int knob_k(int K, int heads, int channels, bool vec4) {
  static const int kf = [] {
    const char* h = getenv("KGX_DOT_K");
    return h ? atoi(h) : 0;
  }();
  if (K >= 4 && vec4 && (kf == 4 || kf == 8 || kf == 16) && channels % kf == 0 &&
      heads * next_pow2(channels / kf) <= 64)
    return kf;
  return K;
}

void set_layout(DotArgs& a, int K) {
  a.LH = next_pow2((a.C + K - 1) / K);
  a.lgLH = log2i(a.LH);
  a.G = next_pow2(a.H * a.LH);
  a.lgG = log2i(a.G);
}

}  // namespace
}  // namespace kgx

using namespace kgx;

extern "C" int kgx_dot_attention(const int32_t* rowptr, const int32_t* rows, int64_t n_rows, const int32_t* items,
                                 int64_t n_items, const int32_t* split, int64_t n_split, const int32_t* col,
                                 const float* q, int64_t ld_q, const float* k, int64_t ld_k, const float* v,
                                 int64_t ld_v, int heads, int channels, float scale, float* out, int64_t ld_out,
                                 float* partials, float* stats, const int32_t* drop_key, float drop_p,
                                 uint64_t drop_seed, kgx_stream_t stream_) {
  hipStream_t stream = as_stream(stream_);
  KGX_REQUIRE(heads > 0 && channels > 0 && n_rows >= 0 && n_items >= 0 && n_split >= 0, KGX_ERR_ARG,
              "kgx_dot_attention: bad sizes");
  if (n_rows == 0) return KGX_OK;
  const int64_t HC = int64_t(heads) * channels;
  const int64_t lim = int64_t(1) << 31;
  KGX_REQUIRE(rowptr && rows && col && q && k && v && out, KGX_ERR_ARG, "kgx_dot_attention: null pointer");
  KGX_REQUIRE(ld_q >= HC && ld_k >= HC && ld_v >= HC && ld_out >= HC, KGX_ERR_ARG,
              "kgx_dot_attention: leading dimension < heads*channels");
  KGX_REQUIRE(ld_q < lim && ld_k < lim && ld_v < lim && ld_out < lim, KGX_ERR_ARG,
              "kgx_dot_attention: leading dimension >= 2^31");
  KGX_REQUIRE(drop_p >= 0.0f && drop_p < 1.0f, KGX_ERR_ARG, "kgx_dot_attention: dropout p must be in [0, 1)");
  const bool use_items = items != nullptr;
  KGX_REQUIRE(!use_items || n_split == 0 || (split && partials), KGX_ERR_ARG,
              "kgx_dot_attention: split rows need split list and partials");
  auto fits = [&](int b) {
    const int e = b / 4;
    return ld_q % e == 0 && ld_k % e == 0 && ld_v % e == 0 && ld_out % e == 0 && aligned(q, b) && aligned(k, b) &&
           aligned(v, b) && aligned(out, b) && aligned(partials, b);
  };
  const bool vec4 = fits(16);
  int K = pick_k(heads, channels, vec4, fits(8));
  KGX_REQUIRE(K > 0, KGX_ERR_UNSUPPORTED,
              "kgx_dot_attention: heads=%d x channels=%d needs more than 64 lanes per row (unsupported shape)", heads,
              channels);
  K = knob_k(K, heads, channels, vec4);
  DotArgs a{};
  a.rowptr = rowptr;
  a.rows = rows;
  a.n_rows = n_rows;
  a.items = use_items ? reinterpret_cast<const int4*>(items) : nullptr;
  a.n_items = use_items ? n_items : 0;
  a.split = reinterpret_cast<const int4*>(split);
  a.n_split = use_items ? n_split : 0;
  a.col = col;
  a.q = q;
  a.ld_q = ld_q;
  a.k = k;
  a.ld_k = ld_k;
  a.v = v;
  a.ld_v = ld_v;
  a.H = heads;
  a.C = channels;
  a.scale = scale;
  a.out = out;
  a.ld_o = ld_out;
  a.partials = partials;
  a.ld_p = (HC + 2 * heads + 3) / 4 * 4;
  a.stats = stats;
  if (drop_key && drop_p > 0.0f) {
    a.drop_key = drop_key;
    a.drop_seed = drop_seed;
    a.drop_thresh = uint32_t(double(drop_p) * 4294967296.0);
    a.drop_scale = 1.0f / (1.0f - drop_p);
  }
  set_layout(a, K);
  switch (K) {
    case 1: return launch_fwd_u<1>(a, stream);
    case 2: return launch_fwd_u<2>(a, stream);
    case 4: return launch_fwd_u<4>(a, stream);
    case 8: return launch_fwd_u<8>(a, stream);
    default: return launch_fwd_u<16>(a, stream);
  }
}

extern "C" int kgx_dot_attention_backward(
    const int32_t* rowptr, const int32_t* rows, int64_t n_rows, const int32_t* items, int64_t n_items,
    const int32_t* split, int64_t n_split, const int32_t* col, const float* q, int64_t ld_q, const float* k,
    int64_t ld_k, const float* v, int64_t ld_v, int heads, int channels, float scale, const float* out,
    int64_t ld_out, const float* stats, const float* grad_out, int64_t ld_grad, const int32_t* t_rowptr,
    const int32_t* t_rows, int64_t n_src, const int32_t* t_items, int64_t t_n_items, const int32_t* t_split,
    int64_t t_n_split, const int32_t* t_col, const int32_t* t_key, float* grad_q, int64_t ld_gq, float* grad_k,
    int64_t ld_gk, float* grad_v, int64_t ld_gv, float* dsum_ws, float* partials, const int32_t* drop_key,
    float drop_p, uint64_t drop_seed, kgx_stream_t stream_) {
  hipStream_t stream = as_stream(stream_);
  KGX_REQUIRE(heads > 0 && channels > 0 && n_rows >= 0 && n_src >= 0 && n_items >= 0 && n_split >= 0 &&
                  t_n_items >= 0 && t_n_split >= 0,
              KGX_ERR_ARG, "kgx_dot_attention_backward: bad sizes");
  if (n_rows == 0 && n_src == 0) return KGX_OK;
  const int64_t HC = int64_t(heads) * channels;
  const int64_t lim = int64_t(1) << 31;
  KGX_REQUIRE(rowptr && rows && col && q && k && v && out && stats && grad_out && t_rowptr && t_rows && t_col &&
                  grad_q && grad_k && grad_v && dsum_ws,
              KGX_ERR_ARG, "kgx_dot_attention_backward: null pointer");
  KGX_REQUIRE(ld_q >= HC && ld_k >= HC && ld_v >= HC && ld_out >= HC && ld_grad >= HC && ld_gq >= HC &&
                  ld_gk >= HC && ld_gv >= HC,
              KGX_ERR_ARG, "kgx_dot_attention_backward: leading dimension < heads*channels");
  KGX_REQUIRE(ld_q < lim && ld_k < lim && ld_v < lim && ld_out < lim && ld_grad < lim && ld_gq < lim &&
                  ld_gk < lim && ld_gv < lim,
              KGX_ERR_ARG, "kgx_dot_attention_backward: leading dimension >= 2^31");
  KGX_REQUIRE(drop_p >= 0.0f && drop_p < 1.0f, KGX_ERR_ARG,
              "kgx_dot_attention_backward: dropout p must be in [0, 1)");
  const bool dropping = drop_key && drop_p > 0.0f;
  KGX_REQUIRE(!dropping || t_key, KGX_ERR_ARG, "kgx_dot_attention_backward: dropout needs t_key");
  KGX_REQUIRE((!items || n_split == 0 || split) && (!t_items || t_n_split == 0 || t_split), KGX_ERR_ARG,
              "kgx_dot_attention_backward: split rows need a split list");
  KGX_REQUIRE(((!items || n_split == 0) && (!t_items || t_n_split == 0)) || partials, KGX_ERR_ARG,
              "kgx_dot_attention_backward: split rows need partials");
  auto fits = [&](int b) {
    const int e = b / 4;
    return ld_q % e == 0 && ld_k % e == 0 && ld_v % e == 0 && ld_out % e == 0 && ld_grad % e == 0 &&
           ld_gq % e == 0 && ld_gk % e == 0 && ld_gv % e == 0 && HC % e == 0 && aligned(q, b) && aligned(k, b) &&
           aligned(v, b) && aligned(out, b) && aligned(grad_out, b) && aligned(grad_q, b) && aligned(grad_k, b) &&
           aligned(grad_v, b) && aligned(partials, b);
  };
  const bool vec4 = fits(16);
  int K = pick_k(heads, channels, vec4, fits(8));
  KGX_REQUIRE(K > 0, KGX_ERR_UNSUPPORTED,
              "kgx_dot_attention_backward: heads=%d x channels=%d needs more than 64 lanes per row (unsupported "
              "shape)",
              heads, channels);
  K = knob_k(K, heads, channels, vec4);
  DotArgs a{};
  a.rowptr = rowptr;
  a.rows = rows;
  a.n_rows = n_rows;
  a.items = items ? reinterpret_cast<const int4*>(items) : nullptr;
  a.n_items = items ? n_items : 0;
  a.split = reinterpret_cast<const int4*>(split);
  a.n_split = items ? n_split : 0;
  a.col = col;
  a.q = q;
  a.ld_q = ld_q;
  a.k = k;
  a.ld_k = ld_k;
  a.v = v;
  a.ld_v = ld_v;
  a.H = heads;
  a.C = channels;
  a.scale = scale;
  a.out = const_cast<float*>(out);  // read only in the backward kernels
  a.ld_o = ld_out;
  a.partials = partials;
  a.ld_p = 2 * HC;
  a.stats = const_cast<float*>(stats);  // read only in the backward kernels
  if (dropping) {
    a.drop_key = drop_key;
    a.drop_seed = drop_seed;
    a.drop_thresh = uint32_t(double(drop_p) * 4294967296.0);
    a.drop_scale = 1.0f / (1.0f - drop_p);
  }
  a.grad = grad_out;
  a.ld_g = ld_grad;
  a.dsum = dsum_ws;
  a.grad_q = grad_q;
  a.ld_gq = ld_gq;
  a.grad_k = grad_k;
  a.ld_gk = ld_gk;
  a.grad_v = grad_v;
  a.ld_gv = ld_gv;
  a.t_rowptr = t_rowptr;
  a.t_rows = t_rows;
  a.t_n_rows = n_src;
  a.t_items = t_items ? reinterpret_cast<const int4*>(t_items) : nullptr;
  a.t_n_items = t_items ? t_n_items : 0;
  a.t_split = reinterpret_cast<const int4*>(t_split);
  a.t_n_split = t_items ? t_n_split : 0;
  a.t_col = t_col;
  a.t_key = t_key;
  set_layout(a, K);
  switch (K) {
    case 1: return launch_bwd<1>(a, stream);
    case 2: return launch_bwd<2>(a, stream);
    case 4: return launch_bwd<4>(a, stream);
    case 8: return launch_bwd<8>(a, stream);
    default: return launch_bwd<16>(a, stream);
  }
}
