// Fused dot-product (query / key / value) graph attention for the kgx engine
// (gfx950, wave64): PyG's TransformerConv message passing without edge
// features, DGL's SDDMM -> edge_softmax -> SpMM chain in one kernel.
//
// Forward, destination row i, head h, edges e of the row (j_e = col[e]):
//   s_e = scale * <q[i,h,:], k[j_e,h,:]>,  m = max_e s_e,  l = sum_e exp(s_e - m)
//   out[i,h,:] = sum_e exp(s_e - m) / l * mask_e * v[j_e,h,:]
// The lane layout, the online softmax with fp64 numerator / denominator, the
// hub-split schedule with a chunk-order fix-up and the (seed, edge id, head)
// dropout mask are the core kgx_gatv2 runs on too (kgx_attn.h).  Two rows are
// gathered per edge (k_j and v_j), both unconditionally from clamped addresses,
// masked on use.
//
// With an edge table (kgx_dot_attention_edge; PyG's edge_dim) a third row is
// gathered per edge and added to both, k'_e = k[j_e] + eps_e and v'_e = v[j_e]
// + eps_e, one rounded add per element, before any use; the kernels are
// templated on that (EDGE), and the instantiations without it are the code of
// the op without edge features.
//
// The score is bilinear, so both backward passes recompute p_e from q, k and
// the saved (m, l): no E x H workspace, and no atomics -- every output element
// has one writer and a fixed summation order, so a run gives the same bits
// every time.
#include "kgx_attn.h"

namespace kgx {
namespace {

struct DotArgs {
  Sched sched;  // forward CSR + its schedule
  const int32_t* col;
  const float* q;
  int64_t ld_q;
  const float* k;
  int64_t ld_k;
  const float* v;
  int64_t ld_v;
  int H, C;
  float scale;
  // forward: written; stats keep the denominator l (no epsilon).  Backward: out and stats are the
  // forward's, read only, and partials are rows of ld_p = 2*H*C floats
  AttnOut o;
  Drop drop;
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
  Sched t_sched;         // transposed graph + its schedule
  const int32_t* t_col;  // destination row of each transposed slot
  Drop t_drop;           // drop, keyed by the input edge id of each transposed slot
  AttnLayout lay;
  // edge features (EDGE kernels only): table [n_e, ld_e], the edge row of each forward / transposed
  // slot (e_idx null: the slot itself); a row outside [0, n_e) is a slot without a feature
  const float* e;
  int64_t ld_e;
  int32_t n_e;
  const int32_t* e_idx;
  const int32_t* t_e_idx;
  float* grad_e;  // backward: one row per kept slot's edge row, written by the destination pass
  int64_t ld_ge;
};

// k' = k + eps, v' = v + eps (eps = 0 for a slot without an edge row): one rounded add each.
template <int K>
__device__ __forceinline__ void add_edge(float (&k)[K], float (&v)[K], const float (&e)[K], bool has) {
#pragma unroll
  for (int c = 0; c < K; ++c) {
    const float x = has ? e[c] : 0.0f;
    k[c] += x;
    v[c] += x;
  }
}

// torch's softmax over a row's edges: no epsilon, so a row without edges is
// written as zeros, and -inf scores (masked edges) weigh exactly 0.
struct DotSoftmax {
  static constexpr bool kBias = false, kZeroEmptyRow = true;
  template <int K>
  static constexpr int fixup_batch() {
    return K >= 16 ? 8 : 16;  // B*K <= 128 registers of chunk loads in flight
  }
  static __device__ __forceinline__ double den(double l) { return l; }
  // -inf == -inf: nothing weighed yet, and expf(-inf - -inf) is NaN
  static __device__ __forceinline__ double rescale(float m, float m_new) {
    return m == m_new ? 1.0 : double(expf(m - m_new));
  }
  // exp(s - m) with a -inf score (or a chunk of them, which holds zeros) weighing 0 whatever m is;
  // +inf and NaN scores give NaN, which poisons their (row, head) only.
  static __device__ __forceinline__ float weight(float s, float m) {
    return s == -__builtin_inff() ? 0.0f : expf(s - m);
  }
};

template <int K, int U, bool EDGE>
__global__ __launch_bounds__(kBlock) void dot_attention_kernel(DotArgs a) {
  const HeadLanes<K> L(a.lay, a.H, a.C);
  const int64_t ngroups = group_count(a.lay.lgG);
  const int64_t n_work = a.sched.n_work();

  for (int64_t it = first_group(a.lay.lgG); it < n_work; it += ngroups) {
    int32_t row, beg, end, slot;
    work_item(a.sched, it, row, beg, end, slot);
    float qd[K];
    double acc[K];
    vload<K>(qd, a.q + int64_t(row) * a.ld_q + L.f);
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
      for (int u = 0; u < U; ++u) dm[u] = a.drop.multiplier(u < n ? e + u : end - 1, L.head);
      // unconditional loads from clamped addresses (edges past the end re-read the last one), masked on use
      float ks[U][K], vs[U][K];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        vload<K>(ks[u], a.k + row_off(j[u], a.ld_k) + L.f);
        vload<K>(vs[u], a.v + row_off(j[u], a.ld_v) + L.f);
      }
      if constexpr (EDGE) {  // the third row, loaded like the other two
        float es[U][K];
        bool he[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          int32_t r;
          he[u] = edge_row(a.e_idx, a.n_e, u < n ? e + u : end - 1, r);
          vload<K>(es[u], a.e + row_off(he[u] ? r : 0, a.ld_e) + L.f);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) add_edge<K>(ks[u], vs[u], es[u], he[u]);
      }
      float s[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float p = 0.0f;
#pragma unroll
        for (int c = 0; c < K; ++c) p += qd[c] * ks[u][c];
        // a padding lane's partial is dropped here, whatever it read (an inf of another head included)
        s[u] = a.scale * group_reduce(L.valid ? p : 0.0f, a.lay.LH);
      }
      softmax_block<K, U, DotSoftmax>(s, n, dm, vs, m, l, acc);
    }

    if (!L.valid) continue;
    if (slot >= 0) store_partial<K>(a.o, a.H, a.H * a.C, L, slot, m, l, acc);
    else finish_row<K, DotSoftmax>(a.o, a.H, L, row, m, l, acc, end <= beg);
  }
}

// Merges the chunk partials of split rows in chunk order.
template <int K>
__global__ __launch_bounds__(kBlock) void dot_attention_fixup_kernel(DotArgs a) {
  fixup_rows<K, DotSoftmax>(a.sched, a.lay, a.H, a.C, a.o);
}

// ---------------------------------------------------------------------------
// Backward.  With G = d loss / d out, D[i,h] = <G[i,h,:], out[i,h,:]> (holds
// under dropout: out contains the mask), p_e = exp(s_e - m) / l:
//   ds_e      = p_e (mask_e <G_i, v_j>_h - D[i,h])
//   grad_q[i] = scale sum_e ds_e k[j_e]                 destination pass
//   grad_v[j] = sum_{e: j_e = j} p_e mask_e G_i          source pass
//   grad_k[j] = scale sum_{e: j_e = j} ds_e q_i          source pass
// Both passes recompute s_e from q and k with the forward's operation order.
// EDGE: k' and v' stand for k[j_e] and v[j_e] throughout, formed by the
// forward's add, and the destination pass, which holds q_i and G_i and has
// ds_e and p_e per edge, stores
//   grad_e[eps_e] = scale ds_e q_i + p_e mask_e G_i
// (chunks of a split row store their own edges' rows: no partials).  The
// source pass gathers eps_e beside q_i and G_i.  The unroll stays the same:
// no instantiation spills (DESIGN.md §12 has the registers).
// ---------------------------------------------------------------------------
template <int K>
constexpr int bwd_unroll() {
  return K <= 4 ? 8 : (K == 8 ? 4 : 2);  // two K-wide rows per edge in flight: 64 registers
}

template <int K, bool EDGE>
__global__ __launch_bounds__(kBlock) void dot_attention_bwd_dst_kernel(DotArgs a) {
  constexpr int U = bwd_unroll<K>();
  const HeadLanes<K> L(a.lay, a.H, a.C);
  const int head = L.head, sub = L.sub, f = L.f, hh = L.head0();
  const bool valid = L.valid;
  const int64_t ngroups = group_count(a.lay.lgG);
  const int64_t n_work = a.sched.n_work();
  for (int64_t it = first_group(a.lay.lgG); it < n_work; it += ngroups) {
    int32_t row, beg, end, slot;
    work_item(a.sched, it, row, beg, end, slot);
    float qd[K], gr[K], o[K], gq[K];
    vload<K>(qd, a.q + int64_t(row) * a.ld_q + f);
    vload<K>(gr, a.grad + int64_t(row) * a.ld_g + f);
    vload<K>(o, a.o.out + int64_t(row) * a.o.ld_o + f);
    float dp = 0.0f;
#pragma unroll
    for (int c = 0; c < K; ++c) {
      gq[c] = 0.0f;
      dp += gr[c] * o[c];
    }
    const float D = group_reduce(valid ? dp : 0.0f, a.lay.LH);  // padding lanes' partials are dropped
    // every chunk of a split row computes the same D; the row's first chunk stores it
    if (valid && sub == 0 && (slot < 0 || beg == a.sched.rowptr[row])) a.dsum[int64_t(row) * a.H + head] = D;
    const float m = a.o.stats[int64_t(row) * 2 * a.H + hh];
    const float l = a.o.stats[int64_t(row) * 2 * a.H + a.H + hh];
    for (int32_t e = beg; e < end; e += U) {
      float ks[U][K], vs[U][K];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t j = a.col[e + u < end ? e + u : end - 1];
        vload<K>(ks[u], a.k + row_off(j, a.ld_k) + f);
        vload<K>(vs[u], a.v + row_off(j, a.ld_v) + f);
      }
      int32_t er[U];  // EDGE: the slot's edge row, -1 without one
      if constexpr (EDGE) {
        float es[U][K];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          int32_t r;
          const bool he = edge_row(a.e_idx, a.n_e, e + u < end ? e + u : end - 1, r);
          vload<K>(es[u], a.e + row_off(he ? r : 0, a.ld_e) + f);
          er[u] = he ? r : -1;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) add_edge<K>(ks[u], vs[u], es[u], er[u] >= 0);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float ps = 0.0f, pa = 0.0f;
#pragma unroll
        for (int c = 0; c < K; ++c) {
          ps += qd[c] * ks[u][c];
          pa += gr[c] * vs[u][c];
        }
        const float s = a.scale * group_reduce(valid ? ps : 0.0f, a.lay.LH);
        const float da = group_reduce(valid ? pa : 0.0f, a.lay.LH);
        if (e + u < end) {
          const float p = __fdiv_rn(DotSoftmax::weight(s, m), l);
          const float dmu = a.drop.multiplier(e + u, head);
          const float ds = p * (dmu * da - D);
#pragma unroll
          for (int c = 0; c < K; ++c) gq[c] += ds * ks[u][c];
          if constexpr (EDGE) {  // eps_e enters the score like k_j and the message like v_j: its one writer is here
            if (valid && er[u] >= 0) {
              const float sds = a.scale * ds, pm = p * dmu;
              float ge[K];
#pragma unroll
              for (int c = 0; c < K; ++c) ge[c] = sds * qd[c] + pm * gr[c];
              vstore<K>(a.grad_e + row_off(er[u], a.ld_ge) + f, ge);
            }
          }
        }
      }
    }
    if (!valid) continue;
#pragma unroll
    for (int c = 0; c < K; ++c) gq[c] *= a.scale;
    if (slot >= 0) vstore<K>(a.o.partials + int64_t(slot) * a.o.ld_p + f, gq);
    else vstore<K>(a.grad_q + int64_t(row) * a.ld_gq + f, gq);
  }
}

template <int K, bool EDGE>
__global__ __launch_bounds__(kBlock) void dot_attention_bwd_src_kernel(DotArgs a) {
  constexpr int U = bwd_unroll<K>();
  const HeadLanes<K> L(a.lay, a.H, a.C);
  const int head = L.head, f = L.f, hh = L.head0();
  const bool valid = L.valid;
  const int HC = a.H * a.C;
  const int64_t ngroups = group_count(a.lay.lgG);
  const int64_t n_work = a.t_sched.n_work();
  for (int64_t it = first_group(a.lay.lgG); it < n_work; it += ngroups) {
    int32_t j, beg, end, slot;
    work_item(a.t_sched, it, j, beg, end, slot);
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
        mv[u] = a.o.stats[row_off(i, 2 * a.H) + hh];
        lv[u] = a.o.stats[row_off(i, 2 * a.H) + a.H + hh];
        Dv[u] = a.dsum[row_off(i, a.H) + hh];
        vload<K>(qi[u], a.q + row_off(i, a.ld_q) + f);
        vload<K>(gi[u], a.grad + row_off(i, a.ld_g) + f);
      }
      float es[EDGE ? U : 1][K];  // EDGE: eps of each slot's edge, gathered beside q_i and G_i
      bool he[U];
      if constexpr (EDGE) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          int32_t r;
          he[u] = edge_row(a.t_e_idx, a.n_e, e + u < end ? e + u : end - 1, r);
          vload<K>(es[u], a.e + row_off(he[u] ? r : 0, a.ld_e) + f);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float ps = 0.0f, pa = 0.0f;
        if constexpr (EDGE) {
          float ke[K], ve[K];
#pragma unroll
          for (int c = 0; c < K; ++c) {
            ke[c] = kj[c];
            ve[c] = vj[c];
          }
          add_edge<K>(ke, ve, es[u], he[u]);
#pragma unroll
          for (int c = 0; c < K; ++c) {
            ps += qi[u][c] * ke[c];
            pa += gi[u][c] * ve[c];
          }
        } else {
#pragma unroll
          for (int c = 0; c < K; ++c) {
            ps += qi[u][c] * kj[c];
            pa += gi[u][c] * vj[c];
          }
        }
        const float s = a.scale * group_reduce(valid ? ps : 0.0f, a.lay.LH);
        const float da = group_reduce(valid ? pa : 0.0f, a.lay.LH);
        if (e + u < end) {
          const float p = __fdiv_rn(DotSoftmax::weight(s, mv[u]), lv[u]);
          const float dmu = a.t_drop.multiplier(e + u, head);
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
      float* p = a.o.partials + int64_t(slot) * a.o.ld_p;
      vstore<K>(p + f, gv);
      vstore<K>(p + HC + f, gk);
    } else {
      vstore<K>(a.grad_v + int64_t(j) * a.ld_gv + f, gv);
      vstore<K>(a.grad_k + int64_t(j) * a.ld_gk + f, gk);
    }
  }
}

// Edges per online-softmax rescale: 2 for K >= 4, measured at C3 (8 heads x 16,
// R-MAT 1M / 10M, forward medians of 20): K = 8: 1.43 ms at 2, 1.44 at 3, 1.51
// at 4; K = 4: 1.38 / 1.51 / 1.47; K = 16: 1.55 / 1.53 / not run.  Two rows per
// edge are already in flight, and 2 leaves K = 8 at 94 registers (5 waves per
// SIMD against 4 at 3).  K <= 2 (float2 / scalar fallback) keeps 4 and was not
// swept.  KGX_DOT_U overrides it for A/B runs (DESIGN.md §12 has the table),
// except with an edge table at K = 16: three rows of 16 at U = 3 or 4 do not
// fit 256 registers (the compiler parks 32 / 52 of them in AGPRs at one wave
// per SIMD), so those two are not built.
template <int K, bool EDGE>
int launch_fwd(const DotArgs& a, hipStream_t s) {
  if constexpr (EDGE && K == 16) {
    return launch_with_fixup(dot_attention_kernel<K, 2, EDGE>, dot_attention_fixup_kernel<K>, a, s);
  } else {
    static const int uf = env_int("KGX_DOT_U");
    const int U = (uf >= 2 && uf <= 4) ? uf : (K <= 2 ? 4 : 2);
    switch (U) {
      case 2: return launch_with_fixup(dot_attention_kernel<K, 2, EDGE>, dot_attention_fixup_kernel<K>, a, s);
      case 3: return launch_with_fixup(dot_attention_kernel<K, 3, EDGE>, dot_attention_fixup_kernel<K>, a, s);
      default: return launch_with_fixup(dot_attention_kernel<K, 4, EDGE>, dot_attention_fixup_kernel<K>, a, s);
    }
  }
}

// The destination pass sums one row per slot (grad_q), the source pass two (grad_v | grad_k).
template <int K, bool EDGE>
int launch_bwd(const DotArgs& a, hipStream_t s) {
  const int HC = a.H * a.C;
  if (const int rc = launch_resident(dot_attention_bwd_dst_kernel<K, EDGE>, a.sched.n_work(), a.lay.G, a, s)) return rc;
  if (const int rc = launch_chunk_sum(a.sched, a.o.partials, a.o.ld_p, HC, HC, a.grad_q, a.ld_gq, a.grad_q, a.ld_gq, s))
    return rc;
  if (const int rc = launch_resident(dot_attention_bwd_src_kernel<K, EDGE>, a.t_sched.n_work(), a.lay.G, a, s)) return rc;
  return launch_chunk_sum(a.t_sched, a.o.partials, a.o.ld_p, HC, 2 * HC, a.grad_v, a.ld_gv, a.grad_k, a.ld_gk, s);
}

}  // namespace
}  // namespace kgx

using namespace kgx;

extern "C" int kgx_dot_attention_edge(const int32_t* rowptr, const int32_t* rows, int64_t n_rows,
                                      const int32_t* items, int64_t n_items, const int32_t* split, int64_t n_split,
                                      const int32_t* col, const float* q, int64_t ld_q, const float* k,
                                      int64_t ld_k, const float* v, int64_t ld_v, const float* e, int64_t ld_e,
                                      int64_t n_e, const int32_t* e_idx, int heads, int channels, float scale,
                                      float* out, int64_t ld_out, float* partials, float* stats,
                                      const int32_t* drop_key, float drop_p, uint64_t drop_seed,
                                      kgx_stream_t stream_) {
  hipStream_t stream = as_stream(stream_);
  KGX_REQUIRE(heads > 0 && channels > 0 && n_rows >= 0 && n_items >= 0 && n_split >= 0, KGX_ERR_ARG,
              "kgx_dot_attention: bad sizes");
  const int64_t HC = int64_t(heads) * channels;
  const int64_t lim = int64_t(1) << 31;
  KGX_REQUIRE(!e || (n_e >= 0 && n_e < lim), KGX_ERR_ARG, "kgx_dot_attention: edge table rows outside [0, 2^31)");
  KGX_REQUIRE(!e || ld_e >= HC, KGX_ERR_ARG, "kgx_dot_attention: leading dimension of e < heads*channels");
  KGX_REQUIRE(!e || ld_e < lim, KGX_ERR_ARG, "kgx_dot_attention: leading dimension of e >= 2^31");
  if (n_rows == 0) return KGX_OK;
  if (e && n_e == 0) e = nullptr;  // no row to read: every slot is without a feature
  KGX_REQUIRE(rowptr && rows && col && q && k && v && out, KGX_ERR_ARG, "kgx_dot_attention: null pointer");
  KGX_REQUIRE(ld_q >= HC && ld_k >= HC && ld_v >= HC && ld_out >= HC, KGX_ERR_ARG,
              "kgx_dot_attention: leading dimension < heads*channels");
  KGX_REQUIRE(ld_q < lim && ld_k < lim && ld_v < lim && ld_out < lim, KGX_ERR_ARG,
              "kgx_dot_attention: leading dimension >= 2^31");
  KGX_REQUIRE_DROP_P(drop_p, "kgx_dot_attention");
  KGX_REQUIRE(!items || n_split == 0 || (split && partials), KGX_ERR_ARG,
              "kgx_dot_attention: split rows need split list and partials");
  const auto fits = [&](int b) {
    return attn_vec_ok(b, {q, k, v, out, partials, e}, {ld_q, ld_k, ld_v, ld_out, e ? ld_e : 0});
  };
  const bool vec4 = fits(16);
  int K = attn_pick_k(heads, channels, vec4, fits(8));
  KGX_REQUIRE(K > 0, KGX_ERR_UNSUPPORTED,
              "kgx_dot_attention: heads=%d x channels=%d needs more than 64 lanes per row (unsupported shape)", heads,
              channels);
  static const int kf = env_int("KGX_DOT_K");
  K = attn_knob_k(K, heads, channels, vec4, kf);
  DotArgs a{};
  a.sched = make_sched(rowptr, rows, n_rows, items, n_items, split, n_split);
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
  a.o = {out, ld_out, partials, attn_partial_ld(heads, channels), stats, nullptr};
  a.drop = make_drop(drop_key, drop_p, drop_seed);
  a.lay = attn_layout(heads, channels, K);
  if (!e) return dispatch_k(K, [&](auto kk) { return launch_fwd<decltype(kk)::value, false>(a, stream); });
  a.e = e;
  a.ld_e = ld_e;
  a.n_e = int32_t(n_e);
  a.e_idx = e_idx;
  return dispatch_k(K, [&](auto kk) { return launch_fwd<decltype(kk)::value, true>(a, stream); });
}

extern "C" int kgx_dot_attention(const int32_t* rowptr, const int32_t* rows, int64_t n_rows, const int32_t* items,
                                 int64_t n_items, const int32_t* split, int64_t n_split, const int32_t* col,
                                 const float* q, int64_t ld_q, const float* k, int64_t ld_k, const float* v,
                                 int64_t ld_v, int heads, int channels, float scale, float* out, int64_t ld_out,
                                 float* partials, float* stats, const int32_t* drop_key, float drop_p,
                                 uint64_t drop_seed, kgx_stream_t stream_) {
  return kgx_dot_attention_edge(rowptr, rows, n_rows, items, n_items, split, n_split, col, q, ld_q, k, ld_k, v, ld_v,
                                nullptr, 0, 0, nullptr, heads, channels, scale, out, ld_out, partials, stats,
                                drop_key, drop_p, drop_seed, stream_);
}

extern "C" int kgx_dot_attention_edge_backward(
    const int32_t* rowptr, const int32_t* rows, int64_t n_rows, const int32_t* items, int64_t n_items,
    const int32_t* split, int64_t n_split, const int32_t* col, const float* q, int64_t ld_q, const float* k,
    int64_t ld_k, const float* v, int64_t ld_v, const float* e, int64_t ld_e, int64_t n_e, const int32_t* e_idx,
    int heads, int channels, float scale, const float* out, int64_t ld_out, const float* stats,
    const float* grad_out, int64_t ld_grad, const int32_t* t_rowptr, const int32_t* t_rows, int64_t n_src,
    const int32_t* t_items, int64_t t_n_items, const int32_t* t_split, int64_t t_n_split, const int32_t* t_col,
    const int32_t* t_key, const int32_t* t_e_idx, float* grad_q, int64_t ld_gq, float* grad_k, int64_t ld_gk,
    float* grad_v, int64_t ld_gv, float* grad_e, int64_t ld_ge, float* dsum_ws, float* partials,
    const int32_t* drop_key, float drop_p, uint64_t drop_seed, kgx_stream_t stream_) {
  hipStream_t stream = as_stream(stream_);
  KGX_REQUIRE(heads > 0 && channels > 0 && n_rows >= 0 && n_src >= 0 && n_items >= 0 && n_split >= 0 &&
                  t_n_items >= 0 && t_n_split >= 0,
              KGX_ERR_ARG, "kgx_dot_attention_backward: bad sizes");
  const int64_t HC = int64_t(heads) * channels;
  const int64_t lim = int64_t(1) << 31;
  KGX_REQUIRE(!e || (n_e >= 0 && n_e < lim), KGX_ERR_ARG,
              "kgx_dot_attention_backward: edge table rows outside [0, 2^31)");
  KGX_REQUIRE(!e || (grad_e && t_e_idx), KGX_ERR_ARG,
              "kgx_dot_attention_backward: an edge table needs grad_e and t_e_idx");
  KGX_REQUIRE(!e || (ld_e >= HC && ld_ge >= HC), KGX_ERR_ARG,
              "kgx_dot_attention_backward: leading dimension of e or grad_e < heads*channels");
  KGX_REQUIRE(!e || (ld_e < lim && ld_ge < lim), KGX_ERR_ARG,
              "kgx_dot_attention_backward: leading dimension of e or grad_e >= 2^31");
  if (n_rows == 0 && n_src == 0) return KGX_OK;
  if (e && n_e == 0) e = nullptr;  // no row to read or write
  if (!e) grad_e = nullptr;
  KGX_REQUIRE(rowptr && rows && col && q && k && v && out && stats && grad_out && t_rowptr && t_rows && t_col &&
                  grad_q && grad_k && grad_v && dsum_ws,
              KGX_ERR_ARG, "kgx_dot_attention_backward: null pointer");
  KGX_REQUIRE(ld_q >= HC && ld_k >= HC && ld_v >= HC && ld_out >= HC && ld_grad >= HC && ld_gq >= HC &&
                  ld_gk >= HC && ld_gv >= HC,
              KGX_ERR_ARG, "kgx_dot_attention_backward: leading dimension < heads*channels");
  KGX_REQUIRE(ld_q < lim && ld_k < lim && ld_v < lim && ld_out < lim && ld_grad < lim && ld_gq < lim &&
                  ld_gk < lim && ld_gv < lim,
              KGX_ERR_ARG, "kgx_dot_attention_backward: leading dimension >= 2^31");
  KGX_REQUIRE_DROP_P(drop_p, "kgx_dot_attention_backward");
  const bool dropping = drop_key && drop_p > 0.0f;
  KGX_REQUIRE(!dropping || t_key, KGX_ERR_ARG, "kgx_dot_attention_backward: dropout needs t_key");
  KGX_REQUIRE((!items || n_split == 0 || split) && (!t_items || t_n_split == 0 || t_split), KGX_ERR_ARG,
              "kgx_dot_attention_backward: split rows need a split list");
  KGX_REQUIRE(((!items || n_split == 0) && (!t_items || t_n_split == 0)) || partials, KGX_ERR_ARG,
              "kgx_dot_attention_backward: split rows need partials");
  const auto fits = [&](int b) {
    return attn_vec_ok(b, {q, k, v, out, grad_out, grad_q, grad_k, grad_v, partials, e, grad_e},
                       {ld_q, ld_k, ld_v, ld_out, ld_grad, ld_gq, ld_gk, ld_gv, HC, e ? ld_e : 0, e ? ld_ge : 0});
  };
  const bool vec4 = fits(16);
  int K = attn_pick_k(heads, channels, vec4, fits(8));
  KGX_REQUIRE(K > 0, KGX_ERR_UNSUPPORTED,
              "kgx_dot_attention_backward: heads=%d x channels=%d needs more than 64 lanes per row (unsupported "
              "shape)",
              heads, channels);
  static const int kf = env_int("KGX_DOT_K");
  K = attn_knob_k(K, heads, channels, vec4, kf);
  DotArgs a{};
  a.sched = make_sched(rowptr, rows, n_rows, items, n_items, split, n_split);
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
  a.o = {const_cast<float*>(out), ld_out, partials, 2 * HC, const_cast<float*>(stats), nullptr};
  a.drop = make_drop(drop_key, drop_p, drop_seed);
  a.grad = grad_out;
  a.ld_g = ld_grad;
  a.dsum = dsum_ws;
  a.grad_q = grad_q;
  a.ld_gq = ld_gq;
  a.grad_k = grad_k;
  a.ld_gk = ld_gk;
  a.grad_v = grad_v;
  a.ld_gv = ld_gv;
  a.t_sched = make_sched(t_rowptr, t_rows, n_src, t_items, t_n_items, t_split, t_n_split);
  a.t_col = t_col;
  a.t_drop = make_drop(dropping ? t_key : nullptr, drop_p, drop_seed);
  a.lay = attn_layout(heads, channels, K);
  if (!e) return dispatch_k(K, [&](auto kk) { return launch_bwd<decltype(kk)::value, false>(a, stream); });
  a.e = e;
  a.ld_e = ld_e;
  a.n_e = int32_t(n_e);
  a.e_idx = e_idx;
  a.t_e_idx = t_e_idx;
  a.grad_e = grad_e;
  a.ld_ge = ld_ge;
  return dispatch_k(K, [&](auto kk) { return launch_bwd<decltype(kk)::value, true>(a, stream); });
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
  return kgx_dot_attention_edge_backward(rowptr, rows, n_rows, items, n_items, split, n_split, col, q, ld_q, k, ld_k,
                                         v, ld_v, nullptr, 0, 0, nullptr, heads, channels, scale, out, ld_out, stats,
                                         grad_out, ld_grad, t_rowptr, t_rows, n_src, t_items, t_n_items, t_split,
                                         t_n_split, t_col, t_key, nullptr, grad_q, ld_gq, grad_k, ld_gk, grad_v,
                                         ld_gv, nullptr, 0, dsum_ws, partials, drop_key, drop_p, drop_seed, stream_);
}
