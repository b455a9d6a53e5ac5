// Fused GATv2 attention aggregation for the kgx engine (gfx950, wave64).
//
// Reference (src/keras_geometric/layers/gatv2_conv.py) materialises, per layer,
// h_j and h_i ([E,H,C] gathers, :245-246), the per-edge scores (:277-284), a
// segment_max / take / exp / segment_sum / take / divide softmax (:291-311),
// alpha*h_j (:257-258) and a segment_sum over [E,H*C] (:313-335).  Here one
// group of G lanes owns a destination row; lane l holds K consecutive channels
// of head l/LH.  Each edge's source row is gathered ONCE; the score is a
// per-lane partial dot product reduced across the LH lanes of the head with
// xor-shuffles; the softmax is computed online (running max m, running sum l,
// rescaled accumulator), U edges per rescale.  HBM traffic is one h_src row per
// edge plus h_dst and out per row — the reference's E x (3 x H*C) intermediates
// never exist.
//
// Numerics: algebraically identical to the reference; the score reduction order
// over C, exp, and the division placement differ at the ulp level, so GATv2 is
// tolerance-checked (|a-b| <= 1e-5*max(1,|b|)), not bit-checked.  The softmax
// numerator and denominator are accumulated in fp64 (exact to ~1e-7 even on
// 10^5-edge hub rows; the fp64 FMAs are free in this HBM-bound kernel).
//
// With an edge table (kgx_gatv2_edge; PyG's GATv2Conv with edge_dim) a second
// row is gathered per edge and enters the score only: z = (h_dst[i] + h_src[j])
// + eps_e, two rounded adds in this order in the forward and both backward
// kernels, so lrelu'(z) is taken at the forward's z.  The message stays
// h_src[j].  The kernels are templated on that (kEdge), and the instantiations
// without it are the code of the op without edge features.
#include "kgx_attn.h"

namespace kgx {
namespace {

struct GatArgs {
  Sched sched;
  const int32_t* col;
  const float* h_src;
  const float* h_dst;
  int64_t ld_h;
  const float* att;
  int H, C;
  float slope;
  AttnOut o;  // stats keep the denominator l + 1e-10
  Drop drop;
  AttnLayout lay;
  // edge features (kEdge kernels only): table [n_e, ld_e], the edge row of each slot (e_idx null: the
  // slot itself); a row outside [0, n_e) is a slot without a feature
  const float* e;
  int64_t ld_e;
  int32_t n_e;
  const int32_t* e_idx;
};

// The reference's softmax: an epsilon-guarded denominator, plain exp weights
// (scores are finite), the bias added where a row is stored.
struct GatSoftmax {
  static constexpr bool kBias = true, kZeroEmptyRow = false;  // an empty row is 0 / 1e-10 (+ bias)
  template <int K>
  static constexpr int fixup_batch() {
    return 16;
  }
  static __device__ __forceinline__ double den(double l) { return l + 1e-10; }
  static __device__ __forceinline__ double rescale(float m, float m_new) { return double(expf(m - m_new)); }
  static __device__ __forceinline__ float weight(float s, float m) { return expf(s - m); }
};

template <int K, bool kEdge>
__global__ __launch_bounds__(kBlock) void gatv2_kernel(GatArgs a) {
  // edges per online-softmax block: 3 measured best at C3 (K = 4): 1.27 ms vs 1.41 at 8, 1.30 at 4
  constexpr int U = K <= 4 ? 3 : (K == 8 ? 3 : 2);
  const HeadLanes<K> L(a.lay, a.H, a.C);
  const int64_t ngroups = group_count(a.lay.lgG);
  const int64_t n_work = a.sched.n_work();

  float att[K];
#pragma unroll
  for (int k = 0; k < K; ++k) att[k] = 0.0f;
  if (L.valid) vload<K>(att, a.att + L.f);

  for (int64_t it = first_group(a.lay.lgG); it < n_work; it += ngroups) {
    int32_t row, beg, end, slot;
    work_item(a.sched, it, row, beg, end, slot);
    float hd[K];
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      hd[k] = 0.0f;
      acc[k] = 0.0;
    }
    if (L.valid) vload<K>(hd, a.h_dst + int64_t(row) * a.ld_h + L.f);
    float m = -__builtin_inff();
    double l = 0.0;

    for (int32_t e = beg; e < end; e += U) {
      const int n = (end - e) < U ? (end - e) : U;
      int32_t c[U];
#pragma unroll
      for (int u = 0; u < U; ++u) c[u] = a.col[u < n ? e + u : end - 1];
      float dm[U];  // attention dropout multiplier per edge (this lane's head)
#pragma unroll
      for (int u = 0; u < U; ++u) dm[u] = a.drop.multiplier(u < n ? e + u : end - 1, L.head);
      // unconditional loads from clamped addresses (padding lanes read column 0
      // of the row; edges past the end re-read the last one), zeroed on padding lanes
      float hs[U][K];
#pragma unroll
      for (int u = 0; u < U; ++u) vload<K>(hs[u], a.h_src + row_off(c[u], a.ld_h) + L.f);
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int k = 0; k < K; ++k) hs[u][k] = L.valid ? hs[u][k] : 0.0f;
      // kEdge: the slot's edge row, loaded like hs; padding lanes and slots without a feature select 0
      float ep[kEdge ? U : 1][K];
      if constexpr (kEdge) {
        bool he[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          int32_t r;
          he[u] = edge_row(a.e_idx, a.n_e, u < n ? e + u : end - 1, r);
          vload<K>(ep[u], a.e + row_off(he[u] ? r : 0, a.ld_e) + L.f);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int k = 0; k < K; ++k) ep[u][k] = (L.valid && he[u]) ? ep[u][k] : 0.0f;
      }
      float s[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float p = 0.0f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          float g = hd[k] + hs[u][k];
          if constexpr (kEdge) g += ep[u][k];
          const float z = g > 0.0f ? g : g * a.slope;  // leaky_relu
          p += z * att[k];
        }
        s[u] = group_reduce(p, a.lay.LH);
      }
      softmax_block<K, U, GatSoftmax>(s, n, dm, hs, m, l, acc);
    }

    if (!L.valid) continue;
    if (slot >= 0) store_partial<K>(a.o, a.H, a.H * a.C, L, slot, m, l, acc);
    else finish_row<K, GatSoftmax>(a.o, a.H, L, row, m, l, acc, end <= beg);
  }
}

// Merges the chunk partials of split rows in chunk order.
template <int K>
__global__ __launch_bounds__(kBlock) void gatv2_fixup_kernel(GatArgs a) {
  fixup_rows<K, GatSoftmax>(a.sched, a.lay, a.H, a.C, a.o);
}

}  // namespace
}  // namespace kgx

using namespace kgx;

extern "C" int kgx_gatv2_edge(const int32_t* rowptr, const int32_t* rows, int64_t n_rows, const int32_t* items,
                              int64_t n_items, const int32_t* split, int64_t n_split, const int32_t* col,
                              const float* h_src, const float* h_dst, int64_t ld_h, const float* e, int64_t ld_e,
                              int64_t n_e, const int32_t* e_idx, const float* att, int heads, int channels,
                              float negative_slope, float* out, int64_t ld_out, const float* bias,
                              float* partials, float* stats, const int32_t* drop_key, float drop_p,
                              uint64_t drop_seed, kgx_stream_t stream_) {
  hipStream_t stream = as_stream(stream_);
  KGX_REQUIRE(heads > 0 && channels > 0 && n_rows >= 0 && n_items >= 0 && n_split >= 0, KGX_ERR_ARG,
              "kgx_gatv2: bad sizes");
  const int64_t HC = int64_t(heads) * channels;
  const int64_t lim = int64_t(1) << 31;
  KGX_REQUIRE(!e || (n_e >= 0 && n_e < lim), KGX_ERR_ARG, "kgx_gatv2: edge table rows outside [0, 2^31)");
  KGX_REQUIRE(!e || ld_e >= HC, KGX_ERR_ARG, "kgx_gatv2: leading dimension of e < heads*channels");
  KGX_REQUIRE(!e || ld_e < lim, KGX_ERR_ARG, "kgx_gatv2: leading dimension of e >= 2^31");
  if (n_rows == 0) return KGX_OK;
  if (e && n_e == 0) e = nullptr;  // no row to read: every slot is without a feature
  KGX_REQUIRE(rowptr && rows && col && h_src && h_dst && att && out, KGX_ERR_ARG, "kgx_gatv2: null pointer");
  KGX_REQUIRE(ld_h >= HC && ld_out >= HC, KGX_ERR_ARG, "kgx_gatv2: leading dimension < heads*channels");
  KGX_REQUIRE(ld_h < (int64_t(1) << 31), KGX_ERR_ARG, "kgx_gatv2: leading dimension >= 2^31");
  KGX_REQUIRE(!items || n_split == 0 || (split && partials), KGX_ERR_ARG,
              "kgx_gatv2: split rows need split list and partials");
  const auto fits = [&](int b) {
    return attn_vec_ok(b, {h_src, h_dst, out, att, bias, partials, e}, {ld_h, ld_out, e ? ld_e : 0});
  };
  const bool vec4 = fits(16);
  int K = attn_pick_k(heads, channels, vec4, fits(8));
  KGX_REQUIRE(K > 0, KGX_ERR_UNSUPPORTED,
              "kgx_gatv2: heads=%d x channels=%d needs more than 64 lanes per row (unsupported shape)", heads,
              channels);
  static const int kf = env_int("KGX_GAT_K");
  K = attn_knob_k(K, heads, channels, vec4, kf);
  KGX_REQUIRE_DROP_P(drop_p, "kgx_gatv2");
  GatArgs a{};
  a.sched = make_sched(rowptr, rows, n_rows, items, n_items, split, n_split);
  a.col = col;
  a.h_src = h_src;
  a.h_dst = h_dst;
  a.ld_h = ld_h;
  a.att = att;
  a.H = heads;
  a.C = channels;
  a.slope = negative_slope;
  a.o = {out, ld_out, partials, attn_partial_ld(heads, channels), stats, bias};
  a.drop = make_drop(drop_key, drop_p, drop_seed);
  a.lay = attn_layout(heads, channels, K);
  if (!e) {
    return dispatch_k(K, [&](auto k) {
      constexpr int kK = decltype(k)::value;
      return launch_with_fixup(gatv2_kernel<kK, false>, gatv2_fixup_kernel<kK>, a, stream);
    });
  }
  a.e = e;
  a.ld_e = ld_e;
  a.n_e = int32_t(n_e);
  a.e_idx = e_idx;
  return dispatch_k(K, [&](auto k) {
    constexpr int kK = decltype(k)::value;
    return launch_with_fixup(gatv2_kernel<kK, true>, gatv2_fixup_kernel<kK>, a, stream);
  });
}

extern "C" int kgx_gatv2(const int32_t* rowptr, const int32_t* rows, int64_t n_rows, const int32_t* items,
                         int64_t n_items, const int32_t* split, int64_t n_split, const int32_t* col,
                         const float* h_src, const float* h_dst, int64_t ld_h, const float* att, int heads,
                         int channels, float negative_slope, float* out, int64_t ld_out, const float* bias,
                         float* partials, float* stats, const int32_t* drop_key, float drop_p,
                         uint64_t drop_seed, kgx_stream_t stream_) {
  return kgx_gatv2_edge(rowptr, rows, n_rows, items, n_items, split, n_split, col, h_src, h_dst, ld_h, nullptr, 0, 0,
                        nullptr, att, heads, channels, negative_slope, out, ld_out, bias, partials, stats, drop_key,
                        drop_p, drop_seed, stream_);
}

// ===========================================================================
// Backward (kgx_gatv2_backward).  Forward per destination row i, head h:
//   z_e = h_dst[i] + h_src[j_e];  s_e = sum_c att[c] lrelu(z_e[c]);
//   alpha_e = exp(s_e - m) / (sum_e' exp(s_e' - m) + 1e-10);
//   out_i = sum_e alpha_e h_src[j_e]  (+ bias)
// With G = d loss / d out (the max shift m carries a ~1e-10-relative term
// through the 1e-10 guard, ignored):
//   dalpha_e = <G_i, h_src[j_e]>_h;  ds_e = alpha_e (dalpha_e - D_i)
//   D_i      = sum_e alpha_e dalpha_e = <G_i, out_i - bias>_h   (no pass over edges)
//   dz_e[c]  = ds_e att[c] lrelu'(z_e[c])          (lrelu'(0) = slope, as torch)
//   d att[c] = sum_e ds_e lrelu(z_e[c]);  d h_dst[i] = sum_e dz_e
//   d h_src[j] = sum_{e: j_e = j} (alpha_e G_i + dz_e)
// The forward keeps (m, denominator) per row and head (kgx_gatv2 `stats`), so
// kernel A is ONE pass over a row's edges, and needs only row constants: hub
// rows are split into the forward's chunks (partial d h_dst rows + fix-up).
// Kernel A stores alpha and ds per (edge, head); kernel B walks the
// TRANSPOSED CSR (its own split schedule) and pulls d h_src -- no atomics
// except the H*C-float d att.
// kEdge (kgx_gatv2_edge_backward): z_e = (h_dst[i] + h_src[j_e]) + eps_e in
// both kernels, by the forward's two adds, and kernel A, which has ds_e per
// edge, stores d eps_e = dz_e into the edge's row of grad_e (chunks of a split
// row store their own edges' rows: no partials); kernel B gathers eps_e beside
// h_dst[i] and G_i.
// ===========================================================================

namespace kgx {
namespace {

struct GatBwdArgs {
  Sched sched;  // destination CSR + its schedule
  const int32_t* col;
  const float* h_src;
  const float* h_dst;
  int64_t ld_h;
  const float* att;
  int H, C;
  float slope;
  const float* out;  // forward output (bias included if bias != null)
  int64_t ld_out;
  const float* bias;
  const float* stats;  // [n, 2H] from the forward
  Drop drop;  // keyed per CSR slot
  const float* grad;
  int64_t ld_g;
  float* alpha;  // [E', H] CSR slot order
  float* ds;     // [E', H]
  float* grad_h_dst;
  int64_t ld_gd;
  float* grad_att;  // [H*C], atomically accumulated
  float* partials;  // [max(n_slots, t_n_slots), H*C]
  Sched t_sched;          // transposed graph + its schedule (kernel B)
  const int32_t* t_col;   // destination row of each transposed slot
  const int32_t* t_slot;  // forward CSR slot of each transposed slot
  float* grad_h_src;
  int64_t ld_gs;
  AttnLayout lay;
  // edge features (kEdge kernels only), as GatArgs; t_e_idx: the edge row of each transposed slot
  const float* e;
  int64_t ld_e;
  int32_t n_e;
  const int32_t* e_idx;
  const int32_t* t_e_idx;
  float* grad_e;  // one row per kept slot's edge row, written by the destination pass
  int64_t ld_ge;
};

// Edges in flight per step.  kEdge gathers one more K-wide row per edge: at K = 16 the unroll is
// halved so that no instantiation spills (DESIGN.md §13 has the registers).
template <int K, bool kEdge>
constexpr int bwd_unroll() {
  return K <= 4 ? 8 : ((kEdge && K == 16) ? 2 : 4);
}

template <int K, bool kEdge>
__global__ __launch_bounds__(kBlock) void gatv2_bwd_rows_kernel(GatBwdArgs a) {
  constexpr int U = bwd_unroll<K, kEdge>();
  const HeadLanes<K> L(a.lay, a.H, a.C);
  const int head = L.head, sub = L.sub, f = L.f;
  const bool valid = L.valid;
  const int HC = a.H * a.C;
  const int64_t ngroups = group_count(a.lay.lgG);
  const int64_t n_work = a.sched.n_work();
  float att[K], gatt[K];
  vload<K>(att, a.att + f);
#pragma unroll
  for (int k = 0; k < K; ++k) {
    gatt[k] = 0.0f;
    if (!valid) att[k] = 0.0f;
  }
  auto lrelu = [&](float g) { return g > 0.0f ? g : g * a.slope; };
  for (int64_t it = first_group(a.lay.lgG); it < n_work; it += ngroups) {
    int32_t row, beg, end, slot;
    work_item(a.sched, it, row, beg, end, slot);
    float hd[K], gr[K], o[K];
    vload<K>(hd, a.h_dst + int64_t(row) * a.ld_h + f);
    vload<K>(gr, a.grad + int64_t(row) * a.ld_g + f);
    vload<K>(o, a.out + int64_t(row) * a.ld_out + f);
    if (a.bias) {
      float b[K];
      vload<K>(b, a.bias + f);
#pragma unroll
      for (int k = 0; k < K; ++k) o[k] -= b[k];
    }
    if (!valid) {
#pragma unroll
      for (int k = 0; k < K; ++k) gr[k] = 0.0f;
    }
    float dp = 0.0f;
#pragma unroll
    for (int k = 0; k < K; ++k) dp += gr[k] * o[k];
    const float D = group_reduce(dp, a.lay.LH);
    const float m = a.stats[int64_t(row) * 2 * a.H + L.head0()];
    const float den = a.stats[int64_t(row) * 2 * a.H + a.H + L.head0()];
    float gd[K];
#pragma unroll
    for (int k = 0; k < K; ++k) gd[k] = 0.0f;
    for (int32_t e = beg; e < end; e += U) {
      float hs[U][K];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t ee = e + u < end ? e + u : end - 1;
        vload<K>(hs[u], a.h_src + row_off(a.col[ee], a.ld_h) + f);
      }
      // kEdge: eps of each slot (0 without an edge row) and the row its gradient goes to (-1: none)
      float ep[kEdge ? U : 1][K];
      int32_t er[kEdge ? U : 1];
      if constexpr (kEdge) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          int32_t r;
          const bool he = edge_row(a.e_idx, a.n_e, e + u < end ? e + u : end - 1, r);
          vload<K>(ep[u], a.e + row_off(he ? r : 0, a.ld_e) + f);
          er[u] = he ? r : -1;
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int k = 0; k < K; ++k) ep[u][k] = er[u] >= 0 ? ep[u][k] : 0.0f;
      }
      // z of the forward: (h_dst + h_src) + eps, the same two rounded adds
      auto zin = [&](int u, int k) {
        float g = hd[k] + hs[u][k];
        if constexpr (kEdge) g += ep[u][k];
        return g;
      };
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float ps = 0.0f, pa = 0.0f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          ps += lrelu(zin(u, k)) * att[k];
          pa += gr[k] * hs[u][k];
        }
        const float sc = group_reduce(ps, a.lay.LH);
        const float da = group_reduce(pa, a.lay.LH);
        if (e + u < end) {
          const float al = __fdiv_rn(expf(sc - m), den);
          // dropout: out = sum alpha*d*h, so d alpha = d * <G, h>; D = <G, out - b> already includes d
          const float dmu = a.drop.multiplier(e + u, head);
          const float dsv = al * (dmu * da - D);
#pragma unroll
          for (int k = 0; k < K; ++k) {
            const float g = zin(u, k);
            gd[k] += dsv * att[k] * (g > 0.0f ? 1.0f : a.slope);
            gatt[k] += dsv * lrelu(g);
          }
          if constexpr (kEdge) {  // d eps = dz: the slot's edge row has its one writer here
            if (valid && er[u] >= 0) {
              float ge[K];
#pragma unroll
              for (int k = 0; k < K; ++k) ge[k] = dsv * att[k] * (zin(u, k) > 0.0f ? 1.0f : a.slope);
              vstore<K>(a.grad_e + row_off(er[u], a.ld_ge) + f, ge);
            }
          }
          if (valid && sub == 0) {
            a.alpha[int64_t(e + u) * a.H + head] = al * dmu;  // the message weight kernel B pulls with
            a.ds[int64_t(e + u) * a.H + head] = dsv;
          }
        }
      }
    }
    if (!valid) continue;
    if (slot >= 0) vstore<K>(a.partials + int64_t(slot) * HC + f, gd);
    else vstore<K>(a.grad_h_dst + int64_t(row) * a.ld_gd + f, gd);
  }
  if (valid) {
#pragma unroll
    for (int k = 0; k < K; ++k) atomicAdd(a.grad_att + f + k, gatt[k]);
  }
}

template <int K, bool kEdge>
__global__ __launch_bounds__(kBlock) void gatv2_bwd_src_kernel(GatBwdArgs a) {
  constexpr int U = bwd_unroll<K, kEdge>();
  const HeadLanes<K> L(a.lay, a.H, a.C);
  const int head = L.head, f = L.f;
  const int HC = a.H * a.C;
  const int64_t ngroups = group_count(a.lay.lgG);
  const int64_t n_work = a.t_sched.n_work();
  if (!L.valid) return;  // no cross-lane work in this kernel
  float att[K];
  vload<K>(att, a.att + f);
  for (int64_t it = first_group(a.lay.lgG); it < n_work; it += ngroups) {
    int32_t j, beg, end, slot;
    work_item(a.t_sched, it, j, beg, end, slot);
    float hs[K], acc[K];
    vload<K>(hs, a.h_src + int64_t(j) * a.ld_h + f);
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0f;
    for (int32_t e = beg; e < end; e += U) {
      float gr[U][K], hd[U][K], al[U], dsv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t ee = e + u < end ? e + u : end - 1;
        const int32_t i = a.t_col[ee];
        const int32_t s = a.t_slot[ee];
        al[u] = a.alpha[row_off(s, a.H) + head];
        dsv[u] = a.ds[row_off(s, a.H) + head];
        vload<K>(gr[u], a.grad + row_off(i, a.ld_g) + f);
        vload<K>(hd[u], a.h_dst + row_off(i, a.ld_h) + f);
      }
      float ep[kEdge ? U : 1][K];  // kEdge: eps of each slot's edge, gathered beside h_dst[i] and G_i
      if constexpr (kEdge) {
        bool he[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          int32_t r;
          he[u] = edge_row(a.t_e_idx, a.n_e, e + u < end ? e + u : end - 1, r);
          vload<K>(ep[u], a.e + row_off(he[u] ? r : 0, a.ld_e) + f);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int k = 0; k < K; ++k) ep[u][k] = he[u] ? ep[u][k] : 0.0f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (e + u < end) {
#pragma unroll
          for (int k = 0; k < K; ++k) {
            float g = hd[u][k] + hs[k];
            if constexpr (kEdge) g += ep[u][k];  // lrelu' at the forward's z
            acc[k] += al[u] * gr[u][k] + dsv[u] * att[k] * (g > 0.0f ? 1.0f : a.slope);
          }
        }
      }
    }
    if (slot >= 0) vstore<K>(a.partials + int64_t(slot) * HC + f, acc);
    else vstore<K>(a.grad_h_src + int64_t(j) * a.ld_gs + f, acc);
  }
}

template <int K, bool kEdge>
int launch_bwd(const GatBwdArgs& a, hipStream_t s) {
  const int HC = a.H * a.C;
  if (const int rc = launch_resident(gatv2_bwd_rows_kernel<K, kEdge>, a.sched.n_work(), a.lay.G, a, s)) return rc;
  if (const int rc = launch_chunk_sum(a.sched, a.partials, HC, HC, HC, a.grad_h_dst, a.ld_gd, a.grad_h_dst, a.ld_gd, s))
    return rc;
  if (const int rc = launch_resident(gatv2_bwd_src_kernel<K, kEdge>, a.t_sched.n_work(), a.lay.G, a, s)) return rc;
  return launch_chunk_sum(a.t_sched, a.partials, HC, HC, HC, a.grad_h_src, a.ld_gs, a.grad_h_src, a.ld_gs, s);
}

}  // namespace
}  // namespace kgx

extern "C" int kgx_gatv2_edge_backward(
    const int32_t* rowptr, const int32_t* rows, int64_t n_rows, const int32_t* items, int64_t n_items,
    const int32_t* split, int64_t n_split, const int32_t* col, const float* h_src, const float* h_dst, int64_t ld_h,
    const float* e, int64_t ld_e, int64_t n_e, const int32_t* e_idx, const float* att, int heads, int channels,
    float negative_slope, const float* out, int64_t ld_out, const float* bias, const float* stats,
    const float* grad_out, int64_t ld_grad, const int32_t* t_rowptr, const int32_t* t_rows, int64_t n_src,
    const int32_t* t_items, int64_t t_n_items, const int32_t* t_split, int64_t t_n_split, const int32_t* t_col,
    const int32_t* t_slot, const int32_t* t_e_idx, float* grad_h_src, float* grad_h_dst, int64_t ld_grad_h,
    float* grad_att, float* grad_e, int64_t ld_ge, float* alpha_ws, float* ds_ws, float* partials,
    const int32_t* drop_key, float drop_p, uint64_t drop_seed, kgx_stream_t stream_) {
  hipStream_t stream = as_stream(stream_);
  KGX_REQUIRE(heads > 0 && channels > 0 && n_rows >= 0 && n_src >= 0 && n_items >= 0 && n_split >= 0 &&
                  t_n_items >= 0 && t_n_split >= 0,
              KGX_ERR_ARG, "kgx_gatv2_backward: bad sizes");
  const int64_t HC = int64_t(heads) * channels;
  const int64_t lim = int64_t(1) << 31;
  KGX_REQUIRE(!e || (n_e >= 0 && n_e < lim), KGX_ERR_ARG, "kgx_gatv2_backward: edge table rows outside [0, 2^31)");
  KGX_REQUIRE(!e || (grad_e && t_e_idx), KGX_ERR_ARG, "kgx_gatv2_backward: an edge table needs grad_e and t_e_idx");
  KGX_REQUIRE(!e || (ld_e >= HC && ld_ge >= HC), KGX_ERR_ARG,
              "kgx_gatv2_backward: leading dimension of e or grad_e < heads*channels");
  KGX_REQUIRE(!e || (ld_e < lim && ld_ge < lim), KGX_ERR_ARG,
              "kgx_gatv2_backward: leading dimension of e or grad_e >= 2^31");
  if (e && n_e == 0) e = nullptr;  // no row to read or write
  if (!e) grad_e = nullptr;
  KGX_REQUIRE(rowptr && rows && col && h_src && h_dst && att && out && stats && grad_out && t_rowptr && t_rows &&
                  t_col && t_slot && grad_h_src && grad_h_dst && grad_att && alpha_ws && ds_ws,
              KGX_ERR_ARG, "kgx_gatv2_backward: null pointer");
  KGX_REQUIRE(ld_h >= HC && ld_grad >= HC && ld_grad_h >= HC && ld_out >= HC, KGX_ERR_ARG,
              "kgx_gatv2_backward: leading dimension < heads*channels");
  KGX_REQUIRE(ld_h < (int64_t(1) << 31) && ld_grad < (int64_t(1) << 31), KGX_ERR_ARG,
              "kgx_gatv2_backward: leading dimension >= 2^31");
  KGX_REQUIRE(((!items || n_split == 0) && (!t_items || t_n_split == 0)) || partials, KGX_ERR_ARG,
              "kgx_gatv2_backward: split rows need partials");
  const auto fits = [&](int b) {
    return attn_vec_ok(b, {h_src, h_dst, att, grad_out, grad_h_src, grad_h_dst, out, bias, partials, e, grad_e},
                       {ld_h, ld_grad, ld_grad_h, ld_out, e ? ld_e : 0, e ? ld_ge : 0});
  };
  const int K = attn_pick_k_smallest(heads, channels, fits(16), fits(8));
  KGX_REQUIRE(K > 0, KGX_ERR_UNSUPPORTED,
              "kgx_gatv2_backward: heads=%d x channels=%d does not fit 64 lanes per row", heads, channels);
  KGX_REQUIRE_DROP_P(drop_p, "kgx_gatv2_backward");
  GatBwdArgs a{};
  a.sched = make_sched(rowptr, rows, n_rows, items, n_items, split, n_split);
  a.col = col;
  a.h_src = h_src;
  a.h_dst = h_dst;
  a.ld_h = ld_h;
  a.att = att;
  a.H = heads;
  a.C = channels;
  a.slope = negative_slope;
  a.out = out;
  a.ld_out = ld_out;
  a.bias = bias;
  a.stats = stats;
  a.drop = make_drop(drop_key, drop_p, drop_seed);
  a.grad = grad_out;
  a.ld_g = ld_grad;
  a.alpha = alpha_ws;
  a.ds = ds_ws;
  a.grad_h_dst = grad_h_dst;
  a.ld_gd = ld_grad_h;
  a.grad_att = grad_att;
  a.partials = partials;
  a.t_sched = make_sched(t_rowptr, t_rows, n_src, t_items, t_n_items, t_split, t_n_split);
  a.t_col = t_col;
  a.t_slot = t_slot;
  a.grad_h_src = grad_h_src;
  a.ld_gs = ld_grad_h;
  a.lay = attn_layout(heads, channels, K);
  if (!e) return dispatch_k(K, [&](auto k) { return launch_bwd<decltype(k)::value, false>(a, stream); });
  a.e = e;
  a.ld_e = ld_e;
  a.n_e = int32_t(n_e);
  a.e_idx = e_idx;
  a.t_e_idx = t_e_idx;
  a.grad_e = grad_e;
  a.ld_ge = ld_ge;
  return dispatch_k(K, [&](auto k) { return launch_bwd<decltype(k)::value, true>(a, stream); });
}

extern "C" int kgx_gatv2_backward(const int32_t* rowptr, const int32_t* rows, int64_t n_rows, const int32_t* items,
                                  int64_t n_items, const int32_t* split, int64_t n_split, const int32_t* col,
                                  const float* h_src, const float* h_dst, int64_t ld_h, const float* att, int heads,
                                  int channels, float negative_slope, const float* out, int64_t ld_out,
                                  const float* bias, const float* stats, const float* grad_out, int64_t ld_grad,
                                  const int32_t* t_rowptr, const int32_t* t_rows, int64_t n_src,
                                  const int32_t* t_items, int64_t t_n_items, const int32_t* t_split,
                                  int64_t t_n_split, const int32_t* t_col, const int32_t* t_slot,
                                  float* grad_h_src, float* grad_h_dst, int64_t ld_grad_h, float* grad_att,
                                  float* alpha_ws, float* ds_ws, float* partials, const int32_t* drop_key,
                                  float drop_p, uint64_t drop_seed, kgx_stream_t stream_) {
  return kgx_gatv2_edge_backward(rowptr, rows, n_rows, items, n_items, split, n_split, col, h_src, h_dst, ld_h,
                                 nullptr, 0, 0, nullptr, att, heads, channels, negative_slope, out, ld_out, bias,
                                 stats, grad_out, ld_grad, t_rowptr, t_rows, n_src, t_items, t_n_items, t_split,
                                 t_n_split, t_col, t_slot, nullptr, grad_h_src, grad_h_dst, ld_grad_h, grad_att,
                                 nullptr, 0, alpha_ws, ds_ws, partials, drop_key, drop_p, drop_seed, stream_);
}
