// Fused GAT attention aggregation for the kgx engine (gfx950, wave64): PyG's
// GATConv, whose score separates into per-node (and per-edge) SCALARS per head:
//   z_e = (a_dst[i,h] + a_src[j,h]) + a_edge[e,h]     s_e = leaky_relu(z_e)
//   alpha_e = softmax over the in-edges of i (s_e)    out[i,h,:] = sum_e alpha_e drop_e h_src[j_e,h,:] (+ bias)
// The lane layout is the attention core's (kgx_attn.h): a group of G lanes owns
// a work item of the destination schedule, lane l holds K channels of head
// l / LH.  What the separable score removes against gatv2.hip: no h_dst row, no
// per-edge dot product over C channels and no cross-lane score reduction (every
// lane of a head forms the same scalar from two or three 4-byte loads), no
// projected [E, H*C] edge table, and no [E, H] alpha / ds pair kept for the
// backward, which recomputes p_e from the scalar tables and the saved stats.
//
// z is formed by exactly the two rounded fp32 adds above, in that order, in every
// kernel (the file is compiled with -ffp-contract=off), so leaky_relu' in the
// backward is taken at the forward's z and exp(s - m) never sees s > m.
//
// The forward's softmax is the online one of kgx_attn.h (softmax_block, U edges per rescale).  A two-sweep
// form (a scalar-only max sweep, then a rescale-free gather) measured 9-11 % slower: DESIGN.md §16.
// Hub chunks store [H*C acc | H m | H l] and the core's fix-up merges them in
// chunk order.
#include "kgx_attn.h"

namespace kgx {
namespace {

// PyG's softmax: exp(s - max) / (sum + 1e-16); otherwise the rules of GatSoftmax
// (gatv2.hip): the bias is added in the store, an empty row is 0 / 1e-16 (+ bias).
struct GatScalarSoftmax {
  static constexpr bool kBias = true, kZeroEmptyRow = false;
  template <int K>
  static constexpr int fixup_batch() {
    return 16;
  }
  static __device__ __forceinline__ double den(double l) { return l + 1e-16; }
  static __device__ __forceinline__ double rescale(float m, float m_new) { return double(expf(m - m_new)); }
  static __device__ __forceinline__ float weight(float s, float m) { return expf(s - m); }
};

// The scalar tables of both directions.  a_edge null: no edge term.
struct GatScalars {
  const float* a_src;
  int64_t ld_as;
  const float* a_dst;
  int64_t ld_ad;
  const float* a_edge;  // [n_e, ld_ae]; the edge row of a slot by edge_row()
  int64_t ld_ae;
  int32_t n_e;
  float slope;
  // z by the two rounded adds, and its leaky_relu
  __device__ __forceinline__ float z(float ad, float as, float ae, bool edge) const {
    float v = ad + as;
    if (edge) v = v + ae;
    return v;
  }
  __device__ __forceinline__ float lrelu(float v) const { return v > 0.0f ? v : v * slope; }
  // a_edge of slot t under index array idx: 0 for a slot without an edge row; r: that row or -1
  __device__ __forceinline__ float edge_term(const int32_t* idx, int32_t t, int head, int32_t& r) const {
    const bool has = edge_row(idx, n_e, t, r);
    const float v = a_edge[row_off(has ? r : 0, ld_ae) + head];  // unconditional load from a clamped address
    if (!has) r = -1;
    return has ? v : 0.0f;
  }
};

struct GatFwdArgs {
  Sched sched;
  const int32_t* col;
  const float* h_src;
  int64_t ld_h;
  GatScalars sc;
  const int32_t* e_idx;  // edge row of each slot (null: the slot itself)
  int H, C;
  AttnOut o;  // stats keep the denominator l + 1e-16
  Drop drop;
  AttnLayout lay;
};

// Edges per online-softmax block, as gatv2.hip.
template <int K>
constexpr int fwd_unroll() {
  return K <= 8 ? 3 : 2;
}

template <int K, bool kEdge>
__global__ __launch_bounds__(kBlock) void gat_kernel(GatFwdArgs a) {
  constexpr int U = fwd_unroll<K>();
  const HeadLanes<K> L(a.lay, a.H, a.C);
  const int hh = L.head < a.H ? L.head : a.H - 1;  // padding heads read a valid column and store nothing
  const int64_t ngroups = group_count(a.lay.lgG);
  const int64_t n_work = a.sched.n_work();
  const GatScalars& sc = a.sc;

  for (int64_t it = first_group(a.lay.lgG); it < n_work; it += ngroups) {
    int32_t row, beg, end, slot;
    work_item(a.sched, it, row, beg, end, slot);
    const float ad = sc.a_dst[int64_t(row) * sc.ld_ad + hh];
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    float m = -__builtin_inff();
    double l = 0.0;

    for (int32_t e = beg; e < end; e += U) {
      const int n = (end - e) < U ? (end - e) : U;
      int32_t c[U];
      float dm[U], as[U], ae[U], v[U][K], s[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t ee = u < n ? e + u : end - 1;  // edges past the end re-read the last one
        c[u] = a.col[ee];
        dm[u] = a.drop.multiplier(ee, L.head);
        int32_t r;
        ae[u] = kEdge ? sc.edge_term(a.e_idx, ee, hh, r) : 0.0f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        as[u] = sc.a_src[row_off(c[u], sc.ld_as) + hh];  // one address across the LH lanes of a head
        vload<K>(v[u], a.h_src + row_off(c[u], a.ld_h) + L.f);  // padding lanes read column 0 and use nothing
      }
#pragma unroll
      for (int u = 0; u < U; ++u) s[u] = sc.lrelu(sc.z(ad, as[u], ae[u], kEdge));
      softmax_block<K, U, GatScalarSoftmax>(s, n, dm, v, m, l, acc);
    }

    if (!L.valid) continue;
    if (slot >= 0) store_partial<K>(a.o, a.H, a.H * a.C, L, slot, m, l, acc);
    else finish_row<K, GatScalarSoftmax>(a.o, a.H, L, row, m, l, acc, end <= beg);
  }
}

template <int K>
__global__ __launch_bounds__(kBlock) void gat_fixup_kernel(GatFwdArgs a) {
  fixup_rows<K, GatScalarSoftmax>(a.sched, a.lay, a.H, a.C, a.o);
}

template <int K>
int launch_fwd(const GatFwdArgs& a, hipStream_t s) {
  if (a.sc.a_edge) return launch_with_fixup(gat_kernel<K, true>, gat_fixup_kernel<K>, a, s);
  return launch_with_fixup(gat_kernel<K, false>, gat_fixup_kernel<K>, a, s);
}

constexpr int64_t kLim = int64_t(1) << 31;

}  // namespace
}  // namespace kgx

using namespace kgx;

extern "C" int kgx_gat(const kgx_gat_args* p, kgx_stream_t stream_) {
  KGX_REQUIRE(p && p->struct_size == sizeof(kgx_gat_args), KGX_ERR_ARG,
              "kgx_gat: struct_size %llu is not this header's %zu", p ? (unsigned long long)p->struct_size : 0ull,
              sizeof(kgx_gat_args));
  hipStream_t stream = as_stream(stream_);
  const int heads = p->heads, channels = p->channels;
  KGX_REQUIRE(heads > 0 && channels > 0 && p->n_rows >= 0 && p->n_items >= 0 && p->n_split >= 0, KGX_ERR_ARG,
              "kgx_gat: bad sizes");
  const int64_t HC = int64_t(heads) * channels;
  const float* a_edge = p->a_edge;
  KGX_REQUIRE(!a_edge || (p->n_e >= 0 && p->n_e < kLim), KGX_ERR_ARG, "kgx_gat: edge table rows outside [0, 2^31)");
  KGX_REQUIRE(!a_edge || (p->ld_ae >= heads && p->ld_ae < kLim), KGX_ERR_ARG,
              "kgx_gat: leading dimension of a_edge < heads or >= 2^31");
  if (p->n_rows == 0) return KGX_OK;
  if (a_edge && p->n_e == 0) a_edge = nullptr;  // no row to read: every slot is without a feature
  KGX_REQUIRE(p->rowptr && p->rows && p->col && p->h_src && p->a_src && p->a_dst && p->out, KGX_ERR_ARG,
              "kgx_gat: null pointer");
  KGX_REQUIRE(p->ld_h >= HC && p->ld_out >= HC, KGX_ERR_ARG, "kgx_gat: leading dimension < heads*channels");
  KGX_REQUIRE(p->ld_as >= heads && p->ld_ad >= heads, KGX_ERR_ARG, "kgx_gat: leading dimension of a_src / a_dst < heads");
  KGX_REQUIRE(p->ld_h < kLim && p->ld_as < kLim, KGX_ERR_ARG, "kgx_gat: leading dimension >= 2^31");
  KGX_REQUIRE(!p->items || p->n_split == 0 || (p->split && p->partials), KGX_ERR_ARG,
              "kgx_gat: split rows need split list and partials");
  const auto fits = [&](int b) {  // the scalar tables are read one float at a time: no alignment asked of them
    return attn_vec_ok(b, {p->h_src, p->out, p->bias, p->partials}, {p->ld_h, p->ld_out});
  };
  const bool vec4 = fits(16);
  int K = attn_pick_k(heads, channels, vec4, fits(8));
  KGX_REQUIRE(K > 0, KGX_ERR_UNSUPPORTED,
              "kgx_gat: heads=%d x channels=%d needs more than 64 lanes per row (unsupported shape)", heads, channels);
  static const int kf = env_int("KGX_GAT_K");
  K = attn_knob_k(K, heads, channels, vec4, kf);
  KGX_REQUIRE_DROP_P(p->drop_p, "kgx_gat");
  GatFwdArgs a{};
  a.sched = make_sched(p->rowptr, p->rows, p->n_rows, p->items, p->n_items, p->split, p->n_split);
  a.col = p->col;
  a.h_src = p->h_src;
  a.ld_h = p->ld_h;
  a.sc = {p->a_src, p->ld_as, p->a_dst, p->ld_ad, a_edge, p->ld_ae, int32_t(a_edge ? p->n_e : 0), p->negative_slope};
  a.e_idx = p->e_idx;
  a.H = heads;
  a.C = channels;
  a.o = {p->out, p->ld_out, p->partials, attn_partial_ld(heads, channels), p->stats, p->bias};
  a.drop = make_drop(p->drop_key, p->drop_p, p->drop_seed);
  a.lay = attn_layout(heads, channels, K);
  return dispatch_k(K, [&](auto k) { return launch_fwd<decltype(k)::value>(a, stream); });
}

// ===========================================================================
// Backward (kgx_gat_backward).  With G = d loss / d out, D[i,h] = <G_i, out_i - bias>_h
// (= sum_e alpha_e drop_e <G_i, h_j>_h: no pass over edges) and (m, den) the saved stats:
//   p_e  = exp(s_e - m_i) / den_i            ds_e = p_e (drop_e <G_i, h_j>_h - D[i,h])
//   dz_e = ds_e leaky_relu'(z_e)             (leaky_relu'(0) = slope, as torch)
//   d h_src[j] = sum_{e: j_e = j} p_e drop_e G_i     d a_src[j,h] = sum_{e: j_e = j} dz_e
//   d a_dst[i,h] = sum_{e into i} dz_e               d a_edge[e,h] = dz_e
// ONE row gather per edge for the whole backward:
//   1. gat_bwd_d_kernel: node-sized, writes D [n_dst, H].
//   2. gat_bwd_src_kernel over the TRANSPOSED CSR and its own hub-split schedule:
//      the group holds h_src[j] and a_src[j,:], gathers G_i and the scalars of i,
//      forms <G_i, h_j>_h with group_reduce, accumulates d h_src[j] and
//      d a_src[j,:] (chunk partials [H*C | H], in-order fix-up), stores dz_e at
//      the edge's forward slot of a [kept, H] table and into its row of
//      d a_edge (one slot per edge row: one writer).
//   3. gat_bwd_dst_kernel: a group of lanes (heads x 8 slots) sums each work
//      item's contiguous dz slots into d a_dst by a fixed tree; hub rows by the
//      forward's chunks and the in-order fix-up.
// No atomics, one writer per element, a fixed summation order.
// ===========================================================================

namespace kgx {
namespace {

struct GatBwdArgs {
  Sched sched;    // destination CSR + its schedule (pass 3)
  Sched t_sched;  // transposed CSR + its schedule (pass 2)
  const int32_t* t_col;    // destination row of each transposed slot
  const int32_t* t_slot;   // forward CSR slot of each transposed slot
  const int32_t* t_e_idx;  // edge row of each transposed slot
  const float* h_src;
  int64_t ld_h;
  GatScalars sc;
  int H, C;
  const float* out;
  int64_t ld_out;
  const float* bias;
  const float* stats;  // [n_dst, 2H] from the forward
  const float* grad;
  int64_t ld_g;
  Drop t_drop;  // keyed by the input edge id of each transposed slot
  float* D;   // [n_dst, H]
  float* dz;  // [kept, H] in forward slot order
  float* t_partials;  // [t_slots, ld_tp]: [H*C d h_src | H d a_src]
  int64_t ld_tp;
  float* d_partials;  // [n_slots, H]
  float* grad_h_src;
  int64_t ld_gh;
  float* grad_a_src;
  int64_t ld_gas;
  float* grad_a_dst;
  int64_t ld_gad;
  float* grad_a_edge;
  int64_t ld_gae;
  AttnLayout lay;
  int lgHp, lgG2;  // pass 3: next_pow2(H) heads x slots per group
};

template <int K>
__global__ __launch_bounds__(kBlock) void gat_bwd_d_kernel(GatBwdArgs a) {
  const HeadLanes<K> L(a.lay, a.H, a.C);
  const int64_t ngroups = group_count(a.lay.lgG);
  for (int64_t row = first_group(a.lay.lgG); row < a.sched.n_rows; row += ngroups) {
    float gr[K], o[K];
    vload<K>(gr, a.grad + row * a.ld_g + L.f);
    vload<K>(o, a.out + row * a.ld_out + L.f);
    if (a.bias) {
      float b[K];
      vload<K>(b, a.bias + L.f);
#pragma unroll
      for (int k = 0; k < K; ++k) o[k] -= b[k];
    }
    float dp = 0.0f;
#pragma unroll
    for (int k = 0; k < K; ++k) dp += gr[k] * o[k];
    const float D = group_reduce(L.valid ? dp : 0.0f, a.lay.LH);  // padding lanes' partials are dropped
    if (L.valid && L.sub == 0) a.D[row * a.H + L.head] = D;
  }
}

template <int K>
constexpr int bwd_unroll() {
  return K <= 4 ? 8 : (K == 8 ? 4 : 2);
}

template <int K, bool kEdge>
__global__ __launch_bounds__(kBlock) void gat_bwd_src_kernel(GatBwdArgs a) {
  constexpr int U = bwd_unroll<K>();
  const HeadLanes<K> L(a.lay, a.H, a.C);
  const int head = L.head, f = L.f, H = a.H;
  const int hh = head < H ? head : H - 1;
  const bool writer = L.valid && L.sub == 0;  // one lane per head stores the head's scalars
  const int HC = H * a.C;
  const int64_t ngroups = group_count(a.lay.lgG);
  const int64_t n_work = a.t_sched.n_work();
  const GatScalars& sc = a.sc;
  for (int64_t it = first_group(a.lay.lgG); it < n_work; it += ngroups) {
    int32_t j, beg, end, slot;
    work_item(a.t_sched, it, j, beg, end, slot);
    float hj[K], acc[K];
    vload<K>(hj, a.h_src + int64_t(j) * a.ld_h + f);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      hj[k] = L.valid ? hj[k] : 0.0f;  // padding lanes add 0 to the head's <G, h>
      acc[k] = 0.0f;
    }
    const float as = sc.a_src[int64_t(j) * sc.ld_as + hh];
    float acc_a = 0.0f;
    for (int32_t e = beg; e < end; e += U) {
      float gr[U][K], ad[U], ae[U], mi[U], den[U], Dv[U], dm[U];
      int32_t fs[U], er[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t ee = e + u < end ? e + u : end - 1;
        const int32_t i = a.t_col[ee];
        fs[u] = a.t_slot[ee];
        er[u] = -1;
        ae[u] = kEdge ? sc.edge_term(a.t_e_idx, ee, hh, er[u]) : 0.0f;
        dm[u] = a.t_drop.multiplier(ee, head);
        ad[u] = sc.a_dst[row_off(i, sc.ld_ad) + hh];
        mi[u] = a.stats[row_off(i, 2 * H) + hh];
        den[u] = a.stats[row_off(i, 2 * H) + H + hh];
        Dv[u] = a.D[row_off(i, H) + hh];
        vload<K>(gr[u], a.grad + row_off(i, a.ld_g) + f);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float pa = 0.0f;
#pragma unroll
        for (int k = 0; k < K; ++k) pa += gr[u][k] * hj[k];
        const float gh = group_reduce(pa, a.lay.LH);  // every lane takes part; edges past the end are dropped below
        if (e + u < end) {
          const float z = sc.z(ad[u], as, ae[u], kEdge);  // the forward's two adds
          const float p = __fdiv_rn(expf(sc.lrelu(z) - mi[u]), den[u]);
          const float w = p * dm[u];  // the message weight
          const float dzv = p * (dm[u] * gh - Dv[u]) * (z > 0.0f ? 1.0f : sc.slope);
#pragma unroll
          for (int k = 0; k < K; ++k) acc[k] += w * gr[u][k];
          acc_a += dzv;
          if (writer) {
            a.dz[row_off(fs[u], H) + head] = dzv;
            if (kEdge && er[u] >= 0) a.grad_a_edge[row_off(er[u], a.ld_gae) + head] = dzv;
          }
        }
      }
    }
    if (!L.valid) continue;
    if (slot >= 0) {
      float* p = a.t_partials + int64_t(slot) * a.ld_tp;
      vstore<K>(p + f, acc);
      if (writer) p[HC + head] = acc_a;
    } else {
      vstore<K>(a.grad_h_src + int64_t(j) * a.ld_gh + f, acc);
      if (writer) a.grad_a_src[int64_t(j) * a.ld_gas + head] = acc_a;
    }
  }
}

// d a_dst: lane (stripe, head) of a group of S x Hp lanes sums dz of the item's slots stripe, stripe + S, ...,
// then the stripes are added by a fixed xor tree.
__global__ __launch_bounds__(kBlock) void gat_bwd_dst_kernel(GatBwdArgs a) {
  constexpr int U = 4;
  const int G2 = 1 << a.lgG2, Hp = 1 << a.lgHp, S = G2 >> a.lgHp;
  const int lane = threadIdx.x & (G2 - 1);
  const int head = lane & (Hp - 1), stripe = lane >> a.lgHp;
  const int hh = head < a.H ? head : a.H - 1;
  const int64_t ngroups = group_count(a.lgG2);
  const int64_t n_work = a.sched.n_work();
  for (int64_t it = first_group(a.lgG2); it < n_work; it += ngroups) {
    int32_t row, beg, end, slot;
    work_item(a.sched, it, row, beg, end, slot);
    float acc = 0.0f;
    for (int32_t e = beg + stripe; e < end; e += U * S) {
      float v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = a.dz[row_off(e + u * S < end ? e + u * S : end - 1, a.H) + hh];
#pragma unroll
      for (int u = 0; u < U; ++u) acc = e + u * S < end ? acc + v[u] : acc;
    }
    for (int off = Hp; off < G2; off <<= 1) acc += __shfl_xor(acc, off, 64);
    if (stripe == 0 && head < a.H) {
      if (slot >= 0) a.d_partials[int64_t(slot) * a.H + head] = acc;
      else a.grad_a_dst[int64_t(row) * a.ld_gad + head] = acc;
    }
  }
}

template <int K>
int launch_bwd(const GatBwdArgs& a, hipStream_t s) {
  const int HC = a.H * a.C;
  if (const int rc = launch_resident(gat_bwd_d_kernel<K>, a.sched.n_rows, a.lay.G, a, s)) return rc;
  const int rc = a.sc.a_edge ? launch_resident(gat_bwd_src_kernel<K, true>, a.t_sched.n_work(), a.lay.G, a, s)
                             : launch_resident(gat_bwd_src_kernel<K, false>, a.t_sched.n_work(), a.lay.G, a, s);
  if (rc) return rc;
  if (const int rc2 = launch_chunk_sum(a.t_sched, a.t_partials, a.ld_tp, HC, HC + a.H, a.grad_h_src, a.ld_gh,
                                       a.grad_a_src, a.ld_gas, s))
    return rc2;
  if (const int rc2 = launch_resident(gat_bwd_dst_kernel, a.sched.n_work(), 1 << a.lgG2, a, s)) return rc2;
  return launch_chunk_sum(a.sched, a.d_partials, a.H, a.H, a.H, a.grad_a_dst, a.ld_gad, a.grad_a_dst, a.ld_gad, s);
}

// Floats between the source pass's chunk partials [H*C | H]: whole float4s.
inline int64_t t_partial_ld(int heads, int channels) { return (int64_t(heads) * channels + heads + 3) / 4 * 4; }

struct BwdCarve {
  float *D, *dz, *t_partials, *d_partials;
  size_t bytes;
};
inline BwdCarve carve_bwd(void* ws, size_t cap, int64_t n_rows, int64_t n_kept, int64_t n_slots, int64_t t_n_slots,
                          int heads, int channels) {
  Carve c(ws, cap);
  BwdCarve b;
  b.D = c.take<float>(size_t(n_rows) * heads);
  b.dz = c.take<float>(size_t(n_kept) * heads);
  b.t_partials = c.take<float>(size_t(t_n_slots) * t_partial_ld(heads, channels));
  b.d_partials = c.take<float>(size_t(n_slots) * heads);
  b.bytes = c.used();
  return b;
}

}  // namespace
}  // namespace kgx

extern "C" int kgx_gat_backward_workspace_bytes(int64_t n_rows, int64_t n_kept, int64_t n_slots, int64_t t_n_slots,
                                                int heads, int channels, size_t* bytes) {
  KGX_REQUIRE(bytes && n_rows >= 0 && n_kept >= 0 && n_slots >= 0 && t_n_slots >= 0 && heads > 0 && channels > 0,
              KGX_ERR_ARG, "kgx_gat_backward_workspace_bytes: bad sizes");
  *bytes = carve_bwd(nullptr, 0, n_rows, n_kept, n_slots, t_n_slots, heads, channels).bytes;
  return KGX_OK;
}

extern "C" int kgx_gat_backward(const kgx_gat_backward_args* p, kgx_stream_t stream_) {
  KGX_REQUIRE(p && p->struct_size == sizeof(kgx_gat_backward_args), KGX_ERR_ARG,
              "kgx_gat_backward: struct_size %llu is not this header's %zu",
              p ? (unsigned long long)p->struct_size : 0ull, sizeof(kgx_gat_backward_args));
  hipStream_t stream = as_stream(stream_);
  const int heads = p->heads, channels = p->channels;
  KGX_REQUIRE(heads > 0 && channels > 0 && p->n_rows >= 0 && p->n_src >= 0 && p->n_items >= 0 && p->n_split >= 0 &&
                  p->t_n_items >= 0 && p->t_n_split >= 0 && p->n_kept >= 0 && p->n_kept < kLim && p->n_slots >= 0 &&
                  p->t_n_slots >= 0,
              KGX_ERR_ARG, "kgx_gat_backward: bad sizes");
  const int64_t HC = int64_t(heads) * channels;
  const float* a_edge = p->a_edge;
  KGX_REQUIRE(!a_edge || (p->n_e >= 0 && p->n_e < kLim), KGX_ERR_ARG,
              "kgx_gat_backward: edge table rows outside [0, 2^31)");
  KGX_REQUIRE(!a_edge || (p->grad_a_edge && p->t_e_idx), KGX_ERR_ARG,
              "kgx_gat_backward: an edge table needs grad_a_edge and t_e_idx");
  KGX_REQUIRE(!a_edge || (p->ld_ae >= heads && p->ld_gae >= heads && p->ld_ae < kLim && p->ld_gae < kLim), KGX_ERR_ARG,
              "kgx_gat_backward: leading dimension of a_edge or grad_a_edge < heads or >= 2^31");
  if (p->n_rows == 0 && p->n_src == 0) return KGX_OK;
  if (a_edge && p->n_e == 0) a_edge = nullptr;  // no row to read or write
  KGX_REQUIRE(p->rowptr && p->rows && p->t_rowptr && p->t_rows && p->h_src && p->a_src && p->a_dst && p->out &&
                  p->stats && p->grad_out && p->grad_h_src && p->grad_a_src && p->grad_a_dst,
              KGX_ERR_ARG, "kgx_gat_backward: null pointer");
  KGX_REQUIRE(p->n_kept == 0 || (p->t_col && p->t_slot), KGX_ERR_ARG, "kgx_gat_backward: null t_col / t_slot");
  KGX_REQUIRE(p->ld_h >= HC && p->ld_out >= HC && p->ld_grad >= HC && p->ld_gh >= HC, KGX_ERR_ARG,
              "kgx_gat_backward: leading dimension < heads*channels");
  KGX_REQUIRE(p->ld_as >= heads && p->ld_ad >= heads && p->ld_gas >= heads && p->ld_gad >= heads, KGX_ERR_ARG,
              "kgx_gat_backward: leading dimension of a scalar table < heads");
  KGX_REQUIRE(p->ld_h < kLim && p->ld_grad < kLim && p->ld_ad < kLim, KGX_ERR_ARG,
              "kgx_gat_backward: leading dimension >= 2^31");
  KGX_REQUIRE_DROP_P(p->drop_p, "kgx_gat_backward");
  const bool dropping = p->drop_p > 0.0f;
  KGX_REQUIRE(!dropping || p->t_key, KGX_ERR_ARG, "kgx_gat_backward: dropout needs t_key");
  const int64_t n_slots = p->items ? p->n_slots : 0, t_n_slots = p->t_items ? p->t_n_slots : 0;
  const BwdCarve ws = carve_bwd(p->workspace, size_t(p->workspace_bytes), p->n_rows, p->n_kept, n_slots, t_n_slots,
                                heads, channels);
  KGX_REQUIRE(p->workspace && p->workspace_bytes >= ws.bytes, KGX_ERR_ARG,
              "kgx_gat_backward: workspace of %llu bytes, %zu needed", (unsigned long long)p->workspace_bytes, ws.bytes);
  const auto fits = [&](int b) {
    return attn_vec_ok(b, {p->h_src, p->out, p->bias, p->grad_out, p->grad_h_src, p->workspace},
                       {p->ld_h, p->ld_out, p->ld_grad, p->ld_gh});
  };
  const int K = attn_pick_k(heads, channels, fits(16), fits(8));
  KGX_REQUIRE(K > 0, KGX_ERR_UNSUPPORTED,
              "kgx_gat_backward: heads=%d x channels=%d needs more than 64 lanes per row (unsupported shape)", heads,
              channels);
  GatBwdArgs a{};
  a.sched = make_sched(p->rowptr, p->rows, p->n_rows, p->items, p->n_items, p->split, p->n_split);
  a.t_sched = make_sched(p->t_rowptr, p->t_rows, p->n_src, p->t_items, p->t_n_items, p->t_split, p->t_n_split);
  a.t_col = p->t_col;
  a.t_slot = p->t_slot;
  a.t_e_idx = p->t_e_idx;
  a.h_src = p->h_src;
  a.ld_h = p->ld_h;
  a.sc = {p->a_src, p->ld_as, p->a_dst, p->ld_ad, a_edge, p->ld_ae, int32_t(a_edge ? p->n_e : 0), p->negative_slope};
  a.H = heads;
  a.C = channels;
  a.out = p->out;
  a.ld_out = p->ld_out;
  a.bias = p->bias;
  a.stats = p->stats;
  a.grad = p->grad_out;
  a.ld_g = p->ld_grad;
  a.t_drop = make_drop(dropping ? p->t_key : nullptr, p->drop_p, p->drop_seed);
  a.D = ws.D;
  a.dz = ws.dz;
  a.t_partials = ws.t_partials;
  a.ld_tp = t_partial_ld(heads, channels);
  a.d_partials = ws.d_partials;
  a.grad_h_src = p->grad_h_src;
  a.ld_gh = p->ld_gh;
  a.grad_a_src = p->grad_a_src;
  a.ld_gas = p->ld_gas;
  a.grad_a_dst = p->grad_a_dst;
  a.ld_gad = p->ld_gad;
  a.grad_a_edge = a_edge ? p->grad_a_edge : nullptr;
  a.ld_gae = p->ld_gae;
  a.lay = attn_layout(heads, channels, K);
  const int Hp = next_pow2(heads);
  a.lgHp = log2i(Hp);
  a.lgG2 = log2i(Hp * (Hp <= 8 ? 8 : 64 / Hp));
  return dispatch_k(K, [&](auto k) { return launch_bwd<decltype(k)::value>(a, stream); });
}
