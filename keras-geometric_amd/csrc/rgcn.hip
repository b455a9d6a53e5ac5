// R-GCN: per-relation aggregate and transform in one pass (gfx950, wave64).
//
//   S_{i,r} = sum_{t in row i*R + r} x[col t]          (the composite CSR of graph.build_relation_csr)
//   out[i]  = bias + xroot[i] W_root + sum_r norm_{i,r} S_{i,r} W_r,   norm = 1 / |row| (mean) or 1 (sum)
//
// No reference counterpart (PyG's RGCNConv).  Unlike spmm_gemm.hip, whose lanes own
// whole rows and whose one W stays in registers for the launch, the weight here
// changes with the relation, so the roles are turned round: the ACCUMULATORS stay
// in registers for the whole tile and the operands stream past them.
//
//   * wfrag::prep_kernel (kgx_wfrag.h) splits W [R, F_in, F_out] and W_root once per call into three
//     bf16 planes (kgx_bf16x3.h, split3_a) stored in MFMA fragment order: fragment
//     (r, kc, cb, plane) is 64 lanes x 16 bytes, lane (m, q) holding column 16 cb + m,
//     k = 32 kc + 8 q .. + 7.  Every tile reads ready fragments (L2) and never splits W.
//   * rgcn_tile_kernel: a block owns a tile of kM = 64 PIECES (node, slot range); all
//     four waves hold the tile's (lo, hi) of every piece for relation r in lane l =
//     piece l, so the tile's 64-bit "non-empty" mask is one ballot, the same in every
//     wave, and a relation no piece of the tile uses costs one load and one ballot: no
//     gather, no W read, no MFMA, no barrier.  Otherwise wave w gathers pieces 16 w ..
//     16 w + 15: a lane group of G = 8 / 16 / 32 lanes (one float4 column each) sums a
//     piece's slots in CSR order, kU rows in flight, absent rows read from the zero row
//     (full exec), scales by the PAIR's degree, splits the sums three ways and writes
//     bf16 planes [3][64][32 KC + 8] to LDS.  After the barrier wave w multiplies the
//     whole tile with ITS column blocks cb = w, w + 4, ..: W_r^T (A operand, from the
//     workspace) times tile^T (B operand, from LDS) on v_mfma_f32_16x16x32_bf16, six
//     significant products, into f32 accumulators [NCBW][4 row blocks] that live in
//     registers across all relations; a 16-piece block with no slot of r is skipped.
//     The root term is relation R: xroot rows against W_root.  A whole-node piece adds
//     bias and stores its row; a piece of a split node stores a partial row (root and
//     bias in the node's first piece) and wfrag::fixup_kernel adds a node's partials in
//     piece order.  No atomics: one writer per element, the same bits from run to run.
#include <hip/hip_runtime.h>

// No packed f32 VALU (v_pk_add_f32 and kin) in this file, as in edge_mp.hip: the feature is taken off every
// function of the device pass, the shared helpers included; the Makefile adds -fno-slp-vectorize.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#include "kgx_bf16x3.h"
#include "kgx_internal.h"
#include "kgx_mfma.h"
#include "kgx_wfrag.h"

namespace kgx {
namespace {

using namespace wfrag;  // Planes, mfma6, split4, the prep and fix-up kernels (shared with nnconv.hip)

constexpr int kM = 64;        // pieces per tile: one per lane of a wave (the tile mask is one ballot)
constexpr int kRB = kM / 16;  // 16-piece MFMA row blocks
constexpr int kWaves = kBlock / 64;
constexpr int kU = 4;         // gathered rows in flight per lane group
constexpr int kPadK = 8;      // bf16 of padding per A-tile row: 16 rows of a fragment read fall on 64 banks
constexpr int kMaxFin = 128, kMaxFout = 256;

struct TileArgs {
  const int32_t* rowptr;  // [n_rows * R + 1]
  const int32_t* col;
  const int32_t* pieces;  // [n_pieces][3]: node, slot_begin, slot_end; the first n_split belong to split nodes
  int64_t n_pieces, n_split;
  int R, F_in, F_out, KC, NCB, mean;
  const float* x;
  uint32_t ld_x;  // < 2^31 (checked at the entry point)
  const float* xroot;
  uint32_t ld_r;
  const short* wf;  // W fragments: [(R + 1) KC NCB][3][kFrag]
  const float* bias;
  float* out;
  uint32_t ld_o;
  float* part;  // [n_split][F_out]
};

// The sum of one piece's slots [s, h) of the current relation, in CSR order, for this lane's four columns.
// The loop count is wave-uniform (the longest of the wave's groups); a group past its end, and a lane past
// F_in, read the zero row, so every lane issues every load.  ROOT: the one row xroot[node].
template <bool ROOT>
__device__ __forceinline__ float4 gather_sum(const TileArgs& a, int32_t s, int32_t h, int32_t node, int c4, bool col_ok) {
  float4 sum = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if constexpr (ROOT) {
    const float* p = (s < h && col_ok) ? a.xroot + row_off(node, a.ld_r) + c4 : kgx_zero_row + c4;
    return ld4(p);
  } else {
    while (__ballot(s < h) != 0) {
      int32_t ci[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) ci[u] = a.col[s + u < h ? s + u : 0];  // slot 0 exists: some piece has a slot
      float4 v[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const float* p = (s + u < h && col_ok) ? a.x + row_off(ci[u], a.ld_x) + c4 : kgx_zero_row + c4;
        v[u] = ld4(p);
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const bool ok = s + u < h;
        sum.x = ok ? __fadd_rn(sum.x, v[u].x) : sum.x;
        sum.y = ok ? __fadd_rn(sum.y, v[u].y) : sum.y;
        sum.z = ok ? __fadd_rn(sum.z, v[u].z) : sum.z;
        sum.w = ok ? __fadd_rn(sum.w, v[u].w) : sum.w;
      }
      s += kU;
    }
    return sum;
  }
}

// NCBW: 16-column blocks per wave (wave w owns blocks w, w + 4, ..): 1 for F_out <= 64, 2 to 128, 4 to 256.
// 3 waves per SIMD asked of the register allocator: what the LDS tile of F_in = 128 (52 KB) lets a CU hold.
template <int NCBW>
__global__ __launch_bounds__(kBlock, 3) void rgcn_tile_kernel(TileArgs a) {
  extern __shared__ __attribute__((aligned(16))) short tile[];  // [3 planes][kM][ldk]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n = lane & 15, q = lane >> 4;
  const int ldk = a.KC * 32 + kPadK, plane = kM * ldk;
  // lane groups of the gather: G lanes cover 4 G >= 32 KC >= F_in columns
  const int lg = a.F_in > 64 ? 5 : (a.F_in > 32 ? 4 : 3);
  const int G = 1 << lg, NG = 64 >> lg;
  const int grp = lane >> lg, c4 = 4 * (lane & (G - 1));
  const bool col_ok = c4 < a.F_in, k_ok = c4 < a.KC * 32;

  // lane l holds piece l of the tile
  const int64_t p0 = int64_t(blockIdx.x) * kM;
  int32_t node = -1, sb = 0, se = 0;
  if (p0 + lane < a.n_pieces) {
    const int32_t* pc = a.pieces + (p0 + lane) * 3;
    node = pc[0], sb = pc[1], se = pc[2];
  }
  const int32_t* rp = a.rowptr + int64_t(node < 0 ? 0 : node) * a.R;  // the node's R pair rows
  int32_t rb_cur = rp[0], re_cur = rp[1];                             // pair (node, 0); R >= 1
  const bool first = node >= 0 && sb == rb_cur;                       // the node's first (or only) piece

  f32x4_t acc[NCBW][kRB];
#pragma unroll
  for (int j = 0; j < NCBW; ++j)
#pragma unroll
    for (int b = 0; b < kRB; ++b) acc[j][b] = f32x4_t{0.0f, 0.0f, 0.0f, 0.0f};

  uint32_t stale = 0xffffu;  // this wave's tile rows that do not hold zeros (all, before the first write)
  const int n_rel = a.xroot ? a.R + 1 : a.R;
  for (int r = 0; r < n_rel; ++r) {
    const bool root = r == a.R;
    int32_t lo, hi, cnt;
    if (!root) {
      const int32_t b = rb_cur, e = re_cur;
      rb_cur = e;
      re_cur = rp[r + 2 <= a.R ? r + 2 : a.R];  // the next pair's end: in flight across this relation
      lo = sb > b ? sb : b;
      hi = se < e ? se : e;
      cnt = e - b;
      if (node < 0) lo = hi = 0;
    } else {
      lo = 0, hi = first ? 1 : 0, cnt = 1;
    }
    const uint64_t tmask = __ballot(lo < hi);  // the same in all four waves
    if (tmask == 0) continue;

    const uint32_t m16 = uint32_t(tmask >> (16 * wave)) & 0xffffu;
    if (m16) {  // this wave's row block is multiplied: every row of it is current or zero
      const uint32_t work = m16 | stale;
      for (int st = 0; st < 16; st += NG) {
        if (((work >> st) & ((1u << NG) - 1u)) == 0) continue;  // wave-uniform
        const int pi = st + grp;                                // NG <= 8: pi < 16
        const int src = 16 * wave + pi;
        const int32_t s = __shfl(lo, src, 64), h = __shfl(hi, src, 64), c = __shfl(cnt, src, 64);
        const int32_t nd = __shfl(node, src, 64);
        float4 sum = root ? gather_sum<true>(a, s, h, nd, c4, col_ok) : gather_sum<false>(a, s, h, nd, c4, col_ok);
        if (a.mean && c > 1) {  // the pair's full degree, not the piece's
          const float d = float(c);
          sum = make_float4(__fdiv_rn(sum.x, d), __fdiv_rn(sum.y, d), __fdiv_rn(sum.z, d), __fdiv_rn(sum.w, d));
        }
        if (k_ok && ((work >> pi) & 1u)) {
          uint32_t ph[2], pm[2], pl[2];
          split4(sum, ph, pm, pl);
          short* row = tile + src * ldk + c4;
          *reinterpret_cast<uint2*>(row) = make_uint2(ph[0], ph[1]);
          *reinterpret_cast<uint2*>(row + plane) = make_uint2(pm[0], pm[1]);
          *reinterpret_cast<uint2*>(row + 2 * plane) = make_uint2(pl[0], pl[1]);
        }
      }
      stale = m16;
    }
    lds_barrier();

    const short* wr = a.wf + int64_t(r) * a.KC * a.NCB * 3 * kFrag + lane * 8;
#pragma unroll 1
    for (int kc = 0; kc < a.KC; ++kc) {
#pragma unroll
      for (int j = 0; j < NCBW; ++j) {
        const int cb = wave + kWaves * j;
        if (cb >= a.NCB) continue;  // wave-uniform
        const short* f = wr + (int64_t(kc) * a.NCB + cb) * 3 * kFrag;
        const Planes w{ld8(f), ld8(f + kFrag), ld8(f + 2 * kFrag)};
#pragma unroll
        for (int b = 0; b < kRB; ++b) {
          if (((tmask >> (16 * b)) & 0xffffu) == 0) continue;  // no piece of this row block has a slot of r
          const short* ar = tile + (16 * b + n) * ldk + kc * 32 + 8 * q;
          const Planes s{ld8(ar), ld8(ar + plane), ld8(ar + 2 * plane)};
          acc[j][b] = mfma6(w, s, acc[j][b]);
        }
      }
    }
    lds_barrier();  // the tile is read before the next relation overwrites it
  }

  // lane (n, q) holds piece 16 b + n, columns 16 cb + 4 q .. + 3
#pragma unroll
  for (int b = 0; b < kRB; ++b) {
    const int src = 16 * b + n;
    const int32_t nd = __shfl(node, src, 64);
    const bool fst = __shfl(int(first), src, 64) != 0;
    const int64_t pidx = p0 + src;
    const bool whole = pidx >= a.n_split;
#pragma unroll
    for (int j = 0; j < NCBW; ++j) {
      const int c = 16 * (wave + kWaves * j) + 4 * q;
      if (nd < 0 || c >= a.F_out) continue;
      f32x4_t v = acc[j][b];
      if (a.bias && (whole || fst)) {
        const float4 bb = ld4(a.bias + c);
        v = f32x4_t{__fadd_rn(v[0], bb.x), __fadd_rn(v[1], bb.y), __fadd_rn(v[2], bb.z), __fadd_rn(v[3], bb.w)};
      }
      float* dst = whole ? a.out + row_off(nd, a.ld_o) + c : a.part + pidx * a.F_out + c;
      *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
}

constexpr int64_t kInt32Limit = int64_t(1) << 31;

size_t rgcn_frag_bytes(int64_t R, int64_t F_in, int64_t F_out) { return frag_bytes(R + 1, F_in, F_out); }
size_t workspace_bytes(int64_t n_split, int64_t R, int64_t F_in, int64_t F_out) {
  return rgcn_frag_bytes(R, F_in, F_out) + align_up(size_t(n_split) * size_t(F_out) * sizeof(float), 256);
}
bool shape_ok(int64_t F_in, int64_t F_out) {
  return F_in >= 4 && F_in <= kMaxFin && F_in % 4 == 0 && F_out >= 4 && F_out <= kMaxFout && F_out % 4 == 0;
}

template <int NCBW>
int launch_tiles(const TileArgs& a, hipStream_t s) {
  const int64_t tiles = (a.n_pieces + kM - 1) / kM;
  const size_t lds = size_t(3) * kM * (a.KC * 32 + kPadK) * sizeof(short);
  hipLaunchKernelGGL(rgcn_tile_kernel<NCBW>, dim3(unsigned(tiles)), dim3(kBlock), lds, s, a);
  KGX_CHECK_LAUNCH();
  return KGX_OK;
}

}  // namespace
}  // namespace kgx

using namespace kgx;

extern "C" int kgx_rgcn_workspace_bytes(int64_t n_pieces, int64_t n_split_pieces, int64_t R, int64_t F_in, int64_t F_out,
                                        size_t* bytes) {
  KGX_REQUIRE(bytes && n_pieces >= 0 && n_split_pieces >= 0 && n_split_pieces <= n_pieces && n_pieces < kInt32Limit &&
                  R >= 1 && R < kInt32Limit,
              KGX_ERR_ARG, "kgx_rgcn_workspace_bytes: n_pieces %lld, n_split_pieces %lld, R %lld", (long long)n_pieces,
              (long long)n_split_pieces, (long long)R);
  KGX_REQUIRE(shape_ok(F_in, F_out), KGX_ERR_UNSUPPORTED,
              "kgx_rgcn_workspace_bytes: F_in = %lld, F_out = %lld (multiples of 4, F_in in [4, 128], F_out in [4, 256])",
              (long long)F_in, (long long)F_out);
  *bytes = workspace_bytes(n_split_pieces, R, F_in, F_out);
  return KGX_OK;
}

extern "C" int kgx_rgcn_run(const kgx_rgcn_args* p, kgx_stream_t stream_) {
  KGX_REQUIRE(p && p->struct_size == sizeof(kgx_rgcn_args), KGX_ERR_ARG,
              "kgx_rgcn_run: struct_size %llu is not this header's %zu", p ? (unsigned long long)p->struct_size : 0ull,
              sizeof(kgx_rgcn_args));
  const char* fn = "kgx_rgcn_run";
  KGX_REQUIRE(p->R >= 1 && p->n_rows >= 0 && p->n_rows * p->R < kInt32Limit, KGX_ERR_ARG,
              "%s: R = %lld, n_rows = %lld (R >= 1 and n_rows * R < 2^31)", fn, (long long)p->R, (long long)p->n_rows);
  KGX_REQUIRE(p->n_pieces >= p->n_rows && p->n_pieces < kInt32Limit && p->n_split_pieces >= 0 &&
                  p->n_split_pieces <= p->n_pieces,
              KGX_ERR_ARG, "%s: n_pieces = %lld, n_split_pieces = %lld for %lld rows (every row has a piece)", fn,
              (long long)p->n_pieces, (long long)p->n_split_pieces, (long long)p->n_rows);
  KGX_REQUIRE(p->F_in >= 1 && p->F_out >= 1 && p->ld_x >= p->F_in && p->ld_out >= p->F_out &&
                  (!p->W_root || p->ld_xroot >= p->F_in),
              KGX_ERR_ARG, "%s: leading dimension below the width (ld_x %lld, ld_xroot %lld, ld_out %lld)", fn,
              (long long)p->ld_x, (long long)p->ld_xroot, (long long)p->ld_out);
  KGX_REQUIRE(p->ld_x < kInt32Limit && p->ld_xroot < kInt32Limit && p->ld_out < kInt32Limit, KGX_ERR_ARG,
              "%s: a leading dimension >= 2^31", fn);
  KGX_REQUIRE(shape_ok(p->F_in, p->F_out), KGX_ERR_UNSUPPORTED,
              "%s: F_in = %lld, F_out = %lld (multiples of 4, F_in in [4, 128], F_out in [4, 256])", fn,
              (long long)p->F_in, (long long)p->F_out);
  if (p->n_rows == 0) return KGX_OK;
  KGX_REQUIRE(p->rowptr && p->pieces && p->x && p->W && p->out && (!p->W_root || p->xroot), KGX_ERR_ARG,
              "%s: null pointer (W_root needs xroot)", fn);
  KGX_REQUIRE(aligned16(p->x) && aligned16(p->out) && aligned16(p->xroot) && aligned16(p->bias) && p->ld_x % 4 == 0 &&
                  p->ld_out % 4 == 0 && p->ld_xroot % 4 == 0,
              KGX_ERR_UNSUPPORTED,
              "%s: x, xroot, out and bias are accessed four floats at a time: 16-byte aligned addresses and leading "
              "dimensions that are multiples of 4", fn);
  const size_t need = workspace_bytes(p->n_split_pieces, p->R, p->F_in, p->F_out);
  KGX_REQUIRE(p->workspace && aligned16(p->workspace) && p->workspace_bytes >= need, KGX_ERR_ARG,
              "%s: workspace of %llu bytes, needs %zu (16-byte aligned)", fn, (unsigned long long)p->workspace_bytes, need);
  hipStream_t stream = as_stream(stream_);

  PrepArgs w{};
  w.W = p->W, w.extra[0] = p->W_root, w.n_extra = 1, w.R = int(p->R), w.F_in = int(p->F_in), w.F_out = int(p->F_out);
  w.KC = k_chunks(p->F_in), w.NCB = col_blocks(p->F_out), w.wf = static_cast<short*>(p->workspace);
  if (const int prc = launch_prep(w, stream); prc != KGX_OK) return prc;

  TileArgs a{};
  a.rowptr = p->rowptr, a.col = p->col, a.pieces = p->pieces, a.n_pieces = p->n_pieces, a.n_split = p->n_split_pieces;
  a.R = w.R, a.F_in = w.F_in, a.F_out = w.F_out, a.KC = w.KC, a.NCB = w.NCB, a.mean = p->mean != 0;
  a.x = p->x, a.ld_x = uint32_t(p->ld_x), a.xroot = p->W_root ? p->xroot : nullptr, a.ld_r = uint32_t(p->ld_xroot);
  a.wf = w.wf, a.bias = p->bias, a.out = p->out, a.ld_o = uint32_t(p->ld_out);
  a.part = reinterpret_cast<float*>(static_cast<char*>(p->workspace) + rgcn_frag_bytes(p->R, p->F_in, p->F_out));
  int rc;
  if (a.NCB <= kWaves)
    rc = launch_tiles<1>(a, stream);
  else if (a.NCB <= 2 * kWaves)
    rc = launch_tiles<2>(a, stream);
  else
    rc = launch_tiles<4>(a, stream);
  if (rc != KGX_OK) return rc;
  if (a.n_split > 0) return launch_fixup(a.pieces, a.n_split, a.F_out, a.part, a.out, a.ld_o, stream);
  return KGX_OK;
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
