// NNConv / ECConv: edge-conditioned aggregate and transform in one pass (gfx950, wave64).
//
//   S_i[d] = sum_{slots t of row i} coef[e_t, d] x[col t]   (d < D),      S_i[D] = sum_t x[col t]
//   out[i] = bias + xroot[i] W_root + norm_i (sum_{d < D} S_i[d] W[d] + S_i[D] W_bias)
//
// which is the edge-conditioned convolution out_i = b + x_i W_root + aggr_j x_j Theta(e_ij) whenever the
// edge network ends in a linear layer, Theta(e) = W_bias + sum_d c_e[d] W[d]: the neighbour sum commutes
// with the weights, so the flops are per node and nothing of size E x F_in x F_out exists.  No reference
// counterpart (PyG's NNConv).  This is rgcn.hip's problem with soft memberships, and the weight
// fragments, the six-product MFMA, the epilogue and the fix-up are shared with it (kgx_wfrag.h).  The
// gather is not: every edge feeds every plane, so there is no per-relation slot range to walk and no
// relation to skip; a lane group keeps one piece's planes in registers instead.
//
//   * wfrag::prep_kernel splits W [D], W_bias and W_root once per call into bf16x3 MFMA fragments.
//   * nnconv_tile_kernel<LG, DC, NCBW>: a block owns kM = 64 pieces (node, slot range).  Wave w owns
//     pieces 16 w .. 16 w + 15; a lane group of G = 2^LG = 8 / 16 / 32 lanes (one float4 column each) owns
//     ROUNDS = G / 4 of them, one after the other.  The planes are walked in chunks of at most DC: per
//     chunk and piece the group walks the piece's slots in CSR order, KU slots in flight, loading the
//     source row once and the edge's coefficients of the chunk once (one address for the whole group),
//     and updates acc[d] = fma(coef[d], x, acc[d]) in registers: ROUNDS x DC float4 per lane.  Absent
//     slots read the zero row with full exec.  The source rows are gathered once per chunk; the repeats
//     hit L2.  The chunk's planes then go through LDS one after another: scale by norm_i, split three
//     ways, write the bf16 tile [3][64][32 KC + 8], barrier, and every wave multiplies the whole tile
//     with ITS column blocks of that plane's weight on v_mfma_f32_16x16x32_bf16 (six significant
//     products), into f32 accumulators that stay in registers across all planes and the root plane.
//     With F_in <= 64 there are two LDS tiles, so a wave splits plane p + 1 while others still
//     multiply plane p, and one barrier per plane is enough.
//   * A whole-node piece adds bias and stores its row; a piece of a cut node stores a partial row and
//     wfrag::fixup_kernel adds them in piece order.  No atomics: one writer per element.
// No packed f32 VALU in this file, as in rgcn.hip and edge_mp.hip: the feature is taken off every function
// of the device pass; the Makefile adds -fno-slp-vectorize.  The push comes BEFORE the HIP header, so its
// helpers (make_float4, make_uint2, ..) carry the same target features as the kernels and are inlined; pushed
// after it they stay out-of-line calls in the gather and staging loops.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#include <hip/hip_runtime.h>

#include "kgx_bf16x3.h"
#include "kgx_internal.h"
#include "kgx_mfma.h"
#include "kgx_wfrag.h"

namespace kgx {
namespace {

using namespace wfrag;

constexpr int kM = 64;        // pieces per tile
constexpr int kRB = kM / 16;  // 16-piece MFMA row blocks
constexpr int kWaves = kBlock / 64;
constexpr int kPadK = 8;  // bf16 of padding per tile row: 16 rows of a fragment read fall on 64 banks
constexpr int kMaxFin = 128, kMaxFout = 256, kMaxD = 32;

// The wave-wide vote and the read of another lane's register, on the builtins.  ds_bpermute reads only lanes
// that are active: every call below sits under wave-uniform control flow.
__device__ __forceinline__ uint64_t wave_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ int32_t wave_shfl(int32_t v, int src) { return __builtin_amdgcn_ds_bpermute(src << 2, v); }

struct TileArgs {
  const int32_t* rowptr;  // [n_rows + 1]
  const int32_t* col;
  const int32_t* e_idx;   // or null: the slot is the edge row
  const int32_t* pieces;  // [n_pieces][3]: node, slot_begin, slot_end; the first n_split belong to cut nodes
  int64_t n_pieces, n_split;
  uint32_t n_src, n_e;
  int D, P, has_wb, n_chunks;  // P = D (+ 1 with W_bias) planes, walked in n_chunks chunks
  int F_in, F_out, KC, NCB, mean, nbuf;
  const float* x;
  uint32_t ld_x;  // < 2^31 (checked at the entry point)
  const float* coef;
  uint32_t ld_c;
  const float* xroot;
  uint32_t ld_r;
  const short* wf;  // W fragments: [(D + 2) KC NCB][3][kFrag]; plane D is W_bias, D + 1 is W_root
  const float* bias;
  float* out;
  uint32_t ld_o;
  float* part;  // [n_split][F_out]
};

// One piece's slots [s, h) in CSR order, for this lane's four columns and the planes d0 .. d0 + DC - 1:
// S[j] += coef[e_t, d0 + j] * x[col t], the plane d == D (W_bias) with the coefficient 1.  The loop count
// is wave-uniform (the longest of the wave's groups); a group past its end, a lane past F_in, a source
// outside [0, n_src) and an edge row outside [0, n_e) read the zero row, so every lane issues every load.
template <int DC, int KU>
__device__ __forceinline__ void gather_planes(const TileArgs& a, int32_t s, int32_t h, int d0, int c4, bool col_ok,
                                              float4 (&S)[DC]) {
#pragma unroll
  for (int j = 0; j < DC; ++j) S[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const int dlim = a.D - d0 < DC ? a.D - d0 : DC;  // coefficient planes of the chunk (<= 0: W_bias alone)
  const int one_j = a.has_wb ? a.D - d0 : -1;      // the W_bias plane's place in the chunk, if it is in it
  while (wave_ballot(s < h) != 0) {
    int32_t ci[KU], ei[KU];
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const int32_t t = s + u < h ? s + u : 0;  // slot 0 exists: some piece has a slot
      ci[u] = a.col[t];
      ei[u] = a.e_idx ? a.e_idx[t] : t;
    }
    float4 v[KU];
    float cf[KU][DC];
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const bool ok = s + u < h;
      const float* xp = (ok && col_ok && uint32_t(ci[u]) < a.n_src) ? a.x + row_off(ci[u], a.ld_x) + c4 : kgx_zero_row + c4;
      v[u] = ld4(xp);
      const float* cp = (ok && dlim > 0 && uint32_t(ei[u]) < a.n_e) ? a.coef + row_off(ei[u], a.ld_c) + d0 : kgx_zero_row;
#pragma unroll
      for (int j = 0; j < DC; ++j) {
        const float raw = cp[j < dlim ? j : 0];
        cf[u][j] = j < dlim ? raw : ((j == one_j && ok) ? 1.0f : 0.0f);
      }
    }
#pragma unroll
    for (int u = 0; u < KU; ++u)
#pragma unroll
      for (int j = 0; j < DC; ++j) {
        S[j].x = __fmaf_rn(cf[u][j], v[u].x, S[j].x);
        S[j].y = __fmaf_rn(cf[u][j], v[u].y, S[j].y);
        S[j].z = __fmaf_rn(cf[u][j], v[u].z, S[j].z);
        S[j].w = __fmaf_rn(cf[u][j], v[u].w, S[j].w);
      }
    s += KU;
  }
}

// four sums of tile row `row` -> the three bf16 planes of the LDS tile
__device__ __forceinline__ void stage_row(short* tb, int row, int ldk, int plane, int c4, float4 sum) {
  uint32_t ph[2], pm[2], pl[2];
  split4(sum, ph, pm, pl);
  short* r = tb + row * ldk + c4;
  *reinterpret_cast<uint2*>(r) = make_uint2(ph[0], ph[1]);
  *reinterpret_cast<uint2*>(r + plane) = make_uint2(pm[0], pm[1]);
  *reinterpret_cast<uint2*>(r + 2 * plane) = make_uint2(pl[0], pl[1]);
}

// The whole LDS tile times this wave's column blocks of one weight plane: W^T (A operand, fragments from the
// workspace) times tile^T (B operand); a 16-piece row block outside `mask` holds no row and is skipped.
template <int NCBW>
__device__ __forceinline__ void mfma_plane(f32x4_t (&acc)[NCBW][kRB], const short* tb, const short* wr, int KC, int NCB,
                                           int ldk, int plane, uint64_t mask, int wave, int n, int q) {
#pragma unroll 1
  for (int kc = 0; kc < KC; ++kc) {
#pragma unroll
    for (int j = 0; j < NCBW; ++j) {
      const int cb = wave + kWaves * j;
      if (cb >= NCB) continue;  // wave-uniform
      const short* f = wr + (int64_t(kc) * NCB + cb) * 3 * kFrag;
      const Planes w{ld8(f), ld8(f + kFrag), ld8(f + 2 * kFrag)};
#pragma unroll
      for (int b = 0; b < kRB; ++b) {
        if (((mask >> (16 * b)) & 0xffffu) == 0) continue;
        const short* ar = tb + (16 * b + n) * ldk + kc * 32 + 8 * q;
        const Planes s{ld8(ar), ld8(ar + plane), ld8(ar + 2 * plane)};
        acc[j][b] = mfma6(w, s, acc[j][b]);
      }
    }
  }
}

// LG: log2 of the lane group (4 G >= F_in columns).  DC: planes per chunk, ROUNDS x DC float4 of sums per
// lane.  NCBW: 16-column blocks per wave (wave w owns blocks w, w + 4, ..): 1 for F_out <= 64, 2 to 128,
// 4 to 256.  Two blocks per CU asked of the register allocator (256 registers a lane).
template <int LG, int DC, int NCBW>
__global__ __launch_bounds__(kBlock, 2) void nnconv_tile_kernel(TileArgs a) {
  extern __shared__ __attribute__((aligned(16))) short tile[];  // [nbuf][3 planes][kM][ldk]
  constexpr int G = 1 << LG, NG = 64 >> LG, ROUNDS = 16 / NG, KU = DC <= 4 ? 4 : 2;
  // the ids from the builtins: the device library's accessors do not carry this file's target attribute
  const int tid = int(__builtin_amdgcn_workitem_id_x()), wave = tid >> 6, lane = tid & 63;
  const int n = lane & 15, q = lane >> 4;
  const int ldk = a.KC * 32 + kPadK, plane = kM * ldk, bufsz = 3 * plane;
  const int grp = lane >> LG, c4 = 4 * (lane & (G - 1));
  const bool col_ok = c4 < a.F_in, k_ok = c4 < a.KC * 32;

  // lane l holds piece l of the tile
  const int64_t p0 = int64_t(__builtin_amdgcn_workgroup_id_x()) * kM;
  int32_t node = -1, sb = 0, se = 0;
  if (p0 + lane < a.n_pieces) {
    const int32_t* pc = a.pieces + (p0 + lane) * 3;
    node = pc[0], sb = pc[1], se = pc[2];
  }
  const int32_t rb = a.rowptr[node < 0 ? 0 : node], re = a.rowptr[node < 0 ? 0 : node + 1];
  const bool first = node >= 0 && sb == rb;  // the node's first (or only) piece
  const int32_t deg = re - rb;               // the node's, not the piece's
  if (node < 0) sb = se = 0;

  f32x4_t acc[NCBW][kRB];
#pragma unroll
  for (int j = 0; j < NCBW; ++j)
#pragma unroll
    for (int b = 0; b < kRB; ++b) acc[j][b] = f32x4_t{0.0f, 0.0f, 0.0f, 0.0f};

  const int64_t wplane = int64_t(a.KC) * a.NCB * 3 * kFrag;
  const short* wf = a.wf + lane * 8;
  int np = 0;  // planes staged so far: the LDS tile of plane np is np % nbuf

  const uint64_t tmask = wave_ballot(sb < se);  // the same in all four waves
  if (tmask != 0) {
    const uint32_t m16 = uint32_t(tmask >> (16 * wave)) & 0xffffu;  // this wave's row block has a slot
    for (int ch = 0; ch < a.n_chunks; ++ch) {
      const int d0 = ch * a.P / a.n_chunks, dc = (ch + 1) * a.P / a.n_chunks - d0;  // dc <= DC
      float4 S[ROUNDS][DC];
      if (m16) {
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
          const int src = 16 * wave + r * NG + grp;
          gather_planes<DC, KU>(a, wave_shfl(sb, src), wave_shfl(se, src), d0, c4, col_ok, S[r]);
        }
        if (a.mean) {
#pragma unroll
          for (int r = 0; r < ROUNDS; ++r) {
            const int32_t c = wave_shfl(deg, 16 * wave + r * NG + grp);
            if (c > 1) {
              const float d = float(c);
#pragma unroll
              for (int j = 0; j < DC; ++j)
                S[r][j] = make_float4(__fdiv_rn(S[r][j].x, d), __fdiv_rn(S[r][j].y, d), __fdiv_rn(S[r][j].z, d),
                                      __fdiv_rn(S[r][j].w, d));
            }
          }
        }
      }
#pragma unroll
      for (int j = 0; j < DC; ++j) {
        if (j < dc) {  // block-uniform
          short* tb = tile + (np % a.nbuf) * bufsz;
          if (m16 && k_ok) {
#pragma unroll
            for (int r = 0; r < ROUNDS; ++r) stage_row(tb, 16 * wave + r * NG + grp, ldk, plane, c4, S[r][j]);
          }
          lds_barrier();
          mfma_plane<NCBW>(acc, tb, wf + (d0 + j) * wplane, a.KC, a.NCB, ldk, plane, tmask, wave, n, q);
          if (a.nbuf == 1) lds_barrier();  // the tile is read before the next plane overwrites it
          ++np;
        }
      }
    }
  }

  // the root plane: xroot rows of the pieces that are their node's first, against W_root
  const uint64_t rmask = a.xroot ? wave_ballot(first) : 0;
  if (rmask != 0) {
    short* tb = tile + (np % a.nbuf) * bufsz;
    if (uint32_t(rmask >> (16 * wave)) & 0xffffu) {  // wave-uniform: the shuffles read every lane
#pragma unroll
      for (int r = 0; r < ROUNDS; ++r) {
        const int src = 16 * wave + r * NG + grp;
        const int32_t nd = wave_shfl(node, src);
        const bool f = wave_shfl(int(first), src) != 0;
        const float* p = (f && col_ok) ? a.xroot + row_off(nd, a.ld_r) + c4 : kgx_zero_row + c4;
        const float4 v = ld4(p);
        if (k_ok) stage_row(tb, src, ldk, plane, c4, v);
      }
    }
    lds_barrier();
    mfma_plane<NCBW>(acc, tb, wf + (a.D + 1) * wplane, a.KC, a.NCB, ldk, plane, rmask, wave, n, q);
  }

  // lane (n, q) holds piece 16 b + n, columns 16 cb + 4 q .. + 3
#pragma unroll
  for (int b = 0; b < kRB; ++b) {
    const int src = 16 * b + n;
    const int32_t nd = wave_shfl(node, src);
    const bool fst = wave_shfl(int(first), src) != 0;
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

// planes per chunk: ROUNDS x DC float4 of sums per lane, 128 registers beside 16 or 32 of output
// accumulators, 64 beside the 64 of F_out > 128 and for F_in <= 32 (DC = 16 spilled)
constexpr int chunk_planes(int LG, int NCBW) { return LG == 3 ? 8 : (NCBW == 4 ? 16 : 32) / (1 << (LG - 2)); }

size_t workspace_bytes(int64_t n_split, int64_t D, int64_t F_in, int64_t F_out) {
  return frag_bytes(D + 2, F_in, F_out) + align_up(size_t(n_split) * size_t(F_out) * sizeof(float), 256);
}
bool shape_ok(int64_t F_in, int64_t F_out, int64_t D) {
  return F_in >= 4 && F_in <= kMaxFin && F_in % 4 == 0 && F_out >= 4 && F_out <= kMaxFout && F_out % 4 == 0 && D >= 1 &&
         D <= kMaxD;
}

template <int LG, int NCBW>
int launch_tiles(TileArgs& a, hipStream_t s) {
  constexpr int DC = chunk_planes(LG, NCBW);
  a.n_chunks = (a.P + DC - 1) / DC;
  a.nbuf = a.KC <= 2 ? 2 : 1;  // two tiles of F_in <= 64 are 55 KB; one of F_in = 128 is 52 KB
  const int64_t tiles = (a.n_pieces + kM - 1) / kM;
  const size_t lds = size_t(a.nbuf) * 3 * kM * (a.KC * 32 + kPadK) * sizeof(short);
  hipLaunchKernelGGL((nnconv_tile_kernel<LG, DC, NCBW>), dim3(unsigned(tiles)), dim3(kBlock), lds, s, a);
  KGX_CHECK_LAUNCH();
  return KGX_OK;
}

template <int LG>
int launch_width(TileArgs& a, hipStream_t s) {
  if (a.NCB <= kWaves) return launch_tiles<LG, 1>(a, s);
  if (a.NCB <= 2 * kWaves) return launch_tiles<LG, 2>(a, s);
  return launch_tiles<LG, 4>(a, s);
}

}  // namespace
}  // namespace kgx

using namespace kgx;

extern "C" int kgx_nnconv_workspace_bytes(int64_t n_pieces, int64_t n_split_pieces, int64_t D, int64_t F_in,
                                          int64_t F_out, size_t* bytes) {
  KGX_REQUIRE(bytes && n_pieces >= 0 && n_split_pieces >= 0 && n_split_pieces <= n_pieces && n_pieces < kInt32Limit,
              KGX_ERR_ARG, "kgx_nnconv_workspace_bytes: n_pieces %lld, n_split_pieces %lld", (long long)n_pieces,
              (long long)n_split_pieces);
  KGX_REQUIRE(shape_ok(F_in, F_out, D), KGX_ERR_UNSUPPORTED,
              "kgx_nnconv_workspace_bytes: F_in = %lld, F_out = %lld, D = %lld (multiples of 4, F_in in [4, 128], F_out "
              "in [4, 256]; D in [1, 32])", (long long)F_in, (long long)F_out, (long long)D);
  *bytes = workspace_bytes(n_split_pieces, D, F_in, F_out);
  return KGX_OK;
}

extern "C" int kgx_nnconv_run(const kgx_nnconv_args* p, kgx_stream_t stream_) {
  KGX_REQUIRE(p && p->struct_size == sizeof(kgx_nnconv_args), KGX_ERR_ARG,
              "kgx_nnconv_run: struct_size %llu is not this header's %zu", p ? (unsigned long long)p->struct_size : 0ull,
              sizeof(kgx_nnconv_args));
  const char* fn = "kgx_nnconv_run";
  KGX_REQUIRE(p->n_rows >= 0 && p->n_rows < kInt32Limit && p->n_src >= 0 && p->n_src < kInt32Limit && p->n_e >= 0 &&
                  p->n_e < kInt32Limit,
              KGX_ERR_ARG, "%s: n_rows = %lld, n_src = %lld, n_e = %lld (each in [0, 2^31))", fn, (long long)p->n_rows,
              (long long)p->n_src, (long long)p->n_e);
  KGX_REQUIRE(p->n_pieces >= p->n_rows && p->n_pieces < kInt32Limit && p->n_split_pieces >= 0 &&
                  p->n_split_pieces <= p->n_pieces,
              KGX_ERR_ARG, "%s: n_pieces = %lld, n_split_pieces = %lld for %lld rows (every row has a piece)", fn,
              (long long)p->n_pieces, (long long)p->n_split_pieces, (long long)p->n_rows);
  KGX_REQUIRE(p->F_in >= 1 && p->F_out >= 1 && p->D >= 1 && p->ld_x >= p->F_in && p->ld_out >= p->F_out &&
                  p->ld_coef >= p->D && (!p->W_root || p->ld_xroot >= p->F_in),
              KGX_ERR_ARG, "%s: leading dimension below the width (ld_x %lld, ld_coef %lld, ld_xroot %lld, ld_out %lld)", fn,
              (long long)p->ld_x, (long long)p->ld_coef, (long long)p->ld_xroot, (long long)p->ld_out);
  KGX_REQUIRE(p->ld_x < kInt32Limit && p->ld_coef < kInt32Limit && p->ld_xroot < kInt32Limit && p->ld_out < kInt32Limit,
              KGX_ERR_ARG, "%s: a leading dimension >= 2^31", fn);
  KGX_REQUIRE(shape_ok(p->F_in, p->F_out, p->D), KGX_ERR_UNSUPPORTED,
              "%s: F_in = %lld, F_out = %lld, D = %lld (multiples of 4, F_in in [4, 128], F_out in [4, 256]; D in [1, 32])",
              fn, (long long)p->F_in, (long long)p->F_out, (long long)p->D);
  if (p->n_rows == 0) return KGX_OK;
  KGX_REQUIRE(p->rowptr && p->pieces && p->x && p->coef && p->W && p->out && (!p->W_root || p->xroot), KGX_ERR_ARG,
              "%s: null pointer (rowptr, pieces, x, coef, W, out; W_root needs xroot)", fn);
  KGX_REQUIRE(aligned16(p->x) && aligned16(p->out) && aligned16(p->xroot) && aligned16(p->bias) && p->ld_x % 4 == 0 &&
                  p->ld_out % 4 == 0 && p->ld_xroot % 4 == 0,
              KGX_ERR_UNSUPPORTED,
              "%s: x, xroot, out and bias are accessed four floats at a time: 16-byte aligned addresses and leading "
              "dimensions that are multiples of 4", fn);
  const size_t need = workspace_bytes(p->n_split_pieces, p->D, p->F_in, p->F_out);
  KGX_REQUIRE(p->workspace && aligned16(p->workspace) && p->workspace_bytes >= need, KGX_ERR_ARG,
              "%s: workspace of %llu bytes, needs %zu (16-byte aligned)", fn, (unsigned long long)p->workspace_bytes, need);
  hipStream_t stream = as_stream(stream_);

  PrepArgs w{};
  w.W = p->W, w.extra[0] = p->W_bias, w.extra[1] = p->W_root, w.n_extra = 2, w.R = int(p->D);
  w.F_in = int(p->F_in), w.F_out = int(p->F_out), w.KC = k_chunks(p->F_in), w.NCB = col_blocks(p->F_out);
  w.wf = static_cast<short*>(p->workspace);
  if (const int rc = launch_prep(w, stream); rc != KGX_OK) return rc;

  TileArgs a{};
  a.rowptr = p->rowptr, a.col = p->col, a.e_idx = p->e_idx, a.pieces = p->pieces;
  a.n_pieces = p->n_pieces, a.n_split = p->n_split_pieces, a.n_src = uint32_t(p->n_src), a.n_e = uint32_t(p->n_e);
  a.D = w.R, a.has_wb = p->W_bias != nullptr, a.P = a.D + a.has_wb;
  a.F_in = w.F_in, a.F_out = w.F_out, a.KC = w.KC, a.NCB = w.NCB, a.mean = p->mean != 0;
  a.x = p->x, a.ld_x = uint32_t(p->ld_x), a.coef = p->coef, a.ld_c = uint32_t(p->ld_coef);
  a.xroot = p->W_root ? p->xroot : nullptr, a.ld_r = uint32_t(p->ld_xroot);
  a.wf = w.wf, a.bias = p->bias, a.out = p->out, a.ld_o = uint32_t(p->ld_out);
  a.part = reinterpret_cast<float*>(static_cast<char*>(p->workspace) + frag_bytes(p->D + 2, p->F_in, p->F_out));
  const int rc = a.F_in > 64 ? launch_width<5>(a, stream) : (a.F_in > 32 ? launch_width<4>(a, stream) : launch_width<3>(a, stream));
  if (rc != KGX_OK) return rc;
  if (a.n_split > 0) return launch_fixup(a.pieces, a.n_split, a.F_out, a.part, a.out, a.ld_o, stream);
  return KGX_OK;
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
