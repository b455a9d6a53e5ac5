// Lane layout of the head / sub-lane attention kernels (gatv2.hip,
// dot_attention.hip): the one statement of how many channels a lane holds and
// how a destination row's heads map onto a group of at most 64 lanes.  Host
// only, plain C++17, no HIP: tests/host/attn_layout_main.cpp compiles it alone.
#pragma once

#include <cstdint>
#include <initializer_list>

namespace kgx {

inline int next_pow2(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}
inline int log2i(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

// Lane l of a group of G lanes holds K consecutive channels of head l / LH
// (LH lanes per head, LH and G powers of two; lanes past C or H are padding).
struct AttnLayout {
  int K, LH, lgLH, G, lgG;
};

// Do `bytes`-wide vector accesses fit an op's operands: every pointer (null:
// absent) aligned to `bytes`, every leading dimension a multiple of bytes / 4
// floats.  Each op passes its own pointer and leading-dimension lists.
inline bool attn_vec_ok(int bytes, std::initializer_list<const void*> ptrs, std::initializer_list<int64_t> lds) {
  for (const void* p : ptrs)
    if (reinterpret_cast<uintptr_t>(p) % bytes) return false;
  for (int64_t ld : lds)
    if (ld % (bytes / 4)) return false;
  return true;
}

inline bool attn_fits(int heads, int channels, int K) { return heads * next_pow2((channels + K - 1) / K) <= 64; }

// Channels per lane of the forward kernels and of the dot-product backward:
// float4 pieces when vec4 holds -- 8 first, then 4, 16, the first that divides
// C and fits a row's heads into 64 lanes -- else float2 (vec2, even C) or
// scalar loads.  0: the shape needs more than 64 lanes per row.  Measured at
// C3 (8 heads x 16, medians): GATv2 forward 0.94 ms at K = 8 (two lanes per
// head, four rows per wave, one DPP step per score) against 1.13 at 4 and 0.98
// at 16; dot-product forward / forward + backward 1.43 / 5.09 ms at 8, 1.38 /
// 5.13 at 4, 1.55 / 5.43 at 16 -- 4 wins that forward by 3 % and gives it back
// in the backward (ranges overlap there), so one rule serves all of them.
inline int attn_pick_k(int heads, int channels, bool vec4, bool vec2) {
  if (vec4) {
    for (int k : {8, 4, 16})
      if (channels % k == 0 && attn_fits(heads, channels, k)) return k;
  }
  const int k = (vec2 && channels % 2 == 0) ? 2 : 1;
  return attn_fits(heads, channels, k) ? k : 0;
}

// Channels per lane of the GATv2 backward: the smallest K dividing C, with
// aligned vector accesses, that fits a row's heads into 64 lanes.  0: none.
inline int attn_pick_k_smallest(int heads, int channels, bool vec4, bool vec2) {
  for (int k = 1; k <= 16; k <<= 1) {
    if (channels % k || (k == 2 && !vec2) || (k >= 4 && !vec4)) continue;
    if (attn_fits(heads, channels, k)) return k;
  }
  return 0;
}

// Experiment knob (A/B only): `forced` channels per lane (an entry point's
// KGX_*_K variable, 0: unset) replace a float4 choice K where the shape allows
// them -- the same lane budget as the automatic choice.
inline int attn_knob_k(int K, int heads, int channels, bool vec4, int forced) {
  if (K >= 4 && vec4 && (forced == 4 || forced == 8 || forced == 16) && channels % forced == 0 &&
      attn_fits(heads, channels, forced))
    return forced;
  return K;
}

inline AttnLayout attn_layout(int heads, int channels, int K) {
  AttnLayout y;
  y.K = K;
  y.LH = next_pow2((channels + K - 1) / K);
  y.lgLH = log2i(y.LH);
  y.G = next_pow2(heads * y.LH);
  y.lgG = log2i(y.G);
  return y;
}

// Floats between the forward's chunk partials [H*C acc | H m | H l]: rounded up
// to a multiple of 4, so every slot starts 16-byte aligned (odd H).
inline int64_t attn_partial_ld(int heads, int channels) {
  return (int64_t(heads) * channels + 2 * heads + 3) / 4 * 4;
}

}  // namespace kgx
