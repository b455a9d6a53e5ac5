// Prints the lane layouts csrc/kgx_attn_layout.h chooses, for
// tests/test_attn_layout_host.py.  Arguments: any number of groups
//   heads channels align ld
// (operands aligned to `align` bytes, every leading dimension `ld` floats).
// One line per group:
//   K LH G  K LH G  ld_p
// the forward rule (attn_pick_k), the GATv2 backward's (attn_pick_k_smallest),
// 0 0 0 where the shape needs more than 64 lanes, and the forward's partial stride.
#include <cstdio>
#include <cstdlib>

#include "kgx_attn_layout.h"

static void print_layout(int heads, int channels, int K) {
  if (K == 0) {
    std::printf("0 0 0");
    return;
  }
  const kgx::AttnLayout y = kgx::attn_layout(heads, channels, K);
  std::printf("%d %d %d", y.K, y.LH, y.G);
}

int main(int argc, char** argv) {
  if (argc < 5 || (argc - 1) % 4 != 0) {
    std::fprintf(stderr, "usage: %s (heads channels align ld)...\n", argv[0]);
    return 2;
  }
  for (int i = 1; i + 3 < argc; i += 4) {
    const int heads = std::atoi(argv[i]), channels = std::atoi(argv[i + 1]);
    const void* p = reinterpret_cast<const void*>(static_cast<uintptr_t>(std::atoll(argv[i + 2])));
    const int64_t ld = std::atoll(argv[i + 3]);
    const bool vec4 = kgx::attn_vec_ok(16, {p, nullptr}, {ld});
    const bool vec2 = kgx::attn_vec_ok(8, {p, nullptr}, {ld});
    print_layout(heads, channels, kgx::attn_pick_k(heads, channels, vec4, vec2));
    std::printf("  ");
    print_layout(heads, channels, kgx::attn_pick_k_smallest(heads, channels, vec4, vec2));
    std::printf("  %lld\n", static_cast<long long>(kgx::attn_partial_ld(heads, channels)));
  }
  return 0;
}
