// Stand-alone sweep of the run-time-geometry conv planner
// (torchbeast_amd/ops/hip/conv_any_plan.h): every (h, w) in 1..256 squared,
// each channel pair of the deep net, n in {1, 64, 2592}.
//
// CPU only, no torch and no HIP; built plain and with
// -fsanitize=address,undefined. See README_conv_any_plan.md.

#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "conv_any_plan.h"

using namespace tbamd;

static int failures = 0;
#define EXPECT(cond)                                                      \
  do {                                                                    \
    if (!(cond)) {                                                        \
      if (++failures <= 20) {                                             \
        std::fprintf(stderr, "EXPECT failed: %s (%s:%d) ci=%d h=%d w=%d " \
                     "co=%d n=%lld\n", #cond, __FILE__, __LINE__, g_ci,   \
                     g_h, g_w, g_co, (long long)g_n);                     \
      }                                                                   \
    }                                                                     \
  } while (0)

static int g_ci, g_h, g_w, g_co;
static int64_t g_n;

static uint32_t rng_state = 2463534242u;
static uint32_t rng() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state;
}

static void check_div(uint32_t m, uint32_t d, uint32_t magic) {
  EXPECT(conv_any_div(m, d, magic) == m / d);
}

static void check_plan(int ci, int h, int w, int co, int64_t n) {
  g_ci = ci, g_h = h, g_w = w, g_co = co, g_n = n;
  const ConvAnyPlan p = conv_any_plan(ci, h, w, co, n);
  EXPECT(p.ok);
  if (!p.ok) return;
  // The bands cover H exactly once; the last may be short, never empty.
  EXPECT(p.rows >= 1 && p.bands >= 1);
  EXPECT((int64_t)p.bands * p.rows >= h);
  EXPECT((int64_t)(p.bands - 1) * p.rows < h);
  // The band's fragments fit the chosen capacity instantiation.
  const int frags = (p.rows * w + 15) / 16;
  EXPECT(p.cap == 2 || p.cap == kConvAnyMaxCap);
  EXPECT(frags <= kConvAnyWaves * p.cap);
  // The staged tile fits the allocation, and that the budget; the swizzle
  // permutes 16 B slots within 128 B lines, so whole lines are allocated.
  EXPECT(p.lds_bytes >= (p.rows + 2) * (w + 2) * ci * 2);
  EXPECT(p.lds_bytes <= kConvAnyLdsBudget && p.lds_bytes % 128 == 0);
  // The domains the kernel's two multiply-shift divisions are checked on.
  EXPECT(p.rows * w <= 1024);
  EXPECT((p.rows + 2) * conv_any_cpr(ci, w) <= 4096);
  EXPECT(p.magic_w == ((1u << 20) + w - 1) / w);
  // The chunks cover N*H*W exactly once, in whole staging rounds.
  const int64_t M = n * h * w;
  EXPECT(p.mc >= kConvAnyWgradStep && p.mc % kConvAnyWgradStep == 0);
  EXPECT(p.nchunks >= 1 && p.nchunks * p.mc >= M);
  EXPECT((p.nchunks - 1) * p.mc < M);
  // Grid dimensions: x = n or chunks (32 bits), y = bands or 3 (16 bits).
  EXPECT(n <= 0x7fffffffll && p.nchunks <= 0x7fffffffll && p.bands <= 65535);
  EXPECT(M < (1ll << 31));
  // The wgrad kernel's position -> (sample, row, column) divisions.
  const uint32_t hw = (uint32_t)(h * w), um = (uint32_t)M;
  const uint32_t probes[] = {0u, hw - 1, hw, um - 1, um / 2, um - hw};
  for (uint32_t m : probes) {
    check_div(m, hw, p.magic_hw);
    check_div(m % hw, (uint32_t)w, p.magic_w32);
  }
  for (int i = 0; i < 4; ++i) {
    const uint32_t m = rng() % um;
    check_div(m, hw, p.magic_hw);
    check_div(m % hw, (uint32_t)w, p.magic_w32);
  }
}

static void check_refused(int64_t ci, int64_t h, int64_t w, int64_t co,
                          int64_t n) {
  g_ci = (int)ci, g_h = (int)h, g_w = (int)w, g_co = (int)co, g_n = n;
  EXPECT(!conv_any_plan(ci, h, w, co, n).ok);
}

int main() {
  const int pairs[5][2] = {{8, 16}, {16, 16}, {16, 32}, {32, 16}, {32, 32}};
  const int64_t ns[3] = {1, 64, 2592};
  int64_t plans = 0;

  // The forward kernel's m / W and chunk / cpr, on their whole domains.
  g_h = 0, g_co = 0, g_n = 0;
  for (int w = 1; w <= kConvAnyMaxDim; ++w) {
    g_w = w;
    const uint32_t magic = ((1u << 20) + w - 1) / w;
    for (uint32_t m = 0; m < 1024; ++m) EXPECT(((m * magic) >> 20) == m / w);
    for (int ci : {8, 16, 32}) {
      g_ci = ci;
      const uint32_t cpr = (uint32_t)conv_any_cpr(ci, w);
      const uint32_t mc = 0xFFFFFFFFu / cpr + 1;
      for (uint32_t i = 0; i <= 4096; ++i) {
        EXPECT((uint32_t)(((uint64_t)i * mc) >> 32) == i / cpr);
      }
    }
  }
  // conv_any_div at the ends of the uint32 range, every divisor the
  // kernels can pass.
  for (uint32_t d = 1; d <= 65536; ++d) {
    const uint32_t magic = conv_any_magic32(d);
    for (uint32_t m : {0u, 1u, d - 1, d, d + 1, 0x7fffffffu, 0xffffffffu}) {
      check_div(m, d, magic);
    }
  }

  for (const auto& pr : pairs) {
    for (int h = 1; h <= kConvAnyMaxDim; ++h) {
      for (int w = 1; w <= kConvAnyMaxDim; ++w) {
        for (int64_t n : ns) {
          check_plan(pr[0], h, w, pr[1], n);
          ++plans;
        }
      }
    }
  }
  // conv_any_plan(ci, h, w, co, 1).ok is the "supported" verdict.
  check_refused(16, 0, 8, 16, 1);
  check_refused(16, 8, 0, 16, 1);
  check_refused(16, 257, 8, 16, 1);
  check_refused(16, 8, 257, 16, 1);
  check_refused(16, -1, 8, 16, 1);
  check_refused(4, 8, 8, 16, 1);
  check_refused(16, 8, 8, 24, 1);
  check_refused(8, 8, 8, 32, 1);
  check_refused(16, 8, 8, 8, 1);
  check_refused(16, 8, 8, 16, 0);
  check_refused(16, 256, 256, 16, 32768);  // N*H*W = 2^31

  // The 84-family bands of the template kernels at learner batch sizes.
  g_n = 2592;
  EXPECT(conv_any_plan(8, 84, 84, 16, 2592).rows == 7);
  EXPECT(conv_any_plan(32, 11, 11, 32, 2592).rows == 11);
  // A serve batch of 64 still gives 2 workgroups per CU where a band of 128
  // positions allows it.
  g_n = 64;
  EXPECT(64 * conv_any_plan(8, 64, 64, 16, 64).bands >= kConvAnyMinBlocks);
  EXPECT(64 * conv_any_plan(8, 72, 96, 16, 64).bands >= kConvAnyMinBlocks);
  EXPECT(64 * conv_any_plan(16, 36, 48, 16, 64).bands >= kConvAnyMinBlocks);

  if (failures != 0) {
    std::fprintf(stderr, "%d FAILURES\n", failures);
    return 1;
  }
  std::printf("conv_any_plan ok: %lld plans\nALL OK\n", (long long)plans);
  return 0;
}
