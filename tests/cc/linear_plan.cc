// Stand-alone sweep of the MFMA linear layer's planner
// (torchbeast_amd/ops/hip/linear_plan.h): every M in 1..5000 and a spread of
// larger ones, N in 64..1024 by 64, K in 32..4096 by 32.
//
// CPU only, no torch and no HIP; built plain and with
// -fsanitize=address,undefined. See README_linear_plan.md.

#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "linear_plan.h"

using namespace tbamd;

static int failures = 0;
static int64_t g_m, g_n, g_k;
#define EXPECT(cond)                                                       \
  do {                                                                     \
    if (!(cond) && ++failures <= 20) {                                     \
      std::fprintf(stderr, "EXPECT failed: %s (%s:%d) m=%lld n=%lld "      \
                   "k=%lld\n", #cond, __FILE__, __LINE__, (long long)g_m,  \
                   (long long)g_n, (long long)g_k);                        \
    }                                                                      \
  } while (0)

// Parts [split(i), split(i + 1)) cover [0, total) once, none empty, and
// differ in length by at most one.
static void check_split(int total, int parts) {
  EXPECT(parts >= 1 && parts <= total);
  EXPECT(linear_split(total, parts, 0) == 0);
  EXPECT(linear_split(total, parts, parts) == total);
  for (int i = 0; i < parts; ++i) {
    const int len =
        linear_split(total, parts, i + 1) - linear_split(total, parts, i);
    EXPECT(len >= total / parts && len <= total / parts + 1 && len >= 1);
  }
}

static long check_plan(int64_t m, int64_t n, int64_t k) {
  g_m = m, g_n = n, g_k = k;
  const LinearPlan p = linear_plan(m, n, k);
  EXPECT(p.ok);
  if (!p.ok) return 0;
  EXPECT((int64_t)p.tiles_m * kLinTile >= m);
  EXPECT((int64_t)(p.tiles_m - 1) * kLinTile < m);
  EXPECT((int64_t)p.tiles_n * kLinTile == n);
  EXPECT((int64_t)p.tiles_k * kLinTile >= k);
  EXPECT((int64_t)(p.tiles_k - 1) * kLinTile < k);
  EXPECT((int64_t)p.ksteps * kLinKStep == k);
  EXPECT((int64_t)p.rounds * kLinWgradRound >= m);
  EXPECT((int64_t)(p.rounds - 1) * kLinWgradRound < m);
  // Grid limits: x 31 bits, y and z 16 bits.
  EXPECT(p.tiles_n <= 65535 && p.tiles_k <= 65535);
  EXPECT(p.slices >= 1 && p.slices <= kLinMaxSlices);
  EXPECT(p.chunks >= 1 && p.chunks <= kLinMaxChunks);
  check_split(p.ksteps, p.slices);
  check_split(p.rounds, p.chunks);
  if (p.slices > 1) {
    EXPECT(p.ksteps / p.slices >= kLinMinSliceSteps);
    // No more slices than the target needs.
    EXPECT((int64_t)p.tiles_m * p.tiles_n * (p.slices - 1) < kLinTargetBlocks);
  }
  if (p.chunks > 1) {
    EXPECT((int64_t)p.tiles_n * p.tiles_k * (p.chunks - 1) < kLinTargetBlocks);
  }
  return 1;
}

int main() {
  long plans = 0;
  for (int64_t n = 64; n <= 1024; n += 64) {
    for (int64_t k = 32; k <= 4096; k += 32) {
      for (int64_t m = 1; m <= 5000; m += (m < 520 ? 1 : 61)) {
        plans += check_plan(m, n, k);
      }
      for (int64_t m :
           {(int64_t)65537, (int64_t)1 << 20, kLinMaxM - 1, kLinMaxM}) {
        plans += check_plan(m, n, k);
      }
    }
  }
  // The serve sizes of the 3136 -> 512 fc fill the device; the learner's
  // batch finishes in the GEMM kernel.
  for (int64_t m : {(int64_t)64, (int64_t)128, (int64_t)256}) {
    const LinearPlan p = linear_plan(m, 512, 3136);
    g_m = m, g_n = 512, g_k = 3136;
    EXPECT(p.ok && (int64_t)p.tiles_m * p.tiles_n * p.slices >= 256);
  }
  {
    const LinearPlan p = linear_plan(2592, 512, 3136);
    g_m = 2592, g_n = 512, g_k = 3136;
    EXPECT(p.ok && p.tiles_m == 41 && p.tiles_n == 8 && p.slices == 1);
    EXPECT(p.tiles_k == 49 && p.chunks == 1);
    const LinearPlan q = linear_plan(2560, 256, 3872);
    // 40 x 4 tiles: the deep net's fc is cut in two, forward and wgrad.
    EXPECT(q.ok && q.slices == 2 && q.tiles_k == 61 && q.chunks == 2);
  }
  // Refused shapes.
  g_m = g_n = g_k = -1;
  EXPECT(!linear_plan(0, 64, 32).ok && !linear_plan(-1, 64, 32).ok);
  EXPECT(!linear_plan(kLinMaxM + 1, 64, 32).ok);
  EXPECT(!linear_plan(5, 0, 32).ok && !linear_plan(5, 32, 32).ok);
  EXPECT(!linear_plan(5, 96, 32).ok && !linear_plan(5, 64, 0).ok);
  EXPECT(!linear_plan(5, 64, 48).ok && !linear_plan(5, 64, -32).ok);
  EXPECT(!linear_plan(5, 65536ll * 64, 32).ok);
  EXPECT(!linear_plan(5, 64, 65536ll * 64).ok);
  EXPECT(linear_plan(5, 65535ll * 64, 65535ll * 64).ok);

  if (failures) {
    std::fprintf(stderr, "linear_plan: %d failures\n", failures);
    return 1;
  }
  std::printf("linear_plan ok: %ld plans / ALL OK\n", plans);
  return 0;
}
