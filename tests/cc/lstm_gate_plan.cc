// Stand-alone sweep of the persistent MFMA LSTM planner
// (torchbeast_amd/ops/hip/lstm_gate_plan.h): every B in 1..128 and H in
// 1..1100, with the planner's picks and with every override.
//
// CPU only, no torch and no HIP; built plain and with
// -fsanitize=address,undefined. See README_lstm_gate_plan.md.

#include <cstdint>
#include <cstdio>
#include <vector>

#include "lstm_gate_plan.h"

using namespace tbamd;

static int failures = 0;
static int g_b, g_h, g_f, g_w;
#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond) && ++failures <= 20) {                                      \
      std::fprintf(stderr, "EXPECT failed: %s (%s:%d) b=%d h=%d hs_f=%d "   \
                   "hs_b=%d\n", #cond, __FILE__, __LINE__, g_b, g_h, g_f,   \
                   g_w);                                                    \
    }                                                                       \
  } while (0)

// Workgroups of `hs` units, dealt as the kernels deal them (r0 = g * hs,
// live while r0 + r < H), own every unit exactly once.
static void check_cover(int grid, int hs, int H) {
  EXPECT(grid >= 1);
  std::vector<int> owners(H, 0);
  for (int g = 0; g < grid; ++g) {
    for (int r = 0; r < hs; ++r) {
      if (g * hs + r < H) ++owners[g * hs + r];
    }
  }
  for (int u = 0; u < H; ++u) EXPECT(owners[u] == 1);
  EXPECT((grid - 1) * hs < H);  // no workgroup without a unit
}

static long check_plan(int b, int h, int hs_f, int hs_b) {
  g_b = b, g_h = h, g_f = hs_f, g_w = hs_b;
  const LstmGatePlan p = lstm_gate_plan(b, h, hs_f, hs_b);
  const bool required = b >= 1 && b <= 64 && h >= 1 && h <= 1024;
  EXPECT(p.ok == required);
  EXPECT(p.ok == lstm_gate_plan(b, h).ok);  // overrides never change `ok`
  if (!p.ok) return 0;
  EXPECT(p.hs_f == 4 || p.hs_f == 8 || p.hs_f == 16);
  EXPECT(p.hs_b == 16 || p.hs_b == 32);
  if (hs_f == 4 || hs_f == 8 || hs_f == 16) EXPECT(p.hs_f == hs_f);
  if (hs_b == 16 || hs_b == 32) EXPECT(p.hs_b == hs_b);
  check_cover(p.grid_f, p.hs_f, h);
  check_cover(p.grid_b, p.hs_b, h);
  // Batch fragments and padded extents.
  EXPECT(p.bp == 16 * p.nf && p.bp >= b && p.bp - b < 16 && p.nf <= 4);
  EXPECT(p.kp % kGateKStep == 0 && p.kp >= h && p.kp - h < kGateKStep);
  EXPECT(p.ks_f * kGateKStep == p.kp);
  EXPECT(p.hq % 4 == 0 && p.hq >= h && p.hq - h < 4);
  EXPECT(p.gp % kGateKStep == 0 && p.gp >= 4 * p.hq &&
         p.gp - 4 * p.hq < kGateKStep);
  EXPECT(p.ks_b * kGateKStep == p.gp);
  // A published group of four never leaves its row or its gate block.
  EXPECT(p.grid_f * p.hs_f <= p.kp + 12);
  EXPECT((p.grid_f * p.hs_f + 3) / 4 * 4 - 4 < p.kp);
  // Every k-step has a wave and a register slot.
  EXPECT(p.ks_f <= kGateWaves * kGateFwdKpw);
  EXPECT(p.ks_b <= kGateWaves * kGateBwdKpw);
  EXPECT(p.lds_f == lstm_gate_lds_f(b, p.bp, p.hs_f));
  EXPECT(p.lds_b == lstm_gate_lds_b(b, p.bp, p.hs_b));
  EXPECT(p.lds_f > 0 && p.lds_f <= kGateLdsLimit);
  EXPECT(p.lds_b > 0 && p.lds_b <= kGateLdsLimit);
  return 1;
}

int main() {
  long plans = 0;
  for (int b = 0; b <= 128; ++b) {
    for (int h = 0; h <= 1100; ++h) {
      for (int hs_f : {0, 4, 8, 16, 5}) {
        for (int hs_b : {0, 16, 32, 48}) plans += check_plan(b, h, hs_f, hs_b);
      }
    }
  }
  // The bench shape: 33 workgroups both ways, 17 and 65 k-steps.
  {
    g_b = 32, g_h = 519, g_f = g_w = 0;
    const LstmGatePlan p = lstm_gate_plan(32, 519);
    EXPECT(p.ok && p.hs_f == 16 && p.hs_b == 16 && p.grid_f == 33);
    EXPECT(p.grid_b == 33 && p.kp == 544 && p.ks_f == 17 && p.hq == 520);
    EXPECT(p.gp == 2080 && p.ks_b == 65 && p.nf == 2 && p.bp == 32);
    EXPECT(lstm_gate_plan(32, 519, 4, 0).grid_f == 130);
  }
  EXPECT(!lstm_gate_plan(-1, 8).ok && !lstm_gate_plan(8, -1).ok);
  EXPECT(!lstm_gate_plan(1ll << 40, 8).ok && !lstm_gate_plan(8, 1ll << 40).ok);
  if (failures) {
    std::fprintf(stderr, "lstm_gate_plan: %d failures\n", failures);
    return 1;
  }
  std::printf("lstm_gate_plan ok: %ld plans / ALL OK\n", plans);
  return 0;
}
