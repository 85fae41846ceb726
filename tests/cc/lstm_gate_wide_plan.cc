// Stand-alone sweep of the wide-batch persistent MFMA LSTM planner
// (torchbeast_amd/ops/hip/lstm_gate_wide_plan.h): every B in 0..300 and H in
// 0..1100.
//
// CPU only, no torch and no HIP; built plain and with
// -fsanitize=address,undefined. See README_lstm_gate_wide_plan.md.

#include <cstdint>
#include <cstdio>
#include <vector>

#include "lstm_gate_wide_plan.h"

using namespace tbamd;

static int failures = 0;
static int g_b, g_h;
#define EXPECT(cond)                                                       \
  do {                                                                     \
    if (!(cond) && ++failures <= 20) {                                     \
      std::fprintf(stderr, "EXPECT failed: %s (%s:%d) b=%d h=%d\n", #cond, \
                   __FILE__, __LINE__, g_b, g_h);                          \
    }                                                                      \
  } while (0)

// Workgroups of `hs` units, dealt as the kernels deal them (r0 = g * hs,
// live while r0 + r < H), own every unit exactly once.
static void check_units(int grid, int hs, int H) {
  std::vector<int> owners(H, 0);
  for (int g = 0; g < grid; ++g) {
    for (int r = 0; r < hs; ++r) {
      if (g * hs + r < H) ++owners[g * hs + r];
    }
  }
  for (int u = 0; u < H; ++u) EXPECT(owners[u] == 1);
  EXPECT(grid >= 1 && (grid - 1) * hs < H);  // no workgroup without a unit
}

// Wave w, slot j holds fragment w + 8 j when that is below nf, as the kernels
// deal them: every fragment has exactly one owner, where the planner says.
static void check_fragments(const LstmGateWidePlan& p) {
  std::vector<int> owners(p.nf, 0);
  for (int w = 0; w < kWideWaves; ++w) {
    for (int j = 0; j < p.nfw; ++j) {
      const int f = w + j * kWideWaves;
      if (f >= p.nf) continue;
      ++owners[f];
      EXPECT(lstm_gate_wide_wave(f) == w && lstm_gate_wide_slot(f) == j);
    }
  }
  for (int f = 0; f < p.nf; ++f) EXPECT(owners[f] == 1);
}

static long check_plan(int b, int h) {
  g_b = b, g_h = h;
  const LstmGateWidePlan p = lstm_gate_wide_plan(b, h);
  EXPECT(p.ok == (b >= 1 && b <= 256 && h >= 1 && h <= 1024));
  if (!p.ok) return 0;
  EXPECT(p.hs_f == 16 && p.hs_b == 16);
  check_units(p.grid_f, p.hs_f, h);
  check_units(p.grid_b, p.hs_b, h);
  EXPECT(p.bp == 16 * p.nf && p.bp >= b && p.bp - b < 16 && p.bp <= 256);
  EXPECT(p.nfw == 1 || p.nfw == 2);
  check_fragments(p);
  EXPECT(p.kp % kWideKStep == 0 && p.kp >= h && p.kp - h < kWideKStep);
  EXPECT(p.ks_f * kWideKStep == p.kp);
  EXPECT(p.hq % 4 == 0 && p.hq >= h && p.hq - h < 4);
  EXPECT(p.gp % kWideKStep == 0 && p.gp >= 4 * p.hq &&
         p.gp - 4 * p.hq < kWideKStep);
  EXPECT(p.ks_b * kWideKStep == p.gp);
  // A lane's four published units stay inside the exchange row.
  EXPECT(p.grid_f * p.hs_f <= p.kp && p.grid_b * p.hs_b <= p.kp);
  // Weight rows: 16-byte aligned, an odd number of 16-byte units apart.
  EXPECT(p.ldw == p.kp + kWidePad && (p.ldw / 8) % 2 == 1 && p.ldw % 8 == 0);
  EXPECT(p.ldg == p.gp + kWidePad && (p.ldg / 8) % 2 == 1 && p.ldg % 8 == 0);
  EXPECT(p.lds_f == 2ll * 64 * p.ldw && p.lds_b == 2ll * 16 * p.ldg);
  EXPECT(p.lds_f > 0 && p.lds_f <= kWideLdsLimit);
  EXPECT(p.lds_b > 0 && p.lds_b <= kWideLdsLimit);
  return 1;
}

int main() {
  long plans = 0;
  for (int b = 0; b <= 300; ++b) {
    for (int h = 0; h <= 1100; ++h) plans += check_plan(b, h);
  }
  // The largest shape: 64 workgroups, 16 fragments, 129 KiB and 128.25 KiB.
  {
    g_b = 256, g_h = 1024;
    const LstmGateWidePlan p = lstm_gate_wide_plan(256, 1024);
    EXPECT(p.ok && p.grid_f == 64 && p.nf == 16 && p.nfw == 2);
    EXPECT(p.ks_f == 32 && p.ks_b == 128 && p.lds_f == 132096);
    EXPECT(p.lds_b == 131328);
    const LstmGateWidePlan q = lstm_gate_wide_plan(138, 519);
    EXPECT(q.ok && q.grid_f == 33 && q.nf == 9 && q.nfw == 2 && q.kp == 544);
    EXPECT(q.hq == 520 && q.gp == 2080 && q.ks_b == 65);
  }
  EXPECT(!lstm_gate_wide_plan(-1, 8).ok && !lstm_gate_wide_plan(8, -1).ok);
  EXPECT(!lstm_gate_wide_plan(1ll << 40, 8).ok);
  EXPECT(!lstm_gate_wide_plan(8, 1ll << 40).ok);
  if (failures) {
    std::fprintf(stderr, "lstm_gate_wide_plan: %d failures\n", failures);
    return 1;
  }
  std::printf("lstm_gate_wide_plan ok: %ld plans / ALL OK\n", plans);
  return 0;
}
