// Stand-alone sweep of the LSTM projection planner
// (torchbeast_amd/ops/hip/lstm_proj_plan.h): every M in 1..600 and a spread
// of larger ones, I and H in 1..140 and around 257, 519 and 1024.
//
// CPU only, no torch and no HIP; built plain and with
// -fsanitize=address,undefined. See README_lstm_proj_plan.md.

#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "lstm_proj_plan.h"

using namespace tbamd;

static int failures = 0;
static int64_t g_m, g_i, g_h;
#define EXPECT(cond)                                                       \
  do {                                                                     \
    if (!(cond) && ++failures <= 20) {                                     \
      std::fprintf(stderr, "EXPECT failed: %s (%s:%d) m=%lld i=%lld "      \
                   "h=%lld\n", #cond, __FILE__, __LINE__, (long long)g_m,  \
                   (long long)g_i, (long long)g_h);                        \
    }                                                                      \
  } while (0)

// `tiles` tiles of `unit` cover [0, n) once: the last one short, never empty.
static void check_cover(int tiles, int unit, int64_t n) {
  EXPECT((int64_t)tiles * unit >= n);
  EXPECT((int64_t)(tiles - 1) * unit < n);
}

// Parts [split(i), split(i + 1)) cover [0, total) once, none empty.
static void check_split(int total, int parts, int min_len) {
  EXPECT(parts >= 1 && parts <= total);
  EXPECT(lstm_proj_split(total, parts, 0) == 0);
  EXPECT(lstm_proj_split(total, parts, parts) == total);
  for (int i = 0; i < parts; ++i) {
    const int len = lstm_proj_split(total, parts, i + 1) -
                    lstm_proj_split(total, parts, i);
    EXPECT(len >= total / parts && len <= total / parts + 1 && len >= 1);
    EXPECT(parts == 1 || len >= min_len);
  }
}

static long check_plan(int64_t m, int64_t i, int64_t h) {
  g_m = m, g_i = i, g_h = h;
  const LstmProjPlan p = lstm_proj_plan(m, i, h);
  EXPECT(p.ok);
  if (!p.ok) return 0;
  EXPECT(p.n4 == 4 * h);
  check_cover(p.tiles_m, kProjTile, m);
  check_cover(p.tiles_n4, kProjTile, p.n4);
  // The virtual operand [in | hm]: I + H columns, each in exactly one tile,
  // no tile across the boundary.
  check_cover(p.tiles_i, kProjTile, i);
  check_cover(p.tiles_h, kProjTile, h);
  check_cover(p.rounds, kProjRound, m);
  // Packs: the k-steps cover the contraction, padded by less than a step.
  EXPECT(p.ip >= i && p.ip - i < kProjKStep && p.ip % kProjKStep == 0);
  EXPECT(p.np >= p.n4 && p.np - p.n4 < kProjKStep && p.np % kProjKStep == 0);
  EXPECT(p.fwd_ksteps * kProjKStep == p.ip);
  EXPECT(p.dgrad_ksteps * kProjKStep == p.np);
  // Grid limits: x 31 bits, y and z 16 bits.
  EXPECT(p.tiles_n4 <= 65535 && p.tiles_i + p.tiles_h <= 65535);
  EXPECT(p.fwd_slices <= kProjMaxSlices && p.dgrad_slices <= kProjMaxSlices);
  EXPECT(p.chunks <= kProjMaxChunks);
  check_split(p.fwd_ksteps, p.fwd_slices, kProjMinSliceSteps);
  check_split(p.dgrad_ksteps, p.dgrad_slices, kProjMinSliceSteps);
  check_split(p.rounds, p.chunks, 1);
  // No more parts than reaching the target needs.
  if (p.fwd_slices > 1) {
    EXPECT((int64_t)p.tiles_m * p.tiles_n4 * (p.fwd_slices - 1) <
           kProjTargetBlocks);
  }
  if (p.dgrad_slices > 1) {
    EXPECT((int64_t)p.tiles_m * p.tiles_i * (p.dgrad_slices - 1) <
           kProjTargetBlocks);
  }
  if (p.chunks > 1) {
    EXPECT((int64_t)p.tiles_n4 * (p.tiles_i + p.tiles_h) * (p.chunks - 1) <
           kProjTargetBlocks);
  }
  EXPECT(p.slab == 4 * h * (i + h) + 4 * h);
  EXPECT(p.lds_nt > 0 && p.lds_nt <= kProjLdsLimit);
  EXPECT(p.lds_wgrad > 0 && p.lds_wgrad <= kProjLdsLimit);
  EXPECT(p.lds_nt == 2 * 2 * kProjTile * kProjLdsK * 2);
  EXPECT(p.lds_wgrad ==
         2 * 2 * kProjTile * kProjLdsM * 2 + 16 * kProjTile * 4);
  return 1;
}

int main() {
  std::vector<int64_t> widths;
  for (int64_t w = 1; w <= 140; ++w) widths.push_back(w);
  for (int64_t w : {255, 256, 257, 511, 512, 513, 519, 521, 1023, 1024, 1025})
    widths.push_back(w);
  long plans = 0;
  for (int64_t i : widths) {
    for (int64_t h : widths) {
      for (int64_t m = 1; m <= 5000; m += (m < 600 ? 1 : 61)) {
        plans += check_plan(m, i, h);
      }
      for (int64_t m :
           {(int64_t)65537, (int64_t)1 << 20, kProjMaxM - 1, kProjMaxM}) {
        plans += check_plan(m, i, h);
      }
    }
  }
  plans += check_plan(5, kProjMaxWidth, kProjMaxWidth);
  // The shapes the issue names.
  {
    const LstmProjPlan p = lstm_proj_plan(2560, 519, 519);
    g_m = 2560, g_i = g_h = 519;
    EXPECT(p.ok && p.tiles_m == 40 && p.tiles_n4 == 33 && p.tiles_i == 9);
    EXPECT(p.tiles_h == 9 && p.fwd_slices == 1 && p.dgrad_slices == 1);
    EXPECT(p.chunks == 1 && p.dgrad_ksteps == 65 && p.fwd_ksteps == 17);
    const LstmProjPlan q = lstm_proj_plan(2560, 257, 256);
    g_i = 257, g_h = 256;
    // 16 x 9 wgrad tiles: 20 rounds in two chunks; 40 x 5 dgrad tiles: two
    // slices of 16 k-steps.
    EXPECT(q.ok && q.tiles_n4 == 16 && q.tiles_i + q.tiles_h == 9);
    EXPECT(q.chunks == 2 && q.rounds == 20 && q.dgrad_slices == 2);
    const LstmProjPlan r = lstm_proj_plan(130, 257, 256);
    g_m = 130;
    EXPECT(r.ok && r.rounds == 2 && r.chunks == 2);
  }
  // Refused shapes.
  g_m = g_i = g_h = -1;
  EXPECT(!lstm_proj_plan(0, 5, 5).ok && !lstm_proj_plan(-1, 5, 5).ok);
  EXPECT(!lstm_proj_plan(kProjMaxM + 1, 5, 5).ok);
  EXPECT(!lstm_proj_plan(5, 0, 5).ok && !lstm_proj_plan(5, 5, 0).ok);
  EXPECT(!lstm_proj_plan(5, -3, 5).ok && !lstm_proj_plan(5, 5, -3).ok);
  EXPECT(!lstm_proj_plan(5, kProjMaxWidth + 1, 5).ok);
  EXPECT(!lstm_proj_plan(5, 5, kProjMaxWidth + 1).ok);

  if (failures) {
    std::fprintf(stderr, "lstm_proj_plan: %d failures\n", failures);
    return 1;
  }
  std::printf("lstm_proj_plan ok: %ld plans / ALL OK\n", plans);
  return 0;
}
