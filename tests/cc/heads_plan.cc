// Stand-alone sweep of the MFMA heads planner
// (torchbeast_amd/ops/hip/heads_plan.h): every M in 1..4096 and D in 1..1024
// with A and the form cycling, every (A, form) at a spread of (M, D), and
// the largest admitted sizes.
//
// CPU only, no torch and no HIP; built plain and with
// -fsanitize=address,undefined. See README_heads_plan.md.

#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "heads_plan.h"

using namespace tbamd;

static int failures = 0;
static int64_t g_m, g_d, g_e, g_a;
#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond) && ++failures <= 20) {                                      \
      std::fprintf(stderr, "EXPECT failed: %s (line %d) m=%lld d=%lld "     \
                   "extra=%lld a=%lld\n", #cond, __LINE__, (long long)g_m,  \
                   (long long)g_d, (long long)g_e, (long long)g_a);         \
    }                                                                       \
  } while (0)

static int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

static long check_plan(int64_t m, int64_t d, int64_t extra, int64_t a) {
  g_m = m, g_d = d, g_e = extra, g_a = a;
  const HeadsPlan p = heads_plan(m, d, extra, a);
  EXPECT(p.ok && heads_form_ok(d, extra, a));
  if (!p.ok) return 0;
  EXPECT(p.np == 16 * p.nf && p.np >= a + 1 && p.np - 16 < a + 1);
  EXPECT(p.nf >= 1 && p.nf <= 4 && p.kc == d + extra);
  EXPECT(p.tiles_m == ceil_div(m, kHeadsRows));
  EXPECT(p.tiles_mx == ceil_div(m, kHeadsDxRows));
  EXPECT(p.tiles_d == ceil_div(d, kHeadsKTile) && p.tiles_d <= 65535);
  EXPECT(p.tiles_k == ceil_div(d + extra, kHeadsKTile));
  EXPECT(p.rounds == ceil_div(m, kHeadsRound));
  // Chunks: grid y, never empty, no more than the target needs.
  EXPECT(p.chunks >= 1 && p.chunks <= kHeadsMaxChunks && p.chunks <= p.rounds);
  EXPECT(p.chunks == 1 ||
         (int64_t)p.tiles_k * (p.chunks - 1) < kHeadsTargetBlocks);
  EXPECT(heads_split(p.rounds, p.chunks, 0) == 0);
  EXPECT(heads_split(p.rounds, p.chunks, p.chunks) == p.rounds);
  for (int i = 0; i < p.chunks; ++i) {
    const int len = heads_split(p.rounds, p.chunks, i + 1) -
                    heads_split(p.rounds, p.chunks, i);
    EXPECT(len >= 1 && len >= p.rounds / p.chunks &&
           len <= p.rounds / p.chunks + 1);
  }
  // Static LDS stays under the 64 KiB a workgroup may declare.
  EXPECT(heads_lds_fwd(p.nf) <= 65536 && heads_lds_dgrad(p.nf) <= 65536 &&
         heads_lds_wgrad(p.nf) <= 65536);
  return 1;
}

static int64_t extra_of(int form, int64_t a) {
  return form == 0 ? 0 : form == 1 ? 1 : 1 + a;
}

int main() {
  long plans = 0;
  for (int64_t m = 1; m <= 4096; ++m) {
    for (int64_t d = 1; d <= 1024; ++d) {
      const int64_t a = 1 + (m * 31 + d * 7) % kHeadsMaxA;
      plans += check_plan(m, d, extra_of((int)((m + d) % 3), a), a);
    }
  }
  for (int64_t a = 1; a <= kHeadsMaxA; ++a) {
    for (int form = 0; form < 3; ++form) {
      for (int64_t m : {(int64_t)1, (int64_t)81, (int64_t)2592, kHeadsMaxM}) {
        for (int64_t d : {(int64_t)1, (int64_t)512, kHeadsMaxK - 64}) {
          plans += check_plan(m, d, extra_of(form, a), a);
        }
      }
    }
  }
  // The learner's shapes: 9 column tiles, 41 (40) rounds in 29 chunks.
  {
    const HeadsPlan p = heads_plan(2592, 512, 7, 6);
    g_m = 2592, g_d = 512, g_e = 7, g_a = 6;
    EXPECT(p.ok && p.nf == 1 && p.tiles_m == 162 && p.tiles_k == 9);
    EXPECT(p.rounds == 41 && p.chunks == 29 && p.tiles_mx == 41);
    const HeadsPlan q = heads_plan(2560, 256, 0, 15);
    EXPECT(q.ok && q.nf == 1 && q.tiles_k == 4 && q.chunks == 32);
    const HeadsPlan r = heads_plan(kHeadsRound + 17, 257, 1, 6);
    EXPECT(r.ok && r.rounds == 2 && r.chunks == 2);
  }
  // Refused.
  g_m = g_d = g_e = g_a = -1;
  EXPECT(!heads_plan(0, 8, 0, 6).ok && !heads_plan(kHeadsMaxM + 1, 8, 0, 6).ok);
  EXPECT(!heads_plan(5, 0, 0, 6).ok && !heads_plan(5, 8, 0, 0).ok);
  EXPECT(!heads_plan(5, 8, 0, 64).ok && !heads_plan(5, 8, 2, 6).ok);
  EXPECT(!heads_plan(5, 8, 6, 6).ok && !heads_plan(5, 8, -1, 6).ok);
  EXPECT(!heads_plan(5, kHeadsMaxK, 1, 6).ok && heads_plan(5, kHeadsMaxK, 0, 6).ok);

  if (failures) {
    std::fprintf(stderr, "heads_plan: %d failures\n", failures);
    return 1;
  }
  std::printf("heads_plan ok: %ld plans / ALL OK\n", plans);
  return 0;
}
