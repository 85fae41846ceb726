// Host-side planner for the fp32 MFMA learner heads (heads_mfma.hip). Plain
// C++: no torch, no HIP, so tests/cc/heads_plan.cc can sweep it on the CPU.
//
// The A policy rows and the baseline row are one operand of
// NP = 16 ceil((A + 1) / 16) rows (NF = NP / 16 fragments, at most 4). The
// core input is [M, Kc], Kc = D + extra: D real columns of x and `extra`
// synthesised ones (0: plain, 1: clipped reward, 1 + A: reward and one-hot
// last action).
//
// Forward: one 256-thread workgroup per 16 rows, all NP outputs, K walked in
// tiles of kHeadsKTile columns whose 16 k-steps are dealt to the four waves.
//
// dX: 64 x 64 tiles of dx[M, D], contraction over the A + 1 head rows.
//
// dW/db: ceil(Kc / 64) column tiles, contraction over M in staging rounds of
// kHeadsRound rows. The tiles alone never reach kHeadsTargetBlocks, so the
// rounds are dealt to `chunks` workgroups per tile (the chunk rule of
// linear_plan.h): the smallest count that reaches the target, at most
// kHeadsMaxChunks (heads_reduce_kernel walks the chunks serially) and never
// more than there are rounds.
//
// heads_split deals `total` units to `parts` as evenly as floor division
// does: part i gets [split(i), split(i + 1)), never empty while
// parts <= total.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define TBAMD_HEADS_HD __host__ __device__
#else
#define TBAMD_HEADS_HD
#endif

namespace tbamd {

constexpr int kHeadsMaxA = 63;
constexpr int kHeadsRows = 16;    // forward rows per workgroup
constexpr int kHeadsKTile = 64;   // columns per staged tile, all kernels
constexpr int kHeadsDxRows = 64;  // dX rows per workgroup
constexpr int kHeadsRound = 64;   // dW rows per staging round
constexpr int kHeadsTargetBlocks = 256;  // one workgroup per CU
constexpr int kHeadsMaxChunks = 32;
constexpr int64_t kHeadsMaxM = (1ll << 31) - 256;
constexpr int64_t kHeadsMaxK = 65535ll * kHeadsKTile;  // grid y: 16 bits
// LDS row strides in floats: rows stay 16-byte aligned, and the fragment
// reads (16 rows x 4 k, or 4 k x 16 columns) spread over the banks.
constexpr int kHeadsLdsK = kHeadsKTile + 4;
constexpr int kHeadsLdsC = kHeadsKTile + 8;

struct HeadsPlan {
  bool ok = false;
  int np = 0;        // 16 ceil((A + 1) / 16)
  int nf = 0;        // np / 16
  int kc = 0;        // D + extra
  int tiles_m = 0;   // forward: ceil(M / 16)
  int tiles_mx = 0;  // dX: ceil(M / 64)
  int tiles_d = 0;   // dX: ceil(D / 64)
  int tiles_k = 0;   // dW: ceil(Kc / 64)
  int rounds = 0;    // dW: ceil(M / 64)
  int chunks = 0;    // dW: M-chunks
};

TBAMD_HEADS_HD inline int heads_split(int total, int parts, int i) {
  return (int)((int64_t)total * i / parts);
}

// The three forms of the core input, and the range of A.
inline bool heads_form_ok(int64_t d, int64_t extra, int64_t a) {
  if (a < 1 || a > kHeadsMaxA) return false;
  if (d < 1 || d > kHeadsMaxK) return false;
  if (extra != 0 && extra != 1 && extra != 1 + a) return false;
  return d + extra <= kHeadsMaxK;
}

inline HeadsPlan heads_plan(int64_t m, int64_t d, int64_t extra, int64_t a) {
  HeadsPlan p;
  if (m < 1 || m > kHeadsMaxM || !heads_form_ok(d, extra, a)) return p;
  p.nf = (int)((a + 1 + 15) / 16);
  p.np = 16 * p.nf;
  p.kc = (int)(d + extra);
  p.tiles_m = (int)((m + kHeadsRows - 1) / kHeadsRows);
  p.tiles_mx = (int)((m + kHeadsDxRows - 1) / kHeadsDxRows);
  p.tiles_d = (int)((d + kHeadsKTile - 1) / kHeadsKTile);
  p.tiles_k = (p.kc + kHeadsKTile - 1) / kHeadsKTile;
  p.rounds = (int)((m + kHeadsRound - 1) / kHeadsRound);
  int64_t c = (kHeadsTargetBlocks + p.tiles_k - 1) / p.tiles_k;
  if (c > kHeadsMaxChunks) c = kHeadsMaxChunks;
  if (c > p.rounds) c = p.rounds;
  p.chunks = (int)c;
  p.ok = true;
  return p;
}

// Static LDS of each kernel in bytes for nf fragments; the kernels size
// their arrays by the same expressions.
constexpr int64_t heads_lds_fwd(int nf) {
  return 4ll * (kHeadsRows * kHeadsLdsK + 16 * nf * kHeadsLdsK + 4 * nf * 256);
}
constexpr int64_t heads_lds_dgrad(int nf) {
  return 4ll * (kHeadsDxRows * (16 * nf + 4) + 16 * nf * kHeadsLdsC +
                kHeadsDxRows * kHeadsLdsK);
}
constexpr int64_t heads_lds_wgrad(int nf) {
  return 4ll * (kHeadsRound * (16 * nf + 8) + kHeadsRound * kHeadsLdsC +
                4 * 16 * nf);
}

}  // namespace tbamd
