// Host-side planner for the bf16 MFMA LSTM projection kernels
// (lstm_proj_mfma.hip). Plain C++: no torch, no HIP, so
// tests/cc/lstm_proj_plan.cc can sweep it on the CPU.
//
// One LSTM layer with M = T * B rows, input width I and hidden width H has
//   forward  precomp[M, 4H] = in[M, I] . W_ih[4H, I]^T + (b_ih + b_hh)
//   dgrad    dx[M, I]       = dg[M, 4H] . W_ih[4H, I]
//   wgrad    dW_ih[4H, I]   = dg^T . in,  dW_hh[4H, H] = dg^T . hm,
//            db[4H]         = column sums of dg
// for any M, I, H >= 1. Every kernel computes 64 x 64 output tiles with one
// 256-thread workgroup and walks its contraction axis in k-steps of 32 (one
// v_mfma_f32_16x16x32_bf16 deep) through two LDS buffers.
//
// Packs: wb = bf16 [4H, Ip], wt = bf16 [I, Np], Ip and Np being I and 4H
// rounded up to the k-step and the padding zeros, so the K-loops of forward
// (Ip / 32 steps) and dgrad (Np / 32 steps) never see a tail on the weight
// side.
//
// Forward and dgrad: ceil(M / 64) x ceil(4H / 64) resp. ceil(I / 64) tiles.
// Below kProjTargetBlocks tiles the k-steps are cut into `slices` runs, one
// workgroup per (tile, slice); lstm_proj_reduce_kernel sums the fp32 partials
// in slice order (and adds the biases). A slice has at least
// kProjMinSliceSteps k-steps.
//
// Wgrad: one launch over ceil(4H / 64) x (ceil(I / 64) + ceil(H / 64)) tiles
// of the virtual right-hand operand [in | hm]; a tile never straddles the
// two. The contraction runs over M in staging rounds of kProjRound rows;
// below kProjTargetBlocks tiles the rounds are dealt to `chunks` workgroups
// per tile, reduced the same way. One slab of 4H * (I + H) + 4H floats holds
// dW_ih, dW_hh and db in that order.
//
// lstm_proj_split deals `total` units to `parts` as evenly as floor division
// does: part i gets [split(i), split(i + 1)), never empty while
// parts <= total.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define TBAMD_PROJ_HD __host__ __device__
#else
#define TBAMD_PROJ_HD
#endif

namespace tbamd {

constexpr int kProjTile = 64;
constexpr int kProjKStep = 32;
constexpr int kProjRound = 128;
constexpr int kProjTargetBlocks = 256;  // one workgroup per CU
constexpr int kProjMaxSlices = 32;
constexpr int kProjMinSliceSteps = 4;
constexpr int kProjMaxChunks = 32;
constexpr int64_t kProjMaxM = (1ll << 31) - 256;
constexpr int64_t kProjMaxWidth = 1ll << 19;  // I and H; 4H / 64 fits grid.y
constexpr int kProjLdsK = kProjKStep + 8;     // bf16 per staged row: 80 B
constexpr int kProjLdsM = kProjRound + 8;     // wgrad: 272 B
constexpr int64_t kProjLdsLimit = 160 * 1024;  // gfx950, per workgroup

struct LstmProjPlan {
  bool ok = false;
  int n4 = 0;            // 4H
  int ip = 0, np = 0;    // I and 4H rounded up to the k-step
  int tiles_m = 0;       // ceil(M / 64)
  int tiles_n4 = 0;      // ceil(4H / 64)
  int tiles_i = 0;       // ceil(I / 64)
  int tiles_h = 0;       // ceil(H / 64)
  int fwd_ksteps = 0;    // Ip / 32
  int fwd_slices = 0;
  int dgrad_ksteps = 0;  // Np / 32
  int dgrad_slices = 0;
  int rounds = 0;        // ceil(M / 128): wgrad staging rounds
  int chunks = 0;        // wgrad M-chunks
  int64_t slab = 0;      // 4H * (I + H) + 4H floats
  int64_t lds_nt = 0;    // bytes of dynamic LDS, forward and dgrad
  int64_t lds_wgrad = 0;
};

TBAMD_PROJ_HD inline int lstm_proj_split(int total, int parts, int i) {
  return (int)((int64_t)total * i / parts);
}

inline int lstm_proj_ceil(int64_t a, int b) { return (int)((a + b - 1) / b); }

inline int lstm_proj_parts(int64_t tiles, int units, int min_units, int cap) {
  int64_t s = (kProjTargetBlocks + tiles - 1) / tiles;
  if (s > cap) s = cap;
  if (s > units / min_units) s = units / min_units;
  return s < 1 ? 1 : (int)s;
}

inline LstmProjPlan lstm_proj_plan(int64_t m, int64_t i, int64_t h) {
  LstmProjPlan p;
  if (m < 1 || m > kProjMaxM) return p;
  if (i < 1 || i > kProjMaxWidth || h < 1 || h > kProjMaxWidth) return p;
  p.n4 = (int)(4 * h);
  p.ip = lstm_proj_ceil(i, kProjKStep) * kProjKStep;
  p.np = lstm_proj_ceil(p.n4, kProjKStep) * kProjKStep;
  p.tiles_m = lstm_proj_ceil(m, kProjTile);
  p.tiles_n4 = lstm_proj_ceil(p.n4, kProjTile);
  p.tiles_i = lstm_proj_ceil(i, kProjTile);
  p.tiles_h = lstm_proj_ceil(h, kProjTile);
  p.fwd_ksteps = p.ip / kProjKStep;
  p.dgrad_ksteps = p.np / kProjKStep;
  p.rounds = lstm_proj_ceil(m, kProjRound);
  p.fwd_slices =
      lstm_proj_parts((int64_t)p.tiles_m * p.tiles_n4, p.fwd_ksteps,
                      kProjMinSliceSteps, kProjMaxSlices);
  p.dgrad_slices =
      lstm_proj_parts((int64_t)p.tiles_m * p.tiles_i, p.dgrad_ksteps,
                      kProjMinSliceSteps, kProjMaxSlices);
  p.chunks = lstm_proj_parts((int64_t)p.tiles_n4 * (p.tiles_i + p.tiles_h),
                             p.rounds, 1, kProjMaxChunks);
  p.slab = (int64_t)p.n4 * (i + h) + p.n4;
  // Two buffers of an A and a B tile each; the wgrad adds the db scratch.
  p.lds_nt = 2ll * 2 * kProjTile * kProjLdsK * 2;
  p.lds_wgrad = 2ll * 2 * kProjTile * kProjLdsM * 2 + 16ll * kProjTile * 4;
  p.ok = p.lds_nt <= kProjLdsLimit && p.lds_wgrad <= kProjLdsLimit;
  return p;
}

}  // namespace tbamd
