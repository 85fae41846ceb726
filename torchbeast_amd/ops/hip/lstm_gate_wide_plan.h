// Host-side planner for the wide-batch persistent MFMA LSTM unroll kernels
// (lstm_gate_wide.hip). Plain C++: no torch, no HIP, so
// tests/cc/lstm_gate_wide_plan.cc can sweep it on the CPU.
//
// One layer, batch 1 <= B <= 256, hidden width 1 <= H <= 1024. Both kernels
// run 8 waves per workgroup and a workgroup owns kWideHs = 16 hidden units.
// The batch is the N side of every MFMA (v_mfma_f32_16x16x32_bf16): nf =
// ceil(B / 16) fragments, and the WAVES SPLIT THE BATCH: fragment f belongs
// to wave f % 8, slot f / 8, so a wave owns nfw = ceil(nf / 8) in {1, 2}
// fragments at most and walks all of K for them. No partial sums exist.
//
//   forward   gates[4 x 16, B] = W_hh[4 gates x 16 units, H] . h[B, H]^T
//             four M fragments, one per gate; K = H in ks_f k-steps of 32.
//             LDS: the bf16 weight slice [64][ldw], ldw = kp + kWidePad.
//             Exchange buffer: bf16 [2][bp][kp], kp = H rounded up to 32.
//   backward  dh[16, B] = W_hh[:, 16 units]^T . dgates[B, 4 hq]^T
//             one M fragment; the contraction index is gate * hq + unit with
//             hq = H rounded up to 4 (the convention of lstm_gate_plan.h).
//             LDS: the bf16 weight slice [16][ldg], ldg = gp + kWidePad.
//             Exchange buffer: bf16 [2][bp][gp], gp = 4 hq rounded up to 32.
//
// The cell state and the gradients a workgroup carries from step to step
// live in registers, so the weight slice is all the dynamic LDS there is.
//
// Units per workgroup are fixed at 16: the cell path is lane-local only when
// one M fragment holds one gate of 16 units (see lstm_gate_wide.hip), and
// every workgroup reads the whole exchange buffer once per step, so a smaller
// slice multiplies that traffic by the larger grid.
#pragma once

#include <cstdint>

namespace tbamd {

constexpr int kWideWaves = 8;
constexpr int kWideThreads = 64 * kWideWaves;
constexpr int kWideKStep = 32;
constexpr int kWideHs = 16;   // units per workgroup, both directions
constexpr int kWidePad = 8;   // bf16 between weight rows in LDS (16 bytes)
constexpr int kWideMaxB = 256;
constexpr int kWideMaxH = 1024;
constexpr int64_t kWideLdsLimit = 160 * 1024;  // gfx950, per workgroup

struct LstmGateWidePlan {
  bool ok = false;
  int hs_f = 0, hs_b = 0;      // units per workgroup
  int grid_f = 0, grid_b = 0;  // workgroups
  int nf = 0, bp = 0, nfw = 0;  // batch fragments, padded batch, per wave
  int kp = 0, ks_f = 0, ldw = 0;         // forward: padded K, k-steps, pitch
  int hq = 0, gp = 0, ks_b = 0, ldg = 0;  // backward
  int64_t lds_f = 0, lds_b = 0;  // bytes of dynamic LDS
};

inline int lstm_gate_wide_ceil(int a, int b) { return (a + b - 1) / b * b; }

// The wave and the register slot that own batch fragment f.
inline int lstm_gate_wide_wave(int f) { return f % kWideWaves; }
inline int lstm_gate_wide_slot(int f) { return f / kWideWaves; }

inline LstmGateWidePlan lstm_gate_wide_plan(int64_t b, int64_t h) {
  LstmGateWidePlan p;
  if (b < 1 || b > kWideMaxB || h < 1 || h > kWideMaxH) return p;
  const int B = (int)b, H = (int)h;
  p.hs_f = p.hs_b = kWideHs;
  p.grid_f = p.grid_b = (H + kWideHs - 1) / kWideHs;
  p.nf = (B + 15) / 16;
  p.bp = 16 * p.nf;
  p.nfw = (p.nf + kWideWaves - 1) / kWideWaves;
  p.kp = lstm_gate_wide_ceil(H, kWideKStep);
  p.ks_f = p.kp / kWideKStep;
  p.ldw = p.kp + kWidePad;
  p.hq = lstm_gate_wide_ceil(H, 4);
  p.gp = lstm_gate_wide_ceil(4 * p.hq, kWideKStep);
  p.ks_b = p.gp / kWideKStep;
  p.ldg = p.gp + kWidePad;
  p.lds_f = 2ll * 4 * kWideHs * p.ldw;
  p.lds_b = 2ll * kWideHs * p.ldg;
  p.ok = p.nfw <= 2 && p.lds_f <= kWideLdsLimit && p.lds_b <= kWideLdsLimit;
  return p;
}

}  // namespace tbamd
