// Host-side planner for the persistent MFMA LSTM unroll kernels
// (lstm_gate_mfma.hip). Plain C++: no torch, no HIP, so
// tests/cc/lstm_gate_plan.cc can sweep it on the CPU.
//
// One layer, batch B, hidden width H. Both kernels run 8 waves per
// workgroup; the waves deal the k-steps (32 deep, one
// v_mfma_f32_16x16x32_bf16) round-robin and keep their W_hh fragments in
// registers for the whole unroll, so the k-step count bounds the shapes:
//
//   forward   gates[4 hs_f, B] += W_hh[rows of hs_f units, H] . h[B, H]^T
//             hs_f in {4, 8, 16} units per workgroup = 1, 2, 4 M fragments;
//             K = H in kp / 32 k-steps, at most kGateFwdKpw per wave.
//             Exchange buffer: bf16 [2][bp][kp], kp = H rounded up to 32.
//   backward  dh[hs_b, B] = W_hh[:, hs_b units]^T . dgates[B, 4 hq]^T
//             hs_b in {16, 32} units = 1, 2 M fragments; the contraction
//             index is gate * hq + unit with hq = H rounded up to 4, so the
//             four bf16 a lane group publishes are one aligned 8-byte word
//             that no other workgroup writes. K in gp / 32 k-steps, at most
//             kGateBwdKpw per wave. Exchange buffer: bf16 [2][bp][gp],
//             gp = 4 hq rounded up to 32.
//
// The batch is the N side: nf = ceil(B / 16) fragments, bp = 16 nf rows in
// both exchange buffers; rows from B on stay zero.
#pragma once

#include <cstdint>

namespace tbamd {

constexpr int kGateWaves = 8;
constexpr int kGateThreads = 64 * kGateWaves;
constexpr int kGateKStep = 32;
constexpr int kGateFwdKpw = 4;   // forward k-steps per wave, at most
constexpr int kGateBwdKpw = 16;  // backward
constexpr int kGateMaxB = 64;
constexpr int kGateMaxH = kGateWaves * kGateFwdKpw * kGateKStep;  // 1024
constexpr int kGatePartPad = 4;  // floats between partial rows in LDS
constexpr int64_t kGateLdsLimit = 160 * 1024;  // gfx950, per workgroup

struct LstmGatePlan {
  bool ok = false;
  int hs_f = 0, hs_b = 0;      // units per workgroup
  int grid_f = 0, grid_b = 0;  // workgroups
  int nf = 0, bp = 0;          // batch fragments, padded batch
  int kp = 0, ks_f = 0;        // forward: padded K, k-steps
  int hq = 0, gp = 0, ks_b = 0;  // backward: gate pitch, padded K, k-steps
  int64_t lds_f = 0, lds_b = 0;  // bytes of dynamic LDS
};

inline int lstm_gate_ceil(int a, int b) { return (a + b - 1) / b * b; }

// Dynamic LDS of the forward: per-wave partials [waves][bp][4 hs_f + pad]
// and the cell state [B][hs_f], fp32.
inline int64_t lstm_gate_lds_f(int b, int bp, int hs_f) {
  return 4ll * kGateWaves * bp * (4 * hs_f + kGatePartPad) + 4ll * b * hs_f;
}

// Backward: partials [waves][bp][hs_b + pad], dc and dh [B][hs_b] each.
inline int64_t lstm_gate_lds_b(int b, int bp, int hs_b) {
  return 4ll * kGateWaves * bp * (hs_b + kGatePartPad) + 8ll * b * hs_b;
}

// hs_f_want / hs_b_want: 0 for the planner's pick, otherwise an override
// (TBAMD_LSTM_GATE_HS_F / _HS_B) that is taken when it is one of the
// supported sizes and fits the LDS, and ignored otherwise.
inline LstmGatePlan lstm_gate_plan(int64_t b, int64_t h, int hs_f_want = 0,
                                   int hs_b_want = 0) {
  LstmGatePlan p;
  if (b < 1 || b > kGateMaxB || h < 1 || h > kGateMaxH) return p;
  const int B = (int)b, H = (int)h;
  p.nf = (B + 15) / 16;
  p.bp = 16 * p.nf;
  p.kp = lstm_gate_ceil(H, kGateKStep);
  p.ks_f = p.kp / kGateKStep;
  p.hq = lstm_gate_ceil(H, 4);
  p.gp = lstm_gate_ceil(4 * p.hq, kGateKStep);
  p.ks_b = p.gp / kGateKStep;
  // Picks from the sweep at [T=80, B=32, H=519] (profiles/PROFILE_r14.md):
  // forward 1.00 / 0.78 / 0.74 ms per layer at hs_f = 4 / 8 / 16 (130 / 65 /
  // 33 workgroups: the barrier, not the matrix work, is what a step costs),
  // backward 1.35 / 1.66 ms at hs_b = 16 / 32.
  p.hs_f = 16;
  p.hs_b = 16;
  if ((hs_f_want == 4 || hs_f_want == 8 || hs_f_want == 16) &&
      lstm_gate_lds_f(B, p.bp, hs_f_want) <= kGateLdsLimit) {
    p.hs_f = hs_f_want;
  }
  if ((hs_b_want == 16 || hs_b_want == 32) &&
      lstm_gate_lds_b(B, p.bp, hs_b_want) <= kGateLdsLimit) {
    p.hs_b = hs_b_want;
  }
  p.grid_f = (H + p.hs_f - 1) / p.hs_f;
  p.grid_b = (H + p.hs_b - 1) / p.hs_b;
  p.lds_f = lstm_gate_lds_f(B, p.bp, p.hs_f);
  p.lds_b = lstm_gate_lds_b(B, p.bp, p.hs_b);
  p.ok = p.ks_f <= kGateWaves * kGateFwdKpw &&
         p.ks_b <= kGateWaves * kGateBwdKpw && p.lds_f <= kGateLdsLimit &&
         p.lds_b <= kGateLdsLimit;
  return p;
}

}  // namespace tbamd
