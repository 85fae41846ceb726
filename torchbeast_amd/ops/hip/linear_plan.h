// Host-side planner for the bf16 MFMA linear layer (linear_mfma.hip). Plain
// C++: no torch, no HIP, so tests/cc/linear_plan.cc can sweep it on the CPU.
//
// y[M, N] = x[M, K] . W[N, K]^T. Every kernel of the family computes 64 x 64
// output tiles with one 256-thread workgroup and walks its contraction axis in
// steps of 32 (one v_mfma_f32_16x16x32_bf16 deep).
//
// Forward: ceil(M / 64) x N / 64 tiles. At serve sizes (M = 64..256) that is
// 8 to 32 workgroups on 256 CUs, so K is cut into `slices` runs of k-steps,
// one workgroup per (tile, slice); fp32 partials are summed in slice order by
// linear_reduce_kernel, which applies bias and ReLU. slices is the smallest
// count that reaches kLinTargetBlocks workgroups, at most kLinMaxSlices (the
// reduce walks the slices serially) and never so many that a slice has fewer
// than kLinMinSliceSteps k-steps. One slice finishes in the GEMM kernel.
//
// Dgrad: the same kernel over ceil(M / 64) x ceil(K / 64) tiles, contraction
// over N, never sliced.
//
// Wgrad: N / 64 x ceil(K / 64) tiles, contraction over M in staging rounds of
// kLinWgradRound rows. When the tiles alone do not reach kLinTargetBlocks the
// rounds are dealt to `chunks` workgroups per tile, reduced like the slices.
//
// linear_split deals `total` units to `parts` as evenly as floor division
// does: part i gets [split(i), split(i + 1)), never empty while
// parts <= total.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define TBAMD_LIN_HD __host__ __device__
#else
#define TBAMD_LIN_HD
#endif

namespace tbamd {

constexpr int kLinTile = 64;
constexpr int kLinKStep = 32;
constexpr int kLinTargetBlocks = 256;  // one workgroup per CU
constexpr int kLinMaxSlices = 32;
constexpr int kLinMinSliceSteps = 2;
constexpr int kLinWgradRound = 128;
constexpr int kLinMaxChunks = 32;
constexpr int64_t kLinMaxM = (1ll << 31) - 256;

struct LinearPlan {
  bool ok = false;
  int tiles_m = 0;   // ceil(M / 64)
  int tiles_n = 0;   // N / 64
  int tiles_k = 0;   // ceil(K / 64): dgrad and wgrad output columns
  int ksteps = 0;    // K / 32
  int slices = 0;    // forward K-slices
  int rounds = 0;    // ceil(M / 128): wgrad staging rounds
  int chunks = 0;    // wgrad M-chunks
};

TBAMD_LIN_HD inline int linear_split(int total, int parts, int i) {
  return (int)((int64_t)total * i / parts);
}

inline LinearPlan linear_plan(int64_t m, int64_t n, int64_t k) {
  LinearPlan p;
  if (m < 1 || m > kLinMaxM) return p;
  if (n < kLinTile || n % kLinTile != 0) return p;
  if (k < kLinKStep || k % kLinKStep != 0) return p;
  // Grid y carries the column tiles: 16 bits.
  if (n / kLinTile > 65535 || (k + kLinTile - 1) / kLinTile > 65535) return p;
  p.tiles_m = (int)((m + kLinTile - 1) / kLinTile);
  p.tiles_n = (int)(n / kLinTile);
  p.tiles_k = (int)((k + kLinTile - 1) / kLinTile);
  p.ksteps = (int)(k / kLinKStep);
  p.rounds = (int)((m + kLinWgradRound - 1) / kLinWgradRound);

  const int64_t tiles = (int64_t)p.tiles_m * p.tiles_n;
  int64_t s = (kLinTargetBlocks + tiles - 1) / tiles;
  if (s > kLinMaxSlices) s = kLinMaxSlices;
  if (s > p.ksteps / kLinMinSliceSteps) s = p.ksteps / kLinMinSliceSteps;
  p.slices = s < 1 ? 1 : (int)s;

  const int64_t wtiles = (int64_t)p.tiles_n * p.tiles_k;
  int64_t c = (kLinTargetBlocks + wtiles - 1) / wtiles;
  if (c > kLinMaxChunks) c = kLinMaxChunks;
  if (c > p.rounds) c = p.rounds;
  p.chunks = c < 1 ? 1 : (int)c;
  p.ok = true;
  return p;
}

}  // namespace tbamd
