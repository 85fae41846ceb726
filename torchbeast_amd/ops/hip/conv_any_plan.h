// Host-side planner for the run-time-geometry 3x3 s1 p1 MFMA convs
// (conv_mfma.hip: conv_any_kernel, wgrad_any_kernel). Plain C++: no torch,
// no HIP, so tests/cc/conv_any_plan.cc can sweep it on the CPU.
//
// Forward/dgrad: one 512-thread workgroup per (sample, band of R output
// rows). It stages the band's zero-padded input tile, (R + 2) x (W + 2) x CI
// bf16, in LDS and owns ceil(R * W / 16) accumulator fragments, dealt
// round-robin to its 8 waves. R is the largest row count that
//   (a) keeps the band within 8 waves x kConvAnyMaxCap fragments,
//   (b) keeps the tile within kConvAnyLdsBudget (two workgroups per CU),
//   (c) still gives n * bands >= kConvAnyMinBlocks workgroups, unless that
//       would leave a band with fewer than one fragment per wave (128
//       positions): a grid of starved workgroups is slower than a short one.
// The bands are then evened out (R = ceil(H / bands)), so the last band is
// short by less than one row per band.
//
// Wgrad: the N*H*W output positions are cut into chunks of MC positions
// (a multiple of the kernel's 64-position staging round), one workgroup per
// (chunk, ky). MC aims at kConvAnyWgradChunks chunks and is at least 256:
// 3 x 256 workgroups are all resident at once on 256 CUs, and
// reduce_partials_kernel walks the chunk axis serially in each thread, so
// more, shorter chunks only lengthen the reduction (measured: 441 chunks
// took 2.3x the time of 56 at 16->16 @42, N = 64).
#pragma once

#include <cstdint>

namespace tbamd {

constexpr int kConvAnyMaxDim = 256;
constexpr int kConvAnyWaves = 8;
constexpr int kConvAnyMaxCap = 5;   // accumulator fragments per wave
constexpr int kConvAnyLdsBudget = 64 * 1024;
constexpr int kConvAnyMinBlocks = 512;  // 2 per CU on 256 CUs
constexpr int kConvAnyWgradChunks = 256;
constexpr int kConvAnyWgradStep = 64;

struct ConvAnyPlan {
  bool ok = false;
  // forward / dgrad
  int rows = 0;        // output rows per band (R)
  int bands = 0;       // ceil(H / R)
  int lds_bytes = 0;   // (R + 2) * (W + 2) * CI * 2, rounded up to 128
  int cap = 0;         // fragment-capacity instantiation: 2 or 5
  uint32_t magic_w = 0;    // m / W  == (m * magic_w) >> 20, m < 1024
  uint32_t magic_cpr = 0;  // i / cpr == umulhi(i, magic_cpr), i < 4096
  // wgrad
  int mc = 0;              // positions per chunk
  int64_t nchunks = 0;     // ceil(N*H*W / MC)
  uint32_t magic_hw = 0;   // floor(2^32 / (H*W)) (see conv_any_div)
  uint32_t magic_w32 = 0;  // floor(2^32 / W)
};

// Exact m / d for any uint32 m, given magic = conv_any_magic32(d): the
// estimate is short by at most one.
inline uint32_t conv_any_magic32(uint32_t d) {
  return d == 1 ? 0xFFFFFFFFu : (uint32_t)((1ull << 32) / d);
}
inline uint32_t conv_any_div(uint32_t m, uint32_t d, uint32_t magic) {
  uint32_t q = (uint32_t)(((uint64_t)m * magic) >> 32);
  if (m - q * d >= d) ++q;
  return q;
}

inline bool conv_any_channels_ok(int64_t ci, int64_t co) {
  return (ci == 8 && co == 16) || (ci == 16 && (co == 16 || co == 32)) ||
         (ci == 32 && (co == 16 || co == 32));
}

// 16 B chunks per staged LDS row.
inline int conv_any_cpr(int ci, int w) { return (w + 2) * ci / 8; }

inline ConvAnyPlan conv_any_plan(int64_t ci, int64_t h, int64_t w, int64_t co,
                                 int64_t n) {
  ConvAnyPlan p;
  if (!conv_any_channels_ok(ci, co)) return p;
  if (h < 1 || w < 1 || h > kConvAnyMaxDim || w > kConvAnyMaxDim) return p;
  if (n < 1 || n * h * w >= (1ll << 31)) return p;
  const int H = (int)h, W = (int)w, CI = (int)ci;

  const int row_bytes = (W + 2) * CI * 2;
  const int r_frag = (kConvAnyWaves * kConvAnyMaxCap * 16) / W;  // >= 2
  const int r_lds = kConvAnyLdsBudget / row_bytes - 2;
  if (r_lds < 1) return p;
  int r_max = r_frag < r_lds ? r_frag : r_lds;
  if (r_max > H) r_max = H;
  // (c): the bands wanted for the grid, and the rows that gives.
  const int64_t want_bands = (kConvAnyMinBlocks + n - 1) / n;
  int r_grid = want_bands >= H ? 1 : (int)(H / want_bands);
  const int r_work = (128 + W - 1) / W;
  int r = r_grid > r_work ? r_grid : r_work;
  if (r > r_max) r = r_max;
  p.bands = (H + r - 1) / r;
  p.rows = (H + p.bands - 1) / p.bands;
  p.lds_bytes = ((p.rows + 2) * row_bytes + 127) / 128 * 128;
  const int frags = (p.rows * W + 15) / 16;
  const int need = (frags + kConvAnyWaves - 1) / kConvAnyWaves;
  p.cap = need <= 2 ? 2 : kConvAnyMaxCap;
  p.magic_w = ((1u << 20) + W - 1) / W;
  p.magic_cpr = 0xFFFFFFFFu / (uint32_t)conv_any_cpr(CI, W) + 1;

  const int64_t M = n * h * w;
  int64_t mc = (M + kConvAnyWgradChunks - 1) / kConvAnyWgradChunks;
  mc = (mc + kConvAnyWgradStep - 1) / kConvAnyWgradStep * kConvAnyWgradStep;
  if (mc < 256) mc = 256;
  p.mc = (int)mc;
  p.nchunks = (M + mc - 1) / mc;
  p.magic_hw = conv_any_magic32((uint32_t)(H * W));
  p.magic_w32 = conv_any_magic32((uint32_t)W);
  p.ok = true;
  return p;
}

}  // namespace tbamd
