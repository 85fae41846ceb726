// Device-side gather of an inference batch from rollout rows: the pointer
// table that gather_rows_kernel (runtime_kernels.hip) reads.
//
// In the row form every request is a row of a rollout slot inside ONE pinned
// slab, whose host addresses the GPU can read as they are. A batch of b
// requests becomes a table of b frame pointers and b reward pointers; the
// kernel copies frame r into row r of the batch and clamps reward r. The
// table lives in pinned host memory as well and is read in place, so forming
// a batch costs 16 bytes of host writes per request and no host copy of any
// frame.
//
// A wrong pointer in the table is a GPU fault, so the table is only ever
// filled through build_row_table(), which checks every range against the
// slab first.
//
// Everything in this header is host code and needs neither torch nor HIP.

#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>

namespace tbruntime {

// Widest access of 16, 8, 4 or 1 bytes that divides every value OR-ed into
// `bits` (addresses and lengths). Same rule as unpack_rollouts_kernel.
inline unsigned row_access_width(uint64_t bits) {
  if ((bits & 15u) == 0) return 16;
  if ((bits & 7u) == 0) return 8;
  if ((bits & 3u) == 0) return 4;
  return 1;
}

// Fill the table for a batch of `b` rows. frame_of(r) / reward_of(r) give
// row r's frame (`fsz` bytes) and reward (one float) addresses; every
// [frame, frame + fsz) and [reward, reward + 4) must lie inside the slab
// [slab, slab + slab_bytes) and every reward must be 4-byte aligned, else
// nothing usable is left in the table and std::out_of_range /
// std::invalid_argument is thrown. Returns the common access width of the
// frames: row_access_width over fsz and every frame address.
template <typename FrameOf, typename RewardOf>
unsigned build_row_table(int64_t b, FrameOf frame_of, RewardOf reward_of,
                         int64_t fsz, const uint8_t* slab, int64_t slab_bytes,
                         const uint8_t** frame_table,
                         const float** reward_table) {
  if (b < 1 || fsz < 1) {
    throw std::invalid_argument("row table: empty batch or frame");
  }
  if (slab == nullptr || slab_bytes < 1) {
    throw std::invalid_argument("row table: no slab");
  }
  const uintptr_t lo = reinterpret_cast<uintptr_t>(slab);
  const uintptr_t hi = lo + (uintptr_t)slab_bytes;
  // p >= lo first, so hi - p cannot wrap.
  auto inside = [lo, hi](uintptr_t p, uint64_t n) {
    return p >= lo && p <= hi && (uint64_t)(hi - p) >= n;
  };
  uint64_t bits = (uint64_t)fsz;
  for (int64_t r = 0; r < b; ++r) {
    const auto f = reinterpret_cast<uintptr_t>(frame_of(r));
    const auto w = reinterpret_cast<uintptr_t>(reward_of(r));
    if (!inside(f, (uint64_t)fsz) || !inside(w, 4)) {
      throw std::out_of_range("row table: row " + std::to_string(r) +
                              " leaves the rollout slab");
    }
    if ((w & 3u) != 0) {
      throw std::invalid_argument("row table: reward of row " +
                                  std::to_string(r) + " is not 4-byte aligned");
    }
    bits |= (uint64_t)f;
    frame_table[r] = reinterpret_cast<const uint8_t*>(f);
    reward_table[r] = reinterpret_cast<const float*>(w);
  }
  return row_access_width(bits);
}

}  // namespace tbruntime
