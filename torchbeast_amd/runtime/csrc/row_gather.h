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
// The recurrent row form adds a second table of the same kind, for the
// agent state: build_state_table() below.
//
// Everything in this header is host code and needs neither torch nor HIP.

#pragma once

#include <algorithm>
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

// The table the LSTM serve kernels (lstm_stage_state_kernel and
// lstm_serve_layer_kernel, runtime_kernels.hip) read: per request
// the address its recurrent state is read from, the address the new state is
// written to (`n_floats` = 2 * L * H floats each: h [L, H], then c [L, H])
// and the address of its row's done byte.
//
// state_in_of(r) / state_out_of(r) must be 4-byte aligned ranges inside the
// state block [state, state + state_bytes), done_of(r) one byte inside the
// rollout slab [slab, slab + slab_bytes). No two of the 2 * b state ranges
// may overlap: two requests of one stream would read or write the same
// half, and a state written where another request's (or the next step's)
// state is read breaks the rule that an answer goes to the half nobody
// reads. (The kernels themselves are ordered by their stream: the stage
// kernel has read every in range before a layer kernel writes an out range.
// The check guards the two-halves invariant, not a race between
// workgroups.) Everything is checked before anything
// is stored; the exceptions are build_row_table()'s (std::out_of_range for a
// range that leaves its region, std::invalid_argument for the rest).
// `scratch` (grown as needed, reusable across calls) holds the sorted range
// starts.
template <typename InOf, typename OutOf, typename DoneOf, typename Scratch>
void build_state_table(int64_t b, InOf state_in_of, OutOf state_out_of,
                       DoneOf done_of, int64_t n_floats, const void* state,
                       int64_t state_bytes, const uint8_t* slab,
                       int64_t slab_bytes, Scratch& scratch,
                       const float** in_table, float** out_table,
                       const uint8_t** done_table) {
  if (b < 1 || n_floats < 1) {
    throw std::invalid_argument("state table: empty batch or state");
  }
  if (state == nullptr || state_bytes < 1) {
    throw std::invalid_argument("state table: no state block");
  }
  if (slab == nullptr || slab_bytes < 1) {
    throw std::invalid_argument("state table: no slab");
  }
  const uint64_t n_bytes = (uint64_t)n_floats * 4u;
  const uintptr_t s_lo = reinterpret_cast<uintptr_t>(state);
  const uintptr_t s_hi = s_lo + (uintptr_t)state_bytes;
  const uintptr_t d_lo = reinterpret_cast<uintptr_t>(slab);
  const uintptr_t d_hi = d_lo + (uintptr_t)slab_bytes;
  // p >= lo first, so hi - p cannot wrap.
  auto inside = [](uintptr_t p, uint64_t n, uintptr_t lo, uintptr_t hi) {
    return p >= lo && p <= hi && (uint64_t)(hi - p) >= n;
  };
  scratch.clear();
  for (int64_t r = 0; r < b; ++r) {
    const auto i = reinterpret_cast<uintptr_t>(state_in_of(r));
    const auto o = reinterpret_cast<uintptr_t>(state_out_of(r));
    const auto d = reinterpret_cast<uintptr_t>(done_of(r));
    if (!inside(i, n_bytes, s_lo, s_hi) || !inside(o, n_bytes, s_lo, s_hi)) {
      throw std::out_of_range("state table: state of row " +
                              std::to_string(r) + " leaves the state block");
    }
    if (!inside(d, 1, d_lo, d_hi)) {
      throw std::out_of_range("state table: done byte of row " +
                              std::to_string(r) + " leaves the rollout slab");
    }
    if (((i | o) & 3u) != 0) {
      throw std::invalid_argument("state table: state of row " +
                                  std::to_string(r) +
                                  " is not 4-byte aligned");
    }
    scratch.push_back(i);
    scratch.push_back(o);
  }
  // All ranges have one length: two of them overlap exactly when two
  // neighbouring starts of the sorted list are closer than that.
  std::sort(scratch.begin(), scratch.end());
  for (size_t k = 1; k < scratch.size(); ++k) {
    if ((uint64_t)(scratch[k] - scratch[k - 1]) < n_bytes) {
      throw std::invalid_argument(
          "state table: two state ranges overlap (one stream twice in a "
          "batch, or a state written where another is read)");
    }
  }
  for (int64_t r = 0; r < b; ++r) {
    in_table[r] = reinterpret_cast<const float*>(state_in_of(r));
    out_table[r] = reinterpret_cast<float*>(
        reinterpret_cast<uintptr_t>(state_out_of(r)));
    done_table[r] = reinterpret_cast<const uint8_t*>(done_of(r));
  }
}

}  // namespace tbruntime
