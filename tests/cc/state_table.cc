// Stand-alone check of build_state_table() (row_gather.h), the only writer of
// the pointer table that lstm_serve_layer_kernel reads. Host code only: needs
// neither torch nor HIP. Build and run notes: README_state_table.md.

#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

#include "row_gather.h"

using namespace tbruntime;

#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__,     \
                   __LINE__, #cond);                                  \
      std::exit(1);                                                   \
    }                                                                 \
  } while (0)

namespace {

struct Batch {
  std::vector<int64_t> in_off, out_off, done_off;
};

struct Regions {
  const uint8_t* state;
  int64_t state_bytes;
  const uint8_t* slab;
  int64_t slab_bytes;
};

std::vector<const float*> in_tab;
std::vector<float*> out_tab;
std::vector<const uint8_t*> done_tab;
std::vector<uintptr_t> scratch;

// Runs the builder over offsets into the two regions; returns 1, or 0 when
// it threw out_of_range and -1 when it threw invalid_argument. The tables
// are filled with a sentinel first: a refused batch must leave them alone.
float sentinel_f;
uint8_t sentinel_b;

int build(const Regions& g, const Batch& batch, int64_t n_floats) {
  const int64_t b = (int64_t)batch.in_off.size();
  const size_t n = (size_t)(b > 0 ? b : 1);
  in_tab.assign(n, &sentinel_f);
  out_tab.assign(n, &sentinel_f);
  done_tab.assign(n, &sentinel_b);
  // Addresses are formed as integers: a case may name a range outside its
  // region, and such a pointer must never exist as a pointer into storage.
  const auto sbase = reinterpret_cast<uintptr_t>(g.state);
  const auto dbase = reinterpret_cast<uintptr_t>(g.slab);
  int result;
  try {
    build_state_table(
        b,
        [&](int64_t r) {
          return reinterpret_cast<const uint8_t*>(
              sbase + (uintptr_t)batch.in_off[r]);
        },
        [&](int64_t r) {
          return reinterpret_cast<const uint8_t*>(
              sbase + (uintptr_t)batch.out_off[r]);
        },
        [&](int64_t r) {
          return reinterpret_cast<const uint8_t*>(
              dbase + (uintptr_t)batch.done_off[r]);
        },
        n_floats, g.state, g.state_bytes, g.slab, g.slab_bytes, scratch,
        in_tab.data(), out_tab.data(), done_tab.data());
    return 1;
  } catch (const std::out_of_range&) {
    result = 0;
  } catch (const std::invalid_argument&) {
    result = -1;
  }
  for (size_t r = 0; r < n; ++r) {
    CHECK(in_tab[r] == &sentinel_f && out_tab[r] == &sentinel_f &&
          done_tab[r] == &sentinel_b);
  }
  return result;
}

}  // namespace

int main() {
  // Both regions sit in the middle of larger allocations, so ranges before
  // and after them are still addresses this program owns.
  const int64_t kState = 8192, kSlab = 1024, kGuard = 512;
  std::vector<uint8_t> state_storage(kState + 2 * kGuard + 16);
  std::vector<uint8_t> slab_storage(kSlab + 2 * kGuard);
  auto p = reinterpret_cast<uintptr_t>(state_storage.data()) + kGuard;
  p = (p + 15) & ~uintptr_t(15);
  Regions g{reinterpret_cast<const uint8_t*>(p), kState,
            slab_storage.data() + kGuard, kSlab};
  const int64_t kFloats = 2 * 2 * 13;  // (h, c) x L = 2 x H = 13
  const int64_t N = 4 * kFloats;       // 208 bytes per half

  // What is stored: in, out and done addresses as given, through which the
  // memory can really be read and written.
  {
    Batch batch{{0, 6 * N, 2 * N + 4}, {N, 7 * N, 3 * N + 4}, {7, 0, kSlab - 1}};
    CHECK(build(g, batch, kFloats) == 1);
    for (int r = 0; r < 3; ++r) {
      CHECK(reinterpret_cast<const uint8_t*>(in_tab[r]) ==
            g.state + batch.in_off[r]);
      CHECK(reinterpret_cast<const uint8_t*>(out_tab[r]) ==
            g.state + batch.out_off[r]);
      CHECK(done_tab[r] == g.slab + batch.done_off[r]);
      float sum = 0.f;
      for (int64_t k = 0; k < kFloats; ++k) {
        out_tab[r][k] = (float)k;
        sum += in_tab[r][k];
      }
      CHECK(sum == 0.f && *done_tab[r] == 0);
    }
  }
  // A range ending exactly at the block's end is inside (in and out); one
  // float more, or one byte more, is not.
  {
    Batch batch{{0}, {kState - N}, {0}};
    CHECK(build(g, batch, kFloats) == 1);
    Batch swapped{{kState - N}, {0}, {0}};
    CHECK(build(g, swapped, kFloats) == 1);
    batch.out_off[0] = kState - N + 4;
    CHECK(build(g, batch, kFloats) == 0);
    batch.out_off[0] = kState - N + 1;
    CHECK(build(g, batch, kFloats) == 0);
    swapped.in_off[0] = kState - N + 4;
    CHECK(build(g, swapped, kFloats) == 0);
  }
  // Ranges beginning before the block; a state larger than the block.
  {
    Batch in_before{{-4}, {N}, {0}};
    CHECK(build(g, in_before, kFloats) == 0);
    Batch out_before{{0}, {-N}, {0}};
    CHECK(build(g, out_before, kFloats) == 0);
    Batch second{{0, -16}, {N, 2 * N}, {0, 1}};
    CHECK(build(g, second, kFloats) == 0);
    Batch big{{0}, {0}, {0}};
    CHECK(build(g, big, kState / 4 + 1) == 0);
  }
  // The done byte: the slab's last byte is inside, the next one and the one
  // before the slab are not.
  {
    Batch batch{{0}, {N}, {kSlab - 1}};
    CHECK(build(g, batch, kFloats) == 1);
    batch.done_off[0] = kSlab;
    CHECK(build(g, batch, kFloats) == 0);
    batch.done_off[0] = -1;
    CHECK(build(g, batch, kFloats) == 0);
  }
  // Misaligned state addresses; empty inputs; missing regions.
  {
    Batch mis_in{{2}, {N}, {0}};
    CHECK(build(g, mis_in, kFloats) == -1);
    Batch mis_out{{0}, {N + 1}, {0}};
    CHECK(build(g, mis_out, kFloats) == -1);
    Batch none;
    CHECK(build(g, none, kFloats) == -1);
    Batch one{{0}, {N}, {0}};
    CHECK(build(g, one, 0) == -1);
    Regions no_state{nullptr, kState, g.slab, kSlab};
    CHECK(build(no_state, one, kFloats) == -1);
    Regions no_slab{g.state, kState, nullptr, kSlab};
    CHECK(build(no_slab, one, kFloats) == -1);
  }
  // Overlaps: one stream twice (same in, same out, or both), an in range
  // that is another request's (or its own) out range, partial overlaps by
  // one float either way round. Back to back is fine.
  {
    Batch twice{{0, 0}, {N, N}, {0, 1}};
    CHECK(build(g, twice, kFloats) == -1);
    Batch same_in{{0, 0}, {N, 2 * N}, {0, 1}};
    CHECK(build(g, same_in, kFloats) == -1);
    Batch same_out{{0, 2 * N}, {N, N}, {0, 1}};
    CHECK(build(g, same_out, kFloats) == -1);
    Batch chained{{0, N}, {N, 2 * N}, {0, 1}};
    CHECK(build(g, chained, kFloats) == -1);
    Batch self{{0}, {0}, {0}};
    CHECK(build(g, self, kFloats) == -1);
    Batch partial{{0}, {N - 4}, {0}};
    CHECK(build(g, partial, kFloats) == -1);
    Batch partial_rev{{N - 4}, {0}, {0}};
    CHECK(build(g, partial_rev, kFloats) == -1);
    Batch far{{0, 3 * N - 4}, {N, 2 * N}, {0, 1}};
    CHECK(build(g, far, kFloats) == -1);
    Batch back_to_back{{0, 2 * N}, {N, 3 * N}, {0, 1}};
    CHECK(build(g, back_to_back, kFloats) == 1);
  }
  // A full-sized batch in shuffled order: 19 streams, halves alternating.
  {
    Batch batch;
    for (int k = 0; k < 19; ++k) {
      const int s = (k * 7) % 19, half = k & 1;
      batch.in_off.push_back((2 * s + half) * N);
      batch.out_off.push_back((2 * s + (half ^ 1)) * N);
      batch.done_off.push_back(k);
    }
    CHECK(build(g, batch, kFloats) == 1);
    batch.in_off[18] = batch.out_off[3];
    CHECK(build(g, batch, kFloats) == -1);
  }
  std::printf("state_table ok\nALL OK\n");
  return 0;
}
