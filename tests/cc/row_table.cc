// Stand-alone check of build_row_table() (row_gather.h), the only writer of
// the pointer table that gather_rows_kernel reads. Host code only: needs
// neither torch nor HIP. Build and run notes: README_row_table.md.

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
  std::vector<int64_t> frame_off, reward_off;
};

// Runs the builder over offsets into `slab`; returns the width, or 0 when
// it threw out_of_range and -1 when it threw invalid_argument.
int build(const uint8_t* slab,
          int64_t slab_bytes, const Batch& batch, int64_t fsz,
          std::vector<const uint8_t*>* ft, std::vector<const float*>* rt) {
  const int64_t b = (int64_t)batch.frame_off.size();
  ft->assign(b > 0 ? b : 1, nullptr);
  rt->assign(b > 0 ? b : 1, nullptr);
  // Addresses are formed as integers: a case may name a row outside the
  // slab, and such a pointer must never exist as a pointer into `storage`.
  const auto base = reinterpret_cast<uintptr_t>(slab);
  try {
    return (int)build_row_table(
        b,
        [&](int64_t r) {
          return reinterpret_cast<const uint8_t*>(
              base + (uintptr_t)batch.frame_off[r]);
        },
        [&](int64_t r) {
          return reinterpret_cast<const uint8_t*>(
              base + (uintptr_t)batch.reward_off[r]);
        },
        fsz, slab, slab_bytes, ft->data(), rt->data());
  } catch (const std::out_of_range&) {
    return 0;
  } catch (const std::invalid_argument&) {
    return -1;
  }
}

}  // namespace

int main() {
  // A 16-byte aligned "slab" in the middle of a larger allocation, so rows
  // before and after it are still addresses this program owns.
  const int64_t kSlab = 4096, kGuard = 256;
  std::vector<uint8_t> storage(kSlab + 2 * kGuard + 16);
  auto p = reinterpret_cast<uintptr_t>(storage.data()) + kGuard;
  p = (p + 15) & ~uintptr_t(15);
  const uint8_t* slab = reinterpret_cast<const uint8_t*>(p);
  std::vector<const uint8_t*> ft;
  std::vector<const float*> rt;

  // Pointers and width: offsets = 0, 4, 8, 1 (mod 16).
  const struct {
    int64_t shift;
    int64_t fsz;
    int width;
  } cases[] = {{0, 64, 16}, {4, 64, 4}, {8, 64, 8}, {1, 64, 1},
               {0, 100, 4},  {0, 63, 1}, {0, 72, 8}, {8, 72, 8}};
  for (const auto& c : cases) {
    Batch batch;
    for (int r = 0; r < 5; ++r) {
      batch.frame_off.push_back(128 * r + c.shift);
      batch.reward_off.push_back(2048 + 4 * r);
    }
    CHECK(build(slab, kSlab, batch, c.fsz, &ft, &rt) == c.width);
    for (int r = 0; r < 5; ++r) {
      CHECK(ft[r] == slab + 128 * r + c.shift);
      CHECK(reinterpret_cast<const uint8_t*>(rt[r]) == slab + 2048 + 4 * r);
    }
  }
  // One misaligned row narrows the whole batch.
  {
    Batch batch{{0, 128, 260}, {2048, 2052, 2056}};
    CHECK(build(slab, kSlab, batch, 64, &ft, &rt) == 4);
  }
  // A row ending exactly at the slab's end is inside; one byte more is not.
  {
    Batch batch{{kSlab - 64}, {kSlab - 4}};
    CHECK(build(slab, kSlab, batch, 64, &ft, &rt) == 16);
    batch.frame_off[0] = kSlab - 63;
    CHECK(build(slab, kSlab, batch, 64, &ft, &rt) == 0);
    batch.frame_off[0] = 0;
    batch.reward_off[0] = kSlab;  // 4-aligned, but past the end
    CHECK(build(slab, kSlab, batch, 64, &ft, &rt) == 0);
  }
  // A row beginning before the slab.
  {
    Batch batch{{0, -16}, {2048, 2052}};
    CHECK(build(slab, kSlab, batch, 64, &ft, &rt) == 0);
    Batch rew{{0, 64}, {2048, -4}};
    CHECK(build(slab, kSlab, rew, 64, &ft, &rt) == 0);
  }
  // A frame larger than the slab, a misaligned reward, empty inputs.
  {
    Batch batch{{0}, {0}};
    CHECK(build(slab, kSlab, batch, kSlab + 1, &ft, &rt) == 0);
    Batch mis{{0}, {2050}};
    CHECK(build(slab, kSlab, mis, 64, &ft, &rt) == -1);
    Batch none;
    CHECK(build(slab, kSlab, none, 64, &ft, &rt) == -1);
    CHECK(build(slab, kSlab, batch, 0, &ft, &rt) == -1);
    CHECK(build(nullptr, kSlab, batch, 64, &ft, &rt) == -1);
  }
  CHECK(row_access_width(0) == 16 && row_access_width(24) == 8 &&
        row_access_width(12) == 4 && row_access_width(2) == 1 &&
        row_access_width(7) == 1);
  std::printf("row_table ok\nALL OK\n");
  return 0;
}
