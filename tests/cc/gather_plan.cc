// Stand-alone check of the learner queue's gather planner and of the host
// reference unpack (rollout_gather.h) over a real PinnedSlabPool.
//
// CPU only (TBAMD_NO_PIN is set before anything asks for pinned memory);
// built like stress_actor_rows.cc, plain and with
// -fsanitize=address,undefined. See README_gather_plan.md.
//
// Every case builds B = 3 rollouts of 5 rows (a 1x8x16 u8 frame plus the
// seven small leaves) in pool slots, plans, "DMAs" each slot window into a
// host staging row with memcpy, runs the host unpack into the arena outputs
// and compares byte for byte with torch::cat along batch_dim.

#include <torch/torch.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#if __has_include("queues_hip.h")
#include "queues_hip.h"
#else
#include "queues.h"
#endif

using namespace tbruntime;

static int failures = 0;
#define EXPECT(cond)                                             \
  do {                                                           \
    if (!(cond)) {                                               \
      std::fprintf(stderr, "EXPECT failed: %s (%s:%d)\n", #cond, \
                   __FILE__, __LINE__);                          \
      ++failures;                                                \
    }                                                            \
  } while (0)

constexpr int64_t kB = 3;
constexpr int64_t kRows = 5;

struct LeafSpec {
  std::vector<int64_t> step;  // one step's shape after [rows, 1]
  torch::ScalarType dtype;
};

static std::vector<LeafSpec> rollout_leaves() {
  return {
      {{1, 8, 16}, torch::kUInt8},  // frame, 128-byte rows
      {{}, torch::kFloat32},        // reward
      {{}, torch::kBool},           // done
      {{}, torch::kInt32},          // episode_step
      {{}, torch::kFloat32},        // episode_return
      {{}, torch::kInt64},          // action
      {{6}, torch::kFloat32},       // policy_logits, 24-byte rows
      {{}, torch::kFloat32},        // baseline
  };
}

static std::vector<int64_t> leaf_shape(const LeafSpec& l, int64_t batch_dim) {
  std::vector<int64_t> shape =
      batch_dim == 1 ? std::vector<int64_t>{kRows, 1}
                     : std::vector<int64_t>{1, kRows};
  shape.insert(shape.end(), l.step.begin(), l.step.end());
  return shape;
}

static uint32_t rng_state = 12345;
static void fill_random(const torch::Tensor& t) {
  auto* p = static_cast<uint8_t*>(t.data_ptr());
  const int64_t n = t.numel() * (int64_t)t.element_size();
  for (int64_t i = 0; i < n; ++i) {
    rng_state = rng_state * 1664525u + 1013904223u;
    p[i] = (uint8_t)(rng_state >> 24);
  }
  if (t.scalar_type() == torch::kBool) {
    for (int64_t i = 0; i < n; ++i) p[i] &= 1;
  }
}

// Carve `specs` out of a fresh slot; pad_before >= 0 carves 256 bytes in
// front of that leaf, so it lies at another offset than in a plain slot.
static std::vector<torch::Tensor> carve_item(
    PinnedSlabPool& pool, const std::vector<LeafSpec>& specs,
    int64_t batch_dim, int pad_before = -1) {
  auto slot = pool.acquire(8192, nullptr);
  std::vector<torch::Tensor> leaves;
  for (size_t i = 0; i < specs.size(); ++i) {
    if ((int)i == pad_before) slot.carve({256}, torch::kUInt8);
    leaves.push_back(slot.carve(leaf_shape(specs[i], batch_dim),
                                specs[i].dtype));
    fill_random(leaves.back());
  }
  return leaves;
}

static void release_all(PinnedSlabPool& pool,
                        const std::vector<std::vector<torch::Tensor>>& flats) {
  std::vector<const void*> ptrs;
  for (const auto& f : flats) {
    for (const auto& t : f) ptrs.push_back(t.data_ptr());
  }
  for (int pass = 0; pass < 2; ++pass) {
    // The second call must find nothing left to release.
    pool.mark_consumed_many(ptrs, nullptr);
    auto st = pool.stats();
    EXPECT(st["slab_free"] + st["slab_pending"] + st["slab_held"] ==
           st["slab_slots"]);
    EXPECT(st["slab_held"] == 0);
    EXPECT(st["slab_free"] == st["slab_slots"]);
  }
}

// Byte equality (the random fill makes NaNs, which torch::equal rejects).
static bool same_bytes(const torch::Tensor& a, const torch::Tensor& b) {
  return a.scalar_type() == b.scalar_type() && a.sizes() == b.sizes() &&
         a.is_contiguous() && b.is_contiguous() &&
         std::memcmp(a.data_ptr(), b.data_ptr(),
                     a.numel() * a.element_size()) == 0;
}

// Plan, copy, unpack, compare. `want` is the expected gathered mask (empty:
// the plan must be empty).
static void check(const std::vector<std::vector<torch::Tensor>>& flats,
                  int64_t batch_dim, const SlabGeometry& geom,
                  const std::vector<char>& want) {
  const GatherPlan plan = plan_gather(flats, batch_dim, geom);
  if (want.empty()) {
    EXPECT(plan.empty());
    return;
  }
  EXPECT(!plan.empty());
  EXPECT(plan.gathered == want);
  if (plan.empty() || plan.gathered != want) return;
  EXPECT(plan.B == (int64_t)flats.size());
  EXPECT(plan.stride() % 256 == 0 && plan.stride() >= plan.win_bytes);

  // The window is the hull of the slab columns, and starts in item b's slot.
  int64_t lo = INT64_MAX, hi = 0;
  for (const auto& c : plan.columns) {
    lo = std::min(lo, c.slot_off);
    hi = std::max(hi, c.slot_off + c.item_bytes());
    EXPECT(c.src_off == c.slot_off - plan.win_off);
    for (size_t b = 0; b < flats.size(); ++b) {
      EXPECT(plan.window_start[b] + c.src_off ==
             static_cast<const uint8_t*>(flats[b][c.leaf].data_ptr()));
    }
  }
  EXPECT(plan.win_off == lo && plan.win_bytes == hi - lo);

  const int64_t stride = plan.stride();
  std::vector<uint8_t> staging(plan.staging_bytes(), 0xCD);
  for (int64_t b = 0; b < plan.B; ++b) {
    std::memcpy(staging.data() + b * stride, plan.window_start[b],
                plan.win_bytes);
  }
  GatherOutputs out = make_gather_outputs(plan, torch::kCPU);
  unpack_rollouts_host(staging.data(), stride, plan.B, out.columns.data(),
                       (int)out.columns.size());
  std::vector<torch::Tensor> column(flats.size());
  for (size_t c = 0; c < plan.columns.size(); ++c) {
    for (size_t b = 0; b < flats.size(); ++b) {
      column[b] = flats[b][plan.columns[c].leaf];
    }
    const torch::Tensor ref = torch::cat(column, batch_dim);
    const torch::Tensor& got = out.leaves[c];
    EXPECT(got.is_contiguous());
    EXPECT(got.scalar_type() == ref.scalar_type());
    EXPECT(got.sizes() == ref.sizes());
    EXPECT((static_cast<const uint8_t*>(got.data_ptr()) -
            static_cast<const uint8_t*>(out.arena.data_ptr())) % 256 == 0);
    EXPECT(same_bytes(got, ref));
  }
}

int main() {
  setenv("TBAMD_NO_PIN", "1", 1);
  auto pool = std::make_shared<PinnedSlabPool>(/*budget_bytes=*/0,
                                               /*min_slots=*/8);
  const auto specs = rollout_leaves();
  const std::vector<char> all(8, 1);

  // No slab yet: nothing to gather from.
  {
    std::vector<std::vector<torch::Tensor>> flats(1);
    flats[0].push_back(torch::zeros({kRows, 1}));
    EXPECT(plan_gather(flats, 1, pool->geometry()).empty());
  }

  for (int64_t batch_dim : {1, 0}) {
    std::vector<std::vector<torch::Tensor>> flats;
    for (int64_t b = 0; b < kB; ++b) {
      flats.push_back(carve_item(*pool, specs, batch_dim));
    }
    const SlabGeometry geom = pool->geometry();
    EXPECT(geom.base != nullptr && geom.slot_bytes == 8192);
    check(flats, batch_dim, geom, all);
    if (batch_dim == 1) {
      // The row sizes the unpack kernel has paths for.
      const GatherPlan plan = plan_gather(flats, 1, geom);
      const int64_t inner[] = {128, 4, 1, 4, 4, 8, 24, 4};
      for (size_t c = 0; c < plan.columns.size() && c < 8; ++c) {
        EXPECT(plan.columns[c].outer == kRows);
        EXPECT(plan.columns[c].inner_bytes == inner[c]);
      }
    }
    // Items in another order than their slots.
    std::swap(flats[0], flats[2]);
    check(flats, batch_dim, geom, all);
    release_all(*pool, flats);
  }

  {  // One leaf outside the slab: it falls back, the others are gathered.
    std::vector<std::vector<torch::Tensor>> flats;
    for (int64_t b = 0; b < kB; ++b) {
      flats.push_back(carve_item(*pool, specs, 1));
      flats.back().push_back(torch::randn({2, 1, 4}));
    }
    std::vector<char> want = all;
    want.push_back(0);
    check(flats, 1, pool->geometry(), want);
    // Outside the slab in one item only.
    std::vector<std::vector<torch::Tensor>> one = flats;
    for (auto& f : one) f.pop_back();
    one[1][4] = one[1][4].clone();
    want = all;
    want[4] = 0;
    check(one, 1, pool->geometry(), want);
    release_all(*pool, flats);
  }

  {  // Offsets differ between items: that column falls back.
    std::vector<std::vector<torch::Tensor>> flats;
    for (int64_t b = 0; b < kB; ++b) {
      flats.push_back(carve_item(*pool, specs, 1, b == 2 ? 7 : -1));
    }
    std::vector<char> want = all;
    want[7] = 0;
    check(flats, 1, pool->geometry(), want);
    release_all(*pool, flats);
  }

  {  // Shape, dtype or batch size disagree: those columns fall back.
    std::vector<LeafSpec> wide = specs;
    std::vector<std::vector<torch::Tensor>> flats;
    for (int64_t b = 0; b < kB; ++b) {
      flats.push_back(carve_item(*pool, wide, 1));
    }
    flats[1][1] = flats[1][1].view(torch::kInt32);          // dtype
    flats[2][6] = flats[2][6].view({kRows, 1, 2, 3});       // shape
    flats[0][5] = flats[0][5].view(torch::kInt32).view({kRows, 2});
    for (int64_t b = 1; b < kB; ++b) {                      // size(1) == 2
      flats[b][5] = flats[b][5].view(torch::kInt32).view({kRows, 2});
    }
    flats[0][3] = flats[0][3].view({kRows});                // no batch dim
    std::vector<char> want = all;
    want[1] = want[6] = want[5] = want[3] = 0;
    // Leaves 5 and 3 cannot be cat-ed with their column any more; only the
    // classification is checked.
    const GatherPlan plan = plan_gather(flats, 1, pool->geometry());
    EXPECT(plan.gathered == want);
    release_all(*pool, flats);
  }

  {  // One item's leaves in two slots: the whole batch falls back.
    std::vector<std::vector<torch::Tensor>> flats;
    for (int64_t b = 0; b < kB; ++b) {
      flats.push_back(carve_item(*pool, specs, 1));
    }
    std::vector<torch::Tensor> other = carve_item(*pool, specs, 1);
    flats[1][3] = other[3];  // same offset, another slot
    check(flats, 1, pool->geometry(), {});
    flats.push_back(other);  // for the release only
    release_all(*pool, flats);
  }

  {  // More than 16 slab columns: the whole batch falls back; 16 are fine.
    std::vector<LeafSpec> many(17, LeafSpec{{}, torch::kFloat32});
    std::vector<std::vector<torch::Tensor>> flats;
    for (int64_t b = 0; b < kB; ++b) {
      flats.push_back(carve_item(*pool, many, 1));
    }
    check(flats, 1, pool->geometry(), {});
    for (auto& f : flats) f.pop_back();
    check(flats, 1, pool->geometry(), std::vector<char>(16, 1));
    release_all(*pool, flats);
  }

  {  // A CPU queue over the pool: unchanged, nothing is gathered.
    BatchingQueue queue(/*batch_dim=*/1, /*min=*/kB, /*max=*/kB);
    queue.set_source_pool(pool);
    std::vector<std::vector<torch::Tensor>> flats;
    for (int64_t b = 0; b < kB; ++b) {
      flats.push_back(carve_item(*pool, specs, 1));
      TensorNest::vector_t leaves(flats.back().begin(), flats.back().end());
      queue.enqueue(TensorNest(std::move(leaves)));
    }
    auto [batch, n] = queue.dequeue_many();
    EXPECT(n == kB);
    std::vector<torch::Tensor> got = batch.flatten();
    EXPECT(got.size() == 8);
    std::vector<torch::Tensor> column(kB);
    for (size_t i = 0; i < got.size() && i < 8; ++i) {
      for (int64_t b = 0; b < kB; ++b) column[b] = flats[b][i];
      EXPECT(same_bytes(got[i], torch::cat(column, 1)));
    }
    auto st = queue.stats();
    EXPECT(st["dequeues"] == 1);
    EXPECT(st["gather_dequeues"] == 0 && st["gather_columns"] == 0);
    EXPECT(st["slab_free"] + st["slab_pending"] + st["slab_held"] ==
           st["slab_slots"]);
    EXPECT(st["slab_held"] == 0);
  }

  if (failures != 0) {
    std::fprintf(stderr, "%d FAILURES\n", failures);
    return 1;
  }
  std::printf("gather_plan ok\nALL OK\n");
  return 0;
}
