// Learner-batch assembly from whole rollout slots: the planner, the column
// descriptors shared with the unpack kernel, a host reference unpack and the
// hook through which BatchingQueue reaches the kernel.
//
// An actor fills one PinnedSlabPool slot per rollout; all columns of the
// rollout lie at the same slot-relative offsets in every slot. A batch of B
// rollouts therefore needs B contiguous host-to-device copies of one byte
// window per slot into a device staging buffer (row b = item b's window),
// plus one kernel that transposes the staged rows into the batched leaves.
//
// With outer = prod(shape[:batch_dim]) and inner_bytes =
// prod(shape[batch_dim+1:]) * elsize, item b's element (o, .) of a column
// lands at  dst + (o * B + b) * inner_bytes  -- batch_dim 0 and 1 alike.
//
// Everything in this header is host code and needs no GPU.

#pragma once

#include <torch/extension.h>

#include <atomic>
#include <cstdint>
#include <cstring>
#include <vector>

namespace tbruntime {

constexpr int kMaxGatherColumns = 16;
// Largest staging buffer (B * window, window rounded up to 256 bytes) the
// gather path will ask for; a bigger batch keeps the per-leaf copies.
// Full-resolution frames (3x210x160, unroll 80, B = 32) need ~260 MB.
constexpr int64_t kGatherStagingCapBytes = int64_t(1) << 30;

// One column as the unpack kernel sees it (passed by value in its
// arguments): read `outer` rows of `inner_bytes` from every staging row at
// `src_off`, write them B-interleaved to `dst`.
struct UnpackColumn {
  int64_t src_off;
  int64_t inner_bytes;
  int64_t outer;
  uint8_t* dst;
};

// Launches the unpack kernel on the CURRENT stream of the device that owns
// `staging`. Installed by the extension module (the stand-alone test
// programs include the queues without linking any kernel).
using UnpackHook = void (*)(const uint8_t* staging, int64_t stride, int64_t B,
                            const UnpackColumn* columns, int n_columns);

inline std::atomic<UnpackHook>& unpack_hook_slot() {
  static std::atomic<UnpackHook> hook{nullptr};
  return hook;
}
inline void set_unpack_hook(UnpackHook hook) { unpack_hook_slot().store(hook); }
inline UnpackHook unpack_hook() { return unpack_hook_slot().load(); }

// The same unpack on host memory, as a plain memcpy loop: the oracle of the
// kernel tests and of tests/cc/gather_plan.cc.
inline void unpack_rollouts_host(const uint8_t* staging, int64_t stride,
                                 int64_t B, const UnpackColumn* columns,
                                 int n_columns) {
  for (int c = 0; c < n_columns; ++c) {
    const UnpackColumn& col = columns[c];
    for (int64_t o = 0; o < col.outer; ++o) {
      for (int64_t b = 0; b < B; ++b) {
        std::memcpy(col.dst + (o * B + b) * col.inner_bytes,
                    staging + b * stride + col.src_off + o * col.inner_bytes,
                    col.inner_bytes);
      }
    }
  }
}

inline int64_t round_up_256(int64_t n) { return (n + 255) & ~int64_t(255); }

// Where a pool's slots lie (PinnedSlabPool::geometry()).
struct SlabGeometry {
  const uint8_t* base = nullptr;
  int64_t slot_bytes = 0;
  int64_t total_bytes = 0;

  bool contains(const void* ptr) const {
    const auto* p = static_cast<const uint8_t*>(ptr);
    return base != nullptr && p >= base && p < base + total_bytes;
  }
};

struct GatherColumn {
  size_t leaf;       // position among the flattened leaves of an item
  int64_t slot_off;  // of the column inside its slot
  int64_t src_off;   // of the column inside the window
  int64_t outer;
  int64_t inner_bytes;
  torch::ScalarType dtype;
  std::vector<int64_t> out_shape;  // the item's shape with B at batch_dim

  int64_t item_bytes() const { return outer * inner_bytes; }
};

struct GatherPlan {
  int64_t B = 0;
  int64_t win_off = 0;    // smallest slot offset over the slab columns
  int64_t win_bytes = 0;  // up to the largest end over the slab columns
  std::vector<const uint8_t*> window_start;  // per item: slot base + win_off
  std::vector<GatherColumn> columns;
  std::vector<char> gathered;  // per leaf position

  bool empty() const { return columns.empty(); }
  int64_t stride() const { return round_up_256(win_bytes); }
  int64_t staging_bytes() const { return B * stride(); }
};

// Classify the leaf positions of B dequeued items (flats[b] = item b's
// flattened leaves). A position is a slab column when, for every item, the
// leaf is a contiguous CPU tensor inside the slab with size(batch_dim) == 1
// and shape, dtype and slot-relative offset agree across items. All slab
// columns of an item must lie in one slot, there may be at most
// kMaxGatherColumns of them and the staging need must stay under the cap;
// otherwise the plan is empty and the whole batch keeps the per-leaf path.
// Positions that are no slab column keep that path one by one.
inline GatherPlan plan_gather(
    const std::vector<std::vector<torch::Tensor>>& flats, int64_t batch_dim,
    const SlabGeometry& geom) {
  GatherPlan plan;
  if (flats.empty() || geom.base == nullptr || geom.slot_bytes <= 0) {
    return plan;
  }
  const int64_t B = (int64_t)flats.size();
  const size_t n_leaves = flats[0].size();
  for (const auto& f : flats) {
    if (f.size() != n_leaves) return plan;  // apply_columns will complain
  }
  plan.B = B;
  plan.gathered.assign(n_leaves, 0);

  // Slot-relative offset of a leaf that lies wholly inside one slot; -1
  // otherwise.
  auto slot_offset = [&](const torch::Tensor& t, int64_t* slot) -> int64_t {
    if (!t.defined() || !t.device().is_cpu() || !t.is_contiguous()) return -1;
    if (t.dim() <= batch_dim || t.size(batch_dim) != 1) return -1;
    const int64_t nbytes = t.numel() * (int64_t)t.element_size();
    if (nbytes <= 0 || !geom.contains(t.data_ptr())) return -1;
    const int64_t pos = static_cast<const uint8_t*>(t.data_ptr()) - geom.base;
    const int64_t off = pos % geom.slot_bytes;
    if (off + nbytes > geom.slot_bytes) return -1;
    *slot = pos / geom.slot_bytes;
    return off;
  };

  std::vector<int64_t> item_slot(B, -1);
  for (size_t i = 0; i < n_leaves; ++i) {
    const torch::Tensor& first = flats[0][i];
    int64_t slot = -1;
    const int64_t off = slot_offset(first, &slot);
    if (off < 0) continue;
    bool ok = true;
    std::vector<int64_t> slots(B);
    slots[0] = slot;
    for (int64_t b = 1; b < B && ok; ++b) {
      const torch::Tensor& t = flats[b][i];
      ok = slot_offset(t, &slots[b]) == off &&
           t.scalar_type() == first.scalar_type() &&
           t.sizes() == first.sizes();
    }
    if (!ok) continue;
    for (int64_t b = 0; b < B; ++b) {
      if (item_slot[b] < 0) item_slot[b] = slots[b];
      // One item spread over two slots: not a rollout an actor filled.
      if (item_slot[b] != slots[b]) return GatherPlan();
    }
    GatherColumn col;
    col.leaf = i;
    col.slot_off = off;
    col.src_off = 0;
    col.outer = 1;
    for (int64_t d = 0; d < batch_dim; ++d) col.outer *= first.size(d);
    col.inner_bytes = (int64_t)first.element_size();
    for (int64_t d = batch_dim + 1; d < first.dim(); ++d) {
      col.inner_bytes *= first.size(d);
    }
    col.dtype = first.scalar_type();
    col.out_shape = first.sizes().vec();
    col.out_shape[batch_dim] = B;
    // The kernel indexes rows (outer * B of them) with 32 bits.
    if (col.outer * B >= (int64_t(1) << 31)) continue;
    plan.columns.push_back(std::move(col));
  }
  if (plan.columns.empty() ||
      plan.columns.size() > (size_t)kMaxGatherColumns) {
    return GatherPlan();
  }
  int64_t lo = plan.columns[0].slot_off, hi = 0;
  for (const auto& c : plan.columns) {
    lo = std::min(lo, c.slot_off);
    hi = std::max(hi, c.slot_off + c.item_bytes());
  }
  plan.win_off = lo;
  plan.win_bytes = hi - lo;
  if (plan.staging_bytes() > kGatherStagingCapBytes) return GatherPlan();
  for (auto& c : plan.columns) {
    c.src_off = c.slot_off - lo;
    plan.gathered[c.leaf] = 1;
  }
  plan.window_start.resize(B);
  for (int64_t b = 0; b < B; ++b) {
    plan.window_start[b] = geom.base + item_slot[b] * geom.slot_bytes + lo;
  }
  return plan;
}

// The gathered outputs of one batch: ONE allocation (an arena of 256-byte
// aligned sub-tensors, each viewed to its leaf's dtype and shape) and the
// kernel's column descriptors pointing into it.
// Lifetime: every leaf is a view of the arena, so a consumer that keeps any
// one leaf alive (even a [T+1, B] reward) keeps the whole batch's block,
// frames included (~73 MB at the headline shape), out of the caching
// allocator. Clone a small leaf that has to outlive its batch.
struct GatherOutputs {
  torch::Tensor arena;
  std::vector<torch::Tensor> leaves;    // one per plan column
  std::vector<UnpackColumn> columns;
};

inline GatherOutputs make_gather_outputs(const GatherPlan& plan,
                                         torch::Device device) {
  GatherOutputs out;
  int64_t total = 0;
  for (const auto& c : plan.columns) {
    total += round_up_256(c.item_bytes() * plan.B);
  }
  out.arena = torch::empty(
      {total}, torch::TensorOptions().dtype(torch::kUInt8).device(device));
  auto* base = static_cast<uint8_t*>(out.arena.data_ptr());
  int64_t off = 0;
  for (const auto& c : plan.columns) {
    const int64_t nbytes = c.item_bytes() * plan.B;
    out.leaves.push_back(
        out.arena.narrow(0, off, nbytes).view(c.dtype).view(c.out_shape));
    out.columns.push_back(
        UnpackColumn{c.src_off, c.inner_bytes, c.outer, base + off});
    off += round_up_256(nbytes);
  }
  return out;
}

}  // namespace tbruntime
