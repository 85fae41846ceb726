// Batching queues for the actor-learner runtime.
//
// Capability parity with the reference's BatchingQueue / DynamicBatcher
// (ref: src/cc/actorpool.cc:72-340), redesigned for MI355X:
// - dequeue/batch assembly concatenates into HIP-*pinned* host tensors
//   (cat_out into a pinned destination) so the learner/inference H2D copy
//   is a true DMA on a side stream, instead of pageable torch::cat output.
// - one generic bounded MPMC queue underlies both the learner rollout queue
//   and the inference request queue.
// - DynamicBatcher requests come in two forms: a tensor nest plus a promise
//   (compute()/compute_async(), the Python surface), or a ROW of a rollout
//   slot that an actor stream fills in place (RowLayout / ActorMailbox
//   below). Batch::get_inputs()/set_outputs() work on both; the C++ runner
//   reads and writes rows directly and finishes with complete_rows().
// - PinnedSlabPool slots have explicit FREE/ACQUIRED/PENDING states and a
//   dequeue releases all its slots in one critical section.
// - per-stage CPU-time counters of the actor and serve threads are folded
//   into BatchingQueue::stats() / DynamicBatcher::stats().
// - a GPU-output BatchingQueue fed from a PinnedSlabPool assembles a batch
//   with one DMA per rollout slot plus one unpack kernel (rollout_gather.h)
//   instead of one strided copy per rollout and leaf.

#pragma once

#include <ATen/cuda/CUDAContext.h>
#include <ATen/cuda/CUDAEvent.h>
#include <hip/hip_runtime_api.h>
#include <torch/extension.h>

#include <time.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <future>
#include <map>
#include <memory>
#include <mutex>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "nest.h"
#include "rollout_gather.h"

namespace tbruntime {

using TensorNest = Nest<torch::Tensor>;

inline int64_t now_us() {
  return std::chrono::duration_cast<std::chrono::microseconds>(
             std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

// TBAMD_ACTOR_FASTPATH=0 (A/B runs only) keeps actors on the nest/promise
// loops and the runner on the tensor serve code; anything else leaves the
// row fast path on.
inline bool actor_fastpath_enabled() {
  const char* v = std::getenv("TBAMD_ACTOR_FASTPATH");
  return !(v != nullptr && std::string(v) == "0");
}

// Lightweight perf counters (atomics; read via .stats() from Python).
struct StageStats {
  std::atomic<int64_t> n{0};
  std::atomic<int64_t> sum_us{0};
  void add(int64_t us) {
    n.fetch_add(1, std::memory_order_relaxed);
    sum_us.fetch_add(us, std::memory_order_relaxed);
  }
  void reset() {
    n.store(0, std::memory_order_relaxed);
    sum_us.store(0, std::memory_order_relaxed);
  }
};

// CPU time this thread has consumed so far (not wall time: a blocked thread
// does not advance it, a spinning one does).
inline int64_t thread_cpu_ns() {
  timespec ts;
  clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts);
  return (int64_t)ts.tv_sec * 1000000000LL + ts.tv_nsec;
}

// Per-stage CPU-time totals of a group of threads (the actor threads or the
// serve threads). Threads sample thread_cpu_ns() at stage boundaries once
// per sweep / per batch -- never per request -- and add the differences
// here. `items` counts env steps (actors) or requests served (serve).
struct CpuStageCounters {
  static constexpr int kStages = 5;
  std::atomic<int64_t> ns[kStages];
  std::atomic<int64_t> rounds{0};  // sweeps or batches
  std::atomic<int64_t> items{0};
  CpuStageCounters() { reset(); }
  void reset() {
    for (auto& v : ns) v.store(0, std::memory_order_relaxed);
    rounds.store(0, std::memory_order_relaxed);
    items.store(0, std::memory_order_relaxed);
  }
  void add(int stage, int64_t d) {
    ns[stage].fetch_add(d, std::memory_order_relaxed);
  }
  void report(const char* prefix, const char* const* names,
              const char* rounds_name, const char* items_name,
              std::map<std::string, double>* out) const {
    if (rounds.load() == 0) return;
    for (int i = 0; i < kStages; ++i) {
      (*out)[std::string(prefix) + "_cpu_us_" + names[i]] =
          ns[i].load() / 1e3;
    }
    (*out)[std::string(prefix) + "_" + rounds_name] = (double)rounds.load();
    (*out)[std::string(prefix) + "_" + items_name] = (double)items.load();
  }
};

enum ActorStage { kActorEnvStep, kActorIssue, kActorWait, kActorCollect,
                  kActorFlush };
enum ServeStage { kServeBatchWait, kServeGather, kServeEnqueue,
                  kServeSyncWait, kServeFanout };
inline const char* const* actor_stage_names() {
  static const char* const n[] = {"env_step", "issue", "wait", "collect",
                                  "flush"};
  return n;
}
inline const char* const* serve_stage_names() {
  static const char* const n[] = {"batch_wait", "gather", "enqueue",
                                  "sync_wait", "fanout"};
  return n;
}

class ClosedQueue : public std::runtime_error {
 public:
  using std::runtime_error::runtime_error;
};

class AsyncError : public std::runtime_error {
 public:
  using std::runtime_error::runtime_error;
};

inline bool pinned_memory_wanted() {
  static const bool wanted = [] {
    if (std::getenv("TBAMD_NO_PIN")) return false;
    return torch::cuda::is_available();
  }();
  return wanted;
}

// Concatenate leaves along `dim` into a pinned destination when a GPU is
// present (so the later .to(device, non_blocking=True) is DMA).
inline torch::Tensor cat_pinned(const std::vector<torch::Tensor>& tensors,
                                int64_t dim) {
  TORCH_CHECK(!tensors.empty(), "cat_pinned: empty tensor list");
  if (!pinned_memory_wanted() || tensors[0].is_cuda()) {
    return torch::cat(tensors, dim);
  }
  auto shape = tensors[0].sizes().vec();
  int64_t total = 0;
  for (const auto& t : tensors) total += t.size(dim);
  shape[dim] = total;
  int64_t bytes = tensors[0].element_size();
  for (auto d : shape) bytes *= d;
  if (bytes < 65536) {
    // Small outputs (slot ids, scalars): ragged pinned allocations would
    // hit hipHostMalloc (a device-wide sync) for every new size; a plain
    // cat + pageable H2D is far cheaper at this size.
    return torch::cat(tensors, dim);
  }
  torch::Tensor out = torch::empty(
      shape, tensors[0].options().pinned_memory(true));
  torch::cat_out(out, tensors, dim);
  return out;
}

// ---------------------------------------------------------------------------
// PinnedSlabPool: fixed-capacity pinned rollout buffering with backpressure.
//
// One pinned slab carved into equal rollout-sized slots (slot size fixed by
// the first acquire; every rollout of a run has the same shape). An actor
// stream acquires a slot up front and fills its carved VIEWS row by row
// (the nest/promise path instead cats its finished rollout into them), so
// .is_pinned() stays true and H2D copies stay DMA, and enqueues them.
// Rollout tensors never escape the learner-side BatchingQueue (both
// assembly modes produce fresh batched outputs), so slot recycling is
// driven by the queue alone: after assembling a batch it calls
// mark_consumed_many(leaf pointers, event) once, and each slot returns to
// the free list once that dequeue's copy event has completed (immediately
// in CPU mode). acquire() blocks when the budget is exhausted — this is the
// backpressure that bounds rollout memory to the configured budget
// (BASELINE.json north star: buffering sized against a memory budget, not
// unbounded ad-hoc allocations).
// ---------------------------------------------------------------------------

class PinnedSlabPool {
 public:
  explicit PinnedSlabPool(int64_t budget_bytes, int64_t min_slots = 64)
      : budget_bytes_(budget_bytes), min_slots_(min_slots) {}

  // Handle for filling one slot; carve() returns pinned slab views.
  struct Slot {
    PinnedSlabPool* pool;
    int64_t index;
    int64_t used = 0;

    uint8_t* base() const {
      return pool->slab_.data_ptr<uint8_t>() + index * pool->slot_bytes_;
    }

    torch::Tensor carve(std::vector<int64_t> shape, torch::ScalarType dtype) {
      int64_t numel = 1;
      for (auto d : shape) numel *= d;
      const int64_t nbytes = numel * (int64_t)torch::elementSize(dtype);
      const int64_t aligned = (used + 255) & ~int64_t(255);
      TORCH_CHECK(aligned + nbytes <= pool->slot_bytes_,
                  "rollout slot overflow");
      torch::Tensor flat = pool->slab_.narrow(
          0, index * pool->slot_bytes_ + aligned, nbytes);
      used = aligned + nbytes;
      return flat.view(dtype).reshape(shape);
    }
  };

  // Blocks until a slot is free; `cancelled` (checked every 50 ms) lets
  // shutdown unwind the actor threads.
  Slot acquire(int64_t slot_bytes, const std::function<bool()>& cancelled) {
    std::unique_lock<std::mutex> lk(mu_);
    if (!slab_.defined()) {
      slot_bytes_ = (slot_bytes + 4095) & ~int64_t(4095);
      int64_t slots = budget_bytes_ / slot_bytes_;
      if (slots < min_slots_) slots = min_slots_;
      pinned_ = pinned_memory_wanted();
      slab_ = torch::empty(
          {slots * slot_bytes_},
          torch::TensorOptions().dtype(torch::kUInt8).pinned_memory(pinned_));
      for (int64_t i = slots - 1; i >= 0; --i) free_.push_back(i);
      state_.assign(slots, SlotState::FREE);
      total_slots_ = slots;
    }
    TORCH_CHECK(slot_bytes <= slot_bytes_,
                "rollout larger than the slab slot size");
    for (;;) {
      reap_pending();
      if (!free_.empty()) {
        const int64_t idx = free_.back();
        free_.pop_back();
        state_[idx] = SlotState::ACQUIRED;
        ++held_;
        return Slot{this, idx, 0};
      }
      backpressure_waits_.fetch_add(1, std::memory_order_relaxed);
      cv_.wait_for(lk, std::chrono::milliseconds(50));
      if (cancelled && cancelled()) {
        throw ClosedQueue("slab pool acquire cancelled");
      }
    }
  }

  // Consumer-side: the slot holding `ptr` was read by copies whose
  // completion `ev` tracks (ev == nullptr for synchronous CPU assembly).
  // One call per slot: a second call for the same slot could land after the
  // slot was freed and re-acquired and would free it under its new owner.
  // A consumer that sees several pointers into one slot (the leaves of a
  // rollout) uses mark_consumed_many instead.
  void mark_consumed(const void* ptr,
                     const std::shared_ptr<at::cuda::CUDAEvent>& ev) {
    mark_consumed_many({ptr}, ev);
  }

  // Release every slot that one dequeue read, in ONE critical section over
  // the unique slot indices, so a slot cannot be freed, handed to another
  // actor and then freed again by a later leaf of the same dequeue.
  // Pointers outside the slab are ignored.
  void mark_consumed_many(const std::vector<const void*>& ptrs,
                          const std::shared_ptr<at::cuda::CUDAEvent>& ev) {
    std::lock_guard<std::mutex> lk(mu_);
    if (!slab_.defined()) return;
    const uint8_t* base = slab_.data_ptr<uint8_t>();
    std::vector<int64_t> idxs;
    idxs.reserve(ptrs.size());
    for (const void* ptr : ptrs) {
      const auto* p = static_cast<const uint8_t*>(ptr);
      if (p < base || p >= base + total_slots_ * slot_bytes_) continue;
      idxs.push_back((p - base) / slot_bytes_);
    }
    std::sort(idxs.begin(), idxs.end());
    idxs.erase(std::unique(idxs.begin(), idxs.end()), idxs.end());
    for (int64_t idx : idxs) {
      // Only a slot somebody holds can be released; FREE or PENDING here
      // means it was released already.
      if (state_[idx] != SlotState::ACQUIRED) continue;
      --held_;
      if (ev == nullptr) {
        state_[idx] = SlotState::FREE;
        free_.push_back(idx);
      } else {
        state_[idx] = SlotState::PENDING;
        pending_.emplace_back(idx, ev);
      }
    }
    if (!idxs.empty()) cv_.notify_all();
  }

  bool manages(const void* ptr) const {
    std::lock_guard<std::mutex> lk(mu_);
    if (!slab_.defined()) return false;
    const uint8_t* base = slab_.data_ptr<uint8_t>();
    const auto* p = static_cast<const uint8_t*>(ptr);
    return p >= base && p < base + total_slots_ * slot_bytes_;
  }

  // Where the slots lie (all zero before the first acquire); fixed from
  // then on.
  SlabGeometry geometry() const {
    std::lock_guard<std::mutex> lk(mu_);
    if (!slab_.defined()) return SlabGeometry();
    return SlabGeometry{slab_.data_ptr<uint8_t>(), slot_bytes_,
                        total_slots_ * slot_bytes_};
  }

  // Is the slab page-locked, i.e. can the GPU read slot addresses as they
  // are? False before the first acquire, under TBAMD_NO_PIN and without a
  // GPU.
  bool is_pinned() const {
    std::lock_guard<std::mutex> lk(mu_);
    return slab_.defined() && pinned_;
  }

  std::map<std::string, double> stats() const {
    std::lock_guard<std::mutex> lk(mu_);
    std::map<std::string, double> out;
    out["slab_slots"] = (double)total_slots_;
    out["slab_slot_bytes"] = (double)slot_bytes_;
    out["slab_free"] = (double)free_.size();
    out["slab_pending"] = (double)pending_.size();
    out["slab_held"] = (double)held_;
    out["slab_backpressure_waits"] = (double)backpressure_waits_.load();
    return out;
  }

 private:
  // FREE: on free_. ACQUIRED: held by an actor (filling) or travelling
  // through the learner queue. PENDING: read by H2D copies still in
  // flight; freed at reap time. A slot is freed only from ACQUIRED (no
  // event) or from PENDING (reap).
  enum class SlotState : uint8_t { FREE, ACQUIRED, PENDING };

  void reap_pending() {
    for (auto it = pending_.begin(); it != pending_.end();) {
      if (it->second->query()) {
        state_[it->first] = SlotState::FREE;
        free_.push_back(it->first);
        it = pending_.erase(it);
      } else {
        ++it;
      }
    }
  }

  const int64_t budget_bytes_;
  const int64_t min_slots_;
  mutable std::mutex mu_;
  std::condition_variable cv_;
  torch::Tensor slab_;
  bool pinned_ = false;
  int64_t slot_bytes_ = 0;
  int64_t total_slots_ = 0;
  std::vector<int64_t> free_;
  std::vector<SlotState> state_;
  int64_t held_ = 0;
  std::vector<std::pair<int64_t, std::shared_ptr<at::cuda::CUDAEvent>>>
      pending_;
  std::atomic<int64_t> backpressure_waits_{0};
};

inline TensorNest batch_nests(const std::vector<const TensorNest*>& nests,
                              int64_t batch_dim) {
  return TensorNest::apply_columns(
      nests, [batch_dim](const std::vector<torch::Tensor>& column) {
        return cat_pinned(column, batch_dim);
      });
}

// Batch assembly with the destination ON THE GPU: each (pinned) source
// tensor is copied with one async H2D into its slice of a device-resident
// output. Replaces {CPU cat -> one huge H2D} with B small DMAs that
// interleave with inference traffic, and eliminates the host-side memcpy
// entirely (the "rollouts DMA straight into the learner" design,
// SURVEY.md §2.2).
inline torch::Tensor copy_column_to_device(
    const std::vector<torch::Tensor>& column, int64_t batch_dim,
    torch::Device device) {
  auto shape = column[0].sizes().vec();
  int64_t total = 0;
  for (const auto& t : column) total += t.size(batch_dim);
  shape[batch_dim] = total;
  torch::Tensor out = torch::empty(shape, column[0].options().device(device));
  int64_t offset = 0;
  for (const auto& t : column) {
    out.narrow(batch_dim, offset, t.size(batch_dim))
        .copy_(t, /*non_blocking=*/true);
    offset += t.size(batch_dim);
  }
  return out;
}

inline TensorNest batch_nests_to_device(
    const std::vector<const TensorNest*>& nests, int64_t batch_dim,
    torch::Device device) {
  return TensorNest::apply_columns(
      nests,
      [batch_dim, device](const std::vector<torch::Tensor>& column) {
        return copy_column_to_device(column, batch_dim, device);
      });
}

// ---------------------------------------------------------------------------
// Generic bounded MPMC queue.
// ---------------------------------------------------------------------------

template <typename Item>
class BoundedQueue {
 public:
  explicit BoundedQueue(std::optional<int64_t> max_size = std::nullopt)
      : max_size_(max_size) {}

  void enqueue(Item item) {
    {
      std::unique_lock<std::mutex> lock(mu_);
      not_full_.wait(lock, [this] {
        return closed_ || !max_size_ ||
               static_cast<int64_t>(items_.size()) < *max_size_;
      });
      if (closed_) throw ClosedQueue("enqueue to closed queue");
      items_.push_back(std::move(item));
    }
    not_empty_.notify_one();
  }

  // Enqueue several items under one lock acquisition and one wake-up (the
  // consumer that drains only part of the queue wakes the next one, see
  // dequeue_many). A bounded queue may overshoot its bound by one call.
  void enqueue_many(std::vector<Item>& items) {
    if (items.empty()) return;
    {
      std::unique_lock<std::mutex> lock(mu_);
      not_full_.wait(lock, [this] {
        return closed_ || !max_size_ ||
               static_cast<int64_t>(items_.size()) < *max_size_;
      });
      if (closed_) throw ClosedQueue("enqueue to closed queue");
      for (auto& item : items) items_.push_back(std::move(item));
    }
    items.clear();
    not_empty_.notify_one();
  }

  // Block until at least min_n items (or timeout with >=1, or close).
  // Returns up to max_n items. Throws ClosedQueue when closed and drained.
  std::vector<Item> dequeue_many(int64_t min_n, int64_t max_n,
                                 std::optional<std::chrono::milliseconds>
                                     timeout = std::nullopt) {
    std::unique_lock<std::mutex> lock(mu_);
    auto have_min = [this, min_n] {
      return closed_ || static_cast<int64_t>(items_.size()) >= min_n;
    };
    if (timeout) {
      // After the deadline, settle for any non-empty prefix.
      if (!not_empty_.wait_for(lock, *timeout, have_min)) {
        not_empty_.wait(lock, [this] { return closed_ || !items_.empty(); });
      }
    } else {
      not_empty_.wait(lock, have_min);
    }
    if (items_.empty()) {
      // Only reachable when closed.
      throw ClosedQueue("queue is closed");
    }
    int64_t n = std::min<int64_t>(items_.size(), max_n);
    std::vector<Item> out;
    out.reserve(n);
    for (int64_t i = 0; i < n; ++i) {
      out.push_back(std::move(items_.front()));
      items_.pop_front();
    }
    const bool leftover = !items_.empty();
    lock.unlock();
    not_full_.notify_all();
    // enqueue_many wakes one consumer for many items: pass the wake on.
    if (leftover) not_empty_.notify_one();
    return out;
  }

  int64_t size() const {
    std::lock_guard<std::mutex> lock(mu_);
    return items_.size();
  }

  void close() {
    {
      std::lock_guard<std::mutex> lock(mu_);
      if (closed_) throw ClosedQueue("queue was already closed");
      closed_ = true;
    }
    not_empty_.notify_all();
    not_full_.notify_all();
  }

  bool is_closed() const {
    std::lock_guard<std::mutex> lock(mu_);
    return closed_;
  }

  // close(), and in the same critical section remove and return the queued
  // items `pred` selects.
  template <typename Pred>
  std::vector<Item> close_and_take(Pred pred) {
    std::vector<Item> taken;
    {
      std::lock_guard<std::mutex> lock(mu_);
      if (closed_) throw ClosedQueue("queue was already closed");
      closed_ = true;
      std::deque<Item> kept;
      for (auto& item : items_) {
        if (pred(item)) {
          taken.push_back(std::move(item));
        } else {
          kept.push_back(std::move(item));
        }
      }
      items_.swap(kept);
    }
    not_empty_.notify_all();
    not_full_.notify_all();
    return taken;
  }

 private:
  mutable std::mutex mu_;
  std::condition_variable not_empty_;
  std::condition_variable not_full_;
  std::deque<Item> items_;
  std::optional<int64_t> max_size_;
  bool closed_ = false;
};

// ---------------------------------------------------------------------------
// Learner-facing queue of rollouts, batched along batch_dim on dequeue.
// ---------------------------------------------------------------------------

class BatchingQueue {
 public:
  BatchingQueue(int64_t batch_dim = 0,
                std::optional<int64_t> minimum_batch_size = std::nullopt,
                std::optional<int64_t> maximum_batch_size = std::nullopt,
                std::optional<int64_t> timeout_ms = std::nullopt,
                bool check_inputs = true,
                std::optional<int64_t> maximum_queue_size = std::nullopt,
                std::optional<std::string> output_device = std::nullopt)
      : output_device_(output_device
                           ? std::optional<torch::Device>(
                                 torch::Device(*output_device))
                           : std::nullopt),
        batch_dim_(batch_dim),
        min_batch_size_(minimum_batch_size ? *minimum_batch_size : 1),
        max_batch_size_(maximum_batch_size
                            ? *maximum_batch_size
                            : std::numeric_limits<int64_t>::max()),
        timeout_(timeout_ms
                     ? std::optional<std::chrono::milliseconds>(
                           std::chrono::milliseconds(*timeout_ms))
                     : std::nullopt),
        check_inputs_(check_inputs),
        max_queue_size_(maximum_queue_size),
        queue_(maximum_queue_size) {
    if (min_batch_size_ < 1) {
      throw std::invalid_argument("Min batch size must be >= 1");
    }
    if (max_batch_size_ < min_batch_size_) {
      throw std::invalid_argument(
          "Max batch size must be >= min batch size");
    }
    if (maximum_queue_size && *maximum_queue_size < 1) {
      throw std::invalid_argument("Max queue size must be >= 1");
    }
    // TBAMD_QUEUE_GATHER=0 keeps the per-leaf copies for every batch (A/B).
    const char* g = std::getenv("TBAMD_QUEUE_GATHER");
    gather_enabled_ = !(g != nullptr && std::string(g) == "0");
  }

  int64_t batch_dim() const { return batch_dim_; }

  void enqueue(TensorNest item) {
    if (check_inputs_) {
      if (item.empty()) throw std::invalid_argument("Empty input");
      item.for_each([this](const torch::Tensor& t) {
        if (t.dim() <= batch_dim_) {
          throw std::invalid_argument(
              "Enqueued tensors must have more than batch_dim dims");
        }
      });
    }
    queue_.enqueue(std::move(item));
  }

  // One batched nest (cat along batch_dim) + the number of rollouts in it.
  std::pair<TensorNest, int64_t> dequeue_many() {
    const int64_t t0 = now_us();
    std::vector<TensorNest> items =
        queue_.dequeue_many(min_batch_size_, max_batch_size_, timeout_);
    const int64_t t1 = now_us();
    std::vector<const TensorNest*> ptrs;
    ptrs.reserve(items.size());
    for (const auto& n : items) ptrs.push_back(&n);
    TensorNest batched;
    if (output_device_ && output_device_->is_cuda()) {
      // Assemble directly on the GPU: async copies on a dedicated copy
      // stream, then make the caller's stream wait on them.
      if (!copy_stream_) {
        copy_stream_ = std::make_unique<at::cuda::CUDAStream>(
            at::cuda::getStreamFromPool(false, output_device_->index()));
      }
      at::cuda::CUDAStream current =
          at::cuda::getCurrentCUDAStream(output_device_->index());
      // Set by the gather path once nothing enqueued later reads a slot.
      std::shared_ptr<at::cuda::CUDAEvent> release_ev;
      {
        at::cuda::CUDAStreamGuard guard(*copy_stream_);
        if (!(gather_enabled_ && source_pool_ && unpack_hook() != nullptr &&
              gather_to_device(ptrs, &batched, &release_ev))) {
          batched = batch_nests_to_device(ptrs, batch_dim_, *output_device_);
        }
      }
      auto ev = std::make_shared<at::cuda::CUDAEvent>();
      ev->record(*copy_stream_);
      ev->block(current);
      // The batch blocks were allocated on the copy stream but are consumed
      // (and eventually freed) on the caller's stream: tell the caching
      // allocator, or it may recycle them while the consumer still reads.
      batched.for_each([&current](const torch::Tensor& t) {
        t.record_stream(current);
      });
      if (source_pool_) {
        // Slab-pooled rollout slots recycle once the H2D copies complete.
        source_pool_->mark_consumed_many(leaf_pointers(ptrs),
                                         release_ev ? release_ev : ev);
      }
    } else {
      batched = batch_nests(ptrs, batch_dim_);
      if (source_pool_) {
        source_pool_->mark_consumed_many(leaf_pointers(ptrs), nullptr);
      }
    }
    auto result = std::make_pair(std::move(batched),
                                 static_cast<int64_t>(items.size()));
    wait_stats_.add(t1 - t0);
    cat_stats_.add(now_us() - t1);
    return result;
  }

  int64_t size() const { return queue_.size(); }
  void close() { queue_.close(); }
  bool is_closed() const { return queue_.is_closed(); }
  std::optional<int64_t> max_queue_size() const { return max_queue_size_; }
  int64_t max_batch_size() const { return max_batch_size_; }

  // CPU-time counters of the actor threads feeding this queue (they show
  // up in stats() so a driver that prints stats() prints them too).
  CpuStageCounters& actor_counters() { return actor_counters_; }

  std::map<std::string, double> stats() const {
    std::map<std::string, double> out;
    actor_counters_.report("actor", actor_stage_names(), "sweeps",
                           "env_steps", &out);
    out["dequeues"] = wait_stats_.n.load();
    if (wait_stats_.n > 0) {
      out["avg_wait_ms"] = wait_stats_.sum_us / 1e3 / wait_stats_.n;
      out["avg_cat_ms"] = cat_stats_.sum_us / 1e3 / cat_stats_.n;
    }
    if (source_pool_) {
      for (const auto& kv : source_pool_->stats()) out[kv.first] = kv.second;
    }
    // Dequeues assembled by slot DMA + unpack kernel, and the leaf
    // positions they gathered (the rest took the per-leaf copies).
    out["gather_dequeues"] = (double)gather_dequeues_.load();
    out["gather_columns"] = (double)gather_columns_.load();
    return out;
  }

  void set_source_pool(std::shared_ptr<PinnedSlabPool> pool) {
    source_pool_ = std::move(pool);
  }

  // Drop accumulated latency stats (steady-state measurement after warmup).
  void reset_stats() {
    wait_stats_.reset();
    cat_stats_.reset();
    actor_counters_.reset();
    gather_dequeues_.store(0, std::memory_order_relaxed);
    gather_columns_.store(0, std::memory_order_relaxed);
  }

 private:
  // Batch assembly from whole slots (rollout_gather.h), on the current
  // (copy) stream: one DMA per item from its slot window into its staging
  // row, one unpack kernel into a single output arena, and the per-leaf
  // copies for the positions that are no slab column. Returns false, with
  // nothing enqueued, when the plan is empty. *release_ev is set when the
  // slots may be recycled as soon as the DMAs are done.
  bool gather_to_device(const std::vector<const TensorNest*>& nests,
                        TensorNest* batched,
                        std::shared_ptr<at::cuda::CUDAEvent>* release_ev) {
    std::vector<std::vector<torch::Tensor>> flats;
    flats.reserve(nests.size());
    for (const auto* n : nests) flats.push_back(n->flatten());
    const SlabGeometry geom = source_pool_->geometry();
    const GatherPlan plan = plan_gather(flats, batch_dim_, geom);
    if (plan.empty()) return false;
    const UnpackHook unpack = unpack_hook();
    at::cuda::CUDAStream stream =
        at::cuda::getCurrentCUDAStream(output_device_->index());

    // Does a position left to the per-leaf copies read slot memory? Then
    // the slots are released by the caller's event, after those copies.
    bool fallback_reads_slab = false;
    for (size_t i = 0; i < plan.gathered.size(); ++i) {
      if (plan.gathered[i]) continue;
      for (const auto& f : flats) {
        if (f[i].defined() && f[i].device().is_cpu() &&
            geom.contains(f[i].data_ptr())) {
          fallback_reads_slab = true;
        }
      }
    }

    GatherOutputs outputs;
    {
      // Several learner threads may dequeue at once; the staging buffer is
      // shared, so one batch's DMAs and its kernel are enqueued together.
      std::lock_guard<std::mutex> lk(gather_mu_);
      const int64_t stride = plan.stride();
      // Persistent staging: grown only when a larger batch arrives. It is
      // written and read on the copy stream alone, so reuse is safe by
      // stream order: the next batch's DMAs queue up behind this batch's
      // unpack kernel (and a replaced buffer goes back to the allocator
      // on the same stream).
      if (!staging_.defined() || staging_.numel() < plan.B * stride) {
        staging_ = torch::empty({plan.B * stride},
                                torch::TensorOptions()
                                    .dtype(torch::kUInt8)
                                    .device(*output_device_));
      }
      auto* staging = staging_.data_ptr<uint8_t>();
      for (int64_t b = 0; b < plan.B; ++b) {
        const hipError_t err = hipMemcpyAsync(
            staging + b * stride, plan.window_start[b], plan.win_bytes,
            hipMemcpyHostToDevice, stream.stream());
        TORCH_CHECK(err == hipSuccess, "rollout gather: hipMemcpyAsync: ",
                    hipGetErrorString(err));
      }
      if (!fallback_reads_slab) {
        // The last read of any slot: recycle them before the unpack runs.
        *release_ev = std::make_shared<at::cuda::CUDAEvent>();
        (*release_ev)->record(stream);
      }
      outputs = make_gather_outputs(plan, *output_device_);
      unpack(staging, stride, plan.B, outputs.columns.data(),
             (int)outputs.columns.size());
    }

    std::vector<torch::Tensor> leaves(plan.gathered.size());
    for (size_t c = 0; c < plan.columns.size(); ++c) {
      leaves[plan.columns[c].leaf] = std::move(outputs.leaves[c]);
    }
    std::vector<torch::Tensor> column(flats.size());
    for (size_t i = 0; i < leaves.size(); ++i) {
      if (plan.gathered[i]) continue;
      for (size_t b = 0; b < flats.size(); ++b) column[b] = flats[b][i];
      leaves[i] = copy_column_to_device(column, batch_dim_, *output_device_);
    }
    *batched = nests[0]->pack_from(std::move(leaves));
    gather_dequeues_.fetch_add(1, std::memory_order_relaxed);
    gather_columns_.fetch_add((int64_t)plan.columns.size(),
                              std::memory_order_relaxed);
    return true;
  }

  static std::vector<const void*> leaf_pointers(
      const std::vector<const TensorNest*>& nests) {
    std::vector<const void*> out;
    for (const auto* n : nests) {
      n->for_each(
          [&out](const torch::Tensor& t) { out.push_back(t.data_ptr()); });
    }
    return out;
  }

  const std::optional<torch::Device> output_device_;
  const int64_t batch_dim_;
  const int64_t min_batch_size_;
  const int64_t max_batch_size_;
  const std::optional<std::chrono::milliseconds> timeout_;
  const bool check_inputs_;
  const std::optional<int64_t> max_queue_size_;
  BoundedQueue<TensorNest> queue_;
  std::shared_ptr<PinnedSlabPool> source_pool_;
  std::unique_ptr<at::cuda::CUDAStream> copy_stream_;
  bool gather_enabled_ = true;
  std::mutex gather_mu_;
  torch::Tensor staging_;  // device, B x window; see gather_to_device
  std::atomic<int64_t> gather_dequeues_{0};
  std::atomic<int64_t> gather_columns_{0};
  mutable StageStats wait_stats_;
  mutable StageStats cat_stats_;
  CpuStageCounters actor_counters_;
};

// ---------------------------------------------------------------------------
// DynamicBatcher: many blocking compute() callers -> one batched inference.
// ---------------------------------------------------------------------------

// ---------------------------------------------------------------------------
// Rollout rows and completion mailboxes (the actor fast path).
//
// An env stream that fills its rollout in place owns one pinned slot carved
// into [T+1, 1, ...] columns, one per env leaf and per agent-output leaf.
// Step t is a ROW of every column: a raw pointer plus a row-byte size. An
// inference request for such a step is a small POD (slot base, row, layout,
// mailbox, env index) instead of a tensor nest plus a promise; whoever
// serves it reads the env leaves from the row, writes the agent outputs
// into the same row and posts the env index to the owning actor thread's
// mailbox -- one lock and at most one wake per actor thread per batch.
// ---------------------------------------------------------------------------

struct RowLeaf {
  std::vector<int64_t> shape;  // one step, leading [1, 1, ...] included
  torch::ScalarType dtype;
  int64_t row_bytes;
  int64_t offset;  // of the column inside the slot (256-byte aligned)
};

struct RowLayout {
  TensorNest env_template;    // structure of one step's env outputs
  TensorNest agent_template;  // structure of one step's agent outputs
  std::vector<RowLeaf> leaves;  // env leaves first, then agent leaves
  size_t n_env = 0;
  int64_t rows = 0;  // T + 1
  int64_t slot_bytes = 0;
  // Obs-slab mode's row form: the C++ runner gathers frames and rewards on
  // the GPU straight from the rows (runtime_kernels.hip gather_rows) instead
  // of copying them through pinned staging on the host.
  bool device_gather = false;

  static RowLeaf describe(const torch::Tensor& t) {
    TORCH_CHECK(t.dim() >= 1 && t.size(0) == 1,
                "rollout rows need step leaves with a leading time dim of 1, "
                "got shape ", t.sizes());
    RowLeaf l;
    l.shape = t.sizes().vec();
    l.dtype = t.scalar_type();
    l.row_bytes = t.numel() * (int64_t)t.element_size();
    l.offset = 0;
    return l;
  }

  static std::shared_ptr<RowLayout> make(const TensorNest& env_outputs,
                                         const TensorNest& agent_outputs,
                                         int64_t rows) {
    auto out = std::make_shared<RowLayout>();
    out->env_template = env_outputs;
    out->agent_template = agent_outputs;
    out->rows = rows;
    env_outputs.for_each(
        [&](const torch::Tensor& t) { out->leaves.push_back(describe(t)); });
    out->n_env = out->leaves.size();
    agent_outputs.for_each(
        [&](const torch::Tensor& t) { out->leaves.push_back(describe(t)); });
    int64_t used = 0;
    for (auto& l : out->leaves) {
      // Same packing as PinnedSlabPool::Slot::carve.
      l.offset = (used + 255) & ~int64_t(255);
      used = l.offset + rows * l.row_bytes;
    }
    out->slot_bytes = used + 4096;
    // The templates only give structure; do not keep the first step alive.
    auto drop = [](const torch::Tensor&) { return torch::Tensor(); };
    out->env_template = out->env_template.map(drop);
    out->agent_template = out->agent_template.map(drop);
    return out;
  }

  bool leaf_matches(size_t i, const torch::Tensor& t) const {
    const RowLeaf& l = leaves[i];
    return t.scalar_type() == l.dtype && t.sizes().vec() == l.shape;
  }

  // Is a row the flagship step: env leaves (frame u8 [1, 1, C, H, W], reward
  // f32, ...) and agent leaves (action i64, logits f32 [A], baseline f32)?
  // The C++ runner reads a row's reward and writes its agent outputs through
  // typed pointers on the strength of exactly these checks.
  bool is_flagship_step(int64_t A) const {
    if (n_env < 3 || leaves.size() != n_env + 3) return false;
    const RowLeaf& frame = leaves[0];
    const RowLeaf& reward = leaves[1];
    const RowLeaf& action = leaves[n_env];
    const RowLeaf& logits = leaves[n_env + 1];
    const RowLeaf& baseline = leaves[n_env + 2];
    return frame.dtype == torch::kUInt8 && frame.shape.size() == 5 &&
           reward.dtype == torch::kFloat32 && reward.row_bytes == 4 &&
           action.dtype == torch::kInt64 && action.row_bytes == 8 &&
           logits.dtype == torch::kFloat32 && logits.row_bytes == 4 * A &&
           baseline.dtype == torch::kFloat32 && baseline.row_bytes == 4;
  }
};

// State rows: the recurrent state of every env stream of a pool in ONE
// block, [n_streams, 2 halves, 2 (h, c), L, H] f32, pinned when a GPU is
// there so that the serve kernels read and write it in place. A stream's
// state lives in its current half; whoever answers a row request writes the
// new state into the other half, and the halves swap when the request is
// posted (Batch::complete_rows), so a writer never touches what a reader of
// the same step reads. Allocated once, with a quantised size: a fresh
// pinned allocation synchronises the device.
struct StateBlock {
  torch::Tensor storage;  // f32, at least n_streams * 4 * L * H elements
  int64_t n_streams = 0, L = 0, H = 0;
  bool pinned = false;

  // Is `state` a pair (h, c) of contiguous f32 [L, 1, H] tensors?
  static bool describes(const TensorNest& state, int64_t* L, int64_t* H) {
    if (!state.is_vector() || state.vector().size() != 2) return false;
    const auto& v = state.vector();
    if (!v[0].is_leaf() || !v[1].is_leaf()) return false;
    const torch::Tensor& h = v[0].leaf();
    const torch::Tensor& c = v[1].leaf();
    for (const torch::Tensor* t : {&h, &c}) {
      if (!t->defined() || !t->device().is_cpu() ||
          t->scalar_type() != torch::kFloat32 || t->dim() != 3 ||
          t->size(1) != 1 || t->size(0) < 1 || t->size(2) < 1 ||
          !t->is_contiguous()) {
        return false;
      }
    }
    if (h.sizes() != c.sizes()) return false;
    *L = h.size(0);
    *H = h.size(2);
    return true;
  }

  static std::shared_ptr<StateBlock> make(int64_t n_streams, int64_t L,
                                          int64_t H) {
    auto out = std::make_shared<StateBlock>();
    out->n_streams = n_streams;
    out->L = L;
    out->H = H;
    out->pinned = pinned_memory_wanted();
    // Quantised to 64 KiB.
    const int64_t quantum = 16384;
    const int64_t numel =
        (n_streams * 4 * L * H + quantum - 1) / quantum * quantum;
    out->storage = torch::zeros(
        {numel}, torch::TensorOptions().dtype(torch::kFloat32).pinned_memory(
                     out->pinned));
    return out;
  }

  // Can `state` (an answer's state slice: any device, any strides) be
  // copied into a half: an (h, c) pair of f32 [L, 1, H] tensors?
  bool takes(const TensorNest& state) const {
    if (!state.is_vector() || state.vector().size() != 2) return false;
    for (const auto& leaf : state.vector()) {
      if (!leaf.is_leaf() || !leaf.leaf().defined()) return false;
      const torch::Tensor& t = leaf.leaf();
      if (t.scalar_type() != torch::kFloat32 || t.dim() != 3 ||
          t.size(0) != L || t.size(1) != 1 || t.size(2) != H) {
        return false;
      }
    }
    return true;
  }

  int64_t half_floats() const { return 2 * L * H; }
  float* base() const { return storage.data_ptr<float>(); }
  int64_t used_bytes() const { return n_streams * 2 * half_floats() * 4; }
  float* half(int64_t stream, int half) const {
    return base() + (stream * 2 + half) * half_floats();
  }
  // (h, c) views [L, 1, H] of one half; they keep the block alive.
  TensorNest views(int64_t stream, int half) const {
    const int64_t off = (stream * 2 + half) * half_floats();
    return TensorNest(TensorNest::vector_t{
        TensorNest(storage.narrow(0, off, L * H).view({L, 1, H})),
        TensorNest(storage.narrow(0, off + L * H, L * H).view({L, 1, H}))});
  }
};

// Completion queue of one actor thread, shared with every request of that
// thread still in flight (so a serve thread can never post into a dead
// actor thread's memory). state[i] is env i's agent state: read by the
// server as the request's input state, replaced by the new state before i
// is posted to `ready`. With state rows (state_block set) the state is not
// replaced: half_views[2 * i + cur_half[i]] is env i's state, the answer is
// written into the other half and cur_half[i] flips before i is posted.
struct ActorMailbox {
  std::mutex mu;
  std::condition_variable cv;
  std::vector<int32_t> ready;
  enum Failure { kNone, kAsync, kClosed };
  Failure failed = kNone;
  std::string error;
  std::vector<TensorNest> state;
  std::shared_ptr<const RowLayout> layout;
  // The slab the rows point into: kept alive for requests in flight, and
  // asked for its bounds by whoever hands row addresses to the GPU.
  std::shared_ptr<PinnedSlabPool> slab;
  // State rows (see StateBlock); all empty without them.
  std::shared_ptr<StateBlock> state_block;
  std::vector<int32_t> stream_index;    // env i's stream in the block
  std::vector<uint8_t> cur_half;        // env i's current half
  std::vector<TensorNest> half_views;   // [2 * i + half]

  bool has_state_rows() const { return state_block != nullptr; }
  float* state_in(int32_t i) const {
    return state_block->half(stream_index[i], cur_half[i]);
  }
  float* state_out(int32_t i) const {
    return state_block->half(stream_index[i], cur_half[i] ^ 1);
  }

  int64_t outstanding = 0;  // requests submitted and not yet answered

  void submitted(int64_t n) {
    std::lock_guard<std::mutex> lk(mu);
    outstanding += n;
  }
  void post(const int32_t* idx, size_t n) {
    {
      std::lock_guard<std::mutex> lk(mu);
      ready.insert(ready.end(), idx, idx + n);
      outstanding -= (int64_t)n;
    }
    cv.notify_one();
  }
  // An unwinding actor thread waits (bounded) until nobody works on its
  // requests any more, so that when ActorPool::run() returns no consumer is
  // still computing an answer for this pool.
  void wait_idle(std::chrono::milliseconds limit) {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait_for(lk, limit, [this] { return outstanding <= 0; });
  }
  // The first failure wins. kAsync: a batch was dropped (AsyncError);
  // kClosed: the batcher was closed under the request (ClosedQueue).
  void fail(const std::string& what, Failure kind, int64_t n_requests = 1) {
    {
      std::lock_guard<std::mutex> lk(mu);
      outstanding -= n_requests;
      if (failed == kNone) {
        failed = kind;
        error = what;
      }
    }
    cv.notify_all();
  }
  // Blocks (no polling) until completions or a failure arrive; swaps the
  // ready indices into `out`.
  void wait(std::vector<int32_t>* out) {
    out->clear();
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [this] { return failed != kNone || !ready.empty(); });
    if (failed == kAsync) throw AsyncError(error);
    if (failed == kClosed) throw ClosedQueue(error);
    out->swap(ready);
  }
};

class DynamicBatcher {
 public:
  struct Request {
    TensorNest inputs;
    int64_t batch_size;  // along batch_dim
    std::shared_ptr<std::promise<TensorNest>> promise;
    // Row form (promise == nullptr, inputs unused): see ActorMailbox.
    std::shared_ptr<ActorMailbox> mailbox;
    const RowLayout* layout = nullptr;
    uint8_t* slot_base = nullptr;
    int32_t row = 0;
    int32_t env_index = 0;

    bool is_row() const { return mailbox != nullptr; }
    uint8_t* leaf_ptr(size_t leaf) const {
      const RowLeaf& l = layout->leaves[leaf];
      return slot_base + l.offset + (int64_t)row * l.row_bytes;
    }
    // The agent state this request is to be answered from: with state rows
    // an (h, c) nest of views of the stream's current half.
    const TensorNest& state() const {
      if (mailbox->has_state_rows()) {
        return mailbox
            ->half_views[2 * env_index + mailbox->cur_half[env_index]];
      }
      return mailbox->state[env_index];
    }
    // The env leaves of the row as a [1, 1, ...] nest of views.
    TensorNest env_nest() const {
      std::vector<torch::Tensor> leaves;
      for (size_t i = 0; i < layout->n_env; ++i) {
        const RowLeaf& l = layout->leaves[i];
        leaves.push_back(torch::from_blob(
            leaf_ptr(i), l.shape, torch::TensorOptions().dtype(l.dtype)));
      }
      return layout->env_template.pack_from(std::move(leaves));
    }
  };

  class Batch {
   public:
    Batch(int64_t batch_dim, std::vector<Request> requests, bool check_outputs,
          StageStats* service_stats = nullptr)
        : batch_dim_(batch_dim),
          requests_(std::move(requests)),
          check_outputs_(check_outputs),
          service_stats_(service_stats),
          created_us_(now_us()) {
      for (const auto& r : requests_) {
        if (r.is_row()) {
          ++n_rows_;
          if (r.layout != requests_[0].layout) uniform_rows_ = false;
        }
      }
    }

    ~Batch() {
      if (!fulfilled_) {
        const char* what = "Batch destroyed before set_outputs was called";
        auto eptr = std::make_exception_ptr(AsyncError(what));
        // fulfilled_count_ promises already carry values (set_outputs threw
        // mid-way); breaking those again would raise future_error out of a
        // destructor, so only fail the rest.
        for (size_t i = fulfilled_count_; i < requests_.size(); ++i) {
          if (requests_[i].promise) requests_[i].promise->set_exception(eptr);
        }
        // Row requests are posted only once everything succeeded, so none
        // of them has been answered: every owning actor thread gets the
        // error (it throws AsyncError out of its wait).
        for (const auto& r : requests_) {
          if (r.is_row()) r.mailbox->fail(what, ActorMailbox::kAsync);
        }
      }
    }

    int64_t size() const {
      int64_t total = 0;
      for (const auto& r : requests_) total += r.batch_size;
      return total;
    }

    // True when every request is a row of one layout: the C++ runner then
    // gathers and scatters rows itself (requests(), complete_rows()).
    bool all_rows() const {
      return n_rows_ == requests_.size() && uniform_rows_ && n_rows_ > 0;
    }
    const std::vector<Request>& requests() const { return requests_; }

    TensorNest get_inputs() {
      if (all_rows() && batch_dim_ <= 1) return gather_rows();
      // Nest requests, or a mix (start-up, when some streams still send
      // their first step as a nest): rows join as [1, 1, ...] views.
      std::vector<TensorNest> row_nests;
      row_nests.reserve(n_rows_);
      for (const auto& r : requests_) {
        if (r.is_row()) {
          row_nests.push_back(
              TensorNest(TensorNest::vector_t{r.env_nest(), r.state()}));
        }
      }
      std::vector<const TensorNest*> ptrs;
      ptrs.reserve(requests_.size());
      size_t k = 0;
      for (const auto& r : requests_) {
        ptrs.push_back(r.is_row() ? &row_nests[k++] : &r.inputs);
      }
      return batch_nests(ptrs, batch_dim_);
    }

    void set_outputs(TensorNest outputs) {
      if (fulfilled_) {
        throw std::runtime_error("set_outputs called twice");
      }
      if (check_outputs_) {
        const int64_t expected = size();
        outputs.for_each([this, expected](const torch::Tensor& t) {
          if (t.dim() <= batch_dim_) {
            throw std::invalid_argument(
                "With batch_dim == " + std::to_string(batch_dim_) +
                ", output shape must have at least " +
                std::to_string(batch_dim_ + 1) + " dims but got " +
                std::to_string(t.dim()));
          }
          if (t.size(batch_dim_) != expected) {
            throw std::invalid_argument(
                "Output shape must have the same batch dimension as the "
                "input batch size. Expected: " + std::to_string(expected) +
                ". Observed: " + std::to_string(t.size(batch_dim_)));
          }
        });
      }
      // Slice for every caller BEFORE fulfilling any promise: narrow() can
      // throw on a mis-shaped output (when check_outputs is off), and a
      // half-fulfilled batch would make the destructor re-break satisfied
      // promises.
      std::vector<TensorNest> slices;
      slices.reserve(requests_.size());
      int64_t offset = 0;
      for (auto& req : requests_) {
        slices.push_back(
            outputs.map([this, offset, &req](const torch::Tensor& t) {
              return t.narrow(batch_dim_, offset, req.batch_size);
            }));
        offset += req.batch_size;
      }
      if (n_rows_ > 0) {
        // Validate every row request's slice against its carved columns
        // before writing any: a mismatch throws here, the batch stays
        // unfulfilled and its destructor fails the actors loudly.
        for (size_t i = 0; i < requests_.size(); ++i) {
          if (requests_[i].is_row()) check_row_slice(requests_[i], slices[i]);
        }
        for (size_t i = 0; i < requests_.size(); ++i) {
          if (requests_[i].is_row()) scatter_row(requests_[i], slices[i]);
        }
      }
      for (size_t i = 0; i < requests_.size(); ++i) {
        if (requests_[i].promise) {
          requests_[i].promise->set_value(std::move(slices[i]));
        }
        fulfilled_count_ = i + 1;
      }
      complete_rows();
    }

    // Post every row request to its actor thread (grouped: one lock and one
    // wake per mailbox) and mark the batch served. The caller has written
    // the agent outputs into the rows and the new states into the
    // mailboxes. set_outputs() ends with this; the C++ runner calls it
    // directly after scattering rows itself.
    void complete_rows() {
      if (fulfilled_) throw std::runtime_error("batch completed twice");
      if (n_rows_ > 0) {
        std::vector<std::pair<ActorMailbox*, int32_t>> order;
        order.reserve(n_rows_);
        for (const auto& r : requests_) {
          if (!r.is_row()) continue;
          // State rows: the answer's state sits in the other half. The
          // mailbox lock taken by post() publishes the flip to the actor.
          if (r.mailbox->has_state_rows()) {
            r.mailbox->cur_half[r.env_index] ^= 1;
          }
          order.emplace_back(r.mailbox.get(), r.env_index);
        }
        std::sort(order.begin(), order.end());
        std::vector<int32_t> idx;
        for (size_t i = 0; i < order.size();) {
          size_t j = i;
          idx.clear();
          for (; j < order.size() && order[j].first == order[i].first; ++j) {
            idx.push_back(order[j].second);
          }
          order[i].first->post(idx.data(), idx.size());
          i = j;
        }
      }
      fulfilled_count_ = requests_.size();
      fulfilled_ = true;
      if (service_stats_ != nullptr) {
        service_stats_->add(now_us() - created_us_);
      }
    }

   private:
    // One output tensor per leaf, filled by copying each request's row; no
    // per-request tensor. Needs batch_dim <= 1 (step leaves are [1, 1, ...],
    // so the batched leaf is the rows back to back).
    TensorNest gather_rows() {
      const RowLayout& layout = *requests_[0].layout;
      const int64_t b = (int64_t)requests_.size();
      std::vector<torch::Tensor> leaves;
      leaves.reserve(layout.n_env);
      for (size_t i = 0; i < layout.n_env; ++i) {
        const RowLeaf& l = layout.leaves[i];
        TORCH_CHECK((int64_t)l.shape.size() > batch_dim_ &&
                        l.shape[batch_dim_] == 1,
                    "row leaf has no batch dimension of size 1");
        auto shape = l.shape;
        shape[batch_dim_] = b;
        auto opts = torch::TensorOptions().dtype(l.dtype);
        // Same pinning rule as cat_pinned.
        if (pinned_memory_wanted() && b * l.row_bytes >= 65536) {
          opts = opts.pinned_memory(true);
        }
        torch::Tensor out = torch::empty(shape, opts);
        auto* dst = static_cast<uint8_t*>(out.data_ptr());
        for (int64_t r = 0; r < b; ++r) {
          std::memcpy(dst + r * l.row_bytes, requests_[r].leaf_ptr(i),
                      l.row_bytes);
        }
        leaves.push_back(std::move(out));
      }
      std::vector<const TensorNest*> states;
      states.reserve(requests_.size());
      for (const auto& r : requests_) states.push_back(&r.state());
      return TensorNest(TensorNest::vector_t{
          layout.env_template.pack_from(std::move(leaves)),
          batch_nests(states, batch_dim_)});
    }

    static const TensorNest& agent_part(const TensorNest& slice) {
      if (!slice.is_vector() || slice.vector().size() != 2) {
        throw std::invalid_argument(
            "inference must return ((action, ...), agent_state)");
      }
      return slice.vector()[0];
    }

    void check_row_slice(const Request& req, const TensorNest& slice) const {
      const RowLayout& layout = *req.layout;
      size_t i = layout.n_env;
      agent_part(slice).for_each([&](const torch::Tensor& t) {
        if (i >= layout.leaves.size() || !layout.leaf_matches(i, t)) {
          throw std::invalid_argument(
              "agent output leaf " + std::to_string(i - layout.n_env) +
              " disagrees with the dtype/shape the rollout slots were "
              "carved for");
        }
        ++i;
      });
      if (i != layout.leaves.size()) {
        throw std::invalid_argument(
            "agent outputs have fewer leaves than the rollout slots were "
            "carved for");
      }
      if (req.mailbox->has_state_rows() &&
          !req.mailbox->state_block->takes(slice.vector()[1])) {
        throw std::invalid_argument(
            "agent state disagrees with the (h, c) [L, 1, H] float32 state "
            "rows of the pool");
      }
    }

    void scatter_row(const Request& req, const TensorNest& slice) {
      const RowLayout& layout = *req.layout;
      size_t i = layout.n_env;
      agent_part(slice).for_each([&](const torch::Tensor& t) {
        torch::Tensor c = t.is_cuda() ? t.cpu() : t.contiguous();
        std::memcpy(req.leaf_ptr(i), c.data_ptr(), layout.leaves[i].row_bytes);
        ++i;
      });
      if (req.mailbox->has_state_rows()) {
        // Into the half nobody reads (check_row_slice vouches for the
        // shapes); complete_rows() makes it the current one.
        const StateBlock& blk = *req.mailbox->state_block;
        float* out = req.mailbox->state_out(req.env_index);
        const int64_t n = blk.L * blk.H;
        int64_t k = 0;
        for (const auto& leaf : slice.vector()[1].vector()) {
          const torch::Tensor& t = leaf.leaf();
          torch::Tensor c = (t.is_cuda() ? t.cpu() : t).contiguous();
          std::memcpy(out + k * n, c.data_ptr<float>(), n * sizeof(float));
          ++k;
        }
        return;
      }
      req.mailbox->state[req.env_index] = slice.vector()[1];
    }

    const int64_t batch_dim_;
    std::vector<Request> requests_;
    const bool check_outputs_;
    StageStats* service_stats_;
    const int64_t created_us_;
    size_t n_rows_ = 0;
    bool uniform_rows_ = true;
    bool fulfilled_ = false;
    size_t fulfilled_count_ = 0;
  };

  DynamicBatcher(int64_t batch_dim = 0,
                 std::optional<int64_t> minimum_batch_size = std::nullopt,
                 std::optional<int64_t> maximum_batch_size = std::nullopt,
                 std::optional<int64_t> timeout_ms = std::nullopt,
                 bool check_outputs = true)
      : batch_dim_(batch_dim),
        min_batch_size_(minimum_batch_size ? *minimum_batch_size : 1),
        max_batch_size_(maximum_batch_size
                            ? *maximum_batch_size
                            : std::numeric_limits<int64_t>::max()),
        timeout_(timeout_ms
                     ? std::optional<std::chrono::milliseconds>(
                           std::chrono::milliseconds(*timeout_ms))
                     : std::nullopt),
        check_outputs_(check_outputs),
        queue_(std::nullopt) {}

  // Called by actor threads; blocks until the consumer sets outputs.
  // Enqueue a request and return the future (the multi-env actor loop
  // waits on several of these at once).
  std::future<TensorNest> compute_async(TensorNest inputs) {
    if (inputs.empty()) {
      throw std::invalid_argument("compute() on empty nest");
    }
    int64_t batch_size = -1;
    inputs.for_each([this, &batch_size](const torch::Tensor& t) {
      if (t.dim() <= batch_dim_) {
        throw std::invalid_argument("Input needs more dims than batch_dim");
      }
      if (batch_size < 0) {
        batch_size = t.size(batch_dim_);
      } else if (t.size(batch_dim_) != batch_size) {
        throw std::invalid_argument(
            "Input tensors disagree on the batch dimension");
      }
    });
    auto promise = std::make_shared<std::promise<TensorNest>>();
    std::future<TensorNest> future = promise->get_future();
    queue_.enqueue(Request{std::move(inputs), batch_size, std::move(promise)});
    return future;
  }

  // Row requests of one actor thread: one lock acquisition for all of them.
  // `requests` is emptied.
  void submit_rows(std::vector<Request>& requests) {
    queue_.enqueue_many(requests);
  }

  int64_t max_batch_size() const { return max_batch_size_; }

  // CPU-time counters of the threads serving this batcher.
  CpuStageCounters& serve_counters() { return serve_counters_; }

  // Batches the C++ runner served on its row path (rows read and written in
  // place, persistent staging) rather than through get_inputs/set_outputs.
  void count_row_batch() {
    row_batches_.fetch_add(1, std::memory_order_relaxed);
  }
  // Those of them whose frames and rewards the GPU gathered from the rows.
  void count_device_gather_batch() {
    device_gather_batches_.fetch_add(1, std::memory_order_relaxed);
  }

  // Those of them that were recurrent: states read from and written to the
  // pool's state rows by the LSTM serve kernels.
  void count_state_row_batch() {
    state_row_batches_.fetch_add(1, std::memory_order_relaxed);
  }

  TensorNest compute(TensorNest inputs) {
    const int64_t t0 = now_us();
    std::future<TensorNest> future = compute_async(std::move(inputs));
    if (future.wait_for(std::chrono::minutes(10)) ==
        std::future_status::timeout) {
      throw AsyncError("compute() timed out after 10 minutes");
    }
    auto result = future.get();  // Rethrows AsyncError from a dropped batch.
    roundtrip_stats_.add(now_us() - t0);
    return result;
  }

  std::shared_ptr<Batch> get_batch() {
    const int64_t t0 = now_us();
    std::vector<Request> requests =
        queue_.dequeue_many(min_batch_size_, max_batch_size_, timeout_);
    formation_stats_.add(now_us() - t0);
    int64_t total = 0;
    for (const auto& r : requests) total += r.batch_size;
    batch_size_stats_.add(total);
    return std::make_shared<Batch>(batch_dim_, std::move(requests),
                                   check_outputs_, &service_stats_);
  }

  int64_t size() const { return queue_.size(); }

  // Queued nest requests stay for the consumers to drain, as before. Queued
  // row requests are withdrawn and their actor threads told at once: such a
  // thread ends at its next submit anyway, so serving them is wasted work,
  // and a thread whose requests nobody serves any more (consumers gone)
  // would otherwise sit in its mailbox forever.
  void close() {
    std::vector<Request> rows =
        queue_.close_and_take([](const Request& r) { return r.is_row(); });
    for (const auto& r : rows) {
      r.mailbox->fail("inference batcher closed", ActorMailbox::kClosed);
    }
  }
  bool is_closed() const { return queue_.is_closed(); }

  std::map<std::string, double> stats() const {
    std::map<std::string, double> out;
    serve_counters_.report("serve", serve_stage_names(), "batches",
                           "requests", &out);
    out["serve_row_batches"] = (double)row_batches_.load();
    out["serve_device_gather_batches"] =
        (double)device_gather_batches_.load();
    out["serve_state_row_batches"] = (double)state_row_batches_.load();
    out["computes"] = roundtrip_stats_.n.load();
    out["batches"] = batch_size_stats_.n.load();
    if (roundtrip_stats_.n > 0) {
      out["avg_roundtrip_ms"] =
          roundtrip_stats_.sum_us / 1e3 / roundtrip_stats_.n;
    }
    if (batch_size_stats_.n > 0) {
      out["avg_batch_size"] =
          double(batch_size_stats_.sum_us) / batch_size_stats_.n;
      out["avg_formation_wait_ms"] =
          formation_stats_.sum_us / 1e3 / formation_stats_.n;
    }
    if (service_stats_.n > 0) {
      out["avg_service_ms"] = service_stats_.sum_us / 1e3 / service_stats_.n;
    }
    return out;
  }

  void reset_stats() {
    roundtrip_stats_.reset();
    formation_stats_.reset();
    batch_size_stats_.reset();
    service_stats_.reset();
    serve_counters_.reset();
    row_batches_.store(0, std::memory_order_relaxed);
    device_gather_batches_.store(0, std::memory_order_relaxed);
    state_row_batches_.store(0, std::memory_order_relaxed);
  }

 private:
  const int64_t batch_dim_;
  const int64_t min_batch_size_;
  const int64_t max_batch_size_;
  const std::optional<std::chrono::milliseconds> timeout_;
  const bool check_outputs_;
  BoundedQueue<Request> queue_;
  mutable StageStats roundtrip_stats_;
  mutable StageStats formation_stats_;
  mutable StageStats service_stats_;
  mutable StageStats batch_size_stats_;  // sum_us field holds summed sizes
  CpuStageCounters serve_counters_;
  std::atomic<int64_t> row_batches_{0};
  std::atomic<int64_t> device_gather_batches_{0};
  std::atomic<int64_t> state_row_batches_{0};
};

}  // namespace tbruntime
