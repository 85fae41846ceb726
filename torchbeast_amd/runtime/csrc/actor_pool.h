// ActorPool: one driver thread per environment, funneling single steps
// through the DynamicBatcher for batched GPU inference and complete
// [T+1, 1, ...] rollouts into the learner BatchingQueue.
//
// Capability parity with the reference ActorPool (ref:
// src/cc/actorpool.cc:342-564): rollouts overlap by one step (the last step
// of rollout k is the first of rollout k+1), and the agent state recorded
// with a rollout is the state *before* the inference of its first step.
//
// Two implementations:
// - loop_rows (default whenever the pool has a rollout budget; in obs-slab
//   mode only for a stateless agent, or a recurrent one with state rows
//   (recurrent_rows / TBAMD_RECURRENT_ROWS=1, off by default), whose batches
//   the runner then gathers from the rows on the GPU): every env stream
//   holds a pinned slab slot carved into [T+1, 1, ...] columns and fills it
//   row by row in place. With state rows the (h, c) state of every stream
//   lives in one pinned block as well (StateBlock, queues.h). Envs write their
//   step into the row (EnvConnection::step_into), requests are row PODs
//   submitted under one lock per sweep, and the thread blocks on its own
//   ActorMailbox (queues.h) -- no per-step tensors, promises or polling. A
//   finished rollout is enqueued as the carved views.
// - loop / loop_multi (no rollout budget, obs-slab mode with a recurrent
//   agent, or TBAMD_ACTOR_FASTPATH=0 for A/B runs): per-step nests (slot
//   ids into a second pinned slab in obs-slab mode), promise/future
//   requests, rollouts cat-ed at flush time.

#pragma once

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <future>
#include <mutex>
#include <memory>
#include <string>
#include <vector>

#include "env_transport.h"
#include "queues.h"

namespace tbruntime {

class ActorPool {
 public:
  ActorPool(int64_t unroll_length, std::shared_ptr<BatchingQueue> learner_queue,
            std::shared_ptr<DynamicBatcher> inference_batcher,
            std::vector<std::string> env_server_addresses,
            TensorNest initial_agent_state, int64_t seed_base = 0,
            bool use_obs_slab = false, int64_t rollout_budget_mb = 0,
            int64_t envs_per_thread = 1,
            std::optional<bool> recurrent_rows = std::nullopt)
      : unroll_length_(unroll_length),
        learner_queue_(std::move(learner_queue)),
        inference_batcher_(std::move(inference_batcher)),
        addresses_(std::move(env_server_addresses)),
        initial_agent_state_(std::move(initial_agent_state)),
        seed_base_(seed_base),
        use_obs_slab_(use_obs_slab),
        envs_per_thread_(std::max<int64_t>(1, envs_per_thread)) {
    if (unroll_length_ < 1) {
      throw std::invalid_argument("unroll_length must be >= 1");
    }
    if (rollout_budget_mb > 0) {
      // Budget-sized pinned rollout ring with backpressure (replaces
      // unbounded ad-hoc pinned allocations); the learner queue recycles
      // slots after its H2D assembly completes.
      //
      // Slot floor = actors + learner-queue capacity + two learner batches.
      // Every slot is FREE, held by a stream, in the learner queue (at most
      // its capacity Q) or PENDING (read by H2D copies; freed in finite
      // time whatever the actors do). A stream fills one slot; at the end
      // of a rollout it acquires the next slot BEFORE it enqueues the
      // finished one (row T is copied to the new row 0 while the old slot
      // is still its own), so a stream blocked in acquire() holds exactly
      // one slot. If every stream were blocked there, streams would hold
      // `actors` slots and the queue at most Q, so at least two batches'
      // worth of slots are FREE or PENDING and some acquire() returns:
      // no deadlock. A stream not in acquire() waits for inference, which
      // needs no slot, or sits in enqueue() on a full learner queue. The
      // latter holds TWO slots (the finished one, not yet queued, and its
      // new one), so streams can hold up to 2 x actors slots in all; but a
      // full queue means the learner can dequeue -- assuming, as every
      // driver configures, a queue capacity of at least the learner batch
      // size -- and each dequeue frees slots and queue room, so those
      // streams move on without acquiring anything. The two batches are
      // throughput slack: one batch being copied (PENDING) while the next
      // one forms.
      const int64_t queue_cap = learner_queue_->max_queue_size().value_or(64);
      const int64_t batch =
          std::min<int64_t>(learner_queue_->max_batch_size(), 1024);
      rollout_pool_ = std::make_shared<PinnedSlabPool>(
          rollout_budget_mb * (1 << 20),
          /*min_slots=*/(int64_t)addresses_.size() + queue_cap + 2 * batch);
      learner_queue_->set_source_pool(rollout_pool_);
    }
    // TBAMD_ACTOR_FASTPATH=0 keeps the nest/promise loops below (A/B only).
    const bool fastpath = actor_fastpath_enabled();
    // State rows (opt-in): an (h, c) agent state lives in one pinned block
    // of the pool's (StateBlock, queues.h) instead of per-request tensors,
    // and the C++ runner's LSTM serve kernels read and write it in place.
    // recurrent_rows = true insists (a state of another form is an error);
    // unset, TBAMD_RECURRENT_ROWS=1 asks for it where the state allows.
    int64_t state_L = 0, state_H = 0;
    const bool state_fits =
        StateBlock::describes(initial_agent_state_, &state_L, &state_H);
    if (recurrent_rows.has_value()) {
      if (*recurrent_rows && !state_fits) {
        throw std::invalid_argument(
            "recurrent_rows needs an agent state (h, c) of contiguous "
            "float32 [L, 1, H] tensors");
      }
      recurrent_rows_ = *recurrent_rows;
    } else {
      const char* v = std::getenv("TBAMD_RECURRENT_ROWS");
      recurrent_rows_ = v != nullptr && std::string(v) == "1" && state_fits;
    }
    // Obs-slab mode has a row form: the frame is written once, into its
    // rollout row, and the runner gathers the batch from the rows on the GPU
    // (RowLayout::device_gather). No second slab, no slot ids. For a
    // stateless agent always; for a recurrent one with state rows. Without
    // them a recurrent agent on rows would fall back to a host gather of its
    // frames, so it keeps the slot-id loops.
    device_gather_ = use_obs_slab_ && rollout_pool_ != nullptr && fastpath &&
                     (initial_agent_state_.empty() || recurrent_rows_);
    use_rows_ = rollout_pool_ != nullptr && fastpath &&
                (!use_obs_slab_ || device_gather_);
    if (recurrent_rows_ && use_rows_) {
      // Once, before any actor thread runs: a fresh pinned allocation
      // synchronises the device.
      state_block_ =
          StateBlock::make((int64_t)addresses_.size(), state_L, state_H);
    }
  }

  // Pinned observation slab (slot per actor). Valid once the first env has
  // produced an observation; the inference runner gathers from it by slot
  // id instead of cat-ing per-request frame tensors. Empty (at once) when
  // the pool is not in obs-slab mode or takes the row form, which has no
  // such slab.
  std::vector<torch::Tensor> obs_slab() {
    if (device_gather_ || !use_obs_slab_) return {};
    std::unique_lock<std::mutex> lk(slab_mu_);
    slab_cv_.wait(lk, [this] { return slab_ready_ || failed_; });
    if (failed_ && !slab_ready_) {
      throw std::runtime_error("actor pool failed before producing obs");
    }
    return {slab_frames_, slab_rew_, slab_done_};
  }

  // Blocks until every actor thread exits (via queue close or error).
  // Rethrows the first actor failure.
  void run() {
    std::vector<std::future<void>> futures;
    const size_t k = (size_t)envs_per_thread_;
    if (k > 1 || use_rows_) {
      // Event-driven mode: each thread drives k env streams with
      // overlapped inference requests. 512 actor threads were measured
      // host-scheduling-bound (serve latency scaled with thread count,
      // profiles/PROFILE_r2.md); k envs per thread keeps the same env
      // parallelism with 1/k threads. Best for in-process synthetic envs
      // whose step() is microseconds; socket envs keep k == 1 so a slow
      // remote env cannot stall its neighbors.
      const size_t nthreads = (addresses_.size() + k - 1) / k;
      futures.reserve(nthreads);
      for (size_t t = 0; t < nthreads; ++t) {
        const size_t lo = t * k;
        const size_t hi = std::min(addresses_.size(), lo + k);
        futures.push_back(std::async(std::launch::async, [this, lo, hi] {
          try {
            if (use_rows_) {
              loop_rows(lo, hi);
            } else {
              loop_multi(lo, hi);
            }
          } catch (...) {
            {
              std::lock_guard<std::mutex> lk(slab_mu_);
              failed_ = true;
            }
            slab_cv_.notify_all();
            throw;
          }
        }));
      }
      collect(futures);
      return;
    }
    futures.reserve(addresses_.size());
    for (size_t i = 0; i < addresses_.size(); ++i) {
      futures.push_back(std::async(std::launch::async, [this, i] {
        try {
          loop(addresses_[i], i);
        } catch (...) {
          // Wake obs_slab() waiters so setup can't hang on a dead actor.
          {
            std::lock_guard<std::mutex> lk(slab_mu_);
            failed_ = true;
          }
          slab_cv_.notify_all();
          throw;
        }
      }));
    }
    collect(futures);
  }

  uint64_t count() const { return step_count_.load(std::memory_order_relaxed); }

 private:
  // Copy this actor's observation into its pinned slot; the request nest
  // then carries only the slot id (gathered GPU-side by the runner).
  void fill_slot(int64_t slot, const TensorNest& env_outputs) {
    const auto& f = env_outputs.vector();
    const torch::Tensor frame = f[0].leaf();
    if (!slab_ready_) {
      std::lock_guard<std::mutex> lk(slab_mu_);
      if (!slab_ready_) {
        const int64_t n = (int64_t)addresses_.size();
        auto fshape = frame.sizes().vec();  // [1,1,C,H,W]
        std::vector<int64_t> slab_shape = {n};
        slab_shape.insert(slab_shape.end(), fshape.begin() + 2, fshape.end());
        // Pinned only when a GPU exists (pinned allocs require HIP);
        // CPU runs use the slab purely as shared host storage.
        auto hopts =
            torch::TensorOptions().pinned_memory(torch::cuda::is_available());
        slab_frames_ = torch::empty(slab_shape, hopts.dtype(torch::kUInt8));
        slab_rew_ = torch::zeros({n}, hopts.dtype(torch::kFloat32));
        slab_done_ = torch::zeros({n}, hopts.dtype(torch::kUInt8));
        slab_ready_ = true;
        slab_cv_.notify_all();
      }
    }
    const int64_t fsz = slab_frames_.stride(0);
    std::memcpy(
        static_cast<uint8_t*>(slab_frames_.data_ptr()) + slot * fsz,
        frame.data_ptr(), fsz);
    slab_rew_.data_ptr<float>()[slot] = f[1].leaf().item<float>();
    slab_done_.data_ptr<uint8_t>()[slot] = f[2].leaf().item<bool>() ? 1 : 0;
  }

  void collect(std::vector<std::future<void>>& futures) {
    std::exception_ptr first_error;
    for (auto& f : futures) {
      try {
        f.get();
      } catch (const ClosedQueue&) {
        // Normal shutdown path.
      } catch (...) {
        if (!first_error) first_error = std::current_exception();
      }
    }
    if (first_error) std::rethrow_exception(first_error);
  }

  // One thread, several env streams, overlapped inference futures. A
  // request is outstanding per env; completions are collected with a
  // short-timeout wait on one pending future plus a zero-timeout scan of
  // the rest (completions are correlated: batchmates finish together).
  void loop_multi(size_t lo, size_t hi) {
    struct EnvSlot {
      std::unique_ptr<EnvConnection> env;
      TensorNest env_outputs;
      TensorNest agent_state;
      TensorNest rollout_initial_state;
      TensorNest state_before;
      TensorNest slot_req;
      std::vector<TensorNest> rollout;
      std::future<TensorNest> pending;
      bool has_pending = false;
    };
    const size_t n = hi - lo;
    std::vector<EnvSlot> envs(n);
    for (size_t i = 0; i < n; ++i) {
      EnvSlot& e = envs[i];
      e.env = make_env_connection(addresses_[lo + i],
                                  seed_base_ + (int64_t)(lo + i) + 1);
      e.env_outputs = e.env->initial();
      e.agent_state = initial_agent_state_;
      e.rollout_initial_state = initial_agent_state_;
      e.rollout.reserve(unroll_length_ + 1);
      if (use_obs_slab_) {
        e.slot_req = TensorNest(torch::full(
            {1, 1}, (int64_t)(lo + i),
            torch::TensorOptions().dtype(torch::kInt32)));
      }
    }

    auto issue = [&](size_t i) {
      EnvSlot& e = envs[i];
      e.state_before = e.agent_state;
      TensorNest request;
      if (use_obs_slab_) {
        fill_slot((int64_t)(lo + i), e.env_outputs);
        request = TensorNest(TensorNest::vector_t{e.slot_req, e.agent_state});
      } else {
        request =
            TensorNest(TensorNest::vector_t{e.env_outputs, e.agent_state});
      }
      e.pending = inference_batcher_->compute_async(std::move(request));
      e.has_pending = true;
    };

    for (size_t i = 0; i < n; ++i) issue(i);

    // CPU-time counters, sampled per sweep: this loop interleaves collect,
    // env step and issue per env, so all three land under "collect".
    CpuStageCounters& cnt = learner_queue_->actor_counters();
    int64_t flush_ns = 0;
    for (;;) {
      const int64_t c0 = thread_cpu_ns();
      // Block briefly on the first pending future, then sweep all.
      size_t first = n;
      for (size_t i = 0; i < n; ++i) {
        if (envs[i].has_pending) {
          first = i;
          break;
        }
      }
      if (first == n) throw std::logic_error("no pending inference");
      envs[first].pending.wait_for(std::chrono::microseconds(500));
      const int64_t c1 = thread_cpu_ns();
      int64_t stepped = 0;
      flush_ns = 0;

      for (size_t i = 0; i < n; ++i) {
        EnvSlot& e = envs[i];
        if (!e.has_pending ||
            e.pending.wait_for(std::chrono::seconds(0)) !=
                std::future_status::ready) {
          continue;
        }
        e.has_pending = false;
        TensorNest result = e.pending.get();  // rethrows AsyncError
        if (!result.is_vector() || result.vector().size() != 2) {
          throw std::runtime_error(
              "inference must return ((action, ...), agent_state)");
        }
        TensorNest agent_outputs = result.vector()[0];
        e.agent_state = result.vector()[1];

        if (e.rollout.empty()) e.rollout_initial_state = e.state_before;
        e.rollout.push_back(
            TensorNest(TensorNest::vector_t{e.env_outputs, agent_outputs}));

        if (static_cast<int64_t>(e.rollout.size()) == unroll_length_ + 1) {
          const int64_t f0 = thread_cpu_ns();
          flush_rollout(e.rollout, e.rollout_initial_state);
          TensorNest last = std::move(e.rollout.back());
          e.rollout.clear();
          e.rollout.push_back(std::move(last));
          e.rollout_initial_state = e.state_before;
          flush_ns += thread_cpu_ns() - f0;
        }

        const torch::Tensor& action = agent_outputs.front();
        e.env_outputs = e.env->step(action);
        step_count_.fetch_add(1, std::memory_order_relaxed);
        issue(i);
        ++stepped;
      }
      const int64_t c2 = thread_cpu_ns();
      cnt.add(kActorWait, c1 - c0);
      cnt.add(kActorCollect, c2 - c1 - flush_ns);
      cnt.add(kActorFlush, flush_ns);
      cnt.rounds.fetch_add(1, std::memory_order_relaxed);
      cnt.items.fetch_add(stepped, std::memory_order_relaxed);
    }
  }

  // ---- rollout rows written in place (the default with a slab pool) ----

  struct RowStream {
    std::unique_ptr<EnvConnection> env;
    TensorNest views;            // the slot carved into [T+1, 1, ...] columns
    std::vector<uint8_t*> col;   // column base pointer per leaf
    uint8_t* base = nullptr;     // slot base
    int64_t t = 0;               // row whose inference is in flight / done
    TensorNest state_before;     // agent state before row t's inference
    TensorNest rollout_initial_state;
  };

  // The carved layout is pool-wide and learnt from the first complete step
  // any stream sees (its env outputs and the agent outputs answering them).
  std::shared_ptr<const RowLayout> ensure_layout(
      const TensorNest& env_outputs, const TensorNest& agent_outputs) {
    std::lock_guard<std::mutex> lk(layout_mu_);
    if (!layout_) {
      auto layout =
          RowLayout::make(env_outputs, agent_outputs, unroll_length_ + 1);
      layout->device_gather = device_gather_;
      layout_ = std::move(layout);
    }
    return layout_;
  }

  // Acquire a slot for `s` and carve it. Blocks on pool backpressure.
  void acquire_row_slot(RowStream& s, const RowLayout& layout) {
    auto slot = rollout_pool_->acquire(
        layout.slot_bytes, [this] { return learner_queue_->is_closed(); });
    s.base = slot.base();
    s.col.resize(layout.leaves.size());
    std::vector<torch::Tensor> views;
    views.reserve(layout.leaves.size());
    for (size_t i = 0; i < layout.leaves.size(); ++i) {
      const RowLeaf& l = layout.leaves[i];
      auto shape = l.shape;
      shape[0] = layout.rows;
      torch::Tensor v = slot.carve(shape, l.dtype);
      s.col[i] = s.base + l.offset;
      TORCH_CHECK(v.data_ptr() == s.col[i], "row layout / carve mismatch");
      views.push_back(std::move(v));
    }
    std::vector<torch::Tensor> env_views(views.begin(),
                                         views.begin() + layout.n_env);
    std::vector<torch::Tensor> agent_views(views.begin() + layout.n_env,
                                           views.end());
    s.views = TensorNest(TensorNest::vector_t{
        layout.env_template.pack_from(std::move(env_views)),
        layout.agent_template.pack_from(std::move(agent_views))});
  }

  // State rows: the state answering a stream's first step (a nest request)
  // becomes half 0 of the stream, its current half.
  void store_first_state(ActorMailbox& mailbox, size_t i,
                         const TensorNest& state) const {
    int64_t L = 0, H = 0;
    const TensorNest host = state.map([](const torch::Tensor& t) {
      return (t.is_cuda() ? t.cpu() : t).contiguous();
    });
    if (!StateBlock::describes(host, &L, &H) || L != state_block_->L ||
        H != state_block_->H) {
      throw std::runtime_error(
          "first step's agent state disagrees with the pool's state rows");
    }
    float* dst = state_block_->half(mailbox.stream_index[i], 0);
    const int64_t n = L * H;
    std::memcpy(dst, host.vector()[0].leaf().data_ptr<float>(), n * 4);
    std::memcpy(dst + n, host.vector()[1].leaf().data_ptr<float>(), n * 4);
    mailbox.cur_half[i] = 0;
  }

  // One thread, several env streams, each filling its rollout slot in
  // place. Requests are row PODs submitted under one lock per sweep; the
  // thread blocks on its own mailbox, drains every ready env, steps those
  // envs and resubmits.
  void loop_rows(size_t lo, size_t hi) {
    const size_t n = hi - lo;
    const int64_t T = unroll_length_;
    std::vector<RowStream> streams(n);
    auto mailbox = std::make_shared<ActorMailbox>();
    mailbox->slab = rollout_pool_;
    const bool state_rows = state_block_ != nullptr;
    if (!state_rows) {
      mailbox->state.assign(n, initial_agent_state_);
    } else {
      // mailbox->state stays empty: the states are halves of the block.
      mailbox->state_block = state_block_;
      mailbox->stream_index.resize(n);
      mailbox->cur_half.assign(n, 0);
      mailbox->half_views.reserve(2 * n);
      for (size_t i = 0; i < n; ++i) {
        mailbox->stream_index[i] = (int32_t)(lo + i);
        for (int half = 0; half < 2; ++half) {
          mailbox->half_views.push_back(
              state_block_->views((int64_t)(lo + i), half));
        }
      }
    }

    // The first step of every stream travels as a nest request with a
    // promise: its answer shows the agent-output dtypes and shapes the
    // slots must be carved for before any row exists. Nothing is computed
    // twice and nothing is discarded; the step becomes row 0.
    std::vector<TensorNest> first_env(n);
    std::vector<std::future<TensorNest>> first(n);
    for (size_t i = 0; i < n; ++i) {
      RowStream& s = streams[i];
      s.env = make_env_connection(addresses_[lo + i],
                                  seed_base_ + (int64_t)(lo + i) + 1);
      first_env[i] = s.env->initial();
      s.state_before = initial_agent_state_;
      s.rollout_initial_state = initial_agent_state_;
      first[i] = inference_batcher_->compute_async(TensorNest(
          TensorNest::vector_t{first_env[i], initial_agent_state_}));
    }
    std::shared_ptr<const RowLayout> layout;
    std::vector<int32_t> ready;
    for (size_t i = 0; i < n; ++i) {
      RowStream& s = streams[i];
      TensorNest result = first[i].get();  // rethrows AsyncError
      if (!result.is_vector() || result.vector().size() != 2) {
        throw std::runtime_error(
            "inference must return ((action, ...), agent_state)");
      }
      const TensorNest& agent_outputs = result.vector()[0];
      if (state_rows) {
        store_first_state(*mailbox, i, result.vector()[1]);
      } else {
        mailbox->state[i] = result.vector()[1];
      }
      layout = ensure_layout(first_env[i], agent_outputs);
      acquire_row_slot(s, *layout);
      size_t leaf = 0;
      auto store = [&](const torch::Tensor& t) {
        if (leaf >= layout->leaves.size() || !layout->leaf_matches(leaf, t)) {
          throw std::runtime_error(
              "first step leaf " + std::to_string(leaf) +
              " disagrees with the carved rollout layout");
        }
        torch::Tensor c = t.contiguous();
        std::memcpy(s.col[leaf], c.data_ptr(), layout->leaves[leaf].row_bytes);
        ++leaf;
      };
      first_env[i].for_each(store);
      agent_outputs.for_each(store);
      if (leaf != layout->leaves.size()) {
        throw std::runtime_error("first step has too few leaves");
      }
      s.t = 0;
      ready.push_back((int32_t)i);
    }
    first_env.clear();
    first.clear();
    mailbox->layout = layout;
    const size_t n_env = layout->n_env;
    const RowLeaf& action_leaf = layout->leaves[n_env];

    CpuStageCounters& cnt = learner_queue_->actor_counters();
    std::vector<DynamicBatcher::Request> requests;
    std::vector<uint8_t*> leaf_ptr(n_env);
    int64_t c0 = thread_cpu_ns();
    try {
      for (;;) {
        // collect: row t of every ready stream is complete. A full rollout
        // is enqueued as its carved views; the stream moves to a new slot
        // whose row 0 is a copy of row T (rollouts overlap by one step).
        int64_t flush_ns = 0;
        for (int32_t i : ready) {
          RowStream& s = streams[i];
          if (s.t != T) continue;
          const int64_t f0 = thread_cpu_ns();
          TensorNest finished = std::move(s.views);
          std::vector<uint8_t*> old_col = s.col;
          acquire_row_slot(s, *layout);
          for (size_t l = 0; l < layout->leaves.size(); ++l) {
            const int64_t rb = layout->leaves[l].row_bytes;
            std::memcpy(s.col[l], old_col[l] + T * rb, rb);
          }
          learner_queue_->enqueue(TensorNest(TensorNest::vector_t{
              std::move(finished), s.rollout_initial_state}));
          s.rollout_initial_state = s.state_before;
          s.t = 0;
          flush_ns += thread_cpu_ns() - f0;
        }
        const int64_t c1 = thread_cpu_ns();

        // env step: answer row t's action, result lands in row t + 1.
        for (int32_t i : ready) {
          RowStream& s = streams[i];
          for (size_t l = 0; l < n_env; ++l) {
            leaf_ptr[l] = s.col[l] + (s.t + 1) * layout->leaves[l].row_bytes;
          }
          StepRow row{layout.get(), leaf_ptr.data(),
                      s.col[n_env] + s.t * action_leaf.row_bytes, &action_leaf};
          s.env->step_into(row);
          ++s.t;
        }
        step_count_.fetch_add(ready.size(), std::memory_order_relaxed);
        const int64_t c2 = thread_cpu_ns();

        // issue: one request per stepped env, one lock for all of them.
        requests.clear();
        for (int32_t i : ready) {
          RowStream& s = streams[i];
          if (!state_rows) {
            s.state_before = mailbox->state[i];
          } else if (s.t == T) {
            // Only row T's state is ever recorded (as the next rollout's
            // initial state), and the block goes on changing under it: a
            // real copy, once per rollout.
            s.state_before =
                mailbox->half_views[2 * i + mailbox->cur_half[i]].map(
                    [](const torch::Tensor& t) { return t.clone(); });
          }
          DynamicBatcher::Request r;
          r.batch_size = 1;
          r.mailbox = mailbox;
          r.layout = layout.get();
          r.slot_base = s.base;
          r.row = (int32_t)s.t;
          r.env_index = i;
          requests.push_back(std::move(r));
        }
        const int64_t stepped = (int64_t)ready.size();
        mailbox->submitted(stepped);
        try {
          inference_batcher_->submit_rows(requests);
        } catch (...) {
          mailbox->submitted(-stepped);
          throw;
        }
        const int64_t c3 = thread_cpu_ns();

        mailbox->wait(&ready);  // throws AsyncError for a dropped batch
        const int64_t c4 = thread_cpu_ns();
        cnt.add(kActorCollect, c1 - c0 - flush_ns);
        cnt.add(kActorFlush, flush_ns);
        cnt.add(kActorEnvStep, c2 - c1);
        cnt.add(kActorIssue, c3 - c2);
        cnt.add(kActorWait, c4 - c3);
        cnt.rounds.fetch_add(1, std::memory_order_relaxed);
        cnt.items.fetch_add(stepped, std::memory_order_relaxed);
        c0 = c4;
      }
    } catch (...) {
      // Leaving (closed queues or a failure): let consumers finish what
      // they hold of this thread's requests first.
      mailbox->wait_idle(std::chrono::milliseconds(2000));
      throw;
    }
  }

  // Stack a complete [T+1] rollout into a pinned destination and enqueue.
  void flush_rollout(const std::vector<TensorNest>& rollout,
                     const TensorNest& rollout_initial_state) {
    std::vector<const TensorNest*> steps;
    steps.reserve(rollout.size());
    for (const auto& s : rollout) steps.push_back(&s);
    TensorNest stacked;
    if (rollout_pool_) {
      if (rollout_slot_bytes_ == 0) {
        int64_t total = 0;
        TensorNest::apply_columns(
            steps, [&total](const std::vector<torch::Tensor>& column) {
              int64_t rows = 0;
              for (const auto& t : column) rows += t.size(0);
              // Logical row bytes (exactly what carve() will allocate).
              // NOT stride(0): batch-split agent outputs are views whose
              // stride spans the whole serve batch, which varies per
              // serve — racing estimators would disagree on the total and
              // a late, larger store would overflow the fixed slot size.
              const int64_t row_numel =
                  column[0].numel() / std::max<int64_t>(1, column[0].size(0));
              const int64_t bytes =
                  rows * row_numel * column[0].element_size();
              total += (bytes + 255) & ~int64_t(255);
              return column[0];
            });
        rollout_slot_bytes_ = total + 4096;
      }
      auto slot = rollout_pool_->acquire(
          rollout_slot_bytes_, [this] { return learner_queue_->is_closed(); });
      stacked = TensorNest::apply_columns(
          steps, [&slot](const std::vector<torch::Tensor>& column) {
            auto shape = column[0].sizes().vec();
            int64_t rows = 0;
            for (const auto& t : column) rows += t.size(0);
            shape[0] = rows;
            torch::Tensor out = slot.carve(shape, column[0].scalar_type());
            torch::cat_out(out, column, 0);
            return out;
          });
    } else {
      stacked = TensorNest::apply_columns(
          steps, [](const std::vector<torch::Tensor>& column) {
            return cat_pinned(column, /*dim=*/0);
          });
    }
    learner_queue_->enqueue(TensorNest(
        TensorNest::vector_t{std::move(stacked), rollout_initial_state}));
  }

  void loop(const std::string& address, uint64_t seed) {
    auto env = make_env_connection(address, seed_base_ + seed + 1);

    TensorNest env_outputs = env->initial();
    TensorNest agent_state = initial_agent_state_;
    TensorNest rollout_initial_state = initial_agent_state_;

    // Slot-id request leaf (constant per actor, reused every step).
    TensorNest slot_req;
    if (use_obs_slab_) {
      slot_req = TensorNest(torch::full({1, 1}, (int64_t)seed,
                                        torch::TensorOptions().dtype(
                                            torch::kInt32)));
    }

    std::vector<TensorNest> rollout;
    rollout.reserve(unroll_length_ + 1);

    for (;;) {
      TensorNest state_before = agent_state;
      TensorNest request;
      if (use_obs_slab_) {
        fill_slot((int64_t)seed, env_outputs);
        request = TensorNest(TensorNest::vector_t{slot_req, agent_state});
      } else {
        request = TensorNest(TensorNest::vector_t{env_outputs, agent_state});
      }
      TensorNest result = inference_batcher_->compute(std::move(request));
      if (!result.is_vector() || result.vector().size() != 2) {
        throw std::runtime_error(
            "inference must return ((action, ...), agent_state)");
      }
      TensorNest agent_outputs = result.vector()[0];
      agent_state = result.vector()[1];

      if (rollout.empty()) rollout_initial_state = state_before;
      rollout.push_back(
          TensorNest(TensorNest::vector_t{env_outputs, agent_outputs}));

      if (static_cast<int64_t>(rollout.size()) == unroll_length_ + 1) {
        flush_rollout(rollout, rollout_initial_state);
        // Overlap by one step: the rollout we just sent ends with the step
        // whose pre-inference state is `state_before`.
        TensorNest last = std::move(rollout.back());
        rollout.clear();
        rollout.push_back(std::move(last));
        rollout_initial_state = state_before;
      }

      const torch::Tensor& action = agent_outputs.front();
      env_outputs = env->step(action);
      step_count_.fetch_add(1, std::memory_order_relaxed);
    }
  }

  const int64_t unroll_length_;
  std::shared_ptr<BatchingQueue> learner_queue_;
  std::shared_ptr<DynamicBatcher> inference_batcher_;
  std::vector<std::string> addresses_;
  TensorNest initial_agent_state_;
  const int64_t seed_base_;
  const bool use_obs_slab_;
  const int64_t envs_per_thread_;
  std::mutex slab_mu_;
  std::condition_variable slab_cv_;
  std::atomic<bool> slab_ready_{false};
  bool failed_ = false;
  torch::Tensor slab_frames_, slab_rew_, slab_done_;
  std::shared_ptr<PinnedSlabPool> rollout_pool_;
  bool use_rows_ = false;
  bool device_gather_ = false;  // obs-slab mode on rows, see the constructor
  bool recurrent_rows_ = false;  // state rows asked for, see the constructor
  std::shared_ptr<StateBlock> state_block_;  // set when they are in use
  std::mutex layout_mu_;
  std::shared_ptr<const RowLayout> layout_;
  std::atomic<int64_t> rollout_slot_bytes_{0};
  std::atomic<uint64_t> step_count_{0};
};

}  // namespace tbruntime
