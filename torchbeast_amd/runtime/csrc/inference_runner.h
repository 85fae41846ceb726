// C++ inference engine: GIL-free behavior-model forwards.
//
// The reference serves inference from Python threads
// (ref: polybeast_learner.py:269-285); at MI355X throughput that path is
// GIL-bound (measured ~20-45 ms service latency for ~0.3 ms of GPU work).
// This runner consumes DynamicBatcher batches entirely in C++, each serve
// thread on a HIP stream of its own. serve() is a pipeline of stages that
// hand a ServeInputs along:
//   input   a device batch padded to 64, from one of three request forms:
//           rows of rollout slots, gathered into persistent staging on the
//           host (one memcpy per frame, one H2D) or, in obs-slab mode, by
//           gather_rows_kernel over the host link (inputs_from_rows); actor
//           ids into the pinned obs slab, gathered by gather_obs
//           (inputs_from_slots); tensors, cat-ed on the host by the batcher,
//           then H2D (inputs_from_tensors).
//   trunk   frames -> conv features -> fc: hand-written MFMA or fused conv
//           kernels, ATen/MIOpen for the rest. bf16 weight packs are cached
//           until mark_weights_dirty().
//   tail    heads, the batch's one stream synchronise, delivery: fused heads
//           scattered into the rows (tail_fused_rows) or into pinned tensors
//           (tail_fused), the LSTM serve kernels on the pool's pinned state
//           rows plus the heads, scattered into the rows (tail_lstm_rows,
//           for pools with recurrent_rows), or LSTM core + ATen heads + D2H
//           (tail_generic).
//   finish  counters, warmed batch sizes, TBAMD_SERVE_TIMINGS.
// Behavior-model weights are VIEWS of the learner's flat actor buffer, so
// weight sync stays one flat device copy with no runner involvement.

#pragma once

#include <ATen/cuda/CUDAContext.h>
#include <c10/cuda/CUDAGuard.h>
#include <hip/hip_runtime_api.h>
#include <torch/extension.h>

#include <atomic>
#include <cstdlib>
#include <mutex>
#include <set>
#include <thread>
#include <vector>

#include "../../ops/hip/atari_trunk.h"
#include "../../ops/hip/conv_mfma.h"
#include "queues.h"
#include "runtime_kernels.h"

namespace tbruntime {

class InferenceRunner {
 public:
  // weights order:
  //  shallow AtariNet (use_last_action=False):
  //   conv1.w, conv1.b, conv2.w, conv2.b, conv3.w, conv3.b,
  //   fc.w, fc.b, policy.w, policy.b, baseline.w, baseline.b
  //  deep IMPALA ResNet: per section (x3): conv.w, conv.b,
  //   res0.conv0.{w,b}, res0.conv1.{w,b}, res1.conv0.{w,b}, res1.conv1.{w,b}
  //   then fc.w, fc.b, policy.w, policy.b, baseline.w, baseline.b
  //  both: then per LSTM layer: w_ih, w_hh, b_ih, b_hh.
  InferenceRunner(std::shared_ptr<DynamicBatcher> batcher,
                  std::vector<torch::Tensor> weights, int64_t num_lstm_layers,
                  bool greedy = false, std::string model_type = "shallow")
      : batcher_(std::move(batcher)),
        weights_(std::move(weights)),
        num_lstm_layers_(num_lstm_layers),
        greedy_(greedy),
        deep_(model_type == "deep") {
    const size_t trunk = deep_ ? 30 : 6;
    head_base_ = trunk + 2;  // fc.w, fc.b come first after the trunk
    lstm_base_ = trunk + 6;  // fc(2) + policy(2) + baseline(2)
    TORCH_CHECK(weights_.size() >= lstm_base_ + 4 * (size_t)num_lstm_layers,
                "runner weight list too short for model/lstm config");
    TORCH_CHECK(weights_[0].is_cuda(), "runner weights must be on the GPU");
    device_ = weights_[0].device();
    // Deep 84x84 trunk serves on the hand-written MFMA 3x3 kernels
    // (conv_mfma.hip resnet_conv); MIOpen for other geometries, unless
    // TBAMD_RESNET_ANY=1 puts those on resnet_conv_any (see trunk()).
    deep_mfma_ = deep_ && !aten_only_ && weights_[0].size(0) == 16 &&
                 weights_[0].size(1) <= 8 && weights_[0].size(2) == 3 &&
                 tbamd::resnet_conv_supported(16, 42, 16);
    // The fused heads take a stateless core of [fc output, reward].
    fused_heads_ = !aten_only_ && num_lstm_layers_ == 0 &&
                   weights_[head_base_].size(0) <= 64 &&
                   weights_[head_base_].size(1) ==
                       weights_[head_base_ - 2].size(0) + 1;
    // The LSTM serve kernels take [fc output, reward] into layer 0 and hand
    // the last layer's h to the heads. A core too wide for the layer
    // kernel's LDS tile is served through get_inputs() / tail_generic.
    lstm_rows_ = !aten_only_ && num_lstm_layers_ > 0 &&
                 weights_[head_base_].size(0) <= 64;
    for (int64_t l = 0; l < num_lstm_layers_ && lstm_rows_; ++l) {
      const auto& w_ih = weights_[lstm_base_ + 4 * l];
      const auto& w_hh = weights_[lstm_base_ + 4 * l + 1];
      const int64_t H = weights_[lstm_base_ + 1].size(1);
      const int64_t I = l == 0 ? weights_[head_base_ - 2].size(0) + 1 : H;
      lstm_rows_ = w_ih.dim() == 2 && w_hh.dim() == 2 && w_hh.size(1) == H &&
                   w_ih.size(1) == I && w_ih.size(0) == 4 * H &&
                   w_hh.size(0) == 4 * H &&
                   w_ih.scalar_type() == torch::kFloat32 &&
                   weights_[head_base_].size(1) == H &&
                   lstm_serve_layer_fits(I, H);
    }
  }

  ~InferenceRunner() { stop(); }

  void start(int64_t num_threads) {
    running_ = true;
    for (int64_t i = 0; i < num_threads; ++i) {
      threads_.emplace_back([this] { loop(); });
    }
  }

  void stop() {
    running_ = false;
    if (batcher_ && !batcher_->is_closed()) {
      try {
        batcher_->close();
      } catch (...) {
      }
    }
    for (auto& t : threads_) {
      if (t.joinable()) t.join();
    }
    threads_.clear();
  }

  int64_t batches() const { return batches_.load(); }
  int64_t steps() const { return steps_.load(); }

  // Observation slab (from ActorPool::obs_slab) enabling the slot-id fast
  // path: requests carry only actor ids; frames/reward/done are gathered
  // GPU-side straight from the pinned slab.
  void set_obs_slab(torch::Tensor frames, torch::Tensor rew,
                    torch::Tensor done) {
    slab_frames_ = std::move(frames);
    slab_rew_ = std::move(rew);
    slab_done_ = std::move(done);
    frame_shape_ = std::vector<int64_t>(slab_frames_.sizes().begin() + 1,
                                        slab_frames_.sizes().end());
    has_slab_ = true;
  }

  // Learner weight sync happened: drop the cached bf16-packed trunk
  // weights (repacked lazily by the next serve).
  void mark_weights_dirty() { weights_version_.fetch_add(1); }

 private:
  void loop() {
    c10::cuda::CUDAGuard device_guard(device_);
    at::cuda::CUDAStream stream =
        at::cuda::getStreamFromPool(/*isHighPriority=*/true, device_.index());
    at::cuda::CUDAStreamGuard stream_guard(stream);
    torch::NoGradGuard no_grad;
    RowStaging staging;
    CpuMarks marks;
    marks.timing = serve_timing_;
    CpuStageCounters& cnt = batcher_->serve_counters();

    while (running_) {
      std::shared_ptr<DynamicBatcher::Batch> batch;
      marks.begin();
      try {
        batch = batcher_->get_batch();
      } catch (const ClosedQueue&) {
        break;
      }
      marks.mark(kServeBatchWait);
      try {
        serve(*batch, stream, staging, marks);
      } catch (const std::exception& e) {
        // Drop this batch (its promises break with AsyncError and the
        // affected actors surface it) but keep the engine serving.
        fprintf(stderr, "InferenceRunner error (batch dropped): %s\n",
                e.what());
        // The failed batch may have left H2D copies out of the persistent
        // staging in flight: nothing may reuse it before they are done.
        try {
          stream.synchronize();
        } catch (const std::exception& e2) {
          fprintf(stderr, "InferenceRunner: synchronise after error: %s\n",
                  e2.what());
        }
      }
      for (int i = 0; i < CpuStageCounters::kStages; ++i) {
        cnt.add(i, marks.ns[i]);
      }
      cnt.rounds.fetch_add(1, std::memory_order_relaxed);
      cnt.items.fetch_add(batch->size(), std::memory_order_relaxed);
    }
  }

  // Per-batch time sampling for one serve thread. mark(stage) charges the
  // CPU time since the previous sample to `stage`. Under TBAMD_SERVE_TIMINGS
  // stamp() also takes the batch's wall-clock stage boundaries (microseconds):
  // start, inputs on the host ("cat"), forward enqueued, outputs on the host.
  struct CpuMarks {
    int64_t last = 0;
    int64_t ns[CpuStageCounters::kStages];
    bool timing = false;
    int64_t t0 = 0, t_cat = 0, t_fwd = 0, t_sync = 0;
    void begin() {
      for (auto& v : ns) v = 0;
      last = thread_cpu_ns();
    }
    void mark(int stage) {
      const int64_t now = thread_cpu_ns();
      ns[stage] += now - last;
      last = now;
    }
    void stamp(int64_t& t) {
      if (timing) t = now_us();
    }
  };

  // Persistent staging of one serve thread for row batches: allocated once
  // for the batcher's maximum batch (rounded up to 64), reused every batch.
  // Reuse is safe because a thread serves one batch at a time and every
  // batch ends with a stream synchronise before its fan-out.
  // With device_gather the host side of the inputs is only the pointer
  // table the gather kernel reads ([2, cap] addresses: frames, rewards);
  // h_frames ([cap, fsz] pinned, ~100 MB for full-resolution frames at cap
  // 1024) and h_rew are then not allocated.
  struct RowStaging {
    int64_t cap = 0, fsz = 0, A = 0;
    bool device_gather = false;
    torch::Tensor h_frames, h_rew, d_frames, d_rew;  // inputs
    torch::Tensor h_table;                           // pinned, device gather
    torch::Tensor h_action, h_logits, h_base;        // pinned outputs
    // Recurrent row batches (tail_lstm_rows): the state table ([3, cap]
    // addresses: state in, state out, done byte; pinned), h of every layer
    // ([cap, H] each, device) and this thread's packed LSTM weights, kept
    // until mark_weights_dirty().
    int64_t lstm_cap = 0;
    torch::Tensor h_state_table;
    std::vector<torch::Tensor> d_h;
    torch::Tensor d_state;  // [cap, 2 L H]: the batch's masked old state
    std::vector<LstmLayerPack> lstm_pack;
    int64_t lstm_pack_version = -1;
    std::vector<uintptr_t> table_scratch;
  };

  // What the input stage hands to the trunk and the tail.
  struct ServeInputs {
    int64_t b = 0, bp = 0, C = 0, H = 0, W = 0;
    torch::Tensor frames;   // [bp, C, H, W] u8, device; rows >= b hold some
                            // valid u8 frame
    torch::Tensor rew;      // [bp, 1] f32, clamped to [-1, 1]
    torch::Tensor notdone;  // f32, at least b long; undefined for row batches
    std::vector<torch::Tensor> state;  // [] or h, c [L, b, H]
    TensorNest source;  // the batcher's nest the copies above read from
    bool rows = false;  // outputs go back through RowStaging into the rows
    bool state_rows = false;  // ... and the LSTM state lives in state rows
  };

  // Compute batches are multiples of 64 so kernel/solution caches see a
  // handful of shapes, not every ragged batch size.
  static int64_t pad64(int64_t n) { return (n + 63) / 64 * 64; }

  void ensure_staging(RowStaging& st, int64_t bp,
                      const std::vector<int64_t>& chw, int64_t A,
                      bool device_gather) {
    const int64_t fsz = chw[0] * chw[1] * chw[2];
    if (st.cap >= bp && st.fsz == fsz && st.A == A &&
        st.device_gather == device_gather &&
        st.d_frames.size(1) == chw[0] && st.d_frames.size(2) == chw[1]) {
      return;
    }
    const int64_t want = batcher_->max_batch_size();
    int64_t cap = bp;
    if (want <= 8192) cap = std::max(cap, pad64(want));
    auto hopts = torch::TensorOptions().pinned_memory(true);
    auto dopts = torch::TensorOptions().device(device_);
    if (device_gather) {
      st.h_table = torch::zeros({2, cap}, hopts.dtype(torch::kInt64));
      st.h_frames = torch::Tensor();
      st.h_rew = torch::Tensor();
    } else {
      st.h_frames = torch::empty({cap, fsz}, hopts.dtype(torch::kUInt8));
      st.h_rew = torch::empty({cap}, hopts.dtype(torch::kFloat32));
      st.h_table = torch::Tensor();
    }
    st.device_gather = device_gather;
    // Zero once: pad rows (>= b) are never written again, see
    // inputs_from_rows.
    st.d_frames = torch::zeros({cap, chw[0], chw[1], chw[2]},
                               dopts.dtype(torch::kUInt8));
    st.d_rew = torch::zeros({cap, 1}, dopts.dtype(torch::kFloat32));
    st.h_action = torch::empty({cap}, hopts.dtype(torch::kInt64));
    st.h_logits = torch::empty({cap, A}, hopts.dtype(torch::kFloat32));
    st.h_base = torch::empty({cap}, hopts.dtype(torch::kFloat32));
    st.cap = cap;
    st.fsz = fsz;
    st.A = A;
  }

  // Can this batch take the allocation-free row path? Stateless model with
  // the fused heads, every request a row of the flagship step layout.
  bool rows_servable(const DynamicBatcher::Batch& batch) const {
    if (!batch.all_rows() || !fused_heads_ || legacy_serve_) return false;
    const auto& req = batch.requests()[0];
    return !req.mailbox->has_state_rows() && req.state().empty() &&
           req.layout->is_flagship_step(weights_[head_base_].size(0));
  }

  // The recurrent case: an LSTM model, every request a row of the flagship
  // step layout (with a one-byte done leaf) whose mailbox carries the
  // pool's pinned state block, of the weights' L and H. Anything else (an
  // unpinned block under TBAMD_NO_PIN, for one) goes through get_inputs().
  bool state_rows_servable(const DynamicBatcher::Batch& batch) const {
    if (!batch.all_rows() || !lstm_rows_ || legacy_serve_) return false;
    const auto& reqs = batch.requests();
    const RowLayout& l = *reqs[0].layout;
    if (!l.is_flagship_step(weights_[head_base_].size(0)) ||
        l.leaves[2].dtype != torch::kBool || l.leaves[2].row_bytes != 1) {
      return false;
    }
    const StateBlock* block = reqs[0].mailbox->state_block.get();
    if (block == nullptr || !block->pinned || block->L != num_lstm_layers_ ||
        block->H != weights_[lstm_base_ + 1].size(1)) {
      return false;
    }
    const ActorMailbox* last = nullptr;
    for (const auto& r : reqs) {
      if (r.mailbox.get() == last) continue;
      last = r.mailbox.get();
      if (last->state_block.get() != block) return false;
    }
    return true;
  }

  static void hip_check(hipError_t e, const char* what) {
    TORCH_CHECK(e == hipSuccess, what, ": ", hipGetErrorString(e));
  }

  void trace(const char* what) {
    if (trace_) {
      fprintf(stderr, "[serve %p] %s\n", (void*)this, what);
      fflush(stderr);
    }
  }

  void serve(DynamicBatcher::Batch& batch, at::cuda::CUDAStream& stream,
             RowStaging& staging, CpuMarks& marks) {
    trace("begin");
    marks.stamp(marks.t0);
    ServeInputs in;
    if (rows_servable(batch)) {
      in = inputs_from_rows(batch, stream, staging, marks);
    } else if (state_rows_servable(batch)) {
      in = inputs_from_rows(batch, stream, staging, marks);
      in.state_rows = true;
    } else {
      // nest = ((frame, reward, done, ...), state)  [classic requests]
      //      = (slot_ids, state)                     [obs-slab requests]
      TensorNest nest = batch.get_inputs();
      marks.stamp(marks.t_cat);
      in = nest.vector()[0].is_leaf() ? inputs_from_slots(nest)
                                      : inputs_from_tensors(nest);
      in.source = std::move(nest);
      marks.mark(kServeGather);
    }
    trace("cat-done");
    // Only the MIOpen (deep ResNet) path needs first-serve-per-shape
    // serialization: concurrent solution-finds for a brand-new conv shape
    // across streams have been observed to fault; once found, the solution
    // cache makes later serves safe to run fully in parallel. The
    // hand-written trunk kernels have no such state. Held until the outputs
    // are delivered; the size counts as warmed only if that succeeds.
    const int64_t bq = pad64(batch.size());
    std::unique_lock<std::mutex> warm_lock;
    if (deep_ && !deep_mfma_) {
      bool is_new;
      {
        std::lock_guard<std::mutex> g(warm_mu_);
        is_new = warmed_sizes_.count(bq) == 0;
      }
      if (is_new) warm_lock = std::unique_lock<std::mutex>(serve_mu_);
    }
    torch::Tensor x = trunk(in, stream);
    if (in.state_rows) {
      tail_lstm_rows(batch, in, x, stream, staging, marks);
    } else if (!fused_heads_) {
      tail_generic(batch, in, x, stream, marks);
    } else if (in.rows) {
      tail_fused_rows(batch, in, x, stream, staging, marks);
    } else {
      tail_fused(batch, in, x, stream, marks);
    }
    finish(in, staging, marks, warm_lock.owns_lock() ? bq : 0);
  }

  // ---- input stage ----
  // Row batch: gather each request's frame into the pinned staging (the
  // one host copy before DMA), clamp rewards on the host while at it,
  // then one H2D for frames and one for rewards. No tensor is
  // allocated and no clamp / not / cast / fill kernel runs.
  //
  // Pad rows [b, bp) are NOT zeroed. The trunk convolves each sample
  // on its own, fc is a row-wise GEMM and the heads kernel launches
  // exactly b workgroups, so no row >= b ever reaches an output; and
  // whatever a pad row holds (the zeros it was allocated with, or an
  // older batch's frame) is a valid u8 frame, so nothing non-finite can
  // arise from it either. The same holds for the device gather:
  // its kernel writes rows [0, b) of d_frames / d_rew and nothing else.
  ServeInputs inputs_from_rows(DynamicBatcher::Batch& batch,
                               at::cuda::CUDAStream& stream,
                               RowStaging& staging, CpuMarks& marks) {
    const auto& reqs = batch.requests();
    const RowLayout& l = *reqs[0].layout;
    ServeInputs in;
    in.rows = true;
    in.b = (int64_t)reqs.size();
    in.bp = pad64(in.b);
    in.C = l.leaves[0].shape[2];
    in.H = l.leaves[0].shape[3];
    in.W = l.leaves[0].shape[4];
    const int64_t b = in.b;
    // Device gather: the GPU reads each frame and reward from its row in
    // the pinned rollout slab (large frames, where the host copy below is
    // what bounds the serve thread). Needs host addresses the GPU can
    // read, i.e. a pinned slab.
    const auto& pool = reqs[0].mailbox->slab;
    const bool device_gather =
        (row_gather_ == kRowGatherAuto ? l.device_gather
                                       : row_gather_ == kRowGatherDevice) &&
        pool != nullptr && pool->is_pinned();
    ensure_staging(staging, in.bp, {in.C, in.H, in.W},
                   weights_[head_base_].size(0), device_gather);
    const int64_t fsz = staging.fsz;
    if (device_gather) {
      // One layout per batch means one pool per batch. The table is
      // written only here, and only with addresses checked against the
      // slab: a stray one would be a GPU fault.
      const SlabGeometry slab = pool->geometry();
      int64_t* table = staging.h_table.data_ptr<int64_t>();
      auto** ft = reinterpret_cast<const uint8_t**>(table);
      auto** rt = reinterpret_cast<const float**>(table + staging.cap);
      build_row_table(
          b, [&reqs](int64_t r) { return reqs[r].leaf_ptr(0); },
          [&reqs](int64_t r) { return reqs[r].leaf_ptr(1); }, fsz, slab.base,
          slab.total_bytes, ft, rt);
      marks.mark(kServeGather);
      marks.stamp(marks.t_cat);
      // Rows and table stay as they are until this batch's synchronise:
      // actors rewrite a row only after complete_rows(), the table is
      // this thread's, and loop() synchronises after a failed batch.
      launch_gather_rows(ft, rt, b, fsz, staging.d_frames.data_ptr<uint8_t>(),
                         staging.d_rew.data_ptr<float>());
    } else {
      uint8_t* hf = staging.h_frames.data_ptr<uint8_t>();
      float* hr = staging.h_rew.data_ptr<float>();
      for (int64_t r = 0; r < b; ++r) {
        std::memcpy(hf + r * fsz, reqs[r].leaf_ptr(0), fsz);
        const float v = *reinterpret_cast<const float*>(reqs[r].leaf_ptr(1));
        hr[r] = v < -1.f ? -1.f : (v > 1.f ? 1.f : v);
      }
      marks.mark(kServeGather);
      marks.stamp(marks.t_cat);  // gather is this path's "cat"
      hip_check(hipMemcpyAsync(staging.d_frames.data_ptr(), hf, b * fsz,
                               hipMemcpyHostToDevice, stream.stream()),
                "frame H2D");
      hip_check(hipMemcpyAsync(staging.d_rew.data_ptr(), hr, b * 4,
                               hipMemcpyHostToDevice, stream.stream()),
                "reward H2D");
    }
    in.frames = staging.d_frames.narrow(0, 0, in.bp);
    in.rew = staging.d_rew.narrow(0, 0, in.bp);
    return in;
  }

  // Slot-id requests: gather_obs reads frames, rewards and dones of the
  // named actors from the pinned obs slab and zeroes the pad rows.
  ServeInputs inputs_from_slots(const TensorNest& nest) {
    TORCH_CHECK(has_slab_, "slot-id request but no obs slab configured");
    const torch::Tensor ids = nest.vector()[0].leaf();  // [1, b] int32
    ServeInputs in;
    in.b = ids.size(1);
    in.bp = pad64(in.b);
    in.C = frame_shape_[0];
    in.H = frame_shape_[1];
    in.W = frame_shape_[2];
    auto g = gather_obs(slab_frames_, slab_rew_, slab_done_, ids, in.bp,
                        frame_shape_);
    in.frames = g[0];
    in.rew = g[1];
    in.notdone = g[2];
    in.state = nest.vector()[1].flatten();
    return in;
  }

  // Tensor requests, already cat-ed on the host by the batcher: H2D into a
  // fresh padded batch, pad rows zeroed.
  ServeInputs inputs_from_tensors(const TensorNest& nest) {
    const auto& env = nest.vector()[0].vector();
    const torch::Tensor frame = env[0].leaf();   // [1, b, C, H, W] u8
    const torch::Tensor reward = env[1].leaf();  // [1, b] f32
    const torch::Tensor done = env[2].leaf();    // [1, b] bool
    auto opts = torch::TensorOptions().device(device_);
    ServeInputs in;
    const int64_t b = in.b = frame.size(1);
    const int64_t bp = in.bp = pad64(b);
    in.C = frame.size(2);
    in.H = frame.size(3);
    in.W = frame.size(4);
    in.frames = torch::empty({bp, in.C, in.H, in.W}, opts.dtype(torch::kUInt8));
    in.frames.narrow(0, 0, b).copy_(frame.reshape({b, in.C, in.H, in.W}),
                                    /*non_blocking=*/true);
    if (bp > b) in.frames.narrow(0, b, bp - b).zero_();
    in.rew = torch::empty({bp, 1}, opts.dtype(torch::kFloat32));
    in.rew.narrow(0, 0, b)
        .copy_(reward.to(opts.dtype(torch::kFloat32), true).reshape({b, 1}))
        .clamp_(-1, 1);
    if (bp > b) in.rew.narrow(0, b, bp - b).zero_();
    in.notdone = (~done.reshape({b}))
                     .to(opts.dtype(torch::kFloat32), /*non_blocking=*/true);
    in.state = nest.vector()[1].flatten();
    return in;
  }

  // ---- trunk ----
  // bf16-packed trunk weights (3 tensors shallow, 15 deep), cached until the
  // learner's next sync (mark_weights_dirty). The packing thread
  // synchronizes its stream before publishing so other serve streams read
  // complete data.
  std::vector<torch::Tensor> packed_weights(at::cuda::CUDAStream& stream) {
    std::lock_guard<std::mutex> g(pack_mu_);
    const int64_t v = weights_version_.load();
    if (packed_version_ != v) {
      packed_ = deep_ ? pack_deep() : pack_shallow();
      stream.synchronize();
      packed_version_ = v;
    }
    return packed_;
  }

  std::vector<torch::Tensor> pack_shallow() const {
    return {weights_[0].reshape({32, -1}).to(torch::kBFloat16).contiguous(),
            weights_[2].permute({0, 2, 3, 1}).reshape({64, -1})
                .to(torch::kBFloat16).contiguous(),
            weights_[4].permute({0, 2, 3, 1}).reshape({64, -1})
                .to(torch::kBFloat16).contiguous()};
  }

  std::vector<torch::Tensor> pack_deep() const {
    std::vector<torch::Tensor> packed;
    for (size_t wi = 0; wi < 30; wi += 2) {
      torch::Tensor w = weights_[wi];
      if (wi == 0 && w.size(1) < 8) {  // first conv: pad channels
        w = torch::cat({w, w.new_zeros({w.size(0), 8 - w.size(1), 3, 3})}, 1);
      }
      auto f = w.permute({0, 2, 3, 1}).reshape({w.size(0), -1})
                   .to(torch::kBFloat16);
      const int64_t k = f.size(1), kpad = (k + 31) / 32 * 32 - k;
      if (kpad) f = torch::cat({f, f.new_zeros({f.size(0), kpad})}, 1);
      packed.push_back(f.contiguous());
    }
    return packed;
  }

  // Frames to features to fc: [bp, fc width], post-relu.
  torch::Tensor trunk(const ServeInputs& in, at::cuda::CUDAStream& stream) {
    const int64_t bp = in.bp, C = in.C, H = in.H, W = in.W;
    torch::Tensor x;
    if (deep_ && deep_mfma_ && C <= 8 &&
        ((H == 84 && W == 84) || (resnet_any_ && deep_any_supported(H, W)))) {
      // 84x84 on the template kernels; with TBAMD_RESNET_ANY=1 every other
      // supported frame size on the run-time-geometry ones. No MIOpen runs
      // on either, so neither needs the first-serve lock.
      x = trunk_deep_mfma(in, packed_weights(stream));
    } else if (deep_) {
      x = in.frames.to(torch::kFloat32).mul_(1.0f / 255.0f);
      size_t wi = 0;
      for (int sec = 0; sec < 3; ++sec) {
        x = at::conv2d(x, weights_[wi], weights_[wi + 1], 1, 1);
        wi += 2;
        x = at::max_pool2d(x, 3, 2, 1);
        for (int res = 0; res < 2; ++res) {
          torch::Tensor y = at::conv2d(at::relu(x), weights_[wi],
                                       weights_[wi + 1], 1, 1);
          y = at::conv2d(y.relu_(), weights_[wi + 2], weights_[wi + 3], 1, 1);
          wi += 4;
          x = x + y;
        }
      }
      x = at::relu(x).reshape({bp, -1});
    } else if (!aten_only_ && ((C == 4 && H == 84 && W == 84) ||
                               (C == 3 && H == 210 && W == 160))) {
      // MFMA implicit-GEMM trunk (bf16 operands, fp32 accumulate) — flat
      // per-batch cost at every dynamic batch size, unlike the per-sample
      // fused kernel whose grid is the batch (underfills the 256 CUs below
      // ~512 samples and was measured dominating GPU time at small
      // batches: profiles/PROFILE_r2.md).
      const std::vector<torch::Tensor> wp = packed_weights(stream);
      trace("trunk");
      x = tbamd::conv_trunk_fwd(in.frames, wp[0], weights_[1], wp[1],
                                weights_[3], wp[2], weights_[5],
                                /*want_stash=*/false)[0];
      trace("trunk-done");
    } else if (!aten_only_ && bp <= 384 &&
               tbamd::atari_trunk_supported(C, H, W)) {
      // Hand-written fused CDNA4 conv trunk: one kernel for the u8
      // normalize + 3 convs (non-84x84 geometries).
      x = tbamd::atari_trunk_fwd(in.frames, weights_[0], weights_[1],
                                 weights_[2], weights_[3], weights_[4],
                                 weights_[5], /*save_for_backward=*/false)[0];
    } else {
      x = in.frames.to(torch::kFloat32).mul_(1.0f / 255.0f);
      x = at::conv2d(x, weights_[0], weights_[1], /*stride=*/4).relu_();
      x = at::conv2d(x, weights_[2], weights_[3], 2).relu_();
      x = at::conv2d(x, weights_[4], weights_[5], 1).relu_();
      x = x.reshape({bp, -1});
    }
    return at::linear(x, weights_[head_base_ - 2], weights_[head_base_ - 1])
        .relu_();
  }

  // bf16 channels_last ResNet trunk, every conv on the MFMA template.
  // Every forward conv of the three sections at an (H, W) frame.
  static bool deep_any_supported(int64_t h, int64_t w) {
    const int64_t widths[3] = {16, 32, 32};
    int64_t ci = 8;
    for (int sec = 0; sec < 3; ++sec) {
      if (!tbamd::resnet_conv_any_supported(ci, h, w, widths[sec])) return false;
      h = (h + 1) / 2;
      w = (w + 1) / 2;
      ci = widths[sec];
      if (!tbamd::resnet_conv_any_supported(ci, h, w, ci)) return false;
    }
    return true;
  }

  torch::Tensor trunk_deep_mfma(const ServeInputs& in,
                                const std::vector<torch::Tensor>& wp) {
    auto x8 = torch::empty({in.bp, 8, in.H, in.W},
                           torch::TensorOptions().device(device_).dtype(
                               torch::kBFloat16),
                           torch::MemoryFormat::ChannelsLast);
    x8.zero_();
    x8.narrow(1, 0, in.C).copy_(in.frames, /*non_blocking=*/true);
    x8.mul_(1.0f / 255.0f);
    size_t wi = 0, pi = 0;
    // The template geometries keep their kernels; any other (h, w) runs
    // the run-time-geometry ones (trunk() has checked they are supported).
    auto conv = [&](torch::Tensor t, int64_t ci, int64_t h, int64_t w,
                    int64_t co) {
      auto o = (h == w && tbamd::resnet_conv_supported(ci, h, co))
                   ? tbamd::resnet_conv(t, wp[pi], weights_[wi + 1], ci, h, co,
                                        /*fwd=*/true)
                   : tbamd::resnet_conv_any(
                         t.contiguous(torch::MemoryFormat::ChannelsLast),
                         wp[pi], weights_[wi + 1], /*fwd=*/true);
      ++pi;
      wi += 2;
      return o.permute({0, 3, 1, 2});
    };
    const int64_t widths[3] = {16, 32, 32};
    int64_t h = in.H, w = in.W, ci = 8;
    torch::Tensor t = x8;
    for (int sec = 0; sec < 3; ++sec) {
      t = conv(t, ci, h, w, widths[sec]);
      t = at::max_pool2d(t, 3, 2, 1);
      h = (h + 1) / 2;
      w = (w + 1) / 2;
      ci = widths[sec];
      for (int res = 0; res < 2; ++res) {
        torch::Tensor y = conv(at::relu(t), ci, h, w, ci);
        y = conv(at::relu(y), ci, h, w, ci);
        t = t + y;
      }
    }
    return at::relu(t).to(torch::kFloat32).reshape({in.bp, -1});
  }

  // ---- tails ----
  // The one stream synchronise of a batch: after its last enqueue, before
  // any host read of the outputs and any fan-out.
  void synchronize(at::cuda::CUDAStream& stream, CpuMarks& marks) {
    marks.mark(kServeEnqueue);
    stream.synchronize();
    marks.mark(kServeSyncWait);
  }

  int64_t next_seed() {
    return greedy_
               ? 0
               : (int64_t)(seed_ctr_.fetch_add(1) * 0x9E3779B97F4A7C15ull);
  }

  // Fused heads + Gumbel sample written straight into this thread's pinned
  // staging, scattered into the rows, then each actor thread woken once.
  void tail_fused_rows(DynamicBatcher::Batch& batch, const ServeInputs& in,
                       const torch::Tensor& x, at::cuda::CUDAStream& stream,
                       RowStaging& staging, CpuMarks& marks) {
    const int64_t b = in.b;
    trace("heads");
    fused_heads_sample_out(
        x, in.rew, weights_[head_base_], weights_[head_base_ + 1],
        weights_[head_base_ + 2], weights_[head_base_ + 3], b, greedy_,
        next_seed(), staging.h_action.data_ptr<int64_t>(),
        staging.h_logits.data_ptr<float>(), staging.h_base.data_ptr<float>());
    synchronize(stream, marks);
    scatter_staged_outputs(batch.requests(), staging, b);
    marks.stamp(marks.t_sync);
    batch.complete_rows();
    marks.mark(kServeFanout);
  }

  // The pinned staging's action / logits / baseline into the rows.
  static void scatter_staged_outputs(
      const std::vector<DynamicBatcher::Request>& reqs,
      const RowStaging& staging, int64_t b) {
    const size_t na = reqs[0].layout->n_env;
    const int64_t A = staging.A;
    const int64_t* ha = staging.h_action.data_ptr<int64_t>();
    const float* hl = staging.h_logits.data_ptr<float>();
    const float* hb = staging.h_base.data_ptr<float>();
    // Typed writes: RowLayout::is_flagship_step vouches for the leaves.
    for (int64_t r = 0; r < b; ++r) {
      *reinterpret_cast<int64_t*>(reqs[r].leaf_ptr(na)) = ha[r];
      std::memcpy(reqs[r].leaf_ptr(na + 1), hl + r * A, A * 4);
      *reinterpret_cast<float*>(reqs[r].leaf_ptr(na + 2)) = hb[r];
    }
  }

  // Table, per-layer h and weight pack of the recurrent tail: allocated when
  // the staging's capacity changes, repacked after mark_weights_dirty().
  // Each serve thread packs for itself, on its own stream: stream order
  // alone makes the pack complete before the kernels read it.
  void ensure_lstm_staging(RowStaging& st) {
    const int64_t H = weights_[lstm_base_ + 1].size(1);
    if (st.lstm_cap != st.cap) {
      st.h_state_table = torch::zeros(
          {3, st.cap},
          torch::TensorOptions().dtype(torch::kInt64).pinned_memory(true));
      st.d_state = torch::zeros(
          {st.cap, 2 * num_lstm_layers_ * H},
          torch::TensorOptions().device(device_).dtype(torch::kFloat32));
      st.d_h.clear();
      for (int64_t l = 0; l < num_lstm_layers_; ++l) {
        st.d_h.push_back(torch::zeros(
            {st.cap, H},
            torch::TensorOptions().device(device_).dtype(torch::kFloat32)));
      }
      st.lstm_cap = st.cap;
    }
    const int64_t v = weights_version_.load();
    if (st.lstm_pack_version != v) {
      st.lstm_pack.clear();
      for (int64_t l = 0; l < num_lstm_layers_; ++l) {
        st.lstm_pack.push_back(pack_lstm_layer(
            weights_[lstm_base_ + 4 * l], weights_[lstm_base_ + 4 * l + 1],
            weights_[lstm_base_ + 4 * l + 2],
            weights_[lstm_base_ + 4 * l + 3]));
      }
      st.lstm_pack_version = v;
    }
  }

  // Recurrent row batch: one lstm_serve_layer kernel per layer, reading
  // each request's (h, c) from its stream's current half of the pool's
  // state block and writing the new state into the other half, then the
  // heads on the last layer's h, written into this thread's pinned staging
  // and scattered into the rows. No ATen op, no tensor allocated. The new
  // states are in the block when the synchronise returns; complete_rows()
  // swaps the halves.
  void tail_lstm_rows(DynamicBatcher::Batch& batch, const ServeInputs& in,
                      const torch::Tensor& x, at::cuda::CUDAStream& stream,
                      RowStaging& staging, CpuMarks& marks) {
    const int64_t b = in.b;
    const auto& reqs = batch.requests();
    ensure_lstm_staging(staging);
    const StateBlock& block = *reqs[0].mailbox->state_block;
    const SlabGeometry slab = reqs[0].mailbox->slab->geometry();
    // The table is written only here, and only with checked addresses.
    int64_t* table = staging.h_state_table.data_ptr<int64_t>();
    auto** in_tab = reinterpret_cast<const float**>(table);
    auto** out_tab = reinterpret_cast<float**>(table + staging.cap);
    auto** done_tab =
        reinterpret_cast<const uint8_t**>(table + 2 * staging.cap);
    build_state_table(
        b,
        [&reqs](int64_t r) {
          return reqs[r].mailbox->state_in(reqs[r].env_index);
        },
        [&reqs](int64_t r) {
          return reqs[r].mailbox->state_out(reqs[r].env_index);
        },
        [&reqs](int64_t r) { return reqs[r].leaf_ptr(2); },
        block.half_floats(), block.base(), block.used_bytes(), slab.base,
        slab.total_bytes, staging.table_scratch, in_tab, out_tab, done_tab);
    trace("lstm");
    const int64_t L = num_lstm_layers_;
    const int64_t H = block.H;
    TORCH_CHECK(x.is_contiguous() && x.scalar_type() == torch::kFloat32 &&
                    x.size(0) >= b,
                "lstm tail: trunk output must be contiguous f32 [bp, D]");
    launch_lstm_stage_state(in_tab, done_tab, b, block.half_floats(),
                            staging.d_state.data_ptr<float>());
    for (int64_t l = 0; l < L; ++l) {
      launch_lstm_serve_layer(
          out_tab, staging.d_state.data_ptr<float>(),
          l == 0 ? x.data_ptr<float>() : staging.d_h[l - 1].data_ptr<float>(),
          l == 0 ? x.size(1) : H,
          l == 0 ? in.rew.data_ptr<float>() : nullptr, staging.lstm_pack[l], b,
          l, L, staging.d_h[l].data_ptr<float>());
    }
    launch_heads_sample(
        staging.d_h[L - 1].data_ptr<float>(), nullptr, H,
        weights_[head_base_], weights_[head_base_ + 1],
        weights_[head_base_ + 2], weights_[head_base_ + 3], b, greedy_,
        next_seed(), staging.h_action.data_ptr<int64_t>(),
        staging.h_logits.data_ptr<float>(), staging.h_base.data_ptr<float>());
    marks.stamp(marks.t_fwd);
    synchronize(stream, marks);
    scatter_staged_outputs(reqs, staging, b);
    marks.stamp(marks.t_sync);
    batch.complete_rows();
    marks.mark(kServeFanout);
  }

  // Fused heads + Gumbel sample, written straight into fresh pinned host
  // tensors: replaces cat/2x linear/rand/log/argmax/3x D2H.
  void tail_fused(DynamicBatcher::Batch& batch, const ServeInputs& in,
                  const torch::Tensor& x, at::cuda::CUDAStream& stream,
                  CpuMarks& marks) {
    const int64_t b = in.b;
    trace("heads");
    auto hs = fused_heads_sample(
        x, in.rew, weights_[head_base_], weights_[head_base_ + 1],
        weights_[head_base_ + 2], weights_[head_base_ + 3], b, greedy_,
        next_seed());
    trace("heads-sync");
    synchronize(stream, marks);
    trace("heads-done");
    marks.stamp(marks.t_sync);
    TensorNest::vector_t agent_out{
        TensorNest(hs[0].reshape({1, b})),
        TensorNest(hs[1].reshape({1, b, -1})),
        TensorNest(hs[2].reshape({1, b})),
    };
    batch.set_outputs(TensorNest(TensorNest::vector_t{
        TensorNest(std::move(agent_out)), TensorNest(TensorNest::vector_t{})}));
    marks.mark(kServeFanout);
  }

  // LSTM core (if any), ATen heads, D2H into pinned host tensors.
  void tail_generic(DynamicBatcher::Batch& batch, const ServeInputs& in,
                    const torch::Tensor& x, at::cuda::CUDAStream& stream,
                    CpuMarks& marks) {
    const int64_t b = in.b, bp = in.bp;
    torch::Tensor core = at::cat({x, in.rew}, 1);

    std::vector<torch::Tensor> new_state_gpu;
    if (num_lstm_layers_ > 0) {
      TORCH_CHECK(in.state.size() == 2, "lstm runner needs (h, c) state");
      const int64_t L = in.state[0].size(0);
      const int64_t H = in.state[0].size(2);
      auto opts = torch::TensorOptions().device(device_);
      torch::Tensor nd = in.notdone.narrow(0, 0, b).reshape({1, b, 1});
      auto pad_state = [&](const torch::Tensor& s) {
        torch::Tensor g = torch::zeros({L, bp, H}, opts.dtype(torch::kFloat32));
        g.narrow(1, 0, b).copy_(
            s.to(opts.dtype(torch::kFloat32), true) * nd);
        return g;
      };
      torch::Tensor h = pad_state(in.state[0]);
      torch::Tensor c = pad_state(in.state[1]);
      torch::Tensor layer_in = core;
      std::vector<torch::Tensor> hs, cs;
      for (int64_t l = 0; l < num_lstm_layers_; ++l) {
        const auto& w_ih = weights_[lstm_base_ + 4 * l];
        const auto& w_hh = weights_[lstm_base_ + 4 * l + 1];
        const auto& b_ih = weights_[lstm_base_ + 4 * l + 2];
        const auto& b_hh = weights_[lstm_base_ + 4 * l + 3];
        torch::Tensor gates = at::addmm(b_ih + b_hh, layer_in, w_ih.t())
                                  .addmm_(h[l], w_hh.t());
        auto chunks = gates.chunk(4, 1);
        torch::Tensor ig = at::sigmoid(chunks[0]);
        torch::Tensor fg = at::sigmoid(chunks[1]);
        torch::Tensor gg = at::tanh(chunks[2]);
        torch::Tensor og = at::sigmoid(chunks[3]);
        torch::Tensor c_new = fg * c[l] + ig * gg;
        torch::Tensor h_new = og * at::tanh(c_new);
        hs.push_back(h_new);
        cs.push_back(c_new);
        layer_in = h_new;
      }
      core = layer_in;
      new_state_gpu = {at::stack(hs).narrow(1, 0, b),
                       at::stack(cs).narrow(1, 0, b)};
    }

    torch::Tensor logits =
        at::linear(core, weights_[head_base_], weights_[head_base_ + 1])
            .narrow(0, 0, b);
    torch::Tensor baseline =
        at::linear(core, weights_[head_base_ + 2], weights_[head_base_ + 3])
            .narrow(0, 0, b)
            .reshape({b});
    torch::Tensor action;
    if (greedy_) {
      action = at::argmax(logits, -1);
    } else {
      // Gumbel-argmax categorical sampling: exactly softmax(logits), no
      // host sync, three elementwise kernels (at::multinomial stalls).
      torch::Tensor u = at::rand_like(logits).clamp_(1e-20, 1.0);
      action = at::argmax(logits - at::log(-at::log(u)), -1);
    }

    // D2H into pinned host tensors, one stream sync for the whole batch.
    auto to_host = [&](const torch::Tensor& t) {
      torch::Tensor out = torch::empty(
          t.sizes(), t.options().device(torch::kCPU).pinned_memory(
                         pinned_memory_wanted()));
      out.copy_(t, /*non_blocking=*/true);
      return out;
    };
    marks.stamp(marks.t_fwd);
    torch::Tensor a_h = to_host(action);
    torch::Tensor l_h = to_host(logits);
    torch::Tensor b_h = to_host(baseline);
    TensorNest::vector_t state_out;
    for (const auto& s : new_state_gpu) state_out.emplace_back(to_host(s));
    synchronize(stream, marks);
    marks.stamp(marks.t_sync);

    TensorNest::vector_t agent_out{
        TensorNest(a_h.reshape({1, b})),
        TensorNest(l_h.reshape({1, b, -1})),
        TensorNest(b_h.reshape({1, b})),
    };
    batch.set_outputs(TensorNest(TensorNest::vector_t{
        TensorNest(std::move(agent_out)), TensorNest(std::move(state_out))}));
    marks.mark(kServeFanout);
  }

  // ---- epilogue ----
  // The batch is delivered. `warmed` is its quantized size if it was served
  // under the first-serve lock (still held here), else 0.
  void finish(const ServeInputs& in, const RowStaging& staging,
              const CpuMarks& marks, int64_t warmed) {
    if (in.rows) {
      batcher_->count_row_batch();
      if (staging.device_gather) batcher_->count_device_gather_batch();
      if (in.state_rows) batcher_->count_state_row_batch();
    }
    batches_.fetch_add(1, std::memory_order_relaxed);
    steps_.fetch_add(in.b, std::memory_order_relaxed);
    if (warmed) {
      std::lock_guard<std::mutex> g(warm_mu_);
      warmed_sizes_.insert(warmed);
    }
    if (!serve_timing_) return;
    // The fused tails have no D2H of their own: forward and synchronise are
    // one figure there.
    const int64_t t_fwd = fused_heads_ ? marks.t_sync : marks.t_fwd;
    t_cat_us_.fetch_add(marks.t_cat - marks.t0, std::memory_order_relaxed);
    t_fwd_us_.fetch_add(t_fwd - marks.t_cat, std::memory_order_relaxed);
    t_d2h_us_.fetch_add(marks.t_sync - t_fwd, std::memory_order_relaxed);
    const int64_t n = timed_batches_.fetch_add(1) + 1;
    if (n % 500 != 0) return;
    const double cat = (double)t_cat_us_.load() / n;
    const double fwd = (double)t_fwd_us_.load() / n;
    if (fused_heads_) {
      fprintf(stderr,
              "[serve timings over %lld batches] cat=%.0fus "
              "fwd+sync=%.0fus\n",
              (long long)n, cat, fwd);
    } else {
      fprintf(stderr,
              "[serve timings over %lld batches] cat=%.0fus fwd=%.0fus "
              "d2h+sync=%.0fus\n",
              (long long)n, cat, fwd, (double)t_d2h_us_.load() / n);
    }
  }

  bool has_slab_ = false;
  torch::Tensor slab_frames_, slab_rew_, slab_done_;
  std::vector<int64_t> frame_shape_;
  std::mutex pack_mu_;
  std::vector<torch::Tensor> packed_;  // see packed_weights
  int64_t packed_version_ = -1;
  std::atomic<int64_t> weights_version_{0};
  std::atomic<uint64_t> seed_ctr_{1};
  // Benchmarking: serve everything through library ops (the strategy
  // comparison in scripts/inference_speed_profiling.py).
  const bool aten_only_ = std::getenv("TBAMD_RUNNER_ATEN") != nullptr;
  // TBAMD_RESNET_ANY=1: deep frames other than 84x84 on the MFMA kernels.
  const bool resnet_any_ = [] {
    const char* v = std::getenv("TBAMD_RESNET_ANY");
    return v != nullptr && v[0] == '1' && v[1] == '\0';
  }();
  const bool serve_timing_ = std::getenv("TBAMD_SERVE_TIMINGS") != nullptr;
  const bool trace_ = std::getenv("TBAMD_SERVE_TRACE") != nullptr;
  // TBAMD_ACTOR_FASTPATH=0: tensor serve code only (A/B against rows).
  const bool legacy_serve_ = !actor_fastpath_enabled();
  // TBAMD_ROW_GATHER=host|device forces either gather for every row batch
  // (A/B only). Default: what the pool's layout asks for, i.e. the device
  // gather in obs-slab mode and the host gather otherwise.
  enum RowGather { kRowGatherAuto, kRowGatherHost, kRowGatherDevice };
  const RowGather row_gather_ = [] {
    const char* v = std::getenv("TBAMD_ROW_GATHER");
    if (v == nullptr || *v == '\0') return kRowGatherAuto;
    if (std::string(v) == "host") return kRowGatherHost;
    if (std::string(v) == "device") return kRowGatherDevice;
    throw std::invalid_argument("TBAMD_ROW_GATHER must be host or device");
  }();
  std::atomic<int64_t> t_cat_us_{0}, t_fwd_us_{0}, t_d2h_us_{0};
  std::atomic<int64_t> timed_batches_{0};
  std::mutex warm_mu_;
  std::mutex serve_mu_;
  std::set<int64_t> warmed_sizes_;
  std::shared_ptr<DynamicBatcher> batcher_;
  std::vector<torch::Tensor> weights_;
  const int64_t num_lstm_layers_;
  const bool greedy_;
  bool deep_ = false;
  bool deep_mfma_ = false;    // deep trunk on the MFMA kernels (at 84x84;
                              // any supported size under resnet_any_)
  bool fused_heads_ = false;  // fused heads tail, else LSTM/ATen heads
  bool lstm_rows_ = false;    // LSTM serve kernels fit this model's core
  size_t head_base_ = 8;
  size_t lstm_base_ = 12;
  torch::Device device_ = torch::kCPU;
  std::atomic<bool> running_{false};
  std::atomic<int64_t> batches_{0};
  std::atomic<int64_t> steps_{0};
  std::vector<std::thread> threads_;
};

}  // namespace tbruntime
