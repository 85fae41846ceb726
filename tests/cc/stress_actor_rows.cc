// Stand-alone stress of the actor fast path (rollout rows written in place,
// row requests, completion mailboxes, slab-slot recycling): a real ActorPool
// over 64 native synthetic envs, 8 per thread, served by 4 C++ consumer
// threads, drained by a learner thread in batches of 8 rollouts.
//
// CPU only; built like stress_queues.cc (plain, -fsanitize=thread,
// -fsanitize=address), see tests/cc/README.md.
//
// Checks
//  - ownership: a synthetic env's frame is a function of its seed and step
//    count alone, so every row names the stream that wrote it. Each dequeued
//    rollout must be T+1 consecutive steps of ONE stream -- the frames are
//    the per-slot owner canary: written by the owner from acquire on,
//    verified at dequeue. A slot handed to two streams mixes rows and fails.
//  - continuity: each stream's rollouts arrive in order, overlapping by
//    exactly one step.
//  - the recorded agent outputs are the policy's answer to the row.
//  - slot accounting and a clean close.

#include <torch/torch.h>

#include <atomic>
#include <cstdio>
#include <future>
#include <thread>
#include <vector>

#if __has_include("actor_pool_hip.h")
#include "actor_pool_hip.h"
#else
#include "actor_pool.h"
#endif

using tbruntime::ActorPool;
using tbruntime::BatchingQueue;
using tbruntime::ClosedQueue;
using tbruntime::DynamicBatcher;
using tbruntime::TensorNest;

static std::atomic<int> failures{0};
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      std::fprintf(stderr, "EXPECT failed: %s (%s:%d)\n", #cond,  \
                   __FILE__, __LINE__);                           \
      failures.fetch_add(1);                                      \
    }                                                             \
  } while (0)

constexpr int kEnvs = 64;
constexpr int kPerThread = 8;
constexpr int kUnroll = 4;
constexpr int kEpisode = 10;
constexpr int kRolloutsPerStream = 12;
constexpr int kSteps = kUnroll * (kRolloutsPerStream + 4) + 2;

// Frame bytes 0 and 1 of env `e` (0-based, seed e + 1) at step k; mirrors
// NativeSyntheticEnv (xorshift state, independent of the actions).
static std::vector<std::vector<uint16_t>> expected_frames() {
  std::vector<std::vector<uint16_t>> out(kEnvs);
  for (int e = 0; e < kEnvs; ++e) {
    uint64_t s = (uint64_t)(e + 1) * 2654435761ull + 1;
    for (int k = 0; k < kSteps; ++k) {
      if (k > 0) {
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
      }
      const uint8_t low = s & 0xFF, x = (s >> 8) & 0xFF;
      out[e].push_back((uint16_t)(((low ^ x) & 0xFF) << 8 | low));
    }
  }
  return out;
}

static int64_t policy_action(int f0, int es) { return (f0 + es) % 3; }
static float policy_baseline(int f0, int f1) { return (f0 - f1) / 255.f; }

// One consumer: rows are answered in place when the whole batch is rows
// (every other such batch goes through get_inputs/set_outputs instead, the
// generic surface), nest requests through get_inputs/set_outputs.
static void consumer(std::shared_ptr<DynamicBatcher> batcher, int id) {
  int n = id;
  try {
    for (;;) {
      auto batch = batcher->get_batch();
      if (batch->all_rows() && (++n % 2 == 0)) {
        for (const auto& r : batch->requests()) {
          const size_t na = r.layout->n_env;
          const uint8_t* f = r.leaf_ptr(0);
          const int es = *reinterpret_cast<const int32_t*>(r.leaf_ptr(3));
          *reinterpret_cast<int64_t*>(r.leaf_ptr(na)) = policy_action(f[0], es);
          float* lg = reinterpret_cast<float*>(r.leaf_ptr(na + 1));
          lg[0] = f[0] / 255.f;
          lg[1] = f[1] / 255.f;
          lg[2] = es / 255.f;
          *reinterpret_cast<float*>(r.leaf_ptr(na + 2)) =
              policy_baseline(f[0], f[1]);
        }
        batch->complete_rows();
        continue;
      }
      TensorNest in = batch->get_inputs();
      const auto& env = in.vector()[0].vector();
      const torch::Tensor frame = env[0].leaf();
      const int64_t b = frame.size(1);
      torch::Tensor f = frame.reshape({b, -1});
      torch::Tensor f0 = f.select(1, 0).to(torch::kInt64);
      torch::Tensor f1 = f.select(1, 1).to(torch::kInt64);
      torch::Tensor es = env[3].leaf().reshape({b}).to(torch::kInt64);
      torch::Tensor action = ((f0 + es) % 3).reshape({1, b});
      torch::Tensor logits =
          (torch::stack({f0, f1, es}, -1).to(torch::kFloat32) / 255.f)
              .reshape({1, b, 3});
      torch::Tensor baseline =
          ((f0 - f1).to(torch::kFloat32) / 255.f).reshape({1, b});
      batch->set_outputs(TensorNest(TensorNest::vector_t{
          TensorNest(TensorNest::vector_t{TensorNest(action),
                                          TensorNest(logits),
                                          TensorNest(baseline)}),
          in.vector()[1]}));
    }
  } catch (const ClosedQueue&) {
  }
}

int main() {
  auto learner_queue = std::make_shared<BatchingQueue>(
      /*batch_dim=*/1, /*min=*/8, /*max=*/8, /*timeout_ms=*/std::nullopt,
      /*check_inputs=*/true, /*max_queue=*/16);
  auto batcher = std::make_shared<DynamicBatcher>(
      /*batch_dim=*/1, /*min=*/1, /*max=*/32, /*timeout_ms=*/1);
  std::vector<std::string> addresses(
      kEnvs, "synthetic:1x8x16:3:" + std::to_string(kEpisode));
  ActorPool pool(kUnroll, learner_queue, batcher, addresses,
                 TensorNest(TensorNest::vector_t{}), /*seed_base=*/0,
                 /*use_obs_slab=*/false, /*rollout_budget_mb=*/1, kPerThread);

  auto pool_done = std::async(std::launch::async, [&] { pool.run(); });
  std::vector<std::thread> consumers;
  for (int c = 0; c < 4; ++c) consumers.emplace_back(consumer, batcher, c);

  const auto frames = expected_frames();
  std::vector<int> next_step(kEnvs, 0);  // step of each stream's next row 0
  std::vector<int> got(kEnvs, 0);
  int64_t rollouts = 0;
  std::thread learner([&] {
    try {
      for (;;) {
        auto [batch, n] = learner_queue->dequeue_many();
        EXPECT(n == 8);
        std::vector<torch::Tensor> leaves = batch.flatten();
        EXPECT(leaves.size() == 8);
        const torch::Tensor& frame = leaves[0];  // [T+1, 8, 1, 8, 16]
        EXPECT(frame.size(0) == kUnroll + 1 && frame.size(1) == 8);
        auto fr = frame.reshape({kUnroll + 1, 8, -1});
        for (int64_t col = 0; col < 8; ++col) {
          uint16_t sig[kUnroll + 1];
          for (int t = 0; t <= kUnroll; ++t) {
            const int f0 = fr[t][col][0].item<uint8_t>();
            const int f1 = fr[t][col][1].item<uint8_t>();
            sig[t] = (uint16_t)(f0 << 8 | f1);
            const int es = leaves[3][t][col].item<int32_t>();
            EXPECT(leaves[5][t][col].item<int64_t>() ==
                   policy_action(f0, es));
            EXPECT(leaves[7][t][col].item<float>() ==
                   policy_baseline(f0, f1));
            EXPECT(leaves[6][t][col][2].item<float>() == es / 255.f);
          }
          // The one stream whose next rollout this is.
          int owner = -1, owners = 0;
          for (int e = 0; e < kEnvs; ++e) {
            const int k = next_step[e];
            if (k + kUnroll >= kSteps) continue;
            bool match = true;
            for (int t = 0; t <= kUnroll && match; ++t) {
              match = frames[e][k + t] == sig[t];
            }
            if (match) {
              owner = e;
              ++owners;
            }
          }
          EXPECT(owners == 1);
          if (owners == 1) {
            const int k = next_step[owner];
            for (int t = 0; t <= kUnroll; ++t) {
              const int step = k + t;
              const int es = leaves[3][t][col].item<int32_t>();
              const bool done = leaves[2][t][col].item<bool>();
              const int want =
                  step == 0 ? 0 : (step - 1) % kEpisode + 1;
              EXPECT(es == want);
              EXPECT(done == (step == 0 || want == kEpisode));
            }
            next_step[owner] += kUnroll;
            ++got[owner];
          }
          ++rollouts;
        }
        bool all = true;
        for (int e = 0; e < kEnvs; ++e) all = all && got[e] >= kRolloutsPerStream;
        if (all) return;
        for (int e = 0; e < kEnvs; ++e) {
          if (next_step[e] + 2 * kUnroll >= kSteps) return;  // table exhausted
        }
      }
    } catch (const ClosedQueue&) {
      EXPECT(false && "learner queue closed early");
    }
  });
  learner.join();
  for (int e = 0; e < kEnvs; ++e) EXPECT(got[e] >= 1);

  auto st = learner_queue->stats();
  EXPECT(st["slab_free"] + st["slab_pending"] + st["slab_held"] ==
         st["slab_slots"]);
  EXPECT(st["slab_held"] >= kEnvs);
  EXPECT(st["slab_slots"] >= kEnvs + 16 + 2 * 8);

  batcher->close();
  learner_queue->close();
  const bool unwound = pool_done.wait_for(std::chrono::seconds(10)) ==
                       std::future_status::ready;
  EXPECT(unwound);
  if (!unwound) {
    std::fprintf(stderr, "actor pool did not unwind; aborting\n");
    std::_Exit(2);
  }
  try {
    pool_done.get();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "pool.run() threw: %s\n", e.what());
    failures.fetch_add(1);
  }
  for (auto& t : consumers) t.join();

  if (failures.load() != 0) {
    std::fprintf(stderr, "%d FAILURES\n", failures.load());
    return 1;
  }
  std::printf(
      "actor_rows stress ok (%lld rollouts, %d slots, %d backpressure "
      "waits)\nALL OK\n",
      (long long)rollouts, (int)st["slab_slots"],
      (int)st["slab_backpressure_waits"]);
  return 0;
}
