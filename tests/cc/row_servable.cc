// Stand-alone check of RowLayout::is_flagship_step() (queues.h): the layout
// test that lets the C++ runner read a row's reward and write its agent
// outputs through typed pointers. Layouts are built with RowLayout::make from
// CPU tensors. Host code only. Build and run notes: README_row_servable.md.

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

#define REQUIRE(cond)                                                 \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "%s:%d: REQUIRE failed: %s\n", __FILE__,   \
                   __LINE__, #cond);                                  \
      std::exit(1);                                                   \
    }                                                                 \
  } while (0)

namespace {

constexpr int64_t kA = 6;

TensorNest nest_of(const std::vector<torch::Tensor>& leaves) {
  TensorNest::vector_t v;
  for (const auto& t : leaves) v.emplace_back(t);
  return TensorNest(std::move(v));
}

// One step of the flagship env: frame, reward, done, episode_step,
// episode_return.
std::vector<torch::Tensor> flagship_env() {
  return {torch::zeros({1, 1, 4, 84, 84}, torch::kUInt8),
          torch::zeros({1, 1}, torch::kFloat32),
          torch::zeros({1, 1}, torch::kBool),
          torch::zeros({1, 1}, torch::kInt32),
          torch::zeros({1, 1}, torch::kFloat32)};
}

// action, policy logits, baseline.
std::vector<torch::Tensor> flagship_agent() {
  return {torch::zeros({1, 1}, torch::kInt64),
          torch::zeros({1, 1, kA}, torch::kFloat32),
          torch::zeros({1, 1}, torch::kFloat32)};
}

bool accepted(const std::vector<torch::Tensor>& env,
              const std::vector<torch::Tensor>& agent, int64_t A = kA) {
  return RowLayout::make(nest_of(env), nest_of(agent), /*rows=*/5)
      ->is_flagship_step(A);
}

}  // namespace

int main() {
  REQUIRE(accepted(flagship_env(), flagship_agent()));
  {  // the minimum: three env leaves, and another frame geometry
    auto env = flagship_env();
    env.resize(3);
    env[0] = torch::zeros({1, 1, 3, 210, 160}, torch::kUInt8);
    REQUIRE(accepted(env, flagship_agent()));
  }
  {  // frame not u8
    auto env = flagship_env();
    env[0] = torch::zeros({1, 1, 4, 84, 84}, torch::kFloat32);
    REQUIRE(!accepted(env, flagship_agent()));
  }
  {  // frame not 5-D
    auto env = flagship_env();
    env[0] = torch::zeros({1, 1, 4 * 84 * 84}, torch::kUInt8);
    REQUIRE(!accepted(env, flagship_agent()));
  }
  {  // reward f64
    auto env = flagship_env();
    env[1] = torch::zeros({1, 1}, torch::kFloat64);
    REQUIRE(!accepted(env, flagship_agent()));
  }
  {  // action i32
    auto agent = flagship_agent();
    agent[0] = torch::zeros({1, 1}, torch::kInt32);
    REQUIRE(!accepted(flagship_env(), agent));
  }
  {  // logits width not equal to A, from either side
    auto agent = flagship_agent();
    agent[1] = torch::zeros({1, 1, kA + 1}, torch::kFloat32);
    REQUIRE(!accepted(flagship_env(), agent));
    REQUIRE(!accepted(flagship_env(), flagship_agent(), kA - 1));
  }
  {  // a fourth agent leaf
    auto agent = flagship_agent();
    agent.push_back(torch::zeros({1, 1}, torch::kFloat32));
    REQUIRE(!accepted(flagship_env(), agent));
  }
  {  // fewer than three env leaves
    auto env = flagship_env();
    env.resize(2);
    REQUIRE(!accepted(env, flagship_agent()));
  }
  std::printf("row_servable ok\nALL OK\n");
  return 0;
}
