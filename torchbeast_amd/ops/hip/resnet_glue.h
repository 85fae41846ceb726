// The deep ResNet's glue between its 3x3 convs (gfx950): max-pool 3x3 s2 p1
// with the ReLU behind it, ReLU / skip add / add + ReLU, and the trunk's exit
// (ReLU, fp32, NCHW flatten), each with its backward. See resnet_glue.hip.
//
// Every activation is a 4-D bf16 tensor of logical shape [N, C, H, W] that is
// contiguous in channels_last (memory order N, H, W, C), C in {16, 32}, with
// a 16-byte aligned base. Results are allocated the same way.
#pragma once

#include <torch/extension.h>

#include <cstdint>
#include <optional>
#include <tuple>
#include <vector>

namespace tbamd {

// Band plan of the pool forward. A workgroup pools `rows` output rows of one
// sample from min(2 rows + 1, H) input rows staged in LDS. `rows` is the
// largest count whose stage fits half of the device's LDS per workgroup (so
// that two workgroups share a CU), the whole of it if even one output row
// needs more; it is then lowered while the grid is below two workgroups per
// CU. Fewer bands mean fewer halo rows read twice.
struct GluePoolPlan {
  bool ok = false;
  int rows = 0;     // output rows per band (R); the last band may be short
  int bands = 0;    // ceil(OH / rows)
  int64_t lds = 0;  // bytes of LDS per workgroup
};

inline GluePoolPlan glue_pool_plan(int64_t n, int64_t h, int64_t w, int64_t c,
                                   int64_t lds_limit, int64_t cus) {
  GluePoolPlan p;
  if (n < 1 || h < 1 || w < 1 || (c != 16 && c != 32) || lds_limit < 1 ||
      cus < 1 || w > lds_limit || h > INT32_MAX)
    return p;
  const int64_t oh = (h + 1) / 2;
  const int64_t row = w * c * 2;  // bytes of one input row
  const int64_t least = (h < 3 ? h : 3) * row;  // one output row's stage
  const int64_t budget = least <= lds_limit / 2 ? lds_limit / 2 : lds_limit;
  if (least > budget) return p;
  const int64_t fit = budget / row;  // input rows that fit, >= min(3, h)
  int64_t r = fit >= h ? oh : (fit - 1) / 2;
  while (r > 1 && n * ((oh + r - 1) / r) < 2 * cus) --r;
  const int64_t bands = (oh + r - 1) / r;
  if (n * bands > INT32_MAX) return p;
  const int64_t staged = 2 * r + 1 < h ? 2 * r + 1 : h;
  p.rows = (int)r;
  p.bands = (int)bands;
  p.lds = staged * row;
  p.ok = true;
  return p;
}

// {rows, bands, lds bytes} of the plan on x's device for an [n, c, h, w]
// input; throws where the pool cannot run.
std::vector<int64_t> resnet_glue_pool_plan(int64_t n, int64_t h, int64_t w,
                                           int64_t c, int64_t device);

// x [N,C,H,W] -> {y [N,C,OH,OW] = maxpool3x3 s2 p1 (x), r = relu(y),
// idx uint8 [N,C,OH,OW]: the winning tap ky * 3 + kx}. OH = ceil(H / 2).
std::vector<torch::Tensor> resnet_glue_pool_fwd(torch::Tensor x);

// dx [N,C,H,W] of the pool for g = g_y + g_r * [y > 0]. Either gradient may
// be missing (zero); y is read only with g_r and only for its sign, so
// relu(y) serves as well.
torch::Tensor resnet_glue_pool_bwd(std::optional<torch::Tensor> g_y,
                                   std::optional<torch::Tensor> g_r,
                                   std::optional<torch::Tensor> y,
                                   torch::Tensor idx, int64_t h, int64_t w);

// (z, r): z = a + s where s is given, r = relu(z) (relu(a) without s) where
// want_r. What was not asked for is None; s or want_r must be given.
std::tuple<std::optional<torch::Tensor>, std::optional<torch::Tensor>>
resnet_glue_ew_fwd(torch::Tensor a, std::optional<torch::Tensor> s,
                   bool want_r);

// g_z + g_r * [z > 0]: the gradient of a and of s alike. z (or relu(z)) is
// read only with g_r.
torch::Tensor resnet_glue_ew_bwd(std::optional<torch::Tensor> g_z,
                                 std::optional<torch::Tensor> g_r,
                                 std::optional<torch::Tensor> z);

// x [N,C,H,W] bf16 channels_last -> fp32 [N, C*H*W] in NCHW order, ReLU
// applied.
torch::Tensor resnet_glue_flat_fwd(torch::Tensor x);

// g fp32 [N, C*H*W] -> bf16 channels_last [N,C,H,W], zero where x <= 0.
torch::Tensor resnet_glue_flat_bwd(torch::Tensor g, torch::Tensor x);

}  // namespace tbamd
