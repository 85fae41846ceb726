// bf16 MFMA linear layer for the fc behind the conv trunks (gfx950). See
// linear_mfma.hip for the kernels and linear_plan.h for the work split.
#pragma once

#include <torch/extension.h>

#include <vector>

namespace tbamd {

// M >= 1, N % 64 == 0, K % 32 == 0 (and the grid limits of linear_plan.h).
bool linear_supported(int64_t m, int64_t n, int64_t k);

// w: fp32 [N, K]. Returns {bf16 [N, K] (forward operand), bf16 [K, N] (dgrad
// operand)}, both round-to-nearest-even.
std::vector<torch::Tensor> linear_pack(torch::Tensor w);

// y[M, N] = relu?(x[M, K] . wb[N, K]^T + bias). x, bias, y fp32; x is rounded
// to bf16 while it is staged.
torch::Tensor linear_fwd(torch::Tensor x, torch::Tensor wb, torch::Tensor bias,
                         bool relu);

// dx[M, K] = (dy ⊙ [y > 0]) . W, with W as wt = bf16 [K, N]. dy, y fp32
// [M, N]; mask = false drops the ReLU mask (y is then not read).
torch::Tensor linear_dgrad(torch::Tensor dy, torch::Tensor y, torch::Tensor wt,
                           bool mask);

// {dW [N, K], db [N]} fp32: dW = (dy ⊙ mask)^T . x, db = sum over rows of
// dy ⊙ mask. Both are views of one buffer.
std::vector<torch::Tensor> linear_wgrad(torch::Tensor dy, torch::Tensor y,
                                        torch::Tensor x, bool mask);

}  // namespace tbamd
