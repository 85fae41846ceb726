// bf16 MFMA input projection of the learner LSTM and its gradients (gfx950).
// See lstm_proj_mfma.hip for the kernels and lstm_proj_plan.h for the work
// split. M = T * B rows, I input columns, H hidden units; any M, I, H >= 1.
#pragma once

#include <torch/extension.h>

#include <vector>

namespace tbamd {

bool lstm_proj_supported(int64_t m, int64_t i, int64_t h);

// w_ih: fp32 [4H, I]. Returns {wb = bf16 [4H, Ip] (forward operand), wt =
// bf16 [I, Np] (dgrad operand)}, round-to-nearest-even, Ip and Np being I and
// 4H rounded up to 32 and the padding zeros.
std::vector<torch::Tensor> lstm_proj_pack(torch::Tensor w_ih);

// precomp[M, 4H] = in[M, I] . wb^T + (b_ih + b_hh). in is rounded to bf16
// while it is staged.
torch::Tensor lstm_proj_fwd(torch::Tensor in, torch::Tensor wb,
                            torch::Tensor b_ih, torch::Tensor b_hh);

// dx[M, I] = dg[M, 4H] . W_ih, with W_ih as wt.
torch::Tensor lstm_proj_dgrad(torch::Tensor dg, torch::Tensor wt, int64_t i);

// {dW_ih [4H, I], dW_hh [4H, H], db [4H]} fp32 from one launch: dg^T . in,
// dg^T . hm and the column sums of dg. All three are views of one buffer.
std::vector<torch::Tensor> lstm_proj_wgrad(torch::Tensor dg, torch::Tensor in,
                                           torch::Tensor hm);

}  // namespace tbamd
