// Persistent done-masked LSTM unroll with the gate GEMMs on bf16 MFMA for
// batches up to 256 (gfx950). Same contract as lstm_gate_fwd_launch /
// lstm_gate_bwd_launch of lstm_gate_mfma.h and so of lstm4: same inputs, same
// stash [gates, hm, cm, c], same outputs. See lstm_gate_wide.hip for the
// kernels and lstm_gate_wide_plan.h for the work split.
#pragma once

#include <torch/extension.h>

#include <vector>

namespace tbamd {

// 1 <= B <= 256 and 1 <= H <= 1024.
bool lstm_gate_wide_supported(int64_t b, int64_t h);

// precomp [T,B,4H], w_hh_bf bf16 [4H,H], notdone [T,B], h0/c0 [B,H];
// out, hm, cm, c_stash [T,B,H], gates [T,B,4H], hT/cT [B,H] are written.
void lstm_gate_wide_fwd_launch(torch::Tensor precomp, torch::Tensor w_hh_bf,
                               torch::Tensor notdone, torch::Tensor h0,
                               torch::Tensor c0, torch::Tensor out,
                               torch::Tensor gates, torch::Tensor hm,
                               torch::Tensor cm, torch::Tensor c_stash,
                               torch::Tensor hT, torch::Tensor cT);

// w_hh_bf is bf16 [4H,H] as in the forward (no transposed copy); dgates
// [T,B,4H] (pre-activation grads), dh_out/dc_out [B,H] are written.
void lstm_gate_wide_bwd_launch(torch::Tensor gates, torch::Tensor cm,
                               torch::Tensor c_stash, torch::Tensor w_hh_bf,
                               torch::Tensor notdone, torch::Tensor d_out,
                               torch::Tensor d_hT, torch::Tensor d_cT,
                               torch::Tensor dgates, torch::Tensor dh_out,
                               torch::Tensor dc_out);

// One layer, fp32 w_hh [4H,H] (rounded to bf16 here):
// {out, hT, cT, gates, hm, cm, c}.
std::vector<torch::Tensor> lstm_gate_wide_fwd(torch::Tensor precomp,
                                              torch::Tensor w_hh,
                                              torch::Tensor notdone,
                                              torch::Tensor h0,
                                              torch::Tensor c0);

// {dgates, dh0, dc0}.
std::vector<torch::Tensor> lstm_gate_wide_bwd(
    torch::Tensor gates, torch::Tensor cm, torch::Tensor c_stash,
    torch::Tensor w_hh, torch::Tensor notdone, torch::Tensor d_out,
    torch::Tensor d_hT, torch::Tensor d_cT);

}  // namespace tbamd
