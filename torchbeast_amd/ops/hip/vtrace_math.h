// The per-element V-trace arithmetic, shared by vtrace_kernel and
// vtrace_iw_kernel (tbops.hip) and impala_tail_kernel (impala_tail.hip): all
// three call these, so the entry points cannot drift. A clip threshold of
// +inf means "do not clip": fminf(rho, inf) is rho exactly. c is clipped at 1
// regardless, then scaled by lambda (arXiv:1802.01561 Remark 2); lambda = 1
// multiplies exactly.
#pragma once

#include <hip/hip_runtime.h>

__device__ __forceinline__ void vtrace_clip(float log_rho, float clip_rho,
                                            float lambda, float* crho,
                                            float* c) {
  const float rho = __expf(log_rho);
  *crho = fminf(rho, clip_rho);
  *c = lambda * fminf(rho, 1.f);
}

__device__ __forceinline__ float vtrace_delta(float crho, float r, float disc,
                                              float v_next, float v) {
  return crho * (r + disc * v_next - v);
}

__device__ __forceinline__ float vtrace_scan_step(float delta, float disc,
                                                  float c, float acc) {
  return delta + disc * c * acc;
}

__device__ __forceinline__ float vtrace_advantage(float log_rho, float clip_pg,
                                                  float r, float disc,
                                                  float vs_next, float v) {
  const float rho = __expf(log_rho);
  return fminf(rho, clip_pg) * (r + disc * vs_next - v);
}
