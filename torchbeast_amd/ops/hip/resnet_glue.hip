// The deep ResNet's glue between its 3x3 convs (gfx950). Each section of the
// trunk is conv, max-pool 3x3 s2 p1, then two residual blocks of
// (ReLU, conv, ReLU, conv, + skip); behind the last section the features are
// ReLU'd, widened to fp32 and flattened in NCHW order. The convs are MFMA
// kernels (conv_mfma.hip); this file is everything between them, as
// stand-alone memory-bound kernels on bf16 NHWC activations:
//
//   pool_fwd   y = maxpool(x), r = relu(y), idx = winning tap, one pass
//   pool_bwd   dx gathered from g_y + g_r [y > 0]
//   ew_fwd     z = a + s, r = relu(z)         (either half optional)
//   ew_bwd     g_z + g_r [z > 0]
//   flat_fwd   relu, bf16 NHWC -> fp32 NCHW rows
//   flat_bwd   fp32 NCHW rows -> bf16 NHWC, masked by x > 0
//
// Common to all: C in {16, 32}; a lane owns 8 channels of one position, one
// 16-byte vector, and every access to an activation is one such vector
// (vector index = position * C/8 + channel group, 64-bit). Arithmetic is
// fp32 inside the lane and every output is rounded to bf16 (nearest even)
// exactly once. There are no atomics and no workgroup depends on another.
//
// pool_fwd: one workgroup per (sample, band of R output rows). The band's
// min(2R + 1, H) input rows are contiguous in NHWC, so they are staged with
// one linear sweep of 16-byte loads; the nine taps then come from LDS and an
// input row is read from memory once per band (the one halo row between two
// bands twice) instead of 2.25 times. Neighbouring lanes read LDS vectors 2C
// bytes apart for neighbouring ox, which costs a two-way bank conflict on
// the tap reads; the kernel is bound by its three global writes. Padding
// taps are skipped, never read. The running maximum follows max_pool2d on
// the CPU: it starts at -inf with the first tap inside the image, and a tap
// replaces it if it is greater or is a NaN.
//
// pool_bwd: gather, one lane per input vector. Row h lies in window row h/2
// (tap row 1 for even h, 2 for odd h) and, for odd h, in window row
// (h + 1)/2 with tap row 0; columns alike. So at most four windows, each
// compared by tap id: the stored byte is never an address.
//
// flat: a workgroup transposes a tile of 128 positions x C channels of one
// sample through LDS, tile[c][p] in fp32. The NHWC side moves 16-byte
// vectors; the NCHW side moves runs of 128 consecutive floats per channel,
// one float per lane (a sample's rows start at multiples of H*W floats,
// which need not be 16-byte aligned). Rows are padded so that the 8-channel
// scatter of a wave (C/8 channel groups x 64 / (C/8) positions) covers all
// 64 banks once: 8 * stride = 16 (mod 64) for C = 32, 32 (mod 64) for C = 16.

#include <ATen/cuda/CUDAContext.h>
#include <c10/cuda/CUDAGuard.h>
#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include <climits>
#include <cmath>

#include "resnet_glue.h"

namespace tbamd {

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1 << 20;  // grid-stride kernels
constexpr int kFlatTile = 128;       // positions per flatten tile

__device__ __forceinline__ float bf_lo(unsigned int w) {
  return __uint_as_float(w << 16);
}
__device__ __forceinline__ float bf_hi(unsigned int w) {
  return __uint_as_float(w & 0xffff0000u);
}

__device__ __forceinline__ void unpack8(const uint4& v, float f[8]) {
  f[0] = bf_lo(v.x); f[1] = bf_hi(v.x);
  f[2] = bf_lo(v.y); f[3] = bf_hi(v.y);
  f[4] = bf_lo(v.z); f[5] = bf_hi(v.z);
  f[6] = bf_lo(v.w); f[7] = bf_hi(v.w);
}

// fp32 -> bf16 bits, round to nearest even; a NaN stays a quiet NaN.
__device__ __forceinline__ unsigned int bf_round(float f) {
  const unsigned int u = __float_as_uint(f);
  if (f != f) return (u >> 16) | 0x40u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

__device__ __forceinline__ uint4 pack8(const float f[8]) {
  uint4 v;
  v.x = bf_round(f[0]) | (bf_round(f[1]) << 16);
  v.y = bf_round(f[2]) | (bf_round(f[3]) << 16);
  v.z = bf_round(f[4]) | (bf_round(f[5]) << 16);
  v.w = bf_round(f[6]) | (bf_round(f[7]) << 16);
  return v;
}

// relu as ATen has it: a NaN stays.
__device__ __forceinline__ float relu1(float v) {
  return (v > 0.f || v != v) ? v : 0.f;
}

// g_a + g_b * [m > 0] for one vector; a missing operand is a null pointer.
__device__ __forceinline__ void combine8(const uint4* __restrict__ ga,
                                         const uint4* __restrict__ gb,
                                         const uint4* __restrict__ mask,
                                         int64_t i, float g[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) g[j] = 0.f;
  if (ga != nullptr) unpack8(ga[i], g);
  if (gb != nullptr) {
    float b[8], m[8];
    unpack8(gb[i], b);
    unpack8(mask[i], m);
#pragma unroll
    for (int j = 0; j < 8; ++j) g[j] += m[j] > 0.f ? b[j] : 0.f;
  }
}

template <int C>
__global__ void __launch_bounds__(kThreads) glue_pool_fwd_kernel(
    const uint4* __restrict__ x,  // [N,H,W,C/8] vectors
    uint4* __restrict__ y,        // [N,OH,OW,C/8]
    uint4* __restrict__ r,        // [N,OH,OW,C/8]
    uint2* __restrict__ idx,      // [N,OH,OW,C/8] x 8 bytes
    int H, int W, int OH, int OW, int R, int bands) {
  constexpr int CG = C / 8;
  extern __shared__ uint4 stage[];  // [min(2R+1, H)][W][CG]

  const int64_t n = blockIdx.x / bands;
  const int band = blockIdx.x % bands;
  const int oy0 = band * R;
  const int rb = min(R, OH - oy0);
  // Input rows of the band, inside the image: at most 2 rb + 1 of them.
  const int iy0 = max(2 * oy0 - 1, 0);
  const int iy1 = min(2 * (oy0 + rb - 1) + 1, H - 1);
  const int rowv = W * CG;
  const int nstage = (iy1 - iy0 + 1) * rowv;
  const uint4* __restrict__ src = x + (n * H + iy0) * (int64_t)rowv;
  for (int i = threadIdx.x; i < nstage; i += kThreads) stage[i] = src[i];
  __syncthreads();

  const int items = rb * OW * CG;
  for (int i = threadIdx.x; i < items; i += kThreads) {
    const int cg = i % CG;
    const int ox = (i / CG) % OW;
    const int oy = oy0 + i / (CG * OW);
    float m[8];
    unsigned int tap[8];
    // The first tap inside the image: rows and columns -1 are padding.
    const unsigned int first = (oy == 0 ? 3u : 0u) + (ox == 0 ? 1u : 0u);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      m[j] = -INFINITY;
      tap[j] = first;
    }
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = 2 * oy - 1 + ky;
      if (iy < 0 || iy >= H) continue;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = 2 * ox - 1 + kx;
        if (ix < 0 || ix >= W) continue;
        float v[8];
        unpack8(stage[((iy - iy0) * W + ix) * CG + cg], v);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (v[j] > m[j] || v[j] != v[j]) {
            m[j] = v[j];
            tap[j] = ky * 3 + kx;
          }
        }
      }
    }
    float rl[8];
    uint4 yv;  // a bf16 widened and cut back is the same bits
    yv.x = (__float_as_uint(m[0]) >> 16) | (__float_as_uint(m[1]) & 0xffff0000u);
    yv.y = (__float_as_uint(m[2]) >> 16) | (__float_as_uint(m[3]) & 0xffff0000u);
    yv.z = (__float_as_uint(m[4]) >> 16) | (__float_as_uint(m[5]) & 0xffff0000u);
    yv.w = (__float_as_uint(m[6]) >> 16) | (__float_as_uint(m[7]) & 0xffff0000u);
#pragma unroll
    for (int j = 0; j < 8; ++j) rl[j] = relu1(m[j]);
    uint4 rv;
    rv.x = (__float_as_uint(rl[0]) >> 16) | (__float_as_uint(rl[1]) & 0xffff0000u);
    rv.y = (__float_as_uint(rl[2]) >> 16) | (__float_as_uint(rl[3]) & 0xffff0000u);
    rv.z = (__float_as_uint(rl[4]) >> 16) | (__float_as_uint(rl[5]) & 0xffff0000u);
    rv.w = (__float_as_uint(rl[6]) >> 16) | (__float_as_uint(rl[7]) & 0xffff0000u);
    uint2 iv;
    iv.x = tap[0] | (tap[1] << 8) | (tap[2] << 16) | (tap[3] << 24);
    iv.y = tap[4] | (tap[5] << 8) | (tap[6] << 16) | (tap[7] << 24);
    const int64_t o = ((n * OH + oy) * OW + ox) * CG + cg;
    y[o] = yv;
    r[o] = rv;
    idx[o] = iv;
  }
}

template <int C>
__global__ void __launch_bounds__(kThreads) glue_pool_bwd_kernel(
    const uint4* __restrict__ g_y,   // [N,OH,OW,C/8] or null
    const uint4* __restrict__ g_r,   // same, or null
    const uint4* __restrict__ mask,  // y or relu(y); read only with g_r
    const uint2* __restrict__ idx,   // [N,OH,OW,C/8] x 8 bytes
    uint4* __restrict__ dx,          // [N,H,W,C/8]
    int H, int W, int OH, int OW, int64_t total) {
  constexpr int CG = C / 8;
  const int64_t step = (int64_t)gridDim.x * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total;
       i += step) {
    const int cg = (int)(i % CG);
    const int64_t p = i / CG;
    const int w = (int)(p % W);
    const int64_t q = p / W;
    const int h = (int)(q % H);
    const int64_t n = q / H;

    // The windows that hold (h, w) and this position's tap in each.
    const int ny = ((h & 1) && (h >> 1) + 1 < OH) ? 2 : 1;
    const int nx = ((w & 1) && (w >> 1) + 1 < OW) ? 2 : 1;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int a = 0; a < ny; ++a) {
      const int oy = (h >> 1) + a;
      const int ky = a ? 0 : ((h & 1) ? 2 : 1);
      for (int b = 0; b < nx; ++b) {
        const int ox = (w >> 1) + b;
        const int kx = b ? 0 : ((w & 1) ? 2 : 1);
        const unsigned int tap = ky * 3 + kx;
        const int64_t o = ((n * OH + oy) * OW + ox) * CG + cg;
        float g[8];
        combine8(g_y, g_r, mask, o, g);
        const uint2 iv = idx[o];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const unsigned int word = j < 4 ? iv.x : iv.y;
          const unsigned int t = (word >> (8 * (j & 3))) & 0xffu;
          acc[j] += t == tap ? g[j] : 0.f;
        }
      }
    }
    dx[i] = pack8(acc);
  }
}

__global__ void __launch_bounds__(kThreads) glue_ew_fwd_kernel(
    const uint4* __restrict__ a, const uint4* __restrict__ s,  // s may be null
    uint4* __restrict__ z,  // written where s is given
    uint4* __restrict__ r,  // may be null
    int64_t total) {
  const int64_t step = (int64_t)gridDim.x * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total;
       i += step) {
    uint4 zv = a[i];
    float f[8];
    if (s != nullptr) {
      float t[8];
      unpack8(zv, f);
      unpack8(s[i], t);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] += t[j];
      zv = pack8(f);
      z[i] = zv;
    }
    if (r != nullptr) {
      // relu of the rounded sum: exact, so r is rounded once as well.
      unpack8(zv, f);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = relu1(f[j]);
      r[i] = pack8(f);
    }
  }
}

__global__ void __launch_bounds__(kThreads) glue_ew_bwd_kernel(
    const uint4* __restrict__ g_z, const uint4* __restrict__ g_r,
    const uint4* __restrict__ mask, uint4* __restrict__ g, int64_t total) {
  const int64_t step = (int64_t)gridDim.x * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total;
       i += step) {
    float f[8];
    combine8(g_z, g_r, mask, i, f);
    g[i] = pack8(f);
  }
}

template <int C>
constexpr int flat_stride() {
  return kFlatTile + (C == 32 ? 2 : 4);
}

template <int C>
__global__ void __launch_bounds__(kThreads) glue_flat_fwd_kernel(
    const uint4* __restrict__ x,  // [N,HW,C/8]
    float* __restrict__ out,      // [N,C,HW]
    int64_t HW, int tiles) {
  constexpr int CG = C / 8;
  constexpr int LD = flat_stride<C>();
  __shared__ float tile[C * LD];
  const int64_t n = blockIdx.x / tiles;
  const int64_t p0 = (int64_t)(blockIdx.x % tiles) * kFlatTile;
  const int np = HW - p0 < kFlatTile ? (int)(HW - p0) : kFlatTile;

  for (int i = threadIdx.x; i < np * CG; i += kThreads) {
    const int cg = i % CG, p = i / CG;
    float f[8];
    unpack8(x[(n * HW + p0 + p) * CG + cg], f);
#pragma unroll
    for (int j = 0; j < 8; ++j) tile[(cg * 8 + j) * LD + p] = relu1(f[j]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < C * kFlatTile; i += kThreads) {
    const int c = i / kFlatTile, p = i % kFlatTile;
    if (p < np) out[(n * C + c) * HW + p0 + p] = tile[c * LD + p];
  }
}

template <int C>
__global__ void __launch_bounds__(kThreads) glue_flat_bwd_kernel(
    const float* __restrict__ g,  // [N,C,HW]
    const uint4* __restrict__ x,  // [N,HW,C/8]
    uint4* __restrict__ dx,       // [N,HW,C/8]
    int64_t HW, int tiles) {
  constexpr int CG = C / 8;
  constexpr int LD = flat_stride<C>();
  __shared__ float tile[C * LD];
  const int64_t n = blockIdx.x / tiles;
  const int64_t p0 = (int64_t)(blockIdx.x % tiles) * kFlatTile;
  const int np = HW - p0 < kFlatTile ? (int)(HW - p0) : kFlatTile;

  for (int i = threadIdx.x; i < C * kFlatTile; i += kThreads) {
    const int c = i / kFlatTile, p = i % kFlatTile;
    if (p < np) tile[c * LD + p] = g[(n * C + c) * HW + p0 + p];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < np * CG; i += kThreads) {
    const int cg = i % CG, p = i / CG;
    const int64_t o = (n * HW + p0 + p) * CG + cg;
    float m[8], f[8];
    unpack8(x[o], m);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      f[j] = m[j] > 0.f ? tile[(cg * 8 + j) * LD + p] : 0.f;
    dx[o] = pack8(f);
  }
}

// ---- host side -----------------------------------------------------------

// A tensor of the wrong shape, layout or dtype would be an out-of-bounds or
// misaligned access on the device; reject it on the host instead.
void check_act(const torch::Tensor& t, const char* op, const char* name,
               at::ScalarType dtype = torch::kBFloat16) {
  TORCH_CHECK(t.is_cuda(), op, ": ", name, " must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == dtype, op, ": ", name, " must be ", dtype,
              ", got ", t.scalar_type());
  TORCH_CHECK(t.dim() == 4, op, ": ", name, " must be [N, C, H, W], got ",
              t.dim(), " dimensions");
  TORCH_CHECK(t.size(1) == 16 || t.size(1) == 32, op, ": ", name,
              " must have 16 or 32 channels, got C=", t.size(1));
  TORCH_CHECK(t.size(0) >= 1 && t.size(2) >= 1 && t.size(3) >= 1 &&
                  t.size(2) <= INT_MAX && t.size(3) <= INT_MAX,
              op, ": ", name, " has an empty or oversized dimension: ",
              t.sizes());
  TORCH_CHECK(t.is_contiguous(at::MemoryFormat::ChannelsLast), op, ": ", name,
              " must be contiguous in channels_last");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, op, ": ",
              name, " must be 16-byte aligned");
}

// An optional companion of `first`: same device and shape.
void check_like(const std::optional<torch::Tensor>& t,
                const torch::Tensor& first, const char* op, const char* name,
                at::ScalarType dtype = torch::kBFloat16) {
  if (!t.has_value()) return;
  check_act(*t, op, name, dtype);
  TORCH_CHECK(t->device() == first.device(), op, ": ", name, " is on ",
              t->device(), ", expected ", first.device());
  TORCH_CHECK(t->sizes() == first.sizes(), op, ": ", name, " has shape ",
              t->sizes(), ", expected ", first.sizes());
}

const uint4* vec_or_null(const std::optional<torch::Tensor>& t) {
  return t.has_value() ? reinterpret_cast<const uint4*>(t->data_ptr())
                       : nullptr;
}

torch::Tensor empty_act(at::IntArrayRef sizes, const torch::Tensor& like,
                        at::ScalarType dtype = torch::kBFloat16) {
  return torch::empty(sizes, like.options().dtype(dtype).memory_format(
                                 at::MemoryFormat::ChannelsLast));
}

unsigned int stride_grid(int64_t total) {
  const int64_t blocks = (total + kThreads - 1) / kThreads;
  return (unsigned int)(blocks < kMaxBlocks ? blocks : kMaxBlocks);
}

void check_launch(const char* op) {
  const hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, op, ": launch failed: ",
              hipGetErrorString(err));
}

GluePoolPlan pool_plan_or_throw(int64_t n, int64_t h, int64_t w, int64_t c,
                                int device) {
  const auto* prop = at::cuda::getDeviceProperties(device);
  const GluePoolPlan plan = glue_pool_plan(
      n, h, w, c, (int64_t)prop->sharedMemPerBlock, prop->multiProcessorCount);
  TORCH_CHECK(plan.ok && plan.lds <= (int64_t)prop->sharedMemPerBlock,
              "resnet_glue_pool_fwd: x [N=", n, ", C=", c, ", H=", h, ", W=",
              w, "] needs ", (h < 3 ? h : 3) * w * c * 2,
              " bytes of LDS for one output row, the device allows ",
              prop->sharedMemPerBlock,
              " per workgroup (or N * bands exceeds the grid limit)");
  return plan;
}

}  // namespace

std::vector<int64_t> resnet_glue_pool_plan(int64_t n, int64_t h, int64_t w,
                                           int64_t c, int64_t device) {
  const GluePoolPlan plan = pool_plan_or_throw(n, h, w, c, (int)device);
  return {plan.rows, plan.bands, plan.lds};
}

std::vector<torch::Tensor> resnet_glue_pool_fwd(torch::Tensor x) {
  const char* op = "resnet_glue_pool_fwd";
  check_act(x, op, "x");
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int64_t OH = (H + 1) / 2, OW = (W + 1) / 2;
  const GluePoolPlan plan = pool_plan_or_throw(N, H, W, C, x.get_device());

  const at::cuda::CUDAGuard device_guard(x.device());
  auto y = empty_act({N, C, OH, OW}, x);
  auto r = empty_act({N, C, OH, OW}, x);
  auto idx = empty_act({N, C, OH, OW}, x, torch::kUInt8);

  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((unsigned int)(N * plan.bands)),
                       dim3(kThreads), (size_t)plan.lds,
                       at::cuda::getCurrentCUDAStream(),
                       reinterpret_cast<const uint4*>(x.data_ptr()),
                       reinterpret_cast<uint4*>(y.data_ptr()),
                       reinterpret_cast<uint4*>(r.data_ptr()),
                       reinterpret_cast<uint2*>(idx.data_ptr()), (int)H,
                       (int)W, (int)OH, (int)OW, plan.rows, plan.bands);
  };
  if (C == 16) {
    launch(glue_pool_fwd_kernel<16>);
  } else {
    launch(glue_pool_fwd_kernel<32>);
  }
  check_launch(op);
  return {y, r, idx};
}

torch::Tensor resnet_glue_pool_bwd(std::optional<torch::Tensor> g_y,
                                   std::optional<torch::Tensor> g_r,
                                   std::optional<torch::Tensor> y,
                                   torch::Tensor idx, int64_t h, int64_t w) {
  const char* op = "resnet_glue_pool_bwd";
  check_act(idx, op, "idx", torch::kUInt8);
  TORCH_CHECK(g_y.has_value() || g_r.has_value(), op,
              ": g_y and g_r are both missing");
  TORCH_CHECK(!g_r.has_value() || y.has_value(), op,
              ": y is needed with g_r");
  check_like(g_y, idx, op, "g_y");
  check_like(g_r, idx, op, "g_r");
  if (g_r.has_value()) check_like(y, idx, op, "y");
  const int64_t N = idx.size(0), C = idx.size(1);
  const int64_t OH = idx.size(2), OW = idx.size(3);
  TORCH_CHECK(h >= 1 && w >= 1 && h <= INT_MAX && w <= INT_MAX &&
                  (h + 1) / 2 == OH && (w + 1) / 2 == OW, op,
              ": an input of h=", h, ", w=", w, " pools to [",
              (h + 1) / 2, ", ", (w + 1) / 2, "], idx is [", OH, ", ", OW,
              "]");

  const at::cuda::CUDAGuard device_guard(idx.device());
  auto dx = empty_act({N, C, h, w}, idx, torch::kBFloat16);
  const int64_t total = N * h * w * (C / 8);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(stride_grid(total)), dim3(kThreads), 0,
                       at::cuda::getCurrentCUDAStream(), vec_or_null(g_y),
                       vec_or_null(g_r),
                       g_r.has_value() ? vec_or_null(y) : nullptr,
                       reinterpret_cast<const uint2*>(idx.data_ptr()),
                       reinterpret_cast<uint4*>(dx.data_ptr()), (int)h, (int)w,
                       (int)OH, (int)OW, total);
  };
  if (C == 16) {
    launch(glue_pool_bwd_kernel<16>);
  } else {
    launch(glue_pool_bwd_kernel<32>);
  }
  check_launch(op);
  return dx;
}

std::tuple<std::optional<torch::Tensor>, std::optional<torch::Tensor>>
resnet_glue_ew_fwd(torch::Tensor a, std::optional<torch::Tensor> s,
                   bool want_r) {
  const char* op = "resnet_glue_ew_fwd";
  check_act(a, op, "a");
  check_like(s, a, op, "s");
  TORCH_CHECK(s.has_value() || want_r, op,
              ": nothing to do without s and without want_r");

  const at::cuda::CUDAGuard device_guard(a.device());
  std::optional<torch::Tensor> z, r;
  if (s.has_value()) z = torch::empty_like(a);
  if (want_r) r = torch::empty_like(a);
  const int64_t total = a.numel() / 8;
  hipLaunchKernelGGL(
      glue_ew_fwd_kernel, dim3(stride_grid(total)), dim3(kThreads), 0,
      at::cuda::getCurrentCUDAStream(),
      reinterpret_cast<const uint4*>(a.data_ptr()), vec_or_null(s),
      const_cast<uint4*>(vec_or_null(z)), const_cast<uint4*>(vec_or_null(r)),
      total);
  check_launch(op);
  return {z, r};
}

torch::Tensor resnet_glue_ew_bwd(std::optional<torch::Tensor> g_z,
                                 std::optional<torch::Tensor> g_r,
                                 std::optional<torch::Tensor> z) {
  const char* op = "resnet_glue_ew_bwd";
  TORCH_CHECK(g_z.has_value() || g_r.has_value(), op,
              ": g_z and g_r are both missing");
  TORCH_CHECK(!g_r.has_value() || z.has_value(), op,
              ": z is needed with g_r");
  const torch::Tensor& first = g_z.has_value() ? *g_z : *g_r;
  check_act(first, op, g_z.has_value() ? "g_z" : "g_r");
  check_like(g_r, first, op, "g_r");
  if (g_r.has_value()) check_like(z, first, op, "z");

  const at::cuda::CUDAGuard device_guard(first.device());
  auto g = torch::empty_like(first);
  const int64_t total = first.numel() / 8;
  hipLaunchKernelGGL(glue_ew_bwd_kernel, dim3(stride_grid(total)),
                     dim3(kThreads), 0, at::cuda::getCurrentCUDAStream(),
                     vec_or_null(g_z), vec_or_null(g_r),
                     g_r.has_value() ? vec_or_null(z) : nullptr,
                     reinterpret_cast<uint4*>(g.data_ptr()), total);
  check_launch(op);
  return g;
}

namespace {

// Workgroups of the flatten kernels: tiles of kFlatTile positions per sample.
int64_t flat_tiles(int64_t hw) { return (hw + kFlatTile - 1) / kFlatTile; }

}  // namespace

torch::Tensor resnet_glue_flat_fwd(torch::Tensor x) {
  const char* op = "resnet_glue_flat_fwd";
  check_act(x, op, "x");
  const int64_t N = x.size(0), C = x.size(1), HW = x.size(2) * x.size(3);
  const int64_t tiles = flat_tiles(HW);
  TORCH_CHECK(tiles <= INT_MAX && N * tiles <= INT_MAX, op, ": x ", x.sizes(),
              " needs ", N * tiles, " workgroups, the grid allows ", INT_MAX);

  const at::cuda::CUDAGuard device_guard(x.device());
  auto out = torch::empty({N, C * HW}, x.options().dtype(torch::kFloat32));
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((unsigned int)(N * tiles)), dim3(kThreads),
                       0, at::cuda::getCurrentCUDAStream(),
                       reinterpret_cast<const uint4*>(x.data_ptr()),
                       out.data_ptr<float>(), HW, (int)tiles);
  };
  if (C == 16) {
    launch(glue_flat_fwd_kernel<16>);
  } else {
    launch(glue_flat_fwd_kernel<32>);
  }
  check_launch(op);
  return out;
}

torch::Tensor resnet_glue_flat_bwd(torch::Tensor g, torch::Tensor x) {
  const char* op = "resnet_glue_flat_bwd";
  check_act(x, op, "x");
  const int64_t N = x.size(0), C = x.size(1), HW = x.size(2) * x.size(3);
  TORCH_CHECK(g.is_cuda() && g.device() == x.device(), op, ": g is on ",
              g.device(), ", expected ", x.device());
  TORCH_CHECK(g.scalar_type() == torch::kFloat32, op,
              ": g must be float32, got ", g.scalar_type());
  TORCH_CHECK(g.dim() == 2 && g.size(0) == N && g.size(1) == C * HW, op,
              ": g has shape ", g.sizes(), ", expected [", N, ", ", C * HW,
              "]");
  TORCH_CHECK(g.is_contiguous(), op, ": g must be contiguous");
  const int64_t tiles = flat_tiles(HW);
  TORCH_CHECK(tiles <= INT_MAX && N * tiles <= INT_MAX, op, ": x ", x.sizes(),
              " needs ", N * tiles, " workgroups, the grid allows ", INT_MAX);

  const at::cuda::CUDAGuard device_guard(x.device());
  auto dx = torch::empty_like(x);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((unsigned int)(N * tiles)), dim3(kThreads),
                       0, at::cuda::getCurrentCUDAStream(),
                       g.data_ptr<float>(),
                       reinterpret_cast<const uint4*>(x.data_ptr()),
                       reinterpret_cast<uint4*>(dx.data_ptr()), HW, (int)tiles);
  };
  if (C == 16) {
    launch(glue_flat_bwd_kernel<16>);
  } else {
    launch(glue_flat_bwd_kernel<32>);
  }
  check_launch(op);
  return dx;
}

}  // namespace tbamd
