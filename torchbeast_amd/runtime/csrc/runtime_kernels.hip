// GPU kernels for the C++ inference engine (gfx950).
//
// gather_obs: zero-copy assembly of an inference batch straight from the
// actors' pinned observation slab. Actors write frame/reward/done into
// their own slot (host, pinned); requests carry only the 4-byte slot id;
// this kernel reads the slab over the host link and materializes the
// batched GPU tensors in one launch. Replaces the per-request host-side
// nest cat + pageable H2D copy that dominated serve latency
// (profiles/PROFILE_r2.md: cat ~3.7 ms/batch at batch ~100).
//
// fused_heads_sample: fc-output [bp,512] + clipped reward -> policy
// logits, baseline and a Gumbel-argmax action sample in ONE kernel,
// writing results directly into pinned host output buffers (no separate
// D2H copies). Replaces ~12 ATen ops per serve.
//
// unpack_rollouts: the learner queue's batch assembly. B rollout slots are
// DMAed whole into a staging buffer; this kernel transposes them into the
// [T+1, B, ...] leaves in one launch (rollout_gather.h has the layout).
//
// gather_rows: the inference batch of the row form in obs-slab mode (large
// frames). Requests are rows of the pinned rollout slab; the kernel reads a
// pinned table of row addresses (row_gather.h) and copies frames and clamped
// rewards over the host link into the serve thread's device staging, so no
// frame is copied on the host at all.
//
// lstm_serve_layer: the recurrent tail of a row batch. One bf16 MFMA kernel
// per LSTM layer computes the gates and the cell update for the whole batch,
// reading each request's (h, c) from the pool's pinned state rows and
// writing the new state back there; the heads kernel then takes the last
// layer's h as its core. Replaces ~40 ATen launches and the state's D2H
// copies per batch of a two-layer core.

#include <ATen/cuda/CUDAContext.h>
#include <c10/cuda/CUDAGuard.h>
#include <hip/hip_runtime.h>
#include <hiprand/hiprand_kernel.h>
#include <torch/extension.h>

#include <tuple>
#include <vector>

#include "runtime_kernels.h"

namespace tbruntime {

namespace {

__global__ void gather_obs_kernel(
    const uint8_t* __restrict__ slab_frames,  // host pinned [A, fsz]
    const float* __restrict__ slab_rew,       // host pinned [A]
    const uint8_t* __restrict__ slab_done,    // host pinned [A]
    const int* __restrict__ ids,              // device [b]
    int b, int bp, int fsz,
    uint8_t* __restrict__ out_frames,  // [bp, fsz]
    float* __restrict__ out_rew,       // [bp, 1] clamped to [-1, 1]
    float* __restrict__ out_nd) {      // [bp] 1 - done
  const int s = blockIdx.x;
  if (s >= bp) return;
  uint8_t* dst = out_frames + (int64_t)s * fsz;
  if (s >= b) {
    for (int i = threadIdx.x * 16; i < fsz; i += blockDim.x * 16) {
      *reinterpret_cast<uint4*>(dst + i) = uint4{0, 0, 0, 0};
    }
    if (threadIdx.x == 0) {
      out_rew[s] = 0.f;
      out_nd[s] = 1.f;
    }
    return;
  }
  const uint8_t* src = slab_frames + (int64_t)ids[s] * fsz;
  for (int i = threadIdx.x * 16; i < fsz; i += blockDim.x * 16) {
    *reinterpret_cast<uint4*>(dst + i) = *reinterpret_cast<const uint4*>(src + i);
  }
  if (threadIdx.x == 0) {
    const float r = slab_rew[ids[s]];
    out_rew[s] = r < -1.f ? -1.f : (r > 1.f ? 1.f : r);
    out_nd[s] = slab_done[ids[s]] ? 0.f : 1.f;
  }
}

// One workgroup per sample; the core vector is staged in LDS, then each wave
// computes head dot products. The core is [x, rew] (length D+1, the
// stateless model) or, with rew == nullptr, x alone (length D: the last
// LSTM layer's h of the recurrent tail).
__global__ __launch_bounds__(256) void heads_sample_kernel(
    const float* __restrict__ x,         // [bp, D] fc output (post-relu) or h
    const float* __restrict__ rew,       // [bp, 1] or nullptr
    const float* __restrict__ policy_w,  // [A, Dc]
    const float* __restrict__ policy_b,  // [A]
    const float* __restrict__ base_w,    // [1, Dc]
    const float* __restrict__ base_b,    // [1]
    int b, int D, int A, uint64_t seed, int greedy,
    int64_t* __restrict__ out_action,  // host pinned [b]
    float* __restrict__ out_logits,    // host pinned [b, A]
    float* __restrict__ out_base) {    // host pinned [b]
  const int s = blockIdx.x;
  if (s >= b) return;
  extern __shared__ float s_core[];  // [Dc]
  const int Dc = rew != nullptr ? D + 1 : D;
  for (int i = threadIdx.x; i < D; i += blockDim.x) {
    s_core[i] = x[(int64_t)s * D + i];
  }
  if (rew != nullptr && threadIdx.x == 0) s_core[D] = rew[s];
  __syncthreads();

  // One lane group per output row (A logits + 1 baseline): wave-strided
  // dot products, then lane-0 reduction via shuffles.
  __shared__ float s_logits[64];  // A <= 64
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int nwaves = blockDim.x >> 6;
  for (int row = wave; row <= A; row += nwaves) {
    const float* w = (row < A) ? policy_w + (int64_t)row * Dc : base_w;
    float acc = 0.f;
    for (int i = lane; i < Dc; i += 64) acc += s_core[i] * w[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      acc += __shfl_down(acc, off, 64);
    }
    if (lane == 0) {
      if (row < A) {
        const float v = acc + policy_b[row];
        s_logits[row] = v;
        out_logits[(int64_t)s * A + row] = v;
      } else {
        out_base[s] = acc + base_b[0];
      }
    }
  }
  __syncthreads();

  if (threadIdx.x == 0) {
    int best = 0;
    if (greedy) {
      float bv = s_logits[0];
      for (int a = 1; a < A; ++a) {
        if (s_logits[a] > bv) {
          bv = s_logits[a];
          best = a;
        }
      }
    } else {
      hiprandStatePhilox4_32_10_t rng;
      hiprand_init(seed, s, 0, &rng);
      float bv = -1e30f;
      for (int a = 0; a < A; ++a) {
        // hiprand_uniform is (v + 1) * 2^-32 rounded to float: at least
        // 2^-32, so the inner log is finite, but exactly 1.0f for the top
        // ~2^7 values of v, where -log(-log(1)) = +inf would win against
        // any logit. The largest float below 1 caps the Gumbel value at
        // -log(-log(1 - 2^-24)) ~ 16.6 and changes no other draw.
        const float u = fminf(hiprand_uniform(&rng), 0x1.fffffep-1f);
        const float g = s_logits[a] - __logf(-__logf(u));
        if (g > bv) {
          bv = g;
          best = a;
        }
      }
    }
    out_action[s] = best;
  }
}

// unpack_rollouts: staging [B, stride] holds one rollout slot window per
// row; column c has `outer` rows of `inner_bytes` at src_off in every
// staging row. Output row (o, b) of a column goes to
// dst + (o * B + b) * inner_bytes, i.e. the [outer, B, inner] leaf.
//
// Workgroups are dealt to columns on the host (block_begin): a wide column
// (inner_bytes >= kWideRowBytes) gets one workgroup per output row, the
// lanes striding over the row; a narrow one gets one lane per output row.
// Either way the only division is one 32-bit (row / B) per workgroup or
// per lane, never per element. The access width (16, 8, 4 or 1 bytes) is
// the widest that divides the row length, the staging stride and both base
// addresses; it is uniform over a column.
// Limitation: the two paths are sized for the rollout slot's columns, frame
// rows of tens of KB and leaves of a few bytes. A row of 256..4095 bytes
// keeps only inner_bytes/16 of the workgroup's 256 lanes busy (16 lanes at
// 256 bytes), and a row of up to 255 bytes is copied serially by one lane
// with uncoalesced accesses. Both are correct but far below bandwidth; a
// mid-width column (LSTM-sized state, say) moved into the slab would want a
// wavefront-per-row path first.
constexpr int kUnpackThreads = 256;
constexpr int64_t kWideRowBytes = 256;

struct UnpackArgs {
  UnpackColumn col[kMaxGatherColumns];
  uint32_t block_begin[kMaxGatherColumns + 1];
  int32_t n_cols;
  int32_t B;
  int64_t stride;
};

template <typename V>
__device__ __forceinline__ void copy_strided(uint8_t* __restrict__ dst,
                                             const uint8_t* __restrict__ src,
                                             int64_t nbytes, int first,
                                             int step) {
  const int n = (int)(nbytes / (int64_t)sizeof(V));
  auto* d = reinterpret_cast<V*>(dst);
  const auto* s = reinterpret_cast<const V*>(src);
  for (int i = first; i < n; i += step) d[i] = s[i];
}

__device__ __forceinline__ void copy_row(uint8_t* dst, const uint8_t* src,
                                         int64_t nbytes, unsigned align,
                                         int first, int step) {
  if ((align & 15u) == 0) {
    copy_strided<uint4>(dst, src, nbytes, first, step);
  } else if ((align & 7u) == 0) {
    copy_strided<uint2>(dst, src, nbytes, first, step);
  } else if ((align & 3u) == 0) {
    copy_strided<uint32_t>(dst, src, nbytes, first, step);
  } else {
    copy_strided<uint8_t>(dst, src, nbytes, first, step);
  }
}

__global__ __launch_bounds__(kUnpackThreads) void unpack_rollouts_kernel(
    const uint8_t* __restrict__ staging, const UnpackArgs args) {
  int c = 0;
  while (c + 1 < args.n_cols && blockIdx.x >= args.block_begin[c + 1]) ++c;
  const UnpackColumn col = args.col[c];
  const uint32_t local = blockIdx.x - args.block_begin[c];
  const uint32_t B = (uint32_t)args.B;
  const uint32_t rows = (uint32_t)col.outer * B;
  const uint8_t* src0 = staging + col.src_off;
  const unsigned align =
      (unsigned)(((uint64_t)col.inner_bytes | (uint64_t)args.stride |
                  (uint64_t)(uintptr_t)src0 | (uint64_t)(uintptr_t)col.dst) &
                 15u);
  if (col.inner_bytes >= kWideRowBytes) {
    const uint32_t row = local;  // one workgroup per output row
    if (row >= rows) return;
    const uint32_t o = row / B, b = row - o * B;
    copy_row(col.dst + (int64_t)row * col.inner_bytes,
             src0 + (int64_t)b * args.stride + (int64_t)o * col.inner_bytes,
             col.inner_bytes, align, (int)threadIdx.x, kUnpackThreads);
  } else {
    const uint32_t row = local * kUnpackThreads + threadIdx.x;
    if (row >= rows) return;
    const uint32_t o = row / B, b = row - o * B;
    copy_row(col.dst + (int64_t)row * col.inner_bytes,
             src0 + (int64_t)b * args.stride + (int64_t)o * col.inner_bytes,
             col.inner_bytes, align, 0, 1);
  }
}

// gather_rows: an inference batch gathered straight from rollout rows. The
// table (pinned host memory, read in place) holds one frame pointer and one
// reward pointer per request, all inside the pinned rollout slab
// (row_gather.h checks that on the host). Frame r goes to out_frames row r,
// reward r is clamped to [-1, 1] into out_rew[r]; rows >= b of both outputs
// are not touched.
//
// Grid (chunks_per_frame, b): a frame is cut into kChunk-byte pieces so that
// a small batch of large frames still covers the chip (b = 64 frames of
// 100,800 bytes make 448 workgroups at 16 KB) and no workgroup queues a whole
// frame's host-link reads behind one another. The two block indices are the
// chunk and the row: no division anywhere. Lanes stride over the chunk with
// `width`-byte accesses (16, 8, 4 or 1; uniform per launch, computed on the
// host over fsz and every source address; kChunk is a multiple of 16 and
// the destination rows are fsz apart in a 256-byte aligned buffer, so both
// sides are aligned). Host rows are read once: non-temporal loads. The
// destination is read next by the trunk: plain stores.
constexpr int kGatherRowsThreads = 256;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// Copies n_bytes (a multiple of sizeof(V)) with all lanes of the workgroup.
// A full chunk has a compile-time trip count, so its loads are all issued
// before the first store waits on one: kChunk / (256 * 16) host-link reads
// in flight per lane.
template <typename V, int kChunk>
__device__ __forceinline__ void gather_chunk(uint8_t* __restrict__ dst,
                                             const uint8_t* __restrict__ src,
                                             int n_bytes) {
  auto* d = reinterpret_cast<V*>(dst);
  const auto* s = reinterpret_cast<const V*>(src);
  constexpr int kPerLane = kChunk / (kGatherRowsThreads * (int)sizeof(V));
  if constexpr (kPerLane <= 16) {
    if (n_bytes == kChunk) {
      V v[kPerLane];
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) {
        v[k] = __builtin_nontemporal_load(s + k * kGatherRowsThreads +
                                          (int)threadIdx.x);
      }
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) {
        d[k * kGatherRowsThreads + (int)threadIdx.x] = v[k];
      }
      return;
    }
  }
  const int n = n_bytes / (int)sizeof(V);
  for (int i = (int)threadIdx.x; i < n; i += kGatherRowsThreads) {
    d[i] = __builtin_nontemporal_load(s + i);
  }
}

template <int kChunk>
__global__ __launch_bounds__(kGatherRowsThreads) void gather_rows_kernel(
    const uint8_t* const* __restrict__ frame_src,  // host pinned [b]
    const float* const* __restrict__ rew_src,      // host pinned [b]
    int fsz, int width,
    uint8_t* __restrict__ out_frames,  // [cap, fsz]
    float* __restrict__ out_rew) {     // [cap]
  static_assert(kChunk % (kGatherRowsThreads * 16) == 0, "chunk granularity");
  const int r = blockIdx.y;
  const int begin = (int)blockIdx.x * kChunk;
  const int n = min(kChunk, fsz - begin);
  const uint8_t* src = frame_src[r] + begin;
  uint8_t* dst = out_frames + (int64_t)r * fsz + begin;
  if (width == 16) {
    gather_chunk<u32x4, kChunk>(dst, src, n);
  } else if (width == 8) {
    gather_chunk<u32x2, kChunk>(dst, src, n);
  } else if (width == 4) {
    gather_chunk<uint32_t, kChunk>(dst, src, n);
  } else {
    gather_chunk<uint8_t, kChunk>(dst, src, n);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const float v = __builtin_nontemporal_load(rew_src[r]);
    out_rew[r] = v < -1.f ? -1.f : (v > 1.f ? 1.f : v);
  }
}

// lstm_serve_layer: one LSTM layer, one time step, for an inference batch
// whose recurrent state lives in pinned host memory (the pool's state rows).
// For request r and hidden unit j
//   gates = W_ih in_r + W_hh (nd_r h_prev_r) + b_ih + b_hh      (i, f, g, o)
//   c'    = sigmoid(f) (nd_r c_prev_r) + sigmoid(i) tanh(g)
//   h'    = sigmoid(o) tanh(c')
// as a bf16 MFMA GEMM (v_mfma_f32_16x16x32_bf16, f32 accumulation) with
// M = requests, N = 4 gates x Hn, K = Ip + Hk: in_r and the masked h_prev_r
// are rounded to bf16 into one LDS row of length Kp = Ip + Hk, the packed
// weights [4, Hn, Kp] bf16 hold W_ih in columns [0, I) and W_hh in columns
// [Ip, Ip + H), zero elsewhere (Ip, Hk: I, H rounded up to 32; Hn: H rounded
// up to 16), so odd sizes such as 513 cost a padded k-step and masked
// stores, not a special case. The cell path and the stored state are f32.
//
// A workgroup owns 16 requests x 16 hidden units with all four gate rows of
// those units, so the cell update needs no second pass: grid (Hn / 16,
// ceil(b / 16)), e.g. 33 x 8 = 264 workgroups for H = 513 at b = 128. Its
// four waves split K (wave w takes k-steps w, w + 4, ...: the loop is bound
// by the latency of streaming the weights from L2, and four short loops
// hide more of it than one long one), each with one A fragment from LDS
// and four B fragments (one per gate) straight from global memory per
// k-step, no barrier in the loop. The partial sums meet in LDS, then thread
// t finishes request t / 16, unit t % 16.
//
// The previous state comes from `staged`, device memory that
// lstm_stage_state_kernel (below) filled from the pinned state rows once per
// batch, with a done row's state already zeroed. The first version read
// h_prev over the host link in every workgroup, i.e. Hn / 16 = 33 times per
// request and layer; those workgroups sat on the CUs (and on 51 KB of LDS
// each) waiting for the link, and `bench.py --use_lstm` fell from 89k to 65k
// SPS (profiles/PROFILE_r7.md). h' and c' are written to pinned host memory
// through the table of build_state_table() (row_gather.h), which has checked
// every address and that no out range overlaps an in range, with ordinary
// stores. h' also goes to `h_out` (device), the next layer's or the heads'
// input. Only requests [0, b) are touched: the rows that pad the last
// 16-row tile are zero in LDS and never dereference the table, nor are they
// stored.
constexpr int kLstmThreads = 256;
constexpr int kLstmTile = 16;  // requests and hidden units per workgroup
constexpr int kLstmRowPad = 8;  // bf16 elements between LDS rows

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f32x4 = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ float sigmoidf_(float v) {
  return 1.f / (1.f + __expf(-v));
}

// The batch's previous state, read ONCE from the pinned state rows: request
// r's 2 L H floats (h [L, H], then c) go to row r of `staged` (device), or
// zeros if its row's done byte is set (selected, not multiplied: a done
// row's old state is not read at all). One workgroup per request; only
// requests [0, b) are touched.
__global__ __launch_bounds__(256) void lstm_stage_state_kernel(
    const float* const* __restrict__ state_in,    // host pinned [b]
    const uint8_t* const* __restrict__ done_src,  // host pinned [b]
    int n_floats,
    float* __restrict__ staged) {  // device [>= b, n_floats]
  const int r = blockIdx.x;
  const bool keep = *done_src[r] == 0;
  const float* src = state_in[r];
  float* dst = staged + (int64_t)r * n_floats;
  for (int i = threadIdx.x; i < n_floats; i += 256) {
    dst[i] = keep ? __builtin_nontemporal_load(src + i) : 0.f;
  }
}

__global__ __launch_bounds__(kLstmThreads) void lstm_serve_layer_kernel(
    float* const* __restrict__ state_out,  // host pinned [b]
    const float* __restrict__ staged,      // device [>= b, 2 L H], masked
    const float* __restrict__ in,    // device [>= b, in_stride]
    const float* __restrict__ rew,   // device [>= b] or nullptr (layers > 0)
    const __bf16* __restrict__ W,    // [4 * Hn, Kp]
    const float* __restrict__ bias,  // [4 * Hn], b_ih + b_hh
    int b, int layer, int L, int H, int I, int in_stride, int Ip, int Kp,
    int Hn,
    float* __restrict__ h_out) {  // device [>= b, H]
  extern __shared__ __attribute__((aligned(16))) char lstm_smem[];
  const int lda = Kp + kLstmRowPad;
  __bf16* A = reinterpret_cast<__bf16*>(lstm_smem);
  float* red = reinterpret_cast<float*>(lstm_smem + kLstmTile * lda * 2);
  __shared__ float* s_out[kLstmTile];

  const int tid = threadIdx.x;
  const int u0 = blockIdx.x * kLstmTile;
  const int m0 = blockIdx.y * kLstmTile;
  if (tid < kLstmTile) {
    const int r = m0 + tid;
    s_out[tid] = r < b ? state_out[r] : nullptr;
  }

  // Stage [in_r, nd_r h_prev_r] as bf16: 16 lanes per request.
  const int row = tid >> 4;
  const int q = tid & 15;
  const int r = m0 + row;
  const bool valid = r < b;
  const float* prev = staged + (int64_t)(valid ? r : 0) * 2 * L * H;
  {
    __bf16* a = A + row * lda;
    const float* xin = in + (int64_t)(valid ? r : 0) * in_stride;
    const int nx = rew != nullptr ? I - 1 : I;
    for (int k = q; k < Ip; k += 16) {
      float v = 0.f;
      if (valid) {
        if (k < nx) {
          v = xin[k];
        } else if (k < I) {
          v = rew[r];
        }
      }
      a[k] = (__bf16)v;
    }
    const float* hp = prev + (int64_t)layer * H;
    for (int j = q; j < Kp - Ip; j += 16) {
      a[Ip + j] = (__bf16)((valid && j < H) ? hp[j] : 0.f);
    }
  }
  __syncthreads();

  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int ln = lane & 15;
  const int lg = lane >> 4;
  f32x4 acc[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) acc[g] = {0.f, 0.f, 0.f, 0.f};
  // A[m = ln][k = 8 lg + j] from LDS, B[k = 8 lg + j][n = ln] from the
  // packed weights, which hold unit n's row k-contiguous.
  const __bf16* al = A + ln * lda + lg * 8;
  const __bf16* wl = W + (int64_t)(u0 + ln) * Kp + lg * 8;
  const int64_t gate_stride = (int64_t)Hn * Kp;
  const int ksteps = Kp >> 5;
  for (int ks = wave; ks < ksteps; ks += kLstmThreads / 64) {
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(al + ks * 32);
    bf16x8 w[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      w[g] = *reinterpret_cast<const bf16x8*>(wl + g * gate_stride + ks * 32);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, w[g], acc[g], 0, 0, 0);
    }
  }
  // C: column (unit) = lane & 15, row (request) = 4 (lane >> 4) + register.
#pragma unroll
  for (int g = 0; g < 4; ++g) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      red[((wave * 4 + g) * kLstmTile + lg * 4 + i) * kLstmTile + ln] =
          acc[g][i];
    }
  }
  __syncthreads();

  const int j = u0 + q;
  if (!valid || j >= H) return;
  float gates[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    float v = bias[g * Hn + j];
#pragma unroll
    for (int w = 0; w < kLstmThreads / 64; ++w) {
      v += red[((w * 4 + g) * kLstmTile + row) * kLstmTile + q];
    }
    gates[g] = v;
  }
  const int64_t lh = (int64_t)layer * H + j;
  const float c_prev = prev[(int64_t)L * H + lh];
  const float c_new =
      sigmoidf_(gates[1]) * c_prev + sigmoidf_(gates[0]) * tanhf(gates[2]);
  const float h_new = sigmoidf_(gates[3]) * tanhf(c_new);
  float* out = s_out[row];
  out[lh] = h_new;
  out[(int64_t)L * H + lh] = c_new;
  h_out[(int64_t)r * H + j] = h_new;
}

}  // namespace

// Host wrappers -------------------------------------------------------------

int64_t gather_rows_chunk_bytes() { return kGatherRowsChunkBytes; }

void launch_gather_rows(const uint8_t* const* frame_src,
                        const float* const* rew_src, int64_t b, int64_t fsz,
                        uint8_t* out_frames, float* out_rew,
                        int64_t chunk_bytes) {
  TORCH_CHECK(b >= 1 && fsz >= 1, "gather_rows: empty batch or frame");
  TORCH_CHECK(frame_src != nullptr && rew_src != nullptr &&
                  out_frames != nullptr && out_rew != nullptr,
              "gather_rows: null argument");
  TORCH_CHECK(fsz < (int64_t(1) << 31), "gather_rows: frame too large");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(out_frames) % 16 == 0,
              "gather_rows: output frames must be 16-byte aligned");
  const int64_t chunks = (fsz + chunk_bytes - 1) / chunk_bytes;
  // gridDim.y carries the row.
  TORCH_CHECK(b <= 65535 && b * chunks < (int64_t(1) << 31),
              "gather_rows: grid too big");
  // The table is pinned host memory: the host reads it as well.
  uint64_t bits = (uint64_t)fsz;
  for (int64_t r = 0; r < b; ++r) {
    bits |= (uint64_t)reinterpret_cast<uintptr_t>(frame_src[r]);
  }
  const int width = (int)row_access_width(bits);
  const dim3 grid((uint32_t)chunks, (uint32_t)b);
  const dim3 block(kGatherRowsThreads);
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
#define TBAMD_GATHER_ROWS(KB)                                                \
  hipLaunchKernelGGL(gather_rows_kernel<KB * 1024>, grid, block, 0, stream, \
                     frame_src, rew_src, (int)fsz, width, out_frames, out_rew)
  switch (chunk_bytes) {
    case 4096: TBAMD_GATHER_ROWS(4); break;
    case 8192: TBAMD_GATHER_ROWS(8); break;
    case 16384: TBAMD_GATHER_ROWS(16); break;
    case 32768: TBAMD_GATHER_ROWS(32); break;
    default: TORCH_CHECK(false, "gather_rows: chunk must be 4, 8, 16 or 32 KB");
  }
#undef TBAMD_GATHER_ROWS
  const hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "gather_rows launch: ",
              hipGetErrorString(err));
}

std::tuple<torch::Tensor, torch::Tensor> gather_rows(
    torch::Tensor slab, std::vector<int64_t> frame_offsets,
    std::vector<int64_t> reward_offsets, int64_t fsz, int64_t cap,
    int64_t chunk_bytes) {
  TORCH_CHECK(slab.device().is_cpu() && slab.scalar_type() == torch::kUInt8 &&
                  slab.is_contiguous() && slab.is_pinned(),
              "gather_rows: slab must be a contiguous pinned uint8 tensor");
  const int64_t b = (int64_t)frame_offsets.size();
  TORCH_CHECK(b >= 1 && reward_offsets.size() == frame_offsets.size() &&
                  cap >= b && fsz >= 1,
              "gather_rows: need 1 <= b <= cap offsets of each kind");
  const int64_t total = slab.numel();
  for (int64_t r = 0; r < b; ++r) {
    const int64_t f = frame_offsets[r], w = reward_offsets[r];
    TORCH_CHECK_INDEX(f >= 0 && f <= total && fsz <= total - f,
                      "gather_rows: frame ", r, " leaves the slab");
    TORCH_CHECK_INDEX(w >= 0 && w <= total && 4 <= total - w,
                      "gather_rows: reward ", r, " leaves the slab");
  }
  if (chunk_bytes == 0) chunk_bytes = kGatherRowsChunkBytes;
  auto table = torch::empty({2 * b}, torch::TensorOptions()
                                         .dtype(torch::kInt64)
                                         .pinned_memory(true));
  auto** ft = reinterpret_cast<const uint8_t**>(table.data_ptr<int64_t>());
  auto** rt = reinterpret_cast<const float**>(table.data_ptr<int64_t>() + b);
  const uint8_t* base = slab.data_ptr<uint8_t>();
  // Checks every range once more, against the slab's addresses.
  build_row_table(
      b, [&](int64_t r) { return base + frame_offsets[r]; },
      [&](int64_t r) { return base + reward_offsets[r]; }, fsz, base, total,
      ft, rt);
  auto dev = torch::Device(torch::kCUDA, at::cuda::current_device());
  auto frames = torch::full({cap, fsz}, 0xA5,
                            torch::TensorOptions().dtype(torch::kUInt8).device(dev));
  auto rew = torch::full({cap, 1}, -7.0f,
                         torch::TensorOptions().dtype(torch::kFloat32).device(dev));
  launch_gather_rows(ft, rt, b, fsz, frames.data_ptr<uint8_t>(),
                     rew.data_ptr<float>(), chunk_bytes);
  // The kernel reads `table` and `slab` in place: neither may go away or
  // change under it.
  at::cuda::getCurrentCUDAStream().synchronize();
  return {frames, rew};
}

void launch_unpack_rollouts(const uint8_t* staging, int64_t stride, int64_t B,
                            const UnpackColumn* columns, int n_columns) {
  TORCH_CHECK(n_columns >= 1 && n_columns <= kMaxGatherColumns,
              "unpack_rollouts: 1..", kMaxGatherColumns, " columns");
  TORCH_CHECK(B >= 1 && stride >= 1, "unpack_rollouts: empty batch");
  UnpackArgs args;
  args.n_cols = n_columns;
  args.B = (int32_t)B;
  args.stride = stride;
  int64_t blocks = 0;
  for (int c = 0; c < n_columns; ++c) {
    const UnpackColumn& col = columns[c];
    TORCH_CHECK(col.inner_bytes >= 1 && col.inner_bytes < (int64_t(1) << 31) &&
                    col.outer >= 1 && col.src_off >= 0 && col.dst != nullptr,
                "unpack_rollouts: bad column ", c);
    TORCH_CHECK(col.src_off + col.outer * col.inner_bytes <= stride,
                "unpack_rollouts: column ", c, " overruns the staging row");
    const int64_t rows = col.outer * B;
    TORCH_CHECK(rows < (int64_t(1) << 31), "unpack_rollouts: too many rows");
    args.col[c] = col;
    args.block_begin[c] = (uint32_t)blocks;
    blocks += col.inner_bytes >= kWideRowBytes
                  ? rows
                  : (rows + kUnpackThreads - 1) / kUnpackThreads;
    TORCH_CHECK(blocks < (int64_t(1) << 31), "unpack_rollouts: grid too big");
  }
  for (int c = n_columns; c <= kMaxGatherColumns; ++c) {
    args.block_begin[c] = (uint32_t)blocks;
  }
  for (int c = n_columns; c < kMaxGatherColumns; ++c) {
    args.col[c] = UnpackColumn{0, 0, 0, nullptr};
  }
  hipLaunchKernelGGL(unpack_rollouts_kernel, dim3((uint32_t)blocks),
                     dim3(kUnpackThreads), 0,
                     at::cuda::getCurrentCUDAStream(), staging, args);
  const hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "unpack_rollouts launch: ",
              hipGetErrorString(err));
}

std::vector<torch::Tensor> unpack_rollouts(
    torch::Tensor staging, int64_t stride, int64_t B,
    std::vector<std::tuple<int64_t, int64_t, int64_t>> columns) {
  TORCH_CHECK(staging.is_cuda() && staging.scalar_type() == torch::kUInt8 &&
                  staging.is_contiguous(),
              "unpack_rollouts: staging must be a contiguous uint8 GPU tensor");
  TORCH_CHECK(B >= 1 && stride >= 1 && staging.numel() >= B * stride,
              "unpack_rollouts: staging smaller than B * stride");
  at::cuda::CUDAGuard device_guard(staging.device());
  int64_t total = 0;
  for (const auto& c : columns) {
    TORCH_CHECK(std::get<1>(c) >= 1 && std::get<2>(c) >= 1,
                "unpack_rollouts: empty column");
    total += round_up_256(std::get<1>(c) * B * std::get<2>(c));
  }
  torch::Tensor arena = torch::empty({total}, staging.options());
  std::vector<UnpackColumn> desc;
  std::vector<torch::Tensor> out;
  int64_t off = 0;
  for (const auto& c : columns) {
    const int64_t outer = std::get<1>(c), inner = std::get<2>(c);
    const int64_t nbytes = outer * B * inner;
    desc.push_back(UnpackColumn{std::get<0>(c), inner, outer,
                                arena.data_ptr<uint8_t>() + off});
    out.push_back(arena.narrow(0, off, nbytes).view({outer, B, inner}));
    off += round_up_256(nbytes);
  }
  launch_unpack_rollouts(staging.data_ptr<uint8_t>(), stride, B, desc.data(),
                         (int)desc.size());
  return out;
}

// Returns {frames [bp,C,H,W] u8 (GPU), rew [bp,1] f32 (GPU), nd [bp] f32}.
std::vector<torch::Tensor> gather_obs(torch::Tensor slab_frames,
                                      torch::Tensor slab_rew,
                                      torch::Tensor slab_done,
                                      torch::Tensor ids_cpu, int64_t bp,
                                      std::vector<int64_t> frame_shape) {
  // Every check before any allocation or launch: the kernel reads the slabs
  // in place over the host link, so a stray id, a pageable slab or a frame
  // size the 16-byte accesses do not divide would be a GPU fault.
  int64_t fsz = 1;
  for (auto d : frame_shape) fsz *= d;
  TORCH_CHECK(fsz >= 16 && fsz % 16 == 0 && fsz < (int64_t(1) << 31),
              "gather_obs: frame bytes must be a multiple of 16 below 2^31, "
              "got ", fsz);
  const auto host_slab = [](const torch::Tensor& t, torch::ScalarType ty) {
    return t.defined() && t.device().is_cpu() && t.scalar_type() == ty &&
           t.is_contiguous() && t.is_pinned();
  };
  TORCH_CHECK(host_slab(slab_frames, torch::kUInt8) && slab_frames.dim() >= 1,
              "gather_obs: frame slab must be a contiguous pinned uint8 CPU "
              "tensor");
  TORCH_CHECK(host_slab(slab_rew, torch::kFloat32),
              "gather_obs: reward slab must be a contiguous pinned float32 "
              "CPU tensor");
  TORCH_CHECK(host_slab(slab_done, torch::kUInt8),
              "gather_obs: done slab must be a contiguous pinned uint8 CPU "
              "tensor");
  const int64_t slots = slab_frames.size(0);
  TORCH_CHECK(slots >= 1 && slab_rew.numel() == slots &&
                  slab_done.numel() == slots,
              "gather_obs: the slabs disagree on the slot count (",
              slab_frames.size(0), " frames, ", slab_rew.numel(),
              " rewards, ", slab_done.numel(), " dones)");
  TORCH_CHECK(slab_frames.numel() == slots * fsz,
              "gather_obs: frame_shape does not match the frame slab");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(slab_frames.data_ptr()) % 16 == 0,
              "gather_obs: frame slab must be 16-byte aligned");
  TORCH_CHECK(ids_cpu.defined() && ids_cpu.device().is_cpu() &&
                  (ids_cpu.scalar_type() == torch::kInt32 ||
                   ids_cpu.scalar_type() == torch::kInt64),
              "gather_obs: ids must be an int32 or int64 CPU tensor");
  const int64_t b = ids_cpu.numel();
  TORCH_CHECK(b >= 1 && b <= bp && bp < (int64_t(1) << 31),
              "gather_obs: need 1 <= b <= bp, got b = ", b, ", bp = ", bp);
  {
    const torch::Tensor flat = ids_cpu.reshape({-1});
    const int64_t stride = flat.stride(0);
    const bool wide = flat.scalar_type() == torch::kInt64;
    for (int64_t r = 0; r < b; ++r) {
      const int64_t id = wide ? flat.data_ptr<int64_t>()[r * stride]
                              : (int64_t)flat.data_ptr<int32_t>()[r * stride];
      TORCH_CHECK(id >= 0 && id < slots, "gather_obs: id ", id, " of request ",
                  r, " is outside the slab's ", slots, " slots");
    }
  }
  auto dev = torch::Device(torch::kCUDA, at::cuda::current_device());
  auto opts = torch::TensorOptions().device(dev);
  // Pad the ids staging to the quantized batch size so the pinned-alloc
  // cache sees a handful of sizes (a fresh hipHostMalloc device-syncs).
  auto ids_pin = torch::zeros({bp}, torch::TensorOptions()
                                        .dtype(torch::kInt32)
                                        .pinned_memory(true));
  ids_pin.narrow(0, 0, b).copy_(ids_cpu.to(torch::kInt32).reshape({-1}));
  auto ids = ids_pin.to(dev, /*non_blocking=*/true);
  std::vector<int64_t> oshape = {bp};
  oshape.insert(oshape.end(), frame_shape.begin(), frame_shape.end());
  auto frames = torch::empty(oshape, opts.dtype(torch::kUInt8));
  auto rew = torch::empty({bp, 1}, opts.dtype(torch::kFloat32));
  auto nd = torch::empty({bp}, opts.dtype(torch::kFloat32));
  hipLaunchKernelGGL(gather_obs_kernel, dim3((uint32_t)bp), dim3(256), 0,
                     at::cuda::getCurrentCUDAStream(),
                     slab_frames.data_ptr<uint8_t>(),
                     slab_rew.data_ptr<float>(),
                     slab_done.data_ptr<uint8_t>(), ids.data_ptr<int>(),
                     (int)b, (int)bp, (int)fsz, frames.data_ptr<uint8_t>(),
                     rew.data_ptr<float>(), nd.data_ptr<float>());
  const hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "gather_obs launch: ",
              hipGetErrorString(err));
  return {frames, rew, nd};
}

namespace {

bool f32_on_gpu(const torch::Tensor& t) {
  return t.defined() && t.is_cuda() && t.scalar_type() == torch::kFloat32 &&
         t.is_contiguous();
}

// Host checks of the heads kernel's weights, for a core of Dc elements. The
// kernel indexes all four by A and Dc alone, so a bias on the CPU or a short
// one would be a GPU fault.
void check_heads_weights(const torch::Tensor& policy_w,
                         const torch::Tensor& policy_b,
                         const torch::Tensor& base_w,
                         const torch::Tensor& base_b, int64_t Dc) {
  TORCH_CHECK(f32_on_gpu(policy_w) && f32_on_gpu(policy_b) &&
                  f32_on_gpu(base_w) && f32_on_gpu(base_b),
              "heads_sample: weights and biases must be contiguous float32 "
              "GPU tensors");
  TORCH_CHECK(policy_b.device() == policy_w.device() &&
                  base_w.device() == policy_w.device() &&
                  base_b.device() == policy_w.device() &&
                  policy_w.device().index() == at::cuda::current_device(),
              "heads_sample: weights and biases must be on the current GPU");
  TORCH_CHECK(policy_w.dim() == 2 && base_w.dim() == 2,
              "heads_sample: weights must be [A, Dc] and [1, Dc]");
  const int64_t A = policy_w.size(0);
  TORCH_CHECK(A >= 1 && A <= 64,
              "heads_sample: 1 to 64 actions supported, got ", A);
  TORCH_CHECK(Dc >= 1 && policy_w.size(1) == Dc && base_w.size(1) == Dc,
              "heads_sample: head weights do not match the core's length ",
              Dc);
  TORCH_CHECK(base_w.size(0) == 1 && policy_b.numel() == A &&
                  base_b.numel() == 1,
              "heads_sample: need policy_b of A elements, base_w of one row "
              "and base_b of one element");
  // The core in dynamic LDS beside the kernel's 64 static floats.
  const size_t limit = at::cuda::getCurrentDeviceProperties()->sharedMemPerBlock;
  TORCH_CHECK((size_t)Dc * sizeof(float) + 64 * sizeof(float) <= limit,
              "heads_sample: a core of ", Dc, " floats does not fit the ",
              limit, " bytes of LDS");
}

// Host checks of the core as tensors: x [>= b, D], rew (if any) >= b
// elements, both on the weights' GPU.
void check_heads_inputs(const torch::Tensor& x, const torch::Tensor* rew,
                        const torch::Tensor& policy_w, int64_t b) {
  TORCH_CHECK(f32_on_gpu(x) && x.dim() == 2,
              "heads_sample: x must be a contiguous float32 [n, D] GPU "
              "tensor");
  TORCH_CHECK(rew == nullptr || f32_on_gpu(*rew),
              "heads_sample: rew must be a contiguous float32 GPU tensor");
  TORCH_CHECK(policy_w.defined() && x.device() == policy_w.device() &&
                  (rew == nullptr || rew->device() == x.device()),
              "heads_sample: x, rew and the weights must be on one GPU");
  TORCH_CHECK(b >= 1 && x.size(0) >= b && (rew == nullptr || rew->numel() >= b),
              "heads_sample: batch of ", b, " exceeds its inputs");
}

}  // namespace

// Writes action/logits/baseline into freshly allocated PINNED host tensors;
// caller syncs the stream before reading them.
std::vector<torch::Tensor> fused_heads_sample(torch::Tensor x,
                                              torch::Tensor rew,
                                              torch::Tensor policy_w,
                                              torch::Tensor policy_b,
                                              torch::Tensor base_w,
                                              torch::Tensor base_b, int64_t b,
                                              bool greedy, int64_t seed) {
  // Checked here too: nothing is allocated for a call that will not launch.
  check_heads_inputs(x, &rew, policy_w, b);
  check_heads_weights(policy_w, policy_b, base_w, base_b, x.size(1) + 1);
  const int A = policy_w.size(0);
  // Allocate pinned outputs at the quantized batch size (cache-friendly;
  // ragged sizes would hipHostMalloc + device-sync per serve), then hand
  // back narrowed views.
  const int64_t bq = (b + 63) / 64 * 64;
  auto hopts = torch::TensorOptions().pinned_memory(true);
  auto action = torch::empty({bq}, hopts.dtype(torch::kInt64)).narrow(0, 0, b);
  auto logits =
      torch::empty({bq, A}, hopts.dtype(torch::kFloat32)).narrow(0, 0, b);
  auto baseline =
      torch::empty({bq}, hopts.dtype(torch::kFloat32)).narrow(0, 0, b);
  launch_heads_sample(x.data_ptr<float>(), rew.data_ptr<float>(), x.size(1),
                      policy_w, policy_b, base_w, base_b, b, greedy, seed,
                      action.data_ptr<int64_t>(), logits.data_ptr<float>(),
                      baseline.data_ptr<float>());
  return {action, logits, baseline};
}

void fused_heads_sample_out(const torch::Tensor& x, const torch::Tensor& rew,
                            const torch::Tensor& policy_w,
                            const torch::Tensor& policy_b,
                            const torch::Tensor& base_w,
                            const torch::Tensor& base_b, int64_t b,
                            bool greedy, int64_t seed, int64_t* out_action,
                            float* out_logits, float* out_baseline) {
  check_heads_inputs(x, &rew, policy_w, b);
  launch_heads_sample(x.data_ptr<float>(), rew.data_ptr<float>(), x.size(1),
                      policy_w, policy_b, base_w, base_b, b, greedy, seed,
                      out_action, out_logits, out_baseline);
}

void launch_heads_sample(const float* core, const float* rew, int64_t D,
                         const torch::Tensor& policy_w,
                         const torch::Tensor& policy_b,
                         const torch::Tensor& base_w,
                         const torch::Tensor& base_b, int64_t b, bool greedy,
                         int64_t seed, int64_t* out_action, float* out_logits,
                         float* out_baseline) {
  const int64_t Dc = rew != nullptr ? D + 1 : D;
  TORCH_CHECK(D >= 1 && Dc < (int64_t(1) << 31),
              "heads_sample: bad core length ", D);
  check_heads_weights(policy_w, policy_b, base_w, base_b, Dc);
  TORCH_CHECK(b >= 1 && b < (int64_t(1) << 31), "heads_sample: bad batch ", b);
  TORCH_CHECK(core != nullptr && out_action != nullptr &&
                  out_logits != nullptr && out_baseline != nullptr,
              "heads_sample: null argument");
  const int A = policy_w.size(0);
  const size_t lds = (size_t)Dc * sizeof(float);
  hipLaunchKernelGGL(heads_sample_kernel, dim3((uint32_t)b), dim3(256), lds,
                     at::cuda::getCurrentCUDAStream(), core, rew,
                     policy_w.data_ptr<float>(), policy_b.data_ptr<float>(),
                     base_w.data_ptr<float>(), base_b.data_ptr<float>(),
                     (int)b, (int)D, A, (uint64_t)seed, greedy ? 1 : 0,
                     out_action, out_logits, out_baseline);
  const hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "heads_sample launch: ",
              hipGetErrorString(err));
}

void heads_sample(torch::Tensor x, std::optional<torch::Tensor> rew,
                  torch::Tensor policy_w, torch::Tensor policy_b,
                  torch::Tensor base_w, torch::Tensor base_b, int64_t b,
                  bool greedy, int64_t seed, torch::Tensor action,
                  torch::Tensor logits, torch::Tensor baseline) {
  const torch::Tensor* r = rew.has_value() ? &*rew : nullptr;
  check_heads_inputs(x, r, policy_w, b);
  at::cuda::CUDAGuard device_guard(x.device());
  check_heads_weights(policy_w, policy_b, base_w, base_b,
                      x.size(1) + (r != nullptr ? 1 : 0));
  const int64_t A = policy_w.size(0);
  const auto pinned = [](const torch::Tensor& t, torch::ScalarType ty) {
    return t.defined() && t.device().is_cpu() && t.scalar_type() == ty &&
           t.is_contiguous() && t.is_pinned();
  };
  TORCH_CHECK(pinned(action, torch::kInt64) && action.numel() >= b,
              "heads_sample: action must be a contiguous pinned int64 CPU "
              "tensor of at least b elements");
  TORCH_CHECK(pinned(logits, torch::kFloat32) && logits.dim() == 2 &&
                  logits.size(0) >= b && logits.size(1) == A,
              "heads_sample: logits must be a contiguous pinned float32 CPU "
              "tensor [>= b, A]");
  TORCH_CHECK(pinned(baseline, torch::kFloat32) && baseline.numel() >= b,
              "heads_sample: baseline must be a contiguous pinned float32 CPU "
              "tensor of at least b elements");
  launch_heads_sample(x.data_ptr<float>(),
                      r != nullptr ? r->data_ptr<float>() : nullptr, x.size(1),
                      policy_w, policy_b, base_w, base_b, b, greedy, seed,
                      action.data_ptr<int64_t>(), logits.data_ptr<float>(),
                      baseline.data_ptr<float>());
  // The outputs are host memory the kernel writes over the link.
  at::cuda::getCurrentCUDAStream().synchronize();
}

// ---- LSTM serve step ------------------------------------------------------

namespace {
int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }
}  // namespace

// LDS of one workgroup of lstm_serve_layer_kernel: the bf16 A tile and the
// four waves' partial sums.
static size_t lstm_layer_lds_bytes(int64_t Kp) {
  return (size_t)kLstmTile * (size_t)(Kp + kLstmRowPad) * 2 +
         (size_t)(kLstmThreads / 64) * 4 * kLstmTile * kLstmTile *
             sizeof(float);
}

bool lstm_serve_layer_fits(int64_t I, int64_t H) {
  if (I < 1 || H < 1) return false;
  return lstm_layer_lds_bytes(round_up(I, 32) + round_up(H, 32)) <= 64 * 1024;
}

LstmLayerPack pack_lstm_layer(const torch::Tensor& w_ih,
                              const torch::Tensor& w_hh,
                              const torch::Tensor& b_ih,
                              const torch::Tensor& b_hh) {
  TORCH_CHECK(w_ih.is_cuda() && w_ih.dim() == 2 && w_hh.dim() == 2 &&
                  w_ih.scalar_type() == torch::kFloat32 &&
                  w_hh.scalar_type() == torch::kFloat32,
              "lstm pack: f32 GPU weight matrices expected");
  LstmLayerPack p;
  p.H = w_hh.size(1);
  p.I = w_ih.size(1);
  TORCH_CHECK(w_ih.size(0) == 4 * p.H && w_hh.size(0) == 4 * p.H &&
                  b_ih.numel() == 4 * p.H && b_hh.numel() == 4 * p.H,
              "lstm pack: weights disagree on the hidden size");
  p.Ip = round_up(p.I, 32);
  p.Kp = p.Ip + round_up(p.H, 32);
  p.Hn = round_up(p.H, kLstmTile);
  auto bf = w_ih.options().dtype(torch::kBFloat16);
  p.w = torch::zeros({4, p.Hn, p.Kp}, bf);
  p.w.narrow(1, 0, p.H).narrow(2, 0, p.I).copy_(w_ih.reshape({4, p.H, p.I}));
  p.w.narrow(1, 0, p.H).narrow(2, p.Ip, p.H).copy_(w_hh.reshape({4, p.H, p.H}));
  p.bias = torch::zeros({4, p.Hn}, w_ih.options());
  p.bias.narrow(1, 0, p.H).copy_((b_ih + b_hh).reshape({4, p.H}));
  return p;
}

void launch_lstm_stage_state(const float* const* state_in,
                             const uint8_t* const* done_src, int64_t b,
                             int64_t n_floats, float* staged) {
  TORCH_CHECK(b >= 1 && n_floats >= 1 && n_floats < (int64_t(1) << 31),
              "lstm stage: bad batch or state size");
  TORCH_CHECK(state_in != nullptr && done_src != nullptr && staged != nullptr,
              "lstm stage: null argument");
  hipLaunchKernelGGL(lstm_stage_state_kernel, dim3((uint32_t)b), dim3(256), 0,
                     at::cuda::getCurrentCUDAStream(), state_in, done_src,
                     (int)n_floats, staged);
  const hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "lstm_stage_state launch: ",
              hipGetErrorString(err));
}

void launch_lstm_serve_layer(float* const* state_out, const float* staged,
                             const float* in, int64_t in_stride,
                             const float* rew, const LstmLayerPack& p,
                             int64_t b, int64_t layer, int64_t L,
                             float* h_out) {
  TORCH_CHECK(b >= 1 && layer >= 0 && layer < L, "lstm serve: bad batch/layer");
  TORCH_CHECK(state_out != nullptr && staged != nullptr && in != nullptr &&
                  h_out != nullptr,
              "lstm serve: null argument");
  TORCH_CHECK(p.w.defined() && p.w.is_contiguous() &&
                  p.w.numel() == 4 * p.Hn * p.Kp && p.Kp % 32 == 0 &&
                  p.Ip % 32 == 0 && p.Hn % kLstmTile == 0 && p.I <= p.Ip &&
                  p.Ip + p.H <= p.Kp && p.H <= p.Hn &&
                  p.bias.numel() == 4 * p.Hn,
              "lstm serve: inconsistent weight pack");
  TORCH_CHECK(in_stride >= (rew != nullptr ? p.I - 1 : p.I),
              "lstm serve: input rows shorter than the layer's input");
  const int64_t mtiles = (b + kLstmTile - 1) / kLstmTile;
  TORCH_CHECK(mtiles <= 65535, "lstm serve: batch too large");
  const size_t lds = lstm_layer_lds_bytes(p.Kp);
  TORCH_CHECK(lds <= 64 * 1024, "lstm serve: layer too wide for one LDS tile");
  hipLaunchKernelGGL(
      lstm_serve_layer_kernel, dim3((uint32_t)(p.Hn / kLstmTile),
                                    (uint32_t)mtiles),
      dim3(kLstmThreads), lds, at::cuda::getCurrentCUDAStream(), state_out,
      staged, in, rew,
      reinterpret_cast<const __bf16*>(p.w.data_ptr()), p.bias.data_ptr<float>(),
      (int)b, (int)layer, (int)L, (int)p.H, (int)p.I, (int)in_stride,
      (int)p.Ip, (int)p.Kp, (int)p.Hn, h_out);
  const hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, "lstm_serve_layer launch: ",
              hipGetErrorString(err));
}

std::vector<torch::Tensor> lstm_serve_step(
    torch::Tensor x, torch::Tensor rew, std::vector<torch::Tensor> lstm_weights,
    torch::Tensor policy_w, torch::Tensor policy_b, torch::Tensor base_w,
    torch::Tensor base_b, torch::Tensor state_block,
    std::vector<int64_t> in_offsets, std::vector<int64_t> out_offsets,
    torch::Tensor done_slab, std::vector<int64_t> done_offsets, int64_t cap,
    bool greedy, int64_t seed) {
  const int64_t b = (int64_t)in_offsets.size();
  TORCH_CHECK(state_block.device().is_cpu() &&
                  state_block.scalar_type() == torch::kFloat32 &&
                  state_block.is_contiguous() && state_block.is_pinned(),
              "lstm_serve_step: state block must be a contiguous pinned "
              "float32 tensor");
  TORCH_CHECK(done_slab.device().is_cpu() &&
                  done_slab.scalar_type() == torch::kUInt8 &&
                  done_slab.is_contiguous() && done_slab.is_pinned(),
              "lstm_serve_step: done slab must be a contiguous pinned uint8 "
              "tensor");
  TORCH_CHECK(b >= 1 && out_offsets.size() == in_offsets.size() &&
                  done_offsets.size() == in_offsets.size() && cap >= b,
              "lstm_serve_step: need 1 <= b <= cap offsets of each kind");
  TORCH_CHECK(!lstm_weights.empty() && lstm_weights.size() % 4 == 0,
              "lstm_serve_step: four weight tensors per layer");
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.is_contiguous() &&
                  x.scalar_type() == torch::kFloat32 && x.size(0) >= b &&
                  rew.is_cuda() && rew.is_contiguous() &&
                  rew.scalar_type() == torch::kFloat32 && rew.numel() >= b,
              "lstm_serve_step: x [n, D] and rew [n] f32 on the GPU, n >= b");
  at::cuda::CUDAGuard device_guard(x.device());
  const int64_t L = (int64_t)lstm_weights.size() / 4;
  TORCH_CHECK(lstm_weights[1].dim() == 2, "lstm_serve_step: w_hh is [4H, H]");
  const int64_t H = lstm_weights[1].size(1);
  // The one writer of addresses the kernels follow; it checks all of them,
  // before anything is launched.
  auto table = torch::empty({3 * b}, torch::TensorOptions()
                                         .dtype(torch::kInt64)
                                         .pinned_memory(true));
  int64_t* t = table.data_ptr<int64_t>();
  auto** in_tab = reinterpret_cast<const float**>(t);
  auto** out_tab = reinterpret_cast<float**>(t + b);
  auto** done_tab = reinterpret_cast<const uint8_t**>(t + 2 * b);
  const auto* sbase = reinterpret_cast<const uint8_t*>(state_block.data_ptr());
  const uint8_t* dbase = done_slab.data_ptr<uint8_t>();
  std::vector<uintptr_t> scratch;
  build_state_table(
      b, [&](int64_t r) { return sbase + in_offsets[r]; },
      [&](int64_t r) { return sbase + out_offsets[r]; },
      [&](int64_t r) { return dbase + done_offsets[r]; }, 2 * L * H, sbase,
      state_block.numel() * 4, dbase, done_slab.numel(), scratch, in_tab,
      out_tab, done_tab);
  std::vector<LstmLayerPack> packs;
  for (int64_t l = 0; l < L; ++l) {
    packs.push_back(pack_lstm_layer(lstm_weights[4 * l], lstm_weights[4 * l + 1],
                                    lstm_weights[4 * l + 2],
                                    lstm_weights[4 * l + 3]));
    TORCH_CHECK(packs[l].H == H &&
                    packs[l].I == (l == 0 ? x.size(1) + 1 : H),
                "lstm_serve_step: layer ", l, " does not fit its input");
  }
  auto dopts = torch::TensorOptions().device(x.device());
  auto hopts = torch::TensorOptions().pinned_memory(true);
  const int64_t A = policy_w.size(0);
  std::vector<torch::Tensor> hs;
  for (int64_t l = 0; l < L; ++l) {
    hs.push_back(torch::full({cap, H}, -7.0f, dopts.dtype(torch::kFloat32)));
  }
  auto action = torch::full({cap}, -7, hopts.dtype(torch::kInt64));
  auto logits = torch::full({cap, A}, -7.0f, hopts.dtype(torch::kFloat32));
  auto baseline = torch::full({cap}, -7.0f, hopts.dtype(torch::kFloat32));
  auto staged = torch::empty({cap, 2 * L * H}, dopts.dtype(torch::kFloat32));
  launch_lstm_stage_state(in_tab, done_tab, b, 2 * L * H,
                          staged.data_ptr<float>());
  for (int64_t l = 0; l < L; ++l) {
    launch_lstm_serve_layer(
        out_tab, staged.data_ptr<float>(),
        l == 0 ? x.data_ptr<float>() : hs[l - 1].data_ptr<float>(),
        l == 0 ? x.size(1) : H, l == 0 ? rew.data_ptr<float>() : nullptr,
        packs[l], b, l, L, hs[l].data_ptr<float>());
  }
  launch_heads_sample(hs[L - 1].data_ptr<float>(), nullptr, H, policy_w,
                      policy_b, base_w, base_b, b, greedy, seed,
                      action.data_ptr<int64_t>(), logits.data_ptr<float>(),
                      baseline.data_ptr<float>());
  // Table, state block and done slab are read (and the block written) in
  // place: nothing may go away or change under the kernels.
  at::cuda::getCurrentCUDAStream().synchronize();
  std::vector<torch::Tensor> out{action, logits, baseline};
  for (auto& h : hs) out.push_back(h);
  return out;
}

}  // namespace tbruntime
