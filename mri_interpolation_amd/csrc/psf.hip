// PsfSirenNet's point-spread-function ops (reference models.py:397-539):
//   psf_expand     x_to_psf_x: x.repeat_interleave(S, 0) + psf_coordinates.repeat(n, 1)   models.py:520-526
//   psf_reduce     psf_conv(z.T).T, the Conv1d of kernel S and stride S (and the backward of the expansion)
//                                                                                         models.py:535
//   psf_broadcast  the Conv1d's backward                                                  models.py:535
//   psf_mse_loss   psf_conv + F.mse_loss(z, y) + their backward, the training step's loss models.py:529-537
//
// Determinism: every sum over the S samples of a target is owned by ONE segment of lanes (a wave, or a
// half-wave when S <= 32); lane j takes samples j, j + G, j + 2G, ... in that order, in float64, and the
// G lane sums meet in a xor butterfly (a + b == b + a: every lane ends with the same bits).  Which
// workgroup runs a target never matters, so the results do not depend on the grid.  The loss is a
// second, single-workgroup pass over the n reduced values in a fixed order (float64).
#include <math.h>

#include <algorithm>

#include "common.h"

namespace mri {
namespace {

constexpr int kPsfMaxSamples = 4096;
constexpr int kPsfMaxDim = 8;
constexpr int kThreads = 256;
constexpr int kLossThreads = 1024;

// float64 sum over the G lanes of a segment (G = 32 or 64), the same bits in every lane
template <int G>
__device__ __forceinline__ double segment_sum(double v) {
#pragma unroll
  for (int m = G / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, G);
  return v;
}

// ---------------------------------------------------------------------------------- expansion
// out[(b S + k) D + c] = x[b D + c] + off[k D + c]: four consecutive output floats per thread, one
// 16-byte store where the output is aligned (a store stream; the inputs are tiny and stay in cache).
// I: the index type, 32-bit whenever the output allows it (64-bit divisions are long software sequences)
template <typename I>
__global__ __launch_bounds__(kThreads) void psf_expand_kernel(const float* __restrict__ x,
                                                              const float* __restrict__ off,
                                                              int64_t total, int S, int D,
                                                              float* __restrict__ out, int vec) {
  const int64_t stride = (int64_t)gridDim.x * kThreads * 4;
  for (int64_t e0 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 4; e0 < total; e0 += stride) {
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t e = e0 + j;
      if (e < total) {
        const I r = (I)e / (I)D;
        const int c = (int)((I)e - r * (I)D);
        const I b = r / (I)S;
        const int k = (int)(r - b * (I)S);
        v[j] = x[(int64_t)b * D + c] + off[k * D + c];
      }
    }
    if (vec && e0 + 3 < total) {
      *reinterpret_cast<float4*>(out + e0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      for (int j = 0; j < 4 && e0 + j < total; ++j) out[e0 + j] = v[j];
    }
  }
}

// ---------------------------------------------------------------------------------- reduction
// out[b C + c] = sum_k w_k in[(b S + k) C + c] (w == NULL: w_k = 1), one segment of G lanes per target
template <int G>
__global__ __launch_bounds__(kThreads) void psf_reduce_kernel(const float* __restrict__ in, int64_t n,
                                                              int S, int C, const float* __restrict__ w,
                                                              float* __restrict__ out) {
  const int lane = threadIdx.x % G;
  const int64_t segs = (int64_t)gridDim.x * (kThreads / G);
  for (int64_t b = (int64_t)blockIdx.x * (kThreads / G) + threadIdx.x / G; b < n; b += segs) {
    const float* src = in + b * S * C;
    for (int c = 0; c < C; ++c) {
      double acc = 0.0;
      for (int k = lane; k < S; k += G) {
        const double z = (double)src[(int64_t)k * C + c];
        acc += w ? (double)w[k] * z : z;
      }
      acc = segment_sum<G>(acc);
      if (lane == 0) out[b * C + c] = (float)acc;
    }
  }
}

// dz[b S + k] = scale w_k g[b]
__global__ __launch_bounds__(kThreads) void psf_broadcast_kernel(const float* __restrict__ g, int64_t total,
                                                                 int S, const float* __restrict__ w,
                                                                 float scale, float* __restrict__ dz) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) {
    const int64_t b = e / S;
    const int k = (int)(e - b * S);
    dz[e] = (scale * w[k]) * g[b];
  }
}

// ---------------------------------------------------------------------------------- training loss
// zbar_b = sum_k w_k z[b S + k] (float64, then rounded as the Conv1d's f32 output), diff = zbar_b - y_b;
// dz[b S + k] = w_k * (diff * gs) with gs = 2 / (n_total grad_divisor): autograd's order (mse_loss backward,
// then the Conv1d's backward)
template <int G>
__global__ __launch_bounds__(kThreads) void psf_loss_grad_kernel(const float* __restrict__ z,
                                                                 const float* __restrict__ target, int64_t n,
                                                                 int S, const float* __restrict__ w, float gs,
                                                                 float* __restrict__ zbar,
                                                                 float* __restrict__ dz) {
  const int lane = threadIdx.x % G;
  const int64_t segs = (int64_t)gridDim.x * (kThreads / G);
  for (int64_t b = (int64_t)blockIdx.x * (kThreads / G) + threadIdx.x / G; b < n; b += segs) {
    const float* src = z + b * S;
    double acc = 0.0;
    for (int k = lane; k < S; k += G) acc += (double)w[k] * (double)src[k];
    const float zb = (float)segment_sum<G>(acc);
    const float g = (zb - target[b]) * gs;
    if (lane == 0) zbar[b] = zb;
    if (dz) {
      float* dst = dz + b * S;
      for (int k = lane; k < S; k += G) dst[k] = w[k] * g;
    }
  }
}

// loss_out[0] += sum_b (zbar_b - y_b)^2 / n_total: one workgroup, thread t sums b = t, t + T, ... in order,
// then a fixed tree over the threads (float64 throughout)
__global__ __launch_bounds__(kLossThreads) void psf_loss_sum_kernel(const float* __restrict__ zbar,
                                                                    const float* __restrict__ target, int64_t n,
                                                                    double inv_total, float* __restrict__ loss_out) {
  __shared__ double part[kLossThreads];
  double acc = 0.0;
  for (int64_t b = threadIdx.x; b < n; b += kLossThreads) {
    const float diff = zbar[b] - target[b];
    acc += (double)diff * (double)diff;
  }
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int s = kLossThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss_out[0] += (float)(part[0] * inv_total);
}

int segment_blocks(int64_t n, int G) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, kThreads / G), 8192));
}

}  // namespace
}  // namespace mri

using namespace mri;

extern "C" int mri_psf_expand(const float* x, int64_t n, int32_t dim_in, const float* offsets, int32_t S,
                              float* x_psf, void* stream) {
  MRI_REQUIRE(n >= 0, "negative n");
  MRI_REQUIRE(S >= 1 && S <= kPsfMaxSamples, "PSF samples S = %d outside [1, %d]", S, kPsfMaxSamples);
  MRI_REQUIRE(dim_in >= 1 && dim_in <= kPsfMaxDim, "dim_in = %d outside [1, %d]", dim_in, kPsfMaxDim);
  if (n == 0) return MRI_OK;
  MRI_REQUIRE(x && offsets && x_psf, "NULL device pointer");
  const int64_t total = n * S * dim_in;
  const int vec = (reinterpret_cast<uintptr_t>(x_psf) & 15) == 0;
  const int blocks = (int)std::min<int64_t>(ceil_div(ceil_div(total, 4), kThreads), 8192);
  if (total + 4 <= (int64_t)UINT32_MAX) {
    hipLaunchKernelGGL(psf_expand_kernel<uint32_t>, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, x,
                       offsets, total, S, dim_in, x_psf, vec);
  } else {
    hipLaunchKernelGGL(psf_expand_kernel<int64_t>, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, x,
                       offsets, total, S, dim_in, x_psf, vec);
  }
  return check_launch("psf_expand_kernel");
}

extern "C" int mri_psf_reduce(const float* in, int64_t n, int32_t S, int32_t C, const float* w, float* out,
                              void* stream) {
  MRI_REQUIRE(n >= 0, "negative n");
  MRI_REQUIRE(S >= 1 && S <= kPsfMaxSamples, "PSF samples S = %d outside [1, %d]", S, kPsfMaxSamples);
  MRI_REQUIRE(C >= 1 && C <= kPsfMaxDim, "channels C = %d outside [1, %d]", C, kPsfMaxDim);
  if (n == 0) return MRI_OK;
  MRI_REQUIRE(in && out, "NULL device pointer");
  if (S <= 32) {
    hipLaunchKernelGGL(psf_reduce_kernel<32>, dim3(segment_blocks(n, 32)), dim3(kThreads), 0,
                       (hipStream_t)stream, in, n, S, C, w, out);
  } else {
    hipLaunchKernelGGL(psf_reduce_kernel<64>, dim3(segment_blocks(n, 64)), dim3(kThreads), 0,
                       (hipStream_t)stream, in, n, S, C, w, out);
  }
  return check_launch("psf_reduce_kernel");
}

extern "C" int mri_psf_broadcast(const float* g, int64_t n, int32_t S, const float* w, float scale, float* dz,
                                 void* stream) {
  MRI_REQUIRE(n >= 0, "negative n");
  MRI_REQUIRE(S >= 1 && S <= kPsfMaxSamples, "PSF samples S = %d outside [1, %d]", S, kPsfMaxSamples);
  if (n == 0) return MRI_OK;
  MRI_REQUIRE(g && w && dz, "NULL device pointer");
  const int64_t total = n * S;
  const int blocks = (int)std::min<int64_t>(ceil_div(total, kThreads), 8192);
  hipLaunchKernelGGL(psf_broadcast_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, g, total, S,
                     w, scale, dz);
  return check_launch("psf_broadcast_kernel");
}

extern "C" int mri_psf_mse_loss(const float* z, const float* target, int64_t n, int64_t n_total, int32_t S,
                                const float* w, float grad_divisor, float* zbar_out, float* loss_out,
                                float* dz, void* stream) {
  MRI_REQUIRE(n >= 0 && n <= n_total, "need 0 <= n <= n_total (got %lld, %lld)", (long long)n,
              (long long)n_total);
  MRI_REQUIRE(S >= 1 && S <= kPsfMaxSamples, "PSF samples S = %d outside [1, %d]", S, kPsfMaxSamples);
  MRI_REQUIRE(grad_divisor > 0.f, "grad_divisor must be positive");
  if (n == 0) return MRI_OK;
  MRI_REQUIRE(z && target && w && zbar_out && loss_out, "NULL device pointer");
  const float gs = (float)(2.0 / ((double)n_total * (double)grad_divisor));
  hipStream_t st = (hipStream_t)stream;
  if (S <= 32) {
    hipLaunchKernelGGL(psf_loss_grad_kernel<32>, dim3(segment_blocks(n, 32)), dim3(kThreads), 0, st, z, target,
                       n, S, w, gs, zbar_out, dz);
  } else {
    hipLaunchKernelGGL(psf_loss_grad_kernel<64>, dim3(segment_blocks(n, 64)), dim3(kThreads), 0, st, z, target,
                       n, S, w, gs, zbar_out, dz);
  }
  if (int rc = check_launch("psf_loss_grad_kernel")) return rc;
  hipLaunchKernelGGL(psf_loss_sum_kernel, dim3(1), dim3(kLossThreads), 0, st, zbar_out, target, n,
                     1.0 / (double)n_total, loss_out);
  return check_launch("psf_loss_sum_kernel");
}
