// Train-mode BatchNorm1d + activation of the reference's default HashMLP decoder block
// (Linear -> BatchNorm1d -> GELU -> Dropout(0), reference models.py:728-737; torch.nn.BatchNorm1d):
//   bn_stats         batch mean / biased variance per feature, the running-buffer update of train(),
//                    and (mean, invstd) into a save area
//   bn_act_forward   y = act(gamma (z - mean) invstd + beta), training form (save area) or eval form
//                    (running statistics)
//   bn_act_backward  g = dy act'(u), dbeta = sum g, dgamma = sum g xhat,
//                    dz = gamma invstd (g - dbeta / n - xhat dgamma / n)
//
// What the backward keeps: nothing but z (the Linear's output, which the step holds anyway) and the 2 C
// floats of the save area.  xhat = (z - mean) invstd and u = gamma xhat + beta are recomputed with the
// forward's own expressions (no contraction: the same bits), act'(u) is evaluated once, in the reduction
// pass, which leaves g = dy act'(u) in the dz buffer for the second pass.
//
// Layout: z (n, C) row-major.  A workgroup of 256 threads is a TX x TY tile, TX = the column groups (four
// columns per thread with 16-byte loads where C, the leading dimensions and the pointers allow it, else
// one), TY = 256 / TX rows: for C = 64 a wave covers four whole rows, for C = 1 it is one lane per row.
// Every thread keeps its columns for all its rows, so per-feature partial sums stay in registers.
//
// Determinism: the rows are cut into `chunks` contiguous chunks (a function of n and C only).  Inside a
// chunk thread (tx, ty) adds rows ty, ty + TY, ... in increasing order, in float64; the TY partial sums of
// a column meet in a fixed LDS tree; the chunk sums are written out (no atomics) and a second kernel adds
// them, 16 lanes per column taking chunks j, j + 16, ... in order, then a xor butterfly (a + b == b + a).
// Which workgroup runs when never matters: same inputs, same bits.
//
// Variance: the sums are taken of d = z - z[0, c] (exact in float64) and d^2 (an f32 x f32 product is exact
// in float64), so var = (S2 - S1^2 / n) / n loses nothing to a mean that dwarfs the spread.
#include <math.h>

#include <algorithm>

#include "common.h"
#include "device_math.h"

namespace mri {
namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 4;         // rows in flight per thread
constexpr int kMaxChunks = 1024;   // row chunks of the two reduction passes
constexpr int kChunkElems = 4096;  // a chunk is worth at least this many elements
constexpr int kFinLanes = 16;      // lanes per column of the finalising kernels
constexpr int kMaxFeatures = 1024;

struct Tile {
  int V, tx_bits, tiles;
};

inline Tile tile_for(int C, bool vec) {
  Tile t;
  t.V = vec ? 4 : 1;
  const int groups = C / t.V;
  t.tx_bits = 0;
  while ((1 << t.tx_bits) < groups && t.tx_bits < 8) ++t.tx_bits;
  t.tiles = (int)ceil_div(groups, 1 << t.tx_bits);
  return t;
}

inline int chunks_for(int64_t n, int C) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(n * C / kChunkElems, kMaxChunks));
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int V>
__device__ __forceinline__ void load_v(const float* p, float* v) {
  if constexpr (V == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
    v[0] = p[0];
  }
}

// per-column constants (read once per thread): plain loads, so that only the matrices need 16-byte alignment
// (gamma / beta and their gradients are views into the optimiser's flat buffers at any 4-byte offset)
template <int V>
__device__ __forceinline__ void load_c(const float* p, float* v) {
#pragma unroll
  for (int j = 0; j < V; ++j) v[j] = p[j];
}

template <int V>
__device__ __forceinline__ void store_v(float* p, const float* v) {
  if constexpr (V == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    p[0] = v[0];
  }
}

template <int ACT>
__device__ __forceinline__ float act_f(float u) {
  if constexpr (ACT == MRI_ACT_RELU) return u > 0.f ? u : 0.f;
  if constexpr (ACT == MRI_ACT_GELU) return gelu_f(u);
  return u;
}

template <int ACT>
__device__ __forceinline__ float act_grad_f(float u) {
  if constexpr (ACT == MRI_ACT_RELU) return u > 0.f ? 1.f : 0.f;
  if constexpr (ACT == MRI_ACT_GELU) return gelu_grad_f(u);
  return 1.f;
}

// the TY partial sums of every column of the tile meet in sh[q][ty = 0]: a fixed tree over ty
template <int Q>
__device__ __forceinline__ void tile_tree(double (*sh)[kThreads], const double* acc, int tx_bits) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int q = 0; q < Q; ++q) sh[q][tid] = acc[q];
  for (int s = (kThreads >> tx_bits) / 2; s > 0; s >>= 1) {
    __syncthreads();
    if ((tid >> tx_bits) < s) {
#pragma unroll
      for (int q = 0; q < Q; ++q) sh[q][tid] += sh[q][tid + (s << tx_bits)];
    }
  }
  __syncthreads();
}

// ------------------------------------------------------------------------------------ statistics
// part[(chunk * 2 + 0) * C + c] = sum over the chunk's rows of d = z - z[0, c], [.. + 1 ..] of d^2
template <int V>
__global__ __launch_bounds__(kThreads) void bn_stats_partial_kernel(const float* __restrict__ z, int64_t ldz,
                                                                    int64_t n, int C, int tx_bits,
                                                                    int64_t chunk, double* __restrict__ part) {
  __shared__ double sh[2 * V][kThreads];
  const int tx = threadIdx.x & ((1 << tx_bits) - 1), ty = threadIdx.x >> tx_bits;
  const int TY = kThreads >> tx_bits;
  const int col = ((blockIdx.y << tx_bits) + tx) * V;
  const int64_t r0 = (int64_t)blockIdx.x * chunk;
  const int64_t r1 = r0 + chunk < n ? r0 + chunk : n;
  double acc[2 * V];
#pragma unroll
  for (int q = 0; q < 2 * V; ++q) acc[q] = 0.0;
  if (col < C) {
    float k[V];
    load_v<V>(z + col, k);
    for (int64_t r = r0 + ty; r < r1; r += (int64_t)TY * kUnroll) {
      float v[kUnroll][V];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int64_t rr = r + (int64_t)u * TY;
        if (rr < r1) load_v<V>(z + rr * ldz + col, v[u]);
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        if (r + (int64_t)u * TY < r1) {
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const double d = (double)v[u][j] - (double)k[j];
            acc[j] += d;
            acc[V + j] += d * d;
          }
        }
      }
    }
  }
  tile_tree<2 * V>(sh, acc, tx_bits);
  if (ty == 0 && col < C) {
    double* dst = part + (int64_t)blockIdx.x * 2 * C + col;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      dst[j] = sh[j][threadIdx.x];
      dst[C + j] = sh[V + j][threadIdx.x];
    }
  }
}

// the chunk sums of column c, added by kFinLanes lanes in a fixed order; every lane returns the same bits
__device__ __forceinline__ void column_sums(const double* __restrict__ part, int chunks, int C, int c, int lane,
                                            double* s_a, double* s_b) {
  double a = 0.0, b = 0.0;
  if (c < C) {
    for (int k = lane; k < chunks; k += kFinLanes) {
      a += part[(int64_t)k * 2 * C + c];
      b += part[(int64_t)k * 2 * C + C + c];
    }
  }
#pragma unroll
  for (int m = kFinLanes / 2; m > 0; m >>= 1) {
    a += __shfl_xor(a, m, kFinLanes);
    b += __shfl_xor(b, m, kFinLanes);
  }
  *s_a = a, *s_b = b;
}

__global__ __launch_bounds__(kThreads) void bn_stats_final_kernel(const double* __restrict__ part, int chunks,
                                                                  const float* __restrict__ z, int64_t n, int C,
                                                                  double momentum, double eps,
                                                                  float* __restrict__ running_mean,
                                                                  float* __restrict__ running_var,
                                                                  long long* __restrict__ tracked,
                                                                  float* __restrict__ save) {
  const int c = blockIdx.x * (kThreads / kFinLanes) + threadIdx.x / kFinLanes;
  const int lane = threadIdx.x % kFinLanes;
  double s1, s2;
  column_sums(part, chunks, C, c, lane, &s1, &s2);
  if (c < C && lane == 0) {
    const double inv_n = 1.0 / (double)n;
    const double mean = (double)z[c] + s1 * inv_n;
    const double var = fmax(0.0, (s2 - s1 * s1 * inv_n) * inv_n);
    save[c] = (float)mean;
    save[C + c] = (float)(1.0 / sqrt(var + eps));
    if (running_mean) running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * mean);
    if (running_var) {
      const double unbiased = var * ((double)n / (double)(n - 1));
      running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * unbiased);
    }
  }
  if (tracked && blockIdx.x == 0 && threadIdx.x == 0) tracked[0] += 1;
}

// ------------------------------------------------------------------------------------ forward
// eval == 0: (mean_src, scale_src) = the batch's (mean, invstd); else the running statistics, invstd =
// 1 / sqrt(var + eps).  y may be z.
template <int V, int ACT>
__global__ __launch_bounds__(kThreads) void bn_act_forward_kernel(const float* z, int64_t ldz, int64_t n, int C,
                                                                  int tx_bits, const float* __restrict__ mean_src,
                                                                  const float* __restrict__ scale_src, int eval,
                                                                  float eps, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, float* y,
                                                                  int64_t ldy) {
  const int tx = threadIdx.x & ((1 << tx_bits) - 1), ty = threadIdx.x >> tx_bits;
  const int TY = kThreads >> tx_bits;
  const int col = ((blockIdx.y << tx_bits) + tx) * V;
  if (col >= C) return;
  float mean[V], invstd[V], ga[V], be[V];
  load_c<V>(mean_src + col, mean);
  load_c<V>(scale_src + col, invstd);
  load_c<V>(gamma + col, ga);
  load_c<V>(beta + col, be);
  if (eval) {
#pragma unroll
    for (int j = 0; j < V; ++j) invstd[j] = 1.0f / sqrtf(invstd[j] + eps);
  }
  const int64_t stride = (int64_t)gridDim.x * TY * kUnroll;
  for (int64_t r = (int64_t)blockIdx.x * TY * kUnroll + ty; r < n; r += stride) {
    float v[kUnroll][V];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t rr = r + (int64_t)u * TY;
      if (rr < n) load_v<V>(z + rr * ldz + col, v[u]);
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t rr = r + (int64_t)u * TY;
      if (rr < n) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float xhat = (v[u][j] - mean[j]) * invstd[j];
          v[u][j] = act_f<ACT>(ga[j] * xhat + be[j]);
        }
        store_v<V>(y + rr * ldy + col, v[u]);
      }
    }
  }
}

// ------------------------------------------------------------------------------------ backward
// pass 1: g = dy act'(u) into dz (dz may be dy); part = chunk sums of g and g xhat
template <int V, int ACT>
__global__ __launch_bounds__(kThreads) void bn_bwd_partial_kernel(const float* dy, int64_t lddy,
                                                                  const float* __restrict__ z, int64_t ldz,
                                                                  int64_t n, int C, int tx_bits, int64_t chunk,
                                                                  const float* __restrict__ save,
                                                                  const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, float* dz,
                                                                  int64_t lddz, double* __restrict__ part) {
  __shared__ double sh[2 * V][kThreads];
  const int tx = threadIdx.x & ((1 << tx_bits) - 1), ty = threadIdx.x >> tx_bits;
  const int TY = kThreads >> tx_bits;
  const int col = ((blockIdx.y << tx_bits) + tx) * V;
  const int64_t r0 = (int64_t)blockIdx.x * chunk;
  const int64_t r1 = r0 + chunk < n ? r0 + chunk : n;
  const bool write_g = ACT != MRI_ACT_IDENTITY || dz != dy;
  double acc[2 * V];
#pragma unroll
  for (int q = 0; q < 2 * V; ++q) acc[q] = 0.0;
  if (col < C) {
    float mean[V], invstd[V], ga[V], be[V];
    load_c<V>(save + col, mean);
    load_c<V>(save + C + col, invstd);
    load_c<V>(gamma + col, ga);
    load_c<V>(beta + col, be);
    for (int64_t r = r0 + ty; r < r1; r += (int64_t)TY * kUnroll) {
      float v[kUnroll][V], g[kUnroll][V];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int64_t rr = r + (int64_t)u * TY;
        if (rr < r1) {
          load_v<V>(z + rr * ldz + col, v[u]);
          load_v<V>(dy + rr * lddy + col, g[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int64_t rr = r + (int64_t)u * TY;
        if (rr < r1) {
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const float xhat = (v[u][j] - mean[j]) * invstd[j];
            g[u][j] = g[u][j] * act_grad_f<ACT>(ga[j] * xhat + be[j]);
            acc[j] += (double)g[u][j];
            acc[V + j] += (double)g[u][j] * (double)xhat;
          }
          if (write_g) store_v<V>(dz + rr * lddz + col, g[u]);
        }
      }
    }
  }
  tile_tree<2 * V>(sh, acc, tx_bits);
  if (ty == 0 && col < C) {
    double* dst = part + (int64_t)blockIdx.x * 2 * C + col;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      dst[j] = sh[j][threadIdx.x];
      dst[C + j] = sh[V + j][threadIdx.x];
    }
  }
}

// dbeta / dgamma (written or added to) and the two batch means pass 2 needs
__global__ __launch_bounds__(kThreads) void bn_bwd_final_kernel(const double* __restrict__ part, int chunks,
                                                                int64_t n, int C, float* __restrict__ d_gamma,
                                                                float* __restrict__ d_beta, int overwrite,
                                                                float* __restrict__ means) {
  const int c = blockIdx.x * (kThreads / kFinLanes) + threadIdx.x / kFinLanes;
  const int lane = threadIdx.x % kFinLanes;
  double sg, sgx;
  column_sums(part, chunks, C, c, lane, &sg, &sgx);
  if (c < C && lane == 0) {
    d_beta[c] = overwrite ? (float)sg : d_beta[c] + (float)sg;
    d_gamma[c] = overwrite ? (float)sgx : d_gamma[c] + (float)sgx;
    means[c] = (float)(sg / (double)n);
    means[C + c] = (float)(sgx / (double)n);
  }
}

// pass 2: dz = gamma invstd (g - mean(g) - xhat mean(g xhat)), g read from dz
template <int V>
__global__ __launch_bounds__(kThreads) void bn_bwd_dz_kernel(const float* __restrict__ z, int64_t ldz, int64_t n,
                                                             int C, int tx_bits, const float* __restrict__ save,
                                                             const float* __restrict__ gamma,
                                                             const float* __restrict__ means, float* dz,
                                                             int64_t lddz) {
  const int tx = threadIdx.x & ((1 << tx_bits) - 1), ty = threadIdx.x >> tx_bits;
  const int TY = kThreads >> tx_bits;
  const int col = ((blockIdx.y << tx_bits) + tx) * V;
  if (col >= C) return;
  float mean[V], invstd[V], scale[V], mg[V], mgx[V];
  load_c<V>(save + col, mean);
  load_c<V>(save + C + col, invstd);
  load_c<V>(gamma + col, scale);
  load_c<V>(means + col, mg);
  load_c<V>(means + C + col, mgx);
#pragma unroll
  for (int j = 0; j < V; ++j) scale[j] = scale[j] * invstd[j];
  const int64_t stride = (int64_t)gridDim.x * TY * kUnroll;
  for (int64_t r = (int64_t)blockIdx.x * TY * kUnroll + ty; r < n; r += stride) {
    float v[kUnroll][V], g[kUnroll][V];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t rr = r + (int64_t)u * TY;
      if (rr < n) {
        load_v<V>(z + rr * ldz + col, v[u]);
        load_v<V>(dz + rr * lddz + col, g[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t rr = r + (int64_t)u * TY;
      if (rr < n) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float xhat = (v[u][j] - mean[j]) * invstd[j];
          g[u][j] = scale[j] * ((g[u][j] - mg[j]) - xhat * mgx[j]);
        }
        store_v<V>(dz + rr * lddz + col, g[u]);
      }
    }
  }
}

int64_t part_bytes(int64_t n, int C) { return (int64_t)chunks_for(n, C) * 2 * C * (int64_t)sizeof(double); }

int check_shape(int64_t n, int32_t C) {
  MRI_REQUIRE(n >= 2, "BatchNorm needs n >= 2 rows in training (got %lld)", (long long)n);
  MRI_REQUIRE(C >= 1 && C <= kMaxFeatures, "features C = %d outside [1, %d]", C, kMaxFeatures);
  return MRI_OK;
}

int elementwise_blocks(int64_t n, const Tile& t) {
  const int64_t rows = (int64_t)(kThreads >> t.tx_bits) * kUnroll;
  return (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, rows), 2048 / t.tiles + 1));
}

bool bn_activation_ok(int a) { return a == MRI_ACT_IDENTITY || a == MRI_ACT_RELU || a == MRI_ACT_GELU; }

template <int V>
void launch_forward(int activation, dim3 grid, hipStream_t st, const float* z, int64_t ldz, int64_t n, int C,
                    int tx_bits, const float* mean_src, const float* scale_src, int eval, float eps,
                    const float* gamma, const float* beta, float* y, int64_t ldy) {
  switch (activation) {
    case MRI_ACT_RELU:
      hipLaunchKernelGGL((bn_act_forward_kernel<V, MRI_ACT_RELU>), grid, dim3(kThreads), 0, st, z, ldz, n, C,
                         tx_bits, mean_src, scale_src, eval, eps, gamma, beta, y, ldy);
      break;
    case MRI_ACT_GELU:
      hipLaunchKernelGGL((bn_act_forward_kernel<V, MRI_ACT_GELU>), grid, dim3(kThreads), 0, st, z, ldz, n, C,
                         tx_bits, mean_src, scale_src, eval, eps, gamma, beta, y, ldy);
      break;
    default:
      hipLaunchKernelGGL((bn_act_forward_kernel<V, MRI_ACT_IDENTITY>), grid, dim3(kThreads), 0, st, z, ldz, n, C,
                         tx_bits, mean_src, scale_src, eval, eps, gamma, beta, y, ldy);
  }
}

template <int V>
void launch_bwd_partial(int activation, dim3 grid, hipStream_t st, const float* dy, int64_t lddy, const float* z,
                        int64_t ldz, int64_t n, int C, int tx_bits, int64_t chunk, const float* save,
                        const float* gamma, const float* beta, float* dz, int64_t lddz, double* part) {
  switch (activation) {
    case MRI_ACT_RELU:
      hipLaunchKernelGGL((bn_bwd_partial_kernel<V, MRI_ACT_RELU>), grid, dim3(kThreads), 0, st, dy, lddy, z, ldz,
                         n, C, tx_bits, chunk, save, gamma, beta, dz, lddz, part);
      break;
    case MRI_ACT_GELU:
      hipLaunchKernelGGL((bn_bwd_partial_kernel<V, MRI_ACT_GELU>), grid, dim3(kThreads), 0, st, dy, lddy, z, ldz,
                         n, C, tx_bits, chunk, save, gamma, beta, dz, lddz, part);
      break;
    default:
      hipLaunchKernelGGL((bn_bwd_partial_kernel<V, MRI_ACT_IDENTITY>), grid, dim3(kThreads), 0, st, dy, lddy, z,
                         ldz, n, C, tx_bits, chunk, save, gamma, beta, dz, lddz, part);
  }
}

}  // namespace
}  // namespace mri

using namespace mri;

extern "C" int64_t mri_bn_workspace_bytes(int64_t n, int32_t C) {
  if (n < 1 || C < 1 || C > kMaxFeatures) return -1;
  return part_bytes(n, C) + 2 * (int64_t)C * (int64_t)sizeof(float);
}

extern "C" int mri_bn_stats(const float* z, int64_t ldz, int64_t n, int32_t C, double momentum, double eps,
                            float* running_mean, float* running_var, int64_t* num_batches_tracked, float* save,
                            void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = check_shape(n, C)) return rc;
  MRI_REQUIRE(ldz >= C, "ldz = %lld < C = %d", (long long)ldz, C);
  MRI_REQUIRE(momentum >= 0.0 && momentum <= 1.0 && eps >= 0.0, "momentum %g outside [0, 1] or eps %g < 0",
              momentum, eps);
  MRI_REQUIRE(z && save && workspace, "NULL device pointer");
  MRI_REQUIRE(workspace_bytes >= mri_bn_workspace_bytes(n, C) && aligned16(workspace),
              "workspace of %lld bytes: mri_bn_workspace_bytes asks for %lld, 16-byte aligned",
              (long long)workspace_bytes, (long long)mri_bn_workspace_bytes(n, C));
  const bool vec = C % 4 == 0 && ldz % 4 == 0 && aligned16(z);
  const Tile t = tile_for(C, vec);
  const int chunks = chunks_for(n, C);
  const int64_t chunk = ceil_div(n, chunks);
  double* part = static_cast<double*>(workspace);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(chunks, t.tiles);
  if (vec) {
    hipLaunchKernelGGL(bn_stats_partial_kernel<4>, grid, dim3(kThreads), 0, st, z, ldz, n, C, t.tx_bits, chunk,
                       part);
  } else {
    hipLaunchKernelGGL(bn_stats_partial_kernel<1>, grid, dim3(kThreads), 0, st, z, ldz, n, C, t.tx_bits, chunk,
                       part);
  }
  if (int rc = check_launch("bn_stats_partial_kernel")) return rc;
  hipLaunchKernelGGL(bn_stats_final_kernel, dim3((int)ceil_div(C, kThreads / kFinLanes)), dim3(kThreads), 0, st,
                     part, chunks, z, n, C, momentum, eps, running_mean, running_var,
                     reinterpret_cast<long long*>(num_batches_tracked), save);
  return check_launch("bn_stats_final_kernel");
}

extern "C" int mri_bn_act_forward(const float* z, int64_t ldz, int64_t n, int32_t C, const float* save,
                                  const float* running_mean, const float* running_var, double eps,
                                  const float* gamma, const float* beta, int32_t activation, float* y, int64_t ldy,
                                  void* stream) {
  MRI_REQUIRE(n >= 0, "negative n");
  MRI_REQUIRE(C >= 1 && C <= kMaxFeatures, "features C = %d outside [1, %d]", C, kMaxFeatures);
  MRI_REQUIRE(bn_activation_ok(activation), "bad activation %d (identity, ReLU or GELU)", activation);
  if (n == 0) return MRI_OK;
  MRI_REQUIRE(ldz >= C && ldy >= C, "leading dimension below C = %d", C);
  MRI_REQUIRE(z && y && gamma && beta, "NULL device pointer");
  MRI_REQUIRE(save || (running_mean && running_var),
              "neither batch statistics (save) nor running statistics were given");
  MRI_REQUIRE(y == z ? ldy == ldz : true, "y aliases z with another leading dimension");
  MRI_REQUIRE(eps >= 0.0, "eps %g < 0", eps);
  const int eval = save == nullptr;
  const float* mean_src = eval ? running_mean : save;
  const float* scale_src = eval ? running_var : save + C;
  const bool vec = C % 4 == 0 && ldz % 4 == 0 && ldy % 4 == 0 && aligned16(z) && aligned16(y);
  const Tile t = tile_for(C, vec);
  const dim3 grid(elementwise_blocks(n, t), t.tiles);
  hipStream_t st = (hipStream_t)stream;
  if (vec) {
    launch_forward<4>(activation, grid, st, z, ldz, n, C, t.tx_bits, mean_src, scale_src, eval, (float)eps, gamma,
                      beta, y, ldy);
  } else {
    launch_forward<1>(activation, grid, st, z, ldz, n, C, t.tx_bits, mean_src, scale_src, eval, (float)eps, gamma,
                      beta, y, ldy);
  }
  return check_launch("bn_act_forward_kernel");
}

extern "C" int mri_bn_act_backward(const float* dy, int64_t lddy, const float* z, int64_t ldz, int64_t n, int32_t C,
                                   const float* save, const float* gamma, const float* beta, int32_t activation,
                                   float* dz, int64_t lddz, float* d_gamma, float* d_beta, int32_t overwrite,
                                   void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = check_shape(n, C)) return rc;
  MRI_REQUIRE(bn_activation_ok(activation), "bad activation %d (identity, ReLU or GELU)", activation);
  MRI_REQUIRE(lddy >= C && ldz >= C && lddz >= C, "leading dimension below C = %d", C);
  MRI_REQUIRE(dy && z && save && gamma && beta && dz && d_gamma && d_beta && workspace, "NULL device pointer");
  MRI_REQUIRE(dz != z, "dz must not alias z (it may alias dy)");
  MRI_REQUIRE(dz == dy ? lddz == lddy : true, "dz aliases dy with another leading dimension");
  MRI_REQUIRE(workspace_bytes >= mri_bn_workspace_bytes(n, C) && aligned16(workspace),
              "workspace of %lld bytes: mri_bn_workspace_bytes asks for %lld, 16-byte aligned",
              (long long)workspace_bytes, (long long)mri_bn_workspace_bytes(n, C));
  double* part = static_cast<double*>(workspace);
  float* means = reinterpret_cast<float*>(static_cast<char*>(workspace) + part_bytes(n, C));
  const bool vec = C % 4 == 0 && lddy % 4 == 0 && ldz % 4 == 0 && lddz % 4 == 0 && aligned16(dy) && aligned16(z) &&
                   aligned16(dz);
  const Tile t = tile_for(C, vec);
  const int chunks = chunks_for(n, C);
  const int64_t chunk = ceil_div(n, chunks);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(chunks, t.tiles);
  if (vec) {
    launch_bwd_partial<4>(activation, grid, st, dy, lddy, z, ldz, n, C, t.tx_bits, chunk, save, gamma, beta, dz,
                          lddz, part);
  } else {
    launch_bwd_partial<1>(activation, grid, st, dy, lddy, z, ldz, n, C, t.tx_bits, chunk, save, gamma, beta, dz,
                          lddz, part);
  }
  if (int rc = check_launch("bn_bwd_partial_kernel")) return rc;
  hipLaunchKernelGGL(bn_bwd_final_kernel, dim3((int)ceil_div(C, kThreads / kFinLanes)), dim3(kThreads), 0, st, part,
                     chunks, n, C, d_gamma, d_beta, overwrite, means);
  if (int rc = check_launch("bn_bwd_final_kernel")) return rc;
  const dim3 grid2(elementwise_blocks(n, t), t.tiles);
  if (vec) {
    hipLaunchKernelGGL(bn_bwd_dz_kernel<4>, grid2, dim3(kThreads), 0, st, z, ldz, n, C, t.tx_bits, save, gamma, means,
                       dz, lddz);
  } else {
    hipLaunchKernelGGL(bn_bwd_dz_kernel<1>, grid2, dim3(kThreads), 0, st, z, ldz, n, C, t.tx_bits, save, gamma, means,
                       dz, lddz);
  }
  return check_launch("bn_bwd_dz_kernel");
}
