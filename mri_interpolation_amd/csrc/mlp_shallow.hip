// Shallow decoder: k_in -> H -> 1 with an activation after each of the two Linears, one persistent kernel
// per call (include/mri_inr.h, mri_shallow_mlp_*).  The decoder of the notebook's HashMLP without BatchNorm:
// Linear(16, 64) -> GELU -> Linear(64, 1) -> GELU.
//
// A wave owns RT = 16 CT rows of the batch per round.  Every matrix product is the f32 MFMA 16x16x4
// (a k-ordered chain of f32 multiply-adds: the accuracy of the layer kernels); its operand maps, lane l,
// j = l & 15, g = l >> 4:   A[i = j][k = g]   B[k = g][col = j]   C/D[row = 4 g + reg][col = j].
//
//   z1^T (H x rows) = W1 (H x k_in) . x^T (k_in x rows)     A = W1 from LDS, B = x straight from HBM
//       (feature-major x: lane (g, j) reads x[4 s + g][row j], 16 consecutive floats per lane group;
//       rows >= k_in are zeros in registers).  The result has the batch row on the LANE and the hidden
//       unit h = 16 t + 4 g + reg in the registers.
//   z2 = a1 . w2 + b2: each lane multiplies its registers by its w2 values, two butterfly steps over g
//       (exact products summed in float64, rounded once).
//   dz1^T = dz2 w2 (.) act'(z1): elementwise on the accumulator registers.
//   d_x^T (k_in x rows) = W1^T (k_in x H) . dz1^T     sums over h, the REGISTER index of dz1^T: register
//       `reg` of tile t is the B operand of k-step (t, reg), whose four k values are h = 16 t + 4 g + reg,
//       so A is W1[16 t + 4 g + reg][j] -- no lane movement, no LDS.
//   dW1 (H x k_in) = dz1^T (H x rows) . x (rows x k_in)     sums over the batch row, the LANE index of
//       both operands: the one LDS transpose of the tile.  dz1^T and x^T are written to a wave-private
//       LDS image [h or k][row] and read back with the row on the k axis.
//   dw2, db1: per-lane sums over the rounds, reduced over the 16 row lanes once at the end; db2 and
//       the loss likewise.  The four waves add their parts in wave order in LDS, the workgroup writes ONE
//       slab of partial sums to the workspace, and slab_reduce_kernel<16, 5> (slab.h) adds the slabs in a fixed order:
//       no float atomics, bitwise reproducible.  The grid depends on n alone.
#include "common.h"
#include "device_math.h"
#include "slab.h"

#include <algorithm>

namespace mri {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxBlocks = 512;  // two workgroups per CU

struct ShallowArgs {
  const float *x, *target, *w1, *b1, *w2, *b2;
  float *y, *dx, *partial;
  int64_t n;
  int k_in, act_hidden, act_out;
  float grad_scale, inv_n;
};

template <int ACT>
__device__ __forceinline__ float act_value(float z) {
  if (ACT == MRI_ACT_RELU) return z > 0.f ? z : 0.f;
  if (ACT == MRI_ACT_GELU) return gelu_f(z);
  return z;
}
template <int ACT>
__device__ __forceinline__ float act_grad(float z) {
  if (ACT == MRI_ACT_RELU) return z > 0.f ? 1.f : 0.f;
  if (ACT == MRI_ACT_GELU) return gelu_grad_f(z);
  return 1.f;
}

// a1 = act(z1) in place; d = act'(z1) when training
template <int ACT, int T, int CT, bool TRAIN>
__device__ __forceinline__ void hidden_activation(f32x4 (&z)[T][CT], f32x4 (&d)[T][CT]) {
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float v = z[t][c][q];
        if (TRAIN) d[t][c][q] = act_grad<ACT>(v);
        z[t][c][q] = act_value<ACT>(v);
      }
}

__device__ __forceinline__ void out_activation(int act, float z2, float* y, float* g) {
  switch (act) {
    case MRI_ACT_RELU: *y = act_value<MRI_ACT_RELU>(z2), *g = act_grad<MRI_ACT_RELU>(z2); break;
    case MRI_ACT_GELU: *y = act_value<MRI_ACT_GELU>(z2), *g = act_grad<MRI_ACT_GELU>(z2); break;
    default: *y = z2, *g = 1.f;
  }
}

__device__ __forceinline__ float sum_over_rows(float v) {  // over the 16 lanes j of a lane group
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  return v;
}

// H hidden units, KP = k_in padded to a multiple of 16 (zeros), CT 16-row column tiles per wave and round.
template <int H, int KP, int CT, bool TRAIN>
__global__ __launch_bounds__(kThreads) void shallow_mlp_kernel(const ShallowArgs a) {
  constexpr int T = H / 16, KT = KP / 16, KS = KP / 4;
  constexpr int RT = 16 * CT, RTP = RT + 2;  // + 2: the transposed reads of a half-wave hit 32 banks
  constexpr int WP = KP + 2;
  constexpr int kWaveImage = (H + KP) * RTP;
  static_assert(H * 32 + 2 * H + 2 <= kWaves * kWaveImage, "the slab is assembled in the wave images");
  __shared__ float w1s[H * WP];
  __shared__ __attribute__((aligned(16))) float b1s[H];
  __shared__ __attribute__((aligned(16))) float w2s[H];
  __shared__ float image[TRAIN ? kWaves * kWaveImage : 1];

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
  const int k_in = a.k_in;
  for (int e = threadIdx.x; e < H * KP; e += kThreads) {
    const int h = e / KP, kk = e % KP;
    w1s[h * WP + kk] = kk < k_in ? a.w1[h * k_in + kk] : 0.f;
  }
  for (int e = threadIdx.x; e < H; e += kThreads) b1s[e] = a.b1[e], w2s[e] = a.w2[e];
  __syncthreads();
  const float b2 = a.b2[0];

  f32x4 dw1[T][KT], dw2[T], db1[T];
  float db2 = 0.f, loss = 0.f;
  if (TRAIN) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
      dw2[t] = db1[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) dw1[t][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }

  const int64_t block_rows = (int64_t)kWaves * RT;
  const int64_t n_tiles = (a.n + block_rows - 1) / block_rows;
  const int rounds = (int)((n_tiles + gridDim.x - 1) / gridDim.x);  // the same for every workgroup (barriers)
  for (int round = 0; round < rounds; ++round) {
    const int64_t row0 = ((int64_t)blockIdx.x + (int64_t)round * gridDim.x) * block_rows + wave * RT;

    // x^T as the B operand: lane (g, j) holds x[4 s + g][row0 + 16 c + j]
    float xr[KS][CT];
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        const int kk = 4 * s + g;
        const int64_t r = row0 + 16 * c + j;
        xr[s][c] = (kk < k_in && r < a.n) ? a.x[(int64_t)kk * a.n + r] : 0.f;
      }

    f32x4 z[T][CT], d[T][CT];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const f32x4 bias = *reinterpret_cast<const f32x4*>(&b1s[16 * t + 4 * g]);
#pragma unroll
      for (int c = 0; c < CT; ++c) z[t][c] = bias;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const float w = w1s[(16 * t + j) * WP + 4 * s + g];
#pragma unroll
        for (int c = 0; c < CT; ++c) z[t][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, xr[s][c], z[t][c], 0, 0, 0);
      }
    }
    switch (a.act_hidden) {
      case MRI_ACT_RELU: hidden_activation<MRI_ACT_RELU, T, CT, TRAIN>(z, d); break;
      case MRI_ACT_GELU: hidden_activation<MRI_ACT_GELU, T, CT, TRAIN>(z, d); break;
      default: hidden_activation<MRI_ACT_IDENTITY, T, CT, TRAIN>(z, d);
    }

    float dz2[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      // the one long sum of a row (H terms that cancel): exact products added in float64 and rounded once, so
      // that y carries the rounding of a1 only (16 f64 multiply-adds per lane beside ~10^3 VALU instructions
      // of activation work)
      double acc2 = 0.0;
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const f32x4 w2 = *reinterpret_cast<const f32x4*>(&w2s[16 * t + 4 * g]);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc2 += (double)z[t][c][q] * (double)w2[q];
      }
      acc2 += __shfl_xor(acc2, 16);
      acc2 += __shfl_xor(acc2, 32);
      const float z2 = (float)(acc2 + (double)b2);
      float yv, gv;
      out_activation(a.act_out, z2, &yv, &gv);
      const int64_t r = row0 + 16 * c + j;
      const bool valid = r < a.n;
      if (a.y && valid && g == 0) a.y[r] = yv;
      if (TRAIN) {
        const float diff = yv - (valid ? a.target[r] : 0.f);
        dz2[c] = valid ? (a.grad_scale * diff) * gv : 0.f;
        if (valid && g == 0) loss += diff * diff, db2 += dz2[c];
      }
    }
    if (!TRAIN) continue;

#pragma unroll
    for (int t = 0; t < T; ++t) {
      const f32x4 w2 = *reinterpret_cast<const f32x4*>(&w2s[16 * t + 4 * g]);
#pragma unroll
      for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          dw2[t][q] += dz2[c] * z[t][c][q];
          const float v = (dz2[c] * w2[q]) * d[t][c][q];
          d[t][c][q] = v;  // dz1^T
          db1[t][q] += v;
        }
    }

    if (a.dx) {
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        f32x4 acc[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float w = w1s[(16 * t + 4 * g + q) * WP + 16 * kt + j];
#pragma unroll
            for (int c = 0; c < CT; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, d[t][c][q], acc[c], 0, 0, 0);
          }
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int kk = 16 * kt + 4 * g + q;
            const int64_t r = row0 + 16 * c + j;
            if (kk < k_in && r < a.n) a.dx[(int64_t)kk * a.n + r] = acc[c][q];
          }
      }
    }

    // the transpose: [k][row] and [h][row] images of this wave's tile, read back with the row on the k axis
    float* xs = image + wave * kWaveImage;
    float* dzs = xs + KP * RTP;
    __syncthreads();  // the previous round's reads are done
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int c = 0; c < CT; ++c) xs[(4 * s + g) * RTP + 16 * c + j] = xr[s][c];
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int q = 0; q < 4; ++q) dzs[(16 * t + 4 * g + q) * RTP + 16 * c + j] = d[t][c][q];
    __syncthreads();
#pragma unroll
    for (int s = 0; s < RT / 4; ++s) {
      float xb[KT];
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) xb[kt] = xs[(16 * kt + j) * RTP + 4 * s + g];
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const float da = dzs[(16 * t + j) * RTP + 4 * s + g];
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) dw1[t][kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(da, xb[kt], dw1[t][kt], 0, 0, 0);
      }
    }
  }
  if (!TRAIN) return;

  // one slab per workgroup (ShallowSlab), the waves added in wave order
  const ShallowSlab lay{H, k_in};
  const int slab = lay.floats();
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) db1[t][q] = sum_over_rows(db1[t][q]), dw2[t][q] = sum_over_rows(dw2[t][q]);
  db2 = sum_over_rows(db2);
  loss = sum_over_rows(loss);
  float* red = image;
  for (int w = 0; w < kWaves; ++w) {
    __syncthreads();
    if (wave != w) continue;
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int h = 16 * t + 4 * g + q;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
          const int kk = 16 * kt + j;
          float* p_w1 = lay.w1(red);
          if (kk < k_in) p_w1[h * k_in + kk] = w ? p_w1[h * k_in + kk] + dw1[t][kt][q] : dw1[t][kt][q];
        }
        if (j == 0) {
          float* pb = lay.b1(red) + h;
          float* pw = lay.w2(red) + h;
          *pb = w ? *pb + db1[t][q] : db1[t][q];
          *pw = w ? *pw + dw2[t][q] : dw2[t][q];
        }
      }
    if (lane == 0) {
      float* pb = lay.b2(red);
      float* pl = lay.loss(red);
      *pb = w ? *pb + db2 : db2;
      *pl = w ? *pl + loss : loss;
    }
  }
  __syncthreads();
  float* out = a.partial + (int64_t)blockIdx.x * slab;
  for (int e = threadIdx.x; e < slab; e += kThreads) out[e] = e == lay.loss(0) ? red[e] * a.inv_n : red[e];
}

bool act_ok(int act) { return act == MRI_ACT_IDENTITY || act == MRI_ACT_RELU || act == MRI_ACT_GELU; }

bool supported(int k_in, int hidden, int dim_out, int act_hidden, int act_out) {
  return dim_out == 1 && k_in >= 1 && k_in <= 32 && (hidden == 32 || hidden == 64 || hidden == 128) &&
         act_ok(act_hidden) && act_ok(act_out);
}

// rows of a workgroup's tile per round: 16 CT per wave.  CT = 2 at 32 hidden units; at 64, CT = 1 keeps the
// training kernel under 256 registers (two waves per SIMD): 70 against 96 us at n = 2^18, k_in = 16
int block_rows(int hidden) { return kWaves * (hidden <= 32 ? 32 : 16); }

int pick_blocks(int hidden, int64_t n) {
  return (int)std::min<int64_t>(ceil_div(n, block_rows(hidden)), kMaxBlocks);
}

template <int H, int KP, int CT>
void launch_one(const ShallowArgs& a, bool train, int blocks, hipStream_t st) {
  if (train)
    hipLaunchKernelGGL((shallow_mlp_kernel<H, KP, CT, true>), dim3(blocks), dim3(kThreads), 0, st, a);
  else
    hipLaunchKernelGGL((shallow_mlp_kernel<H, KP, CT, false>), dim3(blocks), dim3(kThreads), 0, st, a);
}

int launch(const ShallowArgs& a, int hidden, bool train, hipStream_t st) {
  const int blocks = pick_blocks(hidden, a.n);
  const bool wide = a.k_in > 16;
  if (hidden == 32)
    wide ? launch_one<32, 32, 2>(a, train, blocks, st) : launch_one<32, 16, 2>(a, train, blocks, st);
  else if (hidden == 64)
    wide ? launch_one<64, 32, 1>(a, train, blocks, st) : launch_one<64, 16, 1>(a, train, blocks, st);
  else
    wide ? launch_one<128, 32, 1>(a, train, blocks, st) : launch_one<128, 16, 1>(a, train, blocks, st);
  return check_launch("shallow_mlp_kernel");
}

}  // namespace
}  // namespace mri

using namespace mri;

extern "C" int mri_shallow_mlp_supported(int32_t k_in, int32_t hidden, int32_t dim_out, int32_t act_hidden,
                                         int32_t act_out) {
  return supported(k_in, hidden, dim_out, act_hidden, act_out) ? 1 : 0;
}

extern "C" int64_t mri_shallow_mlp_workspace_bytes(int32_t k_in, int32_t hidden, int64_t n) {
  if (!supported(k_in, hidden, 1, MRI_ACT_IDENTITY, MRI_ACT_IDENTITY)) return -1;
  return (int64_t)pick_blocks(hidden, std::max<int64_t>(n, 1)) * ShallowSlab{hidden, k_in}.floats() * 4;
}

extern "C" int mri_shallow_mlp_forward(const float* x, int64_t n, int32_t k_in, int32_t hidden, const float* w1,
                                       const float* b1, const float* w2, const float* b2, int32_t act_hidden,
                                       int32_t act_out, float* y, void* stream) {
  MRI_REQUIRE(supported(k_in, hidden, 1, act_hidden, act_out),
              "shallow decoder %d -> %d -> 1 with activations %d, %d is not supported", k_in, hidden, act_hidden,
              act_out);
  MRI_REQUIRE(n >= 0, "negative n");
  if (n == 0) return MRI_OK;
  MRI_REQUIRE(x && w1 && b1 && w2 && b2 && y, "NULL device pointer");
  ShallowArgs a{};
  a.x = x, a.w1 = w1, a.b1 = b1, a.w2 = w2, a.b2 = b2, a.y = y;
  a.n = n, a.k_in = k_in, a.act_hidden = act_hidden, a.act_out = act_out;
  return launch(a, hidden, false, (hipStream_t)stream);
}

extern "C" int mri_shallow_mlp_train(const float* x, const float* target, int64_t n, int64_t n_total, int32_t k_in,
                                     int32_t hidden, const float* w1, const float* b1, const float* w2,
                                     const float* b2, int32_t act_hidden, int32_t act_out, float grad_divisor,
                                     float* d_w1, float* d_b1, float* d_w2, float* d_b2, float* d_x, float* loss_out,
                                     float* y, int32_t overwrite, void* workspace, int64_t workspace_bytes,
                                     void* stream) {
  MRI_REQUIRE(supported(k_in, hidden, 1, act_hidden, act_out),
              "shallow decoder %d -> %d -> 1 with activations %d, %d is not supported", k_in, hidden, act_hidden,
              act_out);
  MRI_REQUIRE(n >= 0 && grad_divisor > 0.f, "bad n / grad_divisor");
  MRI_REQUIRE(n_total >= n, "slice of %lld rows of a batch of %lld", (long long)n, (long long)n_total);
  if (n == 0) return MRI_OK;
  MRI_REQUIRE(x && target && w1 && b1 && w2 && b2, "NULL device pointer");
  MRI_REQUIRE(d_w1 && d_b1 && d_w2 && d_b2 && loss_out, "NULL gradient pointer");
  const ShallowSlab lay{hidden, k_in};
  const int slab = lay.floats();
  const int blocks = pick_blocks(hidden, n);
  MRI_REQUIRE(workspace && workspace_bytes >= (int64_t)blocks * slab * 4,
              "shallow decoder needs a workspace of %lld bytes (mri_shallow_mlp_workspace_bytes)",
              (long long)blocks * slab * 4);
  ShallowArgs a{};
  a.x = x, a.target = target, a.w1 = w1, a.b1 = b1, a.w2 = w2, a.b2 = b2;
  a.y = y, a.dx = d_x, a.partial = static_cast<float*>(workspace);
  a.n = n, a.k_in = k_in, a.act_hidden = act_hidden, a.act_out = act_out;
  a.grad_scale = (float)(2.0 / ((double)n_total * (double)grad_divisor));
  a.inv_n = (float)(1.0 / (double)n_total);
  if (int rc = launch(a, hidden, true, (hipStream_t)stream)) return rc;
  return reduce_slabs<16>(a.partial, blocks, slab, segments(lay, overwrite ? 1 : 0, d_w1, d_b1, d_w2, d_b2, loss_out),
                          (hipStream_t)stream);
}
