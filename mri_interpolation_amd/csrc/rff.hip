// RffNet (reference models.py:542-584): Gaussian Fourier features and a ReLU MLP on them.
//
//   vp = (fl32(2 pi) x) b^T        z = [cos(vp) | sin(vp)]        (rff.layers.GaussianEncoding: the coordinates are
//   scaled first, then multiplied; cosines first), then n_layers Linears 2F -> H -> ... -> H -> 1, ReLU behind EVERY
//   one, the last included (models.py:46-56).
//
//   rff_encode_kernel           z (n, 2F): one thread per (row, frequency), a wave writes 64 consecutive cosines and
//                               64 consecutive sines.
//   rff_encode_backward_kernel  dx[i, d] = fl32(2 pi) sum_f b[f, d] (cos(vp_f) dz[i, F + f] - sin(vp_f) dz[i, f]): one
//                               wave per row, lane <-> frequencies f = lane, lane + 64, ... in ascending order, then a
//                               butterfly over the lanes: a fixed order, no atomics.
//   rff_forward_kernel          inference with F == H: one persistent 512-thread workgroup per CU walks row tiles with
//                               the geometry of modsiren_forward_kernel (modsiren.hip).  The VALU encodes the tile into
//                               two f32 LDS images, cos and sin; z never exists in HBM.  The first Linear (H, 2F) is two
//                               H x H products, W[:, :F] on the cos image and W[:, F:] on the sin image, into ONE
//                               accumulator on the bf16 matrix pipe with three-term operands (bf16x3.h); every later
//                               H x H Linear is one product on the image the layer before left.  The weights are split
//                               once per call and streamed from L2 in 16-deep chunks by LDS-DMA (chain_tile.h).  The
//                               head is a row . w dot product per wave.
#include <algorithm>

#include "bf16x3.h"
#include "common.h"
#include "device_math.h"
#include "siren_chain.h"

namespace mri {
namespace {

using namespace chain;

constexpr float kTwoPi = 6.283185307179586f;  // fl32(2 pi): what `2 * np.pi * v` multiplies a float32 tensor by
// The dot product (fl32(2 pi) x) . b_f is a chain of fused multiply-adds in axis order from 0: what torch's CPU matmul
// computes for these short contractions, bit for bit, and one rounding per axis instead of two.
constexpr int kEncIn = 8;                     // coordinates the encoding kernels take
constexpr int kFwdIn = 4;                     // ... and the fused inference kernel

// ---------------------------------------------------------------------------------------------------- encoding
__global__ __launch_bounds__(256) void rff_encode_kernel(const float* __restrict__ x, int64_t n, int dim_in,
                                                         const float* __restrict__ b, int n_freq,
                                                         float* __restrict__ z) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n * n_freq) return;
  const int64_t row = i / n_freq;
  const int f = (int)(i - row * n_freq);
  float u = 0.f;
  for (int d = 0; d < dim_in; ++d) u = __builtin_fmaf(kTwoPi * x[row * dim_in + d], b[f * dim_in + d], u);
  float s, c;
  sincos_fast(u, &s, &c);  // (beyond |u| = 8192 the library's full-range sincosf)
  float* __restrict__ o = z + row * 2 * n_freq;
  o[f] = c;
  o[n_freq + f] = s;
}

__global__ __launch_bounds__(256) void rff_encode_backward_kernel(const float* __restrict__ x, int64_t n, int dim_in,
                                                                  const float* __restrict__ b, int n_freq,
                                                                  const float* __restrict__ dz,
                                                                  float* __restrict__ dx) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;  // (a whole wave)
  float xs[kEncIn], acc[kEncIn];
#pragma unroll
  for (int d = 0; d < kEncIn; ++d) xs[d] = d < dim_in ? kTwoPi * x[row * dim_in + d] : 0.f, acc[d] = 0.f;
  const float* __restrict__ g = dz + row * 2 * n_freq;
  for (int f = lane; f < n_freq; f += 64) {
    float bf[kEncIn], u = 0.f;
#pragma unroll
    for (int d = 0; d < kEncIn; ++d) {
      bf[d] = d < dim_in ? b[f * dim_in + d] : 0.f;
      if (d < dim_in) u = __builtin_fmaf(xs[d], bf[d], u);
    }
    float s, c;
    sincos_fast(u, &s, &c);
    const float t = c * g[n_freq + f] - s * g[f];
#pragma unroll
    for (int d = 0; d < kEncIn; ++d) acc[d] += bf[d] * t;
  }
#pragma unroll
  for (int d = 0; d < kEncIn; ++d) {
    float v = acc[d];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0 && d < dim_in) dx[row * dim_in + d] = kTwoPi * v;
  }
}

// ------------------------------------------------------------------------------------------- fused inference
// Geometry of modsiren.hip's MShape: a wave owns a 32 x 32 tile of the layer output, two images of 64 rows at H = 128,
// 128 rows at H = 64.
template <int HH>
struct RShape : TileShape<HH, 32> {
  using T = TileShape<HH, 32>;
  static constexpr int rpt = T::rows / T::groups;  // rows per thread of the encoding phase: 16
  static_assert(HH == 64 || HH == 128, "hidden width");
};

struct RffArgs {
  const float* x;  // (n, dim_in)
  int64_t n;
  int dim_in, L;               // L Linears: [0] (H, 2H); [1 .. L-2] (H, H); [L-1] the head (1, H)
  const float* b;              // (H, dim_in)
  const float* bias[kMaxSine];
  const float* w_head;
  float* y;                    // (n)
  const char* wsplit;          // split W_0[:, :H] | W_0[:, H:] | W_1 | ... | W_{L-2} (split_matrix_bytes each)
};

template <class S>
struct RffSmem {
  char wbuf[2][2][S::chunk_bytes] __attribute__((aligned(16)));  // [buffer][matrix: cos / only, sin]
  float img_c[S::rows * S::ld];  // cos(vp), then every layer's output
  float img_s[S::rows * S::ld];  // sin(vp)
  float xs[S::rows * kFwdIn];    // x (chain::stage_coords); the encoding phase scales it by fl32(2 pi)
  float bias[kMaxSine][S::H];
  float w_last[S::H];
};

__device__ __forceinline__ float relu_f(float v) { return v > 0.f ? v : 0.f; }

template <class S>
__global__ __launch_bounds__(kThreads) void rff_forward_kernel(const RffArgs a) {
  __shared__ RffSmem<S> sm;
  constexpr int H = S::H;
  const Lanes<S> ln;
  const int tid = ln.tid, n0 = ln.n0;
  const int L = a.L, n_mm = L - 1;  // matrix layers 1 .. n_mm of the chunk stream: Linear l - 1; layer 1 has two matrices
  const int dim_in = a.dim_in;

  for (int l = 0; l < n_mm; ++l) load_vector<H>(sm.bias[l], a.bias[l], tid);
  load_vector<H>(sm.w_last, a.w_head, tid);
  const float b_last = a.bias[L - 1][0];
  // the encoding phase: thread <-> (frequency, group of rows); the frequency's row of b stays in registers
  const int col = tid % H, r0 = (tid / H) * S::rpt;
  float br[kFwdIn];
#pragma unroll
  for (int d = 0; d < kFwdIn; ++d) br[d] = d < dim_in ? a.b[col * dim_in + d] : 0.f;

  const int64_t tiles = (a.n + S::rows - 1) / S::rows;
  const float* c_row = sm.img_c + ln.fragment_offset();
  const float* s_row = sm.img_s + ln.fragment_offset();
  int boff[1];
  ln.weight_offsets(boff);
  const int64_t smb = split_matrix_bytes(H);

  ChunkStream<S, 1> stream(n_mm, tiles);
  auto issue = [&](int layer, int kc, int buf) {
    if (layer == 1) {
      issue_chunk<S>(a.wsplit, kc, sm.wbuf[buf][0], ln.wave, ln.lane);
      issue_chunk<S>(a.wsplit + smb, kc, sm.wbuf[buf][1], ln.wave, ln.lane);
    } else {
      issue_chunk<S>(a.wsplit + (int64_t)layer * smb, kc, sm.wbuf[buf][0], ln.wave, ln.lane);
    }
  };
  stream.prime(issue);

  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t m0 = tile * S::rows;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // previous tile is done with the images / xs
    stage_coords<kFwdIn>(sm.xs, a.x, m0, S::rows, a.n, dim_in, tid);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // ---- the encoding on the VALU: both images -----------------------------------------------------------------------
#pragma unroll 1
    for (int r = 0; r < S::rpt; r += 2) {
      const float4 xa = *reinterpret_cast<const float4*>(sm.xs + (r0 + r) * kFwdIn);
      const float4 xb = *reinterpret_cast<const float4*>(sm.xs + (r0 + r + 1) * kFwdIn);
      float u0 = (kTwoPi * xa.x) * br[0], u1 = (kTwoPi * xb.x) * br[0];
      u0 = __builtin_fmaf(kTwoPi * xa.y, br[1], u0), u1 = __builtin_fmaf(kTwoPi * xb.y, br[1], u1);
      u0 = __builtin_fmaf(kTwoPi * xa.z, br[2], u0), u1 = __builtin_fmaf(kTwoPi * xb.z, br[2], u1);
      u0 = __builtin_fmaf(kTwoPi * xa.w, br[3], u0), u1 = __builtin_fmaf(kTwoPi * xb.w, br[3], u1);
      float s0, c0, s1, c1;
      sincos_fast2(u0, u1, &s0, &c0, &s1, &c1);
      sm.img_c[(r0 + r) * S::ld + col] = c0;
      sm.img_c[(r0 + r + 1) * S::ld + col] = c1;
      sm.img_s[(r0 + r) * S::ld + col] = s0;
      sm.img_s[(r0 + r + 1) * S::ld + col] = s1;
    }
    // ---- the H x H layers: relu(image W^T + bias) back into the cos image ------------------------------------------------
    auto layer = [&](int l, auto dual) {
      constexpr bool DUAL = decltype(dual)::value;  // the first Linear: cos and sin halves into one accumulator
      f32x16 acc[1];
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[0][r] = 0.f;
      x3::Frag fc, fs;
#pragma unroll
      for (int kc = 0; kc < S::chunks; ++kc, stream.consumed()) {
        stream.advance(tile, l, kc, issue);
        if (kc == 0) {
          fc = first_fragment(c_row);
          if (DUAL) fs = first_fragment(s_row);
        }
        mma_step<S>(acc, fc, c_row, kc, sm.wbuf[stream.buffer()][0], boff);
        if (DUAL) mma_step<S>(acc, fs, s_row, kc, sm.wbuf[stream.buffer()][1], boff);
      }
      const float bj = sm.bias[l - 1][n0];
      float v[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) v[r] = relu_f(acc[0][r] + bj);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();  // every wave has read the images for the last time
      store_acc<S>(sm.img_c, ln, v);
    };
    layer(1, std::true_type{});
    for (int l = 2; l <= n_mm; ++l) layer(l, std::false_type{});
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // the image is complete
    // ---- head: y[row] = relu(image[row] . w_head + b_head), one wave per row -------------------------------------------
    {
      const HeadDot<S> head(sm.w_last, ln.lane);
#pragma unroll 4
      for (int i = 0; i < S::rows / 8; ++i) {
        const int row = ln.wave * (S::rows / 8) + i;
        const float acc1 = head(sm.img_c + row * S::ld);
        if (ln.lane == 0 && m0 + row < a.n) a.y[m0 + row] = relu_f(acc1 + b_last);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------ host side
bool rff_supported(int dim_in, int hidden, int n_freq, int n_layers, int dim_out) {
  return (hidden == 64 || hidden == 128) && n_freq == hidden && dim_in >= 1 && dim_in <= kFwdIn && n_layers >= 2 &&
         n_layers <= kMaxSine && dim_out == 1;
}
template <class S>
int rff_blocks(int64_t n) { return (int)std::min<int64_t>(ceil_div(n, S::rows), 256); }  // one workgroup per CU
// the two halves of the first Linear and the n_layers - 2 square ones
int64_t rff_split_bytes(int hidden, int n_layers) { return (int64_t)n_layers * split_matrix_bytes(hidden); }

int check_encode(const float* x, int64_t n, int dim_in, const float* b, int n_freq) {
  MRI_REQUIRE(dim_in >= 1 && dim_in <= kEncIn, "RFF encoding: dim_in = %d is not supported (1 .. %d)", dim_in, kEncIn);
  MRI_REQUIRE(n_freq >= 1, "RFF encoding: n_freq = %d is not supported (>= 1)", n_freq);
  MRI_REQUIRE(n >= 0 && n < (1ll << 31), "n = %lld out of range", (long long)n);
  MRI_REQUIRE(n * n_freq < (1ll << 38), "n * n_freq = %lld out of range (one launch)", (long long)(n * n_freq));
  if (n == 0) return MRI_OK;
  MRI_REQUIRE(x, "x is NULL");
  MRI_REQUIRE(b, "b is NULL");
  MRI_REQUIRE(aligned_to(x, 4), "x must be 4-byte aligned");
  MRI_REQUIRE(aligned_to(b, 4), "b must be 4-byte aligned");
  return MRI_OK;
}

}  // namespace
}  // namespace mri

using namespace mri;

extern "C" int mri_rff_encode(const float* x, int64_t n, int32_t dim_in, const float* b, int32_t n_freq, float* z,
                              void* stream) {
  if (int rc = check_encode(x, n, dim_in, b, n_freq)) return rc;
  if (n == 0) return MRI_OK;
  MRI_REQUIRE(z, "z is NULL");
  MRI_REQUIRE(aligned_to(z, 4), "z must be 4-byte aligned");
  hipLaunchKernelGGL(rff_encode_kernel, dim3((unsigned)ceil_div(n * n_freq, 256)), dim3(256), 0, (hipStream_t)stream,
                     x, n, dim_in, b, n_freq, z);
  return check_launch("rff_encode_kernel");
}

extern "C" int mri_rff_encode_backward_input(const float* x, int64_t n, int32_t dim_in, const float* b,
                                             int32_t n_freq, const float* dz, float* dx, void* stream) {
  if (int rc = check_encode(x, n, dim_in, b, n_freq)) return rc;
  if (n == 0) return MRI_OK;
  MRI_REQUIRE(dz, "dz is NULL");
  MRI_REQUIRE(dx, "dx is NULL");
  MRI_REQUIRE(aligned_to(dz, 4), "dz must be 4-byte aligned");
  MRI_REQUIRE(aligned_to(dx, 4), "dx must be 4-byte aligned");
  hipLaunchKernelGGL(rff_encode_backward_kernel, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, (hipStream_t)stream, x,
                     n, dim_in, b, n_freq, dz, dx);
  return check_launch("rff_encode_backward_kernel");
}

extern "C" int mri_rff_forward_supported(int32_t dim_in, int32_t hidden, int32_t n_freq, int32_t n_layers,
                                         int32_t dim_out) {
  return rff_supported(dim_in, hidden, n_freq, n_layers, dim_out) ? 1 : 0;
}

extern "C" int64_t mri_rff_forward_workspace_bytes(int32_t hidden, int32_t n_layers) {
  if (!rff_supported(1, hidden, hidden, n_layers, 1)) return -1;
  return rff_split_bytes(hidden, n_layers);
}

extern "C" int mri_rff_forward(const float* x, int64_t n, int32_t dim_in, int32_t hidden, int32_t n_freq,
                               int32_t n_layers, const float* b, const float* const* weight,
                               const float* const* bias, float* y, void* workspace, int64_t workspace_bytes,
                               void* stream) {
  MRI_REQUIRE(hidden == 64 || hidden == 128, "fused RFF forward: hidden = %d is not supported (64 / 128)", hidden);
  MRI_REQUIRE(n_freq == hidden, "fused RFF forward: n_freq = %d is not supported (n_freq == hidden = %d)", n_freq,
              hidden);
  MRI_REQUIRE(dim_in >= 1 && dim_in <= kFwdIn, "fused RFF forward: dim_in = %d is not supported (1 .. %d)", dim_in,
              kFwdIn);
  MRI_REQUIRE(n_layers >= 2 && n_layers <= kMaxSine, "fused RFF forward: n_layers = %d is not supported (2 .. %d)",
              n_layers, kMaxSine);
  MRI_REQUIRE(rff_supported(dim_in, hidden, n_freq, n_layers, 1), "fused RFF forward: %d -> %d x %d -> 1 is not supported",
              dim_in, hidden, n_layers);
  MRI_REQUIRE(n >= 0 && n < (1ll << 31), "n = %lld out of range", (long long)n);
  if (n == 0) return MRI_OK;
  MRI_REQUIRE(x, "x is NULL");
  MRI_REQUIRE(b, "b is NULL");
  MRI_REQUIRE(y, "y is NULL");
  MRI_REQUIRE(weight, "weight is NULL");
  MRI_REQUIRE(bias, "bias is NULL");
  MRI_REQUIRE(aligned_to(x, 4), "x must be 4-byte aligned");
  MRI_REQUIRE(aligned_to(b, 4), "b must be 4-byte aligned");
  MRI_REQUIRE(aligned_to(y, 4), "y must be 4-byte aligned");
  const int64_t need = rff_split_bytes(hidden, n_layers);
  MRI_REQUIRE(workspace && workspace_bytes >= need && aligned_to(workspace, 16),
              "workspace: the fused RFF forward needs %lld bytes, 16-byte aligned (mri_rff_forward_workspace_bytes)",
              (long long)need);
  RffArgs a{};
  a.x = x, a.n = n, a.dim_in = dim_in, a.L = n_layers, a.b = b, a.y = y;
  for (int l = 0; l < n_layers; ++l) {
    MRI_REQUIRE(weight[l], "weight[%d] is NULL", l);
    MRI_REQUIRE(bias[l], "bias[%d] is NULL", l);
    MRI_REQUIRE(aligned_to(weight[l], 4) && aligned_to(bias[l], 4), "weight[%d] / bias[%d] must be 4-byte aligned", l, l);
    a.bias[l] = bias[l];
  }
  a.w_head = weight[n_layers - 1];
  a.wsplit = static_cast<const char*>(workspace);
  hipStream_t st = (hipStream_t)stream;
  char* const out = static_cast<char*>(workspace);
  const int64_t smb = split_matrix_bytes(hidden);
  // Linear 0 is (H, 2F): its cos half starts at column 0, its sin half at column F, both with row stride 2F
  const float* const halves[2] = {weight[0], weight[0] + n_freq};
  if (int rc = split_weights_ld(halves, 2, hidden, 2 * n_freq, false, out, smb, st)) return rc;
  if (int rc = split_weights_ld(weight + 1, n_layers - 2, hidden, hidden, false, out + 2 * smb, smb, st)) return rc;
  return dispatch_hidden_mod(hidden, [&](auto h) {
    using S = RShape<decltype(h)::value>;
    hipLaunchKernelGGL((rff_forward_kernel<S>), dim3(rff_blocks<S>(n)), dim3(kThreads), 0, st, a);
    return check_launch("rff_forward_kernel");
  });
}
