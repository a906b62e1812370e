// GaborNet (reference models.py:757-788 RealGaborLayer, :836-885 GaborNet): a stack of real Gabor (WIRE) layers,
//
//   a_l = cos(w0 (a_{l-1} Wf_l^T + bf_l)) (.) exp(-(c (a_{l-1} Ws_l^T + bs_l))^2)         (`freqs` and `scale`: two Linears
//   on the same input; omega = w0 * freqs(a), scale = scale(a) * c, cos(omega) * exp(-(scale ** 2))), the LAST layer
//   included: the head is a Gabor layer of width 1, so y lies in (-1, 1].
//
//   gabor_activation_kernel           out = gabor_f(u, s) elementwise over (n, H) (device_math.h): with two identity
//   gabor_activation_backward_kernel  Linears in front it is the generic layer path of every width; the backward gives
//                                     du = -g w0 sin(w0 u) e and ds = -2 c (c s) cos(w0 u) e g, e = exp(-(c s)^2).
//   gabor_forward_kernel              inference of the whole network: one persistent 512-thread workgroup per CU walks row
//                                     tiles on the tile loop of chain_tile.h with ONE f32 LDS image.  Layer 0 (K = dim_in,
//                                     both Linears) runs on the VALU as siren_chain.hip's first layer does.  Layers
//                                     1 .. L-2 are two H x H products each, acc_f += img Wf^T and acc_s += img Ws^T, from
//                                     the same image fragment (mma_step_pair) on the bf16 matrix pipe with three-term
//                                     operands (bf16x3.h); the weights are split once per call and streamed from L2 as a
//                                     PAIR of 16-deep chunks per step by LDS-DMA.  The epilogue is lane-local: the two
//                                     accumulators of a lane hold the same (row, column).  The head is two row . w dot
//                                     products per row.  Nothing (n, H)-sized touches memory, no atomics, a fixed
//                                     summation order.
#include <algorithm>
#include <cmath>

#include "bf16x3.h"
#include "common.h"
#include "device_math.h"
#include "entry_args.h"
#include "siren_chain.h"

namespace mri {
namespace {

using namespace chain;

constexpr int kFwdIn = 4;  // coordinates the fused inference kernel takes

// ------------------------------------------------------------------------------------------------ the activation
__global__ __launch_bounds__(256) void gabor_activation_kernel(const float* __restrict__ u, const float* __restrict__ s,
                                                               int64_t count, float w0, float c,
                                                               float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  out[i] = gabor_f(u[i], s[i], w0, c);
}

// with omega = w0 u, sigma = c s, e = exp(-sigma^2): du = -((g w0) sin(omega)) e, ds = -((((2 c) sigma) cos(omega)) e) g
__global__ __launch_bounds__(256) void gabor_activation_backward_kernel(const float* __restrict__ u,
                                                                        const float* __restrict__ s,
                                                                        const float* __restrict__ g, int64_t count,
                                                                        float w0, float c, float* __restrict__ du,
                                                                        float* __restrict__ ds) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  float sn, cs;
  sincos_fast(w0 * u[i], &sn, &cs);
  const float sigma = c * s[i], e = gauss_envelope(s[i], c), gi = g[i];
  du[i] = -(((gi * w0) * sn) * e);
  ds[i] = -(((((2.f * c) * sigma) * cs) * e) * gi);
}

// ------------------------------------------------------------------------------------------- fused inference
// Geometry of siren_chain.hip's Shape: a wave owns a 32 x 64 tile of the layer output in EACH of the two accumulator
// sets (four 32 x 32 accumulators), one image of 128 rows at H = 128 and 256 rows at H = 64.
template <int HH>
struct GShape : TileShape<HH, 64> {
  using T = TileShape<HH, 64>;
  static constexpr int rpt = T::rows / T::groups;  // rows per thread of layer 0: 32
  static constexpr int hpw = T::rows / 8;          // rows per wave of the head: 16 / 32
  static_assert(HH == 64 || HH == 128, "hidden width");
  static_assert(hpw <= 64, "a lane keeps one row of the head");
};

struct GaborArgs {
  const float* x;  // (n, dim_in)
  int64_t n;
  int dim_in, L;   // L layers: [0] (H, dim_in); [1 .. L-2] (H, H); [L-1] the head (1, H); each a freqs / scale pair
  float w0, c;
  const float* wf0;  // freqs / scale weights of layer 0
  const float* ws0;
  const float* bias_f[kMaxSine];
  const float* bias_s[kMaxSine];
  const float* wf_head;
  const float* ws_head;
  float* y;            // (n)
  const char* wsplit;  // split Wf_1 | Ws_1 | Wf_2 | Ws_2 | ... (split_matrix_bytes each)
};

template <class S>
struct GaborSmem {
  char wbuf[2][2][S::chunk_bytes] __attribute__((aligned(16)));  // [buffer][matrix: freqs, scale]
  float img[S::rows * S::ld];                                    // every layer's output
  float xs[S::rows * kFwdIn] __attribute__((aligned(16)));       // x (chain::stage_coords)
  float bias_f[kMaxSine][S::H];
  float bias_s[kMaxSine][S::H];
  float wh_f[S::H];
  float wh_s[S::H];
};

// a layer-0 pre-activation: the products of the axes added in axis order (absent axes: x = 0 and w = 0, an exact no-op)
__device__ __forceinline__ float first_dot(const float4& x, const float (&w)[kFwdIn], float bias) {
  float z = x.x * w[0];
  z += x.y * w[1];
  z += x.z * w[2];
  z += x.w * w[3];
  return z + bias;
}

template <class S>
__global__ __launch_bounds__(kThreads) void gabor_forward_kernel(const GaborArgs a) {
  __shared__ GaborSmem<S> sm;
  constexpr int H = S::H, NT = S::NT;
  const Lanes<S> ln;
  const int tid = ln.tid, n0 = ln.n0;
  const int L = a.L, n_mm = L - 2;  // matrix layers 1 .. n_mm of the chunk stream: Gabor layer l, a pair of matrices
  const int dim_in = a.dim_in;
  const float w0 = a.w0, c = a.c;

  for (int l = 0; l < L - 1; ++l) {
    load_vector<H>(sm.bias_f[l], a.bias_f[l], tid);
    load_vector<H>(sm.bias_s[l], a.bias_s[l], tid);
  }
  load_vector<H>(sm.wh_f, a.wf_head, tid);
  load_vector<H>(sm.wh_s, a.ws_head, tid);
  const float bf_last = a.bias_f[L - 1][0], bs_last = a.bias_s[L - 1][0];
  // layer 0: thread <-> (column, group of rows); the column's rows of Wf_0 and Ws_0 stay in registers
  const int col = tid % H, r0 = (tid / H) * S::rpt;
  float wf[kFwdIn], wsc[kFwdIn];
#pragma unroll
  for (int d = 0; d < kFwdIn; ++d) {
    wf[d] = d < dim_in ? a.wf0[col * dim_in + d] : 0.f;
    wsc[d] = d < dim_in ? a.ws0[col * dim_in + d] : 0.f;
  }
  const float bf0 = a.bias_f[0][col], bs0 = a.bias_s[0][col];

  const int64_t tiles = (a.n + S::rows - 1) / S::rows;
  const float* a_row = sm.img + ln.fragment_offset();
  int boff[NT];
  ln.weight_offsets(boff);
  const int64_t smb = split_matrix_bytes(H);

  ChunkStream<S, 1> stream(n_mm, tiles);
  auto issue = [&](int layer, int kc, int buf) {
    const char* pair = a.wsplit + (int64_t)(layer - 1) * 2 * smb;
    issue_chunk<S>(pair, kc, sm.wbuf[buf][0], ln.wave, ln.lane);
    issue_chunk<S>(pair + smb, kc, sm.wbuf[buf][1], ln.wave, ln.lane);
  };
  stream.prime(issue);

  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t m0 = tile * S::rows;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // previous tile is done with the image / xs
    stage_coords<kFwdIn>(sm.xs, a.x, m0, S::rows, a.n, dim_in, tid);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // ---- layer 0 on the VALU ---------------------------------------------------------------------------------------------
#pragma unroll 2
    for (int r = 0; r < S::rpt; r += 2) {
      const float4 xa = *reinterpret_cast<const float4*>(sm.xs + (r0 + r) * kFwdIn);
      const float4 xb = *reinterpret_cast<const float4*>(sm.xs + (r0 + r + 1) * kFwdIn);
      float o0, o1;
      gabor_f2(first_dot(xa, wf, bf0), first_dot(xb, wf, bf0), first_dot(xa, wsc, bs0), first_dot(xb, wsc, bs0), w0, c,
               &o0, &o1);
      sm.img[(r0 + r) * S::ld + col] = o0;
      sm.img[(r0 + r + 1) * S::ld + col] = o1;
    }
    // ---- the H x H layers: gabor(image Wf^T + bf, image Ws^T + bs) back into the image ------------------------------------
    for (int l = 1; l <= n_mm; ++l) {
      f32x16 acc_f[NT], acc_s[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc_f[t][r] = 0.f, acc_s[t][r] = 0.f;
      x3::Frag fa;
#pragma unroll
      for (int kc = 0; kc < S::chunks; ++kc, stream.consumed()) {
        stream.advance(tile, l, kc, issue);
        if (kc == 0) fa = first_fragment(a_row);  // (the stream's barrier completed the image)
        mma_step_pair<S>(acc_f, acc_s, fa, a_row, kc, sm.wbuf[stream.buffer()][0], sm.wbuf[stream.buffer()][1], boff);
      }
      float v[NT][16];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const float bf = sm.bias_f[l][n0 + 32 * t], bs = sm.bias_s[l][n0 + 32 * t];
#pragma unroll
        for (int r = 0; r < 16; r += 2)
          gabor_f2(acc_f[t][r] + bf, acc_f[t][r + 1] + bf, acc_s[t][r] + bs, acc_s[t][r + 1] + bs, w0, c, &v[t][r],
                   &v[t][r + 1]);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();  // every wave has read the image for the last time
#pragma unroll
      for (int t = 0; t < NT; ++t) store_acc<S>(sm.img, ln, v[t], t);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // the image is complete
    // ---- head: a Gabor layer of width 1.  A wave owns hpw consecutive rows: the two dot products of row i arrive in
    //      lane 0 and are parked in lane i, then the lanes evaluate their rows together and store them side by side ---------
    {
      const HeadDot<S> head_f(sm.wh_f, ln.lane), head_s(sm.wh_s, ln.lane);
      float my_f = 0.f, my_s = 0.f;
#pragma unroll 4
      for (int i = 0; i < S::hpw; ++i) {
        const float* img_row = sm.img + (ln.wave * S::hpw + i) * S::ld;
        const float df = head_f(img_row), ds = head_s(img_row);
        const float uf = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(df)));
        const float us = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(ds)));
        if (ln.lane == i) my_f = uf, my_s = us;
      }
      const int64_t row = m0 + ln.wave * S::hpw + ln.lane;
      if (ln.lane < S::hpw && row < a.n) a.y[row] = gabor_f(my_f + bf_last, my_s + bs_last, w0, c);
    }
  }
}

// ------------------------------------------------------------------------------------------------------ host side
// the fused chain's shape rule, each argument refused by name
int check_gabor_shape(const char* what, int dim_in, int hidden, int n_layers, int dim_out) {
  MRI_REQUIRE(hidden == 64 || hidden == 128, "%s: hidden = %d is not supported (64 / 128)", what, hidden);
  MRI_REQUIRE(dim_in >= 1 && dim_in <= kFwdIn, "%s: dim_in = %d is not supported (1 .. %d)", what, dim_in, kFwdIn);
  MRI_REQUIRE(n_layers >= 2 && n_layers <= kMaxSine, "%s: n_layers = %d is not supported (2 .. %d)", what, n_layers,
              kMaxSine);
  MRI_REQUIRE(dim_out == 1, "%s: dim_out = %d is not supported (1)", what, dim_out);
  return MRI_OK;
}
bool gabor_supported(int dim_in, int hidden, int n_layers, int dim_out) {
  return check_gabor_shape("fused Gabor forward", dim_in, hidden, n_layers, dim_out) == MRI_OK;
}
// the freqs / scale pair of every H x H layer
int64_t gabor_split_bytes(int hidden, int n_layers) { return (int64_t)2 * (n_layers - 2) * split_matrix_bytes(hidden); }

int check_activation(const char* what, const float* u, const float* s, int64_t n, int hidden, float w0, float c) {
  MRI_REQUIRE(hidden >= 1, "%s: hidden = %d is not supported (>= 1)", what, hidden);
  MRI_CHECK(check_rows(n));
  MRI_REQUIRE(n * hidden < (1ll << 38), "n * hidden = %lld out of range (one launch)", (long long)(n * hidden));
  MRI_CHECK(check_finite(what, "w0", w0));
  MRI_CHECK(check_finite(what, "c", c));
  if (n == 0) return MRI_OK;
  return check_buffers({{"u", u}, {"s", s}}, 4);
}

}  // namespace
}  // namespace mri

using namespace mri;

extern "C" int mri_gabor_activation(const float* u, const float* s, int64_t n, int32_t hidden, float w0, float c,
                                    float* out, void* stream) {
  MRI_CHECK(check_activation("Gabor activation", u, s, n, hidden, w0, c));
  if (n == 0) return MRI_OK;
  MRI_CHECK(check_buffer("out", out, 4));
  const int64_t count = n * hidden;
  hipLaunchKernelGGL(gabor_activation_kernel, dim3((unsigned)ceil_div(count, 256)), dim3(256), 0, (hipStream_t)stream, u,
                     s, count, w0, c, out);
  return check_launch("gabor_activation_kernel");
}

extern "C" int mri_gabor_activation_backward(const float* u, const float* s, const float* g, int64_t n, int32_t hidden,
                                             float w0, float c, float* du, float* ds, void* stream) {
  MRI_CHECK(check_activation("Gabor activation backward", u, s, n, hidden, w0, c));
  if (n == 0) return MRI_OK;
  MRI_CHECK(check_buffers({{"g", g}, {"du", du}, {"ds", ds}}, 4));
  const int64_t count = n * hidden;
  hipLaunchKernelGGL(gabor_activation_backward_kernel, dim3((unsigned)ceil_div(count, 256)), dim3(256), 0,
                     (hipStream_t)stream, u, s, g, count, w0, c, du, ds);
  return check_launch("gabor_activation_backward_kernel");
}

extern "C" int mri_gabor_forward_supported(int32_t dim_in, int32_t hidden, int32_t n_layers, int32_t dim_out) {
  return gabor_supported(dim_in, hidden, n_layers, dim_out) ? 1 : 0;
}

extern "C" int64_t mri_gabor_forward_workspace_bytes(int32_t hidden, int32_t n_layers) {
  if (!gabor_supported(1, hidden, n_layers, 1)) return -1;
  return gabor_split_bytes(hidden, n_layers);
}

extern "C" int mri_gabor_forward(const float* x, int64_t n, int32_t dim_in, int32_t hidden, int32_t n_layers,
                                 const float* const* freq_weight, const float* const* freq_bias,
                                 const float* const* scale_weight, const float* const* scale_bias, float w0, float c,
                                 float* y, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* const what = "fused Gabor forward";
  MRI_CHECK(check_gabor_shape(what, dim_in, hidden, n_layers, 1));
  MRI_CHECK(check_finite(what, "w0", w0));
  MRI_CHECK(check_finite(what, "c", c));
  MRI_CHECK(check_rows(n));
  if (n == 0) return MRI_OK;
  MRI_CHECK(check_buffers({{"x", x}, {"y", y}}, 4));
  MRI_CHECK(check_buffers({{"freq_weight", freq_weight}, {"freq_bias", freq_bias}, {"scale_weight", scale_weight},
                           {"scale_bias", scale_bias}}, kAnyAlignment));
  MRI_CHECK(check_workspace(what, "mri_gabor_forward_workspace_bytes", workspace, workspace_bytes,
                            gabor_split_bytes(hidden, n_layers)));
  MRI_CHECK(check_pointers({{"freq_weight", freq_weight}, {"freq_bias", freq_bias}, {"scale_weight", scale_weight},
                            {"scale_bias", scale_bias}}, 0, n_layers, 4));
  GaborArgs a{};
  a.x = x, a.n = n, a.dim_in = dim_in, a.L = n_layers, a.w0 = w0, a.c = c, a.y = y;
  for (int l = 0; l < n_layers; ++l) a.bias_f[l] = freq_bias[l], a.bias_s[l] = scale_bias[l];
  a.wf0 = freq_weight[0], a.ws0 = scale_weight[0];
  a.wf_head = freq_weight[n_layers - 1], a.ws_head = scale_weight[n_layers - 1];
  a.wsplit = static_cast<const char*>(workspace);
  hipStream_t st = (hipStream_t)stream;
  // layer l's pair lies side by side: Wf_l at (l - 1) 2 smb, Ws_l one matrix behind it
  const int64_t smb = split_matrix_bytes(hidden);
  char* const out = static_cast<char*>(workspace);
  if (int rc = split_weights_ld(freq_weight + 1, n_layers - 2, hidden, hidden, false, out, 2 * smb, st)) return rc;
  if (int rc = split_weights_ld(scale_weight + 1, n_layers - 2, hidden, hidden, false, out + smb, 2 * smb, st)) return rc;
  return dispatch_hidden_mod(hidden, [&](auto h) {
    using S = GShape<decltype(h)::value>;
    hipLaunchKernelGGL((gabor_forward_kernel<S>), dim3(persistent_blocks(n, S::rows)), dim3(kThreads), 0, st, a);
    return check_launch("gabor_forward_kernel");
  });
}
