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
//                               head is a row . w dot product per wave.  Its training form (LOSS) also writes every
//                               hidden a_l once, dLoss/dp per row and the workgroup's share of the loss.
//   rff_gradient_kernel         y AND dy/dx, forward mode: the inference walk with four (dim_in <= 3) or eight (dim_in = 4)
//                               rows per point in both images, the value row and the tangent rows of the axes; a tangent
//                               passes a ReLU where its value row's pre-activation is positive.
//   rff_backward_kernel         the same walk from the head down with ONE image, dz_l = da_l (.) [a_l > 0]; dz_l leaves
//                               once per Linear, da_{l-1} = dz_l W_l against the transposed splits; bias and head
//                               gradients go to the workgroup's slab (slab.h, RffBwdSlab).
//   rff_wgrad0_kernel           dW_0 = [dz_0^T cos(vp) | dz_0^T sin(vp)] on the plan of siren_wgrad_kernel: dz_0 streams
//                               through LDS, the chunk's cos / sin rows are recomputed from x and b as the forward
//                               computes them; z does not exist in HBM in training either.
// No float atomics: every cross-workgroup sum goes through per-workgroup slabs added in a fixed order.
#include <algorithm>

#include "bf16x3.h"
#include "common.h"
#include "device_math.h"
#include "entry_args.h"
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
  // the training form (LOSS)
  float* act[kMaxSine];        // a_l (n, H), l = 0 .. L-2
  const float* target;         // (n)
  float grad_scale, inv_n;     // 2 / (n_total divisor), 1 / n_total
  float* dy_out;               // (n): dLoss / dp, the head's ReLU applied
  float* partial;              // [gridDim.x]: loss partial sums
};

template <class S>
struct RffSmem {
  char wbuf[2][2][S::chunk_bytes] __attribute__((aligned(16)));  // [buffer][matrix: cos / only, sin]
  float img_c[S::rows * S::ld];  // cos(vp), then every layer's output
  float img_s[S::rows * S::ld];  // sin(vp)
  float xs[S::rows * kFwdIn];    // x (chain::stage_coords); the encoding phase scales it by fl32(2 pi)
  float bias[kMaxSine][S::H];
  float w_last[S::H];
  float tgt[S::rows];            // LOSS: the tile's targets
  float red[8];                  //       the waves' loss sums
};

__device__ __forceinline__ float relu_f(float v) { return v > 0.f ? v : 0.f; }

// vp of one row and one frequency: the FMA chain in axis order (absent axes: x = 0 and b = 0, an exact no-op).  The
// forward's encoding phase and the first Linear's weight gradient both call this, so the recomputed z is the forward's.
__device__ __forceinline__ float rff_phase(const float4& x, const float (&br)[kFwdIn]) {
  float u = (kTwoPi * x.x) * br[0];
  u = __builtin_fmaf(kTwoPi * x.y, br[1], u);
  u = __builtin_fmaf(kTwoPi * x.z, br[2], u);
  u = __builtin_fmaf(kTwoPi * x.w, br[3], u);
  return u;
}

// LOSS: the training form: a_l leaves after every hidden epilogue, the head also writes dLoss/dp per row and adds up
// this workgroup's share of mean((y - target)^2).  y is the inference form's, bit for bit.
template <bool LOSS, class S>
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
  const int lane_off = ln.global_offset();
  const int64_t smb = split_matrix_bytes(H);
  float g_loss = 0.f;

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
    const bool full_tile = m0 + S::rows <= a.n;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // previous tile is done with the images / xs / tgt
    stage_coords<kFwdIn>(sm.xs, a.x, m0, S::rows, a.n, dim_in, tid);
    if (LOSS && tid < S::rows) sm.tgt[tid] = m0 + tid < a.n ? a.target[m0 + tid] : 0.f;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // ---- the encoding on the VALU: both images -----------------------------------------------------------------------
#pragma unroll 1
    for (int r = 0; r < S::rpt; r += 2) {
      const float4 xa = *reinterpret_cast<const float4*>(sm.xs + (r0 + r) * kFwdIn);
      const float4 xb = *reinterpret_cast<const float4*>(sm.xs + (r0 + r + 1) * kFwdIn);
      const float u0 = rff_phase(xa, br), u1 = rff_phase(xb, br);
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
      if constexpr (LOSS) {  // a_{l-1} leaves straight from the registers it is computed in
        float* __restrict__ ga = a.act[l - 1] + m0 * H;
        int off = lane_off;
        asm volatile("" : "+v"(off));
        const int64_t rows_left = ln.rows_left(a.n - m0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int dr = acc_row(r, 0);
          if (full_tile || dr < rows_left) ga[off + dr * H] = v[r];
        }
      }
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
        if (ln.lane == 0 && m0 + row < a.n) {
          const float yv = relu_f(acc1 + b_last);
          a.y[m0 + row] = yv;
          if constexpr (LOSS) {  // models.py:64 F.mse_loss: mean((y - target)^2); dLoss/dp = [y > 0] 2 (y - t) / N
            const float diff = yv - sm.tgt[row];
            g_loss += diff * diff;
            a.dy_out[m0 + row] = yv > 0.f ? diff * a.grad_scale : 0.f;
          }
        }
      }
    }
  }
  if constexpr (LOSS) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
    if (ln.lane == 0) sm.red[ln.wave] = g_loss;
    __syncthreads();
    if (tid == 0) {
      float sl = 0.f;
      for (int w = 0; w < 8; ++w) sl += sm.red[w];
      a.partial[blockIdx.x] = sl * a.inv_n;
    }
  }
}

// ------------------------------------------------------------------------- values and coordinate gradient, forward mode
// y and dy/dx from ONE walk of rff_forward_kernel's inference tile loop.  With u_f = (fl32(2 pi) x) . b_f, z = [cos u |
// sin u], p_0 = z W_0^T + beta_0, a_l = relu(p_l), p_l = a_{l-1} W_l^T + beta_l, y = relu(p_{L-1}), the tangent
// T_l^d = d a_l / d x_d:
//   Tz^d  = [-fl32(2 pi) b[:, d] (.) sin u | fl32(2 pi) b[:, d] (.) cos u]
//   T_0^d = [p_0 > 0] (.) (Tz^d W_0^T)       T_l^d = [p_l > 0] (.) (T_{l-1}^d W_l^T)       (no bias on tangent rows)
//   dy / dx_d = [p_{L-1} > 0] (T_{L-2}^d . w_head)                                         (ReLU'(0) = 0, as torch)
// The tangent rows go through the value row's products as more rows of BOTH images.  dim_in <= 3: a point owns four
// consecutive rows at a 4-aligned position, [value, d/dx_0, d/dx_1, d/dx_2] (the cos image: the cos halves, the sin
// image: the sin halves).  dim_in = 4: eight rows in siren_gradient.hip's order [value, d/dx_0, d/dx_1, d/dx_2 | value,
// d/dx_3, 0, 0], the value row written twice, so that register 4 q of EITHER lane half is a value row and 4 q + 1 ..
// 4 q + 3 are its tangents (acc_row): the epilogue is lane-local and a tangent register needs only the sign of its
// value register's pre-activation.  The value rows are rff_forward_kernel's, expression by expression: y is its y
// bit for bit.  Nothing (n, H)-sized is written: the call reads n dim_in floats and writes n (1 + dim_in).  No atomics,
// a fixed summation order.
template <int HH, int SL>
struct RGradShape : TileShape<HH, 32, SL> {
  using T = TileShape<HH, 32, SL>;
  static constexpr int ppt = T::points / T::groups;  // points per thread of the encoding phase: 4 (8 slots: 2)
  static_assert(HH == 64 || HH == 128, "hidden width");
  static_assert(SL == 4 || SL == 8, "image rows per point");
  static_assert(ppt % 2 == 0 && ppt * T::groups == T::points, "encoding-phase mapping");
  static_assert((T::rows / 8) % SL == 0, "a point's rows belong to one wave of the head");
};

struct RffGradArgs {
  const float* x;  // (n, dim_in)
  int64_t n;
  int dim_in, L;   // as RffArgs
  const float* b;  // (H, dim_in)
  const float* bias[kMaxSine];
  const float* w_head;
  float* y;            // (n)
  float* dydx;         // (n, dim_in)
  const char* wsplit;  // as RffArgs
};

template <class S>
struct RffGradSmem {
  char wbuf[2][2][S::chunk_bytes] __attribute__((aligned(16)));  // [buffer][matrix: cos / only, sin]
  float img_c[S::rows * S::ld];  // point p in rows slots p .. : cos u and the cos halves of Tz^d, then every layer's output
  float img_s[S::rows * S::ld];  //                              sin u and the sin halves of Tz^d
  float xs[S::points * S::slots] __attribute__((aligned(16)));  // coordinates of the tile's points, padded to slots
  float bias[kMaxSine][S::H];
  float w_last[S::H];
};

template <class S>
__global__ __launch_bounds__(kThreads) void rff_gradient_kernel(const RffGradArgs a) {
  __shared__ RffGradSmem<S> sm;
  constexpr int H = S::H, kSlots = S::slots;
  const Lanes<S> ln;
  const int tid = ln.tid, n0 = ln.n0;
  const int L = a.L, n_mm = L - 1;  // as rff_forward_kernel
  const int dim_in = a.dim_in;

  for (int l = 0; l < n_mm; ++l) load_vector<H>(sm.bias[l], a.bias[l], tid);
  load_vector<H>(sm.w_last, a.w_head, tid);
  const float b_last = a.bias[L - 1][0];
  // the encoding phase: thread <-> (frequency, group of points); the frequency's row of b stays in registers, and
  // fl32(2 pi) b[:, d], the factor of axis d's tangent rows (0 for an absent axis: its rows come out as zeros)
  const int col = tid % H, q0 = (tid / H) * S::ppt;
  float br[kFwdIn], tb[kFwdIn];
#pragma unroll
  for (int d = 0; d < kFwdIn; ++d) {
    br[d] = d < dim_in ? a.b[col * dim_in + d] : 0.f;
    tb[d] = kTwoPi * br[d];
  }

  const int64_t tiles = (a.n + S::points - 1) / S::points;
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
    const int64_t p0 = tile * S::points;  // first point of the tile
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // previous tile is done with the images / xs
    stage_coords<kSlots>(sm.xs, a.x, p0, S::points, a.n, dim_in, tid);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // ---- the encoding on the VALU: all rows of a point in both images ------------------------------------------------
#pragma unroll 1
    for (int i = 0; i < S::ppt; i += 2) {
      const float4 xa = *reinterpret_cast<const float4*>(sm.xs + (q0 + i) * kSlots);
      const float4 xb = *reinterpret_cast<const float4*>(sm.xs + (q0 + i + 1) * kSlots);
      const float u0 = rff_phase(xa, br), u1 = rff_phase(xb, br);
      float s0, c0, s1, c1;
      sincos_fast2(u0, u1, &s0, &c0, &s1, &c1);
      const bool live0 = p0 + q0 + i < a.n, live1 = p0 + q0 + i + 1 < a.n;
      float* rc0 = sm.img_c + (q0 + i) * kSlots * S::ld + col;
      float* rc1 = rc0 + kSlots * S::ld;
      float* rs0 = sm.img_s + (q0 + i) * kSlots * S::ld + col;
      float* rs1 = rs0 + kSlots * S::ld;
      rc0[0] = live0 ? c0 : 0.f, rc1[0] = live1 ? c1 : 0.f;
      rs0[0] = live0 ? s0 : 0.f, rs1[0] = live1 ? s1 : 0.f;
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        rc0[(1 + d) * S::ld] = live0 ? -(tb[d] * s0) : 0.f;
        rc1[(1 + d) * S::ld] = live1 ? -(tb[d] * s1) : 0.f;
        rs0[(1 + d) * S::ld] = live0 ? tb[d] * c0 : 0.f;
        rs1[(1 + d) * S::ld] = live1 ? tb[d] * c1 : 0.f;
      }
      if constexpr (kSlots == 8) {  // upper lane half of the accumulator: the value row again, d/dx_3, two zero rows
        rc0[4 * S::ld] = live0 ? c0 : 0.f, rc1[4 * S::ld] = live1 ? c1 : 0.f;
        rs0[4 * S::ld] = live0 ? s0 : 0.f, rs1[4 * S::ld] = live1 ? s1 : 0.f;
        rc0[5 * S::ld] = live0 ? -(tb[3] * s0) : 0.f, rc1[5 * S::ld] = live1 ? -(tb[3] * s1) : 0.f;
        rs0[5 * S::ld] = live0 ? tb[3] * c0 : 0.f, rs1[5 * S::ld] = live1 ? tb[3] * c1 : 0.f;
        rc0[6 * S::ld] = rc0[7 * S::ld] = 0.f, rc1[6 * S::ld] = rc1[7 * S::ld] = 0.f;
        rs0[6 * S::ld] = rs0[7 * S::ld] = 0.f, rs1[6 * S::ld] = rs1[7 * S::ld] = 0.f;
      }
    }
    // ---- the H x H layers, back into the cos image ---------------------------------------------------------------------
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
      // epilogue: registers 4 q .. 4 q + 3 are one point's value and tangent rows (8 slots: of either half of the
      // point, the value row being there twice); the tangents pass where the value's pre-activation is positive
      const float bj = sm.bias[l - 1][n0];
      float v[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float p = acc[0][4 * q] + bj;
        v[4 * q] = relu_f(p);
#pragma unroll
        for (int j = 1; j < 4; ++j) v[4 * q + j] = p > 0.f ? acc[0][4 * q + j] : 0.f;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();  // every wave has read the images for the last time
      store_acc<S>(sm.img_c, ln, v);
    };
    layer(1, std::true_type{});
    for (int l = 2; l <= n_mm; ++l) layer(l, std::false_type{});
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // the image is complete
    // ---- head: image row . w_head, one wave per row and a point's rows in ONE wave, the value row first: slot 0 ->
    //      y = relu(. + b_head), slot 1 + d -> dydx[:, d] where the value's pre-activation is positive; of the upper four
    //      of 8 slots only slot 5 -> dydx[:, 3] is stored ----------------------------------------------------------------
    {
      const HeadDot<S> head(sm.w_last, ln.lane);
      bool pos = false;  // (lane 0's: of the point whose rows the wave is walking)
#pragma unroll 4
      for (int i = 0; i < S::rows / 8; ++i) {
        const int row = ln.wave * (S::rows / 8) + i;  // wave-uniform
        const int slot = row % kSlots;
        const int64_t p = p0 + row / kSlots;
        const int axis = slot < 4 ? slot - 1 : (slot == 5 ? 3 : kFwdIn);  // wave-uniform; -1: the value
        if (axis >= dim_in || p >= a.n) continue;
        const float acc1 = head(sm.img_c + row * S::ld);
        if (ln.lane == 0) {
          if (slot == 0) {
            const float pre = acc1 + b_last;
            pos = pre > 0.f;
            a.y[p] = relu_f(pre);
          } else {
            a.dydx[p * dim_in + axis] = pos ? acc1 : 0.f;
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ backward chain
// Per tile, from the head down, with da_l in accumulator registers:
//   dz_l = da_l (.) [a_l > 0]            (the mask from the saved a_l; ReLU'(0) = 0, as torch)
// becomes the LDS image (the A operand of the next product) and leaves for HBM once, for EVERY l: dz_0 feeds
// rff_wgrad0_kernel.  db_l, the image's column sums: a lane adds its 16 rows of its column as it writes them, the
// lane halves meet in a shuffle, the row blocks in LDS, and column c's ONE owner thread adds the tile's sum to the
// workgroup's slab (plain read-add-write in program order; the first tile overwrites).  Then da_{l-1} = dz_l W_l on
// the MFMAs against the transposed splits.  On the toolkit's helpers (chain_tile.h) throughout.
struct RffBwdArgs {
  const float* dy;  // (n): dLoss / dp
  int64_t n;
  int L;
  const float* w_head;          // (1, H)
  const float* act[kMaxSine];   // a_l, l = 0 .. L-2
  float* dz[kMaxSine];          // (n, H), l = 0 .. L-2
  float* partial;               // [gridDim.x][RffBwdSlab]
  const char* wtsplit;          // split W_l^T, l = 1 .. L-2 (split_matrix_bytes each)
};

template <class S>
struct RffBwdSmem {
  char wbuf[2][S::chunk_bytes] __attribute__((aligned(16)));
  float img[S::rows * S::ld];
  float red[S::RB][S::H];  // column sums of the row blocks
  float w_last[S::H];
  float dy[S::rows];
};

template <class S>
__global__ __launch_bounds__(kThreads) void rff_backward_kernel(const RffBwdArgs a) {
  __shared__ RffBwdSmem<S> sm;
  constexpr int H = S::H;
  const Lanes<S> ln;
  const int tid = ln.tid, n0 = ln.n0;
  const int L = a.L, n_mm = L - 2;  // the chunk stream's layer l is Linear l: W_l^T, l = n_mm .. 1
  load_vector<H>(sm.w_last, a.w_head, tid);

  const int64_t tiles = (a.n + S::rows - 1) / S::rows;
  const float* z_row = sm.img + ln.fragment_offset();
  int boff[1];
  ln.weight_offsets(boff);
  const int lane_off = ln.global_offset();
  const int64_t smb = split_matrix_bytes(H);

  const RffBwdSlab lay{H, L};
  float* const slab = a.partial + (int64_t)blockIdx.x * lay.floats();

  ChunkStream<S, -1> stream(n_mm, tiles);
  auto issue = [&](int layer, int kc, int buf) {
    issue_chunk<S>(a.wtsplit + (int64_t)(layer - 1) * smb, kc, sm.wbuf[buf], ln.wave, ln.lane);
  };
  stream.prime(issue);

  // a saved (n, H) tensor in the accumulator layout (zeros beyond n)
  auto load_acc = [&](const float* __restrict__ src, int64_t m0, bool tile_full, float (&v)[16]) {
    const float* __restrict__ g = src + m0 * H;
    int off = lane_off;
    asm volatile("" : "+v"(off));
    const int64_t rows_left = ln.rows_left(a.n - m0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int dr = acc_row(r, 0);
      v[r] = (tile_full || dr < rows_left) ? g[off + dr * H] : 0.f;
    }
  };

  // dW_head: (lane's column, its rows).  db_head (tid < rows) = sum of dLoss/dp, signed terms that cancel almost
  // entirely once the head bias has converged: summed in float64, one addition per thread and tile
  // (modsiren_backward_kernel)
  float g_wh = 0.f;
  double g_bh = 0.0;

  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t m0 = tile * S::rows;
    const bool full_tile = m0 + S::rows <= a.n;
    const bool first_tile = tile == (int64_t)blockIdx.x;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // previous tile is done with the image / red / dy
    if (tid < S::rows) {
      const float v = m0 + tid < a.n ? a.dy[m0 + tid] : 0.f;
      sm.dy[tid] = v;
      g_bh += (double)v;
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // ---- head: da_{L-2} = dy w_head; dW_head += dy^T a_{L-2} ---------------------------------------------------------
    float da[16], av[16];
    load_acc(a.act[L - 2], m0, full_tile, av);
    {
      const float wl = sm.w_last[n0];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float dyv = sm.dy[ln.row(r)];
        g_wh += dyv * av[r];
        da[r] = dyv * wl;
      }
    }
    for (int l = L - 2; l >= 0; --l) {
      if (l < L - 2) load_acc(a.act[l], m0, full_tile, av);
      float zs[16], col_sum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        zs[r] = av[r] > 0.f ? da[r] : 0.f;
        col_sum += zs[r];
      }
      col_sum += __shfl_xor(col_sum, 32, 64);  // the lane halves hold different rows of one column
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();  // every wave has read the image and red for the last time
      store_acc<S>(sm.img, ln, zs);
      if (ln.lh == 0) sm.red[ln.rb][n0] = col_sum;
      {  // the weight gradients read it
        float* __restrict__ gz = a.dz[l] + m0 * H;
        int off = lane_off;
        asm volatile("" : "+v"(off));
        const int64_t rows_left = ln.rows_left(a.n - m0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int dr = acc_row(r, 0);
          if (full_tile || dr < rows_left) gz[off + dr * H] = zs[r];
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();  // image and red complete
      if (tid < H) {  // db_l: column tid's owner
        float sum = 0.f;
#pragma unroll
        for (int q = 0; q < S::RB; ++q) sum += sm.red[q][tid];
        float* p = lay.b(slab, l) + tid;
        *p = first_tile ? sum : *p + sum;
      }
      if (l == 0) break;
      // ---- da_{l-1} = dz_l W_l ---------------------------------------------------------------------------------------
      f32x16 acc[1];
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[0][r] = 0.f;
      x3::Frag fz;
#pragma unroll
      for (int kc = 0; kc < S::chunks; ++kc, stream.consumed()) {
        stream.advance(tile, l, kc, issue);
        if (kc == 0) fz = first_fragment(z_row);
        mma_step<S>(acc, fz, z_row, kc, sm.wbuf[stream.buffer()], boff);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) da[r] = acc[0][r];
    }
  }

  // ---- head gradients of this workgroup ------------------------------------------------------------------------------
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();
  g_wh += __shfl_xor(g_wh, 32, 64);
  if (ln.lh == 0) sm.red[ln.rb][n0] = g_wh;
  __syncthreads();
  if (tid < H) {
    float sum = 0.f;
#pragma unroll
    for (int q = 0; q < S::RB; ++q) sum += sm.red[q][tid];
    lay.w_head(slab)[tid] = sum;
  }
  double* red64 = reinterpret_cast<double*>(sm.img);  // scratch: [rows]
  if (tid < S::rows) red64[tid] = g_bh;
  __syncthreads();
  if (tid == 0) {
    double sb = 0.0;
    for (int c = 0; c < S::rows; ++c) sb += red64[c];
    float* p_bh = lay.b_head(slab);
    p_bh[0] = (float)sb, p_bh[1] = 0.f, p_bh[2] = 0.f, p_bh[3] = 0.f;
  }
}

// ------------------------------------------------------------------------------- the first Linear's weight gradient
// dW_0 (H, 2F) = [dz_0^T c | dz_0^T s], on the plan of siren_wgrad_kernel (siren_chain.hip): a persistent workgroup holds
// the H x H result tiles of BOTH halves in MFMA accumulators and streams its share of the batch in 32-row chunks.  dz_0
// arrives by LDS-DMA; the chunk's cos and sin rows are NOT loaded: the VALU computes them into LDS from x and b with
// the forward's own FMA chain and sincos (rff_phase, sincos_fast2), so they are the forward's z bit for bit and no
// (n, 2F) tensor exists in training either.  The encoding of chunk c + 1 is written while the matrix pipe works on
// chunk c (all three LDS arrays are double buffered): one barrier per chunk.  Rows beyond n: their dz_0 rows are
// zeroed, as there, so the finite cos / sin computed for them (from the batch's last row) contribute 0.
constexpr int kWr0 = 32;  // batch rows per chunk: siren_wgrad_kernel's, so that wgrad_blocks / wgrad_slab_floats size this grid too

template <int HH>
struct RffWgradShape {
  static constexpr int H = HH, TD = H / 32, tiles = TD * TD;
  static constexpr bool wide = tiles >= 8;             // every wave owns TI x TJ tiles (of each half)
  static constexpr int TI = wide ? TD / 4 : 1, TJ = wide ? TD / 2 : 1;
  static constexpr int RS = wide ? 1 : 8 / tiles;      // waves per tile, splitting the row pairs
  static constexpr int pieces = H / 8;                 // 1-KiB DMA pieces of a 32 x H chunk
  static constexpr int rpt = kWr0 * H / kThreads;      // rows per thread of the encoding: 8 at H = 128, 4 at H = 64
  static_assert(HH == 64 || HH == 128, "hidden width");
  static_assert((kWr0 / 2 / RS) % 8 == 0, "a 16-deep step contracts eight of a wave's row pairs");
};

struct RffWgradArgs {
  const float* x;   // (n, dim_in)
  const float* b;   // (H, dim_in)
  const float* dz;  // dz_0 (n, H)
  int64_t n;
  int dim_in;
  float* partial_c;  // [slabs][H * H]: dz_0^T cos
  float* partial_s;  // [slabs][H * H]: dz_0^T sin
};

template <class W>
struct RffWgradSmem {
  float z[2][kWr0 * W::H];
  float c[2][kWr0 * W::H];
  float s[2][kWr0 * W::H];
};

template <class W>
__global__ __launch_bounds__(kThreads) void rff_wgrad0_kernel(const RffWgradArgs g) {
  __shared__ RffWgradSmem<W> sm;
  constexpr int H = W::H, TI = W::TI, TJ = W::TJ, RS = W::RS;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, lh = lane >> 5;
  // rows (n) / columns (k) of a half of dW_0 this wave owns, and its share of a chunk's row pairs
  const int tile = W::wide ? 0 : wave % W::tiles, split = W::wide ? 0 : wave / W::tiles;
  const int n_base = W::wide ? (wave >> 1) * TI * 32 : (tile / W::TD) * 32;
  const int k_base = W::wide ? (wave & 1) * TJ * 32 : (tile % W::TD) * 32;
  const int64_t chunks = (g.n + kWr0 - 1) / kWr0;
  const int64_t per = (chunks + gridDim.x - 1) / gridDim.x;
  const int64_t c_lo = (int64_t)blockIdx.x * per, c_hi = c_lo + per < chunks ? c_lo + per : chunks;
  // the encoding: thread <-> (frequency, group of rows); the frequency's row of b stays in registers
  const int col = tid % H, r0 = (tid / H) * W::rpt;
  const int dim_in = g.dim_in;
  float br[kFwdIn];
#pragma unroll
  for (int d = 0; d < kFwdIn; ++d) br[d] = d < dim_in ? g.b[col * dim_in + d] : 0.f;

  f32x16 acc[2][TI][TJ];  // [half: cos, sin]
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int ti = 0; ti < TI; ++ti)
#pragma unroll
      for (int tj = 0; tj < TJ; ++tj)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[h][ti][tj][r] = 0.f;

  auto issue = [&](int64_t c, int buf) {  // 32 rows of dz_0, contiguous in HBM
#pragma unroll
    for (int i = 0; i < (W::pieces + 7) / 8; ++i) {
      const int piece = wave + 8 * i;
      if (W::pieces % 8 != 0 && piece >= W::pieces) break;
      int64_t row = c * kWr0 + piece * (256 / H) + (lane * 4) / H;
      if (row >= g.n) row = g.n - 1;  // stays inside the buffer; such rows are zeroed below
      const int64_t src = row * H + (lane * 4) % H;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(g.dz + src),
                                       (__attribute__((address_space(3))) void*)(sm.z[buf] + piece * 256), 16, 0, 0);
    }
  };
  auto coords = [&](int64_t row) {  // (a wave's threads share the row: H >= 64)
    if (row >= g.n) row = g.n - 1;
    const float* __restrict__ p = g.x + row * dim_in;
    float4 v;
    v.x = p[0];
    v.y = dim_in > 1 ? p[1] : 0.f;
    v.z = dim_in > 2 ? p[2] : 0.f;
    v.w = dim_in > 3 ? p[3] : 0.f;
    return v;
  };
  auto encode = [&](int64_t c, int buf) {
#pragma unroll 1
    for (int r = 0; r < W::rpt; r += 2) {
      const float4 xa = coords(c * kWr0 + r0 + r), xb = coords(c * kWr0 + r0 + r + 1);
      const float u0 = rff_phase(xa, br), u1 = rff_phase(xb, br);
      float s0, c0, s1, c1;
      sincos_fast2(u0, u1, &s0, &c0, &s1, &c1);
      sm.c[buf][(r0 + r) * H + col] = c0;
      sm.c[buf][(r0 + r + 1) * H + col] = c1;
      sm.s[buf][(r0 + r) * H + col] = s0;
      sm.s[buf][(r0 + r + 1) * H + col] = s1;
    }
  };
  if (c_lo < c_hi) issue(c_lo, 0), encode(c_lo, 0);
  for (int64_t c = c_lo; c < c_hi; ++c) {
    const int buf = (int)(c - c_lo) & 1;
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // chunk c: dz_0 landed and cos / sin written, for every wave; the other buffers are free
    if (c + 1 < c_hi) issue(c + 1, buf ^ 1);
    if ((c + 1) * kWr0 > g.n) {  // the batch ends inside this chunk: rows beyond it contribute 0
      const int live = (int)(g.n - c * kWr0);
      for (int e = tid; e < (kWr0 - live) * H; e += kThreads) sm.z[buf][live * H + e] = 0.f;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
    const float* zp = sm.z[buf] + lh * H + n_base + l31;
    const float* cp = sm.c[buf] + lh * H + k_base + l31;
    const float* sp = sm.s[buf] + lh * H + k_base + l31;
    constexpr int kPairs = kWr0 / 2 / RS;  // row pairs of this wave: split, split + RS, ...
    // a 16-deep step contracts eight of the wave's row pairs: lane half lh holds row 2 pair + lh, element j of both
    // operands = pair split + (8 s + j) RS (siren_wgrad_kernel's operand map)
#pragma unroll
    for (int s = 0; s < kPairs / 8; ++s) {
      float raw[8];
      x3::Frag fz[TI];
#pragma unroll
      for (int ti = 0; ti < TI; ++ti) {
#pragma unroll
        for (int j = 0; j < 8; ++j) raw[j] = zp[2 * (split + (8 * s + j) * RS) * H + ti * 32];
        fz[ti] = x3::split8(raw);
      }
#pragma unroll
      for (int tj = 0; tj < TJ; ++tj) {
#pragma unroll
        for (int j = 0; j < 8; ++j) raw[j] = cp[2 * (split + (8 * s + j) * RS) * H + tj * 32];
        const x3::Frag fc = x3::split8(raw);
#pragma unroll
        for (int j = 0; j < 8; ++j) raw[j] = sp[2 * (split + (8 * s + j) * RS) * H + tj * 32];
        const x3::Frag fs = x3::split8(raw);
#pragma unroll
        for (int ti = 0; ti < TI; ++ti) {
          acc[0][ti][tj] = mma6_32(fz[ti], fc, acc[0][ti][tj]);
          acc[1][ti][tj] = mma6_32(fz[ti], fs, acc[1][ti][tj]);
        }
      }
    }
    if (c + 1 < c_hi) encode(c + 1, buf ^ 1);
  }
  const int64_t at = ((int64_t)blockIdx.x * RS + split) * H * H;
  // (H = 64: the `tiles` waves that share a split cover the whole H x H slab between them)
#pragma unroll
  for (int ti = 0; ti < TI; ++ti)
#pragma unroll
    for (int tj = 0; tj < TJ; ++tj)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int e = (n_base + ti * 32 + acc_row(r, lh)) * H + k_base + tj * 32 + l31;
        g.partial_c[at + e] = acc[0][ti][tj][r];
        g.partial_s[at + e] = acc[1][ti][tj][r];
      }
}

// ------------------------------------------------------------------------------------------------------ host side
// the fused chains' shape rule (inference, coordinate gradient, training), each argument refused by name
int check_rff_shape(const char* what, int dim_in, int hidden, int n_freq, int n_layers, int dim_out) {
  MRI_REQUIRE(hidden == 64 || hidden == 128, "%s: hidden = %d is not supported (64 / 128)", what, hidden);
  MRI_REQUIRE(n_freq == hidden, "%s: n_freq = %d is not supported (n_freq == hidden = %d)", what, n_freq, hidden);
  MRI_REQUIRE(dim_in >= 1 && dim_in <= kFwdIn, "%s: dim_in = %d is not supported (1 .. %d)", what, dim_in, kFwdIn);
  MRI_REQUIRE(n_layers >= 2 && n_layers <= kMaxSine, "%s: n_layers = %d is not supported (2 .. %d)", what, n_layers,
              kMaxSine);
  MRI_REQUIRE(dim_out == 1, "%s: dim_out = %d is not supported (1)", what, dim_out);
  return MRI_OK;
}
bool rff_supported(int dim_in, int hidden, int n_freq, int n_layers, int dim_out) {
  return check_rff_shape("fused RFF chain", dim_in, hidden, n_freq, n_layers, dim_out) == MRI_OK;
}
int rff_blocks(int hidden, int64_t n) {
  return persistent_blocks(n, hidden == 128 ? RShape<128>::rows : RShape<64>::rows);
}
// the two halves of the first Linear and the n_layers - 2 square ones
int64_t rff_split_bytes(int hidden, int n_layers) { return (int64_t)n_layers * split_matrix_bytes(hidden); }
// ... into `out`: Linear 0 is (H, 2F), its cos half starts at column 0, its sin half at column F, both with row stride 2F
int split_forward_weights(const float* const* weight, int hidden, int n_freq, int n_layers, char* out, hipStream_t st) {
  const int64_t smb = split_matrix_bytes(hidden);
  const float* const halves[2] = {weight[0], weight[0] + n_freq};
  if (int rc = split_weights_ld(halves, 2, hidden, 2 * n_freq, false, out, smb, st)) return rc;
  return split_weights_ld(weight + 1, n_layers - 2, hidden, hidden, false, out + 2 * smb, smb, st);
}
template <class S>
int launch_rff_gradient(const RffGradArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((rff_gradient_kernel<S>), dim3(persistent_blocks(a.n, S::points)), dim3(kThreads), 0, st, a);
  return check_launch("rff_gradient_kernel");
}

int check_encode(const float* x, int64_t n, int dim_in, const float* b, int n_freq) {
  MRI_REQUIRE(dim_in >= 1 && dim_in <= kEncIn, "RFF encoding: dim_in = %d is not supported (1 .. %d)", dim_in, kEncIn);
  MRI_REQUIRE(n_freq >= 1, "RFF encoding: n_freq = %d is not supported (>= 1)", n_freq);
  MRI_CHECK(check_rows(n));
  MRI_REQUIRE(n * n_freq < (1ll << 38), "n * n_freq = %lld out of range (one launch)", (long long)(n * n_freq));
  if (n == 0) return MRI_OK;
  return check_buffers({{"x", x}, {"b", b}}, 4);
}

}  // namespace
}  // namespace mri

using namespace mri;

extern "C" int mri_rff_encode(const float* x, int64_t n, int32_t dim_in, const float* b, int32_t n_freq, float* z,
                              void* stream) {
  MRI_CHECK(check_encode(x, n, dim_in, b, n_freq));
  if (n == 0) return MRI_OK;
  MRI_CHECK(check_buffer("z", z, 4));
  hipLaunchKernelGGL(rff_encode_kernel, dim3((unsigned)ceil_div(n * n_freq, 256)), dim3(256), 0, (hipStream_t)stream,
                     x, n, dim_in, b, n_freq, z);
  return check_launch("rff_encode_kernel");
}

extern "C" int mri_rff_encode_backward_input(const float* x, int64_t n, int32_t dim_in, const float* b,
                                             int32_t n_freq, const float* dz, float* dx, void* stream) {
  MRI_CHECK(check_encode(x, n, dim_in, b, n_freq));
  if (n == 0) return MRI_OK;
  MRI_CHECK(check_buffers({{"dz", dz}, {"dx", dx}}, 4));
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
  const char* const what = "fused RFF forward";
  MRI_CHECK(check_rff_shape(what, dim_in, hidden, n_freq, n_layers, 1));
  MRI_CHECK(check_rows(n));
  if (n == 0) return MRI_OK;
  MRI_CHECK(check_buffers({{"x", x}, {"b", b}, {"y", y}}, 4));
  MRI_CHECK(check_buffers({{"weight", weight}, {"bias", bias}}, kAnyAlignment));
  MRI_CHECK(check_workspace(what, "mri_rff_forward_workspace_bytes", workspace, workspace_bytes,
                            rff_split_bytes(hidden, n_layers)));
  MRI_CHECK(check_pointers({{"weight", weight}, {"bias", bias}}, 0, n_layers, 4));
  RffArgs a{};
  a.x = x, a.n = n, a.dim_in = dim_in, a.L = n_layers, a.b = b, a.y = y;
  std::copy(bias, bias + n_layers, a.bias);
  a.w_head = weight[n_layers - 1];
  a.wsplit = static_cast<const char*>(workspace);
  hipStream_t st = (hipStream_t)stream;
  if (int rc = split_forward_weights(weight, hidden, n_freq, n_layers, static_cast<char*>(workspace), st)) return rc;
  return dispatch_hidden_mod(hidden, [&](auto h) {
    using S = RShape<decltype(h)::value>;
    hipLaunchKernelGGL((rff_forward_kernel<false, S>), dim3(rff_blocks(hidden, n)), dim3(kThreads), 0, st, a);
    return check_launch("rff_forward_kernel");
  });
}

extern "C" int mri_rff_gradient_supported(int32_t dim_in, int32_t hidden, int32_t n_freq, int32_t n_layers,
                                          int32_t dim_out) {
  return rff_supported(dim_in, hidden, n_freq, n_layers, dim_out) ? 1 : 0;
}

extern "C" int64_t mri_rff_gradient_workspace_bytes(int32_t hidden, int32_t n_layers) {
  if (!rff_supported(1, hidden, hidden, n_layers, 1)) return -1;
  return rff_split_bytes(hidden, n_layers);
}

extern "C" int mri_rff_gradient(const float* x, int64_t n, int32_t dim_in, int32_t hidden, int32_t n_freq,
                                int32_t n_layers, const float* b, const float* const* weight,
                                const float* const* bias, float* y, float* dydx, void* workspace,
                                int64_t workspace_bytes, void* stream) {
  const char* const what = "fused RFF gradient";
  MRI_CHECK(check_rff_shape(what, dim_in, hidden, n_freq, n_layers, 1));
  MRI_CHECK(check_gradient_io(x, n, y, dydx));
  if (n == 0) return MRI_OK;
  MRI_CHECK(check_buffer("b", b, 4));
  MRI_CHECK(check_buffers({{"weight", weight}, {"bias", bias}}, kAnyAlignment));
  MRI_CHECK(check_workspace(what, "mri_rff_gradient_workspace_bytes", workspace, workspace_bytes,
                            rff_split_bytes(hidden, n_layers)));
  MRI_CHECK(check_pointers({{"weight", weight}, {"bias", bias}}, 0, n_layers, 4));
  RffGradArgs a{};
  a.x = x, a.n = n, a.dim_in = dim_in, a.L = n_layers, a.b = b, a.y = y, a.dydx = dydx;
  std::copy(bias, bias + n_layers, a.bias);
  a.w_head = weight[n_layers - 1];
  a.wsplit = static_cast<const char*>(workspace);
  hipStream_t st = (hipStream_t)stream;
  if (int rc = split_forward_weights(weight, hidden, n_freq, n_layers, static_cast<char*>(workspace), st)) return rc;
  return dispatch_hidden_mod(hidden, [&](auto h) {
    return dim_in <= 3 ? launch_rff_gradient<RGradShape<decltype(h)::value, 4>>(a, st)
                       : launch_rff_gradient<RGradShape<decltype(h)::value, 8>>(a, st);
  });
}

// ---------------------------------------------------------------------------------------------------- training
namespace mri {
namespace {

// workspace of the two training calls: [slabs of partial sums][forward splits: n_layers][transposed splits: n_layers - 2]
int64_t rff_slab_bytes(int64_t n, int hidden, int L) {
  const int64_t blocks = rff_blocks(hidden, n);
  // the chain kernel's slabs (the forward's loss shares fit inside), the square weight gradients' and dW_0's two halves
  const int64_t chain = std::max<int64_t>(blocks * RffBwdSlab{hidden, L}.floats(), 256);
  const int64_t bytes = std::max(chain, 2 * wgrad_slab_floats(n, hidden)) * 4;
  return (bytes + 255) / 256 * 256;
}
int64_t rff_train_bytes(int64_t n, int hidden, int L) {
  return rff_slab_bytes(n, hidden, L) + (int64_t)(2 * L - 2) * split_matrix_bytes(hidden);
}

}  // namespace
}  // namespace mri

extern "C" int mri_rff_train_supported(int32_t dim_in, int32_t hidden, int32_t n_freq, int32_t n_layers,
                                       int32_t dim_out) {
  return rff_supported(dim_in, hidden, n_freq, n_layers, dim_out) ? 1 : 0;
}

extern "C" int64_t mri_rff_backward_workspace_bytes(int64_t n, int32_t hidden, int32_t n_layers) {
  if (n < 1 || n >= (1ll << 31) || !rff_supported(1, hidden, hidden, n_layers, 1)) return -1;
  return rff_train_bytes(n, hidden, n_layers);
}

extern "C" int mri_rff_forward_loss(const float* x, const float* target, int64_t n, int64_t n_total, int32_t dim_in,
                                    int32_t hidden, int32_t n_freq, int32_t n_layers, const float* b,
                                    const float* const* weight, const float* const* bias, float grad_divisor,
                                    float* const* act, float* y, float* dy, float* loss_out, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
  const char* const what = "fused RFF forward with loss";
  MRI_CHECK(check_rff_shape(what, dim_in, hidden, n_freq, n_layers, 1));
  MRI_CHECK(check_batch_slice(n, n_total, grad_divisor));
  if (n == 0) return MRI_OK;
  MRI_CHECK(check_buffers({{"x", x}, {"target", target}, {"b", b}}, 4));
  MRI_CHECK(check_buffers({{"weight", weight}, {"bias", bias}, {"act", act}}, kAnyAlignment));
  MRI_CHECK(check_buffers({{"y", y}, {"dy", dy}, {"loss_out", loss_out}}, 4));
  MRI_CHECK(check_pointers({{"weight", weight}, {"bias", bias}}, 0, n_layers, 4));
  // (the weight-gradient kernels stream act in 16-byte pieces)
  MRI_CHECK(check_pointers({{"act", act}}, 0, n_layers - 1, 16));
  MRI_CHECK(check_workspace(what, "mri_rff_backward_workspace_bytes", workspace, workspace_bytes,
                            rff_train_bytes(n, hidden, n_layers)));
  RffArgs a{};
  a.x = x, a.n = n, a.dim_in = dim_in, a.L = n_layers, a.b = b, a.y = y;
  std::copy(bias, bias + n_layers, a.bias);
  std::copy(act, act + n_layers - 1, a.act);
  char* const wsplit = static_cast<char*>(workspace) + rff_slab_bytes(n, hidden, n_layers);
  a.w_head = weight[n_layers - 1], a.wsplit = wsplit;
  a.target = target, a.dy_out = dy, a.partial = static_cast<float*>(workspace);
  a.grad_scale = (float)(2.0 / ((double)n_total * (double)grad_divisor));
  a.inv_n = (float)(1.0 / (double)n_total);
  hipStream_t st = (hipStream_t)stream;
  if (int rc = split_forward_weights(weight, hidden, n_freq, n_layers, wsplit, st)) return rc;
  const int blocks = rff_blocks(hidden, n);
  if (int rc = dispatch_hidden_mod(hidden, [&](auto h) {
        using S = RShape<decltype(h)::value>;
        hipLaunchKernelGGL((rff_forward_kernel<true, S>), dim3(blocks), dim3(kThreads), 0, st, a);
        return check_launch("rff_forward_kernel");
      }))
    return rc;
  SegmentTable<1> t{};  // slabs of one float: the workgroups' loss shares, added in workgroup order
  t.vector(0, 1, loss_out);
  return reduce_slabs<1>(a.partial, blocks, 1, t, st);
}

extern "C" int mri_rff_backward(const float* x, const float* dy, int64_t n, int32_t dim_in, int32_t hidden,
                                int32_t n_freq, int32_t n_layers, const float* b, const float* const* weight,
                                const float* const* act, float* const* dz, float* const* d_weight,
                                float* const* d_bias, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* const what = "fused RFF backward";
  MRI_CHECK(check_rff_shape(what, dim_in, hidden, n_freq, n_layers, 1));
  MRI_CHECK(check_rows(n));
  if (n == 0) return MRI_OK;
  const int L = n_layers;
  MRI_CHECK(check_buffers({{"x", x}, {"dy", dy}, {"b", b}}, 4));
  MRI_CHECK(check_buffers({{"weight", weight}, {"act", act}, {"dz", dz}, {"d_weight", d_weight}, {"d_bias", d_bias}},
                          kAnyAlignment));
  MRI_CHECK(check_pointers({{"weight", weight}, {"d_weight", d_weight}, {"d_bias", d_bias}}, 0, L, 4));
  MRI_CHECK(check_pointers({{"act", act}, {"dz", dz}}, 0, L - 1, 16));
  MRI_CHECK(check_workspace(what, "mri_rff_backward_workspace_bytes", workspace, workspace_bytes,
                            rff_train_bytes(n, hidden, L)));
  RffBwdArgs a{};
  a.dy = dy, a.n = n, a.L = L;
  std::copy(act, act + L - 1, a.act);
  std::copy(dz, dz + L - 1, a.dz);
  a.w_head = weight[L - 1];
  a.partial = static_cast<float*>(workspace);
  const int64_t smb = split_matrix_bytes(hidden);
  char* const wtsplit = static_cast<char*>(workspace) + rff_slab_bytes(n, hidden, L) + (int64_t)L * smb;
  a.wtsplit = wtsplit;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = split_weights_ld(weight + 1, L - 2, hidden, hidden, true, wtsplit, smb, st)) return rc;
  const int blocks = rff_blocks(hidden, n);
  if (int rc = dispatch_hidden_mod(hidden, [&](auto h) {
        using S = RShape<decltype(h)::value>;
        hipLaunchKernelGGL((rff_backward_kernel<S>), dim3(blocks), dim3(kThreads), 0, st, a);
        return check_launch("rff_backward_kernel");
      }))
    return rc;
  const RffBwdSlab lay{hidden, L};
  if (int rc = reduce_slabs<1>(a.partial, blocks, lay.floats(), segments(lay, d_weight, d_bias), st)) return rc;
  for (int l = L - 2; l >= 1; --l) {  // dW_l = dz_l^T a_{l-1}
    WgradArgs g{};
    g.n = n, g.partial = static_cast<float*>(workspace), g.dz = dz[l], g.act = act[l - 1];
    if (int rc = wgrad_any_ld(hidden, g, d_weight[l], hidden, st)) return rc;
  }
  // dW_0 = [dz_0^T cos | dz_0^T sin]: the two halves' slabs lie behind one another
  RffWgradArgs g{};
  g.x = x, g.b = b, g.dz = dz[0], g.n = n, g.dim_in = dim_in;
  g.partial_c = static_cast<float*>(workspace);
  g.partial_s = g.partial_c + wgrad_slab_floats(n, hidden);
  const int wb = wgrad_blocks(n), slabs = wb * wgrad_split(hidden), count = hidden * hidden;
  if (int rc = dispatch_hidden_mod(hidden, [&](auto h) {
        using W = RffWgradShape<decltype(h)::value>;
        static_assert(W::RS == (W::H >= 128 ? 1 : 2), "wgrad_split");
        hipLaunchKernelGGL((rff_wgrad0_kernel<W>), dim3(wb), dim3(kThreads), 0, st, g);
        return check_launch("rff_wgrad0_kernel");
      }))
    return rc;
  if (int rc = sum_wgrad_slabs(g.partial_c, slabs, count, SlabDest{d_weight[0], hidden, hidden, 2 * n_freq}, st))
    return rc;
  return sum_wgrad_slabs(g.partial_s, slabs, count, SlabDest{d_weight[0] + n_freq, hidden, hidden, 2 * n_freq}, st);
}
