// Fused modulated-SIREN coordinate gradient for gfx950: y and dy/dx of ModulatedSirenNet(dim_in <= 3 -> H x L -> 1)
// from ONE walk of the two-image chain, forward mode.
//
// Replaces, for the coordinate gradient, autograd through the layer-by-layer forward (reference models.py:236-260
// Modulator.forward and :311-322 the layer loop of ModulatedSirenNet.forward).  Notation of modsiren.hip: z = x,
//   ps_l = a_{l-1} Ws_l^T + bs_l            pm_l = h_{l-1} Wm_l[:, :H]^T + z Wm_l[:, H:]^T + bm_l
//   s_l = sin(w_l ps_l)    h_l = relu(pm_l)    a_l = s_l (.) h_l    y = a_{L-1} . w_head + b_head
// and the tangents Th_l^d = d h_l / d x_d, Ta_l^d = d a_l / d x_d:
//   Th_0^d = [pm_0 > 0] (.) Wm_0[:, d]
//   Ta_0^d = w_0 cos(w_0 ps_0) (.) Ws_0[:, d] (.) h_0 + s_0 (.) Th_0^d
//   Th_l^d = [pm_l > 0] (.) (Th_{l-1}^d Wm_l[:, :H]^T + Wm_l[:, H + d])
//   Ta_l^d = w_l cos(w_l ps_l) (.) (Ta_{l-1}^d Ws_l^T) (.) h_l + s_l (.) Th_l^d
//   dy / dx_d = Ta_{L-1}^d . w_head                                            (ReLU'(0) = 0, as torch)
//
// The value row and the tangent rows of both images go through the same two matrix products as more rows, without
// bias, so the LDS-image tile loop (chain_tile.h), walked as modsiren_forward_kernel walks it with a Ws / Wm pair per
// layer, serves when both images hold, per POINT, four consecutive rows at a 4-aligned position: the value row (a, h) and the tangent rows of x_0, x_1, x_2 (Ta^d, Th^d); rows of absent
// axes and of points beyond n are never stored.  The accumulator layout of the 32x32 MFMA (acc_row) puts rows 4 q ..
// 4 q + 3 of a wave's row block into registers 4 q .. 4 q + 3 of ONE lane: the epilogue, where the tangent rows need
// the value row's w cos(.), s, h and sign, is lane-local -- no shuffles, no LDS traffic beyond the value row's z --
// and one register in four pays a sincos.  Nothing (n, H)-sized reaches memory: the call reads n dim_in floats and
// writes n (1 + dim_in).
//
// No atomics and a fixed summation order: two calls on the same input agree bitwise.
#include <algorithm>

#include "bf16x3.h"
#include "common.h"
#include "device_math.h"
#include "entry_args.h"
#include "siren_chain.h"

namespace mri {
namespace {

using namespace chain;

constexpr int kSlots = 4;         // image rows of a point: value, d/dx_0, d/dx_1, d/dx_2
constexpr int kGradIn = 3;        // axes the slots hold

// Geometry of modsiren.hip's MShape (a wave owns a 32 x 32 tile of BOTH layer outputs), the rows counted in points of
// four image rows: 64 rows = 16 points at H = 128, 128 rows = 32 points at H = 64.
template <int H>
using MGradShape = TileShape<H, 32, kSlots>;

struct MGradArgs {
  const float* x;  // (n, dim_in)
  int64_t n;
  int dim_in, L;
  const float* ws[kMaxSine + 1];  // SIREN stack: [0] (H, dim_in); [1 .. L-1] (H, H); [L] the head (1, H)
  const float* bs[kMaxSine + 1];
  const float* wm[kMaxSine];      // modulator: [0] (H, dim_in); [l] (H, H + dim_in), hidden columns first
  const float* bm[kMaxSine];
  float w0_first, w0;
  float* y;                       // (n)
  float* dydx;                    // (n, dim_in)
  const char* wsplit;             // per layer l = 1 .. L-1: split Ws_l | split Wm_l[:, :H] (split_matrix_bytes each)
};

template <class S>
struct MGradSmem {
  char wbuf[2][2][S::chunk_bytes] __attribute__((aligned(16)));  // [buffer][matrix: Ws, Wm]
  float img_a[S::rows * S::ld];     // point p in rows 4 p .. 4 p + 3: a, Ta^0, Ta^1, Ta^2
  float img_h[S::rows * S::ld];     //                                 h, Th^0, Th^1, Th^2
  float xs[S::points * kSlots] __attribute__((aligned(16)));  // coordinates of the tile's points, padded to 4
  float bias_s[kMaxSine][S::H];
  float bias_m[kMaxSine][S::H];
  float w_last[S::H];
};

template <class S>
__global__ __launch_bounds__(kThreads) void modsiren_gradient_kernel(const MGradArgs a) {
  __shared__ MGradSmem<S> sm;
  constexpr int H = S::H;
  constexpr int kPpt = S::points / S::groups;  // points per thread of layer 0's (column, group of points) mapping: 4
  static_assert(H == 64 || H == 128, "hidden width");
  static_assert(kPpt % 2 == 0 && kPpt * S::groups == S::points, "first-layer mapping");
  const Lanes<S> ln;
  const int tid = ln.tid, n0 = ln.n0;  // n0: this lane's output column
  const int L = a.L, n_mm = L - 1;
  const int dim_in = a.dim_in;

  for (int l = 0; l < L; ++l) load_vector<H>(sm.bias_s[l], a.bs[l], tid), load_vector<H>(sm.bias_m[l], a.bm[l], tid);
  load_vector<H>(sm.w_last, a.ws[L], tid);
  const float b_last = a.bs[L][0];

  const int64_t tiles = (a.n + S::points - 1) / S::points;
  const float* a_row = sm.img_a + ln.fragment_offset();
  const float* h_row = sm.img_h + ln.fragment_offset();
  int boff[1];
  ln.weight_offsets(boff);
  const int64_t smb = split_matrix_bytes(H);

  ChunkStream<S, 1> stream(n_mm, tiles);
  auto issue2 = [&](int layer, int kc, int buf) {  // both matrices of layer `layer` (1 .. L-1), chunk kc
    const char* base = a.wsplit + (int64_t)(2 * (layer - 1)) * smb;
    issue_chunk<S>(base, kc, sm.wbuf[buf][0], ln.wave, ln.lane);
    issue_chunk<S>(base + smb, kc, sm.wbuf[buf][1], ln.wave, ln.lane);
  };
  stream.prime(issue2);

  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t p0 = tile * S::points;  // first point of the tile
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // previous tile is done with the images / xs
    stage_coords<kSlots>(sm.xs, a.x, p0, S::points, a.n, dim_in, tid);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // ---- layer 0 of both stacks on the VALU: thread <-> (column, group of points), all four rows of both images ----
    {
      const int col = tid % H, q0 = (tid / H) * kPpt;
      float wsr[kGradIn], wmr[kGradIn];
#pragma unroll
      for (int d = 0; d < kGradIn; ++d) {  // (0 for an absent axis: its tangent rows come out as zeros)
        wsr[d] = d < dim_in ? a.ws[0][col * dim_in + d] : 0.f;
        wmr[d] = d < dim_in ? a.wm[0][col * dim_in + d] : 0.f;
      }
      const float bsj = sm.bias_s[0][col], bmj = sm.bias_m[0][col];
      const float w0f = a.w0_first;
#pragma unroll 1
      for (int i = 0; i < kPpt; i += 2) {
        float zs0 = 0.f, zs1 = 0.f, zm0 = 0.f, zm1 = 0.f;
#pragma unroll
        for (int d = 0; d < kGradIn; ++d) {
          const float x0 = sm.xs[(q0 + i) * kSlots + d], x1 = sm.xs[(q0 + i + 1) * kSlots + d];
          zs0 += x0 * wsr[d], zs1 += x1 * wsr[d];
          zm0 += x0 * wmr[d], zm1 += x1 * wmr[d];
        }
        float s0, c0, s1, c1;
        sincos_fast2(w0f * (zs0 + bsj), w0f * (zs1 + bsj), &s0, &c0, &s1, &c1);
        const float pm0 = zm0 + bmj, pm1 = zm1 + bmj;
        const bool live0 = p0 + q0 + i < a.n, live1 = p0 + q0 + i + 1 < a.n;
        const bool pos0 = pm0 > 0.f, pos1 = pm1 > 0.f;
        const float h0 = pos0 ? pm0 : 0.f, h1 = pos1 ? pm1 : 0.f;
        const float d0 = w0f * c0, d1 = w0f * c1;
        float* ra0 = sm.img_a + (q0 + i) * kSlots * S::ld + col;
        float* ra1 = ra0 + kSlots * S::ld;
        float* rh0 = sm.img_h + (q0 + i) * kSlots * S::ld + col;
        float* rh1 = rh0 + kSlots * S::ld;
        ra0[0] = live0 ? s0 * h0 : 0.f, ra1[0] = live1 ? s1 * h1 : 0.f;
        rh0[0] = live0 ? h0 : 0.f, rh1[0] = live1 ? h1 : 0.f;
#pragma unroll
        for (int d = 0; d < kGradIn; ++d) {
          const float th0 = pos0 ? wmr[d] : 0.f, th1 = pos1 ? wmr[d] : 0.f;
          rh0[(1 + d) * S::ld] = live0 ? th0 : 0.f;
          rh1[(1 + d) * S::ld] = live1 ? th1 : 0.f;
          ra0[(1 + d) * S::ld] = live0 ? (d0 * wsr[d]) * h0 + s0 * th0 : 0.f;
          ra1[(1 + d) * S::ld] = live1 ? (d1 * wsr[d]) * h1 + s1 * th1 : 0.f;
        }
      }
    }
    // ---- H x H layers: two products per layer ------------------------------------------------------------------------
    for (int l = 1; l <= n_mm; ++l) {
      f32x16 acc_s[1], acc_m[1];
#pragma unroll
      for (int r = 0; r < 16; ++r) acc_s[0][r] = 0.f, acc_m[0][r] = 0.f;
      x3::Frag fa, fh;
#pragma unroll
      for (int kc = 0; kc < S::chunks; ++kc, stream.consumed()) {
        stream.advance(tile, l, kc, issue2);
        if (kc == 0) fa = first_fragment(a_row), fh = first_fragment(h_row);
        mma_step<S>(acc_s, fa, a_row, kc, sm.wbuf[stream.buffer()][0], boff);
        mma_step<S>(acc_m, fh, h_row, kc, sm.wbuf[stream.buffer()][1], boff);
      }
      // ---- epilogue: registers 4 q .. 4 q + 3 are one point's value and tangent rows of both products ----------------
      float wt[kGradIn];
#pragma unroll
      for (int d = 0; d < kGradIn; ++d) wt[d] = d < dim_in ? a.wm[l][n0 * (H + dim_in) + H + d] : 0.f;
      const float bsj = sm.bias_s[l][n0], bmj = sm.bias_m[l][n0];
      const float w0 = a.w0;
      float pa[16], ph[16];
#pragma unroll
      for (int q = 0; q < 4; q += 2) {
        // the points of registers 4 q and 4 q + 4: image rows rb 32 + 8 q + 4 lh and + 8
        const int pt = ln.rb * (32 / kSlots) + 2 * q + ln.lh;
        const float4 x0 = *reinterpret_cast<const float4*>(sm.xs + pt * kSlots);
        const float4 x1 = *reinterpret_cast<const float4*>(sm.xs + (pt + 2) * kSlots);
        float t0 = x0.x * wt[0], t1 = x1.x * wt[0];
        t0 += x0.y * wt[1], t1 += x1.y * wt[1];
        t0 += x0.z * wt[2], t1 += x1.z * wt[2];
        const float pm0 = (acc_m[0][4 * q] + t0) + bmj, pm1 = (acc_m[0][4 * q + 4] + t1) + bmj;
        const bool pos0 = pm0 > 0.f, pos1 = pm1 > 0.f;
        const float h0 = pos0 ? pm0 : 0.f, h1 = pos1 ? pm1 : 0.f;
        float s0, c0, s1, c1;
        sincos_fast2(w0 * (acc_s[0][4 * q] + bsj), w0 * (acc_s[0][4 * q + 4] + bsj), &s0, &c0, &s1, &c1);
        const float d0 = w0 * c0, d1 = w0 * c1;
        pa[4 * q] = s0 * h0, pa[4 * q + 4] = s1 * h1;
        ph[4 * q] = h0, ph[4 * q + 4] = h1;
#pragma unroll
        for (int j = 1; j < 4; ++j) {
          const float th0 = pos0 ? acc_m[0][4 * q + j] + wt[j - 1] : 0.f;
          const float th1 = pos1 ? acc_m[0][4 * q + 4 + j] + wt[j - 1] : 0.f;
          ph[4 * q + j] = th0, ph[4 * q + 4 + j] = th1;
          pa[4 * q + j] = (d0 * acc_s[0][4 * q + j]) * h0 + s0 * th0;
          pa[4 * q + 4 + j] = (d1 * acc_s[0][4 * q + 4 + j]) * h1 + s1 * th1;
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();  // every wave has read both images for the last time
      store_acc<S>(sm.img_a, ln, pa);
      store_acc<S>(sm.img_h, ln, ph);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // image a complete
    // ---- head: image row of a . w_head, one wave per row; slot 0 -> y (+ bias), slot 1 + d -> dydx[:, d] -----------
    {
      const HeadDot<S> head(sm.w_last, ln.lane);
#pragma unroll 4
      for (int i = 0; i < S::rows / 8; ++i) {
        const int row = ln.wave * (S::rows / 8) + i;  // wave-uniform
        const int slot = row % kSlots;
        const int64_t p = p0 + row / kSlots;
        if (slot - 1 >= dim_in || p >= a.n) continue;
        const float acc1 = head(sm.img_a + row * S::ld);
        if (ln.lane == 0) {
          if (slot == 0)
            a.y[p] = acc1 + b_last;
          else
            a.dydx[p * dim_in + (slot - 1)] = acc1;
        }
      }
    }
  }
}

// the shapes of the fused training step (modsiren.hip) with at most kGradIn axes, each argument refused by name
int check_mgrad_shape(const char* what, int dim_in, int hidden, int n_layers, int dim_out) {
  MRI_REQUIRE(hidden == 64 || hidden == 128, "%s: hidden = %d is not supported (64 / 128)", what, hidden);
  MRI_REQUIRE(dim_in >= 1 && dim_in <= kGradIn, "%s: dim_in = %d is not supported (1 .. %d)", what, dim_in, kGradIn);
  MRI_REQUIRE(n_layers >= 2 && n_layers <= kMaxSine, "%s: n_layers = %d is not supported (2 .. %d)", what, n_layers,
              kMaxSine);
  MRI_REQUIRE(dim_out == 1, "%s: dim_out = %d is not supported (1)", what, dim_out);
  return MRI_OK;
}
bool mgrad_supported(int dim_in, int hidden, int n_layers, int dim_out) {
  return check_mgrad_shape("modulated SIREN gradient", dim_in, hidden, n_layers, dim_out) == MRI_OK;
}

int64_t mgrad_split_bytes(int hidden, int L) { return 2 * (int64_t)(L - 1) * split_matrix_bytes(hidden); }

template <int H>
int launch_mgrad(const MGradArgs& a, hipStream_t st) {
  using S = MGradShape<H>;
  hipLaunchKernelGGL((modsiren_gradient_kernel<S>), dim3(persistent_blocks(a.n, S::points)), dim3(kThreads), 0, st, a);
  return check_launch("modsiren_gradient_kernel");
}

}  // namespace
}  // namespace mri

using namespace mri;

extern "C" int mri_modsiren_gradient_supported(int32_t dim_in, int32_t hidden, int32_t n_layers, int32_t dim_out) {
  return mgrad_supported(dim_in, hidden, n_layers, dim_out) ? 1 : 0;
}

extern "C" int64_t mri_modsiren_gradient_workspace_bytes(int32_t hidden, int32_t n_layers) {
  if (!mgrad_supported(1, hidden, n_layers, 1)) return -1;
  return mgrad_split_bytes(hidden, n_layers);
}

extern "C" int mri_modsiren_gradient(const float* x, int64_t n, int32_t dim_in, int32_t hidden, int32_t n_layers,
                                     const float* const* siren_weight, const float* const* siren_bias,
                                     const float* const* mod_weight, const float* const* mod_bias, float w0_first,
                                     float w0, float* y, float* dydx, void* workspace, int64_t workspace_bytes,
                                     void* stream) {
  const char* const what = "modulated SIREN gradient";
  MRI_CHECK(check_mgrad_shape(what, dim_in, hidden, n_layers, 1));
  MRI_CHECK(check_gradient_io(x, n, y, dydx));
  if (n == 0) return MRI_OK;
  MRI_CHECK(check_buffers({{"siren_weight", siren_weight}, {"siren_bias", siren_bias}, {"mod_weight", mod_weight},
                           {"mod_bias", mod_bias}}, kAnyAlignment));
  MRI_CHECK(check_workspace(what, "mri_modsiren_gradient_workspace_bytes", workspace, workspace_bytes,
                            mgrad_split_bytes(hidden, n_layers)));
  // (a NULL entry keeps this entry point's first wording, which says which of the two networks and which layer)
  for (int l = 0; l <= n_layers; ++l)
    MRI_REQUIRE(siren_weight[l] && siren_bias[l], "NULL SIREN parameter pointer (layer %d)", l);
  MRI_CHECK(check_pointers({{"siren_weight", siren_weight}}, 0, n_layers + 1, 16));
  for (int l = 0; l < n_layers; ++l)
    MRI_REQUIRE(mod_weight[l] && mod_bias[l], "NULL modulator parameter pointer (layer %d)", l);
  MRI_CHECK(check_pointers({{"mod_weight", mod_weight}}, 0, n_layers, 16));
  MGradArgs a{};
  a.x = x, a.n = n, a.dim_in = dim_in, a.L = n_layers, a.w0_first = w0_first, a.w0 = w0, a.y = y, a.dydx = dydx;
  std::copy(siren_weight, siren_weight + n_layers + 1, a.ws);
  std::copy(siren_bias, siren_bias + n_layers + 1, a.bs);
  std::copy(mod_weight, mod_weight + n_layers, a.wm);
  std::copy(mod_bias, mod_bias + n_layers, a.bm);
  a.wsplit = static_cast<const char*>(workspace);
  hipStream_t st = (hipStream_t)stream;
  char* const out = static_cast<char*>(workspace);
  const int64_t smb = split_matrix_bytes(hidden);
  if (int rc = split_weights_ld(siren_weight + 1, n_layers - 1, hidden, hidden, false, out, 2 * smb, st)) return rc;
  if (int rc = split_weights_ld(mod_weight + 1, n_layers - 1, hidden, hidden + dim_in, false, out + smb, 2 * smb, st))
    return rc;
  return dispatch_hidden_mod(hidden, [&](auto h) { return launch_mgrad<decltype(h)::value>(a, st); });
}
