// Fused SIREN coordinate gradient for gfx950: y and dy/dx of SirenNet(dim_in <= 4 -> H x n -> 1) from ONE walk of
// the chain, forward mode.
//
// With a_l = sin(w_l z_l), z_l = a_{l-1} W_l^T + b_l and the tangent T_l^d = d a_l / d x_d:
//
//   T_0^d = w_0 cos(w_0 z_0) (.) W_0[:, d]
//   T_l^d = (w_l cos(w_l z_l)) (.) (T_{l-1}^d W_l^T)       the product of the value row, on more rows, without bias
//   dy / dx_d = T_{L-1}^d . w_head
//
// so the LDS-image tile loop (chain_tile.h), walked as siren_forward_kernel walks it in inference mode, serves when
// the activation image holds, per POINT, four consecutive rows at a 4-aligned position: the value row and the tangent rows of x_0,
// x_1, x_2 (rows of absent axes and of points beyond n are zero and are never stored).  The accumulator layout of the
// 32x32 MFMA (acc_row) puts rows 4 q .. 4 q + 3 of a wave's row block into registers 4 q .. 4 q + 3 of ONE lane: the
// epilogue, where the tangent rows need the value row's w cos(.), is lane-local -- no shuffles, no LDS traffic --
// and only one register in four pays a sincos.  The weight chunks (LDS-DMA, double buffered), the bf16x3 products
// and the split weights are those of the forward kernel (chain_tile.h, siren_chain.h); nothing (n, H)-sized reaches memory: the
// call reads n dim_in floats and writes n (1 + dim_in).
//
// dim_in = 4 (a dynamic sequence: x, y, z, t) takes the EIGHT-slot instantiation of the same kernel body: a point's
// rows sit at an 8-aligned position in the order [value, d/dx_0, d/dx_1, d/dx_2 | value, d/dx_3, 0, 0].  acc_row puts
// rows 8 q .. 8 q + 3 into registers 4 q .. 4 q + 3 of lane l31 and rows 8 q + 4 .. 8 q + 7 into the same registers of
// lane l31 + 32, so with the value row written TWICE by the first layer (the rows of an MFMA are independent: the
// copy in slot 4 stays identical to slot 0 through every layer) register 4 q is a value row and 4 q + 1 .. 4 q + 3
// are its tangents in BOTH lane halves: the epilogue is the four-slot form's expression, still lane-local, and the
// copy's sincos runs in the instructions the wave issues anyway.  A tile holds half the points (8 / 16 / 32 / 32);
// the image, its stride and the weight stream are unchanged.  The head skips slots 4, 6 and 7.
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

constexpr int kGradMaxIn = 4;   // axes the eight-slot form holds (the four-slot form: 3)

// Geometry for hidden width H: that of the forward kernel (image rows of a tile: 64, 128, 256, 256 for H = 256 .. 32),
// the rows counted in points of SL image rows: 4 (value, d/dx_0, d/dx_1, d/dx_2) for dim_in <= 3, 8 (value, d/dx_0 ..
// d/dx_2 | value, d/dx_3, 0, 0) for dim_in = 4.  Points of a tile: 16, 32, 64, 64 (8 slots: 8, 16, 32, 32).
template <int HH, int SL>
struct GradShape : TileShape<HH, 64, SL> {
  using T = TileShape<HH, 64, SL>;
  static constexpr int max_in = SL == 4 ? 3 : 4;        // axes the slots hold
  static constexpr int ppt = T::points / T::groups;     // points per thread of the first layer: 8, 8, 8, 4 (8 slots: 4, 4, 4, 2)
  static_assert(SL == 4 || SL == 8, "image rows per point");
  static_assert(ppt % 2 == 0 && ppt * T::groups == T::points, "first-layer mapping");
};

template <class S>
struct GradSmem {
  char wbuf[2][S::chunk_bytes] __attribute__((aligned(16)));  // weight chunks: term planes [n][2 slots of 8 bf16]
  float img[S::rows * S::ld];        // the tile's image: point p in rows slots p .. slots p + slots - 1
  float xs[S::points * S::slots];    // coordinates of the tile's points, padded to slots
  float bias[kMaxSine][S::H];
  float w_last[S::H];
};

struct GradArgs {
  const float* x;                  // (n, dim_in) row-major
  int64_t n;
  int dim_in, n_sine;
  const float* w[kMaxSine + 1];    // [0] (H, dim_in); [1 .. n_sine-1] (H, H); [n_sine] (1, H)
  const float* b[kMaxSine + 1];
  float w0_first, w0;
  float* y;                        // (n)
  float* dydx;                     // (n, dim_in) row-major
  const char* wsplit;              // split W of layers 1 .. n_sine-1 (split_matrix_bytes each)
};

template <class S>
__global__ __launch_bounds__(kThreads) void siren_gradient_kernel(const GradArgs a) {
  __shared__ GradSmem<S> sm;
  constexpr int H = S::H, NT = S::NT, kSlots = S::slots, kMaxIn = S::max_in;
  const Lanes<S> ln;
  const int tid = ln.tid;
  const int n_mm = a.n_sine - 1;  // H x H layers

  // ---- small resident parameters ------------------------------------------------------------
  for (int l = 0; l < a.n_sine; ++l) load_vector<H>(sm.bias[l], a.b[l], tid);
  load_vector<H>(sm.w_last, a.w[a.n_sine], tid);
  const float b_last = a.b[a.n_sine][0];

  const int64_t tiles = (a.n + S::points - 1) / S::points;
  const float* a_row = sm.img + ln.fragment_offset();
  int boff[NT];
  ln.weight_offsets(boff);

  ChunkStream<S, 1> stream(n_mm, tiles);
  auto issue = [&](int layer, int kc, int buf) {  // the matrix of layer `layer` (1 .. n_mm), chunk kc
    issue_chunk<S>(a.wsplit + (layer - 1) * split_matrix_bytes(H), kc, sm.wbuf[buf], ln.wave, ln.lane);
  };
  stream.prime(issue);

  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t p0 = tile * S::points;  // first point of the tile
    // ---- coordinates -> LDS ---------------------------------------------------------------------
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // previous tile is done with img / xs
    stage_coords<kSlots>(sm.xs, a.x, p0, S::points, a.n, a.dim_in, tid);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // ---- first layer on the VALU: thread <-> (column, group of points) --------------------------
    {
      const int col = tid % H, q0 = (tid / H) * S::ppt;
      float wr[kMaxIn];
#pragma unroll
      for (int d = 0; d < kMaxIn; ++d) wr[d] = d < a.dim_in ? a.w[0][col * a.dim_in + d] : 0.f;
      const float bias = sm.bias[0][col];
#pragma unroll
      for (int i = 0; i < S::ppt; i += 2) {
        float z0 = 0.f, z1 = 0.f;
#pragma unroll
        for (int d = 0; d < kMaxIn; ++d) {
          if (d < a.dim_in) {
            z0 += sm.xs[(q0 + i) * kSlots + d] * wr[d];
            z1 += sm.xs[(q0 + i + 1) * kSlots + d] * wr[d];
          }
        }
        float s0, c0, s1, c1;
        sincos_fast2(a.w0_first * (z0 + bias), a.w0_first * (z1 + bias), &s0, &c0, &s1, &c1);
        const bool live0 = p0 + q0 + i < a.n, live1 = p0 + q0 + i + 1 < a.n;
        const float d0 = a.w0_first * c0, d1 = a.w0_first * c1;
        float* r0 = sm.img + (q0 + i) * kSlots * S::ld + col;
        float* r1 = r0 + kSlots * S::ld;
        r0[0] = live0 ? s0 : 0.f;
        r1[0] = live1 ? s1 : 0.f;
#pragma unroll
        for (int d = 0; d < 3; ++d) {  // (wr[d] = 0 for an absent axis)
          r0[(1 + d) * S::ld] = live0 ? d0 * wr[d] : 0.f;
          r1[(1 + d) * S::ld] = live1 ? d1 * wr[d] : 0.f;
        }
        if constexpr (kSlots == 8) {  // upper lane half of the accumulator: the value row again, d/dx_3, two zero rows
          r0[4 * S::ld] = live0 ? s0 : 0.f;
          r1[4 * S::ld] = live1 ? s1 : 0.f;
          r0[5 * S::ld] = live0 ? d0 * wr[3] : 0.f;
          r1[5 * S::ld] = live1 ? d1 * wr[3] : 0.f;
          r0[6 * S::ld] = r0[7 * S::ld] = 0.f;
          r1[6 * S::ld] = r1[7 * S::ld] = 0.f;
        }
      }
    }
    // ---- H x H layers --------------------------------------------------------------------------
    for (int l = 1; l <= n_mm; ++l) {
      f32x16 acc[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
      x3::Frag fa;
#pragma unroll
      for (int kc = 0; kc < S::chunks; ++kc, stream.consumed()) {
        stream.advance(tile, l, kc, issue);
        if (kc == 0) fa = first_fragment(a_row);  // (the stream's barrier completed the image)
        mma_step<S>(acc, fa, a_row, kc, sm.wbuf[stream.buffer()], boff);
      }
      // ---- epilogue: registers 4 q .. 4 q + 3 are one point's value and tangent rows (8 slots: of either half
      //      of the point, the value row being there twice) -----------------------------------------------
      const float w0 = a.w0;
      float pa[NT][16];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const float bj = sm.bias[l][ln.n0 + 32 * t];
#pragma unroll
        for (int q = 0; q < 4; q += 2) {
          float s0, c0, s1, c1;
          sincos_fast2(w0 * (acc[t][4 * q] + bj), w0 * (acc[t][4 * q + 4] + bj), &s0, &c0, &s1, &c1);
          const float d0 = w0 * c0, d1 = w0 * c1;
          pa[t][4 * q] = s0, pa[t][4 * q + 4] = s1;
#pragma unroll
          for (int j = 1; j < 4; ++j) {
            pa[t][4 * q + j] = d0 * acc[t][4 * q + j];
            pa[t][4 * q + 4 + j] = d1 * acc[t][4 * q + 4 + j];
          }
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();  // every wave has read the image for the last time
#pragma unroll
      for (int t = 0; t < NT; ++t) store_acc<S>(sm.img, ln, pa[t], t);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // image complete
    // ---- head: image row . w_head, one wave per row; slot 0 -> y (+ bias), slot 1 + d -> dydx[:, d]; of the
    //      upper four of 8 slots only slot 5 -> dydx[:, 3] is stored ------------------------------------------
    {
      const HeadDot<S> head(sm.w_last, ln.lane);
#pragma unroll 4
      for (int i = 0; i < S::rows / 8; ++i) {
        const int row = ln.wave * (S::rows / 8) + i;  // wave-uniform
        const int slot = row % kSlots;
        const int64_t p = p0 + row / kSlots;
        const int axis = slot < 4 ? slot - 1 : (slot == 5 ? 3 : kMaxIn);  // wave-uniform; -1: the value
        if (axis >= a.dim_in || p >= a.n) continue;
        const float acc1 = head(sm.img + row * S::ld);
        if (ln.lane == 0) {
          if (slot == 0)
            a.y[p] = acc1 + b_last;
          else
            a.dydx[p * a.dim_in + axis] = acc1;
        }
      }
    }
  }
}

// dim_in = 4 is served by the eight-slot form for exactly the cases of the four-slot form.
int check_gradient_shape(const char* what, int dim_in, int hidden, int n_sine, int dim_out) {
  MRI_REQUIRE(hidden == 32 || hidden == 64 || hidden == 128 || hidden == 256,
              "%s: hidden = %d is not supported (32 / 64 / 128 / 256)", what, hidden);
  MRI_REQUIRE(dim_in >= 1 && dim_in <= kGradMaxIn, "%s: dim_in = %d is not supported (1 .. %d)", what, dim_in,
              kGradMaxIn);
  MRI_REQUIRE(n_sine >= 1 && n_sine <= kMaxSine, "%s: n_sine_layers = %d is not supported (1 .. %d)", what, n_sine,
              kMaxSine);
  MRI_REQUIRE(dim_out == 1, "%s: dim_out = %d is not supported (1)", what, dim_out);
  return MRI_OK;
}
bool gradient_supported(int dim_in, int hidden, int n_sine, int dim_out) {
  return check_gradient_shape("SIREN gradient", dim_in, hidden, n_sine, dim_out) == MRI_OK;
}

int64_t gradient_split_bytes(int hidden, int n_sine) {
  return n_sine > 1 ? (n_sine - 1) * split_matrix_bytes(hidden) : 0;
}

template <int H, int SL>
int launch_slots(const GradArgs& a, hipStream_t st) {
  using S = GradShape<H, SL>;
  hipLaunchKernelGGL((siren_gradient_kernel<S>), dim3(persistent_blocks(a.n, S::points)), dim3(kThreads), 0, st, a);
  return check_launch("siren_gradient_kernel");
}

template <int H>
int launch_gradient(const GradArgs& a, hipStream_t st) {
  return a.dim_in <= 3 ? launch_slots<H, 4>(a, st) : launch_slots<H, 8>(a, st);
}

}  // namespace
}  // namespace mri

using namespace mri;

extern "C" int mri_siren_gradient_supported(int32_t dim_in, int32_t hidden, int32_t n_sine_layers,
                                            int32_t dim_out) {
  return gradient_supported(dim_in, hidden, n_sine_layers, dim_out) ? 1 : 0;
}

extern "C" int64_t mri_siren_gradient_workspace_bytes(int32_t hidden, int32_t n_sine_layers) {
  if (!gradient_supported(1, hidden, n_sine_layers, 1)) return -1;
  return gradient_split_bytes(hidden, n_sine_layers);
}

extern "C" int mri_siren_gradient(const float* x, int64_t n, int32_t dim_in, int32_t hidden,
                                  int32_t n_sine_layers, const float* const* weight,
                                  const float* const* bias, float w0_first, float w0, float* y, float* dydx,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
  const char* const what = "SIREN gradient";
  MRI_CHECK(check_gradient_shape(what, dim_in, hidden, n_sine_layers, 1));
  MRI_CHECK(check_gradient_io(x, n, y, dydx));
  if (n == 0) return MRI_OK;
  MRI_CHECK(check_buffers({{"weight", weight}, {"bias", bias}}, kAnyAlignment));
  MRI_CHECK(check_workspace(what, "mri_siren_gradient_workspace_bytes", workspace, workspace_bytes,
                            gradient_split_bytes(hidden, n_sine_layers)));
  MRI_CHECK(check_pointers({{"weight", weight}}, 0, n_sine_layers + 1, 16));
  MRI_CHECK(check_pointers({{"bias", bias}}, 0, n_sine_layers + 1, kAnyAlignment));
  GradArgs a{};
  a.x = x, a.n = n, a.dim_in = dim_in, a.n_sine = n_sine_layers;
  a.w0_first = w0_first, a.w0 = w0, a.y = y, a.dydx = dydx;
  std::copy(weight, weight + n_sine_layers + 1, a.w);
  std::copy(bias, bias + n_sine_layers + 1, a.b);
  a.wsplit = static_cast<const char*>(workspace);
  hipStream_t st = (hipStream_t)stream;
  if (int rc = split_weights_ld(weight + 1, n_sine_layers - 1, hidden, hidden, false, static_cast<char*>(workspace),
                                split_matrix_bytes(hidden), st))
    return rc;
  return dispatch_hidden(hidden, [&](auto h) { return launch_gradient<decltype(h)::value>(a, st); });
}
