// Declarations shared by the two families of fused SIREN chain kernels: siren_chain.hip (the activation image of a
// row tile in LDS, every width) and siren_rows.hip (H = 256: the activations of a wave's rows in registers).
// modsiren.hip (ModulatedSirenNet: two images per row tile) and the two coordinate-gradient files share the weight-split /
// weight-gradient launches of siren_chain.hip.  The device side of the LDS-image tile loop is chain_tile.h; what the
// entry points ask of their arguments (check_gradient_io among it) is entry_args.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "bf16x3.h"
#include "chain_tile.h"
#include "common.h"
#include "slab.h"

namespace mri {

struct ChainArgs {
  const float* x;                   // (n, dim_in) row-major
  int64_t n;
  int dim_in, n_sine;
  const float* w[kMaxSine + 1];     // [0] (H, dim_in); [1 .. n_sine-1] (H, H); [n_sine] (1, H)
  const float* b[kMaxSine + 1];
  float w0_first, w0;
  float* act[kMaxSine];             // (n, H) per sine layer, or null (inference)
  float* deriv[kMaxSine];
  float* y;                         // (n)
  // loss mode (MODE 2): the head's backward runs in the forward kernel's tail, where the last sine
  // layer's output and derivative are still in registers
  const float* target;              // (n)
  float grad_scale, inv_n;          // 2 / (n_total divisor), 1 / n_total
  float* dz_last;                   // (n, H): dLoss / d(pre-activation of the last sine layer)
  float* partial;                   // [gridDim.x][SirenFwdSlab]
  const char* wsplit;               // split W of layers 1 .. n_sine-1 (split_matrix_bytes each)
  float* dy_ws;                     // siren_rows.hip, loss mode: dLoss/dy per row, in the workspace (rows_dy_offset)
};

// Split weights (siren_split_weights_kernel): per H x H matrix, chunk kc = contraction indices
// [16 kc, 16 kc + 16), term planes h | m | l of [H rows][2 slots][8 bf16]; slot q of row n holds
// contraction indices 16 kc + 4 q + e and 16 kc + 8 + 4 q + e (e = 0..3): the eight positions lane
// half q of a 32x32x16 MFMA contracts when the other operand is read from the f32 image as two
// 16-byte fragments at k = 4 q and 8 + 4 q.  A chunk is contiguous: 3 x H x 32 bytes.
__host__ __device__ inline int64_t split_matrix_bytes(int H) { return (int64_t)(H / kKc) * 3 * H * 32; }

struct BwdArgs {
  const float* x;                  // (n, dim_in)
  const float* dy;                 // (n): dLoss / dy
  int64_t n;
  int dim_in, n_sine;
  const float* w[kMaxSine + 1];    // as ChainArgs
  const float* act_last;           // (n, H): output of the last sine layer
  const float* deriv[kMaxSine];    // (n, H) per sine layer: w0 cos(.)
  float* dz[kMaxSine];             // (n, H) for sine layers 1 .. n_sine-1 ([0] unused)
  float* partial;                  // [gridDim.x][SirenBwdSlab]
  const char* wtsplit;             // split W^T of layers 1 .. n_sine-1 (split_matrix_bytes each)
  int head_done;                   // dz[n_sine-1] is an INPUT (the forward kernel's loss mode wrote it)
  const float* dy_ws;              // siren_rows.hip: dLoss/dy per row, where the loss-mode forward kernel left it
};


struct WgradArgs {
  const float* dz;    // (n, H)
  const float* act;   // (n, H): the layer's input
  int64_t n;
  float* partial;     // [slabs][H * H]
};

// siren_rows.hip
bool rows_supported(int hidden, int n_sine);
int64_t rows_dy_offset(int64_t n, int hidden, int n_sine);  // bytes into the workspace's slab region
int rows_blocks(int64_t n);
int forward_rows(const ChainArgs& a, int mode, hipStream_t st);
bool rows_backward_supported(int hidden, int n_sine, int dim_in, int head_done);
int backward_rows(const BwdArgs& a, hipStream_t st);

// siren_chain.hip, for modsiren.hip: the weight-split and weight-gradient launches with leading dimensions.
// split_weights_ld: `count` matrices whose H x H block starts at w[m] with row stride `ld` floats; matrix m's planes go
// to out + m * out_stride bytes (layout: split_matrix_bytes).
int split_weights_ld(const float* const* w, int count, int hidden, int ld, bool transposed, char* out,
                     int64_t out_stride, hipStream_t st);
// dW[:, :H] += dz^T act, summed over the slabs in a fixed order into a row-major matrix of row stride `ld` floats
int wgrad_any_ld(int hidden, const WgradArgs& g, float* d_weight, int ld, hipStream_t st);
int64_t wgrad_slab_floats(int64_t n, int hidden);  // floats of WgradArgs::partial
// ... for rff.hip, whose first Linear's weight gradient has a kernel of its own on the same plan: the slab geometry
// (workgroups for n rows, slabs per workgroup) and slab_sum_kernel's launch: to += the `slabs` slabs of `count` floats
// at `partial`, in the tree order of slab.h
int wgrad_blocks(int64_t n);
int wgrad_split(int hidden);
int sum_wgrad_slabs(const float* partial, int slabs, int count, const SlabDest& to, hipStream_t st);

// ---- host-side helpers of the entry points -----------------------------------------------------------------------
// f(std::integral_constant<int, H>) for the hidden width of a plain chain (32 / 64 / 128 / 256, checked by the caller)
template <class F>
int dispatch_hidden(int hidden, F&& f) {
  switch (hidden) {
    case 32: return f(std::integral_constant<int, 32>{});
    case 64: return f(std::integral_constant<int, 64>{});
    case 128: return f(std::integral_constant<int, 128>{});
    default: return f(std::integral_constant<int, 256>{});
  }
}
// ... of a modulated chain (64 / 128)
template <class F>
int dispatch_hidden_mod(int hidden, F&& f) {
  return hidden == 128 ? f(std::integral_constant<int, 128>{}) : f(std::integral_constant<int, 64>{});
}

}  // namespace mri
