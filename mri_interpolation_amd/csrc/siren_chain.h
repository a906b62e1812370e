// Declarations shared by the two families of fused SIREN chain kernels: siren_chain.hip (the activation image of a
// row tile in LDS, every width) and siren_rows.hip (H = 256: the activations of a wave's rows in registers).
// modsiren.hip (ModulatedSirenNet: two images per row tile) shares the tile-loop device helpers below (namespace chain) and the
// weight-split / weight-gradient launches of siren_chain.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bf16x3.h"
#include "common.h"

namespace mri {

constexpr int kKc = 16;        // contraction depth of a weight chunk: one bf16 MFMA step
constexpr int kMaxSine = MRI_SIREN_MAX_LAYERS;  // sine layers, the first one included
constexpr int kMaxIn = 8;

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
  float* partial;                   // [gridDim.x][fwd_slab_floats]
  const char* wsplit;               // split W of layers 1 .. n_sine-1 (split_matrix_bytes each)
  float* dy_ws;                     // siren_rows.hip, loss mode: dLoss/dy per row, in the workspace (rows_dy_offset)
};

// loss-mode slab: dW_head [H] | db_last [H] | db_head, loss (padded to 4)
__host__ __device__ inline int fwd_slab_floats(int hidden) { return 2 * hidden + 4; }

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
  float* partial;                  // [gridDim.x][bwd_slab_floats]
  const char* wtsplit;             // split W^T of layers 1 .. n_sine-1 (split_matrix_bytes each)
  int head_done;                   // dz[n_sine-1] is an INPUT (the forward kernel's loss mode wrote it)
  const float* dy_ws;              // siren_rows.hip: dLoss/dy per row, where the loss-mode forward kernel left it
};

// slab: dW_head [H] | db_head [1] (padded to 4) | db_l [n_sine][H] | dW_first [H][kMaxIn]
__host__ __device__ inline int bwd_slab_floats(int hidden, int n_sine) {
  return hidden + 4 + n_sine * hidden + hidden * kMaxIn;
}


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

// ---- device helpers of the LDS-image tile loops (siren_chain.hip, modsiren.hip) ----------------------------------
namespace chain {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kThreads = 512;  // 8 waves

// row of register r of a 32x32 accumulator: (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
__device__ __forceinline__ int acc_row(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

// acc += A B over a 16-deep step, operands in their three bf16 terms: the six products, smallest first
__device__ __forceinline__ f32x16 mfma32x3(const x3::u32x4& a, const x3::u32x4& b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(x3::bf16x8, a),
                                                 __builtin_bit_cast(x3::bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mma6_32(const x3::Frag& a, const x3::Frag& b, f32x16 c) {
  c = mfma32x3(a.l, b.h, c);
  c = mfma32x3(a.h, b.l, c);
  c = mfma32x3(a.m, b.m, c);
  c = mfma32x3(a.m, b.h, c);
  c = mfma32x3(a.h, b.m, c);
  c = mfma32x3(a.h, b.h, c);
  return c;
}
__device__ __forceinline__ x3::Frag split_octets(const float4& lo, const float4& hi) {
  const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  return x3::split8(v);
}

// Queue the LDS-DMA of chunk kc of one split matrix into `dst`: 16-byte slots, lane = slot.  The
// slot a lane FETCHES is its LDS slot with the half bit XORed by bit 3 of the row, the involution
// the fragment reads undo: the 16 lanes of a ds_read_b128 group then touch 16 different slots.
template <class S>
__device__ __forceinline__ void issue_chunk(const char* __restrict__ wsplit, int kc, char* dst,
                                            int wave, int lane) {
  constexpr int slots = 6 * S::H;  // 3 planes x H rows x 2
  const char* src = wsplit + (int64_t)kc * S::chunk_bytes;
#pragma unroll
  for (int i = 0; i < (slots + kThreads - 1) / kThreads; ++i) {
    const int base = (wave + 8 * i) * 64;
    if (slots % kThreads != 0 && base >= slots) break;
    const int slot = base + lane, n = (slot >> 1) % S::H;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void*)(src + 16 * (slot ^ ((n >> 3) & 1))),
        (__attribute__((address_space(3))) void*)(dst + 16 * base), 16, 0, 0);
  }
}

// One 16-deep chunk of acc[t] += img[rows][k] * W[cols_t][k] for the wave's 32 x CT tile.  boff[t]: byte offset of
// the lane's slot of its column 32 t in a term plane.  The image operand is software-pipelined over the chunks of a
// layer (round 4): `fa` holds THIS chunk's fragment, already split (the image is complete when a layer starts, only
// the weights arrive chunk by chunk); the f32 words of the NEXT chunk's fragment (`a_next`: the lane's image row at
// that chunk's first k, + 4 lh; null for a layer's last chunk) are requested together with this chunk's weight
// fragments and split while this chunk's MFMAs execute.  Measured neutral against reading and splitting in front of
// the chunk's own MFMAs (config 3 12.82 against 12.81 ms, same flags, same box; EXPERIMENTS.md corrects the first
// claim); the weight fragments a chunk ahead as well (a three-deep DMA ring) measured slower.
template <int NT, int H>
__device__ __forceinline__ void mma_chunk(f32x16 (&acc)[NT], x3::Frag& fa, const float* __restrict__ a_next,
                                          const char* __restrict__ wb, const int (&boff)[NT]) {
  x3::Frag fb[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    fb[t].h = *reinterpret_cast<const x3::u32x4*>(wb + boff[t]);
    fb[t].m = *reinterpret_cast<const x3::u32x4*>(wb + H * 32 + boff[t]);
    fb[t].l = *reinterpret_cast<const x3::u32x4*>(wb + 2 * H * 32 + boff[t]);
  }
  float4 n_lo = {0.f, 0.f, 0.f, 0.f}, n_hi = n_lo;
  if (a_next) n_lo = *reinterpret_cast<const float4*>(a_next), n_hi = *reinterpret_cast<const float4*>(a_next + 8);
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = mma6_32(fa, fb[t], acc[t]);
  if (a_next) fa = split_octets(n_lo, n_hi);
}
// Scheduling pattern for a region of N MFMAs with LDS reads and vector work to hide beside them: after each of the
// first four MFMAs READS_PER LDS reads, after each of the others VALU_PER vector instructions.
template <int N, int READS_PER, int VALU_PER, int I = 0>
__device__ __forceinline__ void sched_interleave() {
  if constexpr (I < N) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    if constexpr (I < 4)
      __builtin_amdgcn_sched_group_barrier(0x100, READS_PER, 0);
    else
      __builtin_amdgcn_sched_group_barrier(0x002, VALU_PER, 0);
    sched_interleave<N, READS_PER, VALU_PER, I + 1>();
  }
}
// the first fragment of a layer (behind the barrier that completes the image)
__device__ __forceinline__ x3::Frag first_fragment(const float* __restrict__ a_k) {
  return split_octets(*reinterpret_cast<const float4*>(a_k), *reinterpret_cast<const float4*>(a_k + 8));
}

}  // namespace chain

}  // namespace mri
