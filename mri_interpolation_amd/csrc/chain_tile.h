// The device side of the LDS-image tile loop (namespace chain).  Ten persistent kernels walk it: siren_forward_kernel
// and siren_backward_kernel (siren_chain.hip), modsiren_forward_kernel and modsiren_backward_kernel (modsiren.hip),
// siren_gradient_kernel (siren_gradient.hip), modsiren_gradient_kernel (modsiren_gradient.hip), rff_forward_kernel,
// rff_gradient_kernel and rff_backward_kernel (rff.hip), gabor_forward_kernel (gabor.hip: the pair form of the
// matrix step, one image fragment for two weight matrices).  Their epilogues
// differ and stay with them; what they decide alike is written here once:
//
//   TileShape            the geometry of a tile for a hidden width
//   Lanes                where a lane sits in it: its fragment row, its output column, its accumulator rows
//   slot_swizzle         the LDS slot swizzle of a weight chunk: issue_chunk writes it, weight_slot_offset reads it
//   ChunkStream          the order of the weight-chunk stream: which chunk follows chunk s, and into which buffer
//   acc_row              accumulator register -> image row; store_acc / Lanes::row / Lanes::global_offset build on it
//   stage_coords, load_vector, HeadDot   the blocks every kernel has: coordinates and resident vectors into LDS, the
//                        head's row . w_head
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bf16x3.h"

namespace mri {

constexpr int kKc = 16;        // contraction depth of a weight chunk: one bf16 MFMA step

namespace chain {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kThreads = 512;  // 8 waves

// Geometry for hidden width H: a wave owns a 32 x CT tile of the (rows x H) layer output, CT = min(H, CT_CAP): 64
// columns for the kernels with one image, 32 for those with two, which so take half the rows and the same ~66 KiB
// of images.  The 8 waves are RB row blocks x CB column blocks, so narrower networks take taller tiles.  SL: image
// rows per point (1; 4 or 8 for the coordinate gradients, whose tiles count in points).
template <int HH, int CT_CAP, int SL = 1>
struct TileShape {
  static constexpr int H = HH;
  static constexpr int slots = SL;
  static constexpr int CT = H < CT_CAP ? H : CT_CAP;  // columns of a wave's tile
  static constexpr int NT = CT / 32;                  // 32 x 32 MFMA tiles per wave
  static constexpr int CB = H / CT, RB = 8 / CB;      // column / row blocks of the 8 waves
  static constexpr int rows = 32 * RB;                // image rows of a tile
  static constexpr int points = rows / SL;            // points of a tile
  static constexpr int ld = H + 4;                    // image row stride: rows 4 banks apart (mod 64)
  static constexpr int chunks = H / kKc;              // weight chunks per layer (and matrix)
  static constexpr int chunk_bytes = 3 * H * 32;      // a weight chunk: three term planes of [H][16] bf16
  static constexpr int groups = kThreads / H;         // row / point groups of the (column, group) phases
  static_assert(H == 32 || H == 64 || H == 128 || H == 256, "hidden width");
  static_assert(CT_CAP == 32 || CT_CAP == 64, "column tile of a wave");
  static_assert(SL == 1 || SL == 4 || SL == 8, "image rows per point");
};

// row of register r of a 32x32 accumulator: (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
__device__ __forceinline__ int acc_row(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

// Weight chunk in LDS: term planes of [row][2 slots of 16 bytes].  A row's two slots are stored swapped when bit 3 of
// the row is set, so that the 16 lanes of a ds_read_b128 group touch 16 different slots.  XOR with this bit is an
// involution: issue_chunk applies it to the slot it FETCHES, weight_slot_offset to the slot it READS, and the two
// cancel.  No other code knows the swizzle.
__device__ __forceinline__ int slot_swizzle(int row) { return (row >> 3) & 1; }

// Queue the LDS-DMA of chunk kc of one split matrix into `dst`: 16-byte slots, lane = slot.
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
        (const __attribute__((address_space(1))) void*)(src + 16 * (slot ^ slot_swizzle(n))),
        (__attribute__((address_space(3))) void*)(dst + 16 * base), 16, 0, 0);
  }
}
// byte offset, in a term plane, of the slot lane half lh reads for output column `col`
__device__ __forceinline__ int weight_slot_offset(int col, int lh) { return 32 * col + 16 * (lh ^ slot_swizzle(col)); }

// Where this lane sits in the tile.
template <class S>
struct Lanes {
  const int tid, lane, wave, l31, lh;
  const int rb, cb;  // the wave's row / column block
  const int n0;      // the lane's output column in MFMA tile 0; tile t: + 32 t
  __device__ __forceinline__ Lanes()
      : tid(threadIdx.x), lane(tid & 63), wave(__builtin_amdgcn_readfirstlane(tid >> 6)), l31(lane & 31),
        lh(lane >> 5), rb(wave / S::CB), cb(wave % S::CB), n0(cb * S::CT + l31) {}
  // the lane's A-operand fragments in an image: its row at k = 4 lh, as an element offset; chunk kc: + 16 kc
  __device__ __forceinline__ int fragment_offset() const { return (rb * 32 + l31) * S::ld + 4 * lh; }
  // image row of accumulator register r
  __device__ __forceinline__ int row(int r) const { return rb * 32 + acc_row(r, lh); }
  // element offset of (row(0), n0) in a tile's row-major (rows, H) block in global memory; register r of MFMA
  // tile t: + acc_row(r, 0) H + 32 t
  __device__ __forceinline__ int global_offset() const { return (rb * 32 + 4 * lh) * S::H + n0; }
  // the tile's rows from row(0) down that exist, given the rows from the tile's first row down
  __device__ __forceinline__ int64_t rows_left(int64_t from_tile_top) const { return from_tile_top - rb * 32 - 4 * lh; }
  // the lane's B-operand slots of a weight chunk, per MFMA tile
  __device__ __forceinline__ void weight_offsets(int (&boff)[S::NT]) const {
#pragma unroll
    for (int t = 0; t < S::NT; ++t) boff[t] = weight_slot_offset(n0 + 32 * t, lh);
  }
};

// The weight-chunk stream of a workgroup.  Chunk s -- counted over layers and tiles -- lives in buffer s & 1, and its
// follower is queued as soon as every wave is done with chunk s - 1: the next k-chunk of this layer; otherwise chunk
// 0 of the next layer in walk order; otherwise, only if this workgroup has another tile, chunk 0 of that tile's
// first layer.  STEP: + 1 walks the H x H layers 1 .. n_mm (the forward kernels), - 1 walks n_mm .. 1 (the backward
// kernels).  `issue(layer, kc, buffer)` queues chunk kc of that layer: one matrix, or a Ws / Wm pair.
template <class S, int STEP>
struct ChunkStream {
  static_assert(STEP == 1 || STEP == -1, "walk direction");
  const int n_mm;
  const int64_t tiles;
  int s = 0;
  __device__ __forceinline__ ChunkStream(int n_mm_, int64_t tiles_) : n_mm(n_mm_), tiles(tiles_) {}
  __device__ __forceinline__ int first_layer() const { return STEP > 0 ? 1 : n_mm; }
  __device__ __forceinline__ int buffer() const { return s & 1; }  // of the chunk the MFMAs read now
  __device__ __forceinline__ void consumed() { ++s; }

  // chunk 0 of the first layer, if there is a layer and this workgroup has a tile
  template <class Issue>
  __device__ __forceinline__ void prime(Issue&& issue) const {
    if (n_mm > 0 && (int64_t)blockIdx.x < tiles) issue(first_layer(), 0, 0);
  }
  // In front of chunk kc of layer l of `tile`: wait until chunk s has landed, queue its follower.  `mark` runs
  // between the barrier and the issue (the profiling build's clock reads).
  template <class Issue, class Mark>
  __device__ __forceinline__ void advance(int64_t tile, int l, int kc, Issue&& issue, Mark&& mark) const {
    // Chunk s has landed (this wave's own pieces; vmcnt counts loads, stores and LDS-DMA together).  The stores
    // dripped at the start of the previous chunk have had a whole chunk to retire, so waiting for everything costs
    // nothing: counted waits that left them in flight measured 6.27 against 6.29 ms per 2^20-row pass.
#ifndef SIREN_EXPERIMENT_NO_DMA_WAIT  // timing experiment only (results are then wrong)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // ... for every wave (and the images are complete), and buffer (s + 1) & 1 is free
    mark();
    const bool more_k = kc + 1 < S::chunks;
    const bool more_l = STEP > 0 ? l < n_mm : l > 1;
    const int nl = more_k ? l : (more_l ? l + STEP : first_layer());
    if (more_k || more_l || tile + gridDim.x < tiles) issue(nl, more_k ? kc + 1 : 0, (s + 1) & 1);
    __builtin_amdgcn_sched_barrier(0);
  }
  template <class Issue>
  __device__ __forceinline__ void advance(int64_t tile, int l, int kc, Issue&& issue) const {
    advance(tile, l, kc, issue, [] {});
  }
};

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
// Chunk kc of a layer on the image whose fragment row is `a_row`, against the weight chunk at `wb`: every chunk but
// the last reads the next one's fragment (the caller splits the first, behind the stream's barrier).
template <class S>
__device__ __forceinline__ void mma_step(f32x16 (&acc)[S::NT], x3::Frag& fa, const float* a_row, int kc, const char* wb,
                                         const int (&boff)[S::NT]) {
  mma_chunk<S::NT, S::H>(acc, fa, kc + 1 < S::chunks ? a_row + (kc + 1) * kKc : nullptr, wb, boff);
}
// The pair form: acc0[t] += img W0^T and acc1[t] += img W1^T over one 16-deep chunk, the two weight chunks at wb0 / wb1
// (the same layout, so one boff serves both).  The image fragment `fa` is read and split ONCE and feeds both products;
// the next chunk's fragment is requested with the weight fragments and split behind the MFMAs, as in mma_chunk.
template <int NT, int H>
__device__ __forceinline__ void mma_chunk_pair(f32x16 (&acc0)[NT], f32x16 (&acc1)[NT], x3::Frag& fa,
                                               const float* __restrict__ a_next, const char* __restrict__ wb0,
                                               const char* __restrict__ wb1, const int (&boff)[NT]) {
  x3::Frag fb0[NT], fb1[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    fb0[t].h = *reinterpret_cast<const x3::u32x4*>(wb0 + boff[t]);
    fb0[t].m = *reinterpret_cast<const x3::u32x4*>(wb0 + H * 32 + boff[t]);
    fb0[t].l = *reinterpret_cast<const x3::u32x4*>(wb0 + 2 * H * 32 + boff[t]);
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    fb1[t].h = *reinterpret_cast<const x3::u32x4*>(wb1 + boff[t]);
    fb1[t].m = *reinterpret_cast<const x3::u32x4*>(wb1 + H * 32 + boff[t]);
    fb1[t].l = *reinterpret_cast<const x3::u32x4*>(wb1 + 2 * H * 32 + boff[t]);
  }
  float4 n_lo = {0.f, 0.f, 0.f, 0.f}, n_hi = n_lo;
  if (a_next) n_lo = *reinterpret_cast<const float4*>(a_next), n_hi = *reinterpret_cast<const float4*>(a_next + 8);
#pragma unroll
  for (int t = 0; t < NT; ++t) acc0[t] = mma6_32(fa, fb0[t], acc0[t]);
#pragma unroll
  for (int t = 0; t < NT; ++t) acc1[t] = mma6_32(fa, fb1[t], acc1[t]);
  if (a_next) fa = split_octets(n_lo, n_hi);
}
template <class S>
__device__ __forceinline__ void mma_step_pair(f32x16 (&acc0)[S::NT], f32x16 (&acc1)[S::NT], x3::Frag& fa,
                                              const float* a_row, int kc, const char* wb0, const char* wb1,
                                              const int (&boff)[S::NT]) {
  mma_chunk_pair<S::NT, S::H>(acc0, acc1, fa, kc + 1 < S::chunks ? a_row + (kc + 1) * kKc : nullptr, wb0, wb1, boff);
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

// MFMA tile t of the wave's layer output, from registers in the accumulator layout into an image
template <class S>
__device__ __forceinline__ void store_acc(float (&img)[S::rows * S::ld], const Lanes<S>& ln, const float (&v)[16],
                                          int t = 0) {
#pragma unroll
  for (int r = 0; r < 16; ++r) img[ln.row(r) * S::ld + ln.n0 + t * 32] = v[r];
}

// Coordinates of `count` rows / points from `first` on into xs, STRIDE floats each: zeros for absent axes and
// beyond n.
template <int STRIDE>
__device__ __forceinline__ void stage_coords(float* xs, const float* x, int64_t first, int count,
                                             int64_t n, int dim_in, int tid) {
  for (int e = tid; e < count * STRIDE; e += kThreads) {
    const int row = e / STRIDE, d = e % STRIDE;
    xs[e] = (d < dim_in && first + row < n) ? x[(first + row) * dim_in + d] : 0.f;
  }
}

// a resident H-vector (a bias, the head's weights) into LDS
template <int H>
__device__ __forceinline__ void load_vector(float* dst, const float* src, int tid) {
  for (int e = tid; e < H; e += kThreads) dst[e] = src[e];
}

// The head: an image row . w_head by one wave.  The lane's elements of w_head stay in registers.
template <class S>
struct HeadDot {
  static constexpr int kPer = S::H >= 64 ? S::H / 64 : 1;  // elements per lane (H = 32: half the lanes)
  float wv[kPer];
  const int lane;
  __device__ __forceinline__ HeadDot(const float* w_last, int lane_) : lane(lane_) {
#pragma unroll
    for (int j = 0; j < kPer; ++j) wv[j] = lane + 64 * j < S::H ? w_last[lane + 64 * j] : 0.f;
  }
  // the sum arrives in lane 0
  __device__ __forceinline__ float operator()(const float* img_row) const {
    float acc1 = 0.f;
#pragma unroll
    for (int j = 0; j < kPer; ++j)
      if (lane + 64 * j < S::H) acc1 += img_row[lane + 64 * j] * wv[j];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc1 += __shfl_down(acc1, off, 64);
    return acc1;
  }
};

}  // namespace chain

}  // namespace mri
