// Gradient slabs.  Every fused training kernel ends by writing its workgroup's partial parameter gradients (and its
// share of the loss) into one "slab" of the caller's workspace; a second launch adds the slabs in a FIXED order into
// the gradient tensors.  No float atomics: the training path is bitwise reproducible.  This header is the one place
// that says what a slab looks like (a layout struct per kernel family), where its elements go (the segment table)
// and in which order slabs are added (the two column sums).  DESIGN.md, "Gradient slabs".
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"

namespace mri {

constexpr int kMaxSine = MRI_SIREN_MAX_LAYERS;  // sine layers of a chain, the first one included
constexpr int kMaxIn = 8;                       // coordinates of a chain; its small-K slab rows are padded to this

// ---- layouts -----------------------------------------------------------------------------------------------------------
// A field accessor takes a base and steps from it to the field, in slab order: a pointer to the slab gives the field's
// pointer (the producers), 0 gives its offset in floats (the segment tables, floats()).  Pointer steps, not a summed
// offset: the producers compile to the instructions of the hand-written `p_b1 = p_w1 + H * k_in` chains they replace,
// all but shallow_mlp_kernel (scalar address arithmetic in its epilogue) and modsiren_backward_kernel (one scalar shift
// moved in its prologue); DESIGN.md, "Gradient slabs", has both with their timings.
#define MRI_SLAB_FIELD template <class P> __host__ __device__ P

// tiny MLP (mlp_fused.hip, mlp_x3.hip): dW1 [H][k_in] | db1 [H] | dW2 [H][H] | db2 [H] | dW3 [H] | db3 [1] | loss [1]
struct MlpSlab {
  int H, k_in;
  static constexpr int kSegments = 7;
  MRI_SLAB_FIELD w1(P p) const { return p; }
  MRI_SLAB_FIELD b1(P p) const { return w1(p) + H * k_in; }
  MRI_SLAB_FIELD w2(P p) const { return b1(p) + H; }
  MRI_SLAB_FIELD b2(P p) const { return w2(p) + H * H; }
  MRI_SLAB_FIELD w3(P p) const { return b2(p) + H; }
  MRI_SLAB_FIELD b3(P p) const { return w3(p) + H; }
  MRI_SLAB_FIELD loss(P p) const { return b3(p) + 1; }
  __host__ __device__ int floats() const { return loss(0) + 1; }
};

// shallow decoder (mlp_shallow.hip): dW1 [H][k_in] | db1 [H] | dw2 [H] | db2 [1] | loss [1], the waves added in wave order
struct ShallowSlab {
  int H, k_in;
  static constexpr int kSegments = 5;
  MRI_SLAB_FIELD w1(P p) const { return p; }
  MRI_SLAB_FIELD b1(P p) const { return w1(p) + H * k_in; }
  MRI_SLAB_FIELD w2(P p) const { return b1(p) + H; }
  MRI_SLAB_FIELD b2(P p) const { return w2(p) + H; }
  MRI_SLAB_FIELD loss(P p) const { return b2(p) + 1; }
  __host__ __device__ int floats() const { return loss(0) + 1; }
};

// SIREN loss-mode forward (siren_chain.hip, siren_rows.hip): dW_head [H] | db_last [H] | db_head, loss (padded to 4)
struct SirenFwdSlab {
  int H;
  static constexpr int kSegments = 4;
  MRI_SLAB_FIELD w_head(P p) const { return p; }
  MRI_SLAB_FIELD b_last(P p) const { return w_head(p) + H; }
  MRI_SLAB_FIELD b_head(P p) const { return b_last(p) + H; }
  MRI_SLAB_FIELD loss(P p) const { return b_head(p) + 1; }
  __host__ __device__ int floats() const { return b_head(0) + 4; }
};

// SIREN backward (siren_chain.hip, siren_rows.hip):
// dW_head [H] | db_head [1] (padded to 4) | db_l [L][H] | dW_first [H][kMaxIn]
struct SirenBwdSlab {
  int H, L;
  static constexpr int kSegments = kMaxSine + 3;      // L <= kMaxSine
  MRI_SLAB_FIELD w_head(P p) const { return p; }
  MRI_SLAB_FIELD b_head(P p) const { return w_head(p) + H; }
  MRI_SLAB_FIELD b(P p, int l) const { return b_head(p) + 4 + l * H; }
  MRI_SLAB_FIELD w_first(P p) const { return b(p, L); }
  __host__ __device__ int floats() const { return w_first(0) + H * kMaxIn; }
};

// modulated backward (modsiren.hip):
// dWm small-K [L][H][kMaxIn] | dWs_0 [H][kMaxIn] | dbm [L][H] | dbs [L][H] | dW_head [H] | db_head (padded to 4)
struct ModBwdSlab {
  int H, L;
  static constexpr int kSegments = 3 * kMaxSine + 3;  // L <= kMaxSine
  MRI_SLAB_FIELD wm(P p, int l) const { return p + l * H * kMaxIn; }
  MRI_SLAB_FIELD ws0(P p) const { return wm(p, L); }
  MRI_SLAB_FIELD bm(P p, int l) const { return ws0(p) + H * kMaxIn + l * H; }
  MRI_SLAB_FIELD bs(P p, int l) const { return bm(p, L) + l * H; }
  MRI_SLAB_FIELD w_head(P p) const { return bs(p, L); }
  MRI_SLAB_FIELD b_head(P p) const { return w_head(p) + H; }
  __host__ __device__ int floats() const { return b_head(0) + 4; }
};

// RffNet backward (rff.hip), L Linears: dW_head [H] | db_head (padded to 4) | db_l [L-1][H], l = 0 .. L-2
struct RffBwdSlab {
  int H, L;
  static constexpr int kSegments = kMaxSine + 1;      // L <= kMaxSine
  MRI_SLAB_FIELD w_head(P p) const { return p; }
  MRI_SLAB_FIELD b_head(P p) const { return w_head(p) + H; }
  MRI_SLAB_FIELD b(P p, int l) const { return b_head(p) + 4 + l * H; }
  __host__ __device__ int floats() const { return b(0, L - 1); }
};
#undef MRI_SLAB_FIELD

// ---- the segment table: where element e of a summed slab goes ---------------------------------------------------------
// A destination: a row-major block of `cols` slab columns whose first `valid` columns go to dst, rows `stride` floats apart.
struct SlabDest {
  float* dst;
  int cols, valid, stride;
  // q: the element's index in the block
  __device__ void write(int q, float sum, int overwrite) const {
    float* p = dst + q;  // dense (every vector): no division
    if (stride != cols || valid != cols) {
      const int row = q / cols, col = q % cols;
      if (col >= valid) return;
      p = dst + (int64_t)row * stride + col;
    }
    *p = overwrite ? sum : *p + sum;
  }
};

// Segment i covers slab elements [begin, begin + len) and goes to to[i].  Elements no segment claims (padding, the
// columns d >= dim_in of a kMaxIn-wide row) are not written.  Passed by value as a kernel argument, so N is the family's
// own count (each layout's kSegments): a launch pays for the kernel arguments it carries and the begins it scans.
template <int N>
struct SegmentTable {
  int n = 0;
  int overwrite = 0;  // 0: dst += sum; 1: dst = sum
  // The begins and lengths lie together (every lane scans them: scalar loads); a lane reads only its own segment's
  // destination.
  int begin[N], len[N];
  SlabDest to[N];

  // segments are added in slab order (find() relies on ascending begins)
  void matrix(int at, int rows, int n_cols, int n_valid, float* dst, int stride) {
    begin[n] = at, len[n] = rows * n_cols, to[n] = SlabDest{dst, n_cols, n_valid, stride};
    ++n;
  }
  void vector(int at, int count, float* dst) { matrix(at, 1, count, count, dst, count); }

  // The segment of slab element e (the last one that begins at or before it) and e's index in it; q < 0 where no
  // segment claims e.  The kernel calls this BEFORE it sums and write() after: the destination is a lane-indexed load
  // from the kernel arguments, one round trip that so runs beside the slab loads.
  struct Hit {
    SlabDest to;
    int q;
  };
  __device__ Hit find(int e) const {
    int s = 0, b = begin[0], l = len[0];
#pragma unroll
    for (int i = 1; i < N; ++i)
      if (i < n && e >= begin[i]) s = i, b = begin[i], l = len[i];
    const int q = e - b;
    return Hit{to[s], q < l ? q : -1};
  }
  __device__ void write(const Hit& h, float sum) const {
    if (h.q >= 0) h.to.write(h.q, sum, overwrite);
  }
};

inline SegmentTable<MlpSlab::kSegments> segments(const MlpSlab& s, int overwrite, float* d_w1, float* d_b1, float* d_w2,
                                                 float* d_b2, float* d_w3, float* d_b3, float* loss) {
  SegmentTable<MlpSlab::kSegments> t{};
  t.overwrite = overwrite;
  t.vector(s.w1(0), s.H * s.k_in, d_w1), t.vector(s.b1(0), s.H, d_b1), t.vector(s.w2(0), s.H * s.H, d_w2);
  t.vector(s.b2(0), s.H, d_b2), t.vector(s.w3(0), s.H, d_w3), t.vector(s.b3(0), 1, d_b3), t.vector(s.loss(0), 1, loss);
  return t;
}

inline SegmentTable<ShallowSlab::kSegments> segments(const ShallowSlab& s, int overwrite, float* d_w1, float* d_b1,
                                                     float* d_w2, float* d_b2, float* loss) {
  SegmentTable<ShallowSlab::kSegments> t{};
  t.overwrite = overwrite;
  t.vector(s.w1(0), s.H * s.k_in, d_w1), t.vector(s.b1(0), s.H, d_b1), t.vector(s.w2(0), s.H, d_w2);
  t.vector(s.b2(0), 1, d_b2), t.vector(s.loss(0), 1, loss);
  return t;
}

inline SegmentTable<SirenFwdSlab::kSegments> segments(const SirenFwdSlab& s, float* d_w_head, float* d_b_last,
                                                      float* d_b_head, float* loss) {
  SegmentTable<SirenFwdSlab::kSegments> t{};
  t.vector(s.w_head(0), s.H, d_w_head), t.vector(s.b_last(0), s.H, d_b_last);
  t.vector(s.b_head(0), 1, d_b_head), t.vector(s.loss(0), 1, loss);
  return t;
}

// d_w / d_b: [0] the first layer (H, dim_in), [1 .. L-1] the H x H layers (their dW: slab_sum_kernel), [L] the head
inline SegmentTable<SirenBwdSlab::kSegments> segments(const SirenBwdSlab& s, int dim_in, float* const* d_w,
                                                      float* const* d_b) {
  SegmentTable<SirenBwdSlab::kSegments> t{};
  t.vector(s.w_head(0), s.H, d_w[s.L]), t.vector(s.b_head(0), 1, d_b[s.L]);
  for (int l = 0; l < s.L; ++l) t.vector(s.b(0, l), s.H, d_b[l]);
  t.matrix(s.w_first(0), s.H, kMaxIn, dim_in, d_w[0], dim_in);
  return t;
}

// d_wm[0] is (H, dim_in); d_wm[l >= 1] is (H, H + dim_in) and takes its last dim_in columns here
inline SegmentTable<ModBwdSlab::kSegments> segments(const ModBwdSlab& s, int dim_in, float* const* d_ws,
                                                    float* const* d_bs, float* const* d_wm, float* const* d_bm) {
  SegmentTable<ModBwdSlab::kSegments> t{};
  t.matrix(s.wm(0, 0), s.H, kMaxIn, dim_in, d_wm[0], dim_in);
  for (int l = 1; l < s.L; ++l) t.matrix(s.wm(0, l), s.H, kMaxIn, dim_in, d_wm[l] + s.H, s.H + dim_in);
  t.matrix(s.ws0(0), s.H, kMaxIn, dim_in, d_ws[0], dim_in);
  for (int l = 0; l < s.L; ++l) t.vector(s.bm(0, l), s.H, d_bm[l]);
  for (int l = 0; l < s.L; ++l) t.vector(s.bs(0, l), s.H, d_bs[l]);
  t.vector(s.w_head(0), s.H, d_ws[s.L]), t.vector(s.b_head(0), 1, d_bs[s.L]);
  return t;
}

// d_w / d_b: the L Linears of an RffNet; [L-1] is the head (the dW of Linears 0 .. L-2: slab_sum_kernel)
inline SegmentTable<RffBwdSlab::kSegments> segments(const RffBwdSlab& s, float* const* d_w, float* const* d_b) {
  SegmentTable<RffBwdSlab::kSegments> t{};
  t.vector(s.w_head(0), s.H, d_w[s.L - 1]), t.vector(s.b_head(0), 1, d_b[s.L - 1]);
  for (int l = 0; l + 1 < s.L; ++l) t.vector(s.b(0, l), s.H, d_b[l]);
  return t;
}

// ---- the two orders -----------------------------------------------------------------------------------------------------
// (1) Chains.  G thread groups; group g adds its contiguous G-th of the slabs in slab order, one float32 chain, eight
// loads in flight (these kernels are bound by the latency of their dependent rounds of loads, not by bytes: a load per
// addition was 63 us of round trips); then the groups' sums are added in group order.  G = 1 is the plain chain.  An
// empty group (few slabs) contributes its 0.  `part`: G x E floats of LDS, E = elements per workgroup; lane = the
// element's index in the workgroup.  Every thread of the workgroup calls this; the sum is valid where grp == 0.
template <int G, int E>
__device__ __forceinline__ float chain_column_sum(const float* __restrict__ partial, int slabs, int slab, int e, int lane,
                                                  int grp, float (*part)[E]) {
  const int per = (slabs + G - 1) / G;
  const int b_lo = grp * per, b_hi = min(slabs, b_lo + per);
  float s = 0.f;
  if (e < slab) {
    const float* p = partial + e;
    int b = b_lo;
    for (; b + 8 <= b_hi; b += 8) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = p[(int64_t)(b + j) * slab];
#pragma unroll
      for (int j = 0; j < 8; ++j) s += v[j];
    }
    for (; b < b_hi; ++b) s += p[(int64_t)b * slab];
  }
  if (G == 1) return s;
  part[grp][lane] = s;
  __syncthreads();
  if (grp != 0) return 0.f;
  s = part[0][lane];
#pragma unroll
  for (int g = 1; g < G; ++g) s += part[g][lane];
  return s;
}

// G = 1: 256 elements per workgroup; G > 1: 64 elements x G groups.  G = 4 for the tiny MLP (<= 512 slabs), 16 for the
// shallow decoder (up to 512 slabs of few floats: without the groups the chain's rounds are all the kernel does), 1 for
// the chain kernels' <= 256 slabs.
template <int G>
struct SlabReduce {
  static constexpr int elements = G == 1 ? 256 : 64, threads = elements * G;
  static unsigned blocks(int slab) { return (unsigned)ceil_div(slab, elements); }
};

template <int G, int N>
__global__ __launch_bounds__(SlabReduce<G>::threads) void slab_reduce_kernel(const float* __restrict__ partial, int slabs,
                                                                             int slab, const SegmentTable<N> t) {
  constexpr int E = SlabReduce<G>::elements;
  __shared__ float part[G == 1 ? 1 : G][E];
  const int lane = threadIdx.x % E, grp = threadIdx.x / E, e = blockIdx.x * E + lane;
  const auto to = t.find(e);
  const float s = chain_column_sum<G, E>(partial, slabs, slab, e, lane, grp, part);
  if (grp == 0 && e < slab) t.write(to, s);
}

template <int G, int N>
int reduce_slabs(const float* partial, int slabs, int slab, const SegmentTable<N>& t, hipStream_t st) {
  hipLaunchKernelGGL((slab_reduce_kernel<G, N>), dim3(SlabReduce<G>::blocks(slab)), dim3(SlabReduce<G>::threads), 0, st,
                     partial, slabs, slab, t);
  return check_launch("slab_reduce_kernel");
}

// (2) Trees in float64, for the H x H weight-gradient slabs (siren_wgrad_kernel).  There are 256 x wgrad_split slabs
// (2048 at H = 32, 512 at H = 64) of signed terms, and one float32 chain that long moved an H x H gradient by up to
// 3.7e-6 of its largest element when the same rows were cut into two launches (tests/test_gpu_tile_loop.py).  So eight
// slabs meet in a float32 tree (three roundings deep) and the trees' sums are added in float64.  A thread waits for a
// round of loads before it issues the next, and what it computes behind the last load of a round is exposed: sixteen
// loads a round, so that the longer tail comes half as often.
__device__ __forceinline__ float sum8(const float* v) {
  return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
}

__device__ __forceinline__ float tree_column_sum(const float* __restrict__ p, int slabs, int slab) {
  double sum = 0.0;
  int b = 0;
  for (; b + 16 <= slabs; b += 16) {
    float v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = p[(int64_t)(b + j) * slab];
    sum += (double)sum8(v) + (double)sum8(v + 8);
  }
  for (; b + 8 <= slabs; b += 8) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = p[(int64_t)(b + j) * slab];
    sum += (double)sum8(v);
  }
  for (; b < slabs; ++b) sum += (double)p[(int64_t)b * slab];
  return (float)sum;
}

}  // namespace mri
