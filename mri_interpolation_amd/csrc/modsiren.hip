// Fused modulated-SIREN chain kernels for gfx950: TWO states of a row tile stay on chip across all layers.
//
// Replaces, for ModulatedSirenNet(dim_in <= 8 -> H x L -> 1) with H in {64, 128} (reference models.py:236-260
// Modulator.forward: Linear + ReLU on cat(hidden, z) per layer; :117-156 SirenLayer.forward; :263-322
// ModulatedSirenNet.forward: x = siren_layer(x) * mod per layer, then the linear head), the per-layer launches of the
// autograd path (two linear_act, a cat, a modulate and their backward: ~16 launches per layer, each an (n, H) round
// trip through HBM):
//
//   modsiren_forward_kernel   one persistent 512-thread workgroup per CU walks row tiles.  Two f32 images live in
//     LDS: a_l (the modulated activation) and h_l (the modulator's hidden state), beside the tile's z = x.  Layer 0
//     of both stacks (K = dim_in) runs on the VALU.  Every later layer is two H x H products on the bf16 matrix pipe
//     with three-term operands (bf16x3.h, f32-accurate): a_{l-1} Ws_l^T and h_{l-1} Wm_l[:, :H]^T, both weight
//     matrices pre-split and streamed from L2 in 16-deep chunks by LDS-DMA (the LDS-image tile loop of
//     chain_tile.h, here with a Ws / Wm pair per chunk).  The dim_in tail columns of Wm_l, the biases, sincos, ReLU and the
//     product are register work in the epilogue.  Training writes four (n, H) tensors per layer, each once:
//     a_l, h_l, h_l (.) w_l cos(.) and s_l = sin(.).
//   modsiren_backward_kernel  the same walk from the head down with the images dzs_l / dzm_l (see there).
//   H x H weight gradients    siren_wgrad_kernel and its fixed-order slab sum, once per (dzs_l, a_{l-1}) and once per
//     (dzm_l, h_{l-1}); the latter lands in the first H columns of the (H, H + dim_in) matrix.
//
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

// Geometry: a wave owns a 32 x 32 tile of BOTH layer outputs (one MFMA tile per product), the 8 waves are RB row
// blocks x CB column blocks.  Half the rows of siren_chain.hip's Shape<H>, so that two images take the ~66 KiB one
// takes there: 64 rows at H = 128, 128 rows at H = 64.
template <int HH>
struct MShape : TileShape<HH, 32> {
  using T = TileShape<HH, 32>;
  static constexpr int rpt = T::rows / T::groups;  // rows per thread of the (column, row group) phases: 16
  static_assert(HH == 64 || HH == 128, "hidden width");
};

struct ModArgs {
  const float* x;  // (n, dim_in)
  int64_t n;
  int dim_in, L;
  const float* ws[kMaxSine + 1];  // SIREN stack: [0] (H, dim_in); [1 .. L-1] (H, H); [L] the head (1, H)
  const float* bs[kMaxSine + 1];
  const float* wm[kMaxSine];      // modulator: [0] (H, dim_in); [l] (H, H + dim_in), hidden columns first
  const float* bm[kMaxSine];
  float w0_first, w0;
  float* act[kMaxSine];   // training: a_l = s_l (.) h_l
  float* hid[kMaxSine];   //           h_l = relu(pm_l)
  float* dcos[kMaxSine];  //           h_l (.) w_l cos(w_l ps_l)
  float* sn[kMaxSine];    //           s_l = sin(w_l ps_l)
  float* y;               // (n)
  const float* target;    // loss mode
  float grad_scale, inv_n;
  float* dy_out;          // (n): dLoss / dy
  float* partial;         // [gridDim.x]: loss partial sums
  const char* wsplit;     // per layer l = 1 .. L-1: split Ws_l | split Wm_l[:, :H] (split_matrix_bytes each)
};

template <class S>
struct MFwdSmem {
  char wbuf[2][2][S::chunk_bytes] __attribute__((aligned(16)));  // [buffer][matrix: Ws, Wm]
  float img_a[S::rows * S::ld];
  float img_h[S::rows * S::ld];
  float xs[S::rows * kMaxIn];
  float bias_s[kMaxSine][S::H];
  float bias_m[kMaxSine][S::H];
  float w_last[S::H];
  float tgt[S::rows];
  float red[8];
};

__device__ __forceinline__ float relu_f(float v) { return v > 0.f ? v : 0.f; }

// Inference (a.act[0] null: only y is written) or training (the four per-layer tensors leave for HBM): a wave-uniform
// run-time flag -- a separate inference instantiation allocated 256 registers and spilled, this one 176 --; LOSS:
// training with the loss: also dLoss/dy per row and this workgroup's share of mean((y - target)^2).
template <bool LOSS, class S>
__global__ __launch_bounds__(kThreads) void modsiren_forward_kernel(const ModArgs a) {
  __shared__ MFwdSmem<S> sm;
  constexpr int H = S::H;
  const bool STORE = a.act[0] != nullptr;
  const Lanes<S> ln;
  const int tid = ln.tid, n0 = ln.n0;  // n0: this lane's output column
  const int L = a.L, n_mm = L - 1;
  const int dim_in = a.dim_in;

  for (int l = 0; l < L; ++l) load_vector<H>(sm.bias_s[l], a.bs[l], tid), load_vector<H>(sm.bias_m[l], a.bm[l], tid);
  load_vector<H>(sm.w_last, a.ws[L], tid);
  const float b_last = a.bs[L][0];

  const int64_t tiles = (a.n + S::rows - 1) / S::rows;
  const float* a_row = sm.img_a + ln.fragment_offset();
  const float* h_row = sm.img_h + ln.fragment_offset();
  int boff[1];
  ln.weight_offsets(boff);
  const int lane_off = ln.global_offset();
  const int64_t smb = split_matrix_bytes(H);

  ChunkStream<S, 1> stream(n_mm, tiles);
  auto issue2 = [&](int layer, int kc, int buf) {  // both matrices of layer `layer` (1 .. L-1), chunk kc
    const char* base = a.wsplit + (int64_t)(2 * (layer - 1)) * smb;
    issue_chunk<S>(base, kc, sm.wbuf[buf][0], ln.wave, ln.lane);
    issue_chunk<S>(base + smb, kc, sm.wbuf[buf][1], ln.wave, ln.lane);
  };
  stream.prime(issue2);
  float g_loss = 0.f;

  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t m0 = tile * S::rows;
    const bool full_tile = m0 + S::rows <= a.n;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // previous tile is done with the images / xs / tgt
    stage_coords<kMaxIn>(sm.xs, a.x, m0, S::rows, a.n, dim_in, tid);
    if (LOSS && tid < S::rows) sm.tgt[tid] = m0 + tid < a.n ? a.target[m0 + tid] : 0.f;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // ---- layer 0 of both stacks on the VALU: thread <-> (column, group of rows) ---------------------------------
    {
      const int col = tid % H, r0 = (tid / H) * S::rpt;
      float wsr[kMaxIn], wmr[kMaxIn];
#pragma unroll
      for (int d = 0; d < kMaxIn; ++d) {
        wsr[d] = d < dim_in ? a.ws[0][col * dim_in + d] : 0.f;
        wmr[d] = d < dim_in ? a.wm[0][col * dim_in + d] : 0.f;
      }
      const float bsj = sm.bias_s[0][col], bmj = sm.bias_m[0][col];
      const float w0f = a.w0_first;
#pragma unroll 1
      for (int r = 0; r < S::rpt; r += 2) {
        float zs0 = 0.f, zs1 = 0.f, zm0 = 0.f, zm1 = 0.f;
#pragma unroll
        for (int d = 0; d < kMaxIn; ++d) {
          const float x0 = sm.xs[(r0 + r) * kMaxIn + d], x1 = sm.xs[(r0 + r + 1) * kMaxIn + d];
          zs0 += x0 * wsr[d], zs1 += x1 * wsr[d];
          zm0 += x0 * wmr[d], zm1 += x1 * wmr[d];
        }
        float s0, c0, s1, c1;
        sincos_fast2(w0f * (zs0 + bsj), w0f * (zs1 + bsj), &s0, &c0, &s1, &c1);
        const float h0 = relu_f(zm0 + bmj), h1 = relu_f(zm1 + bmj);
        sm.img_a[(r0 + r) * S::ld + col] = s0 * h0;
        sm.img_a[(r0 + r + 1) * S::ld + col] = s1 * h1;
        sm.img_h[(r0 + r) * S::ld + col] = h0;
        sm.img_h[(r0 + r + 1) * S::ld + col] = h1;
        __builtin_amdgcn_sched_barrier(0);
        if (STORE) {
          const int64_t row = m0 + r0 + r;
          if (row < a.n) {
            a.act[0][row * H + col] = s0 * h0, a.hid[0][row * H + col] = h0;
            a.dcos[0][row * H + col] = h0 * (w0f * c0), a.sn[0][row * H + col] = s0;
          }
          if (row + 1 < a.n) {
            a.act[0][(row + 1) * H + col] = s1 * h1, a.hid[0][(row + 1) * H + col] = h1;
            a.dcos[0][(row + 1) * H + col] = h1 * (w0f * c1), a.sn[0][(row + 1) * H + col] = s1;
          }
        }
      }
    }
    // ---- H x H layers: two products per layer -----------------------------------------------------------------------
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
      // ---- epilogue: the z tail of the modulator, biases, sincos, ReLU, product ----------------------------------------
      float wt[kMaxIn];
#pragma unroll
      for (int d = 0; d < kMaxIn; ++d) wt[d] = d < dim_in ? a.wm[l][n0 * (H + dim_in) + H + d] : 0.f;
      const float bsj = sm.bias_s[l][n0], bmj = sm.bias_m[l][n0];
      const float w0 = a.w0;
      float pa[16], ph[16];
      // (training: the four tensors leave straight from the registers they are computed in)
      float* __restrict__ ga = STORE ? a.act[l] + m0 * H : nullptr;
      float* __restrict__ gh = STORE ? a.hid[l] + m0 * H : nullptr;
      float* __restrict__ gd = STORE ? a.dcos[l] + m0 * H : nullptr;
      float* __restrict__ gs = STORE ? a.sn[l] + m0 * H : nullptr;
      int off = lane_off;
      asm volatile("" : "+v"(off));
      const int64_t rows_left = ln.rows_left(a.n - m0);
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        const int row = ln.row(r);
        const float4 xa0 = *reinterpret_cast<const float4*>(sm.xs + row * kMaxIn);
        const float4 xb0 = *reinterpret_cast<const float4*>(sm.xs + row * kMaxIn + 4);
        const float4 xa1 = *reinterpret_cast<const float4*>(sm.xs + (row + 1) * kMaxIn);
        const float4 xb1 = *reinterpret_cast<const float4*>(sm.xs + (row + 1) * kMaxIn + 4);
        float t0 = xa0.x * wt[0], t1 = xa1.x * wt[0];
        t0 += xa0.y * wt[1], t1 += xa1.y * wt[1];
        t0 += xa0.z * wt[2], t1 += xa1.z * wt[2];
        t0 += xa0.w * wt[3], t1 += xa1.w * wt[3];
        t0 += xb0.x * wt[4], t1 += xb1.x * wt[4];
        t0 += xb0.y * wt[5], t1 += xb1.y * wt[5];
        t0 += xb0.z * wt[6], t1 += xb1.z * wt[6];
        t0 += xb0.w * wt[7], t1 += xb1.w * wt[7];
        const float h0 = relu_f((acc_m[0][r] + t0) + bmj), h1 = relu_f((acc_m[0][r + 1] + t1) + bmj);
        float s0, c0, s1, c1;
        sincos_fast2(w0 * (acc_s[0][r] + bsj), w0 * (acc_s[0][r + 1] + bsj), &s0, &c0, &s1, &c1);
        pa[r] = s0 * h0, pa[r + 1] = s1 * h1;
        ph[r] = h0, ph[r + 1] = h1;
        if ((r & 3) == 2) __builtin_amdgcn_sched_barrier(0);  // (else every z read of the epilogue is hoisted to its top: spills)
        if (STORE) {
          const int dr = acc_row(r, 0);
          if (full_tile || dr < rows_left) {
            ga[off + dr * H] = pa[r], gh[off + dr * H] = h0;
            gd[off + dr * H] = h0 * (w0 * c0), gs[off + dr * H] = s0;
          }
          if (full_tile || dr + 1 < rows_left) {
            ga[off + (dr + 1) * H] = pa[r + 1], gh[off + (dr + 1) * H] = h1;
            gd[off + (dr + 1) * H] = h1 * (w0 * c1), gs[off + (dr + 1) * H] = s1;
          }
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();  // every wave has read both images for the last time
      store_acc<S>(sm.img_a, ln, pa);
      store_acc<S>(sm.img_h, ln, ph);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // image a complete
    // ---- head: y[row] = a_{L-1}[row] . w_head + b_head, one wave per row --------------------------------------------
    {
      const HeadDot<S> head(sm.w_last, ln.lane);
#pragma unroll 4
      for (int i = 0; i < S::rows / 8; ++i) {
        const int row = ln.wave * (S::rows / 8) + i;
        const float acc1 = head(sm.img_a + row * S::ld);
        if (ln.lane == 0 && m0 + row < a.n) {
          const float yv = acc1 + b_last;
          a.y[m0 + row] = yv;
          if (LOSS) {  // models.py:64 F.mse_loss: mean((y - target)^2); dLoss/dy = 2 (y - t) / N
            const float diff = yv - sm.tgt[row];
            g_loss += diff * diff;
            a.dy_out[m0 + row] = diff * a.grad_scale;
          }
        }
      }
    }
  }
  if (LOSS) {
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

// ------------------------------------------------------------------------------------------------------------------
// Backward chain.  Per tile, from the head down, with da_l and g_l = dzm_{l+1} Wm_{l+1}[:, :H] in accumulator registers:
//   dzs_l = da_l (.) [h_l w_l cos]          dzm_l = (da_l (.) s_l + g_l) (.) [h_l > 0]     (ReLU'(0) = 0, as torch)
// both become LDS images (the A operands of the next two products) and, for l >= 1, leave for HBM once for the H x H
// weight gradients.  From the images the VALU takes every small-K gradient: the bias column sums, the dim_in tail
// columns of dWm_l, dWs_0 and dWm_0; element (layer, column, d) has ONE owner thread in the workgroup, which adds its
// tile sums to the workgroup's slab in global memory (plain read-add-write in program order; the first tile
// overwrites).  Then da_{l-1} = dzs_l Ws_l and g_{l-1} = dzm_l Wm_l[:, :H] on the MFMAs against the transposed splits.
struct ModBwdArgs {
  const float* x;
  const float* dy;  // (n)
  int64_t n;
  int dim_in, L;
  const float* w_head;           // (1, H)
  const float* act_last;         // a_{L-1}
  const float* hid[kMaxSine];
  const float* dcos[kMaxSine];
  const float* sn[kMaxSine];
  float* dzs[kMaxSine];          // (n, H) for l >= 1 ([0] unused)
  float* dzm[kMaxSine];
  float* partial;                // [gridDim.x][ModBwdSlab]
  const char* wtsplit;           // per layer l = 1 .. L-1: split Ws_l^T | split Wm_l[:, :H]^T
};

template <class S>
struct MBwdSmem {
  char wbuf[2][2][S::chunk_bytes] __attribute__((aligned(16)));
  float img_s[S::rows * S::ld];
  float img_m[S::rows * S::ld];
  float xs[S::rows * kMaxIn];
  float w_last[S::H];
  float dy[S::rows];
};

template <class S>
__global__ __launch_bounds__(kThreads) void modsiren_backward_kernel(const ModBwdArgs a) {
  __shared__ MBwdSmem<S> sm;
  constexpr int H = S::H;
  // EXCEPTION to the toolkit (chain_tile.h): this kernel keeps its own copies of the lane coordinates, the coordinate
  // staging, the w_head load, the image write-back and the stream's advance (its order is ChunkStream::advance's, STEP
  // = -1).  On the helpers it measured 1.60 against 1.44 ms (H = 64) and 2.90 against 2.84 ms (H = 128) per 262144-row
  // call, six layers; with these copies it runs at the old speed.  A change to the stream order or to acc_row's
  // callers has to be made here as well.
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, lh = lane >> 5;
  const int rb = wave / S::CB, cb = wave % S::CB;
  const int n0 = cb * 32 + l31;
  const int L = a.L, dim_in = a.dim_in;
  for (int e = tid; e < H; e += kThreads) sm.w_last[e] = a.w_head[e];

  const int64_t tiles = (a.n + S::rows - 1) / S::rows;
  const float* s_row = sm.img_s + (rb * 32 + l31) * S::ld + 4 * lh;
  const float* m_row = sm.img_m + (rb * 32 + l31) * S::ld + 4 * lh;
  const int boff[1] = {weight_slot_offset(n0, lh)};
  const int lane_off = (rb * 32 + 4 * lh) * H + n0;
  const int64_t smb = split_matrix_bytes(H);

  const ModBwdSlab lay{H, L};
  float* const slab = a.partial + (int64_t)blockIdx.x * lay.floats();
  float* const p_wm = lay.wm(slab, 0);
  float* const p_ws0 = lay.ws0(slab);
  float* const p_bm = lay.bm(slab, 0);
  float* const p_bs = lay.bs(slab, 0);
  float* const p_wh = lay.w_head(slab);
  float* const p_bh = lay.b_head(slab);

  ChunkStream<S, -1> stream(L - 1, tiles);
  auto issue2 = [&](int layer, int kc, int buf) {
    const char* base = a.wtsplit + (int64_t)(2 * (layer - 1)) * smb;
    issue_chunk<S>(base, kc, sm.wbuf[buf][0], wave, lane);
    issue_chunk<S>(base + smb, kc, sm.wbuf[buf][1], wave, lane);
  };
  stream.prime(issue2);

  // a saved (n, H) tensor in the accumulator layout (zeros beyond n)
  auto load_acc = [&](const float* __restrict__ src, int64_t m0, bool tile_full, float (&v)[16]) {
    const float* __restrict__ g = src + m0 * H;
    int off = lane_off;
    asm volatile("" : "+v"(off));
    const int64_t rows_left = a.n - m0 - rb * 32 - 4 * lh;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int dr = acc_row(r, 0);
      v[r] = (tile_full || dr < rows_left) ? g[off + dr * H] : 0.f;
    }
  };

  // dW_head: (lane's column, its rows).  db_head (tid < rows) = sum of dLoss/dy, signed terms that cancel almost
  // entirely once the head bias has converged: summed in float64, one addition per thread and tile
  float g_wh = 0.f;
  double g_bh = 0.0;

  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t m0 = tile * S::rows;
    const bool full_tile = m0 + S::rows <= a.n;
    const bool first_tile = tile == (int64_t)blockIdx.x;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // previous tile is done with the images / xs / dy
    for (int e = tid; e < S::rows * kMaxIn; e += kThreads) {
      const int row = e / kMaxIn, d = e % kMaxIn;
      sm.xs[e] = (d < dim_in && m0 + row < a.n) ? a.x[(m0 + row) * dim_in + d] : 0.f;
    }
    if (tid < S::rows) {
      const float v = m0 + tid < a.n ? a.dy[m0 + tid] : 0.f;
      sm.dy[tid] = v;
      g_bh += (double)v;
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // ---- head: da_{L-1} = dy w_head; dW_head += dy^T a_{L-1} ---------------------------------------------------------
    float da[16], gm[16];
    {
      float av[16];
      load_acc(a.act_last, m0, full_tile, av);
      const float wl = sm.w_last[n0];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float dyv = sm.dy[rb * 32 + acc_row(r, lh)];
        g_wh += dyv * av[r];
        da[r] = dyv * wl;
        gm[r] = 0.f;
      }
    }
    for (int l = L - 1; l >= 0; --l) {
      // ---- dzs_l, dzm_l ------------------------------------------------------------------------------------------------
      float zs[16], zm[16];
      {
        float dv[16], sv[16], hv[16];
        load_acc(a.dcos[l], m0, full_tile, dv);
        load_acc(a.sn[l], m0, full_tile, sv);
        load_acc(a.hid[l], m0, full_tile, hv);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          zs[r] = da[r] * dv[r];
          zm[r] = hv[r] > 0.f ? da[r] * sv[r] + gm[r] : 0.f;
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();  // every wave has read both images for the last time
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        sm.img_s[(rb * 32 + acc_row(r, lh)) * S::ld + n0] = zs[r];
        sm.img_m[(rb * 32 + acc_row(r, lh)) * S::ld + n0] = zm[r];
      }
      if (l >= 1) {  // the H x H weight gradients read them
        float* __restrict__ gs = a.dzs[l] + m0 * H;
        float* __restrict__ gz = a.dzm[l] + m0 * H;
        int off = lane_off;
        asm volatile("" : "+v"(off));
        const int64_t rows_left = a.n - m0 - rb * 32 - 4 * lh;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int dr = acc_row(r, 0);
          if (full_tile || dr < rows_left) gs[off + dr * H] = zs[r], gz[off + dr * H] = zm[r];
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();  // both images complete
      // ---- small-K gradients on the VALU: (column, d) owners --------------------------------------------------------------
      for (int p = tid; p < H * kMaxIn; p += kThreads) {
        const int col = p % H, d = p / H;  // d is wave-uniform (H >= 64)
        if (d < dim_in) {
          float sum_m = 0.f, sum_s = 0.f;
          if (l == 0) {
#pragma unroll 8
            for (int row = 0; row < S::rows; ++row) {
              const float xv = sm.xs[row * kMaxIn + d];
              sum_m += sm.img_m[row * S::ld + col] * xv;
              sum_s += sm.img_s[row * S::ld + col] * xv;
            }
            float* q = p_ws0 + col * kMaxIn + d;
            *q = first_tile ? sum_s : *q + sum_s;
          } else {
#pragma unroll 8
            for (int row = 0; row < S::rows; ++row) sum_m += sm.img_m[row * S::ld + col] * sm.xs[row * kMaxIn + d];
          }
          float* q = p_wm + (l * H + col) * kMaxIn + d;
          *q = first_tile ? sum_m : *q + sum_m;
        }
        if (d == 0) {  // bias gradients: column sums
          float bm = 0.f, bs = 0.f;
#pragma unroll 8
          for (int row = 0; row < S::rows; ++row) bm += sm.img_m[row * S::ld + col], bs += sm.img_s[row * S::ld + col];
          float* qm = p_bm + l * H + col;
          float* qs = p_bs + l * H + col;
          *qm = first_tile ? bm : *qm + bm;
          *qs = first_tile ? bs : *qs + bs;
        }
      }
      if (l == 0) break;
      // ---- da_{l-1} = dzs_l Ws_l, g_{l-1} = dzm_l Wm_l[:, :H] -------------------------------------------------------------
      f32x16 acc_s[1], acc_m[1];
#pragma unroll
      for (int r = 0; r < 16; ++r) acc_s[0][r] = 0.f, acc_m[0][r] = 0.f;
      x3::Frag fs, fm;
#pragma unroll
      for (int kc = 0; kc < S::chunks; ++kc, stream.consumed()) {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();  // chunk s landed for every wave; the other buffer is free
        {
          const bool more_k = kc + 1 < S::chunks;
          const int nl = more_k ? l : (l > 1 ? l - 1 : L - 1);
          if (more_k || l > 1 || tile + gridDim.x < tiles) issue2(nl, more_k ? kc + 1 : 0, (stream.s + 1) & 1);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (kc == 0) fs = first_fragment(s_row), fm = first_fragment(m_row);
        mma_chunk<1, H>(acc_s, fs, kc + 1 < S::chunks ? s_row + (kc + 1) * kKc : nullptr, sm.wbuf[stream.s & 1][0], boff);
        mma_chunk<1, H>(acc_m, fm, kc + 1 < S::chunks ? m_row + (kc + 1) * kKc : nullptr, sm.wbuf[stream.s & 1][1], boff);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) da[r] = acc_s[0][r], gm[r] = acc_m[0][r];
    }
  }

  // ---- head gradients of this workgroup ------------------------------------------------------------------------------
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();
  float* red = sm.img_s;  // scratch: [row block][H], then [rows]
  g_wh += __shfl_xor(g_wh, 32, 64);  // the lane halves hold different rows of one column
  if (lh == 0) red[rb * H + n0] = g_wh;
  __syncthreads();
  if (tid < H) {
    float sum = 0.f;
#pragma unroll
    for (int q = 0; q < S::RB; ++q) sum += red[q * H + tid];
    p_wh[tid] = sum;
  }
  __syncthreads();
  double* red64 = reinterpret_cast<double*>(sm.img_m);
  if (tid < S::rows) red64[tid] = g_bh;
  __syncthreads();
  if (tid == 0) {
    double sb = 0.0;
    for (int c = 0; c < S::rows; ++c) sb += red64[c];
    p_bh[0] = (float)sb, p_bh[1] = 0.f, p_bh[2] = 0.f, p_bh[3] = 0.f;
  }
}

// ------------------------------------------------------------------------------------------------------ host side
int check_mod_shape(int dim_in, int hidden, int n_layers, int dim_out) {
  MRI_REQUIRE((hidden == 64 || hidden == 128) && dim_in >= 1 && dim_in <= kMaxIn && n_layers >= 2 &&
                  n_layers <= kMaxSine && dim_out == 1,
              "fused modulated SIREN: %d -> %d x %d -> %d is not supported (hidden 64 / 128, 1 <= dim_in <= 8, "
              "2 <= n_layers <= %d, dim_out 1)", dim_in, hidden, n_layers, dim_out, kMaxSine);
  return MRI_OK;
}
bool mod_supported(int dim_in, int hidden, int n_layers, int dim_out) {
  return check_mod_shape(dim_in, hidden, n_layers, dim_out) == MRI_OK;
}

int mod_tile_rows(int hidden) { return hidden == 128 ? 64 : 128; }
int mod_blocks(int hidden, int64_t n) { return persistent_blocks(n, mod_tile_rows(hidden)); }
int64_t mod_split_bytes(int hidden, int L) { return 2 * (int64_t)(L - 1) * split_matrix_bytes(hidden); }
int64_t mod_slab_bytes(int64_t n, int hidden, int L) {
  const int64_t chain = std::max<int64_t>((int64_t)mod_blocks(hidden, n) * ModBwdSlab{hidden, L}.floats(), 256);
  const int64_t bytes = std::max(chain, wgrad_slab_floats(n, hidden)) * 4;
  return (bytes + 255) / 256 * 256;
}

int mod_split(const float* const* ws, const float* const* wm, int dim_in, int hidden, int L, bool transposed,
              char* out, hipStream_t st) {
  const int64_t smb = split_matrix_bytes(hidden);
  if (int rc = split_weights_ld(ws + 1, L - 1, hidden, hidden, transposed, out, 2 * smb, st)) return rc;
  return split_weights_ld(wm + 1, L - 1, hidden, hidden + dim_in, transposed, out + smb, 2 * smb, st);
}

int launch_mod_forward(int hidden, const ModArgs& a, int mode, hipStream_t st) {
  const dim3 grid(mod_blocks(hidden, a.n)), block(kThreads);
  return dispatch_hidden_mod(hidden, [&](auto h) {
    using S = MShape<decltype(h)::value>;
    if (mode == 2) hipLaunchKernelGGL((modsiren_forward_kernel<true, S>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((modsiren_forward_kernel<false, S>), grid, block, 0, st, a);
    return check_launch("modsiren_forward_kernel");
  });
}

// the four saved (n, hidden) tensors per layer (the backward's weight-gradient kernels stream act / hid in 16-byte pieces:
// one contract for the four, in the forward too)
int check_saved(const void* act, const void* hid, const void* dcos, const void* sn, int L) {
  return check_pointers({{"act", act}, {"hid", hid}, {"dcos", dcos}, {"sn", sn}}, 0, L, 16);
}

// the checks and the argument block the three forward entry points share
int fill_forward(ModArgs& a, const float* x, int64_t n, int dim_in, int hidden, int L, const float* const* sw,
                 const float* const* sb, const float* const* mw, const float* const* mb, float w0_first, float w0,
                 float* const* act, float* const* hid, float* const* dcos, float* const* sn, float* y, bool train) {
  MRI_CHECK(check_buffers({{"x", x}, {"siren_weight", sw}, {"siren_bias", sb}, {"mod_weight", mw}, {"mod_bias", mb},
                           {"y", y}}, kAnyAlignment));
  a.x = x, a.n = n, a.dim_in = dim_in, a.L = L, a.w0_first = w0_first, a.w0 = w0, a.y = y;
  MRI_CHECK(check_pointers({{"siren_weight", sw}, {"siren_bias", sb}}, 0, L + 1, kAnyAlignment));
  MRI_CHECK(check_pointers({{"mod_weight", mw}, {"mod_bias", mb}}, 0, L, kAnyAlignment));
  for (int l = 0; l <= L; ++l) a.ws[l] = sw[l], a.bs[l] = sb[l];
  for (int l = 0; l < L; ++l) a.wm[l] = mw[l], a.bm[l] = mb[l];
  if (!train) return MRI_OK;
  MRI_CHECK(check_saved(act, hid, dcos, sn, L));
  for (int l = 0; l < L; ++l) a.act[l] = act[l], a.hid[l] = hid[l], a.dcos[l] = dcos[l], a.sn[l] = sn[l];
  return MRI_OK;
}

}  // namespace
}  // namespace mri

using namespace mri;

extern "C" int mri_modsiren_supported(int32_t dim_in, int32_t hidden, int32_t n_layers, int32_t dim_out) {
  return mod_supported(dim_in, hidden, n_layers, dim_out) ? 1 : 0;
}

extern "C" int64_t mri_modsiren_forward_workspace_bytes(int32_t hidden, int32_t n_layers) {
  if (!mod_supported(1, hidden, n_layers, 1)) return -1;
  return mod_split_bytes(hidden, n_layers);
}

extern "C" int64_t mri_modsiren_backward_workspace_bytes(int64_t n, int32_t hidden, int32_t n_layers) {
  if (n < 1 || n >= (1ll << 31) || !mod_supported(1, hidden, n_layers, 1)) return -1;
  return mod_slab_bytes(n, hidden, n_layers) + mod_split_bytes(hidden, n_layers);
}

extern "C" int mri_modsiren_forward(const float* x, int64_t n, int32_t dim_in, int32_t hidden, int32_t n_layers,
                                    const float* const* siren_weight, const float* const* siren_bias,
                                    const float* const* mod_weight, const float* const* mod_bias, float w0_first,
                                    float w0, float* const* act, float* const* hid, float* const* dcos,
                                    float* const* sn, float* y, void* workspace, int64_t workspace_bytes,
                                    void* stream) {
  MRI_CHECK(check_mod_shape(dim_in, hidden, n_layers, 1));
  MRI_CHECK(check_rows(n));
  if (n == 0) return MRI_OK;
  const bool train = act || hid || dcos || sn;
  MRI_CHECK(check_workspace("modulated SIREN forward", "mri_modsiren_forward_workspace_bytes", workspace,
                            workspace_bytes, mod_split_bytes(hidden, n_layers)));
  ModArgs a{};
  if (int rc = fill_forward(a, x, n, dim_in, hidden, n_layers, siren_weight, siren_bias, mod_weight, mod_bias,
                            w0_first, w0, act, hid, dcos, sn, y, train))
    return rc;
  a.wsplit = static_cast<const char*>(workspace);
  hipStream_t st = (hipStream_t)stream;
  if (int rc = mod_split(siren_weight, mod_weight, dim_in, hidden, n_layers, false, static_cast<char*>(workspace), st))
    return rc;
  return launch_mod_forward(hidden, a, train ? 1 : 0, st);
}

extern "C" int mri_modsiren_forward_loss(const float* x, const float* target, int64_t n, int64_t n_total,
                                         int32_t dim_in, int32_t hidden, int32_t n_layers,
                                         const float* const* siren_weight, const float* const* siren_bias,
                                         const float* const* mod_weight, const float* const* mod_bias,
                                         float w0_first, float w0, float grad_divisor, float* const* act,
                                         float* const* hid, float* const* dcos, float* const* sn, float* y, float* dy,
                                         float* loss_out, void* workspace, int64_t workspace_bytes, void* stream) {
  MRI_CHECK(check_mod_shape(dim_in, hidden, n_layers, 1));
  MRI_CHECK(check_batch_slice(n, n_total, grad_divisor));
  if (n == 0) return MRI_OK;
  MRI_CHECK(check_buffers({{"target", target}, {"dy", dy}, {"loss_out", loss_out}}, kAnyAlignment));
  MRI_CHECK(check_workspace("modulated SIREN forward with loss", "mri_modsiren_backward_workspace_bytes", workspace,
                            workspace_bytes, mri_modsiren_backward_workspace_bytes(n, hidden, n_layers)));
  ModArgs a{};
  if (int rc = fill_forward(a, x, n, dim_in, hidden, n_layers, siren_weight, siren_bias, mod_weight, mod_bias,
                            w0_first, w0, act, hid, dcos, sn, y, true))
    return rc;
  char* const wsplit = static_cast<char*>(workspace) + mod_slab_bytes(n, hidden, n_layers);
  a.wsplit = wsplit, a.target = target, a.dy_out = dy, a.partial = static_cast<float*>(workspace);
  a.grad_scale = (float)(2.0 / ((double)n_total * (double)grad_divisor));
  a.inv_n = (float)(1.0 / (double)n_total);
  hipStream_t st = (hipStream_t)stream;
  if (int rc = mod_split(siren_weight, mod_weight, dim_in, hidden, n_layers, false, wsplit, st)) return rc;
  if (int rc = launch_mod_forward(hidden, a, 2, st)) return rc;
  SegmentTable<1> t{};  // slabs of one float: the workgroups' loss shares, added in workgroup order
  t.vector(0, 1, loss_out);
  return reduce_slabs<1>(a.partial, mod_blocks(hidden, n), 1, t, st);
}

extern "C" int mri_modsiren_backward(const float* x, const float* dy, int64_t n, int32_t dim_in, int32_t hidden,
                                     int32_t n_layers, const float* const* siren_weight,
                                     const float* const* mod_weight, const float* const* act,
                                     const float* const* hid, const float* const* dcos, const float* const* sn,
                                     float* const* dzs, float* const* dzm, float* const* d_siren_weight,
                                     float* const* d_siren_bias, float* const* d_mod_weight,
                                     float* const* d_mod_bias, void* workspace, int64_t workspace_bytes,
                                     void* stream) {
  MRI_CHECK(check_mod_shape(dim_in, hidden, n_layers, 1));
  MRI_CHECK(check_rows(n));
  if (n == 0) return MRI_OK;
  const int L = n_layers;
  MRI_CHECK(check_buffers({{"x", x}, {"dy", dy}, {"siren_weight", siren_weight}, {"mod_weight", mod_weight},
                           {"act", act}, {"hid", hid}, {"dcos", dcos}, {"sn", sn}, {"dzs", dzs}, {"dzm", dzm},
                           {"d_siren_weight", d_siren_weight}, {"d_siren_bias", d_siren_bias},
                           {"d_mod_weight", d_mod_weight}, {"d_mod_bias", d_mod_bias}}, kAnyAlignment));
  MRI_CHECK(check_workspace("modulated SIREN backward", "mri_modsiren_backward_workspace_bytes", workspace,
                            workspace_bytes, mri_modsiren_backward_workspace_bytes(n, hidden, L)));
  MRI_CHECK(check_pointers({{"siren_weight", siren_weight}, {"d_siren_weight", d_siren_weight},
                            {"d_siren_bias", d_siren_bias}}, 0, L + 1, kAnyAlignment));
  MRI_CHECK(check_pointers({{"mod_weight", mod_weight}, {"d_mod_weight", d_mod_weight}, {"d_mod_bias", d_mod_bias}}, 0,
                           L, kAnyAlignment));
  MRI_CHECK(check_saved(act, hid, dcos, sn, L));
  MRI_CHECK(check_pointers({{"dzs", dzs}, {"dzm", dzm}}, 1, L - 1, 16));
  ModBwdArgs a{};
  a.x = x, a.dy = dy, a.n = n, a.dim_in = dim_in, a.L = L;
  for (int l = 0; l < L; ++l)
    a.hid[l] = hid[l], a.dcos[l] = dcos[l], a.sn[l] = sn[l], a.dzs[l] = dzs[l], a.dzm[l] = dzm[l];
  a.w_head = siren_weight[L], a.act_last = act[L - 1];
  a.partial = static_cast<float*>(workspace);
  char* const wtsplit = static_cast<char*>(workspace) + mod_slab_bytes(n, hidden, L);
  a.wtsplit = wtsplit;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = mod_split(siren_weight, mod_weight, dim_in, hidden, L, true, wtsplit, st)) return rc;
  const int blocks = mod_blocks(hidden, n);
  if (int rc = dispatch_hidden_mod(hidden, [&](auto h) {
        hipLaunchKernelGGL((modsiren_backward_kernel<MShape<decltype(h)::value>>), dim3(blocks), dim3(kThreads), 0, st, a);
        return check_launch("modsiren_backward_kernel");
      }))
    return rc;
  const ModBwdSlab lay{hidden, L};
  if (int rc = reduce_slabs<1>(a.partial, blocks, lay.floats(),
                               segments(lay, dim_in, d_siren_weight, d_siren_bias, d_mod_weight, d_mod_bias), st))
    return rc;
  for (int l = L - 1; l >= 1; --l) {  // dWs_l = dzs_l^T a_{l-1};  dWm_l[:, :H] = dzm_l^T h_{l-1}
    WgradArgs g{};
    g.n = n, g.partial = static_cast<float*>(workspace);
    g.dz = dzs[l], g.act = act[l - 1];
    if (int rc = wgrad_any_ld(hidden, g, d_siren_weight[l], hidden, st)) return rc;
    g.dz = dzm[l], g.act = hid[l - 1];
    if (int rc = wgrad_any_ld(hidden, g, d_mod_weight[l], hidden + dim_in, st)) return rc;
  }
  return MRI_OK;
}
