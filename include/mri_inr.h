/*
 * mri_inr.h -- C ABI of the MI355X (gfx950) hot path for Benjamin-Fouquet/mri_interpolation.
 *
 * The reference is pure Python: its hot path sits behind Python class surfaces, not an FFI
 * (SURVEY.md section 8b).  Each entry point below names the reference op chain it replaces
 * (file:line into the reference repository); the Python classes in mri_interpolation_amd/ bind
 * these with ctypes (see INTEGRATION.md for the stub a reference maintainer would add).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (a torch tensor's data_ptr())
 *     unless the parameter is documented as host memory; the library never allocates,
 *     frees or retains memory;
 *   - `stream` is a hipStream_t passed as void*; calls only enqueue work on it and never
 *     synchronise; the library keeps no global state besides the last-error string;
 *   - all matrices are float32, row-major, with an explicit leading dimension in elements;
 *   - alignment: every float pointer is 4-byte aligned.  An entry point either takes ANY such pointer and any
 *     leading dimension (it picks 16-byte accesses where pointer, leading dimension and row count allow them and
 *     4-byte accesses elsewhere: same values), or names the arguments that must be 16-byte aligned and refuses
 *     others with MRI_ERR_INVALID_ARGUMENT before anything is queued.  Where nothing is said, any 4-byte aligned
 *     pointer is served (tests/test_gpu_layout.py);
 *   - return value 0 = success, negative = mri_status; mri_last_error() returns a
 *     thread-local message for the last failure.  No C++ exception crosses this boundary.
 */
#ifndef MRI_INR_H
#define MRI_INR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRI_MAX_LEVELS 32
#define MRI_MAX_DIM 7 /* len(PRIMES), reference encoding.py:40,90-92 */

typedef enum mri_status {
  MRI_OK = 0,
  MRI_ERR_INVALID_ARGUMENT = -1,
  MRI_ERR_UNSUPPORTED = -2,
  MRI_ERR_LAUNCH = -3
} mri_status;

typedef enum mri_activation {
  MRI_ACT_IDENTITY = 0,
  MRI_ACT_RELU = 1, /* nn.ReLU,  reference models.py:31,54 */
  MRI_ACT_SINE = 2, /* sin(w0*z), reference models.py:108-114 */
  MRI_ACT_GELU = 3  /* nn.GELU (erf form), reference models.py:672,736 */
} mri_activation;

/* How mri_linear_backward_data turns dL/d(activation output) into dL/d(pre-activation). */
typedef enum mri_deriv_mode {
  MRI_DERIV_NONE = 0,     /* no multiply (identity / network input)                     */
  MRI_DERIV_MUL = 1,      /* multiply by a stored derivative matrix (sine, gelu)        */
  MRI_DERIV_RELU_MASK = 2 /* multiply by (stored activation output > 0)                 */
} mri_deriv_mode;

/* Host-side description of a multiresolution hash grid (HOST memory, copied by value).
 * Mirrors what MultiResHashGrid / MultiResHashGridV2 compute in __init__
 * (reference encoding.py:168-185, 310-330): one resolution per level and axis, one table
 * size per level, tables concatenated in one flat (sum T_l, F) float32 array. */
typedef struct mri_grid_desc {
  int32_t dim;        /* D, 1..MRI_MAX_DIM                                   */
  int32_t n_levels;   /* L, 1..MRI_MAX_LEVELS                                */
  int32_t n_features; /* F, one of 1, 2, 4, 8 (others are refused)           */
  int32_t reserved;
  float resolution[MRI_MAX_LEVELS][MRI_MAX_DIM + 1]; /* res_l on axis d (float32, as the
                                                        reference multiplies in float32)  */
  uint32_t table_size[MRI_MAX_LEVELS];               /* T_l, any value >= 1 (not only 2^k) */
  uint64_t table_offset[MRI_MAX_LEVELS];             /* first row of level l in the flat table */
} mri_grid_desc;

/* Library / build identification: "mri_inr <version> gfx950". */
const char* mri_version(void);
const char* mri_last_error(void);
/* Tuning knobs, process-wide, read when a call plans its launches.  Defaults in parentheses.
 * Speed-only knobs whose results are BITWISE those of the default (tests/test_gpu_knobs.py):
 *   "xcd_affinity" 0/1 (1): block -> level map of the hash-grid forward (and of the global-atomic
 *   backward, whose f32 atomics add in no fixed order whatever the map);
 *   table-gradient knobs of the binned path (methods 0 / 2, every contribution is one f32 product turned
 *   into fixed point and the sums are int64, so how the work is cut changes no bit):
 *   "bwd_dense_max_parts" n (4): levels of at most n table slices skip the records (dense path);
 *   "bwd_fuse_dense" 0/1 (1): the dense levels share the launch of the record accumulation;
 *   "bwd_dense_blocks" n >= 1 (96), "bwd_blocks_per_level" n >= 1 (64): workgroups of the dense levels /
 *   per binned level (values below 1 are stored as 1);
 *   "mlp_stagger" 0..8 (0): segments team 1 of the 128-wide f32-MFMA decoder runs behind team 0
 *   (other values are rejected).
 * Speed-only knobs that keep results within fp32 summation-order noise:
 *   "fwd_pair" 0/1 (1): F = 2 forward, two lanes per (coordinate, level) with the partial sums added last,
 *   or one lane adding the corners in order;
 *   "bwd_lds_max_parts" n (256): under method 0, levels of more than n slices take global f32 atomics;
 *   "mlp_x3" 0/1/2 (1): which kernel serves the decoder -- 1 the bf16-pipe kernel with exact three-term
 *   operands, 2 its four-wave form (128-wide), 0 the f32-MFMA kernels;
 *   "siren_rows" 0/1 (1): SirenNet of width 256 -- 1 the chain kernels that keep a wave's rows in
 *   registers across the layers (csrc/siren_rows.hip), 0 the LDS-image kernels of every other width.
 * 0/1 knobs store any nonzero value as 1.  The workspace size and the plan of the table-gradient backward
 * depend on the knobs: they must not change between mri_hashgrid_backward_workspace_bytes /
 * mri_hashgrid_backward_prepare and the backward calls that use that workspace, nor during the life of a
 * fused training step (its count-ahead stage prepares the next step's backward).
 * ONE option trades accuracy, for grids with two features per level: "bwd_records" 0 (default) / 1,
 * the gradient records of mri_hashgrid_backward* (see there).  0: every contribution w * g is the f32
 * product the reference's autograd forms, their sum per table entry is exact.  1: each contribution is
 * rounded to 18-21 significant bits (8-byte packed records) before the exact sum -- 13 us faster per
 * step at BASELINE config 4 and NOT f32-equivalent (per table entry 17x the median error of the f32
 * records against float64, tests/test_gpu_round3.py).  Other values are rejected.
 * Both calls return MRI_ERR_INVALID_ARGUMENT for an unknown name. */
int mri_set_option(const char* name, int32_t value);
/* The current value of a knob (HOST pointer), as mri_set_option stored it. */
int mri_get_option(const char* name, int32_t* value);

/* ---- hash-grid encoding --------------------------------------------------------------
 * Replaces, per level, the op chain of _HashGrid.forward / _HashGridV2.forward
 * (reference encoding.py:108-128, 232-270) incl. fast_hash (encoding.py:69-78), and the
 * torch.cat over levels (encoding.py:190-191, 335-336).
 *   x    (n, D) row-major coordinates.
 *   table  (sum T_l, F); with F = 2 or 4 it must be 16-byte aligned, else refused: F = 2 rows are read 8 bytes at
 *        a time ("fwd_pair" 0: two neighbouring rows with one 16-byte load where the level starts at an even
 *        row), F = 4 rows 16 bytes at a time.
 *   out  element (row i, level l, feature f) is written to
 *        out[l * out_level_stride + i * out_row_stride + f * out_feat_stride].
 *        Reference layout (n, L*F): level stride F, row stride L*F, feature stride 1.
 *        Feature-major layout (L*F, n) used inside the fused trainer (coalesced stores,
 *        read back by mri_linear_forward with x_row_stride 1): level stride F*n, row
 *        stride 1, feature stride n.  Any 4-byte aligned pointer and any strides.
 */
int mri_hashgrid_forward(const mri_grid_desc* grid, const float* x, int64_t n,
                         const float* table, float* out, int64_t out_level_stride,
                         int64_t out_row_stride, int64_t out_feat_stride, void* stream);

/* Replaces the autograd of the same chain: aten::embedding_dense_backward per level plus
 * the mul/sum backward (reference encoding.py:127-128).
 * d_table (sum T_l, F) is ACCUMULATED into (caller zeroes it).  d_out uses the same
 * three-stride addressing as `out` above.
 *   method 0 = choose per level; 1 = global float atomics; 2 = LDS owner-computes scan with
 *   64-bit fixed-point accumulation (bitwise reproducible gradients).
 *   Accuracy of methods 0 / 2 (the binned path): the contributions of a table entry are added as
 *   integers in units of 2^-e, e chosen per level so that n * max|d_out| * 2^e < 2^61: the sum is exact
 *   but for what lies below that unit -- a contribution smaller than 2^-40 of the level's max |d_out|
 *   (n = 2^18; 2^-(58 - log2 n) in general) is truncated toward zero, so an entry whose only
 *   contributions are that small reads 0 where the reference holds a denormal-scale value.  With
 *   mri_set_option("bwd_records", 1) each contribution is first rounded to 18-21 significant bits and
 *   the cut-off is 2^-45 of the level's maximum (2^(E-45), E the exponent of max |d_out|).
 *   workspace: device scratch of at least mri_hashgrid_backward_workspace_bytes(grid, n)
 *   bytes, 16-byte aligned; no initialisation needed (the call clears what it needs), it
 *   may be shared by calls with different grids / n on the same stream.  May be NULL for
 *   method 1.  x, d_out (any strides) and d_table: any 4-byte aligned pointer.
 */
int64_t mri_hashgrid_backward_workspace_bytes(const mri_grid_desc* grid, int64_t n);
/* Optional split: the first stage of the binned backward (counting the records per table
 * slice) needs only the coordinates, so a trainer can run it on a side stream beside the
 * forward pass and then call mri_hashgrid_backward with `method | MRI_BWD_PREPARED` on the same
 * workspace (same grid, n and method; nothing else may use the workspace in between).  The two calls may be told
 * different workspace_bytes for that pointer, each at least the reported size: where a region lies depends on the
 * grid, n, the method and the knobs alone, never on the surplus (tests/test_gpu_workspace.py). */
#define MRI_BWD_PREPARED 16
/* `method | MRI_BWD_OVERWRITE`: d_table is OVERWRITTEN with the gradient (every row of every
 * level is written) instead of accumulated into, which saves the caller's memset and the
 * read half of the accumulation. */
#define MRI_BWD_OVERWRITE 32
int mri_hashgrid_backward_prepare(const mri_grid_desc* grid, const float* x, int64_t n,
                                  int32_t method, void* workspace, int64_t workspace_bytes,
                                  void* stream);
int mri_hashgrid_backward(const mri_grid_desc* grid, const float* x, const float* d_out,
                          int64_t n, int64_t dout_level_stride, int64_t dout_row_stride,
                          int64_t dout_feat_stride, float* d_table, int32_t method,
                          void* workspace, int64_t workspace_bytes, void* stream);
/* Same, for the levels whose bit is set in `level_mask` only (bit l = level l): the gradient of
 * one level group at a time, so that a data-parallel caller can start reducing a finished group
 * (all-reduce over RCCL) while the next one is computed.  With MRI_BWD_PREPARED one
 * mri_hashgrid_backward_prepare call on the workspace serves every group; without it each call
 * recounts all levels.  Rows of levels outside the mask are not touched. */
int mri_hashgrid_backward_levels(const mri_grid_desc* grid, const float* x, const float* d_out,
                                 int64_t n, int64_t dout_level_stride, int64_t dout_row_stride,
                                 int64_t dout_feat_stride, float* d_table, int32_t method,
                                 uint32_t level_mask, void* workspace, int64_t workspace_bytes,
                                 void* stream);
/* Table gradient AND the table's optimiser step in one pass (one rank, no gradient accumulation):
 * embedding_dense_backward x L followed by torch.optim.Adam.step on the embedding weights (reference
 * models.py:68-70 configure_optimizers, :61-66 training_step).  Where a gradient entry is complete
 * the Adam update of mri_adam_step (same operations, same order: bit-identical results) is applied
 * to table / exp_avg / exp_avg_sq in place; the gradient itself is never written (8 bytes of HBM
 * traffic per table parameter and step less, and the optimiser launch shrinks to the decoder).
 * `step` is the 1-based step number, `grad_scale` multiplies the gradient first.  method: 0 / 2
 * (+ MRI_BWD_PREPARED); returns MRI_ERR_UNSUPPORTED if a level of the grid would take the atomic
 * kernel (then call mri_hashgrid_backward + mri_adam_step). */
int mri_hashgrid_backward_adam(const mri_grid_desc* grid, const float* x, const float* d_out,
                               int64_t n, int64_t dout_level_stride, int64_t dout_row_stride,
                               int64_t dout_feat_stride, float* table, float* exp_avg,
                               float* exp_avg_sq, double lr, double beta1, double beta2, double eps,
                               int32_t step, float grad_scale, int32_t method, void* workspace,
                               int64_t workspace_bytes, void* stream);

/* ---- fully connected layers (f32 MFMA) ------------------------------------------------
 * y = act(w0 * (x W^T + b))   with W (N, K) row-major as nn.Linear / SirenLayer store it.
 * Replaces F.linear + activation: reference models.py:46-56 (BaseMLP.layers),
 * models.py:153-156 (SirenLayer.forward), models.py:730-736 (HashMLP decoder Linear+act).
 *   x element (m, k) at x[m*x_row_stride + k*x_col_stride]  (x_col_stride 1 = row-major,
 *     x_row_stride 1 = feature-major (K, M) as written by the level-major encoder output).
 *   deriv (optional, (M, ldd)) receives d act / d z  (w0*cos(w0 z) for sine, gelu'(z));
 *     pass NULL for identity / relu (relu's mask is recovered from y).
 *   w0 is only used by MRI_ACT_SINE.
 * The four linear entry points take any 4-byte aligned pointers and any strides / leading dimensions: operands
 * are read, and full output tiles written, 16 bytes at a time where pointer and stride allow it.
 */
int mri_linear_forward(const float* x, int64_t x_row_stride, int64_t x_col_stride,
                       const float* weight, const float* bias /* may be NULL */, int64_t m,
                       int32_t n, int32_t k, int32_t activation, float w0, float* y,
                       int64_t ldy, float* deriv /* may be NULL */, int64_t ldd, void* stream);

/* dx = (dy W) (.) g   where g is chosen by deriv_mode from `deriv` ((M, K), leading dim ldd):
 * the gradient w.r.t. the PREVIOUS layer's pre-activation (autograd of F.linear followed by
 * the previous activation's backward).  dx element (m, k) at dx[m*dx_row_stride + k*dx_col_stride]
 * (deriv_mode must be MRI_DERIV_NONE when dx_col_stride != 1).
 */
int mri_linear_backward_data(const float* dy, int64_t lddy, const float* weight, int64_t m,
                             int32_t n, int32_t k, int32_t deriv_mode, const float* deriv,
                             int64_t ldd, float* dx, int64_t dx_row_stride,
                             int64_t dx_col_stride, void* stream);

/* d_weight (N, K) += dy^T x ;  d_bias (N) += column sums of dy (d_bias may be NULL).
 * Accumulates with float atomics (caller zeroes the gradient buffers once per step).
 * x addressed with the same two strides as in mri_linear_forward. */
int mri_linear_backward_weight(const float* dy, int64_t lddy, const float* x,
                               int64_t x_row_stride, int64_t x_col_stride, int64_t m, int32_t n,
                               int32_t k, float* d_weight, float* d_bias, void* stream);

/* In-place dy *= g (same deriv modes as above) -- activation after the LAST Linear
 * (BaseMLP keeps one, reference models.py:54). */
int mri_apply_deriv(float* dy, int64_t lddy, int32_t deriv_mode, const float* deriv,
                    int64_t ldd, int64_t m, int32_t n, void* stream);

/* ---- frequency encoding ----------------------------------------------------------------------
 * `Frequency.forward` (reference encoding.py:43-66): for every row and input axis d,
 * out[d*2L + l] = sin(x_d * 2^l), out[d*2L + L + l] = cos(x_d * 2^l), l = 0..L-1.
 *   x (n, dim) row-major with leading dimension ldx; out (n, dim*2L) with leading dimension ldo.
 * mri_frequency_backward writes (does not accumulate) dx (n, dim) from d_out (n, dim*2L).
 * 4-byte accesses only: any pointers, any leading dimensions. */
int mri_frequency_forward(const float* x, int64_t ldx, int64_t n, int32_t dim, int32_t n_levels,
                          float* out, int64_t ldo, void* stream);
int mri_frequency_backward(const float* x, int64_t ldx, const float* d_out, int64_t ldg, int64_t n,
                           int32_t dim, int32_t n_levels, float* dx, int64_t lddx, void* stream);

/* ---- fused tiny MLP ------------------------------------------------------------------------
 * The decoder of BASELINE configs 2/4/5: k_in -> hidden -> hidden -> 1, ReLU on the hidden
 * layers, linear output (reference config/hash_config.json "network"; module form
 * models.py:46-56 / 730-744 with ReLU, no BatchNorm).  ONE persistent kernel per call:
 * activations never leave the CU; k_in <= 32: weights in registers, products on the bf16 matrix
 * pipe with every f32 operand split exactly into three bf16 terms (f32-accurate, csrc/bf16x3.h);
 * hidden 64 with 32 < k_in <= 64: weights resident in LDS, products on the f32 MFMA.
 *   x        (k_in, n) FEATURE-MAJOR input features (the layout mri_hashgrid_forward writes)
 *   w1 (hidden, k_in), w2 (hidden, hidden), w3 (1, hidden) row-major as nn.Linear stores them
 * mri_tiny_mlp_supported: 1 if (k_in, hidden, dim_out) has a fused kernel
 *   (hidden 128 with k_in <= 32, hidden 64 with k_in <= 64, dim_out 1), else 0.
 * mri_tiny_mlp_forward:  y[n] = MLP(x).
 * mri_tiny_mlp_train:    forward + F.mse_loss(target, y) + backward in one pass:
 *   d_w*, d_b* += parameter gradients, loss_out[0] += mean squared error,
 *   d_x (k_in, n) feature-major = dLoss/dx (optional, may be NULL), y (optional) predictions.
 *   Gradients are those of mean((y - target)^2) / grad_divisor.  Per-workgroup partial sums go
 *   through `workspace` (mri_tiny_mlp_workspace_bytes, no initialisation needed) and are added
 *   in a fixed order: results are bitwise reproducible.
 * Alignment: x / d_x / y / target and every parameter and gradient pointer may be any 4-byte aligned address (the
 *   f32-MFMA kernels read x 16 bytes at a time where its address and leading dimension allow it), except that
 *   the 128-wide f32-MFMA kernel (option "mlp_x3" = 0, and mri_tiny_mlp_train_overlapped) refuses a w2 that is
 *   not 16-byte aligned. */
int mri_tiny_mlp_supported(int32_t k_in, int32_t hidden, int32_t dim_out);
int64_t mri_tiny_mlp_workspace_bytes(int32_t k_in, int32_t hidden, int64_t n);
int mri_tiny_mlp_forward(const float* x, int64_t n, int32_t k_in, int32_t hidden, const float* w1,
                         const float* b1, const float* w2, const float* b2, const float* w3,
                         const float* b3, float* y, void* stream);
int mri_tiny_mlp_train(const float* x, const float* target, int64_t n, int32_t k_in,
                       int32_t hidden, const float* w1, const float* b1, const float* w2,
                       const float* b2, const float* w3, const float* b3, float grad_divisor,
                       float* d_w1, float* d_b1, float* d_w2, float* d_b2, float* d_w3,
                       float* d_b3, float* d_x /* may be NULL */, float* loss_out,
                       float* y /* may be NULL */, void* workspace, int64_t workspace_bytes,
                       void* stream);
/* Same, but d_w*, d_b* and loss_out are overwritten instead of accumulated into. */
int mri_tiny_mlp_train_overwrite(const float* x, const float* target, int64_t n, int32_t k_in,
                                 int32_t hidden, const float* w1, const float* b1,
                                 const float* w2, const float* b2, const float* w3,
                                 const float* b3, float grad_divisor, float* d_w1, float* d_b1,
                                 float* d_w2, float* d_b2, float* d_w3, float* d_b3, float* d_x,
                                 float* loss_out, float* y, void* workspace,
                                 int64_t workspace_bytes, void* stream);

/* The same step for a SLICE of a batch: columns [0, n) of feature-major blocks x / d_x whose feature
 * rows are x_ld elements apart (x_ld >= n), `n` targets, out of a batch of n_total coordinates --
 * the mean of the loss and the gradient scale are taken over n_total, so the slices of a batch
 * add up to the whole-batch call (first slice with overwrite = 1, the others with 0).  Lets a
 * caller run the encoder of slice k+1 beside the decoder of slice k. */
int mri_tiny_mlp_train_slice(const float* x, int64_t x_ld, const float* target, int64_t n,
                             int64_t n_total, int32_t k_in, int32_t hidden, const float* w1,
                             const float* b1, const float* w2, const float* b2, const float* w3,
                             const float* b3, float grad_divisor, float* d_w1, float* d_b1,
                             float* d_w2, float* d_b2, float* d_w3, float* d_b3, float* d_x,
                             float* loss_out, float* y, int32_t overwrite, void* workspace,
                             int64_t workspace_bytes, void* stream);

/* mri_tiny_mlp_train[_overwrite] that also reports max |d_x| per PAIR of feature rows: dx_pair_absmax
 * ((k_in + 1) / 2 non-negative floats: with an odd k_in the last row has an entry of its own) is raised with atomic
 * maxima, so the caller zeroes it before the call.
 * With a hash-grid encoder of two features per level this is max |dLoss / d features| per level, the scale
 * mri_hashgrid_backward_scaled needs for its gradient records -- taken where d_x is produced instead of by
 * a pass over it.  Served by the bf16-pipe decoder kernel only (mri_tiny_mlp_dx_absmax_supported, else
 * MRI_ERR_UNSUPPORTED); d_x must be requested. */
int mri_tiny_mlp_dx_absmax_supported(int32_t k_in, int32_t hidden);
int mri_tiny_mlp_train_dx_absmax(const float* x, const float* target, int64_t n, int32_t k_in,
                                 int32_t hidden, const float* w1, const float* b1, const float* w2,
                                 const float* b2, const float* w3, const float* b3, float grad_divisor,
                                 float* d_w1, float* d_b1, float* d_w2, float* d_b2, float* d_w3,
                                 float* d_b3, float* d_x, float* loss_out, float* y, int32_t overwrite,
                                 float* dx_pair_absmax, void* workspace, int64_t workspace_bytes,
                                 void* stream);

/* mri_hashgrid_backward_levels with max |d_out| per level supplied by the caller (level_absmax, n_levels
 * non-negative floats, each >= the true maximum's binade is what matters: values above it would clip;
 * NULL = found by a pass over d_out, as the other entry points do).  Grids with two features per level
 * store their gradient records relative to that scale (csrc/hashgrid_bwd.hip, packed records). */
int mri_hashgrid_backward_scaled(const mri_grid_desc* grid, const float* x, const float* d_out, int64_t n,
                                 int64_t dout_level_stride, int64_t dout_row_stride,
                                 int64_t dout_feat_stride, float* d_table, int32_t flags,
                                 uint32_t level_mask, const float* level_absmax, void* workspace,
                                 int64_t workspace_bytes, void* stream);

/* Encoder + decoder in ONE kernel (reference models.py:739-754, HashMLP.forward = encoder -> ReLU MLP,
 * with F.mse_loss and the decoder's autograd): the decoder's workgroups look the features of their
 * next row tile up themselves while the matrix pipe works on the current one, so the lookup kernel
 * and the feature block (2 x 4 L F bytes per coordinate) disappear.  Same arithmetic as
 * mri_hashgrid_forward followed by mri_tiny_mlp_train[_overwrite]: bit-identical loss, gradients and
 * d_enc.  Grids with n_features = 2, dim 2..4, <= 16 levels, < 2^29 table rows; hidden 64 or 128
 * (mri_hash_tiny_mlp_supported, else MRI_ERR_UNSUPPORTED).  coords (n, dim) row-major; d_enc
 * (2 L, d_enc_ld) feature-major = dLoss / d features, the input of mri_hashgrid_backward; workspace as
 * mri_tiny_mlp_workspace_bytes(2 L, hidden, n).  table must be 16-byte aligned (as for mri_hashgrid_forward). */
int mri_hash_tiny_mlp_supported(const mri_grid_desc* grid, int32_t hidden);
int mri_hash_tiny_mlp_train(const mri_grid_desc* grid, const float* table, const float* coords,
                            const float* target, int64_t n, int32_t hidden, const float* w1,
                            const float* b1, const float* w2, const float* b2, const float* w3,
                            const float* b3, float grad_divisor, float* d_w1, float* d_b1,
                            float* d_w2, float* d_b2, float* d_w3, float* d_b3, float* d_enc,
                            int64_t d_enc_ld, float* loss_out, float* y, int32_t overwrite,
                            void* workspace, int64_t workspace_bytes, void* stream);

/* ---- fused shallow decoder -------------------------------------------------------------------
 * The decoder of the notebook's HashMLP without BatchNorm (reference models.py:712-739 minus the
 * BatchNorm1d, notebook cell 37): k_in -> hidden -> 1 with an activation after EACH of the two Linears,
 *   y = act_out(act_hidden(x W1^T + b1) . w2 + b2),
 * in ONE persistent kernel per call: nothing (n, hidden)-sized goes to memory (csrc/mlp_shallow.hip; the
 * three matrix products are f32 MFMAs).
 *   1 <= k_in <= 32, hidden in {32, 64, 128}, dim_out 1, biases on both layers; act_hidden and act_out
 *   each one of MRI_ACT_IDENTITY / MRI_ACT_RELU / MRI_ACT_GELU (mri_shallow_mlp_supported: 1 or 0).
 *   x (k_in, n) FEATURE-MAJOR (the layout mri_hashgrid_forward writes), w1 (hidden, k_in), w2 (1, hidden)
 *   row-major as nn.Linear stores them, y (n).
 * mri_shallow_mlp_train: forward + F.mse_loss(target, y) + backward in one pass over a slice of n rows of a
 *   batch of n_total (n <= n_total; the mean of the loss and the gradient scale are taken over n_total, so
 *   the slices of a batch add up to the whole batch): gradients of mean((y - target)^2) / grad_divisor.
 *   overwrite = 0: d_w1, d_b1, d_w2, d_b2 and loss_out[0] are ADDED to, 1: overwritten.  d_x (k_in, n)
 *   feature-major = dLoss / dx is written (optional, may be NULL), y (optional) receives the predictions.
 *   Per-workgroup partial sums go through `workspace` (mri_shallow_mlp_workspace_bytes, -1 for an
 *   unsupported shape; no initialisation needed) and are added in a fixed order: bitwise reproducible.
 * n = 0 is a no-op; NULL buffers, an unsupported shape or a short workspace return
 * MRI_ERR_INVALID_ARGUMENT before anything is queued.  4-byte accesses to every caller buffer: any pointers. */
int mri_shallow_mlp_supported(int32_t k_in, int32_t hidden, int32_t dim_out, int32_t act_hidden,
                              int32_t act_out);
int64_t mri_shallow_mlp_workspace_bytes(int32_t k_in, int32_t hidden, int64_t n);
int mri_shallow_mlp_forward(const float* x, int64_t n, int32_t k_in, int32_t hidden, const float* w1,
                            const float* b1, const float* w2, const float* b2, int32_t act_hidden,
                            int32_t act_out, float* y, void* stream);
int mri_shallow_mlp_train(const float* x, const float* target, int64_t n, int64_t n_total, int32_t k_in,
                          int32_t hidden, const float* w1, const float* b1, const float* w2,
                          const float* b2, int32_t act_hidden, int32_t act_out, float grad_divisor,
                          float* d_w1, float* d_b1, float* d_w2, float* d_b2, float* d_x /* may be NULL */,
                          float* loss_out, float* y /* may be NULL */, int32_t overwrite, void* workspace,
                          int64_t workspace_bytes, void* stream);

/* Gradient w.r.t. the COORDINATES: the reference detaches only the integer part of x * res
 * (encoding.py:111-113), so autograd carries d out / d x through the interpolation weights:
 * d_x[i][d] = res_d * sum over levels and corners of (+-1) prod_{e != d} w_e * <d_out, row>.
 * Not on the training path (coordinates carry no gradient there); d_x is (n, D) row-major. */
int mri_hashgrid_backward_input(const mri_grid_desc* grid, const float* x, const float* d_out,
                                int64_t n, int64_t dout_level_stride, int64_t dout_row_stride,
                                int64_t dout_feat_stride, const float* table, float* d_x,
                                void* stream);

/* ---- lookup and decoder running side by side ----------------------------------------------
 * The decoder kernel is bound by the f32 matrix rate and leaves the texture path idle; the lookup
 * is bound by the texture path, needs no LDS and 27 registers.  Launched on two streams they share
 * the CUs: mri_hashgrid_forward_signal (queue it FIRST) produces the feature-major block
 * (L*2, out_ld) slice by slice -- a slice = slice_rows consecutive coordinates =
 * mri_tiny_mlp_round_rows(), what one round of the decoder's workgroups reads -- and adds
 * mri_hashgrid_forward_signal_blocks() to ready[slice] as its blocks finish (write-through stores,
 * agent-scope counter; the counters only ever grow: the caller keeps the running total and passes
 * it as ready_target).  mri_tiny_mlp_train_overlapped is mri_tiny_mlp_train[_overwrite] whose
 * workgroups wait for ready[r] >= ready_target before touching round r's rows (bounded wait: a
 * producer that never arrives sets *status = 1 instead of hanging the GPU).  Same results as the
 * two plain calls, bit for bit.  Needs n_features == 2, 2 <= dim <= 4, hidden == 128.
 * mri_hashgrid_forward_signal takes any slice_rows >= 1, any out pointer and any out_ld >= n (table as for
 * mri_hashgrid_forward): a slice is stored 16 bytes at a time where out is 16-byte aligned, out_ld % 4 == 0 and the
 * slice starts at a multiple of 4 rows (every slice when slice_rows % 4 == 0), 4 bytes at a time elsewhere. */
int64_t mri_hashgrid_forward_signal_blocks(const mri_grid_desc* grid, int64_t slice_rows);
int mri_hashgrid_forward_signal(const mri_grid_desc* grid, const float* x, int64_t n,
                                const float* table, float* out, int64_t out_ld,
                                int64_t slice_rows, uint64_t* ready, void* stream);
int64_t mri_tiny_mlp_round_rows(int32_t k_in, int32_t hidden, int64_t n);
int mri_tiny_mlp_train_overlapped(const float* x, const float* target, int64_t n, int32_t k_in,
                                  int32_t hidden, const float* w1, const float* b1,
                                  const float* w2, const float* b2, const float* w3,
                                  const float* b3, float grad_divisor, float* d_w1, float* d_b1,
                                  float* d_w2, float* d_b2, float* d_w3, float* d_b3, float* d_x,
                                  float* loss_out, int32_t overwrite, const uint64_t* ready,
                                  uint64_t ready_target, int32_t* status, void* workspace,
                                  int64_t workspace_bytes, void* stream);

/* ---- fused SIREN chain -------------------------------------------------------------------
 * SirenNet.forward (reference models.py:230-233): n_sine_layers x [F.linear -> sin(w0 .)]
 * (SirenLayer.forward, models.py:153-156; the first layer with w0_first) and the linear head,
 * in ONE persistent kernel: a row tile's activations stay on chip across all layers -- in the
 * registers of the wave that owns the rows at hidden = 256 (csrc/siren_rows.hip), in an LDS image
 * at the other widths (csrc/siren_chain.hip) --, the hidden x hidden weights stream from L2.
 * Supported: hidden in
 * {32, 64, 128, 256}, dim_in <= 8, 1 <= n_sine_layers <= MRI_SIREN_MAX_LAYERS, one output, biases everywhere
 * (mri_siren_supported); other shapes go layer by layer through mri_linear_*.
 * weight / bias: HOST arrays of n_sine_layers + 1 device pointers -- [0] (hidden, dim_in),
 * [1 .. n-1] (hidden, hidden), [n] the head (1, hidden); all row-major, 16-byte aligned.
 * act / deriv: HOST arrays of n_sine_layers device pointers to (n, hidden) row-major, 16-byte aligned buffers
 * that receive each sine layer's output and its derivative w0 cos(.) for the backward pass, or both
 * NULL (inference: nothing but y is written).  y: (n) predictions.
 * Alignment (the three SIREN calls): weight[l], act[l], deriv[l], dz[l], dz_last and workspace must be 16-byte
 * aligned, else MRI_ERR_INVALID_ARGUMENT names the argument; x, y, target, dy, the biases and every gradient
 * output are accessed 4 bytes at a time.
 * workspace: mri_siren_forward_workspace_bytes device bytes, 16-byte aligned (0 bytes / NULL with one
 * sine layer): each call first splits the hidden x hidden weights there into the three bf16 terms
 * the matrix pipe multiplies (f32-accurate, csrc/bf16x3.h), in the order the kernel streams them. */
#define MRI_SIREN_MAX_LAYERS 8
int mri_siren_supported(int32_t dim_in, int32_t hidden, int32_t n_sine_layers, int32_t dim_out);
int64_t mri_siren_forward_workspace_bytes(int32_t hidden, int32_t n_sine_layers);
int mri_siren_forward(const float* x, int64_t n, int32_t dim_in, int32_t hidden,
                      int32_t n_sine_layers, const float* const* weight,
                      const float* const* bias, float w0_first, float w0, float* const* act,
                      float* const* deriv, float* y, void* workspace, int64_t workspace_bytes,
                      void* stream);

/* Backward of the same network (autograd of models.py:230-233 + the loss gradient dy the caller
 * got from mri_mse_loss): dz walks the layers inside LDS (one persistent kernel), each hidden x hidden
 * weight gradient is one persistent kernel that keeps the whole result in MFMA
 * accumulators; partial sums meet in `workspace` and are added in a fixed order (bitwise
 * reproducible).  act / deriv: what mri_siren_forward stored; dz: HOST array of n_sine_layers
 * device pointers to (n, hidden) scratch ([0] unused, may be NULL); d_weight / d_bias: HOST arrays
 * of n_sine_layers + 1 device pointers, gradients are ADDED to them.  head_done = 1: the head's
 * backward was done by mri_siren_forward_loss (dy, act / deriv [n_sine_layers - 1] unused).
 * head_done = 1 continues THAT call: same n, same network, the SAME `workspace` bytes, untouched in
 * between, and the same "siren_rows" option -- at hidden = 256 the two calls share the work of the head
 * (what the forward call leaves in dz[n_sine_layers - 1] and in the workspace is private to the pair). */
int64_t mri_siren_backward_workspace_bytes(int64_t n, int32_t hidden, int32_t n_sine_layers);
int mri_siren_backward(const float* x, const float* dy, int64_t n, int32_t dim_in, int32_t hidden,
                       int32_t n_sine_layers, const float* const* weight,
                       const float* const* act, const float* const* deriv, float* const* dz,
                       float* const* d_weight, float* const* d_bias, int32_t head_done,
                       void* workspace, int64_t workspace_bytes, void* stream);
/* Training forward WITH the loss (models.py:61-66 training_step: y_pred = forward(x);
 * F.mse_loss(y, y_pred)): the kernel of mri_siren_forward also compares its predictions with
 * `target`, and runs the head's backward in the tile's tail, where the last sine layer's output
 * and derivative are still in registers (they are NOT written to act / deriv [n_sine_layers - 1],
 * which may be NULL): dz_last (n, hidden) = dLoss / d(pre-activation of the last sine layer), and,
 * ADDED to them, d_w_head (1, hidden), d_b_head (1), d_b_last (hidden), loss_out[0] += mean over
 * n_total (n <= n_total: a slice of a batch).  Gradients are scaled by 1 / grad_divisor.  Follow
 * with mri_siren_backward(..., head_done = 1, dy = NULL), which then starts from dz_last =
 * dz[n_sine_layers - 1].  Needs n_sine_layers >= 2; workspace: mri_siren_backward_workspace_bytes. */
int mri_siren_forward_loss(const float* x, const float* target, int64_t n, int64_t n_total,
                           int32_t dim_in, int32_t hidden, int32_t n_sine_layers,
                           const float* const* weight, const float* const* bias, float w0_first,
                           float w0, float grad_divisor, float* const* act, float* const* deriv,
                           float* dz_last, float* y, float* d_w_head, float* d_b_head,
                           float* d_b_last, float* loss_out, void* workspace,
                           int64_t workspace_bytes, void* stream);

/* Values AND the gradient with respect to the coordinates of the same network, y (n) and dydx (n, dim_in)
 * row-major, dydx[i, d] = d y[i] / d x[i, d], in ONE persistent kernel (csrc/siren_gradient.hip): forward mode --
 * the tangent of sine layer l is w_l cos(w_l z_l) (.) (tangent of layer l - 1) W_l^T, the value row's product on
 * more rows --, so a point travels as four consecutive rows of the LDS activation image (value, d/dx_0, d/dx_1,
 * d/dx_2) through the tile loop of mri_siren_forward's inference kernel; the hidden x hidden products run on the
 * same bf16x3 form.  dim_in = 4 takes the eight-row form of the same kernel (value, d/dx_0, d/dx_1, d/dx_2 | value,
 * d/dx_3, 0, 0: the value row twice, so that each half of a point meets its own w cos(.) in one lane).
 * Nothing (n, hidden)-sized is written: the call reads n dim_in floats and writes n (1 + dim_in).
 * No atomics, a fixed summation order: bitwise reproducible.  At most 256 workgroups walk the tiles of 1024 / hidden
 * points (64 at hidden 32); half as many points per tile with dim_in = 4.
 * Supported (mri_siren_gradient_supported is the truth): hidden in {32, 64, 128, 256}, 1 <= dim_in <= 4,
 * 1 <= n_sine_layers <= MRI_SIREN_MAX_LAYERS, dim_out = 1; anything else is refused with MRI_ERR_INVALID_ARGUMENT,
 * the offending argument named in mri_last_error.  n = 0 returns 0 without a launch.
 * weight / bias: as mri_siren_forward (weight[l] 16-byte aligned); x, y and dydx are accessed 4 bytes at a time at
 * any 4-byte aligned address.  workspace: mri_siren_gradient_workspace_bytes device bytes (what
 * mri_siren_forward_workspace_bytes reports: the split weights; -1 for an unsupported width or depth), 16-byte
 * aligned, 0 bytes / NULL with one sine layer. */
int mri_siren_gradient_supported(int32_t dim_in, int32_t hidden, int32_t n_sine_layers, int32_t dim_out);
int64_t mri_siren_gradient_workspace_bytes(int32_t hidden, int32_t n_sine_layers);
int mri_siren_gradient(const float* x, int64_t n, int32_t dim_in, int32_t hidden, int32_t n_sine_layers,
                       const float* const* weight, const float* const* bias, float w0_first, float w0, float* y,
                       float* dydx, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- fused modulated SIREN chain ---------------------------------------------------------------
 * ModulatedSirenNet.forward (reference models.py:263-322): per layer l the SIREN layer sin(w_l (a_{l-1} Ws_l^T +
 * bs_l)) (SirenLayer.forward, models.py:153-156; w_0 = w0_first) multiplied elementwise by the modulator's hidden
 * state h_l = relu([h_{l-1}, z] Wm_l^T + bm_l) (Modulator.forward, models.py:236-260; z = x, layer 0 sees z only),
 * then the linear head -- in ONE persistent kernel (csrc/modsiren.hip): both states of a row tile stay in LDS across
 * all layers, the hidden x hidden weights of both stacks stream from L2.
 * Supported (mri_modsiren_supported is the truth): 1 <= dim_in <= 8, hidden in {64, 128},
 * 2 <= n_layers <= MRI_SIREN_MAX_LAYERS, dim_out = 1, biases everywhere.  An unsupported shape is refused with
 * MRI_ERR_INVALID_ARGUMENT and its reason in mri_last_error.
 * siren_weight / siren_bias: HOST arrays of n_layers + 1 device pointers -- [0] (hidden, dim_in), [1 .. n-1]
 * (hidden, hidden), [n] the head (1, hidden).  mod_weight / mod_bias: HOST arrays of n_layers device pointers --
 * [0] (hidden, dim_in), [l] (hidden, hidden + dim_in), the hidden columns first (the reference concatenates
 * (hidden, z)).  All row-major and contiguous.
 * act / hid / dcos / sn: HOST arrays of n_layers device pointers to (n, hidden) row-major, 16-byte aligned buffers
 * (checked by all three calls, as dzs / dzm and the workspace are; every other pointer: any 4-byte aligned address)
 * that receive, per layer, a_l = s_l h_l, h_l, h_l w_l cos(.) and s_l = sin(.) for the backward pass -- or all four
 * NULL (inference: nothing but y is written).  y: (n) predictions.
 * workspace: mri_modsiren_forward_workspace_bytes device bytes, 16-byte aligned: each call first splits the hidden x
 * hidden blocks of both stacks there into the three bf16 terms the matrix pipe multiplies (f32-accurate,
 * csrc/bf16x3.h). */
int mri_modsiren_supported(int32_t dim_in, int32_t hidden, int32_t n_layers, int32_t dim_out);
int64_t mri_modsiren_forward_workspace_bytes(int32_t hidden, int32_t n_layers);
int mri_modsiren_forward(const float* x, int64_t n, int32_t dim_in, int32_t hidden, int32_t n_layers,
                         const float* const* siren_weight, const float* const* siren_bias,
                         const float* const* mod_weight, const float* const* mod_bias, float w0_first, float w0,
                         float* const* act, float* const* hid, float* const* dcos, float* const* sn, float* y,
                         void* workspace, int64_t workspace_bytes, void* stream);
/* Training forward WITH the loss (models.py:61-66 training_step: y_pred = forward(x); F.mse_loss(y, y_pred)): the
 * same kernel also compares its predictions with `target`: dy (n) = 2 (y - target) / (n_total grad_divisor), and
 * loss_out[0] += sum (y - target)^2 / n_total (n <= n_total: a slice of a batch), the workgroups' shares added in a
 * fixed order.  Follow with mri_modsiren_backward(dy).  workspace: mri_modsiren_backward_workspace_bytes. */
int mri_modsiren_forward_loss(const float* x, const float* target, int64_t n, int64_t n_total, int32_t dim_in,
                              int32_t hidden, int32_t n_layers, const float* const* siren_weight,
                              const float* const* siren_bias, const float* const* mod_weight,
                              const float* const* mod_bias, float w0_first, float w0, float grad_divisor,
                              float* const* act, float* const* hid, float* const* dcos, float* const* sn, float* y,
                              float* dy, float* loss_out, void* workspace, int64_t workspace_bytes, void* stream);
/* Backward of the same network (autograd of models.py:263-322 from dy = dLoss / dy): da and the modulator's dz walk
 * the layers inside LDS (one persistent kernel) and leave once per layer as dzs / dzm -- HOST arrays of n_layers
 * device pointers to (n, hidden) 16-byte aligned scratch ([0] unused, may be NULL) --; each hidden x hidden weight
 * gradient is one persistent kernel (the SIREN chain's).  Bias gradients, the head, the first layers and the dim_in
 * tail columns of the modulator weights are summed per workgroup; all partial sums meet in `workspace` and are added
 * in a fixed order: no float atomics, bitwise reproducible.  act / hid / dcos / sn: what the forward call stored.
 * d_siren_weight / d_siren_bias (n_layers + 1 pointers) and d_mod_weight / d_mod_bias (n_layers): gradients are
 * ADDED to them.  No gradient with respect to x. */
int64_t mri_modsiren_backward_workspace_bytes(int64_t n, int32_t hidden, int32_t n_layers);
int mri_modsiren_backward(const float* x, const float* dy, int64_t n, int32_t dim_in, int32_t hidden,
                          int32_t n_layers, const float* const* siren_weight, const float* const* mod_weight,
                          const float* const* act, const float* const* hid, const float* const* dcos,
                          const float* const* sn, float* const* dzs, float* const* dzm,
                          float* const* d_siren_weight, float* const* d_siren_bias, float* const* d_mod_weight,
                          float* const* d_mod_bias, void* workspace, int64_t workspace_bytes, void* stream);
/* Values AND the gradient with respect to the coordinates of the same network, y (n) and dydx (n, dim_in) row-major,
 * dydx[i, d] = d y[i] / d x[i, d], in ONE persistent kernel (csrc/modsiren_gradient.hip) instead of autograd through
 * Modulator.forward (reference models.py:236-260) and the layer loop of ModulatedSirenNet.forward (models.py:311-322).
 * Forward mode: with Th_l^d = d h_l / d x_d and Ta_l^d = d a_l / d x_d,
 *   Th_l^d = [pm_l > 0] (.) (Th_{l-1}^d Wm_l[:, :hidden]^T + Wm_l[:, hidden + d])          (ReLU'(0) = 0, as torch)
 *   Ta_l^d = w_l cos(w_l ps_l) (.) (Ta_{l-1}^d Ws_l^T) (.) h_l + s_l (.) Th_l^d,       dy / dx_d = Ta_{L-1}^d . w_head,
 * the two products of the value rows on more rows, without bias: a point travels as four consecutive rows (value,
 * d/dx_0, d/dx_1, d/dx_2) of BOTH LDS images through the tile loop of mri_modsiren_forward's kernel, on the same
 * bf16x3 form.  Nothing (n, hidden)-sized is written: the call reads n dim_in floats and writes n (1 + dim_in).  No
 * atomics, a fixed summation order: bitwise reproducible.  At most 256 workgroups walk tiles of 2048 / hidden points.
 * Supported (mri_modsiren_gradient_supported is the truth): what mri_modsiren_supported accepts with dim_in <= 3;
 * anything else is refused with MRI_ERR_INVALID_ARGUMENT, the offending argument named in mri_last_error.  n = 0
 * returns 0 without a launch.  Parameters as mri_modsiren_forward, every weight matrix 16-byte aligned; x, y and dydx
 * are accessed 4 bytes at a time at any 4-byte aligned address.  workspace: mri_modsiren_gradient_workspace_bytes
 * device bytes (what mri_modsiren_forward_workspace_bytes reports: the split weights of both stacks; -1 for an
 * unsupported width or depth), 16-byte aligned; its contents on entry do not matter. */
int mri_modsiren_gradient_supported(int32_t dim_in, int32_t hidden, int32_t n_layers, int32_t dim_out);
int64_t mri_modsiren_gradient_workspace_bytes(int32_t hidden, int32_t n_layers);
int mri_modsiren_gradient(const float* x, int64_t n, int32_t dim_in, int32_t hidden, int32_t n_layers,
                          const float* const* siren_weight, const float* const* siren_bias,
                          const float* const* mod_weight, const float* const* mod_bias, float w0_first, float w0,
                          float* y, float* dydx, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- RffNet: Gaussian Fourier features and a ReLU MLP (csrc/rff.hip) ------------------------
 * (reference models.py:542-584.)  rff.layers.GaussianEncoding holds a frozen b (n_freq, dim_in) and computes
 * vp = (fl32(2 pi) x) b^T -- the coordinates are scaled first, then multiplied -- and z = [cos(vp) | sin(vp)],
 * cosines first.  Sine and cosine are correct for every finite argument: the Cody-Waite fast path up to |vp| = 8192,
 * the library's full-range sincosf beyond.  Every buffer is contiguous row-major and accessed 4 bytes at a time at
 * any 4-byte aligned address; nothing is written beyond row n; n = 0 returns 0 without a launch.
 * mri_rff_encode (models.py:542-584, the encoder): z (n, 2 n_freq).  1 <= dim_in <= 8, n_freq >= 1.
 * mri_rff_encode_backward_input (models.py:542-584, autograd of the encoder with respect to x):
 *   dx[i, d] = fl32(2 pi) sum_f b[f, d] (cos(vp_f) dz[i, n_freq + f] - sin(vp_f) dz[i, f]),
 *   one wave per row, summed in a fixed order: no atomics, bitwise reproducible.  b gets no gradient (it is frozen). */
int mri_rff_encode(const float* x, int64_t n, int32_t dim_in, const float* b, int32_t n_freq, float* z, void* stream);
int mri_rff_encode_backward_input(const float* x, int64_t n, int32_t dim_in, const float* b, int32_t n_freq,
                                  const float* dz, float* dx, void* stream);
/* Inference of the whole network (models.py:542-584: the encoder, then `decoder`, n_layers Linears
 * 2 n_freq -> hidden -> ... -> hidden -> 1 with ReLU behind EVERY one, the last included) in ONE persistent kernel:
 * the VALU encodes a row tile into two f32 LDS images (cos, sin) -- z is never written, 8 n_freq bytes of HBM
 * traffic per point saved each way --; the first Linear is two hidden x hidden products, W_0[:, :n_freq] on the cos
 * image and W_0[:, n_freq:] on the sin image, into one accumulator on the bf16 matrix pipe with three-term operands
 * (f32-accurate); Linears 1 .. n_layers - 2 are one product each; bias and ReLU are the epilogue; the head is a dot
 * product per row, plus bias, then ReLU: y (n) >= 0.  512 threads, at most 256 workgroups, tiles of 64 rows at
 * hidden 128 and 128 rows at hidden 64.  Fixed summation order: two calls agree bitwise.
 * Supported (mri_rff_forward_supported is the truth): hidden 64 / 128, n_freq == hidden, 1 <= dim_in <= 4,
 * 2 <= n_layers <= 8, dim_out 1, a bias on every Linear; anything else is refused with MRI_ERR_INVALID_ARGUMENT, the
 * offending argument named in mri_last_error.  weight / bias: HOST arrays of n_layers device pointers ([0] (hidden,
 * 2 n_freq), [1 .. n_layers-2] (hidden, hidden), [n_layers-1] (1, hidden)).  workspace:
 * mri_rff_forward_workspace_bytes device bytes (the split weights: n_layers hidden x hidden matrices in three bf16
 * terms; -1 for an unsupported width or depth), 16-byte aligned; its contents on entry do not matter. */
int mri_rff_forward_supported(int32_t dim_in, int32_t hidden, int32_t n_freq, int32_t n_layers, int32_t dim_out);
int64_t mri_rff_forward_workspace_bytes(int32_t hidden, int32_t n_layers);
int mri_rff_forward(const float* x, int64_t n, int32_t dim_in, int32_t hidden, int32_t n_freq, int32_t n_layers,
                    const float* b, const float* const* weight, const float* const* bias, float* y, void* workspace,
                    int64_t workspace_bytes, void* stream);
/* Values AND the gradient with respect to the coordinates of the same network (models.py:542-584), y (n) and dydx
 * (n, dim_in) row-major, dydx[i, d] = d y[i] / d x[i, d], in ONE persistent kernel instead of autograd through the
 * layer path.  Forward mode: with vp as above, p_l the pre-activation of Linear l and T_l^d = d relu(p_l) / d x_d,
 *   Tz^d  = [-fl32(2 pi) b[:, d] (.) sin(vp) | fl32(2 pi) b[:, d] (.) cos(vp)]
 *   T_0^d = [p_0 > 0] (.) (Tz^d W_0^T),   T_l^d = [p_l > 0] (.) (T_{l-1}^d W_l^T),
 *   dy / dx_d = [p_head > 0] (T_{n_layers-2}^d . w_head)                                 (ReLU'(0) = 0, as torch)
 * the products of the value rows on more rows, without bias: a point travels as four consecutive rows (value, d/dx_0,
 * d/dx_1, d/dx_2; dim_in <= 3) or eight (value, d/dx_0 .. d/dx_2 | value, d/dx_3, 0, 0; dim_in = 4) of BOTH LDS images
 * through the tile loop of mri_rff_forward's kernel, on the same bf16x3 form.  y is mri_rff_forward's bit for bit.
 * Nothing (n, hidden)-sized is written: the call reads n dim_in floats and writes n (1 + dim_in).  No atomics, a fixed
 * summation order: bitwise reproducible.  At most 256 workgroups walk tiles of 2048 / hidden points (dim_in = 4: 1024 /
 * hidden).
 * mri_rff_gradient_supported (models.py:542-584): exactly what mri_rff_forward_supported accepts.
 * mri_rff_gradient_workspace_bytes (models.py:542-584): what mri_rff_forward_workspace_bytes reports (the split
 *   weights; -1 for an unsupported width or depth), 16-byte aligned; its contents on entry do not matter.
 * mri_rff_gradient (models.py:542-584, autograd of the network with respect to x): every argument is validated before
 *   any pointer reaches the device (MRI_ERR_INVALID_ARGUMENT, the offending argument named in mri_last_error); n = 0
 *   returns 0 without a launch.  b / weight / bias as mri_rff_forward; x, y and dydx are accessed 4 bytes at a time
 *   at any 4-byte aligned address, nothing is written beyond row n. */
int mri_rff_gradient_supported(int32_t dim_in, int32_t hidden, int32_t n_freq, int32_t n_layers, int32_t dim_out);
int64_t mri_rff_gradient_workspace_bytes(int32_t hidden, int32_t n_layers);
int mri_rff_gradient(const float* x, int64_t n, int32_t dim_in, int32_t hidden, int32_t n_freq, int32_t n_layers,
                     const float* b, const float* const* weight, const float* const* bias, float* y, float* dydx,
                     void* workspace, int64_t workspace_bytes, void* stream);
/* ---- RffNet: fused training step (csrc/rff.hip) ---------------------------------------------
 * Forward with the loss and the backward chain of the same network, in place of training_step + autograd over the
 * layer ops (models.py:542-584 RffNet.forward; models.py:61-66 training_step: F.mse_loss).  Notation: Linears
 * 0 .. L-1 (L = n_layers), z = [c | s], a_0 = relu(z W_0^T + b_0), ..., a_{L-2}, p = a_{L-2} . w_head + b_head,
 * y = relu(p).  b is frozen: no gradient with respect to b or x.  z (n, 2 n_freq) exists in HBM in NEITHER call.
 * mri_rff_train_supported (models.py:542-584; models.py:61-66): exactly what mri_rff_forward_supported accepts.
 * mri_rff_backward_workspace_bytes (models.py:542-584; models.py:61-66): ONE size for both calls, -1 for an
 *   unsupported width or depth or n outside 1 .. 2^31 - 1.  With G = min(ceil(n / rows), 256) chain workgroups (rows =
 *   64 at hidden 128, 128 at hidden 64), slab = hidden + 4 + (n_layers - 1) hidden floats, and Wg = min(ceil(n / 32),
 *   256) * (hidden == 64 ? 2 : 1) weight-gradient slabs of hidden^2 floats:
 *     bytes = round_up_256(4 max(G slab, 256, 2 Wg hidden^2)) + (2 n_layers - 2) * 6 hidden^2
 *   (the slabs; the n_layers forward splits and the n_layers - 2 transposed splits in three bf16 terms).  It does not
 *   grow with n once n fills 256 workgroups.  16-byte aligned; its contents on entry do not matter.
 * mri_rff_forward_loss (models.py:542-584; models.py:61-66): mri_rff_forward's kernel in its training form.  y (n) is
 *   bitwise mri_rff_forward's.  act: HOST array of n_layers - 1 device pointers to (n, hidden) row-major, 16-byte
 *   aligned buffers that receive a_0 .. a_{L-2}, each written once; nothing beyond row n.  dy (n) =
 *   (y > 0) ? 2 (y - target) / (n_total grad_divisor) : 0, that is dLoss/dp with the head's ReLU applied (ReLU'(0) = 0,
 *   as torch).  loss_out[0] += sum (y - target)^2 / n_total (n <= n_total: a slice of a batch, as
 *   mri_modsiren_forward_loss), the workgroups' shares added in a fixed order.
 * mri_rff_backward (models.py:542-584; models.py:61-66, autograd from dy): one persistent kernel walks the Linears
 *   from the head down with dz_l = da_l (.) [a_l > 0] in ONE LDS image and da_{l-1} = dz_l W_l on the bf16 matrix pipe
 *   (three-term operands); dz: HOST array of n_layers - 1 device pointers to (n, hidden) 16-byte aligned scratch, each
 *   written once.  dW_l (l = 1 .. L-2) = dz_l^T a_{l-1}: the SIREN chain's weight-gradient kernel.  dW_0 =
 *   [dz_0^T c | dz_0^T s]: a kernel of its own that recomputes c and s from x and b as the forward computes them.
 *   Bias and head gradients are summed per workgroup; all partial sums meet in `workspace` and are added in a fixed
 *   order: no float atomics, bitwise reproducible.  d_weight / d_bias (n_layers pointers each): gradients are ADDED.
 * Both calls validate every argument before any pointer reaches the device (NULLs, the alignment of act / dz /
 * workspace, ranges including n <= n_total, a short workspace, unsupported shapes: MRI_ERR_INVALID_ARGUMENT with the
 * offending argument named in mri_last_error).  n = 0 returns 0 without a launch.  Every other pointer: any 4-byte
 * aligned address.  weight / bias as mri_rff_forward. */
int mri_rff_train_supported(int32_t dim_in, int32_t hidden, int32_t n_freq, int32_t n_layers, int32_t dim_out);
int64_t mri_rff_backward_workspace_bytes(int64_t n, int32_t hidden, int32_t n_layers);
int mri_rff_forward_loss(const float* x, const float* target, int64_t n, int64_t n_total, int32_t dim_in,
                         int32_t hidden, int32_t n_freq, int32_t n_layers, const float* b, const float* const* weight,
                         const float* const* bias, float grad_divisor, float* const* act, float* y, float* dy,
                         float* loss_out, void* workspace, int64_t workspace_bytes, void* stream);
int mri_rff_backward(const float* x, const float* dy, int64_t n, int32_t dim_in, int32_t hidden, int32_t n_freq,
                     int32_t n_layers, const float* b, const float* const* weight, const float* const* act,
                     float* const* dz, float* const* d_weight, float* const* d_bias, void* workspace,
                     int64_t workspace_bytes, void* stream);

/* ---- GaborNet: real Gabor (WIRE) layers (csrc/gabor.hip) -----------------------------------
 * (reference models.py:757-788 RealGaborLayer, models.py:836-885 GaborNet.)  A layer holds two Linears on the same
 * input, `freqs` and `scale`, and computes omega = w0 * freqs(a), scale = scale(a) * c, cos(omega) * exp(-(scale ** 2))
 * (models.py:785-788); the network is n_layers such layers dim_in -> hidden -> ... -> hidden -> dim_out, the LAST one
 * included.  The cosine is correct for every finite argument (the Cody-Waite fast path up to |omega| = 8192, the
 * library's full-range sincosf beyond); the envelope forms t = fl(fl(c s)^2) in the reference's order and is within
 * 2 ulp of exp(-t) of that float32 t while the result is a normal float (below: within 2^-126, flushing allowed); s =
 * +-inf gives 0, NaN gives NaN, as torch.  Every buffer is contiguous row-major and accessed 4 bytes at a time at any
 * 4-byte aligned address; nothing is written beyond element n hidden; n = 0 returns 0 without a launch.
 * mri_gabor_activation (models.py:785-788, behind the two Linears): out (n, hidden) = cos(w0 u) exp(-(c s)^2)
 *   elementwise over u, s (n, hidden).  hidden >= 1, n hidden < 2^38, w0 and c finite.
 * mri_gabor_activation_backward (models.py:785-788, autograd): with omega = w0 u, sigma = c s, e = exp(-sigma^2),
 *   du = -g w0 sin(omega) e and ds = -2 c sigma cos(omega) e g; g, du, ds (n, hidden).  du and ds are OVERWRITTEN. */
int mri_gabor_activation(const float* u, const float* s, int64_t n, int32_t hidden, float w0, float c, float* out,
                         void* stream);
int mri_gabor_activation_backward(const float* u, const float* s, const float* g, int64_t n, int32_t hidden, float w0,
                                  float c, float* du, float* ds, void* stream);
/* Inference of the whole network (models.py:836-885 GaborNet.forward; models.py:784-788 per layer) in ONE persistent
 * kernel: layer 0 (dim_in -> hidden, both Linears) runs on the VALU into an f32 LDS image of the row tile; layers
 * 1 .. n_layers - 2 are two hidden x hidden products each from the SAME image into two accumulators on the bf16 matrix
 * pipe with three-term operands (f32-accurate), their weights streamed as a pair of chunks; the epilogue
 * cos(w0 (acc_f + b_f)) exp(-(c (acc_s + b_s))^2) writes the image back; the head is a Gabor layer too, two dot products
 * per row plus biases: y (n) lies in (-1, 1].  Nothing (n, hidden)-sized is written.  512 threads, at most 256
 * workgroups, tiles of 128 rows at hidden 128 and 256 rows at hidden 64.  No atomics, a fixed summation order: two
 * calls agree bitwise.
 * mri_gabor_forward_supported (models.py:836-864) is the truth about what is served: hidden 64 / 128,
 *   1 <= dim_in <= 4, 2 <= n_layers <= 8, dim_out 1, a bias on every Linear; anything else is refused.
 * mri_gabor_forward_workspace_bytes (models.py:860-864): 2 (n_layers - 2) hidden x hidden matrices in three bf16 terms,
 *   12 (n_layers - 2) hidden^2 bytes (0 for n_layers = 2: workspace may then be NULL); -1 for an unsupported width or
 *   depth.  The size is exact, 16-byte aligned; its contents on entry do not matter.
 * mri_gabor_forward (models.py:866-867, 882-885): every argument is validated before any pointer reaches the device
 *   (MRI_ERR_INVALID_ARGUMENT, the offending argument named in mri_last_error).  freq_weight / freq_bias / scale_weight /
 *   scale_bias: HOST arrays of n_layers device pointers ([0] (hidden, dim_in), [1 .. n_layers-2] (hidden, hidden),
 *   [n_layers-1] (1, hidden); biases (hidden), the last (1)).  w0 and c finite. */
int mri_gabor_forward_supported(int32_t dim_in, int32_t hidden, int32_t n_layers, int32_t dim_out);
int64_t mri_gabor_forward_workspace_bytes(int32_t hidden, int32_t n_layers);
int mri_gabor_forward(const float* x, int64_t n, int32_t dim_in, int32_t hidden, int32_t n_layers,
                      const float* const* freq_weight, const float* const* freq_bias,
                      const float* const* scale_weight, const float* const* scale_bias, float w0, float c, float* y,
                      void* workspace, int64_t workspace_bytes, void* stream);

/* ---- PsfSirenNet: the acquisition point-spread function -----------------------------------
 * (reference models.py:397-539.)  A target voxel b is the network averaged over S sample points around it:
 * rows b*S + k of the expanded batch hold x[b] + offsets[k], and the voxel value is sum_k w_k z[b*S + k]
 * (psf_conv, a Conv1d of kernel S and stride S).  1 <= S <= 4096, 1 <= dim_in (C) <= 8; every buffer is
 * contiguous row-major.  Sums over the S samples of a target are owned by one wave (half-wave when S <= 32),
 * taken in a fixed lane order in float64: results are bitwise reproducible and independent of the grid.
 * mri_psf_expand (x_to_psf_x, models.py:520-526): x_psf (n*S, dim_in) = x.repeat_interleave(S, 0) +
 *   offsets.repeat(n, 1), one f32 add per element (bit-exact); offsets (S, dim_in).
 * mri_psf_reduce: out (n, C)[b, c] = sum_k w_k in[b*S + k, c]; w (S) or NULL for w_k = 1.  The Conv1d
 *   forward (C = 1, models.py:535) and the backward of the expansion (C = dim_in, w = NULL).
 * mri_psf_broadcast: dz (n*S)[b*S + k] = scale * w_k * g[b], the Conv1d's backward.
 * mri_psf_mse_loss (training_step, models.py:529-537: psf_conv, then F.mse_loss(z, y)): zbar_out (n)
 *   receives the reduced values, loss_out[0] += sum_b (zbar_b - y_b)^2 / n_total (ADDED; the caller zeroes),
 *   dz (n*S) = w_k * 2 (zbar_b - y_b) / (n_total * grad_divisor) (written; NULL: no gradient).  n <= n_total:
 *   a slice of n whole targets of a batch of n_total, as mri_siren_forward_loss.
 * Any 4-byte aligned pointers (mri_psf_expand stores 16 bytes at a time where x_psf is 16-byte aligned). */
int mri_psf_expand(const float* x, int64_t n, int32_t dim_in, const float* offsets, int32_t S,
                   float* x_psf, void* stream);
int mri_psf_reduce(const float* in, int64_t n, int32_t S, int32_t C, const float* w, float* out,
                   void* stream);
int mri_psf_broadcast(const float* g, int64_t n, int32_t S, const float* w, float scale, float* dz,
                      void* stream);
int mri_psf_mse_loss(const float* z, const float* target, int64_t n, int64_t n_total, int32_t S,
                     const float* w, float grad_divisor, float* zbar_out, float* loss_out, float* dz,
                     void* stream);

/* ---- BatchNorm1d + activation (the default HashMLP decoder block) ----------------------------
 * (torch.nn.BatchNorm1d as used at reference models.py:728-737: Linear -> BatchNorm1d -> GELU -> Dropout(0).)
 * z (n, C) float32 row-major with a leading dimension, 1 <= C <= 1024; training needs n >= 2.  Every
 * per-feature sum is taken in float64 in an order fixed by (n, C, 16-byte alignment of the matrices) alone --
 * contiguous row chunks, a fixed tree inside a chunk, the chunk sums added in a fixed order, no atomics:
 * bitwise reproducible.  `workspace`: mri_bn_workspace_bytes(n, C) bytes, 16-byte aligned, shared by
 * mri_bn_stats and mri_bn_act_backward (the backward leaves two batch means in it between its kernels).
 * mri_bn_stats (BatchNorm1d.forward in train(), the statistics): save (2, C) = batch mean and
 *   invstd = 1 / sqrt(var + eps) with the BIASED variance (sums of z - z[0, c] and its square: exact in
 *   float64 whatever the mean); running_mean = (1 - momentum) running_mean + momentum mean, running_var
 *   likewise with the UNBIASED variance var n / (n - 1), num_batches_tracked[0] += 1 (int64, on the
 *   device).  Any of the three buffers may be NULL (not tracked).
 * mri_bn_act_forward: y = act(gamma * ((z - mean) * invstd) + beta), act one of MRI_ACT_IDENTITY / RELU /
 *   GELU.  save != NULL: the batch statistics of mri_bn_stats (training); save == NULL: the eval form
 *   with running_mean and invstd = 1 / sqrt(running_var + eps); no buffer is written.  y may be z.
 * mri_bn_act_backward (autograd of the same): g = dy * act'(u), dbeta = sum g, dgamma = sum g xhat,
 *   dz = gamma invstd (g - dbeta / n - xhat dgamma / n); xhat and u are recomputed from z and save with the
 *   forward's expressions (nothing else is kept for the backward).  d_gamma / d_beta are written
 *   (overwrite != 0) or added to; dz may alias dy (same leading dimension), not z.
 * The matrices (z, y, dy, dz) may be any 4-byte aligned pointers with any leading dimension >= C (16-byte accesses
 * when all matrices of a call are 16-byte aligned, their leading dimensions and C multiples of 4); gamma, beta,
 * save, the running buffers and the gradients are read and written float by float. */
int64_t mri_bn_workspace_bytes(int64_t n, int32_t C);
int mri_bn_stats(const float* z, int64_t ldz, int64_t n, int32_t C, double momentum, double eps,
                 float* running_mean, float* running_var, int64_t* num_batches_tracked, float* save,
                 void* workspace, int64_t workspace_bytes, void* stream);
int mri_bn_act_forward(const float* z, int64_t ldz, int64_t n, int32_t C, const float* save,
                       const float* running_mean, const float* running_var, double eps, const float* gamma,
                       const float* beta, int32_t activation, float* y, int64_t ldy, void* stream);
int mri_bn_act_backward(const float* dy, int64_t lddy, const float* z, int64_t ldz, int64_t n, int32_t C,
                        const float* save, const float* gamma, const float* beta, int32_t activation,
                        float* dz, int64_t lddz, float* d_gamma, float* d_beta, int32_t overwrite,
                        void* workspace, int64_t workspace_bytes, void* stream);

/* ---- loss ------------------------------------------------------------------------------
 * F.mse_loss(y, y_pred) (reference models.py:64): loss_out[0] += mean((pred-target)^2)
 * (device scalar, caller zeroes), d_pred = 2 (pred - target) / (count * grad_divisor) if
 * d_pred != NULL.  pred/target/d_pred are contiguous with `count` elements.
 * grad_divisor > 1 pre-averages gradients over data-parallel ranks.  4-byte accesses: any pointers. */
int mri_mse_loss(const float* pred, const float* target, int64_t count, float grad_divisor,
                 float* loss_out, float* d_pred, void* stream);

/* ---- optimiser -------------------------------------------------------------------------
 * torch.optim.Adam, single step over one flat buffer (reference models.py:68-70; defaults
 * betas (0.9, 0.999), eps 1e-8, no weight decay).  `step` is the 1-based step count.
 * grad_scale multiplies the gradient first (1/world_size after an all-reduce sum).
 * The four pointers may be any 4-byte aligned range of their buffers as long as they share
 * one offset within a 16-byte line (the same slice of four 16-byte aligned buffers does):
 * data-parallel ranks step each level group as soon as its reduction has landed. */
int mri_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                  int64_t count, double lr, double beta1, double beta2, double eps,
                  int32_t step, float grad_scale, void* stream);

/* ---- one training step, queued by one call ----------------------------------------------------
 * The per-batch body of the reference's training loop for its HashMLP path with the tiny-MLP decoder
 * (reference launcher.py:156-165 pl.Trainer.fit -> models.py:61-70 training_step / backward / Adam.step, with
 * the DataLoader of datamodules.py:198-205 producing the next batch meanwhile) as ONE host call that
 * composes the entry points above:
 *   side stream: [count this batch's gradient records if `counted` = 0]; sample + gather the NEXT batch;
 *                zero its absmax buffer; count its records
 *   main stream: lookup -> decoder forward + MSE + backward (overwriting every gradient) -> table gradient
 *                (MRI_BWD_PREPARED | MRI_BWD_OVERWRITE) -> Adam over [param, param + n_params)
 * The side work of a call is awaited by the next call (`join_pending` = 1) or through `ev_join`.
 * All pointers are device pointers except `grid`, `shape`, `axis_offset` (host); streams and events are the
 * caller's.  Feature-major (2 L, n) blocks `enc`, `d_enc`.  Same launches on the same data as the separate
 * calls: results are bit-identical.  Why: queued op by op from an interpreter the step costs more host
 * time than GPU time on a slow host.  One launch fewer than the separate calls: with n_params > 0
 * the table gradient's last conversion (int64 sums -> f32, bin_finalize_kernel) is done by the Adam kernel as it
 * fetches the gradient (the same expression: the same bits) -- `d_table` then does NOT hold the gradient of those
 * levels after the call.  That fold needs param / grad / exp_avg / exp_avg_sq 16-byte aligned; other ranges (one
 * 4-byte aligned offset within a 16-byte line, as mri_adam_step asks) run the conversion launch and mri_adam_step:
 * the same bits.  `table` as for mri_hashgrid_forward, checked at the top of the call, before anything is queued. */
typedef struct mri_fused_step_args {
  const mri_grid_desc* grid;
  float* table;                                  /* (sum T_l, F), inside the flat parameter buffer */
  const float *w1, *b1, *w2, *b2, *w3, *b3;      /* decoder k_in -> hidden -> hidden -> 1 */
  float *d_table, *d_w1, *d_b1, *d_w2, *d_b2, *d_w3, *d_b3, *loss;
  int32_t hidden, bwd_method, counted, join_pending;
  const float* coords;                           /* (n, D) this step's batch */
  const float* target;                           /* (n) */
  int64_t n;
  float *enc, *d_enc;                            /* (2 L, n) each */
  void* tiny_ws;                                 /* mri_tiny_mlp_workspace_bytes */
  int64_t tiny_ws_bytes;
  void* bwd_ws;                                  /* mri_hashgrid_backward_workspace_bytes, this batch's */
  int64_t bwd_ws_bytes;
  float* absmax;                                 /* 32 zeroed floats, or NULL (pass over d_enc instead) */
  float *param, *grad, *exp_avg, *exp_avg_sq;    /* Adam: one range of the flat buffers */
  int64_t n_params;
  double lr, beta1, beta2, eps;
  int32_t step;                                  /* 1-based */
  float grad_scale;
  int64_t* next_idx;                             /* NULL: no batch is produced */
  float *next_coords, *next_target;
  int64_t next_n;
  void* next_bwd_ws;                             /* NULL: the next batch is not counted ahead */
  int64_t next_bwd_ws_bytes;
  float* next_absmax;
  uint64_t seed;                                 /* mri_sample_indices(seed, first, lo, hi, next_n) */
  int64_t first, lo, hi;
  int32_t dim, reserved;
  int64_t shape[MRI_MAX_DIM], axis_offset[MRI_MAX_DIM];
  const float *axes, *volume;                    /* mri_gather_batch */
  void *stream, *stream_side, *ev_fork, *ev_join;
  void* ev_phase[5];                             /* all NULL, or five timing events recorded on `stream` around
                                                    lookup | decoder | table gradient | Adam (a measuring caller
                                                    brackets the phases without leaving this call) */
  float grad_divisor;                            /* gradients of mean((y - t)^2) / grad_divisor; 0 = 1.  Data
                                                    parallel: the world size, with n_params = 0 -- the caller
                                                    reduces `grad` over the ranks and steps (mri_adam_step) */
  float reserved2;
} mri_fused_step_args;
int mri_fused_step(const mri_fused_step_args* args);
int64_t mri_fused_step_args_bytes(void); /* sizeof(mri_fused_step_args): lets a binding check its layout */

/* ---- coordinate-batch producer ------------------------------------------------------------
 * Replaces MriImage.__getitem__ + DataLoader(shuffle=True) collate (reference
 * datamodules.py:140-172, 198-205) with on-device generation.
 * mri_sample_indices: idx_out[i] = lo + perm_epoch((first + i) mod (hi-lo)), a keyed
 *   bijection of [0, hi-lo) (without-replacement shuffle, one key per epoch/seed).
 * mri_gather_batch: flat C-order voxel index -> coordinates (row-major (n, D)) through the
 *   per-axis linspace tables (`axes` = concatenation of the D axis arrays built with
 *   torch.linspace on the host, axis_offset[d] = start of axis d) and targets from `volume`.
 *   shape / axis_offset are HOST arrays of length D.  4-byte (idx: 8-byte) accesses: any such pointers. */
int mri_sample_indices(uint64_t seed, int64_t first, int64_t lo, int64_t hi, int64_t n,
                       int64_t* idx_out, void* stream);
int mri_gather_batch(const int64_t* idx, int64_t n, int32_t dim, const int64_t* shape,
                     const float* axes, const int64_t* axis_offset, const float* volume,
                     float* coords_out, float* target_out /* may be NULL */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MRI_INR_H */
