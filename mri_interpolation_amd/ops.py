"""Tensor-level wrappers over the C ABI (include/mri_inr.h) and the autograd glue.

PyTorch is plumbing here: it owns device memory and the stream; every computation below
is a call into libmri_inr.so.  CPU tensors are rejected -- there is no fallback.
"""
import ctypes as C
from typing import Optional, Sequence

import torch

from . import _lib
from ._lib import (ACT_GELU, ACT_IDENTITY, ACT_RELU, ACT_SINE, DERIV_MUL, DERIV_NONE,  # noqa: F401
                   DERIV_RELU_MASK, GridDesc)


# --------------------------------------------------------------------------- helpers
def _gpu(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("mri_interpolation_amd: the hot path runs on MI355X only; got a "
                               f"{t.device} tensor (no CPU fallback exists)")
        if t.dtype != torch.float32 and t.dtype != torch.int64:
            raise TypeError(f"expected float32/int64 tensor, got {t.dtype}")


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    # the raw handle of the current stream: torch.cuda.current_stream() builds a Stream object and resolves
    # the device three times over (8 us per call, a dozen calls per training step: tools/host_profile.py)
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(torch.cuda.current_device()))


def _rowmajor(t: torch.Tensor) -> torch.Tensor:
    """2-D view with unit column stride (copies only if needed)."""
    if t.dim() != 2:
        t = t.reshape(-1, t.shape[-1])
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t


def make_grid_desc(dim: int, resolutions: Sequence[Sequence[float]], sizes: Sequence[int],
                   n_features: int) -> GridDesc:
    """Host descriptor from per-level per-axis resolutions and table sizes."""
    if not (1 <= dim <= _lib.MAX_DIM):
        raise ValueError(f"HashGrid only supports 1..{_lib.MAX_DIM}-D inputs")
    if not (1 <= len(sizes) <= _lib.MAX_LEVELS):
        raise ValueError(f"n_levels must be in 1..{_lib.MAX_LEVELS}")
    g = GridDesc()
    g.dim, g.n_levels, g.n_features = dim, len(sizes), n_features
    off = 0
    for l, (res, size) in enumerate(zip(resolutions, sizes)):
        for d in range(dim):
            g.resolution[l][d] = float(res[d])
        g.table_size[l] = int(size)
        g.table_offset[l] = off
        off += int(size)
    return g


def grid_rows(desc: GridDesc) -> int:
    return sum(desc.table_size[l] for l in range(desc.n_levels))


def _enc_strides(desc: GridDesc, n: int, feature_major: bool):
    f = desc.n_features
    if feature_major:  # (L*F, n)
        return f * n, 1, n
    return f, desc.n_levels * f, 1  # reference layout (n, L*F)


# --------------------------------------------------------------------------- hash grid
def hashgrid_forward(desc: GridDesc, x: torch.Tensor, table: torch.Tensor,
                     out: Optional[torch.Tensor] = None, feature_major: bool = False,
                     row_offset: int = 0):
    """Encode the rows of `x`.  With `row_offset`, `x` is a slice of a larger batch whose features
    live in `out` (the whole batch's buffer): the slice's features go to rows / columns
    [row_offset, row_offset + len(x))."""
    _gpu(x, table, out)
    x = _rowmajor(x).contiguous()
    n, width = x.shape[0], desc.n_levels * desc.n_features
    if x.shape[1] != desc.dim:
        raise ValueError(f"x has {x.shape[1]} columns, encoder expects {desc.dim}")
    if out is None:
        out = torch.empty((width, n) if feature_major else (n, width), device=x.device,
                          dtype=torch.float32)
    n_total = out.shape[1] if feature_major else out.shape[0]
    if row_offset < 0 or row_offset + n > n_total:
        raise ValueError("slice does not fit the output buffer")
    sl, sr, sf = _enc_strides(desc, n_total, feature_major)
    base = out.data_ptr() + 4 * row_offset * sr
    _lib.call("mri_hashgrid_forward", C.byref(desc), _ptr(x), n, _ptr(table), C.c_void_p(base), sl,
              sr, sf, _stream())
    return out


def _grow_scratch(cache, device, need_bytes, dtype=torch.float32):
    """The process-wide scratch of one kernel family: one tensor per device in the dict `cache` (device index ->
    tensor), of at least need_bytes.  It only ever grows; before a larger one replaces it the device is synchronised,
    so no kernel of any stream can still be using the buffer that goes back to the allocator.  need_bytes <= 0 (a call
    that needs none, or a shape the library is about to refuse with its reason): whatever is cached, else 64 elements
    (floats, by default) that are not kept."""
    ws = cache.get(device.index)
    if need_bytes <= 0:
        return ws if ws is not None else torch.empty(64, dtype=dtype, device=device)
    if ws is None or ws.numel() * ws.element_size() < need_bytes:
        if ws is not None:
            torch.cuda.synchronize(device)
        size = torch.empty((), dtype=dtype).element_size()
        ws = cache[device.index] = torch.empty((need_bytes + size - 1) // size, dtype=dtype, device=device)
    return ws


def _outputs(what, x, y, dydx=False):
    """y (n, 1) of a chain call on x (n, dim_in) and, unless dydx is False, dydx (n, dim_in): allocated where None,
    else held to their sizes (the library sees pointers only)."""
    n, dim_in = x.shape[0], x.shape[-1]
    if y is None:
        y = torch.empty((n, 1), device=x.device, dtype=torch.float32)
    if y.numel() != n:
        raise ValueError(f"{what}: y holds n values")
    if dydx is False:
        return y
    if dydx is None:
        dydx = torch.empty((n, dim_in), device=x.device, dtype=torch.float32)
    if dydx.shape != (n, dim_in):
        raise ValueError(f"{what}: y holds n values, dydx is (n, dim_in)")
    return y, dydx


def _check_stack(what, weights, want, vectors=(), matrices=(), label="Linear", at_least=2, buffers=None, flat=None,
                 extra=()):
    """What the library cannot see behind its pointers (a mismatched shape would be read or written out of bounds on
    the device).  A stack of Linears: weights[i] is of shape want[i] (want None: not held to shapes), every list of
    `vectors` holds one (want[i][0],) tensor per weight (biases, their gradients), every list of `matrices` one of shape
    want[i] (weight gradients).  buffers = (n, hidden, count, {name: list}): `count` per-layer (n, hidden) tensors in
    each list (an entry may be None where the library takes NULL); flat = (n, {name: tensor}): n values each; `extra`:
    further tensors.  Everything contiguous float32."""
    per_weight = list(vectors) + list(matrices)
    if len(weights) < at_least or any(len(o) != len(weights) for o in per_weight):
        raise ValueError(f"{what}: at least {at_least} {label}s, one bias / gradient per weight")
    for i, shape in enumerate(want or ()):
        got = [tuple(o[i].shape) for o in [weights] + list(matrices)], [tuple(v[i].shape) for v in vectors]
        if any(s != shape for s in got[0]) or any(s != (shape[0],) for s in got[1]):
            raise ValueError(f"{what}: {label} {i} is {shape} with a bias of {shape[0]}, got {got[0]} and {got[1]}")
    n, hidden, count, lists = buffers or (0, 0, 0, {})
    for name, seq in lists.items():
        if len(seq) != count:
            raise ValueError(f"{what}: {name} needs {count} (n, hidden) buffers, one per layer")
        if any(t is not None and tuple(t.shape) != (n, hidden) for t in seq):
            raise ValueError(f"{what}: {name} buffers are (n, hidden) = ({n}, {hidden})")
    n, named = flat or (0, {})
    for name, t in named.items():
        if t.numel() != n:
            raise ValueError(f"{what}: {name} holds n = {n} values")
    every = list(weights) + [t for o in per_weight for t in o] + [t for s in lists.values() for t in s if t is not None]
    for t in every + list(named.values()) + list(extra):
        if not t.is_contiguous() or t.dtype != torch.float32:
            raise ValueError(f"{what} needs contiguous float32 parameters and buffers")


_bwd_workspace = {}  # device index -> scratch (the library clears what it needs per call)


def backward_workspace_bytes(desc: GridDesc, n: int) -> int:
    need = _lib.load().mri_hashgrid_backward_workspace_bytes(C.byref(desc), n)
    if need < 0:
        _lib.check(-1, "mri_hashgrid_backward_workspace_bytes")
    return int(need)


def backward_workspace(desc: GridDesc, n: int, device) -> torch.Tensor:
    """Process-wide scratch of the module / autograd path (FusedStep owns its own buffer): _grow_scratch."""
    return _grow_scratch(_bwd_workspace, device, backward_workspace_bytes(desc, n), torch.int64)


def hashgrid_backward_prepare(desc: GridDesc, x: torch.Tensor, method: int = 0, stream=None,
                              ws: Optional[torch.Tensor] = None):
    """First stage of the binned backward (record counts per table slice): needs only `x`, so
    it can be queued on a side stream while the forward pass runs.  Follow with
    hashgrid_backward(..., prepared=True) on the same workspace `ws` (int64 tensor of at least
    backward_workspace_bytes(); default: the process-wide one)."""
    _gpu(x)
    n = x.shape[0]
    if ws is None:
        ws = backward_workspace(desc, n, x.device)
    st = C.c_void_p(stream.cuda_stream) if stream is not None else _stream()
    _lib.call("mri_hashgrid_backward_prepare", C.byref(desc), _ptr(x), n, method, _ptr(ws),
              ws.numel() * 8, st)


def hashgrid_backward(desc: GridDesc, x: torch.Tensor, d_out: torch.Tensor,
                      d_table: torch.Tensor, feature_major: bool = False, method: int = 0,
                      prepared: bool = False, overwrite: bool = False,
                      level_mask: Optional[int] = None, ws: Optional[torch.Tensor] = None,
                      level_absmax: Optional[torch.Tensor] = None):
    """d_table += scatter of d_out (or d_table = ..., with overwrite=True); `level_mask`
    restricts the call to the levels whose bit is set (one level group of a bucketed,
    data-parallel backward); `level_absmax` (n_levels floats on the device): max |d_out| per level
    when the caller has it already (tiny_mlp_train(..., dx_absmax=)), saving a pass over d_out."""
    _gpu(x, d_out, d_table)
    x = _rowmajor(x).contiguous()
    n = x.shape[0]
    if not d_out.is_contiguous():
        d_out = d_out.contiguous()
    sl, sr, sf = _enc_strides(desc, n, feature_major)
    if method == 1:
        ws = None
    elif ws is None:
        ws = backward_workspace(desc, n, x.device)
    flags = (method | (_lib.BWD_PREPARED if prepared else 0)
             | (_lib.BWD_OVERWRITE if overwrite else 0))
    if level_absmax is not None:
        _gpu(level_absmax)
        if level_absmax.numel() < desc.n_levels or level_absmax.dtype != torch.float32:
            raise ValueError("level_absmax: one float32 per level")
        _lib.call("mri_hashgrid_backward_scaled", C.byref(desc), _ptr(x), _ptr(d_out), n, sl, sr,
                  sf, _ptr(d_table), flags, (0xFFFFFFFF if level_mask is None else level_mask) & 0xFFFFFFFF,
                  _ptr(level_absmax), _ptr(ws), ws.numel() * 8 if ws is not None else 0, _stream())
    elif level_mask is None:
        _lib.call("mri_hashgrid_backward", C.byref(desc), _ptr(x), _ptr(d_out), n, sl, sr, sf,
                  _ptr(d_table), flags, _ptr(ws), ws.numel() * 8 if ws is not None else 0,
                  _stream())
    else:
        _lib.call("mri_hashgrid_backward_levels", C.byref(desc), _ptr(x), _ptr(d_out), n, sl, sr,
                  sf, _ptr(d_table), flags, level_mask & 0xFFFFFFFF, _ptr(ws),
                  ws.numel() * 8 if ws is not None else 0, _stream())
    return d_table


def hashgrid_backward_adam(desc: GridDesc, x: torch.Tensor, d_out: torch.Tensor, table: torch.Tensor,
                           exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, lr: float, beta1: float,
                           beta2: float, eps: float, step: int, grad_scale: float = 1.0,
                           feature_major: bool = False, method: int = 0, prepared: bool = False,
                           ws: Optional[torch.Tensor] = None) -> bool:
    """Table gradient and the table's Adam step in one pass (mri_hashgrid_backward_adam): `table`,
    `exp_avg`, `exp_avg_sq` are updated in place, no gradient tensor is produced.  Returns False
    (nothing done) when a level of the grid is not served by the binned kernels."""
    _gpu(x, d_out, table, exp_avg, exp_avg_sq)
    x = _rowmajor(x).contiguous()
    n = x.shape[0]
    if not d_out.is_contiguous():
        d_out = d_out.contiguous()
    if not (table.is_contiguous() and exp_avg.is_contiguous() and exp_avg_sq.is_contiguous()):
        raise ValueError("hashgrid_backward_adam needs contiguous table / moment buffers")
    sl, sr, sf = _enc_strides(desc, n, feature_major)
    if method == 1:
        return False
    if ws is None:
        ws = backward_workspace(desc, n, x.device)
    flags = method | (_lib.BWD_PREPARED if prepared else 0)
    rc = _lib.load().mri_hashgrid_backward_adam(
        C.byref(desc), _ptr(x), _ptr(d_out), n, sl, sr, sf, _ptr(table), _ptr(exp_avg), _ptr(exp_avg_sq),
        float(lr), float(beta1), float(beta2), float(eps), int(step), float(grad_scale), flags, _ptr(ws),
        ws.numel() * 8, _stream())
    if rc == _lib.ERR_UNSUPPORTED:
        return False
    _lib.check(rc, "mri_hashgrid_backward_adam")
    return True


def hashgrid_backward_input(desc: GridDesc, x: torch.Tensor, d_out: torch.Tensor,
                            table: torch.Tensor, feature_major: bool = False) -> torch.Tensor:
    """d loss / d x (n, D): the reference keeps x -> x*res - trunc(x*res) differentiable
    (encoding.py:111-113), so callers that track coordinates (e.g. spatial derivatives of the
    implicit image) get their gradient; the training path never asks for it."""
    _gpu(x, d_out, table)
    x = _rowmajor(x).contiguous()
    n = x.shape[0]
    if not d_out.is_contiguous():
        d_out = d_out.contiguous()
    sl, sr, sf = _enc_strides(desc, n, feature_major)
    dx = torch.empty_like(x)
    _lib.call("mri_hashgrid_backward_input", C.byref(desc), _ptr(x), _ptr(d_out), n, sl, sr, sf,
              _ptr(table), _ptr(dx), _stream())
    return dx


class HashGridFunction(torch.autograd.Function):
    """Autograd node for the encoder: gradient to the table (the training path) and, when the
    caller tracks the coordinates, to x (the reference keeps that path, encoding.py:113)."""

    @staticmethod
    def forward(ctx, x, table, desc):
        ctx.desc = desc
        ctx.save_for_backward(x, table)
        return hashgrid_forward(desc, x, table)

    @staticmethod
    def backward(ctx, d_out):
        x, table = ctx.saved_tensors
        d_out = d_out.contiguous()
        d_x = d_table = None
        if ctx.needs_input_grad[1]:
            d_table = torch.zeros(table.shape, device=d_out.device, dtype=torch.float32)
            hashgrid_backward(ctx.desc, x, d_out, d_table)
        if ctx.needs_input_grad[0]:
            d_x = hashgrid_backward_input(ctx.desc, x, d_out, table).reshape(x.shape)
        return d_x, d_table, None


# --------------------------------------------------------------------------- linear layers
def linear_forward(x, weight, bias, activation=ACT_IDENTITY, w0=1.0, out=None, deriv=None,
                   x_feature_major=False):
    """y = act(w0 * (x W^T + b)); x is (M, K), or (K, M) when x_feature_major."""
    _gpu(x, weight, bias, out, deriv)
    n, k = weight.shape
    if x_feature_major:
        if not x.is_contiguous():
            x = x.contiguous()
        m, xrs, xcs = x.shape[1], 1, x.shape[1]
        if x.shape[0] != k:
            raise ValueError(f"x has {x.shape[0]} features, weight expects {k}")
    else:
        x = _rowmajor(x)
        m, xrs, xcs = x.shape[0], x.stride(0), 1
        if x.shape[1] != k:
            raise ValueError(f"x has {x.shape[1]} features, weight expects {k}")
    if not weight.is_contiguous():
        weight = weight.contiguous()
    if out is None:
        out = torch.empty((m, n), device=x.device, dtype=torch.float32)
    _lib.call("mri_linear_forward", _ptr(x), xrs, xcs, _ptr(weight), _ptr(bias), m, n, k,
              activation, float(w0), _ptr(out), out.stride(0), _ptr(deriv),
              deriv.stride(0) if deriv is not None else 0, _stream())
    return out


def linear_backward_data(dy, weight, deriv_mode=DERIV_NONE, deriv=None, dx=None,
                         dx_feature_major=False):
    _gpu(dy, weight, deriv, dx)
    dy = _rowmajor(dy)
    n, k = weight.shape
    m = dy.shape[0]
    if not weight.is_contiguous():
        weight = weight.contiguous()
    if dx is None:
        dx = torch.empty((k, m) if dx_feature_major else (m, k), device=dy.device,
                         dtype=torch.float32)
    drs, dcs = (1, dx.stride(0)) if dx_feature_major else (dx.stride(0), 1)
    _lib.call("mri_linear_backward_data", _ptr(dy), dy.stride(0), _ptr(weight), m, n, k,
              deriv_mode, _ptr(deriv), deriv.stride(0) if deriv is not None else 0, _ptr(dx),
              drs, dcs, _stream())
    return dx


def linear_backward_weight(dy, x, d_weight, d_bias=None, x_feature_major=False):
    """d_weight += dy^T x, d_bias += colsum(dy)."""
    _gpu(dy, x, d_weight, d_bias)
    dy = _rowmajor(dy)
    n, k = d_weight.shape
    m = dy.shape[0]
    if x_feature_major:
        if not x.is_contiguous():
            x = x.contiguous()
        xrs, xcs = 1, x.shape[1]
    else:
        x = _rowmajor(x)
        xrs, xcs = x.stride(0), 1
    _lib.call("mri_linear_backward_weight", _ptr(dy), dy.stride(0), _ptr(x), xrs, xcs, m, n, k,
              _ptr(d_weight), _ptr(d_bias), _stream())


def apply_deriv(dy, deriv_mode, deriv):
    _gpu(dy, deriv)
    if deriv_mode == DERIV_NONE:
        return dy
    _lib.call("mri_apply_deriv", _ptr(dy), dy.stride(0), deriv_mode, _ptr(deriv),
              deriv.stride(0), dy.shape[0], dy.shape[1], _stream())
    return dy


def deriv_mode_for(activation: int) -> int:
    return {ACT_IDENTITY: DERIV_NONE, ACT_RELU: DERIV_RELU_MASK, ACT_SINE: DERIV_MUL,
            ACT_GELU: DERIV_MUL}[activation]


class LinearActFunction(torch.autograd.Function):
    """y = act(w0 (x W^T + b)) as one MFMA kernel, with its three backward GEMMs."""

    @staticmethod
    def forward(ctx, x, weight, bias, activation, w0):
        lead = x.shape[:-1]
        x2 = _rowmajor(x)
        need_deriv = activation in (ACT_SINE, ACT_GELU)
        deriv = torch.empty((x2.shape[0], weight.shape[0]), device=x.device,
                            dtype=torch.float32) if need_deriv else None
        y = linear_forward(x2, weight, bias, activation, w0, deriv=deriv)
        ctx.activation = activation
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x2, weight, deriv if need_deriv else y)
        ctx.lead = lead
        return y.reshape(*lead, weight.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, weight, g = ctx.saved_tensors
        dz = dy.reshape(-1, weight.shape[0]).contiguous()
        mode = deriv_mode_for(ctx.activation)
        if mode != DERIV_NONE:
            dz = apply_deriv(dz.clone() if dz.data_ptr() == dy.data_ptr() else dz, mode, g)
        dx = d_w = d_b = None
        if ctx.needs_input_grad[0]:
            dx = linear_backward_data(dz, weight).reshape(*ctx.lead, weight.shape[1])
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            d_w = torch.zeros_like(weight)
            d_b = torch.zeros(weight.shape[0], device=dy.device) if ctx.has_bias else None
            linear_backward_weight(dz, x2, d_w, d_b)
        return dx, d_w, d_b, None, None


def linear_act(x, weight, bias, activation=ACT_IDENTITY, w0=1.0):
    return LinearActFunction.apply(x, weight, bias, activation, w0)


class ModulateFunction(torch.autograd.Function):
    """y = x (.) m, the elementwise modulation of reference models.py:318-320 (`x *= mod`)."""

    @staticmethod
    def forward(ctx, x, m):
        x2, m2 = _rowmajor(x), _rowmajor(m)
        ctx.save_for_backward(x2, m2)
        return apply_deriv(x2.clone(), DERIV_MUL, m2)

    @staticmethod
    def backward(ctx, dy):
        x2, m2 = ctx.saved_tensors
        dy = _rowmajor(dy)
        dx = apply_deriv(dy.clone(), DERIV_MUL, m2) if ctx.needs_input_grad[0] else None
        dm = apply_deriv(dy.clone(), DERIV_MUL, x2) if ctx.needs_input_grad[1] else None
        return dx, dm


def modulate(x, m):
    return ModulateFunction.apply(x, m)


# --------------------------------------------------------------------------- frequency encoding
def frequency_forward(x, n_levels: int, out=None):
    _gpu(x, out)
    x = _rowmajor(x)
    n, dim = x.shape
    if out is None:
        out = torch.empty((n, dim * 2 * n_levels), device=x.device, dtype=torch.float32)
    _lib.call("mri_frequency_forward", _ptr(x), x.stride(0), n, dim, n_levels, _ptr(out),
              out.stride(0), _stream())
    return out


def frequency_backward(x, d_out, n_levels: int):
    _gpu(x, d_out)
    x, d_out = _rowmajor(x), _rowmajor(d_out)
    n, dim = x.shape
    dx = torch.empty((n, dim), device=x.device, dtype=torch.float32)
    _lib.call("mri_frequency_backward", _ptr(x), x.stride(0), _ptr(d_out), d_out.stride(0), n,
              dim, n_levels, _ptr(dx), dx.stride(0), _stream())
    return dx


class FrequencyFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, n_levels):
        lead = x.shape[:-1]
        x2 = _rowmajor(x.reshape(-1, x.shape[-1]))
        ctx.save_for_backward(x2)
        ctx.n_levels, ctx.shape = n_levels, x.shape
        return frequency_forward(x2, n_levels).reshape(*lead, x.shape[-1] * 2 * n_levels)

    @staticmethod
    def backward(ctx, d_out):
        (x2,) = ctx.saved_tensors
        dx = frequency_backward(x2, d_out.reshape(x2.shape[0], -1), ctx.n_levels)
        return dx.reshape(ctx.shape), None


# --------------------------------------------------------------------------- Gaussian Fourier features (RffNet)
def rff_encode_forward(x, b, out=None):
    """z (n, 2F) = [cos(vp) | sin(vp)], vp = (fl32(2 pi) x) b^T (csrc/rff.hip); b (F, dim_in)."""
    _gpu(x, b, out)
    x, b = _rowmajor(x).contiguous(), b.contiguous()
    n, dim_in = x.shape
    if b.dim() != 2 or b.shape[1] != dim_in:
        raise ValueError(f"rff_encode: b is (n_frequencies, dim_in = {dim_in}), got {tuple(b.shape)}")
    if out is None:
        out = torch.empty((n, 2 * b.shape[0]), device=x.device, dtype=torch.float32)
    if tuple(out.shape) != (n, 2 * b.shape[0]) or not out.is_contiguous():
        raise ValueError("rff_encode: out is contiguous (n, 2 n_frequencies)")
    _lib.call("mri_rff_encode", _ptr(x), n, dim_in, _ptr(b), b.shape[0], _ptr(out), _stream())
    return out


def rff_encode_backward_input(x, b, d_out, dx=None):
    """dx (n, dim_in) of rff_encode_forward from d_out (n, 2F): one wave per row, a fixed summation order."""
    _gpu(x, b, d_out, dx)
    x, b, d_out = _rowmajor(x).contiguous(), b.contiguous(), _rowmajor(d_out).contiguous()
    n, dim_in = x.shape
    if tuple(d_out.shape) != (n, 2 * b.shape[0]):
        raise ValueError("rff_encode_backward_input: d_out is (n, 2 n_frequencies)")
    if dx is None:
        dx = torch.empty((n, dim_in), device=x.device, dtype=torch.float32)
    if tuple(dx.shape) != (n, dim_in) or not dx.is_contiguous():
        raise ValueError("rff_encode_backward_input: dx is contiguous (n, dim_in)")
    _lib.call("mri_rff_encode_backward_input", _ptr(x), n, dim_in, _ptr(b), b.shape[0], _ptr(d_out), _ptr(dx),
              _stream())
    return dx


class RffEncodeFunction(torch.autograd.Function):
    """The frozen projection b gets no gradient (reference: requires_grad=False)."""

    @staticmethod
    def forward(ctx, x, b):
        x2 = _rowmajor(x.reshape(-1, x.shape[-1])).contiguous()
        ctx.save_for_backward(x2, b)
        ctx.shape = x.shape
        return rff_encode_forward(x2, b).reshape(*x.shape[:-1], 2 * b.shape[0])

    @staticmethod
    def backward(ctx, d_out):
        x2, b = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None
        dx = rff_encode_backward_input(x2, b, d_out.reshape(x2.shape[0], -1))
        return dx.reshape(ctx.shape), None


def rff_encode(x, b):
    """Differentiable with respect to x (RffEncodeFunction)."""
    return RffEncodeFunction.apply(x, b)


def rff_forward_supported(dim_in: int, hidden: int, n_frequencies: int, n_layers: int, dim_out: int) -> bool:
    return bool(_lib.load().mri_rff_forward_supported(dim_in, hidden, n_frequencies, n_layers, dim_out))


_rff_ws = {}


def _rff_check(what, x, b, weights, vectors=(), matrices=(), per_layer=None, flat=None, extra=()):
    """(n, dim_in, hidden, n_layers) of an RffNet call, held to _check_stack: b (n_frequencies, dim_in), the first
    Linear on the 2 n_frequencies encoded features, one (n, hidden) buffer per hidden Linear in each list of
    `per_layer`, n values in each tensor of `flat`."""
    n, dim_in = x.shape
    n_layers, hidden = len(weights), weights[0].shape[0]
    if b.dim() != 2 or b.shape[1] != dim_in:
        raise ValueError(f"{what}: b is (n_frequencies, dim_in = {dim_in}), got {tuple(b.shape)}")
    want = [(hidden, 2 * b.shape[0])] + [(hidden, hidden)] * (n_layers - 2) + [(1, hidden)]
    _check_stack(what, weights, want, vectors, matrices, buffers=(n, hidden, n_layers - 1, per_layer or {}),
                 flat=(n, flat or {}), extra=[b] + list(extra))
    return n, dim_in, hidden, n_layers


def rff_forward(x, b, weights, biases, y=None):
    """y (n, 1) = RffNet(x), ReLU behind every Linear, in one persistent kernel (csrc/rff.hip): the encoding lives in
    two LDS images, nothing (n, hidden)-sized is written.  weights / biases: the decoder's Linears, the head last."""
    _gpu(x, b, y, *weights, *biases)
    x = _rowmajor(x).contiguous()
    y = _outputs("rff_forward", x, y)
    n, dim_in, hidden, n_layers = _rff_check("rff_forward", x, b, weights, [biases], extra=[y])
    ws = _grow_scratch(_rff_ws, x.device, _lib.load().mri_rff_forward_workspace_bytes(hidden, n_layers))
    _lib.call("mri_rff_forward", _ptr(x), n, dim_in, hidden, b.shape[0], n_layers, _ptr(b), _ptr_array(weights),
              _ptr_array(biases), _ptr(y), _ptr(ws), ws.numel() * 4, _stream())
    return y


def rff_gradient_supported(dim_in: int, hidden: int, n_frequencies: int, n_layers: int, dim_out: int) -> bool:
    return bool(_lib.load().mri_rff_gradient_supported(dim_in, hidden, n_frequencies, n_layers, dim_out))


def rff_gradient(x, b, weights, biases, y=None, dydx=None):
    """(y (n, 1), dydx (n, dim_in)) = RffNet(x) and its gradient with respect to x, dydx[i, d] = dy[i] / dx[i, d], in one
    persistent kernel (csrc/rff.hip): the value and the tangents of a point travel the Linears together, four rows per
    point in each of the two LDS images (eight for dim_in = 4); nothing (n, hidden)-sized is written.  y is
    rff_forward's bit for bit.  Parameters as rff_forward."""
    _gpu(x, b, y, dydx, *weights, *biases)
    x = _rowmajor(x).contiguous()
    y, dydx = _outputs("rff_gradient", x, y, dydx)
    n, dim_in, hidden, n_layers = _rff_check("rff_gradient", x, b, weights, [biases], extra=[y, dydx])
    ws = _grow_scratch(_rff_ws, x.device, _lib.load().mri_rff_gradient_workspace_bytes(hidden, n_layers))
    _lib.call("mri_rff_gradient", _ptr(x), n, dim_in, hidden, b.shape[0], n_layers, _ptr(b), _ptr_array(weights),
              _ptr_array(biases), _ptr(y), _ptr(dydx), _ptr(ws), ws.numel() * 4, _stream())
    return y, dydx


def rff_train_supported(dim_in: int, hidden: int, n_frequencies: int, n_layers: int, dim_out: int) -> bool:
    return bool(_lib.load().mri_rff_train_supported(dim_in, hidden, n_frequencies, n_layers, dim_out))


def rff_train_workspace(n: int, hidden: int, n_layers: int, device) -> torch.Tensor:
    """Scratch of rff_forward_loss and rff_backward for batches of up to n rows (partial sums, split weights)."""
    need = _lib.load().mri_rff_backward_workspace_bytes(max(int(n), 1), hidden, n_layers)
    if need < 0:
        raise ValueError(f"fused RFF step: hidden {hidden} x {n_layers} Linears is not supported")
    return torch.empty((need + 3) // 4, dtype=torch.float32, device=device)


_rff_train_ws = {}


def _rff_train_scratch(device, n, hidden, n_layers, ws):
    if ws is not None:  # the caller's own (FusedStep's, one per batch size): the library checks its size
        _gpu(ws)
        return ws
    # (need < 0: the library refuses the shape with its reason)
    return _grow_scratch(_rff_train_ws, device,
                         _lib.load().mri_rff_backward_workspace_bytes(max(int(n), 1), hidden, n_layers))


def rff_forward_loss(x, target, b, weights, biases, act, y, dy, loss_out, n_total=None, grad_divisor: float = 1.0,
                     ws=None):
    """Training forward of an RffNet with mse_loss(y, target) in the same kernel (mri_rff_forward_loss,
    include/mri_inr.h): act [n_layers - 1] x (n, hidden) receive the hidden activations, dy (n, 1) receives dLoss / dp
    (the head's ReLU applied), loss_out is ADDED to.  Follow with rff_backward(x, dy, ...)."""
    _gpu(x, target, b, y, dy, loss_out, ws, *weights, *biases, *act)
    x = _rowmajor(x).contiguous()
    target = target.reshape(-1).contiguous()
    n, dim_in, hidden, n_layers = _rff_check("rff_forward_loss", x, b, weights, [biases], per_layer=dict(act=act),
                                             flat=dict(target=target, y=y, dy=dy))
    if target.dtype != torch.float32 or loss_out.dtype != torch.float32 or loss_out.numel() < 1:
        raise ValueError("rff_forward_loss needs a float32 target and a float32 loss_out of one element")
    ws = _rff_train_scratch(x.device, n, hidden, n_layers, ws)
    _lib.call("mri_rff_forward_loss", _ptr(x), _ptr(target), n, n if n_total is None else n_total, dim_in, hidden,
              b.shape[0], n_layers, _ptr(b), _ptr_array(weights), _ptr_array(biases), float(grad_divisor),
              _ptr_array(act), _ptr(y), _ptr(dy), _ptr(loss_out), _ptr(ws), ws.numel() * 4, _stream())
    return y


def rff_backward(x, dy, b, weights, act, dz, d_weights, d_biases, ws=None):
    """Backward of rff_forward_loss from dy = dLoss / dp (mri_rff_backward): one chain kernel, a slab reduction, one
    weight-gradient kernel per Linear.  act: what the forward stored; dz [n_layers - 1] x (n, hidden): scratch.
    Gradients are ADDED to d_weights / d_biases (one per Linear, the head last).  b gets none: it is frozen."""
    _gpu(x, dy, b, ws, *weights, *act, *dz, *d_weights, *d_biases)
    x = _rowmajor(x).contiguous()
    n, dim_in, hidden, n_layers = _rff_check("rff_backward", x, b, weights, [d_biases], [d_weights],
                                             per_layer=dict(act=act, dz=dz), flat=dict(dy=dy))
    ws = _rff_train_scratch(x.device, n, hidden, n_layers, ws)
    _lib.call("mri_rff_backward", _ptr(x), _ptr(dy), n, dim_in, hidden, b.shape[0], n_layers, _ptr(b),
              _ptr_array(weights), _ptr_array(act), _ptr_array(dz), _ptr_array(d_weights), _ptr_array(d_biases),
              _ptr(ws), ws.numel() * 4, _stream())


# --------------------------------------------------------------------------- real Gabor layers (GaborNet)
def _gabor_pair(what, u, s):
    if u.shape != s.shape or u.dim() < 1 or u.dtype != torch.float32 or s.dtype != torch.float32:
        raise ValueError(f"{what}: u and s are float32 tensors of one shape, got {tuple(u.shape)} and {tuple(s.shape)}")
    hidden = u.shape[-1]
    return u.reshape(-1, hidden).contiguous(), s.reshape(-1, hidden).contiguous(), hidden


def gabor_activation_forward(u, s, w0: float, c: float, out=None):
    """out = cos(w0 u) exp(-(c s)^2) elementwise (csrc/gabor.hip); u, s (..., hidden)."""
    _gpu(u, s, out)
    u2, s2, hidden = _gabor_pair("gabor_activation", u, s)
    if out is None:
        out = torch.empty_like(u2)
    if out.numel() != u2.numel() or not out.is_contiguous() or out.dtype != torch.float32:
        raise ValueError("gabor_activation: out is a contiguous float32 tensor of u's size")
    _lib.call("mri_gabor_activation", _ptr(u2), _ptr(s2), u2.shape[0], hidden, float(w0), float(c), _ptr(out), _stream())
    return out.reshape(u.shape)


def gabor_activation_backward(u, s, g, w0: float, c: float):
    """(du, ds) of gabor_activation_forward from the gradient g of its output."""
    _gpu(u, s, g)
    u2, s2, hidden = _gabor_pair("gabor_activation_backward", u, s)
    if g.shape != u.shape or g.dtype != torch.float32:
        raise ValueError(f"gabor_activation_backward: g has u's shape {tuple(u.shape)}, got {tuple(g.shape)}")
    g2 = g.reshape(-1, hidden).contiguous()
    du, ds = torch.empty_like(u2), torch.empty_like(u2)
    _lib.call("mri_gabor_activation_backward", _ptr(u2), _ptr(s2), _ptr(g2), u2.shape[0], hidden, float(w0), float(c),
              _ptr(du), _ptr(ds), _stream())
    return du.reshape(u.shape), ds.reshape(u.shape)


class GaborActivationFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, s, w0, c):
        ctx.save_for_backward(u, s)
        ctx.w0, ctx.c = w0, c
        return gabor_activation_forward(u, s, w0, c)

    @staticmethod
    def backward(ctx, g):
        u, s = ctx.saved_tensors
        du, ds = gabor_activation_backward(u, s, g.contiguous(), ctx.w0, ctx.c)
        return du, ds, None, None


def gabor_activation(u, s, w0: float, c: float):
    """cos(w0 u) exp(-(c s)^2), differentiable with respect to u and s (GaborActivationFunction)."""
    return GaborActivationFunction.apply(u, s, float(w0), float(c))


def gabor_forward_supported(dim_in: int, hidden: int, n_layers: int, dim_out: int) -> bool:
    return bool(_lib.load().mri_gabor_forward_supported(dim_in, hidden, n_layers, dim_out))


_gabor_ws = {}


def _gabor_check(what, x, freq_weights, freq_biases, scale_weights, scale_biases, outputs):
    """(n, dim_in, hidden, n_layers) of an inference call.  The library sees pointers only: a mismatched shape would be
    read out of bounds on the device."""
    if x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError(f"{what}: x is float32 (n, dim_in), got {x.dtype} {tuple(x.shape)}")
    n, dim_in = x.shape
    n_layers = len(freq_weights)
    if len(scale_weights) != n_layers:
        raise ValueError(f"{what}: a freqs and a scale Linear per layer")
    hidden = freq_weights[0].shape[0] if n_layers else 0
    want = [(hidden, dim_in)] + [(hidden, hidden)] * (n_layers - 2) + [(1, hidden)]
    _check_stack(what, freq_weights, want, [freq_biases], label="freqs Linear", extra=outputs)
    _check_stack(what, scale_weights, want, [scale_biases], label="scale Linear")
    return n, dim_in, hidden, n_layers


def gabor_forward(x, freq_weights, freq_biases, scale_weights, scale_biases, w0: float, c: float, y=None):
    """y (n, 1) = GaborNet(x) in one persistent kernel (csrc/gabor.hip): every layer cos(w0 freqs(a)) exp(-(c scale(a))^2),
    the head included; nothing (n, hidden)-sized is written.  The four lists hold the layers' parameters, the head last."""
    _gpu(x, y, *freq_weights, *freq_biases, *scale_weights, *scale_biases)
    x = _rowmajor(x).contiguous()
    y = _outputs("gabor_forward", x, y)
    n, dim_in, hidden, n_layers = _gabor_check("gabor_forward", x, freq_weights, freq_biases, scale_weights,
                                               scale_biases, [y])
    ws = _grow_scratch(_gabor_ws, x.device, _lib.load().mri_gabor_forward_workspace_bytes(hidden, n_layers))
    _lib.call("mri_gabor_forward", _ptr(x), n, dim_in, hidden, n_layers, _ptr_array(freq_weights),
              _ptr_array(freq_biases), _ptr_array(scale_weights), _ptr_array(scale_biases), float(w0), float(c), _ptr(y),
              _ptr(ws), ws.numel() * 4, _stream())
    return y


# --------------------------------------------------------------------------- fused tiny MLP
def tiny_mlp_supported(k_in: int, hidden: int, dim_out: int) -> bool:
    return bool(_lib.load().mri_tiny_mlp_supported(k_in, hidden, dim_out))


_mlp_workspace = {}


def _tiny_workspace(k_in, hidden, n, device):
    return _grow_scratch(_mlp_workspace, device, _lib.load().mri_tiny_mlp_workspace_bytes(k_in, hidden, n))


def tiny_mlp_forward(x_fm, params, y=None):
    """y (n, 1) = MLP(x) for feature-major x (k_in, n); params = [(w1,b1),(w2,b2),(w3,b3)]."""
    (w1, b1), (w2, b2), (w3, b3) = params
    _gpu(x_fm, w1, b1, w2, b2, w3, b3, y)
    k_in, n = x_fm.shape
    if y is None:
        y = torch.empty((n, 1), device=x_fm.device, dtype=torch.float32)
    _lib.call("mri_tiny_mlp_forward", _ptr(x_fm), n, k_in, w1.shape[0], _ptr(w1), _ptr(b1),
              _ptr(w2), _ptr(b2), _ptr(w3), _ptr(b3), _ptr(y), _stream())
    return y


def tiny_mlp_dx_absmax_supported(k_in: int, hidden: int) -> bool:
    """Can tiny_mlp_train report max |d_x| per pair of feature rows (dx_absmax=)?"""
    return bool(_lib.load().mri_tiny_mlp_dx_absmax_supported(int(k_in), int(hidden)))


def tiny_mlp_train(x_fm, target, params, grads, loss_out, d_x=None, y=None,
                   grad_divisor: float = 1.0, overwrite: bool = False, dx_absmax=None):
    """Forward + MSE + backward of the tiny MLP in one kernel; grads accumulate (or are
    overwritten, together with loss_out, when overwrite=True).  `dx_absmax` (k_in / 2 zeroed floats
    on the device) receives max |d_x| per pair of feature rows (hashgrid_backward's level_absmax)."""
    (w1, b1), (w2, b2), (w3, b3) = params
    (g1, gb1), (g2, gb2), (g3, gb3) = grads
    _gpu(x_fm, target, w1, b1, w2, b2, w3, b3, g1, gb1, g2, gb2, g3, gb3, loss_out, d_x, y)
    k_in, n = x_fm.shape
    ws = _tiny_workspace(k_in, w1.shape[0], n, x_fm.device)
    if dx_absmax is not None:
        _gpu(dx_absmax)
        if dx_absmax.numel() < (k_in + 1) // 2 or dx_absmax.dtype != torch.float32:
            raise ValueError("dx_absmax: one float32 per pair of feature rows")
        _lib.call("mri_tiny_mlp_train_dx_absmax", _ptr(x_fm), _ptr(target), n, k_in, w1.shape[0],
                  _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(w3), _ptr(b3), float(grad_divisor),
                  _ptr(g1), _ptr(gb1), _ptr(g2), _ptr(gb2), _ptr(g3), _ptr(gb3), _ptr(d_x),
                  _ptr(loss_out), _ptr(y), 1 if overwrite else 0, _ptr(dx_absmax), _ptr(ws),
                  ws.numel() * 4, _stream())
        return loss_out
    _lib.call("mri_tiny_mlp_train_overwrite" if overwrite else "mri_tiny_mlp_train", _ptr(x_fm),
              _ptr(target), n, k_in, w1.shape[0], _ptr(w1),
              _ptr(b1), _ptr(w2), _ptr(b2), _ptr(w3), _ptr(b3), float(grad_divisor), _ptr(g1),
              _ptr(gb1), _ptr(g2), _ptr(gb2), _ptr(g3), _ptr(gb3), _ptr(d_x), _ptr(loss_out),
              _ptr(y), _ptr(ws), ws.numel() * 4, _stream())
    return loss_out


def hash_tiny_mlp_supported(desc: GridDesc, hidden: int) -> bool:
    """Is there a one-kernel form of encoder + decoder step for this grid and decoder width?"""
    return bool(_lib.load().mri_hash_tiny_mlp_supported(C.byref(desc), int(hidden)))


def hash_tiny_mlp_train(desc: GridDesc, table, coords, target, params, grads, loss_out, d_enc,
                        y=None, grad_divisor: float = 1.0, overwrite: bool = False):
    """hashgrid_forward + tiny_mlp_train in one kernel (mri_hash_tiny_mlp_train): the decoder looks the
    features up itself; `d_enc` (2 L, ld >= n) feature-major receives dLoss / d features."""
    (w1, b1), (w2, b2), (w3, b3) = params
    (g1, gb1), (g2, gb2), (g3, gb3) = grads
    _gpu(table, coords, target, w1, b1, w2, b2, w3, b3, g1, gb1, g2, gb2, g3, gb3, loss_out, d_enc, y)
    coords = _rowmajor(coords).contiguous()
    n = coords.shape[0]
    k_in = 2 * desc.n_levels
    if d_enc is not None and (d_enc.shape[0] != k_in or d_enc.stride(1) != 1 or d_enc.shape[1] < n):
        raise ValueError("d_enc must be a feature-major (2 L, >= n) block")
    ws = _tiny_workspace(k_in, w1.shape[0], n, coords.device)
    _lib.call("mri_hash_tiny_mlp_train", C.byref(desc), _ptr(table), _ptr(coords), _ptr(target), n,
              w1.shape[0], _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(w3), _ptr(b3),
              float(grad_divisor), _ptr(g1), _ptr(gb1), _ptr(g2), _ptr(gb2), _ptr(g3), _ptr(gb3),
              _ptr(d_enc), d_enc.stride(0) if d_enc is not None else n, _ptr(loss_out), _ptr(y),
              1 if overwrite else 0, _ptr(ws), ws.numel() * 4, _stream())
    return loss_out


def tiny_mlp_train_slice(x_fm, target, col_offset: int, n: int, params, grads, loss_out, d_x,
                         grad_divisor: float = 1.0, overwrite: bool = False):
    """tiny_mlp_train for columns [col_offset, col_offset + n) of the feature-major batch block
    x_fm (k_in, n_total) and of d_x; the loss mean and gradient scale are those of the whole
    batch, so the slices of a batch add up to the whole-batch call."""
    (w1, b1), (w2, b2), (w3, b3) = params
    (g1, gb1), (g2, gb2), (g3, gb3) = grads
    _gpu(x_fm, target, w1, b1, w2, b2, w3, b3, g1, gb1, g2, gb2, g3, gb3, loss_out, d_x)
    k_in, n_total = x_fm.shape
    if col_offset < 0 or col_offset + n > n_total or target.numel() != n_total:
        raise ValueError("slice does not fit the batch")
    ws = _tiny_workspace(k_in, w1.shape[0], n, x_fm.device)
    at = lambda t: C.c_void_p(t.data_ptr() + 4 * col_offset)  # noqa: E731
    _lib.call("mri_tiny_mlp_train_slice", at(x_fm), n_total, at(target), n, n_total, k_in,
              w1.shape[0], _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(w3), _ptr(b3),
              float(grad_divisor), _ptr(g1), _ptr(gb1), _ptr(g2), _ptr(gb2), _ptr(g3), _ptr(gb3),
              at(d_x) if d_x is not None else None, _ptr(loss_out), None, 1 if overwrite else 0,
              _ptr(ws), ws.numel() * 4, _stream())
    return loss_out


# --------------------------------------------------------------------------- fused shallow decoder
SHALLOW_ACTIVATIONS = (ACT_IDENTITY, ACT_RELU, ACT_GELU)


def shallow_mlp_supported(k_in: int, hidden: int, dim_out: int, act_hidden: int, act_out: int) -> bool:
    """Is there a one-kernel form of k_in -> hidden -> dim_out with these two activation codes?"""
    return bool(_lib.load().mri_shallow_mlp_supported(int(k_in), int(hidden), int(dim_out), int(act_hidden),
                                                      int(act_out)))


_shallow_workspace_cache = {}


def _shallow_workspace(k_in, hidden, n, device):
    need = _lib.load().mri_shallow_mlp_workspace_bytes(k_in, hidden, n)
    if need < 0:
        raise ValueError(f"shallow decoder {k_in} -> {hidden} -> 1 is not supported")
    return _grow_scratch(_shallow_workspace_cache, device, need)


def shallow_mlp_forward(x_fm, params, activations, y=None):
    """y (n, 1) = act_out(act_hidden(x W1^T + b1) w2^T + b2) for feature-major x (k_in, n);
    params = [(w1, b1), (w2, b2)], activations = (act_hidden, act_out)."""
    (w1, b1), (w2, b2) = params
    _gpu(x_fm, w1, b1, w2, b2, y)
    k_in, n = x_fm.shape
    if y is None:
        y = torch.empty((n, 1), device=x_fm.device, dtype=torch.float32)
    _lib.call("mri_shallow_mlp_forward", _ptr(x_fm), n, k_in, w1.shape[0], _ptr(w1), _ptr(b1), _ptr(w2),
              _ptr(b2), int(activations[0]), int(activations[1]), _ptr(y), _stream())
    return y


def shallow_mlp_train(x_fm, target, params, activations, grads, loss_out, d_x=None, y=None,
                      grad_divisor: float = 1.0, overwrite: bool = False, n_total: Optional[int] = None, ws=None):
    """Forward + MSE + backward of the shallow decoder in one kernel; grads and loss_out accumulate (or are
    overwritten when overwrite=True).  `n_total`: the rows of the whole batch this call is a slice of."""
    (w1, b1), (w2, b2) = params
    (g1, gb1), (g2, gb2) = grads
    _gpu(x_fm, target, w1, b1, w2, b2, g1, gb1, g2, gb2, loss_out, d_x, y)
    k_in, n = x_fm.shape
    if not x_fm.is_contiguous() or (d_x is not None and not d_x.is_contiguous()):
        raise ValueError("shallow_mlp_train: x and d_x are contiguous feature-major (k_in, n) blocks")
    if target.numel() != n:
        raise ValueError(f"shallow_mlp_train: {target.numel()} targets for {n} rows")
    if not target.is_contiguous():
        target = target.contiguous()
    if ws is None:
        ws = _shallow_workspace(k_in, w1.shape[0], n, x_fm.device)
    _lib.call("mri_shallow_mlp_train", _ptr(x_fm), _ptr(target), n, n if n_total is None else int(n_total), k_in,
              w1.shape[0], _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), int(activations[0]), int(activations[1]),
              float(grad_divisor), _ptr(g1), _ptr(gb1), _ptr(g2), _ptr(gb2), _ptr(d_x), _ptr(loss_out), _ptr(y),
              1 if overwrite else 0, _ptr(ws), ws.numel() * 4, _stream())
    return loss_out


# ----------------------------------------------------------- lookup and decoder side by side
def tiny_mlp_round_rows(k_in: int, hidden: int, n: int) -> int:
    """Rows one round of the decoder kernel's workgroups reads (0: no overlapped form)."""
    return int(_lib.load().mri_tiny_mlp_round_rows(k_in, hidden, n))


def hashgrid_signal_blocks(desc: GridDesc, slice_rows: int) -> int:
    """What mri_hashgrid_forward_signal adds to a slice's counter (-1: unsupported grid)."""
    return int(_lib.load().mri_hashgrid_forward_signal_blocks(C.byref(desc), slice_rows))


def hashgrid_forward_signal(desc: GridDesc, x, table, out_fm, slice_rows: int, ready):
    """Feature-major lookup on the CURRENT stream that reports finished slices in `ready`
    (uint64 counters, one per slice of `slice_rows` coordinates, never reset by the library)."""
    _gpu(x, table, out_fm)
    x = _rowmajor(x).contiguous()
    n = x.shape[0]
    if out_fm.shape[0] != desc.n_levels * desc.n_features or out_fm.shape[1] < n \
            or not out_fm.is_contiguous():
        raise ValueError("out_fm must be a contiguous (L*F, >= n) block")
    if ready.dtype != torch.int64 or ready.numel() * slice_rows < n:
        raise ValueError("ready: one int64 counter per slice")
    _lib.call("mri_hashgrid_forward_signal", C.byref(desc), _ptr(x), n, _ptr(table), _ptr(out_fm),
              out_fm.shape[1], slice_rows, C.c_void_p(ready.data_ptr()), _stream())
    return out_fm


def tiny_mlp_train_overlapped(x_fm, target, params, grads, loss_out, d_x, ready, ready_target: int,
                              status, grad_divisor: float = 1.0, overwrite: bool = True):
    """tiny_mlp_train whose workgroups wait for the producer of x_fm (hashgrid_forward_signal,
    queued earlier on ANOTHER stream) slice by slice."""
    (w1, b1), (w2, b2), (w3, b3) = params
    (g1, gb1), (g2, gb2), (g3, gb3) = grads
    _gpu(x_fm, target, w1, b1, w2, b2, w3, b3, g1, gb1, g2, gb2, g3, gb3, loss_out, d_x)
    k_in, n = x_fm.shape
    ws = _tiny_workspace(k_in, w1.shape[0], n, x_fm.device)
    _lib.call("mri_tiny_mlp_train_overlapped", _ptr(x_fm), _ptr(target), n, k_in, w1.shape[0],
              _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(w3), _ptr(b3), float(grad_divisor),
              _ptr(g1), _ptr(gb1), _ptr(g2), _ptr(gb2), _ptr(g3), _ptr(gb3), _ptr(d_x),
              _ptr(loss_out), 1 if overwrite else 0, C.c_void_p(ready.data_ptr()),
              C.c_uint64(ready_target), C.c_void_p(status.data_ptr()), _ptr(ws), ws.numel() * 4,
              _stream())
    return loss_out


# --------------------------------------------------------------------------- fused SIREN chain
def siren_supported(dim_in: int, hidden: int, n_sine_layers: int, dim_out: int) -> bool:
    return bool(_lib.load().mri_siren_supported(dim_in, hidden, n_sine_layers, dim_out))


def _ptr_array(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def siren_forward(x, weights, biases, w0_first: float, w0: float, act=None, deriv=None, y=None):
    """y (n, 1) = SirenNet(x) in one persistent kernel (csrc/siren_chain.hip).  weights / biases:
    the sine layers' then the head's; act / deriv: per sine layer (n, hidden) buffers that receive
    sin(.) and w0 cos(.) for the backward pass (both None: inference, nothing but y is written)."""
    _gpu(x, y, *weights, *biases, *(act or []), *(deriv or []))
    x = _rowmajor(x).contiguous()
    n, dim_in = x.shape
    n_sine, hidden = len(weights) - 1, weights[0].shape[0]
    if y is None:
        y = torch.empty((n, 1), device=x.device, dtype=torch.float32)
    for t in list(weights) + list(biases) + list(act or []) + list(deriv or []):
        if not t.is_contiguous():
            raise ValueError("siren_forward needs contiguous parameters and buffers")
    if (act is None) != (deriv is None) or (act is not None and
                                            (len(act) != n_sine or len(deriv) != n_sine)):
        raise ValueError("act and deriv: one (n, hidden) buffer per sine layer, or both None")
    ws = _siren_scratch(x.device, max(n, 1), hidden, n_sine)  # holds the split weights
    _lib.call("mri_siren_forward", _ptr(x), n, dim_in, hidden, n_sine, _ptr_array(weights),
              _ptr_array(biases), float(w0_first), float(w0),
              _ptr_array(act) if act is not None else None,
              _ptr_array(deriv) if deriv is not None else None, _ptr(y), _ptr(ws), ws.numel() * 4,
              _stream())
    return y


_siren_workspace = {}


def _siren_scratch(device, n, hidden, n_sine):
    return _grow_scratch(_siren_workspace, device, _lib.load().mri_siren_backward_workspace_bytes(n, hidden, n_sine))


def siren_gradient_supported(dim_in: int, hidden: int, n_sine_layers: int, dim_out: int) -> bool:
    return bool(_lib.load().mri_siren_gradient_supported(dim_in, hidden, n_sine_layers, dim_out))


def siren_gradient(x, weights, biases, w0_first: float, w0: float, y=None, dydx=None):
    """(y (n, 1), dydx (n, dim_in)) = SirenNet(x) and its gradient with respect to x, dydx[i, d] = dy[i] / dx[i, d],
    in one persistent kernel (csrc/siren_gradient.hip): the value and the dim_in <= 4 tangents of a point travel the
    chain together (four image rows per point for dim_in <= 3, eight for dim_in = 4: a 4-D volume, time among the
    axes), nothing (n, hidden)-sized is written.  weights / biases: the sine layers' then the head's."""
    _gpu(x, y, dydx, *weights, *biases)
    x = _rowmajor(x).contiguous()
    n, dim_in = x.shape
    n_sine, hidden = len(weights) - 1, weights[0].shape[0]
    y, dydx = _outputs("siren_gradient", x, y, dydx)
    for t in list(weights) + list(biases) + [y, dydx]:
        if not t.is_contiguous():
            raise ValueError("siren_gradient needs contiguous parameters and buffers")
    ws = _siren_scratch(x.device, max(n, 1), hidden, n_sine)  # holds the split weights
    _lib.call("mri_siren_gradient", _ptr(x), n, dim_in, hidden, n_sine, _ptr_array(weights), _ptr_array(biases),
              float(w0_first), float(w0), _ptr(y), _ptr(dydx), _ptr(ws), ws.numel() * 4, _stream())
    return y, dydx


def _opt_ptr_array(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() if t is not None else None for t in tensors])


def siren_forward_loss(x, target, weights, biases, w0_first: float, w0: float, act, deriv, dz_last,
                       y, d_w_head, d_b_head, d_b_last, loss_out, grad_divisor: float = 1.0,
                       n_total=None):
    """Training forward of the fused SIREN chain with F.mse_loss and the head's backward in the
    same kernel (mri_siren_forward_loss, include/mri_inr.h).  act / deriv: per sine layer
    (n, hidden) buffers, the LAST layer's may be None (it stays on chip); dz_last (n, hidden)
    receives the gradient w.r.t. the last sine layer's pre-activation; d_w_head, d_b_head,
    d_b_last and loss_out are ADDED to.  Follow with siren_backward(..., head_done=True)."""
    _gpu(x, target, y, dz_last, d_w_head, d_b_head, d_b_last, loss_out, *weights, *biases,
         *[t for t in list(act) + list(deriv) if t is not None])
    x = _rowmajor(x).contiguous()
    n, dim_in = x.shape
    n_sine, hidden = len(weights) - 1, weights[0].shape[0]
    if len(act) != n_sine or len(deriv) != n_sine:
        raise ValueError("act and deriv: one entry per sine layer (the last may be None)")
    if target.numel() != n or not target.is_contiguous() or y.numel() != n or \
            dz_last.shape != (n, hidden):
        raise ValueError("siren_forward_loss: target / y (n, 1) contiguous, dz_last (n, hidden)")
    for t in list(weights) + list(biases) + [t for t in list(act) + list(deriv) if t is not None] + \
            [dz_last, y, d_w_head, d_b_head, d_b_last]:
        if not t.is_contiguous():
            raise ValueError("siren_forward_loss needs contiguous parameters and buffers")
    ws = _siren_scratch(x.device, n, hidden, n_sine)
    _lib.call("mri_siren_forward_loss", _ptr(x), _ptr(target), n, n if n_total is None else n_total,
              dim_in, hidden, n_sine, _ptr_array(weights), _ptr_array(biases), float(w0_first),
              float(w0), float(grad_divisor), _opt_ptr_array(act), _opt_ptr_array(deriv),
              _ptr(dz_last), _ptr(y), _ptr(d_w_head), _ptr(d_b_head), _ptr(d_b_last), _ptr(loss_out),
              _ptr(ws), ws.numel() * 4, _stream())
    return y


def siren_backward(x, dy, weights, act, deriv, dz, d_weights, d_biases, head_done: bool = False):
    """Gradients of the fused SIREN chain, ADDED to d_weights / d_biases (sine layers, then the
    head).  dy: (n, 1) loss gradient w.r.t. the prediction; act / deriv: what siren_forward
    stored; dz: per sine layer (n, hidden) scratch (dz[0] may be None).  head_done: the head's
    backward already ran in siren_forward_loss, which left its result in dz[-1] (dy and the last
    act / deriv are not read, and may be None)."""
    _gpu(x, dy, *weights, *[t for t in list(act) + list(deriv) + list(dz) if t is not None],
         *d_weights, *d_biases)
    x = _rowmajor(x).contiguous()
    n, dim_in = x.shape
    n_sine, hidden = len(weights) - 1, weights[0].shape[0]
    if not (len(act) == len(deriv) == len(dz) == n_sine and
            len(d_weights) == len(d_biases) == n_sine + 1):
        raise ValueError("siren_backward: one act / deriv / dz per sine layer, one gradient per layer")
    ws = _siren_scratch(x.device, n, hidden, n_sine)
    _lib.call("mri_siren_backward", _ptr(x), _ptr(dy), n, dim_in, hidden, n_sine,
              _ptr_array(weights), _opt_ptr_array(act), _opt_ptr_array(deriv), _opt_ptr_array(dz),
              _ptr_array(d_weights), _ptr_array(d_biases), 1 if head_done else 0, _ptr(ws),
              ws.numel() * 4, _stream())


# --------------------------------------------------------------------------- fused modulated SIREN chain
def modsiren_supported(dim_in: int, hidden: int, n_layers: int, dim_out: int) -> bool:
    return bool(_lib.load().mri_modsiren_supported(dim_in, hidden, n_layers, dim_out))


def modsiren_workspace(n: int, hidden: int, n_layers: int, device) -> torch.Tensor:
    """Scratch of the three modulated-SIREN calls for batches of up to n rows (partial sums, split weights)."""
    need = _lib.load().mri_modsiren_backward_workspace_bytes(max(int(n), 1), hidden, n_layers)
    if need < 0:
        raise ValueError(f"fused modulated SIREN: hidden {hidden} x {n_layers} layers is not supported")
    return torch.empty((need + 3) // 4, dtype=torch.float32, device=device)


_modsiren_ws = {}


def _modsiren_scratch(device, n, hidden, n_layers, ws, need=None):
    if ws is not None:  # the caller's own (FusedStep's, one per batch size): the library checks its size
        _gpu(ws)
        return ws
    if need is None:  # (the gradient call passes its own: the split weights alone, whatever n)
        need = _lib.load().mri_modsiren_backward_workspace_bytes(max(int(n), 1), hidden, n_layers)
    return _grow_scratch(_modsiren_ws, device, need)  # (need < 0: the library refuses the shape with its reason)


def _modsiren_check(what, n, hidden, n_layers, per_layer, params):
    """_check_stack of the per-layer (n, hidden) buffers and the parameters, the latter not held to shapes."""
    _check_stack(what, params, None, at_least=0, buffers=(n, hidden, n_layers, per_layer))


def modsiren_forward(x, siren_weights, siren_biases, mod_weights, mod_biases, w0_first: float, w0: float,
                     saved=None, y=None, ws=None):
    """y (n, 1) = ModulatedSirenNet(x) in one persistent kernel (csrc/modsiren.hip).  siren_weights / siren_biases:
    the SIREN layers' then the head's; mod_weights / mod_biases: the modulator's layers.  saved: None (inference:
    nothing but y is written) or a dict of four lists act / hid / dcos / sn of per-layer (n, hidden) buffers that
    receive a_l, h_l, h_l w_l cos(.) and sin(.) for modsiren_backward."""
    _gpu(x, y, *siren_weights, *siren_biases, *mod_weights, *mod_biases)
    x = _rowmajor(x).contiguous()
    n, dim_in = x.shape
    n_layers, hidden = len(mod_weights), mod_weights[0].shape[0]
    if len(siren_weights) != n_layers + 1 or len(siren_biases) != n_layers + 1 or len(mod_biases) != n_layers:
        raise ValueError("modsiren_forward: n_layers + 1 SIREN weights / biases (the head last), n_layers modulator's")
    if y is None:
        y = torch.empty((n, 1), device=x.device, dtype=torch.float32)
    _modsiren_check("modsiren_forward", n, hidden, n_layers, saved or {},
                    list(siren_weights) + list(siren_biases) + list(mod_weights) + list(mod_biases) + [y])
    if saved is not None:
        _gpu(*[t for k in ("act", "hid", "dcos", "sn") for t in saved[k]])
    ws = _modsiren_scratch(x.device, n, hidden, n_layers, ws)
    arrays = [_ptr_array(saved[k]) if saved is not None else None for k in ("act", "hid", "dcos", "sn")]
    _lib.call("mri_modsiren_forward", _ptr(x), n, dim_in, hidden, n_layers, _ptr_array(siren_weights),
              _ptr_array(siren_biases), _ptr_array(mod_weights), _ptr_array(mod_biases), float(w0_first), float(w0),
              *arrays, _ptr(y), _ptr(ws), ws.numel() * 4, _stream())
    return y


def modsiren_gradient_supported(dim_in: int, hidden: int, n_layers: int, dim_out: int) -> bool:
    return bool(_lib.load().mri_modsiren_gradient_supported(dim_in, hidden, n_layers, dim_out))


def modsiren_gradient(x, siren_weights, siren_biases, mod_weights, mod_biases, w0_first: float, w0: float,
                      y=None, dydx=None):
    """(y (n, 1), dydx (n, dim_in)) = ModulatedSirenNet(x) and its gradient with respect to x, dydx[i, d] =
    dy[i] / dx[i, d], in one persistent kernel (csrc/modsiren_gradient.hip): the value and the dim_in <= 3 tangents
    of a point travel both stacks together, four rows per point in each of the two LDS images; nothing
    (n, hidden)-sized is written.  Parameters as modsiren_forward."""
    _gpu(x, y, dydx, *siren_weights, *siren_biases, *mod_weights, *mod_biases)
    x = _rowmajor(x).contiguous()
    n, dim_in = x.shape
    n_layers, hidden = len(mod_weights), mod_weights[0].shape[0]
    if len(siren_weights) != n_layers + 1 or len(siren_biases) != n_layers + 1 or len(mod_biases) != n_layers:
        raise ValueError("modsiren_gradient: n_layers + 1 SIREN weights / biases (the head last), n_layers modulator's")
    y, dydx = _outputs("modsiren_gradient", x, y, dydx)
    _modsiren_check("modsiren_gradient", n, hidden, n_layers, {},
                    list(siren_weights) + list(siren_biases) + list(mod_weights) + list(mod_biases) + [y, dydx])
    ws = _modsiren_scratch(x.device, n, hidden, n_layers, None,  # holds the split weights
                           need=_lib.load().mri_modsiren_gradient_workspace_bytes(hidden, n_layers))
    _lib.call("mri_modsiren_gradient", _ptr(x), n, dim_in, hidden, n_layers, _ptr_array(siren_weights),
              _ptr_array(siren_biases), _ptr_array(mod_weights), _ptr_array(mod_biases), float(w0_first), float(w0),
              _ptr(y), _ptr(dydx), _ptr(ws), ws.numel() * 4, _stream())
    return y, dydx


def modsiren_forward_loss(x, target, siren_weights, siren_biases, mod_weights, mod_biases, w0_first: float,
                          w0: float, saved, y, dy, loss_out, grad_divisor: float = 1.0, n_total=None, ws=None):
    """Training forward of the fused modulated SIREN chain with F.mse_loss in the same kernel
    (mri_modsiren_forward_loss, include/mri_inr.h): dy (n, 1) receives dLoss / dy, loss_out is ADDED to.  Follow with
    modsiren_backward(x, dy, ...)."""
    _gpu(x, target, y, dy, loss_out, *siren_weights, *siren_biases, *mod_weights, *mod_biases,
         *[t for k in ("act", "hid", "dcos", "sn") for t in saved[k]])
    x = _rowmajor(x).contiguous()
    n, dim_in = x.shape
    n_layers, hidden = len(mod_weights), mod_weights[0].shape[0]
    if len(siren_weights) != n_layers + 1 or len(siren_biases) != n_layers + 1 or len(mod_biases) != n_layers:
        raise ValueError("modsiren_forward_loss: n_layers + 1 SIREN weights / biases, n_layers modulator's")
    if target.numel() != n or y.numel() != n or dy.numel() != n:
        raise ValueError("modsiren_forward_loss: target / y / dy hold n values")
    _modsiren_check("modsiren_forward_loss", n, hidden, n_layers, saved,
                    list(siren_weights) + list(siren_biases) + list(mod_weights) + list(mod_biases) + [target, y, dy])
    ws = _modsiren_scratch(x.device, n, hidden, n_layers, ws)
    _lib.call("mri_modsiren_forward_loss", _ptr(x), _ptr(target), n, n if n_total is None else n_total, dim_in,
              hidden, n_layers, _ptr_array(siren_weights), _ptr_array(siren_biases), _ptr_array(mod_weights),
              _ptr_array(mod_biases), float(w0_first), float(w0), float(grad_divisor),
              *[_ptr_array(saved[k]) for k in ("act", "hid", "dcos", "sn")], _ptr(y), _ptr(dy), _ptr(loss_out),
              _ptr(ws), ws.numel() * 4, _stream())
    return y


def modsiren_backward(x, dy, siren_weights, mod_weights, saved, dzs, dzm, d_siren_weights, d_siren_biases,
                      d_mod_weights, d_mod_biases, ws=None):
    """Gradients of the fused modulated SIREN chain, ADDED to the four gradient lists (SIREN layers then the head;
    the modulator's layers).  dy: (n, 1) loss gradient w.r.t. the prediction; saved: what the forward call stored;
    dzs / dzm: per layer (n, hidden) scratch ([0] may be None)."""
    _gpu(x, dy, *siren_weights, *mod_weights, *[t for k in ("act", "hid", "dcos", "sn") for t in saved[k]],
         *[t for t in list(dzs) + list(dzm) if t is not None], *d_siren_weights, *d_siren_biases, *d_mod_weights,
         *d_mod_biases)
    x = _rowmajor(x).contiguous()
    n, dim_in = x.shape
    n_layers, hidden = len(mod_weights), mod_weights[0].shape[0]
    if not (len(siren_weights) == len(d_siren_weights) == len(d_siren_biases) == n_layers + 1 and
            len(d_mod_weights) == len(d_mod_biases) == n_layers):
        raise ValueError("modsiren_backward: one gradient per parameter (n_layers + 1 SIREN, n_layers modulator)")
    if dy.numel() != n:
        raise ValueError("modsiren_backward: dy holds n values")
    _modsiren_check("modsiren_backward", n, hidden, n_layers, dict(saved, dzs=dzs, dzm=dzm),
                    list(siren_weights) + list(mod_weights) + list(d_siren_weights) + list(d_siren_biases) +
                    list(d_mod_weights) + list(d_mod_biases) + [dy])
    ws = _modsiren_scratch(x.device, n, hidden, n_layers, ws)
    _lib.call("mri_modsiren_backward", _ptr(x), _ptr(dy), n, dim_in, hidden, n_layers, _ptr_array(siren_weights),
              _ptr_array(mod_weights), *[_ptr_array(saved[k]) for k in ("act", "hid", "dcos", "sn")],
              _opt_ptr_array(dzs), _opt_ptr_array(dzm), _ptr_array(d_siren_weights), _ptr_array(d_siren_biases),
              _ptr_array(d_mod_weights), _ptr_array(d_mod_biases), _ptr(ws), ws.numel() * 4, _stream())


# --------------------------------------------------------------------------- loss / optimiser
def mse_loss(pred, target, loss_out, d_pred=None, grad_divisor: float = 1.0):
    """loss_out[0] += mean((pred - target)^2); d_pred = 2 (pred - target) / (N * divisor)."""
    _gpu(pred, target, loss_out, d_pred)
    if not (pred.is_contiguous() and target.is_contiguous()):
        raise ValueError("mse_loss needs contiguous tensors")
    if pred.numel() != target.numel():
        raise ValueError("pred and target differ in size")
    _lib.call("mri_mse_loss", _ptr(pred), _ptr(target), pred.numel(), float(grad_divisor),
              _ptr(loss_out), _ptr(d_pred), _stream())
    return loss_out


class MSELossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target):
        loss = torch.zeros(1, device=pred.device, dtype=torch.float32)
        d_pred = torch.empty_like(pred, memory_format=torch.contiguous_format)
        mse_loss(pred.contiguous(), target.contiguous(), loss, d_pred)
        ctx.save_for_backward(d_pred)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (d_pred,) = ctx.saved_tensors
        return d_pred * g, None


# --------------------------------------------------------------------------- PsfSirenNet's PSF
def _contiguous(*tensors):
    for t in tensors:
        if t is not None and not t.is_contiguous():
            raise ValueError("the PSF ops need contiguous tensors")


def psf_expand(x, offsets, out=None):
    """x_psf (n S, dim_in): row b S + k = x[b] + offsets[k] (mri_psf_expand); offsets (S, dim_in)."""
    _gpu(x, offsets, out)
    _contiguous(x, offsets, out)
    n, dim_in = x.shape
    S = offsets.shape[0]
    if offsets.shape[1] != dim_in:
        raise ValueError(f"offsets {tuple(offsets.shape)} do not match x {tuple(x.shape)}")
    if out is None:
        out = torch.empty((n * S, dim_in), device=x.device, dtype=torch.float32)
    elif out.shape != (n * S, dim_in):
        raise ValueError(f"out {tuple(out.shape)}: expected {(n * S, dim_in)}")
    _lib.call("mri_psf_expand", _ptr(x), n, dim_in, _ptr(offsets), S, _ptr(out), _stream())
    return out


def psf_reduce(x, S: int, w=None, out=None):
    """out (n, C)[b] = sum_k w_k x[b S + k] for x (n S, C); w (S,) or None for ones (mri_psf_reduce)."""
    _gpu(x, w, out)
    _contiguous(x, w, out)
    rows, C = x.shape
    if rows % S:
        raise ValueError(f"{rows} rows are not whole groups of S = {S}")
    if w is not None and w.numel() != S:
        raise ValueError(f"w has {w.numel()} values, S = {S}")
    n = rows // S
    if out is None:
        out = torch.empty((n, C), device=x.device, dtype=torch.float32)
    _lib.call("mri_psf_reduce", _ptr(x), n, S, C, _ptr(w), _ptr(out), _stream())
    return out


def psf_broadcast(g, S: int, w, scale: float = 1.0, out=None):
    """dz (n S, 1)[b S + k] = scale w_k g[b] for g (n, 1) (mri_psf_broadcast)."""
    _gpu(g, w, out)
    _contiguous(g, w, out)
    n = g.numel()
    if w.numel() != S:
        raise ValueError(f"w has {w.numel()} values, S = {S}")
    if out is None:
        out = torch.empty((n * S, 1), device=g.device, dtype=torch.float32)
    _lib.call("mri_psf_broadcast", _ptr(g), n, S, _ptr(w), float(scale), _ptr(out), _stream())
    return out


def psf_mse_loss(z, target, S: int, w, loss_out, zbar, dz=None, n_total=None, grad_divisor: float = 1.0):
    """Training loss of PsfSirenNet (mri_psf_mse_loss): zbar (n) = PSF-weighted sums of z (n S),
    loss_out[0] += sum (zbar - target)^2 / n_total, dz = w_k 2 (zbar_b - target_b) / (n_total divisor)."""
    _gpu(z, target, w, loss_out, zbar, dz)
    _contiguous(z, target, w, zbar, dz)
    n = target.numel()
    if z.numel() != n * S or zbar.numel() != n or (dz is not None and dz.numel() != n * S) or w.numel() != S:
        raise ValueError(f"psf_mse_loss: z / dz (n S), target / zbar (n), w (S) with n = {n}, S = {S}")
    _lib.call("mri_psf_mse_loss", _ptr(z), _ptr(target), n, n if n_total is None else int(n_total), S,
              _ptr(w), float(grad_divisor), _ptr(zbar), _ptr(loss_out), _ptr(dz), _stream())
    return loss_out


class PsfExpandFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, offsets):
        ctx.S = offsets.shape[0]
        return psf_expand(x.contiguous(), offsets.contiguous())

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None
        return psf_reduce(g.contiguous(), ctx.S), None


class PsfConvFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, w):
        w = w.detach().reshape(-1).contiguous()
        ctx.save_for_backward(w)
        return psf_reduce(z.contiguous().reshape(-1, 1), w.numel(), w)

    @staticmethod
    def backward(ctx, g):
        (w,) = ctx.saved_tensors
        return psf_broadcast(g.contiguous(), w.numel(), w), None


def psf_expand_ad(x, offsets):
    """Differentiable psf_expand (its backward sums the S rows of each target)."""
    return PsfExpandFunction.apply(x, offsets)


def psf_conv(z, w):
    """psf_conv(z.T).T of the reference: (n S, 1) -> (n, 1) with the fixed PSF weights w."""
    return PsfConvFunction.apply(z, w)


# --------------------------------------------------------------------------- BatchNorm1d + activation
_BN_ACTIVATIONS = (ACT_IDENTITY, ACT_RELU, ACT_GELU)


def bn_workspace_bytes(n: int, C: int) -> int:
    need = _lib.load().mri_bn_workspace_bytes(int(n), int(C))
    if need < 0:
        raise ValueError(f"BatchNorm kernels: n = {n}, C = {C} is not a supported shape (1 <= C <= 1024)")
    return need


def bn_workspace(n: int, C: int, device) -> torch.Tensor:
    """Scratch of bn_stats / bn_act_backward for a batch of n rows and C features (float64 chunk sums)."""
    return torch.empty((bn_workspace_bytes(n, C) + 7) // 8, dtype=torch.float64, device=device)


def _bn_matrix(t, C, what):
    if t.dim() != 2 or t.shape[1] != C or t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < C):
        raise ValueError(f"{what} {tuple(t.shape)} (strides {tuple(t.stride())}): expected (n, {C}) with unit "
                         "column stride")


def _bn_vectors(C, **vectors):
    for name, t in vectors.items():
        if t is not None and (t.numel() != C or not t.is_contiguous()):
            raise ValueError(f"{name} {tuple(t.shape)}: expected {C} contiguous values")


def _bn_workspace_arg(ws, n, C, device):
    if ws is None:
        return bn_workspace(n, C, device)
    if ws.numel() * ws.element_size() < bn_workspace_bytes(n, C):
        raise ValueError(f"BatchNorm workspace of {ws.numel() * ws.element_size()} bytes, "
                         f"{bn_workspace_bytes(n, C)} needed")
    return ws


def bn_stats(z, running_mean=None, running_var=None, num_batches_tracked=None, momentum: float = 0.1,
             eps: float = 1e-5, save=None, ws=None):
    """Batch statistics of z (n, C) and nn.BatchNorm1d's train() update of its buffers, in place
    (mri_bn_stats).  Returns save (2, C): batch mean and 1 / sqrt(biased var + eps)."""
    _gpu(z, running_mean, running_var, save)
    n, C = z.shape[0], z.shape[-1]
    _bn_matrix(z, C, "z")
    if n < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(z.shape)}")
    _bn_vectors(C, running_mean=running_mean, running_var=running_var)
    if num_batches_tracked is not None and (num_batches_tracked.dtype != torch.int64
                                            or not num_batches_tracked.is_cuda):
        raise TypeError("num_batches_tracked must be an int64 tensor on the GPU")
    if save is None:
        save = torch.empty((2, C), device=z.device, dtype=torch.float32)
    elif save.numel() != 2 * C or not save.is_contiguous():
        raise ValueError(f"save {tuple(save.shape)}: expected (2, {C}) contiguous")
    ws = _bn_workspace_arg(ws, n, C, z.device)
    _lib.call("mri_bn_stats", _ptr(z), z.stride(0), n, C, float(momentum), float(eps), _ptr(running_mean),
              _ptr(running_var), _ptr(num_batches_tracked), _ptr(save), _ptr(ws), ws.numel() * ws.element_size(),
              _stream())
    return save


def bn_act_forward(z, gamma, beta, activation=ACT_IDENTITY, save=None, running_mean=None, running_var=None,
                   eps: float = 1e-5, out=None):
    """y = act(gamma (z - mean) invstd + beta) (mri_bn_act_forward).  `save` (from bn_stats): the training
    form; else the eval form with the running statistics, which are not modified.  `out` may be z."""
    _gpu(z, gamma, beta, save, running_mean, running_var, out)
    n, C = z.shape[0], z.shape[-1]
    _bn_matrix(z, C, "z")
    if activation not in _BN_ACTIVATIONS:
        raise ValueError(f"activation code {activation}: identity, ReLU or GELU")
    if save is None and (running_mean is None or running_var is None):
        raise ValueError("bn_act_forward needs `save` (training) or running_mean and running_var (eval)")
    _bn_vectors(C, gamma=gamma, beta=beta, running_mean=running_mean, running_var=running_var)
    if save is not None and (save.numel() != 2 * C or not save.is_contiguous()):
        raise ValueError(f"save {tuple(save.shape)}: expected (2, {C}) contiguous")
    if out is None:
        out = torch.empty((n, C), device=z.device, dtype=torch.float32)
    _bn_matrix(out, C, "out")
    if out.shape[0] != n:
        raise ValueError(f"out has {out.shape[0]} rows, z {n}")
    _lib.call("mri_bn_act_forward", _ptr(z), z.stride(0), n, C, _ptr(save),
              None if save is not None else _ptr(running_mean), None if save is not None else _ptr(running_var),
              float(eps), _ptr(gamma), _ptr(beta), activation, _ptr(out), out.stride(0), _stream())
    return out


def bn_act_backward(dy, z, save, gamma, beta, d_gamma, d_beta, activation=ACT_IDENTITY, dz=None,
                    overwrite: bool = False, ws=None):
    """Backward of bn_act_forward's training form (mri_bn_act_backward): returns dz (default: in place of
    dy); d_gamma / d_beta are added to, or written with `overwrite`."""
    _gpu(dy, z, save, gamma, beta, d_gamma, d_beta, dz)
    n, C = z.shape[0], z.shape[-1]
    _bn_matrix(z, C, "z")
    _bn_matrix(dy, C, "dy")
    if dy.shape[0] != n:
        raise ValueError(f"dy has {dy.shape[0]} rows, z {n}")
    if n < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(z.shape)}")
    if activation not in _BN_ACTIVATIONS:
        raise ValueError(f"activation code {activation}: identity, ReLU or GELU")
    _bn_vectors(C, gamma=gamma, beta=beta, d_gamma=d_gamma, d_beta=d_beta)
    if save.numel() != 2 * C or not save.is_contiguous():
        raise ValueError(f"save {tuple(save.shape)}: expected (2, {C}) contiguous")
    if dz is None:
        dz = dy
    _bn_matrix(dz, C, "dz")
    if dz.shape[0] != n:
        raise ValueError(f"dz has {dz.shape[0]} rows, z {n}")
    ws = _bn_workspace_arg(ws, n, C, z.device)
    _lib.call("mri_bn_act_backward", _ptr(dy), dy.stride(0), _ptr(z), z.stride(0), n, C, _ptr(save), _ptr(gamma),
              _ptr(beta), activation, _ptr(dz), dz.stride(0), _ptr(d_gamma), _ptr(d_beta), 1 if overwrite else 0,
              _ptr(ws), ws.numel() * ws.element_size(), _stream())
    return dz


def adam_step(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step,
              grad_scale: float = 1.0):
    _gpu(param, grad, exp_avg, exp_avg_sq)
    _lib.call("mri_adam_step", _ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq),
              param.numel(), float(lr), float(beta1), float(beta2), float(eps), int(step),
              float(grad_scale), _stream())


# --------------------------------------------------------------------------- batch producer
def sample_indices(seed: int, first: int, lo: int, hi: int, n: int, out=None, device="cuda"):
    if out is None:
        out = torch.empty(n, device=device, dtype=torch.int64)
    _gpu(out)
    _lib.call("mri_sample_indices", C.c_uint64(seed & (2 ** 64 - 1)), first, lo, hi, n, _ptr(out),
              _stream())
    return out


def gather_batch(idx, shape: Sequence[int], axes: torch.Tensor, axis_offset: Sequence[int],
                 volume: Optional[torch.Tensor], coords=None, target=None):
    _gpu(idx, axes, volume, coords, target)
    n, dim = idx.numel(), len(shape)
    if coords is None:
        coords = torch.empty((n, dim), device=idx.device, dtype=torch.float32)
    if target is None and volume is not None:
        target = torch.empty((n, 1), device=idx.device, dtype=torch.float32)
    shp = (C.c_int64 * dim)(*[int(s) for s in shape])
    off = (C.c_int64 * dim)(*[int(o) for o in axis_offset])
    _lib.call("mri_gather_batch", _ptr(idx), n, dim, shp, _ptr(axes), off, _ptr(volume),
              _ptr(coords), _ptr(target), _stream())
    return coords, target
