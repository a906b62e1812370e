"""GaborNet on the GPU (csrc/gabor.hip): the envelope and the Gabor product on exact arguments, the activation's
backward, the layer path against the reference's fixtures, the fused inference kernel, the dispatch of `predict_step`,
three Adam steps through Trainer, the launcher.

R = rows per tile of the fused kernel as built (TileShape<H, 64>): 128 at hidden 128, 256 at hidden 64; at most 256
workgroups walk the tiles (include/mri_inr.h), so n = 256 R + R + 3 takes the persistent loop past a workgroup's first
tile and ends in a partial one.

Every network-level comparison is the yardstick's (tests/yardstick.py, defaults: factor 2, floor 1e-6): the kernel is no
worse an f32 evaluation than the reference's, both measured against the op sequence in float64 on the same float32
inputs (tests/gabor_ref.py).  A Gabor stack amplifies rounding by about w0 per layer, so no fixed tolerance would be
right at both (w0, sigma) = (5, 1) and the class defaults (30, 10).

The device-math bounds (tests 1 and 2) are the promise of csrc/device_math.h, per element, with w0 = 1 so that the
cosine's argument is the float32 u itself and t = fl(fl(c s)^2) recomputed in numpy float32 as the kernel forms it:

    |out - cos64(u) exp64(-t)| <= exp64(-t) (2^-23 + 2^-22 + 2^-24) (1 + 2^-20) + 2^-126

2^-23: the cosine's absolute error (tests/exact_args.py); 2^-22: the envelope's 2 ulp; 2^-24: the product's rounding;
(1 + 2^-20) covers the second-order terms; 2^-126 is the absolute allowance where the result leaves the normal range.
"""
import functools

import numpy as np
import pytest
import torch

import exact_args
import gabor_ref
from conftest import load_golden, rel_err
from layout import Placer, ptr, variants
from test_gabor_cpu import net_from_fixture
from test_gpu_device_math import C_CYCLE, hidden_weight, same_bits
from test_gpu_workspace import arr, hold
from yardstick import AFTER_ADAM_MAX_FACTOR, assert_no_worse
from oracle import mlp as omlp

pytestmark = pytest.mark.gpu

ROWS = {128: 128, 64: 256}  # R: the built tile
GRID_BLOCKS = 256
REL = (2.0 ** -23 + 2.0 ** -22 + 2.0 ** -24) * (1.0 + 2.0 ** -20)
TINY = 2.0 ** -126


@pytest.fixture(scope="module")
def amd():
    from mri_interpolation_amd import _lib, models, ops
    assert torch.cuda.is_available(), "these tests need the GPU"
    _lib.load()
    return type("NS", (), dict(lib=_lib, h=_lib.load(), ops=ops, models=models))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy()


# ============================================================================================ 1. exact arguments
def scale_arguments(c, finite_only=False):
    """float32 s with |c s| over 200 values per binade from 2^-10 to 2^4, both signs, then 0, +inf, -inf, NaN."""
    parts = []
    for e in range(-10, 4):
        m = np.exp2(e) * (1.0 + np.arange(200) / 200.0) / c
        parts += [m, -m]
    parts.append(np.array([0.0] if finite_only else [0.0, np.inf, -np.inf, np.nan]))
    return np.concatenate(parts).astype(np.float32)


def envelope_t(s, c):
    """t = fl(fl(c s)^2) in float32, as gauss_envelope forms it."""
    with np.errstate(over="ignore", invalid="ignore"):
        sc = (np.float32(c) * s.astype(np.float32)).astype(np.float32)
        return (sc * sc).astype(np.float32)


def check_gabor(site, out, u32, s32, c):
    """Every element of `out` against cos64(u) exp64(-t) under the module docstring's bound; s = +-inf gives 0, NaN NaN."""
    assert out.dtype == np.float32 and out.shape == u32.shape == s32.shape
    t = envelope_t(s32, c).astype(np.float64)
    nan = np.isnan(s32)
    assert np.isnan(out[nan]).all(), f"{site}: the envelope of NaN is not NaN"
    inf = np.isinf(s32)
    assert (out[inf] == 0).all(), f"{site}: the envelope of +-inf is not 0"
    ok = ~nan
    with np.errstate(over="ignore", under="ignore"):
        e64 = np.exp(-np.where(ok, t, 0.0))
    want = np.cos(u32.astype(np.float64)) * e64
    err = np.abs(out.astype(np.float64) - want)
    bound = e64 * REL + TINY
    ratio = np.where(ok, err / bound, 0.0)
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print(f"{site}: max error / bound {ratio[at]:.3f} at u = {u32[at]!r}, s = {s32[at]!r}: kernel {out[at]!r}, float64 {want[at]!r}")
    assert not np.isnan(out[ok]).any(), f"{site}: NaN from finite arguments"
    assert ratio[at] <= 1.0, f"{site}: element {at}: error {err[at]:.3e} > bound {bound[at]:.3e} (u {u32[at]!r}, s {s32[at]!r})"


def paired(u, s, columns=3):
    """(n, columns) arrays: u in every column, s cycled with a different shift per column."""
    n = u.size
    idx = (np.arange(n)[:, None] + 1871 * np.arange(columns)[None, :]) % s.size
    return np.repeat(u[:, None], columns, 1).copy(), s[idx].copy()


@pytest.mark.parametrize("c", [1.0, 10.0])
def test_activation_on_exact_arguments(amd, c):
    u, s = paired(exact_args.sincos_arguments(), scale_arguments(c))
    assert np.isnan(s).any() and np.isinf(s).any() and (s == 0).any() and (np.abs(u) > 8192).any()
    out = host(amd.ops.gabor_activation_forward(dev(u), dev(s), 1.0, c))
    check_gabor(f"gabor_activation c = {c:g}", out, u, s, c)
    t = envelope_t(s, c)
    assert (out[(t == 0) & (u == 0)] == 1.0).all()


@pytest.mark.parametrize("c", [1.0, 10.0])
@pytest.mark.parametrize("hidden", [64, 128])
def test_fused_layers_on_exact_arguments(amd, hidden, c):
    """The same argument sets through the fused kernel: layer 0 on the VALU, one hidden layer on the matrix pipe, the head.
    Layer 0: x[:, 0] holds the cosine's set and x[:, 1] the envelope's, Wf_0[j] = (s_j, 0), Ws_0[j] = (0, s_j) with
    s_j = 1, 2, 1, 2 ..., biases 0: the arguments of element (i, j) are s_j x[i, 0] and s_j x[i, 1] exactly (the other
    product is an exact 0, so the non-finite envelope arguments stay with test 1: 0 * inf would reach the cosine).
    Hidden layer: rows of Wf_1 / Ws_1 with ONE nonzero power of two (tests/test_gpu_device_math.py hidden_weight), a
    bias on the scale side: the arguments are c_j a_0[i, i_j] (+ b_j), exact in the bf16x3 product.  Head: one-hot
    rows, so y[i] = gabor(a_1[i, jf], a_1[i, js]).  The kernel stores nothing but y, so the layers below the head are
    pinned through the activation kernel, which shares device_math.h with the fused kernel: fed the exact arguments
    stage by stage it must reproduce y BIT FOR BIT, and each of its stages is held to the float64 bound on every
    element.  Eight (jf, js) pairs spread the head over the waves' column blocks."""
    ops = amd.ops
    u_set, s_set = exact_args.sincos_arguments(), scale_arguments(c, finite_only=True)
    n = u_set.size
    x = np.stack([u_set, s_set[np.arange(n) % s_set.size]], axis=1).astype(np.float32)
    sj = (1.0 + (np.arange(hidden) % 2)).astype(np.float32)
    wf0, ws0 = np.zeros((hidden, 2), np.float32), np.zeros((hidden, 2), np.float32)
    wf0[:, 0], ws0[:, 1] = sj, sj[::-1]
    u0, s0 = x[:, :1] * wf0[None, :, 0], x[:, 1:] * ws0[None, :, 1]
    a0 = host(ops.gabor_activation_forward(dev(u0), dev(s0), 1.0, c))
    check_gabor(f"H {hidden} c {c:g} layer 0", a0, u0.astype(np.float32), s0.astype(np.float32), c)
    wf1, idx_f, cf = hidden_weight(hidden, hidden, 1, C_CYCLE)
    ws1, idx_s, cs = hidden_weight(hidden, hidden, 2, (1.0, 0.25, 4.0, 2.0 ** -6, 16.0))
    bs1 = (gabor_ref.uniform((hidden,), 77 + hidden, -1.0, 1.0).numpy() / np.float32(c)).astype(np.float32)
    u1 = (a0[:, idx_f] * cf[None, :]).astype(np.float32)
    s1 = ((a0[:, idx_s] * cs[None, :]).astype(np.float32) + bs1[None, :]).astype(np.float32)
    a1 = host(ops.gabor_activation_forward(dev(u1), dev(s1), 1.0, c))
    check_gabor(f"H {hidden} c {c:g} hidden layer", a1, u1, s1, c)
    assert (np.abs(u1) > 8192).any() and (a1 != 0).mean() > 0.2
    zeros = torch.zeros(hidden, device="cuda")
    for k in range(8):
        jf, js = (13 * k + 1) % hidden, (29 * k + 7) % hidden
        whf, whs = np.zeros((1, hidden), np.float32), np.zeros((1, hidden), np.float32)
        whf[0, jf] = whs[0, js] = 1.0
        y = host(ops.gabor_forward(dev(x), [dev(wf0), dev(wf1), dev(whf)], [zeros, zeros, zeros[:1]],
                                   [dev(ws0), dev(ws1), dev(whs)], [zeros, dev(bs1), zeros[:1]], 1.0, c)).reshape(-1)
        uh, sh = a1[:, jf].copy(), a1[:, js].copy()
        want = host(ops.gabor_activation_forward(dev(uh), dev(sh), 1.0, c))
        assert same_bits(y, want), (f"H {hidden} c {c:g} head ({jf}, {js}): the fused kernel's y is not the activation "
                                    f"kernel's composition bit for bit ({int((y != want).sum())} rows differ)")
        check_gabor(f"H {hidden} c {c:g} head ({jf}, {js})", y, uh, sh, c)


# ============================================================================================ 2. activation backward
@pytest.mark.parametrize("c", [1.0, 2.0])
def test_activation_backward_on_exact_arguments(amd, c):
    """du = -g w0 sin(w0 u) e and ds = -2 c sigma cos(w0 u) e g against float64 autograd, w0 = 1, c a power of two, g a
    power of two per element, and s with 12 significant bits: sigma = c s and t = sigma^2 are then exact in float32 and
    float64 alike, so the float64 reference differentiates the very function the kernel evaluates.  The kernel's
    roundings: sin / cos 2^-23 absolute, the envelope 2^-22 relative, and ONE rounded product on each path behind the
    exact products by powers of two (du: (g sin) e; ds: two, (2 c sigma cos) and (. e)), so with e = exp64(-t)
        |du - du64| <= g (e (2^-23 + 2^-22 + 2^-24) (1 + 2^-20) + 2^-126)
        |ds - ds64| <= g 2 c |sigma| (e (2^-23 + 2^-22 + 2^-23) (1 + 2^-20) + 2^-126) + 2^-126
    (the last term: the rounding of a result below the normal range)."""
    u_set = exact_args.sincos_arguments()
    s_set = scale_arguments(c, finite_only=True).view(np.uint32) & np.uint32(0xFFFFF000)
    u, s = paired(u_set, s_set.view(np.float32))
    g = np.exp2(((np.arange(u.size) * 7) % 11 - 5).astype(np.float32)).reshape(u.shape).astype(np.float32)
    sigma = (np.float32(c) * s).astype(np.float64)
    assert ((sigma * sigma).astype(np.float32).astype(np.float64) == sigma * sigma).all(), "t is exact"
    du, ds = amd.ops.gabor_activation_backward(dev(u), dev(s), dev(g), 1.0, c)
    du, ds = host(du), host(ds)
    ug = torch.from_numpy(u).double().requires_grad_(True)
    sg = torch.from_numpy(s).double().requires_grad_(True)
    out = torch.cos(ug) * torch.exp(-((sg * c) ** 2))
    du64, ds64 = [t.numpy() for t in torch.autograd.grad((out * torch.from_numpy(g).double()).sum(), [ug, sg])]
    e = np.exp(-sigma * sigma)
    gd = g.astype(np.float64)
    bound_u = gd * (e * REL + TINY)
    bound_s = gd * 2 * c * np.abs(sigma) * (e * (2.0 ** -23 + 2.0 ** -22 + 2.0 ** -23) * (1 + 2.0 ** -20) + TINY) + TINY
    for name, got, want, bound in (("du", du, du64, bound_u), ("ds", ds, ds64, bound_s)):
        err = np.abs(got.astype(np.float64) - want)
        ratio = err / bound
        at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        print(f"{name} (c = {c:g}): max error / bound {ratio[at]:.3f} at u = {u[at]!r}, s = {s[at]!r}")
        assert np.isfinite(got).all() and ratio[at] <= 1.0, \
            f"{name}: element {at}: error {err[at]:.3e} > bound {bound[at]:.3e} (u {u[at]!r}, s {s[at]!r}, g {g[at]!r})"
    # through autograd: the Function hands the same two tensors back
    uc, sc = dev(u).requires_grad_(True), dev(s).requires_grad_(True)
    gu, gs = torch.autograd.grad(amd.ops.gabor_activation(uc, sc, 1.0, c), [uc, sc], dev(g))
    assert same_bits(host(gu), du) and same_bits(host(gs), ds)


# ============================================================================================ 3. layer path, fixtures
@pytest.mark.parametrize("name", ["gabor_2d_3x64", "gabor_3d_5x128"])
def test_layer_path_against_the_fixture_and_float64(amd, name):
    fx = load_golden(name)
    m = fx.meta
    assert m["reference_f32_vs_f64"] <= 5e-6
    net = net_from_fixture(fx).cuda()
    x, y = torch.from_numpy(fx["x"]), torch.from_numpy(fx["y"])
    pred64, loss64, dx64, grads64 = gabor_ref.step(x, y, gabor_ref.fixture_params(fx), m["w0"], m["sigma"])
    xc = x.cuda().requires_grad_(True)
    pred = net(xc)
    assert pred.requires_grad and pred.shape == (m["rows"], 1)
    dx, = torch.autograd.grad(pred.sum(), xc, retain_graph=True)
    loss = net.criterion(y.cuda(), pred)
    params = [t for l in net.layers for t in (l.freqs.weight, l.freqs.bias, l.scale.weight, l.scale.bias)]
    grads = torch.autograd.grad(loss, params)
    assert_no_worse(host(pred), fx["pred"], pred64.numpy(), f"{name}: pred")
    assert_no_worse(np.array([float(loss.detach())]), np.array([float(fx["loss"])]), np.array([float(loss64)]), f"{name}: loss")
    assert_no_worse(host(dx), fx["dx"], dx64.numpy(), f"{name}: dy/dx")
    keys = [f"g{k}_{i}" for i in range(m["n_layers"]) for k in ("wf", "bf", "ws", "bs")]
    for key, got, want64 in zip(keys, grads, grads64):
        assert_no_worse(host(got), fx[key], want64.numpy(), f"{name}: {key}")
    y_g, dydx = net.eval().forward_with_gradient(x.cuda())  # --save_gradient's route: the generic body
    assert_no_worse(host(dydx), fx["dx"], dx64.numpy(), f"{name}: forward_with_gradient")
    assert_no_worse(host(y_g), fx["pred"], pred64.numpy(), f"{name}: forward_with_gradient's y")
    with torch.no_grad():  # eval mode, no grad: the fused kernel
        assert_no_worse(host(net(x.cuda())), fx["pred"], pred64.numpy(), f"{name}: pred through the fused kernel")


# ============================================================================================ 4. fused inference
FUSED_CASES = [(1, 64, 2, 5.0, 1.0), (2, 64, 3, 5.0, 1.0), (3, 128, 3, 5.0, 1.0), (4, 128, 4, 5.0, 1.0),
               (3, 64, 8, 5.0, 1.0), (3, 128, 5, 30.0, 10.0)]


@functools.lru_cache(maxsize=None)
def fused_case(d, hidden, L, w0, c, n=None):
    """x, the parameters (tests/gabor_ref.py grid_params: the fixtures' weight grid) and the CPU's float32 and float64 y."""
    seed = 9100 + hidden + L + 10 * d
    n = 2 * ROWS[hidden] + 3 if n is None else n
    x = gabor_ref.uniform((n, d), seed + 5)
    params = gabor_ref.grid_params(d, hidden, L, seed)
    with torch.no_grad():
        y32 = gabor_ref.forward(x, params, w0, c, torch.float32).reshape(-1)
        y64 = gabor_ref.forward(x, params, w0, c, torch.float64).reshape(-1)
    return x, params, y32, y64


def device_params(params):
    return tuple([p[k].cuda() for p in params] for k in range(4))


def layer_path(amd, x, fw, fb, sw, sb, w0, c):
    h = x
    for wf, bf, ws, bs in zip(fw, fb, sw, sb):
        h = amd.ops.gabor_activation_forward(amd.ops.linear_act(h, wf, bf), amd.ops.linear_act(h, ws, bs), w0, c)
    return h


@pytest.mark.parametrize("d,hidden,L,w0,c", FUSED_CASES)
def test_fused_forward_against_float64_and_the_layer_path(amd, d, hidden, L, w0, c):
    """n = 2 tiles + 3 rows.  At the class defaults (30, 10) the reference's own float32 forward is ~1e-3 from float64:
    only the yardstick can judge there."""
    assert amd.ops.gabor_forward_supported(d, hidden, L, 1)
    x, params, y32, y64 = fused_case(d, hidden, L, w0, c)
    fw, fb, sw, sb = device_params(params)
    xc = x.cuda()
    y = amd.ops.gabor_forward(xc, fw, fb, sw, sb, w0, c)
    assert y.shape == (x.shape[0], 1)
    y = host(y).reshape(-1)
    assert np.isfinite(y).all() and np.abs(y).max() <= 1.0
    tag = f"{d} -> {hidden} x {L} -> 1, (w0, sigma) = ({w0:g}, {c:g})"
    lp = host(layer_path(amd, xc, fw, fb, sw, sb, w0, c)).reshape(-1)
    for what, arr_ in (("fused", y), ("layer path", lp), ("CPU float32", y32.numpy())):
        print(f"{tag}: {what} {rel_err(arr_, y64.numpy())[0]:.2e} / {rel_err(arr_, y64.numpy())[1]:.2e} from float64")
    assert_no_worse(y, y32.numpy(), y64.numpy(), f"y ({tag})")
    assert_no_worse(y, lp, y64.numpy(), f"y against the layer path ({tag})")
    assert_no_worse(lp, y32.numpy(), y64.numpy(), f"the layer path's y ({tag})")


@pytest.mark.parametrize("hidden", [64, 128])
def test_fused_forward_unused_coordinate_is_inert(amd, hidden):
    """The dim_in = 2 network embedded in dim_in = 3 with a zero third column in both first-layer matrices (and arbitrary
    third coordinates) gives the same y bitwise: the sum over the axes runs in axis order and only gains x_2 * 0."""
    x, params, _, _ = fused_case(2, hidden, 3, 5.0, 1.0)
    fw, fb, sw, sb = device_params(params)
    y = amd.ops.gabor_forward(x.cuda(), fw, fb, sw, sb, 5.0, 1.0)
    pad = torch.zeros(hidden, 1, device="cuda")
    fw3, sw3 = [torch.cat([fw[0], pad], 1).contiguous()] + fw[1:], [torch.cat([sw[0], pad], 1).contiguous()] + sw[1:]
    x3 = torch.cat([x, gabor_ref.uniform((x.shape[0], 1), 99)], dim=1).cuda()
    y3 = amd.ops.gabor_forward(x3, fw3, fb, sw3, sb, 5.0, 1.0)
    assert torch.equal(y, y3) and float(y.abs().max()) > 0.1


def test_fused_forward_past_the_first_tile_and_one_tile_rows(amd):
    """n = 256 R + R + 3 rows at hidden 128 (R = 128: every workgroup's second tile, workgroup 0's partial third) against
    float64; two calls agree bitwise; rows 0 .. R-1 equal a one-tile call's bitwise (a row's result does not depend on
    the tile it rides in or on the grid)."""
    d, hidden, L, w0, c = 3, 128, 3, 5.0, 1.0
    R = ROWS[hidden]
    n = GRID_BLOCKS * R + R + 3
    x, params, y32, y64 = fused_case(d, hidden, L, w0, c, n)
    fw, fb, sw, sb = device_params(params)
    xc = x.cuda()
    y1 = amd.ops.gabor_forward(xc, fw, fb, sw, sb, w0, c).clone()
    y2 = amd.ops.gabor_forward(xc, fw, fb, sw, sb, w0, c)
    assert torch.equal(y1, y2) and torch.isfinite(y1).all()
    assert_no_worse(host(y1).reshape(-1), y32.numpy(), y64.numpy(), f"y (n = {n})")
    one = amd.ops.gabor_forward(xc[:R].contiguous(), fw, fb, sw, sb, w0, c)
    assert torch.equal(one, y1[:R]), "rows 0 .. R-1 differ from the one-tile call"
    last = amd.ops.gabor_forward(xc[n - 3:].contiguous(), fw, fb, sw, sb, w0, c)
    assert torch.equal(last, y1[n - 3:]), "the partial last tile differs from a call of its own"


@pytest.mark.parametrize("d,hidden,L", [(3, 128, 3), (2, 64, 3)])
def test_fused_forward_layout_guard_bands_and_rows_beyond_n(amd, d, hidden, L):
    n, extra = 2 * ROWS[hidden] - 1, 5
    x, params, y32, y64 = fused_case(d, hidden, L, 5.0, 1.0)
    x = x[:n]
    fw, fb, sw, sb = device_params(params)
    nan_bits = torch.full((1,), float("nan")).view(torch.int32).item()
    aligned = None
    for tag, layout in variants(dict(x=None, y=None), lds=False):
        p = Placer(layout, tag)
        xv, yv = p.inp("x", x.reshape(-1)), p.out("y", (n + extra,))
        if tag != "aligned":
            assert any(t.data_ptr() % 16 != 0 for t in (xv, yv)) and all(t.data_ptr() % 4 == 0 for t in (xv, yv))
        amd.ops.gabor_forward(xv.view(n, d), fw, fb, sw, sb, 5.0, 1.0, y=yv[:n])
        p.verify()
        assert (yv[n:].view(torch.int32) == nan_bits).all(), f"{tag}: y rows >= n were written"
        got = yv[:n].cpu().clone()
        if aligned is None:
            aligned = got
            assert_no_worse(got.numpy(), y32[:n].numpy(), y64[:n].numpy(), f"{tag}: y")
        assert torch.equal(got, aligned), f"{tag}: differs from the aligned call"


def workspace_entry(amd, d, hidden, L, n):
    x, params, y32, y64 = fused_case(d, hidden, L, 5.0, 1.0)
    assert n <= x.shape[0]
    xc = x[:n].cuda()
    fw, fb, sw, sb = device_params(params)
    st = amd.ops._stream()

    def launch(run, ws, nb):
        y = run.out((n,))
        amd.lib.call("mri_gabor_forward", ptr(xc), n, d, hidden, L, arr(fw), arr(fb), arr(sw), arr(sb), 5.0, 1.0, ptr(y),
                     ptr(ws), nb, st)
        return dict(y=y)

    return launch, amd.h.mri_gabor_forward_workspace_bytes(hidden, L), (y32[:n], y64[:n])


@pytest.mark.parametrize("d,hidden,L", [(2, 64, 3), (4, 128, 4)])
def test_fused_forward_workspace_contract(amd, d, hidden, L):
    """tests/test_gpu_workspace.py `hold`: exactly the reported size between guards, zero-filled, after a larger call of
    another shape on the same buffer, filled with two bit patterns (one of them NaNs) -- bitwise equal outputs --, and
    one byte short refused with the outputs and the guards untouched."""
    n = 2 * ROWS[hidden] + 3
    launch, need, (y32, y64) = workspace_entry(amd, d, hidden, L, n)
    assert need == 2 * (L - 2) * 6 * hidden * hidden
    big = workspace_entry(amd, 3, 64, 8, 70)[:2]
    if big[1] <= need:
        big = None

    def judge(got):
        assert_no_worse(got["y"].numpy().reshape(-1), y32.numpy(), y64.numpy(), "workspace, zero-filled: y")
    hold(f"fused Gabor forward {d} -> {hidden} x {L}, n = {n}:", launch, need, judge, big)


# ============================================================================================ 5. dispatch
def spy_on_kernel(amd, monkeypatch):
    calls, real = [], amd.ops.gabor_forward
    monkeypatch.setattr(amd.ops, "gabor_forward", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def test_predict_step_takes_the_fused_kernel_where_supported(amd, monkeypatch):
    torch.manual_seed(5)
    net = amd.models.GaborNet(dim_in=3, dim_hidden=64, dim_out=1, n_layers=3, sigma=1.0, w0=5.0,
                              fused_inference=True).cuda().eval()
    x = gabor_ref.uniform((300, 3), 31).cuda()
    calls = spy_on_kernel(amd, monkeypatch)
    with torch.no_grad():
        want = net.layers(x)
    assert calls == []
    y = net.predict_step((x, None), 0)
    assert calls == [1] and y.shape == (300, 1) and not y.requires_grad
    params = [tuple(t.detach().cpu() for t in (l.freqs.weight, l.freqs.bias, l.scale.weight, l.scale.bias)) for l in net.layers]
    with torch.no_grad():
        y64 = gabor_ref.forward(x.cpu(), params, 5.0, 1.0).numpy()
    assert_no_worse(host(y), host(want), y64, "predict_step against the layer path")
    with torch.no_grad():
        assert torch.equal(net(x), y) and calls == [1, 1]
    net(x)  # grad enabled: the differentiable layer path
    net.train()
    with torch.no_grad():
        net(x)
    assert calls == [1, 1]


@pytest.mark.parametrize("kw", [dict(dim_hidden=32), dict(dim_out=2), dict(fused_inference=False)],
                         ids=["hidden_32", "dim_out_2", "fused_inference_off"])
def test_predict_step_takes_the_layer_path_elsewhere(amd, monkeypatch, kw):
    torch.manual_seed(6)
    args = dict(dim_in=3, dim_hidden=64, dim_out=1, n_layers=3, sigma=1.0, w0=5.0, fused_inference=True)
    args.update(kw)
    net = amd.models.GaborNet(**args).cuda().eval()
    x = gabor_ref.uniform((67, 3), 32).cuda()
    calls = spy_on_kernel(amd, monkeypatch)
    assert net._inference_plan(x) is None
    with torch.no_grad():
        want = net.layers(x)
        y = net.predict_step((x, None), 0)
    assert calls == [] and torch.equal(y, want) and torch.isfinite(y).all() and y.shape == (67, args["dim_out"])


# ============================================================================================ 6. Adam, launcher
def test_e2e_gabor_adam_golden_through_trainer(amd):
    """Three Adam steps through Trainer.fit on the autograd path (training_step + autograd + the flat Adam kernel), under
    the yardstick's after-Adam factors: no worse than the reference's float32 parameters against the same steps in
    float64."""
    from mri_interpolation_amd import trainer
    fx = load_golden("e2e_gabor_adam")
    m = fx.meta
    net = net_from_fixture(fx).cuda()
    batches = [(torch.from_numpy(fx[f"x_{s}"]).cuda(), torch.from_numpy(fx[f"y_{s}"]).cuda()) for s in range(m["steps"])]
    p64 = [t.double().requires_grad_(True) for p in gabor_ref.fixture_params(fx) for t in p]
    opt64 = omlp.Adam([p.detach() for p in p64], lr=m["lr"])
    tr = trainer.Trainer(max_epochs=1, distributed=False)
    for s in range(m["steps"]):
        tr.fit(net, batches[s:s + 1])
        assert tr.fused is None, "GaborNet trains on the autograd path"
        x, y = torch.from_numpy(fx[f"x_{s}"]), torch.from_numpy(fx[f"y_{s}"])
        pred = gabor_ref.forward(x, [tuple(p64[4 * i:4 * i + 4]) for i in range(m["n_layers"])], m["w0"], m["sigma"])
        opt64.step(torch.autograd.grad(((pred - y.double()) ** 2).mean(), p64))
        for i, lay in enumerate(net.layers):
            for k, t in zip(("wf", "bf", "ws", "bs"), (lay.freqs.weight, lay.freqs.bias, lay.scale.weight, lay.scale.bias)):
                assert_no_worse(host(t), fx[f"{k}_{s}_{i}"], p64[4 * i + ("wf", "bf", "ws", "bs").index(k)].detach().numpy(),
                                f"{k}{i} step {s}", max_factor=AFTER_ADAM_MAX_FACTOR)
    assert tr.global_step == m["steps"] and net.optimizer.step_count == m["steps"]


def test_launcher_gabornet_save_gradient(amd, tmp_path, capsys):
    """--model_class GaborNet on the synthetic phantom for one epoch with --save_gradient: a finite prediction in the
    Gabor head's range and a finite gradient volume of the right shape, through the generic body."""
    import launcher
    from mri_interpolation_amd import nifti
    out = tmp_path / "run"
    launcher.main(["--model_class", "GaborNet", "--synthetic", "16,16,8", "--dim_hidden", "64", "--n_layers", "3",
                   "--sigma", "1.0", "--w0", "5", "--epochs", "1", "--batch_size", "512", "--save_gradient", "--out_dir", str(out),
                   "--log_every", "1"])
    printed = capsys.readouterr().out
    losses = [float(line.split("loss")[1]) for line in printed.splitlines() if line.startswith("epoch ") and "loss" in line]
    assert len(losses) == 4 and np.isfinite(losses).all()
    pred = nifti.load(str(out / "pred.nii.gz"))
    assert pred.shape == (16, 16, 8) and np.isfinite(pred).all() and np.abs(pred).max() <= 1.0
    grad = nifti.load(str(out / "gradient.nii.gz"))
    assert grad.shape == (16, 16, 8, 3) and grad.dtype == np.float32 and np.isfinite(grad).all() and np.abs(grad).max() > 0
    text = (out / "config.txt").read_text()  # (no new field: tests/test_gabor_cpu.py)
    assert "model_class : GaborNet" in text and "w0 : 5.0" in text and "sigma : 1.0" in text
