"""The fused RffNet coordinate gradient (csrc/rff.hip rff_gradient_kernel: y and dy/dx from one walk of the two-image
chain, forward mode) on the GPU: against what the reference produced, against float64 autograd, against the inference
kernel, and through every layer above the kernel -- ops, `RffNet.forward_with_gradient(fused=True)`,
`Trainer(fused_rff=True).predict_with_gradient` and `launcher.py --fused_rff --save_gradient`.

P = points per tile: image rows / 4 for dim_in <= 3 (16 at hidden 128, 32 at hidden 64), image rows / 8 for dim_in = 4
(8 / 16); at most 256 workgroups walk the tiles (include/mri_inr.h), so n = 256 P + 5 makes the persistent loop wrap
and end in a partial tile.

ReLU kinks: a pre-activation within rounding of zero makes two correct float32 evaluations of the gradient differ by a
whole term, so the float64 comparisons run on the rows test_gpu_rff_step.selected_rows keeps (its rule is restated
below for sigma = 10): chosen on the CPU from the float64 reference alone, every pre-activation at least 2e-5 from
zero, at most 3 % of the drawn rows dropped, the float32 sign pattern equal to the float64 one, the head live on 20 -
80 % of the rows -- all asserted there.  Nothing is excluded from a comparison afterwards.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import exact_args
from conftest import REL_TOL, ROOT, assert_close, load_golden
from layout import Placer, ptr, variants
from test_gpu_rff_step import DRAWN, MARGIN, RffRef, close_or_no_worse, he_init, load_net, selected_rows, uniform
from test_gpu_siren_gradient import autograd_through_forward, check_detached
from test_gpu_workspace import arr, hold

pytestmark = pytest.mark.gpu

GRID_BLOCKS = 256
TWO_PI = np.float32(2 * np.pi)  # fl32(2 pi): `2 * np.pi * v` on a float32 tensor


def points(d, hidden):
    """Points of a tile: four image rows each for dim_in <= 3, eight for dim_in = 4."""
    return {128: 64, 64: 128}[hidden] // (4 if d <= 3 else 8)


def sizes(d, hidden):
    p = points(d, hidden)
    return [1, p - 1, p, p + 1, 2 * p + 3, GRID_BLOCKS * p + 5]


@pytest.fixture(scope="module")
def amd():
    from mri_interpolation_amd import _lib, datamodules, models, ops, trainer
    assert torch.cuda.is_available(), "these tests need the GPU"
    return type("NS", (), dict(lib=_lib, h=_lib.load(), ops=ops, models=models, trainer=trainer, datamodules=datamodules))


def reference(ref, x):
    """(y (n), dydx (n, dim_in), the head's pre-activation (n)) of an RffRef by autograd in its dtype on the CPU (the
    rows are independent: the gradient of the sum is the per-row gradient)."""
    xg = x.to(ref.dtype).clone().requires_grad_(True)
    h = ref.encode(xg)
    for w, v in ref.params:
        pre = F.linear(h, w, v)
        h = torch.relu(pre)
    g, = torch.autograd.grad(h.sum(), xg)
    return h.detach().reshape(-1), g, pre.detach().reshape(-1)


def kernel(amd, x, b, params):
    y, g = amd.ops.rff_gradient(x.cuda(), b.cuda(), [w.cuda() for w, _ in params], [v.cuda() for _, v in params])
    torch.cuda.synchronize()
    return y.cpu().reshape(-1), g.cpu()


def selected_rows_sigma(d, H, L, sigma):
    """test_gpu_rff_step.selected_rows' rule, word for word, with b ~ N(0, sigma^2)."""
    seed = 9500 + H + L + 10 * d
    drawn = DRAWN[H]
    x = uniform((drawn, d), seed + 5)
    b, params = he_init(d, H, L, seed, sigma=sigma)
    pre = RffRef(b, params, torch.float64).preactivations(x)
    dot = pre[-1].reshape(-1) - params[-1][1].double()
    params = params[:-1] + [(params[-1][0], (-dot.median()).float().reshape(1))]
    r64, r32 = RffRef(b, params, torch.float64), RffRef(b, params, torch.float32)
    pre64 = r64.preactivations(x)
    live = float((pre64[-1] > 0).double().mean())
    assert 0.2 <= live <= 0.8, f"({d}, {H}, {L}), sigma {sigma:g}: {live:.3f} of the outputs are live"
    keep = torch.ones(drawn, dtype=torch.bool)
    for p in pre64:
        keep &= (p.abs() >= MARGIN).all(dim=1)
    dropped = 1.0 - float(keep.float().mean())
    print(f"({d}, {H}, {L}), sigma {sigma:g}: {100 * dropped:.3f} % of the drawn rows within {MARGIN} of a kink, "
          f"{live:.3f} live")
    assert dropped <= 0.03
    x = x[keep].contiguous()
    for a, c in zip(r64.preactivations(x), r32.preactivations(x)):
        assert torch.equal(a > 0, c > 0), "float32 and float64 disagree on a ReLU sign of a selected row"
    return x, b, params, r64, r32


@functools.lru_cache(maxsize=None)
def case(d, H, L, sigma=1.0):
    """b, the Linears, the selected rows and the float32 / float64 references (y, dydx, the head's pre-activation) on
    as many of them as the largest size takes.  Computed once per shape, shared, never modified; a test takes the
    first n rows."""
    if sigma == 1.0:
        x, _, b, params, r64, r32 = selected_rows(d, H, L)
    else:
        x, b, params, r64, r32 = selected_rows_sigma(d, H, L, sigma)
    top = sizes(d, H)[-1]
    assert x.shape[0] >= top
    x = x[:top].contiguous()
    return b, params, x, reference(r32, x), reference(r64, x)


# ---------------------------------------------------------------------------------------------- 1. the reference
@pytest.mark.parametrize("name", ["rff_2d_3x64", "rff_3d_6x128"])
def test_against_what_the_reference_produced(amd, name):
    fx = load_golden(name)
    m = fx.meta
    assert m["min_abs_preactivation"] >= 1e-5
    params = [(torch.from_numpy(fx[f"w_{i}"]), torch.from_numpy(fx[f"b_{i}"])) for i in range(m["n_layers"])]
    assert amd.ops.rff_gradient_supported(m["dim_in"], m["dim_hidden"], m["n_frequencies"], m["n_layers"], 1)
    y, dydx = kernel(amd, torch.from_numpy(fx["x"]), torch.from_numpy(fx["b"]), params)
    assert y.shape == (fx["x"].shape[0],) and dydx.shape == fx["x"].shape
    assert_close(y.numpy().reshape(-1, 1), fx["pred"], REL_TOL, f"{name}: y")
    assert_close(dydx.numpy(), fx["dx"], REL_TOL, f"{name}: dydx")


# ---------------------------------------------------------------------------------------------- 2. float64
SHAPES = [(3, 128, 6), (2, 64, 3), (1, 64, 2), (3, 64, 8), (3, 128, 2), (4, 64, 8), (4, 128, 3)]


def float64_case(amd, d, H, L, sigma):
    assert amd.ops.rff_gradient_supported(d, H, H, L, 1)
    b, params, x_all, (y32, g32, _), (y64, g64, _) = case(d, H, L, sigma)
    for n in sizes(d, H):
        y, dydx = kernel(amd, x_all[:n], b, params)
        assert y.shape == (n,) and dydx.shape == (n, d)
        assert torch.isfinite(y).all() and torch.isfinite(dydx).all()
        tag = f"{d} -> {H} x {L} -> 1, sigma {sigma:g}, n = {n}"
        close_or_no_worse(y.numpy(), y32[:n].numpy(), y64[:n].numpy(), f"y ({tag})")
        close_or_no_worse(dydx.numpy(), g32[:n].numpy(), g64[:n].numpy(), f"dydx ({tag})")


@pytest.mark.parametrize("d,H,L", SHAPES)
def test_against_float64(amd, d, H, L):
    """Within REL_TOL of float64 autograd, or no worse a float32 evaluation than float32 autograd on the CPU
    (close_or_no_worse), at n = 1, P - 1, P, P + 1, 2 P + 3 and 256 P + 5."""
    float64_case(amd, d, H, L, 1.0)


@pytest.mark.parametrize("d,H,L", [(3, 128, 6), (4, 64, 8)])
def test_against_float64_sigma_10(amd, d, H, L):
    float64_case(amd, d, H, L, 10.0)


# ---------------------------------------------------------------------------------------------- 3. exact zeros
@pytest.mark.parametrize("d,H,L", [(3, 128, 6), (4, 64, 8)])
def test_a_clamped_head_gives_exact_zeros(amd, d, H, L):
    """Where the float64 head pre-activation is below -2e-5 the head's ReLU clamps: y and every dydx entry are exactly
    0.  The case holds such rows and live ones."""
    b, params, x, _, (y64, g64, pre64) = case(d, H, L)
    dead = pre64 < -MARGIN
    assert bool(dead.any()) and bool((pre64 > MARGIN).any())
    y, dydx = kernel(amd, x, b, params)
    assert bool((y[dead] == 0).all()), "a clamped row's y is not exactly 0"
    assert bool((dydx[dead] == 0).all()), "a clamped row's gradient is not exactly 0"
    assert bool((y[~dead] > 0).all()) and bool((dydx[~dead].abs().sum(dim=1) > 0).all())


# ---------------------------------------------------------------------------------------------- 4. the inference kernel
@pytest.mark.parametrize("d,H,L,n", [(3, 128, 6, 70001), (2, 64, 3, 2 * 32 + 3), (4, 64, 3, 2 * 16 + 3)])
def test_y_is_the_inference_kernels_bitwise_and_two_calls_agree(amd, d, H, L, n):
    """The value rows are rff_forward_kernel's expression by expression (rff_phase, sincos_fast2, the chunk order,
    HeadDot) and the rows of an MFMA are independent: y equals ops.rff_forward's bit for bit."""
    b, params = he_init(d, H, L, 41, sigma=10.0)
    x = uniform((n, d), 42)
    # the head's bias moved by the median of its float64 pre-activation: about half of the rows live, half clamped
    centre = RffRef(b, params, torch.float64).preactivations(x)[-1].median()
    params = params[:-1] + [(params[-1][0], (params[-1][1].double() - centre).float())]
    y1, g1 = kernel(amd, x, b, params)
    y2, g2 = kernel(amd, x, b, params)
    assert torch.isfinite(g1).all() and float(g1.abs().max()) > 0 and float(y1.max()) > 0
    assert torch.equal(y1, y2) and torch.equal(g1, g2)
    fwd = amd.ops.rff_forward(x.cuda(), b.cuda(), [w.cuda() for w, _ in params], [v.cuda() for _, v in params])
    assert torch.equal(y1, fwd.cpu().reshape(-1)), "y differs from ops.rff_forward's"


# ---------------------------------------------------------------------------------------------- 5. unused slots
@pytest.mark.parametrize("H", [64, 128])
@pytest.mark.parametrize("d", [1, 2])
def test_unused_slots_are_inert(amd, H, d):
    """The network embedded in dim_in = 3 with zero columns of b (and arbitrary extra coordinates) gives the same y and
    the same d gradient columns BITWISE: the phase's FMA chain runs in axis order and only gains terms x_d * 0 at its
    end, and the rows of a point never mix in the products.  The extra columns are exactly zero."""
    L, n = 3, 2 * points(d, H) + 3
    b, params, x_all, _, _ = case(d, H, L)
    x = x_all[:n]
    y, dydx = kernel(amd, x, b, params)
    assert dydx.shape == (n, d) and float(dydx.abs().max()) > 0
    b3 = torch.cat([b, torch.zeros(H, 3 - d)], dim=1)
    x3 = torch.cat([x, uniform((n, 3 - d), 99)], dim=1)
    y3, dydx3 = kernel(amd, x3, b3, params)
    assert dydx3.shape == (n, 3)
    assert torch.equal(y3, y) and torch.equal(dydx3[:, :d], dydx)
    assert bool((dydx3[:, d:] == 0).all())


@pytest.mark.parametrize("H", [64, 128])
def test_the_eight_slot_form_is_the_four_slot_form(amd, H):
    """The dim_in = 3 network embedded in dim_in = 4 the same way: the eight-slot call against the four-slot call."""
    L, n = 3, 2 * points(3, H) + 3
    b, params, x_all, _, _ = case(3, H, L)
    x = x_all[:n]
    y, dydx = kernel(amd, x, b, params)
    b4 = torch.cat([b, torch.zeros(H, 1)], dim=1)
    x4 = torch.cat([x, uniform((n, 1), 98)], dim=1)
    y4, dydx4 = kernel(amd, x4, b4, params)
    assert dydx4.shape == (n, 4) and float(dydx.abs().max()) > 0
    assert torch.equal(y4, y) and torch.equal(dydx4[:, :3], dydx)
    assert bool((dydx4[:, 3] == 0).all())


# ---------------------------------------------------------------------------------------------- 6. exact arguments
@pytest.mark.parametrize("half", ["cos", "sin"])
def test_tangent_rows_on_exact_arguments(amd, half):
    """dim_in 1, H = F = 64, L = 2, b[0] = 1 and every other b = 0: u = fl32(fl32(2 pi) x) exactly.  One weight 1 on the
    cos (sin) column of frequency 0, beta_0[0] = 2, w_head[0] = 1, everything else 0: y = cos u + 2 (sin u + 2), always
    live, and dydx = -fl32(2 pi) sin u (+fl32(2 pi) cos u).  Against float64 of the float32 u: the project's 2e-7 on sine
    and cosine times 2 pi gives 1.26e-6, two float32 roundings at magnitude 2 pi add 0.75e-6, the bf16x3 products by 1
    and 0 add nothing: 2e-6 absolute on dydx, 5e-7 on y."""
    H = 64
    a = exact_args.sincos_arguments()
    a = a[np.abs(a) <= 1e6]
    big = np.exp2(np.linspace(13.0, np.log2(1e6), 400)).astype(np.float32) * np.where(np.arange(400) % 2, -1, 1)
    x = np.concatenate([a, big.astype(np.float32)]).astype(np.float32) / TWO_PI
    u = (TWO_PI * x).astype(np.float32).astype(np.float64)
    assert (np.abs(u) <= 8192).sum() > 4000 and ((np.abs(u) > 8192) & (np.abs(u) <= 1e6)).sum() > 500
    b = torch.zeros(H, 1)
    b[0, 0] = 1.0
    w0, beta0, wh = torch.zeros(H, 2 * H), torch.zeros(H), torch.zeros(1, H)
    w0[0, 0 if half == "cos" else H] = 1.0
    beta0[0], wh[0, 0] = 2.0, 1.0
    y, dydx = kernel(amd, torch.from_numpy(x).reshape(-1, 1), b, [(w0, beta0), (wh, torch.zeros(1))])
    want_y = (np.cos(u) if half == "cos" else np.sin(u)) + 2.0
    want_g = float(TWO_PI) * (-np.sin(u) if half == "cos" else np.cos(u))
    err_y = np.abs(y.numpy().astype(np.float64) - want_y).max()
    err_g = np.abs(dydx.numpy().astype(np.float64).reshape(-1) - want_g).max()
    print(f"{half} column: y {err_y:.3e}, dydx {err_g:.3e} from float64 on exact arguments")
    assert err_g <= 2e-6 and err_y <= 5e-7


# ---------------------------------------------------------------------------------------------- 7. layout
@pytest.mark.parametrize("d,H,L", [(3, 128, 3), (2, 64, 3), (4, 64, 3)])
def test_layout_guard_bands_and_rows_beyond_n(amd, d, H, L):
    """x, y and dydx at 4-byte aligned addresses that are not 16-byte aligned, n one short of a tile: the guard bands
    around y and dydx keep every bit, the rows >= n of both outputs are untouched, x is unchanged, and the results
    equal the aligned call's bitwise."""
    n, extra = 3 * points(d, H) - 1, 5
    b, params, x_all, (y32, g32, _), (y64, g64, _) = case(d, H, L)
    x = x_all[:n]
    bc, ws, bs = b.cuda(), [w.cuda() for w, _ in params], [v.cuda() for _, v in params]
    nan_bits = torch.full((1,), float("nan")).view(torch.int32).item()
    aligned = None
    for tag, layout in variants(dict(x=None, y=None, dydx=None), lds=False):
        p = Placer(layout, tag)
        xv = p.inp("x", x.reshape(-1))
        yv, gv = p.out("y", (n + extra,)), p.out("dydx", ((n + extra) * d,))
        if tag != "aligned":
            assert any(t.data_ptr() % 16 != 0 for t in (xv, yv, gv)) and all(t.data_ptr() % 4 == 0 for t in (xv, yv, gv))
        amd.ops.rff_gradient(xv.view(n, d), bc, ws, bs, y=yv[:n], dydx=gv[:n * d].view(n, d))
        p.verify()
        assert (yv[n:].view(torch.int32) == nan_bits).all(), f"{tag}: y rows >= n were written"
        assert (gv[n * d:].view(torch.int32) == nan_bits).all(), f"{tag}: dydx rows >= n were written"
        got = yv[:n].cpu().clone(), gv[:n * d].cpu().clone().view(n, d)
        if aligned is None:
            aligned = got
            close_or_no_worse(got[0].numpy(), y32[:n].numpy(), y64[:n].numpy(), f"{tag}: y")
            close_or_no_worse(got[1].numpy(), g32[:n].numpy(), g64[:n].numpy(), f"{tag}: dydx")
        assert torch.equal(got[0], aligned[0]) and torch.equal(got[1], aligned[1]), f"{tag}: differs from the aligned call"


# ---------------------------------------------------------------------------------------------- 8. workspace
def workspace_entry(amd, d, H, L, n):
    b, params, x_all, f32, f64 = case(d, H, L)
    x = x_all[:n].cuda()
    bc, ws_, bs = b.cuda(), [w.cuda() for w, _ in params], [v.cuda() for _, v in params]
    st = amd.ops._stream()

    def launch(run, ws, nb):
        y, g = run.out((n,)), run.out((n, d))
        amd.lib.call("mri_rff_gradient", ptr(x), n, d, H, H, L, ptr(bc), arr(ws_), arr(bs), ptr(y), ptr(g), ptr(ws),
                     nb, st)
        return dict(y=y, dydx=g)

    refs = tuple(dict(y=r[0][:n], dydx=r[1][:n]) for r in (f32, f64))
    return launch, amd.h.mri_rff_gradient_workspace_bytes(H, L), refs


@pytest.mark.parametrize("d,H,L,n", [(2, 64, 3, 2 * 32 + 3), (4, 128, 2, 256 * 8 + 5)])
def test_workspace_contract(amd, d, H, L, n):
    """tests/test_gpu_workspace.py `hold`: exactly the reported size between guards, zero-filled, after a larger call
    of another shape on the same buffer, filled with 0x5A5A5A5A and 0xFFFFFFFF -- bitwise equal outputs --, and one
    byte short refused with the outputs and the guards untouched."""
    launch, need, (f32, f64) = workspace_entry(amd, d, H, L, n)
    assert need == L * 6 * H * H
    big = workspace_entry(amd, 3, 128, 8, 70)[:2]  # the largest workspace of the supported set
    assert big[1] > need

    def judge(got):
        for name, value in got.items():
            close_or_no_worse(value.numpy().reshape(-1), f32[name].numpy().reshape(-1), f64[name].numpy().reshape(-1),
                              f"workspace, zero-filled: {name}")
    hold(f"RFF gradient {d} -> {H} x {L}, n = {n}:", launch, need, judge, big)


# ---------------------------------------------------------------------------------------------- 9. dispatch
def spy_on_kernel(amd, monkeypatch):
    calls, real = [], amd.ops.rff_gradient
    monkeypatch.setattr(amd.ops, "rff_gradient", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def test_dispatch_default_is_the_generic_body_and_fused_takes_the_kernel(amd, monkeypatch):
    d, H, L = 3, 64, 3
    b, params, x_all, _, _ = case(d, H, L)
    net = load_net(amd, d, H, L, b, params).eval()
    x = x_all[:131].cuda()  # rows clear of every kink
    calls = spy_on_kernel(amd, monkeypatch)
    want_y, want_g = autograd_through_forward(net, x)
    for kw in ({}, dict(fused=False)):
        y, g = net.forward_with_gradient(x, **kw)
        check_detached(net, y, g)
        assert torch.equal(y, want_y) and torch.equal(g, want_g), "the default is not autograd through forward"
    assert calls == []
    y, g = net.forward_with_gradient(x, fused=True)
    assert calls == [1], "fused=True on a supported net did not take the kernel (once)"
    check_detached(net, y, g)
    assert y.shape == (131, 1) and g.shape == (131, 3)
    assert_close(y.cpu().numpy(), want_y.cpu().numpy(), REL_TOL, "kernel y against the generic body")
    assert_close(g.cpu().numpy(), want_g.cpu().numpy(), REL_TOL, "kernel dydx against the generic body")


@pytest.mark.parametrize("kw", [dict(n_frequencies=32), dict(activation=nn.GELU), dict(dim_hidden=32, n_frequencies=32),
                                dict(dim_in=5), dict(fused_inference=False)],
                         ids=["F_ne_H", "gelu", "hidden_32", "dim_in_5", "fused_inference_off"])
def test_dispatch_fused_falls_back_to_the_generic_body(amd, monkeypatch, kw):
    torch.manual_seed(5)
    args = dict(dim_in=3, dim_hidden=64, dim_out=1, n_layers=3, n_frequencies=64, sigma=1.0)
    args.update(kw)
    net = amd.models.RffNet(**args).cuda().eval()
    d = args["dim_in"]
    x = uniform((67, d), 3).cuda()
    calls = spy_on_kernel(amd, monkeypatch)
    want_y, want_g = autograd_through_forward(net, x)
    y, g = net.forward_with_gradient(x, fused=True)
    assert calls == []
    check_detached(net, y, g)
    assert torch.equal(y, want_y) and torch.equal(g, want_g)
    assert y.shape == (67, 1) and g.shape == (67, d) and torch.isfinite(g).all()


def test_dispatch_dim_out_2_raises(amd):
    net = amd.models.RffNet(3, 64, 2, 3, n_frequencies=64).cuda()
    with pytest.raises(ValueError, match="dim_out"):
        net.forward_with_gradient(torch.zeros(4, 3, device="cuda"), fused=True)
    with pytest.raises(ValueError, match="dim_out"):
        net.forward_with_gradient(torch.zeros(4, 3, device="cuda"))


# ---------------------------------------------------------------------------------------------- 10. trainer
def test_trainer_predict_with_gradient_is_the_per_batch_twin(amd, monkeypatch):
    torch.manual_seed(11)
    vol = amd.datamodules.phantom_volume((8, 8, 4)).cpu().numpy()
    ds = amd.datamodules.MriImage(volume=vol)
    loader = amd.datamodules.DeviceLoader(ds, 100, shuffle=False)  # 256 voxels: batches of 100, 100, 56
    net = amd.models.RffNet(dim_in=3, dim_hidden=64, dim_out=1, n_layers=3, n_frequencies=64, sigma=1.0).cuda()
    batches = [x for x, _ in loader]
    calls = spy_on_kernel(amd, monkeypatch)
    ys, gs = amd.trainer.Trainer(max_epochs=1, max_steps=1, precision=32, log_every=0,
                                 fused_rff=True).predict_with_gradient(net, loader)
    assert len(calls) == 3
    assert [tuple(y.shape) for y in ys] == [(100, 1), (100, 1), (56, 1)]
    assert [tuple(g.shape) for g in gs] == [(100, 3), (100, 3), (56, 3)]
    for x, y, g in zip(batches, ys, gs):
        dy, dg = net.forward_with_gradient(x, fused=True)
        assert torch.equal(y, dy) and torch.equal(g, dg)
    del calls[:]
    ys, gs = amd.trainer.Trainer(max_epochs=1, max_steps=1, precision=32, log_every=0).predict_with_gradient(net, loader)
    assert calls == []
    for x, y, g in zip(batches, ys, gs):
        dy, dg = autograd_through_forward(net, x)
        assert torch.equal(y, dy) and torch.equal(g, dg)


# ---------------------------------------------------------------------------------------------- 11. launcher
@pytest.mark.parametrize("synthetic,shape", [("16,16,8", (16, 16, 8, 3)), ("8,8,4,5", (8, 8, 4, 5, 4))], ids=["3d", "4d"])
def test_launcher_fused_rff_save_gradient(amd, tmp_path, synthetic, shape):
    from mri_interpolation_amd import nifti
    out = tmp_path / "run"
    cmd = [sys.executable, os.path.join(ROOT, "launcher.py"), "--model_class", "RffNet", "--fused_rff", "--save_gradient",
           "--synthetic", synthetic, "--dim_hidden", "64", "--n_frequencies", "64", "--n_layers", "3", "--epochs", "1",
           "--out_dir", str(out), "--log_every", "0"]
    r = subprocess.run(["timeout", "-k", "10", "300"] + cmd, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    grad = nifti.load(str(out / "gradient.nii.gz"))
    assert grad.shape == shape and grad.dtype == np.float32
    assert np.isfinite(grad).all() and np.abs(grad).max() > 0
    assert (out / "pred.nii.gz").exists()
