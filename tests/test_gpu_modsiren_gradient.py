"""The fused modulated SIREN coordinate gradient (csrc/modsiren_gradient.hip: y and dy/dx of ModulatedSirenNet from one
walk of the two-image chain) on the GPU: against what the reference produced, against float64, and through every layer
above the kernel -- ops, `ModulatedSirenNet.forward_with_gradient(fused=True)`, `Trainer(fused_modulated=True)
.predict_with_gradient` and `launcher.py --fused_modulated --save_gradient`.

P = points per tile = image rows / 4: 16 at hidden 128, 32 at hidden 64; at most 256 workgroups walk the tiles
(include/mri_inr.h), so n = 256 P + 5 makes the persistent loop wrap and end in a partial tile.

ReLU kinks: a modulator pre-activation within rounding of zero makes two correct f32 evaluations differ by a whole term
-- in the gradient by a whole weight column --, so the float64 comparisons run on the rows test_gpu_modsiren.py
selected_rows keeps (every float64 pre-activation at least 1e-6 from zero, at most 3 % of the drawn rows dropped, the
float32 sign pattern equal to the float64 one).  Nothing is excluded from a comparison afterwards.
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import REL_TOL, ROOT, assert_close, load_golden
from layout import Placer, ptr, variants
from test_gpu_modsiren import close_or_no_worse, load_net, selected_rows
from test_gpu_siren_gradient import autograd_through_forward, check_detached, check_dx_relation
from test_gpu_workspace import arr, hold
from oracle import detrand
from oracle import mlp as omlp

pytestmark = pytest.mark.gpu

POINTS = {128: 16, 64: 32}
GRID_BLOCKS = 256


@pytest.fixture(scope="module")
def amd():
    from mri_interpolation_amd import _lib, datamodules, models, ops, trainer
    assert torch.cuda.is_available(), "these tests need the GPU"
    _lib.load()
    return type("NS", (), dict(lib=_lib, h=_lib.load(), ops=ops, models=models, trainer=trainer, datamodules=datamodules))


def cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def sizes(hidden):
    p = POINTS[hidden]
    return [1, p - 1, p, p + 1, 2 * p + 3, GRID_BLOCKS * p + 5]


def reference(x, siren, mod, w0_first, w0, dtype):
    """(y (n), dydx (n, dim_in)) by autograd through oracle.mlp.modulated_siren_forward in `dtype` on the CPU (the rows
    are independent: the gradient of the sum is the per-row gradient)."""
    sp, mp = [[(w.to(dtype), b.to(dtype)) for w, b in ps] for ps in (siren, mod)]
    xg = x.to(dtype).clone().requires_grad_(True)
    y = omlp.modulated_siren_forward(xg, sp, mp, w0=w0, w0_initial=w0_first)
    g, = torch.autograd.grad(y.sum(), xg)
    return y.detach().reshape(-1), g


def kernel(amd, x, siren, mod, w0_first=30.0, w0=30.0):
    y, g = amd.ops.modsiren_gradient(x.cuda(), [w.cuda() for w, _ in siren], [b.cuda() for _, b in siren],
                                     [w.cuda() for w, _ in mod], [b.cuda() for _, b in mod], w0_first, w0)
    torch.cuda.synchronize()
    return y.cpu().reshape(-1), g.cpu()


@functools.lru_cache(maxsize=None)
def case(d, hidden, L, w0_first=30.0, w0=30.0):
    """The parameters of test_gpu_modsiren.ModRef's seed scheme, the rows selected_rows keeps of 16384 drawn ones (its
    assertions: at most 3 % dropped, equal ReLU signs in float32 and float64) and the float32 / float64 references on
    all of them.  Computed once per shape, shared, never modified; a test takes the first n rows."""
    seed = 9600 + hidden + L + 10 * d
    x, _, _, _ = selected_rows(d, hidden, L, seed)
    assert x.shape[0] >= sizes(hidden)[-1]
    siren, mod = omlp.siren_init(d, hidden, 1, L, seed), omlp.modulator_init(d, hidden, L, seed + 500)
    return (siren, mod, x, reference(x, siren, mod, w0_first, w0, torch.float32),
            reference(x, siren, mod, w0_first, w0, torch.float64))


# ---------------------------------------------------------------------------------------------- 1. the reference
@pytest.mark.parametrize("name", ["modsiren_grad_3d_6x128", "modsiren_grad_2d_3x64"])
def test_against_what_the_reference_produced(amd, name):
    fx = load_golden(name)
    m = fx.meta
    assert m["min_abs_preactivation"] >= 1e-6
    siren = omlp.siren_init(m["dim_in"], m["dim_hidden"], 1, m["n_layers"], m["seed"])
    mod = omlp.modulator_init(m["dim_in"], m["dim_hidden"], m["n_layers"], m["seed"] + 500)
    assert amd.ops.modsiren_gradient_supported(m["dim_in"], m["dim_hidden"], m["n_layers"], 1)
    y, dydx = kernel(amd, torch.from_numpy(fx["x"]), siren, mod, m["w0_initial"], m["w0"])
    assert y.shape == (fx["x"].shape[0],) and dydx.shape == fx["x"].shape
    assert_close(y.numpy().reshape(-1, 1), fx["pred"], REL_TOL, f"{name}: y")
    assert_close(dydx.numpy(), fx["dydx"], REL_TOL, f"{name}: dydx")
    check_dx_relation(fx, dydx.numpy(), f"{name}: dydx 2 (pred - y) / n against the fixture's dx")


# ---------------------------------------------------------------------------------------------- 2. float64
def float64_case(amd, d, hidden, L, w0_first=30.0, w0=30.0):
    assert amd.ops.modsiren_gradient_supported(d, hidden, L, 1)
    siren, mod, x_all, (y32, g32), (y64, g64) = case(d, hidden, L, w0_first, w0)
    for n in sizes(hidden):
        y, dydx = kernel(amd, x_all[:n], siren, mod, w0_first, w0)
        assert y.shape == (n,) and dydx.shape == (n, d)
        assert torch.isfinite(y).all() and torch.isfinite(dydx).all()
        tag = f"{d} -> {hidden} x {L} -> 1, n = {n}, w0 {w0_first:g} / {w0:g}"
        close_or_no_worse(y.numpy(), y32[:n].numpy(), y64[:n].numpy(), f"y ({tag})")
        close_or_no_worse(dydx.numpy(), g32[:n].numpy(), g64[:n].numpy(), f"dydx ({tag})")


@pytest.mark.parametrize("d,hidden,L", [(3, 128, 6), (2, 64, 3), (1, 64, 2), (3, 64, 8), (3, 128, 2)])
def test_against_float64(amd, d, hidden, L):
    """Within REL_TOL of float64 autograd, or no worse a float32 evaluation than float32 autograd on the CPU
    (test_gpu_modsiren.close_or_no_worse), at n = 1, P - 1, P, P + 1, 2 P + 3 and 256 P + 5."""
    float64_case(amd, d, hidden, L)


def test_against_float64_with_two_frequencies(amd):
    float64_case(amd, 3, 64, 3, w0_first=20.0, w0=30.0)


# ---------------------------------------------------------------------------------------------- 3. unused slots
@pytest.mark.parametrize("hidden", [64, 128])
@pytest.mark.parametrize("d", [1, 2])
def test_unused_slots_are_inert(amd, hidden, d):
    """The network embedded in dim_in = 3 with zero columns in Ws_0, Wm_0 and the tail of every Wm_l (and arbitrary extra
    coordinates) gives the same y and the same d gradient columns BITWISE: the sums over the axes run in axis order, so
    the embedded ones only gain terms x_d * 0 = +-0 at their end, and the rows of a point never mix in the H x H
    products.  The extra columns are exactly zero."""
    L, n = 3, 2 * POINTS[hidden] + 3
    siren, mod, x_all, _, _ = case(d, hidden, L)
    x = x_all[:n]
    y, dydx = kernel(amd, x, siren, mod)
    assert dydx.shape == (n, d)
    pad = torch.zeros(hidden, 3 - d)
    siren3 = [(torch.cat([siren[0][0], pad], dim=1), siren[0][1])] + list(siren[1:])
    mod3 = [(torch.cat([w, pad], dim=1), b) for w, b in mod]
    assert mod3[0][0].shape == (hidden, 3) and mod3[1][0].shape == (hidden, hidden + 3)
    extra = torch.from_numpy(detrand.uniform(n * (3 - d), 99, -1.0, 1.0).reshape(n, 3 - d).copy())
    y3, dydx3 = kernel(amd, torch.cat([x, extra], dim=1), siren3, mod3)
    assert dydx3.shape == (n, 3)
    assert torch.equal(y3, y) and torch.equal(dydx3[:, :d], dydx)
    assert (dydx3[:, d:] == 0).all()


# ---------------------------------------------------------------------------------------------- 4. the forward kernel, 5.
@pytest.mark.parametrize("d,hidden,L,n", [(3, 128, 6, 70001), (2, 64, 3, 2 * 32 + 3)])
def test_two_calls_agree_bitwise_and_y_is_the_forward_kernels(amd, d, hidden, L, n):
    siren = omlp.siren_init(d, hidden, 1, L, 41)
    mod = omlp.modulator_init(d, hidden, L, 541)
    x = torch.from_numpy(detrand.uniform(n * d, 42, -1.0, 1.0).reshape(n, d).copy())
    y1, g1 = kernel(amd, x, siren, mod)
    y2, g2 = kernel(amd, x, siren, mod)
    assert torch.isfinite(g1).all() and float(g1.abs().max()) > 0
    assert torch.equal(y1, y2) and torch.equal(g1, g2)
    fwd = amd.ops.modsiren_forward(x.cuda(), [w.cuda() for w, _ in siren], [b.cuda() for _, b in siren],
                                   [w.cuda() for w, _ in mod], [b.cuda() for _, b in mod], 30.0, 30.0)
    assert_close(y1.numpy(), fwd.cpu().numpy().reshape(-1), REL_TOL, "y against ops.modsiren_forward")


# ---------------------------------------------------------------------------------------------- 6. layout
@pytest.mark.parametrize("d,hidden,L", [(3, 128, 3), (2, 64, 3)])
def test_layout_guard_bands_and_rows_beyond_n(amd, d, hidden, L):
    """x, y and dydx at 4-byte aligned addresses that are not 16-byte aligned, n one short of a tile: the guard bands
    around y and dydx keep every bit, the rows >= n of both outputs are untouched, x is unchanged, and the results
    equal the aligned call's bitwise."""
    n, extra = 3 * POINTS[hidden] - 1, 5
    siren, mod, x_all, (y32, g32), (y64, g64) = case(d, hidden, L)
    x = x_all[:n]
    sw, sb = [w.cuda() for w, _ in siren], [b.cuda() for _, b in siren]
    mw, mb = [w.cuda() for w, _ in mod], [b.cuda() for _, b in mod]
    nan_bits = torch.full((1,), float("nan")).view(torch.int32).item()
    aligned = None
    for tag, layout in variants(dict(x=None, y=None, dydx=None), lds=False):
        p = Placer(layout, tag)
        xv = p.inp("x", x.reshape(-1))
        yv, gv = p.out("y", (n + extra,)), p.out("dydx", ((n + extra) * d,))
        if tag != "aligned":
            assert any(t.data_ptr() % 16 != 0 for t in (xv, yv, gv)) and all(t.data_ptr() % 4 == 0 for t in (xv, yv, gv))
        amd.ops.modsiren_gradient(xv.view(n, d), sw, sb, mw, mb, 30.0, 30.0, y=yv[:n], dydx=gv[:n * d].view(n, d))
        p.verify()
        assert (yv[n:].view(torch.int32) == nan_bits).all(), f"{tag}: y rows >= n were written"
        assert (gv[n * d:].view(torch.int32) == nan_bits).all(), f"{tag}: dydx rows >= n were written"
        got = yv[:n].cpu().clone(), gv[:n * d].cpu().clone().view(n, d)
        if aligned is None:
            aligned = got
            close_or_no_worse(got[0].numpy(), y32[:n].numpy(), y64[:n].numpy(), f"{tag}: y")
            close_or_no_worse(got[1].numpy(), g32[:n].numpy(), g64[:n].numpy(), f"{tag}: dydx")
        assert torch.equal(got[0], aligned[0]) and torch.equal(got[1], aligned[1]), f"{tag}: differs from the aligned call"


# ---------------------------------------------------------------------------------------------- 7. workspace
def workspace_entry(amd, d, hidden, L, n):
    siren, mod, x_all, f32, f64 = case(d, hidden, L)
    x = x_all[:n].cuda()
    sw, sb = [w.cuda() for w, _ in siren], [b.cuda() for _, b in siren]
    mw, mb = [w.cuda() for w, _ in mod], [b.cuda() for _, b in mod]
    st = amd.ops._stream()

    def launch(run, ws, nb):
        y, g = run.out((n,)), run.out((n, d))
        amd.lib.call("mri_modsiren_gradient", ptr(x), n, d, hidden, L, arr(sw), arr(sb), arr(mw), arr(mb), 30.0, 30.0,
                     ptr(y), ptr(g), ptr(ws), nb, st)
        return dict(y=y, dydx=g)

    refs = tuple(dict(y=r[0][:n], dydx=r[1][:n]) for r in (f32, f64))
    return launch, amd.h.mri_modsiren_gradient_workspace_bytes(hidden, L), refs


@pytest.mark.parametrize("d,hidden,L,n", [(2, 64, 3, 2 * 32 + 3), (3, 128, 2, 256 * 16 + 5)])
def test_workspace_contract(amd, d, hidden, L, n):
    """tests/test_gpu_workspace.py `hold`: exactly the reported size between guards, zero-filled, after a larger call
    of another shape on the same buffer, filled with 0x5A5A5A5A and 0xFFFFFFFF -- bitwise equal outputs --, and one
    byte short refused with the outputs and the guards untouched."""
    launch, need, (f32, f64) = workspace_entry(amd, d, hidden, L, n)
    assert need == 2 * (L - 1) * 6 * hidden * hidden
    big = workspace_entry(amd, 3, 192 - hidden, 6, 70)[:2]
    assert big[1] > need

    def judge(got):
        for name, value in got.items():
            close_or_no_worse(value.numpy().reshape(-1), f32[name].numpy().reshape(-1), f64[name].numpy().reshape(-1),
                              f"workspace, zero-filled: {name}")
    hold(f"modulated SIREN gradient {d} -> {hidden} x {L}, n = {n}:", launch, need, judge, big)


# ---------------------------------------------------------------------------------------------- 8. dispatch
def spy_on_kernel(amd, monkeypatch):
    calls, real = [], amd.ops.modsiren_gradient
    monkeypatch.setattr(amd.ops, "modsiren_gradient", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def test_dispatch_default_is_the_generic_body_and_fused_takes_the_kernel(amd, monkeypatch):
    d, hidden, L = 3, 64, 3
    _, _, x_all, _, _ = case(d, hidden, L)
    net = load_net(amd, dict(dim_in=d, dim_hidden=hidden, n_layers=L, seed=9600 + hidden + L + 10 * d))
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


@pytest.mark.parametrize("kw", [dict(dim_in=4), dict(dim_hidden=32), dict(use_bias=False), dict(final_activation=nn.Tanh())],
                         ids=["dim_in_4", "hidden_32", "no_bias", "tanh_head"])
def test_dispatch_fused_falls_back_to_the_generic_body(amd, monkeypatch, kw):
    torch.manual_seed(5)
    args = dict(dim_in=3, dim_hidden=64, dim_out=1, n_layers=3)
    args.update(kw)
    net = amd.models.ModulatedSirenNet(**args).cuda()
    d = args["dim_in"]
    x = cuda(detrand.uniform(67 * d, 3, -1.0, 1.0).reshape(67, d))
    calls = spy_on_kernel(amd, monkeypatch)
    want_y, want_g = autograd_through_forward(net, x)
    y, g = net.forward_with_gradient(x, fused=True)
    assert calls == []
    check_detached(net, y, g)
    assert torch.equal(y, want_y) and torch.equal(g, want_g)
    assert g.abs().max() > 0


def test_dispatch_dim_out_2_raises(amd):
    net = amd.models.ModulatedSirenNet(3, 64, 2, 3).cuda()
    with pytest.raises(ValueError, match="dim_out"):
        net.forward_with_gradient(torch.zeros(4, 3, device="cuda"), fused=True)
    with pytest.raises(ValueError, match="dim_out"):
        net.forward_with_gradient(torch.zeros(4, 3, device="cuda"))


# ---------------------------------------------------------------------------------------------- 9. trainer
def test_trainer_predict_with_gradient_is_the_per_batch_twin(amd, monkeypatch):
    torch.manual_seed(11)
    vol = amd.datamodules.phantom_volume((8, 8, 4)).cpu().numpy()
    ds = amd.datamodules.MriImage(volume=vol, norm_siren=True)
    loader = amd.datamodules.DeviceLoader(ds, 100, shuffle=False)  # 256 voxels: batches of 100, 100, 56
    net = amd.models.ModulatedSirenNet(dim_in=3, dim_hidden=64, dim_out=1, n_layers=3).cuda()
    batches = [x for x, _ in loader]
    calls = spy_on_kernel(amd, monkeypatch)
    ys, gs = amd.trainer.Trainer(max_epochs=1, max_steps=1, precision=32, log_every=0,
                                 fused_modulated=True).predict_with_gradient(net, loader)
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


# ---------------------------------------------------------------------------------------------- 10. launcher
def test_launcher_fused_modulated_save_gradient(amd, tmp_path):
    from mri_interpolation_amd import nifti
    out = tmp_path / "run"
    cmd = [sys.executable, os.path.join(ROOT, "launcher.py"), "--model_class", "ModulatedSirenNet", "--fused_modulated",
           "--save_gradient", "--synthetic", "16,16,8", "--dim_hidden", "64", "--n_layers", "3", "--epochs", "1",
           "--out_dir", str(out), "--log_every", "0"]
    r = subprocess.run(["timeout", "-k", "10", "300"] + cmd, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    grad = nifti.load(str(out / "gradient.nii.gz"))
    assert grad.shape == (16, 16, 8, 3) and grad.dtype == np.float32
    assert np.isfinite(grad).all() and np.abs(grad).max() > 0
    assert (out / "pred.nii.gz").exists()
