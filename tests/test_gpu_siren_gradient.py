"""The fused SIREN coordinate gradient (csrc/siren_gradient.hip: y and dy/dx from one walk of the chain) on the GPU:
against what the reference produced, against float64, and through every layer above the kernel -- ops, the model
classes' `forward_with_gradient`, `Trainer.predict_with_gradient` and `launcher.py --save_gradient`.

P = points per tile = image rows / 4: 16, 32, 64 (and 64) at hidden 256, 128, 64 (and 32); at most 256 workgroups walk
the tiles (include/mri_inr.h), so n = 256 P + 5 makes the persistent loop wrap and end in a partial tile.
"""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import REL_TOL, assert_close, load_golden
from layout import Placer, variants
from yardstick import assert_no_worse
from oracle import detrand
from oracle import mlp as omlp

pytestmark = pytest.mark.gpu

POINTS = {256: 16, 128: 32, 64: 64, 32: 64}
GRID_BLOCKS = 256


@pytest.fixture(scope="module")
def amd():
    from mri_interpolation_amd import _lib, checkpoint, datamodules, models, ops, trainer
    assert torch.cuda.is_available(), "these tests need the GPU"
    _lib.load()
    return type("NS", (), dict(lib=_lib, ops=ops, models=models, trainer=trainer, datamodules=datamodules,
                               checkpoint=checkpoint))


def cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def reference(x, params, w0_first, w0, dtype):
    """(y (n), dydx (n, dim_in)) by autograd through oracle.mlp.siren_forward in `dtype` on the CPU (the rows are
    independent: the gradient of the sum is the per-row gradient)."""
    ps = [(w.to(dtype), b.to(dtype)) for w, b in params]
    xg = x.to(dtype).clone().requires_grad_(True)
    y = omlp.siren_forward(xg, ps, w0=w0, w0_initial=w0_first)
    g, = torch.autograd.grad(y.sum(), xg)
    return y.detach().reshape(-1), g


def kernel(amd, x, params, w0_first=30.0, w0=30.0):
    y, g = amd.ops.siren_gradient(x.cuda(), [w.cuda() for w, _ in params], [b.cuda() for _, b in params], w0_first, w0)
    torch.cuda.synchronize()
    return y.cpu().reshape(-1), g.cpu()


@functools.lru_cache(maxsize=None)
def case(hidden, dim_in, n_sine, n, w0_first=30.0, w0=30.0):
    """Parameters (oracle.mlp.siren_init), coordinates drawn by oracle.detrand in [-1, 1] with rows at exactly -1, 0
    and 1 among them, and the float32 / float64 references.  Computed once, shared, never modified."""
    params = omlp.siren_init(dim_in, hidden, 1, n_sine, 1000 + hidden + 10 * n_sine + dim_in, w0=w0)
    x = torch.from_numpy(detrand.uniform(n * dim_in, 7 * n + dim_in, -1.0, 1.0).reshape(n, dim_in).copy())
    for row, v in zip((n // 2, n - 1, 0), (-1.0, 0.0, 1.0)):  # (n = 1: the row ends at exactly 1)
        x[row] = v
    return params, x, reference(x, params, w0_first, w0, torch.float32), reference(x, params, w0_first, w0, torch.float64)


def load_siren(amd, fx, cls=None, **kw):
    m = fx.meta
    net = (cls or amd.models.SirenNet)(dim_in=m["dim_in"], dim_hidden=m["dim_hidden"], dim_out=1, n_layers=m["n_layers"], **kw)
    params = omlp.siren_init(m["dim_in"], m["dim_hidden"], 1, m["n_layers"], m["seed"])
    with torch.no_grad():
        for layer, (w, b) in zip(list(net.layers) + [net.last_layer], params):
            layer.weight.copy_(w)
            if layer.bias is not None:
                layer.bias.copy_(b)
    return net.cuda(), params


def check_dx_relation(fx, dydx, what):
    """The fixture's dx is the reference's own x.grad of its training_step loss mean((pred - y)^2):
    dx = dydx (.) 2 (pred - y) / n."""
    n = fx["x"].shape[0]
    scale = 2.0 * (fx["pred"].astype(np.float64) - fx["y"].astype(np.float64)) / n
    assert_close(np.asarray(dydx, dtype=np.float64) * scale, fx["dx"], REL_TOL, what)


# ---------------------------------------------------------------------------------------------- 1. the reference
@pytest.mark.parametrize("name", ["siren_3d_5x256", "siren_2d_3x64"])
def test_against_what_the_reference_produced(amd, name):
    fx = load_golden(name)
    m = fx.meta
    params = omlp.siren_init(m["dim_in"], m["dim_hidden"], 1, m["n_layers"], m["seed"])
    assert amd.ops.siren_gradient_supported(m["dim_in"], m["dim_hidden"], m["n_layers"], 1)
    y, dydx = kernel(amd, torch.from_numpy(fx["x"]), params, m["w0_initial"], m["w0"])
    assert y.shape == (fx["x"].shape[0],) and dydx.shape == fx["x"].shape
    assert_close(y.numpy().reshape(-1, 1), fx["pred"], REL_TOL, f"{name}: y")
    check_dx_relation(fx, dydx.numpy(), f"{name}: dydx 2 (pred - y) / n against the fixture's dx")


# ---------------------------------------------------------------------------------------------- 2. float64
SWEEP = [
    # hidden, dim_in, n_sine, n          n in {1, P - 1, P, P + 1, 2 P + 3} per width
    (256, 3, 3, 1), (256, 1, 2, 15), (256, 2, 8, 16), (256, 3, 2, 17), (256, 3, 3, 35),
    (128, 2, 3, 1), (128, 3, 2, 31), (128, 1, 3, 32), (128, 3, 8, 33), (128, 2, 2, 67),
    (64, 1, 8, 1), (64, 2, 2, 63), (64, 3, 3, 64), (64, 3, 2, 65), (64, 1, 3, 131),
    (128, 3, 3, GRID_BLOCKS * 32 + 5),  # the persistent loop wraps and ends in a partial tile
]


def yardstick_case(amd, hidden, dim_in, n_sine, n, w0_first=30.0, w0=30.0):
    assert amd.ops.siren_gradient_supported(dim_in, hidden, n_sine, 1)
    params, x, (y32, g32), (y64, g64) = case(hidden, dim_in, n_sine, n, w0_first, w0)
    y, dydx = kernel(amd, x, params, w0_first, w0)
    assert y.shape == (n,) and dydx.shape == (n, dim_in)
    assert torch.isfinite(y).all() and torch.isfinite(dydx).all()
    tag = f"{dim_in} -> {hidden} x {n_sine} -> 1, n = {n}, w0 {w0_first:g} / {w0:g}"
    assert_no_worse(y.numpy(), y32.numpy(), y64.numpy(), f"y ({tag})")
    assert_no_worse(dydx.numpy(), g32.numpy(), g64.numpy(), f"dydx ({tag})")


@pytest.mark.parametrize("hidden,dim_in,n_sine,n", SWEEP)
def test_against_float64(amd, hidden, dim_in, n_sine, n):
    """The kernel is no worse a float32 evaluation than float32 autograd on the CPU: both against the same
    computation in float64 on the same float32 inputs (yardstick.assert_no_worse, factor 2, floor 1e-6)."""
    yardstick_case(amd, hidden, dim_in, n_sine, n)


def test_against_float64_with_two_frequencies(amd):
    yardstick_case(amd, 64, 3, 3, 131, w0_first=20.0, w0=30.0)


@pytest.mark.parametrize("hidden,dim_in,n_sine,n", [(32, 3, 3, 131), (64, 2, 1, 65)])
def test_against_float64_optional_shapes(amd, hidden, dim_in, n_sine, n):
    """hidden = 32 and a single sine layer: where mri_siren_gradient_supported says yes, the same bar holds."""
    if not amd.ops.siren_gradient_supported(dim_in, hidden, n_sine, 1):
        assert not amd.lib.load().mri_siren_gradient_supported(dim_in, hidden, n_sine, 1)
        return  # refused: SirenNet.forward_with_gradient serves it with the generic body
    yardstick_case(amd, hidden, dim_in, n_sine, n)


# ---------------------------------------------------------------------------------------------- 3. unused slots
@pytest.mark.parametrize("hidden,dim_in,n", [(256, 1, 35), (64, 2, 131), (128, 1, 67), (128, 2, 33)])
def test_unused_slots_are_inert(amd, hidden, dim_in, n):
    """The network embedded in dim_in = 3 with zero weight columns (and arbitrary extra coordinates) gives the same
    y and the same dim_in gradient columns BITWISE: the first layer adds the axes' products in axis order, so the
    embedded sum only gains terms x_d * 0 = +-0 at its end, and the rows of a point never mix in the H x H products.
    The extra columns are exactly zero."""
    params, x, _, _ = case(hidden, dim_in, 3, n)
    y, dydx = kernel(amd, x, params)
    assert dydx.shape == (n, dim_in)
    w_first = torch.cat([params[0][0], torch.zeros(hidden, 3 - dim_in)], dim=1)
    extra = torch.from_numpy(detrand.uniform(n * (3 - dim_in), 99, -1.0, 1.0).reshape(n, 3 - dim_in).copy())
    y3, dydx3 = kernel(amd, torch.cat([x, extra], dim=1), [(w_first, params[0][1])] + list(params[1:]))
    assert dydx3.shape == (n, 3)
    assert torch.equal(y3, y) and torch.equal(dydx3[:, :dim_in], dydx)
    assert (dydx3[:, dim_in:] == 0).all()


# ---------------------------------------------------------------------------------------------- 4. layout
@pytest.mark.parametrize("hidden,dim_in,n", [(256, 3, 35), (64, 2, 131)])
def test_layout_guard_bands_and_rows_beyond_n(amd, hidden, dim_in, n):
    """x, y and dydx at 4-byte aligned addresses that are not 16-byte aligned: the guard bands around y and dydx keep
    every bit, the rows >= n of both outputs are untouched, x is unchanged, and the results equal the aligned call's
    bitwise."""
    n_sine, extra = 3, 5
    params, x, _, (y64, g64) = case(hidden, dim_in, n_sine, n)
    w, b = [p[0].cuda() for p in params], [p[1].cuda() for p in params]
    nan_bits = torch.full((1,), float("nan")).view(torch.int32).item()
    aligned = None
    for tag, layout in variants(dict(x=None, y=None, dydx=None), lds=False):
        p = Placer(layout, tag)
        xv = p.inp("x", x.reshape(-1))
        yv, gv = p.out("y", (n + extra,)), p.out("dydx", ((n + extra) * dim_in,))
        if tag != "aligned":
            assert any(t.data_ptr() % 16 != 0 for t in (xv, yv, gv)) and all(t.data_ptr() % 4 == 0 for t in (xv, yv, gv))
        amd.ops.siren_gradient(xv.view(n, dim_in), w, b, 30.0, 30.0, y=yv[:n], dydx=gv[:n * dim_in].view(n, dim_in))
        p.verify()
        assert (yv[n:].view(torch.int32) == nan_bits).all(), f"{tag}: y rows >= n were written"
        assert (gv[n * dim_in:].view(torch.int32) == nan_bits).all(), f"{tag}: dydx rows >= n were written"
        got = yv[:n].cpu().clone(), gv[:n * dim_in].cpu().clone().view(n, dim_in)
        assert_close(got[0].numpy(), y64.numpy(), REL_TOL, f"{tag}: y")
        assert_close(got[1].numpy(), g64.numpy(), REL_TOL, f"{tag}: dydx")
        if aligned is None:
            aligned = got
        assert torch.equal(got[0], aligned[0]) and torch.equal(got[1], aligned[1]), f"{tag}: differs from the aligned call"


# ---------------------------------------------------------------------------------------------- 5. reproducibility
@pytest.mark.parametrize("hidden,n", [(256, 35), (128, GRID_BLOCKS * 32 + 5), (64, 131)])
def test_two_calls_agree_bitwise_and_y_is_the_forward_kernels(amd, hidden, n):
    params, x, _, _ = case(hidden, 3, 3, n)
    y1, g1 = kernel(amd, x, params)
    y2, g2 = kernel(amd, x, params)
    assert torch.equal(y1, y2) and torch.equal(g1, g2)
    fwd = amd.ops.siren_forward(x.cuda(), [w.cuda() for w, _ in params], [b.cuda() for _, b in params], 30.0, 30.0)
    assert_close(y1.numpy(), fwd.cpu().numpy().reshape(-1), REL_TOL, "y against ops.siren_forward")


# ---------------------------------------------------------------------------------------------- 6. dispatch
def autograd_through_forward(net, x):
    xg = x.detach().clone().requires_grad_(True)
    y = net(xg)
    g, = torch.autograd.grad(y.sum(), xg)
    return y.detach(), g.detach()


def no_kernel(amd, monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the fused gradient kernel must not serve this model")
    monkeypatch.setattr(amd.ops, "siren_gradient", refuse)


def check_detached(net, y, g):
    assert not y.requires_grad and not g.requires_grad and y.grad_fn is None and g.grad_fn is None
    assert all(p.grad is None for p in net.parameters())


def test_dispatch_hidden_352_takes_the_generic_body(amd, monkeypatch):
    fx = load_golden("siren_2d_4x352")
    net, _ = load_siren(amd, fx)
    assert not amd.ops.siren_gradient_supported(2, 352, 4, 1)
    no_kernel(amd, monkeypatch)
    y, g = net.forward_with_gradient(cuda(fx["x"]))
    assert y.shape == (192, 1) and g.shape == (192, 2)
    check_detached(net, y, g)
    assert_close(y.cpu().numpy(), fx["pred"], REL_TOL, "y")
    check_dx_relation(fx, g.cpu().numpy(), "hidden 352: dydx 2 (pred - y) / n against the fixture's dx")


@pytest.mark.parametrize("kw", [dict(final_activation=nn.Tanh()), dict(use_bias=False)], ids=["tanh_head", "no_bias"])
def test_dispatch_other_heads_and_no_bias_take_the_generic_body(amd, monkeypatch, kw):
    fx = load_golden("siren_2d_3x64")
    net, _ = load_siren(amd, fx, **kw)
    x = cuda(fx["x"])
    want_y, want_g = autograd_through_forward(net, x)
    no_kernel(amd, monkeypatch)
    y, g = net.forward_with_gradient(x)
    check_detached(net, y, g)
    assert torch.equal(y, want_y) and torch.equal(g, want_g)
    assert g.abs().max() > 0


def test_dispatch_modulated_siren_is_autograd_through_its_own_forward(amd, monkeypatch):
    torch.manual_seed(5)
    net = amd.models.ModulatedSirenNet(3, 64, 1, 3).cuda()
    x = cuda(detrand.uniform(131 * 3, 3, -1.0, 1.0).reshape(131, 3))
    want_y, want_g = autograd_through_forward(net, x)
    y, g = net.forward_with_gradient(x)
    check_detached(net, y, g)
    assert torch.equal(y, want_y) and torch.equal(g, want_g), "ModulatedSirenNet: not its own forward's gradient"
    # the plain chain of its inner SirenNet is another function: a wrong dispatch cannot pass the line above
    py, pg = amd.models.SirenNet.forward_with_gradient(net.siren, x)
    assert not torch.allclose(py, want_y, rtol=1e-3, atol=1e-3) and not torch.allclose(pg, want_g, rtol=1e-3, atol=1e-3)
    no_kernel(amd, monkeypatch)
    net.forward_with_gradient(x)


def test_dispatch_plain_and_psf_siren_take_the_kernel(amd, monkeypatch):
    fx = load_golden("siren_3d_5x256")
    plain, params = load_siren(amd, fx)
    psf, _ = load_siren(amd, fx, cls=amd.models.PsfSirenNet, coordinates_spacing=(0.01, 0.01, 0.1), n_sample=3)
    x = cuda(fx["x"])
    want_y, want_g = amd.ops.siren_gradient(x, [w.cuda() for w, _ in params], [b.cuda() for _, b in params], 30.0, 30.0)
    calls, real = [], amd.ops.siren_gradient
    monkeypatch.setattr(amd.ops, "siren_gradient", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    for net in (plain, psf):
        before = len(calls)
        y, g = net.forward_with_gradient(x)
        assert len(calls) == before + 1, f"{type(net).__name__} did not take the kernel"
        check_detached(net, y, g)
        assert y.shape == (192, 1) and g.shape == (192, 3)
        assert torch.equal(y, want_y) and torch.equal(g, want_g)
    # and the kernel's answer is the generic body's, at the parity bar
    gy, gg = amd.models.BaseMLP.forward_with_gradient(plain, x)
    check_detached(plain, gy, gg)
    assert_close(want_y.cpu().numpy(), gy.cpu().numpy(), REL_TOL, "kernel y against the generic body")
    assert_close(want_g.cpu().numpy(), gg.cpu().numpy(), REL_TOL, "kernel dydx against the generic body")


def test_hashmlp_generic_body_runs_through_the_hash_grid(amd):
    """HashMLP has no fused form: autograd through its forward, the coordinates' gradient coming out of the hash grid's
    input backward.  Plumbing: shapes, detachment, equality with autograd spelled out, and agreement with central
    differences on most rows (the encoder is piecewise multilinear and the decoder has ReLU kinks: rows whose +-h
    neighbours straddle a cell face or a kink are the exceptions, so a share of the rows is asked for, not all)."""
    torch.manual_seed(7)
    net = amd.models.HashMLP(3, 4, 2, 12, 4, 16, dim_hidden=64, dim_out=1, n_layers=3, activation=nn.ReLU,
                             batch_norm=False, final_activation=False).cuda().eval()
    with torch.no_grad():
        net.encoder.table.copy_(cuda(detrand.uniform(net.encoder.table.numel(), 21, -1.0, 1.0).reshape(net.encoder.table.shape)))
    x = cuda(detrand.uniform(257 * 3, 22, 0.05, 0.95).reshape(257, 3))
    want_y, want_g = autograd_through_forward(net, x)
    y, g = net.forward_with_gradient(x)
    check_detached(net, y, g)
    assert y.shape == (257, 1) and g.shape == (257, 3) and torch.isfinite(g).all() and g.abs().max() > 0
    assert torch.equal(y, want_y) and torch.equal(g, want_g)
    h, fd = 1e-3, []
    with torch.no_grad():
        for d in range(3):
            e = torch.zeros(3, device="cuda")
            e[d] = h
            fd.append((net(x + e).double() - net(x - e).double()) / (2 * h))
    fd = torch.cat(fd, dim=1)
    near = (fd - g.double()).abs() <= 5e-2 * g.abs().max().double()
    assert near.double().mean() >= 0.8, f"only {float(near.double().mean()):.2f} of the entries agree with central differences"


# ---------------------------------------------------------------------------------------------- 7. trainer, launcher
def test_predict_with_gradient_is_the_per_batch_twin_of_predict(amd):
    torch.manual_seed(11)
    vol = amd.datamodules.phantom_volume((8, 8, 4)).cpu().numpy()
    ds = amd.datamodules.MriImage(volume=vol, norm_siren=True)
    loader = amd.datamodules.DeviceLoader(ds, 100, shuffle=False)  # 256 voxels: batches of 100, 100, 56
    net = amd.models.SirenNet(dim_in=3, dim_hidden=64, dim_out=1, n_layers=3).cuda()
    trainer = amd.trainer.Trainer(max_epochs=1, max_steps=1, precision=32, log_every=0)
    ys, gs = trainer.predict_with_gradient(net, loader)
    batches = [x for x, _ in loader]
    assert [tuple(y.shape) for y in ys] == [(100, 1), (100, 1), (56, 1)]
    assert [tuple(g.shape) for g in gs] == [(100, 3), (100, 3), (56, 3)]
    for x, y, g in zip(batches, ys, gs):
        dy, dg = net.forward_with_gradient(x)
        assert torch.equal(y, dy) and torch.equal(g, dg)
    preds = trainer.predict(net, loader)
    assert len(preds) == len(ys)
    for y, pr in zip(ys, preds):  # (two kernels, two summation orders where the widths' kernels differ: the parity bar)
        assert y.shape == pr.shape
        assert_close(y.cpu().numpy(), pr.cpu().numpy(), REL_TOL, "y of predict_with_gradient against predict")


def test_launcher_save_gradient_on_the_gpu_path(amd, tmp_path):
    import launcher
    from mri_interpolation_amd import nifti
    out = str(tmp_path / "run")
    launcher.main(["--synthetic", "16,16,8", "--model_class", "SirenNet", "--dim_hidden", "64", "--n_layers", "3",
                   "--max_steps", "2", "--save_gradient", "--out_dir", out, "--log_every", "0"])
    grad = nifti.load(os.path.join(out, "gradient.nii.gz"))
    assert grad.shape == (16, 16, 8, 3) and grad.dtype == np.float32 and np.isfinite(grad).all()
    ckpt, = os.listdir(os.path.join(out, "checkpoints"))
    net = amd.models.SirenNet(dim_in=3, dim_hidden=64, dim_out=1, n_layers=3)
    amd.checkpoint.load(os.path.join(out, "checkpoints", ckpt), net)
    net = net.cuda()
    vol = amd.datamodules.phantom_volume((16, 16, 8)).cpu().numpy()
    ds = amd.datamodules.MriImage(volume=vol, norm_siren=True)
    loader = amd.datamodules.DeviceLoader(ds, 4096, shuffle=False)  # BaseConfig's batch size: one batch
    trainer = amd.trainer.Trainer(max_epochs=1, max_steps=1, precision=32, log_every=0)
    ys, gs = trainer.predict_with_gradient(net, loader)
    scale = np.asarray(launcher.gradient_voxel_scale((16, 16, 8), True), dtype=np.float32)
    assert tuple(scale) == (np.float32(2 / 15), np.float32(2 / 15), np.float32(2 / 7))
    want = (torch.concat(gs).cpu().numpy().astype(np.float32) * scale).reshape(16, 16, 8, 3)
    assert np.abs(want).max() > 0
    assert np.array_equal(grad, want)
    pred = nifti.load(os.path.join(out, "pred.nii.gz"))
    assert_close(torch.concat(ys).cpu().numpy().reshape(16, 16, 8), pred, REL_TOL, "y against pred.nii.gz")
