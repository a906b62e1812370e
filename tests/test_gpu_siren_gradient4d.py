"""The fused SIREN coordinate gradient with FOUR input axes (csrc/siren_gradient.hip, the eight-slot form: a point
travels as [value, d/dx_0, d/dx_1, d/dx_2 | value, d/dx_3, 0, 0]) on the GPU: against what the reference produced,
against float64, against the four-slot form bitwise, and through every layer above the kernel -- ops,
`SirenNet.forward_with_gradient`, `Trainer.predict_with_gradient` and `launcher.py --save_gradient`, the gradient
volumes on the interpolation grids included.

P = points per tile = image rows / 8: 8, 16, 32 (and 32) at hidden 256, 128, 64 (and 32); at most 256 workgroups walk
the tiles (include/mri_inr.h), so n = 256 P + 5 makes the persistent loop wrap and end in a partial tile.
"""
import dataclasses
import functools
import os

import numpy as np
import pytest
import torch

from conftest import REL_TOL, assert_close, load_golden
from layout import Placer, variants
from yardstick import assert_no_worse
from oracle import detrand
from oracle import mlp as omlp

pytestmark = pytest.mark.gpu

POINTS = {256: 8, 128: 16, 64: 32, 32: 32}
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
def inputs(hidden, dim_in, n_sine, n, w0=30.0):
    """Parameters (oracle.mlp.siren_init) and coordinates drawn by oracle.detrand in [-1, 1] with rows at exactly -1,
    0 and 1 among them.  Computed once, shared, never modified."""
    params = omlp.siren_init(dim_in, hidden, 1, n_sine, 1000 + hidden + 10 * n_sine + dim_in, w0=w0)
    x = torch.from_numpy(detrand.uniform(n * dim_in, 7 * n + dim_in, -1.0, 1.0).reshape(n, dim_in).copy())
    for row, v in zip((n // 2, n - 1, 0), (-1.0, 0.0, 1.0)):  # (n = 1: the row ends at exactly 1)
        x[row] = v
    return params, x


@functools.lru_cache(maxsize=None)
def case(hidden, n_sine, n, w0_first=30.0, w0=30.0):
    """inputs() with dim_in = 4 and the float32 / float64 references."""
    params, x = inputs(hidden, 4, n_sine, n, w0)
    return params, x, reference(x, params, w0_first, w0, torch.float32), reference(x, params, w0_first, w0, torch.float64)


# ---------------------------------------------------------------------------------------------- 1. the reference
@pytest.mark.parametrize("name", ["siren_4d_4x64", "siren_4d_3x256"])
def test_against_what_the_reference_produced(amd, name):
    """y, dydx and the reference's own x.grad of its training loss, dx = dydx (.) 2 (pred - y) / n."""
    fx = load_golden(name)
    m = fx.meta
    assert m["dim_in"] == 4
    params = omlp.siren_init(4, m["dim_hidden"], 1, m["n_layers"], m["seed"])
    assert amd.ops.siren_gradient_supported(4, m["dim_hidden"], m["n_layers"], 1)
    y, dydx = kernel(amd, torch.from_numpy(fx["x"]), params, m["w0_initial"], m["w0"])
    n = fx["x"].shape[0]
    assert y.shape == (n,) and dydx.shape == (n, 4)
    assert_close(y.numpy().reshape(-1, 1), fx["pred"], REL_TOL, f"{name}: y")
    assert_close(dydx.numpy(), fx["dydx"], REL_TOL, f"{name}: dydx")
    scale = 2.0 * (fx["pred"].astype(np.float64) - fx["y"].astype(np.float64)) / n
    assert_close(dydx.numpy().astype(np.float64) * scale, fx["dx"], REL_TOL,
                 f"{name}: dydx 2 (pred - y) / n against the fixture's dx")


# ---------------------------------------------------------------------------------------------- 2. float64
SWEEP = [
    # hidden, n_sine, n          n in {1, P - 1, P, P + 1, 2 P + 3} per width
    (256, 3, 1), (256, 2, 7), (256, 8, 8), (256, 2, 9), (256, 3, 19),
    (128, 3, 1), (128, 2, 15), (128, 3, 16), (128, 8, 17), (128, 2, 35),
    (64, 8, 1), (64, 2, 31), (64, 3, 32), (64, 2, 33), (64, 3, 67),
    (32, 3, 67),
    (64, 1, 33),  # a single sine layer: no H x H product, the first layer's image goes to the head
    (128, 3, GRID_BLOCKS * 16 + 5),  # the persistent loop wraps and ends in a partial tile
]


def yardstick_case(amd, hidden, n_sine, n, w0_first=30.0, w0=30.0):
    assert amd.ops.siren_gradient_supported(4, hidden, n_sine, 1)
    params, x, (y32, g32), (y64, g64) = case(hidden, n_sine, n, w0_first, w0)
    y, dydx = kernel(amd, x, params, w0_first, w0)
    assert y.shape == (n,) and dydx.shape == (n, 4)
    assert torch.isfinite(y).all() and torch.isfinite(dydx).all()
    tag = f"4 -> {hidden} x {n_sine} -> 1, n = {n}, w0 {w0_first:g} / {w0:g}"
    assert_no_worse(y.numpy(), y32.numpy(), y64.numpy(), f"y ({tag})")
    assert_no_worse(dydx.numpy(), g32.numpy(), g64.numpy(), f"dydx ({tag})")


@pytest.mark.parametrize("hidden,n_sine,n", SWEEP)
def test_against_float64(amd, hidden, n_sine, n):
    """The kernel is no worse a float32 evaluation than float32 autograd on the CPU: both against the same
    computation in float64 on the same float32 inputs (yardstick.assert_no_worse, factor 2, floor 1e-6)."""
    assert n in (1, POINTS[hidden] - 1, POINTS[hidden], POINTS[hidden] + 1, 2 * POINTS[hidden] + 3,
                 GRID_BLOCKS * POINTS[hidden] + 5)
    yardstick_case(amd, hidden, n_sine, n)


def test_against_float64_with_two_frequencies(amd):
    yardstick_case(amd, 64, 3, 67, w0_first=20.0, w0=30.0)


# ---------------------------------------------------------------------------------------------- 3. eight slots / four
@pytest.mark.parametrize("hidden,n", [(256, 19), (64, 67)])
@pytest.mark.parametrize("dim_in", [1, 2, 3])
def test_eight_slots_equal_four_slots_bitwise(amd, hidden, n, dim_in):
    """A dim_in = 1, 2, 3 network embedded in dim_in = 4 with zero weight columns (and arbitrary extra coordinates)
    runs the eight-slot form; y and the shared gradient columns equal the four-slot kernel's BITWISE: the first layer
    adds the axes' products in axis order, so the embedded sum only gains terms x_d * 0 = +-0 at its end, the rows of
    a point never mix in the H x H products (an MFMA's rows are independent, and a row meets the same weight chunks in
    the same order wherever it sits in the image), the epilogue is one expression for both forms and the head sums a
    row the same way.  The extra columns are exactly zero."""
    params, x = inputs(hidden, dim_in, 3, n)
    y, dydx = kernel(amd, x, params)
    assert dydx.shape == (n, dim_in)
    w_first = torch.cat([params[0][0], torch.zeros(hidden, 4 - dim_in)], dim=1)
    extra = torch.from_numpy(detrand.uniform(n * (4 - dim_in), 99, -1.0, 1.0).reshape(n, 4 - dim_in).copy())
    y4, dydx4 = kernel(amd, torch.cat([x, extra], dim=1), [(w_first, params[0][1])] + list(params[1:]))
    assert dydx4.shape == (n, 4)
    assert dydx.abs().max() > 0
    assert torch.equal(y4, y), f"y: {int((y4 != y).sum())} of {n} values differ"
    assert torch.equal(dydx4[:, :dim_in], dydx), f"dydx: {int((dydx4[:, :dim_in] != dydx).sum())} entries differ"
    assert (dydx4[:, dim_in:] == 0).all()


# ---------------------------------------------------------------------------------------------- 4. layout
@pytest.mark.parametrize("hidden,n", [(256, 19), (64, 67)])
def test_layout_guard_bands_and_rows_beyond_n(amd, hidden, n):
    """x, y and dydx at 4-byte aligned addresses that are not 16-byte aligned: the guard bands around y and dydx keep
    every bit, the rows >= n of both outputs are untouched, x is unchanged, and the results equal the aligned call's
    bitwise."""
    n_sine, extra, dim_in = 3, 5, 4
    params, x, _, (y64, g64) = case(hidden, n_sine, n)
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
@pytest.mark.parametrize("hidden,n", [(256, 19), (128, GRID_BLOCKS * 16 + 5)])
def test_two_calls_agree_bitwise_and_y_is_the_forward_kernels(amd, hidden, n):
    params, x, _, _ = case(hidden, 3, n)
    y1, g1 = kernel(amd, x, params)
    y2, g2 = kernel(amd, x, params)
    assert torch.equal(y1, y2) and torch.equal(g1, g2)
    fwd = amd.ops.siren_forward(x.cuda(), [w.cuda() for w, _ in params], [b.cuda() for _, b in params], 30.0, 30.0)
    assert_close(y1.numpy(), fwd.cpu().numpy().reshape(-1), REL_TOL, "y against ops.siren_forward")


# ---------------------------------------------------------------------------------------------- 6. dispatch
def load_siren(amd, fx, **kw):
    m = fx.meta
    net = amd.models.SirenNet(dim_in=m["dim_in"], dim_hidden=m["dim_hidden"], dim_out=1, n_layers=m["n_layers"], **kw)
    params = omlp.siren_init(m["dim_in"], m["dim_hidden"], 1, m["n_layers"], m["seed"])
    with torch.no_grad():
        for layer, (w, b) in zip(list(net.layers) + [net.last_layer], params):
            layer.weight.copy_(w)
            if layer.bias is not None:
                layer.bias.copy_(b)
    return net.cuda(), params


def check_detached(net, y, g):
    assert not y.requires_grad and not g.requires_grad and y.grad_fn is None and g.grad_fn is None
    assert all(p.grad is None for p in net.parameters())


def test_dispatch_four_axes_take_the_kernel(amd, monkeypatch):
    fx = load_golden("siren_4d_4x64")
    net, params = load_siren(amd, fx)
    x = cuda(fx["x"])
    calls, real = [], amd.ops.siren_gradient
    monkeypatch.setattr(amd.ops, "siren_gradient", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    y, g = net.forward_with_gradient(x)
    torch.cuda.synchronize()
    assert len(calls) == 1, "SirenNet(dim_in=4) did not take the kernel"
    check_detached(net, y, g)
    assert y.shape == (96, 1) and g.shape == (96, 4)
    want_y, want_g = real(x, [w.cuda() for w, _ in params], [b.cuda() for _, b in params], 30.0, 30.0)
    assert torch.equal(y, want_y) and torch.equal(g, want_g)
    # and the kernel's answer is the generic body's: both against float64 on the CPU
    gy, gg = amd.models.BaseMLP.forward_with_gradient(net, x)
    assert len(calls) == 1
    check_detached(net, gy, gg)
    y64, g64 = reference(torch.from_numpy(fx["x"]), params, 30.0, 30.0, torch.float64)
    assert_no_worse(y.cpu().numpy().reshape(-1), gy.cpu().numpy().reshape(-1), y64.numpy(), "y against the generic body")
    assert_no_worse(g.cpu().numpy(), gg.cpu().numpy(), g64.numpy(), "dydx against the generic body")


def test_dispatch_four_axes_without_bias_take_the_generic_body(amd, monkeypatch):
    fx = load_golden("siren_4d_4x64")
    net, _ = load_siren(amd, fx, use_bias=False)
    x = cuda(fx["x"])
    xg = x.detach().clone().requires_grad_(True)
    want_y = net(xg)
    want_g, = torch.autograd.grad(want_y.sum(), xg)

    def refuse(*a, **k):
        raise AssertionError("the fused gradient kernel must not serve this model")
    monkeypatch.setattr(amd.ops, "siren_gradient", refuse)
    y, g = net.forward_with_gradient(x)
    check_detached(net, y, g)
    assert torch.equal(y, want_y.detach()) and torch.equal(g, want_g.detach())
    assert g.shape == (96, 4) and g.abs().max() > 0


# ---------------------------------------------------------------------------------------------- 7. trainer, launcher
def test_predict_with_gradient_on_a_4d_volume_is_the_per_batch_twin(amd):
    torch.manual_seed(11)
    vol = amd.datamodules.phantom_volume((8, 8, 4, 6)).cpu().numpy()
    ds = amd.datamodules.MriImage(volume=vol, norm_siren=True)
    loader = amd.datamodules.DeviceLoader(ds, 500, shuffle=False)  # 1536 voxels: batches of 500, 500, 500, 36
    net = amd.models.SirenNet(dim_in=4, dim_hidden=64, dim_out=1, n_layers=3).cuda()
    trainer = amd.trainer.Trainer(max_epochs=1, max_steps=1, precision=32, log_every=0)
    ys, gs = trainer.predict_with_gradient(net, loader)
    batches = [x for x, _ in loader]
    assert [tuple(y.shape) for y in ys] == [(500, 1)] * 3 + [(36, 1)]
    assert [tuple(g.shape) for g in gs] == [(500, 4)] * 3 + [(36, 4)]
    for x, y, g in zip(batches, ys, gs):
        dy, dg = net.forward_with_gradient(x)
        assert torch.equal(y, dy) and torch.equal(g, dg)
    assert torch.concat(gs)[:, 3].abs().max() > 0


def launcher_net(amd, out, dim_in):
    ckpt, = os.listdir(os.path.join(out, "checkpoints"))
    net = amd.models.SirenNet(dim_in=dim_in, dim_hidden=64, dim_out=1, n_layers=3)
    amd.checkpoint.load(os.path.join(out, "checkpoints", ckpt), net)
    return net.cuda()


def test_launcher_save_gradient_on_a_4d_volume(amd, tmp_path):
    import launcher
    from mri_interpolation_amd import nifti
    shape = (8, 8, 4, 6)
    out = str(tmp_path / "run")
    launcher.main(["--synthetic", "8,8,4,6", "--model_class", "SirenNet", "--dim_hidden", "64", "--n_layers", "3",
                   "--max_steps", "2", "--save_gradient", "--out_dir", out, "--log_every", "0"])
    grad = nifti.load(os.path.join(out, "gradient.nii.gz"))
    assert grad.shape == shape + (4,) and grad.dtype == np.float32 and np.isfinite(grad).all()
    net = launcher_net(amd, out, 4)
    vol = amd.datamodules.phantom_volume(shape).cpu().numpy()
    ds = amd.datamodules.MriImage(volume=vol, norm_siren=True)
    loader = amd.datamodules.DeviceLoader(ds, 4096, shuffle=False)  # BaseConfig's batch size: one batch
    trainer = amd.trainer.Trainer(max_epochs=1, max_steps=1, precision=32, log_every=0)
    ys, gs = trainer.predict_with_gradient(net, loader)
    scale = np.asarray(launcher.gradient_voxel_scale(shape, True), dtype=np.float32)
    assert tuple(scale) == (np.float32(2 / 7), np.float32(2 / 7), np.float32(2 / 3), np.float32(2 / 5))
    want = (torch.concat(gs).cpu().numpy().astype(np.float32) * scale).reshape(shape + (4,))
    assert np.abs(want[..., 3]).max() > 0
    assert np.array_equal(grad, want)
    pred = nifti.load(os.path.join(out, "pred.nii.gz"))
    assert_close(torch.concat(ys).cpu().numpy().reshape(shape), pred, REL_TOL, "y against pred.nii.gz")


def test_launcher_save_gradient_on_an_interpolation_grid(amd, tmp_path, monkeypatch):
    import launcher
    from mri_interpolation_amd import config as cfg, nifti
    grid = (20, 12, 9)
    base = cfg.BaseConfig
    monkeypatch.setattr(cfg, "BaseConfig", lambda: dataclasses.replace(base(), interp_shapes=[grid]))
    out = str(tmp_path / "run")
    launcher.main(["--synthetic", "16,16,8", "--model_class", "SirenNet", "--dim_hidden", "64", "--n_layers", "3",
                   "--batch_size", "1000", "--max_steps", "2", "--save_gradient", "--out_dir", out, "--log_every", "0"])
    interp = nifti.load(os.path.join(out, f"interpolation{grid}.nii.gz"))
    grad = nifti.load(os.path.join(out, f"gradient_interpolation{grid}.nii.gz"))
    assert interp.shape == grid
    assert grad.shape == grid + (3,) and grad.dtype == np.float32 and np.isfinite(grad).all()
    assert nifti.load(os.path.join(out, "gradient.nii.gz")).shape == (16, 16, 8, 3)
    net = launcher_net(amd, out, 3)
    loader = amd.datamodules.GridLoader(grid, 1000, norm_siren=True)  # 2160 points: batches of 1000, 1000, 160
    trainer = amd.trainer.Trainer(max_epochs=1, max_steps=1, precision=32, log_every=0)
    ys, gs = trainer.predict_with_gradient(net, loader)
    scale = np.asarray(launcher.gradient_voxel_scale(grid, True), dtype=np.float32)
    assert tuple(scale) == (np.float32(2 / 19), np.float32(2 / 11), np.float32(2 / 8))
    want = (torch.concat(gs).cpu().numpy().astype(np.float32) * scale).reshape(grid + (3,))
    assert np.abs(want).max() > 0
    assert np.array_equal(grad, want)
    assert_close(torch.concat(ys).cpu().numpy().reshape(grid), interp, REL_TOL, "y against the interpolation volume")
