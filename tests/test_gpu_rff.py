"""RffNet on the GPU (csrc/rff.hip): the encoding kernel and its input gradient, the fused inference kernel, the
reference's fixtures through `forward` + autograd, three Adam steps, the dispatch of `predict_step`, the launcher.

P = rows per tile of the fused kernel: 64 at hidden 128, 128 at hidden 64; at most 256 workgroups walk the tiles
(include/mri_inr.h), so n = 256 P + 5 takes the persistent loop past a workgroup's first tile and ends in a partial one.

ReLU kinks: y is continuous across them, so the comparisons of y drop no rows.  The fixtures' gradients are compared on
inputs whose every float64 pre-activation is at least 1e-5 from zero (tests/golden/make_golden_rff.py: a condition on
the input, recorded in `meta`).
"""
import dataclasses
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import exact_args
from conftest import REL_TOL, assert_close, load_golden, rel_err
from layout import Placer, ptr, variants
from test_gpu_workspace import arr, hold
from test_rff_cpu import net_from_fixture
from yardstick import AFTER_ADAM_MAX_FACTOR, assert_no_worse
from oracle import detrand
from oracle import mlp as omlp

pytestmark = pytest.mark.gpu

ROWS = {128: 64, 64: 128}
GRID_BLOCKS = 256
TWO_PI = np.float32(2 * np.pi)  # fl32(2 pi): `2 * np.pi * v` on a float32 tensor


@pytest.fixture(scope="module")
def amd():
    from mri_interpolation_amd import _lib, models, ops
    assert torch.cuda.is_available(), "these tests need the GPU"
    _lib.load()
    return type("NS", (), dict(lib=_lib, h=_lib.load(), ops=ops, models=models))


def close_or_no_worse(kernel, f32_ref, f64, what):
    """Within REL_TOL of float64, or no worse an f32 evaluation than the CPU's (yardstick: factor 2, floor 1e-6)."""
    e_max, e_l2 = rel_err(kernel, f64)
    print(f"{what}: kernel {e_max:.2e} / {e_l2:.2e} from float64")
    if e_max <= REL_TOL and e_l2 <= REL_TOL:
        return
    assert_no_worse(kernel, f32_ref, f64, what)


def uniform(shape, seed, lo=0.0, hi=1.0):
    return torch.from_numpy(detrand.uniform(int(np.prod(shape)), seed, lo, hi).reshape(shape).copy())


def gaussian(shape, seed, sigma):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * sigma


def encode_ref(x, b, dtype):
    """[cos | sin] of (fl32(2 pi) x) b^T in `dtype` on the CPU: the scaling in float32 IS the reference's op for float32,
    the float64 evaluation runs the same op sequence on the same float32 inputs."""
    vp = (float(TWO_PI) * x.to(dtype)) @ b.to(dtype).T if dtype == torch.float64 else (TWO_PI * x) @ b.T
    return torch.cat((torch.cos(vp), torch.sin(vp)), dim=-1)


# ============================================================================================ 1. encode, exact argument
def test_encode_exact_argument(amd):
    """dim_in 1, b = [[1.0]], one frequency: the kernel's argument is exactly the float32 u = fl32(fl32(2 pi) x), so the
    float64 sine and cosine of u are what a correct kernel rounds: 2e-7 absolute, on |u| in [0, 8192] (the fast path) and
    (8192, 1e6] (the library path), magnitudes, signs, quadrant multiples and ties mixed in every wave
    (tests/exact_args.py)."""
    a = exact_args.sincos_arguments()
    a = a[np.abs(a) <= 1e6]
    big = np.exp2(np.linspace(13.0, np.log2(1e6), 400)).astype(np.float32) * np.where(np.arange(400) % 2, -1, 1)
    x = np.concatenate([a, big.astype(np.float32)]).astype(np.float32) / TWO_PI
    u = (TWO_PI * x).astype(np.float32)
    assert (np.abs(u) <= 8192).sum() > 4000 and ((np.abs(u) > 8192) & (np.abs(u) <= 1e6)).sum() > 500
    assert np.abs(u).max() <= 1e6 * (1 + 1e-6) and (u == 0).any()
    z = amd.ops.rff_encode_forward(torch.from_numpy(x).reshape(-1, 1).cuda(), torch.ones(1, 1, device="cuda")).cpu().numpy()
    assert z.shape == (x.size, 2)
    err_c = np.abs(z[:, 0].astype(np.float64) - np.cos(u.astype(np.float64)))
    err_s = np.abs(z[:, 1].astype(np.float64) - np.sin(u.astype(np.float64)))
    print(f"cos {err_c.max():.3e}, sin {err_s.max():.3e} from float64 on exact arguments")
    assert err_c.max() <= 2e-7 and err_s.max() <= 2e-7


# ============================================================================================ 2. encode, general
ENCODE_SHAPES = [(1, 1), (2, 64), (3, 128), (4, 96), (8, 7)]
ENCODE_N = [1, 255, 256, 257, 70001]


@functools.lru_cache(maxsize=None)
def encode_case(d, n_freq, sigma):
    """x, b, an incoming gradient and the CPU references on the largest n (a test takes the first n rows)."""
    n = ENCODE_N[-1]
    x, b = uniform((n, d), 7000 + 10 * d + n_freq), gaussian((n_freq, d), 7100 + d + n_freq, sigma)
    return x, b, encode_ref(x, b, torch.float32), encode_ref(x, b, torch.float64)


@pytest.mark.parametrize("sigma", [1.0, 10.0])
@pytest.mark.parametrize("d,n_freq", ENCODE_SHAPES)
def test_encode_against_float64(amd, d, n_freq, sigma):
    x, b, z32, z64 = encode_case(d, n_freq, sigma)
    bc = b.cuda()
    for n in ENCODE_N:
        z = amd.ops.rff_encode_forward(x[:n].cuda(), bc).cpu()
        assert z.shape == (n, 2 * n_freq) and torch.isfinite(z).all()
        assert_no_worse(z.numpy(), z32[:n].numpy(), z64[:n].numpy(), f"z ({d}, {n_freq}), sigma {sigma:g}, n = {n}")
    z1 = amd.ops.rff_encode_forward(x.cuda(), bc)
    z2 = amd.ops.rff_encode_forward(x.cuda(), bc)
    assert torch.equal(z1, z2)


@pytest.mark.parametrize("d,n_freq", [(3, 128), (8, 7)])
def test_encode_layout_guard_bands(amd, d, n_freq):
    """x and z at 4-byte aligned addresses that are not 16-byte aligned, dz and dx as well: guard bands keep every bit,
    rows >= n are untouched, inputs are unchanged, and the results equal the aligned call's bitwise."""
    n, extra = 257, 3
    x, b, _, _ = encode_case(d, n_freq, 10.0)
    x, bc = x[:n], b.cuda()
    dz = uniform((n, 2 * n_freq), 7300 + d, -1.0, 1.0)
    nan_bits = torch.full((1,), float("nan")).view(torch.int32).item()
    st = amd.ops._stream()
    aligned = None
    for tag, layout in variants(dict(x=None, z=None, dz=None, dx=None), lds=False):
        p = Placer(layout, tag)
        xv, dzv = p.inp("x", x.reshape(-1)), p.inp("dz", dz.reshape(-1))
        zv, dxv = p.out("z", ((n + extra) * 2 * n_freq,)), p.out("dx", ((n + extra) * d,))
        amd.lib.call("mri_rff_encode", ptr(xv), n, d, ptr(bc), n_freq, ptr(zv), st)
        amd.lib.call("mri_rff_encode_backward_input", ptr(xv), n, d, ptr(bc), n_freq, ptr(dzv), ptr(dxv), st)
        p.verify()
        assert (zv[n * 2 * n_freq:].view(torch.int32) == nan_bits).all(), f"{tag}: z rows >= n were written"
        assert (dxv[n * d:].view(torch.int32) == nan_bits).all(), f"{tag}: dx rows >= n were written"
        got = zv[:n * 2 * n_freq].cpu().clone(), dxv[:n * d].cpu().clone()
        assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all()
        aligned = got if aligned is None else aligned
        assert torch.equal(got[0], aligned[0]) and torch.equal(got[1], aligned[1]), f"{tag}: differs from the aligned call"


@pytest.mark.parametrize("sigma", [1.0, 10.0])
@pytest.mark.parametrize("d,n_freq", ENCODE_SHAPES)
def test_encode_input_gradient_against_float64_autograd(amd, d, n_freq, sigma):
    n = 257
    x, b, _, _ = encode_case(d, n_freq, sigma)
    x = x[:n]
    dz = uniform((n, 2 * n_freq), 7200 + d + n_freq, -1.0, 1.0)
    xg = x.double().clone().requires_grad_(True)
    want, = torch.autograd.grad((encode_ref(xg, b, torch.float64) * dz.double()).sum(), xg)
    xc = x.cuda().requires_grad_(True)
    bc = b.cuda()
    z = amd.ops.rff_encode(xc, bc)
    got, = torch.autograd.grad(z, xc, dz.cuda())
    assert got.shape == (n, d)
    assert_close(got.cpu().numpy(), want.numpy(), REL_TOL, f"dx ({d}, {n_freq}), sigma {sigma:g}")
    again = amd.ops.rff_encode_backward_input(x.cuda(), bc, dz.cuda())
    assert torch.equal(got, again), "two calls of the input gradient differ"
    # b is frozen: no gradient flows to it even when it asks for one
    bg = b.cuda().requires_grad_(True)
    assert torch.autograd.grad(amd.ops.rff_encode(xc, bg).sum(), [xc, bg], allow_unused=True)[1] is None


# ============================================================================================ 3. fused inference
FUSED_SHAPES = [(3, 128, 6), (2, 64, 3), (1, 64, 2), (4, 64, 8), (3, 128, 2)]


def sizes(hidden):
    p = ROWS[hidden]
    return [1, p - 1, p, p + 1, 2 * p + 3, GRID_BLOCKS * p + 5]


def rff_init(d, hidden, L, seed, sigma=10.0):
    """b (hidden, d) and the decoder's (weight, bias) pairs: uniform in He's bound, so that the signal keeps its size
    through the depth (`centred_head` then moves the head's bias so that the head clamps half of the rows)."""
    b = gaussian((hidden, d), seed, sigma)
    params = []
    for i in range(L):
        fan_in, fan_out = (2 * hidden if i == 0 else hidden), (1 if i == L - 1 else hidden)
        bound = float(np.sqrt(6.0 / fan_in))
        params.append((uniform((fan_out, fan_in), seed + 10 * i + 1, -bound, bound), uniform((fan_out,), seed + 10 * i + 2, -0.1, 0.1)))
    return b, params


def rff_ref(x, b, params, dtype):
    """(y (n), the head's pre-activation (n)) of the formulas in `dtype` on the CPU."""
    with torch.no_grad():
        h = encode_ref(x, b, dtype)
        for w, bias in params:
            p = F.linear(h, w.to(dtype), bias.to(dtype))
            h = torch.relu(p)
    return h.reshape(-1), p.reshape(-1)


def centred_head(x, b, params):
    """The same parameters with the head's bias moved by the median of the head's float64 pre-activation over x: behind
    a deep ReLU stack the head's sum has one sign on almost every row, and a head that clamps no row (or every row)
    shows nothing about the clamp."""
    _, pre64 = rff_ref(x, b, params, torch.float64)
    w, bias = params[-1]
    return params[:-1] + [(w, (bias.double() - pre64.median()).float())]


@functools.lru_cache(maxsize=None)
def fused_case(d, hidden, L):
    seed = 8100 + hidden + L + 10 * d
    n = sizes(hidden)[-1]
    x = uniform((n, d), seed + 5)
    b, params = rff_init(d, hidden, L, seed)
    params = centred_head(x, b, params)
    y32, _ = rff_ref(x, b, params, torch.float32)
    y64, pre64 = rff_ref(x, b, params, torch.float64)
    assert 0.1 < float((pre64 < -1e-6).double().mean()) < 0.9, "the head clamps a share of the rows, not all"
    return x, b, params, y32, y64, pre64


def device_params(b, params):
    return b.cuda(), [w.cuda() for w, _ in params], [v.cuda() for _, v in params]


def layer_path(amd, x, bc, ws, bs):
    h = amd.ops.rff_encode_forward(x, bc)
    for w, v in zip(ws, bs):
        h = amd.ops.linear_act(h, w, v, amd.ops.ACT_RELU, 1.0)
    return h


@pytest.mark.parametrize("d,hidden,L", FUSED_SHAPES)
def test_fused_forward_against_float64_and_the_layer_path(amd, d, hidden, L):
    assert amd.ops.rff_forward_supported(d, hidden, hidden, L, 1)
    x, b, params, y32, y64, pre64 = fused_case(d, hidden, L)
    bc, ws, bs = device_params(b, params)
    for n in sizes(hidden):
        xc = x[:n].cuda()
        y = amd.ops.rff_forward(xc, bc, ws, bs)
        assert y.shape == (n, 1)
        y = y.cpu().reshape(-1)
        assert torch.isfinite(y).all() and float(y.min()) >= 0.0
        tag = f"{d} -> {hidden} x {L} -> 1, n = {n}"
        close_or_no_worse(y.numpy(), y32[:n].numpy(), y64[:n].numpy(), f"y ({tag})")
        clamped = pre64[:n] < -1e-6
        assert (y[clamped] == 0).all(), f"{tag}: a row the float64 head puts below -1e-6 is not exactly 0"
        lp = layer_path(amd, xc, bc, ws, bs).cpu().numpy().reshape(-1)
        print(f"y against the layer path ({tag}): {rel_err(y.numpy(), lp)[0]:.2e}")
        assert_close(y.numpy(), lp, REL_TOL, f"y against the layer path ({tag})")
    assert bool((pre64 < -1e-6).any()) and float(y64.max()) > 0


@pytest.mark.parametrize("hidden", [64, 128])
def test_fused_forward_unused_coordinate_is_inert(amd, hidden):
    """The dim_in = 2 network embedded in dim_in = 3 with a zero third column of b (and arbitrary third coordinates)
    gives the same y bitwise: the sum over the axes runs in axis order and only gains a term x_2 * 0 at its end."""
    L, n = 3, 2 * ROWS[hidden] + 3
    x, b, params, _, _, _ = fused_case(2, hidden, L)
    bc, ws, bs = device_params(b, params)
    y = amd.ops.rff_forward(x[:n].cuda(), bc, ws, bs)
    b3 = torch.cat([b, torch.zeros(hidden, 1)], dim=1).cuda()
    x3 = torch.cat([x[:n], uniform((n, 1), 99)], dim=1).cuda()
    y3 = amd.ops.rff_forward(x3, b3, ws, bs)
    assert torch.equal(y, y3) and float(y.max()) > 0


def test_fused_forward_two_calls_agree_bitwise(amd):
    d, hidden, L, n = 3, 128, 6, 70001
    x = uniform((n, d), 8001)
    b, params = rff_init(d, hidden, L, 8002)
    bc, ws, bs = device_params(b, centred_head(x, b, params))
    xc = x.cuda()
    y1 = amd.ops.rff_forward(xc, bc, ws, bs).clone()
    y2 = amd.ops.rff_forward(xc, bc, ws, bs)
    assert torch.equal(y1, y2) and float(y1.max()) > 0 and torch.isfinite(y1).all()


@pytest.mark.parametrize("d,hidden,L", [(3, 128, 3), (2, 64, 3)])
def test_fused_forward_layout_guard_bands_and_rows_beyond_n(amd, d, hidden, L):
    n, extra = 3 * ROWS[hidden] - 1, 5
    x, b, params, y32, y64, _ = fused_case(d, hidden, L)
    x = x[:n]
    bc, ws, bs = device_params(b, params)
    nan_bits = torch.full((1,), float("nan")).view(torch.int32).item()
    aligned = None
    for tag, layout in variants(dict(x=None, y=None), lds=False):
        p = Placer(layout, tag)
        xv, yv = p.inp("x", x.reshape(-1)), p.out("y", (n + extra,))
        if tag != "aligned":
            assert any(t.data_ptr() % 16 != 0 for t in (xv, yv)) and all(t.data_ptr() % 4 == 0 for t in (xv, yv))
        amd.ops.rff_forward(xv.view(n, d), bc, ws, bs, y=yv[:n])
        p.verify()
        assert (yv[n:].view(torch.int32) == nan_bits).all(), f"{tag}: y rows >= n were written"
        got = yv[:n].cpu().clone()
        if aligned is None:
            aligned = got
            close_or_no_worse(got.numpy(), y32[:n].numpy(), y64[:n].numpy(), f"{tag}: y")
        assert torch.equal(got, aligned), f"{tag}: differs from the aligned call"


def workspace_entry(amd, d, hidden, L, n):
    x, b, params, y32, y64, _ = fused_case(d, hidden, L)
    xc = x[:n].cuda()
    bc, ws_, bs = device_params(b, params)
    st = amd.ops._stream()

    def launch(run, ws, nb):
        y = run.out((n,))
        amd.lib.call("mri_rff_forward", ptr(xc), n, d, hidden, hidden, L, ptr(bc), arr(ws_), arr(bs), ptr(y), ptr(ws), nb, st)
        return dict(y=y)

    return launch, amd.h.mri_rff_forward_workspace_bytes(hidden, L), (y32[:n], y64[:n])


@pytest.mark.parametrize("d,hidden,L,n", [(2, 64, 3, 2 * 128 + 3), (3, 128, 2, 256 * 64 + 5)])
def test_fused_forward_workspace_contract(amd, d, hidden, L, n):
    """tests/test_gpu_workspace.py `hold`: exactly the reported size between guards, zero-filled, after a larger call of
    another shape on the same buffer, filled with two bit patterns -- bitwise equal outputs --, and one byte short
    refused with the outputs and the guards untouched."""
    launch, need, (y32, y64) = workspace_entry(amd, d, hidden, L, n)
    assert need == L * 6 * hidden * hidden
    big = workspace_entry(amd, 3, 128, 8, 70)[:2]  # the largest workspace of the supported set
    assert big[1] > need

    def judge(got):
        close_or_no_worse(got["y"].numpy().reshape(-1), y32.numpy(), y64.numpy(), "workspace, zero-filled: y")
    hold(f"fused RFF forward {d} -> {hidden} x {L}, n = {n}:", launch, need, judge, big)


# ============================================================================================ 4. fixtures
@pytest.mark.parametrize("name", ["rff_2d_3x64", "rff_3d_6x128"])
def test_fixture_through_forward_and_autograd(amd, name):
    fx = load_golden(name)
    m = fx.meta
    assert m["min_abs_preactivation"] >= 1e-5
    net = net_from_fixture(fx).cuda()
    x = torch.from_numpy(fx["x"]).cuda().requires_grad_(True)
    y = torch.from_numpy(fx["y"]).cuda()
    pred = net(x)
    dx, = torch.autograd.grad(pred.sum(), x, retain_graph=True)
    loss = net.criterion(y, pred)
    linears = [l for l in net.decoder if isinstance(l, nn.Linear)]
    grads = torch.autograd.grad(loss, [t for l in linears for t in (l.weight, l.bias)])
    assert net.encoder.b.grad is None
    assert_close(pred.detach().cpu().numpy(), fx["pred"], REL_TOL, f"{name}: pred")
    assert abs(float(loss) - float(fx["loss"])) <= REL_TOL * abs(float(fx["loss"]))
    assert_close(dx.cpu().numpy(), fx["dx"], REL_TOL, f"{name}: dx")
    for i in range(m["n_layers"]):
        assert_close(grads[2 * i].cpu().numpy(), fx[f"gw_{i}"], REL_TOL, f"{name}: gw{i}")
        assert_close(grads[2 * i + 1].cpu().numpy(), fx[f"gb_{i}"], REL_TOL, f"{name}: gb{i}")
    y_g, dydx = net.eval().forward_with_gradient(x.detach())  # --save_gradient's route
    assert_close(dydx.cpu().numpy(), fx["dx"], REL_TOL, f"{name}: forward_with_gradient")
    assert_close(y_g.cpu().numpy(), fx["pred"], REL_TOL, f"{name}: forward_with_gradient's y")
    with torch.no_grad():  # eval mode, no grad: the fused kernel
        assert_close(net(x.detach()).cpu().numpy(), fx["pred"], REL_TOL, f"{name}: pred through the fused kernel")


def test_e2e_rff_adam_golden(amd):
    """Three Adam steps through training_step + autograd + the flat Adam kernel, under the yardstick's after-Adam factors:
    no worse than the reference's float32 parameters against the same steps in float64."""
    fx = load_golden("e2e_rff_adam")
    m = fx.meta
    net = net_from_fixture(fx).cuda()
    b_before = net.encoder.b.detach().clone()
    opt = net.configure_optimizers()
    linears = [l for l in net.decoder if isinstance(l, nn.Linear)]
    b64 = torch.from_numpy(fx["b"]).double()
    p64 = [torch.from_numpy(fx[f"{k}_{i}"]).double().requires_grad_(True) for i in range(m["n_layers"]) for k in ("w", "b")]
    opt64 = omlp.Adam([p.detach() for p in p64], lr=m["lr"])
    for s in range(m["steps"]):
        x, y = torch.from_numpy(fx[f"x_{s}"]), torch.from_numpy(fx[f"y_{s}"])
        opt.zero_grad()
        loss = net.training_step((x.cuda(), y.cuda()), s)
        loss.backward()
        opt.step()
        assert abs(float(loss) - float(fx[f"loss_{s}"])) <= REL_TOL * abs(float(fx[f"loss_{s}"]))
        h = encode_ref(x, b64, torch.float64)
        for i in range(m["n_layers"]):
            h = torch.relu(F.linear(h, p64[2 * i], p64[2 * i + 1]))
        opt64.step(torch.autograd.grad(((h - y.double()) ** 2).mean(), p64))
        for i, lin in enumerate(linears):
            assert_no_worse(lin.weight.detach().cpu().numpy(), fx[f"w_{s}_{i}"], p64[2 * i].detach().numpy(),
                            f"w{i} step {s}", max_factor=AFTER_ADAM_MAX_FACTOR)
            assert_no_worse(lin.bias.detach().cpu().numpy(), fx[f"b_{s}_{i}"], p64[2 * i + 1].detach().numpy(),
                            f"b{i} step {s}", max_factor=AFTER_ADAM_MAX_FACTOR)
    assert torch.equal(net.encoder.b, b_before) and opt.step_count == m["steps"]


# ============================================================================================ 5. dispatch
def spy_on_kernel(amd, monkeypatch):
    calls, real = [], amd.ops.rff_forward
    monkeypatch.setattr(amd.ops, "rff_forward", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def test_predict_step_takes_the_fused_kernel_where_supported(amd, monkeypatch):
    torch.manual_seed(5)
    net = amd.models.RffNet(3, 64, 1, 3, n_frequencies=64).cuda().eval()
    x = uniform((300, 3), 31).cuda()
    calls = spy_on_kernel(amd, monkeypatch)
    with torch.no_grad():
        want = net.decoder(net.encoder(x))
    assert calls == []
    y = net.predict_step((x, None), 0)
    assert calls == [1] and y.shape == (300, 1) and not y.requires_grad
    assert_close(y.cpu().numpy(), want.cpu().numpy(), REL_TOL, "predict_step against the layer path")
    with torch.no_grad():
        assert torch.equal(net(x), y) and calls == [1, 1]
    net(x)  # grad enabled: the differentiable layer path
    net.train()
    with torch.no_grad():
        net(x)
    assert calls == [1, 1]
    off = amd.models.RffNet(3, 64, 1, 3, n_frequencies=64, fused_inference=False).cuda().eval()
    assert off._inference_plan(x) is None
    assert off.predict_step((x, None), 0).shape == (300, 1) and calls == [1, 1]


@pytest.mark.parametrize("kw", [dict(n_frequencies=32), dict(activation=nn.GELU), dict(dim_hidden=32, n_frequencies=32)],
                         ids=["F_ne_H", "gelu", "hidden_32"])
def test_predict_step_takes_the_layer_path_elsewhere(amd, monkeypatch, kw):
    torch.manual_seed(6)
    args = dict(dim_in=3, dim_hidden=64, dim_out=1, n_layers=3, n_frequencies=64)
    args.update(kw)
    net = amd.models.RffNet(**args).cuda().eval()
    x = uniform((67, 3), 32).cuda()
    calls = spy_on_kernel(amd, monkeypatch)
    assert net._inference_plan(x) is None
    with torch.no_grad():
        want = net.decoder(net.encoder(x))
        y = net.predict_step((x, None), 0)
    assert calls == [] and torch.equal(y, want) and torch.isfinite(y).all()


# ============================================================================================ 6. launcher
def test_launcher_rffnet_save_gradient(amd, tmp_path, monkeypatch, capsys):
    """The issue's command line, in process (as tests/test_gpu_siren_gradient4d.py runs the launcher) so that the
    configuration can carry an interpolation grid: BaseConfig has none of its own.  4 batches of 4096 per epoch: the 20
    steps are 5 epochs."""
    import launcher
    from mri_interpolation_amd import config as cfg, nifti
    grid = (40, 24, 20)
    base = cfg.BaseConfig
    monkeypatch.setattr(cfg, "BaseConfig", lambda: dataclasses.replace(base(), interp_shapes=[grid]))
    out = tmp_path / "run"
    launcher.main(["--model_class", "RffNet", "--synthetic", "32,32,16", "--dim_hidden", "64", "--n_frequencies", "64",
                   "--n_layers", "3", "--max_steps", "20", "--save_gradient", "--epochs", "5", "--out_dir", str(out),
                   "--log_every", "1"])
    printed = capsys.readouterr().out
    losses = [float(line.split("loss")[1]) for line in printed.splitlines() if line.startswith("epoch ") and "loss" in line]
    assert len(losses) == 20 and np.isfinite(losses).all()
    # an epoch is a permutation of the same 16384 voxels in four batches: the means of two epochs compare like with like
    assert np.mean(losses[-4:]) < np.mean(losses[:4]), f"the loss does not fall: {losses}"
    pred = nifti.load(str(out / "pred.nii.gz"))
    assert pred.shape == (32, 32, 16) and np.isfinite(pred).all() and pred.min() >= 0
    grad = nifti.load(str(out / "gradient.nii.gz"))
    assert grad.shape == (32, 32, 16, 3) and grad.dtype == np.float32 and np.isfinite(grad).all()
    interp = sorted(p.name for p in out.iterdir() if p.name.startswith("interpolation"))
    assert interp == [f"interpolation{grid}.nii.gz"]
    vol = nifti.load(str(out / interp[0]))
    assert vol.shape == grid and np.isfinite(vol).all() and vol.max() > 0
    gvol = nifti.load(str(out / f"gradient_interpolation{grid}.nii.gz"))
    assert gvol.shape == grid + (3,) and np.isfinite(gvol).all()
    assert "n_frequencies : 64" in (out / "config.txt").read_text()
