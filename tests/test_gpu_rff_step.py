"""The fused RffNet training step (csrc/rff.hip: rff_forward_kernel's training form, rff_backward_kernel,
rff_wgrad0_kernel) against float64 autograd of the formulas, the reference's fixtures, and the autograd path.

P = rows per tile of the chain kernels: 64 at hidden 128, 128 at hidden 64; at most 256 workgroups walk the tiles.

ReLU kinks.  A pre-activation within rounding of zero makes two correct float32 evaluations differ by a whole gradient
term, so the inputs of the selected-row tests are chosen on the CPU from the float64 reference alone, before anything
runs on the GPU, and nothing is excluded from any comparison afterwards: sigma = 1, He-uniform weights (bound
sqrt(6 / fan_in)), x uniform in [0, 1] (oracle.detrand), the head's bias minus the median of the float64 head dot
product (about half the outputs live: asserted within [0.2, 0.8]); kept are the rows whose EVERY float64
pre-activation, in all Linears, is at least 2e-5 from zero (at most 3 % of the drawn rows may go: asserted), and the
float32 CPU evaluation must have the float64 sign pattern on every kept row (asserted).  20480 rows are drawn at
hidden 128 and 36864 at hidden 64, so that the kept rows fill more than 256 tiles.

The comparison rule is tests/test_gpu_modsiren.py's close_or_no_worse: within REL_TOL of float64, else no worse a
float32 evaluation than the CPU's (yardstick.assert_no_worse)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import REL_TOL, ROOT, assert_close, load_golden, rel_err
from layout import place, ptr
from test_gpu_workspace import arr, hold
from test_rff_cpu import net_from_fixture
from yardstick import AFTER_ADAM_MAX_FACTOR, assert_no_worse
from oracle import detrand
from oracle import mlp as omlp

pytestmark = pytest.mark.gpu

ROWS = {128: 64, 64: 128}
DRAWN = {128: 20480, 64: 36864}
MARGIN = 2e-5
TWO_PI = np.float32(2 * np.pi)  # fl32(2 pi): `2 * np.pi * v` on a float32 tensor
SHAPES = [(3, 128, 6), (2, 64, 3), (1, 64, 2), (4, 64, 8), (3, 128, 2)]


@pytest.fixture(scope="module")
def amd():
    from mri_interpolation_amd import _lib, config, datamodules, models, ops, trainer
    assert torch.cuda.is_available(), "these tests need the GPU"
    return type("NS", (), dict(lib=_lib, h=_lib.load(), ops=ops, models=models, trainer=trainer, config=config,
                               datamodules=datamodules))


def close_or_no_worse(kernel, f32_ref, f64, what):
    """Within REL_TOL of float64, or no worse an f32 evaluation than the CPU's (yardstick: factor 2, floor 1e-6)."""
    e_max, e_l2 = rel_err(kernel, f64)
    print(f"{what}: kernel {e_max:.2e} / {e_l2:.2e} from float64")
    if e_max <= REL_TOL and e_l2 <= REL_TOL:
        return
    assert_no_worse(kernel, f32_ref, f64, what)


def scalar(v):
    return np.array([float(v)])


def uniform(shape, seed, lo=0.0, hi=1.0):
    return torch.from_numpy(detrand.uniform(int(np.prod(shape)), seed, lo, hi).reshape(shape).copy())


# ------------------------------------------------------------------------------------------ float64 / float32 CPU
class RffRef:
    """The formulas of RffNet on the CPU in `dtype`, gradients by autograd.  The scaling by fl32(2 pi) is the
    reference's float32 op; the float64 evaluation runs the same op sequence on the same float32 inputs."""

    def __init__(self, b, params, dtype):
        self.b, self.dtype = b.detach().to(dtype), dtype
        self.params = [(w.detach().to(dtype).clone().requires_grad_(True),
                        v.detach().to(dtype).clone().requires_grad_(True)) for w, v in params]

    def parameters(self):  # (w, b) per Linear, the head last
        return [t for wb in self.params for t in wb]

    def encode(self, x):
        if self.dtype == torch.float64:
            vp = (float(TWO_PI) * x.to(self.dtype)) @ self.b.T
        else:
            vp = (TWO_PI * x) @ self.b.T
        return torch.cat((torch.cos(vp), torch.sin(vp)), dim=-1)

    def preactivations(self, x):
        out = []
        with torch.no_grad():
            h = self.encode(x.cpu())
            for w, v in self.params:
                out.append(F.linear(h, w, v))
                h = torch.relu(out[-1])
        return out

    def loss_and_grads(self, x, y, n_total=None, divisor=1.0):
        x, y = x.cpu(), y.cpu().to(self.dtype).reshape(-1, 1)
        h = self.encode(x)
        for w, v in self.params:
            h = torch.relu(F.linear(h, w, v))
        n_total = x.shape[0] if n_total is None else n_total
        loss = ((h - y) ** 2).sum() / n_total
        grads = torch.autograd.grad(loss / divisor, self.parameters())
        return h.detach(), loss.detach(), [g.detach() for g in grads]


def he_init(d, hidden, L, seed, sigma):
    """b (hidden, d) ~ N(0, sigma^2) and the Linears' (weight, bias): uniform in He's bound sqrt(6 / fan_in)."""
    b = torch.randn((hidden, d), generator=torch.Generator().manual_seed(seed)) * sigma
    params = []
    for i in range(L):
        fan_in, fan_out = (2 * hidden if i == 0 else hidden), (1 if i == L - 1 else hidden)
        bound = float(np.sqrt(6.0 / fan_in))
        params.append((uniform((fan_out, fan_in), seed + 10 * i + 1, -bound, bound),
                       uniform((fan_out,), seed + 10 * i + 2, -0.1, 0.1)))
    return b, params


@functools.lru_cache(maxsize=None)
def selected_rows(d, H, L, drawn=None):
    """x, y, b, params, float64 and float32 references of the rows that stay clear of every ReLU kink, with the
    conditions the module docstring states.  Chosen from the float64 reference alone."""
    seed = 9500 + H + L + 10 * d
    drawn = DRAWN[H] if drawn is None else drawn
    x = uniform((drawn, d), seed + 5)
    y = uniform((drawn, 1), seed + 6)
    b, params = he_init(d, H, L, seed, sigma=1.0)
    pre = RffRef(b, params, torch.float64).preactivations(x)
    dot = pre[-1].reshape(-1) - params[-1][1].double()
    params = params[:-1] + [(params[-1][0], (-dot.median()).float().reshape(1))]
    r64, r32 = RffRef(b, params, torch.float64), RffRef(b, params, torch.float32)
    pre64 = r64.preactivations(x)
    live = float((pre64[-1] > 0).double().mean())
    assert 0.2 <= live <= 0.8, f"({d}, {H}, {L}): {live:.3f} of the outputs are live"
    keep = torch.ones(drawn, dtype=torch.bool)
    for p in pre64:
        keep &= (p.abs() >= MARGIN).all(dim=1)
    dropped = 1.0 - float(keep.float().mean())
    print(f"({d}, {H}, {L}): {100 * dropped:.3f} % of the drawn rows within {MARGIN} of a kink, {live:.3f} live")
    assert dropped <= 0.03
    x, y = x[keep].contiguous(), y[keep].contiguous()
    for a, c in zip(r64.preactivations(x), r32.preactivations(x)):
        assert torch.equal(a > 0, c > 0), "float32 and float64 disagree on a ReLU sign of a selected row"
    return x, y, b, params, r64, r32


def device_params(b, params):
    return b.cuda(), [w.cuda() for w, _ in params], [v.cuda() for _, v in params]


def kernel_pass(amd, b, params, x, y, n_total=None, divisor=1.0, grads=None):
    """ops.rff_forward_loss + rff_backward; gradients (w, b per Linear, RffRef.parameters()'s order) start at zero or
    at `grads`, which are added to.  Returns (y, dy, loss, gradients) on the device."""
    ops = amd.ops
    bc, ws, bs = device_params(b, params)
    n, L, H = x.shape[0], len(ws), ws[0].shape[0]
    new = lambda *s: torch.empty(*s, device="cuda")  # noqa: E731
    act, dz = [new(n, H) for _ in range(L - 1)], [new(n, H) for _ in range(L - 1)]
    yk, dy, loss = new(n, 1), new(n, 1), torch.zeros(1, device="cuda")
    if grads is None:
        grads = [torch.zeros_like(t) for pair in zip(ws, bs) for t in pair]
    xg, tg = x.cuda(), y.cuda()
    ops.rff_forward_loss(xg, tg, bc, ws, bs, act, yk, dy, loss, n_total=n_total, grad_divisor=divisor)
    ops.rff_backward(xg, dy, bc, ws, act, dz, grads[0::2], grads[1::2])
    return yk, dy, loss, grads


def names(L):
    return [f"{'w' if j == 0 else 'b'}{i}" for i in range(L) for j in range(2)]


# ------------------------------------------------------------------------------------------ 1. kernels vs float64
@pytest.mark.parametrize("d,H,L", SHAPES)
def test_kernels_against_float64(amd, d, H, L):
    assert amd.ops.rff_train_supported(d, H, H, L, 1)
    x_all, y_all, b, params, r64, r32 = selected_rows(d, H, L)
    P = ROWS[H]
    assert x_all.shape[0] > 256 * P, "every workgroup's persistent loop passes its first tile"
    bc, ws, bs = device_params(b, params)
    for n in (x_all.shape[0], 1, P - 1, P + 1, 2 * P + 3):
        x, y = x_all[:n], y_all[:n]
        p64, l64, g64 = r64.loss_and_grads(x, y)
        p32, l32, g32 = r32.loss_and_grads(x, y)
        pk, dy, lk, gk = kernel_pass(amd, b, params, x, y)
        assert torch.equal(pk, amd.ops.rff_forward(x.cuda(), bc, ws, bs)), "training and inference y differ"
        tag = f"({d}, {H}, {L}) n = {n}: "
        close_or_no_worse(pk.cpu().numpy(), p32.numpy(), p64.numpy(), tag + "y")
        close_or_no_worse(scalar(lk), scalar(l32), scalar(l64), tag + "loss")
        for name, a, c32, c64 in zip(names(L), gk, g32, g64):
            assert a.shape == c64.shape
            close_or_no_worse(a.cpu().numpy(), c32.numpy(), c64.numpy(), tag + name)


# ------------------------------------------------------------------------------------------ 2. the reference's fixtures
def fused_step(amd, net):
    step = amd.trainer.FusedStep(net, net.configure_optimizers(), rff=True)
    assert step.use_rff and not step.use_chain and not step.use_tiny and step.encoder is None
    return step


def fixture_ref(fx, dtype):
    return RffRef(torch.from_numpy(fx["b"]), [(torch.from_numpy(fx[f"w_{i}"]), torch.from_numpy(fx[f"b_{i}"]))
                                              for i in range(fx.meta["n_layers"])], dtype)


@pytest.mark.parametrize("name", ["rff_2d_3x64", "rff_3d_6x128"])
def test_fixtures_through_the_fused_step(amd, name):
    fx = load_golden(name)
    m = fx.meta
    assert m["min_abs_preactivation"] >= 1e-5
    net = net_from_fixture(fx).cuda()
    step = fused_step(amd, net)
    x, y = torch.from_numpy(fx["x"]), torch.from_numpy(fx["y"])
    p64, l64, g64 = fixture_ref(fx, torch.float64).loss_and_grads(x, y)
    pred = step.forward(x.cuda(), train=False)[0]
    close_or_no_worse(pred.cpu().numpy(), fx["pred"], p64.numpy(), f"{name}: pred")
    loss = float(step.train_step(x.cuda(), y.cuda(), step=False))
    close_or_no_worse(scalar(loss), scalar(fx["loss"]), scalar(l64), f"{name}: loss")
    r = step.rff
    for i in range(m["n_layers"]):
        close_or_no_worse(r["d_weights"][i].cpu().numpy(), fx[f"gw_{i}"], g64[2 * i].numpy(), f"{name}: gw{i}")
        close_or_no_worse(r["d_biases"][i].cpu().numpy(), fx[f"gb_{i}"], g64[2 * i + 1].numpy(), f"{name}: gb{i}")
    # encoder.b is in no flat buffer
    assert len(step.flat.params) == 2 * m["n_layers"] and all(p is not net.encoder.b for p in step.flat.params)


# ------------------------------------------------------------------------------------------ 3. three Adam steps
def test_e2e_rff_adam_golden(amd):
    fx = load_golden("e2e_rff_adam")
    m = fx.meta
    net = net_from_fixture(fx).cuda()
    b_before = net.encoder.b.detach().clone()
    step = fused_step(amd, net)
    linears = [l for l in net.decoder if isinstance(l, nn.Linear)]
    r64 = fixture_ref(fx, torch.float64)
    opt64 = omlp.Adam([p.detach() for p in r64.parameters()], lr=m["lr"])
    for s in range(m["steps"]):
        x, y = torch.from_numpy(fx[f"x_{s}"]), torch.from_numpy(fx[f"y_{s}"])
        loss = float(step.train_step(x.cuda(), y.cuda()))
        assert abs(loss - float(fx[f"loss_{s}"])) <= REL_TOL * abs(float(fx[f"loss_{s}"]))
        _, _, g64 = r64.loss_and_grads(x, y)
        opt64.step(g64)
        for i, lin in enumerate(linears):
            w64, b64 = r64.params[i]
            assert_no_worse(lin.weight.detach().cpu().numpy(), fx[f"w_{s}_{i}"], w64.detach().numpy(),
                            f"w{i} step {s}", max_factor=AFTER_ADAM_MAX_FACTOR)
            assert_no_worse(lin.bias.detach().cpu().numpy(), fx[f"b_{s}_{i}"], b64.detach().numpy(),
                            f"b{i} step {s}", max_factor=AFTER_ADAM_MAX_FACTOR)
    assert torch.equal(net.encoder.b, b_before) and step.opt.step_count == m["steps"]


# ------------------------------------------------------------------------------------------ 4. two evaluations agree
def load_net(amd, d, H, L, b, params, lr=1e-4):
    net = amd.models.RffNet(dim_in=d, dim_hidden=H, dim_out=1, n_layers=L, n_frequencies=H, sigma=1.0, lr=lr)
    sd = {"encoder.b": b}
    for i, (w, v) in enumerate(params):
        sd[f"decoder.{2 * i}.weight"], sd[f"decoder.{2 * i}.bias"] = w, v
    net.load_state_dict(sd)
    return net.cuda()


def test_autograd_path_and_fused_pass_agree(amd):
    d, H, L = 3, 128, 4
    x, y, b, params, r64, _ = selected_rows(d, H, L)
    net = load_net(amd, d, H, L, b, params)
    step = fused_step(amd, net)
    xg, yg = x.cuda(), y.cuda()
    loss_f = step.train_step(xg, yg, step=False).cpu().clone()
    linears = [l for l in net.decoder if isinstance(l, nn.Linear)]
    tensors = [t for l in linears for t in (l.weight, l.bias)]
    # the flat buffer holds the decoder's parameters in the reference's order, and nothing else
    assert len(step.flat.params) == len(tensors) and all(p is t for p, t in zip(step.flat.params, tensors))
    flat = step.flat.grad.detach().cpu().clone()
    g_fused = [flat[off:off + t.numel()].view(t.shape) for off, t in zip(step.flat.offsets, tensors)]
    loss_m = net.training_step((xg, yg), 0)
    g_module = [g.cpu() for g in torch.autograd.grad(loss_m, tensors)]
    _, l64, g64 = r64.loss_and_grads(x, y)
    close_or_no_worse(scalar(loss_f), scalar(loss_m.detach()), scalar(l64), "loss")
    for name, a, c32, c64 in zip(names(L), g_fused, g_module, g64):
        close_or_no_worse(a.numpy(), c32.numpy(), c64.numpy(), f"gradient {name}")
    # what lies between the parameters (each starts on a 16-byte boundary) stays zero
    covered = torch.zeros(flat.numel(), dtype=torch.bool)
    for off, t in zip(step.flat.offsets, tensors):
        covered[off:off + t.numel()] = True
    assert bool((flat[~covered] == 0).all())


# ------------------------------------------------------------------------------------------ 5. bitwise reproducibility
@pytest.mark.parametrize("n", [70001, 1 << 16])
def test_bitwise_reproducible(amd, n):
    d, H, L = 3, 128, 6
    b, params = he_init(d, H, L, 41, sigma=10.0)
    step = fused_step(amd, load_net(amd, d, H, L, b, params))
    x, y = uniform((n, d), 42).cuda(), uniform((n, 1), 43).cuda()
    out = []
    for _ in range(2):
        loss = step.train_step(x, y, step=False)
        out.append((loss.clone(), step.flat.grad.clone()))
    assert torch.isfinite(out[0][1]).all() and float(out[0][1].abs().max()) > 0
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


# ------------------------------------------------------------------------------------------ 6. accumulation
def test_accumulation(amd):
    d, H, L = 2, 64, 3
    x, y, b, params, r64, r32 = selected_rows(d, H, L)
    x, y = x[:4001], y[:4001]
    n, cut = x.shape[0], 1777
    _, _, g64 = r64.loss_and_grads(x, y)
    _, l32, g32 = r32.loss_and_grads(x, y)
    # two slices of one batch: n_total = n, the second call adds to what the first left
    _, _, loss_a, grads = kernel_pass(amd, b, params, x[:cut], y[:cut], n_total=n)
    _, _, loss_b, grads = kernel_pass(amd, b, params, x[cut:], y[cut:], n_total=n, grads=grads)
    _, l64, _ = r64.loss_and_grads(x, y)
    close_or_no_worse(scalar(float(loss_a) + float(loss_b)), scalar(l32), scalar(l64), "two slices: loss")
    for name, a, c32, c64 in zip(names(L), grads, g32, g64):
        close_or_no_worse(a.cpu().numpy(), c32.numpy(), c64.numpy(), f"two slices: {name}")
    # gradients are ADDED: a constant in the buffers comes back under the zero-start result, one rounding apart
    const = 0.25
    _, _, _, zero = kernel_pass(amd, b, params, x, y)
    filled = [torch.full_like(t, const) for t in zero]
    _, _, _, filled = kernel_pass(amd, b, params, x, y, grads=filled)
    for name, f, z in zip(names(L), filled, zero):
        f, z = f.double().cpu(), z.double().cpu()
        assert bool(((f - const - z).abs() <= 2.0 ** -24 * f.abs()).all()), f"prefilled {name}: not const + gradient"
        assert float(z.abs().max()) > 0
    # FusedStep: first=True starts afresh, first=False adds
    step = fused_step(amd, load_net(amd, d, H, L, b, params))
    xg, yg = x.cuda(), y.cuda()
    step.train_step(xg, yg, first=True, step=False)
    once = step.flat.grad.clone()
    step.train_step(xg, yg, first=True, step=False, divisor=2.0)
    step.train_step(xg, yg, first=False, step=False, divisor=2.0)
    assert_close(step.flat.grad.cpu().numpy(), once.cpu().numpy(), REL_TOL, "two half-weighted passes")


# ------------------------------------------------------------------------------------------ 7. exact zeros
@pytest.mark.parametrize("d,H,L", [(3, 128, 4), (2, 64, 3)])
def test_exact_zeros(amd, d, H, L):
    n = 2 * ROWS[H] + 3
    x, y = uniform((n, d), 71), uniform((n, 1), 72, 0.1, 1.0)
    b, params = he_init(d, H, L, 73, sigma=1.0)
    dead = params[:-1] + [(params[-1][0], torch.full((1,), -100.0))]
    yk, dy, loss, grads = kernel_pass(amd, b, dead, x, y)
    assert bool((yk == 0).all()) and bool((dy == 0).all())
    assert all(bool((g == 0).all()) for g in grads), "a dead head passes no gradient"
    want = float((y.double() ** 2).mean())
    assert abs(float(loss) - want) <= REL_TOL * want
    # every pre-activation exactly 0: ReLU'(0) = 0
    zeros = [(torch.zeros_like(w), torch.zeros_like(v)) for w, v in params]
    yk, dy, loss, grads = kernel_pass(amd, b, zeros, x, y)
    assert bool((yk == 0).all()) and bool((dy == 0).all())
    assert all(bool((g == 0).all()) for g in grads), "ReLU'(0) = 0"
    assert abs(float(loss) - want) <= REL_TOL * want


# ------------------------------------------------------------------------------------------ 8. guard bands, workspace
@pytest.mark.parametrize("d,H,L", [(3, 128, 3), (2, 64, 3)])
def test_guard_bands(amd, d, H, L):
    x_all, y_all, b, params, r64, r32 = selected_rows(d, H, L)
    bc, ws, bs = device_params(b, params)
    st = amd.ops._stream()
    for n in (1, ROWS[H] + 1):
        x, y = x_all[:n], y_all[:n]
        checks = []

        def put(shape, offset=0, fill=float("nan")):
            view, check = place(torch.full(shape, fill), offset)
            checks.append(check)
            return view
        act, dz = [put((n, H)) for _ in range(L - 1)], [put((n, H)) for _ in range(L - 1)]
        yk, dy, loss = put((n,), 1), put((n,), 3), put((1,), 2, 0.0)
        gw, gb = [put(tuple(w.shape), 0, 0.0) for w in ws], [put(tuple(v.shape), 1, 0.0) for v in bs]
        need = amd.h.mri_rff_backward_workspace_bytes(n, H, L)
        wsp = torch.empty((need + 3) // 4, device="cuda")
        xg, tg = x.cuda(), y.reshape(-1).cuda()
        amd.lib.call("mri_rff_forward_loss", ptr(xg), ptr(tg), n, n, d, H, H, L, ptr(bc), arr(ws), arr(bs), 1.0,
                     arr(act), ptr(yk), ptr(dy), ptr(loss), ptr(wsp), need, st)
        amd.lib.call("mri_rff_backward", ptr(xg), ptr(dy), n, d, H, H, L, ptr(bc), arr(ws), arr(act), arr(dz),
                     arr(gw), arr(gb), ptr(wsp), need, st)
        for check in checks:
            check(what=f"({d}, {H}, {L}) n = {n}")
        assert all(bool(torch.isfinite(t).all()) for t in act + dz + [yk, dy, loss] + gw + gb), "an element was not stored"
        p64, l64, g64 = r64.loss_and_grads(x, y)
        p32, l32, g32 = r32.loss_and_grads(x, y)
        close_or_no_worse(yk.cpu().numpy(), p32.numpy().reshape(-1), p64.numpy().reshape(-1), f"n = {n}: y")
        got = [t for pair in zip(gw, gb) for t in pair]
        for name, a, c32, c64 in zip(names(L), got, g32, g64):
            close_or_no_worse(a.cpu().numpy(), c32.numpy(), c64.numpy(), f"n = {n}: {name}")


def train_entry(amd, d, H, L, n):
    x, y, b, params, r64, r32 = selected_rows(d, H, L)
    xg, tg = x[:n].cuda(), y[:n].reshape(-1).cuda()
    bc, ws, bs = device_params(b, params)
    st = amd.ops._stream()

    def launch(run, wsp, nb):
        act, dz = [run.scratch((n, H)) for _ in range(L - 1)], [run.scratch((n, H)) for _ in range(L - 1)]
        yk, dy, loss = run.out((n,)), run.out((n,)), run.out((1,), 0.0)
        gw, gb = [run.out(w.shape, 0.0) for w in ws], [run.out(v.shape, 0.0) for v in bs]
        amd.lib.call("mri_rff_forward_loss", ptr(xg), ptr(tg), n, n, d, H, H, L, ptr(bc), arr(ws), arr(bs), 1.0,
                     arr(act), ptr(yk), ptr(dy), ptr(loss), ptr(wsp), nb, st)
        amd.lib.call("mri_rff_backward", ptr(xg), ptr(dy), n, d, H, H, L, ptr(bc), arr(ws), arr(act), arr(dz),
                     arr(gw), arr(gb), ptr(wsp), nb, st)
        out = dict(y=yk, dy=dy, loss=loss)
        for i in range(L):
            out[f"w{i}"], out[f"b{i}"] = gw[i], gb[i]
        return out

    refs = (r32.loss_and_grads(x[:n], y[:n]), r64.loss_and_grads(x[:n], y[:n]))
    return launch, amd.h.mri_rff_backward_workspace_bytes(n, H, L), refs


@pytest.mark.parametrize("d,H,L,n", [(2, 64, 3, 2 * 128 + 3), (3, 128, 2, 256 * 64 + 5)])
def test_workspace_contract(amd, d, H, L, n):
    """tests/test_gpu_workspace.py `hold`: exactly the reported size between guards, zero-filled, after a larger call of
    another shape on the same buffer, filled with two bit patterns (0xFFFFFFFF: NaN) -- bitwise equal outputs --, and one
    byte short refused with the outputs and the guards untouched."""
    launch, need, ((p32, l32, g32), (p64, l64, g64)) = train_entry(amd, d, H, L, n)
    assert need > 0 and need % 16 == 0
    big = train_entry(amd, 3, 128, 6, 16400)[:2]  # the largest workspace of the supported widths at this depth
    assert big[1] > need

    def judge(got):
        close_or_no_worse(got["y"].numpy(), p32.numpy().reshape(-1), p64.numpy().reshape(-1), "workspace: y")
        close_or_no_worse(got["loss"].numpy(), scalar(l32), scalar(l64), "workspace: loss")
        for i, name in enumerate(names(L)):
            close_or_no_worse(got[name].numpy(), g32[i].numpy(), g64[i].numpy(), f"workspace: {name}")
    hold(f"fused RFF step {d} -> {H} x {L}, n = {n}:", launch, need, judge, big)


# ------------------------------------------------------------------------------------------ 9. Trainer and launcher
def _phantom_run(amd, **trainer_kw):
    torch.manual_seed(0)
    vol = amd.datamodules.phantom_volume((32, 32, 32)).contiguous().cpu().numpy()
    c = amd.config.BaseConfig().resolve(vol.shape)
    c.batch_size = 4096
    net = amd.models.RffNet(dim_in=3, dim_hidden=64, dim_out=1, n_layers=3, n_frequencies=64, sigma=2.0, lr=1e-3)
    dm = amd.datamodules.MriDataModule(config=c, volume=vol)
    dm.prepare_data()
    tr = amd.trainer.Trainer(max_epochs=3, log_every=1, **trainer_kw)
    tr.fit(net, dm.train_dataloader())
    return tr, net, dm


def test_trainer_opt_in(amd):
    tr, net, dm = _phantom_run(amd, fused_rff=True)
    assert tr.fused is not None and tr.fused.use_rff
    assert len(tr.history) == tr.global_step == 24 and np.isfinite(tr.history).all()
    assert tr.history[-1] < tr.history[0]
    pred = torch.cat(tr.predict(net, dm.test_dataloader()))
    assert pred.shape == (32 ** 3, 1) and bool(torch.isfinite(pred).all()) and float(pred.min()) >= 0
    twin, _, _ = _phantom_run(amd)  # the default keyword: training_step + autograd
    assert twin.fused is None and len(twin.history) == 24
    # the first step sees the same parameters and the same batch on both paths
    assert abs(tr.history[0] - twin.history[0]) <= REL_TOL * abs(twin.history[0]), (tr.history[0], twin.history[0])
    assert twin.history[-1] < twin.history[0]


def test_steady_loop_refuses_the_rff_plan(amd):
    b, params = he_init(2, 64, 3, 61, sigma=1.0)
    step = fused_step(amd, load_net(amd, 2, 64, 3, b, params))
    pipe = type("Pipe", (), dict(loader=None, group=1))()
    why = amd.trainer.SteadyLoop.unsupported(step, pipe)
    assert why and "RffNet" in why
    # the loss is taken inside the forward kernel: there is no separate forward(train=True) / backward() pair
    x = uniform((5, 2), 62).cuda()
    with pytest.raises(RuntimeError, match="train_step"):
        step.forward(x, train=True)
    with pytest.raises(RuntimeError, match="train_step"):
        step.backward(x, x[:, :1], None)


def test_launcher_fused_rff(tmp_path):
    out = str(tmp_path / "run")
    cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "launcher.py"), "--model_class", "RffNet",
           "--fused_rff", "--synthetic", "32,32,16", "--dim_hidden", "64", "--n_frequencies", "64", "--n_layers", "3",
           "--epochs", "2", "--batch_size", "4096", "--log_every", "0", "--out_dir", out]
    done = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout[-2000:]
    txt = open(os.path.join(out, "config.txt")).read()
    assert "model_class : RffNet" in txt
    assert os.path.exists(os.path.join(out, "pred.nii.gz"))
