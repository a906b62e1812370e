"""PsfSirenNet on the MI355X: the four PSF kernels (csrc/psf.hip) against torch / float64, the module path
and the fused PSF step against the reference's golden vectors, chunking, n_sample = 1, and the launcher."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REL_TOL, ROOT, assert_close, load_golden, rel_err
from yardstick import AFTER_ADAM_MAX_FACTOR, assert_no_worse
from oracle import detrand
from oracle import mlp as omlp

pytestmark = pytest.mark.gpu

SAMPLE_SPACING = (1.0 / 351.0, 1.0 / 351.0, 1.0 / 5.0)


@pytest.fixture(scope="module")
def amd():
    from mri_interpolation_amd import _lib, models, ops, trainer
    assert torch.cuda.is_available(), "these tests need the GPU"
    _lib.load()
    return type("NS", (), dict(lib=_lib, ops=ops, models=models, trainer=trainer))


def cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def rnd(n, seed, lo=-1.0, hi=1.0):
    return torch.from_numpy(detrand.uniform(n, seed, lo, hi))


def load_psf(amd, m, spacing=None):
    net = amd.models.PsfSirenNet(dim_in=m["dim_in"], dim_hidden=m["dim_hidden"], n_layers=m["n_layers"],
                                 coordinates_spacing=tuple(spacing or m["coordinates_spacing"]),
                                 n_sample=m["n_sample"], lr=m.get("lr", 1e-4))
    with torch.no_grad():
        for layer, (w, b) in zip(list(net.layers) + [net.last_layer],
                                 omlp.siren_init(m["dim_in"], m["dim_hidden"], 1, m["n_layers"], m["seed"])):
            layer.weight.copy_(w)
            layer.bias.copy_(b)
    return net.cuda()


class Psf64:
    """float64 yardstick: the oracle's SIREN through the PSF, the same op sequence on the same f32 inputs
    (the expansion is the f32 add both implementations do)."""

    def __init__(self, m, offsets, w):
        self.params = [(a.double().clone(), b.double().clone())
                       for a, b in omlp.siren_init(m["dim_in"], m["dim_hidden"], 1, m["n_layers"], m["seed"])]
        self.offsets, self.w = offsets.float().cpu(), w.double().cpu().reshape(-1)

    def parameters(self):
        return [t for wb in self.params for t in wb]

    def loss_and_grads(self, x, y):
        ps = self.parameters()
        for p in ps:
            p.requires_grad_(True)
            p.grad = None
        S, n = self.w.numel(), x.shape[0]
        xp = (x.float().cpu().repeat_interleave(S, 0) + self.offsets.repeat(n, 1)).double()
        z = omlp.siren_forward(xp, self.params)
        zbar = (z.reshape(n, S) * self.w).sum(1, keepdim=True)
        loss = omlp.mse_loss(zbar, y.double().cpu())
        loss.backward()
        grads = [p.grad.clone() for p in ps]
        for p in ps:
            p.requires_grad_(False)
        return float(loss), zbar.detach(), grads


def close_or_no_worse(kernel, ref, f64, what):
    """The parity bar; where the reference's own f32 evaluation is further than that from float64, the
    kernel must be no worse an evaluation than it (tests/yardstick.py)."""
    if max(rel_err(kernel, ref)) <= REL_TOL:
        return
    assert_no_worse(kernel, ref, f64, what)


# ------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("dim_in,spacing,n_sample", [(3, SAMPLE_SPACING, 5), (3, SAMPLE_SPACING, 3),
                                                     (4, (0.1, 0.2, 0.3), 3), (2, (0.05,), 7), (8, (0.1, 0.1), 4)])
def test_expand_is_the_torch_expression_bit_for_bit(amd, dim_in, spacing, n_sample):
    from mri_interpolation_amd import models
    off, _ = models.psf_table(spacing, n_sample, dim_in)
    n = 1001
    x = rnd(n * dim_in, 5, -1.0, 1.0).reshape(n, dim_in)
    want = x.repeat_interleave(off.shape[0], 0) + off.repeat(n, 1)
    got = amd.ops.psf_expand(x.cuda(), off.cuda())
    assert torch.equal(got.cpu(), want)
    # autograd: the expansion's backward sums each target's S rows
    xg = x.cuda().requires_grad_(True)
    g = rnd(n * off.shape[0] * dim_in, 6).reshape(-1, dim_in)
    amd.ops.psf_expand_ad(xg, off.cuda()).backward(g.cuda())
    want_dx = g.double().reshape(n, -1, dim_in).sum(1)
    assert max(rel_err(xg.grad.cpu().numpy(), want_dx.numpy())) <= 1e-6


@pytest.mark.parametrize("S,C", [(1, 1), (27, 1), (27, 3), (125, 1), (125, 8), (343, 2), (4096, 1)])
def test_reduce_broadcast_and_loss_against_float64(amd, S, C):
    ops = amd.ops
    n = 777 if S < 4096 else 37
    z = rnd(n * S * C, S + C).reshape(n * S, C).cuda()
    w = rnd(S, 3 * S, 0.0, 1.0).cuda()
    w64 = w.double().cpu()
    z64 = z.double().cpu().reshape(n, S, C)
    want = (z64 * w64[None, :, None]).sum(1)
    for ww, ref in ((w, want), (None, z64.sum(1))):
        a = ops.psf_reduce(z, S, ww)
        b = ops.psf_reduce(z, S, ww)
        assert torch.equal(a, b)
        assert max(rel_err(a.cpu().numpy(), ref.numpy())) <= 1e-6
    g = rnd(n, 9).reshape(n, 1).cuda()
    dz = ops.psf_broadcast(g, S, w, 0.5)
    ref = 0.5 * w64[None, :] * g.double().cpu()
    assert max(rel_err(dz.cpu().numpy().reshape(n, S), ref.numpy())) <= 1e-6
    if C != 1:
        return
    y = rnd(n, 11).cuda()
    out = []
    for _ in range(2):
        loss, zbar, d = torch.zeros(1, device="cuda"), torch.empty(n, device="cuda"), torch.empty(n * S, device="cuda")
        ops.psf_mse_loss(z.reshape(-1), y, S, w, loss, zbar, d, grad_divisor=2.0)
        out.append((loss, zbar, d))
    for u, v in zip(*out):
        assert torch.equal(u, v)
    loss, zbar, d = out[0]
    zb64 = (z64[..., 0] * w64).sum(1)
    diff64 = zbar.double().cpu() - y.double().cpu()
    assert max(rel_err(zbar.cpu().numpy(), zb64.numpy())) <= 1e-6
    assert abs(float(loss) - float(((zb64 - y.double().cpu()) ** 2).mean())) <= 1e-6 * float(loss)
    ref_d = w64[None, :] * (2.0 * diff64 / (n * 2.0))[:, None]
    assert max(rel_err(d.cpu().numpy().reshape(n, S), ref_d.numpy())) <= 1e-6


def test_sliced_loss_calls_add_up_to_the_whole(amd):
    ops, S, n = amd.ops, 27, 1000
    z = rnd(n * S, 21).cuda()
    y = rnd(n, 22).cuda()
    w = rnd(S, 23, 0.0, 1.0).cuda()
    whole = [torch.zeros(1, device="cuda"), torch.empty(n, device="cuda"), torch.empty(n * S, device="cuda")]
    ops.psf_mse_loss(z, y, S, w, whole[0], whole[1], whole[2])
    parts = [torch.zeros(1, device="cuda"), torch.empty(n, device="cuda"), torch.empty(n * S, device="cuda")]
    for lo, hi in ((0, 333), (333, 900), (900, 1000)):
        ops.psf_mse_loss(z[lo * S:hi * S], y[lo:hi], S, w, parts[0], parts[1][lo:hi], parts[2][lo * S:hi * S],
                         n_total=n)
    assert torch.equal(parts[1], whole[1]) and torch.equal(parts[2], whole[2])
    assert abs(float(parts[0]) - float(whole[0])) <= 1e-6 * float(whole[0])


# ------------------------------------------------------------------------------------------ models
@pytest.mark.parametrize("name", ["psf_siren_3d_4x64_ns5", "psf_siren_3d_6x128_ns3"])
def test_module_path_and_fused_step_match_the_reference(amd, name):
    fx = load_golden(name)
    m = fx.meta
    net = load_psf(amd, m)
    assert np.array_equal(net.psf_conv.weight.detach().cpu().numpy(), fx["psf_weight"])
    x, y = cuda(fx["x"]), cuda(fx["y"])
    y64 = Psf64(m, net.psf_coordinates, net.psf_weights())
    loss64, zbar64, grads64 = y64.loss_and_grads(x, y)
    layers = list(net.layers) + [net.last_layer]
    # module path: training_step + autograd over the HIP ops
    loss = net.training_step((x, y), 0)
    loss.backward()
    with torch.no_grad():
        zbar = amd.ops.psf_conv(net(net.x_to_psf_x(x)), net.psf_conv.weight)
    close_or_no_worse(zbar.cpu().numpy(), fx["zbar"], zbar64.numpy(), "zbar")
    assert abs(float(loss) - float(fx["loss"])) <= REL_TOL * abs(float(fx["loss"]))
    module_grads = []
    for i, layer in enumerate(layers):
        close_or_no_worse(layer.weight.grad.cpu().numpy(), fx[f"gw_{i}"], grads64[2 * i].numpy(), f"gw{i}")
        close_or_no_worse(layer.bias.grad.cpu().numpy(), fx[f"gb_{i}"], grads64[2 * i + 1].numpy(), f"gb{i}")
        module_grads += [layer.weight.grad.clone(), layer.bias.grad.clone()]
    # the fused PSF step on the chain kernels
    step = amd.trainer.FusedStep(net, net.configure_optimizers())
    assert step.use_chain and step.psf is not None and step.psf["S"] == m["n_sample"] ** 3
    w_before = net.psf_conv.weight.detach().clone()
    step.opt.step = lambda: None  # gradients only: keep the parameters for the comparison
    fused_loss = float(step.train_step(x, y))
    assert abs(fused_loss - float(fx["loss"])) <= REL_TOL * abs(float(fx["loss"]))
    for i, layer in enumerate(layers):
        gw, gb = step.flat.grad_view(layer.weight), step.flat.grad_view(layer.bias)
        close_or_no_worse(gw.cpu().numpy(), fx[f"gw_{i}"], grads64[2 * i].numpy(), f"fused gw{i}")
        close_or_no_worse(gb.cpu().numpy(), fx[f"gb_{i}"], grads64[2 * i + 1].numpy(), f"fused gb{i}")
        assert_close(gw.cpu().numpy(), module_grads[2 * i].cpu().numpy(), REL_TOL, f"fused vs module gw{i}")
        assert_close(gb.cpu().numpy(), module_grads[2 * i + 1].cpu().numpy(), REL_TOL, f"fused vs module gb{i}")
    assert torch.equal(net.psf_conv.weight, w_before)


def test_e2e_psf_adam_golden(amd):
    fx = load_golden("e2e_psf_adam")
    m = fx.meta
    net = load_psf(amd, m)
    w_before = net.psf_conv.weight.detach().clone()
    assert np.array_equal(w_before.cpu().numpy(), fx["psf_weight"])
    step = amd.trainer.FusedStep(net, net.configure_optimizers())
    assert step.use_chain and step.psf is not None
    y64 = Psf64(m, net.psf_coordinates, net.psf_weights())
    opt64 = omlp.Adam(y64.parameters(), lr=m["lr"])
    layers = list(net.layers) + [net.last_layer]
    for s in range(m["steps"]):
        x, y = cuda(fx[f"x_{s}"]), cuda(fx[f"y_{s}"])
        loss = float(step.train_step(x, y))
        assert abs(loss - float(fx[f"loss_{s}"])) <= REL_TOL * abs(float(fx[f"loss_{s}"]))
        _, _, g64 = y64.loss_and_grads(x, y)
        opt64.step(g64)
        for i, layer in enumerate(layers):
            w64, b64 = y64.params[i]
            assert_no_worse(layer.weight.detach().cpu().numpy(), fx[f"w_{s}_{i}"], w64.numpy(), f"w{i} step {s}",
                            max_factor=AFTER_ADAM_MAX_FACTOR)
            assert_no_worse(layer.bias.detach().cpu().numpy(), fx[f"b_{s}_{i}"], b64.numpy(), f"b{i} step {s}",
                            max_factor=AFTER_ADAM_MAX_FACTOR)
    assert torch.equal(net.psf_conv.weight, w_before)


def test_chunked_step_agrees_with_one_chunk(amd):
    m = dict(dim_in=3, dim_hidden=64, n_layers=3, n_sample=3, seed=95, coordinates_spacing=SAMPLE_SPACING)
    n = 300
    x = rnd(n * 3, 31).reshape(n, 3).cuda()
    y = rnd(n, 32).reshape(n, 1).cuda()
    out = []
    for budget in (1 << 20, 27 * 64):  # one chunk; chunks of 64 targets (the last one 44)
        net = load_psf(amd, m)
        step = amd.trainer.FusedStep(net, net.configure_optimizers(), psf_row_budget=budget)
        step.opt.step = lambda: None
        loss = float(step.train_step(x, y))
        out.append((loss, step.flat.grad.clone()))
    assert abs(out[0][0] - out[1][0]) <= 1e-6 * out[0][0]
    assert_close(out[1][1].cpu().numpy(), out[0][1].cpu().numpy(), 1e-6, "chunked gradient")


def test_one_sample_is_siren_at_the_shifted_point(amd):
    m = dict(dim_in=3, dim_hidden=128, n_layers=4, n_sample=1, seed=96, coordinates_spacing=(0.01, 0.02, 0.2))
    n = 500
    x = rnd(n * 3, 41).reshape(n, 3).cuda()
    y = rnd(n, 42).reshape(n, 1).cuda()
    psf = load_psf(amd, m)
    siren = amd.models.SirenNet(3, 128, 1, 4).cuda()
    siren.load_state_dict({k: v for k, v in psf.state_dict().items() if k != "psf_conv.weight"})
    shifted = x - torch.tensor(m["coordinates_spacing"], device="cuda")
    assert torch.equal(psf.x_to_psf_x(x), shifted)
    ps = amd.trainer.FusedStep(psf, psf.configure_optimizers())
    ss = amd.trainer.FusedStep(siren, siren.configure_optimizers())
    ps.opt.step = ss.opt.step = lambda: None
    lp = float(ps.train_step(x, y))
    _, ws = ss.forward(shifted, train=True)
    ss.backward(shifted, y, ws)
    assert abs(lp - float(ss.loss)) <= 1e-6 * lp
    assert_close(ps.flat.grad.cpu().numpy(), ss.flat.grad.cpu().numpy(), 1e-6, "gradients")


def test_unchained_width_trains_through_training_step(amd):
    """dim_hidden 96 has no chain kernel: FusedStep refuses, Trainer.fit runs training_step + autograd."""
    m = dict(dim_in=3, dim_hidden=96, n_layers=2, n_sample=3, seed=97, coordinates_spacing=SAMPLE_SPACING)
    net = load_psf(amd, m)
    with pytest.raises(ValueError, match="chain"):
        amd.trainer.FusedStep(net, net.configure_optimizers())
    n = 200
    x = rnd(n * 3, 51).reshape(n, 3).cuda()
    y = rnd(n, 52).reshape(n, 1).cuda()
    loss = net.training_step((x, y), 0)
    loss.backward()
    loss64, _, g64 = Psf64(m, net.psf_coordinates, net.psf_weights()).loss_and_grads(x, y)
    assert abs(float(loss) - loss64) <= REL_TOL * loss64
    for i, layer in enumerate(list(net.layers) + [net.last_layer]):
        assert_close(layer.weight.grad.cpu().numpy(), g64[2 * i].numpy(), REL_TOL, f"gw{i}")
    w = net.psf_conv.weight.detach().clone()
    tr = amd.trainer.Trainer(max_steps=2, distributed=False)
    tr.fit(net, [(x, y), (x, y)])
    assert tr.fused is None and tr.global_step == 2
    assert torch.equal(net.psf_conv.weight, w)


def test_launcher_end_to_end(amd, tmp_path):
    out = tmp_path / "run"
    cmd = [sys.executable, os.path.join(ROOT, "launcher.py"), "--model_class", "PsfSirenNet", "--synthetic",
           "32,32,8", "--n_sample", "3", "--max_steps", "20", "--dim_hidden", "64", "--n_layers", "3",
           "--out_dir", str(out), "--accelerator", "gpu", "--log_every", "5"]
    r = subprocess.run(["timeout", "-k", "10", "300"] + cmd, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert (out / "pred.nii.gz").exists()
    assert any(p.name.endswith(".ckpt") for p in (out / "checkpoints").iterdir())
    ck = torch.load(next((out / "checkpoints").iterdir()), map_location="cpu", weights_only=True)
    assert ck["state_dict"]["psf_conv.weight"].shape == (1, 1, 27)
