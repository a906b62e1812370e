"""The fused modulated SIREN step (csrc/modsiren.hip, FusedStep(modulated=True)) on the MI355X:
1. the kernels against the float64 autograd of the formulas;  2. the reference's fixtures through FusedStep;
3. three Adam steps against e2e_modsiren_adam;  4. autograd path and fused pass agree;  5. bitwise reproducibility;
6. gradient accumulation;  7. inference;  8. Trainer(fused_modulated=True);  9. launcher --fused_modulated.

ReLU kinks: a modulator pre-activation within rounding of zero makes two correct f32 evaluations differ by a whole
term (tests/test_gpu_shallow.py section 2), so section 1 SELECTS its inputs on the CPU before anything runs: of 16384
drawn rows it keeps those whose every float64 pre-activation is at least 1e-6 from zero (at most 3 % may go), and
checks that the float32 CPU evaluation has the float64 sign pattern on them.  Nothing is excluded from a comparison.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import REL_TOL, assert_close, load_golden, rel_err
from yardstick import AFTER_ADAM_MAX_FACTOR, assert_no_worse
from oracle import detrand
from oracle import mlp as omlp

pytestmark = pytest.mark.gpu

W0 = 30.0
SHAPES = [(2, 64, 3), (3, 128, 4), (3, 128, 6), (1, 64, 2), (8, 128, 6), (3, 64, 8)]


@pytest.fixture(scope="module")
def amd():
    from mri_interpolation_amd import _lib, config, datamodules, models, ops, trainer
    assert torch.cuda.is_available(), "these tests need the GPU"
    _lib.load()
    return type("NS", (), dict(lib=_lib, ops=ops, models=models, trainer=trainer, config=config,
                               datamodules=datamodules))


def cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def close_or_no_worse(kernel, f32_ref, f64, what):
    """The rule of section 1: within REL_TOL of float64, or no worse an f32 evaluation than the CPU's."""
    e_max, e_l2 = rel_err(kernel, f64)
    print(f"{what}: kernel {e_max:.2e} / {e_l2:.2e} from float64")
    if e_max <= REL_TOL and e_l2 <= REL_TOL:
        return
    assert_no_worse(kernel, f32_ref, f64, what)


# ------------------------------------------------------------------------------------------ float64 / float32 CPU
class ModRef:
    """The formulas of ModulatedSirenNet on the CPU in `dtype`, gradients by autograd."""

    def __init__(self, d, H, L, seed, dtype):
        self.siren = [(w.to(dtype).requires_grad_(True), b.to(dtype).requires_grad_(True))
                      for w, b in omlp.siren_init(d, H, 1, L, seed)]
        self.mod = [(w.to(dtype).requires_grad_(True), b.to(dtype).requires_grad_(True))
                    for w, b in omlp.modulator_init(d, H, L, seed + 500)]
        self.dtype = dtype

    def parameters(self):  # SIREN layers, head, modulator layers: (w, b) each
        return [t for wb in self.siren + self.mod for t in wb]

    def preactivations(self, x):
        z = x.to(self.dtype)
        h, out = z, []
        with torch.no_grad():
            for w, b in self.mod:
                pm = F.linear(h, w, b)
                out.append(pm)
                h = torch.cat((torch.relu(pm), z), dim=1)
        return out

    def loss_and_grads(self, x, y, n_total=None, divisor=1.0):
        x, y = x.cpu().to(self.dtype), y.cpu().to(self.dtype).reshape(-1, 1)
        pred = omlp.modulated_siren_forward(x, self.siren, self.mod, W0, W0)
        n_total = x.shape[0] if n_total is None else n_total
        loss = ((pred - y) ** 2).sum() / n_total
        grads = torch.autograd.grad(loss / divisor, self.parameters())
        return pred.detach(), loss.detach(), [g.detach() for g in grads]


def selected_rows(d, H, L, seed, drawn=16384):
    """x, y of the rows that stay clear of every ReLU kink, with the conditions the module docstring states."""
    x = torch.from_numpy(detrand.uniform(drawn * d, seed + 1, -1.0, 1.0).reshape(drawn, d))
    y = torch.from_numpy(detrand.uniform(drawn, seed + 2, -1.0, 1.0).reshape(drawn, 1))
    r64, r32 = ModRef(d, H, L, seed, torch.float64), ModRef(d, H, L, seed, torch.float32)
    pm64 = r64.preactivations(x)
    keep = torch.ones(drawn, dtype=torch.bool)
    for pm in pm64:
        keep &= (pm.abs() >= 1e-6).all(dim=1)
    dropped = 1.0 - float(keep.float().mean())
    print(f"({d}, {H}, {L}): {100 * dropped:.3f} % of the drawn rows within 1e-6 of a kink")
    assert dropped <= 0.03
    x, y = x[keep].contiguous(), y[keep].contiguous()
    for a, b in zip(r64.preactivations(x), r32.preactivations(x)):
        assert torch.equal(a > 0, b > 0), "float32 and float64 disagree on a ReLU sign of a selected row"
    return x, y, r64, r32


def kernel_loss_and_grads(amd, r32, x, y):
    """ops.modsiren_forward_loss + modsiren_backward on zeroed gradients; the order of ModRef.parameters()."""
    ops = amd.ops
    sw, sb = [w.detach().cuda() for w, _ in r32.siren], [b.detach().cuda() for _, b in r32.siren]
    mw, mb = [w.detach().cuda() for w, _ in r32.mod], [b.detach().cuda() for _, b in r32.mod]
    n, L, H = x.shape[0], len(mw), mw[0].shape[0]
    new = lambda *s: torch.empty(*s, device="cuda")  # noqa: E731
    saved = {k: [new(n, H) for _ in range(L)] for k in ("act", "hid", "dcos", "sn")}
    dz = [[None] + [new(n, H) for _ in range(L - 1)] for _ in range(2)]
    yk, dy, loss = new(n, 1), new(n, 1), torch.zeros(1, device="cuda")
    g = [[torch.zeros_like(t) for t in ts] for ts in (sw, sb, mw, mb)]
    xg, tg = x.cuda(), y.cuda()
    ops.modsiren_forward_loss(xg, tg, sw, sb, mw, mb, W0, W0, saved, yk, dy, loss)
    ops.modsiren_backward(xg, dy, sw, mw, saved, dz[0], dz[1], g[0], g[1], g[2], g[3])
    y_inf = ops.modsiren_forward(xg, sw, sb, mw, mb, W0, W0)
    assert torch.equal(y_inf, yk), "inference and training kernels give different predictions"
    grads = [t for pair in zip(g[0], g[1]) for t in pair] + [t for pair in zip(g[2], g[3]) for t in pair]
    return yk.cpu(), loss.cpu()[0], [t.cpu() for t in grads]


# ------------------------------------------------------------------------------------------ 1. kernels vs float64
@pytest.mark.parametrize("d,H,L", SHAPES)
def test_kernels_against_float64(amd, d, H, L):
    assert amd.ops.modsiren_supported(d, H, L, 1)
    x_all, y_all, r64, r32 = selected_rows(d, H, L, 9000 + H + L)
    names = [f"siren {'w' if j == 0 else 'b'}{i}" for i in range(L + 1) for j in range(2)] + \
            [f"mod {'w' if j == 0 else 'b'}{i}" for i in range(L) for j in range(2)]
    for n in (x_all.shape[0], 1, 37, 257):
        x, y = x_all[:n], y_all[:n]
        p64, l64, g64 = r64.loss_and_grads(x, y)
        p32, l32, g32 = r32.loss_and_grads(x, y)
        pk, lk, gk = kernel_loss_and_grads(amd, r32, x, y)
        tag = f"({d}, {H}, {L}) n = {n}: "
        close_or_no_worse(pk.numpy(), p32.numpy(), p64.numpy(), tag + "y")
        close_or_no_worse(np.array([float(lk)]), np.array([float(l32)]), np.array([float(l64)]), tag + "loss")
        for name, a, b, c in zip(names, gk, g32, g64):
            assert a.shape == c.shape
            close_or_no_worse(a.numpy(), b.numpy(), c.numpy(), tag + name)


# ------------------------------------------------------------------------------------------ 2. the reference's fixtures
def load_net(amd, m, lr=1e-4):
    net = amd.models.ModulatedSirenNet(dim_in=m["dim_in"], dim_hidden=m["dim_hidden"], dim_out=1,
                                       n_layers=m["n_layers"], lr=lr)
    siren = omlp.siren_init(m["dim_in"], m["dim_hidden"], 1, m["n_layers"], m["seed"])
    mod = omlp.modulator_init(m["dim_in"], m["dim_hidden"], m["n_layers"], m["seed"] + 500)
    with torch.no_grad():
        for layer, (w, b) in zip(list(net.siren.layers) + [net.siren.last_layer], siren):
            layer.weight.copy_(w)
            layer.bias.copy_(b)
        for seq, (w, b) in zip(net.modulator.layers, mod):
            seq[0].weight.copy_(w)
            seq[0].bias.copy_(b)
    return net.cuda()


def fused_step(amd, net):
    step = amd.trainer.FusedStep(net, net.configure_optimizers(), modulated=True)
    assert step.use_modulated and not step.use_chain and not step.use_tiny and step.encoder is None
    return step


def step_grads(step):
    """(SIREN weight, bias) per layer and the head, then (modulator weight, bias) per layer: the flat buffer's views."""
    m = step.modulated
    return list(zip(m["d_sw"], m["d_sb"])), list(zip(m["d_mw"], m["d_mb"]))


@pytest.mark.parametrize("name", ["modsiren_2d", "modsiren_3d", "modsiren_3d_6x128"])
def test_fixtures_through_the_fused_step(amd, name):
    fx = load_golden(name)
    net = load_net(amd, fx.meta)
    assert sorted(net.state_dict().keys()) == fx.meta["state_dict_keys"]
    step = fused_step(amd, net)
    x, y = cuda(fx["x"]), cuda(fx["y"])
    pred = step.forward(x, train=False)[0]
    assert_close(pred.cpu().numpy(), fx["pred"], REL_TOL, "pred")
    loss = float(step.train_step(x, y, step=False))
    assert abs(loss - float(fx["loss"])) <= REL_TOL * abs(float(fx["loss"]))
    siren_g, mod_g = step_grads(step)
    for i, (gw, gb) in enumerate(siren_g):
        assert_close(gw.cpu().numpy(), fx[f"siren_gw_{i}"], REL_TOL, f"siren gw{i}")
        assert_close(gb.cpu().numpy(), fx[f"siren_gb_{i}"], REL_TOL, f"siren gb{i}")
    for i, (gw, gb) in enumerate(mod_g):
        assert_close(gw.cpu().numpy(), fx[f"mod_gw_{i}"], REL_TOL, f"mod gw{i}")
        assert_close(gb.cpu().numpy(), fx[f"mod_gb_{i}"], REL_TOL, f"mod gb{i}")


# ------------------------------------------------------------------------------------------ 3. three Adam steps
def test_e2e_modsiren_adam_golden(amd):
    fx = load_golden("e2e_modsiren_adam")
    m = fx.meta
    net = load_net(amd, m, lr=m["lr"])
    dead = {k: v.detach().clone() for k, v in net.state_dict().items()
            if k.startswith("layers.") or k.startswith("last_layer.")}
    assert len(dead) >= 4 and not any(k.startswith(("siren.", "modulator.")) for k in dead)
    step = fused_step(amd, net)
    r64 = ModRef(m["dim_in"], m["dim_hidden"], m["n_layers"], m["seed"], torch.float64)
    opt64 = omlp.Adam([p.detach() for p in r64.parameters()], lr=m["lr"])
    # (Adam steps the detached tensors, which share storage with the leaves autograd differentiates)
    siren_layers = list(net.siren.layers) + [net.siren.last_layer]
    mod_layers = [seq[0] for seq in net.modulator.layers]
    for s in range(m["steps"]):
        x, y = cuda(fx[f"x_{s}"]), cuda(fx[f"y_{s}"])
        loss = float(step.train_step(x, y))
        assert abs(loss - float(fx[f"loss_{s}"])) <= REL_TOL * abs(float(fx[f"loss_{s}"]))
        _, _, g64 = r64.loss_and_grads(x, y)
        opt64.step(g64)
        for kind, layers, params64 in (("siren", siren_layers, r64.siren), ("mod", mod_layers, r64.mod)):
            for i, layer in enumerate(layers):
                w64, b64 = params64[i]
                assert_no_worse(layer.weight.detach().cpu().numpy(), fx[f"{kind}_w_{s}_{i}"], w64.detach().numpy(),
                                f"{kind} w{i} step {s}", max_factor=AFTER_ADAM_MAX_FACTOR)
                assert_no_worse(layer.bias.detach().cpu().numpy(), fx[f"{kind}_b_{s}_{i}"], b64.detach().numpy(),
                                f"{kind} b{i} step {s}", max_factor=AFTER_ADAM_MAX_FACTOR)
    for k, v in net.state_dict().items():  # the dead default stack: no gradient, bit-unchanged through Adam
        if k in dead:
            assert torch.equal(v, dead[k]), k


# ------------------------------------------------------------------------------------------ 4. two evaluations agree
def _case(amd, d=3, H=128, L=4, n=3000, seed=9300):
    x, y, r64, r32 = selected_rows(d, H, L, seed, drawn=n)
    net = load_net(amd, dict(dim_in=d, dim_hidden=H, n_layers=L, seed=seed))
    return net, x.cuda(), y.cuda(), r64


def _flat_in_ref_order(step):
    siren_g, mod_g = step_grads(step)
    return [t.detach().cpu().clone() for pair in siren_g + mod_g for t in pair]


def test_autograd_path_and_fused_pass_agree(amd):
    net, x, y, r64 = _case(amd)
    step = fused_step(amd, net)
    loss_f = step.train_step(x, y, step=False).cpu().clone()
    g_fused = _flat_in_ref_order(step)
    flat_a = step.flat.grad.clone()
    loss_m = net.training_step((x, y), 0)
    params = [t for l in list(net.siren.layers) + [net.siren.last_layer] for t in (l.weight, l.bias)] + \
             [t for seq in net.modulator.layers for t in (seq[0].weight, seq[0].bias)]
    g_module = [g.cpu() for g in torch.autograd.grad(loss_m, params)]
    _, l64, g64 = r64.loss_and_grads(x, y)
    close_or_no_worse(np.array([float(loss_f)]), np.array([float(loss_m.detach())]), np.array([float(l64)]), "loss")
    for i, (a, b, c) in enumerate(zip(g_fused, g_module, g64)):
        close_or_no_worse(a.numpy(), b.numpy(), c.numpy(), f"gradient {i}")
    # forward(train=True) + backward() against train_step
    _, ws = step.forward(x, train=True)
    step.backward(x, y, ws)
    close_or_no_worse(np.array([float(step.loss)]), np.array([float(loss_f)]), np.array([float(l64)]),
                      "loss of forward + backward")
    for i, (a, b, c) in enumerate(zip(_flat_in_ref_order(step), g_fused, g64)):
        close_or_no_worse(a.numpy(), b.numpy(), c.numpy(), f"forward + backward gradient {i}")
    assert_close(step.flat.grad.cpu().numpy(), flat_a.cpu().numpy(), REL_TOL, "flat gradient")


# ------------------------------------------------------------------------------------------ 5. bitwise reproducibility
@pytest.mark.parametrize("n", [70001, 1 << 16])
def test_bitwise_reproducible(amd, n):
    net = load_net(amd, dict(dim_in=3, dim_hidden=128, n_layers=6, seed=41))
    step = fused_step(amd, net)
    x = torch.from_numpy(detrand.uniform(n * 3, 42, -1.0, 1.0).reshape(n, 3)).cuda()
    y = torch.from_numpy(detrand.uniform(n, 43, -1.0, 1.0).reshape(n, 1)).cuda()
    out = []
    for _ in range(2):
        loss = step.train_step(x, y, step=False)
        out.append((loss.clone(), step.flat.grad.clone()))
    assert torch.isfinite(out[0][1]).all() and float(out[0][1].abs().max()) > 0
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


# ------------------------------------------------------------------------------------------ 6. accumulation
def test_accumulation(amd):
    net, x, y, r64 = _case(amd, d=2, H=64, L=3, n=4000, seed=9400)
    n, half = x.shape[0], x.shape[0] // 2
    step = fused_step(amd, net)
    step.train_step(x, y, step=False)
    whole = _flat_in_ref_order(step)
    whole_flat = step.flat.grad.clone()
    # two unequal "halves" of n rows are two batches of their own: the mean of their two gradients
    step.train_step(x[:half], y[:half], first=True, step=False, divisor=2.0)
    step.train_step(x[half:2 * half], y[half:2 * half], first=False, step=False, divisor=2.0)
    halves = _flat_in_ref_order(step)
    _, _, g64 = r64.loss_and_grads(x[:2 * half], y[:2 * half])
    ref = ModRef(2, 64, 3, 9400, torch.float32)
    _, _, g32 = ref.loss_and_grads(x[:2 * half], y[:2 * half])
    for i, (a, b, c) in enumerate(zip(halves, g32, g64)):
        close_or_no_worse(a.numpy(), b.numpy(), c.numpy(), f"two halves, gradient {i}")
    # a non-first call adds to what the buffer holds
    step.train_step(x, y, first=True, step=False)
    step.train_step(x, y, first=False, step=False)
    assert_close(step.flat.grad.cpu().numpy(), 2.0 * whole_flat.cpu().numpy(), REL_TOL, "prefilled gradients")
    assert len(whole) == len(halves)


# ------------------------------------------------------------------------------------------ 7. inference
@pytest.mark.parametrize("n", [1, 37, 70001])
def test_inference(amd, n):
    net = load_net(amd, dict(dim_in=3, dim_hidden=64, n_layers=4, seed=51))
    step = fused_step(amd, net)
    x = torch.from_numpy(detrand.uniform(n * 3, 52, -1.0, 1.0).reshape(n, 3)).cuda()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    pred, ws = step.forward(x, train=False)
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - before
    with torch.no_grad():
        want = net(x.clone())
    assert_close(pred.cpu().numpy(), want.cpu().numpy(), REL_TOL, f"inference n = {n}")
    # no per-layer buffers: the prediction and the split weights, nothing of (n, hidden)
    assert "saved" not in ws and "dzs" not in ws and (n, True) not in step._ws
    split = amd.lib.load().mri_modsiren_forward_workspace_bytes(64, 4)
    assert grown <= n * 4 + split + (1 << 20), grown  # (the allocator rounds; one (n, 64) buffer at 70001 is 17 MiB)


# ------------------------------------------------------------------------------------------ 8. Trainer
def _phantom_run(amd, **trainer_kw):
    torch.manual_seed(0)
    vol = amd.datamodules.phantom_volume((64, 48, 5))[:, :, 2].contiguous().cpu().numpy()  # one slice of the phantom
    c = amd.config.BaseConfig().resolve(vol.shape)
    c.batch_size = 1024
    net = amd.models.ModulatedSirenNet(dim_in=2, dim_hidden=64, dim_out=1, n_layers=3, lr=1e-4)
    dm = amd.datamodules.MriDataModule(config=c, volume=vol)
    dm.prepare_data()
    tr = amd.trainer.Trainer(max_epochs=8, log_every=1, **trainer_kw)
    tr.fit(net, dm.train_dataloader())
    return tr, net, dm


def test_trainer_opt_in(amd):
    tr, net, dm = _phantom_run(amd, fused_modulated=True)
    assert tr.fused is not None and tr.fused.use_modulated
    assert len(tr.history) == tr.global_step == 24 and np.isfinite(tr.history).all()
    assert tr.history[-1] < tr.history[0]
    pred = torch.cat(tr.predict(net, dm.test_dataloader()))
    assert pred.shape == (64 * 48, 1) and bool(torch.isfinite(pred).all())
    tr, net, dm = _phantom_run(amd)  # the default keyword: training_step + autograd
    assert tr.fused is None and len(tr.history) == 24


def test_steady_loop_refuses_the_modulated_plan(amd):
    net = load_net(amd, dict(dim_in=2, dim_hidden=64, n_layers=3, seed=61))
    step = fused_step(amd, net)
    pipe = type("Pipe", (), dict(loader=None, group=1))()
    why = amd.trainer.SteadyLoop.unsupported(step, pipe)
    assert why and "ModulatedSirenNet" in why


# ------------------------------------------------------------------------------------------ 9. launcher
def test_launcher_fused_modulated(tmp_path):
    import launcher
    from mri_interpolation_amd import nifti
    fx = load_golden("sample_slice_z3_t7")
    raw = fx["raw_int16"].astype(np.float32) * np.float32(fx.meta["scl_slope"])
    path = str(tmp_path / "slice.nii.gz")
    nifti.save(raw, path)
    out = str(tmp_path / "run")
    launcher.main(["--model_class", "ModulatedSirenNet", "--fused_modulated", "--image_path", path,
                   "--batch_size", "4096", "--epochs", "2", "--dim_hidden", "64", "--n_layers", "3", "--out_dir", out,
                   "--log_every", "0"])
    txt = open(os.path.join(out, "config.txt")).read()
    assert "model_class : ModulatedSirenNet" in txt
    flag = [l for l in txt.splitlines() if l.startswith("fused_modulated")]
    assert flag and flag[0].split(":")[1].strip() == "True", txt
    psnr = float([l for l in txt.splitlines() if l.startswith("psnr_db")][0].split(":")[1])
    assert np.isfinite(psnr) and psnr > 5.0, psnr
