"""The BatchNorm kernels (csrc/batchnorm.hip) and FusedStep's BatchNorm plan on the MI355X.

1. the three kernels against float64 (torch.nn.functional.batch_norm + activation + autograd on the CPU, same
   float32 inputs), well and ill conditioned, the eval form, bitwise reproducibility, accumulation and aliasing;
2. the reference's fixture `hashmlp_bn_adam` through FusedStep(batch_norm=True).train_step;
3. the fused step against training_step + autograd at size, both judged against float64;
4. state: module forward in eval(), checkpoint round trip;  5. gradient accumulation;
6. Trainer(fused_batchnorm=True) and the launcher flag;  7. no autograd graph, no allocation per step.
"""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import REL_TOL, assert_close, load_golden, rel_err
from yardstick import AFTER_ADAM_MAX_FACTOR, assert_no_worse
from oracle import detrand
from oracle import hashgrid as ohash
from oracle import mlp as omlp

pytestmark = pytest.mark.gpu

ACTS = {"identity": 0, "relu": 1, "gelu": 3}
ACT_FN = {"identity": lambda u: u, "relu": F.relu, "gelu": F.gelu}
OUTPUTS = ("y", "running_mean", "running_var", "dz", "dgamma", "dbeta")


@pytest.fixture(scope="module")
def amd():
    from mri_interpolation_amd import _lib, checkpoint, config, datamodules, models, ops, trainer
    assert torch.cuda.is_available(), "these tests need the GPU"
    _lib.load()
    return type("NS", (), dict(lib=_lib, ops=ops, models=models, trainer=trainer, datamodules=datamodules,
                               checkpoint=checkpoint, config=config))


# --------------------------------------------------------------------------- 1. kernels against float64
@functools.lru_cache(maxsize=2)
def _case(n, C, mean, spread, seed=0):
    """z of the given mean and standard deviation (uniform), dy, gamma, beta and initial running buffers."""
    half = spread * 3.0 ** 0.5
    z = torch.from_numpy(detrand.uniform(n * C, seed + 1, mean - half, mean + half).reshape(n, C))
    dy = torch.from_numpy(detrand.uniform(n * C, seed + 2, -1.0, 1.0).reshape(n, C))
    gamma = torch.from_numpy(detrand.uniform(C, seed + 3, 0.5, 1.5))
    beta = torch.from_numpy(detrand.uniform(C, seed + 4, -0.2, 0.2))
    rm = torch.from_numpy(detrand.uniform(C, seed + 5, -0.1, 0.1))
    rv = torch.from_numpy(detrand.uniform(C, seed + 6, 0.5, 1.5))
    return z, dy, gamma, beta, rm, rv


def _reference(case, act, dtype):
    """F.batch_norm (training) + activation + autograd on the CPU in `dtype`."""
    z, dy, gamma, beta, rm, rv = (t.to(dtype).clone() for t in case)
    z.requires_grad_(True), gamma.requires_grad_(True), beta.requires_grad_(True)
    y = ACT_FN[act](F.batch_norm(z, rm, rv, gamma, beta, True, 0.1, 1e-5))
    y.backward(dy)
    return dict(y=y.detach(), running_mean=rm, running_var=rv, dz=z.grad, dgamma=gamma.grad, dbeta=beta.grad)


def _kernels(ops, case, act, alias=False, tracked=None):
    """bn_stats -> bn_act_forward -> bn_act_backward on the GPU; returns the same dict, on the CPU."""
    z, dy, gamma, beta, rm, rv = (t.cuda() for t in case)  # (.cuda() copies: the case's tensors stay as they are)
    if tracked is None:
        tracked = torch.zeros((), dtype=torch.int64, device="cuda")
    save = ops.bn_stats(z, rm, rv, tracked, 0.1, 1e-5)
    y = ops.bn_act_forward(z, gamma, beta, ACTS[act], save=save)
    dg, db = torch.empty_like(gamma), torch.empty_like(beta)
    dz = ops.bn_act_backward(dy, z, save, gamma, beta, dg, db, ACTS[act], dz=None if alias else torch.empty_like(dy),
                             overwrite=True)
    assert (dz.data_ptr() == dy.data_ptr()) == alias
    torch.cuda.synchronize()
    out = dict(y=y, running_mean=rm, running_var=rv, dz=dz, dgamma=dg, dbeta=db, save=save)
    return {k: v.cpu() for k, v in out.items()}, int(tracked)


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("n,C", [(320, 64), (10000, 64), (1 << 18, 64), (1 << 18, 1), ((1 << 18) + 3, 128),
                                 (4099, 256)])
def test_kernels_against_float64(amd, n, C, act):
    """1a + 1e: every output within REL_TOL of float64; a second run gives the same bits."""
    case = _case(n, C, 0.3, 1.0)
    want = _reference(case, act, torch.float64)
    got, tracked = _kernels(amd.ops, case, act)
    assert tracked == 1
    for k in OUTPUTS:
        e = rel_err(got[k].numpy(), want[k].numpy())
        print(f"({n}, {C}) {act} {k}: {e[0]:.2e} / {e[1]:.2e}")
        assert_close(got[k].numpy(), want[k].numpy(), REL_TOL, f"({n}, {C}) {act} {k}")
    again, _ = _kernels(amd.ops, case, act)
    for k in OUTPUTS + ("save",):
        assert torch.equal(got[k], again[k]), f"({n}, {C}) {act} {k}: two runs differ"


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("n", [2, 3])
def test_kernels_on_two_and_three_rows(amd, n, act):
    """1b: eps dominates var here, so PyTorch's own f32 result is the yardstick's reference."""
    case = _case(n, 64, 0.3, 1.0)
    f32, f64 = _reference(case, act, torch.float32), _reference(case, act, torch.float64)
    got, _ = _kernels(amd.ops, case, act)
    for k in OUTPUTS:
        assert_no_worse(got[k].numpy(), f32[k].numpy(), f64[k].numpy(), f"n = {n} {act} {k}")


@pytest.mark.parametrize("act", list(ACTS))
def test_kernels_on_an_ill_conditioned_batch(amd, act):
    """1c: mean 100, spread 0.01.  The f32 inputs no longer resolve z - mean, so y and the gradients are held
    to PyTorch's f32 result; the running variance is held to REL_TOL of float64, which a plain f32
    E[z^2] - E[z]^2 misses."""
    case = _case(10000, 64, 100.0, 0.01)
    f32, f64 = _reference(case, act, torch.float32), _reference(case, act, torch.float64)
    got, _ = _kernels(amd.ops, case, act)
    for k in ("y", "dz", "dgamma", "dbeta"):
        assert_no_worse(got[k].numpy(), f32[k].numpy(), f64[k].numpy(), f"ill-conditioned {act} {k}")
    e = rel_err(got["running_var"].numpy(), f64["running_var"].numpy())
    print(f"ill-conditioned running_var: {e[0]:.2e} / {e[1]:.2e}")
    assert_close(got["running_var"].numpy(), f64["running_var"].numpy(), REL_TOL, "ill-conditioned running_var")
    assert_close(got["running_mean"].numpy(), f64["running_mean"].numpy(), REL_TOL, "ill-conditioned running_mean")
    # the batch variance itself (not diluted by the running buffer's history): invstd of the save area
    z64 = case[0].double()
    invstd64 = 1.0 / torch.sqrt(z64.var(0, unbiased=False) + 1e-5)
    assert_close(got["save"][1].numpy(), invstd64.numpy(), REL_TOL, "ill-conditioned invstd")


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("n,C", [(10000, 64), (4099, 1), (1 << 18, 128)])
def test_eval_form(amd, n, C, act):
    """1d: the eval form against its formula in float64; the three buffers stay bit-identical."""
    z, _, gamma, beta, rm, rv = _case(n, C, 0.3, 1.0)
    u = gamma.double() * (z.double() - rm.double()) / torch.sqrt(rv.double() + 1e-5) + beta.double()
    want = ACT_FN[act](u)
    rm_d, rv_d = rm.cuda(), rv.cuda()
    got = amd.ops.bn_act_forward(z.cuda(), gamma.cuda(), beta.cuda(), ACTS[act], running_mean=rm_d,
                                 running_var=rv_d, eps=1e-5)
    assert_close(got.cpu().numpy(), want.numpy(), REL_TOL, f"eval ({n}, {C}) {act}")
    assert torch.equal(rm_d.cpu(), rm) and torch.equal(rv_d.cpu(), rv)
    zd = z.cuda()
    in_place = amd.ops.bn_act_forward(zd, gamma.cuda(), beta.cuda(), ACTS[act], running_mean=rm_d, running_var=rv_d,
                                      eps=1e-5, out=zd)
    assert in_place.data_ptr() == zd.data_ptr() and torch.equal(in_place, got)


@pytest.mark.parametrize("n,C", [(10000, 64), (1 << 18, 1), (4099, 256)])
def test_accumulation_and_aliasing(amd, n, C):
    """1f: overwrite=False adds to dgamma / dbeta; dz in place of dy gives the same bits as a separate dz."""
    ops = amd.ops
    case = _case(n, C, 0.3, 1.0)
    apart, _ = _kernels(ops, case, "gelu")
    aliased, _ = _kernels(ops, case, "gelu", alias=True)
    for k in ("dz", "dgamma", "dbeta"):
        assert torch.equal(apart[k], aliased[k]), k
    z, dy, gamma, beta = (t.cuda() for t in case[:4])
    save = ops.bn_stats(z)
    before_g = torch.from_numpy(detrand.uniform(C, 50, -1.0, 1.0))
    before_b = torch.from_numpy(detrand.uniform(C, 51, -1.0, 1.0))
    dg, db = before_g.cuda(), before_b.cuda()
    ops.bn_act_backward(dy.clone(), z, save, gamma, beta, dg, db, ACTS["gelu"], overwrite=False)
    assert torch.equal(dg.cpu(), before_g + apart["dgamma"]) and torch.equal(db.cpu(), before_b + apart["dbeta"])
    # a strided view (leading dimension above C) gives what the packed matrix gives
    wide = torch.zeros(n, C + 4, device="cuda")
    wide[:, :C] = z
    assert torch.equal(ops.bn_stats(wide[:, :C]), save)


def test_one_row_is_refused(amd):
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        amd.ops.bn_stats(torch.zeros(1, 64, device="cuda"))


# --------------------------------------------------------------------------- 2. the reference's fixture
def test_reference_fixture_through_the_fused_step(amd):
    """`hashmlp_bn_adam` (made from the reference, tests/golden/make_golden.py), set up as
    test_gpu_round3.py::test_hashmlp_batchnorm_decoder_gradients_and_adam does, driven by
    FusedStep(batch_norm=True).train_step."""
    fx = load_golden("hashmlp_bn_adam")
    m, c = fx.meta, fx.meta["ctor"]
    net = amd.models.HashMLP(dim_in=3, n_levels=c["n_levels"], n_features_per_level=c["n_features_per_level"],
                             log2_hashmap_size=c["log2_hashmap_size"], base_resolution=tuple(c["base_resolution"]),
                             finest_resolution=tuple(c["finest_resolution"]), dim_hidden=64, dim_out=1, n_layers=2,
                             lr=m["lr"])
    with torch.no_grad():
        net.encoder.table.copy_(torch.cat(ohash.init_tables(m["sizes"], 1, m["table_seed"], m["table_scale"])))
        for blk, (w, b) in zip(net.decoder, omlp.linear_init(m["dims"], m["mlp_seed"])):
            blk[0].weight.copy_(w)
            blk[0].bias.copy_(b)
            blk[1].weight.copy_(torch.from_numpy(detrand.uniform(blk[1].weight.numel(), m["bn_seeds"][0], 0.5, 1.5)))
            blk[1].bias.copy_(torch.from_numpy(detrand.uniform(blk[1].bias.numel(), m["bn_seeds"][1], -0.2, 0.2)))
    net.cuda().train()
    opt = net.configure_optimizers()
    fused = amd.trainer.FusedStep(net, opt, batch_norm=True)
    assert fused.bn and not fused.use_tiny and not fused.use_chain
    gv = fused.flat.grad_view
    b_first = [blk[0].bias.detach().cpu().numpy().copy() for blk in net.decoder]
    for step in range(m["steps"]):
        x = torch.as_tensor(fx[f"x_{step}"]).cuda()
        y = torch.as_tensor(fx[f"y_{step}"]).cuda()
        b_before = [blk[0].bias.detach().cpu().numpy().copy() for blk in net.decoder]
        loss = fused.train_step(x, y)
        assert loss.grad_fn is None
        assert abs(float(loss) - float(fx[f"loss_{step}"])) <= REL_TOL * float(fx[f"loss_{step}"])
        if step == 0:  # (Adam does not touch the flat gradient buffer: it still holds this step's gradients)
            g = gv(net.encoder.table).cpu().numpy()
            for l in range(net.encoder.n_levels):
                lo, hi = net.encoder._row_span(l)
                want = np.zeros((hi - lo, 1), dtype=np.float32)
                want[fx[f"grad_idx_{l}"]] = fx[f"grad_val_{l}"]
                assert set(np.nonzero(g[lo:hi, 0])[0]) <= set(fx[f"grad_idx_{l}"].tolist()), f"level {l}: stray slot"
                assert_close(g[lo:hi], want, REL_TOL, f"table gradient level {l}")
            for i, blk in enumerate(net.decoder):
                assert_close(gv(blk[0].weight).cpu().numpy(), fx[f"gw_{i}"], REL_TOL, f"gw{i}")
                assert_close(gv(blk[1].weight).cpu().numpy(), fx[f"bn_gw_{i}"], REL_TOL, f"bn gw{i}")
                assert_close(gv(blk[1].bias).cpu().numpy(), fx[f"bn_gb_{i}"], REL_TOL, f"bn gb{i}")
                # zero in exact arithmetic, the column sum of dz here (not special-cased)
                assert float(gv(blk[0].bias).abs().max()) <= 1e-5 * float(gv(blk[0].weight).abs().max())
        for i, blk in enumerate(net.decoder):
            assert_close(blk[0].weight.detach().cpu().numpy(), fx[f"w_{step}_{i}"], REL_TOL, f"w{i} step {step}")
            assert_close(blk[1].weight.detach().cpu().numpy(), fx[f"bn_w_{step}_{i}"], REL_TOL, f"bn w{i} step {step}")
            assert_close(blk[1].bias.detach().cpu().numpy(), fx[f"bn_b_{step}_{i}"], REL_TOL, f"bn b{i} step {step}")
            b_ref = fx[f"b_{step - 1}_{i}"] if step else b_first[i]
            own = blk[1].running_mean.cpu().numpy() - 0.1 * b_before[i]
            ref = fx[f"bn_mean_{step}_{i}"] - 0.1 * b_ref
            assert np.abs(own - ref).max() <= REL_TOL * np.abs(fx[f"bn_mean_{step}_{i}"]).max(), (i, step)
            assert_close(blk[1].running_var.cpu().numpy(), fx[f"bn_var_{step}_{i}"], REL_TOL, f"bn var{i} step {step}")
        table = net.encoder.table.detach().cpu().numpy()
        for l in range(net.encoder.n_levels):
            lo, hi = net.encoder._row_span(l)
            assert_close(table[lo:hi][fx[f"grad_idx_{l}"]], fx[f"table_{step}_{l}"], REL_TOL, f"table {l} step {step}")
    for blk in net.decoder:
        assert int(blk[1].num_batches_tracked) == m["steps"] == 2
    # eval form from the reference's final state (the rows x_0 touches are in the fixture)
    last = m["steps"] - 1
    with torch.no_grad():
        for l in range(net.encoder.n_levels):
            lo, hi = net.encoder._row_span(l)
            net.encoder.table.data[lo:hi][torch.as_tensor(fx[f"grad_idx_{l}"].astype(np.int64)).cuda()] = \
                torch.as_tensor(fx[f"table_{last}_{l}"]).cuda()
        for i, blk in enumerate(net.decoder):
            blk[0].weight.copy_(torch.as_tensor(fx[f"w_{last}_{i}"]))
            blk[0].bias.copy_(torch.as_tensor(fx[f"b_{last}_{i}"]))
            blk[1].weight.copy_(torch.as_tensor(fx[f"bn_w_{last}_{i}"]))
            blk[1].bias.copy_(torch.as_tensor(fx[f"bn_b_{last}_{i}"]))
            blk[1].running_mean.copy_(torch.as_tensor(fx[f"bn_mean_{last}_{i}"]))
            blk[1].running_var.copy_(torch.as_tensor(fx[f"bn_var_{last}_{i}"]))
        pred, _ = fused.forward(torch.as_tensor(fx["x_0"]).cuda(), train=False)
    assert_close(pred.cpu().numpy(), fx["pred_eval_after"], REL_TOL, "eval-mode prediction")


# --------------------------------------------------------------------------- 3. fused against the module path
HASH_CONFIG = dict(n_levels=4, n_features_per_level=1, log2_hashmap_size=23, base_resolution=(64, 64, 5),
                   finest_resolution=(352, 352, 15), dim_hidden=64, n_layers=2)  # reference config/base.py
THREE_BLOCKS = dict(n_levels=4, n_features_per_level=2, log2_hashmap_size=19, base_resolution=(64, 64, 5),
                    finest_resolution=(352, 352, 15), dim_hidden=128, n_layers=3)


def _build(amd, cfg, seed=7, table_scale=0.5):
    net = amd.models.HashMLP(dim_in=3, dim_out=1, lr=5e-3, **cfg)
    f = cfg["n_features_per_level"]
    with torch.no_grad():
        net.encoder.table.copy_(torch.cat(ohash.init_tables(net.encoder.sizes, f, seed, table_scale)))
        dims = [cfg["n_levels"] * f] + [cfg["dim_hidden"]] * (cfg["n_layers"] - 1) + [1]
        for i, (blk, (w, b)) in enumerate(zip(net.decoder, omlp.linear_init(dims, seed + 1))):
            blk[0].weight.copy_(w)
            blk[0].bias.copy_(b)
            blk[1].weight.copy_(torch.from_numpy(detrand.uniform(blk[1].weight.numel(), seed + 10 + i, 0.5, 1.5)))
            blk[1].bias.copy_(torch.from_numpy(detrand.uniform(blk[1].bias.numel(), seed + 20 + i, -0.2, 0.2)))
    return net.cuda().train()


def _batches(n, steps, seed=100):
    return [(torch.from_numpy(detrand.uniform(n * 3, seed + s, 0.0, 1.0).reshape(n, 3)),
             torch.from_numpy(detrand.uniform(n, seed + 50 + s, 0.0, 1.0).reshape(n, 1))) for s in range(steps)]


def _snapshot(net):
    s = dict(table=net.encoder.table.detach().cpu().clone())
    for i, blk in enumerate(net.decoder):
        s[f"w{i}"], s[f"b{i}"] = blk[0].weight.detach().cpu().clone(), blk[0].bias.detach().cpu().clone()
        s[f"bn_w{i}"], s[f"bn_b{i}"] = blk[1].weight.detach().cpu().clone(), blk[1].bias.detach().cpu().clone()
        s[f"rm{i}"], s[f"rv{i}"] = blk[1].running_mean.cpu().clone(), blk[1].running_var.cpu().clone()
    return s


def _float64_steps(net, batches, lr):
    """The same steps in float64 on the CPU from `net`'s current state: oracle encoder, F.linear,
    F.batch_norm (training), GELU, MSE, the oracle's Adam.  Returns (losses, state, biases used per step)."""
    enc = net.encoder
    res, _ = ohash.resolutions_for(3, enc.n_levels, net.log2_hashmap_size, net.base_resolution,
                                   net.finest_resolution)
    table = enc.table.detach().double().cpu()
    tables = [table[slice(*enc._row_span(l))].clone() for l in range(enc.n_levels)]
    lin = [(blk[0].weight.detach().double().cpu(), blk[0].bias.detach().double().cpu()) for blk in net.decoder]
    bn = [dict(weight=blk[1].weight.detach().double().cpu(), bias=blk[1].bias.detach().double().cpu(),
               running_mean=blk[1].running_mean.double().cpu(), running_var=blk[1].running_var.double().cpu())
          for blk in net.decoder]
    params = tables + [t for w, b in lin for t in (w, b)] + [t for s in bn for t in (s["weight"], s["bias"])]
    opt = omlp.Adam(params, lr=lr)
    losses, biases = [], []
    for x, y in batches:
        biases.append([b.clone() for _, b in lin])
        for p in params:
            p.requires_grad_(True)
            p.grad = None
        pred = omlp.hashmlp_decoder_forward(ohash.encode(x.double(), tables, res), lin, bn, True)
        loss = omlp.mse_loss(pred, y.double())
        loss.backward()
        grads = [p.grad for p in params]
        for p in params:
            p.requires_grad_(False)
        opt.step(grads)
        losses.append(float(loss))
    state = dict(table=torch.cat(tables))
    for i, ((w, b), s) in enumerate(zip(lin, bn)):
        state.update({f"w{i}": w, f"b{i}": b, f"bn_w{i}": s["weight"], f"bn_b{i}": s["bias"],
                      f"rm{i}": s["running_mean"], f"rv{i}": s["running_var"]})
    return losses, state, biases


def _bias_history(biases, layer):
    """sum_k 0.1 * 0.9^(t - k) * b_k: what the Linear biases used in steps 1..t put into the running mean."""
    t = len(biases)
    return sum(0.1 * 0.9 ** (t - 1 - k) * biases[k][layer].double().cpu() for k in range(t))


@pytest.mark.parametrize("cfg,n", [(HASH_CONFIG, 10000), (THREE_BLOCKS, 1 << 18)], ids=["hashconfig", "three_blocks"])
def test_fused_against_module_path_at_size(amd, cfg, n):
    batches = _batches(n, 3)
    fused_net, module_net = _build(amd, cfg), _build(amd, cfg)
    l64, s64, b64 = _float64_steps(fused_net, batches, 5e-3)
    fused = amd.trainer.FusedStep(fused_net, fused_net.configure_optimizers(), batch_norm=True)
    opt = module_net.configure_optimizers()
    l_fused, l_module, b_fused, b_module = [], [], [], []
    for k, (x, y) in enumerate(batches):
        x, y = x.cuda(), y.cuda()
        b_fused.append([blk[0].bias.detach().clone() for blk in fused_net.decoder])
        b_module.append([blk[0].bias.detach().clone() for blk in module_net.decoder])
        l_fused.append(float(fused.train_step(x, y)))
        opt.zero_grad()
        loss = module_net.training_step((x, y), k)
        loss.backward()
        opt.step()
        l_module.append(float(loss))
    s_fused, s_module = _snapshot(fused_net), _snapshot(module_net)
    assert_no_worse(np.array(l_fused), np.array(l_module), np.array(l64), "losses")
    n_blocks = len(fused_net.decoder)
    for i in range(n_blocks):
        assert int(fused_net.decoder[i][1].num_batches_tracked) == 3
        for k in (f"w{i}", f"bn_w{i}", f"bn_b{i}"):
            assert_no_worse(s_fused[k].numpy(), s_module[k].numpy(), s64[k].numpy(), f"{k} after 3 steps",
                            max_factor=AFTER_ADAM_MAX_FACTOR)
        assert_no_worse(s_fused[f"rv{i}"].numpy(), s_module[f"rv{i}"].numpy(), s64[f"rv{i}"].numpy(),
                        f"running_var {i}", max_factor=AFTER_ADAM_MAX_FACTOR)
        # the Linear biases random-walk on rounding noise (tests/test_oracle_golden.py:333-355): each side's
        # running mean is compared with its own biases' contribution taken out
        own = [s[f"rm{i}"].double() - _bias_history(b, i) for s, b in
               ((s_fused, b_fused), (s_module, b_module), (s64, b64))]
        assert_no_worse(own[0].numpy(), own[1].numpy(), own[2].numpy(), f"running_mean {i}",
                        max_factor=AFTER_ADAM_MAX_FACTOR)
    assert_no_worse(s_fused["table"].numpy(), s_module["table"].numpy(), s64["table"].numpy(), "table after 3 steps",
                    max_factor=AFTER_ADAM_MAX_FACTOR)


# --------------------------------------------------------------------------- 4. state
SMALL = dict(n_levels=4, n_features_per_level=2, log2_hashmap_size=14, base_resolution=(8, 8, 4),
             finest_resolution=(32, 32, 16), dim_hidden=32, n_layers=2)


def test_state_is_the_modules_state(amd, tmp_path):
    net = _build(amd, SMALL)
    opt = net.configure_optimizers()
    fused = amd.trainer.FusedStep(net, opt, batch_norm=True)
    for x, y in _batches(4096, 5):
        fused.train_step(x.cuda(), y.cuda())
    x = _batches(3000, 1, seed=900)[0][0].cuda()
    with torch.no_grad():
        want = fused.forward(x, train=False)[0].clone()
        net.eval()
        module = net(x)
        net.train()
    assert_close(module.cpu().numpy(), want.cpu().numpy(), REL_TOL, "module forward in eval() against the fused eval form")
    sd = net.state_dict()
    for i in range(2):
        assert int(sd[f"decoder.{i}.1.num_batches_tracked"]) == 5
        assert not torch.equal(sd[f"decoder.{i}.1.running_mean"].cpu(), torch.zeros_like(sd[f"decoder.{i}.1.running_mean"]).cpu())
    path = str(tmp_path / "bn.ckpt")
    amd.checkpoint.save(path, net, opt, epoch=0, global_step=5)
    fresh = amd.models.HashMLP(dim_in=3, dim_out=1, lr=5e-3, **SMALL).cuda()
    amd.checkpoint.load(path, fresh)
    again = amd.trainer.FusedStep(fresh, fresh.configure_optimizers(), batch_norm=True)
    with torch.no_grad():
        got = again.forward(x, train=False)[0]
    assert torch.equal(got, want)


# --------------------------------------------------------------------------- 5. accumulation
def test_gradient_accumulation_matches_the_module_path(amd):
    fused_net, module_net = _build(amd, SMALL), _build(amd, SMALL)
    fused = amd.trainer.FusedStep(fused_net, fused_net.configure_optimizers(), batch_norm=True)
    opt = module_net.configure_optimizers()
    (xa, ya), (xb, yb) = [(x.cuda(), y.cuda()) for x, y in _batches(2048, 2)]
    fused.train_step(xa, ya, first=True, step=False, divisor=2.0)
    fused.train_step(xb, yb, first=False, step=True, divisor=2.0)
    opt.zero_grad()
    for k, (x, y) in enumerate(((xa, ya), (xb, yb))):
        (module_net.training_step((x, y), k) / 2.0).backward()
    grads_module = {k: p.grad.detach().cpu().clone() for k, p in module_net.named_parameters()}
    opt.step()
    for (k, p), (_, q) in zip(fused_net.named_parameters(), module_net.named_parameters()):
        if k.endswith(".0.bias"):  # Linear bias in front of BatchNorm: rounding noise on both sides
            continue
        assert_close(fused.flat.grad_view(p).cpu().numpy(), grads_module[k].numpy(), REL_TOL, f"accumulated grad {k}")
    for i in range(2):
        assert int(fused_net.decoder[i][1].num_batches_tracked) == 2
        assert_close(fused_net.decoder[i][1].running_var.cpu().numpy(),
                     module_net.decoder[i][1].running_var.cpu().numpy(), REL_TOL, f"running_var {i}")
        assert_close(fused_net.decoder[i][0].weight.detach().cpu().numpy(),
                     module_net.decoder[i][0].weight.detach().cpu().numpy(), REL_TOL, f"w{i} after the step")


# --------------------------------------------------------------------------- 6. Trainer and launcher
def _reference_decoder_run(amd, **trainer_kw):
    torch.manual_seed(0)
    vol = amd.datamodules.phantom_volume((32, 32, 16)).cpu().numpy()
    c = amd.config.HashConfig().resolve(vol.shape)
    c.batch_size = 4096
    net = amd.models.HashMLP(dim_in=3, n_levels=4, n_features_per_level=2, log2_hashmap_size=14,
                             base_resolution=(8, 8, 4), finest_resolution=(32, 32, 16), dim_hidden=32, dim_out=1,
                             n_layers=2, lr=5e-3)
    dm = amd.datamodules.MriDataModule(config=c, volume=vol)
    dm.prepare_data()
    tr = amd.trainer.Trainer(max_epochs=6, log_every=1, **trainer_kw)
    tr.fit(net, dm.train_dataloader())
    return tr, net, dm


def test_trainer_opt_in_boundary(amd):
    tr, net, dm = _reference_decoder_run(amd, fused_batchnorm=True)
    assert tr.fused is not None and tr.fused.bn
    assert len(tr.history) == tr.global_step == 24 and tr.history[-1] < tr.history[0]
    pred = torch.cat(tr.predict(net, dm.test_dataloader()))
    assert pred.shape == (32 * 32 * 16, 1) and bool(torch.isfinite(pred).all())
    assert int(net.decoder[0][1].num_batches_tracked) == 24
    tr, net, dm = _reference_decoder_run(amd)  # the default keyword: today's autograd path
    assert tr.fused is None and len(tr.history) == tr.global_step == 24


def test_launcher_flag(tmp_path):
    import launcher
    from mri_interpolation_amd import nifti
    out = str(tmp_path / "run")
    launcher.main(["--synthetic", "32,32,16", "--fused_batchnorm", "--max_steps", "20", "--out_dir", out,
                   "--log_every", "0"])
    assert nifti.load(os.path.join(out, "pred.nii.gz")).shape == (32, 32, 16)
    txt = open(os.path.join(out, "config.txt")).read()
    assert "model_class : HashMLP" in txt and "psnr_db" in txt


# --------------------------------------------------------------------------- 7. no graph, no allocation
def test_no_autograd_graph_and_no_allocation_per_step(amd):
    net = _build(amd, SMALL)
    fused = amd.trainer.FusedStep(net, net.configure_optimizers(), batch_norm=True)
    x, y = [t.cuda() for t in _batches(4096, 1)[0]]
    for _ in range(3):
        loss = fused.train_step(x, y)
    assert loss.grad_fn is None and not loss.requires_grad
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for _ in range(10):
        fused.train_step(x, y)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
