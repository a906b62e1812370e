"""The fused RffNet training step's host side: ABI symbols, shape support, workspace sizes, argument validation before
any device call, FusedStep's plan and its refusals, the Trainer / launcher flag.  CPU only (the kernels:
tests/test_gpu_rff_step.py)."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mri_inr.h")
SYMBOLS = ("mri_rff_train_supported", "mri_rff_backward_workspace_bytes", "mri_rff_forward_loss", "mri_rff_backward")
LIB_MAX = 8  # MRI_SIREN_MAX_LAYERS


@pytest.fixture(scope="module")
def lib():
    from mri_interpolation_amd import _lib
    from mri_interpolation_amd.build import build
    build()
    return _lib


def _header_arguments(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared in mri_inr.h"
    return [a for a in m.group(1).split(",") if a.strip()]


def test_symbols_are_declared_bound_and_exported(lib):
    handle = lib.load()
    bound = dict(lib.SIGNATURES)
    bound.update(lib.INT64_GETTERS)
    bound.update(lib.INT_GETTERS)
    for name in SYMBOLS:
        assert name in bound, f"{name} has no signature in _lib"
        assert len(_header_arguments(name)) == len(bound[name]), name
        assert hasattr(handle, name), f"{name} is not exported by the library"
    assert "mri_rff_train_supported" in lib.INT_GETTERS
    assert "mri_rff_backward_workspace_bytes" in lib.INT64_GETTERS
    assert len(lib.SIGNATURES["mri_rff_forward_loss"]) == 19 and len(lib.SIGNATURES["mri_rff_backward"]) == 16
    from mri_interpolation_amd import ops
    assert all(callable(getattr(ops, f)) for f in ("rff_train_supported", "rff_train_workspace", "rff_forward_loss",
                                                   "rff_backward"))
    # the header cites what it replaces, at every entry point
    text = open(HEADER).read()
    block = text[text.index("RffNet: fused training step"):text.index("mri_rff_train_supported(int32_t")]
    for name in SYMBOLS:
        at = block.index(name + " (")
        assert "models.py:542-584" in block[at:at + 120] and "models.py:61-66" in block[at:at + 120], name


def test_train_supported_is_forward_supported(lib):
    h = lib.load()
    seen = set()
    for d in range(0, 7):
        for hidden in (32, 48, 64, 96, 128, 256):
            for n_freq in (hidden, 64, 128, 1):
                for L in range(0, LIB_MAX + 2):
                    for dim_out in (1, 2):
                        args = (d, hidden, n_freq, L, dim_out)
                        got = h.mri_rff_train_supported(*args)
                        assert got == h.mri_rff_forward_supported(*args), args
                        seen.add(got)
    assert seen == {0, 1}
    assert h.mri_rff_train_supported(3, 128, 128, 6, 1) == 1 and h.mri_rff_train_supported(2, 64, 64, 2, 1) == 1
    assert h.mri_rff_train_supported(5, 64, 64, 3, 1) == 0 and h.mri_rff_train_supported(3, 128, 64, 3, 1) == 0
    from mri_interpolation_amd import ops
    assert ops.rff_train_supported(3, 128, 128, 6, 1) and not ops.rff_train_supported(3, 48, 48, 6, 1)


def test_workspace_bytes(lib):
    h = lib.load()
    size = h.mri_rff_backward_workspace_bytes
    for hidden, L in [(64, 2), (64, 3), (64, 8), (128, 2), (128, 6), (128, 8)]:
        ns = (1, 37, 129, 4096, 5000, 70001, 1 << 18, 1 << 20)
        sizes = [size(n, hidden, L) for n in ns]
        assert all(s > 0 and s % 16 == 0 for s in sizes), sizes
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
        assert sizes[-2] == sizes[-1], "nothing n-sized inside once n fills 256 workgroups"
        assert sizes[-1] == size((1 << 31) - 1, hidden, L)
        # the formula of the header
        for n, got in zip(ns, sizes):
            rows = 64 if hidden == 128 else 128
            G = min(-(-n // rows), 256)
            slab = hidden + 4 + (L - 1) * hidden
            Wg = min(-(-n // 32), 256) * (2 if hidden == 64 else 1)
            body = 4 * max(G * slab, 256, 2 * Wg * hidden * hidden)
            assert got == -(-body // 256) * 256 + (2 * L - 2) * 6 * hidden * hidden, (n, hidden, L)
        assert sizes[0] > h.mri_rff_forward_workspace_bytes(hidden, L)
        assert sizes[-1] <= 64 << 20
    for hidden in (32, 48, 96, 256):
        assert size(1000, hidden, 4) == -1
    assert size(1000, 64, 1) == -1 and size(1000, 64, LIB_MAX + 1) == -1
    assert size(0, 64, 4) == -1 and size(1 << 31, 64, 4) == -1
    from mri_interpolation_amd import ops
    with pytest.raises(ValueError, match="not supported"):
        ops.rff_train_workspace(100, 48, 4, "cpu")


def _arrays(count, value):
    return (C.c_void_p * count)(*([value] * count))


def test_validation_before_touching_the_device(lib):
    h = lib.load()
    fake = 4096
    fakep = C.c_void_p(fake)
    base = dict(n=8, n_total=8, d=2, H=64, F=64, L=3, divisor=1.0, ws_bytes=1 << 26)
    fwd_ptrs = ("x", "target", "b", "weight", "bias", "act", "y", "dy", "loss_out", "ws")
    bwd_ptrs = ("x", "dy", "b", "weight", "act", "dz", "d_weight", "d_bias", "ws")

    def pointers(names, kw):
        L = kw.get("L", base["L"])
        count = max(1, min(L, 16))
        out = {}
        for name in names:
            if name in ("weight", "bias", "act", "dz", "d_weight", "d_bias"):
                out[name] = _arrays(count, fake)
            else:
                out[name] = fakep
        out.update({k: v for k, v in kw.items() if k in names})
        return out

    def forward_loss(**kw):
        a = dict(base)
        a.update({k: v for k, v in kw.items() if k in base})
        p = pointers(fwd_ptrs, kw)
        return h.mri_rff_forward_loss(p["x"], p["target"], a["n"], a["n_total"], a["d"], a["H"], a["F"], a["L"], p["b"],
                                      p["weight"], p["bias"], a["divisor"], p["act"], p["y"], p["dy"], p["loss_out"],
                                      p["ws"], a["ws_bytes"], None)

    def backward(**kw):
        a = dict(base)
        a.update({k: v for k, v in kw.items() if k in base})
        p = pointers(bwd_ptrs, kw)
        return h.mri_rff_backward(p["x"], p["dy"], a["n"], a["d"], a["H"], a["F"], a["L"], p["b"], p["weight"], p["act"],
                                  p["dz"], p["d_weight"], p["d_bias"], p["ws"], a["ws_bytes"], None)

    def refused(rc, word):
        assert rc == -1
        msg = h.mri_last_error().decode()
        assert msg and word in msg, (word, msg)

    # n = 0: a no-op, whatever the buffers
    nulls_f = {k: None for k in fwd_ptrs}
    nulls_b = {k: None for k in bwd_ptrs}
    assert forward_loss(n=0, n_total=0, **nulls_f) == 0 and forward_loss(n=0, n_total=5, **nulls_f) == 0
    assert backward(n=0, **nulls_b) == 0
    # each unsupported shape argument, by name
    for call in (forward_loss, backward):
        refused(call(H=48, F=48), "hidden")
        refused(call(H=256, F=256), "hidden")
        refused(call(F=32), "n_freq")
        refused(call(H=128, F=64), "n_freq")
        refused(call(d=0), "dim_in")
        refused(call(d=5), "dim_in")
        refused(call(L=1), "n_layers")
        refused(call(L=LIB_MAX + 1), "n_layers")
        refused(call(n=-1), "n =")
        refused(call(n=1 << 31, n_total=1 << 31), "n =")
    # a slice larger than its batch, a divisor that is no divisor
    refused(forward_loss(n=8, n_total=7), "n_total")
    refused(forward_loss(divisor=0.0), "grad_divisor")
    refused(forward_loss(divisor=-1.0), "grad_divisor")
    # every NULL, by name
    for name in fwd_ptrs:
        refused(forward_loss(**{name: None}), "workspace" if name == "ws" else name + " is NULL")
    for name in bwd_ptrs:
        refused(backward(**{name: None}), "workspace" if name == "ws" else name + " is NULL")
    # NULL pointers inside the arrays
    L = base["L"]
    for name in ("weight", "bias", "act"):
        refused(forward_loss(**{name: _arrays(L, None)}), name + "[0] is NULL")
    for name in ("weight", "act", "dz", "d_weight", "d_bias"):
        refused(backward(**{name: _arrays(L, None)}), name + "[0] is NULL")
    second = (C.c_void_p * L)(fake, None, fake)
    refused(forward_loss(act=second), "act[1] is NULL")
    refused(backward(dz=second), "dz[1] is NULL")
    # misaligned saved tensors (the weight-gradient kernels stream them in 16-byte pieces), workspace
    refused(forward_loss(act=_arrays(L, fake + 4)), "act[0] must be 16-byte aligned")
    refused(backward(act=_arrays(L, fake + 8)), "act[0] must be 16-byte aligned")
    refused(backward(dz=(C.c_void_p * L)(fake, fake + 4, fake)), "dz[1] must be 16-byte aligned")
    refused(forward_loss(ws=C.c_void_p(fake + 4)), "workspace must be 16-byte aligned")
    refused(backward(ws=C.c_void_p(fake + 8)), "workspace must be 16-byte aligned")
    refused(forward_loss(x=C.c_void_p(fake + 2)), "4-byte aligned")
    # a workspace one byte short
    need = h.mri_rff_backward_workspace_bytes(base["n"], base["H"], base["L"])
    refused(forward_loss(ws_bytes=need - 1), "workspace")
    refused(backward(ws_bytes=need - 1), "workspace")
    refused(backward(ws_bytes=0), "workspace")


def test_ops_reject_cpu_tensors(lib):
    from mri_interpolation_amd import ops
    H, d, n = 64, 2, 5
    b = torch.zeros(H, d)
    ws = [torch.zeros(H, 2 * H), torch.zeros(H, H), torch.zeros(1, H)]
    bs = [torch.zeros(H), torch.zeros(H), torch.zeros(1)]
    act = [torch.zeros(n, H), torch.zeros(n, H)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rff_forward_loss(torch.zeros(n, d), torch.zeros(n, 1), b, ws, bs, act, torch.zeros(n, 1), torch.zeros(n, 1),
                             torch.zeros(1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rff_backward(torch.zeros(n, d), torch.zeros(n, 1), b, ws, act, [torch.zeros(n, H), torch.zeros(n, H)],
                         [torch.zeros_like(w) for w in ws], [torch.zeros_like(v) for v in bs])


# ------------------------------------------------------------------------------------------ the plan
def _net(**kw):
    from mri_interpolation_amd import models
    args = dict(dim_in=3, dim_hidden=64, dim_out=1, n_layers=4, n_frequencies=64)
    args.update(kw)
    return models.RffNet(**args)


def test_without_the_keyword_nothing_changes(lib):
    from mri_interpolation_amd import trainer
    net = _net()
    assert trainer.fusable_layers(net) is None
    assert trainer.fusable_layers(net, batch_norm=True, modulated=True) is None
    with pytest.raises(ValueError, match="not a fusable chain"):
        trainer.FusedStep(net, net.configure_optimizers())


@pytest.mark.parametrize("d,H,L", [(3, 64, 4), (2, 128, 2), (3, 128, 6), (4, 64, 8), (1, 64, 3)])
def test_plan_lists_the_linears_in_order(lib, d, H, L):
    from mri_interpolation_amd import ops, trainer
    net = _net(dim_in=d, dim_hidden=H, n_layers=L, n_frequencies=H)
    plan = trainer.fusable_layers(net, rff=True)
    assert isinstance(plan, trainer.RffPlan)
    encoder, layers = plan
    assert encoder is None and len(layers) == L
    assert [tuple(l.weight.shape) for l in layers] == [(H, 2 * H)] + [(H, H)] * (L - 2) + [(1, H)]
    for i, l in enumerate(layers):
        assert l.weight is net.decoder[2 * i].weight and l.bias is net.decoder[2 * i].bias
        assert l.activation == ops.ACT_RELU
    # the frozen projection rides beside the layers, not among them, and the optimiser never sees it
    assert plan.b is net.encoder.b and tuple(plan.b.shape) == (H, d)
    planned = {id(l.weight) for l in layers} | {id(l.bias) for l in layers}
    assert id(net.encoder.b) not in planned
    opt = net.configure_optimizers()
    assert len(opt._params) == 2 * L and all(p is not net.encoder.b for p in opt._params)


def test_refusals_name_their_reason(lib):
    from mri_interpolation_amd import models, trainer
    plan = lambda net: trainer.fusable_layers(net, rff=True)  # noqa: E731
    with pytest.raises(ValueError, match="n_frequencies = 32 != dim_hidden = 64"):
        plan(_net(n_frequencies=32))
    with pytest.raises(ValueError, match="dim_hidden = 48"):
        plan(_net(dim_hidden=48, n_frequencies=48))
    with pytest.raises(ValueError, match="dim_hidden = 256"):
        plan(_net(dim_hidden=256, n_frequencies=256))
    with pytest.raises(ValueError, match="dim_in = 5"):
        plan(_net(dim_in=5))
    with pytest.raises(ValueError, match="dim_out = 2"):
        plan(_net(dim_out=2))
    with pytest.raises(ValueError, match="1 Linears"):
        plan(_net(n_layers=1))
    with pytest.raises(ValueError, match="9 Linears"):
        plan(_net(n_layers=9))
    net = _net()
    net.decoder[2].bias = None
    with pytest.raises(ValueError, match="without a bias"):
        plan(net)
    with pytest.raises(ValueError, match="activation other than the fused ReLU"):
        plan(_net(activation=torch.nn.GELU))
    with pytest.raises(ValueError, match="activation other than the fused ReLU"):
        plan(_net(activation=torch.nn.Tanh))
    # the keyword changes nothing for the other models
    siren = models.SirenNet(dim_in=2, dim_hidden=64, n_layers=3)
    a, b = trainer.fusable_layers(siren), trainer.fusable_layers(siren, rff=True)
    assert a[0] is None and b[0] is None and len(a[1]) == len(b[1]) == 4
    assert all(p.weight is q.weight for p, q in zip(a[1], b[1]))
    assert not isinstance(b, trainer.RffPlan)
    assert trainer.fusable_layers(models.ModulatedSirenNet(dim_in=2, dim_hidden=64, n_layers=3), rff=True) is None


def test_steady_loop_names_the_plan(lib):
    from mri_interpolation_amd import trainer
    step = type("Step", (), dict(psf=None, bn=False, use_modulated=False, use_rff=True))()
    pipe = type("Pipe", (), dict(loader=None, group=1))()
    why = trainer.SteadyLoop.unsupported(step, pipe)
    assert why and "RffNet" in why and "eagerly" in why


def test_trainer_and_launcher_flag(lib):
    import launcher
    from mri_interpolation_amd import trainer
    from mri_interpolation_amd.trainer import Trainer
    assert Trainer(distributed=False).fused_rff is False
    assert Trainer(distributed=False, fused_rff=True).fused_rff is True
    assert Trainer(distributed=False, fused_rff=True).fused_modulated is False
    assert launcher.parse_args([]).fused_rff is False
    args = launcher.parse_args(["--model_class", "RffNet", "--fused_rff", "--dim_hidden", "64", "--n_frequencies", "64"])
    assert args.fused_rff is True and args.model_class == "RffNet"
    # the keyword reaches the plan: FusedStep(rff=True) gets as far as the flat buffers, which need the GPU
    net = _net()
    with pytest.raises(RuntimeError, match="GPU"):
        trainer.FusedStep(net, net.configure_optimizers(), rff=True)
    bad = _net(n_frequencies=32)
    with pytest.raises(ValueError, match="n_frequencies"):
        trainer.FusedStep(bad, bad.configure_optimizers(), rff=True)
