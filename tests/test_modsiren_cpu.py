"""The fused modulated SIREN step's host side: ABI symbols, shape support, workspace sizes, argument validation before
any device call, FusedStep's plan and its refusals, the Trainer / launcher flag.  CPU only (the kernels:
tests/test_gpu_modsiren.py)."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mri_inr.h")
SYMBOLS = ("mri_modsiren_supported", "mri_modsiren_forward_workspace_bytes", "mri_modsiren_backward_workspace_bytes",
           "mri_modsiren_forward", "mri_modsiren_forward_loss", "mri_modsiren_backward")


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
    assert "mri_modsiren_supported" in lib.INT_GETTERS
    assert "mri_modsiren_forward_workspace_bytes" in lib.INT64_GETTERS
    assert "mri_modsiren_backward_workspace_bytes" in lib.INT64_GETTERS
    from mri_interpolation_amd import ops
    assert all(callable(getattr(ops, f)) for f in ("modsiren_supported", "modsiren_forward", "modsiren_forward_loss",
                                                   "modsiren_backward"))
    # the header cites what it replaces
    text = open(HEADER).read()
    block = text[text.index("fused modulated SIREN chain"):text.index("mri_modsiren_supported(int32_t")]
    assert "models.py:263-322" in block and "models.py:236-260" in block


def test_supported_shapes(lib):
    h = lib.load()
    for d in range(1, 9):
        for hidden in (64, 128):
            for L in range(2, 9):
                assert h.mri_modsiren_supported(d, hidden, L, 1) == 1, (d, hidden, L)
    assert h.mri_modsiren_supported(3, 128, 6, 2) == 0   # dim_out 2
    assert h.mri_modsiren_supported(9, 128, 6, 1) == 0   # dim_in 9
    assert h.mri_modsiren_supported(3, 48, 6, 1) == 0    # no kernel of that width
    assert h.mri_modsiren_supported(0, 64, 3, 1) == 0
    assert h.mri_modsiren_supported(3, 64, 9, 1) == 0    # beyond MRI_SIREN_MAX_LAYERS
    from mri_interpolation_amd import ops
    assert ops.modsiren_supported(3, 128, 6, 1) and not ops.modsiren_supported(3, 48, 6, 1)


def test_workspace_bytes(lib):
    h = lib.load()
    for hidden, L in [(64, 2), (64, 8), (128, 4), (128, 6)]:
        fwd = h.mri_modsiren_forward_workspace_bytes(hidden, L)
        # both stacks' H x H blocks in three bf16 terms: 2 (L - 1) H H 6 bytes
        assert fwd == 2 * (L - 1) * hidden * hidden * 6
        sizes = [h.mri_modsiren_backward_workspace_bytes(n, hidden, L) for n in (1, 37, 4096, 70001, 1 << 18, 1 << 22)]
        assert sizes[0] > fwd
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
        assert sizes[-1] <= 64 << 20
    assert h.mri_modsiren_forward_workspace_bytes(48, 4) == -1
    assert h.mri_modsiren_backward_workspace_bytes(1000, 48, 4) == -1
    assert h.mri_modsiren_backward_workspace_bytes(0, 64, 4) == -1
    assert h.mri_modsiren_backward_workspace_bytes(1000, 64, 1) == -1


def _arrays(count, value):
    return (C.c_void_p * count)(*([value] * count))


def test_validation_before_touching_the_device(lib):
    h = lib.load()
    fake, L, H, d = 4096, 3, 64, 2
    fakep = C.c_void_p(fake)

    def forward(n=8, d=d, H=H, L=L, p=fakep, arr=fake, ws=fakep, ws_bytes=1 << 24, saved=None):
        a = lambda k: _arrays(k, arr)  # noqa: E731
        return h.mri_modsiren_forward(p, n, d, H, L, a(L + 1), a(L + 1), a(L), a(L), 30.0, 30.0, saved, saved, saved,
                                      saved, p, ws, ws_bytes, None)

    def forward_loss(n=8, n_total=8, divisor=1.0, p=fakep, ws=fakep, ws_bytes=1 << 24, H=H):
        a = lambda k: _arrays(k, fake)  # noqa: E731
        return h.mri_modsiren_forward_loss(p, p, n, n_total, d, H, L, a(L + 1), a(L + 1), a(L), a(L), 30.0, 30.0,
                                           divisor, a(L), a(L), a(L), a(L), p, p, p, ws, ws_bytes, None)

    def backward(n=8, p=fakep, arr=fake, ws=fakep, ws_bytes=1 << 24, L=L):
        a = lambda k: _arrays(k, arr)  # noqa: E731
        return h.mri_modsiren_backward(p, p, n, d, H, L, a(L + 1), a(L), a(L), a(L), a(L), a(L), a(L), a(L), a(L + 1),
                                       a(L + 1), a(L), a(L), ws, ws_bytes, None)

    def refused(rc, word):
        assert rc == -1
        msg = h.mri_last_error().decode()
        assert msg and word in msg, msg

    # n = 0: a no-op, whatever the buffers
    assert forward(n=0, p=None) == 0 and forward_loss(n=0, n_total=0, p=None) == 0 and backward(n=0, p=None) == 0
    # unsupported shapes come with their reason
    refused(forward(H=48), "not supported")
    refused(forward(d=9), "not supported")
    refused(forward(L=1), "not supported")
    refused(forward_loss(H=96), "not supported")
    refused(backward(L=9), "not supported")
    # NULL data, NULL parameter pointers inside the arrays
    refused(forward(p=None), "NULL")
    refused(forward(arr=None), "NULL")
    refused(forward_loss(p=None), "NULL")
    refused(backward(p=None), "NULL")
    refused(backward(arr=None), "NULL")
    # a training call without its four buffer arrays' contents
    refused(forward(saved=_arrays(L, None)), "NULL")
    # workspace: missing, short, misaligned
    need_f = h.mri_modsiren_forward_workspace_bytes(H, L)
    need_b = h.mri_modsiren_backward_workspace_bytes(8, H, L)
    refused(forward(ws=None), "workspace")
    refused(forward(ws_bytes=need_f - 1), "workspace")
    refused(forward(ws=C.c_void_p(4100)), "workspace")
    refused(forward_loss(ws_bytes=need_b - 1), "workspace")
    refused(backward(ws_bytes=need_b - 1), "workspace")
    refused(backward(ws=None), "workspace")
    # n out of range, a slice larger than its batch, a divisor that is no divisor
    refused(forward(n=-1), "n")
    refused(forward_loss(n=8, n_total=7), "n_total")
    refused(forward_loss(divisor=0.0), "divisor")
    # misaligned saved tensors (the weight-gradient kernels stream them in 16-byte pieces)
    refused(backward(arr=4100), "aligned")


def test_ops_reject_cpu_tensors(lib):
    from mri_interpolation_amd import ops
    sw = [torch.zeros(64, 2), torch.zeros(64, 64), torch.zeros(1, 64)]
    sb = [torch.zeros(64), torch.zeros(64), torch.zeros(1)]
    mw, mb = [torch.zeros(64, 2), torch.zeros(64, 66)], [torch.zeros(64), torch.zeros(64)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.modsiren_forward(torch.zeros(5, 2), sw, sb, mw, mb, 30.0, 30.0)


# ------------------------------------------------------------------------------------------ the plan
def _net(**kw):
    from mri_interpolation_amd import models
    args = dict(dim_in=3, dim_hidden=64, dim_out=1, n_layers=4)
    args.update(kw)
    return models.ModulatedSirenNet(**args)


def test_without_the_keyword_nothing_changes(lib):
    from mri_interpolation_amd import trainer
    net = _net()
    assert trainer.fusable_layers(net) is None
    with pytest.raises(ValueError, match="not a fusable chain"):
        trainer.FusedStep(net, net.configure_optimizers())


@pytest.mark.parametrize("d,H,L", [(3, 64, 4), (2, 128, 2), (3, 128, 6), (8, 64, 8)])
def test_plan_lists_both_stacks_in_order(lib, d, H, L):
    from mri_interpolation_amd import ops, trainer
    net = _net(dim_in=d, dim_hidden=H, n_layers=L, w0=20.0, w0_initial=25.0)
    plan = trainer.fusable_layers(net, modulated=True)
    assert isinstance(plan, trainer.ModulatedPlan)
    encoder, layers = plan
    assert encoder is None and layers == plan.modulator + plan.siren
    assert [tuple(l.weight.shape) for l in plan.modulator] == [(H, d)] + [(H, H + d)] * (L - 1)
    assert [tuple(l.weight.shape) for l in plan.siren] == [(H, d)] + [(H, H)] * (L - 1) + [(1, H)]
    for i, l in enumerate(plan.modulator):
        assert l.weight is net.modulator.layers[i][0].weight and l.bias is net.modulator.layers[i][0].bias
        assert l.activation == ops.ACT_RELU
    for i, l in enumerate(plan.siren[:-1]):
        assert l.weight is net.siren.layers[i].weight and l.bias is net.siren.layers[i].bias
        assert l.activation == ops.ACT_SINE and l.w0 == (25.0 if i == 0 else 20.0)
    assert plan.siren[-1].weight is net.siren.last_layer.weight and plan.siren[-1].activation == ops.ACT_IDENTITY
    # the dead default stack is no part of the plan
    planned = {id(l.weight) for l in layers}
    assert all(id(l.weight) not in planned for l in list(net.layers) + [net.last_layer])


def test_refusals_name_their_reason(lib):
    from mri_interpolation_amd import models, trainer
    plan = lambda net: trainer.fusable_layers(net, modulated=True)  # noqa: E731
    with pytest.raises(ValueError, match="final_activation"):
        plan(_net(final_activation=torch.nn.Sigmoid()))
    with pytest.raises(ValueError, match="use_bias"):
        plan(_net(use_bias=False))
    net = _net()
    net.siren.layers[2].activation = torch.nn.Tanh()
    net.siren.layers[2]._code = models._activation_code(net.siren.layers[2].activation)
    with pytest.raises(ValueError, match="non-Sine activation"):
        plan(net)
    with pytest.raises(ValueError, match="unsupported width or depth"):
        plan(_net(dim_hidden=48))
    with pytest.raises(ValueError, match="unsupported width or depth"):
        plan(_net(n_layers=1))
    with pytest.raises(ValueError, match="unsupported width or depth"):
        plan(_net(n_layers=9))
    with pytest.raises(ValueError, match="unsupported width or depth"):
        plan(_net(dim_in=9))
    with pytest.raises(ValueError, match="unsupported width or depth"):
        plan(_net(dim_out=2))
    net = _net()
    net.siren.layers[2].activation = models.Sine(10.0)
    net.siren.layers[2]._code = models._activation_code(net.siren.layers[2].activation)
    with pytest.raises(ValueError, match="different w0"):
        plan(net)
    # FusedStep hands the reason on
    bad = _net(dim_hidden=48)
    with pytest.raises(ValueError, match="unsupported width or depth"):
        trainer.FusedStep(bad, bad.configure_optimizers(), modulated=True)
    # the keyword changes nothing for the other models
    siren = models.SirenNet(dim_in=2, dim_hidden=64, n_layers=3)
    a, b = trainer.fusable_layers(siren), trainer.fusable_layers(siren, modulated=True)
    assert a[0] is None and b[0] is None and len(a[1]) == len(b[1]) == 4
    assert all(p.weight is q.weight for p, q in zip(a[1], b[1]))
    assert not isinstance(b, trainer.ModulatedPlan)


def test_trainer_and_launcher_flag(lib):
    import launcher
    from mri_interpolation_amd.trainer import Trainer
    assert Trainer(distributed=False).fused_modulated is False
    assert Trainer(distributed=False, fused_modulated=True).fused_modulated is True
    assert launcher.parse_args([]).fused_modulated is False
    args = launcher.parse_args(["--model_class", "ModulatedSirenNet", "--fused_modulated"])
    assert args.fused_modulated is True and args.model_class == "ModulatedSirenNet"
