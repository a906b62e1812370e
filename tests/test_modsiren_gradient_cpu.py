"""The modulated SIREN coordinate gradient without a device: the C ABI of csrc/modsiren_gradient.hip (symbols, supported
shapes, workspace, argument validation before any HIP call), and the layers above the kernel as far as they can be seen
without a GPU -- `ModulatedSirenNet.forward_with_gradient(fused=...)` on CPU tensors and which keyword
`Trainer.predict_with_gradient` passes.  CPU only."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

INVALID = -1  # MRI_ERR_INVALID_ARGUMENT
LIB_MAX = 8   # MRI_SIREN_MAX_LAYERS
NAMES = ("mri_modsiren_gradient_supported", "mri_modsiren_gradient_workspace_bytes", "mri_modsiren_gradient")


@pytest.fixture(scope="module")
def lib():
    from mri_interpolation_amd import _lib
    from mri_interpolation_amd.build import build
    build()
    return _lib


# ------------------------------------------------------------------------------------------------ ABI
def test_symbols_are_declared_bound_and_exported(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mri_inr.h")).read(), flags=re.S)
    h = lib.load()
    bound = {**lib.SIGNATURES, **lib.INT64_GETTERS, **lib.INT_GETTERS}
    for name in NAMES:
        decl = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert decl, f"{name} is not declared in include/mri_inr.h"
        assert name in bound, f"{name} has no binding in _lib.py"
        assert hasattr(h, name), f"{name} is not exported by the library"
        assert len(bound[name]) == len(decl.group(1).split(",")), f"{name}: the binding's argument count"
    assert "mri_modsiren_gradient" in lib.SIGNATURES and len(lib.SIGNATURES["mri_modsiren_gradient"]) == 16
    assert "mri_modsiren_gradient_workspace_bytes" in lib.INT64_GETTERS
    assert "mri_modsiren_gradient_supported" in lib.INT_GETTERS


def test_supported_shapes_and_workspace(lib):
    h = lib.load()
    assert lib.MAX_SIREN_LAYERS == LIB_MAX
    for hidden in (64, 128):
        for L in range(2, LIB_MAX + 1):
            for dim_in in (1, 2, 3):
                assert h.mri_modsiren_gradient_supported(dim_in, hidden, L, 1) == 1, (dim_in, hidden, L)
                assert h.mri_modsiren_supported(dim_in, hidden, L, 1) == 1
            assert h.mri_modsiren_gradient_workspace_bytes(hidden, L) == 2 * (L - 1) * 6 * hidden * hidden
            assert h.mri_modsiren_gradient_workspace_bytes(hidden, L) == h.mri_modsiren_forward_workspace_bytes(hidden, L)
    for dim_in in (0, 4, 8):
        assert h.mri_modsiren_gradient_supported(dim_in, 128, 6, 1) == 0, dim_in
    for hidden in (32, 256):
        assert h.mri_modsiren_gradient_supported(3, hidden, 6, 1) == 0, hidden
        assert h.mri_modsiren_gradient_workspace_bytes(hidden, 6) == -1
    for L in (1, LIB_MAX + 1):
        assert h.mri_modsiren_gradient_supported(3, 128, L, 1) == 0, L
        assert h.mri_modsiren_gradient_workspace_bytes(128, L) == -1
    assert h.mri_modsiren_gradient_supported(3, 128, 6, 2) == 0


def _call(h, x=64, sw=None, sb=None, mw=None, mb=None, y=64, dydx=64, ws=256, ws_bytes=1 << 30, n=8, dim_in=3, hidden=64,
          L=3):
    """mri_modsiren_gradient with fake (never dereferenced) device addresses; the four parameter arrays default to real
    HOST arrays of fake device pointers, 0 stands for a NULL array.  Every call here is refused before anything is
    launched or read."""
    arr = (C.c_void_p * (LIB_MAX + 1))(*[256] * (LIB_MAX + 1))
    arrays = [arr if a is None else (None if isinstance(a, int) else a) for a in (sw, sb, mw, mb)]
    p = lambda v: None if v is None else C.c_void_p(v)  # noqa: E731
    return h.mri_modsiren_gradient(p(x), n, dim_in, hidden, L, *arrays, 30.0, 30.0, p(y), p(dydx), p(ws), ws_bytes, None)


def test_argument_validation_without_a_device(lib):
    h = lib.load()
    err = lambda: h.mri_last_error().decode()  # noqa: E731
    # an empty batch is a no-op and touches no device
    assert h.mri_modsiren_gradient(None, 0, 3, 64, 3, None, None, None, None, 30.0, 30.0, None, None, None, 0, None) == 0
    # every NULL buffer, the way tests/test_abi.py calls the other entry points
    args = (None, 8, 3, 128, 6, None, None, None, None, 30.0, 30.0, None, None, None, 0, None)
    assert len(args) == len(lib.SIGNATURES["mri_modsiren_gradient"])
    assert h.mri_modsiren_gradient(*args) == INVALID and err()
    for name, kw in (("x", dict(x=None)), ("siren_weight", dict(sw=0)), ("siren_bias", dict(sb=0)),
                     ("mod_weight", dict(mw=0)), ("mod_bias", dict(mb=0)), ("y", dict(y=None)),
                     ("dydx", dict(dydx=None)), ("workspace", dict(ws=None))):
        assert _call(h, **kw) == INVALID, name
        assert name in err(), (name, err())
    null_layer = (C.c_void_p * (LIB_MAX + 1))(*([256] * 2 + [None] + [256] * (LIB_MAX - 2)))
    for kw in (dict(sw=null_layer), dict(sb=null_layer)):
        assert _call(h, **kw) == INVALID and "SIREN" in err() and "layer 2" in err(), err()
    for kw in (dict(mw=null_layer), dict(mb=null_layer)):
        assert _call(h, **kw) == INVALID and "modulator" in err() and "layer 2" in err(), err()
    # weights and workspace: 16-byte aligned; a short workspace
    odd = (C.c_void_p * (LIB_MAX + 1))(*([256] + [256 + 4] + [256] * (LIB_MAX - 1)))
    assert _call(h, sw=odd) == INVALID and "siren_weight[1]" in err() and "16-byte" in err(), err()
    assert _call(h, mw=odd) == INVALID and "mod_weight[1]" in err() and "16-byte" in err(), err()
    assert _call(h, ws=256 + 4) == INVALID and "workspace" in err() and "16-byte" in err(), err()
    assert _call(h, ws_bytes=h.mri_modsiren_gradient_workspace_bytes(64, 3) - 1) == INVALID and "workspace" in err()
    assert _call(h, ws_bytes=h.mri_modsiren_gradient_workspace_bytes(64, 3), x=None) == INVALID and "x" in err()
    # x, y, dydx: any 4-byte aligned address, nothing coarser
    for name in ("x", "y", "dydx"):
        assert _call(h, **{name: 64 + 2}) == INVALID and name in err() and "4-byte" in err(), (name, err())
    # the ranges name the argument
    for hidden in (32, 96, 256):
        assert _call(h, hidden=hidden) == INVALID and "hidden" in err(), err()
    for dim_in in (0, 4, 8):
        assert _call(h, dim_in=dim_in) == INVALID and "dim_in" in err(), err()
    for L in (1, LIB_MAX + 1):
        assert _call(h, L=L) == INVALID and "n_layers" in err(), err()
    assert _call(h, n=-1) == INVALID and "out of range" in err(), err()
    assert _call(h, n=1 << 31) == INVALID and "out of range" in err(), err()


def _parameters(dim_in=3, hidden=64, L=3):
    sw = [torch.zeros(hidden, dim_in)] + [torch.zeros(hidden, hidden) for _ in range(L - 1)] + [torch.zeros(1, hidden)]
    sb = [torch.zeros(hidden) for _ in range(L)] + [torch.zeros(1)]
    mw = [torch.zeros(hidden, dim_in)] + [torch.zeros(hidden, hidden + dim_in) for _ in range(L - 1)]
    mb = [torch.zeros(hidden) for _ in range(L)]
    return sw, sb, mw, mb


def test_ops_reject_cpu_tensors(lib):
    from mri_interpolation_amd import ops
    assert ops.modsiren_gradient_supported(3, 64, 3, 1) and not ops.modsiren_gradient_supported(4, 64, 3, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.modsiren_gradient(torch.zeros(4, 3), *_parameters(), 30.0, 30.0)


# ------------------------------------------------------------------------------------------------ model, trainer
def _torch_ops(monkeypatch):
    """The two layer ops of ModulatedSirenNet.forward restated in plain PyTorch, so that the generic body runs on CPU
    tensors (the library's ops refuse them)."""
    from mri_interpolation_amd import ops

    def linear_act(x, w, b, act=ops.ACT_IDENTITY, w0=1.0):
        z = F.linear(x, w, b)
        return {ops.ACT_IDENTITY: lambda: z, ops.ACT_RELU: lambda: torch.relu(z),
                ops.ACT_SINE: lambda: torch.sin(w0 * z)}[act]()

    monkeypatch.setattr(ops, "linear_act", linear_act)
    monkeypatch.setattr(ops, "modulate", lambda a, b: a * b)


def test_on_the_cpu_both_forms_are_the_generic_body(lib, monkeypatch):
    from mri_interpolation_amd import models, ops
    _torch_ops(monkeypatch)

    def refuse(*a, **k):
        raise AssertionError("the kernel cannot serve a CPU tensor")
    monkeypatch.setattr(ops, "modsiren_gradient", refuse)
    torch.manual_seed(4)
    net = models.ModulatedSirenNet(3, 64, 1, 3)
    x = torch.rand(37, 3) * 2 - 1
    assert net._gradient_plan(x) is None
    want_y, want_g = models.BaseMLP.forward_with_gradient(net, x)
    xg = x.clone().requires_grad_(True)
    ay = net(xg)
    ag, = torch.autograd.grad(ay.sum(), xg)
    assert torch.equal(want_y, ay.detach()) and torch.equal(want_g, ag)
    for kw in ({}, dict(fused=False), dict(fused=True)):
        y, g = net.forward_with_gradient(x, **kw)
        assert y.shape == (37, 1) and g.shape == (37, 3) and g.abs().max() > 0
        assert torch.equal(y, want_y) and torch.equal(g, want_g), kw
        assert not y.requires_grad and not g.requires_grad and y.grad_fn is None and g.grad_fn is None
        assert all(p.grad is None for p in net.parameters())
    with pytest.raises(ValueError, match="dim_out"):
        models.ModulatedSirenNet(3, 64, 2, 3).forward_with_gradient(x, fused=True)
    with pytest.raises(ValueError, match="dim_out"):
        models.ModulatedSirenNet(3, 64, 2, 3).forward_with_gradient(x)


def test_trainer_passes_fused_only_for_a_modulated_net_under_fused_modulated(monkeypatch):
    """Trainer.predict_with_gradient, seen through spies on the two classes' methods (the models stay where they are:
    a parameter that claims to be on the GPU keeps the trainer from moving them)."""
    from mri_interpolation_amd import models, trainer
    seen = []

    def spy(name):
        def forward_with_gradient(self, x, **kw):
            seen.append((name, dict(kw)))
            return torch.zeros(x.shape[0], 1), torch.zeros(x.shape[0], x.shape[1])
        return forward_with_gradient

    monkeypatch.setattr(models.ModulatedSirenNet, "forward_with_gradient", spy("modulated"))
    monkeypatch.setattr(models.SirenNet, "forward_with_gradient", spy("plain"))
    monkeypatch.setattr(torch.nn.Module, "cuda", lambda self, *a, **k: self)
    loader = [(torch.zeros(5, 3), None), (torch.zeros(2, 3), None)]
    modulated, plain = models.ModulatedSirenNet(3, 64, 1, 3), models.SirenNet(3, 64, 1, 3)
    for fused_modulated in (True, False):
        tr = trainer.Trainer(max_epochs=1, log_every=0, distributed=False, fused_modulated=fused_modulated)
        for net in (modulated, plain):
            ys, gs = tr.predict_with_gradient(net, loader)
            assert [tuple(y.shape) for y in ys] == [(5, 1), (2, 1)] and [tuple(g.shape) for g in gs] == [(5, 3), (2, 3)]
    assert seen == [("modulated", dict(fused=True))] * 2 + [("plain", {})] * 2 + [("modulated", {})] * 2 + [("plain", {})] * 2
    assert trainer.Trainer(max_epochs=1, distributed=False).fused_modulated is False
