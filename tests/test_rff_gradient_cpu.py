"""The RffNet coordinate gradient without a device: the C ABI of rff_gradient_kernel's entry points in csrc/rff.hip
(symbols, supported shapes, workspace, argument validation before any HIP call), and the layers above the kernel as far
as they can be seen without a GPU -- `RffNet.forward_with_gradient(fused=...)` on CPU tensors and which keyword
`Trainer.predict_with_gradient` passes.  CPU only."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

INVALID = -1  # MRI_ERR_INVALID_ARGUMENT
LIB_MAX = 8   # MRI_SIREN_MAX_LAYERS
NAMES = ("mri_rff_gradient_supported", "mri_rff_gradient_workspace_bytes", "mri_rff_gradient")


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
    assert "mri_rff_gradient" in lib.SIGNATURES and len(lib.SIGNATURES["mri_rff_gradient"]) == 14
    assert "mri_rff_gradient_workspace_bytes" in lib.INT64_GETTERS
    assert "mri_rff_gradient_supported" in lib.INT_GETTERS


def test_supported_is_the_forward_kernels_and_the_workspace_its_split_weights(lib):
    h = lib.load()
    assert lib.MAX_SIREN_LAYERS == LIB_MAX
    accepted = 0
    for hidden in (32, 64, 128, 256):
        for L in range(1, 10):
            shape_ok = hidden in (64, 128) and 2 <= L <= LIB_MAX
            want = L * 6 * hidden * hidden if shape_ok else -1
            assert h.mri_rff_gradient_workspace_bytes(hidden, L) == want, (hidden, L)
            assert h.mri_rff_gradient_workspace_bytes(hidden, L) == h.mri_rff_forward_workspace_bytes(hidden, L)
            for dim_in in range(0, 6):
                for n_freq in (hidden, hidden // 2):
                    for dim_out in (1, 2):
                        got = h.mri_rff_gradient_supported(dim_in, hidden, n_freq, L, dim_out)
                        assert got == h.mri_rff_forward_supported(dim_in, hidden, n_freq, L, dim_out), \
                            (dim_in, hidden, n_freq, L, dim_out)
                        assert got == int(shape_ok and 1 <= dim_in <= 4 and n_freq == hidden and dim_out == 1)
                        accepted += got
    assert accepted == 2 * 7 * 4


def _call(h, x=64, b=64, w=None, bias=None, y=64, dydx=64, ws=256, ws_bytes=1 << 30, n=8, dim_in=3, hidden=64,
          n_freq=None, L=3):
    """mri_rff_gradient with fake (never dereferenced) device addresses; weight / bias default to real HOST arrays of
    fake device pointers, 0 stands for a NULL array.  Every call here is refused before anything is launched or
    read."""
    arr = (C.c_void_p * LIB_MAX)(*[256] * LIB_MAX)
    w, bias = [arr if a is None else (None if isinstance(a, int) else a) for a in (w, bias)]
    p = lambda v: None if v is None else C.c_void_p(v)  # noqa: E731
    return h.mri_rff_gradient(p(x), n, dim_in, hidden, hidden if n_freq is None else n_freq, L, p(b), w, bias, p(y),
                              p(dydx), p(ws), ws_bytes, None)


def test_argument_validation_without_a_device(lib):
    h = lib.load()
    err = lambda: h.mri_last_error().decode()  # noqa: E731
    # an empty batch is a no-op and touches no device
    assert h.mri_rff_gradient(None, 0, 3, 64, 64, 3, None, None, None, None, None, None, 0, None) == 0
    # every NULL buffer, the way tests/test_abi.py calls the other entry points
    args = (None, 8, 3, 128, 128, 6, None, None, None, None, None, None, 0, None)
    assert len(args) == len(lib.SIGNATURES["mri_rff_gradient"])
    assert h.mri_rff_gradient(*args) == INVALID and err()
    for name, kw in (("x", dict(x=None)), ("b", dict(b=None)), ("weight", dict(w=0)), ("bias", dict(bias=0)),
                     ("y", dict(y=None)), ("dydx", dict(dydx=None)), ("workspace", dict(ws=None))):
        assert _call(h, **kw) == INVALID, name
        assert name in err(), (name, err())
    null_layer = (C.c_void_p * LIB_MAX)(*([256] * 2 + [None] + [256] * (LIB_MAX - 3)))
    assert _call(h, w=null_layer) == INVALID and "weight[2]" in err(), err()
    assert _call(h, bias=null_layer) == INVALID and "bias[2]" in err(), err()
    # the workspace: 16-byte aligned, and not one byte short
    need = h.mri_rff_gradient_workspace_bytes(64, 3)
    assert _call(h, ws=256 + 4) == INVALID and "workspace" in err() and "16-byte" in err(), err()
    assert _call(h, ws_bytes=need - 1) == INVALID and "workspace" in err() and str(need) in err(), err()
    assert _call(h, ws_bytes=need, x=None) == INVALID and "x" in err()  # (the exact size passes that check)
    # x, b, y, dydx: any 4-byte aligned address, nothing coarser
    for name in ("x", "b", "y", "dydx"):
        assert _call(h, **{name: 64 + 2}) == INVALID and name in err() and "4-byte" in err(), (name, err())
    odd = (C.c_void_p * LIB_MAX)(*([256] + [256 + 2] + [256] * (LIB_MAX - 2)))
    assert _call(h, w=odd) == INVALID and "weight[1]" in err() and "4-byte" in err(), err()
    # the ranges name the argument
    for hidden in (32, 96, 256):
        assert _call(h, hidden=hidden) == INVALID and "hidden" in err(), err()
    assert _call(h, hidden=128, n_freq=64) == INVALID and "n_freq" in err(), err()
    for dim_in in (0, 5, 8):
        assert _call(h, dim_in=dim_in) == INVALID and "dim_in" in err(), err()
    for L in (1, LIB_MAX + 1):
        assert _call(h, L=L) == INVALID and "n_layers" in err(), err()
    for n in (-1, 1 << 31):
        assert _call(h, n=n) == INVALID and "out of range" in err(), err()


def test_ops_reject_cpu_tensors_and_mismatched_shapes(lib, monkeypatch):
    from mri_interpolation_amd import ops
    assert ops.rff_gradient_supported(4, 64, 64, 3, 1) and not ops.rff_gradient_supported(5, 64, 64, 3, 1)
    assert not ops.rff_gradient_supported(3, 128, 64, 6, 1)
    x, b = torch.zeros(4, 3), torch.zeros(64, 3)
    ws, bs = [torch.zeros(64, 128), torch.zeros(1, 64)], [torch.zeros(64), torch.zeros(1)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rff_gradient(x, b, ws, bs)
    # the C side cannot see shapes: a mismatch is refused in ops, on any device
    monkeypatch.setattr(ops, "_gpu", lambda *t: None)

    def reached(*a, **k):
        raise AssertionError("the library was called with mismatched shapes")
    monkeypatch.setattr(ops._lib, "call", reached)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(ops, "_rff_ws", {})  # (the host-side scratch of this test stays its own)
    for kw in (dict(b=torch.zeros(64, 2)), dict(ws=[torch.zeros(64, 64), ws[1]]), dict(bs=bs[:1]),
               dict(y=torch.zeros(5, 1)), dict(dydx=torch.zeros(4, 2))):
        args = dict(b=b, ws=ws, bs=bs, y=None, dydx=None)
        args.update(kw)
        with pytest.raises(ValueError, match="rff_gradient"):
            ops.rff_gradient(x, args["b"], args["ws"], args["bs"], y=args["y"], dydx=args["dydx"])
    with pytest.raises(AssertionError, match="mismatched"):  # (matching shapes do reach the library)
        ops.rff_gradient(x, b, ws, bs)


# ------------------------------------------------------------------------------------------------ model, trainer
def _torch_ops(monkeypatch):
    """The two ops of RffNet.forward restated in plain PyTorch, so that the generic body runs on CPU tensors (the
    library's ops refuse them)."""
    from mri_interpolation_amd import ops
    two_pi = np.float32(2 * np.pi)

    def rff_encode(x, b):
        vp = (two_pi * x) @ b.T
        return torch.cat((torch.cos(vp), torch.sin(vp)), dim=-1)

    def linear_act(x, w, b, act=ops.ACT_IDENTITY, w0=1.0):
        z = F.linear(x, w, b)
        return {ops.ACT_IDENTITY: lambda: z, ops.ACT_RELU: lambda: torch.relu(z)}[act]()

    monkeypatch.setattr(ops, "rff_encode", rff_encode)
    monkeypatch.setattr(ops, "linear_act", linear_act)


def test_on_the_cpu_both_forms_are_the_generic_body(lib, monkeypatch):
    from mri_interpolation_amd import models, ops
    _torch_ops(monkeypatch)
    calls = []
    monkeypatch.setattr(ops, "rff_gradient", lambda *a, **k: calls.append(1))
    torch.manual_seed(4)
    net = models.RffNet(3, 64, 1, 3, n_frequencies=64, sigma=1.0)
    x = torch.rand(37, 3)
    assert net._inference_plan(x) is None
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
    assert calls == [], "the kernel cannot serve a CPU tensor"
    with pytest.raises(ValueError, match="dim_out"):
        models.RffNet(3, 64, 2, 3, n_frequencies=64).forward_with_gradient(x, fused=True)
    with pytest.raises(ValueError, match="dim_out"):
        models.RffNet(3, 64, 2, 3, n_frequencies=64).forward_with_gradient(x)


def test_trainer_passes_fused_only_for_an_rff_net_under_fused_rff(monkeypatch):
    """Trainer.predict_with_gradient, seen through spies on the classes' methods (the models stay where they are: a
    parameter that claims to be on the GPU keeps the trainer from moving them)."""
    from mri_interpolation_amd import models, trainer
    seen = []

    def spy(name):
        def forward_with_gradient(self, x, **kw):
            seen.append((name, dict(kw)))
            return torch.zeros(x.shape[0], 1), torch.zeros(x.shape[0], x.shape[1])
        return forward_with_gradient

    monkeypatch.setattr(models.RffNet, "forward_with_gradient", spy("rff"))
    monkeypatch.setattr(models.ModulatedSirenNet, "forward_with_gradient", spy("modulated"))
    monkeypatch.setattr(models.SirenNet, "forward_with_gradient", spy("plain"))
    monkeypatch.setattr(torch.nn.Module, "cuda", lambda self, *a, **k: self)
    loader = [(torch.zeros(5, 3), None), (torch.zeros(2, 3), None)]
    nets = (models.RffNet(3, 64, 1, 3, n_frequencies=64), models.ModulatedSirenNet(3, 64, 1, 3),
            models.SirenNet(3, 64, 1, 3))
    for kw in (dict(fused_rff=True), {}):
        tr = trainer.Trainer(max_epochs=1, log_every=0, distributed=False, **kw)
        for net in nets:
            ys, gs = tr.predict_with_gradient(net, loader)
            assert [tuple(y.shape) for y in ys] == [(5, 1), (2, 1)] and [tuple(g.shape) for g in gs] == [(5, 3), (2, 3)]
    others = [("modulated", {})] * 2 + [("plain", {})] * 2
    assert seen == [("rff", dict(fused=True))] * 2 + others + [("rff", {})] * 2 + others
    assert trainer.Trainer(max_epochs=1, distributed=False).fused_rff is False
