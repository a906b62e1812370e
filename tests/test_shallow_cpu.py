"""The shallow decoder's host side: ABI symbols, shape support, workspace sizes, argument validation before any
device call, FusedStep's plan predicate and the launcher flag.  CPU only (the kernels: tests/test_gpu_shallow.py)."""
import ctypes as C
import itertools
import os
import re

import pytest
import torch

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mri_inr.h")
SYMBOLS = ("mri_shallow_mlp_supported", "mri_shallow_mlp_workspace_bytes", "mri_shallow_mlp_forward",
           "mri_shallow_mlp_train")
IDENTITY, RELU, SINE, GELU = 0, 1, 2, 3
FUSED_ACTS = (IDENTITY, RELU, GELU)


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
    assert "mri_shallow_mlp_workspace_bytes" in lib.INT64_GETTERS and "mri_shallow_mlp_supported" in lib.INT_GETTERS
    from mri_interpolation_amd import ops
    assert all(callable(getattr(ops, f)) for f in ("shallow_mlp_supported", "shallow_mlp_forward",
                                                   "shallow_mlp_train"))
    # the header cites what it replaces
    text = open(HEADER).read()
    block = text[text.index("fused shallow decoder"):text.index("mri_shallow_mlp_supported(")]
    assert "models.py:712-739" in block and "cell 37" in block


def test_supported_shapes(lib):
    h = lib.load()
    for (k, hidden), (a, b) in itertools.product([(16, 64), (4, 64), (32, 128), (5, 32)],
                                                 itertools.product(FUSED_ACTS, FUSED_ACTS)):
        assert h.mri_shallow_mlp_supported(k, hidden, 1, a, b) == 1, (k, hidden, a, b)
    assert h.mri_shallow_mlp_supported(33, 64, 1, GELU, GELU) == 0
    assert h.mri_shallow_mlp_supported(0, 64, 1, GELU, GELU) == 0
    assert h.mri_shallow_mlp_supported(16, 96, 1, GELU, GELU) == 0
    assert h.mri_shallow_mlp_supported(16, 64, 2, GELU, GELU) == 0
    assert h.mri_shallow_mlp_supported(16, 64, 1, SINE, GELU) == 0
    assert h.mri_shallow_mlp_supported(16, 64, 1, GELU, SINE) == 0


def test_workspace_bytes(lib):
    h = lib.load()
    for k, hidden in [(16, 64), (4, 64), (32, 128), (5, 32)]:
        sizes = [h.mri_shallow_mlp_workspace_bytes(k, hidden, n) for n in (1, 31, 384, 20000, 70001, 1 << 18, 1 << 22)]
        assert sizes[0] >= (hidden * k + 2 * hidden + 2) * 4  # at least one slab of partial sums
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
        assert sizes[-1] <= 64 << 20
    assert h.mri_shallow_mlp_workspace_bytes(33, 64, 1000) == -1
    assert h.mri_shallow_mlp_workspace_bytes(16, 96, 1000) == -1


def _train_args(n=8, n_total=8, k=16, hidden=64, acts=(GELU, GELU), ptr=None, ws=None, ws_bytes=0, divisor=1.0):
    p = ptr
    return (p, p, n, n_total, k, hidden, p, p, p, p, acts[0], acts[1], divisor, p, p, p, p, p, p, p, 1, ws, ws_bytes,
            None)


def test_validation_before_touching_the_device(lib):
    h = lib.load()
    fwd = lambda n, k=16, hidden=64, acts=(GELU, GELU), p=None: h.mri_shallow_mlp_forward(  # noqa: E731
        p, n, k, hidden, p, p, p, p, acts[0], acts[1], p, None)
    assert len(_train_args()) == len(lib.SIGNATURES["mri_shallow_mlp_train"])
    # n = 0: a no-op, whatever the buffers
    assert fwd(0) == 0 and h.mri_shallow_mlp_train(*_train_args(n=0, n_total=0)) == 0
    assert h.mri_shallow_mlp_train(*_train_args(n=0, n_total=5)) == 0

    def refused(rc, word):
        assert rc == -1
        msg = h.mri_last_error().decode()
        assert msg and word in msg, msg

    # NULL buffers
    refused(fwd(8), "NULL")
    refused(h.mri_shallow_mlp_train(*_train_args()), "NULL")
    # a fake, never dereferenced address for the data: the gradient buffers and the workspace are still checked
    fake = C.c_void_p(4096)
    need = h.mri_shallow_mlp_workspace_bytes(16, 64, 8)
    refused(h.mri_shallow_mlp_train(*_train_args(ptr=fake, ws=None, ws_bytes=need)), "workspace")
    refused(h.mri_shallow_mlp_train(*_train_args(ptr=fake, ws=fake, ws_bytes=need - 1)), "workspace")
    # negative n, a slice larger than its batch, a divisor that is no divisor
    refused(fwd(-1, p=fake), "negative")
    refused(h.mri_shallow_mlp_train(*_train_args(n=-1, ptr=fake, ws=fake, ws_bytes=need)), "n")
    refused(h.mri_shallow_mlp_train(*_train_args(n=8, n_total=7, ptr=fake, ws=fake, ws_bytes=need)), "batch")
    refused(h.mri_shallow_mlp_train(*_train_args(ptr=fake, ws=fake, ws_bytes=need, divisor=0.0)), "grad_divisor")
    # unsupported shapes and activations
    refused(fwd(8, k=33, p=fake), "not supported")
    refused(fwd(8, hidden=96, p=fake), "not supported")
    refused(fwd(8, acts=(SINE, GELU), p=fake), "not supported")
    refused(h.mri_shallow_mlp_train(*_train_args(k=33, ptr=fake, ws=fake, ws_bytes=1 << 20)), "not supported")
    refused(h.mri_shallow_mlp_train(*_train_args(acts=(GELU, SINE), ptr=fake, ws=fake, ws_bytes=1 << 20)),
            "not supported")


def test_ops_reject_cpu_tensors(lib):
    from mri_interpolation_amd import ops
    x, w1, b1, w2, b2 = torch.zeros(16, 8), torch.zeros(64, 16), torch.zeros(64), torch.zeros(1, 64), torch.zeros(1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.shallow_mlp_forward(x, [(w1, b1), (w2, b2)], (GELU, GELU))


def test_plan_predicate(lib):
    """FusedStep._shallow_plan needs a device; its decision is this pure function of shapes and codes."""
    from mri_interpolation_amd.trainer import shallow_plan_matches as plan
    nb = dict(has_encoder=True, batch_norm=False, shapes=[(64, 16), (1, 64)], has_bias=[True, True],
              activations=[GELU, GELU])
    assert plan(**nb)
    for a, b in itertools.product(FUSED_ACTS, FUSED_ACTS):
        assert plan(**dict(nb, activations=[a, b]))
    assert plan(**dict(nb, shapes=[(128, 32), (1, 128)])) and plan(**dict(nb, shapes=[(32, 5), (1, 32)]))
    assert not plan(**dict(nb, has_encoder=False))
    assert not plan(**dict(nb, batch_norm=True))
    assert not plan(**dict(nb, has_bias=[True, False])) and not plan(**dict(nb, has_bias=[False, True]))
    assert not plan(**dict(nb, activations=[SINE, GELU])) and not plan(**dict(nb, activations=[GELU, SINE]))
    assert not plan(**dict(nb, shapes=[(64, 16), (2, 64)]))          # dim_out 2
    assert not plan(**dict(nb, shapes=[(64, 16), (1, 32)]))          # widths that do not chain
    assert not plan(**dict(nb, shapes=[(96, 16), (1, 96)]))          # no kernel of that width
    assert not plan(**dict(nb, shapes=[(64, 33), (1, 64)]))          # k_in beyond the kernel
    three = dict(nb, shapes=[(64, 16), (64, 64), (1, 64)], has_bias=[True] * 3, activations=[RELU, RELU, IDENTITY])
    assert not plan(**three)                                          # the tiny-MLP plan's shape, not this one
    assert not plan(**dict(nb, shapes=[(1, 16)], has_bias=[True], activations=[GELU]))
    # the kernel's own word is asked last and decides
    asked = []
    assert not plan(**nb, supported=lambda *a: asked.append(a) or False)
    assert asked == [(16, 64, 1, GELU, GELU)]


def test_launcher_no_batchnorm_builds_the_notebook_decoder(lib):
    import launcher
    from mri_interpolation_amd import config as cfg, models, ops
    args = launcher.parse_args(["--no_batchnorm"])
    assert args.no_batchnorm and not args.tiny_mlp and not launcher.parse_args([]).no_batchnorm
    config = cfg.HashConfig().resolve((48, 40, 32))
    assert config.batch_norm
    launcher.apply_decoder_flags(config, args)
    net = launcher.build_model(config, models)
    assert isinstance(net, models.HashMLP) and len(net.decoder) == 2
    assert not any(isinstance(m, torch.nn.BatchNorm1d) for m in net.modules())
    assert [blk[0].activation_code for blk in net.decoder] == [ops.ACT_GELU, ops.ACT_GELU]
    # without the flag the BatchNorm blocks stay; on another model class the flag changes nothing
    plain = cfg.HashConfig().resolve((48, 40, 32))
    launcher.apply_decoder_flags(plain, launcher.parse_args([]))
    assert sum(isinstance(m, torch.nn.BatchNorm1d) for m in launcher.build_model(plain, models).modules()) == 2
    siren = cfg.BaseConfig().resolve((48, 40))
    assert launcher.apply_decoder_flags(siren, args) is siren and not hasattr(siren, "batch_norm")
