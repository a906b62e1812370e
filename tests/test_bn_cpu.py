"""The fused BatchNorm step's host side: ABI symbols, the BatchNorm plan of `fusable_layers`, every refusal
with its reason, the Trainer keyword and the launcher flag.  CPU only (the kernels: tests/test_gpu_bn.py)."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mri_inr.h")
BN_SYMBOLS = ("mri_bn_stats", "mri_bn_act_forward", "mri_bn_act_backward", "mri_bn_workspace_bytes")


@pytest.fixture(scope="module")
def lib():
    from mri_interpolation_amd import _lib
    from mri_interpolation_amd.build import build
    build()
    return _lib


def default_hashmlp(**kw):
    """The reference's default model family (config/base.py HashConfig) at a small size: Linear ->
    BatchNorm1d -> GELU -> Dropout(0) blocks, also on the last layer."""
    from mri_interpolation_amd import models
    args = dict(dim_in=3, n_levels=4, n_features_per_level=1, log2_hashmap_size=12, base_resolution=(8, 8, 4),
                finest_resolution=(32, 32, 16), dim_hidden=64, dim_out=1, n_layers=2, lr=5e-3)
    args.update(kw)
    return models.HashMLP(**args)


def _header_arguments(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared in mri_inr.h"
    return [a for a in m.group(1).split(",") if a.strip()]


def test_bn_symbols_are_declared_bound_and_exported(lib):
    handle = lib.load()
    bound = dict(lib.SIGNATURES)
    bound.update(lib.INT64_GETTERS)
    for name in BN_SYMBOLS:
        assert name in bound, f"{name} has no signature in _lib"
        assert len(_header_arguments(name)) == len(bound[name]), name
        assert hasattr(handle, name), f"{name} is not exported by the library"
    assert "mri_bn_workspace_bytes" in lib.INT64_GETTERS


def test_bn_entry_points_validate_before_touching_the_device(lib):
    h = lib.load()
    # workspace: chunk sums (float64, two per feature and chunk) + two batch means per feature
    assert h.mri_bn_workspace_bytes(10000, 64) >= 2 * 64 * 8 + 2 * 64 * 4
    assert h.mri_bn_workspace_bytes(1 << 20, 256) <= 8 << 20
    assert h.mri_bn_workspace_bytes(16, 0) == -1 and h.mri_bn_workspace_bytes(16, 1 << 20) == -1
    # n < 2 in training: refused with the reason, as nn.BatchNorm1d refuses it
    assert h.mri_bn_stats(None, 64, 1, 64, 0.1, 1e-5, None, None, None, None, None, 0, None) == -1
    assert "n >= 2" in h.mri_last_error().decode()
    assert h.mri_bn_act_backward(None, 64, None, 64, 1, 64, None, None, None, 0, None, 64, None, None, 0, None, 0,
                                 None) == -1
    assert "n >= 2" in h.mri_last_error().decode()
    # NULL buffers, a bad activation, a short leading dimension
    assert h.mri_bn_stats(None, 64, 8, 64, 0.1, 1e-5, None, None, None, None, None, 0, None) == -1
    assert h.mri_bn_act_forward(None, 64, 8, 64, None, None, None, 1e-5, None, None, 0, None, 64, None) == -1
    assert h.mri_bn_act_forward(None, 64, 8, 64, None, None, None, 1e-5, None, None, 2, None, 64, None) == -1
    assert "activation" in h.mri_last_error().decode()  # sine is not a BatchNorm epilogue
    assert h.mri_bn_act_forward(None, 32, 8, 64, None, None, None, 1e-5, None, None, 0, None, 64, None) == -1
    assert h.mri_bn_act_backward(None, 64, None, 64, 8, 64, None, None, None, 0, None, 64, None, None, 0, None, 0,
                                 None) == -1
    # an empty inference batch is a no-op
    assert h.mri_bn_act_forward(None, 64, 0, 64, None, None, None, 1e-5, None, None, 0, None, 64, None) == 0


def test_default_hashmlp_is_a_plan_only_with_batch_norm():
    from mri_interpolation_amd import ops, trainer
    net = default_hashmlp()
    assert trainer.fusable_layers(net) is None  # today's default: training_step + autograd
    enc, layers = trainer.fusable_layers(net, batch_norm=True)
    assert enc is net.encoder and len(layers) == len(net.decoder) == 2
    for layer, block in zip(layers, net.decoder):
        assert layer.bn is block[1] and isinstance(layer.bn, torch.nn.BatchNorm1d)
        assert layer.weight is block[0].weight and layer.bias is block[0].bias
        assert layer.activation == ops.ACT_IDENTITY and layer.bn_activation == ops.ACT_GELU
    # three blocks, ReLU, a linear last block (nn.Identity behind the BatchNorm)
    net3 = default_hashmlp(n_layers=3, dim_hidden=128, n_features_per_level=2, activation=torch.nn.ReLU,
                           final_activation=False)
    _, layers3 = trainer.fusable_layers(net3, batch_norm=True)
    assert [l.bn_activation for l in layers3] == [ops.ACT_RELU, ops.ACT_RELU, ops.ACT_IDENTITY]
    # the keyword changes nothing for the models that fuse without it
    tiny = default_hashmlp(n_layers=3, activation=torch.nn.ReLU, batch_norm=False, final_activation=False)
    plain, with_kw = trainer.fusable_layers(tiny), trainer.fusable_layers(tiny, batch_norm=True)
    assert plain is not None and all(l.bn is None for l in with_kw[1])
    assert [l.activation for l in plain[1]] == [l.activation for l in with_kw[1]]


def _refused(net, match, world=1):
    from mri_interpolation_amd import trainer
    with pytest.raises(ValueError, match=match):
        trainer.FusedStep(net, net.configure_optimizers(), world, batch_norm=True)


def test_every_refusal_raises_value_error_with_its_reason():
    _refused(default_hashmlp(), "shard-invariant", world=2)
    _refused(default_hashmlp(dropout=0.25), "dropout p = 0.25")
    _refused(default_hashmlp(activation=torch.nn.Tanh), "Tanh")
    net = default_hashmlp()
    net.decoder[0][2] = torch.nn.GELU(approximate="tanh")  # only the erf form has a kernel
    _refused(net, "no fused code")
    for kw, reason in ((dict(momentum=None), "momentum=None"),
                       (dict(track_running_stats=False), "track_running_stats=False"),
                       (dict(affine=False), "affine=False")):
        net = default_hashmlp()
        net.decoder[1][1] = torch.nn.BatchNorm1d(1, **kw)
        _refused(net, reason)
    # without the keyword the model is "not a fusable chain", whatever its BatchNorm looks like
    from mri_interpolation_amd import trainer
    with pytest.raises(ValueError, match="not a fusable chain"):
        trainer.FusedStep(default_hashmlp(), default_hashmlp().configure_optimizers())


def test_trainer_keyword_and_launcher_flag():
    import launcher
    from mri_interpolation_amd.trainer import Trainer
    assert Trainer(distributed=False).fused_batchnorm is False
    assert Trainer(distributed=False, fused_batchnorm=True).fused_batchnorm is True
    assert launcher.parse_args([]).fused_batchnorm is False
    args = launcher.parse_args(["--synthetic", "32,32,16", "--fused_batchnorm", "--max_steps", "20"])
    assert args.fused_batchnorm is True and args.max_steps == 20


def test_steady_loop_refuses_the_batchnorm_plan():
    from mri_interpolation_amd import trainer
    step = type("S", (), dict(psf=None, bn=True))()
    assert "BatchNorm" in trainer.SteadyLoop.unsupported(step, type("P", (), dict(loader=None))())


def test_ops_wrappers_reject_cpu_tensors_and_bad_shapes():
    from mri_interpolation_amd import ops
    z = torch.zeros(8, 4)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.bn_stats(z)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.bn_act_forward(z, torch.ones(4), torch.zeros(4), save=torch.zeros(2, 4))
    assert ops.bn_workspace_bytes(8, 4) > 0
    with pytest.raises(ValueError, match="supported shape"):
        ops.bn_workspace_bytes(8, 5000)
    assert C.sizeof(C.c_double) == 8  # the workspace is counted in float64 elements
