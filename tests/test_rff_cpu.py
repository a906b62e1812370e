"""RffNet without a device: the C ABI of csrc/rff.hip (symbols, the supported set, argument validation before any HIP
call), and the layers above the kernels as far as they can be seen without a GPU -- the class's state dict against the
reference's fixture, the frozen projection, reference-layout checkpoints, the launcher's flags.  CPU only."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import REL_TOL, ROOT, assert_close, load_golden

INVALID = -1  # MRI_ERR_INVALID_ARGUMENT
LIB_MAX = 8   # MRI_SIREN_MAX_LAYERS
NAMES = ("mri_rff_encode", "mri_rff_encode_backward_input", "mri_rff_forward_supported",
         "mri_rff_forward_workspace_bytes", "mri_rff_forward")


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
    assert len(lib.SIGNATURES["mri_rff_encode"]) == 7 and len(lib.SIGNATURES["mri_rff_encode_backward_input"]) == 8
    assert len(lib.SIGNATURES["mri_rff_forward"]) == 13
    assert "mri_rff_forward_workspace_bytes" in lib.INT64_GETTERS and "mri_rff_forward_supported" in lib.INT_GETTERS
    assert "csrc/rff.hip" in open(os.path.join(ROOT, "include", "mri_inr.h")).read()
    from mri_interpolation_amd import build
    assert "rff.hip" in build.SOURCES


def test_supported_truth_table_and_workspace(lib):
    h = lib.load()
    for hidden in (64, 128):
        for dim_in in (1, 2, 3, 4):
            for L in range(2, LIB_MAX + 1):
                assert h.mri_rff_forward_supported(dim_in, hidden, hidden, L, 1) == 1, (dim_in, hidden, L)
        for L in range(2, LIB_MAX + 1):  # n_layers split hidden x hidden matrices in three bf16 terms
            assert h.mri_rff_forward_workspace_bytes(hidden, L) == L * 6 * hidden * hidden
    for hidden, n_freq in ((128, 64), (64, 128), (128, 127), (64, 1)):
        assert h.mri_rff_forward_supported(3, hidden, n_freq, 6, 1) == 0, (hidden, n_freq)
    for hidden in (32, 256):
        assert h.mri_rff_forward_supported(3, hidden, hidden, 6, 1) == 0, hidden
        assert h.mri_rff_forward_workspace_bytes(hidden, 6) == -1
    for dim_in in (0, 5):
        assert h.mri_rff_forward_supported(dim_in, 128, 128, 6, 1) == 0, dim_in
    for L in (1, LIB_MAX + 1):
        assert h.mri_rff_forward_supported(3, 128, 128, L, 1) == 0, L
        assert h.mri_rff_forward_workspace_bytes(128, L) == -1
    assert h.mri_rff_forward_supported(3, 128, 128, 6, 2) == 0


def _forward(h, x=64, b=64, w=None, bias=None, y=64, ws=256, ws_bytes=1 << 30, n=8, dim_in=3, hidden=64, n_freq=None,
             L=3):
    """mri_rff_forward with fake (never dereferenced) device addresses; weight / bias default to real HOST arrays of
    fake device pointers, 0 stands for a NULL array.  Every call here is refused before anything is launched."""
    arr = (C.c_void_p * LIB_MAX)(*[256] * LIB_MAX)
    w, bias = [arr if a is None else (None if isinstance(a, int) else a) for a in (w, bias)]
    p = lambda v: None if v is None else C.c_void_p(v)  # noqa: E731
    return h.mri_rff_forward(p(x), n, dim_in, hidden, hidden if n_freq is None else n_freq, L, p(b), w, bias, p(y),
                             p(ws), ws_bytes, None)


def test_forward_refusals_name_their_argument(lib):
    h = lib.load()
    err = lambda: h.mri_last_error().decode()  # noqa: E731
    # an empty batch is a no-op and touches no device
    assert h.mri_rff_forward(None, 0, 3, 64, 64, 3, None, None, None, None, None, 0, None) == 0
    for name, kw in (("x", dict(x=None)), ("b", dict(b=None)), ("weight", dict(w=0)), ("bias", dict(bias=0)),
                     ("y", dict(y=None)), ("workspace", dict(ws=None))):
        assert _forward(h, **kw) == INVALID, name
        assert name in err(), (name, err())
    null_layer = (C.c_void_p * LIB_MAX)(*([256] * 2 + [None] + [256] * (LIB_MAX - 3)))
    assert _forward(h, w=null_layer) == INVALID and "weight[2]" in err(), err()
    assert _forward(h, bias=null_layer) == INVALID and "bias[2]" in err(), err()
    need = h.mri_rff_forward_workspace_bytes(64, 3)
    assert _forward(h, ws=256 + 4) == INVALID and "workspace" in err() and "16-byte" in err(), err()
    assert _forward(h, ws_bytes=need - 1) == INVALID and "workspace" in err() and str(need) in err(), err()
    assert _forward(h, ws_bytes=need, x=None) == INVALID and "x" in err()  # (the exact size passes that check)
    for name in ("x", "b", "y"):
        assert _forward(h, **{name: 64 + 2}) == INVALID and name in err() and "4-byte" in err(), (name, err())
    for hidden in (32, 96, 256):
        assert _forward(h, hidden=hidden) == INVALID and "hidden" in err(), err()
    assert _forward(h, hidden=128, n_freq=64) == INVALID and "n_freq" in err(), err()
    for dim_in in (0, 5, 8):
        assert _forward(h, dim_in=dim_in) == INVALID and "dim_in" in err(), err()
    for L in (1, LIB_MAX + 1):
        assert _forward(h, L=L) == INVALID and "n_layers" in err(), err()
    for n in (-1, 1 << 31):
        assert _forward(h, n=n) == INVALID and "out of range" in err(), err()


def test_encode_refusals_name_their_argument(lib):
    h = lib.load()
    err = lambda: h.mri_last_error().decode()  # noqa: E731
    p = C.c_void_p
    assert h.mri_rff_encode(None, 0, 3, None, 128, None, None) == 0
    assert h.mri_rff_encode_backward_input(None, 0, 3, None, 128, None, None, None) == 0
    for name, args in (("x", (None, 8, 3, p(64), 16, p(64), None)), ("b", (p(64), 8, 3, None, 16, p(64), None)),
                       ("z", (p(64), 8, 3, p(64), 16, None, None)), ("dim_in", (p(64), 8, 9, p(64), 16, p(64), None)),
                       ("dim_in", (p(64), 8, 0, p(64), 16, p(64), None)), ("n_freq", (p(64), 8, 3, p(64), 0, p(64), None)),
                       ("z", (p(64), 8, 3, p(64), 16, p(66), None)), ("x", (p(66), 8, 3, p(64), 16, p(64), None))):
        assert h.mri_rff_encode(*args) == INVALID and name in err(), (name, err())
    for name, args in (("x", (None, 8, 3, p(64), 16, p(64), p(64), None)), ("b", (p(64), 8, 3, None, 16, p(64), p(64), None)),
                       ("dz", (p(64), 8, 3, p(64), 16, None, p(64), None)), ("dx", (p(64), 8, 3, p(64), 16, p(64), None, None)),
                       ("dim_in", (p(64), 8, 9, p(64), 16, p(64), p(64), None)),
                       ("dx", (p(64), 8, 3, p(64), 16, p(64), p(66), None))):
        assert h.mri_rff_encode_backward_input(*args) == INVALID and name in err(), (name, err())


def test_ops_reject_cpu_tensors(lib):
    from mri_interpolation_amd import ops
    assert ops.rff_forward_supported(3, 128, 128, 6, 1) and not ops.rff_forward_supported(3, 128, 64, 6, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rff_encode(torch.zeros(4, 3), torch.zeros(16, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rff_forward(torch.zeros(4, 3), torch.zeros(64, 3), [torch.zeros(64, 128), torch.zeros(1, 64)],
                        [torch.zeros(64), torch.zeros(1)])


def test_rff_forward_checks_shapes_before_the_library_sees_pointers(lib, monkeypatch):
    """The C side cannot see shapes: a mismatched b or weight must be refused in ops, on any device."""
    from mri_interpolation_amd import ops
    monkeypatch.setattr(ops, "_gpu", lambda *t: None)

    def reached(*a, **k):
        raise AssertionError("the library was called with mismatched shapes")
    monkeypatch.setattr(ops._lib, "call", reached)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    x, b = torch.zeros(4, 3), torch.zeros(64, 3)
    ws, bs = [torch.zeros(64, 128), torch.zeros(64, 64), torch.zeros(1, 64)], [torch.zeros(64), torch.zeros(64), torch.zeros(1)]
    bad = [dict(b=torch.zeros(64, 2)), dict(b=torch.zeros(32, 3)), dict(b=torch.zeros(64)),
           dict(ws=[torch.zeros(64, 64)] + ws[1:]), dict(ws=[ws[0], torch.zeros(64, 32), ws[2]]),
           dict(ws=ws[:2] + [torch.zeros(2, 64)]), dict(ws=ws[:2] + [torch.zeros(1, 32)]),
           dict(bs=[torch.zeros(32)] + bs[1:]), dict(bs=bs[:2] + [torch.zeros(2)]), dict(bs=bs[:2]),
           dict(ws=ws[2:], bs=bs[2:])]
    for kw in bad:
        args = dict(b=b, ws=ws, bs=bs)
        args.update(kw)
        with pytest.raises(ValueError, match="rff_forward"):
            ops.rff_forward(x, args["b"], args["ws"], args["bs"])
    with pytest.raises(AssertionError, match="mismatched"):  # (matching shapes do reach the library)
        ops.rff_forward(x, b, ws, bs)


# ------------------------------------------------------------------------------------------------ the class
def _torch_ops(monkeypatch):
    """The two ops of RffNet.forward restated in plain PyTorch, so that the layer path runs on CPU tensors."""
    from mri_interpolation_amd import ops

    def linear_act(x, w, b, act=ops.ACT_IDENTITY, w0=1.0):
        z = F.linear(x, w, b)
        return {ops.ACT_IDENTITY: lambda: z, ops.ACT_RELU: lambda: torch.relu(z), ops.ACT_GELU: lambda: F.gelu(z)}[act]()

    def rff_encode(x, b):
        vp = (float(np.float32(2 * np.pi)) * x) @ b.T
        return torch.cat((torch.cos(vp), torch.sin(vp)), dim=-1)

    monkeypatch.setattr(ops, "linear_act", linear_act)
    monkeypatch.setattr(ops, "rff_encode", rff_encode)


def net_from_fixture(fx, **kw):
    from mri_interpolation_amd import models
    m = fx.meta
    net = models.RffNet(dim_in=m["dim_in"], dim_hidden=m["dim_hidden"], dim_out=1, n_layers=m["n_layers"],
                        n_frequencies=m["n_frequencies"], sigma=m["sigma"], lr=m.get("lr", 1e-4), **kw)
    sd = {"encoder.b": torch.from_numpy(fx["b"])}
    for i in range(m["n_layers"]):
        sd[f"decoder.{2 * i}.weight"] = torch.from_numpy(fx[f"w_{i}"])
        sd[f"decoder.{2 * i}.bias"] = torch.from_numpy(fx[f"b_{i}"])
    net.load_state_dict(sd)
    return net


@pytest.mark.parametrize("name", ["rff_2d_3x64", "rff_3d_6x128", "e2e_rff_adam"])
def test_state_dict_is_the_reference_s_without_the_dead_stack(lib, name):
    fx = load_golden(name)
    m = fx.meta
    assert m["min_abs_preactivation"] >= 1e-5 and m["rows"] == 192
    net = net_from_fixture(fx)
    sd = net.state_dict()
    assert sorted(sd.keys()) == m["state_dict_keys"]
    assert {k: list(v.shape) for k, v in sd.items()} == m["shapes"]
    assert list(sd.keys())[0] == "encoder.b" and not any(k.startswith("layers.") for k in sd)
    assert m["dead_keys"] and all(k.startswith("layers.") for k in m["dead_keys"])  # the reference does carry it
    assert not hasattr(net, "layers")


def test_b_is_frozen_and_adam_does_not_count_it(lib):
    from mri_interpolation_amd import encoding, models
    torch.manual_seed(3)
    net = models.RffNet(3, 64, 1, 3, n_frequencies=64, sigma=10.0)
    b = net.encoder.b
    assert isinstance(net.encoder, encoding.GaussianEncoding) and isinstance(b, nn.Parameter)
    assert b.shape == (64, 3) and not b.requires_grad
    assert 5.0 < float(b.std()) < 15.0  # randn * sigma
    opt = net.configure_optimizers()
    held = list(opt._params)
    assert all(p is not b for p in held) and len(held) == 6
    assert {id(p) for p in held} == {id(p) for p in net.parameters() if p.requires_grad}
    assert (net.n_frequencies, net.sigma, net.lr, net.dim_in, net.dim_hidden, net.n_layers) == (64, 10.0, 1e-4, 3, 64, 3)
    with pytest.raises(ValueError):
        encoding.GaussianEncoding(sigma=1.0)
    assert encoding.GaussianEncoding(b=torch.ones(5, 2)).b.shape == (5, 2)


def test_reference_layout_checkpoint_with_dead_layers_loads(lib, tmp_path):
    from mri_interpolation_amd import checkpoint
    fx = load_golden("rff_2d_3x64")
    net = net_from_fixture(fx)
    ref_sd = checkpoint.reference_state_dict(net)
    dead = [k for k in ref_sd if k.startswith("layers.")]
    assert dead == [f"layers.{2 * i}.{p}" for i in range(8) for p in ("weight", "bias")]  # BaseMLP's own defaults
    assert sorted(dead) == sorted(fx.meta["dead_keys"])
    assert ref_sd["layers.0.weight"].shape == (128, 2) and ref_sd["layers.14.weight"].shape == (1, 128)
    assert list(ref_sd)[len(dead)] == "encoder.b"
    path = str(tmp_path / "rff.ckpt")
    ckpt = checkpoint.save(path, net, epoch=0, global_step=0)
    names = checkpoint._reference_parameter_names(net)
    assert ckpt["optimizer_states"][0]["param_groups"][0]["params"] == list(range(len(names))) and "encoder.b" in names
    other = net_from_fixture(fx)
    with torch.no_grad():
        for p in other.parameters():
            p.add_(1.0)
    checkpoint.load(path, other)
    for (k, a), (_, b) in zip(net.state_dict().items(), other.state_dict().items()):
        assert torch.equal(a, b), k
    assert not other.encoder.b.requires_grad


def test_activation_follows_the_last_linear_and_forward_is_the_reference_s(lib, monkeypatch):
    from mri_interpolation_amd import models, ops
    _torch_ops(monkeypatch)
    for name in ("rff_2d_3x64", "rff_3d_6x128"):
        fx = load_golden(name)
        net = net_from_fixture(fx)
        mods = list(net.decoder)
        assert len(mods) == 2 * fx.meta["n_layers"]
        assert all(isinstance(m, models.FusedLinear) and m.activation_code == ops.ACT_RELU for m in mods[0::2])
        assert all(isinstance(m, models._Fused) for m in mods[1::2])
        assert mods[-2].out_features == 1 and mods[0].in_features == 2 * fx.meta["n_frequencies"]
        x = torch.from_numpy(fx["x"])
        pred = net(x).detach()
        assert float(pred.min()) == 0.0 and (fx["pred"] == 0).any(), "the head's ReLU clamps"
        assert_close(pred.detach().numpy(), fx["pred"], REL_TOL, f"{name}: pred on the CPU")
        y, g = net.forward_with_gradient(x)
        assert_close(g.numpy(), fx["dx"], REL_TOL, f"{name}: the input gradient on the CPU")
        assert net._inference_plan(x) is None  # a CPU tensor: the layer path
    gelu = models.RffNet(2, 64, 1, 3, n_frequencies=64, activation=nn.GELU)
    assert all(m.activation_code == ops.ACT_GELU for m in list(gelu.decoder)[0::2])
    assert float(gelu(torch.rand(50, 2)).detach().min()) < 0.0


def test_launcher_parses_the_new_flags_and_builds_the_class(lib):
    import launcher
    from mri_interpolation_amd import config as cfg, models
    args = launcher.parse_args(["--model_class", "RffNet", "--n_frequencies", "64", "--sigma", "5.5", "--dim_hidden", "64",
                                "--n_layers", "3", "--save_gradient"])
    assert (args.model_class, args.n_frequencies, args.sigma) == ("RffNet", 64, 5.5)
    none = launcher.parse_args([])
    assert none.n_frequencies is None and none.sigma is None
    base = cfg.BaseConfig()
    assert (base.n_frequencies, base.sigma) == (128, 10.0)
    config = cfg.apply_overrides(cfg.BaseConfig(), dict(model_class="RffNet", n_frequencies=64, sigma=5.5, dim_hidden=64,
                                                        n_layers=3)).resolve((8, 8, 4))
    net = launcher.build_model(config, models)
    assert isinstance(net, models.RffNet) and net.encoder.b.shape == (64, 3) and net.sigma == 5.5
    assert net.decoder[0].weight.shape == (64, 128) and len(net.decoder) == 6
    launcher.check_save_gradient(models.RffNet, 1)
