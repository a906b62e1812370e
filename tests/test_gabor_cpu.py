"""GaborNet without a device: the C ABI of csrc/gabor.hip (symbols, the supported set, argument validation before any
HIP call), and the layers above the kernels as far as they can be seen without a GPU -- the class's state dict against
the reference's fixture, reference-layout checkpoints, the refusal of the complex layer, the launcher, the trainer's
dispatch.  CPU only."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

import gabor_ref
from conftest import REL_TOL, ROOT, assert_close, load_golden

INVALID = -1  # MRI_ERR_INVALID_ARGUMENT
LIB_MAX = 8   # MRI_SIREN_MAX_LAYERS
NAMES = ("mri_gabor_activation", "mri_gabor_activation_backward", "mri_gabor_forward_supported",
         "mri_gabor_forward_workspace_bytes", "mri_gabor_forward")
FIXTURES = ("gabor_2d_3x64", "gabor_3d_5x128", "e2e_gabor_adam")


@pytest.fixture(scope="module")
def lib():
    from mri_interpolation_amd import _lib
    from mri_interpolation_amd.build import build
    build()
    return _lib


# ------------------------------------------------------------------------------------------------ ABI
def test_symbols_are_declared_bound_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "mri_inr.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    h = lib.load()
    bound = {**lib.SIGNATURES, **lib.INT64_GETTERS, **lib.INT_GETTERS}
    for name in NAMES:
        decl = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert decl, f"{name} is not declared in include/mri_inr.h"
        assert name in bound, f"{name} has no binding in _lib.py"
        assert hasattr(h, name), f"{name} is not exported by the library"
        assert len(bound[name]) == len(decl.group(1).split(",")), f"{name}: the binding's argument count"
        assert re.search(name + r" \(models\.py:\d+", header), f"{name}: no reference line citation in the header"
    assert len(lib.SIGNATURES["mri_gabor_activation"]) == 8 and len(lib.SIGNATURES["mri_gabor_activation_backward"]) == 10
    assert len(lib.SIGNATURES["mri_gabor_forward"]) == 15
    assert "mri_gabor_forward_workspace_bytes" in lib.INT64_GETTERS and "mri_gabor_forward_supported" in lib.INT_GETTERS
    assert "csrc/gabor.hip" in header
    from mri_interpolation_amd import build
    assert "gabor.hip" in build.SOURCES and build.EXTRA_FLAGS["gabor.hip"] == build.EXTRA_FLAGS["rff.hip"]


def test_supported_truth_table_and_workspace(lib):
    h = lib.load()
    for hidden in (64, 128):
        for dim_in in (1, 2, 3, 4):
            for L in range(2, LIB_MAX + 1):
                assert h.mri_gabor_forward_supported(dim_in, hidden, L, 1) == 1, (dim_in, hidden, L)
        for L in range(2, LIB_MAX + 1):  # a freqs / scale pair of split hidden x hidden matrices per square layer
            assert h.mri_gabor_forward_workspace_bytes(hidden, L) == 2 * (L - 2) * 6 * hidden * hidden
    for hidden in (32, 96, 256):
        assert h.mri_gabor_forward_supported(3, hidden, 4, 1) == 0, hidden
        assert h.mri_gabor_forward_workspace_bytes(hidden, 4) == -1
    for dim_in in (0, 5):
        assert h.mri_gabor_forward_supported(dim_in, 128, 4, 1) == 0, dim_in
    for L in (1, LIB_MAX + 1):
        assert h.mri_gabor_forward_supported(3, 128, L, 1) == 0, L
        assert h.mri_gabor_forward_workspace_bytes(128, L) == -1
    assert h.mri_gabor_forward_supported(3, 128, 4, 2) == 0


def _forward(h, x=64, fw=None, fb=None, sw=None, sb=None, y=64, ws=256, ws_bytes=1 << 30, n=8, dim_in=3, hidden=64, L=3,
             w0=5.0, c=1.0):
    """mri_gabor_forward with fake (never dereferenced) device addresses; the four parameter arrays default to real HOST
    arrays of fake device pointers, 0 stands for a NULL array.  Every call here is refused before anything is launched."""
    arr = (C.c_void_p * LIB_MAX)(*[256] * LIB_MAX)
    fw, fb, sw, sb = [arr if a is None else (None if isinstance(a, int) else a) for a in (fw, fb, sw, sb)]
    p = lambda v: None if v is None else C.c_void_p(v)  # noqa: E731
    return h.mri_gabor_forward(p(x), n, dim_in, hidden, L, fw, fb, sw, sb, w0, c, p(y), p(ws), ws_bytes, None)


def test_forward_refusals_name_their_argument(lib):
    h = lib.load()
    err = lambda: h.mri_last_error().decode()  # noqa: E731
    # an empty batch is a no-op and touches no device
    assert h.mri_gabor_forward(None, 0, 3, 64, 3, None, None, None, None, 5.0, 1.0, None, None, 0, None) == 0
    for name, kw in (("x", dict(x=None)), ("y", dict(y=None)), ("freq_weight", dict(fw=0)), ("freq_bias", dict(fb=0)),
                     ("scale_weight", dict(sw=0)), ("scale_bias", dict(sb=0)), ("workspace", dict(ws=None))):
        assert _forward(h, **kw) == INVALID, name
        assert name in err(), (name, err())
    null_layer = (C.c_void_p * LIB_MAX)(*([256] * 2 + [None] + [256] * (LIB_MAX - 3)))
    for key, name in (("fw", "freq_weight"), ("fb", "freq_bias"), ("sw", "scale_weight"), ("sb", "scale_bias")):
        assert _forward(h, **{key: null_layer}) == INVALID and name + "[2]" in err(), err()
    odd_layer = (C.c_void_p * LIB_MAX)(*([256] + [258] + [256] * (LIB_MAX - 2)))
    assert _forward(h, sw=odd_layer) == INVALID and "scale_weight[1]" in err() and "4-byte" in err(), err()
    need = h.mri_gabor_forward_workspace_bytes(64, 3)
    assert need == 12 * 64 * 64
    assert _forward(h, ws=256 + 4) == INVALID and "workspace" in err() and "16-byte" in err(), err()
    assert _forward(h, ws_bytes=need - 1) == INVALID and "workspace" in err() and str(need) in err(), err()
    assert _forward(h, ws_bytes=need, x=None) == INVALID and "x" in err()  # (the exact size passes that check)
    assert _forward(h, L=2, ws=None, ws_bytes=0, x=None) == INVALID and "x is NULL" in err()  # two layers need none
    for name in ("x", "y"):
        assert _forward(h, **{name: 64 + 2}) == INVALID and name in err() and "4-byte" in err(), (name, err())
    for hidden in (32, 96, 256):
        assert _forward(h, hidden=hidden) == INVALID and "hidden" in err(), err()
    for dim_in in (0, 5, 8):
        assert _forward(h, dim_in=dim_in) == INVALID and "dim_in" in err(), err()
    for L in (1, LIB_MAX + 1):
        assert _forward(h, L=L) == INVALID and "n_layers" in err(), err()
    for n in (-1, 1 << 31):
        assert _forward(h, n=n) == INVALID and "out of range" in err(), err()
    assert _forward(h, w0=float("inf")) == INVALID and "w0" in err(), err()
    assert _forward(h, c=float("nan")) == INVALID and "c is not finite" in err(), err()


def test_activation_refusals_name_their_argument(lib):
    h = lib.load()
    err = lambda: h.mri_last_error().decode()  # noqa: E731
    p = C.c_void_p
    assert h.mri_gabor_activation(None, None, 0, 64, 5.0, 1.0, None, None) == 0
    assert h.mri_gabor_activation_backward(None, None, None, 0, 64, 5.0, 1.0, None, None, None) == 0
    for name, args in (("u", (None, p(64), 8, 16, 5.0, 1.0, p(64), None)), ("s", (p(64), None, 8, 16, 5.0, 1.0, p(64), None)),
                       ("out", (p(64), p(64), 8, 16, 5.0, 1.0, None, None)), ("hidden", (p(64), p(64), 8, 0, 5.0, 1.0, p(64), None)),
                       ("out of range", (p(64), p(64), -1, 16, 5.0, 1.0, p(64), None)),
                       ("n * hidden", (p(64), p(64), 1 << 30, 1 << 10, 5.0, 1.0, p(64), None)),
                       ("w0", (p(64), p(64), 8, 16, float("nan"), 1.0, p(64), None)),
                       ("u", (p(66), p(64), 8, 16, 5.0, 1.0, p(64), None)), ("out", (p(64), p(64), 8, 16, 5.0, 1.0, p(66), None))):
        assert h.mri_gabor_activation(*args) == INVALID and name in err(), (name, err())
    ok = (p(64), p(64), p(64), 8, 16, 5.0, 1.0, p(64), p(64), None)
    for name, at, bad in (("u", 0, None), ("s", 1, None), ("g", 2, None), ("du", 7, None), ("ds", 8, None), ("g", 2, p(66)),
                          ("ds", 8, p(66)), ("hidden", 4, 0)):
        args = list(ok)
        args[at] = bad
        assert h.mri_gabor_activation_backward(*args) == INVALID and name in err(), (name, err())


# ------------------------------------------------------------------------------------------------ ops
def test_ops_reject_cpu_tensors(lib):
    from mri_interpolation_amd import ops
    assert ops.gabor_forward_supported(3, 128, 6, 1) and not ops.gabor_forward_supported(3, 32, 6, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gabor_activation(torch.zeros(4, 8), torch.zeros(4, 8), 5.0, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gabor_activation_backward(torch.zeros(4, 8), torch.zeros(4, 8), torch.zeros(4, 8), 5.0, 1.0)
    ws, bs = [torch.zeros(64, 3), torch.zeros(1, 64)], [torch.zeros(64), torch.zeros(1)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gabor_forward(torch.zeros(4, 3), ws, bs, ws, bs, 5.0, 1.0)


def test_gabor_ops_check_shapes_before_the_library_sees_pointers(lib, monkeypatch):
    """The C side cannot see shapes: a mismatched weight must be refused in ops, on any device."""
    from mri_interpolation_amd import ops
    monkeypatch.setattr(ops, "_gpu", lambda *t: None)

    def reached(*a, **k):
        raise AssertionError("the library was called with mismatched shapes")
    monkeypatch.setattr(ops._lib, "call", reached)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    x = torch.zeros(4, 3)
    ws, bs = [torch.zeros(64, 3), torch.zeros(64, 64), torch.zeros(1, 64)], [torch.zeros(64), torch.zeros(64), torch.zeros(1)]
    bad_w = [[torch.zeros(64, 2)] + ws[1:], [ws[0], torch.zeros(64, 32), ws[2]], ws[:2] + [torch.zeros(2, 64)],
             ws[:2] + [torch.zeros(1, 32)], ws[2:], [ws[0].double()] + ws[1:]]
    bad_b = [[torch.zeros(32)] + bs[1:], bs[:2] + [torch.zeros(2)], bs[:2]]
    for w in bad_w:
        for args in ((w, bs, ws, bs), (ws, bs, w, bs)):
            with pytest.raises(ValueError, match="gabor_forward"):
                ops.gabor_forward(x, *args, 5.0, 1.0)
    for b in bad_b:
        for args in ((ws, b, ws, bs), (ws, bs, ws, b)):
            with pytest.raises(ValueError, match="gabor_forward"):
                ops.gabor_forward(x, *args, 5.0, 1.0)
    with pytest.raises(ValueError, match="gabor_forward"):
        ops.gabor_forward(torch.zeros(4, 2), ws, bs, ws, bs, 5.0, 1.0)
    with pytest.raises(ValueError, match="gabor_forward"):
        ops.gabor_forward(x, ws, bs, ws, bs, 5.0, 1.0, y=torch.zeros(3, 1))
    with pytest.raises(ValueError, match="gabor_activation"):
        ops.gabor_activation_forward(torch.zeros(4, 8), torch.zeros(4, 7), 5.0, 1.0)
    with pytest.raises(ValueError, match="gabor_activation_backward"):
        ops.gabor_activation_backward(torch.zeros(4, 8), torch.zeros(4, 8), torch.zeros(4, 7), 5.0, 1.0)
    with pytest.raises(AssertionError, match="mismatched"):  # (matching shapes do reach the library)
        ops.gabor_forward(x, ws, bs, ws, bs, 5.0, 1.0)
    with pytest.raises(AssertionError, match="mismatched"):
        ops.gabor_activation_forward(torch.zeros(4, 8), torch.zeros(4, 8), 5.0, 1.0)


# ------------------------------------------------------------------------------------------------ the class
def _torch_ops(monkeypatch):
    """The two ops of GaborNet.forward restated in plain PyTorch, so that the layer path runs on CPU tensors."""
    from mri_interpolation_amd import ops

    def linear_act(x, w, b, act=ops.ACT_IDENTITY, w0=1.0):
        assert act == ops.ACT_IDENTITY and w0 == 1.0
        return F.linear(x, w, b)

    monkeypatch.setattr(ops, "linear_act", linear_act)
    monkeypatch.setattr(ops, "gabor_activation", lambda u, s, w0, c: torch.cos(w0 * u) * torch.exp(-((s * c) ** 2)))


def net_from_fixture(fx, **kw):
    from mri_interpolation_amd import models
    m = fx.meta
    net = models.GaborNet(models.RealGaborLayer, m["dim_in"], m["dim_hidden"], 1, m["n_layers"], m["sigma"], m["w0"],
                          m.get("lr", 1e-4), **kw)
    sd = {}
    for i, p in enumerate(gabor_ref.fixture_params(fx)):
        for key, t in zip(("freqs.weight", "freqs.bias", "scale.weight", "scale.bias"), p):
            sd[f"layers.{i}.{key}"] = t
    net.load_state_dict(sd)
    return net


@pytest.mark.parametrize("name", FIXTURES)
def test_state_dict_is_the_reference_s(lib, name):
    fx = load_golden(name)
    m = fx.meta
    assert m["reference_f32_vs_f64"] <= 5e-6 and m["rows"] == 192 and (m["w0"], m["sigma"]) == (5.0, 1.0)
    net = net_from_fixture(fx)
    sd = net.state_dict()
    assert sorted(sd.keys()) == m["state_dict_keys"]
    assert {k: list(v.shape) for k, v in sd.items()} == m["shapes"]
    assert list(sd.keys())[:4] == [f"layers.0.{k}" for k in ("freqs.weight", "freqs.bias", "scale.weight", "scale.bias")]
    assert len(sd) == 4 * m["n_layers"]
    assert (net.sigma, net.w0, net.lr, net.dim_in, net.dim_hidden, net.n_layers) == \
        (m["sigma"], m["w0"], m.get("lr", 1e-4), m["dim_in"], m["dim_hidden"], m["n_layers"])
    assert all((l.omega_0, l.scale_0) == (m["w0"], m["sigma"]) for l in net.layers)


def test_forward_is_the_reference_s_and_the_head_is_a_gabor_layer(lib, monkeypatch):
    from mri_interpolation_amd import models
    _torch_ops(monkeypatch)
    for name in FIXTURES[:2]:
        fx = load_golden(name)
        net = net_from_fixture(fx)
        assert all(isinstance(l, models.RealGaborLayer) for l in net.layers) and net.layers[-1].freqs.out_features == 1
        x = torch.from_numpy(fx["x"])
        pred = net(x).detach()
        assert float(pred.abs().max()) <= 1.0
        assert_close(pred.numpy(), fx["pred"], REL_TOL, f"{name}: pred on the CPU")
        y, g = net.forward_with_gradient(x)
        assert_close(g.numpy(), fx["dx"], REL_TOL, f"{name}: the input gradient on the CPU")
        assert net._inference_plan(x) is None  # a CPU tensor: the layer path
        net.criterion = lambda target, pred: F.mse_loss(pred, target)  # (the loss kernel has no CPU form either)
        loss = net.training_step((x, torch.from_numpy(fx["y"])), 0)
        assert abs(float(loss.detach()) - float(fx["loss"])) <= REL_TOL * abs(float(fx["loss"]))


def test_complex_gabor_layer_is_refused(lib):
    from mri_interpolation_amd import models
    with pytest.raises(ValueError, match="ComplexGaborLayer"):
        models.GaborNet(models.ComplexGaborLayer, 3, 64, 1, 3, 1.0, 5.0, 1e-4)
    with pytest.raises(ValueError, match="ComplexGaborLayer"):
        models.ComplexGaborLayer(3, 64)
    with pytest.raises(ValueError, match="layer_cls"):
        models.GaborNet(torch.nn.Linear, 3, 64, 1, 3, 1.0, 5.0, 1e-4)
    net = models.GaborNet(dim_in=3, dim_hidden=64, dim_out=1, n_layers=3)  # the reference's layer defaults
    assert (net.w0, net.sigma, net.layer_cls) == (30.0, 10.0, models.RealGaborLayer)
    lay = models.RealGaborLayer(3, 8)
    assert (lay.omega_0, lay.scale_0, lay.is_first, lay.dim_in) == (30.0, 10.0, False, 3)
    assert models.RealGaborLayer(3, 8, bias=False).freqs.bias is None


def test_reference_layout_checkpoint_round_trips(lib, tmp_path):
    from mri_interpolation_amd import checkpoint
    fx = load_golden("gabor_2d_3x64")
    net = net_from_fixture(fx)
    ref_sd = checkpoint.reference_state_dict(net)
    assert sorted(ref_sd) == fx.meta["state_dict_keys"] and list(ref_sd) == list(net.state_dict())
    path = str(tmp_path / "gabor.ckpt")
    ckpt = checkpoint.save(path, net, epoch=0, global_step=0)
    assert sorted(ckpt["state_dict"]) == fx.meta["state_dict_keys"]
    assert ckpt["optimizer_states"][0]["param_groups"][0]["params"] == list(range(4 * fx.meta["n_layers"]))
    other = net_from_fixture(fx)
    with torch.no_grad():
        for p in other.parameters():
            p.add_(1.0)
    checkpoint.load(path, other)
    for (k, a), (_, b) in zip(net.state_dict().items(), other.state_dict().items()):
        assert torch.equal(a, b), k


# ------------------------------------------------------------------------------------------------ launcher, trainer
def test_launcher_parses_and_builds_the_class(lib):
    import launcher
    from mri_interpolation_amd import config as cfg, models
    args = launcher.parse_args(["--model_class", "GaborNet", "--sigma", "1.5", "--w0", "5", "--dim_hidden", "64",
                                "--n_layers", "3", "--save_gradient"])
    assert (args.model_class, args.sigma, args.w0) == ("GaborNet", 1.5, 5.0) and launcher.parse_args([]).w0 is None
    assert "gabor" not in " ".join(f.name for f in __import__("dataclasses").fields(cfg.BaseConfig)).lower()  # no new field
    config = cfg.apply_overrides(cfg.BaseConfig(), dict(model_class="GaborNet", sigma=1.5, w0=5.0, dim_hidden=64,
                                                        n_layers=3)).resolve((8, 8, 4))
    net = launcher.build_model(config, models)
    assert isinstance(net, models.GaborNet) and (net.sigma, net.w0) == (1.5, 5.0) and net.fused_inference in (True, False)
    assert len(net.layers) == 3 and net.layers[0].freqs.weight.shape == (64, 3) and net.layers[2].scale.weight.shape == (1, 64)
    launcher.check_save_gradient(models.GaborNet, 1)


def test_trainer_keeps_gabornet_on_the_autograd_path(lib):
    from mri_interpolation_amd import models, trainer
    net = models.GaborNet(dim_in=3, dim_hidden=64, dim_out=1, n_layers=3, sigma=1.0, w0=5.0)
    assert trainer.fusable_layers(net) is None
    assert trainer.fusable_layers(net, batch_norm=True, modulated=True, rff=True) is None
    why = trainer.SteadyLoop.unsupported(None, None)
    assert why and "GaborNet" in why and "autograd" in why
    with pytest.raises(ValueError, match="GaborNet"):
        trainer.SteadyLoop(None, None)
