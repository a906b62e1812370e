"""The SIREN coordinate gradient without a device: the C ABI of csrc/siren_gradient.hip (symbols, supported shapes,
workspace, argument validation before any HIP call), the launcher's voxel-unit scale, `launcher.py --save_gradient` on
the CPU path, and which `forward_with_gradient` each model class binds.  CPU only."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

INVALID = -1  # MRI_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def lib():
    from mri_interpolation_amd import _lib
    from mri_interpolation_amd.build import build
    build()
    return _lib


# ------------------------------------------------------------------------------------------------ ABI
def test_symbols_supported_shapes_and_workspace(lib):
    h = lib.load()
    for name in ("mri_siren_gradient_supported", "mri_siren_gradient_workspace_bytes", "mri_siren_gradient"):
        assert hasattr(h, name), name
    for hidden in (64, 128, 256):
        for dim_in in (1, 2, 3):
            for n_sine in range(2, lib.MAX_SIREN_LAYERS + 1):
                assert h.mri_siren_gradient_supported(dim_in, hidden, n_sine, 1) == 1, (dim_in, hidden, n_sine)
                assert h.mri_siren_gradient_workspace_bytes(hidden, n_sine) == \
                    h.mri_siren_forward_workspace_bytes(hidden, n_sine) > 0
    assert h.mri_siren_gradient_supported(2, 352, 4, 1) == 0
    assert h.mri_siren_gradient_supported(9, 64, 4, 1) == 0
    assert h.mri_siren_gradient_supported(3, 64, 4, 2) == 0
    assert h.mri_siren_gradient_supported(0, 64, 4, 1) == 0
    assert h.mri_siren_gradient_supported(3, 64, lib.MAX_SIREN_LAYERS + 1, 1) == 0
    assert h.mri_siren_gradient_workspace_bytes(96, 3) == -1
    # the optional shapes: _supported is the truth, and the workspace follows it
    for dim_in, hidden, n_sine in ((3, 32, 3), (3, 64, 1), (4, 64, 3)):
        if h.mri_siren_gradient_supported(dim_in, hidden, n_sine, 1):
            assert h.mri_siren_gradient_workspace_bytes(hidden, n_sine) == h.mri_siren_forward_workspace_bytes(hidden, n_sine)


def _call(h, x=64, weight=None, bias=None, y=64, dydx=64, ws=256, ws_bytes=1 << 30, n=8, dim_in=3, hidden=64, n_sine=3):
    """mri_siren_gradient with fake (never dereferenced) device addresses; `weight` / `bias` default to real HOST
    arrays of fake device pointers.  Every call here is refused before anything is launched or read."""
    arr = (C.c_void_p * (lib_max + 1))(*[256] * (lib_max + 1))
    weight = arr if weight is None else weight
    bias = arr if bias is None else bias
    p = lambda v: None if v is None else C.c_void_p(v)  # noqa: E731
    wp = weight if not isinstance(weight, int) else None
    bp = bias if not isinstance(bias, int) else None
    return h.mri_siren_gradient(p(x), n, dim_in, hidden, n_sine, wp, bp, 30.0, 30.0, p(y), p(dydx), p(ws), ws_bytes, None)


lib_max = 8  # MRI_SIREN_MAX_LAYERS


def test_argument_validation_without_a_device(lib):
    h = lib.load()
    assert lib.MAX_SIREN_LAYERS == lib_max
    err = lambda: h.mri_last_error().decode()  # noqa: E731
    # an empty batch is a no-op and touches no device
    assert h.mri_siren_gradient(None, 0, 3, 64, 3, None, None, 30.0, 30.0, None, None, None, 0, None) == 0
    # every NULL buffer, the way tests/test_abi.py calls the other entry points
    assert h.mri_siren_gradient(None, 8, 3, 256, 5, None, None, 30.0, 30.0, None, None, None, 0, None) == INVALID
    assert err()
    for name, kw in (("x", dict(x=None)), ("weight", dict(weight=0)), ("bias", dict(bias=0)), ("y", dict(y=None)),
                     ("dydx", dict(dydx=None)), ("workspace", dict(ws=None))):
        assert _call(h, **kw) == INVALID, name
        assert name in err(), (name, err())
    null_layer = (C.c_void_p * (lib_max + 1))(*([256] * 2 + [None] + [256] * (lib_max - 2)))
    assert _call(h, weight=null_layer) == INVALID and "weight[2]" in err(), err()
    assert _call(h, bias=null_layer) == INVALID and "bias[2]" in err(), err()
    # a misaligned or short workspace
    assert _call(h, ws=256 + 4) == INVALID and "workspace" in err() and "16-byte" in err(), err()
    assert _call(h, ws_bytes=h.mri_siren_gradient_workspace_bytes(64, 3) - 1) == INVALID and "workspace" in err()
    # x, y, dydx: any 4-byte aligned address, nothing coarser
    for name in ("x", "y", "dydx"):
        assert _call(h, **{name: 64 + 2}) == INVALID and name in err() and "4-byte" in err(), (name, err())
    # unsupported shapes name the argument
    assert _call(h, hidden=352) == INVALID and "hidden" in err(), err()
    assert _call(h, hidden=96) == INVALID and "hidden" in err(), err()
    assert _call(h, dim_in=9) == INVALID and "dim_in" in err(), err()
    assert _call(h, dim_in=0) == INVALID and "dim_in" in err(), err()
    assert _call(h, n_sine=lib_max + 1) == INVALID and "n_sine_layers" in err(), err()
    assert _call(h, n=-1) == INVALID and "out of range" in err(), err()


def test_ops_reject_cpu_tensors(lib):
    from mri_interpolation_amd import ops
    w = [torch.zeros(64, 3), torch.zeros(64, 64), torch.zeros(1, 64)]
    b = [torch.zeros(64), torch.zeros(64), torch.zeros(1)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.siren_gradient(torch.zeros(4, 3), w, b, 30.0, 30.0)


# ------------------------------------------------------------------------------------------------ voxel scale
def test_voxel_scale_values():
    import launcher
    assert launcher.gradient_voxel_scale((5, 3, 1), norm_siren=True) == (2.0 / 4, 2.0 / 2, 0.0)
    assert launcher.gradient_voxel_scale((5, 3, 1), norm_siren=False) == (1.0 / 4, 1.0 / 2, 0.0)
    assert launcher.gradient_voxel_scale((352, 352, 6, 15)) == (2.0 / 351, 2.0 / 351, 2.0 / 5, 2.0 / 14)
    assert launcher.gradient_voxel_scale((2,), norm_siren=False) == (1.0,)


@pytest.mark.parametrize("norm_siren", [True, False])
def test_voxel_scale_turns_the_analytic_gradient_of_a_ramp_into_np_gradient(norm_siren):
    """f(x) = a . x + c sampled on the loader's grid: df/dx_d = a_d everywhere, and a_d times the scale is the
    difference between neighbouring voxels, which is what np.gradient returns on a linear ramp (edges included)."""
    import launcher
    shape, a = (7, 5, 3, 1), np.array([0.75, -1.5, 2.25, 4.0])
    # the loader's grid, linspace(lo, 1, s) per axis, in float64 (the float32 grid is it rounded to 6e-8)
    axes = [np.linspace(-1.0 if norm_siren else 0.0, 1.0, s) for s in shape]
    coords = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, len(shape))
    ramp = (coords @ a + 0.3).reshape(shape)
    scaled = a * np.asarray(launcher.gradient_voxel_scale(shape, norm_siren))
    for d, s in enumerate(shape):
        if s == 1:
            assert scaled[d] == 0.0
            continue
        np.testing.assert_allclose(np.gradient(ramp, axis=d), np.full(shape, scaled[d]), rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------------------------ launcher, CPU path
def test_launcher_save_gradient_on_the_cpu_path(tmp_path, monkeypatch):
    """Plumbing, not numerics: gradient.nii.gz has the shape and the unit the flag promises, and its values are the
    derivative of what pred.nii.gz holds (central differences of cpu_path.predict at +-1e-3 in coordinates)."""
    import launcher
    from mri_interpolation_amd import _lib, checkpoint, cpu_path, models, nifti
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the CPU mode must not load the library")))
    out = str(tmp_path / "run")
    launcher.main(["--accelerator", "cpu", "--model_class", "SirenNet", "--synthetic", "8,8,4", "--save_gradient",
                   "--max_steps", "2", "--out_dir", out, "--log_every", "0"])
    assert os.path.exists(os.path.join(out, "pred.nii.gz"))
    grad = nifti.load(os.path.join(out, "gradient.nii.gz"))
    assert grad.shape == (8, 8, 4, 3) and grad.dtype == np.float32 and np.isfinite(grad).all()
    assert nifti.read_header(os.path.join(out, "gradient.nii.gz"))["datatype"] == 16  # NIfTI float32
    ckpt, = os.listdir(os.path.join(out, "checkpoints"))
    net = models.SirenNet(dim_in=3, dim_hidden=128, dim_out=1, n_layers=6)  # BaseConfig's defaults
    checkpoint.load(os.path.join(out, "checkpoints", ckpt), net)
    coords = cpu_path.grid_coords((8, 8, 4), norm_siren=True).double()
    net = net.double()
    h, fd = 1e-3, []
    for d in range(3):
        e = torch.zeros(3, dtype=torch.float64)
        e[d] = h
        fd.append((cpu_path.predict(net, coords + e, 4096) - cpu_path.predict(net, coords - e, 4096)) / (2 * h))
    fd = torch.cat(fd, dim=1).numpy() * np.asarray(launcher.gradient_voxel_scale((8, 8, 4), True))
    fd = fd.reshape(8, 8, 4, 3)
    assert np.abs(fd).max() > 0
    assert np.abs(grad - fd).max() <= 1e-2 * np.abs(fd).max()
    # and it is the derivative of the prediction the run saved
    pred = nifti.load(os.path.join(out, "pred.nii.gz"))
    np.testing.assert_allclose(pred, cpu_path.predict(net, coords, 4096).reshape(8, 8, 4).numpy(), atol=1e-5)


def test_cpu_path_gradient_is_per_row():
    from mri_interpolation_amd import cpu_path, models
    torch.manual_seed(3)
    net = models.SirenNet(dim_in=2, dim_hidden=32, dim_out=1, n_layers=2)
    x = cpu_path.grid_coords((5, 4))
    y, g = cpu_path.predict_with_gradient(net, x, 7)  # batches of 7, 7, 6
    assert y.shape == (20, 1) and g.shape == (20, 2) and not y.requires_grad and not g.requires_grad
    assert torch.equal(y, cpu_path.predict(net, x, 7))
    one = torch.cat([cpu_path.predict_with_gradient(net, x[i:i + 1], 1)[1] for i in range(20)])
    assert torch.allclose(g, one, rtol=1e-5, atol=1e-6)
    assert all(p.grad is None for p in net.parameters())


# ------------------------------------------------------------------------------------------------ model selection
def test_save_gradient_parses_and_hashmlp_selects_the_generic_body():
    import launcher
    from mri_interpolation_amd import models
    args = launcher.parse_args(["--model_class", "HashMLP", "--save_gradient"])
    assert args.save_gradient is True and launcher.parse_args(["--model_class", "HashMLP"]).save_gradient is False
    generic = models.BaseMLP.forward_with_gradient
    assert models.HashMLP.forward_with_gradient is generic
    assert models.ModulatedSirenNet.forward_with_gradient is not models.SirenNet.forward_with_gradient
    assert models.PsfSirenNet.forward_with_gradient is models.SirenNet.forward_with_gradient
    launcher.check_save_gradient(models.HashMLP, 1)  # passes: nothing raised
    launcher.check_save_gradient(models.SirenNet, 1)
    with pytest.raises(SystemExit, match="one output"):
        launcher.check_save_gradient(models.SirenNet, 2)

    class NoGradient:
        pass
    with pytest.raises(SystemExit, match="forward_with_gradient"):
        launcher.check_save_gradient(NoGradient, 1)


def test_dispatch_with_a_fake_ops(monkeypatch):
    """Which body each class takes, seen through a recording stand-in for the kernel call: SirenNet on CPU tensors and
    ModulatedSirenNet anywhere never reach it; dim_out != 1 raises."""
    from mri_interpolation_amd import models, ops
    calls = []
    monkeypatch.setattr(ops, "siren_gradient", lambda *a, **k: calls.append("kernel"))
    generic = []
    monkeypatch.setattr(models.BaseMLP, "forward_with_gradient", lambda self, x: generic.append(type(self).__name__))
    x = torch.zeros(4, 3)
    models.SirenNet(3, 64, 1, 3).forward_with_gradient(x)              # a CPU tensor: generic
    models.ModulatedSirenNet(3, 64, 1, 3).forward_with_gradient(x)     # another forward: generic
    assert calls == [] and generic == ["SirenNet", "ModulatedSirenNet"]
    with pytest.raises(ValueError, match="dim_out"):
        models.SirenNet(3, 64, 2, 3).forward_with_gradient(x)
    monkeypatch.undo()
    with pytest.raises(ValueError, match="dim_out"):
        models.BaseMLP(3, 2, 16, 2).forward_with_gradient(x)
