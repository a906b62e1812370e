"""The SIREN coordinate gradient for 4-D volumes without a device: the C ABI's new range (dim_in = 4, the eight-slot
form of csrc/siren_gradient.hip), `launcher.py --save_gradient` on a 4-D volume on the CPU path (a 5-D NIfTI), and the
gradient volumes on the interpolation grids (`gradient_interpolation{shape}.nii.gz`).  CPU only."""
import ctypes as C
import dataclasses
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
def test_four_axes_are_supported_and_five_are_not(lib):
    h = lib.load()
    for hidden in (32, 64, 128, 256):
        for n_sine in (1, 3, lib.MAX_SIREN_LAYERS):
            assert h.mri_siren_gradient_supported(4, hidden, n_sine, 1) == 1, (hidden, n_sine)
    assert h.mri_siren_gradient_supported(5, 64, 3, 1) == 0
    assert h.mri_siren_gradient_supported(0, 64, 3, 1) == 0
    # what the four-slot form refuses stays refused with four axes
    assert h.mri_siren_gradient_supported(4, 352, 3, 1) == 0
    assert h.mri_siren_gradient_supported(4, 64, 3, 2) == 0
    assert h.mri_siren_gradient_supported(4, 64, lib.MAX_SIREN_LAYERS + 1, 1) == 0
    assert h.mri_siren_gradient_supported(4, 64, 0, 1) == 0


def test_workspace_is_unchanged(lib):
    """The workspace holds the split hidden x hidden weights: it depends on neither dim_in nor the slot count."""
    h = lib.load()
    for hidden in (32, 64, 128, 256):
        assert h.mri_siren_gradient_workspace_bytes(hidden, 1) == 0
        for n_sine in (2, 3, lib.MAX_SIREN_LAYERS):
            assert h.mri_siren_gradient_workspace_bytes(hidden, n_sine) == \
                h.mri_siren_forward_workspace_bytes(hidden, n_sine) > 0
    assert h.mri_siren_gradient_workspace_bytes(96, 3) == -1
    assert h.mri_siren_gradient_workspace_bytes(64, lib.MAX_SIREN_LAYERS + 1) == -1


def test_five_axes_are_refused_by_name_before_any_device_call(lib):
    h = lib.load()
    n_ptr = lib.MAX_SIREN_LAYERS + 1
    arr = (C.c_void_p * n_ptr)(*[256] * n_ptr)  # fake device addresses, never dereferenced
    p = C.c_void_p
    for dim_in in (5, 0):
        rc = h.mri_siren_gradient(p(64), 8, dim_in, 64, 3, arr, arr, 30.0, 30.0, p(64), p(64), p(256), 1 << 30, None)
        err = h.mri_last_error().decode()
        assert rc == INVALID and "dim_in" in err and "1 .. 4" in err, err


# ------------------------------------------------------------------------------------------------ launcher, CPU path
def run_cpu_launcher(tmp_path, monkeypatch, synthetic, extra=(), interp_shapes=()):
    import launcher
    from mri_interpolation_amd import _lib, config as cfg
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the CPU mode must not load the library")))
    base = cfg.BaseConfig
    monkeypatch.setattr(cfg, "BaseConfig", lambda: dataclasses.replace(base(), interp_shapes=[tuple(s) for s in interp_shapes]))
    out = str(tmp_path / "run")
    launcher.main(["--accelerator", "cpu", "--model_class", "SirenNet", "--synthetic", synthetic, "--dim_hidden", "32",
                   "--n_layers", "3", "--batch_size", "100", "--max_steps", "2", "--out_dir", out, "--log_every", "0",
                   *extra])
    return out


def trained_net(out, dim_in):
    from mri_interpolation_amd import checkpoint, models
    ckpt, = os.listdir(os.path.join(out, "checkpoints"))
    net = models.SirenNet(dim_in=dim_in, dim_hidden=32, dim_out=1, n_layers=3)
    checkpoint.load(os.path.join(out, "checkpoints", ckpt), net)
    return net


def test_launcher_save_gradient_on_a_4d_volume_on_the_cpu_path(tmp_path, monkeypatch):
    """gradient.nii.gz of a 4-D volume is a 5-D NIfTI, image_shape + (4,), float32: cpu_path.predict_with_gradient of
    the saved network in the launcher's batches, times the voxel scale (the temporal derivative in the last column)."""
    import launcher
    from mri_interpolation_amd import cpu_path, nifti
    shape = (6, 5, 4, 3)
    out = run_cpu_launcher(tmp_path, monkeypatch, "6,5,4,3", ["--save_gradient"])
    path = os.path.join(out, "gradient.nii.gz")
    grad = nifti.load(path)
    assert grad.shape == shape + (4,) and grad.dtype == np.float32 and np.isfinite(grad).all()
    assert nifti.read_header(path)["datatype"] == 16  # NIfTI float32
    assert nifti.load(os.path.join(out, "pred.nii.gz")).shape == shape
    net = trained_net(out, 4)
    _, g = cpu_path.predict_with_gradient(net, cpu_path.grid_coords(shape, norm_siren=True), 100)
    scale = np.asarray(launcher.gradient_voxel_scale(shape, True), dtype=np.float32)
    assert tuple(scale) == (np.float32(2 / 5), np.float32(2 / 4), np.float32(2 / 3), np.float32(2 / 2))
    want = (g.numpy().astype(np.float32) * scale).reshape(shape + (4,))
    assert np.abs(want[..., 3]).max() > 0
    assert np.array_equal(grad, want)
    assert not [f for f in os.listdir(out) if f.startswith("gradient_interpolation")]


@pytest.mark.parametrize("save_gradient", [True, False], ids=["save_gradient", "plain"])
def test_interpolation_grid_gradient_on_the_cpu_path(tmp_path, monkeypatch, save_gradient):
    """With --save_gradient every interpolation{shape}.nii.gz gets a gradient_interpolation{shape}.nii.gz beside it,
    shape + (dim_in,), in voxel steps of THAT grid; without the flag nothing new is written."""
    import launcher
    from mri_interpolation_amd import cpu_path, nifti
    shape, grid = (6, 5, 4), (9, 7, 5)
    out = run_cpu_launcher(tmp_path, monkeypatch, "6,5,4", ["--save_gradient"] if save_gradient else [], [grid, (4, 4)])
    interp = nifti.load(os.path.join(out, f"interpolation{grid}.nii.gz"))
    assert interp.shape == grid
    assert not os.path.exists(os.path.join(out, "interpolation(4, 4).nii.gz"))  # (a 2-D shape on a 3-D volume is skipped)
    assert not os.path.exists(os.path.join(out, "gradient_interpolation(4, 4).nii.gz"))
    path = os.path.join(out, f"gradient_interpolation{grid}.nii.gz")
    if not save_gradient:
        assert not os.path.exists(path) and not os.path.exists(os.path.join(out, "gradient.nii.gz"))
        return
    grad = nifti.load(path)
    assert grad.shape == grid + (3,) and grad.dtype == np.float32 and np.isfinite(grad).all()
    net = trained_net(out, 3)
    y, g = cpu_path.predict_with_gradient(net, cpu_path.grid_coords(grid, norm_siren=True), 100)
    scale = np.asarray(launcher.gradient_voxel_scale(grid, True), dtype=np.float32)
    assert tuple(scale) == (np.float32(2 / 8), np.float32(2 / 6), np.float32(2 / 4))
    want = (g.numpy().astype(np.float32) * scale).reshape(grid + (3,))
    assert np.abs(want).max() > 0
    assert np.array_equal(grad, want)
    assert np.array_equal(interp, y.numpy().reshape(grid))
    # the volume's own gradient is still there, on its own grid and in its own voxel steps
    own = nifti.load(os.path.join(out, "gradient.nii.gz"))
    _, g0 = cpu_path.predict_with_gradient(net, cpu_path.grid_coords(shape, norm_siren=True), 100)
    own_scale = np.asarray(launcher.gradient_voxel_scale(shape, True), dtype=np.float32)
    assert np.array_equal(own, (g0.numpy().astype(np.float32) * own_scale).reshape(shape + (3,)))


def test_save_gradient_volume_defaults_write_gradient_nii(tmp_path):
    """The shape and file name arguments default to the volume's own: the call the launcher made before them."""
    import launcher
    from mri_interpolation_amd import config as cfg, nifti
    config = cfg.BaseConfig().resolve((3, 2, 2, 2))
    config.norm_siren = True
    dydx = torch.arange(24 * 4, dtype=torch.float32).reshape(24, 4)
    got = launcher.save_gradient_volume(dydx, config, str(tmp_path), nifti)
    assert os.listdir(str(tmp_path)) == ["gradient.nii.gz"]
    want = (dydx.numpy() * np.asarray([1.0, 2.0, 2.0, 2.0], dtype=np.float32)).reshape(3, 2, 2, 2, 4)
    assert np.array_equal(got, want) and np.array_equal(nifti.load(str(tmp_path / "gradient.nii.gz")), want)
    other = launcher.save_gradient_volume(dydx, config, str(tmp_path), nifti, shape=(2, 3, 2, 2), name="g.nii.gz")
    assert other.shape == (2, 3, 2, 2, 4) and nifti.load(str(tmp_path / "g.nii.gz")).shape == (2, 3, 2, 2, 4)
    assert np.array_equal(other.reshape(24, 4), dydx.numpy() * np.asarray([2.0, 1.0, 2.0, 2.0], dtype=np.float32))
