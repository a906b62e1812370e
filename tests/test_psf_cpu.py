"""PsfSirenNet (reference models.py:397-539) without a GPU: constructor surface, the PSF tables against
the reference's, the k < dim_in layout, the launcher's default spacing, a checkpoint round trip and the
argument checks of the four PSF entry points of the C ABI."""
import inspect

import numpy as np
import pytest
import torch

from conftest import load_golden

SAMPLE_SPACING = (1.0 / 351.0, 1.0 / 351.0, 1.0 / 5.0)


@pytest.fixture(scope="module")
def models():
    from mri_interpolation_amd import models
    return models


def test_constructor_signature_matches_the_reference(models):
    params = inspect.signature(models.PsfSirenNet.__init__).parameters
    want = dict(dim_in=3, dim_hidden=64, dim_out=1, n_layers=4, w0=30.0, w0_initial=30.0, use_bias=True,
                final_activation=None, lr=1e-4, coordinates_spacing=None, n_sample=5)
    assert list(params)[1:] == list(want)
    assert {k: params[k].default for k in want} == want
    import mri_interpolation_amd
    assert mri_interpolation_amd.PsfSirenNet is models.PsfSirenNet
    assert issubclass(models.PsfSirenNet, models.SirenNet)


@pytest.mark.parametrize("name", ["psf_siren_3d_4x64_ns5", "psf_siren_3d_6x128_ns3"])
def test_state_dict_keys_and_tables_match_the_golden(models, name):
    fx = load_golden(name)
    m = fx.meta
    net = models.PsfSirenNet(dim_in=3, dim_hidden=m["dim_hidden"], n_layers=m["n_layers"],
                             coordinates_spacing=tuple(m["coordinates_spacing"]), n_sample=m["n_sample"])
    assert list(net.state_dict()) == m["state_dict_keys"]
    assert np.array_equal(net.psf_coordinates.numpy(), fx["psf_coordinates"])
    assert np.array_equal(net.psf_conv.weight.detach().numpy(), fx["psf_weight"])
    assert not net.psf_conv.weight.requires_grad
    assert net.n_psf == m["n_sample"] ** 3


@pytest.mark.parametrize("n_sample", [1, 3, 5])
def test_psf_tables_bit_equal_to_the_reference(models, n_sample):
    fx = load_golden("psf_tables")
    net = models.PsfSirenNet(coordinates_spacing=SAMPLE_SPACING, n_sample=n_sample)
    assert np.array_equal(net.psf_coordinates.numpy(), fx[f"coords_{n_sample}"])
    assert np.array_equal(net.psf_conv.weight.detach().numpy(), fx[f"weight_{n_sample}"])
    if n_sample == 1:  # linspace(a, b, 1) == [a]: offset -s, weight 1
        assert np.array_equal(net.psf_coordinates.numpy(), -np.array([SAMPLE_SPACING], dtype=np.float32))
        assert net.psf_conv.weight.item() == 1.0


def test_missing_spacing_raises(models):
    with pytest.raises(ValueError, match="No PSF spacing defined"):
        models.PsfSirenNet()
    with pytest.raises(ValueError, match="dim_out"):
        models.PsfSirenNet(dim_out=2, coordinates_spacing=SAMPLE_SPACING)
    with pytest.raises(ValueError, match="coordinates_spacing"):
        models.PsfSirenNet(dim_in=2, coordinates_spacing=SAMPLE_SPACING)


def test_fewer_psf_axes_than_input_axes(models):
    net = models.PsfSirenNet(dim_in=4, coordinates_spacing=(0.1, 0.25), n_sample=3)
    off = net.psf_coordinates.numpy()
    assert off.shape == (9, 4)
    assert (off[:, 2:] == 0).all()
    # ij order, the last PSF axis fastest
    lin = torch.linspace(-0.1, 0.1, 3).numpy(), torch.linspace(-0.25, 0.25, 3).numpy()
    assert np.array_equal(off[:, 0], np.repeat(lin[0], 3)) and np.array_equal(off[:, 1], np.tile(lin[1], 3))
    w = net.psf_conv.weight.detach().reshape(3, 3).numpy().astype(np.float64)
    assert abs(w.sum() - 1.0) < 1e-6
    assert np.allclose(w, np.outer(w.sum(1), w.sum(0)), rtol=1e-6)  # a product of two Gaussians
    one = models.PsfSirenNet(dim_in=2, coordinates_spacing=(0.5,), n_sample=5)
    assert one.n_psf == 5 and (one.psf_coordinates[:, 1] == 0).all()


def test_optimizer_leaves_the_psf_weight_out(models):
    net = models.PsfSirenNet(coordinates_spacing=SAMPLE_SPACING, n_sample=3)
    opt = net.configure_optimizers()
    assert all(p is not net.psf_conv.weight for p in opt._params)
    assert len(opt._params) == len(list(net.parameters())) - 1


def test_launcher_spacing_is_half_the_pitch():
    import launcher
    assert launcher.psf_spacing((352, 352, 6), 3, norm_siren=True) == (1 / 351, 1 / 351, 1 / 5)
    assert launcher.psf_spacing((352, 352, 6), 3, norm_siren=False) == (0.5 / 351, 0.5 / 351, 0.5 / 5)
    assert launcher.psf_spacing((32, 1, 8, 15), 3, norm_siren=True) == (1 / 31, 0.0, 1 / 7)
    assert launcher.psf_spacing((352, 352), 2) == (1 / 351, 1 / 351)
    from mri_interpolation_amd import config as cfg, models
    c = cfg.BaseConfig()
    c.model_class, c.n_sample, c.norm_siren = "PsfSirenNet", 3, True
    c.resolve((32, 32, 8))
    c.dim_hidden, c.n_layers = 64, 3
    net = launcher.build_model(c, models)
    assert isinstance(net, models.PsfSirenNet) and net.n_psf == 27
    assert net.coordinates_spacing == (1 / 31, 1 / 31, 1 / 7)


def test_checkpoint_round_trip_keeps_the_psf_weight(models, tmp_path):
    from mri_interpolation_amd import checkpoint
    net = models.PsfSirenNet(dim_in=3, dim_hidden=32, n_layers=2, coordinates_spacing=SAMPLE_SPACING,
                             n_sample=3)
    w = net.psf_conv.weight.detach().clone()
    path = str(tmp_path / "psf.ckpt")
    ckpt = checkpoint.save(path, net, epoch=0, global_step=1)
    assert torch.equal(ckpt["state_dict"]["psf_conv.weight"], w)
    other = models.PsfSirenNet(dim_in=3, dim_hidden=32, n_layers=2, coordinates_spacing=SAMPLE_SPACING,
                               n_sample=3)
    with torch.no_grad():
        other.psf_conv.weight.zero_()
    checkpoint.load(path, other)
    assert torch.equal(other.psf_conv.weight, w)
    for k, v in net.state_dict().items():
        assert torch.equal(other.state_dict()[k], v), k


def test_psf_entry_points_reject_bad_arguments_without_hip():
    from mri_interpolation_amd import _lib
    from mri_interpolation_amd.build import build
    build()
    h = _lib.load()
    fake = 4096  # never dereferenced: every call below fails its checks first
    bad = {
        "mri_psf_expand": [(None, 8, 3, None, 27, None, None),        # NULL buffers
                           (fake, 8, 3, fake, 0, fake, None),         # S = 0
                           (fake, 8, 3, fake, 4097, fake, None),      # S > 4096
                           (fake, 8, 9, fake, 27, fake, None)],       # dim_in > 8
        "mri_psf_reduce": [(None, 8, 27, 1, None, None, None),
                           (fake, 8, 0, 1, fake, fake, None),
                           (fake, 8, 4097, 1, fake, fake, None),
                           (fake, 8, 27, 0, fake, fake, None)],
        "mri_psf_broadcast": [(None, 8, 27, None, 1.0, None, None),
                              (fake, 8, 0, fake, 1.0, fake, None),
                              (fake, 8, 4097, fake, 1.0, fake, None)],
        "mri_psf_mse_loss": [(None, None, 8, 8, 27, None, 1.0, None, None, None, None),
                             (fake, fake, 8, 8, 0, fake, 1.0, fake, fake, fake, None),
                             (fake, fake, 8, 8, 4097, fake, 1.0, fake, fake, fake, None),
                             (fake, fake, 9, 8, 27, fake, 1.0, fake, fake, fake, None),   # n > n_total
                             (fake, fake, 8, 8, 27, fake, 0.0, fake, fake, fake, None)],  # divisor
    }
    for name, calls in bad.items():
        for args in calls:
            assert len(args) == len(_lib.SIGNATURES[name]), name
            assert getattr(h, name)(*args) == -1, (name, args)
            assert h.mri_last_error().decode(), name
    # empty batches are a no-op
    assert h.mri_psf_expand(None, 0, 3, None, 27, None, None) == 0
    assert h.mri_psf_mse_loss(None, None, 0, 0, 27, None, 1.0, None, None, None, None) == 0
