"""Checkpoints in Lightning's layout (mri_interpolation_amd/checkpoint.py): what the reference's
`model_cls.load_from_checkpoint` (reference launcher.py:97-117, strict) needs to be in the file, a round trip
of parameters, Adam moments and step count, and a strict load into the reference's own classes and optimiser
(their keys, shapes, parameter order and Adam as tests/golden/reference_checkpoint.npz captured them)."""
import pytest
import torch

from conftest import load_golden

from mri_interpolation_amd import checkpoint, models


def _hash():
    torch.manual_seed(5)
    return models.HashMLP(dim_in=3, n_levels=3, n_features_per_level=2, log2_hashmap_size=9,
                          base_resolution=4, finest_resolution=32, dim_hidden=16, dim_out=1, n_layers=2, lr=5e-3)


def _siren():
    torch.manual_seed(6)
    return models.SirenNet(dim_in=3, dim_hidden=16, dim_out=1, n_layers=3, lr=1e-4)


def _fake_moments(model, seed):
    g = torch.Generator().manual_seed(seed)
    sd = model.state_dict()
    buffers = {n for n, _ in model.named_buffers()}
    return {k: (torch.randn(v.shape, generator=g), torch.rand(v.shape, generator=g))
            for k, v in sd.items() if k not in buffers and v.dtype == torch.float32}


class _CpuAdam:
    """The attributes checkpoint.load() touches of optim.Adam, over CPU tensors (the real one is GPU-only)."""

    def __init__(self, model):
        self.betas, self.eps, self.step_count = (0.9, 0.999), 1e-8, 0
        self.param_groups = [dict(lr=model.lr)]
        params = list(model.parameters())
        offsets, total = [], 0
        for p in params:
            offsets.append(total)
            total += (p.numel() + 3) // 4 * 4
        self.flat = type("Flat", (), dict(params=params, offsets=offsets, exp_avg=torch.zeros(total),
                                          exp_avg_sq=torch.zeros(total)))()

    def flatten(self):
        return self.flat


@pytest.mark.parametrize("build", [_hash, _siren])
def test_layout_and_round_trip(tmp_path, build):
    model = build()
    moments = _fake_moments(model, 11)
    ckpt = checkpoint.lightning_checkpoint(model, epoch=3, global_step=40, moments=moments, step=40)
    # what Lightning's loader indexes unconditionally, and what Trainer.fit(ckpt_path=) restores
    for key in ("pytorch-lightning_version", "state_dict", "optimizer_states", "lr_schedulers", "epoch", "global_step"):
        assert key in ckpt, key
    assert isinstance(ckpt["pytorch-lightning_version"], str) and ckpt["epoch"] == 3 and ckpt["global_step"] == 40
    sd = ckpt["state_dict"]
    if build is _hash:  # the reference's dead BaseMLP stack: Linear(2,128), Linear(128,1)
        assert list(sd)[:4] == ["layers.0.weight", "layers.0.bias", "layers.2.weight", "layers.2.bias"]
        assert sd["layers.0.weight"].shape == (128, 2) and sd["layers.2.weight"].shape == (1, 128)
        assert "encoder.levels.2.embedding.weight" in sd and "decoder.1.1.running_var" in sd
    opt = ckpt["optimizer_states"][0]
    names = checkpoint._reference_parameter_names(model)
    assert opt["param_groups"][0]["params"] == list(range(len(names)))
    assert set(opt["state"]) == {i for i, n in enumerate(names) if not n.startswith("layers.") or build is _siren}
    path = str(tmp_path / "epoch=3-step=40.ckpt")
    torch.save(ckpt, path)
    # a fresh model and optimiser resume from it: parameters, moments, step count
    fresh = build()
    with torch.no_grad():
        for p in fresh.parameters():
            p.add_(1.0)
    adam = _CpuAdam(fresh)
    checkpoint.load(path, fresh, adam, resume_optimizer=True)
    for (k, a), (_, b) in zip(model.state_dict().items(), fresh.state_dict().items()):
        assert torch.equal(a, b), k
    assert adam.step_count == 40 and adam.param_groups[0]["lr"] == model.lr
    got = {}
    for p, off in zip(adam.flat.params, adam.flat.offsets):
        got[id(p)] = (adam.flat.exp_avg[off:off + p.numel()].view(p.shape), adam.flat.exp_avg_sq[off:off + p.numel()].view(p.shape))
    for name, p in fresh.named_parameters():
        m, v = got[id(p)]
        if name.endswith("encoder.table"):
            for l in range(fresh.encoder.n_levels):
                lo, hi = fresh.encoder._row_span(l)
                want = moments[f"encoder.levels.{l}.embedding.weight"]
                assert torch.equal(m[lo:hi], want[0]) and torch.equal(v[lo:hi], want[1])
        else:
            assert torch.equal(m, moments[name][0]) and torch.equal(v, moments[name][1]), name


def _reference_stand_in(entry):
    """A module with exactly the state-dict keys, shapes and parameter order of the reference's module
    (tests/golden/reference_checkpoint.npz, captured from the reference classes by make_golden.py): what
    `load_state_dict(strict=True)` and the optimiser's `load_state_dict` check of the reference module."""
    root = torch.nn.Module()
    params = set(entry["param_names"])
    for key, shape in entry["state"]:
        *path, leaf = key.split(".")
        mod = root
        for part in path:
            if part not in mod._modules:
                mod.add_module(part, torch.nn.Module())
            mod = mod._modules[part]
        if key in params:
            mod.register_parameter(leaf, torch.nn.Parameter(torch.zeros(shape)))
        else:
            mod.register_buffer(leaf, torch.zeros(shape, dtype=torch.int64 if leaf == "num_batches_tracked"
                                                  else torch.float32))
    assert [n for n, _ in root.named_parameters()] == entry["param_names"]
    return root


@pytest.mark.parametrize("kind", ["hash", "siren"])
def test_reference_classes_load_the_checkpoint_strictly(tmp_path, kind):
    """The file goes through `load_state_dict(strict=True)` of the reference's own HashMLP / SirenNet (what
    `load_from_checkpoint` does after Lightning's migration step) and its optimizer state through the
    reference's `configure_optimizers()` Adam -- both as the fixture captured them from the reference classes."""
    fx = load_golden("reference_checkpoint")
    entry = fx.meta[kind]
    if kind == "hash":
        model = _hash()
    else:
        model = _siren()
        # the parameters the reference's forward was evaluated on (a reference-layout state dict)
        sd = {k: torch.from_numpy(fx[f"siren_sd_{i}"]) for i, (k, _) in enumerate(entry["state"])}
        model.load_state_dict(sd)
    ref = _reference_stand_in(entry)
    moments = _fake_moments(model, 12)
    path = str(tmp_path / "c.ckpt")
    torch.save(checkpoint.lightning_checkpoint(model, epoch=0, global_step=9, moments=moments, step=9), path)
    ckpt = torch.load(path, weights_only=True)
    result = ref.load_state_dict(ckpt["state_dict"], strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    if kind == "siren":
        x = torch.from_numpy(fx["siren_x"])
        for k, v in sd.items():
            assert torch.equal(ckpt["state_dict"][k], v), k
        with torch.no_grad():  # same parameters: the reference's forward on them is the oracle's
            from oracle import mlp as omlp
            sdict = dict(ref.named_parameters())
            params = [(sdict[w], sdict[b]) for w, b in entry["forward_layers"]]
            want = omlp.siren_forward(x, [(w.detach(), b.detach()) for w, b in params])
            assert torch.allclose(torch.from_numpy(fx["siren_y"]), want, atol=1e-6)
    o = entry["optimizer"]
    opt = getattr(torch.optim, o["cls"])(ref.parameters(), lr=o["lr"], betas=tuple(o["betas"]), eps=o["eps"],
                                         weight_decay=o["weight_decay"], amsgrad=o["amsgrad"])
    opt.load_state_dict(ckpt["optimizer_states"][0])
    ref_params = list(ref.parameters())
    names = [n for n, _ in ref.named_parameters()]
    assert names == checkpoint._reference_parameter_names(model)
    for i, p in enumerate(ref_params):
        st = opt.state.get(p)
        if names[i].startswith("layers.") and kind == "hash":
            assert not st  # the dead stack never had a gradient
            continue
        assert st["exp_avg"].shape == p.shape and float(st["step"]) == 9.0
        assert torch.equal(st["exp_avg"], moments[names[i]][0])


def test_default_resume_is_the_references_weights_only_with_a_fresh_adam(tmp_path):
    """Reference launcher.py:97-165: `load_from_checkpoint(path, ..., lr=config.lr)` then `trainer.fit(model,
    loader)` with no ckpt_path -- the weights come back, Adam starts at step 0 with zero moments at the
    COMMAND LINE's learning rate.  `resume_optimizer=True` is Lightning's fit(ckpt_path=): moments and step
    count too, still at the configured lr unless `restore_lr=True`."""
    model = _hash()
    moments = _fake_moments(model, 5)
    path = str(tmp_path / "c.ckpt")
    torch.save(checkpoint.lightning_checkpoint(model, epoch=0, global_step=7, moments=moments, step=7), path)
    assert torch.load(path, weights_only=True)["optimizer_states"][0]["param_groups"][0]["lr"] == model.lr

    def fresh_pair(lr):
        fresh = _hash()
        with torch.no_grad():
            for p in fresh.parameters():
                p.add_(1.0)
        adam = _CpuAdam(fresh)
        adam.param_groups[0]["lr"] = lr  # what `--lr` configured
        return fresh, adam

    fresh, adam = fresh_pair(1e-2)
    checkpoint.load(path, fresh, adam)  # the default
    for (k, a), (_, b) in zip(model.state_dict().items(), fresh.state_dict().items()):
        assert torch.equal(a, b), k
    assert adam.step_count == 0 and adam.param_groups[0]["lr"] == 1e-2
    assert not adam.flat.exp_avg.any() and not adam.flat.exp_avg_sq.any()

    fresh, adam = fresh_pair(1e-2)
    checkpoint.load(path, fresh, adam, resume_optimizer=True)
    assert adam.step_count == 7 and adam.param_groups[0]["lr"] == 1e-2 and adam.flat.exp_avg.any()

    fresh, adam = fresh_pair(1e-2)
    checkpoint.load(path, fresh, adam, resume_optimizer=True, restore_lr=True)
    assert adam.step_count == 7 and adam.param_groups[0]["lr"] == model.lr
    with pytest.raises(ValueError):
        checkpoint.load(path, fresh, None, resume_optimizer=True)


def test_load_never_unpickles_objects_unless_asked(tmp_path):
    """A file that needs the unrestricted unpickler is refused (the original error surfaces, nothing is
    retried behind the caller's back); `allow_pickle=True` is the explicit opt-in."""
    model = _siren()
    ckpt = checkpoint.lightning_checkpoint(model, epoch=0, global_step=1, moments=_fake_moments(model, 3), step=1)
    ckpt["callbacks"] = {"cb": _Opaque()}
    path = str(tmp_path / "lightning.ckpt")
    torch.save(ckpt, path)
    import pickle
    with pytest.raises(pickle.UnpicklingError):
        checkpoint.load(path, _siren())
    checkpoint.load(path, _siren(), allow_pickle=True)
    with pytest.raises(FileNotFoundError):  # genuine errors are not masked either
        checkpoint.load(str(tmp_path / "missing.ckpt"), _siren())


class _Opaque:
    """Stands for the callback / hyper-parameter objects a Lightning checkpoint may hold."""


def test_saving_is_deterministic_and_leaves_the_rng_alone():
    model = _hash()
    torch.manual_seed(99)
    before = torch.random.get_rng_state()
    a = checkpoint.reference_state_dict(model)
    assert torch.equal(before, torch.random.get_rng_state())
    torch.manual_seed(5)
    b = checkpoint.reference_state_dict(model)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_a_sharded_optimizer_state_is_refused():
    model = _siren()
    adam = _CpuAdam(model)
    adam.sharded = True
    with pytest.raises(RuntimeError, match="sharded"):
        checkpoint._moments_by_name(model, adam)
