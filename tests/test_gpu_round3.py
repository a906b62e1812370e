"""Round-3 parity cases on the MI355X.

* The table-gradient record formats (`mri_set_option("bwd_records", ...)`) judged PER SLOT against a
  float64 evaluation of the same sum, with rigorous bounds: an f32 product is within 2^-24 of its
  magnitude, so no f32 evaluation of a slot can be expected closer than 2^-24 (sum of magnitudes + |sum|).
  Reference: autograd of encoding.py:127-128 (f32 products, f32 accumulation).
* A 200-step training run with packed against f32 records.
* float64 yardsticks for what rounds 1-2 compared at widened tolerances.
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import REL_TOL, ROOT, assert_close, load_golden
from yardstick import cfg4_gradient_case as _cfg4_gradient_case
from oracle import detrand
from oracle import hashgrid as ohash
from oracle import mlp as omlp
from oracle import train as otrain

pytestmark = pytest.mark.gpu

FIN4 = 16 * 1.4 ** 15
U = 2.0 ** -24  # unit roundoff of f32


@pytest.fixture(scope="module")
def amd():
    from mri_interpolation_amd import _lib, datamodules, encoding, models, ops, trainer
    assert torch.cuda.is_available(), "these tests need the GPU"
    _lib.load()
    yield type("NS", (), dict(lib=_lib, ops=ops, encoding=encoding, models=models,
                              trainer=trainer, datamodules=datamodules))
    _lib.set_option("bwd_records", 0)


def _report(name, payload):
    """Numbers a reader of DESIGN.md wants to see again: written beside the other GPU artefacts."""
    out = os.path.join(ROOT, "gpurun_out")
    if os.path.isdir(out):
        with open(os.path.join(out, name), "w") as f:
            json.dump(payload, f, indent=1)


# --------------------------------------------------------------------------- record formats
def _per_slot_stats(got, total, mag, floor):
    """max, rms and median of |got - exact| / |exact| over the slots whose exact value is above `floor`."""
    sel = total.abs() > floor
    rel = ((got[sel] - total[sel]).abs() / total[sel].abs())
    return float(rel.max()), float(rel.pow(2).mean().sqrt()), int(sel.sum()), float(rel.median())


def test_record_formats_per_slot_against_float64(amd):
    """BASELINE config 4 at its full batch (2^18 coordinates, 16 levels, T 2^19): every table-gradient
    path -- f32 records (default), packed 8-byte records, global f32 atomics -- against the float64 sum,
    slot by slot."""
    ops = amd.ops
    n = 1 << 18
    enc = amd.encoding.MultiResHashGrid(3, 16, 2, 19, 16, FIN4).cuda()
    res, sizes = ohash.resolutions_for(3, 16, 19, 16, FIN4)
    x, d = _cfg4_gradient_case(n, 71)
    yard = ohash.table_gradient_f64(x, d, sizes, res, 2)
    xg, dg = x.cuda(), d.t().contiguous().cuda()  # feature-major, as the fused step hands it over

    def run(method, records):
        amd.lib.set_option("bwd_records", records)
        g = torch.zeros_like(enc.table.data)
        ops.hashgrid_backward(enc.desc, xg, dg, g, feature_major=True, method=method)
        return g.double().cpu()

    paths = {"f32_records": run(2, 0), "packed_records": run(2, 1), "f32_atomics": run(1, 0)}
    amd.lib.set_option("bwd_records", 0)
    stats = {k: [] for k in ("f32_records", "packed_records", "f32_atomics")}
    for l in range(16):
        lo, hi = enc._row_span(l)
        total, mag, count = yard[l]
        gmax = float(d[:, 2 * l:2 * l + 2].abs().max())
        k = count.double().unsqueeze(1)
        # fixed point: one unit of 2^-40 max|g| per record at most (level_exponent keeps >= 40 bits)
        fixed = k * gmax * 2.0 ** -40
        bound_exact = U * (mag + total.abs()) * 1.001 + fixed
        # packed: every product first rounded to >= 18 significant bits (2^-18 of its magnitude on top
        # of its own f32 rounding), contributions below 2^(E-45) may vanish (E = exponent of max|g|)
        bound_packed = (2.0 ** -18 + U) * mag * 1.001 + U * total.abs() + fixed + k * gmax * 2.0 ** -43
        # f32 atomics: products rounded, then k - 1 rounded additions of partial sums <= mag
        bound_atomic = U * mag * (k + 1.0) * 1.001
        for name, bound in (("f32_records", bound_exact), ("packed_records", bound_packed),
                            ("f32_atomics", bound_atomic)):
            err = (paths[name][lo:hi] - total).abs()
            worst = float((err - bound).max())
            assert worst <= 0.0, f"{name} level {l}: a slot exceeds its bound by {worst:.3e}"
            # nothing in a slot no corner hashes to
            assert float(paths[name][lo:hi][count == 0].abs().max()) == 0.0 if (count == 0).any() else True
            stats[name].append(_per_slot_stats(paths[name][lo:hi], total, mag,
                                               1e-6 * float(total.abs().max())))
            # the usual per-level bound of the parity suite
            assert_close(paths[name][lo:hi].numpy(), total.numpy(), REL_TOL, f"{name} level {l}")
    summary = {k: dict(max_rel=max(s[0] for s in v), rms_rel=float(np.sqrt(np.mean([s[1] ** 2 for s in v]))),
                       median_rel=float(np.median([s[3] for s in v])), slots=sum(s[2] for s in v))
               for k, v in stats.items()}
    summary["ratio_packed_over_f32_records_rms"] = summary["packed_records"]["rms_rel"] / summary["f32_records"]["rms_rel"]
    summary["ratio_atomics_over_f32_records_rms"] = summary["f32_atomics"]["rms_rel"] / summary["f32_records"]["rms_rel"]
    _report("r3_records_accuracy.json", summary)
    print(json.dumps(summary))
    # the default records are at least as accurate as the reference's own accumulation (f32 atomics /
    # sequential f32 adds); the packed ones are NOT f32: measured here, they stay an option
    assert summary["f32_records"]["rms_rel"] <= summary["f32_atomics"]["rms_rel"] * 1.05
    assert summary["f32_records"]["median_rel"] <= U
    assert summary["ratio_packed_over_f32_records_rms"] <= 64.0


def test_record_formats_on_the_golden_encoders(amd):
    """Every golden encoder fixture through both F = 2 record formats: nothing lands in a slot the
    reference did not touch, the f32 records lose no entry the reference filled above 2^-36 of the
    level's maximum (the fixed-point unit is 2^-40 of max |d_out|), the packed ones none above 1e-9 of it."""
    for name in ("enc_cfg2", "enc_cfg4", "enc_cfg5_4d", "enc_defaults_2d", "enc_v2_cfg5", "enc_v2_notebook"):
        fx = load_golden(name)
        c = dict(fx.meta["ctor"])
        cls = getattr(amd.encoding, c.pop("cls"))
        dim = c.pop("dim")
        for key in ("base_resolution", "finest_resolution"):
            if isinstance(c.get(key), list):
                c[key] = tuple(c[key])
        enc = cls(dim, **c).cuda()
        if enc.n_features_per_level != 2:
            continue
        x, d_out = torch.as_tensor(fx["x"]).cuda(), torch.as_tensor(fx["d_out"]).cuda()
        for records, floor in ((0, 2.0 ** -36), (1, 1e-9)):
            amd.lib.set_option("bwd_records", records)
            g = torch.zeros_like(enc.table.data)
            amd.ops.hashgrid_backward(enc.desc, x, d_out, g, method=2)
            g = g.cpu()
            for l in range(enc.n_levels):
                lo, hi = enc._row_span(l)
                got = g[lo:hi].numpy()
                want = np.zeros_like(got)
                want[fx[f"grad_idx_{l}"]] = fx[f"grad_val_{l}"]
                nz = np.nonzero(np.abs(got).sum(axis=1))[0]
                assert np.isin(nz, fx[f"grad_idx_{l}"]).all(), f"{name} level {l}: stray slot"
                big = np.abs(want) > floor * np.abs(want).max()
                assert (got[big] != 0).all(), f"{name} level {l} records {records}: lost entry"
                assert_close(got, want, REL_TOL, f"{name} level {l} records {records}")
    amd.lib.set_option("bwd_records", 0)


def _train_cfg4_like(amd, records, steps, shape=(96, 96, 96)):
    """`steps` fused steps of the config-4 model (hash L16 F2 T2^19 growth 1.4 + MLP 128) on the analytic
    phantom with shuffled on-device batches; returns (flat parameters, PSNR over all voxels)."""
    amd.lib.set_option("bwd_records", records)
    dev = torch.device("cuda", 0)
    vol = amd.datamodules.phantom_volume(shape, device=dev)
    ds = amd.datamodules.MriImage(volume=vol, device=dev)
    loader = amd.datamodules.DeviceLoader(ds, 1 << 16, shuffle=True, drop_last=True, seed=1337)
    torch.manual_seed(1337)
    net = amd.models.HashMLP(3, 16, 2, 19, 16, FIN4, dim_hidden=128, n_layers=3,
                             activation=torch.nn.ReLU, batch_norm=False, final_activation=False,
                             lr=5e-3).cuda()
    step = amd.trainer.FusedStep(net, net.configure_optimizers())
    assert step.use_tiny
    pipe = amd.datamodules.BatchPipeline(loader)
    for _ in range(steps):
        coords, target = pipe.current()
        step.train_step(coords, target, pipe.produce_next)
        pipe.advance()
    preds = []
    with torch.no_grad():
        for xb, _ in amd.datamodules.DeviceLoader(ds, 1 << 18, shuffle=False):
            preds.append(step.forward(xb)[0].clone())
    db = amd.trainer.psnr(torch.cat(preds), ds.pixels)
    return step.flat.param.detach().double().cpu(), db


def test_packed_records_over_200_steps(amd):
    """200 Adam steps with packed records against the same run with f32 records: what the 18-21-bit
    records cost a TRAINING RUN.  Two f32-record runs are bitwise identical
    (the step is deterministic), so every difference below is the packed format's."""
    p_f32, db_f32 = _train_cfg4_like(amd, 0, 200)
    p_again, db_again = _train_cfg4_like(amd, 0, 200)
    p_pack, db_pack = _train_cfg4_like(amd, 1, 200)
    amd.lib.set_option("bwd_records", 0)
    assert torch.equal(p_f32, p_again) and db_f32 == db_again, "the f32-record run is not reproducible"
    diff = (p_pack - p_f32).abs()
    scale = float(p_f32.abs().max())
    rel_max, rel_l2 = float(diff.max()) / scale, float(diff.norm() / p_f32.norm())
    _report("r3_packed_200_steps.json", dict(psnr_f32_records=db_f32, psnr_packed_records=db_pack,
                                             param_rel_to_max=rel_max, param_rel_l2=rel_l2))
    print(f"200 steps: PSNR f32 records {db_f32:.4f} dB, packed {db_pack:.4f} dB; "
          f"parameters differ by {rel_max:.3e} of max, {rel_l2:.3e} in L2")
    assert abs(db_pack - db_f32) <= 0.01, (db_f32, db_pack)


# --------------------------------------------------------------------------- the reference's default model
def test_hashmlp_batchnorm_decoder_gradients_and_adam(amd):
    """`config.model_cls = HashMLP` as the reference builds it (models.py:712-739): encoder + Linear ->
    BatchNorm1d -> GELU -> Dropout(0) blocks in train() mode through the module / autograd path -- the HIP
    encoder and Linear kernels under torch's BatchNorm -- against the reference: loss, every gradient
    (tables, Linear and BatchNorm parameters), running statistics, two Adam steps."""
    fx = load_golden("hashmlp_bn_adam")
    m, c = fx.meta, fx.meta["ctor"]
    net = amd.models.HashMLP(dim_in=3, n_levels=c["n_levels"], n_features_per_level=c["n_features_per_level"],
                             log2_hashmap_size=c["log2_hashmap_size"],
                             base_resolution=tuple(c["base_resolution"]),
                             finest_resolution=tuple(c["finest_resolution"]), dim_hidden=64, dim_out=1,
                             n_layers=2, lr=m["lr"])
    assert net.encoder.sizes == m["sizes"] and isinstance(net.decoder[0][1], torch.nn.BatchNorm1d)
    with torch.no_grad():
        net.encoder.table.copy_(torch.cat(ohash.init_tables(m["sizes"], 1, m["table_seed"], m["table_scale"])))
        for blk, (w, b) in zip(net.decoder, omlp.linear_init(m["dims"], m["mlp_seed"])):
            blk[0].weight.copy_(w)
            blk[0].bias.copy_(b)
            blk[1].weight.copy_(torch.from_numpy(detrand.uniform(blk[1].weight.numel(), m["bn_seeds"][0], 0.5, 1.5)))
            blk[1].bias.copy_(torch.from_numpy(detrand.uniform(blk[1].bias.numel(), m["bn_seeds"][1], -0.2, 0.2)))
    net.cuda().train()
    opt = net.configure_optimizers()
    b_first = [blk[0].bias.detach().cpu().numpy().copy() for blk in net.decoder]
    for step in range(m["steps"]):
        x = torch.as_tensor(fx[f"x_{step}"]).cuda()
        y = torch.as_tensor(fx[f"y_{step}"]).cuda()
        b_before = [blk[0].bias.detach().cpu().numpy().copy() for blk in net.decoder]
        opt.zero_grad()
        loss = net.training_step((x, y), step)
        loss.backward()
        assert abs(float(loss) - float(fx[f"loss_{step}"])) <= REL_TOL * float(fx[f"loss_{step}"])
        if step == 0:
            g = net.encoder.table.grad.cpu().numpy()
            for l in range(net.encoder.n_levels):
                lo, hi = net.encoder._row_span(l)
                want = np.zeros((hi - lo, 1), dtype=np.float32)
                want[fx[f"grad_idx_{l}"]] = fx[f"grad_val_{l}"]
                assert set(np.nonzero(g[lo:hi, 0])[0]) <= set(fx[f"grad_idx_{l}"].tolist()), f"level {l}: stray slot"
                assert_close(g[lo:hi], want, REL_TOL, f"table gradient level {l}")
            for i, blk in enumerate(net.decoder):
                assert_close(blk[0].weight.grad.cpu().numpy(), fx[f"gw_{i}"], REL_TOL, f"gw{i}")
                assert_close(blk[1].weight.grad.cpu().numpy(), fx[f"bn_gw_{i}"], REL_TOL, f"bn gw{i}")
                assert_close(blk[1].bias.grad.cpu().numpy(), fx[f"bn_gb_{i}"], REL_TOL, f"bn gb{i}")
                # the Linear bias in front of a train-mode BatchNorm: exactly zero in exact arithmetic,
                # rounding noise in any f32 evaluation (tests/test_oracle_golden.py says what follows from it)
                assert float(blk[0].bias.grad.abs().max()) <= 1e-5 * float(blk[0].weight.grad.abs().max())
        opt.step()
        for i, blk in enumerate(net.decoder):
            assert_close(blk[0].weight.detach().cpu().numpy(), fx[f"w_{step}_{i}"], REL_TOL,
                         f"w{i} step {step}")
            assert_close(blk[1].weight.detach().cpu().numpy(), fx[f"bn_w_{step}_{i}"], REL_TOL, f"bn w{i} step {step}")
            assert_close(blk[1].bias.detach().cpu().numpy(), fx[f"bn_b_{step}_{i}"], REL_TOL, f"bn b{i} step {step}")
            b_ref = fx[f"b_{step - 1}_{i}"] if step else b_first[i]
            own = blk[1].running_mean.cpu().numpy() - 0.1 * b_before[i]
            ref = fx[f"bn_mean_{step}_{i}"] - 0.1 * b_ref
            assert np.abs(own - ref).max() <= REL_TOL * np.abs(fx[f"bn_mean_{step}_{i}"]).max(), (i, step)
            assert_close(blk[1].running_var.cpu().numpy(), fx[f"bn_var_{step}_{i}"], REL_TOL, f"bn var{i} step {step}")
        table = net.encoder.table.detach().cpu().numpy()
        for l in range(net.encoder.n_levels):
            lo, hi = net.encoder._row_span(l)
            assert_close(table[lo:hi][fx[f"grad_idx_{l}"]], fx[f"table_{step}_{l}"], REL_TOL, f"table {l} step {step}")
    # eval mode from the reference's final state (the rows x_0 touches are in the fixture)
    last = m["steps"] - 1
    with torch.no_grad():
        for l in range(net.encoder.n_levels):
            lo, hi = net.encoder._row_span(l)
            net.encoder.table.data[lo:hi][torch.as_tensor(fx[f"grad_idx_{l}"].astype(np.int64)).cuda()] = \
                torch.as_tensor(fx[f"table_{last}_{l}"]).cuda()
        for i, blk in enumerate(net.decoder):
            blk[0].weight.copy_(torch.as_tensor(fx[f"w_{last}_{i}"]))
            blk[0].bias.copy_(torch.as_tensor(fx[f"b_{last}_{i}"]))
            blk[1].weight.copy_(torch.as_tensor(fx[f"bn_w_{last}_{i}"]))
            blk[1].bias.copy_(torch.as_tensor(fx[f"bn_b_{last}_{i}"]))
            blk[1].running_mean.copy_(torch.as_tensor(fx[f"bn_mean_{last}_{i}"]))
            blk[1].running_var.copy_(torch.as_tensor(fx[f"bn_var_{last}_{i}"]))
        net.eval()
        pred = net.predict_step((torch.as_tensor(fx["x_0"]).cuda(), None), 0)
    assert_close(pred.cpu().numpy(), fx["pred_eval_after"], REL_TOL, "eval-mode prediction")


# --------------------------------------------------------------------------- checkpoints
def test_launcher_checkpoint_resumes_parameters_and_optimizer(amd, tmp_path):
    """`launcher.py` writes Lightning's default checkpoint in Lightning's layout (checkpoint.py); loaded
    into a fresh model + optimiser (`resume_optimizer=True`, Lightning's fit(ckpt_path=)) it restores
    parameters, BOTH Adam moments and the step count bit for bit.  `--checkpoint_path` alone is the
    reference's resume (launcher.py:97-165: weights from the file, a fresh Adam at --lr);
    `--resume_optimizer` continues the optimiser too."""
    import glob
    import launcher
    from mri_interpolation_amd import checkpoint
    out = str(tmp_path / "run")
    argv = ["--model_class", "HashMLP", "--tiny_mlp", "--synthetic", "24,24,24", "--batch_size", "2048",
            "--epochs", "2", "--out_dir", out, "--log_every", "0"]
    launcher.main(argv)
    files = glob.glob(os.path.join(out, "checkpoints", "epoch=1-step=*.ckpt"))
    assert len(files) == 1
    ckpt = torch.load(files[0], weights_only=True)
    steps = ckpt["global_step"]
    assert steps >= 2 and ckpt["epoch"] == 1 and ckpt["pytorch-lightning_version"]
    assert any(k.startswith("layers.") for k in ckpt["state_dict"])  # the reference's dead stack (Q3)
    state = ckpt["optimizer_states"][0]["state"]
    assert state and all(float(s["step"]) == steps for s in state.values())
    # a fresh model with the same constructor arguments
    sd = ckpt["state_dict"]
    n_levels = len([k for k in sd if k.startswith("encoder.levels.")])
    hidden, k_in = sd["decoder.0.0.weight"].shape
    net = amd.models.HashMLP(3, n_levels, k_in // n_levels, 19, 16, FIN4, dim_hidden=hidden, n_layers=3,
                             activation=torch.nn.ReLU, batch_norm=False, final_activation=False, lr=5e-3)
    if [tuple(sd[f"encoder.levels.{l}.embedding.weight"].shape) for l in range(n_levels)] != \
            [(s, k_in // n_levels) for s in net.encoder.sizes]:
        pytest.skip("the launcher's default --tiny_mlp encoder is not the one rebuilt here")
    net.cuda()
    opt = net.configure_optimizers()
    checkpoint.load(files[0], net, opt, map_location="cuda", resume_optimizer=True)
    assert opt.step_count == steps
    again = checkpoint.lightning_checkpoint(net, opt, epoch=1, global_step=steps)
    for k, v in ckpt["state_dict"].items():
        if not k.startswith("layers."):
            assert torch.equal(v, again["state_dict"][k]), k
    for i, s in state.items():
        t = again["optimizer_states"][0]["state"][i]
        assert torch.equal(s["exp_avg"], t["exp_avg"]) and torch.equal(s["exp_avg_sq"], t["exp_avg_sq"]), i
    # the launcher resumes from it.  Default = the reference: weights only, Adam restarts at step 0 with the
    # learning rate of THIS command line; --resume_optimizer continues moments and step count (still at --lr)
    out2 = str(tmp_path / "resumed")
    launcher.main(argv[:-4] + ["--out_dir", out2, "--log_every", "0", "--checkpoint_path", files[0],
                               "--lr", "0.002"])
    resumed = glob.glob(os.path.join(out2, "checkpoints", "*.ckpt"))
    assert len(resumed) == 1
    r = torch.load(resumed[0], weights_only=True)
    rs = r["optimizer_states"][0]
    assert all(float(s["step"]) == steps for s in rs["state"].values()), "a fresh Adam counts from zero"
    assert rs["param_groups"][0]["lr"] == 0.002, "--lr was ignored on resume"
    out3 = str(tmp_path / "continued")
    launcher.main(argv[:-4] + ["--out_dir", out3, "--log_every", "0", "--checkpoint_path", files[0],
                               "--resume_optimizer", "--lr", "0.002"])
    r = torch.load(glob.glob(os.path.join(out3, "checkpoints", "*.ckpt"))[0], weights_only=True)
    rs = r["optimizer_states"][0]
    assert all(float(s["step"]) == 2 * steps for s in rs["state"].values()), "the optimiser's step count restarted"
    assert rs["param_groups"][0]["lr"] == 0.002


# --------------------------------------------------------------------------- batch producer
@pytest.mark.parametrize("steps", [None, 7])
def test_grouped_batch_production_gives_the_same_batches(amd, steps):
    """BatchPipeline(group = R) produces R batches per launch pair: every batch -- coordinates and targets --
    equals what the one-batch-per-launch pipeline yields, over epoch boundaries, with a short last batch
    (steps = None) and with the cyclic fixed-step walk of a data-parallel shard (steps = 7), driven through
    the produce_next / produce_late / advance protocol of FusedStep.train_step."""
    dev = torch.device("cuda", 0)
    vol = amd.datamodules.phantom_volume((20, 18, 16), device=dev)
    ds = amd.datamodules.MriImage(volume=vol, device=dev)

    def walk(group, n_batches):
        loader = amd.datamodules.DeviceLoader(ds, 1000, shuffle=True, seed=11, lo=100, hi=5700, steps=steps)
        pipe = amd.datamodules.BatchPipeline(loader, group=group)
        out = []
        for _ in range(n_batches):
            c, t = pipe.current()
            out.append((c.clone(), t.clone()))
            nxt = pipe.produce_next()
            pipe.produce_late()
            pipe.advance()
            assert nxt.data_ptr() == pipe.current()[0].data_ptr() and nxt.shape == pipe.current()[0].shape
        return out

    per_epoch = 7 if steps else 6      # 5600 voxels: five batches of 1000 and one of 600
    ref = walk(1, 3 * per_epoch + 2)
    assert [c.shape[0] for c, _ in ref[:per_epoch]] == ([1000] * 7 if steps else [1000] * 5 + [600])
    for group in (2, 4, 8):
        got = walk(group, 3 * per_epoch + 2)
        for k, ((c0, t0), (c1, t1)) in enumerate(zip(ref, got)):
            assert torch.equal(c0, c1) and torch.equal(t0, t1), (group, k)


# --------------------------------------------------------------------------- the natively queued step
@pytest.mark.parametrize("hidden,records", [(128, 0), (64, 0), (128, 1)])
def test_steady_loop_equals_the_eager_loop(amd, hidden, records):
    """trainer.SteadyLoop queues the fused step with ONE library call (`mri_fused_step`): after 70 steps over
    several epochs -- eager steps mixed in -- parameters, both Adam moments and the step count equal the eager
    loop's bit for bit.  (Round 3's hipGraph-replay form and its spatially ordered batches were removed in round 4.)"""
    amd.lib.set_option("bwd_records", records)
    dev = torch.device("cuda", 0)
    vol = amd.datamodules.phantom_volume((40, 40, 40), device=dev)
    ds = amd.datamodules.MriImage(volume=vol, device=dev)

    def build():
        torch.manual_seed(1337)
        net = amd.models.HashMLP(3, 16, 2, 15, 16, 512, dim_hidden=hidden, n_layers=3, activation=torch.nn.ReLU,
                                 batch_norm=False, final_activation=False, lr=5e-3).cuda()
        step = amd.trainer.FusedStep(net, net.configure_optimizers())
        loader = amd.datamodules.DeviceLoader(ds, 4096, shuffle=True, drop_last=True, seed=1337)
        return net, step, amd.datamodules.BatchPipeline(loader)

    n_steps = 70
    _, eager, pipe_e = build()
    losses_e = []
    for _ in range(n_steps):
        c, t = pipe_e.current()
        losses_e.append(float(eager.train_step(c, t, pipe_e.produce_next)))
        pipe_e.advance()
    _, st, pipe_g = build()
    loop = amd.trainer.SteadyLoop(st, pipe_g).capture(warm_steps=4)
    done = 4
    assert pipe_g.k == done and st.opt.step_count == done
    losses_g = []
    while done < n_steps:
        if done in (20, 21, 37):  # eager steps in between, odd and even parity, back to back and alone
            losses_g.append(float(loop.eager_step()))
        else:
            losses_g.append(float(loop.step_once()))
        done += 1
    loop.finish()
    torch.cuda.synchronize()
    amd.lib.set_option("bwd_records", 0)
    assert losses_g == losses_e[4:], "losses differ"
    assert st.opt.step_count == eager.opt.step_count == n_steps and pipe_g.k == pipe_e.k
    assert torch.equal(st.flat.param, eager.flat.param), "parameters differ"
    assert torch.equal(st.flat.exp_avg, eager.flat.exp_avg) and torch.equal(st.flat.exp_avg_sq, eager.flat.exp_avg_sq)
    # the loop refuses what it cannot replay
    _, st2, pipe2 = build()
    st2.world, st2.grad_buckets = 2, 4  # several ranks: only the plain all-reduce form is queued natively
    assert "plain all-reduce" in amd.trainer.SteadyLoop.unsupported(st2, pipe2)
    st2.grad_buckets = 1
    assert amd.trainer.SteadyLoop.unsupported(st2, pipe2) is None
    short = amd.datamodules.DeviceLoader(ds, 4096, shuffle=True, drop_last=False, seed=1)
    assert "full" in amd.trainer.SteadyLoop.unsupported(st, amd.datamodules.BatchPipeline(short))
    with pytest.raises(ValueError, match="native"):
        amd.trainer.SteadyLoop(st2, pipe2, mode="graph")


def test_trainer_fit_with_native_steps_equals_eager_fit(amd):
    """Trainer.fit queues steady-state steps through SteadyLoop (one mri_fused_step call each) once four eager
    steps have set the state up; the parameters after three epochs equal Trainer(native_steps=False)'s bit for
    bit, the step counts agree, and a range that leaves a short last batch falls back to eager steps."""
    dev = torch.device("cuda", 0)
    vol = amd.datamodules.phantom_volume((32, 32, 32), device=dev)
    ds = amd.datamodules.MriImage(volume=vol, device=dev)
    out = []
    for native in (True, False):
        torch.manual_seed(1337)
        net = amd.models.HashMLP(3, 16, 2, 15, 16, 512, dim_hidden=128, n_layers=3, activation=torch.nn.ReLU,
                                 batch_norm=False, final_activation=False, lr=5e-3).cuda()
        loader = amd.datamodules.DeviceLoader(ds, 2048, shuffle=True, seed=7)  # 32768 voxels: 16 full batches
        tr = amd.trainer.Trainer(max_epochs=3, native_steps=native, log_every=0)
        tr.fit(net, loader)
        torch.cuda.synchronize()
        out.append((tr.fused.flat.param.clone(), tr.global_step, tr.fused.opt.step_count))
    assert out[0][1] == out[1][1] == 48 and out[0][2] == out[1][2] == 48
    assert torch.equal(out[0][0], out[1][0]), "native steps changed the parameters"
    torch.manual_seed(1337)
    net = amd.models.HashMLP(3, 16, 2, 15, 16, 512, dim_hidden=128, n_layers=3, activation=torch.nn.ReLU,
                             batch_norm=False, final_activation=False, lr=5e-3).cuda()
    ragged = amd.datamodules.DeviceLoader(ds, 3000, shuffle=True, seed=7)  # last batch of an epoch: 2768 rows
    tr = amd.trainer.Trainer(max_epochs=2, log_every=0)
    tr.fit(net, ragged)
    assert tr.global_step == 2 * 11 and bool(torch.isfinite(tr.fused.flat.param).all())


