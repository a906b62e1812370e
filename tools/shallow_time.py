"""The notebook's HashMLP (Linear -> GELU decoder, no BatchNorm) per training step on the MI355X, three ways:

    python tools/shallow_time.py [--out DIR] [batch ...]        (default: 20000 262144, DIR = profiles)

(a) the module path with autograd (training_step + loss.backward() + Adam), (b) FusedStep with
use_shallow = False (the layer kernels of csrc/linear*.hip), (c) FusedStep with the one-kernel shallow decoder
(csrc/mlp_shallow.hip).  The model is the notebook's (cell 37; reference models.py:712-739 without BatchNorm):
V2 grid L8 F2 T2^23 (64,64,5) -> (512,512,15), decoder 16 -> 64 -> 1 with GELU behind both Linears, lr 5e-3.
All three run in one process on the same seeded batch from the same initial state; after a warm-up the legs
alternate and each number is the median over the legs of a leg's mean step time (HIP events around `steps`
steps).  forward(train=False) is timed both ways at 2^20 rows.  Writes DIR/r07_shallow_b<batch>.json with the
per-leg values, the fused step's phases (FusedStep.phase_ms), the bytes the decoder kernel must move over its
time, and coordinate samples per second beside the reference's published figures."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mri_interpolation_amd import _lib, models, trainer  # noqa: E402

NOTEBOOK = dict(dim_in=3, n_levels=8, n_features_per_level=2, log2_hashmap_size=23, base_resolution=(64, 64, 5),
                finest_resolution=(512, 512, 15), dim_hidden=64, dim_out=1, n_layers=2, activation=torch.nn.GELU,
                batch_norm=False, lr=5e-3)
REFERENCE = dict(train_coords_per_s=325e3, predict_coords_per_s=823e3,
                 note="the reference's only published figures for this model (BASELINE.md): an unnamed CUDA GPU, "
                      "DataLoader-bound -- context, not a same-node comparison")
PREDICT_ROWS = 1 << 20


def leg_ms(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def summary(legs):
    return dict(median_ms=statistics.median(legs), spread_ms=max(legs) - min(legs), legs_ms=legs)


def measure(batch, warmup=10, steps=30, legs=7):
    torch.manual_seed(0)
    nets = [models.HashMLP(**NOTEBOOK).cuda().train() for _ in range(3)]
    with torch.no_grad():
        nets[0].encoder.table.uniform_(-0.5, 0.5)
    for net in nets[1:]:
        net.load_state_dict(nets[0].state_dict())
    g = torch.Generator().manual_seed(1)
    x = torch.rand(batch, 3, generator=g).cuda()
    y = torch.rand(batch, 1, generator=g).cuda()
    opt = nets[0].configure_optimizers()

    def autograd_step():
        opt.zero_grad()
        loss = nets[0].training_step((x, y), 0)
        loss.backward()
        opt.step()

    layerwise = trainer.FusedStep(nets[1], nets[1].configure_optimizers())
    fused = trainer.FusedStep(nets[2], nets[2].configure_optimizers())
    if not fused.use_shallow:
        raise RuntimeError("the shallow plan did not match the notebook's decoder")
    layerwise.use_shallow = False
    forms = dict(autograd=autograd_step, layerwise=lambda: layerwise.train_step(x, y),
                 fused=lambda: fused.train_step(x, y))
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(legs):  # alternate, so that all forms see the same clocks and neighbours
        for k, fn in forms.items():
            times[k].append(leg_ms(fn, steps))
    res = dict(batch=batch, config={k: (v.__name__ if isinstance(v, type) else v) for k, v in NOTEBOOK.items()},
               device=torch.cuda.get_device_name(0), steps_per_leg=steps, legs=legs,
               train={k: summary(v) for k, v in times.items()})
    b, c = res["train"]["layerwise"], res["train"]["fused"]
    margin = max(b["spread_ms"], c["spread_ms"])
    res["fused_vs_layerwise"] = dict(gain_ms=b["median_ms"] - c["median_ms"], larger_spread_ms=margin,
                                     ratio=c["median_ms"] / b["median_ms"],
                                     beyond_spread=b["median_ms"] - c["median_ms"] > margin)
    for name, step in (("fused", fused), ("layerwise", layerwise)):
        step.phase_events = {}
        for _ in range(20):
            forms[name]()
        res[f"{name}_phases_ms"] = step.phase_ms()
        step.phase_events = None
    k_in = fused.layers[0].weight.shape[1]
    must_move = 4 * batch * (2 * k_in + 2)  # x and d_x (k_in, n), target and y (n)
    dec_ms = res["fused_phases_ms"]["mlp_fused"]
    res["decoder_kernel"] = dict(bytes_floor=must_move, ms=dec_ms, tb_per_s=must_move / (dec_ms * 1e-3) / 1e12,
                                 note="the bracket holds the decoder kernel and its slab reduction, launch gaps "
                                      "included")
    # inference, both ways, on PREDICT_ROWS rows
    xp = torch.rand(PREDICT_ROWS, 3, generator=g).cuda()
    pred = {}
    with torch.no_grad():
        for name, step in (("layerwise", layerwise), ("fused", fused)):
            for _ in range(3):
                step.forward(xp, train=False)
        torch.cuda.synchronize()
        ptimes = dict(layerwise=[], fused=[])
        for _ in range(legs):
            for name, step in (("layerwise", layerwise), ("fused", fused)):
                ptimes[name].append(leg_ms(lambda: step.forward(xp, train=False), 10))
    res["predict"] = dict(rows=PREDICT_ROWS, **{k: summary(v) for k, v in ptimes.items()})
    res["coords_per_s"] = dict(
        train={k: batch / (v["median_ms"] * 1e-3) for k, v in res["train"].items()},
        predict={k: PREDICT_ROWS / (res["predict"][k]["median_ms"] * 1e-3) for k in ("layerwise", "fused")},
        reference=REFERENCE)
    return res


def main():
    argv = sys.argv[1:]
    out = os.path.join(ROOT, "profiles")
    if "--out" in argv:
        i = argv.index("--out")
        out = argv[i + 1]
        del argv[i:i + 2]
    batches = [int(a) for a in argv] or [20000, 1 << 18]
    _lib.load()
    os.makedirs(out, exist_ok=True)
    for batch in batches:
        res = measure(batch)
        print(json.dumps({k: v for k, v in res.items() if k not in ("config",)}, indent=1))
        path = os.path.join(out, f"r07_shallow_b{batch}.json")
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
        print("->", path)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
