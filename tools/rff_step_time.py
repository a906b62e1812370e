"""A full RffNet training step (forward, loss, backward, Adam) on the MI355X, per step of n rows:

    python tools/rff_step_time.py [--out DIR] [--legs K] [--steps S]   (default: DIR = profiles, 7 legs)

(a) autograd  `training_step` + autograd over the layer ops + the flat Adam kernel: what `Trainer` runs without
              `fused_rff`, untouched by the fused step and so the yardstick,
(b) fused     `FusedStep(rff=True).train_step`: rff_forward_loss -> rff_backward -> adam (csrc/rff.hip), no autograd
              graph, the encoding z (n, 2F) never written.

Shapes: 3 -> 128 x 6 -> 1 (F = 128) at n = 2^18; 2 -> 64 x 3 -> 1 (F = 64) at n = 2^18 and at the notebook's batch of
5000.  All legs run in one process on the same seeded rows; the two forms train twin networks (same seed).  After a
warm-up of both forms of every shape the legs alternate, and each number is the median over the legs of a leg's mean
step time (HIP events around `steps` steps, synchronised).  Kernel launches per step are counted with the profiler; the
peak memory of one step is torch.cuda.max_memory_allocated above what is allocated before the step (workspaces, which
both forms keep between steps, are allocated by then: the peak is what a step adds, the held bytes are reported beside
it).  The claim per shape is whether (a) - (b) exceeds the largest leg spread of the run at that shape
(`beyond_spread`).  Writes DIR/rff_step_b262144.json."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mri_interpolation_amd import _lib, models, trainer  # noqa: E402

CASES = [(dict(dim_in=3, dim_hidden=128, dim_out=1, n_layers=6, n_frequencies=128), 1 << 18),
         (dict(dim_in=2, dim_hidden=64, dim_out=1, n_layers=3, n_frequencies=64), 1 << 18),
         (dict(dim_in=2, dim_hidden=64, dim_out=1, n_layers=3, n_frequencies=64), 5000)]


def leg_ms(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def summary(legs):
    return dict(median_ms=statistics.median(legs), min_ms=min(legs), max_ms=max(legs), spread_ms=max(legs) - min(legs),
                legs_ms=legs)


def launches(fn):
    """Kernel launches of one step, as the profiler sees them on the device."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return len([e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                and not e.name.lower().startswith(("memcpy", "memset"))])


def peak_bytes(fn):
    """(held before the step, peak of the caching allocator during one step above that)."""
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(before), int(torch.cuda.max_memory_allocated() - before)


def forms_of(config, n):
    g = torch.Generator().manual_seed(1)
    x = torch.rand(n, config["dim_in"], generator=g).cuda()
    y = torch.rand(n, 1, generator=g).cuda()
    nets = []
    for _ in range(2):  # twins
        torch.manual_seed(0)
        nets.append(models.RffNet(lr=1e-4, **config).cuda())
    plain, fused_net = nets
    opt = plain.configure_optimizers()
    opt.flatten()
    step = trainer.FusedStep(fused_net, fused_net.configure_optimizers(), rff=True)
    if not step.use_rff:
        raise RuntimeError("the fused RFF step does not take this network")
    last = {}

    def autograd():
        opt.zero_grad()
        loss = plain.training_step((x, y), 0)
        loss.backward()
        opt.step()
        last["autograd"] = loss.detach()

    def fused():
        last["fused"] = step.train_step(x, y)

    return dict(autograd=autograd, fused=fused), last


def measure(config, n, forms, last, steps, legs):
    times = {k: [] for k in forms}
    for _ in range(legs):  # alternate, so that every form sees the same clocks and neighbours
        for k, fn in forms.items():
            times[k].append(leg_ms(fn, steps))
    res = dict(n=n, config=config, device=torch.cuda.get_device_name(0), steps_per_leg=steps, legs=legs,
               per_step={k: summary(v) for k, v in times.items()})
    # the twins have taken the same number of steps on the same rows: their losses stay together
    res["last_loss"] = {k: float(v) for k, v in last.items()}
    t = {k: v["median_ms"] for k, v in res["per_step"].items()}
    spread = max(v["spread_ms"] for v in res["per_step"].values())
    res["fused_vs_autograd"] = dict(gain_ms=t["autograd"] - t["fused"], largest_spread_ms=spread,
                                    ratio=t["fused"] / t["autograd"], beyond_spread=t["autograd"] - t["fused"] > spread)
    res["ns_per_point"] = {k: v * 1e6 / n for k, v in t.items()}
    res["launches_per_step"] = {k: launches(fn) for k, fn in forms.items()}
    mem = {k: peak_bytes(fn) for k, fn in forms.items()}
    res["held_bytes_before_step"] = {k: v[0] for k, v in mem.items()}
    res["peak_bytes_per_step"] = {k: v[1] for k, v in mem.items()}
    return res


def take(argv, flag, default, kind):
    if flag in argv:
        i = argv.index(flag)
        value = kind(argv[i + 1])
        del argv[i:i + 2]
        return value
    return default


def main():
    argv = sys.argv[1:]
    out = take(argv, "--out", os.path.join(ROOT, "profiles"), str)
    legs = take(argv, "--legs", 7, int)
    steps = take(argv, "--steps", 0, int)
    _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("rff_step_time: no GPU (a step time is measured on the MI355X or not at all)")
    os.makedirs(out, exist_ok=True)
    results = []
    for config, n in CASES:  # one case at a time: the autograd path of the wide network holds ~2.5 GB of graph
        forms, last = forms_of(config, n)
        for _ in range(3):  # both forms warm before the first timed leg
            for fn in forms.values():
                fn()
        torch.cuda.synchronize()
        res = measure(config, n, forms, last, steps or (5 if n >= 1 << 16 else 50), legs)
        print(json.dumps(res, indent=1))
        results.append(res)
        del forms, last
        torch.cuda.empty_cache()
    path = os.path.join(out, "rff_step_b262144.json")
    with open(path, "w") as f:
        json.dump(dict(fused_beyond_spread_at_every_shape=all(r["fused_vs_autograd"]["beyond_spread"] for r in results),
                       shapes=results), f, indent=1)
    print("->", path)


if __name__ == "__main__":
    main()
