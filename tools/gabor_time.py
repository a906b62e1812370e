"""GaborNet inference on the MI355X, per call of n rows:

    python tools/gabor_time.py [--out DIR] [--n ROWS]   (default: n = 2^18, DIR = profiles)

(a) torch    the same network in plain PyTorch-ROCm ops (F.linear, torch.cos, torch.exp): no project code at all,
(b) layers   the layer path: two linear.hip launches and one gabor_activation launch per layer (csrc/gabor.hip),
(c) fused    ops.gabor_forward: one persistent kernel (csrc/gabor.hip), one LDS image, nothing (n, hidden)-sized written.

Two networks: 3 -> 128 x 6 -> 1 and 2 -> 64 x 3 -> 1, at the class defaults (w0, sigma) = (30, 10).  All legs run in
one process on the same seeded rows; after a warm-up of every form of both shapes the legs alternate and each number
is the median over seven legs of a leg's mean call time (HIP events around `calls` calls, synchronised).  Kernel
launches per call are counted with the profiler; the peak memory of one call is torch.cuda.max_memory_allocated above
what is allocated before the call.  The fused kernel is GaborNet's default inference path only if it beats BOTH other
legs by more than the largest leg spread of the run at BOTH shapes (`fused_beyond_spread_at_every_shape`).  Writes
DIR/gabor_forward_b<rows>.json."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from mri_interpolation_amd import _lib, models, ops  # noqa: E402

NETS = [dict(dim_in=3, dim_hidden=128, dim_out=1, n_layers=6, sigma=10.0, w0=30.0),
        dict(dim_in=2, dim_hidden=64, dim_out=1, n_layers=3, sigma=10.0, w0=30.0)]


def leg_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def summary(legs):
    return dict(median_ms=statistics.median(legs), min_ms=min(legs), max_ms=max(legs), spread_ms=max(legs) - min(legs),
                legs_ms=legs)


def launches(fn):
    """Kernel launches of one call, as the profiler sees them on the device."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return len([e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                and not e.name.lower().startswith(("memcpy", "memset"))])


def peak_bytes(fn):
    """Peak of the caching allocator during one call, above what the call finds allocated."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return int(peak)


def forms_of(config, n):
    torch.manual_seed(0)
    net = models.GaborNet(fused_inference=True, **config).cuda().eval()
    g = torch.Generator().manual_seed(1)
    x = torch.rand(n, config["dim_in"], generator=g).cuda()
    plan = net._inference_plan(x)
    if plan is None:
        raise RuntimeError("the fused Gabor inference kernel does not take this network")
    params = [(l.freqs.weight.detach(), l.freqs.bias.detach(), l.scale.weight.detach(), l.scale.bias.detach())
              for l in net.layers]
    w0, c = float(config["w0"]), float(config["sigma"])

    def plain():
        with torch.no_grad():
            h = x
            for wf, bf, ws, bs in params:
                omega = w0 * F.linear(h, wf, bf)
                scale = F.linear(h, ws, bs) * c
                h = torch.cos(omega) * torch.exp(-(scale ** 2))
            return h

    def layers():
        with torch.no_grad():
            return net.layers(x)

    return dict(torch=plain, layers=layers, fused=lambda: ops.gabor_forward(x, **plan))


def measure(config, n, forms, calls=5, legs=7):
    outs = {k: fn() for k, fn in forms.items()}
    scale = outs["torch"].abs().max().clamp_min(1e-30)
    agree = {k: float((outs[k] - outs["torch"]).abs().max() / scale) for k in ("layers", "fused")}
    del outs
    times = {k: [] for k in forms}
    for _ in range(legs):  # alternate, so that every form sees the same clocks and neighbours
        for k, fn in forms.items():
            times[k].append(leg_ms(fn, calls))
    res = dict(n=n, config=config, device=torch.cuda.get_device_name(0), calls_per_leg=calls, legs=legs,
               max_rel_from_torch=agree, per_call={k: summary(v) for k, v in times.items()})
    t = {k: v["median_ms"] for k, v in res["per_call"].items()}
    spread = max(v["spread_ms"] for v in res["per_call"].values())
    best_other = min(t["torch"], t["layers"])
    res["fused_vs_others"] = dict(gain_over_torch_ms=t["torch"] - t["fused"], gain_over_layers_ms=t["layers"] - t["fused"],
                                  largest_spread_ms=spread, ratio_to_best_other=t["fused"] / best_other,
                                  beyond_spread=best_other - t["fused"] > spread)
    res["ns_per_point"] = {k: v * 1e6 / n for k, v in t.items()}
    res["launches_per_call"] = {k: launches(fn) for k, fn in forms.items()}
    res["peak_bytes_per_call"] = {k: peak_bytes(fn) for k, fn in forms.items()}
    res["bytes_per_call"] = dict(fused=4 * n * (config["dim_in"] + 1))
    return res


def main():
    argv = sys.argv[1:]
    out, n = os.path.join(ROOT, "profiles"), 1 << 18
    if "--out" in argv:
        i = argv.index("--out")
        out = argv[i + 1]
        del argv[i:i + 2]
    if "--n" in argv:
        i = argv.index("--n")
        n = int(argv[i + 1])
        del argv[i:i + 2]
    _lib.load()
    os.makedirs(out, exist_ok=True)
    all_forms = [forms_of(config, n) for config in NETS]
    for forms in all_forms:  # every shape warm before the first timed leg
        for _ in range(3):
            for fn in forms.values():
                fn()
    torch.cuda.synchronize()
    results = []
    for config, forms in zip(NETS, all_forms):
        res = measure(config, n, forms)
        print(json.dumps(res, indent=1))
        results.append(res)
    decision = all(r["fused_vs_others"]["beyond_spread"] for r in results)
    path = os.path.join(out, f"gabor_forward_b{n}.json")
    with open(path, "w") as f:
        json.dump(dict(n=n, fused_beyond_spread_at_every_shape=decision, shapes=results), f, indent=1)
    print("->", path)


if __name__ == "__main__":
    main()
