"""RffNet inference on the MI355X, per call of n rows:

    python tools/rff_time.py [--out DIR] [--n ROWS]   (default: n = 2^18, DIR = profiles)

(a) layers   the layer path: the encoding kernel (csrc/rff.hip) writes z (n, 2F), then one linear.hip launch per Linear
             with the ReLU fused -- what a user has without the fused kernel, and the yardstick,
(b) fused    ops.rff_forward: one persistent kernel (csrc/rff.hip), the encoding in two LDS images, z never written.

Two networks: 3 -> 128 x 6 -> 1 and 2 -> 64 x 3 -> 1 (n_frequencies = dim_hidden).  All legs run in one process on the
same seeded rows; after a warm-up of both forms of both shapes the legs alternate and each number is the median over
seven legs of a leg's mean call time (HIP events around `calls` calls, synchronised).  Kernel launches per call are
counted with the profiler; the peak memory of one call is torch.cuda.max_memory_allocated above what is allocated
before the call.  The fused kernel is RffNet's default inference path only if (a) - (b) exceeds the largest leg spread
of the run at BOTH shapes (`fused_beyond_spread_at_every_shape`).  Writes DIR/rff_forward_b<rows>.json."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mri_interpolation_amd import _lib, models, ops  # noqa: E402

NETS = [dict(dim_in=3, dim_hidden=128, dim_out=1, n_layers=6, n_frequencies=128),
        dict(dim_in=2, dim_hidden=64, dim_out=1, n_layers=3, n_frequencies=64)]


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
    net = models.RffNet(**config).cuda().eval()
    g = torch.Generator().manual_seed(1)
    x = torch.rand(n, config["dim_in"], generator=g).cuda()
    plan = net._inference_plan(x)
    if plan is None:
        raise RuntimeError("the fused RFF inference kernel does not take this network")

    def layers():
        with torch.no_grad():
            return net.decoder(net.encoder(x))

    return dict(layers=layers, fused=lambda: ops.rff_forward(x, **plan))


def measure(config, n, forms, calls=5, legs=7):
    fy, ly = forms["fused"](), forms["layers"]()
    agree = float((fy - ly).abs().max() / ly.abs().max().clamp_min(1e-30))
    del fy, ly
    times = {k: [] for k in forms}
    for _ in range(legs):  # alternate, so that every form sees the same clocks and neighbours
        for k, fn in forms.items():
            times[k].append(leg_ms(fn, calls))
    res = dict(n=n, config=config, device=torch.cuda.get_device_name(0), calls_per_leg=calls, legs=legs,
               fused_vs_layers_max_rel=agree, per_call={k: summary(v) for k, v in times.items()})
    t = {k: v["median_ms"] for k, v in res["per_call"].items()}
    spread = max(v["spread_ms"] for v in res["per_call"].values())
    res["fused_vs_layers"] = dict(gain_ms=t["layers"] - t["fused"], largest_spread_ms=spread,
                                  ratio=t["fused"] / t["layers"], beyond_spread=t["layers"] - t["fused"] > spread)
    res["ns_per_point"] = {k: v * 1e6 / n for k, v in t.items()}
    res["launches_per_call"] = {k: launches(fn) for k, fn in forms.items()}
    res["peak_bytes_per_call"] = {k: peak_bytes(fn) for k, fn in forms.items()}
    res["bytes_per_call"] = dict(fused=4 * n * (config["dim_in"] + 1),
                                 z_not_written=8 * n * config["n_frequencies"])
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
    decision = all(r["fused_vs_layers"]["beyond_spread"] for r in results)
    path = os.path.join(out, f"rff_forward_b{n}.json")
    with open(path, "w") as f:
        json.dump(dict(n=n, fused_beyond_spread_at_every_shape=decision, shapes=results), f, indent=1)
    print("->", path)


if __name__ == "__main__":
    main()
