"""RffNet values and coordinate gradient on the MI355X, per call of n rows:

    python tools/rff_gradient_time.py [--out DIR] [--n ROWS]   (default: n = 2^18, DIR = profiles)

(a) autograd   the generic body, RffNet.forward_with_gradient(x): autograd through the encoding op and the layer ops
               -- the default, and the yardstick: what a user had before the kernel,
(b) kernel     forward_with_gradient(x, fused=True): the fused gradient kernel (csrc/rff.hip rff_gradient_kernel),
(c) forward    ops.rff_forward inference on the same rows (values only): the kernel (b) shares its tile loop with.

Three networks: 3 -> 128 x 6 -> 1 and 3 -> 64 x 4 -> 1 (four image rows per point) and 4 -> 128 x 6 -> 1 (the
eight-slot form), n_frequencies == dim_hidden.  All legs run in one process on the same seeded rows; after a warm-up
of every form of every shape the legs alternate and each number is the median over seven legs of a leg's mean call
time (HIP events around `calls` calls, synchronised).  The cost model: SL image rows per point (4, or 8 for dim_in = 4)
through every product and one sincos per point and frequency, so (b) should stay under SL x (c).  Kernel launches per
call are counted with the profiler; the peak memory of one call of (a) and of (b) is torch.cuda.max_memory_allocated
above what is allocated before the call.  Writes DIR/rff_gradient_b<rows>.json."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mri_interpolation_amd import _lib, models, ops  # noqa: E402

NETS = [dict(dim_in=3, dim_hidden=128, dim_out=1, n_layers=6, n_frequencies=128),
        dict(dim_in=3, dim_hidden=64, dim_out=1, n_layers=4, n_frequencies=64),
        dict(dim_in=4, dim_hidden=128, dim_out=1, n_layers=6, n_frequencies=128)]


def slots(config):
    """Image rows per point of the gradient kernel."""
    return 4 if config["dim_in"] <= 3 else 8


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
        raise RuntimeError("the fused RFF kernels do not take this network")
    y = torch.empty(n, 1, device="cuda")
    return dict(autograd=lambda: net.forward_with_gradient(x), kernel=lambda: net.forward_with_gradient(x, fused=True),
                forward=lambda: ops.rff_forward(x, y=y, **plan))


def measure(config, n, forms, calls=5, legs=7):
    ky, kg = forms["kernel"]()
    ay, ag = forms["autograd"]()
    agree = dict(y=float((ky - ay).abs().max() / ay.abs().max()), dydx=float((kg - ag).abs().max() / ag.abs().max()))
    del ky, kg, ay, ag
    times = {k: [] for k in forms}
    for _ in range(legs):  # alternate, so that every form sees the same clocks and neighbours
        for k, fn in forms.items():
            times[k].append(leg_ms(fn, calls))
    res = dict(n=n, config=config, device=torch.cuda.get_device_name(0), calls_per_leg=calls, legs=legs,
               slots=slots(config), kernel_vs_autograd_max_rel=agree, per_call={k: summary(v) for k, v in times.items()})
    t = {k: v["median_ms"] for k, v in res["per_call"].items()}
    spread = max(v["spread_ms"] for v in res["per_call"].values())
    res["kernel_vs_autograd"] = dict(gain_ms=t["autograd"] - t["kernel"], largest_spread_ms=spread,
                                     ratio=t["kernel"] / t["autograd"], beyond_spread=t["autograd"] - t["kernel"] > spread)
    res["kernel_over_forward"] = dict(ratio=t["kernel"] / t["forward"], cost_model_bound=float(slots(config)))
    res["ns_per_point"] = {k: v * 1e6 / n for k, v in t.items()}
    res["launches_per_call"] = {k: launches(fn) for k, fn in forms.items()}
    res["peak_bytes_per_call"] = {k: peak_bytes(forms[k]) for k in ("autograd", "kernel")}
    res["bytes_per_call"] = dict(kernel=4 * n * (2 * config["dim_in"] + 1))
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
    path = os.path.join(out, f"rff_gradient_b{n}.json")
    with open(path, "w") as f:
        json.dump(dict(n=n, shapes=results), f, indent=1)
    print("->", path)


if __name__ == "__main__":
    main()
