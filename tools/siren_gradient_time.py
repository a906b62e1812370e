"""SirenNet values and coordinate gradient on the MI355X, per call of n rows:

    python tools/siren_gradient_time.py [--out DIR] [--n ROWS]   (default: n = 2^18, DIR = profiles)

(a) kernel        SirenNet.forward_with_gradient: the fused gradient kernel (csrc/siren_gradient.hip),
(b) autograd      BaseMLP.forward_with_gradient: autograd through the model's own forward (the layer ops), what a user
                  had before the kernel,
(c) forward       ops.siren_forward inference on the same rows (values only) -- at hidden 256 the register-resident
                  rows kernel by default --, and
(c0) forward_lds  the same with the "siren_rows" option at 0: the LDS-image forward kernel, the form the gradient
                  kernel shares its tile loop with (the like-for-like ratio).

Four networks: BASELINE config 3's (3 -> 256 x 5 -> 1) and 3 -> 64 x 4 -> 1, and for a 4-D volume (the kernel's
eight-slot form) 4 -> 256 x 5 -> 1 and 4 -> 128 x 6 -> 1, the width and depth the launcher's SirenNet defaults to.
All legs run in one process on the same seeded rows; after a warm-up of every form the legs alternate and each
number is the median over the legs of a leg's mean call time (HIP events around `calls` calls, synchronised).  The
cost model: four image rows per point (eight with dim_in = 4) through the H x H products and one sincos per four
rows, so (a) should stay under 4 x (c0) (8 x with dim_in = 4).  Kernel launches per call are counted with the
profiler.  Writes DIR/siren_gradient_<hidden>x<layers>_n<rows>.json (siren_gradient_d4_... for dim_in = 4)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mri_interpolation_amd import _lib, models, ops  # noqa: E402

NETS = [dict(dim_in=3, dim_hidden=256, dim_out=1, n_layers=5), dict(dim_in=3, dim_hidden=64, dim_out=1, n_layers=4),
        dict(dim_in=4, dim_hidden=256, dim_out=1, n_layers=5), dict(dim_in=4, dim_hidden=128, dim_out=1, n_layers=6)]


def slots(dim_in):
    """Image rows per point of the gradient kernel."""
    return 4 if dim_in <= 3 else 8


def profile_name(config, n):
    """The 3-D networks keep the names of the committed profiles; other input dimensions carry theirs."""
    dim = "" if config["dim_in"] == 3 else f"d{config['dim_in']}_"
    return f"siren_gradient_{dim}{config['dim_hidden']}x{config['n_layers']}_n{n}.json"


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


def measure(config, n, warmup=3, calls=5, legs=7):
    torch.manual_seed(0)
    net = models.SirenNet(**config).cuda().eval()
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(n, config["dim_in"], generator=g) * 2 - 1).cuda()
    plan = net._gradient_plan(x)
    if plan is None:
        raise RuntimeError("the fused gradient kernel does not take this network")
    y = torch.empty(n, 1, device="cuda")
    rows_default = _lib.get_option("siren_rows")

    def forward():
        ops.siren_forward(x, plan["weights"], plan["biases"], plan["w0_first"], plan["w0"], y=y)

    def forward_lds():
        _lib.set_option("siren_rows", 0)
        try:
            forward()
        finally:
            _lib.set_option("siren_rows", rows_default)

    forms = dict(kernel=lambda: net.forward_with_gradient(x), autograd=lambda: models.BaseMLP.forward_with_gradient(net, x),
                 forward=forward, forward_lds=forward_lds)
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    ky, kg = forms["kernel"]()
    ay, ag = forms["autograd"]()
    agree = dict(y=float((ky - ay).abs().max() / ay.abs().max()), dydx=float((kg - ag).abs().max() / ag.abs().max()))
    times = {k: [] for k in forms}
    for _ in range(legs):  # alternate, so that every form sees the same clocks and neighbours
        for k, fn in forms.items():
            times[k].append(leg_ms(fn, calls))
    res = dict(n=n, config=config, device=torch.cuda.get_device_name(0), calls_per_leg=calls, legs=legs,
               siren_rows_default=rows_default, kernel_vs_autograd_max_rel=agree,
               per_call={k: summary(v) for k, v in times.items()})
    t = {k: v["median_ms"] for k, v in res["per_call"].items()}
    spread = max(v["spread_ms"] for v in res["per_call"].values())
    res["kernel_vs_autograd"] = dict(gain_ms=t["autograd"] - t["kernel"], largest_spread_ms=spread,
                                     ratio=t["kernel"] / t["autograd"], beyond_spread=t["autograd"] - t["kernel"] > spread)
    res["kernel_over_forward"] = dict(default=t["kernel"] / t["forward"], lds_form=t["kernel"] / t["forward_lds"],
                                      cost_model_bound=float(slots(config["dim_in"])))
    res["ns_per_point"] = {k: v * 1e6 / n for k, v in t.items()}
    res["launches_per_call"] = {k: launches(fn) for k, fn in forms.items()}
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
    for config in NETS:
        res = measure(config, n)
        print(json.dumps(res, indent=1))
        path = os.path.join(out, profile_name(config, n))
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
        print("->", path)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
