"""ModulatedSirenNet per training step on the MI355X, two ways:

    python tools/modsiren_time.py [--out DIR] [--fused-only STEPS] [batch ...]   (default: 262144 4096, DIR = profiles)

(a) the module path with autograd (training_step + loss.backward() + Adam: what Trainer() runs for this model),
(b) FusedStep(modulated=True), the kernel chain of csrc/modsiren.hip.  The model is the reference's own configuration
(config/base.py: dim_in 3, dim_hidden 128, n_layers 6).  Both run in one process on the same seeded rows from the same
initial state; after a warm-up of every shape the legs alternate and each number is the median over the legs of a
leg's mean step time (HIP events around `steps` steps, synchronised).  Kernel launches per step are counted with the
profiler on one step of each path.  Writes DIR/modsiren_b<batch>.json with the per-leg values, the fused step's
phases and the bytes per step computed from the shapes.
--fused-only STEPS runs nothing but STEPS fused steps at the first batch size (for a kernel trace of its own)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mri_interpolation_amd import _lib, models, trainer  # noqa: E402

CONFIG = dict(dim_in=3, dim_hidden=128, dim_out=1, n_layers=6, lr=1e-4)


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
    """Kernel launches of one call, as the profiler sees them on the device."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
             and not e.name.lower().startswith(("memcpy", "memset"))]
    return len(names)


def build(batch):
    torch.manual_seed(0)
    nets = [models.ModulatedSirenNet(**CONFIG).cuda().train() for _ in range(2)]
    nets[1].load_state_dict(nets[0].state_dict())
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(batch, CONFIG["dim_in"], generator=g) * 2 - 1).cuda()
    y = torch.rand(batch, 1, generator=g).cuda()
    return nets, x, y


def bytes_per_step(batch):
    """What the fused step must move through HBM, from the shapes: per layer four saved (n, H) tensors written once
    and read once (h_l twice: the ReLU mask and the next layer's weight gradient; a_l once for the weight gradient or
    the head), and for the L - 1 H x H layers dzs / dzm written once and read once."""
    H, L, d = CONFIG["dim_hidden"], CONFIG["n_layers"], CONFIG["dim_in"]
    nh = 4 * batch * H
    forward = 4 * L * nh + 4 * batch * (d + 3)
    backward = 3 * L * nh + nh + 2 * (L - 1) * nh + 4 * batch * (d + 1)
    wgrad = 4 * (L - 1) * nh
    return dict(forward=forward, backward=backward, weight_gradients=wgrad, total=forward + backward + wgrad)


def measure(batch, warmup=5, steps=10, legs=7):
    nets, x, y = build(batch)
    opt = nets[0].configure_optimizers()

    def autograd_step():
        opt.zero_grad()
        loss = nets[0].training_step((x, y), 0)
        loss.backward()
        opt.step()

    fused = trainer.FusedStep(nets[1], nets[1].configure_optimizers(), modulated=True)
    if not fused.use_modulated:
        raise RuntimeError("the modulated plan did not match")
    forms = dict(autograd=autograd_step, fused=lambda: fused.train_step(x, y))
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(legs):  # alternate, so that both forms see the same clocks and neighbours
        for k, fn in forms.items():
            times[k].append(leg_ms(fn, steps))
    res = dict(batch=batch, config=CONFIG, device=torch.cuda.get_device_name(0), steps_per_leg=steps, legs=legs,
               train={k: summary(v) for k, v in times.items()})
    a, f = res["train"]["autograd"], res["train"]["fused"]
    margin = max(a["spread_ms"], f["spread_ms"])
    res["fused_vs_autograd"] = dict(gain_ms=a["median_ms"] - f["median_ms"], larger_spread_ms=margin,
                                    ratio=f["median_ms"] / a["median_ms"],
                                    beyond_spread=a["median_ms"] - f["median_ms"] > margin)
    res["launches_per_step"] = {k: launches(fn) for k, fn in forms.items()}
    fused.phase_events = {}
    for _ in range(10):
        forms["fused"]()
    res["fused_phases_ms"] = fused.phase_ms()
    fused.phase_events = None
    res["bytes_per_step"] = bytes_per_step(batch)
    total_ms = res["fused_phases_ms"].get("mlp_fwd", 0.0) + res["fused_phases_ms"].get("mlp_bwd", 0.0)
    if total_ms > 0:
        res["hbm_tb_per_s"] = res["bytes_per_step"]["total"] / (total_ms * 1e-3) / 1e12
    return res


def main():
    argv = sys.argv[1:]
    out = os.path.join(ROOT, "profiles")
    if "--out" in argv:
        i = argv.index("--out")
        out = argv[i + 1]
        del argv[i:i + 2]
    fused_only = 0
    if "--fused-only" in argv:
        i = argv.index("--fused-only")
        fused_only = int(argv[i + 1])
        del argv[i:i + 2]
    batches = [int(a) for a in argv] or [1 << 18, 4096]
    _lib.load()
    if fused_only:
        nets, x, y = build(batches[0])
        fused = trainer.FusedStep(nets[1], nets[1].configure_optimizers(), modulated=True)
        for _ in range(fused_only):
            fused.train_step(x, y)
        torch.cuda.synchronize()
        print(json.dumps(dict(batch=batches[0], fused_steps=fused_only, loss=float(fused.loss))))
        return
    os.makedirs(out, exist_ok=True)
    for batch in batches:
        res = measure(batch)
        print(json.dumps(res, indent=1))
        path = os.path.join(out, f"modsiren_b{batch}.json")
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
        print("->", path)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
