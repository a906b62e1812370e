"""The reference's default HashMLP (BatchNorm + GELU decoder) per training step on the MI355X: the autograd
path (training_step + loss.backward() + Adam, BatchNorm in PyTorch ops) against FusedStep's BatchNorm plan:

    python tools/bn_time.py [batch ...]        (default: 10000 262144)

The model is config/base.py's HashConfig: V2 grid L4 F1 T2^23 (64,64,5) -> (352,352,15), decoder 4 -> 64 -> 1,
lr 5e-3.  Both paths run in one process on the same batch from the same initial state; after a warm-up the legs
alternate and each number is the median over the legs of a leg's mean step time (HIP events around `steps`
steps).  Writes profiles/r06_bn_b<batch>.json with both numbers, the fused step's phases (FusedStep.phase_ms)
and, for the three BatchNorm kernel groups, the bytes they move (the reads and writes DESIGN.md lists) over
their time."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mri_interpolation_amd import _lib, models, trainer  # noqa: E402

HASH_CONFIG = dict(dim_in=3, n_levels=4, n_features_per_level=1, log2_hashmap_size=23, base_resolution=(64, 64, 5),
                   finest_resolution=(352, 352, 15), dim_hidden=64, dim_out=1, n_layers=2, lr=5e-3)
# matrix passes (n x C floats, read or written) of each phase: bn_stats reads z; bn_fwd reads z, writes y;
# bn_bwd reads dy and z and writes g, then reads g and z and writes dz
PASSES = dict(bn_stats=1, bn_fwd=2, bn_bwd=6)


def leg_ms(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def measure(batch, warmup=20, steps=50, legs=7):
    torch.manual_seed(0)
    nets = [models.HashMLP(**HASH_CONFIG).cuda().train() for _ in range(2)]
    nets[1].load_state_dict(nets[0].state_dict())
    for net in nets:
        with torch.no_grad():
            net.encoder.table.uniform_(-0.5, 0.5)
    nets[1].encoder.table.data.copy_(nets[0].encoder.table.data)
    x = torch.rand(batch, 3, device="cuda")
    y = torch.rand(batch, 1, device="cuda")
    opt = nets[0].configure_optimizers()

    def autograd_step():
        opt.zero_grad()
        loss = nets[0].training_step((x, y), 0)
        loss.backward()
        opt.step()

    fused = trainer.FusedStep(nets[1], nets[1].configure_optimizers(), batch_norm=True)

    def fused_step():
        fused.train_step(x, y)

    for _ in range(warmup):
        autograd_step()
        fused_step()
    torch.cuda.synchronize()
    a_ms, f_ms = [], []
    for _ in range(legs):  # alternate, so that both see the same clocks and neighbours
        a_ms.append(leg_ms(autograd_step, steps))
        f_ms.append(leg_ms(fused_step, steps))
    res = dict(batch=batch, config={k: v for k, v in HASH_CONFIG.items()}, device=torch.cuda.get_device_name(0),
               steps_per_leg=steps, legs=legs, autograd_ms=statistics.median(a_ms), fused_ms=statistics.median(f_ms),
               autograd_legs_ms=a_ms, fused_legs_ms=f_ms)
    res["fused_over_autograd"] = res["fused_ms"] / res["autograd_ms"]
    fused.phase_events = {}
    for _ in range(20):
        fused_step()
    phases = fused.phase_ms()  # mean over the recorded brackets
    fused.phase_events = None
    blocks = len(fused.layers)
    per_block = ("mlp_fwd", "bn_stats", "bn_fwd", "bn_bwd")  # bracketed once per block: a step is blocks x the mean
    res["fused_phases_ms"] = {k: v * (blocks if k in per_block else 1) for k, v in phases.items()}
    res["fused_phases_note"] = ("ms per step, summed over the decoder blocks; mlp_bwd includes bn_bwd; an event "
                                "bracket includes its launch gaps")
    elems = batch * sum(l.weight.shape[0] for l in fused.layers)
    res["bn_streaming"] = {k: dict(bytes=4 * elems * p, ms=res["fused_phases_ms"][k],
                                   tb_per_s=4 * elems * p / (res["fused_phases_ms"][k] * 1e-3) / 1e12)
                           for k, p in PASSES.items()}
    return res


def main():
    batches = [int(a) for a in sys.argv[1:]] or [10000, 1 << 18]
    _lib.load()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    for batch in batches:
        res = measure(batch)
        print(json.dumps({k: v for k, v in res.items() if not k.endswith("legs_ms")}, indent=1))
        path = os.path.join(ROOT, "profiles", f"r06_bn_b{batch}.json")
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
        print("->", path)


if __name__ == "__main__":
    main()
