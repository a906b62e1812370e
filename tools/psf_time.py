"""PsfSirenNet's fused training step against the plain SirenNet FusedStep on the same n S rows and the same
chain shape (MI355X):  python tools/psf_time.py [n] [n_sample] [hidden] [n_layers]

Defaults: the launcher's BaseConfig, n = 4096 targets, n_sample = 3 (S = 27), 6 x 128.  Writes
profiles/r05_psf_n<n>_ns<n_sample>_<n_layers>x<hidden>.json: milliseconds per step (median of the repeats,
HIP events) of
  psf           FusedStep.train_step of PsfSirenNet on n targets (expand, chain forward, PSF loss, chain backward, Adam)
  plain         FusedStep.train_step of SirenNet on n S rows (its default: loss and head fused into the forward kernel)
  plain_unfused the same with the separate loss kernel (chain_loss = False): the kernels the PSF step runs
and the PSF step's phases."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mri_interpolation_amd import _lib, models, trainer  # noqa: E402


def median_ms(fn, warmup=5, reps=30):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def main():
    args = [int(a) for a in sys.argv[1:]]
    n, ns, hidden, n_layers = (args + [4096, 3, 128, 6][len(args):])[:4]
    _lib.load()
    torch.manual_seed(0)
    psf = models.PsfSirenNet(3, hidden, 1, n_layers, coordinates_spacing=(1 / 351, 1 / 351, 1 / 5),
                             n_sample=ns).cuda()
    S = psf.n_psf
    siren = models.SirenNet(3, hidden, 1, n_layers).cuda()
    siren.load_state_dict({k: v for k, v in psf.state_dict().items() if k != "psf_conv.weight"})
    x = torch.rand(n, 3, device="cuda") * 2 - 1
    y = torch.rand(n, 1, device="cuda") * 2 - 1
    xs = psf.x_to_psf_x(x).detach().contiguous()
    ys = torch.rand(n * S, 1, device="cuda") * 2 - 1
    ps = trainer.FusedStep(psf, psf.configure_optimizers())
    ss = trainer.FusedStep(siren, siren.configure_optimizers())
    assert ps.use_chain and ss.use_chain and ps.psf is not None
    res = dict(n=n, n_sample=ns, S=S, rows=n * S, hidden=hidden, n_layers=n_layers,
               device=torch.cuda.get_device_name(0))
    res["psf_ms"] = median_ms(lambda: ps.train_step(x, y))
    res["plain_ms"] = median_ms(lambda: ss.train_step(xs, ys))
    ss.chain_loss = False
    res["plain_unfused_ms"] = median_ms(lambda: ss.train_step(xs, ys))
    res["psf_over_plain"] = res["psf_ms"] / res["plain_ms"] - 1
    res["psf_over_plain_unfused"] = res["psf_ms"] / res["plain_unfused_ms"] - 1
    ps.phase_events = {}
    median_ms(lambda: ps.train_step(x, y), warmup=0, reps=10)
    res["psf_phases_ms"] = ps.phase_ms()
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    path = os.path.join(ROOT, "profiles", f"r05_psf_n{n}_ns{ns}_{n_layers}x{hidden}.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("->", path)


if __name__ == "__main__":
    main()
