#!/usr/bin/env python3
"""Golden vectors of the reference's RffNet (models.py:542-584: Gaussian Fourier features, then a ReLU MLP with the
activation behind every Linear):

    python tests/golden/make_golden_rff.py

Same rules as make_golden.py (whose `import_reference` / `save` this script uses): the reference's own `models.py`,
unmodified, builds and runs the network on the CPU; only its inputs and outputs are stored.  The `rff` package is not
installed anywhere, so `rff.layers.GaussianEncoding` is a stand-in written here from the package's documented formula:
b = randn(encoded_size, input_size) * sigma as a frozen parameter, vp = 2 * np.pi * v @ b.T, cat((cos(vp), sin(vp)), -1).

The weights are ours (the reference's constructor draws them from the global RNG): uniform on a grid of 256 values in
+-2^k, 2^k the power of two nearest to He's bound sqrt(6 / fan_in), so that pre-activations are O(1) through the depth
and the stored matrices compress.  ReLU makes every gradient jump where a pre-activation crosses zero, so the input
seed is searched until the smallest |pre-activation| over all layers and rows, evaluated in float64, is >= 1e-5; the
value and the seed are recorded in `meta`.  That is a condition on the input, checked here, not a tolerance.
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_golden import import_reference, save  # noqa: E402

from oracle import detrand  # noqa: E402

MIN_PREACT = 1e-5
ROWS = 192


class GaussianEncoding(torch.nn.Module):
    """Stand-in for rff.layers.GaussianEncoding(sigma, input_size, encoded_size)."""

    def __init__(self, sigma=None, input_size=None, encoded_size=None, b=None):
        super().__init__()
        if b is None:
            b = torch.randn((encoded_size, input_size)) * sigma
        self.b = torch.nn.parameter.Parameter(b, requires_grad=False)

    def forward(self, v):
        vp = 2 * np.pi * v @ self.b.T
        return torch.cat((torch.cos(vp), torch.sin(vp)), dim=-1)


def grid_weights(shape, fan_in, seed):
    bound = 2.0 ** round(math.log2(math.sqrt(6.0 / fan_in)))
    k = detrand.integers(int(np.prod(shape)), seed, -128, 128).astype(np.float32)
    return torch.from_numpy((k * np.float32(bound / 128.0)).reshape(shape))


def build(models, m):
    torch.manual_seed(m["seed"])  # the stand-in's randn: b
    net = models.RffNet(dim_in=m["dim_in"], dim_hidden=m["dim_hidden"], dim_out=1, n_layers=m["n_layers"],
                        n_frequencies=m["n_frequencies"], sigma=m["sigma"], lr=m.get("lr", 1e-4))
    linears = [l for l in net.decoder if isinstance(l, torch.nn.Linear)]
    with torch.no_grad():
        for i, lin in enumerate(linears):
            lin.weight.copy_(grid_weights(tuple(lin.weight.shape), lin.in_features, m["seed"] + 10 * i + 1))
            lin.bias.copy_(grid_weights(tuple(lin.bias.shape), 6 * 64, m["seed"] + 10 * i + 2))  # +-2^-3
    return net, linears


def min_preactivation(net, linears, x):
    """Smallest |pre-activation| over all Linears and rows, the op sequence in float64 on the float32 inputs."""
    with torch.no_grad():
        vp = (float(np.float32(2 * np.pi)) * torch.from_numpy(x).double()) @ net.encoder.b.double().T
        h, closest = torch.cat((torch.cos(vp), torch.sin(vp)), dim=-1), np.inf
        for lin in linears:
            p = torch.nn.functional.linear(h, lin.weight.double(), lin.bias.double())
            closest = min(closest, float(p.abs().min()))
            h = torch.relu(p)
    return closest, float((h > 0).double().mean())


def draw(m, net, linears, first_seed, batches=1):
    """The first input seed >= first_seed whose `batches` consecutive batches all keep MIN_PREACT (and a head that is
    alive on a quarter of the rows)."""
    for seed in range(first_seed, first_seed + 4000):
        xs = [detrand.uniform(ROWS * m["dim_in"], seed + 1000 * k, 0.0, 1.0).reshape(ROWS, m["dim_in"])
              for k in range(batches)]
        found = [min_preactivation(net, linears, x) for x in xs]
        if all(c >= MIN_PREACT and alive >= 0.25 for c, alive in found):
            return seed, xs, min(c for c, _ in found)
    raise SystemExit("no input seed keeps the pre-activations clear of zero")


def parameters(net, linears):
    arrays = dict(b=net.encoder.b.detach().numpy().copy())
    for i, lin in enumerate(linears):
        arrays[f"w_{i}"] = lin.weight.detach().numpy().copy()
        arrays[f"b_{i}"] = lin.bias.detach().numpy().copy()
    return arrays


def step_arrays(net, linears, x, y):
    """pred, loss, every parameter gradient and the gradient of pred.sum() with respect to x."""
    for lin in linears:
        lin.weight.grad = lin.bias.grad = None
    xt = torch.from_numpy(x).clone().requires_grad_(True)
    pred = net(xt)
    dx, = torch.autograd.grad(pred.sum(), xt, retain_graph=True)
    loss = torch.nn.functional.mse_loss(torch.from_numpy(y), pred)
    loss.backward()
    arrays = dict(x=x, y=y, pred=pred.detach().numpy().copy(), loss=np.float32(loss.item()), dx=dx.numpy().copy())
    for i, lin in enumerate(linears):
        arrays[f"gw_{i}"] = lin.weight.grad.numpy().copy()
        arrays[f"gb_{i}"] = lin.bias.grad.numpy().copy()
    assert net.encoder.b.grad is None and not net.encoder.b.requires_grad
    return arrays


def meta_of(m, net, seed_x, closest):
    keys = sorted(net.state_dict().keys())
    return dict(m, seed_x=seed_x, min_abs_preactivation=closest, rows=ROWS,
                state_dict_keys=[k for k in keys if not k.startswith("layers.")],
                dead_keys=[k for k in keys if k.startswith("layers.")],
                shapes={k: list(v.shape) for k, v in net.state_dict().items() if not k.startswith("layers.")})


def step_fixture(models, name, m):
    net, linears = build(models, m)
    seed_x, (x,), closest = draw(m, net, linears, m["seed"] + 100)
    y = detrand.uniform(ROWS, seed_x + 7, 0.0, 1.0).reshape(ROWS, 1)
    arrays = parameters(net, linears)
    arrays.update(step_arrays(net, linears, x, y))
    save(name, meta_of(m, net, seed_x, closest), **arrays)


def adam_fixture(models):
    """Three Adam steps of the 2-D net: the parameters before, and per step the batch, the loss and every parameter
    after the step (`configure_optimizers` hands Adam every parameter, the frozen b and the dead default stack
    included: they never have a gradient and never move)."""
    m = dict(dim_in=2, dim_hidden=64, n_frequencies=64, n_layers=3, sigma=10.0, seed=83, lr=1e-4, steps=3)
    net, linears = build(models, m)
    seed_x, xs, closest = draw(m, net, linears, m["seed"] + 100, batches=m["steps"])
    arrays = parameters(net, linears)
    opt = net.configure_optimizers()
    b_before = net.encoder.b.detach().clone()
    for step, x in enumerate(xs):
        y = detrand.uniform(ROWS, seed_x + 7 + 1000 * step, 0.0, 1.0).reshape(ROWS, 1)
        if step == 0:
            arrays.update({k + "_first": v for k, v in step_arrays(net, linears, x, y).items() if k not in ("x", "y")})
        opt.zero_grad()
        loss = net.training_step((torch.from_numpy(x).clone(), torch.from_numpy(y)), step)
        loss.backward()
        opt.step()
        arrays[f"x_{step}"], arrays[f"y_{step}"] = x, y
        arrays[f"loss_{step}"] = np.float32(loss.item())
        for i, lin in enumerate(linears):
            arrays[f"w_{step}_{i}"] = lin.weight.detach().numpy().copy()
            arrays[f"b_{step}_{i}"] = lin.bias.detach().numpy().copy()
    assert torch.equal(net.encoder.b, b_before)
    save("e2e_rff_adam", meta_of(m, net, seed_x, closest), **arrays)


def main():
    _, models = import_reference()
    sys.modules["rff.layers"].GaussianEncoding = GaussianEncoding
    step_fixture(models, "rff_2d_3x64", dict(dim_in=2, dim_hidden=64, n_frequencies=64, n_layers=3, sigma=10.0, seed=81))
    step_fixture(models, "rff_3d_6x128", dict(dim_in=3, dim_hidden=128, n_frequencies=128, n_layers=6, sigma=10.0,
                                              seed=82))
    adam_fixture(models)


if __name__ == "__main__":
    main()
