#!/usr/bin/env python3
"""Golden vectors of the reference's GaborNet with real Gabor layers (models.py:757-788, 836-885):

    python tests/golden/make_golden_gabor.py

Same rules as make_golden.py (whose `import_reference` / `save` this script uses): the reference's own `models.py`,
unmodified, builds `GaborNet(layer_cls=RealGaborLayer, ...)` and runs it on the CPU; only its inputs and outputs are
stored.

The weights are ours (the reference's constructor draws them from the global RNG): uniform on a grid of 256 values in
+-2^k, 2^k the power of two nearest to nn.Linear's bound 1 / sqrt(fan_in), so that the stored matrices compress
(tests/gabor_ref.py `grid_params`).  All fixtures use w0 = 5 and sigma = 1: a Gabor stack amplifies rounding by about
w0 per layer, and at the class defaults (30, 10) the reference's float32 forward is already 5e-3 from float64 -- a
fixture whose own values are that far from the function would hold no kernel to anything.  The script measures the
reference's float32 forward against float64 of the same ops on the same inputs (tests/gabor_ref.py), records it in
`meta` and aborts above MAX_REF_ERROR: a condition on the inputs, checked here, not a tolerance.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

from make_golden import import_reference, save  # noqa: E402

import gabor_ref  # noqa: E402
from oracle import detrand  # noqa: E402

MAX_REF_ERROR = 5e-6
ROWS = 192
W0, SIGMA = 5.0, 1.0
NAMES = ("wf", "bf", "ws", "bs")


def build(models, m):
    net = models.GaborNet(models.RealGaborLayer, m["dim_in"], m["dim_hidden"], 1, m["n_layers"], m["sigma"], m["w0"],
                          m.get("lr", 1e-4))
    params = gabor_ref.grid_params(m["dim_in"], m["dim_hidden"], m["n_layers"], m["seed"])
    with torch.no_grad():
        for lay, (wf, bf, ws, bs) in zip(net.layers, params):
            lay.freqs.weight.copy_(wf), lay.freqs.bias.copy_(bf)
            lay.scale.weight.copy_(ws), lay.scale.bias.copy_(bs)
    return net


def tensors(net):
    return [(l.freqs.weight, l.freqs.bias, l.scale.weight, l.scale.bias) for l in net.layers]


def parameters(net, tag=""):
    return {f"{k}_{tag}{i}": t.detach().numpy().copy() for i, p in enumerate(tensors(net)) for k, t in zip(NAMES, p)}


def reference_error(net, m, x):
    """max |f32 - f64| / max |f64| of the reference's forward on x."""
    with torch.no_grad():
        y32 = net(torch.from_numpy(x)).numpy().astype(np.float64)
        y64 = gabor_ref.forward(torch.from_numpy(x), [tuple(t.detach() for t in p) for p in tensors(net)], m["w0"],
                                m["sigma"]).numpy()
    err = float(np.abs(y32 - y64).max() / np.abs(y64).max())
    if err > MAX_REF_ERROR:
        raise SystemExit(f"the reference's float32 forward is {err:.2e} from float64 (> {MAX_REF_ERROR:g}): these inputs "
                         "make no fixture")
    return err


def step_arrays(net, x, y):
    """pred, loss, every parameter gradient and the gradient of pred.sum() with respect to x."""
    net.zero_grad()
    xt = torch.from_numpy(x).clone().requires_grad_(True)
    pred = net(xt)
    dx, = torch.autograd.grad(pred.sum(), xt, retain_graph=True)
    loss = torch.nn.functional.mse_loss(pred, torch.from_numpy(y))
    loss.backward()
    arrays = dict(x=x, y=y, pred=pred.detach().numpy().copy(), loss=np.float32(loss.item()), dx=dx.numpy().copy())
    arrays.update({f"g{k}_{i}": t.grad.numpy().copy() for i, p in enumerate(tensors(net)) for k, t in zip(NAMES, p)})
    return arrays


def meta_of(m, net, err):
    sd = net.state_dict()
    return dict(m, rows=ROWS, reference_f32_vs_f64=err, state_dict_keys=sorted(sd.keys()),
                shapes={k: list(v.shape) for k, v in sd.items()})


def inputs(m, k=0):
    x = detrand.uniform(ROWS * m["dim_in"], m["seed"] + 100 + 1000 * k, 0.0, 1.0).reshape(ROWS, m["dim_in"])
    y = detrand.uniform(ROWS, m["seed"] + 107 + 1000 * k, -1.0, 1.0).reshape(ROWS, 1)
    return x, y


def step_fixture(models, name, m):
    net = build(models, m)
    x, y = inputs(m)
    err = reference_error(net, m, x)
    arrays = parameters(net)
    arrays.update(step_arrays(net, x, y))
    save(name, meta_of(m, net, err), **arrays)


def adam_fixture(models):
    """Three Adam steps of the 2-D net: the parameters before, and per step the batch, the loss and every parameter
    after the step."""
    m = dict(dim_in=2, dim_hidden=64, n_layers=3, w0=W0, sigma=SIGMA, seed=93, lr=1e-4, steps=3)
    net = build(models, m)
    arrays = parameters(net)
    opt = net.configure_optimizers()
    err = 0.0
    for step in range(m["steps"]):
        x, y = inputs(m, step)
        err = max(err, reference_error(net, m, x))
        opt.zero_grad()
        loss = net.training_step((torch.from_numpy(x).clone(), torch.from_numpy(y)), step)
        loss.backward()
        opt.step()
        arrays[f"x_{step}"], arrays[f"y_{step}"] = x, y
        arrays[f"loss_{step}"] = np.float32(loss.item())
        arrays.update(parameters(net, f"{step}_"))
    save("e2e_gabor_adam", meta_of(m, net, err), **arrays)


def main():
    _, models = import_reference()
    step_fixture(models, "gabor_2d_3x64", dict(dim_in=2, dim_hidden=64, n_layers=3, w0=W0, sigma=SIGMA, seed=91))
    step_fixture(models, "gabor_3d_5x128", dict(dim_in=3, dim_hidden=128, n_layers=5, w0=W0, sigma=SIGMA, seed=92))
    adam_fixture(models)


if __name__ == "__main__":
    main()
