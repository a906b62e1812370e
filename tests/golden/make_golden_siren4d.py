#!/usr/bin/env python3
"""Golden vectors of the reference's SirenNet (models.py:108-233) on FOUR input axes -- a dynamic volume, time
among the coordinates --, beside the SIREN fixtures of make_golden.py:

    python tests/golden/make_golden_siren4d.py

Same rules as make_golden.py (whose `import_reference` / `save` this script uses): the reference's own
`models.py`, unmodified, builds and runs the network; only its inputs and outputs are stored, and the
network weights are rebuilt from seeds with oracle.mlp.siren_init.  Beside what the 2-D / 3-D SIREN fixtures
hold (x, y, pred, the reference's x.grad of its training_step loss as dx) each file holds dydx, the gradient of
the reference's forward with respect to the coordinates (autograd.grad(pred.sum(), x): the rows are independent).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_golden import ROOT, import_reference, save  # noqa: E402,F401

from oracle import detrand, mlp as omlp  # noqa: E402

DIM_IN = 4


def fixture(models, name, hidden, n_layers, n, seed):
    net = models.SirenNet(dim_in=DIM_IN, dim_hidden=hidden, dim_out=1, n_layers=n_layers)
    with torch.no_grad():
        for layer, (w, b) in zip(list(net.layers) + [net.last_layer], omlp.siren_init(DIM_IN, hidden, 1, n_layers, seed)):
            layer.weight.copy_(w)
            layer.bias.copy_(b)
    x = detrand.uniform(n * DIM_IN, seed + 1, -1.0, 1.0).reshape(n, DIM_IN)
    for row, v in zip((n // 2, n - 1, 0), (-1.0, 0.0, 1.0)):  # the ends and the middle of every axis
        x[row] = v
    y = detrand.uniform(n, seed + 2, -1.0, 1.0).reshape(n, 1)
    xt = torch.from_numpy(x).requires_grad_(True)
    pred = net(xt)
    dydx, = torch.autograd.grad(pred.sum(), xt, retain_graph=True)
    loss = net.training_step((xt, torch.from_numpy(y)), 0)
    loss.backward()
    save(name, dict(dim_in=DIM_IN, dim_hidden=hidden, n_layers=n_layers, seed=seed, w0=30.0, w0_initial=30.0),
         x=x, y=y, pred=pred.detach().numpy(), dx=xt.grad.numpy(), dydx=dydx.numpy())


def main():
    _, models = import_reference()
    fixture(models, "siren_4d_4x64", 64, 4, 96, 71)
    fixture(models, "siren_4d_3x256", 256, 3, 40, 72)


if __name__ == "__main__":
    main()
