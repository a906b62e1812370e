#!/usr/bin/env python3
"""Golden vectors of the reference's ModulatedSirenNet (models.py:236-322) for the fused coordinate gradient, beside
those of make_golden_modsiren.py:

    python tests/golden/make_golden_modsiren_gradient.py

Same rules as make_golden.py (whose `import_reference` / `save` this script uses, with `build` of
make_golden_modsiren.py): the reference's own `models.py`, unmodified, builds and runs the network on the CPU; only its
inputs and outputs are stored, and the network weights are rebuilt from seeds with oracle.mlp.siren_init /
modulator_init.  Each file holds x, y, pred, dydx -- the gradient of the reference's forward with respect to the
coordinates (autograd.grad(pred.sum(), x): the rows are independent) -- and dx, the reference's x.grad of its
training_step loss.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_golden import ROOT, import_reference, save  # noqa: E402,F401
from make_golden_modsiren import build  # noqa: E402

from oracle import detrand, mlp as omlp  # noqa: E402


def closest_kink(x, dim_in, hidden, n_layers, seed):
    """The smallest |modulator pre-activation| over the rows, in float64."""
    with torch.no_grad():
        mod64 = [(w.double(), b.double()) for w, b in omlp.modulator_init(dim_in, hidden, n_layers, seed + 500)]
        h, z, closest = torch.from_numpy(x).double(), torch.from_numpy(x).double(), np.inf
        for w, b in mod64:
            pm = torch.nn.functional.linear(h, w, b)
            closest = min(closest, float(pm.abs().min()))
            h = torch.cat((torch.relu(pm), z), dim=1)
    return closest


def fixture(models, name, dim_in, hidden, n_layers, n, seed):
    net, _, _ = build(models, dim_in, hidden, n_layers, seed)
    x = detrand.uniform(n * dim_in, seed + 1, -1.0, 1.0).reshape(n, dim_in)
    y = detrand.uniform(n, seed + 2, -1.0, 1.0).reshape(n, 1)
    # the fixture is only as good as its distance from the ReLU kinks: a pre-activation within rounding of zero makes
    # two correct f32 evaluations differ by a whole term, in the gradient by a whole column of a weight matrix
    closest = closest_kink(x, dim_in, hidden, n_layers, seed)
    assert closest >= 1e-6, f"{name}: a modulator pre-activation {closest:.3e} from zero, take another seed"
    xt = torch.from_numpy(x).clone().requires_grad_(True)
    pred = net(xt)
    dydx, = torch.autograd.grad(pred.sum(), xt)
    xt.grad = None
    loss = net.training_step((xt, torch.from_numpy(y)), 0)
    loss.backward()
    save(name, dict(dim_in=dim_in, dim_hidden=hidden, n_layers=n_layers, seed=seed, w0=30.0, w0_initial=30.0,
                    min_abs_preactivation=closest),
         x=x, y=y, pred=pred.detach().numpy(), dx=xt.grad.numpy(), dydx=dydx.numpy())


def main():
    _, models = import_reference()
    fixture(models, "modsiren_grad_3d_6x128", 3, 128, 6, 160, 169)  # the shape of the reference's config/base.py
    fixture(models, "modsiren_grad_2d_3x64", 2, 64, 3, 192, 166)


if __name__ == "__main__":
    main()
