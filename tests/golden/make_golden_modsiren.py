#!/usr/bin/env python3
"""Golden vectors of the reference's ModulatedSirenNet (models.py:236-322) for the fused modulated step, beside
those of make_golden.py (modsiren_2d, modsiren_3d):

    python tests/golden/make_golden_modsiren.py

Same rules as make_golden.py (whose `import_reference` / `save` this script uses): the reference's own `models.py`,
unmodified, builds and runs the network on the CPU; only its inputs and outputs are stored, and the network weights
are rebuilt from seeds with oracle.mlp.siren_init / modulator_init.
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


def build(models, dim_in, hidden, n_layers, seed, **kw):
    """The reference network with the weights of extra_models' seed scheme (siren: seed, modulator: seed + 500)."""
    net = models.ModulatedSirenNet(dim_in=dim_in, dim_hidden=hidden, dim_out=1, n_layers=n_layers, **kw)
    siren_layers = list(net.siren.layers) + [net.siren.last_layer]
    mod_layers = [seq[0] for seq in net.modulator.layers]
    with torch.no_grad():
        for layer, (w, b) in zip(siren_layers, omlp.siren_init(dim_in, hidden, 1, n_layers, seed)):
            layer.weight.copy_(w)
            layer.bias.copy_(b)
        for layer, (w, b) in zip(mod_layers, omlp.modulator_init(dim_in, hidden, n_layers, seed + 500)):
            layer.weight.copy_(w)
            layer.bias.copy_(b)
    return net, siren_layers, mod_layers


def step_fixture(models, name, dim_in, hidden, n_layers, n, seed):
    """One forward / loss / backward, the arrays of make_golden.py's modsiren fixtures."""
    net, siren_layers, mod_layers = build(models, dim_in, hidden, n_layers, seed)
    x = detrand.uniform(n * dim_in, seed + 1, -1.0, 1.0).reshape(n, dim_in)
    y = detrand.uniform(n, seed + 2, -1.0, 1.0).reshape(n, 1)
    pred = net(torch.from_numpy(x).clone())  # the reference multiplies in place
    loss = torch.nn.functional.mse_loss(torch.from_numpy(y), pred)
    loss.backward()
    arrays = dict(x=x, y=y, pred=pred.detach().numpy(), loss=np.float32(loss.item()))
    for i, layer in enumerate(siren_layers):
        arrays[f"siren_gw_{i}"] = layer.weight.grad.numpy().copy()
        arrays[f"siren_gb_{i}"] = layer.bias.grad.numpy().copy()
    for i, layer in enumerate(mod_layers):
        arrays[f"mod_gw_{i}"] = layer.weight.grad.numpy().copy()
        arrays[f"mod_gb_{i}"] = layer.bias.grad.numpy().copy()
    # the fixture is only as good as its distance from the ReLU kinks: a pre-activation within rounding of zero
    # makes two correct f32 evaluations differ by a whole term
    with torch.no_grad():
        mod64 = [(w.double(), b.double()) for w, b in omlp.modulator_init(dim_in, hidden, n_layers, seed + 500)]
        h, z, closest = torch.from_numpy(x).double(), torch.from_numpy(x).double(), np.inf
        for w, b in mod64:
            pm = torch.nn.functional.linear(h, w, b)
            closest = min(closest, float(pm.abs().min()))
            h = torch.cat((torch.relu(pm), z), dim=1)
    assert closest >= 1e-6, f"{name}: a modulator pre-activation {closest:.3e} from zero, take another seed"
    save(name, dict(dim_in=dim_in, dim_hidden=hidden, n_layers=n_layers, seed=seed, w0=30.0, w0_initial=30.0,
                    min_abs_preactivation=closest, state_dict_keys=sorted(net.state_dict().keys())), **arrays)


def adam_fixture(models):
    """Three Adam steps: inputs, loss and every parameter after each step (the dead default stack included in the
    optimiser, as `configure_optimizers` builds it over every parameter)."""
    m = dict(dim_in=3, dim_hidden=64, n_layers=3, seed=67, lr=1e-4, steps=3, n=256)
    net, siren_layers, mod_layers = build(models, m["dim_in"], m["dim_hidden"], m["n_layers"], m["seed"], lr=m["lr"])
    opt = net.configure_optimizers()
    arrays = {}
    for step in range(m["steps"]):
        x = detrand.uniform(m["n"] * m["dim_in"], 670 + step, -1.0, 1.0).reshape(m["n"], m["dim_in"])
        y = detrand.uniform(m["n"], 680 + step, -1.0, 1.0).reshape(m["n"], 1)
        opt.zero_grad()
        loss = net.training_step((torch.from_numpy(x).clone(), torch.from_numpy(y)), step)
        loss.backward()
        opt.step()
        arrays[f"x_{step}"], arrays[f"y_{step}"] = x, y
        arrays[f"loss_{step}"] = np.float32(loss.item())
        for i, layer in enumerate(siren_layers):
            arrays[f"siren_w_{step}_{i}"] = layer.weight.detach().numpy().copy()
            arrays[f"siren_b_{step}_{i}"] = layer.bias.detach().numpy().copy()
        for i, layer in enumerate(mod_layers):
            arrays[f"mod_w_{step}_{i}"] = layer.weight.detach().numpy().copy()
            arrays[f"mod_b_{step}_{i}"] = layer.bias.detach().numpy().copy()
    save("e2e_modsiren_adam", dict(m, w0=30.0, w0_initial=30.0), **arrays)


def main():
    _, models = import_reference()
    step_fixture(models, "modsiren_3d_6x128", 3, 128, 6, 160, 65)  # the shape of the reference's config/base.py
    adam_fixture(models)


if __name__ == "__main__":
    main()
