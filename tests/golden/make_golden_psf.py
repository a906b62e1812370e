#!/usr/bin/env python3
"""Golden vectors of the reference's PsfSirenNet (models.py:397-539), beside those of make_golden.py:

    python tests/golden/make_golden_psf.py

Same rules as make_golden.py (whose `import_reference` / `save` this script uses): the reference's own
`models.py`, unmodified, builds and runs the network; only its inputs and outputs are stored, and the
network weights are rebuilt from seeds with oracle.mlp.siren_init.
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

# half the voxel pitch of the sample volume (352 x 352 x 6) on the [-1, 1] axes: (2 / (s - 1)) / 2
SAMPLE_SPACING = (1.0 / 351.0, 1.0 / 351.0, 1.0 / 5.0)


def build(models, dim_in, hidden, n_layers, spacing, n_sample, seed):
    net = models.PsfSirenNet(dim_in=dim_in, dim_hidden=hidden, dim_out=1, n_layers=n_layers,
                             coordinates_spacing=spacing, n_sample=n_sample)
    layers = list(net.layers) + [net.last_layer]
    with torch.no_grad():
        for layer, (w, b) in zip(layers, omlp.siren_init(dim_in, hidden, 1, n_layers, seed)):
            layer.weight.copy_(w)
            layer.bias.copy_(b)
    return net, layers


def step_fixture(models, name, hidden, n_layers, n_sample, n, seed):
    net, layers = build(models, 3, hidden, n_layers, SAMPLE_SPACING, n_sample, seed)
    x = detrand.uniform(n * 3, seed + 1, -1.0, 1.0).reshape(n, 3)
    y = detrand.uniform(n, seed + 2, -1.0, 1.0).reshape(n, 1)
    xt, yt = torch.from_numpy(x), torch.from_numpy(y)
    loss = net.training_step((xt, yt), 0)
    loss.backward()
    with torch.no_grad():
        zbar = net.psf_conv(net(net.x_to_psf_x(xt)).T).T
    arrays = dict(x=x, y=y, psf_coordinates=net.psf_coordinates.numpy(),
                  psf_weight=net.psf_conv.weight.detach().numpy(), zbar=zbar.numpy(),
                  loss=np.float32(loss.item()))
    for i, layer in enumerate(layers):
        arrays[f"gw_{i}"] = layer.weight.grad.numpy().copy()
        arrays[f"gb_{i}"] = layer.bias.grad.numpy().copy()
    save(name, dict(dim_in=3, dim_hidden=hidden, n_layers=n_layers, n_sample=n_sample, seed=seed,
                    coordinates_spacing=list(SAMPLE_SPACING),
                    state_dict_keys=list(net.state_dict().keys())), **arrays)


def tables_fixture(models):
    """psf_coordinates / psf_conv.weight for n_sample 1, 3, 5 (the constructor alone)."""
    arrays = {}
    for ns in (1, 3, 5):
        net = models.PsfSirenNet(coordinates_spacing=SAMPLE_SPACING, n_sample=ns)
        arrays[f"coords_{ns}"] = net.psf_coordinates.numpy()
        arrays[f"weight_{ns}"] = net.psf_conv.weight.detach().numpy()
    save("psf_tables", dict(coordinates_spacing=list(SAMPLE_SPACING), n_samples=[1, 3, 5]), **arrays)


def adam_fixture(models):
    m = dict(dim_in=3, dim_hidden=64, n_layers=3, n_sample=3, seed=91, lr=1e-4, steps=3, n=256)
    net, layers = build(models, 3, m["dim_hidden"], m["n_layers"], SAMPLE_SPACING, m["n_sample"], m["seed"])
    opt = net.configure_optimizers()  # torch.optim.Adam over every parameter; psf_conv.weight has no grad
    arrays = dict(psf_weight=net.psf_conv.weight.detach().numpy().copy())
    for step in range(m["steps"]):
        x = detrand.uniform(m["n"] * 3, 920 + step, -1.0, 1.0).reshape(m["n"], 3)
        y = detrand.uniform(m["n"], 940 + step, -1.0, 1.0).reshape(m["n"], 1)
        opt.zero_grad()
        loss = net.training_step((torch.from_numpy(x), torch.from_numpy(y)), step)
        loss.backward()
        opt.step()
        arrays[f"x_{step}"], arrays[f"y_{step}"] = x, y
        arrays[f"loss_{step}"] = np.float32(loss.item())
        for i, layer in enumerate(layers):
            arrays[f"w_{step}_{i}"] = layer.weight.detach().numpy().copy()
            arrays[f"b_{step}_{i}"] = layer.bias.detach().numpy().copy()
    assert np.array_equal(net.psf_conv.weight.detach().numpy(), arrays["psf_weight"])
    save("e2e_psf_adam", dict(m, coordinates_spacing=list(SAMPLE_SPACING)), **arrays)


def main():
    _, models = import_reference()
    tables_fixture(models)
    step_fixture(models, "psf_siren_3d_4x64_ns5", 64, 4, 5, 64, 93)
    step_fixture(models, "psf_siren_3d_6x128_ns3", 128, 6, 3, 96, 94)
    adam_fixture(models)


if __name__ == "__main__":
    main()
