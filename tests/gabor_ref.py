"""The GaborNet op sequence of the reference (models.py:784-788, 866-867) restated in plain PyTorch on the CPU, in any
dtype: the float64 evaluation on the float32 inputs is the yardstick's third leg (tests/yardstick.py), the float32
evaluation is the reference's own arithmetic.  Pure host code: used by the tests, tests/golden/make_golden_gabor.py
and tools/gabor_time.py (which runs the same ops on the GPU as its project-free leg).

    omega = w0 * freqs(a)        scale = scale(a) * c        a' = cos(omega) * exp(-(scale ** 2))

`params`: one (freqs.weight, freqs.bias, scale.weight, scale.bias) tuple per layer, the head last.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import detrand


def layer(h, wf, bf, ws, bs, w0, c):
    omega = w0 * F.linear(h, wf, bf)
    scale = F.linear(h, ws, bs) * c
    return torch.cos(omega) * torch.exp(-(scale ** 2))


def forward(x, params, w0, c, dtype=torch.float64):
    """y (n, dim_out) of the stack in `dtype`; differentiable when x or the parameters ask for it."""
    h = x.to(dtype)
    for p in params:
        h = layer(h, *[t.to(dtype) for t in p], w0, c)
    return h


def grid_values(shape, fan_in, seed):
    """Uniform on the grid k 2^e / 128, k = -128 .. 127, 2^e the power of two nearest to nn.Linear's own bound
    1 / sqrt(fan_in): 256 values, so the stored matrices compress."""
    bound = 2.0 ** round(math.log2(1.0 / math.sqrt(fan_in)))
    k = detrand.integers(int(np.prod(shape)), seed, -128, 128).astype(np.float32)
    return torch.from_numpy((k * np.float32(bound / 128.0)).reshape(shape))


def grid_params(dim_in, hidden, n_layers, seed, dim_out=1):
    params = []
    for i in range(n_layers):
        fan_in, fan_out = (dim_in if i == 0 else hidden), (dim_out if i == n_layers - 1 else hidden)
        params.append(tuple(grid_values(shape, fan_in, seed + 10 * i + j)
                            for j, shape in enumerate([(fan_out, fan_in), (fan_out,), (fan_out, fan_in), (fan_out,)], 1)))
    return params


def uniform(shape, seed, lo=0.0, hi=1.0):
    return torch.from_numpy(detrand.uniform(int(np.prod(shape)), seed, lo, hi).reshape(shape).copy())


def fixture_params(fx, prefix="", n_layers=None):
    n_layers = fx.meta["n_layers"] if n_layers is None else n_layers
    return [tuple(torch.from_numpy(fx[f"{k}_{prefix}{i}"]) for k in ("wf", "bf", "ws", "bs")) for i in range(n_layers)]


def step(x, y, params, w0, c, dtype=torch.float64):
    """(pred, loss, d pred.sum() / dx, [gradients of F.mse_loss(pred, y) in the order of `params`, flattened])."""
    xg = x.to(dtype).clone().requires_grad_(True)
    ps = [tuple(t.to(dtype).clone().requires_grad_(True) for t in p) for p in params]
    pred = forward(xg, ps, w0, c, dtype)
    dx, = torch.autograd.grad(pred.sum(), xg, retain_graph=True)
    loss = F.mse_loss(pred, y.to(dtype))
    grads = torch.autograd.grad(loss, [t for p in ps for t in p])
    return pred.detach(), loss.detach(), dx, list(grads)
