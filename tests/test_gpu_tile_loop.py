"""The persistent tile loop of the six chain kernels (csrc/chain_tile.h) PAST A WORKGROUP'S FIRST TILE, on the GPU.

At most 256 workgroups walk the tiles, so a workgroup reaches a second tile only when n > T = 256 R (R: tests/tile_loop.py,
held to the library by tests/test_tile_loop_cpu.py).  Across a tile boundary travel the weight prefetch
(`tile + gridDim.x < tiles`), the parity of the weight buffer (`s & 1` runs on), the pending activation stores
(pend_l / pend_m0), the workgroup's running sums (g_wh, g_bl, g_loss, g_bh, first_tile) and the LDS images, which only the
barrier at a tile's top keeps apart.  A mistake there gives the same wrong bits on every run: the reproducibility tests
cannot see it.  Every case runs at n = T, T + 1, T + R + 3 and 2 T + R + 3 (tile_loop.batch_sizes) and asserts

  (a) float64: y, the loss, every gradient AND every saved per-row buffer, layer by layer, against the float64
      evaluation on the CPU -- the SIREN chain at REL_TOL, the modulated chain by test_gpu_modsiren.close_or_no_worse,
      the coordinate gradients by yardstick.assert_no_worse;
  (b) cut: the whole launch against two launches cut at a tile boundary (rows [0, T) -- one tile per workgroup, what the
      older tests hold to float64 -- and [T, n); n = T: cut at T / 2), n_total = n in both.  Nothing a row computes
      depends on its tile or on n, so y, dy and every per-row buffer are BIT-identical; the summed gradients and the loss
      differ in summation order alone and are held to 2e-6 (the bar of test_gpu_rows.py between two orders);
  (c) tail only: the gradients again with dLoss/dy zero on the rows in front of the cut (dy zeroed, or target = y there),
      against the float64 gradient of the loss of the other rows: a sum over 65 thousand rows hides one tile's error.

Coordinates are uniform in [-1, 1], targets in [0, 1] (tile_loop.intensities says why).  A buffer a kernel has to fill
starts as NaN.  The first run of (b) found the float32 chain of csrc/siren_chain.hip's slab_sum_kernel (H x H weight
gradients, 3.7e-6 between the whole launch and the two at hidden 32), not the tile loop; the kernel says what it does now.

Which test holds a kernel's second tile to a reference:

  siren_forward_kernel<1> (act / deriv stored), siren_backward_kernel      test_siren_chain, training form
  siren_forward_kernel<2> (loss in the forward), backward with head_done   test_siren_chain, loss form (n_sine >= 2)
  siren_forward_kernel<0> (inference)                                      test_siren_chain, inference
      hidden 32, 64, 128 with 1, 2, 3 sine layers; hidden 256 with 1 layer, and with 3 under option siren_rows = 0
  modsiren_forward_kernel<true>, modsiren_backward_kernel                  test_modsiren_chain
  modsiren_forward_kernel<false> (inference)                               test_modsiren_chain (bits of the training y)
  siren_gradient_kernel, four and eight slots, hidden 256 / 128 / 64 / 32  test_siren_gradient
  modsiren_gradient_kernel                                                 test_modsiren_gradient (T and T + 1; 256 P + 5
                                                                           is test_gpu_modsiren_gradient.py's)
  siren_rows.hip (hidden 256, a loop of its own)                           test_gpu_rows.py (n = 70001)
"""
import functools

import numpy as np
import pytest
import torch

from conftest import REL_TOL, rel_err
from test_gpu_modsiren import close_or_no_worse, kernel_loss_and_grads, selected_rows  # (selected_rows: two ModRef)
from test_gpu_modsiren_gradient import case as mod_gradient_case, kernel as mod_gradient_kernel
from test_gpu_siren_gradient import case as gradient_case, kernel as gradient_kernel
from tile_loop import (GRID_BLOCKS, MOD_GRAD_POINTS, MOD_ROWS, SIREN_ROWS, SIZE_NAMES, W0, batch_sizes, intensities,
                       mod_reference, siren_float64, siren_grad_points, uniform)
from yardstick import assert_no_worse
from oracle import mlp as omlp

pytestmark = pytest.mark.gpu

ORDER_TOL = 2e-6  # two summation orders of the same float32 terms (tests/test_gpu_rows.py)


@pytest.fixture(scope="module")
def amd():
    from mri_interpolation_amd import _lib, ops
    assert torch.cuda.is_available(), "these tests need the GPU"
    _lib.load()
    return type("NS", (), dict(lib=_lib, ops=ops))


def cut_of(n, rows):
    """Where the two launches of (b) meet, and where the tail of (c) starts: T; T / 2 when n = T."""
    t = GRID_BLOCKS * rows
    assert n >= t and t % (2 * rows) == 0
    return t if n > t else t // 2


def nan(*shape):
    """A buffer the kernel has to fill: a row it misses fails (a) and (b) alike."""
    return torch.full(shape, float("nan"), device="cuda")


def views(tensors, lo, hi):
    return [None if t is None else t[lo:hi] for t in tensors]


def same_bits(whole, cut, what):
    for i, (a, b) in enumerate(zip(whole, cut)):
        if a is None:
            assert b is None
            continue
        if not torch.equal(a, b):
            bad = torch.nonzero((a != b).reshape(a.shape[0], -1).any(dim=1)).reshape(-1)
            raise AssertionError(f"{what}[{i}]: the whole launch and the two launches cut at a tile boundary differ in "
                                 f"{bad.numel()} rows, the first {int(bad[0])}, the last {int(bad[-1])}")


def hold(kernel, f64, what, tol=REL_TOL):
    e_max, e_l2 = rel_err(kernel.detach().cpu().numpy(), f64.detach().cpu().numpy())
    print(f"tile loop {what}: {e_max:.2e} / {e_l2:.2e}")
    assert e_max <= tol and e_l2 <= tol, f"{what}: rel-to-max {e_max:.3e}, rel-L2 {e_l2:.3e} > {tol}"


def hold_scalar(kernel, want, what, tol=REL_TOL):
    """The rule of test_siren_chain_matches_oracle_and_layerwise for a loss."""
    print(f"tile loop {what}: {abs(kernel - want) / max(abs(want), 0.1):.2e}")
    assert abs(kernel - want) <= tol * max(abs(want), 0.1), f"{what}: {kernel!r} against {want!r}"


def hold_range(kernel, f64, what):
    """... and for predictions: relative to the output range."""
    err = float((kernel.detach().cpu().double() - f64).abs().max()) / max(float(f64.abs().max()), 0.1)
    print(f"tile loop {what}: {err:.2e}")
    assert err <= REL_TOL, f"{what}: {err:.3e} of the output range"


# ================================================================================================ 1. the SIREN chain
SIREN_CASES = [  # hidden, dim_in, n_sine: 1 layer streams no weights, 2 give more_l false, 3 walk layers both ways
    (32, 1, 1), (32, 3, 2), (32, 8, 3), (64, 3, 1), (64, 8, 2), (64, 1, 3), (128, 8, 1), (128, 1, 2), (128, 3, 3),
    (256, 3, 1),   # one sine layer: the image kernels serve hidden 256 by default
    (256, 3, 3),   # under option siren_rows = 0
]


class SirenChain:
    """The ops-level calls on one network and batch; `cuts`: the row ranges, one launch each."""

    def __init__(self, ops, params, x, target):
        self.ops = ops
        self.w, self.b = [w.cuda() for w, _ in params], [b.cuda() for _, b in params]
        self.x, self.t = x.cuda(), target.cuda()
        self.n, self.H, self.L = x.shape[0], params[0][0].shape[0], len(params) - 1

    def per_row(self, count):
        return [nan(self.n, self.H) for _ in range(count)]

    def zero_grads(self):
        return [torch.zeros_like(t) for t in self.w], [torch.zeros_like(t) for t in self.b]

    def forward(self, cuts, act=None, deriv=None):
        y = nan(self.n, 1)
        for lo, hi in cuts:
            self.ops.siren_forward(self.x[lo:hi], self.w, self.b, W0, W0, act=act and views(act, lo, hi),
                                   deriv=deriv and views(deriv, lo, hi), y=y[lo:hi])
        return y

    def backward(self, cuts, dy, act, deriv):
        """siren_backward(head_done=False) on zeroed gradients: dz, (gw, gb)."""
        dz, (gw, gb) = [None] + self.per_row(self.L - 1), self.zero_grads()
        for lo, hi in cuts:
            self.ops.siren_backward(self.x[lo:hi], dy[lo:hi], self.w, views(act, lo, hi), views(deriv, lo, hi),
                                    views(dz, lo, hi), gw, gb)
        return dz, gw, gb

    def loss_form(self, cuts, target):
        """siren_forward_loss + siren_backward(head_done=True) per range, n_total = n, on zeroed gradients."""
        L = self.L
        act, deriv = self.per_row(L - 1) + [None], self.per_row(L - 1) + [None]  # the last layer's stay on chip
        dz, (gw, gb) = [None] + self.per_row(L - 1), self.zero_grads()
        y, loss = nan(self.n, 1), torch.zeros(1, device="cuda")
        for lo, hi in cuts:
            a, d, z = views(act, lo, hi), views(deriv, lo, hi), views(dz, lo, hi)
            self.ops.siren_forward_loss(self.x[lo:hi], target[lo:hi], self.w, self.b, W0, W0, a, d, z[-1], y[lo:hi],
                                        gw[L], gb[L], gb[L - 1], loss, n_total=self.n)
            self.ops.siren_backward(self.x[lo:hi], None, self.w, a, d, z, gw, gb, head_done=True)
        return dict(y=y, loss=float(loss), act=act, deriv=deriv, dz=dz, gw=gw, gb=gb)


def hold_grads(gw, gb, want, what, tol=REL_TOL):
    for i, (w, b) in enumerate(zip(gw, gb)):
        hold(w, want[2 * i], f"{what} gw{i}", tol)
        hold(b, want[2 * i + 1], f"{what} gb{i}", tol)


def siren_chain_case(ops, hidden, dim_in, n_sine, n):
    cut = cut_of(n, SIREN_ROWS[hidden])
    whole, two = [(0, n)], [(0, cut), (cut, n)]
    seed = 7000 + hidden + 10 * n_sine + dim_in
    params = omlp.siren_init(dim_in, hidden, 1, n_sine, seed)
    x, target = uniform(n, dim_in, seed + 1), intensities(n, seed + 2)
    f64 = siren_float64(params, x, target, cut)
    k = SirenChain(ops, params, x, target)
    tag = f"siren {dim_in} -> {hidden} x {n_sine}, n = {n}:"

    # ---- inference
    y_inf = k.forward(whole)
    hold_range(y_inf, f64["y"], f"{tag} inference y")
    same_bits([y_inf], [k.forward(two)], f"{tag} inference y")

    # ---- training form: siren_forward with act / deriv, mri_mse_loss, siren_backward(head_done=False)
    act, deriv = k.per_row(n_sine), k.per_row(n_sine)
    y = k.forward(whole, act, deriv)
    loss, dy = torch.zeros(1, device="cuda"), nan(n, 1)
    ops.mse_loss(y, k.t, loss, dy)
    dz, gw, gb = k.backward(whole, dy, act, deriv)
    hold_range(y, f64["y"], f"{tag} training y")
    hold_scalar(float(loss), f64["loss"], f"{tag} training loss")
    for l in range(n_sine):
        hold(act[l], f64["act"][l], f"{tag} training act[{l}]")
        hold(deriv[l], f64["deriv"][l], f"{tag} training deriv[{l}]")
        if l >= 1:
            hold(dz[l], f64["dz"][l], f"{tag} training dz[{l}]")
    hold_grads(gw, gb, f64["grads"], f"{tag} training")
    act2, deriv2 = k.per_row(n_sine), k.per_row(n_sine)
    same_bits([y], [k.forward(two, act2, deriv2)], f"{tag} training y")
    same_bits(act + deriv, act2 + deriv2, f"{tag} training act / deriv")
    dz2, gw2, gb2 = k.backward(two, dy, act, deriv)  # (dy of the whole batch: mri_mse_loss divides by its own n)
    same_bits(dz, dz2, f"{tag} training dz")
    hold_grads(gw2, gb2, [t for pair in zip(gw, gb) for t in pair], f"{tag} training, cut against whole,", ORDER_TOL)
    dy_tail = dy.clone()
    dy_tail[:cut] = 0.0
    _, gw3, gb3 = k.backward(whole, dy_tail, act, deriv)
    hold_grads(gw3, gb3, f64["grads_tail"], f"{tag} training, tail only,")
    if n_sine < 2:
        return

    # ---- loss form: siren_forward_loss, siren_backward(head_done=True)
    r = k.loss_form(whole, k.t)
    assert torch.equal(r["y"], y), f"{tag} the loss form and the training form give different predictions"
    hold_scalar(r["loss"], f64["loss"], f"{tag} loss-form loss")
    for l in range(n_sine):
        if l < n_sine - 1:
            hold(r["act"][l], f64["act"][l], f"{tag} loss-form act[{l}]")
            hold(r["deriv"][l], f64["deriv"][l], f"{tag} loss-form deriv[{l}]")
        if l >= 1:
            hold(r["dz"][l], f64["dz"][l], f"{tag} loss-form dz[{l}]")
    hold_grads(r["gw"], r["gb"], f64["grads"], f"{tag} loss-form")
    r2 = k.loss_form(two, k.t)
    same_bits([r["y"]] + r["act"] + r["deriv"] + r["dz"], [r2["y"]] + r2["act"] + r2["deriv"] + r2["dz"],
              f"{tag} loss-form y / act / deriv / dz")
    hold_scalar(r2["loss"], r["loss"], f"{tag} loss-form, cut against whole, loss", ORDER_TOL)
    hold_grads(r2["gw"], r2["gb"], [t for pair in zip(r["gw"], r["gb"]) for t in pair],
               f"{tag} loss-form, cut against whole,", ORDER_TOL)
    target_tail = k.t.clone()
    target_tail[:cut] = r["y"][:cut]  # y - target is exactly zero in front of the cut
    r3 = k.loss_form(whole, target_tail)
    assert torch.equal(r3["y"], y)
    hold_scalar(r3["loss"], f64["loss_tail"], f"{tag} loss-form, tail only, loss")
    hold_grads(r3["gw"], r3["gb"], f64["grads_tail"], f"{tag} loss-form, tail only,")


@pytest.mark.parametrize("size", SIZE_NAMES)
@pytest.mark.parametrize("hidden,dim_in,n_sine", SIREN_CASES)
def test_siren_chain(amd, hidden, dim_in, n_sine, size):
    """siren_forward_kernel in its three modes and siren_backward_kernel with and without head_done: (a), (b), (c)."""
    assert amd.ops.siren_supported(dim_in, hidden, n_sine, 1)
    n = batch_sizes(SIREN_ROWS[hidden])[size]
    lib = amd.lib.load()
    image_kernels = hidden == 256 and n_sine >= 2  # (csrc/siren_rows.hip's by default; the image kernels under the option)
    try:
        if image_kernels:
            assert lib.mri_set_option(b"siren_rows", 0) == 0
        siren_chain_case(amd.ops, hidden, dim_in, n_sine, n)
    finally:
        if image_kernels:
            assert lib.mri_set_option(b"siren_rows", 1) == 0


# ================================================================================================ 2. the modulated chain
MOD_CASES = [(3, 128, 2), (3, 128, 3), (2, 64, 2), (1, 64, 3)]  # dim_in, hidden, layers
MOD_DRAWN = {128: (17200, 34600), 64: (34400, 69000)}  # rows drawn for n <= T + R + 3 / for 2 T + R + 3
MOD_KEYS = ("act", "hid", "dcos", "sn")


@functools.lru_cache(maxsize=None)
def mod_rows(d, H, L, drawn):
    """The rows clear of every ReLU kink (test_gpu_modsiren.selected_rows: at most 3 % of the drawn ones dropped, the
    float32 signs those of float64) and the two references' parameters: drawn once per shape, shared, never modified."""
    return selected_rows(d, H, L, 9700 + H + L + 10 * d, drawn=drawn)


class ModChain:
    def __init__(self, ops, r32, x, target):
        self.ops = ops
        self.sw, self.sb = [w.detach().cuda() for w, _ in r32.siren], [b.detach().cuda() for _, b in r32.siren]
        self.mw, self.mb = [w.detach().cuda() for w, _ in r32.mod], [b.detach().cuda() for _, b in r32.mod]
        self.x, self.t = x.cuda(), target.cuda()
        self.n, self.L, self.H = x.shape[0], len(self.mw), self.mw[0].shape[0]

    def forward_loss(self, cuts):
        saved = {key: [nan(self.n, self.H) for _ in range(self.L)] for key in MOD_KEYS}
        y, dy, loss = nan(self.n, 1), nan(self.n, 1), torch.zeros(1, device="cuda")
        for lo, hi in cuts:
            self.ops.modsiren_forward_loss(self.x[lo:hi], self.t[lo:hi], self.sw, self.sb, self.mw, self.mb, W0, W0,
                                           {key: views(saved[key], lo, hi) for key in MOD_KEYS}, y[lo:hi], dy[lo:hi],
                                           loss, n_total=self.n)
        return saved, y, dy, float(loss)

    def backward(self, cuts, dy, saved):
        """modsiren_backward on zeroed gradients: dzs, dzm, the gradients in the order of ModRef.parameters()."""
        dzs = [None] + [nan(self.n, self.H) for _ in range(self.L - 1)]
        dzm = [None] + [nan(self.n, self.H) for _ in range(self.L - 1)]
        g = [[torch.zeros_like(t) for t in ts] for ts in (self.sw, self.sb, self.mw, self.mb)]
        for lo, hi in cuts:
            self.ops.modsiren_backward(self.x[lo:hi], dy[lo:hi], self.sw, self.mw,
                                       {key: views(saved[key], lo, hi) for key in MOD_KEYS}, views(dzs, lo, hi),
                                       views(dzm, lo, hi), g[0], g[1], g[2], g[3])
        return dzs, dzm, [t for pair in zip(g[0], g[1]) for t in pair] + [t for pair in zip(g[2], g[3]) for t in pair]


def np_of(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("size", SIZE_NAMES)
@pytest.mark.parametrize("d,H,L", MOD_CASES)
def test_modsiren_chain(amd, d, H, L, size):
    """modsiren_forward_kernel<true> and modsiren_backward_kernel: (a) by close_or_no_worse, (b), (c)."""
    assert amd.ops.modsiren_supported(d, H, L, 1)
    n = batch_sizes(MOD_ROWS[H])[size]
    x_all, y_all, r64, r32 = mod_rows(d, H, L, MOD_DRAWN[H][size == "2T+R+3"])
    assert x_all.shape[0] >= n, f"only {x_all.shape[0]} rows kept, n = {n}"
    x, target = x_all[:n], 0.5 * y_all[:n] + 0.5  # in [0, 1]: tile_loop.intensities
    cut = cut_of(n, MOD_ROWS[H])
    whole, two = [(0, n)], [(0, cut), (cut, n)]
    f64, f32 = mod_reference(r64, x, target, cut), mod_reference(r32, x, target, cut)
    k = ModChain(amd.ops, r32, x, target)
    tag = f"modsiren ({d}, {H}, {L}) n = {n}:"

    def check(kernel, key, what, *index):
        a, b = f32[key], f64[key]
        for i in index:
            a, b = a[i], b[i]
        close_or_no_worse(np_of(kernel), np_of(a), np_of(b), f"{tag} {what}")

    saved, y, dy, loss = k.forward_loss(whole)
    dzs, dzm, grads = k.backward(whole, dy, saved)
    check(y, "y", "y")
    close_or_no_worse(np.array([loss]), np.array([f32["loss"]]), np.array([f64["loss"]]), f"{tag} loss")
    dy_of = lambda r: 2.0 * (r["y"] - target.to(r["y"].dtype).reshape(-1, 1)) / n  # noqa: E731
    close_or_no_worse(np_of(dy), np_of(dy_of(f32)), np_of(dy_of(f64)), f"{tag} dy")
    for l in range(L):
        for key in MOD_KEYS:
            check(saved[key][l], key, f"{key}[{l}]", l)
        if l >= 1:
            check(dzs[l], "dzs", f"dzs[{l}]", l)
            check(dzm[l], "dzm", f"dzm[{l}]", l)
    for i, g in enumerate(grads):
        check(g, "grads", f"gradient {i}", i)
    # the same calls through test_gpu_modsiren's runner (which also holds the inference kernel's y to the training bits)
    y_r, loss_r, grads_r = kernel_loss_and_grads(amd, r32, x, target)
    assert torch.equal(y_r, y.cpu()) and float(loss_r) == loss
    assert all(torch.equal(a, b.cpu()) for a, b in zip(grads_r, grads))

    # ---- (b) two launches cut at a tile boundary
    saved2, y2, dy2, loss2 = k.forward_loss(two)
    same_bits([y, dy] + [t for key in MOD_KEYS for t in saved[key]], [y2, dy2] + [t for key in MOD_KEYS for t in saved2[key]],
              f"{tag} y / dy / act / hid / dcos / sn")
    hold_scalar(loss2, loss, f"{tag} cut against whole, loss", ORDER_TOL)
    dzs2, dzm2, grads2 = k.backward(two, dy, saved)
    same_bits(dzs + dzm, dzs2 + dzm2, f"{tag} dzs / dzm")
    for i, (a, b) in enumerate(zip(grads2, grads)):
        hold(a, b, f"{tag} cut against whole, gradient {i}", ORDER_TOL)

    # ---- (c) the tail alone
    dy_tail = dy.clone()
    dy_tail[:cut] = 0.0
    _, _, grads3 = k.backward(whole, dy_tail, saved)
    for i, g in enumerate(grads3):
        check(g, "grads_tail", f"tail only, gradient {i}", i)


# ================================================================================================ 3. coordinate gradients
GRADIENT_CASES = [(hidden, dim_in, n_sine, size)
                  for hidden, dim_in, n_sine in [(256, 3, 3), (64, 2, 2), (32, 3, 3), (256, 4, 3), (64, 4, 2)]
                  for size in SIZE_NAMES] + \
                 [(128, dim_in, 3, size) for dim_in in (3, 4) for size in ("T", "T+1")]


def cat_of_two(run, x, cut):
    a, b = run(x[:cut]), run(x[cut:])
    return [torch.cat(pair) for pair in zip(a, b)]


@pytest.mark.parametrize("hidden,dim_in,n_sine,size", GRADIENT_CASES)
def test_siren_gradient(amd, hidden, dim_in, n_sine, size):
    """siren_gradient_kernel, four slots (dim_in <= 3) and eight (dim_in = 4): (a) by assert_no_worse, (b)."""
    assert amd.ops.siren_gradient_supported(dim_in, hidden, n_sine, 1)
    points = siren_grad_points(hidden, dim_in)
    n = batch_sizes(points)[size]
    params, x, (y32, g32), (y64, g64) = gradient_case(hidden, dim_in, n_sine, n)
    y, dydx = gradient_kernel(amd, x, params)
    assert y.shape == (n,) and dydx.shape == (n, dim_in)
    tag = f"siren gradient {dim_in} -> {hidden} x {n_sine}, n = {n}:"
    assert_no_worse(y.numpy(), y32.numpy(), y64.numpy(), f"{tag} y")
    assert_no_worse(dydx.numpy(), g32.numpy(), g64.numpy(), f"{tag} dydx")
    same_bits([y, dydx], cat_of_two(lambda part: gradient_kernel(amd, part, params), x, cut_of(n, points)), f"{tag} y / dydx")


@pytest.mark.parametrize("size", ["T", "T+1"])
@pytest.mark.parametrize("d,H,L", [(3, 128, 3), (2, 64, 3)])
def test_modsiren_gradient(amd, d, H, L, size):
    """modsiren_gradient_kernel at exactly one tile per workgroup, and with one workgroup alone on a second tile."""
    assert amd.ops.modsiren_gradient_supported(d, H, L, 1)
    n = batch_sizes(MOD_GRAD_POINTS[H])[size]
    siren, mod, x_all, (y32, g32), (y64, g64) = mod_gradient_case(d, H, L)
    assert x_all.shape[0] >= n
    x = x_all[:n]
    y, dydx = mod_gradient_kernel(amd, x, siren, mod)
    assert y.shape == (n,) and dydx.shape == (n, d)
    tag = f"modsiren gradient ({d}, {H}, {L}) n = {n}:"
    assert_no_worse(y.numpy(), y32[:n].numpy(), y64[:n].numpy(), f"{tag} y")
    assert_no_worse(dydx.numpy(), g32[:n].numpy(), g64[:n].numpy(), f"{tag} dydx")
    same_bits([y, dydx], cat_of_two(lambda part: mod_gradient_kernel(amd, part, siren, mod), x, cut_of(n, MOD_GRAD_POINTS[H])),
              f"{tag} y / dydx")
