"""Every sin / cos and GELU epilogue of the library against float64 ON EXACT ARGUMENTS (csrc/device_math.h:
sincos_fast, sincos_fast2, sincos_fast2_core, gelu_f, gelu_grad_f; the library sincosf on the cold paths).

The whole-network tests compare at 1e-5 of a tensor's maximum on arguments of a few tens.  Here each site is fed
arguments that are known exactly in float32 (tests/exact_args.py), so the float64 reference is the function of the
very number the kernel evaluated, and the bound is the functions' own promise:

    |sin_k - sin64(u)| <= 2^-23 min(1, 2 |u|)        |cos_k - cos64(u)| <= 2^-23        (w0 = 1, every finite u)
    w0 = 2^k scales the derivative's bound; w0 = 30 adds the product's rounding: 30 * 2^-23 + 30 * 2^-24
    GELU, per binade of |z|: max error <= 2 x the error of CPU float32 F.gelu (and its autograd) + 2^-23

How an argument is made exact.  First layers: one input column holds the argument set, W[j, that column] = s_j
alternating 1, 2, everything else 0, bias 0: the argument of element (i, j) is s_j x_i, and the two elements of every
packed pair differ.  Hidden layers: row j of W has one nonzero, a power of two c_j (1, 64, 4096, 2^14, 2^20 in turn)
at column i_j; the argument is c_j a[row, i_j] with `a` the kernel's OWN stored bits of the layer below, read back
-- exact whatever that layer did, because a power of two has one bf16 term and the three terms of `a` times it add
up without rounding (bf16x3.h, tests/test_bf16x3_cpu.py).  mri_linear_forward shows that directly: its identity
activation returns those arguments bit for bit.  One hidden layer per chain run has a bias: f32(c a) + f32(b).
Every element of every column is checked; no element is skipped.  The only elements exempt from the numeric bound
are planted +inf / -inf / NaN arguments, whose sin and w0 cos must be NaN.

Call sites (file:line) and the test that reaches them:

  sin / cos
    linear_small.hip:30   sincos_fast, K <= 8             test_linear_sine[small-*], test_sine_w0_30[linear_small]
    linear.hip:366        sincos_fast, direct epilogue    test_linear_sine[offset-*] (unchecked tiles), [n48-*] and the
                                                          ragged last row tile of every MFMA case (checked tiles)
    linear.hip:439        sincos_fast2, staged epilogue   test_linear_sine[staged-*] (first layer and hidden layer),
                                                          test_sine_w0_30[linear_staged]
    linear.hip:455        sincos_fast, staged, unpacked   NOT REACHABLE: the sine case of the staged epilogue always takes
                                                          the packed loop at :435-444 and `continue`s; the switch below it
                                                          only ever sees ReLU / GELU / identity
    siren_chain.hip:201   sincos_fast2, first layer       test_siren_sine[32 / 64 / 128 / 256-image], n = 6531 and 129
    siren_chain.hip:255   sincos_fast2, hidden layers     the same runs, layers 1 and 2
    siren_rows.hip:319    sincos_fast2_core, first layer  test_siren_sine[256-rows], test_sine_w0_30[siren_rows]
    siren_rows.hip:443-477  the core written out slice by slice between the MFMAs (hidden layers)   the same runs
    siren_rows.hip:167    sincosf, the per-tile repair (called at :324 first layer, :567 hidden)    the same runs (every
                          tile holds arguments beyond 8192) and test_nonfinite_and_cold_path_isolation[siren_rows] (one
                          row / one unit beyond 8192 among in-range neighbours)
    siren_gradient.hip:144  sincos_fast2, first layer     test_siren_gradient_first_layer (dim_in 1 ... 4: four and eight slots)
    siren_gradient.hip:200  sincos_fast2, hidden layers   test_siren_gradient_hidden_layer
    modsiren.hip:156 / :228   first / hidden layers       test_modsiren_sine[64 / 128], test_sine_w0_30[modsiren]
    modsiren_gradient.hip:145  first layer                test_modsiren_gradient_composition (full range), and at 0 in
                                                          test_modsiren_gradient_zero_input
    modsiren_gradient.hip:207  hidden layers              test_modsiren_gradient_zero_input (u = the bias, 64 + arguments)
    frequency.hip:28      sincosf                         test_frequency_forward (frequency.hip:47, the backward's, is the
                                                          same call on the same product; it has no exact per-element output)
  GELU
    linear_small.hip:34-35  gelu_grad_f / gelu_f          test_linear_gelu[small]
    linear.hip:371-372      direct epilogue               test_linear_gelu[offset], [n48]
    linear.hip:460-461      staged epilogue               test_linear_gelu[staged]
    mlp_shallow.hip:51 / :57  act_value / act_grad        test_shallow_gelu (hidden and output position, 32 / 64 / 128 units;
                                                          gelu' through shallow_mlp_train's d_x with targets that make
                                                          dLoss/dy an exact power of two: exact there too)
    batchnorm.hip:95 / :102   act_f / act_grad_f          test_bn_gelu (eval and training forward, d_beta of the backward)

Nothing here has a tolerance of its own making: the sine bounds are the ones above, the GELU reference error is
computed at run time.  MRI_YARDSTICK_PRINT=1 prints the observed maximum per site (as tests/yardstick.py does).
Measured on an MI355X: sin and w0 cos at most 9.13e-8 / 9.11e-8 (0.77 of the bound; the library path 6.7e-8), dydx of
the gradient kernels 0.51 of its bound, sin(sin x) 0.38; gelu 3.75e-7 where CPU float32 F.gelu is at 8.9e-7, gelu'
1.09e-7 where its autograd is at 2.4e-7 -- at every site the same figures, as the sites share device_math.h.

What these tests found: test_sine_w0_30[siren_rows] failed on the hidden layers of the rows kernels (errors up to 2.6e-2
in sin and 0.22 in w0 cos at |u| between 2^21 and 2^25).  siren_rows.hip's range check of a finished tile stood behind
`if constexpr (i == kTiles) RP_MARK(4)`; RP_MARK expands to nothing outside the profiling build, so the check became
that statement's body and only the last of the eight feature tiles was ever checked: features 0 ... 223 beyond 8192
kept the branch-free values (accurate up to about 2^20, where the quadrant number stops being exact in float32; NaN
for infinite arguments either way, which is why nothing else noticed).  With w0 = 1 the largest hidden argument here
is 2^20 and the branch-free value still meets the bound, so it is the w0 = 30 run that holds the repair itself.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_args as ea
import layout
from oracle import detrand

pytestmark = pytest.mark.gpu

U23 = ea.U23
C_CYCLE = (1.0, 64.0, 4096.0, 2.0 ** 14, 2.0 ** 20)
_cache = {}


def sine_set():
    if "sin" not in _cache:
        _cache["sin"] = ea.sincos_arguments()
    return _cache["sin"]


def gelu_set():
    if "gelu" not in _cache:
        _cache["gelu"] = ea.gelu_arguments()
    return _cache["gelu"]


@pytest.fixture(scope="module")
def amd():
    from mri_interpolation_amd import _lib, ops
    assert torch.cuda.is_available(), "these tests need the GPU"
    _lib.load()
    return type("NS", (), dict(lib=_lib, ops=ops))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def nans(*shape):
    return torch.full(shape, float("nan"), device="cuda", dtype=torch.float32)


def say(text):
    if os.environ.get("MRI_YARDSTICK_PRINT"):
        print("device-math " + text)


def _worst(err, bound, u, got):
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    ratio = np.where(np.isnan(err), np.inf, ratio)
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[at]), f"element {at}: argument {u[at]!r}, kernel {got[at]!r}, error {err[at]:.3e}, bound {bound[at]:.3e}"


def check_sincos(site, sin_k, dcos_k, u32, w0=1.0, planted=None, sin_scale=1.0):
    """sin_k / dcos_k (float32 arrays) against sin64(u) / w0 cos64(u), u32 the exact float32 argument of each element.
    planted: boolean mask of the elements whose argument is non-finite ON PURPOSE (None: there are none)."""
    assert sin_k.dtype == np.float32 and u32.dtype == np.float32 and sin_k.shape == u32.shape
    u = u32.astype(np.float64)
    finite = np.isfinite(u)
    if planted is None:
        assert finite.all(), f"{site}: a non-finite argument nobody planted"
    else:
        assert np.array_equal(~finite, planted), f"{site}: the non-finite arguments are not the planted ones"
        assert np.isnan(sin_k[planted]).all(), f"{site}: sin of a non-finite argument is not NaN"
        assert dcos_k is None or np.isnan(dcos_k[planted]).all(), f"{site}: w0 cos of a non-finite argument is not NaN"
    us = np.where(finite, u, 0.0)
    pow2 = np.frexp(w0)[0] == 0.5
    es = np.where(finite, np.abs(sin_k.astype(np.float64) - np.sin(us)), 0.0)
    bs = sin_scale * ea.sin_bound(us)
    rs, where_s = _worst(es, bs, u32, sin_k)
    text = f"{site}: sin max error {np.nanmax(es):.3e} ({rs:.2f} of its bound)"
    if dcos_k is not None:
        ec = np.where(finite, np.abs(dcos_k.astype(np.float64) - w0 * np.cos(us)), 0.0)
        bc = np.full(ec.shape, abs(w0) * U23 * (1.0 if pow2 else 1.5))
        rc, where_c = _worst(ec, bc, u32, dcos_k)
        text += f", w0 cos max error {np.nanmax(ec):.3e} ({rc:.2f} of its bound, w0 = {w0:g})"
    say(text)
    assert rs <= 1.0, f"{site}: sin: {where_s}"
    if dcos_k is not None:
        assert rc <= 1.0, f"{site}: w0 cos: {where_c}"
    zero = finite & (u == 0)
    assert (sin_k[zero] == 0).all(), f"{site}: sin(0) is not exactly 0"


def same_bits(a, b):
    return bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


# ------------------------------------------------------------------------------------------- weights and arguments
def first_weight(n_out, k, col):
    """W[j, col] = s_j = 1, 2, 1, 2 ...; the rest 0."""
    w = np.zeros((n_out, k), dtype=np.float32)
    w[:, col] = 1.0 + (np.arange(n_out) % 2)
    return w


def hidden_weight(h, k, layer, cs):
    """Row j: one nonzero c_j = cs[j % len(cs)] at column i_j = (7 j + 3 + layer) % k (a permutation when k = h)."""
    j = np.arange(h)
    idx = (7 * j + 3 + layer) % k
    c = np.asarray(cs, dtype=np.float32)[j % len(cs)]
    w = np.zeros((h, k), dtype=np.float32)
    w[j, idx] = c
    return w, idx, c


def first_args(x_col, w, col, w0):
    """float32 w0 * (s_j x_i): one product by 1 or 2 (exact), one by w0."""
    z = x_col[:, None].astype(np.float32) * w[None, :, col]
    return (np.float32(w0) * z).astype(np.float32)


def hidden_args(a_prev, idx, c, bias, w0):
    """float32 w0 * (c_j a[:, i_j] + b_j): the product is exact, then one f32 add and one f32 product."""
    with np.errstate(invalid="ignore", over="ignore"):
        z = a_prev[:, idx] * c[None, :]
        if bias is not None:
            z = z + bias[None, :].astype(np.float32)
        return (np.float32(w0) * z).astype(np.float32)


def inputs(values, dim_in, col, fill_seed=None):
    x = np.zeros((values.size, dim_in), dtype=np.float32)
    if fill_seed is not None:  # finite values in the columns whose weights are 0
        x[:] = detrand.uniform(values.size * dim_in, fill_seed, -3.0, 3.0).reshape(values.size, dim_in)
    x[:, col] = values
    return x


def planted_case():
    """In-range arguments (|s_j x| <= 8192) with +inf, -inf, NaN in three rows and ONE row beyond 8192."""
    v = sine_set()
    v = v[np.abs(v) <= 4096][:1000].copy()
    rows = {37: np.inf, 410: -np.inf, 777: np.nan}
    for r, val in rows.items():
        v[r] = val
    v[600] = 1.0e9
    bad = np.zeros(v.size, dtype=bool)
    bad[list(rows)] = True
    return v, bad


# ------------------------------------------------------------------------------------------- linear_forward
LINEAR_SHAPES = {"small": (3, 64, 0), "staged": (32, 64, 0), "offset": (32, 64, 1), "n48": (32, 48, 0)}


def _linear_call(amd, x, w, act, w0, offset):
    """(out, deriv, identity) of mri_linear_forward; out / deriv under guard bands, `offset` floats off a 16-byte line."""
    ops = amd.ops
    n, n_out = x.shape[0], w.shape[0]
    bias = torch.zeros(n_out, device="cuda")
    out, chk_o = layout.place(torch.full((n, n_out), float("nan")), offset, ld=n_out)
    der, chk_d = layout.place(torch.full((n, n_out), float("nan")), offset, ld=n_out)
    ops.linear_forward(x, w, bias, act, w0, out=out, deriv=der)
    ident = ops.linear_forward(x, w, bias, ops.ACT_IDENTITY, 1.0)
    chk_o(what="out"), chk_d(what="deriv")
    return host(out), host(der), host(ident)


def _linear_sine(amd, tag, values, w0=1.0, planted_rows=None):
    k, n_out, offset = LINEAR_SHAPES[tag]
    w = first_weight(n_out, k, 0)
    x = inputs(values, k, 0)
    s, d, ident = _linear_call(amd, dev(x), dev(w), amd.ops.ACT_SINE, w0, offset)
    z = first_args(values, w, 0, 1.0)
    assert same_bits(ident, z), f"linear {tag}: the identity activation does not return s_j x_i bit for bit"
    planted = None if planted_rows is None else np.repeat(planted_rows[:, None], n_out, 1)
    check_sincos(f"linear_forward {tag} first layer (n {values.size}, K {k}, N {n_out}, w0 {w0:g})", s, d,
                 first_args(values, w, 0, w0), w0, planted)
    return s


@pytest.mark.parametrize("n", [None, 129])
@pytest.mark.parametrize("tag", list(LINEAR_SHAPES))
def test_linear_sine(amd, tag, n):
    """mri_linear_forward's three sine epilogues on the whole argument set, and (staged / offset: K = N = 64) a hidden
    layer on the stored bits of the first."""
    values = sine_set()[:n]
    a1 = _linear_sine(amd, tag, values)
    k, n_out, offset = LINEAR_SHAPES[tag]
    if tag not in ("staged", "offset"):
        return
    w2, idx, c = hidden_weight(64, 64, 1, C_CYCLE)
    s, d, ident = _linear_call(amd, dev(a1), dev(w2), amd.ops.ACT_SINE, 1.0, offset)
    u = hidden_args(a1, idx, c, None, 1.0)
    assert same_bits(ident, u), f"linear {tag}: c_j a[:, i_j] is not exact in the kernel's product"
    check_sincos(f"linear_forward {tag} hidden layer (n {values.size})", s, d, u)


# ------------------------------------------------------------------------------------------- siren_forward
def _siren_run(amd, hidden, rows_opt, values, w0=1.0, cs=C_CYCLE, planted_rows=None, big_unit=None):
    ops, lib = amd.ops, amd.lib.load()
    n, dim_in, col = values.size, 3, (hidden // 32) % 3
    w_first = first_weight(hidden, dim_in, col)
    layers = [hidden_weight(hidden, hidden, l, cs) for l in (1, 2)]
    if big_unit is not None:  # one unit of layer 1 beyond 8192 for most rows, its tile's neighbours in range
        w1, idx1, c1 = layers[0]
        w1[big_unit, idx1[big_unit]] = c1[big_unit] = 2.0 ** 20
    b2 = detrand.uniform(hidden, 77 + hidden, -1.0, 1.0)
    head = detrand.uniform(hidden, 78 + hidden, -1.0, 1.0).reshape(1, hidden)
    weights = [dev(w_first), dev(layers[0][0]), dev(layers[1][0]), dev(head)]
    biases = [torch.zeros(hidden, device="cuda"), torch.zeros(hidden, device="cuda"), dev(b2), torch.zeros(1, device="cuda")]
    act, deriv = [nans(n, hidden) for _ in range(3)], [nans(n, hidden) for _ in range(3)]
    try:
        assert lib.mri_set_option(b"siren_rows", rows_opt) == 0
        ops.siren_forward(dev(inputs(values, dim_in, col)), weights, biases, w0, w0, act=act, deriv=deriv)
        torch.cuda.synchronize()
    finally:
        assert lib.mri_set_option(b"siren_rows", 1) == 0
    act, deriv = [host(t) for t in act], [host(t) for t in deriv]
    planted = None if planted_rows is None else np.repeat(planted_rows[:, None], hidden, 1)
    form = "rows" if hidden == 256 and rows_opt else "image"
    site = f"siren_forward H {hidden} {form} kernels (n {n}, w0 {w0:g})"
    check_sincos(site + " layer 0", act[0], deriv[0], first_args(values, w_first, col, w0), w0, planted)
    for l, bias in ((1, None), (2, b2)):
        _, idx, c = layers[l - 1]
        check_sincos(site + f" layer {l}", act[l], deriv[l], hidden_args(act[l - 1], idx, c, bias, w0), w0, planted)


SIREN_FORMS = [(32, 1), (64, 1), (128, 1), (256, 1), (256, 0)]


@pytest.mark.parametrize("n", [None, 129])
@pytest.mark.parametrize("hidden,rows_opt", SIREN_FORMS, ids=["32", "64", "128", "256-rows", "256-image"])
def test_siren_sine(amd, hidden, rows_opt, n):
    """The fused SIREN chain: first layer and two hidden layers (the second with a bias), every width; width 256 with
    the rows-in-registers kernels and with the LDS-image kernels."""
    _siren_run(amd, hidden, rows_opt, sine_set()[:n])


# ------------------------------------------------------------------------------------------- modsiren_forward
def _neutral_modulator(hidden, dim_in, n_layers):
    """Weights 0, biases 1: h_l = relu(1) = 1, so act = sin and dcos = w0 cos exactly."""
    mw = [torch.zeros(hidden, dim_in if l == 0 else hidden + dim_in, device="cuda") for l in range(n_layers)]
    mb = [torch.ones(hidden, device="cuda") for _ in range(n_layers)]
    return mw, mb


def _modsiren_run(amd, hidden, values, w0=1.0, cs=C_CYCLE, planted_rows=None, big_unit=None):
    ops = amd.ops
    n, dim_in, col, n_layers = values.size, 2, (hidden // 64) % 2, 3
    w_first = first_weight(hidden, dim_in, col)
    layers = [hidden_weight(hidden, hidden, l, cs) for l in (1, 2)]
    if big_unit is not None:
        w1, idx1, c1 = layers[0]
        w1[big_unit, idx1[big_unit]] = c1[big_unit] = 2.0 ** 20
    b2 = detrand.uniform(hidden, 177 + hidden, -1.0, 1.0)
    head = detrand.uniform(hidden, 178 + hidden, -1.0, 1.0).reshape(1, hidden)
    sw = [dev(w_first), dev(layers[0][0]), dev(layers[1][0]), dev(head)]
    sb = [torch.zeros(hidden, device="cuda"), torch.zeros(hidden, device="cuda"), dev(b2), torch.zeros(1, device="cuda")]
    mw, mb = _neutral_modulator(hidden, dim_in, n_layers)
    saved = {key: [nans(n, hidden) for _ in range(n_layers)] for key in ("act", "hid", "dcos", "sn")}
    ops.modsiren_forward(dev(inputs(values, dim_in, col)), sw, sb, mw, mb, w0, w0, saved=saved)
    torch.cuda.synchronize()
    saved = {key: [host(t) for t in v] for key, v in saved.items()}
    planted = None if planted_rows is None else np.repeat(planted_rows[:, None], hidden, 1)
    site = f"modsiren_forward H {hidden} (n {n}, w0 {w0:g})"
    for l in range(n_layers):
        live = np.ones((n, hidden), bool) if planted is None else ~planted
        assert (saved["hid"][l][live] == 1).all(), f"{site}: the neutral modulator is not 1 (layer {l})"
        assert same_bits(saved["act"][l][live], saved["sn"][l][live]), f"{site}: act != sin under h = 1 (layer {l})"
        if l == 0:
            u = first_args(values, w_first, col, w0)
        else:
            _, idx, c = layers[l - 1]
            u = hidden_args(saved["act"][l - 1], idx, c, b2 if l == 2 else None, w0)
        check_sincos(site + f" layer {l}", saved["sn"][l], saved["dcos"][l], u, w0, planted)


@pytest.mark.parametrize("n", [None, 129])
@pytest.mark.parametrize("hidden", [64, 128])
def test_modsiren_sine(amd, hidden, n):
    """The fused modulated-SIREN chain under a neutral modulator: sn and dcos of three layers."""
    _modsiren_run(amd, hidden, sine_set()[:n])


# ------------------------------------------------------------------------------------------- w0 = 30, non-finite
FAMILIES = ["linear_small", "linear_staged", "siren_image", "siren_rows", "modsiren"]


def _family_run(amd, family, values, **kw):
    if family == "linear_small":
        _linear_sine(amd, "small", values, kw.get("w0", 1.0), kw.get("planted_rows"))
    elif family == "linear_staged":
        _linear_sine(amd, "staged", values, kw.get("w0", 1.0), kw.get("planted_rows"))
    elif family == "siren_image":
        _siren_run(amd, 64, 1, values, **kw)
    elif family == "siren_rows":
        _siren_run(amd, 256, 1, values, **kw)
    else:
        _modsiren_run(amd, 64, values, **kw)


@pytest.mark.parametrize("family", FAMILIES)
def test_sine_w0_30(amd, family):
    """The networks' real w0: the argument is f32(30) * f32(z), the derivative carries one more rounding."""
    _family_run(amd, family, sine_set(), w0=30.0)


@pytest.mark.parametrize("family", FAMILIES)
def test_nonfinite_and_cold_path_isolation(amd, family):
    """+inf, -inf and NaN planted in three rows give NaN there and nowhere else; one row (first layer) and one unit
    (hidden layer, chains) beyond 8192 send their tile down the cold path, whose in-range neighbours still meet the
    bound.  Hidden weights are 1 here, so nothing else leaves the fast path's range."""
    values, bad = planted_case()
    kw = dict(planted_rows=bad)
    if not family.startswith("linear"):
        kw.update(cs=(1.0,), big_unit=5)
    _family_run(amd, family, values, **kw)


# ------------------------------------------------------------------------------------------- gradient kernels
def _one_hot_head(hidden, j):
    head = np.zeros((1, hidden), dtype=np.float32)
    head[0, j] = 1.0
    return dev(head), torch.zeros(1, device="cuda")


def _siren_gradient_first(amd, dim_in, hidden, d0, j, values):
    """One sine layer, W1[j, d0] = 1, head e_j: (y, dydx) = (sin x_d0, cos x_d0 in column d0)."""
    w1 = np.zeros((hidden, dim_in), dtype=np.float32)
    w1[j, d0] = 1.0
    head, hb = _one_hot_head(hidden, j)
    x = inputs(values, dim_in, d0, fill_seed=300 + dim_in)
    y, g = amd.ops.siren_gradient(dev(x), [dev(w1), head], [torch.zeros(hidden, device="cuda"), hb], 1.0, 1.0,
                                  y=nans(values.size, 1), dydx=nans(values.size, dim_in))
    torch.cuda.synchronize()
    return host(y)[:, 0], host(g)


GRAD_WIDTH = {1: 32, 2: 64, 3: 128, 4: 256}


def test_siren_gradient_first_layer(amd):
    """siren_gradient.hip's first-layer sincos in every tangent slot of the four-slot (dim_in <= 3) and eight-slot
    (dim_in = 4) kernels, units 0, 1, 31, 32, H - 1."""
    values, turn = sine_set(), 0
    for dim_in, hidden in GRAD_WIDTH.items():
        units = sorted({0, 1, 31, 32 % hidden, hidden - 1})
        for d0 in range(dim_in):
            for j in {units[turn % len(units)], units[(turn + 2) % len(units)]}:
                y, g = _siren_gradient_first(amd, dim_in, hidden, d0, j, values)
                check_sincos(f"siren_gradient first layer (dim_in {dim_in}, H {hidden}, axis {d0}, unit {j})", y, g[:, d0], values)
                others = np.delete(g, d0, axis=1)
                assert (others == 0).all(), f"dim_in {dim_in}, axis {d0}, unit {j}: a gradient in an axis with weight 0"
            turn += 1


@pytest.mark.parametrize("dim_in,hidden,d0,j1,j2", [(2, 64, 1, 31, 32), (4, 128, 3, 127, 0), (3, 256, 0, 1, 255)])
def test_siren_gradient_hidden_layer(amd, dim_in, hidden, d0, j1, j2):
    """Two sine layers, W2[j2, j1] = c: y = sin(c a1), dydx = cos(c a1) c d1 with a1 = sin x and d1 = cos x the bits
    of the one-layer call (the same first-layer code).  The tangent c d1 is exact, the kernel rounds the product once:
    |error| <= 2^-23 |c d1| (the cosine) + 2 * 2^-24 |cos(u) c d1| (f32 roundings)."""
    values = sine_set()
    a1, g1 = _siren_gradient_first(amd, dim_in, hidden, d0, j1, values)
    d1 = g1[:, d0]
    w1 = np.zeros((hidden, dim_in), dtype=np.float32)
    w1[j1, d0] = 1.0
    head, hb = _one_hot_head(hidden, j2)
    x = dev(inputs(values, dim_in, d0, fill_seed=300 + dim_in))
    zeros = torch.zeros(hidden, device="cuda")
    for c in C_CYCLE:
        w2 = np.zeros((hidden, hidden), dtype=np.float32)
        w2[j2, j1] = c
        y, g = amd.ops.siren_gradient(x, [dev(w1), dev(w2), head], [zeros, zeros, hb], 1.0, 1.0,
                                      y=nans(values.size, 1), dydx=nans(values.size, dim_in))
        torch.cuda.synchronize()
        y, g = host(y)[:, 0], host(g)
        u = (np.float32(c) * a1).astype(np.float32)
        site = f"siren_gradient hidden layer (dim_in {dim_in}, H {hidden}, c {c:g})"
        check_sincos(site, y, None, u)
        tangent = float(c) * d1.astype(np.float64)
        want = np.cos(u.astype(np.float64)) * tangent
        err = np.abs(g[:, d0].astype(np.float64) - want)
        bound = U23 * np.abs(tangent) + 2.0 * 2.0 ** -24 * np.abs(want)
        ratio, where = _worst(err, bound, u, g[:, d0])
        say(f"{site}: dydx max error {err.max():.3e} ({ratio:.2f} of its bound)")
        assert ratio <= 1.0, f"{site}: dydx: {where}"
        assert (np.delete(g, d0, axis=1) == 0).all(), f"{site}: a gradient in an axis with weight 0"


def _zero_input_arguments():
    v = sine_set()
    picked = v[::v.size // 64][:64]
    lim = np.float32(8192.0)
    extra = np.array([lim, -lim, np.nextafter(lim, np.float32(np.inf)), np.nextafter(lim, np.float32(0)), 0.0,
                      v[np.abs(v) > 2.0 ** 20][0], np.float32(np.pi / 2), np.float32(-3 * np.pi / 2)], dtype=np.float32)
    return np.concatenate([picked, extra])


def test_modsiren_gradient_zero_input(amd):
    """modsiren_gradient.hip's hidden-layer sincos (the kernel has >= 2 layers and stores nothing per layer): x = 0,
    W1[i, d0] = 1, b1 = 0 give a1 = sin(0) = 0 with tangent cos(0) = 1 -- asserted exactly in the stored-output kernel
    first --, so unit j of layer 2 evaluates u = b2_j exactly: y = sin(b2_j), dydx[:, d0] = cos(b2_j) W2[j, i]."""
    ops = amd.ops
    for hidden in (64, 128):
        for dim_in in (1, 2, 3):
            mw, mb = _neutral_modulator(hidden, dim_in, 2)
            saved = {key: [nans(4, hidden) for _ in range(2)] for key in ("act", "hid", "dcos", "sn")}
            sw = [torch.ones(hidden, dim_in, device="cuda"), torch.zeros(hidden, hidden, device="cuda"),
                  torch.zeros(1, hidden, device="cuda")]
            sb = [torch.zeros(hidden, device="cuda"), torch.zeros(hidden, device="cuda"), torch.zeros(1, device="cuda")]
            ops.modsiren_forward(torch.zeros(4, dim_in, device="cuda"), sw, sb, mw, mb, 1.0, 1.0, saved=saved)
            for l in range(2):
                assert (host(saved["sn"][l]) == 0).all() and (host(saved["dcos"][l]) == 1).all(), \
                    "sin(0) = 0 and cos(0) = 1 exactly"
    args = _zero_input_arguments()
    assert (np.abs(args) > 8192).sum() >= 3 and (np.abs(args) <= 8192).sum() >= 40
    got_y, got_g, want_c = [], [], []
    for t, b2j in enumerate(args):
        hidden, dim_in = (64, 128)[t % 2], 1 + t % 3
        d0, i, j = (t // 3) % dim_in, (5 * t + 2) % hidden, (11 * t + (0, 1, 31, 32, hidden - 1)[t % 5]) % hidden
        c = C_CYCLE[t % len(C_CYCLE)]
        w1 = np.zeros((hidden, dim_in), dtype=np.float32)
        w1[i, d0] = 1.0
        w2 = np.zeros((hidden, hidden), dtype=np.float32)
        w2[j, i] = c
        b2 = detrand.uniform(hidden, 500 + t, -40.0, 40.0)
        b2[j] = b2j
        head, hb = _one_hot_head(hidden, j)
        mw, mb = _neutral_modulator(hidden, dim_in, 2)
        y, g = ops.modsiren_gradient(torch.zeros(4, dim_in, device="cuda"), [dev(w1), dev(w2), head],
                                     [torch.zeros(hidden, device="cuda"), dev(b2), hb], mw, mb, 1.0, 1.0,
                                     y=nans(4, 1), dydx=nans(4, dim_in))
        y, g = host(y)[:, 0], host(g)
        assert (np.delete(g, d0, axis=1) == 0).all(), f"argument {b2j!r}: a gradient in an axis with weight 0"
        assert (y == y[0]).all() and (g[:, d0] == g[0, d0]).all(), f"argument {b2j!r}: the four equal rows differ"
        got_y.append(y[0]), got_g.append(g[0, d0] / np.float32(c)), want_c.append(c)
    # (dydx / c is exact: c is a power of two; the bound w0-scales the same way)
    check_sincos("modsiren_gradient hidden layer, zero input", np.array(got_y, np.float32), np.array(got_g, np.float32), args)


@pytest.mark.parametrize("hidden,dim_in,d0", [(64, 1, 0), (128, 2, 1), (64, 3, 2), (128, 3, 0)])
def test_modsiren_gradient_composition(amd, hidden, dim_in, d0):
    """The full argument range at modsiren_gradient.hip's first layer: W1[i, d0] = 1, W2[j, i] = 1, y = sin(sin(x))
    against float64 at twice the sine bound (the inner sine's error passes through the outer with slope <= 1)."""
    values = sine_set()
    i, j = 31, 32
    w1 = np.zeros((hidden, dim_in), dtype=np.float32)
    w1[i, d0] = 1.0
    w2 = np.zeros((hidden, hidden), dtype=np.float32)
    w2[j, i] = 1.0
    head, hb = _one_hot_head(hidden, j)
    mw, mb = _neutral_modulator(hidden, dim_in, 2)
    zeros = torch.zeros(hidden, device="cuda")
    y, g = amd.ops.modsiren_gradient(dev(inputs(values, dim_in, d0, fill_seed=600 + dim_in)), [dev(w1), dev(w2), head],
                                     [zeros, zeros, hb], mw, mb, 1.0, 1.0, y=nans(values.size, 1),
                                     dydx=nans(values.size, dim_in))
    y, g = host(y)[:, 0], host(g)
    u = values.astype(np.float64)
    err = np.abs(y.astype(np.float64) - np.sin(np.sin(u)))
    ratio, where = _worst(err, 2.0 * ea.sin_bound(u), values, y)
    say(f"modsiren_gradient composition (H {hidden}, dim_in {dim_in}): sin(sin x) max error {err.max():.3e} "
        f"({ratio:.2f} of its bound)")
    assert ratio <= 1.0, f"sin(sin x): {where}"
    assert (np.delete(g, d0, axis=1) == 0).all() and np.isfinite(g).all()


# ------------------------------------------------------------------------------------------- frequency encoding
def test_frequency_forward(amd):
    """frequency.hip: sincosf of v 2^l, l = 0 ... 11 (the product is exact; 2^30 2^11 is finite, no scaling needed)."""
    v = sine_set()
    x = np.stack([v, v[::-1]], axis=1)
    levels = 12
    out = host(amd.ops.frequency_forward(dev(x), levels, out=nans(v.size, 2 * 2 * levels)))
    out = out.reshape(v.size, 2, 2, levels)  # row, axis, sin | cos, level
    u = (x[:, :, None] * np.exp2(np.arange(levels, dtype=np.float32))[None, None, :]).astype(np.float32)
    assert np.isfinite(u).all()
    check_sincos("frequency_forward (12 levels)", np.ascontiguousarray(out[:, :, 0]), np.ascontiguousarray(out[:, :, 1]), u)


# ------------------------------------------------------------------------------------------- GELU
def _gelu_references(z32):
    """(gelu64, gelu'64, gelu32, gelu'32) of float32 arguments: F.gelu (erf form) and its autograd on the CPU."""
    out = []
    for dtype in (torch.float64, torch.float32):
        z = torch.from_numpy(z32.astype(np.float32).ravel()).to(dtype).requires_grad_(True)
        y = F.gelu(z)
        g, = torch.autograd.grad(y.sum(), z)
        out += [y.detach().numpy().astype(np.float64), g.numpy().astype(np.float64)]
    return out


def check_gelu(site, y_k, g_k, z32):
    """Per binade of |z|: the kernel's max error from float64 <= 2 x CPU float32 F.gelu's (its autograd's) + 2^-23."""
    z32 = np.ascontiguousarray(z32, dtype=np.float32).ravel()
    y64, g64, y32, g32 = _gelu_references(z32)
    b = ea.binade(z32)
    for name, got, want, ref in (("gelu", y_k, y64, y32), ("gelu'", g_k, g64, g32)):
        if got is None:
            continue
        got = np.asarray(got).ravel()
        assert got.dtype == np.float32 and got.shape == z32.shape
        err, ref_err = np.abs(got.astype(np.float64) - want), np.abs(ref - want)
        worst = 0.0
        for e in np.unique(b):
            m = b == e
            k, r = err[m].max(), ref_err[m].max()
            worst = max(worst, k)
            at = np.flatnonzero(m)[int(np.argmax(np.where(np.isnan(err[m]), np.inf, err[m])))]
            assert k <= 2.0 * r + U23, (f"{site}: {name}, binade 2^{e}: kernel {k:.3e} from float64, float32 reference "
                                        f"{r:.3e}; worst at z = {z32[at]!r}: kernel {got[at]!r}, float64 {want[at]!r}")
        say(f"{site}: {name} max error {worst:.3e} (float32 reference {ref_err.max():.3e})")


@pytest.mark.parametrize("tag", list(LINEAR_SHAPES))
def test_linear_gelu(amd, tag):
    """mri_linear_forward's GELU epilogues: out = gelu(s_j z_i), deriv = gelu'(s_j z_i), every column."""
    k, n_out, offset = LINEAR_SHAPES[tag]
    values = gelu_set()
    w = first_weight(n_out, k, 0)
    y, d, ident = _linear_call(amd, dev(inputs(values, k, 0)), dev(w), amd.ops.ACT_GELU, 1.0, offset)
    z = first_args(values, w, 0, 1.0)
    assert same_bits(ident, z)
    check_gelu(f"linear_forward {tag} GELU", y, d, z)


def _exact_targets(y):
    """Targets t (float32) with y - t = +-2^e exactly in float32 (1 where |y| < 2^-25): dLoss/dy = 2 (y - t) / (n
    divisor) is then that power of two for divisor = 2 / n, and the d_x that comes back is gelu' times it, exactly."""
    y = y.astype(np.float32)
    tiny = np.abs(y) < 2.0 ** -25
    _, e = np.frexp(np.where(tiny, 1.0, y).astype(np.float64))
    p = np.ldexp(1.0, e - 2).astype(np.float32)  # 2^(floor(log2 |y|) - 1) <= |y| / 2: y - p is exact (Sterbenz)
    t = np.where(tiny, np.float32(-1.0), y - np.sign(y) * p).astype(np.float32)
    diff = (y - t).astype(np.float32)
    assert (np.frexp(diff)[0] == np.where(diff > 0, 0.5, -0.5)).all() and (diff != 0).all()
    return t, diff


@pytest.mark.parametrize("hidden,k_in", [(32, 16), (64, 16), (128, 16), (64, 24)])
@pytest.mark.parametrize("where", ["hidden", "out"])
def test_shallow_gelu(amd, hidden, k_in, where):
    """mlp_shallow.hip with one-hot W1 rows (unit h reads feature h % k_in) and a one-hot w2 (unit h0): y = gelu of
    feature h0 % k_in, with GELU in the hidden position (output identity) or in the output position (hidden identity).
    gelu' comes back exactly through shallow_mlp_train's d_x: the target makes y - t a power of two, the gradient
    divisor 2 / n makes dLoss/dy = y - t, and every other term of the d_x product is 0."""
    ops = amd.ops
    values = gelu_set()
    n = values.size
    x_fm = np.stack([np.roll(values, 37 * f) for f in range(k_in)])
    acts = (ops.ACT_GELU, ops.ACT_IDENTITY) if where == "hidden" else (ops.ACT_IDENTITY, ops.ACT_GELU)
    w1 = np.zeros((hidden, k_in), dtype=np.float32)
    w1[np.arange(hidden), np.arange(hidden) % k_in] = 1.0
    xg = dev(x_fm)
    for h0 in (0, 5, 17, hidden - 1):
        f0 = h0 % k_in
        w2 = np.zeros((1, hidden), dtype=np.float32)
        w2[0, h0] = 1.0
        params = [(dev(w1), torch.zeros(hidden, device="cuda")), (dev(w2), torch.zeros(1, device="cuda"))]
        y = host(ops.shallow_mlp_forward(xg, params, acts, y=nans(n, 1)))[:, 0]
        t, diff = _exact_targets(y)
        grads = [(nans(hidden, k_in), nans(hidden)), (nans(1, hidden), nans(1))]
        d_x, y2 = nans(k_in, n), nans(n, 1)
        ops.shallow_mlp_train(xg, dev(t.reshape(n, 1)), params, acts, grads, nans(1), d_x=d_x, y=y2, overwrite=True,
                              grad_divisor=2.0 / n)  # 2 / (n * divisor) = 1 once rounded to float32
        d_x = host(d_x)
        assert same_bits(host(y2)[:, 0], y), "the training kernel's y differs from the inference kernel's"
        assert (np.delete(d_x, f0, axis=0) == 0).all(), "d_x in a feature no live unit reads"
        site = f"shallow_mlp H {hidden} k_in {k_in}, GELU in the {where} position, unit {h0}"
        check_gelu(site, y, (d_x[f0] / diff).astype(np.float32), x_fm[f0])


def test_bn_gelu(amd):
    """batchnorm.hip: gamma = 0 and beta_c = the argument make u = beta_c whatever the statistics; the eval and the
    training forward give gelu(beta_c) in every row, and a dy that is 1 in one row and 0 elsewhere gives
    d_beta_c = gelu'(beta_c) (the float64 column sum has one nonzero term)."""
    ops = amd.ops
    values = gelu_set()
    rows = 6
    for lo in range(0, values.size, 1024):
        beta = values[lo:lo + 1024]
        c = beta.size
        z = dev(detrand.uniform(rows * c, 900 + lo, -2.0, 2.0).reshape(rows, c))
        gamma, bg = torch.zeros(c, device="cuda"), dev(beta)
        rm, rv = dev(detrand.uniform(c, 901 + lo, -1.0, 1.0)), dev(detrand.uniform(c, 902 + lo, 0.5, 2.0))
        y_eval = host(ops.bn_act_forward(z, gamma, bg, ops.ACT_GELU, running_mean=rm, running_var=rv, out=nans(rows, c)))
        save = ops.bn_stats(z)
        y_train = host(ops.bn_act_forward(z, gamma, bg, ops.ACT_GELU, save=save, out=nans(rows, c)))
        dy = torch.zeros(rows, c, device="cuda")
        dy[3] = 1.0
        d_gamma, d_beta = nans(c), nans(c)
        ops.bn_act_backward(dy, z, save, gamma, bg, d_gamma, d_beta, ops.ACT_GELU, dz=torch.empty_like(dy), overwrite=True)
        arg = np.repeat(beta[None, :], rows, 0)
        check_gelu(f"bn_act_forward eval (C {c})", y_eval, None, arg)
        check_gelu(f"bn_act_forward training (C {c})", y_train, None, arg)
        check_gelu(f"bn_act_backward d_beta (C {c})", None, host(d_beta), beta)
