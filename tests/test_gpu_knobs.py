"""The tuning knobs of mri_set_option against the default and against float64 (include/mri_inr.h).

Every "speed-only" knob picks another kernel or another way of cutting the work; the header promises
that the results do not change beyond fp32 summation order, and for most knobs that no bit changes:
  * forward, `xcd_affinity`: which block serves which (level, chunk) -- the per-coordinate arithmetic
    does not depend on the block, so the features are bitwise those of the default;
  * forward, `fwd_pair` 0: one lane adds the corners in order instead of two lanes adding half each --
    another summation order, judged against float64 like the golden forward test;
  * table gradient (methods 0 / 2, f32 records): every contribution is the f32 product g * w turned into
    fixed point in a per-level unit, and the sums are int64.  Integer addition is associative, so how a
    level is cut (dense path or records, slices, splits, launches) changes no bit;
  * `bwd_lds_max_parts` moves levels to global f32 atomics: held per slot to the float64 bound of any
    sequential f32 accumulation;
  * `mlp_stagger`: team 1 of the 128-wide f32-MFMA decoder runs behind team 0; the teams own their tiles
    and the merge order is fixed, so no bit changes.
Knobs are set BEFORE a workspace is sized or a backward prepared (make_plan reads them) and restored in a
`finally`; at the end of the module every knob is back at its documented default.
"""
import contextlib

import numpy as np
import pytest
import torch

from conftest import REL_TOL, assert_close, load_golden
from yardstick import AFTER_ADAM_MAX_FACTOR, KNOB_DEFAULTS, assert_no_worse, cfg4_gradient_case
from oracle import detrand
from oracle import hashgrid as ohash
from oracle import mlp as omlp
from oracle import train as otrain

pytestmark = pytest.mark.gpu

U = 2.0 ** -24  # unit roundoff of f32
FIN4 = 16 * 1.4 ** 15
ACC_WORDS = 16384  # LDS accumulators of an accumulate workgroup (hashgrid_bwd.hip kAccWords)
MAX_PARTS = 256    # slices per level the binned path serves (kMaxParts)

F2_GOLDENS = ["enc_cfg2", "enc_cfg4", "enc_cfg5_4d", "enc_defaults_2d", "enc_v2_cfg5", "enc_v2_notebook"]
ALL_GOLDENS = F2_GOLDENS + ["enc_f4_small", "enc_v2_hashconfig"]


def _lib():
    from mri_interpolation_amd import _lib as lib
    return lib


def _knob_values():
    return {name: _lib().get_option(name) for name in KNOB_DEFAULTS}


@contextlib.contextmanager
def knobs(**values):
    """Set knobs for the body, restore the values read before in any case."""
    lib = _lib()
    saved = {name: lib.get_option(name) for name in values}
    try:
        for name, value in values.items():
            lib.set_option(name, value)
        yield
    finally:
        for name, value in saved.items():
            lib.set_option(name, value)


@pytest.fixture(scope="module")
def amd():
    from mri_interpolation_amd import _lib as lib, encoding, models, ops, trainer
    assert torch.cuda.is_available(), "these tests need the GPU"
    lib.load()
    assert _knob_values() == KNOB_DEFAULTS, "a knob was left off its default before this module"
    yield type("NS", (), dict(lib=lib, ops=ops, encoding=encoding, models=models, trainer=trainer))
    assert _knob_values() == KNOB_DEFAULTS, "a knob was left off its default by this module"


def cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------ grid cases
class Case:
    """A grid (encoder module), its float32 table, coordinates and incoming gradient (n, L * F)."""

    def __init__(self, enc, res, sizes, x, d_out):
        self.enc, self.res, self.sizes = enc, res, list(sizes)
        self.x, self.d_out = x, d_out  # CPU float32
        self.dim, self.F, self.L = enc.dim, enc.n_features_per_level, enc.n_levels
        self.xg, self.dg = cuda(x), cuda(d_out)
        self._f64 = None

    def f64(self):
        if self._f64 is None:
            self._f64 = ohash.table_gradient_f64(torch.as_tensor(self.x), torch.as_tensor(self.d_out),
                                                 self.sizes, self.res, self.F)
        return self._f64

    def parts(self, l):
        return -(-self.sizes[l] // (ACC_WORDS // self.F))

    def binned(self, l, method, lds_max_parts=KNOB_DEFAULTS["bwd_lds_max_parts"]):
        """make_plan: does level l take the binned (fixed-point) path?"""
        p = self.parts(l)
        return (self.dim <= 4 and self.F <= 4 and p <= MAX_PARTS
                and (method == 2 or (method == 0 and p <= lds_max_parts)))


def _golden_encoder(amd, name):
    fx = load_golden(name)
    c = dict(fx.meta["ctor"])
    cls = getattr(amd.encoding, c.pop("cls"))
    dim = c.pop("dim")
    for k in ("base_resolution", "finest_resolution"):
        if isinstance(c.get(k), list):
            c[k] = tuple(c[k])
    enc = cls(dim, **c)
    tabs = ohash.init_tables(enc.sizes, enc.n_features_per_level, fx.meta["table_seed"], fx.meta["table_scale"])
    with torch.no_grad():
        enc.table.copy_(torch.cat(tabs))
    res = [r[0] for r in enc.resolutions] if enc.isotropic else [list(r) for r in enc.resolutions]
    sizes = list(enc.sizes)
    assert sizes == fx.meta["sizes"]
    return fx, enc.cuda(), res, sizes


def golden_case(amd, name):
    fx, enc, res, sizes = _golden_encoder(amd, name)
    return Case(enc, res, sizes, np.asarray(fx["x"], np.float32), np.asarray(fx["d_out"], np.float32))


def random_case(amd, seed, dim, n_levels, log2t, base, finest, n, feats=2):
    """Seeded grid; coordinates up to one cell of the coarsest level outside [0, 1] on every axis (the
    reference extrapolates there), so that the two corners of a pair can lie in different slices."""
    enc = amd.encoding.MultiResHashGrid(dim, n_levels, feats, log2t, base, finest)
    res, sizes = ohash.resolutions_for(dim, n_levels, log2t, base, finest)
    assert list(enc.sizes) == list(sizes)
    with torch.no_grad():
        enc.table.copy_(torch.from_numpy(detrand.uniform(enc.table.numel(), seed, -0.5, 0.5)
                                         .reshape(enc.table.shape)))
    h = 1.0 / base
    x = detrand.uniform(n * dim, seed + 1, -h, 1.0 + h).reshape(n, dim).astype(np.float32)
    d = detrand.uniform(n * n_levels * feats, seed + 2, -1.0, 1.0).reshape(n, n_levels * feats)
    spread = detrand.uniform(n, seed + 3, -6.0, 2.0).reshape(n, 1)
    d = (d * np.exp2(spread)).astype(np.float32)
    return Case(enc.cuda(), res, sizes, x, d)


# ------------------------------------------------------------------------------ forward
FWD_RANDOM = [(1, 2), (5, 3), (8, 4), (9, 3), (16, 3)]  # (levels, dim): lpx / min_cnt of the affinity map
FWD_N = [1, 127, 128, 129, 70001, 1 << 18]


def encode_f64(x, tables, res, sizes):
    """oracle encode with the f32 cells and weights of the reference, the products and sums in float64."""
    out = []
    for t, r, size in zip(tables, res, sizes):
        slot, w = ohash.level_slots_and_weights(x, size, r)
        out.append((w.double().unsqueeze(-1) * t.double()[slot]).sum(dim=-2))
    return torch.cat(out, dim=-1)


def _forward_under_knobs(amd, enc, xg, want32, want64, what):
    fwd = amd.ops.hashgrid_forward
    base = fwd(enc.desc, xg, enc.table.data)
    base_fm = fwd(enc.desc, xg, enc.table.data, feature_major=True)
    with knobs(xcd_affinity=0):
        assert torch.equal(fwd(enc.desc, xg, enc.table.data), base), f"{what}: xcd_affinity 0"
        assert torch.equal(fwd(enc.desc, xg, enc.table.data, feature_major=True), base_fm), what
    with knobs(fwd_pair=0):
        single = fwd(enc.desc, xg, enc.table.data)
        assert torch.equal(fwd(enc.desc, xg, enc.table.data, feature_major=True).t(), single), what
        with knobs(xcd_affinity=0):
            assert torch.equal(fwd(enc.desc, xg, enc.table.data), single), f"{what}: fwd_pair 0, affinity 0"
    got = single.cpu().numpy()
    if want32 is not None:
        assert_close(got, want32, 1e-6, f"{what}: fwd_pair 0 against the golden")
    assert_close(got, want64, 1e-6, f"{what}: fwd_pair 0 against float64")
    assert_close(got, base.cpu().numpy(), 1e-6, f"{what}: fwd_pair 0 against the pair kernel")
    assert_close(base.cpu().numpy(), want64, 1e-6, f"{what}: default against float64")


@pytest.mark.parametrize("name", F2_GOLDENS)
def test_forward_knobs_on_the_golden_encoders(amd, name):
    fx, enc, res, sizes = _golden_encoder(amd, name)
    x = torch.as_tensor(np.asarray(fx["x"], np.float32))
    tabs = [enc.table.data[a:b].cpu() for a, b in (enc._row_span(l) for l in range(enc.n_levels))]
    _forward_under_knobs(amd, enc, cuda(x), fx["out"], encode_f64(x, tabs, res, sizes).numpy(), name)


@pytest.mark.parametrize("levels,dim", FWD_RANDOM)
def test_forward_knobs_on_random_grids(amd, levels, dim):
    for k, n in enumerate(FWD_N):
        seed = 5000 + 100 * levels + k
        log2t = 15 if levels > 1 else 12
        enc = amd.encoding.MultiResHashGrid(dim, levels, 2, log2t, 6, 150)
        res, sizes = ohash.resolutions_for(dim, levels, log2t, 6, 150)
        with torch.no_grad():
            enc.table.copy_(torch.from_numpy(detrand.uniform(enc.table.numel(), seed, -1, 1)
                                             .reshape(enc.table.shape)))
        enc = enc.cuda()
        x = torch.from_numpy(detrand.uniform(n * dim, seed + 1, -0.2, 1.2).reshape(n, dim).astype(np.float32))
        tabs = [enc.table.data[a:b].cpu() for a, b in (enc._row_span(l) for l in range(levels))]
        _forward_under_knobs(amd, enc, cuda(x), None, encode_f64(x, tabs, res, sizes).numpy(),
                             f"L{levels} D{dim} n {n}")


# ------------------------------------------------------------------------------ table gradient
# each knob on its own, then a few together; every entry bitwise equal to the default
BWD_SWEEP = ([dict(bwd_dense_max_parts=v) for v in (0, 1, 4, 64, 1 << 30)]
             + [dict(bwd_fuse_dense=v) for v in (0, 1)]
             + [dict(bwd_dense_blocks=v) for v in (1, 7, 96, 4096)]
             + [dict(bwd_blocks_per_level=v) for v in (1, 3, 64, 1024)]
             + [dict(xcd_affinity=v) for v in (0, 1)]
             + [dict(bwd_dense_max_parts=64, bwd_fuse_dense=0, bwd_dense_blocks=7),
                dict(bwd_dense_max_parts=0, bwd_blocks_per_level=1024),
                dict(bwd_dense_max_parts=1 << 30, bwd_dense_blocks=4096, xcd_affinity=0),
                dict(bwd_fuse_dense=0, bwd_blocks_per_level=3, bwd_dense_blocks=1),
                dict(bwd_dense_max_parts=8, bwd_blocks_per_level=1, bwd_dense_blocks=1)])

ADAM = dict(lr=5e-3, beta1=0.9, beta2=0.999, eps=1e-8, step=3, grad_scale=0.75)


def _bwd_paths(amd, case, method):
    """Every way of calling the table gradient, under the knobs set now: plain accumulate into a nonzero
    buffer, overwrite into garbage, two level groups, the prepared split, and the fused Adam step.  The
    workspace is sized here, after the knobs were set."""
    ops, enc, xg, dg = amd.ops, case.enc, case.xg, case.dg
    ws = torch.empty(ops.backward_workspace_bytes(enc.desc, xg.shape[0]) // 8 + 2, dtype=torch.int64,
                     device="cuda")
    g0 = torch.from_numpy(detrand.uniform(enc.table.numel(), 77, -1e-3, 1e-3).reshape(enc.table.shape)).cuda()
    out = {}
    acc = g0.clone()
    ops.hashgrid_backward(enc.desc, xg, dg, acc, method=method, ws=ws)
    out["accumulate"] = acc
    over = torch.full_like(g0, 7.0)
    ops.hashgrid_backward(enc.desc, xg, dg, over, method=method, overwrite=True, ws=ws)
    out["overwrite"] = over
    even = sum(1 << l for l in range(0, case.L, 2))
    odd = ((1 << case.L) - 1) & ~even
    split = torch.zeros_like(g0)
    ops.hashgrid_backward(enc.desc, xg, dg, split, method=method, level_mask=odd, ws=ws)
    ops.hashgrid_backward(enc.desc, xg, dg, split, method=method, level_mask=even, ws=ws)
    out["level_mask"] = split
    prep = torch.zeros_like(g0)
    ops.hashgrid_backward_prepare(enc.desc, xg, method=method, ws=ws)
    ops.hashgrid_backward(enc.desc, xg, dg, prep, method=method, prepared=True, level_mask=even, ws=ws)
    ops.hashgrid_backward(enc.desc, xg, dg, prep, method=method, prepared=True, level_mask=odd, ws=ws)
    out["prepared"] = prep
    p = enc.table.data.clone()
    m = torch.from_numpy(detrand.uniform(p.numel(), 78, -1e-4, 1e-4).reshape(p.shape)).cuda()
    v = torch.from_numpy(detrand.uniform(p.numel(), 79, 0.0, 1e-7).reshape(p.shape)).cuda()
    a = ADAM
    fused = ops.hashgrid_backward_adam(enc.desc, xg, dg, p, m, v, a["lr"], a["beta1"], a["beta2"], a["eps"],
                                       a["step"], a["grad_scale"], method=method, ws=ws)
    all_binned = all(case.binned(l, method, amd.lib.get_option("bwd_lds_max_parts")) for l in range(case.L))
    assert fused == all_binned, "fused Adam serves exactly the grids whose levels are all binned"
    if fused:
        out["adam"] = torch.cat([p, m, v], dim=1)
    torch.cuda.synchronize()
    return out, g0


def _check_exact_bound(case, grad, what):
    """Per slot: |grad - exact| <= U (sum |w g| + |sum|) + 2 units of the fixed point, the bound of the f32
    records (test_record_formats_per_slot_against_float64), with the unit of level_exponent; and no slot
    the reference leaves empty is written."""
    n = case.x.shape[0]
    log_n = int(n).bit_length()
    for l, (total, mag, count) in enumerate(case.f64()):
        lo, hi = case.enc._row_span(l)
        got = grad[lo:hi].double().cpu()
        gmax = float(np.abs(case.d_out[:, l * case.F:(l + 1) * case.F]).max())
        if gmax == 0.0:
            assert float(got.abs().max()) == 0.0
            continue
        E = int(np.floor(np.log2(gmax)))
        unit = 2.0 ** (E + 1 + log_n - 61)
        bound = U * (mag + total.abs()) * 1.001 + 2.0 * unit * count.double().unsqueeze(1)
        worst = float(((got - total).abs() - bound).max())
        assert worst <= 0.0, f"{what} level {l}: a slot exceeds its float64 bound by {worst:.3e}"
        if (count == 0).any():
            assert float(got[count == 0].abs().max()) == 0.0, f"{what} level {l}: stray slot"


_CASES = {}


def bwd_case(amd, key):
    if key not in _CASES:
        if key in ALL_GOLDENS:
            _CASES[key] = golden_case(amd, key)
        elif key == "cfg4_full":  # BASELINE config 4 at its full batch
            enc = amd.encoding.MultiResHashGrid(3, 16, 2, 19, 16, FIN4)
            res, sizes = ohash.resolutions_for(3, 16, 19, 16, FIN4)
            x, d = cfg4_gradient_case(1 << 18, 71)
            _CASES[key] = Case(enc.cuda(), res, sizes, x.numpy(), d.numpy())
        else:
            seed, dim, levels, log2t, base, finest, n = BWD_RANDOM[key]
            _CASES[key] = random_case(amd, seed, dim, levels, log2t, base, finest, n)
    return _CASES[key]


# (seed, D, levels, log2 T, base, finest, n): n in {1, 33, 4097, 70001}, D 2..4; table sizes res^D below the
# cap (1331, 2197, ...: not powers of two), levels cut into 1 to 123 slices
BWD_RANDOM = {"d3_n1": (11, 3, 8, 17, 11, 400, 1), "d2_n33": (12, 2, 6, 16, 20, 900, 33),
              "d4_n4097": (13, 4, 5, 18, 5, 40, 4097), "d3_n70001": (14, 3, 12, 19, 11, 700, 70001),
              "d3_odd_sizes": (15, 3, 8, 20, 11, 100, 70001)}
BWD_KEYS = ALL_GOLDENS + ["cfg4_full"] + list(BWD_RANDOM)


@pytest.mark.parametrize("method", [0, 2])
@pytest.mark.parametrize("key", BWD_KEYS)
def test_table_gradient_is_bitwise_the_default_under_every_knob(amd, key, method):
    case = bwd_case(amd, key)
    if key == "d3_odd_sizes":
        assert any(s & (s - 1) for s in case.sizes) and any(case.parts(l) > 1 for l in range(case.L))
    with knobs(**KNOB_DEFAULTS):
        ref, _ = _bwd_paths(amd, case, method)
    binned = [case.binned(l, method) for l in range(case.L)]
    exact = torch.zeros_like(ref["accumulate"], dtype=torch.bool)
    for l in range(case.L):
        lo, hi = case.enc._row_span(l)
        exact[lo:hi] = binned[l]
    # the default against float64: every binned level within the bound of exact fixed-point sums
    if all(binned):
        _check_exact_bound(case, ref["overwrite"], f"{key} method {method} default")
    # the ways of calling it agree with each other (levels on global atomics add in no fixed order)
    assert torch.equal(ref["level_mask"][exact], ref["prepared"][exact])
    assert torch.equal(ref["level_mask"][exact], ref["overwrite"][exact])
    for setting in BWD_SWEEP:
        with knobs(**setting):
            got, _ = _bwd_paths(amd, case, method)
        for path, want in ref.items():
            g = got[path]
            if path == "adam":
                assert torch.equal(g, want), f"{key} method {method} {setting}: {path}"
                continue
            assert torch.equal(g[exact], want[exact]), f"{key} method {method} {setting}: {path}"
            if not exact.all():  # atomic levels: the same sums in another order
                assert_close(g[~exact].cpu().numpy(), want[~exact].cpu().numpy(), REL_TOL,
                             f"{key} {setting} {path} atomic levels")


@pytest.mark.parametrize("key", ["cfg4_full", "enc_cfg5_4d", "enc_f4_small", "d3_n70001"])
@pytest.mark.parametrize("lds_max_parts", [0, 8, 256])
def test_levels_over_the_lds_limit_take_atomics_within_the_f32_bound(amd, key, lds_max_parts):
    """Method 0 with `bwd_lds_max_parts`: levels of more slices take global f32 atomics.  Those are held per
    slot to the float64 bound of a sequential f32 accumulation (k products and k - 1 additions); the levels
    still binned stay bitwise those of the default; nothing lands in a slot no corner hashes to and no slot
    the reference fills is lost."""
    case = bwd_case(amd, key)
    with knobs(**KNOB_DEFAULTS):
        ref = torch.zeros_like(case.enc.table.data)
        amd.ops.hashgrid_backward(case.enc.desc, case.xg, case.dg, ref, method=0)
    with knobs(bwd_lds_max_parts=lds_max_parts):
        got = torch.zeros_like(case.enc.table.data)
        amd.ops.hashgrid_backward(case.enc.desc, case.xg, case.dg, got, method=0)
    torch.cuda.synchronize()
    took_atomics = 0
    for l, (total, mag, count) in enumerate(case.f64()):
        lo, hi = case.enc._row_span(l)
        g = got[lo:hi].double().cpu()
        if case.binned(l, 0, lds_max_parts):
            assert torch.equal(got[lo:hi], ref[lo:hi]), f"{key} level {l}: binned level changed"
            continue
        took_atomics += 1
        k = count.double().unsqueeze(1)
        bound_atomic = U * mag * (k + 1.0) * 1.001
        worst = float(((g - total).abs() - bound_atomic).max())
        assert worst <= 0.0, f"{key} level {l}: a slot exceeds the f32-atomics bound by {worst:.3e}"
        nz = g.abs().sum(dim=1) != 0
        assert not (nz & (count == 0)).any(), f"{key} level {l}: stray slot"
        big = total.abs().sum(dim=1) > 1e-9 * float(total.abs().max())
        assert nz[big].all(), f"{key} level {l}: lost slot"
        assert_close(g.numpy(), total.numpy(), REL_TOL, f"{key} level {l}")
    expected = sum(not case.binned(l, 0, lds_max_parts) for l in range(case.L))
    assert took_atomics == expected
    if lds_max_parts == 0:
        assert took_atomics == case.L


# ------------------------------------------------------------------------------ decoder
@pytest.mark.parametrize("n,k_in", [(1 << 18, 32), (70001, 32), (33, 32), (5000, 7), (1, 32), (65, 32)])
def test_decoder_stagger_is_bitwise_lockstep(amd, n, k_in):
    """mlp_x3 0, H 128 (the two-team f32-MFMA kernel): team 1 `mlp_stagger` segments behind team 0.  The
    teams own their tiles and the slab merge has a fixed order, so predictions, loss, every parameter
    gradient and d_x are those of lockstep, bit for bit -- also where a workgroup's second team has no
    tile (n = 1, 33, 65) -- and lockstep itself is within REL_TOL of the float64 decoder."""
    H = 128
    ops = amd.ops
    torch.manual_seed(n + k_in)
    params = [(torch.randn(H, k_in, device="cuda") * 0.2, torch.randn(H, device="cuda") * 0.1),
              (torch.randn(H, H, device="cuda") * 0.1, torch.randn(H, device="cuda") * 0.1),
              (torch.randn(1, H, device="cuda") * 0.1, torch.randn(1, device="cuda") * 0.1)]
    x = (torch.rand(k_in, n, device="cuda") * 2 - 1).contiguous()
    t = torch.rand(n, 1, device="cuda")

    def run():
        grads = [(torch.zeros_like(w_), torch.zeros_like(b_)) for w_, b_ in params]
        dx, y, loss = torch.empty_like(x), torch.empty(n, 1, device="cuda"), torch.zeros(1, device="cuda")
        ops.tiny_mlp_train(x, t, params, grads, loss, d_x=dx, y=y, overwrite=True)
        torch.cuda.synchronize()
        return [y, loss, dx] + [g_ for wb in grads for g_ in wb]

    with knobs(mlp_x3=0, mlp_stagger=0):
        ref = run()
    for stagger in (1, 2, 6, 8):
        with knobs(mlp_x3=0, mlp_stagger=stagger):
            got = run()
        for i, (u, v) in enumerate(zip(got, ref)):
            assert torch.equal(u, v), f"stagger {stagger}: output {i} differs from lockstep"
    # lockstep against the float64 decoder (rows at a ReLU kink may flip the mask in either evaluation:
    # judged on the forward and the loss, where one row moves the result by 1e-7 at most)
    p64 = [(w_.double().cpu(), b_.double().cpu()) for w_, b_ in params]
    y64 = omlp.relu_mlp_forward(x.t().double().cpu(), p64, False)
    assert_close(ref[0].cpu().numpy(), y64.numpy(), REL_TOL, "lockstep prediction")
    loss64 = float(((y64 - t.double().cpu()) ** 2).mean())
    assert abs(float(ref[1]) - loss64) <= REL_TOL * loss64


# ------------------------------------------------------------------------------ trainer
TRAINER_EXACT = [dict(xcd_affinity=0), dict(bwd_dense_max_parts=0), dict(bwd_dense_max_parts=1 << 30),
                 dict(bwd_fuse_dense=0), dict(bwd_dense_blocks=7), dict(bwd_blocks_per_level=1024),
                 dict(bwd_blocks_per_level=1), dict(mlp_x3=0, mlp_stagger=6)]


def _cfg4_like(amd, seed=23):
    """A config-4-shaped model: 16 levels, log2 T 15, ReLU 32 -> 128 -> 128 -> 1; the f32 oracle copy."""
    finest = 16 * 1.4 ** 15
    model = otrain.HashMlpModel(3, 16, 2, 15, 16, finest, [128, 128], seed=seed, table_scale=1e-2)
    net = amd.models.HashMLP(3, 16, 2, 15, 16, finest, dim_hidden=128, n_layers=3,
                             activation=torch.nn.ReLU, batch_norm=False, final_activation=False, lr=5e-3)
    with torch.no_grad():
        net.encoder.table.copy_(torch.cat(model.tables))
        for blk, (w, b) in zip(net.decoder, model.mlp):
            blk[0].weight.copy_(w)
            blk[0].bias.copy_(b)
    return model, net.cuda()


def _batches(n=70001, steps=3):
    return [(torch.from_numpy(detrand.uniform(n * 3, 300 + s, 0.0, 1.0).reshape(n, 3)),
             torch.from_numpy(detrand.uniform(n, 400 + s, 0.0, 1.0).reshape(n, 1))) for s in range(steps)]


def _train(amd, batches, **setting):
    """3 Adam steps through FusedStep, built AFTER the knobs are set (its count-ahead stage plans the next
    step's backward with them) and dropped before they are restored."""
    with knobs(**setting):
        model, net = _cfg4_like(amd)
        step = amd.trainer.FusedStep(net, net.configure_optimizers())
        assert step.use_tiny
        losses = [float(step.train_step(x.cuda(), y.cuda())) for x, y in batches]
        torch.cuda.synchronize()
        flat = step.flat.param.detach().clone()
        table = net.encoder.table.data.clone()
        mlp = [(blk[0].weight.data.clone(), blk[0].bias.data.clone()) for blk in net.decoder]
        del step
    return model, losses, flat, table, mlp


def test_trainer_steps_are_bitwise_the_default_under_the_exact_knobs(amd):
    batches = _batches()
    _, losses, flat, _, _ = _train(amd, batches, **KNOB_DEFAULTS)
    for setting in TRAINER_EXACT:
        if setting.get("mlp_x3") == 0:  # another decoder kernel: compare with its own lockstep run
            _, ref_losses, ref_flat, _, _ = _train(amd, batches, mlp_x3=0)
        else:
            ref_losses, ref_flat = losses, flat
        _, got_losses, got_flat, _, _ = _train(amd, batches, **setting)
        assert got_losses == ref_losses, setting
        assert torch.equal(got_flat, ref_flat), setting


def test_trainer_steps_with_the_single_lane_forward_are_no_worse_than_the_oracle(amd):
    batches = _batches()
    model, losses, _, table, mlp = _train(amd, batches, fwd_pair=0)
    model64 = otrain.as_double(model)  # float64 yardstick, copied BEFORE the f32 oracle steps
    ref_losses, _ = otrain.train_steps(model, batches, 5e-3)
    otrain.train_steps(model64, [(x.double(), y.double()) for x, y in batches], 5e-3)
    for got, want in zip(losses, ref_losses):
        assert abs(got - float(want)) <= REL_TOL * float(want)
    table = table.cpu()
    row = 0
    for level, (t32, t64) in enumerate(zip(model.tables, model64.tables)):
        assert_no_worse(table[row:row + t32.shape[0]].numpy(), t32.numpy(), t64.numpy(),
                        f"table level {level} after Adam", max_factor=AFTER_ADAM_MAX_FACTOR)
        row += t32.shape[0]
    for (w, b), (w32, b32), (w64, b64) in zip(mlp, model.mlp, model64.mlp):
        assert_no_worse(w.cpu().numpy(), w32.numpy(), w64.numpy(), "decoder weight after Adam",
                        max_factor=AFTER_ADAM_MAX_FACTOR)
        assert_no_worse(b.cpu().numpy(), b32.numpy(), b64.numpy(), "decoder bias after Adam",
                        max_factor=AFTER_ADAM_MAX_FACTOR)
