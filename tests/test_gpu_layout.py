"""Every entry point of include/mri_inr.h on the OTHER side of its alignment predicates, under guard bands.

The kernels choose between 16-byte and 4-byte accesses from a pointer's alignment, a leading dimension and the
end of a row range; contiguous, freshly allocated tensors only ever reach the 16-byte side.  Here every pointer
and leading-dimension argument is placed (tests/layout.py) at offsets of 1, 2, 3 floats and at leading dimensions
width + 1, + 3, + 4 -- each argument on its own, all together, and all aligned -- with row counts = 0..3 (mod 4)
that hold a full tile and a ragged tail.  Every case is held to:
  * the op's float64 / oracle reference, at the criterion the op's own test uses;
  * the all-aligned call on the same values: torch.equal where the two branches differ in access width only,
    1e-6 (the bar test_linear_forward_backward sets between layout variants) where the order of a sum differs;
  * guard bands: not one float outside an output's or an input's logical elements is written;
  * inputs bit-identical after the call.
Arguments an entry point refuses instead (16-byte aligned by contract) are shown to be refused by the host-side
check, before the first launch: RuntimeError naming the argument, outputs untouched, the aligned call passes.

Inventory, from reading csrc/ (a: 16-byte and 4-byte path chosen by a predicate; b: refused by MRI_REQUIRE unless
16-byte aligned; c: 4-byte accesses only).  No argument is left with an unchecked 16-byte access.
  mri_hashgrid_forward            x c | table b (F = 2, 4; c otherwise) | out + strides a (8-byte row store, F = 2)
  mri_hashgrid_forward_signal     x c | table b | out, out_ld, slice start a
  mri_hashgrid_backward*, _prepare x c | d_out + strides a (dense levels, feature-major) | d_table c | workspace b
  mri_hashgrid_backward_adam      as above | table, exp_avg, exp_avg_sq c
  mri_hashgrid_backward_input     all c
  mri_hash_tiny_mlp_train         table b | coords, target, d_enc, parameters, gradients c
  mri_linear_forward              x + strides a | weight a | bias c | y, ldy a | deriv, ldd a
  mri_linear_backward_data        dy, lddy a | weight a | deriv, ldd a (n <= 4) / c | dx + strides a
  mri_linear_backward_weight      dy, lddy a | x + strides a | d_weight, d_bias c (atomics)
  mri_apply_deriv, mri_frequency_*, mri_mse_loss, mri_gather_batch, mri_sample_indices, mri_shallow_mlp_*   all c
  mri_tiny_mlp_* (bf16 pipe)      all c
  mri_tiny_mlp_* (f32 MFMA)       x, x_ld a | w2 b (128-wide) / c (64-wide) | everything else c
  mri_siren_forward, _forward_loss, _backward   weight, act, deriv, dz, dz_last, workspace b | x, y, target, dy, bias,
                                  gradients c
  mri_modsiren_forward, _forward_loss, _backward   act, hid, dcos, sn, dzs, dzm, workspace b | everything else c
  mri_psf_expand                  x_psf a | x, offsets c;   mri_psf_reduce, _broadcast, _mse_loss   all c
  mri_bn_stats, _act_forward, _act_backward   z, y, dy, dz + leading dimensions a | workspace b | the rest c
  mri_adam_step                   the four buffers a (head, 16-byte body, tail) and b (one offset in a 16-byte line)
  mri_fused_step                  param / grad / moments a (`fold`, else conversion launch + mri_adam_step) | table b
Inventoried by reading only, without a case here: mri_hashgrid_backward_adam, _backward_input, _backward_scaled and
_prepare (they share mri_hashgrid_backward's kernels and checks; _backward_scaled and _prepare run inside the
mri_fused_step case), mri_tiny_mlp_train_overlapped (its w2 refusal is mri_tiny_mlp_train_slice's, tested; the call
itself waits on a producer and stays out of a layout test), mri_sample_indices, mri_tiny_mlp_train_dx_absmax.
What a workspace may HOLD and how large it must be (exact size between guards, dirty contents, reuse by another shape)
is tests/test_gpu_workspace.py's subject; here a workspace is only shown to be refused off a 16-byte boundary.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import REL_TOL, assert_close
from layout import OFFSETS, Placer, place, ptr, variants
from yardstick import assert_no_worse
from oracle import detrand
from oracle import hashgrid as ohash
from oracle import mlp as omlp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    from mri_interpolation_amd import _lib, ops
    assert torch.cuda.is_available(), "these tests need the GPU"
    _lib.load()
    saved = {k: _lib.get_option(k) for k in ("fwd_pair", "mlp_x3", "bwd_records", "siren_rows")}
    yield type("NS", (), dict(lib=_lib, ops=ops, call=staticmethod(_lib.call), stream=staticmethod(ops._stream)))
    for k, v in saved.items():
        _lib.set_option(k, v)


@pytest.fixture
def option(amd):
    """set(name, value) for the duration of one test."""
    before = {}

    def set_(name, value):
        before.setdefault(name, amd.lib.get_option(name))
        amd.lib.set_option(name, value)

    yield set_
    for k, v in before.items():
        amd.lib.set_option(k, v)


def uniform(shape, seed, lo=-1.0, hi=1.0):
    return torch.from_numpy(detrand.uniform(int(np.prod(shape)), seed, lo, hi).reshape(shape).copy())


def cpu(t):
    return t.detach().cpu().clone()


def over_layouts(widths, run, reference, same_bits, lds=True):
    """run(Placer) -> {name: tensor} under every layout of `widths`; reference(name, got, tag) judges one output
    against the high-precision result; against the aligned call: torch.equal if same_bits (True, or the set of
    output names that are bitwise) else 1e-6."""
    aligned = None
    for tag, layout in variants(widths, lds):
        p = Placer(layout, tag)
        got = {k: cpu(v) for k, v in run(p).items()}
        p.verify()
        for name, value in got.items():
            reference(name, value, tag)
        if aligned is None:
            aligned = got
            continue
        for name, value in got.items():
            if same_bits is True or (same_bits and name in same_bits):
                assert torch.equal(value, aligned[name]), f"{tag}: {name} differs from the aligned call"
            else:
                assert_close(value.numpy(), aligned[name].numpy(), 1e-6, f"{tag}: {name} against the aligned call")


def refused(call, word, outputs=()):
    """The host-side check refuses `call` with a message that names the argument; no output was touched."""
    with pytest.raises(RuntimeError, match=word):
        call()
    for name, check in outputs:
        check(what=f"after the refusal: {name}")


# ================================================================================================ the helper
def test_guard_bands_see_a_stray_store():
    """place() itself: alignment, padding columns, and a write one float past a row is reported."""
    for off in (0,) + OFFSETS:
        view, check = place(torch.zeros(3, 5), off, ld=7)
        assert view.data_ptr() % 16 == 4 * off and view.stride() == (7, 1)
        check(unchanged=True)
        view.fill_(1.0)  # the logical elements may change
        check()
        with pytest.raises(AssertionError, match="input was modified"):
            check(unchanged=True)
        view.as_strided((1,), (1,), view.storage_offset() + 5).fill_(0.0)  # a padding column
        with pytest.raises(AssertionError, match="outside the tensor"):
            check()
    vec, check = place(torch.zeros(9), 2)
    vec.as_strided((1,), (1,), vec.storage_offset() + 9).fill_(0.0)  # one past the end
    with pytest.raises(AssertionError, match="outside the tensor"):
        check()


# ================================================================================================ linear layers
# linear.hip: operand load mode (16-byte loads along the unit-stride axis), staged 16-byte epilogue; linear_small.hip:
# small_n_forward_kernel / small_n_backward_data_kernel `vec`.  m = one 128-row tile + a ragged tail, = 1..0 (mod 4).
LINEAR_M = [129, 130, 131, 132]
LINEAR_NK = [(64, 32), (65, 33), (1, 64), (4, 256), (128, 3), (128, 8)]
ACT_CODE = {"identity": 0, "relu": 1, "sine": 2, "gelu": 3}


@functools.lru_cache(maxsize=None)
def linear_case(m, n, k, act):
    """x, W, b (ranges of test_linear_forward_backward), dy, a derivative matrix g, and the float64 results."""
    w0 = 30.0 if act == "sine" else 1.0
    bound = 1.0 / np.sqrt(k) if act != "sine" else np.sqrt(6.0 / k) / 30.0
    x, w, b = uniform((m, k), 1), uniform((n, k), 2, -bound, bound), uniform((n,), 3, -bound, bound)
    dy, g = uniform((m, n), 4), uniform((m, k), 5)
    z = w0 * (x.double() @ w.double().T + b.double())
    zr = z.clone().requires_grad_(True)
    y = {"identity": lambda t: t, "relu": torch.relu, "sine": torch.sin, "gelu": F.gelu}[act](zr)
    y.sum().backward()
    want = dict(y=y.detach(), deriv=zr.grad * w0, dx=dy.double() @ w.double(), dw=dy.double().T @ x.double(),
                db=dy.double().sum(0))
    want["dx_mul"] = want["dx"] * g.double()
    want["dx_mask"] = torch.where(g > 0, want["dx"], torch.zeros_like(want["dx"]))
    return dict(x=x, w=w, b=b, dy=dy, g=g, w0=w0), want


def linear_reference(want, rename=None):
    def judge(name, got, tag):
        assert_close(got.numpy(), want[(rename or {}).get(name, name)].numpy(), REL_TOL, f"{tag}: {name}")
    return judge


@pytest.mark.parametrize("m", LINEAR_M)
@pytest.mark.parametrize("n,k", LINEAR_NK)
def test_linear_forward(amd, m, n, k):
    # 1e-6 against the aligned call: small_n's 16-byte path sums four k per lane, its 4-byte path one; the staged
    # epilogue evaluates the sine in pairs (sincos_fast2), the direct one singly
    for act in ("relu", "sine"):
        case, want = linear_case(m, n, k, act)
        with_deriv = act == "sine"
        for feature_major in (False, True):
            def run(p):
                xs = p.inp("x", case["x"].T.contiguous() if feature_major else case["x"])
                w, b = p.inp("w", case["w"].reshape(-1)), p.inp("b", case["b"])
                y = p.out("y", (m, n))
                d = p.out("deriv", (m, n)) if with_deriv else None
                xrs, xcs = (1, xs.stride(0)) if feature_major else (xs.stride(0), 1)
                amd.call("mri_linear_forward", ptr(xs), xrs, xcs, ptr(w), ptr(b), m, n, k, ACT_CODE[act],
                         case["w0"], ptr(y), y.stride(0), ptr(d), d.stride(0) if with_deriv else 0, amd.stream())
                return dict(y=y, deriv=d) if with_deriv else dict(y=y)
            widths = dict(x=m if feature_major else k, w=None, b=None, y=n)
            if with_deriv:
                widths["deriv"] = n
            over_layouts(widths, run, linear_reference(want), same_bits=False)


@pytest.mark.parametrize("m", LINEAR_M)
@pytest.mark.parametrize("n,k", LINEAR_NK)
def test_linear_backward_data(amd, m, n, k):
    # 1e-6: the two layouts of dx run different kernels at tiny widths; same-kernel variants only change widths
    case, want = linear_case(m, n, k, "relu")
    for mode, key in ((0, "dx"), (1, "dx_mul"), (2, "dx_mask")):
        def run(p):
            dy, w = p.inp("dy", case["dy"]), p.inp("w", case["w"].reshape(-1))
            g = p.inp("deriv", case["g"]) if mode else None
            dx = p.out("dx", (m, k))
            amd.call("mri_linear_backward_data", ptr(dy), dy.stride(0), ptr(w), m, n, k, mode, ptr(g),
                     g.stride(0) if mode else 0, ptr(dx), dx.stride(0), 1, amd.stream())
            return dict(dx=dx)
        widths = dict(dy=n, w=None, dx=k)
        if mode:
            widths["deriv"] = k
        over_layouts(widths, run, linear_reference(want, {"dx": key}), same_bits=False)

    def run_fm(p):  # feature-major dx (k, m): what the fused trainer hands the encoder
        dy, w = p.inp("dy", case["dy"]), p.inp("w", case["w"].reshape(-1))
        dx = p.out("dx", (k, m))
        amd.call("mri_linear_backward_data", ptr(dy), dy.stride(0), ptr(w), m, n, k, 0, None, 0, ptr(dx), 1,
                 dx.stride(0), amd.stream())
        return dict(dx=dx)
    over_layouts(dict(dy=n, w=None, dx=m), run_fm,
                 lambda name, got, tag: assert_close(got.T.numpy(), want["dx"].numpy(), REL_TOL, f"{tag}: dx (k, m)"),
                 same_bits=False)


@pytest.mark.parametrize("m", LINEAR_M)
@pytest.mark.parametrize("n,k", LINEAR_NK)
def test_linear_backward_weight(amd, m, n, k):
    # 1e-6: float atomics add the batch splits in no fixed order
    case, want = linear_case(m, n, k, "relu")
    for feature_major in (False, True):
        def run(p):
            dy = p.inp("dy", case["dy"])
            xs = p.inp("x", case["x"].T.contiguous() if feature_major else case["x"])
            dw, db = p.out("dw", (n * k,), 0.0), p.out("db", (n,), 0.0)
            xrs, xcs = (1, xs.stride(0)) if feature_major else (xs.stride(0), 1)
            amd.call("mri_linear_backward_weight", ptr(dy), dy.stride(0), ptr(xs), xrs, xcs, m, n, k, ptr(dw),
                     ptr(db), amd.stream())
            return dict(dw=dw.reshape(n, k), db=db)
        over_layouts(dict(dy=n, x=m if feature_major else k, dw=None, db=None), run, linear_reference(want),
                     same_bits=False)


def test_apply_deriv(amd):
    m, n = 131, 65
    case, _ = linear_case(m, 65, 33, "relu")
    g = uniform((m, n), 6)
    for mode in (1, 2):
        want = case["dy"] * g if mode == 1 else torch.where(g > 0, case["dy"], torch.zeros(()))

        def run(p):
            dy, gg = p.out("dy", (m, n)), p.inp("deriv", g)
            dy.copy_(case["dy"])
            amd.call("mri_apply_deriv", ptr(dy), dy.stride(0), mode, ptr(gg), gg.stride(0), m, n, amd.stream())
            return dict(dy=dy)
        # same bits: one multiply per element, 4-byte accesses whatever the layout
        over_layouts(dict(dy=n, deriv=n), run, lambda name, got, tag: torch.equal(got, want) or pytest.fail(tag),
                     same_bits=True)


# ================================================================================================ BatchNorm
BN_ACT = {"identity": 0, "gelu": 3}


@functools.lru_cache(maxsize=None)
def bn_case(n, C):
    z, dy = uniform((n, C), 21, -1.4, 2.0), uniform((n, C), 22)
    gamma, beta = uniform((C,), 23, 0.5, 1.5), uniform((C,), 24, -0.2, 0.2)
    rm, rv = uniform((C,), 25, -0.1, 0.1), uniform((C,), 26, 0.5, 1.5)
    want = {}
    for act, fn in (("identity", lambda u: u), ("gelu", F.gelu)):
        z64, g64, b64 = (t.double().clone().requires_grad_(True) for t in (z, gamma, beta))
        rm64, rv64 = rm.double().clone(), rv.double().clone()
        y = fn(F.batch_norm(z64, rm64, rv64, g64, b64, True, 0.1, 1e-5))
        y.backward(dy.double())
        u = gamma.double() * (z.double() - rm.double()) / torch.sqrt(rv.double() + 1e-5) + beta.double()
        want[act] = dict(y=y.detach(), running_mean=rm64, running_var=rv64, dz=z64.grad, d_gamma=g64.grad,
                         d_beta=b64.grad, y_eval=fn(u),
                         save=torch.stack([z.double().mean(0), 1 / torch.sqrt(z.double().var(0, unbiased=False) + 1e-5)]))
    return dict(z=z, dy=dy, gamma=gamma, beta=beta, rm=rm, rv=rv), want


@pytest.mark.parametrize("n", [130, 131])
@pytest.mark.parametrize("C", [4, 64, 66])
def test_batchnorm(amd, n, C):
    """mri_bn_stats, mri_bn_act_forward (training and eval form), mri_bn_act_backward: the three `vec` predicates
    of batchnorm.hip (C % 4, every leading dimension, every matrix pointer)."""
    # 1e-6 against the aligned call: the order of the float64 column sums is fixed by (n, C, alignment) -- the
    # 16-byte path cuts the tile differently -- so the rounded f32 statistics may differ in the last bit
    case, want_all = bn_case(n, C)
    ws_bytes = amd.lib.load().mri_bn_workspace_bytes(n, C)
    ws = torch.empty(ws_bytes // 4 + 4, device="cuda")
    for act, code in BN_ACT.items():
        want = want_all[act]

        def run(p, ws_off=0, only=None):
            wsp = ws[ws_off:]
            z, dy = p.inp("z", case["z"]), p.inp("dy", case["dy"])
            gamma, beta = p.inp("gamma", case["gamma"]), p.inp("beta", case["beta"])
            rm, rv, save = p.out("rm", (C,)), p.out("rv", (C,)), p.out("save", (2 * C,))
            rm.copy_(case["rm"]), rv.copy_(case["rv"])
            rm0, rv0 = p.inp("rm0", case["rm"]), p.inp("rv0", case["rv"])
            y, y_eval, dz = p.out("y", (n, C)), p.out("y_eval", (n, C)), p.out("dz", (n, C))
            dg, db = p.out("d_gamma", (C,)), p.out("d_beta", (C,))
            st = amd.stream()
            if only in (None, "stats"):
                amd.call("mri_bn_stats", ptr(z), z.stride(0), n, C, 0.1, 1e-5, ptr(rm), ptr(rv), None, ptr(save),
                         ptr(wsp), ws_bytes, st)
            if only is None:
                amd.call("mri_bn_act_forward", ptr(z), z.stride(0), n, C, ptr(save), None, None, 1e-5, ptr(gamma),
                         ptr(beta), code, ptr(y), y.stride(0), st)
                amd.call("mri_bn_act_forward", ptr(z), z.stride(0), n, C, None, ptr(rm0), ptr(rv0), 1e-5, ptr(gamma),
                         ptr(beta), code, ptr(y_eval), y_eval.stride(0), st)
            if only in (None, "backward"):
                amd.call("mri_bn_act_backward", ptr(dy), dy.stride(0), ptr(z), z.stride(0), n, C, ptr(save), ptr(gamma),
                         ptr(beta), code, ptr(dz), dz.stride(0), ptr(dg), ptr(db), 1, ptr(wsp), ws_bytes, st)
            return dict(y=y, y_eval=y_eval, dz=dz, d_gamma=dg, d_beta=db, running_mean=rm, running_var=rv,
                        save=save.reshape(2, C))

        def judge(name, got, tag):  # test_kernels_against_float64 / test_eval_form: REL_TOL of float64
            assert_close(got.numpy(), want[name].numpy(), REL_TOL, f"({n}, {C}) {act} {tag}: {name}")
        over_layouts(dict(z=C, dy=C, y=C, y_eval=C, dz=C, gamma=None, beta=None, save=None, d_gamma=None, rm=None),
                     run, judge, same_bits=False)
        for entry in ("stats", "backward"):  # the workspace is 16-byte aligned by contract: each entry point on its own
            pl = Placer({}, f"{entry}: workspace + 1")
            refused(lambda: run(pl, ws_off=1, only=entry), "workspace.*16-byte aligned")
            for name, check, is_input in pl.checks:  # (rm / rv were filled by the test itself)
                check(unchanged=name not in ("rm", "rv"), what=f"{entry}: workspace + 1 refused: {name}")
            pl = Placer({}, "aligned call after the refusal")
            for name, value in run(pl).items():
                judge(name, cpu(value), pl.tag)


# ================================================================================================ hash grid
# D = 3, F = 2, five levels, T = 2^12.  Base 4 puts every level at an even table row; base 5 (125 rows in level 0)
# puts every later level at an ODD row, 8-byte aligned only: the forward must not fetch 16-byte row pairs there.
GRIDS = {"even": (4, 64), "odd": (5, 80)}
HASH_N = [4097, 4098, 4099, 4100]


@functools.lru_cache(maxsize=None)
def hash_case(grid, n):
    base, finest = GRIDS[grid]
    res, sizes = ohash.resolutions_for(3, 5, 12, base, finest)
    tables = ohash.init_tables(sizes, 2, 77, 0.5)
    x = uniform((n, 3), 31, 0.0, 1.0)
    d_out = uniform((n, 10), 32) * torch.exp2(uniform((n, 1), 33, -6.0, 2.0))
    out = ohash.encode(x, tables, res)
    grad = ohash.table_gradient_f64(x, d_out, sizes, res, 2)
    return dict(res=res, sizes=sizes, table=torch.cat(tables), x=x, d_out=d_out, out=out, grad=[g[0] for g in grad])


def hash_desc(amd, case):
    return amd.ops.make_grid_desc(3, [[r] * 3 for r in case["res"]], case["sizes"], 2)


@pytest.mark.parametrize("n", HASH_N)
@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("pair", [1, 0])
def test_hashgrid_forward(amd, option, pair, grid, n):
    """mri_hashgrid_forward, both F = 2 kernels ("fwd_pair"), row-major and feature-major `out`."""
    option("fwd_pair", pair)
    case = hash_case(grid, n)
    desc = hash_desc(amd, case)
    table = case["table"].cuda()
    for feature_major in (False, True):
        def run(p):
            x = p.inp("x", case["x"].reshape(-1))
            out = p.out("out", (10, n) if feature_major else (n, 10))
            ld = out.stride(0)
            sl, sr, sf = (2 * ld, 1, ld) if feature_major else (2, ld, 1)
            amd.call("mri_hashgrid_forward", C.byref(desc), ptr(x), n, ptr(table), ptr(out), sl, sr, sf, amd.stream())
            return dict(out=out.T if feature_major else out)
        # same bits: the arithmetic per (coordinate, level) does not depend on where the result is stored;
        # 1e-6 of the oracle is test_encoder_forward_golden's bar
        over_layouts(dict(x=None, out=n if feature_major else 10), run,
                     lambda name, got, tag: assert_close(got.numpy(), case["out"].numpy(), 1e-6, f"{tag}: out"),
                     same_bits=True)


@pytest.mark.parametrize("entry", ["forward", "signal", "fused"])
def test_hashgrid_table_must_be_aligned(amd, entry):
    """Two-feature rows are read 8 and 16 bytes at a time: a table that does not start on a 16-byte boundary is
    refused by the host-side check of each entry point that looks features up."""
    n = 300
    case = hash_case("even", 4097)
    desc = hash_desc(amd, case)
    x, t = case["x"][:n].contiguous().cuda(), uniform((n,), 34, 0.0, 1.0).cuda()
    params = [(w.cuda(), b.cuda()) for w, b in omlp.linear_init([10, 64, 64, 1], 5)]
    grads = [(torch.zeros_like(w), torch.zeros_like(b)) for w, b in params]
    ws = torch.empty(amd.lib.load().mri_tiny_mlp_workspace_bytes(10, 64, n) // 4 + 4, device="cuda")
    ready = torch.zeros(8, dtype=torch.int64, device="cuda")

    def call(table, out, loss):
        if entry == "forward":
            amd.call("mri_hashgrid_forward", C.byref(desc), ptr(x), n, ptr(table), ptr(out), 2 * n, 1, n, amd.stream())
        elif entry == "signal":
            amd.call("mri_hashgrid_forward_signal", C.byref(desc), ptr(x), n, ptr(table), ptr(out), n, 128, ptr(ready),
                     amd.stream())
        else:
            (w1, b1), (w2, b2), (w3, b3) = params
            flat = [ptr(g) for pair in grads for g in pair]
            amd.call("mri_hash_tiny_mlp_train", C.byref(desc), ptr(table), ptr(x), ptr(t), n, 64, ptr(w1), ptr(b1),
                     ptr(w2), ptr(b2), ptr(w3), ptr(b3), 1.0, *flat, ptr(out), n, ptr(loss), None, 1, ptr(ws),
                     ws.numel() * 4, amd.stream())

    for off in OFFSETS:
        table, _ = place(case["table"].reshape(-1), off)
        out, check_out = place(torch.full((10, n), float("nan")), 0)
        loss, check_loss = place(torch.full((1,), float("nan")), 0)
        sentinel_out, sentinel_loss = cpu(out), cpu(loss)
        refused(lambda: call(table, out, loss), "table must be 16-byte aligned",
                [("out guards", check_out), ("loss guards", check_loss)])
        torch.cuda.synchronize()
        assert torch.equal(cpu(out).view(torch.int32), sentinel_out.view(torch.int32)), "the refused call wrote `out`"
        assert torch.equal(cpu(loss).view(torch.int32), sentinel_loss.view(torch.int32))
        assert int(ready.sum()) == 0
    table, _ = place(case["table"].reshape(-1), 0)
    out, check_out = place(torch.full((10, n), float("nan")), 0)
    loss = torch.zeros(1, device="cuda")
    call(table, out, loss)
    check_out()
    assert bool(torch.isfinite(out).all())
    if entry != "fused":
        assert_close(cpu(out).T.numpy(), case["out"][:n].numpy(), 1e-6, "the aligned call")


@pytest.mark.parametrize("method,records", [(0, 0), (0, 1), (1, 0), (2, 0), (2, 1)])  # (the atomic kernel has no records)
@pytest.mark.parametrize("n", HASH_N)
def test_hashgrid_backward(amd, option, n, method, records):
    """mri_hashgrid_backward: the dense levels' 16-byte read of a feature-major d_out (hashgrid_bwd.hip,
    dense_absmax_kernel) and the 4-byte reads of every other path; both record formats."""
    option("bwd_records", records)
    case = hash_case("even", n)
    desc = hash_desc(amd, case)
    rows = sum(case["sizes"])
    ws_bytes = amd.ops.backward_workspace_bytes(desc, n)
    ws = torch.empty(ws_bytes // 8 + 2, dtype=torch.int64, device="cuda")
    spans = np.cumsum([0] + list(case["sizes"]))

    def judge(name, got, tag):  # per level, REL_TOL of the float64 sum (test_record_formats_per_slot_against_float64)
        for l in range(5):
            assert_close(got[spans[l]:spans[l + 1]].numpy(), case["grad"][l].numpy(), REL_TOL,
                         f"method {method} records {records} {tag}: level {l}")

    ws_used = [ws]
    for feature_major in (False, True):
        def run(p):
            x = p.inp("x", case["x"].reshape(-1))
            d = p.inp("d_out", case["d_out"].T.contiguous() if feature_major else case["d_out"])
            g = p.out("d_table", (rows * 2,), 0.0)
            ld = d.stride(0)
            sl, sr, sf = (2 * ld, 1, ld) if feature_major else (2, ld, 1)
            amd.call("mri_hashgrid_backward", C.byref(desc), ptr(x), ptr(d), n, sl, sr, sf, ptr(g), method,
                     ptr(ws_used[0]) if method != 1 else None, ws_bytes if method != 1 else 0, amd.stream())
            return dict(d_table=g.reshape(rows, 2))
        # methods 0 / 2: int64 sums of fixed-point products, bitwise reproducible (README) -> same bits; method 1:
        # float atomics in no fixed order -> 1e-6
        over_layouts(dict(x=None, d_out=n if feature_major else 10, d_table=None), run, judge,
                     same_bits=method != 1)
    if method != 1:  # the binned path's workspace is 16-byte aligned by contract
        ws_used[0] = ws.view(torch.float32)[1:]
        pl = Placer({}, "workspace + 4 bytes")
        refused(lambda: run(pl), "workspace must be 16-byte aligned")
        for name, check, _ in pl.checks:
            check(unchanged=True, what=f"workspace refused: {name}")
        ws_used[0] = ws
        pl = Placer({}, "aligned call after the refusal")
        judge("d_table", cpu(run(pl)["d_table"]), pl.tag)


@pytest.mark.parametrize("slice_rows", [128, 130, 257])
@pytest.mark.parametrize("n", [1000, 1001, 1002, 1003])
def test_hashgrid_forward_signal(amd, slice_rows, n):
    """The producer alone (no consumer, nothing waits): its feature-major block against mri_hashgrid_forward on the
    same rows, bit for bit, for slices that do not start on a quad of columns (slice_rows % 4 != 0) as well."""
    case = hash_case("odd", 4097)
    desc = hash_desc(amd, case)
    table, xs = case["table"].cuda(), case["x"][:n].contiguous().cuda()
    plain = torch.empty(10, n, device="cuda")
    amd.call("mri_hashgrid_forward", C.byref(desc), ptr(xs), n, ptr(table), ptr(plain), 2 * n, 1, n, amd.stream())
    plain = cpu(plain)
    slices = -(-n // slice_rows)
    per_slice = amd.ops.hashgrid_signal_blocks(desc, slice_rows)
    assert per_slice > 0

    def run(p):
        x, out = p.inp("x", xs.reshape(-1)), p.out("out", (10, n))
        ready = torch.zeros(slices, dtype=torch.int64, device="cuda")
        amd.call("mri_hashgrid_forward_signal", C.byref(desc), ptr(x), n, ptr(table), ptr(out), out.stride(0),
                 slice_rows, ptr(ready), amd.stream())
        torch.cuda.synchronize()
        assert ready.tolist() == [per_slice] * slices, "every block reports its slice once"
        return dict(out=out)

    def judge(name, got, tag):
        assert torch.equal(got, plain), f"slice_rows {slice_rows} {tag}: differs from mri_hashgrid_forward"
        assert_close(got.T.numpy(), case["out"][:n].numpy(), 1e-6, f"{tag}: oracle")
    over_layouts(dict(x=None, out=n), run, judge, same_bits=True)  # same lookups, only the store width differs


# ================================================================================================ loss, optimiser
@pytest.mark.parametrize("count", [1024, 1025, 1026, 1027])
def test_mse_loss(amd, count):
    pred, target = uniform((count,), 41), uniform((count,), 42, 0.0, 1.0)
    diff = pred.double() - target.double()
    want = dict(loss=(diff ** 2).mean().reshape(1), d_pred=2 * diff / (count * 2.0))

    def run(p):
        a, b = p.inp("pred", pred), p.inp("target", target)
        loss, d = p.out("loss", (1,), 0.0), p.out("d_pred", (count,))
        amd.call("mri_mse_loss", ptr(a), ptr(b), count, 2.0, ptr(loss), ptr(d), amd.stream())
        return dict(loss=loss, d_pred=d)

    def judge(name, got, tag):
        assert_close(got.numpy(), want[name].numpy(), REL_TOL, f"{tag}: {name}")
    # d_pred: same bits (elementwise); the loss meets in one float atomic per workgroup, in no fixed order: 1e-6
    over_layouts(dict(pred=None, target=None, d_pred=None, loss=None), run, judge, same_bits={"d_pred"})


@pytest.mark.parametrize("count", [1027, 1028, 1029, 1030])
def test_adam_step(amd, count):
    """The four buffers share their offset inside a 16-byte line (head elements one by one, then 16-byte pieces, then
    a 4-byte tail); four different offsets are refused."""
    p0, g0 = uniform((count,), 51), uniform((count,), 52, -1e-2, 1e-2)
    m0, v0 = uniform((count,), 53, -1e-3, 1e-3), uniform((count,), 54, 0.0, 1e-4)
    lr, b1, b2, eps, step, scale = 1e-3, 0.9, 0.999, 1e-8, 3, 0.5
    g = g0.double() * scale
    m = m0.double() + (g - m0.double()) * (1 - b1)
    v = v0.double() * b2 + (1 - b2) * g * g
    want = dict(m=m, v=v, p=p0.double() - (lr / (1 - b1 ** step)) * m / (v.sqrt() / np.sqrt(1 - b2 ** step) + eps))
    aligned = None
    for off in (0,) + OFFSETS:
        pl = Placer({k: (off, None) for k in "pgmv"}, f"offset {off}")
        p, m_, v_ = pl.out("p", (count,)), pl.out("m", (count,)), pl.out("v", (count,))
        p.copy_(p0), m_.copy_(m0), v_.copy_(v0)
        g_ = pl.inp("g", g0)
        amd.call("mri_adam_step", ptr(p), ptr(g_), ptr(m_), ptr(v_), count, lr, b1, b2, eps, step, scale, amd.stream())
        pl.verify()
        got = dict(p=cpu(p), m=cpu(m_), v=cpu(v_))
        for k in got:
            assert_close(got[k].numpy(), want[k].numpy(), REL_TOL, f"offset {off}: {k}")
        aligned = aligned or got
        for k in got:  # same operations per element in the head, the 16-byte body and the tail
            assert torch.equal(got[k], aligned[k]), f"offset {off}: {k} differs from the aligned step"
    for which in range(4):  # one buffer elsewhere in its line: refused before the launch, whichever it is
        for off in OFFSETS:
            bufs = [place(t, off if i == which else 0) for i, t in enumerate((p0, g0, m0, v0))]
            args = [ptr(view) for view, _ in bufs]
            refused(lambda: amd.call("mri_adam_step", *args, count, lr, b1, b2, eps, step, scale, amd.stream()),
                    "Adam buffers must share")
            for name, (_, check) in zip(("param", "grad", "exp_avg", "exp_avg_sq"), bufs):
                check(unchanged=True, what=f"{name} after the refusal (buffer {which} + {off})")
    bufs = [place(t, 0) for t in (p0, g0, m0, v0)]  # the aligned call after the refusals
    amd.call("mri_adam_step", *[ptr(view) for view, _ in bufs], count, lr, b1, b2, eps, step, scale, amd.stream())
    for (view, check), key in zip(bufs, ("p", None, "m", "v")):
        check(unchanged=key is None)
        if key:
            assert torch.equal(cpu(view), aligned[key]), f"{key}: the aligned step after the refusals"


# ================================================================================================ PSF, frequency, batches
@pytest.mark.parametrize("S", [5, 27])
def test_psf(amd, S):
    n, D = 33, 3
    x, off, w = uniform((n, D), 61, 0.0, 1.0), uniform((S, D), 62, -0.01, 0.01), uniform((S,), 63, 0.0, 0.1)
    z, t, gsrc = uniform((n * S,), 64), uniform((n,), 65, 0.0, 1.0), uniform((n,), 66)
    zbar = (z.double().reshape(n, S) * w.double()).sum(1)
    gs = 2.0 / (n * 1.0)
    want = dict(x_psf=(x[:, None, :] + off[None, :, :]).reshape(n * S * D).double(), zbar=zbar,
                reduced=(x.double()[:, None, :] + off.double()[None]).sum(1).reshape(-1),
                bcast=(0.5 * w.double()[None, :] * gsrc.double()[:, None]).reshape(-1),
                loss=((zbar - t.double()) ** 2).mean().reshape(1),
                dz=(w.double()[None, :] * ((zbar.float().double() - t.double()) * gs)[:, None]).reshape(-1))

    def run(p):
        xs, offs, ws = p.inp("x", x.reshape(-1)), p.inp("offsets", off.reshape(-1)), p.inp("w", w)
        zs, ts, gv = p.inp("z", z), p.inp("target", t), p.inp("g", gsrc)
        x_psf, red, bc = p.out("x_psf", (n * S * D,)), p.out("reduced", (n * D,)), p.out("bcast", (n * S,))
        zb, loss, dz = p.out("zbar", (n,)), p.out("loss", (1,), 0.0), p.out("dz", (n * S,))
        st = amd.stream()
        amd.call("mri_psf_expand", ptr(xs), n, D, ptr(offs), S, ptr(x_psf), st)
        amd.call("mri_psf_reduce", ptr(x_psf), n, S, D, None, ptr(red), st)
        amd.call("mri_psf_broadcast", ptr(gv), n, S, ptr(ws), 0.5, ptr(bc), st)
        amd.call("mri_psf_mse_loss", ptr(zs), ptr(ts), n, n, S, ptr(ws), 1.0, ptr(zb), ptr(loss), ptr(dz), st)
        return dict(x_psf=x_psf, reduced=red, bcast=bc, zbar=zb, loss=loss, dz=dz)

    def judge(name, got, tag):
        if name == "x_psf":  # one f32 add per element: bit-exact (include/mri_inr.h)
            assert torch.equal(got, want[name].float()), f"{tag}: x_psf"
        else:
            assert_close(got.numpy(), want[name].numpy(), REL_TOL, f"S {S} {tag}: {name}")
    # same bits: sums in a fixed lane order in float64, independent of the grid (README); the expansion only
    # changes its store width
    over_layouts(dict(x=None, offsets=None, w=None, z=None, target=None, g=None, x_psf=None, reduced=None, bcast=None,
                      zbar=None, dz=None), run, judge, same_bits=True)


@pytest.mark.parametrize("n", [130, 131])
def test_frequency(amd, n):
    dim, L = 3, 4
    x, g = uniform((n, dim), 71), uniform((n, dim * 2 * L), 72)
    x64 = x.double().clone().requires_grad_(True)
    out = ohash.frequency_encode(x64, L)
    out.backward(g.double())
    want = dict(out=out.detach(), dx=x64.grad)

    def run(p):
        xs, gs = p.inp("x", x), p.inp("d_out", g)
        o, dx = p.out("out", (n, dim * 2 * L)), p.out("dx", (n, dim))
        amd.call("mri_frequency_forward", ptr(xs), xs.stride(0), n, dim, L, ptr(o), o.stride(0), amd.stream())
        amd.call("mri_frequency_backward", ptr(xs), xs.stride(0), ptr(gs), gs.stride(0), n, dim, L, ptr(dx),
                 dx.stride(0), amd.stream())
        return dict(out=o, dx=dx)

    def judge(name, got, tag):  # test_frequency_encoding_golden: 1e-6 on the encoding, REL_TOL on its gradient
        assert_close(got.numpy(), want[name].numpy(), 1e-6 if name == "out" else REL_TOL, f"{tag}: {name}")
    over_layouts(dict(x=dim, d_out=dim * 2 * L, out=dim * 2 * L, dx=dim), run, judge,
                 same_bits=True)  # 4-byte accesses only, the same expression per element


def test_gather_batch(amd):
    shape, n = (5, 6, 7), 301
    axes = [torch.linspace(0, 1, s) for s in shape]
    volume = uniform((int(np.prod(shape)),), 81, 0.0, 1.0)
    idx = torch.from_numpy(np.random.default_rng(3).integers(0, volume.numel(), n))
    pos = np.stack(np.unravel_index(idx.numpy(), shape), 1)
    want = dict(coords=torch.stack([axes[d][pos[:, d]] for d in range(3)], 1).reshape(-1), target=volume[idx])
    shape_c, off_c = (C.c_int64 * 3)(*shape), (C.c_int64 * 3)(0, 5, 11)
    idx_d = idx.cuda()

    def run(p):
        ax, vol = p.inp("axes", torch.cat(axes)), p.inp("volume", volume)
        co, ta = p.out("coords", (n * 3,)), p.out("target", (n,))
        amd.call("mri_gather_batch", ptr(idx_d), n, 3, shape_c, ptr(ax), off_c, ptr(vol), ptr(co), ptr(ta),
                 amd.stream())
        return dict(coords=co, target=ta)
    over_layouts(dict(axes=None, volume=None, coords=None, target=None), run,
                 lambda name, got, tag: torch.equal(got, want[name]) or pytest.fail(f"{tag}: {name}"),
                 same_bits=True)  # copies


# ================================================================================================ fused decoders
@functools.lru_cache(maxsize=None)
def tiny_case(hidden, n, k_in=32):
    params = omlp.linear_init([k_in, hidden, hidden, 1], 7 + k_in)
    x, t = uniform((n, k_in), 91), uniform((n, 1), 92, 0.0, 1.0)
    out = {}
    for dtype in (torch.float32, torch.float64):
        ps = [(w.to(dtype).clone().requires_grad_(True), b.to(dtype).clone().requires_grad_(True)) for w, b in params]
        xr = x.to(dtype).clone().requires_grad_(True)
        y = omlp.relu_mlp_forward(xr, ps, final_activation=False)
        loss = omlp.mse_loss(y, t.to(dtype))
        loss.backward()
        res = dict(y=y.detach().reshape(-1), loss=loss.detach().reshape(1), d_x=xr.grad.T)
        for i, (w, b) in enumerate(ps):
            res[f"d_w{i + 1}"], res[f"d_b{i + 1}"] = w.grad.reshape(-1), b.grad
        out[dtype] = res
    return dict(params=params, x=x, t=t), out[torch.float32], out[torch.float64]


@pytest.mark.parametrize("n", [300, 301, 302, 303])
@pytest.mark.parametrize("x3", [1, 0])
@pytest.mark.parametrize("hidden", [64, 128])
def test_tiny_mlp(amd, option, hidden, x3, n):
    """mri_tiny_mlp_train_slice / mri_tiny_mlp_forward with x and d_x at shifted bases and padded leading dimensions,
    on the bf16-pipe kernel ("mlp_x3" 1) and the f32-MFMA kernels (0: `fast_io` and the per-tile alignment tests
    of mlp_fused.hip); every parameter and gradient pointer at any offset -- except w2 of the 128-wide f32-MFMA
    kernel, which must be 16-byte aligned."""
    option("mlp_x3", x3)
    case, f32, f64 = tiny_case(hidden, n)
    k = 32
    w2_free = not (hidden == 128 and x3 == 0)
    ws_bytes = amd.lib.load().mri_tiny_mlp_workspace_bytes(k, hidden, n)
    ws = torch.empty(ws_bytes // 4 + 4, device="cuda")

    def run(p):
        x, t = p.inp("x", case["x"].T.contiguous()), p.inp("target", case["t"].reshape(-1))
        names = ("w1", "b1", "w2", "b2", "w3", "b3")
        par = [p.inp(nm, v.reshape(-1)) for nm, v in zip(names, [q for wb in case["params"] for q in wb])]
        grd = [p.out("d_" + nm, (v.numel(),)) for nm, v in zip(names, [q for wb in case["params"] for q in wb])]
        ld = x.stride(0)  # the slice entry point: ONE leading dimension for x and d_x
        d_x = p.out("d_x", (k, n), ld=ld)
        y, y_inf, loss = p.out("y", (n,)), p.out("y_inf", (n,)), p.out("loss", (1,))
        amd.call("mri_tiny_mlp_train_slice", ptr(x), ld, ptr(t), n, n, k, hidden, *[ptr(q) for q in par], 1.0,
                 *[ptr(q) for q in grd], ptr(d_x), ptr(loss), ptr(y), 1, ptr(ws), ws_bytes, amd.stream())
        out = dict(y=y, loss=loss, d_x=d_x, **{"d_" + nm: q for nm, q in zip(names, grd)})
        if ld == n:  # the inference entry point takes a packed block
            amd.call("mri_tiny_mlp_forward", ptr(x), n, k, hidden, *[ptr(q) for q in par], ptr(y_inf), amd.stream())
            out["y_inf"] = y_inf
        return out

    def judge(name, got, tag):  # test_tiny_mlp_fused_kernel: REL_TOL of the oracle (here evaluated in float64)
        key = "y" if name == "y_inf" else name
        assert_close(got.numpy(), f64[key].numpy(), REL_TOL, f"{hidden} x3={x3} {tag}: {name}")

    widths = dict(x=n, d_x=None, target=None, y=None, w1=None, b1=None, b2=None, w3=None, d_w1=None, d_w2=None, d_b3=None)
    if w2_free:
        widths["w2"] = None
    # same bits: per-workgroup partial sums added in a fixed order, bitwise reproducible (mri_inr.h)
    over_layouts(widths, run, judge, same_bits=True)
    if not w2_free:
        for off in OFFSETS:
            pl = Placer({"w2": (off, None)}, f"w2 + {off}")
            outs = {}

            def run_refused():
                outs.update(run(pl))
            refused(run_refused, "w2 must be 16-byte aligned")
            for name, check, is_input in pl.checks:
                check(unchanged=True, what=f"w2 + {off} refused: {name}")  # outputs still hold their NaN fill
        pl = Placer({}, "aligned call after the refusals")
        for name, value in run(pl).items():
            judge(name, cpu(value), pl.tag)


def test_tiny_mlp_slice_at_an_odd_column(amd, option):
    """mri_tiny_mlp_train_slice on columns [37, 37 + 263) of a (32, 303) block: 37 is no multiple of 4, so every
    feature row of the slice starts off a 16-byte boundary although the block itself is aligned."""
    n_total, col, n, k, hidden = 303, 37, 263, 32, 128
    case, _, _ = tiny_case(hidden, n_total)
    names = ("w1", "b1", "w2", "b2", "w3", "b3")
    flat = [q for wb in case["params"] for q in wb]
    ps = [(w.double().clone().requires_grad_(True), b.double().clone().requires_grad_(True)) for w, b in case["params"]]
    xr = case["x"][col:col + n].double().clone().requires_grad_(True)
    loss = ((omlp.relu_mlp_forward(xr, ps, final_activation=False) - case["t"][col:col + n].double()) ** 2).sum() / n_total
    loss.backward()
    for x3 in (1, 0):
        option("mlp_x3", x3)
        ws_bytes = amd.lib.load().mri_tiny_mlp_workspace_bytes(k, hidden, n)
        ws = torch.empty(ws_bytes // 4 + 4, device="cuda")
        pl = Placer({}, f"x3 = {x3}")
        x, t = pl.inp("x", case["x"].T.contiguous()), pl.inp("target", case["t"].reshape(-1))
        par = [pl.inp(nm, v.reshape(-1)) for nm, v in zip(names, flat)]
        grd = [pl.out("d_" + nm, (v.numel(),)) for nm, v in zip(names, flat)]
        d_x, lo = pl.out("d_x", (k, n_total), 0.0), pl.out("loss", (1,))
        at = lambda tensor: C.c_void_p(tensor.data_ptr() + 4 * col)  # noqa: E731
        amd.call("mri_tiny_mlp_train_slice", at(x), n_total, at(t), n, n_total, k, hidden, *[ptr(q) for q in par], 1.0,
                 *[ptr(q) for q in grd], at(d_x), ptr(lo), None, 1, ptr(ws), ws_bytes, amd.stream())
        pl.verify()
        d = cpu(d_x)
        assert float(d[:, :col].abs().max()) == 0.0 and float(d[:, col + n:].abs().max()) == 0.0, "columns outside the slice"
        assert_close(d[:, col:col + n].numpy(), xr.grad.T.numpy(), REL_TOL, f"x3 = {x3}: d_x of the slice")
        assert abs(float(lo) - float(loss)) <= REL_TOL * float(loss)
        for (w, b), gw, gb in zip(ps, grd[0::2], grd[1::2]):
            assert_close(cpu(gw).numpy(), w.grad.reshape(-1).numpy(), REL_TOL, f"x3 = {x3}: dW")
            assert_close(cpu(gb).numpy(), b.grad.numpy(), REL_TOL, f"x3 = {x3}: db")
        # the same columns as a packed, 16-byte aligned block of their own: the same tiles, the same sums, the same bits
        pa = Placer({}, f"x3 = {x3}, packed")
        xa, ta = pa.inp("x", case["x"][col:col + n].T.contiguous()), pa.inp("target", case["t"][col:col + n].reshape(-1))
        para = [pa.inp(nm, v.reshape(-1)) for nm, v in zip(names, flat)]
        grda = [pa.out("d_" + nm, (v.numel(),)) for nm, v in zip(names, flat)]
        d_xa, loa = pa.out("d_x", (k, n)), pa.out("loss", (1,))
        amd.call("mri_tiny_mlp_train_slice", ptr(xa), n, ptr(ta), n, n_total, k, hidden, *[ptr(q) for q in para], 1.0,
                 *[ptr(q) for q in grda], ptr(d_xa), ptr(loa), None, 1, ptr(ws), ws_bytes, amd.stream())
        pa.verify()
        assert torch.equal(cpu(d_xa), d[:, col:col + n]), f"x3 = {x3}: d_x differs from the aligned block's"
        assert torch.equal(cpu(loa), cpu(lo)), f"x3 = {x3}: loss differs from the aligned block's"
        for nm, ga, gs in zip(names, grda, grd):
            assert torch.equal(cpu(ga), cpu(gs)), f"x3 = {x3}: d_{nm} differs from the aligned block's"


@pytest.mark.parametrize("n", [300, 301, 302, 303])
def test_shallow_mlp(amd, n):
    """mlp_shallow.hip has no alignment predicate: every caller buffer is accessed 4 bytes at a time."""
    k, h = 32, 64
    g = torch.Generator().manual_seed(9000 + n)
    x, t = torch.rand(n, k, generator=g) * 2 - 1, torch.rand(n, 1, generator=g)
    w1, b1 = (torch.rand(h, k, generator=g) * 2 - 1) / k ** 0.5, (torch.rand(h, generator=g) * 2 - 1) / k ** 0.5
    w2, b2 = (torch.rand(1, h, generator=g) * 2 - 1) / h ** 0.5, (torch.rand(1, generator=g) * 2 - 1) / h ** 0.5
    refs = {}
    for dtype in (torch.float32, torch.float64):
        xs, a1, c1, a2, c2 = (v.to(dtype).clone().requires_grad_(True) for v in (x, w1, b1, w2, b2))
        y = F.gelu(F.gelu(xs @ a1.T + c1) @ a2.T + c2)
        loss = ((y - t.to(dtype)) ** 2).sum() / n
        loss.backward()
        refs[dtype] = dict(y=y.detach().reshape(-1), loss=loss.detach().reshape(1), d_x=xs.grad.T, d_w1=a1.grad.reshape(-1),
                           d_b1=c1.grad, d_w2=a2.grad.reshape(-1), d_b2=c2.grad)
    ws_bytes = amd.lib.load().mri_shallow_mlp_workspace_bytes(k, h, n)
    ws = torch.empty(ws_bytes // 4 + 4, device="cuda")

    def run(p):
        xs, ts = p.inp("x", x.T.contiguous().reshape(-1)), p.inp("target", t.reshape(-1))
        par = [p.inp(nm, v.reshape(-1)) for nm, v in (("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2))]
        grd = [p.out("d_" + nm, (v.numel(),)) for nm, v in (("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2))]
        d_x, y, y_inf, loss = p.out("d_x", (k * n,)), p.out("y", (n,)), p.out("y_inf", (n,)), p.out("loss", (1,))
        amd.call("mri_shallow_mlp_train", ptr(xs), ptr(ts), n, n, k, h, *[ptr(q) for q in par], 3, 3, 1.0,
                 *[ptr(q) for q in grd], ptr(d_x), ptr(loss), ptr(y), 1, ptr(ws), ws_bytes, amd.stream())
        amd.call("mri_shallow_mlp_forward", ptr(xs), n, k, h, *[ptr(q) for q in par], 3, 3, ptr(y_inf), amd.stream())
        return dict(y=y, y_inf=y_inf, loss=loss, d_x=d_x.reshape(k, n), d_w1=grd[0], d_b1=grd[1], d_w2=grd[2], d_b2=grd[3])

    def judge(name, got, tag):  # test_gpu_shallow._check
        key = "y" if name == "y_inf" else name
        assert_no_worse(got.numpy(), refs[torch.float32][key].numpy(), refs[torch.float64][key].numpy(), f"{tag}: {name}")
        if key in ("y", "d_x"):
            assert_close(got.numpy(), refs[torch.float64][key].numpy(), REL_TOL, f"{tag}: {name}")
    # same bits: partial sums added in a fixed order, bitwise reproducible (mri_inr.h)
    over_layouts(dict(x=None, target=None, w1=None, b1=None, w2=None, b2=None, d_x=None, y=None, d_w1=None, d_b2=None),
                 run, judge, same_bits=True)


# ================================================================================================ SIREN chains
def arr(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() if t is not None else None for t in tensors])


@functools.lru_cache(maxsize=None)
def siren_case(hidden, n, dim_in=3, L=3):
    params = omlp.siren_init(dim_in, hidden, 1, L, 17)
    x, t = uniform((n, dim_in), 101), uniform((n, 1), 102, 0.0, 1.0)
    out = {}
    for dtype in (torch.float32, torch.float64):
        ps = [(w.to(dtype).clone().requires_grad_(True), b.to(dtype).clone().requires_grad_(True)) for w, b in params]
        y = omlp.siren_forward(x.to(dtype), ps)
        loss = omlp.mse_loss(y, t.to(dtype))
        loss.backward()
        res = dict(y=y.detach().reshape(-1), loss=loss.detach().reshape(1))
        for i, (w, b) in enumerate(ps):
            res[f"d_w{i}"], res[f"d_b{i}"] = w.grad.reshape(-1), b.grad
        out[dtype] = res
    return dict(params=params, x=x, t=t), out[torch.float32], out[torch.float64]


@pytest.mark.parametrize("hidden,n", [(64, 300), (64, 303), (256, 130), (256, 131)])
def test_siren_chain(amd, hidden, n):
    """mri_siren_forward / _forward_loss / _backward, one width per kernel family (64: LDS-image kernels, 256: rows
    kernels).  x, y, target, dy, the biases and every gradient output -- of the first layer, a hidden layer and the
    head, which different code serves -- are accessed 4 bytes at a time: any offset.  weight / act / deriv / dz /
    dz_last / workspace are 16-byte aligned by contract: each entry point, called on its own, refuses them otherwise
    before its first launch."""
    case, f32, f64 = siren_case(hidden, n)
    L, dim_in = 3, 3
    ws_bytes = amd.lib.load().mri_siren_backward_workspace_bytes(n, hidden, L)
    ws = torch.empty(ws_bytes // 4 + 4, device="cuda")

    def setup(p, shift=None):
        """Every buffer of the three calls and the calls themselves; `shift` = (name, layer) moves ONE of the 16-byte
        arguments one float off its boundary."""
        def buf(name, layer, values, is_input=False):
            v, check = place(values, 1 if shift == (name, layer) else 0)
            p.checks.append((f"{name}[{layer}]", check, is_input))
            return v
        nan = torch.full((n * hidden,), float("nan"))
        x, t = p.inp("x", case["x"].reshape(-1)), p.inp("target", case["t"].reshape(-1))
        w = [buf("weight", l, wl.reshape(-1), True) for l, (wl, _) in enumerate(case["params"])]
        b = [p.inp(f"bias{l}", bl) for l, (_, bl) in enumerate(case["params"])]
        act, der = [buf("act", l, nan) for l in range(L)], [buf("deriv", l, nan) for l in range(L)]
        dz = [None] + [buf("dz", l, nan) for l in range(1, L)]
        d_w = [p.out(f"d_weight{l}", (wl.numel(),), 0.0) for l, (wl, _) in enumerate(case["params"])]
        d_b = [p.out(f"d_bias{l}", (bl.numel(),), 0.0) for l, (_, bl) in enumerate(case["params"])]
        g_w = [p.out(f"g_weight{l}", (wl.numel(),), 0.0) for l, (wl, _) in enumerate(case["params"])]
        g_b = [p.out(f"g_bias{l}", (bl.numel(),), 0.0) for l, (_, bl) in enumerate(case["params"])]
        y, y2, dy = p.out("y", (n,)), p.out("y2", (n,)), p.out("dy", (n,))
        loss, loss2 = p.out("loss", (1,), 0.0), p.out("loss2", (1,), 0.0)
        wsp = ws[1:] if shift == ("workspace", 0) else ws
        st = amd.stream()
        calls = dict(
            forward=lambda: amd.call("mri_siren_forward", ptr(x), n, dim_in, hidden, L, arr(w), arr(b), 30.0, 30.0,
                                     arr(act), arr(der), ptr(y), ptr(wsp), ws_bytes, st),
            loss=lambda: amd.call("mri_mse_loss", ptr(y), ptr(t), n, 1.0, ptr(loss), ptr(dy), st),
            backward=lambda: amd.call("mri_siren_backward", ptr(x), ptr(dy), n, dim_in, hidden, L, arr(w), arr(act),
                                      arr(der), arr(dz), arr(d_w), arr(d_b), 0, ptr(wsp), ws_bytes, st),
            # the fused pair: forward with the loss and the head's backward, then the rest
            forward_loss=lambda: amd.call("mri_siren_forward_loss", ptr(x), ptr(t), n, n, dim_in, hidden, L, arr(w), arr(b),
                                          30.0, 30.0, 1.0, arr(act[:-1] + [None]), arr(der[:-1] + [None]), ptr(dz[L - 1]),
                                          ptr(y2), ptr(g_w[L]), ptr(g_b[L]), ptr(g_b[L - 1]), ptr(loss2), ptr(wsp),
                                          ws_bytes, st),
            backward_rest=lambda: amd.call("mri_siren_backward", ptr(x), None, n, dim_in, hidden, L, arr(w),
                                           arr(act[:-1] + [None]), arr(der[:-1] + [None]), arr(dz), arr(g_w), arr(g_b), 1,
                                           ptr(wsp), ws_bytes, st))
        out = dict(y=y, loss=loss, y2=y2, loss2=loss2)
        for l in range(L + 1):
            out[f"d_w{l}"], out[f"d_b{l}"], out[f"g_w{l}"], out[f"g_b{l}"] = d_w[l], d_b[l], g_w[l], g_b[l]
        return calls, out

    def run(p):
        calls, out = setup(p)
        for name in ("forward", "loss", "backward", "forward_loss", "backward_rest"):
            calls[name]()
        return out

    def judge(name, got, tag):  # test_siren_golden: REL_TOL of the reference (here evaluated in float64)
        key = {"y2": "y", "loss2": "loss"}.get(name, name.replace("g_", "d_"))
        assert_close(got.numpy(), f64[key].numpy(), REL_TOL, f"{hidden} {tag}: {name}")
    # same bits: fixed-order partial sums, bitwise reproducible (mri_inr.h); these arguments only move 4-byte accesses
    widths = dict(x=None, target=None, y=None, y2=None, dy=None)
    for l in (0, 1, L):  # first layer, a hidden layer, the head
        widths.update({f"bias{l}": None, f"d_weight{l}": None, f"d_bias{l}": None})
    widths.update({f"g_weight{L}": None, f"g_bias{L}": None, f"g_bias{L - 1}": None})  # forward_loss's own outputs
    over_layouts(widths, run, judge, same_bits=True)
    # each entry point on its own with ONE argument shifted: refused by its own host-side check (nothing it needs from an
    # earlier call is read before that), every buffer as placed, and the aligned sequence passes afterwards
    cases = [(entry, (name, 1)) for entry in ("forward", "forward_loss", "backward") for name in ("weight", "act", "deriv")]
    cases += [("forward_loss", ("dz", L - 1)), ("backward", ("dz", 1))]  # (dz[L - 1] is forward_loss's dz_last)
    cases += [(entry, ("workspace", 0)) for entry in ("forward", "forward_loss", "backward")]
    for entry, shift in cases:
        pl = Placer({}, f"{entry}: {shift[0]}[{shift[1]}] + 1")
        calls, _ = setup(pl, shift)
        word = "dz_last" if (entry, shift[0]) == ("forward_loss", "dz") else shift[0]
        refused(calls[entry], "16-byte aligned workspace" if word == "workspace" else f"{word}.*16-byte aligned")
        for what, check, _ in pl.checks:
            check(unchanged=True, what=f"{pl.tag} refused: {what}")
    pl = Placer({}, "aligned calls after the refusals")
    for name, value in run(pl).items():
        judge(name, cpu(value), pl.tag)
    pl.verify()


@functools.lru_cache(maxsize=None)
def modsiren_case(n, hidden=64, dim_in=3, L=3):
    siren = omlp.siren_init(dim_in, hidden, 1, L, 23)
    mod = omlp.modulator_init(dim_in, hidden, L, 523)
    x, t = uniform((n, dim_in), 111), uniform((n, 1), 112, 0.0, 1.0)
    out = {}
    for dtype in (torch.float32, torch.float64):
        sp = [(w.to(dtype).clone().requires_grad_(True), b.to(dtype).clone().requires_grad_(True)) for w, b in siren]
        mp = [(w.to(dtype).clone().requires_grad_(True), b.to(dtype).clone().requires_grad_(True)) for w, b in mod]
        y = omlp.modulated_siren_forward(x.to(dtype), sp, mp)
        loss = omlp.mse_loss(y, t.to(dtype))
        loss.backward()
        res = dict(y=y.detach().reshape(-1), loss=loss.detach().reshape(1))
        for i, (w, b) in enumerate(sp):
            res[f"s_w{i}"], res[f"s_b{i}"] = w.grad.reshape(-1), b.grad
        for i, (w, b) in enumerate(mp):
            res[f"m_w{i}"], res[f"m_b{i}"] = w.grad.reshape(-1), b.grad
        out[dtype] = res
    return dict(siren=siren, mod=mod, x=x, t=t), out[torch.float32], out[torch.float64]


@pytest.mark.parametrize("n", [300, 303])
def test_modsiren_chain(amd, n):
    """mri_modsiren_forward / _forward_loss / _backward at width 64.  The (n, hidden) buffers act / hid / dcos / sn / dzs /
    dzm and the workspace are 16-byte aligned by contract: each of the three calls, on its own, refuses them otherwise.
    Everything else at any offset, for the first layer, a hidden layer and the head -- the weights too: the operand
    split reads them float by float."""
    case, f32, f64 = modsiren_case(n)
    hidden, L, dim_in = 64, 3, 3
    ws_bytes = amd.lib.load().mri_modsiren_backward_workspace_bytes(n, hidden, L)
    ws = torch.empty(ws_bytes // 4 + 4, device="cuda")
    kinds = ("act", "hid", "dcos", "sn")

    def setup(p, shift=None):
        def buf(name, layer):
            v, check = place(torch.full((n * hidden,), float("nan")), 1 if shift == (name, layer) else 0)
            p.checks.append((f"{name}[{layer}]", check, False))
            return v
        x, t = p.inp("x", case["x"].reshape(-1)), p.inp("target", case["t"].reshape(-1))
        sw = [p.inp(f"siren_weight{l}", w.reshape(-1)) for l, (w, _) in enumerate(case["siren"])]
        sb = [p.inp(f"siren_bias{l}", b) for l, (_, b) in enumerate(case["siren"])]
        mw = [p.inp(f"mod_weight{l}", w.reshape(-1)) for l, (w, _) in enumerate(case["mod"])]
        mb = [p.inp(f"mod_bias{l}", b) for l, (_, b) in enumerate(case["mod"])]
        saved = {k: [buf(k, l) for l in range(L)] for k in kinds}
        saved2 = {k: [buf(k + "'", l) for l in range(L)] for k in kinds} if shift is None else saved
        dzs, dzm = [None] + [buf("dzs", l) for l in range(1, L)], [None] + [buf("dzm", l) for l in range(1, L)]
        g_sw = [p.out(f"d_siren_weight{l}", (w.numel(),), 0.0) for l, (w, _) in enumerate(case["siren"])]
        g_sb = [p.out(f"d_siren_bias{l}", (b.numel(),), 0.0) for l, (_, b) in enumerate(case["siren"])]
        g_mw = [p.out(f"d_mod_weight{l}", (w.numel(),), 0.0) for l, (w, _) in enumerate(case["mod"])]
        g_mb = [p.out(f"d_mod_bias{l}", (b.numel(),), 0.0) for l, (_, b) in enumerate(case["mod"])]
        y, y_inf, y_tr, dy, loss = (p.out("y", (n,)), p.out("y_inf", (n,)), p.out("y_tr", (n,)), p.out("dy", (n,)),
                                    p.out("loss", (1,), 0.0))
        wsp = ws[1:] if shift == ("workspace", 0) else ws
        st = amd.stream()
        params = (arr(sw), arr(sb), arr(mw), arr(mb))
        calls = dict(
            forward_loss=lambda: amd.call("mri_modsiren_forward_loss", ptr(x), ptr(t), n, n, dim_in, hidden, L, *params,
                                          30.0, 30.0, 1.0, *[arr(saved[k]) for k in kinds], ptr(y), ptr(dy), ptr(loss),
                                          ptr(wsp), ws_bytes, st),
            backward=lambda: amd.call("mri_modsiren_backward", ptr(x), ptr(dy), n, dim_in, hidden, L, arr(sw), arr(mw),
                                      *[arr(saved[k]) for k in kinds], arr(dzs), arr(dzm), arr(g_sw), arr(g_sb), arr(g_mw),
                                      arr(g_mb), ptr(wsp), ws_bytes, st),
            inference=lambda: amd.call("mri_modsiren_forward", ptr(x), n, dim_in, hidden, L, *params, 30.0, 30.0, None,
                                       None, None, None, ptr(y_inf), ptr(wsp), ws_bytes, st),
            forward=lambda: amd.call("mri_modsiren_forward", ptr(x), n, dim_in, hidden, L, *params, 30.0, 30.0,
                                     *[arr(saved2[k]) for k in kinds], ptr(y_tr), ptr(wsp), ws_bytes, st))
        out = dict(y=y, y_inf=y_inf, y_tr=y_tr, loss=loss)
        for l in range(L + 1):
            out[f"s_w{l}"], out[f"s_b{l}"] = g_sw[l], g_sb[l]
        for l in range(L):
            out[f"m_w{l}"], out[f"m_b{l}"] = g_mw[l], g_mb[l]
        return calls, out

    def run(p):
        calls, out = setup(p)
        for name in ("forward_loss", "backward", "inference", "forward"):
            calls[name]()
        return out

    def judge(name, got, tag):  # test_modulated_siren_golden: REL_TOL of the reference (here evaluated in float64)
        assert_close(got.numpy(), f64["y" if name in ("y_inf", "y_tr") else name].numpy(), REL_TOL, f"{tag}: {name}")
    widths = dict(x=None, target=None, y=None, dy=None)
    for l in (0, 1, L):  # first layer, a hidden layer, the head (the modulator has no head)
        widths.update({f"siren_weight{l}": None, f"siren_bias{l}": None, f"d_siren_weight{l}": None,
                       f"d_siren_bias{l}": None})
    for l in (0, 1):
        widths.update({f"mod_weight{l}": None, f"mod_bias{l}": None, f"d_mod_weight{l}": None, f"d_mod_bias{l}": None})
    # same bits: no float atomics, partial sums in a fixed order (mri_inr.h)
    over_layouts(widths, run, judge, same_bits=True)
    cases = [(entry, (name, 1)) for entry in ("forward", "forward_loss", "backward") for name in kinds]
    cases += [("backward", ("dzs", 1)), ("backward", ("dzm", 1))]
    cases += [(entry, ("workspace", 0)) for entry in ("forward", "forward_loss", "backward")]
    for entry, shift in cases:
        pl = Placer({}, f"{entry}: {shift[0]}[{shift[1]}] + 1")
        calls, _ = setup(pl, shift)
        refused(calls[entry], "16-byte aligned workspace" if shift[0] == "workspace" else f"{shift[0]}.*16-byte aligned")
        for what, check, _ in pl.checks:
            check(unchanged=True, what=f"{pl.tag} refused: {what}")
    pl = Placer({}, "aligned calls after the refusals")
    for name, value in run(pl).items():
        judge(name, cpu(value), pl.tag)
    pl.verify()


# ================================================================================================ one-call training step
def test_fused_step_plain_adam_branch(amd):
    """mri_fused_step with param / grad / exp_avg / exp_avg_sq one float off a 16-byte boundary: its `fold` test is
    false, so the table gradient's conversion launch and mri_adam_step (head elements, then 16-byte pieces) run
    instead of the folded Adam kernel.  Same bits as the folded step on the same values; the gradients it leaves in
    `grad` against float64.  (The table itself stays on a 16-byte boundary inside the shifted range: the lookup
    reads its rows 8 bytes at a time.)"""
    n, hidden, k = 4097, 64, 10
    case = hash_case("even", n)
    desc = hash_desc(amd, case)
    dec = omlp.linear_init([k, hidden, hidden, 1], 11)
    target = uniform((n,), 121, 0.0, 1.0)
    pieces = [case["table"].reshape(-1)] + [q.reshape(-1) for wb in dec for q in wb]
    lr, b1, b2, eps = 1e-2, 0.9, 0.999, 1e-8
    h = amd.lib.load()
    tiny_bytes, bwd_bytes = h.mri_tiny_mlp_workspace_bytes(k, hidden, n), amd.ops.backward_workspace_bytes(desc, n)
    tiny_ws = torch.empty(tiny_bytes // 4 + 4, device="cuda")
    bwd_ws = torch.empty(bwd_bytes // 8 + 2, dtype=torch.int64, device="cuda")
    side, ev_fork, ev_join = torch.cuda.Stream(), torch.cuda.Event(), torch.cuda.Event()
    ev_fork.record(), ev_join.record()
    torch.cuda.synchronize()

    last = {}

    def run(off, table_shift=0):
        pad = 4 - off + table_shift  # floats of the range in front of the table
        flat = torch.cat([torch.zeros(pad)] + pieces)
        total = flat.numel()
        pl = Placer({name: (off, None) for name in ("param", "grad", "exp_avg", "exp_avg_sq")}, f"range + {off}")
        param, grad = pl.out("param", (total,)), pl.out("grad", (total,), 0.0)
        m, v = pl.out("exp_avg", (total,), 0.0), pl.out("exp_avg_sq", (total,), 0.0)
        param.copy_(flat)
        last.update(pl=pl, param=param, flat=flat)
        coords, tgt = pl.inp("coords", case["x"].reshape(-1)), pl.inp("target", target)
        enc, d_enc, loss = pl.out("enc", (k, n)), pl.out("d_enc", (k, n)), pl.out("loss", (1,))
        starts = np.cumsum([pad] + [q.numel() for q in pieces])
        at = lambda t, i: t.data_ptr() + 4 * int(starts[i])  # noqa: E731
        a = amd.lib.FusedStepArgs()
        a.grid, a.table, a.d_table = C.pointer(desc), at(param, 0), at(grad, 0)
        a.w1, a.b1, a.w2, a.b2, a.w3, a.b3 = (at(param, i) for i in range(1, 7))
        a.d_w1, a.d_b1, a.d_w2, a.d_b2, a.d_w3, a.d_b3 = (at(grad, i) for i in range(1, 7))
        assert a.table % 16 == 4 * table_shift and param.data_ptr() % 16 == 4 * off
        a.loss, a.hidden, a.bwd_method, a.counted, a.join_pending = loss.data_ptr(), hidden, 0, 0, 0
        a.coords, a.target, a.n, a.enc, a.d_enc = coords.data_ptr(), tgt.data_ptr(), n, enc.data_ptr(), d_enc.data_ptr()
        a.tiny_ws, a.tiny_ws_bytes, a.bwd_ws, a.bwd_ws_bytes = tiny_ws.data_ptr(), tiny_bytes, bwd_ws.data_ptr(), bwd_bytes
        a.param, a.grad, a.exp_avg, a.exp_avg_sq = param.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr()
        a.n_params, a.lr, a.beta1, a.beta2, a.eps, a.step, a.grad_scale = total, lr, b1, b2, eps, 1, 1.0
        a.dim, a.grad_divisor = 3, 1.0
        a.stream = torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())
        a.stream_side, a.ev_fork, a.ev_join = side.cuda_stream, ev_fork.cuda_event, ev_join.cuda_event
        amd.call("mri_fused_step", C.byref(a))
        torch.cuda.synchronize()
        pl.verify()
        return {name: cpu(t)[pad:] for name, t in (("param", param), ("grad", grad), ("exp_avg", m), ("exp_avg_sq", v))} | \
            dict(loss=cpu(loss), enc=cpu(enc), d_enc=cpu(d_enc))

    # a table off its 16-byte boundary is refused at the top of the call, before the side stream's first launch
    for table_shift in OFFSETS:
        refused(lambda: run(0, table_shift), "table must be 16-byte aligned")
        torch.cuda.synchronize()
        for name, check, is_input in last["pl"].checks:
            check(unchanged=name != "param", what=f"table + {table_shift} refused: {name}")
        assert torch.equal(cpu(last["param"]), last["flat"]), "the refused step moved a parameter"
    folded, plain = run(0), run(1)
    for name in ("param", "exp_avg", "exp_avg_sq", "loss", "enc", "d_enc"):  # same operations, same order (mri_inr.h)
        assert torch.equal(plain[name], folded[name]), f"{name}: the plain Adam branch differs from the folded step"
    # float64 on the same float32 inputs
    tabs = [t.double().requires_grad_(True) for t in torch.split(case["table"], list(case["sizes"]))]
    ps = [(w.double().clone().requires_grad_(True), b.double().clone().requires_grad_(True)) for w, b in dec]
    y = omlp.relu_mlp_forward(ohash.encode(case["x"], tabs, case["res"]), ps, final_activation=False)
    loss = omlp.mse_loss(y.reshape(-1), target.double())
    loss.backward()
    assert abs(float(plain["loss"]) - float(loss)) <= REL_TOL * float(loss)
    want = [t.grad.reshape(-1) for t in tabs] + [q.grad.reshape(-1) for wb in ps for q in wb]
    got = torch.split(plain["grad"], [w.numel() for w in want])
    for i, (g, w) in enumerate(zip(got, want)):
        assert_close(g.numpy(), w.numpy(), REL_TOL, f"gradient tensor {i} after the plain step")
    assert not torch.equal(plain["param"], torch.cat(pieces)), "Adam moved nothing"
