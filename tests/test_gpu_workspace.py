"""Every kernel workspace of include/mri_inr.h held to its contract: the size function's answer is enough, the buffer
needs no initialisation, and it may be shared by calls of other shapes on the same stream.

The entry points are called through the C ABI, so that the test owns the buffer: tests/layout.py place_workspace puts a
workspace of EXACTLY the reported size between two guards of sentinels and fills it with a chosen 32-bit pattern.  Each
(entry point, shape) case makes these runs on identical inputs:
  a. baseline: zero-filled, exactly sized.  The outputs are held to the entry point's own float64 reference at the
     criterion its current tests use (REL_TOL of float64; the shallow decoder and BatchNorm on two rows:
     yardstick.assert_no_worse; the modulated chain: test_gpu_modsiren.py's close_or_no_worse on rows clear of a
     ReLU kink);
  b. stale: directly before, the same buffer served the same entry point at a LARGER, differently shaped problem (the
     buffer is sized for the larger of the two, the small call is told its own byte count).  Where every other shape
     of the family needs less (both clamped), the partner is the differently shaped call and the buffer the larger;
  c. filled with 0x5A5A5A5A (a large finite float, a large counter), then with 0xFFFFFFFF (a NaN, -1);
  d. short: workspace_bytes - 1 is refused with MRI_ERR_INVALID_ARGUMENT, the outputs (pre-filled with the sentinel)
     and the guards untouched.
Every output of b and c is bit for bit that of a (the kernels here are documented bitwise reproducible: no tolerance),
and the guards are intact after every run.  b runs before c and 0x5A before 0xFF: the mildest dirt first, so that the
first failure of a buggy kernel is a comparison.  Nothing documented as unordered takes part: no hash-grid level on
global float atomics, no mri_linear_backward_weight, no mri_mse_loss.  (n, hidden) scratch that a call documents as
scratch (dz, dzs / dzm, dz_last, enc / d_enc) is NaN-filled in every run.

Row counts come from the clamps in csrc/: one n below one tile, one ragged n below the clamp, one n just past
clamp x tile rows, where the slab count is the clamped one.

Inventory: every entry point that takes a workspace | its size function | cases
  mri_hashgrid_backward          | mri_hashgrid_backward_workspace_bytes | test_table_gradient: methods 0, 2
  mri_hashgrid_backward_levels   | same | two level groups on one prepared workspace
  mri_hashgrid_backward_prepare  | same | + MRI_BWD_PREPARED, with and without MRI_BWD_OVERWRITE; the short run
  mri_hashgrid_backward_scaled   | same | level maxima given (F = 2)
  mri_hashgrid_backward_adam     | same | against mri_hashgrid_backward + mri_adam_step, bit for bit
                                   grids D 3 / L 16 / F 2 / 2^15 (every level dense under the defaults), D 4 / F 2,
                                   D 2 / F 4, D 3 / F 1 and D 3 / F 2 / 2^17 (dense and binned levels together); n 1, 63,
                                   2049, 4097, 70001 under the defaults; every knob at both values once
                                   (test_table_gradient_knobs), size taken AFTER the knobs
  (prepare with the exact size, backward with a larger count: test_prepare_and_backward_with_different_byte_counts)
  mri_tiny_mlp_train, _overwrite, _slice (two slices), _dx_absmax | mri_tiny_mlp_workspace_bytes | test_decoder:
                                   (k_in, hidden) (32, 128) (32, 64) (7, 128) (40, 64), "mlp_x3" 0 / 1 / 2 with the
                                   size taken BEFORE the knob, n 17, 2501, 16385 (128-wide) / 32769 (64-wide)
  mri_hash_tiny_mlp_train        | mri_tiny_mlp_workspace_bytes(2 L, hidden, n) | test_decoder, k_in 32
  mri_tiny_mlp_train_overlapped  | left out: the call waits on a producer (as in test_gpu_layout.py); it shares
                                   tiny_mlp_train_impl's size check and slab layout with the three calls above
  mri_shallow_mlp_train          | mri_shallow_mlp_workspace_bytes | test_shallow: hidden 32 / 64 / 128, k_in 5 / 32,
                                   both `overwrite` values
  mri_siren_forward              | mri_siren_forward_workspace_bytes | test_siren: training and inference form
  mri_siren_forward_loss + mri_siren_backward(head_done = 1) | mri_siren_backward_workspace_bytes | the pair, dirtied
                                   before the first call only
  mri_siren_backward(head_done = 0) | mri_siren_backward_workspace_bytes | test_siren
  mri_siren_gradient             | mri_siren_gradient_workspace_bytes | dim_in 3 and 4
                                   hidden 32 / 64 / 128, 256 with "siren_rows" 0 and 1; depths 1, 2, 5
  mri_modsiren_forward (both forms), _forward_loss, _backward | mri_modsiren_forward_ / _backward_workspace_bytes |
                                   test_modsiren: hidden 64 / 128, L 2 / 6, dim_in 1 / 3
  mri_bn_stats, mri_bn_act_backward | mri_bn_workspace_bytes | test_batchnorm: (2, 1) (320, 64) (4099, 130)
                                   (70001, 128), dirtied before each of the two calls
  mri_fused_step                 | tiny_ws, bwd_ws, next_bwd_ws | test_fused_step: two consecutive steps, the
                                   counted-ahead workspace of step 1 is the bwd_ws of step 2
The Python owners of scratch -- ops.backward_workspace, _tiny_workspace, _shallow_workspace, _siren_scratch,
modsiren_workspace, the caches _rff_ws, _rff_train_ws, _gabor_ws and _modsiren_ws (test_ops_*) and trainer.FusedStep,
one case per plan (test_fused_step_owns_clean_scratch) -- are grown by a large call of another shape, filled with 0xFF
bytes and held to the bits of the zero-filled run.  (The pool they all call, ops._grow_scratch: test_scratch_cpu.py.)
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import REL_TOL, assert_close
from layout import SENTINEL, place, place_workspace, ptr
from yardstick import KNOB_DEFAULTS, assert_no_worse
from test_gpu_modsiren import close_or_no_worse
from oracle import detrand
from oracle import hashgrid as ohash
from oracle import mlp as omlp

pytestmark = pytest.mark.gpu

NAN = float("nan")
FILLS = (0x5A5A5A5A, 0xFFFFFFFF)
BWD_PREPARED, BWD_OVERWRITE = 16, 32


@pytest.fixture(scope="module")
def amd():
    from mri_interpolation_amd import _lib, ops
    assert torch.cuda.is_available(), "these tests need the GPU"
    _lib.load()
    knobs = {name: _lib.get_option(name) for name in KNOB_DEFAULTS}
    assert knobs == KNOB_DEFAULTS, "a knob was left off its default before this module"
    yield type("NS", (), dict(lib=_lib, h=_lib.load(), ops=ops, call=staticmethod(_lib.call),
                              stream=staticmethod(ops._stream)))
    assert {name: _lib.get_option(name) for name in KNOB_DEFAULTS} == KNOB_DEFAULTS, "a knob was left off its default"


@pytest.fixture
def option(amd):
    """set(name, value) for the duration of one test; the values read before come back in any case."""
    before = {}

    def set_(name, value):
        before.setdefault(name, amd.lib.get_option(name))
        amd.lib.set_option(name, value)

    yield set_
    for k, v in before.items():
        amd.lib.set_option(k, v)


def uniform(shape, seed, lo=-1.0, hi=1.0):
    return torch.from_numpy(detrand.uniform(int(np.prod(shape)), seed, lo, hi).reshape(shape).copy())


def arr(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() if t is not None else None for t in tensors])


def bits(t):
    return t.contiguous().view(torch.int32)


class Run:
    """The output and scratch buffers of ONE run.  An output is NaN-filled unless the call adds to it; when the call
    is expected to be refused every buffer holds the sentinel instead, and untouched() proves that it still does."""

    def __init__(self, refuse=False):
        self.refuse, self.made, self.checks = refuse, [], []

    def out(self, shape, fill=NAN, dtype=torch.float32):
        t = torch.full(tuple(shape) if not isinstance(shape, int) else (shape,), fill, dtype=dtype, device="cuda")
        if self.refuse:
            t.view(torch.int32).fill_(SENTINEL)
        self.made.append(t)
        return t

    def scratch(self, shape):
        """(n, hidden) scratch a call documents as private: NaN in every run."""
        return self.out(shape)

    def guarded(self, count, fill):
        """A small output between guard bands of its own (tests/layout.py place): verify() sees a store past it."""
        t, check = place(torch.full((count,), fill), 0)
        if self.refuse:
            t.view(torch.int32).fill_(SENTINEL)
        self.made.append(t)
        self.checks.append(check)
        return t

    def verify(self, what):
        for check in self.checks:
            check(what=what)

    def untouched(self, what):
        torch.cuda.synchronize()
        for i, t in enumerate(self.made):
            assert bool((t.view(torch.int32) == SENTINEL).all()), f"{what}: the refused call wrote output {i}"


def hold(tag, launch, need, judge, stale=None):
    """Runs a - d of one (entry point, shape): launch(run, workspace, bytes) -> {name: device tensor}."""
    assert need >= 0, f"{tag}: the size function refused the shape ({need})"

    def one(ws, check, what):
        run = Run()
        got = launch(run, ws, need)
        check(f"{tag}, {what}")
        run.verify(f"{tag}, {what}")
        return got

    ws, check = place_workspace(need, 0)
    base = one(ws, check, "zero-filled workspace")
    judge({k: v.detach().cpu() for k, v in base.items()})
    runs = []
    if stale is not None and need > 0:
        launch_big, need_big = stale
        assert need_big > 0
        ws, check = place_workspace(max(need, need_big), 0)
        launch_big(Run(), ws, need_big)
        check(f"{tag}, the larger call before the stale run")
        runs.append(("after a differently shaped call on the same buffer", one(ws, check, "stale workspace")))
    for fill in FILLS if need > 0 else ():
        ws, check = place_workspace(need, fill)
        runs.append((f"workspace filled with {fill:#010x}", one(ws, check, f"workspace filled with {fill:#010x}")))
    for what, got in runs:
        for name, value in got.items():
            assert torch.equal(bits(value), bits(base[name])), f"{tag}, {what}: {name} differs from the zero-filled run"
    if need > 0:
        ws, check = place_workspace(need, 0)
        run = Run(refuse=True)
        with pytest.raises(RuntimeError, match=r"failed \(-1\)"):  # MRI_ERR_INVALID_ARGUMENT
            launch(run, ws, need - 1)
        run.untouched(f"{tag}, workspace one byte short")
        run.verify(f"{tag}, workspace one byte short")
        check(f"{tag}, workspace one byte short")


def hold_all(tag, small, judge, big=None):
    for entry, (launch, need) in small.items():
        hold(f"{tag} {entry}", launch, need, judge, big[entry] if big is not None else None)


def judge_close(want, tag, tol=REL_TOL):
    def judge(got):
        for name, value in got.items():
            if name in want:
                assert_close(value.double().numpy().reshape(-1), want[name].double().numpy().reshape(-1), tol,
                             f"{tag}: {name}")
    return judge


# ================================================================================================ the helper
def test_place_workspace_sees_an_overrun():
    for n_bytes in (0, 4, 1000, 4 << 20):
        ws, check = place_workspace(n_bytes, 0x5A5A5A5A)
        assert ws.numel() * 4 == (n_bytes + 15) // 16 * 16 and (n_bytes == 0 or ws.data_ptr() % 16 == 0)
        assert n_bytes == 0 or bool((ws == 0x5A5A5A5A).all())
        ws.fill_(7)  # the workspace itself may change
        check("inside")
    ws, check = place_workspace(1000, 0, guard_bytes=64)
    behind = ws.as_strided((1,), (1,), ws.storage_offset() + ws.numel() + 3)
    behind.fill_(0)
    with pytest.raises(AssertionError, match=r"the first 20 bytes past its end"):  # 1008 + 12 - 1000
        check("one word behind")
    behind.fill_(SENTINEL)
    ws.as_strided((1,), (1,), ws.storage_offset() - 1).fill_(0)
    with pytest.raises(AssertionError, match=r"4 bytes before its start"):
        check("one word in front")
    ws, check = place_workspace(8 << 20, 0)  # each guard: at least a quarter of the workspace
    assert ws.storage_offset() * 4 >= 2 << 20


# ================================================================================================ SIREN chains
# Tile rows 256 / 256 / 128 / 64 (hidden 32 / 64 / 128 / 256), rows kernels 128, weight-gradient kernel 32; every
# kernel's grid is clamped at 256 workgroups: 65537, 32769, 16385 and 8193 rows are the first past a clamp.
@functools.lru_cache(maxsize=None)
def siren_inputs(hidden, L, n, dim_in):
    params = omlp.siren_init(dim_in, hidden, 1, L, 17 + hidden + L)
    return params, uniform((n, dim_in), 101 + dim_in), uniform((n,), 102, 0.0, 1.0)


@functools.lru_cache(maxsize=None)
def siren_refs(hidden, L, n, dim_in):
    params, x, t = siren_inputs(hidden, L, n, dim_in)
    ps = [(w.double().clone().requires_grad_(True), b.double().clone().requires_grad_(True)) for w, b in params]
    xg = x.double().clone().requires_grad_(True)
    y = omlp.siren_forward(xg, ps).reshape(-1)
    dydx, = torch.autograd.grad(y.sum(), xg, retain_graph=True)
    loss = omlp.mse_loss(y, t.double())
    loss.backward()
    want = dict(y=y.detach(), loss=loss.detach().reshape(1), dydx=dydx)
    for l, (w, b) in enumerate(ps):
        want[f"d_w{l}"], want[f"d_b{l}"] = w.grad, b.grad
    return want


def siren_entries(amd, hidden, L, n, dim_in):
    params, x, t = siren_inputs(hidden, L, n, dim_in)
    w, b = [p[0].cuda() for p in params], [p[1].cuda() for p in params]
    xd, td, st = x.cuda(), t.cuda(), amd.stream()
    fwd_bytes = amd.h.mri_siren_forward_workspace_bytes(hidden, L)
    bwd_bytes = amd.h.mri_siren_backward_workspace_bytes(n, hidden, L)
    grad_bytes = amd.h.mri_siren_gradient_workspace_bytes(hidden, L)

    def grads(run):
        return [run.out(v.shape, 0.0) for v in w], [run.out(v.shape, 0.0) for v in b]

    def named(d_w, d_b, **more):
        out = dict(more)
        for l in range(L + 1):
            out[f"d_w{l}"], out[f"d_b{l}"] = d_w[l], d_b[l]
        return out

    def forward(run, ws, nb):
        act, der = [run.out((n, hidden)) for _ in range(L)], [run.out((n, hidden)) for _ in range(L)]
        y = run.out((n,))
        amd.call("mri_siren_forward", ptr(xd), n, dim_in, hidden, L, arr(w), arr(b), 30.0, 30.0, arr(act), arr(der),
                 ptr(y), ptr(ws), nb, st)
        return dict(y=y, act_first=act[0], act_last=act[-1], deriv_last=der[-1])

    def inference(run, ws, nb):
        y = run.out((n,))
        amd.call("mri_siren_forward", ptr(xd), n, dim_in, hidden, L, arr(w), arr(b), 30.0, 30.0, None, None, ptr(y),
                 ptr(ws), nb, st)
        return dict(y=y)

    def pair(run, ws, nb):  # the workspace is private to the pair: dirty before the first call only
        act = [run.out((n, hidden)) for _ in range(L - 1)] + [None]
        der = [run.out((n, hidden)) for _ in range(L - 1)] + [None]
        dz = [None] + [run.scratch((n, hidden)) for _ in range(1, L)]
        (d_w, d_b), y, loss = grads(run), run.out((n,)), run.out((1,), 0.0)
        amd.call("mri_siren_forward_loss", ptr(xd), ptr(td), n, n, dim_in, hidden, L, arr(w), arr(b), 30.0, 30.0, 1.0,
                 arr(act), arr(der), ptr(dz[L - 1]), ptr(y), ptr(d_w[L]), ptr(d_b[L]), ptr(d_b[L - 1]), ptr(loss),
                 ptr(ws), nb, st)
        amd.call("mri_siren_backward", ptr(xd), None, n, dim_in, hidden, L, arr(w), arr(act), arr(der), arr(dz),
                 arr(d_w), arr(d_b), 1, ptr(ws), nb, st)
        return named(d_w, d_b, y=y, loss=loss)

    def backward(run, ws, nb):  # act / deriv from a forward call on a workspace of its own; dy by torch, elementwise
        own = torch.zeros(max(fwd_bytes, 16) // 4, dtype=torch.int32, device="cuda")
        act = [torch.full((n, hidden), NAN, device="cuda") for _ in range(L)]
        der = [torch.full((n, hidden), NAN, device="cuda") for _ in range(L)]
        y = torch.full((n,), NAN, device="cuda")
        amd.call("mri_siren_forward", ptr(xd), n, dim_in, hidden, L, arr(w), arr(b), 30.0, 30.0, arr(act), arr(der),
                 ptr(y), ptr(own) if fwd_bytes else None, fwd_bytes, st)
        dy = (y - td) * (2.0 / n)
        dz = [None] + [run.scratch((n, hidden)) for _ in range(1, L)]
        d_w, d_b = grads(run)
        amd.call("mri_siren_backward", ptr(xd), ptr(dy), n, dim_in, hidden, L, arr(w), arr(act), arr(der), arr(dz),
                 arr(d_w), arr(d_b), 0, ptr(ws), nb, st)
        return named(d_w, d_b)

    def gradient(run, ws, nb):
        y, g = run.out((n,)), run.out((n, dim_in))
        amd.call("mri_siren_gradient", ptr(xd), n, dim_in, hidden, L, arr(w), arr(b), 30.0, 30.0, ptr(y), ptr(g),
                 ptr(ws), nb, st)
        return dict(y=y, dydx=g)

    entries = dict(forward=(forward, fwd_bytes), inference=(inference, fwd_bytes), backward=(backward, bwd_bytes))
    if L >= 2:
        entries["forward_loss + backward(head_done)"] = (pair, bwd_bytes)
    if dim_in <= 4:
        entries["gradient"] = (gradient, grad_bytes)
    return entries


# (hidden, sine layers, n, dim_in, "siren_rows")
SIREN = [(32, 1, 100, 3, 1), (32, 2, 3001, 4, 1), (32, 5, 65537, 3, 1),
         (64, 1, 65537, 4, 1), (64, 2, 100, 3, 1), (64, 5, 3001, 3, 1),
         (128, 1, 3001, 3, 1), (128, 2, 32769, 3, 1), (128, 5, 60, 4, 1),
         (256, 1, 3001, 3, 1), (256, 2, 16385, 3, 1), (256, 2, 32769, 4, 1), (256, 5, 33, 3, 1),
         (256, 2, 16385, 3, 0), (256, 5, 3001, 4, 0), (256, 1, 33, 3, 0)]
OTHER_WIDTH = {32: 64, 64: 128, 128: 64, 256: 128}


@pytest.mark.parametrize("hidden,L,n,dim_in,rows", SIREN)
def test_siren(amd, option, hidden, L, n, dim_in, rows):
    option("siren_rows", rows)
    small = siren_entries(amd, hidden, L, n, dim_in)
    # the larger call: another n, another width where that needs more, else another depth of this width
    h = amd.h
    need = h.mri_siren_backward_workspace_bytes(n, hidden, L)
    partner = (OTHER_WIDTH[hidden], 2 if L == 3 else 3, 70001, 7 - dim_in)
    if h.mri_siren_backward_workspace_bytes(partner[2], partner[0], partner[1]) <= need:
        partner = (hidden, 6, 70001 if hidden < 256 else 20001, 7 - dim_in)
    assert h.mri_siren_backward_workspace_bytes(partner[2], partner[0], partner[1]) > need
    big = siren_entries(amd, *partner)
    want = siren_refs(hidden, L, n, dim_in)
    tag = f"SIREN {dim_in} -> {hidden} x {L}, n = {n}, rows kernels {rows}:"
    for entry, (launch, nbytes) in small.items():
        hold(f"{tag} {entry}", launch, nbytes, judge_close(want, f"{tag} {entry}"), big.get(entry))


# ================================================================================================ modulated SIREN
# Tile rows 128 / 64 (hidden 64 / 128), grids clamped at 256 workgroups.
@functools.lru_cache(maxsize=None)
def modsiren_inputs(hidden, L, n, dim_in):
    """Rows that stay clear of every ReLU kink of the modulator (test_gpu_modsiren.py selected_rows: a pre-activation
    within 1e-6 of zero, or of another sign in float32 than in float64, is no statement about the kernel)."""
    siren, mod = omlp.siren_init(dim_in, hidden, 1, L, 23 + hidden + L), omlp.modulator_init(dim_in, hidden, L, 523 + hidden)
    drawn = n + n // 8 + 64
    x = uniform((drawn, dim_in), 111 + dim_in)
    keep = torch.ones(drawn, dtype=torch.bool)
    signs = []
    for dtype in (torch.float64, torch.float32):
        z = x.to(dtype)
        h, sign = z, []
        for w, b in mod:
            pm = F.linear(h, w.to(dtype), b.to(dtype))
            keep &= (pm.abs() >= 1e-6).all(dim=1)
            sign.append(pm > 0)
            h = torch.cat((torch.relu(pm), z), dim=1)
        signs.append(sign)
    for s64, s32 in zip(*signs):
        keep &= (s64 == s32).all(dim=1)
    assert int(keep.sum()) >= n, "too many rows at a ReLU kink"
    return siren, mod, x[keep][:n].contiguous(), uniform((n,), 112, 0.0, 1.0)


@functools.lru_cache(maxsize=None)
def modsiren_refs(hidden, L, n, dim_in):
    siren, mod, x, t = modsiren_inputs(hidden, L, n, dim_in)
    refs = []
    for dtype in (torch.float32, torch.float64):
        sp = [(w.to(dtype).clone().requires_grad_(True), b.to(dtype).clone().requires_grad_(True)) for w, b in siren]
        mp = [(w.to(dtype).clone().requires_grad_(True), b.to(dtype).clone().requires_grad_(True)) for w, b in mod]
        y = omlp.modulated_siren_forward(x.to(dtype), sp, mp).reshape(-1)
        loss = omlp.mse_loss(y, t.to(dtype))
        loss.backward()
        want = dict(y=y.detach(), loss=loss.detach().reshape(1), dy=2.0 * (y.detach() - t.to(dtype)) / n)
        for l, (w, b) in enumerate(sp):
            want[f"s_w{l}"], want[f"s_b{l}"] = w.grad, b.grad
        for l, (w, b) in enumerate(mp):
            want[f"m_w{l}"], want[f"m_b{l}"] = w.grad, b.grad
        refs.append(want)
    return tuple(refs)


def judge_modsiren(refs, tag):
    """test_gpu_modsiren.py section 1: within REL_TOL of float64, or no worse an f32 evaluation than the CPU's."""
    f32, f64 = refs

    def judge(got):
        for name, value in got.items():
            if name in f64:
                close_or_no_worse(value.numpy().reshape(-1), f32[name].numpy().reshape(-1), f64[name].numpy().reshape(-1),
                                  f"{tag}: {name}")
    return judge


def modsiren_entries(amd, hidden, L, n, dim_in):
    siren, mod, x, t = modsiren_inputs(hidden, L, n, dim_in)
    sw, sb = [p[0].cuda() for p in siren], [p[1].cuda() for p in siren]
    mw, mb = [p[0].cuda() for p in mod], [p[1].cuda() for p in mod]
    xd, td, st = x.cuda(), t.cuda(), amd.stream()
    fwd_bytes = amd.h.mri_modsiren_forward_workspace_bytes(hidden, L)
    bwd_bytes = amd.h.mri_modsiren_backward_workspace_bytes(n, hidden, L)
    params = lambda: (arr(sw), arr(sb), arr(mw), arr(mb))  # noqa: E731

    def saved(make):
        return [[make((n, hidden)) for _ in range(L)] for _ in range(4)]

    def forward(run, ws, nb):
        keep, y = saved(run.out), run.out((n,))
        amd.call("mri_modsiren_forward", ptr(xd), n, dim_in, hidden, L, *params(), 30.0, 30.0, *[arr(k) for k in keep],
                 ptr(y), ptr(ws), nb, st)
        return dict(y=y, act_last=keep[0][-1], hid_last=keep[1][-1], dcos_first=keep[2][0], sn_last=keep[3][-1])

    def inference(run, ws, nb):
        y = run.out((n,))
        amd.call("mri_modsiren_forward", ptr(xd), n, dim_in, hidden, L, *params(), 30.0, 30.0, None, None, None, None,
                 ptr(y), ptr(ws), nb, st)
        return dict(y=y)

    def forward_loss(run, ws, nb, make=None):
        make = make or run.out
        keep, y, dy, loss = saved(make), make((n,)), make((n,)), make((1,), 0.0)
        amd.call("mri_modsiren_forward_loss", ptr(xd), ptr(td), n, n, dim_in, hidden, L, *params(), 30.0, 30.0, 1.0,
                 *[arr(k) for k in keep], ptr(y), ptr(dy), ptr(loss), ptr(ws), nb, st)
        return dict(y=y, dy=dy, loss=loss, act_last=keep[0][-1], keep=keep)

    def forward_loss_entry(run, ws, nb):
        out = forward_loss(run, ws, nb)
        del out["keep"]
        return out

    def backward(run, ws, nb):  # the saved tensors and dy from a forward call on a workspace of its own
        own = torch.zeros(bwd_bytes // 4 + 4, dtype=torch.int32, device="cuda")
        fwd = forward_loss(None, own, bwd_bytes,
                           make=lambda shape, fill=NAN: torch.full(tuple(shape), fill, device="cuda"))
        dzs = [None] + [run.scratch((n, hidden)) for _ in range(1, L)]
        dzm = [None] + [run.scratch((n, hidden)) for _ in range(1, L)]
        g_sw, g_sb = [run.out(v.shape, 0.0) for v in sw], [run.out(v.shape, 0.0) for v in sb]
        g_mw, g_mb = [run.out(v.shape, 0.0) for v in mw], [run.out(v.shape, 0.0) for v in mb]
        amd.call("mri_modsiren_backward", ptr(xd), ptr(fwd["dy"]), n, dim_in, hidden, L, arr(sw), arr(mw),
                 *[arr(k) for k in fwd["keep"]], arr(dzs), arr(dzm), arr(g_sw), arr(g_sb), arr(g_mw), arr(g_mb),
                 ptr(ws), nb, st)
        out = {}
        for l in range(L + 1):
            out[f"s_w{l}"], out[f"s_b{l}"] = g_sw[l], g_sb[l]
        for l in range(L):
            out[f"m_w{l}"], out[f"m_b{l}"] = g_mw[l], g_mb[l]
        return out

    return dict(forward=(forward, fwd_bytes), inference=(inference, fwd_bytes),
                forward_loss=(forward_loss_entry, bwd_bytes), backward=(backward, bwd_bytes))


MODSIREN = [(hidden, L, n, dim_in) for hidden, ns in ((64, (50, 3001, 32769)), (128, (50, 3001, 16385)))
            for L, dim_in in ((2, 1), (6, 3)) for n in ns]


@pytest.mark.parametrize("hidden,L,n,dim_in", MODSIREN)
def test_modsiren(amd, hidden, L, n, dim_in):
    small = modsiren_entries(amd, hidden, L, n, dim_in)
    h = amd.h
    need = h.mri_modsiren_backward_workspace_bytes(n, hidden, L)
    partner = (192 - hidden, 3 if L == 2 else 4, 70001, 4 - dim_in)
    if h.mri_modsiren_backward_workspace_bytes(partner[2], partner[0], partner[1]) <= need:
        partner = (hidden, 7, 70001, 4 - dim_in)
    assert h.mri_modsiren_backward_workspace_bytes(partner[2], partner[0], partner[1]) > need
    big = modsiren_entries(amd, *partner)
    want = modsiren_refs(hidden, L, n, dim_in)
    tag = f"modulated SIREN {dim_in} -> {hidden} x {L}, n = {n}:"
    for entry, (launch, nbytes) in small.items():
        hold(f"{tag} {entry}", launch, nbytes, judge_modsiren(want, f"{tag} {entry}"), big[entry])


# ================================================================================================ decoder
# Tile rows 32 (bf16-pipe kernel), 2 x 32 (128-wide team kernel), 64 (64-wide f32-MFMA kernel); clamps 256 / 256 / 512.
@functools.lru_cache(maxsize=None)
def tiny_inputs(k_in, hidden, n):
    return omlp.linear_init([k_in, hidden, hidden, 1], 7 + k_in + hidden), uniform((n, k_in), 91), uniform((n,), 92, 0.0, 1.0)


def tiny_refs_from(params, feats, t):
    ps = [(w.double().clone().requires_grad_(True), b.double().clone().requires_grad_(True)) for w, b in params]
    xr = feats.double().clone().requires_grad_(True)
    y = omlp.relu_mlp_forward(xr, ps, final_activation=False).reshape(-1)
    loss = omlp.mse_loss(y, t.double())
    loss.backward()
    want = dict(y=y.detach(), loss=loss.detach().reshape(1), d_x=xr.grad.T)
    for i, (w, b) in enumerate(ps):
        want[f"d_w{i + 1}"], want[f"d_b{i + 1}"] = w.grad, b.grad
    return want


@functools.lru_cache(maxsize=None)
def tiny_refs(k_in, hidden, n):
    params, x, t = tiny_inputs(k_in, hidden, n)
    return tiny_refs_from(params, x, t)


@functools.lru_cache(maxsize=None)
def decoder_grid(n):
    """D 3, L 16, F 2, T 2^15: the encoder of the one-kernel lookup + decoder step (k_in = 32)."""
    res, sizes = ohash.resolutions_for(3, 16, 15, 16, 512)
    tables = ohash.init_tables(sizes, 2, 78, 0.5)
    return res, sizes, tables, uniform((n, 3), 93, 0.0, 1.0)


@functools.lru_cache(maxsize=None)
def hash_tiny_refs(hidden, n):
    params, _, t = tiny_inputs(32, hidden, n)
    res, sizes, tables, coords = decoder_grid(n)
    feats = ohash.encode(coords, [tb.double() for tb in tables], res)
    want = tiny_refs_from(params, feats, t)
    want["d_enc"] = want.pop("d_x")
    return want


def decoder_entries(amd, k_in, hidden, n):
    params, x, t = tiny_inputs(k_in, hidden, n)
    flat = [q.cuda() for wb in params for q in wb]  # w1 b1 w2 b2 w3 b3
    xd, td, st = x.T.contiguous().cuda(), t.cuda(), amd.stream()
    need = amd.h.mri_tiny_mlp_workspace_bytes(k_in, hidden, n)
    names = ("d_w1", "d_b1", "d_w2", "d_b2", "d_w3", "d_b3")

    def outs(run, fill):
        grd = [run.out(q.shape, fill) for q in flat]
        return grd, run.out((k_in, n)), run.out((1,), fill), run.out((n,))

    def result(grd, d_x, loss, y, **more):
        return dict(zip(names, grd), d_x=d_x, loss=loss, y=y, **more)

    def train(run, ws, nb):
        grd, d_x, loss, y = outs(run, 0.0)
        amd.call("mri_tiny_mlp_train", ptr(xd), ptr(td), n, k_in, hidden, *[ptr(q) for q in flat], 1.0,
                 *[ptr(g) for g in grd], ptr(d_x), ptr(loss), ptr(y), ptr(ws), nb, st)
        return result(grd, d_x, loss, y)

    def overwrite(run, ws, nb):
        grd, d_x, loss, y = outs(run, NAN)
        amd.call("mri_tiny_mlp_train_overwrite", ptr(xd), ptr(td), n, k_in, hidden, *[ptr(q) for q in flat], 1.0,
                 *[ptr(g) for g in grd], ptr(d_x), ptr(loss), ptr(y), ptr(ws), nb, st)
        return result(grd, d_x, loss, y)

    n1 = n - n // 3  # the larger slice first: it is the one whose size the workspace has

    def slices(run, ws, nb):
        grd, d_x, loss, y = outs(run, NAN)
        at = lambda tensor, col: C.c_void_p(tensor.data_ptr() + 4 * col)  # noqa: E731
        for col, cols, over in ((0, n1, 1), (n1, n - n1, 0)):
            amd.call("mri_tiny_mlp_train_slice", at(xd, col), n, at(td, col), cols, n, k_in, hidden,
                     *[ptr(q) for q in flat], 1.0, *[ptr(g) for g in grd], at(d_x, col), ptr(loss), at(y, col), over,
                     ptr(ws), nb, st)
        return result(grd, d_x, loss, y)

    def dx_absmax(run, ws, nb):
        grd, d_x, loss, y = outs(run, NAN)
        top = run.guarded((k_in + 1) // 2, 0.0)  # an odd k_in: the last row has an entry of its own
        amd.call("mri_tiny_mlp_train_dx_absmax", ptr(xd), ptr(td), n, k_in, hidden, *[ptr(q) for q in flat], 1.0,
                 *[ptr(g) for g in grd], ptr(d_x), ptr(loss), ptr(y), 1, ptr(top), ptr(ws), nb, st)
        return result(grd, d_x, loss, y, dx_pair_absmax=top)

    entries = {"train": (train, need), "train_overwrite": (overwrite, need),
               "train_slice x 2": (slices, amd.h.mri_tiny_mlp_workspace_bytes(k_in, hidden, n1)),
               "train_dx_absmax": (dx_absmax, need)}
    if k_in == 32:
        res, sizes, tables, coords = decoder_grid(n)
        desc = amd.ops.make_grid_desc(3, [[r] * 3 for r in res], sizes, 2)
        table, cd = torch.cat(tables).cuda(), coords.cuda()

        def hash_train(run, ws, nb):
            grd, d_enc, loss, y = outs(run, NAN)
            amd.call("mri_hash_tiny_mlp_train", C.byref(desc), ptr(table), ptr(cd), ptr(td), n, hidden,
                     *[ptr(q) for q in flat], 1.0, *[ptr(g) for g in grd], ptr(d_enc), n, ptr(loss), ptr(y), 1, ptr(ws),
                     nb, st)
            out = result(grd, d_enc, loss, y)
            out["d_enc"] = out.pop("d_x")
            return out
        entries["hash_tiny_mlp_train"] = (hash_train, need, desc)
    return entries


DECODER = [(k_in, hidden, n) for k_in, hidden in ((32, 128), (32, 64), (7, 128), (40, 64))
           for n in (17, 2501, 16385 if hidden == 128 else 32769)]


@pytest.mark.parametrize("x3", [1, 0, 2])
@pytest.mark.parametrize("k_in,hidden,n", DECODER)
def test_decoder(amd, option, k_in, hidden, n, x3):
    small = decoder_entries(amd, k_in, hidden, n)  # sizes BEFORE the knob: sized for whichever kernel runs
    big = decoder_entries(amd, k_in if k_in == 32 else 32 - k_in % 32, 192 - hidden, 70001)
    option("mlp_x3", x3)
    want = tiny_refs(k_in, hidden, n)
    tag = f"decoder {k_in} -> {hidden}, n = {n}, mlp_x3 {x3}:"
    for entry, item in small.items():
        launch, need = item[0], item[1]
        if entry == "train_dx_absmax" and not amd.h.mri_tiny_mlp_dx_absmax_supported(k_in, hidden):
            continue
        if entry == "hash_tiny_mlp_train" and not amd.h.mri_hash_tiny_mlp_supported(C.byref(item[2]), hidden):
            continue
        ref = hash_tiny_refs(hidden, n) if entry == "hash_tiny_mlp_train" else want
        close = judge_close(ref, f"{tag} {entry}")

        def judge(got):
            close(got)
            if "dx_pair_absmax" in got:  # the maxima of the d_x the same call produced, exactly
                rows = torch.cat([got["d_x"], torch.zeros(k_in % 2, n)]).abs()
                pairs = rows.reshape((k_in + 1) // 2, 2 * n).max(1).values
                assert torch.equal(got["dx_pair_absmax"], pairs), f"{tag} {entry}: max |d_x| per feature pair"
        hold(f"{tag} {entry}", launch, need, judge, big[entry][:2] if entry in big else None)


# ================================================================================================ shallow decoder
# Rows per workgroup: block_rows() = 4 waves x 32 rows (hidden 32) or x 16 rows; the grid is clamped at 512.
@functools.lru_cache(maxsize=None)
def shallow_case(k_in, hidden, n):
    g = torch.Generator().manual_seed(9000 + n + hidden + k_in)
    x, t = torch.rand(n, k_in, generator=g) * 2 - 1, torch.rand(n, 1, generator=g)
    w1 = (torch.rand(hidden, k_in, generator=g) * 2 - 1) / k_in ** 0.5
    b1 = (torch.rand(hidden, generator=g) * 2 - 1) / k_in ** 0.5
    w2 = (torch.rand(1, hidden, generator=g) * 2 - 1) / hidden ** 0.5
    b2 = (torch.rand(1, generator=g) * 2 - 1) / hidden ** 0.5
    refs = {}
    for dtype in (torch.float32, torch.float64):
        xs, a1, c1, a2, c2 = (v.to(dtype).clone().requires_grad_(True) for v in (x, w1, b1, w2, b2))
        y = F.gelu(F.gelu(xs @ a1.T + c1) @ a2.T + c2)
        loss = ((y - t.to(dtype)) ** 2).sum() / n
        loss.backward()
        refs[dtype] = dict(y=y.detach().reshape(-1), loss=loss.detach().reshape(1), d_x=xs.grad.T, d_w1=a1.grad,
                           d_b1=c1.grad, d_w2=a2.grad, d_b2=c2.grad)
    return (x, t, w1, b1, w2, b2), refs[torch.float32], refs[torch.float64]


def shallow_entries(amd, k_in, hidden, n):
    (x, t, *par), _, _ = shallow_case(k_in, hidden, n)
    xd, td, par, st = x.T.contiguous().cuda(), t.reshape(-1).cuda(), [p.cuda() for p in par], amd.stream()
    need = amd.h.mri_shallow_mlp_workspace_bytes(k_in, hidden, n)

    def make(over):
        def train(run, ws, nb):
            fill = NAN if over else 0.0
            grd = [run.out(p.shape, fill) for p in par]
            d_x, loss, y = run.out((k_in, n)), run.out((1,), fill), run.out((n,))
            amd.call("mri_shallow_mlp_train", ptr(xd), ptr(td), n, n, k_in, hidden, *[ptr(p) for p in par], 3, 3, 1.0,
                     *[ptr(g) for g in grd], ptr(d_x), ptr(loss), ptr(y), over, ptr(ws), nb, st)
            return dict(zip(("d_w1", "d_b1", "d_w2", "d_b2"), grd), d_x=d_x, loss=loss, y=y)
        return train
    return {"train, overwrite 0": (make(0), need), "train, overwrite 1": (make(1), need)}


SHALLOW = [(k_in, hidden, n) for hidden in (32, 64, 128) for k_in in (5, 32)
           for n in (9, 3001, 65537 if hidden == 32 else 32769)]


@pytest.mark.parametrize("k_in,hidden,n", SHALLOW)
def test_shallow(amd, k_in, hidden, n):
    small = shallow_entries(amd, k_in, hidden, n)
    big = shallow_entries(amd, 37 - k_in, {32: 64, 64: 128, 128: 64}[hidden], 70001)
    _, f32, f64 = shallow_case(k_in, hidden, n)
    tag = f"shallow decoder {k_in} -> {hidden}, n = {n}:"

    def judge(got):  # test_gpu_shallow._check
        for name, value in got.items():
            assert_no_worse(value.numpy().reshape(-1), f32[name].numpy().reshape(-1), f64[name].numpy().reshape(-1),
                            f"{tag} {name}")
            if name in ("y", "d_x"):
                assert_close(value.numpy(), f64[name].numpy(), REL_TOL, f"{tag} {name}")
    hold_all(tag, small, judge, big)


# ================================================================================================ BatchNorm
@functools.lru_cache(maxsize=None)
def bn_case(n, C):
    z, dy = uniform((n, C), 21, -1.4, 2.0), uniform((n, C), 22)
    gamma, beta = uniform((C,), 23, 0.5, 1.5), uniform((C,), 24, -0.2, 0.2)
    rm, rv = uniform((C,), 25, -0.1, 0.1), uniform((C,), 26, 0.5, 1.5)
    refs = {}
    for dtype in (torch.float32, torch.float64):
        zr, gr, br = (v.to(dtype).clone().requires_grad_(True) for v in (z, gamma, beta))
        rmr, rvr = rm.to(dtype).clone(), rv.to(dtype).clone()
        F.gelu(F.batch_norm(zr, rmr, rvr, gr, br, True, 0.1, 1e-5)).backward(dy.to(dtype))
        zd = z.to(dtype)
        save = torch.stack([zd.mean(0), 1 / torch.sqrt(zd.var(0, unbiased=False) + 1e-5)])
        refs[dtype] = dict(running_mean=rmr, running_var=rvr, save=save, dz=zr.grad, d_gamma=gr.grad, d_beta=br.grad)
    return dict(z=z, dy=dy, gamma=gamma, beta=beta, rm=rm, rv=rv), refs[torch.float32], refs[torch.float64]


def bn_entries(amd, n, C):
    case = bn_case(n, C)[0]
    dev = {k: v.cuda() for k, v in case.items()}
    st = amd.stream()
    need = amd.h.mri_bn_workspace_bytes(n, C)

    def stats(run, ws, nb):
        rm, rv, save = run.out((C,)), run.out((C,)), run.out((2, C))
        if not run.refuse:
            rm.copy_(dev["rm"]), rv.copy_(dev["rv"])
        amd.call("mri_bn_stats", ptr(dev["z"]), C, n, C, 0.1, 1e-5, ptr(rm), ptr(rv), None, ptr(save), ptr(ws), nb, st)
        return dict(running_mean=rm, running_var=rv, save=save)

    def backward(run, ws, nb):  # the statistics from mri_bn_stats on a workspace of its own
        own = torch.zeros(need // 4 + 4, dtype=torch.int32, device="cuda")
        save = torch.full((2, C), NAN, device="cuda")
        amd.call("mri_bn_stats", ptr(dev["z"]), C, n, C, 0.1, 1e-5, None, None, None, ptr(save), ptr(own), need, st)
        dz, dg, db = run.out((n, C)), run.out((C,)), run.out((C,))
        amd.call("mri_bn_act_backward", ptr(dev["dy"]), C, ptr(dev["z"]), C, n, C, ptr(save), ptr(dev["gamma"]),
                 ptr(dev["beta"]), 3, ptr(dz), C, ptr(dg), ptr(db), 1, ptr(ws), nb, st)
        return dict(dz=dz, d_gamma=dg, d_beta=db)

    return dict(stats=(stats, need), act_backward=(backward, need))


BN = [(2, 1), (320, 64), (4099, 130), (70001, 128)]


@pytest.mark.parametrize("n,C", BN)
def test_batchnorm(amd, n, C):
    small = bn_entries(amd, n, C)
    big = bn_entries(amd, 90001, 257)
    assert big["stats"][1] > small["stats"][1]
    _, f32, f64 = bn_case(n, C)
    tag = f"BatchNorm ({n}, {C}):"

    def judge(got):  # test_gpu_bn.py: REL_TOL of float64; on two rows eps dominates var and PyTorch's f32 is the yardstick
        for name, value in got.items():
            if n > 3:
                assert_close(value.numpy(), f64[name].numpy(), REL_TOL, f"{tag} {name}")
            elif name != "save":
                assert_no_worse(value.numpy(), f32[name].numpy(), f64[name].numpy(), f"{tag} {name}")
    hold_all(tag, small, judge, big)


# ================================================================================================ table gradient
# make_plan: a level of at most "bwd_dense_max_parts" (4) slices of 16384 / F slots is dense, the others are binned;
# the dense levels are split over coordinate ranges from n = 2 x 2048 on.  No level here takes global float atomics.
GRIDS = {  # dim, levels, features, log2 T, base, finest                         slices per level (dense up to 4)
    "D3 F2": (3, 16, 2, 15, 16, 512),      # every level dense under the defaults     1 .. 4
    "D4 F2": (4, 8, 2, 17, 4, 32),         #                                           1 1 8 16 16 16 16 16
    "D2 F4": (2, 8, 4, 15, 16, 4096),      #                                           1 1 1 1 2 3 6 8
    "D3 F1": (3, 6, 1, 17, 8, 512),        #                                           1 1 2 7 8 8
    "D3 F2 2^17": (3, 8, 2, 17, 16, 256),  # dense and binned levels together          1 1 2 3 5 8 14 16
}
HASH_N = [1, 63, 2049, 4097, 70001]


@functools.lru_cache(maxsize=None)
def grid_case(name, n):
    dim, L, feats, log2_t, base, finest = GRIDS[name]
    res, sizes = ohash.resolutions_for(dim, L, log2_t, base, finest)
    x = uniform((n, dim), 31 + dim, 0.0, 1.0)
    d_out = uniform((n, L * feats), 32) * torch.exp2(uniform((n, 1), 33, -6.0, 2.0))
    grad = [g[0] for g in ohash.table_gradient_f64(x, d_out, sizes, res, feats)]
    return dict(dim=dim, L=L, F=feats, res=res, sizes=sizes, x=x, d_out=d_out, grad=torch.cat(grad))


def grid_desc(amd, case):
    return amd.ops.make_grid_desc(case["dim"], [[r] * case["dim"] for r in case["res"]], case["sizes"], case["F"])


def table_entries(amd, name, n, method):
    """Sizes are taken HERE: set the knobs first."""
    case = grid_case(name, n)
    desc = grid_desc(amd, case)
    L, feats, rows = case["L"], case["F"], sum(case["sizes"])
    xd, st = case["x"].cuda(), amd.stream()
    dd = case["d_out"].T.contiguous().cuda()  # feature-major (L F, n), as the trainer hands it over
    sl, sr, sf = feats * n, 1, n
    need = amd.h.mri_hashgrid_backward_workspace_bytes(C.byref(desc), n)
    low, high = (1 << (L // 2)) - 1, ((1 << L) - 1) & ~((1 << (L // 2)) - 1)
    absmax = dd.abs().reshape(L, feats * n).max(1).values.contiguous()
    g0, seed = uniform((rows, feats), 35, -1e-3, 1e-3).cuda(), uniform((rows, feats), 36).cuda()
    lr, b1, b2, eps, step = 1e-2, 0.9, 0.999, 1e-8, 2

    def plain(flags, base):
        def launch(run, ws, nb):
            g = run.out((rows, feats), NAN if flags & BWD_OVERWRITE else 0.0)
            if base is not None and not run.refuse:
                g.copy_(base)
            amd.call("mri_hashgrid_backward", C.byref(desc), ptr(xd), ptr(dd), n, sl, sr, sf, ptr(g), method | flags,
                     ptr(ws), nb, st)
            return dict(d_table=g)
        return launch

    def prepared(flags):
        def launch(run, ws, nb):
            g = run.out((rows, feats), NAN if flags & BWD_OVERWRITE else 0.0)
            amd.call("mri_hashgrid_backward_prepare", C.byref(desc), ptr(xd), n, method, ptr(ws), nb, st)
            amd.call("mri_hashgrid_backward", C.byref(desc), ptr(xd), ptr(dd), n, sl, sr, sf, ptr(g),
                     method | BWD_PREPARED | flags, ptr(ws), nb, st)
            return dict(d_table=g)
        return launch

    def levels(run, ws, nb):  # two level groups on one prepared workspace
        g = run.out((rows, feats), 0.0)
        amd.call("mri_hashgrid_backward_prepare", C.byref(desc), ptr(xd), n, method, ptr(ws), nb, st)
        for mask in (high, low):
            amd.call("mri_hashgrid_backward_levels", C.byref(desc), ptr(xd), ptr(dd), n, sl, sr, sf, ptr(g),
                     method | BWD_PREPARED, mask, ptr(ws), nb, st)
        return dict(d_table=g)

    def levels_unprepared(run, ws, nb):  # each call recounts; the second group's call finds the first one's leavings
        g = run.out((rows, feats), 0.0)
        for mask in (low, high):
            amd.call("mri_hashgrid_backward_levels", C.byref(desc), ptr(xd), ptr(dd), n, sl, sr, sf, ptr(g), method,
                     mask, ptr(ws), nb, st)
        return dict(d_table=g)

    def scaled(run, ws, nb):
        g = run.out((rows, feats))
        amd.call("mri_hashgrid_backward_scaled", C.byref(desc), ptr(xd), ptr(dd), n, sl, sr, sf, ptr(g),
                 method | BWD_OVERWRITE, (1 << L) - 1, ptr(absmax) if feats == 2 else None, ptr(ws), nb, st)
        return dict(d_table=g)

    def adam(run, ws, nb):
        p, m, v = run.out((rows, feats)), run.out((rows, feats)), run.out((rows, feats))
        if not run.refuse:
            p.copy_(seed), m.copy_(g0), v.copy_(g0 * g0)
        amd.call("mri_hashgrid_backward_adam", C.byref(desc), ptr(xd), ptr(dd), n, sl, sr, sf, ptr(p), ptr(m), ptr(v),
                 lr, b1, b2, eps, step, 0.5, method, ptr(ws), nb, st)
        return dict(param=p, exp_avg=m, exp_avg_sq=v)

    def adam_reference(d_table):
        """mri_adam_step on the gradient mri_hashgrid_backward left: the fused form is documented bit-identical."""
        p, m, v = seed.clone(), g0.clone(), g0 * g0
        amd.call("mri_adam_step", ptr(p), ptr(d_table), ptr(m), ptr(v), rows * feats, lr, b1, b2, eps, step, 0.5, st)
        torch.cuda.synchronize()
        return dict(param=p.cpu(), exp_avg=m.cpu(), exp_avg_sq=v.cpu())

    entries = {"backward": plain(0, None), "backward | OVERWRITE": plain(BWD_OVERWRITE, None),
               "backward onto a gradient": plain(0, g0),
               "prepare + PREPARED": prepared(0), "prepare + PREPARED | OVERWRITE": prepared(BWD_OVERWRITE),
               "backward_levels x 2, prepared": levels, "backward_levels x 2": levels_unprepared,
               "backward_scaled": scaled, "backward_adam": adam}
    return {k: (v, need) for k, v in entries.items()}, case, g0, adam_reference


def table_judge(amd, case, g0, adam_reference, tag):
    spans = np.cumsum([0] + list(case["sizes"]))
    state = {}

    def judge_for(entry):
        def judge(got):
            if entry == "backward_adam":
                want = adam_reference(state["d_table"])
                for name, value in got.items():
                    assert torch.equal(value, want[name]), f"{tag} {entry}: {name} differs from backward + mri_adam_step"
                return
            g = got["d_table"].double()
            if entry == "backward onto a gradient":
                g = g - g0.cpu().double()  # (accumulated onto values 1e-3 of the gradient's scale)
            for l in range(case["L"]):  # per level, REL_TOL of the float64 sum (test_gpu_layout.py)
                assert_close(g[spans[l]:spans[l + 1]].numpy(), case["grad"][spans[l]:spans[l + 1]].numpy(), REL_TOL,
                             f"{tag} {entry}: level {l}")
            if entry == "backward | OVERWRITE":
                state["d_table"] = got["d_table"].cuda()
        return judge
    return judge_for


def run_table_cases(amd, name, n, method, tag):
    small, case, g0, adam_reference = table_entries(amd, name, n, method)
    other = {"D3 F2": "D2 F4", "D4 F2": "D3 F2", "D2 F4": "D4 F2", "D3 F1": "D3 F2", "D3 F2 2^17": "D2 F4"}[name]
    big, *_ = table_entries(amd, other, 90001, method)
    judge_for = table_judge(amd, case, g0, adam_reference, tag)
    order = ["backward | OVERWRITE"] + [k for k in small if k != "backward | OVERWRITE"]  # (backward_adam's reference)
    for entry in order:
        launch, need = small[entry]
        hold(f"{tag} {entry}", launch, need, judge_for(entry), big[entry])


@pytest.mark.parametrize("method", [0, 2])
@pytest.mark.parametrize("n", HASH_N)
@pytest.mark.parametrize("name", list(GRIDS))
def test_table_gradient(amd, name, n, method):
    run_table_cases(amd, name, n, method, f"table gradient {name}, n = {n}, method {method}:")


KNOBS = [dict(bwd_records=1), dict(bwd_dense_max_parts=0), dict(bwd_fuse_dense=0), dict(bwd_blocks_per_level=1),
         dict(bwd_dense_blocks=1),
         dict(bwd_records=1, bwd_dense_max_parts=0, bwd_fuse_dense=0, bwd_blocks_per_level=1, bwd_dense_blocks=1)]


@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: " ".join(f"{a}={b}" for a, b in k.items()))
@pytest.mark.parametrize("name,n", [("D3 F2 2^17", 4097), ("D2 F4", 70001)])
def test_table_gradient_knobs(amd, option, name, n, knobs):
    """Every knob of make_plan at its other value (the defaults are bwd_records 0, bwd_dense_max_parts 4,
    bwd_fuse_dense 1, bwd_blocks_per_level 64, bwd_dense_blocks 96), set BEFORE the size is asked for."""
    for knob, value in knobs.items():
        option(knob, value)
    run_table_cases(amd, name, n, 0, f"table gradient {name}, n = {n}, {knobs}:")


def test_prepare_and_backward_with_different_byte_counts(amd):
    """mri_hashgrid_backward_prepare with the exact size, then MRI_BWD_PREPARED with a larger count over the same
    (larger, dirty) buffer: the layout of the workspace does not depend on the surplus, so the result is that of
    the pair on equal counts, bit for bit."""
    name, n = "D3 F2 2^17", 4097
    case = grid_case(name, n)
    desc = grid_desc(amd, case)
    rows, feats = sum(case["sizes"]), case["F"]
    xd, dd, st = case["x"].cuda(), case["d_out"].T.contiguous().cuda(), amd.stream()
    need = amd.h.mri_hashgrid_backward_workspace_bytes(C.byref(desc), n)
    results = []
    for surplus, fill in ((0, 0), (4096 + 48, 0), (4096 + 48, FILLS[0]), (1 << 20, FILLS[1])):
        ws, check = place_workspace(need + surplus, fill)
        g = torch.full((rows, feats), NAN, device="cuda")
        amd.call("mri_hashgrid_backward_prepare", C.byref(desc), ptr(xd), n, 0, ptr(ws), need, st)
        amd.call("mri_hashgrid_backward", C.byref(desc), ptr(xd), ptr(dd), n, feats * n, 1, n, ptr(g),
                 BWD_PREPARED | BWD_OVERWRITE, ptr(ws), need + surplus, st)
        check(f"prepare told {need}, backward told {need + surplus}")
        results.append(g)
    spans = np.cumsum([0] + list(case["sizes"]))
    for l in range(case["L"]):
        assert_close(results[0][spans[l]:spans[l + 1]].cpu().numpy(), case["grad"][spans[l]:spans[l + 1]].numpy(), REL_TOL,
                     f"equal byte counts: level {l}")
    for g, what in zip(results[1:], ("zero-filled", "0x5A", "0xFF")):
        assert torch.equal(bits(g), bits(results[0])), f"backward told a larger count over a {what} buffer differs"


# ================================================================================================ one-call training step
def test_fused_step(amd):
    """mri_fused_step, two consecutive steps: tiny_ws, bwd_ws and next_bwd_ws each exactly sized between guards and
    dirty; the workspace step 1 counts batch 2's records into is the bwd_ws of step 2 (so it is dirtied before step 1
    only), the other two are dirtied again between the steps.  absmax stays zeroed, as its contract says.  Step 1
    against float64; every buffer Adam owns after step 2 bit for bit that of the zero-filled run."""
    name, n, hidden = "D3 F2 2^17", 4097, 128
    case = grid_case(name, n)
    desc = grid_desc(amd, case)
    k = case["L"] * case["F"]
    tables = ohash.init_tables(case["sizes"], 2, 77, 0.5)
    dec = omlp.linear_init([k, hidden, hidden, 1], 11)
    target = uniform((n,), 121, 0.0, 1.0)
    shape = (20, 21, 22)
    axes = torch.cat([torch.linspace(0, 1, s) for s in shape]).cuda()
    volume = uniform((int(np.prod(shape)),), 81, 0.0, 1.0).cuda()
    pieces = [torch.cat(tables).reshape(-1)] + [q.reshape(-1) for wb in dec for q in wb]
    flat = torch.cat(pieces)
    starts = np.cumsum([0] + [q.numel() for q in pieces])
    tiny_bytes = amd.h.mri_tiny_mlp_workspace_bytes(k, hidden, n)
    bwd_bytes = amd.h.mri_hashgrid_backward_workspace_bytes(C.byref(desc), n)
    side, ev_fork, ev_join = torch.cuda.Stream(), torch.cuda.Event(), torch.cuda.Event()
    ev_fork.record(), ev_join.record()
    torch.cuda.synchronize()

    def two_steps(fill):
        word = fill - (1 << 32) if fill >= 1 << 31 else fill
        (tiny, check_tiny), (ws_a, check_a), (ws_b, check_b) = (place_workspace(b, fill)
                                                                for b in (tiny_bytes, bwd_bytes, bwd_bytes))
        param, grad = flat.cuda(), torch.zeros(flat.numel(), device="cuda")
        m, v = torch.zeros_like(grad), torch.zeros_like(grad)
        coords, tgt = case["x"].cuda(), target.cuda()
        next_idx = torch.zeros(n, dtype=torch.int64, device="cuda")
        next_coords, next_target = torch.full((n, 3), NAN, device="cuda"), torch.full((n,), NAN, device="cuda")
        enc, d_enc = torch.full((k, n), NAN, device="cuda"), torch.full((k, n), NAN, device="cuda")
        absmax, loss = torch.zeros(2, 32, device="cuda"), torch.full((1,), NAN, device="cuda")
        at = lambda t, i: t.data_ptr() + 4 * int(starts[i])  # noqa: E731
        a = amd.lib.FusedStepArgs()
        a.grid, a.table, a.d_table = C.pointer(desc), at(param, 0), at(grad, 0)
        a.w1, a.b1, a.w2, a.b2, a.w3, a.b3 = (at(param, i) for i in range(1, 7))
        a.d_w1, a.d_b1, a.d_w2, a.d_b2, a.d_w3, a.d_b3 = (at(grad, i) for i in range(1, 7))
        a.loss, a.hidden, a.bwd_method, a.counted, a.join_pending = loss.data_ptr(), hidden, 0, 0, 0
        a.coords, a.target, a.n, a.enc, a.d_enc = coords.data_ptr(), tgt.data_ptr(), n, enc.data_ptr(), d_enc.data_ptr()
        a.tiny_ws, a.tiny_ws_bytes, a.bwd_ws, a.bwd_ws_bytes = tiny.data_ptr(), tiny_bytes, ws_a.data_ptr(), bwd_bytes
        a.absmax, a.next_absmax = absmax[0].data_ptr(), absmax[1].data_ptr()
        a.param, a.grad, a.exp_avg, a.exp_avg_sq = param.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr()
        a.n_params, a.lr, a.beta1, a.beta2, a.eps, a.step, a.grad_scale = flat.numel(), 1e-2, 0.9, 0.999, 1e-8, 1, 1.0
        a.next_idx, a.next_coords, a.next_target, a.next_n = (next_idx.data_ptr(), next_coords.data_ptr(),
                                                              next_target.data_ptr(), n)
        a.next_bwd_ws, a.next_bwd_ws_bytes = ws_b.data_ptr(), bwd_bytes
        a.seed, a.first, a.lo, a.hi, a.dim, a.grad_divisor = 5, 0, 0, volume.numel(), 3, 1.0
        for d in range(3):
            a.shape[d], a.axis_offset[d] = shape[d], int(sum(shape[:d]))
        a.axes, a.volume = axes.data_ptr(), volume.data_ptr()
        a.stream = torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())
        a.stream_side, a.ev_fork, a.ev_join = side.cuda_stream, ev_fork.cuda_event, ev_join.cuda_event
        amd.call("mri_fused_step", C.byref(a))
        torch.cuda.synchronize()
        for check, what in ((check_tiny, "tiny_ws"), (check_a, "bwd_ws"), (check_b, "next_bwd_ws")):
            check(f"fused step 1, {what} filled with {fill:#010x}")
        first = dict(loss1=loss.clone(), grad1=grad[int(starts[1]):].clone(), next_coords=next_coords.clone(),
                     next_target=next_target.clone())
        assert bool(torch.isfinite(next_coords).all()) and bool(torch.isfinite(next_target).all())
        tiny.fill_(word), ws_a.fill_(word)  # (ws_b holds batch 2's count: private to the pair of steps)
        enc.fill_(NAN), d_enc.fill_(NAN)
        a.coords, a.target, a.counted, a.join_pending, a.step = next_coords.data_ptr(), next_target.data_ptr(), 1, 1, 2
        a.bwd_ws, a.absmax = ws_b.data_ptr(), absmax[1].data_ptr()
        a.next_idx, a.next_bwd_ws, a.next_bwd_ws_bytes, a.next_absmax = None, None, 0, None
        amd.call("mri_fused_step", C.byref(a))
        torch.cuda.synchronize()
        for check, what in ((check_tiny, "tiny_ws"), (check_a, "the other workspace"), (check_b, "bwd_ws")):
            check(f"fused step 2, {what} filled with {fill:#010x}")
        return dict(first, param=param, exp_avg=m, exp_avg_sq=v, loss2=loss.clone(), grad2=grad[int(starts[1]):].clone())

    base = two_steps(0)
    tabs = [t.double().requires_grad_(True) for t in tables]
    ps = [(w.double().clone().requires_grad_(True), b.double().clone().requires_grad_(True)) for w, b in dec]
    y = omlp.relu_mlp_forward(ohash.encode(case["x"], tabs, case["res"]), ps, final_activation=False)
    loss = omlp.mse_loss(y.reshape(-1), target.double())
    loss.backward()
    assert abs(float(base["loss1"]) - float(loss.detach())) <= REL_TOL * float(loss.detach())
    want = torch.cat([q.grad.reshape(-1) for wb in ps for q in wb])
    assert_close(base["grad1"].cpu().numpy(), want.numpy(), REL_TOL, "decoder gradients of step 1")
    assert not torch.equal(base["param"].cpu(), flat) and float(base["loss2"]) != float(base["loss1"])
    for fill in FILLS:
        got = two_steps(fill)
        for name, value in got.items():
            assert torch.equal(bits(value), bits(base[name])), f"workspaces filled with {fill:#010x}: {name} differs"


# ================================================================================================ the Python owners
def dirty(obj):
    """0xFF bytes over every CUDA tensor reachable from obj (dicts, lists, tuples)."""
    if isinstance(obj, torch.Tensor):
        if obj.is_cuda and obj.numel():
            (obj.view(torch.uint8) if obj.is_contiguous() else obj).fill_(255 if obj.is_contiguous() else NAN)
    elif isinstance(obj, dict):
        for v in obj.values():
            dirty(v)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            dirty(v)


def clean(obj):
    if isinstance(obj, torch.Tensor):
        if obj.is_cuda:
            obj.zero_()
    elif isinstance(obj, dict):
        for v in obj.values():
            clean(v)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            clean(v)


def owner_runs(amd, cache, grow, small, what):
    """`cache`: the dict ops keeps its scratch in.  grow() makes it large with a call of another shape; small() -> outputs
    runs on the zero-filled, then on the 0xFF-filled cache: the same bits."""
    grow()
    torch.cuda.synchronize()
    assert cache, f"{what}: the large call left no scratch behind"
    sizes = {k: v.numel() for k, v in cache.items()}
    clean(cache)
    base = small()
    torch.cuda.synchronize()
    dirty(cache)
    got = small()
    torch.cuda.synchronize()
    assert {k: v.numel() for k, v in cache.items()} == sizes, f"{what}: the small call replaced the large scratch"
    for name, value in got.items():
        assert torch.equal(bits(value), bits(base[name])), f"{what}: {name} differs on a scratch of 0xFF bytes"
    return base


def test_ops_backward_workspace(amd):
    ops = amd.ops
    small_case, big_case = grid_case("D3 F2 2^17", 2049), grid_case("D2 F4", 70001)

    def run(case):
        desc = grid_desc(amd, case)
        g = torch.zeros(sum(case["sizes"]), case["F"], device="cuda")
        ops.hashgrid_backward_prepare(desc, case["x"].cuda(), method=0)
        ops.hashgrid_backward(desc, case["x"].cuda(), case["d_out"].cuda(), g, method=0, prepared=True)
        g2 = torch.full_like(g, NAN)
        ops.hashgrid_backward(desc, case["x"].cuda(), case["d_out"].cuda(), g2, method=2, overwrite=True)
        return dict(prepared=g, overwritten=g2)
    base = owner_runs(amd, ops._bwd_workspace, lambda: run(big_case), lambda: run(small_case), "ops.backward_workspace")
    for name, value in base.items():
        assert_close(value.cpu().numpy(), small_case["grad"].numpy(), REL_TOL, f"ops.hashgrid_backward: {name}")


def test_ops_tiny_workspace(amd):
    ops = amd.ops

    def run(k_in, hidden, n):
        params, x, t = tiny_inputs(k_in, hidden, n)
        par = [(w.cuda(), b.cuda()) for w, b in params]
        grads = [(torch.full_like(w, NAN), torch.full_like(b, NAN)) for w, b in par]
        loss, d_x, y = (torch.full(s, NAN, device="cuda") for s in ((1,), (k_in, n), (n,)))
        ops.tiny_mlp_train(x.T.contiguous().cuda(), t.cuda(), par, grads, loss, d_x=d_x, y=y, overwrite=True)
        out = dict(loss=loss, d_x=d_x, y=y)
        for i, (gw, gb) in enumerate(grads):
            out[f"d_w{i + 1}"], out[f"d_b{i + 1}"] = gw, gb
        return out
    base = owner_runs(amd, ops._mlp_workspace, lambda: run(32, 64, 70001), lambda: run(7, 128, 2501), "ops._tiny_workspace")
    judge_close(tiny_refs(7, 128, 2501), "ops.tiny_mlp_train")({k: v.cpu() for k, v in base.items()})


def test_ops_shallow_workspace(amd):
    ops = amd.ops

    def run(k_in, hidden, n):
        (x, t, w1, b1, w2, b2), _, _ = shallow_case(k_in, hidden, n)
        par = [(w1.cuda(), b1.cuda()), (w2.cuda(), b2.cuda())]
        grads = [(torch.full_like(w, NAN), torch.full_like(b, NAN)) for w, b in par]
        loss, d_x, y = (torch.full(s, NAN, device="cuda") for s in ((1,), (k_in, n), (n,)))
        ops.shallow_mlp_train(x.T.contiguous().cuda(), t.reshape(-1).cuda(), par, (3, 3), grads, loss, d_x=d_x, y=y,
                              overwrite=True)
        return dict(loss=loss, d_x=d_x, y=y, d_w1=grads[0][0], d_b1=grads[0][1], d_w2=grads[1][0], d_b2=grads[1][1])
    base = owner_runs(amd, ops._shallow_workspace_cache, lambda: run(32, 128, 70001), lambda: run(5, 32, 3001),
                      "ops._shallow_workspace")
    _, f32, f64 = shallow_case(5, 32, 3001)
    for name, value in base.items():
        assert_no_worse(value.cpu().numpy().reshape(-1), f32[name].numpy().reshape(-1), f64[name].numpy().reshape(-1),
                        f"ops.shallow_mlp_train: {name}")


def test_ops_siren_scratch(amd):
    ops = amd.ops

    def run(hidden, L, n, dim_in):
        params, x, t = siren_inputs(hidden, L, n, dim_in)
        w, b = [p[0].cuda() for p in params], [p[1].cuda() for p in params]
        new = lambda: torch.full((n, hidden), NAN, device="cuda")  # noqa: E731
        act, der = [new() for _ in range(L - 1)] + [None], [new() for _ in range(L - 1)] + [None]
        dz = [None] + [new() for _ in range(1, L)]
        d_w, d_b = [torch.zeros_like(v) for v in w], [torch.zeros_like(v) for v in b]
        y, loss = torch.full((n, 1), NAN, device="cuda"), torch.zeros(1, device="cuda")
        xd = x.cuda()
        ops.siren_forward_loss(xd, t.reshape(-1, 1).cuda(), w, b, 30.0, 30.0, act, der, dz[-1], y, d_w[L], d_b[L],
                               d_b[L - 1], loss)
        ops.siren_backward(xd, None, w, act, der, dz, d_w, d_b, head_done=True)
        out = dict(y=y.reshape(-1), loss=loss)
        for l in range(L + 1):
            out[f"d_w{l}"], out[f"d_b{l}"] = d_w[l], d_b[l]
        return out
    base = owner_runs(amd, ops._siren_workspace, lambda: run(128, 3, 70001, 2), lambda: run(64, 5, 3001, 3),
                      "ops._siren_scratch")
    judge_close(siren_refs(64, 5, 3001, 3), "ops.siren_forward_loss + siren_backward")({k: v.cpu() for k, v in base.items()})


def test_ops_modsiren_workspace(amd):
    """ops.modsiren_workspace hands the caller a buffer of its own: sized for a larger batch of another depth it still
    serves the small calls, whatever it holds."""
    ops = amd.ops
    hidden, L, n, dim_in = 64, 2, 3001, 1
    siren, mod, x, t = modsiren_inputs(hidden, L, n, dim_in)
    sw, sb = [p[0].cuda() for p in siren], [p[1].cuda() for p in siren]
    mw, mb = [p[0].cuda() for p in mod], [p[1].cuda() for p in mod]
    ws = ops.modsiren_workspace(70001, hidden, 6, torch.device("cuda", torch.cuda.current_device()))
    assert ws.numel() * 4 > amd.h.mri_modsiren_backward_workspace_bytes(n, hidden, L)

    def run():
        new = lambda *s: torch.full(s, NAN, device="cuda")  # noqa: E731
        saved = {key: [new(n, hidden) for _ in range(L)] for key in ("act", "hid", "dcos", "sn")}
        dzs, dzm = [None] + [new(n, hidden) for _ in range(1, L)], [None] + [new(n, hidden) for _ in range(1, L)]
        y, dy, loss = new(n, 1), new(n, 1), torch.zeros(1, device="cuda")
        g = [[torch.zeros_like(v) for v in group] for group in (sw, sb, mw, mb)]
        xd = x.cuda()
        ops.modsiren_forward_loss(xd, t.reshape(-1, 1).cuda(), sw, sb, mw, mb, 30.0, 30.0, saved, y, dy, loss, ws=ws)
        ops.modsiren_backward(xd, dy, sw, mw, saved, dzs, dzm, g[0], g[1], g[2], g[3], ws=ws)
        out = dict(y=y.reshape(-1), loss=loss, dy=dy.reshape(-1))
        for l in range(L + 1):
            out[f"s_w{l}"], out[f"s_b{l}"] = g[0][l], g[1][l]
        for l in range(L):
            out[f"m_w{l}"], out[f"m_b{l}"] = g[2][l], g[3][l]
        return out
    ws.zero_()
    base = run()
    torch.cuda.synchronize()
    dirty(ws)
    got = run()
    torch.cuda.synchronize()
    for name, value in got.items():
        assert torch.equal(bits(value), bits(base[name])), f"ops.modsiren_workspace: {name} differs on 0xFF bytes"
    judge_modsiren(modsiren_refs(hidden, L, n, dim_in), "ops.modsiren_*")({k: v.cpu() for k, v in base.items()})


def test_ops_rff_scratch(amd):
    """ops._rff_ws behind rff_forward and rff_gradient: the references and the judgement of test_gpu_rff_gradient.py."""
    from test_gpu_rff_gradient import reference
    from test_gpu_rff_step import close_or_no_worse as judge, he_init, selected_rows, uniform as unit
    ops = amd.ops
    x_all, _, b, params, r64, r32 = selected_rows(2, 64, 3)
    x = x_all[:300].contiguous()

    def run(x, b, params):
        bc, ws, bs = b.cuda(), [w.cuda() for w, _ in params], [v.cuda() for _, v in params]
        n, d = x.shape
        y, y2, dydx = (torch.full(s, NAN, device="cuda") for s in ((n, 1), (n, 1), (n, d)))
        ops.rff_forward(x.cuda(), bc, ws, bs, y=y)
        ops.rff_gradient(x.cuda(), bc, ws, bs, y=y2, dydx=dydx)
        return dict(y=y.reshape(-1), gradient_y=y2.reshape(-1), dydx=dydx)
    base = owner_runs(amd, ops._rff_ws, lambda: run(unit((300, 3), 41), *he_init(3, 128, 4, 9741, 1.0)),
                      lambda: run(x, b, params), "ops._rff_ws")
    (y32, g32, _), (y64, g64, _) = reference(r32, x), reference(r64, x)
    for name, f32, f64 in (("y", y32, y64), ("gradient_y", y32, y64), ("dydx", g32, g64)):
        judge(base[name].cpu().numpy(), f32.numpy(), f64.numpy(), f"ops.rff_forward / rff_gradient: {name}")


def test_ops_rff_train_scratch(amd):
    """ops._rff_train_ws behind rff_forward_loss + rff_backward without a workspace of the caller's: the references and
    the judgement of test_gpu_rff_step.py."""
    from test_gpu_rff_step import close_or_no_worse as judge, he_init, kernel_pass, names, scalar, selected_rows, \
        uniform as unit
    x_all, y_all, b, params, r64, r32 = selected_rows(2, 64, 3)
    x, t = x_all[:300].contiguous(), y_all[:300].contiguous()

    def run(x, t, b, params):
        y, dy, loss, grads = kernel_pass(amd, b, params, x, t)
        return dict(zip(names(len(params)), grads), y=y, dy=dy, loss=loss)
    base = owner_runs(amd, amd.ops._rff_train_ws,
                      lambda: run(unit((3001, 3), 42), unit((3001, 1), 43), *he_init(3, 128, 4, 9742, 1.0)),
                      lambda: run(x, t, b, params), "ops._rff_train_ws")
    (p32, l32, g32), (p64, l64, g64) = r32.loss_and_grads(x, t), r64.loss_and_grads(x, t)
    judge(base["y"].cpu().numpy(), p32.numpy(), p64.numpy(), "ops.rff_forward_loss: y")
    judge(scalar(base["loss"]), scalar(l32), scalar(l64), "ops.rff_forward_loss: loss")
    for name, c32, c64 in zip(names(len(params)), g32, g64):
        judge(base[name].cpu().numpy(), c32.numpy(), c64.numpy(), f"ops.rff_backward: {name}")


def test_ops_gabor_scratch(amd):
    """ops._gabor_ws behind gabor_forward: the reference and the judgement of test_gpu_gabor.py."""
    import gabor_ref
    from test_gpu_gabor import device_params, fused_case
    w0, c = 5.0, 1.0
    x, params, y32, y64 = fused_case(2, 64, 3, w0, c, 300)

    def run(x, params):
        y = torch.full((x.shape[0], 1), NAN, device="cuda")
        amd.ops.gabor_forward(x.cuda(), *device_params(params), w0, c, y=y)
        return dict(y=y.reshape(-1))
    base = owner_runs(amd, amd.ops._gabor_ws,
                      lambda: run(gabor_ref.uniform((300, 3), 44), gabor_ref.grid_params(3, 128, 4, 9744)),
                      lambda: run(x, params), "ops._gabor_ws")
    assert_no_worse(base["y"].cpu().numpy(), y32.numpy(), y64.numpy(), "ops.gabor_forward: y")


def test_ops_modsiren_scratch(amd):
    """ops._modsiren_ws behind the inference form of modsiren_forward and modsiren_gradient, neither with a workspace of
    the caller's: modsiren_refs and, for dydx, float64 autograd through it (test_gpu_modsiren_gradient.reference)."""
    from test_gpu_modsiren_gradient import reference
    ops = amd.ops
    small, big = (64, 2, 300, 3), (128, 3, 3001, 3)

    def run(hidden, L, n, dim_in):
        siren, mod, x, _ = modsiren_inputs(hidden, L, n, dim_in)
        par = [[p[k].cuda() for p in stack] for stack in (siren, mod) for k in (0, 1)]
        y, y2, dydx = (torch.full(s, NAN, device="cuda") for s in ((n, 1), (n, 1), (n, dim_in)))
        ops.modsiren_forward(x.cuda(), *par, 30.0, 30.0, y=y)
        ops.modsiren_gradient(x.cuda(), *par, 30.0, 30.0, y=y2, dydx=dydx)
        return dict(y=y.reshape(-1), gradient_y=y2.reshape(-1), dydx=dydx)
    base = {k: v.cpu() for k, v in owner_runs(amd, ops._modsiren_ws, lambda: run(*big), lambda: run(*small),
                                              "ops._modsiren_ws").items()}
    judge_modsiren(modsiren_refs(*small), "ops.modsiren_forward")(dict(y=base["y"]))
    judge_modsiren(modsiren_refs(*small), "ops.modsiren_gradient")(dict(y=base["gradient_y"]))
    siren, mod, x, _ = modsiren_inputs(*small)
    (_, g32), (_, g64) = (reference(x, siren, mod, 30.0, 30.0, dtype) for dtype in (torch.float32, torch.float64))
    close_or_no_worse(base["dydx"].numpy(), g32.numpy(), g64.numpy(), "ops.modsiren_gradient: dydx")


def _hash_net(models, **kw):
    return models.HashMLP(3, 8, 2, 15, 16, 256, dim_out=1, lr=5e-3, **kw)


PLANS = {  # plan -> (model factory, FusedStep keywords, dim_in)
    "tiny-MLP hash": (lambda m: _hash_net(m, dim_hidden=128, n_layers=3, activation=torch.nn.ReLU, batch_norm=False,
                                          final_activation=False), {}, 3),
    "shallow": (lambda m: _hash_net(m, dim_hidden=64, n_layers=2, activation=torch.nn.GELU, batch_norm=False), {}, 3),
    "BatchNorm": (lambda m: _hash_net(m, dim_hidden=64, n_layers=3), dict(batch_norm=True), 3),
    "SIREN chain 64": (lambda m: m.SirenNet(3, 64, 1, 4, lr=1e-3), {}, 3),
    "SIREN chain 256": (lambda m: m.SirenNet(3, 256, 1, 3, lr=1e-3), {}, 3),
    "modulated": (lambda m: m.ModulatedSirenNet(dim_in=2, dim_hidden=64, dim_out=1, n_layers=3, lr=1e-3),
                  dict(modulated=True), 2),
    "PSF": (lambda m: m.PsfSirenNet(dim_in=3, dim_hidden=64, n_layers=3, lr=1e-3, coordinates_spacing=(0.01, 0.01, 0.01),
                                    n_sample=3), {}, 3),
}


@pytest.mark.parametrize("plan", list(PLANS))
def test_fused_step_owns_clean_scratch(amd, plan):
    """trainer.FusedStep, one case per plan: two identical models, three steps each on the same batches; the second
    model's scratch (everything reachable from _ws and _bwd_ws, after forget_ahead(): the prepared count of the next
    batch legitimately lives in _bwd_ws between steps) is filled with 0xFF bytes before every step.  Parameters,
    Adam moments and losses: the same bits.

    The BatchNorm plan is the one plan that trains through the layer kernels, i.e. through mri_mse_loss and
    mri_linear_backward_weight, whose float atomics add in no fixed order (include/mri_inr.h): at 1500 rows two runs
    on CLEAN scratch differ (parameters by 2.0e-2 .. 2.4e-2 of their maximum after three steps), which says nothing
    about scratch.  Its batch is therefore 100 rows: mri_linear_backward_weight cuts the batch into
    ceil(m / (4 * 32)) splits and mri_mse_loss into ceil(count / 256) workgroups (csrc/linear.hip, train_ops.hip), so
    up to 128 rows every atomic destination receives exactly ONE addend, onto zero -- an ordered sum.  The plan's
    scratch (enc, d_enc, y, deriv, dz, z, bn_save, bn_ws, both _bwd_ws) is all in use at that size."""
    from mri_interpolation_amd import models, trainer
    factory, kw, dim_in = PLANS[plan]
    n = 100 if plan == "BatchNorm" else 1500
    batches = [(uniform((n, dim_in), 200 + s, 0.0, 1.0).cuda(), uniform((n, 1), 300 + s, 0.0, 1.0).cuda())
               for s in range(3)]

    def train(dirt):
        torch.manual_seed(1234)
        net = factory(models).cuda()
        step = trainer.FusedStep(net, net.configure_optimizers(), **kw)
        assert {"tiny-MLP hash": step.use_tiny, "shallow": step.use_shallow, "BatchNorm": step.bn,
                "modulated": step.use_modulated, "PSF": step.psf is not None}.get(plan, step.use_chain), plan
        losses = []
        for x, y in batches:
            if dirt:
                step.forget_ahead()
                torch.cuda.synchronize()
                dirty(step._ws), dirty(step._bwd_ws)
            losses.append(step.train_step(x, y).clone())
        torch.cuda.synchronize()
        if dirt:
            assert step._ws, "the step kept no workspace: nothing was dirtied"
        return dict(param=step.flat.param.clone(), exp_avg=step.flat.exp_avg.clone(),
                    exp_avg_sq=step.flat.exp_avg_sq.clone(), losses=torch.cat([l.reshape(1) for l in losses]))

    base, got = train(False), train(True)
    assert bool(torch.isfinite(base["losses"]).all()) and bool(torch.isfinite(base["param"]).all())
    again = train(False) if plan == "BatchNorm" else base  # (do two runs on clean scratch agree at all?)
    for name, value in got.items():
        d = (value.double() - base[name].double()).abs().max() / base[name].double().abs().max()
        same = torch.equal(bits(again[name]), bits(base[name]))
        print(f"FusedStep ({plan}) {name}: dirty against clean {float(d):.2e} of the maximum; two clean runs "
              f"{'agree' if same else 'DIFFER'} bit for bit")
        assert torch.equal(bits(value), bits(base[name])), \
            (f"FusedStep ({plan}): {name} differs after three steps ({float(d):.2e} of its maximum; two runs on clean "
             f"scratch {'agree' if same else 'differ too'})")
