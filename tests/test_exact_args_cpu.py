"""The argument sets of tests/exact_args.py hold what the device-math tests rely on, and the bound those tests hold
the kernels to is reachable by a correct float32 evaluation on exactly these inputs (no GPU needed)."""
import numpy as np
import torch

import exact_args as ea


def test_sets_are_reproducible_and_small():
    a, b = ea.sincos_arguments(), ea.sincos_arguments()
    assert a.dtype == np.float32 and a.tobytes() == b.tobytes()
    g, h = ea.gelu_arguments(), ea.gelu_arguments()
    assert g.dtype == np.float32 and g.tobytes() == h.tobytes()
    assert 2000 <= a.size <= ea.MAX_LEN and 2000 <= g.size <= ea.MAX_LEN
    assert np.isfinite(a).all() and np.isfinite(g).all()
    # shuffled: neither sorted, and every 64-row stretch of the sine set mixes signs and both sides of 8192
    assert not (np.diff(a) >= 0).all() and not (np.diff(g) >= 0).all()
    blocks = a[:a.size // 64 * 64].reshape(-1, 64)
    assert ((blocks > 0).any(1) & (blocks < 0).any(1)).all()
    assert np.count_nonzero((np.abs(blocks) > 8192).any(1) & (np.abs(blocks) <= 8192).any(1)) >= 0.9 * len(blocks)


def test_sine_set_contents():
    v = ea.sincos_arguments()
    k = ea.quadrant_ks()
    assert len(k) == ea.N_K and np.abs(k).min() >= 1 and np.abs(k).max() == ea.K_MAX
    for parity in (0, 1):  # odd and even, positive and negative quadrant numbers
        assert np.count_nonzero((k > 0) & (np.abs(k) % 2 == parity)) >= 50
        assert np.count_nonzero((k < 0) & (np.abs(k) % 2 == parity)) >= 50
    assert ea.near_grid_count(v, 0.0) >= 5 * ea.N_K
    assert ea.near_grid_count(v, 0.5) >= 5 * ea.N_K
    assert ea.near_grid_count(v[v < 0], 0.0) >= 1000 and ea.near_grid_count(v[v > 0], 0.0) >= 1000
    lim = np.float32(8192.0)
    for s in (1.0, -1.0):
        assert (v == np.float32(s) * lim).any()
    assert (v == np.nextafter(lim, np.float32(0))).any() and (v == np.nextafter(lim, np.float32(np.inf))).any()
    mag = np.abs(v)
    assert mag[mag > 0].min() == np.float32(2.0 ** -20) and mag.max() == np.float32(2.0 ** 30)
    assert np.count_nonzero(mag > 8192) >= ea.N_BIG and np.count_nonzero(v == 0) == 1
    assert np.count_nonzero((mag >= 2.0 ** -20) & (mag < 1)) >= 500  # the small end, where the bound is relative


def test_gelu_set_contents():
    g = ea.gelu_arguments()
    b = ea.binade(g)
    for e in range(-6, 3):
        assert np.count_nonzero((b == e) & (g > 0)) >= 200 and np.count_nonzero((b == e) & (g < 0)) >= 200
    assert (g == 0).any() and (g == 12).any() and (g == -12).any() and (g == 6).any() and (g == -6).any()
    assert np.abs(g).max() == 12 and np.abs(g[g != 0]).min() == np.float32(2.0 ** -6)


def _fma(a, b, c):
    """fmaf: the product of two float32 is exact in float64; the sum is rounded to float64, then to float32."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def sincos_fast_host(u, c2=-7.54978941586159635335e-08, s1=-1.6666654611e-1, quadrant=None, pair_fault=False):
    """csrc/device_math.h sincos_fast, operation for operation, in numpy (|u| <= 8192), with the faults to inject."""
    f = np.float32
    u = np.asarray(u, dtype=np.float32)
    k = np.rint(u * f(0.636619772367581343))
    r = _fma(k, f(-1.57079625129699707031e+00), u)
    r = _fma(k, f(c2), r)
    r = _fma(k, f(-5.39030252995776476554e-15), r)
    z = r * r
    ps = _fma(f(-1.9515295891e-4), z, f(8.3321608736e-3))
    ps = _fma(ps, z, f(s1))
    sn = _fma(ps * z, r, r)
    pc = _fma(f(2.443315711809948e-5), z, f(-1.388731625493765e-3))
    pc = _fma(pc, z, f(4.166664568298827e-2))
    cs = _fma(pc * z, z, _fma(f(-0.5), z, f(1.0)))
    q = k.astype(np.int64) & 3 if quadrant is None else quadrant(k)
    if pair_fault:  # the second element of each packed pair takes the first's quadrant
        q = q.copy()
        q[1::2] = q[0:-1:2][:q[1::2].size]
    s_, c_ = np.where(q & 1, cs, sn), np.where(q & 1, sn, cs)
    return np.where(q & 2, -s_, s_).astype(np.float32), np.where((q + 1) & 2, -c_, c_).astype(np.float32)


def _misses(s, c, u):
    u64 = u.astype(np.float64)
    return (int(np.count_nonzero(~(np.abs(s - np.sin(u64)) <= ea.sin_bound(u64)))),
            int(np.count_nonzero(~(np.abs(c - np.cos(u64)) <= ea.U23))))


def test_bound_on_this_set_sees_the_faults_it_is_for():
    """A host restatement of sincos_fast meets the bound on the first-layer arguments s_j x_i of the GPU tests (its
    maxima, 8.54e-8 / 8.41e-8, are the ones the kernels show on the MI355X), and stops meeting it with: a wrong third
    digit in the second Cody-Waite constant, a wrong sixth digit in the sine polynomial's leading coefficient, a quadrant
    taken from |k| (wrong for negative odd k), a pair whose second element takes the first's quadrant.  (What the
    bound cannot see, for the record: the fourth digit of that constant moves the maximum to 1.15e-7, the seventh of
    that coefficient to 9.8e-8 -- both under 2^-23.)"""
    v = ea.sincos_arguments()
    u = np.concatenate([v, np.float32(2) * v])
    u = u[np.abs(u) <= 8192]
    assert _misses(*sincos_fast_host(u), u) == (0, 0)
    faults = {"c2 third digit": dict(c2=-7.55978941586159635335e-08),
              "s1 sixth digit": dict(s1=-1.6666554611e-1),
              "quadrant from |k|": dict(quadrant=lambda k: np.abs(k).astype(np.int64) & 3),
              "pair": dict(pair_fault=True)}
    for name, kw in faults.items():
        bad_s, bad_c = _misses(*sincos_fast_host(u, **kw), u)
        assert bad_s >= 1000 and bad_c >= 1000, (name, bad_s, bad_c)


def test_bound_is_reachable_in_float32():
    """torch's CPU float32 sin / cos of the set sit within the bound the kernels are held to."""
    v = ea.sincos_arguments()
    t = torch.from_numpy(v)
    s64, c64 = np.sin(v.astype(np.float64)), np.cos(v.astype(np.float64))
    es = np.abs(torch.sin(t).numpy().astype(np.float64) - s64)
    ec = np.abs(torch.cos(t).numpy().astype(np.float64) - c64)
    assert (es <= ea.sin_bound(v)).all(), (es / ea.sin_bound(np.where(v == 0, 1, v))).max()
    assert (ec <= ea.U23).all(), ec.max()
    assert torch.sin(t)[t == 0].item() == 0.0 and torch.cos(t)[t == 0].item() == 1.0
