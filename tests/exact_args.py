"""Arguments for the device-math tests (tests/test_gpu_device_math.py): float32 values that a kernel can be made
to evaluate sin / cos / GELU at EXACTLY, so that the float64 reference is the function of the same number the
kernel saw and no argument rounding is amplified (sin near 8192 turns one ulp of its argument into 1e-3).

Pure numpy, deterministic: the order is a fixed oracle.detrand permutation, so that every row tile of a kernel mixes
magnitudes, signs, and in-range with out-of-range values (the cold paths run beside the fast ones).
"""
import numpy as np

from oracle import detrand

HALF_PI = np.pi / 2
FAST_LIMIT = np.float32(8192.0)  # csrc/device_math.h: beyond it, the library sincosf
K_MAX = 5215                     # the last multiple of pi/2 below 8192
N_K = 500
N_LOG = 512
N_BIG = 500
MAX_LEN = 8192
U23 = 2.0 ** -23


def _neighbours(v):
    """The float32 nearest to each float64 v and its neighbours at +-1 and +-2 ulp: (len(v), 5)."""
    c = np.asarray(v, dtype=np.float64).astype(np.float32)
    up1, dn1 = np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))
    up2, dn2 = np.nextafter(up1, np.float32(np.inf)), np.nextafter(dn1, np.float32(-np.inf))
    return np.stack([dn2, dn1, c, up1, up2], axis=1)


def quadrant_ks():
    """N_K signed quadrant numbers spread over 1 ... K_MAX: both parities with both signs (the step of ~10.45 mixes
    the parities, the sign follows the index in pairs).  k = 0 stays out: its neighbours are denormals, below the
    2^-20 the set starts at; exactly 0.0 is in the set on its own."""
    k = np.rint(np.linspace(1, K_MAX, N_K)).astype(np.int64)
    sign = np.where((np.arange(N_K) // 2) % 2 == 0, 1, -1)
    return k * sign


def _shuffled(v, seed):
    order = np.argsort(detrand.unit24(v.size, seed), kind="stable")
    return np.ascontiguousarray(v[order], dtype=np.float32)


def sincos_arguments():
    """float32 (6531,): see the module docstring of tests/test_gpu_device_math.py for what each part is there for."""
    mags =np.exp2(np.linspace(-20.0, 13.0, N_LOG)).astype(np.float32)
    mags[0], mags[-1] = np.float32(2.0 ** -20), FAST_LIMIT
    k = quadrant_ks().astype(np.float64)
    multiples = _neighbours(k * HALF_PI).ravel()                        # one of sin / cos ~ 0, the other ~ +-1
    ties = _neighbours((k + np.sign(k) * 0.5) * HALF_PI).ravel()        # r ~ +-pi/4: the rintf tie
    edge = np.array([FAST_LIMIT, np.nextafter(FAST_LIMIT, np.float32(0)), np.nextafter(FAST_LIMIT, np.float32(np.inf)),
                     -FAST_LIMIT, -np.nextafter(FAST_LIMIT, np.float32(0)),
                     -np.nextafter(FAST_LIMIT, np.float32(np.inf))], dtype=np.float32)
    big = np.exp2(np.linspace(13.0, 30.0, N_BIG + 1)[1:]).astype(np.float32)  # (8192, 2^30]: the library path
    big[-1] = np.float32(2.0 ** 30)
    big = big * np.where(np.arange(N_BIG) % 2 == 0, 1.0, -1.0).astype(np.float32)
    v = np.concatenate([mags, -mags, multiples, ties, edge, big, np.zeros(1, np.float32)]).astype(np.float32)
    assert v.size <= MAX_LEN and np.isfinite(v).all()
    return _shuffled(v, 20261)


def gelu_arguments():
    """float32: 200 values per binade [2^e, 2^(e+1)), e = -6 ... 2, both signs; 0; +-(6 ... 12) where erff saturates."""
    parts = [np.zeros(1)]
    for e in range(-6, 3):
        m = np.exp2(e) * (1.0 + np.arange(200) / 200.0)
        parts += [m, -m]
    sat = np.linspace(6.0, 12.0, 49)
    parts += [sat, -sat]
    v = np.concatenate(parts).astype(np.float32)
    assert v.size <= MAX_LEN
    return _shuffled(v, 20262)


def near_grid_count(v, offset):
    """How many values of v lie within 2 ulp (of their own magnitude) of (k + offset) pi/2 for an integer k >= 1
    (offset 0: the multiples; 0.5: the ties), counted on |v|."""
    a = np.abs(v.astype(np.float64))
    k = np.rint(a / HALF_PI - offset)
    grid = ((k + offset) * HALF_PI).astype(np.float32).astype(np.float64)
    ulp = np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)
    return int(np.count_nonzero((k >= 1) & (np.abs(a - grid) <= 2.0 * ulp)))


def sin_bound(u):
    """|sin_kernel(u) - sin64(u)| <= 2^-23 min(1, 2 |u|) for every finite float32 u (cos: 2^-23)."""
    return U23 * np.minimum(1.0, 2.0 * np.abs(np.asarray(u, dtype=np.float64)))


def binade(z):
    """Binade index of |z| (floor(log2 |z|)); zeros get their own index -200."""
    z = np.asarray(z, dtype=np.float64)
    _, e = np.frexp(np.abs(z))
    return np.where(z == 0, -200, e - 1).astype(np.int64)
