"""The inputs of the Poisson-disk tests (tests/test_poisson_host.py on the CPU, tests/test_gpu_poisson.py on the device), and a
cache of what tests/poisson_ref.py says about them: a reference is computed once per (cloud, radius) and never changed."""
import numpy as np

import poisson_ref as R

F32 = np.float32
RESIDENT_MAX = 8192                                   # sapcu_amd.poisson.PD_RESIDENT_MAX (asserted equal by the GPU tests)


def sphere(C, seed=0):
    g = np.random.default_rng(seed).standard_normal((C, 3))
    return (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(F32)


def plane(C, seed=1):
    p = np.random.default_rng(seed).random((C, 3))
    p[:, 2] = 0.5
    return p.astype(F32)


def equal(C):
    return np.tile(np.array([[0.3, -0.4, 0.5]], F32), (C, 1))


def lattice():
    """4 x 4 x 4 points at spacing 0.25: every coordinate, difference and squared distance is exact in f32."""
    a = np.arange(4, dtype=F32) * F32(0.25)
    return np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3).astype(F32)


def offset(C, seed=2):
    """A unit sphere around (1000, 1000, 1000): the coordinates carry 2^-14 of absolute rounding, and so does the binning."""
    return (sphere(C, seed) + F32(1000)).astype(F32)


def line(C=300):
    """The adversarial case: a sorted line at spacing 0.01; at r = 0.015 every point waits for the one before it."""
    p = np.zeros((C, 3), F32)
    p[:, 0] = np.arange(C, dtype=F32) * F32(0.01)
    return p


def typical_radius(C, area=4 * np.pi):
    """About the radius at which a surface of `area` keeps a quarter of C candidates (0.7 sqrt(area / n), the prototype's figure)."""
    return F32(0.7 * np.sqrt(area / max(C / 4.0, 1.0)))


CLOUDS = {"sphere": sphere, "plane": plane, "equal": equal, "offset": offset}
_cache = {}


def _key(P, r):
    return (P.shape, P.tobytes(), F32(r).tobytes())


def ref_select(P, r):
    """(keep, count) of poisson_ref.select, cached."""
    k = ("select",) + _key(P, r)
    if k not in _cache:
        _cache[k] = R.select(P, r)
    return _cache[k]


def ref_rounds(P, r):
    """(keep, count, rounds) of poisson_ref.select_rounds, cached."""
    k = ("rounds",) + _key(P, r)
    if k not in _cache:
        _cache[k] = R.select_rounds(P, r)
    return _cache[k]


def ref_subsample(P, n, steps):
    k = ("subsample", n, steps) + _key(P, 0)
    if k not in _cache:
        _cache[k] = R.subsample(P, n, steps, selector=ref_select)
    return _cache[k]
