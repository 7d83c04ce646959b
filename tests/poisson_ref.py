"""Poisson-disk selection of csrc/sapcu_poisson.h restated in numpy: f32, one separately rounded operation per step, brute force.

It is the reference of tests/test_gpu_poisson.py (``==`` on every output) and has no grid: the device's cell grid is only an
accelerator, and these functions are what it has to reproduce.

  select(P, r)         the greedy definition: row i is kept iff no kept lower row j has d2(i, j) < r2 (strict), r2 = r * r,
                       d2 = (dx*dx + dy*dy) + dz*dz with dx = P[i,0] - P[j,0] and so on.
  select_rounds(P, r)  the synchronous parallel form — a candidate is accepted once every lower row within r is rejected, rejected
                       once one of them is accepted, and stays undecided until then; every round reads the states the round before
                       left — with the number of rounds it ran (at least one).  Same set as ``select``.
  subsample(P, n, steps)  the bisection on r whose last ``lo`` keeps at least n rows, and the first n kept rows.
"""
import numpy as np

F32 = np.float32


def radius2(r):
    r = F32(r)
    return F32(r * r)


def select(P, r):
    """(keep bool [C], count)."""
    P = np.ascontiguousarray(P, F32)
    r2 = radius2(r)
    keep = np.zeros(len(P), bool)
    kept = np.zeros_like(P)                           # the kept lower rows, in order: only they can drop row i
    m = 0
    for i in range(len(P)):
        d = P[i][None, :] - kept[:m]
        d = d * d
        if not np.any(((d[:, 0] + d[:, 1]) + d[:, 2]) < r2):
            keep[i] = True
            kept[m] = P[i]
            m += 1
    return keep, m


def conflicts(P, r, chunk=256):
    """(I, J) int64: every pair with J < I and d2(I, J) < r2, from the full table of distances, `chunk` rows at a time."""
    P = np.ascontiguousarray(P, F32)
    r2 = radius2(r)
    I, J = [], []
    for a in range(0, len(P), chunk):
        b = min(a + chunk, len(P))
        d = P[a:b, None, :] - P[None, :b, :]
        d *= d
        near = ((d[..., 0] + d[..., 1]) + d[..., 2]) < r2
        near &= np.arange(b)[None, :] < np.arange(a, b)[:, None]
        i, j = np.nonzero(near)
        I.append(i + a)
        J.append(j)
    return np.concatenate(I), np.concatenate(J)


def select_rounds(P, r):
    """(keep bool [C], count, rounds): the synchronous-round form; every round reads the states the round before left."""
    I, J = conflicts(P, r)
    C = len(P)
    state = np.zeros(C, np.int8)                      # 0 undecided, 1 accepted, 2 rejected
    rounds = 0
    for _ in range(C):
        rounds += 1
        und = state == 0
        hit = np.bincount(I[state[J] == 1], minlength=C) > 0
        wait = np.bincount(I[state[J] == 0], minlength=C) > 0
        state = np.where(und & hit, 2, np.where(und & ~hit & ~wait, 1, state)).astype(np.int8)
        if not (state == 0).any():
            break
    keep = state == 1
    return keep, int(keep.sum()), rounds


def start_radius(P):
    """The bisection's first ``hi``: the diagonal of the bounding box, f32."""
    P = np.ascontiguousarray(P, F32)
    e = P.max(0) - P.min(0)
    return F32(np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]))


def subsample(P, n, steps=20, selector=select):
    """(idx int32 [n], r f32, count, keep bool [C])."""
    P = np.ascontiguousarray(P, F32)
    assert 1 <= n <= len(P)
    lo, hi = F32(0), start_radius(P)
    for _ in range(steps):
        mid = F32(F32(0.5) * F32(lo + hi))
        if selector(P, mid)[1] >= n:
            lo = mid
        else:
            hi = mid
    keep, count = selector(P, lo)[:2]
    return np.flatnonzero(keep)[:n].astype(np.int32), F32(lo), count, keep


def nn_cv(P):
    """Coefficient of variation of the nearest-neighbour distances of a cloud (f64)."""
    P = np.asarray(P, np.float64)
    d = np.sqrt(((P[:, None, :] - P[None, :, :]) ** 2).sum(-1))
    np.fill_diagonal(d, np.inf)
    nn = d.min(1)
    return float(nn.std() / nn.mean())
