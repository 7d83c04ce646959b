"""The definition of the Sinkhorn figures of sapcu_amd/sinkhorn.py, in numpy (include/sapcu_sinkhorn.h).

Everything takes a working precision ``wp`` (np.float64: the definition; np.longdouble: the "truth" of
tests/golden/sinkhorn_cases.npz, rounded to f64 at the end).  The inputs are f64 clouds, and so is the squared distance: s_ij is
part of the definition in f64, ((x-y)_x^2 + (x-y)_y^2) + (x-y)_z^2 in separately rounded operations; what follows it runs in ``wp``.

Also here: the case table both the generator (tests/golden/make_sinkhorn_cases.py) and the tests build their inputs from, with
numpy PCG64 from (name, seed); nothing but the results is stored.
"""
import zlib

import numpy as np

F64 = np.float64


# ------------------------------------------------------------------------------------------------------ the definition
def sqdist(x, y):
    """s [n,m] in f64, three separately rounded products and two sums in this order."""
    x, y = np.asarray(x, dtype=F64), np.asarray(y, dtype=F64)
    dx = x[:, None, 0] - y[None, :, 0]
    dy = x[:, None, 1] - y[None, :, 1]
    dz = x[:, None, 2] - y[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def cost(x, y, p, wp=F64):
    s = sqdist(x, y)
    assert p in (1, 2)
    return s.astype(wp) * wp(0.5) if p == 2 else np.sqrt(s.astype(wp))


def softmin_c(C, pot, eps, wp=F64):
    """softmin_eps over the columns of C [n,m] with the column potential ``pot`` [m] and uniform weights 1/m."""
    eps = wp(eps)
    m = C.shape[1]
    h = np.log(wp(1.0) / wp(m)) + np.asarray(pot, dtype=wp) / eps
    arg = h[None, :] - C / eps
    mx = arg.max(axis=1)
    return -eps * (mx + np.log(np.exp(arg - mx[:, None]).sum(axis=1)))


def softmin(x, y, pot_y, p, eps, wp=F64):
    return softmin_c(cost(x, y, p, wp), pot_y, eps, wp)


def diameter(x, y=None):
    """The diagonal of the common bounding box, f64."""
    both = np.asarray(x, dtype=F64) if y is None else np.concatenate([np.asarray(x, dtype=F64), np.asarray(y, dtype=F64)])
    e = both.max(axis=0) - both.min(axis=0)
    return float(np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]))


def eps_list(p, blur, iters, scaling=None, diam=None):
    """Every eps of the run in order, Python floats: the pre-schedule eps_k = max(D^p s^(p k), blur^p) up to, not including, the
    first that equals blur^p, then ``iters`` times blur^p."""
    final = float(blur) ** p
    out = []
    if scaling is not None:
        k = 0
        while True:
            e = max(float(diam) ** p * float(scaling) ** (p * k), final)
            if e == final:
                break
            out.append(e)
            k += 1
    return out + [final] * iters


def potentials(x, y, p, eps_seq, wp=F64):
    """(f, g) after one alternating iteration per entry of ``eps_seq``, from f = g = 0: f from g, then g from the new f."""
    C = cost(x, y, p, wp)
    Ct = np.ascontiguousarray(C.T)
    f, g = np.zeros(C.shape[0], dtype=wp), np.zeros(C.shape[1], dtype=wp)
    for e in eps_seq:
        f = softmin_c(C, g, e, wp)
        g = softmin_c(Ct, f, e, wp)
    return f, g


def symmetric_potential(x, p, eps_seq, wp=F64):
    """f of OT(a, a): f <- (f + softmin(f)) / 2 per entry of ``eps_seq``, from 0."""
    C = cost(x, x, p, wp)
    f = np.zeros(C.shape[0], dtype=wp)
    for e in eps_seq:
        f = wp(0.5) * (f + softmin_c(C, f, e, wp))
    return f


def plan_rows(x, y, f, g, p, eps, wp=F64):
    """(r, c): r_i = sum_j P_ij, c_i = sum_j P_ij C_ij for P_ij = a_i b_j exp((f_i + g_j - C_ij) / eps)."""
    C = cost(x, y, p, wp)
    n, m = C.shape
    f, g = np.asarray(f, dtype=wp), np.asarray(g, dtype=wp)
    P = (wp(1.0) / wp(n)) * (wp(1.0) / wp(m)) * np.exp(((f[:, None] + g[None, :]) - C) / wp(eps))
    return P.sum(axis=1), (P * C).sum(axis=1)


def figures(x, y, f, g, p, eps, wp=F64):
    """ot, primal_cost, marginal_error and the row vectors, all in ``wp``."""
    n = len(f)
    r, c = plan_rows(x, y, f, g, p, eps, wp)
    f, g = np.asarray(f, dtype=wp), np.asarray(g, dtype=wp)
    return {"ot": f.sum() / wp(n) + g.sum() / wp(len(g)), "primal_cost": c.sum(), "marginal_error": np.abs(r - wp(1.0) / wp(n)).sum(),
            "r": r, "c": c}


def run_case(case, wp=F64):
    """Everything the golden file stores for one case, in ``wp``: f, g, r, c, ot, primal_cost, marginal_error."""
    x, y = case_inputs(case)
    seq = eps_list(case["p"], case["blur"], case["iters"], case.get("scaling"), diameter(x, y))
    f, g = potentials(x, y, case["p"], seq, wp)
    out = figures(x, y, f, g, case["p"], float(case["blur"]) ** case["p"], wp)
    out.update(f=f, g=g)
    return out


def exact_emd(x, y, p):
    """The optimum of the transport problem with uniform weights, f64: an assignment for n = m, a linear program otherwise."""
    from scipy.optimize import linear_sum_assignment, linprog
    C = cost(x, y, p)
    n, m = C.shape
    if n == m:
        i, j = linear_sum_assignment(C)
        return float(C[i, j].sum() / n)
    A = np.zeros((n + m, n * m))
    for i in range(n):
        A[i, i * m:(i + 1) * m] = 1.0
    for j in range(m):
        A[n + j, j::m] = 1.0
    b = np.concatenate([np.full(n, 1.0 / n), np.full(m, 1.0 / m)])
    res = linprog(C.reshape(-1), A_eq=A[:-1], b_eq=b[:-1], bounds=(0, None), method="highs")       # (one marginal is redundant)
    assert res.status == 0, res.message
    return float(res.fun)


# ------------------------------------------------------------------------------------------------------ the cases
def ulp(v):
    return float(np.spacing(np.float64(abs(v))))


def case_inputs(case):
    """(x [n,3], y [m,3]) f64 of a case, from numpy PCG64 seeded by the case."""
    rng = np.random.Generator(np.random.PCG64(case["seed"]))
    n, m, kind = case["n"], case["m"], case["kind"]
    x, y = rng.uniform(size=(n, 3)), rng.uniform(size=(m, 3))
    if kind == "shift":                          # unit-cube clouds, the second shifted by 0.05
        y = y + 0.05
    elif kind == "same":                         # x = y: s_ii = 0
        assert n == m
        y = x.copy()
    elif kind == "dup":                          # every point several times over, in both clouds, and shared between them
        x[n // 2:] = x[:n - n // 2]
        y[:m // 3] = x[:m // 3] if m // 3 <= n else y[:m // 3]
        y[m // 2:] = y[:m - m // 2]
    elif kind == "far":                          # two clouds 50 apart
        y[:, 0] += 50.0
    elif kind == "offset":                       # coordinates near 1e3
        x, y = x + 1000.0, y + 1000.0 + 0.05
    else:
        assert kind == "cube"
    return np.ascontiguousarray(x), np.ascontiguousarray(y)


def _case(name, n, m, p, blur, iters, kind="shift", scaling=None, family="", sandwich=False):
    return {"name": name, "n": n, "m": m, "p": p, "blur": blur, "iters": iters, "kind": kind, "scaling": scaling, "family": family,
            "sandwich": sandwich}


def boundary_columns(split_plan, rows):
    """The column counts around the tile and around every count at which the number of chunks changes, for ``rows`` rows, up to
    320 columns.  ``split_plan(rows, cols)`` -> (tile, shortest chunk, chunks, columns per chunk): sapcu_amd.sinkhorn.split_plan."""
    tile = split_plan(rows, 1)[0]
    edges = {tile}
    for m in range(2, 321):
        if split_plan(rows, m)[2] != split_plan(rows, m - 1)[2]:
            edges.add(m - 1)                     # the last count with the smaller number of chunks
    cols = sorted({c for e in edges for c in (e - 1, e, e + 1) if 1 <= c <= 320})
    return cols, sorted(edges)


def build_cases(split_plan):
    """The case table.  Sandwich cases: the settings of the issue's table (eps = blur ** p), unit-cube clouds, the second shifted
    by 0.05."""
    cases = [
        _case("sandwich-p1-e05-96", 96, 96, 1, 0.05, 200, family="sandwich", sandwich=True),
        _case("sandwich-p1-e02-96", 96, 96, 1, 0.02, 600, family="sandwich", sandwich=True),
        _case("sandwich-p2-e01-96", 96, 96, 2, 0.1, 600, family="sandwich", sandwich=True),
        _case("sandwich-p1-e05-64x160", 64, 160, 1, 0.05, 300, family="sandwich", sandwich=True),
    ]
    for p in (1, 2):
        for n, m in ((1, 1), (1, 300), (300, 1)):
            cases.append(_case("tiny-%dx%d-p%d" % (n, m, p), n, m, p, 0.05, 20, family="tiny"))
        for n in (63, 64, 65):
            cases.append(_case("wave-%d-p%d" % (n, p), n, 70, p, 0.05, 30, family="wave"))
    cols, _ = boundary_columns(split_plan, 100)
    for k, m in enumerate(cols):
        cases.append(_case("cols-%d" % m, 100, m, 1 + k % 2, 0.05, 20, family="boundary"))
    cases += [
        _case("same-p1", 150, 150, 1, 0.05, 40, kind="same", family="duplicates"),
        _case("same-p2", 150, 150, 2, 0.05, 40, kind="same", family="duplicates"),
        _case("dup-p1", 130, 200, 1, 0.05, 40, kind="dup", family="duplicates"),
        _case("far-p1", 120, 140, 1, 0.01, 30, kind="far", family="separated"),
        _case("far-p2", 120, 140, 2, 0.01, 30, kind="far", family="separated"),
        _case("offset-p1", 160, 129, 1, 0.05, 40, kind="offset", family="offset"),
        _case("offset-p2", 160, 129, 2, 0.05, 40, kind="offset", family="offset"),
        _case("blur10-p1", 200, 180, 1, 10.0, 30, family="large-blur"),
        _case("blur10-p2", 200, 180, 2, 10.0, 30, family="large-blur"),
        _case("scaled-p1", 192, 257, 1, 0.05, 30, scaling=0.5, family="scaled"),
        _case("scaled-p2", 192, 257, 2, 0.05, 30, scaling=0.5, family="scaled"),
    ]
    for c in cases:
        c["seed"] = zlib.crc32(c["name"].encode())
    assert len({c["name"] for c in cases}) == len(cases)
    return cases


QUANTITIES = ("pot", "ot", "primal_cost", "r", "c")


def errors(got, truth):
    """max |got - truth| per quantity of QUANTITIES (pot: over f and g), f64; ``truth`` in f64 or wider."""
    wide = lambda v: np.asarray(v, dtype=np.longdouble)
    d = lambda k: float(np.max(np.abs(wide(got[k]) - wide(truth[k]))))
    return {"pot": max(d("f"), d("g")), "ot": d("ot"), "primal_cost": d("primal_cost"), "r": d("r"), "c": d("c")}


def credited_errors(err):
    """The err_np of the accuracy bar per quantity of QUANTITIES, from a case's stored ``err``: numpy's own error on the quantity,
    and for the two scalar figures at least its error on one term of the sum they are (the potentials for ``ot``, c for
    ``primal_cost``): an error that cancels by chance in numpy's sum is not an accuracy the definition has."""
    e = dict(zip(QUANTITIES, (float(v) for v in err)))
    e["ot"] = max(e["ot"], e["pot"])
    e["primal_cost"] = max(e["primal_cost"], e["c"])
    return [e[q] for q in QUANTITIES]
