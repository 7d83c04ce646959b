"""The (launcher, epilogue) table, the shapes and the operand families of the GEMM epilogue sweep (tests/test_gemm_cases_host.py
checks their conditions without a GPU, tests/test_gpu_gemm_epilogues.py runs them through tests/micro/gemm_probe.hip).

Two operand families make `==` the comparison.  With s = w_scale(k), a power of two:

  family I   A = m_a, W = m_w s, with integers m in [-2, 2]: every product and every partial sum is a small multiple of s, exact in
             f32 in any order, so all five launchers must produce the integer product itself.
  family S   x = m + j 2^-12 with j in {-1, 0, 1} (j = 0 where m = 0); A = x_a, W = x_w s.  f16 rounding gives hi = m and
             lo = j 2^-12 exactly — for A, and scaled by 16 s for the pre-scaled weights — so the value the split-f16 kernels
             DEFINE, hi hi + hi lo + lo hi (the lo lo term is never formed), is a sum of multiples of 16 s 2^-12 whose absolute
             values add up to less than 2^24 quanta: exact in f32 in any order.  It differs from the true product wherever a
             lo lo term is missing, so a kernel that fed one pass from the wrong plane or the wrong row would not pass for noise.

Bias and residual are integers / 4.  s keeps the pre-activations within a few units, where the neurons, GELU and the leaky slope are
not saturated (a saturated neuron would hide a wrong accumulator).  Everything is sliced out of one A_max / W_max per (family, k),
so an output depends on its (row, column, k) only and each reference is computed once."""
import collections
import functools

import numpy as np

EPI = {"BIAS": 0, "LIF": 1, "GELU": 2, "RESID": 3, "LRELU": 4, "RESID_GELU": 5, "LIF_ATTN": 6, "LRELU_MAX": 7, "LIF_MAX": 8}   # common.h GemmEpi
LAUNCHERS = ("f32", "sf16", "ring", "bt", "shortk")      # the shim's launcher numbers: launch_gemm, _sf16, _sf16_ring, _sf16_bt, _shortk
A_SPLIT = ("ring", "bt")                                  # these read A as split rows
SOURCES = {"f32": "gemm_f32.hip", "sf16": "gemm_sf16.hip", "ring": "gemm_sf16_ring.hip", "bt": "gemm_sf16_bt.hip", "shortk": "gemm_shortk.hip"}

# ---------------------------------------------------------------------------------------------- the pair table
TABLE = [
    ("f32", "BIAS"), ("f32", "LIF"), ("f32", "GELU"), ("f32", "RESID"), ("f32", "LRELU"), ("f32", "RESID_GELU"), ("f32", "LIF_ATTN"),
    ("sf16", "BIAS"), ("sf16", "LIF"), ("sf16", "GELU"), ("sf16", "RESID"), ("sf16", "LRELU"), ("sf16", "RESID_GELU"), ("sf16", "LIF_ATTN"),
    ("sf16", "LRELU_MAX"), ("sf16", "LIF_MAX"),
    ("ring", "BIAS"), ("ring", "LIF"), ("ring", "GELU"), ("ring", "RESID"), ("ring", "LRELU"), ("ring", "RESID_GELU"), ("ring", "LIF_ATTN"),
    ("bt", "BIAS"), ("bt", "LIF"), ("bt", "LIF_ATTN"), ("bt", "LRELU_MAX"),
    ("shortk", "LIF"), ("shortk", "LIF_MAX"),
]
REFUSED = [(l, e) for l in LAUNCHERS for e in EPI if (l, e) not in TABLE]

NEURON = ("LIF", "LIF_ATTN", "LIF_MAX")
GELU = ("GELU", "RESID_GELU")
RESID = ("RESID", "RESID_GELU")
MAXES = ("LRELU_MAX", "LIF_MAX")
EXACT = ("BIAS", "RESID", "LRELU", "LRELU_MAX")           # at most one f32 rounding of an exact value: compared on bits

# ---------------------------------------------------------------------------------------------- shapes
ROWS = (1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 255, 256, 257)
ROWS_BT = (1024, 1025, 1027, 1028, 1055, 1056, 1057, 1151, 1152, 1153, 1279, 1280, 1281)     # gemm_sf16_bt_ok starts at 4 * 256 rows
ROWS_SHORTK_MAX = (48, 96, 144, 1008)                     # the register max takes whole patches of 48 rows
COLS = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 132, 255, 256, 260)
COLS_BT = (128, 256, 384)
KS = {"f32": (32, 64, 96, 256, 288, 320), "ring": (32, 64, 96, 256, 288, 320), "bt": (32, 64, 96, 128), "sf16": (64, 128, 192),
      "shortk": (64, 128, 192)}
K0 = 64                                                   # the depth of the row and column sweeps: every launcher takes it
ALL_KS = tuple(sorted({k for ks in KS.values() for k in ks}))
R_MAX, N_MAX = 1281, 384
MAX_MS = (1, 3, 5, 48, 100, 128, 130)
MAX_M0 = 5                                                # the group size of the max epilogues on the shape sweeps
LIF_TS = (1, 4)
ATTN_M, ATTN_KK = 5, 3                                    # edge rows: kk neighbours per point, m points per patch
Q_ROWS = ((R_MAX - 1) // ATTN_KK // ATTN_M + 1) * ATTN_M  # point rows the edge table of R_MAX edge rows can name

Shape = collections.namedtuple("Shape", "r n k max_m")


def _max_rows(base, max_m):
    """A row count >= base that max_m divides, and (max_m > 1) one it does not."""
    r = -(-base // max_m) * max_m
    return (r,) if max_m == 1 else (r, r + 1)


def star(launcher, epi):
    """The shapes of one pair: the row sweep at two widths, the column sweep, the K sweep; for a max epilogue the group sizes too."""
    shortk_max = (launcher, epi) == ("shortk", "LIF_MAX")
    bt = launcher == "bt"
    mm = 48 if shortk_max else (MAX_M0 if epi in MAXES else 0)
    rows = ROWS_SHORTK_MAX if shortk_max else ROWS_BT if bt else ROWS
    widths = (128, 384) if bt else (132, 131)             # 132: the ring's float4 consumers, 131: its element-wise ones
    r0 = 144 if shortk_max else 1153 if bt else 129
    n0 = 128 if bt else 132
    out = [Shape(r, n, K0, mm) for r in rows for n in widths]
    out += [Shape(r0, n, K0, mm) for n in (COLS_BT if bt else COLS)]
    out += [Shape(r0, n0, k, mm) for k in KS[launcher]]
    if epi in MAXES and not shortk_max:
        out += [Shape(r, n0, K0, m) for m in MAX_MS for r in _max_rows(1025 if bt else 129, m)]
    return out


Layout = collections.namedtuple("Layout", "name lda ldc ldr misalign c_split c2_split")


def layouts(launcher, epi, s):
    """Compact, then every pitched form the launcher takes.  lda = k + 32 is the interleaved split-row format, k + 8 the two-plane
    one; `misalign` moves bias, neuron parameters, residual and kf by one float (the ring's element-wise consumers); the big tile
    declines what is not 16-byte aligned, so it keeps them aligned and its ldc a multiple of 4."""
    bt = launcher == "bt"
    n32 = -(-s.n // 32) * 32
    out = [Layout("compact", s.k, s.n, s.n, 0, 0, 0),
           Layout("pitched", s.k + 32, s.n + 4, s.n + 8, 0, 0, 0),
           Layout("odd", s.k + 8, s.n + 4 if bt else s.n + 1, s.n + 3, 0 if bt else 1, 0, 0)]
    if epi not in MAXES:                                  # a max epilogue stores no C
        attn = epi == "LIF_ATTN"
        out += [Layout("split32", s.k, n32, s.n, 0, 0 if attn else 1, 1 if attn else 0),      # attention: pe stays f32, attn_in leaves split
                Layout("split", s.k + 8, s.n + 4, s.n + 8, 0, 1, 1 if attn else 0)]
    return out


def families(launcher):
    return ("I",) if launcher == "f32" else ("I", "S")    # the exact-f32 kernel computes the true product: family I only


def steps(epi):
    return LIF_TS if epi in NEURON else (0,)


def accepts(launcher, epi, s):
    """What the launcher's own predicate says of a compact call of this shape (the sweep asserts the predicate agrees)."""
    if (launcher, epi) not in TABLE or s.k % 32 or (launcher in ("sf16", "shortk") and s.k % 64):
        return False
    if launcher == "bt":
        return s.r >= 1024 and s.n % 128 == 0
    if launcher == "shortk":
        return s.k <= 192 and (epi == "LIF" or (s.max_m == 48 and s.r % 48 == 0))
    return True


def partner(launcher, epi, family, s):
    """The other launcher that runs the same case for the bit-for-bit comparison across launchers, or None."""
    for other in ("sf16", "ring", "f32", "shortk"):
        if other != launcher and (family == "I" or other != "f32") and accepts(other, epi, s):
            return other
    return None


def expected_runs(launcher, epi):
    """(launches of the pair itself, launches of its partners) on the sweep, from the tables alone."""
    own = sum(len(layouts(launcher, epi, s)) for s in star(launcher, epi)) * len(families(launcher)) * len(steps(epi))
    others = sum(partner(launcher, epi, f, s) is not None for s in star(launcher, epi) for f in families(launcher)) * len(steps(epi))
    return own, others


# ---------------------------------------------------------------------------------------------- operands
def w_scale(k):
    return 2.0 ** -int(np.floor(np.log2(np.sqrt(k))))


def split16(x):
    """(hi, lo) as the kernels split an f32: hi = f16_rn(x), lo = f16_rn(x - hi), numpy's own rounding."""
    x = np.asarray(x, np.float32)
    hi = x.astype(np.float16)
    return hi, (x - hi.astype(np.float32)).astype(np.float16)


@functools.lru_cache(maxsize=None)
def operands(family, k):
    """A [R_MAX, k] and W [N_MAX, k] in f32, and `acc` [R_MAX, N_MAX] in f64: the value the kernels define for A . W^T (the
    three-term sum of the split operands, weights pre-scaled by 16, then / 16); read-only."""
    rng = np.random.default_rng([k, {"I": 1, "S": 2}[family]])

    def draw(rows):
        m = rng.integers(-2, 3, size=(rows, k)).astype(np.float64)
        if family == "I":
            return m
        j = rng.integers(-1, 2, size=(rows, k)).astype(np.float64)
        return m + np.where(m == 0, 0.0, j) * 2.0 ** -12

    a = draw(R_MAX).astype(np.float32)
    w = (draw(N_MAX) * w_scale(k)).astype(np.float32)
    ah, al = (p.astype(np.float64) for p in split16(a))
    wh, wl = (p.astype(np.float64) for p in split16(w * np.float32(16.0)))
    acc = (ah @ wh.T + ah @ wl.T + al @ wh.T) / 16.0
    for arr in (a, w, acc):
        arr.setflags(write=False)
    return a, w, acc


@functools.lru_cache(maxsize=None)
def columns():
    """bias [N_MAX] and residual [R_MAX, N_MAX] (integers / 4), raw neuron parameters [4, N_MAX] drawn as
    test_ring_gemm_neuron_epilogue_and_split_row_output draws them, integer q | kf rows [Q_ROWS, 2 N_MAX + 4] and the in-patch
    neighbour index of every edge row."""
    rng = np.random.default_rng(29)
    bias = (rng.integers(-8, 9, size=N_MAX) / 4.0).astype(np.float32)
    resid = (rng.integers(-8, 9, size=(R_MAX, N_MAX)) / 4.0).astype(np.float32)
    raw = np.stack([rng.uniform(0.05, 1.1, N_MAX), rng.uniform(0.0, 0.2, N_MAX), rng.uniform(0.05, 1.0, N_MAX),
                    rng.normal(0.5, 0.3, N_MAX)]).astype(np.float32)
    qk = rng.integers(-4, 5, size=(Q_ROWS, 2 * N_MAX + 4)).astype(np.float32)
    idx = rng.integers(0, ATTN_M, size=R_MAX).astype(np.int32)
    for arr in (bias, resid, raw, qk, idx):
        arr.setflags(write=False)
    return bias, resid, raw, qk, idx


def edge_rows():
    """(point row, neighbour row) of every edge row: what launch_edge_table writes for `idx`."""
    idx = columns()[4]
    pt = np.arange(R_MAX) // ATTN_KK
    return np.stack([pt, (pt // ATTN_M) * ATTN_M + idx], 1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def argument(family, k, resid):
    """f64 [R_MAX, N_MAX]: what enters the activation — acc + bias (+ residual), exact."""
    bias, res = columns()[:2]
    x = operands(family, k)[2] + bias.astype(np.float64)
    return x + res if resid else x


def lrelu(x32):
    return np.where(x32 >= 0, x32, np.float32(0.2) * x32).astype(np.float32)


def gelu64(x):
    from scipy.special import erf
    return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))


def group_max(v, max_m):
    """[ceil(r / max_m), n]: the maximum over each group of max_m rows (the last one may be short)."""
    r = v.shape[0]
    return np.stack([v[g:g + max_m].max(0) for g in range(0, r, max_m)])
