"""Power-of-two scaling as an exact symmetry of LU, the solves and the row reductions (TESTS ONLY): the case tables
and builders that tests/test_scaled_host.py (CPU: the reference arithmetic alone satisfies every relation) and
tests/test_gpu_scaled.py (the library on the MI355X) share.

Multiplying by a power of two commutes with every IEEE rounding while no intermediate leaves the normal range.  So
for A' = A diag(2^d), d an integer vector (uniform: d_j = s):

  partial pivoting takes the same rows;  L' == L bit for bit;  U'[:, j] == U[:, j] 2^{d_j} bit for bit;
  det: same sign and mantissa, exp2' = exp2 + sum(d);
  A' X' = B 2^t       ->  X'[i] = X[i] 2^{t - d_i};     A'^T X' = diag(2^d) B  ->  X' == X;
  inverse             ->  rows scaled by 2^{-d_i};       rcond, pivot ratio, last correction: unchanged (uniform);
  norms scale by 2^s (uniform); row reduction of 2^s A with tolerance 2^s tol: same rank and pivots, pivot rows of R
  bit-identical (they are normalised), the rows below the rank -- non-zero right of the bar only -- times 2^s.

On a planted input (tests/planted.py, tests/planted_rref.py) the left-hand sides are also known in advance: every
operation on them is exact, so the scaled planted factors are the exact answer, subnormal pivots included (an entry
is a multiple of 2^{s-2}, which every scale used here keeps representable).
"""
import numpy as np

import planted as pl
import planted_rref as pr

DTYPES = (np.float32, np.float64)
U_ROUND = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}
TINY = {"float32": 2.0 ** -126, "float64": 2.0 ** -1022}      # smallest normal number
SEED = 11                 # planted systems: the seed of tests/test_gpu_planted.py
ORDERS = (64, 129, 300, 641)   # one panel; a 1-column ragged panel; three panels and the MFMA update; the look-ahead driver
LOOKAHEAD_MIN = 128       # option lookahead_min for order 641: five full panels and one column under the look-ahead driver
DRIVERS_300 = tuple((panel, look) for panel in (0, 3, 4) for look in (0, 1))
NRHS = (1, 3, 17)         # the cooperative few-right-hand-side path and the block sweeps

# exponents of the factorisation (A, B): every intermediate of a planted elimination stays normal -- the smallest
# non-zero factor entry is 1/4 at unit scale, 2^-122 = 16 * 2^-126 at -120
FACTOR_EXP = {"float32": dict(down=-120, up=118, alt=100), "float64": dict(down=-1000, up=1010, alt=1000)}
FACTOR_KINDS = ("down", "up", "mixed", "alternating")
# the solves, the inverse and the condition estimate also form inverses of triangular blocks, which grow with the
# inverse scale (C, D)
SOLVE_EXP = {"float32": dict(down=-40, up=40), "float64": dict(down=-500, up=500)}
SOLVE_KINDS = ("down", "up", "mixed")
# U(-1, 1) matrices, one 2^s: the margin is for the entries that cancellation leaves far below the input scale
RANDOM_EXP = {"float32": (-40, 40), "float64": (-800, 800)}
RANDOM_SEED = 5
# F: every pivot (4 or 8 times 2^s) is subnormal, every entry (a multiple of 2^{s-2}) still representable
SUBNORMAL_EXP = {"float32": -130, "float64": -1030}
SUBNORMAL_ORDERS = (64, 300)
SUBNORMAL_PANELS = (0, 3, 4)
# F, second input: 2^base everywhere, column ONE_SUBNORMAL_COLUMN (second panel of order 300) 2^extra further down
ONE_SUBNORMAL = {"float32": (-100, -30), "float64": (-1000, -30)}
ONE_SUBNORMAL_COLUMN = 200
# E: row reductions.  (case id of planted_rref.CASES, why): the smallest rows of the path table that reach the
# per-column kernels, the blocked reduction (largest-magnitude rule) and api.hip rref_first_fast (first-non-zero rule, fp64)
RREF_CASE_IDS = ("percol-40x60-bar45", "blocked-600x160-bar129", "blocked-600x400-pivots-at-bar-1-and-bar")
RREF_SUBNORMAL_CASE_ID = "blocked-600x160-bar129"
RREF_TOL_ORDERS = (40, 300)
RREF_TOL = 0.75
TRACE_SHAPE = (6, 8, 6)   # m, n, bar of the traced reduction
TRACE_EXP = (-1000, 1010)
# G: the planted system of order 300 with row GRADED_ROW of U times 2^-33 = 1.16e-10: pivot ratio about 1e-10, at
# 2^-1010 and 2^+1000
GRADED_N, GRADED_ROW, GRADED_LOG2 = 300, 150, -33
GRADED_EXP = (-1010, 1000)

def name(dtype):
    return np.dtype(dtype).name


def _vector(table, dtype, kind, n):
    e = table[name(dtype)]
    if kind == "unit":
        return np.zeros(n, dtype=np.int64)
    if kind in ("down", "up"):
        return np.full(n, e[kind], dtype=np.int64)
    if kind == "mixed":
        rng = np.random.default_rng([SEED, int(n), 7])
        return rng.integers(e["down"], e["up"] + 1, n).astype(np.int64)
    if kind == "alternating":
        return np.where(np.arange(n) % 2 == 0, e["alt"], -e["alt"]).astype(np.int64)
    raise ValueError(kind)


def factor_exponents(dtype, kind, n):
    """The column exponents d of a factorisation case: "down" / "up" uniform, "mixed" per-column integers uniform in
    [down, up], "alternating" +-alt by column (sum 0 for an even order, alt for an odd one)."""
    return _vector(FACTOR_EXP, dtype, kind, n)


def solve_exponents(dtype, kind, n):
    return _vector(SOLVE_EXP, dtype, kind, n)


def rhs_exponent(dtype, kind):
    """t of A' X = 2^t B: half the scale of the matrix, the other way."""
    e = SOLVE_EXP[name(dtype)]
    return {"down": -e["down"] // 2, "up": -e["up"] // 2, "mixed": e["up"] // 4}[kind]


def one_subnormal_exponents(dtype, n):
    base, extra = ONE_SUBNORMAL[name(dtype)]
    d = np.full(n, base, dtype=np.int64)
    d[ONE_SUBNORMAL_COLUMN] += extra
    return d


def scale_columns(A, d, dtype):
    """A diag(2^d) in `dtype`, exactly (ldexp; the callers keep the result representable)."""
    return np.ldexp(np.asarray(A).astype(dtype), np.asarray(d, dtype=np.int32)[None, :]).astype(dtype)


def scale_rows(X, d, dtype=None):
    """diag(2^d) X, exactly."""
    X = np.asarray(X)
    return np.ldexp(X, np.asarray(d, dtype=np.int32).reshape((-1,) + (1,) * (X.ndim - 1))).astype(dtype or X.dtype)


def scale(X, s, dtype=None):
    X = np.asarray(X)
    return np.ldexp(X, int(s)).astype(dtype or X.dtype)


_PLANTED = {}


def planted(n):
    """A, L, U, perm, ipiv of the planted system of order n (float64; kept)."""
    if n not in _PLANTED:
        A, L, U, perm = pl.planted(n, SEED)
        _PLANTED[n] = (A, L, U, perm, pl.ipiv_of_perm(perm))
    return _PLANTED[n]


def planted_lu_scaled(n, d):
    """The factors of planted(n) diag(2^d): L below the diagonal, U diag(2^d) on and above (float64, exact)."""
    _, L, U, _, _ = planted(n)
    return np.tril(L, -1) + np.ldexp(U, np.asarray(d, dtype=np.int32)[None, :])


def det_expected(n, d):
    """sign, mant, exp2 of det(planted(n) diag(2^d)) = +-2^k: mant = 1/2, exp2 = 1 + sum log2|U_kk| + sum d."""
    _, _, U, perm, _ = planted(n)
    diag = np.diag(U)
    log2 = np.log2(np.abs(diag))
    assert np.array_equal(log2, np.round(log2))
    return pl.perm_sign(perm) * float(np.prod(np.sign(diag))), 0.5, 1 + int(log2.sum()) + int(np.sum(d))


def planted_rhs(n, nrhs, trans=False):
    """X0 (small integers) and B = A X0 (A^T X0), exact in fp32: the right-hand sides of tests/test_gpu_planted.py."""
    A = planted(n)[0]
    rng = np.random.default_rng([SEED, int(n), int(nrhs), int(trans)])
    X0 = rng.integers(-3, 4, (n, nrhs)).astype(np.float64)
    X0[0, :] = 3.0
    B = (A.T if trans else A) @ X0
    assert np.array_equal(B.astype(np.float32).astype(np.float64), B)
    return X0, B


def random_matrix(n, dtype, seed=RANDOM_SEED):
    """U(-1, 1) rounded to `dtype`."""
    return np.random.default_rng([int(seed), int(n)]).uniform(-1.0, 1.0, (n, n)).astype(dtype)


def random_rhs(n, nrhs, dtype, seed=RANDOM_SEED):
    return np.random.default_rng([int(seed), int(n), int(nrhs)]).uniform(-1.0, 1.0, (n, nrhs)).astype(dtype)


def is_normal_or_zero(X, dtype):
    """Every entry of X (float64 values) is zero or a normal number of `dtype`."""
    a = np.abs(np.asarray(X, dtype=np.float64))
    return bool(np.all((a == 0) | ((a >= TINY[name(dtype)]) & (a <= float(np.finfo(dtype).max)))))


# ------------------------------------------------------------------------------------------------ E: row reductions
def rref_exponents(dtype):
    e = FACTOR_EXP[name(dtype)]
    return (e["down"], e["up"])


def rref_cases():
    return [pr.case_by_id(cid) for cid in RREF_CASE_IDS]


def rref_expected(R_unit, rank, s):
    """The reduction of 2^s A from that of A: the pivot rows are normalised and do not change, the rows from the rank
    on (non-zero right of the bar only) are multiplied by 2^s."""
    want = np.array(R_unit, copy=True)
    want[rank:] = np.ldexp(want[rank:], int(s))
    return want


def trace_matrix():
    """6 x 8 of small integers and quarters, bar 6: the traced reduction (the reference's operation order)."""
    m, n, _ = TRACE_SHAPE
    rng = np.random.default_rng([SEED, m, n])
    return rng.integers(-12, 13, (m, n)).astype(np.float64) / 4.0


# ------------------------------------------------------------------------------------------------ G: Matrix surface
def graded_system():
    """A, B, X0 with A X0 = B: the planted system of order 300 with row GRADED_ROW of its U factor multiplied by 2^-33
    before the product is formed.  The smallest pivot is then about 1e-10 of the largest entry; every entry is a
    multiple of 2^-35, so every elimination step is still exact in fp64, and so is B = A X0 for the small integers X0,
    at unit scale and at every scale of GRADED_EXP (a multiple of 2^-1045 is representable)."""
    _, L, U, perm, _ = planted(GRADED_N)
    U = U.copy()
    U[GRADED_ROW] = np.ldexp(U[GRADED_ROW], GRADED_LOG2)
    A = np.empty_like(U)
    A[perm] = L @ U
    X0 = np.random.default_rng([SEED, GRADED_N, 3]).integers(-3, 4, (GRADED_N, 3)).astype(np.float64)
    X0[0, :] = 3.0
    return A, A @ X0, X0


def pivot_ratio(A):
    """min|U_kk| / max|A| of a same-precision elimination."""
    LU, _, info = pl.eliminate(A, A.dtype)
    assert info == 0
    return float(np.abs(np.diag(LU)).min() / np.abs(A).max())
