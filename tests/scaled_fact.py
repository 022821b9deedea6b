"""Power-of-two scaling as an exact symmetry of the Cholesky family and of Householder QR (TESTS ONLY): the case
tables and builders that tests/test_scaled_fact_host.py (CPU: the numpy models and LAPACK alone satisfy every relation)
and tests/test_gpu_scaled_fact.py (the library on the MI355X) share.  The sibling of tests/scaled.py, which does the
same for LU, the solves and the row reductions; nothing ran Cholesky or QR away from unit scale before.

Multiplying by a power of two commutes with every IEEE rounding -- of a product, a sum, a quotient, and of a square
root when the power is even -- while no intermediate leaves the normal range.  D = diag(2^d), d an integer vector
("uniform": every d_i = s).

Cholesky, A' = D A D (upper storage):
  potrf   info unchanged, U' == U D;                      potrs, B' = 2^t D B:  X' == 2^t D^-1 X;
  potri   inv' == D^-1 inv D^-1;                          podet  same sign and mantissa, exp2' = exp2 + 2 sum(d);
  uniform only:  norm_sym' = 4^s norm_sym;  pocon: the same rcond and as many solves;  porfs (A' = 4^s A, U' = 2^s U,
  B' = 2^(t+s) B, start 2^(t-s) X0): X' == 2^(t-s) X, ferr, berr, steps and solves unchanged;
  not positive definite (a zero or a negative pivot): the same info, the rows before the failing pivot scaled alike.
QR, A' = 2^r A D (one row factor, column exponents d):
  geqrf   tau and everything below the diagonal unchanged, R' == 2^r R D;       orgqr unchanged;
  ormqr of 2^t C: 2^t times the result;
  gels, B' = 2^t B:  X'[i] == X[i] 2^(t - r - d_i), the tail rows of Q^T B and col_norms times 2^t, info unchanged;
  a zero column (cpu_qr.planted_zero_column): the same info = j + 1.

What it is there to catch: a Gram sum, alpha^2 + g or colnrm2 formed in fp32 (kernels_qr.hip promises fp64 for both
precisions, and no dlarfg rescaling: at 2^-80 and 2^+70 the square of an fp32 entry leaves the fp32 range, not the fp64
one); a threshold written as a constant; a product formed in an order that overflows (tau v w as (tau w) v) -- all of
which hide at unit scale.

The exponent tables.  Each is derived from the largest and the smallest intermediate the routine forms, and
tests/test_scaled_fact_host.py proves case by case that the reference arithmetic stays inside the relation (and that
inputs and results are normal numbers or zero):
  CHOL_EXP (potrf, potrs, podet, not positive definite).  The entries of A' carry 2^(d_i + d_j): a uniform s puts them
    at 4^s.  The largest intermediate is a'_ij itself (planted: integers below 2^22); the smallest are the products
    u_ki u_kj of the trailing update and the terms of inv(U11)^T A12, of size 4^s u^2 and, in a rounded matrix, whatever
    cancellation leaves of them: fp32 4^-45 = 2^-90 leaves 36 binades above the smallest normal number, fp64 4^-450
    leaves 122.  Mixed d draws from a narrower range because a'_ij spans 2^(2 lo) .. 2^(2 hi) in one matrix and the block
    inverse holds 2^(-d_i) beside it (the models were seen to pass on [-25, 25] and [-200, 200]).
  CHOL_INV_EXP (potri, pocon, porfs; lansy with them).  They form inv(A), of scale 4^-s where A has 4^s, and their
    product: both ends of the range are in use at once, so the table is half as wide -- as SOLVE_EXP is for LU.  porfs
    also carries LAPACK's guard: a row of |b| + |A| |x| at or below safe2 = (n + 1) safmin / u (2^-94 in fp32 at
    n = 300) is treated differently, which is a threshold by design; 2^(t + s) times the row sums stays far above it.
  QR_EXP (geqrf, ormqr, orgqr, gels, colnrm2).  The stored entries carry 2^(r + d_c); the Gram sums carry
    2^(2 r + d_j + d_c) and are fp64 for both precisions, so what limits the table is the STORED entries: after the
    cancellation of a rounded input (down to 2^-24 of the column in fp32) they must stay normal.  fp32 uniform -80 and
    +70 (entries near 2^-77 and 2^+73, squares 2^-154 and 2^+146: outside fp32, inside fp64 -- at -75 the squares of
    the planted integers are still exact as fp32 SUBNORMAL numbers, and an fp32 Gram sum of them goes unnoticed); fp64
    uniform -400 and +400 (squares 2^-800 and 2^+800).  Mixed: [-50, 50] and [-400, 400].  The solve with R forms
    inv(R) 2^-r D^-1 times Q^T B 2^t: the result carries 2^(t - r - d_i), inside the range for T_RHS and R_ROWS below.
"""
import functools

import numpy as np

import cpu_chol as cc
import cpu_posx as cp
import cpu_qr as cq
import scaled as sc

DTYPES = sc.DTYPES
name = sc.name
SEED = 11

CHOL_ORDERS = (129, 300)            # a ragged second block; three blocks and the MFMA update
CHOL_NRHS = (1, 17)                 # the few-column path and the block sweeps
CHOL_EXP = {"float32": dict(down=-45, up=45, mixed=(-25, 25), alt=20),
            "float64": dict(down=-450, up=450, mixed=(-200, 200), alt=150)}
CHOL_KINDS = ("down", "up", "mixed", "alternating")
CHOL_INV_EXP = {"float32": dict(down=-20, up=20, mixed=(-12, 12)),
                "float64": dict(down=-225, up=225, mixed=(-100, 100))}
CHOL_INV_KINDS = ("down", "up", "mixed")
UNIFORM_KINDS = ("down", "up")
NOT_PD = ((129, 128, "zero"), (300, 5, "negative"), (300, 200, "zero"), (300, 257, "negative"))   # n, row, kind

QR_SHAPE = (300, 200)               # two panels, a ragged second one, more than one row slab
QR_HADAMARD = (4, 129)              # 385 x 129: dense reflectors
QR_NRHS = 7
QR_EXP = {"float32": dict(down=-80, up=70, mixed=(-50, 50), alt=40),
          "float64": dict(down=-400, up=400, mixed=(-400, 400), alt=300)}
QR_KINDS = ("down", "up", "mixed", "alternating")
R_ROWS = 3                          # r of A' = 2^r A D
T_RHS = 13                          # t of B' = 2^t B and of ormqr's 2^t C
QR_ZERO_COLUMNS = (5, 128)          # in the 300 x 200 plant


def exponents(table, dtype, kind, n):
    """d of a case: "down" / "up" uniform, "mixed" per-index integers uniform in the table's mixed range,
    "alternating" +-alt by index, "unit" zeros."""
    e = table[name(dtype)]
    if kind == "unit":
        return np.zeros(n, dtype=np.int64)
    if kind in ("down", "up"):
        return np.full(n, e[kind], dtype=np.int64)
    if kind == "mixed":
        lo, hi = e["mixed"]
        return np.random.default_rng([SEED, int(n), 7]).integers(lo, hi + 1, n).astype(np.int64)
    if kind == "alternating":
        return np.where(np.arange(n) % 2 == 0, e["alt"], -e["alt"]).astype(np.int64)
    raise ValueError(kind)


def is_uniform(d):
    return int(np.min(d)) == int(np.max(d))


def rhs_exponent(dtype, kind, table):
    """t of B' = 2^t D B for the Cholesky solves: a third of the matrix's exponent the other way (mixed: a small odd
    one)."""
    e = table[name(dtype)]
    return {"down": -e["down"] // 3, "up": -e["up"] // 3, "mixed": 5, "alternating": -3}[kind]


def scale_sym(A, d):
    """D A D, exactly (the callers keep it representable)."""
    d = np.asarray(d, dtype=np.int32)
    return np.ldexp(A, d[:, None] + d[None, :]).astype(A.dtype)


def scale_cols(X, d, extra=0):
    """2^extra X D."""
    return np.ldexp(X, np.asarray(d, dtype=np.int32)[None, :] + int(extra)).astype(X.dtype)


def scale_rows(X, d, extra=0):
    """2^extra D X (X a matrix or a vector)."""
    X = np.asarray(X)
    e = np.asarray(d, dtype=np.int32).reshape((-1,) + (1,) * (X.ndim - 1)) + int(extra)
    return np.ldexp(X, e).astype(X.dtype)


def upper_scaled(R, d, extra=0):
    """The factor array R with its upper triangle times 2^extra D from the right, the strictly lower triangle as it
    is: what potrf (extra = 0) and geqrf (extra = r) must return for the scaled input, bit for bit."""
    out = np.array(R, copy=True)
    n = R.shape[1]
    top = np.triu(np.ones((min(R.shape[0], n), n), dtype=bool))
    out[:top.shape[0]][top] = scale_cols(R[:top.shape[0]], d, extra)[top]
    return out


def normal_or_zero(X, dtype):
    return sc.is_normal_or_zero(np.asarray(X, dtype=np.float64), dtype)


# ------------------------------------------------------------------ Cholesky inputs
def chol_matrix(source, n, dtype):
    """The symmetric matrix of a case: "planted" cpu_chol.planted (U^T U of small integers), "rounded" cpu_chol.spd."""
    return cc.planted(n, dtype=dtype)[1] if source == "planted" else cc.spd(n, 0, dtype)


@functools.lru_cache(maxsize=None)
def _chol_rhs(source, n, nrhs):
    rng = np.random.default_rng([SEED, int(n), int(nrhs), source == "planted"])
    if source == "planted":
        X0 = rng.integers(-3, 4, (n, nrhs)).astype(np.float64)
        return cc.planted(n)[1] @ X0
    return rng.uniform(-1.0, 1.0, (n, nrhs))


def chol_rhs(source, n, nrhs, dtype):
    """planted: B = A X0 for integer X0 in [-3, 3] (exact in fp32); rounded: U(-1, 1)."""
    return _chol_rhs(source, n, nrhs).astype(dtype)


def podet_expected(n, d):
    """sign, mant, exp2 of det(D A D) for the planted A = U^T U: + 2^k, mant 1/2, exp2 = 1 + 2 sum log2 u_kk + 2 sum d."""
    diag = np.diagonal(cc.planted(n)[0])
    log2 = np.log2(diag)
    assert np.array_equal(log2, np.round(log2))
    return 1.0, 0.5, 1 + 2 * int(log2.sum()) + 2 * int(np.sum(d))


def refine_start(X):
    """The start of the porfs cases: the solution times (1 +- 2^-10) by row (cpu_posx.perturbed), so that steps are
    taken."""
    return cp.perturbed(X)


# ------------------------------------------------------------------ QR inputs
def qr_case(source, dtype):
    """(A, B, planted): "planted" cpu_qr.planted at QR_SHAPE with its right-hand sides, "hadamard" the dense-reflector
    plant at QR_HADAMARD, "rounded" cpu_qr.rounded_case at QR_SHAPE with QR_NRHS columns of U(-1, 1).  planted: None,
    or (R as the model returns it at unit scale is exact; x0) for the inputs whose answer is known in advance."""
    if source == "planted":
        m, n = QR_SHAPE
        A = cq.planted(m, n, dtype=dtype)[1]
        x0, B, _ = cq.planted_rhs(m, n, QR_NRHS, dtype=dtype)
        return A, B, x0
    if source == "hadamard":
        q, n = QR_HADAMARD
        A = cq.hadamard_plant(q, n, dtype=dtype)[1]
        x0, B, _ = cq.hadamard_rhs(q, n, QR_NRHS, dtype=dtype)
        return A, B, x0
    m, n = QR_SHAPE
    return cq.rounded_case(m, n, dtype)[0], cq.uniform(m, QR_NRHS, 2, dtype), None


QR_SOURCES = ("planted", "hadamard", "rounded")


def qr_scaled_input(A, d, dtype):
    return scale_cols(A.astype(dtype), d, R_ROWS)


def gels_expected(Bo, n, d):
    """B_out of gels for (2^r A D, 2^t B) from that of (A, B): rows [0, n) times 2^(t - r - d_i), the tail times 2^t."""
    out = np.array(Bo, copy=True)
    out[:n] = scale_rows(Bo[:n], -np.asarray(d), T_RHS - R_ROWS)
    out[n:] = np.ldexp(Bo[n:], T_RHS)
    return out
