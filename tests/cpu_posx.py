"""CPU statement of the condition estimate and the error bounds of the Cholesky family (lsx_lansy_*, lsx_pocon_*,
lsx_porfs_*): numpy twins of what the device runs, the inputs of the tests and their yardsticks.  The counterpart of
cpu_cond.py / cpu_refine.py for symmetric positive definite matrices in upper storage.

Every twin reads `np.triu(A)` (or `np.triu(U)`) and nothing else, as the kernels do: the symmetric residual uses every
stored a_ij, j > i, for row i and for row j and a diagonal element once; the norm adds a column of the upper triangle
and the row right of the diagonal; pocon is lacn2 (cpu_refine.lacn2) around x <- inv(U) inv(U^T) x, the operator being
symmetric; one column of porfs is cpu_refine.gerfs_twin with the symmetric residual and solves through cpu_chol.potrs.
The twins do not model the order of summation, so they agree with the GPU to rounding, not bit for bit.
"""
from __future__ import annotations

import functools

import numpy as np

import cpu_chol as cc
import cpu_refine as cr

ORDERS = (1, 2, 33, 127, 128, 129, 257, 300, 600)
TWIN_ORDERS = (1, 2, 33, 129, 300)       # what the host file proves of the twins (the issue's list)
# exponent range s of the scaling D = diag(2^k), k uniform in [-s, s]: the estimate's agreement bound 64 n eps cond_1
# has to stay <= 0.35 (fp32: s = 1 gives 1.2 at n = 300), the refinement runs on both.  In fp32 s = 0 still gives 0.66
# at n = 600 (cond_1 = 144), so the fp32 condition cases add 2 I to the matrix: G G^T / n + 3 I, 0.18 at n = 600.
SCALE_COND = {"f64": 6, "f32": 0}
SHIFT_COND = {"f64": 0.0, "f32": 2.0}
SCALE_REFINE = {"f64": 6, "f32": 1}
DTYPES = {"f64": np.float64, "f32": np.float32}
EPS = {"f64": float(np.finfo(np.float64).eps), "f32": float(np.finfo(np.float32).eps)}
MAXRHS = 11


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def _scaled(n, seed, s, shift):
    S = cc.spd(n, seed) + shift * np.eye(n)
    k = np.random.default_rng(9000 + 31 * n + seed).integers(-s, s + 1, n)
    d = 2.0 ** k
    return S * d[:, None] * d[None, :]      # exact: powers of two


def scaled_spd(n, seed=0, s=0, dtype=np.float64, shift=0.0):
    """D S D with S = cpu_chol.spd(n, seed) + shift I and D = diag(2^k), k uniform in [-s, s]; symmetric, rounded to
    dtype."""
    return _scaled(n, seed, s, float(shift)).astype(dtype)


def rhs(A, nrhs, seed):
    """(B, XT) in the precision of A: B = A XT formed column by column in fp64, so a column has the same bits however
    many are asked for."""
    n = A.shape[0]
    rng = np.random.default_rng(400 + seed)
    XT = rng.uniform(-1, 1, (n, nrhs))
    A64 = A.astype(np.float64)
    B = np.empty((n, nrhs))
    for j in range(nrhs):
        B[:, j] = A64 @ XT[:, j]
    return B.astype(A.dtype), XT.astype(A.dtype)


def perturbed(X):
    """X times (1 +- 2^-10), alternating by row: the start of the refinement tests.  A Cholesky solve of these
    matrices already has a backward error of 1.5 - 2 u, which a refinement step does not reliably lower."""
    f = np.where(np.arange(X.shape[0]) % 2 == 0, 1.0 + 2.0 ** -10, 1.0 - 2.0 ** -10)
    return (X.astype(np.float64) * (f[:, None] if X.ndim == 2 else f)).astype(X.dtype)


def full_from_upper(A):
    """The symmetric matrix whose upper triangle is that of A (the lower triangle of A is not looked at)."""
    Uo = np.triu(A, 1)
    return np.triu(A) + Uo.T


# ------------------------------------------------------------------ twins
def resid_bound_sym(A, x, b):
    """r = b - A x and w = |b| + |A| |x| from np.triu(A) alone, sums in fp64, rounded once to the working precision."""
    dt = A.dtype
    D = np.triu(A).astype(np.float64)
    Uo = np.triu(A, 1).astype(np.float64)
    x64, b64 = x.astype(np.float64), b.astype(np.float64)
    ax = D @ x64 + Uo.T @ x64
    aax = np.abs(D) @ np.abs(x64) + np.abs(Uo).T @ np.abs(x64)
    return (b64 - ax).astype(dt), (np.abs(b64) + aax).astype(dt)


def lansy(A):
    """1-norm (= infinity-norm) of the symmetric matrix given by np.triu(A), sums in fp64; a NaN gives NaN."""
    n = A.shape[0]
    if n == 0:
        return 0.0
    D = np.abs(np.triu(A).astype(np.float64))
    s = D.sum(axis=0) + np.triu(D, 1).sum(axis=1)
    return float("nan") if np.any(np.isnan(s)) else float(np.max(s))


def potrs_few(U, B):
    """X = inv(U) inv(U^T) B as the few-column path sweeps: forward as cpu_chol.potrs, backward through the whole
    128 x 128 block inverses (no 64-row halves); only triu(U) is used."""
    n = U.shape[0]
    X = np.array(B, dtype=U.dtype, copy=True).reshape(n, -1)
    Uu = np.triu(U)
    inv = {}
    for kb in range(0, n, cc.SB):
        e = min(kb + cc.SB, n)
        inv[kb] = cc.diag_block(Uu[kb:e, kb:e], factored=True)[1]
    for kb in range(0, n, cc.SB):                                  # U^T Y = B
        e = min(kb + cc.SB, n)
        X[kb:e] = inv[kb].T @ X[kb:e]
        if e < n:
            X[e:] = X[e:] - Uu[kb:e, e:].T @ X[kb:e]
    for kb in range(((n - 1) // cc.SB) * cc.SB, -1, -cc.SB):       # U X = Y
        e = min(kb + cc.SB, n)
        X[kb:e] = inv[kb] @ X[kb:e]
        if kb > 0:
            X[:kb] = X[:kb] - Uu[:kb, kb:e] @ X[kb:e]
    return X.reshape(np.shape(B))


# the (n, nrhs) of tests/test_gpu_chol.py::test_planted_solve that the few-column path serves (nrhs <= 8), same seeds
PLANTED_FEW = ((1, 1), (2, 7), (128, 1), (129, 7), (600, 1))
# ... and those of them that are NOT exact in fp32: a few entries of an fp32 128 x 128 block inverse need more than 24
# bits and X is dense here, so they meet non-zeros.  The model of the block sweeps (cpu_chol.potrs) is
# inexact on the same two and exact on the others, like the twin of the few-column path: tests/test_posx_host.py.
PLANTED_FEW_INEXACT_F32 = ((128, 1), (129, 7))


def planted_exact(n, nrhs, dtype):
    return np.dtype(dtype) == np.float64 or (n, nrhs) not in PLANTED_FEW_INEXACT_F32


def planted_system(n, nrhs, dtype):
    """(U, A, X, B) of test_planted_solve: the planted factor, integer X in [-3, 3], B = A X (exact)."""
    U, A = cc.planted(n, dtype=dtype)
    X = np.random.default_rng(n + nrhs).integers(-3, 4, (n, nrhs)).astype(dtype)
    B = (A.astype(np.float64) @ X.astype(np.float64)).astype(dtype)
    return U, A, X, B


def pocon_twin(U, anorm, count=None):
    """LAPACK's pocon: (1 / est) / anorm, est from lacn2 around x <- inv(U) inv(U^T) x for both kase values."""
    n = U.shape[0]
    if n == 0:
        return 1.0
    d = np.diag(U)
    if anorm == 0 or np.any(d == 0) or np.any(np.isnan(d)):
        return 0.0
    Uu = np.triu(U)
    est = cr.lacn2(n, lambda kase, x: cc.potrs(Uu, x), U.dtype, count)
    return (1.0 / est) / anorm if (est > 0 and np.isfinite(est)) else 0.0


def porfs_twin(A, U, b, x, steps=None, solves=None):
    """One right-hand side of porfs: (x refined, ferr, berr).  The structure of cpu_refine.gerfs_twin."""
    n, dt = A.shape[0], A.dtype
    if n == 0:
        return x, 0.0, 0.0
    u = cr.unit(dt)
    Uu = np.triu(U)
    x = x.copy()
    lstres, count = 3.0, 0
    while True:
        r, w = resid_bound_sym(A, x, b)
        berr = cr.berr_of(r, w)
        if berr > u and 2.0 * berr <= lstres and count < cr.ITMAX:
            x = (x + cc.potrs(Uu, r)).astype(dt)
            lstres = berr
            count += 1
        else:
            break
    if steps is not None:
        steps.append(count)
    if berr != berr:
        return x, berr, berr
    W = cr.weights(r, w)

    def apply(kase, v):      # M = diag(W) inv(A): inv(A) is symmetric
        if kase == 1:
            return (W * cc.potrs(Uu, v)).astype(dt)
        return cc.potrs(Uu, (W * v).astype(dt)).astype(dt)

    est = cr.lacn2(n, apply, dt, solves)
    xmax = float(np.max(np.abs(x)))
    return x, (est / xmax if xmax != 0 else est), berr


# ------------------------------------------------------------------ cases, computed once and never modified
_cond = {}


def cond_case(n, prec):
    """The condition-estimate case of (n, precision): the matrix, LAPACK's factor of it, its norm, LAPACK's pocon on
    that factor, the exact reciprocal condition number and the agreement bound 64 n eps cond_1 (cpu_cond.bound)."""
    from scipy.linalg import lapack

    key = (n, prec)
    if key not in _cond:
        dt = DTYPES[prec]
        A = scaled_spd(n, 0, SCALE_COND[prec], dt, SHIFT_COND[prec])
        pre = "d" if prec == "f64" else "s"
        c, info = getattr(lapack, pre + "potrf")(A, lower=0)
        assert info == 0
        Ul = np.triu(c).astype(dt)
        anorm = float(np.abs(A.astype(np.float64)).sum(axis=0).max())
        rl, info = getattr(lapack, pre + "pocon")(c, anorm, uplo="U")
        assert info == 0
        A64 = A.astype(np.float64)
        cond1 = float(np.linalg.norm(A64, 1) * np.linalg.norm(np.linalg.inv(A64), 1))
        for a in (A, Ul):
            a.setflags(write=False)
        _cond[key] = dict(n=n, prec=prec, A=A, U_lapack=Ul, anorm=anorm, rcond_lapack=float(rl), cond1_exact=cond1,
                          rcond_exact=1.0 / cond1, bound=64.0 * n * EPS[prec] * cond1)
    return _cond[key]


_refine = {}


def refine_case(n, prec):
    """The refinement case of (n, precision): A, B (MAXRHS columns), the numpy model's factor and solution, the
    perturbed start, the true solution of every column for the rounded data, and the inverse of A."""
    key = (n, prec)
    if key not in _refine:
        dt = DTYPES[prec]
        A = scaled_spd(n, 1, SCALE_REFINE[prec], dt)
        B, _ = rhs(A, MAXRHS, n)
        A64 = A.astype(np.float64)
        truth = []
        for j in range(MAXRHS):
            bj = B[:, j].astype(np.float64)
            truth.append(cr.fraction_solve(A64, bj) if n <= 2 else cr.longdouble_solve(A64, bj))
        inv = np.linalg.inv(A64)
        R, info = cc.potrf(A)
        assert info == 0
        Um = np.triu(R)
        X0 = perturbed(cc.potrs(Um, B))
        for a in (A, B, inv, Um, X0):
            a.setflags(write=False)
        _refine[key] = dict(A=A, B=B, truth=truth, inv=inv, U_model=Um, X0_model=X0)
    return _refine[key]


def check_columns(tag, n, prec, A, B, truth, inv, X, ferr, berr, steps, solves):
    """The yardsticks of tests/test_gpu_refine.py::_check_columns for a refined X (n x k) of the first k columns of B,
    without the 'improves' clause (the start is perturbed, see `perturbed`).  Prints every figure before it asserts."""
    u = cr.unit(DTYPES[prec])
    k = X.shape[1]
    for j in range(k):
        om = cr.omega(A, X[:, j], B[:, j])
        err = cr.true_error(X[:, j], truth[j])
        exact = cr.exact_bound(A, X[:, j], B[:, j], inv=inv)
        print(f"{tag} col {j}: berr/u {berr[j] / u:.3f} omega/u {om / u:.3f} |diff|/u {abs(berr[j] - om) / u:.3f} allowed "
              f"{(n + 1) * (1 + om):.1f}  ferr {ferr[j]:.3e} exact bound {exact:.3e} ratio {ferr[j] / exact:.3f} "
              f"true error {err:.3e}  steps(max) {steps} solves {solves}")
        assert abs(berr[j] - om) <= (n + 1) * u * (1 + om)
        assert om <= 4 * u
        assert ferr[j] >= err
        assert exact / 6 <= ferr[j] <= 3 * exact
    assert 1 <= steps <= 5
    assert (4 if n > 1 else 1) * k <= solves <= 11 * k
