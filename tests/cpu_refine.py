"""CPU statement of the refined solve with error bounds (lsx_gerfs_*): LAPACK's gerfs in numpy, the counterpart of
cpu_cond.py.  The twin is the readable form of what the device runs: residual and componentwise bound in one pass,
the guarded backward error, the refinement loop with its three stopping tests, and lacn2 wrapped around solves with
op(A) and op(A)^T for the forward bound.  Also the inputs of the tests (badly scaled systems on which the first solve
is componentwise backward-unstable, so that refinement has something to do) and the independent yardsticks: the
backward error in extended precision, the exact value of the quantity lacn2 estimates, and true solutions.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

U = {np.dtype(np.float64): 2.0 ** -53, np.dtype(np.float32): 2.0 ** -24}      # LAPACK's lamch('E')
SAFMIN = {np.dtype(np.float64): 2.0 ** -1022, np.dtype(np.float32): 2.0 ** -126}
ITMAX = 5


def unit(dtype) -> float:
    return U[np.dtype(dtype)]


def scaled_system(n: int, seed: int, nrhs=None):
    """Columns scaled by 2^-30 .. 2^30, every third row by 2^-20, a solution scaled against the columns: (A, b, xt).
    nrhs=None gives vectors; nrhs=k gives n x k arrays whose first column is that vector."""
    rng = np.random.default_rng(seed)
    M = rng.uniform(-1, 1, (n, n))
    d = 2.0 ** rng.integers(-30, 31, n)
    A = M * d[None, :]
    A[::3] *= 2.0 ** -20
    xt = rng.uniform(-1, 1, n) / d
    if nrhs is None:
        return A, A @ xt, xt
    XT = np.empty((n, nrhs))
    XT[:, 0] = xt
    for j in range(1, nrhs):
        XT[:, j] = rng.uniform(-1, 1, n) / d
    B = np.empty((n, nrhs))
    for j in range(nrhs):
        B[:, j] = A @ XT[:, j]          # column by column: column 0 has the bits of the vector form
    return A, B, XT


def op(A, trans):
    return A.T if trans else A


def resid_bound(A, x, b, trans=False):
    """r = b - op(A) x and w = |b| + |op(A)| |x|, sums in fp64, rounded once to the working precision."""
    dt = A.dtype
    M, x64, b64 = op(A, trans).astype(np.float64), x.astype(np.float64), b.astype(np.float64)
    return (b64 - M @ x64).astype(dt), (np.abs(b64) + np.abs(M) @ np.abs(x64)).astype(dt)


def safe(n, dtype):
    s1 = (n + 1) * SAFMIN[np.dtype(dtype)]
    return s1, s1 / unit(dtype)


def berr_of(r, w):
    """max_i |r_i| / w_i, guarded as in dgerfs where w_i <= safe2; a NaN wins."""
    n = r.shape[0]
    if n == 0:
        return 0.0
    s1, s2 = safe(n, r.dtype)
    r, w = np.abs(r.astype(np.float64)), w.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(w > s2, r / w, (r + s1) / (w + s1))
    return float("nan") if np.any(np.isnan(q)) else float(np.max(q))


def sign(x):
    return np.where(x >= 0, 1.0, -1.0).astype(x.dtype)


def lacn2(n, apply, dtype, count=None):
    """LAPACK's lacn2: estimate of the 1-norm of M from apply(1, x) = M x and apply(2, x) = M^T x (the loop of
    cpu_cond.rcond_twin with the operator left open).  count (a list) receives the number of applications."""
    napp = [0]

    def ap(kase, x):
        napp[0] += 1
        return apply(kase, x)

    asum = lambda v: float(np.sum(np.abs(v.astype(np.float64))))   # noqa: E731
    x = ap(1, np.full(n, 1.0 / n, dtype=dtype))
    est = asum(x)
    if n > 1:
        isgn = sign(x)
        x = ap(2, isgn)
        j = int(np.argmax(np.abs(x)))
        for it in range(2, 6):
            e = np.zeros(n, dtype=dtype)
            e[j] = 1.0
            x = ap(1, e)
            estold, est = est, asum(x)
            if np.array_equal(sign(x), isgn) or est <= estold:
                break
            isgn = sign(x)
            x = ap(2, isgn)
            jlast, j = j, int(np.argmax(np.abs(x)))
            if not (x[jlast] != abs(x[j]) and it < 5):
                break
        alt = (np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * (1.0 + np.arange(n) / (n - 1.0))).astype(dtype)
        est = max(est, 2.0 * asum(ap(1, alt)) / (3.0 * n))
    if count is not None:
        count.append(napp[0])
    return est


def weights(r, w):
    """W = |r| + (n + 1) u w, plus safe1 where w <= safe2 (dgerfs)."""
    n = r.shape[0]
    s1, s2 = safe(n, r.dtype)
    r64, w64 = np.abs(r.astype(np.float64)), w.astype(np.float64)
    return (r64 + (n + 1) * unit(r.dtype) * w64 + np.where(w64 > s2, 0.0, s1)).astype(r.dtype)


def gerfs_twin(A, lu_piv, b, x, trans=False, steps=None, solves=None):
    """One right-hand side of gerfs: returns (x refined, ferr, berr).  lu_piv = scipy.linalg.lu_factor(A), all in
    the working precision of A.  steps / solves (lists) receive the refinement steps and the estimator's solves."""
    from scipy.linalg import lu_solve

    n, dt = A.shape[0], A.dtype
    if n == 0:
        return x, 0.0, 0.0
    u = unit(dt)
    x = x.copy()
    lstres, count = 3.0, 0
    while True:
        r, w = resid_bound(A, x, b, trans)
        berr = berr_of(r, w)
        if berr > u and 2.0 * berr <= lstres and count < ITMAX:
            x = (x + lu_solve(lu_piv, r, trans=1 if trans else 0).astype(dt)).astype(dt)
            lstres = berr
            count += 1
        else:
            break
    if steps is not None:
        steps.append(count)
    if berr != berr:
        return x, berr, berr
    W = weights(r, w)

    def apply(kase, v):      # M = diag(W) inv(op A)^T: ||M||_1 = || inv(op A) diag(W) ||_inf
        if kase == 1:
            return (W * lu_solve(lu_piv, v, trans=0 if trans else 1)).astype(dt)
        return lu_solve(lu_piv, (W * v).astype(dt), trans=1 if trans else 0).astype(dt)

    est = lacn2(n, apply, dt, solves)
    xmax = float(np.max(np.abs(x)))
    return x, (est / xmax if xmax != 0 else est), berr


def omega(A, x, b, trans=False) -> float:
    """Componentwise backward error max_i |b - op(A) x|_i / (|b| + |op(A)| |x|)_i in extended precision (0/0 = 0)."""
    if A.shape[0] == 0:
        return 0.0
    M, xl, bl = op(A, trans).astype(np.longdouble), x.astype(np.longdouble), b.astype(np.longdouble)
    r = np.abs(bl - M @ xl)
    w = np.abs(bl) + np.abs(M) @ np.abs(xl)
    q = np.where(w > 0, r / np.where(w > 0, w, 1), np.where(r > 0, np.inf, 0))
    return float(np.max(q))


def exact_bound(A, x, b, trans=False, inv=None) -> float:
    """|| |inv(op A)| (|r| + (n + 1) u w) ||_inf / ||x||_inf: what lacn2 estimates in gerfs, from numpy's inverse
    (fp64 whatever the precision of the data, whose unit roundoff u enters).  inv: that inverse of op(A), if the
    caller has it already."""
    n = A.shape[0]
    r, w = resid_bound(A, x, b, trans)
    Wt = np.abs(r.astype(np.float64)) + (n + 1) * unit(A.dtype) * w.astype(np.float64)
    if inv is None:
        inv = np.linalg.inv(op(A, trans).astype(np.float64))
    return float(np.max(np.abs(inv) @ Wt) / np.max(np.abs(x.astype(np.float64))))


def fraction_solve(A, b):
    """Exact solution of op-free A x = b over the rationals (Gaussian elimination on Fractions); small n only."""
    n = A.shape[0]
    M = [[Fraction(float(v)) for v in row] + [Fraction(float(bv))] for row, bv in zip(A, b)]
    for k in range(n):
        p = next(i for i in range(k, n) if M[i][k] != 0)
        M[k], M[p] = M[p], M[k]
        piv = M[k][k]
        for i in range(k + 1, n):
            if M[i][k] != 0:
                f = M[i][k] / piv
                M[i] = [a - f * c for a, c in zip(M[i], M[k])]
    x = [Fraction(0)] * n
    for k in range(n - 1, -1, -1):
        x[k] = (M[k][n] - sum(M[k][j] * x[j] for j in range(k + 1, n))) / M[k][k]
    return x


def longdouble_solve(A, b, trans=False):
    """Solution of op(A) x = b in extended precision: an fp64 LU, residuals and updates in longdouble, until the
    update no longer changes x (the fp64 factors contract by cond * 2^-53 per step)."""
    from scipy.linalg import lu_factor, lu_solve

    M = op(A, trans).astype(np.float64)
    Ml, bl = M.astype(np.longdouble), b.astype(np.longdouble)
    f = lu_factor(M)
    x = lu_solve(f, b.astype(np.float64)).astype(np.longdouble)
    for _ in range(40):
        r = bl - Ml @ x
        d = lu_solve(f, r.astype(np.float64)).astype(np.longdouble)
        xn = x + d
        if np.array_equal(xn, x) or np.max(np.abs(d)) <= 4 * np.finfo(np.longdouble).eps * np.max(np.abs(xn)):
            return xn
        x = xn
    return x


def true_error(x, xt) -> float:
    """max|x - xt| / max|x| with xt a list of Fractions or a longdouble array."""
    if len(x) == 0:
        return 0.0
    if isinstance(xt[0], Fraction):
        num = max(abs(Fraction(float(v)) - t) for v, t in zip(x, xt))
        den = max(abs(Fraction(float(v))) for v in x)
        return float(num / den) if den else float(num)
    xl = x.astype(np.longdouble)
    den = np.max(np.abs(xl))
    num = np.max(np.abs(xl - xt))
    return float(num / den) if den else float(num)
