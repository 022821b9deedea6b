"""CPU statement of the condition estimate: the cases of tests/golden/rcond_cases.json and a numpy/scipy twin of the
iteration the device runs (LAPACK's lacn2 around solves with L U and its transpose, as gecon arranges them).

The twin is the readable form of lsx_gecon_*: the same start vector, the same stopping tests in the same order, the
same final test with the alternating vector.  Like gecon it solves with L and U alone -- the interchanges permute the
columns of the inverse and change neither its 1- nor its infinity-norm.
"""
from __future__ import annotations

import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rcond_cases.json")
EPS = {"f64": float(np.finfo(np.float64).eps), "f32": float(np.finfo(np.float32).eps)}
DTYPE = {"f64": np.float64, "f32": np.float32}


def matrix(kind: str, n: int, seed: int) -> np.ndarray:
    """The fp64 input of a fixture case, regenerated (nothing large is stored)."""
    from linalg_solver_amd import gen

    if n == 0:
        return np.zeros((0, 0))
    if kind == "u11":
        return gen.system(gen.U11, seed, n)[0]
    if kind == "int5":
        return gen.system(gen.INT5, seed, n)[0]
    if kind == "u11_shift":       # U11 + sqrt(n) I: moderately conditioned, for the fp32 cases
        return gen.system(gen.U11, seed, n)[0] + np.sqrt(n) * np.eye(n)
    if kind == "unit_upper":      # 1 on the diagonal, -1 above it: every pivot is 1, cond grows like 2^n
        return np.eye(n) - np.triu(np.ones((n, n)), 1)
    if kind == "u11_zero_col":    # column 17 (0-based) zero: an exactly zero pivot in any operation order
        A = gen.system(gen.U11, seed, n)[0]
        A[:, 17] = 0.0
        return A
    raise ValueError(kind)


def load_cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def bound(case) -> float:
    """Agreement bound of the estimate against LAPACK's: 64 n eps cond_1 (eps of the working precision)."""
    return 64.0 * case["n"] * EPS[case["prec"]] * case["cond1_exact"]


def sign(x):
    return np.where(x >= 0, 1.0, -1.0).astype(x.dtype)       # sign(0) = +1, as LAPACK


def rcond_twin(LU: np.ndarray, anorm: float, norm: str = "1", count=None) -> float:
    """1 / (anorm * est||inv(L U)||) in the 1-norm ("1") or the infinity-norm ("I"); LU in its working precision,
    sums in fp64.  count (a list) receives the number of solves."""
    from scipy.linalg import solve_triangular as trs

    n = LU.shape[0]
    if n == 0:
        return 1.0
    if anorm == 0 or np.any(np.diag(LU) == 0):
        return 0.0
    nsolve = [0]

    def solve(kase, x):            # kase 1: inv(A) x, kase 2: inv(A^T) x; the infinity-norm is the 1-norm of A^T
        nsolve[0] += 1
        if (kase == 1) == (norm == "1"):
            return trs(LU, trs(LU, x, lower=True, unit_diagonal=True), lower=False)
        return trs(LU, trs(LU, x, lower=False, trans=1), lower=True, unit_diagonal=True, trans=1)

    asum = lambda v: float(np.sum(np.abs(v.astype(np.float64))))   # noqa: E731
    x = solve(1, np.full(n, 1.0 / n, dtype=LU.dtype))
    est = asum(x)
    if n > 1:
        isgn = sign(x)
        x = solve(2, isgn)
        j = int(np.argmax(np.abs(x)))                              # first index on ties
        for it in range(2, 6):
            e = np.zeros(n, dtype=LU.dtype)
            e[j] = 1.0
            x = solve(1, e)
            estold, est = est, asum(x)
            if np.array_equal(sign(x), isgn) or est <= estold:
                break
            isgn = sign(x)
            x = solve(2, isgn)
            jlast, j = j, int(np.argmax(np.abs(x)))
            if not (x[jlast] != abs(x[j]) and it < 5):
                break
        alt = (np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * (1.0 + np.arange(n) / (n - 1.0))).astype(LU.dtype)
        est = max(est, 2.0 * asum(solve(1, alt)) / (3.0 * n))
    if count is not None:
        count.append(nsolve[0])
    return (1.0 / est) / anorm if (est > 0 and np.isfinite(est)) else 0.0
