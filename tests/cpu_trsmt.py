"""CPU statement of the blocked transposed solve: a numpy twin of the sweeps the device runs for many right-hand sides
(lsx_getrs_t_* with nrhs >= "getrs_t_blocked_min"), the inputs the GPU tests use, and the bounds both are held to.

The twin is the readable form of lu_solve_transposed_blocked (csrc/api.hip): 128-row blocks, the diagonal blocks applied
as explicit inverses, every other operation a product C -= A^T B with A a block row of U or L as it lies in the
row-major factors, two work arrays that take turns, and the row scatter at the end.  It rounds where numpy's matmul
rounds, not where the MFMA tile does: it shows what the algorithm costs in accuracy, not the device's bits.
"""
from __future__ import annotations

import numpy as np

SB = 128                # block edge of the sweeps
ORDERS = [129, 256, 257, 300, 1000, 2100]
NCOLS = 256             # right-hand sides generated per order; tests take the leading ones

# the bounds of tests/test_gpu_transposed.py, which the blocked path is held to as well
TOL_NUMPY = 1e-9        # fp64 against np.linalg.solve(A.T, B)
TOL_FACTORS = 1e-11     # fp64 against substitution on the same factors (variant against variant)
TOL_RESID = 1e-9        # times n: max |A^T X - B|
TOL32 = 1e-4            # fp32: norm-wise backward error


def system(n: int):
    """A and the right-hand sides of order n: the matrices of tests/test_gpu_transposed.py, more columns of the same
    stream (an entry depends on the seed and its position only)."""
    from linalg_solver_amd import gen

    A, _ = gen.system(gen.U11, 1300 + n, n)
    return A, gen.fill(gen.U11, 2300 + n, n, NCOLS)


def system32(n: int, nrhs: int):
    """The fp32 inputs: the matrix stream of test_transposed_solve_fp32."""
    from linalg_solver_amd import gen

    A, _ = gen.system(gen.U11, 950 + n, n)
    return A, np.random.default_rng(n).uniform(-1, 1, (n, nrhs))


def perm_of(ipiv) -> np.ndarray:
    p = np.arange(len(ipiv))
    for k, q in enumerate(ipiv):
        p[k], p[q] = p[q], p[k]
    return p   # (P b)[i] = b[p[i]]


def substitution(LU, ipiv, B):
    """Plain substitution on the given factors: U^T y = b, L^T z = y, x[perm] = z."""
    from scipy.linalg import solve_triangular as trs

    Z = trs(LU, trs(LU, B, lower=False, trans=1), lower=True, unit_diagonal=True, trans=1)
    X = np.empty_like(Z)
    X[perm_of(ipiv)] = Z
    return X


def block_inverses(LU: np.ndarray):
    """inv(U_kk) and inv(L_kk) of the 128-row diagonal blocks, natural orientation, in the precision of LU."""
    from scipy.linalg import solve_triangular as trs

    n = LU.shape[0]
    invU, invL = [], []
    for kb in range(0, n, SB):
        D = LU[kb:kb + SB, kb:kb + SB]
        eye = np.eye(D.shape[0], dtype=LU.dtype)
        invU.append(trs(D, eye, lower=False).astype(LU.dtype))
        invL.append(trs(D, eye, lower=True, unit_diagonal=True).astype(LU.dtype))
    return invL, invU


def blocked_transposed_solve(LU: np.ndarray, ipiv, B: np.ndarray) -> np.ndarray:
    """A^T X = B from P A = L U by the blocked sweeps, in the precision of LU."""
    n = LU.shape[0]
    invL, invU = block_inverses(LU)
    W = np.array(B, dtype=LU.dtype, copy=True)
    Y = np.empty_like(W)
    for kb in range(0, n, SB):                            # forward: U^T Y = B
        ke = min(kb + SB, n)
        Y[kb:ke] = invU[kb // SB].T @ W[kb:ke]
        W[ke:] -= LU[kb:ke, ke:].T @ Y[kb:ke]
    for kb in range((n - 1) // SB * SB, -1, -SB):         # backward: L^T Z = Y, Z into W
        ke = min(kb + SB, n)
        W[kb:ke] = invL[kb // SB].T @ Y[kb:ke]
        Y[:kb] -= LU[kb:ke, :kb].T @ W[kb:ke]
    X = np.empty_like(W)
    X[perm_of(ipiv)] = W                                  # the scatter: X[perm[i]] = Z[i]
    return X


def backward_error32(A, X, B) -> float:
    """The norm-wise backward error of test_transposed_solve_fp32."""
    return float(np.linalg.norm(A.T @ X.astype(np.float64) - B) /
                 (np.linalg.norm(A) * np.linalg.norm(X) + np.linalg.norm(B)))
