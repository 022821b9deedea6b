"""The SPD inverse of linalg_solver_amd/csrc (trtri_upper_t / potri_dev in api.hip, lauum_tn_kernel in kernels_gemm.hip)
written down in numpy, the planted-inverse builder of its tests, and LAPACK's test ratio for an inverse.

inv(A) = inv(U) inv(U)^T = V^T V with V = inv(U^T), lower triangular.  The model follows the driver step for step in the
working precision: phase 1 is the forward substitution U^T V = I over 128-row steps, block row kb on its columns
[0, kb + jb) only, the diagonal blocks through cpu_chol.diag_block(factored=True) -- the block inverses the kernels
form; phase 2 is the trapezoid product, tile (I, J) of 128 x 128 summed over k >= 128 J only.  It does not model the
order of summation inside a product, so on rounded inputs it agrees with the GPU to rounding; on the planted inputs
every intermediate is exactly representable and both must return the planted inverse exactly
(tests/test_potri_host.py proves that of the model for every order and seed the GPU tests use).
"""
import functools

import numpy as np

import cpu_chol as cc

SB = cc.SB
PLANTED_ORDERS = [1, 2, 127, 128, 129, 257, 300, 384, 400, 600]
PLANTED_SEED = 1


# ------------------------------------------------------------------ builders
@functools.lru_cache(maxsize=None)
def _planted(n, seed):
    rng = np.random.default_rng(2000 * n + seed)
    d = rng.choice(np.array([1, 2, 4, 8]), n)
    N = np.zeros((n, n), dtype=np.int64)
    mask = np.triu(rng.random((n, n)) < min(1.0, 8.0 / n), 1)
    mask &= (np.arange(n)[:, None] % 2 == 0) & (np.arange(n)[None, :] % 2 == 1)
    vals = rng.integers(1, 4, (n, n)) * rng.choice(np.array([-1, 1]), (n, n))
    N[mask] = vals[mask]
    assert not (N @ N).any()
    eye = np.eye(n, dtype=np.int64)
    U = d[:, None] * (eye - N)
    A = U.T @ U
    W = (eye + N) * (8 // d)[None, :]            # 8 inv(U) = (I + N) 8 D^-1
    X64 = W @ W.T                                # 64 inv(A)
    assert np.array_equal((U @ W), 8 * eye)
    return d, U, A, W, X64


def planted(n, seed=PLANTED_SEED, dtype=np.float64):
    """(U, A, V, X): U = D (I - N) with D diagonal in {1, 2, 4, 8} and N strictly upper, entries of +-{1, 2, 3} with
    probability min(1, 8 / n) on (even row, odd column) positions only, so N^2 = 0 and inv(U) = (I + N) D^-1.
    A = U^T U is integer-valued; V = inv(U^T) = D^-1 (I + N)^T has entries k / 8; X = inv(A) = V^T V has entries
    k / 64.  Everything is exact in fp32 and fp64.  Fresh copies."""
    d, U, A, W, X64 = _planted(n, seed)
    return U.astype(dtype), A.astype(dtype), (W.T / 8.0).astype(dtype), (X64 / 64.0).astype(dtype)


def planted_magnitudes(n, seed=PLANTED_SEED):
    """(max |A|, max |64 inv(A)|) of the planted pair, as integers."""
    _, _, A, _, X64 = _planted(n, seed)
    return int(np.abs(A).max()), int(np.abs(X64).max())


def planted_det_parts(n, seed=PLANTED_SEED):
    """det(A) = prod d_i^2 as (sign, mant, exp2): an exact power of two, mant = 0.5, exp2 = 1 + 2 sum log2 d_i."""
    d = _planted(n, seed)[0]
    return 1.0, 0.5, 1 + 2 * int(np.log2(d).sum())


def lower_blocks_nan(V):
    """A copy of V whose blocks strictly above the diagonal 128-blocks hold NaN."""
    out = V.copy()
    n = V.shape[0]
    for kb in range(0, n, SB):
        out[kb:kb + SB, min(kb + SB, n):] = np.nan
    return out


# ------------------------------------------------------------------ the algorithm
def trtri_upper_t(U, V=None):
    """V = inv(U^T) on and below the diagonal 128-blocks; only triu(U) is used.  V: an array to write into (the blocks
    strictly above its diagonal blocks keep what they hold); default: zeros there."""
    n = U.shape[0]
    if V is None:
        V = np.zeros((n, n), dtype=U.dtype)
    for kb in range(0, n, SB):                                  # the identity where the sweep works
        e = min(kb + SB, n)
        V[kb:e, :e] = np.eye(e - kb, e, kb, dtype=U.dtype)
    for kb in range(0, n, SB):
        e = min(kb + SB, n)
        inv = cc.diag_block(np.triu(U[kb:e, kb:e]), factored=True)[1]
        V[kb:e, :e] = inv.T @ V[kb:e, :e]
        if e < n:
            V[e:, :e] = V[e:, :e] - U[kb:e, e:].T @ V[kb:e, :e]
    return V


def lauum_tn(V, C=None):
    """Upper triangle of C = V^T V for a lower-triangular V, tile (I, J) of 128 x 128 over k >= 128 J only: the blocks of
    V strictly above its diagonal blocks are never read.  The strictly lower triangle of C keeps what it holds."""
    n = V.shape[0]
    if C is None:
        C = np.zeros((n, n), dtype=V.dtype)
    for j0 in range(0, n, SB):
        j1 = min(j0 + SB, n)
        for i0 in range(0, j0 + 1, SB):
            i1 = min(i0 + SB, n)
            P = V[j0:, i0:i1].T @ V[j0:, j0:j1]
            if i0 == j0:
                up = np.triu(np.ones(P.shape, dtype=bool))
                C[i0:i1, j0:j1] = np.where(up, P, C[i0:i1, j0:j1])
            else:
                C[i0:i1, j0:j1] = P
    return C


def potri(R):
    """LAPACK's potri on a copy of the factor array R: the upper triangle becomes that of inv(A), the strictly lower
    triangle is R's, untouched.  Returns (result, info): info = i + 1 for the first zero or NaN u_ii."""
    d = np.diagonal(R)
    bad = np.flatnonzero((d == 0) | np.isnan(d))
    info = int(bad[0]) + 1 if bad.size else 0
    with np.errstate(all="ignore"):
        V = trtri_upper_t(np.triu(R))
        return lauum_tn(V, R.copy()), info


def symmetrize(X):
    """Both triangles from the upper one."""
    T = np.triu(X)
    return T + np.triu(T, 1).T


# ------------------------------------------------------------------ yardstick (np.longdouble)
def inverse_ratio(A, X):
    """LAPACK's test ratio of an inverse (dpot03): ||I - A X||_1 / (n u ||A||_1 ||X||_1), A and X symmetric and full as
    stored, u the unit roundoff of X's type, evaluated in extended precision."""
    n = A.shape[0]
    u = cc.UNIT[np.dtype(X.dtype)]
    Al = np.asarray(A, dtype=np.longdouble)
    Xl = np.asarray(X, dtype=np.longdouble)
    R = np.eye(n, dtype=np.longdouble) - Al @ Xl
    one = lambda M: np.abs(M).sum(axis=0).max()
    return float(one(R) / (n * u * one(Al) * one(Xl)))
