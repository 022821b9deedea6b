"""The Cholesky algorithm of linalg_solver_amd/csrc (kernels_chol.hip, potrf_dev / potrs_dev in api.hip) written down
in numpy, the input builders of the Cholesky tests, and their yardsticks.

The model follows the kernels step for step in the working precision -- 128-row steps; inside a diagonal block the
rows in dpotf2's order with the row scaled by the reciprocal of u_jj; inv(U11) formed alongside as the forward
substitution with U11^T applied to the identity; the block row as inv(U11)^T A12; the trailing update on the upper
triangle only; the solve through the 128 x 128 block inverses (forward, U^T Y = B) and their 64 x 64 diagonal blocks
(backward, U X = Y).  It does not model the order of summation inside a product or the fused multiply-adds, so on
rounded inputs it agrees with the GPU to rounding, not bit for bit; on the planted inputs below every intermediate is
exactly representable and both must return the planted factor exactly (tests/test_chol_host.py proves that of the model
for every seed the GPU tests use).
"""
import functools

import numpy as np

SB = 128
UNIT = {np.dtype(np.float64): 2.0 ** -53, np.dtype(np.float32): 2.0 ** -24}


def gamma(m, dtype):
    """Higham's gamma_m = m u / (1 - m u)."""
    u = UNIT[np.dtype(dtype)]
    return m * u / (1.0 - m * u)


# ------------------------------------------------------------------ builders
@functools.lru_cache(maxsize=None)
def _planted(n, seed):
    rng = np.random.default_rng(1000 * n + seed)
    U = np.zeros((n, n), dtype=np.int64)
    mask = np.triu(rng.random((n, n)) < min(1.0, 8.0 / n), 1)
    vals = rng.integers(1, 4, (n, n)) * rng.choice(np.array([-1, 1]), (n, n))
    U[mask] = vals[mask]
    U[np.arange(n), np.arange(n)] = rng.choice(np.array([2, 4, 8]), n)
    A = U.T @ U
    assert np.abs(A).max() < 2 ** 22, "the planted matrix must be exact in fp32"
    return U, A


# The seed of the planted tests.  The factor is exact at this density, but a few entries of an fp32 block inverse are
# not (inverse entries are dyadic fractions whose numerators can outgrow 24 bits); the result stays exact as long as
# such an entry only meets zeros of the block row.  At seed 0, n = 129 one of them meets a non-zero (the model and the
# GPU are then off by a rounding in that column); seeds 1 .. 5 are exact at every order used, which
# tests/test_chol_host.py proves for this one before the GPU is asked.
PLANTED_SEED = 1


def planted(n, seed=PLANTED_SEED, dtype=np.float64):
    """(U, A): U upper with u_kk in {2, 4, 8} and non-zero integers of [-3, 3] above the diagonal with probability
    min(1, 8 / n); A = U^T U, integer-valued and below 2^22: exact in fp32 and fp64.  Fresh copies."""
    U, A = _planted(n, seed)
    return U.astype(dtype), A.astype(dtype)


def planted_not_pd(n, j, kind, seed=PLANTED_SEED, dtype=np.float64):
    """(U, A) with a_jj spoilt so that the pivot of row j is exactly zero ("zero": lowered by u_jj^2), negative
    ("negative": lowered by u_jj^2 + 1) or NaN ("nan")."""
    U, A = planted(n, seed, dtype)
    if kind == "zero":
        A[j, j] -= U[j, j] ** 2
    elif kind == "negative":
        A[j, j] -= U[j, j] ** 2 + 1
    elif kind == "nan":
        A[j, j] = np.nan
    else:
        raise ValueError(kind)
    return U, A


@functools.lru_cache(maxsize=None)
def _spd(n, seed):
    G = np.random.default_rng(77 * n + seed).standard_normal((n, n))
    A = G @ G.T / n + np.eye(n)
    return (A + A.T) / 2


def spd(n, seed=0, dtype=np.float64):
    """A = G G^T / n + I with G standard normal, rounded to dtype (symmetric: both triangles hold the same values)."""
    return _spd(n, seed).astype(dtype)


def fill_lower(A, value):
    """A copy of A whose strictly lower triangle holds `value` (NaN or a canary)."""
    out = A.copy()
    out[np.tril_indices(A.shape[0], -1)] = value
    return out


# ------------------------------------------------------------------ the algorithm
def diag_block(Ablk, factored=False):
    """One diagonal block (jb <= 128), the sweep of kernels_chol.hip.  Ablk: its upper triangle is used.
    factored=False: returns (U11, inv(U11), done) -- done == jb, or the row whose pivot was <= 0 or NaN (then the rows
    before it are final and the inverse is the identity, as the kernel emits it).
    factored=True: Ablk holds U11 already; returns (U11, inv(U11), jb)."""
    dt = Ablk.dtype.type
    jb = Ablk.shape[0]
    M = np.triu(Ablk).astype(Ablk.dtype)        # upper: the matrix; strictly lower: W = inv(U)^T, unscaled
    rinv = np.ones(jb, dtype=Ablk.dtype)
    ujj = np.ones(jb, dtype=Ablk.dtype)
    idx = np.arange(jb)
    done = jb
    for j in range(jb):
        row = M[j].copy()
        d = row[j]
        if not factored:
            if not d > 0:
                done = j
                break
            ujj[j] = np.sqrt(d)
        else:
            ujj[j] = d
        r = dt(1) / ujj[j]
        rinv[j] = r
        xa = row * r                                            # u_jc for c > j, scaled w_jc for c < j
        xw = np.where(idx < j, xa, np.where(idx == j, r, dt(0)))
        ui = (row if factored else xa)[j + 1:]                  # u_ji, i > j
        rows = idx[j + 1:, None]
        cols = idx[None, :]
        x = np.where(cols < rows, xw[None, :], dt(0) if factored else xa[None, :])
        M[j + 1:] = M[j + 1:] - ui[:, None] * x
    U = np.triu(M) * rinv[:, None]
    U[idx, idx] = ujj
    if done < jb:
        U[done:] = np.triu(Ablk)[done:]
        return U, np.eye(jb, dtype=Ablk.dtype), done
    W = np.tril(M, -1) * rinv[:, None]
    W[idx, idx] = rinv
    return U, np.ascontiguousarray(W.T), jb


def potrf(A):
    """(R, info): the blocked right-looking factorisation on a copy; triu(R) is the factor, the strictly lower triangle of R
    is A's, untouched.  info = 0, or j + 1 for the first failing pivot (the rest of the upper triangle is unspecified)."""
    R = A.copy()
    n = R.shape[0]
    info = 0
    up = None
    for kb in range(0, n, SB):
        jb = min(SB, n - kb)
        e = kb + jb
        if info == 0:
            U11, V, done = diag_block(R[kb:e, kb:e])
            R[kb:e, kb:e] = np.triu(U11) + np.tril(R[kb:e, kb:e], -1)
            if done < jb:
                info = kb + done + 1
        else:
            V = np.eye(jb, dtype=R.dtype)
        if e >= n:
            break
        R[kb:e, e:] = V.T @ R[kb:e, e:]                         # U12 = inv(U11)^T A12
        U12 = R[kb:e, e:]
        up = np.triu(np.ones((n - e, n - e), dtype=bool))
        R[e:, e:] = np.where(up, R[e:, e:] - U12.T @ U12, R[e:, e:])
    return R, info


def potrs(U, B):
    """X = inv(U) inv(U^T) B through the block inverses, as potrs_dev sweeps; only triu(U) is used."""
    n = U.shape[0]
    X = np.array(B, dtype=U.dtype, copy=True).reshape(n, -1)
    inv = {}
    for kb in range(0, n, SB):
        e = min(kb + SB, n)
        inv[kb] = diag_block(np.triu(U[kb:e, kb:e]), factored=True)[1]
    for kb in range(0, n, SB):                                  # U^T Y = B
        e = min(kb + SB, n)
        X[kb:e] = inv[kb].T @ X[kb:e]
        if e < n:
            X[e:] = X[e:] - U[kb:e, e:].T @ X[kb:e]
    for kb in range(((n - 1) // SB) * SB, -1, -SB):             # U X = Y, 64-row halves inside a block
        e = min(kb + SB, n)
        V = inv[kb]
        h = kb + 64
        if e > h:
            X[h:e] = V[64:, 64:] @ X[h:e]
            X[kb:h] = X[kb:h] - np.triu(U)[kb:h, h:e] @ X[h:e]
            X[kb:h] = V[:64, :64] @ X[kb:h]
        else:
            X[kb:e] = V[:e - kb, :e - kb] @ X[kb:e]
        if kb > 0:
            X[:kb] = X[:kb] - U[:kb, kb:e] @ X[kb:e]
    return X.reshape(np.shape(B))


# ------------------------------------------------------------------ yardsticks (np.longdouble)
def _utu(U):
    """U^T U for an upper triangular longdouble U, block row by block row (a third of the dense product)."""
    n = U.shape[0]
    P = np.zeros((n, n), dtype=np.longdouble)
    for k0 in range(0, n, 64):
        k1 = min(k0 + 64, n)
        P[k0:, k0:] += U[k0:k1, k0:].T @ U[k0:k1, k0:]
    return P


def factor_residual(A, U):
    """max_ij |A - U^T U|_ij / (|U^T| |U|)_ij over the upper triangle, A and U taken as they are stored."""
    Ul = np.triu(U).astype(np.longdouble)
    num = np.abs(np.asarray(A, dtype=np.longdouble) - _utu(Ul))
    den = _utu(np.abs(Ul))
    up = np.triu_indices(Ul.shape[0])
    return float(np.max(num[up] / den[up]))


def solve_residual(A, U, b, x):
    """max_i |b - A x|_i / (|U^T| |U| |x|)_i, the largest over the columns; A symmetric (full), as stored."""
    Al = np.asarray(A, dtype=np.longdouble)
    Ul = np.abs(np.triu(U).astype(np.longdouble))
    n = Al.shape[0]
    bl = np.asarray(b, dtype=np.longdouble).reshape(n, -1)
    xl = np.asarray(x, dtype=np.longdouble).reshape(n, -1)
    num = np.abs(bl - Al @ xl)
    den = Ul.T @ (Ul @ np.abs(xl))
    zero = den == 0                       # sparse planted factors: a row whose terms all vanish must vanish exactly
    ratio = np.where(zero, np.where(num == 0, 0.0, np.inf), num / np.where(zero, 1.0, den))
    return float(np.max(ratio))
