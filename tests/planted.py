"""Planted factorisations: matrices whose LU factorisation with partial pivoting is known without running anything
(TESTS ONLY).

planted(n, seed) returns A, L, U, perm with A[perm] == L @ U exactly and

  L   unit lower; a strictly-lower entry is non-zero with probability min(1, 16/n), drawn from {+-1/4, +-1/2};
  U   upper; |U_kk| in {4, 8}, a strictly-upper entry non-zero with the same probability, an integer in [-3, 3];
  perm a random permutation.

Every entry of A and of every Schur complement L[k:, k:] @ U[k:, k:] is a multiple of 1/4 and a sum of at most n
products of magnitude <= 3/2 (in practice a few dozen: both factors are sparse), far below 2^24 / 4.  So every
operation of Gaussian elimination is exact in fp32 and in fp64, whatever the order of the sums.  The candidates of
column k are L[i, k] * U_kk with |L[i, k]| <= 1/2 off the diagonal: the pivot is unique, no tie rule is involved.
Hence, for either precision: factors tril(L, -1) + U, info = 0, and ipiv = the interchange sequence that realises
perm (ipiv_of_perm).  Both factors are sparse on purpose: with a dense random U the inverse of U grows like 1e50 at
n = 300, and one rounding in a blocked algorithm could move a later pivot.

zero_at = k plants U_kk = 0: the columns before k are unaffected, column k has no non-zero candidate, so the
elimination reports info = k + 1 after the planted pivot prefix ipiv[:k].
"""
import numpy as np


def ipiv_of_perm(perm):
    """The LAPACK-style interchange sequence (step k swaps rows k and ipiv[k], 0-based) after which row k holds the
    original row perm[k].  O(n): `at` says which original row sits at a position, `pos` is its inverse."""
    n = len(perm)
    at = np.arange(n)
    pos = np.arange(n)
    ipiv = np.empty(n, dtype=np.int32)
    for k in range(n):
        r = int(perm[k])
        p = int(pos[r])           # where the wanted row is now; p >= k because rows 0..k-1 are final
        ipiv[k] = p
        o = int(at[k])
        at[k], at[p] = r, o
        pos[r], pos[o] = k, p
    return ipiv


def perm_of_ipiv(ipiv, n=None):
    """The inverse conversion: p with (P A)[i] = A[p[i]]."""
    p = np.arange(len(ipiv) if n is None else n)
    for k, q in enumerate(ipiv):
        p[k], p[q] = p[q], p[k]
    return p


def perm_sign(perm):
    """+1.0 / -1.0: parity of the permutation, from its cycles."""
    seen = np.zeros(len(perm), dtype=bool)
    sign = 1.0
    for i in range(len(perm)):
        if not seen[i]:
            j, length = i, 0
            while not seen[j]:
                seen[j] = True
                j = int(perm[j])
                length += 1
            if length % 2 == 0:
                sign = -sign
    return sign


def planted_factors(n, seed, zero_at=None):
    """L, U, perm of the module docstring (float64 arrays)."""
    rng = np.random.default_rng([int(seed), int(n)])
    p = min(1.0, 16.0 / n)
    L = np.where(rng.random((n, n)) < p, rng.choice(np.array([-0.5, -0.25, 0.25, 0.5]), (n, n)), 0.0)
    L = np.tril(L, -1)
    L[np.arange(n), np.arange(n)] = 1.0
    U = np.where(rng.random((n, n)) < p, rng.integers(-3, 4, (n, n)).astype(np.float64), 0.0)
    U = np.triu(U, 1)
    U[np.arange(n), np.arange(n)] = rng.choice(np.array([-8.0, -4.0, 4.0, 8.0]), n)
    if zero_at is not None:
        U[zero_at, zero_at] = 0.0
    perm = rng.permutation(n)
    return L, U, perm


def planted(n, seed, zero_at=None, matmul=None):
    """A, L, U, perm with A[perm] == L @ U.  matmul: a replacement for numpy's product (the product is exact in any
    summation order, so a test on a GPU box may form it there at large orders)."""
    L, U, perm = planted_factors(n, seed, zero_at)
    PA = (L @ U) if matmul is None else matmul(L, U)
    A = np.empty_like(PA)
    A[perm] = PA
    return A, L, U, perm


def planted_lu(L, U):
    """The factor matrix a getrf returns: L below the diagonal, U on and above it."""
    return np.tril(L, -1) + U


def eliminate(A, dtype):
    """Plain right-looking Gaussian elimination with partial pivoting in `dtype`, first maximum wins (the rule of
    LAPACK's i?amax and of this library).  Returns LU, ipiv, info as lsx_getrf_* define them: info = k + 1 for the
    first exactly-zero pivot, and the elimination goes on."""
    a = np.array(A, dtype=dtype, order="C", copy=True)
    n = a.shape[0]
    ipiv = np.zeros(n, dtype=np.int32)
    info = 0
    for k in range(n):
        p = k + int(np.argmax(np.abs(a[k:, k])))
        ipiv[k] = p
        if p != k:
            a[[k, p]] = a[[p, k]]
        if a[k, k] == 0:
            info = info or k + 1
            continue
        a[k + 1:, k] /= a[k, k]
        a[k + 1:, k + 1:] -= np.outer(a[k + 1:, k], a[k, k + 1:])
    return a, ipiv, info


def cond_inf_triangular(T, lower, unit=False):
    """||T||_inf ||T^-1||_inf in fp64."""
    from numpy.linalg import norm

    n = T.shape[0]
    M = np.tril(T) if lower else np.triu(T)
    if unit:
        M = M.copy()
        M[np.arange(n), np.arange(n)] = 1.0
    return float(norm(M, np.inf) * norm(np.linalg.inv(M), np.inf))


def tie_matrix(n, j, rows, seed, dtype=np.float64):
    """A = blockdiag(I_j, B), B of order m = n - j: eliminating the first j columns multiplies by zero, so the
    candidates of column j are B[:, 0] exactly, whatever the precision.  B[rows, 0] = +-1 (mixed signs: the last of
    `rows` is negative), |B[i, 0]| <= 1/2 elsewhere, the rest of B uniform in [-1, 1] rounded to `dtype`.  Partial
    pivoting with the first-index rule gives ipiv[:j] = arange(j), ipiv[j] = j + min(rows)."""
    rng = np.random.default_rng([int(seed), int(n), int(j)])
    m = n - j
    B = rng.uniform(-1.0, 1.0, (m, m)).astype(dtype).astype(np.float64)
    B[:, 0] *= 0.5
    rows = sorted(rows)
    B[rows, 0] = 1.0
    B[rows[-1], 0] = -1.0 if len(rows) > 1 else 1.0
    if len(rows) > 2:
        B[rows[1::2], 0] = -1.0
    A = np.zeros((n, n))
    A[np.arange(j), np.arange(j)] = 1.0
    A[j:, j:] = B
    return A
