"""The Householder QR of linalg_solver_amd/csrc (kernels_qr.hip, geqrf_dev / ormqr_dev / orgqr_dev / gels_dev in
api.hip) written down in numpy, the input builders of the QR tests, and their yardsticks.

The model follows the kernels in the working precision with fp64 where they have it: 128-column panels; inside a panel
one step per column from the Gram row g_c = sum_{i > j} a_ij a_ic (fp64), the scalars in fp64, every stored element
rounded once; T from G = V^T V by dlarft's recurrence (fp64 sums, one rounding per element); the block apply
W = V^T C, W <- T^T W or T W, C -= V W; the solve with R through the 64 x 64 diagonal-block inverses of
launch_chol_inv (cpu_chol.diag_block).  It does not model the order of summation inside a product or the fused
multiply-adds, so on rounded inputs it agrees with the GPU to rounding; on the planted inputs below every intermediate
is a small integer (or a power of two) and the model, LAPACK and the GPU must agree bit for bit
(tests/test_qr_host.py proves that of the model and LAPACK for every shape and seed the GPU tests use).

Two plants: A = P [U; 0], whose reflectors are e_j +- e_k (one-term Gram sums; it crosses the tau = 0 branch and the
block edges), and A = [0; H[:, :n] U] with a Sylvester-Hadamard H, whose reflectors are dense and whose Gram sums
cancel exactly (see "the dense-reflector plant" below).  The tall shapes of either (16500 and 16514 rows) are the
first with qr_slab_rows = 128, two 64-row chunks per slab of qr_panel_step_kernel.
"""
import functools

import numpy as np

import cpu_chol as cc

QB = 128
UNIT = cc.UNIT


# ------------------------------------------------------------------ builders
@functools.lru_cache(maxsize=None)
def _planted(m, n, seed):
    rng = np.random.default_rng(100000 * m + 100 * n + seed)
    U = np.zeros((n, n), dtype=np.int64)
    mask = np.triu(rng.random((n, n)) < min(1.0, 8.0 / n), 1)
    vals = rng.integers(1, 4, (n, n)) * rng.choice(np.array([-1, 1]), (n, n))
    U[mask] = vals[mask]
    U[np.arange(n), np.arange(n)] = rng.choice(np.array([2, 4, 8]), n) * rng.choice(np.array([-1, 1]), n)
    perm = rng.permutation(m)              # row i of [U; 0] goes to row perm[i] of A
    for i in range(0, n, 7):               # every seventh row stays where it is: tau_i = 0, at any m
        k = int(np.nonzero(perm == i)[0][0])
        perm[k], perm[i] = perm[i], i
    A =np.zeros((m, n), dtype=np.int64)
    A[perm[:n]] = U
    return U, A, perm


PLANTED_SEED = 1


def planted(m, n, seed=PLANTED_SEED, dtype=np.float64):
    """(U, A, perm): U (n x n) upper with a diagonal of +-{2, 4, 8} and non-zero integers of [-3, 3] above it with
    probability min(1, 8 / n); A = P [U; 0] (m x n), row i of [U; 0] at row perm[i].  At step j the rows at or below j
    hold one non-zero in column j, so tau_j is 0 (it sits on the diagonal) or 1 (v = e_j +- e_k, r_jj = -|u_jj|)."""
    U, A, perm = _planted(m, n, seed)
    return U.astype(dtype), A.astype(dtype), perm.copy()


def planted_wide(seed=PLANTED_SEED, dtype=np.float64):
    """129 x 300: a 129 x 129 plant with 171 integer columns of [-3, 3] appended."""
    _, A, _ = planted(129, 129, seed, dtype)
    extra = np.random.default_rng(4242 + seed).integers(-3, 4, (129, 171)).astype(dtype)
    return np.ascontiguousarray(np.hstack([A, extra]))


def planted_zero_column(m, n, j, seed=PLANTED_SEED, dtype=np.float64):
    """The plant with column j and row j of U set to zero (A has a zero column and one more zero row): tau_j = 0 and
    r_jj = 0, the first zero on the diagonal; every later column still has at most one non-zero below the diagonal."""
    U, A, perm = planted(m, n, seed, dtype)
    U[:, j] = 0
    U[j, :] = 0
    A[:, j] = 0
    A[perm[j], :] = 0
    return U, A, perm


def planted_rhs(m, n, nrhs, seed=PLANTED_SEED, dtype=np.float64):
    """(x0, b, enorm): b = A x0 + e with integer x0 in [-3, 3] and integer e non-zero only on the zero rows of A, hence
    orthogonal to the range of A: the least-squares solution is x0 and the residual norms are ||e||_2 (fp64)."""
    _, A, perm = planted(m, n, seed, dtype)
    rng = np.random.default_rng(7 * m + 3 * n + nrhs + seed)
    x0 = rng.integers(-3, 4, (n, nrhs))
    e = np.zeros((m, nrhs), dtype=np.int64)
    e[perm[n:]] = rng.integers(-3, 4, (m - n, nrhs))
    b = A.astype(np.int64) @ x0 + e
    return x0.astype(dtype), b.astype(dtype), np.sqrt((e.astype(np.float64) ** 2).sum(axis=0))


# ------------------------------------------------------------------ the dense-reflector plant
# In the plant above every reflector is e_j +- e_k: each Gram sum g_c = sum_{i > j} a_ij a_ic of the panel step, each
# slot of the cross-slab reduction, each entry of V^T V and each V^T C / C -= V W product has ONE non-zero term, so a
# dropped, doubled or misplaced slab slot, 64-row chunk or K-slice changes nothing those tests can see.  Here every
# reflector is dense and the results are still exact.
#
# H: the Sylvester Hadamard matrix of order N = 4^q, h_ij = (-1)^popcount(i & j); H^T H = N I.
# A = [0 (n x n); H[:, :n] U] with U the signed sparse upper plant of _planted(n, n, seed), n <= N.  At step j the
# column below the diagonal is u_jj H[:, j] (the earlier reflectors removed the other columns of H exactly), so
# alpha = 0, g_j = 4^q u_jj^2, beta = -2^q |u_jj|, tau_j = 1, s = 2^-q / |u_jj| and, with S = diag(sign u_jj):
#   R = -2^q S U,   rows n.. of the array = 2^-q H[:, :n] S,   the strict lower triangle of the top n rows = 0,
#   V^T V = 2 I and T = I,   Q = -2^-q [0; H[:, :n]] S.
# Every reflector has N non-zeros; every off-diagonal Gram sum is N terms of +-integers that cancel to exactly zero or
# add up to 4^q u_jj u_jc.  tests/test_qr_host.py proves all of it of the model and of LAPACK.
# (q, n): 385 x 129 two panels; 512 x 256 two full panels; 1324 x 300 three panels; 16514 x 130 THE TALL CASE:
# qr_slab_rows(16514) = 128, so a workgroup of qr_panel_step_kernel runs its 64-row chunk loop twice (130 slabs, the
# last of 2 rows), the second panel (16386 rows) as well; columns 64 .. 127 put the diagonal row in a second chunk.
HADAMARD_SHAPES = [(4, 129), (4, 256), (5, 300), (7, 130)]
HADAMARD_TALL = (7, 130)
HADAMARD_NRHS = {(4, 129): 7, (4, 256): 64, (5, 300): 200, (7, 130): 3}
TALL_SPARSE = [(16500, 5), (16500, 129)]    # the one-non-zero plant with two chunks per slab: tau = 0 rows included


def hadamard_columns(q, cols):
    """Columns `cols` of the Sylvester Hadamard matrix of order 4^q, as int64 (4^q x len(cols))."""
    N = 4 ** q
    x = np.arange(N, dtype=np.int64)[:, None] & np.asarray(cols, dtype=np.int64)[None, :]
    for sh in (16, 8, 4, 2, 1):               # parity of the set bits
        x ^= x >> sh
    return 1 - 2 * (x & 1)


@functools.lru_cache(maxsize=None)
def _hadamard_plant(q, n, seed):
    N = 4 ** q
    assert 1 <= n <= N
    U = _planted(n, n, seed)[0]
    H = hadamard_columns(q, np.arange(n))
    return U, np.vstack([np.zeros((n, n), dtype=np.int64), H @ U]), H


def hadamard_plant(q, n, seed=PLANTED_SEED, dtype=np.float64):
    """(U, A): A = [0; H[:, :n] U], (n + 4^q) x n, small integers.  Fresh copies."""
    U, A, _ = _hadamard_plant(q, n, seed)
    return U.astype(dtype), A.astype(dtype)


def hadamard_expected(q, n, seed=PLANTED_SEED, dtype=np.float64):
    """(QR, tau, Q): the exact factorisation of hadamard_plant in LAPACK's layout, and the thin Q."""
    U, _, H = _hadamard_plant(q, n, seed)
    S = np.sign(np.diagonal(U))
    below = np.ldexp((H * S[None, :]).astype(np.float64), -q)
    QR = np.vstack([np.ldexp(-(S[:, None] * U).astype(np.float64), q), below])
    Q = np.vstack([np.zeros((n, n)), -below])
    return QR.astype(dtype), np.ones(n, dtype=dtype), Q.astype(dtype)


def hadamard_rhs(q, n, nrhs, seed=PLANTED_SEED, dtype=np.float64):
    """(x0, b, enorm): b = A x0 + [0; e], x0 integer in [-3, 3], column c of e = k_c H[:, p_c] with an integer k_c of
    [-3, 3] and p_c >= n -- a Hadamard column orthogonal to the range of A: the least-squares solution is x0 and the
    residual norm 2^q |k_c|.  n = 4^q leaves no such column: e = 0."""
    N = 4 ** q
    _, A, _ = _hadamard_plant(q, n, seed)
    rng = np.random.default_rng(11 * N + 3 * n + nrhs + seed)
    x0 = rng.integers(-3, 4, (n, nrhs))
    k = rng.integers(-3, 4, nrhs) if n < N else np.zeros(nrhs, dtype=np.int64)
    p = rng.integers(n, N, nrhs) if n < N else np.zeros(nrhs, dtype=np.int64)
    b = A @ x0
    b[n:] += hadamard_columns(q, p) * k[None, :]
    assert np.abs(b).max() < 2 ** 22
    return x0.astype(dtype), b.astype(dtype), np.ldexp(np.abs(k).astype(np.float64), q)


def hadamard_c(m, ncols, dtype=np.float64):
    """The integer C (m x ncols, entries of [-3, 3]) that ormqr is applied to on the Hadamard plant."""
    return np.random.default_rng(1000 * ncols + m).integers(-3, 4, (m, ncols)).astype(dtype)


@functools.lru_cache(maxsize=None)
def hadamard_model(q, n, dtype_name, seed=PLANTED_SEED):
    """(QR, tau) of the numpy model on the Hadamard plant, computed once, read-only."""
    QR, tau = geqrf(hadamard_plant(q, n, seed, np.dtype(dtype_name).type)[1])
    QR.setflags(write=False)
    tau.setflags(write=False)
    return QR, tau


@functools.lru_cache(maxsize=None)
def _uniform(m, n, seed):
    return np.random.default_rng(31 * m + n + seed).uniform(-1.0, 1.0, (m, n))


def uniform(m, n, seed=0, dtype=np.float64):
    return _uniform(m, n, seed).astype(dtype)


# the shapes of the planted GPU tests: the block edges (127, 128, 129), more than one block (257, 384), square, one
# extra row, and tall enough for more than one row slab (300, 600)
PLANTED_SHAPES = sorted({(m, n) for n in (1, 2, 127, 128, 129, 257, 384) for m in (n, n + 1, 300 if n < 300 else 600)})
GELS_SHAPES = [(129, 129), (300, 129), (257, 200), (600, 384)]
GELS_NRHS = [1, 7, 64, 200]
ZERO_COLUMNS = [0, 5, 127, 128, 200]      # in the 300 x 257 plant
LAPACK_THRESH = 30.0                       # LAPACK's own test programs accept these ratios below 30


# ------------------------------------------------------------------ the algorithm
def panel(P, gram_rows=None):
    """The jb reflectors of the panel P (mp x jb, working precision), in place; returns tau.  gram_rows (a boolean
    mask over the panel's rows, default all): the rows whose terms enter the Gram sums -- only for showing that an
    input tells a complete sum from one that misses a chunk of rows."""
    dt = P.dtype
    mp, jb = P.shape
    tau = np.zeros(jb, dtype=dt)
    with np.errstate(all="ignore"):
        for j in range(jb):
            below = P[j + 1:, j:].astype(np.float64)
            if gram_rows is None:
                g = below[:, 0] @ below if mp > j + 1 else np.zeros(jb - j)
            else:
                g = (below[:, 0] * gram_rows[j + 1:]) @ below if mp > j + 1 else np.zeros(jb - j)
            alpha = float(P[j, j])
            if g[0] == 0.0:
                continue
            beta = -np.copysign(np.sqrt(alpha * alpha + g[0]), alpha)
            t = (beta - alpha) / beta
            s = 1.0 / (alpha - beta)
            v = (s * below[:, 0]).astype(dt)
            w = P[j, j + 1:].astype(np.float64) + s * g[1:]
            P[j, j + 1:] = (P[j, j + 1:].astype(np.float64) - t * w).astype(dt)
            P[j + 1:, j + 1:] = (below[:, 1:] - (t * v.astype(np.float64))[:, None] * w[None, :]).astype(dt)
            P[j + 1:, j] = v
            P[j, j] = dt.type(beta)
            tau[j] = dt.type(t)
    return tau


def extract_v(P):
    """The unit lower trapezoid of the panel with explicit ones and zeros."""
    V = np.tril(P, -1)
    jb = P.shape[1]
    V[np.arange(jb), np.arange(jb)] = 1
    return V


def larft(V, tau):
    """dlarft, forward, columnwise, from G = V^T V."""
    dt = V.dtype
    jb = V.shape[1]
    with np.errstate(all="ignore"):
        G = V.T @ V
        T = np.zeros((jb, jb), dtype=dt)
        for i in range(jb):
            if tau[i] != 0:
                T[:i, i] = (-float(tau[i]) * (T[:i, :i].astype(np.float64) @ G[:i, i].astype(np.float64))).astype(dt)
            T[i, i] = tau[i]
    return T


def block_apply(V, T, C, trans):
    """C <- (I - V T V^T)^T C (trans) or (I - V T V^T) C, in place."""
    with np.errstate(all="ignore"):
        W = V.T @ C
        W = (T.T if trans else T) @ W
        C -= V @ W


def geqrf(A):
    """(QR, tau) on a copy, LAPACK's layout."""
    QR = np.array(A, copy=True)
    m, n = QR.shape
    k = min(m, n)
    tau = np.zeros(k, dtype=QR.dtype)
    for kb in range(0, k, QB):
        jb = min(QB, k - kb)
        P = QR[kb:, kb:kb + jb]
        tau[kb:kb + jb] = panel(P)
        if kb + jb < n:
            V = extract_v(P)
            block_apply(V, larft(V, tau[kb:kb + jb]), QR[kb:, kb + jb:], True)
    return QR, tau


def ormqr(QR, tau, C, trans=True):
    """Q^T C (trans) or Q C on a copy, V and T formed again per block."""
    X = np.array(C, dtype=QR.dtype, copy=True)
    k = len(tau)
    starts = list(range(0, k, QB))
    for kb in (starts if trans else starts[::-1]):
        jb = min(QB, k - kb)
        V = extract_v(QR[kb:, kb:kb + jb])
        block_apply(V, larft(V, tau[kb:kb + jb]), X[kb:], trans)
    return X


def orgqr(QR, tau, n=None):
    m = QR.shape[0]
    n = QR.shape[1] if n is None else n
    return ormqr(QR, tau, np.eye(m, n, dtype=QR.dtype), trans=False)


def solve_upper(R, Y):
    """X = inv(R) Y through the 64 x 64 diagonal-block inverses, as sweep_backward takes the 128-row steps; only
    triu(R) is used."""
    n = R.shape[0]
    X = np.array(Y, dtype=R.dtype, copy=True).reshape(n, -1)
    Ru = np.triu(R)
    with np.errstate(all="ignore"):
        for kb in range(((n - 1) // QB) * QB, -1, -QB):
            e = min(kb + QB, n)
            V = cc.diag_block(Ru[kb:e, kb:e], factored=True)[1]
            h = kb + 64
            if e > h:
                X[h:e] = V[64:, 64:] @ X[h:e]
                X[kb:h] = X[kb:h] - Ru[kb:h, h:e] @ X[h:e]
                X[kb:h] = V[:64, :64] @ X[kb:h]
            else:
                X[kb:e] = V[:e - kb, :e - kb] @ X[kb:e]
            if kb > 0:
                X[:kb] = X[:kb] - Ru[:kb, kb:e] @ X[kb:e]
    return X


def diag_info(R):
    d = np.diagonal(R)
    bad = np.nonzero((d == 0) | np.isnan(d))[0]
    return int(bad[0]) + 1 if len(bad) else 0


def gels(A, B):
    """(QR, tau, B_out, info): B_out rows [0, n) the solution, rows [n, m) the tail of Q^T B."""
    m, n = A.shape
    QR, tau = geqrf(A)
    Bo = ormqr(QR, tau, np.array(B, dtype=A.dtype).reshape(m, -1), True)
    info = diag_info(QR[:n, :n])
    Bo[:n] = solve_upper(QR[:n, :n], Bo[:n])
    return QR, tau, Bo, info


# ------------------------------------------------------------------ yardsticks (np.longdouble, LAPACK's normalisations)
def _norm1(M):
    return np.abs(M).sum(axis=0).max() if M.size else np.longdouble(0)


def qr_ratios(A, Q, R, wide=np.longdouble):
    """(||A - Q R||_1 / (m u ||A||_1),  ||I - Q^T Q||_1 / (m u)) with u the unit roundoff of A's type, evaluated in
    `wide`."""
    u = UNIT[np.dtype(A.dtype)]
    m = A.shape[0]
    Al, Ql, Rl = (np.asarray(x, dtype=wide) for x in (A, Q, R))
    r1 = _norm1(Al - Ql @ Rl) / (m * u * _norm1(Al))
    r2 = _norm1(np.eye(Ql.shape[1], dtype=wide) - Ql.T @ Ql) / (m * u)
    return float(r1), float(r2)


def ls_ratio(A, b, x, wide=np.longdouble):
    """||A^T (b - A x)||_1 / (m u ||A||_1 (||b||_1 + ||A||_1 ||x||_1))."""
    u = UNIT[np.dtype(A.dtype)]
    m = A.shape[0]
    Al = np.asarray(A, dtype=wide)
    bl = np.asarray(b, dtype=wide).reshape(m, -1)
    xl = np.asarray(x, dtype=wide).reshape(A.shape[1], -1)
    an = _norm1(Al)
    return float(_norm1(Al.T @ (bl - Al @ xl)) / (m * u * an * (_norm1(bl) + an * _norm1(xl))))


# the four rounded shapes of the comparison beside LAPACK, and their right-hand sides
ROUNDED = [(129, 129), (300, 129), (600, 384), (1000, 257)]
ROUNDED_NRHS = 3
# ... and, apart from them, the tall shape of the Hadamard plant: two 64-row chunks per slab of the panel kernel, a
# K of 16386 in the TN products of the block apply, 16384 rows under colnrm2
ROUNDED_TALL = [(16514, 130)]


def rounded_case(m, n, dtype):
    A = uniform(m, n, 0, dtype)
    b = uniform(m, ROUNDED_NRHS, 1, dtype)
    return A, b


def tall_wide(dtype):
    """The type the ratios of ROUNDED_TALL are evaluated in: fp64 for fp32 results (29 more bits than the data, and a
    BLAS product instead of seconds of np.longdouble), np.longdouble for fp64 results."""
    return np.float64 if np.dtype(dtype) == np.float32 else np.longdouble


def _triple(A, b, QR, tau, x, wide=np.longdouble):
    n = A.shape[1]
    Q = orgqr(QR, tau, n)
    r1, r2 = qr_ratios(A, Q, np.triu(QR[:n]), wide)
    return r1, r2, ls_ratio(A, b, x, wide)


@functools.lru_cache(maxsize=None)
def model_ratios(m, n, dtype_name, wide=np.longdouble):
    """The three ratios of the numpy model on the rounded case."""
    dtype = np.dtype(dtype_name).type
    A, b = rounded_case(m, n, dtype)
    QR, tau, Bo, _ = gels(A, b)
    return _triple(A, b, QR, tau, Bo[:n], wide)


@functools.lru_cache(maxsize=None)
def lapack_ratios(m, n, dtype_name, wide=np.longdouble):
    """The three ratios of LAPACK (scipy) on the rounded case."""
    from scipy.linalg import lapack

    dtype = np.dtype(dtype_name).type
    p = "d" if dtype == np.float64 else "s"
    A, b = rounded_case(m, n, dtype)
    qr_, tau, _, info = getattr(lapack, p + "geqrf")(A)
    assert info == 0
    Q, _, info = getattr(lapack, p + "orgqr")(qr_[:, :n], tau)
    assert info == 0
    _, x, info = getattr(lapack, p + "gels")(A, b)
    assert info == 0
    r1, r2 = qr_ratios(A, Q, np.triu(qr_[:n]), wide)
    return r1, r2, ls_ratio(A, b, x[:n], wide)
