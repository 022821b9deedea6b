"""The one-sided Jacobi SVD of linalg_solver_amd/csrc (kernels_svd.hip, gesvdj_run / gelss_dev in api.hip) written down
in numpy, the input builders of the SVD tests, and their yardsticks.

The model follows the kernels in the working precision with fp64 where they have it: W = A (m <= n) or the R of
cpu_qr.geqrf (m > n); sweeps of P - 1 rounds in the round-robin order; per pair the three sums, the decision and the
rotation in fp64, every stored element rounded once; Z alike; s_i = ||w_i||_2 in fp64, the stable descending sort,
V^T = w / s, U = Z^T or cpu_qr.ormqr(Q, [Z^T; 0]).  A matrix whose row norms are not finite is not iterated on.  It does
not model the order of summation or the fused multiply-adds, so on rounded inputs it agrees with the GPU to rounding and
may take another number of sweeps; on the planted inputs below every sum is exact and the model and the GPU must agree
bit for bit, with one sweep and no rotation.

The pairs of a round are disjoint, so the model rotates all of them at once.
"""
import functools

import numpy as np

import cpu_chol as cc
import cpu_qr as cq

UNIT = cc.UNIT
LAPACK_THRESH = cq.LAPACK_THRESH
MAX_SWEEPS = 30


# ------------------------------------------------------------------ the pair order
def round_pairs(p, r):
    """(I, J): the pairs i < j of round r among p rows.  Closed form: position 0 holds player 0, position s >= 1 player
    ((s - 1 - r) mod (P - 1)) + 1 with P = p + (p & 1); position t meets position P - 1 - t; the phantom is skipped."""
    P = p + (p & 1)
    pos = np.arange(P)
    player = np.where(pos == 0, 0, (pos - 1 - r) % max(P - 1, 1) + 1)
    t = np.arange(P // 2)
    a, b = player[t], player[P - 1 - t]
    i, j = np.minimum(a, b), np.maximum(a, b)
    keep = j < p
    return i[keep], j[keep]


def round_pairs_by_rotation(p, r):
    """The same round from the list rotation the closed form abbreviates: player 0 stays, the others move one seat per
    round; the list is folded in the middle."""
    P = p + (p & 1)
    seats = [0] + list(np.roll(np.arange(1, P), r))
    out = []
    for t in range(P // 2):
        i, j = sorted((seats[t], seats[P - 1 - t]))
        if j < p:
            out.append((int(i), int(j)))
    return out


# ------------------------------------------------------------------ the algorithm
def row_norms(W):
    w = W.astype(np.float64)
    with np.errstate(all="ignore"):
        return np.sqrt((w * w).sum(axis=1))


def rotation(a, b, c):
    """(cs, sn) of the pairs with sums a, b, c (arrays), all fp64."""
    with np.errstate(all="ignore"):
        zeta = (b - a) / (2.0 * c)
        az = np.abs(zeta)
        sgn = np.where(zeta < 0, -1.0, 1.0)
        t = np.where(az > 2.0 ** 500, 1.0 / (2.0 * zeta), sgn / (az + np.sqrt(1.0 + zeta * zeta)))
        cs = 1.0 / np.sqrt(1.0 + t * t)
    return cs, cs * t


def jacobi(W, Z=None, max_sweeps=MAX_SWEEPS, drop=None):
    """The sweeps on W (p x q) and Z (p x p or None), in place.  Returns (sweeps, rotations, last): last = rotations of the
    last sweep.  drop = (lo, hi): columns [lo, hi) are left out of the three sums -- only for showing that an input tells
    a complete sum from one that misses a chunk."""
    dt = W.dtype
    p, q = W.shape
    tol = np.sqrt(float(q)) * UNIT[np.dtype(dt)]
    P = p + (p & 1)
    sweeps = rotations = last = 0
    for sweep in range(1, max_sweeps + 1):
        last = 0
        for r in range(P - 1):
            I, J = round_pairs(p, r)
            if not len(I):
                continue
            wi, wj = W[I].astype(np.float64), W[J].astype(np.float64)
            si, sj = wi, wj
            if drop is not None:
                si, sj = wi.copy(), wj.copy()
                si[:, drop[0]:drop[1]] = 0
                sj[:, drop[0]:drop[1]] = 0
            with np.errstate(all="ignore"):
                a, b, c = (si * si).sum(axis=1), (sj * sj).sum(axis=1), (si * sj).sum(axis=1)
                rot = np.abs(c) > tol * np.sqrt(a) * np.sqrt(b)      # a NaN fails the comparison
            if not rot.any():
                continue
            cs, sn = rotation(a[rot], b[rot], c[rot])
            cs, sn = cs[:, None], sn[:, None]
            Ir, Jr = I[rot], J[rot]
            W[Ir] = (cs * wi[rot] - sn * wj[rot]).astype(dt)
            W[Jr] = (sn * wi[rot] + cs * wj[rot]).astype(dt)
            if Z is not None:
                zi, zj = Z[Ir].astype(np.float64), Z[Jr].astype(np.float64)
                Z[Ir] = (cs * zi - sn * zj).astype(dt)
                Z[Jr] = (sn * zi + cs * zj).astype(dt)
            last += int(rot.sum())
        sweeps = sweep
        rotations += last
        if last == 0:
            break
    return sweeps, rotations, last


def gesvdj(A, jobz=1, max_sweeps=MAX_SWEEPS, drop=None):
    """dict(U, s, Vt, info, sweeps, rotations) of the model; U and Vt are None with jobz = 0 and for an input that is not
    finite (s all NaN then)."""
    A = np.asarray(A)
    dt = A.dtype
    m, n = A.shape
    k = min(m, n)
    if m > n:
        QR, tau = cq.geqrf(A)
        W = np.triu(QR[:n]).copy()
    else:
        W = np.array(A, copy=True)
    Z = np.eye(k, dtype=dt) if jobz else None
    out = dict(U=None, s=np.full(k, np.nan), Vt=None, info=0, sweeps=0, rotations=0)
    if k == 0 or not np.all(np.isfinite(row_norms(W))):
        return out
    sweeps, rotations, last = jacobi(W, Z, max_sweeps, drop)
    out.update(sweeps=sweeps, rotations=min(rotations, 2 ** 31 - 1))
    sig = row_norms(W)
    if not np.all(np.isfinite(sig)):
        return out
    out["info"] = 1 if last != 0 else 0
    order = np.argsort(-sig, kind="stable")
    out["s"] = sig[order]
    if jobz:
        with np.errstate(all="ignore"):
            Vt = np.where(sig[:, None] == 0, 0.0, W.astype(np.float64) / sig[:, None]).astype(dt)
        out["Vt"] = Vt[order]
        U = np.zeros((m, k), dtype=dt)
        U[:k] = Z[order].T
        out["U"] = cq.ormqr(QR, tau, U, trans=False) if m > n else U
    return out


def default_rcond(m, n, dtype):
    return max(m, n) * UNIT[np.dtype(dtype)]


def gelss(A, B, rcond=-1.0):
    """dict(x, rank, s, info): X = V diag(1 / s_i, i < rank) U^T B in the working precision."""
    A = np.asarray(A)
    dt = A.dtype
    m, n = A.shape
    B = np.asarray(B, dtype=dt).reshape(m, -1)
    f = gesvdj(A)
    s = f["s"]
    if np.isnan(s).any():
        return dict(x=np.full((n, B.shape[1]), np.nan, dtype=dt), rank=0, s=s, info=0)
    thr = (default_rcond(m, n, dt) if rcond < 0 else rcond) * s[0]
    rank = int(np.sum(s > thr))
    Y = f["U"].T @ B
    with np.errstate(all="ignore"):
        Y[:rank] = (Y[:rank].astype(np.float64) * (1.0 / s[:rank, None])).astype(dt)
    Y[rank:] = 0
    return dict(x=f["Vt"].T @ Y, rank=rank, s=s, info=f["info"])


# ------------------------------------------------------------------ yardsticks (np.longdouble)
def _norm1(M):
    return np.abs(M).sum(axis=0).max() if M.size else np.longdouble(0)


def lapack_values(A):
    """LAPACK's singular values of A in fp64."""
    return np.linalg.svd(np.asarray(A, dtype=np.float64), compute_uv=False)


def svd_ratios(A, U, s, Vt, s_ref=None):
    """(||A - U diag(s) V^T||_1 / (max(m, n) u ||A||_1),  ||I - U^T U||_1 / (m u),  ||I - V^T V^T^T||_1 / (n u),
    max|s - s_ref| / (k u s_ref[0])), u the unit roundoff of A's type, evaluated in np.longdouble."""
    wide = np.longdouble
    u = UNIT[np.dtype(A.dtype)]
    m, n = A.shape
    k = min(m, n)
    s_ref = lapack_values(A) if s_ref is None else s_ref
    Al, Ul, Vl = (np.asarray(x, dtype=wide) for x in (A, U, Vt))
    sl = np.asarray(s, dtype=wide)
    r1 = _norm1(Al - (Ul * sl[None, :]) @ Vl) / (max(m, n) * u * _norm1(Al))
    r2 = _norm1(np.eye(k, dtype=wide) - Ul.T @ Ul) / (m * u)
    r3 = _norm1(np.eye(k, dtype=wide) - Vl @ Vl.T) / (n * u)
    r4 = np.abs(sl - np.asarray(s_ref, dtype=wide)).max() / (k * u * s_ref[0])
    return float(r1), float(r2), float(r3), float(r4)


# rounded U(-1, 1) inputs: odd and even p, the phantom player, wide inputs, tall inputs through a two-block QR
ROUNDED = [(1, 1), (2, 2), (3, 3), (5, 7), (7, 5), (129, 129), (5, 300), (300, 129), (130, 257)]


def rounded(m, n, dtype):
    return cq.uniform(m, n, 0, dtype)


@functools.lru_cache(maxsize=None)
def model_result(m, n, dtype_name):
    f = gesvdj(rounded(m, n, np.dtype(dtype_name).type))
    for v in f.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def model_ratios(m, n, dtype_name):
    f = model_result(m, n, dtype_name)
    return svd_ratios(rounded(m, n, np.dtype(dtype_name).type), f["U"], f["s"], f["Vt"])


@functools.lru_cache(maxsize=None)
def lapack_ratios(m, n, dtype_name):
    """The four ratios of LAPACK's gesdd (through numpy) in the same precision."""
    A = rounded(m, n, np.dtype(dtype_name).type)
    U, s, Vt = np.linalg.svd(A, full_matrices=False)
    assert U.dtype == A.dtype
    return svd_ratios(A, U, s, Vt)


@functools.lru_cache(maxsize=None)
def pooled_bounds(dtype_name):
    """Per ratio: twice the largest value the model or LAPACK attains on any ROUNDED shape in that precision (pooled,
    because single-shape ratios of 0.01 carry no headroom; the factor 2 is the project's margin for QR)."""
    rows = [model_ratios(m, n, dtype_name) for m, n in ROUNDED] + [lapack_ratios(m, n, dtype_name) for m, n in ROUNDED]
    return tuple(2.0 * max(r[i] for r in rows) for i in range(4))


# ------------------------------------------------------------------ exact plants
# (a) permuted, scaled unit rows with a zero row and negative entries: A[i, col[i]] = d[i].  No two rows share a column,
# so every c is exactly zero: one sweep, no rotation, s = the sorted |d|, V^T rows +-e_col, U a permutation, and
# U diag(s) V^T == A bit for bit.  The tall shape is the transpose pattern: geqrf on columns with one non-zero each is
# exact (cpu_qr: reflectors e_j +- e_k).
UNIT_ROWS_D = np.array([3 * 2.0 ** 2, -5 * 2.0 ** -1, 0.0, 7 * 2.0 ** 3, -1.0, 3 * 2.0 ** -4])
UNIT_ROWS_D_POW2 = np.array([2.0 ** 2, -2.0 ** -1, 0.0, 2.0 ** 3, -1.0, 2.0 ** -4])
UNIT_ROWS_COL = np.array([4, 0, 7, 8, 2, 5])


def unit_rows(tall=False, pow2=False, dtype=np.float64):
    """6 x 9 (or its 9 x 6 transpose pattern): returns (A, s) with s the expected values."""
    d = UNIT_ROWS_D_POW2 if pow2 else UNIT_ROWS_D
    A = np.zeros((6, 9), dtype=dtype)
    A[np.arange(6), UNIT_ROWS_COL] = d
    if tall:
        A = np.ascontiguousarray(A.T)
    return A, np.sort(np.abs(d))[::-1].copy()


def unit_rows_rhs(tall=False, nrhs=3, dtype=np.float64):
    """(B, X) for the powers-of-two variant: integer B, X = pinv(A) B exactly (divisions by powers of two)."""
    A, _ = unit_rows(tall, True, np.float64)
    m, n = A.shape
    B = np.random.default_rng(77 + m).integers(-3, 4, (m, nrhs)).astype(np.float64)
    P = np.zeros((n, m))
    nz = A != 0
    P.T[nz] = 1.0 / A[nz]
    return B.astype(dtype), (P @ B).astype(dtype)


# (b) rows of a Sylvester-Hadamard matrix scaled by powers of two, followed by zero columns.  Every c is a sum of N terms
# +-d_i d_j that cancel exactly, so a dropped or doubled chunk of a row shows up as a rotation.  s_i = sqrt(N) |d_i|,
# V^T rows = sign(d_i) H_i / sqrt(N), U the permutation of the stable sort.
# (rows, q, cols, row stride): N = 4^q, rows i * stride of H.
#   130 x 257: rows 0 .. 129 of the order-256 matrix and one zero column (an odd width, one group short of a full pass).
#   6 x 4096: 2048 fp64 groups of 16 bytes = exactly the longest row the round kernel keeps in registers (8 passes of its
#     load loop; fp32: 4 passes), no padding.
#   6 x 16387: longer than the register form holds in either precision, so the round kernel reads the rows again (its
#     sum loop and its rotation loop run 33 / 17 times), with 3 zero columns and a padded leading dimension.
# The rows i * N / 8 differ in high bits only: leaving an aligned chunk of up to N / 8 columns out of the sums leaves
# c != 0 for some pair (tests/test_svd_host.py proves it of the model).
HADAMARD = [(130, 4, 257, 1), (6, 6, 4096, 512), (6, 7, 16387, 2048)]


@functools.lru_cache(maxsize=None)
def _hadamard_rows(rows, q, cols, stride):
    N = 4 ** q
    H = cq.hadamard_columns(q, np.arange(rows) * stride).T          # symmetric: rows = columns
    e = np.random.default_rng(5 * rows + q).integers(-8, 9, rows)
    sgn = np.random.default_rng(7 * rows + q).choice(np.array([-1.0, 1.0]), rows)
    d = sgn * np.ldexp(1.0, e)
    A = np.zeros((rows, cols))
    A[:, :N] = H * d[:, None]
    return A, H, d


def hadamard_rows(rows, q, cols, stride, dtype=np.float64):
    """(A, U, s, Vt): the plant and its exact decomposition."""
    A, H, d = _hadamard_rows(rows, q, cols, stride)
    N = 4 ** q
    order = np.argsort(-np.abs(d), kind="stable")
    s = np.ldexp(np.abs(d), q)[order]
    Vt = np.zeros((rows, cols))
    Vt[:, :N] = np.ldexp(H * np.sign(d)[:, None], -q)
    U = np.eye(rows)[:, order]
    return A.astype(dtype), U.astype(dtype), s, Vt[order].astype(dtype)


def hadamard_doubled(dtype=np.float64):
    """(A, s): 6 x 8192, the 6 x 4096 plant twice side by side -- the longest fp32 row the round kernel keeps in registers
    (all 8 passes of its loops; fp64: 4096 groups, re-read).  The rows stay exactly orthogonal, so one sweep and no
    rotation are still exact statements; s_i = sqrt(8192) |d_i| is not a power of two and is compared to rounding."""
    rows, q, cols, stride = HADAMARD[1]
    A, _, d = _hadamard_rows(rows, q, cols, stride)
    return np.hstack([A, A]).astype(dtype), np.sort(np.sqrt(8192.0) * np.abs(d))[::-1]


# ------------------------------------------------------------------ rank and minimum norm
RANK_SHAPES = [(40, 60), (60, 40)]
RANK = 7


@functools.lru_cache(maxsize=None)
def _rank_product(m, n):
    rng = np.random.default_rng(1000 * m + n)
    while True:
        B = rng.integers(-3, 4, (m, RANK))
        C = rng.integers(-3, 4, (RANK, n))
        if np.linalg.matrix_rank(B) == RANK and np.linalg.matrix_rank(C) == RANK:
            break
    b = rng.integers(-3, 4, (m, 2))
    return B, C, b


def rank_product(m, n, dtype=np.float64):
    """(A, b, x): A = B C of rank 7 with integer factors in [-3, 3], integer b (m x 2), and the minimum-norm solution
    x = C^T (C C^T)^-1 (B^T B)^-1 B^T b formed in np.longdouble."""
    B, C, b = _rank_product(m, n)
    wide = np.longdouble
    Bl, Cl, bl = B.astype(wide), C.astype(wide), b.astype(wide)
    x = Cl.T @ _solve_wide(Cl @ Cl.T, _solve_wide(Bl.T @ Bl, Bl.T @ bl))
    return (B @ C).astype(dtype), b.astype(dtype), x


def _solve_wide(M, R):
    """M^-1 R for a small SPD M by Gauss-Jordan in np.longdouble (numpy's solvers stop at fp64)."""
    M = np.array(M, dtype=np.longdouble)
    R = np.array(R, dtype=np.longdouble)
    n = M.shape[0]
    for j in range(n):
        piv = j + int(np.argmax(np.abs(M[j:, j])))
        M[[j, piv]] = M[[piv, j]]
        R[[j, piv]] = R[[piv, j]]
        R[j] = R[j] / M[j, j]
        M[j] = M[j] / M[j, j]
        for i in range(n):
            if i != j:
                R[i] = R[i] - M[i, j] * R[j]
                M[i] = M[i] - M[i, j] * M[j]
    return R


def wide_case(dtype=np.float64):
    """(A, b, x) at 5 x 300: rounded U(-1, 1), x = A^T (A A^T)^-1 b in np.longdouble."""
    A = rounded(5, 300, dtype)
    b = cq.uniform(5, 2, 3, dtype)
    Al, bl = A.astype(np.longdouble), b.astype(np.longdouble)
    return A, b, Al.T @ _solve_wide(Al @ Al.T, bl)


def rel_err(x, x_ref):
    x_ref = np.asarray(x_ref, dtype=np.longdouble)
    return float(np.abs(np.asarray(x, dtype=np.longdouble) - x_ref).max() / np.abs(x_ref).max())


def pinv_residuals(A, X):
    """The four Moore-Penrose residuals (max norm, relative), in np.longdouble: A X A - A, X A X - X, and the asymmetry of
    A X and of X A."""
    Al, Xl = np.asarray(A, dtype=np.longdouble), np.asarray(X, dtype=np.longdouble)
    AX, XA = Al @ Xl, Xl @ Al
    amax, xmax = np.abs(Al).max(), np.abs(Xl).max()
    return (float(np.abs(AX @ Al - Al).max() / amax), float(np.abs(XA @ Xl - Xl).max() / xmax),
            float(np.abs(AX - AX.T).max()), float(np.abs(XA - XA.T).max()))


# ------------------------------------------------------------------ graded input
GRADED = (96, 64)


def graded_values(n=GRADED[1]):
    return 2.0 ** (-np.arange(n) / 2.0)


def graded(dtype=np.float64):
    """96 x 64, Q1 diag(2^(-i / 2)) Q2 with orthonormal factors from QR of rounded matrices: sigma_i = 2^(-i / 2), a
    condition number of 3e9.  Tall on purpose: the iteration then runs on the R of a QR, which the model finishes in 10
    to 11 sweeps; the square 64 x 64 matrix of the same values takes it 21 to 23 (rows of equal norm, no QR in front),
    too close to the cap of 30 for a test that must not depend on the summation order."""
    m, n = GRADED
    Q1 = np.linalg.qr(cq.uniform(m, m, 13, np.float64))[0][:, :n]
    Q2 = np.linalg.qr(cq.uniform(n, n, 12, np.float64))[0]
    return ((Q1 * graded_values(n)[None, :]) @ Q2).astype(dtype)
