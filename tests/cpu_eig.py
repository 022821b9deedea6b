"""The two-sided Jacobi eigensolver of linalg_solver_amd/csrc (kernels_eig.hip, syevj_dev in api.hip) written down in
numpy, the input builders of the eigensolver tests, and their yardsticks.

The model follows the kernels in the working precision with fp64 where they have it: W from the upper triangle of A,
mirrored; thr = u ||A||_F from the upper triangle; sweeps of P - 1 rounds in the round-robin order of cpu_svd; all
decisions of a round from W as it stands before the round (a = w_ii, b = w_jj, c = w_ij, the upper element); the rows of
the rotated pairs, rounded once, then the columns of the row-rotated matrix, rounded again, then w_ij = w_ji = 0; rows of
Z like rows of W; w = the diagonal, sorted ascending (stable), V[:, i] the row of Z that belongs to w[i].  It does not
model the order of the norm's sum or the fused multiply-adds, so on rounded inputs it agrees with the GPU to rounding and
may take another number of sweeps; on the diagonal plants nothing is rounded and the model and the GPU must agree bit for
bit, with one sweep and no rotation.
"""
import functools

import numpy as np

import cpu_qr as cq
import cpu_svd as cs
from cpu_svd import rotation, round_pairs

UNIT = cs.UNIT
LAPACK_THRESH = cq.LAPACK_THRESH
MAX_SWEEPS = 60            # the default of "syevj_max_sweeps"
NT = 256                   # threads of a pair's workgroup (EIG_NT)


# ------------------------------------------------------------------ the algorithm
def upper_fro(A):
    """||A||_F of the symmetric matrix given by the upper triangle, the off-diagonal squares counted twice, in fp64."""
    up = np.triu(np.asarray(A).astype(np.float64))
    with np.errstate(all="ignore"):
        return float(np.sqrt(2.0 * (up * up).sum() - (np.diag(up) ** 2).sum()))


def threshold(A):
    return UNIT[np.dtype(A.dtype)] * upper_fro(A)


def syevj(A, jobz=1, max_sweeps=MAX_SWEEPS):
    """dict(w, V, info, sweeps, rotations) of the model; V is None with jobz = 0 and for an input whose upper triangle is
    not finite (w all NaN then).  The strictly lower triangle of A is not looked at."""
    A = np.asarray(A)
    dt = A.dtype
    n = A.shape[0]
    out = dict(w=np.full(n, np.nan), V=None, info=0, sweeps=0, rotations=0)
    W = (np.triu(A) + np.triu(A, 1).T).astype(dt)
    nrm = upper_fro(A)
    if n == 0 or not np.isfinite(nrm):
        return out
    thr = UNIT[np.dtype(dt)] * nrm
    Z = np.eye(n, dtype=dt) if jobz else None
    P = n + (n & 1)
    sweeps = rotations = last = 0
    for sweep in range(1, max_sweeps + 1):
        last = 0
        for r in range(P - 1):
            I, J = round_pairs(n, r)
            if not len(I):
                continue
            a, b, c = (W[I, I].astype(np.float64), W[J, J].astype(np.float64), W[I, J].astype(np.float64))
            rot = np.abs(c) > thr                                  # a NaN fails the comparison
            if not rot.any():
                continue
            cs_, sn = rotation(a[rot], b[rot], c[rot])
            Ir, Jr = I[rot], J[rot]
            wi, wj = W[Ir].astype(np.float64), W[Jr].astype(np.float64)
            W[Ir] = (cs_[:, None] * wi - sn[:, None] * wj).astype(dt)
            W[Jr] = (sn[:, None] * wi + cs_[:, None] * wj).astype(dt)
            ci, cj = W[:, Ir].astype(np.float64), W[:, Jr].astype(np.float64)
            W[:, Ir] = (cs_[None, :] * ci - sn[None, :] * cj).astype(dt)
            W[:, Jr] = (sn[None, :] * ci + cs_[None, :] * cj).astype(dt)
            W[Ir, Jr] = 0
            W[Jr, Ir] = 0
            if Z is not None:
                zi, zj = Z[Ir].astype(np.float64), Z[Jr].astype(np.float64)
                Z[Ir] = (cs_[:, None] * zi - sn[:, None] * zj).astype(dt)
                Z[Jr] = (sn[:, None] * zi + cs_[:, None] * zj).astype(dt)
            last += int(rot.sum())
        sweeps = sweep
        rotations += last
        if last == 0:
            break
    out.update(sweeps=sweeps, rotations=min(rotations, 2 ** 31 - 1), info=1 if last != 0 else 0)
    lam = np.diag(W).astype(np.float64)
    order = np.argsort(lam, kind="stable")
    out["w"] = lam[order]
    if jobz:
        out["V"] = np.ascontiguousarray(Z[order].T)
    return out


# ------------------------------------------------------------------ yardsticks (np.longdouble)
def _norm1(M):
    return np.abs(M).sum(axis=0).max() if M.size else np.longdouble(0)


def lapack_values(A):
    """LAPACK's eigenvalues of the fp64 image of A (upper triangle)."""
    return np.linalg.eigvalsh(np.asarray(A, dtype=np.float64), UPLO="U")


def eig_ratios(A, w, V, w_ref=None):
    """(||A - V diag(w) V^T||_1 / (n u ||A||_1),  ||I - V^T V||_1 / (n u),  max|w - w_ref| / (n u max|w_ref|)), u the unit
    roundoff of A's type, evaluated in np.longdouble.  A is taken as the symmetric matrix its upper triangle gives."""
    wide = np.longdouble
    u = UNIT[np.dtype(A.dtype)]
    n = A.shape[0]
    w_ref = lapack_values(A) if w_ref is None else w_ref
    Al = np.triu(A).astype(wide) + np.triu(A, 1).T.astype(wide)
    Vl, wl = np.asarray(V, dtype=wide), np.asarray(w, dtype=wide)
    r1 = _norm1(Al - (Vl * wl[None, :]) @ Vl.T) / (n * u * max(_norm1(Al), wide(1e-300)))
    r2 = _norm1(np.eye(n, dtype=wide) - Vl.T @ Vl) / (n * u)
    r3 = np.abs(wl - np.asarray(w_ref, dtype=wide)).max() / (n * u * max(np.abs(w_ref).max(), 1e-300))
    return float(r1), float(r2), float(r3)


def lapack_eigh_ratios(A):
    """The three ratios of LAPACK's eigh (through numpy) in the precision of A."""
    w, V = np.linalg.eigh(A, UPLO="U")
    assert V.dtype == A.dtype
    return eig_ratios(A, w.astype(np.float64), V)


# ------------------------------------------------------------------ rounded inputs
# symmetrised U(-1, 1): no pair, one pair, the phantom player, odd and even orders across a 16-byte group boundary,
# padded leading dimensions in fp32, and at 515 -- the smallest odd order with more pairs per round (258) than a
# workgroup has threads (256) -- the second pass of the rotation kernel's loop over column pairs
ROUNDED = [1, 2, 3, 5, 64, 129, 130, 257, 515]
assert 515 // 2 > NT >= 513 // 2


@functools.lru_cache(maxsize=None)
def _rounded64(n):
    M = np.random.default_rng(9000 + n).uniform(-1.0, 1.0, (n, n))
    return (M + M.T) / 2


def rounded(n, dtype=np.float64):
    A = _rounded64(n).astype(dtype)
    return np.triu(A) + np.triu(A, 1).T          # symmetric after the rounding as well


def _freeze(f):
    for v in f.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def model_result(n, dtype_name):
    return _freeze(syevj(rounded(n, np.dtype(dtype_name).type)))


@functools.lru_cache(maxsize=None)
def model_ratios(n, dtype_name):
    f = model_result(n, dtype_name)
    return eig_ratios(rounded(n, np.dtype(dtype_name).type), f["w"], f["V"])


@functools.lru_cache(maxsize=None)
def lapack_ratios(n, dtype_name):
    return lapack_eigh_ratios(rounded(n, np.dtype(dtype_name).type))


@functools.lru_cache(maxsize=None)
def pooled_bounds(dtype_name):
    """Per ratio: twice the largest value the model or LAPACK's eigh attains on any ROUNDED order in that precision
    (pooled as cpu_svd.pooled_bounds; the factor 2 is the project's margin)."""
    rows = [model_ratios(n, dtype_name) for n in ROUNDED] + [lapack_ratios(n, dtype_name) for n in ROUNDED]
    return tuple(2.0 * max(r[i] for r in rows) for i in range(3))


# ------------------------------------------------------------------ special inputs, n = 96
SPECIAL_N = 96
SPECIAL = ["pm_pairs", "repeated", "rank3", "graded", "cycle"]


def special_values(name, n=SPECIAL_N):
    if name == "pm_pairs":                      # +-1 .. +-48: a solver routed through the SVD mixes the two eigenspaces
        k = np.arange(1, n // 2 + 1, dtype=np.float64)
        return np.concatenate([k, -k])
    if name == "repeated":
        return np.repeat([1.0, 2.0, -3.0, 0.0], n // 4)
    if name == "rank3":
        return np.concatenate([[5.0, -2.0, 1.0], np.zeros(n - 3)])
    if name == "graded":
        return 2.0 ** (-np.arange(n) / 2.0)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _special64(name):
    n = SPECIAL_N
    if name == "cycle":                         # adjacency of the n-cycle: a zero diagonal, zeta = 0 at the first rotations
        A = np.zeros((n, n))
        idx = np.arange(n)
        A[idx, (idx + 1) % n] = 1.0
        return A + A.T
    Q = np.linalg.qr(cq.uniform(n, n, 5, np.float64))[0]
    A = (Q * special_values(name)[None, :]) @ Q.T
    return (A + A.T) / 2


def special(name, dtype=np.float64):
    A = _special64(name).astype(dtype)
    return np.triu(A) + np.triu(A, 1).T


@functools.lru_cache(maxsize=None)
def special_model(name, dtype_name):
    return _freeze(syevj(special(name, np.dtype(dtype_name).type)))


@functools.lru_cache(maxsize=None)
def special_model_ratios(name, dtype_name):
    f = special_model(name, dtype_name)
    return eig_ratios(special(name, np.dtype(dtype_name).type), f["w"], f["V"])


@functools.lru_cache(maxsize=None)
def special_lapack_ratios(name, dtype_name):
    return lapack_eigh_ratios(special(name, np.dtype(dtype_name).type))


@functools.lru_cache(maxsize=None)
def special_bounds(name, dtype_name):
    """Per ratio: twice the larger of the model's and LAPACK's value on that input."""
    a, b = special_model_ratios(name, dtype_name), special_lapack_ratios(name, dtype_name)
    return tuple(2.0 * max(x, y) for x, y in zip(a, b))


def vectors_through_svd(A):
    """(w, V) the way a solver routed through the SVD would form them: V from cpu_svd.gesvdj, w_i = v_i^T A v_i.  Right
    for a definite matrix; where +l and -l are both eigenvalues the SVD cannot tell their eigenspaces apart."""
    f = cs.gesvdj(A)
    V = np.ascontiguousarray(f["Vt"].T)
    w = np.einsum("ij,ij->j", V.astype(np.float64), A.astype(np.float64) @ V.astype(np.float64))
    order = np.argsort(w, kind="stable")
    return w[order], np.ascontiguousarray(V[:, order])


# ------------------------------------------------------------------ exact plants
PLANT_N = [7, 130]


@functools.lru_cache(maxsize=None)
def _plant_diag(n):
    """n distinct values: n - 1 of the 130 numbers +-3 * 2^k, -32 <= k <= 32, and a zero, in scrambled order."""
    rng = np.random.default_rng(40 + n)
    k = np.arange(-32, 33)
    pool = np.concatenate([3.0 * np.ldexp(1.0, k), -3.0 * np.ldexp(1.0, k)])
    d = np.concatenate([pool[rng.permutation(len(pool))[:n - 1]], [0.0]])[rng.permutation(n)]
    assert len(set(d.tolist())) == n and (d < 0).any() and (d > 0).any() and (d == 0).any()
    return d


def plant_diagonal(n, dtype=np.float64):
    """(A, w, V): a diagonal matrix with distinct entries, its sorted diagonal, and the permutation matrix of the sort.
    One sweep, no rotation; nothing is rounded."""
    d = _plant_diag(n)
    order = np.argsort(d, kind="stable")
    return np.diag(d).astype(dtype), d[order].copy(), np.eye(n)[:, order].astype(dtype)


def plant_threshold(n, dtype=np.float64):
    """(A, above): the diagonal plant with off-diagonal entries planted at disjoint pairs i < j of the upper triangle
    (mirrored): 2 thr at the pairs `above`, thr / 2 at about as many others, thr the threshold of the diagonal plant.  The
    planted entries are 2^-22 of the norm or less, so they move the norm, and with it the threshold, by a relative 2^-40
    at most, and the summation order by less.  No index belongs to two planted pairs, so a rotation -- by whatever
    angle -- mixes only zeros into its rows and columns: exactly len(above) rotations are counted in a first sweep."""
    A, _, _ = plant_diagonal(n, dtype)
    A = A.copy()
    thr = threshold(A)
    idx = np.random.default_rng(70 + n).permutation(n)
    pairs = [tuple(sorted(map(int, idx[2 * t:2 * t + 2]))) for t in range(min(n // 2, 40))]
    above, below = pairs[::2], pairs[1::2]
    for sel, f in ((above, 2.0), (below, 0.5)):
        for i, j in sel:
            A[i, j] = A[j, i] = f * thr
    return A, sorted(above)
