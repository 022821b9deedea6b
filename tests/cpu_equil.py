"""CPU statement of equilibration and the expert driver (lsx_geequ_*, lsx_laqge_*, lsx_gesvx_*): LAPACK's geequ,
laqge and the steps of gesvx in numpy, built on cpu_refine.gerfs_twin and cpu_cond.rcond_twin.  All arithmetic runs
in the working precision of the input (fp64 or fp32): maxima, products and one division per scale factor, so the
results have LAPACK's bits (tests/test_equil_host.py proves that before the GPU is asked anything).

Also the inputs of the tests, one builder per outcome of laqge:
    "both"  cpu_refine.scaled_system: columns 2^-30 .. 2^30, every third row 2^-20           -> BOTH
    "row"   uniform(-1, 1) rows times 2^integers(-40, 41), a plain solution                   -> ROW (colcnd ~ 0.9)
    "col"   the same on the columns, the solution divided by the scales                       -> COL, or BOTH where
            one column dominates a row by less than a tenth of what it does in another (common for small n): seed_for
            picks a seed with the outcome the builder is named after
    "none"  gen.U11 systems                                                                    -> NONE
"""
from __future__ import annotations

import numpy as np

import cpu_cond
import cpu_refine as cr

NONE, ROW, COL, BOTH = 0, 1, 2, 3
EQUED_OF_LAPACK = {b"N": NONE, b"R": ROW, b"C": COL, b"B": BOTH}
THRESH = 0.1
PREC = {np.dtype(np.float64): 2.0 ** -52, np.dtype(np.float32): 2.0 ** -23}      # LAPACK's lamch('P')
KINDS = ("both", "row", "col", "none")
EXPECTED = {"both": BOTH, "row": ROW, "col": COL, "none": NONE}


def _rhs(A, rng, nrhs, scale):
    """Solutions uniform(-1, 1) * scale and their right-hand sides; nrhs=None gives vectors."""
    n = A.shape[0]
    k = 1 if nrhs is None else nrhs
    XT = np.empty((n, k))
    B = np.empty((n, k))
    for j in range(k):
        XT[:, j] = rng.uniform(-1, 1, n) * scale
        B[:, j] = A @ XT[:, j]
    return (A, B[:, 0], XT[:, 0]) if nrhs is None else (A, B, XT)


def row_scaled(n: int, seed: int, nrhs=None):
    rng = np.random.default_rng(seed)
    M = rng.uniform(-1, 1, (n, n))
    d = 2.0 ** rng.integers(-40, 41, n)
    return _rhs(M * d[:, None], rng, nrhs, 1.0)


def col_scaled(n: int, seed: int, nrhs=None):
    rng = np.random.default_rng(seed)
    M = rng.uniform(-1, 1, (n, n))
    d = 2.0 ** rng.integers(-40, 41, n)
    return _rhs(M * d[None, :], rng, nrhs, 1.0 / d)


def unit_scaled(n: int, seed: int, nrhs=None):
    from linalg_solver_amd import gen

    A = gen.system(gen.U11, seed, n)[0]
    return _rhs(A, np.random.default_rng(seed), nrhs, 1.0)


def system(kind: str, n: int, seed: int, nrhs=None):
    """(A, B, XT) of one builder, fp64."""
    if kind == "both":
        return cr.scaled_system(n, seed, nrhs)
    return {"row": row_scaled, "col": col_scaled, "none": unit_scaled}[kind](n, seed, nrhs)


_seed = {}


def seed_for(kind: str, n: int, start: int = 0) -> int:
    """The first seed from `start` on at which the builder's fp64 matrix gets the outcome it is named after from the
    twin (which test_equil_host.py holds to LAPACK's); orders below 33 are too small to force one: `start`."""
    key = (kind, n, start)
    if key not in _seed:
        seed = start
        while n >= 33:
            A = system(kind, n, seed)[0]
            r, c, rowcnd, colcnd, amax, info = geequ_twin(A)
            if info == 0 and laqge_decide(rowcnd, colcnd, amax, A.dtype) == EXPECTED[kind]:
                break
            seed += 1
        _seed[key] = seed
    return _seed[key]


def limits(dtype):
    """(smlnum, bignum) of geequ and (small, large) of laqge, as scalars of the working precision."""
    dt = np.dtype(dtype).type
    sml = dt(cr.SAFMIN[np.dtype(dtype)])
    small = dt(cr.SAFMIN[np.dtype(dtype)] / PREC[np.dtype(dtype)])
    return sml, dt(1) / sml, small, dt(1) / small


def _scale_of(v, sml, big):
    with np.errstate(invalid="ignore"):
        t = np.where(v > sml, v, sml)
        t = np.where(t < big, t, big)
    return (v.dtype.type(1) / t).astype(v.dtype)


def geequ_twin(A):
    """dgeequ.f / sgeequ.f: (r, c, rowcnd, colcnd, amax, info).  With info != 0 the ratios that were not reached are
    0 and r / c are not to be used; a NaN entry gives amax = NaN."""
    dt = A.dtype.type
    m, n = A.shape
    sml, big, _, _ = limits(A.dtype)
    r, c = np.ones(m, dtype=A.dtype), np.ones(n, dtype=A.dtype)
    if m == 0 or n == 0:
        return r, c, 1.0, 1.0, 0.0, 0
    absA = np.abs(A)
    rmax = np.max(absA, axis=1)
    amax = float(np.max(rmax))                       # numpy's max hands a NaN on
    rcmin, rcmax = min(big, np.fmin.reduce(rmax)), np.max(rmax)
    r = _scale_of(rmax, sml, big)
    if rcmin == 0:
        return r, c, 0.0, 0.0, amax, int(np.argmax(rmax == 0)) + 1
    rowcnd = float(max(rcmin, sml) / min(rcmax, big))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        cmax = np.max((absA * r[:, None]).astype(A.dtype), axis=0)
    rcmin, rcmax = min(big, np.fmin.reduce(cmax)), np.max(cmax)
    c = _scale_of(cmax, sml, big)
    if rcmin == 0:
        return r, c, rowcnd, 0.0, amax, m + int(np.argmax(cmax == 0)) + 1
    return r, c, rowcnd, float(max(dt(rcmin), sml) / min(dt(rcmax), big)), amax, 0


def laqge_decide(rowcnd, colcnd, amax, dtype) -> int:
    _, _, small, large = limits(dtype)
    rows = not (rowcnd >= THRESH and small <= amax <= large)
    cols = not (colcnd >= THRESH)
    return (ROW if rows else 0) | (COL if cols else 0)


def laqge_twin(A, r, c, rowcnd, colcnd, amax):
    """dlaqge.f: (equed, scaled matrix); both sides: (c_j * r_i) * a_ij, in that association."""
    equed = laqge_decide(rowcnd, colcnd, amax, A.dtype)
    with np.errstate(over="ignore", under="ignore"):
        if equed == ROW:
            S = r[:, None] * A
        elif equed == COL:
            S = c[None, :] * A
        elif equed == BOTH:
            S = (c[None, :] * r[:, None]) * A
        else:
            S = A.copy()
    return equed, S.astype(A.dtype)


def max_abs(M) -> float:
    return float(np.max(np.abs(M))) if M.size else 0.0


def gesvx_twin(A, B, trans=False, equil=True):
    """dgesvx.f step for step (fact = 'E' / 'N') for a matrix B of right-hand sides (n x nrhs, nrhs may be 0), all in
    the working precision of A.  Returns a dict: equed, r, c, rowcnd, colcnd, amax, geequ_info, Aeq, Beq, lu, piv,
    rpvgrw, rcond, X (None when the factorisation broke down), ferr, ferr_undivided, berr, info."""
    from scipy.linalg import get_lapack_funcs, lu_solve

    dt = A.dtype
    n, nrhs = A.shape[0], B.shape[1]
    out = dict(equed=NONE, r=np.ones(n, dtype=dt), c=np.ones(n, dtype=dt), rowcnd=1.0, colcnd=1.0, amax=0.0, geequ_info=0,
               Aeq=A.copy(), Beq=B.copy(), lu=None, piv=None, rpvgrw=1.0, rcond=1.0, X=None, ferr=np.zeros(nrhs),
               ferr_undivided=np.zeros(nrhs), berr=np.zeros(nrhs), info=0)
    if n == 0:
        out["X"] = B.copy()
        return out
    if equil:
        r, c, rowcnd, colcnd, amax, ginfo = geequ_twin(A)
        out.update(amax=amax, geequ_info=ginfo)
        if ginfo == 0:
            out.update(r=r, c=c)
        if ginfo == 0 and amax == amax:
            out.update(rowcnd=rowcnd, colcnd=colcnd)
            out["equed"], out["Aeq"] = laqge_twin(A, r, c, rowcnd, colcnd, amax)
    equed, Aeq = out["equed"], out["Aeq"]
    rowequ, colequ = bool(equed & ROW), bool(equed & COL)
    if not trans and rowequ:
        out["Beq"] = (out["r"][:, None] * B).astype(dt)
    if trans and colequ:
        out["Beq"] = (out["c"][:, None] * B).astype(dt)
    Beq = out["Beq"]
    getrf, = get_lapack_funcs(("getrf",), (Aeq,))
    lu, piv, info = getrf(Aeq)
    lu = np.ascontiguousarray(lu)
    out.update(lu=lu, piv=piv, info=int(info))
    k = info if info > 0 else n
    umax = max_abs(np.triu(lu[:k, :k]))
    out["rpvgrw"] = 1.0 if umax == 0 else float(dt.type(max_abs(Aeq[:, :k])) / dt.type(umax))
    if info > 0:
        out.update(rcond=0.0, ferr=np.full(nrhs, np.inf), ferr_undivided=np.full(nrhs, np.inf), berr=np.full(nrhs, np.inf))
        return out
    anorm = float(np.linalg.norm(Aeq.astype(np.float64), np.inf if trans else 1))
    out["rcond"] = cpu_cond.rcond_twin(lu, anorm, "I" if trans else "1")
    X = np.empty((n, nrhs), dtype=dt)
    for j in range(nrhs):
        x0 = lu_solve((lu, piv), Beq[:, j], trans=1 if trans else 0).astype(dt)
        X[:, j], out["ferr_undivided"][j], out["berr"][j] = cr.gerfs_twin(Aeq, (lu, piv), Beq[:, j], x0, trans)
    out["ferr"] = out["ferr_undivided"].copy()
    if not trans and colequ:
        X = (out["c"][:, None] * X).astype(dt)
        out["ferr"] /= out["colcnd"]
    elif trans and rowequ:
        X = (out["r"][:, None] * X).astype(dt)
        out["ferr"] /= out["rowcnd"]
    out["X"] = X
    if out["rcond"] < cr.unit(dt):
        out["info"] = n + 1
    return out


def lacn2_endpoints(Aeq, trans=False):
    """Every rcond the estimator can return for A_eq of order 1 or 2, from the fp64 inverse: lacn2's estimate is the
    1-norm of the column of the inverse it ends on (ties, and the sign of a component that is zero but for rounding,
    decide which), or the alternating vector's estimate if that is larger -- and gecon solves with L U alone, whose
    inverse has the columns of inv(A) in the order the interchanges left them, so that vector meets them in either
    order.  For the orders at which two correct runs of the iteration can end differently."""
    from itertools import permutations

    A64 = Aeq.astype(np.float64)
    n = A64.shape[0]
    assert n <= 2
    M = np.linalg.inv(A64).T if trans else np.linalg.inv(A64)     # the infinity-norm is the 1-norm of the transpose
    anorm = float(np.linalg.norm(A64, np.inf if trans else 1))
    cols = np.abs(M).sum(axis=0)
    alts = [0.0]
    if n > 1:
        v = np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * (1.0 + np.arange(n) / (n - 1.0))
        alts = [2.0 * float(np.abs(M[:, list(p)] @ v).sum()) / (3.0 * n) for p in permutations(range(n))]
    return sorted({1.0 / (anorm * max(float(cj), alt)) for cj in cols for alt in alts})


# ---- planted inputs: each decides one branch of geequ / laqge exactly (every entry a power of two)
def planted_rows(n, lo_exp, dtype=np.float64):
    """Row maxima 1 and 2^lo_exp (odd rows), columns alike: rowcnd = 2^lo_exp exactly, colcnd = 1."""
    A = np.ones((n, n), dtype=dtype)
    A[1::2] *= dtype(2.0 ** lo_exp)
    return A


def planted_cols(n, lo_exp, dtype=np.float64):
    return np.ascontiguousarray(planted_rows(n, lo_exp, dtype).T)


def planted_tiny(n, dtype=np.float64):
    """Well scaled (entries +-1 and +-1/2 times one power of two) but of magnitude 2^-980 (fp32: 2^-110), below
    laqge's small: rows are scaled although rowcnd = 1."""
    e = -980 if np.dtype(dtype) == np.float64 else -110
    rng = np.random.default_rng(n)
    A = rng.choice(np.array([1.0, -1.0, 0.5, -0.5]), (n, n))
    A[np.arange(n), np.arange(n)] = 1.0                  # every row and column has an entry of the full magnitude
    return (A * 2.0 ** e).astype(dtype)
