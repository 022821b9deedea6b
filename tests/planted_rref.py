"""Planted echelon forms: rectangular matrices whose row reduction is known without running anything (TESTS ONLY).
The construction is that of tests/planted.py, with an echelon factor in the place of U.

planted_echelon(m, n, r, seed, pivots=..., identity_perm=False) returns A, L, E, S, perm with A[perm] == L @ E exactly:

  S    the r pivot columns, sorted ("random", "tail": packed at the right end, "blocks": only columns of every
       second 128-column block and columns 0..2, so that whole blocks hold no pivot, or a given column set);
  E    r x n echelon: E[i, S[i]] in {+-4, +-8}, zero left of it, integers in [-3, 3] right of it -- in later pivot
       columns with probability min(1, 16 / max(m, n)) (E[:, S] stays well conditioned), in the other columns with
       probability 1/2 (the values that are checked are not mostly zero);
  L    m x r unit lower trapezoidal, a strictly lower entry non-zero with probability min(1, 16 / max(m, n)) (or
       `ldens`: a tall matrix of few columns would otherwise be nearly empty), from {+-1/4, +-1/2};
  perm a random row permutation, or the identity.

Every entry of A and of every Schur complement L[k:, k:] @ E[k:] is a short sum of multiples of 1/4.  Under the
largest-magnitude rule forward elimination is therefore exact in fp32 and in fp64, a column that is not in S is
exactly zero from the pivot row down, and the candidates of column S[k] are L[i, k] E[k, S[k]] with |L[i, k]| <= 1/2
off the diagonal: pivot k is the unique largest candidate.  For either precision and any tolerance below the pivots,
with r' = #{S < bar} and S' = S[:r']:

  rank r', pivots (k, S[k]); rows at and after r' zero left of the bar; rows before it  inv(E[:r', S']) @ E[:r'].

With identity_perm=True the first candidate of column S[k] is row k itself, so the first-non-zero rule exchanges no
rows either, pivots on +-4 / +-8 (a power of two: normalising is exact) and eliminates below with the multipliers
L[i, k] E[k, S[k]]: the rows from r' on are L[r':, r':] @ E[r':] exactly, right of the bar included -- the entries that
depend on the rule.

reduce_reference is the documented algorithm in numpy, in the working type (tests/test_rref_planted_host.py holds it
to the plant before the GPU is asked anything); CASES is the list of shapes both test files go through.
"""
import numpy as np

FIRST, MAX = 0, 1          # linalg_solver_amd._native.PIVOT_FIRST / PIVOT_MAX
RULE_NAME = {FIRST: "first", MAX: "max"}
U_ROUND = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}
SEED = 17
BLOCKED_MIN = 256 * 256    # kernels_rref_blk.hip rref_blocked / api.hip rref_first_fast: m * bar below this is per-column
FIRST_FAST_MAX_ROWS = 8192  # api.hip rref_first_fast


def spread(lo, hi, k, seed=0):
    """k distinct columns of [lo, hi), sorted."""
    rng = np.random.default_rng([int(seed), int(lo), int(hi), int(k)])
    return tuple(int(c) for c in np.sort(rng.choice(np.arange(lo, hi), k, replace=False)))


def pivot_columns(n, r, pivots, rng):
    if isinstance(pivots, str):
        if pivots == "random":
            S = rng.choice(n, r, replace=False)
        elif pivots == "tail":
            S = np.arange(n - r, n)
        elif pivots == "blocks":
            cand = np.array([c for c in range(n) if (c // 128) % 2 == 1 or c < 3])
            S = rng.choice(cand, r, replace=False)
        else:
            raise ValueError(pivots)
    else:
        S = np.array(pivots, dtype=np.int64)
        assert len(S) == r and len(set(S.tolist())) == r and S.min() >= 0 and S.max() < n
    return np.sort(S).astype(np.int64)


def planted_echelon(m, n, r, seed, pivots="random", identity_perm=False, ldens=None, matmul=None):
    """A, L, E, S, perm of the module docstring (float64 arrays).  The random stream does not depend on
    identity_perm: both variants share L, E and S.  matmul: a replacement for numpy's product (exact in any order)."""
    assert 0 <= r <= min(m, n)
    rng = np.random.default_rng([int(seed), int(m), int(n), int(r)])
    p = min(1.0, 16.0 / max(m, n))
    S = pivot_columns(n, r, pivots, rng) if r else np.zeros(0, dtype=np.int64)
    L = np.where(rng.random((m, r)) < (p if ldens is None else ldens), rng.choice(np.array([-0.5, -0.25, 0.25, 0.5]), (m, r)), 0.0)
    L = np.tril(L, -1)
    L[np.arange(r), np.arange(r)] = 1.0
    is_pivot = np.zeros(n, dtype=bool)
    is_pivot[S] = True
    E = np.where(rng.random((r, n)) < np.where(is_pivot, p, 0.5)[None, :], rng.integers(-3, 4, (r, n)).astype(np.float64), 0.0)
    E[np.arange(n)[None, :] <= S[:, None]] = 0.0
    E[np.arange(r), S] = rng.choice(np.array([-8.0, -4.0, 4.0, 8.0]), r)
    shuffled = rng.permutation(m)
    perm = np.arange(m) if identity_perm else shuffled
    PA = (L @ E) if matmul is None else matmul(L, E)
    A = np.empty_like(PA)
    A[perm] = PA
    return A, L, E, S, perm


def tri_solve_upper(T, B):
    """inv(T) @ B for an upper triangular T: numpy's extended precision up to order 320 (where it is wider than
    fp64), rounded to fp64 at the end; fp64 substitution above."""
    r = T.shape[0]
    wide = r <= 320 and np.finfo(np.longdouble).nmant > 52
    dt = np.longdouble if wide else np.float64
    T, X = T.astype(dt), B.astype(dt).copy()
    for i in range(r - 1, -1, -1):
        if i + 1 < r:
            X[i] -= T[i, i + 1:] @ X[i + 1:]
        X[i] /= T[i, i]
    return X.astype(np.float64)


def cond_inf_upper(T, solve=tri_solve_upper):
    r = T.shape[0]
    ninf = lambda M: float(np.abs(M).sum(axis=1).max())   # noqa: E731
    return ninf(T) * ninf(solve(T, np.eye(r)))


def planted_answer(L, E, S, bar, solve=tri_solve_upper):
    """rank r', the pivot list, R0 = inv(E[:r', S']) @ E[:r'] (r' x n), cond_inf(E[:r', S']), and the rows from r' on as
    the first-non-zero rule leaves them without interchanges: L[r':, r':] @ E[r':]."""
    rp = int(np.sum(S < bar))
    piv = [(k, int(S[k])) for k in range(rp)]
    T = E[:rp][:, S[:rp]]
    R0 = solve(T, E[:rp]) if rp else np.zeros((0, E.shape[1]))
    cond = cond_inf_upper(T, solve) if rp else 1.0
    low = L[rp:, rp:] @ E[rp:]
    return rp, piv, R0, cond, low


def default_tol_at_input(A, bar, dtype):
    """32 eps max(m, n) max|A[:, :bar]|: the default tolerance before the first elimination step."""
    m, n = A.shape
    return 32.0 * float(np.finfo(dtype).eps) * max(m, n) * float(np.abs(A[:, :bar]).max(initial=0.0))


def reduce_reference(A, bar, dtype, rule, tol=-1.0, amax_cols="left"):
    """The documented row reduction in numpy, in `dtype`: per column, first-non-zero or largest-magnitude pivot below
    the pivot row, |a| <= tol counts as zero (the column is cleared from the pivot row down and skipped), default
    tolerance 32 eps max(m, n) * (running maximum of the working matrix left of the bar, the finished pivot rows
    above the current one left out: they are normalised, not at the scale of the data), elimination above and below
    in one sweep.  amax_cols="all" takes the running maximum over the carried-along columns too: NOT the documented
    rule, kept to show what it does to a large right-hand side.  Returns R, pivots."""
    a = np.array(A, dtype=dtype)
    m, n = a.shape
    eps_scale = 32.0 * float(np.finfo(dtype).eps) * max(m, n)
    amax = float(np.abs(a[:, :bar]).max(initial=0.0))
    hi = n if amax_cols == "all" else bar
    pi, piv = 0, []
    for pj in range(bar):
        if pi >= m:
            break
        t = tol if tol >= 0 else eps_scale * amax
        col = np.abs(a[pi:, pj].astype(np.float64))
        if rule == FIRST:
            nz = np.nonzero(col > t)[0]
            p = pi + int(nz[0]) if len(nz) else -1
        else:
            p = pi + int(np.argmax(col))
            if not col[p - pi] > t:
                p = -1
        if p < 0:
            a[pi:, pj] = 0
            continue
        if p != pi:
            a[[pi, p]] = a[[p, pi]]
        a[pi, pj:] = a[pi, pj:] / a[pi, pj]
        a[pi, pj] = 1
        f = a[:, pj].copy()
        f[pi] = 0
        rows = np.nonzero(f)[0]
        if len(rows):
            a[rows, pj:] -= np.outer(f[rows], a[pi, pj:])
            amax = max(amax, float(np.abs(a[rows[rows > pi], pj:hi]).max(initial=0.0)))
        piv.append((pi, pj))
        pi += 1
    return a, piv


# ------------------------------------------------------------------------------------------------ the shapes
# id, m, n, r, pivots, bar; f32: "default" (default tolerance), a number (that explicit tolerance), None (fp64 only);
# ldens: density of L where the default would leave it empty.  The id names the path LSX_PIVOT_MAX takes; under
# LSX_PIVOT_FIRST a blocked shape takes api.hip rref_first_fast in fp64 up to 8192 rows and the per-column kernels
# otherwise (path_of).
def _case(id, m, n, r, pivots, bar, f32="default", ldens=None, rules=(FIRST, MAX)):
    return dict(id=id, m=m, n=n, r=r, pivots=pivots, bar=bar, f32=f32, ldens=ldens, rules=rules)


PER_COLUMN_CASES = [
    _case("percol-1x1", 1, 1, 1, "random", 1),
    _case("percol-1x7", 1, 7, 1, (2,), 7),
    _case("percol-7x1", 7, 1, 1, "random", 1),
    _case("percol-40x60-bar45", 40, 60, 25, "random", 45),
    _case("percol-200x300-bar250", 200, 300, 120, "random", 250),
]
BLOCKED_CASES = (
    [_case(f"blocked-600x{bar + 31}-bar{bar}", 600, bar + 31, 90, "random", bar) for bar in (127, 128, 129, 255, 256, 257)]
    + [_case(f"blocked-600x700-rank{k}", 600, 700, k + 3, spread(0, 650, k, 1) + (655, 670, 699), 650) for k in (1, 127, 128, 129, 257)]
    + [
        _case("blocked-300x900-full-row-rank", 300, 900, 300, "random", 900),
        _case("blocked-300x900-full-row-rank-bar600", 300, 900, 300, spread(0, 600, 300, 2), 600),
        _case("blocked-900x300-full-column-rank", 900, 300, 300, "random", 300),
        _case("blocked-600x500-pivots-at-the-right-end", 600, 500, 200, "tail", 500),
        _case("blocked-600x700-blocks-without-a-pivot", 600, 700, 150, "blocks", 700),
        _case("blocked-600x700-blocks-without-a-pivot-bar600", 600, 700, 150, "blocks", 600),
        _case("blocked-600x400-pivot-in-the-last-column", 600, 400, 100, spread(0, 399, 99, 3) + (399,), 400),
        _case("blocked-600x400-pivots-at-bar-1-and-bar", 600, 400, 82, spread(0, 299, 80, 4) + (299, 300), 300),
        _case("blocked-600x500-bar200-cuts-a-block", 600, 500, 150, "random", 200),
    ]
)
# 70000 rows: the 65535-row stride of rrb_finish_kernel and of the gathers; 4 x 20000: 157 blocks, the last pivot in
# the last one.  fp32 with an explicit tolerance: test_rref_planted_host.py shows why.
F32_EXPLICIT_TOL = 0.5
EXTREME_CASES = [
    _case("blocked-70000x8-bar7", 70000, 8, 6, (0, 1, 3, 4, 6, 7), 7, f32=F32_EXPLICIT_TOL, ldens=0.5),
    _case("blocked-4x20000-bar19990", 4, 20000, 4, (5, 9000, 15000, 19985), 19990, f32=F32_EXPLICIT_TOL),
]
# both sides of the m <= 8192 switch of rref_first_fast; bar small: the per-column side costs two launches per column
SWITCH_CASES = [
    _case("blocked-8192x40-bar24", 8192, 40, 22, "random", 24, f32=None, ldens=0.25),
    _case("blocked-8200x40-bar24", 8200, 40, 22, "random", 24, f32=None, ldens=0.25),
]
CASES = PER_COLUMN_CASES + BLOCKED_CASES + EXTREME_CASES + SWITCH_CASES
# shuffled rows under the first-non-zero rule, against oracle/rowreduce.py on Fractions
SHUFFLED_FIRST_CASES = [
    _case("percol-40x60-bar45-shuffled", 40, 60, 25, "random", 45),
    _case("percol-60x40-bar33-shuffled", 60, 40, 30, "random", 33),
    _case("blocked-300x340-bar320-shuffled", 300, 340, 40, "random", 320, f32=None),
]
# cases whose carried-along columns are scaled by 2^k (bar < n), one or more on every path
SCALED_CASE_IDS = ["percol-40x60-bar45", "percol-200x300-bar250", "blocked-600x160-bar129", "blocked-600x700-rank129",
                   "blocked-600x400-pivots-at-bar-1-and-bar"]
SCALE_EXPONENTS = {"float64": (20, 40, 50), "float32": (10, 20)}
BENCH_CASE = _case("blocked-8192x8192-rank4096-shuffled", 8192, 8192, 4096, "random", 8192, f32=None, rules=(MAX,))


def case_by_id(cid):
    return next(c for c in CASES if c["id"] == cid)


def path_of(case, rule, dtype):
    """Which implementation the shape, rule and type select at the default options."""
    if case["m"] * case["bar"] < BLOCKED_MIN:
        return "per-column"
    if rule == MAX:
        return "blocked"
    if np.dtype(dtype) == np.float64 and case["m"] <= FIRST_FAST_MAX_ROWS:
        return "first-fast"
    return "per-column"


def dtypes_of(case):
    return [np.float64] if case["f32"] is None else [np.float32, np.float64]


def tol_of(case, dtype):
    return float(case["f32"]) if np.dtype(dtype) == np.float32 and case["f32"] not in (None, "default") else -1.0


def build(case, rule, matmul=None, shuffled=None):
    """The planted input of a case: rows shuffled under the largest-magnitude rule, in place under the first-non-zero
    rule (unless `shuffled` says otherwise)."""
    ident = (rule == FIRST) if shuffled is None else not shuffled
    return planted_echelon(case["m"], case["n"], case["r"], SEED, case["pivots"], identity_perm=ident, ldens=case["ldens"],
                           matmul=matmul)


def verify(label, dtype, A, bar, answer, R, piv, rank, check_low, R_ref=None):
    """The checks of a planted case on a result (R, piv, rank): exact structure, values of the pivot rows against
    answer = planted_answer(...) within 4 r u cond_inf(E[:, S']) max(1, max|R0|) wherever that is below 1e-3, and
    (check_low) the rows below the rank right of the bar within 8 u max|A|.  Prints one line; R_ref: the numpy
    reference's result, whose error is printed beside the measured one."""
    rp, want_piv, R0, cond, low = answer
    u = U_ROUND[np.dtype(dtype).name]
    assert R.dtype == np.dtype(dtype) and R.shape == A.shape, label
    assert rank == rp, f"{label}: rank {rank}, planted {rp}"
    assert [tuple(p) for p in piv] == want_piv, f"{label}: pivots differ from the plant, first at {_first_diff(piv, want_piv)}"
    pc = [c for _, c in want_piv]
    assert np.all(np.isfinite(R)), label
    assert np.array_equal(R[:rp][:, pc], np.eye(rp, dtype=R.dtype)), f"{label}: pivot columns are not unit vectors"
    assert not R[rp:, :bar].any(), f"{label}: non-zero entry below the rank left of the bar"
    R64 = R.astype(np.float64)
    err = float(np.abs(R64[:rp] - R0).max(initial=0.0))
    bound = 4 * max(rp, 1) * u * cond * max(1.0, float(np.abs(R0).max(initial=0.0)))
    line = f"RREF {label}: rank {rank}, cond_inf {cond:.1f}, pivot rows err {err:.3e} (bound {bound:.3e}{'' if bound < 1e-3 else ', not asserted'})"
    if R_ref is not None:
        line += f", numpy {float(np.abs(R_ref.astype(np.float64)[:rp] - R0).max(initial=0.0)):.3e}"
    lerr = lbound = None
    if check_low:
        lerr = float(np.abs(R64[rp:, bar:] - low[:, bar:]).max(initial=0.0))
        lbound = 8 * u * float(np.abs(A).max(initial=0.0))
        line += f"; rows below the rank right of the bar err {lerr:.3e} (bound {lbound:.3e}, max {float(np.abs(low[:, bar:]).max(initial=0.0)):.1f})"
    print(line)
    if bound < 1e-3:
        assert err <= bound, label
    if check_low:
        assert lerr <= lbound, label
    return err, bound, lerr, lbound


def _first_diff(a, b):
    for k, (x, y) in enumerate(zip(a, b)):
        if tuple(x) != tuple(y):
            return k, tuple(x), tuple(y)
    return min(len(a), len(b)), len(a), len(b)


def tolerance_matrix(n, tol, zero_cols, dtype, seed=5):
    """A row-shuffled diagonal matrix of order n in `dtype`: the entries of the columns in zero_cols equal `tol`
    exactly, every second other one is the next number above tol, the rest lie in [1, 8] with mixed signs.  Called
    with tol = tol: pivot columns = the complement of zero_cols in order, R = the selection matrix of those rows,
    the columns of zero_cols exactly zero.  Returns A, the pivot columns, and the row each column's entry sits in."""
    rng = np.random.default_rng([int(seed), int(n)])
    t = np.dtype(dtype).type(tol)
    assert float(t) == tol, "tol must be a number of the working type"
    d = rng.integers(8, 65, n).astype(np.float64) / 8.0 * rng.choice(np.array([-1.0, 1.0]), n)
    d[::2] = float(np.nextafter(t, np.dtype(dtype).type(np.inf)))
    d[1::4] *= -1.0
    Z = np.array(sorted(zero_cols), dtype=np.int64)
    d[Z] = tol
    d[Z[::2]] = -tol
    rows = rng.permutation(n)
    A = np.zeros((n, n), dtype=dtype)
    A[rows, np.arange(n)] = d.astype(dtype)
    keep = np.array([c for c in range(n) if c not in set(Z.tolist())], dtype=np.int64)
    return A, keep, rows
