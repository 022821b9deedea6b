"""The planted-echelon oracle (tests/planted_rref.py) proved on the CPU before the GPU is held to it.

For every shape, type and rule that tests/test_gpu_rref_planted.py uses: the construction is exact in fp32; the numpy
restatement of the documented algorithm (planted_rref.reduce_reference: per column, either rule, |a| <= tol is zero,
default tolerance 32 eps max(m, n) * running maximum left of the bar), run in the working type with the tolerance
the GPU test passes, returns the planted rank and pivots on its own and stays inside the bounds the GPU test
asserts.  At small orders the plant and the restatement are held to oracle/rowreduce.py in rational arithmetic,
with rows in place and shuffled.  The last tests show what the default tolerance does at 70000 rows in fp32, and what
a running maximum taken over the carried-along columns does to a large right-hand side.
"""
from fractions import Fraction

import numpy as np
import pytest

import planted_rref as pr
from oracle import rowreduce

ALL_CASES = pr.CASES + pr.SHUFFLED_FIRST_CASES


def _name(dtype):
    return np.dtype(dtype).name


def _rational(A, bar):
    exact, piv, _ = rowreduce.row_reduce([[Fraction(v) for v in row] for row in A.tolist()], bar)
    return np.array([[float(v) for v in row] for row in exact]), [tuple(p) for p in piv]


@pytest.mark.parametrize("case", ALL_CASES + [pr.BENCH_CASE], ids=lambda c: c["id"])
def test_planted_echelon_is_exact(case):
    if case is pr.BENCH_CASE:      # the same generator at a quarter of the order: the full product is formed on the GPU
        case = dict(case, m=2048, n=2048, r=1024, bar=2048)
    A, L, E, S, perm = pr.build(case, pr.MAX)
    m, n, r = case["m"], case["n"], case["r"]
    assert A.shape == (m, n) and L.shape == (m, r) and E.shape == (r, n) and len(S) == r
    assert np.array_equal(A.astype(np.float32).astype(np.float64), A), "A must survive the round trip through fp32"
    assert np.array_equal(A * 4, np.round(A * 4)) and np.abs(A).max(initial=0.0) < 2 ** 10
    assert np.array_equal(A[perm], L @ E)
    assert np.array_equal((L.astype(np.float32) @ E.astype(np.float32)).astype(np.float64), A[perm])
    assert np.array_equal((E.T @ L.T).T, A[perm])
    assert np.all(np.diff(S) > 0) and sorted(perm.tolist()) == list(range(m))
    assert np.array_equal(L[np.arange(r), np.arange(r)], np.ones(r)) and np.all(np.triu(L[:r], 1) == 0)
    assert np.all(np.abs(np.tril(L, -1)) <= 0.5)
    assert np.all(np.isin(np.abs(E[np.arange(r), S]), (4.0, 8.0)))
    assert np.all(E[np.arange(n)[None, :] < S[:, None]] == 0) and np.all(np.abs(E) <= 8) and np.array_equal(E, np.round(E))
    A2, L2, E2, S2, perm2 = pr.build(case, pr.FIRST)
    assert np.array_equal(perm2, np.arange(m)) and np.array_equal(L2, L) and np.array_equal(E2, E) and np.array_equal(A2, L @ E)
    if isinstance(case["pivots"], str) and case["pivots"] == "blocks":
        blocks_with = set((S // 128).tolist())
        assert any(b not in blocks_with for b in range(n // 128)), "the pattern must leave a whole block without a pivot"


@pytest.mark.parametrize("rule", [pr.FIRST, pr.MAX], ids=lambda r: pr.RULE_NAME[r])
@pytest.mark.parametrize("case", pr.CASES, ids=lambda c: c["id"])
def test_reference_reduction_returns_the_plant(case, rule):
    """Both types, with the tolerance the GPU test passes: rank, pivots, unit pivot columns and zero rows exactly,
    values inside the GPU test's bounds (pr.verify asserts all of it)."""
    A, L, E, S, perm = pr.build(case, rule)
    bar = case["bar"]
    answer = pr.planted_answer(L, E, S, bar)
    assert answer[0] == int(np.sum(S < bar)) and (answer[0] < case["r"] or bar == case["n"] or S.max() < bar)
    for dtype in pr.dtypes_of(case):
        tol = pr.tol_of(case, dtype)
        if tol < 0 and dtype == np.float32:
            assert pr.default_tol_at_input(A, bar, dtype) < 1.0, "not an fp32 case with the default tolerance"
        R, piv = pr.reduce_reference(A, bar, dtype, rule, tol)
        label = f"{case['id']} {_name(dtype)} {pr.RULE_NAME[rule]} numpy"
        err, bound, lerr, _ = pr.verify(label, dtype, A, bar, answer, R, piv, len(piv), check_low=rule == pr.FIRST)
        assert bound < 1e-3 or dtype == np.float32, "every fp64 case must be one whose values are asserted"
        if rule == pr.FIRST:
            assert lerr == 0.0, "without interchanges the rows below the rank are exact"


@pytest.mark.parametrize("m,n,r,bar", [(40, 60, 25, 45), (60, 40, 30, 33), (30, 50, 30, 50), (30, 50, 20, 50)])
def test_plant_against_rational_arithmetic(m, n, r, bar):
    """Rows in place: the rational run of the reference's rule returns the planted pivots, inv(E[:r', S']) E[:r'] on
    top and L[r':, r':] E[r':] below -- every entry, right of the bar included."""
    A, L, E, S, perm = pr.planted_echelon(m, n, r, pr.SEED, identity_perm=True)
    rp, piv, R0, cond, low = pr.planted_answer(L, E, S, bar)
    X, xpiv = _rational(A, bar)
    assert xpiv == piv
    assert np.abs(X[:rp] - R0).max() <= 2.0 ** -50 * max(1.0, np.abs(R0).max())
    assert np.array_equal(X[rp:], low)
    if rp < r:
        assert np.abs(low[:, bar:]).max() > 0, "the rule-dependent entries must not be all zero"


@pytest.mark.parametrize("case", pr.SHUFFLED_FIRST_CASES, ids=lambda c: c["id"])
def test_shuffled_first_rule_against_rational_arithmetic(case):
    """Shuffled rows under the first-non-zero rule: the rule exchanges rows, and the restatement in the working type
    agrees with the rational run on the pivots (what the GPU test asserts in both types) and, in fp64, within the GPU
    test's 1e-9 * scale."""
    A, L, E, S, perm = pr.build(case, pr.FIRST, shuffled=True)
    bar = case["bar"]
    X, xpiv = _rational(A, bar)
    assert [c for _, c in xpiv] == [int(c) for c in S[S < bar]]
    assert not np.array_equal(perm[:len(xpiv)], np.arange(len(xpiv)))
    scale = max(1.0, float(np.abs(X).max()))
    for dtype in pr.dtypes_of(case):
        R, piv = pr.reduce_reference(A, bar, dtype, pr.FIRST)
        err = float(np.abs(R.astype(np.float64) - X).max()) / scale
        print(f"SHUFFLED {case['id']} {_name(dtype)} numpy: err / scale {err:.3e}, scale {scale:.1f}")
        assert piv == xpiv
        if dtype == np.float64:
            assert err < 1e-9


@pytest.mark.parametrize("n", [40, 300])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=_name)
@pytest.mark.parametrize("rule", [pr.FIRST, pr.MAX], ids=lambda r: pr.RULE_NAME[r])
def test_tolerance_matrix(n, dtype, rule):
    tol = 0.75
    Z = pr.spread(0, n, n // 5, 9) + ((n - 1,) if n == 300 else ())
    Z = tuple(sorted(set(Z)))
    A, keep, rows = pr.tolerance_matrix(n, tol, Z, dtype)
    assert A.dtype == dtype and np.count_nonzero(A) == n
    assert np.all(np.abs(A[rows[list(Z)], list(Z)]) == tol) and np.all(np.abs(A[rows[keep], keep]) > tol)
    assert np.abs(A[rows[keep], keep]).min() == np.nextafter(dtype(tol), dtype(np.inf))
    R, piv = pr.reduce_reference(A, n, dtype, rule, tol)
    assert [c for _, c in piv] == keep.tolist() and [r for r, _ in piv] == list(range(len(keep)))
    want = np.zeros((n, n), dtype=dtype)
    want[np.arange(len(keep)), keep] = 1
    assert np.array_equal(R, want)
    # one step down in the tolerance and the columns of Z are pivots too
    assert len(pr.reduce_reference(A, n, dtype, rule, float(np.nextafter(dtype(tol), dtype(0))))[1]) == n


def test_default_tolerance_of_the_extreme_shapes_in_fp32():
    """Why 70000 x 8 is not an fp32 case with the default tolerance: 32 * 2^-23 * 70000 * max|A| = 0.27 max|A| is above
    the non-zero candidates of magnitude 1 and 2 (|L[i, k] E[k, S[k]]|) already at max|A| = 8 and reaches the smallest
    pivot magnitude, 4, at max|A| = 15: "non-zero" would no longer mean non-zero.  A default-tolerance fp32 case
    keeps it below 1 (test_reference_reduction_returns_the_plant asserts that).  The explicit tolerance lies below
    every non-zero entry a planted reduction meets, so it returns the plant (same test); the 4 x 20000 shape gets the
    same explicit tolerance.  In fp64 the default is far below 1 for both."""
    tall = pr.case_by_id("blocked-70000x8-bar7")
    A = pr.build(tall, pr.MAX)[0]
    t32 = pr.default_tol_at_input(A, tall["bar"], np.float32)
    print(f"70000 x 8: default fp32 tolerance at the input {t32:.3f}, max|A| {np.abs(A).max()}")
    assert t32 >= 1.0 and t32 / float(np.abs(A).max()) * 15.0 >= 4.0
    assert pr.tol_of(tall, np.float32) == pr.F32_EXPLICIT_TOL < 1.0 and pr.tol_of(tall, np.float64) == -1.0
    for case in pr.EXTREME_CASES:
        A = pr.build(case, pr.MAX)[0]
        assert pr.default_tol_at_input(A, case["bar"], np.float64) < 1e-8
        assert np.abs(A[A != 0]).min() >= 0.25 and 0 < pr.tol_of(case, np.float32) < 1.0


def test_a_running_maximum_over_the_carried_columns_loses_pivots():
    """Scaling the columns right of the bar by 2^k must not change rank or pivots, and commutes with every rounding:
    left of the bar bit-identical, right of it 2^k times the unscaled result.  The documented rule (running maximum
    left of the bar) has that property; the maximum over all columns raises the tolerance above the pivots."""
    for cid in ("percol-40x60-bar45", "percol-200x300-bar250"):
        case = pr.case_by_id(cid)
        bar = case["bar"]
        for rule in (pr.FIRST, pr.MAX):
            A, L, E, S, perm = pr.build(case, rule)
            for dtype in pr.dtypes_of(case):
                R0, piv0 = pr.reduce_reference(A, bar, dtype, rule)
                for k in pr.SCALE_EXPONENTS[_name(dtype)]:
                    A2 = A.copy()
                    A2[:, bar:] *= 2.0 ** k
                    R, piv = pr.reduce_reference(A2, bar, dtype, rule)
                    assert piv == piv0 and np.array_equal(R[:, :bar], R0[:, :bar])
                    assert np.array_equal(R[:, bar:], R0[:, bar:] * dtype(2.0 ** k))
                k = pr.SCALE_EXPONENTS[_name(dtype)][-1]
                lost = len(piv0) - len(pr.reduce_reference(A2, bar, dtype, rule, amax_cols="all")[1])
                print(f"{cid} {_name(dtype)} {pr.RULE_NAME[rule]}: carried columns * 2^{k}, maximum over all columns loses {lost} of {len(piv0)} pivots")
                assert lost > 0
    # the 3 x 2 system of Matrix.find_preimage_of: consistent, rank 2, solution [1, 1] * 2^50
    A = np.array([[2.0, 1.0], [1.0, 3.0], [3.0, 4.0]])
    aug = np.hstack([A, (A @ np.ones(2) * 2.0 ** 50)[:, None]])
    for rule in (pr.FIRST, pr.MAX):
        R, piv = pr.reduce_reference(aug, 2, np.float64, rule)
        assert piv == [(0, 0), (1, 1)] and np.all(np.abs(R[:2, 2] / 2.0 ** 50 - 1.0) < 1e-15) and abs(R[2, 2]) < 4.0
        if rule == pr.FIRST:     # pivots 2 and 5/2: every operation is exact
            assert R[:2, 2].tolist() == [2.0 ** 50, 2.0 ** 50] and R[2, 2] == 0
        assert len(pr.reduce_reference(aug, 2, np.float64, rule, amax_cols="all")[1]) == 1
