"""The row reductions on the MI355X against echelon forms known in advance (tests/planted_rref.py, proved on the CPU by
tests/test_rref_planted_host.py): lsx_rref_f64 / lsx_rref_f32 through dense.rref and lsx_rref_f64_dev through
DeviceSolver.rref_, both pivot rules, every implementation behind them.

  path         code                                      taken when
  per-column   kernels_rref.hip launch_rref              m * bar < 256 * 256; option rref_blocked = 0; the first-non-zero
                                                         rule whenever the next path declines
  blocked      kernels_rref_blk.hip rref_blocked<T>      LSX_PIVOT_MAX and m * bar >= 256 * 256, fp64 and fp32
  first-fast   api.hip rref_first_fast (fp64)            LSX_PIVOT_FIRST, m <= 8192, m * bar >= 256 * 256

Every printed line names the path of its case (planted_rref.path_of), and `rref_first_used` is asserted wherever the
first-non-zero rule runs in fp64.

1. Planted echelon forms (planted_rref.CASES).  Rank and pivot list ==, R[:r][:, pc] == I, R[r:, :bar] == 0.  Pivot
   rows within 4 r u cond_inf(E[:, S']) max(1, max|R0|) of R0 = inv(E[:r, S']) E[:r] (u = 2^-24 / 2^-53), asserted where
   that bound is below 1e-3, printed everywhere beside the error of the numpy restatement in the same type.  Under
   LSX_PIVOT_FIRST the rows are planted in place, and the rows below the rank right of the bar -- the entries that
   depend on the rule -- are held to L[r:, r:] E[r:, bar:] within 8 u max|A|.  Under LSX_PIVOT_MAX both values of the
   option rref_blocked are held to the plant, not to each other.
2. The first-non-zero rule on shuffled rows against oracle/rowreduce.py in rational arithmetic: pivots ==, values
   within 1e-9 * scale in fp64.
3. Bench scale: 8192 x 8192, rank 4096, pivot columns over the whole width, rows shuffled, LSX_PIVOT_MAX on device
   tensors; product and oracle formed on the GPU by torch in fp64.
4. Tolerance: |a| <= tol counts as zero.  A shuffled diagonal matrix with entries equal to tol in chosen columns and the
   next number above tol elsewhere: nothing is eliminated, the answer is exact.
5. Scaling the carried-along columns by 2^k changes neither rank nor pivots, leaves the left block bit-identical and
   multiplies the right block by exactly 2^k (a power of two commutes with every rounding): every path, and the
   Matrix surface.
"""
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import planted_rref as pr  # noqa: E402
from oracle import rowreduce  # noqa: E402

RULES = [pr.FIRST, pr.MAX]
TOL = 0.75


@pytest.fixture(scope="module")
def la():
    import linalg_solver_amd as la

    la.default_handle()
    return la


@pytest.fixture(scope="module")
def dev():
    import torch

    from linalg_solver_amd.device import DeviceSolver

    assert torch.cuda.is_available()
    return DeviceSolver()


def _name(dtype):
    return np.dtype(dtype).name


def _rule_id(rule):
    return pr.RULE_NAME[rule]


def _case_id(case):
    return case["id"]


_PLANT = {}


def _plant(case, rule):
    """Input and planted answer of a case, kept for the module."""
    key = (case["id"], rule)
    if key not in _PLANT:
        A, L, E, S, perm = pr.build(case, rule)
        _PLANT[key] = (A, pr.planted_answer(L, E, S, case["bar"]))
    return _PLANT[key]


def _host(la, A, bar, dtype, rule, tol):
    """dense.rref (lsx_rref_f64 / lsx_rref_f32) -> R, pivots, rank, rref_first_used."""
    from linalg_solver_amd import dense

    R, piv, rank = dense.rref(A.astype(dtype), bar_col=bar, tol=tol, pivot_rule=rule, dtype=dtype)
    return R, piv, rank, la.default_handle().get_option("rref_first_used")


def _device(dev, A, bar, rule, tol):
    """DeviceSolver.rref_ (lsx_rref_f64_dev) -> R, pivots, rank, rref_first_used."""
    import torch

    dR = torch.from_numpy(np.ascontiguousarray(A, dtype=np.float64)).cuda()
    dpiv, drank = dev.rref_(dR, bar_col=bar, tol=tol, pivot_rule=rule)
    torch.cuda.synchronize()
    rank = int(drank.item())
    p = dpiv.cpu().numpy()
    return dR.cpu().numpy(), [(int(p[2 * i]), int(p[2 * i + 1])) for i in range(rank)], rank, dev.h.get_option("rref_first_used")


def _entry_points(la, dev, dtype):
    """(name, run(A, bar, rule, tol), handle) for a type: lsx_rref_f64_dev has no fp32 form."""
    pts = [("dense.rref", lambda A, bar, rule, tol: _host(la, A, bar, dtype, rule, tol), la.default_handle())]
    if np.dtype(dtype) == np.float64:
        pts.append(("rref_", lambda A, bar, rule, tol: _device(dev, A, bar, rule, tol), dev.h))
    return pts


def _with_blocked(handle, value, fn):
    try:
        handle.set_option("rref_blocked", value)
        return fn()
    finally:
        handle.set_option("rref_blocked", 1)


# ------------------------------------------------------------------------------------------------ 1. planted
@pytest.mark.parametrize("rule", RULES, ids=_rule_id)
@pytest.mark.parametrize("case", pr.CASES, ids=_case_id)
def test_planted_reduction(la, dev, case, rule):
    bar = case["bar"]
    A, answer = _plant(case, rule)
    for dtype in pr.dtypes_of(case):
        tol = pr.tol_of(case, dtype)
        R_ref, _ = pr.reduce_reference(A, bar, dtype, rule, tol)
        default_path = pr.path_of(case, rule, dtype)
        for name, run, handle in _entry_points(la, dev, dtype):
            # option rref_blocked = 0 sends every shape and rule to the per-column kernels
            for blocked in ((1,) if default_path == "per-column" else (1, 0)):
                path = default_path if blocked else "per-column"
                R, piv, rank, used = _with_blocked(handle, blocked, lambda: run(A, bar, rule, tol))
                label = f"{case['id']} {_name(dtype)} {pr.RULE_NAME[rule]} path={path} {name} rref_blocked={blocked}"
                if rule == pr.FIRST and np.dtype(dtype) == np.float64:
                    assert used == (1 if path == "first-fast" else 0), f"{label}: rref_first_used = {used}"
                pr.verify(label, dtype, A, bar, answer, R, piv, rank, check_low=rule == pr.FIRST, R_ref=R_ref)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=_name)
@pytest.mark.parametrize("rule", RULES, ids=_rule_id)
def test_input_without_a_pivot_has_rank_zero(la, dev, rule, dtype):
    """300 x 300 of zeros, and of entries +-tol with bar_col = 250: the rank-0 branch of rref_first_fast (fp64,
    first-non-zero rule) and of the blocked form.  |a| <= tol counts as zero: rank 0, the left block exactly zero on
    every path, the carried-along columns untouched."""
    sign = np.where(np.random.default_rng(3).random((300, 300)) < 0.5, -1.0, 1.0)
    for what, A, bar, tol in (("zeros", np.zeros((300, 300)), 300, -1.0), ("tol", sign * TOL, 250, TOL)):
        want = A.copy()
        want[:, :bar] = 0.0
        for name, run, handle in _entry_points(la, dev, dtype):
            for blocked in (1, 0):
                R, piv, rank, used = _with_blocked(handle, blocked, lambda: run(A, bar, rule, tol))
                label = f"RANK0 {what} {_name(dtype)} {pr.RULE_NAME[rule]} {name} rref_blocked={blocked}"
                print(f"{label}: rank {rank}, entries differing {int(np.count_nonzero(R != want))}")
                assert rank == 0 and piv == [] and np.array_equal(R, want.astype(dtype)), label
                if rule == pr.FIRST and np.dtype(dtype) == np.float64:
                    assert used == blocked, label


# ------------------------------------------------------------------------------------------------ 2. shuffled rows
@pytest.mark.parametrize("case", pr.SHUFFLED_FIRST_CASES, ids=_case_id)
def test_first_rule_on_shuffled_rows_against_rational_arithmetic(la, dev, case):
    A, L, E, S, perm = pr.build(case, pr.FIRST, shuffled=True)
    bar = case["bar"]
    exact, xpiv, _ = rowreduce.row_reduce([[Fraction(v) for v in row] for row in A.tolist()], bar)
    X = np.array([[float(v) for v in row] for row in exact])
    xpiv = [tuple(p) for p in xpiv]
    scale = max(1.0, float(np.abs(X).max()))
    for dtype in pr.dtypes_of(case):
        path = pr.path_of(case, pr.FIRST, dtype)
        for name, run, handle in _entry_points(la, dev, dtype):
            R, piv, rank, used = run(A, bar, pr.FIRST, -1.0)
            err = float(np.abs(R.astype(np.float64) - X).max()) / scale
            print(f"SHUFFLED {case['id']} {_name(dtype)} first path={path} {name}: rank {rank}, err / scale {err:.3e}, scale {scale:.1f}")
            assert rank == len(xpiv) and piv == xpiv
            pc = [c for _, c in piv]
            assert np.array_equal(R[:rank][:, pc], np.eye(rank, dtype=dtype)) and not R[rank:, :bar].any()
            if np.dtype(dtype) == np.float64:
                assert used == (1 if path == "first-fast" else 0)
                assert err < 1e-9


# ------------------------------------------------------------------------------------------------ 3. bench scale
def _mm_gpu(a, b):
    import torch

    return (torch.from_numpy(np.ascontiguousarray(a)).cuda() @ torch.from_numpy(np.ascontiguousarray(b)).cuda()).cpu().numpy()


def _solve_upper_gpu(T, B):
    """inv(T) B for an upper triangular T by halving: T = [[a, b], [0, d]] gives X2 = inv(d) B2, X1 = inv(a) (B1 - b X2);
    blocks of order <= 512 by substitution on the CPU, the products by torch on the GPU in fp64."""
    r = T.shape[0]
    if r <= 512:
        import scipy.linalg as sl

        return sl.solve_triangular(T, B, lower=False)
    h = r // 2
    X2 = _solve_upper_gpu(T[h:, h:], B[h:])
    X1 = _solve_upper_gpu(T[:h, :h], B[:h] - _mm_gpu(T[:h, h:], X2))
    return np.vstack([X1, X2])


def test_planted_reduction_at_bench_scale(dev):
    import torch

    case = pr.BENCH_CASE
    m, n, r, bar = case["m"], case["n"], case["r"], case["bar"]
    A, L, E, S, perm = pr.build(case, pr.MAX, matmul=_mm_gpu)
    assert int(S[-1]) > n - 64 and int((S >= n // 2).sum()) > r // 4, "pivot columns are spread over the whole width"
    answer = pr.planted_answer(L, E, S, bar, solve=_solve_upper_gpu)
    dR = torch.from_numpy(A).cuda()
    dpiv, drank = dev.rref_(dR, bar_col=bar, pivot_rule=pr.MAX)
    torch.cuda.synchronize()
    rank = int(drank.item())
    p = dpiv.cpu().numpy()
    piv = [(int(p[2 * i]), int(p[2 * i + 1])) for i in range(min(rank, r))]
    pr.verify(f"{case['id']} float64 max path=blocked rref_", np.float64, A, bar, answer, dR.cpu().numpy(), piv, rank, check_low=False)


# ------------------------------------------------------------------------------------------------ 4. tolerance
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=_name)
@pytest.mark.parametrize("rule", RULES, ids=_rule_id)
@pytest.mark.parametrize("n", [40, 300])
def test_an_entry_equal_to_the_tolerance_counts_as_zero(la, dev, n, rule, dtype):
    Z = tuple(sorted(set(pr.spread(0, n, n // 5, 9) + ((n - 1,) if n == 300 else ()))))
    A, keep, rows = pr.tolerance_matrix(n, TOL, Z, dtype)
    want = np.zeros((n, n), dtype=dtype)
    want[np.arange(len(keep)), keep] = 1
    want_piv = [(k, int(c)) for k, c in enumerate(keep)]
    case = dict(m=n, bar=n)
    default_path = pr.path_of(case, rule, dtype)
    for name, run, handle in _entry_points(la, dev, dtype):
        for blocked in ((1,) if default_path == "per-column" else (1, 0)):
            path = default_path if blocked else "per-column"
            R, piv, rank, used = _with_blocked(handle, blocked, lambda: run(A.astype(np.float64), n, rule, TOL))
            label = f"TOL n={n} {_name(dtype)} {pr.RULE_NAME[rule]} path={path} {name}"
            print(f"{label}: rank {rank} (expected {len(keep)}), entries differing from the selection matrix {int(np.count_nonzero(R != want))}")
            assert rank == len(keep) and piv == want_piv, label
            assert np.array_equal(R, want), label
            if rule == pr.FIRST and np.dtype(dtype) == np.float64:
                assert used == (1 if path == "first-fast" else 0), label


# ------------------------------------------------------------------------------------------------ 5. scaling
@pytest.mark.parametrize("rule", RULES, ids=_rule_id)
@pytest.mark.parametrize("cid", pr.SCALED_CASE_IDS)
def test_scaling_the_carried_columns_by_a_power_of_two(la, dev, cid, rule):
    case = pr.case_by_id(cid)
    bar = case["bar"]
    assert bar < case["n"]
    A, answer = _plant(case, rule)
    rp, want_piv = answer[0], answer[1]
    for dtype in pr.dtypes_of(case):
        path = pr.path_of(case, rule, dtype)
        for name, run, handle in _entry_points(la, dev, dtype):
            R0, piv0, rank0, _ = run(A, bar, rule, -1.0)
            results = []
            for k in pr.SCALE_EXPONENTS[_name(dtype)]:
                A2 = A.copy()
                A2[:, bar:] *= 2.0 ** k
                results.append((k,) + tuple(run(A2, bar, rule, -1.0)[:3]))
            print(f"SCALED {cid} {_name(dtype)} {pr.RULE_NAME[rule]} path={path} {name}: planted rank {rp}, unscaled {rank0}, "
                  + ", ".join(f"2^{k}: {rank}" for k, _, _, rank in results))
            assert rank0 == rp and piv0 == want_piv
            for k, R, piv, rank in results:
                assert rank == rp and piv == want_piv, f"{cid} {_name(dtype)} {name}: carried columns * 2^{k} changed the pivots"
                assert np.array_equal(R[:, :bar], R0[:, :bar]), f"2^{k}: the left block must not change"
                assert np.array_equal(R[:, bar:], R0[:, bar:] * np.dtype(dtype).type(2.0 ** k)), f"2^{k}: the right block must scale exactly"


def test_a_large_right_hand_side_through_the_matrix_surface(la):
    """[[2, 1], [1, 3], [3, 4]] x = 2^50 A [1, 1]: consistent, rank 2 (m * bar < 256 * 256: the per-column kernels under
    both rules).  Under the first-non-zero rule the pivots are 2 and 5/2 and every operation is exact."""
    A = [[2.0, 1.0], [1.0, 3.0], [3.0, 4.0]]
    b = [3.0 * 2.0 ** 50, 4.0 * 2.0 ** 50, 7.0 * 2.0 ** 50]
    sol = la.Matrix(A).find_preimage_of(b)
    print(f"find_preimage_of with b = 2^50 * A [1, 1]: {sol!r}")
    assert isinstance(sol, la.Matrix.AffineSubspace)
    assert sol.get_one() == [2.0 ** 50, 2.0 ** 50] and sol.dim() == 0
    red, piv, _, _ = la.Matrix([row + [v] for row, v in zip(A, b)]).row_reduce(bar_col=2)
    assert piv == [(0, 0), (1, 1)] and red == [[1.0, 0.0, 2.0 ** 50], [0.0, 1.0, 2.0 ** 50], [0.0, 0.0, 0.0]]
    # a planted input with its carried-along columns scaled, through Matrix.row_reduce_array
    case = pr.case_by_id("percol-40x60-bar45")
    Ap, answer = _plant(case, pr.FIRST)
    A2 = Ap.copy()
    A2[:, case["bar"]:] *= 2.0 ** 50
    R0, piv0 = la.Matrix.from_numpy(Ap).row_reduce_array(bar_col=case["bar"])
    R, piv = la.Matrix.from_numpy(A2).row_reduce_array(bar_col=case["bar"])
    print(f"row_reduce_array 40 x 60, carried columns * 2^50: {len(piv)} pivots, planted {answer[0]}")
    assert piv0 == answer[1] and piv == answer[1]
    assert np.array_equal(R[:, :45], R0[:, :45]) and np.array_equal(R[:, 45:], R0[:, 45:] * 2.0 ** 50)
