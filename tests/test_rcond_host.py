"""The condition estimate without a GPU: the numpy twin of the iteration (tests/cpu_cond.py) against every LAPACK
value of tests/golden/rcond_cases.json, and the argument checks of the new Python keywords, which fire before any
device work.
"""
import math

import numpy as np
import pytest

import cpu_cond

CASES = cpu_cond.load_cases()
REGULAR = [c for c in CASES if c["kind"] in ("u11", "int5", "u11_shift") and c["n"] > 1]


def _id(c):
    return f"{c['kind']}-{c['n']}-{c['prec']}"


def _factors(case, how):
    import scipy.linalg as sl

    A = cpu_cond.matrix(case["kind"], case["n"], case["seed"]).astype(cpu_cond.DTYPE[case["prec"]])
    if how == "lapack":
        return A, sl.lu_factor(A)[0]
    from oracle import capi   # the scalar unblocked twin: the same factorisation, rounded differently

    LU, _, info = capi.getrf(A.astype(np.float64))
    assert info == 0
    return A, LU


def test_fixture_covers_the_cases_the_estimate_is_specified_on():
    have = {(c["kind"], c["n"], c["prec"]) for c in CASES}
    want = ({("u11", n, "f64") for n in (0, 1, 5, 64, 129, 300, 1000, 2048)} | {("int5", n, "f64") for n in (129, 300, 1000)} |
            {("u11_shift", n, "f32") for n in (64, 129, 300)} | {("unit_upper", n, "f64") for n in (40, 60, 100)} |
            {("u11_zero_col", 64, "f64")})
    assert have == want
    for c in REGULAR:
        assert c["seed"] == 1300 + c["n"]
        assert cpu_cond.bound(c) <= 0.35, "a bound above 0.35 checks nothing: the case does not belong here"


# LAPACK's own factors in the working precision, and for fp64 the scalar twin's as well
TWIN_RUNS = [(c, "lapack") for c in REGULAR] + [(c, "scalar_twin") for c in REGULAR if c["prec"] == "f64"]


@pytest.mark.parametrize("case,how", TWIN_RUNS, ids=[f"{_id(c)}-{h}" for c, h in TWIN_RUNS])
def test_twin_agrees_with_lapack_gecon(case, how):
    A, LU = _factors(case, how)
    bound = cpu_cond.bound(case)
    for nm, ordv in (("1", 1), ("I", np.inf)):
        anorm = float(np.linalg.norm(A.astype(np.float64), ordv))
        assert anorm == pytest.approx(case["anorm"][nm], rel=1e-6 if case["prec"] == "f32" else 1e-13)
        count = []
        rc = cpu_cond.rcond_twin(LU, anorm, nm, count)
        ref, exact = case["rcond_lapack"][nm], case["rcond_exact"][nm]
        print(f"{_id(case)} {how} norm {nm}: twin {rc:.6e} lapack {ref:.6e} exact {exact:.6e} "
              f"|ratio-1| {abs(rc / ref - 1):.2e} bound {bound:.2e} solves {count[0]}")
        assert abs(rc / ref - 1.0) <= bound
        assert rc >= exact * (1.0 - bound)         # the method bounds ||inv(A)|| from below
        assert 4 <= count[0] <= 11


def test_twin_on_the_matrix_the_pivot_ratio_is_blind_to():
    case = next(c for c in CASES if c["kind"] == "unit_upper" and c["n"] == 60)
    A = cpu_cond.matrix("unit_upper", 60, case["seed"])
    assert np.all(np.diag(A) == 1.0) and np.min(np.abs(np.diag(A))) / np.max(np.abs(A)) == 1.0   # what the proxy sees
    rc = cpu_cond.rcond_twin(A.copy(), float(np.linalg.norm(A, 1)), "1")    # upper triangular: its own U, L = I
    assert rc < 2.3e-16 and abs(rc / case["rcond_lapack"]["1"] - 1.0) <= 1e-12


def test_twin_edge_cases():
    assert cpu_cond.rcond_twin(np.zeros((0, 0)), 0.0) == 1.0
    assert cpu_cond.rcond_twin(np.array([[4.0]]), 4.0) == pytest.approx(1.0, rel=1e-15)
    sing = next(c for c in CASES if c["kind"] == "u11_zero_col")
    assert sing["singular"] and sing["info"] == 18 and sing["rcond_lapack"] == {"1": 0.0, "I": 0.0}
    _, LU = _factors(sing, "lapack")
    assert cpu_cond.rcond_twin(LU, sing["anorm"]["1"]) == 0.0


def test_new_keywords_reject_bad_arguments_before_any_device_work():
    import linalg_solver_amd as la
    from linalg_solver_amd import dense

    sq, rect = np.eye(3), np.ones((2, 3))
    piv = np.arange(3, dtype=np.int32)
    with pytest.raises(ValueError, match="wrong number of rows"):
        dense.lu_solve(sq, piv, np.ones(4), trans=True)
    with pytest.raises(ValueError, match="square"):
        dense.lu_solve(rect, piv, np.ones(2), trans=True)
    with pytest.raises(ValueError, match="square"):
        dense.solve(rect, np.ones(2), trans=True)
    with pytest.raises(ValueError, match="wrong number of rows"):
        dense.solve(sq, np.ones((4, 2)), trans=True)
    with pytest.raises(ValueError, match="norm must be 1 or inf"):
        dense.norm(sq, which=2)
    with pytest.raises(ValueError, match="2-D"):
        dense.norm(np.ones(3))
    with pytest.raises(ValueError, match="square"):
        dense.rcond(rect)
    with pytest.raises(ValueError, match="norm must be 1 or inf"):
        dense.rcond(sq, norm="fro")
    with pytest.raises(TypeError, match="float64 or float32"):
        dense.rcond(sq, dtype=np.float16)
    with pytest.raises(ValueError, match="square"):
        dense.lu_rcond(rect, piv, 1.0)
    with pytest.raises(ValueError, match="anorm"):
        dense.lu_rcond(sq, piv, math.nan)
    with pytest.raises(ValueError, match="shorter"):
        dense.lu_rcond(sq, piv[:2], 1.0)
    m = la.Matrix([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    with pytest.raises(ValueError, match="square"):
        m.rcond()
    with pytest.raises(ValueError, match="square"):
        m.cond()
    with pytest.raises(ValueError, match="square"):
        m.solve_array([1.0, 2.0], trans=True)
    with pytest.raises(ValueError, match="dimensions must match"):
        la.Matrix([[1.0, 2.0], [3.0, 4.0]]).solve_array([1.0], trans=True)
    with pytest.raises(ValueError, match="norm must be 1 or inf"):
        la.Matrix([[1.0, 2.0], [3.0, 4.0]]).rcond(norm=2)


def test_new_symbols_are_bound():
    from linalg_solver_amd import _native

    for name in ("lsx_getrs_t_f64", "lsx_getrs_t_f32", "lsx_getrs_t_f64_dev", "lsx_getrs_t_f32_dev", "lsx_lange_f64_dev",
                 "lsx_lange_f32_dev", "lsx_gecon_f64", "lsx_gecon_f32", "lsx_gecon_f64_dev", "lsx_gecon_f32_dev",
                 "lsx_rcond_f64", "lsx_rcond_f32"):
        assert name in _native.EXPORTS
    assert (_native.NORM_ONE, _native.NORM_INF) == (0, 1)
