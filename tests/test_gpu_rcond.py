"""Condition estimate from the LU factors (lsx_gecon_* / lsx_rcond_*) on the MI355X against LAPACK's dgecon / sgecon
and the exact value, both recorded in tests/golden/rcond_cases.json (tests/golden/gen_rcond_golden.py).

Agreement bound per case: |rcond / rcond_lapack - 1| <= 64 n eps cond_1 (cpu_cond.bound): both sides run the same
iteration and differ through the rounding of their factors and solves only.  Against the exact value only the lower
side is asserted: the method bounds ||inv(A)|| from below, and LAPACK itself is up to 1.8 x optimistic on these cases.
"""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import cpu_cond  # noqa: E402

CASES = cpu_cond.load_cases()
REGULAR = [c for c in CASES if c["kind"] in ("u11", "int5", "u11_shift") and c["n"] > 1]
NORMS = (("1", 1), ("I", np.inf))


def _id(c):
    return f"{c['kind']}-{c['n']}-{c['prec']}"


def _case(kind, n):
    return next(c for c in CASES if c["kind"] == kind and c["n"] == n)


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


@pytest.mark.parametrize("case", REGULAR, ids=_id)
def test_rcond_agrees_with_lapack_and_bounds_the_exact_value(la, case):
    from linalg_solver_amd import dense

    dt = cpu_cond.DTYPE[case["prec"]]
    A = cpu_cond.matrix(case["kind"], case["n"], case["seed"]).astype(dt)
    bound = cpu_cond.bound(case)
    assert bound <= 0.35
    LU, ipiv, info = dense.lu_factor(A, dtype=dt)
    assert info == 0
    h = la.default_handle()
    for nm, which in NORMS:
        ref, exact = case["rcond_lapack"][nm], case["rcond_exact"][nm]
        rc, rinfo = dense.rcond(A, norm=which, dtype=dt)          # norm + factorisation + estimate in one call
        solves = h.get_option("gecon_solves")
        rc2 = dense.lu_rcond(LU, ipiv, case["anorm"][nm], norm=which)   # from existing factors, LAPACK's contract
        print(f"{_id(case)} norm {nm}: rcond {rc:.6e} from factors {rc2:.6e} lapack {ref:.6e} exact {exact:.6e} "
              f"|ratio-1| {abs(rc / ref - 1):.2e} bound {bound:.2e} solves {solves}")
        assert rinfo == 0
        assert abs(rc / ref - 1.0) <= bound
        assert abs(rc2 / ref - 1.0) <= bound
        assert rc >= exact * (1.0 - bound) and rc2 >= exact * (1.0 - bound)
        assert 4 <= solves <= 11 and 4 <= h.get_option("gecon_solves") <= 11     # 2 * 5 + 1 at most


def test_rcond_sees_what_the_pivot_ratio_misses(la):
    """1 on the diagonal, -1 above: every pivot is 1, the matrix is singular to working precision."""
    from linalg_solver_amd import dense

    for n in (40, 60, 100):
        case = _case("unit_upper", n)
        A = cpu_cond.matrix("unit_upper", n, case["seed"])
        for nm, which in NORMS:
            rc, info = dense.rcond(A, norm=which)
            print(f"unit_upper n={n} norm {nm}: rcond {rc!r} lapack {case['rcond_lapack'][nm]!r}")
            assert info == 0 and abs(rc / case["rcond_lapack"][nm] - 1.0) <= 1e-12
    A = cpu_cond.matrix("unit_upper", 60, 0)
    rc, _ = dense.rcond(A)
    x, info, ratio = dense.solve(A, np.ones(60))
    assert rc < 2.3e-16            # below eps: the digits of a solve are noise ...
    assert info == 0 and x is not None and ratio == 1.0   # ... and the pivot ratio calls the matrix perfectly regular
    assert la.Matrix.from_numpy(A).cond() > 1e19


def test_rcond_numerical_outcomes_are_values(la):
    from linalg_solver_amd import dense

    sing = _case("u11_zero_col", 64)
    A = cpu_cond.matrix("u11_zero_col", 64, sing["seed"])
    for which in (1, np.inf):
        assert dense.rcond(A, norm=which) == (0.0, 18)
        assert dense.rcond(A.astype(np.float32), norm=which, dtype=np.float32) == (0.0, 18)
    assert la.Matrix.from_numpy(A).rcond() == 0.0 and la.Matrix.from_numpy(A).cond() == math.inf
    LU, ipiv, info = dense.lu_factor(A)
    assert info == 18 and dense.lu_rcond(LU, ipiv, sing["anorm"]["1"]) == 0.0     # U_ii == 0 from existing factors
    assert dense.rcond(np.zeros((0, 0))) == (1.0, 0)
    assert dense.lu_rcond(np.zeros((0, 0)), np.zeros(0, dtype=np.int32), 0.0) == 1.0
    one = _case("u11", 1)
    A1 = cpu_cond.matrix("u11", 1, one["seed"])
    assert dense.rcond(A1)[0] == pytest.approx(1.0, rel=1e-15)
    assert dense.lu_rcond(np.eye(3), np.arange(3, dtype=np.int32), 0.0) == 0.0     # anorm == 0
    assert dense.rcond(np.zeros((3, 3))) == (0.0, 1)


def test_gecon_arguments(la):
    h = la.default_handle()
    lib = h.lib
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    LU, piv, rc = np.eye(4), np.arange(4, dtype=np.int32), C.c_double(-1.0)
    pLU, pP = LU.ctypes.data_as(dp), piv.ctypes.data_as(ip)
    assert lib.lsx_gecon_f64(h.ptr, 0, 4, pLU, 4, pP, float("nan"), C.byref(rc)) == -1 and b"anorm" in lib.lsx_last_error()
    assert lib.lsx_gecon_f64(h.ptr, 2, 4, pLU, 4, pP, 1.0, C.byref(rc)) == -1      # unknown norm
    assert lib.lsx_gecon_f64(h.ptr, 0, 4, pLU, 3, pP, 1.0, C.byref(rc)) == -1      # lda < n
    assert lib.lsx_gecon_f64(h.ptr, 0, 4, None, 4, pP, 1.0, C.byref(rc)) == -1
    assert lib.lsx_gecon_f64(h.ptr, 0, 4, pLU, 4, pP, 1.0, None) == -1
    assert lib.lsx_rcond_f64(h.ptr, 0, 4, None, 4, C.byref(rc), None) == -1
    assert lib.lsx_gecon_f64(h.ptr, 0, 4, pLU, 4, pP, 1.0, C.byref(rc)) == 0 and rc.value == 1.0   # the identity
    assert lib.lsx_gecon_f64(h.ptr, 1, 0, None, 0, None, 0.0, C.byref(rc)) == 0 and rc.value == 1.0


@pytest.mark.parametrize("kind,n", [("u11", 300), ("int5", 1000), ("u11", 2048)])
def test_rcond_on_device_tensors(la, dev, kind, n):
    """Matrix.from_dlpack(tensor).rcond() and DeviceSolver.norm / .rcond on factors with lda > n."""
    import torch

    case = _case(kind, n)
    A = cpu_cond.matrix(kind, n, case["seed"])
    bound = cpu_cond.bound(case)
    t = torch.from_numpy(A).cuda()
    host = la.Matrix.from_numpy(A).rcond()
    for nm, which in NORMS:
        ref = case["rcond_lapack"][nm]
        rc_dl = la.Matrix.from_dlpack(t).rcond(norm=which)
        LUp = torch.zeros(n, n + 8, dtype=torch.float64, device="cuda")
        LU = LUp[:, :n]
        LU.copy_(t)
        anorm = dev.norm(LU, which)
        ipiv, info = dev.getrf_(LU)
        rc_dev = dev.rcond(LU, ipiv, anorm, norm=which)
        print(f"{kind} n={n} norm {nm}: dlpack {rc_dl:.6e} device {rc_dev:.6e} lapack {ref:.6e}")
        assert int(info.item()) == 0
        assert abs(rc_dl / ref - 1.0) <= bound and abs(rc_dev / ref - 1.0) <= bound
        assert 4 <= dev.h.get_option("gecon_solves") <= 11
        if nm == "1":
            assert abs(rc_dl / host - 1.0) <= bound
    assert la.Matrix.from_dlpack(t).cond() == pytest.approx(1.0 / la.Matrix.from_dlpack(t).rcond(), rel=1e-12)
