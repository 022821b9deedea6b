"""The yardsticks of the Cholesky tests, proved on the CPU before the GPU is asked (tests/test_gpu_chol.py):
LAPACK (scipy's dpotrf / spotrf) and the numpy model of the kernels (tests/cpu_chol.py) return the planted factors
exactly, report the planted failures with LAPACK's info and prefix, and stay inside Higham's bounds on the rounded
inputs -- the model too, although its explicit block inverses do not formally satisfy the theorem.
"""
import numpy as np
import pytest
from scipy.linalg import lapack

import cpu_chol as cc

ORDERS = [1, 2, 64, 127, 128, 129, 257, 384, 512, 600]
DTYPES = [np.float64, np.float32]
ROUNDED = [129, 300, 600]
FAIL_ROWS = [0, 5, 127, 128, 300]


def _lapack_potrf(A):
    fn = lapack.dpotrf if A.dtype == np.float64 else lapack.spotrf
    c, info = fn(A, lower=0, clean=1)
    return c, info


def _lapack_potrs(U, B):
    fn = lapack.dpotrs if U.dtype == np.float64 else lapack.spotrs
    x, info = fn(U, B, lower=0)
    assert info == 0
    return x


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", ORDERS)
def test_planted_factor_is_returned_exactly(n, dtype):
    U, A = cc.planted(n, cc.PLANTED_SEED, dtype)
    c, info = _lapack_potrf(A)
    assert info == 0 and np.array_equal(np.triu(c), U), "LAPACK"
    R, info = cc.potrf(cc.fill_lower(A, np.nan))
    assert info == 0 and np.array_equal(np.triu(R), U), "the model of the kernels"
    assert np.isnan(R[np.tril_indices(n, -1)]).all(), "the model never touches the lower triangle"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [64, 128, 100])
def test_planted_block_inverse_is_exact(n, dtype):
    """inv(U11) as the diagonal-block kernel forms it: exact in fp64 on the planted blocks (V U = I with no rounding
    anywhere); in fp32 a few entries need more than 24 bits and come out within one rounding of the exact inverse."""
    U, A = cc.planted(n, cc.PLANTED_SEED, dtype)
    U11, V, done = cc.diag_block(A)
    assert done == n and np.array_equal(U11, U)
    _, V64, _ = cc.diag_block(A.astype(np.float64))
    assert np.array_equal(V64 @ U.astype(np.float64), np.eye(n)), "the fp64 inverse is exact"
    if dtype == np.float64:
        assert np.array_equal(V, V64)
    else:
        assert np.all(np.abs(V.astype(np.float64) - V64) <= 2.0 ** -24 * np.abs(V64) * 4)
    assert np.array_equal(np.tril(V, -1), np.zeros_like(V))
    _, V2, _ = cc.diag_block(U, factored=True)
    assert np.array_equal(V2, V)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["zero", "negative", "nan"])
@pytest.mark.parametrize("j", FAIL_ROWS)
def test_not_positive_definite_info_and_prefix(j, kind, dtype):
    n = 384
    U, A = cc.planted_not_pd(n, j, kind, cc.PLANTED_SEED, dtype)
    if kind != "nan":     # (dpotf2 tests the pivot with disnan; the optimised potrf behind scipy may not: no claim there)
        c, info = _lapack_potrf(A)
        assert info == j + 1, "LAPACK"
        assert np.array_equal(np.triu(c)[:j, :j], U[:j, :j])
    R, info = cc.potrf(A)
    assert info == j + 1, "the model"
    assert np.array_equal(np.triu(R)[:j, :j], U[:j, :j])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", ROUNDED)
def test_rounded_inputs_stay_inside_highams_bounds(n, dtype):
    """A = G G^T / n + I.  Factor: max |A - U^T U| / (|U^T| |U|) <= gamma_{n+1}; solve: max |b - A x| / (|U^T| |U| |x|)
    <= gamma_{3n+1}.  Both for LAPACK and for the model on exactly the inputs the GPU gets."""
    A = cc.spd(n, 0, dtype)
    B = np.random.default_rng(n).standard_normal((n, 7)).astype(dtype)
    u = cc.UNIT[np.dtype(dtype)]
    for name, factor, solve in (("lapack", lambda a: _lapack_potrf(a), _lapack_potrs),
                                ("model", lambda a: cc.potrf(a), cc.potrs)):
        R, info = factor(A.copy())
        assert info == 0
        fr = cc.factor_residual(A, R)
        X = solve(R, B)
        sr = cc.solve_residual(A, R, B, X)
        print(f"{name} n={n} {np.dtype(dtype).name}: factor {fr / u:.2f} u (bound {cc.gamma(n + 1, dtype) / u:.0f} u), "
              f"solve {sr / u:.2f} u (bound {cc.gamma(3 * n + 1, dtype) / u:.0f} u)")
        assert fr <= cc.gamma(n + 1, dtype), name
        assert sr <= cc.gamma(3 * n + 1, dtype), name


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,nrhs", [(1, 1), (129, 7), (257, 64), (600, 3)])
def test_model_solve_on_planted_factors(n, nrhs, dtype):
    """potrs of the model against the planted system with an integer solution: U^T U X = B is solved to the working
    precision (small integers: the products are exact, the block inverses are not integers)."""
    U, A = cc.planted(n, cc.PLANTED_SEED, dtype)
    X = np.random.default_rng(n + nrhs).integers(-3, 4, (n, nrhs)).astype(dtype)
    B = (A.astype(np.float64) @ X.astype(np.float64)).astype(dtype)
    got = cc.potrs(cc.fill_lower(U, np.nan), B)
    assert not np.isnan(got).any()
    assert cc.solve_residual(A, U, B, got) <= cc.gamma(3 * n + 1, dtype)
