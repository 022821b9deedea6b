"""The blocked transposed solve on the CPU (tests/cpu_trsmt.py): the algorithm of the device path, on the inputs of
tests/test_gpu_transposed_blocked.py, held to that test's bounds.  What the algorithm itself cannot meet, no kernel
can; what it meets here with margin is a fair demand on the device.  No GPU.
"""
import numpy as np
import pytest

import cpu_trsmt as T
from helpers import relerr


def _factors(A):
    from scipy.linalg import lu_factor

    LU, ipiv = lu_factor(A)
    return np.ascontiguousarray(LU), ipiv.astype(np.int32)


@pytest.mark.parametrize("n", T.ORDERS)
def test_blocked_sweeps_fp64_within_the_device_bounds(n):
    A, B = T.system(n)
    B = np.ascontiguousarray(B[:, :72])
    LU, ipiv = _factors(A)
    X = T.blocked_transposed_solve(LU, ipiv, B)
    e_ref = relerr(X, np.linalg.solve(A.T, B))
    e_own = relerr(X, T.substitution(LU, ipiv, B))
    res = float(np.max(np.abs(A.T @ X - B)))
    print(f"n={n}: vs numpy {e_ref:.2e}  vs substitution on the same factors {e_own:.2e}  residual {res:.2e}")
    assert e_ref < T.TOL_NUMPY
    assert e_own < T.TOL_FACTORS
    assert res < T.TOL_RESID * n


@pytest.mark.parametrize("n,nrhs", [(300, 64), (1000, 72), (2048, 130)])
def test_blocked_sweeps_fp32_backward_error(n, nrhs):
    A, B = T.system32(n, nrhs)
    LU, ipiv = _factors(A.astype(np.float32))
    assert LU.dtype == np.float32
    X = T.blocked_transposed_solve(LU, ipiv, B.astype(np.float32))
    berr = T.backward_error32(A, X, B)
    print(f"fp32 n={n} nrhs={nrhs}: backward error {berr:.2e}")
    assert X.dtype == np.float32 and berr < T.TOL32


@pytest.mark.parametrize("n", [129, 300])
def test_twin_scatters(n):
    """LU = I with interchanges that are no involution: the twin multiplies by ones and must return Pm @ B exactly."""
    rng = np.random.default_rng(n)
    B = rng.uniform(-1, 1, (n, 5))
    Pm = np.eye(n)[rng.permutation(n)]
    LU, ipiv = _factors(Pm)
    assert np.array_equal(T.blocked_transposed_solve(LU, ipiv, B), Pm @ B)


def test_single_column_and_ragged_widths():
    A, B = T.system(257)
    LU, ipiv = _factors(A)
    for w in (1, 7, 65):
        X = T.blocked_transposed_solve(LU, ipiv, B[:, :w])
        assert X.shape == (257, w) and relerr(X, T.substitution(LU, ipiv, B[:, :w])) < T.TOL_FACTORS
