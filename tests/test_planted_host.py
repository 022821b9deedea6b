"""The planted-factorisation oracle (tests/planted.py) proved on the CPU before the GPU is held to it: the
construction is exact in fp32, and three independent eliminations (the C twin oracle/lu_twin.c in fp64, a numpy
elimination in fp32 and in fp64, LAPACK's sgetrf / dgetrf through scipy) return the planted factors and the planted
interchange sequence bit for bit.
"""
import numpy as np
import pytest

import planted as pl

ORDERS = (1, 2, 3, 64, 65, 129, 300, 1000)
# every order tests/test_gpu_planted.py uses up to 2048
GPU_ORDERS_TO_2048 = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 1000, 1537, 2048)


@pytest.mark.parametrize("n", ORDERS + (2048,))
def test_planted_matrix_is_exact(n):
    A, L, U, perm = pl.planted(n, 7)
    assert np.array_equal(A.astype(np.float32).astype(np.float64), A), "A must survive the round trip through fp32"
    assert np.array_equal(A * 4, np.round(A * 4)) and np.max(np.abs(A)) < 2 ** 10    # multiples of 1/4, small
    assert np.array_equal(A[perm], L @ U)
    # the same product accumulated in fp32 and in another order: still exact
    assert np.array_equal((L.astype(np.float32) @ U.astype(np.float32)).astype(np.float64), A[perm])
    assert np.array_equal((U.T @ L.T).T, A[perm])
    assert np.array_equal(np.diag(L), np.ones(n)) and np.all(np.abs(np.tril(L, -1)) <= 0.5) and np.all(np.triu(L, 1) == 0)
    assert np.all(np.isin(np.abs(np.diag(U)), (4.0, 8.0))) and np.all(np.tril(U, -1) == 0)
    assert np.all(np.abs(np.triu(U, 1)) <= 3) and np.array_equal(U, np.round(U))
    assert sorted(perm.tolist()) == list(range(n))


@pytest.mark.parametrize("n", (1, 2, 5, 64, 300))
def test_interchange_sequence_realises_the_permutation(n):
    rng = np.random.default_rng(n)
    for _ in range(5):
        perm = rng.permutation(n)
        ipiv = pl.ipiv_of_perm(perm)
        assert ipiv.dtype == np.int32 and np.all(ipiv >= np.arange(n)) and np.all(ipiv < n)
        assert np.array_equal(pl.perm_of_ipiv(ipiv), perm)
        rows = np.arange(n)
        for k, p in enumerate(ipiv):     # the sequential definition
            rows[[k, p]] = rows[[p, k]]
        assert np.array_equal(rows, perm)
        if n <= 64:
            assert pl.perm_sign(perm) == round(np.linalg.det(np.eye(n)[perm]))
        assert pl.perm_sign(perm) == (-1.0) ** int((ipiv != np.arange(n)).sum())


@pytest.mark.parametrize("n", ORDERS)
def test_cpu_eliminations_reproduce_the_planted_factors(n):
    import scipy.linalg as sl

    from oracle import capi

    A, L, U, perm = pl.planted(n, 11)
    want_lu, want_piv = pl.planted_lu(L, U), pl.ipiv_of_perm(perm)
    LU, ipiv, info = capi.getrf(A)
    assert info == 0 and np.array_equal(ipiv, want_piv) and np.array_equal(LU, want_lu)
    for dtype in (np.float32, np.float64):
        LU, ipiv, info = pl.eliminate(A, dtype)
        assert LU.dtype == dtype and info == 0
        assert np.array_equal(ipiv, want_piv), f"{np.dtype(dtype).name}: first differing column {int(np.nonzero(ipiv != want_piv)[0][0])}"
        assert np.array_equal(LU.astype(np.float64), want_lu)
        getrf, = sl.get_lapack_funcs(("getrf",), (np.zeros(1, dtype=dtype),))
        LU, piv, info = getrf(A.astype(dtype))
        assert info == 0 and np.array_equal(piv, want_piv) and np.array_equal(LU.astype(np.float64), want_lu)


@pytest.mark.parametrize("n,k", [(300, 5), (300, 200), (300, 299), (65, 64), (1, 0)])
def test_planted_zero_pivot(n, k):
    from oracle import capi

    A, L, U, perm = pl.planted(n, 13, zero_at=k)
    assert U[k, k] == 0 and np.array_equal(A[perm], L @ U)
    want = pl.ipiv_of_perm(perm)
    _, ipiv, info = capi.getrf(A)
    assert info == k + 1 and np.array_equal(ipiv[:k], want[:k])
    for dtype in (np.float32, np.float64):
        _, ipiv, info = pl.eliminate(A, dtype)
        assert info == k + 1 and np.array_equal(ipiv[:k], want[:k])


@pytest.mark.parametrize("n", GPU_ORDERS_TO_2048)
def test_planted_factors_are_well_conditioned(n):
    """A condition on the inputs: the GPU test must not be able to fail for a reason other than the kernels."""
    for seed in (11, 13):      # the seeds of tests/test_gpu_planted.py
        L, U, _ = pl.planted_factors(n, seed)
        cl, cu = pl.cond_inf_triangular(L, True), pl.cond_inf_triangular(U, False)
        assert cl < 1e5 and cu < 1e5, (n, seed, cl, cu)


@pytest.mark.parametrize("n,j,rows", [(300, 0, (0, 299)), (400, 128, (255, 256)), (300, 5, (1, 294)),
                                       (200, 127, tuple(range(73)))])
@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_tie_matrix_pivots(n, j, rows, dtype):
    A = pl.tie_matrix(n, j, rows, 3, dtype)
    assert np.array_equal(A.astype(dtype).astype(np.float64), A)
    col = np.abs(A[j:, j])
    assert np.array_equal(np.nonzero(col == col.max())[0], np.array(sorted(rows))) and len(set(A[j:, j][list(rows)])) == min(2, len(rows))
    LU, ipiv, info = pl.eliminate(A, dtype)
    assert info == 0 and np.array_equal(ipiv[:j], np.arange(j)) and ipiv[j] == j + min(rows)
