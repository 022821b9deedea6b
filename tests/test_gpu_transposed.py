"""Transposed solves A^T X = B from the factors of A (lsx_getrs_t_*) and the matrix norms (lsx_lange_*_dev) on the
MI355X, through the C ABI.  Tolerances are those of tests/test_gpu_parity.py: fp64 1e-9 relative, fp32 1e-4,
residual 1e-9 n, variant against variant 1e-11.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from helpers import relerr  # noqa: E402

TOL64 = 1e-9
TOL32 = 1e-4

ORDERS = [1, 5, 64, 128, 129, 300, 1000, 2048, 2100]
NRHS = [1, 2, 3, 8, 9, 40]


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


_FACTORS = {}


def _system(n):
    """A, the library's factors of it, and right-hand sides (40 columns; tests take the leading ones)."""
    from linalg_solver_amd import dense, gen

    if n not in _FACTORS:
        A, _ = gen.system(gen.U11, 1300 + n, n)
        B = gen.fill(gen.U11, 2300 + n, n, 40)
        LU, ipiv, info = dense.lu_factor(A)
        assert info == 0
        _FACTORS[n] = (A, B, LU, ipiv)
    return _FACTORS[n]


def _perm(ipiv):
    p = np.arange(len(ipiv))
    for k, q in enumerate(ipiv):
        p[k], p[q] = p[q], p[k]
    return p   # (P b)[i] = b[p[i]]


def _cpu_transposed_from_factors(LU, ipiv, B):
    """Substitution on the given factors: U^T y = b, L^T z = y, x[perm] = z."""
    from scipy.linalg import solve_triangular as trs

    Z = trs(LU, trs(LU, B, lower=False, trans=1), lower=True, unit_diagonal=True, trans=1)
    X = np.empty_like(Z)
    X[_perm(ipiv)] = Z
    return X


@pytest.mark.parametrize("n", ORDERS)
@pytest.mark.parametrize("nrhs", NRHS)
def test_transposed_solve_fp64(la, n, nrhs):
    from linalg_solver_amd import dense

    A, B40, LU, ipiv = _system(n)
    B = np.ascontiguousarray(B40[:, :nrhs])
    X = dense.lu_solve(LU, ipiv, B, trans=True)
    X2 = dense.lu_solve(LU, ipiv, B, trans=True)
    ref = np.linalg.solve(A.T, B)
    own = _cpu_transposed_from_factors(LU, ipiv, B)
    e_ref, e_own, res = relerr(X, ref), relerr(X, own), float(np.max(np.abs(A.T @ X - B)))
    print(f"n={n} nrhs={nrhs}: vs numpy {e_ref:.2e}  vs substitution on own factors {e_own:.2e}  residual {res:.2e}")
    assert X.shape == B.shape and np.array_equal(X, X2), "two calls must give identical bits"
    assert e_ref < TOL64
    assert e_own < 1e-11
    assert res < 1e-9 * n


@pytest.mark.parametrize("n,nrhs", [(300, 1), (1000, 4), (2048, 1)])
def test_transposed_solve_fp32(la, n, nrhs):
    from linalg_solver_amd import dense, gen

    A, _ = gen.system(gen.U11, 950 + n, n)
    B = np.random.default_rng(n).uniform(-1, 1, (n, nrhs))
    LU, ipiv, info = dense.lu_factor(A.astype(np.float32), dtype=np.float32)
    assert info == 0
    x = dense.lu_solve(LU, ipiv, B.astype(np.float32), trans=True)
    assert x.dtype == np.float32 and np.array_equal(x, dense.lu_solve(LU, ipiv, B.astype(np.float32), trans=True))
    # norm-wise backward error of the fp32 solve (the formula of test_cooperative_triangular_solve_fp32)
    resid = np.linalg.norm(A.T @ x.astype(np.float64) - B) / (np.linalg.norm(A) * np.linalg.norm(x) + np.linalg.norm(B))
    print(f"fp32 n={n} nrhs={nrhs}: backward error {resid:.2e}")
    assert resid < TOL32


@pytest.mark.parametrize("n", [5, 128, 300, 1000])
def test_transposed_equals_solve_with_the_transposed_matrix(la, n):
    from linalg_solver_amd import dense

    A, B40, LU, ipiv = _system(n)
    B = np.ascontiguousarray(B40[:, :3])
    LUt, ipivt, info = dense.lu_factor(A.T.copy())
    assert info == 0
    assert relerr(dense.lu_solve(LU, ipiv, B, trans=True), dense.lu_solve(LUt, ipivt, B)) < TOL64
    Xs, sinfo, ratio = dense.solve(A, B, trans=True)
    assert sinfo == 0 and ratio > 0 and relerr(Xs, np.linalg.solve(A.T, B)) < TOL64
    # the Matrix front end, vector and matrix right-hand sides
    m = la.Matrix.from_numpy(A)
    assert relerr(m.solve_array(B, trans=True), np.linalg.solve(A.T, B)) < TOL64
    assert relerr(m.solve_array(B[:, 0], trans=True), np.linalg.solve(A.T, B[:, 0])) < TOL64
    assert relerr(m.solve_array(B), np.linalg.solve(A, B)) < TOL64   # the default is the plain solve, as before


@pytest.mark.parametrize("n", [7, 128, 129, 300])
def test_scatter_not_gather(la, n):
    """Matrices whose interchanges are not an involution: a gather where the scatter belongs gives a wrong answer."""
    from linalg_solver_amd import dense, gen

    rng = np.random.default_rng(n)
    B = rng.uniform(-1, 1, (n, 2))
    Pm = np.eye(n)[rng.permutation(n)]                          # a permutation matrix: x = P b exactly
    LU, ipiv, info = dense.lu_factor(Pm)
    assert info == 0
    assert np.array_equal(dense.lu_solve(LU, ipiv, B, trans=True), Pm @ B)
    assert np.array_equal(dense.lu_solve(LU, ipiv, B), Pm.T @ B)
    R = np.eye(n)[::-1] + 1e-3 * gen.fill(gen.U11, 77 + n, n, n)   # an interchange in every column
    LU, ipiv, info = dense.lu_factor(R)
    assert info == 0 and int((ipiv != np.arange(n)).sum()) >= n // 2
    assert relerr(dense.lu_solve(LU, ipiv, B, trans=True), np.linalg.solve(R.T, B)) < TOL64


@pytest.mark.parametrize("n", [100, 300, 1000])
def test_transposed_solve_on_device_pointers_with_padding(dev, n):
    """lda > n and ldb > nrhs through the _dev form, on torch's current stream."""
    import torch

    A, B40, _, _ = _system(n)
    nrhs = 5
    LUp = torch.zeros(n, n + 24, dtype=torch.float64, device="cuda")
    LU = LUp[:, :n]
    LU.copy_(torch.from_numpy(A))
    ipiv, info = dev.getrf_(LU)
    Bp = torch.full((n, nrhs + 3), 7.0, dtype=torch.float64, device="cuda")
    Bv = Bp[:, :nrhs]
    Bv.copy_(torch.from_numpy(B40[:, :nrhs]))
    dev.getrs_(LU, ipiv, Bv, trans=True)      # enqueued on torch's current stream: the torch ops below are ordered behind it
    assert int(info.item()) == 0
    assert relerr(Bv.cpu().numpy(), np.linalg.solve(A.T, B40[:, :nrhs])) < TOL64
    assert bool((Bp[:, nrhs:] == 7.0).all()), "the padding columns of B must not be touched"
    # plain after transposed and the reverse on one handle: the two share their work space
    X1 = torch.from_numpy(B40[:, :2].copy()).cuda()
    dev.getrs_(LU, ipiv, X1)
    X2 = torch.from_numpy(B40[:, :2].copy()).cuda()
    dev.getrs_(LU, ipiv, X2, trans=True)
    X3 = torch.from_numpy(B40[:, :2].copy()).cuda()
    dev.getrs_(LU, ipiv, X3)
    torch.cuda.synchronize()
    assert relerr(X1.cpu().numpy(), np.linalg.solve(A, B40[:, :2])) < TOL64
    assert relerr(X2.cpu().numpy(), np.linalg.solve(A.T, B40[:, :2])) < TOL64
    assert torch.equal(X1, X3)


def test_transposed_solve_arguments(la):
    h = la.default_handle()
    lib = h.lib
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    LU = np.eye(4)
    piv = np.arange(4, dtype=np.int32)
    B = np.ones((4, 2))
    pLU, pP, pB = LU.ctypes.data_as(dp), piv.ctypes.data_as(ip), B.ctypes.data_as(dp)
    assert lib.lsx_getrs_t_f64(h.ptr, 4, 2, pLU, 3, pP, pB, 2) == -1 and b"bad argument" in lib.lsx_last_error()   # lda < n
    assert lib.lsx_getrs_t_f64(h.ptr, 4, 2, pLU, 4, pP, pB, 1) == -1 and b"bad argument" in lib.lsx_last_error()   # ldb < nrhs
    assert lib.lsx_getrs_t_f64(h.ptr, 4, 2, None, 4, pP, pB, 2) == -1 and b"bad argument" in lib.lsx_last_error()
    assert lib.lsx_getrs_t_f64(h.ptr, 4, 2, pLU, 4, None, pB, 2) == -1
    assert lib.lsx_getrs_t_f64(h.ptr, 4, 2, pLU, 4, pP, None, 2) == -1
    assert lib.lsx_getrs_t_f64_dev(h.ptr, 4, 2, None, 4, None, None, 2) == -1
    assert lib.lsx_getrs_t_f64(h.ptr, 0, 2, None, 0, None, None, 2) == 0      # nothing to do
    assert lib.lsx_getrs_t_f64(h.ptr, 4, 0, pLU, 4, pP, None, 0) == 0
    assert lib.lsx_getrs_t_f32(h.ptr, 0, 0, None, 0, None, None, 0) == 0
    assert lib.lsx_getrs_t_f64(h.ptr, 4, 2, pLU, 4, pP, pB, 2) == 0 and np.array_equal(B, np.ones((4, 2)))


@pytest.mark.parametrize("m,n", [(1, 1), (5, 7), (129, 64), (1000, 1000), (2048, 2100)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_matrix_norms(dev, m, n, dtype):
    import torch

    from linalg_solver_amd import gen

    A = gen.fill(gen.U11, 40 + m, m, n, dtype=dtype)
    Ap = torch.full((m, n + 9), 1e30, dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda")
    Av = Ap[:, :n]                                             # lda > n; the padding must not be read
    Av.copy_(torch.from_numpy(A))
    a64 = np.abs(A.astype(np.float64))
    eps = float(np.finfo(np.float64).eps)                       # sums are accumulated in fp64 for both types
    for which, ref in ((1, a64.sum(axis=0).max()), (np.inf, a64.sum(axis=1).max())):
        v1, v2 = dev.norm(Av, which), dev.norm(Av, which)
        torch.cuda.synchronize()
        v = float(v1.item())
        print(f"norm {which} of {m}x{n} {np.dtype(dtype).name}: {v!r} numpy {ref!r}")
        assert abs(v - ref) <= 4 * max(m, n) * eps * ref
        assert v == float(v2.item())


def test_norm_front_ends_and_edge_cases(la, dev):
    import torch

    from linalg_solver_amd import dense, gen

    A = gen.fill(gen.INT5, 3, 33, 21)
    assert dense.norm(A, 1) == np.abs(A).sum(axis=0).max() and dense.norm(A, np.inf) == np.abs(A).sum(axis=1).max()
    assert dense.norm(np.zeros((0, 3))) == 0.0
    An = A.copy()
    An[4, 5] = np.nan
    assert np.isnan(dense.norm(An, 1)) and np.isnan(dense.norm(An, np.inf))
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    assert dev.lib.lsx_lange_f64_dev(dev.h.ptr, 2, 3, 3, out.data_ptr(), 3, out.data_ptr()) == -1   # unknown norm
    assert dev.lib.lsx_lange_f64_dev(dev.h.ptr, 0, 3, 3, out.data_ptr(), 2, out.data_ptr()) == -1   # lda < n
