"""The blocked transposed solve for many right-hand sides (lsx_getrs_t_* with nrhs >= "getrs_t_blocked_min", n > 128) on
the MI355X: the assertions of tests/test_gpu_transposed.py on the new path, path against path, column independence,
the scatter, padded device views, every front end and the two options.  Inputs and bounds: tests/cpu_trsmt.py, where
tests/test_trsmt_host.py shows the algorithm itself inside them.  Every test sets the option it needs and the previous
value comes back afterwards.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import cpu_trsmt as T  # noqa: E402
from helpers import relerr  # noqa: E402


@pytest.fixture(scope="module")
def la():
    import linalg_solver_amd as la

    la.default_handle()
    return la


@pytest.fixture
def blocked_min(la):
    """Setter of "getrs_t_blocked_min" on the default handle; the value found there is restored."""
    h = la.default_handle()
    before = h.get_option("getrs_t_blocked_min")
    yield lambda v: h.set_option("getrs_t_blocked_min", v)
    h.set_option("getrs_t_blocked_min", before)


@pytest.fixture(scope="module")
def dev():
    import torch

    from linalg_solver_amd.device import DeviceSolver

    assert torch.cuda.is_available()
    return DeviceSolver()


def _path(handle) -> int:
    return handle.get_option("getrs_t_path")


_FACTORS = {}


def _system(n):
    """A, right-hand sides, and the library's own factors of A, computed once per order and never written."""
    from linalg_solver_amd import dense

    if n not in _FACTORS:
        A, B = T.system(n)
        LU, ipiv, info = dense.lu_factor(A)
        assert info == 0
        for a in (A, B, LU, ipiv):
            a.setflags(write=False)
        _FACTORS[n] = (A, B, LU, ipiv)
    return _FACTORS[n]


_CASES = [(n, nrhs, 64) for n in T.ORDERS for nrhs in (64, 65, 72, 130, 256)] + \
         [(n, nrhs, 1) for n in T.ORDERS for nrhs in (1, 7)]


@pytest.mark.parametrize("n,nrhs,option", _CASES)
def test_blocked_transposed_solve_fp64(la, blocked_min, n, nrhs, option):
    from linalg_solver_amd import dense

    A, Ball, LU, ipiv = _system(n)
    B = np.ascontiguousarray(Ball[:, :nrhs])
    blocked_min(option)
    X = dense.lu_solve(LU, ipiv, B, trans=True)
    assert _path(la.default_handle()) == 1
    X2 = dense.lu_solve(LU, ipiv, B, trans=True)
    assert _path(la.default_handle()) == 1
    ref = np.linalg.solve(A.T, B)
    own = T.substitution(LU, ipiv, B)
    e_ref, e_own, res = relerr(X, ref), relerr(X, own), float(np.max(np.abs(A.T @ X - B)))
    print(f"n={n} nrhs={nrhs}: vs numpy {e_ref:.2e}  vs substitution on own factors {e_own:.2e}  residual {res:.2e}")
    assert X.shape == B.shape and np.array_equal(X, X2), "two calls must give identical bits"
    assert e_ref < T.TOL_NUMPY
    assert e_own < T.TOL_FACTORS
    assert res < T.TOL_RESID * n


@pytest.mark.parametrize("n,nrhs", [(129, 64), (300, 72), (1000, 130), (2100, 65)])
def test_blocked_against_grouped(la, blocked_min, n, nrhs):
    """The two paths on the same call: different summation orders, the variant-against-variant bound."""
    from linalg_solver_amd import dense

    _, Ball, LU, ipiv = _system(n)
    B = np.ascontiguousarray(Ball[:, :nrhs])
    blocked_min(0)
    Xg = dense.lu_solve(LU, ipiv, B, trans=True)
    assert _path(la.default_handle()) == 0
    blocked_min(64)
    Xb = dense.lu_solve(LU, ipiv, B, trans=True)
    assert _path(la.default_handle()) == 1
    e = relerr(Xb, Xg)
    print(f"n={n} nrhs={nrhs}: blocked against grouped {e:.2e}")
    assert e < T.TOL_FACTORS


@pytest.mark.parametrize("n", [257, 1000])
def test_a_column_does_not_depend_on_its_neighbours(la, blocked_min, n):
    from linalg_solver_amd import dense

    _, Ball, LU, ipiv = _system(n)
    blocked_min(64)
    wide = dense.lu_solve(LU, ipiv, np.ascontiguousarray(Ball[:, :200]), trans=True)
    assert _path(la.default_handle()) == 1
    part = dense.lu_solve(LU, ipiv, np.ascontiguousarray(Ball[:, :64]), trans=True)
    assert _path(la.default_handle()) == 1
    assert np.array_equal(part, wide[:, :64])


@pytest.mark.parametrize("n,nrhs", [(300, 64), (1000, 72), (2048, 130)])
def test_blocked_transposed_solve_fp32(la, blocked_min, n, nrhs):
    from linalg_solver_amd import dense

    A, B = T.system32(n, nrhs)
    LU, ipiv, info = dense.lu_factor(A.astype(np.float32), dtype=np.float32)
    assert info == 0
    blocked_min(64)
    x = dense.lu_solve(LU, ipiv, B.astype(np.float32), trans=True)
    assert _path(la.default_handle()) == 1
    x2 = dense.lu_solve(LU, ipiv, B.astype(np.float32), trans=True)
    assert x.dtype == np.float32 and np.array_equal(x, x2)
    berr = T.backward_error32(A, x, B)
    print(f"fp32 n={n} nrhs={nrhs}: backward error {berr:.2e}")
    assert berr < T.TOL32


@pytest.mark.parametrize("n", [129, 300])
def test_scatter_not_gather_on_the_blocked_path(la, blocked_min, n):
    """LU = I with interchanges that are no involution: products with ones and exact zeros, so x = P b exactly -- and a
    gather where the scatter belongs gives another matrix."""
    from linalg_solver_amd import dense

    rng = np.random.default_rng(n)
    B = rng.uniform(-1, 1, (n, 72))
    Pm = np.eye(n)[rng.permutation(n)]
    LU, ipiv, info = dense.lu_factor(Pm)
    assert info == 0 and not np.array_equal(Pm @ B, Pm.T @ B)
    blocked_min(64)
    X = dense.lu_solve(LU, ipiv, B, trans=True)
    assert _path(la.default_handle()) == 1
    assert np.array_equal(X, Pm @ B)


@pytest.mark.parametrize("n", [300, 1000])
def test_device_pointers_with_padding(dev, n):
    """lda > n, ldb > nrhs and an odd element offset (the bounds-checked tiles), NaN beside LU, 7.0 beside B, on torch's
    current stream: same bits as the aligned call, padding untouched."""
    import torch

    A, Ball, _, _ = _system(n)
    nrhs = 72
    before = dev.h.get_option("getrs_t_blocked_min")
    dev.h.set_option("getrs_t_blocked_min", 64)
    try:
        LU = torch.from_numpy(A.copy()).cuda()
        ipiv, info = dev.getrf_(LU)
        ref = torch.from_numpy(np.ascontiguousarray(Ball[:, :nrhs])).cuda()
        dev.getrs_(LU, ipiv, ref, trans=True)
        assert _path(dev.h) == 1
        lda, ldb = n + 25, nrhs + 3                      # odd
        bufLU = torch.full((1 + n * lda,), float("nan"), dtype=torch.float64, device="cuda")
        LUv = bufLU[1:].view(n, lda)[:, :n]
        LUv.copy_(LU)
        bufB = torch.full((1 + n * ldb,), 7.0, dtype=torch.float64, device="cuda")
        Bp = bufB[1:].view(n, ldb)
        Bv = Bp[:, :nrhs]
        Bv.copy_(torch.from_numpy(np.ascontiguousarray(Ball[:, :nrhs])))
        dev.getrs_(LUv, ipiv, Bv, trans=True)
        assert _path(dev.h) == 1
        torch.cuda.synchronize()
        assert int(info.item()) == 0
        assert torch.equal(Bv, ref), "the padded view must get the bits of the aligned call"
        assert bool((Bp[:, nrhs:] == 7.0).all()) and float(bufB[0]) == 7.0, "the padding of B must not be touched"
        assert relerr(Bv.cpu().numpy(), np.linalg.solve(A.T, Ball[:, :nrhs])) < T.TOL_NUMPY
    finally:
        dev.h.set_option("getrs_t_blocked_min", before)


def test_front_ends(la, dev, blocked_min, monkeypatch):
    """One case each, n = 300 and 72 columns with the option at 64."""
    import torch

    import linalg_solver_amd.device as device_mod
    from linalg_solver_amd import dense

    n, nrhs = 300, 72
    A, Ball, LU, ipiv = _system(n)
    B = np.ascontiguousarray(Ball[:, :nrhs])
    ref = np.linalg.solve(A.T, B)
    h = la.default_handle()
    blocked_min(64)

    X = dense.lu_solve(LU, ipiv, B, trans=True)
    assert _path(h) == 1 and relerr(X, ref) < T.TOL_NUMPY
    dense.lu_solve(LU, ipiv, B[:, :3], trans=True)
    assert _path(h) == 0                                   # the read-back follows the last call
    Xs, sinfo, ratio = dense.solve(A, B, trans=True)
    assert _path(h) == 1 and sinfo == 0 and ratio > 0 and np.array_equal(Xs, X)

    m = la.Matrix.from_numpy(A)
    h.set_option("getrs_t_blocked_min", 0)
    dense.lu_solve(LU, ipiv, B, trans=True)
    h.set_option("getrs_t_blocked_min", 64)
    Xm = m.solve_array(B, trans=True)                      # host operands: the default handle
    assert _path(h) == 1 and np.array_equal(np.asarray(Xm), X)

    before = dev.h.get_option("getrs_t_blocked_min")
    dev.h.set_option("getrs_t_blocked_min", 64)
    try:
        tLU, tB = torch.from_numpy(LU.copy()).cuda(), torch.from_numpy(B).cuda()
        dev.getrs_(tLU, torch.from_numpy(ipiv.copy()).cuda(), tB, trans=True)
        assert _path(dev.h) == 1 and np.array_equal(tB.cpu().numpy(), X)
    finally:
        dev.h.set_option("getrs_t_blocked_min", before)

    # device operands: Matrix makes a solver of its own; give that one the option too and keep it for the read-back
    made = []

    class Recording(device_mod.DeviceSolver):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.h.set_option("getrs_t_blocked_min", 64)
            made.append(self)

    monkeypatch.setattr(device_mod, "DeviceSolver", Recording)
    Xd = la.Matrix.from_dlpack(torch.from_numpy(A.copy()).cuda()).solve_array(torch.from_numpy(B).cuda(), trans=True)
    assert len(made) == 1 and _path(made[0].h) == 1
    assert hasattr(Xd, "is_cuda") and Xd.is_cuda and relerr(Xd.cpu().numpy(), ref) < T.TOL_NUMPY

    # lsx_gesvr_f64 with trans = 1: its initial solve takes the blocked path, its corrections are single columns
    Xr, ferr, berr, rinfo = dense.solve_bounded(A, B, trans=True)
    assert rinfo == 0 and _path(h) == 1
    print(f"gesvr trans: max berr/u {berr.max() / 2.0 ** -53:.2f}  max ferr {ferr.max():.2e}")
    assert np.all(berr <= 4 * 2.0 ** -53) and np.all(ferr > 0) and np.all(ferr < 1e-9)
    assert relerr(Xr, ref) < T.TOL_NUMPY


def test_options(la, blocked_min):
    from linalg_solver_amd import dense

    h = la.default_handle()
    lib = h.lib
    default = h.get_option("getrs_t_blocked_min")
    assert default >= 64 and default % 8 == 0              # existing callers (at most 40 columns) keep their path
    assert lib.lsx_set_option(h.ptr, b"getrs_t_blocked_min", -1) == -1 and b"bad argument" in lib.lsx_last_error()
    assert lib.lsx_set_option(h.ptr, b"getrs_t_path", 1) == -1 and b"unknown option" in lib.lsx_last_error()
    assert h.get_option("getrs_t_blocked_min") == default
    for v in (1, 8, 64, 100000, 0):
        blocked_min(v)
        assert h.get_option("getrs_t_blocked_min") == v
    _, Ball, LU, ipiv = _system(300)
    blocked_min(0)
    dense.lu_solve(LU, ipiv, np.ascontiguousarray(Ball[:, :72]), trans=True)
    assert _path(h) == 0
    blocked_min(1)
    A100, B100 = T.system(129)
    A100, B100 = np.ascontiguousarray(A100[:100, :100]), B100[:100]
    LU100, ipiv100, info = dense.lu_factor(A100)
    assert info == 0
    for nrhs in (1, 7, 64, 72, 256):                        # n <= 128 is one workgroup whatever the option says
        Bn = np.ascontiguousarray(B100[:, :nrhs])
        X = dense.lu_solve(LU100, ipiv100, Bn, trans=True)
        assert _path(h) == 0 and relerr(X, np.linalg.solve(A100.T, Bn)) < T.TOL_NUMPY
    v = C.c_int(-5)
    assert lib.lsx_get_option(h.ptr, b"getrs_t_path", C.byref(v)) == 0 and v.value == 0
