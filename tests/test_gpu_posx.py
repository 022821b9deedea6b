"""Condition estimate and error bounds of the Cholesky family on the MI355X (lsx_lansy_* / lsx_pocon_* / lsx_porcond_* /
lsx_porfs_* / lsx_posvr_*, the few-column path of lsx_potrs_* and the symmetric residual pass), through the C ABI,
`dense`, `DeviceSolver` and `Matrix`.  The yardsticks are those tests/test_posx_host.py proves of the numpy twins on the
same inputs.  Every test that passes a matrix or a factor fills its strictly lower triangle with NaN and again with a
canary: it comes back bit for bit, and no NaN reaches a result.  Nothing here is cooperative: lsx_check_status is
LSX_OK after every test.
"""
import ctypes as C

import numpy as np
import pytest

import cpu_chol as cc
import cpu_posx as cp
import cpu_refine as cr

pytestmark = pytest.mark.gpu

ORDERS = cp.ORDERS
NRHS = (1, 3, 8, 9, 11)
PRECS = ("f64", "f32")
FILLS = [np.nan, -777.25]
FILL_IDS = ["nan", "canary"]


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


@pytest.fixture(autouse=True)
def _status_is_ok(la, dev):
    yield
    assert dev.lib.lsx_check_status(dev.h.ptr) == 0
    assert dev.lib.lsx_check_status(la.default_handle().ptr) == 0


@pytest.fixture
def few(la, dev):
    """potrs_few_max = 8 on both handles for the duration of a test."""
    handles = (dev.h, la.default_handle())
    for h in handles:
        h.set_option("potrs_few_max", 8)
    yield
    for h in handles:
        h.set_option("potrs_few_max", 0)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _t(a):
    import torch

    return torch.from_numpy(np.array(a, order="C")).cuda()


def _tdt(prec):
    import torch

    return torch.float64 if prec == "f64" else torch.float32


def _hptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double if a.dtype == np.float64 else C.c_float))


def _offset_view(src, ld, offset, fillv=float("nan")):
    import torch

    rows, cols = src.shape
    buf = torch.full((offset + rows * ld + 8,), fillv, dtype=src.dtype, device="cuda")
    view = buf[offset:offset + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(src)
    return buf, view


def _view_in(src, kind, odd_off, odd_pad):
    """src inside a NaN-filled buffer: "odd" = element offset odd_off and an odd leading dimension (element-wise
    forms); "padded" = 16-byte aligned with a leading dimension above the width (16-byte forms with ld != n)."""
    cols = src.shape[1]
    if kind == "odd":
        buf, v = _offset_view(src, cols + odd_pad + (cols % 2), odd_off)
        assert v.stride(0) % 2 == 1
        return buf, v, odd_off
    ld = (cols + 15) // 16 * 16 + 16
    buf, v = _offset_view(src, ld, 16)
    assert v.data_ptr() % 16 == 0 and v.stride(0) % 4 == 0 and v.stride(0) > cols
    return buf, v, 16


def _nothing_outside(buf, v, off):
    import torch

    rows, cols = v.shape
    outside = torch.ones_like(buf, dtype=torch.bool)
    outside[off:off + rows * v.stride(0)].view(rows, v.stride(0))[:, :cols] = False
    return bool(torch.isnan(buf[outside]).all())


def _hook(dev, prec, tA, tB, tX, ncols=None, col=0, out=None):
    """lsx_diag_resid_bound_sym_*_dev on columns [col, col + ncols) of tB / tX: (R, W) as numpy (or the views given)."""
    import torch

    n = tA.shape[0]
    ncols = tB.shape[1] - col if ncols is None else ncols
    if out is None:
        R = torch.full((n, ncols), float("nan"), dtype=tA.dtype, device="cuda")
        W = torch.full((n, ncols), float("nan"), dtype=tA.dtype, device="cuda")
    else:
        R, W = out
    es = tA.element_size()
    fn = getattr(dev.lib, f"lsx_diag_resid_bound_sym_{prec}_dev")
    assert fn(dev.h.ptr, n, ncols, tA.data_ptr(), max(tA.stride(0), 1), tB.data_ptr() + col * es, max(tB.stride(0), 1),
              tX.data_ptr() + col * es, max(tX.stride(0), 1), R.data_ptr(), W.data_ptr(), max(R.stride(0), 1)) == 0
    dev.h.synchronize()
    return R.cpu().numpy(), W.cpu().numpy()


def _pocon_abi(dev, prec, U, anorm, device):
    """(status, rcond) of lsx_pocon_* (host buffers) or lsx_pocon_*_dev on a copy in HBM."""
    n = U.shape[0]
    rc = C.c_double(-7.0)
    if device:
        tU = _t(U)
        st = getattr(dev.lib, f"lsx_pocon_{prec}_dev")(dev.h.ptr, n, tU.data_ptr() if n else None, max(n, 1), anorm,
                                                        C.byref(rc))
        assert n == 0 or _same(tU.cpu().numpy(), U), "the factor is read only"
    else:
        Uc = np.ascontiguousarray(U)
        st = getattr(dev.lib, f"lsx_pocon_{prec}")(dev.h.ptr, n, _hptr(Uc) if n else None, max(n, 1), anorm, C.byref(rc))
    return st, rc.value


# ------------------------------------------------------------------ the symmetric residual pass (hook)
_sym = {}


def _sym_case(n, prec):
    """A (the refinement matrix), B, X (not the solution) and the longdouble residual and bound of the full matrix."""
    if (n, prec) not in _sym:
        dt = cp.DTYPES[prec]
        A = cp.scaled_spd(n, 1, cp.SCALE_REFINE[prec], dt)
        B, XT = cp.rhs(A, 8, n)
        X = cp.perturbed(XT)
        Al, Bl, Xl = (v.astype(np.longdouble) for v in (A, B, X))
        r = Bl - Al @ Xl
        w = np.abs(Bl) + np.abs(Al) @ np.abs(Xl)
        for a in (A, B, X, r, w):
            a.setflags(write=False)
        _sym[(n, prec)] = (A, B, X, r, w)
    return _sym[(n, prec)]


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", ORDERS)
def test_symmetric_pass_against_the_full_matrix(dev, n, prec, fill):
    """Against the longdouble residual and bound of the FULL symmetric matrix, with the tolerance
    test_gpu_refine.py::test_residual_and_bound_kernel_directly applies to the general kernel (2 gamma_n w for the two
    orders of n fp64 terms, plus the rounding of the result).  Two calls give identical bits; a column alone and a
    group of 3 have the bits they have in the group of 8; A comes back bit for bit."""
    A, B, X, r, w = _sym_case(n, prec)
    u = cr.unit(cp.DTYPES[prec])
    Afill = cc.fill_lower(A, fill)
    tA, tB, tX = _t(Afill), _t(B), _t(X)
    R, W = _hook(dev, prec, tA, tB, tX)
    assert not np.isnan(R).any() and not np.isnan(W).any()
    R2, W2 = _hook(dev, prec, tA, tB, tX)
    assert _same(R, R2) and _same(W, W2)
    r64, w64 = r.astype(np.float64), w.astype(np.float64)
    tol = 2 * n * 2.0 ** -53 * w64 + 2 * u * np.abs(r64)
    worst = float(np.max(np.abs(R.astype(np.longdouble) - r) / tol))
    print(f"sym pass {prec} n={n}: max |r - r_ld| / bound {worst:.3f}")
    assert np.all(np.abs(R.astype(np.longdouble) - r) <= tol)
    assert np.all(np.abs(W.astype(np.longdouble) - w) <= 2 * n * 2.0 ** -53 * w64 + 2 * u * w64)
    for j in (0, 5, 7):
        R1, W1 = _hook(dev, prec, tA, tB, tX, ncols=1, col=j)
        assert _same(R1[:, 0], R[:, j]) and _same(W1[:, 0], W[:, j]), "a column alone"
    R3, W3 = _hook(dev, prec, tA, tB, tX, ncols=3, col=2)
    assert _same(R3, R[:, 2:5]) and _same(W3, W[:, 2:5])
    assert _same(tA.cpu().numpy(), Afill), "A is read only, its lower triangle included"
    fn = getattr(dev.lib, f"lsx_diag_resid_bound_sym_{prec}_dev")
    assert fn(dev.h.ptr, 4, 9, None, 4, None, 9, None, 9, None, None, 9) == -1 and b"bad argument" in dev.lib.lsx_last_error()


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("layout", ["odd", "padded"])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", (129, 300))
def test_symmetric_pass_on_views(dev, n, prec, layout, fill):
    """Mis-aligned, odd-lda and padded views inside NaN buffers: the bits of the aligned call, nothing outside R and W
    written, A untouched."""
    import torch

    A, B, X, _, _ = _sym_case(n, prec)
    Afill = cc.fill_lower(A, fill)
    R, W = _hook(dev, prec, _t(Afill), _t(B), _t(X))
    bufA, vA, offA = _view_in(_t(Afill), layout, 1, 3)
    _, vB, _ = _view_in(_t(B), layout, 3, 5)
    _, vX, _ = _view_in(_t(X), layout, 5, 1)
    z = torch.zeros(n, 8, dtype=_tdt(prec), device="cuda")
    bufR, vR, offR = _view_in(z, layout, 1, 3)
    bufW, vW, offW = _view_in(z, layout, 3, 3)       # one leading dimension serves R and W
    assert vR.stride(0) == vW.stride(0)
    keepA = bufA.clone()
    Rv, Wv = _hook(dev, prec, vA, vB, vX, out=(vR, vW))
    assert _same(vR.cpu().numpy(), R) and _same(vW.cpu().numpy(), W)
    assert _nothing_outside(bufR, vR, offR) and _nothing_outside(bufW, vW, offW)
    assert _same(bufA.cpu().numpy(), keepA.cpu().numpy())


# ------------------------------------------------------------------ lansy
def _lansy(dev, prec, tA):
    import torch

    n = tA.shape[0]
    out = torch.full((1,), -3.0, dtype=torch.float64, device="cuda")
    assert getattr(dev.lib, f"lsx_lansy_{prec}_dev")(dev.h.ptr, n, tA.data_ptr() if n else None, max(tA.stride(0), 1),
                                                      out.data_ptr()) == 0
    dev.h.synchronize()
    return float(out.item())


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", ORDERS)
def test_lansy(dev, n, prec, fill):
    import torch

    dt = cp.DTYPES[prec]
    A = cp.scaled_spd(n, 0, cp.SCALE_COND[prec], dt, cp.SHIFT_COND[prec])
    ref = float(np.abs(A.astype(np.float64)).sum(axis=0).max())
    Afill = cc.fill_lower(A, fill)
    tA = _t(Afill)
    got = _lansy(dev, prec, tA)
    assert abs(got - ref) <= n * 2.0 ** -53 * ref
    assert _lansy(dev, prec, tA) == got and float(dev.norm_sym(tA).item()) == got, "two calls, DeviceSolver"
    assert _same(tA.cpu().numpy(), Afill)
    _, P = cc.planted(n, dtype=dt)
    Pf = cc.fill_lower(P, fill)
    assert _lansy(dev, prec, _t(Pf)) == float(np.abs(P.astype(np.float64)).sum(axis=0).max()), "integers: exact"
    _, vA, _ = _view_in(tA, "odd", 1, 3)
    assert _lansy(dev, prec, vA) == got
    _, vA, _ = _view_in(tA, "padded", 1, 3)
    assert _lansy(dev, prec, vA) == got
    Pn = Pf.copy()
    Pn[n // 2, n - 1] = np.nan
    assert np.isnan(_lansy(dev, prec, _t(Pn)))
    assert _lansy(dev, prec, torch.zeros(0, 0, dtype=_tdt(prec), device="cuda")) == 0.0
    fn = getattr(dev.lib, f"lsx_lansy_{prec}_dev")
    assert fn(dev.h.ptr, n, tA.data_ptr(), n - 1, tA.data_ptr()) == -1 and fn(dev.h.ptr, -1, None, 1, tA.data_ptr()) == -1
    assert fn(dev.h.ptr, n, None, n, tA.data_ptr()) == -1 and fn(dev.h.ptr, n, tA.data_ptr(), n, None) == -1


# ------------------------------------------------------------------ the few-column solve
def _potrs_dev(dev, U, B):
    tU, tB = _t(U), _t(B)
    dev.potrs_(tU, tB)
    dev.h.synchronize()
    assert _same(tU.cpu().numpy(), U), "the factor is read only"
    return tB.cpu().numpy()


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("dtype", (np.float64, np.float32))
@pytest.mark.parametrize("n,nrhs", cp.PLANTED_FEW)
def test_few_column_planted_solve(dev, few, n, nrhs, dtype, fill):
    """The systems of test_gpu_chol.py::test_planted_solve with nrhs <= 8: the integer solution bit for bit wherever the
    host twin (and the model of the block sweeps) is exact -- everywhere but fp32 (128, 1) and (129, 7), see
    cpu_posx.PLANTED_FEW_INEXACT_F32 -- and inside gamma_{3n+1} everywhere."""
    U, A, X, B = cp.planted_system(n, nrhs, dtype)
    got = _potrs_dev(dev, cc.fill_lower(U, fill), B)
    assert dev.h.get_option("potrs_path") == 1
    assert not np.isnan(got).any()
    if cp.planted_exact(n, nrhs, dtype):
        assert np.array_equal(got, X)
    assert cc.solve_residual(A, U, B, got) <= cc.gamma(3 * n + 1, dtype)


_fac = {}


def _lib_factor(n, prec, seed=0):
    """The library's own Cholesky factor of cpu_chol.spd(n, seed) (one factorisation per matrix and precision)."""
    from linalg_solver_amd import dense

    if (n, prec, seed) not in _fac:
        A = cc.spd(n, seed, cp.DTYPES[prec])
        U, info = dense.cho_factor(A, dtype=cp.DTYPES[prec])
        assert info == 0
        U.setflags(write=False)
        A.setflags(write=False)
        _fac[(n, prec, seed)] = (A, U)
    return _fac[(n, prec, seed)]


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", ORDERS)
def test_few_column_solve_within_highams_bound_and_paths(dev, n, prec, fill):
    """Rounded inputs inside gamma_{3n+1} for nrhs = 1, 3, 8; potrs_path reads 1 there, 0 for nrhs = 9 and with the
    option at 0; with the option at 0 the result has the bits of a handle on which the option was never set."""
    from linalg_solver_amd.device import DeviceSolver

    dt = cp.DTYPES[prec]
    A, U = _lib_factor(n, prec)
    Ufill = cc.fill_lower(U, fill)
    B = np.random.default_rng(n).standard_normal((n, 9)).astype(dt)
    pristine = DeviceSolver()
    before = {k: _potrs_dev(pristine, Ufill, B[:, :k]) for k in (1, 8, 9)}
    assert pristine.h.get_option("potrs_path") == 0 and pristine.h.get_option("potrs_few_max") == 0
    dev.h.set_option("potrs_few_max", 8)
    try:
        for k in (1, 3, 8):
            X = _potrs_dev(dev, Ufill, B[:, :k])
            assert dev.h.get_option("potrs_path") == 1
            assert not np.isnan(X).any()
            res = cc.solve_residual(A, U, B[:, :k], X)
            print(f"few-column potrs {prec} n={n} nrhs={k}: {res / cc.UNIT[np.dtype(dt)]:.2f} u")
            assert res <= cc.gamma(3 * n + 1, dt)
            assert _same(X, _potrs_dev(dev, Ufill, B[:, :k])), "two calls"
        X9 = _potrs_dev(dev, Ufill, B)
        assert dev.h.get_option("potrs_path") == 0 and _same(X9, before[9])
        dev.h.set_option("potrs_few_max", 3)
        _potrs_dev(dev, Ufill, B[:, :4])
        assert dev.h.get_option("potrs_path") == 0
    finally:
        dev.h.set_option("potrs_few_max", 0)
    for k in (1, 8):
        X = _potrs_dev(dev, Ufill, B[:, :k])
        assert dev.h.get_option("potrs_path") == 0 and _same(X, before[k]), "option at 0: the sweeps, the same bits"
    assert dev.lib.lsx_set_option(dev.h.ptr, b"potrs_few_max", 9) == -1
    assert dev.lib.lsx_set_option(dev.h.ptr, b"potrs_few_max", -1) == -1
    assert dev.lib.lsx_set_option(dev.h.ptr, b"potrs_path", 1) == -1, "read only"
    assert pristine.lib.lsx_check_status(pristine.h.ptr) == 0


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("layout", ["odd", "padded"])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n,nrhs", [(129, 7), (300, 1), (257, 8)])
def test_few_column_solve_on_views(dev, few, n, nrhs, prec, layout, fill):
    dt = cp.DTYPES[prec]
    A, U = _lib_factor(n, prec)
    Ufill = cc.fill_lower(U, fill)
    B = np.random.default_rng(n + 1).standard_normal((n, nrhs)).astype(dt)
    ref = _potrs_dev(dev, Ufill, B)
    bufU, vU, offU = _view_in(_t(Ufill), layout, 1, 3)
    bufB, vB, offB = _view_in(_t(B), layout, 3, 5)
    keepU = bufU.clone()
    dev.potrs_(vU, vB)
    dev.h.synchronize()
    assert dev.h.get_option("potrs_path") == 1
    assert _same(vB.cpu().numpy(), ref)
    assert _nothing_outside(bufB, vB, offB) and _same(bufU.cpu().numpy(), keepU.cpu().numpy())


# ------------------------------------------------------------------ pocon
@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", ORDERS)
def test_pocon_agrees_with_lapack_and_bounds_the_exact_value(la, dev, n, prec, fill):
    """On LAPACK's own factor of the same input: within cpu_cond.bound (64 n eps cond_1 <= 0.35) of LAPACK's pocon, at
    least the exact rcond times (1 - bound), 4 .. 11 solves; the host, _dev, dense and DeviceSolver forms agree bit for
    bit."""
    from linalg_solver_amd import dense

    case = cp.cond_case(n, prec)
    bound, ref, exact, anorm = case["bound"], case["rcond_lapack"], case["rcond_exact"], case["anorm"]
    assert bound <= 0.35
    Ufill = cc.fill_lower(case["U_lapack"], fill)
    st, rc = _pocon_abi(dev, prec, Ufill, anorm, device=False)
    solves = dev.h.get_option("pocon_solves")
    print(f"pocon {prec} n={n}: rcond {rc:.6e} lapack {ref:.6e} exact {exact:.6e} |ratio-1| {abs(rc / ref - 1):.2e} "
          f"bound {bound:.2e} solves {solves}")
    assert st == 0 and abs(rc / ref - 1.0) <= bound
    assert rc >= exact * (1.0 - bound)
    assert (4 <= solves <= 11) if n > 1 else solves == 1
    st, rc_dev = _pocon_abi(dev, prec, Ufill, anorm, device=True)
    assert st == 0 and rc_dev == rc and dev.h.get_option("pocon_solves") == solves
    assert dense.cho_rcond(Ufill, anorm) == rc
    assert la.default_handle().get_option("pocon_solves") == solves
    tU = _t(Ufill)
    assert dev.pocon(tU, anorm) == rc and _same(tU.cpu().numpy(), Ufill)
    # the norm the library computes is LAPACK's to rounding, and the one-call form agrees with the chain of its parts
    Afill = cc.fill_lower(case["A"], fill)
    rc1, info = dense.rcond_pos(Afill, dtype=cp.DTYPES[prec])
    tA = _t(Afill)
    an = dev.norm_sym(tA)
    assert int(dev.potrf_(tA).item()) == 0
    assert info == 0 and rc1 == dev.pocon(tA, an)
    assert abs(rc1 / ref - 1.0) <= bound and rc1 >= exact * (1.0 - bound)


def test_pocon_through_matrix(la, dev):
    from linalg_solver_amd import dense

    n = 129
    A = cc.fill_lower(cp.cond_case(n, "f64")["A"], np.nan)
    rc, info = dense.rcond_pos(A)
    assert info == 0
    for M in (la.Matrix.from_numpy(A), la.Matrix.from_dlpack(_t(A))):
        assert M.rcond_pos_def() == rc
        assert M.cond_pos_def() == 1.0 / rc
    _, N = cc.planted_not_pd(140, 130, "negative")
    for M in (la.Matrix.from_numpy(N), la.Matrix.from_dlpack(_t(N))):
        with pytest.raises(ValueError, match="leading minor of order 131"):
            M.rcond_pos_def()


@pytest.mark.parametrize("prec", PRECS)
def test_pocon_outcomes_are_values(la, dev, prec):
    from linalg_solver_amd import dense

    dt = cp.DTYPES[prec]
    U, A = cc.planted(140, dtype=dt)
    Uf = cc.fill_lower(U, np.nan)
    for device in (False, True):
        assert _pocon_abi(dev, prec, np.zeros((0, 0), dtype=dt), 1.0, device) == (0, 1.0)
        assert _pocon_abi(dev, prec, Uf, 0.0, device) == (0, 0.0)
        for bad in (0.0, np.nan):
            Z = Uf.copy()
            Z[131, 131] = bad
            assert _pocon_abi(dev, prec, Z, 3.0, device) == (0, 0.0), "an exactly zero or NaN u_ii"
        Z = Uf.copy()
        Z[3, 9] = np.inf
        assert _pocon_abi(dev, prec, Z, 3.0, device) == (0, 0.0), "an estimate that is not a finite number"
        for bad in (np.nan, -1.0):
            st, _ = _pocon_abi(dev, prec, Uf, bad, device)
            assert st == -1 and b"anorm" in dev.lib.lsx_last_error()
    rc = C.c_double(0)
    fn = getattr(dev.lib, f"lsx_pocon_{prec}")
    assert fn(dev.h.ptr, 4, _hptr(np.ascontiguousarray(Uf)), 3, 1.0, C.byref(rc)) == -1
    assert fn(dev.h.ptr, 4, None, 4, 1.0, C.byref(rc)) == -1 and fn(dev.h.ptr, 4, _hptr(np.ascontiguousarray(Uf)), 4, 1.0, None) == -1
    with pytest.raises(ValueError):
        dense.cho_rcond(Uf, float("nan"))
    # not positive definite: rcond = 0 and potrf's info
    for j, kind in ((0, "zero"), (130, "negative"), (5, "nan")):
        _, N = cc.planted_not_pd(140, j, kind, dtype=dt)
        assert dense.rcond_pos(cc.fill_lower(N, np.nan), dtype=dt) == (0.0, j + 1)
    assert dense.rcond_pos(np.zeros((0, 0), dtype=dt), dtype=dt) == (1.0, 0)


# ------------------------------------------------------------------ porfs
_start = {}


def _refine_start(n, prec):
    """The library's factor of the refinement matrix and the perturbed start: its own solution times (1 +- 2^-10)."""
    from linalg_solver_amd import dense

    if (n, prec) not in _start:
        case = cp.refine_case(n, prec)
        U, info = dense.cho_factor(case["A"], dtype=cp.DTYPES[prec])
        assert info == 0
        X0 = cp.perturbed(dense.cho_solve(U, case["B"]))
        U.setflags(write=False)
        X0.setflags(write=False)
        _start[(n, prec)] = (U, X0)
    return _start[(n, prec)]


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("nrhs", NRHS)
@pytest.mark.parametrize("n", ORDERS)
def test_porfs_agrees_with_the_yardsticks(la, n, nrhs, prec, fill):
    from linalg_solver_amd import dense

    case = cp.refine_case(n, prec)
    A, B = case["A"], case["B"]
    U, X0 = _refine_start(n, prec)
    Afill, Ufill = cc.fill_lower(A, fill), cc.fill_lower(U, fill)
    keepA, keepU = Afill.copy(), Ufill.copy()
    Bk, X0k = np.ascontiguousarray(B[:, :nrhs]), np.ascontiguousarray(X0[:, :nrhs])
    X, ferr, berr = dense.cho_refine(Afill, Ufill, Bk, X0k)
    h = la.default_handle()
    steps, solves = h.get_option("porfs_steps"), h.get_option("porfs_solves")
    assert X.dtype == cp.DTYPES[prec] and X.shape == (n, nrhs) and ferr.shape == berr.shape == (nrhs,)
    assert not np.isnan(X).any() and _same(Afill, keepA) and _same(Ufill, keepU)
    cp.check_columns(f"porfs {prec} n={n} nrhs={nrhs}", n, prec, A, B, case["truth"], case["inv"], X, ferr, berr, steps,
                     solves)


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", (129, 300))
def test_porfs_device_form_two_calls_and_column_subsets(la, dev, n, prec, fill):
    """lsx_porfs_*_dev through DeviceSolver has the bits of the host-buffer form; two calls give the same bits; a
    column's X, ferr and berr do not depend on the columns passed with it; A and U come back bit for bit."""
    from linalg_solver_amd import dense

    case = cp.refine_case(n, prec)
    A, B = case["A"], case["B"]
    U, X0 = _refine_start(n, prec)
    Afill, Ufill = cc.fill_lower(A, fill), cc.fill_lower(U, fill)
    X, ferr, berr = dense.cho_refine(Afill, Ufill, B, X0)
    tA, tU, tB, tX = _t(Afill), _t(Ufill), _t(B), _t(X0)
    fd, bd = dev.porfs_(tA, tU, tB, tX)
    assert _same(tX.cpu().numpy(), X) and _same(fd, ferr) and _same(bd, berr)
    assert _same(tA.cpu().numpy(), Afill) and _same(tU.cpu().numpy(), Ufill) and _same(tB.cpu().numpy(), B)
    assert dev.h.get_option("porfs_steps") == la.default_handle().get_option("porfs_steps")
    X2, f2, b2 = dense.cho_refine(Afill, Ufill, B, X0)
    assert _same(X2, X) and _same(f2, ferr) and _same(b2, berr)
    for cols in ([0], [4], [10], [1, 2, 3], [8, 9, 10], [0, 8]):
        Xs, fs, bs = dense.cho_refine(Afill, Ufill, np.ascontiguousarray(B[:, cols]), np.ascontiguousarray(X0[:, cols]))
        assert _same(Xs, X[:, cols]) and _same(fs, ferr[cols]) and _same(bs, berr[cols]), cols
    xv, fv, bv = dense.cho_refine(Afill, Ufill, np.array(B[:, 4]), np.array(X0[:, 4]))
    assert xv.shape == (n,) and _same(xv, X[:, 4]) and fv == ferr[4] and bv == berr[4] and isinstance(fv, float)


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("dtype", (np.float64, np.float32))
@pytest.mark.parametrize("n", (5, 130, 300))
def test_porfs_leaves_an_exact_solution_alone(la, n, dtype, fill):
    from linalg_solver_amd import dense

    U, A = cc.planted(n, dtype=dtype)
    X = np.random.default_rng(n).integers(-3, 4, (n, 3)).astype(dtype)
    B = (A.astype(np.float64) @ X.astype(np.float64)).astype(dtype)
    X2, ferr, berr = dense.cho_refine(cc.fill_lower(A, fill), cc.fill_lower(U, fill), B, X)
    assert np.all(berr == 0.0) and la.default_handle().get_option("porfs_steps") == 0 and _same(X2, X)
    assert np.all(np.isfinite(ferr)) and np.all(ferr >= 0)


@pytest.mark.parametrize("prec", PRECS)
def test_porfs_outcomes_are_values(la, dev, prec):
    import torch

    from linalg_solver_amd import dense

    n, dt = 129, cp.DTYPES[prec]
    case = cp.refine_case(n, prec)
    A, B = cc.fill_lower(case["A"], np.nan), np.array(case["B"][:, :3])
    U, X0 = _refine_start(n, prec)
    U, X0 = cc.fill_lower(U, np.nan), np.array(X0[:, :3])
    X, ferr, berr = dense.cho_refine(A, U, B, X0)
    # NaN in one column of B: NaN bounds for that column only, the other columns' bits unchanged
    Bn = B.copy()
    Bn[7, 1] = np.nan
    Xn, fn_, bn = dense.cho_refine(A, U, Bn, X0)
    assert np.isnan(fn_[1]) and np.isnan(bn[1]) and _same(Xn[:, 1], X0[:, 1]), "no step for that column"
    for j in (0, 2):
        assert _same(Xn[:, j], X[:, j]) and fn_[j] == ferr[j] and bn[j] == berr[j]
    # NaN in the upper triangle of A reaches every column; NaN in X its own
    An = A.copy()
    An[3, 100] = np.nan
    _, fa, ba = dense.cho_refine(An, U, B, X0)
    assert np.isnan(fa).all() and np.isnan(ba).all()
    Xq = X0.copy()
    Xq[5, 2] = np.nan
    _, fx, bx = dense.cho_refine(A, U, B, Xq)
    assert np.isnan(fx[2]) and np.isnan(bx[2]) and fx[0] == ferr[0] and bx[1] == berr[1]
    # an exactly zero or NaN u_ii: X untouched, +inf bounds
    for bad in (0.0, np.nan):
        Z = U.copy()
        Z[128, 128] = bad
        Xz, fz, bz = dense.cho_refine(A, Z, B, X0)
        assert _same(Xz, X0) and np.all(np.isposinf(fz)) and np.all(np.isposinf(bz))
        tX = _t(X0)
        fz, bz = dev.porfs_(_t(A), _t(Z), _t(B), tX)
        assert _same(tX.cpu().numpy(), X0) and np.all(np.isposinf(fz)) and np.all(np.isposinf(bz))
    # zero extents
    e = np.zeros((0, 0), dtype=dt)
    X_, f_, b_ = dense.cho_refine(e, e, np.zeros((0, 2), dtype=dt), np.zeros((0, 2), dtype=dt))
    assert X_.shape == (0, 2) and np.array_equal(f_, [0.0, 0.0]) and np.array_equal(b_, [0.0, 0.0])
    X_, f_, b_ = dense.cho_refine(A, U, np.zeros((n, 0), dtype=dt), np.zeros((n, 0), dtype=dt))
    assert X_.shape == (n, 0) and f_.shape == (0,) and b_.shape == (0,)
    # arguments
    sfx = prec
    fn = getattr(dev.lib, f"lsx_porfs_{sfx}_dev")
    tA, tU, tB, tX = _t(A), _t(U), _t(B), _t(X0)
    fe, be = np.zeros(3), np.zeros(3)
    dp = C.POINTER(C.c_double)
    args = lambda **k: (dev.h.ptr, k.get("n", n), k.get("nrhs", 3), k.get("A", tA.data_ptr()), k.get("lda", n),   # noqa: E731
                        k.get("U", tU.data_ptr()), k.get("ldu", n), k.get("B", tB.data_ptr()), k.get("ldb", 3),
                        k.get("X", tX.data_ptr()), k.get("ldx", 3), k.get("ferr", fe.ctypes.data_as(dp)),
                        k.get("berr", be.ctypes.data_as(dp)))
    for bad in (dict(n=-1), dict(nrhs=-1), dict(lda=n - 1), dict(ldu=n - 1), dict(ldb=2), dict(ldx=2), dict(A=None),
                dict(U=None), dict(B=None), dict(X=None), dict(ferr=None), dict(berr=None)):
        assert fn(*args(**bad)) == -1 and b"bad argument" in dev.lib.lsx_last_error(), bad
    torch.cuda.synchronize()
    assert _same(tX.cpu().numpy(), X0)
    with pytest.raises(ValueError):
        dev.porfs_(tA, tU, tB, tX[:, :2])
    with pytest.raises(TypeError):
        dev.porfs_(tA, tU, tB, tX.to(torch.float32 if prec == "f64" else torch.float64))
    with pytest.raises(ValueError):
        dense.cho_refine(A, U, B, X0[:, :2])


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("layout", ["odd", "padded"])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", (129, 300))
def test_porfs_on_views(dev, n, prec, layout, fill):
    case = cp.refine_case(n, prec)
    U, X0 = _refine_start(n, prec)
    A, B = cc.fill_lower(case["A"], fill), np.array(case["B"][:, :9])
    U, X0 = cc.fill_lower(U, fill), np.array(X0[:, :9])
    tX = _t(X0)
    ferr, berr = dev.porfs_(_t(A), _t(U), _t(B), tX)
    bufA, vA, _ = _view_in(_t(A), layout, 1, 3)
    bufU, vU, _ = _view_in(_t(U), layout, 3, 1)
    bufB, vB, _ = _view_in(_t(B), layout, 5, 5)
    bufX, vX, offX = _view_in(_t(X0), layout, 7, 3)
    keep = [b.clone() for b in (bufA, bufU, bufB)]
    fv, bv = dev.porfs_(vA, vU, vB, vX)
    assert _same(vX.cpu().numpy(), tX.cpu().numpy()) and _same(fv, ferr) and _same(bv, berr)
    assert _nothing_outside(bufX, vX, offX)
    for b, k in zip((bufA, bufU, bufB), keep):
        assert _same(b.cpu().numpy(), k.cpu().numpy())


# ------------------------------------------------------------------ posvr and the Python layers
@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("prec", PRECS)
def test_posvr_and_dense_layers(la, prec, fill):
    from linalg_solver_amd import dense

    n, dt = 200, cp.DTYPES[prec]
    u = cr.unit(dt)
    A = cc.spd(n, 3, dt)
    Afill = cc.fill_lower(A, fill)
    B, XT = cp.rhs(A, 9, 5)
    X, ferr, berr, info = dense.solve_pos_bounded(Afill, B, dtype=dt)
    assert info == 0 and X.shape == (n, 9) and X.dtype == dt and ferr.shape == berr.shape == (9,)
    assert not np.isnan(X).any() and np.all(berr <= 4 * u) and np.all(ferr > 0) and np.all(ferr < 1e3 * n * u)
    for j in range(9):
        err = float(np.max(np.abs(X[:, j].astype(np.float64) - XT[:, j])) / np.max(np.abs(X[:, j])))
        assert err <= ferr[j] + 4 * n * u, "B = A XT was rounded to the working precision"
    # the same through the parts: factor, solve, refine
    U, finfo = dense.cho_factor(Afill, dtype=dt)
    X0 = dense.cho_solve(U, B)
    Xr, fr, br = dense.cho_refine(Afill, U, B, X0)
    assert finfo == 0 and _same(Xr, X) and _same(fr, ferr) and _same(br, berr)
    xv, fv, bv, info = dense.solve_pos_bounded(Afill, np.array(B[:, 0]), dtype=dt)
    assert info == 0 and xv.shape == (n,) and isinstance(fv, float) and isinstance(bv, float)
    assert bv <= 4 * u and 0 < fv < 1e3 * n * u      # (the unrefined solve may give a column other bits alone than in a group)
    # not positive definite
    _, N = cc.planted_not_pd(140, 130, "negative", dtype=dt)
    Bn = np.ones((140, 2), dtype=dt)
    Xn, fn_, bn, info = dense.solve_pos_bounded(cc.fill_lower(N, fill), Bn, dtype=dt)
    assert Xn is None and info == 131 and np.all(np.isposinf(fn_)) and np.all(np.isposinf(bn))
    xn, f1, b1, info = dense.solve_pos_bounded(cc.fill_lower(N, fill), Bn[:, 0], dtype=dt)
    assert xn is None and info == 131 and f1 == float("inf") and b1 == float("inf")
    Xe, fe, be, info = dense.solve_pos_bounded(np.zeros((0, 0), dtype=dt), np.zeros((0, 2), dtype=dt), dtype=dt)
    assert info == 0 and Xe.shape == (0, 2) and np.array_equal(fe, [0, 0]) and np.array_equal(be, [0, 0])


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
def test_matrix_solve_pos_def_array(la, fill):
    """Shapes and types as test_gpu_refine.py::test_matrix_solve_array_with_bounds; a host Matrix and a device Matrix
    agree within the sum of their ferr; a matrix that is not positive definite is a ValueError naming the minor."""
    from linalg_solver_amd import dense

    n = 129
    A = cc.spd(n, 4)
    Afill = cc.fill_lower(A, fill)
    B, _ = cp.rhs(A, 3, 8)
    M = la.Matrix.from_numpy(np.array(Afill))
    plain = M.solve_pos_def_array(np.array(B))
    assert isinstance(plain, np.ndarray) and plain.tobytes() == M.solve_array(np.array(B), pos_def=True).tobytes()
    X, ferr, berr = M.solve_pos_def_array(np.array(B), bounds=True)
    Xa, fa, ba, info = dense.solve_pos_bounded(Afill, B)
    assert info == 0 and X.tobytes() == Xa.tobytes() and ferr.tobytes() == fa.tobytes() and berr.tobytes() == ba.tobytes()
    assert X.shape == (n, 3) and ferr.shape == berr.shape == (3,)
    assert np.all(ba <= 4 * 2.0 ** -53) and np.all(fa > 0) and np.all(fa < 1e-9)
    xv, fv, bv = M.solve_pos_def_array(np.array(B[:, 0]), bounds=True)
    x1, f1, b1 = M.solve_pos_def_array(np.array(B[:, :1]), bounds=True)
    assert xv.shape == (n,) and xv.tobytes() == x1[:, 0].tobytes() and fv == f1[0] and bv == b1[0]
    assert isinstance(fv, float) and isinstance(bv, float)
    dA = _t(Afill)
    Md = la.Matrix.from_dlpack(dA)
    Xd, fd, bd = Md.solve_pos_def_array(_t(B), bounds=True)
    assert Xd.is_cuda and Xd.shape == (n, 3) and fd.shape == bd.shape == (3,)
    for j in range(3):
        xd, xa = Xd.cpu().numpy()[:, j], Xa[:, j]
        assert np.max(np.abs(xd - xa)) <= fd[j] * np.max(np.abs(xd)) + fa[j] * np.max(np.abs(xa))
    assert np.all(bd <= 4 * 2.0 ** -53) and np.all(fd > 0) and np.all(np.isfinite(fd))
    xdv, fdv, bdv = Md.solve_pos_def_array(np.array(B[:, 0]), bounds=True)
    assert xdv.shape == (n,) and isinstance(fdv, float) and isinstance(bdv, float) and bdv <= 4 * 2.0 ** -53
    assert _same(dA.cpu().numpy(), Afill), "the caller's tensor is never written"
    _, N = cc.planted_not_pd(140, 130, "negative")
    for Mn in (la.Matrix.from_numpy(N), la.Matrix.from_dlpack(_t(N))):
        with pytest.raises(ValueError, match="leading minor of order 131"):
            Mn.solve_pos_def_array(np.ones(140), bounds=True)
    with pytest.raises(ValueError, match="pos_def"):
        M.solve_array(np.array(B), pos_def=True, bounds=True)


# ------------------------------------------------------------------ nothing else moved
def test_gerfs_and_gecon_keep_their_bits_around_porfs_and_pocon(la):
    """lsx_gerfs_f64 and lsx_gecon_f64 before and after a porfs / pocon call on the same handle: the shared loop and
    the shared work space (the cond and refine buffers) leave them their bits."""
    from linalg_solver_amd import dense

    n = 300
    Ag, Bg, _ = cr.scaled_system(n, 100 + n, 3)
    LU, ipiv, info = dense.lu_factor(Ag)
    assert info == 0
    X0 = dense.lu_solve(LU, ipiv, Bg)
    anorm = float(np.abs(Ag).sum(axis=0).max())

    def lu_side():
        out = []
        for trans in (False, True):
            X, f, b = dense.lu_refine(Ag, LU, ipiv, Bg, dense.lu_solve(LU, ipiv, Bg, trans=trans), trans=trans)
            out += [X.tobytes(), f.tobytes(), b.tobytes()]
        return out + [dense.lu_rcond(LU, ipiv, anorm).hex(), dense.lu_rcond(LU, ipiv, anorm, norm=np.inf).hex()]

    before = lu_side()
    case = cp.refine_case(n, "f64")
    U, Xs = _refine_start(n, "f64")
    dense.cho_refine(cc.fill_lower(case["A"], np.nan), cc.fill_lower(U, np.nan), case["B"], Xs)
    dense.cho_rcond(cc.fill_lower(U, np.nan), 5.0)
    dense.rcond_pos(case["A"])
    assert lu_side() == before
    assert X0.shape == Bg.shape
