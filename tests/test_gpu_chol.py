"""Cholesky factorisation and solves on the MI355X (lsx_potrf_* / lsx_potrs_* / lsx_posv_* / lsx_syrk_tn_sub_*), through
the C ABI, `dense`, `DeviceSolver` and `Matrix`.  The yardsticks are those tests/test_chol_host.py proves on the CPU:
planted factors bit for bit, LAPACK's info and prefix for matrices that are not positive definite, Higham's bounds on
rounded inputs.  Every case runs with the strictly lower triangle filled with NaN and again with a canary value: it
must come back bit for bit, and no NaN may reach a result.
"""
import ctypes as C

import numpy as np
import pytest

import cpu_chol as cc

pytestmark = pytest.mark.gpu

ORDERS = [1, 2, 64, 127, 128, 129, 257, 384, 512, 600]
DTYPES = [np.float64, np.float32]
FILLS = [np.nan, -777.25]
FILL_IDS = ["nan", "canary"]


@pytest.fixture(scope="module")
def dev():
    import torch

    from linalg_solver_amd.device import DeviceSolver

    assert torch.cuda.is_available()
    return DeviceSolver()


def _sfx(dtype):
    return "f64" if np.dtype(dtype) == np.float64 else "f32"


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _lower_untouched(R, A):
    lo = np.tril_indices(A.shape[0], -1)
    return np.array_equal(_bits(R)[lo], _bits(A)[lo])


def _potrf_dev(dev, A):
    """lsx_potrf_*_dev on a device copy of A: (result as numpy, info)."""
    import torch

    t = torch.from_numpy(np.ascontiguousarray(A)).cuda()
    info = dev.potrf_(t)
    torch.cuda.synchronize()
    return t.cpu().numpy(), int(info.item())


def _potrs_dev(dev, U, B):
    import torch

    tU = torch.from_numpy(np.ascontiguousarray(U)).cuda()
    tB = torch.from_numpy(np.ascontiguousarray(B)).cuda()
    dev.potrs_(tU, tB)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(tU.cpu().numpy()), _bits(U)), "the factor is read only"
    return tB.cpu().numpy()


def _potrf_host(dev, A):
    """lsx_potrf_* (host buffers) on a copy: (result, info)."""
    R = np.ascontiguousarray(A).copy()
    n = R.shape[0]
    info = C.c_int(-7)
    ct = C.c_double if R.dtype == np.float64 else C.c_float
    fn = getattr(dev.lib, f"lsx_potrf_{_sfx(R.dtype)}")
    assert fn(dev.h.ptr, n, R.ctypes.data_as(C.POINTER(ct)), n, C.byref(info)) == 0
    return R, info.value


def _posv_host(dev, A, B):
    A = np.ascontiguousarray(A)
    X = np.ascontiguousarray(B).copy()
    keep = A.copy()
    n, nrhs = X.shape
    info = C.c_int(-7)
    ct = C.c_double if A.dtype == np.float64 else C.c_float
    fn = getattr(dev.lib, f"lsx_posv_{_sfx(A.dtype)}")
    assert fn(dev.h.ptr, n, nrhs, A.ctypes.data_as(C.POINTER(ct)), n, X.ctypes.data_as(C.POINTER(ct)), nrhs,
              C.byref(info)) == 0
    assert np.array_equal(_bits(A), _bits(keep)), "posv does not modify A"
    return X, info.value


# ------------------------------------------------------------------ planted factors, bit for bit
@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", ORDERS)
def test_planted_factor_bit_for_bit(dev, n, dtype, fill):
    U, A = cc.planted(n, dtype=dtype)
    Ain = cc.fill_lower(A, fill)
    R, info = _potrf_dev(dev, Ain)
    assert info == 0
    assert np.array_equal(np.triu(R), U)
    assert _lower_untouched(R, Ain)
    Rh, info = _potrf_host(dev, Ain)
    assert info == 0 and np.array_equal(np.triu(Rh), U) and _lower_untouched(Rh, Ain), "host-buffer form"


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,nrhs", [(1, 1), (2, 7), (128, 1), (129, 7), (257, 64), (384, 200), (600, 64), (600, 1)])
def test_planted_solve(dev, n, nrhs, dtype, fill):
    """potrs from the planted factor with the lower triangle spoilt, nrhs 1, 7, 64, 200; posv of the planted matrix."""
    U, A = cc.planted(n, dtype=dtype)
    X = np.random.default_rng(n + nrhs).integers(-3, 4, (n, nrhs)).astype(dtype)
    B = (A.astype(np.float64) @ X.astype(np.float64)).astype(dtype)
    bound = cc.gamma(3 * n + 1, dtype)
    got = _potrs_dev(dev, cc.fill_lower(U, fill), B)
    assert not np.isnan(got).any()
    r = cc.solve_residual(A, U, B, got)
    print(f"potrs n={n} nrhs={nrhs} {np.dtype(dtype).name}: {r / cc.UNIT[np.dtype(dtype)]:.2f} u")
    assert r <= bound
    Xp, info = _posv_host(dev, cc.fill_lower(A, fill), B)
    assert info == 0 and not np.isnan(Xp).any()
    assert cc.solve_residual(A, U, B, Xp) <= bound


# ------------------------------------------------------------------ not positive definite
@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["zero", "negative", "nan"])
@pytest.mark.parametrize("j", [0, 5, 127, 128, 300])
def test_not_positive_definite(dev, j, kind, dtype, fill):
    n = 384
    U, A = cc.planted_not_pd(n, j, kind, dtype=dtype)
    Ain = cc.fill_lower(A, fill)
    R, info = _potrf_dev(dev, Ain)
    assert info == j + 1
    assert np.array_equal(np.triu(R)[:j, :j], U[:j, :j])
    assert _lower_untouched(R, Ain)
    Rh, info = _potrf_host(dev, Ain)
    assert info == j + 1 and np.array_equal(np.triu(Rh)[:j, :j], U[:j, :j]) and _lower_untouched(Rh, Ain)
    B = np.random.default_rng(j).standard_normal((n, 3)).astype(dtype)
    X, info = _posv_host(dev, Ain, B)
    assert info == j + 1
    assert np.array_equal(_bits(X), _bits(B)), "posv leaves B untouched when the matrix is not positive definite"


def test_not_positive_definite_through_matrix_and_dense(dev):
    import torch

    from linalg_solver_amd import dense
    from linalg_solver_amd.matrix import Matrix

    n, j = 140, 130
    U, A = cc.planted_not_pd(n, j, "negative")
    b = np.ones(n)
    X, info, _ = dense.solve(A, b, assume_pos=True)
    assert X is None and info == j + 1
    Uf, info = dense.cho_factor(A)
    assert info == j + 1 and np.array_equal(Uf[:j, :j], U[:j, :j])
    for M in (Matrix.from_numpy(A), Matrix.from_dlpack(torch.from_numpy(A).cuda())):
        with pytest.raises(ValueError, match=f"leading minor of order {j + 1}"):
            M.solve_array(b, pos_def=True)
        with pytest.raises(ValueError, match=f"leading minor of order {j + 1}"):
            M.cholesky_array()


# ------------------------------------------------------------------ the update on its own
def _offset_view(src, ld, offset, fillv=float("nan")):
    """(buffer, view): src as a view with leading dimension ld at element `offset` of a buffer filled with fillv."""
    import torch

    rows, cols = src.shape
    buf = torch.full((offset + rows * ld + 8,), fillv, dtype=src.dtype, device="cuda")
    view = buf[offset:offset + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(src)
    return buf, view


def _view_in(src, kind, odd_off, odd_pad):
    """src inside a NaN-filled buffer: "odd" = element offset odd_off and an odd leading dimension (the element-wise
    forms); "padded" = 16-byte aligned with a leading dimension above the width (the 16-byte forms with ld != n)."""
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


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("layout", ["aligned", "odd", "padded"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [16, 100, 128])
@pytest.mark.parametrize("n", [1, 127, 128, 129, 384, 400])
def test_syrk_tn_sub_has_the_bits_of_gemm_tn_sub(dev, n, k, dtype, layout, fill):
    """Upper triangle: bit-equal to lsx_gemm_tn_sub_*_dev(n, n, k, A, A, C) on a copy.  Strictly lower triangle: bit for
    bit what was put there, NaN or a canary (the full product gets a copy with finite values there)."""
    import torch

    rng = np.random.default_rng(31 * n + k)
    A = rng.uniform(-1, 1, (k, n)).astype(dtype)
    Cm = rng.uniform(-1, 1, (n, n)).astype(dtype)
    tA, full = torch.from_numpy(A).cuda(), torch.from_numpy(Cm).cuda()
    dev.gemm_tn_sub_(full, tA, tA)
    Cfill = cc.fill_lower(Cm, fill)
    Cin = torch.from_numpy(Cfill).cuda()
    if layout == "aligned":
        vA, vC, bufC, off = tA, Cin.clone(), None, 0
    else:
        _, vA, _ = _view_in(tA, layout, 1, 3)
        bufC, vC, off = _view_in(Cin, layout, 3, 5)
    dev.syrk_tn_sub_(vC, vA)
    torch.cuda.synchronize()
    got = vC.cpu().numpy()
    up = np.triu_indices(n)
    assert np.array_equal(_bits(got)[up], _bits(full.cpu().numpy())[up])
    assert _lower_untouched(got, Cfill), "the strictly lower triangle is untouched"
    if bufC is not None:
        assert _nothing_outside(bufC, vC, off), "nothing outside C may be written"


# ------------------------------------------------------------------ views
@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("layout", ["odd", "padded"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,nrhs", [(129, 7), (300, 64), (384, 5)])
def test_views_match_the_aligned_call(dev, n, nrhs, dtype, layout, fill):
    """potrf / potrs on views inside NaN-filled buffers -- offset with odd leading dimensions (element-wise forms), and
    16-byte aligned with padded rows (16-byte forms, lda != n): the bits of the aligned call, nothing outside the views
    written, the lower triangle (NaN or a canary) bit for bit untouched."""
    import torch

    A = cc.fill_lower(cc.spd(n, 1, dtype), fill)
    B = np.random.default_rng(n).standard_normal((n, nrhs)).astype(dtype)
    ref = torch.from_numpy(A).cuda()
    assert int(dev.potrf_(ref).item()) == 0
    refX = torch.from_numpy(B).cuda()
    dev.potrs_(ref, refX)
    bufA, vA, offA = _view_in(torch.from_numpy(A).cuda(), layout, 1, 3)
    bufB, vB, offB = _view_in(torch.from_numpy(B).cuda(), layout, 3, 5)
    assert int(dev.potrf_(vA).item()) == 0
    got = vA.cpu().numpy()
    dev.potrs_(vA, vB)
    torch.cuda.synchronize()
    up = np.triu_indices(n)
    assert np.array_equal(_bits(got)[up], _bits(ref.cpu().numpy())[up])
    assert _lower_untouched(got, A) and _lower_untouched(ref.cpu().numpy(), A)
    assert np.array_equal(_bits(vA.cpu().numpy()), _bits(got)), "potrs reads the factor only"
    assert np.array_equal(_bits(vB.cpu().numpy()), _bits(refX.cpu().numpy()))
    assert _nothing_outside(bufA, vA, offA) and _nothing_outside(bufB, vB, offB), "nothing outside the views is written"


# ------------------------------------------------------------------ rounded inputs against Higham's bounds
@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [129, 300, 600])
def test_rounded_inputs_within_highams_bounds(dev, n, dtype, fill):
    """A = G G^T / n + I.  max |A - U^T U| / (|U^T| |U|) <= gamma_{n+1};  max |b - A x| / (|U^T| |U| |x|) <= gamma_{3n+1}
    for x from potrs, and, as a second factorisation of the same full matrix, for x from lsx_gesv_* by the same
    yardstick (not value against value)."""
    from linalg_solver_amd import dense

    A = cc.spd(n, 0, dtype)
    B = np.random.default_rng(n).standard_normal((n, 7)).astype(dtype)
    u = cc.UNIT[np.dtype(dtype)]
    Ain = cc.fill_lower(A, fill)
    R, info = _potrf_dev(dev, Ain)
    assert info == 0 and _lower_untouched(R, Ain) and not np.isnan(np.triu(R)).any()
    fr = cc.factor_residual(A, R)
    X = _potrs_dev(dev, R, B)
    assert not np.isnan(X).any()
    sr = cc.solve_residual(A, R, B, X)
    Xlu, linfo, _ = dense.solve(A, B, dtype=dtype)
    assert linfo == 0
    lr = cc.solve_residual(A, R, B, Xlu)
    print(f"n={n} {np.dtype(dtype).name}: factor {fr / u:.2f} u (bound {cc.gamma(n + 1, dtype) / u:.0f} u), potrs "
          f"{sr / u:.2f} u, gesv {lr / u:.2f} u (bound {cc.gamma(3 * n + 1, dtype) / u:.0f} u)")
    assert fr <= cc.gamma(n + 1, dtype)
    assert sr <= cc.gamma(3 * n + 1, dtype)
    assert lr <= cc.gamma(3 * n + 1, dtype)


# ------------------------------------------------------------------ remaining cases
@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_two_calls_give_identical_bits(dev, dtype, fill):
    n, nrhs = 300, 64
    A = cc.fill_lower(cc.spd(n, 2, dtype), fill)
    B = np.random.default_rng(5).standard_normal((n, nrhs)).astype(dtype)
    R1, _ = _potrf_dev(dev, A)
    R2, _ = _potrf_dev(dev, A)
    assert np.array_equal(_bits(R1), _bits(R2)) and _lower_untouched(R1, A)
    assert np.array_equal(_bits(_potrs_dev(dev, R1, B)), _bits(_potrs_dev(dev, R1, B)))


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_host_layers(dev, dtype, fill):
    """dense.cho_factor / cho_solve / solve(assume_pos=True) and Matrix.cholesky_array / solve_array(pos_def=True) on
    the same system, host and device-resident; trans=True is accepted."""
    import torch

    from linalg_solver_amd import dense
    from linalg_solver_amd.matrix import Matrix

    n = 200
    A = cc.spd(n, 3, dtype)
    B = np.random.default_rng(9).standard_normal((n, 5)).astype(dtype)
    bound = cc.gamma(3 * n + 1, dtype)
    Afill = cc.fill_lower(A, fill)
    U, info = dense.cho_factor(Afill, dtype=dtype)
    assert info == 0 and np.array_equal(np.tril(U, -1), np.zeros_like(U)) and U.dtype == dtype
    assert cc.factor_residual(A, U) <= cc.gamma(n + 1, dtype)
    X = dense.cho_solve(U, B)
    assert cc.solve_residual(A, U, B, X) <= bound
    x1 = dense.cho_solve(U, B[:, 0])
    assert x1.shape == (n,) and cc.solve_residual(A, U, B[:, :1], x1) <= bound
    Ufill = cc.fill_lower(U, fill)                     # the solve must not look below the diagonal of the factor either
    assert np.array_equal(_bits(dense.cho_solve(Ufill, B)), _bits(X))
    X2, info, _ = dense.solve(Afill, B, dtype=dtype, assume_pos=True)
    assert info == 0 and cc.solve_residual(A, U, B, X2) <= bound
    if dtype == np.float64:
        b = B[:, 0]
        dA = torch.from_numpy(Afill).cuda()
        for M in (Matrix.from_numpy(Afill), Matrix.from_dlpack(dA)):
            Um = M.cholesky_array()
            Um = Um.cpu().numpy() if hasattr(Um, "cpu") else Um
            assert np.array_equal(_bits(Um), _bits(U))
            for kw in ({}, {"trans": True}):
                x = M.solve_array(b, pos_def=True, **kw)
                x = x.cpu().numpy() if hasattr(x, "cpu") else x
                assert x.shape == (n,) and cc.solve_residual(A, U, b, x) <= bound
            Xm = M.solve_array(B, pos_def=True)
            Xm = Xm.cpu().numpy() if hasattr(Xm, "cpu") else Xm
            assert Xm.shape == B.shape and cc.solve_residual(A, U, B, Xm) <= bound
        assert np.array_equal(_bits(dA.cpu().numpy()), _bits(Afill)), "the caller's tensor is never written"


def test_matrix_keyword_conflicts(dev):
    from linalg_solver_amd.matrix import Matrix

    M = Matrix.from_numpy(np.eye(4) * 4.0)      # U = 2 I: every operation is exact
    b = np.ones(4)
    with pytest.raises(ValueError, match="pos_def"):
        M.solve_array(b, pos_def=True, bounds=True)
    with pytest.raises(ValueError, match="pos_def"):
        M.solve_array(b, pos_def=True, equilibrate=True)
    assert np.array_equal(M.solve_array(b, pos_def=True), np.full(4, 0.25))
    assert np.array_equal(M.solve_array(b), np.full(4, 0.25)), "the default path is unchanged"


@pytest.mark.parametrize("dtype", DTYPES)
def test_argument_errors_and_empty_problems(dev, dtype):
    import torch

    lib, h, sfx = dev.lib, dev.h.ptr, _sfx(dtype)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    n, nrhs = 8, 3
    A = torch.eye(n, dtype=tdt, device="cuda") * 4
    B = torch.ones(n, nrhs, dtype=tdt, device="cuda")
    info = torch.full((1,), -9, dtype=torch.int32, device="cuda")
    a, b, i = A.data_ptr(), B.data_ptr(), info.data_ptr()
    potrf, potrs = getattr(lib, f"lsx_potrf_{sfx}_dev"), getattr(lib, f"lsx_potrs_{sfx}_dev")
    syrk = getattr(lib, f"lsx_syrk_tn_sub_{sfx}_dev")
    assert potrf(h, n, a, n - 1, i) == -1 and b"bad argument" in lib.lsx_last_error()
    assert potrf(h, -1, a, n, i) == -1
    assert potrf(h, n, None, n, i) == -1
    assert potrs(h, n, nrhs, a, n - 1, b, nrhs) == -1
    assert potrs(h, n, nrhs, a, n, b, nrhs - 1) == -1
    assert potrs(h, -1, nrhs, a, n, b, nrhs) == -1
    assert potrs(h, n, -1, a, n, b, nrhs) == -1
    assert potrs(h, n, nrhs, None, n, b, nrhs) == -1
    assert potrs(h, n, nrhs, a, n, None, nrhs) == -1
    assert syrk(h, n, 4, a, n - 1, a, n) == -1
    assert syrk(h, n, 4, a, n, a, n - 1) == -1
    assert syrk(h, -1, 4, a, n, a, n) == -1 and syrk(h, n, -1, a, n, a, n) == -1
    assert syrk(h, n, 4, None, n, a, n) == -1 and syrk(h, n, 4, a, n, None, n) == -1
    # empty problems: LSX_OK, nothing touched, no pointers needed
    assert potrf(h, 0, None, 1, None) == 0 and potrf(h, 0, a, n, i) == 0
    assert potrs(h, 0, nrhs, None, 1, None, nrhs) == 0 and potrs(h, n, 0, None, n, None, 1) == 0
    assert potrs(h, n, 0, a, n, b, nrhs) == 0
    assert syrk(h, 0, 4, None, 1, None, 1) == 0 and syrk(h, n, 0, None, n, None, n) == 0
    ct = C.c_double if dtype == np.float64 else C.c_float
    hb = np.ones((n, nrhs), dtype=dtype)
    hinfo = C.c_int(-9)
    for name in ("potrs", "posv"):
        fn = getattr(lib, f"lsx_{name}_{sfx}")
        args = (h, n, 0, None, n, hb.ctypes.data_as(C.POINTER(ct)), nrhs)
        assert fn(*args, C.byref(hinfo)) == 0 if name == "posv" else fn(*args) == 0
    assert getattr(lib, f"lsx_potrf_{sfx}")(h, 0, None, 1, C.byref(hinfo)) == 0
    assert getattr(lib, f"lsx_posv_{sfx}")(h, n, nrhs, None, n, hb.ctypes.data_as(C.POINTER(ct)), nrhs, None) == -1
    torch.cuda.synchronize()
    assert bool((A == torch.eye(n, dtype=tdt, device="cuda") * 4).all()) and bool((B == 1).all())
    assert int(info.item()) == -9 and hinfo.value == -9 and np.array_equal(hb, np.ones((n, nrhs), dtype=dtype))
    # d_info may be NULL
    assert potrf(h, n, a, n, None) == 0
    torch.cuda.synchronize()
    assert bool((torch.triu(A) == torch.eye(n, dtype=tdt, device="cuda") * 2).all())
    with pytest.raises(ValueError):
        dev.potrf_(A.t()[:, :])          # not row-major
    with pytest.raises(ValueError):
        dev.potrf_(B)
    for bad in (torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32),
                torch.zeros(0, dtype=torch.int32, device="cuda")):
        with pytest.raises(ValueError, match="info"):
            dev.potrf_(A, bad)
    with pytest.raises(ValueError):
        dev.potrs_(A, B[:4])
    with pytest.raises(TypeError):
        dev.potrs_(A, B.to(torch.float32 if dtype == np.float64 else torch.float64))
    with pytest.raises(ValueError):
        dev.syrk_tn_sub_(A, B)
