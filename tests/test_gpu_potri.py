"""The SPD inverse and determinant from the Cholesky factor on the MI355X (lsx_potri_* / lsx_poinv_* / lsx_lauum_tn_* /
lsx_trtri_upper_t_* / lsx_symmetrize_upper_* / lsx_podet_*), through the C ABI, `dense`, `DeviceSolver` and `Matrix`.
The yardsticks are those tests/test_potri_host.py proves on the CPU: planted inverses bit for bit, the bits of the
full-depth product for the trapezoid product, LAPACK's test ratio beside LAPACK's own result on rounded inputs.  Every
case runs with the strictly lower triangle filled with NaN and again with a canary value: it must come back bit for bit.
"""
import ctypes as C
import math

import numpy as np
import pytest

import cpu_chol as cc
import cpu_potri as cp

pytestmark = pytest.mark.gpu

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


def _ct(dtype):
    return C.c_double if np.dtype(dtype) == np.float64 else C.c_float


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _lower_untouched(R, A):
    lo = np.tril_indices(A.shape[0], -1)
    return np.array_equal(_bits(R)[lo], _bits(A)[lo])


def _upper_equal(R, X):
    up = np.triu_indices(X.shape[0])
    return np.array_equal(_bits(R)[up], _bits(X)[up])


def _tiles(n):
    t = (n + 127) // 128
    return t * (t + 1) // 2


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _potri_dev(dev, R):
    """lsx_potri_*_dev on a device copy of the factor array R: (result as numpy, info)."""
    import torch

    t = _cuda(R)
    info = dev.potri_(t)
    torch.cuda.synchronize()
    return t.cpu().numpy(), int(info.item())


def _potri_host(dev, R):
    X = np.ascontiguousarray(R).copy()
    n = X.shape[0]
    info = C.c_int(-7)
    fn = getattr(dev.lib, f"lsx_potri_{_sfx(X.dtype)}")
    assert fn(dev.h.ptr, n, X.ctypes.data_as(C.POINTER(_ct(X.dtype))), n, C.byref(info)) == 0
    return X, info.value


def _poinv_host(dev, A, out=None):
    A = np.ascontiguousarray(A)
    keep = A.copy()
    n = A.shape[0]
    X = np.full((n, n), 5.5, dtype=A.dtype) if out is None else out
    info = C.c_int(-7)
    p = C.POINTER(_ct(A.dtype))
    fn = getattr(dev.lib, f"lsx_poinv_{_sfx(A.dtype)}")
    assert fn(dev.h.ptr, n, A.ctypes.data_as(p), n, X.ctypes.data_as(p), n, C.byref(info)) == 0
    assert np.array_equal(_bits(A), _bits(keep)), "poinv does not modify A"
    return X, info.value


def _offset_view(src, ld, offset, fillv=float("nan")):
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


# ------------------------------------------------------------------ planted inverses, bit for bit
@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", cp.PLANTED_ORDERS)
def test_planted_inverse_bit_for_bit(dev, n, dtype, fill):
    """lsx_potri_*_dev, the host form and lsx_poinv_* return the planted inverse exactly; the strictly lower triangle
    comes back bit for bit except from poinv, whose two triangles are equal."""
    U, A, V, X = cp.planted(n, dtype=dtype)
    Uin = cc.fill_lower(U, fill)
    R, info = _potri_dev(dev, Uin)
    assert info == 0 and _upper_equal(R, X) and _lower_untouched(R, Uin)
    assert dev.h.get_option("potri_tiles") == _tiles(n)
    assert dev.h.get_option("potri_order") == 0
    Rh, info = _potri_host(dev, Uin)
    assert info == 0 and _upper_equal(Rh, X) and _lower_untouched(Rh, Uin), "host-buffer form"
    Xf, info = _poinv_host(dev, cc.fill_lower(A, fill))
    assert info == 0 and np.array_equal(_bits(Xf), _bits(X)), "poinv: the full inverse, both triangles"


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", cp.PLANTED_ORDERS)
def test_planted_inverse_through_the_python_layers(dev, n, dtype, fill):
    import torch

    from linalg_solver_amd import dense
    from linalg_solver_amd.matrix import Matrix

    U, A, V, X = cp.planted(n, dtype=dtype)
    Afill = cc.fill_lower(A, fill)
    assert np.array_equal(_bits(dense.cho_inverse(cc.fill_lower(U, fill))), _bits(X))
    Xd, info, ratio = dense.inv(Afill, dtype=dtype, assume_pos=True)
    assert info == 0 and ratio == 1.0 and Xd.dtype == dtype and np.array_equal(_bits(Xd), _bits(X))
    t = _cuda(cc.fill_lower(U, fill))
    assert int(dev.potri_(t).item()) == 0
    got = t.cpu().numpy()
    assert _upper_equal(got, X) and _lower_untouched(got, cc.fill_lower(U, fill))
    dev.symmetrize_upper_(t)
    assert np.array_equal(_bits(t.cpu().numpy()), _bits(X)), "symmetrize_upper_ mirrors the upper triangle"
    if dtype == np.float64:
        dA = _cuda(Afill)
        for M in (Matrix.from_numpy(Afill), Matrix.from_dlpack(dA)):
            Xm = M.inverse_array(pos_def=True)
            Xm = Xm.cpu().numpy() if hasattr(Xm, "cpu") else Xm
            assert np.array_equal(_bits(Xm), _bits(X))
        assert np.array_equal(_bits(dA.cpu().numpy()), _bits(Afill)), "the caller's tensor is never written"


# ------------------------------------------------------------------ the two phases on their own
@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("layout", ["aligned", "odd", "padded"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 127, 128, 129, 384, 400])
def test_lauum_tn_has_the_bits_of_the_full_product(dev, n, dtype, layout, fill):
    """Upper triangle: bit-equal to the full-depth TN product of the zero-completed V onto zeros -- in fp64
    lsx_gemm_tn_add_f64_dev; in fp32, which has no add form, lsx_gemm_tn_sub_f32_dev with the first operand negated:
    the sign is folded into that operand on its way into LDS, so the MFMA sees the same numbers.  V carries NaN in the
    blocks strictly above its diagonal blocks; nothing outside the upper triangle of C is written.  Both tile orders."""
    import torch

    rng = np.random.default_rng(17 * n + 3)
    V0 = np.tril(rng.uniform(-1, 1, (n, n))).astype(dtype)
    tV0 = _cuda(V0)
    full = torch.zeros(n, n, dtype=tV0.dtype, device="cuda")
    if dtype == np.float64:
        dev.gemm_tn_add_(full, tV0, tV0)
    else:
        dev.gemm_tn_sub_(full, -tV0, tV0)
    Cfill = cc.fill_lower(np.full((n, n), 3.25, dtype=dtype), fill)
    tV, Cin = _cuda(cp.lower_blocks_nan(V0)), _cuda(Cfill)
    if layout == "aligned":
        vV, vC, bufC, off = tV, Cin, None, 0
    else:
        _, vV, _ = _view_in(tV, layout, 1, 3)
        bufC, vC, off = _view_in(Cin, layout, 3, 5)
    want = full.cpu().numpy()
    try:
        for order in (0, 1):
            vC.copy_(_cuda(Cfill))
            dev.h.set_option("potri_order", order)
            dev.lauum_tn_(vC, vV)
            torch.cuda.synchronize()
            got = vC.cpu().numpy()
            assert dev.h.get_option("potri_order") == order
            assert dev.h.get_option("potri_tiles") == _tiles(n)
            assert _upper_equal(got, want), f"order {order}"
            assert _lower_untouched(got, Cfill), "the strictly lower triangle is untouched"
            if bufC is not None:
                assert _nothing_outside(bufC, vC, off), "nothing outside C may be written"
    finally:
        dev.h.set_option("potri_order", 0)


@pytest.mark.parametrize("layout", ["aligned", "odd", "padded"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", cp.PLANTED_ORDERS)
def test_trtri_upper_t_planted(dev, n, dtype, layout):
    """Planted V exactly; the blocks above the diagonal blocks of dV keep their NaN; U is read only."""
    import torch

    U, A, V, X = cp.planted(n, dtype=dtype)
    Uin = cc.fill_lower(U, np.nan)
    tU = _cuda(Uin)
    Vin = _cuda(np.full((n, n), np.nan, dtype=dtype))
    if layout == "aligned":
        vU, vV, bufV, off = tU, Vin, None, 0
    else:
        _, vU, _ = _view_in(tU, layout, 1, 3)
        bufV, vV, off = _view_in(Vin, layout, 3, 5)
    dev.trtri_upper_t_(vV, vU)
    torch.cuda.synchronize()
    assert np.array_equal(vV.cpu().numpy(), cp.lower_blocks_nan(V), equal_nan=True)
    assert np.array_equal(_bits(vU.cpu().numpy()), _bits(Uin)), "the factor is read only"
    if bufV is not None:
        assert _nothing_outside(bufV, vV, off)


@pytest.mark.parametrize("layout", ["aligned", "odd", "padded"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 31, 32, 33, 129, 400])
def test_symmetrize_upper(dev, n, dtype, layout):
    import torch

    Aup = np.random.default_rng(n).uniform(-1, 1, (n, n)).astype(dtype)
    t = _cuda(cc.fill_lower(Aup, np.nan))
    if layout == "aligned":
        v, buf, off = t, None, 0
    else:
        buf, v, off = _view_in(t, layout, 3, 5)
    dev.symmetrize_upper_(v)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(v.cpu().numpy()), _bits(cp.symmetrize(Aup)))
    if buf is not None:
        assert _nothing_outside(buf, v, off)


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("layout", ["aligned", "odd", "padded"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 127, 129, 300, 384, 400])
def test_potri_is_its_two_phases(dev, n, dtype, layout, fill):
    """lsx_potri_*_dev has the bits of lsx_trtri_upper_t_*_dev followed by lsx_lauum_tn_*_dev with the option
    "lauum_descending" = 1, the k-slab order potri always runs, on rounded inputs where the order shows; that form too
    leaves the strictly lower triangle of C and everything outside it alone and never reads the blocks of V above its
    diagonal blocks (they hold NaN), in both tile orders.  With the option at 0 the product differs in some element once
    a tile has more than one slab: the two orders are two roundings, not one."""
    import torch

    A = cc.fill_lower(cc.spd(n, 5, dtype), fill)
    tU = _cuda(A)
    assert int(dev.potrf_(tU).item()) == 0
    want = tU.clone()
    assert int(dev.potri_(want).item()) == 0
    want = want.cpu().numpy()
    tV = _cuda(np.full((n, n), np.nan, dtype=dtype))
    dev.trtri_upper_t_(tV, tU)
    Cfill = cc.fill_lower(np.full((n, n), 3.25, dtype=dtype), fill)
    if layout == "aligned":
        vV, vC, bufC, off = tV, _cuda(Cfill), None, 0
    else:
        _, vV, _ = _view_in(tV, layout, 1, 3)
        bufC, vC, off = _view_in(_cuda(Cfill), layout, 3, 5)
    assert dev.h.get_option("lauum_descending") == 0
    try:
        dev.h.set_option("lauum_descending", 1)
        for order in (0, 1):
            vC.copy_(_cuda(Cfill))
            dev.h.set_option("potri_order", order)
            dev.lauum_tn_(vC, vV)
            torch.cuda.synchronize()
            got = vC.cpu().numpy()
            assert _upper_equal(got, want), f"order {order}"
            assert _lower_untouched(got, Cfill)
            if bufC is not None:
                assert _nothing_outside(bufC, vC, off)
        dev.h.set_option("lauum_descending", 0)
        dev.lauum_tn_(vC, vV)
        torch.cuda.synchronize()
        assert _upper_equal(vC.cpu().numpy(), want) == (n <= 16)
    finally:
        dev.h.set_option("lauum_descending", 0)
        dev.h.set_option("potri_order", 0)


# ------------------------------------------------------------------ rounded inputs beside LAPACK
@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [129, 300, 600])
def test_rounded_inputs_beside_lapack(dev, n, dtype, fill):
    """LAPACK's test ratio ||I - A X||_1 / (n u ||A||_1 ||X||_1) in extended precision, for the GPU's potrf + potri and
    for scipy's potrf + potri of the same input: the GPU may be at most 4x LAPACK's.

    lsx_potri_* sums every tile of V^T V over its k-slabs of 16 in DESCENDING order.  On these diagonally dominant inputs
    the term k = col of sum_{k >= col} v[k][row] v[k][col] carries v[col][col] and dominates; ascending k meets it first,
    so every later addition is rounded at the size of the whole sum, which measured 4.1 to 5.8 x LAPACK's ratio at
    n = 300 and 600 (dlauu2 adds that term last).  Measured on the MI355X with the descending slabs (GPU, LAPACK,
    quotient; the fill makes no difference):
        n = 129  fp64 0.00895  0.00577  1.55     fp32 0.00700  0.00461  1.52
        n = 300  fp64 0.00307  0.00196  1.56     fp32 0.00290  0.00194  1.50
        n = 600  fp64 0.00160  0.00101  1.59     fp32 0.00158  0.00101  1.56
    DESIGN.md section 3.9."""
    import torch
    from scipy.linalg import lapack

    A = cc.spd(n, 0, dtype)
    Ain = cc.fill_lower(A, fill)
    t = _cuda(Ain)
    assert int(dev.potrf_(t).item()) == 0
    assert int(dev.potri_(t).item()) == 0
    torch.cuda.synchronize()
    got = t.cpu().numpy()
    assert _lower_untouched(got, Ain) and not np.isnan(np.triu(got)).any()
    pre = "d" if dtype == np.float64 else "s"
    c, i1 = getattr(lapack, pre + "potrf")(A, lower=0)
    L, i2 = getattr(lapack, pre + "potri")(c, lower=0)
    assert i1 == 0 and i2 == 0
    mine, theirs = cp.inverse_ratio(A, cp.symmetrize(got)), cp.inverse_ratio(A, cp.symmetrize(L))
    print(f"potri n={n} {np.dtype(dtype).name}: GPU {mine:.5f}, LAPACK {theirs:.5f}, GPU / LAPACK {mine / theirs:.2f}")
    assert mine <= 4 * theirs


# ------------------------------------------------------------------ further cases
@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_two_calls_give_identical_bits(dev, dtype, fill):
    n = 300
    A = cc.fill_lower(cc.spd(n, 2, dtype), fill)
    t = _cuda(A)
    assert int(dev.potrf_(t).item()) == 0
    R = t.cpu().numpy()
    X1, i1 = _potri_dev(dev, R)
    X2, i2 = _potri_dev(dev, R)
    assert i1 == 0 and i2 == 0 and np.array_equal(_bits(X1), _bits(X2)) and _lower_untouched(X1, A)


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("layout", ["odd", "padded"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [129, 300, 384])
def test_views_match_the_aligned_call(dev, n, dtype, layout, fill):
    import torch

    A = cc.fill_lower(cc.spd(n, 1, dtype), fill)
    ref = _cuda(A)
    assert int(dev.potrf_(ref).item()) == 0
    R = ref.cpu().numpy()
    assert int(dev.potri_(ref).item()) == 0
    buf, v, off = _view_in(_cuda(R), layout, 1, 3)
    assert int(dev.potri_(v).item()) == 0
    torch.cuda.synchronize()
    got = v.cpu().numpy()
    assert _upper_equal(got, ref.cpu().numpy()) and _lower_untouched(got, A)
    assert _nothing_outside(buf, v, off), "nothing outside the view is written"


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bad", [0.0, np.nan], ids=["zero", "nan"])
@pytest.mark.parametrize("i", [0, 127, 128, 300])
def test_zero_or_nan_on_the_diagonal(dev, i, bad, dtype, fill):
    """info = i + 1 and the call returns; the lower triangle stays untouched whatever the upper one holds."""
    n = 384
    U = cp.planted(n, dtype=dtype)[0]
    U[i, i] = bad
    Uin = cc.fill_lower(U, fill)
    R, info = _potri_dev(dev, Uin)
    assert info == i + 1 and _lower_untouched(R, Uin)
    Rh, info = _potri_host(dev, Uin)
    assert info == i + 1 and _lower_untouched(Rh, Uin)
    t = _cuda(Uin)
    name = f"lsx_potri_{_sfx(dtype)}_dev"                         # d_info may be NULL
    assert getattr(dev.lib, name)(dev.h.ptr, n, t.data_ptr(), n, None) == 0
    assert _lower_untouched(t.cpu().numpy(), Uin)


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("j", [0, 127, 128, 300])
def test_not_positive_definite_poinv(dev, j, dtype, fill):
    n = 384
    U, A = cc.planted_not_pd(n, j, "negative", dtype=dtype)
    out = np.full((n, n), 5.5, dtype=dtype)
    X, info = _poinv_host(dev, cc.fill_lower(A, fill), out)
    assert info == j + 1 and (X == 5.5).all(), "poinv leaves Ainv untouched when the matrix is not positive definite"
    s, m, e, hinfo = C.c_double(9), C.c_double(9), C.c_int64(9), C.c_int(-7)
    Ain = np.ascontiguousarray(cc.fill_lower(A, fill))
    fn = getattr(dev.lib, f"lsx_podet_{_sfx(dtype)}")
    assert fn(dev.h.ptr, n, Ain.ctypes.data_as(C.POINTER(_ct(dtype))), n, C.byref(s), C.byref(m), C.byref(e), C.byref(hinfo)) == 0
    assert hinfo.value == j + 1 and (s.value, m.value, e.value) == (0.0, 0.0, 0)


def test_not_positive_definite_through_matrix_and_dense(dev):
    from linalg_solver_amd import dense
    from linalg_solver_amd.matrix import Matrix

    n, j = 140, 130
    U, A = cc.planted_not_pd(n, j, "negative")
    X, info, ratio = dense.inv(A, assume_pos=True)
    assert X is None and info == j + 1 and ratio == 1.0
    for fn in (dense.det_parts, dense.slogdet, dense.det):
        with pytest.raises(ValueError, match=f"leading minor of order {j + 1}"):
            fn(A, assume_pos=True)
    assert dense.det_parts_pos(A) == (0.0, 0.0, 0, j + 1)
    for M in (Matrix.from_numpy(A), Matrix.from_dlpack(_cuda(A))):
        with pytest.raises(ValueError, match=f"leading minor of order {j + 1}"):
            M.inverse_array(pos_def=True)
        with pytest.raises(ValueError, match=f"leading minor of order {j + 1}"):
            M.slogdet(pos_def=True)


# ------------------------------------------------------------------ determinant
@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", cp.PLANTED_ORDERS)
def test_planted_determinant_exactly(dev, n, dtype, fill):
    from linalg_solver_amd import dense

    U, A, _, _ = cp.planted(n, dtype=dtype)
    want = cp.planted_det_parts(n)
    got = dev.podet_parts(_cuda(cc.fill_lower(U, fill))).cpu().numpy()
    assert tuple(got) == want
    Afill = cc.fill_lower(A, fill)
    assert dense.det_parts(Afill, dtype=dtype, assume_pos=True) == want
    assert dense.det_parts_pos(Afill, dtype=dtype) == want + (0,)
    s, logdet = dense.slogdet(Afill, dtype=dtype, assume_pos=True)
    assert s == 1.0 and logdet == math.log(0.5) + want[2] * math.log(2.0)
    if want[2] < 1000:
        assert dense.det(Afill, assume_pos=True) == math.ldexp(0.5, want[2])
    Uz = U.copy()
    Uz[n // 2, n // 2] = 0
    assert tuple(dev.podet_parts(_cuda(Uz)).cpu().numpy()) == (0.0, 0.0, 0.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_determinant_beside_the_lu_route(dev, dtype):
    """slogdet of spd(300) by both routes: the logarithms agree to n u relative to the sum of |log u_ii^2| terms -- each
    u_ii carries a relative error of a few u from either factorisation, n of them add up in the logarithm."""
    from linalg_solver_amd import dense
    from linalg_solver_amd.matrix import Matrix

    n = 300
    A = cc.spd(n, 0, dtype)
    s1, l1 = dense.slogdet(A, dtype=dtype)
    s2, l2 = dense.slogdet(cc.fill_lower(A, np.nan), dtype=dtype, assume_pos=True)
    u = cc.UNIT[np.dtype(dtype)]
    print(f"slogdet n={n} {np.dtype(dtype).name}: LU {l1!r}, Cholesky {l2!r}, difference {abs(l1 - l2) / u:.1f} u")
    assert s1 == 1.0 and s2 == 1.0 and abs(l1 - l2) <= n * u * max(1.0, abs(l1))
    if dtype == np.float64:
        assert Matrix.from_numpy(A).slogdet(pos_def=True) == (s2, l2)
        assert Matrix.from_numpy(A).slogdet() == (s1, l1), "the default path is unchanged"


# ------------------------------------------------------------------ arguments, empty problems, shared work space
@pytest.mark.parametrize("dtype", DTYPES)
def test_argument_errors_and_empty_problems(dev, dtype):
    import torch

    from linalg_solver_amd._native import LsxError

    lib, h, sfx = dev.lib, dev.h.ptr, _sfx(dtype)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    n = 8
    A = torch.eye(n, dtype=tdt, device="cuda") * 2
    B = torch.ones(n, 3, dtype=tdt, device="cuda")
    V = torch.ones(n, n, dtype=tdt, device="cuda")
    info = torch.full((1,), -9, dtype=torch.int32, device="cuda")
    out = torch.full((3,), -9.0, dtype=torch.float64, device="cuda")
    a, v, i, o = A.data_ptr(), V.data_ptr(), info.data_ptr(), out.data_ptr()
    potri, sym = getattr(lib, f"lsx_potri_{sfx}_dev"), getattr(lib, f"lsx_symmetrize_upper_{sfx}_dev")
    lauum, trtri = getattr(lib, f"lsx_lauum_tn_{sfx}_dev"), getattr(lib, f"lsx_trtri_upper_t_{sfx}_dev")
    podet = getattr(lib, f"lsx_podet_{sfx}_dev")
    assert potri(h, n, a, n - 1, i) == -1 and b"bad argument" in lib.lsx_last_error()
    assert potri(h, -1, a, n, i) == -1 and potri(h, n, None, n, i) == -1
    assert sym(h, n, a, n - 1) == -1 and sym(h, -1, a, n) == -1 and sym(h, n, None, n) == -1
    for fn in (lauum, trtri):
        assert fn(h, n, a, n - 1, v, n) == -1 and fn(h, n, a, n, v, n - 1) == -1 and fn(h, -1, a, n, v, n) == -1
        assert fn(h, n, None, n, v, n) == -1 and fn(h, n, a, n, None, n) == -1
    assert podet(h, n, a, n - 1, o) == -1 and podet(h, -1, a, n, o) == -1
    assert podet(h, n, None, n, o) == -1 and podet(h, n, a, n, None) == -1
    # empty problems: LSX_OK, nothing touched, no pointers needed
    assert potri(h, 0, None, 1, None) == 0 and potri(h, 0, a, n, i) == 0
    assert sym(h, 0, None, 1) == 0 and lauum(h, 0, None, 1, None, 1) == 0 and trtri(h, 0, None, 1, None, 1) == 0
    ct = _ct(dtype)
    hinfo = C.c_int(-9)
    hx = np.full((n, n), 5.5, dtype=dtype)
    assert getattr(lib, f"lsx_potri_{sfx}")(h, 0, None, 1, C.byref(hinfo)) == 0
    assert getattr(lib, f"lsx_poinv_{sfx}")(h, 0, None, 1, None, 1, C.byref(hinfo)) == 0
    assert getattr(lib, f"lsx_poinv_{sfx}")(h, n, None, n, hx.ctypes.data_as(C.POINTER(ct)), n, None) == -1
    assert getattr(lib, f"lsx_poinv_{sfx}")(h, n, hx.ctypes.data_as(C.POINTER(ct)), n, None, n, None) == -1
    assert getattr(lib, f"lsx_potri_{sfx}")(h, n, None, n, None) == -1
    torch.cuda.synchronize()
    assert bool((A == torch.eye(n, dtype=tdt, device="cuda") * 2).all()) and bool((V == 1).all())
    assert int(info.item()) == -9 and hinfo.value == -9 and (hx == 5.5).all() and bool((out == -9).all())
    s, m, e = C.c_double(9), C.c_double(9), C.c_int64(9)
    assert getattr(lib, f"lsx_podet_{sfx}")(h, 0, None, 1, C.byref(s), C.byref(m), C.byref(e), None) == 0
    assert (s.value, m.value, e.value) == (1.0, 0.5, 1), "det([]) = 1"
    assert getattr(lib, f"lsx_podet_{sfx}")(h, n, None, n, C.byref(s), C.byref(m), C.byref(e), None) == -1
    assert podet(h, 0, None, 1, o) == 0
    assert tuple(out.cpu().numpy()) == (1.0, 0.5, 1.0)
    # d_info may be NULL; U = 2 I gives inv(A) = I / 4
    assert potri(h, n, a, n, None) == 0
    torch.cuda.synchronize()
    assert bool((A == torch.eye(n, dtype=tdt, device="cuda") / 4).all())
    with pytest.raises(ValueError):
        dev.potri_(V.t())          # not row-major
    with pytest.raises(ValueError):
        dev.potri_(B)
    for bad in (torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32),
                torch.zeros(0, dtype=torch.int32, device="cuda")):
        with pytest.raises(ValueError, match="info"):
            dev.potri_(A, bad)
    other = torch.float32 if dtype == np.float64 else torch.float64
    with pytest.raises(ValueError):
        dev.lauum_tn_(A, B)
    with pytest.raises(TypeError):
        dev.lauum_tn_(A, V.to(other))
    with pytest.raises(ValueError):
        dev.trtri_upper_t_(B, A)
    with pytest.raises(TypeError):
        dev.trtri_upper_t_(V.to(other), A)
    with pytest.raises(ValueError):
        dev.symmetrize_upper_(B)
    with pytest.raises(ValueError):
        dev.podet_parts(B)
    with pytest.raises(LsxError):
        dev.h.set_option("potri_order", 2)
    with pytest.raises(LsxError):
        dev.h.set_option("potri_tiles", 1)                      # read-only


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_handle_walks_orders_and_families(dtype):
    """One long-lived handle walks orders 300, 129, 600 across potrf_, potri_, getri and potrs_ and gets the bits a fresh
    handle gives each call: the carves of the inverse do not disturb the others'."""
    import torch

    from linalg_solver_amd.device import DeviceSolver

    old = DeviceSolver()

    def run(d, n):
        A = cc.spd(n, 4, dtype)
        B = np.random.default_rng(n).standard_normal((n, 9)).astype(dtype)
        U = _cuda(A)
        assert int(d.potrf_(U).item()) == 0
        X = U.clone()
        assert int(d.potri_(X).item()) == 0
        LU = _cuda(A)
        ipiv, info = d.getrf_(LU)
        Inv = d.getri(LU, ipiv)
        S = _cuda(B)
        d.potrs_(U, S)
        X2 = U.clone()
        assert int(d.potri_(X2).item()) == 0
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (U, X, Inv, S, X2)]

    for n in (300, 129, 600):
        got, want = run(old, n), run(DeviceSolver(), n)
        for g, w in zip(got, want):
            assert np.array_equal(_bits(g), _bits(w))
        assert np.array_equal(_bits(got[1]), _bits(got[4])), "potri after getri and potrs: the same bits"
