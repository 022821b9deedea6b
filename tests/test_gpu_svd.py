"""The one-sided Jacobi SVD and minimum-norm least squares on the MI355X (lsx_gesvdj_* / lsx_gelss_*), through the C ABI,
`dense`, `DeviceSolver` and `Matrix`, in both precisions.  The yardsticks are those tests/test_svd_host.py proves on the
CPU: on the planted inputs the numpy model (tests/cpu_svd.py) and the GPU must agree bit for bit with one sweep and no
rotation, and on rounded inputs the GPU's four ratios stay within the pooled bounds (twice the largest value the model
or LAPACK attains).  GPU results are compared with each other bit for bit.

Shapes of the Hadamard plant (cpu_svd.HADAMARD): 130 x 257 -- an even p of 65 workgroups per round, an odd width that
ends in one zero column and the padding of the work matrix; 6 x 4096 -- the longest fp64 row svd_round_kernel keeps in
registers, all 8 passes of its load, sum and store loops (fp32: 4 of 8); 6 x 16387 -- longer than the register form
holds in either precision, so the re-reading form runs its sum loop and its rotation loop 33 (fp64) / 17 (fp32) times.
Every c there is a sum of N terms that cancel exactly: a dropped or doubled chunk of a row shows up as a rotation.
cpu_svd.hadamard_doubled, 6 x 8192, is the longest fp32 row of the register form (all 8 passes); its values are not
powers of two, so there the exact statements are one sweep and no rotation.
"""
import ctypes as C

import numpy as np
import pytest

import cpu_qr as cq
import cpu_svd as cs

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
ERR_ARG = -1


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


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _t(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sync():
    import torch

    torch.cuda.synchronize()


def _svd(dev, A, compute_uv=True):
    """(U, s, Vt, info, sweeps, rotations) as numpy through DeviceSolver.gesvdj_."""
    U, s, Vt, info = dev.gesvdj_(_t(A), compute_uv=compute_uv)
    sw, rot = dev.h.get_option("gesvdj_sweeps"), dev.h.get_option("gesvdj_rotations")
    return (None if U is None else U.cpu().numpy()), s.cpu().numpy(), (None if Vt is None else Vt.cpu().numpy()), info, sw, rot


def _gelss(dev, A, B, rcond=-1.0):
    tb = _t(B)
    X, s, rank, info = dev.gelss_(_t(A), tb, rcond)
    assert _same_bits(tb.cpu().numpy(), np.ascontiguousarray(B)), "B is read only"
    return X.cpu().numpy(), s.cpu().numpy(), rank, info


# ------------------------------------------------------------------ exact plants
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tall", [False, True], ids=["6x9", "9x6"])
def test_unit_rows_exact(dev, tall, dtype):
    from linalg_solver_amd import dense

    A, s0 = cs.unit_rows(tall, False, dtype)
    U, s, Vt, info, sweeps, rot = _svd(dev, A)
    assert (info, sweeps, rot) == (0, 1, 0)
    assert _same_bits(s, s0)
    assert np.array_equal((U.astype(np.float64) * s) @ Vt.astype(np.float64), A)
    assert np.array_equal(U.T @ U, np.eye(6)) and not Vt[-1].any()
    m = cs.gesvdj(A)
    assert np.array_equal(U, m["U"]) and np.array_equal(Vt, m["Vt"])
    Uh, sh, Vh, ih = dense.svd(A, dtype=dtype, handle=dev.h)
    assert ih == 0 and _same_bits(sh, s) and _same_bits(Uh, U) and _same_bits(Vh, Vt), "host-buffer form"
    A2, _ = cs.unit_rows(tall, True, dtype)
    B, X0 = cs.unit_rows_rhs(tall, 3, dtype)
    X, s2, rank, info = _gelss(dev, A2, B)
    assert rank == 5 and info == 0 and np.array_equal(X, X0)
    Xh, resid, rk, sh2 = dense.lstsq_min_norm(A2, B, dtype=dtype, handle=dev.h)
    assert rk == 5 and _same_bits(Xh, X) and _same_bits(sh2, s2)
    assert np.allclose(resid, np.linalg.norm(B.astype(np.float64) - A2.astype(np.float64) @ X0.astype(np.float64), axis=0),
                       rtol=1e-6, atol=0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("spec", cs.HADAMARD, ids=lambda s: f"{s[0]}x{s[2]}")
def test_hadamard_rows_exact(dev, spec, dtype):
    A, U0, s0, Vt0 = cs.hadamard_rows(*spec, dtype=dtype)
    U, s, Vt, info, sweeps, rot = _svd(dev, A)
    assert (info, sweeps, rot) == (0, 1, 0), "a rotation here is a chunk of a row dropped or doubled in a sum"
    assert _same_bits(s, s0) and np.array_equal(U, U0) and np.array_equal(Vt, Vt0)
    _, sv, _, info, sweeps, rot = _svd(dev, A, compute_uv=False)
    assert (info, sweeps, rot) == (0, 1, 0) and _same_bits(sv, s)


@pytest.mark.parametrize("dtype", DTYPES)
def test_doubled_hadamard_rows_take_one_sweep(dev, dtype):
    """6 x 8192: the longest fp32 row svd_round_kernel keeps in registers, all 8 passes of its loops (fp64: re-read)."""
    A, s0 = cs.hadamard_doubled(dtype)
    U, s, Vt, info, sweeps, rot = _svd(dev, A)
    assert (info, sweeps, rot) == (0, 1, 0), "a rotation here is a chunk of a row dropped or doubled in a sum"
    assert np.allclose(s, s0, rtol=4 * cs.UNIT[np.dtype(np.float64)], atol=0)
    m = cs.gesvdj(A)
    assert np.array_equal(U, m["U"]) and np.allclose(Vt, m["Vt"], rtol=4 * cs.UNIT[np.dtype(dtype)], atol=0)


# ------------------------------------------------------------------ rounded inputs
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n", cs.ROUNDED)
def test_rounded_ratios_within_pooled_bounds(dev, m, n, dtype):
    from linalg_solver_amd import dense

    A = cs.rounded(m, n, dtype)
    U, s, Vt, info, sweeps, rot = _svd(dev, A)
    assert info == 0 and 1 <= sweeps < 30
    assert U.shape == (m, min(m, n)) and Vt.shape == (min(m, n), n) and np.all(np.diff(s) <= 0)
    got = cs.svd_ratios(A, U, s, Vt)
    bound = cs.pooled_bounds(np.dtype(dtype).name)
    print(np.dtype(dtype).name, m, n, "sweeps", sweeps, "gpu", got, "model", cs.model_ratios(m, n, np.dtype(dtype).name),
          "lapack", cs.lapack_ratios(m, n, np.dtype(dtype).name), "bound", bound)
    for g, b in zip(got, bound):
        assert g <= b
    _, s0, _, _, _, _ = _svd(dev, A, compute_uv=False)
    assert _same_bits(s0, s), "jobz = 0 gives the bits of jobz = 1"
    U2, s2, Vt2, _, _, _ = _svd(dev, A)
    assert _same_bits(U2, U) and _same_bits(s2, s) and _same_bits(Vt2, Vt), "two calls give the same bits"
    Uh, sh, Vh, ih = dense.svd(A, dtype=dtype, handle=dev.h)
    assert ih == 0 and _same_bits(sh, s) and _same_bits(Uh, U) and _same_bits(Vh, Vt), "host-buffer form"
    assert _same_bits(dense.svdvals(A, dtype=dtype, handle=dev.h), s)


@pytest.mark.parametrize("dtype", DTYPES)
def test_graded_matrix(dev, dtype):
    """sigma_i = 2^(-i / 2) at n = 64 (cpu_svd.graded): the model needs 10 to 11 sweeps, away from the cap of 30."""
    G = cs.graded(dtype)
    U, s, Vt, info, sweeps, rot = _svd(dev, G)
    assert info == 0 and sweeps <= 20
    got = cs.svd_ratios(G, U, s, Vt)
    m = cs.gesvdj(G)
    model = cs.svd_ratios(G, m["U"], m["s"], m["Vt"])
    Ul, sl, Vl = np.linalg.svd(G, full_matrices=False)
    lap = cs.svd_ratios(G, Ul, sl, Vl)
    print(np.dtype(dtype).name, "graded sweeps", sweeps, "model sweeps", m["sweeps"], "gpu", got, "model", model, "lapack", lap)
    for g, a, b in zip(got, model, lap):
        assert g <= 2.0 * max(a, b)


# ------------------------------------------------------------------ rank and minimum norm
def _lstsq_same_precision(A, b):
    return np.linalg.lstsq(A, b, rcond=cs.default_rcond(*A.shape, A.dtype))[0]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n", cs.RANK_SHAPES)
def test_rank_deficient_minimum_norm(dev, m, n, dtype):
    A, b, x = cs.rank_product(m, n, dtype)
    X, s, rank, info = _gelss(dev, A, b)
    assert rank == cs.RANK and info == 0
    got = cs.rel_err(X, x)
    model, lap = cs.rel_err(cs.gelss(A, b)["x"], x), cs.rel_err(_lstsq_same_precision(A, b), x)
    print(np.dtype(dtype).name, m, n, "gpu", got, "model", model, "lstsq", lap)
    assert got <= 2.0 * max(model, lap)


@pytest.mark.parametrize("dtype", DTYPES)
def test_wide_minimum_norm(dev, dtype):
    A, b, x = cs.wide_case(dtype)
    X, s, rank, info = _gelss(dev, A, b)
    assert rank == 5 and info == 0
    got = cs.rel_err(X, x)
    model, lap = cs.rel_err(cs.gelss(A, b)["x"], x), cs.rel_err(_lstsq_same_precision(A, b), x)
    print(np.dtype(dtype).name, "5x300 gpu", got, "model", model, "lstsq", lap)
    assert got <= 2.0 * max(model, lap)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["rank7_40x60", "rank7_60x40", "rounded_7x5", "rounded_5x7"])
def test_pinv_moore_penrose(dev, case, dtype):
    from linalg_solver_amd import dense

    if case.startswith("rank7"):
        m, n = (40, 60) if case.endswith("40x60") else (60, 40)
        A = cs.rank_product(m, n, dtype)[0]
    else:
        A = cs.rounded(*((7, 5) if case.endswith("7x5") else (5, 7)), dtype)
    X = dense.pinv(A, dtype=dtype, handle=dev.h)
    assert X.shape == A.shape[::-1] and X.dtype == A.dtype
    got = cs.pinv_residuals(A, X)
    model = cs.pinv_residuals(A, cs.gelss(A, np.eye(A.shape[0], dtype=dtype))["x"])
    lap = cs.pinv_residuals(A, np.linalg.pinv(A, rcond=cs.default_rcond(*A.shape, dtype)))
    print(np.dtype(dtype).name, case, "gpu", got, "model", model, "numpy", lap)
    for g, a, b in zip(got, model, lap):
        assert g <= 2.0 * max(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_matrix(dev, dtype):
    Zm = np.zeros((6, 6), dtype=dtype)
    U, s, Vt, info, sweeps, rot = _svd(dev, Zm)
    assert info == 0 and sweeps == 1 and rot == 0
    assert np.array_equal(s, np.zeros(6)) and np.array_equal(Vt, Zm) and np.array_equal(U.T @ U, np.eye(6))
    X, s2, rank, info = _gelss(dev, Zm, np.ones((6, 2), dtype=dtype))
    assert rank == 0 and info == 0 and np.array_equal(X, np.zeros((6, 2))) and np.array_equal(s2, np.zeros(6))


# ------------------------------------------------------------------ outcomes
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("m,n", [(5, 7), (7, 5), (130, 257), (300, 129)])
def test_nan_and_infinity_give_nan_values(dev, m, n, bad, dtype):
    A = cs.rounded(m, n, dtype).copy()
    A[m // 2, n // 3] = bad
    for uv in (True, False):
        _, s, _, info, sweeps, _ = _svd(dev, A, compute_uv=uv)
        assert np.isnan(s).all() and info == 0 and sweeps <= 1
    X, s, rank, info = _gelss(dev, A, np.ones((m, 2), dtype=dtype))
    assert np.isnan(s).all() and np.isnan(X).all() and rank == 0 and info == 0
    dev.h.check_status()


@pytest.mark.parametrize("dtype", DTYPES)
def test_sweep_cap_sets_info(dev, dtype):
    A = cs.rounded(5, 7, dtype)
    default = dev.h.get_option("gesvdj_max_sweeps")
    assert default == 30
    try:
        dev.h.set_option("gesvdj_max_sweeps", 1)
        U, s, Vt, info, sweeps, rot = _svd(dev, A)
        assert info == 1 and sweeps == 1 and rot > 0
        assert np.isfinite(s).all() and np.isfinite(U).all() and np.isfinite(Vt).all()
    finally:
        dev.h.set_option("gesvdj_max_sweeps", default)
    assert _svd(dev, A)[3] == 0
    lib = dev.lib
    for v in (0, 61, -1):
        assert lib.lsx_set_option(dev.h.ptr, b"gesvdj_max_sweeps", v) == ERR_ARG
    assert lib.lsx_set_option(dev.h.ptr, b"gesvdj_sweeps", 1) == ERR_ARG, "read-only"
    assert lib.lsx_set_option(dev.h.ptr, b"gesvdj_rotations", 1) == ERR_ARG, "read-only"
    assert dev.h.get_option("gesvdj_max_sweeps") == default


@pytest.mark.parametrize("dtype", DTYPES)
def test_argument_errors_and_empty_problems(dev, dtype):
    import torch

    lib, h, sf = dev.lib, dev.h.ptr, _sfx(dtype)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    A = torch.full((8, 8), 3.0, dtype=tdt, device="cuda")
    B = torch.full((8, 8), 5.0, dtype=tdt, device="cuda")
    W = torch.full((8, 8), 6.0, dtype=tdt, device="cuda")
    S = torch.full((8,), 7.0, dtype=torch.float64, device="cuda")
    a, b_, w, s = A.data_ptr(), B.data_ptr(), W.data_ptr(), S.data_ptr()
    svd, lss = getattr(lib, f"lsx_gesvdj_{sf}_dev"), getattr(lib, f"lsx_gelss_{sf}_dev")
    info, rank = C.c_int(5), C.c_int(5)
    pi, pr = C.byref(info), C.byref(rank)
    assert svd(h, 1, -1, 4, a, 8, s, b_, 8, w, 8, pi) == ERR_ARG and svd(h, 1, 4, -1, a, 8, s, b_, 8, w, 8, pi) == ERR_ARG
    assert svd(h, 2, 4, 4, a, 8, s, b_, 8, w, 8, pi) == ERR_ARG and svd(h, -1, 4, 4, a, 8, s, b_, 8, w, 8, pi) == ERR_ARG
    assert svd(h, 1, 4, 4, a, 3, s, b_, 8, w, 8, pi) == ERR_ARG, "lda < n"
    assert svd(h, 1, 4, 6, a, 8, s, b_, 3, w, 8, pi) == ERR_ARG, "ldu < k"
    assert svd(h, 1, 4, 6, a, 8, s, b_, 8, w, 5, pi) == ERR_ARG, "ldvt < n"
    assert svd(h, 1, 4, 4, None, 8, s, b_, 8, w, 8, pi) == ERR_ARG and svd(h, 1, 4, 4, a, 8, None, b_, 8, w, 8, pi) == ERR_ARG
    assert svd(h, 1, 4, 4, a, 8, s, None, 8, w, 8, pi) == ERR_ARG and svd(h, 1, 4, 4, a, 8, s, b_, 8, None, 8, pi) == ERR_ARG
    assert lss(h, -1, 4, 1, a, 8, b_, 8, w, 8, -1.0, s, pr, pi) == ERR_ARG and lss(h, 4, 4, -1, a, 8, b_, 8, w, 8, -1.0, s, pr, pi) == ERR_ARG
    assert lss(h, 4, 4, 2, a, 3, b_, 8, w, 8, -1.0, s, pr, pi) == ERR_ARG
    assert lss(h, 4, 4, 2, a, 8, b_, 1, w, 8, -1.0, s, pr, pi) == ERR_ARG and lss(h, 4, 4, 2, a, 8, b_, 8, w, 1, -1.0, s, pr, pi) == ERR_ARG
    assert lss(h, 4, 4, 2, None, 8, b_, 8, w, 8, -1.0, s, pr, pi) == ERR_ARG and lss(h, 4, 4, 2, a, 8, None, 8, w, 8, -1.0, s, pr, pi) == ERR_ARG
    assert lss(h, 4, 4, 2, a, 8, b_, 8, None, 8, -1.0, s, pr, pi) == ERR_ARG
    assert getattr(lib, f"lsx_gesvdj_{sf}")(h, 1, 4, 4, None, 4, None, None, 4, None, 4, None) == ERR_ARG
    assert getattr(lib, f"lsx_gelss_{sf}")(h, 4, 4, 1, None, 4, None, 1, None, 1, -1.0, None, None, None, None) == ERR_ARG
    _sync()
    assert bool((A == 3).all()) and bool((B == 5).all()) and bool((W == 6).all()) and bool((S == 7).all())
    # zero extents: LSX_OK, nothing touched, pointers may be NULL
    assert svd(h, 1, 0, 4, None, 4, None, None, 0, None, 4, pi) == 0 and info.value == 0
    assert svd(h, 1, 4, 0, None, 0, None, None, 0, None, 0, None) == 0 and svd(h, 0, 0, 0, None, 0, None, None, 0, None, 0, None) == 0
    rank.value = 5
    assert lss(h, 0, 4, 2, None, 4, None, 2, None, 2, -1.0, None, pr, pi) == 0 and rank.value == 0
    assert lss(h, 4, 0, 2, None, 0, None, 2, None, 2, -1.0, None, None, None) == 0
    assert lss(h, 4, 4, 0, None, 4, None, 0, None, 0, -1.0, None, None, None) == 0
    # values only: U and Vt may be NULL, s and info may not / may
    assert svd(h, 0, 8, 8, a, 8, s, None, 0, None, 0, None) == 0
    _sync()
    assert np.allclose(S.cpu().numpy(), [24.0] + [0.0] * 7) and bool((B == 5).all()) and bool((W == 6).all())
    # gelss without s
    A.fill_(3.0)
    assert lss(h, 8, 8, 1, a, 8, b_, 8, w, 8, -1.0, None, pr, pi) == 0 and rank.value == 1
    dev.h.check_status()


# ------------------------------------------------------------------ invariances, as bit equalities
GUARD = 64


class View:
    """rows x cols with leading dimension ld, `off` elements behind a 16-byte boundary, inside a buffer filled with
    `fill` (NaN or a canary)."""

    def __init__(self, rows, cols, pad, off, dtype, fill, data=None):
        import torch

        ld = cols + pad
        tdt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
        self.ld = ld
        self.buf = torch.full((GUARD + off + rows * ld + GUARD,), fill, dtype=tdt, device="cuda")
        self.t = torch.as_strided(self.buf, (rows, cols), (ld, 1), GUARD + off)
        inside = torch.zeros(self.buf.numel(), dtype=torch.bool, device="cuda")
        torch.as_strided(inside, (rows, cols), (ld, 1), GUARD + off).fill_(True)
        self.outside = ~inside
        self.ibits = torch.int64 if self.buf.element_size() == 8 else torch.int32
        self.keep = self.buf.view(self.ibits)[self.outside].clone()
        if data is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(data)))

    def untouched(self):
        _sync()
        return bool((self.buf.view(self.ibits)[self.outside] == self.keep).all())

    def numpy(self):
        return self.t.cpu().numpy()


@pytest.mark.parametrize("fill", [float("nan"), -777.25], ids=["nan", "canary"])
@pytest.mark.parametrize("layout", ["odd", "padded"])
@pytest.mark.parametrize("m,n", [(5, 7), (130, 257), (300, 129)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_views(dev, dtype, m, n, layout, fill):
    """A, s, U, Vt, B and X as views (odd: one element off a 16-byte boundary with an odd leading dimension; padded:
    aligned with two elements of padding) inside NaN- or canary-filled buffers: the bits of the aligned call, nothing
    outside the view written."""
    lib, h, sf = dev.lib, dev.h.ptr, _sfx(dtype)
    k, nrhs = min(m, n), 3
    A, B = cs.rounded(m, n, dtype), cq.uniform(m, nrhs, 2, dtype)
    off = 1 if layout == "odd" else 0
    pad = (lambda c: 3 if (c + 3) % 2 else 4) if layout == "odd" else (lambda c: 2)
    U0, s0, Vt0, info0, sw0, rot0 = _svd(dev, A)
    X0, _, rank0, _ = _gelss(dev, A, B)
    vA, vU, vVt = View(m, n, pad(n), off, dtype, fill, A), View(m, k, pad(k), off, dtype, fill), View(k, n, pad(n), off, dtype, fill)
    vs = View(1, k, 0, off, np.float64, fill)
    info = C.c_int(7)
    assert getattr(lib, f"lsx_gesvdj_{sf}_dev")(h, 1, m, n, vA.t.data_ptr(), vA.ld, vs.t.data_ptr(), vU.t.data_ptr(), vU.ld,
                                               vVt.t.data_ptr(), vVt.ld, C.byref(info)) == 0
    assert info.value == info0 == 0
    assert (dev.h.get_option("gesvdj_sweeps"), dev.h.get_option("gesvdj_rotations")) == (sw0, rot0)
    assert _same_bits(vs.numpy()[0], s0) and _same_bits(vU.numpy(), U0) and _same_bits(vVt.numpy(), Vt0)
    assert vA.untouched() and vs.untouched() and vU.untouched() and vVt.untouched()
    vA2, vB, vX = View(m, n, pad(n), off, dtype, fill, A), View(m, nrhs, pad(nrhs) + 1, off, dtype, fill, B), View(n, nrhs, pad(nrhs), off, dtype, fill)
    vs2 = View(1, k, 0, off, np.float64, fill)
    rank = C.c_int(-1)
    assert getattr(lib, f"lsx_gelss_{sf}_dev")(h, m, n, nrhs, vA2.t.data_ptr(), vA2.ld, vB.t.data_ptr(), vB.ld, vX.t.data_ptr(),
                                              vX.ld, -1.0, vs2.t.data_ptr(), C.byref(rank), C.byref(info)) == 0
    assert rank.value == rank0 == k and info.value == 0
    assert _same_bits(vX.numpy(), X0) and _same_bits(vs2.numpy()[0], s0) and _same_bits(vB.numpy(), B)
    assert vA2.untouched() and vB.untouched() and vX.untouched() and vs2.untouched()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n", [(5, 7), (7, 5), (130, 257), (300, 129)])
def test_power_of_two_scaling_is_an_exact_symmetry(dev, m, n, dtype):
    A = cs.rounded(m, n, dtype)
    U0, s0, Vt0, info0, sw0, rot0 = _svd(dev, A)
    for d in (20, -20):
        U, s, Vt, info, sw, rot = _svd(dev, np.ldexp(A, d))
        assert _same_bits(U, U0) and _same_bits(Vt, Vt0) and _same_bits(s, np.ldexp(s0, d))
        assert (info, sw, rot) == (info0, sw0, rot0)


def test_one_handle_across_lu_cholesky_qr_and_svd(dev):
    """Work-space ownership: the earlier families' results have the same bits before and after an SVD call."""
    import cpu_chol as cc

    _, Aq, _ = cq.planted(300, 129)
    _, bq, _ = cq.planted_rhs(300, 129, 7)
    _, S = cc.planted(257)
    G = cq.uniform(384, 384, 3)

    def families():
        ta, tb = _t(Aq), _t(bq)
        dev.gels_(ta, tb)
        tc = _t(S)
        dev.potrf_(tc)
        lu = _t(G)
        ipiv, _ = dev.getrf_(lu)
        X = _t(G.copy())
        dev.getrs_(lu, ipiv, X)
        _sync()
        return [t.cpu().numpy() for t in (ta, tb, tc, lu, X)]

    before = families()
    first = _svd(dev, cs.rounded(300, 129, np.float64))
    _gelss(dev, cs.rounded(130, 257, np.float32), cq.uniform(130, 3, 2, np.float32))
    after = families()
    for x, y in zip(before, after):
        assert _same_bits(x, y)
    second = _svd(dev, cs.rounded(300, 129, np.float64))
    for x, y in zip(first[:3], second[:3]):
        assert _same_bits(x, y)
    dev.h.check_status()


# ------------------------------------------------------------------ the Python layers
def test_host_layers(dev):
    """dense, DeviceSolver and Matrix, host route and device-tensor route, on a rank-deficient and a full-rank case."""
    import torch

    from linalg_solver_amd import Matrix, dense

    A, b, x = cs.rank_product(40, 60)
    U, s, Vt, info = dense.svd(A, handle=dev.h)
    assert info == 0 and np.allclose((U * s) @ Vt, A, rtol=0, atol=1e-12)
    assert dense.matrix_rank(A, handle=dev.h) == cs.RANK and dense.matrix_rank(A, rcond=0.9, handle=dev.h) == 1
    X, resid, rank, s2 = dense.lstsq_min_norm(A, b, handle=dev.h)
    assert rank == cs.RANK and _same_bits(s2, s) and cs.rel_err(X, x) < 1e-12
    assert np.allclose(resid, np.linalg.norm(b - A @ np.asarray(x, dtype=np.float64), axis=0), rtol=1e-9, atol=0)
    xv, rv, rk, _ = dense.lstsq_min_norm(A, b[:, 0], handle=dev.h)
    assert xv.shape == (60,) and rk == cs.RANK and np.allclose(xv, X[:, 0], rtol=0, atol=1e-13) and abs(rv - resid[0]) < 1e-12

    M = Matrix.from_numpy(A)
    Md = Matrix.from_dlpack(_t(A))
    Um, sm, Vm = M.svd_array()
    Ud, sd, Vd = Md.svd_array()
    assert _same_bits(sm, s) and _same_bits(Um, U) and _same_bits(Vm, Vt)
    assert torch.is_tensor(Ud) and _same_bits(sd.cpu().numpy(), s) and _same_bits(Ud.cpu().numpy(), U) and _same_bits(Vd.cpu().numpy(), Vt)
    assert _same_bits(M.singular_values(), s) and _same_bits(Md.singular_values().cpu().numpy(), s)
    for mat in (M, Md):
        assert mat.norm2() == s[0] and mat.cond2() == s[0] / s[-1]
        assert mat.numerical_rank() == cs.RANK and mat.numerical_rank(rcond=0.9) == 1
    P = M.pinv_array()
    Pd = Md.pinv_array()
    assert P.shape == (60, 40) and _same_bits(Pd.cpu().numpy(), P) and _same_bits(P, dense.pinv(A, handle=dev.h))
    assert max(cs.pinv_residuals(A, P)) < 1e-11
    # min_norm=True serves any shape and rank; the default keeps every current behaviour
    xm, rm = M.least_squares_array(b, residuals=True, min_norm=True)
    assert _same_bits(xm, X) and _same_bits(rm, resid)
    assert np.allclose(M.least_squares_array(b[:, 0], min_norm=True), X[:, 0], rtol=0, atol=1e-13)
    xd, rd = Md.least_squares_array(_t(b), residuals=True, min_norm=True)
    assert torch.is_tensor(xd) and _same_bits(xd.cpu().numpy(), X) and np.allclose(rd.cpu().numpy(), resid, rtol=1e-9, atol=0)
    with pytest.raises(ValueError):
        M.least_squares_array(b)                                  # wide, min_norm=False: as before
    At, bt, xt = cs.rank_product(60, 40)
    Mt = Matrix.from_numpy(At)
    assert cs.rel_err(Mt.least_squares_array(bt, min_norm=True), xt) < 1e-12
    zc = Matrix([[1.0, 0.0], [1.0, 0.0], [1.0, 0.0]])                   # a zero column: r_22 == 0 exactly
    assert isinstance(zc.least_squares_array([1.0, 2.0, 6.0]), Matrix.NoSolution)      # through QR: as before
    assert np.allclose(zc.least_squares_array([1.0, 2.0, 6.0], min_norm=True), [3.0, 0.0], rtol=0, atol=1e-14)
    assert cs.rel_err(Matrix.from_dlpack(_t(At)).least_squares_array(_t(bt), min_norm=True).cpu().numpy(), xt) < 1e-12
    Zm = Matrix.from_numpy(np.zeros((6, 6)))
    assert Zm.cond2() == float("inf") and Zm.norm2() == 0.0 and Zm.numerical_rank() == 0
    assert np.array_equal(Zm.least_squares_array(np.ones(6), min_norm=True), np.zeros(6))
    small = Matrix([[1, 0], [0, 1], [1, 1]])
    assert small.rank() == 2 and small.numerical_rank() == 2
    assert np.allclose(small.least_squares_array([1, 1, 3], min_norm=True), [4 / 3, 4 / 3])
