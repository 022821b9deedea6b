"""The symmetric eigensolver by two-sided Jacobi on the MI355X (lsx_syevj_*), through the C ABI (host and _dev forms),
`dense`, `DeviceSolver` and `Matrix`, in both precisions.  The yardsticks are those tests/test_eig_host.py proves on the
CPU: on the diagonal plants the numpy model (tests/cpu_eig.py) and the GPU must agree bit for bit with one sweep and no
rotation, on the threshold plants exactly the pairs above the threshold are counted, and on rounded and special inputs
the GPU's three ratios stay within twice the largest value the model or LAPACK attains.  GPU results are compared with
each other bit for bit.

Orders (cpu_eig.ROUNDED): 1 -- no pair; 2 -- one pair; 3, 5 -- the phantom player; 64, 129, 130, 257 -- odd and even
across a 16-byte group boundary, padded leading dimensions; 515 -- 258 positions per round, more than the 256 threads
of a pair's workgroup, so eig_round_kernel's loop over column pairs takes a second pass.
"""
import ctypes as C

import numpy as np
import pytest

import cpu_eig as ce
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
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _t(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sync():
    import torch

    torch.cuda.synchronize()


def _eig(dev, A, compute_v=True):
    """(w, V, info, sweeps, rotations) as numpy through DeviceSolver.syevj_."""
    w, V, info = dev.syevj_(_t(A), compute_v=compute_v)
    sw, rot = dev.h.get_option("syevj_sweeps"), dev.h.get_option("syevj_rotations")
    return w.cpu().numpy(), (None if V is None else V.cpu().numpy()), info, sw, rot


def _all_entry_points_agree(dev, A, w, V):
    """The C ABI host form (through dense), the values-only forms and a second call give the bits of (w, V)."""
    from linalg_solver_amd import dense

    dtype = A.dtype.type
    w0, V0, _, _, _ = _eig(dev, A, compute_v=False)
    assert V0 is None and _same_bits(w0, w), "jobz = 0 gives the bits of jobz = 1"
    w2, V2, _, _, _ = _eig(dev, A)
    assert _same_bits(w2, w) and _same_bits(V2, V), "two calls give the same bits"
    wh, Vh, ih = dense.eigh(A, dtype=dtype, handle=dev.h)
    assert ih == 0 and _same_bits(wh, w) and _same_bits(Vh, V), "host-buffer form"
    assert _same_bits(dense.eigvalsh(A, dtype=dtype, handle=dev.h), w)


# ------------------------------------------------------------------ exact plants
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", ce.PLANT_N)
def test_diagonal_plant_exact(dev, n, dtype):
    A, w0, V0 = ce.plant_diagonal(n, dtype)
    w, V, info, sweeps, rot = _eig(dev, A)
    assert (info, sweeps, rot) == (0, 1, 0)
    assert _same_bits(w, w0) and _same_bits(V, V0), "the sorted diagonal and the permutation matrix, entries exactly 0 and 1"
    m = ce.syevj(A)
    assert _same_bits(w, m["w"]) and _same_bits(V, m["V"])
    _all_entry_points_agree(dev, A, w, V)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", ce.PLANT_N)
def test_planted_thresholds_count_exactly_the_pairs_above(dev, n, dtype):
    A, above = ce.plant_threshold(n, dtype)
    default = dev.h.get_option("syevj_max_sweeps")
    try:
        dev.h.set_option("syevj_max_sweeps", 1)
        for uv in (True, False):
            w, V, info, sweeps, rot = _eig(dev, A, compute_v=uv)
            assert (info, sweeps, rot) == (1, 1, len(above)), "2 thr rotates, thr / 2 does not"
    finally:
        dev.h.set_option("syevj_max_sweeps", default)
    w, V, info, sweeps, rot = _eig(dev, A)
    assert (info, sweeps, rot) == (0, 2, len(above))


# ------------------------------------------------------------------ rounded and special inputs
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", ce.ROUNDED)
def test_rounded_ratios_within_pooled_bounds(dev, n, dtype):
    name = np.dtype(dtype).name
    A = ce.rounded(n, dtype)
    w, V, info, sweeps, rot = _eig(dev, A)
    assert info == 0 and 1 <= sweeps <= ce.MAX_SWEEPS // 2
    assert w.shape == (n,) and w.dtype == np.float64 and V.shape == (n, n) and np.all(np.diff(w) >= 0)
    got = ce.eig_ratios(A, w, V)
    bound = ce.pooled_bounds(name)
    print(name, n, "sweeps", sweeps, "rotations", rot, "gpu", got, "model", ce.model_ratios(n, name), "lapack",
          ce.lapack_ratios(n, name), "bound", bound)
    for g, b in zip(got, bound):
        assert g <= b
    _all_entry_points_agree(dev, A, w, V)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ce.SPECIAL)
def test_special_inputs_within_their_bounds(dev, case, dtype):
    name = np.dtype(dtype).name
    A = ce.special(case, dtype)
    w, V, info, sweeps, rot = _eig(dev, A)
    assert info == 0 and 1 <= sweeps <= ce.MAX_SWEEPS // 2
    got = ce.eig_ratios(A, w, V)
    bound = ce.special_bounds(case, name)
    print(name, case, "sweeps", sweeps, "model sweeps", ce.special_model(case, name)["sweeps"], "gpu", got, "model",
          ce.special_model_ratios(case, name), "lapack", ce.special_lapack_ratios(case, name), "bound", bound)
    for g, b in zip(got, bound):
        assert g <= b
    w0 = _eig(dev, A, compute_v=False)[0]
    assert _same_bits(w0, w)


# ------------------------------------------------------------------ outcomes
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("n", [5, 130])
def test_nan_and_infinity_give_nan_values(dev, n, bad, dtype):
    from linalg_solver_amd import dense

    A = ce.rounded(n, dtype).copy()
    A[n // 3, n // 2] = bad                       # upper triangle only: the matrix is what that triangle says
    for uv in (True, False):
        w, _, info, sweeps, rot = _eig(dev, A, compute_v=uv)
        assert np.isnan(w).all() and (info, sweeps, rot) == (0, 0, 0)
    wh, _, ih = dense.eigh(A, dtype=dtype, handle=dev.h)
    assert np.isnan(wh).all() and ih == 0
    B = ce.rounded(n, dtype).copy()
    B[n // 2, n // 3] = bad                       # strictly lower: never read
    w, V, info, _, _ = _eig(dev, B)
    w1, V1, _, _, _ = _eig(dev, ce.rounded(n, dtype))
    assert info == 0 and _same_bits(w, w1) and _same_bits(V, V1)
    dev.h.check_status()


@pytest.mark.parametrize("dtype", DTYPES)
def test_sweep_cap_sets_info(dev, dtype):
    A = ce.rounded(64, dtype)
    default = dev.h.get_option("syevj_max_sweeps")
    assert default == 60
    try:
        dev.h.set_option("syevj_max_sweeps", 1)
        w, V, info, sweeps, rot = _eig(dev, A)
        assert info == 1 and sweeps == 1 and rot > 0
        assert np.isfinite(w).all() and np.all(np.diff(w) >= 0) and np.isfinite(V).all()
    finally:
        dev.h.set_option("syevj_max_sweeps", default)
    assert _eig(dev, A)[2] == 0
    lib = dev.lib
    for v in (0, 101, -1):
        assert lib.lsx_set_option(dev.h.ptr, b"syevj_max_sweeps", v) == ERR_ARG
    assert lib.lsx_set_option(dev.h.ptr, b"syevj_sweeps", 1) == ERR_ARG, "read-only"
    assert lib.lsx_set_option(dev.h.ptr, b"syevj_rotations", 1) == ERR_ARG, "read-only"
    assert dev.h.get_option("syevj_max_sweeps") == default
    dev.h.set_option("syevj_max_sweeps", 100)
    dev.h.set_option("syevj_max_sweeps", default)


@pytest.mark.parametrize("dtype", DTYPES)
def test_argument_errors_and_empty_problems(dev, dtype):
    import torch

    lib, h, sf = dev.lib, dev.h.ptr, _sfx(dtype)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    A = torch.full((8, 8), 3.0, dtype=tdt, device="cuda")
    V = torch.full((8, 8), 5.0, dtype=tdt, device="cuda")
    S = torch.full((8,), 7.0, dtype=torch.float64, device="cuda")
    a, v, s = A.data_ptr(), V.data_ptr(), S.data_ptr()
    eig, eig_host = getattr(lib, f"lsx_syevj_{sf}_dev"), getattr(lib, f"lsx_syevj_{sf}")
    info = C.c_int(5)
    pi = C.byref(info)
    assert eig(h, 1, -1, a, 8, s, v, 8, pi) == ERR_ARG, "n < 0"
    assert eig(h, 1, 4, a, 3, s, v, 8, pi) == ERR_ARG, "lda < n"
    assert eig(h, 2, 4, a, 8, s, v, 8, pi) == ERR_ARG and eig(h, -1, 4, a, 8, s, v, 8, pi) == ERR_ARG, "jobz"
    assert eig(h, 1, 4, a, 8, s, v, 3, pi) == ERR_ARG, "ldv < n with jobz = 1"
    assert eig(h, 1, 4, None, 8, s, v, 8, pi) == ERR_ARG and eig(h, 1, 4, a, 8, None, v, 8, pi) == ERR_ARG
    assert eig(h, 1, 4, a, 8, s, None, 8, pi) == ERR_ARG and eig(h, 0, 4, a, 8, None, None, 0, pi) == ERR_ARG
    Ah = np.full((4, 4), 3.0, dtype=dtype)
    wh = np.full(4, 7.0)
    Vh = np.full((4, 4), 5.0, dtype=dtype)
    ct = C.c_double if dtype == np.float64 else C.c_float
    pa, pw, pv = Ah.ctypes.data_as(C.POINTER(ct)), wh.ctypes.data_as(C.POINTER(C.c_double)), Vh.ctypes.data_as(C.POINTER(ct))
    assert eig_host(h, 1, -1, pa, 4, pw, pv, 4, pi) == ERR_ARG and eig_host(h, 1, 4, pa, 3, pw, pv, 4, pi) == ERR_ARG
    assert eig_host(h, 3, 4, pa, 4, pw, pv, 4, pi) == ERR_ARG and eig_host(h, 1, 4, pa, 4, pw, pv, 3, pi) == ERR_ARG
    assert eig_host(h, 1, 4, None, 4, pw, pv, 4, pi) == ERR_ARG and eig_host(h, 1, 4, pa, 4, None, pv, 4, pi) == ERR_ARG
    assert eig_host(h, 1, 4, pa, 4, pw, None, 4, pi) == ERR_ARG
    _sync()
    assert bool((A == 3).all()) and bool((V == 5).all()) and bool((S == 7).all())
    assert (Ah == 3).all() and (wh == 7).all() and (Vh == 5).all()
    # n == 0: LSX_OK, *info = 0, nothing touched, pointers may be NULL
    info.value = 5
    assert eig(h, 1, 0, None, 0, None, None, 0, pi) == 0 and info.value == 0
    assert eig(h, 0, 0, None, 0, None, None, 0, None) == 0
    info.value = 5
    assert eig_host(h, 1, 0, None, 0, None, None, 0, pi) == 0 and info.value == 0
    # values only: V may be NULL with any ldv, info may be NULL
    assert eig(h, 0, 8, a, 8, s, None, 0, None) == 0
    _sync()
    assert np.allclose(S.cpu().numpy(), [0.0] * 7 + [24.0], rtol=1e-6, atol=1e-5) and bool((V == 5).all())
    assert eig_host(h, 0, 4, pa, 4, pw, None, 0, None) == 0
    assert np.allclose(wh, [0.0] * 3 + [12.0], rtol=1e-6, atol=1e-5) and (Ah == 3).all(), "the host form leaves A alone"
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
@pytest.mark.parametrize("n", [5, 130, 257])
@pytest.mark.parametrize("dtype", DTYPES)
def test_views(dev, dtype, n, layout, fill):
    """A (its strictly lower triangle NaN), w and V as views (odd: one element off a 16-byte boundary with an odd leading
    dimension; padded: aligned with two elements of padding) inside NaN- or canary-filled buffers: the bits of the
    aligned clean call, nothing outside w and V written."""
    lib, h, sf = dev.lib, dev.h.ptr, _sfx(dtype)
    A = ce.rounded(n, dtype)
    off = 1 if layout == "odd" else 0
    pad = (lambda c: 3 if (c + 3) % 2 else 4) if layout == "odd" else (lambda c: 2)
    w0, V0, info0, sw0, rot0 = _eig(dev, A)
    Al = A.copy()
    Al[np.tril_indices(n, -1)] = np.nan
    for jobz in (1, 0):
        vA, vV = View(n, n, pad(n), off, dtype, fill, Al), View(n, n, pad(n), off, dtype, fill)
        vw = View(1, n, 0, off, np.float64, fill)
        a_before = _bits(vA.numpy()).copy()
        info = C.c_int(7)
        assert getattr(lib, f"lsx_syevj_{sf}_dev")(h, jobz, n, vA.t.data_ptr(), vA.ld, vw.t.data_ptr(),
                                                  vV.t.data_ptr() if jobz else None, vV.ld, C.byref(info)) == 0
        assert info.value == info0 == 0
        assert (dev.h.get_option("syevj_sweeps"), dev.h.get_option("syevj_rotations")) == (sw0, rot0)
        assert _same_bits(vw.numpy()[0], w0)
        assert vA.untouched() and vw.untouched() and vV.untouched()
        if jobz:
            assert _same_bits(vV.numpy(), V0)
        else:
            fill_bits = _bits(np.array([fill], dtype=dtype))[0]
            assert (_bits(vV.numpy()) == fill_bits).all(), "jobz = 0 writes no vector"
        assert np.array_equal(_bits(vA.numpy()), a_before), "the kernels only read the upper triangle"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [5, 130, 257])
def test_power_of_two_scaling_is_an_exact_symmetry(dev, n, dtype):
    A = ce.rounded(n, dtype)
    w0, V0, info0, sw0, rot0 = _eig(dev, A)
    for d in (20, -20):
        w, V, info, sw, rot = _eig(dev, np.ldexp(A, d))
        assert _same_bits(V, V0) and _same_bits(w, np.ldexp(w0, d))
        assert (info, sw, rot) == (info0, sw0, rot0)


def test_one_handle_across_lu_cholesky_qr_svd_and_the_eigensolver(dev):
    """Work-space ownership: the earlier families' results have the same bits before and after eigensolver calls."""
    import cpu_chol as cc

    _, Aq, _ = cq.planted(300, 129)
    _, bq, _ = cq.planted_rhs(300, 129, 7)
    _, S = cc.planted(257)
    G = cq.uniform(384, 384, 3)
    R = cs.rounded(130, 257, np.float64)

    def families():
        ta, tb = _t(Aq), _t(bq)
        dev.gels_(ta, tb)
        tc = _t(S)
        dev.potrf_(tc)
        lu = _t(G)
        ipiv, _ = dev.getrf_(lu)
        X = _t(G.copy())
        dev.getrs_(lu, ipiv, X)
        U, s, Vt, _ = dev.gesvdj_(_t(R))
        _sync()
        return [t.cpu().numpy() for t in (ta, tb, tc, lu, X, U, s, Vt)]

    before = families()
    first = _eig(dev, ce.rounded(257, np.float64))
    _eig(dev, ce.rounded(130, np.float32), compute_v=False)
    after = families()
    for x, y in zip(before, after):
        assert _same_bits(x, y)
    second = _eig(dev, ce.rounded(257, np.float64))
    assert _same_bits(first[0], second[0]) and _same_bits(first[1], second[1])
    dev.h.check_status()


# ------------------------------------------------------------------ the Python layers
def test_host_layers(dev):
    """dense, DeviceSolver and Matrix, host route and device-tensor route."""
    import torch

    from linalg_solver_amd import Matrix, dense

    A = ce.special("pm_pairs")
    w, V, info = dense.eigh(A, handle=dev.h)
    assert info == 0 and w.dtype == np.float64 and np.allclose((V * w) @ V.T, A, rtol=0, atol=1e-11)
    assert np.allclose(w, np.sort(ce.special_values("pm_pairs")), rtol=0, atol=1e-11)
    w1, V1, info1 = dense.eigh(A, eigvals_only=True, handle=dev.h)
    assert V1 is None and info1 == 0 and _same_bits(w1, w) and _same_bits(dense.eigvalsh(A, handle=dev.h), w)
    w32, V32, _ = dense.eigh(A, dtype=np.float32, handle=dev.h)
    assert w32.dtype == np.float64 and V32.dtype == np.float32 and np.allclose(w32, w, rtol=0, atol=5e-3)
    with pytest.raises(ValueError):
        dense.eigh(np.zeros((3, 4)), handle=dev.h)
    we, Ve, ie = dense.eigh(np.zeros((0, 0)), handle=dev.h)
    assert we.shape == (0,) and Ve.shape == (0, 0) and ie == 0

    wd, Vd, infod = dev.syevj_(_t(A))
    assert torch.is_tensor(wd) and wd.dtype == torch.float64 and infod == 0
    assert _same_bits(wd.cpu().numpy(), w) and _same_bits(Vd.cpu().numpy(), V)
    wd0, Vd0, _ = dev.syevj_(_t(A), compute_v=False)
    assert Vd0 is None and _same_bits(wd0.cpu().numpy(), w)
    with pytest.raises(ValueError):
        dev.syevj_(_t(np.zeros((3, 4))))

    M = Matrix.from_numpy(A)
    Md = Matrix.from_dlpack(_t(A))
    wm, Vm = M.eigh_array()
    wt, Vt = Md.eigh_array()
    assert _same_bits(wm, w) and _same_bits(Vm, V)
    assert torch.is_tensor(wt) and torch.is_tensor(Vt) and _same_bits(wt.cpu().numpy(), w) and _same_bits(Vt.cpu().numpy(), V)
    assert _same_bits(M.eigvalsh(), w) and torch.is_tensor(Md.eigvalsh()) and _same_bits(Md.eigvalsh().cpu().numpy(), w)
    # symmetry is the caller's assertion: only the upper triangle is used
    L = A.copy()
    L[np.tril_indices(len(A), -1)] = 123.0
    assert _same_bits(Matrix.from_numpy(L).eigvalsh(), w)
    for bad in (Matrix.from_numpy(np.zeros((3, 4))), Matrix.from_dlpack(_t(np.zeros((3, 4))))):
        with pytest.raises(ValueError):
            bad.eigh_array()
        with pytest.raises(ValueError):
            bad.eigvalsh()
    small = Matrix([[2, 1], [1, 2]])
    ws, Vs = small.eigh_array()
    assert np.allclose(ws, [1.0, 3.0], rtol=0, atol=1e-15) and np.allclose(np.abs(Vs), np.sqrt(0.5), rtol=0, atol=1e-15)
