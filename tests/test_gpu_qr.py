"""Householder QR and least squares on the MI355X (lsx_geqrf_* / lsx_ormqr_* / lsx_orgqr_* / lsx_gels_* /
lsx_colnrm2_*), through the C ABI, `dense`, `DeviceSolver` and `Matrix`.  The yardsticks are those
tests/test_qr_host.py proves on the CPU: on the planted inputs the numpy model (tests/cpu_qr.py), LAPACK and the GPU
must agree exactly -- every intermediate is a small integer or a power of two -- and on rounded inputs the GPU's three
LAPACK ratios stay within twice the larger of the model's and LAPACK's.  Against the model, results are compared as
numbers (the model has no fused multiply-adds, so the sign of a zero is not its to predict); GPU results are compared
with each other bit for bit.

Two kinds of planted input.  cpu_qr.planted (A = P [U; 0]) crosses the tau = 0 branch and the block edges, but its
reflectors are e_j +- e_k: every Gram sum g_c of qr_panel_step_kernel, every slab slot, every entry of V^T V and every
V^T C / C -= V W product on the MFMA tiles has ONE non-zero term, so a dropped, doubled or misplaced slot, 64-row chunk
or K-slice would pass.  cpu_qr.hadamard_plant (A = [0; H[:, :n] U], H Sylvester-Hadamard of order 4^q) has reflectors
with 4^q non-zeros and sums of 4^q terms that cancel exactly, and is exact all the same.  Its tall shape 16514 x 130
(and cpu_qr.TALL_SPARSE, 16500 rows of the first kind) is the first with qr_slab_rows(mp) = 128 > 64: 130 slabs, the
last of 2 rows, every workgroup running the kernel's 64-row chunk loop twice -- the second chunk, the barrier that
guards colv_s / colj_s between chunks, the `continue` above lo_row inside a two-chunk slab, a diagonal row in a second
chunk (columns 64 .. 127) -- and with it launch_gemm_tn_acc at K = 16386 and colnrm2_kernel over 16384 rows.
"""
import ctypes as C

import numpy as np
import pytest

import cpu_qr as cq

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


def _geqrf(dev, A):
    t = _t(A)
    tau = dev.geqrf_(t)
    _sync()
    return t.cpu().numpy(), tau.cpu().numpy()[:min(A.shape)]


def _ormqr(dev, QR, tau, Cm, trans):
    tq, tt, tc = _t(QR), _t(tau), _t(Cm)
    dev.ormqr_(tq, tt, tc, trans=trans)
    _sync()
    assert _same_bits(tq.cpu().numpy(), QR), "the factored array is read only"
    return tc.cpu().numpy()


def _gels(dev, A, B):
    ta, tb = _t(A), _t(B)
    tau, info = dev.gels_(ta, tb)
    n = A.shape[1]
    res = dev.col_norms(tb[n:]) if A.shape[0] > n else None
    _sync()
    return ta.cpu().numpy(), tau.cpu().numpy()[:n], tb.cpu().numpy(), int(info.item()), None if res is None else res.cpu().numpy()


# ------------------------------------------------------------------ planted factorisation
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n", cq.PLANTED_SHAPES)
def test_planted_factor(dev, m, n, dtype):
    """R, V and tau of the plant, through lsx_geqrf_*_dev and the host form."""
    from linalg_solver_amd import dense

    _, A, _ = cq.planted(m, n, dtype=dtype)
    QR, tau = cq.geqrf(A)
    G, gt = _geqrf(dev, A)
    assert np.array_equal(G, QR) and np.array_equal(gt, tau)
    H, ht = dense.qr_factor(A, dtype=dtype, handle=dev.h)
    assert _same_bits(H, G) and _same_bits(ht, gt), "host-buffer form"


@pytest.mark.parametrize("dtype", DTYPES)
def test_planted_wide(dev, dtype):
    A = cq.planted_wide(dtype=dtype)
    QR, tau = cq.geqrf(A)
    G, gt = _geqrf(dev, A)
    assert np.array_equal(G, QR) and np.array_equal(gt, tau)


# ------------------------------------------------------------------ planted ormqr / orgqr
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n", cq.GELS_SHAPES)
def test_planted_ormqr_orgqr(dev, m, n, dtype):
    _, A, _ = cq.planted(m, n, dtype=dtype)
    QR, tau = cq.geqrf(A)
    QtA = _ormqr(dev, QR, tau, A, True)
    assert np.array_equal(QtA[:n], np.triu(QR[:n])) and not QtA[n:].any(), "Q^T A = R exactly"
    for ncols in (1, 7, 200):
        Cm = np.random.default_rng(ncols).integers(-3, 4, (m, ncols)).astype(dtype)
        for k in (n, max(1, n - 70)):
            W = _ormqr(dev, QR, tau[:k], Cm, True)
            assert np.array_equal(W, cq.ormqr(QR, tau[:k], Cm, True))
            assert np.array_equal(_ormqr(dev, QR, tau[:k], W, False), Cm), "Q (Q^T C) = C exactly"
    tq = _t(QR)
    Q = dev.orgqr(tq, _t(tau)).cpu().numpy()
    assert np.array_equal(Q, cq.orgqr(QR, tau)) and np.all(np.isin(Q, (-1, 0, 1)))
    k = max(1, n - 70)
    assert np.array_equal(dev.orgqr(tq, _t(tau[:k])).cpu().numpy(), cq.orgqr(QR, tau[:k])), "k < n"


# ------------------------------------------------------------------ planted least squares
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nrhs", cq.GELS_NRHS)
@pytest.mark.parametrize("m,n", cq.GELS_SHAPES)
def test_planted_gels(dev, m, n, nrhs, dtype):
    from linalg_solver_amd import dense

    _, A, _ = cq.planted(m, n, dtype=dtype)
    x0, b, enorm = cq.planted_rhs(m, n, nrhs, dtype=dtype)
    QR, tau, Bo, info, res = _gels(dev, A, b)
    assert info == 0
    assert np.array_equal(Bo[:n], x0), "the solution is the planted one exactly"
    mq, mt = cq.geqrf(A)
    assert np.array_equal(QR, mq) and np.array_equal(tau, mt)
    if m > n:
        assert np.all(np.abs(res - enorm) <= np.spacing(enorm)), "one rounding of the square root"
    x, resid, info = dense.lstsq(A, b, dtype=dtype, handle=dev.h)
    assert info == 0 and np.array_equal(x, x0)
    assert np.all(np.abs(resid - enorm) <= np.spacing(enorm))


# ------------------------------------------------------------------ the dense-reflector plant, and the tall shapes
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("q,n", cq.HADAMARD_SHAPES)
def test_hadamard_factor(dev, q, n, dtype):
    """R, V and tau of the Hadamard plant, device-pointer and host-buffer form: the model, which is the closed form."""
    from linalg_solver_amd import dense

    _, A = cq.hadamard_plant(q, n, dtype=dtype)
    QR, tau = cq.hadamard_model(q, n, np.dtype(dtype).name)
    G, gt = _geqrf(dev, A)
    print(f"HADAMARD {A.shape[0]}x{n} {np.dtype(dtype).name}: entries differing {int(np.count_nonzero(G != QR))}, "
          f"tau differing {int(np.count_nonzero(gt != tau))}")
    assert np.array_equal(G, QR) and np.array_equal(gt, tau)
    want, wtau, _ = cq.hadamard_expected(q, n, dtype=dtype)
    assert np.array_equal(G, want) and np.array_equal(gt, wtau), "the closed form"
    H, ht = dense.qr_factor(A, dtype=dtype, handle=dev.h)
    assert _same_bits(H, G) and _same_bits(ht, gt), "host-buffer form"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("q,n", cq.HADAMARD_SHAPES)
def test_hadamard_ormqr_orgqr(dev, q, n, dtype):
    _, A = cq.hadamard_plant(q, n, dtype=dtype)
    m = A.shape[0]
    QR, tau = (np.array(x) for x in cq.hadamard_model(q, n, np.dtype(dtype).name))
    QtA = _ormqr(dev, QR, tau, A, True)
    assert np.array_equal(QtA[:n], np.triu(QR[:n])) and not QtA[n:].any(), "Q^T A = R exactly"
    for ncols in (1, 7, 200):
        Cm = cq.hadamard_c(m, ncols, dtype)
        for k in (n, max(1, n - 70)):
            W = _ormqr(dev, QR, tau[:k], Cm, True)
            assert np.array_equal(W, cq.ormqr(QR, tau[:k], Cm, True)), f"Q^T C, ncols {ncols}, k {k}"
            assert np.array_equal(_ormqr(dev, QR, tau[:k], W, False), Cm), "Q (Q^T C) = C exactly"
            assert np.array_equal(_ormqr(dev, QR, tau[:k], Cm, False), cq.ormqr(QR, tau[:k], Cm, False)), f"Q C, ncols {ncols}, k {k}"
    tq = _t(QR)
    Q = dev.orgqr(tq, _t(tau)).cpu().numpy()
    assert np.array_equal(Q, cq.hadamard_expected(q, n, dtype=dtype)[2]), "the closed form"
    k = max(1, n - 70)
    assert np.array_equal(dev.orgqr(tq, _t(tau[:k])).cpu().numpy(), cq.orgqr(QR, tau[:k])), "k < n"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("q,n", cq.HADAMARD_SHAPES)
def test_hadamard_gels(dev, q, n, dtype):
    from linalg_solver_amd import dense

    _, A = cq.hadamard_plant(q, n, dtype=dtype)
    x0, b, enorm = cq.hadamard_rhs(q, n, cq.HADAMARD_NRHS[(q, n)], dtype=dtype)
    QR, tau, Bo, info, res = _gels(dev, A, b)
    assert info == 0
    assert np.array_equal(Bo[:n], x0), "the solution is the planted one exactly"
    mq, mt = cq.hadamard_model(q, n, np.dtype(dtype).name)
    assert np.array_equal(QR, mq) and np.array_equal(tau, mt)
    assert np.all(np.abs(res - enorm) <= np.spacing(enorm)), "one rounding of the square root"
    x, resid, info = dense.lstsq(A, b, dtype=dtype, handle=dev.h)
    assert info == 0 and np.array_equal(x, x0)
    assert np.all(np.abs(resid - enorm) <= np.spacing(enorm))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n", cq.TALL_SPARSE)
def test_tall_sparse_plant(dev, m, n, dtype):
    """The one-non-zero plant at 16500 rows: the tau = 0 branch, the planted least-squares solution and the zero
    column's info with two chunks per slab."""
    U, A, _ = cq.planted(m, n, dtype=dtype)
    x0, b, enorm = cq.planted_rhs(m, n, 3, dtype=dtype)
    QR, tau, Bo, info, res = _gels(dev, A, b)
    mq, mt = cq.geqrf(A)
    assert np.array_equal(QR, mq) and np.array_equal(tau, mt) and (tau == 0).any() and (tau == 1).any()
    assert info == 0 and np.array_equal(Bo[:n], x0)
    assert np.all(np.abs(res - enorm) <= np.spacing(enorm))
    j = n - 2
    _, Z, _ = cq.planted_zero_column(m, n, j, dtype=dtype)
    zq, zt, _, zinfo, _ = _gels(dev, Z, b)
    mq, mt = cq.geqrf(Z)
    assert np.array_equal(zq, mq) and np.array_equal(zt, mt)
    assert zt[j] == 0 and zq[j, j] == 0 and zinfo == j + 1


# ------------------------------------------------------------------ rank-deficient, zero and NaN inputs
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("j", cq.ZERO_COLUMNS)
def test_zero_column(dev, j, dtype):
    from linalg_solver_amd import Matrix, dense

    m, n = 300, 257
    _, A, _ = cq.planted_zero_column(m, n, j, dtype=dtype)
    b = np.random.default_rng(j).integers(-3, 4, (m, 3)).astype(dtype)
    QR, tau, _, info, _ = _gels(dev, A, b)
    mq, mt = cq.geqrf(A)
    assert np.array_equal(QR, mq) and np.array_equal(tau, mt)
    assert tau[j] == 0 and QR[j, j] == 0 and info == j + 1
    x, resid, hinfo = dense.lstsq(A, b, dtype=dtype, handle=dev.h)
    assert hinfo == j + 1 and x is None and np.all(np.isinf(resid))
    if dtype == np.float64:
        assert isinstance(Matrix.from_numpy(A).least_squares_array(b), Matrix.NoSolution)


@pytest.mark.parametrize("dtype", DTYPES)
def test_all_zero_and_nan(dev, dtype):
    m, n = 300, 129
    Z = np.zeros((m, n), dtype=dtype)
    G, gt = _geqrf(dev, Z)
    assert not G.any() and not gt.any()
    _, _, _, info, _ = _gels(dev, Z, np.ones((m, 2), dtype=dtype))
    assert info == 1
    A = cq.uniform(m, n, 0, dtype)
    A[200, 40] = np.nan
    G, gt = _geqrf(dev, A)
    ref, _ = _geqrf(dev, cq.uniform(m, n, 0, dtype))
    assert np.isnan(G).any() and np.isnan(gt[40:]).any()
    assert _same_bits(G[:, :40], ref[:, :40]) and _same_bits(gt[:40], _geqrf(dev, cq.uniform(m, n, 0, dtype))[1][:40]), \
        "the columns before the NaN are factored before it is reached"
    _, _, _, info, _ = _gels(dev, A, np.ones((m, 2), dtype=dtype))
    assert info > 0, "a NaN on the diagonal of R is reported"


# ------------------------------------------------------------------ rounded inputs beside LAPACK
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n", cq.ROUNDED)
def test_rounded_beside_lapack(dev, m, n, dtype):
    """U(-1, 1) inputs: each of the GPU's three ratios (||A - QR||_1 / (m u ||A||_1), ||I - Q^T Q||_1 / (m u), the
    least-squares ratio) is at most twice the larger of the model's and LAPACK's for the same input.  The margin of 2
    covers the order of summation inside the MFMA products and the fused multiply-adds.  The values are printed.
    Measured on an MI355X (GPU | model | LAPACK, the first two ratios; the third is below 0.0004 everywhere):
      129 x 129   fp64 0.094 | 0.080 | 0.057 and 1.62 | 1.43 | 0.65    fp32 0.081 | 0.071 | 0.055 and 1.33 | 0.97 | 0.63
      300 x 129   fp64 0.039 | 0.034 | 0.025 and 0.40 | 0.30 | 0.17    fp32 0.035 | 0.030 | 0.023 and 0.36 | 0.29 | 0.16
      600 x 384   fp64 0.028 | 0.022 | 0.014 and 0.40 | 0.30 | 0.18    fp32 0.029 | 0.020 | 0.013 and 0.46 | 0.29 | 0.17
      1000 x 257  fp64 0.014 | 0.010 | 0.008 and 0.14 | 0.09 | 0.06    fp32 0.014 | 0.009 | 0.008 and 0.12 | 0.08 | 0.05
    The GPU is 1.1 to 1.6 times the model: inside the margin."""
    name = np.dtype(dtype).name
    A, b = cq.rounded_case(m, n, dtype)
    QR, tau, Bo, info, _ = _gels(dev, A, b)
    assert info == 0
    Q = dev.orgqr(_t(QR), _t(tau)).cpu().numpy()
    r1, r2 = cq.qr_ratios(A, Q, np.triu(QR[:n]))
    r3 = cq.ls_ratio(A, b, Bo[:n])
    mod, lap = cq.model_ratios(m, n, name), cq.lapack_ratios(m, n, name)
    print(f"{m}x{n} {name}: GPU {r1:.4f} {r2:.4f} {r3:.4f} | model {mod[0]:.4f} {mod[1]:.4f} {mod[2]:.4f} | "
          f"LAPACK {lap[0]:.4f} {lap[1]:.4f} {lap[2]:.4f}")
    for got, a, c in zip((r1, r2, r3), mod, lap):
        assert got <= 2.0 * max(a, c)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n", cq.ROUNDED_TALL)
def test_rounded_tall_beside_lapack(dev, m, n, dtype):
    """The rule of test_rounded_beside_lapack at the tall shape (two chunks per slab, K = 16386 in the TN products,
    16384 rows under colnrm2): each GPU ratio at most twice the larger of the model's and LAPACK's.  The fp32 ratios
    are evaluated in fp64, not np.longdouble (cpu_qr.tall_wide); the fp64 case spends its seconds in np.longdouble
    products on the host.  The values are printed.

    Measured on an MI355X (GPU | model | LAPACK):
                ||A - QR||_1 ratio            ||I - Q^T Q||_1 ratio         least-squares ratio
      fp64   0.00026 | 0.00032 | 0.00034   0.00119 | 0.00557 | 0.00085   3.70e-8 | 3.83e-8 | 3.25e-8
      fp32   0.00026 | 0.00023 | 0.00033   0.00108 | 0.00076 | 0.00094   3.35e-8 | 2.29e-8 | 3.24e-8
    When it was first run this test failed: 0.00050, 0.00365, 1.31e-7 in fp64 (the third 3.4 times the model's) and
    0.00051, 0.00372, 1.52e-7 in fp32 (4.0 and 4.7 times LAPACK's).  The cause, read in kernels_gemm.hip and
    reproduced on the CPU: launch_gemm_tn_acc gives every tile of C to one workgroup that walks all of K in one MFMA
    accumulator of the working precision, so G = V^T V and W = V^T C were single running sums of 16386 terms (the
    numpy model with those two products summed row after row gives 0.00049, 0.00370, 1.53e-7 in fp32 and 1.28e-7 in
    fp64: the GPU's figures).  api.hip now cuts the depth of these two products into 1024-row pieces above 4096 rows
    and adds the pieces in fp64 (qr_vt_times); the same emulation predicted 0.00025, 0.00099, 3.3e-8 for that."""
    name, wide = np.dtype(dtype).name, cq.tall_wide(dtype)
    A, b = cq.rounded_case(m, n, dtype)
    QR, tau, Bo, info, _ = _gels(dev, A, b)
    assert info == 0
    Q = dev.orgqr(_t(QR), _t(tau)).cpu().numpy()
    r1, r2 = cq.qr_ratios(A, Q, np.triu(QR[:n]), wide)
    r3 = cq.ls_ratio(A, b, Bo[:n], wide)
    mod, lap = cq.model_ratios(m, n, name, wide), cq.lapack_ratios(m, n, name, wide)
    print(f"{m}x{n} {name}: GPU {r1:.5f} {r2:.5f} {r3:.2e} | model {mod[0]:.5f} {mod[1]:.5f} {mod[2]:.2e} | "
          f"LAPACK {lap[0]:.5f} {lap[1]:.5f} {lap[2]:.2e}")
    for got, a, c in zip((r1, r2, r3), mod, lap):
        assert got <= 2.0 * max(a, c)


# ------------------------------------------------------------------ views
GUARD = 64


class View:
    """rows x cols with leading dimension ld, `off` elements behind a 16-byte boundary, inside a buffer filled with
    `fill` (NaN or a canary)."""

    def __init__(self, rows, cols, pad, off, dtype, fill, data=None):
        import torch

        ld = cols + pad
        tdt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
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
@pytest.mark.parametrize("dtype", DTYPES)
def test_views(dev, dtype, layout, fill):
    """A, tau, C, B and Q as views (odd: one element off a 16-byte boundary with an odd leading dimension; padded:
    aligned with two elements of padding) inside NaN- or canary-filled buffers: the bits of the aligned call, nothing
    outside the view written."""
    m, n, nrhs = 300, 200, 7
    _views(dev, dtype, layout, fill, cq.rounded_case(m, n, dtype)[0], cq.uniform(m, nrhs, 2, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_views_tall(dev, dtype):
    """The tall Hadamard shape (two chunks per slab) as odd views inside NaN-filled buffers."""
    q, n = cq.HADAMARD_TALL
    _views(dev, dtype, "odd", float("nan"), cq.hadamard_plant(q, n, dtype=dtype)[1], cq.hadamard_rhs(q, n, 3, dtype=dtype)[1])


def _views(dev, dtype, layout, fill, A, b):
    (m, n), nrhs = A.shape, b.shape[1]
    pad, off = (3 if (n + 3) % 2 else 4, 1) if layout == "odd" else (2, 0)
    QR0, tau0 = _geqrf(dev, A)
    vA = View(m, n, pad, off, dtype, fill, A)
    vtau = View(1, n, 0, off, dtype, fill)
    dev.geqrf_(vA.t, vtau.t[0])
    assert _same_bits(vA.numpy(), QR0) and _same_bits(vtau.numpy()[0], tau0)
    assert vA.untouched() and vtau.untouched()
    for trans in (True, False):
        C0 = _ormqr(dev, QR0, tau0, b, trans)
        vC = View(m, nrhs, pad + 1, off, dtype, fill, b)
        dev.ormqr_(vA.t, vtau.t[0], vC.t, trans=trans)
        assert _same_bits(vC.numpy(), C0) and vC.untouched() and vA.untouched()
    Q0 = dev.orgqr(_t(QR0), _t(tau0)).cpu().numpy()
    vQ = View(m, n, pad, off, dtype, fill)
    dev.orgqr(vA.t, vtau.t[0], out=vQ.t)
    assert _same_bits(vQ.numpy(), Q0) and vQ.untouched()
    _, _, B0, info0, res0 = _gels(dev, A, b)
    vA2, vB, vt2 = View(m, n, pad, off, dtype, fill, A), View(m, nrhs, pad + 1, off, dtype, fill, b), View(1, n, 0, off, dtype, fill)
    _, info = dev.gels_(vA2.t, vB.t, tau=vt2.t[0])
    res = dev.col_norms(vB.t[n:]).cpu().numpy()
    assert int(info.item()) == info0 == 0
    assert _same_bits(vB.numpy(), B0) and _same_bits(vA2.numpy(), QR0) and _same_bits(res, res0)
    assert vA2.untouched() and vB.untouched() and vt2.untouched()


# ------------------------------------------------------------------ further cases
@pytest.mark.parametrize("dtype", DTYPES)
def test_two_calls_give_identical_bits(dev, dtype):
    A, b = cq.rounded_case(600, 384, dtype)
    first, second = _gels(dev, A, b), _gels(dev, A, b)
    for x, y in zip(first[:3], second[:3]):
        assert _same_bits(x, y)
    assert _same_bits(first[4], second[4])


@pytest.mark.parametrize("dtype", DTYPES)
def test_argument_errors_and_empty_problems(dev, dtype):
    import torch

    lib, h, s = dev.lib, dev.h.ptr, _sfx(dtype)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    A = torch.full((8, 8), 3.0, dtype=tdt, device="cuda")
    B = torch.full((8, 8), 5.0, dtype=tdt, device="cuda")
    tau = torch.full((8,), 7.0, dtype=tdt, device="cuda")
    a, b_, t = A.data_ptr(), B.data_ptr(), tau.data_ptr()
    geqrf, ormqr, orgqr = (getattr(lib, f"lsx_{f}_{s}_dev") for f in ("geqrf", "ormqr", "orgqr"))
    gels, nrm = getattr(lib, f"lsx_gels_{s}_dev"), getattr(lib, f"lsx_colnrm2_{s}_dev")
    assert geqrf(h, -1, 4, a, 8, t) == ERR_ARG and geqrf(h, 4, -1, a, 8, t) == ERR_ARG
    assert geqrf(h, 4, 4, a, 3, t) == ERR_ARG and geqrf(h, 4, 4, None, 8, t) == ERR_ARG and geqrf(h, 4, 4, a, 8, None) == ERR_ARG
    assert ormqr(h, 2, 4, 4, 4, a, 8, t, b_, 8) == ERR_ARG and ormqr(h, 1, 4, 4, 5, a, 8, t, b_, 8) == ERR_ARG
    assert ormqr(h, 1, 4, 4, 4, a, 8, t, b_, 3) == ERR_ARG and ormqr(h, 1, 4, 4, 4, a, 3, t, b_, 8) == ERR_ARG
    assert ormqr(h, 1, 4, 4, 4, a, 8, t, None, 8) == ERR_ARG and ormqr(h, 1, -1, 4, 0, a, 8, t, b_, 8) == ERR_ARG
    assert orgqr(h, 4, 5, 4, a, 8, t, b_, 8) == ERR_ARG and orgqr(h, 4, 3, 4, a, 8, t, b_, 8) == ERR_ARG
    assert orgqr(h, 4, 4, 4, a, 8, t, b_, 3) == ERR_ARG and orgqr(h, 4, 4, 4, a, 8, t, None, 8) == ERR_ARG
    assert gels(h, 3, 4, 1, a, 8, t, b_, 8, None) == ERR_ARG, "m < n"
    assert gels(h, 4, 4, 2, a, 8, t, b_, 1, None) == ERR_ARG and gels(h, 4, 4, 2, a, 8, None, b_, 8, None) == ERR_ARG
    assert nrm(h, 4, 4, a, 3, b_) == ERR_ARG and nrm(h, 4, 4, None, 8, b_) == ERR_ARG
    for fn in (getattr(lib, f"lsx_geqrf_{s}"),):
        assert fn(h, 4, 4, None, 4, None) == ERR_ARG
    assert getattr(lib, f"lsx_gels_{s}")(h, 3, 4, 1, None, 4, None, 1, None, 1, None, None) == ERR_ARG
    # empty problems: LSX_OK, nothing touched, pointers may be NULL
    assert geqrf(h, 0, 4, None, 4, None) == 0 and geqrf(h, 4, 0, None, 0, None) == 0
    assert ormqr(h, 1, 4, 0, 4, None, 4, None, None, 0) == 0 and ormqr(h, 0, 4, 4, 0, None, 0, None, None, 4) == 0
    assert orgqr(h, 0, 0, 0, None, 0, None, None, 0) == 0
    assert gels(h, 4, 0, 2, None, 0, None, None, 2, None) == 0 and gels(h, 4, 4, 0, None, 4, None, None, 0, None) == 0
    assert gels(h, 0, 0, 0, None, 0, None, None, 0, None) == 0
    assert nrm(h, 0, 4, None, 4, None) == 0 and nrm(h, 4, 0, None, 0, None) == 0
    _sync()
    assert bool((A == 3).all()) and bool((B == 5).all()) and bool((tau == 7).all())
    # k = 0 reflectors: Q is the identity
    Q = torch.full((5, 3), 9.0, dtype=tdt, device="cuda")
    assert orgqr(h, 5, 3, 0, None, 0, None, Q.data_ptr(), 3) == 0
    assert np.array_equal(Q.cpu().numpy(), np.eye(5, 3))


def test_one_handle_across_lu_cholesky_and_qr(dev):
    """Work-space ownership: the three families in turn on one handle, twice, with the same results."""
    import torch

    import cpu_chol as cc

    _, A, _ = cq.planted(300, 129)
    x0, b, _ = cq.planted_rhs(300, 129, 7)
    U, S = cc.planted(257)
    G = cq.uniform(384, 384, 3)
    for _ in range(2):
        _, _, Bo, info, _ = _gels(dev, A, b)
        assert info == 0 and np.array_equal(Bo[:129], x0)
        t = _t(S)
        assert int(dev.potrf_(t).item()) == 0 and np.array_equal(np.triu(t.cpu().numpy()), U)
        lu = _t(G)
        ipiv, info = dev.getrf_(lu)
        X = _t(G.copy())
        dev.getrs_(lu, ipiv, X)
        assert int(info.item()) == 0 and torch.allclose(X, torch.eye(384, dtype=torch.float64, device="cuda"), atol=1e-9)
        QR, tau = _geqrf(dev, A)
        assert np.array_equal(QR, cq.geqrf(A)[0])


@pytest.mark.parametrize("kind", ["planted", "rounded"])
def test_host_layers(dev, kind):
    """dense, DeviceSolver and Matrix on one planted and one rounded case."""
    import torch

    from linalg_solver_amd import Matrix, dense

    m, n, nrhs = 300, 129, 3
    if kind == "planted":
        _, A, _ = cq.planted(m, n)
        x0, b, enorm = cq.planted_rhs(m, n, nrhs)
    else:
        A, b = cq.rounded_case(m, n, np.float64)
        x0 = np.linalg.lstsq(A, b, rcond=None)[0]
        enorm = np.linalg.norm(b - A @ x0, axis=0)
    tol = 0.0 if kind == "planted" else 1e-11
    QR, tau = dense.qr_factor(A, handle=dev.h)
    mq, mt = cq.geqrf(A)
    assert np.allclose(QR, mq, rtol=0, atol=tol * 10) and np.allclose(tau, mt, rtol=0, atol=tol * 10)
    assert np.allclose(dense.qr_multiply(QR, tau, A, trans=True, handle=dev.h)[:n], np.triu(QR[:n]), rtol=0, atol=tol * 10)
    assert np.allclose(dense.qr_multiply(QR, tau, dense.qr_multiply(QR, tau, b[:, 0], handle=dev.h), trans=False, handle=dev.h),
                       b[:, 0], rtol=0, atol=tol * 10)
    Q, R = dense.qr(A, handle=dev.h)
    assert Q.shape == (m, n) and R.shape == (n, n) and np.allclose(Q @ R, A, rtol=0, atol=tol * 10)
    assert np.allclose(Q.T @ Q, np.eye(n), rtol=0, atol=tol * 10)
    x, resid, info = dense.lstsq(A, b, handle=dev.h)
    assert info == 0 and np.allclose(x, x0, rtol=0, atol=tol) and np.allclose(resid, enorm, rtol=1e-12, atol=0)
    xv, rv, info = dense.lstsq(A, b[:, 0], handle=dev.h)
    assert info == 0 and xv.shape == (n,) and np.array_equal(xv, x[:, 0]) and rv == resid[0]
    M = Matrix.from_numpy(A)
    xm, rm = M.least_squares_array(b, residuals=True)
    assert np.array_equal(xm, x) and np.array_equal(rm, resid)
    assert np.array_equal(M.least_squares_array(b[:, 0]), x[:, 0])
    Qm, Rm = M.qr_array()
    assert np.array_equal(Qm, Q) and np.array_equal(Rm, R)
    with pytest.raises(ValueError):
        Matrix.from_numpy(A.T.copy()).least_squares_array(np.zeros(n))
    with pytest.raises(ValueError):
        Matrix.from_numpy(A.T.copy()).qr_array()
    Md = Matrix.from_dlpack(_t(A))
    xd, rd = Md.least_squares_array(_t(b), residuals=True)
    assert torch.is_tensor(xd) and np.array_equal(xd.cpu().numpy(), x) and np.array_equal(rd.cpu().numpy(), resid)
    Qd, Rd = Md.qr_array()
    assert np.array_equal(Qd.cpu().numpy(), Q) and np.array_equal(Rd.cpu().numpy(), R)
    # the row reduction keeps its answer for an inconsistent system
    if kind == "planted":
        small = Matrix([[1, 0], [0, 1], [1, 1]])
        assert isinstance(small.find_preimage_of([1, 1, 3]), Matrix.NoSolution)
        assert np.allclose(small.least_squares_array([1, 1, 3]), [4 / 3, 4 / 3])
