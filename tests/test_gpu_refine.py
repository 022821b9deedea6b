"""Refined solves with forward and backward error bounds (lsx_gerfs_* / lsx_gesvr_*) on the MI355X, through
`dense`, `DeviceSolver`, `Matrix` and the C ABI, against yardsticks that do not share code with the library
(tests/cpu_refine.py: the backward error in extended precision, the exact value of what the estimator estimates,
true solutions; tests/test_refine_host.py proves that statement against LAPACK's dgesvx on the CPU).

Bounds (u = 2^-53 / 2^-24, LAPACK's lamch('E')):
  |berr - omega(x)| <= (n + 1) u (1 + omega): each computed r_i and w_i carries at most gamma_{n+1} w_i (in fp32 the
      fp64 accumulation makes it tighter; the same bound is kept);
  omega(x) <= 4 u, and for n >= 33 strictly below the unrefined solve's;
  1 <= gerfs_steps <= 5 for these inputs with n >= 33;
  ferr >= the true error max|x - xt| / max|x|;
  exact_bound(x) / 6 <= ferr <= 3 exact_bound(x): W_gpu <= W_cpu + 2 (n + 1) u w <= 3 W_cpu above; below, 2 for the
      same rounding times 3 for lacn2 being a lower bound of the norm.
"""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import cpu_cond  # noqa: E402
import cpu_refine as cr  # noqa: E402
import planted  # noqa: E402

ORDERS = (1, 2, 63, 64, 65, 127, 128, 129, 257, 300, 1025)
NRHS = (1, 3, 8, 9)
DTYPES = {"f64": np.float64, "f32": np.float32}
MAXRHS = 9


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


_ref = {}


def _reference(n, prec, trans):
    """Inputs and CPU yardsticks of one (n, precision, trans), computed once and never modified: A, B (9 columns) in
    the working precision, the true solution of every column FOR THAT (rounded) DATA, and the inverse of op(A)."""
    key = (n, prec, trans)
    if key not in _ref:
        dt = DTYPES[prec]
        A, B, _ = cr.scaled_system(n, 100 + n, MAXRHS)
        A, B = A.astype(dt), B.astype(dt)
        A64 = A.astype(np.float64)
        truth = []
        for j in range(MAXRHS):
            bj = B[:, j].astype(np.float64)
            truth.append(cr.fraction_solve(cr.op(A64, trans), bj) if n <= 2 else cr.longdouble_solve(A64, bj, trans))
        inv = np.linalg.inv(cr.op(A64, trans))
        for a in (A, B, inv):
            a.setflags(write=False)
        _ref[key] = (A, B, truth, inv)
    return _ref[key]


_fac = {}


def _factors(n, prec):
    """The library's own factors of the case's matrix (one factorisation per matrix and precision)."""
    from linalg_solver_amd import dense

    if (n, prec) not in _fac:
        A = _reference(n, prec, False)[0]
        LU, ipiv, info = dense.lu_factor(A, dtype=DTYPES[prec])
        assert info == 0
        _fac[(n, prec)] = (LU, ipiv)
    return _fac[(n, prec)]


def _check_columns(tag, n, prec, trans, X0, X, ferr, berr, steps):
    A, B, truth, inv = _reference(n, prec, trans)
    u = cr.unit(DTYPES[prec])
    for j in range(X.shape[1]):
        om0 = cr.omega(A, X0[:, j], B[:, j], trans)
        om = cr.omega(A, X[:, j], B[:, j], trans)
        err = cr.true_error(X[:, j], truth[j])
        exact = cr.exact_bound(A, X[:, j], B[:, j], trans, inv=inv)
        print(f"{tag} col {j}: berr/u {berr[j] / u:.3f} omega/u {om / u:.3f} (unrefined {om0 / u:.1f}) |diff|/u "
              f"{abs(berr[j] - om) / u:.3f} allowed {(n + 1) * (1 + om):.1f}  ferr {ferr[j]:.3e} exact bound {exact:.3e} "
              f"ratio {ferr[j] / exact:.3f} true error {err:.3e}  steps(max) {steps}")
        assert abs(berr[j] - om) <= (n + 1) * u * (1 + om)
        assert om <= 4 * u
        if n >= 33:
            assert om < om0
        assert ferr[j] >= err
        assert exact / 6 <= ferr[j] <= 3 * exact
    if n >= 33:
        assert 1 <= steps <= 5


@pytest.mark.parametrize("prec", ("f64", "f32"))
@pytest.mark.parametrize("trans", (False, True), ids=("N", "T"))
@pytest.mark.parametrize("nrhs", NRHS)
@pytest.mark.parametrize("n", ORDERS)
def test_refined_solve_agrees_with_the_yardsticks(la, n, nrhs, trans, prec):
    from linalg_solver_amd import dense

    A, B, _, _ = _reference(n, prec, trans)
    LU, ipiv = _factors(n, prec)
    Bk = np.ascontiguousarray(B[:, :nrhs])
    X0 = dense.lu_solve(LU, ipiv, Bk, trans=trans)
    X, ferr, berr = dense.lu_refine(A, LU, ipiv, Bk, X0, trans=trans)
    h = la.default_handle()
    steps, solves = h.get_option("gerfs_steps"), h.get_option("gerfs_solves")
    assert X.dtype == DTYPES[prec] and X.shape == (n, nrhs) and ferr.shape == berr.shape == (nrhs,)
    assert (4 if n > 1 else 1) * nrhs <= solves <= 11 * nrhs
    _check_columns(f"gerfs {prec} n={n} nrhs={nrhs} {'T' if trans else 'N'}", n, prec, trans, X0, X, ferr, berr, steps)


@pytest.mark.parametrize("prec", ("f64", "f32"))
@pytest.mark.parametrize("trans", (False, True), ids=("N", "T"))
@pytest.mark.parametrize("n", (129, 300))
def test_device_solver_and_one_call_driver(la, dev, n, trans, prec):
    """DeviceSolver.gerfs_ on tensors with lda > n, and dense.solve_bounded (lsx_gesvr_*), held to the same bounds."""
    import torch

    from linalg_solver_amd import dense

    A, B, _, _ = _reference(n, prec, trans)
    nrhs = MAXRHS
    tA = torch.from_numpy(np.array(A)).cuda()
    LUp = torch.zeros(n, n + 8, dtype=tA.dtype, device="cuda")
    LU = LUp[:, :n]
    LU.copy_(tA)
    ipiv, info = dev.getrf_(LU)
    assert int(info.item()) == 0
    tB = torch.from_numpy(np.array(B)).cuda()
    X = tB.clone()
    dev.getrs_(LU, ipiv, X, trans=trans)
    X0 = X.cpu().numpy()
    ferr, berr = dev.gerfs_(tA, LU, ipiv, tB, X, trans=trans)
    steps = dev.h.get_option("gerfs_steps")
    _check_columns(f"DeviceSolver {prec} n={n} {'T' if trans else 'N'}", n, prec, trans, X0, X.cpu().numpy(), ferr, berr,
                   steps)
    Xb, ferr_b, berr_b, binfo = dense.solve_bounded(A, B, trans=trans, dtype=DTYPES[prec])
    steps_b = la.default_handle().get_option("gerfs_steps")
    assert binfo == 0
    LUh, ipivh = _factors(n, prec)
    _check_columns(f"solve_bounded {prec} n={n} {'T' if trans else 'N'}", n, prec, trans,
                   dense.lu_solve(LUh, ipivh, np.array(B), trans=trans), Xb, ferr_b, berr_b, steps_b)
    # a vector is the one-column matrix (the unrefined solve inside takes another kernel for 9 columns than for 1, so
    # the 9-column call above is not the comparison)
    xv, fv, bv, vinfo = dense.solve_bounded(A, B[:, 0], trans=trans, dtype=DTYPES[prec])
    x1, f1, b1, info1 = dense.solve_bounded(A, np.array(B[:, :1]), trans=trans, dtype=DTYPES[prec])
    assert vinfo == 0 and info1 == 0 and xv.shape == (n,) and isinstance(fv, float) and isinstance(bv, float)
    assert xv.tobytes() == x1[:, 0].tobytes() and fv == f1[0] and bv == b1[0]


@pytest.mark.parametrize("dtype", (np.float64, np.float32))
@pytest.mark.parametrize("trans", (False, True), ids=("N", "T"))
@pytest.mark.parametrize("n", (5, 130, 300))
def test_an_exact_solution_is_left_alone(la, n, trans, dtype):
    """Planted system: A, its factors, x (small integers) and b = op(A) x are exactly representable, so r = 0 in any
    order of the sums: berr == 0, no step, X unchanged bit for bit."""
    from linalg_solver_amd import dense

    A, L, U, perm = planted.planted(n, 7)
    rng = np.random.default_rng(n)
    X = rng.integers(-3, 4, (n, 3)).astype(np.float64)
    B = cr.op(A, trans) @ X
    assert np.all(B == np.round(B * 4) / 4) and np.max(np.abs(B)) < 2.0 ** 20
    LU, ipiv = planted.planted_lu(L, U).astype(dtype), planted.ipiv_of_perm(perm).astype(np.int32)
    Xr, ferr, berr = dense.lu_refine(A.astype(dtype), LU, ipiv, B.astype(dtype), X.astype(dtype), trans=trans)
    assert np.array_equal(berr, np.zeros(3)) and la.default_handle().get_option("gerfs_steps") == 0
    assert Xr.dtype == dtype and Xr.tobytes() == X.astype(dtype).tobytes()
    assert np.all(ferr >= 0) and np.all(np.isfinite(ferr))


@pytest.mark.parametrize("prec", ("f64", "f32"))
@pytest.mark.parametrize("trans", (False, True), ids=("N", "T"))
@pytest.mark.parametrize("n", (65, 300))
def test_two_calls_and_column_subsets_give_the_same_bits(la, n, trans, prec):
    from linalg_solver_amd import dense

    A, B, _, _ = _reference(n, prec, trans)
    LU, ipiv = _factors(n, prec)
    X0 = dense.lu_solve(LU, ipiv, np.array(B), trans=trans)
    X1, f1, b1 = dense.lu_refine(A, LU, ipiv, B, X0, trans=trans)
    X2, f2, b2 = dense.lu_refine(A, LU, ipiv, B, X0, trans=trans)
    assert X1.tobytes() == X2.tobytes() and f1.tobytes() == f2.tobytes() and b1.tobytes() == b2.tobytes()
    for j in (0, 4, 7, 8):
        xj, fj, bj = dense.lu_refine(A, LU, ipiv, np.array(B[:, j]), np.array(X0[:, j]), trans=trans)
        assert xj.tobytes() == np.ascontiguousarray(X1[:, j]).tobytes(), f"column {j} alone differs from the group"
        assert fj == f1[j] and bj == b1[j]


def test_numerical_outcomes_are_values(la, dev):
    import torch

    from linalg_solver_amd import dense

    h = la.default_handle()
    e = np.zeros((0, 0))
    X, ferr, berr = dense.lu_refine(e, e, np.zeros(0, dtype=np.int32), np.zeros((0, 2)), np.zeros((0, 2)))
    assert X.shape == (0, 2) and np.array_equal(ferr, [0, 0]) and np.array_equal(berr, [0, 0])           # n = 0
    A, B, _, _ = _reference(64, "f64", False)
    LU, ipiv = _factors(64, "f64")
    X, ferr, berr = dense.lu_refine(A, LU, ipiv, np.zeros((64, 0)), np.zeros((64, 0)))                      # nrhs = 0
    assert X.shape == (64, 0) and ferr.shape == (0,) and berr.shape == (0,)
    xb, fb, bb, info = dense.solve_bounded(e, np.zeros((0, 1)))
    assert info == 0 and xb.shape == (0, 1) and fb[0] == 0 and bb[0] == 0
    # an exactly zero pivot: +inf bounds, X untouched
    sing = cpu_cond.matrix("u11_zero_col", 64, 1364)
    for dt in (np.float64, np.float32):
        S = sing.astype(dt)
        SLU, sp, sinfo = dense.lu_factor(S, dtype=dt)
        assert sinfo == 18
        Xin = np.arange(64 * 2, dtype=dt).reshape(64, 2)
        for trans in (False, True):
            Xs, fs, bs = dense.lu_refine(S, SLU, sp, np.ones((64, 2), dtype=dt), Xin, trans=trans)
            assert np.all(np.isposinf(fs)) and np.all(np.isposinf(bs)) and Xs.tobytes() == Xin.tobytes()
        xs, fs, bs, sinfo = dense.solve_bounded(S, np.ones((64, 2)), dtype=dt)
        assert xs is None and sinfo == 18 and np.all(np.isposinf(fs)) and np.all(np.isposinf(bs))
    tS = torch.from_numpy(sing).cuda()
    tLU = tS.clone()
    tp, _ = dev.getrf_(tLU)
    tX = torch.ones(64, 2, dtype=torch.float64, device="cuda")
    fs, bs = dev.gerfs_(tS, tLU, tp, torch.ones(64, 2, dtype=torch.float64, device="cuda"), tX)
    assert np.all(np.isposinf(fs)) and np.all(np.isposinf(bs)) and bool((tX == 1).all())
    # a NaN in one column of B: NaN bounds for that column only, the others as without it
    for trans in (False, True):
        A, B, _, _ = _reference(129, "f64", trans)
        LU, ipiv = _factors(129, "f64")
        X0 = dense.lu_solve(LU, ipiv, np.array(B[:, :4]), trans=trans)
        Xg, fg, bg = dense.lu_refine(A, LU, ipiv, B[:, :4], X0, trans=trans)
        Bn = np.array(B[:, :4])
        Bn[5, 2] = np.nan
        Xn, fn, bn = dense.lu_refine(A, LU, ipiv, Bn, X0, trans=trans)
        assert math.isnan(fn[2]) and math.isnan(bn[2])
        assert Xn[:, 2].tobytes() == np.ascontiguousarray(X0[:, 2]).tobytes()       # no refinement step
        for j in (0, 1, 3):
            assert fn[j] == fg[j] and bn[j] == bg[j] and np.array_equal(Xn[:, j], Xg[:, j])
    assert h.get_option("gerfs_steps") >= 0


def test_gerfs_arguments(la, dev):
    import torch

    h = la.default_handle()
    lib = h.lib
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    A, piv = np.eye(4), np.arange(4, dtype=np.int32)
    B, X = np.ones((4, 2)), np.ones((4, 2))
    fe, be = np.zeros(2), np.zeros(2)
    pA, pP, pB, pX, pf, pb = (A.ctypes.data_as(dp), piv.ctypes.data_as(ip), B.ctypes.data_as(dp), X.ctypes.data_as(dp),
                              fe.ctypes.data_as(dp), be.ctypes.data_as(dp))
    ok = lambda *a: lib.lsx_gerfs_f64(h.ptr, *a)   # noqa: E731
    assert ok(2, 4, 2, pA, 4, pA, 4, pP, pB, 2, pX, 2, pf, pb) == -1 and b"bad argument" in lib.lsx_last_error()  # trans
    assert ok(-1, 4, 2, pA, 4, pA, 4, pP, pB, 2, pX, 2, pf, pb) == -1
    assert ok(0, 4, 2, pA, 3, pA, 4, pP, pB, 2, pX, 2, pf, pb) == -1       # lda < n
    assert ok(0, 4, 2, pA, 4, pA, 3, pP, pB, 2, pX, 2, pf, pb) == -1       # ldlu < n
    assert ok(0, 4, 2, pA, 4, pA, 4, pP, pB, 1, pX, 2, pf, pb) == -1       # ldb < nrhs
    assert ok(0, 4, 2, pA, 4, pA, 4, pP, pB, 2, pX, 1, pf, pb) == -1       # ldx < nrhs
    assert ok(0, 4, 2, None, 4, pA, 4, pP, pB, 2, pX, 2, pf, pb) == -1
    assert ok(0, 4, 2, pA, 4, pA, 4, pP, pB, 2, None, 2, pf, pb) == -1
    assert ok(0, 4, 2, pA, 4, pA, 4, pP, pB, 2, pX, 2, None, pb) == -1
    assert ok(0, 0, 2, None, 0, None, 0, None, None, 2, None, 2, pf, pb) == 0 and fe[0] == 0 and be[1] == 0
    assert ok(1, 4, 0, pA, 4, pA, 4, pP, None, 0, None, 0, None, None) == 0
    assert ok(0, 4, 2, pA, 4, pA, 4, pP, pB, 2, pX, 2, pf, pb) == 0 and np.array_equal(X, np.ones((4, 2)))   # the identity
    assert np.array_equal(be, [0, 0]) and np.all(fe > 0) and np.all(fe < 1e-14)
    info = C.c_int(-5)
    assert lib.lsx_gesvr_f64(h.ptr, 3, 4, 2, pA, 4, pB, 2, pX, 2, pf, pb, C.byref(info)) == -1
    assert lib.lsx_gesvr_f64(h.ptr, 0, 4, 2, pA, 2, pB, 2, pX, 2, pf, pb, C.byref(info)) == -1
    # the device-pointer form
    tA = torch.eye(4, dtype=torch.float64, device="cuda")
    tp = torch.arange(4, dtype=torch.int32, device="cuda")
    tB = torch.ones(4, 2, dtype=torch.float64, device="cuda")
    tX = tB.clone()
    d = lambda tr, lda, ldx: dev.lib.lsx_gerfs_f64_dev(dev.h.ptr, tr, 4, 2, tA.data_ptr(), lda, tA.data_ptr(), 4,   # noqa: E731
                                                       tp.data_ptr(), tB.data_ptr(), 2, tX.data_ptr(), ldx, pf, pb)
    assert d(2, 4, 2) == -1 and d(0, 3, 2) == -1 and d(0, 4, 1) == -1 and d(0, 4, 2) == 0
    assert dev.lib.lsx_gerfs_f64_dev(dev.h.ptr, 0, 4, 2, None, 4, None, 4, None, None, 2, None, 2, pf, pb) == -1


@pytest.mark.parametrize("prec", ("f64", "f32"))
@pytest.mark.parametrize("n", (200, 131))
def test_gerfs_on_views(dev, n, prec):
    """A, LU, B and X as padded, offset and misaligned views inside NaN-filled buffers (test_gpu_views.View): nothing
    outside X's view is written, A / LU / B are not written at all, and X, ferr, berr have the bits of the call on
    contiguous 16-byte aligned tensors.

    The plain residual kernel takes its 16-byte path when A's base is 16-byte aligned and lda and n are multiples of
    2 (fp64) / 4 (fp32): here n = 200 with (off, pad) = (0, 0) in both precisions and (0, 2) in fp64.  Every other
    combination takes the element-wise path: n = 131 (odd) always; (0, 2) in fp32 (lda % 4 == 2); (0, 1) and (0, 3)
    (odd lda); off = 1 (fp64: 8-byte aligned only; fp32: 4-byte), off = 2 in fp32 (8-byte aligned, not 16) and off = 3.
    The transposed residual has one (element-wise) form."""
    import torch

    from test_gpu_views import OFFS, View

    dt = DTYPES[prec]
    nrhs = MAXRHS
    A0, B0, _ = cr.scaled_system(n, 9, nrhs)
    A0, B0 = A0.astype(dt), B0.astype(dt)
    tA = torch.from_numpy(A0).cuda()
    tLU = tA.clone()
    ipiv, info = dev.getrf_(tLU)
    assert int(info.item()) == 0
    tB = torch.from_numpy(B0).cuda()
    LU0 = tLU.cpu().numpy()
    for trans in (False, True):
        X0 = tB.clone()
        dev.getrs_(tLU, ipiv, X0, trans=trans)
        Xref = X0.clone()
        fref, bref = dev.gerfs_(tA, tLU, ipiv, tB, Xref, trans=trans)
        assert dev.h.get_option("gerfs_steps") >= 1
        x0 = X0.cpu().numpy()
        for off in OFFS[np.dtype(dt).name]:
            for pad in (0, 1, 2, 3):
                vA = View(n, n, n + pad, off, dt, A0)
                vLU = View(n, n, n + (pad + 1) % 4, (off + 1) % 2, dt, LU0)
                vB = View(n, nrhs, nrhs + pad, off, dt, B0)
                vX = View(n, nrhs, nrhs + (3 - pad), off, dt, x0)
                f, b = dev.gerfs_(vA.t, vLU.t, ipiv, vB.t, vX.t, trans=trans)
                for v, w in ((vA, "A"), (vLU, "LU"), (vB, "B"), (vX, "X")):
                    v.check_padding(f"gerfs {w} off={off} pad={pad}")
                assert vA.numpy().tobytes() == A0.tobytes() and vLU.numpy().tobytes() == LU0.tobytes()
                assert vB.numpy().tobytes() == B0.tobytes()
                what = f"gerfs views {prec} n={n} trans={trans} off={off} pad={pad}"
                assert np.all(np.isfinite(vX.numpy())), what
                assert vX.numpy().tobytes() == Xref.cpu().numpy().tobytes(), what + ": X differs from the aligned call"
                assert f.tobytes() == fref.tobytes() and b.tobytes() == bref.tobytes(), what


# rcond of the parent commit (before gecon's loop became the function it now shares with gerfs), as float.hex():
# (kind, n) -> norm -> (lsx_rcond_*, lsx_gecon_* from the library's own factors)
GECON_BEFORE = {
    ("u11", 300): {"1": ("0x1.252d248d12a34p-13", "0x1.252d248d12a38p-13"),
                   "I": ("0x1.204742d04e0fap-13", "0x1.204742d04e0f5p-13")},
    ("int5", 1000): {"1": ("0x1.c11903a020485p-16", "0x1.c11903a020485p-16"),
                     "I": ("0x1.5f7585315dcf2p-16", "0x1.5f7585315dcf2p-16")},
    ("u11_shift", 129): {"1": ("0x1.f980f39da8b0ap-7", "0x1.f980fa5466f61p-7"),
                         "I": ("0x1.6083778d6e0e7p-6", "0x1.6083711885b66p-6")},
}


@pytest.mark.parametrize("kind,n", [("u11", 300), ("int5", 1000), ("u11_shift", 129)])
def test_gecon_is_bit_identical_after_the_shared_loop(la, kind, n):
    from linalg_solver_amd import dense

    case = next(c for c in cpu_cond.load_cases() if c["kind"] == kind and c["n"] == n)
    dt = cpu_cond.DTYPE[case["prec"]]
    A = cpu_cond.matrix(kind, n, case["seed"]).astype(dt)
    LU, ipiv, info = dense.lu_factor(A, dtype=dt)
    assert info == 0
    for nm, which in (("1", 1), ("I", np.inf)):
        rc = dense.rcond(A, norm=which, dtype=dt)[0]
        rc2 = dense.lu_rcond(LU, ipiv, case["anorm"][nm], norm=which)
        print(f"GECON {kind} {n} {nm} {rc.hex()} {rc2.hex()}")
        assert (rc.hex(), rc2.hex()) == GECON_BEFORE[(kind, n)][nm]


@pytest.mark.parametrize("trans", (False, True), ids=("N", "T"))
def test_matrix_solve_array_with_bounds(la, trans):
    from linalg_solver_amd import dense

    from linalg_solver_amd import gen

    # a matrix at unit scale: solve_array calls the badly scaled systems of the other tests singular by its pivot
    # ratio, with and without bounds
    n = 129
    A = gen.system(gen.U11, 5, n)[0]
    B = np.random.default_rng(5).uniform(-1, 1, (n, 3))
    M = la.Matrix.from_numpy(np.array(A))
    plain = M.solve_array(np.array(B[:, :3]), trans=trans)
    plain2 = M.solve_array(np.array(B[:, :3]), trans=trans, bounds=False)
    ref, rinfo, _ = dense.solve(A, np.array(B[:, :3]), trans=trans)
    assert rinfo == 0 and isinstance(plain, np.ndarray) and plain.tobytes() == ref.tobytes() == plain2.tobytes()
    X, ferr, berr = M.solve_array(np.array(B[:, :3]), trans=trans, bounds=True)
    LU, ipiv, info = dense.lu_factor(A)
    assert info == 0
    X0 = dense.lu_solve(LU, ipiv, np.array(B[:, :3]), trans=trans)
    Xa, fa, ba = dense.lu_refine(A, LU, ipiv, B[:, :3], X0, trans=trans)            # the ABI, step by step
    assert np.all(ba <= 4 * 2.0 ** -53) and np.all(fa > 0) and np.all(fa < 1e-9)
    assert X.tobytes() == Xa.tobytes() and ferr.tobytes() == fa.tobytes() and berr.tobytes() == ba.tobytes()
    Xb, fb, bb, binfo = dense.solve_bounded(A, np.array(B[:, :3]), trans=trans)      # the ABI, one call
    assert binfo == 0 and Xb.tobytes() == Xa.tobytes() and fb.tobytes() == fa.tobytes() and bb.tobytes() == ba.tobytes()
    # a vector is the one-column matrix (the unrefined solve gives a column other bits in a group of 3 than alone)
    xv, fv, bv = M.solve_array(np.array(B[:, 0]), trans=trans, bounds=True)
    x1, f1, b1 = M.solve_array(np.array(B[:, :1]), trans=trans, bounds=True)
    assert xv.shape == (n,) and xv.tobytes() == x1[:, 0].tobytes() and fv == f1[0] and bv == b1[0]
    assert isinstance(fv, float) and isinstance(bv, float)
    import torch

    # the same matrix as a tensor in HBM (from_dlpack): the device branch; a device getrs on contiguous tensors
    # against the host path's staged copies is the same arithmetic, so the bits are compared too
    Md = la.Matrix.from_dlpack(torch.from_numpy(np.array(A)).cuda())
    Xd, fd, bd = Md.solve_array(torch.from_numpy(np.array(B[:, :3])).cuda(), trans=trans, bounds=True)
    assert Xd.is_cuda and Xd.shape == (n, 3) and fd.shape == bd.shape == (3,)
    print(f"from_dlpack bounds trans={trans}: same bits as the host path: X {Xd.cpu().numpy().tobytes() == Xa.tobytes()} "
          f"ferr {fd.tobytes() == fa.tobytes()} berr {bd.tobytes() == ba.tobytes()}")
    for j in range(3):      # each ferr bounds its own column's error relative to its own max |x|
        xd, xa = Xd.cpu().numpy()[:, j], Xa[:, j]
        assert np.max(np.abs(xd - xa)) <= fd[j] * np.max(np.abs(xd)) + fa[j] * np.max(np.abs(xa))
    assert np.all(bd <= 4 * 2.0 ** -53) and np.all(fd > 0) and np.all(np.isfinite(fd))
    xdv, fdv, bdv = Md.solve_array(np.array(B[:, 0]), trans=trans, bounds=True)       # a host vector against HBM data
    assert xdv.shape == (n,) and isinstance(fdv, float) and isinstance(bdv, float) and bdv <= 4 * 2.0 ** -53
    for S in (cpu_cond.matrix("u11_zero_col", 64, 1364), np.array(_reference(129, "f64", trans)[0])):
        for sing in (la.Matrix.from_numpy(S), la.Matrix.from_dlpack(torch.from_numpy(S).cuda())):
            # an exactly zero pivot; a pivot ratio below n eps
            assert isinstance(sing.solve_array(np.ones(len(S)), trans=trans, bounds=True), la.Matrix.NoSolution)
            assert isinstance(sing.solve_array(np.ones(len(S)), trans=trans), la.Matrix.NoSolution)


@pytest.mark.parametrize("prec", ("f64", "f32"))
@pytest.mark.parametrize("trans", (False, True), ids=("N", "T"))
@pytest.mark.parametrize("nrhs", (1, 2, 3, 4, 8))
def test_residual_and_bound_kernel_directly(dev, nrhs, trans, prec):
    """lsx_diag_resid_bound_*_dev, the kernel alone, against cpu_refine.resid_bound: n = 600 (two staged chunks of
    x, three row chunks of the transposed form; 16-byte path: aligned, lda = n = 600 a multiple of 4) and n = 601 with
    lda = 603 (element-wise path), NR = 1, 2, 4 (3 columns padded), 4 and 8.

    Bound: both sides add n products in fp64 in different orders, so |r - r_cpu| <= 2 gamma_n w with gamma_n = n 2^-53
    (w is the sum of the absolute values of all terms), plus one rounding of the result to the working precision,
    u |r|; the same for w against itself.  Two calls and the two paths on the same data give identical bits."""
    import torch

    dt = DTYPES[prec]
    tdt = torch.float64 if prec == "f64" else torch.float32
    fn = getattr(dev.lib, f"lsx_diag_resid_bound_{prec}_dev")
    u = cr.unit(dt)
    for n, lda in ((600, 600), (601, 603)):
        A, B, XT = cr.scaled_system(n, 31, 8)
        A, B = A.astype(dt), np.ascontiguousarray(B[:, :nrhs]).astype(dt)
        X = (XT[:, :nrhs] * (1 + 1e-3)).astype(dt)              # not the solution: r is not tiny against w
        tA = torch.zeros(n, lda, dtype=tdt, device="cuda")
        tA[:, :n] = torch.from_numpy(A).cuda()
        tB, tX = torch.from_numpy(B).cuda(), torch.from_numpy(np.ascontiguousarray(X)).cuda()

        def run(a, ld):
            R = torch.full((n, nrhs), float("nan"), dtype=tdt, device="cuda")
            W = torch.full((n, nrhs), float("nan"), dtype=tdt, device="cuda")
            assert fn(dev.h.ptr, int(trans), n, nrhs, a.data_ptr(), ld, tB.data_ptr(), nrhs, tX.data_ptr(), nrhs,
                      R.data_ptr(), W.data_ptr(), nrhs) == 0
            dev.h.synchronize()
            return R.cpu().numpy(), W.cpu().numpy()
        R, W = run(tA, lda)
        R2, W2 = run(tA, lda)
        assert R.tobytes() == R2.tobytes() and W.tobytes() == W2.tobytes()
        if lda == n:        # the same data one element behind a 16-byte boundary: the element-wise path, same bits
            buf = torch.zeros(n * n + 8, dtype=tdt, device="cuda")
            shifted = buf[1:1 + n * n].view(n, n)
            shifted.copy_(tA)
            assert shifted.data_ptr() % 16 != 0 and tA.data_ptr() % 16 == 0
            R3, W3 = run(shifted, n)
            assert R.tobytes() == R3.tobytes() and W.tobytes() == W3.tobytes()
        worst = 0.0
        for j in range(nrhs):
            r, w = cr.resid_bound(A, X[:, j], B[:, j], trans)
            r, w, gr, gw = (v.astype(np.float64) for v in (r, w, R[:, j], W[:, j]))
            tol = 2 * n * 2.0 ** -53 * w + 2 * u * np.abs(r)
            worst = max(worst, float(np.max(np.abs(gr - r) / tol)))
            assert np.all(np.abs(gr - r) <= tol)
            assert np.all(np.abs(gw - w) <= 2 * n * 2.0 ** -53 * w + 2 * u * w)
        print(f"resid_bound {prec} n={n} lda={lda} nrhs={nrhs} trans={trans}: max |r - r_cpu| / bound {worst:.3f}")
    assert fn(dev.h.ptr, 0, 4, 9, None, 4, None, 9, None, 9, None, None, 9) == -1       # more than 8 columns
    assert fn(dev.h.ptr, 2, 4, 1, None, 4, None, 1, None, 1, None, None, 1) == -1
