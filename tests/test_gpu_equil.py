"""Equilibration and the expert driver (lsx_geequ_*, lsx_laqge_*, lsx_gesvx_*) on the MI355X, through `dense`,
`DeviceSolver`, `Matrix` and the C ABI, against the CPU statement tests/cpu_equil.py (which tests/test_equil_host.py
holds to LAPACK's dgeequ / dgesvx) and against yardsticks that share no code with the library (cpu_refine: the backward
error in extended precision, the exact value of what the estimator estimates, true solutions).

Orders 1, 2, 63, 64, 65, 129, 257, 300: the lane (2 / 4 elements), wave (64 lanes), 128-row block and 256-row chunk
edges of the kernels; 1025 once, for the partition of the partial column maxima (5 chunks).

Bit for bit against the twin: r, c, rowcnd, colcnd, amax, info, equed, the scaled matrix, the scaled right-hand sides
(maxima, products and one IEEE division per factor: nothing depends on an order of summation).

Bounds on the rest (u = 2^-53 / 2^-24, eps = 2 u), all in the EQUILIBRATED coordinates A_eq y = b_eq, where gerfs runs;
y = x / c (or x / r) is recovered with one rounding per component, after the driver's own rounding in x = c y, and a
relative perturbation u of y moves the componentwise backward error by at most u: the 2 u below.
  |berr - omega(y)| <= (n + 1) u (1 + omega) + 2 u and omega(y) <= 4 u + 2 u          (test_gpu_refine.py's, plus that)
  exact_bound(y) / 6 <= ferr colcnd <= 3 exact_bound(y)                                 (test_gpu_refine.py's window)
  where ferr was not divided (nothing scaled x): ferr >= the true error of x for the equilibrated data
  |rcond / rcond_twin - 1| <= 64 n eps / rcond_twin, test_gpu_rcond.py's margin (it requires <= 0.35 of its own cases;
      in fp32 the equilibrated matrices here have 64 n eps cond = 0.44 .. 300, where the precision cannot resolve
      the estimate and the margin says little; it is asserted all the same), and 0 < rcond <= 1 + 4 u
      n = 1, 2: within that margin of one of the values the iteration can end on (cpu_equil.lacn2_endpoints, from the
      fp64 inverse) instead of the twin's -- the sign of a component that is zero but for rounding decides on which
      column lacn2 ends (test_equil_host.py; here row_scaled n = 2 fp32: 0.484 against the twin's 0.396)
  |rpvgrw / rpvgrw_twin - 1| <= 2 n^2 u + 4 u: both sides take max|A_eq| (identical) over max|U|, and two LU
      factorisations with the same pivots differ by |dU| <= 2 gamma_n |L| |U| <= 2 n^2 u max|U| (|l_ij| <= 1)

Measured (one MI355X; all orders, builders, trans, 0 / 1 / 3 / 9 columns): fp64 berr at most 2.87 u, omega(y) at most
1.77 u, |berr - omega| at most 1.79 u, ferr colcnd = 0.61 .. 1.14 x the exact bound and at least 4.4 x the true error;
fp32 0.96 u, 0.96 u, 0.21 u, 0.50 .. 1.00 x, 5.0 x.  rcond differs from the twin's by 2.1e-13 (fp64, 7.6e-6 of the
margin) and 5.4e-4 (fp32) for n > 2; rpvgrw by 0 (fp64) and 1.9e-5 (fp32).  The whole file takes 12 s.

The initial solve inside gesvx handles all columns in one call, as lsx_gesvr_* does (that is what makes equil = 0
bit-identical to it), and the few-column solve kernels give a column other bits in a group than alone.  So "a column
gets the same bits whichever columns ride along" is asserted where the library can promise it: for equed, r, c, rcond
and rpvgrw outright, and for x / ferr / berr given the solve -- the refinement and the bounds of any subset of columns,
run through lsx_gerfs_*_dev on what the device form returned, reproduce the driver's bits.
"""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import cpu_equil as ce  # noqa: E402
import cpu_refine as cr  # noqa: E402

ORDERS = (1, 2, 63, 64, 65, 129, 257, 300)
RECT = ((5, 300), (300, 5), (129, 257))
NRHS = (0, 1, 3, 9)
MAXRHS = 9
DTYPES = {"f64": np.float64, "f32": np.float32}
EPS = {"f64": 2.0 ** -52, "f32": 2.0 ** -23}


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


def _reference(kind, n, prec, trans, nrhs=MAXRHS):
    """Inputs, twin and yardsticks of one case, computed once and never modified: A, B in the working precision, the
    twin's results for all columns, the true solutions of the EQUILIBRATED (rounded) system and inv(op A_eq)."""
    key = (kind, n, prec, trans, nrhs)
    if key not in _ref:
        dt = DTYPES[prec]
        A, B, _ = ce.system(kind, n, ce.seed_for(kind, n), nrhs)
        A, B = A.astype(dt), B.astype(dt)
        tw = ce.gesvx_twin(A, B, trans=trans, equil=True)
        Aeq64 = tw["Aeq"].astype(np.float64)
        truth = []
        for j in range(nrhs):
            bj = tw["Beq"][:, j].astype(np.float64)
            truth.append(cr.fraction_solve(cr.op(Aeq64, trans), bj) if n <= 2 else cr.longdouble_solve(Aeq64, bj, trans))
        inv = np.linalg.inv(cr.op(Aeq64, trans))
        for a in (A, B, inv, tw["Aeq"], tw["Beq"]):
            a.setflags(write=False)
        _ref[key] = (A, B, tw, truth, inv)
    return _ref[key]


def _check_geequ(dev, A, what):
    """geequ and laqge on the device against the twin, bit for bit; returns the twin's equed."""
    import torch

    m, n = A.shape
    r, c, rowcnd, colcnd, amax, info = ce.geequ_twin(A)
    tA = torch.from_numpy(np.array(A)).cuda()
    tr, tc, ts = dev.geequ(tA)
    st = ts.cpu().numpy()
    assert (st[3], st[2]) == (info, amax) or (math.isnan(amax) and math.isnan(st[2]) and st[3] == info), what
    if info != 0 or math.isnan(amax):
        return None
    assert (st[0], st[1]) == (rowcnd, colcnd), what
    assert tr.cpu().numpy().tobytes() == r.tobytes(), what + ": r"
    assert tc.cpu().numpy().tobytes() == c.tobytes(), what + ": c"
    equed, S = ce.laqge_twin(A, r, c, rowcnd, colcnd, amax)
    got = dev.laqge_(tA, tr, tc, st[0], st[1], st[2])
    assert got == equed, what
    assert tA.cpu().numpy().tobytes() == S.tobytes(), what + ": scaled matrix"
    return equed


@pytest.mark.parametrize("prec", ("f64", "f32"))
@pytest.mark.parametrize("kind", ce.KINDS)
def test_geequ_and_laqge_have_the_twins_bits(dev, kind, prec):
    dt = DTYPES[prec]
    for n in ORDERS:
        seed = ce.seed_for(kind, n)
        equed = _check_geequ(dev, ce.system(kind, n, seed)[0].astype(dt), f"{kind} {prec} n={n}")
        if n >= 33:
            assert equed == ce.EXPECTED[kind]
    big = ce.system(kind, 300, 4)[0].astype(dt)
    for m, n in RECT:
        _check_geequ(dev, np.ascontiguousarray(big[:m, :n]), f"{kind} {prec} {m}x{n}")


@pytest.mark.parametrize("prec", ("f64", "f32"))
def test_partial_column_maxima_at_1025(dev, prec):
    assert _check_geequ(dev, ce.system("both", 1025, 0)[0].astype(DTYPES[prec]), f"both {prec} n=1025") == ce.BOTH


@pytest.mark.parametrize("prec", ("f64", "f32"))
def test_planted_cases(la, dev, prec):
    import torch

    from linalg_solver_amd import dense

    dt = DTYPES[prec]
    for n in (6, 130):
        for build, side in ((ce.planted_rows, ce.ROW), (ce.planted_cols, ce.COL)):
            assert _check_geequ(dev, build(n, -3, dt), f"planted 2^-3 n={n}") == ce.NONE      # 0.125 >= 0.1
            assert _check_geequ(dev, build(n, -4, dt), f"planted 2^-4 n={n}") == side         # 0.0625 < 0.1
        assert _check_geequ(dev, ce.planted_tiny(n, dt), f"planted tiny n={n}") == ce.ROW     # amax < small
    A0 = ce.system("both", 130, 0)[0].astype(dt)
    for kind, info in (("row", 5), ("col", 130 + 3)):
        Z = A0.copy()
        if kind == "row":
            Z[4] = 0
            Z[77] = 0
        else:
            Z[:, 2] = 0
            Z[:, 99] = 0
        assert _check_geequ(dev, Z, f"zero {kind}") is None
        _, _, ts = dev.geequ(torch.from_numpy(Z).cuda())
        assert ts.cpu().numpy()[3] == info
        tw = ce.gesvx_twin(Z, np.ones((130, 2), dtype=dt))
        x, ferr, berr, rc, growth, equed, r, c, ginfo = dense.solve_expert(Z, np.ones((130, 2)), dtype=dt)
        print(f"zero {kind} {prec}: info {ginfo} twin {tw['info']} rpvgrw {growth:.6e} twin {tw['rpvgrw']:.6e}")
        assert x is None and equed == ce.NONE and rc == 0.0 and 1 <= ginfo <= 130 and ginfo == tw["info"]
        assert np.all(np.isposinf(ferr)) and np.all(np.isposinf(berr))
        assert np.all(r == 1) and np.all(c == 1)                                   # left untouched: the wrapper's ones
        assert abs(growth / tw["rpvgrw"] - 1.0) <= 2 * 130 * 130 * cr.unit(dt) + 4 * cr.unit(dt)
    # empty shapes
    for m, n in ((0, 3), (3, 0)):
        _, _, ts = dev.geequ(torch.zeros(m, n, dtype=torch.float64 if prec == "f64" else torch.float32, device="cuda"))
        assert ts.cpu().numpy().tolist() == [1.0, 1.0, 0.0, 0.0]
    x, ferr, berr, rc, growth, equed, r, c, info = dense.solve_expert(np.zeros((0, 0)), np.zeros((0, 1)), dtype=dt)
    assert (rc, growth, equed, info) == (1.0, 1.0, ce.NONE, 0) and x.shape == (0, 1) and ferr[0] == 0 and berr[0] == 0


@pytest.mark.parametrize("prec", ("f64", "f32"))
def test_nan(la, dev, prec):
    import torch

    from linalg_solver_amd import dense

    dt = DTYPES[prec]
    A, B, _ = ce.system("both", 129, 0, 3)
    A, B = A.astype(dt), B.astype(dt)
    N = A.copy()
    N[77, 5] = np.nan
    _, _, ts = dev.geequ(torch.from_numpy(N).cuda())
    assert math.isnan(ts.cpu().numpy()[2])
    rt, ct = ce.geequ_twin(N)[:2]
    for equil in (True, False):
        x, ferr, berr, rc, growth, equed, r, c, info = dense.solve_expert(N, B, equilibrate=equil, dtype=dt)
        assert x is None and equed == ce.NONE and info == 0 and math.isnan(rc) and math.isnan(growth)
        assert np.all(np.isnan(ferr)) and np.all(np.isnan(berr))
        if equil:           # geequ's info is 0: its factors are handed out although nothing is scaled
            assert r.tobytes() == rt.tobytes() and np.array_equal(c, ct, equal_nan=True)
        # the ABI and the device form: no output is left unwritten behind info = 0 -- X is NaN throughout
        X = np.zeros((129, 3), dtype=dt)
        h = la.default_handle()
        ct_, dp = (C.c_double, C.POINTER(C.c_double)) if prec == "f64" else (C.c_float, C.POINTER(C.c_float))
        eq, inf_, rcd, gr = C.c_int(-1), C.c_int(-1), C.c_double(0), C.c_double(0)
        fe, be, rr, cc = np.zeros(3), np.zeros(3), np.ones(129, dtype=dt), np.ones(129, dtype=dt)
        dd = C.POINTER(C.c_double)
        assert getattr(h.lib, f"lsx_gesvx_{prec}")(h.ptr, int(equil), 0, 129, 3, N.ctypes.data_as(dp), 129, B.ctypes.data_as(dp), 3,
                                                   X.ctypes.data_as(dp), 3, C.byref(eq), rr.ctypes.data_as(dp),
                                                   cc.ctypes.data_as(dp), C.byref(rcd), fe.ctypes.data_as(dd),
                                                   be.ctypes.data_as(dd), C.byref(gr), C.byref(inf_)) == 0
        assert np.all(np.isnan(X)) and inf_.value == 0 and math.isnan(rcd.value)
        tX = torch.zeros(129, 3, dtype=torch.float64 if prec == "f64" else torch.float32, device="cuda")
        for Xarg in (tX, None):
            out = dev.gesvx_(torch.from_numpy(N).cuda(), torch.from_numpy(B).cuda(), equilibrate=equil, X=Xarg)
            assert out["info"] == 0 and math.isnan(out["rcond"]) and bool(torch.isnan(out["X"]).all())
            assert np.all(np.isnan(out["ferr"])) and np.all(np.isnan(out["berr"]))
    # Matrix: NoSolution on the host and on the device path, with and without bounds
    N64 = N.astype(np.float64)
    for M in (la.Matrix.from_numpy(N64), la.Matrix.from_dlpack(torch.from_numpy(N64).cuda())):
        for bounds in (False, True):
            for tr in (False, True):
                assert isinstance(M.solve_array(np.ones(129), trans=tr, bounds=bounds, equilibrate=True), la.Matrix.NoSolution)
        assert math.isnan(M.rcond(equilibrate=True))
    # an exactly zero pivot on the device form: X as the method allocated it (NaN), never allocator garbage
    Z = A.copy()
    Z[:, 17] = 0
    out = dev.gesvx_(torch.from_numpy(Z).cuda(), torch.from_numpy(B).cuda())
    assert out["info"] == 18 and out["rcond"] == 0.0 and bool(torch.isnan(out["X"]).all())
    Bn = B.copy()
    Bn[5, 1] = np.nan                                                           # reaches column 1 only
    good = dense.solve_expert(A, B, dtype=dt)
    bad = dense.solve_expert(A, Bn, dtype=dt)
    assert bad[5] == good[5] == ce.BOTH and math.isnan(bad[1][1]) and math.isnan(bad[2][1])
    for j in (0, 2):
        assert bad[1][j] == good[1][j] and bad[2][j] == good[2][j] and np.array_equal(bad[0][:, j], good[0][:, j])


def _check_solution(tag, kind, n, prec, trans, k, X, ferr, berr, equed, nrhs=MAXRHS):
    """Columns 0 .. k-1 of a gesvx result against the yardsticks of the nrhs-column reference, in the equilibrated
    coordinates."""
    A, B, tw, truth, inv = _reference(kind, n, prec, trans, nrhs)
    dt = DTYPES[prec]
    u = cr.unit(dt)
    scaled_x = (not trans and equed & ce.COL) or (trans and equed & ce.ROW)
    back = tw["c"] if (not trans and equed & ce.COL) else tw["r"] if scaled_x else None
    div = tw["colcnd"] if (not trans and equed & ce.COL) else tw["rowcnd"] if scaled_x else 1.0
    for j in range(k):
        y = (X[:, j] / back).astype(dt) if scaled_x else X[:, j]
        om = cr.omega(tw["Aeq"], y, tw["Beq"][:, j], trans)
        exact = cr.exact_bound(tw["Aeq"], y, tw["Beq"][:, j], trans, inv=inv)
        err = cr.true_error(y, truth[j])
        slack = 2 * u if scaled_x else 0.0
        print(f"{tag} col {j}: berr/u {berr[j] / u:.3f} omega/u {om / u:.3f} |diff|/u {abs(berr[j] - om) / u:.3f} allowed "
              f"{(n + 1) * (1 + om) + slack / u:.1f}  ferr {ferr[j]:.3e} undivided {ferr[j] * div:.3e} exact bound {exact:.3e} "
              f"ratio {ferr[j] * div / exact:.3f} true error {err:.3e}")
        assert abs(berr[j] - om) <= (n + 1) * u * (1 + om) + slack
        assert om <= 4 * u + slack
        assert exact / 6 <= ferr[j] * div <= 3 * exact
        if not scaled_x:
            assert ferr[j] >= err


@pytest.mark.parametrize("prec", ("f64", "f32"))
@pytest.mark.parametrize("trans", (False, True), ids=("N", "T"))
@pytest.mark.parametrize("n", ORDERS)
@pytest.mark.parametrize("kind", ce.KINDS)
def test_gesvx_equilibrated(la, kind, n, trans, prec):
    from linalg_solver_amd import dense

    dt = DTYPES[prec]
    A, B, tw, _, _ = _reference(kind, n, prec, trans)
    u = cr.unit(dt)
    for k in NRHS:
        tag = f"gesvx {kind} {prec} n={n} nrhs={k} {'T' if trans else 'N'}"
        X, ferr, berr, rc, growth, equed, r, c, info = dense.solve_expert(A, np.ascontiguousarray(B[:, :k]), trans=trans,
                                                                          dtype=dt)
        assert equed == tw["equed"] and r.tobytes() == tw["r"].tobytes() and c.tobytes() == tw["c"].tobytes(), tag
        if n >= 33:
            assert equed == ce.EXPECTED[kind]
        rbound = 64.0 * n * EPS[prec] / tw["rcond"]
        print(f"{tag}: equed {equed} rcond {rc:.6e} twin {tw['rcond']:.6e} |ratio-1| {abs(rc / tw['rcond'] - 1):.2e} allowed "
              f"{rbound:.2e}  rpvgrw {growth:.6e} twin {tw['rpvgrw']:.6e} info {info}")
        if n <= 2:       # a column the iteration can end on, as on the CPU (module docstring)
            assert min(abs(rc / e - 1.0) for e in ce.lacn2_endpoints(tw["Aeq"], trans)) <= rbound
        else:
            assert abs(rc / tw["rcond"] - 1.0) <= rbound
            assert info == tw["info"] or rbound > 0.35
        assert 0 < rc <= 1.0 + 4 * u and info in (0, n + 1) and (info == n + 1) == (rc < u)   # n = 1: 1 to rounding
        assert abs(growth / tw["rpvgrw"] - 1.0) <= 2 * n * n * u + 4 * u
        assert X.dtype == dt and X.shape == (n, k) and ferr.shape == berr.shape == (k,)
        _check_solution(tag, kind, n, prec, trans, k, X, ferr, berr, equed)


@pytest.mark.parametrize("trans", (False, True), ids=("N", "T"))
def test_gesvx_at_1025(la, trans):
    from linalg_solver_amd import dense

    A, B, tw, _, _ = _reference("both", 1025, "f64", trans, 3)
    X, ferr, berr, rc, growth, equed, r, c, info = dense.solve_expert(A, B, trans=trans)
    assert equed == ce.BOTH == tw["equed"] and r.tobytes() == tw["r"].tobytes() and c.tobytes() == tw["c"].tobytes()
    assert abs(rc / tw["rcond"] - 1.0) <= 64.0 * 1025 * EPS["f64"] / tw["rcond"] <= 0.35 and info == 0
    assert abs(growth / tw["rpvgrw"] - 1.0) <= 2 * 1025 * 1025 * cr.unit(np.float64)
    _check_solution(f"gesvx 1025 {'T' if trans else 'N'}", "both", 1025, "f64", trans, 3, X, ferr, berr, equed, nrhs=3)


@pytest.mark.parametrize("prec", ("f64", "f32"))
@pytest.mark.parametrize("trans", (False, True), ids=("N", "T"))
@pytest.mark.parametrize("n", (65, 129, 300))
def test_gesvx_unequilibrated_is_gesvr_and_rcond(la, n, trans, prec):
    """equil = 0 on a badly scaled system, and equil = 1 on one that needs no scaling: the bits of lsx_gesvr_* and
    lsx_rcond_*."""
    from linalg_solver_amd import dense

    dt = DTYPES[prec]
    for kind, equil in (("both", False), ("none", False), ("none", True)):
        A, B, _, _, _ = _reference(kind, n, prec, trans)
        for k in (1, 3, 9):
            Bk = np.ascontiguousarray(B[:, :k])
            X, ferr, berr, rc, growth, equed, r, c, info = dense.solve_expert(A, Bk, trans=trans, equilibrate=equil, dtype=dt)
            Xr, fr, br, rinfo = dense.solve_bounded(A, Bk, trans=trans, dtype=dt)
            rcr, _ = dense.rcond(A, norm=np.inf if trans else 1, dtype=dt)
            what = f"{kind} equil={equil} {prec} n={n} nrhs={k} trans={trans}"
            assert equed == ce.NONE and rinfo == 0 and info in (0, n + 1), what
            assert X.tobytes() == Xr.tobytes() and ferr.tobytes() == fr.tobytes() and berr.tobytes() == br.tobytes(), what
            assert rc == rcr, what
            if not equil:
                assert np.all(r == 1) and np.all(c == 1), what                  # left untouched: the wrapper's ones


@pytest.mark.parametrize("prec", ("f64", "f32"))
@pytest.mark.parametrize("trans", (False, True), ids=("N", "T"))
@pytest.mark.parametrize("kind", ce.KINDS)
def test_device_form_and_determinism(la, dev, kind, trans, prec):
    """lsx_gesvx_*_dev: dA / dB return scaled, dLU / d_ipiv are the factors a caller can go on with; two calls give the
    same bits; what does not depend on the right-hand sides does not, and the refinement of any subset of columns
    reproduces the driver's bits (module docstring)."""
    import torch

    from linalg_solver_amd import dense

    n = 129
    dt = DTYPES[prec]
    A, B, tw, _, _ = _reference(kind, n, prec, trans)
    tA, tB = torch.from_numpy(np.array(A)).cuda(), torch.from_numpy(np.array(B)).cuda()
    out = dev.gesvx_(tA, tB, trans=trans)
    assert out["equed"] == tw["equed"] and (out["rowcnd"], out["colcnd"]) == (tw["rowcnd"], tw["colcnd"])
    assert tA.cpu().numpy().tobytes() == tw["Aeq"].tobytes() and tB.cpu().numpy().tobytes() == tw["Beq"].tobytes()
    tA2, tB2 = torch.from_numpy(np.array(A)).cuda(), torch.from_numpy(np.array(B)).cuda()
    out2 = dev.gesvx_(tA2, tB2, trans=trans)
    for key in ("X", "LU", "ipiv", "r", "c"):
        assert torch.equal(out[key], out2[key]), key
    for key in ("equed", "rowcnd", "colcnd", "rcond", "rpvgrw", "info"):
        assert out[key] == out2[key], key
    assert out["ferr"].tobytes() == out2["ferr"].tobytes() and out["berr"].tobytes() == out2["berr"].tobytes()
    hX, hf, hb, hrc, hg, heq, hr, hc, hinfo = dense.solve_expert(A, B, trans=trans, dtype=dt)     # the host form
    assert heq == out["equed"] and hr.tobytes() == out["r"].cpu().numpy().tobytes()
    assert hc.tobytes() == out["c"].cpu().numpy().tobytes()
    # nothing but x, ferr, berr depends on the right-hand sides
    for k in (0, 1, 4):
        sub = dev.gesvx_(torch.from_numpy(np.array(A)).cuda(), torch.from_numpy(np.array(B[:, :k])).cuda(), trans=trans)
        for key in ("equed", "rowcnd", "colcnd", "rcond", "rpvgrw", "info"):
            assert sub[key] == out[key], key
        assert torch.equal(sub["LU"], out["LU"]) and torch.equal(sub["r"], out["r"]) and torch.equal(sub["c"], out["c"])
    # go on from the factors: solve, refine a subset of the columns, scale back -- the driver's bits
    scaled_x = (not trans and out["equed"] & ce.COL) or (trans and out["equed"] & ce.ROW)
    back = out["c"] if (not trans and out["equed"] & ce.COL) else out["r"]
    div = out["colcnd"] if (not trans and out["equed"] & ce.COL) else out["rowcnd"]
    X0 = tB.clone()
    dev.getrs_(out["LU"], out["ipiv"], X0, trans=trans)
    for cols in ((0, 1, 2, 3, 4, 5, 6, 7, 8), (4,), (0, 7, 8)):
        idx = torch.tensor(cols, device="cuda")
        Bs, Xs = tB[:, idx].contiguous(), X0[:, idx].contiguous()
        fs, bs = dev.gerfs_(tA, out["LU"], out["ipiv"], Bs, Xs, trans=trans)
        if scaled_x:
            Xs = back[:, None] * Xs
            fs = fs / div
        assert torch.equal(Xs, out["X"][:, idx]), f"columns {cols}"
        assert fs.tobytes() == out["ferr"][list(cols)].tobytes() and bs.tobytes() == out["berr"][list(cols)].tobytes()


@pytest.mark.parametrize("prec", ("f64", "f32"))
@pytest.mark.parametrize("n", (200, 131))
def test_new_entry_points_on_views(dev, n, prec):
    """lsx_geequ_*_dev, lsx_laqge_*_dev and lsx_gesvx_*_dev on padded, offset and odd-aligned views inside NaN-filled
    buffers (test_gpu_views.View): nothing outside a view is written and the results have the bits of the aligned call.
    n = 200 with off = 0 and pad in {0, 2} (fp64) / {0} (fp32) takes the 16-byte forms, everything else -- n = 131, an odd
    or (fp32) non-multiple-of-4 leading dimension, any offset -- the element-wise ones."""
    import torch

    from test_gpu_views import OFFS, View

    dt = DTYPES[prec]
    nrhs = 3
    A0, B0, _ = ce.system("both", n, 0, nrhs)
    A0, B0 = A0.astype(dt), B0.astype(dt)
    r0, c0, s0 = dev.geequ(torch.from_numpy(A0).cuda())
    st = s0.cpu().numpy()
    for trans in (False, True):
        tAeq, tBeq = torch.from_numpy(A0).cuda(), torch.from_numpy(B0).cuda()
        reft = dev.gesvx_(tAeq, tBeq, trans=trans)
        assert reft["equed"] == ce.BOTH
        Aeq, Beq = tAeq.cpu().numpy(), tBeq.cpu().numpy()
        back = (reft["r"] if trans else reft["c"]).cpu().numpy().astype(np.float64)
        div = reft["rowcnd"] if trans else reft["colcnd"]
        for off in OFFS[np.dtype(dt).name]:
            for pad in (0, 1, 2, 3):
                what = f"views {prec} n={n} trans={trans} off={off} pad={pad}"
                vA = View(n, n, n + pad, off, dt, A0)
                vr = View(1, n, n, (off + 1) % 2, dt)
                vc = View(1, n, n, off, dt)
                if not trans:
                    name = f"lsx_geequ_{prec}_dev"
                    stats = torch.zeros(4, dtype=torch.float64, device="cuda")
                    assert getattr(dev.lib, name)(dev.h.ptr, n, n, vA.t.data_ptr(), n + pad, vr.t.data_ptr(), vc.t.data_ptr(),
                                                  stats.data_ptr()) == 0
                    for v, w in ((vA, "A"), (vr, "r"), (vc, "c")):
                        v.check_padding(what + " geequ " + w)
                    assert vA.numpy().tobytes() == A0.tobytes() and stats.cpu().numpy().tobytes() == st.tobytes(), what
                    assert torch.equal(vr.t[0], r0) and torch.equal(vc.t[0], c0), what
                    # the measurement hook that runs one pass at a time: the same kernels, the same results
                    vr2, vc2 = View(1, n, n, off, dt), View(1, n, n, (off + 1) % 2, dt)
                    stats2 = torch.zeros(4, dtype=torch.float64, device="cuda")
                    hook = getattr(dev.lib, f"lsx_diag_geequ_pass_{prec}_dev")
                    for passes in (1, 2):
                        assert hook(dev.h.ptr, passes, n, n, vA.t.data_ptr(), n + pad, vr2.t.data_ptr(), vc2.t.data_ptr(),
                                    stats2.data_ptr()) == 0
                    for v, w in ((vA, "A"), (vr2, "r"), (vc2, "c")):
                        v.check_padding(what + " geequ passes " + w)
                    assert stats2.cpu().numpy().tobytes() == st.tobytes() and vA.numpy().tobytes() == A0.tobytes(), what
                    assert torch.equal(vr2.t[0], r0) and torch.equal(vc2.t[0], c0), what
                    assert dev.laqge_(vA.t, vr.t[0], vc.t[0], st[0], st[1], st[2]) == ce.BOTH
                    vA.check_padding(what + " laqge")
                    assert vA.numpy().tobytes() == Aeq.tobytes(), what + ": scaled matrix"
                    vA = View(n, n, n + pad, off, dt, A0)
                vLU = View(n, n, n + (pad + 1) % 4, (off + 1) % 2, dt)
                vB = View(n, nrhs, nrhs + pad, off, dt, B0)
                vX = View(n, nrhs, nrhs + (3 - pad), off, dt)
                got = dev.gesvx_(vA.t, vB.t, trans=trans, LU=vLU.t, X=vX.t)
                for v, w in ((vA, "A"), (vLU, "LU"), (vB, "B"), (vX, "X")):
                    v.check_padding(what + " gesvx " + w)
                for key in ("equed", "rowcnd", "colcnd", "info"):
                    assert got[key] == reft[key], what
                assert torch.equal(got["r"], reft["r"]) and torch.equal(got["c"], reft["c"]), what
                assert np.all(np.isfinite(vX.numpy())), what
                # the scaled data are bit-identical whatever the layout; the factors, and with them x and the bounds,
                # agree to rounding (test_gpu_views.py: the two forms of the LU kernels are not promised the same bits):
                # each side within its own undivided ferr of the truth, in the equilibrated coordinates
                assert vA.numpy().tobytes() == Aeq.tobytes() and vB.numpy().tobytes() == Beq.tobytes(), what
                for j in range(nrhs):
                    yg = vX.numpy()[:, j].astype(np.float64) / back
                    yr = reft["X"].cpu().numpy()[:, j].astype(np.float64) / back
                    assert np.max(np.abs(yg - yr)) <= ((got["ferr"][j] * div) * np.max(np.abs(yg)) +
                                                       (reft["ferr"][j] * div) * np.max(np.abs(yr))), what
                print(f"{what}: same bits as the aligned call: X {vX.numpy().tobytes() == reft['X'].cpu().numpy().tobytes()} "
                      f"rcond {got['rcond'] == reft['rcond']}")


def test_arguments(la, dev):
    import torch

    h = la.default_handle()
    lib = h.lib
    dp = C.POINTER(C.c_double)
    A, B, X = np.eye(4), np.ones((4, 2)), np.zeros((4, 2))
    r, c = np.ones(4), np.ones(4)
    fe, be = np.zeros(2), np.zeros(2)
    eq, info, rc, gr = C.c_int(-1), C.c_int(-1), C.c_double(-1), C.c_double(-1)
    pA, pB, pX, pr, pc, pf, pb = (v.ctypes.data_as(dp) for v in (A, B, X, r, c, fe, be))
    tail = (C.byref(eq), pr, pc, C.byref(rc), pf, pb, C.byref(gr), C.byref(info))
    ok = lambda *a: lib.lsx_gesvx_f64(h.ptr, *a)   # noqa: E731
    assert ok(2, 0, 4, 2, pA, 4, pB, 2, pX, 2, *tail) == -1 and b"bad argument" in lib.lsx_last_error()   # equil
    assert ok(1, 2, 4, 2, pA, 4, pB, 2, pX, 2, *tail) == -1                                               # trans
    assert ok(1, 0, -1, 2, pA, 4, pB, 2, pX, 2, *tail) == -1
    assert ok(1, 0, 4, 2, pA, 3, pB, 2, pX, 2, *tail) == -1                                               # lda < n
    assert ok(1, 0, 4, 2, pA, 4, pB, 1, pX, 2, *tail) == -1                                               # ldb < nrhs
    assert ok(1, 0, 4, 2, pA, 4, pB, 2, pX, 1, *tail) == -1                                               # ldx < nrhs
    assert ok(1, 0, 4, 2, None, 4, pB, 2, pX, 2, *tail) == -1
    assert ok(1, 0, 4, 2, pA, 4, None, 2, pX, 2, *tail) == -1
    assert ok(1, 0, 4, 2, pA, 4, pB, 2, pX, 2, C.byref(eq), None, pc, C.byref(rc), pf, pb, C.byref(gr), C.byref(info)) == -1
    assert ok(1, 0, 4, 2, pA, 4, pB, 2, pX, 2, C.byref(eq), pr, pc, None, pf, pb, C.byref(gr), C.byref(info)) == -1
    assert ok(1, 0, 4, 2, pA, 4, pB, 2, pX, 2, C.byref(eq), pr, pc, C.byref(rc), None, pb, C.byref(gr), C.byref(info)) == -1
    assert ok(0, 0, 4, 2, pA, 4, pB, 2, pX, 2, C.byref(eq), None, None, C.byref(rc), pf, pb, C.byref(gr), C.byref(info)) == 0
    assert ok(1, 0, 4, 2, pA, 4, pB, 2, pX, 2, *tail) == 0 and np.array_equal(X, np.ones((4, 2)))          # the identity
    assert (eq.value, info.value, rc.value, gr.value) == (0, 0, 1.0, 1.0) and np.array_equal(be, [0, 0])
    assert ok(1, 1, 4, 0, pA, 4, None, 0, None, 0, C.byref(eq), pr, pc, C.byref(rc), None, None, C.byref(gr),
              C.byref(info)) == 0 and rc.value == 1.0
    assert ok(1, 0, 0, 2, None, 0, None, 2, None, 2, *tail) == 0 and (rc.value, gr.value, eq.value) == (1.0, 1.0, 0)
    # device forms
    tA = torch.eye(4, dtype=torch.float64, device="cuda")
    tr, tc = torch.ones(4, dtype=torch.float64, device="cuda"), torch.ones(4, dtype=torch.float64, device="cuda")
    ts = torch.zeros(4, dtype=torch.float64, device="cuda")
    g = lambda m, n, a, lda, rr, cc, ss: dev.lib.lsx_geequ_f64_dev(dev.h.ptr, m, n, a, lda, rr, cc, ss)   # noqa: E731
    assert g(-1, 4, tA.data_ptr(), 4, tr.data_ptr(), tc.data_ptr(), ts.data_ptr()) == -1
    assert g(4, 4, tA.data_ptr(), 3, tr.data_ptr(), tc.data_ptr(), ts.data_ptr()) == -1
    assert g(4, 4, None, 4, tr.data_ptr(), tc.data_ptr(), ts.data_ptr()) == -1
    assert g(4, 4, tA.data_ptr(), 4, None, tc.data_ptr(), ts.data_ptr()) == -1
    assert g(4, 4, tA.data_ptr(), 4, tr.data_ptr(), tc.data_ptr(), None) == -1
    assert g(0, 4, None, 4, None, None, ts.data_ptr()) == 0
    assert g(4, 4, tA.data_ptr(), 4, tr.data_ptr(), tc.data_ptr(), ts.data_ptr()) == 0
    dev.h.synchronize()
    assert ts.cpu().numpy().tolist() == [1.0, 1.0, 1.0, 0.0]
    q = lambda m, lda, a, e: dev.lib.lsx_laqge_f64_dev(dev.h.ptr, m, 4, a, lda, tr.data_ptr(), tc.data_ptr(), 1.0, 1.0,   # noqa: E731
                                                       1.0, e)
    assert q(-1, 4, tA.data_ptr(), C.byref(eq)) == -1 and q(4, 3, tA.data_ptr(), C.byref(eq)) == -1
    assert q(4, 4, None, C.byref(eq)) == -1 and q(4, 4, tA.data_ptr(), None) == -1
    assert q(4, 4, tA.data_ptr(), C.byref(eq)) == 0 and eq.value == 0
    tLU, tp = torch.zeros(4, 4, dtype=torch.float64, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    tB = torch.ones(4, 2, dtype=torch.float64, device="cuda")
    tX = torch.zeros(4, 2, dtype=torch.float64, device="cuda")

    def d(equil, trans, lda, ldlu, a=tA.data_ptr(), rr=tr.data_ptr()):
        return dev.lib.lsx_gesvx_f64_dev(dev.h.ptr, equil, trans, 4, 2, a, lda, tLU.data_ptr(), ldlu, tp.data_ptr(),
                                         tB.data_ptr(), 2, tX.data_ptr(), 2, C.byref(eq), rr, tc.data_ptr(), None, None,
                                         C.byref(rc), pf, pb, C.byref(gr), C.byref(info))
    assert d(3, 0, 4, 4) == -1 and d(1, 2, 4, 4) == -1 and d(1, 0, 3, 4) == -1 and d(1, 0, 4, 3) == -1
    assert d(1, 0, 4, 4, a=None) == -1 and d(1, 0, 4, 4, rr=None) == -1
    assert d(1, 0, 4, 4) == 0 and bool((tX == 1).all()) and rc.value == 1.0


def test_matrix_with_equilibrate(la):
    """scaled_system(129, 0): solve_array calls it singular by the pivot ratio and keeps doing so; equilibrate=True solves
    it, within ferr of the extended-precision solution (ferr is LAPACK's divided one here: a bound, if a vacuous one, so
    the undivided one of the equilibrated coordinates is checked too); rcond goes from below 1e-20 to above 1e-7."""
    import torch

    from linalg_solver_amd import dense

    n = 129
    A, b, _ = cr.scaled_system(n, 0)
    xt = cr.longdouble_solve(A, b)
    for M, on_device in ((la.Matrix.from_numpy(np.array(A)), False),
                         (la.Matrix.from_dlpack(torch.from_numpy(np.array(A)).cuda()), True)):
        assert isinstance(M.solve_array(np.array(b)), la.Matrix.NoSolution)
        assert isinstance(M.solve_array(np.array(b), bounds=True), la.Matrix.NoSolution)
        x = M.solve_array(np.array(b), equilibrate=True)
        xb, ferr, berr = M.solve_array(np.array(b), bounds=True, equilibrate=True)
        xm, fm, bm = M.solve_array(np.array(b).reshape(n, 1), bounds=True, equilibrate=True)
        if on_device:
            assert x.is_cuda and xb.is_cuda
            x, xb, xm = x.cpu().numpy(), xb.cpu().numpy(), xm.cpu().numpy()
            assert torch.equal(M._dev.cpu(), torch.from_numpy(A)), "the caller's tensor was modified"
        assert x.shape == (n,) and x.tobytes() == xb.tobytes() == xm[:, 0].tobytes()
        assert isinstance(ferr, float) and isinstance(berr, float) and (ferr, berr) == (fm[0], bm[0])
        err = cr.true_error(x, xt)
        _, _, _, _, _, equed, r, c, _ = dense.solve_expert(A, b)
        tw = ce.gesvx_twin(A, b.reshape(n, 1))
        yerr = cr.true_error(x / c, xt / c.astype(np.longdouble))
        print(f"Matrix equilibrate device={on_device}: true error {err:.3e} ferr {ferr:.3e} berr/u {berr / 2.0 ** -53:.2f} "
              f"equilibrated coordinates: error {yerr:.3e} undivided ferr {ferr * tw['colcnd']:.3e}")
        assert equed == ce.BOTH and err <= ferr and berr <= 4 * 2.0 ** -53
        assert yerr <= ferr * tw["colcnd"] * (1 + 1e-12) + 4 * 2.0 ** -53
        rc0, rc1 = M.rcond(), M.rcond(equilibrate=True)
        ri0, ri1 = M.rcond(norm=np.inf), M.rcond(norm=np.inf, equilibrate=True)
        print(f"Matrix rcond device={on_device}: {rc0:.3e} -> {rc1:.3e} (1-norm), {ri0:.3e} -> {ri1:.3e} (inf-norm)")
        assert rc0 < 1e-20 and rc1 > 1e-7 and ri0 < 1e-20 and ri1 > 1e-7
        assert M.cond(equilibrate=True) == pytest.approx(1.0 / rc1, rel=1e-12) and M.cond() > 1e20
        assert rc1 == dense.solve_expert(A, np.zeros((n, 0)))[3] and ri1 == dense.solve_expert(A, np.zeros((n, 0)), trans=True)[3]
        # LAPACK's criterion: an exactly zero pivot is NoSolution with equilibrate=True too
        Z = np.array(A)
        Z[:, 17] = 0.0
        S = la.Matrix.from_dlpack(torch.from_numpy(Z).cuda()) if on_device else la.Matrix.from_numpy(Z)
        assert isinstance(S.solve_array(np.ones(n), equilibrate=True), la.Matrix.NoSolution)
        assert S.rcond(equilibrate=True) == 0.0
