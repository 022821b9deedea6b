"""The CPU statement of equilibration and the expert driver (tests/cpu_equil.py) against LAPACK's dgeequ / sgeequ and
dgesvx(fact='E'), before the GPU is asked anything (tests/test_gpu_equil.py).  No GPU needed.

Bit for bit: r, c, rowcnd, colcnd, amax, info against geequ on square and rectangular inputs of all four builders in
both precisions; equed and the scaled matrix against gesvx's.

Against dgesvx(fact='E') with the margins of test_rcond_host.py and test_refine_host.py: |rcond / rcond_lapack - 1| <=
64 n eps / rcond; ferr within 2 % for n >= 33 (n <= 2 is left out of this one comparison for the reason given in
test_refine_host.py: a BLAS with fused multiply-adds computes the residual of one or two products exactly); both berr
at most 4 u.  For n = 1 and 2 the two rcond are not held to each other but each to the values the iteration can end on
(cpu_equil.lacn2_endpoints: 1 / (anorm * the 1-norm of a column of the inverse), from the fp64 inverse, within the same
margin): lacn2 starts from x = inv(op A) (1/n, 1/n), a component of which can be an exact zero that rounding turns into
+-1e-19, and the sign of that noise decides which column the iteration ends on.  Measured on col_scaled n = 2 seed 2
transposed: the twin returns 0.3306, LAPACK the other column's 0.4314; both are correct runs and no margin relates
them (test_rcond_host.py's cases start at n = 5).  x is compared in the equilibrated coordinates, where ferr (before LAPACK divides it by colcnd / rowcnd)
bounds each side's error: max|y_twin - y_lapack| <= (ferr_twin max|y_twin| + ferr_lapack max|y_lapack|) + 4 u max|y|.

Measured here (scipy 1.15, OpenBLAS), n in {1, 2, 33, 129, 300}, seeds 0..2, the four builders, A x = b and A^T x = b:
for n >= 33 rcond differs from LAPACK's by 4e-15 at worst (relative; the smallest margin is 1.5e-10) and ferr by 0.35 %;
berr is at most 1.42 u (twin) and 1.43 u (LAPACK); the x gap reaches 0.08 of its bound.  On scaled_system, A x = b, the
divided ferr is 9.1e3 .. 1.4e8 (colcnd 1.2e-18 .. 1.8e-16): LAPACK's contract, kept.

The observable effects (n = 33, 129, 300, seeds 0..2, LAPACK's own numbers): unequilibrated rcond 3.0e-27 .. 1.9e-24 on
scaled_system and 4.2e-27 .. 5.5e-24 on row_scaled, against 1.5e-5 .. 3.1e-4 and 6.6e-5 .. 1.4e-3 equilibrated;
min|U_ii| / max|A| on scaled_system 4.3e-24 .. 6.7e-22 against n eps = 7e-15 .. 7e-14.
"""
import numpy as np
import pytest

import cpu_equil as ce
import cpu_refine as cr

ORDERS = (1, 2, 33, 129, 300)
SEEDS = (0, 1, 2)
U64 = 2.0 ** -53
EPS64 = 2.0 ** -52
RECT = ((5, 300), (300, 5), (129, 257))
GPU_ORDERS = (33, 129, 300)      # the (n, seed) on which tests/test_gpu_equil.py relies for the observable effects


def _geequ(dtype):
    from scipy.linalg import lapack

    return lapack.dgeequ if np.dtype(dtype) == np.float64 else lapack.sgeequ


def _assert_geequ_bits(A, what):
    r, c, rowcnd, colcnd, amax, info = ce.geequ_twin(A)
    lr, lc, lrow, lcol, lamax, linfo = _geequ(A.dtype)(np.asfortranarray(A))
    assert info == linfo, what
    assert amax == lamax, what
    if info == 0:
        assert r.dtype == A.dtype and r.tobytes() == lr.astype(A.dtype).tobytes(), what + ": r"
        assert c.tobytes() == lc.astype(A.dtype).tobytes(), what + ": c"
        assert rowcnd == lrow and colcnd == lcol, what
    return r, c, rowcnd, colcnd, amax, info


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("kind", ce.KINDS)
def test_geequ_twin_has_lapacks_bits(kind, dtype):
    for n in ORDERS + (64, 257):
        for seed in SEEDS:
            A = ce.system(kind, n, seed)[0].astype(dtype)
            _assert_geequ_bits(A, f"{kind} n={n} seed={seed}")
    big = ce.system(kind, 300, 4)[0].astype(dtype)
    for m, n in RECT:
        _assert_geequ_bits(np.ascontiguousarray(big[:m, :n]), f"{kind} {m}x{n}")
    assert ce.geequ_twin(np.zeros((0, 3), dtype=dtype))[2:] == (1.0, 1.0, 0.0, 0)
    assert ce.geequ_twin(np.zeros((3, 0), dtype=dtype))[2:] == (1.0, 1.0, 0.0, 0)


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("kind", ce.KINDS)
def test_laqge_twin_has_gesvx_equed_and_scaled_matrix(kind, dtype):
    from scipy.linalg import lapack

    gesvx = lapack.dgesvx if dtype == np.float64 else lapack.sgesvx
    for n in (2, 33, 129):
        for seed in SEEDS:
            A, b, _ = ce.system(kind, n, seed)
            A, b = A.astype(dtype), b.astype(dtype)
            r, c, rowcnd, colcnd, amax, info = ce.geequ_twin(A)
            assert info == 0
            equed, S = ce.laqge_twin(A, r, c, rowcnd, colcnd, amax)
            out = gesvx(A, b.reshape(n, 1), fact="E")
            what = f"{kind} n={n} seed={seed}"
            assert ce.EQUED_OF_LAPACK[out[3]] == equed, what
            assert S.tobytes() == np.ascontiguousarray(out[0]).astype(dtype).tobytes(), what + ": scaled matrix"


@pytest.mark.parametrize("kind", ce.KINDS)
def test_every_builder_reaches_the_outcome_it_is_named_after(kind):
    """By LAPACK's own decision, at the seed cpu_equil.seed_for picks, in both precisions (the fp32 rounding of these
    matrices moves no maximum across a threshold)."""
    from scipy.linalg import lapack

    for n in (33, 63, 64, 65, 129, 257, 300):
        seed = ce.seed_for(kind, n)
        A, b, _ = ce.system(kind, n, seed)
        assert ce.EQUED_OF_LAPACK[lapack.dgesvx(A, b.reshape(n, 1), fact="E")[3]] == ce.EXPECTED[kind], (n, seed)
        out32 = lapack.sgesvx(A.astype(np.float32), b.astype(np.float32).reshape(n, 1), fact="E")
        assert ce.EQUED_OF_LAPACK[out32[3]] == ce.EXPECTED[kind], (n, seed)
        print(f"{kind} n={n}: seed {seed}")


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
def test_planted_thresholds(dtype):
    n = 6
    for build, side in ((ce.planted_rows, ce.ROW), (ce.planted_cols, ce.COL)):
        A = build(n, -3, dtype)                                    # ratio 0.125 >= 0.1: left alone
        r, c, rowcnd, colcnd, amax, info = _assert_geequ_bits(A, "planted 2^-3")
        assert (rowcnd, colcnd) == ((0.125, 1.0) if side == ce.ROW else (1.0, 0.125)) and info == 0 and amax == 1.0
        assert ce.laqge_twin(A, r, c, rowcnd, colcnd, amax)[0] == ce.NONE
        A = build(n, -4, dtype)                                    # ratio 0.0625 < 0.1: scaled
        r, c, rowcnd, colcnd, amax, info = _assert_geequ_bits(A, "planted 2^-4")
        equed, S = ce.laqge_twin(A, r, c, rowcnd, colcnd, amax)
        assert equed == side and np.all(S == 1.0)
    A = ce.planted_tiny(n, dtype)                                  # amax < small: rows, although rowcnd = 1
    r, c, rowcnd, colcnd, amax, info = _assert_geequ_bits(A, "planted tiny")
    assert rowcnd == 1.0 and colcnd == 1.0 and amax < ce.limits(dtype)[2]
    equed, S = ce.laqge_twin(A, r, c, rowcnd, colcnd, amax)
    assert equed == ce.ROW and np.max(np.abs(S)) == 1.0


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
def test_zero_row_and_zero_column(dtype):
    from scipy.linalg import lapack

    gesvx = lapack.dgesvx if dtype == np.float64 else lapack.sgesvx
    A0 = ce.system("both", 9, 0)[0].astype(dtype)
    Z = A0.copy()
    Z[4] = 0
    Z[7] = 0
    assert _assert_geequ_bits(Z, "zero rows")[5] == 5              # the first one, 1-based
    tw = ce.gesvx_twin(Z, np.ones((9, 1), dtype=dtype))
    out = gesvx(Z, np.ones((9, 1), dtype=dtype), fact="E")
    assert tw["equed"] == ce.NONE == ce.EQUED_OF_LAPACK[out[3]] and tw["geequ_info"] == 5
    assert 1 <= tw["info"] <= 9 and tw["info"] == out[11] and tw["rcond"] == 0.0 == out[8] and tw["X"] is None
    assert np.all(np.isposinf(tw["ferr"])) and np.all(np.isposinf(tw["berr"]))
    Z = A0.copy()
    Z[:, 2] = 0
    Z[:, 6] = 0
    assert _assert_geequ_bits(Z, "zero columns")[5] == 9 + 3       # m + j
    tw = ce.gesvx_twin(Z, np.ones((9, 1), dtype=dtype))
    out = gesvx(Z, np.ones((9, 1), dtype=dtype), fact="E")
    assert tw["equed"] == ce.NONE == ce.EQUED_OF_LAPACK[out[3]] and tw["info"] == out[11] == 3 and tw["rcond"] == 0.0
    N = A0.copy()
    N[3, 5] = np.nan
    assert np.isnan(ce.geequ_twin(N)[4])


CASES = [(k, n, s, t) for k in ce.KINDS for n in ORDERS for s in SEEDS for t in (False, True)]


def _id(c):
    return f"{c[0]}-n{c[1]}-s{c[2]}-{'T' if c[3] else 'N'}"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_gesvx_twin_agrees_with_lapack(case):
    from scipy.linalg import lapack

    kind, n, seed, trans = case
    A, b, _ = ce.system(kind, n, seed)
    B = b.reshape(n, 1)
    tw = ce.gesvx_twin(A, B, trans=trans, equil=True)
    out = lapack.dgesvx(A, B, fact="E", trans="T" if trans else "N")
    lequed, lr, lc, lx, lrc, lferr, lberr, linfo = (ce.EQUED_OF_LAPACK[out[3]], out[4], out[5], out[7][:, 0], out[8],
                                                    float(out[9][0]), float(out[10][0]), out[11])
    assert tw["equed"] == lequed and tw["info"] == linfo and linfo in (0, n + 1)
    if lequed & ce.ROW:
        assert tw["r"].tobytes() == lr.tobytes()
    if lequed & ce.COL:
        assert tw["c"].tobytes() == lc.tobytes()
    ferr, berr, rc, x = float(tw["ferr"][0]), float(tw["berr"][0]), tw["rcond"], tw["X"][:, 0]
    rbound = 64.0 * n * EPS64 / lrc
    # equilibrated coordinates: where ferr, undivided, bounds the error
    back = tw["c"] if (not trans and lequed & ce.COL) else tw["r"] if (trans and lequed & ce.ROW) else np.ones(n)
    div = tw["colcnd"] if (not trans and lequed & ce.COL) else tw["rowcnd"] if (trans and lequed & ce.ROW) else 1.0
    y, ly = x / back, lx / back
    ymax = max(np.max(np.abs(y)), np.max(np.abs(ly)))
    xbound = ferr * div * np.max(np.abs(y)) + lferr * div * np.max(np.abs(ly)) + 4 * U64 * ymax
    xgap = float(np.max(np.abs(y - ly)))
    print(f"{_id(case)}: equed {lequed} rcond twin {rc:.6e} lapack {lrc:.6e} |ratio-1| {abs(rc / lrc - 1):.2e} allowed "
          f"{rbound:.2e}  ferr twin {ferr:.6e} lapack {lferr:.6e} ratio-1 {ferr / lferr - 1:+.2e}  berr/u twin "
          f"{berr / U64:.2f} lapack {lberr / U64:.2f}  x gap / bound {xgap / xbound:.3f}  divisor {div:.2e}")
    if n >= 33:
        assert abs(rc / lrc - 1.0) <= rbound
        assert abs(ferr / lferr - 1.0) <= 0.02
    else:                                      # n = 1, 2: each on a column the iteration can end on (module docstring)
        ends = ce.lacn2_endpoints(tw["Aeq"], trans)
        print(f"{_id(case)}: rcond the iteration can end on {ends}")
        assert min(abs(rc / e - 1.0) for e in ends) <= rbound and min(abs(lrc / e - 1.0) for e in ends) <= rbound
    assert berr <= 4 * U64 and lberr <= 4 * U64
    assert xgap <= xbound


@pytest.mark.parametrize("n", GPU_ORDERS)
@pytest.mark.parametrize("seed", SEEDS)
def test_the_builders_make_equilibration_observable(n, seed):
    """What the GPU test relies on, from LAPACK alone: without equilibration rcond is below 1e-20 on scaled_system and
    row_scaled, with it above 1e-7; and Matrix's pivot-ratio rule rejects scaled_system."""
    from scipy.linalg import lapack

    for kind in ("both", "row"):
        A, b, _ = ce.system(kind, n, seed)
        plain = lapack.dgesvx(A, b.reshape(n, 1), fact="N")
        eq = lapack.dgesvx(A, b.reshape(n, 1), fact="E")
        ratio = float(np.min(np.abs(np.diag(plain[1]))) / np.max(np.abs(A)))
        print(f"{kind} n={n} seed={seed}: rcond {plain[8]:.2e} equilibrated {eq[8]:.2e} equed {eq[3]} pivot ratio "
              f"{ratio:.2e} n eps {n * EPS64:.1e}")
        assert plain[8] < 1e-20 and eq[8] > 1e-7
        assert ce.EQUED_OF_LAPACK[eq[3]] == ce.EXPECTED[kind]
        if kind == "both":
            assert ratio <= n * EPS64


def test_unequilibrated_twin_is_the_refined_solve():
    """equil=False is gerfs on the matrix as it is: the same numbers as cpu_refine's statement."""
    from scipy.linalg import lu_factor, lu_solve

    A, b, _ = cr.scaled_system(33, 1)
    tw = ce.gesvx_twin(A, b.reshape(33, 1), equil=False)
    f = lu_factor(A)
    x, ferr, berr = cr.gerfs_twin(A, f, b, lu_solve(f, b))
    assert tw["equed"] == ce.NONE and tw["X"][:, 0].tobytes() == x.tobytes()
    assert tw["ferr"][0] == ferr and tw["berr"][0] == berr


def test_new_symbols_and_keywords():
    import linalg_solver_amd as la
    from linalg_solver_amd import _native, dense

    for sfx in ("f64", "f32"):
        for name in (f"lsx_geequ_{sfx}_dev", f"lsx_laqge_{sfx}_dev", f"lsx_gesvx_{sfx}", f"lsx_gesvx_{sfx}_dev"):
            assert name in _native.EXPORTS
    assert (_native.EQUED_NONE, _native.EQUED_ROW, _native.EQUED_COL, _native.EQUED_BOTH) == (0, 1, 2, 3)
    with pytest.raises(ValueError, match="square"):
        dense.solve_expert(np.ones((2, 3)), np.ones(2))
    with pytest.raises(ValueError, match="wrong number of rows"):
        dense.solve_expert(np.eye(3), np.ones(4))
    with pytest.raises(TypeError, match="float64 or float32"):
        dense.solve_expert(np.eye(3), np.ones(3), dtype=np.float16)
    m = la.Matrix([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    with pytest.raises(ValueError, match="square"):
        m.rcond(equilibrate=True)
    with pytest.raises(ValueError, match="square"):
        m.solve_array([1.0, 2.0], equilibrate=True)
    with pytest.raises(ValueError, match="dimensions must match"):
        la.Matrix([[1.0, 2.0], [3.0, 4.0]]).solve_array([1.0], equilibrate=True)
    with pytest.raises(ValueError, match="norm must be 1 or inf"):
        la.Matrix([[1.0, 2.0], [3.0, 4.0]]).rcond(norm=2, equilibrate=True)
