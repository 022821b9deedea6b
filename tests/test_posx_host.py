"""The yardsticks of tests/test_gpu_posx.py, proved on the CPU before the GPU is asked: the numpy twins of the symmetric
residual, of lansy, of pocon and of porfs (tests/cpu_posx.py) against LAPACK (scipy's dpocon / spocon and dposvx /
sposvx with fact = 'N'; this scipy has no dporfs) and against the general twins of tests/cpu_refine.py.  Every assertion
the GPU file makes of the library is made here of the twin, on the same inputs.
"""
import numpy as np
import pytest
from scipy.linalg import lapack

import cpu_chol as cc
import cpu_posx as cp
import cpu_refine as cr

PRECS = ("f64", "f32")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", cp.TWIN_ORDERS)
def test_symmetric_residual_twin_equals_the_general_one(n, prec):
    """From np.triu(A) alone (the lower triangle holds NaN) against cpu_refine.resid_bound on the full matrix, to the
    tolerance tests/test_gpu_refine.py applies to the kernel: two fp64 sums of n terms in different orders."""
    dt = cp.DTYPES[prec]
    A = cp.scaled_spd(n, 1, cp.SCALE_REFINE[prec], dt)
    B, XT = cp.rhs(A, 2, n)
    X = cp.perturbed(XT)
    u = cr.unit(dt)
    for j in range(2):
        r, w = cr.resid_bound(A, X[:, j], B[:, j])
        rs, ws = cp.resid_bound_sym(cc.fill_lower(A, np.nan), X[:, j], B[:, j])
        assert not np.isnan(rs).any() and not np.isnan(ws).any()
        r, w, rs, ws = (v.astype(np.float64) for v in (r, w, rs, ws))
        assert np.all(np.abs(rs - r) <= 2 * n * 2.0 ** -53 * w + 2 * u * np.abs(r))
        assert np.all(np.abs(ws - w) <= 2 * n * 2.0 ** -53 * w + 2 * u * w)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", cp.TWIN_ORDERS)
def test_lansy_twin(n, prec):
    dt = cp.DTYPES[prec]
    A = cp.scaled_spd(n, 0, cp.SCALE_COND[prec], dt, cp.SHIFT_COND[prec])
    ref = float(np.abs(A.astype(np.float64)).sum(axis=0).max())
    got = cp.lansy(cc.fill_lower(A, np.nan))
    assert abs(got - ref) <= n * 2.0 ** -53 * ref
    U, P = cc.planted(n, dtype=dt)
    assert cp.lansy(cc.fill_lower(P, np.nan)) == float(np.abs(P.astype(np.float64)).sum(axis=0).max()), "integers: exact"
    Pn = cc.fill_lower(P, -777.25)
    Pn[0, n - 1] = np.nan
    assert np.isnan(cp.lansy(Pn))
    assert cp.lansy(np.zeros((0, 0), dtype=dt)) == 0.0
    assert np.array_equal(cp.full_from_upper(cc.fill_lower(A, np.nan)), A)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", cp.ORDERS)
def test_pocon_twin_agrees_with_lapack(n, prec):
    """On LAPACK's own factor of the same input: within 64 n eps cond_1 of LAPACK's pocon, at least the exact rcond
    times (1 - bound), 4 .. 11 solves.  The inputs keep the bound <= 0.35."""
    case = cp.cond_case(n, prec)
    bound = case["bound"]
    assert bound <= 0.35
    count = []
    rc = cp.pocon_twin(cc.fill_lower(case["U_lapack"], np.nan), case["anorm"], count)
    print(f"pocon twin {prec} n={n}: {rc:.6e} lapack {case['rcond_lapack']:.6e} exact {case['rcond_exact']:.6e} bound "
          f"{bound:.2e} solves {count[0]}")
    assert abs(rc / case["rcond_lapack"] - 1.0) <= bound
    assert rc >= case["rcond_exact"] * (1.0 - bound)
    assert (4 <= count[0] <= 11) if n > 1 else count[0] == 1
    assert abs(cp.lansy(case["A"]) / case["anorm"] - 1.0) <= n * 2.0 ** -53


def test_pocon_twin_outcomes():
    U, A = cc.planted(5)
    assert cp.pocon_twin(np.zeros((0, 0)), 1.0) == 1.0
    assert cp.pocon_twin(U, 0.0) == 0.0
    Z = U.copy()
    Z[2, 2] = 0.0
    assert cp.pocon_twin(Z, 3.0) == 0.0
    Z[2, 2] = np.nan
    assert cp.pocon_twin(Z, 3.0) == 0.0


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", cp.TWIN_ORDERS)
def test_porfs_twin_meets_the_yardsticks_beside_lapack(n, prec):
    """Perturbed start: 1 .. 5 steps, omega <= 4 u, |berr - omega| <= (n + 1) u (1 + omega), ferr above the true error
    and within [1/6, 3] of the exact value of what lacn2 estimates; LAPACK's posvx(fact = 'N') of the same system is
    printed beside it and held to the same berr and ferr yardsticks."""
    dt = cp.DTYPES[prec]
    case = cp.refine_case(n, prec)
    A, B = case["A"], case["B"]
    k = 3
    X = np.empty((n, k), dtype=dt)
    ferr, berr, steps, solves = np.zeros(k), np.zeros(k), [], []
    Afill, Ufill = cc.fill_lower(A, np.nan), cc.fill_lower(case["U_model"], np.nan)
    for j in range(k):
        X[:, j], ferr[j], berr[j] = cp.porfs_twin(Afill, Ufill, B[:, j], case["X0_model"][:, j], steps, solves)
    assert not np.isnan(X).any()
    cp.check_columns(f"porfs twin {prec} n={n}", n, prec, A, B, case["truth"], case["inv"], X, ferr, berr, max(steps),
                     sum(solves))
    posvx = lapack.dposvx if prec == "f64" else lapack.sposvx
    out = posvx(A, np.ascontiguousarray(B[:, :k]), fact="N", lower=0)
    xl, fl, bl, info = out[5], out[7], out[8], out[9]
    assert info == 0
    u = cr.unit(dt)
    for j in range(k):
        om = cr.omega(A, xl[:, j].astype(dt), B[:, j])
        err = cr.true_error(xl[:, j].astype(dt), case["truth"][j])
        print(f"  lapack col {j}: berr/u {bl[j] / u:.3f} omega/u {om / u:.3f} ferr {fl[j]:.3e} true error {err:.3e}")
        assert abs(bl[j] - om) <= (n + 1) * u * (1 + om) and fl[j] >= err


@pytest.mark.parametrize("dtype", (np.float64, np.float32))
@pytest.mark.parametrize("n", (5, 130, 300))
def test_porfs_twin_leaves_an_exact_solution_alone(n, dtype):
    U, A = cc.planted(n, dtype=dtype)
    x = np.random.default_rng(n).integers(-3, 4, n).astype(dtype)
    b = (A.astype(np.float64) @ x.astype(np.float64)).astype(dtype)
    steps = []
    x2, ferr, berr = cp.porfs_twin(cc.fill_lower(A, np.nan), cc.fill_lower(U, np.nan), b, x, steps)
    assert berr == 0.0 and steps == [0] and np.array_equal(x2, x)


@pytest.mark.parametrize("dtype", (np.float64, np.float32))
@pytest.mark.parametrize("n,nrhs", cp.PLANTED_FEW)
def test_few_column_twin_is_exact_on_the_planted_systems(n, nrhs, dtype):
    """The seeds of tests/test_gpu_chol.py::test_planted_solve: the sweep of the few-column path (whole 128 x 128 block
    inverses in the backward direction too) returns the integer solution exactly wherever the model of the block
    sweeps does: everywhere in fp64, and in fp32 except at (128, 1) and (129, 7), where entries of an fp32 block
    inverse that need more than 24 bits meet non-zeros of the dense X.  There both stay inside gamma_{3n+1}."""
    U, A, X, B = cp.planted_system(n, nrhs, dtype)
    got = cp.potrs_few(cc.fill_lower(U, np.nan), B)
    sweeps = cc.potrs(cc.fill_lower(U, np.nan), B)
    assert not np.isnan(got).any()
    assert np.array_equal(sweeps, X) == cp.planted_exact(n, nrhs, dtype), "where the block sweeps are exact"
    if cp.planted_exact(n, nrhs, dtype):
        assert np.array_equal(got, X)
    assert cc.solve_residual(A, U, B, got) <= cc.gamma(3 * n + 1, dtype)


@pytest.mark.parametrize("dtype", (np.float64, np.float32))
@pytest.mark.parametrize("n", (129, 300, 600))
def test_few_column_twin_within_highams_bound(n, dtype):
    A = cc.spd(n, 0, dtype)
    B = np.random.default_rng(n).standard_normal((n, 7)).astype(dtype)
    R, info = cc.potrf(A)
    assert info == 0
    X = cp.potrs_few(cc.fill_lower(np.triu(R), np.nan), B)
    assert cc.solve_residual(A, R, B, X) <= cc.gamma(3 * n + 1, dtype)
