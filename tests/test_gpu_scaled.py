"""Power-of-two scaling as an exact symmetry of the library on the MI355X (tests/scaled.py; the relations are proved
of the reference arithmetic alone by tests/test_scaled_host.py).  Every assertion is an equality, or a bound the
planted tests already use, applied where the scaling puts the entries:

A. getrf, host-buffer and device-pointer form, every panel and driver at order 300, the look-ahead driver at 641:
   planted pivots, info 0, factors within 8 u max|A| 2^{d_j} COLUMN BY COLUMN of the scaled planted factors, and
   bit for bit the library's own unit-scale factors times diag(2^d); random matrices: same pivots, factors times 2^s.
B. det of a planted matrix is +-2^k: sign and mantissa 1/2 exactly, exp2 = 1 + sum log2|U_kk| + sum d as integers.
C. getrs, transposed getrs (grouped and blocked), gesv, getri, the refined fp32 solve: bit for bit the unit-scale
   results with the rows rescaled; pivot ratio and last correction unchanged; on planted inputs the rescaled solution
   also meets the bounds of test_gpu_planted._solve_checks.
D. rcond, gecon from device factors, the norms: rcond and the number of solves unchanged, the norms times 2^s.
E. Row reductions, both rules, blocked on and off, host and device form: rank, pivots and all of R as at unit scale
   (scaled.rref_expected), default tolerance and an explicit one scaled with the data; the tolerance edge at scale;
   the traced reduction.
F. Subnormal pivots: the factors are the scaled planted ones bit for bit, as LAPACK's getf2 returns them.
G. Matrix.solve_array / inverse_array at 2^-1010 and 2^+1000 of a system whose pivot ratio is about 1e-10: a solution,
   not NoSolution, and bit for bit the unit-scale one (the inverse times 2^-s, inf where that product overflows).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import planted_rref as pr  # noqa: E402
import scaled as sc  # noqa: E402

DTYPES = list(sc.DTYPES)
DEFAULTS = dict(panel=4, lookahead=1, lookahead_min=0)


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


def _set(handles, **opts):
    for h in handles:
        for k, v in opts.items():
            h.set_option(k, v)


def _restore(handles):
    _set(handles, **DEFAULTS)


def _drivers(n):
    """The option sets an order is factored under."""
    if n == 300:
        return [dict(panel=p, lookahead=look, lookahead_min=sc.LOOKAHEAD_MIN) for p, look in sc.DRIVERS_300]
    if n == 641:
        return [dict(lookahead_min=sc.LOOKAHEAD_MIN)]
    return [dict()]


def _factor_host(A, dtype):
    from linalg_solver_amd import dense

    return dense.lu_factor(A, dtype=dtype)


def _factor_dev(dev, A):
    import torch

    dA = torch.from_numpy(np.ascontiguousarray(A)).cuda()
    dpiv, dinfo = dev.getrf_(dA)
    torch.cuda.synchronize()
    return dA, dpiv, int(dinfo.item())


def _scaled_factors(LU, d):
    """LU diag(2^d) on and above the diagonal, L as it is: what the factors of A diag(2^d) must be, bit for bit."""
    n = LU.shape[0]
    up = np.triu_indices(n)
    want = np.array(LU, copy=True)
    want[up] = sc.scale_columns(LU, d, LU.dtype)[up]
    return want


def _check_columns(n, dtype, d, LU, ipiv, info, label):
    """A priori: planted pivots, info 0, and every column within 8 u max|A| 2^{d_j} of the scaled planted factors."""
    A, _, _, _, want_piv = sc.planted(n)
    assert info == 0, label
    assert LU.dtype == np.dtype(dtype), label
    assert np.array_equal(ipiv, want_piv), f"{label}: first differing column {int(np.nonzero(ipiv != want_piv)[0][0])} of {n}"
    assert np.all(np.isfinite(LU)), label
    err = np.abs(LU.astype(np.float64) - sc.planted_lu_scaled(n, d)).max(axis=0)
    bound = 8 * sc.U_ROUND[sc.name(dtype)] * float(np.abs(A).max()) * np.exp2(d.astype(np.float64))
    worst = int(np.argmax(err / bound))
    print(f"SCALED {sc.name(dtype)} n={n} {label}: columns differing {int(np.count_nonzero(err))}, worst column {worst}: "
          f"{err[worst]:.3e} (bound {bound[worst]:.3e}, 2^{int(d[worst])})")
    assert np.all(err <= bound), f"{label}: column {worst}"


# ------------------------------------------------------------------------------------------------ A, B
@pytest.mark.parametrize("dtype", DTYPES, ids=sc.name)
@pytest.mark.parametrize("n", sc.ORDERS)
def test_planted_factors_and_determinant_scale_by_column(la, dev, n, dtype):
    from linalg_solver_amd import dense

    A = sc.planted(n)[0]
    zero = sc.factor_exponents(dtype, "unit", n)
    handles = (la.default_handle(), dev.h)
    try:
        for opts in _drivers(n):
            _set(handles, **opts)
            label = " ".join(f"{k}={v}" for k, v in opts.items()) or "default"
            LU0, ipiv0, info0 = _factor_host(A.astype(dtype), dtype)
            _check_columns(n, dtype, zero, LU0, ipiv0, info0, f"unit lu_factor {label}")
            dLU0, dpiv0, dinfo0 = _factor_dev(dev, A.astype(dtype))
            assert dinfo0 == 0 and np.array_equal(dLU0.cpu().numpy(), LU0) and np.array_equal(dpiv0.cpu().numpy()[:n], ipiv0)
            for kind in sc.FACTOR_KINDS:
                d = sc.factor_exponents(dtype, kind, n)
                As = sc.scale_columns(A, d, dtype)
                LU, ipiv, info = _factor_host(As, dtype)
                _check_columns(n, dtype, d, LU, ipiv, info, f"{kind} lu_factor {label}")
                assert np.array_equal(LU, _scaled_factors(LU0, d)), f"{kind} lu_factor {label}: not the unit-scale factors times diag(2^d)"
                dLU, dpiv, dinfo = _factor_dev(dev, As)
                _check_columns(n, dtype, d, dLU.cpu().numpy(), dpiv.cpu().numpy()[:n], dinfo, f"{kind} getrf_ {label}")
                assert np.array_equal(dLU.cpu().numpy(), LU), f"{kind} {label}: the two entry points must agree bit for bit"
                # B
                want = sc.det_expected(n, d)
                got = tuple(float(v) for v in dev.det_parts(dLU, dpiv).cpu().numpy())
                host = dense.det_parts(As, dtype=dtype)
                print(f"DET {sc.name(dtype)} n={n} {kind} {label}: {got}, lsx_det {host}, expected {want}")
                assert got == (want[0], want[1], float(want[2])), f"{kind} {label}"
                assert host == want, f"{kind} {label}"
    finally:
        _restore(handles)


@pytest.mark.parametrize("dtype", DTYPES, ids=sc.name)
@pytest.mark.parametrize("n", sc.ORDERS)
def test_random_factors_scale_uniformly(la, dev, n, dtype):
    A = sc.random_matrix(n, dtype)
    handles = (la.default_handle(), dev.h)
    try:
        for opts in _drivers(n):
            _set(handles, **opts)
            LU0, ipiv0, info0 = _factor_host(A, dtype)
            assert info0 == 0
            for s in sc.RANDOM_EXP[sc.name(dtype)]:
                d = np.full(n, s, dtype=np.int64)
                want = _scaled_factors(LU0, d)
                LU, ipiv, info = _factor_host(sc.scale(A, s), dtype)
                dLU, dpiv, dinfo = _factor_dev(dev, sc.scale(A, s))
                print(f"RANDOM {sc.name(dtype)} n={n} 2^{s} {opts}: entries differing {int(np.count_nonzero(LU != want))}, "
                      f"pivots differing {int(np.count_nonzero(ipiv != ipiv0))}")
                assert info == 0 and dinfo == 0
                assert np.array_equal(ipiv, ipiv0) and np.array_equal(dpiv.cpu().numpy()[:n], ipiv0)
                assert np.array_equal(LU, want) and np.array_equal(dLU.cpu().numpy(), want)
    finally:
        _restore(handles)


# ------------------------------------------------------------------------------------------------ C
def _solve_options(n):
    """Order 300: every substitution mode, and the blocked transposed sweeps from one right-hand side on.  Each set is
    applied on top of the defaults."""
    if n == 300:
        return [dict(trsv=0), dict(trsv=1), dict(trsv=2), dict(getrs_t_blocked_min=1)]
    return [dict()]


@pytest.mark.parametrize("dtype", DTYPES, ids=sc.name)
@pytest.mark.parametrize("kind", sc.SOLVE_KINDS)
@pytest.mark.parametrize("n", sc.ORDERS)
def test_solves_and_inverse_of_a_scaled_planted_matrix(la, dev, n, kind, dtype):
    import torch

    import test_gpu_planted as tgp
    from linalg_solver_amd import dense

    A = sc.planted(n)[0]
    d = sc.solve_exponents(dtype, kind, n)
    t = sc.rhs_exponent(dtype, kind)
    uniform = int(d.min()) == int(d.max())
    A0, As = A.astype(dtype), sc.scale_columns(A, d, dtype)
    handles = (la.default_handle(), dev.h)
    saved = [{k: h.get_option(k) for k in ("trsv", "getrs_t_blocked_min")} for h in handles]
    cuda = lambda M: torch.from_numpy(np.ascontiguousarray(M)).cuda()   # noqa: E731
    try:
        for opts in _solve_options(n):
            for h, was in zip(handles, saved):
                _set((h,), **was)
            _set(handles, **opts)
            dLU0, dpiv0, i0 = _factor_dev(dev, A0)
            dLU, dpiv, i1 = _factor_dev(dev, As)
            assert i0 == 0 and i1 == 0
            LU0, LU, ipiv = dLU0.cpu().numpy(), dLU.cpu().numpy(), dpiv.cpu().numpy()[:n]
            for nrhs in sc.NRHS:
                label = f"{kind} nrhs={nrhs} {opts}"
                X0, B = sc.planted_rhs(n, nrhs)
                B0, Bs = B.astype(dtype), sc.scale(B.astype(dtype), t)
                Xu = dev.getrs_(dLU0, dpiv0, cuda(B0)).cpu().numpy()
                X = dev.getrs_(dLU, dpiv, cuda(Bs)).cpu().numpy()
                assert np.array_equal(X, sc.scale_rows(Xu, t - d)), f"getrs_ {label}"
                tgp._solve_checks(n, dtype, A, sc.scale_rows(X.astype(np.float64), d - t), X0, B, f"scaled getrs_ {label}")
                assert np.array_equal(dense.lu_solve(LU, ipiv, Bs), X), f"lu_solve {label}"
                Xg0, gi0, ratio0 = dense.solve(A0, B0, dtype=dtype)
                Xg, gi, ratio = dense.solve(As, Bs, dtype=dtype)
                assert gi0 == 0 and gi == 0 and np.array_equal(Xg, sc.scale_rows(Xg0, t - d)), f"gesv {label}"
                if uniform:
                    assert ratio == ratio0, f"gesv {label}: pivot ratio {ratio!r}, at unit scale {ratio0!r}"
                # A'^T X = diag(2^d) B has the solution of A^T X = B
                X0t, Bt = sc.planted_rhs(n, nrhs, trans=True)
                Bt0, Bts = Bt.astype(dtype), sc.scale_rows(Bt.astype(dtype), d)
                Xtu = dev.getrs_(dLU0, dpiv0, cuda(Bt0), trans=True).cpu().numpy()
                Xt = dev.getrs_(dLU, dpiv, cuda(Bts), trans=True).cpu().numpy()
                path = dev.h.get_option("getrs_t_path")
                if "getrs_t_blocked_min" in opts:
                    assert path == 1, f"getrs_ trans {label}: the blocked sweeps were not taken"
                assert np.array_equal(Xt, Xtu), f"getrs_ trans {label} (path {path})"
                tgp._solve_checks(n, dtype, A, Xt, X0t, Bt, f"scaled getrs_ trans {label}", trans=True)
                assert np.array_equal(dense.lu_solve(LU, ipiv, Bts, trans=True), Xt), f"lu_solve trans {label}"
            inv0 = dev.getri(dLU0, dpiv0).cpu().numpy()
            inv = dev.getri(dLU, dpiv).cpu().numpy()
            assert np.all(np.isfinite(inv0))
            assert np.array_equal(inv, sc.scale_rows(inv0, -d)), f"getri {kind} {opts}"
            hinv0, hi0, hr0 = dense.inv(A0, dtype=dtype)
            hinv, hi, hr = dense.inv(As, dtype=dtype)
            assert hi0 == 0 and hi == 0 and np.array_equal(hinv, sc.scale_rows(hinv0, -d)), f"lsx_getri {kind} {opts}"
            if uniform:
                assert hr == hr0
    finally:
        for h, was in zip(handles, saved):
            _set((h,), **was)


@pytest.mark.parametrize("source", ("planted", "random"))
@pytest.mark.parametrize("n", (129, 300))
def test_refined_solve_of_a_uniformly_scaled_system(la, dev, n, source):
    from linalg_solver_amd import dense

    if source == "planted":
        A, B = sc.planted(n)[0].astype(np.float32), sc.planted_rhs(n, 3)[1].astype(np.float32)
    else:
        A, B = sc.random_matrix(n, np.float32), sc.random_rhs(n, 3, np.float32)
    X0, info0, ratio0, corr0 = dense.solve_refined(A, B)
    assert info0 == 0 and np.all(np.isfinite(X0))
    for s in sc.RANDOM_EXP["float32"]:
        t = -s // 2
        X, info, ratio, corr = dense.solve_refined(sc.scale(A, s), sc.scale(B, t))
        print(f"REFINED {source} n={n} 2^{s}: pivot ratio {ratio!r} ({ratio0!r}), last correction {corr!r} ({corr0!r}), "
              f"entries differing {int(np.count_nonzero(X != sc.scale(X0, t - s)))}")
        assert info == 0 and ratio == ratio0 and corr == corr0
        assert np.array_equal(X, sc.scale(X0, t - s))


# ------------------------------------------------------------------------------------------------ D
@pytest.mark.parametrize("dtype", DTYPES, ids=sc.name)
@pytest.mark.parametrize("norm", (1, "inf"))
@pytest.mark.parametrize("source", ("planted", "random"))
@pytest.mark.parametrize("n", (129, 300))
def test_condition_estimate_and_norms_of_a_uniformly_scaled_matrix(la, dev, n, source, norm, dtype):
    import torch

    from linalg_solver_amd import dense

    A = sc.planted(n)[0].astype(dtype) if source == "planted" else sc.random_matrix(n, dtype)
    exps = tuple(sc.SOLVE_EXP[sc.name(dtype)].values()) if source == "planted" else sc.RANDOM_EXP[sc.name(dtype)]
    h = la.default_handle()

    def run(M):
        rc, info = dense.rcond(M, norm, dtype=dtype)
        solves = h.get_option("gecon_solves")
        hnorm = dense.norm(M, norm, dtype=dtype)
        dM = torch.from_numpy(M).cuda()
        dnorm = dev.norm(dM, norm)
        dpiv, dinfo = dev.getrf_(dM)
        drc = dev.rcond(dM, dpiv, dnorm, norm)
        assert info == 0 and int(dinfo.item()) == 0
        return rc, solves, hnorm, float(dnorm.item()), drc, dev.h.get_option("gecon_solves")

    rc0, solves0, hnorm0, dnorm0, drc0, dsolves0 = run(A)
    assert 0 < rc0 < 1 and rc0 == drc0 and hnorm0 == dnorm0 and solves0 == dsolves0 > 0
    for s in exps:
        rc, solves, hnorm, dnorm, drc, dsolves = run(sc.scale(A, s))
        print(f"RCOND {sc.name(dtype)} n={n} {source} norm={norm} 2^{s}: {rc!r} ({rc0!r}), solves {solves} ({solves0}), norm {hnorm!r}")
        assert rc == rc0 and drc == rc0
        assert solves == solves0 and dsolves == solves0
        assert hnorm == float(np.ldexp(hnorm0, s)) and dnorm == hnorm


# ------------------------------------------------------------------------------------------------ E
def _rref_host(la, A, bar, dtype, rule, tol):
    from linalg_solver_amd import dense

    R, piv, rank = dense.rref(A.astype(dtype), bar_col=bar, tol=tol, pivot_rule=rule, dtype=dtype)
    return R, piv, rank, la.default_handle().get_option("rref_first_used")


def _rref_device(dev, A, bar, rule, tol):
    import torch

    dR = torch.from_numpy(np.ascontiguousarray(A, dtype=np.float64)).cuda()
    dpiv, drank = dev.rref_(dR, bar_col=bar, tol=tol, pivot_rule=rule)
    torch.cuda.synchronize()
    rank = int(drank.item())
    p = dpiv.cpu().numpy()
    return dR.cpu().numpy(), [(int(p[2 * i]), int(p[2 * i + 1])) for i in range(rank)], rank, dev.h.get_option("rref_first_used")


def _rref_entry_points(la, dev, dtype):
    pts = [("dense.rref", lambda A, bar, rule, tol: _rref_host(la, A, bar, dtype, rule, tol), la.default_handle())]
    if np.dtype(dtype) == np.float64:
        pts.append(("rref_", lambda A, bar, rule, tol: _rref_device(dev, A, bar, rule, tol), dev.h))
    return pts


def _with_blocked(handle, value, fn):
    try:
        handle.set_option("rref_blocked", value)
        return fn()
    finally:
        handle.set_option("rref_blocked", 1)


def _rref_paths(la, dev, case, rule, dtype):
    """(label, run, path) for every entry point and both values of rref_blocked that change the path."""
    default_path = pr.path_of(case, rule, dtype)
    for name, run, handle in _rref_entry_points(la, dev, dtype):
        for blocked in ((1,) if default_path == "per-column" else (1, 0)):
            path = default_path if blocked else "per-column"
            yield (f"{sc.name(dtype)} {pr.RULE_NAME[rule]} path={path} {name}",
                   lambda A, bar, tol, run=run, handle=handle, blocked=blocked: _with_blocked(handle, blocked, lambda: run(A, bar, rule, tol)),
                   path)


EXPLICIT_TOL = 0.5    # below every planted pivot candidate (>= 1), above every entry that must count as zero (0)


@pytest.mark.parametrize("rule", (pr.FIRST, pr.MAX), ids=lambda r: pr.RULE_NAME[r])
@pytest.mark.parametrize("case", sc.rref_cases(), ids=lambda c: c["id"])
def test_uniformly_scaled_planted_echelon_forms(la, dev, case, rule):
    A, L, E, S, perm = pr.build(case, rule)
    bar = case["bar"]
    answer = pr.planted_answer(L, E, S, bar)
    for dtype in pr.dtypes_of(case):
        for label, run, path in _rref_paths(la, dev, case, rule, dtype):
            for tol in (-1.0, EXPLICIT_TOL):
                R0, piv0, rank0, used0 = run(A, bar, tol)
                pr.verify(f"{case['id']} {label} tol={tol} unit", dtype, A, bar, answer, R0, piv0, rank0, check_low=rule == pr.FIRST)
                for s in sc.rref_exponents(dtype):
                    As = sc.scale(A.astype(dtype), s).astype(np.float64)
                    R, piv, rank, used = run(As, bar, tol if tol < 0 else float(np.ldexp(tol, s)))
                    want = sc.rref_expected(R0, rank0, s)
                    print(f"SCALED RREF {case['id']} {label} tol={tol} 2^{s}: rank {rank} ({rank0}), entries differing "
                          f"{int(np.count_nonzero(R != want))}")
                    assert rank == rank0 and piv == piv0, f"{label} 2^{s}"
                    if rule == pr.FIRST and np.dtype(dtype) == np.float64:
                        assert used == used0 == (1 if path == "first-fast" else 0), label
                    assert np.array_equal(R, want), f"{label} tol={tol} 2^{s}"


@pytest.mark.parametrize("dtype", DTYPES, ids=sc.name)
@pytest.mark.parametrize("rule", (pr.FIRST, pr.MAX), ids=lambda r: pr.RULE_NAME[r])
@pytest.mark.parametrize("n", sc.RREF_TOL_ORDERS)
def test_scaled_entry_equal_to_the_scaled_tolerance_counts_as_zero(la, dev, n, rule, dtype):
    Z = tuple(sorted(set(pr.spread(0, n, n // 5, 9) + ((n - 1,) if n == 300 else ()))))
    A, keep, _ = pr.tolerance_matrix(n, sc.RREF_TOL, Z, dtype)
    want = np.zeros((n, n), dtype=dtype)
    want[np.arange(len(keep)), keep] = 1
    want_piv = [(k, int(c)) for k, c in enumerate(keep)]
    case = dict(m=n, bar=n)
    for s in sc.rref_exponents(dtype):
        As = sc.scale(A, s).astype(np.float64)
        tol = float(np.ldexp(sc.RREF_TOL, s))
        for label, run, path in _rref_paths(la, dev, case, rule, dtype):
            R, piv, rank, _ = run(As, n, tol)
            print(f"SCALED TOL n={n} {label} 2^{s}: rank {rank} (expected {len(keep)}), entries differing {int(np.count_nonzero(R != want))}")
            assert rank == len(keep) and piv == want_piv, f"{label} 2^{s}"
            assert np.array_equal(R, want), f"{label} 2^{s}"


def test_traced_reduction_of_a_scaled_matrix(la):
    from linalg_solver_amd import dense

    m, n, bar = sc.TRACE_SHAPE
    A = sc.trace_matrix()
    R0, piv0, steps0, mask0, _, _ = dense.rref_trace(A, bar_col=bar)
    assert len(piv0) == m and not mask0.any()
    for s in sc.TRACE_EXP:
        R, piv, steps, mask, _, _ = dense.rref_trace(sc.scale(A, s), bar_col=bar)
        assert piv == piv0 and steps == steps0 and not mask.any()
        assert np.array_equal(R, R0), f"2^{s}"


# ------------------------------------------------------------------------------------------------ F
@pytest.mark.parametrize("dtype", DTYPES, ids=sc.name)
@pytest.mark.parametrize("panel", sc.SUBNORMAL_PANELS)
@pytest.mark.parametrize("n", sc.SUBNORMAL_ORDERS)
def test_subnormal_pivots_give_the_scaled_planted_factors(la, dev, n, panel, dtype):
    """Every pivot subnormal (2^-130 / 2^-1030), and at order 300 one subnormal pivot in the second panel: the
    reciprocal of such a pivot is not a finite number, LAPACK's getf2 divides by it."""
    A, _, _, _, want_piv = sc.planted(n)
    cases = [("all", np.full(n, sc.SUBNORMAL_EXP[sc.name(dtype)], dtype=np.int64))]
    if n > sc.ONE_SUBNORMAL_COLUMN:
        cases.append(("one", sc.one_subnormal_exponents(dtype, n)))
    handles = (la.default_handle(), dev.h)
    try:
        _set(handles, panel=panel)
        for what, d in cases:
            As = sc.scale_columns(A, d, dtype)
            want = sc.planted_lu_scaled(n, d).astype(dtype)
            dLU, dpiv, dinfo = _factor_dev(dev, As)
            results = (("lu_factor",) + tuple(_factor_host(As, dtype)),
                       ("getrf_", dLU.cpu().numpy(), dpiv.cpu().numpy()[:n], dinfo))
            for name, LU, ipiv, info in results:
                label = f"SUBNORMAL {sc.name(dtype)} n={n} panel={panel} {what} {name}"
                print(f"{label}: info {info}, finite {bool(np.all(np.isfinite(LU)))}, pivots differing {int(np.count_nonzero(ipiv != want_piv))}, "
                      f"entries differing {int(np.count_nonzero(LU != want))}")
                assert info == 0, label
                assert np.array_equal(ipiv, want_piv), label
                assert np.all(np.isfinite(LU)), label
                assert np.array_equal(LU, want), label
    finally:
        _restore(handles)


def test_subnormal_pivots_in_the_blocked_row_reduction(la, dev):
    case = pr.case_by_id(sc.RREF_SUBNORMAL_CASE_ID)
    bar = case["bar"]
    A, L, E, S, perm = pr.build(case, pr.MAX)
    answer = pr.planted_answer(L, E, S, bar)
    assert pr.path_of(case, pr.MAX, np.float64) == "blocked"
    for dtype in pr.dtypes_of(case):
        s = sc.SUBNORMAL_EXP[sc.name(dtype)]
        for name, run, handle in _rref_entry_points(la, dev, dtype):
            R0, piv0, rank0, _ = run(A, bar, pr.MAX, -1.0)
            pr.verify(f"{case['id']} {sc.name(dtype)} {name} unit", dtype, A, bar, answer, R0, piv0, rank0, check_low=False)
            R, piv, rank, _ = run(sc.scale(A.astype(dtype), s).astype(np.float64), bar, pr.MAX, -1.0)
            want = sc.rref_expected(R0, rank0, s)
            print(f"SUBNORMAL RREF {sc.name(dtype)} {name} 2^{s}: rank {rank} ({rank0}), finite {bool(np.all(np.isfinite(R)))}, "
                  f"entries differing {int(np.count_nonzero(R != want))}")
            assert rank == rank0 and piv == piv0
            assert np.array_equal(R, want)


# ------------------------------------------------------------------------------------------------ G
@pytest.mark.parametrize("s", sc.GRADED_EXP)
def test_matrix_surface_solves_a_graded_system_at_any_scale(la, s):
    """Pivot ratio about 1e-10, far above n eps: a solution, not NoSolution, at 2^-1010 (largest entry below 1e-300)
    and at 2^+1000 -- through host arrays and through device tensors."""
    import torch

    A, B, X0 = sc.graded_system()
    As, Bs = sc.scale(A, s), sc.scale(B, s)
    M = la.Matrix
    X = M.from_numpy(A).solve_array(B)
    inv = M.from_numpy(A).inverse_array()
    assert not isinstance(X, M.NoSolution) and not isinstance(inv, M.NoSolution)
    assert np.array_equal(X, X0), "the planted system is solved exactly at unit scale"
    Xb0, ferr0, berr0 = M.from_numpy(A).solve_array(B, bounds=True)
    assert np.array_equal(Xb0, X0) and np.all(np.isfinite(ferr0)) and np.all(np.isfinite(berr0))
    assert np.array_equal(np.array(M.from_numpy(A).inverse().items), inv), "inverse() and inverse_array() at unit scale"
    with np.errstate(over="ignore"):
        want_inv = np.ldexp(inv, -s)      # entries of the inverse reach 2^31: times 2^1010 some of them overflow
    cuda = lambda V: torch.from_numpy(V).cuda()   # noqa: E731
    for name, mk, arr in (("from_numpy", lambda V: M.from_numpy(V), lambda V: V),
                          ("from_dlpack", lambda V: M.from_dlpack(cuda(V)), lambda V: V if isinstance(V, M.NoSolution) else V.cpu().numpy())):
        Xs = arr(mk(As).solve_array(Bs if name == "from_numpy" else cuda(Bs)))
        invs = arr(mk(As).inverse_array())
        print(f"GRADED {name} 2^{s}: solve_array {'NoSolution' if isinstance(Xs, M.NoSolution) else 'solved'}, "
              f"inverse_array {'NoSolution' if isinstance(invs, M.NoSolution) else 'inverted'}")
        assert not isinstance(Xs, M.NoSolution), f"{name}: solve_array"
        assert not isinstance(invs, M.NoSolution), f"{name}: inverse_array"
        assert np.array_equal(Xs, X), f"{name}: solve_array differs in {int(np.count_nonzero(Xs != X))} entries"
        assert np.array_equal(invs, want_inv), f"{name}: inverse_array differs in {int(np.count_nonzero(invs != want_inv))} entries"
        got = mk(As).solve_array(Bs if name == "from_numpy" else cuda(Bs), bounds=True)
        assert not isinstance(got, M.NoSolution), f"{name}: solve_array(bounds=True)"
        Xb, ferr, berr = arr(got[0]), np.asarray(got[1]), np.asarray(got[2])
        print(f"GRADED {name} 2^{s} bounds=True: ferr {ferr} ({ferr0}), berr {berr} ({berr0})")
        assert np.array_equal(Xb, Xb0), f"{name}: solve_array(bounds=True) differs in {int(np.count_nonzero(Xb != Xb0))} entries"
        assert np.all(np.isfinite(ferr)) and np.all(np.isfinite(berr)), f"{name}: bounds"
        got = mk(As).inverse()          # the list-valued form
        assert not isinstance(got, M.NoSolution), f"{name}: inverse"
        assert np.array_equal(np.array(got.items), want_inv), f"{name}: inverse"
