"""The handle's device buffers on a long-lived handle: one `DeviceSolver` walks the orders 129, 300, 520, 257, 129 --
its buffers grow, are then reused at smaller sizes, and are shared between the LU, Cholesky, refinement, equilibration
and row-reduction families -- and every output of every call is compared bit for bit with the same call on a
`DeviceSolver` created for that call alone and closed after it.  129 and 257 straddle the 128-row step, 520 takes the
structured inverse, and the 300 x 300 row reductions take the blocked forms.  Where a family has a device-pointer form
and a host-buffer form, both run.  fp64; inputs are the project's `gen` fills with fixed seeds.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ORDERS = (129, 300, 520, 257, 129)


def _t(a):
    import torch

    return torch.from_numpy(np.array(a, order="C")).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _flat(out):
    """Every array / scalar of a call's result, in order."""
    if isinstance(out, dict):
        return [x for k in sorted(out) for x in _flat(out[k])]
    if isinstance(out, (tuple, list)):
        return [x for o in out for x in _flat(o)]
    if hasattr(out, "detach"):
        return [_np(out)]
    return [np.asarray(out)]


def _same_bits(label, got, want):
    got, want = _flat(got), _flat(want)
    assert len(got) == len(want), label
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{label}: output {i} {g.dtype}{g.shape} vs {w.dtype}{w.shape}"
        assert g.tobytes() == w.tobytes(), f"{label}: output {i} differs from a fresh handle's"


def test_long_lived_handle_gives_a_fresh_handles_bits():
    import torch

    from linalg_solver_amd import _native as N
    from linalg_solver_amd import dense, gen
    from linalg_solver_amd.device import DeviceSolver

    assert torch.cuda.is_available()
    solver = DeviceSolver()

    def both(label, call):
        """call(s) on the long-lived solver and on one made for this call alone: same bits.  Returns the former's."""
        got = call(solver)
        fresh = DeviceSolver()
        try:
            want = call(fresh)
        finally:
            fresh.h.close()
        _same_bits(label, got, want)
        return got

    def with_option(key, value, call):
        def run(s):
            s.h.set_option(key, value)
            try:
                return call(s)
            finally:
                s.h.set_option(key, 0)
        return run

    for step, n in enumerate(ORDERS):
        tag = f"n={n} (step {step})"
        A = gen.fill(gen.U11, 11 + n, n, n)
        Bs = {k: gen.fill(gen.U11, 23 + n, n, k, col_off=gen.RHS_COL - 64) for k in (1, 2, 3, 9, 64)}
        anorm = float(np.abs(A).sum(axis=0).max())

        # ---- LU family
        def getrf_dev(s):
            LU = _t(A)
            ipiv, info = s.getrf_(LU)
            return LU, ipiv, info
        LU, ipiv, info = (_np(x) for x in both(f"getrf dev {tag}", getrf_dev))
        assert info[0] == 0
        LUh, ipivh, infoh = both(f"getrf host {tag}", lambda s: dense.lu_factor(A, handle=s.h))
        assert infoh == 0 and LUh.tobytes() == LU.tobytes() and np.array_equal(ipivh, ipiv[:n])

        X9 = None
        for trans, cols, path in ((False, (1, 9), None), (True, (1, 64), "getrs_t_path")):
            for k in cols:
                def solve_dev(s, k=k, trans=trans):
                    X = s.getrs_(_t(LU), _t(ipiv), _t(Bs[k]), trans=trans)
                    return X, (s.h.get_option(path) if path else 0)
                X, took = both(f"getrs{'_t' if trans else ''} dev nrhs={k} {tag}", solve_dev)
                if path:
                    assert took == (1 if k == 64 else 0), f"{tag}: nrhs={k} took the wrong transposed path"
                if not trans and k == 9:
                    X9 = _np(X)
                both(f"getrs{'_t' if trans else ''} host nrhs={k} {tag}",
                     lambda s, k=k, trans=trans: dense.lu_solve(LU, ipiv, Bs[k], handle=s.h, trans=trans))

        both(f"getri dev {tag}", lambda s: s.getri(_t(LU), _t(ipiv)))
        both(f"getri host {tag}", lambda s: dense.inv(A, handle=s.h))

        def gecon_dev(s):
            return s.rcond(_t(LU), _t(ipiv), anorm), s.h.get_option("gecon_solves")
        both(f"gecon dev {tag}", gecon_dev)
        both(f"gecon host {tag}", lambda s: (dense.lu_rcond(LU, ipiv, anorm, handle=s.h), s.h.get_option("gecon_solves")))

        def gerfs_dev(s):
            X = _t(X9)
            ferr, berr = s.gerfs_(_t(A), _t(LU), _t(ipiv), _t(Bs[9]), X)
            return X, ferr, berr, s.h.get_option("gerfs_steps"), s.h.get_option("gerfs_solves")
        both(f"gerfs dev {tag}", gerfs_dev)
        both(f"gerfs host {tag}", lambda s: (dense.lu_refine(A, LU, ipiv, Bs[9], X9, handle=s.h),
                                             s.h.get_option("gerfs_steps"), s.h.get_option("gerfs_solves")))

        # ---- Cholesky family: G G^T / n + 3 I
        S = A @ A.T / n + 3.0 * np.eye(n)
        S = (S + S.T) / 2
        snorm = float(np.abs(S).sum(axis=0).max())

        def potrf_dev(s):
            U = _t(S)
            info = s.potrf_(U)
            return U, info
        U, pinfo = (_np(x) for x in both(f"potrf dev {tag}", potrf_dev))
        assert pinfo[0] == 0
        U = np.triu(U)
        Uh, pinfoh = both(f"potrf host {tag}", lambda s: dense.cho_factor(S, handle=s.h))
        assert pinfoh == 0 and Uh.tobytes() == U.tobytes()

        Xp = None
        for few in (0, 8):
            def potrs_dev(s):
                X = s.potrs_(_t(U), _t(Bs[3]))
                return X, s.h.get_option("potrs_path")
            X, took = both(f"potrs dev potrs_few_max={few} {tag}", with_option("potrs_few_max", few, potrs_dev))
            assert took == (1 if few else 0), f"{tag}: potrs_few_max={few} took the wrong path"
            both(f"potrs host potrs_few_max={few} {tag}",
                 with_option("potrs_few_max", few, lambda s: dense.cho_solve(U, Bs[3], handle=s.h)))
        Xp = _np(both(f"potrs dev nrhs=9 {tag}", lambda s: s.potrs_(_t(U), _t(Bs[9]))))

        both(f"pocon dev {tag}", lambda s: (s.pocon(_t(U), snorm), s.h.get_option("pocon_solves")))
        both(f"pocon host {tag}", lambda s: (dense.cho_rcond(U, snorm, handle=s.h), s.h.get_option("pocon_solves")))

        def porfs_dev(s):
            X = _t(Xp)
            ferr, berr = s.porfs_(_t(S), _t(U), _t(Bs[9]), X)
            return X, ferr, berr, s.h.get_option("porfs_steps"), s.h.get_option("porfs_solves")
        both(f"porfs dev {tag}", porfs_dev)
        both(f"porfs host {tag}", lambda s: (dense.cho_refine(S, U, Bs[9], Xp, handle=s.h),
                                             s.h.get_option("porfs_steps"), s.h.get_option("porfs_solves")))

        # ---- expert driver on a matrix whose rows geequ has to scale
        Ar = A * np.ldexp(1.0, (np.arange(n) % 13) - 6)[:, None]
        def gesvx_dev(s):
            Ad, Bd = _t(Ar), _t(Bs[2])
            out = s.gesvx_(Ad, Bd, equilibrate=True)
            return out, Ad, Bd
        out = both(f"gesvx dev {tag}", gesvx_dev)[0]
        assert out["info"] == 0 and out["equed"] != N.EQUED_NONE
        both(f"gesvx host {tag}", lambda s: dense.solve_expert(Ar, Bs[2], equilibrate=True, handle=s.h))

        # ---- row reduction of a rank-150 integer matrix under both pivot rules (blocked forms: m * bar >= 256^2)
        if n == 300:
            P = gen.fill(gen.INT5, 5, n, 150) @ gen.fill(gen.INT5, 6, 150, n)
            for rule in (N.PIVOT_MAX, N.PIVOT_FIRST):
                def rref_dev(s, rule=rule):
                    R = _t(P)
                    piv, rank = s.rref_(R, bar_col=n, pivot_rule=rule)
                    return R, piv, rank, s.h.get_option("rref_first_used")
                R, piv, rank, used = both(f"rref dev rule={rule} {tag}", rref_dev)
                assert int(_np(rank)[0]) == 150
                assert used == (1 if rule == N.PIVOT_FIRST else 0), "the first-rule reduction did not take its blocked form"
                both(f"rref host rule={rule} {tag}", lambda s, rule=rule: dense.rref(P, bar_col=n, handle=s.h, pivot_rule=rule))

    solver.h.check_status()
    solver.h.close()
