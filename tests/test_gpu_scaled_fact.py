"""Power-of-two scaling as an exact symmetry of the Cholesky family and of Householder QR on the MI355X
(tests/scaled_fact.py states the relations and derives the exponent tables; tests/test_scaled_fact_host.py proves them
of the numpy models and LAPACK alone).  Every comparison is the library at scale against the library at unit scale
after np.ldexp, bit for bit; where a planted answer is known in advance, against that as well.  No tolerance appears.

Cholesky, A' = D A D with the strictly lower triangle NaN-filled: potrf (device-pointer and host-buffer form), potrs
through the few-column path and the block sweeps, podet, potri; for a uniform D also lansy, pocon (rcond and the
number of solves) and porfs (X, ferr, berr, steps, solves); a zero and a negative pivot report the same info at scale.
QR, A' = 2^r A D: geqrf (both forms), orgqr, ormqr of 2^t C for both trans, gels and col_norms with B' = 2^t B, the
zero column's info.  The fp32 cases at 2^-80 and 2^+70 put the square of every entry outside the fp32 range: a Gram
sum, alpha^2 + g or a column norm formed in fp32 fails there, as does tau v w formed in an order that overflows.
"""
import numpy as np
import pytest

import cpu_chol as cc
import cpu_qr as cq
import scaled_fact as sf

pytestmark = pytest.mark.gpu

DTYPES = list(sf.DTYPES)
SOURCES = ("planted", "rounded")
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    import torch

    from linalg_solver_amd.device import DeviceSolver

    assert torch.cuda.is_available()
    return DeviceSolver()


def _t(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _lower_untouched(R, A):
    lo = np.tril_indices(A.shape[0], -1)
    return np.array_equal(_bits(R)[lo], _bits(A)[lo])


def _potrf(dev, A):
    """potrf_ on a device copy of A with its strictly lower triangle NaN-filled: (device factor, numpy factor, info)."""
    Ain = cc.fill_lower(A, NAN)
    t = _t(Ain)
    info = int(dev.potrf_(t).item())
    R = t.cpu().numpy()
    assert _lower_untouched(R, Ain)
    return t, R, info


def _upper_same(R, want):
    """The upper triangles hold the same bits."""
    up = np.triu_indices(R.shape[0])
    return np.array_equal(_bits(R)[up], _bits(np.ascontiguousarray(want))[up])


# ------------------------------------------------------------------------------------------------ potrf, potrs, podet
@pytest.mark.parametrize("dtype", DTYPES, ids=sf.name)
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("n", sf.CHOL_ORDERS)
def test_potrf_potrs_podet(dev, n, source, dtype):
    from linalg_solver_amd import dense

    A = sf.chol_matrix(source, n, dtype)
    tR0, R0, info0 = _potrf(dev, A)
    assert info0 == 0
    det0 = dev.podet_parts(tR0).cpu().numpy()
    if source == "planted":
        assert np.array_equal(np.triu(R0), cc.planted(n, dtype=dtype)[0])
    for kind in sf.CHOL_KINDS:
        d = sf.exponents(sf.CHOL_EXP, dtype, kind, n)
        As = sf.scale_sym(A, d)
        tR, R, info = _potrf(dev, As)
        print(f"SCALED potrf {sf.name(dtype)} n={n} {source} {kind}: info {info}, entries differing "
              f"{int(np.count_nonzero(np.triu(R) != np.triu(sf.upper_scaled(R0, d))))}")
        assert info == 0 and _upper_same(R, sf.upper_scaled(R0, d)), kind
        if source == "planted":
            assert np.array_equal(np.triu(R), sf.scale_cols(cc.planted(n, dtype=dtype)[0], d)), "the planted factor times D"
        Uh, hinfo = dense.cho_factor(cc.fill_lower(As, NAN), dtype=dtype, handle=dev.h)
        assert hinfo == 0 and _upper_same(Uh, R), f"{kind}: host-buffer form"
        det = dev.podet_parts(tR).cpu().numpy()
        assert det[0] == det0[0] == 1.0 and det[1] == det0[1] and det[2] == det0[2] + 2 * int(d.sum()), (kind, det, det0)
        if source == "planted":
            assert tuple(float(v) for v in det) == tuple(float(v) for v in sf.podet_expected(n, d))
        t = sf.rhs_exponent(dtype, kind, sf.CHOL_EXP)
        for nrhs in sf.CHOL_NRHS:
            B = sf.chol_rhs(source, n, nrhs, dtype)
            X0 = dev.potrs_(tR0, _t(B)).cpu().numpy()
            Xs = dev.potrs_(tR, _t(sf.scale_rows(B, d, t))).cpu().numpy()
            assert np.all(np.isfinite(X0)) and _same_bits(Xs, sf.scale_rows(X0, -d, t)), f"potrs {kind} nrhs={nrhs}"
            assert _same_bits(dense.cho_solve(R, sf.scale_rows(B, d, t), handle=dev.h), Xs), f"cho_solve {kind} nrhs={nrhs}"


# ------------------------------------------------------------------------------------------------ potri
@pytest.mark.parametrize("dtype", DTYPES, ids=sf.name)
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("n", sf.CHOL_ORDERS)
def test_potri(dev, n, source, dtype):
    A = sf.chol_matrix(source, n, dtype)
    tP0, R0, info0 = _potrf(dev, A)
    assert info0 == 0 and int(dev.potri_(tP0).item()) == 0
    P0 = tP0.cpu().numpy()
    assert np.all(np.isfinite(np.triu(P0))) and _lower_untouched(P0, R0)
    for kind in sf.CHOL_INV_KINDS:
        d = sf.exponents(sf.CHOL_INV_EXP, dtype, kind, n)
        tP, R, info = _potrf(dev, sf.scale_sym(A, d))
        assert info == 0 and _upper_same(R, sf.upper_scaled(R0, d)), kind
        assert int(dev.potri_(tP).item()) == 0
        P = tP.cpu().numpy()
        print(f"SCALED potri {sf.name(dtype)} n={n} {source} {kind}: entries differing "
              f"{int(np.count_nonzero(np.triu(P) != np.triu(sf.scale_sym(np.triu(P0), -d))))}")
        assert _upper_same(P, sf.scale_sym(np.triu(P0), -d)) and _lower_untouched(P, R), kind


# ------------------------------------------------------------------------------------------------ lansy, pocon, porfs
@pytest.mark.parametrize("dtype", DTYPES, ids=sf.name)
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("n", sf.CHOL_ORDERS)
def test_norm_condition_estimate_and_refinement_of_a_uniformly_scaled_matrix(dev, n, source, dtype):
    A = sf.chol_matrix(source, n, dtype)
    B = sf.chol_rhs(source, n, 3, dtype)

    def run(As, Bs, scale_x):
        tA = _t(cc.fill_lower(As, NAN))
        anorm = float(dev.norm_sym(tA).item())
        tU, U, info = _potrf(dev, As)
        assert info == 0
        rc = dev.pocon(tU, anorm)
        csolves = dev.h.get_option("pocon_solves")
        tX = _t(scale_x(sf.refine_start(start)))
        ferr, berr = dev.porfs_(tA, tU, _t(Bs), tX)
        return anorm, rc, csolves, tX.cpu().numpy(), ferr, berr, dev.h.get_option("porfs_steps"), dev.h.get_option("porfs_solves")

    tU0, _, info0 = _potrf(dev, A)
    assert info0 == 0
    start = dev.potrs_(tU0, _t(B)).cpu().numpy()
    an0, rc0, cs0, X0, ferr0, berr0, steps0, solves0 = run(A, B, lambda X: X)
    assert 0 < rc0 < 1 and cs0 >= 1 and steps0 >= 1 and np.all(np.isfinite(X0)) and np.all(np.isfinite(ferr0))
    for kind in sf.UNIFORM_KINDS:
        d = sf.exponents(sf.CHOL_INV_EXP, dtype, kind, n)
        s, t = int(d[0]), sf.rhs_exponent(dtype, kind, sf.CHOL_INV_EXP)
        an, rc, cs, X, ferr, berr, steps, solves = run(sf.scale_sym(A, d), sf.scale_rows(B, d, t), lambda X: sf.scale_rows(X, -d, t))
        print(f"SCALED {sf.name(dtype)} n={n} {source} 2^{s}: norm {an!r} ({an0!r}), rcond {rc!r} ({rc0!r}), solves {cs} ({cs0}), "
              f"ferr {ferr} ({ferr0}), berr {berr} ({berr0}), steps {steps} ({steps0}), solves {solves} ({solves0})")
        assert an == float(np.ldexp(an0, 2 * s))
        assert rc == rc0 and cs == cs0
        assert _same_bits(X, sf.scale_rows(X0, -d, t))
        assert np.array_equal(ferr, ferr0) and np.array_equal(berr, berr0) and steps == steps0 and solves == solves0


# ------------------------------------------------------------------------------------------------ not positive definite
@pytest.mark.parametrize("dtype", DTYPES, ids=sf.name)
@pytest.mark.parametrize("n,j,what", sf.NOT_PD)
def test_not_positive_definite_at_scale(dev, n, j, what, dtype):
    U, A = cc.planted_not_pd(n, j, what, dtype=dtype)
    _, R0, info0 = _potrf(dev, A)
    assert info0 == j + 1 and np.array_equal(np.triu(R0)[:j, :j], U[:j, :j])
    for kind in sf.CHOL_KINDS:
        d = sf.exponents(sf.CHOL_EXP, dtype, kind, n)
        _, R, info = _potrf(dev, sf.scale_sym(A, d))
        assert info == j + 1, kind
        assert np.array_equal(np.triu(R)[:j, :j], sf.scale_cols(U, d)[:j, :j]), f"{kind}: the rows before the failing pivot"


# ------------------------------------------------------------------------------------------------ QR
def _gels(dev, A, B):
    import torch

    ta, tb = _t(A), _t(B)
    tau, info = dev.gels_(ta, tb)
    n = A.shape[1]
    res = dev.col_norms(tb[n:])
    torch.cuda.synchronize()
    return ta.cpu().numpy(), tau.cpu().numpy()[:n], tb.cpu().numpy(), int(info.item()), res.cpu().numpy()


def _ormqr(dev, QR, tau, Cm, trans):
    tc = _t(Cm)
    dev.ormqr_(_t(QR), _t(tau), tc, trans=trans)
    return tc.cpu().numpy()


@pytest.mark.parametrize("dtype", DTYPES, ids=sf.name)
@pytest.mark.parametrize("source", sf.QR_SOURCES)
def test_geqrf_ormqr_orgqr_gels(dev, source, dtype):
    from linalg_solver_amd import dense

    A, B, x0 = sf.qr_case(source, dtype)
    m, n = A.shape
    r, t = sf.R_ROWS, sf.T_RHS
    QR0, tau0, Bo0, info0, res0 = _gels(dev, A, B)
    assert info0 == 0 and np.all(np.isfinite(QR0)) and np.all(np.isfinite(Bo0))
    if x0 is not None:
        assert np.array_equal(Bo0[:n], x0), "the planted solution at unit scale"
    Q0 = dev.orgqr(_t(QR0), _t(tau0)).cpu().numpy()
    W0 = {trans: _ormqr(dev, QR0, tau0, B, trans) for trans in (True, False)}
    x_host0, resid0, hinfo0 = dense.lstsq(A, B, dtype=dtype, handle=dev.h)
    assert hinfo0 == 0
    for kind in sf.QR_KINDS:
        d = sf.exponents(sf.QR_EXP, dtype, kind, n)
        As, Bs = sf.qr_scaled_input(A, d, dtype), np.ldexp(B, t)
        QR, tau, Bo, info, res = _gels(dev, As, Bs)
        want = sf.upper_scaled(QR0, d, r)
        print(f"SCALED QR {sf.name(dtype)} {source} {kind}: info {info}, tau differing {int(np.count_nonzero(_bits(tau) != _bits(tau0)))}, "
              f"factor entries differing {int(np.count_nonzero(_bits(QR) != _bits(want)))}, "
              f"B entries differing {int(np.count_nonzero(_bits(Bo) != _bits(sf.gels_expected(Bo0, n, d))))}")
        assert info == 0, kind
        assert _same_bits(tau, tau0) and _same_bits(QR, want), f"{kind}: tau and V unchanged, R' = 2^r R D"
        assert _same_bits(Bo, sf.gels_expected(Bo0, n, d)), f"{kind}: X'[i] = X[i] 2^(t - r - d_i), the tail times 2^t"
        assert _same_bits(res, np.ldexp(res0, t)), f"{kind}: col_norms"
        if x0 is not None:
            assert np.array_equal(Bo[:n], sf.scale_rows(x0, -d, t - r)), f"{kind}: the planted solution, scaled"
        ta = _t(As)
        gt = dev.geqrf_(ta)
        assert _same_bits(ta.cpu().numpy(), QR) and _same_bits(gt.cpu().numpy()[:n], tau), f"{kind}: geqrf_ alone"
        H, ht = dense.qr_factor(As, dtype=dtype, handle=dev.h)
        assert _same_bits(H, QR) and _same_bits(ht, tau), f"{kind}: host-buffer form"
        assert _same_bits(dev.orgqr(_t(QR), _t(tau)).cpu().numpy(), Q0), f"{kind}: orgqr"
        for trans in (True, False):
            assert _same_bits(_ormqr(dev, QR, tau, Bs, trans), np.ldexp(W0[trans], t)), f"{kind}: ormqr trans={trans}"
        x, resid, hinfo = dense.lstsq(As, Bs, dtype=dtype, handle=dev.h)
        assert hinfo == 0 and _same_bits(x, sf.scale_rows(x_host0, -d, t - r)) and _same_bits(resid, np.ldexp(resid0, t)), f"{kind}: lstsq"


@pytest.mark.parametrize("dtype", DTYPES, ids=sf.name)
@pytest.mark.parametrize("j", sf.QR_ZERO_COLUMNS)
def test_zero_column_at_scale(dev, j, dtype):
    m, n = sf.QR_SHAPE
    _, A, _ = cq.planted_zero_column(m, n, j, dtype=dtype)
    B = np.random.default_rng(j).integers(-3, 4, (m, 3)).astype(dtype)
    QR0, tau0, _, info0, _ = _gels(dev, A, B)
    assert info0 == j + 1 and tau0[j] == 0 and QR0[j, j] == 0
    for kind in sf.QR_KINDS:
        d = sf.exponents(sf.QR_EXP, dtype, kind, n)
        QR, tau, _, info, _ = _gels(dev, sf.qr_scaled_input(A, d, dtype), np.ldexp(B, sf.T_RHS))
        assert info == j + 1, kind
        assert _same_bits(tau, tau0) and _same_bits(QR, sf.upper_scaled(QR0, d, sf.R_ROWS)), kind
