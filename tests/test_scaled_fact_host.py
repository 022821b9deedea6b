"""CPU proof of tests/scaled_fact.py: the reference arithmetic alone -- the numpy models of the Cholesky family
(cpu_chol, cpu_potri, cpu_posx) and of Householder QR (cpu_qr), and LAPACK's potrf -- satisfies every relation that
tests/test_gpu_scaled_fact.py asserts of the library, bit for bit, for the same inputs, orders and exponents, and every
input and result is a normal number or zero.  So a failure on the GPU is the library's, not the relation's, and an
exponent at which the reference itself left the relation would show here (none of the tables needed narrowing below
what scaled_fact.py derives).  No tolerance appears anywhere.
"""
import functools

import numpy as np
import pytest
from scipy.linalg import lapack

import cpu_chol as cc
import cpu_posx as cp
import cpu_potri as cpi
import cpu_qr as cq
import scaled_fact as sf

DTYPES = list(sf.DTYPES)
SOURCES = ("planted", "rounded")


def _p(dtype):
    return "d" if np.dtype(dtype) == np.float64 else "s"


def _exact_scaling(As, A, e):
    """As is A times 2^e entry by entry, exactly, and normal or zero in its type."""
    return np.array_equal(As.astype(np.float64), np.ldexp(A.astype(np.float64), e)) and sf.normal_or_zero(As, As.dtype)


@functools.lru_cache(maxsize=None)
def _chol_unit(source, n, dname):
    A = sf.chol_matrix(source, n, np.dtype(dname).type)
    R, info = cc.potrf(A)
    assert info == 0
    for a in (A, R):
        a.setflags(write=False)
    return A, R


# ------------------------------------------------------------------------------------------------ potrf, potrs, podet
@pytest.mark.parametrize("dtype", DTYPES, ids=sf.name)
@pytest.mark.parametrize("kind", sf.CHOL_KINDS)
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("n", sf.CHOL_ORDERS)
def test_potrf_potrs_podet(n, source, kind, dtype):
    A, R0 = _chol_unit(source, n, sf.name(dtype))
    d = sf.exponents(sf.CHOL_EXP, dtype, kind, n)
    d32 = d.astype(np.int32)
    As = sf.scale_sym(A, d)
    assert As.dtype == np.dtype(dtype) and _exact_scaling(As, A, d32[:, None] + d32[None, :])
    R, info = cc.potrf(As)
    want = sf.upper_scaled(R0, d)
    assert info == 0 and np.array_equal(np.triu(R), np.triu(want)) and sf.normal_or_zero(np.triu(R), dtype)
    if source == "planted":
        assert np.array_equal(np.triu(R), sf.scale_cols(cc.planted(n, dtype=dtype)[0], d)), "the planted factor times D"
    # LAPACK's potrf keeps the relation as well
    L0, i0 = getattr(lapack, _p(dtype) + "potrf")(np.array(A), lower=0)
    L1, i1 = getattr(lapack, _p(dtype) + "potrf")(As, lower=0)
    assert i0 == 0 and i1 == 0 and np.array_equal(np.triu(L1), np.triu(sf.upper_scaled(L0, d)))
    # podet: mantissas unchanged, exponents up by d
    m0, e0 = np.frexp(np.diagonal(R0))
    m1, e1 = np.frexp(np.diagonal(R))
    assert np.array_equal(m0, m1) and np.array_equal(e1 - e0, d)
    if source == "planted":
        sign, mant, exp2 = sf.podet_expected(n, d)
        assert np.all(m1 == 0.5) and (sign, mant, exp2) == (1.0, 0.5, 1 + 2 * int(np.sum(e1 - 1)))
    t = sf.rhs_exponent(dtype, kind, sf.CHOL_EXP)
    for nrhs in sf.CHOL_NRHS:
        B = sf.chol_rhs(source, n, nrhs, dtype)
        Bs = sf.scale_rows(B, d, t)
        assert _exact_scaling(Bs, B, d32[:, None] + t)
        for solve in (cc.potrs, cp.potrs_few):
            X0 = solve(np.triu(R0), B)
            Xs = solve(np.triu(R), Bs)
            assert np.array_equal(Xs, sf.scale_rows(X0, -d, t)) and sf.normal_or_zero(Xs, dtype), (nrhs, solve.__name__)


# ------------------------------------------------------------------------------------------------ potri
@pytest.mark.parametrize("dtype", DTYPES, ids=sf.name)
@pytest.mark.parametrize("kind", sf.CHOL_INV_KINDS)
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("n", sf.CHOL_ORDERS)
def test_potri(n, source, kind, dtype):
    A, R0 = _chol_unit(source, n, sf.name(dtype))
    d = sf.exponents(sf.CHOL_INV_EXP, dtype, kind, n)
    R, info = cc.potrf(sf.scale_sym(A, d))
    assert info == 0 and np.array_equal(np.triu(R), np.triu(sf.upper_scaled(R0, d)))
    P0, i0 = cpi.potri(np.array(R0))
    P, i1 = cpi.potri(R)
    assert i0 == 0 and i1 == 0
    assert np.array_equal(np.triu(P), np.triu(sf.scale_sym(P0, -d))) and sf.normal_or_zero(np.triu(P), dtype)


# ------------------------------------------------------------------------------------------------ lansy, pocon, porfs
@pytest.mark.parametrize("dtype", DTYPES, ids=sf.name)
@pytest.mark.parametrize("kind", sf.UNIFORM_KINDS)
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("n", sf.CHOL_ORDERS)
def test_norm_condition_estimate_and_refinement_of_a_uniformly_scaled_matrix(n, source, kind, dtype):
    A, R0 = _chol_unit(source, n, sf.name(dtype))
    d = sf.exponents(sf.CHOL_INV_EXP, dtype, kind, n)
    s = int(d[0])
    As = sf.scale_sym(A, d)
    R, info = cc.potrf(As)
    assert info == 0 and np.array_equal(np.triu(R), np.triu(sf.upper_scaled(R0, d)))
    an0, an = cp.lansy(np.array(A)), cp.lansy(As)
    assert an == float(np.ldexp(an0, 2 * s))
    c0, c1 = [], []
    rc0, rc = cp.pocon_twin(np.triu(R0), an0, c0), cp.pocon_twin(np.triu(R), an, c1)
    assert 0 < rc0 < 1 and rc == rc0 and c0 == c1
    t = sf.rhs_exponent(dtype, kind, sf.CHOL_INV_EXP)
    B = sf.chol_rhs(source, n, 3, dtype)
    X0 = sf.refine_start(cc.potrs(np.triu(R0), B))
    Bs, X0s = sf.scale_rows(B, d, t), sf.scale_rows(X0, -d, t)
    for j in range(B.shape[1]):
        st0, so0, st1, so1 = [], [], [], []
        x, ferr, berr = cp.porfs_twin(np.array(A), np.triu(R0), B[:, j], X0[:, j], st0, so0)
        xs, ferrs, berrs = cp.porfs_twin(As, np.triu(R), Bs[:, j], X0s[:, j], st1, so1)
        assert st0[0] >= 1, "the perturbed start is refined"
        assert np.array_equal(xs, sf.scale_rows(x, -d, t)) and ferrs == ferr and berrs == berr and st0 == st1 and so0 == so1


# ------------------------------------------------------------------------------------------------ not positive definite
@pytest.mark.parametrize("dtype", DTYPES, ids=sf.name)
@pytest.mark.parametrize("kind", sf.CHOL_KINDS)
@pytest.mark.parametrize("n,j,what", sf.NOT_PD)
def test_not_positive_definite_at_scale(n, j, what, kind, dtype):
    U, A = cc.planted_not_pd(n, j, what, dtype=dtype)
    d = sf.exponents(sf.CHOL_EXP, dtype, kind, n)
    As = sf.scale_sym(A, d)
    with np.errstate(all="ignore"):        # what lies after the failing pivot is unspecified, and may overflow
        R0, i0 = cc.potrf(A)
        R, i1 = cc.potrf(As)
    assert i0 == i1 == j + 1
    assert np.array_equal(np.triu(R)[:j, :j], sf.scale_cols(U, d)[:j, :j]), "the rows before the failing pivot: U D"
    assert np.array_equal(np.triu(R)[:j, :j], np.triu(sf.upper_scaled(R0, d))[:j, :j])
    _, li = getattr(lapack, _p(dtype) + "potrf")(As, lower=0)
    assert li == j + 1


# ------------------------------------------------------------------------------------------------ QR
@functools.lru_cache(maxsize=None)
def _qr_unit(source, dname):
    dtype = np.dtype(dname).type
    A, B, x0 = sf.qr_case(source, dtype)
    QR, tau, Bo, info = cq.gels(A, B)
    for a in (A, B, QR, tau, Bo):
        a.setflags(write=False)
    return A, B, x0, QR, tau, Bo, info


@pytest.mark.parametrize("dtype", DTYPES, ids=sf.name)
@pytest.mark.parametrize("kind", sf.QR_KINDS)
@pytest.mark.parametrize("source", sf.QR_SOURCES)
def test_geqrf_ormqr_orgqr_gels(source, kind, dtype):
    A, B, x0, QR0, tau0, Bo0, info0 = _qr_unit(source, sf.name(dtype))
    m, n = A.shape
    d = sf.exponents(sf.QR_EXP, dtype, kind, n)
    r, t = sf.R_ROWS, sf.T_RHS
    As = sf.qr_scaled_input(A, d, dtype)
    assert As.dtype == np.dtype(dtype) and _exact_scaling(As, A, d.astype(np.int32)[None, :] + r)
    if kind in sf.UNIFORM_KINDS and dtype == np.float32:
        sq = float(np.abs(As).max()) ** 2
        assert sq > float(np.finfo(np.float32).max) or sq < float(np.finfo(np.float32).tiny), \
            "the square of an entry is outside the fp32 range: a Gram sum formed in fp32 would fail here"
    Bs = np.ldexp(np.array(B), t)
    QR, tau, Bo, info = cq.gels(As, Bs)
    assert info == info0 == 0
    assert np.array_equal(tau, tau0) and np.array_equal(np.tril(QR, -1), np.tril(QR0, -1))
    assert np.array_equal(QR, sf.upper_scaled(QR0, d, r)) and sf.normal_or_zero(QR, dtype)
    assert np.array_equal(Bo, sf.gels_expected(Bo0, n, d)) and sf.normal_or_zero(Bo, dtype)
    nrm0 = np.sqrt((Bo0[n:].astype(np.float64) ** 2).sum(axis=0))
    assert np.array_equal(np.sqrt((Bo[n:].astype(np.float64) ** 2).sum(axis=0)), np.ldexp(nrm0, t))
    if x0 is not None:
        assert np.array_equal(Bo0[:n], x0), "the planted solution at unit scale"
        assert np.array_equal(Bo[:n], sf.scale_rows(x0, -d, t - r))
    assert np.array_equal(cq.orgqr(QR, tau), cq.orgqr(np.array(QR0), np.array(tau0)))
    for trans in (True, False):
        W0 = cq.ormqr(np.array(QR0), np.array(tau0), B, trans)
        assert np.array_equal(cq.ormqr(QR, tau, Bs, trans), np.ldexp(W0, t))


@pytest.mark.parametrize("dtype", DTYPES, ids=sf.name)
@pytest.mark.parametrize("kind", sf.QR_KINDS)
@pytest.mark.parametrize("j", sf.QR_ZERO_COLUMNS)
def test_zero_column_at_scale(j, kind, dtype):
    m, n = sf.QR_SHAPE
    _, A, _ = cq.planted_zero_column(m, n, j, dtype=dtype)
    d = sf.exponents(sf.QR_EXP, dtype, kind, n)
    QR0, tau0 = cq.geqrf(A)
    QR, tau = cq.geqrf(sf.qr_scaled_input(A, d, dtype))
    assert cq.diag_info(QR0[:n]) == cq.diag_info(QR[:n]) == j + 1 and tau[j] == 0 and QR[j, j] == 0
    assert np.array_equal(tau, tau0) and np.array_equal(QR, sf.upper_scaled(QR0, d, sf.R_ROWS))


def test_every_routine_keeps_a_down_an_up_and_a_mixed_case():
    for kinds in (sf.CHOL_KINDS, sf.CHOL_INV_KINDS, sf.QR_KINDS):
        assert {"down", "up", "mixed"} <= set(kinds)
    assert set(sf.UNIFORM_KINDS) == {"down", "up"}
    for table in (sf.CHOL_EXP, sf.CHOL_INV_EXP, sf.QR_EXP):
        for e in table.values():
            assert e["down"] < 0 < e["up"] and e["mixed"][0] < 0 < e["mixed"][1]
    assert sf.QR_EXP["float32"]["down"] < -64 and sf.QR_EXP["float32"]["up"] > 64
