"""CPU proofs behind tests/test_gpu_qr.py: for every shape and seed the GPU tests use, the numpy model of the QR
kernels (tests/cpu_qr.py) returns the planted factor exactly in both precisions and equals LAPACK (scipy) bit for bit,
and the solve through the block inverses returns the planted least-squares solution exactly.  On rounded inputs the
model's three LAPACK ratios are recorded beside LAPACK's own.
"""
import numpy as np
import pytest
from scipy.linalg import lapack

import cpu_qr as cq

DTYPES = [np.float64, np.float32]


def _p(dtype):
    return "d" if np.dtype(dtype) == np.float64 else "s"


def _lapack_geqrf(A):
    qr_, tau, _, info = getattr(lapack, _p(A.dtype) + "geqrf")(A)
    assert info == 0
    return np.ascontiguousarray(qr_), tau


def _lapack_ormqr(QR, tau, Cm, trans):
    k = len(tau)
    out, _, info = getattr(lapack, _p(QR.dtype) + "ormqr")("L", "T" if trans else "N", np.asfortranarray(QR[:, :k]), tau,
                                                          np.asfortranarray(Cm), max(1, Cm.shape[1]) * 128)
    assert info == 0
    return np.ascontiguousarray(out)


def _check_plant(U, QR, tau):
    n = U.shape[1]
    R = np.triu(QR[:n])
    d = np.diagonal(R)
    S = np.sign(d) * np.sign(np.diagonal(U))
    assert np.array_equal(R, S[:, None] * U), "R is the plant up to the sign of its rows"
    assert np.all((tau == 0) | (tau == 1))
    assert np.array_equal(d[tau == 1], -np.abs(np.diagonal(U))[tau == 1])
    assert np.array_equal(np.abs(d), np.abs(np.diagonal(U)))
    V = np.tril(QR, -1)
    assert np.all(np.isin(V, (-1, 0, 1)))
    assert np.array_equal(np.count_nonzero(V, axis=0), (tau == 1).astype(int)), "v = e_j +- e_k, or nothing"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n", cq.PLANTED_SHAPES)
def test_model_returns_the_plant_and_equals_lapack(m, n, dtype):
    U, A, _ = cq.planted(m, n, dtype=dtype)
    QR, tau = cq.geqrf(A)
    _check_plant(U, QR, tau)
    if n >= 127 and m > n:
        assert (tau == 0).any() and (tau == 1).any(), "both branches of the step are taken"
    Lq, Lt = _lapack_geqrf(A)
    assert np.array_equal(QR, Lq) and np.array_equal(tau, Lt)


@pytest.mark.parametrize("dtype", DTYPES)
def test_wide_plant(dtype):
    A = cq.planted_wide(dtype=dtype)
    QR, tau = cq.geqrf(A)
    Lq, Lt = _lapack_geqrf(A)
    assert np.array_equal(QR, Lq) and np.array_equal(tau, Lt)
    assert np.array_equal(QR, np.round(QR)) and np.all((tau == 0) | (tau == 1))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n", [(129, 129), (300, 129), (257, 200), (600, 384)])
def test_model_ormqr_orgqr(m, n, dtype):
    U, A, _ = cq.planted(m, n, dtype=dtype)
    QR, tau = cq.geqrf(A)
    QtA = cq.ormqr(QR, tau, A, True)
    assert np.array_equal(QtA[:n], np.triu(QR[:n])) and not QtA[n:].any(), "Q^T A = R exactly"
    for ncols in (1, 7, 200):
        Cm = np.random.default_rng(ncols).integers(-3, 4, (m, ncols)).astype(dtype)
        for k in (n, max(1, n - 70)):
            W = cq.ormqr(QR, tau[:k], Cm, True)
            assert np.array_equal(W, _lapack_ormqr(QR, tau[:k], Cm, True))
            assert np.array_equal(cq.ormqr(QR, tau[:k], W, False), Cm), "Q (Q^T C) = C exactly"
            assert np.array_equal(cq.ormqr(QR, tau[:k], Cm, False), _lapack_ormqr(QR, tau[:k], Cm, False))
    Q = cq.orgqr(QR, tau)
    Lq, _, info = getattr(lapack, _p(dtype) + "orgqr")(QR, tau)
    assert info == 0 and np.array_equal(Q, Lq)
    assert np.all(np.isin(Q, (-1, 0, 1))) and np.array_equal(Q.T @ Q, np.eye(n, dtype=dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nrhs", cq.GELS_NRHS)
@pytest.mark.parametrize("m,n", cq.GELS_SHAPES)
def test_model_gels_is_exact(m, n, nrhs, dtype):
    """The solve through the block inverses is exact at cpu_qr.PLANTED_SEED for every shape the GPU tests use."""
    _, A, _ = cq.planted(m, n, dtype=dtype)
    x0, b, enorm = cq.planted_rhs(m, n, nrhs, dtype=dtype)
    QR, tau, Bo, info = cq.gels(A, b)
    assert info == 0
    assert np.array_equal(Bo[:n], x0)
    assert np.array_equal(np.sqrt((Bo[n:].astype(np.float64) ** 2).sum(axis=0)), enorm)
    _, x, info = getattr(lapack, _p(dtype) + "gels")(A, b)
    assert info == 0 and np.array_equal(x[:n].reshape(n, -1), x0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("j", cq.ZERO_COLUMNS)
def test_model_zero_column(j, dtype):
    U, A, _ = cq.planted_zero_column(300, 257, j, dtype=dtype)
    QR, tau = cq.geqrf(A)
    assert tau[j] == 0 and QR[j, j] == 0
    assert cq.diag_info(QR[:257]) == j + 1
    Lq, Lt = _lapack_geqrf(A)
    assert np.array_equal(QR, Lq) and np.array_equal(tau, Lt)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n", cq.ROUNDED)
def test_rounded_ratios_beside_lapack(m, n, dtype):
    """U(-1, 1) inputs: ||A - QR||_1 / (m u ||A||_1), ||I - Q^T Q||_1 / (m u) and the least-squares ratio of the model
    beside LAPACK's; both pass LAPACK's own threshold.  Measured (LAPACK -> model), fp64: 129 x 129 0.053 -> 0.082 and
    0.69 -> 0.70; 1000 x 257 0.0083 -> 0.0117 and 0.056 -> 0.184; fp32 alike."""
    mod = cq.model_ratios(m, n, np.dtype(dtype).name)
    lap = cq.lapack_ratios(m, n, np.dtype(dtype).name)
    print(f"{m}x{n} {np.dtype(dtype).name}: LAPACK {lap[0]:.4f} {lap[1]:.4f} {lap[2]:.4f} -> model {mod[0]:.4f} {mod[1]:.4f} {mod[2]:.4f}")
    assert max(mod) < cq.LAPACK_THRESH and max(lap) < cq.LAPACK_THRESH
