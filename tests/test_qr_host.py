"""CPU proofs behind tests/test_gpu_qr.py: for every shape and seed the GPU tests use, the numpy model of the QR
kernels (tests/cpu_qr.py) returns the planted factor exactly in both precisions and equals LAPACK (scipy) bit for bit,
and the solve through the block inverses returns the planted least-squares solution exactly.  On rounded inputs the
model's three LAPACK ratios are recorded beside LAPACK's own.

The dense-reflector plant (cpu_qr.hadamard_plant).  In the plant A = P [U; 0] every reflector is e_j +- e_k, so every
Gram sum of the panel step, every slab slot, every entry of V^T V and every product of the block apply has one
non-zero term: a sum that drops, doubles or misplaces a slab slot, a 64-row chunk or a K-slice passes those tests.
Behind A = [0; H[:, :n] U] (H Sylvester-Hadamard of order 4^q) every reflector has 4^q non-zeros and the result is
still known exactly; here the closed form, the model and LAPACK are shown equal bit for bit, gels exact, V dense and
tau all ones, and a Gram sum that leaves out any one 64-row chunk of the Hadamard rows is shown to change the result.
The tall shape 16514 x 130 is the first whose panels have slabs of more than 64 rows (qr_slab_rows = 128: the chunk loop
of qr_panel_step_kernel runs twice); cpu_qr.TALL_SPARSE crosses the tau = 0 branch and the zero column with it.
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


# ------------------------------------------------------------------ the dense-reflector plant, and the tall shapes
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("q,n", cq.HADAMARD_SHAPES)
def test_hadamard_closed_form_model_and_lapack_agree(q, n, dtype):
    U, A = cq.hadamard_plant(q, n, dtype=dtype)
    N = 4 ** q
    assert A.shape == (n + N, n) and not A[:n].any() and np.abs(A).max() < 2 ** 10
    want, wtau, _ = cq.hadamard_expected(q, n, dtype=dtype)
    QR, tau = cq.hadamard_model(q, n, np.dtype(dtype).name)
    assert QR.dtype == np.dtype(dtype) and np.array_equal(QR, want) and np.array_equal(tau, wtau)
    Lq, Lt = _lapack_geqrf(A)
    assert np.array_equal(Lq, want) and np.array_equal(Lt, wtau)
    # the plant discriminates: dense reflectors, tau all ones, R = -2^q S U with both signs on the diagonal of U
    assert np.all(tau == 1)
    assert np.array_equal(np.count_nonzero(np.tril(QR, -1), axis=0), np.full(n, N)), "every v_j has 4^q non-zeros"
    assert not np.tril(QR[:n], -1).any()
    S = np.sign(np.diagonal(U))
    assert (S > 0).any() and (S < 0).any()
    assert np.array_equal(np.triu(QR[:n]), -(2.0 ** q) * S[:, None] * U)
    V = cq.extract_v(QR[:, :min(n, cq.QB)])
    G = V.T @ V
    assert np.array_equal(G, 2 * np.eye(G.shape[0])), "V^T V = 2 I"
    assert np.array_equal(cq.larft(V, tau[:G.shape[0]]), np.eye(G.shape[0])), "T = I"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("q,n", cq.HADAMARD_SHAPES)
def test_hadamard_gels_is_exact(q, n, dtype):
    _, A = cq.hadamard_plant(q, n, dtype=dtype)
    nrhs = cq.HADAMARD_NRHS[(q, n)]
    x0, b, enorm = cq.hadamard_rhs(q, n, nrhs, dtype=dtype)
    assert np.array_equal(enorm, np.round(enorm)) and (enorm.any() or n == 4 ** q)
    QR, tau, Bo, info = cq.gels(A, b)
    assert info == 0 and np.array_equal(QR, cq.hadamard_model(q, n, np.dtype(dtype).name)[0])
    assert np.array_equal(Bo[:n], x0)
    assert np.array_equal(np.sqrt((Bo[n:].astype(np.float64) ** 2).sum(axis=0)), enorm)
    _, x, info = getattr(lapack, _p(dtype) + "gels")(A, b)
    assert info == 0 and np.array_equal(x[:n].reshape(n, -1), x0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("q,n", cq.HADAMARD_SHAPES)
def test_hadamard_ormqr_orgqr(q, n, dtype):
    _, A = cq.hadamard_plant(q, n, dtype=dtype)
    m = A.shape[0]
    QR, tau = cq.hadamard_model(q, n, np.dtype(dtype).name)
    QtA = cq.ormqr(QR, tau, A, True)
    assert np.array_equal(QtA[:n], np.triu(QR[:n])) and not QtA[n:].any(), "Q^T A = R exactly"
    for ncols in (1, 7, 200):
        Cm = cq.hadamard_c(m, ncols, dtype)
        for k in (n, max(1, n - 70)):
            W = cq.ormqr(QR, tau[:k], Cm, True)
            assert np.array_equal(W, _lapack_ormqr(QR, tau[:k], Cm, True))
            assert np.array_equal(cq.ormqr(QR, tau[:k], W, False), Cm), "Q (Q^T C) = C exactly"
            assert np.array_equal(cq.ormqr(QR, tau[:k], Cm, False), _lapack_ormqr(QR, tau[:k], Cm, False))
    Q = cq.orgqr(QR, tau)
    Lq, _, info = getattr(lapack, _p(dtype) + "orgqr")(np.array(QR), np.array(tau))
    assert info == 0 and np.array_equal(Q, Lq)
    assert np.array_equal(Q, cq.hadamard_expected(q, n, dtype=dtype)[2])
    assert np.array_equal(Q.T @ Q, np.eye(n, dtype=dtype))
    k = max(1, n - 70)
    Lk, _, info = getattr(lapack, _p(dtype) + "orgqr")(np.array(QR), np.array(tau[:k]))
    assert info == 0 and np.array_equal(cq.orgqr(QR, tau[:k]), Lk), "k < n"


@pytest.mark.parametrize("q,n", [(4, 129), cq.HADAMARD_TALL])
def test_a_gram_sum_without_one_chunk_of_rows_changes_the_result(q, n):
    """The panel of the model with one 64-row chunk left out of its Gram sums: on the Hadamard plant the result
    differs for EVERY chunk that holds Hadamard rows (at 385 x 129; at 16514 x 130 the second chunk of the first slab
    below the zero rows, a chunk in the middle and the 2-row last slab).  On the one-non-zero plant a chunk that holds
    no row of U -- most of them -- can be left out of every sum unnoticed."""
    _, A = cq.hadamard_plant(q, n)
    m = A.shape[0]
    jb = min(n, cq.QB)
    ref = A[:, :jb].copy()
    rtau = cq.panel(ref)
    assert np.array_equal(ref, cq.hadamard_model(q, n, "float64")[0][:, :jb])
    chunks = range(n // 64, (m + 63) // 64) if m < 1000 else (192 // 64, 8000 // 64, (m - 1) // 64)
    for ch in chunks:
        keep = np.ones(m, dtype=bool)
        keep[64 * ch:64 * ch + 64] = False
        assert A[~keep].any()
        P = A[:, :jb].copy()
        tau = cq.panel(P, gram_rows=keep)
        assert not (np.array_equal(P, ref) and np.array_equal(tau, rtau)), f"chunk {ch} goes unnoticed"
    # the one-non-zero plant: most chunks of its 16500 rows hold zeros only, and none of those is missed
    m5, n5 = cq.TALL_SPARSE[0]
    _, B, _ = cq.planted(m5, n5)
    ch = next(c for c in range(2, m5 // 64) if not B[64 * c:64 * c + 64].any())
    keep = np.ones(m5, dtype=bool)
    keep[64 * ch:64 * ch + 64] = False
    P, Pm = B.copy(), B.copy()
    assert np.array_equal(cq.panel(P), cq.panel(Pm, gram_rows=keep)) and np.array_equal(P, Pm)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n", cq.TALL_SPARSE)
def test_tall_sparse_plant(m, n, dtype):
    """The one-non-zero plant at 16500 rows (two chunks per slab), its right-hand sides and a zero column."""
    U, A, _ = cq.planted(m, n, dtype=dtype)
    QR, tau = cq.geqrf(A)
    _check_plant(U, QR, tau)
    assert (tau == 0).any() and (tau == 1).any()
    Lq, Lt = _lapack_geqrf(A)
    assert np.array_equal(QR, Lq) and np.array_equal(tau, Lt)
    x0, b, enorm = cq.planted_rhs(m, n, 3, dtype=dtype)
    _, _, Bo, info = cq.gels(A, b)
    assert info == 0 and np.array_equal(Bo[:n], x0)
    assert np.array_equal(np.sqrt((Bo[n:].astype(np.float64) ** 2).sum(axis=0)), enorm)
    j = n - 2
    _, Z, _ = cq.planted_zero_column(m, n, j, dtype=dtype)
    zq, zt = cq.geqrf(Z)
    assert zt[j] == 0 and zq[j, j] == 0 and cq.diag_info(zq[:n]) == j + 1
    Lq, Lt = _lapack_geqrf(Z)
    assert np.array_equal(zq, Lq) and np.array_equal(zt, Lt)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n", cq.ROUNDED_TALL)
def test_rounded_tall_ratios_beside_lapack(m, n, dtype):
    """The tall U(-1, 1) shape, apart from cpu_qr.ROUNDED: the model and LAPACK pass LAPACK's threshold.  The fp32
    ratios are evaluated in fp64 (cpu_qr.tall_wide): np.longdouble products of this size take seconds.  Measured
    (LAPACK -> model): fp64 0.00034 -> 0.00033, 0.00086 -> 0.0056, 3.2e-8 -> 4.0e-8; fp32 0.00033 -> 0.00023,
    0.00094 -> 0.00076, 3.2e-8 -> 2.3e-8."""
    name, wide = np.dtype(dtype).name, cq.tall_wide(dtype)
    mod, lap = cq.model_ratios(m, n, name, wide), cq.lapack_ratios(m, n, name, wide)
    print(f"{m}x{n} {name}: LAPACK {lap[0]:.5f} {lap[1]:.5f} {lap[2]:.2e} -> model {mod[0]:.5f} {mod[1]:.5f} {mod[2]:.2e}")
    assert max(mod) < cq.LAPACK_THRESH and max(lap) < cq.LAPACK_THRESH


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
