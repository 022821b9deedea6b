"""The numpy model of the SPD inverse (tests/cpu_potri.py) against LAPACK, and the exactness claims the GPU tests of
tests/test_gpu_potri.py rest on, proved on the CPU for every order and seed they use."""
import numpy as np
import pytest
from scipy.linalg import lapack

import cpu_chol as cc
import cpu_potri as cp

DTYPES = [np.float64, np.float32]


def _lapack(name, dtype):
    return getattr(lapack, ("d" if np.dtype(dtype) == np.float64 else "s") + name)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [5, 129, 300])
def test_model_against_lapack_potri(n, dtype):
    """LAPACK's test ratio of the model's inverse, beside the ratio LAPACK's potri reaches on the same input.  The ratio
    is normalised by n u ||A|| ||X||, so a backward-stable inverse keeps it below a constant of order one whatever n
    is; LAPACK's own test suite accepts 30, this asks for 1.  (The two differ by more than noise on these diagonally
    dominant inputs: the model sums k in ascending order, which meets the dominant term v_jj v_ji first and rounds every
    later addition at its size; dlauu2 adds it last.  Both figures are printed.)"""
    A = cc.spd(n, 0, dtype)
    R, info = cc.potrf(A)
    assert info == 0
    X, info = cp.potri(R)
    assert info == 0
    assert np.array_equal(np.tril(X, -1), np.tril(A, -1)), "the strictly lower triangle is untouched"
    c, linfo = _lapack("potrf", dtype)(A, lower=0)
    L, linfo2 = _lapack("potri", dtype)(c, lower=0)
    assert linfo == 0 and linfo2 == 0
    mine, theirs = cp.inverse_ratio(A, cp.symmetrize(X)), cp.inverse_ratio(A, cp.symmetrize(L))
    print(f"n={n} {np.dtype(dtype).name}: model {mine:.3f}, LAPACK {theirs:.3f}")
    assert mine <= 1.0 and theirs <= 1.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [5, 129, 300])
def test_model_against_lapack_trtri(n, dtype):
    """Phase 1 against dtrtri / strtri of the same factor: inv(U)^T, entry by entry to a forward bound
    cond-free for this well-conditioned factor (|V - V_ref| <= gamma_n |inv(U)^T| |U^T| |inv(U)^T|)."""
    U = np.triu(cc.potrf(cc.spd(n, 0, dtype))[0])
    V = cp.trtri_upper_t(U)
    ref, info = _lapack("trtri", dtype)(U, lower=0)
    assert info == 0
    assert np.array_equal(np.triu(V, 1), np.zeros_like(V)), "V is lower triangular, exact zeros above the diagonal"
    Rl = np.abs(ref.T.astype(np.longdouble))
    bound = 2 * cc.gamma(n, dtype) * (Rl @ np.abs(U.T.astype(np.longdouble)) @ Rl)
    assert (np.abs(V.astype(np.longdouble) - ref.T.astype(np.longdouble)) <= bound).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", cp.PLANTED_ORDERS)
def test_planted_inverse_is_exact(n, dtype):
    """Magnitudes below 2^12; cpu_chol.potrf returns U exactly; the blocked phase 1 returns V exactly -- with NaN in
    the blocks it must not touch; the trapezoid product returns inv(A) exactly."""
    U, A, V, X = cp.planted(n, dtype=dtype)
    amax, xmax = cp.planted_magnitudes(n)
    assert amax < 2 ** 12 and xmax < 2 ** 12
    assert np.array_equal(A.astype(np.float64) @ X.astype(np.float64), np.eye(n)), "X is the inverse of A"
    assert np.array_equal(V.astype(np.float64) @ U.T.astype(np.float64), np.eye(n)), "V is the inverse of U^T"
    R, info = cc.potrf(cc.fill_lower(A, np.nan))
    assert info == 0 and np.array_equal(np.triu(R), U)
    Vgot = cp.trtri_upper_t(U, np.full((n, n), np.nan, dtype=dtype))
    assert np.array_equal(Vgot, cp.lower_blocks_nan(V), equal_nan=True)
    Cgot = cp.lauum_tn(Vgot, np.full((n, n), np.nan, dtype=dtype))
    assert np.array_equal(np.triu(Cgot), np.triu(X))
    assert np.isnan(Cgot[np.tril_indices(n, -1)]).all()
    Xp, info = cp.potri(R)
    assert info == 0 and np.array_equal(np.triu(Xp), np.triu(X)) and np.isnan(Xp[np.tril_indices(n, -1)]).all()
    assert np.array_equal(cp.symmetrize(Xp), X)


@pytest.mark.parametrize("n", cp.PLANTED_ORDERS)
def test_planted_determinant_is_a_power_of_two(n):
    U, A, _, _ = cp.planted(n)
    sign, mant, exp2 = cp.planted_det_parts(n)
    assert (sign, mant) == (1.0, 0.5)
    d = np.diagonal(U)
    assert exp2 == 1 + 2 * int(np.log2(d).sum())
    s, logdet = np.linalg.slogdet(A)
    assert s == 1.0 and abs(logdet - (np.log(mant) + exp2 * np.log(2.0))) <= 1e-9 * max(1.0, abs(logdet))


@pytest.mark.parametrize("i", [0, 127, 128, 300])
@pytest.mark.parametrize("bad", [0.0, np.nan])
def test_model_info(i, bad):
    U = cp.planted(384)[0]
    U[i, i] = bad
    _, info = cp.potri(U)
    assert info == i + 1
