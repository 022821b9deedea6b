"""CPU-side proof of the numpy model of the two-sided Jacobi eigensolver (tests/cpu_eig.py), of its builders and of the
bounds the GPU tests (tests/test_gpu_eig.py) hold the kernels to.  Nothing here needs a device.  The model at n = 515
takes numpy about a minute for the two precisions together; it is computed once per process (cpu_eig.model_result)."""
import numpy as np
import pytest

import cpu_eig as ce
import cpu_svd as cs

DTYPES = [np.float64, np.float32]
HALF_CAP = ce.MAX_SWEEPS // 2


# ------------------------------------------------------------------ rounded and special inputs, the bounds
@pytest.mark.parametrize("dtype", DTYPES)
def test_model_and_lapack_ratios_on_the_rounded_orders_and_the_pooled_bounds(dtype):
    name = np.dtype(dtype).name
    for n in ce.ROUNDED:
        A = ce.rounded(n, dtype)
        assert A.dtype == dtype and np.array_equal(A, A.T)
        f = ce.model_result(n, name)
        assert f["info"] == 0 and 1 <= f["sweeps"] <= HALF_CAP
        assert np.all(np.diff(f["w"]) >= 0) and f["V"].shape == (n, n)
        got = ce.model_ratios(n, name)
        print(name, n, f["sweeps"], f["rotations"], got, ce.lapack_ratios(n, name))
        assert all(v < ce.LAPACK_THRESH for v in got)
    b = ce.pooled_bounds(name)
    print(name, "pooled", b)
    assert all(0 < v < 2 * ce.LAPACK_THRESH for v in b)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ce.SPECIAL)
def test_model_on_the_special_inputs(case, dtype):
    name = np.dtype(dtype).name
    A = ce.special(case, dtype)
    assert A.shape == (ce.SPECIAL_N, ce.SPECIAL_N) and np.array_equal(A, A.T)
    f = ce.special_model(case, name)
    assert f["info"] == 0 and 1 <= f["sweeps"] <= HALF_CAP, "a condition on the inputs: half of the default sweep cap"
    got, lap = ce.special_model_ratios(case, name), ce.special_lapack_ratios(case, name)
    print(name, case, f["sweeps"], f["rotations"], got, lap, ce.special_bounds(case, name))
    assert all(v < ce.LAPACK_THRESH for v in got) and all(v < ce.LAPACK_THRESH for v in lap)
    if case != "cycle":
        lam = np.sort(ce.special_values(case))
        assert np.abs(f["w"] - lam).max() <= ce.LAPACK_THRESH * ce.SPECIAL_N * ce.UNIT[np.dtype(dtype)] * np.abs(lam).max()
    else:
        assert not np.diag(A).any()
        lam = np.sort(2.0 * np.cos(2.0 * np.pi * np.arange(ce.SPECIAL_N) / ce.SPECIAL_N))
        assert np.abs(f["w"] - lam).max() <= ce.LAPACK_THRESH * ce.SPECIAL_N * ce.UNIT[np.dtype(dtype)] * 2.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_vectors_through_the_svd_fail_on_the_plus_minus_pairs(dtype):
    """One-sided Jacobi on a symmetric A diagonalises A^2: where +l and -l are both eigenvalues its vectors mix the two
    eigenspaces, and the decomposition ratio is orders of magnitude beyond the bound the GPU test applies."""
    name = np.dtype(dtype).name
    A = ce.special("pm_pairs", dtype)
    w, V = ce.vectors_through_svd(A)
    r = ce.eig_ratios(A, w, V)
    bound = ce.special_bounds("pm_pairs", name)
    print(name, "through the SVD", r, "bound", bound)
    assert r[0] > 1e3 * bound[0]
    assert r[1] <= 30.0, "the vectors are orthonormal all the same: only the first ratio tells"
    # on a definite matrix the same route is fine: the failure is the method's, not the yardstick's
    G = ce.special("graded", dtype)
    wg, Vg = ce.vectors_through_svd(G)
    assert ce.eig_ratios(G, wg, Vg)[0] < ce.LAPACK_THRESH


# ------------------------------------------------------------------ exact plants
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", ce.PLANT_N)
def test_diagonal_plant_is_exact_in_the_model(n, dtype):
    A, w, V = ce.plant_diagonal(n, dtype)
    assert np.array_equal(A.astype(np.float64), np.diag(np.diag(A)).astype(np.float64)), "exact in both precisions"
    f = ce.syevj(A)
    assert (f["sweeps"], f["rotations"], f["info"]) == (1, 0, 0)
    assert np.array_equal(f["w"], w) and np.array_equal(f["V"], V)
    assert set(np.unique(f["V"]).tolist()) == {0.0, 1.0}
    assert np.array_equal(ce.syevj(A, jobz=0)["w"], w)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", ce.PLANT_N)
def test_planted_thresholds_count_exactly_the_pairs_above(n, dtype):
    A, above = ce.plant_threshold(n, dtype)
    thr = ce.threshold(A)
    off = np.triu(A, 1).astype(np.float64)
    I, J = np.nonzero(off)
    assert len(above) >= 2 and len(I) in (2 * len(above), 2 * len(above) - 1)
    assert len(set(I.tolist() + J.tolist())) == 2 * len(I), "no index belongs to two planted pairs"
    big = off[I, J] > thr
    assert sorted(zip(I[big].tolist(), J[big].tolist())) == above
    assert np.all(off[I, J][big] > 1.9 * thr) and np.all(off[I, J][~big] < 0.6 * thr)
    f = ce.syevj(A, max_sweeps=1)
    assert f["sweeps"] == 1 and f["rotations"] == len(above) and f["info"] == 1
    g = ce.syevj(A)
    assert g["info"] == 0 and g["rotations"] == len(above) and g["sweeps"] == 2


# ------------------------------------------------------------------ symmetries and outcomes
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [5, 64])
def test_model_is_invariant_under_powers_of_two(n, dtype):
    A = ce.rounded(n, dtype)
    f0 = ce.model_result(n, np.dtype(dtype).name)
    for d in (20, -20):
        f1 = ce.syevj(np.ldexp(A, d))
        assert np.array_equal(f1["V"], f0["V"]) and np.array_equal(f1["w"], np.ldexp(f0["w"], d))
        assert (f1["sweeps"], f1["rotations"], f1["info"]) == (f0["sweeps"], f0["rotations"], f0["info"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_values_only_gives_the_same_values_and_the_lower_triangle_is_not_read(dtype):
    for n in (5, 64, 129):
        A = ce.rounded(n, dtype)
        f = ce.model_result(n, np.dtype(dtype).name)
        g = ce.syevj(A, jobz=0)
        assert g["V"] is None and np.array_equal(g["w"], f["w"]) and (g["sweeps"], g["rotations"]) == (f["sweeps"], f["rotations"])
        B = A.copy()
        B[np.tril_indices(n, -1)] = np.nan
        assert np.array_equal(ce.syevj(B)["w"], f["w"])


def test_model_outcomes():
    A = ce.rounded(64, np.float64)
    f = ce.syevj(A, max_sweeps=1)
    assert f["info"] == 1 and f["sweeps"] == 1 and np.all(np.isfinite(f["w"])) and np.all(np.diff(f["w"]) >= 0)
    for bad in (np.nan, np.inf):
        B = ce.rounded(5, np.float64).copy()
        B[1, 3] = bad
        f = ce.syevj(B)
        assert np.isnan(f["w"]).all() and f["V"] is None and (f["info"], f["sweeps"], f["rotations"]) == (0, 0, 0)
    f = ce.syevj(np.zeros((6, 6)))
    assert (f["sweeps"], f["rotations"]) == (1, 0) and not f["w"].any() and np.array_equal(f["V"], np.eye(6))
    f = ce.syevj(np.array([[-2.5]]))
    assert (f["sweeps"], f["rotations"]) == (1, 0) and f["w"].tolist() == [-2.5] and f["V"].tolist() == [[1.0]]


def test_the_pair_order_is_the_one_of_the_svd():
    assert ce.round_pairs is cs.round_pairs and ce.rotation is cs.rotation
    assert ce.MAX_SWEEPS == 60 and ce.NT == 256
