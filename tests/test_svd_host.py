"""CPU-side proof of the numpy model of the Jacobi SVD (tests/cpu_svd.py), of its builders and of the bounds the GPU
tests (tests/test_gpu_svd.py) hold the kernels to.  Nothing here needs a device."""
import numpy as np
import pytest

import cpu_svd as cs

DTYPES = [np.float64, np.float32]


# ------------------------------------------------------------------ the pair order
@pytest.mark.parametrize("p", [1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 129, 130])
def test_round_pairs_closed_form_is_the_list_rotation_and_a_sweep_covers_every_pair_once(p):
    P = p + (p & 1)
    seen = []
    for r in range(max(P - 1, 1)):
        I, J = cs.round_pairs(p, r)
        got = sorted(zip(I.tolist(), J.tolist()))
        assert got == sorted(cs.round_pairs_by_rotation(p, r))
        rows = I.tolist() + J.tolist()
        assert len(set(rows)) == len(rows)                     # the pairs of a round share no row
        assert all(i < j < p for i, j in got)
        seen += got
    assert len(seen) == p * (p - 1) // 2 and len(set(seen)) == len(seen)


# ------------------------------------------------------------------ exact plants
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tall", [False, True])
def test_unit_rows_plant_is_exact_in_the_model(tall, dtype):
    A, s = cs.unit_rows(tall, False, dtype)
    f = cs.gesvdj(A)
    assert (f["sweeps"], f["rotations"], f["info"]) == (1, 0, 0)
    assert np.array_equal(f["s"], s)
    assert np.array_equal((f["U"].astype(np.float64) * f["s"]) @ f["Vt"].astype(np.float64), A)
    k = min(A.shape)
    assert np.array_equal(f["U"].T @ f["U"], np.eye(k))        # orthonormal although a singular value is zero
    assert np.array_equal(f["Vt"][-1], np.zeros(A.shape[1]))   # ... and its row of Vt is a row of zeros
    assert np.array_equal(cs.gesvdj(A, jobz=0)["s"], s)
    A2, _ = cs.unit_rows(tall, True, dtype)
    B, X = cs.unit_rows_rhs(tall, 3, dtype)
    g = cs.gelss(A2, B)
    assert g["rank"] == 5 and np.array_equal(g["x"], X)
    assert np.allclose(X, np.linalg.pinv(A2.astype(np.float64)) @ B.astype(np.float64), rtol=1e-6, atol=0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("spec", cs.HADAMARD, ids=lambda s: f"{s[0]}x{s[2]}")
def test_hadamard_rows_plant_is_exact_and_tells_a_dropped_chunk(spec, dtype):
    A, U, s, Vt = cs.hadamard_rows(*spec, dtype=dtype)
    assert A.shape == (spec[0], spec[2]) and np.array_equal((U.astype(np.float64) * s) @ Vt.astype(np.float64), A)
    f = cs.gesvdj(A)
    assert (f["sweeps"], f["rotations"], f["info"]) == (1, 0, 0)
    assert np.array_equal(f["s"], s) and np.array_equal(f["U"], U) and np.array_equal(f["Vt"], Vt)
    # one 16-byte group, one wave's groups, one pass of a workgroup's load loop (fp64: 512 columns, fp32: 1024) left out
    # of the sums: some pair then sees c != 0 and rotates
    N = 4 ** spec[1]
    chunks = [2, 4] if spec[3] == 1 else [2, 4, 128, 256, 512, 1024]
    for ch in chunks:
        for lo in (0, ch, N - ch):
            assert cs.gesvdj(A, drop=(lo, lo + ch))["rotations"] > 0, (ch, lo)


def test_long_plants_take_both_forms_of_the_round_kernel():
    """6 x 4096 is the longest fp64 row that stays in registers (SVD_NT * SVD_KEEP = 2048 groups of 16 bytes), 6 x 16387
    is re-read in both precisions (fp32 keeps 8192 columns)."""
    keep = {np.float64: 256 * 8 * 2, np.float32: 256 * 8 * 4}
    cols = [spec[2] for spec in cs.HADAMARD]
    assert cols == [257, 4096, 16387]
    assert cols[1] == keep[np.float64] and cols[1] > 256 * 4 and cols[2] > keep[np.float32]


@pytest.mark.parametrize("dtype", DTYPES)
def test_doubled_hadamard_plant_keeps_one_sweep_and_tells_a_dropped_chunk(dtype):
    A, s = cs.hadamard_doubled(dtype)
    assert A.shape == (6, 256 * 8 * 4)                          # SVD_NT * SVD_KEEP groups of four fp32
    f = cs.gesvdj(A)
    assert (f["sweeps"], f["rotations"], f["info"]) == (1, 0, 0)
    assert np.allclose(f["s"], s, rtol=4 * cs.UNIT[np.dtype(np.float64)], atol=0)
    for ch in (4, 256, 1024):
        for lo in (0, 4096, 8192 - ch):
            assert cs.gesvdj(A, drop=(lo, lo + ch))["rotations"] > 0, (ch, lo)


# ------------------------------------------------------------------ rounded inputs and the pooled bounds
@pytest.mark.parametrize("dtype", DTYPES)
def test_model_and_lapack_ratios_on_the_rounded_shapes_and_the_pooled_bounds(dtype):
    name = np.dtype(dtype).name
    for m, n in cs.ROUNDED:
        f = cs.model_result(m, n, name)
        assert f["info"] == 0 and 1 <= f["sweeps"] <= 14
        assert np.all(np.diff(f["s"]) <= 0)
        print(name, m, n, f["sweeps"], cs.model_ratios(m, n, name), cs.lapack_ratios(m, n, name))
    b = cs.pooled_bounds(name)
    print(name, "pooled", b)
    assert all(0 < v < cs.LAPACK_THRESH for v in b)


@pytest.mark.parametrize("dtype", DTYPES)
def test_model_is_invariant_under_powers_of_two(dtype):
    A = cs.rounded(5, 7, dtype)
    f0 = cs.gesvdj(A)
    for d in (20, -20):
        f1 = cs.gesvdj(np.ldexp(A, d))
        assert np.array_equal(f1["U"], f0["U"]) and np.array_equal(f1["Vt"], f0["Vt"])
        assert np.array_equal(f1["s"], np.ldexp(f0["s"], d))
        assert (f1["sweeps"], f1["rotations"]) == (f0["sweeps"], f0["rotations"])


# ------------------------------------------------------------------ rank, minimum norm, outcomes
@pytest.mark.parametrize("dtype", DTYPES)
def test_model_minimum_norm_solutions(dtype):
    u = cs.UNIT[np.dtype(dtype)]
    for m, n in cs.RANK_SHAPES:
        A, b, x = cs.rank_product(m, n, dtype)
        g = cs.gelss(A, b)
        assert g["rank"] == cs.RANK
        assert cs.rel_err(g["x"], x) < 1e4 * u
        assert np.abs(np.asarray(A, np.longdouble) @ x - np.asarray(A, np.longdouble) @ np.asarray(
            np.linalg.lstsq(A.astype(np.float64), b.astype(np.float64), rcond=None)[0], np.longdouble)).max() < 1e-9
    A, b, x = cs.wide_case(dtype)
    g = cs.gelss(A, b)
    assert g["rank"] == 5 and cs.rel_err(g["x"], x) < 1e4 * u


def test_model_outcomes():
    A = cs.rounded(5, 7, np.float64)
    f = cs.gesvdj(A, max_sweeps=1)
    assert f["info"] == 1 and f["sweeps"] == 1 and np.all(np.isfinite(f["s"])) and np.all(np.isfinite(f["U"]))
    for shape in ((5, 7), (7, 5)):
        for bad in (np.nan, np.inf):
            B = cs.rounded(*shape, np.float64).copy()
            B[2, 3] = bad
            f = cs.gesvdj(B)
            assert np.isnan(f["s"]).all() and f["info"] == 0 and f["sweeps"] <= 1
    Z = np.zeros((6, 6))
    f = cs.gesvdj(Z)
    assert np.array_equal(f["s"], np.zeros(6)) and np.array_equal(f["Vt"], Z) and np.array_equal(f["U"], np.eye(6))
    g = cs.gelss(Z, np.ones((6, 2)))
    assert g["rank"] == 0 and np.array_equal(g["x"], np.zeros((6, 2)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_model_converges_on_the_graded_matrix_within_20_sweeps(dtype):
    G = cs.graded(dtype)
    assert G.shape == cs.GRADED
    f = cs.gesvdj(G)
    assert f["info"] == 0 and f["sweeps"] <= 20
    ref = cs.graded_values()
    assert np.abs(f["s"] - ref).max() <= 64 * 64 * cs.UNIT[np.dtype(dtype)] * ref[0]
