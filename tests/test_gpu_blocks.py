"""The building blocks of the multi-GPU driver (lsx_trsm_lu_f64_dev, lsx_laswp_f64_dev, lsx_laswp_moves_f64_dev,
lsx_panel_f64_dev with row0 > 0, lsx_gemm_add_f64_dev) and the fp32 update, each against a plain numpy statement of
what it computes.  tests/test_dist_gpu.py reaches them only through whole sharded factorisations.

Bounds: data movement is compared bit for bit.  trsm: 64 jb u max|X| on a well-conditioned unit-lower block, the
constant checked in the same test against a numpy fp64 substitution (both measured against a substitution in extended
precision).  panel: m u max|P| against tests/cpu_ops.CpuOps.panel_.  gemm fp64: the bound of
test_gemm_sub_fp64_against_numpy (1e-13 k).  gemm fp32: 2 k 2^-24 max|A| max|B| for the inner product (each of the
k products and k additions rounds once, |a b| <= max|A| max|B|) plus one rounding of the result.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U64 = 2.0 ** -53
U32 = 2.0 ** -24
GEMM_SHAPES = [(16, 16, 4), (128, 128, 128), (300, 200, 64), (1000, 130, 128), (257, 513, 100), (64, 1, 64),
               (500, 7, 128), (129, 16, 3), (1984, 128, 128), (64, 256, 16), (4032, 384, 128)]


@pytest.fixture(scope="module")
def dev():
    import torch

    from linalg_solver_amd.device import DeviceSolver

    assert torch.cuda.is_available()
    return DeviceSolver()


def _substitute(L, B, dtype):
    """Forward substitution with the STRICTLY lower part of L and an implied unit diagonal, in `dtype`."""
    Ls = np.tril(L, -1).astype(dtype)
    X = B.astype(dtype).copy()
    for i in range(1, L.shape[0]):
        X[i] -= Ls[i, :i] @ X[:i]
    return X


@pytest.mark.parametrize("ncols", [1, 7, 128, 130, 1000])
@pytest.mark.parametrize("jb", [1, 16, 63, 64, 100, 128])
def test_trsm_lu_against_substitution(dev, jb, ncols):
    """L is a block inside a larger matrix whose diagonal and upper part hold garbage (5 .. 9): unit lower means they
    are never read into the result.  B is a block of a larger matrix too; the rest of it must not change."""
    import torch

    rng = np.random.default_rng(jb * 1009 + ncols)
    big = rng.uniform(5.0, 9.0, (jb + 40, jb + 50))
    r0, c0 = 20, 30
    low = np.tril(rng.uniform(-0.5, 0.5, (jb, jb)) / np.sqrt(jb), -1)
    blk = big[r0:r0 + jb, c0:c0 + jb]
    blk[np.tril_indices(jb, -1)] = low[np.tril_indices(jb, -1)]
    Bbig = rng.uniform(-1.0, 1.0, (jb + 7, ncols + 9))
    B = Bbig[3:3 + jb, 4:4 + ncols].copy()
    dL, dB = torch.from_numpy(big).cuda(), torch.from_numpy(Bbig).cuda()
    dev.trsm_lu_(dL[r0:r0 + jb, c0:c0 + jb], dB[3:3 + jb, 4:4 + ncols])
    torch.cuda.synchronize()
    got_big = dB.cpu().numpy()
    got = got_big[3:3 + jb, 4:4 + ncols]
    ref = _substitute(blk, B, np.longdouble)
    own = _substitute(blk, B, np.float64)
    bound = 64 * jb * U64 * float(np.abs(ref).max())
    e_own = float(np.abs(own - ref).max())
    e_gpu = float(np.abs(got - ref).max())
    print(f"trsm_lu jb={jb} ncols={ncols}: GPU {e_gpu:.2e}, numpy fp64 substitution {e_own:.2e}, bound {bound:.2e}")
    assert e_own <= bound, "the constant does not even hold for a plain fp64 substitution"
    assert np.all(np.isfinite(got)) and e_gpu <= bound
    rest = np.ones(Bbig.shape, dtype=bool)
    rest[3:3 + jb, 4:4 + ncols] = False
    assert np.array_equal(got_big[rest], Bbig[rest]) and np.array_equal(dL.cpu().numpy(), big)


def _ipiv_with_chains(rng, rows, row0, jb):
    """Global 0-based targets >= row0 + k with every awkward case: no interchange, a target inside the block that a
    later step moves again (a row that is destination of one move and source of another), a repeated target."""
    piv = np.array([rng.integers(row0 + k, rows) for k in range(jb)], dtype=np.int32)
    if jb >= 8:
        piv[0] = row0 + jb - 1          # row0 <-> last row of the block, which step jb - 1 moves again
        piv[1] = row0 + 5               # inside the block, ahead of step 5
        piv[2] = row0 + 2               # no interchange
        piv[3] = piv[4] = rows - 1      # the same far row twice
        piv[jb - 1] = rows - 2
    return piv


@pytest.mark.parametrize("ncols", [1, 31, 33, 100])
@pytest.mark.parametrize("row0,jb", [(0, 128), (128, 100), (300, 1), (5, 256), (64, 17)])
def test_laswp_is_the_sequential_interchange(dev, row0, jb, ncols):
    import torch

    from cpu_ops import CpuOps

    rows, cols = row0 + jb + 400, 120
    A = np.arange(rows * cols, dtype=np.float64).reshape(rows, cols) + 0.5      # every entry distinct
    piv = _ipiv_with_chains(np.random.default_rng(row0 + jb + ncols), rows, row0, jb)
    want = torch.from_numpy(A.copy())
    CpuOps().laswp_(want[:, :ncols], row0, jb, torch.from_numpy(piv))
    dA = torch.from_numpy(A).cuda()
    dev.laswp_(dA[:, :ncols], row0, jb, torch.from_numpy(piv).cuda())
    torch.cuda.synchronize()
    assert torch.equal(dA.cpu(), want), "interchanges differ from the sequential definition (or left their columns)"
    assert not torch.equal(want, torch.from_numpy(A))


@pytest.mark.parametrize("row0,ncols", [(0, 64), (17, 33), (128, 100), (1000, 7)])
def test_hand_made_gather_list(dev, row0, ncols):
    """Two cycles (lengths 3 and 40) and a plain exchange, scattered over the 256 slots."""
    import torch

    rows, cols = row0 + 400, 110
    A = np.arange(rows * cols, dtype=np.float64).reshape(rows, cols) + 0.25
    rng = np.random.default_rng(row0 + ncols)
    pool = rng.permutation(256)
    slots = iter(rng.permutation(256).tolist())
    mv = np.full((256, 2), -1, dtype=np.int32)
    for cyc in (pool[:3], pool[3:43], pool[43:45]):
        for i in range(len(cyc)):
            mv[next(slots)] = (cyc[i], cyc[(i + 1) % len(cyc)])
    dA = torch.from_numpy(A).cuda()
    dev.laswp_moves_(dA[:, :ncols], row0, torch.from_numpy(mv.reshape(-1)).cuda())
    torch.cuda.synchronize()
    want = A.copy()
    for d, s in mv:
        if d >= 0:
            want[row0 + d, :ncols] = A[row0 + s, :ncols]
    assert np.array_equal(dA.cpu().numpy(), want)


@pytest.mark.parametrize("row0,m,jb", [(0, 700, 128), (128, 1500, 100), (1000, 2600, 128), (128, 600, 17), (1000, 4200, 128)])
def test_panel_on_a_column_block_with_a_row_offset(dev, row0, m, jb):
    """The panel is a column block of a larger matrix that starts at row row0 (ldp > jb): ipiv holds GLOBAL rows and
    equals the numpy panel's, info stays 0, the factors agree to m u, nothing outside the block changes; the gather
    list the panel emitted does to other columns exactly what laswp_ does with the same ipiv."""
    import torch

    from cpu_ops import CpuOps
    from linalg_solver_amd import gen

    rows, cols, c0 = row0 + m, 300, 50
    A0 = gen.fill(gen.U11, 31 + row0 + jb, rows, cols)
    dA = torch.from_numpy(A0).cuda()
    ipiv = torch.zeros(jb, dtype=torch.int32, device="cuda")
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    dev.panel_(dA[row0:, c0:c0 + jb], row0, ipiv, info)
    mv = torch.full((512,), -7, dtype=torch.int32, device="cuda")
    listed = dev.panel_moves_(mv)
    torch.cuda.synchronize()
    Pc = torch.from_numpy(A0[row0:, c0:c0 + jb].copy())
    pc, ic = torch.zeros(jb, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    CpuOps().panel_(Pc, row0, pc, ic)
    got = dA.cpu().numpy()
    piv = ipiv.cpu().numpy()
    assert int(info.item()) == 0 == int(ic[0])
    assert np.all(piv >= row0 + np.arange(jb)) and np.all(piv < rows)
    assert np.array_equal(piv, pc.numpy()), f"first differing column {int(np.nonzero(piv != pc.numpy())[0][0])}"
    ref = Pc.numpy()
    err = float(np.abs(got[row0:, c0:c0 + jb] - ref).max())
    print(f"panel row0={row0} m={m} jb={jb}: max difference from the numpy panel {err:.2e} (bound {m * U64 * np.abs(ref).max():.2e})")
    assert err <= m * U64 * float(np.abs(ref).max())
    outside = np.ones(A0.shape, dtype=bool)
    outside[row0:, c0:c0 + jb] = False
    assert np.array_equal(got[outside], A0[outside])
    # the gather list against the interchange list, on columns the panel did not touch
    assert listed, "the cooperative panels emit a gather list"
    X1, X2 = torch.from_numpy(A0[:, :c0].copy()).cuda(), torch.from_numpy(A0[:, :c0].copy()).cuda()
    dev.laswp_moves_(X1[:, :37], row0, mv)
    dev.laswp_(X2[:, :37], row0, jb, ipiv)
    torch.cuda.synchronize()
    want = torch.from_numpy(A0[:, :c0].copy())
    CpuOps().laswp_(want[:, :37], row0, jb, pc)
    assert torch.equal(X1, X2) and torch.equal(X2.cpu(), want)


@pytest.mark.parametrize("m,n,k", GEMM_SHAPES)
def test_gemm_add_fp64_against_numpy(dev, m, n, k):
    import torch

    rng = np.random.default_rng(m * 7 + n * 3 + k + 1)
    A, B, C = rng.uniform(-1, 1, (m, k)), rng.uniform(-1, 1, (k, n)), rng.uniform(-1, 1, (m, n))
    dA, dB, dC = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda(), torch.from_numpy(C).cuda()
    dev.gemm_add_(dC, dA, dB)
    assert np.max(np.abs(dC.cpu().numpy() - (C + A @ B))) < 1e-13 * k
    dev.gemm_sub_(dC, dA, dB)      # and back
    assert np.max(np.abs(dC.cpu().numpy() - C)) < 1e-13 * k


@pytest.mark.parametrize("m,n,k", GEMM_SHAPES)
def test_gemm_sub_fp32_against_the_fp64_product(dev, m, n, k):
    import torch

    rng = np.random.default_rng(m * 7 + n * 3 + k + 2)
    A, B, C = (rng.uniform(-1, 1, s).astype(np.float32) for s in ((m, k), (k, n), (m, n)))
    dC = torch.from_numpy(C.copy()).cuda()
    dev.gemm_sub_(dC, torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda())
    want = C.astype(np.float64) - A.astype(np.float64) @ B.astype(np.float64)
    bound = 2 * k * U32 * float(np.abs(A).max() * np.abs(B).max()) + U32 * float(np.abs(want).max())
    err = float(np.abs(dC.cpu().numpy().astype(np.float64) - want).max())
    print(f"gemm_sub fp32 {m}x{n}x{k}: {err:.2e} (bound {bound:.2e})")
    assert err <= bound
