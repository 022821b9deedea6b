"""The TN form of the MFMA tile, C -= A^T B with A stored k x m (lsx_gemm_tn_*_dev), on the MI355X: against numpy in
the bounds of tests/test_gpu_blocks.py, on views with odd leading dimensions and offsets, column by column, and its
argument checks.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24

# (m, n, k): interior and ragged tiles, then the thin ones (a single column, a single row, k below one MFMA step)
SHAPES = [(16, 16, 4), (128, 128, 128), (300, 200, 64), (1000, 130, 128), (257, 513, 100), (1984, 128, 128),
          (64, 1, 64), (500, 7, 128), (129, 16, 3), (1, 72, 128), (127, 65, 1)]


@pytest.fixture(scope="module")
def dev():
    import torch

    from linalg_solver_amd.device import DeviceSolver

    assert torch.cuda.is_available()
    return DeviceSolver()


def _operands(m, n, k, salt, dtype=np.float64):
    rng = np.random.default_rng(m * 7 + n * 3 + k + salt)
    return (rng.uniform(-1, 1, (k, m)).astype(dtype), rng.uniform(-1, 1, (k, n)).astype(dtype),
            rng.uniform(-1, 1, (m, n)).astype(dtype))


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_gemm_tn_fp64_against_numpy(dev, m, n, k):
    import torch

    A, B, C = _operands(m, n, k, 11)
    dA, dB, dC = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda(), torch.from_numpy(C).cuda()
    dev.gemm_tn_sub_(dC, dA, dB)
    err = float(np.max(np.abs(dC.cpu().numpy() - (C - A.T @ B))))
    print(f"gemm_tn_sub fp64 {m}x{n}x{k}: {err:.2e} (bound {1e-13 * k:.2e})")
    assert err < 1e-13 * k
    dev.gemm_tn_add_(dC, dA, dB)      # and back
    back = float(np.max(np.abs(dC.cpu().numpy() - C)))
    print(f"  add after sub: {back:.2e}")
    assert back < 1e-13 * k
    dev.gemm_tn_add_(dC, dA, dB)
    assert float(np.max(np.abs(dC.cpu().numpy() - (C + A.T @ B)))) < 1e-13 * k


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_gemm_tn_fp32_against_the_fp64_product(dev, m, n, k):
    import torch

    A, B, C = _operands(m, n, k, 12, np.float32)
    dC = torch.from_numpy(C.copy()).cuda()
    dev.gemm_tn_sub_(dC, torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda())
    want = C.astype(np.float64) - A.astype(np.float64).T @ B.astype(np.float64)
    bound = 2 * k * U32 * float(np.abs(A).max() * np.abs(B).max()) + U32 * float(np.abs(want).max())
    err = float(np.abs(dC.cpu().numpy().astype(np.float64) - want).max())
    print(f"gemm_tn_sub fp32 {m}x{n}x{k}: {err:.2e} (bound {bound:.2e})")
    assert err <= bound


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_zero_extent_leaves_c_unchanged(dev, dtype):
    """Through the C ABI, with real buffers behind the pointers so that a stray access would show."""
    import torch

    tdt = torch.float64 if dtype == np.float64 else torch.float32
    sfx = "f64" if dtype == np.float64 else "f32"
    A = torch.full((16, 40), 2.0, dtype=tdt, device="cuda")
    B = torch.full((16, 24), 2.0, dtype=tdt, device="cuda")
    Cm = torch.full((40, 24), 3.0, dtype=tdt, device="cuda")
    fns = [getattr(dev.lib, f"lsx_gemm_tn_sub_{sfx}_dev")] + ([dev.lib.lsx_gemm_tn_add_f64_dev] if sfx == "f64" else [])
    for fn in fns:
        for m, n, k in ((0, 24, 16), (40, 0, 16), (40, 24, 0), (0, 0, 0)):
            assert fn(dev.h.ptr, m, n, k, A.data_ptr(), 40, B.data_ptr(), 24, Cm.data_ptr(), 24) == 0, (m, n, k)
            assert fn(dev.h.ptr, m, n, k, None, 40, None, 24, None, 24) == 0, "zero extents need no pointers"
    torch.cuda.synchronize()
    assert bool((Cm == 3.0).all())


def _nan_view(rows, cols, ld, offset, src):
    """(buffer, view): src as a rows x cols view at an odd element offset of a NaN-filled buffer with leading dimension ld."""
    import torch

    buf = torch.full((offset + rows * ld + 8,), float("nan"), dtype=src.dtype, device="cuda")
    view = buf[offset:offset + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(src)
    return buf, view


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("m,n,k", [(300, 200, 64), (128, 128, 128), (257, 72, 100), (500, 7, 128)])
def test_views_with_odd_leading_dimensions_match_the_aligned_call(dev, m, n, k, dtype):
    """Operands inside NaN-filled buffers, odd ld, odd offset: the bounds-checked form.  Same bits as the aligned call
    (interior tiles in the 16-byte form where the shape has any), no NaN read, nothing written outside C."""
    import torch

    A, B, C = _operands(m, n, k, 14, dtype)
    tA, tB, tC = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda(), torch.from_numpy(C).cuda()
    ref = tC.clone()
    dev.gemm_tn_sub_(ref, tA, tB)
    _, vA = _nan_view(k, m, m + 3 + (m % 2), 1, tA)           # odd leading dimensions whatever the shape
    _, vB = _nan_view(k, n, n + 5 + (n % 2), 3, tB)
    bufC, vC = _nan_view(m, n, n + 7 + (n % 2), 5, tC)
    assert vA.stride(0) % 2 == 1 and vB.stride(0) % 2 == 1 and vC.stride(0) % 2 == 1
    outside = torch.ones_like(bufC, dtype=torch.bool)
    outside[5:5 + m * vC.stride(0)].view(m, vC.stride(0))[:, :n] = False
    dev.gemm_tn_sub_(vC, vA, vB)
    torch.cuda.synchronize()
    assert torch.equal(vC, ref), "the view must get the bits of the aligned call"
    assert bool(torch.isnan(bufC[outside]).all()), "nothing outside C may be written"


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_column_does_not_depend_on_its_neighbours(dev, dtype):
    """The leading 72 columns of a 200-column call equal the 72-column call bit for bit (also 1 and 7 columns: no
    narrow-n kernel of another summation order)."""
    import torch

    m, n, k = 300, 200, 128
    A, B, C = _operands(m, n, k, 15, dtype)
    tA = torch.from_numpy(A).cuda()
    wide = torch.from_numpy(C).cuda()
    dev.gemm_tn_sub_(wide, tA, torch.from_numpy(B).cuda())
    for w in (72, 7, 1):
        part = torch.from_numpy(np.ascontiguousarray(C[:, :w])).cuda()
        dev.gemm_tn_sub_(part, tA, torch.from_numpy(np.ascontiguousarray(B[:, :w])).cuda())
        assert torch.equal(part, wide[:, :w].contiguous()), w


def test_argument_errors(dev):
    import torch

    lib, h = dev.lib, dev.h.ptr
    m, n, k = 8, 6, 4
    A = torch.zeros(k, m, dtype=torch.float64, device="cuda")
    B = torch.zeros(k, n, dtype=torch.float64, device="cuda")
    C = torch.ones(m, n, dtype=torch.float64, device="cuda")
    a, b, c = A.data_ptr(), B.data_ptr(), C.data_ptr()
    for fn in (lib.lsx_gemm_tn_sub_f64_dev, lib.lsx_gemm_tn_add_f64_dev, lib.lsx_gemm_tn_sub_f32_dev):
        assert fn(h, m, n, k, a, m - 1, b, n, c, n) == -1 and b"bad argument" in lib.lsx_last_error()   # lda < m
        assert fn(h, m, n, k, a, m, b, n - 1, c, n) == -1                                                # ldb < n
        assert fn(h, m, n, k, a, m, b, n, c, n - 1) == -1                                                # ldc < n
        assert fn(h, -1, n, k, a, m, b, n, c, n) == -1
        assert fn(h, m, -1, k, a, m, b, n, c, n) == -1
        assert fn(h, m, n, -1, a, m, b, n, c, n) == -1
        assert fn(h, m, n, k, None, m, b, n, c, n) == -1
        assert fn(h, m, n, k, a, m, None, n, c, n) == -1
        assert fn(h, m, n, k, a, m, b, n, None, n) == -1
    torch.cuda.synchronize()
    assert bool((C == 1.0).all())
    assert lib.lsx_gemm_tn_sub_f64_dev(h, m, n, k, a, m, b, n, c, n) == 0
    with pytest.raises(ValueError):
        dev.gemm_tn_sub_(C, A.t(), B)                      # not row-major
    with pytest.raises(ValueError):
        dev.gemm_tn_sub_(C, B, A)                          # shapes do not chain
    with pytest.raises(TypeError):
        dev.gemm_tn_add_(C.float(), A.float(), B.float())  # add is fp64 only
