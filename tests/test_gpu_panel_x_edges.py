"""The XCD panel (panel = 4, kernels_panel_x.hip) on the edges of its tile load and scatter.

A whole panel (128 columns, rows 16-byte aligned) travels between memory and registers through an LDS image, 64 rows at
a time; every other operand takes the direct loads and stores.  Nothing in the arithmetic depends on the way, so factors,
`ipiv`, `info` and the gather list must equal, bit for bit, those of the two independent panels kept beside it: the
device-scope pipelined panel (panel = 3) and the per-column launches (panel = 0, which emit no gather list).  Entries
are integer-valued, so equal magnitudes meet in the pivot search.

Heights: 128, 129, 191, 256, 257 (one row per lane: one workgroup, a second one with a single row, a partial 64-row slab),
2048 (32 workgroups), 2113 (two rows per lane; the last workgroup's second slab holds one row), 4097 (four rows per
lane; the last workgroup holds one row in its first slab and none in the other three)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEFAULT_PANEL = 4
HEIGHTS = [128, 129, 191, 256, 257, 2048, 2049 + 64, 4096 + 1]


@pytest.fixture(scope="module")
def dev():
    import torch

    from linalg_solver_amd.device import DeviceSolver

    assert torch.cuda.is_available()
    return DeviceSolver()


def _operand(torch, m, jb, how):
    """An m x jb fp64 view: 'aligned' (16-byte aligned base, ld = jb), 'odd_ld' (ld = jb + 1) or 'offset' (even ld, base
    one element past a 16-byte boundary).  Only the first can take the staged path, and only at jb = 128."""
    if how == "aligned":
        return torch.zeros(m, jb, dtype=torch.float64, device="cuda")
    if how == "odd_ld":
        return torch.zeros(m, jb + 1, dtype=torch.float64, device="cuda")[:, :jb]
    ld = jb + 2
    flat = torch.zeros(m * ld + 2, dtype=torch.float64, device="cuda")
    assert flat.data_ptr() % 16 == 0
    return flat[1:1 + m * ld].view(m, ld)[:, :jb]


def _run_panel(torch, dev, mode, P0, how):
    m, jb = P0.shape
    dev.h.set_option("panel", mode)
    P = _operand(torch, m, jb, how)
    P.copy_(P0)
    ipiv = torch.zeros(jb, dtype=torch.int32, device="cuda")
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    dev.panel_(P, 0, ipiv, info)
    mv = torch.zeros(512, dtype=torch.int32, device="cuda")
    listed = dev.panel_moves_(mv)
    torch.cuda.synchronize()
    return P.clone(), ipiv, int(info.item()), mv, listed


@pytest.mark.parametrize("jb,how", [(128, "aligned"), (96, "aligned"), (128, "odd_ld"), (128, "offset")])
@pytest.mark.parametrize("m", HEIGHTS)
def test_single_panel_equals_the_reference_panels_bit_for_bit(dev, m, jb, how):
    import torch

    from linalg_solver_amd import gen

    P0 = torch.empty(m, jb, dtype=torch.float64, device="cuda")
    dev.fill_(P0, gen.INT5, 11 + m)
    try:
        x = _run_panel(torch, dev, 4, P0, how)
        ref3 = _run_panel(torch, dev, 3, P0, how)
        ref0 = _run_panel(torch, dev, 0, P0, how)
    finally:
        dev.h.set_option("panel", DEFAULT_PANEL)
    assert x[4] and ref3[4] and not ref0[4]
    assert not torch.equal(x[0], P0), "the panel was not factored"
    for name, ref in (("panel=3", ref3), ("panel=0", ref0)):
        assert x[2] == ref[2] == 0, (name, x[2], ref[2])
        assert torch.equal(x[1], ref[1]), f"{name}: first differing pivot {int((x[1] != ref[1]).nonzero()[0])}"
        assert torch.equal(x[0], ref[0]), f"{name}: factors differ in {int((x[0] != ref[0]).sum())} entries"
    assert torch.equal(x[3], ref3[3]), "gather lists differ"


@pytest.mark.parametrize("m", [257, 2049 + 64])
def test_gather_list_moves_other_columns_like_the_interchanges(dev, m):
    """The `moves` list of a panel, applied to a block the panel did not touch, against `laswp` by the panel's `ipiv`."""
    import torch

    from linalg_solver_amd import gen

    jb = 128
    P0 = torch.empty(m, jb, dtype=torch.float64, device="cuda")
    dev.fill_(P0, gen.INT5, 5 + m)
    _, ipiv, info, mv, listed = _run_panel(torch, dev, 4, P0, "aligned")
    assert listed and info == 0
    piv = ipiv.cpu().numpy()
    assert np.all(piv >= np.arange(jb)) and np.all(piv < m) and np.any(piv != np.arange(jb))
    B0 = torch.empty(m, 37, dtype=torch.float64, device="cuda")
    dev.fill_(B0, gen.U11, 9)
    X1, X2 = B0.clone(), B0.clone()
    dev.laswp_moves_(X1, 0, mv)
    dev.laswp_(X2, 0, jb, ipiv)
    torch.cuda.synchronize()
    want = B0.cpu().numpy()
    for j in range(jb):       # the sequential definition
        want[[j, piv[j]]] = want[[piv[j], j]]
    assert np.array_equal(X2.cpu().numpy(), want)
    assert torch.equal(X1, X2)


@pytest.mark.parametrize("dtype,n", [("float64", 2560), ("float64", 2564), ("float32", 2560), ("float32", 2564),
                                     ("float32", 4228), ("float32", 2114)])
def test_whole_factorisation_with_look_ahead_equals_the_sequential_one(dev, dtype, n):
    """n = 2560: panels of every height from 2560 down to 128 in steps of 128, all through the staged path (fp64: one
    row per wave instruction, fp32: two).  n = 2564 and 4228 (fp32 there has no single-panel entry point, so its edges
    come from whole matrices): rows and panel bases stay 16-byte aligned, so every full panel is staged, and every
    height is 4 more than a multiple of 128 -- a last workgroup with four rows, its slabs partly or wholly empty, in
    fp32 half-empty wave instructions (two rows each) -- at four, two and one row per lane (4228: heights 4228 and 4100,
    then 3972 ... 2180, then the rest), plus a ragged 4-column last panel on the direct path.  fp32 with n = 2114: rows
    8-byte but not 16-byte aligned, the direct 8-byte path.  Against panel = 4 and panel = 3 without look-ahead."""
    import torch

    from linalg_solver_amd import gen

    dt = getattr(torch, dtype)
    A0 = torch.empty(n, n, dtype=dt, device="cuda")
    dev.fill_(A0, gen.INT5, 77 + n)
    res = []
    before = dev.h.get_option("panel_fallbacks")
    try:
        for mode, look in ((DEFAULT_PANEL, 1), (DEFAULT_PANEL, 0), (3, 0)):
            dev.h.set_option("panel", mode)
            dev.h.set_option("lookahead", look)
            A = A0.clone()
            ipiv, info = dev.getrf_(A)
            torch.cuda.synchronize()
            res.append((A, ipiv, int(info.item())))
        fallbacks = dev.h.get_option("panel_fallbacks") - before
    finally:
        dev.h.set_option("panel", DEFAULT_PANEL)
        dev.h.set_option("lookahead", 1)
    assert fallbacks == 0
    for k in (1, 2):
        assert res[0][2] == res[k][2] == 0
        assert torch.equal(res[0][1], res[k][1]) and torch.equal(res[0][0], res[k][0]), (dtype, n, k)


def test_first_non_zero_rule_through_rref(dev):
    """The body shared with the first-non-zero rule (`panel_xcd_first`, reached through a rank-deficient row reduction with
    bar_col < n): same pivots as the per-column kernels.  The two reductions order their arithmetic differently, so the
    entries are compared to 1e-9 of the largest, the bound test_gpu_parity.py holds either of them to against the exact
    rational run."""
    import linalg_solver_amd as la
    from linalg_solver_amd import _native, dense

    h = la.default_handle()
    m, n, rank, bar = 600, 400, 200, 380
    rng = np.random.default_rng(4)
    Bf = rng.integers(-2, 3, (m, rank))
    Bf[0, :] = 0           # the very first pivot needs an interchange
    Bf[5, :] = Bf[3, :]    # becomes a zero row mid-way
    A = (Bf @ rng.integers(-2, 3, (rank, n))).astype(np.float64)
    try:
        h.set_option("rref_first_fast", 1)
        R1, piv1, r1 = dense.rref(A, bar_col=bar, pivot_rule=_native.PIVOT_FIRST)
        used = h.get_option("rref_first_used")
        h.set_option("rref_first_fast", 0)
        R0, piv0, r0 = dense.rref(A, bar_col=bar, pivot_rule=_native.PIVOT_FIRST)
    finally:
        h.set_option("rref_first_fast", 1)
    assert used == 1, "the blocked first-rule form did not run"
    assert piv1 == piv0 and r1 == r0 == rank
    scale = max(1.0, float(np.max(np.abs(R0))))
    assert np.max(np.abs(R1 - R0)) / scale < 1e-9
