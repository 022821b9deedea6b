"""First calls that outgrow the scratch a new handle starts with.

`lsx_create` reserves 1 MiB of scratch, so at the sizes of the other tests the size a launcher works out for itself
never decides anything.  Here the FIRST call on a fresh handle needs more than that 1 MiB, and every output is compared
bit for bit with the same call on a second handle whose scratch a larger call of the same kind has grown before:

  pipelined panel     `lsx_panel_f64_dev`, panel = 3, 16384 x 32 in 64-row slices (panel_nt = 256, the only slicing
                      that gives this height 256 workgroups): one exchange area of 256 + 256 (2 * 512 + 2 * 128 * 16)
                      bytes = 1.25 MiB.  Panel, pivots and gather list.
  cooperative solve   option trsv = 1, n = 4224, 8 right-hand sides: two exchange areas of 4224 * 8 granules of 16
                      bytes = 1.03 MiB.  The factors come from one getrf_ of a device-filled matrix on a third handle
                      (a factorisation grows scratch itself).
  wide row reduction  m = 4, n = 70000, bar_col = 4 (per-column form): state and two rows of 70000 doubles = 1.07 MiB.

The other users of scratch cannot cross 1 MiB at a size that runs in seconds -- the three XCD exchange areas are 0.8 MiB
together at any order, ipiv_to_perm takes 8 n bytes, the blocked row reduction 12 bytes per 8 rows -- so they are not
stretched for here.  fp64.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


def _fresh_and_grown(call, larger, options=()):
    """call on a new handle, and on a new handle after `larger`: the two results as lists of arrays."""
    from linalg_solver_amd.device import DeviceSolver

    results = []
    for grow_first in (False, True):
        s = DeviceSolver()
        try:
            for key, value in options:
                s.h.set_option(key, value)
            if grow_first:
                larger(s)
            results.append([_np(x) for x in call(s)])
            s.h.check_status()
        finally:
            s.h.close()
    return results


def _assert_same_bits(label, results):
    fresh, grown = results
    assert len(fresh) == len(grown)
    for i, (f, g) in enumerate(zip(fresh, grown)):
        assert f.dtype == g.dtype and f.shape == g.shape, f"{label}: output {i}"
        assert f.tobytes() == g.tobytes(), f"{label}: output {i} of a fresh handle differs from a grown handle's"


def _panel(s, m, jb=32):
    import torch

    from linalg_solver_amd import gen

    P = s.fill_(torch.empty(m, jb, dtype=torch.float64, device="cuda"), gen.U11, 7)
    ipiv = torch.zeros(jb, dtype=torch.int32, device="cuda")
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    moves = torch.zeros(512, dtype=torch.int32, device="cuda")
    s.panel_(P, 0, ipiv, info)
    assert s.panel_moves_(moves), "the pipelined panel kernel did not run"
    return P, ipiv, info, moves


def test_pipelined_panel_first_call_above_one_mib():
    results = _fresh_and_grown(lambda s: _panel(s, 16384), lambda s: _panel(s, 32768),
                               options=(("panel", 3), ("panel_nt", 256)))
    _assert_same_bits("panel 16384 x 32", results)
    P, ipiv, info, moves = results[0]
    assert info[0] == 0 and np.isfinite(P).all()
    assert ipiv.min() >= 0 and ipiv.max() < 16384 and (ipiv >= np.arange(32)).all()


def test_cooperative_few_rhs_first_call_above_one_mib():
    import torch

    from linalg_solver_amd import gen
    from linalg_solver_amd.device import DeviceSolver

    factors = {}
    f = DeviceSolver()
    try:
        for n in (4224, 4608):
            LU = f.fill_(torch.empty(n, n, dtype=torch.float64, device="cuda"), gen.U11, 31 + n)
            ipiv, info = f.getrf_(LU)
            assert int(_np(info)[0]) == 0
            B = f.fill_(torch.empty(n, 8, dtype=torch.float64, device="cuda"), gen.U11, 5, col_off=gen.RHS_COL - 64)
            factors[n] = (LU, ipiv, B)
        f.h.check_status()
    finally:
        f.h.close()

    def solve(s, n):
        LU, ipiv, B = factors[n]
        return (s.getrs_(LU, ipiv, B.clone()),)

    results = _fresh_and_grown(lambda s: solve(s, 4224), lambda s: solve(s, 4608), options=(("trsv", 1),))
    _assert_same_bits("getrs trsv=1 n=4224 nrhs=8", results)
    assert np.isfinite(results[0][0]).all()


def test_wide_row_reduction_first_call_above_one_mib():
    import torch

    from linalg_solver_amd import gen

    def reduce(s, n):
        R = torch.from_numpy(gen.fill(gen.U11, 3, 4, n)).cuda()
        piv, rank = s.rref_(R, bar_col=4)
        return R, piv, rank

    results = _fresh_and_grown(lambda s: reduce(s, 70000), lambda s: reduce(s, 90000))
    _assert_same_bits("rref 4 x 70000", results)
    R, piv, rank = results[0]
    assert int(rank[0]) == 4 and np.array_equal(R[:, :4], np.eye(4)) and np.isfinite(R).all()
