"""Padded, offset and mis-aligned operands through the device-pointer entry points on the MI355X.

Every kernel picks a vector (16-byte) or an element-wise path from the alignment of its base pointers and the parity
of its leading dimensions.  Here every operand is a view (rows, cols, ld, offset_elems) inside a larger 1-D device
buffer that is pre-filled with NaN (`View`).  After the call

  * everything outside the view is still the same NaN, bit for bit: nothing was written to padding;
  * the result is finite: nothing was read from padding into it (a masked-out element that was loaded from padding
    and multiplied by zero would still poison it);
  * pivots, info, rank are EQUAL to those of the same call on a contiguous, 16-byte aligned copy and the values agree
    to n u relative to the largest entry (u = 2^-53 / 2^-24).  The interchanges, the fill and the gather list are pure
    data movement: bit equality.  The vector and the element-wise form of the LU, solve and update kernels take the same
    fused multiply-adds in the same order, so the tests also print whether the bits agree (they are not promised by
    include/lsx.h, so only the n u bound is asserted).

Matrices are well conditioned (a shuffled, moderately dominant diagonal: every column needs an interchange), so the
two forms cannot differ by more than rounding for a reason other than the kernels.

Which case takes which gate (offset_elems `off`, padding `pad` = ld - cols; "fast" = the 16-byte form):

  kernels_gemm.hip `aligned` (interior tiles need 16-byte bases, ld % 2 == 0 in fp64, ld % 4 == 0 in fp32, k % 16 == 0)
      fast: test_update_kernels_on_views combo "aligned" (both dtypes) and "padded_even" (fp64) at (300, 260, 128),
            (1000, 130, 128)
      slow: every combo with an offset operand or an odd ld; fp32 "padded_even" (ld % 4 == 2), "mixed32" (ld % 4 in
            {1, 2, 3}); k = 100 whatever the alignment
  kernels_gemm.hip `tiles64` (fp64 only; m % 64 == 0, n % 128 == 0, few tiles, 16-byte bases, even ld)
      fast: (1984, 128, 128) [32-row tiles] and (4032, 384, 128) [64-row tiles], combos "aligned", "padded_even"
      slow: the same shapes with "a_off", "b_off", "c_off", "odd_ld", "*_odd_only"
      (the skinny n < 16 kernel: (500, 7, 128), (64, 1, 64) under every combo)
  kernels_panel_x.hip / kernels_panel_pipe.hip `wide` (jb == 128, 16-byte base, ld % 2 == 0)
      fast: test_lu_family_on_views n = 200, 1003 with off = 0 and an even ld (panel 4), and
            test_lu_family_on_views_under_the_other_panels (panel 3)
      slow: off = 1 (fp64), off in (1, 2, 3) (fp32; off = 2 is 8-byte but not 16-byte aligned), odd ld, n = 100 (jb < 128)
  kernels_misc.hip `fast` of the 64 x 64 block inverse and of the 128-row block solve (16-byte bases, even ld)
      fast / slow: test_lu_family_on_views as for `wide`; the solves with nrhs = 130 take the block solve on B views
      whose own offset and padding rotate independently of the factor's
  kernels_misc.hip VW forms of the interchanges (16-byte base, ld % 2 == 0 in fp64 / ld % 4 == 0 in fp32, even n)
      fast: test_lu_family_on_views n = 200 pad 0 off 0 (both dtypes), fp64 n = 200 pad 2
      slow: n = 1003 (odd n), odd ld, any offset; fp32 n = 200 pad 2 (ld % 4 == 2): the class that a `% 2` test would
            let through; test_gather_list_on_views: both forms against the sequential definition
  kernels_trsv.hip `vec_ok` (16-byte base, ld % 2 == 0 in fp64 / ld % 4 == 0 in fp32), few right-hand sides (1, 8)
      fast: test_lu_family_on_views off 0 and n = 200 pad 0 / n = 1003 pad 1, 5 (ld = 1004, 1008); slow: the others
  kernels_trsvt.hip `vec` (the same condition, transposed solve, nrhs 1, 8, 9)
      fast / slow: as `vec_ok`
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEFAULT_PANEL = 4
GUARD = 1024          # elements of NaN in front of and behind every view (a multiple of 16 bytes in both dtypes)
PADS = (0, 1, 2, 3, 5)
OFFS = {"float64": (0, 1), "float32": (0, 1, 2, 3)}
U_ROUND = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}
ORDERS = (100, 200, 1003)      # below 128, above 128, ragged near 1000
NRHS = (1, 8, 9, 130)          # few-right-hand-side kernels (<= 8 per group) and the block sweeps


@pytest.fixture(scope="module")
def la():
    import linalg_solver_amd as la

    la.default_handle()
    return la


@pytest.fixture(scope="module")
def dev():
    import torch

    from linalg_solver_amd.device import DeviceSolver

    assert torch.cuda.is_available()
    return DeviceSolver()


def _tdt(dtype):
    import torch

    return torch.float64 if np.dtype(dtype) == np.float64 else torch.float32


class View:
    """rows x cols with leading dimension ld, starting offset_elems elements behind a 16-byte boundary, inside a 1-D
    NaN buffer with GUARD elements on either side."""

    def __init__(self, rows, cols, ld, offset_elems, dtype, data=None):
        import torch

        assert ld >= cols and 0 <= offset_elems
        self.total = GUARD + offset_elems + rows * ld + GUARD
        self.buf = torch.full((self.total,), float("nan"), dtype=_tdt(dtype), device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.start = GUARD + offset_elems
        self.t = torch.as_strided(self.buf, (rows, cols), (ld, 1), self.start)
        assert self.t.data_ptr() % 16 == (offset_elems * self.buf.element_size()) % 16
        inside = torch.zeros(self.total, dtype=torch.bool, device="cuda")
        torch.as_strided(inside, (rows, cols), (ld, 1), self.start).fill_(True)
        self.outside = ~inside
        self.ibits = torch.int64 if self.buf.element_size() == 8 else torch.int32
        self.canary = self.buf.view(self.ibits)[self.outside].clone()
        if data is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(data)))
            self.check_padding("the test's own copy")

    def check_padding(self, what):
        import torch

        torch.cuda.synchronize()
        now = self.buf.view(self.ibits)[self.outside]
        nbad = int((now != self.canary).sum())
        assert nbad == 0, f"{what}: {nbad} padding elements were written"

    def numpy(self):
        return self.t.cpu().numpy()


def _conditioned(n, dtype, seed):
    """Uniform entries plus a diagonal of magnitude 2 sqrt(n), rows shuffled: condition number of a few units, and
    the pivot of every column is its shuffled diagonal entry, far from a tie."""
    rng = np.random.default_rng([seed, n])
    M = rng.uniform(-1.0, 1.0, (n, n))
    M[np.arange(n), np.arange(n)] += 2.0 * np.sqrt(n) * rng.choice(np.array([-1.0, 1.0]), n)
    return M[rng.permutation(n)].astype(dtype)


def _close(got, ref, n, dtype, what):
    """max |got - ref| <= n u max |ref|; returns whether the bits agree."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and np.all(np.isfinite(got)), what
    scale = float(np.max(np.abs(ref))) if ref.size else 0.0
    err = float(np.max(np.abs(got.astype(np.float64) - ref.astype(np.float64)))) if ref.size else 0.0
    assert err <= n * U_ROUND[np.dtype(dtype).name] * scale, f"{what}: {err:.3e} against max|ref| {scale:.3e}"
    return np.array_equal(got, ref)


_REF = {}


def _reference(dev, n, dtype):
    """The whole family on contiguous, 16-byte aligned tensors, at the options in force (the panel modes agree bit
    for bit, tests/test_gpu_parity.py, so one reference serves them all)."""
    import torch

    key = (n, np.dtype(dtype).name)
    if key not in _REF:
        A = _conditioned(n, dtype, 5)
        rng = np.random.default_rng(n)
        B = rng.uniform(-1.0, 1.0, (n, max(NRHS))).astype(dtype)
        LU = torch.from_numpy(A.copy()).cuda()
        assert LU.data_ptr() % 16 == 0
        ipiv, info = dev.getrf_(LU)
        det = dev.det_parts(LU, ipiv).cpu().numpy()
        sol = {}
        for nrhs in NRHS:
            for trans in (False, True):
                X = torch.from_numpy(B[:, :nrhs].copy()).cuda()
                dev.getrs_(LU, ipiv, X, trans=trans)
                sol[(nrhs, trans)] = X.cpu().numpy()
        inv = dev.getri(LU, ipiv).cpu().numpy()
        torch.cuda.synchronize()
        assert int(info.item()) == 0
        # the reference itself is right: residuals in fp64
        A64 = A.astype(np.float64)
        tol = 64 * n * U_ROUND[key[1]]
        assert np.max(np.abs(A64 @ sol[(9, False)].astype(np.float64) - B[:, :9])) <= tol * np.sqrt(n)
        assert np.max(np.abs(A64.T @ sol[(9, True)].astype(np.float64) - B[:, :9])) <= tol * np.sqrt(n)
        assert np.max(np.abs(A64 @ inv.astype(np.float64) - np.eye(n))) <= tol
        assert int((ipiv.cpu().numpy()[:n] != np.arange(n)).sum()) > n // 2
        _REF[key] = (A, B, LU.cpu().numpy(), ipiv.cpu().numpy()[:n], det, sol, inv)
    return _REF[key]


def _lu_family(dev, n, dtype, off, pad):
    name = np.dtype(dtype).name
    A, B, rLU, ripiv, rdet, rsol, rinv = _reference(dev, n, dtype)
    offs = OFFS[name]
    va = View(n, n, n + pad, off, dtype, A)
    ipiv, info = dev.getrf_(va.t)
    va.check_padding("getrf_")
    assert int(info.item()) == 0 and np.array_equal(ipiv.cpu().numpy()[:n], ripiv)
    same = {"getrf": _close(va.numpy(), rLU, n, dtype, "getrf_")}
    det = dev.det_parts(va.t, ipiv).cpu().numpy()
    va.check_padding("det_parts")
    assert det[0] == rdet[0] and det[2] == rdet[2] and abs(det[1] - rdet[1]) <= n * U_ROUND[name] * abs(rdet[1])
    for i, nrhs in enumerate(NRHS):
        for trans in (False, True):
            # the right-hand side's own offset and padding rotate independently of the factor's
            boff = offs[(offs.index(off) + 1 + i + trans) % len(offs)]
            bpad = PADS[(PADS.index(pad) + 2 + i + 2 * trans) % len(PADS)]
            vb = View(n, nrhs, nrhs + bpad, boff, dtype, B[:, :nrhs])
            dev.getrs_(va.t, ipiv, vb.t, trans=trans)
            vb.check_padding(f"getrs_ nrhs={nrhs} trans={trans}: B")
            va.check_padding(f"getrs_ nrhs={nrhs} trans={trans}: LU")
            same[f"getrs{nrhs}{'t' if trans else ''}"] = _close(vb.numpy(), rsol[(nrhs, trans)], n, dtype,
                                                               f"getrs_ nrhs={nrhs} trans={trans} B off={boff} pad={bpad}")
    vo = View(n, n, n + PADS[(PADS.index(pad) + 1) % len(PADS)], offs[(offs.index(off) + 1) % len(offs)], dtype)
    dev.getri(va.t, ipiv, out=vo.t)
    vo.check_padding("getri: out")
    va.check_padding("getri: LU")
    same["getri"] = _close(vo.numpy(), rinv, n, dtype, "getri")
    _close(va.numpy(), rLU, n, dtype, "factors after use")
    print(f"VIEWS {name} n={n} off={off} pad={pad}: same bits as the aligned call: "
          + " ".join(f"{k}={'yes' if v else 'NO'}" for k, v in same.items()))


def _cases():
    out = []
    for dtype in (np.float64, np.float32):
        for off in OFFS[np.dtype(dtype).name]:
            for pad in PADS:
                out.append(pytest.param(dtype, off, pad, id=f"{np.dtype(dtype).name}-off{off}-pad{pad}"))
    return out


@pytest.mark.parametrize("dtype,off,pad", _cases())
@pytest.mark.parametrize("n", ORDERS)
def test_lu_family_on_views(dev, n, dtype, off, pad):
    """getrf_, det_parts, getrs_ (plain and transposed; 1, 8, 9, 130 right-hand sides on views of their own), getri
    into a padded `out`."""
    _lu_family(dev, n, dtype, off, pad)


@pytest.mark.parametrize("dtype,off,pad", [(np.float64, 0, 0), (np.float64, 0, 2), (np.float64, 1, 2), (np.float64, 0, 3),
                                           (np.float32, 0, 0), (np.float32, 0, 2), (np.float32, 2, 0), (np.float32, 3, 1)])
@pytest.mark.parametrize("panel", [0, 3])
def test_lu_family_on_views_under_the_other_panels(dev, panel, dtype, off, pad):
    """The device-scope panel (kernels_panel_pipe.hip) has a `wide` gate of its own; mode 0 is the per-column form."""
    try:
        dev.h.set_option("panel", panel)
        for n in (200, 1003):
            _lu_family(dev, n, dtype, off, pad)
    finally:
        dev.h.set_option("panel", DEFAULT_PANEL)


@pytest.mark.parametrize("off,pad", [(o, p) for o in OFFS["float32"] for p in PADS])
@pytest.mark.parametrize("n", ORDERS)
def test_refined_solve_on_views(dev, n, off, pad):
    import torch

    A = _conditioned(n, np.float32, 9)
    B = np.random.default_rng(n).uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    ref = dev.gesv_refined(torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda())
    va = View(n, n, n + pad, off, np.float32, A)
    vb = View(n, 3, 3 + PADS[(PADS.index(pad) + 3) % 5], (off + 1) % 4, np.float32, B)
    got = dev.gesv_refined(va.t, vb.t)
    va.check_padding("gesv_refined: A")
    vb.check_padding("gesv_refined: B")
    assert np.array_equal(va.numpy(), A) and np.array_equal(vb.numpy(), B), "A and B are inputs"
    X64, X32, LU, ipiv, info, stats = (t.cpu().numpy() for t in got)
    rX64, rX32, rLU, ripiv, rinfo, rstats = (t.cpu().numpy() for t in ref)
    assert info[0] == rinfo[0] == 0 and np.array_equal(ipiv, ripiv)
    bits = (_close(LU, rLU, n, np.float32, "factors"), _close(X32, rX32, n, np.float32, "X32"),
            _close(X64, rX64, n, np.float64, "X64"))
    assert np.max(np.abs(A.astype(np.float64) @ X64 - B)) <= 64 * n * U_ROUND["float64"] * np.sqrt(n)
    print(f"VIEWS gesv_refined n={n} off={off} pad={pad}: same bits (LU, X32, X64) {bits}")


@pytest.mark.parametrize("dtype,off,pad", _cases())
def test_fill_on_views(dev, dtype, off, pad):
    from linalg_solver_amd import gen

    for (m, n), kind in (((37, 53), gen.U11), ((130, 64), gen.INT5), ((1, 1), gen.U11), ((5, 300), gen.INT5)):
        v = View(m, n, n + pad, off, dtype)
        dev.fill_(v.t, kind, 11, row_off=3, col_off=5)
        v.check_padding("fill_")
        assert np.array_equal(v.numpy(), gen.fill(kind, 11, m, n, row_off=3, col_off=5, dtype=dtype))


@pytest.mark.parametrize("off,pad", [(o, p) for o in OFFS["float64"] for p in PADS])
@pytest.mark.parametrize("m,n,rank,bar", [(90, 140, 30, 120), (300, 340, 40, 320), (520, 300, 130, 280)])
def test_rref_on_views(dev, m, n, rank, bar, off, pad):
    """Rectangular and rank-deficient (integer factors: the rank is exact), both pivot rules; the small shape takes the
    per-column kernels, the others the blocked form."""
    import torch

    from linalg_solver_amd import _native

    rng = np.random.default_rng(m * 3 + n)
    A = (rng.integers(-3, 4, (m, rank)) @ rng.integers(-3, 4, (rank, n))).astype(np.float64)
    A[:, 5] = 0.0
    A[:, 17] = 2.0 * A[:, 3] - A[:, 11]
    for rule in (_native.PIVOT_MAX, _native.PIVOT_FIRST):
        R = torch.from_numpy(A.copy()).cuda()
        rpiv, rrank = dev.rref_(R, bar_col=bar, pivot_rule=rule)
        v = View(m, n, n + pad, off, np.float64, A)
        piv, rk = dev.rref_(v.t, bar_col=bar, pivot_rule=rule)
        v.check_padding("rref_")
        r = int(rk.item())
        assert r == int(rrank.item()) == np.linalg.matrix_rank(A[:, :bar])
        assert torch.equal(piv[:2 * r], rpiv[:2 * r])
        same = _close(v.numpy(), R.cpu().numpy(), max(m, n), np.float64, "rref_")
        print(f"VIEWS rref {m}x{n} rule={rule} off={off} pad={pad}: same bits {same}")


# ------------------------------------------------------------------------------------------------ the update kernels
def _combos(name):
    """(A, B, C) -> (off, pad) each.  fp32 adds the offsets 2 and 3 and the ld % 4 classes."""
    z = (0, 0)
    c = {"aligned": (z, z, z), "a_off": ((1, 0), z, z), "b_off": (z, (1, 0), z), "c_off": (z, z, (1, 0)),
         "odd_ld": ((0, 1), (0, 3), (0, 5)), "padded_even": ((0, 2), (0, 2), (0, 2)), "mixed": ((1, 5), (1, 3), (1, 1)),
         "c_odd_only": (z, z, (0, 1)), "a_odd_only": ((0, 3), z, z), "b_odd_only": (z, (0, 5), z)}
    if name == "float32":
        c.update({"a_off2": ((2, 0), z, z), "b_off3": (z, (3, 0), z), "c_off2": (z, z, (2, 0)),
                  "mixed32": ((3, 3), (2, 2), (1, 1))})
    return c


# skinny n < 16; interior + edge strips; k not a multiple of 16; 32-row and 64-row tiles (fp64, aligned); a small one
GEMM_SHAPES = [(500, 7, 128), (64, 1, 64), (300, 260, 128), (1000, 130, 128), (257, 513, 100), (129, 16, 3),
               (1984, 128, 128), (4032, 384, 128), (16, 16, 4)]


def _gemm_params():
    out = []
    for op, dtype in (("sub", np.float64), ("add", np.float64), ("sub", np.float32)):
        name = np.dtype(dtype).name
        for combo in _combos(name):
            out.append(pytest.param(op, dtype, combo, id=f"{op}-{name}-{combo}"))
    return out


@pytest.mark.parametrize("op,dtype,combo", _gemm_params())
def test_update_kernels_on_views(dev, op, dtype, combo):
    """gemm_sub_ (fp64, fp32) and gemm_add_ with each operand padded / offset on its own, against the same call on
    aligned copies and against the fp64 product (bound: 2 k u max|A| max|B| for the inner product plus one rounding
    of C)."""
    import torch

    name = np.dtype(dtype).name
    u = U_ROUND[name]
    (ao, ap), (bo, bp), (co, cp) = _combos(name)[combo]
    for m, n, k in GEMM_SHAPES:
        rng = np.random.default_rng(m * 7 + n * 3 + k)
        A, B, C = (rng.uniform(-1, 1, s).astype(dtype) for s in ((m, k), (k, n), (m, n)))
        fn = dev.gemm_sub_ if op == "sub" else dev.gemm_add_
        rC = torch.from_numpy(C.copy()).cuda()
        fn(rC, torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda())
        va, vb, vc = View(m, k, k + ap, ao, dtype, A), View(k, n, n + bp, bo, dtype, B), View(m, n, n + cp, co, dtype, C)
        fn(vc.t, va.t, vb.t)
        for v, w in ((va, "A"), (vb, "B"), (vc, "C")):
            v.check_padding(f"gemm_{op}_ {m}x{n}x{k} {combo}: {w}")
        assert np.array_equal(va.numpy(), A) and np.array_equal(vb.numpy(), B)
        prod = A.astype(np.float64) @ B.astype(np.float64)
        want = C.astype(np.float64) + (prod if op == "add" else -prod)
        got = vc.numpy()
        assert np.all(np.isfinite(got))
        bound = 2 * k * u * float(np.abs(A).max() * np.abs(B).max()) + u * float(np.abs(want).max())
        err = float(np.abs(got.astype(np.float64) - want).max())
        assert err <= bound, f"{m}x{n}x{k} {combo}: {err:.3e} > {bound:.3e}"
        same = _close(got, rC.cpu().numpy(), k, dtype, f"gemm_{op}_ {m}x{n}x{k} {combo} against the aligned call")
        if not same:
            print(f"VIEWS gemm_{op}_ {name} {m}x{n}x{k} {combo}: bits differ from the aligned call")


# ------------------------------------------------------------------------------------------------ gather lists
@pytest.mark.parametrize("off,pad,ncols", [(0, 0, 64), (0, 0, 44), (1, 0, 64), (0, 1, 64), (0, 2, 33), (1, 3, 31),
                                           (0, 2, 200), (1, 5, 1)])
def test_gather_list_on_views(dev, off, pad, ncols):
    """lsx_laswp_moves_f64_dev takes any alignment (include/lsx.h): the 16-byte form when base, ld and ncols allow it,
    the element-wise form otherwise; both move the first ncols columns of the listed rows and nothing else."""
    import torch

    rows, cols, row0 = 300, max(ncols, 70), 17
    rng = np.random.default_rng(ncols + off)
    A = rng.uniform(-1, 1, (rows, cols))
    mv = np.full((256, 2), -1, dtype=np.int32)
    cyc = rng.permutation(200)[:41]                     # a 41-cycle: every row of it is source and destination
    for i in range(40):
        mv[3 * i, 0], mv[3 * i, 1] = cyc[i], cyc[i + 1]
    mv[255] = (cyc[40], cyc[0])
    v = View(rows, cols, cols + pad, off, np.float64, A)
    dev.laswp_moves_(v.t[:, :ncols], row0, torch.from_numpy(mv.reshape(-1)).cuda())
    v.check_padding("laswp_moves_")
    want = A.copy()
    for d, s in mv:
        if d >= 0:
            want[row0 + d, :ncols] = A[row0 + s, :ncols]
    assert np.array_equal(v.numpy(), want)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_chain_head_refuses_operands_it_cannot_take(la, dtype):
    """The fused head of the look-ahead chain only has the 16-byte form of the interchanges: an offset base, a leading
    dimension or a column count that is not a whole number of 16-byte groups is LSX_ERR_ARG, and nothing is written."""
    import torch

    h = la.default_handle()
    npdt = np.float32 if dtype == "f32" else np.float64
    vw = 4 if dtype == "f32" else 2
    fn = getattr(h.lib, f"lsx_diag_chain_head_{dtype}")
    jb, ld = 128, 304
    Tm = (torch.rand(jb, ld, dtype=_tdt(npdt), device="cuda") - 0.5)
    Ti = torch.zeros(2 * 4096, dtype=_tdt(npdt), device="cuda")
    mv = torch.full((256, 2), -1, dtype=torch.int32, device="cuda")
    mv[0, 0], mv[0, 1], mv[1, 0], mv[1, 1] = 3, 9, 9, 3
    A0 = np.random.default_rng(1).uniform(-1, 1, (jb, 64)).astype(npdt)
    refused = ((1, 0, 64), (0, 1, 64), (0, 0, 63)) + (((2, 0, 64), (0, 2, 64), (0, 0, 62)) if vw == 4 else ())
    for off, pad, ncols in refused:
        v = View(jb, 64, 64 + pad, off, npdt, A0)
        torch.cuda.synchronize()
        rc = fn(h._h, 1, jb, Tm.data_ptr(), ld, Ti.data_ptr(), ncols, v.t.data_ptr(), 64 + pad, 0, mv.data_ptr())
        h.synchronize()
        assert rc == -1, (off, pad, ncols)
        v.check_padding("refused call")
        assert np.array_equal(v.numpy(), A0) and not bool(Ti.any())
    v = View(jb, 64, 64 + vw, 0, npdt, A0)          # what it does take: padded by one whole group
    torch.cuda.synchronize()
    assert fn(h._h, 1, jb, Tm.data_ptr(), ld, Ti.data_ptr(), 64, v.t.data_ptr(), 64 + vw, 0, mv.data_ptr()) == 0
    h.synchronize()
    v.check_padding("accepted call")
    want = A0.copy()
    want[[3, 9]] = A0[[9, 3]]
    assert np.array_equal(v.numpy(), want) and bool(Ti.any())
