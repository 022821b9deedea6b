"""fp32 and fp64 LU on the MI355X against answers known in advance (tests/planted.py, proved on the CPU by
tests/test_planted_host.py), and the tie rule of the pivot search where it is decided.

1. Planted factorisations.  Elimination of a planted matrix is exact in both precisions and every pivot is unique,
   so the library must return the planted interchange sequence EXACTLY, info = 0, and the planted factors to within
   8 u max|A| (u = 2^-24 / 2^-53: a handful of roundings at the scale of the entries; every CPU elimination differs
   in no entry at all -- the count of differing entries is printed).  Orders
   cross every switch of the driver (api.hip getrf_dev): one panel, the 64-row block inverses, nb = 128 and its
   multiples +-1, the look-ahead thresholds 2048 (fp64) and 4096 (fp32), ragged orders above them, and one order
   above the height at which the device-scope panel (mode 3) takes the leading panels from the XCD-scope panel
   (mode 4): xrows = 32 * 64 * (4 | 8) = 8192 rows in fp64, 16384 in fp32.  From the same factors: determinant,
   solves (plain, transposed) with a known integer solution, inverse.
2. Ties.  A = blockdiag(I_j, B): the candidates of column j are B[:, 0] exactly in any precision; equal maxima of
   mixed sign sit in chosen lanes, waves and workgroups of the panel, and the lowest row must win.
3. For every factorisation of this module, in both precisions: |L| <= 1 and the componentwise backward error
   max_ij |P A - L U|_ij / (|L| |U|)_ij <= gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical
   Algorithms, Thm 9.3), the numerator 0 wherever the denominator is.  The ratio is evaluated in fp64, for fp64
   factors up to order 320 in extended precision (_backward_ratio says what that means above 320).  Up to order
   1100 the same ratio of a same-precision numpy elimination is printed beside it.

Reference products of order > 512 are formed by torch on the GPU in fp64 (test plumbing; the planted product is exact
in any summation order).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import planted as pl  # noqa: E402

DEFAULT_PANEL = 4
ORDERS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 1537, 2048, 2075, 3001, 4096, 4131]
# api.hip getrf_dev: `int xrows = 32 * 64 * (sizeof(T) == 8 ? 4 : 8)`; panels taller than that take mode 3
ABOVE_XCD_PANEL = {"float64": 32 * 64 * 4 + 139, "float32": 32 * 64 * 8 + 139}
DTYPES = [np.float32, np.float64]
U_ROUND = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}
SEED = 11
SEED_ZERO = 13


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


def _name(dtype):
    return np.dtype(dtype).name


def _tdev(n):
    return "cuda" if n > 512 else "cpu"


def _mm(a, b):
    """fp64 product; on the GPU above order 512."""
    import torch

    if a.shape[0] <= 512:
        return a @ b
    return (torch.from_numpy(np.ascontiguousarray(a)).cuda() @ torch.from_numpy(np.ascontiguousarray(b)).cuda()).cpu().numpy()


_PLANTED = {}


def _planted(n, seed=SEED):
    """One planted system per order, kept for the module (the largest orders are dropped by their test)."""
    if (n, seed) not in _PLANTED:
        A, L, U, perm = pl.planted(n, seed, matmul=_mm)
        _PLANTED[(n, seed)] = (A, pl.planted_lu(L, U), pl.ipiv_of_perm(perm), perm, np.diag(U).copy())
    return _PLANTED[(n, seed)]


_COND = {}


def _tri_inv(T, lower):
    """Inverse of a triangular fp64 tensor by halving: inv([[a, 0], [c, d]]) = [[a', 0], [-d' c a', d']] (and the
    mirror image), blocks of order <= 512 by numpy.  Products only, so it runs wherever torch can multiply."""
    import torch

    n = T.shape[0]
    if n <= 512:
        return torch.from_numpy(np.linalg.inv(T.cpu().numpy())).to(T.device)
    h = n // 2
    a, d = _tri_inv(T[:h, :h], lower), _tri_inv(T[h:, h:], lower)
    out = torch.zeros_like(T)
    out[:h, :h], out[h:, h:] = a, d
    if lower:
        out[h:, :h] = -(d @ T[h:, :h] @ a)
    else:
        out[:h, h:] = -(a @ T[:h, h:] @ d)
    return out


def _cond_inf_from_factors(A, lu):
    """||A||_inf ||inv(U) inv(L)||_inf: A = P^T L U, and the permutation of the columns of the inverse leaves its row
    sums alone."""
    import torch

    t = torch.from_numpy(lu).cuda()
    L = torch.tril(t, -1)
    L.diagonal().fill_(1.0)
    inv = _tri_inv(torch.triu(t), False) @ _tri_inv(L, True)
    return float(np.abs(A).sum(axis=1).max()) * float(inv.abs().sum(dim=1).max())


def _cond_inf(n, A):
    """cond_inf(A) of the planted matrix of order n: numpy's inverse of A up to 2048; above that from the planted
    factors (well conditioned: tests/test_planted_host.py), with matrix products only -- no general inverse of that
    order is needed.  At 2048 the two are compared."""
    if n not in _COND:
        if n <= 2048:
            inv = np.linalg.inv(A)
            _COND[n] = float(np.abs(A).sum(axis=1).max() * np.abs(inv).sum(axis=1).max())
            if n == 2048:
                assert abs(_cond_inf_from_factors(A, _planted(n)[1]) / _COND[n] - 1) < 1e-8
        else:
            _COND[n] = _cond_inf_from_factors(A, _planted(n)[1])
    return _COND[n]


def _set(handles, **opts):
    for h in handles:
        for k, v in opts.items():
            h.set_option(k, v)


def _restore(handles):
    _set(handles, panel=DEFAULT_PANEL, lookahead=1, lookahead_min=0)


def _backward_ratio(A, LU, ipiv):
    """max |P A - L U| / (|L| |U|) from the given factors, the number of entries where the denominator is 0 and the
    numerator is not, and max |l_ij|.  Evaluated in fp64 (exact enough for fp32 factors); for fp64 factors up to
    order 320 in numpy's extended precision, so that there the evaluation's own rounding is 2^-11 of gamma_n and not
    of its order (above 320 the extended product is too slow; the fp64 evaluation then adds about sqrt(n) u)."""
    import torch

    n = A.shape[0]
    if np.asarray(LU).dtype == np.float64 and n <= 320 and np.finfo(np.longdouble).nmant > 52:
        X = np.asarray(LU).astype(np.longdouble)
        Lg = np.tril(X, -1)
        lmax = float(np.abs(Lg).max()) if n > 1 else 0.0
        Lg[np.arange(n), np.arange(n)] = 1
        Ug = np.triu(X)
        num = np.abs(A[pl.perm_of_ipiv(ipiv, n)].astype(np.longdouble) - Lg @ Ug)
        den = np.abs(Lg) @ np.abs(Ug)
        zero = den == 0
        bad = int(np.count_nonzero((num != 0) & zero))
        ratio = float(np.max(np.where(zero, 0, num / np.where(zero, 1, den))))
        return ratio, bad, lmax
    dv = _tdev(n)
    tLU = torch.from_numpy(np.ascontiguousarray(LU)).to(dv).double()
    PA = torch.from_numpy(A).to(dv)[torch.from_numpy(pl.perm_of_ipiv(ipiv, n)).to(dv)]
    Lg = torch.tril(tLU, -1)
    lmax = float(Lg.abs().max()) if n > 1 else 0.0
    Lg.diagonal().fill_(1.0)
    Ug = torch.triu(tLU)
    num = (PA - Lg @ Ug).abs_()
    den = Lg.abs_() @ Ug.abs_()
    zero = den == 0
    bad = int(((num != 0) & zero).sum())
    ratio = float((num / den.masked_fill(zero, 1.0)).masked_fill(zero, 0.0).max())
    return ratio, bad, lmax


def _check_backward(A, LU, ipiv, dtype, label, with_numpy=True):
    n = A.shape[0]
    u = U_ROUND[_name(dtype)]
    gamma = n * u / (1 - n * u)
    ratio, bad, lmax = _backward_ratio(A, LU, ipiv)
    line = f"BACKWARD {_name(dtype)} n={n} {label}: GPU {ratio:.3e} = {ratio / gamma:.3f} gamma_n, max|L| {lmax!r}"
    if with_numpy and n <= 1100:
        rLU, rpiv, _ = pl.eliminate(A, dtype)
        line += f"; numpy {_backward_ratio(A, rLU, rpiv)[0]:.3e}"
    print(line)
    assert lmax <= 1.0
    assert bad == 0, "P A - L U must vanish wherever |L| |U| does"
    assert ratio <= gamma


def _check_planted_factors(n, dtype, LU, ipiv, info, label):
    A, want_lu, want_piv, _, _ = _planted(n)
    u = U_ROUND[_name(dtype)]
    assert info == 0
    assert LU.dtype == dtype, label
    assert np.array_equal(ipiv, want_piv), f"{label}: first differing column {int(np.nonzero(ipiv != want_piv)[0][0])} of {n}"
    d = np.abs(LU.astype(np.float64) - want_lu)
    amax = float(np.abs(A).max())
    print(f"PLANTED {_name(dtype)} n={n} {label}: entries differing {int(np.count_nonzero(d))}, "
          f"max difference {float(d.max()):.3e} (bound {8 * u * amax:.3e})")
    assert float(d.max()) <= 8 * u * amax


def _factor_on_device(dev, A, dtype):
    import torch

    dA = torch.from_numpy(A.astype(dtype)).cuda()
    dpiv, dinfo = dev.getrf_(dA)
    torch.cuda.synchronize()
    return dA, dpiv, int(dinfo.item())


def _solve_checks(n, dtype, A, X, X0, B, label, trans=False):
    """Normwise backward error <= n u; forward error <= 4 n u cond_inf(A) wherever that is below 1e-3 (printed
    everywhere: substitution on these factors is exact on the CPU)."""
    u = U_ROUND[_name(dtype)]
    X = X.astype(np.float64)
    M = A.T if trans else A
    ninf = lambda V: float(np.abs(V).sum(axis=1).max())   # noqa: E731
    assert np.all(np.isfinite(X))
    bwd = ninf(B - M @ X) / (ninf(M) * ninf(X) + ninf(B))
    fwd = float(np.abs(X - X0).max() / np.abs(X0).max())
    cond = _cond_inf(n, A)
    fbound = 4 * n * u * cond
    print(f"SOLVE {_name(dtype)} n={n} {label}: backward {bwd:.3e} (bound {n * u:.3e}), forward {fwd:.3e} "
          f"(bound {fbound:.3e}{'' if fbound < 1e-3 else ', not asserted'})")
    assert bwd <= n * u
    if fbound < 1e-3:
        assert fwd <= fbound


def _planted_case(la, dev, n, dtype, drop=False):
    """Both entry points at the default options, then everything that is computed from the factors."""
    import torch

    from linalg_solver_amd import dense

    A, want_lu, want_piv, perm, diag_u = _planted(n)
    u = U_ROUND[_name(dtype)]
    LU, ipiv, info = dense.lu_factor(A.astype(dtype), dtype=dtype)
    _check_planted_factors(n, dtype, LU, ipiv, info, "lu_factor")
    dLU, dpiv, dinfo = _factor_on_device(dev, A, dtype)
    _check_planted_factors(n, dtype, dLU.cpu().numpy(), dpiv.cpu().numpy()[:n], dinfo, "getrf_")
    assert np.array_equal(dLU.cpu().numpy(), LU), "the host-buffer and the device-pointer entry point must agree bit for bit"
    _check_backward(A, LU, ipiv, dtype, "planted")

    # determinant: sign and log2|det| are exact integers
    sign, mant, ex = (float(v) for v in dev.det_parts(dLU, dpiv).cpu().numpy())
    want_sign = pl.perm_sign(perm) * float(np.prod(np.sign(diag_u)))
    want_log2 = float(np.sum(np.log2(np.abs(diag_u))))
    print(f"DET {_name(dtype)} n={n}: sign {sign} mant {mant!r} exp2 {ex}; expected sign {want_sign} log2|det| {want_log2}")
    assert sign == want_sign
    assert abs(np.log2(mant) + ex - want_log2) <= n * u

    # solves with a known integer solution: B = A X0 (A^T X0) is exact in fp32
    rng = np.random.default_rng(n)
    for nrhs in (1, 3, 17):
        X0 = rng.integers(-3, 4, (n, nrhs)).astype(np.float64)
        X0[0, :] = 3.0
        B = A @ X0
        assert np.array_equal(B.astype(np.float32).astype(np.float64), B)
        _solve_checks(n, dtype, A, dense.lu_solve(LU, ipiv, B.astype(dtype)), X0, B, f"lu_solve nrhs={nrhs}")
        dB = torch.from_numpy(B.astype(dtype)).cuda()
        dev.getrs_(dLU, dpiv, dB)
        _solve_checks(n, dtype, A, dB.cpu().numpy(), X0, B, f"getrs_ nrhs={nrhs}")
        Bt = A.T @ X0
        dBt = torch.from_numpy(Bt.astype(dtype)).cuda()
        dev.getrs_(dLU, dpiv, dBt, trans=True)
        _solve_checks(n, dtype, A, dBt.cpu().numpy(), X0, Bt, f"getrs_ trans nrhs={nrhs}", trans=True)
        _solve_checks(n, dtype, A, dense.lu_solve(LU, ipiv, Bt.astype(dtype), trans=True), X0, Bt,
                      f"lu_solve trans nrhs={nrhs}", trans=True)

    # inverse
    Ainv = dev.getri(dLU, dpiv)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(Ainv).all())
    dv = _tdev(n)
    R = torch.from_numpy(A).to(dv) @ Ainv.to(dv).double() - torch.eye(n, dtype=torch.float64, device=dv)
    res = float(R.abs().sum(dim=1).max())
    bound = n * u * _cond_inf(n, A)
    print(f"GETRI {_name(dtype)} n={n}: ||A Ainv - I||_inf {res:.3e} (bound n u cond_inf(A) = {bound:.3e})")
    assert res <= bound
    if drop:
        _PLANTED.pop((n, SEED), None)
        _COND.pop(n, None)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n", ORDERS)
def test_planted_factorisation_and_what_follows_from_it(la, dev, n, dtype):
    _planted_case(la, dev, n, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_planted_factorisation_above_the_xcd_panel_height(la, dev, dtype):
    """The leading panels are taller than one XCD holds and go to the device-scope panel."""
    _planted_case(la, dev, ABOVE_XCD_PANEL[_name(dtype)], dtype, drop=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n", [n for n in ORDERS if n <= 1000])
def test_planted_factorisation_under_every_panel_and_driver(la, dev, n, dtype):
    from linalg_solver_amd import dense

    A = _planted(n)[0]
    handles = (la.default_handle(), dev.h)
    try:
        for panel in (0, 3, 4):
            for look in (0, 1):
                _set(handles, panel=panel, lookahead=look, lookahead_min=128)
                LU, ipiv, info = dense.lu_factor(A.astype(dtype), dtype=dtype)
                _check_planted_factors(n, dtype, LU, ipiv, info, f"lu_factor panel={panel} lookahead={look}")
                dLU, dpiv, dinfo = _factor_on_device(dev, A, dtype)
                _check_planted_factors(n, dtype, dLU.cpu().numpy(), dpiv.cpu().numpy()[:n], dinfo,
                                       f"getrf_ panel={panel} lookahead={look}")
    finally:
        _restore(handles)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("panel", [0, 3, 4])
@pytest.mark.parametrize("k", [5, 200, 299])      # first panel, second panel, last column
def test_planted_zero_pivot(la, dev, k, panel, dtype):
    from linalg_solver_amd import dense

    n = 300
    A, _, _, perm = pl.planted(n, SEED_ZERO, zero_at=k)
    want = pl.ipiv_of_perm(perm)
    handles = (la.default_handle(), dev.h)
    try:
        _set(handles, panel=panel)
        _, ipiv, info = dense.lu_factor(A.astype(dtype), dtype=dtype)
        _, dpiv, dinfo = _factor_on_device(dev, A, dtype)
    finally:
        _restore(handles)
    assert info == k + 1 and np.array_equal(ipiv[:k], want[:k])
    assert dinfo == k + 1 and np.array_equal(dpiv.cpu().numpy()[:k], want[:k])


# ------------------------------------------------------------------------------------------------ ties
def _row_sets(m):
    return {"first_last": (0, m - 1), "63_64": (63, 64), "255_256": (255, 256), "1_last": (1, m - 1),
            "last_two": (m - 2, m - 1), "all": tuple(range(m))}


TIE_SHAPES = [(300, 0), (300, 5), (640, 127), (1000, 128), (1000, 200), (2600, 200), (4100, 0), (4100, 128)]
TIE_SETS = ["first_last", "63_64", "255_256", "1_last", "last_two", "all"]


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("which", TIE_SETS)
@pytest.mark.parametrize("n,j", TIE_SHAPES)
def test_lowest_row_wins_a_tie(dev, n, j, which, dtype):
    """Equal maxima in different lanes ({63, 64}: a wave boundary), waves and workgroups ({255, 256}; first and last
    row of the panel) and in every row at once.  Panel 0, 3 and 4 on the device-pointer entry point, each with
    |L| <= 1 and the backward error of its factors."""
    import torch

    rows = _row_sets(n - j)[which]
    A = pl.tie_matrix(n, j, rows, 3, dtype)
    assert np.array_equal(A.astype(dtype).astype(np.float64), A)
    dA0 = torch.from_numpy(A.astype(dtype)).cuda()
    try:
        for panel in (0, 3, 4):
            _set((dev.h,), panel=panel)
            dA = dA0.clone()
            dpiv, dinfo = dev.getrf_(dA)
            torch.cuda.synchronize()
            ipiv = dpiv.cpu().numpy()[:n]
            assert int(dinfo.item()) == 0, panel
            assert np.array_equal(ipiv[:j], np.arange(j)), panel
            assert int(ipiv[j]) == j + min(rows), f"panel={panel}: column {j} took row {int(ipiv[j])}, equal maxima at {rows[:4]}..."
            _check_backward(A, dA.cpu().numpy(), ipiv, dtype, f"ties j={j} rows={which} panel={panel}", with_numpy=panel == 4)
    finally:
        _restore((dev.h,))
