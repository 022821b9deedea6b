"""numpy-level entry points over the C ABI (contiguous fp64 / fp32 buffers).

This is the marshalling-free boundary: `Matrix` (matrix.py) converts its
list-of-lists into one contiguous array and calls these.  Every function runs
on the GPU through liblsx.so; none has a CPU implementation.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Tuple

import numpy as np

from . import _native as N

EPS64 = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)


def _f64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a: np.ndarray, ct):
    return a.ctypes.data_as(C.POINTER(ct))


def _h(handle: Optional[N.Handle]) -> N.Handle:
    return handle if handle is not None else N.default_handle()


def lu_factor(a, handle: Optional[N.Handle] = None, dtype=np.float64) -> Tuple[np.ndarray, np.ndarray, int]:
    """P A = L U (partial pivoting).  Returns (LU, ipiv, info); ipiv is 0-based LAPACK style."""
    h = _h(handle)
    LU = np.array(a, dtype=dtype, order="C", copy=True)
    n = LU.shape[0]
    if LU.ndim != 2 or LU.shape[1] != n:
        raise ValueError("lu_factor needs a square matrix")
    ipiv = np.zeros(max(n, 1), dtype=np.int32)
    info = C.c_int(0)
    if dtype == np.float64:
        N.check(h.lib.lsx_getrf_f64(h.ptr, n, _ptr(LU, C.c_double), n, _ptr(ipiv, C.c_int32), C.byref(info)), "lsx_getrf_f64")
    elif dtype == np.float32:
        N.check(h.lib.lsx_getrf_f32(h.ptr, n, _ptr(LU, C.c_float), n, _ptr(ipiv, C.c_int32), C.byref(info)), "lsx_getrf_f32")
    else:
        raise TypeError("dtype must be float64 or float32")
    return LU, ipiv[:n], info.value


def cho_factor(a, handle: Optional[N.Handle] = None, dtype=np.float64) -> Tuple[np.ndarray, int]:
    """Cholesky factorisation A = U^T U of a symmetric positive definite matrix (lsx_potrf_*).  Only the upper triangle
    of a is used; symmetry is not checked.  Returns (U, info): U is upper triangular with zeros below the diagonal;
    info = j + 1 says the leading minor of order j + 1 is not positive definite (then only U[:j, :j] is meaningful)."""
    ct, sfx = _ct(dtype)
    U = np.array(a, dtype=dtype, order="C", copy=True)
    n = U.shape[0]
    if U.ndim != 2 or U.shape[1] != n:
        raise ValueError("cho_factor needs a square matrix")
    h = _h(handle)
    info = C.c_int(0)
    if n:
        N.check(getattr(h.lib, f"lsx_potrf_{sfx}")(h.ptr, n, _ptr(U, ct), n, C.byref(info)), f"lsx_potrf_{sfx}")
    return np.triu(U), info.value


def cho_solve(U: np.ndarray, b, handle: Optional[N.Handle] = None) -> np.ndarray:
    """Solve A X = B from the factor of cho_factor: X = inv(U) inv(U^T) B (lsx_potrs_*).  Only the upper triangle of U
    is used."""
    U = np.asarray(U)
    if U.ndim != 2 or U.shape[0] != U.shape[1]:
        raise ValueError("cho_solve needs the square factor matrix")
    ct, sfx = _ct(U.dtype)
    n = U.shape[0]
    if np.shape(b)[:1] != (n,):
        raise ValueError("right-hand side has the wrong number of rows")
    h = _h(handle)
    U = np.ascontiguousarray(U)
    X = np.array(b, dtype=U.dtype, order="C", copy=True)
    vec = X.ndim == 1
    if vec:
        X = X.reshape(n, 1).copy()
    if n and X.shape[1]:
        N.check(getattr(h.lib, f"lsx_potrs_{sfx}")(h.ptr, n, X.shape[1], _ptr(U, ct), n, _ptr(X, ct), X.shape[1]),
                f"lsx_potrs_{sfx}")
    return X[:, 0].copy() if vec else X


def cho_inverse(U: np.ndarray, handle: Optional[N.Handle] = None) -> np.ndarray:
    """inv(A) from the factor of cho_factor (lsx_potri_*: inv(A) = V^T V with V = inv(U^T), n^3 flops with the
    factorisation, no pivoting).  Only the upper triangle of U is used.  Returns the full inverse, both triangles,
    exactly symmetric.  A zero or NaN u_ii raises ValueError (cho_factor's info says so beforehand)."""
    U = np.asarray(U)
    if U.ndim != 2 or U.shape[0] != U.shape[1]:
        raise ValueError("cho_inverse needs the square factor matrix")
    ct, sfx = _ct(U.dtype)
    n = U.shape[0]
    h = _h(handle)
    X = np.array(U, dtype=U.dtype, order="C", copy=True)
    info = C.c_int(0)
    if n:
        N.check(getattr(h.lib, f"lsx_potri_{sfx}")(h.ptr, n, _ptr(X, ct), n, C.byref(info)), f"lsx_potri_{sfx}")
    if info.value != 0:
        raise ValueError(f"cho_inverse: u[{info.value - 1}, {info.value - 1}] is zero or NaN, the factor has no inverse")
    X = np.triu(X)
    return X + np.triu(X, 1).T


def qr_factor(a, dtype=np.float64, handle: Optional[N.Handle] = None) -> Tuple[np.ndarray, np.ndarray]:
    """Householder QR of an m x n matrix (lsx_geqrf_*).  Returns (QR, tau) in LAPACK's layout: R on and above the
    diagonal, reflector j below the diagonal of column j (v_jj = 1 implied), tau of length min(m, n)."""
    ct, sfx = _ct(dtype)
    QR = np.array(a, dtype=dtype, order="C", copy=True)
    if QR.ndim != 2:
        raise ValueError("qr_factor needs a matrix")
    m, n = QR.shape
    tau = np.zeros(min(m, n), dtype=dtype)
    if min(m, n):
        h = _h(handle)
        N.check(getattr(h.lib, f"lsx_geqrf_{sfx}")(h.ptr, m, n, _ptr(QR, ct), n, _ptr(tau, ct)), f"lsx_geqrf_{sfx}")
    return QR, tau


def qr_multiply(QR: np.ndarray, tau: np.ndarray, c, trans: bool = True, handle: Optional[N.Handle] = None) -> np.ndarray:
    """Q^T c (trans=True) or Q c from the result of qr_factor, Q = H_0 .. H_{k-1} with k = len(tau) (lsx_ormqr_*)."""
    QR = np.ascontiguousarray(QR)
    if QR.ndim != 2:
        raise ValueError("qr_multiply needs the factored matrix")
    ct, sfx = _ct(QR.dtype)
    m, k = QR.shape[0], len(tau)
    if np.shape(c)[:1] != (m,):
        raise ValueError("qr_multiply: c has the wrong number of rows")
    tau = np.ascontiguousarray(tau, dtype=QR.dtype)
    X = np.array(c, dtype=QR.dtype, order="C", copy=True)
    vec = X.ndim == 1
    if vec:
        X = X.reshape(m, 1).copy()
    if m and k and X.shape[1]:
        h = _h(handle)
        N.check(getattr(h.lib, f"lsx_ormqr_{sfx}")(h.ptr, 1 if trans else 0, m, X.shape[1], k, _ptr(QR, ct), QR.shape[1],
                                                  _ptr(tau, ct), _ptr(X, ct), X.shape[1]), f"lsx_ormqr_{sfx}")
    return X[:, 0].copy() if vec else X


def qr(a, dtype=np.float64, handle: Optional[N.Handle] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(Q, R) of an m x n matrix with m >= n: the thin Q (m x n, lsx_orgqr_*) and the n x n upper triangular R."""
    QR, tau = qr_factor(a, dtype=dtype, handle=handle)
    m, n = QR.shape
    if m < n:
        raise ValueError("qr needs a matrix with at least as many rows as columns")
    ct, sfx = _ct(dtype)
    Q = np.zeros((m, n), dtype=dtype)
    if n:
        h = _h(handle)
        N.check(getattr(h.lib, f"lsx_orgqr_{sfx}")(h.ptr, m, n, n, _ptr(QR, ct), n, _ptr(tau, ct), _ptr(Q, ct), n),
                f"lsx_orgqr_{sfx}")
    return Q, np.triu(QR[:n, :])


def lstsq(a, b, dtype=np.float64, handle: Optional[N.Handle] = None):
    """Least-squares solution of an overdetermined system through Householder QR (lsx_gels_*): min ||b - a x||_2 for an
    m x n matrix with m >= n.  Returns (x, resid, info): resid holds ||b - a x||_2 per right-hand side; info = i + 1
    says r_ii is zero or NaN (a does not have full column rank to working precision): x is then None and resid +inf."""
    ct, sfx = _ct(dtype)
    A = np.array(a, dtype=dtype, order="C", copy=True)
    if A.ndim != 2 or A.shape[0] < A.shape[1]:
        raise ValueError("lstsq needs a matrix with at least as many rows as columns")
    m, n = A.shape
    if np.shape(b)[:1] != (m,):
        raise ValueError("right-hand side has the wrong number of rows")
    B = np.array(b, dtype=dtype, order="C", copy=True)
    vec = B.ndim == 1
    if vec:
        B = B.reshape(m, 1).copy()
    nrhs = B.shape[1]
    X = np.zeros((n, nrhs), dtype=dtype)
    resid = np.zeros(nrhs, dtype=np.float64)
    info = C.c_int(0)
    if n and nrhs:
        h = _h(handle)
        N.check(getattr(h.lib, f"lsx_gels_{sfx}")(h.ptr, m, n, nrhs, _ptr(A, ct), n, _ptr(B, ct), nrhs, _ptr(X, ct), nrhs,
                                                 _ptr(resid, C.c_double), C.byref(info)), f"lsx_gels_{sfx}")
    if info.value != 0:
        return None, (resid[0] if vec else resid), info.value
    return (X[:, 0].copy() if vec else X), (float(resid[0]) if vec else resid), 0


def svd(a, compute_uv: bool = True, dtype=np.float64, handle: Optional[N.Handle] = None):
    """One-sided Jacobi SVD of an m x n matrix (lsx_gesvdj_*): returns (U, s, Vt, info) with the thin factors U (m x k),
    Vt (k x n), k = min(m, n), and s (k float64 values, descending) -- U and Vt are None with compute_uv=False.  info = 1
    says the last allowed sweep still rotated (option "gesvdj_max_sweeps"); the results are returned all the same.
    U is orthonormal for every input; the rows of Vt that belong to an exactly zero singular value are zero rows.  A NaN
    or infinity in a gives s all NaN."""
    ct, sfx = _ct(dtype)
    A = np.ascontiguousarray(a, dtype=dtype)
    if A.ndim != 2:
        raise ValueError("svd needs a matrix")
    m, n = A.shape
    k = min(m, n)
    s = np.zeros(k, dtype=np.float64)
    U = np.zeros((m, k), dtype=dtype) if compute_uv else None
    Vt = np.zeros((k, n), dtype=dtype) if compute_uv else None
    info = C.c_int(0)
    if k:
        h = _h(handle)
        N.check(getattr(h.lib, f"lsx_gesvdj_{sfx}")(h.ptr, 1 if compute_uv else 0, m, n, _ptr(A, ct), n, _ptr(s, C.c_double),
                                                   _ptr(U, ct) if compute_uv else None, k,
                                                   _ptr(Vt, ct) if compute_uv else None, n, C.byref(info)),
                f"lsx_gesvdj_{sfx}")
    return U, s, Vt, info.value


def svdvals(a, dtype=np.float64, handle: Optional[N.Handle] = None) -> np.ndarray:
    """The singular values of a, descending (lsx_gesvdj_* with jobz = 0: the bits svd returns)."""
    return svd(a, compute_uv=False, dtype=dtype, handle=handle)[1]


def eigh(a, eigvals_only: bool = False, dtype=np.float64, handle: Optional[N.Handle] = None):
    """Eigenvalues and eigenvectors of a symmetric matrix by two-sided Jacobi (lsx_syevj_*): returns (w, V, info) with w
    (n float64 values, ascending) and V (n x n, column i the eigenvector of w[i], so a = V diag(w) V^T) -- V is None with
    eigvals_only=True.  Symmetry is the caller's assertion: only the upper triangle of a is used.  info = 1 says the last
    allowed sweep still rotated (option "syevj_max_sweeps"); the results are returned all the same.  A NaN or infinity in
    the upper triangle gives w all NaN."""
    ct, sfx = _ct(dtype)
    A = np.ascontiguousarray(a, dtype=dtype)
    if A.ndim != 2 or A.shape[0] != A.shape[1]:
        raise ValueError("eigh needs a square matrix")
    n = A.shape[0]
    w = np.zeros(n, dtype=np.float64)
    V = None if eigvals_only else np.zeros((n, n), dtype=dtype)
    info = C.c_int(0)
    if n:
        h = _h(handle)
        N.check(getattr(h.lib, f"lsx_syevj_{sfx}")(h.ptr, 0 if eigvals_only else 1, n, _ptr(A, ct), n, _ptr(w, C.c_double),
                                                  None if eigvals_only else _ptr(V, ct), n, C.byref(info)),
                f"lsx_syevj_{sfx}")
    return w, V, info.value


def eigvalsh(a, dtype=np.float64, handle: Optional[N.Handle] = None) -> np.ndarray:
    """The eigenvalues of a symmetric matrix, ascending (lsx_syevj_* with jobz = 0: the bits eigh returns)."""
    return eigh(a, eigvals_only=True, dtype=dtype, handle=handle)[0]


def lstsq_min_norm(a, b, rcond: Optional[float] = None, dtype=np.float64, handle: Optional[N.Handle] = None):
    """The minimum-norm solution of min ||b - a x||_2 for a matrix of any shape and rank, through the SVD (lsx_gelss_*).
    Returns (x, resid, rank, s): resid holds ||b - a x||_2 per right-hand side, rank counts the singular values above
    rcond * s[0] (rcond=None: max(m, n) times the unit roundoff), s the singular values."""
    ct, sfx = _ct(dtype)
    A = np.ascontiguousarray(a, dtype=dtype)
    if A.ndim != 2:
        raise ValueError("lstsq_min_norm needs a matrix")
    m, n = A.shape
    if np.shape(b)[:1] != (m,):
        raise ValueError("right-hand side has the wrong number of rows")
    B = np.ascontiguousarray(b, dtype=dtype)
    vec = B.ndim == 1
    if vec:
        B = B.reshape(m, 1)
    nrhs = B.shape[1]
    k = min(m, n)
    X = np.zeros((n, nrhs), dtype=dtype)
    s = np.zeros(k, dtype=np.float64)
    resid = np.zeros(max(nrhs, 1), dtype=np.float64)
    rank, info = C.c_int(0), C.c_int(0)
    if k and nrhs:
        h = _h(handle)
        N.check(getattr(h.lib, f"lsx_gelss_{sfx}")(h.ptr, m, n, nrhs, _ptr(A, ct), n, _ptr(B, ct), nrhs, _ptr(X, ct), nrhs,
                                                  -1.0 if rcond is None else float(rcond), _ptr(s, C.c_double),
                                                  _ptr(resid, C.c_double), C.byref(rank), C.byref(info)), f"lsx_gelss_{sfx}")
    elif k:
        s = svdvals(A, dtype=dtype, handle=handle)
    elif nrhs:
        resid[:nrhs] = np.sqrt((B.astype(np.float64) ** 2).sum(axis=0))   # n == 0: x is empty and the residual is b
    resid = resid[:nrhs]
    return (X[:, 0].copy() if vec else X), (float(resid[0]) if vec else resid), rank.value, s


def pinv(a, rcond: Optional[float] = None, dtype=np.float64, handle: Optional[N.Handle] = None) -> np.ndarray:
    """The Moore-Penrose pseudo-inverse (n x m): lsx_gelss_* with the identity as right-hand sides."""
    A = np.ascontiguousarray(a, dtype=dtype)
    if A.ndim != 2:
        raise ValueError("pinv needs a matrix")
    return lstsq_min_norm(A, np.eye(A.shape[0], dtype=dtype), rcond=rcond, dtype=dtype, handle=handle)[0]


def matrix_rank(a, rcond: Optional[float] = None, dtype=np.float64, handle: Optional[N.Handle] = None) -> int:
    """The number of singular values above rcond * s[0] (rcond=None: max(m, n) times the unit roundoff)."""
    A = np.ascontiguousarray(a, dtype=dtype)
    if A.ndim != 2:
        raise ValueError("matrix_rank needs a matrix")
    s = svdvals(A, dtype=dtype, handle=handle)
    if not len(s):
        return 0
    if rcond is None:
        rcond = max(A.shape) * (EPS64 if dtype == np.float64 else EPS32) / 2
    return int(np.sum(s > rcond * s[0]))


def _norm_code(which) -> int:
    """1 / "1" / "one" -> the 1-norm (max column sum); inf / "inf" / "I" -> the infinity-norm (max row sum)."""
    if which in (1, "1", "one", "O", "o"):
        return N.NORM_ONE
    if which in (np.inf, math.inf, "inf", "I", "i"):
        return N.NORM_INF
    raise ValueError(f"norm must be 1 or inf, got {which!r}")


def lu_solve(LU: np.ndarray, ipiv: np.ndarray, b, handle: Optional[N.Handle] = None, trans: bool = False) -> np.ndarray:
    """Solve A X = B from the factors of A; trans=True solves A^T X = B from the same factors (lsx_getrs_t_*)."""
    LU = np.asarray(LU)
    if LU.ndim != 2 or LU.shape[0] != LU.shape[1]:
        raise ValueError("lu_solve needs the square factor matrix")
    if LU.dtype not in (np.float64, np.float32):
        raise TypeError("dtype must be float64 or float32")
    if np.shape(b)[:1] != (LU.shape[0],):
        raise ValueError("right-hand side has the wrong number of rows")
    h = _h(handle)
    dt = LU.dtype
    LU = np.ascontiguousarray(LU)
    n = LU.shape[0]
    X = np.array(b, dtype=dt, order="C", copy=True)
    vec = X.ndim == 1
    if vec:
        X = X.reshape(n, 1).copy()
    if X.shape[0] != n:
        raise ValueError("right-hand side has the wrong number of rows")
    ipiv = np.ascontiguousarray(ipiv, dtype=np.int32)
    ct, sfx = _ct(dt)
    name = f"lsx_getrs_t_{sfx}" if trans else f"lsx_getrs_{sfx}"
    N.check(getattr(h.lib, name)(h.ptr, n, X.shape[1], _ptr(LU, ct), n, _ptr(ipiv, C.c_int32), _ptr(X, ct),
                                 X.shape[1]), name)
    return X[:, 0].copy() if vec else X


def _solve_trans(h, A, X, dtype):
    """A^T X = B: factor A once, then the transposed solve from its factors; pivot_ratio as lsx_gesv_* computes it."""
    n = A.shape[0]
    if n == 0:
        return 0, 1.0
    LU, ipiv, info = lu_factor(A, h, dtype)
    amax = float(np.max(np.abs(A)))
    ratio = float(np.min(np.abs(np.diagonal(LU)))) / amax if amax > 0 else 0.0
    if info == 0 and X.shape[1] > 0:
        X[:, :] = lu_solve(LU, ipiv, X, h, trans=True)
    return info, ratio


def solve(a, b, handle: Optional[N.Handle] = None, dtype=np.float64, trans: bool = False, assume_pos: bool = False):
    """Solve A X = B (trans=True: A^T X = B, from the factors of A -- no transposed copy, no second
    factorisation).  Returns (X, info, pivot_ratio); X is None when info != 0.
    assume_pos=True: A is symmetric positive definite and goes through the Cholesky factorisation (lsx_posv_*: no
    pivoting, half the work).  Only the upper triangle of a is used and symmetry is not checked; trans makes no
    difference; info = j + 1 says the leading minor of order j + 1 is not positive definite; pivot_ratio is 1.0
    (nothing is pivoted)."""
    A = np.ascontiguousarray(a, dtype=dtype)
    n = A.shape[0]
    if A.ndim != 2 or A.shape[1] != n:
        raise ValueError("solve needs a square matrix")
    if np.shape(b)[:1] != (n,):
        raise ValueError("right-hand side has the wrong number of rows")
    h = _h(handle)
    X = np.array(b, dtype=dtype, order="C", copy=True)
    vec = X.ndim == 1
    if vec:
        X = X.reshape(n, 1).copy()
    if X.shape[0] != n:
        raise ValueError("right-hand side has the wrong number of rows")
    if assume_pos:
        ct, sfx = _ct(dtype)
        pinfo = C.c_int(0)
        if n and X.shape[1]:
            N.check(getattr(h.lib, f"lsx_posv_{sfx}")(h.ptr, n, X.shape[1], _ptr(A, ct), n, _ptr(X, ct), X.shape[1],
                                                       C.byref(pinfo)), f"lsx_posv_{sfx}")
        elif n:
            pinfo = C.c_int(cho_factor(A, h, dtype)[1])
        if pinfo.value != 0:
            return None, pinfo.value, 1.0
        return (X[:, 0].copy() if vec else X), 0, 1.0
    if trans:
        _ct(dtype)
        tinfo, tratio = _solve_trans(h, A, X, dtype)
        if tinfo != 0:
            return None, tinfo, tratio
        return (X[:, 0].copy() if vec else X), 0, tratio
    info, ratio = C.c_int(0), C.c_double(1.0)
    if dtype == np.float64:
        N.check(h.lib.lsx_gesv_f64(h.ptr, n, X.shape[1], _ptr(A, C.c_double), n, _ptr(X, C.c_double), X.shape[1],
                                   C.byref(info), C.byref(ratio)), "lsx_gesv_f64")
    else:
        N.check(h.lib.lsx_gesv_f32(h.ptr, n, X.shape[1], _ptr(A, C.c_float), n, _ptr(X, C.c_float), X.shape[1],
                                   C.byref(info), C.byref(ratio)), "lsx_gesv_f32")
    if info.value != 0:
        return None, info.value, ratio.value
    return (X[:, 0].copy() if vec else X), 0, ratio.value


def _ct(dtype):
    if dtype == np.float64:
        return C.c_double, "f64"
    if dtype == np.float32:
        return C.c_float, "f32"
    raise TypeError("dtype must be float64 or float32")


def norm(a, which=1, handle: Optional[N.Handle] = None, dtype=np.float64) -> float:
    """Max absolute column sum (which=1) or row sum (which=inf) of a 2-D array, computed on the GPU
    (lsx_lange_*_dev; sums in fp64, fixed order)."""
    code = _norm_code(which)
    ct, sfx = _ct(dtype)
    A = np.ascontiguousarray(a, dtype=dtype)
    if A.ndim != 2:
        raise ValueError("norm needs a 2-D array")
    if A.size == 0:
        return 0.0
    import torch

    h = _h(handle)
    dev = torch.device("cuda", h.device)
    dA = torch.from_numpy(A).to(dev)
    out = torch.zeros(1, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    N.check(getattr(h.lib, f"lsx_lange_{sfx}_dev")(h.ptr, code, A.shape[0], A.shape[1], dA.data_ptr(), A.shape[1],
                                                    out.data_ptr()), f"lsx_lange_{sfx}_dev")
    h.synchronize()
    return float(out.item())


def rcond(a, norm=1, dtype=np.float64, handle: Optional[N.Handle] = None) -> Tuple[float, int]:
    """Reciprocal condition number of a square matrix in the 1- or infinity-norm: norm, factorisation and LAPACK's
    gecon estimate in one call (lsx_rcond_*).  Returns (rcond, info); info > 0 is an exactly zero pivot (rcond 0)."""
    code = _norm_code(norm)
    ct, sfx = _ct(dtype)
    A = np.ascontiguousarray(a, dtype=dtype)
    if A.ndim != 2 or A.shape[0] != A.shape[1]:
        raise ValueError("rcond needs a square matrix")
    h = _h(handle)
    n = A.shape[0]
    rc, info = C.c_double(0.0), C.c_int(0)
    N.check(getattr(h.lib, f"lsx_rcond_{sfx}")(h.ptr, code, n, _ptr(A, ct) if n else None, max(n, 1), C.byref(rc),
                                                C.byref(info)), f"lsx_rcond_{sfx}")
    return rc.value, info.value


def lu_rcond(LU: np.ndarray, ipiv: np.ndarray, anorm: float, norm=1, handle: Optional[N.Handle] = None) -> float:
    """gecon from existing factors: anorm is the 1- (or infinity-) norm of the UNFACTORED matrix (lsx_gecon_*)."""
    code = _norm_code(norm)
    LU = np.asarray(LU)
    if LU.ndim != 2 or LU.shape[0] != LU.shape[1]:
        raise ValueError("lu_rcond needs the square factor matrix")
    ct, sfx = _ct(LU.dtype)
    n = LU.shape[0]
    if len(ipiv) < n:
        raise ValueError("ipiv is shorter than the matrix order")
    anorm = float(anorm)
    if math.isnan(anorm) or anorm < 0:
        raise ValueError("anorm must be a norm of the unfactored matrix (not NaN, not negative)")
    h = _h(handle)
    LU = np.ascontiguousarray(LU)
    ipiv = np.ascontiguousarray(ipiv, dtype=np.int32)
    rc = C.c_double(0.0)
    N.check(getattr(h.lib, f"lsx_gecon_{sfx}")(h.ptr, code, n, _ptr(LU, ct) if n else None, max(n, 1),
                                                _ptr(ipiv, C.c_int32) if n else None, anorm, C.byref(rc)),
            f"lsx_gecon_{sfx}")
    return rc.value


def lu_refine(a, LU, ipiv, b, x, trans: bool = False, handle: Optional[N.Handle] = None):
    """LAPACK's gerfs from existing factors (lsx_gerfs_*): refine the solution x of A X = B (trans=True: A^T X = B)
    until its componentwise backward error stops improving, and bound its error.  a is the UNFACTORED matrix, LU /
    ipiv its factors (lu_factor), x a solution (lu_solve).  Returns (x, ferr, berr): the refined solution (a new
    array), and per right-hand side a bound of max|x - x_true| / max|x| and the componentwise backward error.  Both
    are +inf when a pivot is exactly zero (x is returned as given) and NaN for a column with a NaN in its data."""
    LU = np.asarray(LU)
    if LU.ndim != 2 or LU.shape[0] != LU.shape[1]:
        raise ValueError("lu_refine needs the square factor matrix")
    ct, sfx = _ct(LU.dtype)
    dt = LU.dtype
    n = LU.shape[0]
    A = np.ascontiguousarray(a, dtype=dt)
    if A.shape != (n, n):
        raise ValueError("lu_refine needs the unfactored matrix and its factors: same shape")
    if len(ipiv) < n:
        raise ValueError("ipiv is shorter than the matrix order")
    if np.shape(b)[:1] != (n,) or np.shape(x) != np.shape(b):
        raise ValueError("right-hand side and solution need as many rows as the matrix, and the same shape")
    h = _h(handle)
    LU = np.ascontiguousarray(LU)
    ipiv = np.ascontiguousarray(ipiv, dtype=np.int32)
    B = np.ascontiguousarray(b, dtype=dt)
    X = np.array(x, dtype=dt, order="C", copy=True)
    vec = X.ndim == 1
    if vec:
        B, X = B.reshape(n, 1), X.reshape(n, 1)
    nrhs = X.shape[1]
    ferr, berr = np.zeros(max(nrhs, 1)), np.zeros(max(nrhs, 1))
    ld, ldr = max(n, 1), max(nrhs, 1)
    name = f"lsx_gerfs_{sfx}"
    N.check(getattr(h.lib, name)(h.ptr, int(bool(trans)), n, nrhs, _ptr(A, ct), ld, _ptr(LU, ct), ld,
                                 _ptr(ipiv, C.c_int32), _ptr(B, ct), ldr, _ptr(X, ct), ldr, _ptr(ferr, C.c_double),
                                 _ptr(berr, C.c_double)), name)
    ferr, berr = ferr[:nrhs], berr[:nrhs]
    if vec:
        return X[:, 0].copy(), float(ferr[0]), float(berr[0])
    return X, ferr, berr


def solve_bounded(a, b, trans: bool = False, dtype=np.float64, handle: Optional[N.Handle] = None):
    """Factor, solve, refine and bound in one call (lsx_gesvr_*): returns (x, ferr, berr, info) with ferr / berr as in
    lu_refine (floats for a vector b, arrays for a matrix).  info > 0 is an exactly zero pivot: x is None and the
    bounds are +inf."""
    ct, sfx = _ct(dtype)
    A = np.ascontiguousarray(a, dtype=dtype)
    n = A.shape[0]
    if A.ndim != 2 or A.shape[1] != n:
        raise ValueError("solve_bounded needs a square matrix")
    if np.shape(b)[:1] != (n,):
        raise ValueError("right-hand side has the wrong number of rows")
    h = _h(handle)
    B = np.ascontiguousarray(b, dtype=dtype)
    vec = B.ndim == 1
    if vec:
        B = B.reshape(n, 1)
    nrhs = B.shape[1]
    X = np.zeros((n, nrhs), dtype=dtype)
    ferr, berr = np.zeros(max(nrhs, 1)), np.zeros(max(nrhs, 1))
    info = C.c_int(0)
    ld, ldr = max(n, 1), max(nrhs, 1)
    name = f"lsx_gesvr_{sfx}"
    N.check(getattr(h.lib, name)(h.ptr, int(bool(trans)), n, nrhs, _ptr(A, ct), ld, _ptr(B, ct), ldr, _ptr(X, ct), ldr,
                                 _ptr(ferr, C.c_double), _ptr(berr, C.c_double), C.byref(info)), name)
    ferr, berr = ferr[:nrhs], berr[:nrhs]
    if vec:
        return (None if info.value else X[:, 0].copy()), float(ferr[0]), float(berr[0]), info.value
    return (None if info.value else X), ferr, berr, info.value


def cho_rcond(U: np.ndarray, anorm: float, handle: Optional[N.Handle] = None) -> float:
    """pocon from an existing Cholesky factor (cho_factor): anorm is the 1-norm of the UNFACTORED symmetric matrix
    (lsx_pocon_*).  Only the upper triangle of U is used."""
    U = np.asarray(U)
    if U.ndim != 2 or U.shape[0] != U.shape[1]:
        raise ValueError("cho_rcond needs the square factor matrix")
    ct, sfx = _ct(U.dtype)
    n = U.shape[0]
    anorm = float(anorm)
    if math.isnan(anorm) or anorm < 0:
        raise ValueError("anorm must be a norm of the unfactored matrix (not NaN, not negative)")
    h = _h(handle)
    U = np.ascontiguousarray(U)
    rc = C.c_double(0.0)
    N.check(getattr(h.lib, f"lsx_pocon_{sfx}")(h.ptr, n, _ptr(U, ct) if n else None, max(n, 1), anorm, C.byref(rc)),
            f"lsx_pocon_{sfx}")
    return rc.value


def rcond_pos(a, dtype=np.float64, handle: Optional[N.Handle] = None) -> Tuple[float, int]:
    """Reciprocal condition number (1-norm = infinity-norm) of a symmetric positive definite matrix: norm, Cholesky
    factorisation and LAPACK's pocon estimate in one call (lsx_porcond_*).  Only the upper triangle of a is used.
    Returns (rcond, info); info = j + 1 says the leading minor of order j + 1 is not positive definite (rcond 0)."""
    ct, sfx = _ct(dtype)
    A = np.ascontiguousarray(a, dtype=dtype)
    if A.ndim != 2 or A.shape[0] != A.shape[1]:
        raise ValueError("rcond_pos needs a square matrix")
    h = _h(handle)
    n = A.shape[0]
    rc, info = C.c_double(0.0), C.c_int(0)
    N.check(getattr(h.lib, f"lsx_porcond_{sfx}")(h.ptr, n, _ptr(A, ct) if n else None, max(n, 1), C.byref(rc),
                                                  C.byref(info)), f"lsx_porcond_{sfx}")
    return rc.value, info.value


def cho_refine(a, U, b, x, handle: Optional[N.Handle] = None):
    """LAPACK's porfs from an existing Cholesky factor (lsx_porfs_*): refine the solution x of A X = B until its
    componentwise backward error stops improving, and bound its error.  a is the UNFACTORED symmetric matrix, U its
    factor (cho_factor), x a solution (cho_solve); only the upper triangles of a and U are used.  Returns
    (x, ferr, berr) as lu_refine does: +inf bounds when a u_ii is exactly zero (x is returned as given), NaN for a
    column with a NaN in its data."""
    U = np.asarray(U)
    if U.ndim != 2 or U.shape[0] != U.shape[1]:
        raise ValueError("cho_refine needs the square factor matrix")
    ct, sfx = _ct(U.dtype)
    dt = U.dtype
    n = U.shape[0]
    A = np.ascontiguousarray(a, dtype=dt)
    if A.shape != (n, n):
        raise ValueError("cho_refine needs the unfactored matrix and its factor: same shape")
    if np.shape(b)[:1] != (n,) or np.shape(x) != np.shape(b):
        raise ValueError("right-hand side and solution need as many rows as the matrix, and the same shape")
    h = _h(handle)
    U = np.ascontiguousarray(U)
    B = np.ascontiguousarray(b, dtype=dt)
    X = np.array(x, dtype=dt, order="C", copy=True)
    vec = X.ndim == 1
    if vec:
        B, X = B.reshape(n, 1), X.reshape(n, 1)
    nrhs = X.shape[1]
    ferr, berr = np.zeros(max(nrhs, 1)), np.zeros(max(nrhs, 1))
    ld, ldr = max(n, 1), max(nrhs, 1)
    name = f"lsx_porfs_{sfx}"
    N.check(getattr(h.lib, name)(h.ptr, n, nrhs, _ptr(A, ct), ld, _ptr(U, ct), ld, _ptr(B, ct), ldr, _ptr(X, ct), ldr,
                                 _ptr(ferr, C.c_double), _ptr(berr, C.c_double)), name)
    ferr, berr = ferr[:nrhs], berr[:nrhs]
    if vec:
        return X[:, 0].copy(), float(ferr[0]), float(berr[0])
    return X, ferr, berr


def solve_pos_bounded(a, b, dtype=np.float64, handle: Optional[N.Handle] = None):
    """Cholesky-factor, solve, refine and bound in one call (lsx_posvr_*) for a symmetric positive definite matrix:
    returns (x, ferr, berr, info) with ferr / berr as in cho_refine (floats for a vector b, arrays for a matrix).
    Only the upper triangle of a is used.  info = j + 1 says the leading minor of order j + 1 is not positive
    definite: x is None and the bounds are +inf."""
    ct, sfx = _ct(dtype)
    A = np.ascontiguousarray(a, dtype=dtype)
    n = A.shape[0]
    if A.ndim != 2 or A.shape[1] != n:
        raise ValueError("solve_pos_bounded needs a square matrix")
    if np.shape(b)[:1] != (n,):
        raise ValueError("right-hand side has the wrong number of rows")
    h = _h(handle)
    B = np.ascontiguousarray(b, dtype=dtype)
    vec = B.ndim == 1
    if vec:
        B = B.reshape(n, 1)
    nrhs = B.shape[1]
    X = np.zeros((n, nrhs), dtype=dtype)
    ferr, berr = np.zeros(max(nrhs, 1)), np.zeros(max(nrhs, 1))
    info = C.c_int(0)
    ld, ldr = max(n, 1), max(nrhs, 1)
    name = f"lsx_posvr_{sfx}"
    N.check(getattr(h.lib, name)(h.ptr, n, nrhs, _ptr(A, ct), ld, _ptr(B, ct), ldr, _ptr(X, ct), ldr,
                                 _ptr(ferr, C.c_double), _ptr(berr, C.c_double), C.byref(info)), name)
    ferr, berr = ferr[:nrhs], berr[:nrhs]
    if vec:
        return (None if info.value else X[:, 0].copy()), float(ferr[0]), float(berr[0]), info.value
    return (None if info.value else X), ferr, berr, info.value


def solve_expert(a, b, trans: bool = False, equilibrate: bool = True, dtype=np.float64,
                 handle: Optional[N.Handle] = None):
    """LAPACK's expert driver gesvx in one call (lsx_gesvx_*): equilibrate the matrix if its rows or columns are badly
    scaled (geequ / laqge; equilibrate=False is fact='N'), factor, estimate the condition of the equilibrated matrix,
    solve A X = B (trans=True: A^T X = B), refine and bound.  Returns (x, ferr, berr, rcond, rpvgrw, equed, r, c, info):
    x is None when info is in 1..n (an exactly zero pivot; ferr = berr = +inf, rcond = 0) or when A holds a NaN
    (rcond, rpvgrw, ferr, berr are NaN; info is 0); info == n + 1 says rcond is below the unit roundoff, x and the bounds are still returned.
    equed is N.EQUED_NONE / _ROW / _COL / _BOTH and r, c the scale factors (ones where geequ chose none).  ferr / berr
    are floats for a vector b and arrays for a matrix; ferr is LAPACK's, divided by colcnd / rowcnd after a column /
    row equilibration, which can make it vacuous (include/lsx.h).  b may have zero columns: the equilibrated condition
    number alone."""
    ct, sfx = _ct(dtype)
    A = np.ascontiguousarray(a, dtype=dtype)
    n = A.shape[0]
    if A.ndim != 2 or A.shape[1] != n:
        raise ValueError("solve_expert needs a square matrix")
    if np.shape(b)[:1] != (n,):
        raise ValueError("right-hand side has the wrong number of rows")
    h = _h(handle)
    B = np.ascontiguousarray(b, dtype=dtype)
    vec = B.ndim == 1
    if vec:
        B = B.reshape(n, 1)
    nrhs = B.shape[1]
    X = np.zeros((n, nrhs), dtype=dtype)
    r, c = np.ones(max(n, 1), dtype=dtype), np.ones(max(n, 1), dtype=dtype)
    ferr, berr = np.zeros(max(nrhs, 1)), np.zeros(max(nrhs, 1))
    equed, info = C.c_int(0), C.c_int(0)
    rc, growth = C.c_double(0.0), C.c_double(0.0)
    ld, ldr = max(n, 1), max(nrhs, 1)
    name = f"lsx_gesvx_{sfx}"
    N.check(getattr(h.lib, name)(h.ptr, int(bool(equilibrate)), int(bool(trans)), n, nrhs, _ptr(A, ct), ld, _ptr(B, ct),
                                 ldr, _ptr(X, ct), ldr, C.byref(equed), _ptr(r, ct), _ptr(c, ct), C.byref(rc),
                                 _ptr(ferr, C.c_double), _ptr(berr, C.c_double), C.byref(growth), C.byref(info)), name)
    ferr, berr = ferr[:nrhs], berr[:nrhs]
    solved = (info.value == 0 or info.value == n + 1) and not math.isnan(rc.value)
    if vec:
        x, ferr, berr = (X[:, 0].copy() if solved else None), float(ferr[0]), float(berr[0])
    else:
        x = X if solved else None
    return x, ferr, berr, rc.value, growth.value, equed.value, r[:n], c[:n], info.value


def solve_refined(a, b, sweeps: int = 3, handle: Optional[N.Handle] = None):
    """Mixed-precision solve of A X = B (lsx_gesv_f32_refined): fp32 factors on the fp32 MFMA tile, residuals in
    fp64, `sweeps` corrections.  a and b are taken in fp32 (BASELINE config 5 computes in fp32); returns
    (X as float64, info, pivot_ratio, last_correction) -- X is None when info != 0.  The forward error against
    the fp64 solution of the same system is far below the 1e-4 the configuration asks for, which a plain fp32
    solve of a large random system does not reach (cond * eps32)."""
    h = _h(handle)
    A = np.ascontiguousarray(a, dtype=np.float32)
    n = A.shape[0]
    if A.ndim != 2 or A.shape[1] != n:
        raise ValueError("solve needs a square matrix")
    B = np.array(b, dtype=np.float32, order="C", copy=True)
    vec = B.ndim == 1
    if vec:
        B = B.reshape(n, 1).copy()
    if B.shape[0] != n:
        raise ValueError("right-hand side has the wrong number of rows")
    nrhs = B.shape[1]
    X = np.zeros((n, nrhs), dtype=np.float64)
    info, ratio, corr = C.c_int(0), C.c_double(1.0), C.c_double(0.0)
    N.check(h.lib.lsx_gesv_f32_refined(h.ptr, n, nrhs, _ptr(A, C.c_float), n, _ptr(B, C.c_float), nrhs, None, nrhs,
                                       _ptr(X, C.c_double), nrhs, int(sweeps), C.byref(info), C.byref(ratio),
                                       C.byref(corr)), "lsx_gesv_f32_refined")
    if info.value != 0:
        return None, info.value, ratio.value, corr.value
    return (X[:, 0].copy() if vec else X), 0, ratio.value, corr.value


def inv(a, handle: Optional[N.Handle] = None, dtype=np.float64, assume_pos: bool = False):
    """Returns (inverse or None, info, pivot_ratio).
    assume_pos=True: A is symmetric positive definite and goes through the Cholesky factorisation and LAPACK's potri
    (lsx_poinv_*: n^3 flops instead of 2 n^3, no pivoting).  Only the upper triangle of a is used and symmetry is not
    checked; the inverse comes back with both triangles, exactly symmetric; info = j + 1 says the leading minor of order
    j + 1 is not positive definite; pivot_ratio is 1.0 (nothing is pivoted), as solve(assume_pos=True) returns it."""
    h = _h(handle)
    ct, sfx = _ct(dtype)
    A = np.ascontiguousarray(a, dtype=dtype)
    n = A.shape[0]
    if A.ndim != 2 or A.shape[1] != n:
        raise ValueError("inv needs a square matrix")
    out = np.empty_like(A)
    if assume_pos:
        pinfo = C.c_int(0)
        if n:
            N.check(getattr(h.lib, f"lsx_poinv_{sfx}")(h.ptr, n, _ptr(A, ct), n, _ptr(out, ct), n, C.byref(pinfo)),
                    f"lsx_poinv_{sfx}")
        if pinfo.value != 0:
            return None, pinfo.value, 1.0
        return out, 0, 1.0
    info, ratio = C.c_int(0), C.c_double(1.0)
    N.check(getattr(h.lib, f"lsx_getri_{sfx}")(h.ptr, n, _ptr(A, ct), n, _ptr(out, ct), n, C.byref(info),
                                                C.byref(ratio)), f"lsx_getri_{sfx}")
    if info.value != 0:
        return None, info.value, ratio.value
    return out, 0, ratio.value


def det_parts_pos(a, handle: Optional[N.Handle] = None, dtype=np.float64) -> Tuple[float, float, int, int]:
    """(sign, mant, exp2, info) of det(A) = prod u_ii^2 from the Cholesky factor of a symmetric positive definite matrix
    (lsx_podet_*).  Only the upper triangle of a is used; info = j + 1 says the leading minor of order j + 1 is not
    positive definite, the three parts are 0 then."""
    h = _h(handle)
    ct, sfx = _ct(dtype)
    A = np.ascontiguousarray(a, dtype=dtype)
    n = A.shape[0]
    if A.ndim != 2 or A.shape[1] != n:
        raise ValueError("det needs a square matrix")
    s, m, e, info = C.c_double(0), C.c_double(0), C.c_int64(0), C.c_int(0)
    N.check(getattr(h.lib, f"lsx_podet_{sfx}")(h.ptr, n, _ptr(A, ct), n, C.byref(s), C.byref(m), C.byref(e),
                                                C.byref(info)), f"lsx_podet_{sfx}")
    return s.value, m.value, int(e.value), info.value


def det_parts(a, handle: Optional[N.Handle] = None, dtype=np.float64, assume_pos: bool = False) -> Tuple[float, float, int]:
    """det(A) = sign * mant * 2**exp2 with mant in [0.5, 1) (sign 0 for a singular matrix).
    assume_pos=True: A is symmetric positive definite and the determinant comes from its Cholesky factor
    (det_parts_pos); a matrix that is not positive definite raises ValueError."""
    if assume_pos:
        s, m, e, info = det_parts_pos(a, handle, dtype)
        if info != 0:
            raise ValueError(f"matrix is not positive definite: its leading minor of order {info} is not "
                             "(assume_pos=True asserts a symmetric positive definite matrix)")
        return s, m, e
    h = _h(handle)
    ct, sfx = _ct(dtype)
    A = np.ascontiguousarray(a, dtype=dtype)
    n = A.shape[0]
    if A.ndim != 2 or A.shape[1] != n:
        raise ValueError("det needs a square matrix")
    s, m, e = C.c_double(0), C.c_double(0), C.c_int64(0)
    N.check(getattr(h.lib, f"lsx_det_{sfx}")(h.ptr, n, _ptr(A, ct), n, C.byref(s), C.byref(m), C.byref(e)), f"lsx_det_{sfx}")
    return s.value, m.value, int(e.value)


def slogdet(a, handle: Optional[N.Handle] = None, dtype=np.float64, assume_pos: bool = False) -> Tuple[float, float]:
    s, m, e = det_parts(a, handle, dtype, assume_pos)
    if s == 0.0:
        return 0.0, -math.inf
    return s, math.log(m) + e * math.log(2.0)


def det(a, handle: Optional[N.Handle] = None, assume_pos: bool = False) -> float:
    s, m, e = det_parts(a, handle, assume_pos=assume_pos)
    if s == 0.0:
        return 0.0
    try:
        return s * math.ldexp(m, e)
    except OverflowError:
        return s * math.inf


def matmul(a, b, handle: Optional[N.Handle] = None) -> np.ndarray:
    """C = A @ B on the MFMA tile of the trailing update (residual checks, Matrix.__mul__)."""
    h = _h(handle)
    A, B = _f64(a), _f64(b)
    if A.ndim != 2 or B.ndim != 2 or A.shape[1] != B.shape[0]:
        raise ValueError("Matrix dimensions must match")
    m, k = A.shape
    n = B.shape[1]
    Cm = np.empty((m, n), dtype=np.float64)
    if m and n:
        N.check(h.lib.lsx_matmul_f64(h.ptr, m, n, k, _ptr(A, C.c_double), max(k, 1), _ptr(B, C.c_double), max(n, 1),
                                     _ptr(Cm, C.c_double), n), "lsx_matmul_f64")
    return Cm


def rref(a, bar_col: Optional[int] = None, tol: float = -1.0, handle: Optional[N.Handle] = None,
         pivot_rule: int = N.PIVOT_FIRST, dtype=np.float64):
    """Reduced row echelon form over columns [0, bar_col).  Returns (R, pivots, rank).
    pivot_rule: N.PIVOT_FIRST = the reference's first-non-zero rule, N.PIVOT_MAX = largest |a|."""
    h = _h(handle)
    ct, sfx = _ct(dtype)
    A = np.ascontiguousarray(a, dtype=dtype)
    if A.ndim != 2 or A.shape[0] < 1 or A.shape[1] < 1:
        raise ValueError("rref needs a non-empty 2-D matrix")
    m, n = A.shape
    R = np.empty_like(A)
    piv = np.zeros(2 * min(m, n), dtype=np.int32)
    rank = C.c_int(0)
    N.check(getattr(h.lib, f"lsx_rref_{sfx}")(h.ptr, m, n, int(bar_col or 0), _ptr(A, ct), n, _ptr(R, ct), n,
                                               _ptr(piv, C.c_int32), C.byref(rank), float(tol), int(pivot_rule)),
            f"lsx_rref_{sfx}")
    r = rank.value
    return R, [(int(piv[2 * i]), int(piv[2 * i + 1])) for i in range(r)], r


TRACE_KINDS = ("S", "N", "E", "E")   # step record kind -> label letter (swap, normalise, eliminate below / above)


def rref_trace(a, bar_col: Optional[int] = None, max_snapshots: int = 0, int_mask=None,
               handle: Optional[N.Handle] = None):
    """Row reduction in the reference's own operation order with its step log (lsx_rref_trace_f64;
    linalg.py:547-629).  Returns (R, pivots, steps, int_mask, snaps, snap_int_masks): steps is a list of
    (kind, a, b) with kind 0 = swap rows a,b / 1 = normalise row a / 2 = eliminate below the pivot of
    column a / 3 = eliminate above the pivot of column a (1-based, as in the reference's descriptions).
    int_mask (bool m x n, default all False) says which input entries are Python ints; the returned mask
    says which entries the reference would still hold as ints.  snaps / snap_int_masks hold the matrix
    and its mask after each of the first max_snapshots steps (or None)."""
    h = _h(handle)
    A = _f64(a)
    if A.ndim != 2 or A.shape[0] < 1 or A.shape[1] < 1:
        raise ValueError("rref_trace needs a non-empty 2-D matrix")
    m, n = A.shape
    bar = int(bar_col or 0) or n - 1
    max_steps = 4 * min(m, max(bar, 1)) + 4
    R = np.empty_like(A)
    mask = np.zeros((m, n), dtype=np.uint8)
    if int_mask is not None:
        mask[:, :] = np.asarray(int_mask, dtype=bool)
    piv = np.zeros(2 * min(m, n) + 2, dtype=np.int32)
    steps = np.zeros(4 * max_steps, dtype=np.int32)
    nsnap = max(0, min(int(max_snapshots), max_steps))
    snaps = np.empty((nsnap, m, n), dtype=np.float64) if nsnap else None
    snap_m = np.zeros((nsnap, m, n), dtype=np.uint8) if nsnap else None
    npiv, nsteps = C.c_int(0), C.c_int(0)
    N.check(h.lib.lsx_rref_trace_f64(h.ptr, m, n, int(bar_col or 0), _ptr(A, C.c_double), n, _ptr(R, C.c_double), n,
                                     mask.ctypes.data, _ptr(piv, C.c_int32), C.byref(npiv),
                                     _ptr(steps, C.c_int32), max_steps, C.byref(nsteps),
                                     _ptr(snaps, C.c_double) if nsnap else None,
                                     snap_m.ctypes.data if nsnap else None, nsnap), "lsx_rref_trace_f64")
    pivots = [(int(piv[2 * i]), int(piv[2 * i + 1])) for i in range(npiv.value)]
    recs = [(int(steps[4 * i]), int(steps[4 * i + 1]), int(steps[4 * i + 2])) for i in range(nsteps.value)]
    k = min(nsnap, nsteps.value)
    return R, pivots, recs, mask.astype(bool), (snaps[:k] if nsnap else None), (snap_m[:k].astype(bool) if nsnap else None)
