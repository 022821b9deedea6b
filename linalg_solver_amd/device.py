"""Device-resident entry points: torch tensors in HBM -> liblsx *_dev functions.

torch is plumbing here (allocation, streams, torch.distributed); every
computation is a hand-written HIP kernel reached through the C ABI with the
tensor's ``data_ptr()``.  Tensors must be row-major ("contiguous" or with a
row stride >= ncols and unit column stride), dtype float64 / float32.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _native as N


def _rowmajor(t: torch.Tensor, what: str):
    if t.dim() != 2 or t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        raise ValueError(f"{what}: need a row-major 2-D tensor (unit column stride)")
    if not t.is_cuda:
        raise ValueError(f"{what}: tensor must live on the GPU")


class DeviceSolver:
    """One liblsx handle bound to a torch device and (by default) torch's current stream."""

    def __init__(self, device: Optional[int] = None, use_torch_stream: bool = True):
        if not torch.cuda.is_available():
            raise N.LsxError("no GPU visible to torch; linalg_solver_amd has no CPU fallback")
        self.device = torch.cuda.current_device() if device is None else int(device)
        self.h = N.Handle(self.device)
        self.lib = self.h.lib
        if use_torch_stream:
            self.h.set_stream(torch.cuda.current_stream(self.device).cuda_stream)

    # -- helpers
    def _suffix(self, t: torch.Tensor) -> str:
        if t.dtype == torch.float64:
            return "f64"
        if t.dtype == torch.float32:
            return "f32"
        raise TypeError("dtype must be float64 or float32")

    def fill_(self, A: torch.Tensor, kind: int, seed: int, row_off: int = 0, col_off: int = 0):
        _rowmajor(A, "fill_")
        fn = getattr(self.lib, f"lsx_fill_{self._suffix(A)}_dev")
        N.check(fn(self.h.ptr, kind, seed, A.shape[0], A.shape[1], A.data_ptr(), A.stride(0), row_off, col_off))
        return A

    def getrf_(self, A: torch.Tensor, ipiv: Optional[torch.Tensor] = None, info: Optional[torch.Tensor] = None):
        """In-place P A = L U.  Returns (ipiv int32[n], info int32[1]) device tensors; no host sync."""
        _rowmajor(A, "getrf_")
        n = A.shape[0]
        if A.shape[1] != n:
            raise ValueError("getrf_ needs a square matrix")
        if ipiv is None:
            ipiv = torch.empty(max(n, 1), dtype=torch.int32, device=A.device)
        if info is None:
            info = torch.zeros(1, dtype=torch.int32, device=A.device)
        fn = getattr(self.lib, f"lsx_getrf_{self._suffix(A)}_dev")
        N.check(fn(self.h.ptr, n, A.data_ptr(), A.stride(0), ipiv.data_ptr(), info.data_ptr()), "getrf_dev")
        return ipiv, info

    def getrs_(self, LU: torch.Tensor, ipiv: torch.Tensor, B: torch.Tensor, trans: bool = False):
        """B <- A^-1 B in place (B: n x nrhs); trans=True: B <- A^-T B from the same factors (lsx_getrs_t_*_dev)."""
        _rowmajor(LU, "getrs_")
        _rowmajor(B, "getrs_")
        if LU.shape[0] != LU.shape[1] or B.shape[0] != LU.shape[0]:
            raise ValueError("getrs_: need square factors and a right-hand side with as many rows")
        if B.dtype != LU.dtype:
            raise TypeError("getrs_: factors and right-hand side must have the same dtype")
        name = f"lsx_getrs_t_{self._suffix(LU)}_dev" if trans else f"lsx_getrs_{self._suffix(LU)}_dev"
        N.check(getattr(self.lib, name)(self.h.ptr, LU.shape[0], B.shape[1], LU.data_ptr(), LU.stride(0), ipiv.data_ptr(),
                                        B.data_ptr(), B.stride(0)), name)
        return B

    def potrf_(self, A: torch.Tensor, info: Optional[torch.Tensor] = None):
        """In-place Cholesky factorisation A = U^T U of a symmetric positive definite matrix in HBM, upper storage
        (lsx_potrf_*_dev): the upper triangle of A is overwritten by U, the strictly lower triangle is neither read
        nor written.  Returns info (int32[1] device tensor: 0, or j + 1 for the first non-positive pivot); no host
        sync."""
        _rowmajor(A, "potrf_")
        n = A.shape[0]
        if A.shape[1] != n:
            raise ValueError("potrf_ needs a square matrix")
        if info is None:
            info = torch.zeros(1, dtype=torch.int32, device=A.device)
        elif info.dtype != torch.int32 or info.device != A.device or info.numel() < 1 or not info.is_contiguous():
            raise ValueError("potrf_: info must be a contiguous int32 tensor with at least one entry on A's device")
        name = f"lsx_potrf_{self._suffix(A)}_dev"
        N.check(getattr(self.lib, name)(self.h.ptr, n, A.data_ptr(), max(A.stride(0), 1), info.data_ptr()), name)
        return info

    def potrs_(self, U: torch.Tensor, B: torch.Tensor):
        """B <- inv(U) inv(U^T) B in place from the factor of potrf_ (lsx_potrs_*_dev); only the upper triangle of U
        is read."""
        _rowmajor(U, "potrs_")
        _rowmajor(B, "potrs_")
        if U.shape[0] != U.shape[1] or B.shape[0] != U.shape[0]:
            raise ValueError("potrs_: need the square factor and a right-hand side with as many rows")
        if B.dtype != U.dtype:
            raise TypeError("potrs_: factor and right-hand side must have the same dtype")
        name = f"lsx_potrs_{self._suffix(U)}_dev"
        N.check(getattr(self.lib, name)(self.h.ptr, U.shape[0], B.shape[1], U.data_ptr(), max(U.stride(0), 1),
                                        B.data_ptr(), max(B.stride(0), 1)), name)
        return B

    def syrk_tn_sub_(self, C: torch.Tensor, A: torch.Tensor):
        """Upper triangle of C (n x n) -= A.T @ A with A stored k x n, on the MFMA kernel; the strictly lower triangle
        of C is untouched (lsx_syrk_tn_sub_*_dev)."""
        _rowmajor(C, "syrk_tn_sub_ C")
        _rowmajor(A, "syrk_tn_sub_ A")
        k, n = A.shape
        if tuple(C.shape) != (n, n):
            raise ValueError("syrk_tn_sub_: need A (k x n) and C (n x n)")
        if A.dtype != C.dtype:
            raise TypeError("syrk_tn_sub_: both operands must have the same dtype")
        name = f"lsx_syrk_tn_sub_{self._suffix(C)}_dev"
        N.check(getattr(self.lib, name)(self.h.ptr, n, k, A.data_ptr(), max(A.stride(0), 1), C.data_ptr(),
                                        max(C.stride(0), 1)), name)
        return C

    def _square(self, A: torch.Tensor, what: str) -> int:
        _rowmajor(A, what)
        if A.shape[0] != A.shape[1]:
            raise ValueError(f"{what} needs a square matrix")
        return A.shape[0]

    def potri_(self, U: torch.Tensor, info: Optional[torch.Tensor] = None):
        """In place: the upper triangle of the factor of potrf_ becomes the upper triangle of inv(A) (LAPACK's potri,
        lsx_potri_*_dev); the strictly lower triangle is neither read nor written.  Returns info (int32[1] device
        tensor: 0, or i + 1 for the first u_ii that is zero or NaN); no host sync."""
        n = self._square(U, "potri_")
        if info is None:
            info = torch.zeros(1, dtype=torch.int32, device=U.device)
        elif info.dtype != torch.int32 or info.device != U.device or info.numel() < 1 or not info.is_contiguous():
            raise ValueError("potri_: info must be a contiguous int32 tensor with at least one entry on U's device")
        name = f"lsx_potri_{self._suffix(U)}_dev"
        N.check(getattr(self.lib, name)(self.h.ptr, n, U.data_ptr(), max(U.stride(0), 1), info.data_ptr()), name)
        return info

    def symmetrize_upper_(self, A: torch.Tensor):
        """a_ji = a_ij for every j > i, in place (lsx_symmetrize_upper_*_dev)."""
        n = self._square(A, "symmetrize_upper_")
        name = f"lsx_symmetrize_upper_{self._suffix(A)}_dev"
        N.check(getattr(self.lib, name)(self.h.ptr, n, A.data_ptr(), max(A.stride(0), 1)), name)
        return A

    def lauum_tn_(self, C: torch.Tensor, V: torch.Tensor):
        """Upper triangle of C (n x n) = V.T @ V for a lower-triangular V; the blocks of V strictly above its diagonal
        128-blocks are never read, the strictly lower triangle of C is untouched (lsx_lauum_tn_*_dev)."""
        n = self._square(V, "lauum_tn_ V")
        if self._square(C, "lauum_tn_ C") != n:
            raise ValueError("lauum_tn_: need V (n x n) and C (n x n)")
        if V.dtype != C.dtype:
            raise TypeError("lauum_tn_: both operands must have the same dtype")
        name = f"lsx_lauum_tn_{self._suffix(C)}_dev"
        N.check(getattr(self.lib, name)(self.h.ptr, n, V.data_ptr(), max(V.stride(0), 1), C.data_ptr(),
                                        max(C.stride(0), 1)), name)
        return C

    def trtri_upper_t_(self, V: torch.Tensor, U: torch.Tensor):
        """V = inv(U^T) on and below the diagonal 128-blocks of V, from the upper triangle of U; the blocks of V strictly
        above its diagonal blocks are not written (lsx_trtri_upper_t_*_dev)."""
        n = self._square(U, "trtri_upper_t_ U")
        if self._square(V, "trtri_upper_t_ V") != n:
            raise ValueError("trtri_upper_t_: need U (n x n) and V (n x n)")
        if V.dtype != U.dtype:
            raise TypeError("trtri_upper_t_: both operands must have the same dtype")
        name = f"lsx_trtri_upper_t_{self._suffix(U)}_dev"
        N.check(getattr(self.lib, name)(self.h.ptr, n, U.data_ptr(), max(U.stride(0), 1), V.data_ptr(),
                                        max(V.stride(0), 1)), name)
        return V

    def podet_parts(self, U: torch.Tensor) -> torch.Tensor:
        """Device tensor [sign, mant, exp2] of det(A) = prod u_ii^2 from the factor of potrf_ (lsx_podet_*_dev)."""
        n = self._square(U, "podet_parts")
        out = torch.empty(3, dtype=torch.float64, device=U.device)
        name = f"lsx_podet_{self._suffix(U)}_dev"
        N.check(getattr(self.lib, name)(self.h.ptr, n, U.data_ptr(), max(U.stride(0), 1), out.data_ptr()), name)
        return out

    # -- Householder QR and least squares
    def _tau(self, A: torch.Tensor, tau: Optional[torch.Tensor], k: int, what: str) -> torch.Tensor:
        if tau is None:
            return torch.zeros(max(k, 1), dtype=A.dtype, device=A.device)
        if tau.dtype != A.dtype or tau.device != A.device or tau.dim() != 1 or tau.numel() < k or \
                (tau.numel() > 1 and tau.stride(0) != 1):
            raise ValueError(f"{what}: tau must be a dense vector of the matrix's dtype and device with at least {k} entries")
        return tau

    def geqrf_(self, A: torch.Tensor, tau: Optional[torch.Tensor] = None):
        """In-place Householder QR of A (m x n) in HBM (lsx_geqrf_*_dev): R on and above the diagonal, reflector j below
        the diagonal of column j.  Returns tau (min(m, n) entries of A's dtype); no host sync."""
        _rowmajor(A, "geqrf_")
        m, n = A.shape
        tau = self._tau(A, tau, min(m, n), "geqrf_")
        name = f"lsx_geqrf_{self._suffix(A)}_dev"
        N.check(getattr(self.lib, name)(self.h.ptr, m, n, A.data_ptr(), max(A.stride(0), 1), tau.data_ptr()), name)
        return tau

    def ormqr_(self, QR: torch.Tensor, tau: torch.Tensor, C: torch.Tensor, trans: bool = True):
        """C <- Q^T C (trans=True) or Q C in place, Q from the first len(tau) reflectors of geqrf_'s result
        (lsx_ormqr_*_dev)."""
        _rowmajor(QR, "ormqr_ QR")
        _rowmajor(C, "ormqr_ C")
        k = min(tau.numel(), QR.shape[0], QR.shape[1])
        if C.shape[0] != QR.shape[0]:
            raise ValueError("ormqr_: C needs as many rows as the factored matrix")
        if C.dtype != QR.dtype:
            raise TypeError("ormqr_: both operands must have the same dtype")
        tau = self._tau(QR, tau, k, "ormqr_")
        name = f"lsx_ormqr_{self._suffix(QR)}_dev"
        N.check(getattr(self.lib, name)(self.h.ptr, 1 if trans else 0, QR.shape[0], C.shape[1], k, QR.data_ptr(),
                                        max(QR.stride(0), 1), tau.data_ptr(), C.data_ptr(), max(C.stride(0), 1)), name)
        return C

    def orgqr(self, QR: torch.Tensor, tau: torch.Tensor, out: Optional[torch.Tensor] = None):
        """The thin Q (m x n, m >= n) of geqrf_'s result, out of place (lsx_orgqr_*_dev)."""
        _rowmajor(QR, "orgqr")
        m, n = QR.shape
        if m < n:
            raise ValueError("orgqr: the thin Q needs at least as many rows as columns")
        if out is None:
            out = torch.empty((m, n), dtype=QR.dtype, device=QR.device)
        _rowmajor(out, "orgqr out")
        if tuple(out.shape) != (m, n) or out.dtype != QR.dtype:
            raise ValueError("orgqr: out must have the shape and dtype of the factored matrix")
        k = min(tau.numel(), n)
        tau = self._tau(QR, tau, k, "orgqr")
        name = f"lsx_orgqr_{self._suffix(QR)}_dev"
        N.check(getattr(self.lib, name)(self.h.ptr, m, n, k, QR.data_ptr(), max(QR.stride(0), 1), tau.data_ptr(),
                                        out.data_ptr(), max(out.stride(0), 1)), name)
        return out

    def gels_(self, A: torch.Tensor, B: torch.Tensor, tau: Optional[torch.Tensor] = None,
              info: Optional[torch.Tensor] = None):
        """Least squares in place for m >= n (lsx_gels_*_dev): A becomes its QR, rows [0, n) of B the solution, rows
        [n, m) the tail of Q^T B (col_norms of it gives the residual norms).  Returns (tau, info): info is 0, or
        i + 1 for the first r_ii that is zero or NaN; no host sync."""
        _rowmajor(A, "gels_ A")
        _rowmajor(B, "gels_ B")
        m, n = A.shape
        if m < n:
            raise ValueError("gels_: needs at least as many rows as columns")
        if B.shape[0] != m:
            raise ValueError("gels_: B needs as many rows as A")
        if B.dtype != A.dtype:
            raise TypeError("gels_: both operands must have the same dtype")
        tau = self._tau(A, tau, n, "gels_")
        if info is None:
            info = torch.zeros(1, dtype=torch.int32, device=A.device)
        elif info.dtype != torch.int32 or info.device != A.device or info.numel() < 1 or not info.is_contiguous():
            raise ValueError("gels_: info must be a contiguous int32 tensor with at least one entry on A's device")
        name = f"lsx_gels_{self._suffix(A)}_dev"
        N.check(getattr(self.lib, name)(self.h.ptr, m, n, B.shape[1], A.data_ptr(), max(A.stride(0), 1), tau.data_ptr(),
                                        B.data_ptr(), max(B.stride(0), 1), info.data_ptr()), name)
        return tau, info

    # -- Jacobi SVD and minimum-norm least squares
    def gesvdj_(self, A: torch.Tensor, compute_uv: bool = True):
        """One-sided Jacobi SVD of A (m x n) in HBM (lsx_gesvdj_*_dev); A is DESTROYED.  Returns (U, s, Vt, info): the
        thin factors (None with compute_uv=False), s as a device float64 tensor of min(m, n) entries, descending, and
        info as a host int (1: the last allowed sweep still rotated).  Synchronises the stream: the host reads one
        counter per sweep."""
        import ctypes as C

        _rowmajor(A, "gesvdj_")
        m, n = A.shape
        k = min(m, n)
        s = torch.zeros(k, dtype=torch.float64, device=A.device)
        U = torch.zeros((m, k), dtype=A.dtype, device=A.device) if compute_uv else None
        Vt = torch.zeros((k, n), dtype=A.dtype, device=A.device) if compute_uv else None
        info = C.c_int(0)
        name = f"lsx_gesvdj_{self._suffix(A)}_dev"
        if k:
            N.check(getattr(self.lib, name)(self.h.ptr, 1 if compute_uv else 0, m, n, A.data_ptr(), max(A.stride(0), 1),
                                            s.data_ptr(), U.data_ptr() if compute_uv else None, max(k, 1),
                                            Vt.data_ptr() if compute_uv else None, max(n, 1), C.byref(info)), name)
        return U, s, Vt, info.value

    def gelss_(self, A: torch.Tensor, B: torch.Tensor, rcond: float = -1.0):
        """The minimum-norm least-squares solution for any shape and rank (lsx_gelss_*_dev); A is DESTROYED, B is kept.
        Returns (X, s, rank, info): X (n x nrhs) and s (device float64) are new tensors, rank (singular values above
        rcond * s[0]; rcond < 0: max(m, n) times the unit roundoff) and info are host ints.  Synchronises the stream."""
        import ctypes as C

        _rowmajor(A, "gelss_ A")
        _rowmajor(B, "gelss_ B")
        m, n = A.shape
        if B.shape[0] != m:
            raise ValueError("gelss_: B needs as many rows as A")
        if B.dtype != A.dtype:
            raise TypeError("gelss_: both operands must have the same dtype")
        nrhs = B.shape[1]
        X = torch.zeros((n, nrhs), dtype=A.dtype, device=A.device)
        s = torch.zeros(min(m, n), dtype=torch.float64, device=A.device)
        rank, info = C.c_int(0), C.c_int(0)
        name = f"lsx_gelss_{self._suffix(A)}_dev"
        if m and n and nrhs:
            N.check(getattr(self.lib, name)(self.h.ptr, m, n, nrhs, A.data_ptr(), max(A.stride(0), 1), B.data_ptr(),
                                            max(B.stride(0), 1), X.data_ptr(), max(X.stride(0), 1), float(rcond),
                                            s.data_ptr(), C.byref(rank), C.byref(info)), name)
        return X, s, rank.value, info.value

    # -- symmetric eigensolver by two-sided Jacobi
    def syevj_(self, A: torch.Tensor, compute_v: bool = True):
        """Eigenvalues and eigenvectors of the symmetric A (n x n, only its upper triangle is used) in HBM
        (lsx_syevj_*_dev); A is DESTROYED: what it holds afterwards is unspecified.  Returns (w, V, info): w as a device
        float64 tensor of n entries, ascending, V (n x n, column i the eigenvector of w[i]; None with compute_v=False)
        and info as a host int (1: the last allowed sweep still rotated).  Synchronises the stream: the host reads one
        counter per sweep."""
        import ctypes as C

        _rowmajor(A, "syevj_")
        n = A.shape[0]
        if A.shape[1] != n:
            raise ValueError("syevj_ needs a square matrix")
        w = torch.zeros(n, dtype=torch.float64, device=A.device)
        V = torch.zeros((n, n), dtype=A.dtype, device=A.device) if compute_v else None
        info = C.c_int(0)
        name = f"lsx_syevj_{self._suffix(A)}_dev"
        if n:
            N.check(getattr(self.lib, name)(self.h.ptr, 1 if compute_v else 0, n, A.data_ptr(), max(A.stride(0), 1),
                                            w.data_ptr(), V.data_ptr() if compute_v else None, max(n, 1), C.byref(info)), name)
        return w, V, info.value

    def col_norms(self, A: torch.Tensor) -> torch.Tensor:
        """The 2-norm of every column of A: a device double[n], fp64 sums in a fixed order (lsx_colnrm2_*_dev)."""
        _rowmajor(A, "col_norms")
        out = torch.zeros(A.shape[1], dtype=torch.float64, device=A.device)
        name = f"lsx_colnrm2_{self._suffix(A)}_dev"
        N.check(getattr(self.lib, name)(self.h.ptr, A.shape[0], A.shape[1], A.data_ptr(), max(A.stride(0), 1),
                                        out.data_ptr()), name)
        return out

    @staticmethod
    def _norm_code(which) -> int:
        if which in (1, "1", "one", "O", "o"):
            return N.NORM_ONE
        if which in (float("inf"), "inf", "I", "i"):
            return N.NORM_INF
        raise ValueError(f"norm must be 1 or inf, got {which!r}")

    def norm(self, A: torch.Tensor, which=1) -> torch.Tensor:
        """Max absolute column sum (which=1) or row sum (which=inf) of a tensor in HBM: a device double[1], no host
        sync (lsx_lange_*_dev)."""
        code = self._norm_code(which)
        _rowmajor(A, "norm")
        out = torch.zeros(1, dtype=torch.float64, device=A.device)
        name = f"lsx_lange_{self._suffix(A)}_dev"
        N.check(getattr(self.lib, name)(self.h.ptr, code, A.shape[0], A.shape[1], A.data_ptr(), A.stride(0),
                                        out.data_ptr()), name)
        return out

    def rcond(self, LU: torch.Tensor, ipiv: torch.Tensor, anorm, norm=1) -> float:
        """Reciprocal condition number from factors in HBM (lsx_gecon_*_dev); anorm: that norm of the UNFACTORED
        matrix, a float or the tensor `norm` returned.  Synchronises the stream: the result is a host float."""
        import ctypes as C
        import math

        code = self._norm_code(norm)
        _rowmajor(LU, "rcond")
        if LU.shape[0] != LU.shape[1]:
            raise ValueError("rcond needs square factors")
        anorm = float(anorm.item()) if hasattr(anorm, "item") else float(anorm)
        if math.isnan(anorm) or anorm < 0:
            raise ValueError("anorm must be a norm of the unfactored matrix (not NaN, not negative)")
        rc = C.c_double(0.0)
        name = f"lsx_gecon_{self._suffix(LU)}_dev"
        N.check(getattr(self.lib, name)(self.h.ptr, code, LU.shape[0], LU.data_ptr(), LU.stride(0), ipiv.data_ptr(),
                                        anorm, C.byref(rc)), name)
        return rc.value

    def gerfs_(self, A: torch.Tensor, LU: torch.Tensor, ipiv: torch.Tensor, B: torch.Tensor, X: torch.Tensor,
               trans: bool = False):
        """Refine X (a solution of A X = B, or A^T X = B with trans=True) in place from the factors LU / ipiv of A and
        bound its error: LAPACK's gerfs on tensors in HBM (lsx_gerfs_*_dev).  Returns (ferr, berr) as numpy arrays,
        one entry per right-hand side.  Synchronises the stream: the host drives the iteration."""
        import ctypes as C

        import numpy as np

        for t, w in ((A, "A"), (LU, "LU"), (B, "B"), (X, "X")):
            _rowmajor(t, "gerfs_ " + w)
        n = A.shape[0]
        if A.shape[1] != n or LU.shape != A.shape or B.shape[0] != n or X.shape != B.shape:
            raise ValueError("gerfs_: need a square matrix, its factors, and B / X with as many rows")
        if not (A.dtype == LU.dtype == B.dtype == X.dtype):
            raise TypeError("gerfs_: all operands must have the same dtype")
        if ipiv.dtype != torch.int32 or not ipiv.is_cuda or ipiv.dim() != 1 or not ipiv.is_contiguous() or ipiv.numel() < n:
            raise ValueError("gerfs_: ipiv must be a contiguous int32 tensor on the GPU with at least n entries")
        nrhs = B.shape[1]
        ferr, berr = np.zeros(max(nrhs, 1)), np.zeros(max(nrhs, 1))
        dp = C.POINTER(C.c_double)
        name = f"lsx_gerfs_{self._suffix(A)}_dev"
        N.check(getattr(self.lib, name)(self.h.ptr, int(bool(trans)), n, nrhs, A.data_ptr(), A.stride(0), LU.data_ptr(),
                                        LU.stride(0), ipiv.data_ptr(), B.data_ptr(), B.stride(0), X.data_ptr(),
                                        X.stride(0), ferr.ctypes.data_as(dp), berr.ctypes.data_as(dp)), name)
        return ferr[:nrhs], berr[:nrhs]

    def norm_sym(self, A: torch.Tensor) -> torch.Tensor:
        """1-norm (= infinity-norm) of a symmetric matrix in HBM given by its upper triangle: a device double[1], no
        host sync (lsx_lansy_*_dev).  The strictly lower triangle is not read."""
        _rowmajor(A, "norm_sym")
        if A.shape[0] != A.shape[1]:
            raise ValueError("norm_sym needs a square matrix")
        out = torch.zeros(1, dtype=torch.float64, device=A.device)
        name = f"lsx_lansy_{self._suffix(A)}_dev"
        N.check(getattr(self.lib, name)(self.h.ptr, A.shape[0], A.data_ptr(), max(A.stride(0), 1), out.data_ptr()), name)
        return out

    def pocon(self, U: torch.Tensor, anorm) -> float:
        """Reciprocal condition number from a Cholesky factor in HBM (lsx_pocon_*_dev); anorm: the 1-norm of the
        UNFACTORED matrix, a float or the tensor `norm_sym` returned.  Only the upper triangle of U is read.
        Synchronises the stream: the result is a host float."""
        import ctypes as C
        import math

        _rowmajor(U, "pocon")
        if U.shape[0] != U.shape[1]:
            raise ValueError("pocon needs the square factor")
        anorm = float(anorm.item()) if hasattr(anorm, "item") else float(anorm)
        if math.isnan(anorm) or anorm < 0:
            raise ValueError("anorm must be a norm of the unfactored matrix (not NaN, not negative)")
        rc = C.c_double(0.0)
        name = f"lsx_pocon_{self._suffix(U)}_dev"
        N.check(getattr(self.lib, name)(self.h.ptr, U.shape[0], U.data_ptr(), max(U.stride(0), 1), anorm, C.byref(rc)),
                name)
        return rc.value

    def porfs_(self, A: torch.Tensor, U: torch.Tensor, B: torch.Tensor, X: torch.Tensor):
        """Refine X (a solution of A X = B) in place from the Cholesky factor U of the symmetric positive definite A
        and bound its error: LAPACK's porfs on tensors in HBM (lsx_porfs_*_dev).  Only the upper triangles of A and U
        are read.  Returns (ferr, berr) as numpy arrays, one entry per right-hand side.  Synchronises the stream: the
        host drives the iteration."""
        import ctypes as C

        import numpy as np

        for t, w in ((A, "A"), (U, "U"), (B, "B"), (X, "X")):
            _rowmajor(t, "porfs_ " + w)
        n = A.shape[0]
        if A.shape[1] != n or U.shape != A.shape or B.shape[0] != n or X.shape != B.shape:
            raise ValueError("porfs_: need a square matrix, its factor, and B / X with as many rows")
        if not (A.dtype == U.dtype == B.dtype == X.dtype):
            raise TypeError("porfs_: all operands must have the same dtype")
        nrhs = B.shape[1]
        ferr, berr = np.zeros(max(nrhs, 1)), np.zeros(max(nrhs, 1))
        dp = C.POINTER(C.c_double)
        name = f"lsx_porfs_{self._suffix(A)}_dev"
        N.check(getattr(self.lib, name)(self.h.ptr, n, nrhs, A.data_ptr(), max(A.stride(0), 1), U.data_ptr(),
                                        max(U.stride(0), 1), B.data_ptr(), max(B.stride(0), 1), X.data_ptr(),
                                        max(X.stride(0), 1), ferr.ctypes.data_as(dp), berr.ctypes.data_as(dp)), name)
        return ferr[:nrhs], berr[:nrhs]

    def geequ(self, A: torch.Tensor):
        """LAPACK's geequ on a tensor in HBM (lsx_geequ_*_dev): returns (r, c, stats) as device tensors -- the row and
        column scale factors in A's dtype and stats = [rowcnd, colcnd, amax, info] (4 doubles).  No host sync."""
        _rowmajor(A, "geequ")
        m, n = A.shape
        r = torch.ones(max(m, 1), dtype=A.dtype, device=A.device)
        c = torch.ones(max(n, 1), dtype=A.dtype, device=A.device)
        stats = torch.zeros(4, dtype=torch.float64, device=A.device)
        name = f"lsx_geequ_{self._suffix(A)}_dev"
        N.check(getattr(self.lib, name)(self.h.ptr, m, n, A.data_ptr(), A.stride(0), r.data_ptr(), c.data_ptr(),
                                        stats.data_ptr()), name)
        return r[:m], c[:n], stats

    def laqge_(self, A: torch.Tensor, r: torch.Tensor, c: torch.Tensor, rowcnd: float, colcnd: float, amax: float) -> int:
        """LAPACK's laqge (lsx_laqge_*_dev): scale A in place by the factors of `geequ` if rowcnd, colcnd and amax
        (host floats: stats.tolist()[:3]) say it is worth it.  Returns equed (N.EQUED_*)."""
        import ctypes as C

        _rowmajor(A, "laqge_")
        m, n = A.shape
        for v, k, w in ((r, m, "r"), (c, n, "c")):
            if v.dtype != A.dtype or not v.is_cuda or v.dim() != 1 or (k > 1 and v.stride(0) != 1) or v.numel() < k:
                raise ValueError(f"laqge_: {w} must be a contiguous GPU vector of A's dtype with one entry per "
                                 f"{'row' if w == 'r' else 'column'}")
        equed = C.c_int(0)
        name = f"lsx_laqge_{self._suffix(A)}_dev"
        N.check(getattr(self.lib, name)(self.h.ptr, m, n, A.data_ptr(), A.stride(0), r.data_ptr(), c.data_ptr(),
                                        float(rowcnd), float(colcnd), float(amax), C.byref(equed)), name)
        return equed.value

    def gesvx_(self, A: torch.Tensor, B: torch.Tensor, trans: bool = False, equilibrate: bool = True,
               LU: Optional[torch.Tensor] = None, X: Optional[torch.Tensor] = None):
        """LAPACK's expert driver on tensors in HBM (lsx_gesvx_*_dev) with LAPACK's in / out contract: A leaves
        EQUILIBRATED and B scaled, in place.  Returns a dict: X (the solution of the system as passed in), LU, ipiv
        (factors of the equilibrated matrix), r, c (device tensors), equed, rowcnd, colcnd, rcond, rpvgrw, info (host
        scalars) and ferr, berr (numpy arrays).  B may have zero columns.  Synchronises the stream.
        X is a solution only when info is 0 or n + 1 AND rcond is no NaN: info in 1..n (an exactly zero pivot) leaves X
        as it was (all NaN when this method allocated it), and a NaN in A gives info = 0 with rcond = NaN and X all
        NaN."""
        import ctypes as C

        import numpy as np

        _rowmajor(A, "gesvx_ A")
        n = A.shape[0]
        if B.dim() != 2 or A.shape[1] != n or B.shape[0] != n:
            raise ValueError("gesvx_: need a square matrix and a right-hand side with as many rows")
        nrhs = B.shape[1]
        if nrhs == 0:                      # no right-hand sides: whatever strides an empty tensor reports
            B = torch.empty(n, 0, dtype=B.dtype, device=B.device)
            X = None
        _rowmajor(B, "gesvx_ B")
        if LU is None:
            LU = torch.empty(n, n, dtype=A.dtype, device=A.device)
        if X is None:       # NaN, not whatever the allocator hands out: an exactly zero pivot leaves X unwritten
            X = torch.full((n, nrhs), float("nan"), dtype=A.dtype, device=A.device)
        _rowmajor(LU, "gesvx_ LU")
        _rowmajor(X, "gesvx_ X")
        if tuple(LU.shape) != (n, n) or tuple(X.shape) != (n, nrhs) or not (A.dtype == B.dtype == LU.dtype == X.dtype):
            raise ValueError("gesvx_: LU must be n x n, X n x nrhs, all of one dtype")
        ipiv = torch.empty(max(n, 1), dtype=torch.int32, device=A.device)
        r = torch.ones(max(n, 1), dtype=A.dtype, device=A.device)
        c = torch.ones(max(n, 1), dtype=A.dtype, device=A.device)
        ferr, berr = np.zeros(max(nrhs, 1)), np.zeros(max(nrhs, 1))
        equed, info = C.c_int(0), C.c_int(0)
        rowcnd, colcnd, rc, growth = C.c_double(1.0), C.c_double(1.0), C.c_double(0.0), C.c_double(0.0)
        dp = C.POINTER(C.c_double)
        name = f"lsx_gesvx_{self._suffix(A)}_dev"
        N.check(getattr(self.lib, name)(self.h.ptr, int(bool(equilibrate)), int(bool(trans)), n, nrhs, A.data_ptr(),
                                        max(A.stride(0), 1), LU.data_ptr(), max(LU.stride(0), 1), ipiv.data_ptr(),
                                        B.data_ptr(), max(B.stride(0), 1), X.data_ptr(), max(X.stride(0), 1),
                                        C.byref(equed), r.data_ptr(), c.data_ptr(), C.byref(rowcnd), C.byref(colcnd),
                                        C.byref(rc), ferr.ctypes.data_as(dp), berr.ctypes.data_as(dp), C.byref(growth),
                                        C.byref(info)), name)
        return dict(X=X, LU=LU, ipiv=ipiv[:n], r=r[:n], c=c[:n], equed=equed.value, rowcnd=rowcnd.value,
                    colcnd=colcnd.value, rcond=rc.value, rpvgrw=growth.value, info=info.value, ferr=ferr[:nrhs],
                    berr=berr[:nrhs])

    def getri(self, LU: torch.Tensor, ipiv: torch.Tensor, out: Optional[torch.Tensor] = None):
        _rowmajor(LU, "getri")
        n = LU.shape[0]
        if out is None:
            out = torch.empty(n, n, dtype=LU.dtype, device=LU.device)
        fn = getattr(self.lib, f"lsx_getri_{self._suffix(LU)}_dev")
        N.check(fn(self.h.ptr, n, LU.data_ptr(), LU.stride(0), ipiv.data_ptr(), out.data_ptr(), out.stride(0)), "getri_dev")
        return out

    def det_parts(self, LU: torch.Tensor, ipiv: torch.Tensor) -> torch.Tensor:
        """Device tensor [sign, mant, exp2]."""
        out = torch.empty(3, dtype=torch.float64, device=LU.device)
        fn = getattr(self.lib, f"lsx_det_{self._suffix(LU)}_dev")
        N.check(fn(self.h.ptr, LU.shape[0], LU.data_ptr(), LU.stride(0), ipiv.data_ptr(), out.data_ptr()), "det_dev")
        return out

    def gesv_refined(self, A: torch.Tensor, B: torch.Tensor, sweeps: int = 3):
        """Mixed-precision solve on tensors in HBM: A (n x n fp32, kept), B (n x nrhs fp32, kept).  Returns
        (X fp64, X fp32, LU fp32, ipiv, info, stats) -- stats = [max|d|, max|x|] of the last sweep, then of the
        unrefined solve (device tensor, 4 doubles).  lsx_gesv_f32_refined_dev; asynchronous."""
        _rowmajor(A, "gesv_refined")
        _rowmajor(B, "gesv_refined")
        if A.dtype != torch.float32 or B.dtype != torch.float32:
            raise TypeError("gesv_refined takes fp32 operands")
        n, nrhs = A.shape[0], B.shape[1]
        LU = torch.empty(n, n, dtype=torch.float32, device=A.device)
        X64 = torch.empty(n, nrhs, dtype=torch.float64, device=A.device)
        X32 = torch.empty(n, nrhs, dtype=torch.float32, device=A.device)
        ipiv = torch.empty(max(n, 1), dtype=torch.int32, device=A.device)
        info = torch.zeros(1, dtype=torch.int32, device=A.device)
        stats = torch.zeros(4, dtype=torch.float64, device=A.device)
        N.check(self.lib.lsx_gesv_f32_refined_dev(self.h.ptr, n, nrhs, A.data_ptr(), A.stride(0), LU.data_ptr(), n,
                                                  ipiv.data_ptr(), info.data_ptr(), B.data_ptr(), B.stride(0),
                                                  X64.data_ptr(), nrhs, X32.data_ptr(), nrhs, int(sweeps),
                                                  stats.data_ptr()), "gesv_refined_dev")
        return X64, X32, LU, ipiv, info, stats

    def gemm_sub_(self, C: torch.Tensor, A: torch.Tensor, B: torch.Tensor):
        """C -= A @ B on the MFMA kernel."""
        for t, w in ((C, "C"), (A, "A"), (B, "B")):
            _rowmajor(t, "gemm_sub_ " + w)
        m, k = A.shape
        n = B.shape[1]
        assert B.shape[0] == k and C.shape == (m, n)
        fn = getattr(self.lib, f"lsx_gemm_sub_{self._suffix(C)}_dev")
        N.check(fn(self.h.ptr, m, n, k, A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), C.data_ptr(),
                   C.stride(0)), "gemm_sub_dev")
        return C

    def gemm_add_(self, C: torch.Tensor, A: torch.Tensor, B: torch.Tensor):
        """C += A @ B (fp64) on the same kernel."""
        for t, w in ((C, "C"), (A, "A"), (B, "B")):
            _rowmajor(t, "gemm_add_ " + w)
        m, k = A.shape
        n = B.shape[1]
        assert B.shape[0] == k and C.shape == (m, n) and C.dtype == torch.float64
        N.check(self.lib.lsx_gemm_add_f64_dev(self.h.ptr, m, n, k, A.data_ptr(), A.stride(0), B.data_ptr(),
                                              B.stride(0), C.data_ptr(), C.stride(0)), "gemm_add_dev")
        return C

    def _gemm_tn(self, name: str, C: torch.Tensor, A: torch.Tensor, B: torch.Tensor):
        for t, w in ((C, "C"), (A, "A"), (B, "B")):
            _rowmajor(t, name + "_ " + w)
        k, m = A.shape
        n = B.shape[1]
        if B.shape[0] != k or tuple(C.shape) != (m, n):
            raise ValueError(f"{name}_: need A (k x m), B (k x n) and C (m x n)")
        if not (A.dtype == B.dtype == C.dtype):
            raise TypeError(f"{name}_: all operands must have the same dtype")
        fn = getattr(self.lib, f"lsx_{name}_{self._suffix(C)}_dev")
        N.check(fn(self.h.ptr, m, n, k, A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), C.data_ptr(),
                   C.stride(0)), name + "_dev")
        return C

    def gemm_tn_sub_(self, C: torch.Tensor, A: torch.Tensor, B: torch.Tensor):
        """C -= A.T @ B with A stored k x m (a block row of the factors), on the MFMA kernel; fp64 or fp32."""
        return self._gemm_tn("gemm_tn_sub", C, A, B)

    def gemm_tn_add_(self, C: torch.Tensor, A: torch.Tensor, B: torch.Tensor):
        """C += A.T @ B (fp64) on the same kernel."""
        if C.dtype != torch.float64:
            raise TypeError("gemm_tn_add_ takes fp64 operands")
        return self._gemm_tn("gemm_tn_add", C, A, B)

    def panel_(self, P: torch.Tensor, row0: int, ipiv: torch.Tensor, info: torch.Tensor):
        _rowmajor(P, "panel_")
        N.check(self.lib.lsx_panel_f64_dev(self.h.ptr, P.shape[0], P.shape[1], P.data_ptr(), P.stride(0), row0,
                                           ipiv.data_ptr(), info.data_ptr()), "panel_dev")

    def laswp_(self, A: torch.Tensor, row0: int, jb: int, ipiv: torch.Tensor):
        _rowmajor(A, "laswp_")
        N.check(self.lib.lsx_laswp_f64_dev(self.h.ptr, A.shape[1], A.data_ptr(), A.stride(0), row0, jb,
                                           ipiv.data_ptr()), "laswp_dev")

    def panel_moves_(self, moves: torch.Tensor) -> bool:
        """Copy the gather list of the last panel_ call into `moves` (int32[512]); False if none."""
        import ctypes as C
        ok = C.c_int(0)
        N.check(self.lib.lsx_panel_moves_dev(self.h.ptr, moves.data_ptr(), C.byref(ok)), "panel_moves_dev")
        return bool(ok.value)

    def laswp_moves_(self, A: torch.Tensor, row0: int, moves: torch.Tensor):
        _rowmajor(A, "laswp_moves_")
        N.check(self.lib.lsx_laswp_moves_f64_dev(self.h.ptr, A.shape[1], A.data_ptr(), A.stride(0), row0,
                                                 moves.data_ptr()), "laswp_moves_dev")

    def trsm_lu_(self, L: torch.Tensor, B: torch.Tensor):
        _rowmajor(L, "trsm_lu_")
        _rowmajor(B, "trsm_lu_")
        N.check(self.lib.lsx_trsm_lu_f64_dev(self.h.ptr, L.shape[0], B.shape[1], L.data_ptr(), L.stride(0),
                                             B.data_ptr(), B.stride(0)), "trsm_lu_dev")

    def rref_(self, R: torch.Tensor, bar_col: int = 0, tol: float = -1.0, pivot_rule: int = N.PIVOT_FIRST):
        _rowmajor(R, "rref_")
        m, n = R.shape
        piv = torch.zeros(2 * min(m, n), dtype=torch.int32, device=R.device)
        rank = torch.zeros(1, dtype=torch.int32, device=R.device)
        N.check(self.lib.lsx_rref_f64_dev(self.h.ptr, m, n, bar_col, R.data_ptr(), R.stride(0), piv.data_ptr(),
                                          rank.data_ptr(), tol, pivot_rule), "rref_dev")
        return piv, rank
