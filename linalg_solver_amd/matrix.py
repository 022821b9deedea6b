"""`Matrix`: host-side mirror of the reference's row-reduction surface.

Same names, argument order, defaults, return types and error behaviour as
koskja/linalg-solver's ``linalg_solver.linalg.Matrix`` for the path this
package replaces (citations are to /root/reference/linalg_solver/linalg.py):

    Matrix(items)                      :14-32   validation, public ``items``
    row_reduce(bar_col=None)           :534-630 -> (items, pivots, mats, steps)
    find_preimage_of(vec, log_*...)    :632-680 -> AffineSubspace | NoSolution
    inverse(log_*...)                  :682-743 -> Matrix | NoSolution
    determinant(...)                   :183-207 -> scalar
    rank()                             :745-747 -> int
    kernel()                           :749-756
    AffineSubspace / NoSolution        :491-532
    zero / identity / new_vector / transpose   :410-415, 483-489
    __mul__ / scalar_mul / __neg__             :91-158 (matrix products on the MFMA tile)

All arithmetic runs on the GPU through liblsx.so (dense.py -> _native.py).
There is no CPU fallback: entries must be Python/numpy ints or floats, anything
else (Fraction, sympy objects, Polynomial) raises TypeError -- exact and
symbolic entries remain the reference's job.

Deliberate differences (documented in DESIGN.md):
  * no per-step LaTeX: ``row_reduce`` returns empty ``intermediate_matrices`` /
    ``intermediate_steps`` (these cost the reference >99 % of its run time);
    the ``log_*`` flags are accepted and ignored.
  * pivoting is by largest magnitude with a tolerance (32*eps*max(m,n)*max|working matrix left of bar_col|), so
    ``rank`` / pivot positions are those of exact arithmetic rather than the
    rounding artefacts an exact ``== 0`` test produces on floats
    (SURVEY.md appendix A.9).
  * reduced entries are always ``float`` (the reference leaves untouched entries
    as ``int``); ``determinant`` of an integer matrix is a ``float``.
"""
from __future__ import annotations

import math
from typing import Any, List, Optional, Tuple

import numpy as np

from . import dense

_NUMERIC = (int, float, np.integer, np.floating)


def _pow2_shift(amax: float) -> int:
    """The k for which amax * 2^k lies in [1/2, 1) when amax is further than 2^500 from 1, else 0.  solve_array and
    the inverse multiply such a matrix (and right-hand side) by 2^k before the factorisation and take the power back
    out of the result, so that the block inverses the solves form -- whose entries are reciprocals of pivots -- stay
    finite for a matrix of entries near the ends of the exponent range.  The first step is exact for every entry that
    is still a normal number after it: an entry more than about 2^1022 below the largest one underflows (in
    diag(1e200, 1e-200) one entry becomes 0; the pivot-ratio rule calls such a matrix singular at any scale).  The
    second step is one IEEE multiplication: exact unless the true result overflows (inf) or is subnormal."""
    if not (amax > 0.0) or math.isinf(amax):
        return 0
    e = math.frexp(amax)[1]
    return -e if abs(e) > 500 else 0


def _ldexp_t(t, k: int):
    """torch tensor * 2^k in two steps (2^k itself may not be a finite number); the first leaves every entry that
    the product keeps normal exact, so the result is rounded once at most."""
    return t if k == 0 else (t * math.ldexp(1.0, k // 2)) * math.ldexp(1.0, k - k // 2)


def _as_array(items: List[List[Any]]) -> np.ndarray:
    for row in items:
        for v in row:
            if not isinstance(v, _NUMERIC):
                raise TypeError(
                    f"linalg_solver_amd.Matrix computes on the GPU in fp64 and accepts only int/float "
                    f"entries; got {type(v).__name__}. Exact or symbolic entries are not supported.")
    return np.array(items, dtype=np.float64, order="C").reshape(len(items), len(items[0]) if items else 0)


class Matrix:
    """Mirror of the reference's `Matrix` carrier (linalg.py:11-58).  `items` is the public, mutable
    list-of-lists of the reference.  A matrix built with `from_numpy` / `from_dlpack` keeps the array
    and materialises `items` only when somebody asks for it: at N >= 4096 the O(N^2) Python objects cost
    seconds, the factorisation milliseconds."""

    def __init__(self, items: List[List[Any]], *, backend: str = "auto"):
        # SURVEY 8b's opt-in selector.  "auto" and "hip" are the same thing here -- this package IS the HIP path and
        # ships no other; "cpu" is refused rather than served by a Python fall-back (the reference is the CPU path).
        if backend not in ("auto", "hip"):
            if backend == "cpu":
                raise NotImplementedError("linalg_solver_amd has no CPU backend by design: use the reference "
                                          "linalg_solver.Matrix for exact/symbolic or CPU-only work")
            raise ValueError(f"unknown backend {backend!r}: expected 'auto' or 'hip'")
        self.backend = "hip"
        # linalg.py:14-32 -- same checks, same messages
        if not items:
            raise ValueError("Matrix cannot be empty")
        if not all(isinstance(row, list) for row in items):
            raise ValueError("Matrix items must be a list of lists")
        if not items[0]:
            if any(row for row in items):
                raise ValueError("Matrix rows cannot be empty if columns exist")
            row_len = 0
        else:
            row_len = len(items[0])
            if not all(len(row) == row_len for row in items):
                raise ValueError("All matrix rows must have the same length")
        self._cols = row_len
        self._items = items
        self._src = None   # array backing (from_numpy); dropped as soon as `items` is handed out
        self._dev = None   # device backing (from_dlpack of a tensor in HBM): a view, never copied to the host unasked

    def _host(self):
        """The array backing on the host, fetched from the device view on first need."""
        if self._src is None and getattr(self, "_dev", None) is not None:
            self._src = self._dev.detach().cpu().numpy()
        return self._src

    @property
    def items(self) -> List[List[Any]]:
        if self._items is None:
            self._items = self._host().tolist()
            self._src = None   # the lists are mutable: from here on they are the only truth
            self._dev = None
        return self._items

    @items.setter
    def items(self, value: List[List[Any]]):
        self._items = value
        self._src = None
        self._dev = None

    def _array(self) -> np.ndarray:
        """fp64 image of the entries for the device (validated)."""
        if self._items is None:
            return np.ascontiguousarray(self._host(), dtype=np.float64)
        return _as_array(self._items)

    # ---- container surface ------------------------------------------------
    def __str__(self) -> str:
        return "\n".join(" ".join(str(v) for v in row) for row in self.items)

    def __repr__(self) -> str:
        return f"Matrix({self.items!r})"

    @property
    def rows(self) -> int:
        if self._items is None:
            return (self._dev if getattr(self, "_dev", None) is not None else self._src).shape[0]
        return len(self._items)

    @property
    def cols(self) -> int:
        if self._items is None:
            return (self._dev if getattr(self, "_dev", None) is not None else self._src).shape[1]
        return len(self._items[0]) if self._items else self._cols

    def get_row(self, i: int) -> List[Any]:
        return self.items[i]

    def get_col(self, j: int) -> List[Any]:
        return [row[j] for row in self.items]

    def set_item(self, i: int, j: int, value: Any):
        self.items[i][j] = value
        return self

    @classmethod
    def zero(cls, rows: int, cols: int) -> "Matrix":
        return cls([[0] * cols for _ in range(rows)])

    @classmethod
    def identity(cls, size: int) -> "Matrix":
        return cls([[1 if i == j else 0 for j in range(size)] for i in range(size)])

    @classmethod
    def new_vector(cls, items: List[Any]) -> "Matrix":
        return cls([[v] for v in items])

    @classmethod
    def from_numpy(cls, a) -> "Matrix":
        """2-D integer or floating array -> Matrix without creating the list-of-lists (made on first use
        of `.items`; integer dtypes give int entries, as the reference's examples use)."""
        a = np.array(a, copy=True, order="C")
        if a.ndim != 2 or a.shape[0] == 0:
            raise ValueError("from_numpy needs a non-empty 2-D array")
        if a.dtype.kind not in "iuf":
            raise TypeError(f"from_numpy needs an integer or floating array, got dtype {a.dtype}")
        m = cls.__new__(cls)
        m.backend = "hip"
        m._cols = a.shape[1]
        m._items = None
        m._src = a
        m._dev = None
        return m

    @classmethod
    def from_dlpack(cls, x) -> "Matrix":
        """Any DLPack producer -> Matrix.  A 2-D floating tensor that lives in HBM (torch on the ROCm device) is kept
        as a VIEW: solve_array / inverse_array / lu_device then run on it through the device-pointer entry points
        (`*_dev`) and hand back device tensors, nothing crosses PCIe; the host copy and the list-of-lists are made
        only if `.items` / `to_numpy()` are asked for.  Host producers (numpy, CPU tensors) are copied as before."""
        if hasattr(x, "detach") and hasattr(x, "is_cuda"):
            if x.is_cuda:
                if x.dim() != 2 or x.shape[0] == 0:
                    raise ValueError("from_dlpack needs a non-empty 2-D tensor")
                if not x.dtype.is_floating_point:
                    raise TypeError(f"from_dlpack of a device tensor needs a floating dtype, got {x.dtype}")
                m = cls.__new__(cls)
                m.backend = "hip"
                m._cols = x.shape[1]
                m._items = None
                m._src = None
                m._dev = x.detach()
                return m
            return cls.from_numpy(x.detach().numpy())
        return cls.from_numpy(np.from_dlpack(x))

    def to_numpy(self) -> np.ndarray:
        """fp64 copy of the entries."""
        return np.array(self._array(), copy=True)

    def __dlpack__(self, stream=None):
        if getattr(self, "_dev", None) is not None:
            return self._dev.__dlpack__(stream=stream) if stream is not None else self._dev.__dlpack__()
        return self.to_numpy().__dlpack__()

    def __dlpack_device__(self):
        if getattr(self, "_dev", None) is not None:
            return self._dev.__dlpack_device__()
        return self.to_numpy().__dlpack_device__()

    # ---- device-resident twins: operands and results stay in HBM ------------------------------------
    def _dev64(self):
        import torch

        t = self._dev
        return t if (t.dtype == torch.float64 and t.is_contiguous()) else t.to(torch.float64).contiguous()

    def lu_device(self):
        """(LU, ipiv, info) as device tensors: P A = L U of a matrix built from a device tensor (the view is not
        modified).  lsx_getrf_f64_dev."""
        from .device import DeviceSolver

        if getattr(self, "_dev", None) is None:
            raise ValueError("lu_device needs a Matrix built by from_dlpack from a tensor in HBM")
        dev = DeviceSolver(self._dev.device.index)
        LU = self._dev64().clone()
        ipiv, info = dev.getrf_(LU)
        return LU, ipiv, info

    def _solve_device(self, rhs, trans: bool = False):
        import torch

        from .device import DeviceSolver

        A = self._dev64()
        n = A.shape[0]
        if A.shape[1] != n:
            raise ValueError("solve_array needs a square matrix")
        dev = DeviceSolver(self._dev.device.index)
        ka = _pow2_shift(float(A.abs().max())) if n else 0
        A = _ldexp_t(A, ka)
        LU = A.clone()
        ipiv, info = dev.getrf_(LU)
        if rhs is None:
            X = _ldexp_t(dev.getri(LU, ipiv), ka)
        else:
            B = rhs if hasattr(rhs, "is_cuda") else torch.as_tensor(np.asarray(rhs, dtype=np.float64))
            B = B.to(device=A.device, dtype=torch.float64)
            vec = B.dim() == 1
            if B.shape[0] != n:
                raise ValueError("Matrix dimensions must match")
            kb = _pow2_shift(float(B.abs().max())) if B.numel() else 0
            X = _ldexp_t(B.reshape(n, -1).contiguous(), kb).clone()
            dev.getrs_(LU, ipiv, X, trans=trans)
            X = _ldexp_t(X, ka - kb)
            if vec:
                X = X[:, 0]
        # singular to working precision: the same test as the host path (smallest |pivot| against the largest entry)
        amax = float(A.abs().max()) if n else 0.0
        ratio = float(LU.diagonal().abs().min()) / amax if amax > 0 else 0.0
        code = int(info.item())
        if code < 0:
            # a cooperative kernel timed out on the device (lsx.h: lsx_check_status): that is a failure of the run,
            # not a property of the matrix -- never report it as "singular"
            dev.h.check_status()
            raise RuntimeError(f"device factorisation failed (info = {code})")
        if code != 0 or not (ratio > dense.EPS64 * n):
            return Matrix.NoSolution()
        return X

    # ---- array-valued twins of the list-valued API (no O(N^2) Python objects) ----------------------
    def row_reduce_array(self, bar_col: int = None):
        """row_reduce on arrays: (reduced ndarray, pivots)."""
        A = self._array()
        n = A.shape[1]
        if n == 0:
            raise IndexError("list index out of range")
        bar = bar_col or n - 1
        R, pivots = self._reduce(A, min(bar, n))
        if bar > n and len(pivots) < A.shape[0]:
            raise IndexError("list index out of range")
        return R, pivots

    def _solve_bounded(self, rhs, trans: bool):
        """solve_array(bounds=True): factor once, solve, refine and bound (lsx_gerfs_*); NoSolution by the rule of
        solve_array (exactly zero pivot, or smallest |pivot| / largest |entry| <= n eps)."""
        if getattr(self, "_dev", None) is not None and self._items is None:
            import torch

            from .device import DeviceSolver

            A = self._dev64()
            n = A.shape[0]
            if A.shape[1] != n:
                raise ValueError("solve_array needs a square matrix")
            dev = DeviceSolver(self._dev.device.index)
            ka = _pow2_shift(float(A.abs().max())) if n else 0
            A = _ldexp_t(A, ka)          # a copy when ka != 0: the caller's tensor is never written
            LU = A.clone()
            ipiv, info = dev.getrf_(LU)
            B = rhs if hasattr(rhs, "is_cuda") else torch.as_tensor(np.asarray(rhs, dtype=np.float64))
            B = B.to(device=A.device, dtype=torch.float64)
            vec = B.dim() == 1
            if B.shape[0] != n:
                raise ValueError("Matrix dimensions must match")
            kb = _pow2_shift(float(B.abs().max())) if B.numel() else 0
            B = _ldexp_t(B.reshape(n, -1).contiguous(), kb)
            code = int(info.item())
            if code < 0:
                dev.h.check_status()
                raise RuntimeError(f"device factorisation failed (info = {code})")
            amax = float(A.abs().max()) if n else 0.0
            ratio = float(LU.diagonal().abs().min()) / amax if amax > 0 else 0.0
            if code != 0 or not (ratio > dense.EPS64 * n):
                return Matrix.NoSolution()
            X = B.clone()
            dev.getrs_(LU, ipiv, X, trans=trans)
            ferr, berr = dev.gerfs_(A, LU, ipiv, B, X, trans=trans)   # both bounds are relative: scale-free
            X = _ldexp_t(X, ka - kb)
            return (X[:, 0], float(ferr[0]), float(berr[0])) if vec else (X, ferr, berr)
        A = self._array()
        n = A.shape[0]
        if A.shape[1] != n:
            raise ValueError("solve_array needs a square matrix")
        B = np.asarray(rhs, dtype=np.float64)
        vec = B.ndim == 1
        if B.shape[0] != n:
            raise ValueError("Matrix dimensions must match")
        ka = _pow2_shift(float(np.abs(A).max(initial=0.0)))
        kb = _pow2_shift(float(np.abs(B).max(initial=0.0)))
        A, B = np.ldexp(A, ka), np.ldexp(B.reshape(n, -1), kb)
        LU, ipiv, info = dense.lu_factor(A)
        amax = float(np.max(np.abs(A))) if n else 0.0
        ratio = float(np.min(np.abs(np.diagonal(LU)))) / amax if amax > 0 else 0.0
        if info != 0 or not (ratio > dense.EPS64 * n):
            return Matrix.NoSolution()
        X = dense.lu_solve(LU, ipiv, B, trans=trans)
        X, ferr, berr = dense.lu_refine(A, LU, ipiv, B, X, trans=trans)   # both bounds are relative: scale-free
        X = np.ldexp(X, ka - kb)
        return (X[:, 0], float(ferr[0]), float(berr[0])) if vec else (X, ferr, berr)

    def _solve_equilibrated(self, rhs, trans: bool, bounds: bool):
        """solve_array(equilibrate=True): LAPACK's expert driver (lsx_gesvx_*); NoSolution by LAPACK's criterion, info in
        1..n (an exactly zero pivot) or info == n + 1 (rcond of the equilibrated matrix below the unit roundoff)."""
        if getattr(self, "_dev", None) is not None and self._items is None:
            import torch

            from .device import DeviceSolver

            A = self._dev64()
            n = A.shape[0]
            if A.shape[1] != n:
                raise ValueError("solve_array needs a square matrix")
            B = rhs if hasattr(rhs, "is_cuda") else torch.as_tensor(np.asarray(rhs, dtype=np.float64))
            B = B.to(device=A.device, dtype=torch.float64)
            vec = B.dim() == 1
            if B.shape[0] != n:
                raise ValueError("Matrix dimensions must match")
            dev = DeviceSolver(self._dev.device.index)
            out = dev.gesvx_(A.clone(), B.reshape(n, -1).contiguous().clone(), trans=trans)   # the driver scales in place
            X, ferr, berr, info = out["X"], out["ferr"], out["berr"], out["info"]
            if math.isnan(out["rcond"]):        # a NaN in the matrix: nothing was solved (the host path's x = None)
                X = None
        else:
            A = self._array()
            n = A.shape[0]
            if A.shape[1] != n:
                raise ValueError("solve_array needs a square matrix")
            B = np.asarray(rhs, dtype=np.float64)
            vec = B.ndim == 1
            if B.shape[0] != n:
                raise ValueError("Matrix dimensions must match")
            X, ferr, berr, _, _, _, _, _, info = dense.solve_expert(A, B.reshape(n, -1), trans=trans)
        if info != 0 or X is None:
            return Matrix.NoSolution()
        if vec:
            return (X[:, 0], float(ferr[0]), float(berr[0])) if bounds else X[:, 0]
        return (X, ferr, berr) if bounds else X

    @staticmethod
    def _not_pos_def(info: int) -> ValueError:
        return ValueError(f"matrix is not positive definite: its leading minor of order {info} is not (pos_def=True "
                          "was the caller's assertion; without it the system may well have a solution)")

    def cholesky_array(self):
        """The upper Cholesky factor U (self = U^T U, zeros below the diagonal) of a symmetric positive definite
        matrix: an ndarray, or a device tensor for a matrix built from one.  Only the upper triangle of self is used;
        symmetry is not checked.  ValueError when a leading minor is not positive definite."""
        if getattr(self, "_dev", None) is not None and self._items is None:
            from .device import DeviceSolver

            A = self._dev64()
            if A.shape[0] != A.shape[1]:
                raise ValueError("cholesky_array needs a square matrix")
            U = A.clone()
            info = int(DeviceSolver(self._dev.device.index).potrf_(U).item()) if A.shape[0] else 0
            if info != 0:
                raise self._not_pos_def(info)
            return U.triu()
        A = self._array()
        if A.shape[0] != A.shape[1]:
            raise ValueError("cholesky_array needs a square matrix")
        U, info = dense.cho_factor(A)
        if info != 0:
            raise self._not_pos_def(info)
        return U

    def _solve_pos_def(self, rhs):
        """solve_array(pos_def=True): Cholesky factorisation and solve (lsx_potrf_* / lsx_potrs_*, lsx_posv_*)."""
        if getattr(self, "_dev", None) is not None and self._items is None:
            import torch

            from .device import DeviceSolver

            A = self._dev64()
            n = A.shape[0]
            if A.shape[1] != n:
                raise ValueError("solve_array needs a square matrix")
            B = rhs if hasattr(rhs, "is_cuda") else torch.as_tensor(np.asarray(rhs, dtype=np.float64))
            B = B.to(device=A.device, dtype=torch.float64)
            vec = B.dim() == 1
            if B.shape[0] != n:
                raise ValueError("Matrix dimensions must match")
            dev = DeviceSolver(self._dev.device.index)
            U = A.clone()
            info = int(dev.potrf_(U).item()) if n else 0
            if info != 0:
                raise self._not_pos_def(info)
            X = B.reshape(n, -1).contiguous().clone()
            if n and X.shape[1]:
                dev.potrs_(U, X)
            return X[:, 0] if vec else X
        A = self._array()
        n = A.shape[0]
        if A.shape[1] != n:
            raise ValueError("solve_array needs a square matrix")
        B = np.asarray(rhs, dtype=np.float64)
        vec = B.ndim == 1
        if B.shape[0] != n:
            raise ValueError("Matrix dimensions must match")
        X, info, _ = dense.solve(A, B.reshape(n, -1), assume_pos=True)
        if info != 0:
            raise self._not_pos_def(info)
        return X[:, 0] if vec else X

    def solve_pos_def_array(self, rhs, bounds: bool = False):
        """Solution(s) of self * X = rhs for a symmetric positive definite matrix through the Cholesky factorisation:
        solve_array(rhs, pos_def=True), and with bounds=True refined by LAPACK's porfs (lsx_porfs_* / lsx_posvr_*)
        and returned as (x, ferr, berr) like solve_array(bounds=True): per right-hand side a bound of
        max|x - x_true| / max|x| and the componentwise backward error (floats for a vector rhs, arrays for a matrix).
        One factorisation, no pivoting; only the upper triangle of self is used and symmetry is NOT checked.
        ValueError naming the minor when a leading minor is not positive definite."""
        if not bounds:
            return self._solve_pos_def(rhs)
        if getattr(self, "_dev", None) is not None and self._items is None:
            import torch

            from .device import DeviceSolver

            A = self._dev64()
            n = A.shape[0]
            if A.shape[1] != n:
                raise ValueError("solve_pos_def_array needs a square matrix")
            B = rhs if hasattr(rhs, "is_cuda") else torch.as_tensor(np.asarray(rhs, dtype=np.float64))
            B = B.to(device=A.device, dtype=torch.float64)
            vec = B.dim() == 1
            if B.shape[0] != n:
                raise ValueError("Matrix dimensions must match")
            dev = DeviceSolver(self._dev.device.index)
            U = A.clone()
            info = int(dev.potrf_(U).item()) if n else 0
            if info != 0:
                raise self._not_pos_def(info)
            B = B.reshape(n, -1).contiguous()
            X = B.clone()
            if n and X.shape[1]:
                dev.potrs_(U, X)
            ferr, berr = dev.porfs_(A, U, B, X)
            return (X[:, 0], float(ferr[0]), float(berr[0])) if vec else (X, ferr, berr)
        A = self._array()
        n = A.shape[0]
        if A.shape[1] != n:
            raise ValueError("solve_pos_def_array needs a square matrix")
        B = np.asarray(rhs, dtype=np.float64)
        vec = B.ndim == 1
        if B.shape[0] != n:
            raise ValueError("Matrix dimensions must match")
        X, ferr, berr, info = dense.solve_pos_bounded(A, B.reshape(n, -1))
        if info != 0:
            raise self._not_pos_def(info)
        return (X[:, 0], float(ferr[0]), float(berr[0])) if vec else (X, ferr, berr)

    def rcond_pos_def(self) -> float:
        """Reciprocal condition number 1 / (||A||_1 ||A^-1||_1) of a symmetric positive definite matrix from its
        Cholesky factorisation: LAPACK's pocon estimate (lsx_porcond_f64 / lsx_pocon_f64_dev).  Only the upper triangle
        of self is used.  ValueError naming the minor when a leading minor is not positive definite."""
        if getattr(self, "_dev", None) is not None and self._items is None:
            from .device import DeviceSolver

            A = self._dev64()
            if A.shape[0] != A.shape[1]:
                raise ValueError("rcond_pos_def needs a square matrix")
            dev = DeviceSolver(self._dev.device.index)
            anorm = dev.norm_sym(A)
            U = A.clone()
            info = int(dev.potrf_(U).item()) if A.shape[0] else 0
            if info != 0:
                raise self._not_pos_def(info)
            return dev.pocon(U, anorm)
        A = self._array()
        if A.shape[0] != A.shape[1]:
            raise ValueError("rcond_pos_def needs a square matrix")
        rc, info = dense.rcond_pos(A)
        if info != 0:
            raise self._not_pos_def(info)
        return rc

    def cond_pos_def(self) -> float:
        """Estimated 1-norm condition number 1 / rcond_pos_def(); inf when rcond_pos_def is 0."""
        r = self.rcond_pos_def()
        return float("inf") if r == 0.0 else 1.0 / r

    def solve_array(self, rhs, trans: bool = False, bounds: bool = False, equilibrate: bool = False,
                    pos_def: bool = False):
        """Unique solution(s) of self * X = rhs for a square matrix (rhs: vector or matrix) as an ndarray;
        NoSolution() when the matrix is singular to working precision (use find_preimage_of for the
        general affine answer).  trans=True solves self^T * X = rhs (x * self = rhs^T for rows) from the factors of
        self: no transposed copy, no second factorisation.  bounds=True refines the solution (LAPACK's gerfs) and
        returns (x, ferr, berr): per right-hand side a bound of max|x - x_true| / max|x| and the componentwise
        backward error (floats for a vector rhs, arrays for a matrix).
        equilibrate=True goes through LAPACK's expert driver (gesvx: row and column scaling where the matrix needs it,
        then factor, solve, refine): a matrix that is merely badly scaled -- which the pivot-ratio rule calls singular
        -- is solved, and NoSolution() is LAPACK's criterion instead (an exactly zero pivot, or the reciprocal condition
        number of the EQUILIBRATED matrix below 2^-53).  With bounds=True ferr is LAPACK's, which after a column
        scaling is divided by the scales' spread and can be vacuous (include/lsx.h); berr is not affected.
        pos_def=True asserts that self is symmetric positive definite and takes the Cholesky factorisation (no pivoting,
        half the work).  Only the upper triangle of self is used and symmetry is NOT checked.  trans is accepted and
        makes no difference (self is symmetric); bounds=True or equilibrate=True with it is a ValueError
        (solve_pos_def_array has the bounds).  If a leading
        minor turns out not to be positive definite the assertion was false: ValueError naming the minor, not
        NoSolution() -- the system may well have a solution."""
        if pos_def:
            if bounds or equilibrate:
                raise ValueError("solve_array: pos_def=True cannot be combined with bounds=True or equilibrate=True "
                                 "(solve_pos_def_array(rhs, bounds=True) gives the Cholesky solve with error bounds)")
            return self._solve_pos_def(rhs)
        if equilibrate:
            return self._solve_equilibrated(rhs, trans, bounds)
        if bounds:
            return self._solve_bounded(rhs, trans)
        if getattr(self, "_dev", None) is not None and self._items is None:
            return self._solve_device(rhs, trans)   # operands in HBM: the result is a device tensor too
        A = self._array()
        if A.shape[0] != A.shape[1]:
            raise ValueError("solve_array needs a square matrix")
        B = np.asarray(rhs, dtype=np.float64)
        vec = B.ndim == 1
        if B.shape[0] != A.shape[0]:
            raise ValueError("Matrix dimensions must match")
        ka = _pow2_shift(float(np.abs(A).max(initial=0.0)))
        kb = _pow2_shift(float(np.abs(B).max(initial=0.0)))
        X, info, ratio = dense.solve(np.ldexp(A, ka), np.ldexp(B.reshape(A.shape[0], -1), kb), trans=trans)
        if info != 0 or not (ratio > dense.EPS64 * A.shape[0]):
            return Matrix.NoSolution()
        X = np.ldexp(X, ka - kb)
        return X[:, 0] if vec else X

    def _rcond_equilibrated(self, norm) -> float:
        """gesvx without right-hand sides: trans picks the norm (the infinity-norm of A is the 1-norm of A^T)."""
        trans = dense._norm_code(norm) == dense.N.NORM_INF
        if getattr(self, "_dev", None) is not None and self._items is None:
            import torch

            from .device import DeviceSolver

            A = self._dev64()
            if A.shape[0] != A.shape[1]:
                raise ValueError("rcond needs a square matrix")
            dev = DeviceSolver(self._dev.device.index)
            B = torch.empty(A.shape[0], 0, dtype=torch.float64, device=A.device)
            return dev.gesvx_(A.clone(), B, trans=trans)["rcond"]
        A = self._array()
        if A.shape[0] != A.shape[1]:
            raise ValueError("rcond needs a square matrix")
        return dense.solve_expert(A, np.zeros((A.shape[0], 0)), trans=trans)[3]

    def rcond(self, norm=1, equilibrate: bool = False) -> float:
        """Reciprocal condition number 1 / (||A|| ||A^-1||) in the 1-norm (norm=1) or the infinity-norm
        (norm=inf): LAPACK's gecon estimate from the LU factors (lsx_rcond_f64 / lsx_gecon_f64_dev).  0.0 for a
        matrix with an exactly zero pivot.  Unlike the pivot ratio behind NoSolution it sees ill-conditioning that
        leaves every pivot large.  equilibrate=True: of the matrix after LAPACK's row / column equilibration
        (lsx_gesvx_* without right-hand sides) -- what is left of the conditioning once bad scaling is taken out."""
        if equilibrate:
            return self._rcond_equilibrated(norm)
        if getattr(self, "_dev", None) is not None and self._items is None:
            from .device import DeviceSolver

            A = self._dev64()
            if A.shape[0] != A.shape[1]:
                raise ValueError("rcond needs a square matrix")
            dev = DeviceSolver(self._dev.device.index)
            anorm = dev.norm(A, norm)
            LU = A.clone()
            ipiv, info = dev.getrf_(LU)
            code = int(info.item())
            if code < 0:
                dev.h.check_status()
                raise RuntimeError(f"device factorisation failed (info = {code})")
            return 0.0 if code != 0 else dev.rcond(LU, ipiv, anorm, norm)
        A = self._array()
        if A.shape[0] != A.shape[1]:
            raise ValueError("rcond needs a square matrix")
        return dense.rcond(A, norm)[0]

    def cond(self, norm=1, equilibrate: bool = False) -> float:
        """Estimated condition number 1 / rcond(norm, equilibrate); inf when rcond is 0."""
        r = self.rcond(norm, equilibrate)
        return float("inf") if r == 0.0 else 1.0 / r

    def _inverse_pos_def(self):
        """inverse_array(pos_def=True): Cholesky factorisation and LAPACK's potri (lsx_potrf_* / lsx_potri_*,
        lsx_poinv_*), mirrored into both triangles."""
        if getattr(self, "_dev", None) is not None and self._items is None:
            from .device import DeviceSolver

            A = self._dev64()
            n = A.shape[0]
            if A.shape[1] != n:
                raise ValueError("Matrix must be square to invert.")
            dev = DeviceSolver(self._dev.device.index)
            X = A.clone()
            info = int(dev.potrf_(X).item()) if n else 0
            if info != 0:
                raise self._not_pos_def(info)
            if n:
                dev.potri_(X)
                dev.symmetrize_upper_(X)
            return X
        A = self._array()
        if A.shape[0] != A.shape[1]:
            raise ValueError("Matrix must be square to invert.")
        X, info, _ = dense.inv(A, assume_pos=True)
        if info != 0:
            raise self._not_pos_def(info)
        return X

    def inverse_array(self, pos_def: bool = False) -> "np.ndarray | Matrix.NoSolution":
        """The inverse as an array (a device tensor for a matrix built from one), or NoSolution for a singular matrix.
        pos_def=True asserts that self is symmetric positive definite and takes the Cholesky route (no pivoting, half
        the work of the LU route); only the upper triangle of self is used, the result has both triangles, exactly
        symmetric.  If a leading minor is not positive definite the call raises ValueError, as solve_array(pos_def=True)
        does."""
        if pos_def:
            return self._inverse_pos_def()
        if getattr(self, "_dev", None) is not None and self._items is None:
            if self._dev.shape[0] != self._dev.shape[1]:
                raise ValueError("Matrix must be square to invert.")
            return self._solve_device(None)
        A = self._array()
        if A.shape[0] != A.shape[1]:
            raise ValueError("Matrix must be square to invert.")
        ka = _pow2_shift(float(np.abs(A).max(initial=0.0)))
        X, info, ratio = dense.inv(np.ldexp(A, ka))
        if info != 0 or not (ratio > dense.EPS64 * A.shape[0]):
            return Matrix.NoSolution()
        with np.errstate(over="ignore"):   # the inverse of a matrix of tiny entries may not be representable: inf there
            return np.ldexp(X, ka)

    # ---- Householder QR and least squares (lsx_geqrf_*, lsx_orgqr_*, lsx_gels_*) ----
    def qr_array(self):
        """(Q, R) as arrays (device tensors for a matrix built from one): the thin Q (rows x cols) and the upper
        triangular R (cols x cols) of self = Q R, for rows >= cols; ValueError otherwise."""
        if getattr(self, "_dev", None) is not None and self._items is None:
            import torch

            from .device import DeviceSolver

            QR = self._dev64().clone()
            m, n = QR.shape
            if m < n:
                raise ValueError("qr_array needs at least as many rows as columns")
            dev = DeviceSolver(self._dev.device.index)
            tau = dev.geqrf_(QR)
            return dev.orgqr(QR, tau), torch.triu(QR[:n, :])
        A = self._array()
        if A.shape[0] < A.shape[1]:
            raise ValueError("qr_array needs at least as many rows as columns")
        return dense.qr(A)

    def least_squares_array(self, rhs, residuals: bool = False, min_norm: bool = False, rcond=None):
        """The x that minimises ||rhs - self x||_2, through Householder QR, for rows >= cols (ValueError otherwise; an
        underdetermined system has no unique minimiser).  rhs: a vector or a rows x nrhs array.  residuals=True
        returns (x, ||rhs - self x||_2 per right-hand side).  NoSolution() when a diagonal entry of R is exactly zero or
        NaN -- self does not have full column rank -- as inverse_array answers for a singular matrix.  Unlike
        find_preimage_of this does not ask for a consistent system.
        min_norm=True: the minimiser of smallest 2-norm, through the SVD (lsx_gelss_*), for ANY shape and rank; singular
        values up to rcond * the largest (rcond=None: max(rows, cols) times the unit roundoff) count as zero.  It never
        answers NoSolution()."""
        if min_norm:
            return self._least_squares_min_norm(rhs, residuals, rcond)
        if getattr(self, "_dev", None) is not None and self._items is None:
            import torch

            from .device import DeviceSolver

            A = self._dev64().clone()
            m, n = A.shape
            if m < n:
                raise ValueError("least_squares_array needs at least as many rows as columns")
            B = rhs if hasattr(rhs, "is_cuda") else torch.as_tensor(np.asarray(rhs, dtype=np.float64))
            B = B.to(device=A.device, dtype=torch.float64)
            vec = B.dim() == 1
            if B.shape[0] != m:
                raise ValueError("Matrix dimensions must match")
            W = B.reshape(m, -1).contiguous().clone()
            dev = DeviceSolver(self._dev.device.index)
            _, info = dev.gels_(A, W)
            if int(info.item()) != 0:
                return Matrix.NoSolution()
            X = W[:n, 0].clone() if vec else W[:n].clone()
            if not residuals:
                return X
            res = dev.col_norms(W[n:]) if m > n else torch.zeros(W.shape[1], dtype=torch.float64, device=A.device)
            return X, (res[0] if vec else res)
        A = self._array()
        if A.shape[0] < A.shape[1]:
            raise ValueError("least_squares_array needs at least as many rows as columns")
        b = np.asarray(rhs, dtype=np.float64)
        if b.shape[:1] != (A.shape[0],):
            raise ValueError("Matrix dimensions must match")
        x, resid, info = dense.lstsq(A, b)
        if info != 0:
            return Matrix.NoSolution()
        return (x, resid) if residuals else x

    # ---- Jacobi SVD (lsx_gesvdj_*, lsx_gelss_*) ----
    def _on_device(self) -> bool:
        return getattr(self, "_dev", None) is not None and self._items is None

    def _least_squares_min_norm(self, rhs, residuals, rcond):
        if self._on_device():
            import torch

            from .device import DeviceSolver

            A = self._dev64()
            m = A.shape[0]
            B = rhs if hasattr(rhs, "is_cuda") else torch.as_tensor(np.asarray(rhs, dtype=np.float64))
            B = B.to(device=A.device, dtype=torch.float64)
            vec = B.dim() == 1
            if B.shape[0] != m:
                raise ValueError("Matrix dimensions must match")
            Bm = B.reshape(m, -1).contiguous()
            dev = DeviceSolver(self._dev.device.index)
            X = dev.gelss_(A.clone(), Bm, -1.0 if rcond is None else float(rcond))[0]
            x = X[:, 0].clone() if vec else X
            if not residuals:
                return x
            R = Bm.clone()
            dev.gemm_sub_(R, A.contiguous(), X)
            res = dev.col_norms(R)
            return x, (res[0] if vec else res)
        A = self._array()
        b = np.asarray(rhs, dtype=np.float64)
        if b.shape[:1] != (A.shape[0],):
            raise ValueError("Matrix dimensions must match")
        x, resid, _, _ = dense.lstsq_min_norm(A, b, rcond=rcond)
        return (x, resid) if residuals else x

    def svd_array(self):
        """(U, s, Vt) as arrays (device tensors for a matrix built from one): the thin factors of self = U diag(s) Vt
        with s descending, by one-sided Jacobi (lsx_gesvdj_*).  U is orthonormal for every input; rows of Vt that belong
        to an exactly zero singular value are zero rows."""
        if self._on_device():
            from .device import DeviceSolver

            U, s, Vt, _ = DeviceSolver(self._dev.device.index).gesvdj_(self._dev64().clone())
            return U, s, Vt
        U, s, Vt, _ = dense.svd(self._array())
        return U, s, Vt

    def singular_values(self):
        """The singular values, descending: a numpy array (a device tensor for a matrix built from one)."""
        if self._on_device():
            from .device import DeviceSolver

            return DeviceSolver(self._dev.device.index).gesvdj_(self._dev64().clone(), compute_uv=False)[1]
        return dense.svdvals(self._array())

    def _svals_host(self) -> "np.ndarray":
        s = self.singular_values()
        return s.cpu().numpy() if hasattr(s, "is_cuda") else s

    def norm2(self) -> float:
        """The 2-norm: the largest singular value (0.0 for a matrix without rows or columns)."""
        s = self._svals_host()
        return float(s[0]) if len(s) else 0.0

    def cond2(self) -> float:
        """The 2-norm condition number s[0] / s[-1]; inf when the smallest singular value is exactly zero."""
        s = self._svals_host()
        if not len(s):
            return 1.0
        return float("inf") if s[-1] == 0.0 else float(s[0] / s[-1])

    def numerical_rank(self, rcond=None) -> int:
        """The number of singular values above rcond * the largest (rcond=None: max(rows, cols) times the unit
        roundoff).  rank() keeps its pivot tolerance; this one has none."""
        s = self._svals_host()
        if not len(s):
            return 0
        if rcond is None:
            rcond = max(self.rows, self.cols) * dense.EPS64 / 2
        return int(np.sum(s > rcond * s[0]))

    def pinv_array(self, rcond=None):
        """The Moore-Penrose pseudo-inverse (cols x rows) as an array (a device tensor for a matrix built from one):
        lsx_gelss_* with the identity as right-hand sides."""
        if self._on_device():
            import torch

            from .device import DeviceSolver

            A = self._dev64()
            eye = torch.eye(A.shape[0], dtype=torch.float64, device=A.device)
            return DeviceSolver(self._dev.device.index).gelss_(A.clone(), eye, -1.0 if rcond is None else float(rcond))[0]
        return dense.pinv(self._array(), rcond=rcond)

    # ---- symmetric eigensolver by two-sided Jacobi (lsx_syevj_*) ----
    def eigh_array(self):
        """(w, V) as arrays (device tensors for a matrix built from one): self = V diag(w) V^T with w ascending and
        column i of V the eigenvector of w[i], by two-sided Jacobi (lsx_syevj_*).  Symmetry is the caller's assertion,
        the stance of pos_def=True: only the upper triangle is used.  ValueError for a non-square matrix.  Like
        svd_array this returns what the iteration reached even if the last allowed sweep still rotated; dense.eigh and
        DeviceSolver.syevj_ hand out that info word."""
        if self.rows != self.cols:
            raise ValueError("eigh_array needs a square matrix")
        if self._on_device():
            from .device import DeviceSolver

            w, V, _ = DeviceSolver(self._dev.device.index).syevj_(self._dev64().clone())
            return w, V
        w, V, _ = dense.eigh(self._array())
        return w, V

    def eigvalsh(self):
        """The eigenvalues of the symmetric matrix given by the upper triangle, ascending: a numpy array (a device
        tensor for a matrix built from one).  ValueError for a non-square matrix."""
        if self.rows != self.cols:
            raise ValueError("eigvalsh needs a square matrix")
        if self._on_device():
            from .device import DeviceSolver

            return DeviceSolver(self._dev.device.index).syevj_(self._dev64().clone(), compute_v=False)[0]
        return dense.eigvalsh(self._array())

    def transpose(self) -> "Matrix":
        return Matrix([[self.items[j][i] for j in range(self.rows)] for i in range(self.cols)])

    # ---- products (linalg.py:91-158): matrix x matrix on the GPU, scalars elementwise
    def scalar_mul(self, scalar: Any) -> "Matrix":
        return Matrix([[item * scalar for item in row] for row in self.items])  # linalg.py:91-92

    def __neg__(self) -> "Matrix":
        return self.scalar_mul(-1)

    def __mul__(self, other) -> "Matrix":
        if not isinstance(other, Matrix):
            return self.scalar_mul(other)  # linalg.py:101-103
        if self.cols != other.rows:
            raise ValueError("Matrix dimensions must match")  # linalg.py:104-105
        return Matrix(dense.matmul(self._array(), other._array()).tolist())

    def cformat(self, _arg_of: str = "") -> str:
        body = r"\\".join(" & ".join(_fmt(v) for v in row) for row in self.items)
        return r"\begin{pmatrix}" + body + r"\end{pmatrix}"

    # ---- result carriers (linalg.py:491-532) --------------------------------
    class AffineSubspace:
        def __init__(self, vec: List[Any], mat: Optional["Matrix"]):
            self.vec = vec
            self.generators = mat

        def get_one(self) -> List[Any]:
            return self.vec

        def dim(self) -> int:
            return self.generators.cols  # raises on None exactly like the reference (:500)

        def basis(self) -> List[List[Any]]:
            return self.generators.transpose().items

        def cformat(self, arg_of: str = "") -> str:
            g = self.generators
            point = Matrix.new_vector(self.vec).cformat()
            if g is None or g.rows == 0 or g.cols == 0:
                return " %s " % point
            gens = ", ".join(Matrix.new_vector(g.get_col(i)).cformat() for i in range(g.cols))
            span = r" \LO \left\{ %s \right\} " % gens
            return " %s %s  " % ("" if all(v == 0 for v in self.vec) else point + " + ", span)

        def __repr__(self) -> str:
            return f"AffineSubspace(vec={self.vec!r}, generators={self.generators!r})"

    class NoSolution:
        def __repr__(self) -> str:
            return "NoSolution()"

        def cformat(self, arg_of: str = "") -> str:
            return r"\text{Žádné řešení}"

    # ---- the replaced path --------------------------------------------------
    def _reduce(self, A: np.ndarray, bar: int) -> Tuple[np.ndarray, List[Tuple[int, int]]]:
        """RREF of A over columns [0, bar) on the GPU -> (reduced, pivots)."""
        m, n = A.shape
        if bar <= 0:
            return A.copy(), []
        if m == bar:
            # [A | B] with square A: blocked LU + two block solves instead of a 2n-wide
            # Gauss-Jordan (what linalg.py:649-656 / 704-711 spell as row_reduce(bar_col=n))
            X, info, ratio = dense.solve(A[:, :m], A[:, m:])
            if info == 0 and ratio > dense.EPS64 * m:
                R = np.zeros_like(A)
                R[:, :m] = np.eye(m)
                R[:, m:] = X
                return R, [(k, k) for k in range(m)]
        # Large inputs: ONE call.  The blocked first-rule reduction (csrc/api.hip: rref_first_fast) takes rank and pivot
        # columns from the rank-revealing pass and the reference's row choice (first non-zero row, linalg.py:548-552)
        # from a blocked LU of those columns under that rule, so its result IS the reference's reduction.
        h = dense._h(None)
        R1, pivots1, rank1 = dense.rref(A, bar_col=bar, pivot_rule=dense.N.PIVOT_FIRST)
        if h.get_option("rref_first_used"):
            return R1, pivots1
        # Small inputs (per-column kernels): rank and pivot positions from the well-conditioned rule (largest |a|) ...
        R, pivots, rank = dense.rref(A, bar_col=bar, pivot_rule=dense.N.PIVOT_MAX)
        if rank < m:
            # ... but with rank < m the carried-along columns depend on WHICH rows became pivot rows, so the values
            # come from the pass under the reference's rule when the two agree on the pivots
            if pivots1 == pivots:
                R = R1
            else:
                # the first-non-zero rule, run without magnitude pivoting, settled on other pivot columns than the
                # rank-revealing pass (noise in a dependent column passed its tolerance): the rank-revealing pivots and
                # values are returned, and the caller is TOLD that the carried-along columns are then not the
                # reference's (this used to pass silently)
                import warnings

                warnings.warn("row_reduce: the reference's first-non-zero pivot rule and the rank-revealing pass disagree on "
                              f"the pivot columns ({len(pivots1)} vs {len(pivots)} pivots); returning the rank-revealing "
                              "reduction -- columns right of bar_col and rows below the rank follow its row choice, not the "
                              "reference's", RuntimeWarning, stacklevel=3)
        return R, pivots

    # step descriptions of the reference's log (linalg.py:557-560, 580, 602-604, 626), verbatim: they are
    # part of what row_reduce returns
    _STEP_TEXT = (r"Výměna řádků $R_{%d}$ a $R_{%d}$", r"Normalizace pivotního řádku %s",
                  r"Eliminace prvků pod pivotem ve sloupci %s", r"Eliminace nad pivotem ve sloupci %s")
    TRACE_SNAPSHOT_BYTES = 256 << 20   # cap on the device memory spent on intermediate matrices

    def row_reduce(self, bar_col: int = None, trace=False):
        """linalg.py:534-630.  Returns (reduced_items, pivots, intermediate_matrices, intermediate_steps).

        trace=False (default): the fast paths (blocked LU / rank-revealing RREF); the two logs are empty.
        trace="steps": the reduction runs in the reference's own operation order on the device
        (lsx_rref_trace_f64): reduced_items, pivots and the (label, description) list are identical to
        the reference's, bit for bit; intermediate_matrices stays empty.
        trace=True / "full": additionally the LaTeX of the matrix after every step (first = the initial
        matrix, linalg.py:544), formatted like the reference's fmt.make_latex_augmented_matrix.  Meant
        for small inputs, like the reference's own log; beyond TRACE_SNAPSHOT_BYTES of snapshots the
        list is truncated to the first steps.
        Entry types follow the reference's object arithmetic: ints stay ints until a division or a float
        operand touches them (exact up to 2^53)."""
        A = self._array()
        n = A.shape[1]
        if n == 0:
            raise IndexError("list index out of range")  # reference fails at len(A[0]) / A[0][0]
        bar = bar_col or n - 1  # :543 -- 0 and None both mean n-1
        if trace:
            return self._row_reduce_traced(A, bar, full=(trace != "steps"))
        R, pivots = self._reduce(A, min(bar, n))
        if bar > n and len(pivots) < A.shape[0]:
            # the reference walks pivot_j past the last column here (:548) and fails the same way
            raise IndexError("list index out of range")
        return R.tolist(), pivots, [], []

    def _row_reduce_traced(self, A: np.ndarray, bar: int, full: bool):
        from . import fmt
        m, n = A.shape
        if bar > n:
            raise IndexError("list index out of range")  # the reference indexes A[pi][pj] with pj >= n (:548)
        max_steps = 4 * min(m, bar) + 4
        nsnap = min(max_steps, max(1, self.TRACE_SNAPSHOT_BYTES // (9 * m * n))) if full else 0
        # the reference computes on Python objects: int - int*int stays an int (appendix A.2); the device
        # carries that flag along with every entry
        int_in = [[isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in row] for row in self.items]
        R, pivots, recs, imask, snaps, snap_m = dense.rref_trace(A, bar, max_snapshots=nsnap, int_mask=int_in)

        def typed(values, mask):
            return [[int(values[i][j]) if mask[i][j] else float(values[i][j]) for j in range(n)] for i in range(m)]

        steps, mats = [], []
        if full:
            mats.append(fmt.make_latex_augmented_matrix(self.items, bar_col=bar))
        for k, (kind, a, b) in enumerate(recs):
            text = self._STEP_TEXT[kind] % ((a, b) if kind == 0 else (a,))
            steps.append((f"{dense.TRACE_KINDS[kind]}{k}", text))
            if full and k < len(snaps):
                mats.append(fmt.make_latex_augmented_matrix(typed(snaps[k], snap_m[k]), bar_col=bar))
        return typed(R, imask), pivots, mats, steps

    def find_preimage_of(self, vec: List[Any], log_matrices: bool = False, log_steps: bool = False,
                         log_result: bool = False, trace=False) -> "Matrix.AffineSubspace | Matrix.NoSolution":
        """All solutions of self * x = vec (linalg.py:632-680).

        The log_* flags select the reference's carrier shapes (:998 vs :888) on the fast path.  With
        trace="steps" / True the reduction runs in the reference's own operation order instead (exact
        zero tests, its float rank artefacts included) and `self.last_trace` = (matrices, steps) holds
        what the reference would have written to its LaTeX log."""
        if self.rows != len(vec):
            raise ValueError("Matrix dimensions must match")  # :642-643
        logged = log_matrices or log_steps or log_result
        A = self._array()
        b = _as_array([[v] for v in vec])
        n = A.shape[1]
        if n == 0:
            raise IndexError("list index out of range")
        aug = np.hstack([A, b])
        if trace:
            typed_aug = [list(row) + [v] for row, v in zip(self.items, vec)]   # entry types matter there
            return self._find_preimage_traced(typed_aug, n, full=(trace != "steps"))
        R, pivots = self._reduce(aug, n)
        # :913-934 with a tolerance on the right-hand side: rows below the rank have exact
        # zero coefficients; their rhs is rounding noise unless the system is inconsistent
        amax = float(np.max(np.abs(aug))) if aug.size else 0.0
        rank = len(pivots)
        xmax = float(np.max(np.abs(R[:rank, n]))) if rank else 0.0
        rhs_tol = 8.0 * dense.EPS64 * max(A.shape) * amax * (1.0 + xmax)
        if rank < A.shape[0] and np.any(np.abs(R[rank:, n]) > rhs_tol):
            return Matrix.NoSolution()
        # :937-999
        col_of_row = {r: c for r, c in pivots}
        pivot_cols = {c for _, c in pivots}
        free = [j for j in range(n) if j not in pivot_cols]
        particular: List[Any] = [0] * n
        for r, c in col_of_row.items():
            particular[c] = float(R[r, n])
        gens = []
        for fj in free:
            g: List[Any] = [0] * n
            g[fj] = 1
            for r, c in col_of_row.items():
                g[c] = -float(R[r, fj])
            gens.append(g)
        if gens:
            gen_mat = Matrix([list(col) for col in zip(*gens)])  # generators are columns (:985)
        else:
            gen_mat = None if logged else Matrix.zero(n, 0)  # :998 vs :888
        return Matrix.AffineSubspace(particular, gen_mat)

    def _find_preimage_traced(self, aug: List[List[Any]], n: int, full: bool):
        """The reference's logging path (linalg.py:655-680): reduction in its own operation order, its exact
        inconsistency test (:913-934) and extraction (:937-999).  The reference writes the step log to
        its global LaTeX logger; here it is kept on the object as `last_trace` = (matrices, steps)."""
        items, pivots, mats, steps = Matrix(aug).row_reduce(bar_col=n, trace=("full" if full else "steps"))
        self.last_trace = (mats, steps)
        for row in items:  # :918-934, exact comparisons as in the reference
            if all(v == 0 for v in row[:n]) and row[n] != 0:
                return Matrix.NoSolution()
        col_of_row = {r: c for r, c in pivots}
        pivot_cols = {c for _, c in pivots}
        particular: List[Any] = [0] * n
        for r, c in col_of_row.items():
            particular[c] = items[r][n]
        gens = []
        for fj in [j for j in range(n) if j not in pivot_cols]:
            g: List[Any] = [0] * n
            g[fj] = 1
            for r, c in col_of_row.items():
                g[c] = -items[r][fj]
            gens.append(g)
        gen_mat = Matrix([list(col) for col in zip(*gens)]) if gens else None  # :985, :998
        return Matrix.AffineSubspace(particular, gen_mat)

    def inverse(self, log_matrices: bool = False, log_steps: bool = False, log_result: bool = False, trace=False):
        """linalg.py:682-743: Matrix, or NoSolution() when singular.  trace: as in find_preimage_of."""
        if self.rows != self.cols:
            raise ValueError("Matrix must be square to invert.")  # :692-693
        A = self._array()
        n = A.shape[0]
        if trace:
            # the reference's logging path (:703-743): [A|I] reduced in its own operation order, left block
            # compared with I to 1e-12, right block returned; the log is kept as `last_trace`
            ident = Matrix.identity(n).items
            items, _piv, mats, steps = Matrix([list(self.items[i]) + ident[i] for i in range(n)]).row_reduce(
                bar_col=n, trace=("steps" if trace == "steps" else "full"))
            self.last_trace = (mats, steps)
            for i in range(n):
                for j in range(n):
                    if abs(items[i][j] - (1.0 if i == j else 0.0)) > 1e-12:
                        return Matrix.NoSolution()  # :737
            return Matrix([row[n:] for row in items])
        ka = _pow2_shift(float(np.abs(A).max(initial=0.0)))
        X, info, ratio = dense.inv(np.ldexp(A, ka))
        if info != 0 or not (ratio > dense.EPS64 * n):
            return Matrix.NoSolution()  # :701 / :737
        with np.errstate(over="ignore"):
            return Matrix(np.ldexp(X, ka).tolist())

    def determinant(self, log_permutation_details: bool = False, use_optimal: bool = True) -> Any:
        """linalg.py:183-207.  sign * prod(diag U) from the pivoted LU."""
        if self.rows != self.cols:
            raise ValueError("Determinant requires a square matrix")
        if self.rows == 1:
            return self.items[0][0]  # :200-201
        return dense.det(self._array())

    def slogdet(self, pos_def: bool = False) -> Tuple[float, float]:
        """(sign, log|det|): the overflow-free form of determinant() (new API).
        pos_def=True asserts that self is symmetric positive definite: det = prod u_ii^2 from the Cholesky factor
        (lsx_podet_*), ValueError if a leading minor is not positive definite."""
        if self.rows != self.cols:
            raise ValueError("Determinant requires a square matrix")
        if pos_def:
            s, m, e, info = dense.det_parts_pos(self._array())
            if info != 0:
                raise self._not_pos_def(info)
            return s, math.log(m) + e * math.log(2.0)
        return dense.slogdet(self._array())

    def rank(self) -> int:
        """linalg.py:745-747."""
        A = self._array()
        if A.shape[1] == 0:
            return 0
        # partial pivoting for the rank decision: the first-non-zero rule is the reference's order of
        # operations, but its unpivoted growth can lift rounding noise over the tolerance (a 5 x 7 integer
        # matrix of rank 3 came out as 4)
        from ._native import PIVOT_MAX
        return dense.rref(A, bar_col=A.shape[1], pivot_rule=PIVOT_MAX)[2]

    def kernel(self) -> "Matrix.AffineSubspace":
        """linalg.py:749-756."""
        return self.find_preimage_of([0] * self.rows)


def _fmt(v) -> str:
    if isinstance(v, (int, np.integer)):
        return str(int(v))
    f = float(v)
    if f == math.floor(f) and abs(f) < 1e15:
        return str(int(f))
    return repr(f)
