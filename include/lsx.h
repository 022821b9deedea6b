/* lsx.h -- C ABI of the MI355X-native dense LU / row-reduction library (liblsx.so)
 *
 * This is the drop-in boundary for the numeric core of koskja/linalg-solver's
 *   Matrix.row_reduce()        linalg_solver/linalg.py:534-630
 *   Matrix.find_preimage_of()  linalg_solver/linalg.py:632-680
 *   Matrix.inverse()           linalg_solver/linalg.py:682-743
 *   Matrix.determinant()       linalg_solver/linalg.py:183-207
 *   Matrix.rank()              linalg_solver/linalg.py:745-747
 * It takes the place of the reference's only native slot, the PyO3 module
 * `linalg_helper` (linalg-helper/src/lib.rs:122-143, built by
 * pyproject.toml:18-21): a shared library next to the Python package, entered
 * through plain C symbols (ctypes; see INTEGRATION.md for the binding).
 *
 * Conventions
 *   - Matrices are ROW-MAJOR (the reference stores list-of-rows), element (i,j)
 *     at base[i*ld + j]; ld >= number of columns.
 *   - Every call returns an int status: 0 = ok, <0 = bad argument / HIP error
 *     (text via lsx_last_error()).  Numerical outcomes (singular matrix, rank)
 *     are reported through out-parameters, never through the status, mirroring
 *     the reference's "results are values, not exceptions" rule
 *     (README.md:196-204, linalg.py:673,701,737).
 *   - Caller owns every buffer it passes; the library never frees or keeps them.
 *   - Host-buffer entry points copy to the device, compute there and copy back.
 *     The *_dev entry points work on device pointers already resident in HBM and
 *     are asynchronous on the handle's stream.
 *   - One handle = one GPU = one host thread at a time.  Handles are independent (every call makes the handle's device current for its duration and restores the caller's).
 *   - There is NO CPU fallback: without a usable gfx950 device lsx_create fails.
 */
#ifndef LSX_H
#define LSX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSX_VERSION 100

typedef struct lsx_handle_s *lsx_handle_t;

enum {
    LSX_OK = 0,
    LSX_ERR_ARG = -1,     /* invalid argument */
    LSX_ERR_HIP = -2,     /* a HIP runtime call failed */
    LSX_ERR_NODEVICE = -3,/* no gfx950 device / wrong architecture */
    LSX_ERR_ALLOC = -4,   /* device allocation failed */
    LSX_ERR_INTERNAL = -5 /* in-kernel protocol timeout or invariant violated */
};

/* pivot rules of lsx_rref_* */
enum { LSX_PIVOT_FIRST = 0, LSX_PIVOT_MAX = 1 };

/* input generators: counter-based, identical on host and device */
enum { LSX_FILL_INT5 = 0, LSX_FILL_U11 = 1 };

/* profiling buckets for lsx_prof_read */
enum {
    LSX_PROF_PANEL = 0,  /* panel factorisation kernels */
    LSX_PROF_LASWP = 1,  /* row interchanges outside the panel */
    LSX_PROF_TRSM = 2,   /* triangular inverse + U12 / block solves */
    LSX_PROF_GEMM = 3,   /* trailing update C -= A*B (MFMA) */
    LSX_PROF_OTHER = 4,
    LSX_PROF_GEMM_SKINNY = 5, /* the same update on 64-row tiles (few-tile shapes: the next panel's column block) */
    LSX_PROF_NBUCKETS = 6
};

/* ---- lifetime ---------------------------------------------------------- */
int lsx_device_count(void);
int lsx_create(lsx_handle_t *out, int device);
int lsx_destroy(lsx_handle_t h);
/* Enqueue on an existing hipStream_t (e.g. torch.cuda.current_stream().cuda_stream).
 * NULL is a valid value: HIP's default (null) stream, which is torch's default too. */
int lsx_set_stream(lsx_handle_t h, void *hip_stream);
/* Go back to the private non-blocking stream created by lsx_create. */
int lsx_use_own_stream(lsx_handle_t h);
int lsx_synchronize(lsx_handle_t h);
/* Thread-local text of the last failure on this thread ("" if none). */
const char *lsx_last_error(void);
/* Tunables (defaults in brackets; every variant gives bit-identical factors):
 *   "nb"            panel width, <= 128 [128]
 *   "panel"         0 = per-column launches (the fallback after an exchange time-out), 3 = one launch per panel,
 *                   device-scope pivot exchange (panels taller than one XCD holds, multi-device driver),
 *                   4 = one launch per panel on ONE XCD with the exchange in that XCD's L2 [4]
 *                   (1, 2: superseded kernels, removed; rejected with LSX_ERR_ARG)
 *   "lookahead"     0 = sequential driver, 1 = the next panel is factored on a side stream under the trailing
 *                   update [1]
 *   "lookahead_min" smallest n that takes the look-ahead driver; 0 = the measured break-even: 2048 in fp64 and
 *                   4096 in fp32 with panel = 4 (7168 / 10240 with panel = 3) [0]
 *   "kblock"        panels per trailing update [1]
 *   "trsv"          few-right-hand-side solve: 2 = 128-row steps with helper workgroups, one preparation launch [2],
 *                   1 = one cooperative launch per direction with 64-row steps, 0 = one launch per 128-row step
 *   "left_per_step" look-ahead driver: a panel's interchanges on the columns left of it trail its step [1]; 0 = all panels'
 *                   in one launch at the end
 *   "getri_pairs"   inverse / many-right-hand-side solve at large regular orders: 1 = two 128-row blocks per trailing
 *                   update (depth 256, same bits, 8192^2 inverse 17.6 -> 15.8 ms) [1], 0 = one
 *   "getrs_t_blocked_min"  transposed solve with n > 128: the smallest nrhs that takes the blocked sweeps on the MFMA
 *                   tile instead of groups of 8 columns; any value >= 1, 0 = never [64; measured break-even 32: DESIGN 3.4]
 *   "getrs_t_path"  (read only) 1 if the last lsx_getrs_t_* call on this handle took the blocked sweeps, else 0
 *   "potrs_few_max" Cholesky solve: the largest nrhs that takes the few-column step kernels instead of the block
 *                   sweeps; 0 .. 8, 0 = never [0; measurements: DESIGN 3.8]
 *   "potrs_path"    (read only) 1 if the last lsx_potrs_* call on this handle took the few-column step kernels, else 0
 *   "gemm_waves", "gemm_stagger", "panel_rt", "panel_nt", "hybrid", "xrows_limit", "rref_blocked",
 *   "getri_structured"                      tuning / cross-check switches, see DESIGN.md
 *   "panel_spin_limit", "trsv_spin_limit", "chain_wait_limit"   bounded-spin limits (tests inject time-outs)
 * Returns LSX_ERR_ARG for unknown keys or values. */
int lsx_set_option(lsx_handle_t h, const char *key, int value);
/* The cooperative kernels (panel pivot exchange, few-right-hand-side solve) poll each other with a bounded spin; a
 * time-out -- their workgroups were not all resident, e.g. another kernel held the CUs -- is recorded in a device
 * word.  The host-buffer entry points check it themselves and return LSX_ERR_INTERNAL instead of a result; after
 * *_dev calls (asynchronous, no info word required) this synchronises the handle's stream and reports it:
 * LSX_OK, or LSX_ERR_INTERNAL once (the word is cleared). */
int lsx_check_status(lsx_handle_t h);
int lsx_get_option(lsx_handle_t h, const char *key, int *value);

/* ---- host-buffer entry points (fp64) ------------------------------------ */
/* In-place LU with partial pivoting, P*A = L*U, unit-lower L below the diagonal.
 * ipiv[k] = 0-based row exchanged with row k at step k.  *info = 0, or k+1 for
 * the first k whose pivot was exactly zero (factorisation continues).
 * Numeric domain: the results are equivariant under power-of-two scaling while the intermediates are normal numbers
 * -- A diag(2^d) gives the same pivots, the same bits of L and the columns of U times 2^d, bit for bit; the solves, the
 * inverse, the determinant (exp2 moves by sum d), the condition estimate and the row reductions follow suit.
 * Subnormal pivots are handled as LAPACK's getf2 handles them: the column is divided by the pivot (here: scaled by
 * 2^64, fp32 2^32, exactly, then by the reciprocal), not multiplied by a reciprocal that is not a finite number.
 * That holds for lsx_getrf_* and for lsx_rref_* under LSX_PIVOT_MAX; the solves, the inverse and the blocked
 * first-non-zero reduction (fp64, m * bar_col >= 256 * 256) form inverses of pivot blocks and need pivots whose
 * reciprocal is a finite number. */
int lsx_getrf_f64(lsx_handle_t h, int n, double *A, int lda, int32_t *ipiv, int *info);
/* Solve A X = B from the factors; B (n x nrhs, row-major) is overwritten by X. */
int lsx_getrs_f64(lsx_handle_t h, int n, int nrhs, const double *LU, int lda,
                  const int32_t *ipiv, double *B, int ldb);
/* Factor + solve; A is not modified.  Replaces row_reduce([A|B], bar_col=n) for
 * square non-singular A (find_preimage_of, linalg.py:649-656). */
int lsx_gesv_f64(lsx_handle_t h, int n, int nrhs, const double *A, int lda,
                 double *B, int ldb, int *info, double *pivot_ratio);
/* Inverse; replaces row_reduce([A|I], bar_col=n) (inverse, linalg.py:704-711).
 * *info > 0: singular to working precision (caller returns NoSolution). */
int lsx_getri_f64(lsx_handle_t h, int n, const double *A, int lda, double *Ainv, int ldi,
                  int *info, double *pivot_ratio);
/* det(A) = sign * mant * 2^exp2 with mant in [0.5,1) (or 0): never overflows.
 * Replaces Matrix.determinant for numeric dense input (linalg.py:183-207). */
int lsx_det_f64(lsx_handle_t h, int n, const double *A, int lda, double *sign, double *mant,
                int64_t *exp2);
/* General m x n reduced row echelon form over columns [0,bar_col) with the
 * remaining columns carried along (row_reduce, linalg.py:534-630).  bar_col <= 0
 * means n-1 (linalg.py:543).  pivots holds *rank pairs (row, col), 0-based.
 * Pivot tolerance: |a| <= tol counts as zero; tol < 0 selects 32*eps*max(m,n)*max|working matrix left of bar_col|
 * (the running maximum, re-evaluated as the elimination proceeds; the carried-along columns and the finished pivot
 * rows, which are normalised, do not count).
 * pivot_rule LSX_PIVOT_FIRST takes the first row at or below the pivot row whose
 * entry is non-zero -- the reference's rule (linalg.py:548-552), which also fixes
 * the carried-along columns of rank-deficient / tall inputs; LSX_PIVOT_MAX takes
 * the largest magnitude (same pivot positions, better conditioning). */
int lsx_rref_f64(lsx_handle_t h, int m, int n, int bar_col, const double *A, int lda,
                 double *R, int ldr, int32_t *pivots, int *rank, double tol, int pivot_rule);
/* The fp32 forms of the three callers above (BASELINE config 5 computes in fp32): same meaning, fp32 MFMA tile. */
int lsx_getri_f32(lsx_handle_t h, int n, const float *A, int lda, float *Ainv, int ldi,
                  int *info, double *pivot_ratio);
int lsx_det_f32(lsx_handle_t h, int n, const float *A, int lda, double *sign, double *mant,
                int64_t *exp2);
int lsx_rref_f32(lsx_handle_t h, int m, int n, int bar_col, const float *A, int lda,
                 float *R, int ldr, int32_t *pivots, int *rank, double tol, int pivot_rule);
/* Mixed-precision solve: P A = L U in fp32, then `sweeps` (0..16, 2-3 suffice) corrections with the residual
 * b - A x accumulated in fp64 -- the forward error goes from cond(A) * eps32 to the fp32 rounding of the solution
 * of the fp64 system (config 5's "tolerance 1e-4 vs the fp64 result" is about the solution, which an unrefined fp32
 * solve of a random 8192 x 8192 system misses).  X (fp32, n x nrhs) and / or X64 (fp64) receive the solution;
 * last_correction = max|d| / max|x| of the last sweep (a convergence check: it should be ~eps32 or smaller). */
int lsx_gesv_f32_refined(lsx_handle_t h, int n, int nrhs, const float *A, int lda, const float *B, int ldb,
                         float *X, int ldx, double *X64, int ldx64, int sweeps, int *info,
                         double *pivot_ratio, double *last_correction);
/* Traced row reduction: Matrix.row_reduce in the reference's own operation order (exact-zero pivot
 * test with first-non-zero row swap, normalise, eliminate below, separate backward pass;
 * linalg.py:547-629) with one IEEE rounding per operation, so R, the pivots and the step log are
 * bit-identical to the reference's float arithmetic.  steps receives *nsteps records of 4 int32
 * {kind, a, b, 0}: kind 0 = S (rows a and b swapped, 1-based), 1 = N (pivot row a normalised),
 * 2 = E below the pivot in column a, 3 = E above the pivot in column a (linalg.py:556-606, :624-628).
 * If max_snaps > 0, snaps receives the dense m x n matrix after each of the first max_snaps steps
 * (the reference's intermediate_matrices, linalg.py:553-555 etc.).  max_steps >= 4*min(m,bar_col)
 * always suffices; LSX_ERR_ARG if the log is too small.  int_mask (m x n bytes, may be NULL = all
 * floats) says on entry which entries are Python ints and on return which still are: the reference
 * computes on Python objects, so int - int*int stays an int and only division or a float operand
 * makes a float; snap_int_mask (max_snaps x m x n bytes) is the same per
 * snapshot.  A host layer uses the masks to hand ints back.  The trace path is for small and medium inputs (several launches per column,
 * HBM-bound); the fast paths are lsx_gesv_f64 / lsx_rref_f64. */
int lsx_rref_trace_f64(lsx_handle_t h, int m, int n, int bar_col, const double *A, int lda, double *R,
                       int ldr, unsigned char *int_mask, int32_t *pivots, int *npivots, int32_t *steps,
                       int max_steps, int *nsteps, double *snaps, unsigned char *snap_int_mask,
                       int max_snaps);

/* C (m x n) = A (m x k) * B (k x n) on the MFMA tile of the trailing update.  Replaces the numeric
 * core of Matrix.__mul__ (linalg.py:101-158); used for residual checks A*x - b, A*inv(A) - I. */
int lsx_matmul_f64(lsx_handle_t h, int m, int n, int k, const double *A, int lda, const double *B, int ldb,
                   double *C, int ldc);

/* ---- host-buffer entry points (fp32; BASELINE config 5) ------------------- */
int lsx_getrf_f32(lsx_handle_t h, int n, float *A, int lda, int32_t *ipiv, int *info);
int lsx_getrs_f32(lsx_handle_t h, int n, int nrhs, const float *LU, int lda,
                  const int32_t *ipiv, float *B, int ldb);
int lsx_gesv_f32(lsx_handle_t h, int n, int nrhs, const float *A, int lda, float *B, int ldb,
                 int *info, double *pivot_ratio);

/* ---- transposed solves, norms and the condition estimate from the factors ---- */
/* matrix norms of lsx_lange_* / lsx_gecon_* / lsx_rcond_*: max absolute column sum, max absolute row sum */
enum { LSX_NORM_ONE = 0, LSX_NORM_INF = 1 };
/* Solve A^T X = B (equivalently x A = b for rows) from the factors of A: U^T Y = B, L^T Z = Y, X[perm] = Z -- no
 * second factorisation, no transposed copy of the factors.  B (n x nrhs, row-major) is overwritten by X.  Arguments
 * are validated as in lsx_getrs_*.  Two paths (n <= 128 is one workgroup either way):
 *   grouped   nrhs < "getrs_t_blocked_min" (or that option 0): right-hand sides in groups of up to 8 columns, one launch
 *             per 128-row block step and group, the block rows of the factors streamed through registers -- the path
 *             of few right-hand sides and of the single-column solves inside lsx_gecon_* and lsx_gerfs_*;
 *   blocked   nrhs >= "getrs_t_blocked_min" and n > 128: all columns at once, 128-row block sweeps whose products
 *             C -= A^T B run on the MFMA tile of the trailing update in its TN form (lsx_gemm_tn_sub_*_dev), two
 *             launches per block step whatever nrhs is; extra work space 2 n x nrhs elements.
 * The option "getrs_t_path" reads back which one the last call took.  Deterministic: two calls give identical bits on
 * either path, and on the blocked path a column gets the same bits whichever other columns are passed with it and
 * whatever lda, ldb and the alignment of the operands are.  The two paths sum in different orders: their results
 * agree to rounding, not bit for bit. */
int lsx_getrs_t_f64(lsx_handle_t h, int n, int nrhs, const double *LU, int lda, const int32_t *ipiv,
                    double *B, int ldb);
int lsx_getrs_t_f32(lsx_handle_t h, int n, int nrhs, const float *LU, int lda, const int32_t *ipiv,
                    float *B, int ldb);
/* The same on device pointers, asynchronous on the handle's stream. */
int lsx_getrs_t_f64_dev(lsx_handle_t h, int n, int nrhs, const double *dLU, int lda, const int32_t *d_ipiv,
                        double *dB, int ldb);
int lsx_getrs_t_f32_dev(lsx_handle_t h, int n, int nrhs, const float *dLU, int lda, const int32_t *d_ipiv,
                        float *dB, int ldb);
/* *d_out (device double) = max absolute column sum (LSX_NORM_ONE) or row sum (LSX_NORM_INF) of the m x n matrix at
 * dA (device pointer).  Sums are accumulated in fp64 in a fixed order (two passes, no floating-point atomics): two
 * calls give identical bits; a NaN entry gives NaN.  m == 0 or n == 0 gives 0.  Asynchronous. */
int lsx_lange_f64_dev(lsx_handle_t h, int norm, int m, int n, const double *dA, int lda, double *d_out);
int lsx_lange_f32_dev(lsx_handle_t h, int norm, int m, int n, const float *dA, int lda, double *d_out);
/* Reciprocal condition number *rcond = 1 / (anorm * est||A^-1||) in the 1- or the infinity-norm from the factors of
 * A; anorm is that norm of the UNFACTORED matrix (LAPACK's gecon contract; lsx_lange_*).  The estimate is the
 * iteration of LAPACK's lacn2 step for step: start x = 1/n, at most 5 iterations, the same stopping tests (sign
 * vector unchanged; estimate not increased; x_jlast == |x_j|), the same final test with the alternating vector, the
 * first index on ties -- 4 to 11 single-right-hand-side solves with A and A^T (for LSX_NORM_INF the two swap roles;
 * the option "gecon_solves" reads back how many the last call took).  As in gecon the solves run on L and U alone:
 * the interchanges permute the columns of the inverse and change neither norm, so ipiv is only checked for presence.
 * fp32 factors: solves in fp32, norms and the estimate accumulated in fp64.  The estimate is a LOWER bound of
 * ||A^-1||, so *rcond can exceed the true value, in practice by a small factor.
 * Numerical outcomes are values, not statuses: n == 0 gives 1; anorm == 0, an exactly zero U_ii or a non-finite
 * estimate give 0.  A NaN or negative anorm is LSX_ERR_ARG.  The host drives the iteration and reads one small record
 * per step, so ALL FOUR forms synchronise the handle's stream (the solves and the vector steps run on it); *rcond is
 * a host double in all four.  A time-out of the cooperative solve inside is LSX_ERR_INTERNAL, as from lsx_getrs_*,
 * never a condition number. */
int lsx_gecon_f64(lsx_handle_t h, int norm, int n, const double *LU, int lda, const int32_t *ipiv,
                  double anorm, double *rcond);
int lsx_gecon_f32(lsx_handle_t h, int norm, int n, const float *LU, int lda, const int32_t *ipiv,
                  double anorm, double *rcond);
int lsx_gecon_f64_dev(lsx_handle_t h, int norm, int n, const double *dLU, int lda, const int32_t *d_ipiv,
                      double anorm, double *rcond);
int lsx_gecon_f32_dev(lsx_handle_t h, int norm, int n, const float *dLU, int lda, const int32_t *d_ipiv,
                      double anorm, double *rcond);
/* One call for a host matrix: norm, factorisation, estimate; A is not modified.  *info as lsx_getrf_* (k + 1 for an
 * exactly zero pivot: then *rcond = 0). */
int lsx_rcond_f64(lsx_handle_t h, int norm, int n, const double *A, int lda, double *rcond, int *info);
int lsx_rcond_f32(lsx_handle_t h, int norm, int n, const float *A, int lda, double *rcond, int *info);

/* ---- refined solves with forward and backward error bounds (LAPACK's gerfs) ---- */
/* trans: 0 = A X = B, 1 = A^T X = B.  A is the UNFACTORED matrix, LU / ipiv its factors from lsx_getrf_*.
 * X holds a solution on entry (from lsx_getrs_* / lsx_getrs_t_*) and the refined one on return; ferr[nrhs] and
 * berr[nrhs] are host doubles in all forms (the host drives the iteration and reads one small record per step: all
 * forms synchronise the handle's stream).  No equilibration, no scaling: dgerfs.f step for step (lsx_gesvx_* equilibrates).
 *   berr[j] = max_i |r_i| / w_i with r = b - op(A) x and w = |b| + |op(A)| |x| (guarded as in dgerfs where w_i is
 *     below safe2 = (n + 1) safmin / u): the componentwise backward error of the returned column.  r and w come
 *     from ONE pass over A for up to 8 right-hand sides, accumulated in fp64 (fp32 data: converted on load, rounded
 *     once on store).
 *   A column is corrected (x += inv(op A) r, from the factors with ipiv) while berr > u, it at least halves and
 *     fewer than 5 steps were taken; a column that has stopped keeps its x.  The option "gerfs_steps" reads back the
 *     most steps any column of the last call took.
 *   ferr[j] bounds max_i |x_ij - xtrue_ij| / max_i |x_ij|: lacn2's estimate (the iteration of lsx_gecon_*) of
 *     || |inv(op A)| (|r| + (n + 1) u w) ||_inf, divided by max_i |x_ij| (undivided when that is 0).  It costs 4 to 11
 *     single-right-hand-side solves PER COLUMN, one column after the other (no estimator batched across columns);
 *     the option "gerfs_solves" reads back their number for the last call.
 * u is LAPACK's lamch('E'): 2^-53 (fp64), 2^-24 (fp32), so the results compare directly with dgesvx / sgesvx.
 * Deterministic: every sum has a fixed order, two calls give identical bits, and a column gets the same bits
 * whichever other columns are passed with it.
 * Numerical outcomes are values, not statuses: n == 0 or nrhs == 0 give ferr = berr = 0; an exactly zero or NaN U_ii
 * leaves X untouched with ferr = berr = +inf; a NaN in A, B or X gives berr = ferr = NaN for the columns it reaches
 * and no refinement step for them.  Arguments are validated as in lsx_getrs_* (lda, ldlu >= n; ldb, ldx >= nrhs;
 * trans 0 or 1; non-NULL pointers when n * nrhs > 0).  A time-out of the cooperative solve inside is
 * LSX_ERR_INTERNAL, never a bound. */
int lsx_gerfs_f64(lsx_handle_t h, int trans, int n, int nrhs, const double *A, int lda, const double *LU, int ldlu,
                  const int32_t *ipiv, const double *B, int ldb, double *X, int ldx, double *ferr, double *berr);
int lsx_gerfs_f32(lsx_handle_t h, int trans, int n, int nrhs, const float *A, int lda, const float *LU, int ldlu,
                  const int32_t *ipiv, const float *B, int ldb, float *X, int ldx, double *ferr, double *berr);
/* The same on device pointers for A, LU, ipiv, B and X; ferr / berr stay host arrays. */
int lsx_gerfs_f64_dev(lsx_handle_t h, int trans, int n, int nrhs, const double *dA, int lda, const double *dLU, int ldlu,
                      const int32_t *d_ipiv, const double *dB, int ldb, double *dX, int ldx, double *ferr, double *berr);
int lsx_gerfs_f32_dev(lsx_handle_t h, int trans, int n, int nrhs, const float *dA, int lda, const float *dLU, int ldlu,
                      const int32_t *d_ipiv, const float *dB, int ldb, float *dX, int ldx, double *ferr, double *berr);
/* One call for a host system: factor, solve, refine, bound.  A and B are not modified, X receives the solution;
 * *info as lsx_getrf_* (> 0: X is not written, ferr = berr = +inf). */
int lsx_gesvr_f64(lsx_handle_t h, int trans, int n, int nrhs, const double *A, int lda, const double *B, int ldb,
                  double *X, int ldx, double *ferr, double *berr, int *info);
int lsx_gesvr_f32(lsx_handle_t h, int trans, int n, int nrhs, const float *A, int lda, const float *B, int ldb,
                  float *X, int ldx, double *ferr, double *berr, int *info);
/* Measurement hooks (tools/kbench.py): one residual-and-bound pass for nrhs <= 8 columns, dR / dW (n x nrhs, ldr),
 * and the fp32-in / fp64-sum residual of lsx_gesv_f32_refined on its own. */
int lsx_diag_resid_bound_f64_dev(lsx_handle_t h, int trans, int n, int nrhs, const double *dA, int lda, const double *dB,
                                 int ldb, const double *dX, int ldx, double *dR, double *dW, int ldr);
int lsx_diag_resid_bound_f32_dev(lsx_handle_t h, int trans, int n, int nrhs, const float *dA, int lda, const float *dB,
                                 int ldb, const float *dX, int ldx, float *dR, float *dW, int ldr);
int lsx_diag_resid_mixed_dev(lsx_handle_t h, int n, int nrhs, const float *dA, int lda, const float *dB, int ldb,
                             const double *dX, int ldx, float *dR, int ldr);

/* ---- equilibration and the expert driver (LAPACK's geequ, laqge, gesvx) ---- */
/* Which sides of the matrix lsx_laqge_* / lsx_gesvx_* scaled: A_eq = diag(r) A diag(c) with r or c taken as 1 on a side
 * that was left alone (LAPACK's equed 'N', 'R', 'C', 'B'). */
enum { LSX_EQUED_NONE = 0, LSX_EQUED_ROW = 1, LSX_EQUED_COL = 2, LSX_EQUED_BOTH = 3 };
/* Row and column scale factors of the m x n matrix at dA (device pointer), dgeequ.f / sgeequ.f step for step in the
 * working precision: r_i = 1 / min(max(max_j |a_ij|, smlnum), bignum), c_j = 1 / min(max(max_i |a_ij| r_i, smlnum),
 * bignum) with smlnum = lamch('S'), bignum = 1 / smlnum; d_r (m entries) and d_c (n entries) are device arrays of the
 * matrix's type.  d_stats (device, 4 doubles) = {rowcnd, colcnd, amax, info}: the ratios smallest / largest r_i and
 * c_j, the largest |a_ij|, and LAPACK's info -- i (1-based) for the first exactly zero row, m + j for the first zero
 * column of the row-scaled matrix; with info != 0 the contents of d_r / d_c are unspecified and the ratios that were
 * not reached are 0.  r, c, rowcnd, colcnd and amax equal LAPACK's bit for bit (maxima, products and one IEEE division
 * per factor; nothing depends on an order of summation, on lda or on alignment).  A NaN entry gives amax = NaN.
 * m == 0 or n == 0 gives rowcnd = colcnd = 1, amax = 0, info = 0.  The matrix is streamed twice (rows, then columns),
 * each pass followed by one small launch; no atomics.  Arguments are validated like lsx_lange_*_dev.  Asynchronous. */
int lsx_geequ_f64_dev(lsx_handle_t h, int m, int n, const double *dA, int lda, double *d_r, double *d_c, double *d_stats);
int lsx_geequ_f32_dev(lsx_handle_t h, int m, int n, const float *dA, int lda, float *d_r, float *d_c, double *d_stats);
/* Measurement hook (tools/kbench.py): passes = 1 runs the row pass of lsx_geequ_* and its final step alone, 2 the column
 * pass and its (d_r and d_stats from a row pass), 3 both. */
int lsx_diag_geequ_pass_f64_dev(lsx_handle_t h, int passes, int m, int n, const double *dA, int lda, double *d_r,
                                double *d_c, double *d_stats);
int lsx_diag_geequ_pass_f32_dev(lsx_handle_t h, int passes, int m, int n, const float *dA, int lda, float *d_r,
                                float *d_c, double *d_stats);
/* dlaqge.f / slaqge.f: scale the matrix at dA in place if the factors say it is worth it.  rowcnd, colcnd, amax are HOST
 * scalars (read back from d_stats) and the decision is made on the host: with thresh = 0.1, small = lamch('S') /
 * lamch('P') and large = 1 / small, rows are scaled unless rowcnd >= thresh and small <= amax <= large, columns unless
 * colcnd >= thresh.  *equed (host int) receives LSX_EQUED_*; then ONE launch -- a_ij <- r_i a_ij, c_j a_ij or
 * (c_j r_i) a_ij, dlaqge's association, so the scaled matrix has LAPACK's bits -- or none.  Asynchronous. */
int lsx_laqge_f64_dev(lsx_handle_t h, int m, int n, double *dA, int lda, const double *d_r, const double *d_c,
                      double rowcnd, double colcnd, double amax, int *equed);
int lsx_laqge_f32_dev(lsx_handle_t h, int m, int n, float *dA, int lda, const float *d_r, const float *d_c,
                      double rowcnd, double colcnd, double amax, int *equed);
/* The expert driver, dgesvx.f step for step: equil = 0 is LAPACK's fact = 'N', 1 is fact = 'E'; trans as in
 * lsx_gerfs_*.  A and B are not modified (the contract of lsx_gesvr_*).
 *   1. equil: geequ; if its info is 0 and amax is no NaN, laqge decides and scales; otherwise *equed = LSX_EQUED_NONE.
 *   2. B is scaled by r (trans = 0, rows equilibrated) or by c (trans = 1, columns equilibrated).
 *   3. A copy of the equilibrated matrix is factored.  *info in 1..n (an exactly zero pivot): *rpvgrw is taken over
 *      the leading *info columns, *rcond = 0, ferr = berr = +inf, X is not written.
 *   4. anorm = the 1-norm (trans = 0) or the infinity-norm (trans = 1) of the equilibrated matrix (computed and read
 *      back before step 3, so that a NaN in A is seen before anything is factored).
 *   5. *rpvgrw = max |A_eq| / max |U|, the reciprocal pivot growth (1 when max |U| is 0), in the working precision.
 *   6. *rcond from lsx_gecon_*: the condition of the EQUILIBRATED matrix in that norm.
 *   7. Solve, refine and bound as lsx_gerfs_*, then X is scaled by c (trans = 0, columns equilibrated) or by r (trans = 1,
 *      rows equilibrated): X solves the system that was passed in.
 *   8. ferr is divided by colcnd (trans = 0, columns equilibrated) or by rowcnd (trans = 1, rows equilibrated).  This is
 *      LAPACK's contract and it can make the bound vacuous: on matrices whose columns span 2^-30 .. 2^30 colcnd is about
 *      1e-17 and ferr comes out as 9e3 .. 1.4e8 although the solution is accurate; berr is not affected.
 *   9. *info = n + 1 if *rcond < u (2^-53 / 2^-24): singular to working precision; X and the bounds are still returned.
 * r and c (n entries each, of the matrix's type) are written when equil = 1 and geequ's info is 0, else left untouched
 * (they are written, and nothing is scaled, when amax is NaN).
 * nrhs == 0 is valid and returns *equed, r, c, *rcond and *rpvgrw: the condition number of a badly scaled matrix.
 * n == 0: *rcond = 1, *rpvgrw = 1, *equed = LSX_EQUED_NONE.  A NaN in A (it shows in anorm; with equil = 1 also in amax):
 * nothing is factored, *equed = LSX_EQUED_NONE, *rcond = *rpvgrw = NaN, ferr = berr = NaN, every entry of X is set to NaN
 * (no output is left unwritten behind *info = 0; a caller tests *rcond for NaN), *info = 0.  This is the one input on
 * which equil = 0 does not follow lsx_gesvr_* (+inf bounds from the NaN pivot) and lsx_rcond_*.
 * A NaN in a column of B: ferr = berr = NaN for that column, as in lsx_gerfs_*.  With equil = 0 the results have the bits
 * of lsx_gesvr_* (X, ferr, berr) and of lsx_rcond_* (*rcond); so they have with equil = 1 when nothing is scaled.
 * Numerical outcomes are values, not statuses; a time-out of a cooperative solve inside is LSX_ERR_INTERNAL. */
int lsx_gesvx_f64(lsx_handle_t h, int equil, int trans, int n, int nrhs, const double *A, int lda, const double *B,
                  int ldb, double *X, int ldx, int *equed, double *r, double *c, double *rcond, double *ferr,
                  double *berr, double *rpvgrw, int *info);
int lsx_gesvx_f32(lsx_handle_t h, int equil, int trans, int n, int nrhs, const float *A, int lda, const float *B,
                  int ldb, float *X, int ldx, int *equed, float *r, float *c, double *rcond, double *ferr, double *berr,
                  double *rpvgrw, int *info);
/* The same on device pointers with LAPACK's in / out contract: dA returns the equilibrated matrix, dB the scaled
 * right-hand sides, dLU (n x n, ldlu) / d_ipiv the factors of the equilibrated matrix, dX the solution of the system as
 * passed in, d_r / d_c (required when equil = 1) geequ's factors -- so a caller can go on with lsx_getrs_*_dev /
 * lsx_gerfs_*_dev on the equilibrated system.  *equed, *rowcnd, *colcnd (may be NULL), *rcond, ferr, berr, *rpvgrw and
 * *info are host variables.  Synchronises the handle's stream, as lsx_gecon_* and lsx_gerfs_* do. */
int lsx_gesvx_f64_dev(lsx_handle_t h, int equil, int trans, int n, int nrhs, double *dA, int lda, double *dLU, int ldlu,
                      int32_t *d_ipiv, double *dB, int ldb, double *dX, int ldx, int *equed, double *d_r, double *d_c,
                      double *rowcnd, double *colcnd, double *rcond, double *ferr, double *berr, double *rpvgrw, int *info);
int lsx_gesvx_f32_dev(lsx_handle_t h, int equil, int trans, int n, int nrhs, float *dA, int lda, float *dLU, int ldlu,
                      int32_t *d_ipiv, float *dB, int ldb, float *dX, int ldx, int *equed, float *d_r, float *d_c,
                      double *rowcnd, double *colcnd, double *rcond, double *ferr, double *berr, double *rpvgrw, int *info);

/* ---- Cholesky factorisation and solves for symmetric positive definite matrices (LAPACK's potrf, potrs, posv) ---- */
/* Storage: row-major, UPPER.  On return the upper triangle of A holds U with A = U^T U and u_ii > 0.  Only the upper
 * triangle of A is read; the strictly lower triangle is never read and never written by any kernel, not inside a
 * diagonal 128-block either (LAPACK's uplo contract): it may hold anything, NaN included.  Symmetry is the caller's
 * assertion and is not checked.
 * lsx_potrf_*_dev: asynchronous on the handle's stream.  d_info is a device int and may be NULL.  *d_info = 0, or j + 1
 * (1-based) for the first j whose pivot a_jj - sum_{k<j} u_kj^2 is <= 0 or NaN (dpotf2's test).  With info = j + 1 the
 * leading j x j upper triangle is the factor of the leading j x j submatrix, as in LAPACK; the rest of the upper triangle
 * is unspecified.  Right-looking over 128-row steps on one stream: the diagonal block in one workgroup (rows in dpotf2's
 * order, the row scaled by the reciprocal of u_jj as dpotf2 does), the block row through the TN form of the MFMA tile,
 * the trailing update on the tiles on and above the diagonal only.  No launch after a failed pivot faults or spins: the
 * later diagonal launches read the info word and return, the products between them run on harmless data.  There is no
 * time-out outcome: nothing here is cooperative, no kernel waits on another workgroup, lsx_check_status has nothing to
 * report.  No look-ahead.
 * lsx_potrs_*_dev: B <- inv(U) inv(U^T) B, B n x nrhs row-major.  Any nrhs >= 1 goes through 128-row block sweeps on the
 * MFMA tile (U^T Y = B in the TN form, then U X = Y): one right-hand side costs what 128 cost.  Extra work space
 * 2 n x nrhs elements.  With the option "potrs_few_max" = m (0 .. 8, default 0) a call with 1 <= nrhs <= m takes the
 * few-column path instead: one launch per 128-row block step and direction on a dense copy of the columns, the tiles read
 * straight into registers, still nothing cooperative and no time-out outcome ("potrs_path" reads back which path the
 * last call took).  The two paths round differently; each is deterministic.
 * Host-buffer forms lsx_potrf_* / lsx_potrs_* / lsx_posv_*: copy in, compute, copy out, like lsx_gesv_*; each 128-row
 * block row is moved from its first diagonal column on (inside a diagonal block the elements below the diagonal make the
 * round trip unchanged).  lsx_posv_*: A is not modified, B is overwritten by X, *info as above (may be NULL); with
 * info > 0 B is left untouched.
 * Arguments as lsx_getrs_*: lda >= n, ldb >= nrhs; n == 0 or nrhs == 0 is LSX_OK with nothing touched; pointers must be
 * non-NULL otherwise.  Any alignment and any leading dimension: 16-byte forms where the operands allow, element-wise
 * forms otherwise, same bits.  Deterministic: two calls give identical bits.  (Nothing is promised about a column's
 * bits being independent of the columns passed with it: the backward sweep may pick kernels by nrhs.)
 * Numeric domain: the power-of-two note of lsx_getrf_* does not carry over unexamined (sqrt halves exponents: A 4^d
 * scales U by 2^d, an odd power of two does not scale it by a power of two).  What holds: the factorisation itself
 * forms the reciprocal of every u_jj, and both it and lsx_potrs_* form inverses of 128 x 128 diagonal blocks of U, so
 * every u_jj needs a reciprocal that is a finite number, as the LU solves already require of their pivots. */
int lsx_potrf_f64_dev(lsx_handle_t h, int n, double *dA, int lda, int *d_info);
int lsx_potrf_f32_dev(lsx_handle_t h, int n, float *dA, int lda, int *d_info);
int lsx_potrs_f64_dev(lsx_handle_t h, int n, int nrhs, const double *dU, int lda, double *dB, int ldb);
int lsx_potrs_f32_dev(lsx_handle_t h, int n, int nrhs, const float *dU, int lda, float *dB, int ldb);
int lsx_potrf_f64(lsx_handle_t h, int n, double *A, int lda, int *info);
int lsx_potrf_f32(lsx_handle_t h, int n, float *A, int lda, int *info);
int lsx_potrs_f64(lsx_handle_t h, int n, int nrhs, const double *U, int lda, double *B, int ldb);
int lsx_potrs_f32(lsx_handle_t h, int n, int nrhs, const float *U, int lda, float *B, int ldb);
int lsx_posv_f64(lsx_handle_t h, int n, int nrhs, const double *A, int lda, double *B, int ldb, int *info);
int lsx_posv_f32(lsx_handle_t h, int n, int nrhs, const float *A, int lda, float *B, int ldb, int *info);
/* The trailing update on its own: the upper triangle of dC (n x n) -= dA^T * dA with dA stored k x n, row-major,
 * lda >= n, ldc >= n.  The strictly lower triangle of dC is neither read nor written.  k is taken in ascending order and
 * the tiles above the diagonal take the forms lsx_gemm_tn_sub_*_dev(n, n, k, dA, lda, dA, lda, dC, ldc) gives them, so
 * every element of the upper triangle has the bits of that call.  A zero extent leaves dC untouched (pointers may then
 * be NULL); LSX_ERR_ARG for negative sizes, lda < n, ldc < n or a NULL pointer with non-zero sizes. */
int lsx_syrk_tn_sub_f64_dev(lsx_handle_t h, int n, int k, const double *dA, int lda, double *dC, int ldc);
int lsx_syrk_tn_sub_f32_dev(lsx_handle_t h, int n, int k, const float *dA, int lda, float *dC, int ldc);

/* ---- Cholesky: inverse and determinant from the factor (LAPACK's potri; trtri and lauum as its two phases) ---- */
/* Storage as above: row-major, UPPER, A = U^T U.  inv(A) = inv(U) inv(U)^T = V^T V with V = inv(U^T), lower triangular:
 * n^3/3 flops for V, n^3/3 for the product, against 4/3 n^3 for lsx_getri_* after 2/3 n^3 for lsx_getrf_*; no pivoting.
 * Nothing here is cooperative: no kernel waits on another workgroup, there is no time-out outcome and lsx_check_status
 * has nothing to report.  Deterministic: a fixed order of k in every product, no split-K, no atomics on data; two calls
 * give identical bits; any alignment and leading dimension (16-byte forms where the operands allow, element-wise forms
 * otherwise, same bits).  As for lsx_potrs_*, every u_ii needs a reciprocal that is a finite number.
 *
 * lsx_potri_*_dev: in place.  On return the upper triangle of dU holds the upper triangle of inv(A); the strictly lower
 * triangle is never read and never written, inside a diagonal 128-block either.  Asynchronous on the handle's stream.
 * d_info is a device int and may be NULL: 0, or i + 1 (1-based) for the first u_ii that is exactly zero or NaN (dtrtri's
 * test); the upper triangle is then unspecified and may hold inf or NaN, and no launch faults or waits.  Work space: V,
 * n x ceil16(n) elements, the block inverses of lsx_potrs_* and one 128-row strip, all on the handle.  Arguments as
 * lsx_potrf_*_dev: lda >= n; n == 0 is LSX_OK with nothing touched; dU non-NULL otherwise.
 * lsx_potri_*: the host-buffer form; the upper triangle is staged both ways as in lsx_potrf_* (each 128-row block row from
 * its first diagonal column on), *info (may be NULL) as d_info.
 * lsx_poinv_*: factor, invert and mirror a host matrix in one call.  A is not modified (only its upper triangle is read);
 * Ainv (n x n, ldi >= n) receives the FULL inverse, both triangles, exactly symmetric.  *info as lsx_potrf_* (may be
 * NULL); with info > 0 Ainv is not written.
 *
 * lsx_trtri_upper_t_*_dev: the first phase on its own, dV = inv(dU^T).  Written: row i of dV in the columns
 * [0, 128 (i / 128 + 1)), cut at n -- the blocks on and below the diagonal 128-blocks; inside a diagonal block the
 * entries above the diagonal are exact zeros.  The blocks of dV strictly above the diagonal blocks are never written and
 * never read.  Of dU the upper triangle alone is read.  dU and dV must not overlap.  Forward substitution over 128-row
 * steps on the TN form of the MFMA tile, block row kb on its columns [0, kb + jb) only.
 * lsx_lauum_tn_*_dev: the second phase on its own, the upper triangle of dC (n x n) = dV^T * dV for a lower-triangular dV
 * (n x n, row-major, ldv >= n, ldc >= n).  For col >= row the sum runs over k >= col only, so the tile (I, J) of 128 x 128
 * takes k from 128 J on: the blocks of dV strictly above its diagonal 128-blocks are never read (they may hold NaN);
 * inside a diagonal block the entries above the diagonal are read and must be the zeros of a lower-triangular matrix.
 * The strictly lower triangle of dC is neither read nor written; dC is not read at all.  By default k is taken in
 * ascending order, so every element of the upper triangle has the bits that lsx_gemm_tn_add_*_dev(n, n, n, V0, ldv, V0, ldv, Z, ldc) gives
 * it for V0 = dV with zeros above the diagonal and Z = 0: the skipped terms are products with exact zeros added to a
 * zero accumulator.  One launch when n is a multiple of 128 and the operands are 16-byte aligned with leading dimensions
 * that are multiples of 16 bytes.  The option "potri_order" (0, default: tiles handed out deepest first, by ascending
 * tile column; 1: the order of lsx_syrk_tn_sub_*_dev) picks the tile order of this product here and in lsx_potri_* --
 * same bits either way -- and "potri_tiles" reads back how many tiles the last such product ran: t (t + 1) / 2 with
 * t = ceil(n / 128).  A zero n leaves dC untouched (pointers may then be NULL); LSX_ERR_ARG for a negative n, ldv < n,
 * ldc < n or a NULL pointer with n > 0.
 * Order of summation.  lsx_potri_* runs this product with every tile's k-slabs of 16 taken from the LAST one down to the
 * first (k ascending inside a slab; a partial last slab comes first); the option "lauum_descending" = 1 (default 0) makes
 * lsx_lauum_tn_*_dev do the same, so that lsx_potri_*_dev has the bits of lsx_trtri_upper_t_*_dev followed by
 * lsx_lauum_tn_*_dev under that option.  Why: the term k = col of the sum carries v[col][col], which dominates when V is
 * diagonally dominant; met first, every later addition is rounded at the size of the whole sum (measured: LAPACK's test
 * ratio of the inverse 4 to 6 times that of LAPACK's potri on G G^T / n + I); met after the tail, 1.5 to 1.6 times.  The
 * two orders cost the same time.  The ascending default of the stand-alone entry point keeps its bits comparable with
 * lsx_gemm_tn_add_*_dev.
 * lsx_symmetrize_upper_*_dev: a_ji = a_ij for every j > i -- the only entry point of this family that writes below the
 * diagonal.  A tiled transpose-copy through LDS; the diagonal and the upper triangle are not written.
 *
 * lsx_podet_*_dev: det(A) = prod u_ii^2 from the factor: d_out = {sign, mant, (double)exp2} in the format of
 * lsx_det_*_dev, det = sign * mant * 2^exp2 with mant in [0.5, 1).  sign is 1, or 0 with mant = exp2 = 0 when some u_ii
 * is exactly zero.  n == 0 gives {1, 0.5, 1}.  Asynchronous.
 * lsx_podet_*: factors a copy of a host matrix and returns its determinant; *info as lsx_potrf_* (may be NULL); with
 * info > 0 the three outputs are 0. */
int lsx_potri_f64_dev(lsx_handle_t h, int n, double *dU, int lda, int *d_info);
int lsx_potri_f32_dev(lsx_handle_t h, int n, float *dU, int lda, int *d_info);
int lsx_potri_f64(lsx_handle_t h, int n, double *U, int lda, int *info);
int lsx_potri_f32(lsx_handle_t h, int n, float *U, int lda, int *info);
int lsx_poinv_f64(lsx_handle_t h, int n, const double *A, int lda, double *Ainv, int ldi, int *info);
int lsx_poinv_f32(lsx_handle_t h, int n, const float *A, int lda, float *Ainv, int ldi, int *info);
int lsx_trtri_upper_t_f64_dev(lsx_handle_t h, int n, const double *dU, int lda, double *dV, int ldv);
int lsx_trtri_upper_t_f32_dev(lsx_handle_t h, int n, const float *dU, int lda, float *dV, int ldv);
int lsx_lauum_tn_f64_dev(lsx_handle_t h, int n, const double *dV, int ldv, double *dC, int ldc);
int lsx_lauum_tn_f32_dev(lsx_handle_t h, int n, const float *dV, int ldv, float *dC, int ldc);
int lsx_symmetrize_upper_f64_dev(lsx_handle_t h, int n, double *dA, int lda);
int lsx_symmetrize_upper_f32_dev(lsx_handle_t h, int n, float *dA, int lda);
int lsx_podet_f64_dev(lsx_handle_t h, int n, const double *dU, int lda, double *d_out);
int lsx_podet_f32_dev(lsx_handle_t h, int n, const float *dU, int lda, double *d_out);
int lsx_podet_f64(lsx_handle_t h, int n, const double *A, int lda, double *sign, double *mant, int64_t *exp2, int *info);
int lsx_podet_f32(lsx_handle_t h, int n, const float *A, int lda, double *sign, double *mant, int64_t *exp2, int *info);

/* ---- Householder QR and least squares (LAPACK's geqrf, ormqr, orgqr, gels) ---- */
/* Row-major like everything else: element (i, j) at base[i * ld + j].  Nothing here is cooperative: no kernel waits
 * for another workgroup, there is no spin and no time-out outcome, lsx_check_status has nothing to report.  Everything
 * runs on the handle's stream; the _dev forms are asynchronous, the host-buffer forms copy in, compute, copy out and
 * synchronise.  Any alignment and any leading dimension work and give the same bits; two calls give identical bits.
 *
 * lsx_geqrf_*_dev: A (m x n, any m, n >= 0) = Q R with k = min(m, n) reflectors.  On return R lies on and above the
 * diagonal; reflector j lies below the diagonal of column j with v_jj = 1 implied (LAPACK's layout); d_tau holds k
 * entries of the matrix's type, H_j = I - tau_j v_j v_j^T, A = H_0 .. H_{k-1} R.
 * Arithmetic of reflector j, with g_c = sum_{i > j} a_ij a_ic over the rows below it (c = j .. the panel's last column):
 *     alpha = a_jj,  xnorm^2 = g_j.   g_j == 0: tau_j = 0 and nothing changes (dlarfg).   Otherwise
 *     beta = -copysign(sqrt(alpha^2 + g_j), alpha),  tau = (beta - alpha) / beta,  s = 1 / (alpha - beta),
 *     v_i = s a_ij,  w_c = a_jc + s g_c,  a_jc -= tau w_c,  a_ic -= tau v_i w_c,  a_jj = beta.
 * The sums, their reduction and the scalars are fp64 for both precisions; every stored element is rounded to the
 * matrix's type once.  Columns right of a 128-column panel receive the block reflector I - V T V^T (T as dlarft forms
 * it, from V^T V) through the MFMA tiles.
 * Numeric domain: dlarfg's rescaling loop is not reproduced, so alpha^2 + g_j must be a finite normal number (entries
 * between about 1e-150 and 1e150 in fp64: the sums are fp64 for fp32 matrices too, whose whole range is therefore
 * served).  A NaN propagates to what it reaches; nothing faults or loops on it.
 *
 * lsx_ormqr_*_dev: C (m x ncols) <- Q^T C (trans = 1) or Q C (trans = 0), left side only, Q = H_0 .. H_{k-1} from the
 * first k columns of a factored array (lda >= k) and d_tau.  V and T are formed again per 128-reflector block.
 * lsx_orgqr_*_dev: the thin Q (m x n, k <= n <= m), out of place: Q applied to the leading columns of the identity.
 * lsx_gels_*_dev: min ||b - A x||_2 for m >= n (m < n is LSX_ERR_ARG: minimum-norm solutions need LQ).  dA is
 * overwritten by its QR, d_tau (n entries) by the scalars; dB (m x nrhs) is overwritten: rows [0, n) become the
 * solution, rows [n, m) the tail of Q^T B, whose column norms are the residual norms (dgels's contract).  *d_info (may
 * be NULL) is 0, or i + 1 for the first r_ii that is exactly zero or NaN; the solution rows are then unspecified.  The
 * solve with R never loads what lies below the diagonal.
 * lsx_colnrm2_*_dev: d_out[c] = the 2-norm of column c of A (m x n), n device doubles.  The squares are summed in fp64
 * in a fixed order, without atomics and without scaling: their sum must not overflow.
 *
 * Host forms: lsx_geqrf_*, lsx_ormqr_*, lsx_orgqr_* as above on host buffers.  lsx_gels_*: A (m x n) and B (m x nrhs)
 * are not modified; X is n x nrhs; resid (host double[nrhs], may be NULL) receives ||b - A x||_2 per column; *info (may
 * be NULL) as above, and with info > 0 X is not written and resid is +inf.
 *
 * LSX_ERR_ARG for negative sizes, lda < n (lda < k where only k columns are read), ldc < ncols, ldq < n, ldb or ldx <
 * nrhs, k out of range (k > m; for orgqr k > n or n > m), trans other than 0 or 1, or a NULL pointer with non-zero
 * sizes.  Zero extents are LSX_OK with nothing touched. */
int lsx_geqrf_f64_dev(lsx_handle_t h, int m, int n, double *dA, int lda, double *d_tau);
int lsx_geqrf_f32_dev(lsx_handle_t h, int m, int n, float *dA, int lda, float *d_tau);
int lsx_ormqr_f64_dev(lsx_handle_t h, int trans, int m, int ncols, int k, const double *dQR, int lda, const double *d_tau,
                      double *dC, int ldc);
int lsx_ormqr_f32_dev(lsx_handle_t h, int trans, int m, int ncols, int k, const float *dQR, int lda, const float *d_tau,
                      float *dC, int ldc);
int lsx_orgqr_f64_dev(lsx_handle_t h, int m, int n, int k, const double *dQR, int lda, const double *d_tau, double *dQ,
                      int ldq);
int lsx_orgqr_f32_dev(lsx_handle_t h, int m, int n, int k, const float *dQR, int lda, const float *d_tau, float *dQ,
                      int ldq);
int lsx_gels_f64_dev(lsx_handle_t h, int m, int n, int nrhs, double *dA, int lda, double *d_tau, double *dB, int ldb,
                     int *d_info);
int lsx_gels_f32_dev(lsx_handle_t h, int m, int n, int nrhs, float *dA, int lda, float *d_tau, float *dB, int ldb,
                     int *d_info);
int lsx_colnrm2_f64_dev(lsx_handle_t h, int m, int n, const double *dA, int lda, double *d_out);
int lsx_colnrm2_f32_dev(lsx_handle_t h, int m, int n, const float *dA, int lda, double *d_out);
int lsx_geqrf_f64(lsx_handle_t h, int m, int n, double *A, int lda, double *tau);
int lsx_geqrf_f32(lsx_handle_t h, int m, int n, float *A, int lda, float *tau);
int lsx_ormqr_f64(lsx_handle_t h, int trans, int m, int ncols, int k, const double *QR, int lda, const double *tau, double *C,
                  int ldc);
int lsx_ormqr_f32(lsx_handle_t h, int trans, int m, int ncols, int k, const float *QR, int lda, const float *tau, float *C,
                  int ldc);
int lsx_orgqr_f64(lsx_handle_t h, int m, int n, int k, const double *QR, int lda, const double *tau, double *Q, int ldq);
int lsx_orgqr_f32(lsx_handle_t h, int m, int n, int k, const float *QR, int lda, const float *tau, float *Q, int ldq);
int lsx_gels_f64(lsx_handle_t h, int m, int n, int nrhs, const double *A, int lda, const double *B, int ldb, double *X, int ldx,
                 double *resid, int *info);
int lsx_gels_f32(lsx_handle_t h, int m, int n, int nrhs, const float *A, int lda, const float *B, int ldb, float *X, int ldx,
                 double *resid, int *info);

/* ---- Jacobi SVD and minimum-norm least squares (LAPACK's gesvj / gesvdj, gelss) ---- */
/* A (m x n, row-major, any m, n >= 0) = U diag(s) V^T with k = min(m, n): s holds k DOUBLES for both precisions, in
 * descending order; with jobz = 1 U is m x k and Vt is k x n (the thin factors), with jobz = 0 only s is computed (no
 * rotations are accumulated, no ormqr; U and Vt may be NULL) and s has the bits jobz = 1 gives.  Nothing here is
 * cooperative: no kernel waits for another workgroup, there is no spin and no time-out outcome, lsx_check_status has
 * nothing to report.  With a fixed pair order the result is deterministic: two calls give identical bits, and so do any
 * alignment and any leading dimension of the caller's arrays (they are only copied from and gathered into).
 *
 * Algorithm: one-sided Jacobi on the ROWS of a work matrix W (p x q).  m <= n: W = A (p = m, q = n) and U = Z^T, Z the
 * product of the rotations.  m > n: A = Q R by lsx_geqrf_*, W = R (p = q = n) and U = Q [Z^T; 0] by lsx_ormqr_*.  A sweep
 * pairs every row with every other once, in P - 1 rounds of the round-robin order over P = p + (p & 1) players (round r:
 * position 0 holds player 0, position s >= 1 player ((s - 1 - r) mod (P - 1)) + 1; position t meets position P - 1 - t;
 * a pair with the phantom player of an odd p is skipped); the pairs of a round share no row, a round is one launch.
 * Pair (i < j): a = w_i.w_i, b = w_j.w_j, c = w_i.w_j in fp64 for both precisions, in a fixed order; rotate iff
 * |c| > tol sqrt(a) sqrt(b), tol = sqrt(q) u, u = 2^-53 (fp64) or 2^-24 (fp32) -- dgesvj's CTOL; a NaN fails the
 * comparison.  zeta = (b - a) / (2 c), t = sgn(zeta) / (|zeta| + sqrt(1 + zeta^2)) with sgn(0) = +1 (|zeta| > 2^500:
 * t = 1 / (2 zeta)), cs = 1 / sqrt(1 + t^2), sn = cs t, w_i <- cs w_i - sn w_j, w_j <- sn w_i + cs w_j in fp64, rounded
 * once; rows i, j of Z alike.  A sweep without a rotation ends the iteration; at most "gesvdj_max_sweeps" sweeps run
 * (option, 1 .. 60, default 30 = dgesvj's NSWEEP).  If the last allowed sweep still rotated *info = 1 and the results are
 * returned all the same (dgesvj's INFO > 0); otherwise *info = 0.  The options "gesvdj_sweeps" and "gesvdj_rotations"
 * (saturating at INT_MAX) read back the last call.  Then s_i = sqrt(sum_k w_ik^2) in fp64, sorted descending (stable),
 * and row i of Vt = w_i / s_i.
 * Deviation from LAPACK's layout: U is orthonormal to rounding for EVERY input, and the rows of Vt that belong to an
 * exactly zero singular value are rows of zeros (LAPACK completes them to an orthonormal set).
 * Numeric domain: the sums of squares are not scaled, so sum_k w_ik^2 must be a finite normal fp64 number -- the
 * contract of lsx_colnrm2_*.  Inside it A 2^d gives the same U, Vt, sweeps and rotations, and s 2^d.
 * A NaN or an infinity anywhere in A: every entry of s is NaN, U and Vt are unspecified, *info = 0; nothing iterates
 * ("gesvdj_sweeps" reads 0), loops or faults.
 * The host reads one counter per sweep, so ALL forms synchronise the handle's stream (as lsx_gecon_*, lsx_gerfs_*).
 * info and rank are host ints in all forms (info may be NULL).  The _dev forms destroy dA; d_s is a device array there.
 *
 * lsx_gelss_*: the minimum-norm solution of min ||b - A x||_2 for ANY shape and rank: X (n x nrhs) = V diag(1 / s_i,
 * i < rank) U^T B, the two products on the MFMA tile.  *rank (may be NULL) = the number of s_i > rcond s_0; rcond < 0
 * selects max(m, n) u.  s_0 == 0 gives rank 0 and X = 0.  d_s / s (k doubles) may be NULL.  A NaN or infinity in A gives
 * rank 0, s and X all NaN.  The host form leaves A and B alone; resid (host double[nrhs], may be NULL) receives
 * ||b - A x||_2 per column, from B - A X on the update tile and lsx_colnrm2_*.  dB is not modified.
 *
 * LSX_ERR_ARG for negative sizes, lda < n, jobz other than 0 or 1, with jobz = 1 ldu < k or ldvt < n, ldb or ldx < nrhs,
 * or a NULL pointer with non-zero sizes.  Zero extents (k == 0; for gelss also nrhs == 0) are LSX_OK with nothing
 * touched but *info = 0 and *rank = 0. */
int lsx_gesvdj_f64_dev(lsx_handle_t h, int jobz, int m, int n, double *dA, int lda, double *d_s, double *dU, int ldu,
                       double *dVt, int ldvt, int *info);
int lsx_gesvdj_f32_dev(lsx_handle_t h, int jobz, int m, int n, float *dA, int lda, double *d_s, float *dU, int ldu,
                       float *dVt, int ldvt, int *info);
int lsx_gesvdj_f64(lsx_handle_t h, int jobz, int m, int n, const double *A, int lda, double *s, double *U, int ldu,
                   double *Vt, int ldvt, int *info);
int lsx_gesvdj_f32(lsx_handle_t h, int jobz, int m, int n, const float *A, int lda, double *s, float *U, int ldu, float *Vt,
                   int ldvt, int *info);
int lsx_gelss_f64_dev(lsx_handle_t h, int m, int n, int nrhs, double *dA, int lda, const double *dB, int ldb, double *dX,
                      int ldx, double rcond, double *d_s, int *rank, int *info);
int lsx_gelss_f32_dev(lsx_handle_t h, int m, int n, int nrhs, float *dA, int lda, const float *dB, int ldb, float *dX,
                      int ldx, double rcond, double *d_s, int *rank, int *info);
int lsx_gelss_f64(lsx_handle_t h, int m, int n, int nrhs, const double *A, int lda, const double *B, int ldb, double *X,
                  int ldx, double rcond, double *s, double *resid, int *rank, int *info);
int lsx_gelss_f32(lsx_handle_t h, int m, int n, int nrhs, const float *A, int lda, const float *B, int ldb, float *X,
                  int ldx, double rcond, double *s, double *resid, int *rank, int *info);

/* ---- Symmetric eigensolver by two-sided Jacobi (the vendor libraries' syevj) ---- */
/* A (n x n, symmetric, row-major, UPPER) = V diag(w) V^T.  Only the upper triangle of A is read: the strictly lower
 * triangle may hold anything, NaN included, and no kernel loads it.  w holds n DOUBLES for both precisions, ASCENDING
 * (LAPACK's syev order, a stable sort of the diagonal).  With jobz = 1 V is n x n and column i is the eigenvector of
 * w[i]; with jobz = 0 V may be NULL, no rotations are accumulated and w has the bits jobz = 1 gives.  Nothing here is
 * cooperative: no kernel waits for another workgroup, there is no spin and no time-out outcome, lsx_check_status has
 * nothing to report.  The call is deterministic: two calls give identical bits, and so do any alignment and any leading
 * dimension of the caller's arrays (they are only copied from and gathered into).
 * The host form leaves A alone.  The _dev form must be taken to destroy dA: what it holds afterwards is unspecified.
 * (The present kernels only read its upper triangle and leave every element as it was.)
 *
 * Algorithm.  The work matrix W (n x n, both triangles) is built from the upper triangle of A and mirrored; with
 * jobz = 1 Z = I.  nrm = ||A||_F from the upper triangle, the off-diagonal squares counted twice, summed in fp64 in a
 * fixed order without atomics and without scaling (the numeric domain of lsx_colnrm2_*: nrm^2 a finite normal fp64
 * number).  thr = u nrm, u = 2^-53 (fp64) or 2^-24 (fp32).  A sweep is the P - 1 rounds of the round-robin order of
 * lsx_gesvdj_* over P = n + (n & 1) players.  All decisions of a round are taken from W as it stands before the round:
 * pair (i < j), a = w_ii, b = w_jj, c = w_ij (the UPPER element) in fp64; rotate iff |c| > thr (a NaN fails the
 * comparison); zeta = (b - a) / (2 c), t = sgn(zeta) / (|zeta| + sqrt(1 + zeta^2)) with sgn(0) = +1 (|zeta| > 2^500:
 * t = 1 / (2 zeta)), cs = 1 / sqrt(1 + t^2), sn = cs t.  Then W <- G W G^T over all rotated pairs of the round: rows
 * i, j: x' = cs x - sn y, y' = sn x + cs y in fp64, each element rounded to the matrix's type once; the same on columns
 * i, j of every row of the row-rotated matrix, rounded once again; w_ij = w_ji = 0 exactly; rows i, j of Z like the rows
 * of W.  Rows and columns of pairs that are not rotated keep their bits.  The two triangles are computed in different
 * orders and may drift apart at rounding level; decisions read the upper element only, the eigenvalues are the diagonal.
 * A sweep without a rotation ends the iteration; at most "syevj_max_sweeps" sweeps run (option, 1 .. 100, default 60).
 * If the last allowed sweep still rotated *info = 1 and the results are returned all the same; otherwise *info = 0.  The
 * options "syevj_sweeps" and "syevj_rotations" (saturating at INT_MAX) read back the last call.  Then
 * w_i = (double) w_ii, sorted ascending (stable), and V[:, i] is the row of Z that belongs to it.
 * Inside the numeric domain A 2^d gives the same V, sweeps and rotations, and w 2^d.
 * A NaN or an infinity in the upper triangle of A: every entry of w is NaN, V is unspecified, *info = 0; nothing
 * iterates ("syevj_sweeps" reads 0), loops or faults.
 * The host reads one counter per sweep, so ALL forms synchronise the handle's stream.  info is a host int in all forms
 * and may be NULL; d_w is a device array in the _dev forms.
 * This is the unblocked method: a round streams W and Z once and takes two launches, so it is bandwidth- and
 * launch-bound and meant for orders up to a few thousand.
 *
 * LSX_ERR_ARG for n < 0, lda < n, jobz other than 0 or 1, ldv < n with jobz = 1, or a NULL pointer with n > 0.
 * n == 0 is LSX_OK with *info = 0 and nothing else touched. */
int lsx_syevj_f64_dev(lsx_handle_t h, int jobz, int n, double *dA, int lda, double *d_w, double *dV, int ldv, int *info);
int lsx_syevj_f32_dev(lsx_handle_t h, int jobz, int n, float *dA, int lda, double *d_w, float *dV, int ldv, int *info);
int lsx_syevj_f64(lsx_handle_t h, int jobz, int n, const double *A, int lda, double *w, double *V, int ldv, int *info);
int lsx_syevj_f32(lsx_handle_t h, int jobz, int n, const float *A, int lda, double *w, float *V, int ldv, int *info);

/* ---- Cholesky: condition estimate and error bounds (LAPACK's lansy, pocon, porfs) ---- */
/* Storage as above: row-major, UPPER, A = U^T U.  The strictly lower triangle of A and of U is never loaded and never
 * written by any of these, inside a diagonal tile or block included: it may hold NaN.  Nothing here is cooperative: no
 * kernel waits for another workgroup, there is no time-out outcome and lsx_check_status has nothing to report.
 * Deterministic: every sum has a fixed order, there are no floating-point atomics, two calls give identical bits; any
 * alignment and leading dimension (16-byte loads where the operands allow, element-wise loads otherwise, same bits).
 *
 * lsx_lansy_*_dev: *d_out (a device double) = the 1-norm, which equals the infinity-norm, of the symmetric n x n matrix
 * given by its upper triangle.  Contract of lsx_lange_*_dev: sums in fp64 in a fixed order, a NaN in the upper triangle
 * gives NaN, n == 0 gives 0 (dA may then be NULL).  Asynchronous on the handle's stream.  LSX_ERR_ARG for n < 0,
 * lda < n, a NULL d_out, or a NULL dA with n > 0.
 *
 * lsx_pocon_*: LAPACK's pocon, step for step: *rcond = (1 / est) / anorm, est = lacn2's estimate of the 1-norm of
 * inv(A) from 4 .. 11 single-right-hand-side solves x <- inv(U) inv(U^T) x (1 for n == 1; the option "pocon_solves"
 * reads back how many the last call took).  anorm: the 1-norm of the unfactored matrix (lsx_lansy_*_dev).  Outcomes, as
 * values like lsx_gecon_*: n == 0 gives 1; anorm == 0, an exactly zero or NaN u_ii, or an estimate that is not a finite
 * number give 0; a NaN or negative anorm is LSX_ERR_ARG.  The host form stages the upper triangle of U; the _dev form
 * takes a device factor; both synchronise the handle's stream.
 * lsx_porcond_*: norm, factorisation and estimate of a host matrix in one call; A is not modified.  *info as
 * lsx_potrf_* (may be NULL); with info > 0 *rcond = 0.
 *
 * lsx_porfs_*: LAPACK's porfs, step for step, on the caller's factor: the loop of lsx_gerfs_* (the same code) with the
 * residual r = b - A x and the bound |b| + |A| |x| formed from the upper triangle of A alone (every stored a_ij, j > i,
 * loaded once and used for rows i and j; sums in fp64, rounded once) and corrections by single-right-hand-side solves
 * with U^T and U.  ITMAX = 5, the same stopping rule, safe1 / safe2 guards and per-column lacn2 bound:
 *   berr[j] = max_i |r_i| / (|b| + |A| |x|)_i of column j of the returned X,
 *   ferr[j] >= an estimate of max_i |x_i - xtrue_i| / max_i |x_i|.
 * X holds a solution on entry (lsx_potrs_*) and the refined one on return; A, U and B are not modified.  A column's bits
 * do not depend on the columns passed with it.  Outcomes as lsx_gerfs_*: n == 0 or nrhs == 0 gives zeros and touches
 * nothing; an exactly zero or NaN u_ii leaves X untouched with ferr = berr = +inf; a NaN in the upper triangle of A, in
 * B or in X gives NaN bounds for the columns it reaches and no step for them.  The options "porfs_steps" (most steps
 * any column took) and "porfs_solves" (estimator solves, 4 .. 11 per column for n > 1) read back the last call.
 * ferr, berr: host double[nrhs] in all forms.  Synchronises the handle's stream.  LSX_ERR_ARG for negative sizes,
 * lda < n, ldu < n, ldb < nrhs, ldx < nrhs, or a NULL pointer with non-zero sizes.
 * lsx_posvr_*: potrf + potrs + porfs for a host system; A and B are kept, X receives the refined solution.  *info as
 * lsx_potrf_* (may be NULL); with info > 0 X is not written and the bounds are +inf.
 *
 * lsx_diag_resid_bound_sym_*_dev (measurement / test hook): dR = dB - A dX and dW = |dB| + |A| |dX| for nrhs <= 8
 * columns in one pass over the upper triangle of dA, as porfs forms them; ldr: the leading dimension of dR and dW.
 * nrhs > 8 is LSX_ERR_ARG.  Asynchronous. */
int lsx_lansy_f64_dev(lsx_handle_t h, int n, const double *dA, int lda, double *d_out);
int lsx_lansy_f32_dev(lsx_handle_t h, int n, const float *dA, int lda, double *d_out);
int lsx_pocon_f64(lsx_handle_t h, int n, const double *U, int lda, double anorm, double *rcond);
int lsx_pocon_f32(lsx_handle_t h, int n, const float *U, int lda, double anorm, double *rcond);
int lsx_pocon_f64_dev(lsx_handle_t h, int n, const double *dU, int lda, double anorm, double *rcond);
int lsx_pocon_f32_dev(lsx_handle_t h, int n, const float *dU, int lda, double anorm, double *rcond);
int lsx_porcond_f64(lsx_handle_t h, int n, const double *A, int lda, double *rcond, int *info);
int lsx_porcond_f32(lsx_handle_t h, int n, const float *A, int lda, double *rcond, int *info);
int lsx_porfs_f64(lsx_handle_t h, int n, int nrhs, const double *A, int lda, const double *U, int ldu, const double *B,
                  int ldb, double *X, int ldx, double *ferr, double *berr);
int lsx_porfs_f32(lsx_handle_t h, int n, int nrhs, const float *A, int lda, const float *U, int ldu, const float *B,
                  int ldb, float *X, int ldx, double *ferr, double *berr);
int lsx_porfs_f64_dev(lsx_handle_t h, int n, int nrhs, const double *dA, int lda, const double *dU, int ldu,
                      const double *dB, int ldb, double *dX, int ldx, double *ferr, double *berr);
int lsx_porfs_f32_dev(lsx_handle_t h, int n, int nrhs, const float *dA, int lda, const float *dU, int ldu,
                      const float *dB, int ldb, float *dX, int ldx, double *ferr, double *berr);
int lsx_posvr_f64(lsx_handle_t h, int n, int nrhs, const double *A, int lda, const double *B, int ldb, double *X, int ldx,
                  double *ferr, double *berr, int *info);
int lsx_posvr_f32(lsx_handle_t h, int n, int nrhs, const float *A, int lda, const float *B, int ldb, float *X, int ldx,
                  double *ferr, double *berr, int *info);
int lsx_diag_resid_bound_sym_f64_dev(lsx_handle_t h, int n, int nrhs, const double *dA, int lda, const double *dB, int ldb,
                                     const double *dX, int ldx, double *dR, double *dW, int ldr);
int lsx_diag_resid_bound_sym_f32_dev(lsx_handle_t h, int n, int nrhs, const float *dA, int lda, const float *dB, int ldb,
                                     const float *dX, int ldx, float *dR, float *dW, int ldr);

/* ---- device-pointer entry points (asynchronous on the handle's stream) ---- */
/* d_info: device int (may be NULL).  d_ipiv: device int32[n].
 * *d_info < 0 after the call means the in-kernel pivot exchange timed out (LSX_ERR_INTERNAL
 * in the host-buffer forms): the factors are not valid. */
int lsx_getrf_f64_dev(lsx_handle_t h, int n, double *dA, int lda, int32_t *d_ipiv, int *d_info);
int lsx_getrs_f64_dev(lsx_handle_t h, int n, int nrhs, const double *dLU, int lda,
                      const int32_t *d_ipiv, double *dB, int ldb);
int lsx_getri_f64_dev(lsx_handle_t h, int n, const double *dLU, int lda, const int32_t *d_ipiv,
                      double *dInv, int ldi);
/* d_out[0]=sign, d_out[1]=mant, d_out[2]=(double)exp2 */
/* fp32 forms of the two above, and the device-pointer mixed-precision solve: dA / dB are read, dLU receives the fp32
 * factors, dX64 (n x nrhs fp64) the solution, dX32 (may be NULL) its fp32 rounding, d_stats (4 doubles, may be
 * NULL) = max|d|, max|x| of the last sweep, then of the initial solve. */
int lsx_getri_f32_dev(lsx_handle_t h, int n, const float *dLU, int lda, const int32_t *d_ipiv,
                      float *dInv, int ldi);
int lsx_det_f32_dev(lsx_handle_t h, int n, const float *dLU, int lda, const int32_t *d_ipiv, double *d_out);
int lsx_gesv_f32_refined_dev(lsx_handle_t h, int n, int nrhs, const float *dA, int lda, float *dLU, int ldl,
                             int32_t *d_ipiv, int *d_info, const float *dB, int ldb, double *dX64, int ldx,
                             float *dX32, int ldf, int sweeps, double *d_stats);
int lsx_det_f64_dev(lsx_handle_t h, int n, const double *dLU, int lda, const int32_t *d_ipiv,
                    double *d_out);
int lsx_getrf_f32_dev(lsx_handle_t h, int n, float *dA, int lda, int32_t *d_ipiv, int *d_info);
int lsx_getrs_f32_dev(lsx_handle_t h, int n, int nrhs, const float *dLU, int lda,
                      const int32_t *d_ipiv, float *dB, int ldb);
int lsx_rref_f64_dev(lsx_handle_t h, int m, int n, int bar_col, double *dR, int ldr,
                     int32_t *d_pivots, int *d_rank, double tol, int pivot_rule);

/* Building blocks used by the multi-GPU driver (1-D block-cyclic columns,
 * SURVEY.md section 8e); all on device pointers, row-major. */
/* Factor the m x jb panel at dP (rows are global rows row0..row0+m-1); writes
 * d_ipiv[0..jb) as GLOBAL 0-based row indices and updates *d_info. */
int lsx_panel_f64_dev(lsx_handle_t h, int m, int jb, double *dP, int ldp, int row0,
                      int32_t *d_ipiv, int *d_info);
/* Apply the jb interchanges (k-th: row row0+k <-> d_ipiv[k]) to ncols columns of dA. */
int lsx_laswp_f64_dev(lsx_handle_t h, int ncols, double *dA, int lda, int row0, int jb,
                      const int32_t *d_ipiv);
/* The cooperative panel kernel also emits its interchanges as a gather list (256 x {dst, src}
 * row pairs relative to row0, -1 = unused).  lsx_panel_moves_dev copies the list of the LAST
 * lsx_panel_f64_dev call into d_moves (512 int32; *valid = 0 if that panel used the per-column
 * kernels and produced no list); lsx_laswp_moves_f64_dev applies such a list to ncols columns.
 * The multi-GPU driver ships the list inside the panel broadcast.
 * Requirements of lsx_laswp_moves_f64_dev: d_moves holds 512 int32 and is 8-byte aligned (it is read as 256 pairs);
 * the destinations of the used pairs are distinct; dA is the address of row 0 of the columns to move, row pair
 * (dst, src) means row row0 + dst <- row row0 + src, all sources read before any destination is written.  dA and lda
 * may have any alignment and ncols any value >= 0: 16-byte moves are used when dA is 16-byte aligned and lda and ncols
 * are even, element-wise moves otherwise, with the same result.  (The fused head of the look-ahead chain behind
 * lsx_diag_chain_head_* has the 16-byte form only and answers LSX_ERR_ARG to anything else.) */
int lsx_panel_moves_dev(lsx_handle_t h, int32_t *d_moves, int *valid);
int lsx_laswp_moves_f64_dev(lsx_handle_t h, int ncols, double *dA, int lda, int row0, const int32_t *d_moves);
/* dB (jb x ncols) <- inv(L11) * dB with L11 the unit-lower jb x jb block at dL. */
int lsx_trsm_lu_f64_dev(lsx_handle_t h, int jb, int ncols, const double *dL, int ldl, double *dB,
                        int ldb);
/* dC (m x n) -= dA (m x k) * dB (k x n) on the MFMA path. */
int lsx_gemm_sub_f64_dev(lsx_handle_t h, int m, int n, int k, const double *dA, int lda,
                         const double *dB, int ldb, double *dC, int ldc);
/* dC += dA * dB (same kernel, sign folded into the A operand). */
int lsx_gemm_add_f64_dev(lsx_handle_t h, int m, int n, int k, const double *dA, int lda,
                         const double *dB, int ldb, double *dC, int ldc);
int lsx_gemm_sub_f32_dev(lsx_handle_t h, int m, int n, int k, const float *dA, int lda,
                         const float *dB, int ldb, float *dC, int ldc);
/* "TN" forms of the same tile: dC (m x n) -= dA^T * dB with dA stored k x m, row-major, lda >= m (a block row of U or L
 * as it lies in the factors: the transposed sweeps).  Any m, n, k >= 0, any alignment and leading dimensions; a zero
 * extent leaves dC untouched (pointers may then be NULL).  Every n takes the MFMA tile and k is taken in ascending
 * order, so a column of dC gets the same bits whatever the other columns of the call are and whichever of the interior
 * and bounds-checked forms its tile takes.  LSX_ERR_ARG for negative sizes, lda < m, ldb < n, ldc < n or a NULL pointer
 * with non-zero sizes. */
int lsx_gemm_tn_sub_f64_dev(lsx_handle_t h, int m, int n, int k, const double *dA, int lda,
                            const double *dB, int ldb, double *dC, int ldc);
/* dC += dA^T * dB. */
int lsx_gemm_tn_add_f64_dev(lsx_handle_t h, int m, int n, int k, const double *dA, int lda,
                            const double *dB, int ldb, double *dC, int ldc);
int lsx_gemm_tn_sub_f32_dev(lsx_handle_t h, int m, int n, int k, const float *dA, int lda,
                            const float *dB, int ldb, float *dC, int ldc);

/* Deterministic synthetic inputs written straight into HBM:
 * element (i,j) = f(splitmix64(seed*GOLDEN + (i+row_off)<<32 + (j+col_off))). */
int lsx_fill_f64_dev(lsx_handle_t h, int kind, uint64_t seed, int m, int n, double *dA, int lda,
                     int row_off, int col_off);
int lsx_fill_f32_dev(lsx_handle_t h, int kind, uint64_t seed, int m, int n, float *dA, int lda,
                     int row_off, int col_off);

/* ---- multi-GPU, one call ---------------------------------------------------------------
 * P A = L U of an n x n matrix distributed 1-D block-cyclic by columns over ndev devices of one node: column block
 * b (width nb = the handles' "nb" option, the same on all) lives on device b % ndev; dA[d] is device d's local
 * matrix, all n rows of its blocks side by side, row-major with leading dimension lda[d].  handles[d] was created on
 * device d (several handles on one device are allowed: rehearsal).  Per step the owner factors the panel and writes
 * it to every peer directly (hipMemcpyPeerAsync per link, in row chunks that the receivers consume as they land);
 * no torch.distributed, no collective library.  d_ipiv[d] (n entries, on device d) receives the full interchange
 * list on every device, d_info[d] the info word.  Synchronous: returns when every device has finished.  Factors and
 * pivots are bit-identical to lsx_getrf_f64_dev on one device. */
int lsx_getrf_mg_f64(lsx_handle_t *handles, int ndev, int n, double *const *dA, const int *lda,
                     int32_t *const *d_ipiv, int *const *d_info);

/* ---- measurement --------------------------------------------------------- */
/* When enabled, every kernel launch of the selected buckets is bracketed by HIP
 * events on the launch stream; lsx_prof_read sums them (synchronises).
 * on: 0 = off, 1 = all buckets, otherwise (bucket mask << 1), e.g. 2 << LSX_PROF_GEMM. */
int lsx_prof_enable(lsx_handle_t h, int on);
int lsx_prof_reset(lsx_handle_t h);
int lsx_prof_read(lsx_handle_t h, int bucket, double *ms, long long *launches, double *flops,
                  double *bytes);

/* Diagnostics: sustained MFMA rate of a register-resident loop (synchronous).
 * is_f32 = 0: v_mfma_f64_16x16x4_f64, 1: v_mfma_f32_16x16x4_f32. */
int lsx_diag_mfma_peak(lsx_handle_t h, int is_f32, int iters, int blocks_per_cu, double *tflops,
                       double *clock_mhz /* fp64 only: median in-kernel shader clock, may be NULL */);
/* Diagnostics: cost of one round of the cross-CU record exchange under the panel factorisation
 * (synchronous).  G participants = the workgroups with blockIdx % stride == 0 (stride 8: one XCD under
 * round-robin dispatch); mode 0 = header all-gather, 1 = header all-gather + the 128-granule row of a
 * rotating winner, 2 = ping-pong between two participants; write_through 1 = `sc1` stores (device scope),
 * 0 = plain stores (XCD scope: only meaningful when xcc_ids come back all equal).  xcc_ids[G] may be NULL. */
int lsx_diag_xchg_probe(lsx_handle_t h, int mode, int G, int stride, int write_through, int epochs,
                        double *us_per_epoch, int *xcc_ids, int *nfail);
/* Diagnostics (residency tests): hold `wgs` (1..32) CUs of XCD `xcc` for `ms` milliseconds with a filler kernel on
 * a stream of its own; returns at once. */
int lsx_diag_occupy(lsx_handle_t h, int xcc, int wgs, int ms);
/* Diagnostics: launch nblocks workgroups on a stream created with the given CU mask (nwords = 0: the handle's
 * stream) and report where each landed: out[2 b] = XCC id, out[2 b + 1] = HW_ID register.  Synchronous. */
int lsx_diag_cu_mask_probe(lsx_handle_t h, const uint32_t *mask_words, int nwords, int nblocks, uint32_t *out);
/* Diagnostics: the 64 x 64 block inverses of the unit-lower jb x jb triangle at dT, through the fused head of the
 * look-ahead chain (fused = 1: inverses + the gather list d_moves applied to ncols columns at dA in ONE launch) or
 * through their own launch (fused = 0).  Device pointers, asynchronous on the handle's stream. */
int lsx_diag_chain_head_f32(lsx_handle_t h, int fused, int jb, const float *dT, int ldt, float *dTinv, int ncols,
                            float *dA, int lda, int row0, const int32_t *d_moves);
int lsx_diag_chain_head_f64(lsx_handle_t h, int fused, int jb, const double *dT, int ldt, double *dTinv, int ncols,
                            double *dA, int lda, int row0, const int32_t *d_moves);
/* Copy a piece of the handle's device scratch to the host (stamped diagnostic builds). */
int lsx_diag_read_scratch(lsx_handle_t h, size_t offset, void *dst, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* LSX_H */
