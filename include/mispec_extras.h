/* =============================================================================
 * mispec_extras.h — C ABI of the components OUTSIDE the hot path of SURVEY.md section 8
 * (BASELINE.json north_star): dense operators, the block Davidson solver, the complex-shift
 * operator / solver and the Buckling / Cayley modes of the generalized shift solver.  They were
 * built in rounds 1-2 and are kept working, but they are not part of the thin shim the hot path
 * needs: include/mispec.h alone is that shim.
 * Where they live (round 6): the Davidson solver, the complex factorisation and the complex Hermitian
 * eigensolver and the LOBPCG solver (mispec_davidson_*, mispec_zdense_*, mispec_zcsr_*, mispec_zfac_*, mispec_hermeigs_*, mispec_lobpcg_*: their
 * own kernels, nothing in the real hot path calls them) are in a library of their own, spectra_amd/libmispec_extras.so, built on libmispec.so — link -lmispec_extras
 * -lmispec.  The dense operators and the shift variants share objects with the hot path (the dense
 * GEMV applies the last level of the banded shift solve) and stay in libmispec.so.
 * Conventions (handles, error codes, ownership) as in mispec.h.
 * ============================================================================= */
#ifndef MISPEC_EXTRAS_H
#define MISPEC_EXTRAS_H

#include "mispec.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------
 * Dense operators — replace MatOp/DenseSymMatProd.h:28-105 and MatOp/DenseGenMatProd.h:27-102
 * (y = mat.selfadjointView<Uplo>() * x and y = mat * x).  The matrix is copied to HBM once, row-major.
 * uplo = 'L' / 'U': symmetric, only that triangle of the input is read (and mirrored); 0: general.
 * data_host is rows x cols with leading dimension ld_host, column-major unless row_major != 0.
 * ------------------------------------------------------------------------- */
typedef struct mispec_dense mispec_dense;
int mispec_dense_upload(mispec_ctx* ctx, int64_t rows, int64_t cols, const double* data_host, int64_t ld_host, int row_major,
                        char uplo, mispec_dense** out);
int mispec_dense_destroy(mispec_dense* D);
int64_t mispec_dense_rows(const mispec_dense* D);
int64_t mispec_dense_cols(const mispec_dense* D);
int mispec_dense_gemv(const mispec_dense* D, const double* x_dev, double* y_dev);        /* device pointers */
int mispec_dense_gemv_host(const mispec_dense* D, const double* x_host, double* y_host); /* literal perform_op */
/* Y = D X for a host block of k columns (operator*, DenseSymMatProd.h:93-96) and D(i,j) (operator(), :101-104) */
int mispec_dense_gemm_host(const mispec_dense* D, const double* X_host, int64_t ldx, int k, double* Y_host, int64_t ldy);
int mispec_dense_coeff(const mispec_dense* D, int64_t i, int64_t j, double* out);
/* average ms of `reps` back-to-back GEMV launches (benchmark helper, like mispec_spmv_time) */
int mispec_dense_gemv_time(const mispec_dense* D, const double* x_dev, double* y_dev, int reps, float* ms_per_launch);
/* Factorisation whose operator is the dense matrix (must be square). */
int mispec_fac_create_dense(mispec_ctx* ctx, const mispec_dense* D, int ncv, int symmetric, mispec_fac** out);

/* The same with the operator (A - sigma I)^{-1} of a device-resident shift solver (SymEigsShiftSolver path). */

/* ---------------------------------------------------------------------------
 * DavidsonSymEigsSolver — replaces DavidsonSymEigsSolver.h:18-90 + JDSymEigsBase.h:28-187 (block Davidson with the
 * diagonal-preconditioned-residual correction).  The search space, its image under A and the Ritz vectors live in
 * HBM; the projected eigenproblem (<= 256 x 256) is solved on the host.  The search space holds 256 vectors: a larger
 * nvec_max is lowered to 256 - correction size (earlier restarts, same results).
 * Operators: a device CSR matrix, a dense device matrix, or a device-pointer callback plus diag(A).
 * ------------------------------------------------------------------------- */
typedef struct mispec_davidson mispec_davidson;
int mispec_davidson_create(mispec_ctx* ctx, const mispec_csr* A, int64_t nev, int64_t nvec_init, int64_t nvec_max,
                           mispec_davidson** out);
int mispec_davidson_create_dense(mispec_ctx* ctx, const mispec_dense* D, int64_t nev, int64_t nvec_init, int64_t nvec_max,
                                 mispec_davidson** out);
int mispec_davidson_create_device_op(mispec_ctx* ctx, mispec_device_op_fn op, void* op_user, int64_t n, const double* diag_host,
                                     int64_t nev, int64_t nvec_init, int64_t nvec_max, mispec_davidson** out);
int mispec_davidson_destroy(mispec_davidson* S);
/* set_initial_search_space_size / set_max_search_space_size / set_correction_size (JDSymEigsBase.h:86-105); negative = keep */
int mispec_davidson_set_sizes(mispec_davidson* S, int64_t initial_search_space, int64_t max_search_space, int64_t correction);
int mispec_davidson_get_sizes(const mispec_davidson* S, int64_t* initial_search_space, int64_t* max_search_space, int64_t* correction);
/* compute(selection, maxit = 100, tol = 1e-10) (JDSymEigsBase.h:121-128); with guess_host != NULL compute_with_guess
 * (:130-184) on an n x guess_cols column-major block.  *nconv = converged pairs among the first nev. */
int mispec_davidson_compute(mispec_davidson* S, int selection, int64_t maxit, double tol, const double* guess_host,
                            int64_t guess_cols, int64_t ldg, int64_t* nconv);
int mispec_davidson_info(const mispec_davidson* S);               /* CompInfo as int */
int64_t mispec_davidson_num_iterations(const mispec_davidson* S);
int64_t mispec_davidson_num_operations(const mispec_davidson* S); /* matrix-vector products of the last compute() */
int mispec_davidson_eigenvalues(const mispec_davidson* S, double* out_host);                 /* nev values */
int mispec_davidson_eigenvectors(const mispec_davidson* S, double* out_host, int64_t ld);    /* n x nev, column-major */

/* Complex shift for the general operator (mispec_symshift_create_general): afterwards solve = Re((A - sigma I)^{-1} x), the
 * operator of GenEigsComplexShiftSolver (MatOp/SparseGenComplexShiftSolve.h:74-113, DenseGenComplexShiftSolve.h).  n <= 4096 on
 * the dense path; any n on the iterative path of a handle of mispec_symshift_create_general_complex. */
int mispec_symshift_set_shift_complex(mispec_symshift* S, double sigmar, double sigmai);
/* The general operator for complex shifts, with a solver kind: 0 direct (the dense path; n > 4096 refused), 1 auto (dense up to
 * n = 4096, iterative beyond), 2 iterative (for every n >= 1); anything else, -1 included, is MISPEC_EINVAL (option shift_solver
 * is not read).  Arguments, refusals and the operator built are those of mispec_symshift_create_general_solver.  On the ITERATIVE
 * PATH (path 3) mispec_symshift_set_shift_complex(sigmar, sigmai != 0) applies y = Re((A - sigma I)^{-1} x) by right-preconditioned
 * BiCGStab in complex arithmetic with the complex Jacobi preconditioner 1 / (diag A - sigma) (csrc/shift_zbicgstab.hip): A stays
 * real, a complex product is two real ones, and acceptance, restarts, refusal of a shift whose probe solve does not converge,
 * settings and counters are those of the real method; one ITERATION is two complex products.  A real shift
 * (mispec_symshift_set_shift, or sigmai == 0) runs the real BiCGStab of mispec_symshift_create_general_solver on the same
 * operator, and a handle goes back and forth between the two.  24 more work vectors of n doubles (12 complex ones, two planes
 * each) from the first complex shift on. */
int mispec_symshift_create_general_complex(mispec_ctx* ctx, int64_t n, const int32_t* outer_host, const int32_t* inner_host,
                                           const double* val_host, int row_major, int solver, mispec_symshift** out);
/* The path that constructor takes for dimension n under a solver kind (host arithmetic only): 0 or 3; MISPEC_EINVAL with the
 * constructor's wording where it refuses (direct, n > 4096), and for n < 1 or a solver outside 0 ... 2. */
int mispec_symshift_general_complex_solver_path(int64_t n, int solver);

/* The shift modes of the generalized solver (SymGEigsShiftSolver.h:36-207): operator y = (A - sigma B)^{-1} M x in the
 * B-inner product, with S the pencil solver of mispec_symshift_create_pencil (shift already set), B the matrix of the
 * inner product, and M = B (shift-invert and buckling modes) or, with cayley != 0, M = A + sigma B evaluated as
 * x + 2 sigma (A - sigma B)^{-1} B x (SymGEigsCayleyOp.h:88-99). */
int mispec_fac_create_geigs_shift(mispec_ctx* ctx, const mispec_symshift* S, const mispec_csr* B, int cayley, double sigma, int ncv,
                                  mispec_fac** out);

int mispec_symeigs_create_dense(mispec_ctx* ctx, const mispec_dense* D, int64_t nev, int64_t ncv, mispec_symeigs** out);

/* SymGEigsShiftSolver<SymShiftInvert, SparseSymMatProd, mode>: mode 0 = ShiftInvert (lambda = 1/nu + sigma),
 * 1 = Buckling (lambda = sigma nu / (nu - 1); S built from (K, KG), B = K), 2 = Cayley (lambda = sigma (nu+1)/(nu-1)).
 * Calls set_shift(sigma) on S. */
int mispec_symeigs_create_geigs_shift(mispec_ctx* ctx, mispec_symshift* S, const mispec_csr* B, int mode, int64_t nev, int64_t ncv,
                                      double sigma, mispec_symeigs** out);

/* GenEigsComplexShiftSolver (GenEigsComplexShiftSolver.h:20-150): Arnoldi on x -> Re((A - sigma I)^{-1} x); S from
 * mispec_symshift_create_general.  The solver leaves S at a real probe shift afterwards, like the reference. */
int mispec_geneigs_create_complex_shift(mispec_ctx* ctx, mispec_symshift* S, int64_t nev, int64_t ncv, double sigmar, double sigmai,
                                        mispec_geneigs** out);

int mispec_geneigs_create_dense(mispec_ctx* ctx, const mispec_dense* D, int64_t nev, int64_t ncv, mispec_geneigs** out);

/* ---------------------------------------------------------------------------
 * Complex scalars — the reference's factorisation templates instantiated with std::complex<double>
 * (LinAlg/Arnoldi.h:136-295, LinAlg/Lanczos.h:62-187 over MatOp/DenseGenMatProd.h / DenseHermMatProd.h; test/Arnoldi.cpp:122-158).
 * Complex numbers cross the boundary interleaved: a `double*` of 2 * count entries (re, im), the layout of std::complex<double>.
 * The basis, the residual and a dense operator live in HBM; steps are host-driven in the reference's order.
 * uplo = 'L' / 'U': Hermitian, only that triangle of the input is read (mirrored conjugated, diagonal taken real); 0: general.
 * ------------------------------------------------------------------------- */
typedef struct mispec_zdense mispec_zdense;
int mispec_zdense_upload(mispec_ctx* ctx, int64_t rows, int64_t cols, const double* data_host, int64_t ld_host, int row_major,
                         char uplo, mispec_zdense** out);
int mispec_zdense_destroy(mispec_zdense* D);
int64_t mispec_zdense_rows(const mispec_zdense* D);
int64_t mispec_zdense_cols(const mispec_zdense* D);
int mispec_zdense_gemv_host(const mispec_zdense* D, const double* x_host, double* y_host); /* literal perform_op */
int mispec_zdense_coeff(const mispec_zdense* D, int64_t i, int64_t j, double* out_re_im);
/* user operator on host pointers: y = Op(x), n complex entries each; non-zero return = error */
typedef int (*mispec_zop_fn)(void* user, const double* x_host, double* y_host);
typedef struct mispec_zfac mispec_zfac;
/* hermitian != 0: the three-term flow of Lanczos.h; 0: the full projection of Arnoldi.h */
int mispec_zfac_create_dense(mispec_ctx* ctx, const mispec_zdense* D, int ncv, int hermitian, mispec_zfac** out);
int mispec_zfac_create_op(mispec_ctx* ctx, mispec_zop_fn op, void* op_user, int64_t n, int ncv, int hermitian, mispec_zfac** out);
int mispec_zfac_destroy(mispec_zfac* F);
int mispec_zfac_init(mispec_zfac* F, const double* v0_host, int64_t* op_counter);
int mispec_zfac_factorize(mispec_zfac* F, int from_k, int to_m, int64_t* op_counter);
int mispec_zfac_subspace_dim(const mispec_zfac* F);
int mispec_zfac_f_norm(const mispec_zfac* F, double* out);
int mispec_zfac_get_H(const mispec_zfac* F, double* H_host);            /* ncv x ncv, column-major */
int mispec_zfac_get_V(const mispec_zfac* F, int ncols, double* V_host); /* n x ncols, column-major */
int mispec_zfac_get_f(const mispec_zfac* F, double* f_host);

/* ---------------------------------------------------------------------------
 * Complex Hermitian sparse operator — replaces MatOp/SparseHermMatProd.h (y = mat.selfadjointView<Uplo>() * x) for
 * std::complex<double>.  outer / inner are the compressed index arrays (int32 when index_bytes == 4, int64 when 8; narrowed to int32
 * at ingest, rejected if they do not fit), values the nnz complex entries; row_major != 0: CSR, else CSC.  Only the `uplo` ('L' / 'U')
 * triangle is read: it is mirrored conjugated into full CSR in HBM, the diagonal taken real.
 * ------------------------------------------------------------------------- */
typedef struct mispec_zcsr mispec_zcsr;
int mispec_zcsr_upload(mispec_ctx* ctx, int64_t rows, int64_t cols, const void* outer, const void* inner, int index_bytes,
                       const double* values, int row_major, char uplo, mispec_zcsr** out);
int mispec_zcsr_destroy(mispec_zcsr* A);
int64_t mispec_zcsr_rows(const mispec_zcsr* A);
int64_t mispec_zcsr_cols(const mispec_zcsr* A);
int64_t mispec_zcsr_nnz(const mispec_zcsr* A);                                          /* stored entries after the mirroring */
int mispec_zcsr_spmv_host(const mispec_zcsr* A, const double* x_host, double* y_host); /* literal perform_op */
int mispec_zcsr_coeff(const mispec_zcsr* A, int64_t i, int64_t j, double* out_re_im); /* operator()(i, j) of the mirrored matrix */
/* average ms of `reps` back-to-back products with lanes_per_row = 4, 8 or 16 lanes per row (0 = the default); benchmark helper */
int mispec_zcsr_spmv_time(const mispec_zcsr* A, int lanes_per_row, int reps, float* ms_per_launch);
/* mispec_zcsr_spmv_host with the kernel of lanes_per_row = 4, 8 or 16 lanes per row (anything else: MISPEC_EINVAL): the product of the
 * instantiations mispec_zcsr_spmv_time measures, for tests */
int mispec_zcsr_spmv_host_lanes(const mispec_zcsr* A, int lanes_per_row, const double* x_host, double* y_host);

/* Factorisation whose operator is the device complex sparse matrix (every product stays in HBM). */
int mispec_zfac_create_csr(mispec_ctx* ctx, const mispec_zcsr* A, int ncv, int hermitian, mispec_zfac** out);
/* The restart of HermEigsBase.h:105-155: the new ncv x ncv H from the host; then V[:, :k+1] <- V Q[:, :k+1] for a real ncv x ncv
 * column-major Q (Arnoldi.h:312-340 compress_V), f <- f Q(ncv-1, k-1) + V[:, k] H(k, k-1), beta = |f|, subspace dimension k. */
int mispec_zfac_set_H(mispec_zfac* F, const double* H_host);
int mispec_zfac_compress_real(mispec_zfac* F, const double* Q_host, int k);
/* X = V Y for a real ncv x nvec column-major Y: n x nvec complex, column-major, into X_host */
int mispec_zfac_ritz_vectors(mispec_zfac* F, const double* Y_host, int nvec, double* X_host);
/* benchmark helper on a full ncv-step factorisation: average ms of `reps` launches of which = 0: X^H y (both stages) over the first
 * ncols columns of V and y = f; which = 1: the in-place V Q kernel writing ncols columns (Q = I, V unchanged) */
int mispec_zfac_kernel_time(mispec_zfac* F, int which, int ncols, int reps, float* ms_per_launch);

/* ---------------------------------------------------------------------------
 * HermEigsSolver<OpType> for std::complex<double> (HermEigsSolver.h, HermEigsBase.h) behind handles, for bindings: the operator is a
 * device complex sparse matrix or a device dense Hermitian matrix (mispec_zdense_upload with uplo 'L' / 'U').  selection / sorting are
 * SortRule values (the five symmetric rules); eigenvalues are real, eigenvectors complex (n x nvec, column-major, interleaved).
 * ------------------------------------------------------------------------- */
typedef struct mispec_hermeigs mispec_hermeigs;
int mispec_hermeigs_create_csr(mispec_ctx* ctx, const mispec_zcsr* A, int64_t nev, int64_t ncv, mispec_hermeigs** out);
int mispec_hermeigs_create_dense(mispec_ctx* ctx, const mispec_zdense* D, int64_t nev, int64_t ncv, mispec_hermeigs** out);
int mispec_hermeigs_destroy(mispec_hermeigs* S);
int mispec_hermeigs_init(mispec_hermeigs* S, const double* v0_host); /* v0_host == NULL: SimpleRandom<complex>(0) */
int mispec_hermeigs_compute(mispec_hermeigs* S, int selection, int64_t maxit, double tol, int sorting, int64_t* nconv);
int mispec_hermeigs_info(const mispec_hermeigs* S);
int64_t mispec_hermeigs_num_iterations(const mispec_hermeigs* S);
int64_t mispec_hermeigs_num_operations(const mispec_hermeigs* S);
int mispec_hermeigs_eigenvalues(const mispec_hermeigs* S, double* out_host, int64_t* count);
int mispec_hermeigs_eigenvectors(const mispec_hermeigs* S, int64_t nvec, double* out_host, int64_t* ncols);

/* ---------------------------------------------------------------------------
 * LOBPCGSolver — replaces contrib/LOBPCGSolver.h: the m smallest (or largest) eigenpairs of the SPD pencil A x = lambda B x by the
 * locally optimal block preconditioned conjugate gradient method, with an optional preconditioner (a sparse matrix T applied as
 * R <- T R, or the Jacobi scaling by 1 / diag(A)), a warm start from an n x m block and constraints (deflation against known vectors).
 * The blocks [X | R | P], their images under A and B and the constraints live in HBM; per iteration there is ONE block product with A
 * on the active columns; the Gram matrices (order <= 63) are factored and the reduced eigenproblem is solved on the host.
 * Limits (MISPEC_EINVAL): 1 <= m <= 21 and m < n; at most 21 constraints, m + c < n; A square and unsharded; B and T of A's shape;
 * selection SmallestAlge (7) or LargestAlge (3).  Info: 0 Success, 1 NumericalIssue, 2 NoConvergence, 3 InvalidInput (before compute).
 * After NumericalIssue the eigenvalues / vectors are those of the last completed iteration (a failure in the setup: the start vectors
 * and their Rayleigh quotients).  Gram matrices are factored with pivots below 1e-8 refused, so a tolerance below the rounding level of
 * a residual ends in NumericalIssue, not NoConvergence.
 * ------------------------------------------------------------------------- */
typedef struct mispec_lobpcg mispec_lobpcg;
int mispec_lobpcg_create(mispec_ctx* ctx, const mispec_csr* A, int64_t m, mispec_lobpcg** out);
int mispec_lobpcg_destroy(mispec_lobpcg* S);
int mispec_lobpcg_set_B(mispec_lobpcg* S, const mispec_csr* B);              /* NULL: the standard problem again */
int mispec_lobpcg_set_preconditioner(mispec_lobpcg* S, const mispec_csr* T); /* NULL: none */
int mispec_lobpcg_set_jacobi(mispec_lobpcg* S, int on);                      /* needs a positive diagonal of A */
int mispec_lobpcg_set_constraints(mispec_lobpcg* S, const double* Y_host, int64_t ld, int64_t c); /* n x c, column-major; c = 0: none */
/* n x m column-major start block; without one the columns are SimpleRandom streams, seed j + 1 for column j */
int mispec_lobpcg_set_initial(mispec_lobpcg* S, const double* X_host, int64_t ld);
/* a column is converged when |A x - lambda B x|_2 < tol_abs; *nconv = converged columns (from the fresh products of the end) */
int mispec_lobpcg_compute(mispec_lobpcg* S, int selection, int64_t maxit, double tol_abs, int64_t* nconv);
int mispec_lobpcg_info(const mispec_lobpcg* S);
int64_t mispec_lobpcg_num_iterations(const mispec_lobpcg* S);
int64_t mispec_lobpcg_num_operations(const mispec_lobpcg* S); /* columns multiplied by A */
int64_t mispec_lobpcg_num_retries(const mispec_lobpcg* S);    /* iterations whose Rayleigh-Ritz step was repeated without P */
int mispec_lobpcg_eigenvalues(const mispec_lobpcg* S, double* out);                        /* m values */
int mispec_lobpcg_eigenvectors(const mispec_lobpcg* S, double* out_host, int64_t ld);      /* n x m, B-orthonormal */
int mispec_lobpcg_residuals(const mispec_lobpcg* S, double* out_host, int64_t ld);         /* A X - B X diag(lambda), n x m */
int mispec_lobpcg_residual_norms(const mispec_lobpcg* S, double* out);                     /* m values */
/* The solver's kernels alone, on device pointers (column-major blocks); enqueued on the context's stream, then synchronised.
 * For tests and measurements, not for inner loops: every call allocates and frees its own scratch (16 MB of partial records in HBM and a
 * pinned host buffer); the solver keeps one set per handle.
 * gram: G = U'W, p x q column-major into G_host, 1 <= p, q <= 64; symmetric != 0 (p == q): only i <= j is computed and mirrored.
 * resid: R[:, k] = (AX - lambda BX)[:, idx k] (times dinv[row] when dinv is given) for k < a, and norms2[j] = |AX_j - lambda_j BX_j|^2
 * of the unscaled residual for every j < m <= 21.  block_sub: Z <- Z - Y C for Z n x q, Y n x c, C c x q column-major, q, c <= 21. */
int mispec_lobpcg_gram(mispec_ctx* ctx, const double* U_dev, int64_t ldu, int p, const double* W_dev, int64_t ldw, int q, int64_t n,
                       int symmetric, double* G_host);
int mispec_lobpcg_resid(mispec_ctx* ctx, const double* AX_dev, const double* BX_dev, int64_t ld, int m, int64_t n, const double* lambda_host,
                        const int* idx_host, int a, const double* dinv_dev_or_null, double* R_dev, int64_t ldr, double* norms2_host);
int mispec_lobpcg_block_sub(mispec_ctx* ctx, double* Z_dev, int64_t ldz, int q, const double* Y_dev, int64_t ldy, int c, const double* C_host,
                            int64_t n);
/* average ms of `reps` back-to-back launches (both stages, no read-back) of which = 0: the Gram kernel on p columns of U and q of W;
 * 1: the residual kernel on p columns of U (as AX) and W (as BX), the first q active, R_dev the output; 2: the V*Q combination
 * R_dev[:, :q] = U[:, :p] Q of the Rayleigh-Ritz step (W_dev unused); benchmark helper */
int mispec_lobpcg_kernel_time(mispec_ctx* ctx, int which, const double* U_dev, const double* W_dev, int64_t ld, int p, int q, int64_t n,
                              double* R_dev, int reps, float* ms_per_launch);

#ifdef __cplusplus
}
#endif

#endif /* MISPEC_EXTRAS_H */
