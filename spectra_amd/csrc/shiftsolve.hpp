// Shift-and-invert operator y = (A - sigma I)^{-1} x held on the device (shiftsolve.hip).
#pragma once
#include <memory>

#include "common.hpp"

namespace mispec {
struct BandLevel;
constexpr int64_t kNarrowBandwidth = 8;  // up to here the top level is factored on the device and runs the LDS-staged sweeps
constexpr int64_t kMaxBandwidth = 64;    // banded path: half-bandwidth of A - sigma I the chunk kernels take at any level
constexpr int64_t kMaxDense = 4096;      // dense path: matrix dimension
// Which path a symmetric operator of dimension n and half-bandwidth b takes: the partitioned band factorisation for narrow bands
// (any n) and for bands of up to 64 beyond the dense limit; the dense inverse otherwise (n <= kMaxDense), else unsupported.
inline bool band_path(int64_t n, int64_t b) { return b <= kNarrowBandwidth || (b <= kMaxBandwidth && n > kMaxDense); }
constexpr int64_t kMaxBlockBandwidth = 512;  // block-tridiagonal path: one s x s block (s = half-bandwidth) is 2 MiB of an XCD's 4 MiB L2
// The path of (n, b), for every site that decides one: the chunk path where band_path says so, else the explicit inverse up to
// kMaxDense, else the block-tridiagonal factorisation (shift_blocktri.hip) up to kMaxBlockBandwidth, else none.  The values are
// those of mispec_symshift_path.  `iterative` (shift_minres.hip; shift_bicgstab.hip for a general operator) is never the answer of
// shift_path: an operator takes it only when its solver kind (option shift_solver, mispec_symshift_create_solver,
// mispec_symshift_create_general_solver) asks for it.
enum class ShiftPath { unsupported = -1, inverse = 0, chunk = 1, blocktri = 2, iterative = 3 };
inline ShiftPath shift_path(int64_t n, int64_t b)
{
    if (band_path(n, b))
        return ShiftPath::chunk;
    if (n <= kMaxDense)
        return ShiftPath::inverse;
    return b <= kMaxBlockBandwidth ? ShiftPath::blocktri : ShiftPath::unsupported;
}
// Block-tridiagonal factor of A - sigma B (shift_blocktri.hip): N = ceil(n / s) blocks of s = band_b rows, the last one padded
// with identity rows.  S_0 = D_0, L_i = E_i S_{i-1}^{-1}, S_i = D_i - L_i E_i'; kept are S_i^{-1} and L_i, s x s row-major each.
struct BlockTri
{
    int64_t s = 0, N = 0;
    DevBuf<double> sinv, l;  // N s^2 doubles each (l: block 0 unused)
    DevBuf<double> w;        // s^2: L_i while S_i is formed from E_i, which lies in l's slot until then
    DevBuf<double> y, z;     // N s: the padded vectors of a solve
    DevBuf<unsigned long long> record;  // [0] zero pivot columns, [1] bits of the smallest |pivot| / max |S_i|
    size_t factor_bytes() const { return 2 * size_t(N) * size_t(s) * size_t(s) * sizeof(double); }
};
struct ShiftIterative;  // the iterative path: what its two Krylov methods share (operator, counters; shift_iterative_state.hpp),
struct ShiftMinres;     // MINRES for symmetric operators and pencils (shift_minres.hip),
struct ShiftBicgstab;   // BiCGStab for general operators (shift_bicgstab.hip),
struct ShiftZBicgstab;  // ... and what a handle for complex shifts adds to it: BiCGStab in complex arithmetic (shift_zbicgstab.hip)
// the rule of a general operator (mispec_symshift_general_solver_path): the dense inverse up to kMaxDense under direct and auto,
// beyond it nothing (direct) or the iterative path (auto); iterative takes that path at every n
inline ShiftPath general_shift_path(int64_t n, ShiftSolverKind kind)
{
    if (kind != ShiftSolverKind::iterative && n <= kMaxDense)
        return ShiftPath::inverse;
    return kind == ShiftSolverKind::direct ? ShiftPath::unsupported : ShiftPath::iterative;
}
}  // namespace mispec

struct mispec_symshift
{
    mispec_ctx* ctx = nullptr;
    int64_t n = 0;
    // the selected triangle of A as (row >= col) triplets, host memory (the factorisation is redone per shift)
    std::vector<int64_t> rows, cols;
    std::vector<double> vals;
    int64_t half_bandwidth = 0;
    // banded path: the unshifted band A(i, i-d), n x (band_b + 1) row-major, built once at construction — on the
    // host (separator rows, pivots' scale) and resident in HBM (the device factorisation shifts a copy of it)
    std::vector<double> band0;
    mispec::DevBuf<double> band0_dev;
    int band_b = 0;
    // pencil form (SymShiftInvert, MatOp/SymShiftInvert.h:140-208): the operator is (A - sigma B)^{-1}; B is kept the
    // same way as A (band on host + device, or triplets for the dense path).  Empty: B = I.
    // general (non-symmetric) matrix — SparseGenRealShiftSolve: every stored entry is used as it is; the dense path, or the
    // iterative one (bicgstab below)
    bool general = false;
    bool pencil = false;
    std::vector<double> bandB0;
    mispec::DevBuf<double> bandB0_dev;
    std::vector<int64_t> rowsB, colsB;
    std::vector<double> valsB;
    double sigma = 0.0;
    bool factored = false;
    bool dense = false;
    std::unique_ptr<mispec::BandLevel> top;  // banded path
    std::unique_ptr<mispec::BlockTri> blocktri;  // block-tridiagonal path (65 <= band_b <= 512 beyond the dense limit)
    // iterative path: one of the two is set at construction, and no band and no triplets are kept then
    std::unique_ptr<mispec::ShiftMinres> minres;      // symmetric operator or pencil
    std::unique_ptr<mispec::ShiftBicgstab> bicgstab;  // general operator
    // a handle of mispec_symshift_create_general_complex on the iterative path has both: bicgstab (the operator, the counters, real
    // shifts) and zbicgstab (complex shifts).  sigma_im != 0: a complex shift sigma + i sigma_im is in effect and the solves are
    // zbicgstab's
    std::unique_ptr<mispec::ShiftZBicgstab> zbicgstab;
    double sigma_im = 0.0;
    bool complex_shift() const { return zbicgstab && sigma_im != 0.0; }
    mispec::ShiftIterative* iterative() const;        // whichever is set, or nullptr on a direct path
    mispec::ShiftPath path() const  // a general (non-symmetric) operator has the explicit inverse as its only direct path
    {
        if (minres || bicgstab)
            return mispec::ShiftPath::iterative;
        if (general)
            return n <= mispec::kMaxDense ? mispec::ShiftPath::inverse : mispec::ShiftPath::unsupported;
        return mispec::shift_path(n, half_bandwidth);
    }
    mispec::DevBuf<double> inverse;          // dense path: (A - sigma I)^{-1}, n x n column-major
    mutable mispec::DevBuf<double> stage_x, stage_y;
    // Robustness for indefinite A - sigma I (banded path): what the last factorisation saw and the number of iterative
    // refinement steps every solve performs (calibrated by set_shift on a probe right-hand side; 0 for definite matrices)
    long long boosted_pivots = 0;
    double min_pivot_ratio = 1.0;
    int refine_steps = 0;
    // SparseCholesky beyond the dense limit (cholesky.hip): factor the band itself (sigma = 0) and keep what G^{-1} / G^{-T}
    // need; cholesky_ready only when every pivot of every level was positive (the matrix is positive definite)
    bool want_cholesky = false, cholesky_ready = false;
    long long negative_pivots = 0;
    double probe_backward_error = 0.0;  // of the calibrated solve
    mutable mispec::DevBuf<double> ref_r, ref_dy;
    // Reordered at construction (round 5): a matrix beyond the dense limit whose band is too wide as it comes, but narrow after a
    // reverse Cuthill-McKee ordering (a banded matrix in a scattering row order, a path- or ladder-like graph), is stored as
    // P (A - sigma B) P' with (P x)[i] = x[perm[i]]; the solves keep the caller's index order (gather, solve, scatter).
    std::vector<int32_t> perm_host;     // new -> old; empty: not reordered
    mispec::DevBuf<int32_t> perm_dev;
    mutable mispec::DevBuf<double> perm_x, perm_y;
    // block solves (launch_shiftsolve_block): the panel versions of ref_r / ref_dy and perm_x / perm_y (four columns of leading
    // dimension panel_ld) and the staging blocks of the host entry, allocated at the first use and kept
    mutable mispec::DevBuf<double> panel_r, panel_dy, panel_px, panel_py, stage_X, stage_Y;
    mutable int64_t panel_ld = 0;
    int64_t half_bandwidth_as_given = 0;
    bool reordered() const { return perm_dev.p != nullptr; }
    ~mispec_symshift();
};

namespace mispec {
// y = (A - sigma I)^{-1} x, device pointers of n doubles, enqueued on the context stream
void launch_shiftsolve(const mispec_symshift& S, const double* x_dev, double* y_dev);
// Y[:, c] = (A - sigma B)^{-1} X[:, c] for c < k: column-major device blocks with ldx, ldy >= n that do not overlap, enqueued on
// the context stream.  The columns are cut into panels of 4 and 2 (option shift_block; shiftsolve_block_plan) that share one pass
// over the factor where a kernel is instantiated for that width; every column has exactly the bits launch_shiftsolve — the same
// code at width 1 — gives for it alone.
void launch_shiftsolve_block(const mispec_symshift& S, const double* X_dev, int64_t ldx, int k, double* Y_dev, int64_t ldy);
// Block-tridiagonal path (shift_blocktri.hip).  Factor: assembles the blocks of A - sigma B from the handle's resident band(s) and
// enqueues the whole chain on the context stream without a host synchronisation, then reads the device record once — throws
// "factorization failed with the given shift" for an exactly zero pivot column, returns the smallest pivot ratio.  Refuses with
// MISPEC_ERUNTIME "out of memory" before allocating when the factor does not fit the free device memory.
double blocktri_factor(mispec_symshift& S, double sigma);
// y = M^{-1} x in stored order with that factor: device pointers of n doubles, 2 N + 1 launches on the context stream
void blocktri_solve(const mispec_symshift& S, const double* x_dev, double* y_dev);
// Iterative path (shift_minres.hip): preconditioned MINRES on A - sigma B with the products of the handle's own CSR operators.
// minres_create builds them from the triangle(s) by the SpMV's ingest (B.outer == nullptr: B = I) and keeps diag and the row sums
// of |.|; minres_set_shift forms the Jacobi preconditioner and |M|_inf, solves the probe right-hand side and throws MISPEC_EINVAL
// "... did not converge ..." for a shift it cannot solve; minres_solve is y = (A - sigma B)^{-1} x in the caller's index order and
// throws MISPEC_ERUNTIME with the same wording.
struct TriangleView
{
    const int32_t* outer;
    const int32_t* inner;
    const double* val;
    char uplo;
    int row_major;
};
void minres_create(mispec_symshift& S, const TriangleView& A, const TriangleView& B);
void minres_set_shift(mispec_symshift& S, double sigma);
void minres_solve(const mispec_symshift& S, const double* x_dev, double* y_dev, bool probe = false);
// The same three for a general operator (shift_bicgstab.hip): right-preconditioned BiCGStab on A - sigma I with the products of
// the CSR operator the SpMV's general ingest builds from the compressed input (row_major as for mispec_symshift_create_general).
void bicgstab_create(mispec_symshift& S, const int32_t* outer, const int32_t* inner, const double* val, int row_major);
void bicgstab_set_shift(mispec_symshift& S, double sigma);
void bicgstab_solve(const mispec_symshift& S, const double* x_dev, double* y_dev, bool probe = false);
void bicgstab_alloc(mispec_symshift& S);  // the work vectors of bicgstab_set_shift, at the first shift of either kind
// Complex shifts on such a handle (shift_zbicgstab.hip): zbicgstab_create marks a handle that bicgstab_create built;
// zbicgstab_set_shift (sigmai != 0) forms the complex Jacobi preconditioner and solves the probe; zbicgstab_solve is
// y = Re((A - (sigma + i sigma_im) I)^{-1} x).  Errors as above.
void zbicgstab_create(mispec_symshift& S);
void zbicgstab_set_shift(mispec_symshift& S, double sigmar, double sigmai);
void zbicgstab_solve(const mispec_symshift& S, const double* x_dev, double* y_dev, bool probe = false);
// the probe right-hand side of set_shift's calibration: deterministic values in (-0.5, 0.5), on the context stream
void launch_probe_fill(const mispec_ctx& ctx, int64_t n, double* v_dev);
// the cut of k columns: widths 4 / 2 / 1, widest first.  panel: 0 = what option shift_block says, 1 = single columns, 2 | 4 = the
// widest panel
std::vector<int> shiftsolve_block_plan(int k, int panel);
// y = G^{-1} x (upper == false) / y = G^{-T} x (upper == true) for the factor G G' = A of a positive definite banded A that
// was factored with want_cholesky and sigma = 0
void launch_band_cholesky_solve(const mispec_symshift& S, bool upper, const double* x_dev, double* y_dev);
}  // namespace mispec
