// GenEigsRealShiftSolver<SparseGenRealShiftSolve<double>> from C++ on a non-symmetric matrix beyond the dense path's n = 4096: the
// convection-diffusion operator of a 26 x 28 x 30 grid numbered along the short side (n = 21840) — the Kronecker sum of
// tridiag(lower -1 - c, 2, upper -1 + c) over the three axes, c = 0.1 — constructed with ShiftSolver::Auto: the iterative path
// (mispec_symshift_path_info says 3; ShiftSolver::Direct refuses the matrix at construction).  k = 4, ncv = 20, LargestMagn,
// tol 1e-11, sigma = 0.  The eigenvalues are real,
//   lambda(i, j, l) = sum over the axes of 2 - 2 sqrt(1 - c^2) cos(i pi / (m + 1));
// checked: the four smallest to 1e-9 relative, their imaginary parts zero, max |A X - X Lambda| <= 1e-10.
// Compiles on include/Spectra alone and with tests/cpp/eigen_lite in front.
#include <Spectra/GenEigsRealShiftSolver.h>
#include <Spectra/MatOp/SparseGenRealShiftSolve.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <stdexcept>
#include <vector>

using namespace Spectra;

static int g_failed = 0;
#define REQUIRE(cond)                                                      \
    do                                                                     \
    {                                                                      \
        if (!(cond))                                                       \
        {                                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            g_failed++;                                                    \
        }                                                                  \
    } while (0)

static const int P = 26, Q = 28, R = 30, N = P * Q * R;
static const double C = 0.1;

int main()
{
    // column-major, rows ascending within a column: vertex (i, j, l) -> (l Q + j) P + i; column c holds A(c - s, c) = -1 + C (the
    // upper diagonals) and A(c + s, c) = -1 - C (the lower ones) for the strides s = 1, P, P Q
    std::vector<int> colptr(1, 0), rowind;
    std::vector<double> val;
    for (int c = 0; c < N; c++)
    {
        const bool lo[3] = {c - P * Q >= 0, (c / P) % Q != 0, c % P != 0};          // neighbours at -P Q, -P, -1
        const bool hi[3] = {c % P != P - 1, (c / P) % Q != Q - 1, c + P * Q < N};    // neighbours at +1, +P, +P Q
        const int ls[3] = {P * Q, P, 1}, hs[3] = {1, P, P * Q};
        for (int a = 0; a < 3; a++)
            if (lo[a])
            {
                rowind.push_back(c - ls[a]);
                val.push_back(-1.0 + C);
            }
        rowind.push_back(c);
        val.push_back(6.0);
        for (int a = 0; a < 3; a++)
            if (hi[a])
            {
                rowind.push_back(c + hs[a]);
                val.push_back(-1.0 - C);
            }
        colptr.push_back(int(rowind.size()));
    }
    SparseView<double> A;
    A.rows = A.cols = N;
    A.outer = colptr.data();
    A.inner = rowind.data();
    A.values = val.data();
    A.row_major = false;

    const double pi = std::acos(-1.0), g = std::sqrt(1.0 - C * C);
    std::vector<double> lam;
    for (int i = 1; i <= P; i++)
        for (int j = 1; j <= Q; j++)
            for (int l = 1; l <= R; l++)
                lam.push_back((2.0 - 2.0 * g * std::cos(i * pi / (P + 1))) + (2.0 - 2.0 * g * std::cos(j * pi / (Q + 1))) +
                              (2.0 - 2.0 * g * std::cos(l * pi / (R + 1))));
    std::sort(lam.begin(), lam.end());

    {
        // the default is still the dense path: beyond n = 4096 the constructor refuses
        bool refused = false;
        try
        {
            SparseGenRealShiftSolve<double> direct(A, internal::CtxPtr(), ShiftSolver::Direct);
        }
        catch (const std::invalid_argument&)
        {
            refused = true;
        }
        REQUIRE(refused);
    }
    const int k = 4, m = 20;
    const double sigma = 0.0;
    SparseGenRealShiftSolve<double> op(A, internal::CtxPtr(), ShiftSolver::Auto);
    int path = -7;
    int64_t block_rows = -1, blocks = -1, bytes = -1;
    REQUIRE(mispec_symshift_path_info(op.mispec_solver(), &path, &block_rows, &blocks, &bytes) == MISPEC_OK);
    REQUIRE(path == 3 && block_rows == 0 && blocks == 0 && bytes == 0);
    GenEigsRealShiftSolver<SparseGenRealShiftSolve<double>> eigs(op, k, m, sigma);
    eigs.init();
    const int nconv = (int) eigs.compute(SortRule::LargestMagn, 1000, 1e-11);
    REQUIRE(eigs.info() == CompInfo::Successful);
    REQUIRE(nconv == k);
    if (nconv == k)
    {
        const auto evals = eigs.eigenvalues();
        const auto U = eigs.eigenvectors();
        std::vector<double> got(k);
        double im = 0.0;
        for (int c = 0; c < k; c++)
        {
            got[c] = std::real(evals[c]);
            im = std::max(im, std::abs(std::imag(evals[c])));
        }
        std::sort(got.begin(), got.end());
        double dl = 0.0;
        for (int c = 0; c < k; c++)
            dl = std::max(dl, std::abs(got[c] - lam[c]) / lam[c]);
        double res = 0.0;
        for (int c = 0; c < k; c++)
        {
            std::vector<std::complex<double>> au(N, std::complex<double>(0.0, 0.0));
            for (int j = 0; j < N; j++)
                for (int p = colptr[j]; p < colptr[j + 1]; p++)
                    au[rowind[p]] += val[p] * U(j, c);
            for (int i = 0; i < N; i++)
                res = std::max(res, std::abs(au[i] - evals[c] * U(i, c)));
        }
        int64_t last = 0, total = 0, solves = 0, probe = 0;
        int passes = 0;
        double omega = 1.0;
        REQUIRE(mispec_symshift_iterative_info(op.mispec_solver(), &last, &total, &solves, &passes, &omega, &probe) == MISPEC_OK);
        std::printf("sigma=%g nconv=%d nops=%d solves=%lld iterations=%lld max rel |lambda-closed form|=%.3e max|imag|=%.3e "
                    "||AX-XD||_max=%.3e\n",
                    sigma, nconv, (int) eigs.num_operations(), (long long) solves, (long long) total, dl, im, res);
        REQUIRE(solves >= eigs.num_operations() && total > 0 && probe > 0 && omega <= 1e-13);
        REQUIRE(dl <= 1e-9);
        REQUIRE(im == 0.0);
        REQUIRE(res <= 1e-10);
    }
    if (g_failed)
    {
        std::printf("%d checks FAILED\n", g_failed);
        return 1;
    }
    std::printf("ALL PASSED\n");
    return 0;
}
