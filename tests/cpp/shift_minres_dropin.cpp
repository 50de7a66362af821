// SymEigsShiftSolver<SparseSymShiftSolve<double>> from C++ on a matrix no factorisation here takes: the 7-point Laplacian of a
// 26 x 28 x 30 grid numbered along the short side (n = 21840, half-bandwidth 728), constructed with ShiftSolver::Auto — the iterative
// path (mispec_symshift_path_info says 3; ShiftSolver::Direct still refuses it at set_shift) — k = 4, ncv = 20, LargestMagn,
// tol 1e-11, sigma = 0.  The eigenvalues are
//   lambda(i, j, l) = (2 - 2 cos(i pi / 27)) + (2 - 2 cos(j pi / 29)) + (2 - 2 cos(l pi / 31));
// checked: the four smallest to 1e-9, max |A X - X Lambda| <= 1e-10, max |X'X - I| <= 1e-10.
// Compiles on include/Spectra alone and with tests/cpp/eigen_lite in front.
#include <Spectra/MatOp/SparseSymShiftSolve.h>
#include <Spectra/SymEigsShiftSolver.h>

#include <algorithm>
#include <cmath>
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

int main()
{
    // lower triangle, column-major: vertex (i, j, l) -> (l Q + j) P + i; neighbours at +1, +P and +P Q
    std::vector<int> colptr(1, 0), rowind;
    std::vector<double> val;
    for (int c = 0; c < N; c++)
    {
        rowind.push_back(c);
        val.push_back(6.0);
        if (c % P != P - 1)
        {
            rowind.push_back(c + 1);
            val.push_back(-1.0);
        }
        if ((c / P) % Q != Q - 1)
        {
            rowind.push_back(c + P);
            val.push_back(-1.0);
        }
        if (c + P * Q < N)
        {
            rowind.push_back(c + P * Q);
            val.push_back(-1.0);
        }
        colptr.push_back(int(rowind.size()));
    }
    SparseView<double> A;
    A.rows = A.cols = N;
    A.outer = colptr.data();
    A.inner = rowind.data();
    A.values = val.data();
    A.row_major = false;

    const double pi = std::acos(-1.0);
    std::vector<double> lam;
    for (int i = 1; i <= P; i++)
        for (int j = 1; j <= Q; j++)
            for (int l = 1; l <= R; l++)
                lam.push_back((2.0 - 2.0 * std::cos(i * pi / (P + 1))) + (2.0 - 2.0 * std::cos(j * pi / (Q + 1))) +
                              (2.0 - 2.0 * std::cos(l * pi / (R + 1))));

    {
        // the default is still the direct paths: this band is refused
        SparseSymShiftSolve<double> direct(A, internal::CtxPtr(), ShiftSolver::Direct);
        bool refused = false;
        try
        {
            direct.set_shift(0.0);
        }
        catch (const std::invalid_argument&)
        {
            refused = true;
        }
        REQUIRE(refused);
    }
    const int k = 4, m = 20;
    for (int s = 0; s < 1; s++)
    {
        const double sigma = 0.0;
        SparseSymShiftSolve<double> op(A, internal::CtxPtr(), ShiftSolver::Auto);
        int path = -7;
        int64_t block_rows = -1, blocks = -1, bytes = -1;
        REQUIRE(mispec_symshift_path_info(op.mispec_solver(), &path, &block_rows, &blocks, &bytes) == MISPEC_OK);
        REQUIRE(path == 3 && block_rows == 0 && blocks == 0 && bytes == 0);
        SymEigsShiftSolver<SparseSymShiftSolve<double>> eigs(op, k, m, sigma);
        eigs.init();
        const int nconv = (int) eigs.compute(SortRule::LargestMagn, 1000, 1e-11);
        REQUIRE(eigs.info() == CompInfo::Successful);
        REQUIRE(nconv == k);
        const auto evals = eigs.eigenvalues();
        const auto evecs = eigs.eigenvectors();
        if (nconv != k)
            continue;

        std::vector<double> near(lam);
        std::sort(near.begin(), near.end(), [sigma](double a, double b) { return std::abs(a - sigma) < std::abs(b - sigma); });
        near.resize(k);
        std::sort(near.begin(), near.end());
        std::vector<double> got(k);
        for (int c = 0; c < k; c++)
            got[c] = evals[c];
        std::sort(got.begin(), got.end());
        double dl = 0.0;
        for (int c = 0; c < k; c++)
            dl = std::max(dl, std::abs(got[c] - near[c]));

        double res = 0.0, orth = 0.0;
        std::vector<double> y(N);
        for (int c = 0; c < k; c++)
        {
            std::fill(y.begin(), y.end(), 0.0);
            for (int j = 0; j < N; j++)
                for (int p = colptr[j]; p < colptr[j + 1]; p++)
                {
                    y[rowind[p]] += val[p] * evecs(j, c);
                    if (rowind[p] != j)
                        y[j] += val[p] * evecs(rowind[p], c);
                }
            for (int i = 0; i < N; i++)
                res = std::max(res, std::abs(y[i] - evals[c] * evecs(i, c)));
            for (int d = 0; d < k; d++)
            {
                double dot = 0.0;
                for (int i = 0; i < N; i++)
                    dot += evecs(i, c) * evecs(i, d);
                orth = std::max(orth, std::abs(dot - (c == d ? 1.0 : 0.0)));
            }
        }
        int64_t last = 0, total = 0, solves = 0, probe = 0;
        int passes = 0;
        double omega = 1.0;
        REQUIRE(mispec_symshift_iterative_info(op.mispec_solver(), &last, &total, &solves, &passes, &omega, &probe) == MISPEC_OK);
        std::printf("sigma=%g nconv=%d nops=%d solves=%lld iterations=%lld max|lambda-closed form|=%.3e ||AX-XD||_max=%.3e "
                    "||X'X-I||_max=%.3e\n",
                    sigma, nconv, (int) eigs.num_operations(), (long long) solves, (long long) total, dl, res, orth);
        REQUIRE(solves >= eigs.num_operations() && total > 0 && probe > 0 && omega <= 1e-13);
        REQUIRE(dl <= 1e-9);
        REQUIRE(res <= 1e-10);
        REQUIRE(orth <= 1e-10);
    }
    if (g_failed)
    {
        std::printf("%d checks FAILED\n", g_failed);
        return 1;
    }
    std::printf("ALL PASSED\n");
    return 0;
}
