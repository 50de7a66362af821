// GenEigsComplexShiftSolver<SparseGenComplexShiftSolve<double>> from C++ on a non-symmetric matrix beyond the dense path's n = 4096:
// on a 20 x 21 x 22 grid numbered along the first axis (n = 9240), the Kronecker sum of tridiag(-1, 2, -1) over the first two axes
// and of tridiag(lower -g, 2, upper +g), g = 0.5, over the third — a normal matrix — constructed with ShiftSolver::Auto: the
// iterative path (mispec_symshift_path_info says 3), where the complex shift 1.5 + 1i is solved by BiCGStab in complex arithmetic
// and the solver's real probe shift by the real method.  The default constructor (ShiftSolver::Direct) refuses the matrix.
// k = 4, ncv = 20, LargestMagn, tol 1e-11.  The eigenvalues are
//   lambda(a, b, c) = (2 - 2 cos(a pi / 21)) + (2 - 2 cos(b pi / 22)) + 2 + 2 i g cos(c pi / 23);
// checked: 4 pairs, each within 1e-9 relative of a closed-form eigenvalue, the set {2.04269546 +- 0.99068595i,
// 2.04269546 +- 0.96291729i}, max |A X - X Lambda| <= 1e-10.
// Compiles on include/Spectra alone and with tests/cpp/eigen_lite in front.
#include <Spectra/GenEigsComplexShiftSolver.h>
#include <Spectra/MatOp/SparseGenComplexShiftSolve.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
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

static const int P = 20, Q = 21, R = 22, N = P * Q * R;
static const double G = 0.5;

int main()
{
    // column-major, rows ascending within a column: vertex (i, j, l) -> (l Q + j) P + i; column c holds A(c - s, c) (the upper
    // diagonals) and A(c + s, c) (the lower ones) for the strides s = 1, P, P Q: -1 on the first two axes, +g above and -g below on
    // the third
    std::vector<int> colptr(1, 0), rowind;
    std::vector<double> val;
    for (int c = 0; c < N; c++)
    {
        const bool lo[3] = {c - P * Q >= 0, (c / P) % Q != 0, c % P != 0};          // neighbours at -P Q, -P, -1
        const bool hi[3] = {c % P != P - 1, (c / P) % Q != Q - 1, c + P * Q < N};    // neighbours at +1, +P, +P Q
        const int ls[3] = {P * Q, P, 1}, hs[3] = {1, P, P * Q};
        const double lv[3] = {G, -1.0, -1.0}, hv[3] = {-1.0, -1.0, -G};
        for (int a = 0; a < 3; a++)
            if (lo[a])
            {
                rowind.push_back(c - ls[a]);
                val.push_back(lv[a]);
            }
        rowind.push_back(c);
        val.push_back(6.0);
        for (int a = 0; a < 3; a++)
            if (hi[a])
            {
                rowind.push_back(c + hs[a]);
                val.push_back(hv[a]);
            }
        colptr.push_back(int(rowind.size()));
    }
    SparseView<double> A;
    A.rows = A.cols = N;
    A.outer = colptr.data();
    A.inner = rowind.data();
    A.values = val.data();
    A.row_major = false;

    typedef std::complex<double> Cx;
    const double pi = std::acos(-1.0);
    std::vector<Cx> lam;
    for (int a = 1; a <= P; a++)
        for (int b = 1; b <= Q; b++)
            for (int c = 1; c <= R; c++)
                lam.push_back(Cx((2.0 - 2.0 * std::cos(a * pi / (P + 1))) + (2.0 - 2.0 * std::cos(b * pi / (Q + 1))) + 2.0,
                                 2.0 * G * std::cos(c * pi / (R + 1))));

    {
        // the default is still the dense path: beyond n = 4096 the constructor refuses
        bool refused = false;
        try
        {
            SparseGenComplexShiftSolve<double> direct(A);
        }
        catch (const std::invalid_argument& e)
        {
            refused = std::strstr(e.what(), "only n <= 4096") != nullptr;
        }
        REQUIRE(refused);
    }
    const int k = 4, m = 20;
    const double sigmar = 1.5, sigmai = 1.0;
    SparseGenComplexShiftSolve<double> op(A, internal::CtxPtr(), ShiftSolver::Auto);
    int path = -7;
    int64_t block_rows = -1, blocks = -1, bytes = -1;
    REQUIRE(mispec_symshift_path_info(op.mispec_solver(), &path, &block_rows, &blocks, &bytes) == MISPEC_OK);
    REQUIRE(path == 3 && block_rows == 0 && blocks == 0 && bytes == 0);
    GenEigsComplexShiftSolver<SparseGenComplexShiftSolve<double>> eigs(op, k, m, sigmar, sigmai);
    eigs.init();
    const int nconv = (int) eigs.compute(SortRule::LargestMagn, 1000, 1e-11);
    REQUIRE(eigs.info() == CompInfo::Successful);
    REQUIRE(nconv == k);
    if (nconv == k)
    {
        const auto evals = eigs.eigenvalues();
        const auto U = eigs.eigenvectors();
        const Cx want[4] = {Cx(2.04269546, 0.99068595), Cx(2.04269546, -0.99068595), Cx(2.04269546, 0.96291729), Cx(2.04269546, -0.96291729)};
        double dl = 0.0, dw = 0.0;
        for (int c = 0; c < k; c++)
        {
            const Cx e = evals[c];
            double best = 1e300, bw = 1e300, be = 1e300;
            for (std::size_t j = 0; j < lam.size(); j++)
                best = std::min(best, std::abs(lam[j] - e));
            for (int j = 0; j < k; j++)
            {
                bw = std::min(bw, std::abs(want[j] - e));
                be = std::min(be, std::abs(want[c] - Cx(evals[j])));
            }
            dl = std::max(dl, best / std::abs(e));
            dw = std::max(dw, std::max(bw, be));
            std::printf("lambda[%d] = %.10f %+.10fi\n", c, std::real(e), std::imag(e));
        }
        double res = 0.0;
        for (int c = 0; c < k; c++)
        {
            std::vector<Cx> au(N, Cx(0.0, 0.0));
            for (int j = 0; j < N; j++)
                for (int p = colptr[j]; p < colptr[j + 1]; p++)
                    au[rowind[p]] += val[p] * Cx(U(j, c));
            for (int i = 0; i < N; i++)
                res = std::max(res, std::abs(au[i] - Cx(evals[c]) * Cx(U(i, c))));
        }
        int64_t last = 0, total = 0, solves = 0, probe = 0;
        int passes = 0;
        double omega = 1.0;
        REQUIRE(mispec_symshift_iterative_info(op.mispec_solver(), &last, &total, &solves, &passes, &omega, &probe) == MISPEC_OK);
        std::printf("sigma=%g%+gi nconv=%d nops=%d solves=%lld iterations=%lld max rel |lambda-closed form|=%.3e "
                    "max |lambda-expected set|=%.3e ||AX-XD||_max=%.3e\n",
                    sigmar, sigmai, nconv, (int) eigs.num_operations(), (long long) solves, (long long) total, dl, dw, res);
        REQUIRE(solves >= eigs.num_operations() && total > 0 && probe > 0 && omega <= 1e-13);
        REQUIRE(dl <= 1e-9);
        REQUIRE(dw <= 1e-7);
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
