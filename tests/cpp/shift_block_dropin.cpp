// perform_op_block of the shift-and-invert operators and LOBPCGSolver::setPreconditioner(solver) used from C++:
// K = tridiag(-1, 2, -1) of order 4500 and A = K + E, E = 0.002 x the graph Laplacian of the edges (i, i + 70).
//   1. SparseSymShiftSolve(K) and SymShiftInvert(K, B), B = tridiag(0.3, 2, 0.3): perform_op_block on 5 and 21 columns with leading
//      dimensions n and n + 3 equals perform_op column by column (memcmp).
//   2. LOBPCGSolver(A, X0) with block size 8 and setPreconditioner(SparseSymShiftSolve of K at sigma = 0): info Success within 40
//      iterations, ||A x - lambda x||_2 < 2e-8 per column, X'X = I to 1e-10; a solver of the wrong size throws "Wrong size".
// Compiles on include/Spectra alone and with tests/cpp/eigen_lite in front.
#include <Spectra/MatOp/SparseSymShiftSolve.h>
#include <Spectra/MatOp/SymShiftInvert.h>
#include <Spectra/contrib/LOBPCGSolver.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

using namespace Spectra;

struct Csc
{
    int n = 0;
    std::vector<int> colptr, rowind;
    std::vector<double> val;
    SparseView<double> view() const
    {
        SparseView<double> v;
        v.rows = v.cols = n;
        v.outer = colptr.data();
        v.inner = rowind.data();
        v.values = val.data();
        v.row_major = false;
        return v;
    }
};

// symmetric matrix with constant off-diagonals at the given offsets; lower_only keeps the lower triangle
static Csc band_matrix(int n, const std::vector<int>& offs, const std::vector<double>& offval, const std::vector<double>& diag, bool lower_only)
{
    Csc M;
    M.n = n;
    M.colptr.assign(1, 0);
    for (int j = 0; j < n; j++)
    {
        if (!lower_only)
            for (int k = int(offs.size()) - 1; k >= 0; k--)
                if (j - offs[k] >= 0)
                {
                    M.rowind.push_back(j - offs[k]);
                    M.val.push_back(offval[k]);
                }
        M.rowind.push_back(j);
        M.val.push_back(diag[j]);
        for (std::size_t k = 0; k < offs.size(); k++)
            if (j + offs[k] < n)
            {
                M.rowind.push_back(j + offs[k]);
                M.val.push_back(offval[k]);
            }
        M.colptr.push_back(int(M.rowind.size()));
    }
    return M;
}

static unsigned long long g_state = 88172645463325252ULL;
static double uniform()  // xorshift64, in [0, 1)
{
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return double(g_state >> 11) / 9007199254740992.0;
}

static int g_fail = 0;
static void expect(bool ok, const char* what)
{
    if (!ok)
    {
        std::printf("FAILED: %s\n", what);
        g_fail++;
    }
}

template <typename Op>
static void block_equals_columns(const char* name, const Op& op, int n)
{
    const int ks[2] = {5, 21};
    const int lds[2] = {n, n + 3};
    int bad = 0;
    for (int ki = 0; ki < 2; ki++)
        for (int li = 0; li < 2; li++)
        {
            const int k = ks[ki], ld = lds[li];
            std::vector<double> X(std::size_t(ld) * k, 7.25), Y(std::size_t(ld) * k, -1.0), y(n);
            for (int c = 0; c < k; c++)
                for (int i = 0; i < n; i++)
                    X[std::size_t(c) * ld + i] = 2.0 * uniform() - 1.0;
            op.perform_op_block(X.data(), ld, k, Y.data(), ld);
            for (int c = 0; c < k; c++)
            {
                op.perform_op(X.data() + std::size_t(c) * ld, y.data());
                if (std::memcmp(y.data(), Y.data() + std::size_t(c) * ld, std::size_t(n) * sizeof(double)) != 0)
                    bad++;
                for (int i = n; i < ld; i++)
                    if (Y[std::size_t(c) * ld + i] != -1.0)
                        bad++;
            }
        }
    std::printf("%-28s perform_op_block against perform_op: %d columns differ\n", name, bad);
    expect(bad == 0, "perform_op_block equals perform_op column by column");
}

int main()
{
    const int n = 4500, m = 8;
    const double w = 0.002;
    std::vector<double> two(n, 2.0), dA(n, 2.0);
    for (int i = 0; i < n; i++)
        dA[i] += (i + 70 < n ? w : 0.0) + (i - 70 >= 0 ? w : 0.0);
    const Csc Klow = band_matrix(n, {1}, {-1.0}, two, true);
    const Csc Blow = band_matrix(n, {1}, {0.3}, two, true);
    const Csc A = band_matrix(n, {1, 70}, {-1.0, -w}, dA, false);

    SparseSymShiftSolve<double> Kop(Klow.view());
    Kop.set_shift(0.0);
    block_equals_columns("SparseSymShiftSolve", Kop, n);
    SymShiftInvert<double, Sparse, Sparse> Pop(Klow.view(), Blow.view());
    Pop.set_shift(-0.5);
    block_equals_columns("SymShiftInvert", Pop, n);

    DenseMatrix<double> X0(n, m);
    for (int c = 0; c < m; c++)
        for (int i = 0; i < n; i++)
            X0(i, c) = 2.0 * uniform() - 1.0;
    LOBPCGSolver<double> eigs(A.view(), X0);
    {
        SparseSymShiftSolve<double> T(Klow.view());  // the solver keeps a shared copy: this object may go
        T.set_shift(0.0);
        eigs.setPreconditioner(T);
    }
    eigs.compute(40, 1e-8 / n);
    const DenseVector<double> lam = eigs.eigenvalues();
    const DenseMatrix<double> X = eigs.eigenvectors();
    double worst = 0.0, orth = 0.0;
    for (int c = 0; c < m; c++)
    {
        std::vector<double> r(n, 0.0);
        for (int j = 0; j < n; j++)
            for (int p = A.colptr[j]; p < A.colptr[j + 1]; p++)
                r[A.rowind[p]] += A.val[p] * X(j, c);
        double s = 0.0;
        for (int i = 0; i < n; i++)
            s += (r[i] - lam[c] * X(i, c)) * (r[i] - lam[c] * X(i, c));
        worst = std::fmax(worst, std::sqrt(s));
        for (int d = 0; d < m; d++)
        {
            double g = 0.0;
            for (int i = 0; i < n; i++)
                g += X(i, c) * X(i, d);
            orth = std::fmax(orth, std::fabs(g - (c == d ? 1.0 : 0.0)));
        }
    }
    std::printf("%-28s info %d, %ld iterations, ||AX-XD|| = %.3e, |X'X - I| = %.3e\n", "T = factorisation of K", eigs.info(),
                long(eigs.num_iterations()), worst, orth);
    expect(eigs.info() == 0, "info is Success");
    expect(eigs.num_iterations() <= 40, "within 40 iterations");
    expect(worst < 2e-8, "residual below 2e-8");
    expect(orth < 1e-10, "orthonormal to 1e-10");
    for (int c = 1; c < m; c++)
        expect(lam[c - 1] <= lam[c], "eigenvalues ascending");

    bool thrown = false;
    try
    {
        const Csc small = band_matrix(n - 1, {1}, {-1.0}, std::vector<double>(n - 1, 2.0), true);
        SparseSymShiftSolve<double> T(small.view());
        eigs.setPreconditioner(T);
    }
    catch (const std::invalid_argument& e)
    {
        thrown = std::string(e.what()) == "Wrong size";
    }
    expect(thrown, "a solver of another size throws Wrong size");

    if (g_fail == 0)
        std::printf("ALL PASSED\n");
    return g_fail == 0 ? 0 : 1;
}
