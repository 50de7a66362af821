// contrib/LOBPCGSolver.h used like the reference's class: a banded symmetric matrix of order 1000 (diagonal 1..n, off-diagonals
// +-1, +-2, +-5, +-64 in (-0.5, 0.5)), block size 4, solved four ways — with a sparse preconditioner diag(A)^-1 (setPreconditioner),
// as the pencil (A, B) with B = tridiag(0.3, 2, 0.3) (setB), with the Jacobi preconditioner (setJacobiPreconditioner), and with the
// first four eigenvectors as constraints (setConstraints).  compute(100, 1e-11) is the reference's relative tolerance: the threshold
// is 1e-11 * n = 1e-8.  Bars: info Success, ||A x - lambda B x||_2 < 2e-8 per column (recomputed here on the host), X'BX = I to 1e-10,
// the three standard solves agree to 2e-8 per eigenvalue, the constrained solve is orthogonal to Y and lies above it.
// Compiles on include/Spectra alone and with tests/cpp/eigen_lite in front (DenseMatrix / DenseVector are then the Eigen-named types).
#include <Spectra/contrib/LOBPCGSolver.h>

#include <cmath>
#include <cstdio>
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
    // Y = M X, column by column
    DenseMatrix<double> times(const DenseMatrix<double>& X) const
    {
        DenseMatrix<double> Y(n, X.cols());
        for (Index c = 0; c < X.cols(); c++)
        {
            for (int i = 0; i < n; i++)
                Y(i, c) = 0.0;
            for (int j = 0; j < n; j++)
                for (int p = colptr[j]; p < colptr[j + 1]; p++)
                    Y(rowind[p], c) += val[p] * X(j, c);
        }
        return Y;
    }
};

// symmetric band from per-offset value arrays: entry (i, i + off) = entry (i + off, i) = d[off][i]
static Csc band_matrix(int n, const std::vector<int>& offs, const std::vector<std::vector<double>>& d, const std::vector<double>& diag)
{
    Csc M;
    M.n = n;
    M.colptr.assign(1, 0);
    for (int j = 0; j < n; j++)
    {
        for (int k = int(offs.size()) - 1; k >= 0; k--)  // rows above the diagonal, ascending
            if (j - offs[k] >= 0)
            {
                M.rowind.push_back(j - offs[k]);
                M.val.push_back(d[k][j - offs[k]]);
            }
        M.rowind.push_back(j);
        M.val.push_back(diag[j]);
        for (std::size_t k = 0; k < offs.size(); k++)
            if (j + offs[k] < n)
            {
                M.rowind.push_back(j + offs[k]);
                M.val.push_back(d[k][j]);
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

// the bars on one solve; returns the largest residual norm
static double check(const char* name, LOBPCGSolver<double>& eigs, const Csc& A, const Csc* B, int m)
{
    const DenseVector<double> lam = eigs.eigenvalues();
    const DenseMatrix<double> X = eigs.eigenvectors(), R = eigs.residuals();
    const DenseMatrix<double> AX = A.times(X), BX = B ? B->times(X) : X;
    double worst = 0.0, orth = 0.0, rdiff = 0.0;
    for (int c = 0; c < m; c++)
    {
        double s = 0.0;
        for (int i = 0; i < A.n; i++)
        {
            const double r = AX(i, c) - lam[c] * BX(i, c);
            s += r * r;
            rdiff = std::fmax(rdiff, std::fabs(r - R(i, c)));
        }
        worst = std::fmax(worst, std::sqrt(s));
        for (int d = 0; d < m; d++)
        {
            double g = 0.0;
            for (int i = 0; i < A.n; i++)
                g += X(i, c) * BX(i, d);
            orth = std::fmax(orth, std::fabs(g - (c == d ? 1.0 : 0.0)));
        }
    }
    std::printf("%-28s info %d, %ld iterations, ||AX-BXD|| = %.3e, |X'BX - I| = %.3e\n", name, eigs.info(), long(eigs.num_iterations()), worst, orth);
    expect(eigs.info() == 0, "info is Success");
    expect(eigs.num_iterations() <= 100, "within 100 iterations");
    expect(worst < 2e-8, "residual below 2e-8");
    expect(orth < 1e-10, "B-orthonormal to 1e-10");
    expect(rdiff < 1e-10, "residuals() is A X - B X D");
    for (int c = 1; c < m; c++)
        expect(lam[c - 1] <= lam[c], "eigenvalues ascending");
    return worst;
}

int main()
{
    const int n = 1000, m = 4;
    const std::vector<int> offs = {1, 2, 5, 64};
    std::vector<std::vector<double>> d(offs.size());
    for (std::size_t k = 0; k < offs.size(); k++)
    {
        d[k].resize(std::size_t(n - offs[k]));
        for (double& v : d[k])
            v = uniform() - 0.5;
    }
    std::vector<double> diag(n), dinv(n);
    for (int i = 0; i < n; i++)
    {
        diag[i] = i + 1.0;
        dinv[i] = 1.0 / diag[i];
    }
    const Csc A = band_matrix(n, offs, d, diag);
    const Csc B = band_matrix(n, {1}, {std::vector<double>(std::size_t(n - 1), 0.3)}, std::vector<double>(std::size_t(n), 2.0));
    const Csc T = band_matrix(n, {}, {}, dinv);
    DenseMatrix<double> X0(n, m);
    for (int c = 0; c < m; c++)
        for (int i = 0; i < n; i++)
            X0(i, c) = 2.0 * uniform() - 1.0;

    // 1: standard problem, the preconditioner as a sparse matrix
    LOBPCGSolver<double> s1(A.view(), X0);
    expect(s1.info() == 3, "InvalidInput before compute()");
    s1.setPreconditioner(T.view());
    s1.compute(100, 1e-11);
    check("standard, T = diag(A)^-1", s1, A, nullptr, m);
    const DenseVector<double> lam1 = s1.eigenvalues();

    // 2: the pencil (A, B)
    LOBPCGSolver<double> s2(A.view(), X0);
    s2.setB(B.view());
    s2.setJacobiPreconditioner();
    s2.compute(100, 1e-11);
    check("setB, Jacobi", s2, A, &B, m);

    // 3: Jacobi, from an operator that is already on the device; to 1e-11 so that its vectors can serve as constraints
    SparseSymMatProd<double> Aop(A.view());
    LOBPCGSolver<double> s3(Aop, X0);
    s3.setJacobiPreconditioner();
    s3.compute(100, 1e-11);
    check("setJacobiPreconditioner", s3, A, nullptr, m);
    const DenseVector<double> lam3 = s3.eigenvalues();
    for (int c = 0; c < m; c++)
        expect(std::fabs(lam1[c] - lam3[c]) <= 2e-8, "sparse and Jacobi preconditioners give the same eigenvalues");
    s3.compute(100, 1e-14);  // warm start from the converged block
    expect(s3.info() == 0, "tighter solve converges");
    const DenseMatrix<double> Y = s3.eigenvectors();

    // 4: deflation against the first four eigenvectors
    LOBPCGSolver<double> s4(Aop, X0);
    s4.setJacobiPreconditioner();
    s4.setConstraints(Y);
    s4.compute(100, 1e-11);
    check("setConstraints", s4, A, nullptr, m);
    const DenseVector<double> lam4 = s4.eigenvalues();
    const DenseMatrix<double> X4 = s4.eigenvectors();
    expect(lam4[0] > lam3[m - 1], "constrained eigenvalues lie above the deflated ones");
    double yx = 0.0;
    for (int c = 0; c < m; c++)
        for (int e = 0; e < m; e++)
        {
            double g = 0.0;
            for (int i = 0; i < n; i++)
                g += Y(i, c) * X4(i, e);
            yx = std::fmax(yx, std::fabs(g));
        }
    std::printf("%-28s |Y'X| = %.3e\n", "", yx);
    expect(yx < 1e-10, "orthogonal to the constraints");

    // limits
    bool thrown = false;
    try
    {
        DenseMatrix<double> wide(n, 22);
        LOBPCGSolver<double> bad(Aop, wide);
    }
    catch (const std::invalid_argument&)
    {
        thrown = true;
    }
    expect(thrown, "22 columns are refused");

    if (g_fail == 0)
        std::printf("ALL PASSED\n");
    return g_fail == 0 ? 0 : 1;
}
