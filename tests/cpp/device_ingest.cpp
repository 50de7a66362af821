// SparseSymMatProd::from_device used the way a HIP program would: the lower triangle of a 500-row band is put into device
// memory with hipMalloc / hipMemcpy, the operator is built from those addresses, and SymEigsSolver runs on it.  Everything is
// compared, exactly, with the operator the host constructor builds from the same arrays.  Compiled by
// tests/test_gpu_cpp_device_ingest.py with hipcc (host code only: the headers pass addresses on); needs a GPU to run.
#include <Spectra/MatOp/SparseGenMatProd.h>
#include <Spectra/MatOp/SparseSymMatProd.h>
#include <Spectra/SymEigsSolver.h>

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

using namespace Spectra;

static int failures = 0;
#define REQUIRE(cond)                                                        \
    do                                                                       \
    {                                                                        \
        if (!(cond))                                                         \
        {                                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            failures++;                                                      \
        }                                                                    \
    } while (0)
#define HIP_OK(expr)                                                                        \
    do                                                                                      \
    {                                                                                       \
        const hipError_t e_ = (expr);                                                       \
        if (e_ != hipSuccess)                                                               \
        {                                                                                   \
            std::printf("FAILED %s: %s\n", #expr, hipGetErrorString(e_));                   \
            return 2;                                                                       \
        }                                                                                   \
    } while (0)

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

int main()
{
    // lower triangle, CSC (Eigen's default): column j holds rows j, j + 1, j + 2, j + 40 inside the matrix
    const int n = 500;
    const int offs[4] = {0, 1, 2, 40};
    std::vector<long long> colptr(1, 0), rowind;
    std::vector<double> val;
    for (int j = 0; j < n; j++)
    {
        for (int o : offs)
            if (j + o < n)
            {
                rowind.push_back(j + o);
                val.push_back(o == 0 ? 4.0 + 0.001 * j : 1.0 / (1 + o) + 1e-4 * ((j * 7 + o) % 13));
            }
        colptr.push_back((long long) rowind.size());
    }
    const size_t nnz = rowind.size();

    void *d_outer = nullptr, *d_inner = nullptr, *d_val = nullptr;
    HIP_OK(hipMalloc(&d_outer, colptr.size() * sizeof(long long)));
    HIP_OK(hipMalloc(&d_inner, nnz * sizeof(long long)));
    HIP_OK(hipMalloc(&d_val, nnz * sizeof(double)));
    HIP_OK(hipMemcpy(d_outer, colptr.data(), colptr.size() * sizeof(long long), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_inner, rowind.data(), nnz * sizeof(long long), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_val, val.data(), nnz * sizeof(double), hipMemcpyHostToDevice));

    DeviceSparseView dv;
    dv.rows = dv.cols = n;
    dv.outer = d_outer;
    dv.inner = d_inner;
    dv.values = static_cast<const double*>(d_val);
    dv.index_bytes = 8;
    dv.row_major = false;
    using Op = SparseSymMatProd<double, Lower, ColMajor, long long>;
    Op dev = Op::from_device(dv);
    // the inputs were copied: release them before the operator is used
    HIP_OK(hipFree(d_outer));
    HIP_OK(hipFree(d_inner));
    HIP_OK(hipFree(d_val));

    SparseView<double, long long> hv;
    hv.rows = hv.cols = n;
    hv.outer = colptr.data();
    hv.inner = rowind.data();
    hv.values = val.data();
    hv.row_major = false;
    Op host(hv);

    REQUIRE(dev.rows() == n && dev.cols() == n);
    const int probes[][2] = {{0, 0}, {1, 0}, {0, 1}, {40, 0}, {0, 40}, {499, 459}, {459, 499}, {499, 499}, {3, 300}, {250, 248}};
    for (const auto& ij : probes)
        REQUIRE(same_bits(dev(ij[0], ij[1]), host(ij[0], ij[1])));
    REQUIRE(dev(3, 300) == 0.0 && dev(0, 40) == val[3]);

    const int nev = 4, ncv = 12;
    SymEigsSolver<Op> e_dev(dev, nev, ncv), e_host(host, nev, ncv);
    e_dev.init();
    e_host.init();
    const int c_dev = (int) e_dev.compute(SortRule::LargestMagn), c_host = (int) e_host.compute(SortRule::LargestMagn);
    REQUIRE(e_dev.info() == CompInfo::Successful && e_host.info() == CompInfo::Successful);
    REQUIRE(c_dev == nev && c_host == nev);
    REQUIRE(e_dev.num_iterations() == e_host.num_iterations() && e_dev.num_operations() == e_host.num_operations());
    const auto ev_dev = e_dev.eigenvalues(), ev_host = e_host.eigenvalues();
    for (int i = 0; i < nev; i++)
    {
        std::printf("lambda[%d] = %.17g (device ingest) %.17g (host ingest)\n", i, ev_dev[i], ev_host[i]);
        REQUIRE(same_bits(ev_dev[i], ev_host[i]));
    }

    // the argument checks of the host constructors: Flags against row_major, square
    bool threw = false;
    try
    {
        (void) SparseSymMatProd<double, Lower, RowMajor, long long>::from_device(dv);
    }
    catch (const std::invalid_argument&)
    {
        threw = true;
    }
    REQUIRE(threw);
    threw = false;
    try
    {
        (void) SparseGenMatProd<double, RowMajor>::from_device(dv);
    }
    catch (const std::invalid_argument&)
    {
        threw = true;
    }
    REQUIRE(threw);
    threw = false;
    try
    {
        DeviceSparseView rect = dv;
        rect.cols = n + 1;
        (void) Op::from_device(rect);
    }
    catch (const std::invalid_argument&)
    {
        threw = true;
    }
    REQUIRE(threw);

    std::printf(failures ? "%d FAILURES\n" : "ALL PASSED\n", failures);
    return failures ? 1 : 0;
}
