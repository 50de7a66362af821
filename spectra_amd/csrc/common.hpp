// Shared host-side plumbing of libmispec.so: error propagation across the C ABI,
// the context object, small RAII helpers.  gfx950 / ROCm only — no CUDA shims.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <functional>
#include <utility>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/mispec.h"
#include "../../include/mispec_extras.h"  // the library implements both headers

namespace mispec {

// Error carried through the library and turned into (code, thread-local message) at the C boundary.
struct Error : std::runtime_error
{
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

void set_last_error(const std::string& msg);

#define MISPEC_HIP(expr)                                                                                   \
    do                                                                                                     \
    {                                                                                                      \
        hipError_t _e = (expr);                                                                            \
        if (_e != hipSuccess)                                                                              \
            throw ::mispec::Error(MISPEC_ERUNTIME, std::string(#expr) + ": " + hipGetErrorString(_e) +     \
                                                       " (" __FILE__ ":" + std::to_string(__LINE__) + ")"); \
    } while (0)

#define MISPEC_REQUIRE(cond, msg)                       \
    do                                                  \
    {                                                   \
        if (!(cond))                                    \
            throw ::mispec::Error(MISPEC_EINVAL, msg);  \
    } while (0)

// Wrap the body of an extern "C" entry point.
template <typename F>
int guarded(F&& f) noexcept
{
    try
    {
        f();
        return MISPEC_OK;
    }
    catch (const Error& e)
    {
        set_last_error(e.what());
        return e.code;
    }
    catch (const std::invalid_argument& e)
    {
        set_last_error(e.what());
        return MISPEC_EINVAL;
    }
    catch (const std::logic_error& e)
    {
        set_last_error(e.what());
        return MISPEC_ELOGIC;
    }
    catch (const std::exception& e)
    {
        set_last_error(e.what());
        return MISPEC_ERUNTIME;
    }
    catch (...)
    {
        set_last_error("unknown error");
        return MISPEC_ERUNTIME;
    }
}

// Device buffer owned by a handle.
template <typename T>
struct DevBuf
{
    T* p = nullptr;
    size_t n = 0;
    DevBuf() {}
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void alloc(size_t count)
    {
        release();
        if (count)
            MISPEC_HIP(hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T)));
        n = count;
    }
    void release()
    {
        if (p)
            (void) hipFree(p);
        p = nullptr;
        n = 0;
    }
    void swap(DevBuf& o)
    {
        std::swap(p, o.p);
        std::swap(n, o.n);
    }
};

// Pinned host buffer (D2H targets of the per-step scalars).
template <typename T>
struct PinnedBuf
{
    T* p = nullptr;
    size_t n = 0;
    PinnedBuf() {}
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf()
    {
        if (p)
            (void) hipHostFree(p);
    }
    void alloc(size_t count)
    {
        if (p)
            (void) hipHostFree(p);
        p = nullptr;
        MISPEC_HIP(hipHostMalloc(reinterpret_cast<void**>(&p), count * sizeof(T), hipHostMallocDefault));
        n = count;
    }
};

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// Tuning switches and test hooks: ONE table (ctx.hip; include/mispec.h lists names and values), set through
// mispec_set_option(name, value).  An option that has not been set falls back to its environment variable MISPEC_<NAME> — the
// test-only override of the A/B tools and the parity tests (nothing else reads the environment); an empty variable counts as unset.
// Every read checks the value against the option's entry and throws Error(MISPEC_EINVAL) for one it does not accept, so an entry
// point that reads an option runs inside guarded().  Reads return values, never pointers into the table.
enum class Opt
{
    orth, one_reduction, orth_kernel, host_turn, small, restart_sync, host_steps, overlap, csr_win, spec_corr, exchange, reorder,
    spmv_staged, spmv_tiles, spmm, dia_sym, host_threads, shift, shift_block, shift_solver, count
};
// the values of the choice options, in the order of their entries' lists (`unset` is no value: the option not given)
enum class Orth { onesweep, onesweep_eager, reference, onesweep_wide };
enum class OrthKernel { dma, dma2, reg, unset };
enum class HostTurn { fast, copy };
enum class Small { host, host_serial, device };
enum class Exchange { allgather, halo, unset };
enum class Reorder { automatic, rcm, none };
enum class Tri { automatic, off, on };  // auto | 0 | 1
enum class DiaSym { automatic, off, all };  // auto | 0 | all: which symmetric diagonals the diagonal format mirrors (csr_dia.hip)
enum class Spmm { automatic, off, w2, w4, w8 };  // auto | 0 | 2 | 4 | 8: the widest panel of a block product (spmm.hip)
enum class ShiftBlock { automatic, off, w2, w4 };  // auto | 0 | 2 | 4: the widest panel of a block shift solve (shiftsolve.hip)
// direct | auto | iterative: the paths a shift-and-invert operator may take (shiftsolve.hip, shift_minres.hip); the values are the
// solver kinds of mispec_symshift_create_solver
enum class ShiftSolverKind { direct, automatic, iterative };
// choice option: its value as the enum above, `unset` when it is neither set nor in the environment
int option_choice(Opt o);  // the index of the value in the entry's list, -1 when unset
template <typename E>
E option_choice(Opt o, E unset)
{
    const int i = option_choice(o);
    return i < 0 ? unset : E(i);
}
bool option_flag(Opt o, bool unset);  // options of the values 0 | 1
int option_int(Opt o, int unset);     // integer options: the value, within the entry's range
// option shift: the key=value list of the banded shift solve's kernel variants, which tests require to agree (shiftsolve.hip), parsed;
// a key that is absent keeps its default.  Not a tuning interface: the defaults are the measured best.
struct ShiftOptions
{
    int lds = 1;              // 0: the general sweep kernel for every plain solve
    int batch = 0;            // 8 | 16 | 32 rows per batch of the staged sweeps (0: by half-bandwidth)
    int lanes = 0;            // 8 | 16 | 32 | 64 chunks per wavefront of the solve kernels (0: the default)
    int block_inverse = 256;  // MiB per level for the explicit chunk inverses (0: sweeps everywhere)
    int factor_host = 0;      // factor=host | device: the top level factored on the host / by k_chunk_factor
    int wave = 1;             // 0: the lane-per-chunk kernels for the host-factored wide levels
    int profile = 0;          // 1: set_shift's phases on stderr
    int minres_check = 16;    // 1 ... 64 iterations the iterative path (MINRES and BiCGStab alike) enqueues between two reads of its stop flag
};
ShiftOptions shift_options();

// malloc for the gigabyte-sized host arrays of the ingest stages (free with std::free).  Throws std::bad_alloc.
void* big_host_alloc(size_t bytes);

// Host array whose storage is NOT value-initialised (std::vector<T>::resize zero-fills on one thread and faults every page
// in there; the ingest stages fill gigabyte-sized arrays from many threads instead).  Trivially copyable T only.
template <typename T>
struct RawVec
{
    T* p = nullptr;
    size_t n = 0;
    RawVec() {}
    RawVec(const RawVec&) = delete;
    RawVec& operator=(const RawVec&) = delete;
    RawVec(RawVec&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    RawVec& operator=(RawVec&& o) noexcept
    {
        if (this != &o)
        {
            std::free(p);
            p = o.p;
            n = o.n;
            o.p = nullptr;
            o.n = 0;
        }
        return *this;
    }
    ~RawVec() { std::free(p); }
    void resize_uninitialized(size_t count)
    {
        std::free(p);
        p = count ? static_cast<T*>(big_host_alloc(count * sizeof(T))) : nullptr;
        n = count;
    }
    size_t size() const { return n; }
    T* data() { return p; }
    const T* data() const { return p; }
    T* begin() { return p; }
    T& operator[](size_t i) { return p[i]; }
    const T& operator[](size_t i) const { return p[i]; }
};

// Host threads of the ingest stages (format builders, triangle mirroring, validation passes): the machine's hardware threads,
// at most 64.  Every parallel stage produces the bytes the serial loop would.
int ingest_threads();
// fn(t, begin, end) over `parts` contiguous, nearly equal pieces of [0, n), one std::thread each (inline when parts <= 1);
// an exception thrown by a piece is rethrown on the calling thread.
void parallel_ranges(int64_t n, int parts, const std::function<void(int, int64_t, int64_t)>& fn);

}  // namespace mispec

// The context: one device, one stream, optional communicator for the row-sharded path.
struct mispec_ctx
{
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int num_cu = 256;
    // communicator (world == 1: no collectives are ever called)
    mispec_comm comm{0, 1, nullptr, nullptr, nullptr, nullptr};
    void* comm_owner = nullptr;                 // built-in communicator state to free with the ctx
    void (*comm_owner_free)(void*) = nullptr;

    void make_current() const { MISPEC_HIP(hipSetDevice(device)); }
    int rank() const { return comm.rank; }
    int world() const { return comm.world; }
};
