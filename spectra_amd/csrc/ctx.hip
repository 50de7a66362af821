// Context, error state and the communicators of the row-sharded path.
//
// Multi-GPU model: one process (or, for the loopback test
// communicator, one host thread) per shard; each shard owns a contiguous block
// of rows of A, V, f.  Two collectives exist on the whole path: an all-gather
// of the current Krylov vector before each SpMV and a sum all-reduce of a few
// doubles (alpha, |f|^2, V'f).  The production communicator is RCCL over xGMI;
// librccl.so.1 is dlopen'ed lazily so that a single-GPU user never needs it and
// so that, inside a PyTorch process, torch's already-loaded RCCL is the one used.
#include "common.hpp"

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <condition_variable>
#include <exception>
#include <thread>
#include <cstring>
#include <mutex>

namespace mispec {
static thread_local std::string g_last_error;
void set_last_error(const std::string& msg) { g_last_error = msg; }

void* big_host_alloc(size_t bytes)
{
    // plain malloc: asking for transparent huge pages (madvise) made the first touch SLOWER where it was tried (direct
    // compaction and 2 MiB zeroing inside the page faults: 0.28 -> 2.8 s for the mirroring of a 2M-row matrix)
    void* q = std::malloc(bytes ? bytes : 1);
    if (!q)
        throw std::bad_alloc();
    return q;
}

// ---- options (common.hpp) ----------------------------------------------------------------------------------------------
namespace {
enum class Kind { choice, integer, shift };
constexpr int kMaxValues = 6;  // a list ends at its first null entry
struct OptionEntry
{
    Opt id;
    const char* name;
    const char* env;          // read when the option has not been set
    Kind kind;
    const char* values[kMaxValues];  // choice: the accepted values, in the order of the option's enum in common.hpp
    int lo, hi;               // integer: the accepted range
    const char* meaning;
};
constexpr int kMaxInt = 0x7fffffff;
constexpr OptionEntry kOptions[] = {
    {Opt::orth, "orth", "MISPEC_ORTH", Kind::choice, {"onesweep", "onesweep-eager", "reference", "onesweep-wide"}, 0, 0,
     "control flow of the Lanczos steps of the factorisations created afterwards"},
    {Opt::one_reduction, "one_reduction", "MISPEC_ONE_REDUCTION", Kind::choice, {"0", "1"}, 0, 0,
     "one reduction per one-sweep step (default 1)"},
    {Opt::orth_kernel, "orth_kernel", "MISPEC_ORTH_KERNEL", Kind::choice, {"dma", "dma2", "reg"}, 0, 0,
     "orthogonalisation passes through an LDS-DMA ring of three / two slots or through registers (unset: dma from 131072 rows)"},
    {Opt::host_turn, "host_turn", "MISPEC_HOST_TURN", Kind::choice, {"fast", "copy"}, 0, 0,
     "restart's host turn: pinned-memory kernels or hipMemcpy"},
    {Opt::small, "small", "MISPEC_SMALL", Kind::choice, {"host", "host-serial", "device"}, 0, 0,
     "where the ncv x ncv work of a restart runs"},
    {Opt::restart_sync, "restart_sync", "MISPEC_RESTART_SYNC", Kind::choice, {"0", "1"}, 0, 0, "synchronising fused restart"},
    {Opt::host_steps, "host_steps", "MISPEC_HOST_STEPS", Kind::choice, {"0", "1"}, 0, 0, "host-synchronous steps"},
    {Opt::overlap, "overlap", "MISPEC_OVERLAP", Kind::choice, {"0", "1"}, 0, 0,
     "sharded product: overlap of the exchange with the local rows (default 1)"},
    {Opt::csr_win, "csr_win", "MISPEC_CSR_WIN", Kind::choice, {"0", "1"}, 0, 0, "x windows of the int32 CSR kernel (default 1)"},
    {Opt::spec_corr, "spec_corr", "MISPEC_SPEC_CORR", Kind::integer, {}, 1, 4,
     "corrections enqueued speculatively per step (unset: 2, 1 when sharded)"},
    {Opt::exchange, "exchange", "MISPEC_EXCHANGE", Kind::choice, {"allgather", "halo"}, 0, 0,
     "sharded product: the all-gather or the neighbour exchange (unset: the exchange when the halos are small)"},
    {Opt::reorder, "reorder", "MISPEC_REORDER", Kind::choice, {"auto", "rcm", "none"}, 0, 0,
     "reverse Cuthill-McKee ordering at ingest and of the shift solve"},
    {Opt::spmv_staged, "spmv_staged", "MISPEC_SPMV_STAGED", Kind::choice, {"auto", "0", "1"}, 0, 0, "staged SpMV format"},
    {Opt::spmv_tiles, "spmv_tiles", "MISPEC_SPMV_TILES", Kind::choice, {"auto", "0", "1"}, 0, 0, "column-blocked tile SpMV format"},
    {Opt::spmm, "spmm", "MISPEC_SPMM", Kind::choice, {"auto", "0", "2", "4", "8"}, 0, 0,
     "widest panel of a block product (0: one SpMV per column)"},
    {Opt::dia_sym, "dia_sym", "MISPEC_DIA_SYM", Kind::choice, {"auto", "0", "all"}, 0, 0,
     "diagonal storage: lower diagonals read from their mirrored upper partner (auto: those within reach, 0: none, all)"},
    {Opt::host_threads, "host_threads", "MISPEC_HOST_THREADS", Kind::integer, {}, 1, kMaxInt,
     "upper bound on the host threads of the ingest and of the shift solve's host-side factorisation"},
    {Opt::shift, "shift", "MISPEC_SHIFT", Kind::shift, {}, 0, 0, "kernel variants of the banded shift solve"},
    {Opt::shift_block, "shift_block", "MISPEC_SHIFT_BLOCK", Kind::choice, {"auto", "0", "2", "4"}, 0, 0,
     "widest panel of a block shift solve (0: one solve per column)"},
    {Opt::shift_solver, "shift_solver", "MISPEC_SHIFT_SOLVER", Kind::choice, {"direct", "auto", "iterative"}, 0, 0,
     "shift-and-invert operators constructed afterwards: the direct paths only, the iterative path (shift_minres.hip; shift_bicgstab.hip for a general operator) where "
     "there is no direct one, or the iterative path always (default direct)"},
};
static_assert(sizeof(kOptions) / sizeof(kOptions[0]) == size_t(Opt::count), "one entry per option");
constexpr bool entries_in_order()
{
    for (size_t i = 0; i < size_t(Opt::count); i++)
        if (kOptions[i].id != Opt(i))
            return false;
    return true;
}
static_assert(entries_in_order(), "kOptions is indexed by Opt");

// keys of option shift; a numeric value is stored as its number, any other as its index in the list (no list: an integer >= 0)
struct ShiftKey
{
    const char* key;
    const char* values[kMaxValues];
    int ShiftOptions::*field;
    int lo = 0, hi = kMaxInt;  // no list: the accepted range
};
const ShiftKey kShiftKeys[] = {
    {"lds", {"0", "1"}, &ShiftOptions::lds},
    {"batch", {"8", "16", "32"}, &ShiftOptions::batch},
    {"lanes", {"8", "16", "32", "64"}, &ShiftOptions::lanes},
    {"block_inverse", {}, &ShiftOptions::block_inverse},
    {"factor", {"device", "host"}, &ShiftOptions::factor_host},
    {"wave", {"0", "1"}, &ShiftOptions::wave},
    {"profile", {"0", "1"}, &ShiftOptions::profile},
    {"minres_check", {}, &ShiftOptions::minres_check, 1, 64},
};

struct OptionValues
{
    std::mutex mu;
    bool set[size_t(Opt::count)] = {};
    std::string value[size_t(Opt::count)];
};
OptionValues& option_values()
{
    static OptionValues* v = new OptionValues;  // never destroyed: options may be read from static destructors
    return *v;
}

const OptionEntry* find_option(const char* name)
{
    for (const OptionEntry& e : kOptions)
        if (std::strcmp(e.name, name) == 0)
            return &e;
    return nullptr;
}

// The effective value of option e into `out`: the one set, else its environment variable's.  Returns where it came from (for
// messages), nullptr when there is none.
const char* effective(const OptionEntry& e, std::string& out)
{
    OptionValues& v = option_values();
    {
        std::lock_guard<std::mutex> lock(v.mu);
        if (v.set[size_t(e.id)])
        {
            out = v.value[size_t(e.id)];
            return "mispec_set_option";
        }
    }
    const char* env = std::getenv(e.env);
    if (!env || !*env)
        return nullptr;
    out = env;
    return e.env;
}

int index_of(const char* const (&values)[kMaxValues], const std::string& v)
{
    for (int i = 0; i < kMaxValues && values[i]; i++)
        if (v == values[i])
            return i;
    return -1;
}
bool parse_int(const std::string& v, int lo, int hi, int& out)
{
    if (v.empty() || v.size() > 10)
        return false;
    long long x = 0;
    for (const char c : v)
    {
        if (c < '0' || c > '9')
            return false;
        x = 10 * x + (c - '0');
    }
    out = int(x);
    return x >= lo && x <= hi;
}
std::string join(const char* const (&values)[kMaxValues], const char* sep)
{
    std::string s;
    for (int i = 0; i < kMaxValues && values[i]; i++)
        s += std::string(i ? sep : "") + values[i];
    return s;
}

[[noreturn]] void reject(const OptionEntry& e, const char* origin, const std::string& v)
{
    std::string accepted;
    if (e.kind == Kind::choice)
        accepted = join(e.values, " | ");
    else if (e.kind == Kind::integer)
        accepted = "an integer from " + std::to_string(e.lo) + (e.hi == kMaxInt ? " on" : " to " + std::to_string(e.hi));
    else
    {
        accepted = "a comma list of";
        for (const ShiftKey& k : kShiftKeys)
            accepted += std::string(&k == kShiftKeys ? " " : ", ") + k.key + "=" +
                        (k.values[0] ? join(k.values, "|")
                                     : k.hi == kMaxInt ? std::string("<integer from 0 on>")
                                                       : "<integer from " + std::to_string(k.lo) + " to " + std::to_string(k.hi) + ">");
        accepted += ", each key at most once";
    }
    throw Error(MISPEC_EINVAL, std::string(origin) + ": '" + v + "' is not a value of option " + e.name + " (" + e.meaning +
                                   "); accepted: " + accepted);
}

ShiftOptions parse_shift(const std::string& spec, const char* origin)
{
    ShiftOptions s;
    unsigned seen = 0;
    for (size_t pos = 0; pos <= spec.size();)
    {
        const size_t end = std::min(spec.find(',', pos), spec.size());
        const std::string item = spec.substr(pos, end - pos);
        const size_t eq = item.find('=');
        const ShiftKey* key = nullptr;
        for (const ShiftKey& k : kShiftKeys)
            if (eq != std::string::npos && item.compare(0, eq, k.key) == 0)
                key = &k;
        const unsigned bit = key ? 1u << (key - kShiftKeys) : 0u;
        const std::string v = key ? item.substr(eq + 1) : item;
        int x = 0;
        const int i = key ? index_of(key->values, v) : -1;
        const bool number = parse_int(v, key ? key->lo : 0, key ? key->hi : kMaxInt, x);
        if (!key || (seen & bit) || (key->values[0] ? i < 0 : !number))
            reject(kOptions[size_t(Opt::shift)], origin, spec);
        s.*key->field = number ? x : i;
        seen |= bit;
        pos = end + 1;
    }
    return s;
}

// the index of a choice option's value / an integer option's value; throws for a value the option does not accept
int check(const OptionEntry& e, const std::string& v, const char* origin)
{
    int x = -1;
    if (e.kind == Kind::shift)
        parse_shift(v, origin);
    else if (e.kind == Kind::choice ? (x = index_of(e.values, v)) < 0 : !parse_int(v, e.lo, e.hi, x))
        reject(e, origin, v);
    return x;
}
bool read(Opt o, int& x)
{
    const OptionEntry& e = kOptions[size_t(o)];
    std::string v;
    const char* origin = effective(e, v);
    if (origin)
        x = check(e, v, origin);
    return origin != nullptr;
}
}  // namespace

int option_choice(Opt o)
{
    int x = -1;
    return read(o, x) ? x : -1;
}
bool option_flag(Opt o, bool unset)
{
    int x = 0;
    return read(o, x) ? x != 0 : unset;
}
int option_int(Opt o, int unset)
{
    int x = 0;
    return read(o, x) ? x : unset;
}
ShiftOptions shift_options()
{
    const OptionEntry& e = kOptions[size_t(Opt::shift)];
    std::string v;
    const char* origin = effective(e, v);
    return origin ? parse_shift(v, origin) : ShiftOptions{};
}

int ingest_threads()
{
    static const int n = [] {
        const unsigned hw = std::thread::hardware_concurrency();
        return int(std::min(64u, std::max(1u, hw)));
    }();
    // option host_threads (tests): an upper bound on the host threads of the ingest and of the shift solve's host-side
    // factorisation — their results must not depend on it
    return std::min(n, option_int(Opt::host_threads, n));
}

void parallel_ranges(int64_t n, int parts, const std::function<void(int, int64_t, int64_t)>& fn)
{
    if (n <= 0)
        return;
    parts = int(std::max<int64_t>(1, std::min<int64_t>(parts, n)));
    if (parts == 1)
    {
        fn(0, 0, n);
        return;
    }
    std::vector<std::thread> th;
    std::vector<std::exception_ptr> err(static_cast<size_t>(parts));
    th.reserve(static_cast<size_t>(parts));
    for (int t = 0; t < parts; t++)
    {
        const int64_t b = n * t / parts, e = n * (t + 1) / parts;
        th.emplace_back([&, t, b, e] {
            try
            {
                fn(t, b, e);
            }
            catch (...)
            {
                err[size_t(t)] = std::current_exception();
            }
        });
    }
    for (auto& t : th)
        t.join();
    for (auto& e : err)
        if (e)
            std::rethrow_exception(e);
}
}  // namespace mispec

using namespace mispec;

extern "C" const char* mispec_last_error(void) { return g_last_error.c_str(); }
extern "C" const char* mispec_version(void) { return "0.1.0 (gfx950)"; }

extern "C" int mispec_set_option(const char* name, const char* value)
{
    return guarded([&] {
        MISPEC_REQUIRE(name != nullptr, "mispec_set_option: name is NULL");
        const OptionEntry* e = find_option(name);
        MISPEC_REQUIRE(e, std::string("mispec_set_option: unknown option '") + name + "'");
        if (value)
            check(*e, value, "mispec_set_option");
        OptionValues& v = option_values();
        std::lock_guard<std::mutex> lock(v.mu);
        v.set[size_t(e->id)] = value != nullptr;
        v.value[size_t(e->id)] = value ? value : "";
    });
}

// introspection: the effective string, not checked, in a copy of the calling thread's
extern "C" const char* mispec_get_option(const char* name)
{
    static thread_local std::string copy;
    const char* out = nullptr;
    (void) guarded([&] {
        const OptionEntry* e = name ? find_option(name) : nullptr;
        MISPEC_REQUIRE(e, std::string("mispec_get_option: unknown option '") + (name ? name : "(null)") + "'");
        if (effective(*e, copy))
            out = copy.c_str();
    });
    return out;
}

extern "C" int mispec_ctx_create(int device, void* hip_stream, mispec_ctx** out)
{
    return guarded([&] {
        MISPEC_REQUIRE(out != nullptr, "mispec_ctx_create: out is NULL");
        int ndev = 0;
        hipError_t e = hipGetDeviceCount(&ndev);
        if (e != hipSuccess || ndev <= 0)
            throw Error(MISPEC_ERUNTIME, "mispec_ctx_create: no HIP device available (this library has no CPU fallback)");
        MISPEC_REQUIRE(device >= 0 && device < ndev, "mispec_ctx_create: device index out of range");
        auto* ctx = new mispec_ctx();
        try
        {
            ctx->device = device;
            MISPEC_HIP(hipSetDevice(device));
            hipDeviceProp_t prop;
            MISPEC_HIP(hipGetDeviceProperties(&prop, device));
            ctx->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
            if (hip_stream)
            {
                ctx->stream = static_cast<hipStream_t>(hip_stream);
                ctx->own_stream = false;
            }
            else
            {
                MISPEC_HIP(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
                ctx->own_stream = true;
            }
        }
        catch (...)
        {
            delete ctx;
            throw;
        }
        *out = ctx;
    });
}

extern "C" int mispec_ctx_destroy(mispec_ctx* ctx)
{
    return guarded([&] {
        if (!ctx)
            return;
        (void) hipSetDevice(ctx->device);
        if (ctx->comm_owner && ctx->comm_owner_free)
            ctx->comm_owner_free(ctx->comm_owner);
        if (ctx->own_stream && ctx->stream)
            (void) hipStreamDestroy(ctx->stream);
        delete ctx;
    });
}

extern "C" int mispec_ctx_sync(mispec_ctx* ctx)
{
    return guarded([&] {
        MISPEC_REQUIRE(ctx, "mispec_ctx_sync: ctx is NULL");
        ctx->make_current();
        MISPEC_HIP(hipStreamSynchronize(ctx->stream));
    });
}

extern "C" void* mispec_ctx_stream(mispec_ctx* ctx) { return ctx ? static_cast<void*>(ctx->stream) : nullptr; }

extern "C" int mispec_ctx_set_comm(mispec_ctx* ctx, const mispec_comm* comm)
{
    return guarded([&] {
        MISPEC_REQUIRE(ctx && comm, "mispec_ctx_set_comm: NULL argument");
        MISPEC_REQUIRE(comm->world >= 1 && comm->rank >= 0 && comm->rank < comm->world,
                       "mispec_ctx_set_comm: need 0 <= rank < world");
        MISPEC_REQUIRE(comm->world == 1 || (comm->allgather && comm->allreduce_sum),
                       "mispec_ctx_set_comm: collectives missing");
        MISPEC_REQUIRE((comm->allgather == nullptr) == (comm->allreduce_sum == nullptr),
                       "mispec_ctx_set_comm: give both collectives or none");
        ctx->comm = *comm;
    });
}

// ---------------------------------------------------------------------------------------------
// Row partition: equal blocks, so that the all-gather is a plain equal-count collective.
// The block is even so every shard's slice of a 16-byte-aligned vector stays 16-byte aligned.
// ---------------------------------------------------------------------------------------------
extern "C" int64_t mispec_shard_block(int64_t n, int world)
{
    if (world <= 1)
        return n;
    int64_t b = (n + world - 1) / world;
    return (b + 1) & ~int64_t(1);
}

extern "C" int mispec_shard_range(int64_t n, int world, int rank, int64_t* begin, int64_t* end)
{
    return guarded([&] {
        MISPEC_REQUIRE(begin && end && world >= 1 && rank >= 0 && rank < world && n >= 0, "mispec_shard_range: bad argument");
        const int64_t b = mispec_shard_block(n, world);
        int64_t lo = b * rank, hi = b * (rank + 1);
        if (lo > n)
            lo = n;
        if (hi > n)
            hi = n;
        *begin = lo;
        *end = hi;
    });
}

// ---------------------------------------------------------------------------------------------
// RCCL communicator (dlopen)
// ---------------------------------------------------------------------------------------------
namespace {
struct RcclApi
{
    void* handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};

RcclApi& rccl()
{
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char* nm : names)
        {
            api.handle = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
            if (api.handle)
                break;
        }
        if (!api.handle)
            return;
        api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(dlsym(api.handle, "ncclGetUniqueId"));
        api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(dlsym(api.handle, "ncclCommInitRank"));
        api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(dlsym(api.handle, "ncclCommDestroy"));
        api.AllGather = reinterpret_cast<decltype(api.AllGather)>(dlsym(api.handle, "ncclAllGather"));
        api.AllReduce = reinterpret_cast<decltype(api.AllReduce)>(dlsym(api.handle, "ncclAllReduce"));
        api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(dlsym(api.handle, "ncclGetErrorString"));
        api.Send = reinterpret_cast<decltype(api.Send)>(dlsym(api.handle, "ncclSend"));
        api.Recv = reinterpret_cast<decltype(api.Recv)>(dlsym(api.handle, "ncclRecv"));
        api.GroupStart = reinterpret_cast<decltype(api.GroupStart)>(dlsym(api.handle, "ncclGroupStart"));
        api.GroupEnd = reinterpret_cast<decltype(api.GroupEnd)>(dlsym(api.handle, "ncclGroupEnd"));
    });
    if (!api.handle || !api.GetUniqueId || !api.CommInitRank || !api.AllGather || !api.AllReduce)
        throw Error(MISPEC_ERUNTIME, "RCCL is not available (dlopen librccl.so.1 failed)");
    return api;
}

void rccl_check(ncclResult_t r, const char* what)
{
    if (r != ncclSuccess)
        throw Error(MISPEC_ERUNTIME, std::string(what) + ": " + (rccl().GetErrorString ? rccl().GetErrorString(r) : "RCCL error"));
}

struct RcclComm
{
    ncclComm_t comm = nullptr;
    int rank = 0, world = 1;
};

int rccl_allgather(void* user, const double* send, double* recv, int64_t count, void* stream)
{
    return guarded([&] {
        auto* c = static_cast<RcclComm*>(user);
        rccl_check(rccl().AllGather(send, recv, size_t(count), ncclDouble, c->comm, static_cast<hipStream_t>(stream)),
                   "ncclAllGather");
    });
}
int rccl_allreduce(void* user, double* buf, int64_t count, void* stream)
{
    return guarded([&] {
        auto* c = static_cast<RcclComm*>(user);
        rccl_check(rccl().AllReduce(buf, buf, size_t(count), ncclDouble, ncclSum, c->comm, static_cast<hipStream_t>(stream)),
                   "ncclAllReduce");
    });
}
// Neighbour exchange: every non-empty range is one ncclSend / ncclRecv of a group, so the transfers to all
// peers run concurrently on their own xGMI links.
int rccl_exchange(void* user, const double* send, const int64_t* send_off, const int64_t* send_count, double* recv,
                  const int64_t* recv_off, const int64_t* recv_count, void* stream)
{
    return guarded([&] {
        auto* c = static_cast<RcclComm*>(user);
        hipStream_t s = static_cast<hipStream_t>(stream);
        rccl_check(rccl().GroupStart(), "ncclGroupStart");
        for (int p = 0; p < c->world; p++)
        {
            if (p == c->rank)
                continue;
            if (send_count[p] > 0)
                rccl_check(rccl().Send(send + send_off[p], size_t(send_count[p]), ncclDouble, p, c->comm, s), "ncclSend");
            if (recv_count[p] > 0)
                rccl_check(rccl().Recv(recv + recv_off[p], size_t(recv_count[p]), ncclDouble, p, c->comm, s), "ncclRecv");
        }
        rccl_check(rccl().GroupEnd(), "ncclGroupEnd");
    });
}
void rccl_free(void* p)
{
    auto* c = static_cast<RcclComm*>(p);
    if (c->comm)
        (void) rccl().CommDestroy(c->comm);
    delete c;
}
}  // namespace

extern "C" int mispec_rccl_unique_id(char out[128])
{
    return guarded([&] {
        MISPEC_REQUIRE(out, "mispec_rccl_unique_id: out is NULL");
        static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
        ncclUniqueId id;
        rccl_check(rccl().GetUniqueId(&id), "ncclGetUniqueId");
        std::memcpy(out, &id, 128);
    });
}

extern "C" int mispec_ctx_set_comm_rccl(mispec_ctx* ctx, int rank, int world, const char unique_id[128])
{
    return guarded([&] {
        MISPEC_REQUIRE(ctx && unique_id, "mispec_ctx_set_comm_rccl: NULL argument");
        MISPEC_REQUIRE(world >= 1 && rank >= 0 && rank < world, "mispec_ctx_set_comm_rccl: need 0 <= rank < world");
        ctx->make_current();
        ncclUniqueId id;
        std::memcpy(&id, unique_id, 128);
        auto* c = new RcclComm();
        try
        {
            rccl_check(rccl().CommInitRank(&c->comm, world, id, rank), "ncclCommInitRank");
        }
        catch (...)
        {
            delete c;
            throw;
        }
        if (ctx->comm_owner && ctx->comm_owner_free)
            ctx->comm_owner_free(ctx->comm_owner);
        ctx->comm_owner = c;
        ctx->comm_owner_free = rccl_free;
        c->rank = rank;
        c->world = world;
        const bool p2p = rccl().Send && rccl().Recv && rccl().GroupStart && rccl().GroupEnd;
        ctx->comm = mispec_comm{rank, world, rccl_allgather, rccl_allreduce, c, p2p ? rccl_exchange : nullptr};
    });
}

// ---------------------------------------------------------------------------------------------
// Loopback communicator: `world` host threads of one process, typically all on the same device.
// Used to exercise the sharded code path (partitioning, all-gather assembly, reductions) on a
// 1-GPU box.  Rendezvous through a mutex/condvar barrier; data moves with device-to-device copies.
// Correctness over speed: every collective drains the caller's stream first.
// ---------------------------------------------------------------------------------------------
struct mispec_loopback
{
    int world = 1;
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0;
    uint64_t generation = 0;
    std::vector<const double*> send;
    std::vector<const int64_t*> send_off, send_count;
    std::vector<double*> bufs;
    std::vector<int> devices;
    struct Endpoint
    {
        mispec_loopback* grp;
        int rank;
    };
    std::vector<Endpoint> endpoints;

    void barrier()
    {
        std::unique_lock<std::mutex> lk(mu);
        const uint64_t gen = generation;
        if (++arrived == world)
        {
            arrived = 0;
            generation++;
            cv.notify_all();
        }
        else
            cv.wait(lk, [&] { return generation != gen; });
    }
};

namespace {
int loopback_allgather(void* user, const double* send, double* recv, int64_t count, void* stream)
{
    return guarded([&] {
        auto* ep = static_cast<mispec_loopback::Endpoint*>(user);
        mispec_loopback* g = ep->grp;
        hipStream_t s = static_cast<hipStream_t>(stream);
        MISPEC_HIP(hipStreamSynchronize(s));
        g->send[ep->rank] = send;
        g->barrier();
        for (int r = 0; r < g->world; r++)
            MISPEC_HIP(hipMemcpyAsync(recv + int64_t(r) * count, g->send[r], size_t(count) * sizeof(double),
                                      hipMemcpyDeviceToDevice, s));
        MISPEC_HIP(hipStreamSynchronize(s));
        g->barrier();
    });
}
// pull model: every rank publishes its send buffer and tables, then copies what the peers address to it
int loopback_exchange(void* user, const double* send, const int64_t* send_off, const int64_t* send_count, double* recv,
                      const int64_t* recv_off, const int64_t* recv_count, void* stream)
{
    return guarded([&] {
        auto* ep = static_cast<mispec_loopback::Endpoint*>(user);
        mispec_loopback* g = ep->grp;
        hipStream_t s = static_cast<hipStream_t>(stream);
        MISPEC_HIP(hipStreamSynchronize(s));
        g->send[ep->rank] = send;
        g->send_off[ep->rank] = send_off;
        g->send_count[ep->rank] = send_count;
        g->barrier();
        for (int r = 0; r < g->world; r++)
        {
            if (r == ep->rank || recv_count[r] <= 0)
                continue;
            MISPEC_REQUIRE(g->send_count[r][ep->rank] == recv_count[r], "loopback exchange: send/recv counts disagree");
            MISPEC_HIP(hipMemcpyAsync(recv + recv_off[r], g->send[r] + g->send_off[r][ep->rank],
                                      size_t(recv_count[r]) * sizeof(double), hipMemcpyDeviceToDevice, s));
        }
        MISPEC_HIP(hipStreamSynchronize(s));
        g->barrier();
    });
}
int loopback_allreduce(void* user, double* buf, int64_t count, void* stream)
{
    return guarded([&] {
        auto* ep = static_cast<mispec_loopback::Endpoint*>(user);
        mispec_loopback* g = ep->grp;
        hipStream_t s = static_cast<hipStream_t>(stream);
        MISPEC_HIP(hipStreamSynchronize(s));
        g->bufs[ep->rank] = buf;
        g->barrier();
        std::vector<double> acc(size_t(count), 0.0), tmp(static_cast<size_t>(count));
        for (int r = 0; r < g->world; r++)  // fixed rank order => identical result on every rank
        {
            MISPEC_HIP(hipMemcpy(tmp.data(), g->bufs[r], size_t(count) * sizeof(double), hipMemcpyDeviceToHost));
            for (int64_t i = 0; i < count; i++)
                acc[size_t(i)] += tmp[size_t(i)];
        }
        g->barrier();  // everybody has read every buffer
        MISPEC_HIP(hipMemcpy(buf, acc.data(), size_t(count) * sizeof(double), hipMemcpyHostToDevice));
        g->barrier();
    });
}
}  // namespace

extern "C" int mispec_loopback_create(int world, mispec_loopback** out)
{
    return guarded([&] {
        MISPEC_REQUIRE(out && world >= 1, "mispec_loopback_create: bad argument");
        auto* g = new mispec_loopback();
        g->world = world;
        g->send.assign(size_t(world), nullptr);
        g->send_off.assign(size_t(world), nullptr);
        g->send_count.assign(size_t(world), nullptr);
        g->bufs.assign(size_t(world), nullptr);
        g->endpoints.resize(size_t(world));
        for (int r = 0; r < world; r++)
            g->endpoints[size_t(r)] = {g, r};
        *out = g;
    });
}

extern "C" int mispec_loopback_attach(mispec_loopback* grp, mispec_ctx* ctx, int rank)
{
    return guarded([&] {
        MISPEC_REQUIRE(grp && ctx && rank >= 0 && rank < grp->world, "mispec_loopback_attach: bad argument");
        ctx->comm = mispec_comm{rank, grp->world, loopback_allgather, loopback_allreduce, &grp->endpoints[size_t(rank)],
                                loopback_exchange};
    });
}

extern "C" int mispec_loopback_destroy(mispec_loopback* grp)
{
    return guarded([&] { delete grp; });
}
