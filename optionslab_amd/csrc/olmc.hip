// olmc.hip -- host side of libolmc.so: the C ABI declared in include/olmc.h.
//
// One context per HIP device (stream, workspace of the fused grid reduction,
// a pinned host landing buffer).  Every compute entry point is
//   host: derive the per-contract constants in fp64 (reference order)
//   device: ONE path kernel (its last workgroup writes the reduced sums) -> 8*NV bytes D2H
// and fails loudly when no HIP device is usable -- there is no CPU fallback.
#include "olmc.h"
#include "olmc_local_vol.h"
#include "olmc_local_vol_qmc.h"
#include "olmc_jump.h"
#include "olmc_sabr.h"
#include "olmc_sabr_qmc.h"
#include "olha.h"
#include "olmc_kernels.h"
#include "olmc_local_vol_kernels.h"
#include "olmc_local_vol_qmc_kernels.h"
#include "olmc_jump_kernels.h"
#include "olmc_sabr_kernels.h"
#include "olmc_jump_scenario_kernels.h"
#include "olmc_heston_american_kernels.h"
#include "olmc_sabr_qmc_kernels.h"
#include "olmc_job_board.h"
#include "olmc_device_mem.h"

#include <dlfcn.h>
#include <sched.h>
#include <time.h>
#include <hip/hip_ext.h>
#include <rccl/rccl.h>      // types and enum values only: the library itself is dlopen()ed on first multi-GPU use

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <condition_variable>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <mutex>
#include <optional>
#include <string>
#include <system_error>
#include <thread>
#include <vector>
#include <linux/futex.h>
#include <sys/prctl.h>
#include <sys/syscall.h>
#include <unistd.h>

namespace {

using namespace olmc;

thread_local std::string t_error = "";
thread_local int t_device = -1;

int fail(int code, const std::string& msg) {
    t_error = msg;
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(OLMC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));      \
    } while (0)

constexpr int kMaxDevices = 16;
constexpr int kMaxNV = 2 * OLMC_MAX_BATCH;       // values per workgroup row
constexpr int32_t kMaxGroups = kMaxGrid / kGroupBlocks + 1;
static_assert(kMaxGroups * kMaxNV == kGroupRowsCapacity, "device-side guard must match the group_rows allocation");
constexpr size_t kCounterBytes = sizeof(uint32_t) * (kMaxGroups + 1) * kCounterStride;      // a workspace slot's counters

using Mem = HipMem;

struct EventPair {
    hipEvent_t start, stop;
};

struct DeviceCtx {
    int device = -1;
    int cus = 0;
    hipStream_t stream = nullptr;
    // Reduction workspaces.  Each CALLER stream gets one of kSlots of them to itself (stream order guards it), so
    // independent pricings enqueued on DIFFERENT streams may overlap on the device (the tail of
    // one launch hides under the head of the next) without sharing rows or counters; a ninth, tenth ... stream shares
    // slots with the others, rotating and event-guarded.  Launches on the library's
    // OWN stream (every blocking entry point) use slot kSlots and no event at all: the stream is in-order, so a
    // launch finds the workspace free by construction -- and a blocking call is spared the two barrier packets
    // (hipStreamWaitEvent in front of the kernel, hipEventRecord behind it): ~1 us per call, measured.
    struct WsSlot {
        DeviceBlock<Mem> block_rows;   // doubles, grown on demand (grid x NV, at least 2^16)
        DeviceBlock<Mem> group_rows;   // [kMaxGroups][kMaxNV] doubles
        DeviceBlock<Mem> counters;     // [(kMaxGroups + 1) * kCounterStride] words, zero between launches (self-resetting)
        hipEvent_t done = nullptr;     // recorded after the slot's latest launch (shared slots only)
        bool used = false;
        bool claimed = false;          // `owner` (which may be the NULL stream) is the ONE caller stream that has used this slot so far:
        hipStream_t owner = nullptr;   // its launches need no event (stream order)
        bool shared = false;           // a second stream had to take the slot: event-guarded from then on
    };
    static constexpr int kSlots = 8;    // = the deepest overlap bench.py's `pipelined` pass asks for (--streams 8)
    WsSlot slots[kSlots + 1];
    int next_slot = 0, cur_slot = 0;
    // Completion by polling: a blocking call on the library stream arms done_flag (a word of the same pinned buffer) with a
    // fresh sequence number; the wave that writes the results raises it, and the host reads the results the moment it
    // sees the number instead of waiting for the kernel's completion signal to travel through the runtime.
    uint64_t* h_flag = nullptr;      // host view of the flag word
    uint64_t* d_flag = nullptr;      // device alias
    uint64_t seq = 0;                // last sequence number handed out
    uint64_t armed = 0;              // != 0: the launch just made raises h_flag to this value
    PinnedBlock<Mem> result;         // pinned + mapped [kMaxNV + 1 (+ flag)]: the last workgroup writes the sums straight to the host
    double* h_result = nullptr;      // view of `result`
    double* d_result = nullptr;      // its device alias (zero-copy: no D2H copy node, only a stream sync)
    DeviceBlock<Mem> bulk;           // terminal prices / path matrices / validation taps (bulk_reserve)
    // large results on their way home (copy_to_host): two pinned staging buffers, an event per buffer (allocated by the first large copy)
    PinnedBlock<Mem> stage[2];
    hipEvent_t stage_landed[2] = {nullptr, nullptr};
    BatchWorkspace<Mem, MultiOption, kMultiCounterStride> multi;      // independent-contract batches (olmc_european_multi)
    // the scrambled-Sobol table of the last QMC call, [dims x 30 direction numbers | dims shifts], keyed by its content: FD Greeks
    // and repeated pricings reuse one upload (qmc_table)
    CachedUpload<Mem> sobol;
    // the Brownian-bridge plan of the last bridge-constructed QMC path call, [n uint32 a | b << 16][3 x n doubles ca, cb, sd], keyed
    // by n: it depends on n_steps alone (qmc_bridge_plan)
    CachedUpload<Mem> bridge;
    DeviceBlock<Mem> heston_w;       // the bridge slabs of heston_qmc_kernel: [waves of the grid][2 n][64] doubles (heston_slabs); lv_qmc_price_kernel's [n][64]
    // the local-volatility table of the call in flight (olmc_local_vol.h), fp32 nodes, uploaded by every call: nothing reads it
    // after the lease ends (lv_upload)
    CachedUpload<Mem> lv;
    // "let the old users finish" for everything above but a shared workspace slot: they are all used on the context's own stream
    int drain() const { return Mem::wait(stream); }
    bool busy = false;                  // leased (guarded by the pool's mutex)
    // profiling
    std::vector<EventPair> ev_free, ev_pending;
    int64_t prof_launches = 0;
    double prof_ms = 0.0;
};

// Contexts of one device.  A call LEASES a context for its whole duration (CtxLease): it picks the first idle one under the pool's
// mutex -- a single-threaded caller therefore always works on context 0, exactly round 3's one-context library -- and everything
// after that (argument staging, launches, the wait for the result) runs outside any lock, on the context's own stream, workspace,
// pinned landing buffer and completion word.  Concurrent callers (Streamlit runs one thread per session, SURVEY §8b "Threading")
// get a context each, up to kMaxContexts per device (created on demand, never destroyed before olmc_shutdown); a further caller
// waits for a lease to come back.  Round 3 held ONE mutex around launch AND wait, so N sessions' pricings ran strictly one after
// the other, host launch overhead and device ramp / drain included.
constexpr int kMaxContexts = 8;

struct DevicePool {
    std::mutex mu;
    std::condition_variable idle;       // a lease came back
    std::vector<DeviceCtx*> all;        // grows to kMaxContexts, first idle first
    int device = -1;
};

std::mutex g_mu;                        // serialises the WRITERS of g_pool[] and g_default_device (olmc_init / olmc_shutdown);
std::atomic<DevicePool*> g_pool[kMaxDevices] = {};      // readers (every call's ctx_lease, possibly while another thread initialises a
std::atomic<int> g_default_device{-1};                  // device) take no lock
bool g_profile = false;

int no_users() { return 0; }            // the quiesce of a block allocated once, before anything can use it

int ctx_allocate(DeviceCtx* c) {
    HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    for (auto& sl : c->slots) {
        int rc = sl.group_rows.reserve(sizeof(double) * kMaxNV * kMaxGroups, no_users);
        if (!rc) rc = sl.counters.reserve(kCounterBytes, no_users);
        if (rc) return rc;
        HIP_TRY(hipMemset(sl.counters.get(), 0, kCounterBytes));
        HIP_TRY(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    }
    const int rc = c->result.reserve(sizeof(double) * (kMaxNV + 1 + 15), no_users, 0, 0, /*mapped=*/true);
    if (rc) return rc;
    c->h_result = c->result.as<double>();
    c->d_result = c->result.alias<double>();
    c->h_flag = reinterpret_cast<uint64_t*>(c->h_result + kMaxNV + 8);      // a cache line of its own
    c->d_flag = reinterpret_cast<uint64_t*>(c->d_result + kMaxNV + 8);
    *c->h_flag = 0;
    return OLMC_OK;
}

// Lets a context's work finish, destroys its events and stream (tolerates partially built contexts) and deletes it: its blocks free themselves.
void ctx_release(DeviceCtx* c) {
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (auto& ep : c->ev_pending) { (void)hipEventDestroy(ep.start); (void)hipEventDestroy(ep.stop); }
    for (auto& ep : c->ev_free) { (void)hipEventDestroy(ep.start); (void)hipEventDestroy(ep.stop); }
    for (hipEvent_t ev : c->stage_landed)
        if (ev) (void)hipEventDestroy(ev);
    for (auto& sl : c->slots)
        if (sl.done) (void)hipEventDestroy(sl.done);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int ctx_create(int device, DeviceCtx** out) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(OLMC_ERR_HIP, std::string("no HIP device available: ") + hipGetErrorString(e));
    if (device < 0 || device >= count || device >= kMaxDevices)
        return fail(OLMC_ERR_ARG, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    DeviceCtx* c = new DeviceCtx();
    c->device = device;
    c->cus = prop.multiProcessorCount;
    const int rc = ctx_allocate(c);
    if (rc) {                       // do not leak a half-built context
        ctx_release(c);
        return rc;
    }
    *out = c;
    return OLMC_OK;
}

// RAII lease of one context of the calling thread's device (see DevicePool).
struct CtxLease {
    DeviceCtx* c = nullptr;
    DevicePool* pool = nullptr;
    CtxLease() = default;
    CtxLease(const CtxLease&) = delete;
    CtxLease& operator=(const CtxLease&) = delete;
    ~CtxLease() { release(); }
    void release() {
        if (!c) return;
        {
            std::lock_guard<std::mutex> lock(pool->mu);
            c->busy = false;
        }
        // notify_all: the pool's one condition variable has two kinds of waiter (a lease, in ctx_lease_on; "every context idle", in
        // with_all_contexts) -- notify_one could hand the only wake-up to a waiter whose predicate is still false
        pool->idle.notify_all();
        c = nullptr;
    }
};

int ctx_lease_on(int dev, CtxLease* out) {
    DevicePool* pool = g_pool[dev].load(std::memory_order_acquire);
    if (!pool) return fail(OLMC_ERR_STATE, "device not initialised (call olmc_init)");
    HIP_TRY(hipSetDevice(dev));
    std::unique_lock<std::mutex> lock(pool->mu);
    for (;;) {
        for (DeviceCtx* c : pool->all)
            if (!c->busy) {
                c->busy = true;
                out->c = c;
                out->pool = pool;
                return OLMC_OK;
            }
        if (static_cast<int>(pool->all.size()) < kMaxContexts) {
            DeviceCtx* c = nullptr;
            const int rc = ctx_create(dev, &c);
            if (rc) return rc;
            c->busy = true;
            pool->all.push_back(c);
            out->c = c;
            out->pool = pool;
            return OLMC_OK;
        }
        pool->idle.wait(lock);
    }
}

int ctx_lease(CtxLease* out) {
    int dev = t_device >= 0 ? t_device : g_default_device.load(std::memory_order_acquire);
    if (dev < 0) {
        // lazy init on device 0 so a bare compute call still works (or fails loudly)
        int rc = olmc_init(0);
        if (rc) return rc;
        dev = t_device;
    }
    return ctx_lease_on(dev, out);
}

// The context's bulk buffer with room for `bytes`; a call that keeps several arrays there cuts them from `spans`, in order.
int bulk_reserve(DeviceCtx* c, size_t bytes, Carver* spans = nullptr) {
    const int rc = c->bulk.reserve(bytes, [c] { return c->drain(); });
    if (spans) *spans = c->bulk.carve();
    return rc;
}

// A large result (a path matrix: 100k x 252 doubles = 202 MB; a terminal array of 64M paths = 1 GB) on its way to the CALLER's buffer,
// which is pageable and, coming fresh from NumPy, not even faulted in.  One hipMemcpyAsync into it runs at 10-17 GB/s (round 4: 20 ms for
// the 202 MB): the runtime stages through pinned memory and ONE host thread copies every chunk out, paying every first-touch page
// fault on the way.  Here the device result leaves in 16 MB chunks by DMA into two pinned staging buffers (link rate: ~50 GB/s), and
// while chunk i + 1 is on the link, a handful of host threads copy chunk i out, a slice each -- so the page faults of the destination
// are taken in parallel too.  Work queued on c->stream before the call (the kernel that writes d_src) is ordered before the first DMA;
// the call returns when the last byte is in `dst`.  Bytes are copied, never interpreted: same array as the direct copy, bit for bit.
constexpr size_t kStageBytes = size_t(16) << 20, kStagedFrom = size_t(32) << 20;
int g_staged_copy = 0;       // OLMC_TUNE_STAGED_COPY: 0 = results of 32 MB and more come home through pinned staging buffers and parallel host
                             // copies (default), -1 = always one hipMemcpyAsync into the caller's buffer

int copy_to_host(DeviceCtx* c, void* dst, const void* d_src, size_t bytes) {
    if (bytes < kStagedFrom || g_staged_copy < 0) {
        HIP_TRY(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return OLMC_OK;
    }
    for (int i = 0; i < 2; ++i) {
        const int rc = c->stage[i].reserve(kStageBytes, no_users);
        if (rc) return rc;
        if (!c->stage_landed[i]) HIP_TRY(hipEventCreateWithFlags(&c->stage_landed[i], hipEventDisableTiming));
    }
    cpu_set_t cpus;
    int allowed = 4;
    if (sched_getaffinity(0, sizeof cpus, &cpus) == 0) allowed = CPU_COUNT(&cpus);
    const int n_threads = std::max(1, std::min(8, allowed / 2));
    const int64_t n_chunks = static_cast<int64_t>((bytes + kStageBytes - 1) / kStageBytes);
    std::atomic<int64_t> landed{0};                 // chunks whose DMA has completed: [0, landed) may be copied out
    std::atomic<int> copied[2] = {{0}, {0}};        // threads done with the chunk that sits in staging buffer 0 / 1
    std::atomic<bool> give_up{false};
    auto chunk_len = [&](int64_t i) { return std::min(kStageBytes, bytes - static_cast<size_t>(i) * kStageBytes); };
    auto worker = [&](int w) {
        for (int64_t i = 0; i < n_chunks; ++i) {
            for (uint32_t spins = 0; landed.load(std::memory_order_acquire) <= i; ++spins) {
                if (give_up.load(std::memory_order_relaxed)) return;
                if ((spins & 0xFF) == 0xFF) sched_yield(); else __builtin_ia32_pause();
            }
            const size_t len = chunk_len(i), per = (len / n_threads + 4095) & ~size_t(4095);      // page-sized slices: each page of dst has one toucher
            const size_t lo = std::min(len, per * w), hi = std::min(len, lo + per);
            if (hi > lo) std::memcpy(static_cast<char*>(dst) + static_cast<size_t>(i) * kStageBytes + lo, static_cast<const char*>(c->stage[i & 1].get()) + lo, hi - lo);
            copied[i & 1].fetch_add(1, std::memory_order_release);
        }
    };
    static const bool trace = std::getenv("OLMC_TRACE_COPY") != nullptr;
    using clock = std::chrono::steady_clock;
    auto us_since = [](clock::time_point t) { return std::chrono::duration<double, std::micro>(clock::now() - t).count(); };
    const auto t_begin = clock::now();
    double us_spawn = 0, us_first = 0, us_events = 0, us_workers = 0;
    std::vector<std::thread> threads;
    threads.reserve(n_threads);
    try {
        for (int w = 0; w < n_threads; ++w) threads.emplace_back(worker, w);
    } catch (const std::system_error&) {             // no thread to be had: the single copy still works
        give_up.store(true);
        for (std::thread& t : threads) t.join();
        HIP_TRY(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return OLMC_OK;
    }
    us_spawn = us_since(t_begin);
    hipError_t err = hipSuccess;
    for (int64_t i = 0; i < n_chunks && err == hipSuccess; ++i) {
        const int slot = static_cast<int>(i & 1);
        if (i >= 2) {                               // the chunk that sat in this buffer has been copied out by every thread
            const auto t = clock::now();
            for (uint32_t spins = 0; copied[slot].load(std::memory_order_acquire) < n_threads; ++spins)
                if ((spins & 0xFF) == 0xFF) sched_yield(); else __builtin_ia32_pause();
            copied[slot].store(0, std::memory_order_relaxed);
            us_workers += us_since(t);
        }
        err = hipMemcpyAsync(c->stage[slot].get(), static_cast<const char*>(d_src) + static_cast<size_t>(i) * kStageBytes, chunk_len(i), hipMemcpyDeviceToHost, c->stream);
        if (err == hipSuccess) err = hipEventRecord(c->stage_landed[slot], c->stream);
        if (err == hipSuccess && i >= 1) {
            const auto t = clock::now();
            err = hipEventSynchronize(c->stage_landed[slot ^ 1]);
            if (i == 1) us_first = us_since(t); else us_events += us_since(t);
            if (err == hipSuccess) landed.store(i, std::memory_order_release);
        }
    }
    {
        const auto t = clock::now();
        if (err == hipSuccess) err = hipEventSynchronize(c->stage_landed[(n_chunks - 1) & 1]);
        us_events += us_since(t);
    }
    if (err == hipSuccess) landed.store(n_chunks, std::memory_order_release);
    else give_up.store(true);
    const auto t_join = clock::now();
    for (std::thread& t : threads) t.join();
    if (trace)
        std::fprintf(stderr, "[olmc copy_to_host] %.1f MB, %lld chunks, %d threads: spawn %.0f us, first chunk landed (kernel + DMA) %.0f us, later event waits %.0f us, "
                             "waits for the copy threads %.0f us, last chunk out + join %.0f us, total %.0f us\n", bytes / 1e6, static_cast<long long>(n_chunks), n_threads,
                     us_spawn, us_first, us_events, us_workers, us_since(t_join), us_since(t_begin));
    if (err != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        (void)hipGetLastError();
        return fail(OLMC_ERR_HIP, std::string("copy_to_host: ") + hipGetErrorString(err));
    }
    return OLMC_OK;
}

// Tuning knob (olmc_tune): 0 = automatic.
int g_multi_launch = 0;      // OLMC_TUNE_MULTI_LAUNCH: 0 = multi-GPU calls queue their ranks from one launcher thread per device (default), -1 = serial
int g_grid_cap = 0;          // OLMC_TUNE_GRID_CAP: max workgroups of a launch whose kernel strides (0 = kMaxGrid, kQmcPathMaxGrid)
int g_qmc_block = 0;         // OLMC_TUNE_QMC_BLOCK: 0 = by size, 1 = always eight points per thread, -1 = never (and never split), 2 = always split
int g_poll = 0;              // OLMC_TUNE_POLL: 0 = blocking calls poll a host-mapped flag for completion (default), -1 = hipStreamSynchronize
int g_split_tail = 0;        // OLMC_TUNE_SPLIT_TAIL: 0 = split workgroups for the remainder of a European launch (default), -1 = never
int g_philox_table = 1;      // OLMC_TUNE_PHILOX_TABLE: 1 = European launches carry the Philox prefix table where one applies (default), 0 = never
int g_split_sat = 0;         // OLMC_TUNE_SPLIT_SAT: k > 0: a last round of fewer than k whole workgroups per CU is split too; 0 = never (default:
                             // measured, no gain -- see european_launch_shape)
#ifdef OLMC_WITH_PROBES      // the instrumented build (tools/probe/olmc_probe.hip -> libolmc_probe.so) only: test seams, see include/olmc_probe.h
int g_fault_shard = 0;       // OLMC_PROBE_TUNE_FAULT_SHARD: k > 0 makes rank k - 1 of a multi-GPU call fail before it launches
int g_force_nv = 0;          // OLMC_PROBE_TUNE_FORCE_NV: > 0 makes workspaces REPORT room for this many values per row (test of the device guard)
int g_multi_rehearsal = 0;   // OLMC_PROBE_TUNE_MULTI_REHEARSAL: != 0 runs the n ranks of a multi-GPU call on the caller's ONE device
int g_expect_table = 0;      // OLMC_PROBE_TUNE_EXPECT_TABLE: 1 / -1 = every European launch is expected to carry a / no Philox prefix table ...
std::atomic<int> g_expect_table_misses{0};   // ... and this counts the launches that did otherwise (reported and cleared when the knob is set again)
#endif

// Launch geometry: one workgroup per 256 paths, handed out by the hardware dispatcher
// (measured faster than a fixed 8-workgroups-per-CU grid-stride); beyond kMaxGrid
// workgroups the kernels grid-stride (olmc_host_math.h: path_grid, with the short paths' bound).
int32_t grid_for(int64_t n_paths, int32_t n_steps = INT32_MAX) { return path_grid(n_paths, n_steps, g_grid_cap); }

// Resident workgroups per compute unit of one kernel instantiation (register / LDS limited), asked of the runtime once.
template <typename Kernel>
int resident_workgroups(Kernel kernel) {
    static std::mutex mu;
    static std::vector<std::pair<const void*, int>> cache;
    const void* key = reinterpret_cast<const void*>(kernel);
    std::lock_guard<std::mutex> lock(mu);
    for (const auto& e : cache)
        if (e.first == key) return e.second;
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, kBlock, 0) != hipSuccess || nb < 1) {
        (void)hipGetLastError();
        nb = 1;
    }
    cache.emplace_back(key, nb);
    return nb;
}

// Launch shape of european_path_kernel for pr.count paths: returns the grid and sets pr->split_from.  When one workgroup
// per 256 paths covers the launch (no grid-striding) the first F workgroups own 256 paths each and the remaining paths go to
// split workgroups of 64 paths (four waves x a quarter of the steps each; see the kernel) -- unless the paths have fewer than
// four full fp32 groups (64 steps) to hand out.
//
// F = floor(W / C) C: every CU gets the same number of whole workgroups, the remainder is spread in quarter-length units.
// Round 3 asked whether a THIN last round of whole workgroups (1M paths = 15 per CU = 7 + 7 + 1 at 7 resident per CU) should be
// split too, on the theory that a lone wave per SIMD issues slowly.  It does not: exactly k C whole workgroups take
// 9.4 + 6.03 k us for every k from 1 to 28 (profiles/r03_occupancy_probe.jsonl) -- one wave per SIMD
// already issues at the full rate (four interleaved Philox blocks are enough ILP), the SIMD serves its waves oldest-first
// rather than in rounds (first workgroup of a 7-per-CU launch done after 9 us, last after 48: profiles/r03_phase_stamps.jsonl),
// and OLMC_TUNE_SPLIT_SAT at 2 / 5 / 7 left the 1M x 252 kernel at 100.35 us +- 0.1 (profiles/r03_ab_kernels.txt).  The knob
// stays for measurements; the default is off.
// keep_grid: the launch takes the default grid whatever OLMC_TUNE_GRID_CAP says (the fused Greeks, as the exotic fused Greeks do).
int32_t european_launch_shape(const DeviceCtx* c, PathRange* pr, int occ, bool keep_grid = false) {
    pr->split_from = INT32_MAX;
    const int grid_cap = keep_grid ? 0 : g_grid_cap;
    const int32_t grid = path_grid(pr->count, pr->n_steps, grid_cap);
    const int64_t wgs = (pr->count + kBlock - 1) / kBlock;
    if (g_split_tail < 0 || grid_cap != 0 || wgs != grid) return grid;           // tuned or grid-striding launches keep their shape
    if ((pr->n_steps >> 2) / kGroup < 4 || c->cus < 1) return grid;
    int64_t per_cu = (pr->count / kBlock) / c->cus;                                 // whole 256-path workgroups per CU
    if (occ >= 1 && g_split_sat > 0) {
        const int64_t r = per_cu % occ;
        if (r > 0 && r < std::min(g_split_sat, occ)) per_cu -= r;
    }
    const int64_t full = per_cu * c->cus;
    const int64_t rest = pr->count - full * kBlock;
    if (rest == 0) return grid;
    const int64_t split = (rest + kWave - 1) / kWave;
    if (full + split > kMaxGrid) return grid;
    pr->split_from = static_cast<int32_t>(full);
    return static_cast<int32_t>(full + split);
}

// The kernel launch_european<NSETS, MODE> will pick for a launch that covers every path (the only shape that splits).
template <int NSETS, int MODE>
int european_occupancy(bool anti) {
    if (g_split_sat <= 0) return 0;              // only the measurement knob needs it: nothing on the path of an ordinary call
    return anti ? resident_workgroups(european_path_kernel<NSETS, true, MODE, false>) : resident_workgroups(european_path_kernel<NSETS, false, MODE, false>);
}

// Workspace of the fused grid reduction for a launch of `grid` workgroups x nv values.
int make_ws(DeviceCtx* c, hipStream_t stream, int32_t grid, int nv, double* d_out, double tail, ReduceWs* ws) {
    const bool own = stream == c->stream;
    int idx = DeviceCtx::kSlots;
    if (!own) {
        // a caller stream keeps ONE slot to itself while there are slots to go round (bench.py's 8 streams, a rank's one stream):
        // its launches are ordered by the stream, no event needed.  Only when more streams than slots show up are slots shared,
        // rotating and event-guarded as before.
        idx = -1;
        for (int i = 0; i < DeviceCtx::kSlots && idx < 0; ++i)
            if (c->slots[i].claimed && !c->slots[i].shared && c->slots[i].owner == stream) idx = i;
        for (int i = 0; i < DeviceCtx::kSlots && idx < 0; ++i)
            if (!c->slots[i].claimed) { c->slots[i].claimed = true; c->slots[i].owner = stream; idx = i; }
        if (idx < 0) {
            idx = c->next_slot;
            c->next_slot = (c->next_slot + 1) % DeviceCtx::kSlots;
            DeviceCtx::WsSlot& taken = c->slots[idx];
            if (!taken.shared) {
                // its owner's launches so far carry no event: drain them once, then guard by events.  The owner is a CALLER's stream
                // and may have been destroyed since (a handle this library must not touch again: hipStreamSynchronize on a dead stream
                // is a use-after-free in the runtime, not an error code), so the whole device is drained -- once per slot, ever.
                HIP_TRY(hipDeviceSynchronize());
                taken.shared = true;
                taken.used = false;
            }
        }
    }
    DeviceCtx::WsSlot& sl = c->slots[idx];
    c->cur_slot = idx;
    const bool guarded = !own && sl.shared;
    const size_t need = static_cast<size_t>(grid) * nv;
    int rc = sl.block_rows.reserve(sizeof(double) * need, [&] {      // the slot's launches so far: its one stream's, or the event's
        if (!guarded) HIP_TRY(hipStreamSynchronize(stream));
        else if (sl.used) HIP_TRY(hipEventSynchronize(sl.done));
        return static_cast<int>(OLMC_OK);
    }, sizeof(double) << 16);
    if (rc) return rc;
    if (guarded && sl.used) HIP_TRY(hipStreamWaitEvent(stream, sl.done, 0));   // previous user of this shared slot, whatever its stream
    ws->block_rows = sl.block_rows.as<double>();
    ws->group_rows = sl.group_rows.as<double>();
    ws->counters = sl.counters.as<uint32_t>();
    ws->out = d_out;
    ws->tail = tail;
    ws->row_capacity = sl.block_rows.capacity() / sizeof(double);
#ifdef OLMC_WITH_PROBES
    if (g_force_nv > 0) ws->row_capacity = static_cast<uint64_t>(grid) * g_force_nv;        // the knob UNDER-reports (test of the guard)
#endif
    ws->done_flag = nullptr;
    ws->done_value = 0;
    c->armed = 0;
    if (own && d_out == c->d_result && g_poll >= 0) {      // a blocking call: results and flag land in the same pinned buffer
        c->armed = ++c->seq;
        ws->done_flag = c->d_flag;
        ws->done_value = c->armed;
    }
    return OLMC_OK;
}

// After a failed launch the self-resetting counters may be left dirty.
void ws_recover(DeviceCtx* c) {
    c->armed = 0;
    (void)hipDeviceSynchronize();
    (void)hipGetLastError();
    for (auto& sl : c->slots) (void)hipMemset(sl.counters.get(), 0, kCounterBytes);
}

// The same for the batch workspace (self-resetting ticket counters and the batch's done counter).
void multi_recover(DeviceCtx* c) {
    c->armed = 0;
    (void)hipDeviceSynchronize();
    (void)hipGetLastError();
    if (c->multi.counters()) (void)hipMemset(c->multi.counters(), 0, c->multi.counter_bytes());
}

// Call right after launching a kernel that uses the workspace handed out by make_ws.
int after_launch(DeviceCtx* c, hipStream_t stream) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { ws_recover(c); return fail(OLMC_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e)); }
    if (c->cur_slot == DeviceCtx::kSlots || !c->slots[c->cur_slot].shared) return OLMC_OK;    // one stream's own slot: stream order is the guard
    DeviceCtx::WsSlot& sl = c->slots[c->cur_slot];
    HIP_TRY(hipEventRecord(sl.done, stream));
    sl.used = true;
    return OLMC_OK;
}

// ---- profiling brackets ---------------------------------------------------
int prof_begin(DeviceCtx* c, hipStream_t s, EventPair* ep) {
    if (c->ev_free.empty()) {
        HIP_TRY(hipEventCreate(&ep->start));
        HIP_TRY(hipEventCreate(&ep->stop));
    } else {
        *ep = c->ev_free.back();
        c->ev_free.pop_back();
    }
    HIP_TRY(hipEventRecord(ep->start, s));
    return OLMC_OK;
}

// An event pair for a dispatch that carries its own timestamps (launch_one): nothing is recorded here.
int prof_acquire(DeviceCtx* c, EventPair* ep) {
    if (c->ev_free.empty()) {
        HIP_TRY(hipEventCreate(&ep->start));
        HIP_TRY(hipEventCreate(&ep->stop));
    } else {
        *ep = c->ev_free.back();
        c->ev_free.pop_back();
    }
    return OLMC_OK;
}

int prof_end(DeviceCtx* c, hipStream_t s, const EventPair& ep) {
    HIP_TRY(hipEventRecord(ep.stop, s));
    c->ev_pending.push_back(ep);
    return OLMC_OK;
}

int prof_drain(DeviceCtx* c) {
    for (const EventPair& ep : c->ev_pending) {
        float ms = 0.f;
        // a pair whose launch failed was never recorded: it is skipped, not an error of the measurement
        if (hipEventSynchronize(ep.stop) == hipSuccess && hipEventElapsedTime(&ms, ep.start, ep.stop) == hipSuccess) {
            c->prof_ms += ms;
            c->prof_launches += 1;
        } else {
            (void)hipGetLastError();
        }
        c->ev_free.push_back(ep);
    }
    c->ev_pending.clear();
    return OLMC_OK;
}

// make_contract, group_contracts, finish_stats, poisoned, log_level, nan_stats, GreeksSet, cv_finish and the moment combiners are
// pure host arithmetic: olmc_host_math.h (compiled on its own, under sanitizers, by tests/test_host_math_sanitizers.py).

int check_paths(int64_t path_offset, int64_t n_local, int32_t n_steps) {
    if (n_local < 1) return fail(OLMC_ERR_ARG, "n_paths must be >= 1");
    if (n_steps < 1) return fail(OLMC_ERR_ARG, "n_steps must be >= 1");
    if (path_offset < 0) return fail(OLMC_ERR_ARG, "path_offset must be >= 0");
    return OLMC_OK;
}

PathRange make_range(int64_t path_offset, int64_t n_local, int32_t n_steps, uint64_t seed) {
    PathRange pr;
    pr.first = static_cast<uint64_t>(path_offset);
    pr.count = n_local;
    pr.n_steps = n_steps;
    pr.key0 = static_cast<uint32_t>(seed);
    pr.key1 = static_cast<uint32_t>(seed >> 32);
    pr.split_from = INT32_MAX;
    return pr;
}

// `timed` != nullptr: the dispatch itself carries the event pair (hipExtLaunchKernelGGL): the events take the
// kernel's own begin / end timestamps, as rocprofv3 reads them.  hipEventRecord brackets around a launch also
// time the marker packets on either side (+7..10 us at these durations: 119 vs 109 us in one and the same run).
template <typename Kernel, typename... Args>
void launch_timed(Kernel kernel, dim3 grid, dim3 block, hipStream_t s, const EventPair* timed, const Args&... args) {
    if (timed) hipExtLaunchKernelGGL(kernel, grid, block, 0, s, timed->start, timed->stop, 0, args...);
    else hipLaunchKernelGGL(kernel, grid, block, 0, s, args...);
}

// Compile-time dispatch on a runtime flag: f(std::true_type{}) or f(std::false_type{}), so that one generic lambda names the
// kernel instantiation of either value (kernel<B> with `auto B`).
template <typename F>
void with_bool(bool b, F&& f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// The same over a fused set's width and the antithetic flag: f(integral_constant<int, 8 or 16>, integral_constant<bool, anti>).
template <typename F>
void with_set_anti(int nsets, bool anti, F&& f) {
    with_bool(nsets == 8, [&](auto eight) { with_bool(anti, [&](auto a) { f(std::integral_constant<int, eight ? 8 : 16>{}, a); }); });
}

// Profiling on: take an event pair for the launch that follows and queue it for prof_drain.
int prof_pair(DeviceCtx* c, EventPair* ep, const EventPair** timed) {
    *timed = nullptr;
    if (!g_profile) return OLMC_OK;
    int rc = prof_acquire(c, ep);
    if (rc) return rc;
    c->ev_pending.push_back(*ep);
    *timed = ep;
    return OLMC_OK;
}

// The Philox prefix table of a European launch (PhiloxPrefix, olmc_host_math.h), or none (n_blocks = 0: the kernel's own ten rounds).
// A table needs a grid that covers every path (the strided form walks several paths per thread and keeps its loop), room for every
// block of a path, the trailing partial one included, and ONE high path word for the whole launch.
PhiloxPrefix european_prefix(const PathRange& pr, bool strided) {
    PhiloxPrefix pp;
    const int32_t blocks = (pr.n_steps + 3) / 4;
    const uint64_t last = pr.first + static_cast<uint64_t>(pr.count) - 1;
    const bool table = g_philox_table != 0 && !strided && blocks <= kPrefixBlocks && (last >> 32) == (pr.first >> 32);
    philox_prefix(static_cast<uint64_t>(pr.key0) | static_cast<uint64_t>(pr.key1) << 32, static_cast<uint32_t>(pr.first >> 32), 0u, table ? blocks : 0, &pp);
    return pp;
}

template <int NSETS, int MODE>
void launch_european(bool anti, int32_t grid, hipStream_t s, const PathRange& pr, const ContractSet<NSETS>& cs,
                     const ReduceWs& ws, double* terminal, const EventPair* timed = nullptr) {
    const bool strided = static_cast<int64_t>(grid) * kBlock < pr.count;      // the grid does not cover every path
    const PhiloxPrefix pp = european_prefix(pr, strided);
#ifdef OLMC_WITH_PROBES
    if (g_expect_table != 0 && (g_expect_table > 0) != (pp.n_blocks != 0)) g_expect_table_misses.fetch_add(1, std::memory_order_relaxed);
#endif
    auto launch = [&](auto strided_c, auto a) {
        launch_timed(european_path_kernel<NSETS, a, MODE, strided_c>, dim3(grid), dim3(kBlock), s, timed, pr, cs, ws, terminal, pp);
    };
    // kSumOnly exists only where the grid covers every path (run_batch_device asks for it nowhere else)
    if constexpr (MODE == kSumOnly) with_bool(anti, [&](auto a) { launch(std::false_type{}, a); });
    else with_bool(strided, [&](auto strided_c) { with_bool(anti, [&](auto a) { launch(strided_c, a); }); });
}

// Waits for the launch just made on stream s (defined with the poll below).
int sync_or_recover(DeviceCtx* c, hipStream_t s);

// ONE reducing launch on a context the caller holds (a lease, or a multi-GPU rank's own): the workspace of `grid` workgroups x nv
// values, whose last workgroup writes the sums to d_out (and `tail` behind them when tail >= 0), an event pair when profiling is on
// (unless !profiled), launch(grid, s, timed, ws), the launch check.  The launch that writes into the context's pinned buffer (d_out == c->d_result) BLOCKS: on OLMC_OK the sums
// are in c->h_result.  Any other d_out is a shard's device buffer, and its launch is left queued on `s`.
template <typename Launch>
int launch_reduce(DeviceCtx* c, hipStream_t s, double* d_out, double tail, int nv, int32_t grid, Launch&& launch, bool profiled = true) {
    ReduceWs ws;
    int rc = make_ws(c, s, grid, nv, d_out, tail, &ws);
    if (rc) return rc;
    EventPair ep{};
    const EventPair* timed = nullptr;
    if (profiled) {
        rc = prof_pair(c, &ep, &timed);
        if (rc) return rc;
    }
    launch(grid, s, timed, ws);
    rc = after_launch(c, s);
    if (rc || d_out != c->d_result) return rc;
    return sync_or_recover(c, s);
}

// The stats of one contract from {sum, sumsq} at h; poisoned inputs (`bad`) answer NaN (nan_stats overwrites every field).
void finish_one(const double* h, int64_t n, double r_disc, double T, bool bad, olmc_stats* out) {
    if (bad) nan_stats(n, out);
    else finish_stats(h[0], h[1], n, r_disc, T, out);
}

// The stats of k contracts from one launch's sums: contract i's pair sits at slot pos[i] (pos == nullptr: slot i); a lean launch
// left one sum per slot and no sum of squares.  Poisoned contracts, or all of them when extra_bad, answer NaN.
void finish_set(const double* h, const int* pos, int64_t n, const olmc_option* opts, int64_t k, bool extra_bad, bool lean, olmc_stats* st) {
    for (int64_t i = 0; i < k; ++i) {
        const int64_t slot = pos ? pos[i] : i;
        const olmc_option& o = opts[i];
        if (extra_bad || poisoned(o.S, o.K, o.T, o.r, o.sigma, o.q)) nan_stats(n, &st[i]);
        else if (lean) finish_stats(h[slot], std::nan(""), n, o.r, o.T, &st[i]);      // the price is exact, the standard error was not asked for
        else finish_stats(h[2 * slot], h[2 * slot + 1], n, o.r, o.T, &st[i]);
    }
}

// The per-step constants of a GBM path recursion (exotic_options.py:54-56, gbm_numpy.py:106-108, gbm_qmc.py:38-44).
struct GbmStep {
    double dt, drift, vol;
};
GbmStep gbm_step(double T, int32_t n_steps, double r, double q, double sigma) {
    const double dt = T / n_steps;
    return {dt, (r - q - 0.5 * sigma * sigma) * dt, sigma * std::sqrt(dt)};
}

// ONE launch on stream `s` for k contracts: leaves {sum, sumsq} x k in d_out[0 .. 2k)
// (padded to the kernel's NSETS) and, when tail >= 0, `tail` in d_out[2 * nsets].  Blocks when d_out is c->d_result (launch_reduce).
int run_batch_device(DeviceCtx* c, hipStream_t s, const olmc_option* opts, int32_t k, int64_t path_offset,
                     int64_t n_local, int32_t n_steps, uint64_t seed, int antithetic, double* d_out, double tail,
                     int* pos /* [k]: slot of contract i in d_out, may be NULL when k == 1 */, bool profiled, bool* sums_only = nullptr
                     /* in: the caller needs no sums of squares; out: the launch made left ONE sum per slot (d_out[slot]) */,
                     bool keep_grid = false /* european_launch_shape's */) {
    PathRange pr = make_range(path_offset, n_local, n_steps, seed);
    const bool anti = antithetic != 0;
    const int nsets = k == 1 ? 1 : (k <= 8 ? 8 : 16);
    const int occ = nsets == 1 ? european_occupancy<1, kReduce>(anti) : (nsets == 8 ? european_occupancy<8, kReduce>(anti) : european_occupancy<16, kReduce>(anti));
    const int32_t grid = european_launch_shape(c, &pr, occ, keep_grid);
    // prices only (finite-difference Greeks without their evaluations' standard errors): the sum-only form of the fused kernels,
    // where the launch covers every path
    const bool lean = sums_only && *sums_only && nsets > 1 && static_cast<int64_t>(grid) * kBlock >= n_local;
    if (sums_only) *sums_only = lean;
    return launch_reduce(c, s, d_out, tail, lean ? nsets : 2 * nsets, grid, [&](int32_t g, hipStream_t st, const EventPair* timed, const ReduceWs& ws) {
        auto fused = [&](auto width) {
            ContractSet<width> cs;
            group_contracts<width>(opts, k, n_steps, &cs, pos);
            if (!lean) launch_european<width, kReduce>(anti, g, st, pr, cs, ws, nullptr, timed);
            else launch_european<width, kSumOnly>(anti, g, st, pr, cs, ws, nullptr, timed);
        };
        if (nsets == 1) {
            ContractSet<1> cs;
            cs.c[0] = make_contract(opts[0], n_steps);
            cs.base_mask = 1u; cs.upper_continues_slot0 = 0;
            if (pos) pos[0] = 0;
            launch_european<1, kReduce>(anti, g, st, pr, cs, ws, nullptr, timed);
        } else if (nsets == 8) {
            fused(std::integral_constant<int, 8>{});
        } else {
            fused(std::integral_constant<int, 16>{});
        }
    }, profiled);
}

// Waits for the launch just made on stream s.  If it was armed (make_ws), the host polls the flag word in pinned memory:
// the results are there as soon as the flag shows the launch's sequence number.  The stream itself is left to drain on its
// own (it is in-order, so the next launch still starts after this kernel has retired).
// The poll is a spin only for as long as a spin is cheap: the first kSpinUs (200 us: every interactive size, the 1M x 252
// headline at 100 us) spin with `pause`; from then on every poll is followed by sched_yield(), so a host thread waiting for a
// 6 ms pricing of 64M paths hands its core to any other runnable thread (Streamlit runs one thread per session) instead of
// burning it; after kYieldUs (2 ms) the polls are kSleepUs apart (nanosleep at a 1 us timer slack: < 1 % on anything that long; the calling thread's
// CPU share over a 6 ms pricing falls from 1.0 to 0.34, profiles/r03_call_overhead.jsonl).  Insurance: from 2 ms on the stream
// is queried as well, about once a millisecond -- an error is reported as such, and a stream that reports completion without
// the flag having shown up falls back to the runtime's own wait.
constexpr int64_t kSpinUs = 200, kYieldUs = 2000, kSleepUs = 20;

// A nanosleep() wakes up to the thread's timer slack late -- 50 us by default, as long again as the nap asked for: a 2.3 ms pricing
// came back 0.16 ms after its kernel had ended.  While a call naps its thread's slack is 1 us (restored on the way out).
struct TimerSlack {
    long old = -1;
    void tighten() {
        if (old >= 0) return;
        old = prctl(PR_GET_TIMERSLACK, 0, 0, 0, 0);
        if (old >= 0 && prctl(PR_SET_TIMERSLACK, 1000UL, 0, 0, 0) != 0) old = -1;
    }
    ~TimerSlack() {
        if (old >= 0) (void)prctl(PR_SET_TIMERSLACK, static_cast<unsigned long>(old), 0, 0, 0);
    }
};

int wait_armed(DeviceCtx* c, hipStream_t s) {
    if (c->armed != 0) {
        const uint64_t want = c->armed;
        c->armed = 0;
        using clock = std::chrono::steady_clock;
        const auto t0 = clock::now();
        bool queried = false;
        int phase = 0;                                                           // 0 spin, 1 yield, 2 sleep + query
        TimerSlack slack;
        for (uint32_t spins = 0;; ++spins) {
            if (__atomic_load_n(c->h_flag, __ATOMIC_ACQUIRE) == want) {
                if (queried) (void)hipGetLastError();                        // a hipErrorNotReady answer must not linger as this thread's last error
                return OLMC_OK;
            }
            if (phase == 0) {
                __builtin_ia32_pause();
                if ((spins & 0x3F) == 0x3F && clock::now() - t0 >= std::chrono::microseconds(kSpinUs)) phase = 1;
                continue;
            }
            if (phase == 1) {
                sched_yield();
                if ((spins & 0xF) == 0xF && clock::now() - t0 >= std::chrono::microseconds(kYieldUs)) phase = 2;
                continue;
            }
            if ((spins & 0x3F) == 0) {                                       // the stream is asked every 64th nap (~1.5 ms), the word every time
                const hipError_t q = hipStreamQuery(s);
                queried = true;
                if (q == hipSuccess) break;                                  // retired: fall through to the runtime's wait
                if (q != hipErrorNotReady) {
                    ws_recover(c);
                    return fail(OLMC_ERR_HIP, std::string("hipStreamQuery: ") + hipGetErrorString(q));
                }
            }
            slack.tighten();
            const timespec nap{0, kSleepUs * 1000};
            nanosleep(&nap, nullptr);
        }
        (void)hipGetLastError();
    }
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) { ws_recover(c); return fail(OLMC_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e)); }
    return OLMC_OK;
}

int sync_or_recover(DeviceCtx* c, hipStream_t s) {
    if (s != c->stream) c->armed = 0;               // only launches on the library's own stream are ever armed
    return wait_armed(c, s);
}

int run_batch(const olmc_option* opts, int32_t k, int64_t path_offset, int64_t n_local, int32_t n_steps,
              uint64_t seed, int antithetic, olmc_stats* out, bool prices_only = false, bool keep_grid = false) {
    if (!opts || !out) return fail(OLMC_ERR_ARG, "null pointer");
    if (k < 1 || k > OLMC_MAX_BATCH) return fail(OLMC_ERR_ARG, "batch size must be in [1, OLMC_MAX_BATCH]");
    int rc = check_paths(path_offset, n_local, n_steps);
    if (rc) return rc;
    CtxLease lease;
    rc = ctx_lease(&lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    int pos[OLMC_MAX_BATCH];
    bool lean = prices_only;
    rc = run_batch_device(c, c->stream, opts, k, path_offset, n_local, n_steps, seed, antithetic, c->d_result, -1.0, pos, true, &lean, keep_grid);
    if (rc) return rc;
    finish_set(c->h_result, pos, n_local * (antithetic ? 2 : 1), opts, k, false, lean, out);
    return OLMC_OK;
}

}  // namespace

namespace { void multi_gpu_release(); }      // the multi-GPU engine's streams, buffers and communicators (defined with it)

int olmc::device_mem_fail(hipError_t e, const char* call) { return fail(OLMC_ERR_HIP, std::string(call) + ": " + hipGetErrorString(e)); }

// =============================================================== lifetime ====
extern "C" int olmc_abi_version(void) { return OLMC_ABI_VERSION; }

extern "C" const char* olmc_last_error(void) { return t_error.c_str(); }

extern "C" int olmc_init(int device) {
    std::lock_guard<std::mutex> lock(g_mu);
    // operational safety valves (no rebuild, no code change in the host): OLMC_POLL=0 makes blocking calls wait with
    // hipStreamSynchronize, OLMC_SPLIT_TAIL=0 keeps one launch shape throughout -- the same switches olmc_tune offers
    static const bool env_read = [] {
        const char* p = std::getenv("OLMC_POLL");
        if (p && p[0] == '0') g_poll = -1;
        const char* t = std::getenv("OLMC_SPLIT_TAIL");
        if (t && t[0] == '0') g_split_tail = -1;
        const char* m = std::getenv("OLMC_MULTI_LAUNCH");          // "serial": the multi-GPU entry points queue their ranks from the calling thread
        if (m && m[0] == 's') g_multi_launch = -1;
        const char* sc = std::getenv("OLMC_STAGED_COPY");          // "0": large results come home by one hipMemcpyAsync
        if (sc && sc[0] == '0') g_staged_copy = -1;
        return true;
    }();
    (void)env_read;
    if (device < 0 || device >= kMaxDevices) return fail(OLMC_ERR_ARG, "device index out of range");
    if (!g_pool[device].load(std::memory_order_acquire)) {
        DeviceCtx* c = nullptr;
        int rc = ctx_create(device, &c);            // the first context of the device: a device that cannot be used fails HERE, loudly
        if (rc) return rc;
        DevicePool* pool = new DevicePool();
        pool->device = device;
        pool->all.push_back(c);
        g_pool[device].store(pool, std::memory_order_release);
    } else {
        HIP_TRY(hipSetDevice(device));
    }
    t_device = device;
    if (g_default_device.load() < 0) g_default_device.store(device, std::memory_order_release);
    return OLMC_OK;
}

extern "C" int olmc_shutdown(void) {
    std::lock_guard<std::mutex> lock(g_mu);
    multi_gpu_release();
    for (int d = 0; d < kMaxDevices; ++d) {         // the caller's contract: no call is in flight on any thread
        DevicePool* pool = g_pool[d].load();
        if (!pool) continue;
        const bool usable = hipSetDevice(d) == hipSuccess;
        for (DeviceCtx* c : pool->all) {
            if (usable) ctx_release(c);
            else delete c;
        }
        delete pool;
        g_pool[d].store(nullptr);
    }
    g_default_device.store(-1);
    t_device = -1;
    return OLMC_OK;
}

extern "C" int olmc_device_info(olmc_devinfo* out) {
    if (!out) return fail(OLMC_ERR_ARG, "null pointer");
    CtxLease lease;
    int rc = ctx_lease(&lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, c->device));
    std::memset(out, 0, sizeof(*out));
    std::snprintf(out->name, sizeof(out->name), "%s", prop.name);
    std::snprintf(out->arch, sizeof(out->arch), "%s", prop.gcnArchName);
    out->compute_units = prop.multiProcessorCount;
    out->clock_mhz = prop.clockRate / 1000;
    out->wavefront = prop.warpSize;
    out->device = c->device;
    out->hbm_bytes = static_cast<int64_t>(prop.totalGlobalMem);
    return OLMC_OK;
}

// ===================================================== European reductions ====
extern "C" int olmc_european(double S, double K, double T, double r, double sigma, double q, int is_call,
                             int64_t n_paths, int32_t n_steps, uint64_t seed, int antithetic, olmc_stats* out) {
    const olmc_option o = make_option(S, K, T, r, sigma, q, is_call);
    return run_batch(&o, 1, 0, n_paths, n_steps, seed, antithetic, out);
}

extern "C" int olmc_european_shard(double S, double K, double T, double r, double sigma, double q, int is_call,
                                   int64_t path_offset, int64_t n_local, int32_t n_steps, uint64_t seed,
                                   int antithetic, olmc_stats* out) {
    const olmc_option o = make_option(S, K, T, r, sigma, q, is_call);
    return run_batch(&o, 1, path_offset, n_local, n_steps, seed, antithetic, out);
}

extern "C" int olmc_european_shard_dev(double S, double K, double T, double r, double sigma, double q, int is_call,
                                       int64_t path_offset, int64_t n_local, int32_t n_steps, uint64_t seed,
                                       int antithetic, double* d_triple, void* hip_stream) {
    if (!d_triple) return fail(OLMC_ERR_ARG, "null pointer");
    int rc = check_paths(path_offset, n_local, n_steps);
    if (rc) return rc;
    CtxLease lease;
    rc = ctx_lease(&lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);   // used as given: NULL is the HIP null stream
    const olmc_option o = make_option(S, K, T, r, sigma, q, is_call);
    const double n = static_cast<double>(n_local * (antithetic ? 2 : 1));
    // the path kernel's last workgroup writes {sum, sumsq, n} straight into the caller's buffer
    return run_batch_device(c, s, &o, 1, path_offset, n_local, n_steps, seed, antithetic, d_triple, n, nullptr, true);
}

// Blocking fetch of n (<= 33) doubles that work already queued on stream s leaves at d_src (e.g. the triple after an all-reduce):
// a one-wave kernel behind that work copies them into c's pinned buffer and raises c's completion word, the host polls it -- the
// same hand-over as a blocking pricing, instead of hipMemcpyAsync + hipStreamSynchronize (8 us -> 3 us per step).
namespace {
int fetch_dev(DeviceCtx* c, const double* d_src, int32_t n, hipStream_t s, double* out_host) {
    const uint64_t want = ++c->seq;
    hipLaunchKernelGGL(publish_kernel, dim3(1), dim3(kWave), 0, s, d_src, n, c->d_result, c->d_flag, want);
    HIP_TRY(hipGetLastError());
    int rc = OLMC_OK;
    if (g_poll >= 0) {
        c->armed = want;
        rc = wait_armed(c, s);
    } else {
        hipError_t e = hipStreamSynchronize(s);
        if (e != hipSuccess) rc = fail(OLMC_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    }
    if (rc) return rc;
    for (int32_t i = 0; i < n; ++i) out_host[i] = c->h_result[i];
    return OLMC_OK;
}
}  // namespace

// The fetch on the caller's stream (one process per GPU: the triple after the caller's RCCL all-reduce), through a leased context.
extern "C" int olmc_fetch_dev(const double* d_src, int32_t n, void* hip_stream, double* out_host) {
    if (!d_src || !out_host) return fail(OLMC_ERR_ARG, "null pointer");
    if (n < 1 || n > kMaxNV + 1) return fail(OLMC_ERR_ARG, "n must be in [1, 33]");
    CtxLease lease;
    int rc = ctx_lease(&lease);
    if (rc) return rc;
    return fetch_dev(lease.c, d_src, n, static_cast<hipStream_t>(hip_stream), out_host);
}

extern "C" int olmc_european_batch(const olmc_option* opts, int32_t k, int64_t path_offset, int64_t n_local,
                                   int32_t n_steps, uint64_t seed, int antithetic, olmc_stats* out) {
    return run_batch(opts, k, path_offset, n_local, n_steps, seed, antithetic, out);
}

extern "C" int olmc_combine_stats(const olmc_stats* parts, int32_t n_parts, double r, double T, olmc_stats* out) {
    if (!parts || !out || n_parts < 1) return fail(OLMC_ERR_ARG, "bad arguments");
    if (!combine_stats(parts, n_parts, r, T, out)) return fail(OLMC_ERR_ARG, "no samples");     // fixed rank order => bitwise stable
    return OLMC_OK;
}

// ==================================================== independent contracts ====
extern "C" int olmc_european_multi(const olmc_option* opts, const uint32_t* tags, int64_t n_options, int64_t n_paths,
                                   int32_t n_steps, uint64_t seed, int antithetic, olmc_stats* out) {
    if (!opts || !out) return fail(OLMC_ERR_ARG, "null pointer");
    if (n_options < 1) return fail(OLMC_ERR_ARG, "n_options must be >= 1");
    if (n_options > (int64_t(1) << 31) - 2) return fail(OLMC_ERR_ARG, "too many contracts in one call");
    int rc = check_paths(0, n_paths, n_steps);
    if (rc) return rc;
    CtxLease lease;
    rc = ctx_lease(&lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    const int32_t bpo = static_cast<int32_t>(std::min<int64_t>((n_paths + kBlock - 1) / kBlock, 1024));   // workgroups per contract
    // the batch workspace (BatchWorkspace): contracts go up by one asynchronous DMA from pinned memory, the sums are written into
    // pinned memory by the kernel itself, completion is the polled word of the context
    decltype(c->multi)::Views v;
    rc = c->multi.reserve(static_cast<size_t>(n_options), static_cast<size_t>(bpo), c->stream, &v);
    if (rc) return rc;
    MultiOption* const h = v.h_opts;
    for (int64_t j = 0; j < n_options; ++j) {
        const Contract ct = make_contract(opts[j], n_steps);
        h[j].a = ct.a; h[j].vol = ct.vol; h[j].strike = ct.strike; h[j].sign = ct.sign;
        h[j].tag = tags ? tags[j] : static_cast<uint32_t>(j);
        h[j].pad = 0;
    }
    HIP_TRY(hipMemcpyAsync(v.d_opts, h, sizeof(MultiOption) * n_options, hipMemcpyHostToDevice, c->stream));
    MultiDone md;
    md.done_count = v.d_done;
    md.n_total = static_cast<uint32_t>(n_options);
    md.done_flag = nullptr;
    md.done_value = 0;
    c->armed = 0;
    if (g_poll >= 0) {
        c->armed = ++c->seq;
        md.done_flag = c->d_flag;
        md.done_value = c->armed;
    }
    const PathRange pr = make_range(0, n_paths, n_steps, seed);
    EventPair ep{};
    if (g_profile) { rc = prof_begin(c, c->stream, &ep); if (rc) return rc; }
    for (int64_t base_opt = 0; base_opt < n_options; base_opt += 65535) {
        const unsigned ny = static_cast<unsigned>(std::min<int64_t>(65535, n_options - base_opt));
        with_bool(antithetic != 0, [&](auto a) { launch_timed(european_multi_kernel<a>, dim3(bpo, ny), dim3(kBlock), c->stream, nullptr, pr, v.d_opts, base_opt, v.d_rows, v.d_cnt, v.d_out, md); });
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            multi_recover(c);
            return fail(OLMC_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
        }
    }
    if (g_profile) { rc = prof_end(c, c->stream, ep); if (rc) { multi_recover(c); return rc; } }
    rc = wait_armed(c, c->stream);
    if (rc) { multi_recover(c); return rc; }
    finish_set(v.h_out, nullptr, n_paths * (antithetic ? 2 : 1), opts, n_options, false, false, out);
    return OLMC_OK;
}

// The layout olmc_european_batch / olmc_european_greeks_fd give a set of k contracts (pure host arithmetic: needs no device).
extern "C" int olmc_contract_layout(const olmc_option* opts, int32_t k, int32_t n_steps, int32_t* nsets_out, int32_t* pos, uint32_t* base_mask,
                                    int32_t* upper_continues_slot0, double* scale16) {
    if (!opts || !nsets_out || !pos || !base_mask || !upper_continues_slot0 || !scale16) return fail(OLMC_ERR_ARG, "null pointer");
    if (k < 2 || k > OLMC_MAX_BATCH) return fail(OLMC_ERR_ARG, "a set has 2 .. OLMC_MAX_BATCH contracts");
    if (n_steps < 1) return fail(OLMC_ERR_ARG, "n_steps must be >= 1");
    contract_layout(opts, k, n_steps, nsets_out, pos, base_mask, upper_continues_slot0, scale16);
    return OLMC_OK;
}

// Capacity of the batch workspace as it stands: {contracts, workgroups per contract} (0, 0 before the first batch).
extern "C" int olmc_multi_capacity(int64_t* out2) {
    if (!out2) return fail(OLMC_ERR_ARG, "null pointer");
    CtxLease lease;
    int rc = ctx_lease(&lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    out2[0] = static_cast<int64_t>(c->multi.capacity());
    out2[1] = static_cast<int64_t>(c->multi.rows_per_contract());
    return OLMC_OK;
}

// ================================================== finite-difference Greeks ====
// GreeksSet (olmc_host_math.h): the evaluations of compute_greeks_unified (unified_greeks.py:274-277, 295-358) in the reference's
// get_price() call order, and the finite differences over their prices.
extern "C" int olmc_european_greeks_fd(double S, double K, double T, double r, double sigma, double q, int is_call,
                                       int64_t n_paths, int32_t n_steps, uint64_t seed, int second_order,
                                       double* out9, olmc_stats* evals) {
    if (!out9) return fail(OLMC_ERR_ARG, "null pointer");
    if (!(T > 0.0)) return fail(OLMC_ERR_ARG, "T must be > 0 (price() returns intrinsic value without simulating)");
    const GreeksSet gs(S, K, T, r, sigma, q, is_call, second_order);
    olmc_stats st[OLMC_MAX_BATCH];
    int rc = run_batch(gs.o, gs.k, 0, n_paths, n_steps, seed, 1, st, /*prices_only=*/evals == nullptr, /*keep_grid=*/true);     // no evaluations asked for: no sums of squares
    if (rc) return rc;
    gs.finish(st, T, out9, evals);
    return OLMC_OK;
}

// ============================================================ terminal array ====
extern "C" int olmc_european_terminal(double S, double T, double r, double sigma, double q, int64_t n_paths,
                                      int32_t n_steps, uint64_t seed, int antithetic, double* out_host) {
    if (!out_host) return fail(OLMC_ERR_ARG, "null pointer");
    int rc = check_paths(0, n_paths, n_steps);
    if (rc) return rc;
    CtxLease lease;
    rc = ctx_lease(&lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    const size_t bytes = sizeof(double) * static_cast<size_t>(n_paths) * (antithetic ? 2 : 1);
    rc = bulk_reserve(c, bytes);
    if (rc) return rc;
    PathRange pr = make_range(0, n_paths, n_steps, seed);
    const int32_t grid = european_launch_shape(c, &pr, european_occupancy<1, kTerminal>(antithetic != 0));
    ContractSet<1> cs;
    cs.c[0] = make_contract(make_option(S, 0.0, T, r, sigma, q, 1), n_steps);
    cs.base_mask = 1u; cs.upper_continues_slot0 = 0;
    ReduceWs ws{};   // unused in kTerminal mode
    launch_european<1, kTerminal>(antithetic != 0, grid, c->stream, pr, cs, ws, c->bulk.as<double>());
    HIP_TRY(hipGetLastError());
    return copy_to_host(c, out_host, c->bulk.get(), bytes);
}

// =========================================================== control variate ====
namespace {
// ONE launch of the five control-variate moments (of the UNdiscounted payoff) of contract o, then `tail`, at d_out (launch_reduce).
int cv_device(DeviceCtx* c, hipStream_t s, const olmc_option& o, int64_t path_offset, int64_t n_local, int32_t n_steps, uint64_t seed,
              int antithetic, double* d_out, double tail, bool profiled) {
    PathRange pr = make_range(path_offset, n_local, n_steps, seed);
    const int32_t grid = european_launch_shape(c, &pr, european_occupancy<1, kControlVariate>(antithetic != 0));
    ContractSet<1> cs;
    cs.c[0] = make_contract(o, n_steps);
    cs.base_mask = 1u; cs.upper_continues_slot0 = 0;
    return launch_reduce(c, s, d_out, tail, 5, grid, [&](int32_t g, hipStream_t st, const EventPair* timed, const ReduceWs& ws) {
        launch_european<1, kControlVariate>(antithetic != 0, g, st, pr, cs, ws, nullptr, timed);
    }, profiled);
}
}  // namespace

extern "C" int olmc_european_cv_shard(double S, double K, double T, double r, double sigma, double q, int is_call,
                                      int64_t path_offset, int64_t n_local, int32_t n_steps, uint64_t seed, int antithetic,
                                      olmc_cv_moments* out) {
    if (!out) return fail(OLMC_ERR_ARG, "null pointer");
    int rc = check_paths(path_offset, n_local, n_steps);
    if (rc) return rc;
    CtxLease lease;
    rc = ctx_lease(&lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    rc = cv_device(c, c->stream, make_option(S, K, T, r, sigma, q, is_call), path_offset, n_local, n_steps, seed, antithetic, c->d_result, -1.0, true);
    if (rc) return rc;
    cv_from_device(c->h_result, n_local * (antithetic ? 2 : 1), S, T, r, q, out);       // d = disc * x (monte_carlo.py:175)
    if (poisoned(S, K, T, r, sigma, q)) out->value = std::nan("");
    return OLMC_OK;
}

extern "C" int olmc_european_cv(double S, double K, double T, double r, double sigma, double q, int is_call,
                                int64_t n_paths, int32_t n_steps, uint64_t seed, int antithetic,
                                olmc_cv_moments* out) {
    return olmc_european_cv_shard(S, K, T, r, sigma, q, is_call, 0, n_paths, n_steps, seed, antithetic, out);
}

extern "C" int olmc_combine_cv(const olmc_cv_moments* parts, int32_t n_parts, double S, double T, double r, double q,
                               olmc_cv_moments* out) {
    if (!parts || !out || n_parts < 1) return fail(OLMC_ERR_ARG, "bad arguments");
    if (!combine_cv(parts, n_parts, S, T, r, q, out)) return fail(OLMC_ERR_ARG, "no samples");     // fixed rank order => bitwise stable
    return OLMC_OK;
}

// ======================================================= single-contract exotics ====
namespace {
// One reducing launch of a one-contract path kernel on a leased context, grid_for(n_local) workgroups, then its stats (discounted
// at r_for_discount; NaN when poisoned_inputs).  launch(grid, stream, timed, pr, ws) queues the kernel.
template <typename Launch>
int run_structured(int64_t path_offset, int64_t n_local, int32_t n_steps, uint64_t seed, int antithetic, double r_for_discount,
                   double T, bool poisoned_inputs, olmc_stats* out, Launch launch, int nv = 2, double* raw_sums = nullptr) {
    if (!out) return fail(OLMC_ERR_ARG, "null pointer");
    int rc = check_paths(path_offset, n_local, n_steps);
    if (rc) return rc;
    CtxLease lease;
    rc = ctx_lease(&lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    const PathRange pr = make_range(path_offset, n_local, n_steps, seed);
    rc = launch_reduce(c, c->stream, c->d_result, -1.0, nv, grid_for(n_local),
                       [&](int32_t grid, hipStream_t st, const EventPair* timed, const ReduceWs& ws) { launch(grid, st, timed, pr, ws); });
    if (rc) return rc;
    finish_one(c->h_result, n_local * (antithetic ? 2 : 1), r_for_discount, T, poisoned_inputs, out);
    if (raw_sums) for (int m = 0; m < nv; ++m) raw_sums[m] = c->h_result[m];     // the context is still leased
    return OLMC_OK;
}
}  // namespace

// ===================================================================== Asian ====
extern "C" int olmc_asian(double S, double K, double T, double r, double sigma, double q, int is_call, int avg_kind,
                          int64_t path_offset, int64_t n_local, int32_t n_steps, uint64_t seed, int antithetic,
                          olmc_stats* out) {
    if (!out) return fail(OLMC_ERR_ARG, "null pointer");
    if (avg_kind != OLMC_AVG_ARITHMETIC && avg_kind != OLMC_AVG_GEOMETRIC && avg_kind != OLMC_AVG_ARITHMETIC_FAST)
        return fail(OLMC_ERR_ARG, "bad avg_kind");
    AsianContract ac;
    const GbmStep g = gbm_step(T, n_steps, r, q, sigma);          // exotic_options.py:54-56
    ac.log_s0 = std::log(S);
    ac.s0 = S;
    ac.drift = g.drift;
    ac.vol = g.vol;
    ac.strike = K;
    ac.sign = is_call ? 1.0 : -1.0;
    ac.inv_steps = 1.0 / n_steps;
    const bool anti = antithetic != 0, geo = avg_kind == OLMC_AVG_GEOMETRIC, fast = avg_kind == OLMC_AVG_ARITHMETIC_FAST;
    return run_structured(path_offset, n_local, n_steps, seed, antithetic, r, T, poisoned(S, K, T, r, sigma, q), out,
                          [&](int32_t grid, hipStream_t st, const EventPair* timed, const PathRange& pr, const ReduceWs& ws) {
                              auto go = [&](auto kernel) { launch_timed(kernel, dim3(grid), dim3(kBlock), st, timed, pr, ac, ws); };
                              if (geo) with_bool(anti, [&](auto a) { go(asian_kernel<a, true>); });
                              else if (fast) with_bool(anti, [&](auto a) { go(asian_kernel<a, false>); });
                              else with_bool(anti, [&](auto a) { go(asian_exp64_kernel<a>); });      // reference precision
                          });
}

// The 8 / 14 contracts of compute_greeks_unified over an arithmetic Asian (ExoticAdapter, unified_greeks.py:177-227) in one launch.
extern "C" int olmc_asian_greeks_fd(double S, double K, double T, double r, double sigma, double q, int is_call, int avg_kind, int64_t n_paths,
                                    int32_t n_steps, uint64_t seed, int antithetic, int second_order, double* out9, olmc_stats* evals) {
    if (!out9) return fail(OLMC_ERR_ARG, "null pointer");
    if (!(T > 0.0)) return fail(OLMC_ERR_ARG, "T must be > 0");
    if (avg_kind != OLMC_AVG_ARITHMETIC && avg_kind != OLMC_AVG_GEOMETRIC)
        return fail(OLMC_ERR_ARG, "avg_kind must be OLMC_AVG_ARITHMETIC or OLMC_AVG_GEOMETRIC (the fp32-exponent form has no fused Greeks)");
    const bool geo = avg_kind == OLMC_AVG_GEOMETRIC;
    int rc = check_paths(0, n_paths, n_steps);
    if (rc) return rc;
    const GreeksSet gs(S, K, T, r, sigma, q, is_call, second_order);
    AsianGreeksSet as;
    constexpr double kLog2e = 1.4426950408889634;
    const double unit = geo ? 1.0 : (OLMC_EXP2_TABLE ? kExp2Entries * kLog2e : kLog2e);     // what each kernel's exponential counts in
    if (const char* bad = asian_greeks_layout(gs, n_steps, geo, unit, K, is_call, &as)) return fail(OLMC_ERR_STATE, bad);
    CtxLease lease;
    rc = ctx_lease(&lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    if (n_paths > static_cast<int64_t>(kMaxGrid) * kBlock) return fail(OLMC_ERR_ARG, "n_paths beyond one launch of the fused Asian Greeks kernel (2^26)");
    const PathRange pr = make_range(0, n_paths, n_steps, seed);
    const int32_t grid = static_cast<int32_t>((n_paths + kBlock - 1) / kBlock);      // the grid covers every path
    const int nsets = gs.nsets();
    const bool anti = antithetic != 0;
    rc = launch_reduce(c, c->stream, c->d_result, -1.0, 2 * nsets, grid, [&](int32_t g, hipStream_t st, const EventPair* timed, const ReduceWs& ws) {
        auto go = [&](auto kernel) { launch_timed(kernel, dim3(g), dim3(kBlock), st, timed, pr, as, ws); };
        if (geo) with_set_anti(nsets, anti, [&](auto width, auto a) { go(asian_geometric_greeks_kernel<a, width>); });
        else with_set_anti(nsets, anti, [&](auto width, auto a) { go(asian_exp64_greeks_kernel<a, width>); });
    });
    if (rc) return rc;
    olmc_stats st[OLMC_MAX_BATCH];
    finish_set(c->h_result, nullptr, n_paths * (anti ? 2 : 1), gs.o, gs.k, false, false, st);
    gs.finish(st, T, out9, evals);
    return OLMC_OK;
}

// ========================================================== barrier / lookback ====
namespace {
// The contract of a barrier / lookback path (extrema_kernel, qmc_path_kernel).  `barrier` is the level of a barrier kind (> 0: the
// entry points refuse any other) and 0 where there is none (lookbacks, the Asian payoffs of qmc_path_kernel): log_barrier_rel is then 0.
ExtremaContract make_extrema(double S, double K, double T, double r, double sigma, double q, int is_call, int payoff, double barrier, int32_t n_steps) {
    const GbmStep g = gbm_step(T, n_steps, r, q, sigma);          // exotic_options.py:54-56
    ExtremaContract ec;
    ec.s0 = S;
    ec.log_barrier_rel = barrier > 0.0 ? std::log(barrier / S) : 0.0;
    ec.drift = g.drift;
    ec.vol = g.vol;
    ec.strike = K;
    ec.sign = is_call ? 1.0 : -1.0;
    ec.payoff = payoff;
    ec.pad = 0;
    return ec;
}

int run_extrema(double S, double K, double T, double r, double sigma, double q, int is_call, int payoff, double barrier,
                int64_t path_offset, int64_t n_local, int32_t n_steps, uint64_t seed, int antithetic, olmc_stats* out) {
    const ExtremaContract ec = make_extrema(S, K, T, r, sigma, q, is_call, payoff, barrier, n_steps);
    return run_structured(path_offset, n_local, n_steps, seed, antithetic, r, T, poisoned(S, K, T, r, sigma, q) || std::isnan(barrier), out,
                          [&](int32_t grid, hipStream_t st, const EventPair* timed, const PathRange& pr, const ReduceWs& ws) {
                              with_bool(antithetic != 0, [&](auto a) { launch_timed(extrema_kernel<a>, dim3(grid), dim3(kBlock), st, timed, pr, ec, ws); });
                          });
}
}  // namespace

extern "C" int olmc_barrier(double S, double K, double T, double r, double sigma, double q, int is_call, double barrier,
                            int barrier_kind, int64_t path_offset, int64_t n_local, int32_t n_steps, uint64_t seed,
                            int antithetic, olmc_stats* out) {
    if (!(barrier > 0.0)) return fail(OLMC_ERR_ARG, "Barrier must be positive");
    if (barrier_kind < OLMC_BARRIER_UP_OUT || barrier_kind > OLMC_BARRIER_DOWN_IN) return fail(OLMC_ERR_ARG, "bad barrier_kind");
    return run_extrema(S, K, T, r, sigma, q, is_call, barrier_kind, barrier, path_offset, n_local, n_steps, seed, antithetic, out);
}

extern "C" int olmc_lookback(double S, double K, double T, double r, double sigma, double q, int is_call, int fixed_strike,
                             int64_t path_offset, int64_t n_local, int32_t n_steps, uint64_t seed, int antithetic,
                             olmc_stats* out) {
    return run_extrema(S, K, T, r, sigma, q, is_call, fixed_strike ? kLookbackFixed : kLookbackFloating, 0.0, path_offset,
                       n_local, n_steps, seed, antithetic, out);
}

// The 8 / 14 contracts of compute_greeks_unified over a barrier / lookback option (ExoticAdapter, unified_greeks.py:177-227) in one launch.
extern "C" int olmc_extrema_greeks_fd(double S, double K, double T, double r, double sigma, double q, int is_call, int payoff, double barrier,
                                      int64_t n_paths, int32_t n_steps, uint64_t seed, int antithetic, int second_order, double* out9,
                                      olmc_stats* evals) {
    if (!out9) return fail(OLMC_ERR_ARG, "null pointer");
    if (!(T > 0.0)) return fail(OLMC_ERR_ARG, "T must be > 0");
    if (payoff < kBarrierUpOut || payoff > kLookbackFixed) return fail(OLMC_ERR_ARG, "payoff must be a barrier kind (0..3) or OLMC_LOOKBACK_FLOATING / _FIXED (4, 5)");
    const bool is_barrier = payoff <= kBarrierDownIn;
    if (is_barrier && !(barrier > 0.0)) return fail(OLMC_ERR_ARG, "Barrier must be positive");
    int rc = check_paths(0, n_paths, n_steps);
    if (rc) return rc;
    if (n_paths > static_cast<int64_t>(kMaxGrid) * kBlock) return fail(OLMC_ERR_ARG, "n_paths beyond one launch of the fused Greeks kernel (2^26)");
    const GreeksSet gs(S, K, T, r, sigma, q, is_call, second_order);
    ExtremaGreeksSet es;
    if (const char* bad = extrema_greeks_layout(gs, n_steps, payoff, barrier, K, is_call, &es)) return fail(OLMC_ERR_STATE, bad);
    CtxLease lease;
    rc = ctx_lease(&lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    const PathRange pr = make_range(0, n_paths, n_steps, seed);
    const int32_t grid = static_cast<int32_t>((n_paths + kBlock - 1) / kBlock);      // the grid covers every path
    const int nsets = gs.nsets();
    const bool anti = antithetic != 0;
    rc = launch_reduce(c, c->stream, c->d_result, -1.0, 2 * nsets, grid, [&](int32_t g, hipStream_t st, const EventPair* timed, const ReduceWs& ws) {
        with_set_anti(nsets, anti, [&](auto width, auto a) { launch_timed(extrema_greeks_kernel<a, width>, dim3(g), dim3(kBlock), st, timed, pr, es, ws); });
    });
    if (rc) return rc;
    olmc_stats st[OLMC_MAX_BATCH];
    finish_set(c->h_result, nullptr, n_paths * (anti ? 2 : 1), gs.o, gs.k, std::isnan(barrier), false, st);
    gs.finish(st, T, out9, evals);
    return OLMC_OK;
}

// ======================================================= autocallable / cliquet ====
namespace {
// The checks and the contract of an autocallable, shared by the Philox and the Sobol entry points.
int autocall_check(int32_t observation_freq, int32_t n_steps) {
    if (observation_freq < 1) return fail(OLMC_ERR_ARG, "observation_freq must be >= 1");
    if (n_steps >= 1 && n_steps / observation_freq < 1) return fail(OLMC_ERR_ARG, "no observation date: observation_freq > n_steps");
    return OLMC_OK;
}

struct AutocallSetup {
    AutocallContract ac;
    double obs_rate;       // -r dt f: ln of ac.obs_df (qmc_autocall_kernel takes its redemption discount by one exponential)
    bool bad;              // a NaN input: the result is NaN (poisoned)
};
AutocallSetup make_autocall(double S, double T, double r, double sigma, double q, double autocall_barrier, double coupon_barrier,
                            double coupon_rate, double ki_barrier, int32_t observation_freq, int32_t n_steps) {
    AutocallSetup a;
    AutocallContract& ac = a.ac;
    const GbmStep g = gbm_step(T, n_steps, r, q, sigma);
    ac.drift = g.drift;
    ac.vol = g.vol;
    ac.log_autocall = log_level(autocall_barrier);
    ac.log_coupon = log_level(coupon_barrier);
    ac.log_ki = log_level(ki_barrier);
    ac.obs_freq = observation_freq;
    ac.n_obs = n_steps / observation_freq;                      // len(range(f, M + 1, f))
    ac.coupon_unit = coupon_rate * T / ac.n_obs;                // coupon_rate * ((i+1)/n_obs) * T, accrued per observation (:459-460)
    ac.final_coupon = coupon_rate * T;
    a.obs_rate = -r * g.dt * observation_freq;
    ac.obs_df = std::exp(a.obs_rate);                           // exp(-r t dt) at t = k f, built up by products (:461)
    ac.final_df = std::exp(-r * T);
    a.bad = poisoned(S, 1.0, T, r, sigma, q) || std::isnan(autocall_barrier + coupon_barrier + coupon_rate + ki_barrier);
    return a;
}

int cliquet_check(int32_t n_periods, int32_t n_steps) {
    if (n_periods < 1 || (n_steps >= 1 && n_steps / n_periods < 1)) return fail(OLMC_ERR_ARG, "n_periods must be in [1, n_steps]");
    return OLMC_OK;
}

CliquetContract make_cliquet(double S, double T, double r, double sigma, double q, double local_cap, double local_floor, double global_cap,
                             double global_floor, int32_t n_periods, int32_t n_steps) {
    CliquetContract cc;
    const GbmStep g = gbm_step(T, n_steps, r, q, sigma);
    cc.s0 = S;
    cc.drift = g.drift;
    cc.vol = g.vol;
    cc.local_cap = local_cap; cc.local_floor = local_floor; cc.global_cap = global_cap; cc.global_floor = global_floor;
    cc.steps_per_period = n_steps / n_periods;                  // exotic_options.py:532
    cc.n_periods = n_periods;
    return cc;
}

bool cliquet_poisoned(double S, double T, double r, double sigma, double q, double local_cap, double local_floor, double global_cap, double global_floor) {
    return poisoned(S, 1.0, T, r, sigma, q) || std::isnan(local_cap + local_floor + global_cap + global_floor);
}
}  // namespace

extern "C" int olmc_autocallable(double S, double T, double r, double sigma, double q, double autocall_barrier,
                                 double coupon_barrier, double coupon_rate, double ki_barrier, int32_t observation_freq,
                                 int64_t path_offset, int64_t n_local, int32_t n_steps, uint64_t seed, int antithetic,
                                 olmc_stats* out) {
    if (const int rc = autocall_check(observation_freq, n_steps)) return rc;
    const AutocallSetup a = make_autocall(S, T, r, sigma, q, autocall_barrier, coupon_barrier, coupon_rate, ki_barrier, observation_freq, n_steps);
    const AutocallContract& ac = a.ac;
    // payoffs are already discounted path by path (exotic_options.py:463, 489): no outer discount
    return run_structured(path_offset, n_local, n_steps, seed, antithetic, 0.0, T, a.bad, out,
                          [&](int32_t grid, hipStream_t st, const EventPair* timed, const PathRange& pr, const ReduceWs& ws) {
                              with_bool(antithetic != 0, [&](auto a_) { launch_timed(autocall_kernel<a_>, dim3(grid), dim3(kBlock), st, timed, pr, ac, ws); });
                          });
}

extern "C" int olmc_cliquet(double S, double T, double r, double sigma, double q, double local_cap, double local_floor,
                            double global_cap, double global_floor, int32_t n_periods, int64_t path_offset,
                            int64_t n_local, int32_t n_steps, uint64_t seed, int antithetic, olmc_stats* out) {
    if (const int rc = cliquet_check(n_periods, n_steps)) return rc;
    const CliquetContract cc = make_cliquet(S, T, r, sigma, q, local_cap, local_floor, global_cap, global_floor, n_periods, n_steps);
    const bool bad = cliquet_poisoned(S, T, r, sigma, q, local_cap, local_floor, global_cap, global_floor);
    return run_structured(path_offset, n_local, n_steps, seed, antithetic, r, T, bad, out,
                          [&](int32_t grid, hipStream_t st, const EventPair* timed, const PathRange& pr, const ReduceWs& ws) {
                              with_bool(antithetic != 0, [&](auto a) { launch_timed(cliquet_kernel<a>, dim3(grid), dim3(kBlock), st, timed, pr, cc, ws); });
                          });
}

// ================================================================== full paths ====
namespace {
// The prologue of a path-matrix export: the argument checks, the cap on the `bytes` it keeps on the device (refused with `too_big`),
// a lease and, when `reserve`, a bulk buffer of `bytes`.
int matrix_prologue(int64_t n_paths, int32_t n_steps, double bytes, const char* too_big, CtxLease* lease, bool reserve = true) {
    int rc = check_paths(0, n_paths, n_steps);
    if (rc) return rc;
    if (bytes > 64e9) return fail(OLMC_ERR_ARG, too_big);
    rc = ctx_lease(lease);
    if (rc || !reserve) return rc;
    return bulk_reserve(lease->c, static_cast<size_t>(bytes));
}

// A family without per-context state to set up between the lease and the launch.
int no_setup(DeviceCtx*) { return OLMC_OK; }

// One (n_steps + 1) x n_paths matrix of Philox paths [0, n_paths) to the host, after the caller's null and model checks: the prologue,
// `setup(c)` (the family's per-context hook: the local-volatility table), launch(c, grid, range, the matrix on the device), the copy.
template <typename Setup, typename Launch>
int run_philox_matrix(int64_t n_paths, int32_t n_steps, uint64_t seed, double* out_host, Setup setup, Launch launch) {
    const double bytes = 8.0 * static_cast<double>(n_paths) * (n_steps + 1.0);
    CtxLease lease;
    int rc = matrix_prologue(n_paths, n_steps, bytes, "path matrix would exceed 64 GB", &lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    rc = setup(c);
    if (rc) return rc;
    launch(c, grid_for(n_paths), make_range(0, n_paths, n_steps, seed), c->bulk.as<double>());
    HIP_TRY(hipGetLastError());
    return copy_to_host(c, out_host, c->bulk.get(), static_cast<size_t>(bytes));
}
}  // namespace

extern "C" int olmc_gbm_paths(double S, double T, double r, double sigma, double q, int64_t n_paths, int32_t n_steps,
                              uint64_t seed, int path_major, double* out_host) {
    if (!out_host) return fail(OLMC_ERR_ARG, "null pointer");
    return run_philox_matrix(n_paths, n_steps, seed, out_host, no_setup,
                             [&](DeviceCtx* c, int32_t grid, const PathRange& pr, double* d_paths) {
        LsmContract lc{};
        const GbmStep g = gbm_step(T, n_steps, r, q, sigma);          // gbm_numpy.py:106-108
        lc.log_s0 = std::log(S);
        lc.s_first = S;
        lc.drift = g.drift;
        lc.vol = g.vol;
        lc.n_steps = n_steps;
        with_bool(path_major != 0, [&](auto pm) {
            launch_timed(lsm_paths_kernel<pm>, dim3(grid), dim3(kBlock), c->stream, nullptr, pr, lc, d_paths);
        });
    });
}

extern "C" int olmc_exercise_boundary(double S, double K, double T, double r, double sigma, double q, int is_call,
                                      int64_t n_paths, int32_t n_steps, uint64_t seed, double* boundary_host) {
    if (!boundary_host) return fail(OLMC_ERR_ARG, "null pointer");
    const double bytes = 8.0 * static_cast<double>(n_paths) * (n_steps + 1.0);
    CtxLease lease;
    int rc = matrix_prologue(n_paths, n_steps, bytes, "path matrix would exceed 64 GB", &lease, false);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    const size_t rows = static_cast<size_t>(n_steps) + 1;
    const size_t path_bytes = (static_cast<size_t>(bytes) + 255) / 256 * 256;
    Carver bulk;
    rc = bulk_reserve(c, path_bytes + rows * sizeof(double), &bulk);
    if (rc) return rc;
    double* d_paths = bulk.take<double>(path_bytes / sizeof(double));
    double* d_boundary = bulk.take<double>(rows);
    LsmContract lc{};
    const GbmStep g = gbm_step(T, n_steps, r, q, sigma);          // exotic_options.py:54-56
    lc.log_s0 = std::log(S);
    lc.s_first = std::exp(lc.log_s0);                   // :59-65: column 0 is exp(log S)
    lc.drift = g.drift;
    lc.vol = g.vol;
    lc.n_steps = n_steps;
    const PathRange pr = make_range(0, n_paths, n_steps, seed);
    hipLaunchKernelGGL((lsm_paths_kernel<false>), dim3(grid_for(n_paths)), dim3(kBlock), 0, c->stream, pr, lc, d_paths);
    HIP_TRY(hipGetLastError());
    // np.percentile(x, 10) for a put, 90 for a call (:337-341); NumPy divides q by 100 first
    hipLaunchKernelGGL(exercise_boundary_kernel, dim3(static_cast<uint32_t>(rows)), dim3(kBoundaryThreads), 0, c->stream, d_paths, n_paths, K,
                       is_call ? 1.0 : -1.0, (is_call ? 90.0 : 10.0) / 100.0, d_boundary);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(boundary_host, d_boundary, rows * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return OLMC_OK;
}

// ================================================================ American (LSM) ====
namespace {
// Mean and standard deviation of S_t / K over the in-the-money side of the strike under the model's lognormal law (truncated
// lognormal moments, closed form): the affine map that standardises the regressor of the date-t regression (LsmScale).
// Any finite, positive pair gives the same least-squares fit in exact arithmetic; this one keeps the normal equations well conditioned.
void lsm_regressor_scale(double S, double K, double r, double q, double sigma, double dt, int32_t t, bool is_call, double* centre, double* inv_width) {
    *centre = 1.0;
    *inv_width = 1.0;
    const double m = std::log(S) + (r - q - 0.5 * sigma * sigma) * dt * t, s = sigma * std::sqrt(dt * t), a = std::log(K);
    if (!(s > 0.0) || !std::isfinite(m) || !std::isfinite(a)) return;
    const double side = is_call ? 1.0 : -1.0;            // in the money: side * (ln S_t - ln K) > 0
    auto phi = [](double u) { return 0.5 * std::erfc(-u * 0.70710678118654752440); };
    const double p0 = phi(side * (m - a) / s);
    const double m1 = std::exp(m + 0.5 * s * s) * phi(side * (m + s * s - a) / s);
    const double m2 = std::exp(2.0 * m + 2.0 * s * s) * phi(side * (m + 2.0 * s * s - a) / s);
    if (!(p0 > 1e-280) || !std::isfinite(m1) || !std::isfinite(m2)) return;
    const double mean = m1 / p0, var = m2 / p0 - mean * mean;
    const double width = std::max(std::sqrt(std::max(var, 0.0)), 1e-6 * mean);
    if (!(mean > 0.0) || !std::isfinite(width) || !(width > 0.0)) return;
    *centre = mean / K;
    *inv_width = K / width;
}

// The contract of an LSM pricing on paths of T / n_steps steps (exotic_options.py:54-56, 260-261); column 0 is exp(ln S) (:59-65).
LsmContract lsm_contract(double S, double K, double T, double r, double sigma, double q, int is_call, int32_t n_steps, int32_t poly_degree) {
    LsmContract lc;
    const GbmStep g = gbm_step(T, n_steps, r, q, sigma);
    lc.log_s0 = std::log(S);
    lc.s_first = std::exp(lc.log_s0);
    lc.drift = g.drift;
    lc.vol = g.vol;
    lc.strike = K;
    lc.inv_strike = 1.0 / K;
    lc.sign = is_call ? 1.0 : -1.0;
    lc.discount = std::exp(-r * g.dt);
    lc.degree = poly_degree;
    lc.n_steps = n_steps;
    return lc;
}

// Bytes of an LSM pricing's device buffers: the path matrix and the cash flows, + two buffers of <= 1024 workgroup rows.
double lsm_bytes(int64_t n_paths, int32_t n_steps) { return 8.0 * static_cast<double>(n_paths) * (n_steps + 2.0) + 8.0 * 2 * 1024 * kLsmNV; }

// The step chain of an LSM pricing over the time-major path matrix d_paths [n_steps + 1][n_paths] that a launch queued before it on
// c's stream writes; d_cash [n_paths] and d_rows [2][1024][kLsmNV] are the next the caller's `bulk` hands out.  Leaves the moments of the time-0
// cash flows in c->h_result once the host has waited for them.  scale(t, &centre, &inv_width) gives the regressor's pair of date t.
template <typename Scale>
int lsm_chain_scaled(DeviceCtx* c, const LsmContract& lc, int64_t n_paths, int32_t n_steps, double* d_paths, Carver* bulk, Scale&& scale) {
    double* d_cash = bulk->take<double>(static_cast<size_t>(n_paths));                  // [n_paths]
    double* d_rows = bulk->take<double>(size_t(2) * 1024 * kLsmNV);                     // [2][grid][kLsmNV]: the regression sums a date hands to the next launch
    // The per-date launches move 32 bytes per path and hand 16 sums per workgroup to the next launch, EVERY workgroup of which sums all
    // the rows: at most ONE workgroup per compute unit (<= 256 rows: one round trip), each thread taking its paths U at a time with all
    // 3 U loads in flight.  With one wave per SIMD the register count buys nothing, so U follows the paths a thread has (1, 2, 4, 8:
    // 98 ... 170 VGPRs).  Measured per call, 51 launches (profiles/r04_lsm_ab.jsonl): 1M x 50 -- 898 us at U = 1, 771 / 658 / 628 / 662 at
    // 2 / 4 / 8 / 16; two workgroups per CU 792 / 717 / 674 (U = 1 / 2 / 4), four 978 / 971 / 952 (a workgroup re-reads every row);
    // 200k x 50 -- 366 / 343 / 328 / 345 at U = 1 / 2 / 4 / 8; 50k x 50, where a thread has one path, 275 - 300 whatever U.
    const int32_t grid = std::min<int32_t>(grid_for(n_paths), std::min<int32_t>(c->cus, 1024));
    const int64_t per_thread = (n_paths + static_cast<int64_t>(grid) * kBlock - 1) / (static_cast<int64_t>(grid) * kBlock);
    const int lsm_unroll = per_thread <= 1 ? 1 : per_thread <= 2 ? 2 : per_thread <= 4 ? 4 : 8;
    // every launch sums the rows the launch before it stored, fits the later date from them and stores its own rows: stream order is
    // the only synchronisation, the host waits once at the end.  Only the LAST launch (t_fit == 0: the moments of the time-0 cash
    // flow) goes through the grid reduction and writes into the pinned host buffer.
    ReduceWs ws;
    int rc = make_ws(c, c->stream, grid, kLsmNV, c->d_result, -1.0, &ws);          // arms the completion word for the launch that writes d_result
    if (rc) return rc;
    std::vector<double> centre(static_cast<size_t>(n_steps) + 1, 1.0), inv_width(static_cast<size_t>(n_steps) + 1, 1.0);   // while the path kernel runs
    for (int32_t t = 1; t < n_steps; ++t) scale(t, &centre[t], &inv_width[t]);
    int32_t init = 1;
    for (int32_t t_fit = n_steps - 1; t_fit >= 0; --t_fit) {
        const bool first = init != 0, final_date = t_fit == 0;
        const LsmScale sc{centre[t_fit], inv_width[t_fit], centre[t_fit + 1], inv_width[t_fit + 1]};
        auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, c->stream, n_paths, lc, sc, d_rows, t_fit, d_paths, d_cash, ws); };
        auto pick = [&](auto u) {
            constexpr int U = decltype(u)::value;
            if (first && final_date) go(lsm_step_kernel<U, true, true>);
            else if (first) go(lsm_step_kernel<U, true, false>);
            else if (final_date) go(lsm_step_kernel<U, false, true>);
            else go(lsm_step_kernel<U, false, false>);
        };
        if (lsm_unroll == 1) pick(std::integral_constant<int, 1>{});
        else if (lsm_unroll == 2) pick(std::integral_constant<int, 2>{});
        else if (lsm_unroll == 4) pick(std::integral_constant<int, 4>{});
        else pick(std::integral_constant<int, 8>{});
        rc = after_launch(c, c->stream);
        if (rc) return rc;
        init = 0;
    }
    return sync_or_recover(c, c->stream);
}

// The chain under constant volatility: lsm_regressor_scale's pair with the contract's sigma at every date.
int lsm_chain(DeviceCtx* c, double S, double K, double T, double r, double sigma, double q, int is_call, const LsmContract& lc,
              int64_t n_paths, int32_t n_steps, double* d_paths, Carver* bulk) {
    const double dt = T / n_steps;
    return lsm_chain_scaled(c, lc, n_paths, n_steps, d_paths, bulk, [&](int32_t t, double* centre, double* inv_width) {
        lsm_regressor_scale(S, K, r, q, sigma, dt, t, is_call != 0, centre, inv_width);
    });
}
}  // namespace

extern "C" int olmc_american_lsm(double S, double K, double T, double r, double sigma, double q, int is_call,
                                 int64_t n_paths, int32_t n_steps, int32_t poly_degree, uint64_t seed, olmc_stats* out) {
    if (!out) return fail(OLMC_ERR_ARG, "null pointer");
    if (poly_degree < 1 || poly_degree > kLsmMaxDegree) return fail(OLMC_ERR_ARG, "poly_degree must be in [1, 4]");
    CtxLease lease;
    int rc = matrix_prologue(n_paths, n_steps, lsm_bytes(n_paths, n_steps), "path matrix would exceed 64 GB: lower n_paths or n_steps", &lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    Carver bulk = c->bulk.carve();
    double* d_paths = bulk.take<double>((static_cast<size_t>(n_steps) + 1) * n_paths);   // [n_steps + 1][n_paths]
    const LsmContract lc = lsm_contract(S, K, T, r, sigma, q, is_call, n_steps, poly_degree);
    const PathRange pr = make_range(0, n_paths, n_steps, seed);
    EventPair ep{};
    if (g_profile) { rc = prof_begin(c, c->stream, &ep); if (rc) return rc; }
    hipLaunchKernelGGL((lsm_paths_kernel<false>), dim3(grid_for(n_paths)), dim3(kBlock), 0, c->stream, pr, lc, d_paths);
    HIP_TRY(hipGetLastError());
    rc = lsm_chain(c, S, K, T, r, sigma, q, is_call, lc, n_paths, n_steps, d_paths, &bulk);
    if (rc) return rc;
    if (g_profile) { rc = prof_end(c, c->stream, ep); if (rc) return rc; }
    // the time-0 cash flows are already discounted step by step (:302-304): no outer factor
    finish_one(c->h_result, n_paths, 0.0, T, poisoned(S, K, T, r, sigma, q), out);
    return OLMC_OK;
}

// ===================================================================== Heston ====
namespace {
// The model, as every olmc_heston* entry point hands it inward.
struct HestonModel {
    double kappa, theta, sigma_v, rho, v0;
    bool nan() const { return std::isnan(kappa + theta + sigma_v + rho + v0); }
};

HestonContract make_heston(double S, double K, double T, double r, double q, int is_call, const HestonModel& m, int32_t n_steps) {
    const double kappa = m.kappa, theta = m.theta, sigma_v = m.sigma_v, rho = m.rho;
    HestonContract hc;
    const double dt = T / n_steps;                     // heston.py:218-219
    hc.log_s0 = std::log(S);
    hc.v0 = m.v0;
    hc.mu_dt = (r - q) * dt;
    hc.dt = dt;
    hc.sqrt_dt = std::sqrt(dt);
    hc.kappa_dt = kappa * dt;
    hc.theta = theta;
    hc.sigma_v = sigma_v;
    hc.rho = rho;
    hc.rho_c = std::sqrt(1 - rho * rho);               // :228
    hc.strike = K;
    hc.sign = is_call ? 1.0 : -1.0;
    return hc;
}

// The model checks every Heston entry point makes (Philox and Sobol), and the inputs that answer NaN.
int heston_check(const HestonModel& m) {
    if (!(m.rho >= -1.0 && m.rho <= 1.0)) return fail(OLMC_ERR_ARG, "rho must be in [-1, 1]");
    return OLMC_OK;
}
bool heston_poisoned(double S, double K, double T, double r, double q, const HestonModel& m) { return poisoned(S, K, T, r, 0.0, q) || m.nan(); }

// The scheme divides by kappa, sigma_v and the conditional mean m = v E + theta (1 - E), and starts from v0 itself.
int heston_qe_check(const HestonModel& m) {
    const int rc = heston_check(m);
    if (rc) return rc;
    if (m.kappa <= 0.0) return fail(OLMC_ERR_ARG, "kappa must be positive for the QE scheme");
    if (m.theta <= 0.0) return fail(OLMC_ERR_ARG, "theta must be positive for the QE scheme");
    if (m.sigma_v <= 0.0) return fail(OLMC_ERR_ARG, "sigma_v must be positive for the QE scheme");
    if (m.v0 < 0.0) return fail(OLMC_ERR_ARG, "v0 must be non-negative for the QE scheme");
    return OLMC_OK;
}

int heston_qe_sequential(int construction) {
    if (construction == OLMC_QMC_BRIDGE)
        return fail(OLMC_ERR_ARG, "the QE scheme takes OLMC_QMC_SEQUENTIAL only: its variance draw is a uniform, not a Brownian increment");
    return OLMC_OK;
}

// The launch constants, every one folded here in fp64 (olmc_kernels.h "Heston, quadratic-exponential scheme").
HestonQeContract make_heston_qe(double S, double T, double r, double q, int is_call, const HestonModel& m, int32_t n_steps) {
    const double kappa = m.kappa, theta = m.theta, sigma_v = m.sigma_v, rho = m.rho;
    HestonQeContract hc;
    const double dt = T / n_steps;
    const double e = std::exp(-kappa * dt), one_minus_e = -std::expm1(-kappa * dt);
    const double g = 0.5 * dt * (kappa * rho / sigma_v - 0.5);
    hc.log_s0 = std::log(S);
    hc.v0 = m.v0;
    hc.drift_dt = (r - q) * dt + -rho * kappa * theta * dt / sigma_v;                // (r - q) dt + K0
    hc.e = e;
    hc.theta_1me = theta * one_minus_e;
    hc.c1 = sigma_v * sigma_v * e * one_minus_e / kappa;
    hc.c2 = theta * sigma_v * sigma_v * one_minus_e * one_minus_e / (2.0 * kappa);
    hc.k1 = g - rho / sigma_v;
    hc.k2 = g + rho / sigma_v;
    hc.k3 = 0.5 * dt * (1.0 - rho * rho);                                            // K4 = K3
    hc.sign = is_call ? 1.0 : -1.0;
    return hc;
}

// A discretisation scheme as the entry points that serve both take it: its launch contract and how to make it, the model checks of its
// calls, whether its Sobol form takes the Brownian bridge, and its Philox kernels (the Sobol ones differ in their arguments by kBridge).
struct HestonEuler {
    using Contract = HestonContract;
    static constexpr bool kBridge = true;
    static int check(const HestonModel& m) { return heston_check(m); }
    static Contract make(double S, double T, double r, double q, int is_call, const HestonModel& m, int32_t n_steps) {
        return make_heston(S, 0.0, T, r, q, is_call, m, n_steps);
    }
    template <bool PM> static constexpr auto paths_kernel() { return heston_paths_kernel<PM>; }
    template <bool A> static constexpr auto surface_kernel() { return heston_surface_kernel<A>; }
    template <template <bool> class Product, bool A> static constexpr auto product_kernel() { return heston_product_kernel<Product, A>; }
};
struct HestonQe {
    using Contract = HestonQeContract;
    static constexpr bool kBridge = false;
    static int check(const HestonModel& m) { return heston_qe_check(m); }
    static Contract make(double S, double T, double r, double q, int is_call, const HestonModel& m, int32_t n_steps) {
        return make_heston_qe(S, T, r, q, is_call, m, n_steps);
    }
    template <bool PM> static constexpr auto paths_kernel() { return heston_qe_paths_kernel<PM>; }
    template <bool A> static constexpr auto surface_kernel() { return heston_qe_surface_kernel<A>; }
    template <template <bool> class Product, bool A> static constexpr auto product_kernel() { return heston_qe_product_kernel<Product, A>; }
};
template <typename F>
int with_heston_scheme(int scheme, F&& f) {
    return scheme == OLMC_HESTON_QE ? f(HestonQe{}) : f(HestonEuler{});
}
// The model checks of a Sobol call of the scheme, up to the construction it takes.
template <typename Scheme>
int heston_qmc_scheme_check(const HestonModel& m, int construction) {
    const int rc = Scheme::check(m);
    if (rc || Scheme::kBridge) return rc;
    return heston_qe_sequential(construction);
}

// The two device matrices of a path call (spot, then variance, [n + 1] dates each) in the context's bulk buffer, to the host after `launch`.
template <typename Launch>
int heston_path_matrices(DeviceCtx* c, int64_t n_paths, int32_t n_steps, double* spot_host, double* var_host, Launch&& launch) {
    const size_t bytes = sizeof(double) * static_cast<size_t>(n_paths) * (static_cast<size_t>(n_steps) + 1);
    Carver bulk = c->bulk.carve();
    double* d_spot = bulk.take<double>(bytes / sizeof(double));
    double* d_var = bulk.take<double>(bytes / sizeof(double));
    EventPair ep{};
    const EventPair* timed = nullptr;                  // profiling on: the path kernel counts in olmc_kernel_time
    int rc = prof_pair(c, &ep, &timed);
    if (rc) return rc;
    launch(timed, d_spot, d_var);
    HIP_TRY(hipGetLastError());
    rc = copy_to_host(c, spot_host, d_spot, bytes);
    if (rc) return rc;
    return copy_to_host(c, var_host, d_var, bytes);
}

// Philox: every (S, v) state of paths [0, n_paths) of the scheme's stream.
template <typename Scheme>
int run_heston_paths(double S, double T, double r, double q, const HestonModel& m, int64_t n_paths, int32_t n_steps, uint64_t seed, int path_major,
                     double* spot_host, double* var_host) {
    if (!spot_host || !var_host) return fail(OLMC_ERR_ARG, "null pointer");
    int rc = Scheme::check(m);
    if (rc) return rc;
    const double bytes = 8.0 * static_cast<double>(n_paths) * (n_steps + 1.0);
    CtxLease lease;
    rc = matrix_prologue(n_paths, n_steps, 2 * bytes, "path matrices would exceed 64 GB", &lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    const auto hc = Scheme::make(S, T, r, q, 1, m, n_steps);
    const PathRange pr = make_range(0, n_paths, n_steps, seed);
    return heston_path_matrices(c, n_paths, n_steps, spot_host, var_host, [&](const EventPair* timed, double* d_spot, double* d_var) {
        with_bool(path_major != 0, [&](auto pm) {
            launch_timed(Scheme::template paths_kernel<decltype(pm)::value>(), dim3(grid_for(n_paths)), dim3(kBlock), c->stream, timed, pr, hc, S, d_spot,
                         d_var);
        });
    });
}
}  // namespace

extern "C" int olmc_heston_paths(double S, double T, double r, double q, double kappa, double theta, double sigma_v, double rho,
                                 double v0, int64_t n_paths, int32_t n_steps, uint64_t seed, int path_major, double* spot_host,
                                 double* var_host) {
    return run_heston_paths<HestonEuler>(S, T, r, q, {kappa, theta, sigma_v, rho, v0}, n_paths, n_steps, seed, path_major, spot_host, var_host);
}

extern "C" int olmc_heston(double S, double K, double T, double r, double q, int is_call, double kappa, double theta,
                           double sigma_v, double rho, double v0, int64_t path_offset, int64_t n_local, int32_t n_steps,
                           uint64_t seed, int antithetic, olmc_stats* out) {
    if (!out) return fail(OLMC_ERR_ARG, "null pointer");
    const HestonModel m{kappa, theta, sigma_v, rho, v0};
    const int rc = heston_check(m);
    if (rc) return rc;
    const HestonContract hc = make_heston(S, K, T, r, q, is_call, m, n_steps);
    const bool bad = heston_poisoned(S, K, T, r, q, m);
    return run_structured(path_offset, n_local, n_steps, seed, antithetic, r, T, bad, out,
                          [&](int32_t grid, hipStream_t st, const EventPair* timed, const PathRange& pr, const ReduceWs& ws) {
                              with_bool(antithetic != 0, [&](auto a) { launch_timed(heston_kernel<a>, dim3(grid), dim3(kBlock), st, timed, pr, hc, ws); });
                          });
}

// ============================================================== jump diffusion ====
namespace {
int make_jump(double S, double K, double T, double r, double sigma, double q, int is_call, int model, double lambda_j,
              double a1, double a2, double a3, int32_t n_steps, JumpContract* out) {
    if (model != OLMC_JUMP_MERTON && model != OLMC_JUMP_KOU) return fail(OLMC_ERR_ARG, "bad jump model");
    if (!(lambda_j >= 0.0)) return fail(OLMC_ERR_ARG, "lambda_j must be non-negative");
    if (n_steps < 1) return fail(OLMC_ERR_ARG, "n_steps must be >= 1");
    JumpContract jc;
    const double dt = T / n_steps;
    double kappa;                                            // E[e^Y - 1]
    if (model == OLMC_JUMP_MERTON) {
        jc.mu_j = a1; jc.sigma_j = a2;
        jc.kou_p = 0.0; jc.inv_eta1 = 0.0; jc.inv_eta2 = 0.0;
        kappa = std::exp(a1 + 0.5 * a2 * a2) - 1;            // jump_diffusion.py:64-67
    } else {
        jc.mu_j = 0.0; jc.sigma_j = 0.0;
        jc.kou_p = a1; jc.inv_eta1 = 1.0 / a2; jc.inv_eta2 = 1.0 / a3;
        kappa = a1 * a2 / (a2 - 1) + (1 - a1) * a3 / (a3 + 1) - 1;   // :293-299
    }
    jc.kou = model == OLMC_JUMP_KOU;
    jc.pad = 0;
    jc.log_s0 = std::log(S);
    jc.drift = (r - q - lambda_j * kappa - 0.5 * sigma * sigma) * dt;   // :207 / :346 compensated drift
    jc.vol = sigma * std::sqrt(dt);
    jc.strike = K;
    jc.sign = is_call ? 1.0 : -1.0;
    jc.lam_dt = lambda_j * dt;
    // the device draws the jump count by inversion from p0 = exp(-lambda dt), at most kJumpCap = 64 jumps per step:
    // exact to 1e-15 of probability mass up to lambda dt = 20, silently truncated beyond (and p0 underflows at 745).
    // The reference's np.random.poisson has no such limit, so larger rates are refused rather than mispriced.
    if (jc.lam_dt > 20.0) return fail(OLMC_ERR_ARG, "lambda_j * T / n_steps must be <= 20 jumps per step: raise n_steps");
    jc.p0 = std::exp(-jc.lam_dt);
    *out = jc;
    return OLMC_OK;
}
}  // namespace

extern "C" int olmc_jump_diffusion(double S, double K, double T, double r, double sigma, double q, int is_call, int model,
                                   double lambda_j, double a1, double a2, double a3, int64_t path_offset, int64_t n_local,
                                   int32_t n_steps, uint64_t seed, olmc_stats* out) {
    JumpContract jc;
    int rc = make_jump(S, K, T, r, sigma, q, is_call, model, lambda_j, a1, a2, a3, n_steps, &jc);
    if (rc) return rc;
    const bool bad = poisoned(S, K, T, r, sigma, q) || std::isnan(lambda_j + a1 + a2 + a3);
    return run_structured(path_offset, n_local, n_steps, seed, 0, r, T, bad, out,
                          [&](int32_t grid, hipStream_t st, const EventPair* timed, const PathRange& pr, const ReduceWs& ws) {
                              launch_timed(jump_kernel, dim3(grid), dim3(kBlock), st, timed, pr, jc, ws);
                          });
}

extern "C" int olmc_jump_paths(double S, double T, double r, double sigma, double q, int model, double lambda_j, double a1,
                               double a2, double a3, int64_t n_paths, int32_t n_steps, uint64_t seed, int path_major,
                               double* out_host) {
    if (!out_host) return fail(OLMC_ERR_ARG, "null pointer");
    JumpContract jc;
    const int rc = make_jump(S, 0.0, T, r, sigma, q, 1, model, lambda_j, a1, a2, a3, n_steps, &jc);
    if (rc) return rc;
    return run_philox_matrix(n_paths, n_steps, seed, out_host, no_setup,
                             [&](DeviceCtx* c, int32_t grid, const PathRange& pr, double* d_paths) {
        with_bool(path_major != 0, [&](auto pm) {
            launch_timed(jump_paths_kernel<pm>, dim3(grid), dim3(kBlock), c->stream, nullptr, pr, jc, S, d_paths);
        });
    });
}

// ======================================================================= QMC ====
namespace {
// The Sobol arguments of an entry point as its caller passed them, unchecked: SobolCall::make is their only reader.  Braces refuse a
// 64-bit count where a 32-bit one belongs.  The European family has no construction (it passes OLMC_QMC_SEQUENTIAL) and calls its
// steps `dims`.
struct SobolArgs {
    int construction;
    int64_t point_offset, n_points;
    int32_t n_steps;
    const uint32_t* sv;
    const uint32_t* shift;
    int32_t bits;
    int antithetic;
};

// The Sobol points and tables of one call.  One exists only if make() passed it: every refusal of the construction, the tables and
// the point range has been made, with the dimensions a step takes (1: the GBM and local-volatility paths and the European sums, 2:
// Heston's two factors), before anything below an entry point -- the lease, the upload, a launch -- can ask for them.
class SobolCall {
public:
    const bool bridge;
    const int64_t first, count;              // points [first, first + count) of the one sequence
    const int32_t n_steps, dims_per_step;
    const uint32_t* const sv;
    const uint32_t* const shift;
    const int32_t bits;
    const bool anti;

    // The argument checks of a Sobol call, before any context is leased; *rc and olmc_last_error() say why there is no call.
    static std::optional<SobolCall> make(const SobolArgs& a, int32_t dims_per_step, int* rc) {
        *rc = check(a, dims_per_step);
        if (*rc) return std::nullopt;
        return SobolCall(a.construction == OLMC_QMC_BRIDGE, a.point_offset, a.n_points, a.n_steps, dims_per_step, a.sv, a.shift, a.bits, a.antithetic != 0);
    }
    // The same call over points [lo, lo + n) inside its own: a multi-GPU rank's share.
    SobolCall over(int64_t lo, int64_t n) const { return SobolCall(bridge, lo, n, n_steps, dims_per_step, sv, shift, bits, anti); }

    int32_t dims() const { return n_steps * dims_per_step; }                 // the table's; a plan and a QmcRange count steps
    int64_t samples() const { return count * (anti ? 2 : 1); }
    QmcRange range() const { return QmcRange{static_cast<uint64_t>(first), count, n_steps, anti ? 1 : 0}; }

private:
    SobolCall(bool bridge_, int64_t first_, int64_t count_, int32_t n_steps_, int32_t dims_per_step_, const uint32_t* sv_, const uint32_t* shift_,
              int32_t bits_, bool anti_)
        : bridge(bridge_), first(first_), count(count_), n_steps(n_steps_), dims_per_step(dims_per_step_), sv(sv_), shift(shift_), bits(bits_),
          anti(anti_) {}

    static int check(const SobolArgs& a, int32_t dims_per_step) {
        if (a.construction != OLMC_QMC_SEQUENTIAL && a.construction != OLMC_QMC_BRIDGE) return fail(OLMC_ERR_ARG, "bad construction");
        if (a.construction == OLMC_QMC_BRIDGE && a.n_steps > OLMC_QMC_BRIDGE_MAX_STEPS)
            return fail(OLMC_ERR_ARG, "the Brownian-bridge construction takes at most OLMC_QMC_BRIDGE_MAX_STEPS (1024) dates");
        static_assert(OLMC_QMC_BRIDGE_MAX_STEPS == kQmcBridgeMaxSteps, "the header's cap is the kernel's LDS size");
        if (dims_per_step == 2 && (a.n_steps < 1 || a.n_steps > 10600))
            return fail(OLMC_ERR_ARG, "n_steps must be in [1, 10600]: a step takes two of the 21201 Sobol dimensions");
        const int32_t dims = a.n_steps * dims_per_step;
        if (!a.sv || !a.shift) return fail(OLMC_ERR_ARG, "null pointer");
        if (a.bits != kSobolBits) return fail(OLMC_ERR_ARG, "only 30-bit Sobol tables (SciPy's default) are supported");
        if (dims < 1 || dims > 21201) return fail(OLMC_ERR_ARG, "dims must be in [1, 21201]");
        const int rc = check_paths(a.point_offset, a.n_points, dims);
        if (rc) return rc;
        if (a.point_offset + a.n_points > (int64_t(1) << kSobolBits)) return fail(OLMC_ERR_ARG, "at most 2**30 Sobol points");
        return OLMC_OK;
    }
};

// The scrambled direction matrix and digital shift on the device: [dims x 30 | dims] words, uploaded on c's own stream -- the stream
// every launch that reads them is queued on, so no launch sees a table half travelled or one another caller put there.  The table
// travels only when it differs from the one already there (compared word for word: 31 KB at 252 dims, ~1 us, against two pageable
// uploads): the 8 / 14 pricings of literal FD Greeks and every repeated pricing share one upload.  The caller owns c (a lease, or
// a multi-GPU rank's own context).
int qmc_table(DeviceCtx* c, const SobolCall& q, const uint32_t** d_sv, const uint32_t** d_shift) {
    const size_t sv_words = static_cast<size_t>(q.dims()) * kSobolBits;
    const int rc = c->sobol.put(q.sv, sizeof(uint32_t) * sv_words, q.shift, sizeof(uint32_t) * q.dims(), c->stream, [c] { return c->drain(); });
    if (rc) return rc;
    *d_sv = c->sobol.device<uint32_t>();
    *d_shift = *d_sv + sv_words;
    return OLMC_OK;
}

// gbm_qmc.py:38-44 as an olmc_option -> Contract: dt = T / dims, a = ln S + drift dims, vol = sigma sqrt(dt) = make_contract(o, dims)
// Launch shape of a Sobol kernel.  A workgroup takes 64 points and each of its four waves a quarter of the dimensions (from 16
// dimensions on; round 4 drew that line at 2^18 points and ran one point per thread in between); from 2^22 points on a thread takes
// an aligned block of eight consecutive points instead -- from 2^21 below 128 dimensions, 2^20 below 64, 2^19 below 32: a split wave
// has its fixed costs (masks, coefficients, the fold's prologue) to spread over a quarter of the dimensions.  Round 5 re-measured the
// crossover as the aligned split kernel got faster (profiles/r05_ab_kernels.txt, profiles/r05_qmc_grid.txt; split / eight, us):
// 2^19 x 16: 36 / 32, 2^20 x 16: 65 / 48, 2^19 x 32: 52 / 52, 2^20 x 32: 97 / 82, 2^19 x 48: 68 / 73, 2^20 x 48: 128 / 117, 2^20 x 64:
// 158 / 171, 2^21 x 64: 310 / 293, 2^20 x 252: 530 / 638, 2^21 x 252: 1050 / 1107, 2^22 x 252: 2106 / 2074.  OLMC_TUNE_QMC_BLOCK:
// 1 = always eight points per thread, 2 = always split, -1 = never eight and never split (one point per thread).
// A split grid that one launch cannot hold falls back to one point per thread.  The arithmetic is olmc_host_math.h's qmc_launch_shape.
QmcShape qmc_shape(const SobolCall& q) {
    // QmcShape::aligned: split workgroups whose 64 lanes are a 64-ALIGNED block of points fold the high Gray bits' direction numbers once per wave and
    // dimension and keep the inverse normal's coefficients in registers (olmc_kernels.h qmc_point_sum<true>).  The coefficients'
    // load and the fold's prologue are a fixed cost per wave: it pays from 32 dimensions on (8 per wave; 2^17 x 32: 21.5 -> 19.9 us,
    // 2^18 x 48: 44.6 -> 38.4, 2^14 x 32: even; 16 dimensions: 8.6 -> 8.9, 12.0 -> 12.3).  The one-point form is left to launches of
    // fewer than 16 dimensions and to the knob
    return qmc_launch_shape(q.first, q.count, q.dims(), g_qmc_block, g_grid_cap);
}

// The Sobol shape ladder of the European kernels (qmc_shape), MODE kReduce / kControlVariate / kTerminal.
template <int MODE>
void launch_qmc_european(const QmcShape& sh, int32_t grid, hipStream_t s, const EventPair* timed, const QmcRange& qr, const Contract& ct,
                         const uint32_t* d_sv, const uint32_t* d_shift, const ReduceWs& ws, double* terminal) {
    auto go = [&](auto kernel) { launch_timed(kernel, dim3(grid), dim3(kBlock), s, timed, qr, ct, d_sv, d_shift, ws, terminal); };
    if (sh.blocks && sh.aligned8) go(european_qmc_block_kernel<MODE, true>);
    else if (sh.blocks) go(european_qmc_block_kernel<MODE, false>);
    else if (sh.split && sh.aligned) go(european_qmc_kernel<MODE, true, true>);
    else if (sh.split) go(european_qmc_kernel<MODE, true, false>);
    else go(european_qmc_kernel<MODE, false, false>);
}

// The same for the fused batch kernel.
template <int NSETS>
void launch_qmc_batch(const QmcShape& sh, int32_t grid, hipStream_t s, const EventPair* timed, const QmcRange& qr, const ContractSet<NSETS>& cs,
                      const uint32_t* d_sv, const uint32_t* d_shift, const ReduceWs& ws) {
    auto go = [&](auto kernel) { launch_timed(kernel, dim3(grid), dim3(kBlock), s, timed, qr, cs, d_sv, d_shift, ws); };
    if (sh.blocks && sh.aligned8) go(european_qmc_batch_kernel<NSETS, true, false, true>);
    else if (sh.blocks) go(european_qmc_batch_kernel<NSETS, true, false>);
    else if (sh.split && sh.aligned) go(european_qmc_batch_kernel<NSETS, false, true, true>);
    else if (sh.split) go(european_qmc_batch_kernel<NSETS, false, true>);
    else go(european_qmc_batch_kernel<NSETS, false, false>);
}

// gbm_qmc.py:38-44 on `dims` dates (mirror: the antithetic variant, :70).
Contract qmc_contract(double S, double K, double T, double r, double sigma, double q, int is_call, int32_t dims, bool mirror) {
    const GbmStep g = gbm_step(T, dims, r, q, sigma);
    Contract ct;
    ct.vol = g.vol;
    // gbm_qmc.py:44 (drift * steps) vs :70 (the antithetic variant multiplies the rate by T directly)
    ct.a = mirror ? std::log(S) + (r - q - 0.5 * sigma * sigma) * T : std::log(S) + g.drift * dims;
    ct.strike = K;
    ct.sign = is_call ? 1.0 : -1.0;
    ct.scale = 1.0;
    ct.neg_sign_strike = -ct.sign * K;
    ct.sign_scale = ct.sign;
    return ct;
}

// ONE reducing Sobol launch of contract ct over the points of q, queued on c's own stream behind the table: {sum, sumsq} -- the five
// control-variate moments when `five` -- then `tail` at d_out (launch_reduce: blocks when d_out is c->d_result).
int qmc_device(DeviceCtx* c, const Contract& ct, const SobolCall& q, bool five, double* d_out, double tail, bool profiled) {
    const uint32_t *d_sv, *d_shift;
    int rc = qmc_table(c, q, &d_sv, &d_shift);
    if (rc) return rc;
    const QmcRange qr = q.range();
    const QmcShape sh = qmc_shape(q);
    return launch_reduce(c, c->stream, d_out, tail, five ? 5 : 2, sh.grid, [&](int32_t grid, hipStream_t s, const EventPair* timed, const ReduceWs& ws) {
        if (five) launch_qmc_european<kControlVariate>(sh, grid, s, timed, qr, ct, d_sv, d_shift, ws, nullptr);
        else launch_qmc_european<kReduce>(sh, grid, s, timed, qr, ct, d_sv, d_shift, ws, nullptr);
    }, profiled);
}

// One European call on the points of q (its antithetic flag: the terminal values' mirror half): stats at out, the control variate's
// moments at cv, or the terminal values at terminal_host.
int run_qmc(const olmc_option& o, const SobolCall& q, olmc_stats* out, double* terminal_host, olmc_cv_moments* cv = nullptr) {
    CtxLease lease;
    int rc = ctx_lease(&lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    const Contract ct = qmc_contract(o.S, o.K, o.T, o.r, o.sigma, o.q, o.is_call, q.dims(), q.anti);
    if (!terminal_host) {
        rc = qmc_device(c, ct, q, cv != nullptr, c->d_result, -1.0, true);
        if (rc) return rc;
        if (cv) {       // device moments are of the UNdiscounted payoff x; d = disc * x (monte_carlo.py:175)
            cv_from_device(c->h_result, q.count, o.S, o.T, o.r, o.q, cv);
            if (poisoned(o.S, o.K, o.T, o.r, o.sigma, o.q)) cv->value = std::nan("");
            return OLMC_OK;
        }
        finish_one(c->h_result, q.count, o.r, o.T, poisoned(o.S, o.K, o.T, o.r, o.sigma, o.q), out);
        return OLMC_OK;
    }
    const size_t term_bytes = sizeof(double) * static_cast<size_t>(q.samples());
    Carver bulk;
    rc = bulk_reserve(c, term_bytes, &bulk);
    if (rc) return rc;
    const uint32_t *d_sv, *d_shift;
    rc = qmc_table(c, q, &d_sv, &d_shift);
    if (rc) return rc;
    double* d_term = bulk.take<double>(term_bytes / sizeof(double));
    const QmcShape sh = qmc_shape(q);
    // no reduction workspace is handed out: only the launch status matters
    launch_qmc_european<kTerminal>(sh, sh.grid, c->stream, nullptr, q.range(), ct, d_sv, d_shift, ReduceWs{}, d_term);
    HIP_TRY(hipGetLastError());
    c->armed = 0;
    return copy_to_host(c, terminal_host, d_term, term_bytes);
}

// The European family's Sobol call: no construction, `dims` one-dimension steps; then run_qmc.
int run_qmc_checked(const olmc_option& o, const SobolArgs& a, olmc_stats* out, double* terminal_host, olmc_cv_moments* cv = nullptr) {
    int rc;
    const auto q = SobolCall::make(a, 1, &rc);
    return q ? run_qmc(o, *q, out, terminal_host, cv) : rc;
}
}  // namespace

extern "C" int olmc_european_qmc_cv(double S, double K, double T, double r, double sigma, double q, int is_call,
                                    int64_t point_offset, int64_t n_paths, int32_t dims, const uint32_t* sv,
                                    const uint32_t* shift, int32_t bits, olmc_cv_moments* out) {
    if (!out) return fail(OLMC_ERR_ARG, "null pointer");
    return run_qmc_checked(make_option(S, K, T, r, sigma, q, is_call), {OLMC_QMC_SEQUENTIAL, point_offset, n_paths, dims, sv, shift, bits, 0}, nullptr,
                           nullptr, out);
}

extern "C" int olmc_european_qmc(double S, double K, double T, double r, double sigma, double q, int is_call,
                                 int64_t point_offset, int64_t n_paths, int32_t dims, const uint32_t* sv,
                                 const uint32_t* shift, int32_t bits, olmc_stats* out) {
    if (!out) return fail(OLMC_ERR_ARG, "null pointer");
    return run_qmc_checked(make_option(S, K, T, r, sigma, q, is_call), {OLMC_QMC_SEQUENTIAL, point_offset, n_paths, dims, sv, shift, bits, 0}, out,
                           nullptr);
}

extern "C" int olmc_european_qmc_terminal(double S, double T, double r, double sigma, double q, int64_t point_offset,
                                          int64_t n_paths, int32_t dims, const uint32_t* sv, const uint32_t* shift,
                                          int32_t bits, int antithetic, double* out_host) {
    if (!out_host) return fail(OLMC_ERR_ARG, "null pointer");
    return run_qmc_checked(make_option(S, 0.0, T, r, sigma, q, 1), {OLMC_QMC_SEQUENTIAL, point_offset, n_paths, dims, sv, shift, bits, antithetic},
                           nullptr, out_host);
}

// ============================================================ QMC path payoffs ====
namespace {
// The breadth-first Brownian-bridge plan of n dates (include/olmc.h): node k >= 1 is the midpoint m = (a + b) / 2 of the k-th interval
// of length >= 2 taken from the queue that starts with (0, n), with W_m = ca W_a + cb W_b + sd z_k.  Built here once per n and kept on
// the context's device; the kernel reads node k from lane k of a trip (qmc_path_kernel).
int qmc_bridge_plan(DeviceCtx* c, int32_t n, QmcBridgePlan* plan) {
    const size_t ab_bytes = (sizeof(uint32_t) * static_cast<size_t>(n) + 7) & ~size_t(7), bytes = ab_bytes + sizeof(double) * 3 * n;
    const int rc = c->bridge.ensure(n, bytes, c->stream, [c] { return c->drain(); }, [&](unsigned char* host) {
        uint32_t* ab = reinterpret_cast<uint32_t*>(host);
        double* coef = reinterpret_cast<double*>(host + ab_bytes);
        std::vector<std::pair<int32_t, int32_t>> queue{{0, n}};
        int32_t k = 1;
        for (size_t head = 0; head < queue.size(); ++head) {
            const int32_t a = queue[head].first, b = queue[head].second;
            if (b - a < 2) continue;
            const int32_t m = (a + b) / 2;
            if (k >= n) return fail(OLMC_ERR_ARG, "bridge plan overflow");
            ab[k] = static_cast<uint32_t>(a) | (static_cast<uint32_t>(b) << 16);
            coef[k] = static_cast<double>(b - m) / (b - a);
            coef[n + k] = static_cast<double>(m - a) / (b - a);
            coef[2 * n + k] = std::sqrt(static_cast<double>((m - a) * (b - m)) / (b - a));
            ++k;
            queue.emplace_back(a, m);
            queue.emplace_back(m, b);
        }
        if (k != n) return fail(OLMC_ERR_ARG, "bridge plan is incomplete");
        return static_cast<int>(OLMC_OK);
    });
    if (rc) return rc;
    plan->ab = c->bridge.device<uint32_t>();
    plan->coef = reinterpret_cast<const double*>(c->bridge.device<unsigned char>() + ab_bytes);
    return OLMC_OK;
}

// A Sobol path launch on a context the caller holds: the tables (and the bridge plan) on its device, the points, the grid.
struct QmcPathLaunch {
    const uint32_t* d_sv;
    const uint32_t* d_shift;
    QmcBridgePlan plan;
    QmcRange qr;
    int32_t grid;
    bool bridge, anti;
    double inv_steps;
    double* slabs = nullptr;     // the bridge slabs of the Heston and local-volatility kernels (heston_slabs)
};
int qmc_path_setup(DeviceCtx* c, const SobolCall& q, QmcPathLaunch* pl) {
    int rc = qmc_table(c, q, &pl->d_sv, &pl->d_shift);
    if (rc) return rc;
    pl->plan = QmcBridgePlan{nullptr, nullptr};
    pl->bridge = q.bridge;
    if (pl->bridge) {
        rc = qmc_bridge_plan(c, q.n_steps, &pl->plan);
        if (rc) return rc;
    }
    pl->qr = q.range();
    // Workgroups of a QMC path launch: four points in flight per workgroup, grid-striding beyond kQmcPathMaxGrid (olmc_host_math.h:
    // qmc_point_grid) -- every kernel launched on QmcPathLaunch::grid strides, the fused path Greeks included.
    pl->grid = qmc_point_grid(q.count, g_grid_cap);
    pl->anti = q.anti;
    pl->inv_steps = 1.0 / q.n_steps;
    return OLMC_OK;
}

// f(bool_constant<bridge>, bool_constant<anti>) for a launch's construction and antithetic flag.
template <typename F>
void with_bridge_anti(const QmcPathLaunch& pl, F&& f) {
    with_bool(pl.bridge, [&](auto b) { with_bool(pl.anti, [&](auto a) { f(b, a); }); });
}

// f(integral_constant<int, family>) for kQmcAsianArithmetic, kQmcAsianGeometric or (anything else) kQmcExtrema.
template <typename F>
void with_qmc_path_family(int family, F&& f) {
    if (family == kQmcAsianArithmetic) f(std::integral_constant<int, kQmcAsianArithmetic>{});
    else if (family == kQmcAsianGeometric) f(std::integral_constant<int, kQmcAsianGeometric>{});
    else f(std::integral_constant<int, kQmcExtrema>{});
}

// One reducing Sobol path launch of a checked call: the lease, the tables (and the plan), shape(c, q, &pl) -- which may give the launch a
// grid of its own and reserve what it needs on the context --, launch(grid, stream, timed, pl, ws) under the grid reduction with rows
// of nv values, then finish(sums, samples) on the host's copy of the row.
template <typename Shape, typename Launch, typename Finish>
int run_qmc_reduce(const SobolCall& q, int nv, Shape shape, Launch launch, Finish finish) {
    CtxLease lease;
    int rc = ctx_lease(&lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    QmcPathLaunch pl;
    rc = qmc_path_setup(c, q, &pl);
    if (rc) return rc;
    rc = shape(c, q, &pl);
    if (rc) return rc;
    rc = launch_reduce(c, c->stream, c->d_result, -1.0, nv, pl.grid,
                       [&](int32_t g, hipStream_t s, const EventPair* timed, const ReduceWs& ws) { launch(g, s, timed, pl, ws); });
    if (rc) return rc;
    finish(c->h_result, q.samples());
    return OLMC_OK;
}
// The shape of the GBM path kernels: qmc_path_setup's grid, nothing reserved.
inline int qmc_point_shape(DeviceCtx*, const SobolCall&, QmcPathLaunch*) { return OLMC_OK; }
// The finish of one pricing: the statistics of {sum, sumsq}; r_for_discount as run_structured.
auto qmc_stats(double r_for_discount, double T, bool poisoned_inputs, olmc_stats* out) {
    return [=](const double* h, int64_t n) { finish_one(h, n, r_for_discount, T, poisoned_inputs, out); };
}

// family: kQmcAsianArithmetic / kQmcAsianGeometric (payoff ignored) or kQmcExtrema (payoff = kBarrier* / kLookback*, `barrier` its level).
int run_qmc_path(int family, int payoff, const olmc_option& o, double barrier, const SobolArgs& args, olmc_stats* out) {
    if (!out) return fail(OLMC_ERR_ARG, "null pointer");
    int rc;
    const auto q = SobolCall::make(args, 1, &rc);
    if (!q) return rc;
    const ExtremaContract ec = make_extrema(o.S, o.K, o.T, o.r, o.sigma, o.q, o.is_call, family == kQmcExtrema ? payoff : 0, barrier, q->n_steps);
    const bool bad = poisoned(o.S, o.K, o.T, o.r, o.sigma, o.q) || std::isnan(barrier);
    return run_qmc_reduce(*q, 2, qmc_point_shape, [&](int32_t g, hipStream_t s, const EventPair* timed, const QmcPathLaunch& pl, const ReduceWs& ws) {
        with_qmc_path_family(family, [&](auto f) {
            with_bridge_anti(pl, [&](auto b, auto a) {
                launch_timed(qmc_path_kernel<f, b, a>, dim3(g), dim3(kBlock), s, timed, pl.qr, ec, pl.inv_steps, pl.d_sv, pl.d_shift, pl.plan, ws);
            });
        });
    }, qmc_stats(o.r, o.T, bad, out));
}

// The 8 / 14 contracts of compute_greeks_unified over a Sobol-path option (ExoticAdapter, method="qmc") on points [0, n_points), ONE
// launch of qmc_path_greeks_kernel.  Every family is grouped by extrema_greeks_layout in the Sobol normal's unit (1); the Asian
// families have no level (payoff 0, barrier 0: log_barrier_rel 0, unread).
int run_qmc_path_greeks(int family, int payoff, const olmc_option& o, double barrier, const SobolArgs& args, int second_order, double* out9,
                        olmc_stats* evals) {
    if (!out9) return fail(OLMC_ERR_ARG, "null pointer");
    if (!(o.T > 0.0)) return fail(OLMC_ERR_ARG, "T must be > 0");
    int rc;
    const auto q = SobolCall::make(args, 1, &rc);
    if (!q) return rc;
    const GreeksSet gs(o.S, o.K, o.T, o.r, o.sigma, o.q, o.is_call, second_order);
    ExtremaGreeksSet es;
    if (const char* bad = extrema_greeks_layout(gs, q->n_steps, payoff, barrier, o.K, o.is_call, &es, 1.0)) return fail(OLMC_ERR_STATE, bad);
    const int nsets = gs.nsets();
    return run_qmc_reduce(*q, 2 * nsets, qmc_point_shape, [&](int32_t g, hipStream_t s, const EventPair* timed, const QmcPathLaunch& pl, const ReduceWs& ws) {
        with_qmc_path_family(family, [&](auto f) {
            with_bool(pl.bridge, [&](auto b) {
                with_set_anti(nsets, pl.anti, [&](auto width, auto a) {
                    launch_timed(qmc_path_greeks_kernel<f, b, a, width>, dim3(g), dim3(kBlock), s, timed, pl.qr, es, pl.inv_steps, pl.d_sv, pl.d_shift,
                                 pl.plan, ws);
                });
            });
        });
    }, [&](const double* h, int64_t n) {
        olmc_stats st[OLMC_MAX_BATCH];
        finish_set(h, nullptr, n, gs.o, gs.k, false, false, st);
        gs.finish(st, o.T, out9, evals);
    });
}
}  // namespace

extern "C" int olmc_asian_qmc(double S, double K, double T, double r, double sigma, double q, int is_call, int avg_kind, int construction,
                              int64_t point_offset, int64_t n_points, int32_t n_steps, const uint32_t* sv, const uint32_t* shift, int32_t bits,
                              int antithetic, olmc_stats* out) {
    if (avg_kind != OLMC_AVG_ARITHMETIC && avg_kind != OLMC_AVG_GEOMETRIC) return fail(OLMC_ERR_ARG, "bad avg_kind (arithmetic or geometric)");
    return run_qmc_path(avg_kind == OLMC_AVG_GEOMETRIC ? kQmcAsianGeometric : kQmcAsianArithmetic, 0, make_option(S, K, T, r, sigma, q, is_call), 0.0,
                        {construction, point_offset, n_points, n_steps, sv, shift, bits, antithetic}, out);
}

extern "C" int olmc_extrema_qmc(double S, double K, double T, double r, double sigma, double q, int is_call, int payoff, double barrier,
                                int construction, int64_t point_offset, int64_t n_points, int32_t n_steps, const uint32_t* sv,
                                const uint32_t* shift, int32_t bits, int antithetic, olmc_stats* out) {
    if (payoff < OLMC_BARRIER_UP_OUT || payoff > OLMC_LOOKBACK_FIXED) return fail(OLMC_ERR_ARG, "bad payoff");
    if (payoff <= OLMC_BARRIER_DOWN_IN && !(barrier > 0.0)) return fail(OLMC_ERR_ARG, "Barrier must be positive");
    return run_qmc_path(kQmcExtrema, payoff, make_option(S, K, T, r, sigma, q, is_call), payoff <= OLMC_BARRIER_DOWN_IN ? barrier : 0.0,
                        {construction, point_offset, n_points, n_steps, sv, shift, bits, antithetic}, out);
}

extern "C" int olmc_asian_qmc_greeks_fd(double S, double K, double T, double r, double sigma, double q, int is_call, int avg_kind,
                                        int construction, int64_t n_points, int32_t n_steps, const uint32_t* sv, const uint32_t* shift,
                                        int32_t bits, int antithetic, int second_order, double* out9, olmc_stats* evals) {
    if (avg_kind != OLMC_AVG_ARITHMETIC && avg_kind != OLMC_AVG_GEOMETRIC)
        return fail(OLMC_ERR_ARG, "bad avg_kind (arithmetic or geometric: the fp32-exponent form has no Sobol path)");
    return run_qmc_path_greeks(avg_kind == OLMC_AVG_GEOMETRIC ? kQmcAsianGeometric : kQmcAsianArithmetic, 0, make_option(S, K, T, r, sigma, q, is_call),
                               0.0, {construction, 0, n_points, n_steps, sv, shift, bits, antithetic}, second_order, out9, evals);
}

extern "C" int olmc_extrema_qmc_greeks_fd(double S, double K, double T, double r, double sigma, double q, int is_call, int payoff, double barrier,
                                          int construction, int64_t n_points, int32_t n_steps, const uint32_t* sv, const uint32_t* shift,
                                          int32_t bits, int antithetic, int second_order, double* out9, olmc_stats* evals) {
    if (payoff < OLMC_BARRIER_UP_OUT || payoff > OLMC_LOOKBACK_FIXED) return fail(OLMC_ERR_ARG, "bad payoff");
    if (payoff <= OLMC_BARRIER_DOWN_IN && !(barrier > 0.0)) return fail(OLMC_ERR_ARG, "Barrier must be positive");
    return run_qmc_path_greeks(kQmcExtrema, payoff, make_option(S, K, T, r, sigma, q, is_call), payoff <= OLMC_BARRIER_DOWN_IN ? barrier : 0.0,
                               {construction, 0, n_points, n_steps, sv, shift, bits, antithetic}, second_order, out9, evals);
}

// The autocallable and the cliquet on the Sobol paths of run_qmc_path (include/olmc.h "quasi-Monte Carlo structured products"): the
// contracts of olmc_autocallable / olmc_cliquet, the checks of both sides before any device work.
namespace {
// m with j / d == (2 j m) >> 32 for 0 <= j, d < 2^15 (qmc_date_quotient in olmc_kernels.h has the proof).
uint32_t qmc_date_magic(int32_t d) { return static_cast<uint32_t>((uint64_t(1) << 31) / static_cast<uint64_t>(d)) + 1u; }
}  // namespace

extern "C" int olmc_autocallable_qmc(double S, double T, double r, double sigma, double q, double autocall_barrier, double coupon_barrier,
                                     double coupon_rate, double ki_barrier, int32_t observation_freq, int construction,
                                     int64_t point_offset, int64_t n_points, int32_t n_steps, const uint32_t* sv, const uint32_t* shift,
                                     int32_t bits, int antithetic, olmc_stats* out) {
    if (!out) return fail(OLMC_ERR_ARG, "null pointer");
    int rc;
    const auto call = SobolCall::make({construction, point_offset, n_points, n_steps, sv, shift, bits, antithetic}, 1, &rc);
    if (!call) return rc;
    rc = autocall_check(observation_freq, n_steps);
    if (rc) return rc;
    const AutocallSetup a = make_autocall(S, T, r, sigma, q, autocall_barrier, coupon_barrier, coupon_rate, ki_barrier, observation_freq, n_steps);
    const uint32_t magic = qmc_date_magic(observation_freq);
    // payoffs are already discounted path by path, as olmc_autocallable's: no outer discount
    return run_qmc_reduce(*call, 2, qmc_point_shape, [&](int32_t g, hipStream_t s, const EventPair* timed, const QmcPathLaunch& pl, const ReduceWs& ws) {
        with_bridge_anti(pl, [&](auto b, auto m) {
            launch_timed(qmc_autocall_kernel<b, m>, dim3(g), dim3(kBlock), s, timed, pl.qr, a.ac, a.obs_rate, magic, pl.d_sv, pl.d_shift, pl.plan, ws);
        });
    }, qmc_stats(0.0, T, a.bad, out));
}

extern "C" int olmc_cliquet_qmc(double S, double T, double r, double sigma, double q, double local_cap, double local_floor, double global_cap,
                                double global_floor, int32_t n_periods, int construction, int64_t point_offset, int64_t n_points,
                                int32_t n_steps, const uint32_t* sv, const uint32_t* shift, int32_t bits, int antithetic, olmc_stats* out) {
    if (!out) return fail(OLMC_ERR_ARG, "null pointer");
    int rc;
    const auto call = SobolCall::make({construction, point_offset, n_points, n_steps, sv, shift, bits, antithetic}, 1, &rc);
    if (!call) return rc;
    rc = cliquet_check(n_periods, n_steps);
    if (rc) return rc;
    const CliquetContract cc = make_cliquet(S, T, r, sigma, q, local_cap, local_floor, global_cap, global_floor, n_periods, n_steps);
    const uint32_t magic = qmc_date_magic(cc.steps_per_period);
    const bool bad = cliquet_poisoned(S, T, r, sigma, q, local_cap, local_floor, global_cap, global_floor);
    return run_qmc_reduce(*call, 2, qmc_point_shape, [&](int32_t g, hipStream_t s, const EventPair* timed, const QmcPathLaunch& pl, const ReduceWs& ws) {
        with_bridge_anti(pl, [&](auto b, auto m) {
            launch_timed(qmc_cliquet_kernel<b, m>, dim3(g), dim3(kBlock), s, timed, pl.qr, cc, magic, pl.d_sv, pl.d_shift, pl.plan, ws);
        });
    }, qmc_stats(r, T, bad, out));
}

// ================================================================ QMC path matrix ====
namespace {
// The lease of a Sobol path-matrix call, after its Sobol checks: matrix_prologue with the call's `bytes` (reserved when `reserve`) --
// every refusal before any device work.
int qmc_matrix_prologue(const SobolCall& q, double bytes, CtxLease* lease, bool reserve = true) {
    return matrix_prologue(q.count, q.n_steps, bytes, "path matrix would exceed 64 GB: lower n_paths or n_steps", lease, reserve);
}

// Workgroups of a lanes-over-points launch: one wave per block of 64 points that the call touches, aligned in the absolute point
// index, grid-striding beyond kQmcPathMaxGrid.
int32_t qmc_block_grid(const SobolCall& q) { return qmc_blocks_grid((q.first + q.count - 1) / kWave - q.first / kWave + 1, g_grid_cap); }

// The set-up of a path-matrix launch: the tables, the plan and the range of qmc_path_setup, the grid over the blocks of 64 points.
int qmc_matrix_setup(DeviceCtx* c, const SobolCall& q, QmcPathLaunch* pl) {
    const int rc = qmc_path_setup(c, q, pl);
    pl->grid = qmc_block_grid(q);
    return rc;
}

// The points of q as the path matrix d_paths (lsm_qmc_paths_kernel), queued on c's stream behind the tables and the plan.
int qmc_matrix(DeviceCtx* c, const SobolCall& q, const LsmContract& lc, bool path_major, double* d_paths) {
    QmcPathLaunch pl;
    const int rc = qmc_matrix_setup(c, q, &pl);
    if (rc) return rc;
    with_bool(pl.bridge, [&](auto b) {
        with_bool(path_major, [&](auto pm) {
            launch_timed(lsm_qmc_paths_kernel<b, pm>, dim3(pl.grid), dim3(kBlock), c->stream, nullptr, pl.qr, lc, pl.d_sv, pl.d_shift, pl.plan, d_paths);
        });
    });
    HIP_TRY(hipGetLastError());
    return OLMC_OK;
}
}  // namespace

extern "C" int olmc_american_lsm_qmc(double S, double K, double T, double r, double sigma, double q, int is_call, int construction,
                                     int64_t n_points, int32_t n_steps, const uint32_t* sv, const uint32_t* shift, int32_t bits,
                                     int32_t poly_degree, olmc_stats* out) {
    if (!out) return fail(OLMC_ERR_ARG, "null pointer");
    if (poly_degree < 1 || poly_degree > kLsmMaxDegree) return fail(OLMC_ERR_ARG, "poly_degree must be in [1, 4]");
    int rc;
    const auto call = SobolCall::make({construction, 0, n_points, n_steps, sv, shift, bits, 0}, 1, &rc);
    if (!call) return rc;
    CtxLease lease;
    rc = qmc_matrix_prologue(*call, lsm_bytes(n_points, n_steps), &lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    Carver bulk = c->bulk.carve();
    double* d_paths = bulk.take<double>((static_cast<size_t>(n_steps) + 1) * n_points);  // [n_steps + 1][n_points], then olmc_american_lsm's buffers
    const LsmContract lc = lsm_contract(S, K, T, r, sigma, q, is_call, n_steps, poly_degree);
    EventPair ep{};
    if (g_profile) { rc = prof_begin(c, c->stream, &ep); if (rc) return rc; }
    rc = qmc_matrix(c, *call, lc, false, d_paths);
    if (rc) return rc;
    rc = lsm_chain(c, S, K, T, r, sigma, q, is_call, lc, n_points, n_steps, d_paths, &bulk);
    if (rc) return rc;
    if (g_profile) { rc = prof_end(c, c->stream, ep); if (rc) return rc; }
    finish_one(c->h_result, n_points, 0.0, T, poisoned(S, K, T, r, sigma, q), out);
    return OLMC_OK;
}

extern "C" int olmc_exercise_boundary_qmc(double S, double K, double T, double r, double sigma, double q, int is_call, int construction,
                                          int64_t n_points, int32_t n_steps, const uint32_t* sv, const uint32_t* shift, int32_t bits,
                                          double* boundary_host) {
    if (!boundary_host) return fail(OLMC_ERR_ARG, "null pointer");
    const size_t rows = static_cast<size_t>(n_steps) + 1;
    const double bytes = 8.0 * static_cast<double>(n_points) * (n_steps + 1.0);
    int rc;
    const auto call = SobolCall::make({construction, 0, n_points, n_steps, sv, shift, bits, 0}, 1, &rc);
    if (!call) return rc;
    CtxLease lease;
    rc = qmc_matrix_prologue(*call, bytes, &lease, false);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    const size_t path_bytes = (static_cast<size_t>(bytes) + 255) / 256 * 256;
    Carver bulk;
    rc = bulk_reserve(c, path_bytes + rows * sizeof(double), &bulk);
    if (rc) return rc;
    double* d_paths = bulk.take<double>(path_bytes / sizeof(double));
    double* d_boundary = bulk.take<double>(rows);
    rc = qmc_matrix(c, *call, lsm_contract(S, K, T, r, sigma, q, is_call, n_steps, 1), false, d_paths);
    if (rc) return rc;
    // as olmc_exercise_boundary: np.percentile(x, 10) for a put, 90 for a call (exotic_options.py:337-341)
    hipLaunchKernelGGL(exercise_boundary_kernel, dim3(static_cast<uint32_t>(rows)), dim3(kBoundaryThreads), 0, c->stream, d_paths, n_points, K,
                       is_call ? 1.0 : -1.0, (is_call ? 90.0 : 10.0) / 100.0, d_boundary);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(boundary_host, d_boundary, rows * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return OLMC_OK;
}

extern "C" int olmc_gbm_qmc_paths(double S, double T, double r, double sigma, double q, int construction, int64_t n_points, int32_t n_steps,
                                  const uint32_t* sv, const uint32_t* shift, int32_t bits, int path_major, double* out_host) {
    if (!out_host) return fail(OLMC_ERR_ARG, "null pointer");
    const double bytes = 8.0 * static_cast<double>(n_points) * (n_steps + 1.0);
    int rc;
    const auto call = SobolCall::make({construction, 0, n_points, n_steps, sv, shift, bits, 0}, 1, &rc);
    if (!call) return rc;
    CtxLease lease;
    rc = qmc_matrix_prologue(*call, bytes, &lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    LsmContract lc = lsm_contract(S, S, T, r, sigma, q, 0, n_steps, 1);            // no strike: only the path fields are read
    lc.s_first = S;                                                     // the export's column 0 is S itself, as olmc_gbm_paths'
    rc = qmc_matrix(c, *call, lc, path_major != 0, c->bulk.as<double>());
    if (rc) return rc;
    return copy_to_host(c, out_host, c->bulk.get(), static_cast<size_t>(bytes));
}

// ================================================================ Heston on Sobol paths ====
// olmc_heston / olmc_heston_paths on scrambled-Sobol points (include/olmc.h "quasi-Monte Carlo Heston"): their contract and model
// checks, the table / construction / point-range checks of the other Sobol path calls with two dimensions per step.
namespace {
// The bridge slabs of heston_qmc_kernel / heston_qmc_path_kernel on c: one [2 n][64] slab per RESIDENT wave.  The grid is cut to the workgroups the device holds
// at once (kHestonBridgeBlocksPerCu per CU = two waves per SIMD, of the four its 109-117 VGPRs allow; heston_qmc_path_kernel's 113-131 allow
// three or four) and strides over the blocks beyond, and
// the slabs of a launch stay under kHestonSlabCap (the grid shrinks further): the buffer follows the device and n, not the number of
// points -- 0.5 GiB at 252 steps and 1 GiB from 504 steps on with 256 CUs, kept with the context.
// The sizes are olmc_host_math.h's heston_slab_shape.
int heston_slabs(DeviceCtx* c, int32_t n_steps, int32_t* grid, int32_t factors = 2) {
    const HestonSlabs hs = heston_slab_shape(n_steps, *grid, c->cus, factors);
    *grid = hs.grid;
    return c->heston_w.reserve(hs.bytes, [c] { return c->drain(); });      // a launch may still walk the old slabs
}

// run_qmc_reduce's shape of a Heston price launch (heston_qmc_kernel, heston_qmc_path_kernel): the grid over the blocks of 64 points,
// aligned in the absolute point index, and for the bridge its slabs.
int heston_qmc_shape(DeviceCtx* c, const SobolCall& q, QmcPathLaunch* pl) {
    pl->grid = qmc_block_grid(q);
    pl->slabs = nullptr;
    if (!pl->bridge) return OLMC_OK;
    const int rc = heston_slabs(c, q.n_steps, &pl->grid, q.dims_per_step);
    pl->slabs = c->heston_w.as<double>();
    return rc;
}

// Sobol: every (S, v) state of points [0, n_points) of the scheme's construction.
template <typename Scheme>
int run_heston_qmc_paths(double S, double T, double r, double q, const HestonModel& m, const SobolArgs& args, int path_major, double* spot_host,
                         double* var_host) {
    if (!spot_host || !var_host) return fail(OLMC_ERR_ARG, "null pointer");
    int rc = heston_qmc_scheme_check<Scheme>(m, args.construction);
    if (rc) return rc;
    const auto call = SobolCall::make(args, 2, &rc);
    if (!call) return rc;
    const double bytes = 8.0 * static_cast<double>(call->count) * (call->n_steps + 1.0);
    CtxLease lease;
    rc = qmc_matrix_prologue(*call, 2 * bytes, &lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    const auto hc = Scheme::make(S, T, r, q, 1, m, call->n_steps);
    QmcPathLaunch pl;
    rc = qmc_matrix_setup(c, *call, &pl);
    if (rc) return rc;
    return heston_path_matrices(c, call->count, call->n_steps, spot_host, var_host, [&](const EventPair* timed, double* d_spot, double* d_var) {
        with_bool(path_major != 0, [&](auto pm) {
            if constexpr (Scheme::kBridge) {
                with_bool(pl.bridge, [&](auto b) {
                    launch_timed(heston_qmc_paths_kernel<b, pm>, dim3(pl.grid), dim3(kBlock), c->stream, timed, pl.qr, hc, S, pl.d_sv, pl.d_shift, pl.plan,
                                 d_spot, d_var);
                });
            } else {
                launch_timed(heston_qe_qmc_paths_kernel<pm>, dim3(pl.grid), dim3(kBlock), c->stream, timed, pl.qr, hc, S, pl.d_sv, pl.d_shift, d_spot, d_var);
            }
        });
    });
}
}  // namespace

extern "C" int olmc_heston_qmc(double S, double K, double T, double r, double q, int is_call, double kappa, double theta, double sigma_v,
                               double rho, double v0, int construction, int64_t point_offset, int64_t n_points, int32_t n_steps,
                               const uint32_t* sv, const uint32_t* shift, int32_t bits, int antithetic, olmc_stats* out) {
    if (!out) return fail(OLMC_ERR_ARG, "null pointer");
    const HestonModel hm{kappa, theta, sigma_v, rho, v0};
    int rc = heston_check(hm);
    if (rc) return rc;
    const auto call = SobolCall::make({construction, point_offset, n_points, n_steps, sv, shift, bits, antithetic}, 2, &rc);
    if (!call) return rc;
    const HestonContract hc = make_heston(S, K, T, r, q, is_call, hm, n_steps);
    const bool bad = heston_poisoned(S, K, T, r, q, hm);
    return run_qmc_reduce(*call, 2, heston_qmc_shape, [&](int32_t g, hipStream_t s, const EventPair* timed, const QmcPathLaunch& pl, const ReduceWs& ws) {
        with_bridge_anti(pl, [&](auto b, auto m) {
            launch_timed(heston_qmc_kernel<b, m>, dim3(g), dim3(kBlock), s, timed, pl.qr, hc, pl.d_sv, pl.d_shift, pl.plan, pl.slabs, ws);
        });
    }, qmc_stats(r, T, bad, out));
}

extern "C" int olmc_heston_qmc_paths(double S, double T, double r, double q, double kappa, double theta, double sigma_v, double rho, double v0,
                                     int construction, int64_t n_points, int32_t n_steps, const uint32_t* sv, const uint32_t* shift,
                                     int32_t bits, int path_major, double* spot_host, double* var_host) {
    return run_heston_qmc_paths<HestonEuler>(S, T, r, q, {kappa, theta, sigma_v, rho, v0}, {construction, 0, n_points, n_steps, sv, shift, bits, 0},
                                             path_major, spot_host, var_host);
}

// ============================================================ path payoffs under Heston ====
// Asian, barrier and lookback payoffs on olmc_heston's and olmc_heston_qmc's paths (include/olmc.h "path payoffs under Heston"): their
// contract, model and range checks, one launch of heston_path_kernel / heston_qmc_path_kernel.
namespace {
bool heston_path_is_barrier(int payoff) { return payoff <= OLMC_BARRIER_DOWN_IN; }
// The payoff codes of a family end at last_code: OLMC_PATH_ASIAN_GEOMETRIC here, the family's own European (OLLV_EUROPEAN, OLJD_EUROPEAN)
// where it has one.
int path_payoff_check(int payoff, double barrier, int last_code) {
    if (payoff < OLMC_BARRIER_UP_OUT || payoff > last_code) return fail(OLMC_ERR_ARG, "bad payoff");
    if (heston_path_is_barrier(payoff) && barrier <= 0.0) return fail(OLMC_ERR_ARG, "Barrier must be positive");
    return OLMC_OK;
}
int heston_path_family(int payoff) {
    return payoff == OLMC_PATH_ASIAN_ARITHMETIC ? kQmcAsianArithmetic : payoff == OLMC_PATH_ASIAN_GEOMETRIC ? kQmcAsianGeometric : kQmcExtrema;
}

// What the payoff reads of an ExtremaContract (no drift, no vol: the model is the HestonContract's).  Date 0 of the reference's matrix is
// the spot S itself, so a barrier's date-0 decision is the plain comparison S >= B (up) / S <= B (down), made here: a barrier hit at date
// 0 becomes a level every running extremum meets, and one not hit a level strictly beyond the running extrema's start (ln(S_0 / S) = 0),
// also where ln(B / S) rounds to 0.  Later dates compare ln(S_t / S) with ln(B / S).
ExtremaContract heston_path_contract(double S, double K, int is_call, int payoff, double barrier) {
    ExtremaContract ec;
    ec.s0 = S;
    ec.log_barrier_rel = 0.0;
    if (heston_path_is_barrier(payoff)) {
        const bool up = payoff <= OLMC_BARRIER_UP_IN;
        const double inf = std::numeric_limits<double>::infinity(), tiny = std::numeric_limits<double>::min();
        const double lb = std::log(barrier / S);
        if (up) ec.log_barrier_rel = S >= barrier ? -inf : (lb > 0.0 ? lb : tiny);
        else ec.log_barrier_rel = S <= barrier ? inf : (lb < 0.0 ? lb : -tiny);
    }
    ec.drift = 0.0;
    ec.vol = 0.0;
    ec.strike = K;
    ec.sign = is_call ? 1.0 : -1.0;
    ec.payoff = heston_path_family(payoff) == kQmcExtrema ? payoff : 0;
    ec.pad = 0;
    return ec;
}

// The kernels' contract of a checked payoff code and whether a NaN barrier poisons the result.  A code beyond the Heston payoffs is a
// family's European: like the arithmetic Asian it reads no level and no payoff code.
struct PathPayoff {
    ExtremaContract ec;
    bool nan_barrier;
};
PathPayoff path_payoff(double S, double K, int is_call, int payoff, double barrier) {
    return {heston_path_contract(S, K, is_call, payoff > OLMC_PATH_ASIAN_GEOMETRIC ? OLMC_PATH_ASIAN_ARITHMETIC : payoff, barrier),
            heston_path_is_barrier(payoff) && std::isnan(barrier)};
}

// f(integral_constant<int, family>) for the family of a checked payoff code.
template <typename F>
void with_heston_path_family(int payoff, F&& f) {
    with_qmc_path_family(heston_path_family(payoff), f);
}

// The same for a family that has a European at european_code (kPathEuropean).
template <typename F>
void with_path_family(int payoff, int european_code, F&& f) {
    if (payoff == european_code) f(std::integral_constant<int, kPathEuropean>{});
    else with_heston_path_family(payoff, f);
}
}  // namespace

extern "C" int olmc_heston_path_payoff(double S, double K, double T, double r, double q, int is_call, double kappa, double theta, double sigma_v,
                                       double rho, double v0, int payoff, double barrier, int64_t path_offset, int64_t n_local, int32_t n_steps,
                                       uint64_t seed, int antithetic, olmc_stats* out) {
    if (!out) return fail(OLMC_ERR_ARG, "null pointer");
    const HestonModel hm{kappa, theta, sigma_v, rho, v0};
    int rc = heston_check(hm);
    if (rc) return rc;
    rc = path_payoff_check(payoff, barrier, OLMC_PATH_ASIAN_GEOMETRIC);
    if (rc) return rc;
    const HestonContract hc = make_heston(S, K, T, r, q, is_call, hm, n_steps);
    const PathPayoff pp = path_payoff(S, K, is_call, payoff, barrier);
    const bool bad = heston_poisoned(S, K, T, r, q, hm) || pp.nan_barrier;
    const double inv_steps = 1.0 / n_steps;                  // n_steps < 1 is refused by run_structured before any launch
    return run_structured(path_offset, n_local, n_steps, seed, antithetic, r, T, bad, out,
                          [&](int32_t grid, hipStream_t st, const EventPair* timed, const PathRange& pr, const ReduceWs& ws) {
                              with_heston_path_family(payoff, [&](auto f) {
                                  with_bool(antithetic != 0, [&](auto a) {
                                      launch_timed(heston_path_kernel<f, a>, dim3(grid), dim3(kBlock), st, timed, pr, hc, pp.ec, inv_steps, ws);
                                  });
                              });
                          });
}

extern "C" int olmc_heston_qmc_path_payoff(double S, double K, double T, double r, double q, int is_call, double kappa, double theta, double sigma_v,
                                           double rho, double v0, int payoff, double barrier, int construction, int64_t point_offset,
                                           int64_t n_points, int32_t n_steps, const uint32_t* sv, const uint32_t* shift, int32_t bits,
                                           int antithetic, olmc_stats* out) {
    if (!out) return fail(OLMC_ERR_ARG, "null pointer");
    const HestonModel hm{kappa, theta, sigma_v, rho, v0};
    int rc = heston_check(hm);
    if (rc) return rc;
    rc = path_payoff_check(payoff, barrier, OLMC_PATH_ASIAN_GEOMETRIC);
    if (rc) return rc;
    const auto call = SobolCall::make({construction, point_offset, n_points, n_steps, sv, shift, bits, antithetic}, 2, &rc);
    if (!call) return rc;
    const HestonContract hc = make_heston(S, K, T, r, q, is_call, hm, n_steps);
    const PathPayoff pp = path_payoff(S, K, is_call, payoff, barrier);
    const bool bad = heston_poisoned(S, K, T, r, q, hm) || pp.nan_barrier;
    return run_qmc_reduce(*call, 2, heston_qmc_shape, [&](int32_t g, hipStream_t s, const EventPair* timed, const QmcPathLaunch& pl, const ReduceWs& ws) {
        with_heston_path_family(payoff, [&](auto f) {
            with_bridge_anti(pl, [&](auto b, auto m) {
                launch_timed(heston_qmc_path_kernel<f, b, m>, dim3(g), dim3(kBlock), s, timed, pl.qr, hc, pp.ec, pl.inv_steps, pl.d_sv, pl.d_shift, pl.plan,
                             pl.slabs, ws);
            });
        });
    }, qmc_stats(r, T, bad, out));
}

// ====================================================== a Heston option surface ====
// European payoffs at k (strike, step) cells on the paths of olmc_heston / olmc_heston_qmc (include/olmc.h "a Heston option surface"):
// one launch of heston_surface_kernel / heston_qmc_surface_kernel, the cells sorted by step for the kernel and answered in the caller's
// order.
namespace {
static_assert(kSurfaceCells == OLMC_MAX_BATCH && 2 * kSurfaceCells <= kMaxNV, "a surface launch's row is OLMC_MAX_BATCH pairs wide");

struct SurfaceOrder {
    HestonSurfaceCells cells;
    int32_t slot_of[OLMC_MAX_BATCH];     // caller's cell i sits at the kernel's slot slot_of[i]
};

// The checks of the cell list (after n_steps is known to be >= 1), then the cells by ascending step; equal steps keep the caller's order.
int surface_cells(const double* strikes, const int32_t* steps, int32_t k, int32_t n_steps, SurfaceOrder* so) {
    if (k < 1 || k > OLMC_MAX_BATCH) return fail(OLMC_ERR_ARG, "the number of cells must be in [1, OLMC_MAX_BATCH]");
    for (int32_t i = 0; i < k; ++i)
        if (steps[i] < 1 || steps[i] > n_steps) return fail(OLMC_ERR_ARG, "a cell's step must be in [1, n_steps]");
    int32_t order[OLMC_MAX_BATCH];
    for (int32_t i = 0; i < k; ++i) order[i] = i;
    std::stable_sort(order, order + k, [&](int32_t a, int32_t b) { return steps[a] < steps[b]; });
    for (int32_t j = 0; j < kSurfaceCells; ++j) {
        so->cells.strike[j] = j < k ? strikes[order[j]] : 0.0;
        so->cells.step[j] = j < k ? steps[order[j]] : INT32_MAX;
        if (j < k) so->slot_of[order[j]] = j;
    }
    so->cells.k = k;
    so->cells.last = steps[order[k - 1]];
    return OLMC_OK;
}

// Cell i's stats from the launch's sums: discounted at the grid's time of its step; a NaN strike poisons its own cell, `bad` all of them.
void surface_finish(const double* h, const SurfaceOrder& so, const double* strikes, const int32_t* steps, int32_t k, int64_t n, double r,
                    double dt, bool bad, olmc_stats* out) {
    for (int32_t i = 0; i < k; ++i) {
        const int32_t j = so.slot_of[i];
        if (bad || std::isnan(strikes[i])) nan_stats(n, &out[i]);
        else finish_stats(h[2 * j], h[2 * j + 1], n, r, steps[i] * dt, &out[i]);
    }
}

// Philox: the cells on paths [path_offset, path_offset + n_local) of a family's stream, after the caller's null and model checks: the
// range, the cells, the lease, `setup(c)` (the family's per-context hook: the local-volatility table), one launch of the family's
// surface kernel -- launch(grid, stream, timed, range, cells, ws) --, the cells' stats.
struct PhiloxShard {
    int64_t path_offset, n_local;
    int32_t n_steps;
    uint64_t seed;
    int antithetic;
};
template <typename Setup, typename Launch>
int run_philox_surface(const double* strikes, const int32_t* steps, int32_t k, const PhiloxShard& sh, double r, double T, bool bad, olmc_stats* out,
                       Setup setup, Launch launch) {
    int rc = check_paths(sh.path_offset, sh.n_local, sh.n_steps);
    if (rc) return rc;
    SurfaceOrder so;
    rc = surface_cells(strikes, steps, k, sh.n_steps, &so);
    if (rc) return rc;
    CtxLease lease;
    rc = ctx_lease(&lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    rc = setup(c);
    if (rc) return rc;
    const PathRange pr = make_range(sh.path_offset, sh.n_local, sh.n_steps, sh.seed);
    rc = launch_reduce(c, c->stream, c->d_result, -1.0, 2 * kSurfaceCells, grid_for(sh.n_local),
                       [&](int32_t grid, hipStream_t st, const EventPair* timed, const ReduceWs& ws) {
                           launch(grid, st, timed, pr, so.cells, ws);
                       });
    if (rc) return rc;
    surface_finish(c->h_result, so, strikes, steps, k, sh.n_local * (sh.antithetic ? 2 : 1), r, T / sh.n_steps, bad, out);
    return OLMC_OK;
}

template <typename Scheme>
int run_heston_surface(double S, double T, double r, double q, int is_call, const HestonModel& m, const double* strikes, const int32_t* steps,
                       int32_t k, const PhiloxShard& sh, olmc_stats* out) {
    if (!strikes || !steps || !out) return fail(OLMC_ERR_ARG, "null pointer");
    const int rc = Scheme::check(m);
    if (rc) return rc;
    return run_philox_surface(strikes, steps, k, sh, r, T, heston_poisoned(S, 0.0, T, r, q, m), out, no_setup,
                              [&](int32_t grid, hipStream_t st, const EventPair* timed, const PathRange& pr, const HestonSurfaceCells& cells,
                                  const ReduceWs& ws) {
        const auto hc = Scheme::make(S, T, r, q, is_call, m, sh.n_steps);
        with_bool(sh.antithetic != 0, [&](auto a) {
            launch_timed(Scheme::template surface_kernel<decltype(a)::value>(), dim3(grid), dim3(kBlock), st, timed, pr, hc, cells, ws);
        });
    });
}

// Sobol: the cells on points [point_offset, point_offset + n_points) of the scheme's construction; the shape of a Heston price launch
// (without the bridge: the grid over the aligned blocks, no slabs).
template <typename Scheme>
int run_heston_qmc_surface(double S, double T, double r, double q, int is_call, const HestonModel& m, const double* strikes, const int32_t* steps,
                           int32_t k, const SobolArgs& args, olmc_stats* out) {
    if (!strikes || !steps || !out) return fail(OLMC_ERR_ARG, "null pointer");
    int rc = heston_qmc_scheme_check<Scheme>(m, args.construction);
    if (rc) return rc;
    const auto call = SobolCall::make(args, 2, &rc);
    if (!call) return rc;
    const int32_t n_steps = call->n_steps;
    SurfaceOrder so;
    rc = surface_cells(strikes, steps, k, n_steps, &so);
    if (rc) return rc;
    const auto hc = Scheme::make(S, T, r, q, is_call, m, n_steps);
    const bool bad = heston_poisoned(S, 0.0, T, r, q, m);
    return run_qmc_reduce(*call, 2 * kSurfaceCells, heston_qmc_shape,
                          [&](int32_t g, hipStream_t s, const EventPair* timed, const QmcPathLaunch& pl, const ReduceWs& ws) {
        with_bool(pl.anti, [&](auto a) {
            if constexpr (Scheme::kBridge) {
                with_bool(pl.bridge, [&](auto b) {
                    launch_timed(heston_qmc_surface_kernel<b, a>, dim3(g), dim3(kBlock), s, timed, pl.qr, hc, so.cells, pl.d_sv, pl.d_shift, pl.plan,
                                 pl.slabs, ws);
                });
            } else {
                launch_timed(heston_qe_qmc_surface_kernel<a>, dim3(g), dim3(kBlock), s, timed, pl.qr, hc, so.cells, pl.d_sv, pl.d_shift, ws);
            }
        });
    }, [&](const double* h, int64_t n) { surface_finish(h, so, strikes, steps, k, n, r, T / n_steps, bad, out); });
}
}  // namespace

extern "C" int olmc_heston_surface(double S, double T, double r, double q, int is_call, double kappa, double theta, double sigma_v, double rho,
                                   double v0, const double* strikes, const int32_t* steps, int32_t k, int64_t path_offset, int64_t n_local,
                                   int32_t n_steps, uint64_t seed, int antithetic, olmc_stats* out) {
    return run_heston_surface<HestonEuler>(S, T, r, q, is_call, {kappa, theta, sigma_v, rho, v0}, strikes, steps, k,
                                           {path_offset, n_local, n_steps, seed, antithetic}, out);
}

extern "C" int olmc_heston_qmc_surface(double S, double T, double r, double q, int is_call, double kappa, double theta, double sigma_v,
                                       double rho, double v0, const double* strikes, const int32_t* steps, int32_t k, int construction,
                                       int64_t point_offset, int64_t n_points, int32_t n_steps, const uint32_t* sv, const uint32_t* shift,
                                       int32_t bits, int antithetic, olmc_stats* out) {
    return run_heston_qmc_surface<HestonEuler>(S, T, r, q, is_call, {kappa, theta, sigma_v, rho, v0}, strikes, steps, k,
                                               {construction, point_offset, n_points, n_steps, sv, shift, bits, antithetic}, out);
}

// ====================================================== Dupire local volatility ====
// include/olmc_local_vol.h: the payoffs of olmc_heston_path_payoff, a path matrix and a surface of Europeans on GBM-stream paths whose
// volatility is a bilinear lookup in the caller's table (olmc_local_vol_kernels.h).  Every check comes before the lease; the table goes
// to the device on the context's stream with every call and is read by that call's one launch only.
namespace {
int lv_surface_check(const ollv_surface* s) {
    if (!s || !s->vol) return fail(OLMC_ERR_ARG, "null pointer");
    if (s->n_x < 2 || s->n_x > kLvMaxNx) return fail(OLMC_ERR_ARG, "n_x must be in [2, 256]");
    if (s->n_t < 1 || s->n_t > kLvMaxNt) return fail(OLMC_ERR_ARG, "n_t must be in [1, 64]");
    if (!(s->x_hi > s->x_lo)) return fail(OLMC_ERR_ARG, "x_hi must be > x_lo");
    if (s->n_t > 1 && !(s->t_hi > 0.0)) return fail(OLMC_ERR_ARG, "t_hi must be > 0");
    const int32_t nodes = s->n_t * s->n_x;
    for (int32_t k = 0; k < nodes; ++k) {
        const float a = static_cast<float>(s->vol[k]);          // the value the kernels read
        if (!(std::isfinite(a) && a > 0.0f)) return fail(OLMC_ERR_ARG, "local volatilities must be finite and > 0");
    }
    return OLMC_OK;
}

bool lv_poisoned(double S, double K, double T, double r, double q, const ollv_surface* s) {
    return poisoned(S, K, T, r, 0.0, q) || std::isnan(s->x_lo + s->x_hi) || (s->n_t > 1 && std::isnan(s->t_hi));
}

// The checked table rounded to fp32 onto context c (on its stream, ahead of the launch that reads it) and the model of n_steps steps.
// z_unit: what one unit of the kernel's normals is worth (kZScale: the Philox stream's raw normals; 1: the Sobol kernels' true ones).
int lv_upload(DeviceCtx* c, const ollv_surface* s, double S, double T, double r, double q, int32_t n_steps, LvModel* m, double z_unit = kZScale) {
    const size_t nodes = static_cast<size_t>(s->n_t) * s->n_x;
    const int rc = c->lv.upload(sizeof(float) * nodes, c->stream, [c] { return c->drain(); }, [&](unsigned char* host) {
        float* f = reinterpret_cast<float*>(host);
        for (size_t k = 0; k < nodes; ++k) f[k] = static_cast<float>(s->vol[k]);
        return 0;
    }, sizeof(float) * kLvMaxNt * kLvMaxNx);                // the block is sized for the largest table by the first call
    if (rc) return rc;
    const double dt = T / n_steps;
    m->nodes = c->lv.device<float>();
    m->n_x = s->n_x;
    m->n_t = s->n_t;
    m->x_lo = s->x_lo;
    m->x_scale = (s->n_x - 1) / (s->x_hi - s->x_lo);
    m->t_scale = s->n_t > 1 ? (s->n_t - 1) / s->t_hi : 0.0;
    m->dt = dt;
    m->rq_dt = (r - q) * dt;
    m->half_dt = 0.5 * dt;
    m->vol_unit = std::sqrt(dt) * z_unit;
    m->s0 = S;
    m->log_s0 = std::log(S);
    return OLMC_OK;
}

// launch_timed with the table's dynamic LDS (lv_lds; none for the A/B form of lv_price_kernel, which keeps a row of its own).  Beyond 48 KiB the kernel is told so first (a no-op where the runtime has no such limit).
template <typename Kernel, typename... Args>
void lv_launch(Kernel kernel, const LvModel& m, bool table_in_lds, int32_t grid, hipStream_t s, const EventPair* timed, const Args&... args) {
    const uint32_t lds = table_in_lds ? static_cast<uint32_t>(sizeof(float)) * m.n_t * m.n_x : 0u;
    if (lds > 48u * 1024u) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
        (void)hipGetLastError();
    }
    if (timed) hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), lds, s, timed->start, timed->stop, 0, args...);
    else hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), lds, s, args...);
}
}  // namespace

extern "C" int ollv_price(double S, double K, double T, double r, double q, int is_call, const ollv_surface* surf, int payoff, double barrier,
                          int64_t path_offset, int64_t n_local, int32_t n_steps, uint64_t seed, int antithetic, olmc_stats* out) {
    if (!out) return fail(OLMC_ERR_ARG, "null pointer");
    int rc = lv_surface_check(surf);
    if (rc) return rc;
    rc = path_payoff_check(payoff, barrier, OLLV_EUROPEAN);
    if (rc) return rc;
    rc = check_paths(path_offset, n_local, n_steps);
    if (rc) return rc;
    const PathPayoff pp = path_payoff(S, K, is_call, payoff, barrier);
    const bool bad = lv_poisoned(S, K, T, r, q, surf) || pp.nan_barrier;
    const double inv_steps = 1.0 / n_steps;
    CtxLease lease;
    rc = ctx_lease(&lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    LvModel m;
    rc = lv_upload(c, surf, S, T, r, q, n_steps, &m);
    if (rc) return rc;
    const PathRange pr = make_range(path_offset, n_local, n_steps, seed);
    rc = launch_reduce(c, c->stream, c->d_result, -1.0, 2, grid_for(n_local),
                       [&](int32_t grid, hipStream_t st, const EventPair* timed, const ReduceWs& ws) {
                           with_path_family(payoff, OLLV_EUROPEAN, [&](auto f) {
                               with_bool(antithetic != 0, [&](auto a) { lv_launch(lv_price_kernel<f, a>, m, !OLMC_LV_ROW_LDS, grid, st, timed, pr, m, pp.ec, inv_steps, ws); });
                           });
                       });
    if (rc) return rc;
    finish_one(c->h_result, n_local * (antithetic ? 2 : 1), r, T, bad, out);
    return OLMC_OK;
}

extern "C" int ollv_paths(double S, double T, double r, double q, const ollv_surface* surf, int64_t n_paths, int32_t n_steps, uint64_t seed,
                          int path_major, double* out_host) {
    if (!out_host) return fail(OLMC_ERR_ARG, "null pointer");
    const int rc = lv_surface_check(surf);
    if (rc) return rc;
    LvModel m;
    return run_philox_matrix(n_paths, n_steps, seed, out_host, [&](DeviceCtx* c) { return lv_upload(c, surf, S, T, r, q, n_steps, &m); },
                             [&](DeviceCtx* c, int32_t grid, const PathRange& pr, double* d_paths) {
        with_bool(path_major != 0, [&](auto pm) { lv_launch(lv_paths_kernel<pm>, m, true, grid, c->stream, nullptr, pr, m, d_paths); });
    });
}

extern "C" int ollv_surface_prices(double S, double T, double r, double q, int is_call, const ollv_surface* surf, const double* strikes,
                                   const int32_t* steps, int32_t k, int64_t path_offset, int64_t n_local, int32_t n_steps, uint64_t seed,
                                   int antithetic, olmc_stats* out) {
    if (!strikes || !steps || !out) return fail(OLMC_ERR_ARG, "null pointer");
    const int rc = lv_surface_check(surf);
    if (rc) return rc;
    LvModel m;
    const double sign = is_call ? 1.0 : -1.0;
    return run_philox_surface(strikes, steps, k, {path_offset, n_local, n_steps, seed, antithetic}, r, T, lv_poisoned(S, 0.0, T, r, q, surf), out,
                              [&](DeviceCtx* c) { return lv_upload(c, surf, S, T, r, q, n_steps, &m); },
                              [&](int32_t grid, hipStream_t st, const EventPair* timed, const PathRange& pr, const HestonSurfaceCells& cells,
                                  const ReduceWs& ws) {
        with_bool(antithetic != 0, [&](auto a) { lv_launch(lv_surface_kernel<a>, m, true, grid, st, timed, pr, m, sign, cells, ws); });
    });
}

// ====================================================== SABR ====
// include/olmc_sabr.h: the payoffs of olmc_heston_path_payoff, the two path matrices and a surface of Europeans on paths of the SABR
// process (olmc_sabr_kernels.h).  Every check comes before the lease; the kernel is picked by beta's kind.
namespace {
static_assert(kTagSabr == OLMC_STREAM_SABR, "the kernels' tag is the header's");

int sabr_check(const olsb_model* m, double F) {
    if (!m) return fail(OLMC_ERR_ARG, "null pointer");
    if (m->alpha <= 0.0) return fail(OLMC_ERR_ARG, "alpha must be positive");
    if (!(m->beta >= 0.0 && m->beta <= 1.0)) return fail(OLMC_ERR_ARG, "beta must be in [0, 1]");
    if (!(m->rho >= -1.0 && m->rho <= 1.0)) return fail(OLMC_ERR_ARG, "rho must be in [-1, 1]");
    if (m->nu < 0.0) return fail(OLMC_ERR_ARG, "nu must be non-negative");
    if (F <= 0.0) return fail(OLMC_ERR_ARG, "F must be positive");
    return OLMC_OK;
}

bool sabr_poisoned(double F, double K, double T, double r, const olsb_model* m) {
    return poisoned(F, K, T, r, 0.0, 0.0) || std::isnan(m->alpha + m->beta + m->rho + m->nu);
}

// z_unit: what one unit of the kernel's normals is worth -- kZScale for the Philox kernels' RAW normals, 1 for the Sobol kernels' true ones.
SabrModel make_sabr(double F, double T, const olsb_model* m, int32_t n_steps, double z_unit) {
    const double dt = T / n_steps, unit = std::sqrt(dt) * z_unit;
    SabrModel sm;
    sm.f0 = F;
    sm.log_f0 = std::log(F);
    sm.alpha = m->alpha;
    sm.beta = m->beta;
    sm.half_dt = 0.5 * dt;
    sm.vol_unit = unit;
    sm.a = m->nu * m->rho * unit;
    sm.b = m->nu * std::sqrt(1.0 - m->rho * m->rho) * unit;
    sm.c = -0.5 * m->nu * m->nu * dt;
    return sm;
}

// f(integral_constant<int, kind>) for the kernel of beta: the three special exponents by exact equality, otherwise the general one.
template <typename F>
void with_sabr_kind(double beta, F&& f) {
    if (beta == 1.0) f(std::integral_constant<int, kSabrLognormal>{});
    else if (beta == 0.5) f(std::integral_constant<int, kSabrHalf>{});
    else if (beta == 0.0) f(std::integral_constant<int, kSabrNormal>{});
    else f(std::integral_constant<int, kSabrGeneral>{});
}
}  // namespace

extern "C" int olsb_price(double F, double K, double T, double r, int is_call, const olsb_model* m, int payoff, double barrier, int64_t path_offset,
                          int64_t n_local, int32_t n_steps, uint64_t seed, int antithetic, olmc_stats* out) {
    if (!out) return fail(OLMC_ERR_ARG, "null pointer");
    int rc = sabr_check(m, F);
    if (rc) return rc;
    rc = path_payoff_check(payoff, barrier, OLSB_EUROPEAN);
    if (rc) return rc;
    rc = check_paths(path_offset, n_local, n_steps);
    if (rc) return rc;
    const SabrModel sm = make_sabr(F, T, m, n_steps, kZScale);
    const PathPayoff pp = path_payoff(F, K, is_call, payoff, barrier);
    const bool bad = sabr_poisoned(F, K, T, r, m) || pp.nan_barrier;
    const double inv_steps = 1.0 / n_steps;
    return run_structured(path_offset, n_local, n_steps, seed, antithetic, r, T, bad, out,
                          [&](int32_t grid, hipStream_t st, const EventPair* timed, const PathRange& pr, const ReduceWs& ws) {
                              with_path_family(payoff, OLSB_EUROPEAN, [&](auto f) {
                                  with_sabr_kind(m->beta, [&](auto b) {
                                      with_bool(antithetic != 0, [&](auto a) {
                                          launch_timed(sabr_price_kernel<f, b, a>, dim3(grid), dim3(kBlock), st, timed, pr, sm, pp.ec, inv_steps, ws);
                                      });
                                  });
                              });
                          });
}

extern "C" int olsb_paths(double F, double T, const olsb_model* m, int64_t n_paths, int32_t n_steps, uint64_t seed, int mirror, int path_major,
                          double* forward_host, double* vol_host) {
    if (!forward_host || !vol_host) return fail(OLMC_ERR_ARG, "null pointer");
    int rc = sabr_check(m, F);
    if (rc) return rc;
    const double bytes = 8.0 * static_cast<double>(n_paths) * (n_steps + 1.0);
    CtxLease lease;
    rc = matrix_prologue(n_paths, n_steps, 2 * bytes, "path matrices would exceed 64 GB", &lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    const SabrModel sm = make_sabr(F, T, m, n_steps, kZScale);
    const PathRange pr = make_range(0, n_paths, n_steps, seed);
    const double flip = mirror ? -1.0 : 1.0;
    return heston_path_matrices(c, n_paths, n_steps, forward_host, vol_host, [&](const EventPair* timed, double* d_forward, double* d_vol) {
        with_sabr_kind(m->beta, [&](auto b) {
            with_bool(path_major != 0, [&](auto pm) {
                launch_timed(sabr_paths_kernel<b, pm>, dim3(grid_for(n_paths)), dim3(kBlock), c->stream, timed, pr, sm, flip, d_forward, d_vol);
            });
        });
    });
}

extern "C" int olsb_surface_prices(double F, double T, double r, int is_call, const olsb_model* m, const double* strikes, const int32_t* steps,
                                   int32_t k, int64_t path_offset, int64_t n_local, int32_t n_steps, uint64_t seed, int antithetic, olmc_stats* out) {
    if (!strikes || !steps || !out) return fail(OLMC_ERR_ARG, "null pointer");
    const int rc = sabr_check(m, F);
    if (rc) return rc;
    const double sign = is_call ? 1.0 : -1.0;
    return run_philox_surface(strikes, steps, k, {path_offset, n_local, n_steps, seed, antithetic}, r, T, sabr_poisoned(F, 0.0, T, r, m), out, no_setup,
                              [&](int32_t grid, hipStream_t st, const EventPair* timed, const PathRange& pr, const HestonSurfaceCells& cells,
                                  const ReduceWs& ws) {
        const SabrModel sm = make_sabr(F, T, m, n_steps, kZScale);
        with_sabr_kind(m->beta, [&](auto b) {
            with_bool(antithetic != 0, [&](auto a) {
                launch_timed(sabr_surface_kernel<b, a>, dim3(grid), dim3(kBlock), st, timed, pr, sm, sign, cells, ws);
            });
        });
    });
}

// ====================================================== SABR on Sobol paths ====
// include/olmc_sabr_qmc.h: the three entry points above on scrambled-Sobol points (olmc_sabr_qmc_kernels.h).  The checks are those of
// both sides, from their helpers, in the header's order: pointers, the model and F, the payoff, then the construction, tables and
// points as olmc_heston_qmc (two dimensions per step), then the cells -- all before the lease.  The launches take the shape of a
// Heston price launch (heston_qmc_shape: the bridge's [2 n][64] slabs) and the model in units of true normals.
extern "C" int olsq_price(double F, double K, double T, double r, int is_call, const olsb_model* m, int payoff, double barrier, int construction,
                          int64_t point_offset, int64_t n_points, int32_t n_steps, const uint32_t* sv, const uint32_t* shift, int32_t bits,
                          int antithetic, olmc_stats* out) {
    if (!out) return fail(OLMC_ERR_ARG, "null pointer");
    int rc = sabr_check(m, F);
    if (rc) return rc;
    rc = path_payoff_check(payoff, barrier, OLSB_EUROPEAN);
    if (rc) return rc;
    const auto call = SobolCall::make({construction, point_offset, n_points, n_steps, sv, shift, bits, antithetic}, 2, &rc);
    if (!call) return rc;
    const SabrModel sm = make_sabr(F, T, m, n_steps, 1.0);
    const PathPayoff pp = path_payoff(F, K, is_call, payoff, barrier);
    const bool bad = sabr_poisoned(F, K, T, r, m) || pp.nan_barrier;
    return run_qmc_reduce(*call, 2, heston_qmc_shape, [&](int32_t g, hipStream_t s, const EventPair* timed, const QmcPathLaunch& pl, const ReduceWs& ws) {
        with_path_family(payoff, OLSB_EUROPEAN, [&](auto f) {
            with_bridge_anti(pl, [&](auto b, auto a) {
                with_sabr_kind(m->beta, [&](auto kind) {
                    launch_timed(sabr_qmc_price_kernel<f, kind, b, a>, dim3(g), dim3(kBlock), s, timed, pl.qr, sm, pp.ec, pl.inv_steps, pl.d_sv, pl.d_shift,
                                 pl.plan, pl.slabs, ws);
                });
            });
        });
    }, qmc_stats(r, T, bad, out));
}

extern "C" int olsq_paths(double F, double T, const olsb_model* m, int construction, int64_t n_points, int32_t n_steps, const uint32_t* sv,
                          const uint32_t* shift, int32_t bits, int mirror, int path_major, double* forward_host, double* vol_host) {
    if (!forward_host || !vol_host) return fail(OLMC_ERR_ARG, "null pointer");
    int rc = sabr_check(m, F);
    if (rc) return rc;
    const auto call = SobolCall::make({construction, 0, n_points, n_steps, sv, shift, bits, 0}, 2, &rc);
    if (!call) return rc;
    const double bytes = 8.0 * static_cast<double>(n_points) * (n_steps + 1.0);
    CtxLease lease;
    rc = qmc_matrix_prologue(*call, 2 * bytes, &lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    const SabrModel sm = make_sabr(F, T, m, n_steps, 1.0);
    QmcPathLaunch pl;
    rc = qmc_matrix_setup(c, *call, &pl);
    if (rc) return rc;
    const double flip = mirror ? -1.0 : 1.0;
    return heston_path_matrices(c, n_points, n_steps, forward_host, vol_host, [&](const EventPair* timed, double* d_forward, double* d_vol) {
        with_sabr_kind(m->beta, [&](auto kind) {
            with_bool(pl.bridge, [&](auto b) {
                with_bool(path_major != 0, [&](auto pm) {
                    launch_timed(sabr_qmc_paths_kernel<kind, b, pm>, dim3(pl.grid), dim3(kBlock), c->stream, timed, pl.qr, sm, flip, pl.d_sv, pl.d_shift,
                                 pl.plan, d_forward, d_vol);
                });
            });
        });
    });
}

extern "C" int olsq_surface_prices(double F, double T, double r, int is_call, const olsb_model* m, const double* strikes, const int32_t* steps,
                                   int32_t k, int construction, int64_t point_offset, int64_t n_points, int32_t n_steps, const uint32_t* sv,
                                   const uint32_t* shift, int32_t bits, int antithetic, olmc_stats* out) {
    if (!strikes || !steps || !out) return fail(OLMC_ERR_ARG, "null pointer");
    int rc = sabr_check(m, F);
    if (rc) return rc;
    const auto call = SobolCall::make({construction, point_offset, n_points, n_steps, sv, shift, bits, antithetic}, 2, &rc);
    if (!call) return rc;
    SurfaceOrder so;
    rc = surface_cells(strikes, steps, k, n_steps, &so);
    if (rc) return rc;
    const SabrModel sm = make_sabr(F, T, m, n_steps, 1.0);
    const bool bad = sabr_poisoned(F, 0.0, T, r, m);
    const double sign = is_call ? 1.0 : -1.0;
    return run_qmc_reduce(*call, 2 * kSurfaceCells, heston_qmc_shape,
                          [&](int32_t g, hipStream_t s, const EventPair* timed, const QmcPathLaunch& pl, const ReduceWs& ws) {
        with_bridge_anti(pl, [&](auto b, auto a) {
            with_sabr_kind(m->beta, [&](auto kind) {
                launch_timed(sabr_qmc_surface_kernel<kind, b, a>, dim3(g), dim3(kBlock), s, timed, pl.qr, sm, sign, so.cells, pl.d_sv, pl.d_shift, pl.plan,
                             pl.slabs, ws);
            });
        });
    }, [&](const double* h, int64_t n) { surface_finish(h, so, strikes, steps, k, n, r, T / n_steps, bad, out); });
}

// ====================================================== Dupire local volatility on Sobol paths ====
// include/olmc_local_vol_qmc.h: the three entry points above on scrambled-Sobol points (olmc_local_vol_qmc_kernels.h).  The checks are
// those of both sides, from their helpers: the table, payoff and cells as above, the construction, tables and points as the other
// Sobol path calls (one dimension per step), all before the lease.
namespace {
// The shape of a local-volatility Sobol launch (lv_qmc_price_kernel, lv_qmc_surface_kernel): heston_qmc_shape's grid over the aligned
// blocks of 64 points, for the bridge one [n][64] slab per wave of the grid in the Heston kernels' block (heston_slabs), then the table
// and the model in units of true normals.
auto lv_qmc_shape(const ollv_surface* surf, double S, double T, double r, double q, LvModel* m) {
    return [=](DeviceCtx* c, const SobolCall& call, QmcPathLaunch* pl) {
        const int rc = heston_qmc_shape(c, call, pl);
        return rc ? rc : lv_upload(c, surf, S, T, r, q, call.n_steps, m, 1.0);
    };
}
}  // namespace

extern "C" int olvq_price(double S, double K, double T, double r, double q, int is_call, const ollv_surface* surf, int payoff, double barrier,
                          int construction, int64_t point_offset, int64_t n_points, int32_t n_steps, const uint32_t* sv, const uint32_t* shift,
                          int32_t bits, int antithetic, olmc_stats* out) {
    if (!out) return fail(OLMC_ERR_ARG, "null pointer");
    int rc = lv_surface_check(surf);
    if (rc) return rc;
    rc = path_payoff_check(payoff, barrier, OLLV_EUROPEAN);
    if (rc) return rc;
    const auto call = SobolCall::make({construction, point_offset, n_points, n_steps, sv, shift, bits, antithetic}, 1, &rc);
    if (!call) return rc;
    const PathPayoff pp = path_payoff(S, K, is_call, payoff, barrier);
    const bool bad = lv_poisoned(S, K, T, r, q, surf) || pp.nan_barrier;
    LvModel m;
    return run_qmc_reduce(*call, 2, lv_qmc_shape(surf, S, T, r, q, &m),
                          [&](int32_t g, hipStream_t s, const EventPair* timed, const QmcPathLaunch& pl, const ReduceWs& ws) {
        with_path_family(payoff, OLLV_EUROPEAN, [&](auto f) {
            with_bridge_anti(pl, [&](auto b, auto a) {
                lv_launch(lv_qmc_price_kernel<f, b, a>, m, true, g, s, timed, pl.qr, m, pp.ec, pl.inv_steps, pl.d_sv, pl.d_shift, pl.plan, pl.slabs, ws);
            });
        });
    }, qmc_stats(r, T, bad, out));
}

extern "C" int olvq_paths(double S, double T, double r, double q, const ollv_surface* surf, int construction, int64_t n_points, int32_t n_steps,
                          const uint32_t* sv, const uint32_t* shift, int32_t bits, int path_major, double* out_host) {
    if (!out_host) return fail(OLMC_ERR_ARG, "null pointer");
    int rc = lv_surface_check(surf);
    if (rc) return rc;
    const auto call = SobolCall::make({construction, 0, n_points, n_steps, sv, shift, bits, 0}, 1, &rc);
    if (!call) return rc;
    const double bytes = 8.0 * static_cast<double>(n_points) * (n_steps + 1.0);
    CtxLease lease;
    rc = matrix_prologue(n_points, n_steps, bytes, "path matrix would exceed 64 GB", &lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    QmcPathLaunch pl;
    rc = qmc_matrix_setup(c, *call, &pl);
    if (rc) return rc;
    LvModel m;
    rc = lv_upload(c, surf, S, T, r, q, n_steps, &m, 1.0);
    if (rc) return rc;
    EventPair ep{};
    const EventPair* timed = nullptr;                  // profiling on: the path kernel counts in olmc_kernel_time
    rc = prof_pair(c, &ep, &timed);
    if (rc) return rc;
    with_bool(pl.bridge, [&](auto b) {
        with_bool(path_major != 0, [&](auto pm) {
            lv_launch(lv_qmc_paths_kernel<b, pm>, m, true, pl.grid, c->stream, timed, pl.qr, m, pl.d_sv, pl.d_shift, pl.plan, c->bulk.as<double>());
        });
    });
    HIP_TRY(hipGetLastError());
    return copy_to_host(c, out_host, c->bulk.get(), static_cast<size_t>(bytes));
}

extern "C" int olvq_surface_prices(double S, double T, double r, double q, int is_call, const ollv_surface* surf, const double* strikes,
                                   const int32_t* steps, int32_t k, int construction, int64_t point_offset, int64_t n_points, int32_t n_steps,
                                   const uint32_t* sv, const uint32_t* shift, int32_t bits, int antithetic, olmc_stats* out) {
    if (!strikes || !steps || !out) return fail(OLMC_ERR_ARG, "null pointer");
    int rc = lv_surface_check(surf);
    if (rc) return rc;
    const auto call = SobolCall::make({construction, point_offset, n_points, n_steps, sv, shift, bits, antithetic}, 1, &rc);
    if (!call) return rc;
    SurfaceOrder so;
    rc = surface_cells(strikes, steps, k, n_steps, &so);
    if (rc) return rc;
    const bool bad = lv_poisoned(S, 0.0, T, r, q, surf);
    LvModel m;
    const double sign = is_call ? 1.0 : -1.0;
    return run_qmc_reduce(*call, 2 * kSurfaceCells, lv_qmc_shape(surf, S, T, r, q, &m),
                          [&](int32_t g, hipStream_t s, const EventPair* timed, const QmcPathLaunch& pl, const ReduceWs& ws) {
        with_bridge_anti(pl, [&](auto b, auto a) {
            lv_launch(lv_qmc_surface_kernel<b, a>, m, true, g, s, timed, pl.qr, m, sign, so.cells, pl.d_sv, pl.d_shift, pl.plan, pl.slabs, ws);
        });
    }, [&](const double* h, int64_t n) { surface_finish(h, so, strikes, steps, k, n, r, T / n_steps, bad, out); });
}

// ====================================================== Heston scenario sets and fused Greeks ====
// k scenarios on one set of olmc_heston's / olmc_heston_qmc's draws (include/olmc.h "Heston scenario sets and finite-difference
// Greeks"): the grouping and the kernel's argument are host arithmetic (olmc_host_math.h: heston_scenario_set), the launch is the
// surface's -- the same runners, ranges, grids and slabs, one launch of heston_scenarios_kernel / heston_qmc_scenarios_kernel.
namespace {
static_assert(kHestonRecursions == kAsianGroups && sizeof(HestonScenarioSet) <= 2048, "the scenario set travels by value in the kernel arguments");

// The checks of a scenario list that need no device, in the order olmc.h lists them.
int scenario_check(const olmc_heston_scenario* sc, int32_t k, const olmc_stats* out) {
    if (!sc || !out) return fail(OLMC_ERR_ARG, "null pointer");
    if (k < 1 || k > OLMC_MAX_BATCH) return fail(OLMC_ERR_ARG, "the number of scenarios must be in [1, OLMC_MAX_BATCH]");
    for (int32_t i = 0; i < k; ++i) {
        if (sc[i].T <= 0.0) return fail(OLMC_ERR_ARG, "T must be > 0 in every scenario");
        const int rc = heston_check({sc[i].kappa, sc[i].theta, sc[i].sigma_v, sc[i].rho, sc[i].v0});
        if (rc) return rc;
    }
    int32_t n_rec, group[OLMC_MAX_BATCH];
    if (const char* bad = heston_scenario_groups(sc, k, &n_rec, group)) return fail(OLMC_ERR_ARG, bad);
    return OLMC_OK;
}

// Scenario i's stats from the launch's sums, discounted at its own r and T; a poisoned scenario answers NaN, alone.
void scenario_finish(const double* h, const int32_t* slot_of, const olmc_heston_scenario* sc, int32_t k, int64_t n, olmc_stats* out) {
    for (int32_t i = 0; i < k; ++i) {
        const int32_t j = slot_of[i];
        if (heston_scenario_poisoned(sc[i])) nan_stats(n, &out[i]);
        else finish_stats(h[2 * j], h[2 * j + 1], n, sc[i].r, sc[i].T, &out[i]);
    }
}

// Philox: the scenarios on paths [path_offset, path_offset + n_local) of olmc_heston's stream.
int run_heston_scenarios(const olmc_heston_scenario* sc, int32_t k, int64_t path_offset, int64_t n_local, int32_t n_steps, uint64_t seed,
                         int antithetic, olmc_stats* out) {
    int rc = scenario_check(sc, k, out);
    if (rc) return rc;
    rc = check_paths(path_offset, n_local, n_steps);
    if (rc) return rc;
    HestonScenarioSet set;
    int32_t slot_of[OLMC_MAX_BATCH];
    if (const char* bad = heston_scenario_set(sc, k, n_steps, kZScale, &set, slot_of)) return fail(OLMC_ERR_ARG, bad);
    CtxLease lease;
    rc = ctx_lease(&lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    const PathRange pr = make_range(path_offset, n_local, n_steps, seed);
    rc = launch_reduce(c, c->stream, c->d_result, -1.0, 2 * kSurfaceCells, grid_for(n_local),
                       [&](int32_t grid, hipStream_t st, const EventPair* timed, const ReduceWs& ws) {
                           with_bool(antithetic != 0, [&](auto a) {
                               launch_timed(heston_scenarios_kernel<a>, dim3(grid), dim3(kBlock), st, timed, set, pr, ws);
                           });
                       });
    if (rc) return rc;
    scenario_finish(c->h_result, slot_of, sc, k, n_local * (antithetic ? 2 : 1), out);
    return OLMC_OK;
}

// Sobol: the scenarios on points [point_offset, point_offset + n_points) of olmc_heston_qmc's construction; the shape of a Heston price launch.
int run_heston_qmc_scenarios(const olmc_heston_scenario* sc, int32_t k, const SobolArgs& args, olmc_stats* out) {
    int rc = scenario_check(sc, k, out);
    if (rc) return rc;
    const auto call = SobolCall::make(args, 2, &rc);
    if (!call) return rc;
    HestonScenarioSet set;
    int32_t slot_of[OLMC_MAX_BATCH];
    if (const char* bad = heston_scenario_set(sc, k, call->n_steps, 1.0, &set, slot_of)) return fail(OLMC_ERR_ARG, bad);
    return run_qmc_reduce(*call, 2 * kSurfaceCells, heston_qmc_shape,
                          [&](int32_t g, hipStream_t s, const EventPair* timed, const QmcPathLaunch& pl, const ReduceWs& ws) {
        with_bool(pl.anti, [&](auto a) {           // the surface's nest, not with_bridge_anti's: the kernels keep their order in the code object
            with_bool(pl.bridge, [&](auto b) {
                launch_timed(heston_qmc_scenarios_kernel<b, a>, dim3(g), dim3(kBlock), s, timed, set, pl.qr, pl.d_sv, pl.d_shift, pl.plan, pl.slabs, ws);
            });
        });
    }, [&](const double* h, int64_t n) { scenario_finish(h, slot_of, sc, k, n, out); });
}
}  // namespace

// The grouping of a scenario list (pure host arithmetic: needs no device).
extern "C" int olmc_heston_scenario_layout(const olmc_heston_scenario* sc, int32_t k, int32_t* n_recursions, int32_t* group) {
    if (!sc || !n_recursions || !group) return fail(OLMC_ERR_ARG, "null pointer");
    if (const char* bad = heston_scenario_groups(sc, k, n_recursions, group)) return fail(OLMC_ERR_ARG, bad);
    return OLMC_OK;
}

extern "C" int olmc_heston_scenarios(const olmc_heston_scenario* sc, int32_t k, int64_t path_offset, int64_t n_local, int32_t n_steps,
                                     uint64_t seed, int antithetic, olmc_stats* out) {
    return run_heston_scenarios(sc, k, path_offset, n_local, n_steps, seed, antithetic, out);
}

extern "C" int olmc_heston_qmc_scenarios(const olmc_heston_scenario* sc, int32_t k, int construction, int64_t point_offset, int64_t n_points,
                                         int32_t n_steps, const uint32_t* sv, const uint32_t* shift, int32_t bits, int antithetic,
                                         olmc_stats* out) {
    return run_heston_qmc_scenarios(sc, k, {construction, point_offset, n_points, n_steps, sv, shift, bits, antithetic}, out);
}

// The 7 / 8 / 11 / 14 contracts of compute_greeks_unified under the model, sigma -> v0 = sigma^2 (HestonAdapter, unified_greeks.py:74-104),
// as ONE scenario launch: GreeksSet as it stands (bumps, call order, finish), four recursions.
extern "C" int olmc_heston_greeks_fd(double S, double K, double T, double r, double sigma, double q, int is_call, double kappa, double theta,
                                     double sigma_v, double rho, int64_t n_paths, int32_t n_steps, uint64_t seed, int antithetic,
                                     int second_order, double* out9, olmc_stats* evals) {
    if (!out9) return fail(OLMC_ERR_ARG, "null pointer");
    if (!(T > 0.0)) return fail(OLMC_ERR_ARG, "T must be > 0");
    const GreeksSet gs(S, K, T, r, sigma, q, is_call, second_order);
    olmc_heston_scenario sc[OLMC_MAX_BATCH];
    heston_greeks_scenarios(gs, kappa, theta, sigma_v, rho, sc);
    olmc_stats st[OLMC_MAX_BATCH];
    const int rc = run_heston_scenarios(sc, gs.k, 0, n_paths, n_steps, seed, antithetic, st);
    if (rc) return rc;
    gs.finish(st, T, out9, evals);
    return OLMC_OK;
}

extern "C" int olmc_heston_qmc_greeks_fd(double S, double K, double T, double r, double sigma, double q, int is_call, double kappa,
                                         double theta, double sigma_v, double rho, int construction, int64_t n_points, int32_t n_steps,
                                         const uint32_t* sv, const uint32_t* shift, int32_t bits, int antithetic, int second_order,
                                         double* out9, olmc_stats* evals) {
    if (!out9) return fail(OLMC_ERR_ARG, "null pointer");
    if (!(T > 0.0)) return fail(OLMC_ERR_ARG, "T must be > 0");
    const GreeksSet gs(S, K, T, r, sigma, q, is_call, second_order);
    olmc_heston_scenario sc[OLMC_MAX_BATCH];
    heston_greeks_scenarios(gs, kappa, theta, sigma_v, rho, sc);
    olmc_stats st[OLMC_MAX_BATCH];
    const int rc = run_heston_qmc_scenarios(sc, gs.k, {construction, 0, n_points, n_steps, sv, shift, bits, antithetic}, st);
    if (rc) return rc;
    gs.finish(st, T, out9, evals);
    return OLMC_OK;
}

// ====================================================== Heston, quadratic-exponential scheme ====
// olmc_heston_surface / olmc_heston_paths and their Sobol forms with Andersen's QE step in place of the Euler one (include/olmc.h
// "Heston, quadratic-exponential scheme"): the same checks, ranges, cells and read-out (HestonQe), one launch of the heston_qe_* kernels.

extern "C" int olmc_heston_qe_surface(double S, double T, double r, double q, int is_call, double kappa, double theta, double sigma_v, double rho,
                                      double v0, const double* strikes, const int32_t* steps, int32_t k, int64_t path_offset, int64_t n_local,
                                      int32_t n_steps, uint64_t seed, int antithetic, olmc_stats* out) {
    return run_heston_surface<HestonQe>(S, T, r, q, is_call, {kappa, theta, sigma_v, rho, v0}, strikes, steps, k,
                                        {path_offset, n_local, n_steps, seed, antithetic}, out);
}

extern "C" int olmc_heston_qe_qmc_surface(double S, double T, double r, double q, int is_call, double kappa, double theta, double sigma_v,
                                          double rho, double v0, const double* strikes, const int32_t* steps, int32_t k, int construction,
                                          int64_t point_offset, int64_t n_points, int32_t n_steps, const uint32_t* sv, const uint32_t* shift,
                                          int32_t bits, int antithetic, olmc_stats* out) {
    return run_heston_qmc_surface<HestonQe>(S, T, r, q, is_call, {kappa, theta, sigma_v, rho, v0}, strikes, steps, k,
                                            {construction, point_offset, n_points, n_steps, sv, shift, bits, antithetic}, out);
}

extern "C" int olmc_heston_qe_paths(double S, double T, double r, double q, double kappa, double theta, double sigma_v, double rho, double v0,
                                    int64_t n_paths, int32_t n_steps, uint64_t seed, int path_major, double* spot_host, double* var_host) {
    return run_heston_paths<HestonQe>(S, T, r, q, {kappa, theta, sigma_v, rho, v0}, n_paths, n_steps, seed, path_major, spot_host, var_host);
}

extern "C" int olmc_heston_qe_qmc_paths(double S, double T, double r, double q, double kappa, double theta, double sigma_v, double rho, double v0,
                                        int construction, int64_t n_points, int32_t n_steps, const uint32_t* sv, const uint32_t* shift,
                                        int32_t bits, int path_major, double* spot_host, double* var_host) {
    return run_heston_qmc_paths<HestonQe>(S, T, r, q, {kappa, theta, sigma_v, rho, v0}, {construction, 0, n_points, n_steps, sv, shift, bits, 0},
                                          path_major, spot_host, var_host);
}

// ====================================================== American options under Heston ====
// include/olha.h: the path kernels of olmc_heston_paths / olmc_heston_qe_paths and their Sobol forms, time-major, queued on the
// context's stream ahead of a step chain -- heston_lsm_step_kernel on (S_t, v_t), or lsm_step_kernel on the spot matrix alone.
namespace {
static_assert(OLHA_EULER == OLMC_HESTON_EULER && OLHA_QE == OLMC_HESTON_QE, "with_heston_scheme reads olha.h's scheme codes");

struct HaDateScale {                 // a date's regressors: x = (S_t / K - cx) iwx, y = (v_t - cy) iwy
    double cx = 1.0, iwx = 1.0, cy = 0.0, iwy = 1.0;
};

// The model's expected average variance over [0, t], theta + (v0 - theta)(1 - e^(-kappa t)) / (kappa t): the sigma^2 of the lognormal
// law behind a date's (cx, wx).
double heston_average_variance(const HestonModel& m, double t) {
    const double a = m.kappa * t;
    return m.theta + (m.v0 - m.theta) * (a == 0.0 ? 1.0 : -std::expm1(-a) / a);
}

// lsm_regressor_scale's pair for S_t / K with the date's own sigma, and the conditional mean and standard deviation of the CIR variance
// v_t given v0 for v_t; the width of v_t is clamped below at 1e-6 max(mean, theta) and at 1e-12, so that sigma_v = 0 leaves y finite
// (exactly 0 where v_t is the mean).  A closed form that is not finite leaves the pair at (1, 1) / (0, 1).
HaDateScale heston_lsm_scale(double S, double K, double r, double q, bool is_call, const HestonModel& m, double dt, int32_t t) {
    HaDateScale s;
    const double years = dt * t;
    lsm_regressor_scale(S, K, r, q, std::sqrt(std::max(heston_average_variance(m, years), 0.0)), dt, t, is_call, &s.cx, &s.iwx);
    const double a = m.kappa * years, e = std::exp(-a);
    const double tg = years * (a == 0.0 ? 1.0 : -std::expm1(-a) / a);              // (1 - e^(-kappa t)) / kappa
    const double mean = m.theta + (m.v0 - m.theta) * e;
    const double var = m.sigma_v * m.sigma_v * (m.v0 * e * tg + 0.5 * m.theta * m.kappa * tg * tg);
    const double width = std::max({std::sqrt(std::max(var, 0.0)), 1e-6 * std::max(mean, m.theta), 1e-12});
    if (std::isfinite(mean) && std::isfinite(width)) {
        s.cy = mean;
        s.iwy = 1.0 / width;
    }
    return s;
}

// Bytes of a pricing's device buffers: the two matrices and the cash flows, + two buffers of <= 1024 workgroup rows of nv sums.
double ha_bytes(int64_t n_paths, int32_t n_steps, int nv) {
    return 8.0 * static_cast<double>(n_paths) * (2.0 * (n_steps + 1.0) + 1.0) + 8.0 * 2 * 1024 * nv;
}
int ha_row_width(int basis, int32_t poly_degree) {
    if (basis == OLHA_BASIS_SPOT) return kLsmNV;
    return poly_degree == 1 ? HaBasis<1>::NV : poly_degree == 2 ? HaBasis<2>::NV : HaBasis<3>::NV;
}

// The checks of both entry points that need neither the model nor the counts.
int ha_check(int scheme, int basis, int32_t poly_degree, const olmc_stats* out) {
    if (!out) return fail(OLMC_ERR_ARG, "null pointer");
    if (scheme != OLHA_EULER && scheme != OLHA_QE) return fail(OLMC_ERR_ARG, "bad scheme (OLHA_EULER or OLHA_QE)");
    if (basis != OLHA_BASIS_SPOT_VARIANCE && basis != OLHA_BASIS_SPOT) return fail(OLMC_ERR_ARG, "bad basis (OLHA_BASIS_SPOT_VARIANCE or OLHA_BASIS_SPOT)");
    if (basis == OLHA_BASIS_SPOT_VARIANCE && (poly_degree < 1 || poly_degree > kHaMaxDegree))
        return fail(OLMC_ERR_ARG, "poly_degree must be in [1, 3] for OLHA_BASIS_SPOT_VARIANCE");
    if (basis == OLHA_BASIS_SPOT && (poly_degree < 1 || poly_degree > kLsmMaxDegree))
        return fail(OLMC_ERR_ARG, "poly_degree must be in [1, 4] for OLHA_BASIS_SPOT");
    return OLMC_OK;
}

// lsm_chain's launches with the bivariate step kernel of total degree D over the two time-major matrices; d_cash [n_paths] and d_rows
// [2][1024][NV] are the next the caller's `bulk` hands out.  The grid and U are lsm_chain's: at most one workgroup per CU (every
// workgroup of a launch re-reads every row of the launch before it), U from the paths a thread has.  Leaves {sum, sumsq} of the time-0
// cash flows in c->h_result once the host has waited for them.
template <int D>
int heston_lsm_chain(DeviceCtx* c, const LsmContract& lc, const std::vector<HaDateScale>& scale, int64_t n_paths, int32_t n_steps,
                     const double* d_spot, const double* d_var, Carver* bulk) {
    constexpr int NV = HaBasis<D>::NV;
    double* d_cash = bulk->take<double>(static_cast<size_t>(n_paths));
    double* d_rows = bulk->take<double>(size_t(2) * 1024 * NV);
    const int32_t grid = std::min<int32_t>(grid_for(n_paths), std::min<int32_t>(c->cus, 1024));
    const int64_t per_thread = (n_paths + static_cast<int64_t>(grid) * kBlock - 1) / (static_cast<int64_t>(grid) * kBlock);
    const int unroll = per_thread <= 1 ? 1 : per_thread <= 2 ? 2 : per_thread <= 4 ? 4 : 8;
    ReduceWs ws;
    int rc = make_ws(c, c->stream, grid, 2, c->d_result, -1.0, &ws);               // arms the completion word for the launch that writes d_result
    if (rc) return rc;
    bool first = true;
    for (int32_t t_fit = n_steps - 1; t_fit >= 0; --t_fit) {
        const bool final_date = t_fit == 0;
        const HaDateScale &f = scale[t_fit], &p = scale[t_fit + 1];
        const HaScale sc{f.cx, f.iwx, f.cy, f.iwy, p.cx, p.iwx, p.cy, p.iwy};
        auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, c->stream, n_paths, lc, sc, d_rows, t_fit, d_spot, d_var, d_cash, ws); };
        auto pick = [&](auto u) {
            constexpr int U = decltype(u)::value;
            if (first && final_date) go(heston_lsm_step_kernel<D, U, true, true>);
            else if (first) go(heston_lsm_step_kernel<D, U, true, false>);
            else if (final_date) go(heston_lsm_step_kernel<D, U, false, true>);
            else go(heston_lsm_step_kernel<D, U, false, false>);
        };
        if (unroll == 1) pick(std::integral_constant<int, 1>{});
        else if (unroll == 2) pick(std::integral_constant<int, 2>{});
        else if (unroll == 4) pick(std::integral_constant<int, 4>{});
        else pick(std::integral_constant<int, 8>{});
        rc = after_launch(c, c->stream);
        if (rc) return rc;
        first = false;
    }
    return sync_or_recover(c, c->stream);
}

// One pricing on c, whose bulk buffer holds ha_bytes: `paths(d_spot, d_var)` queues the scheme's time-major path kernel on c's
// stream, the chain of the basis follows it, out answers from the time-0 cash flows (already discounted step by step: no outer factor).
template <typename Paths>
int heston_american(DeviceCtx* c, double S, double K, double T, double r, double q, int is_call, const HestonModel& m, int basis, int32_t poly_degree,
                    int64_t n_paths, int32_t n_steps, Paths&& paths, olmc_stats* out) {
    const size_t cells = (static_cast<size_t>(n_steps) + 1) * static_cast<size_t>(n_paths);
    Carver bulk = c->bulk.carve();
    double* d_spot = bulk.take<double>(cells);          // [n_steps + 1][n_paths] each, then the chain's buffers
    double* d_var = bulk.take<double>(cells);
    EventPair ep{};
    int rc;
    if (g_profile) { rc = prof_begin(c, c->stream, &ep); if (rc) return rc; }
    paths(d_spot, d_var);
    HIP_TRY(hipGetLastError());
    const LsmContract lc = lsm_contract(S, K, T, r, 0.0, q, is_call, n_steps, poly_degree);        // the chains read strike, sign, discount, degree, n_steps
    const double dt = T / n_steps;
    std::vector<HaDateScale> scale(static_cast<size_t>(n_steps) + 1);                             // while the path kernel runs
    for (int32_t t = 1; t < n_steps; ++t) scale[t] = heston_lsm_scale(S, K, r, q, is_call != 0, m, dt, t);
    if (basis == OLHA_BASIS_SPOT) {
        rc = lsm_chain_scaled(c, lc, n_paths, n_steps, d_spot, &bulk, [&](int32_t t, double* centre, double* inv_width) {
            *centre = scale[t].cx;
            *inv_width = scale[t].iwx;
        });
    } else if (poly_degree == 1) {
        rc = heston_lsm_chain<1>(c, lc, scale, n_paths, n_steps, d_spot, d_var, &bulk);
    } else if (poly_degree == 2) {
        rc = heston_lsm_chain<2>(c, lc, scale, n_paths, n_steps, d_spot, d_var, &bulk);
    } else {
        rc = heston_lsm_chain<3>(c, lc, scale, n_paths, n_steps, d_spot, d_var, &bulk);
    }
    if (rc) return rc;
    if (g_profile) { rc = prof_end(c, c->stream, ep); if (rc) return rc; }
    finish_one(c->h_result, n_paths, 0.0, T, heston_poisoned(S, K, T, r, q, m), out);
    return OLMC_OK;
}
constexpr const char* kHaTooBig = "path matrices would exceed 64 GB: lower n_paths or n_steps";
}  // namespace

extern "C" int olha_american_lsm(double S, double K, double T, double r, double q, int is_call, double kappa, double theta, double sigma_v,
                                 double rho, double v0, int scheme, int basis, int32_t poly_degree, int64_t n_paths, int32_t n_steps,
                                 uint64_t seed, olmc_stats* out) {
    int rc = ha_check(scheme, basis, poly_degree, out);
    if (rc) return rc;
    const HestonModel m{kappa, theta, sigma_v, rho, v0};
    return with_heston_scheme(scheme, [&](auto s) -> int {
        using Scheme = decltype(s);
        rc = Scheme::check(m);
        if (rc) return rc;
        CtxLease lease;
        rc = matrix_prologue(n_paths, n_steps, ha_bytes(n_paths, n_steps, ha_row_width(basis, poly_degree)), kHaTooBig, &lease);
        if (rc) return rc;
        DeviceCtx* const c = lease.c;
        const auto hc = Scheme::make(S, T, r, q, 1, m, n_steps);                   // as run_heston_paths makes it: the same matrices
        const PathRange pr = make_range(0, n_paths, n_steps, seed);
        return heston_american(c, S, K, T, r, q, is_call, m, basis, poly_degree, n_paths, n_steps, [&](double* d_spot, double* d_var) {
            hipLaunchKernelGGL(Scheme::template paths_kernel<false>(), dim3(grid_for(n_paths)), dim3(kBlock), 0, c->stream, pr, hc, S, d_spot, d_var);
        }, out);
    });
}

extern "C" int olha_american_lsm_qmc(double S, double K, double T, double r, double q, int is_call, double kappa, double theta, double sigma_v,
                                     double rho, double v0, int scheme, int basis, int32_t poly_degree, int construction, int64_t n_points,
                                     const uint32_t* sv, const uint32_t* shift, int32_t dims, int32_t bits, olmc_stats* out) {
    int rc = ha_check(scheme, basis, poly_degree, out);
    if (rc) return rc;
    if (dims % 2) return fail(OLMC_ERR_ARG, "dims must be even: a step takes two Sobol dimensions");
    const HestonModel m{kappa, theta, sigma_v, rho, v0};
    return with_heston_scheme(scheme, [&](auto s) -> int {
        using Scheme = decltype(s);
        rc = heston_qmc_scheme_check<Scheme>(m, construction);
        if (rc) return rc;
        const auto call = SobolCall::make({construction, 0, n_points, dims / 2, sv, shift, bits, 0}, 2, &rc);
        if (!call) return rc;
        const int32_t n_steps = call->n_steps;
        CtxLease lease;
        rc = matrix_prologue(n_points, n_steps, ha_bytes(n_points, n_steps, ha_row_width(basis, poly_degree)), kHaTooBig, &lease);
        if (rc) return rc;
        DeviceCtx* const c = lease.c;
        const auto hc = Scheme::make(S, T, r, q, 1, m, n_steps);                   // as run_heston_qmc_paths makes it: the same matrices
        QmcPathLaunch pl;
        rc = qmc_matrix_setup(c, *call, &pl);
        if (rc) return rc;
        return heston_american(c, S, K, T, r, q, is_call, m, basis, poly_degree, n_points, n_steps, [&](double* d_spot, double* d_var) {
            if constexpr (Scheme::kBridge) {
                with_bool(pl.bridge, [&](auto b) {
                    hipLaunchKernelGGL((heston_qmc_paths_kernel<decltype(b)::value, false>), dim3(pl.grid), dim3(kBlock), 0, c->stream, pl.qr, hc, S, pl.d_sv,
                                       pl.d_shift, pl.plan, d_spot, d_var);
                });
            } else {
                hipLaunchKernelGGL((heston_qe_qmc_paths_kernel<false>), dim3(pl.grid), dim3(kBlock), 0, c->stream, pl.qr, hc, S, pl.d_sv, pl.d_shift, d_spot, d_var);
            }
        }, out);
    });
}

extern "C" int olha_regressor_scales(double S, double K, double T, double r, double q, int is_call, double kappa, double theta, double sigma_v,
                                     double v0, int32_t n_steps, double* x_centre, double* x_width, double* y_centre, double* y_width) {
    if (!x_centre || !x_width || !y_centre || !y_width) return fail(OLMC_ERR_ARG, "null pointer");
    if (n_steps < 1) return fail(OLMC_ERR_ARG, "n_steps must be >= 1");
    const HestonModel m{kappa, theta, sigma_v, 0.0, v0};
    const double dt = T / n_steps;
    for (int32_t t = 0; t <= n_steps; ++t) {
        const HaDateScale s = t >= 1 && t < n_steps ? heston_lsm_scale(S, K, r, q, is_call != 0, m, dt, t) : HaDateScale{};
        x_centre[t] = s.cx;
        x_width[t] = 1.0 / s.iwx;
        y_centre[t] = s.cy;
        y_width[t] = 1.0 / s.iwy;
    }
    return OLMC_OK;
}

// ====================================================== structured products under Heston ====
// olmc_autocallable / olmc_cliquet and their Sobol forms on Heston paths, by either scheme (include/olmc.h "structured products under
// Heston"): the contracts of make_autocall / make_cliquet (their GBM drift and vol are not read), the model and range checks of the
// scheme's own entry points, one launch of heston_product_kernel, heston_qmc_product_kernel, heston_qe_product_kernel or
// heston_qe_qmc_product_kernel with the product as the policy.
namespace {
int heston_scheme_check(int scheme, const HestonModel& m) {
    if (scheme != OLMC_HESTON_EULER && scheme != OLMC_HESTON_QE) return fail(OLMC_ERR_ARG, "bad scheme (OLMC_HESTON_EULER or OLMC_HESTON_QE)");
    return with_heston_scheme(scheme, [&](auto s) { return decltype(s)::check(m); });
}

// Philox: paths [path_offset, path_offset + n_local) of olmc_heston's stream (Euler) / olmc_heston_qe_surface's (QE).
template <template <bool> class Product>
int run_heston_product(double S, double T, double r, double q, const HestonModel& m, int scheme, const typename Product<false>::Contract& pc,
                       double r_for_discount, bool bad, int64_t path_offset, int64_t n_local, int32_t n_steps, uint64_t seed, int antithetic,
                       olmc_stats* out) {
    return with_heston_scheme(scheme, [&](auto s) {
        using Scheme = decltype(s);
        const auto hc = Scheme::make(S, T, r, q, 1, m, n_steps);
        return run_structured(path_offset, n_local, n_steps, seed, antithetic, r_for_discount, T, bad, out,
                              [&](int32_t grid, hipStream_t st, const EventPair* timed, const PathRange& pr, const ReduceWs& ws) {
                                  with_bool(antithetic != 0, [&](auto a) {
                                      launch_timed(Scheme::template product_kernel<Product, decltype(a)::value>(), dim3(grid), dim3(kBlock), st, timed, pr,
                                                   hc, pc, ws);
                                  });
                              });
    });
}

// The checks of a Sobol call that do not depend on the product, in the order of olmc_heston_qe_qmc_surface, and the call they pass.
std::optional<SobolCall> heston_qmc_product_call(int scheme, const HestonModel& m, const SobolArgs& args, int* rc) {
    *rc = heston_scheme_check(scheme, m);
    if (!*rc && scheme == OLMC_HESTON_QE) *rc = heston_qe_sequential(args.construction);
    if (*rc) return std::nullopt;
    return SobolCall::make(args, 2, rc);
}

// Sobol: the points of olmc_heston_qmc's construction (Euler) / olmc_heston_qe_qmc_surface's (QE: sequential, the grid over the aligned
// blocks, no slabs).
template <template <bool> class Product>
int run_heston_qmc_product(double S, double T, double r, double q, const HestonModel& m, int scheme, const typename Product<false>::Contract& pc,
                           double r_for_discount, bool bad, const SobolCall& call, olmc_stats* out) {
    return with_heston_scheme(scheme, [&](auto s) {
        using Scheme = decltype(s);
        const auto hc = Scheme::make(S, T, r, q, 1, m, call.n_steps);
        return run_qmc_reduce(call, 2, heston_qmc_shape, [&](int32_t g, hipStream_t st, const EventPair* timed, const QmcPathLaunch& pl, const ReduceWs& ws) {
            with_bool(pl.anti, [&](auto a) {
                if constexpr (Scheme::kBridge) {
                    with_bool(pl.bridge, [&](auto b) {
                        launch_timed(heston_qmc_product_kernel<Product, b, a>, dim3(g), dim3(kBlock), st, timed, pl.qr, hc, pc, pl.d_sv, pl.d_shift,
                                     pl.plan, pl.slabs, ws);
                    });
                } else {
                    launch_timed(heston_qe_qmc_product_kernel<Product, a>, dim3(g), dim3(kBlock), st, timed, pl.qr, hc, pc, pl.d_sv, pl.d_shift, ws);
                }
            });
        }, qmc_stats(r_for_discount, T, bad, out));
    });
}
}  // namespace

extern "C" int olmc_heston_autocallable(double S, double T, double r, double q, double kappa, double theta, double sigma_v, double rho, double v0,
                                        double autocall_barrier, double coupon_barrier, double coupon_rate, double ki_barrier,
                                        int32_t observation_freq, int scheme, int64_t path_offset, int64_t n_local, int32_t n_steps,
                                        uint64_t seed, int antithetic, olmc_stats* out) {
    if (!out) return fail(OLMC_ERR_ARG, "null pointer");
    const HestonModel m{kappa, theta, sigma_v, rho, v0};
    int rc = heston_scheme_check(scheme, m);
    if (rc) return rc;
    rc = autocall_check(observation_freq, n_steps);
    if (rc) return rc;
    const AutocallSetup a = make_autocall(S, T, r, 0.0, q, autocall_barrier, coupon_barrier, coupon_rate, ki_barrier, observation_freq, n_steps);
    // payoffs are already discounted path by path, as olmc_autocallable's: no outer discount
    return run_heston_product<HestonAutocall>(S, T, r, q, m, scheme, a.ac, 0.0, a.bad || m.nan(), path_offset, n_local, n_steps, seed, antithetic, out);
}

extern "C" int olmc_heston_autocallable_qmc(double S, double T, double r, double q, double kappa, double theta, double sigma_v, double rho,
                                            double v0, double autocall_barrier, double coupon_barrier, double coupon_rate, double ki_barrier,
                                            int32_t observation_freq, int scheme, int construction, int64_t point_offset, int64_t n_points,
                                            int32_t n_steps, const uint32_t* sv, const uint32_t* shift, int32_t bits, int antithetic,
                                            olmc_stats* out) {
    if (!out) return fail(OLMC_ERR_ARG, "null pointer");
    const HestonModel m{kappa, theta, sigma_v, rho, v0};
    int rc;
    const auto call = heston_qmc_product_call(scheme, m, {construction, point_offset, n_points, n_steps, sv, shift, bits, antithetic}, &rc);
    if (!call) return rc;
    rc = autocall_check(observation_freq, n_steps);
    if (rc) return rc;
    const AutocallSetup a = make_autocall(S, T, r, 0.0, q, autocall_barrier, coupon_barrier, coupon_rate, ki_barrier, observation_freq, n_steps);
    return run_heston_qmc_product<HestonAutocall>(S, T, r, q, m, scheme, a.ac, 0.0, a.bad || m.nan(), *call, out);
}

extern "C" int olmc_heston_cliquet(double S, double T, double r, double q, double kappa, double theta, double sigma_v, double rho, double v0,
                                   double local_cap, double local_floor, double global_cap, double global_floor, int32_t n_periods, int scheme,
                                   int64_t path_offset, int64_t n_local, int32_t n_steps, uint64_t seed, int antithetic, olmc_stats* out) {
    if (!out) return fail(OLMC_ERR_ARG, "null pointer");
    const HestonModel m{kappa, theta, sigma_v, rho, v0};
    int rc = heston_scheme_check(scheme, m);
    if (rc) return rc;
    rc = cliquet_check(n_periods, n_steps);
    if (rc) return rc;
    const CliquetContract cc = make_cliquet(S, T, r, 0.0, q, local_cap, local_floor, global_cap, global_floor, n_periods, n_steps);
    const bool bad = cliquet_poisoned(S, T, r, 0.0, q, local_cap, local_floor, global_cap, global_floor) || m.nan();
    return run_heston_product<HestonCliquet>(S, T, r, q, m, scheme, cc, r, bad, path_offset, n_local, n_steps, seed, antithetic, out);
}

extern "C" int olmc_heston_cliquet_qmc(double S, double T, double r, double q, double kappa, double theta, double sigma_v, double rho, double v0,
                                       double local_cap, double local_floor, double global_cap, double global_floor, int32_t n_periods,
                                       int scheme, int construction, int64_t point_offset, int64_t n_points, int32_t n_steps,
                                       const uint32_t* sv, const uint32_t* shift, int32_t bits, int antithetic, olmc_stats* out) {
    if (!out) return fail(OLMC_ERR_ARG, "null pointer");
    const HestonModel m{kappa, theta, sigma_v, rho, v0};
    int rc;
    const auto call = heston_qmc_product_call(scheme, m, {construction, point_offset, n_points, n_steps, sv, shift, bits, antithetic}, &rc);
    if (!call) return rc;
    rc = cliquet_check(n_periods, n_steps);
    if (rc) return rc;
    const CliquetContract cc = make_cliquet(S, T, r, 0.0, q, local_cap, local_floor, global_cap, global_floor, n_periods, n_steps);
    const bool bad = cliquet_poisoned(S, T, r, 0.0, q, local_cap, local_floor, global_cap, global_floor) || m.nan();
    return run_heston_qmc_product<HestonCliquet>(S, T, r, q, m, scheme, cc, r, bad, *call, out);
}

// ====================================================== path-dependent payoffs under jump diffusion ====
// include/olmc_jump.h: the payoffs of olmc_heston_path_payoff, a surface of Europeans, the autocallable and the cliquet on
// olmc_jump_paths' paths (olmc_jump_kernels.h).  The model's checks are make_jump's, the contracts' those of the Heston entry points of
// the same payoffs; every check comes before the lease.
namespace {
// The checked model as the kernels' contract (K and is_call are read by the surface kernel's sign only).
int jd_contract(double S, double T, double r, double sigma, double q, int is_call, const oljd_model* m, int32_t n_steps, JumpContract* jc) {
    if (!m) return fail(OLMC_ERR_ARG, "null pointer");
    // a NaN intensity is a NaN input (jd_poisoned: NaN results), not a negative one: make_jump's sign check sees 0 in its place
    return make_jump(S, 0.0, T, r, sigma, q, is_call, m->model, std::isnan(m->lambda_j) ? 0.0 : m->lambda_j, m->a1, m->a2, m->a3, n_steps, jc);
}

bool jd_poisoned(double S, double K, double T, double r, double sigma, double q, const oljd_model* m) {
    return poisoned(S, K, T, r, sigma, q) || std::isnan(m->lambda_j + m->a1 + m->a2 + m->a3);
}

template <template <bool> class Product>
int run_jd_product(const JumpContract& jc, const typename Product<false>::Contract& pc, double r_for_discount, double T, bool bad, int64_t path_offset,
                   int64_t n_local, int32_t n_steps, uint64_t seed, int antithetic, olmc_stats* out) {
    return run_structured(path_offset, n_local, n_steps, seed, antithetic, r_for_discount, T, bad, out,
                          [&](int32_t grid, hipStream_t st, const EventPair* timed, const PathRange& pr, const ReduceWs& ws) {
                              with_bool(antithetic != 0, [&](auto a) {
                                  launch_timed(jump_product_kernel<Product, decltype(a)::value>, dim3(grid), dim3(kBlock), st, timed, pr, jc, pc, ws);
                              });
                          });
}
}  // namespace

extern "C" int oljd_price(double S, double K, double T, double r, double sigma, double q, int is_call, const oljd_model* model, int payoff,
                          double barrier, int64_t path_offset, int64_t n_local, int32_t n_steps, uint64_t seed, int antithetic, olmc_stats* out) {
    if (!out) return fail(OLMC_ERR_ARG, "null pointer");
    JumpContract jc;
    int rc = jd_contract(S, T, r, sigma, q, is_call, model, n_steps, &jc);
    if (rc) return rc;
    rc = path_payoff_check(payoff, barrier, OLJD_EUROPEAN);
    if (rc) return rc;
    const PathPayoff pp = path_payoff(S, K, is_call, payoff, barrier);
    const bool bad = jd_poisoned(S, K, T, r, sigma, q, model) || pp.nan_barrier;
    const double inv_steps = 1.0 / n_steps;                  // n_steps < 1 was refused by make_jump
    return run_structured(path_offset, n_local, n_steps, seed, antithetic, r, T, bad, out,
                          [&](int32_t grid, hipStream_t st, const EventPair* timed, const PathRange& pr, const ReduceWs& ws) {
                              with_path_family(payoff, OLJD_EUROPEAN, [&](auto f) {
                                  with_bool(antithetic != 0, [&](auto a) {
                                      launch_timed(jump_path_kernel<f, a>, dim3(grid), dim3(kBlock), st, timed, pr, jc, pp.ec, inv_steps, ws);
                                  });
                              });
                          });
}

extern "C" int oljd_surface_prices(double S, double T, double r, double sigma, double q, int is_call, const oljd_model* model, const double* strikes,
                                   const int32_t* steps, int32_t k, int64_t path_offset, int64_t n_local, int32_t n_steps, uint64_t seed,
                                   int antithetic, olmc_stats* out) {
    if (!strikes || !steps || !out) return fail(OLMC_ERR_ARG, "null pointer");
    JumpContract jc;
    const int rc = jd_contract(S, T, r, sigma, q, is_call, model, n_steps, &jc);
    if (rc) return rc;
    return run_philox_surface(strikes, steps, k, {path_offset, n_local, n_steps, seed, antithetic}, r, T,
                              jd_poisoned(S, 0.0, T, r, sigma, q, model), out, no_setup,
                              [&](int32_t grid, hipStream_t st, const EventPair* timed, const PathRange& pr, const HestonSurfaceCells& cells,
                                  const ReduceWs& ws) {
        with_bool(antithetic != 0, [&](auto a) {
            launch_timed(jump_surface_kernel<a>, dim3(grid), dim3(kBlock), st, timed, pr, jc, cells, ws);
        });
    });
}

extern "C" int oljd_autocallable(double S, double T, double r, double sigma, double q, const oljd_model* model, double autocall_barrier,
                                 double coupon_barrier, double coupon_rate, double ki_barrier, int32_t observation_freq, int64_t path_offset,
                                 int64_t n_local, int32_t n_steps, uint64_t seed, int antithetic, olmc_stats* out) {
    if (!out) return fail(OLMC_ERR_ARG, "null pointer");
    JumpContract jc;
    int rc = jd_contract(S, T, r, sigma, q, 1, model, n_steps, &jc);
    if (rc) return rc;
    rc = autocall_check(observation_freq, n_steps);
    if (rc) return rc;
    const AutocallSetup a = make_autocall(S, T, r, 0.0, q, autocall_barrier, coupon_barrier, coupon_rate, ki_barrier, observation_freq, n_steps);
    // payoffs are already discounted path by path, as olmc_autocallable's: no outer discount
    return run_jd_product<HestonAutocall>(jc, a.ac, 0.0, T, a.bad || jd_poisoned(S, 1.0, T, r, sigma, q, model), path_offset, n_local, n_steps, seed,
                                          antithetic, out);
}

extern "C" int oljd_cliquet(double S, double T, double r, double sigma, double q, const oljd_model* model, double local_cap, double local_floor,
                            double global_cap, double global_floor, int32_t n_periods, int64_t path_offset, int64_t n_local, int32_t n_steps,
                            uint64_t seed, int antithetic, olmc_stats* out) {
    if (!out) return fail(OLMC_ERR_ARG, "null pointer");
    JumpContract jc;
    int rc = jd_contract(S, T, r, sigma, q, 1, model, n_steps, &jc);
    if (rc) return rc;
    rc = cliquet_check(n_periods, n_steps);
    if (rc) return rc;
    const CliquetContract cc = make_cliquet(S, T, r, 0.0, q, local_cap, local_floor, global_cap, global_floor, n_periods, n_steps);
    const bool bad = cliquet_poisoned(S, T, r, sigma, q, local_cap, local_floor, global_cap, global_floor) || jd_poisoned(S, 1.0, T, r, sigma, q, model);
    return run_jd_product<HestonCliquet>(jc, cc, r, T, bad, path_offset, n_local, n_steps, seed, antithetic, out);
}

extern "C" int oljd_paths(double S, double T, double r, double sigma, double q, const oljd_model* model, int64_t n_paths, int32_t n_steps,
                          uint64_t seed, int mirror, int path_major, double* out_host) {
    if (!out_host) return fail(OLMC_ERR_ARG, "null pointer");
    JumpContract jc;
    const int rc = jd_contract(S, T, r, sigma, q, 1, model, n_steps, &jc);
    if (rc) return rc;
    return run_philox_matrix(n_paths, n_steps, seed, out_host, no_setup,
                             [&](DeviceCtx* c, int32_t grid, const PathRange& pr, double* d_paths) {
        with_bool(path_major != 0, [&](auto pm) {
            launch_timed(jump_legs_paths_kernel<pm>, dim3(grid), dim3(kBlock), c->stream, nullptr, pr, jc, S, static_cast<int32_t>(mirror != 0), d_paths);
        });
    });
}

// ====================================================== jump-diffusion scenario sets and fused Greeks ====
// include/olmc_jump_scenarios.h: k scenarios on one walk over olmc_jump_paths' draws.  The grouping and the kernel's argument are host
// arithmetic (olmc_host_math.h: jump_scenario_set), the launch is the Heston scenario sets' -- the same range, grid and rows, one launch
// of jump_scenarios_kernel at the smallest instantiated group bound that holds the launch's groups.
namespace {
static_assert(sizeof(JumpScenarioSet) <= 2048, "the scenario set travels by value in the kernel arguments");
constexpr int kJumpGroupBounds[] = {2, 4, 16};

// The checks of a scenario list that need no device, in the order olmc_jump_scenarios.h lists them: the model's are make_jump's.
int jump_scenario_check(const oljs_scenario* sc, int32_t k, int32_t n_steps, const olmc_stats* out) {
    if (!sc || !out) return fail(OLMC_ERR_ARG, "null pointer");
    if (k < 1 || k > OLMC_MAX_BATCH) return fail(OLMC_ERR_ARG, "the number of scenarios must be in [1, OLMC_MAX_BATCH]");
    if (n_steps < 1) return fail(OLMC_ERR_ARG, "n_steps must be >= 1");
    for (int32_t i = 0; i < k; ++i) {
        const oljs_scenario& s = sc[i];
        if (s.T <= 0.0) return fail(OLMC_ERR_ARG, "T must be > 0 in every scenario");
        JumpContract unused;      // a NaN intensity is a NaN input, not a negative one (jd_contract)
        const int rc = make_jump(s.S, s.K, s.T, s.r, s.sigma, s.q, s.is_call, s.model, std::isnan(s.lambda_j) ? 0.0 : s.lambda_j, s.a1, s.a2, s.a3,
                                 n_steps, &unused);
        if (rc) return rc;
    }
    return OLMC_OK;
}

template <int B = 0>
void launch_jump_scenarios(int32_t n_groups, bool anti, int32_t grid, hipStream_t st, const EventPair* timed, const JumpScenarioSet& set,
                           const PathRange& pr, const ReduceWs& ws) {
    constexpr int bound = kJumpGroupBounds[B];
    if constexpr (B + 1 < static_cast<int>(sizeof kJumpGroupBounds / sizeof *kJumpGroupBounds)) {
        if (n_groups > bound) return launch_jump_scenarios<B + 1>(n_groups, anti, grid, st, timed, set, pr, ws);
    }
    with_bool(anti, [&](auto a) { launch_timed(jump_scenarios_kernel<bound, decltype(a)::value>, dim3(grid), dim3(kBlock), st, timed, set, pr, ws); });
}

int run_jump_scenarios(const oljs_scenario* sc, int32_t k, int64_t path_offset, int64_t n_local, int32_t n_steps, uint64_t seed, int antithetic,
                       olmc_stats* out) {
    int rc = jump_scenario_check(sc, k, n_steps, out);
    if (rc) return rc;
    rc = check_paths(path_offset, n_local, n_steps);
    if (rc) return rc;
    JumpScenarioSet set;
    int32_t slot_of[OLMC_MAX_BATCH];
    if (const char* bad = jump_scenario_set(sc, k, n_steps, &set, slot_of)) return fail(OLMC_ERR_ARG, bad);
    CtxLease lease;
    rc = ctx_lease(&lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    const PathRange pr = make_range(path_offset, n_local, n_steps, seed);
    rc = launch_reduce(c, c->stream, c->d_result, -1.0, 2 * kSurfaceCells, grid_for(n_local),
                       [&](int32_t grid, hipStream_t st, const EventPair* timed, const ReduceWs& ws) {
                           launch_jump_scenarios(set.n_groups, antithetic != 0, grid, st, timed, set, pr, ws);
                       });
    if (rc) return rc;
    const int64_t n = n_local * (antithetic ? 2 : 1);
    for (int32_t i = 0; i < k; ++i) {
        const int32_t j = slot_of[i];
        if (jump_scenario_poisoned(sc[i])) nan_stats(n, &out[i]);
        else finish_stats(c->h_result[2 * j], c->h_result[2 * j + 1], n, sc[i].r, sc[i].T, &out[i]);
    }
    return OLMC_OK;
}
}  // namespace

// The grouping of a scenario list (pure host arithmetic: needs no device).
extern "C" int oljs_layout(const oljs_scenario* sc, int32_t k, int32_t* n_groups, int32_t* group) {
    if (!sc || !n_groups || !group) return fail(OLMC_ERR_ARG, "null pointer");
    if (const char* bad = jump_scenario_groups(sc, k, n_groups, group)) return fail(OLMC_ERR_ARG, bad);
    return OLMC_OK;
}

extern "C" int oljs_scenarios(const oljs_scenario* sc, int32_t k, int64_t path_offset, int64_t n_local, int32_t n_steps, uint64_t seed,
                              int antithetic, olmc_stats* out) {
    return run_jump_scenarios(sc, k, path_offset, n_local, n_steps, seed, antithetic, out);
}

// The 7 / 8 / 11 / 14 contracts of compute_greeks_unified under the model as ONE scenario launch: GreeksSet as it stands (bumps, call
// order, finish), two jump groups (T and T - h_T).
extern "C" int oljs_greeks_fd(double S, double K, double T, double r, double sigma, double q, int is_call, const oljd_model* model,
                              int64_t n_paths, int32_t n_steps, uint64_t seed, int antithetic, int second_order, double* out9,
                              olmc_stats* evals) {
    if (!out9 || !model) return fail(OLMC_ERR_ARG, "null pointer");
    if (!(T > 0.0)) return fail(OLMC_ERR_ARG, "T must be > 0");
    const GreeksSet gs(S, K, T, r, sigma, q, is_call, second_order);
    oljs_scenario sc[OLMC_MAX_BATCH];
    jump_greeks_scenarios(gs, *model, sc);
    olmc_stats st[OLMC_MAX_BATCH];
    const int rc = run_jump_scenarios(sc, gs.k, 0, n_paths, n_steps, seed, antithetic, st);
    if (rc) return rc;
    gs.finish(st, T, out9, evals);
    return OLMC_OK;
}

namespace {
// k (2 .. 16) contracts on the points of q, ONE launch (european_qmc_batch_kernel) whose grid covers them all, queued on c's own
// stream behind the table: the 2 nsets sums then `tail` at d_out, contract i's pair at slot pos[i] (launch_reduce: blocks when d_out
// is c->d_result).
int qmc_batch_device(DeviceCtx* c, const olmc_option* opts, int32_t k, const SobolCall& q, double* d_out, double tail, int* pos, bool profiled) {
    const QmcShape sh = qmc_shape(q);
    if (k < 2 || (sh.units + kBlock - 1) / kBlock > kMaxGrid)
        return fail(OLMC_ERR_ARG, "a shard of fused Sobol contracts needs 2 .. 16 contracts and points one grid covers");
    const uint32_t *d_sv, *d_shift;
    int rc = qmc_table(c, q, &d_sv, &d_shift);
    if (rc) return rc;
    const QmcRange qr = q.range();
    const int32_t dims = q.dims();
    const int32_t grid = sh.split ? sh.grid : static_cast<int32_t>((sh.units + kBlock - 1) / kBlock);     // the grid covers every point / block
    const int nsets = k <= 8 ? 8 : 16;
    return launch_reduce(c, c->stream, d_out, tail, 2 * nsets, grid, [&](int32_t g, hipStream_t s, const EventPair* timed, const ReduceWs& ws) {
        // make_contract(o, dims) IS gbm_qmc.py:38-44: dt = T / dims, drift * dims, sigma sqrt(dt)
        if (nsets == 8) {
            ContractSet<8> cs;
            group_contracts<8>(opts, k, dims, &cs, pos);
            launch_qmc_batch<8>(sh, g, s, timed, qr, cs, d_sv, d_shift, ws);
        } else {
            ContractSet<16> cs;
            group_contracts<16>(opts, k, dims, &cs, pos);
            launch_qmc_batch<16>(sh, g, s, timed, qr, cs, d_sv, d_shift, ws);
        }
    }, profiled);
}

// k contracts on the same Sobol points, ONE launch (qmc_batch_device); falls back to k launches beyond the size one grid covers.
// out[i] = stats of opts[i].
int run_qmc_batch(const olmc_option* opts, int32_t k, const SobolArgs& args, olmc_stats* out) {
    if (!opts || !out) return fail(OLMC_ERR_ARG, "null pointer");
    if (k < 1 || k > OLMC_MAX_BATCH) return fail(OLMC_ERR_ARG, "batch size must be in [1, OLMC_MAX_BATCH]");
    int rc;
    const auto q = SobolCall::make(args, 1, &rc);
    if (!q) return rc;
    const int64_t units = qmc_shape(*q).units;
    if (k == 1 || (units + kBlock - 1) / kBlock > kMaxGrid) {             // one contract, or more points than a grid covers: literal launches
        for (int i = 0; i < k; ++i) {
            rc = run_qmc(opts[i], *q, &out[i], nullptr);
            if (rc) return rc;
        }
        return OLMC_OK;
    }
    CtxLease lease;
    rc = ctx_lease(&lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    int pos[OLMC_MAX_BATCH];
    rc = qmc_batch_device(c, opts, k, *q, c->d_result, -1.0, pos, true);
    if (rc) return rc;
    finish_set(c->h_result, pos, q->count, opts, k, false, false, out);
    return OLMC_OK;
}
}  // namespace

extern "C" int olmc_european_qmc_batch(const olmc_option* opts, int32_t k, int64_t point_offset, int64_t n_paths, int32_t dims,
                                       const uint32_t* sv, const uint32_t* shift, int32_t bits, olmc_stats* out) {
    return run_qmc_batch(opts, k, {OLMC_QMC_SEQUENTIAL, point_offset, n_paths, dims, sv, shift, bits, 0}, out);
}

extern "C" int olmc_european_qmc_greeks_fd(double S, double K, double T, double r, double sigma, double q, int is_call, int64_t n_paths,
                                           int32_t dims, const uint32_t* sv, const uint32_t* shift, int32_t bits, int second_order,
                                           double* out9, olmc_stats* evals) {
    if (!out9) return fail(OLMC_ERR_ARG, "null pointer");
    if (!(T > 0.0)) return fail(OLMC_ERR_ARG, "T must be > 0 (price() returns intrinsic value without simulating)");
    const GreeksSet gs(S, K, T, r, sigma, q, is_call, second_order);
    olmc_stats st[OLMC_MAX_BATCH];
    int rc = run_qmc_batch(gs.o, gs.k, {OLMC_QMC_SEQUENTIAL, 0, n_paths, dims, sv, shift, bits, 0}, st);
    if (rc) return rc;
    gs.finish(st, T, out9, evals);
    return OLMC_OK;
}

// ======================================================== multi-GPU (RCCL) ====
// librccl is resolved lazily (dlopen) so single-GPU users never load it; the TYPES and ENUM VALUES come from
// <rccl/rccl.h> at compile time, so a header / library mismatch is a build-time matter, not a guessed constant.
//
// One process, n ranks (rank d = device d).  An ENGINE exists per list of devices: per rank a context of its own (ctx_create: stream,
// workspaces, Sobol table; in no pool, so nobody else ever leases it), a send / receive buffer and a LAUNCHER THREAD bound to the
// rank's device at birth (one hipSetDevice, ever -- SURVEY §8e: "one host thread per device + ncclCommInitAll"), plus the list's
// communicators.  A rank's table upload, path kernel, collective and fetch all run on its context's stream.  A call
//   1. posts the launch job: every launcher queues its rank's path kernel at once (round 4 queued them one after the other from the
//      calling thread: rank 7's kernel started seven enqueues late);
//   2. queues ONE grouped all-reduce of `count` doubles from the calling thread (3 for a price, 2 nsets + 1 for finite-difference
//      Greeks, 6 for the control variate: SURVEY §8e) -- only after every rank has launched, so a rank that failed leaves no peer
//      waiting inside a collective;
//   3. posts the drain job (launchers 1 .. n-1 wait for their streams) and meanwhile takes the reduced values home through rank 0's
//      polled completion word (fetch_dev); every rank holds the same values.
// Calls on device lists that share no device run concurrently; lists that share one queue behind that device's mutex (two
// communicators driven at once on one device may deadlock inside RCCL).  OLMC_TUNE_MULTI_LAUNCH = -1 keeps round 4's serial form
// (everything from the calling thread) for A/B; both forms give the same bits.
namespace {
struct Rccl {
    void* lib = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
};
Rccl g_rccl;
std::mutex g_rccl_mu;

int rccl_load() {
    std::lock_guard<std::mutex> lock(g_rccl_mu);
    if (g_rccl.lib) return OLMC_OK;
    void* h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) return fail(OLMC_ERR_RCCL, std::string("cannot load librccl: ") + dlerror());
    g_rccl.CommInitAll = reinterpret_cast<decltype(g_rccl.CommInitAll)>(dlsym(h, "ncclCommInitAll"));
    g_rccl.CommDestroy = reinterpret_cast<decltype(g_rccl.CommDestroy)>(dlsym(h, "ncclCommDestroy"));
    g_rccl.AllReduce = reinterpret_cast<decltype(g_rccl.AllReduce)>(dlsym(h, "ncclAllReduce"));
    g_rccl.GroupStart = reinterpret_cast<decltype(g_rccl.GroupStart)>(dlsym(h, "ncclGroupStart"));
    g_rccl.GroupEnd = reinterpret_cast<decltype(g_rccl.GroupEnd)>(dlsym(h, "ncclGroupEnd"));
    g_rccl.GetErrorString = reinterpret_cast<decltype(g_rccl.GetErrorString)>(dlsym(h, "ncclGetErrorString"));
    if (!g_rccl.CommInitAll || !g_rccl.AllReduce || !g_rccl.GroupStart || !g_rccl.GroupEnd || !g_rccl.CommDestroy) {
        dlclose(h);
        return fail(OLMC_ERR_RCCL, "librccl is missing required symbols");
    }
    g_rccl.lib = h;
    return OLMC_OK;
}

std::string rccl_message(const char* what, ncclResult_t r) {
    return std::string(what) + ": " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "rccl error");
}

#define RCCL_TRY(expr)                                                                \
    do {                                                                              \
        ncclResult_t r_ = (expr);                                                     \
        if (r_ != ncclSuccess) return fail(OLMC_ERR_RCCL, rccl_message(#expr, r_));   \
    } while (0)

constexpr int kMultiValues = kMaxNV + 1;            // the widest payload: 2 x 16 sums + n

struct MultiEngine;

struct MultiRank {
    int device = -1;
    DeviceCtx* ctx = nullptr;                       // the rank's own: its stream is the rank stream
    DeviceBlock<Mem> buffers;                       // d_send and d_recv
    double* d_send = nullptr;                       // [kMultiValues] this rank's sums (written by its path kernel's last workgroup)
    double* d_recv = nullptr;                       // [kMultiValues] the reduced sums
    hipEvent_t queued = nullptr;                    // rehearsal only: the rank's path kernel is queued behind this
    std::thread launcher;                           // bound to `device`; runs the engine's jobs for this rank
    int rc = OLMC_OK;                               // of the job it ran last (read by the caller behind the job's completion count)
    std::string error;
    std::chrono::steady_clock::time_point began, ended;     // of that job, on the launcher's clock (olmc_multi_gpu_spans: wake latency, own time)
};

struct MultiEngine {
    std::vector<MultiRank> ranks;                   // sized once, before the launchers start
    std::vector<int> devices;                       // device of every rank: what `ranks` and `comms` were built for
    std::vector<ncclComm_t> comms;                  // empty in a rehearsal
    bool rehearsal = false;
    JobBoard board;                                 // the hand-over between the calling thread and the launchers (olmc_job_board.h)
};

std::mutex g_engines_mu;                            // guards g_engines (never held while a call runs)
std::vector<MultiEngine*> g_engines;                // one per (device list, rehearsal) asked for since the last olmc_shutdown
std::mutex g_multi_dev_mu[kMaxDevices];             // a multi-GPU call holds the mutex of every device of its list (ascending order)
thread_local double t_multi_spans[8] = {0, 0, 0, 0, 0, 0, 0, 0};

void launcher_main(MultiEngine* e, int d, uint32_t seen) {
    MultiRank& rk = e->ranks[d];
    (void)hipSetDevice(rk.device);                  // once: every launch of this thread goes to this device
    t_device = rk.device;
    using clock = std::chrono::steady_clock;
    while (const std::function<int(int)>* work = board_next(e->board, d, seen)) {
        rk.began = clock::now();
        rk.rc = (*work)(d);
        if (rk.rc) rk.error = t_error;
        rk.ended = clock::now();
        board_done(e->board);
    }
}

void engine_post(MultiEngine* e, const std::function<int(int)>* work, int first_rank) { board_post(e->board, work, first_rank); }

// Waits for the posted job; the first failing rank's status and message become the caller's.
int engine_wait(MultiEngine* e) {
    board_wait(e->board);
    for (size_t d = static_cast<size_t>(e->board.first_rank); d < e->ranks.size(); ++d)
        if (e->ranks[d].rc) return fail(e->ranks[d].rc, "rank " + std::to_string(d) + ": " + e->ranks[d].error);
    return OLMC_OK;
}

void engine_destroy(MultiEngine* e) {
    if (std::any_of(e->ranks.begin(), e->ranks.end(), [](const MultiRank& rk) { return rk.launcher.joinable(); })) {
        engine_post(e, nullptr, 0);                 // work == nullptr: leave
        for (MultiRank& rk : e->ranks)
            if (rk.launcher.joinable()) rk.launcher.join();
    }
    for (ncclComm_t cm : e->comms)
        if (cm && g_rccl.CommDestroy) g_rccl.CommDestroy(cm);
    for (MultiRank& rk : e->ranks) {
        if (rk.device < 0 || hipSetDevice(rk.device) != hipSuccess) continue;
        if (rk.ctx) ctx_release(rk.ctx);
        (void)rk.buffers.reset();
        if (rk.queued) (void)hipEventDestroy(rk.queued);
    }
    (void)hipGetLastError();
    delete e;
}

// olmc_shutdown: the caller's contract is that no call is in flight.
void multi_gpu_release() {
    std::vector<MultiEngine*> all;
    {
        std::lock_guard<std::mutex> lock(g_engines_mu);
        all.swap(g_engines);
    }
    for (MultiEngine* e : all) engine_destroy(e);
}

// Contexts, buffers, launchers and communicators for exactly this list of devices.  Called with the devices' mutexes held.
int engine_build(const std::vector<int>& devs, bool rehearsal, MultiEngine** out) {
    MultiEngine* e = new MultiEngine();
    e->rehearsal = rehearsal;
    e->devices = devs;
    e->ranks.resize(devs.size());
    auto bail = [&](int rc) { engine_destroy(e); return rc; };
    for (size_t d = 0; d < devs.size(); ++d) {
        MultiRank& rk = e->ranks[d];
        const int rc = ctx_create(devs[d], &rk.ctx);      // leaves devs[d] the current device
        if (rc) return bail(fail(rc, "multi-GPU engine, rank " + std::to_string(d) + ": " + t_error));
        rk.device = devs[d];
        constexpr int kStride = 64;                  // doubles: the receive buffer starts on its own 512-byte boundary (the collective's vector accesses)
        static_assert(kStride >= kMultiValues, "rank buffers hold the widest payload");
        if (rk.buffers.reserve(sizeof(double) * 2 * kStride, no_users)) return bail(fail(OLMC_ERR_HIP, "multi-GPU engine, rank " + std::to_string(d) + ": " + t_error));
        rk.d_send = rk.buffers.as<double>();
        rk.d_recv = rk.d_send + kStride;
        const hipError_t err = hipEventCreateWithFlags(&rk.queued, hipEventDisableTiming);
        if (err != hipSuccess) return bail(fail(OLMC_ERR_HIP, std::string("multi-GPU engine, rank ") + std::to_string(d) + ": " + hipGetErrorString(err)));
    }
    if (!rehearsal) {
        int rc = rccl_load();
        if (rc) return bail(rc);
        e->comms.assign(devs.size(), nullptr);
        std::vector<int> list = devs;
        const ncclResult_t r = g_rccl.CommInitAll(e->comms.data(), static_cast<int>(list.size()), list.data());
        if (r != ncclSuccess) return bail(fail(OLMC_ERR_RCCL, rccl_message("ncclCommInitAll", r)));
    }
    if (devs.size() > 1) {                           // one rank needs no launcher: the calling thread is as good
        e->board.n_ranks = static_cast<int>(devs.size());
        try {
            for (size_t d = 0; d < devs.size(); ++d) e->ranks[d].launcher = std::thread(launcher_main, e, static_cast<int>(d), e->board.job_no.load());
        } catch (const std::system_error& err) {
            return bail(fail(OLMC_ERR_STATE, std::string("multi-GPU engine: cannot start a launcher thread: ") + err.what()));
        }
    }
    *out = e;
    return OLMC_OK;
}

int engine_for(const std::vector<int>& devs, bool rehearsal, MultiEngine** out) {
    {
        std::lock_guard<std::mutex> lock(g_engines_mu);
        for (MultiEngine* e : g_engines)
            if (e->devices == devs && e->rehearsal == rehearsal) { *out = e; return OLMC_OK; }
    }
    // A caller that keeps changing its device list (a rehearsal sweeping 1 .. 12 ranks on one device) must not pile up streams and
    // parked launchers for ever: beyond kMaxEngines the oldest engines go -- but only engines ALL of whose devices this call has
    // locked (nobody can be inside them), oldest first.
    constexpr size_t kMaxEngines = 4;
    std::vector<MultiEngine*> evicted;
    {
        std::lock_guard<std::mutex> lock(g_engines_mu);
        for (size_t i = 0; i < g_engines.size() && g_engines.size() >= kMaxEngines;) {
            const std::vector<int>& theirs = g_engines[i]->devices;
            const bool ours = std::all_of(theirs.begin(), theirs.end(), [&](int d) { return std::find(devs.begin(), devs.end(), d) != devs.end(); });
            if (!ours) { ++i; continue; }
            evicted.push_back(g_engines[i]);
            g_engines.erase(g_engines.begin() + static_cast<std::ptrdiff_t>(i));
        }
    }
    for (MultiEngine* old : evicted) engine_destroy(old);      // joins its launchers, frees its rank contexts
    MultiEngine* e = nullptr;
    const int rc = engine_build(devs, rehearsal, &e);      // the devices' mutexes are held: nobody else builds this list meanwhile
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(g_engines_mu);
    g_engines.push_back(e);
    *out = e;
    return OLMC_OK;
}

// Whatever way a multi-GPU call leaves (any of its error returns included), the calling thread gets back the library device and
// the HIP current device it came in with, and every rank stream a kernel was already queued on has been drained, so no launch of
// a failed call is still running behind the caller's next one.  It also holds the device mutexes of the call.
struct MultiGpuScope {
    int saved_lib_device, saved_hip_device = -1;
    MultiEngine* engine = nullptr;
    std::vector<int> launched;          // ranks with work queued by this call
    std::vector<int> locked;            // devices whose multi-GPU mutex this call holds
    explicit MultiGpuScope(int lib_device) : saved_lib_device(lib_device) { (void)hipGetDevice(&saved_hip_device); }
    void lock_devices(const std::vector<int>& devs) {
        locked = devs;
        std::sort(locked.begin(), locked.end());
        locked.erase(std::unique(locked.begin(), locked.end()), locked.end());
        for (int d : locked) g_multi_dev_mu[d].lock();
    }
    ~MultiGpuScope() {
        if (engine)
            for (int d : launched) {
                const MultiRank& rk = engine->ranks[d];
                if (hipSetDevice(rk.device) == hipSuccess && hipStreamSynchronize(rk.ctx->stream) != hipSuccess) ws_recover(rk.ctx);
            }
        for (auto it = locked.rbegin(); it != locked.rend(); ++it) g_multi_dev_mu[*it].unlock();
        t_device = saved_lib_device;
        if (saved_hip_device >= 0) (void)hipSetDevice(saved_hip_device);
        (void)hipGetLastError();
    }
};

// The grouped all-reduce of `count` doubles, one per rank stream.  The group is CLOSED on every path out (an error between
// ncclGroupStart and ncclGroupEnd would otherwise leave the calling thread inside an open group for good).
int grouped_allreduce(MultiEngine* e, int count) {
    RCCL_TRY(g_rccl.GroupStart());
    ncclResult_t bad = ncclSuccess;
    for (size_t d = 0; d < e->ranks.size() && bad == ncclSuccess; ++d) {
        const MultiRank& rk = e->ranks[d];
        bad = g_rccl.AllReduce(rk.d_send, rk.d_recv, static_cast<size_t>(count), ncclFloat64, ncclSum, e->comms[d], rk.ctx->stream);
    }
    const ncclResult_t end = g_rccl.GroupEnd();
    if (bad != ncclSuccess) return fail(OLMC_ERR_RCCL, rccl_message("ncclAllReduce", bad));
    if (end != ncclSuccess) return fail(OLMC_ERR_RCCL, rccl_message("ncclGroupEnd", end));
    return OLMC_OK;
}

#ifdef OLMC_WITH_PROBES
// The instrumented build's stand-in for the collective when n ranks are REHEARSED on one device (RCCL refuses two ranks on one
// GPU): every rank adds the n send buffers in rank order.
struct RankBuffers {
    const double* send[kMaxDevices];
};
__global__ void rehearsal_allreduce_kernel(RankBuffers in, int n_ranks, int count, double* __restrict__ recv) {
    const int t = threadIdx.x;
    if (t >= count) return;
    double sum = 0.0;
    for (int r = 0; r < n_ranks; ++r) sum += in.send[r][t];
    recv[t] = sum;
}

int rehearsal_allreduce(MultiEngine* e, int count) {
    const int n = static_cast<int>(e->ranks.size());
    RankBuffers in{};
    for (int d = 0; d < n; ++d) {
        in.send[d] = e->ranks[d].d_send;
        HIP_TRY(hipEventRecord(e->ranks[d].queued, e->ranks[d].ctx->stream));
    }
    for (int d = 0; d < n; ++d) {
        for (int o = 0; o < n; ++o)
            if (o != d) HIP_TRY(hipStreamWaitEvent(e->ranks[d].ctx->stream, e->ranks[o].queued, 0));
        hipLaunchKernelGGL(rehearsal_allreduce_kernel, dim3(1), dim3(kWave), 0, e->ranks[d].ctx->stream, in, n, count, e->ranks[d].d_recv);
        HIP_TRY(hipGetLastError());
    }
    return OLMC_OK;
}
#endif

// The skeleton every multi-GPU entry point shares.  launch(rank, lo, n_local, c, d_send) queues rank's path kernel on the stream of
// the rank's own context c, unprofiled (no olmc_kernel_time drains c's events: c is in no pool), and must leave `count` doubles at
// d_send; host receives their sums.  `launch` runs on the launcher threads, one rank each, at the same time: it must not write
// shared state.
template <typename Launch>
int multi_gpu_run(int n_gpus, int64_t n_paths, int32_t n_steps, int count, Launch launch, double* host, bool sobol_points = false) {
    if (n_gpus < 1 || n_gpus > kMaxDevices) return fail(OLMC_ERR_ARG, "n_gpus out of range");
    int rc = check_paths(0, n_paths, n_steps);
    if (rc) return rc;
    if (n_paths < n_gpus) return fail(OLMC_ERR_ARG, "fewer paths than GPUs");
    if (count < 1 || count > kMultiValues) return fail(OLMC_ERR_STATE, "payload wider than the rank buffers");
    bool rehearsal = false;
#ifdef OLMC_WITH_PROBES
    rehearsal = g_multi_rehearsal != 0;
#endif
    int visible = 0;
    hipError_t e = hipGetDeviceCount(&visible);
    if (e != hipSuccess || visible < (rehearsal ? 1 : n_gpus))
        return fail(OLMC_ERR_HIP, "requested " + std::to_string(n_gpus) + " GPUs, " + std::to_string(visible) + " visible");
    using clock = std::chrono::steady_clock;
    const int home = t_device >= 0 ? t_device : (g_default_device.load() >= 0 ? g_default_device.load() : 0);
    MultiGpuScope scope(home);
    std::vector<int> devs(n_gpus);
    for (int d = 0; d < n_gpus; ++d) devs[d] = rehearsal ? home : d;
    if (home >= kMaxDevices) return fail(OLMC_ERR_ARG, "device index out of range");
    scope.lock_devices(devs);
    for (int d = 0; d < n_gpus; ++d)
        if (!g_pool[devs[d]].load(std::memory_order_acquire)) { rc = olmc_init(devs[d]); if (rc) return rc; }      // olmc_init moves t_device: the guard puts it back
    MultiEngine* eng = nullptr;
    rc = engine_for(devs, rehearsal, &eng);
    if (rc) return rc;
    scope.engine = eng;
    const bool threaded = n_gpus > 1 && g_multi_launch >= 0;
    const auto t0 = clock::now();
    // 1. every rank's path kernel: contiguous global path ranges, rank d owns [d N / P, (d + 1) N / P)  
    const std::function<int(int)> launch_rank = [&](int d) -> int {
        const MultiRank& rk = eng->ranks[d];
        int64_t lo, n_local;
        if (sobol_points) qmc_shard_range(n_paths, d, n_gpus, &lo, &n_local);
        else shard_range(n_paths, d, n_gpus, &lo, &n_local);
#ifdef OLMC_WITH_PROBES
        if (g_fault_shard == d + 1) return fail(OLMC_ERR_HIP, "injected shard failure (OLMC_PROBE_TUNE_FAULT_SHARD)");
#endif
        return launch(d, lo, n_local, rk.ctx, rk.d_send);
    };
    if (threaded) {
        for (int d = 0; d < n_gpus; ++d) scope.launched.push_back(d);       // any of them may have queued work by the time one fails
        engine_post(eng, &launch_rank, 0);
        rc = engine_wait(eng);
        if (rc) return rc;
    } else {
        for (int d = 0; d < n_gpus; ++d) {
            HIP_TRY(hipSetDevice(eng->ranks[d].device));
            t_device = eng->ranks[d].device;
            scope.launched.push_back(d);
            rc = launch_rank(d);
            if (rc) return rc;
        }
    }
    const auto t1 = clock::now();
    auto us = [](clock::time_point a, clock::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
    double wake_max = 0.0, own_max = 0.0, own_min = 0.0;      // launcher threads: how late the slowest one began, how long a rank's own launch took
    if (threaded) {
        own_min = 1e30;
        for (const MultiRank& rk : eng->ranks) {
            wake_max = std::max(wake_max, us(t0, rk.began));
            own_max = std::max(own_max, us(rk.began, rk.ended));
            own_min = std::min(own_min, us(rk.began, rk.ended));
        }
    } else {
        own_max = own_min = us(t0, t1) / n_gpus;
    }
    // 2. the collective: queued on every rank stream before the first wait
    if (!rehearsal) {
        rc = grouped_allreduce(eng, count);
        if (rc) return rc;
    } else {
#ifdef OLMC_WITH_PROBES
        rc = rehearsal_allreduce(eng, count);
        if (rc) return rc;
#endif
    }
    const auto t2 = clock::now();
    // 3. The sums come home the way every blocking pricing's result does: a one-wave kernel behind the all-reduce on rank 0 writes
    // them into a pinned buffer and raises the completion word the host polls (fetch_dev); the other ranks hold the same sums
    // and finish with the same collective -- their launchers wait for their streams meanwhile.
    const std::function<int(int)> drain_rank = [&](int d) -> int {
        const hipError_t err = hipStreamSynchronize(eng->ranks[d].ctx->stream);
        return err == hipSuccess ? OLMC_OK : fail(OLMC_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(err));
    };
    const MultiRank& first = eng->ranks[0];
    HIP_TRY(hipSetDevice(first.device));
    t_device = first.device;
    // from the post to the wait below NOTHING may return: the job refers to this frame
    if (threaded) engine_post(eng, &drain_rank, 0);     // rank 0's launcher too: every launcher ends the call awake, and spins for the next
    rc = fetch_dev(first.ctx, first.d_recv, count, first.ctx->stream, host);
    const auto t3 = clock::now();
    if (threaded) {
        const int rc_drain = engine_wait(eng);          // always: the job refers to this frame
        if (!rc) rc = rc_drain;
    } else if (!rc) {
        for (int d = n_gpus - 1; d >= 1 && !rc; --d) {
            HIP_TRY(hipSetDevice(eng->ranks[d].device));
            rc = drain_rank(d);
        }
    }
    if (rc) return rc;
    const auto t4 = clock::now();
    t_multi_spans[5] = wake_max; t_multi_spans[6] = own_max; t_multi_spans[7] = own_min;
    t_multi_spans[0] = us(t0, t1); t_multi_spans[1] = us(t1, t2); t_multi_spans[2] = us(t2, t3); t_multi_spans[3] = us(t3, t4); t_multi_spans[4] = us(t0, t4);
#ifdef OLMC_WITH_PROBES
    // instrumented build: every rank must hold rank 0's bits (identical finalisation on every rank)
    for (int d = 1; d < n_gpus; ++d) {
        double other[kMultiValues];
        HIP_TRY(hipSetDevice(eng->ranks[d].device));
        HIP_TRY(hipMemcpy(other, eng->ranks[d].d_recv, sizeof(double) * count, hipMemcpyDeviceToHost));
        if (std::memcmp(other, host, sizeof(double) * count) != 0) return fail(OLMC_ERR_STATE, "rank " + std::to_string(d) + " holds other sums than rank 0");
    }
#endif
    scope.launched.clear();                        // rank 0 handed over by its completion word, the others drained: nothing left for the guard
    return OLMC_OK;
}

}  // namespace

extern "C" int olmc_multi_gpu_european(double S, double K, double T, double r, double sigma, double q, int is_call,
                                       int64_t n_paths, int32_t n_steps, uint64_t seed, int antithetic, int n_gpus,
                                       olmc_stats* out) {
    if (!out) return fail(OLMC_ERR_ARG, "null pointer");
    const olmc_option o = make_option(S, K, T, r, sigma, q, is_call);
    double host[3] = {0, 0, 0};
    const int rc = multi_gpu_run(n_gpus, n_paths, n_steps, 3, [&](int, int64_t lo, int64_t n_local, DeviceCtx* c, double* d_send) {
        const double n = static_cast<double>(n_local * (antithetic ? 2 : 1));      // {sum, sumsq, n}
        return run_batch_device(c, c->stream, &o, 1, lo, n_local, n_steps, seed, antithetic, d_send, n, nullptr, false);
    }, host);
    if (rc) return rc;
    finish_one(host, static_cast<int64_t>(host[2]), r, T, poisoned(S, K, T, r, sigma, q), out);
    return OLMC_OK;
}

extern "C" int olmc_multi_gpu_greeks_fd(double S, double K, double T, double r, double sigma, double q, int is_call,
                                        int64_t n_paths, int32_t n_steps, uint64_t seed, int second_order, int n_gpus,
                                        double* out9, olmc_stats* evals) {
    if (!out9) return fail(OLMC_ERR_ARG, "null pointer");
    if (!(T > 0.0)) return fail(OLMC_ERR_ARG, "T must be > 0 (price() returns intrinsic value without simulating)");
    const GreeksSet gs(S, K, T, r, sigma, q, is_call, second_order);
    const int nsets = gs.k <= 8 ? 8 : 16;
    int pos[OLMC_MAX_BATCH] = {};
    double host[kMultiValues] = {};
    const int rc = multi_gpu_run(n_gpus, n_paths, n_steps, 2 * nsets + 1, [&](int rank, int64_t lo, int64_t n_local, DeviceCtx* c, double* d_send) {
        int other[OLMC_MAX_BATCH];                                                               // every rank lays the set out alike: rank 0's
        return run_batch_device(c, c->stream, gs.o, gs.k, lo, n_local, n_steps, seed, 1, d_send, static_cast<double>(2 * n_local),
                                rank == 0 ? pos : other, false);                                 // layout is the one kept
    }, host);
    if (rc) return rc;
    olmc_stats st[OLMC_MAX_BATCH];
    finish_set(host, pos, static_cast<int64_t>(host[2 * nsets]), gs.o, gs.k, false, false, st);
    gs.finish(st, T, out9, evals);
    return OLMC_OK;
}

extern "C" int olmc_multi_gpu_european_cv(double S, double K, double T, double r, double sigma, double q, int is_call,
                                          int64_t n_paths, int32_t n_steps, uint64_t seed, int antithetic, int n_gpus,
                                          olmc_cv_moments* out) {
    if (!out) return fail(OLMC_ERR_ARG, "null pointer");
    const olmc_option o = make_option(S, K, T, r, sigma, q, is_call);
    double host[6] = {};
    const int rc = multi_gpu_run(n_gpus, n_paths, n_steps, 6, [&](int, int64_t lo, int64_t n_local, DeviceCtx* c, double* d_send) {
        return cv_device(c, c->stream, o, lo, n_local, n_steps, seed, antithetic, d_send, static_cast<double>(n_local * (antithetic ? 2 : 1)), false);
    }, host);
    if (rc) return rc;
    cv_from_device(host, static_cast<int64_t>(host[5]), S, T, r, q, out);       // d = disc * x (monte_carlo.py:175)
    if (poisoned(S, K, T, r, sigma, q)) out->value = std::nan("");
    return OLMC_OK;
}

// Scrambled-Sobol pricing over n_gpus devices (gbm_qmc.py:14-46): rank d prices POINTS [d N / P, (d + 1) N / P) of the one sequence --
// the inner boundaries rounded down to multiples of 512 points where a rank owns 4,096 or more (qmc_shard_range: every rank then
// runs the aligned kernels) -- through the point offset every Sobol kernel already takes, the ranks' {sum, sumsq, n} meet in the same all-reduce (count 3).  The
// same points as the one-device call, another association of the sums.
extern "C" int olmc_multi_gpu_european_qmc(double S, double K, double T, double r, double sigma, double q, int is_call,
                                           int64_t n_paths, int32_t dims, const uint32_t* sv, const uint32_t* shift, int32_t bits,
                                           int n_gpus, olmc_stats* out) {
    if (!out) return fail(OLMC_ERR_ARG, "null pointer");
    int rc;
    const auto call = SobolCall::make({OLMC_QMC_SEQUENTIAL, 0, n_paths, dims, sv, shift, bits, 0}, 1, &rc);
    if (!call) return rc;
    const Contract ct = qmc_contract(S, K, T, r, sigma, q, is_call, dims, false);
    double host[3] = {0, 0, 0};
    rc = multi_gpu_run(n_gpus, n_paths, dims, 3, [&](int, int64_t lo, int64_t n_local, DeviceCtx* c, double* d_send) {
        return qmc_device(c, ct, call->over(lo, n_local), false, d_send, static_cast<double>(n_local), false);
    }, host, true);
    if (rc) return rc;
    finish_one(host, static_cast<int64_t>(host[2]), r, T, poisoned(S, K, T, r, sigma, q), out);
    return OLMC_OK;
}

// The 8 / 14 bumped contracts of compute_greeks_unified on a MCMethod.QMC pricer (unified_greeks.py:295-358 over gbm_qmc.py:14-46)
// over n_gpus devices: every rank prices ALL contracts on its block of the Sobol points in one launch (european_qmc_batch_kernel),
// the 2 nsets sums and n meet in the one all-reduce (count 17 / 33, as olmc_multi_gpu_greeks_fd).
extern "C" int olmc_multi_gpu_european_qmc_greeks_fd(double S, double K, double T, double r, double sigma, double q, int is_call,
                                                     int64_t n_paths, int32_t dims, const uint32_t* sv, const uint32_t* shift,
                                                     int32_t bits, int second_order, int n_gpus, double* out9, olmc_stats* evals) {
    if (!out9) return fail(OLMC_ERR_ARG, "null pointer");
    if (!(T > 0.0)) return fail(OLMC_ERR_ARG, "T must be > 0 (price() returns intrinsic value without simulating)");
    int rc;
    const auto call = SobolCall::make({OLMC_QMC_SEQUENTIAL, 0, n_paths, dims, sv, shift, bits, 0}, 1, &rc);
    if (!call) return rc;
    const GreeksSet gs(S, K, T, r, sigma, q, is_call, second_order);
    const int nsets = gs.k <= 8 ? 8 : 16;
    int pos[OLMC_MAX_BATCH] = {};
    double host[kMultiValues] = {};
    rc = multi_gpu_run(n_gpus, n_paths, dims, 2 * nsets + 1, [&](int rank, int64_t lo, int64_t n_local, DeviceCtx* c, double* d_send) {
        int other[OLMC_MAX_BATCH];                                                               // every rank lays the set out alike: rank 0's
        return qmc_batch_device(c, gs.o, gs.k, call->over(lo, n_local), d_send, static_cast<double>(n_local), rank == 0 ? pos : other, false);
    }, host, true);
    if (rc) return rc;
    olmc_stats st[OLMC_MAX_BATCH];
    finish_set(host, pos, static_cast<int64_t>(host[2 * nsets]), gs.o, gs.k, false, false, st);
    gs.finish(st, T, out9, evals);
    return OLMC_OK;
}

// price_with_control_variate on a MCMethod.QMC pricer (monte_carlo.py:154-186 over gbm_qmc.py:14-46) over n_gpus devices: the five
// moments of the rank's block of Sobol points and n (count 6, as olmc_multi_gpu_european_cv).
extern "C" int olmc_multi_gpu_european_qmc_cv(double S, double K, double T, double r, double sigma, double q, int is_call,
                                              int64_t n_paths, int32_t dims, const uint32_t* sv, const uint32_t* shift, int32_t bits,
                                              int n_gpus, olmc_cv_moments* out) {
    if (!out) return fail(OLMC_ERR_ARG, "null pointer");
    int rc;
    const auto call = SobolCall::make({OLMC_QMC_SEQUENTIAL, 0, n_paths, dims, sv, shift, bits, 0}, 1, &rc);
    if (!call) return rc;
    const Contract ct = qmc_contract(S, K, T, r, sigma, q, is_call, dims, false);
    double host[6] = {};
    rc = multi_gpu_run(n_gpus, n_paths, dims, 6, [&](int, int64_t lo, int64_t n_local, DeviceCtx* c, double* d_send) {
        return qmc_device(c, ct, call->over(lo, n_local), true, d_send, static_cast<double>(n_local), false);
    }, host, true);
    if (rc) return rc;
    cv_from_device(host, static_cast<int64_t>(host[5]), S, T, r, q, out);
    if (poisoned(S, K, T, r, sigma, q)) out->value = std::nan("");
    return OLMC_OK;
}

// Host microseconds of the calling thread's last multi-GPU call: {launch phase (launch job posted -> every rank's kernel queued),
// collective queued, result fetched (includes the kernels' run time), other ranks drained, total, the latest launcher's start after the
// post (wake latency), the longest and the shortest single rank's own launch}.
extern "C" int olmc_multi_gpu_spans(double* out8) {
    if (!out8) return fail(OLMC_ERR_ARG, "null pointer");
    for (int i = 0; i < 8; ++i) out8[i] = t_multi_spans[i];
    return OLMC_OK;
}

// ============================================================ validation taps ====
extern "C" int olmc_philox_words(uint64_t seed, int64_t path_offset, int64_t n_paths, int32_t block0, int32_t n_blocks,
                                 uint32_t stream_tag, uint32_t* out_host) {
    if (!out_host || n_paths < 1 || n_blocks < 1 || block0 < 0 || path_offset < 0) return fail(OLMC_ERR_ARG, "bad arguments");
    CtxLease lease;
    int rc = ctx_lease(&lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    const size_t bytes = sizeof(uint32_t) * 4 * static_cast<size_t>(n_paths) * n_blocks;
    Carver bulk;
    rc = bulk_reserve(c, bytes, &bulk);
    if (rc) return rc;
    uint32_t* d_words = bulk.take<uint32_t>(bytes / sizeof(uint32_t));
    const int64_t total = n_paths * n_blocks;
    const int grid = static_cast<int>(std::min<int64_t>((total + 255) / 256, 4096));
    hipLaunchKernelGGL(philox_words_kernel, dim3(grid), dim3(256), 0, c->stream, static_cast<uint64_t>(path_offset), n_paths,
                       block0, n_blocks, stream_tag, static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), d_words);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_host, d_words, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return OLMC_OK;
}

extern "C" int olmc_normals(uint64_t seed, int64_t path_offset, int64_t n_paths, int32_t n_steps, float* out_host) {
    if (!out_host || n_paths < 1 || n_steps < 1 || path_offset < 0) return fail(OLMC_ERR_ARG, "bad arguments");
    CtxLease lease;
    int rc = ctx_lease(&lease);
    if (rc) return rc;
    DeviceCtx* const c = lease.c;
    const size_t bytes = sizeof(float) * static_cast<size_t>(n_paths) * n_steps;
    Carver bulk;
    rc = bulk_reserve(c, bytes, &bulk);
    if (rc) return rc;
    float* d_z = bulk.take<float>(bytes / sizeof(float));
    const int64_t total = n_paths * ((n_steps + 3) / 4);
    const int grid = static_cast<int>(std::min<int64_t>((total + 255) / 256, 4096));
    hipLaunchKernelGGL(normals_kernel, dim3(grid), dim3(256), 0, c->stream, static_cast<uint64_t>(path_offset), n_paths,
                       n_steps, static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), d_z);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_host, d_z, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return OLMC_OK;
}

// ================================================================ measurement ====
extern "C" int olmc_tune(int knob, int value) {
    if (knob == OLMC_TUNE_GRID_CAP && value >= 0) { g_grid_cap = value; return OLMC_OK; }
    if (knob == OLMC_TUNE_QMC_BLOCK && value >= -1 && value <= 2) { g_qmc_block = value; return OLMC_OK; }
    if (knob == OLMC_TUNE_POLL && value >= -1 && value <= 0) { g_poll = value; return OLMC_OK; }
    if (knob == OLMC_TUNE_SPLIT_TAIL && value >= -1 && value <= 0) { g_split_tail = value; return OLMC_OK; }
    if (knob == OLMC_TUNE_SPLIT_SAT && value >= 0 && value <= 16) { g_split_sat = value; return OLMC_OK; }
    if (knob == OLMC_TUNE_MULTI_LAUNCH && value >= -1 && value <= 0) { g_multi_launch = value; return OLMC_OK; }
    if (knob == OLMC_TUNE_STAGED_COPY && value >= -1 && value <= 0) { g_staged_copy = value; return OLMC_OK; }
    if (knob == OLMC_TUNE_PHILOX_TABLE && value >= 0 && value <= 1) { g_philox_table = value; return OLMC_OK; }
    return fail(OLMC_ERR_ARG, "unknown tuning knob or value");
}

namespace {
// Runs fn on EVERY context of the calling thread's device, each taken out of circulation first (waits for the calls in flight).
template <typename Fn>
int with_all_contexts(Fn fn) {
    int dev = t_device >= 0 ? t_device : g_default_device.load(std::memory_order_acquire);
    if (dev < 0) {
        int rc = olmc_init(0);
        if (rc) return rc;
        dev = t_device;
    }
    DevicePool* pool = g_pool[dev].load(std::memory_order_acquire);
    if (!pool) return fail(OLMC_ERR_STATE, "device not initialised (call olmc_init)");
    HIP_TRY(hipSetDevice(dev));
    std::vector<DeviceCtx*> mine;
    {
        std::unique_lock<std::mutex> lock(pool->mu);
        pool->idle.wait(lock, [&] { return std::none_of(pool->all.begin(), pool->all.end(), [](const DeviceCtx* c) { return c->busy; }); });
        mine = pool->all;
        for (DeviceCtx* c : mine) c->busy = true;
    }
    int rc = OLMC_OK;
    for (DeviceCtx* c : mine) {
        const int r = fn(c);
        if (r && !rc) rc = r;
    }
    {
        std::lock_guard<std::mutex> lock(pool->mu);
        for (DeviceCtx* c : mine) c->busy = false;
    }
    pool->idle.notify_all();
    return rc;
}
}  // namespace

extern "C" int olmc_profile_enable(int on) {
    g_profile = on != 0;
    if (g_profile && (t_device >= 0 || g_default_device.load() >= 0)) {
        // pre-create the event pairs a measurement pass will consume, so that no hipEventCreate lands inside a timed call
        // (context 0 is the one a single-threaded measurement runs on; the others create theirs on demand)
        CtxLease lease;
        int rc = ctx_lease(&lease);
        if (rc) return rc;
        DeviceCtx* const c = lease.c;
        constexpr size_t kPool = 4096;
        while (c->ev_free.size() + c->ev_pending.size() < kPool) {
            EventPair ep{};
            HIP_TRY(hipEventCreate(&ep.start));
            HIP_TRY(hipEventCreate(&ep.stop));
            c->ev_free.push_back(ep);
        }
    }
    return OLMC_OK;
}

extern "C" int olmc_profile_reset(void) {
    return with_all_contexts([](DeviceCtx* c) {
        const int rc = prof_drain(c);
        c->prof_launches = 0;
        c->prof_ms = 0.0;
        return rc;
    });
}

extern "C" int olmc_kernel_time(int64_t* launches, double* total_ms) {
    if (!launches || !total_ms) return fail(OLMC_ERR_ARG, "null pointer");
    int64_t n = 0;
    double ms = 0.0;
    const int rc = with_all_contexts([&](DeviceCtx* c) {
        const int r = prof_drain(c);
        n += c->prof_launches;
        ms += c->prof_ms;
        return r;
    });
    if (rc) return rc;
    *launches = n;
    *total_ms = ms;
    return OLMC_OK;
}
