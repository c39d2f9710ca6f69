// olmc_device_mem.h -- who owns a context's device and pinned memory, and what a buffer kept between calls may be trusted to hold.
// Plain C++17 over a small backend, no HIP needed: olmc.hip instantiates it with HipMem (below, the ONE place that names the
// allocation calls), tests/device_mem_harness.cpp compiles it on its own with g++ -fsanitize=address,undefined over a recording
// backend that fails the k-th call on request.
//
// A backend B provides, every function returning 0 or the caller's error status (passed through untouched):
//   B::Stream
//   alloc(void** p, bytes), free(p)                          device memory
//   alloc_pinned(void** p, bytes, mapped), free_pinned(p)    page-locked host memory
//   device_alias(void** d, h)                                the device's address of a mapped pinned block
//   upload(d, h, bytes, stream), zero(d, bytes, stream)      asynchronous, ordered by the stream
//   wait(stream)                                             until everything queued on the stream has finished
//
// The one rule of a buffer that grows: let the old users finish (`quiesce`, a callable: wait for a stream, for an event), free,
// FORGET pointer and capacity, allocate, remember.  A failure at any step leaves the owner empty, never dangling.
#ifndef OLMC_DEVICE_MEM_H
#define OLMC_DEVICE_MEM_H

#include <algorithm>
#include <cassert>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

namespace olmc {

// The capacity a buffer holding `have` takes when `need` no longer fits: never below `floor`, at least `factor` times what it had.
inline size_t grown(size_t need, size_t have, size_t floor, size_t factor) { return std::max(need, std::max(floor, factor * have)); }

// Consecutive typed arrays cut from one block: take<T>(n) is the next n T's.  The block was reserved for their sum.
class Carver {
    char* base_;
    size_t size_, off_ = 0;
public:
    Carver(void* base = nullptr, size_t size = 0) : base_(static_cast<char*>(base)), size_(size) {}
    template <typename T>
    T* take(size_t n) {
        off_ = (off_ + alignof(T) - 1) / alignof(T) * alignof(T);
        assert(off_ + n * sizeof(T) <= size_);                  // an invariant of the caller's own arithmetic, not an input check
        T* p = reinterpret_cast<T*>(base_ + off_);
        off_ += n * sizeof(T);
        return p;
    }
};

// Move-only owner of one block: device memory, or pinned host memory (mapped: with its device alias).
template <class B, bool PINNED>
class Block {
    void* p_ = nullptr;
    void* alias_ = nullptr;
    size_t cap_ = 0;
public:
    Block() = default;
    Block(Block&& o) noexcept { swap(o); }
    Block& operator=(Block&& o) noexcept { Block t(std::move(o)); swap(t); return *this; }
    Block(const Block&) = delete;
    Block& operator=(const Block&) = delete;
    ~Block() { (void)reset(); }
    void swap(Block& o) noexcept { std::swap(p_, o.p_); std::swap(alias_, o.alias_); std::swap(cap_, o.cap_); }

    void* get() const { return p_; }
    size_t capacity() const { return cap_; }                    // bytes
    template <typename T> T* as() const { return static_cast<T*>(p_); }
    template <typename T> T* alias() const { return static_cast<T*>(alias_); }      // mapped pinned blocks only
    Carver carve() const { return Carver(p_, cap_); }

    // Frees now.  The caller knows that nothing uses the block any more.
    int reset() {
        void* p = p_;
        p_ = alias_ = nullptr;
        cap_ = 0;
        if (!p) return 0;
        return PINNED ? B::free_pinned(p) : B::free(p);
    }

    // Room for `bytes`: at once when the block is large enough, else the rule above with grown(bytes, capacity, floor, factor).
    template <typename Quiesce>
    int reserve(size_t bytes, Quiesce&& quiesce, size_t floor = 0, size_t factor = 0, bool mapped = false) {
        if (bytes <= cap_) return 0;
        const size_t cap = grown(bytes, cap_, floor, factor);
        if (p_) {
            int e = quiesce();
            if (e) return e;                                    // still whole: nothing was freed
            e = reset();
            if (e) return e;
        }
        void* p = nullptr;
        int e = PINNED ? B::alloc_pinned(&p, cap, mapped) : B::alloc(&p, cap);
        if (e) return e;
        if (PINNED && mapped) {
            e = B::device_alias(&alias_, p);
            if (e) { alias_ = nullptr; (void)B::free_pinned(p); return e; }
        }
        p_ = p;
        cap_ = cap;
        return 0;
    }
};
template <class B> using DeviceBlock = Block<B, false>;
template <class B> using PinnedBlock = Block<B, true>;

// A device block and the host mirror of what it holds.  Invariant: valid_ only if the copy that put the mirror's bytes into the
// block was enqueued without error -- so after ANY failed step the cache describes nothing and the next call uploads again.
// Every upload reads from the mirror, so the caller's arrays need not outlive the call.  The mirror itself is rewritten by the
// next miss: ensure() lets the stream finish first; put() and upload() do not wait, and rely on what the library's blocking
// calls give them (the launch that reads the block has been waited for) and on a copy out of pageable memory having consumed
// its source when the call that enqueues it returns.
template <class B>
class CachedUpload {
    DeviceBlock<B> dev_;
    std::vector<unsigned char> mirror_;
    int64_t key_ = 0;
    bool valid_ = false;

    template <typename Quiesce, typename Fill>
    int refill(size_t bytes, typename B::Stream s, Quiesce&& quiesce, Fill&& fill, size_t floor = 0) {
        valid_ = false;
        mirror_.resize(bytes);
        int e = fill(mirror_.data());
        if (!e) e = dev_.reserve(bytes, quiesce, floor);
        if (!e) e = B::upload(dev_.get(), mirror_.data(), bytes, s);
        valid_ = e == 0;
        return e;
    }
public:
    template <typename T> const T* device() const { return dev_.template as<const T>(); }

    // Keyed by content: the bytes of a, then of b, travel unless they are what the block already holds.
    template <typename Quiesce>
    int put(const void* a, size_t na, const void* b, size_t nb, typename B::Stream s, Quiesce&& quiesce) {
        if (valid_ && mirror_.size() == na + nb && std::memcmp(mirror_.data(), a, na) == 0 && std::memcmp(mirror_.data() + na, b, nb) == 0) return 0;
        return refill(na + nb, s, quiesce, [&](unsigned char* m) { std::memcpy(m, a, na); std::memcpy(m + na, b, nb); return 0; });
    }
    // Keyed by `key`: build(mirror) writes the `bytes` (zero on entry) that belong to it, and runs only on a miss.
    template <typename Quiesce, typename Build>
    int ensure(int64_t key, size_t bytes, typename B::Stream s, Quiesce&& quiesce, Build&& build) {
        if (valid_ && key_ == key && mirror_.size() == bytes) return 0;
        valid_ = false;
        key_ = key;
        if (const int e = dev_.get() ? quiesce() : 0) return e;      // a copy out of the old mirror may still be on its way
        return refill(bytes, s, quiesce, [&](unsigned char* m) { std::memset(m, 0, bytes); return build(m); });
    }
    // Every call uploads what fill(mirror) writes; the block is allocated with room for `floor` bytes.
    template <typename Quiesce, typename Fill>
    int upload(size_t bytes, typename B::Stream s, Quiesce&& quiesce, Fill&& fill, size_t floor = 0) { return refill(bytes, s, quiesce, fill, floor); }
};

// The workspace of a batch of independent contracts (european_multi_kernel).  Device [ticket counters | done counter | contracts |
// rows]: the counters sit FIRST and are sized by the capacity in contracts, so their place does not move with the batch size, and
// they are zeroed once per layout -- every finisher re-zeroes the counter it consumed.  Pinned + mapped host [contracts | sums].
// The two capacities grow independently: more contracts doubles the contract capacity, more workgroups per contract (a larger
// n_paths on the same batch) only widens the rows -- a convergence sweep over n_paths must not double the capacity each time.
template <class B, class Opt, size_t COUNTER_STRIDE>
class BatchWorkspace {
    DeviceBlock<B> dev_;
    PinnedBlock<B> host_;
    size_t cap_ = 0, bpo_ = 0;                      // contracts; workgroups per contract the rows are sized for
    size_t off_done_ = 0, off_opts_ = 0, off_rows_ = 0, hoff_out_ = 0;
    static size_t align(size_t b) { return (b + 255) / 256 * 256; }
public:
    struct Views {
        uint32_t *d_cnt, *d_done;
        Opt* d_opts;
        double* d_rows;
        Opt* h_opts;
        const double* h_out;
        double* d_out;                              // the device's address of h_out
    };
    size_t capacity() const { return cap_; }
    size_t rows_per_contract() const { return bpo_; }
    void* counters() const { return cap_ ? dev_.get() : nullptr; }      // what a failed launch may have left dirty ...
    size_t counter_bytes() const { return off_opts_; }                  // ... ticket counters and done counter

    int reserve(size_t n_options, size_t bpo, typename B::Stream s, Views* v) {
        if (n_options > cap_ || bpo > bpo_) {
            const size_t cap = n_options > cap_ ? grown(n_options, cap_, 64, 2) : cap_, bpo_cap = std::max(bpo, bpo_);
            const size_t b_cnt = align(sizeof(uint32_t) * cap * COUNTER_STRIDE), b_done = 256, b_opts = align(sizeof(Opt) * cap);
            const size_t b_rows = align(sizeof(double) * 2 * bpo_cap * cap);
            cap_ = bpo_ = 0;                        // until the new layout stands, counters zeroed
            bool waited = false;                    // one wait lets the users of both blocks finish
            auto quiesce = [&] { const int e = waited ? 0 : B::wait(s); waited = true; return e; };
            int e = dev_.reserve(b_cnt + b_done + b_opts + b_rows, quiesce);
            if (!e) e = host_.reserve(b_opts + align(sizeof(double) * 2 * cap), quiesce, 0, 0, true);
            if (!e) e = B::zero(dev_.get(), b_cnt + b_done, s);
            if (e) return e;
            off_done_ = b_cnt; off_opts_ = b_cnt + b_done; off_rows_ = off_opts_ + b_opts; hoff_out_ = b_opts;
            cap_ = cap;
            bpo_ = bpo_cap;
        }
        char* d = dev_.template as<char>();
        v->d_cnt = reinterpret_cast<uint32_t*>(d);
        v->d_done = reinterpret_cast<uint32_t*>(d + off_done_);
        v->d_opts = reinterpret_cast<Opt*>(d + off_opts_);
        v->d_rows = reinterpret_cast<double*>(d + off_rows_);
        v->h_opts = host_.template as<Opt>();
        v->h_out = reinterpret_cast<const double*>(host_.template as<char>() + hoff_out_);
        v->d_out = reinterpret_cast<double*>(host_.template alias<char>() + hoff_out_);
        return 0;
    }
};

}  // namespace olmc

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace olmc {

// The status and message of a failed HIP call: defined by the translation unit that instantiates HipMem.
int device_mem_fail(hipError_t e, const char* call);

struct HipMem {
    using Stream = hipStream_t;
    static int status(hipError_t e, const char* call) { return e == hipSuccess ? 0 : device_mem_fail(e, call); }
    static int alloc(void** p, size_t bytes) { return status(hipMalloc(p, bytes), "hipMalloc"); }
    static int free(void* p) { return status(hipFree(p), "hipFree"); }
    static int alloc_pinned(void** p, size_t bytes, bool mapped) {
        return status(hipHostMalloc(p, bytes, mapped ? hipHostMallocMapped : hipHostMallocDefault), "hipHostMalloc");
    }
    static int free_pinned(void* p) { return status(hipHostFree(p), "hipHostFree"); }
    static int device_alias(void** d, void* h) { return status(hipHostGetDevicePointer(d, h, 0), "hipHostGetDevicePointer"); }
    static int upload(void* d, const void* h, size_t bytes, Stream s) { return status(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s), "hipMemcpyAsync"); }
    static int zero(void* d, size_t bytes, Stream s) { return status(hipMemsetAsync(d, 0, bytes, s), "hipMemsetAsync"); }
    static int wait(Stream s) { return status(hipStreamSynchronize(s), "hipStreamSynchronize"); }
};

}  // namespace olmc
#endif  // __HIPCC__

#endif  // OLMC_DEVICE_MEM_H
