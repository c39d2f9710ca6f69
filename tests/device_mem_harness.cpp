// device_mem_harness.cpp -- optionslab_amd/csrc/olmc_device_mem.h on its own, under g++ -fsanitize=address,undefined
// (tests/test_device_mem_sanitizers.py builds and runs it; it needs no GPU and no HIP).
//
// The header is instantiated with a RECORDING backend: "device" and "pinned" memory are malloc blocks (so AddressSanitizer sees
// every use after free, double free, overrun and leak), asynchronous copies and memsets are DEFERRED until the stream is waited
// for or "a kernel runs" (so a copy whose source did not live long enough is a sanitizer report), every call is counted, and the
// k-th call fails on request.  A block is `dirty` from the moment something queued may touch it until the stream has been waited
// for: freeing a dirty block is the bug "free without quiesce".
//
// `self` runs random sequences of requests against one object of every type, fault-free first and then once for every k up to the
// number of backend calls the fault-free run made, the k-th call failing.
#include "olmc_device_mem.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>

namespace {

#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s (seed %u, fail_at %ld, op %d)\n", __FILE__, __LINE__, #cond, g_seed, Rec::fail_at, g_op); \
            std::exit(1);                                                                    \
        }                                                                                    \
    } while (0)

unsigned g_seed = 0;
int g_op = 0;
long g_checks = 0;
constexpr int kInjected = 77;

struct Rec {
    using Stream = int;
    struct Info { size_t bytes; bool pinned, dirty; };
    struct Pending { void* d; const void* h; size_t bytes; };       // h == nullptr: memset to zero
    static std::map<void*, Info> live;
    static std::vector<Pending> queue;
    static long calls, fail_at, allocs, uploads, waits;

    static bool injected() { return ++calls == fail_at; }
    static Info* find(void* p, size_t bytes) {                      // the live block that holds [p, p + bytes)
        auto it = live.upper_bound(p);
        if (it == live.begin()) return nullptr;
        --it;
        char* base = static_cast<char*>(it->first);
        return static_cast<char*>(p) + bytes <= base + it->second.bytes ? &it->second : nullptr;
    }
    static int make(void** p, size_t bytes, bool pinned) {
        if (injected()) return kInjected;
        ++allocs;
        *p = std::malloc(bytes);
        std::memset(*p, 0xAB, bytes);                               // fresh memory is not zero
        live[*p] = Info{bytes, pinned, false};
        return 0;
    }
    static int drop(void* p, bool pinned);
    static int alloc(void** p, size_t bytes) { return make(p, bytes, false); }
    static int free(void* p) { return drop(p, false); }
    static int alloc_pinned(void** p, size_t bytes, bool) { return make(p, bytes, true); }
    static int free_pinned(void* p) { return drop(p, true); }
    static int device_alias(void** d, void* h) {
        if (injected()) return kInjected;
        *d = h;
        return 0;
    }
    static int enqueue(void* d, const void* h, size_t bytes);
    static int upload(void* d, const void* h, size_t bytes, Stream) { ++uploads; return enqueue(d, h, bytes); }
    static int zero(void* d, size_t bytes, Stream) { return enqueue(d, nullptr, bytes); }
    static void run_queue() {                                       // the device gets to the queued work
        for (const Pending& q : queue) {
            if (q.h) std::memcpy(q.d, q.h, q.bytes);
            else std::memset(q.d, 0, q.bytes);
        }
        queue.clear();
    }
    static int wait(Stream) {
        if (injected()) return kInjected;
        ++waits;
        run_queue();
        for (auto& kv : live) kv.second.dirty = false;
        return 0;
    }
    // a kernel queued on the stream reads or writes the block that holds p
    static void use(void* p) {
        run_queue();
        Info* i = find(p, 1);
        if (!i) { std::fprintf(stderr, "use of a pointer no live block holds\n"); std::exit(1); }
        i->dirty = true;
    }
};
std::map<void*, Rec::Info> Rec::live;
std::vector<Rec::Pending> Rec::queue;
long Rec::calls = 0, Rec::fail_at = -1, Rec::allocs = 0, Rec::uploads = 0, Rec::waits = 0;

int Rec::drop(void* p, bool pinned) {
    const bool fails = injected();
    auto it = live.find(p);
    CHECK(it != live.end());                                        // not a double free, not a pointer nobody allocated
    CHECK(it->second.pinned == pinned);
    CHECK(!it->second.dirty);                                       // no free without a quiesce since the last use
    for (const Pending& q : queue) CHECK(!(static_cast<char*>(q.d) >= static_cast<char*>(p) && static_cast<char*>(q.d) < static_cast<char*>(p) + it->second.bytes));
    live.erase(it);
    std::free(p);                                                   // a failing free has let go of the memory all the same
    return fails ? kInjected : 0;
}

int Rec::enqueue(void* d, const void* h, size_t bytes) {
    if (injected()) return kInjected;
    Info* i = find(d, bytes);
    CHECK(i != nullptr);                                            // inside one live block
    i->dirty = true;
    queue.push_back(Pending{d, h, bytes});
    return 0;
}

struct Opt { double a, vol, strike, sign; uint32_t tag, pad; };     // the size and alignment of the kernels' MultiOption
constexpr size_t kStride = 16;
using Batch = olmc::BatchWorkspace<Rec, Opt, kStride>;

struct World {
    olmc::DeviceBlock<Rec> dev;
    olmc::PinnedBlock<Rec> pin;
    olmc::CachedUpload<Rec> content, keyed, always;
    Batch batch;
    std::vector<unsigned char> content_last;                        // the content request the block holds (empty: none)
    bool keyed_held = false;                                        // the keyed cache holds the plan of ...
    size_t keyed_key = 0, keyed_bytes = 0;                          // ... this key and size
};

auto quiesce = [] { return Rec::wait(0); };

std::vector<unsigned char> random_bytes(std::mt19937& rng, size_t n) {
    std::vector<unsigned char> v(n);
    for (auto& b : v) b = static_cast<unsigned char>(rng());
    return v;
}

// the plan of key n: what the builder writes, and what the block must hold afterwards
void build_plan(int64_t key, unsigned char* m, size_t bytes) {
    for (size_t i = 0; i < bytes; ++i) m[i] = static_cast<unsigned char>(key * 31 + i * 7);
}

bool holds(const void* device, const std::vector<unsigned char>& want) {
    Rec::run_queue();
    return std::memcmp(device, want.data(), want.size()) == 0;
}

struct Op {
    int kind;
    size_t a, b;
    std::vector<unsigned char> bytes;
};

// One request against the world.  Returns the backend's status; on success every property of the request has been checked.
int apply(World& w, const Op& op, bool expect_upload) {
    const long calls0 = Rec::calls, allocs0 = Rec::allocs, uploads0 = Rec::uploads, waits0 = Rec::waits;
    switch (op.kind) {
        case 0: case 1: {                                           // reserve: device / pinned + mapped (grow, shrink, equal)
            const size_t before = op.kind == 0 ? w.dev.capacity() : w.pin.capacity();
            const int e = op.kind == 0 ? w.dev.reserve(op.a, quiesce, 64, op.b) : w.pin.reserve(op.a, quiesce, 0, 0, true);
            void* p = op.kind == 0 ? w.dev.get() : w.pin.get();
            const size_t cap = op.kind == 0 ? w.dev.capacity() : w.pin.capacity();
            CHECK((p == nullptr) == (cap == 0));                    // whole or empty, never dangling
            if (e) return e;
            CHECK(cap >= op.a);
            if (op.a <= before) CHECK(Rec::calls == calls0 && cap == before);
            else if (op.kind == 0) CHECK(cap == std::max(op.a, std::max<size_t>(64, op.b * before)));
            if (op.kind == 1) CHECK(w.pin.alias<void>() == p);
            std::memset(p, 0x5A, cap);                              // every byte is there to write
            if (op.kind == 0) {                                     // carved: consecutive, aligned, inside the block (the sanitizer watches the writes)
                olmc::Carver spans = w.dev.carve();
                const size_t n32 = 1 + op.a % 3, n64 = (cap - 16) / 16, n8 = cap - 16 - 8 * n64;
                uint32_t* a = spans.take<uint32_t>(n32);
                double* b = spans.take<double>(n64);
                char* c = spans.take<char>(n8);
                CHECK(static_cast<void*>(a) == p && reinterpret_cast<char*>(b) == static_cast<char*>(p) + (4 * n32 + 7) / 8 * 8);
                CHECK(c == reinterpret_cast<char*>(b + n64) && c + n8 <= static_cast<char*>(p) + cap);
                for (size_t i = 0; i < n32; ++i) a[i] = 1;
                for (size_t i = 0; i < n64; ++i) b[i] = 2.0;
                std::memset(c, 3, n8);
            }
            Rec::use(p);
            return 0;
        }
        case 2: {                                                   // content-keyed put
            const bool hit_expected = !expect_upload && op.bytes == w.content_last && !w.content_last.empty();
            const bool equal_size = op.bytes.size() == w.content_last.size() && w.content.device<void>() != nullptr;
            int e;
            {
                std::vector<unsigned char> callers = op.bytes;      // the caller's arrays die with the call
                e = w.content.put(callers.data(), op.a, callers.data() + op.a, callers.size() - op.a, 0, quiesce);
            }
            if (e) { w.content_last.clear(); return e; }
            if (hit_expected) CHECK(Rec::calls == calls0);          // a hit issues no backend call at all
            else CHECK(Rec::uploads == uploads0 + 1);
            if (equal_size) CHECK(Rec::allocs == allocs0);          // a miss of equal size issues no allocation
            if (expect_upload) CHECK(Rec::uploads == uploads0 + 1);
            CHECK(holds(w.content.device<void>(), op.bytes));
            w.content_last = op.bytes;
            Rec::use(const_cast<void*>(w.content.device<void>()));
            return 0;
        }
        case 3: {                                                   // key-keyed ensure: the builder runs only on a miss
            const bool hit_expected = !expect_upload && w.keyed_held && w.keyed_key == op.a && w.keyed_bytes == op.b;
            const bool held = w.keyed_held;
            w.keyed_held = false;
            int built = 0;
            const int e = w.keyed.ensure(static_cast<int64_t>(op.a), op.b, 0, quiesce, [&](unsigned char* m) {
                ++built;
                for (size_t i = 0; i < op.b; ++i) CHECK(m[i] == 0);
                build_plan(static_cast<int64_t>(op.a), m, op.b);
                return 0;
            });
            if (e) return e;
            if (hit_expected) CHECK(built == 0 && Rec::calls == calls0);      // the same key hits: no builder, no backend call at all
            else CHECK(built == 1 && Rec::uploads == uploads0 + 1);           // another key, even at the same size, or nothing held: rebuilt
            if (!hit_expected && held && !expect_upload) CHECK(Rec::waits > waits0);          // the stream was waited for before the mirror was rewritten
            w.keyed_held = true; w.keyed_key = op.a; w.keyed_bytes = op.b;
            std::vector<unsigned char> want(op.b);
            build_plan(static_cast<int64_t>(op.a), want.data(), op.b);
            CHECK(holds(w.keyed.device<void>(), want));
            Rec::use(const_cast<void*>(w.keyed.device<void>()));
            return 0;
        }
        case 4: {                                                   // always upload, into a block sized once
            const int e = w.always.upload(op.bytes.size(), 0, quiesce, [&](unsigned char* m) { std::memcpy(m, op.bytes.data(), op.bytes.size()); return 0; }, 512);
            if (e) return e;
            CHECK(Rec::uploads == uploads0 + 1);
            CHECK(holds(w.always.device<void>(), op.bytes));
            Rec::use(const_cast<void*>(w.always.device<void>()));
            return 0;
        }
        case 5: {                                                   // batch workspace: more contracts, wider rows, both, neither
            const size_t n = op.a, bpo = op.b, cap0 = w.batch.capacity(), bpo0 = w.batch.rows_per_contract();
            Batch::Views v{};
            const int e = w.batch.reserve(n, bpo, 0, &v);
            if (e) { CHECK(w.batch.capacity() == 0 && w.batch.counters() == nullptr); return e; }
            const size_t cap = w.batch.capacity(), rows = w.batch.rows_per_contract();
            CHECK(cap >= n && rows >= bpo);
            if (n <= cap0 && bpo <= bpo0) CHECK(Rec::calls == calls0 && cap == cap0 && rows == bpo0);
            else if (cap0) CHECK(cap == (n > cap0 ? std::max(n, std::max<size_t>(2 * cap0, 64)) : cap0) && rows == std::max(bpo, bpo0));
            // the views: inside their blocks (the sanitizer watches every write below), in this order, never overlapping
            char* cnt = reinterpret_cast<char*>(v.d_cnt);
            CHECK(cnt == w.batch.counters());
            CHECK(cnt + sizeof(uint32_t) * cap * kStride <= reinterpret_cast<char*>(v.d_done));
            CHECK(reinterpret_cast<char*>(v.d_done + 1) <= reinterpret_cast<char*>(v.d_opts));
            CHECK(reinterpret_cast<char*>(v.d_opts) == cnt + w.batch.counter_bytes());
            CHECK(reinterpret_cast<char*>(v.d_opts + cap) <= reinterpret_cast<char*>(v.d_rows));
            CHECK(Rec::find(v.d_rows, sizeof(double) * 2 * rows * cap) == Rec::find(cnt, 1));
            CHECK(reinterpret_cast<const char*>(v.h_opts + cap) <= reinterpret_cast<const char*>(v.h_out));
            CHECK(Rec::find(const_cast<double*>(v.h_out), sizeof(double) * 2 * cap) == Rec::find(v.h_opts, 1));
            CHECK(reinterpret_cast<const double*>(v.d_out) == v.h_out);
            Rec::run_queue();
            for (size_t i = 0; i < w.batch.counter_bytes(); ++i) CHECK(cnt[i] == 0);      // zero after every reallocation -- and ever after
            for (size_t j = 0; j < n; ++j) v.h_opts[j] = Opt{1, 2, 3, 4, static_cast<uint32_t>(j), 0};
            Rec::use(v.d_cnt);                                      // the launch: contracts up, rows and sums written, counters re-zeroed
            Rec::use(v.h_opts);
            std::memset(v.d_opts, 0x11, sizeof(Opt) * n);
            std::memset(v.d_rows, 0x22, sizeof(double) * 2 * bpo * n);
            std::memset(v.d_out, 0x33, sizeof(double) * 2 * n);
            return 0;
        }
        case 6: {                                                   // move: there and back, through construction and assignment
            World other;
            other.dev = std::move(w.dev);
            CHECK(w.dev.get() == nullptr && w.dev.capacity() == 0);
            olmc::PinnedBlock<Rec> pin(std::move(w.pin));
            olmc::CachedUpload<Rec> content(std::move(w.content));
            Batch batch(std::move(w.batch));
            w.batch = std::move(batch);
            w.content = std::move(content);
            w.pin = std::move(pin);
            w.dev = std::move(other.dev);
            CHECK(Rec::calls == calls0);
            return 0;
        }
        default: {                                                  // destroy: once the stream has drained, as ctx_release does
            const int e = Rec::wait(0);
            if (e) return e;
            const size_t blocks = Rec::live.size();
            if (op.a == 0) w.dev = olmc::DeviceBlock<Rec>();
            else if (op.a == 1) { w.content = olmc::CachedUpload<Rec>(); w.content_last.clear(); }
            else if (op.a == 2) w.batch = Batch();
            else { w.keyed = olmc::CachedUpload<Rec>(); w.keyed_held = false; }
            CHECK(Rec::live.size() <= blocks);
            return 0;
        }
    }
}

std::vector<Op> make_ops(unsigned seed, int count) {
    std::mt19937 rng(seed);
    std::vector<Op> ops;
    std::vector<unsigned char> last = random_bytes(rng, 124);
    size_t n = 10, bpo = 2;
    for (int i = 0; i < count; ++i) {
        Op op{static_cast<int>(rng() % 8), 0, 0, {}};
        const unsigned how = rng() % 4;
        switch (op.kind) {
            case 0: case 1: op.a = 1 + rng() % 4096; op.b = rng() % 3; break;
            case 2:
                if (how == 1) last = random_bytes(rng, last.size());                       // same size, other words
                else if (how == 2) last = random_bytes(rng, last.size() + 31 * (1 + rng() % 8));     // larger
                else if (how == 3) last = random_bytes(rng, std::max<size_t>(31, last.size() / 2));  // smaller
                op.bytes = last;
                op.a = last.size() / 31 * 30;                       // [dims x 30 | dims] words' worth of split
                break;
            case 3: op.a = 1 + rng() % 4; op.b = 32 * std::min<size_t>(op.a, 3) + 8; break;   // same key, other key; keys 3 and 4 share a size
            case 4: op.bytes = random_bytes(rng, 4 * (1 + rng() % 128)); break;
            case 5:
                if (how & 1) n = n + 1 + rng() % 200;                                      // more contracts
                else if (rng() % 3 == 0) n = 1 + rng() % n;                                // fewer
                if (how & 2) bpo = bpo + 1 + rng() % 5;                                    // wider rows
                op.a = n; op.b = bpo;
                break;
            case 6: break;
            default: op.a = rng() % 4; break;
        }
        ops.push_back(std::move(op));
    }
    return ops;
}

// The sequence of `seed` with the fail_at-th backend call failing (-1: none).  Returns the number of backend calls made.
long run(unsigned seed, long fail_at, int count) {
    g_seed = seed;
    Rec::calls = 0;
    Rec::fail_at = fail_at;
    const std::vector<Op> ops = make_ops(seed, count);
    {
        World w;
        for (g_op = 0; g_op < count; ++g_op) {
            const Op& op = ops[g_op];
            int e = apply(w, op, false);
            if (e) {
                CHECK(e == kInjected && Rec::calls >= fail_at);     // the backend's status comes back untouched
                Rec::run_queue();                                   // time passes
                // the next identical request does the work again and answers as a fresh object does
                e = apply(w, op, op.kind >= 2 && op.kind <= 4);
                CHECK(e == 0);
            }
            ++g_checks;
        }
        if (Rec::wait(0) != 0) CHECK(Rec::wait(0) == 0);          // ctx_release: the stream drains, then the owners go
    }
    CHECK(Rec::live.empty());                                       // every owner freed what it held
    Rec::run_queue();
    return Rec::calls;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2 || std::strcmp(argv[1], "self") != 0) {
        std::fprintf(stderr, "usage: %s self [seeds] [ops per sequence]\n", argv[0]);
        return 2;
    }
    const unsigned seeds = argc > 2 ? static_cast<unsigned>(std::atoi(argv[2])) : 40;
    const int count = argc > 3 ? std::atoi(argv[3]) : 48;
    long runs = 0;
    for (unsigned seed = 1; seed <= seeds; ++seed) {
        const long calls = run(seed, -1, count);
        for (long k = 1; k <= calls; ++k) { run(seed, k, count); ++runs; }
    }
    std::printf("ok %ld requests checked in %ld faulted runs\n", g_checks, runs);
    return 0;
}
