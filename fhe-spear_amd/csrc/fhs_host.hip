// fhs_host.hip -- host side of libfhespear_hip.so: object lifetime, key generation, CKKS
// encode/decode, and every extern "C" entry point of include/fhespear.h.  The parameter tables and
// everything else that needs no device (number theory, argument validation, CRT constants) are
// derived in fhs_tables.h; this file uploads them.
//
// Runtime model (MI355X-first):
//  - one context = one device + one HIP stream; device blocks come from hipMalloc behind a bounded
//    per-size caching free list reused in stream order, so a free never synchronises the host;
//  - calls on a context are serialised by a mutex (ctypes drops the GIL; bg:223-249 may call
//    from a thread pool);
//  - rotations are DEFERRED and batched: fhs_rotate allocates the output and queues the
//    key-switch; the queue is flushed as one batched key-switch by the next operation that is
//    not a rotation at the same level.  The reference's baby-step loop (bg:215-220) issues G-1
//    independent rotations back to back; batching turns 39 workgroups per rotation into
//    39 (G-1) workgroups per launch.  Each rotation is computed exactly as it would be alone.
#include <execinfo.h>
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <algorithm>
#include <csignal>
#include <atomic>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <map>
#include <unordered_map>
#include <chrono>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "../../include/fhespear.h"
#include "fhs_kernels.h"
#include "fhs_modarith.h"
#include "fhs_tables.h"

using fhs::DevTables;
using fhs::KsItem;

// ============================================================================ errors
static thread_local std::string g_err;
static fhs_status fail(fhs_status code, const std::string& msg) {
    g_err = msg;
    return code;
}
// FHESPEAR_SEGV_TRACE=1: print a native backtrace on SIGSEGV (diagnostics for faults outside
// Python frames, e.g. during process teardown, where faulthandler is no longer installed)
static void segv_trace(int sig) {
    void* fr[64];
    const int n = backtrace(fr, 64);
    static const char hdr[] = "[fhespear] native backtrace:\n";
    (void)!write(2, hdr, sizeof(hdr) - 1);
    backtrace_symbols_fd(fr, n, 2);
    signal(sig, SIG_DFL);
    raise(sig);
}
__attribute__((constructor)) static void segv_trace_install() {
    if (getenv("FHESPEAR_SEGV_TRACE")) signal(SIGSEGV, segv_trace);
}
static fhs_status hip_fail(hipError_t e, const char* where) {
    if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation)
        return fail(FHS_ERR_OOM, std::string("HIP out of memory in ") + where);
    return fail(FHS_ERR_HIP, std::string("HIP error in ") + where + ": " + hipGetErrorString(e));
}
#define HIPCHK(expr, where)                                  \
    do {                                                     \
        hipError_t _e = (expr);                              \
        if (_e != hipSuccess) return hip_fail(_e, where);    \
    } while (0)

extern "C" const char* fhs_last_error(void) { return g_err.c_str(); }
extern "C" const char* fhs_version(void) { return "fhespear-mi355x 0.1 (gfx950)"; }
extern "C" int fhs_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
extern "C" fhs_status fhs_device_pci_bus_id(int device, char* buf, int len) {
    if (!buf || len < 13) return fail(FHS_ERR_INVALID, "device_pci_bus_id: buffer of at least 13 bytes");
    hipError_t e = hipDeviceGetPCIBusId(buf, len, device);
    if (e != hipSuccess) return hip_fail(e, "device_pci_bus_id");
    return FHS_OK;
}

// ============================================================================ pure helpers (fhs_tables.h)
extern "C" fhs_status fhs_create_coeff_modulus(uint64_t N, const int* bits, int n, uint64_t* out) {
    if (!bits || !out || n <= 0 || N < 2 || (N & (N - 1))) return fail(FHS_ERR_INVALID, "create_coeff_modulus: bad args");
    for (int i = 0; i < n; ++i)
        if (bits[i] < 2 || bits[i] > 61) return fail(FHS_ERR_INVALID, "create_coeff_modulus: bit size must be in [2, 61]");
    if (!coeff_modulus_search(N, bits, n, out)) return fail(FHS_ERR_INVALID, "create_coeff_modulus: not enough primes");
    return FHS_OK;
}
extern "C" uint64_t fhs_galois_elt_from_step(int step, uint64_t N) { return galois_elt_from_step(step, N); }

// ============================================================================ objects
struct PendingRot {
    KsItem item;
    fhs_ciphertext* out;
    const fhs_ciphertext* in;
};

struct fhs_context {
    int device = 0;
    hipStream_t st = nullptr;
    // side stream of the giant steps with its fork / join events (fhs_kernels.h KsSide): created with `st`, joined
    // back into `st` before every launcher returns, so everything else sees one stream
    fhs::KsSide side{};
    std::recursive_mutex mu;
    uint64_t N = 0;
    int logN = 0, L0 = 0, P = 0, K = 0, dnum = 0;
    std::vector<uint64_t> q;
    std::vector<uint64_t> elts;
    DevTables T{};
    std::vector<void*> tables;     // device allocations owned by the context
    void* items_dev = nullptr;     // KsItem[kMaxItems]
    void* ptrs_dev = nullptr;      // pointer arrays for BSGS (2 x kMaxPtrs)
    std::vector<PendingRot> pending;
    int pending_l = -1;
    std::set<const void*> pending_refs;   // inputs and outputs of queued rotations (destroy must flush)
    std::set<const void*> pending_outs;   // outputs of queued rotations (a consumer must flush)
    int debug_fail_flushes = 0;           // fhs_debug_fail_next_flushes (testing hook)
    int debug_fail_alloc = -1;            // fhs_debug_fail_alloc (testing hook): dalloc calls left before the failure
    std::vector<std::complex<double>> fft_w;   // exp(2 pi i k / N), k < N
    std::vector<std::complex<double>> dec_twist;   // (cos, sin)(pi k / N), k < N
    std::vector<uint64_t> slot_index;          // (5^j mod 2N - 1)/2, j < N/2
    std::atomic<uint64_t> bytes_live{0};
    // lifetime: the caller's reference + one per live object (ciphertext, plaintext, key), so objects
    // may be destroyed after fhs_context_destroy (Python finalisation order is arbitrary)
    std::atomic<int> refs{1};
    // caching allocator: freed device blocks are kept per exact size and reused in stream order
    // (every use of a block is ordered on `st`, aux-stream work is joined back into `st`).  A large
    // device allocation costs host time per GB and a free synchronises (tools/microbench/
    // alloc.hip); ciphertexts and plaintexts come in a handful of sizes, so almost every allocation
    // after warm-up is a free-list pop.  Trimmed on out-of-memory, at context destruction and exit.
    std::unordered_map<size_t, std::vector<void*>> free_blocks;
    // imported switching keys (fhs_*_keys_import): key -> its explicit a_j [dnum][K][N]
    std::unordered_map<const void*, uint64_t*> key_a;
    size_t cached_bytes = 0;
    // bounded: a chain walks down the levels, so every level brings new sizes and the sizes of the
    // levels behind it go cold.  Over the cap, whole sizes are evicted least-recently-used first
    // (a 13-block d=2048 chain otherwise parked 135 GB here).  FHESPEAR_CACHE_BYTES overrides.
    size_t cache_cap = 0;
    uint64_t cache_tick = 0;
    std::unordered_map<size_t, uint64_t> size_tick;   // last dalloc/dfree of each size
    // fhs_debug_alloc_stats (testing hook): blocks evict_cold returned to the device, dalloc_fit calls that took a
    // larger cached block, and the times seal_prepare emptied a non-empty correction cache because of its cap
    uint64_t evicted_blocks = 0, fit_hits = 0, seal_corr_drops = 0;
    // kernel timer (bench): events around the timed kernel launches
    // per-kernel event timer (fhs_kernel_timer): bitmask of fhs::KernelId, completed pairs per id
    uint32_t timer_mask = 0;
    std::vector<hipEvent_t> timer_open;                              // begin event per id
    std::vector<std::vector<std::pair<hipEvent_t, hipEvent_t>>> timer_pairs;
    fhs::KTimer ktimer{};
    // pinned staging ring for launch descriptors (stage_h2d): kRingSegs segments; leaving a segment
    // records an event, re-entering it waits for that event (recorded a whole ring earlier)
    unsigned char* ring = nullptr;
    size_t ring_head = 0;          // next free byte; always inside segment ring_seg (or at its end)
    int ring_seg = 0;
    static constexpr size_t kRingBytes = 16u << 20;
    static constexpr int kRingSegs = 8;
    static constexpr size_t kSegBytes = kRingBytes / kRingSegs;
    hipEvent_t ring_ev[kRingSegs] = {};
    uint64_t ring_waits = 0, ring_blocked = 0;   // segment re-entries; of those, the ones that had to wait
    fhs::Stager stager{};
    std::map<std::pair<int, int>, std::vector<uint64_t>> crt_cache;   // decoder tables per (kk, l) (crt_tables)
    // pinned, grow-only: the decoder's slots (and flags) come back through it
    double* readback = nullptr;
    size_t readback_bytes = 0;
    // grow-only scratch buffers reused across calls (stream order makes reuse safe): a large
    // allocation costs host time per GB
    // SEAL-convention hoisting (fhs_kernels.h SealHoist): the per-(key, level) corrections [2][l+P][N],
    // the zero flag (device word + pinned host word) and the counts of hoisted / fallback flushes
    std::map<std::pair<const uint64_t*, int>, uint64_t*> seal_corr;
    size_t seal_corr_bytes = 0;
    size_t seal_corr_cap = 0;     // bound on seal_corr_bytes (1/16 of the context's device; FHESPEAR_SEAL_CORR_BYTES)
    fhs::SealHoist seal_hoist{};
    enum { SCR_KS, SCR_BSGS_INNER, SCR_BSGS_WS, SCR_BSGS_SUM, SCR_RESCALE, SCR_ENC_PTRS, SCR_COUNT };
    uint64_t* scr[SCR_COUNT] = {};
    size_t scr_bytes[SCR_COUNT] = {};
    static constexpr int kMaxItems = kKsMaxItems;
    static constexpr int kMaxPtrs = kStagedMaxPtrs;
};

struct fhs_ciphertext {
    fhs_context* ctx;
    uint64_t* d;
    int ncomp, ci, l;
    double scale;
    // the queued rotation that was to produce it could not run (flush failed, e.g. out of memory): its limbs are
    // undefined and every later use fails (drop_pending)
    bool lost = false;
    struct PtSlab* slab = nullptr;   // non-null: d points into a batch's shared block (new_cts)
};
// One device block shared by the plaintexts of a batch (new_pts): a block per plaintext cost a hipMalloc per
// diagonal and, once a chain walking down the levels pushed the cache over its cap, thousands of hipFree's
// (round-5 cfg5 leg: 0.5-4.7 s per FFN block instead of ~0.2).  Freed when its last plaintext is destroyed.
struct PtSlab {
    uint64_t* base;
    size_t bytes;
    int refs;
};
struct fhs_plaintext {
    fhs_context* ctx;
    uint64_t* d;
    int ci, l;
    double scale;
    PtSlab* slab = nullptr;   // non-null: d points into a batch's shared block
    // compact shadow of a periodic plaintext (encode_rows_dev): word e >> tlog of each limb (N >> tlog words)
    // equals dense word e; read by the fused BSGS's Hadamard only (2^-tlog of the diagonal bytes).  Plaintexts
    // are immutable, so the two never diverge; every other op reads d.
    uint64_t* dc = nullptr;
    int tlog = 0;
    PtSlab* cslab = nullptr;
};
struct fhs_secret_key {
    fhs_context* ctx;
    uint64_t* s;   // K limbs, NTT
    PrfKey key;    // 256-bit PRF key all secret randomness is drawn from
    uint64_t ctr;  // symmetric-encryption counter
    uint64_t pk_gen = 0;   // public keys generated so far (each gets its own mask stream)
};
struct fhs_public_key {
    fhs_context* ctx;
    uint64_t* pk;  // 2 x L0
    PrfKey rng;    // encryption-mask key: a PRF output of the secret key (reveals nothing about it)
    uint64_t ctr;
};
struct fhs_relin_key {
    fhs_context* ctx;
    uint64_t* key;
};
struct fhs_galois_keys {
    fhs_context* ctx;
    std::map<uint64_t, uint64_t*> keys;
};

static void ctx_retain(fhs_context* c) { c->refs.fetch_add(1); }

// Live contexts, for the out-of-memory path (every context's cached blocks on the device are
// released before the retry) and for the process-exit release.  Device blocks come from plain
// hipMalloc behind the per-size cache: round 1 used stream-ordered pools with an infinite release
// threshold, and a process exiting with a multi-GB pool still mapped crashed inside libamdhip64's
// exit handler (a 13-block d=2048 FFN chain with 135 GB cached), and a pool that had been driven to
// out-of-memory left the next process exit crashing too.  release_at_exit is registered with atexit()
// after the first context's stream exists (i.e. after HIP registered its own handlers), so it runs
// first and returns every cached block.
static std::mutex g_live_mu;
static std::set<fhs_context*> g_live;
static void trim_cache(fhs_context* c);
static void release_at_exit() {
    // try_lock, as trim_other_caches: a thread still inside a context (holding c->mu, possibly about
    // to take g_live_mu on its out-of-memory path) keeps that context's cache rather than deadlock exit
    std::lock_guard<std::mutex> lk(g_live_mu);
    for (fhs_context* c : g_live) {
        std::unique_lock<std::recursive_mutex> cl(c->mu, std::try_to_lock);
        if (cl.owns_lock()) trim_cache(c);
    }
}
static void ctx_release(fhs_context* c);

// switching key in HBM: b_j [dnum][K][N] then the dnum seeds of the uniform a_j, which the key
// inner product regenerates on the fly (SAMPLE_SEEDED): half the bytes of storing (b_j, a_j)
static size_t key_words(const fhs_context* c) { return (size_t)c->dnum * c->K * c->N + (size_t)c->dnum; }
// exported / oracle layout: [dnum][2][K][N]
static size_t key_words_full(const fhs_context* c) { return (size_t)c->dnum * 2 * c->K * c->N; }
static void dfree(fhs_context* c, void* p, size_t bytes);
// an imported key's explicit a_j (null for generated keys, whose a_j are regenerated from seeds)
static const uint64_t* key_akey(const fhs_context* c, const uint64_t* key) {
    auto it = c->key_a.find(key);
    return it == c->key_a.end() ? nullptr : it->second;
}
static void drop_seal_corr(fhs_context* c, const uint64_t* key);
static void free_key(fhs_context* c, uint64_t* key) {
    if (!key) return;
    drop_seal_corr(c, key);
    auto it = c->key_a.find(key);
    if (it != c->key_a.end()) {
        dfree(c, it->second, 8ull * c->dnum * c->K * c->N);
        c->key_a.erase(it);
    }
    dfree(c, key, 8 * key_words(c));
}

static void ctx_sync(fhs_context* c) {
    hipStreamSynchronize(c->st);
    if (c->side.st) hipStreamSynchronize(c->side.st);   // joined into st already; a failed join leaves it to this
}
// every cached block back to the device (the caller holds c->mu)
static void trim_cache(fhs_context* c) {
    if (c->free_blocks.empty()) return;
    if (getenv("FHESPEAR_TRACE_LIFETIME"))
        fprintf(stderr, "[fhespear] trim: %zu cached bytes in %zu sizes, %llu live\n", c->cached_bytes,
                c->free_blocks.size(), (unsigned long long)c->bytes_live.load());
    ctx_sync(c);   // a cached block may still be read by queued work
    for (auto& kv : c->free_blocks)
        for (void* p : kv.second) (void)hipFree(p);
    c->free_blocks.clear();
    c->cached_bytes = 0;
}
// out-of-memory retry: the other contexts on the device give their caches back too (try_lock: a
// context busy on another thread keeps its cache rather than risk a lock-order inversion)
static void trim_other_caches(fhs_context* self) {
    std::lock_guard<std::mutex> lk(g_live_mu);
    for (fhs_context* c : g_live) {
        if (c == self || c->device != self->device) continue;
        std::unique_lock<std::recursive_mutex> cl(c->mu, std::try_to_lock);
        if (cl.owns_lock()) trim_cache(c);
    }
}
static void evict_cold(fhs_context* c, size_t keep) {
    std::vector<void*> victims;
    while (c->cached_bytes > c->cache_cap) {
        size_t victim = 0;
        uint64_t oldest = ~0ull;
        for (auto& kv : c->free_blocks)
            if (kv.first != keep && !kv.second.empty() && c->size_tick[kv.first] < oldest) {
                oldest = c->size_tick[kv.first];
                victim = kv.first;
            }
        if (!victim) victim = keep;   // only the size in hand is cached: shed its blocks
        auto& v = c->free_blocks[victim];
        while (!v.empty() && c->cached_bytes > c->cache_cap) {
            victims.push_back(v.back());
            v.pop_back();
            c->cached_bytes -= victim;
        }
        if (v.empty()) c->free_blocks.erase(victim);
    }
    if (victims.empty()) return;
    ctx_sync(c);
    for (void* p : victims) (void)hipFree(p);
    c->evicted_blocks += victims.size();
}
static hipError_t dalloc(fhs_context* c, uint64_t** p, size_t bytes) {
    if (c->debug_fail_alloc >= 0 && c->debug_fail_alloc-- == 0) return hipErrorOutOfMemory;
    bytes = bytes ? bytes : 8;
    c->size_tick[bytes] = ++c->cache_tick;
    auto it = c->free_blocks.find(bytes);
    if (it != c->free_blocks.end() && !it->second.empty()) {
        *p = static_cast<uint64_t*>(it->second.back());
        it->second.pop_back();
        c->cached_bytes -= bytes;
        c->bytes_live += bytes;
        return hipSuccess;
    }
    void* v = nullptr;
    hipError_t e = hipMalloc(&v, bytes);
    if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) {   // give every cache back, retry once
        (void)hipGetLastError();
        trim_cache(c);
        trim_other_caches(c);
        e = hipMalloc(&v, bytes);
    }
    if (e == hipSuccess) {
        *p = (uint64_t*)v;
        c->bytes_live += bytes;
    } else {
        (void)hipGetLastError();   // not sticky: the next launch's hipGetLastError must not see it
    }
    return e;
}
static void dfree(fhs_context* c, void* p, size_t bytes) {
    if (!p) return;
    bytes = bytes ? bytes : 8;
    c->free_blocks[bytes].push_back(p);
    c->cached_bytes += bytes;
    c->bytes_live -= bytes;
    c->size_tick[bytes] = ++c->cache_tick;
    if (c->cached_bytes > c->cache_cap) evict_cold(c, bytes);
}
// A device temporary owned by a scope: alloc() takes a block (dalloc) and remembers its size, the destructor
// returns it to the context's cache (dfree) -- on every way out of the scope, in stream order, without a
// synchronisation.  Declare it before the launches that use it: it must outlive their enqueueing.
struct DevTmp {
    fhs_context* c;
    uint64_t* p = nullptr;
    size_t bytes = 0;
    explicit DevTmp(fhs_context* c_) : c(c_) {}
    DevTmp(const DevTmp&) = delete;
    DevTmp& operator=(const DevTmp&) = delete;
    DevTmp(DevTmp&& o) noexcept : c(o.c), p(o.p), bytes(o.bytes) { o.p = nullptr; }
    ~DevTmp() { dfree(c, p, bytes); }
    hipError_t alloc(size_t n) {
        const hipError_t e = dalloc(c, &p, n);
        if (e == hipSuccess) bytes = n;
        return e;
    }
    template <class T = uint64_t>
    T* as() const { return reinterpret_cast<T*>(p); }
};
// A switching key under construction: free_key (the key, its imported a_j, its SEAL corrections) unless released
struct KeyTmp {
    fhs_context* c;
    uint64_t* p = nullptr;
    explicit KeyTmp(fhs_context* c_) : c(c_) {}
    KeyTmp(const KeyTmp&) = delete;
    KeyTmp& operator=(const KeyTmp&) = delete;
    ~KeyTmp() { free_key(c, p); }
    hipError_t alloc() { return dalloc(c, &p, 8 * key_words(c)); }
    uint64_t* release() {
        uint64_t* k = p;
        p = nullptr;
        return k;
    }
};
static void destroy_obj(fhs_plaintext* p) { fhs_plaintext_destroy(p); }
static void destroy_obj(fhs_ciphertext* p) { fhs_ciphertext_destroy(p); }
static void destroy_obj(fhs_secret_key* p) { fhs_secret_key_destroy(p); }
static void destroy_obj(fhs_public_key* p) { fhs_public_key_destroy(p); }
static void destroy_obj(fhs_relin_key* p) { fhs_relin_key_destroy(p); }
static void destroy_obj(fhs_galois_keys* p) { fhs_galois_keys_destroy(p); }
// Owning handle of a library object on its way to the caller: destroyed by the object's own destroy function (its
// device blocks back to the cache, its context reference dropped) unless released into *out on success.
template <class Obj>
struct Own {
    Obj* p = nullptr;
    Own() = default;
    explicit Own(Obj* x) : p(x) {}
    Own(const Own&) = delete;
    Own& operator=(const Own&) = delete;
    Own(Own&& o) noexcept : p(o.p) { o.p = nullptr; }
    Own& operator=(Own&& o) noexcept {
        if (this != &o) {
            reset();
            p = o.p;
            o.p = nullptr;
        }
        return *this;
    }
    ~Own() { reset(); }
    void reset() {
        if (p) destroy_obj(p);
        p = nullptr;
    }
    Obj* release() {
        Obj* x = p;
        p = nullptr;
        return x;
    }
    Obj* operator->() const { return p; }
};
using Ct = Own<fhs_ciphertext>;
using Pt = Own<fhs_plaintext>;
// A key object under construction holds its context reference from the start, so its destroy function undoes all
// of a half-built one (null device pointers are skipped)
template <class Obj>
static Own<Obj> adopt_key(Obj* fresh) {
    ctx_retain(fresh->ctx);
    return Own<Obj>(fresh);
}
// Output array of a batch creator: cleared on entry; if the call fails part-way (e.g. device OOM,
// which bg:1164-1170 catches to fall back to on-the-fly encoding) the plaintexts already created
// are destroyed and their slots reset to null, so a failed batch leaves no HBM behind.
template <class Obj>
struct BatchOutT {
    Obj** outs;
    size_t n;
    bool kept = false;
    BatchOutT(Obj** o, size_t count) : outs(o), n(o ? count : 0) {
        for (size_t i = 0; i < n; ++i) outs[i] = nullptr;
    }
    fhs_status keep(fhs_status st) {
        kept = st == FHS_OK;
        return st;
    }
    ~BatchOutT() {
        if (kept) return;
        for (size_t i = 0; i < n; ++i)
            if (outs[i]) {
                destroy_obj(outs[i]);
                outs[i] = nullptr;
            }
    }
};
using BatchOut = BatchOutT<fhs_plaintext>;

static hipError_t scratch(fhs_context* c, int slot, size_t bytes, uint64_t** p) {
    if (bytes > c->scr_bytes[slot]) {
        if (c->scr[slot]) dfree(c, c->scr[slot], c->scr_bytes[slot]);
        c->scr[slot] = nullptr;
        c->scr_bytes[slot] = 0;
        hipError_t e = dalloc(c, &c->scr[slot], bytes);
        if (e != hipSuccess) return e;
        c->scr_bytes[slot] = bytes;
    }
    *p = c->scr[slot];
    return hipSuccess;
}

static fhs_status new_ct(fhs_context* c, int ncomp, int ci, double scale, fhs_ciphertext** out) {
    const int l = c->L0 + 1 - ci;
    if (l < 1) return fail(FHS_ERR_LEVEL, "chain index out of range");
    auto* ct = new fhs_ciphertext{c, nullptr, ncomp, ci, l, scale};
    hipError_t e = dalloc(c, &ct->d, 8ull * ncomp * l * c->N);
    if (e != hipSuccess) {
        delete ct;
        return hip_fail(e, "ciphertext allocation");
    }
    ctx_retain(c);
    *out = ct;
    return FHS_OK;
}
static fhs_status new_pt(fhs_context* c, int ci, double scale, fhs_plaintext** out) {
    const int l = c->L0 + 1 - ci;
    if (l < 1) return fail(FHS_ERR_LEVEL, "chain index out of range");
    auto* pt = new fhs_plaintext{c, nullptr, ci, l, scale};
    hipError_t e = dalloc(c, &pt->d, 8ull * l * c->N);
    if (e != hipSuccess) {
        delete pt;
        return hip_fail(e, "plaintext allocation");
    }
    ctx_retain(c);
    *out = pt;
    return FHS_OK;
}
// A block of at least *bytes: a cached block up to 1.5x the request is taken whole (*bytes becomes its size),
// so the batches of a chain walking down the levels reuse the larger blocks the levels above left in the
// cache instead of allocating (and, over the cap, freeing) one per level.
static hipError_t dalloc_fit(fhs_context* c, uint64_t** p, size_t* bytes) {
    size_t best = 0;
    for (auto& kv : c->free_blocks)
        if (!kv.second.empty() && kv.first >= *bytes && kv.first <= *bytes + *bytes / 2 && (!best || kv.first < best))
            best = kv.first;
    const bool larger = best > *bytes;
    if (best) *bytes = best;
    const hipError_t e = dalloc(c, p, *bytes);
    if (e == hipSuccess && larger) ++c->fit_hits;
    return e;
}
// `count` new plaintexts at chain index ci in one device block (PtSlab, dalloc_fit).  On failure nothing is
// left allocated and outs[0..count) are null.
static fhs_status new_pts(fhs_context* c, size_t count, int ci, double scale, fhs_plaintext** outs) {
    const int l = c->L0 + 1 - ci;
    if (l < 1) return fail(FHS_ERR_LEVEL, "chain index out of range");
    for (size_t k = 0; k < count; ++k) outs[k] = nullptr;
    if (count == 0) return FHS_OK;
    if (count == 1) return new_pt(c, ci, scale, outs);
    const size_t per = (size_t)l * c->N;
    auto* slab = new PtSlab{nullptr, 8 * count * per, 0};
    hipError_t e = dalloc_fit(c, &slab->base, &slab->bytes);
    if (e != hipSuccess) {
        delete slab;
        return hip_fail(e, "plaintext allocation");
    }
    for (size_t k = 0; k < count; ++k) {
        outs[k] = new fhs_plaintext{c, slab->base + k * per, ci, l, scale, slab};
        ++slab->refs;
        ctx_retain(c);
    }
    return FHS_OK;
}
// `count` new ciphertexts in one device block, ciphertext k at base + k ncomp l N words (a batch result that one
// launch writes as count x ncomp contiguous components).  The block returns to the cache when the last of them
// is destroyed.  On failure nothing is left allocated.
static fhs_status new_cts(fhs_context* c, int count, int ncomp, int ci, double scale, std::vector<fhs_ciphertext*>& outs) {
    const int l = c->L0 + 1 - ci;
    if (l < 1) return fail(FHS_ERR_LEVEL, "chain index out of range");
    outs.assign(count, nullptr);
    if (count == 1) return new_ct(c, ncomp, ci, scale, &outs[0]);
    const size_t per = (size_t)ncomp * l * c->N;
    auto* slab = new PtSlab{nullptr, 8 * (size_t)count * per, 0};
    hipError_t e = dalloc(c, &slab->base, slab->bytes);
    if (e != hipSuccess) {
        delete slab;
        return hip_fail(e, "ciphertext allocation");
    }
    for (int k = 0; k < count; ++k) {
        outs[k] = new fhs_ciphertext{c, slab->base + (size_t)k * per, ncomp, ci, l, scale};
        outs[k]->slab = slab;
        ++slab->refs;
        ctx_retain(c);
    }
    return FHS_OK;
}
// The batch counterpart of Ct: n new ciphertexts in one device block (new_cts) on their way to the caller, destroyed
// -- the block back to the cache -- unless committed, so the caller's array is written on success and only then.
// make() is new_cts: nothing is held when it fails.
struct CtBlock {
    fhs_context* c;
    std::vector<fhs_ciphertext*> cts;
    explicit CtBlock(fhs_context* c_) : c(c_) {}
    CtBlock(const CtBlock&) = delete;
    CtBlock& operator=(const CtBlock&) = delete;
    ~CtBlock() {
        for (fhs_ciphertext* ct : cts) destroy_obj(ct);
    }
    fhs_status make(int n, int ncomp, int ci, double scale) { return new_cts(c, n, ncomp, ci, scale, cts); }
    fhs_ciphertext* operator[](size_t i) const { return cts[i]; }
    uint64_t* base() const { return cts[0]->d; }   // [n][ncomp][l][N]: one block, or the single ciphertext
    size_t words_per_ct() const { return (size_t)cts[0]->ncomp * cts[0]->l * c->N; }
    fhs_status commit(fhs_ciphertext** out) {
        std::copy(cts.begin(), cts.end(), out);
        cts.clear();
        return FHS_OK;
    }
};
static size_t ct_bytes(const fhs_ciphertext* ct) { return 8ull * ct->ncomp * ct->l * ct->ctx->N; }
static size_t pt_bytes(const fhs_plaintext* pt) { return 8ull * pt->l * pt->ctx->N; }
// The dense limbs of a plaintext.  A compact-only one (a periodic diagonal batch, encode_rows_dev) gets them on first
// use -- expanded from its shadow on the stream (k_expand_compact) and kept for the rest of its life, so the fused
// BSGS, which reads the shadow, never pays for them.  Plaintexts are immutable: the two copies never diverge.
static hipError_t pt_dense(fhs_context* c, const fhs_plaintext* cpt, const uint64_t** out) {
    auto* pt = const_cast<fhs_plaintext*>(cpt);
    if (!pt->d) {
        if (!pt->dc) return hipErrorInvalidValue;
        uint64_t* d = nullptr;
        hipError_t e = dalloc(c, &d, pt_bytes(pt));
        if (e != hipSuccess) return e;
        e = fhs::launch_expand_compact(pt->dc, d, pt->l, c->N, pt->tlog, c->st);
        if (e != hipSuccess) {
            dfree(c, d, pt_bytes(pt));
            return e;
        }
        pt->d = d;
    }
    *out = pt->d;
    return hipSuccess;
}
#define PT_DENSE(var, pt, where)        \
    const uint64_t* var = nullptr;      \
    HIPCHK(pt_dense(c, (pt), &var), where)
// A new result object held by `var` (Own): released into *out by the caller once everything has been enqueued
#define NEW_CT(var, ...)                                              \
    Ct var;                                                           \
    do {                                                              \
        fhs_status _ns = new_ct(c, __VA_ARGS__, &var.p);              \
        if (_ns != FHS_OK) return _ns;                                \
    } while (0)
#define NEW_PT(var, ...)                                              \
    Pt var;                                                           \
    do {                                                              \
        fhs_status _ns = new_pt(c, __VA_ARGS__, &var.p);              \
        if (_ns != FHS_OK) return _ns;                                \
    } while (0)

// ---------------------------------------------------------------- timing events
// A pool of timing events per device: hipEventCreate can take milliseconds now and then (it may
// allocate a signal through the driver), so the timing hooks -- the bench's per-step events
// (fhs_event_record) and the per-kernel brackets (timer_rec) -- take pre-created events instead of
// creating them between enqueued launches, where a slow creation leaves the GPU idle inside an open
// bracket.  fhs_kernel_timer_arm tops the pool up before a timed region.
static std::mutex g_ev_mu;
static std::map<int, std::vector<hipEvent_t>> g_ev_free;
static std::unordered_map<hipEvent_t, int> g_ev_dev;
// events belong to the device current at creation: create on `dev`, whatever the calling thread has
// current (one thread may drive contexts on two GPUs), and leave the caller's current device as it was
static hipError_t ev_create_on(int dev, hipEvent_t* e) {
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) cur = -1;
    if (cur != dev && hipSetDevice(dev) != hipSuccess) return hipErrorInvalidDevice;
    hipError_t r = hipEventCreate(e);
    if (cur >= 0 && cur != dev) (void)hipSetDevice(cur);
    return r;
}
static hipEvent_t ev_get(int dev) {
    {
        std::lock_guard<std::mutex> lk(g_ev_mu);
        auto& v = g_ev_free[dev];
        if (!v.empty()) {
            hipEvent_t e = v.back();
            v.pop_back();
            return e;
        }
    }
    hipEvent_t e = nullptr;
    if (ev_create_on(dev, &e) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(g_ev_mu);
    g_ev_dev[e] = dev;
    return e;
}
static void ev_put(hipEvent_t e) {
    if (!e) return;
    std::lock_guard<std::mutex> lk(g_ev_mu);
    auto it = g_ev_dev.find(e);
    if (it == g_ev_dev.end()) {
        hipEventDestroy(e);
        return;
    }
    g_ev_free[it->second].push_back(e);
}
static void ev_reserve(int dev, size_t n) {
    std::vector<hipEvent_t> made;
    {
        std::lock_guard<std::mutex> lk(g_ev_mu);
        if (g_ev_free[dev].size() >= n) return;
        n -= g_ev_free[dev].size();
    }
    for (size_t k = 0; k < n; ++k) {
        hipEvent_t e = nullptr;
        if (ev_create_on(dev, &e) != hipSuccess) break;
        made.push_back(e);
    }
    std::lock_guard<std::mutex> lk(g_ev_mu);
    for (hipEvent_t e : made) {
        g_ev_dev[e] = dev;
        g_ev_free[dev].push_back(e);
    }
}

// ---------------------------------------------------------------- host-side latency trace
// FHESPEAR_HOST_TRACE=1 prints the host time of each section of the BSGS entry point (stderr); used
// to check that no call blocks on the GPU queue (tools/debug/host_timing.py).
struct HostTrace {
    bool on;
    std::chrono::steady_clock::time_point t0;
    HostTrace() : on(getenv("FHESPEAR_HOST_TRACE") != nullptr), t0(std::chrono::steady_clock::now()) {}
    void mark(const char* what) {
        if (!on) return;
        const auto t = std::chrono::steady_clock::now();
        fprintf(stderr, "[fhs host] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t - t0).count());
        t0 = t;
    }
};

// ---------------------------------------------------------------- staging
// Small host->device copies on the context stream.  A pageable-source hipMemcpyAsync returns only
// once the copy has run, i.e. once the stream has drained up to it, which would serialise the host
// with the GPU on every launch; staging through a pinned ring keeps the host ahead of the queue.
// The ring is cut into kRingSegs segments and a copy never straddles two.  Leaving segment k records
// an event on the stream after k's last copy; before k is written again -- a whole ring (16 MB of
// descriptors, hundreds of BSGS steps) later -- the host waits for that event, which has long
// completed.  Round 1-3 synchronised the whole stream on every wrap instead: the queue drained to
// empty, and any host delay right after it (e.g. an event creation, see timer_rec) left the GPU idle
// inside whatever kernel bracket was open.
static hipError_t stage_h2d(void* user, void* dst, const void* src, size_t bytes) {
    fhs_context* c = static_cast<fhs_context*>(user);
    constexpr size_t SEG = fhs_context::kSegBytes;
    if (!c->ring || bytes > SEG) {
        hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->st);
        return e == hipSuccess ? hipStreamSynchronize(c->st) : e;
    }
    const int seg = c->ring_seg;
    if (c->ring_head + bytes > (size_t)(seg + 1) * SEG) {   // leave segment `seg` for the next one
        hipEvent_t& out = c->ring_ev[seg];
        if (!out && hipEventCreateWithFlags(&out, hipEventDisableTiming) != hipSuccess) out = nullptr;
        hipError_t e = out ? hipEventRecord(out, c->st) : hipStreamSynchronize(c->st);
        if (e != hipSuccess) return e;
        const int next = (seg + 1) % fhs_context::kRingSegs;
        if (hipEvent_t in = c->ring_ev[next]) {
            ++c->ring_waits;
            if (hipEventQuery(in) == hipErrorNotReady) {
                ++c->ring_blocked;
                e = hipEventSynchronize(in);
                if (e != hipSuccess) return e;
            }
        }
        c->ring_seg = next;
        c->ring_head = (size_t)next * SEG;
    }
    unsigned char* p = c->ring + c->ring_head;
    memcpy(p, src, bytes);
    c->ring_head += (bytes + 255) & ~(size_t)255;
    return hipMemcpyAsync(dst, p, bytes, hipMemcpyHostToDevice, c->st);
}

// ---------------------------------------------------------------- SEAL-convention hoisting
static size_t seal_corr_bytes(const fhs_context* c, int l) { return 8ull * 2 * (l + c->P) * c->N; }
// the corrections of `key` (null: of every key), returned to the block cache in stream order
static void drop_seal_corr(fhs_context* c, const uint64_t* key) {
    for (auto it = c->seal_corr.begin(); it != c->seal_corr.end();) {
        if (key && it->first.first != key) { ++it; continue; }
        dfree(c, it->second, seal_corr_bytes(c, it->first.second));
        c->seal_corr_bytes -= seal_corr_bytes(c, it->first.second);
        it = c->seal_corr.erase(it);
    }
}
// The correction of every rotated item of a flush (computed once per (key, level) and kept with the key),
// and the zero-flag buffers.  Bounded: past FHESPEAR_SEAL_CORR_BYTES (default 1/16 of HBM) the cache is
// emptied before this flush's corrections are made (a chain walks down the levels; the corrections of the
// levels behind it go cold).
static hipError_t seal_prepare(fhs_context* c, std::vector<KsItem>& items, int l) {
    fhs::SealHoist& sh = c->seal_hoist;
    hipError_t e = hipSuccess;
    if (!sh.zflag_dev) {
        uint64_t* z = nullptr;
        e = dalloc(c, &z, 8);
        if (e != hipSuccess) return e;
        sh.zflag_dev = reinterpret_cast<unsigned*>(z);
    }
    if (!sh.zflag_host) {
        void* h = nullptr;
        e = hipHostMalloc(&h, 64, hipHostMallocDefault);
        if (e != hipSuccess) return e;
        sh.zflag_host = static_cast<unsigned*>(h);
    }
    const size_t cap = c->seal_corr_cap;   // per context, from its own device (context_create)
    size_t need = 0;
    for (const KsItem& it : items)
        if (it.elt != 1 && !c->seal_corr.count({it.key, l})) need += seal_corr_bytes(c, l);
    if (need && c->seal_corr_bytes + need > cap) {
        if (!c->seal_corr.empty()) ++c->seal_corr_drops;
        drop_seal_corr(c, nullptr);
    }
    DevTmp mask(c);
    for (KsItem& it : items) {
        if (it.elt == 1) continue;
        auto f = c->seal_corr.find({it.key, l});
        if (f == c->seal_corr.end()) {
            if (!mask.p && (e = mask.alloc(8ull * c->K * c->N)) != hipSuccess) return e;
            uint64_t* corr = nullptr;
            if ((e = dalloc(c, &corr, seal_corr_bytes(c, l))) != hipSuccess) return e;
            f = c->seal_corr.emplace(std::make_pair(it.key, l), corr).first;   // the key's from here (drop_seal_corr)
            c->seal_corr_bytes += seal_corr_bytes(c, l);
            e = fhs::launch_seal_corr(c->T, it.key, it.akey, it.elt, l, mask.p, corr, c->st);
            if (e != hipSuccess) {
                drop_seal_corr(c, it.key);   // not computed: never handed to a later flush
                return e;
            }
        }
        it.corr = f->second;
    }
    return hipSuccess;
}

// ---------------------------------------------------------------- deferred rotations
// Every flush empties the queue.  One that cannot launch marks its outputs lost (every later use of them fails
// loudly, live_ct) and no later flush may launch a key switch on inputs or outputs the caller has destroyed
// meanwhile -- the round-5 world-8 rehearsal's rank-0 abort: a flush failed out of memory, the queue kept its
// pointers, the objects were freed (and their blocks returned to the device when the cache was trimmed), and the
// next flush's key switch read and wrote freed memory.
static fhs_status drop_pending(fhs_context* c, fhs_status st) {
    if (st != FHS_OK)
        for (PendingRot& p : c->pending) p.out->lost = true;
    c->pending.clear();
    c->pending_refs.clear();
    c->pending_outs.clear();
    c->pending_l = -1;
    return st;
}
// the per-kernel event timer the launchers bracket with, when one is armed (fhs_kernel_timer)
static const fhs::KTimer* ktimer(const fhs_context* c) { return c->timer_mask ? &c->ktimer : nullptr; }
static fhs_status flush(fhs_context* c) {
    if (c->pending.empty()) return FHS_OK;
    const int R = (int)c->pending.size(), l = c->pending_l;
    // distinct inputs: rotations of the same ciphertext share one (hoisted) ModUp
    std::vector<KsItem> items(R);
    std::vector<const uint64_t*> uniq;
    std::map<const uint64_t*, int> idx;
    for (int r = 0; r < R; ++r) {
        items[r] = c->pending[r].item;
        auto ins = idx.emplace(items[r].a, (int)uniq.size());
        if (ins.second) uniq.push_back(items[r].a);
        items[r].src = (uint64_t)ins.first->second;
    }
    const int U = (int)uniq.size();
    const size_t wsb = fhs::keyswitch_workspace_bytes(c->T, R, U, l);
    uint64_t* ws = nullptr;
    HostTrace ht;
    hipError_t e = c->debug_fail_flushes > 0 ? (--c->debug_fail_flushes, hipErrorOutOfMemory)
                                             : scratch(c, fhs_context::SCR_KS, wsb, &ws);
    ht.mark("flush: workspace");
    if (e != hipSuccess) return drop_pending(c, hip_fail(e, "key-switch workspace"));
    fhs::SealHoist* sh = nullptr;
    if (c->T.ks_seal && U < R) {   // SEAL convention: one ModUp per shared input
        e = seal_prepare(c, items, l);
        if (e == hipSuccess) sh = &c->seal_hoist;
        else if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) {
            for (auto& it : items) it.corr = nullptr;   // no room for the corrections: per-rotation path
            ++c->seal_hoist.fallback;
            e = hipSuccess;
        }
        ht.mark("flush: seal corrections");
        if (e != hipSuccess) return drop_pending(c, hip_fail(e, "seal corrections"));
    }
    e = fhs::launch_keyswitch(c->T, items.data(), R, reinterpret_cast<const fhs::u64* const*>(uniq.data()), U, l, ws,
                              wsb, c->items_dev, c->stager, c->st, ktimer(c), sh);
    ht.mark("flush: launch keyswitch");
    if (e != hipSuccess) return drop_pending(c, hip_fail(e, "key-switch launch"));
    return drop_pending(c, FHS_OK);
}

struct Guard {
    fhs_context* c;
    std::lock_guard<std::recursive_mutex> lk;
    explicit Guard(fhs_context* c_) : c(c_), lk(c_->mu) {}
};
// a ciphertext whose producing rotation was dropped (drop_pending) is not an operand
static fhs_status live_ct(const fhs_ciphertext* a) {
    if (a && a->lost) return fail(FHS_ERR_INVALID, "ciphertext lost: the queued rotation producing it could not run "
                                                   "(an earlier call reported why)");
    return FHS_OK;
}
#define LIVE(ct)                                   \
    do {                                           \
        fhs_status _ls = live_ct(ct);              \
        if (_ls != FHS_OK) return _ls;             \
    } while (0)
#define ENTER(ctx)                                                           \
    if (!(ctx)) return fail(FHS_ERR_INVALID, "null context");               \
    Guard _g(ctx);                                                           \
    (void)hipGetLastError(); /* a failed HIP call of an earlier entry is not this one's */ \
    do {                                                                     \
        fhs_status _s = flush(ctx);                                          \
        if (_s != FHS_OK) return _s;                                         \
    } while (0)

// ============================================================================ context
static void ctx_free(fhs_context* c);
// One table into a device block of its own, the context's (c->tables) from the moment it exists
static hipError_t upload_table(fhs_context* c, const void* src, size_t bytes, const void** dst) {
    void* d = nullptr;
    const hipError_t e = hipMalloc(&d, bytes);
    if (e != hipSuccess) return e;
    c->tables.push_back(d);
    *dst = d;
    return hipMemcpy(d, src, bytes, hipMemcpyHostToDevice);
}
// Validate, select the device, derive every table on the host (fhs_tables.h), then the device side: nothing
// touches the HIP runtime before the arguments have passed, and from its first resource on the half-built
// context is released by ctx_free on every way out but the last.
extern "C" fhs_status fhs_context_create(uint64_t N, const uint64_t* primes, int nprimes, int special,
                                         const uint64_t* galois_elts, int n_elts, int device, fhs_context** out) {
    if (!out) return fail(FHS_ERR_INVALID, "context_create: null argument");
    if (const char* bad = context_params_error(N, primes, nprimes, special, galois_elts, n_elts))
        return fail(FHS_ERR_INVALID, bad);
    segv_trace_install();
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(FHS_ERR_NODEVICE, "no HIP device: libfhespear_hip needs an MI355X (gfx950)");
    if (device < 0 || device >= ndev) return fail(FHS_ERR_INVALID, "context_create: bad device index");
    HIPCHK(hipSetDevice(device), "hipSetDevice");

    HostTables H;
    if (const char* bad = build_host_tables(N, primes, nprimes, special, H)) return fail(FHS_ERR_INVALID, bad);

    std::unique_ptr<fhs_context, void (*)(fhs_context*)> c(new fhs_context, ctx_free);
    c->device = device;
    c->N = N; c->logN = H.logN; c->K = H.K; c->P = H.P; c->L0 = H.L0; c->dnum = H.dnum;
    c->q.assign(primes, primes + nprimes);
    c->elts = galois_elts && n_elts > 0 ? std::vector<uint64_t>(galois_elts, galois_elts + n_elts) : default_galois_elts(N);
    c->fft_w = std::move(H.fft_w);
    c->slot_index = std::move(H.slot_index);
    HIPCHK(hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking), "hipStreamCreate");
    {   // the side stream's few short kernels go ahead of the long launch they run beside: without priority their
        // large workgroups wait for the long launch's smaller ones to leave whole CUs free, i.e. for its tail
        int prio_lo = 0, prio_hi = 0;
        HIPCHK(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi), "hipDeviceGetStreamPriorityRange");
        HIPCHK(hipStreamCreateWithPriority(&c->side.st, hipStreamNonBlocking, prio_hi), "hipStreamCreate (side)");
    }
    HIPCHK(hipEventCreateWithFlags(&c->side.fork, hipEventDisableTiming), "hipEventCreate (fork)");
    HIPCHK(hipEventCreateWithFlags(&c->side.join, hipEventDisableTiming), "hipEventCreate (join)");
    {
        static std::once_flag exit_once;
        std::call_once(exit_once, [] { atexit(release_at_exit); });
        size_t free_b = 0, total_b = 0;
        (void)hipMemGetInfo(&free_b, &total_b);
        c->cache_cap = total_b / 4;
        if (const char* e = getenv("FHESPEAR_CACHE_BYTES")) c->cache_cap = strtoull(e, nullptr, 10);
        // SEAL-hoisting corrections: 1/16 of this context's device (seal_prepare)
        c->seal_corr_cap = total_b ? total_b / 16 : (size_t)16 << 30;
        if (const char* e = getenv("FHESPEAR_SEAL_CORR_BYTES")) c->seal_corr_cap = strtoull(e, nullptr, 10);
    }
    DevTables& T = c->T;
    T.N = H.N; T.logN = H.logN; T.L0 = H.L0; T.P = H.P; T.K = H.K; T.dnum = H.dnum;
    T.max_qbits = H.max_qbits; T.modup_dp = H.modup_dp; T.md_xform = H.md_xform;
    T.conv_b59 = H.conv_b59; T.all_b59 = H.all_b59;
#define UP(field, count) \
    HIPCHK(upload_table(c.get(), H.field.data(), sizeof(H.field[0]) * (count), (const void**)&T.field), "tables")
#define UP_ALL(field) UP(field, H.field.size())
    UP_ALL(primes); UP_ALL(tw_fwd); UP_ALL(tw_inv);
    UP_ALL(modup_intt); UP_ALL(modup_hat); UP_ALL(modup_R); UP_ALL(modup_Q); UP_ALL(modup_xd); UP_ALL(modup_xt);
    UP_ALL(md_xd); UP_ALL(md_intt); UP_ALL(md_hat); UP_ALL(md_pinv);
    UP_ALL(rescale); UP_ALL(pow2);
    UP_ALL(dec_w); UP(dec_twist, N / 2); UP_ALL(dec_pos);   // the GPU decoder reads the first half of the host's twists
    UP_ALL(enc_w); UP_ALL(enc_twist); UP_ALL(enc_pos);
#undef UP_ALL
#undef UP
    c->dec_twist = std::move(H.dec_twist);
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&c->ring), fhs_context::kRingBytes, hipHostMallocDefault),
           "staging ring");
    c->stager = fhs::Stager{c.get(), stage_h2d};
    HIPCHK(hipMalloc(&c->items_dev, (sizeof(KsItem) + sizeof(void*)) * fhs_context::kMaxItems), "items buffer");
    c->tables.push_back(c->items_dev);
    HIPCHK(hipMalloc(&c->ptrs_dev, sizeof(void*) * 2 * fhs_context::kMaxPtrs), "pointer buffer");
    c->tables.push_back(c->ptrs_dev);
    {
        std::lock_guard<std::mutex> lk(g_live_mu);
        g_live.insert(c.get());
    }
    *out = c.release();
    return FHS_OK;
}

// Also the release of a half-built context (fhs_context_create): whatever does not exist yet is skipped.
static void ctx_free(fhs_context* c) {
    const bool trace = getenv("FHESPEAR_TRACE_LIFETIME") != nullptr;
    if (trace)
        fprintf(stderr, "[fhespear] context %p: freeing (%zu cached bytes, %llu live)\n", (void*)c, c->cached_bytes,
                (unsigned long long)c->bytes_live.load());
    {
        Guard g(c);
        flush(c);
        if (c->st) {
            hipStreamSynchronize(c->st);
            ctx_sync(c);
        }
        for (void* p : c->tables) hipFree(p);
        for (auto& kv : c->seal_corr) hipFree(kv.second);
        c->seal_corr.clear();
        if (c->seal_hoist.zflag_dev) hipFree(c->seal_hoist.zflag_dev);
        if (c->seal_hoist.zflag_host) hipHostFree(c->seal_hoist.zflag_host);
        for (int k = 0; k < fhs_context::SCR_COUNT; ++k)
            if (c->scr[k]) hipFree(c->scr[k]);
        {
            std::lock_guard<std::mutex> lk(g_live_mu);
            g_live.erase(c);
        }
        for (auto& kv : c->free_blocks)
            for (void* p : kv.second) hipFree(p);
        c->free_blocks.clear();
        if (c->ring) hipHostFree(c->ring);
        if (c->readback) hipHostFree(c->readback);
        for (hipEvent_t e : c->ring_ev)
            if (e) hipEventDestroy(e);
        for (auto& v : c->timer_pairs)
            for (auto& pr : v) { ev_put(pr.first); ev_put(pr.second); }
        for (hipEvent_t e : c->timer_open)
            if (e) ev_put(e);
        if (c->side.fork) hipEventDestroy(c->side.fork);
        if (c->side.join) hipEventDestroy(c->side.join);
        if (c->side.st) hipStreamDestroy(c->side.st);
        if (c->st) hipStreamDestroy(c->st);
    }
    delete c;
    if (trace) fprintf(stderr, "[fhespear] context %p: freed\n", (void*)c);
}
static void ctx_release(fhs_context* c) {
    if (c->refs.fetch_sub(1) == 1) ctx_free(c);
}
extern "C" fhs_status fhs_context_destroy(fhs_context* c) {
    if (!c) return FHS_OK;
    ctx_release(c);
    return FHS_OK;
}
extern "C" fhs_status fhs_context_info(const fhs_context* c, uint64_t* N, int* L0, int* P, int* n_elts) {
    if (!c) return fail(FHS_ERR_INVALID, "null context");
    if (N) *N = c->N;
    if (L0) *L0 = c->L0;
    if (P) *P = c->P;
    if (n_elts) *n_elts = (int)c->elts.size();
    return FHS_OK;
}
extern "C" fhs_status fhs_context_galois_elts(const fhs_context* c, uint64_t* out) {
    if (!c || !out) return fail(FHS_ERR_INVALID, "null argument");
    std::copy(c->elts.begin(), c->elts.end(), out);
    return FHS_OK;
}
extern "C" fhs_status fhs_synchronize(fhs_context* c) {
    ENTER(c);
    HIPCHK(hipStreamSynchronize(c->st), "hipStreamSynchronize");
    return FHS_OK;
}
extern "C" fhs_status fhs_memory_in_use(fhs_context* c, uint64_t* bytes) {
    if (!c || !bytes) return fail(FHS_ERR_INVALID, "null argument");
    *bytes = c->bytes_live.load();
    return FHS_OK;
}

// ============================================================================ sampling helpers
// sm64: fhs_modarith.h (host + device)
// 256 bits from the OS entropy pool (a secret key created without a caller-supplied key)
static bool os_random(void* buf, size_t n) {
    FILE* f = fopen("/dev/urandom", "rb");
    if (!f) return false;
    const size_t got = fread(buf, 1, n, f);
    fclose(f);
    return got == n;
}
static uint64_t prf_u64(const PrfKey& K, uint64_t sid) {
    uint64_t w0, w1;
    prf128(K, sid, 0, w0, w1);
    return w0;
}
static uint64_t stream_id(uint64_t kind, uint64_t a, uint64_t b) { return (kind << 56) | (a << 16) | b; }
// Reproducible randomness for parity checks (FHESPEAR_PARITY_RNG set: tests/conftest.py, bench.py, smoke):
// encryption counters start at 0 and a public key's mask key is PRF(secret key, generation) alone, so a
// seeded key reproduces the oracle's ciphertexts.  Otherwise each secret key's symmetric-encryption
// counter starts at a fresh random offset and each public key's mask key has 256 fresh random bits
// mixed in: a secret key recreated from the same 32 key bytes (another process, another context) never
// repeats an encryption mask, which would reveal the difference of the two messages.
// Only the exact value "1" enables it (0, empty or anything else leaves the secure default), and the
// first use in a process says so on stderr: ciphertexts made in this mode reuse mask streams across
// processes and must never leave a test.
static bool parity_rng() {
    const char* v = getenv("FHESPEAR_PARITY_RNG");
    if (!v || strcmp(v, "1") != 0) return false;
    static std::atomic<bool> warned{false};
    if (!warned.exchange(true))
        fprintf(stderr, "[fhespear] FHESPEAR_PARITY_RNG=1: deterministic encryption randomness (parity tests "
                        "only; never for real data)\n");
    return true;
}
enum { ST_SECRET = 1, ST_PUBKEY = 2, ST_RELIN = 3, ST_GALOIS = 4, ST_ENC_SYM = 5, ST_ENC_ASYM = 6, ST_PK_RNG = 7 };

// sample a small polynomial (ternary/CBD) over `limbs` primes and NTT it
static hipError_t sample_small_ntt(fhs_context* c, int mode, const PrfKey& K, uint64_t sid, uint64_t* out, int limbs) {
    hipError_t e = fhs::launch_sample(c->T, mode, K, sid, out, limbs, c->st);
    if (e != hipSuccess) return e;
    return fhs::launch_ntt_fwd(c->T, out, limbs, limbs, 1, 0, c->st);
}

// ============================================================================ keys
extern "C" fhs_status fhs_secret_key_create(fhs_context* c, const uint8_t* key32, fhs_secret_key** out) {
    ENTER(c);
    if (!out) return fail(FHS_ERR_INVALID, "null out");
    PrfKey K{};
    if (key32) {
        for (int w = 0; w < 8; ++w)
            K.k[w] = (uint32_t)key32[4 * w] | ((uint32_t)key32[4 * w + 1] << 8) | ((uint32_t)key32[4 * w + 2] << 16) |
                     ((uint32_t)key32[4 * w + 3] << 24);
    } else if (!os_random(K.k, sizeof(K.k))) {
        return fail(FHS_ERR_INVALID, "secret_key: /dev/urandom unavailable");
    }
    uint64_t ctr0 = 0;   // stream ids carry 40 counter bits: a random start below 2^39 leaves 2^39 encryptions
    if (!parity_rng() && !os_random(&ctr0, sizeof ctr0)) return fail(FHS_ERR_INVALID, "secret_key: /dev/urandom unavailable");
    auto sk = adopt_key(new fhs_secret_key{c, nullptr, K, ctr0 & ((1ull << 39) - 1)});
    HIPCHK(dalloc(c, &sk->s, 8ull * c->K * c->N), "secret key");
    HIPCHK(sample_small_ntt(c, fhs::SAMPLE_TERNARY, sk->key, stream_id(ST_SECRET, 0, 0), sk->s, c->K),
           "secret key sampling");
    *out = sk.release();
    return FHS_OK;
}
extern "C" fhs_status fhs_secret_key_destroy(fhs_secret_key* sk) {
    if (!sk) return FHS_OK;
    fhs_context* c = sk->ctx;
    { Guard g(c); flush(c); dfree(c, sk->s, 8ull * c->K * c->N); }
    delete sk;
    ctx_release(c);
    return FHS_OK;
}

static fhs_status gen_switch_key(fhs_context* c, const PrfKey& K, uint64_t base, const uint64_t* s, const uint64_t* snew,
                                 uint64_t** key_out) {
    KeyTmp key(c);
    HIPCHK(key.alloc(), "switching key");
    const size_t S = (size_t)c->K * c->N;
    DevTmp tmp(c);   // e | a
    HIPCHK(tmp.alloc(16 * S), "switching key");
    uint64_t* ebuf = tmp.p;
    uint64_t* abuf = tmp.p + S;
    std::vector<uint64_t> seeds(c->dnum);
    for (int j = 0; j < c->dnum; ++j) {
        seeds[j] = prf_u64(K, base | (uint64_t)(2 * j));   // public seed of a_j: a PRF output
        HIPCHK(fhs::launch_sample(c->T, fhs::SAMPLE_SEEDED, K, seeds[j], abuf, c->K, c->st), "switching key generation");
        HIPCHK(sample_small_ntt(c, fhs::SAMPLE_CBD, K, base | (uint64_t)(2 * j + 1), ebuf, c->K), "switching key generation");
        HIPCHK(fhs::launch_switch_key_assemble(c->T, key.p + (size_t)j * S, abuf, ebuf, s, snew, j, c->st),
               "switching key generation");
    }
    HIPCHK(hipMemcpyAsync(key.p + (size_t)c->dnum * S, seeds.data(), 8 * seeds.size(), hipMemcpyHostToDevice, c->st),
           "switching key generation");
    HIPCHK(hipStreamSynchronize(c->st), "switching key generation");   // `seeds` is a host temporary
    *key_out = key.release();
    return FHS_OK;
}
// [dnum][2][K][N] with the a_j regenerated from their seeds (the oracle's layout)
static fhs_status export_switch_key(fhs_context* c, const uint64_t* key, uint64_t* host) {
    const size_t S = (size_t)c->K * c->N;
    if (const uint64_t* akey = key_akey(c, key)) {   // imported: (b_j, a_j) as given
        for (int j = 0; j < c->dnum; ++j) {
            HIPCHK(hipMemcpyAsync(host + (size_t)j * 2 * S, key + (size_t)j * S, 8 * S, hipMemcpyDeviceToHost, c->st),
                   "key export");
            HIPCHK(hipMemcpyAsync(host + ((size_t)j * 2 + 1) * S, akey + (size_t)j * S, 8 * S, hipMemcpyDeviceToHost,
                                  c->st), "key export");
        }
        HIPCHK(hipStreamSynchronize(c->st), "key export");
        return FHS_OK;
    }
    std::vector<uint64_t> seeds(c->dnum);
    HIPCHK(hipMemcpyAsync(seeds.data(), key + (size_t)c->dnum * S, 8 * seeds.size(), hipMemcpyDeviceToHost, c->st),
           "key export");
    HIPCHK(hipStreamSynchronize(c->st), "key export");
    DevTmp full(c);
    HIPCHK(full.alloc(8 * key_words_full(c)), "key export");
    for (int j = 0; j < c->dnum; ++j) {
        HIPCHK(hipMemcpyAsync(full.p + (size_t)j * 2 * S, key + (size_t)j * S, 8 * S, hipMemcpyDeviceToDevice, c->st),
               "key export");
        HIPCHK(fhs::launch_sample(c->T, fhs::SAMPLE_SEEDED, PrfKey{}, seeds[j], full.p + ((size_t)j * 2 + 1) * S, c->K,
                                  c->st), "key export");
    }
    HIPCHK(hipMemcpyAsync(host, full.p, 8 * key_words_full(c), hipMemcpyDeviceToHost, c->st), "key export");
    HIPCHK(hipStreamSynchronize(c->st), "key export");
    return FHS_OK;
}

extern "C" fhs_status fhs_gen_relin_key(fhs_context* c, fhs_secret_key* sk, fhs_relin_key** out) {
    ENTER(c);
    if (!sk || !out) return fail(FHS_ERR_INVALID, "null argument");
    DevTmp s2(c);
    HIPCHK(s2.alloc(8ull * c->K * c->N), "relin key");
    HIPCHK(fhs::launch_key_prod(c->T, sk->s, sk->s, s2.p, c->K, c->st), "relin key");
    auto rk = adopt_key(new fhs_relin_key{c, nullptr});
    fhs_status s = gen_switch_key(c, sk->key, stream_id(ST_RELIN, 0, 0), sk->s, s2.p, &rk->key);
    if (s != FHS_OK) return s;
    *out = rk.release();
    return FHS_OK;
}
extern "C" fhs_status fhs_relin_key_destroy(fhs_relin_key* rk) {
    if (!rk) return FHS_OK;
    fhs_context* c = rk->ctx;
    { Guard g(c); flush(c); free_key(c, rk->key); }
    delete rk;
    ctx_release(c);
    return FHS_OK;
}

extern "C" fhs_status fhs_create_galois_keys(fhs_context* c, fhs_secret_key* sk, const uint64_t* elts, int n,
                                             fhs_galois_keys** out) {
    ENTER(c);
    if (!sk || !out) return fail(FHS_ERR_INVALID, "null argument");
    std::vector<uint64_t> list = (elts && n > 0) ? std::vector<uint64_t>(elts, elts + n) : c->elts;
    auto gk = adopt_key(new fhs_galois_keys{c, {}});
    DevTmp sn(c);
    HIPCHK(sn.alloc(8ull * c->K * c->N), "galois keys");
    for (uint64_t elt : list) {
        if (gk->keys.count(elt)) continue;
        if ((elt & 1) == 0 || elt >= 2 * c->N) return hip_fail(hipErrorInvalidValue, "galois key generation");
        HIPCHK(fhs::launch_galois_perm(c->T, sk->s, sn.p, c->K, elt, c->st), "galois key generation");
        // straight into its slot (null until the key is complete; the destroy function skips a null one)
        fhs_status s = gen_switch_key(c, sk->key, stream_id(ST_GALOIS, elt, 0), sk->s, sn.p, &gk->keys[elt]);
        if (s != FHS_OK) return s;
    }
    *out = gk.release();
    return FHS_OK;
}
extern "C" fhs_status fhs_galois_keys_destroy(fhs_galois_keys* gk) {
    if (!gk) return FHS_OK;
    fhs_context* c = gk->ctx;
    {
        Guard g(c);
        flush(c);
        for (auto& kv : gk->keys) free_key(c, kv.second);
    }
    delete gk;
    ctx_release(c);
    return FHS_OK;
}
extern "C" fhs_status fhs_galois_keys_has(const fhs_galois_keys* gk, uint64_t elt, int* has) {
    if (!gk || !has) return fail(FHS_ERR_INVALID, "null argument");
    *has = gk->keys.count(elt) ? 1 : 0;
    return FHS_OK;
}
extern "C" fhs_status fhs_galois_keys_bytes(const fhs_galois_keys* gk, uint64_t* bytes) {
    if (!gk || !bytes) return fail(FHS_ERR_INVALID, "null argument");
    *bytes = (uint64_t)gk->keys.size() * 8 * key_words(gk->ctx);
    return FHS_OK;
}

static fhs_status export_dev(fhs_context* c, const void* d, size_t bytes, void* host) {
    HIPCHK(hipMemcpyAsync(host, d, bytes, hipMemcpyDeviceToHost, c->st), "export");
    HIPCHK(hipStreamSynchronize(c->st), "export sync");
    return FHS_OK;
}
extern "C" fhs_status fhs_galois_key_export(fhs_context* c, const fhs_galois_keys* gk, uint64_t elt, uint64_t* host) {
    ENTER(c);
    if (!gk || !host) return fail(FHS_ERR_INVALID, "null argument");
    auto it = gk->keys.find(elt);
    if (it == gk->keys.end()) return fail(FHS_ERR_KEY, "galois key not present");
    return export_switch_key(c, it->second, host);
}
extern "C" fhs_status fhs_relin_key_export(fhs_context* c, const fhs_relin_key* rk, uint64_t* host) {
    ENTER(c);
    if (!rk || !host) return fail(FHS_ERR_INVALID, "null argument");
    return export_switch_key(c, rk->key, host);
}
// ---- key import ("identical keys": a key set produced elsewhere, e.g. by SEAL, in the export layout)
static bool canonical_limbs(const fhs_context* c, const uint64_t* host, int nlimbs, int limb0) {
    for (int i = 0; i < nlimbs; ++i) {
        const uint64_t q = c->q[(limb0 + i) % c->K];
        const uint64_t* v = host + (size_t)i * c->N;
        for (uint64_t n = 0; n < c->N; ++n)
            if (v[n] >= q) return false;
    }
    return true;
}
// host [dnum][2][K][N] -> b_j in the key, a_j in a companion allocation (key_a)
static fhs_status import_switch_key(fhs_context* c, const uint64_t* host, uint64_t** key_out) {
    const size_t S = (size_t)c->K * c->N;
    for (int j = 0; j < 2 * c->dnum; ++j)
        if (!canonical_limbs(c, host + (size_t)j * S, c->K, 0))
            return fail(FHS_ERR_INVALID, "key import: residues must be canonical (< q_i) in [dnum][2][K][N] order");
    KeyTmp key(c);
    HIPCHK(key.alloc(), "key import");
    uint64_t* a = nullptr;
    HIPCHK(dalloc(c, &a, 8ull * c->dnum * S), "key import");
    c->key_a[key.p] = a;   // from here free_key releases the pair
    for (int j = 0; j < c->dnum; ++j) {
        HIPCHK(hipMemcpyAsync(key.p + (size_t)j * S, host + (size_t)j * 2 * S, 8 * S, hipMemcpyHostToDevice, c->st),
               "key import");
        HIPCHK(hipMemcpyAsync(a + (size_t)j * S, host + ((size_t)j * 2 + 1) * S, 8 * S, hipMemcpyHostToDevice, c->st),
               "key import");
    }
    HIPCHK(hipMemsetAsync(key.p + (size_t)c->dnum * S, 0, 8 * c->dnum, c->st), "key import");
    HIPCHK(hipStreamSynchronize(c->st), "key import");   // pageable host source
    *key_out = key.release();
    return FHS_OK;
}
extern "C" fhs_status fhs_galois_keys_import(fhs_context* c, const uint64_t* elts, int n, const uint64_t* host,
                                             fhs_galois_keys** out) {
    ENTER(c);
    if (!elts || n < 1 || !host || !out) return fail(FHS_ERR_INVALID, "galois_keys_import: bad args");
    auto gk = adopt_key(new fhs_galois_keys{c, {}});
    for (int k = 0; k < n; ++k) {
        if ((elts[k] & 1) == 0 || elts[k] >= 2 * c->N || gk->keys.count(elts[k]))
            return fail(FHS_ERR_INVALID, "galois_keys_import: invalid or repeated galois element");
        fhs_status s = import_switch_key(c, host + (size_t)k * key_words_full(c), &gk->keys[elts[k]]);
        if (s != FHS_OK) return s;
    }
    *out = gk.release();
    return FHS_OK;
}
extern "C" fhs_status fhs_relin_key_import(fhs_context* c, const uint64_t* host, fhs_relin_key** out) {
    ENTER(c);
    if (!host || !out) return fail(FHS_ERR_INVALID, "null argument");
    auto rk = adopt_key(new fhs_relin_key{c, nullptr});
    fhs_status s = import_switch_key(c, host, &rk->key);
    if (s != FHS_OK) return s;
    *out = rk.release();
    return FHS_OK;
}
extern "C" fhs_status fhs_secret_key_import(fhs_context* c, const uint64_t* host, fhs_secret_key** out) {
    ENTER(c);
    if (!host || !out) return fail(FHS_ERR_INVALID, "null argument");
    if (!canonical_limbs(c, host, c->K, 0)) return fail(FHS_ERR_INVALID, "secret_key_import: residues must be < q_i");
    PrfKey K{};
    if (!os_random(K.k, sizeof(K.k))) return fail(FHS_ERR_INVALID, "secret_key_import: /dev/urandom unavailable");
    auto sk = adopt_key(new fhs_secret_key{c, nullptr, K, 0});   // fresh encryption randomness
    HIPCHK(dalloc(c, &sk->s, 8ull * c->K * c->N), "secret_key_import");
    HIPCHK(hipMemcpyAsync(sk->s, host, 8ull * c->K * c->N, hipMemcpyHostToDevice, c->st), "secret_key_import");
    HIPCHK(hipStreamSynchronize(c->st), "secret_key_import");
    *out = sk.release();
    return FHS_OK;
}
// key-switch convention of the context (fhs_kernels.h DevTables::ks_seal)
extern "C" fhs_status fhs_context_set_key_switch_mode(fhs_context* c, int mode) {
    ENTER(c);
    if (mode != FHS_KS_EXACT && mode != FHS_KS_SEAL) return fail(FHS_ERR_INVALID, "key switch mode: 0 exact, 1 seal");
    if (mode == FHS_KS_SEAL && c->P != 1)
        return fail(FHS_ERR_INVALID, "key switch mode seal: SEAL's switch_key_inplace has one special prime (P = 1)");
    c->T.ks_seal = mode == FHS_KS_SEAL;
    drop_seal_corr(c, nullptr);
    return FHS_OK;
}
extern "C" fhs_status fhs_seal_hoist_stats(fhs_context* c, uint64_t* hoisted, uint64_t* fallback) {
    ENTER(c);
    if (!hoisted || !fallback) return fail(FHS_ERR_INVALID, "null argument");
    *hoisted = c->seal_hoist.hoisted;
    *fallback = c->seal_hoist.fallback;
    return FHS_OK;
}
extern "C" fhs_status fhs_context_key_switch_mode(const fhs_context* c, int* mode) {
    if (!c || !mode) return fail(FHS_ERR_INVALID, "null argument");
    *mode = c->T.ks_seal ? FHS_KS_SEAL : FHS_KS_EXACT;
    return FHS_OK;
}
extern "C" fhs_status fhs_secret_key_export(fhs_context* c, const fhs_secret_key* sk, uint64_t* host) {
    ENTER(c);
    if (!sk || !host) return fail(FHS_ERR_INVALID, "null argument");
    return export_dev(c, sk->s, 8ull * c->K * c->N, host);
}

extern "C" fhs_status fhs_gen_public_key(fhs_context* c, fhs_secret_key* sk, fhs_public_key** out) {
    ENTER(c);
    if (!sk || !out) return fail(FHS_ERR_INVALID, "null argument");
    auto pk = adopt_key(new fhs_public_key{c, nullptr, PrfKey{}, 1ull << 20});
    // rng = 256 PRF bits of stream (ST_PK_RNG, generation): two public keys of one secret key never
    // share encryption masks (their key material is the same, so shared masks would reveal m1 - m2)
    const uint64_t gen = sk->pk_gen++;
    for (int w = 0; w < 4; ++w) {
        uint64_t w0, w1;
        prf128(sk->key, stream_id(ST_PK_RNG, gen, 0), (uint32_t)w, w0, w1);
        pk->rng.k[2 * w] = (uint32_t)w0;
        pk->rng.k[2 * w + 1] = (uint32_t)(w0 >> 32);
    }
    if (!parity_rng()) {   // fresh bits: the same secret key recreated elsewhere never repeats a mask stream
        PrfKey nonce{};
        if (!os_random(nonce.k, sizeof nonce.k)) return fail(FHS_ERR_INVALID, "public key: /dev/urandom unavailable");
        for (int w = 0; w < 8; ++w) pk->rng.k[w] ^= nonce.k[w];
    }
    const size_t S = (size_t)c->L0 * c->N;
    HIPCHK(dalloc(c, &pk->pk, 16 * S), "public key");
    DevTmp eb(c);
    HIPCHK(eb.alloc(8 * S), "public key generation");
    HIPCHK(fhs::launch_sample(c->T, fhs::SAMPLE_UNIFORM, sk->key, stream_id(ST_PUBKEY, 0, 0), pk->pk + S, c->L0, c->st),
           "public key generation");
    HIPCHK(sample_small_ntt(c, fhs::SAMPLE_CBD, sk->key, stream_id(ST_PUBKEY, 0, 1), eb.p, c->L0), "public key generation");
    HIPCHK(fhs::launch_encrypt_combine(c->T, 0, pk->pk, pk->pk + S, sk->s, nullptr, nullptr, eb.p, nullptr, nullptr,
                                       c->L0, c->st), "public key generation");
    *out = pk.release();
    return FHS_OK;
}
extern "C" fhs_status fhs_public_key_destroy(fhs_public_key* pk) {
    if (!pk) return FHS_OK;
    fhs_context* c = pk->ctx;
    { Guard g(c); flush(c); dfree(c, pk->pk, 16ull * c->L0 * c->N); }
    delete pk;
    ctx_release(c);
    return FHS_OK;
}
extern "C" fhs_status fhs_public_key_export(fhs_context* c, const fhs_public_key* pk, uint64_t* host) {
    ENTER(c);
    if (!pk || !host) return fail(FHS_ERR_INVALID, "null argument");
    return export_dev(c, pk->pk, 16ull * c->L0 * c->N, host);
}

// ============================================================================ object API
static bool pending_uses(fhs_context* c, const void* p) { return c->pending_refs.count(p) != 0; }

extern "C" fhs_status fhs_ciphertext_destroy(fhs_ciphertext* ct) {
    if (!ct) return FHS_OK;
    fhs_context* c = ct->ctx;
    {
        Guard g(c);
        if (pending_uses(c, ct)) flush(c);
        if (ct->slab) {
            if (--ct->slab->refs == 0) {
                dfree(c, ct->slab->base, ct->slab->bytes);
                delete ct->slab;
            }
        } else {
            dfree(c, ct->d, ct_bytes(ct));
        }
    }
    delete ct;
    ctx_release(c);
    return FHS_OK;
}
extern "C" fhs_status fhs_plaintext_destroy(fhs_plaintext* pt) {
    if (!pt) return FHS_OK;
    fhs_context* c = pt->ctx;
    {
        Guard g(c);
        if (pt->slab) {
            if (--pt->slab->refs == 0) {
                dfree(c, pt->slab->base, pt->slab->bytes);
                delete pt->slab;
            }
        } else {
            dfree(c, pt->d, pt_bytes(pt));
        }
        if (pt->cslab && --pt->cslab->refs == 0) {
            dfree(c, pt->cslab->base, pt->cslab->bytes);
            delete pt->cslab;
        }
    }
    delete pt;
    ctx_release(c);
    return FHS_OK;
}
// Largest batch one launch takes (its item count is a grid dimension of the sampler, NTT, combine, decrypt
// and CRT kernels, and its scratch is count x l x N words); bigger batches are processed in chunks of this
// many items, with the same results as one call per item
static constexpr int kMaxBatch = 4096;
extern "C" fhs_status fhs_ciphertext_info(const fhs_ciphertext* ct, int* ncomp, int* ci, int* l, double* scale) {
    if (!ct) return fail(FHS_ERR_INVALID, "null ciphertext");
    if (ncomp) *ncomp = ct->ncomp;
    if (ci) *ci = ct->ci;
    if (l) *l = ct->l;
    if (scale) *scale = ct->scale;
    return FHS_OK;
}
extern "C" fhs_status fhs_ciphertext_set_scale(fhs_ciphertext* ct, double scale) {
    if (!ct) return fail(FHS_ERR_INVALID, "null ciphertext");
    ct->scale = scale;
    return FHS_OK;
}
extern "C" fhs_status fhs_plaintext_info(const fhs_plaintext* pt, int* ci, int* l, double* scale) {
    if (!pt) return fail(FHS_ERR_INVALID, "null plaintext");
    if (ci) *ci = pt->ci;
    if (l) *l = pt->l;
    if (scale) *scale = pt->scale;
    return FHS_OK;
}
extern "C" fhs_status fhs_ciphertext_export(fhs_context* c, const fhs_ciphertext* ct, uint64_t* host) {
    ENTER(c);
    if (!ct || !host) return fail(FHS_ERR_INVALID, "null argument");
    LIVE(ct);
    return export_dev(c, ct->d, ct_bytes(ct), host);
}
extern "C" fhs_status fhs_plaintext_export(fhs_context* c, const fhs_plaintext* pt, uint64_t* host) {
    ENTER(c);
    if (!pt || !host) return fail(FHS_ERR_INVALID, "null argument");
    PT_DENSE(pd, pt, "plaintext_export");
    return export_dev(c, pd, pt_bytes(pt), host);
}
extern "C" fhs_status fhs_ciphertext_import(fhs_context* c, const uint64_t* host, int ncomp, int ci, double scale,
                                            fhs_ciphertext** out) {
    ENTER(c);
    if (!host || !out || ncomp < 2 || ncomp > 3) return fail(FHS_ERR_INVALID, "ciphertext_import: bad args");
    NEW_CT(ct, ncomp, ci, scale);
    HIPCHK(hipMemcpyAsync(ct->d, host, ct_bytes(ct.p), hipMemcpyHostToDevice, c->st), "ciphertext_import");
    HIPCHK(hipStreamSynchronize(c->st), "ciphertext_import");
    *out = ct.release();
    return FHS_OK;
}
extern "C" fhs_status fhs_plaintext_import(fhs_context* c, const uint64_t* host, int ci, double scale,
                                           fhs_plaintext** out) {
    ENTER(c);
    if (!host || !out) return fail(FHS_ERR_INVALID, "plaintext_import: bad args");
    NEW_PT(pt, ci, scale);
    HIPCHK(hipMemcpyAsync(pt->d, host, pt_bytes(pt.p), hipMemcpyHostToDevice, c->st), "plaintext_import");
    HIPCHK(hipStreamSynchronize(c->st), "plaintext_import");
    *out = pt.release();
    return FHS_OK;
}
extern "C" fhs_status fhs_debug_fail_next_flushes(fhs_context* c, int count) {
    if (!c || count < 0) return fail(FHS_ERR_INVALID, "debug_fail_next_flushes: bad args");
    Guard g(c);
    c->debug_fail_flushes = count;
    return FHS_OK;
}
extern "C" fhs_status fhs_debug_force_fork(fhs_context* c, int on, uint64_t* forked) {
    if (!c) return fail(FHS_ERR_INVALID, "debug_force_fork: null context");
    Guard g(c);
    if (on >= 0) c->side.min_wg = on ? 0 : fhs::kForkMinWg;
    if (forked) *forked = c->side.forked;
    return FHS_OK;
}
extern "C" fhs_status fhs_debug_fail_alloc(fhs_context* c, int nth, int* was_armed) {
    if (!c) return fail(FHS_ERR_INVALID, "debug_fail_alloc: null context");
    Guard g(c);
    if (was_armed) *was_armed = c->debug_fail_alloc >= 0;
    c->debug_fail_alloc = nth < 0 ? -1 : nth;
    return FHS_OK;
}
extern "C" fhs_status fhs_debug_alloc_stats(fhs_context* c, uint64_t* out, int n) {
    if (!c || !out || n < 0) return fail(FHS_ERR_INVALID, "debug_alloc_stats: bad args");
    Guard g(c);
    const uint64_t v[FHS_ALLOC_STATS_COUNT] = {c->cached_bytes,    c->cache_cap,     c->evicted_blocks, c->fit_hits,
                                               c->seal_corr_bytes, c->seal_corr_cap, c->seal_corr_drops};
    for (int i = 0; i < n && i < FHS_ALLOC_STATS_COUNT; ++i) out[i] = v[i];
    return FHS_OK;
}
extern "C" fhs_status fhs_debug_launch_ledger(int op, char* buf, uint64_t len, uint64_t* needed) {
    if (op == FHS_LEDGER_ARM || op == FHS_LEDGER_DISARM) {
        fhs::ledger_arm(op == FHS_LEDGER_ARM);
        return FHS_OK;
    }
    if (op != FHS_LEDGER_READ) return fail(FHS_ERR_INVALID, "debug_launch_ledger: unknown operation");
    const std::string names = fhs::ledger_read();
    if (needed) *needed = names.size() + 1;
    if (!buf || len < names.size() + 1) return fail(FHS_ERR_INVALID, "debug_launch_ledger: buffer too short");
    memcpy(buf, names.c_str(), names.size() + 1);
    return FHS_OK;
}
extern "C" fhs_status fhs_ciphertext_device_ptr(const fhs_ciphertext* ct, void** dptr, uint64_t* bytes) {
    if (!ct || !dptr) return fail(FHS_ERR_INVALID, "null argument");
    fhs_context* c = ct->ctx;
    Guard g(c);
    fhs_status s = flush(c);
    if (s != FHS_OK) return s;
    LIVE(ct);
    *dptr = ct->d;
    if (bytes) *bytes = ct_bytes(ct);
    return FHS_OK;
}

// ============================================================================ encoder
// slots z_j sit at the evaluation point zeta^(5^j); encode solves m(zeta^(5^j)) = scale z_j with
// a length-N complex DFT over the odd exponents (pb:141-149).
// Forward N-point complex FFT for decode (the only user): iterative radix-2, products written out
// as (ac - bd, ad + bc) so no __muldc3 call (std::complex's NaN-recovering multiply) is made.
static void fft_inplace(std::vector<std::complex<double>>& a, const std::vector<std::complex<double>>& w, int logN,
                        size_t wstride = 1) {
    const size_t n = a.size();
    for (size_t i = 0; i < n; ++i) {
        const size_t r = h_bitrev((uint32_t)i, logN);
        if (r > i) std::swap(a[i], a[r]);
    }
    double* x = reinterpret_cast<double*>(a.data());
    const double* wt = reinterpret_cast<const double*>(w.data());
    for (size_t len = 2; len <= n; len <<= 1) {
        const size_t step = n / len * wstride, h = len / 2;
        for (size_t i = 0; i < n; i += len) {
            for (size_t k = 0; k < h; ++k) {
                const double wr = wt[2 * k * step], wi = wt[2 * k * step + 1];
                double* u = x + 2 * (i + k);
                double* v = x + 2 * (i + k + h);
                const double vr = v[0] * wr - v[1] * wi, vi = v[0] * wi + v[1] * wr;
                v[0] = u[0] - vr;
                v[1] = u[1] - vi;
                u[0] += vr;
                u[1] += vi;
            }
        }
    }
}

// values: count vectors of n complex (re,im) (or real when is_real); produces rounded coefficients

// The encoder's periodic-row detection (fhs_kernels.hip k_enc_period): tl = a scratch of one byte per row, left empty
// when no row can take the sparse form (fewer values than slots, a ring below 512, FHESPEAR_ENCODE_DENSE=1)
static hipError_t enc_periods(fhs_context* c, const double* dvals, size_t cnt, size_t n, size_t stride, bool is_real,
                              DevTmp& tl) {
    static const bool dense = getenv("FHESPEAR_ENCODE_DENSE") != nullptr;
    const int smax = fhs::encode_sparse_max_log(c->logN);
    if (dense || smax < 1 || n != c->N / 2 || cnt == 0) return hipSuccess;
    hipError_t e = tl.alloc((cnt + 7) & ~(size_t)7);
    if (e != hipSuccess) return e;
    return fhs::launch_enc_period(dvals, (int)cnt, n, stride, is_real, smax, tl.as<unsigned char>(), c->st);
}
// Encode `cnt` value rows already in HBM (row v at dvals + v * stride doubles) into new plaintexts.
// A batch of >= 32 rows (diagonal batches, not a client's few vectors) whose every row is periodic (tlog >= 1, read
// back after k_enc_period: one wait per batch) is stored compact only, at the batch's smallest tlog
// (fhs_plaintext::dc): the fused BSGS's Hadamard reads it as it is, every other op through pt_dense.  Otherwise (or
// without room for the compact block, or FHESPEAR_ENCODE_NO_SHADOW=1) the batch is dense.
static fhs_status new_pts_compact(fhs_context* c, size_t count, int ci, double scale, int tlog, fhs_plaintext** outs) {
    const int l = c->L0 + 1 - ci;
    const size_t per = (size_t)l * (c->N >> tlog);
    auto* cs = new PtSlab{nullptr, 8 * count * per, 0};
    hipError_t e = dalloc_fit(c, &cs->base, &cs->bytes);
    if (e != hipSuccess) {
        delete cs;
        return hip_fail(e, "plaintext allocation");
    }
    for (size_t k = 0; k < count; ++k) {
        outs[k] = new fhs_plaintext{c, nullptr, ci, l, scale};
        outs[k]->dc = cs->base + k * per;
        outs[k]->tlog = tlog;
        outs[k]->cslab = cs;
        ++cs->refs;
        ctx_retain(c);
    }
    return FHS_OK;
}
// ss_hint >= 0: the caller knows every row is periodic at tlog >= ss_hint (encode_diag_rows' tiled rows), so the
// compact factor needs no read-back of the periods (no host wait); -1: read them back.  rows_known: every row's
// tlog IS ss_hint >= 1 and only its first (N/2) >> ss_hint values are in HBM (stride apart): no detection either.
static fhs_status encode_rows_dev(fhs_context* c, const double* dvals, size_t cnt, size_t n, size_t stride,
                                  bool is_real, double scale, int ci, fhs_plaintext** outs, int ss_hint = -1,
                                  bool rows_known = false) {
    const int l = c->L0 + 1 - ci;
    if (l < 1) return fail(FHS_ERR_LEVEL, "chain index out of range");
    // fused reduction + NTT through a scratch of rounded coefficients (FHESPEAR_ENCODE_UNFUSED=1: the
    // encoder reduces into every limb and the NTT runs in place -- same limbs, A/B and test knob)
    static const bool unfused = getenv("FHESPEAR_ENCODE_UNFUSED") != nullptr;
    static const bool no_shadow = getenv("FHESPEAR_ENCODE_NO_SHADOW") != nullptr;
    DevTmp coef(c), tl(c);
    if (!unfused) HIPCHK(coef.alloc(8 * cnt * c->N), "encode");
    if (rows_known) {
        HIPCHK(tl.alloc((cnt + 7) & ~(size_t)7), "encode");
        HIPCHK(hipMemsetAsync(tl.p, ss_hint, cnt, c->st), "encode");
    } else {
        HIPCHK(enc_periods(c, dvals, cnt, n, stride, is_real, tl), "encode");
    }
    int ss = 0;
    if (tl.p && coef.p && !no_shadow && c->T.max_qbits <= 59 && cnt >= 32) {
        ss = ss_hint;
        if (ss_hint < 0) {
            std::vector<unsigned char> th(cnt);
            HIPCHK(hipMemcpyAsync(th.data(), tl.p, cnt, hipMemcpyDeviceToHost, c->st), "encode");
            HIPCHK(hipStreamSynchronize(c->st), "encode");
            ss = *std::min_element(th.begin(), th.end());
        }
    }
    if (ss > 0 && new_pts_compact(c, cnt, ci, scale, ss, outs) != FHS_OK) {
        (void)hipGetLastError();   // no room for the compact block: a dense batch
        ss = 0;
    }
    if (ss == 0) {
        const fhs_status s0 = new_pts(c, cnt, ci, scale, outs);
        if (s0 != FHS_OK) return s0;
    }
    std::vector<uint64_t*> ptrs(2 * cnt, nullptr);
    for (size_t v = 0; v < cnt; ++v) {
        ptrs[v] = outs[v]->d;   // null for a compact batch
        ptrs[cnt + v] = outs[v]->dc;
    }
    uint64_t* dptrs = nullptr;
    HIPCHK(scratch(c, fhs_context::SCR_ENC_PTRS, 16 * cnt, &dptrs), "encode");
    HIPCHK(stage_h2d(c, dptrs, ptrs.data(), 16 * cnt), "encode");
    HIPCHK(fhs::launch_encode(c->T, dvals, (int)cnt, n, stride, is_real, scale, reinterpret_cast<fhs::u64* const*>(dptrs),
                              l, c->st, coef.as<double>(), tl.as<const unsigned char>(),
                              ss ? reinterpret_cast<fhs::u64* const*>(dptrs + cnt) : nullptr, ss), "encode");
    return FHS_OK;
}
static fhs_status encode_checks(fhs_context* c, size_t n, double scale, int ci) {
    if (n > c->N / 2) return fail(FHS_ERR_INVALID, "encode: more values than slots");
    if (!(scale > 0) || !std::isfinite(scale)) return fail(FHS_ERR_INVALID, "encode: bad scale");
    const int l = c->L0 + 1 - ci;
    if (ci < 1 || l < 1) return fail(FHS_ERR_LEVEL, "encode: chain index out of range");
    return FHS_OK;
}
static fhs_status encode_many(fhs_context* c, const double* vals, size_t count, size_t n, bool is_real, double scale,
                              int ci, fhs_plaintext** outs) {
    fhs_status st = encode_checks(c, n, scale, ci);
    if (st != FHS_OK) return st;
    if (count == 0) return FHS_OK;
    BatchOut bo(outs, count);
    const size_t stride = is_real ? n : 2 * n;
    // values -> HBM (the copy completes before returning: the caller's buffer may be reused), then
    // FFT + exact reduction + NTT on the GPU (k_encode, k_ntt_fwd_ptrs), stream-ordered
    const size_t chunk = 4096;
    HostTrace ht;
    for (size_t base = 0; base < count; base += chunk) {
        const size_t cnt = std::min(chunk, count - base);
        DevTmp dvals(c);
        HIPCHK(dvals.alloc(8 * cnt * stride), "encode staging");
        // stage_h2d: through the pinned ring, no host wait, when it fits a segment (a client batch of a few
        // vectors), else a copy + synchronisation
        if (stride) HIPCHK(stage_h2d(c, dvals.p, vals + base * stride, 8 * cnt * stride), "encode upload");
        ht.mark("encode: upload");
        fhs_status s = encode_rows_dev(c, dvals.as<const double>(), cnt, n, stride, is_real, scale, ci, outs + base);
        ht.mark("encode: objects+launch");
        if (ht.on) { hipStreamSynchronize(c->st); ht.mark("encode: gpu"); }
        if (s != FHS_OK) return s;
    }
    return bo.keep(FHS_OK);
}

// Extension (no reference symbol): the whole caller-side diagonal pipeline of bg:198-203 +
// bg:361-432 on the device -- upload the D x D matrix once (D^2 doubles instead of D x slots),
// gather the rolled, tiled diagonal rows in HBM, encode them.  Values identical to
// encode_*_vector_batch on the host-prepared rows, hence identical limbs.
// The encoder behind encode_matrix_diagonals: diagonal rows `rows[0..nrows)` (indices into 0..D-1, any
// order) of the D x D view, giant group g rolled by g G, tiled, encoded -- out[k] is row rows[k].  Runs
// of consecutive indices are gathered by one launch each (a sharded matvec's rank needs a contiguous
// range of giant groups, or on a grid the same baby share of every group of its column).
static fhs_status encode_diag_rows(fhs_context* c, const double* M1, const double* M2, int64_t ld, int trans, int D,
                                   int G, double scale, int ci, const int* rows, int nrows, fhs_plaintext** out) {
    if (!M1 || !out || (nrows > 0 && !rows)) return fail(FHS_ERR_INVALID, "encode_diagonals: null argument");
    if (D < 1 || G < 1 || G > D) return fail(FHS_ERR_INVALID, "encode_diagonals: need 1 <= G <= D");
    if (ld < D) return fail(FHS_ERR_INVALID, "encode_diagonals: leading dimension below D");
    for (int k = 0; k < nrows; ++k)
        if (rows[k] < 0 || rows[k] >= D) return fail(FHS_ERR_INVALID, "encode_diagonals: row index out of range");
    const size_t n = c->N / 2;
    if ((size_t)D > n) return fail(FHS_ERR_INVALID, "encode_diagonals: dimension larger than the slot count");
    fhs_status st = encode_checks(c, n, scale, ci);
    if (st != FHS_OK) return st;
    const bool is_real = M2 == nullptr;
    BatchOut bo(out, (size_t)nrows);
    const size_t mb = 8ull * D * D;
    DevTmp dm(c);
    HIPCHK(dm.alloc(mb * (is_real ? 1 : 2)), "encode_diagonals matrix");
    // D rows of D doubles, `ld` apart on the host, packed on the device (no host-side copy of a view)
    const double* m1 = dm.as<const double>();
    const double* m2 = is_real ? nullptr : m1 + (size_t)D * D;
    HIPCHK(hipMemcpy2DAsync(dm.p, 8ull * D, M1, 8ull * ld, 8ull * D, D, hipMemcpyHostToDevice, c->st), "encode_diagonals");
    if (!is_real)
        HIPCHK(hipMemcpy2DAsync(dm.p + (size_t)D * D, 8ull * D, M2, 8ull * ld, 8ull * D, D, hipMemcpyHostToDevice, c->st),
               "encode_diagonals");
    HIPCHK(hipStreamSynchronize(c->st), "encode_diagonals");   // caller's buffers may be reused on return
    // the gathered rows repeat with period D (slot j reads column j mod D): periodic at t = n / D when that is a power
    // of two, so the compact factor is known without reading the detected periods back
    int ss_hint = 0;
    if (n % (size_t)D == 0 && ((n / D) & (n / D - 1)) == 0)
        ss_hint = std::min(__builtin_ctzll((unsigned long long)(n / D)), fhs::encode_sparse_max_log(c->logN));
    // The sparse encoder reads only each row's first (N/2) >> ss_hint values, so with ss_hint >= 1 only those are
    // gathered (a whole number of periods) and the periods are not detected: every row takes tlog = ss_hint -- the
    // largest power-of-two period the detector would find in a row of period D (one with a smaller period, e.g. a
    // constant diagonal, keeps the same factor; its encoding is the same polynomial up to the FFT's rounding).
    // FHESPEAR_ENCODE_DENSE=1 / FHESPEAR_ENCODE_UNFUSED=1 keep the full rows and the detector.
    static const bool full_rows = getenv("FHESPEAR_ENCODE_DENSE") || getenv("FHESPEAR_ENCODE_UNFUSED");
    const bool known = ss_hint >= 1 && !full_rows;
    const size_t ng = known ? n >> ss_hint : n, gstride = is_real ? ng : 2 * ng;
    const size_t chunk = 2048;
    for (size_t base = 0; base < (size_t)nrows; base += chunk) {
        const size_t cnt = std::min(chunk, (size_t)nrows - base);
        DevTmp dvals(c);
        HIPCHK(dvals.alloc(8 * cnt * gstride), "encode_diagonals");
        for (size_t k = 0; k < cnt;) {   // one gather per run of consecutive rows
            size_t r = 1;
            while (k + r < cnt && rows[base + k + r] == rows[base + k] + (int)r) ++r;
            HIPCHK(fhs::launch_diag_gather(m1, m2, D, G, (int)ng, rows[base + k], (int)r, trans ? 1 : 0,
                                           dvals.as<double>() + k * gstride, c->st), "encode_diagonals");
            k += r;
        }
        st = encode_rows_dev(c, dvals.as<const double>(), cnt, n, gstride, is_real, scale, ci, out + base, ss_hint, known);
        if (st != FHS_OK) return st;
    }
    return bo.keep(FHS_OK);
}
extern "C" fhs_status fhs_encode_diagonals_ex(fhs_context* c, const double* M1, const double* M2, int64_t ld, int trans,
                                              int D, int G, double scale, int ci, fhs_plaintext** out) {
    ENTER(c);
    std::vector<int> rows(D > 0 ? D : 0);
    for (int k = 0; k < (int)rows.size(); ++k) rows[k] = k;
    return encode_diag_rows(c, M1, M2, ld, trans, D, G, scale, ci, rows.data(), (int)rows.size(), out);
}
extern "C" fhs_status fhs_encode_diagonals_rows(fhs_context* c, const double* M1, const double* M2, int64_t ld,
                                                int trans, int D, int G, double scale, int ci, const int* rows,
                                                int nrows, fhs_plaintext** out) {
    ENTER(c);
    return encode_diag_rows(c, M1, M2, ld, trans, D, G, scale, ci, rows, nrows, out);
}
extern "C" fhs_status fhs_encode_diagonals(fhs_context* c, const double* M1, const double* M2, int D, int G,
                                           double scale, int ci, fhs_plaintext** out) {
    return fhs_encode_diagonals_ex(c, M1, M2, D, 0, D, G, scale, ci, out);
}

// Extended-precision encoder for constant plaintexts (bootstrapping transforms): the f64 FFT of
// the GPU encoder has relative error ~2^-52 log n, i.e. hundreds of integer units at scale 2^59,
// which CoeffToSlot multiplies by |I| ~ K (DESIGN.md §3 bootstrapping).  Here the N/2-point DFT
// runs on the host in x87 long double (64-bit mantissa), each coefficient is rounded exactly to a
// 128-bit integer (hi, lo), and the device reduces it mod every limb and runs the NTT.
static void encode_precise_rows(const fhs_context* c, const double* vals, size_t n_in, size_t r0, size_t r1,
                                long double scale, int64_t* hi, uint64_t* lo, std::atomic<int>* overflow) {
    typedef std::complex<long double> cl;
    const size_t N = c->N, n = N / 2;
    int logn = 0;
    while (((size_t)1 << logn) < n) ++logn;
    const long double pi = acosl(-1.0L);
    std::vector<cl> w(n / 2), tw(n), a(n);
    for (size_t t = 0; t < n / 2; ++t) w[t] = cl(cosl(2 * pi * t / n), -sinl(2 * pi * t / n));   // omega^-t
    for (size_t k = 0; k < n; ++k)                                                              // (2/N) zeta^-k
        tw[k] = cl(cosl(pi * k / N), -sinl(pi * k / N)) * (2.0L / (long double)N);
    const long double two64 = 18446744073709551616.0L;
    for (size_t r = r0; r < r1; ++r) {
        std::fill(a.begin(), a.end(), cl(0, 0));
        for (size_t j = 0; j < n_in; ++j) {                       // Z[s_j] = z_j, 5^j = 4 s_j + 1
            const size_t s = (size_t)(c->slot_index[j] >> 1);
            a[h_bitrev((uint32_t)s, logn)] = cl(vals[(r * n_in + j) * 2], vals[(r * n_in + j) * 2 + 1]);
        }
        for (size_t len = 2; len <= n; len <<= 1) {               // DIT, natural-order output
            const size_t step = n / len;
            for (size_t i = 0; i < n; i += len)
                for (size_t k = 0; k < len / 2; ++k) {
                    const cl u = a[i + k], v = a[i + k + len / 2] * w[k * step];
                    a[i + k] = u + v;
                    a[i + k + len / 2] = u - v;
                }
        }
        for (size_t k = 0; k < n; ++k) {
            const cl ck = a[k] * tw[k];
            const long double part[2] = {ck.real() * scale, ck.imag() * scale};
            for (int h = 0; h < 2; ++h) {
                const long double x = roundl(part[h]);
                if (!(fabsl(x) < 0x1p126L)) { overflow->store(1); continue; }
                const long double xh = floorl(x / two64);
                const size_t idx = r * N + k + (size_t)h * n;
                hi[idx] = (int64_t)xh;
                lo[idx] = (uint64_t)(x - xh * two64);
            }
        }
    }
}
extern "C" fhs_status fhs_encode_precise(fhs_context* c, const double* re_im, size_t count, size_t n, double scale,
                                         int ci, fhs_plaintext** outs) {
    ENTER(c);
    if ((!re_im && n) || !outs) return fail(FHS_ERR_INVALID, "encode_precise: null argument");
    if (n > c->N / 2) return fail(FHS_ERR_INVALID, "encode_precise: more values than slots");
    if (!(scale > 0) || !std::isfinite(scale) || scale > 0x1p126) return fail(FHS_ERR_INVALID, "encode_precise: bad scale");
    const int l = c->L0 + 1 - ci;
    if (ci < 1 || l < 1) return fail(FHS_ERR_LEVEL, "encode: chain index out of range");
    if (count == 0) return FHS_OK;
    BatchOut bo(outs, count);
    const size_t N = c->N;
    std::vector<int64_t> hi(count * N);
    std::vector<uint64_t> lo(count * N);
    const size_t nth = std::max<size_t>(1, std::min<size_t>({count, 16, (size_t)std::thread::hardware_concurrency()}));
    std::vector<std::thread> th;
    std::atomic<int> overflow{0};
    for (size_t t = 0; t < nth; ++t)
        th.emplace_back(encode_precise_rows, c, re_im, n, count * t / nth, count * (t + 1) / nth, (long double)scale,
                        hi.data(), lo.data(), &overflow);
    for (auto& x : th) x.join();
    if (overflow.load()) return fail(FHS_ERR_INVALID, "encode_precise: |value x scale| >= 2^126 (or not finite)");
    DevTmp dbuf(c);
    HIPCHK(dbuf.alloc(16 * count * N), "encode_precise staging");
    HIPCHK(hipMemcpyAsync(dbuf.p, hi.data(), 8 * count * N, hipMemcpyHostToDevice, c->st), "encode_precise");
    HIPCHK(hipMemcpyAsync(dbuf.p + count * N, lo.data(), 8 * count * N, hipMemcpyHostToDevice, c->st), "encode_precise");
    HIPCHK(hipStreamSynchronize(c->st), "encode_precise");
    const fhs_status s = new_pts(c, count, ci, scale, outs);
    if (s != FHS_OK) return s;
    std::vector<uint64_t*> ptrs(count);
    for (size_t v = 0; v < count; ++v) ptrs[v] = outs[v]->d;
    uint64_t* dptrs = nullptr;
    HIPCHK(scratch(c, fhs_context::SCR_ENC_PTRS, 8 * count, &dptrs), "encode_precise");
    HIPCHK(stage_h2d(c, dptrs, ptrs.data(), 8 * count), "encode_precise");
    HIPCHK(fhs::launch_encode_int128(c->T, dbuf.as<const int64_t>(), dbuf.p + count * N, (int)count,
                                     reinterpret_cast<fhs::u64* const*>(dptrs), l, c->st), "encode_precise");
    return bo.keep(FHS_OK);
}

extern "C" fhs_status fhs_encode(fhs_context* c, const double* re_im, size_t n, double scale, int ci,
                                 fhs_plaintext** out) {
    ENTER(c);
    if ((!re_im && n) || !out) return fail(FHS_ERR_INVALID, "encode: null argument");
    return encode_many(c, re_im, 1, n, false, scale, ci, out);
}
extern "C" fhs_status fhs_encode_real(fhs_context* c, const double* v, size_t n, double scale, int ci,
                                      fhs_plaintext** out) {
    ENTER(c);
    if ((!v && n) || !out) return fail(FHS_ERR_INVALID, "encode: null argument");
    return encode_many(c, v, 1, n, true, scale, ci, out);
}
extern "C" fhs_status fhs_encode_batch(fhs_context* c, const double* re_im, size_t count, size_t n, double scale,
                                       int ci, fhs_plaintext** out) {
    ENTER(c);
    if (!re_im || !out) return fail(FHS_ERR_INVALID, "encode_batch: null argument");
    return encode_many(c, re_im, count, n, false, scale, ci, out);
}
extern "C" fhs_status fhs_encode_real_batch(fhs_context* c, const double* v, size_t count, size_t n, double scale,
                                            int ci, fhs_plaintext** out) {
    ENTER(c);
    if (!v || !out) return fail(FHS_ERR_INVALID, "encode_batch: null argument");
    return encode_many(c, v, count, n, true, scale, ci, out);
}

// CRT-compose l residues of each coefficient to a centred double (multi-precision, host)
static void crt_compose(const fhs_context* c, const std::vector<uint64_t>& limbs, int l, std::vector<double>& out) {
    const size_t N = c->N;
    const CrtHost C = crt_host_consts(c->q.data(), l);
    const int W = C.W;
    const std::vector<uint64_t>&Q = C.Q, &hat = C.hat, &ihat = C.ihat, &ihat_s = C.ihat_s, &halfQ = C.halfQ;
    out.assign(N, 0.0);
    const unsigned nth = std::max(1u, std::min<unsigned>(std::thread::hardware_concurrency(), l <= 6 ? 8 : 32));
    std::vector<std::thread> th;
    for (unsigned tix = 0; tix < nth; ++tix)
        th.emplace_back([&, tix]() {
            std::vector<uint64_t> x(W + 1);
            for (size_t n = tix; n < N; n += nth) {
                std::fill(x.begin(), x.end(), 0);
                for (int i = 0; i < l; ++i) {
                    // y = limb * ihat mod q by Shoup (ihat_s = floor(ihat 2^64 / q)); limbs are < q
                    const uint64_t a = limbs[(size_t)i * N + n], qi = c->q[i];
                    const uint64_t qh = (uint64_t)(((hu128)a * ihat_s[i]) >> 64);
                    uint64_t y = a * ihat[i] - qh * qi;
                    if (y >= qi) y -= qi;
                    hu128 carry = 0;
                    const uint64_t* h = &hat[(size_t)i * W];
                    for (int w = 0; w < W; ++w) {
                        const hu128 t = (hu128)h[w] * y + x[w] + carry;
                        x[w] = (uint64_t)t;
                        carry = t >> 64;
                    }
                    x[W] += (uint64_t)carry;
                    for (;;) {   // x < 2Q: at most one subtraction
                        bool ge = x[W] != 0;
                        if (!ge) {
                            ge = true;
                            for (int w = W - 1; w >= 0; --w)
                                if (x[w] != Q[w]) { ge = x[w] > Q[w]; break; }
                        }
                        if (!ge) break;
                        uint64_t br = 0;
                        for (int w = 0; w < W; ++w) {
                            const uint64_t qa = Q[w] + br;
                            const uint64_t nb = (qa < br) || (x[w] < qa);
                            x[w] -= qa;
                            br = nb;
                        }
                        x[W] -= br;
                    }
                }
                bool neg = false;
                for (int w = W - 1; w >= 0; --w)
                    if (x[w] != halfQ[w]) { neg = x[w] > halfQ[w]; break; }
                if (neg) {
                    uint64_t br = 0;
                    for (int w = 0; w < W; ++w) {
                        const uint64_t xa = x[w] + br;
                        const uint64_t nb = (xa < br) || (Q[w] < xa);
                        x[w] = Q[w] - xa;
                        br = nb;
                    }
                }
                double v = 0;
                for (int w = W - 1; w >= 0; --w) v = v * 18446744073709551616.0 + (double)x[w];
                out[n] = neg ? -v : v;
            }
        });
    for (auto& t : th) t.join();
}

// Coefficients of a decrypted plaintext are |x| = |m| scale + noise: the centred CRT over the first
// k limbs (prod q_i >= scale 2^72) is the same integer as over all l, hence the same double, whenever
// |x| < Q_k / 2 -- every plaintext whose coefficients are below 2^71 scale, the range CKKS decoding is
// meant for.  The GPU composes k+1 limbs and checks the result against every other limb (it must equal
// the coefficient's residue mod each q_e): all agree exactly when the composition IS the coefficient
// (both lie in (-Q_l/2, Q_l/2) and agree mod Q_l), so any larger coefficient -- which would otherwise
// decode to an aliased value -- is detected and the decoder composes all l limbs instead.
// FHESPEAR_DECODE_FULL=1 always composes all l limbs.
static int decode_limbs(const fhs_context* c, double scale, int l) {
    double bits = 0, need = std::log2(std::max(scale, 1.0)) + 72.0;
    for (int i = 0; i < l; ++i) {
        bits += std::log2((double)c->q[i]);
        if (bits >= need) return i + 1;
    }
    return l;
}
// A/B and test knobs of the decoder, each read here only: FULL composes all l limbs always, HOST_CRT composes on
// the host (crt_compose), HOST_FFT runs the slot FFT on the host (decode_slots); same doubles either way
struct DecodeKnobs {
    bool full, host_crt, host_fft;
};
static const DecodeKnobs& decode_knobs() {
    static const DecodeKnobs k{getenv("FHESPEAR_DECODE_FULL") != nullptr, getenv("FHESPEAR_DECODE_HOST_CRT") != nullptr,
                               getenv("FHESPEAR_DECODE_HOST_FFT") != nullptr};
    return k;
}
// constants of the centred CRT over the first l <= kCrtMaxL limbs, packed for the GPU composition: the words
// crt_compose reads on the host (crt_host_consts)
static void crt_consts(const fhs_context* c, int l, fhs::CrtConsts& K) {
    const CrtHost C = crt_host_consts(c->q.data(), l);
    K = fhs::CrtConsts{};
    K.l = l;
    K.W = C.W;
    std::copy(C.Q.begin(), C.Q.end(), K.Q);
    std::copy(C.halfQ.begin(), C.halfQ.end(), K.halfQ);
    for (int i = 0; i < l; ++i) {
        K.q[i] = c->q[i];
        K.ihat[i] = C.ihat[i];
        K.ihat_s[i] = C.ihat_s[i];
        std::copy(&C.hat[(size_t)i * C.W], &C.hat[(size_t)i * C.W] + C.W, K.hat[i]);
    }
}
// The composition constants of the first kk limbs and the check tables of limbs kk..l-1 ([CrtConsts as
// words][l - kk vtabs of kCrtVtabWords]), built once per (kk, l) and kept in the context: a client decodes
// the same few levels over and over
constexpr size_t kCrtConstWords = sizeof(fhs::CrtConsts) / 8;
static_assert(sizeof(fhs::CrtConsts) % 8 == 0, "CrtConsts packs into words");
static const std::vector<uint64_t>& crt_tables(fhs_context* c, int kk, int l) {
    std::vector<uint64_t>& tab = c->crt_cache[std::make_pair(kk, l)];
    if (!tab.empty()) return tab;
    fhs::CrtConsts K;
    crt_consts(c, kk, K);
    tab.assign(kCrtConstWords + (size_t)(l - kk) * fhs::kCrtVtabWords, 0);
    std::memcpy(tab.data(), &K, sizeof(K));
    for (int x = 0; x < l - kk; ++x)
        crt_check_table(c->q[kk + x], K.W, tab.data() + kCrtConstWords + (size_t)x * fhs::kCrtVtabWords);
    return tab;
}
// Centred coefficients of the first k limbs as doubles: the INTT, then the composition on the GPU up to kCrtMaxL
// limbs, else (or with FHESPEAR_DECODE_HOST_CRT=1) on the host from the limbs -- same arithmetic, same doubles
static fhs_status decode_compose(fhs_context* c, const fhs_plaintext* pt, int k, std::vector<double>& m) {
    const size_t N = c->N, bytes = 8ull * k * N;
    const bool dev = k <= fhs::kCrtMaxL && !decode_knobs().host_crt;
    DevTmp tmp(c), dbl(c);
    HIPCHK(tmp.alloc(bytes), "decode");
    if (dev) HIPCHK(dbl.alloc(8 * N), "decode");
    PT_DENSE(pd, pt, "decode");
    HIPCHK(hipMemcpyAsync(tmp.p, pd, bytes, hipMemcpyDeviceToDevice, c->st), "decode");
    HIPCHK(fhs::launch_ntt_inv(c->T, tmp.p, k, k, 1, 0, c->st), "decode");
    std::vector<uint64_t> host(dev ? 0 : (size_t)k * N);
    m.resize(N);
    if (dev) {
        fhs::CrtConsts K;
        std::memcpy(&K, crt_tables(c, k, k).data(), sizeof(K));
        HIPCHK(fhs::launch_crt_compose(K, tmp.p, dbl.as<double>(), (int)N, c->st), "decode");
        HIPCHK(hipMemcpyAsync(m.data(), dbl.p, 8 * N, hipMemcpyDeviceToHost, c->st), "decode");
    } else {
        HIPCHK(hipMemcpyAsync(host.data(), tmp.p, bytes, hipMemcpyDeviceToHost, c->st), "decode");
    }
    HIPCHK(hipStreamSynchronize(c->st), "decode");
    if (!dev) crt_compose(c, host, k, m);
    return FHS_OK;
}
// slots z_j = m(zeta^(5^j)) = sum_{k < N/2} (m_k + i m_{k+N/2}) zeta^k omega^(s_j k), omega = zeta^4,
// 5^j = 4 s_j + 1: an N/2-point FFT of the twisted half-pairs, read at s_j = slot_index[j] / 2; the first
// `nslots` slots to re_im
static void decode_slots(const fhs_context* c, const double* m, double scale, size_t nslots, double* re_im) {
    const size_t n = c->N / 2;
    std::vector<std::complex<double>> v(n);
    for (size_t k2 = 0; k2 < n; ++k2) {
        const double a = m[k2] / scale, b = m[k2 + n] / scale;
        const double cr = c->dec_twist[k2].real(), ci = c->dec_twist[k2].imag();
        v[k2] = {a * cr - b * ci, a * ci + b * cr};
    }
    fft_inplace(v, c->fft_w, c->logN - 1, 2);
    for (size_t j = 0; j < nslots; ++j) {
        const std::complex<double> z = v[c->slot_index[j] >> 1];
        re_im[2 * j] = z.real();
        re_im[2 * j + 1] = z.imag();
    }
}
static hipError_t readback_buf(fhs_context* c, size_t bytes, double** out) {
    if (bytes > c->readback_bytes) {   // every earlier use ended with a stream synchronisation
        if (c->readback) hipHostFree(c->readback);
        c->readback = nullptr;
        c->readback_bytes = 0;
        const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&c->readback), bytes, hipHostMallocDefault);
        if (e != hipSuccess) return e;
        c->readback_bytes = bytes;
    }
    *out = c->readback;
    return hipSuccess;
}

// What decode_many decodes: plaintexts, or (cts with sk) ciphertexts decrypted straight into the INTT's buffer
// (fhs_decrypt_decode_batch).  Everything that differs between the two is here.
struct DecodeSrc {
    const fhs_plaintext* const* pts = nullptr;
    const fhs_ciphertext* const* cts = nullptr;
    fhs_secret_key* sk = nullptr;
    bool ok() const { return cts ? sk != nullptr : pts != nullptr; }
    bool null_at(int i) const { return cts ? !cts[i] : !pts[i]; }
    fhs_status live(int i) const { return cts ? live_ct(cts[i]) : FHS_OK; }
    int l(int i) const { return cts ? cts[i]->l : pts[i]->l; }
    double scale(int i) const { return cts ? cts[i]->scale : pts[i]->scale; }
    // one launch brings all `count` items (at one level) to coefficient form's buffer: ciphertexts of one component
    // count, through a staged array of their addresses (ptr_words words, written by ptrs)
    bool batched(int count) const {
        for (int i = 0; cts && i < count; ++i)
            if (cts[i]->ncomp != cts[0]->ncomp) return false;
        return cts != nullptr;
    }
    size_t ptr_words(int count) const { return cts ? (size_t)count : 0; }
    void ptrs(int count, uint64_t* w) const {
        for (int i = 0; cts && i < count; ++i) w[i] = reinterpret_cast<uint64_t>(cts[i]->d);
    }
    hipError_t all_to(fhs_context* c, const uint64_t* ptrs_dev, int count, int lv, uint64_t* dst) const {
        return fhs::launch_decrypt_many(c->T, reinterpret_cast<const fhs::u64* const*>(ptrs_dev), count, cts[0]->ncomp,
                                        sk->s, dst, (size_t)lv * c->N, lv, c->st);
    }
    // item i's l(i) limbs (NTT form) to dst: decrypted there, or copied
    hipError_t item_to(fhs_context* c, int i, uint64_t* dst) const {
        if (cts) return fhs::launch_decrypt(c->T, cts[i]->d, cts[i]->ncomp, sk->s, dst, cts[i]->l, c->st);
        const uint64_t* pd = nullptr;
        const hipError_t e = pt_dense(c, pts[i], &pd);
        return e != hipSuccess ? e : hipMemcpyAsync(dst, pd, 8ull * pts[i]->l * c->N, hipMemcpyDeviceToDevice, c->st);
    }
    // item i's coefficients composed exactly from all its limbs (of the decrypted plaintext)
    fhs_status exact(fhs_context* c, int i, std::vector<double>& m) const {
        if (!cts) return decode_compose(c, pts[i], pts[i]->l, m);
        Pt pt;
        const fhs_status s = fhs_decrypt(c, sk, cts[i], &pt.p);
        return s != FHS_OK ? s : decode_compose(c, pt.p, pt->l, m);
    }
};
// Everything decode_many decides before it touches the device.  aux is one device buffer of words: [scales:
// count][check tables (vtab) of the fast items][one fhs::CrtJob per fast item][source pointers][check flags: FW
// words, zeroed][slots]; all of it before the slots is staged from the host in one copy (decode_head), and flags +
// slots come back in one copy to the pinned read-back buffer: [flags: FW words][per_out doubles per item].
constexpr size_t kCrtJobWords = sizeof(fhs::CrtJob) / 8;
static_assert(sizeof(fhs::CrtJob) % 8 == 0, "CrtJob packs into words");
struct DecodePlan {
    int count = 0, nslots = 0;
    bool host_fft = false;
    std::vector<int> kk;                   // limbs item i composes: what its scale needs + 1, at most its level
    std::vector<char> fast;                // item i composes kk[i] < l limbs on the GPU, checked against the rest
    std::vector<size_t> tmp_at, vtab_at;   // fast item i: its limbs in tmp, its check tables in aux (words)
    int nf = 0, lf = -1, max_nx = 0;       // the fast items: how many, their (last) level, the most check limbs
    bool one_l = true;                     // the fast items share level lf: one INTT launch over all of them
    size_t tmp_words = 0;                  // the fast items' limbs side by side
    size_t jobs0 = 0, ptrs0 = 0, flags0 = 0, FW = 0, slot_words = 0, aux_words = 0;
    size_t per_out = 0;                    // doubles back per item: its slots, or (host FFT) its N coefficients
};
static bool decode_plan(const fhs_context* c, const DecodeSrc& src, int count, int nslots, DecodePlan& P) {
    const DecodeKnobs& knob = decode_knobs();
    const size_t N = c->N;
    P.count = count;
    P.nslots = nslots;
    P.host_fft = knob.host_fft;
    P.kk.assign(count, 0);
    P.fast.assign(count, 0);
    P.tmp_at = P.vtab_at = std::vector<size_t>(count, 0);
    size_t vtab_end = (size_t)count;   // the check tables follow the scales
    for (int i = 0; i < count; ++i) {
        if (src.null_at(i)) return false;
        const int l = src.l(i), k = knob.full ? l : decode_limbs(c, src.scale(i), l);
        P.kk[i] = std::min(l, k + 1);
        P.fast[i] = P.kk[i] < l && P.kk[i] <= fhs::kCrtMaxL && !knob.host_crt;
        if (!P.fast[i]) continue;
        P.one_l &= P.lf < 0 || l == P.lf;
        P.lf = l;
        P.max_nx = std::max(P.max_nx, l - P.kk[i]);
        P.tmp_at[i] = P.tmp_words;
        P.vtab_at[i] = vtab_end;
        P.tmp_words += (size_t)l * N;
        vtab_end += (size_t)(l - P.kk[i]) * fhs::kCrtVtabWords;
        ++P.nf;
    }
    P.jobs0 = vtab_end;
    P.ptrs0 = P.jobs0 + (size_t)P.nf * kCrtJobWords;
    P.flags0 = P.ptrs0 + src.ptr_words(count);
    P.FW = ((size_t)count + 1) / 2;
    P.slot_words = P.host_fft ? 0 : 2 * (size_t)nslots * count;
    P.aux_words = P.flags0 + P.FW + P.slot_words;
    P.per_out = P.host_fft ? N : 2 * (size_t)nslots;
    return true;
}
// The device and pinned buffers of one decode_many call, and the plan's regions of them
struct DecodeBufs {
    DevTmp tmp, dbl, aux, spec;   // limbs of the fast items; count x N coefficients; see DecodePlan; FFT scratch
    double* rb = nullptr;         // the context's pinned read-back buffer
    explicit DecodeBufs(fhs_context* c) : tmp(c), dbl(c), aux(c), spec(c) {}
    const double* scales() const { return aux.as<double>(); }
    unsigned* flags(const DecodePlan& P) const { return reinterpret_cast<unsigned*>(aux.p + P.flags0); }
    double* slots(const DecodePlan& P) const { return reinterpret_cast<double*>(aux.p + P.flags0 + P.FW); }
    double* rb_item(const DecodePlan& P, int i) const { return rb + P.FW + (size_t)i * P.per_out; }
};
// The host image of aux up to the slots, once the buffers exist: the jobs point into them
static std::vector<uint64_t> decode_head(fhs_context* c, const DecodeSrc& src, const DecodePlan& P, const DecodeBufs& B) {
    std::vector<uint64_t> head(P.flags0 + P.FW, 0);
    size_t job = P.jobs0;
    for (int i = 0; i < P.count; ++i) {
        const double sc = src.scale(i);
        std::memcpy(&head[i], &sc, 8);
        if (!P.fast[i]) continue;
        const int kk = P.kk[i], nx = src.l(i) - kk;
        const std::vector<uint64_t>& tab = crt_tables(c, kk, src.l(i));   // [CrtConsts][nx vtabs], cached per (kk, l)
        fhs::CrtJob J{};
        std::memcpy(&J.K, tab.data(), sizeof(fhs::CrtConsts));
        std::memcpy(&head[P.vtab_at[i]], tab.data() + kCrtConstWords, 8 * (size_t)nx * fhs::kCrtVtabWords);
        J.limbs = B.tmp.p + P.tmp_at[i];
        J.out = B.dbl.as<double>() + (size_t)i * c->N;
        J.extra = J.limbs + (size_t)kk * c->N;
        J.vtab = B.aux.p + P.vtab_at[i];
        J.flag = B.flags(P) + i;
        J.nx = nx;
        std::memcpy(&head[job], &J, sizeof(J));
        job += kCrtJobWords;
    }
    src.ptrs(P.count, &head[P.ptrs0]);
    return head;
}
// Allocate, stage, bring the fast items to coefficient form (side by side: one INTT launch over all of them when
// they share a level -- the usual client batch -- else one per item), compose and check them, the slot FFT over
// every item (a slow one's slots are recomputed by decode_exact_item), one copy back, ONE synchronisation.
static fhs_status decode_enqueue(fhs_context* c, const DecodeSrc& src, const DecodePlan& P, DecodeBufs& B,
                                 HostTrace& ht) {
    const size_t N = c->N;
    const int count = P.count;
    HIPCHK(readback_buf(c, 8 * (P.FW + P.per_out * count), &B.rb), "decode");
    if (P.tmp_words) HIPCHK(B.tmp.alloc(8 * P.tmp_words), "decode");
    HIPCHK(B.dbl.alloc(8 * N * count), "decode");
    HIPCHK(B.aux.alloc(8 * P.aux_words), "decode");
    if (!P.host_fft) HIPCHK(B.spec.alloc(16 * (N / 2) * count), "decode");
    const std::vector<uint64_t> head = decode_head(c, src, P, B);
    HIPCHK(stage_h2d(c, B.aux.p, head.data(), 8 * head.size()), "decode");
    if (P.nf == count && P.one_l && src.batched(count)) {
        HIPCHK(src.all_to(c, B.aux.p + P.ptrs0, count, P.lf, B.tmp.p), "decode");
    } else {
        for (int i = 0; i < count; ++i) {
            if (!P.fast[i]) continue;
            HIPCHK(src.item_to(c, i, B.tmp.p + P.tmp_at[i]), "decode");
            if (!P.one_l) HIPCHK(fhs::launch_ntt_inv(c->T, B.tmp.p + P.tmp_at[i], src.l(i), src.l(i), 1, 0, c->st), "decode");
        }
    }
    if (P.nf > 0 && P.one_l) HIPCHK(fhs::launch_ntt_inv(c->T, B.tmp.p, P.lf, P.lf, P.nf, (size_t)P.lf * N, c->st), "decode");
    if (P.nf > 0)
        HIPCHK(fhs::launch_crt_compose_jobs(reinterpret_cast<const fhs::CrtJob*>(B.aux.p + P.jobs0), P.nf, P.max_nx, (int)N,
                                            c->st), "decode");
    if (!P.host_fft)
        HIPCHK(fhs::launch_decode_slots(c->T, B.dbl.as<double>(), B.scales(), count, B.spec.as<double>(), P.nslots,
                                        B.slots(P), c->st), "decode");
    HIPCHK(hipMemcpyAsync(B.rb, B.flags(P), 8 * (P.FW + P.slot_words), hipMemcpyDeviceToHost, c->st), "decode");
    if (P.host_fft)
        HIPCHK(hipMemcpyAsync(B.rb_item(P, 0), B.dbl.p, 8 * P.per_out * count, hipMemcpyDeviceToHost, c->st), "decode");
    ht.mark("decode: enqueue");
    HIPCHK(hipStreamSynchronize(c->st), "decode");
    ht.mark("decode: gpu");
    return FHS_OK;
}
// Item i again, composed exactly from all its limbs (its check failed: an aliased coefficient; or it needs more
// limbs than the GPU composition takes): its coefficients (host FFT) or slots replace the fast path's in rb
static fhs_status decode_exact_item(fhs_context* c, const DecodeSrc& src, const DecodePlan& P, DecodeBufs& B, int i) {
    std::vector<double> m;
    const fhs_status st = src.exact(c, i, m);
    if (st != FHS_OK) return st;
    if (P.host_fft) {
        std::copy(m.begin(), m.end(), B.rb_item(P, i));
        return FHS_OK;
    }
    double* di = B.dbl.as<double>() + (size_t)i * c->N;
    HIPCHK(hipMemcpyAsync(di, m.data(), 8 * c->N, hipMemcpyHostToDevice, c->st), "decode");
    HIPCHK(fhs::launch_decode_slots(c->T, di, B.scales() + i, 1, B.spec.as<double>(), P.nslots, B.slots(P), c->st),
           "decode");
    HIPCHK(hipMemcpyAsync(B.rb_item(P, i), B.slots(P), 8 * P.per_out, hipMemcpyDeviceToHost, c->st), "decode");
    HIPCHK(hipStreamSynchronize(c->st), "decode");
    return FHS_OK;
}
// Decode `count` items to their first `nslots` slots (re_im: count x nslots x (re, im)), all on the GPU: per item
// the INTT, the centred CRT composition of the limbs the scale needs (+1) and the check against the rest; then one
// k_decode_fft + gather over all of them; only the slots come back, through the pinned read-back buffer, after ONE
// synchronisation.  An item whose check fails or that needs more limbs than the GPU composition takes is composed
// exactly and decoded on its own (decode_exact_item).  FHESPEAR_DECODE_HOST_FFT=1 runs the slot FFT on the host
// instead (decode_slots: the same operations, so the same doubles).
static fhs_status decode_many(fhs_context* c, const DecodeSrc& src, int count, int nslots, double* re_im) {
    if (!src.ok() || !re_im || count < 0 || nslots < 1 || (size_t)nslots > c->N / 2)
        return fail(FHS_ERR_INVALID, "decode: bad arguments");
    for (int i = 0; i < count; ++i) {
        const fhs_status s = src.live(i);
        if (s != FHS_OK) return s;
    }
    if (count == 0) return FHS_OK;
    DecodePlan P;
    if (!decode_plan(c, src, count, nslots, P)) return fail(FHS_ERR_INVALID, "decode: null plaintext or ciphertext");
    HostTrace ht;
    DecodeBufs B(c);
    fhs_status st = decode_enqueue(c, src, P, B, ht);
    if (st != FHS_OK) return st;
    const unsigned* hflag = reinterpret_cast<const unsigned*>(B.rb);
    for (int i = 0; i < count; ++i) {
        if (P.fast[i] && hflag[i] == 0) continue;
        if ((st = decode_exact_item(c, src, P, B, i)) != FHS_OK) return st;
    }
    for (int i = 0; i < count; ++i) {
        double* out = re_im + (size_t)i * 2 * nslots;
        if (P.host_fft)
            decode_slots(c, B.rb_item(P, i), src.scale(i), (size_t)nslots, out);
        else
            std::memcpy(out, B.rb_item(P, i), 8 * P.per_out);
    }
    ht.mark("decode: slots");
    return FHS_OK;
}
extern "C" fhs_status fhs_decode(fhs_context* c, const fhs_plaintext* pt, double* re_im) {
    ENTER(c);
    if (!pt || !re_im) return fail(FHS_ERR_INVALID, "decode: null argument");
    return decode_many(c, DecodeSrc{&pt}, 1, (int)(c->N / 2), re_im);
}
extern "C" fhs_status fhs_decrypt_decode_batch(fhs_context* c, fhs_secret_key* sk, const fhs_ciphertext* const* cts,
                                               int count, int nslots, double* re_im) {
    ENTER(c);
    if (!sk || !cts || !re_im || count < 0 || nslots < 1 || (size_t)nslots > c->N / 2)
        return fail(FHS_ERR_INVALID, "decrypt_decode_batch: bad arguments");
    for (int i0 = 0; i0 < count; i0 += kMaxBatch) {   // grid rows and scratch bound one launch
        const fhs_status s = decode_many(c, DecodeSrc{nullptr, cts + i0, sk}, std::min(kMaxBatch, count - i0), nslots,
                                         re_im + (size_t)i0 * 2 * nslots);
        if (s != FHS_OK) return s;
    }
    return FHS_OK;
}
// Client-side batch (the client-aided block decrypts 2-3 outputs per stage): decode_many over all of
// them, one synchronisation, only the first `nslots` slots of each back to the host.
extern "C" fhs_status fhs_decode_batch(fhs_context* c, const fhs_plaintext* const* pts, int count, int nslots,
                                       double* re_im) {
    ENTER(c);
    if (!pts || !re_im || count < 0 || nslots < 1 || (size_t)nslots > c->N / 2)
        return fail(FHS_ERR_INVALID, "decode_batch: bad arguments");
    for (int i0 = 0; i0 < count; i0 += kMaxBatch) {
        const fhs_status s = decode_many(c, DecodeSrc{pts + i0}, std::min(kMaxBatch, count - i0), nslots,
                                         re_im + (size_t)i0 * 2 * nslots);
        if (s != FHS_OK) return s;
    }
    return FHS_OK;
}

// ============================================================================ encryption
extern "C" fhs_status fhs_encrypt_symmetric(fhs_context* c, fhs_secret_key* sk, const fhs_plaintext* pt,
                                            fhs_ciphertext** out) {
    ENTER(c);
    if (!sk || !pt || !out) return fail(FHS_ERR_INVALID, "encrypt: null argument");
    const uint64_t ctr = sk->ctr++;
    NEW_CT(ct, 2, pt->ci, pt->scale);
    const int l = pt->l;
    const size_t S = (size_t)l * c->N;
    DevTmp eb(c);
    HIPCHK(eb.alloc(8 * S), "encrypt");
    HIPCHK(fhs::launch_sample(c->T, fhs::SAMPLE_UNIFORM, sk->key, stream_id(ST_ENC_SYM, ctr, 0), ct->d + S, l, c->st), "encrypt");
    HIPCHK(sample_small_ntt(c, fhs::SAMPLE_CBD, sk->key, stream_id(ST_ENC_SYM, ctr, 1), eb.p, l), "encrypt");
    PT_DENSE(pd, pt, "encrypt");
    HIPCHK(fhs::launch_encrypt_combine(c->T, 0, ct->d, ct->d + S, sk->s, nullptr, nullptr, eb.p, nullptr, pd, l, c->st),
           "encrypt");
    *out = ct.release();
    return FHS_OK;
}
// `count` symmetric encryptions at l limbs into new ciphertexts outs[i] (chain index ci, scale scales[i]):
// of the plaintexts pts[i], or (pts null) of the rounded message coefficients `coef` already in HBM
// (count x N doubles, launch_encode_coef) -- encode and encrypt fused.  Counters as `count` calls.
static fhs_status encrypt_sym_core(fhs_context* c, fhs_secret_key* sk, int count, int l, int ci, const double* scales,
                                   const fhs_plaintext* const* pts, const double* coef, fhs_ciphertext** outs) {
    BatchOutT<fhs_ciphertext> bo(outs, count);
    const size_t S = (size_t)l * c->N;
    for (int i = 0; i < count; ++i) {
        fhs_status s = new_ct(c, 2, ci, scales[i], &outs[i]);
        if (s != FHS_OK) return s;
    }
    const uint64_t ctr0 = sk->ctr;
    sk->ctr += (uint64_t)count;
    const uint64_t step = stream_id(0, 1, 0);   // consecutive counters: stream ids 2^16 apart
    std::vector<uint64_t*> ptrs(2 * (size_t)count, nullptr);
    for (int i = 0; i < count; ++i) {
        ptrs[i] = outs[i]->d;
        if (pts) {
            const uint64_t* pd = nullptr;
            HIPCHK(pt_dense(c, pts[i], &pd), "encrypt");
            ptrs[count + i] = const_cast<uint64_t*>(pd);
        }
    }
    DevTmp eb(c), dptrs(c), small(c);
    HIPCHK(eb.alloc(8 * S * count), "encrypt");
    HIPCHK(dptrs.alloc(16 * (size_t)count), "encrypt");
    HIPCHK(small.alloc(((size_t)c->N * count + 7) & ~(size_t)7), "encrypt");
    HIPCHK(stage_h2d(c, dptrs.p, ptrs.data(), 16 * (size_t)count), "encrypt");
    HIPCHK(fhs::launch_encrypt_sym_batch(c->T, sk->key, stream_id(ST_ENC_SYM, ctr0, 0), stream_id(ST_ENC_SYM, ctr0, 1),
                                         step, dptrs.as<fhs::u64* const>(), sk->s,
                                         pts ? reinterpret_cast<const fhs::u64* const*>(dptrs.p + count) : nullptr,
                                         count, l, small.as<signed char>(), eb.p, c->st, coef), "encrypt");
    return bo.keep(FHS_OK);
}
extern "C" fhs_status fhs_encrypt_symmetric_batch(fhs_context* c, fhs_secret_key* sk, const fhs_plaintext* const* pts,
                                                  int count, fhs_ciphertext** outs) {
    ENTER(c);
    if (!sk || !pts || !outs || count < 0) return fail(FHS_ERR_INVALID, "encrypt_batch: bad arguments");
    for (int i = 0; i < count; ++i)
        if (!pts[i]) return fail(FHS_ERR_INVALID, "encrypt_batch: null plaintext");
    bool same = count > 0;
    for (int i = 1; i < count; ++i) same &= pts[i]->l == pts[0]->l && pts[i]->ci == pts[0]->ci;
    if (!same) {   // mixed levels: one at a time (the same counters in the same order); a failure destroys
                   // the ciphertexts already made, as the batched path does
        BatchOutT<fhs_ciphertext> bo(outs, count);
        for (int i = 0; i < count; ++i) {
            const fhs_status s = fhs_encrypt_symmetric(c, sk, pts[i], &outs[i]);
            if (s != FHS_OK) return s;
        }
        return bo.keep(FHS_OK);
    }
    // chunks of kMaxBatch (grid rows and scratch bound the launch); counters stay consecutive, so the
    // ciphertexts are those of one call per plaintext
    BatchOutT<fhs_ciphertext> bo(outs, count);
    std::vector<double> scales(count);
    for (int i = 0; i < count; ++i) scales[i] = pts[i]->scale;
    for (int i0 = 0; i0 < count; i0 += kMaxBatch) {
        const int n = std::min(kMaxBatch, count - i0);
        const fhs_status s = encrypt_sym_core(c, sk, n, pts[0]->l, pts[0]->ci, scales.data() + i0, pts + i0, nullptr,
                                              outs + i0);
        if (s != FHS_OK) return s;
    }
    return bo.keep(FHS_OK);
}
// The head of both fhs_encode_encrypt_*_batch entries: `count` vectors of n values staged into dvals and encoded to
// their rounded message coefficients in coef (count x N doubles, launch_encode_coef).  Both blocks are the caller's.
static fhs_status encode_coef_batch(fhs_context* c, const double* values, size_t count, size_t n, bool is_real,
                                    double scale, DevTmp& dvals, DevTmp& coef) {
    const size_t stride = is_real ? n : 2 * n;
    HIPCHK(dvals.alloc(8 * count * stride), "encode_encrypt");
    HIPCHK(coef.alloc(8 * count * c->N), "encode_encrypt");
    if (stride) HIPCHK(stage_h2d(c, dvals.p, values, 8 * count * stride), "encode_encrypt");
    DevTmp tl(c);   // periodic rows: the sparse encoding, as encode_*_batch gives them
    HIPCHK(enc_periods(c, dvals.as<const double>(), count, n, stride, is_real, tl), "encode_encrypt");
    HIPCHK(fhs::launch_encode_coef(c->T, dvals.as<const double>(), (int)count, n, stride, is_real, scale,
                                   coef.as<double>(), c->st, tl.as<const unsigned char>()), "encode_encrypt");
    return FHS_OK;
}
// Extension (the client's encrypt_replicated of a stage's inputs, bg:53-58 / 124-127, in one pass):
// encode `count` vectors of n values (real, or interleaved re/im) at `scale` and chain index ci and encrypt
// them with sk -- limb for limb fhs_encode[_real]_batch followed by fhs_encrypt_symmetric_batch, without
// the plaintexts: the message's rounded coefficients go into the error's NTT.
extern "C" fhs_status fhs_encode_encrypt_symmetric_batch(fhs_context* c, fhs_secret_key* sk, const double* values,
                                                         size_t count, size_t n, int is_real, double scale, int ci,
                                                         fhs_ciphertext** outs) {
    ENTER(c);
    if (!sk || !outs || (!values && count && n)) return fail(FHS_ERR_INVALID, "encode_encrypt: null argument");
    fhs_status st = encode_checks(c, n, scale, ci);
    if (st != FHS_OK) return st;
    if (count == 0) return FHS_OK;
    if (count > (size_t)kMaxBatch) return fail(FHS_ERR_INVALID, "encode_encrypt: at most 4096 vectors per call");
    DevTmp dvals(c), coef(c);
    st = encode_coef_batch(c, values, count, n, is_real != 0, scale, dvals, coef);
    if (st != FHS_OK) return st;
    std::vector<double> scales(count, scale);
    return encrypt_sym_core(c, sk, (int)count, c->L0 + 1 - ci, ci, scales.data(), nullptr, coef.as<const double>(), outs);
}
// `count` public-key encryptions at l limbs with the counters ctr0 .. ctr0 + count - 1, which the caller has already
// taken from the key (a failure below does not give them back: a mask stream is never used twice): of the
// plaintexts pts[i], or (pts null) of the rounded message coefficients `coef` (count x N doubles,
// launch_encode_coef) -- encode and encrypt fused.  The new ciphertexts share one device block (new_cts) that
// the combine writes whole; they reach outs[0..count) only on success (outs is not touched otherwise).  Scratch:
// per ciphertext 3 N bytes of small values and 3 l N words of their transforms, then the plaintext pointers (more
// than one plaintext); the batch goes through it in runs of at most kPkScratchBytes.
static constexpr size_t kPkScratchBytes = (size_t)1 << 30;
static fhs_status encrypt_pk_core(fhs_context* c, fhs_public_key* pk, uint64_t ctr0, int count, int l, int ci,
                                  const double* scales, const fhs_plaintext* const* pts, const double* coef,
                                  fhs_ciphertext** outs) {
    CtBlock blk(c);
    fhs_status s = blk.make(count, 2, ci, scales[0]);
    if (s != FHS_OK) return s;
    for (int i = 0; i < count; ++i) blk[i]->scale = scales[i];
    const size_t S = (size_t)l * c->N;
    const int run = (int)std::min<size_t>(count, std::max<size_t>(1, kPkScratchBytes / (24 * S)));
    const size_t ub_bytes = 24 * S * run, small_bytes = (3 * (size_t)c->N * run + 7) & ~(size_t)7;
    std::vector<const uint64_t*> ptrs(pts ? count : 0);
    for (size_t i = 0; i < ptrs.size(); ++i) HIPCHK(pt_dense(c, pts[i], &ptrs[i]), "encrypt");
    const bool by_ptrs = ptrs.size() > 1;   // a single plaintext goes as a kernel argument
    DevTmp tmp(c);
    HIPCHK(tmp.alloc(ub_bytes + small_bytes + (by_ptrs ? 8 * ptrs.size() : 0)), "encrypt");
    unsigned char* small = tmp.as<unsigned char>() + ub_bytes;
    const fhs::u64* const* dptrs = nullptr;
    if (by_ptrs) {
        HIPCHK(stage_h2d(c, small + small_bytes, ptrs.data(), 8 * ptrs.size()), "encrypt");
        dptrs = reinterpret_cast<const fhs::u64* const*>(small + small_bytes);
    }
    const fhs::KTimer* tm = ktimer(c);
    for (int i0 = 0; i0 < count; i0 += run) {
        const int n = std::min(run, count - i0);
        HIPCHK(fhs::launch_encrypt_pk_batch(c->T, pk->rng, stream_id(ST_ENC_ASYM, ctr0 + (uint64_t)i0, 0),
                                            stream_id(0, 1, 0), blk.base() + (size_t)i0 * 2 * S, pk->pk,
                                            pk->pk + (size_t)c->L0 * c->N, dptrs ? dptrs + i0 : nullptr,
                                            ptrs.size() == 1 ? ptrs[0] : nullptr,
                                            coef ? coef + (size_t)i0 * c->N : nullptr, n, l,
                                            reinterpret_cast<signed char*>(small), tmp.p, c->st, tm), "encrypt");
    }
    return blk.commit(outs);
}
extern "C" fhs_status fhs_encrypt_asymmetric(fhs_context* c, fhs_public_key* pk, const fhs_plaintext* pt,
                                             fhs_ciphertext** out) {
    ENTER(c);
    if (!pk || !pt || !out) return fail(FHS_ERR_INVALID, "encrypt: null argument");
    const uint64_t ctr = pk->ctr++;
    return encrypt_pk_core(c, pk, ctr, 1, pt->l, pt->ci, &pt->scale, &pt, nullptr, out);
}
extern "C" fhs_status fhs_encrypt_asymmetric_batch(fhs_context* c, fhs_public_key* pk, const fhs_plaintext* const* pts,
                                                   int count, fhs_ciphertext** outs) {
    ENTER(c);
    if (!pk || !pts || !outs || count < 0) return fail(FHS_ERR_INVALID, "encrypt_batch: bad arguments");
    for (int i = 0; i < count; ++i)
        if (!pts[i]) return fail(FHS_ERR_INVALID, "encrypt_batch: null plaintext");
    if (count == 0) return FHS_OK;
    bool same = true;
    for (int i = 1; i < count; ++i) same &= pts[i]->l == pts[0]->l && pts[i]->ci == pts[0]->ci;
    // Built aside and handed over at the end, so a failure part-way destroys what was made and leaves outs alone.
    // Mixed levels: one at a time; same level: chunks of kMaxBatch (grid rows and scratch bound the launch).  Either
    // way the counters are consecutive and in order, so the ciphertexts are those of one call per plaintext.
    std::vector<fhs_ciphertext*> made(count, nullptr);
    BatchOutT<fhs_ciphertext> bo(made.data(), count);
    std::vector<double> scales(count);
    for (int i = 0; i < count; ++i) scales[i] = pts[i]->scale;
    for (int i0 = 0; i0 < count; i0 += same ? kMaxBatch : 1) {
        const int n = same ? std::min(kMaxBatch, count - i0) : 1;
        const uint64_t ctr0 = pk->ctr;
        pk->ctr += (uint64_t)n;
        const fhs_status s = encrypt_pk_core(c, pk, ctr0, n, pts[i0]->l, pts[i0]->ci, scales.data() + i0, pts + i0,
                                             nullptr, made.data() + i0);
        if (s != FHS_OK) return s;
    }
    for (int i = 0; i < count; ++i) outs[i] = made[i];
    return bo.keep(FHS_OK);
}
// Extension (the public-key client of ct_ct_search.py:54-90 in one pass): encode `count` vectors and encrypt them
// with pk -- limb for limb fhs_encode[_real]_batch followed by fhs_encrypt_asymmetric_batch, without the
// plaintexts: the message's rounded coefficients go into the NTT of e0 (k_ntt_fwd_msg_err).  The counters are taken
// before anything is allocated, so a failed call has used exactly `count` of them.
extern "C" fhs_status fhs_encode_encrypt_asymmetric_batch(fhs_context* c, fhs_public_key* pk, const double* values,
                                                          size_t count, size_t n, int is_real, double scale, int ci,
                                                          fhs_ciphertext** outs) {
    ENTER(c);
    if (!pk || !outs || (!values && count && n)) return fail(FHS_ERR_INVALID, "encode_encrypt: null argument");
    fhs_status st = encode_checks(c, n, scale, ci);
    if (st != FHS_OK) return st;
    if (count == 0) return FHS_OK;
    if (count > (size_t)kMaxBatch) return fail(FHS_ERR_INVALID, "encode_encrypt: at most 4096 vectors per call");
    const uint64_t ctr0 = pk->ctr;
    pk->ctr += (uint64_t)count;
    DevTmp dvals(c), coef(c);
    st = encode_coef_batch(c, values, count, n, is_real != 0, scale, dvals, coef);
    if (st != FHS_OK) return st;
    std::vector<double> scales(count, scale);
    return encrypt_pk_core(c, pk, ctr0, (int)count, c->L0 + 1 - ci, ci, scales.data(), nullptr, coef.as<const double>(), outs);
}
extern "C" fhs_status fhs_decrypt(fhs_context* c, fhs_secret_key* sk, const fhs_ciphertext* ct, fhs_plaintext** out) {
    ENTER(c);
    if (!sk || !ct || !out) return fail(FHS_ERR_INVALID, "decrypt: null argument");
    LIVE(ct);
    NEW_PT(pt, ct->ci, ct->scale);
    HIPCHK(fhs::launch_decrypt(c->T, ct->d, ct->ncomp, sk->s, pt->d, ct->l, c->st), "decrypt");
    *out = pt.release();
    return FHS_OK;
}

// ============================================================================ evaluator
static fhs_status same_level(const fhs_ciphertext* a, const fhs_ciphertext* b) {
    if (a->ci != b->ci) return fail(FHS_ERR_LEVEL, "operands are at different chain indices");
    return FHS_OK;
}
// What the batched entries read off their ciphertext handles: the fields the pure validators of fhs_tables.h judge,
// and the limbs.  append() adds those of in[0..n) after the null and lost checks, in order.
struct CtFields {
    std::vector<int> ncomp, ci;
    std::vector<double> scale;
    std::vector<const uint64_t*> d;
    fhs_status append(const fhs_ciphertext* const* in, size_t n) {
        for (size_t k = 0; k < n; ++k) {
            if (!in[k]) return fail(FHS_ERR_INVALID, "null argument");
            LIVE(in[k]);
            ncomp.push_back(in[k]->ncomp);
            ci.push_back(in[k]->ci);
            scale.push_back(in[k]->scale);
            d.push_back(in[k]->d);
        }
        return FHS_OK;
    }
};
// a validator's rejection (fhs_tables.h ArgErr) as the entry's status
static fhs_status fail_arg(ArgErr cls, const char* msg) {
    return fail(cls == ARG_LEVEL ? FHS_ERR_LEVEL : cls == ARG_SCALE ? FHS_ERR_SCALE : FHS_ERR_INVALID, msg);
}
// The pointer lists of one launch over R items, staged in stream order into the context's pointer buffer: first[0..R),
// then (second non-null) second[0..R).  *da and *db are the two lists on the device; *db is null without a second.
static hipError_t stage_ptr_lists(fhs_context* c, const uint64_t* const* first, const uint64_t* const* second, int R,
                                  const uint64_t* const** da, const uint64_t* const** db) {
    std::vector<const uint64_t*> ptrs(first, first + R);
    if (second) ptrs.insert(ptrs.end(), second, second + R);
    *da = reinterpret_cast<const uint64_t* const*>(c->ptrs_dev);
    *db = second ? *da + R : nullptr;
    return stage_h2d(c, c->ptrs_dev, ptrs.data(), sizeof(void*) * ptrs.size());
}

static fhs_status binop(fhs_context* c, int op, const fhs_ciphertext* a, const fhs_ciphertext* b, fhs_ciphertext** out) {
    if (!a || !b || !out) return fail(FHS_ERR_INVALID, "null argument");
    LIVE(a);
    LIVE(b);
    fhs_status s = same_level(a, b);
    if (s != FHS_OK) return s;
    if (a->ncomp != b->ncomp) return fail(FHS_ERR_INVALID, "ciphertext sizes differ");
    if (!scales_close(a->scale, b->scale)) return fail(FHS_ERR_SCALE, "scale mismatch");
    NEW_CT(r, a->ncomp, a->ci, a->scale);
    const size_t cs = (size_t)a->l * c->N;
    HIPCHK(fhs::launch_eltwise(c->T, op, a->d, b->d, r->d, a->ncomp, a->l, cs, cs, c->st), "eltwise");
    *out = r.release();
    return FHS_OK;
}
extern "C" fhs_status fhs_add(fhs_context* c, const fhs_ciphertext* a, const fhs_ciphertext* b, fhs_ciphertext** out) {
    ENTER(c);
    return binop(c, fhs::OP_ADD, a, b, out);
}
extern "C" fhs_status fhs_sub(fhs_context* c, const fhs_ciphertext* a, const fhs_ciphertext* b, int negate,
                              fhs_ciphertext** out) {
    ENTER(c);
    return binop(c, negate ? fhs::OP_SUBNEG : fhs::OP_SUB, a, b, out);
}
extern "C" fhs_status fhs_negate(fhs_context* c, const fhs_ciphertext* a, fhs_ciphertext** out) {
    ENTER(c);
    if (!a || !out) return fail(FHS_ERR_INVALID, "null argument");
    LIVE(a);
    NEW_CT(r, a->ncomp, a->ci, a->scale);
    const size_t cs = (size_t)a->l * c->N;
    HIPCHK(fhs::launch_eltwise(c->T, fhs::OP_NEG, a->d, nullptr, r->d, a->ncomp, a->l, cs, 0, c->st), "negate");
    *out = r.release();
    return FHS_OK;
}
static fhs_status plainop(fhs_context* c, int op, const fhs_ciphertext* a, const fhs_plaintext* p, fhs_ciphertext** out) {
    if (!a || !p || !out) return fail(FHS_ERR_INVALID, "null argument");
    LIVE(a);
    if (a->ci != p->ci) return fail(FHS_ERR_LEVEL, "ciphertext and plaintext are at different chain indices");
    const double sc = op == fhs::OP_MULP ? a->scale * p->scale : a->scale;
    if (op != fhs::OP_MULP && !scales_close(a->scale, p->scale)) return fail(FHS_ERR_SCALE, "scale mismatch");
    NEW_CT(r, a->ncomp, a->ci, sc);
    const size_t cs = (size_t)a->l * c->N;
    PT_DENSE(pd, p, "plain op");
    HIPCHK(fhs::launch_eltwise(c->T, op, a->d, pd, r->d, a->ncomp, a->l, cs, 0, c->st), "plain op");
    *out = r.release();
    return FHS_OK;
}
extern "C" fhs_status fhs_add_plain(fhs_context* c, const fhs_ciphertext* a, const fhs_plaintext* p, fhs_ciphertext** out) {
    ENTER(c);
    return plainop(c, fhs::OP_ADDP, a, p, out);
}
extern "C" fhs_status fhs_sub_plain(fhs_context* c, const fhs_ciphertext* a, const fhs_plaintext* p, fhs_ciphertext** out) {
    ENTER(c);
    return plainop(c, fhs::OP_SUBP, a, p, out);
}
extern "C" fhs_status fhs_multiply_plain(fhs_context* c, const fhs_ciphertext* a, const fhs_plaintext* p,
                                         fhs_ciphertext** out) {
    ENTER(c);
    return plainop(c, fhs::OP_MULP, a, p, out);
}
extern "C" fhs_status fhs_multiply(fhs_context* c, const fhs_ciphertext* a, const fhs_ciphertext* b, fhs_ciphertext** out) {
    ENTER(c);
    if (!a || !b || !out) return fail(FHS_ERR_INVALID, "null argument");
    LIVE(a);
    LIVE(b);
    fhs_status s = same_level(a, b);
    if (s != FHS_OK) return s;
    if (a->ncomp != 2 || b->ncomp != 2) return fail(FHS_ERR_INVALID, "multiply expects 2-component ciphertexts");
    NEW_CT(r, 3, a->ci, a->scale * b->scale);
    // one pair: its pointers travel as kernel arguments, nothing is staged
    HIPCHK(fhs::launch_tensor(c->T, nullptr, nullptr, a->d, b->d, 1, r->d, a->l, c->st), "multiply");
    *out = r.release();
    return FHS_OK;
}

// Relinearisation of R three-component ciphertexts t3 [R][3][l][N] into dst [R][2][l][N] as ONE batched key switch
// of component 2 (a = comp 2, add0 = comp 0, add1 = comp 1; R = U: every item has its own input).  ws: at least
// wsb = keyswitch_workspace_bytes(R, R, l) bytes of key-switch workspace.
static fhs_status relin_batch(fhs_context* c, const fhs_relin_key* rk, const uint64_t* t3, uint64_t* dst, int R, int l,
                              uint64_t* ws, size_t wsb, const fhs::KTimer* tm) {
    const size_t S = (size_t)l * c->N;
    const uint64_t* akey = key_akey(c, rk->key);
    std::vector<KsItem> items(R);
    std::vector<const uint64_t*> uniq(R);
    for (int r = 0; r < R; ++r) {
        const uint64_t* t = t3 + (size_t)r * 3 * S;
        uint64_t* o = dst + (size_t)r * 2 * S;
        items[r] = KsItem{t + 2 * S, t, t + S, rk->key, o, o + S, 1, (uint64_t)r, akey};
        uniq[r] = t + 2 * S;
    }
    HIPCHK(fhs::launch_keyswitch(c->T, items.data(), R, reinterpret_cast<const fhs::u64* const*>(uniq.data()), R, l, ws,
                                 wsb, c->items_dev, c->stager, c->st, tm), "key-switch");
    return FHS_OK;
}

extern "C" fhs_status fhs_relinearize(fhs_context* c, const fhs_ciphertext* a, const fhs_relin_key* rk,
                                      fhs_ciphertext** out) {
    ENTER(c);
    if (!a || !rk || !out) return fail(FHS_ERR_INVALID, "null argument");
    LIVE(a);
    if (a->ncomp != 3) return fail(FHS_ERR_INVALID, "relinearize expects a 3-component ciphertext");
    NEW_CT(r, 2, a->ci, a->scale);
    const size_t wsb = fhs::keyswitch_workspace_bytes(c->T, 1, 1, a->l);
    uint64_t* ws = nullptr;
    HIPCHK(scratch(c, fhs_context::SCR_KS, wsb, &ws), "key-switch workspace");
    fhs_status s = relin_batch(c, rk, a->d, r->d, 1, a->l, ws, wsb, nullptr);
    if (s != FHS_OK) return s;
    *out = r.release();
    return FHS_OK;
}

extern "C" fhs_status fhs_rescale_to_next(fhs_context* c, const fhs_ciphertext* a, fhs_ciphertext** out) {
    ENTER(c);
    if (!a || !out) return fail(FHS_ERR_INVALID, "null argument");
    LIVE(a);
    if (a->l < 2) return fail(FHS_ERR_LEVEL, "rescale_to_next: no level left (end of modulus switching chain)");
    NEW_CT(r, a->ncomp, a->ci + 1, a->scale / (double)c->q[a->l - 1]);
    uint64_t* scr = nullptr;
    HIPCHK(scratch(c, fhs_context::SCR_RESCALE, 8ull * a->ncomp * c->N, &scr), "rescale");
    HIPCHK(fhs::launch_rescale(c->T, a->d, r->d, scr, a->ncomp, a->l, c->st), "rescale");
    *out = r.release();
    return FHS_OK;
}

static fhs_status drop_ct(fhs_context* c, const fhs_ciphertext* a, int ci, fhs_ciphertext** out) {
    LIVE(a);
    if (ci < a->ci) return fail(FHS_ERR_LEVEL, "mod_switch_to: cannot switch to a higher level");
    NEW_CT(r, a->ncomp, ci, a->scale);
    const size_t row = 8ull * r->l * c->N, pitch = 8ull * a->l * c->N;
    HIPCHK(hipMemcpy2DAsync(r->d, row, a->d, pitch, row, a->ncomp, hipMemcpyDeviceToDevice, c->st), "mod_switch");
    *out = r.release();
    return FHS_OK;
}
extern "C" fhs_status fhs_mod_switch_to_next(fhs_context* c, const fhs_ciphertext* a, fhs_ciphertext** out) {
    ENTER(c);
    if (!a || !out) return fail(FHS_ERR_INVALID, "null argument");
    if (a->l < 2) return fail(FHS_ERR_LEVEL, "mod_switch_to_next: end of modulus switching chain");
    return drop_ct(c, a, a->ci + 1, out);
}
extern "C" fhs_status fhs_mod_switch_to(fhs_context* c, const fhs_ciphertext* a, int ci, fhs_ciphertext** out) {
    ENTER(c);
    if (!a || !out) return fail(FHS_ERR_INVALID, "null argument");
    if (ci > c->L0) return fail(FHS_ERR_LEVEL, "mod_switch_to: chain index out of range");
    return drop_ct(c, a, ci, out);
}
static fhs_status drop_pt(fhs_context* c, const fhs_plaintext* a, int ci, fhs_plaintext** out) {
    if (ci < a->ci || ci > c->L0) return fail(FHS_ERR_LEVEL, "mod_switch_to: bad target chain index");
    NEW_PT(r, ci, a->scale);
    PT_DENSE(pd, a, "mod_switch");
    HIPCHK(hipMemcpyAsync(r->d, pd, pt_bytes(r.p), hipMemcpyDeviceToDevice, c->st), "mod_switch");
    *out = r.release();
    return FHS_OK;
}
extern "C" fhs_status fhs_plain_mod_switch_to_next(fhs_context* c, const fhs_plaintext* a, fhs_plaintext** out) {
    ENTER(c);
    if (!a || !out) return fail(FHS_ERR_INVALID, "null argument");
    return drop_pt(c, a, a->ci + 1, out);
}
extern "C" fhs_status fhs_plain_mod_switch_to(fhs_context* c, const fhs_plaintext* a, int ci, fhs_plaintext** out) {
    ENTER(c);
    if (!a || !out) return fail(FHS_ERR_INVALID, "null argument");
    return drop_pt(c, a, ci, out);
}

// rotation: queued, flushed as one batched key-switch (see file header)
static fhs_status queue_rotation(fhs_context* c, const fhs_ciphertext* a, uint64_t elt, const fhs_galois_keys* gk,
                                 fhs_ciphertext** out) {
    if (!a || !gk || !out) return fail(FHS_ERR_INVALID, "null argument");
    LIVE(a);
    if (a->ncomp != 2) return fail(FHS_ERR_INVALID, "rotate expects a 2-component ciphertext");
    auto it = gk->keys.find(elt);
    if (it == gk->keys.end()) return fail(FHS_ERR_KEY, "galois key for this rotation step is not present");
    if (!c->pending.empty() && (c->pending_l != a->l || (int)c->pending.size() >= fhs_context::kMaxItems ||
                                c->pending_outs.count(a))) {
        fhs_status s = flush(c);
        if (s != FHS_OK) return s;
    }
    fhs_ciphertext* r;   // queued and handed out below: nothing fails in between
    fhs_status s = new_ct(c, 2, a->ci, a->scale, &r);
    if (s != FHS_OK) return s;
    const size_t S = (size_t)a->l * c->N;
    c->pending.push_back(PendingRot{KsItem{a->d + S, a->d, nullptr, it->second, r->d, r->d + S, elt, 0,
                                           key_akey(c, it->second)}, r, a});
    c->pending_l = a->l;
    c->pending_refs.insert(r);
    c->pending_refs.insert(a);
    c->pending_outs.insert(r);
    *out = r;
    return FHS_OK;
}
extern "C" fhs_status fhs_rotate(fhs_context* c, const fhs_ciphertext* a, int step, const fhs_galois_keys* gk,
                                 fhs_ciphertext** out) {
    if (!c) return fail(FHS_ERR_INVALID, "null context");
    Guard g(c);
    if (step == 0 || std::abs(step) >= (int)(c->N / 2)) {
        if (step == 0) return fail(FHS_ERR_INVALID, "rotate: step 0 (use apply_galois for conjugation)");
        return fail(FHS_ERR_INVALID, "rotate: |step| must be < slot count");
    }
    return queue_rotation(c, a, fhs_galois_elt_from_step(step, c->N), gk, out);
}
extern "C" fhs_status fhs_apply_galois(fhs_context* c, const fhs_ciphertext* a, uint64_t elt, const fhs_galois_keys* gk,
                                       fhs_ciphertext** out) {
    if (!c) return fail(FHS_ERR_INVALID, "null context");
    Guard g(c);
    return queue_rotation(c, a, elt, gk, out);
}
extern "C" fhs_status fhs_rotate_many(fhs_context* c, const fhs_ciphertext* const* in, const int* steps, int n,
                                      const fhs_galois_keys* gk, fhs_ciphertext** out) {
    if (!c) return fail(FHS_ERR_INVALID, "null context");
    if (!in || !steps || !out || n < 0) return fail(FHS_ERR_INVALID, "rotate_many: bad args");
    Guard g(c);
    // a batch that fails part-way (an output's allocation, the flush) hands out nothing: the outputs made so far are
    // destroyed -- the first of them still queued flushes the queue on its way out -- and their slots are null.  They
    // used to stay allocated, and queued, behind an error their caller had no handle to answer with.
    BatchOutT<fhs_ciphertext> bo(out, (size_t)n);
    for (int i = 0; i < n; ++i) {
        fhs_status s = queue_rotation(c, in[i], fhs_galois_elt_from_step(steps[i], c->N), gk, &out[i]);
        if (s != FHS_OK) return s;
    }
    return bo.keep(flush(c));
}

// ============================================================================ batched rotate-and-sum
// x_{k+1} = x_k + rotate(x_k, stride 2^k) for n ciphertexts at once (fri:71-75 per FFN column): at step k every
// ciphertext uses the same Galois key, so a step is ONE batched key switch over all of them (R = U = n: every item
// has its own input, nothing is hoisted) whose ModDown also adds sigma(x0) (add0), x0 (add0i) and x1 (add1) -- no
// add launch, no single-rotation flushes.  A step cannot run in place (the automorphism's gather reads arbitrary
// slots of x0), so the steps ping-pong between the results' block (new_cts) and one scratch block of its size,
// starting so that the last step lands in the results; step 0 reads the inputs, which are never written.
// Chunks of at most kMaxItems items, and of at most kInnerSumWsCap bytes of key-switch workspace: that workspace
// (8 N (l + dn E + 2 E + 2 P) bytes per item, + 16 l N in the SEAL convention; E = l + P, dn = ceil(l / P)) is the
// context's grow-only SCR_KS slot, held for the context's life, and 1 GiB of it already gives every stage of a step
// thousands of workgroups (fri's ring, N = 32768, l = 9, P = 1: 31.7 MB per item, 32 items per chunk, 10240
// workgroups of k_ks_ip).  Chunks are independent: each runs all its steps over its own slices of the two blocks.
constexpr size_t kInnerSumWsCap = (size_t)1 << 30;
extern "C" fhs_status fhs_inner_sum_many(fhs_context* c, const fhs_ciphertext* const* in, int n, int dim, int stride,
                                         const fhs_galois_keys* gk, fhs_ciphertext** out_array) {
    ENTER(c);
    if (!in || !gk || !out_array) return fail(FHS_ERR_INVALID, "null argument");
    std::vector<int> steps;
    if (const char* bad = inner_sum_steps(n, dim, stride, c->N, steps)) return fail(FHS_ERR_INVALID, bad);
    for (int i = 0; i < n; ++i) {
        if (!in[i]) return fail(FHS_ERR_INVALID, "null argument");
        LIVE(in[i]);
        if (in[i]->ncomp != 2) return fail(FHS_ERR_INVALID, "inner_sum_many expects 2-component ciphertexts");
        if (in[i]->ci != in[0]->ci) return fail(FHS_ERR_LEVEL, "inner_sum_many: inputs must share one chain index");
    }
    const int K = (int)steps.size(), ci = in[0]->ci, l = in[0]->l;
    // every step's key before anything is allocated or launched
    std::vector<const uint64_t*> keys(K), akeys(K);
    std::vector<uint64_t> elts(K);
    for (int k = 0; k < K; ++k) {
        elts[k] = fhs_galois_elt_from_step(steps[k], c->N);
        auto it = gk->keys.find(elts[k]);
        if (it == gk->keys.end()) return fail(FHS_ERR_KEY, "galois key for this rotation step is not present");
        keys[k] = it->second;
        akeys[k] = key_akey(c, it->second);
    }
    const size_t S = (size_t)l * c->N, per = 2 * S;
    // chunks of equal size (within one, the larger ones first) under both bounds; the workspace is the first chunk's
    const std::vector<std::pair<int, int>> chunks =
        batch_chunks(n, fhs::keyswitch_workspace_bytes(c->T, 1, 1, l), fhs_context::kMaxItems, kInnerSumWsCap);
    const int rchunk = chunks[0].second;
    // every allocation before the first launch; the outputs are the caller's only on success
    uint64_t* ws = nullptr;
    const size_t wsb = K ? fhs::keyswitch_workspace_bytes(c->T, rchunk, rchunk, l) : 0;
    if (K) HIPCHK(scratch(c, fhs_context::SCR_KS, wsb, &ws), "key-switch workspace");
    DevTmp pong(c);
    if (K >= 2) HIPCHK(pong.alloc(8 * (size_t)n * per), "inner_sum_many");
    CtBlock blk(c);
    fhs_status s = blk.make(n, 2, ci, in[0]->scale);
    if (s != FHS_OK) return s;
    for (int i = 0; i < n; ++i) blk[i]->scale = in[i]->scale;
    uint64_t* const res = blk.base();   // [n][2][l][N]
    if (K == 0) {
        for (int i = 0; i < n; ++i)
            HIPCHK(hipMemcpyAsync(res + (size_t)i * per, in[i]->d, 8 * per, hipMemcpyDeviceToDevice, c->st), "inner_sum_many");
    }
    const fhs::KTimer* tm = ktimer(c);
    std::vector<KsItem> items;
    std::vector<const uint64_t*> uniq;
    for (const auto& ch : chunks) {
        const int i0 = ch.first, R = ch.second;
        items.assign(R, KsItem{});
        uniq.resize(R);
        for (int k = 0; k < K; ++k) {
            // step k writes the results' block when an even number of steps follows it
            uint64_t* dst = (K - 1 - k) % 2 == 0 ? res : pong.p;
            const uint64_t* src = k == 0 ? nullptr : ((K - k) % 2 == 0 ? res : pong.p);
            for (int r = 0; r < R; ++r) {
                const uint64_t* x = src ? src + (size_t)(i0 + r) * per : in[i0 + r]->d;
                uint64_t* o = dst + (size_t)(i0 + r) * per;
                items[r] = KsItem{x + S, x, x + S, keys[k], o, o + S, elts[k], (uint64_t)r, akeys[k], nullptr, x};
                uniq[r] = x + S;
            }
            HIPCHK(fhs::launch_keyswitch(c->T, items.data(), R, reinterpret_cast<const fhs::u64* const*>(uniq.data()), R, l,
                                         ws, wsb, c->items_dev, c->stager, c->st, tm), "key-switch");
        }
    }
    return blk.commit(out_array);
}

// ============================================================================ fused BSGS
// giant_elts: null = 5^(g G) (the matvec, bg:478-483); else B Galois elements, giant_elts[0] = 1.
// rescale = false leaves the sum at the product scale (last SlotToCoeff group of the bootstrap).
// ptl > 0: pt_ptrs are the diagonals' compact shadows (pts_ptl)
static fhs_status bsgs_core(fhs_context* c, const fhs_ciphertext* const* baby, int G, const uint64_t* const* pt_ptrs,
                            int D, int B, int ci, double pt_scale, const fhs_galois_keys* gk, fhs_ciphertext** out,
                            const uint64_t* giant_elts = nullptr, bool rescale = true, int ptl = 0) {
    if (G < 1 || D < 1 || !baby) return fail(FHS_ERR_INVALID, "bsgs: bad G/D");
    const int Beff = std::min(B, (D + G - 1) / G);
    if (Beff < 1) return fail(FHS_ERR_INVALID, "bsgs: no giant groups");
    if (G > 2048 || (size_t)D + G > (size_t)fhs_context::kMaxPtrs) return fail(FHS_ERR_INVALID, "bsgs: too many diagonals");
    const int l = baby[0]->l;
    for (int b = 0; b < G; ++b) {
        if (!baby[b] || baby[b]->l != l || baby[b]->ncomp != 2 || baby[b]->ci != ci)
            return fail(FHS_ERR_LEVEL, "bsgs: baby steps and diagonals must share one chain index");
        LIVE(baby[b]);
    }
    if (rescale && l < 2) return fail(FHS_ERR_LEVEL, "bsgs: no level left for the final rescale");
    if (giant_elts && giant_elts[0] != 1) return fail(FHS_ERR_INVALID, "linear_transform: giant group 0 must be the identity");
    HostTrace ht;
    std::vector<const uint64_t*> keys(Beff, nullptr), akeys(Beff, nullptr);
    for (int g = 1; g < Beff; ++g) {
        const uint64_t elt = giant_elts ? giant_elts[g] : fhs_galois_elt_from_step(g * G, c->N);
        auto it = gk->keys.find(elt);
        if (it == gk->keys.end()) return fail(FHS_ERR_KEY, "bsgs: galois key for a giant step is missing");
        keys[g] = it->second;
        akeys[g] = key_akey(c, it->second);
    }
    const size_t S = (size_t)l * c->N;
    // pointer arrays -> device
    std::vector<const uint64_t*> ptrs(G + D);
    for (int b = 0; b < G; ++b) ptrs[b] = baby[b]->d;
    for (int k = 0; k < D; ++k) ptrs[G + k] = pt_ptrs[k];
    ht.mark("keys+ptrs");
    HIPCHK(stage_h2d(c, c->ptrs_dev, ptrs.data(), sizeof(void*) * (G + D)), "bsgs");
    ht.mark("stage ptrs");
    const uint64_t* const* dbaby = reinterpret_cast<const uint64_t* const*>(c->ptrs_dev);
    const uint64_t* const* dpts = dbaby + G;
    uint64_t* inner = nullptr;
    HIPCHK(scratch(c, fhs_context::SCR_BSGS_INNER, 8ull * Beff * 2 * S, &inner), "bsgs inner products");
    const fhs::KTimer* tm = ktimer(c);
    const size_t wsb = std::max<size_t>(8, fhs::bsgs_workspace_bytes(c->T, Beff - 1, l));
    uint64_t* ws = nullptr;
    HIPCHK(scratch(c, fhs_context::SCR_BSGS_WS, wsb, &ws), "bsgs workspace");
    uint64_t* sum = nullptr;
    HIPCHK(scratch(c, fhs_context::SCR_BSGS_SUM, 16 * S, &sum), "bsgs sum");
    ht.mark("workspaces");
    HIPCHK(fhs::launch_bsgs(c->T, dbaby, dpts, G, Beff, D, l, keys.data(), akeys.data(), giant_elts, inner, sum, ws, wsb,
                            c->items_dev, c->stager, c->st, tm, ptl, &c->side),
           "bsgs");
    ht.mark("launch bsgs");
    if (!rescale) {
        NEW_CT(r, 2, ci, baby[0]->scale * pt_scale);
        HIPCHK(hipMemcpyAsync(r->d, sum, 8 * 2 * S, hipMemcpyDeviceToDevice, c->st), "linear_transform");
        *out = r.release();
        return FHS_OK;
    }
    NEW_CT(r, 2, ci + 1, baby[0]->scale * pt_scale / (double)c->q[l - 1]);
    uint64_t* scr = nullptr;
    HIPCHK(scratch(c, fhs_context::SCR_RESCALE, 16ull * c->N, &scr), "bsgs rescale");
    HIPCHK(fhs::launch_rescale(c->T, sum, r->d, scr, 2, l, c->st, tm), "bsgs rescale");
    ht.mark("rescale+frees");
    *out = r.release();
    return FHS_OK;
}

// The Hadamard reads the diagonals' compact shadows when every one has one at the same tlog (encode_rows_dev; the
// same products, 2^-tlog of the bytes), else the dense limbs.  FHESPEAR_BSGS_DENSE=1 always reads the dense limbs.
static int pts_ptl(const fhs_context* c, const fhs_plaintext* const* pts, int D) {
    static const bool dense = getenv("FHESPEAR_BSGS_DENSE") != nullptr;
    if (dense || D < 1 || c->T.max_qbits > 59 || !pts[0]->dc) return 0;
    for (int k = 1; k < D; ++k)
        if (!pts[k]->dc || pts[k]->tlog != pts[0]->tlog) return 0;
    return pts[0]->tlog;
}
extern "C" fhs_status fhs_bsgs_multiply_accumulate(fhs_context* c, const fhs_ciphertext* const* baby, int G,
                                                   const fhs_plaintext* const* pts, int D, int B,
                                                   const fhs_galois_keys* gk, fhs_ciphertext** out) {
    ENTER(c);
    if (!pts || !gk || !out || !baby) return fail(FHS_ERR_INVALID, "null argument");
    std::vector<const uint64_t*> p(D);
    for (int k = 0; k < D; ++k) {
        if (!pts[k] || pts[k]->ci != baby[0]->ci) return fail(FHS_ERR_LEVEL, "bsgs: diagonal at a different chain index");
        if (!scales_close(pts[k]->scale, pts[0]->scale)) return fail(FHS_ERR_SCALE, "bsgs: diagonal scales differ");
    }
    const int ptl = pts_ptl(c, pts, D);
    for (int k = 0; k < D; ++k) {
        p[k] = pts[k]->dc;
        if (!ptl) HIPCHK(pt_dense(c, pts[k], &p[k]), "bsgs");
    }
    return bsgs_core(c, baby, G, p.data(), D, B, baby[0]->ci, pts[0]->scale, gk, out, nullptr, true, ptl);
}

// The Hadamard half of the fused BSGS alone: outs[g] = sum_{b < G} baby[b] (.) pts[g G + b], g < B, not
// rescaled (scale baby * pt).  Used by the baby-step-sharded latency mode (fhespear_dist.bsgs_baby_sharded):
// a rank holding baby steps b in its share forms every giant group's partial inner product.
// inner products of the B groups into dst ([g][2][l][N] words, device memory), stream-ordered
static fhs_status inner_products_core(fhs_context* c, const fhs_ciphertext* const* baby, int G,
                                      const fhs_plaintext* const* pts, int B, uint64_t* dst) {
    if (G < 1 || G > 2048 || B < 1) return fail(FHS_ERR_INVALID, "bsgs_inner_products: 1 <= G <= 2048, B >= 1");
    const int D = B * G, ci = baby[0]->ci, l = baby[0]->l;
    if ((size_t)D + G > (size_t)fhs_context::kMaxPtrs) return fail(FHS_ERR_INVALID, "bsgs_inner_products: too many plaintexts");
    std::vector<const uint64_t*> ptrs(G + D);
    for (int b = 0; b < G; ++b) {
        if (!baby[b] || baby[b]->l != l || baby[b]->ncomp != 2 || baby[b]->ci != ci)
            return fail(FHS_ERR_LEVEL, "bsgs_inner_products: baby steps must share one chain index");
        LIVE(baby[b]);
        ptrs[b] = baby[b]->d;
    }
    for (int k = 0; k < D; ++k) {
        if (!pts[k] || pts[k]->ci != ci) return fail(FHS_ERR_LEVEL, "bsgs_inner_products: plaintext at a different chain index");
        if (!scales_close(pts[k]->scale, pts[0]->scale)) return fail(FHS_ERR_SCALE, "bsgs_inner_products: plaintext scales differ");
    }
    const int ptl = pts_ptl(c, pts, D);
    for (int k = 0; k < D; ++k) {
        ptrs[G + k] = pts[k]->dc;
        if (!ptl) HIPCHK(pt_dense(c, pts[k], &ptrs[G + k]), "bsgs_inner_products");
    }
    HIPCHK(stage_h2d(c, c->ptrs_dev, ptrs.data(), sizeof(void*) * (G + D)), "bsgs_inner_products");
    const uint64_t* const* dbaby = reinterpret_cast<const uint64_t* const*>(c->ptrs_dev);
    HIPCHK(fhs::launch_bsgs_inner(c->T, dbaby, dbaby + G, G, 0, B, D, l, dst, c->st, ptl), "bsgs_inner_products");
    return FHS_OK;
}
extern "C" fhs_status fhs_bsgs_inner_products(fhs_context* c, const fhs_ciphertext* const* baby, int G,
                                              const fhs_plaintext* const* pts, int B, fhs_ciphertext** outs) {
    ENTER(c);
    if (!pts || !outs || !baby || !baby[0]) return fail(FHS_ERR_INVALID, "null argument");
    const int ci = baby[0]->ci;
    const size_t S = (size_t)baby[0]->l * c->N;
    uint64_t* inner = nullptr;
    HIPCHK(scratch(c, fhs_context::SCR_BSGS_INNER, 8ull * std::max(B, 1) * 2 * S, &inner), "bsgs_inner_products");
    fhs_status cs = inner_products_core(c, baby, G, pts, B, inner);
    if (cs != FHS_OK) return cs;
    BatchOutT<fhs_ciphertext> bo(outs, (size_t)B);
    for (int g = 0; g < B; ++g) {
        fhs_status st = new_ct(c, 2, ci, baby[0]->scale * pts[0]->scale, &outs[g]);
        if (st != FHS_OK) return st;
        HIPCHK(hipMemcpyAsync(outs[g]->d, inner + (size_t)g * 2 * S, 16 * S, hipMemcpyDeviceToDevice, c->st),
               "bsgs_inner_products");
    }
    return bo.keep(FHS_OK);
}

// fhs_bsgs_inner_products into caller device memory (e.g. a torch buffer that a reduce-scatter then
// sums): group g at dst + g 2 l N words, ordered on the context stream (fhs_context_stream).
extern "C" fhs_status fhs_bsgs_inner_products_device(fhs_context* c, const fhs_ciphertext* const* baby, int G,
                                                     const fhs_plaintext* const* pts, int B, uint64_t* dst) {
    ENTER(c);
    if (!pts || !dst || !baby || !baby[0]) return fail(FHS_ERR_INVALID, "null argument");
    return inner_products_core(c, baby, G, pts, B, dst);
}

// ============================================================================ fused ct x ct dot products
// Encrypted similarity scores of one query against C database chunks (ct_ct_search.py:92-106): the C sums of J
// tensor products in one launch (k_dot_tensor) into a scratch [C][3][l][N], then ONE relinearization per chunk
// -- a batched key switch of up to kDotKsBatch items (a = comp 2, add0 = comp 0, add1 = comp 1, as
// fhs_relinearize) -- and one rescale launch over all 2 C components: the outputs share one device block
// (new_cts), [C][2][l-1][N], which is exactly the layout launch_rescale writes for 2 C components.
// Key-switch workspace bound: a batch of R items takes keyswitch_workspace_bytes(R, R, l) =
// 8 N R (l + dn E + 2 E + 2 P) bytes (+ 16 R l N in the SEAL convention), E = l + P, dn = ceil(l / P); with
// R <= kDotKsBatch = 64 that is 105 MB at the retrieval shape (N = 8192, l = 3, P = 1) however many chunks the
// database has, and batches run back to back on the stream through the same workspace.
constexpr int kDotKsBatch = 64;
constexpr int kDotMaxChunks = 65535 / 3;
static_assert(kDotKsBatch <= fhs_context::kMaxItems, "a key-switch batch must fit the item buffer");
extern "C" fhs_status fhs_dot_product_many(fhs_context* c, const fhs_ciphertext* const* q, int J,
                                           const fhs_ciphertext* const* db, int C, const fhs_relin_key* rk, int rescale,
                                           fhs_ciphertext** outs) {
    ENTER(c);
    if (!q || !db || !outs) return fail(FHS_ERR_INVALID, "null argument");
    if (J < 1 || C < 1) return fail(FHS_ERR_INVALID, "dot_product_many: J >= 1 and C >= 1");
    // J + C J device pointers in the pointer buffer; 3 C components in one rescale launch (grid.y <= 65535)
    if ((size_t)J * ((size_t)C + 1) > (size_t)fhs_context::kMaxPtrs || C > kDotMaxChunks)
        return fail(FHS_ERR_INVALID, "dot_product_many: too many ciphertexts");
    if (c->N % 128) return fail(FHS_ERR_INVALID, "dot_product_many: poly_modulus_degree must be a multiple of 128");
    const size_t nq = (size_t)J, nd = (size_t)J * C;
    std::vector<const uint64_t*> ptrs(nq + nd);
    for (size_t k = 0; k < nq + nd; ++k) {
        const fhs_ciphertext* a = k < nq ? q[k] : db[k - nq];
        if (!a) return fail(FHS_ERR_INVALID, "null argument");
        LIVE(a);
        fhs_status s = same_level(q[0], a);
        if (s != FHS_OK) return s;
        if (a->ncomp != 2) return fail(FHS_ERR_INVALID, "multiply expects 2-component ciphertexts");
        if (!scales_close(a->scale, k < nq ? q[0]->scale : db[0]->scale)) return fail(FHS_ERR_SCALE, "scale mismatch");
        ptrs[k] = a->d;
    }
    const int ci = q[0]->ci, l = q[0]->l;
    if (rescale && l < 2) return fail(FHS_ERR_LEVEL, "rescale_to_next: no level left (end of modulus switching chain)");
    const size_t S = (size_t)l * c->N;
    const double sc = q[0]->scale * db[0]->scale;
    // every allocation before the first launch; the outputs are the caller's only on success (CtBlock)
    uint64_t *t3 = nullptr, *relin = nullptr, *ws = nullptr, *scr = nullptr;
    HIPCHK(scratch(c, fhs_context::SCR_BSGS_INNER, 8ull * C * 3 * S, &t3), "dot_product_many");
    if (rk && rescale) HIPCHK(scratch(c, fhs_context::SCR_BSGS_SUM, 8ull * C * 2 * S, &relin), "dot_product_many");
    const int Rmax = std::min(C, kDotKsBatch);
    const size_t wsb = rk ? fhs::keyswitch_workspace_bytes(c->T, Rmax, Rmax, l) : 0;
    if (rk) HIPCHK(scratch(c, fhs_context::SCR_KS, wsb, &ws), "key-switch workspace");
    const int ocomp = rk ? 2 : 3;
    if (rescale) HIPCHK(scratch(c, fhs_context::SCR_RESCALE, 8ull * ocomp * C * c->N, &scr), "rescale");
    CtBlock blk(c);
    fhs_status s = blk.make(C, ocomp, rescale ? ci + 1 : ci, rescale ? sc / (double)c->q[l - 1] : sc);
    if (s != FHS_OK) return s;
    uint64_t* const res = blk.base();   // [C][ocomp][l or l - 1][N]
    const fhs::KTimer* tm = ktimer(c);
    HIPCHK(stage_h2d(c, c->ptrs_dev, ptrs.data(), sizeof(void*) * (nq + nd)), "dot_product_many");
    const uint64_t* const* dq = reinterpret_cast<const uint64_t* const*>(c->ptrs_dev);
    // the tensor sums land where the last stage reads them: the outputs' block itself when nothing follows
    uint64_t* tdst = (!rk && !rescale) ? res : t3;
    HIPCHK(fhs::launch_dot_tensor(c->T, dq, dq + J, J, C, l, tdst, c->st, tm), "dot_product_many");
    if (rk) {
        uint64_t* kdst = rescale ? relin : res;   // [C][2][l][N]
        for (int c0 = 0; c0 < C; c0 += kDotKsBatch) {
            s = relin_batch(c, rk, t3 + (size_t)c0 * 3 * S, kdst + (size_t)c0 * 2 * S, std::min(kDotKsBatch, C - c0), l, ws,
                            wsb, tm);
            if (s != FHS_OK) return s;
        }
    }
    if (rescale) HIPCHK(fhs::launch_rescale(c->T, rk ? relin : t3, res, scr, ocomp * C, l, c->st, tm), "rescale");
    return blk.commit(outs);
}

// ============================================================================ batched multiply, relinearize, rescale
// out[i] = [rescale]([relinearize](a[i] (x) b[i])) for n pairs (fri:97-108, ct_ct_square per FFN column and
// ct_ct_multiply per channel), limb-identical to fhs_multiply, fhs_relinearize, fhs_rescale_to_next per pair.  Per
// chunk of R pairs: ONE tensor launch (k_tensor, the pair from the grid) into a scratch [R][3][l][N], ONE batched key
// switch of R items (a = comp 2, add0 = comp 0, add1 = comp 1, as fhs_relinearize) into [R][2][l][N], and ONE
// rescale launch over the chunk's components straight into the chunk's slice of the results' block (new_cts),
// which is contiguous in exactly the layout launch_rescale writes; the last stage present writes the results.
// Chunks (fhs_tables.h batch_chunks) are bounded by kMaxItems and by kMulManyCap bytes of scratch per chunk -- per
// item the key-switch workspace (8 N (l + dn E + 2 E + 2 P), + 16 l N in the SEAL convention; E = l + P,
// dn = ceil(l / P)), the tensor product (24 l N), the relinearized pair (16 l N) and the rescale's last limbs (16 N
// or 24 N), whichever of them the call uses.
extern "C" fhs_status fhs_multiply_relin_many(fhs_context* c, const fhs_ciphertext* const* a,
                                              const fhs_ciphertext* const* b, int n, const fhs_relin_key* rk, int rescale,
                                              fhs_ciphertext** out_array) {
    ENTER(c);
    const bool null_arg = !a || !out_array;
    CtFields h;   // a's then b's
    fhs_status s = FHS_OK;
    if (!null_arg && n >= 1) {
        s = h.append(a, (size_t)n);
        if (s == FHS_OK && b) s = h.append(b, (size_t)n);
    }
    if (s != FHS_OK) return s;
    ArgErr cls;
    if (const char* bad = multiply_many_error(null_arg, n, h.ncomp.data(), h.ci.data(), h.ci.size(), c->L0, rescale, &cls))
        return fail_arg(cls, bad);
    const int ci = a[0]->ci, l = a[0]->l, ocomp = rk ? 2 : 3;
    const size_t S = (size_t)l * c->N;
    // chunks of equal size (within one) under both bounds; the scratch is the largest (first) chunk's
    const size_t item = (rk ? fhs::keyswitch_workspace_bytes(c->T, 1, 1, l) : 0) + ((rk || rescale) ? 8 * 3 * S : 0) +
                        ((rk && rescale) ? 8 * 2 * S : 0) + (rescale ? 8ull * ocomp * c->N : 0);
    const std::vector<std::pair<int, int>> chunks = batch_chunks(n, item, fhs_context::kMaxItems, kMulManyCap);
    const int Rmax = chunks[0].second;
    // every allocation before the first launch; out_array is written only on success
    uint64_t *t3 = nullptr, *relin = nullptr, *ws = nullptr, *scr = nullptr;
    if (rk || rescale) HIPCHK(scratch(c, fhs_context::SCR_BSGS_INNER, 8ull * Rmax * 3 * S, &t3), "multiply_relin_many");
    if (rk && rescale) HIPCHK(scratch(c, fhs_context::SCR_BSGS_SUM, 8ull * Rmax * 2 * S, &relin), "multiply_relin_many");
    const size_t wsb = rk ? fhs::keyswitch_workspace_bytes(c->T, Rmax, Rmax, l) : 0;
    if (rk) HIPCHK(scratch(c, fhs_context::SCR_KS, wsb, &ws), "key-switch workspace");
    if (rescale) HIPCHK(scratch(c, fhs_context::SCR_RESCALE, 8ull * ocomp * Rmax * c->N, &scr), "rescale");
    CtBlock blk(c);
    s = blk.make(n, ocomp, rescale ? ci + 1 : ci, 1.0);
    if (s != FHS_OK) return s;
    for (int i = 0; i < n; ++i) {
        const double sc = a[i]->scale * (b ? b[i] : a[i])->scale;   // fhs_multiply's, then fhs_rescale_to_next's
        blk[i]->scale = rescale ? sc / (double)c->q[l - 1] : sc;
    }
    uint64_t* const res = blk.base();   // [n][ocomp][l or l - 1][N]
    const size_t per_out = blk.words_per_ct();
    const fhs::KTimer* tm = ktimer(c);
    for (const auto& ch : chunks) {
        const int i0 = ch.first, R = ch.second;
        uint64_t* const slice = res + (size_t)i0 * per_out;
        // each stage lands where the next one reads it: the results' slice itself when nothing follows
        uint64_t* const tdst = (rk || rescale) ? t3 : slice;
        if (R == 1) {
            HIPCHK(fhs::launch_tensor(c->T, nullptr, nullptr, a[i0]->d, (b ? b[i0] : a[i0])->d, 1, tdst, l, c->st),
                   "multiply_relin_many");
        } else {
            // the chunk's pointer lists, a's then b's (squares: a's alone, read as both)
            const uint64_t *const *da = nullptr, *const *db = nullptr;
            HIPCHK(stage_ptr_lists(c, h.d.data() + i0, b ? h.d.data() + n + i0 : nullptr, R, &da, &db), "multiply_relin_many");
            HIPCHK(fhs::launch_tensor(c->T, da, b ? db : da, nullptr, nullptr, R, tdst, l, c->st), "multiply_relin_many");
        }
        if (rk) {
            s = relin_batch(c, rk, t3, rescale ? relin : slice, R, l, ws, wsb, tm);
            if (s != FHS_OK) return s;
        }
        if (rescale) HIPCHK(fhs::launch_rescale(c->T, rk ? relin : t3, slice, scr, ocomp * R, l, c->st, tm), "rescale");
    }
    return blk.commit(out_array);
}

// ============================================================================ batched CT x PT multiply and rescale
// out[i] = rescale_to_next(multiply_plain(a[i], p[i])) for n pairs (fri:67-70, the head of ct_pt_dot for every column
// at once; p null: the rescale alone), limb-identical to the two calls per pair.  Per chunk of R pairs (fhs_tables.h
// mulp_rescale_chunks) the two launches of ONE rescale over the 2 R components (launch_rescale_many), which read the
// operands through staged pointer lists and form each product in their loads: no product is stored.  The second
// launch writes the chunk's slice of the results' block (new_cts), which is exactly its [R][2][l - 1][N] layout.
extern "C" fhs_status fhs_multiply_plain_rescale_many(fhs_context* c, const fhs_ciphertext* const* a,
                                                      const fhs_plaintext* const* p, int n, fhs_ciphertext** out_array) {
    ENTER(c);
    const bool null_arg = !a || !out_array;
    const int cnt = (null_arg || n < 1) ? 0 : n;
    CtFields h;
    std::vector<int> pcis(p ? cnt : 0);
    for (int k = 0; k < cnt; ++k) {   // pair by pair: a null plaintext is reported before a lost ciphertext after it
        if (p && !p[k]) return fail(FHS_ERR_INVALID, "null argument");
        const fhs_status s = h.append(a + k, 1);
        if (s != FHS_OK) return s;
        if (p) pcis[k] = p[k]->ci;
    }
    ArgErr cls;
    if (const char* bad = mulp_rescale_many_error(null_arg, n, h.ncomp.data(), h.ci.data(), p ? pcis.data() : nullptr, c->L0, &cls))
        return fail_arg(cls, bad);
    const int ci = a[0]->ci, l = a[0]->l;
    const size_t N = c->N;
    const std::vector<std::pair<int, int>> chunks = mulp_rescale_chunks(n, N);
    const size_t Rmax = (size_t)chunks[0].second;
    // every allocation before the first launch of the call's own kernels; out_array is written only on success
    uint64_t* scr = nullptr;
    HIPCHK(scratch(c, fhs_context::SCR_RESCALE, mulp_rescale_item_bytes(N) * Rmax, &scr), "rescale");
    CtBlock blk(c);
    fhs_status s = blk.make(n, 2, ci + 1, 1.0);
    if (s != FHS_OK) return s;
    std::vector<const uint64_t*> pd(p ? n : 0);
    for (int i = 0; i < n; ++i) {
        double sc = a[i]->scale;                       // fhs_multiply_plain's, then fhs_rescale_to_next's
        if (p) {
            sc = a[i]->scale * p[i]->scale;
            HIPCHK(pt_dense(c, p[i], &pd[i]), "multiply_plain_rescale_many");   // a compact-only plaintext's dense limbs
        }
        blk[i]->scale = sc / (double)c->q[l - 1];
    }
    uint64_t* const res = blk.base();   // [n][2][l - 1][N]
    const size_t per_out = blk.words_per_ct();
    const fhs::KTimer* tm = ktimer(c);
    for (const auto& ch : chunks) {
        const int i0 = ch.first, R = ch.second;
        // the chunk's pointer lists, the ciphertexts' then the plaintexts'
        const uint64_t *const *da = nullptr, *const *dp = nullptr;
        HIPCHK(stage_ptr_lists(c, h.d.data() + i0, p ? pd.data() + i0 : nullptr, R, &da, &dp), "multiply_plain_rescale_many");
        HIPCHK(fhs::launch_rescale_many(c->T, da, dp, R, l, res + (size_t)i0 * per_out, scr, c->st, tm),
               "multiply_plain_rescale_many");
    }
    return blk.commit(out_array);
}

// ============================================================================ plaintext-weighted sums of ciphertexts
// out[i] = sum_j rescale_to_next(multiply_plain(in[j], P_ij)), P_ij the constant plaintext round(W[j ldw + i] scale)
// (fri:79-94, ct_pt_weighted_sum for every output column at once), limb-identical to that loop although the rescale
// rounds per term: with L = l - 1, inv_m = q_L^-1 mod q_m and d_j = INTT_L(in[j] limb L),
//   out_i[comp][m] = sum_j (k_ijm inv_m) c_j[comp][m] - inv_m NTT_m(S_i[comp] mod q_m),
//   S_i[comp][n]   = sum_j centre(k_ijL d_j[comp][n] mod q_L)          (DESIGN.md section 3 "weighted sums").
// One launch takes every input's last limb to coefficient form (k_rescale_intt over a pointer list); then per chunk of
// outputs (fhs_tables.h weighted_sums_chunks) four launches whatever F and E: the rounding sums (k_scalar,
// SCALAR_WSUM_ROUND), their residues and NTT (launch_encode_int128: two) and the weighted sums (k_scalar,
// SCALAR_WSUM_ACC) straight into the chunk's slice of the results' block.
extern "C" fhs_status fhs_weighted_sums(fhs_context* c, const fhs_ciphertext* const* in, int F, const double* W,
                                        int64_t ldw, int E, double scale, fhs_ciphertext** out_array) {
    ENTER(c);
    const bool null_arg = !in || !W || !out_array;
    const int cnt = (null_arg || F < 1 || F > kWsumMaxF) ? 0 : F;
    CtFields h;
    fhs_status s = h.append(in, (size_t)cnt);
    if (s != FHS_OK) return s;
    ArgErr cls;
    if (const char* bad = weighted_sums_error(null_arg, F, E, ldw, scale, h.ncomp.data(), h.ci.data(), h.scale.data(), c->L0, &cls))
        return fail_arg(cls, bad);
    const int ci = in[0]->ci, l = in[0]->l, lm = l - 1;
    if (c->N % 2) return fail(FHS_ERR_INVALID, "weighted_sums: poly_modulus_degree must be even");
    WsumTables Wt;
    if (const char* bad = weighted_sums_tables(W, ldw, F, E, scale, c->q.data(), l, fhs::wsum_tile(), Wt))
        return fail(FHS_ERR_INVALID, bad);
    const size_t N = c->N;
    const std::vector<std::pair<int, int>> chunks = weighted_sums_chunks(E, F, N, l);
    const size_t Rmax = (size_t)chunks[0].second;
    // every allocation before the first launch; out_array is written only on success
    uint64_t *dco = nullptr, *planes = nullptr, *tcorr = nullptr, *wdev = nullptr, *tptrs = nullptr;
    HIPCHK(scratch(c, fhs_context::SCR_RESCALE, 16 * (size_t)F * N, &dco), "weighted_sums");
    HIPCHK(scratch(c, fhs_context::SCR_BSGS_SUM, 32 * Rmax * N, &planes), "weighted_sums");
    HIPCHK(scratch(c, fhs_context::SCR_BSGS_INNER, 16 * Rmax * lm * N, &tcorr), "weighted_sums");
    HIPCHK(scratch(c, fhs_context::SCR_BSGS_WS, 8 * (Wt.wl.size() + Wt.wt.size()), &wdev), "weighted_sums");
    HIPCHK(scratch(c, fhs_context::SCR_ENC_PTRS, 16 * Rmax, &tptrs), "weighted_sums");
    CtBlock blk(c);
    s = blk.make(E, 2, ci + 1, in[0]->scale * scale / (double)c->q[l - 1]);
    if (s != FHS_OK) return s;
    uint64_t* const res = blk.base();   // [E][2][l - 1][N]
    uint64_t* const wt_dev = wdev + Wt.wl.size();
    std::vector<uint64_t*> tp(2 * Rmax);
    for (size_t v = 0; v < 2 * Rmax; ++v) tp[v] = tcorr + v * lm * N;
    HIPCHK(stage_h2d(c, c->ptrs_dev, h.d.data(), sizeof(void*) * h.d.size()), "weighted_sums");
    HIPCHK(stage_h2d(c, tptrs, tp.data(), sizeof(void*) * tp.size()), "weighted_sums");
    HIPCHK(stage_h2d(c, wdev, Wt.wl.data(), 8 * Wt.wl.size()), "weighted_sums");
    HIPCHK(stage_h2d(c, wt_dev, Wt.wt.data(), 8 * Wt.wt.size()), "weighted_sums");
    const uint64_t* const* din = reinterpret_cast<const uint64_t* const*>(c->ptrs_dev);
    const fhs::KTimer* tm = ktimer(c);
    HIPCHK(fhs::launch_last_limbs_intt(c->T, din, F, l, dco, c->st, tm), "weighted_sums");
    for (const auto& ch : chunks)
        HIPCHK(fhs::launch_wsum_chunk(c->T, din, dco, wdev, wt_dev, F, Wt.Epad, ch.first, ch.second, l, planes, tcorr,
                                      reinterpret_cast<fhs::u64* const*>(tptrs), res, c->st, tm), "weighted_sums");
    return blk.commit(out_array);
}

// Test hooks: the per-coefficient routines of fhs_weighted_sums' two pointwise stages (fhs_modarith.h wsum_round_*,
// wsum_*) on the host, in the kernel's order.  round: S = sum_j centre(k_j d_j mod qL) as the signed 128-bit
// hi 2^64 + lo; accumulate: (sum_j kprime_j c_j + wT t) mod q.  Operands must be < q < 2^60.
extern "C" fhs_status fhs_debug_wsum_round(uint64_t qL, const uint64_t* k, const uint64_t* d, int F, int64_t* hi,
                                           uint64_t* lo) {
    if (!k || !d || !hi || !lo || F < 1 || F > kWsumMaxF) return fail(FHS_ERR_INVALID, "debug_wsum_round: bad argument");
    if (qL < 3 || !(qL & 1) || qL >= (1ull << 60)) return fail(FHS_ERR_INVALID, "debug_wsum_round: q must be odd and < 2^60");
    WsumRound s{0, 0, 0};
    for (int j = 0; j < F; ++j) {
        if (k[j] >= qL || d[j] >= qL) return fail(FHS_ERR_INVALID, "debug_wsum_round: operands must be < q");
        wsum_round_term(s, d[j], k[j], h_shoup(k[j], qL), qL);
    }
    wsum_round_finish(s, qL, *hi, *lo);
    return FHS_OK;
}
extern "C" fhs_status fhs_debug_wsum_accumulate(uint64_t q, const uint64_t* kprime, const uint64_t* cj, int F, uint64_t wT,
                                                uint64_t t, uint64_t* out) {
    if (!kprime || !cj || !out || F < 1 || F > kWsumMaxF) return fail(FHS_ERR_INVALID, "debug_wsum_accumulate: bad argument");
    if (q < 3 || !(q & 1) || q >= (1ull << 60)) return fail(FHS_ERR_INVALID, "debug_wsum_accumulate: q must be odd and < 2^60");
    if (wT >= q || t >= q) return fail(FHS_ERR_INVALID, "debug_wsum_accumulate: operands must be < q");
    const uint64_t w = pm_word(q, 14);
    const hu128 r = ~(hu128)0 / q;
    const RedU R{q, (uint64_t)r, (uint64_t)(r >> 64), (unsigned)(w & 127), (unsigned)((w >> 8) & 0xFFFFFFFFu), false, false};
    const unsigned fmask = wsum_fmask(q);
    Wsum s;
    wsum_clear(s);
    for (int j = 0; j < F; ++j) {
        if (kprime[j] >= q || cj[j] >= q) return fail(FHS_ERR_INVALID, "debug_wsum_accumulate: operands must be < q");
        wsum_mac(s, unpack30(pack30(kprime[j])), split30(cj[j]));
        wsum_after(s, j + 1, fmask, R);
    }
    wsum_mac(s, unpack30(pack30(wT)), split30(t));
    *out = wsum_finish(s, R);
    return FHS_OK;
}

// Test hook: k_dot_tensor's per-coefficient schedule (dot3_term / dot3_finish, fhs_modarith.h: accumulate, fold,
// reduce, windows of kDotWindowMax terms adding their reduced sums) on the host for one coefficient of prime q:
// out3 = (sum a0 b0, sum a0 b1 + a1 b0, sum a1 b1) mod q over J terms, with the fold the kernel would take for
// this prime alone (16 products per Acc3 below 2^59, else 8).  Operands must be < q < 2^60.
template <int FOLD>
static void dot_accumulate_host(const RedU& R, const uint64_t* a0, const uint64_t* a1, const uint64_t* b0,
                                const uint64_t* b1, int J, uint64_t* out3) {
    for (int j0 = 0; j0 < J; j0 += kDotWindowMax) {
        const int Jw = std::min(kDotWindowMax, J - j0);
        Dot3 s;
        dot3_clear(s);
        for (int j = 0; j < Jw; ++j)
            dot3_term<FOLD>(s, j, unpack30(pack30(a0[j0 + j])), unpack30(pack30(a1[j0 + j])), split30(b0[j0 + j]),
                            split30(b1[j0 + j]));
        uint64_t prev[3] = {out3[0], out3[1], out3[2]};
        dot3_finish(s, R, j0 ? prev : nullptr, out3);
    }
}
extern "C" fhs_status fhs_debug_dot_accumulate(uint64_t q, const uint64_t* a0, const uint64_t* a1, const uint64_t* b0,
                                               const uint64_t* b1, int J, uint64_t* out3) {
    if (!a0 || !a1 || !b0 || !b1 || !out3 || J < 1) return fail(FHS_ERR_INVALID, "debug_dot_accumulate: bad argument");
    if (q < 3 || q >= (1ull << 60)) return fail(FHS_ERR_INVALID, "debug_dot_accumulate: q must be < 2^60");
    for (int j = 0; j < J; ++j)
        if (a0[j] >= q || a1[j] >= q || b0[j] >= q || b1[j] >= q)
            return fail(FHS_ERR_INVALID, "debug_dot_accumulate: operands must be < q");
    const uint64_t w = pm_word(q, 14);
    const hu128 r = ~(hu128)0 / q;   // floor((2^128 - 1) / q) = floor(2^128 / q): q is odd
    const RedU R{q, (uint64_t)r, (uint64_t)(r >> 64), (unsigned)(w & 127), (unsigned)((w >> 8) & 0xFFFFFFFFu), false, false};
    out3[0] = out3[1] = out3[2] = 0;
    if (q < (1ull << 59)) dot_accumulate_host<16>(R, a0, a1, b0, b1, J, out3);
    else dot_accumulate_host<8>(R, a0, a1, b0, b1, J, out3);
    return FHS_OK;
}

// The giant-step half of the fused BSGS alone: out = sum_j rot_{elts[j]}(inners[j]), every rotation's
// key switch summed before one ModDown (k_giant_sum / k_giant_final), not rescaled.  elts[0] may be 1
// (an unrotated term); otherwise a zero term takes group 0's place.  The baby-step-sharded latency mode
// (fhespear_dist.bsgs_baby_sharded) finishes a rank's giant groups with it.
// src(j): device address of term j's 2 l N words
template <class Src>
static fhs_status giant_steps_core(fhs_context* c, Src src, int k, int ci, double scale, const uint64_t* elts,
                                   const fhs_galois_keys* gk, fhs_ciphertext** out) {
    const int l = c->L0 + 1 - ci;
    for (int j = 0; j < k; ++j) {
        if ((elts[j] & 1) == 0 || elts[j] >= 2 * c->N) return fail(FHS_ERR_INVALID, "bsgs_giant_steps: bad Galois element");
        if (j > 0 && elts[j] == 1) return fail(FHS_ERR_INVALID, "bsgs_giant_steps: only the first term may be unrotated");
    }
    const int pad = elts[0] == 1 ? 0 : 1, B = k + pad;   // group 0 = the unrotated term (or zero)
    std::vector<uint64_t> ge(B, 1);
    std::vector<const uint64_t*> keys(B, nullptr), akeys(B, nullptr);
    for (int g = 1; g < B; ++g) {
        ge[g] = elts[g - pad];
        auto it = gk->keys.find(ge[g]);
        if (it == gk->keys.end()) return fail(FHS_ERR_KEY, "bsgs_giant_steps: galois key missing");
        keys[g] = it->second;
        akeys[g] = key_akey(c, it->second);
    }
    const size_t S = (size_t)l * c->N;
    uint64_t *inner = nullptr, *ws = nullptr, *sum = nullptr;
    HIPCHK(scratch(c, fhs_context::SCR_BSGS_INNER, 8ull * B * 2 * S, &inner), "bsgs_giant_steps");
    if (pad) HIPCHK(hipMemsetAsync(inner, 0, 16 * S, c->st), "bsgs_giant_steps");
    for (int j = 0; j < k; ++j)
        HIPCHK(hipMemcpyAsync(inner + (size_t)(j + pad) * 2 * S, src(j), 16 * S, hipMemcpyDeviceToDevice, c->st),
               "bsgs_giant_steps");
    const size_t wsb = std::max<size_t>(8, fhs::bsgs_workspace_bytes(c->T, B - 1, l));
    HIPCHK(scratch(c, fhs_context::SCR_BSGS_WS, wsb, &ws), "bsgs_giant_steps");
    HIPCHK(scratch(c, fhs_context::SCR_BSGS_SUM, 16 * S, &sum), "bsgs_giant_steps");
    const fhs::KTimer* tm = ktimer(c);
    HIPCHK(fhs::launch_bsgs(c->T, nullptr, nullptr, 1, B, B, l, keys.data(), akeys.data(), ge.data(), inner, sum, ws, wsb,
                            c->items_dev, c->stager, c->st, tm, 0, &c->side),
           "bsgs_giant_steps");
    NEW_CT(r, 2, ci, scale);
    HIPCHK(hipMemcpyAsync(r->d, sum, 16 * S, hipMemcpyDeviceToDevice, c->st), "bsgs_giant_steps");
    *out = r.release();
    return FHS_OK;
}
extern "C" fhs_status fhs_bsgs_giant_steps(fhs_context* c, const fhs_ciphertext* const* inners, int k,
                                           const uint64_t* elts, const fhs_galois_keys* gk, fhs_ciphertext** out) {
    ENTER(c);
    if (!inners || !elts || !gk || !out || k < 1 || !inners[0]) return fail(FHS_ERR_INVALID, "null argument");
    if (k > 511) return fail(FHS_ERR_INVALID, "bsgs_giant_steps: 1 <= k <= 511");
    const int l = inners[0]->l, ci = inners[0]->ci;
    for (int j = 0; j < k; ++j) {
        if (!inners[j] || inners[j]->ncomp != 2 || inners[j]->l != l || inners[j]->ci != ci)
            return fail(FHS_ERR_LEVEL, "bsgs_giant_steps: inner products must be 2-component at one chain index");
        LIVE(inners[j]);
        if (!scales_close(inners[j]->scale, inners[0]->scale)) return fail(FHS_ERR_SCALE, "bsgs_giant_steps: scales differ");
    }
    return giant_steps_core(c, [&](int j) { return inners[j]->d; }, k, ci, inners[0]->scale, elts, gk, out);
}
// the same over k terms laid out contiguously in caller device memory (term j at src + j 2 l N words,
// l = L0 + 1 - chain_index), e.g. the slice a reduce-scatter handed this rank
extern "C" fhs_status fhs_bsgs_giant_steps_device(fhs_context* c, const uint64_t* src, int k, int chain_index,
                                                  double scale, const uint64_t* elts, const fhs_galois_keys* gk,
                                                  fhs_ciphertext** out) {
    ENTER(c);
    if (!src || !elts || !gk || !out) return fail(FHS_ERR_INVALID, "null argument");
    if (k < 1 || k > 511) return fail(FHS_ERR_INVALID, "bsgs_giant_steps: 1 <= k <= 511");
    if (chain_index < 1 || chain_index > c->L0) return fail(FHS_ERR_LEVEL, "bsgs_giant_steps: bad chain index");
    const size_t W = 2 * (size_t)(c->L0 + 1 - chain_index) * c->N;
    return giant_steps_core(c, [&](int j) { return src + (size_t)j * W; }, k, chain_index, scale, elts, gk, out);
}

extern "C" fhs_status fhs_linear_transform(fhs_context* c, const fhs_ciphertext* const* baby, int G,
                                           const fhs_plaintext* const* pts, int D, int B, const uint64_t* giant_elts,
                                           const fhs_galois_keys* gk, int rescale, fhs_ciphertext** out) {
    ENTER(c);
    if (!pts || !gk || !out || !baby || !giant_elts) return fail(FHS_ERR_INVALID, "null argument");
    if (B < 1 || D != B * G) return fail(FHS_ERR_INVALID, "linear_transform: expects D = B * G plaintexts");
    std::vector<const uint64_t*> p(D);
    for (int k = 0; k < D; ++k) {
        if (!pts[k] || pts[k]->ci != baby[0]->ci) return fail(FHS_ERR_LEVEL, "linear_transform: plaintext at a different chain index");
        if (!scales_close(pts[k]->scale, pts[0]->scale)) return fail(FHS_ERR_SCALE, "linear_transform: plaintext scales differ");
    }
    const int ptl = pts_ptl(c, pts, D);
    for (int k = 0; k < D; ++k) {
        p[k] = pts[k]->dc;
        if (!ptl) HIPCHK(pt_dense(c, pts[k], &p[k]), "linear_transform");
    }
    for (int g = 0; g < B; ++g)
        if ((giant_elts[g] & 1) == 0 || giant_elts[g] >= 2 * c->N) return fail(FHS_ERR_INVALID, "linear_transform: bad Galois element");
    return bsgs_core(c, baby, G, p.data(), D, B, baby[0]->ci, pts[0]->scale, gk, out, giant_elts, rescale != 0, ptl);
}

// ============================================================================ bootstrapping primitives
// exact residue of the integer-valued double p modulo q
static uint64_t dbl_int_mod(double p, uint64_t q) {
    const bool neg = p < 0;
    const double a = std::fabs(p);
    uint64_t r;
    if (a < 18446744073709551616.0) {
        r = (uint64_t)a % q;
    } else {
        int e;
        const double f = std::frexp(a, &e);              // a = f 2^e, f in [0.5, 1)
        const uint64_t m = (uint64_t)std::ldexp(f, 53);  // exact 53-bit mantissa
        r = h_mulmod(m % q, h_pow(2, (uint64_t)(e - 53), q), q);
    }
    return neg && r ? q - r : r;
}
static fhs_status scalar_consts(fhs_context* c, double v, int l, fhs::ScalarConsts& K) {
    if (!std::isfinite(v)) return fail(FHS_ERR_INVALID, "constant is not finite");
    if (l > fhs::kMaxScalarLimbs) return fail(FHS_ERR_INVALID, "too many limbs for a constant op");
    const double p = std::round(v);                      // half away from zero
    for (int i = 0; i < l; ++i) {
        K.v[i] = dbl_int_mod(p, c->q[i]);
        K.vs[i] = h_shoup(K.v[i], c->q[i]);
    }
    return FHS_OK;
}
extern "C" fhs_status fhs_multiply_const(fhs_context* c, const fhs_ciphertext* a, double value, double const_scale,
                                         fhs_ciphertext** out) {
    ENTER(c);
    if (!a || !out) return fail(FHS_ERR_INVALID, "null argument");
    LIVE(a);
    if (!(const_scale > 0) || !std::isfinite(const_scale)) return fail(FHS_ERR_INVALID, "multiply_const: bad scale");
    fhs::ScalarConsts K;
    fhs_status s = scalar_consts(c, value * const_scale, a->l, K);
    if (s != FHS_OK) return s;
    NEW_CT(r, a->ncomp, a->ci, a->scale * const_scale);
    HIPCHK(fhs::launch_scalar(c->T, fhs::SCALAR_MUL, a->d, r->d, a->ncomp, a->l, K, c->st), "multiply_const");
    *out = r.release();
    return FHS_OK;
}
extern "C" fhs_status fhs_add_const(fhs_context* c, const fhs_ciphertext* a, double value, fhs_ciphertext** out) {
    ENTER(c);
    if (!a || !out) return fail(FHS_ERR_INVALID, "null argument");
    LIVE(a);
    fhs::ScalarConsts K;
    fhs_status s = scalar_consts(c, value * a->scale, a->l, K);
    if (s != FHS_OK) return s;
    NEW_CT(r, a->ncomp, a->ci, a->scale);
    HIPCHK(fhs::launch_scalar(c->T, fhs::SCALAR_ADD, a->d, r->d, a->ncomp, a->l, K, c->st), "add_const");
    *out = r.release();
    return FHS_OK;
}
extern "C" fhs_status fhs_mod_raise(fhs_context* c, const fhs_ciphertext* a, fhs_ciphertext** out) {
    ENTER(c);
    if (!a || !out) return fail(FHS_ERR_INVALID, "null argument");
    LIVE(a);
    if (a->ncomp != 2) return fail(FHS_ERR_INVALID, "mod_raise expects a 2-component ciphertext");
    NEW_CT(r, 2, 1, a->scale);
    uint64_t* scr = nullptr;
    HIPCHK(scratch(c, fhs_context::SCR_RESCALE, 16ull * c->N, &scr), "mod_raise");
    HIPCHK(fhs::launch_mod_raise(c->T, a->d, a->l, r->d, scr, 2, c->st), "mod_raise");
    *out = r.release();
    return FHS_OK;
}

// ---- EvalMod orchestration in C++ (ckks_bootstrapper._evalmod, pyPhantom/bootstrap.py).  The same
// op sequence as the Python restatement (which the oracle runs): ~300 small ops per EvalMod, whose
// per-call Python overhead dominated the bootstrap.  Every double expression mirrors the Python one
// (same IEEE operations in the same order), so the limbs are identical.
namespace {
struct EmErr {
    fhs_status s;
};
inline void em_try(fhs_status s) {
    if (s != FHS_OK) throw EmErr{s};
}

struct EvalMod {
    fhs_context* c;
    const fhs_relin_key* rk;
    std::map<int, Ct> own;   // T_k computed here (T_1 is borrowed)
    std::map<int, const fhs_ciphertext*> T;

    double q_drop(int ci) const { return (double)c->q[c->L0 - ci]; }   // Bootstrapper._q_drop
    Ct mod_switch(const fhs_ciphertext* a, int ci) {
        fhs_ciphertext* r;
        em_try(fhs_mod_switch_to(c, a, ci, &r));
        return Ct(r);
    }
    Ct mul(const fhs_ciphertext* a, const fhs_ciphertext* b) {   // Bootstrapper._mul
        const int ci = std::max(a->ci, b->ci);
        Ct ta, tb;
        if (a->ci < ci) {
            ta = mod_switch(a, ci);
            a = ta.p;
        }
        if (b->ci < ci) {
            tb = mod_switch(b, ci);
            b = tb.p;
        }
        fhs_ciphertext *m, *r, *s;
        em_try(fhs_multiply(c, a, b, &m));
        Ct M(m);
        em_try(fhs_relinearize(c, M.p, rk, &r));
        Ct R(r);
        em_try(fhs_rescale_to_next(c, R.p, &s));
        return Ct(s);
    }
    Ct add(const fhs_ciphertext* a, const fhs_ciphertext* b) {
        fhs_ciphertext* r;
        em_try(fhs_add(c, a, b, &r));
        return Ct(r);
    }
    Ct sub(const fhs_ciphertext* a, const fhs_ciphertext* b) {
        fhs_ciphertext* r;
        em_try(fhs_sub(c, a, b, 0, &r));
        return Ct(r);
    }
    Ct add_const(const fhs_ciphertext* a, double v) {
        fhs_ciphertext* r;
        em_try(fhs_add_const(c, a, v, &r));
        return Ct(r);
    }
    // value * a landing exactly at (ci, scale): Bootstrapper._scalar
    Ct scalar(const fhs_ciphertext* a, double value, int ci, double scale) {
        if (a->ci > ci - 1) throw EmErr{fail(FHS_ERR_LEVEL, "evalmod: scalar product target level too low")};
        Ct t;
        if (a->ci < ci - 1) {
            t = mod_switch(a, ci - 1);
            a = t.p;
        }
        fhs_ciphertext *m, *r;
        em_try(fhs_multiply_const(c, a, value, scale * q_drop(ci - 1) / a->scale, &m));
        Ct M(m);
        em_try(fhs_rescale_to_next(c, M.p, &r));
        r->scale = scale;
        return Ct(r);
    }
    // Bootstrapper._align: borrowed when already there, else a scalar product by 1.0
    const fhs_ciphertext* align(const fhs_ciphertext* a, int ci, double scale, Ct& hold) {
        if (a->ci == ci && std::fabs(a->scale - scale) <= 1e-9 * scale) return a;
        hold = scalar(a, 1.0, ci, scale);
        return hold.p;
    }
    static int bitlen(int k) {
        int b = 0;
        while (k >> b) ++b;
        return b;
    }
    const fhs_ciphertext* get(int k) {   // Bootstrapper._cheb_basis.get
        auto it = T.find(k);
        if (it != T.end()) return it->second;
        const int a = (k & (k - 1)) ? 1 << (bitlen(k) - 1) : k / 2, b = k - a;
        Ct out;
        if (a == b) {
            const fhs_ciphertext* ta = get(a);
            Ct P = mul(ta, ta);
            Ct P2 = add(P.p, P.p);
            out = add_const(P2.p, -1.0);
        } else {
            const fhs_ciphertext* ta = get(a);
            const fhs_ciphertext* tb = get(b);
            Ct P = mul(ta, tb);
            Ct P2 = add(P.p, P.p);
            Ct hold;
            const fhs_ciphertext* d = align(get(a - b), P2.p->ci, P2.p->scale, hold);
            out = sub(P2.p, d);
        }
        const fhs_ciphertext* r = out.p;
        own[k] = std::move(out);
        T[k] = r;
        return r;
    }
    // Bootstrapper._cheb_eval: sum_k c_k T_k landing exactly at (ci, scale)
    Ct cheb(std::vector<double> cf, int ci, double scale) {
        int deg = (int)cf.size() - 1;
        while (deg > 0 && cf[deg] == 0.0) --deg;
        if (deg < 8) {
            std::vector<int> ks;
            for (int k = 1; k <= deg; ++k)
                if (cf[k] != 0.0) ks.push_back(k);
            if (ks.empty()) ks.push_back(1);
            Ct acc;
            for (int k : ks) {
                Ct t = scalar(get(k), k <= deg ? cf[k] : 0.0, ci, scale);
                acc = acc.p ? add(acc.p, t.p) : std::move(t);
            }
            return cf[0] != 0.0 ? add_const(acc.p, cf[0]) : std::move(acc);
        }
        const int m = 1 << (bitlen(deg) - 1);
        // cheb_split: T_{m+j} = 2 T_m T_j - T_{m-j} (j >= 1), T_m = T_m T_0
        std::vector<double> c2(cf.begin(), cf.begin() + deg + 1);
        c2.resize(2 * m, 0.0);
        std::vector<double> H(m), L(c2.begin(), c2.begin() + m);
        H[0] = c2[m];
        for (int j = 1; j < m; ++j) H[j] = 2.0 * c2[m + j];
        for (int j = 1; j < m; ++j) L[m - j] -= c2[m + j];
        const fhs_ciphertext* Tm = get(m);
        Ct h = cheb(H, ci - 1, scale * q_drop(ci - 1) / Tm->scale);
        Ct P = mul(h.p, Tm);
        P.p->scale = scale;
        Ct Lc = cheb(L, ci, scale);
        return add(P.p, Lc.p);
    }
};
}  // namespace

extern "C" fhs_status fhs_bootstrap_evalmod(fhs_context* c, const fhs_ciphertext* y, const fhs_relin_key* rk,
                                            const double* cc, const double* cs, int ncoef, int r, int cheb_depth,
                                            fhs_ciphertext** out) {
    ENTER(c);
    if (!y || !rk || !cc || !cs || !out || ncoef < 1 || r < 1) return fail(FHS_ERR_INVALID, "evalmod: bad argument");
    LIVE(y);
    try {
        EvalMod e{c, rk, {}, {}};
        e.T[1] = y;
        for (int k : {2, 3, 4, 5, 6, 7, 8, 16, 32}) e.get(k);
        const int ci = y->ci + cheb_depth;
        Ct cv = e.cheb(std::vector<double>(cc, cc + ncoef), ci, y->scale);
        Ct sv = e.cheb(std::vector<double>(cs, cs + ncoef), ci, y->scale);
        for (int step = 0; step < r; ++step) {   // (c, s) -> ((c + s)(c - s), 2 c s)
            Ct P = e.mul(cv.p, sv.p);
            if (step < r - 1) {
                Ct a = e.add(cv.p, sv.p), b = e.sub(cv.p, sv.p);
                cv = e.mul(a.p, b.p);
            }
            sv = e.add(P.p, P.p);
        }
        *out = sv.release();
        return FHS_OK;
    } catch (const EmErr& err) {
        return err.s;
    }
}

extern "C" fhs_status fhs_host_alloc(uint64_t bytes, void** ptr) {
    if (!ptr) return fail(FHS_ERR_INVALID, "null argument");
    HIPCHK(hipHostMalloc(ptr, bytes ? bytes : 8, hipHostMallocDefault), "pinned host allocation");
    return FHS_OK;
}
extern "C" fhs_status fhs_host_free(void* ptr) {
    if (ptr) HIPCHK(hipHostFree(ptr), "pinned host free");
    return FHS_OK;
}
extern "C" fhs_status fhs_offload_plaintexts(fhs_context* c, const fhs_plaintext* const* pts, int count, uint64_t* host) {
    ENTER(c);
    if (!pts || !host || count < 1) return fail(FHS_ERR_INVALID, "offload: bad args");
    const size_t b = pt_bytes(pts[0]);
    for (int k = 0; k < count; ++k) {
        if (pts[k]->l != pts[0]->l) return fail(FHS_ERR_LEVEL, "offload: plaintexts at different levels");
        PT_DENSE(pd, pts[k], "offload");
        HIPCHK(hipMemcpyAsync((char*)host + (size_t)k * b, pd, b, hipMemcpyDeviceToHost, c->st), "offload");
    }
    HIPCHK(hipStreamSynchronize(c->st), "offload");
    return FHS_OK;
}
extern "C" fhs_status fhs_upload_plaintexts(fhs_context* c, const uint64_t* host, int count, int ci, double scale,
                                            fhs_plaintext** outs) {
    ENTER(c);
    if (!host || !outs || count < 1) return fail(FHS_ERR_INVALID, "upload: bad args");
    BatchOut bo(outs, (size_t)count);
    fhs_status s0 = new_pts(c, (size_t)count, ci, scale, outs);
    if (s0 != FHS_OK) return s0;
    for (int k = 0; k < count; ++k) {
        fhs_plaintext* pt = outs[k];
        HIPCHK(hipMemcpyAsync(pt->d, host + (size_t)k * pt->l * c->N, pt_bytes(pt), hipMemcpyHostToDevice, c->st), "upload");
    }
    HIPCHK(hipStreamSynchronize(c->st), "upload");
    return bo.keep(FHS_OK);
}
extern "C" fhs_status fhs_bsgs_from_cpu(fhs_context* c, const fhs_ciphertext* const* baby, int G, const uint64_t* host,
                                        int D, int B, int ci, double scale, const fhs_galois_keys* gk,
                                        fhs_ciphertext** out) {
    ENTER(c);
    if (!baby || !host || !gk || !out) return fail(FHS_ERR_INVALID, "null argument");
    if (ci != baby[0]->ci) return fail(FHS_ERR_LEVEL, "bsgs_from_cpu: diagonals at a different chain index");
    for (int b = 0; b < G; ++b) LIVE(baby[b]);
    const int l = c->L0 + 1 - ci;
    const size_t bytes = 8ull * D * l * c->N;
    DevTmp dev(c);
    HIPCHK(dev.alloc(bytes), "bsgs_from_cpu staging");
    HIPCHK(hipMemcpyAsync(dev.p, host, bytes, hipMemcpyHostToDevice, c->st), "bsgs_from_cpu upload");
    std::vector<const uint64_t*> p(D);
    for (int k = 0; k < D; ++k) p[k] = dev.p + (size_t)k * l * c->N;
    return bsgs_core(c, baby, G, p.data(), D, B, ci, scale, gk, out);
}

// ============================================================================ measurement hooks
extern "C" fhs_status fhs_random_plaintexts(fhs_context* c, uint64_t seed, int count, int ci, double scale,
                                            fhs_plaintext** outs) {
    ENTER(c);
    if (!outs || count < 1) return fail(FHS_ERR_INVALID, "random_plaintexts: bad args");
    BatchOut bo(outs, (size_t)count);
    fhs_status s0 = new_pts(c, (size_t)count, ci, scale, outs);
    if (s0 != FHS_OK) return s0;
    for (int k = 0; k < count; ++k) {
        fhs_plaintext* pt = outs[k];
        HIPCHK(fhs::launch_sample(c->T, fhs::SAMPLE_TESTDATA, PrfKey{}, sm64(seed ^ sm64((7ull << 56) | (uint64_t)k)), pt->d, pt->l, c->st), "random_plaintexts");
    }
    return bo.keep(FHS_OK);
}
extern "C" fhs_status fhs_event_record(fhs_context* c, void** ev) {
    ENTER(c);
    hipEvent_t e = ev_get(c->device);
    if (!e) return fail(FHS_ERR_HIP, "event: hipEventCreate failed");
    HIPCHK(hipEventRecord(e, c->st), "event");
    *ev = (void*)e;
    return FHS_OK;
}
extern "C" fhs_status fhs_event_elapsed(void* a, void* b, float* ms) {
    HIPCHK(hipEventSynchronize((hipEvent_t)b), "event sync");
    HIPCHK(hipEventElapsedTime(ms, (hipEvent_t)a, (hipEvent_t)b), "event elapsed");
    return FHS_OK;
}
extern "C" fhs_status fhs_event_destroy(void* e) {
    ev_put((hipEvent_t)e);   // back to the pool (events are reused, not destroyed)
    return FHS_OK;
}
static void timer_rec(void* vc, int id, int begin, hipStream_t st) {
    auto* c = static_cast<fhs_context*>(vc);
    if (!(c->timer_mask & (1u << id))) return;
    hipEvent_t e = ev_get(c->device);
    if (!e) return;
    hipEventRecord(e, st);
    if (begin) {
        if (c->timer_open[id]) ev_put(c->timer_open[id]);
        c->timer_open[id] = e;
    } else if (c->timer_open[id]) {
        c->timer_pairs[id].push_back({c->timer_open[id], e});
        c->timer_open[id] = nullptr;
    } else {
        ev_put(e);
    }
}
// Arms the timer for the kernels in `mask` (bit i = fhs::KernelId i) after reporting, for kernel
// `kernel_id`, the time and launch count accumulated since the last reset.
extern "C" fhs_status fhs_kernel_timer(fhs_context* c, int kernel_id, float* ms, int* launches, int reset) {
    ENTER(c);
    HIPCHK(hipStreamSynchronize(c->st), "timer sync");
    if ((int)c->timer_pairs.size() < fhs::KID_COUNT) {
        c->timer_pairs.resize(fhs::KID_COUNT);
        c->timer_open.assign(fhs::KID_COUNT, nullptr);
        c->ktimer = fhs::KTimer{c, timer_rec};
    }
    float tot = 0.f;
    int n = 0;
    if (kernel_id >= 0 && kernel_id < fhs::KID_COUNT)
        for (auto& pr : c->timer_pairs[kernel_id]) {
            float t = 0.f;
            if (hipEventElapsedTime(&t, pr.first, pr.second) == hipSuccess) { tot += t; ++n; }
        }
    if (ms) *ms = tot;
    if (launches) *launches = n;
    if (reset) {
        for (auto& v : c->timer_pairs) {
            for (auto& pr : v) { ev_put(pr.first); ev_put(pr.second); }
            v.clear();
        }
    }
    return FHS_OK;
}
extern "C" fhs_status fhs_kernel_timer_arm(fhs_context* c, uint32_t mask) {
    ENTER(c);
    if (c->timer_pairs.size() < (size_t)fhs::KID_COUNT) {
        c->timer_pairs.resize(fhs::KID_COUNT);
        c->timer_open.assign(fhs::KID_COUNT, nullptr);
        c->ktimer = fhs::KTimer{c, timer_rec};
    }
    c->timer_mask = mask;
    if (mask) ev_reserve(c->device, 2048);   // created here, not between the timed launches
    return FHS_OK;
}
// staging-ring statistics (tests / diagnostics): segment re-entries, and how many had to wait
extern "C" fhs_status fhs_staging_stats(fhs_context* c, uint64_t* reentries, uint64_t* blocked) {
    ENTER(c);
    if (reentries) *reentries = c->ring_waits;
    if (blocked) *blocked = c->ring_blocked;
    return FHS_OK;
}
// device-to-device copy of a ciphertext's limbs into caller memory (RCCL interop); synchronises
static fhs_status copy_to_device(fhs_context* c, const fhs_ciphertext* ct, void* dst, bool sync) {
    if (!ct || !dst) return fail(FHS_ERR_INVALID, "null argument");
    LIVE(ct);
    HIPCHK(hipMemcpyAsync(dst, ct->d, ct_bytes(ct), hipMemcpyDeviceToDevice, c->st), "copy_to_device");
    if (sync) HIPCHK(hipStreamSynchronize(c->st), "copy_to_device");
    return FHS_OK;
}
static fhs_status from_device(fhs_context* c, const void* src, int ncomp, int ci, double scale, fhs_ciphertext** out,
                              bool sync) {
    if (!src || !out) return fail(FHS_ERR_INVALID, "null argument");
    NEW_CT(ct, ncomp, ci, scale);
    HIPCHK(hipMemcpyAsync(ct->d, src, ct_bytes(ct.p), hipMemcpyDeviceToDevice, c->st), "from_device");
    if (sync) HIPCHK(hipStreamSynchronize(c->st), "from_device");
    *out = ct.release();
    return FHS_OK;
}
extern "C" fhs_status fhs_ciphertext_copy_to_device(fhs_context* c, const fhs_ciphertext* ct, void* dst) {
    ENTER(c);
    return copy_to_device(c, ct, dst, true);
}
extern "C" fhs_status fhs_ciphertext_from_device(fhs_context* c, const void* src, int ncomp, int ci, double scale,
                                                 fhs_ciphertext** out) {
    ENTER(c);
    return from_device(c, src, ncomp, ci, scale, out, true);
}
extern "C" fhs_status fhs_ciphertext_copy_to_device_async(fhs_context* c, const fhs_ciphertext* ct, void* dst) {
    ENTER(c);
    return copy_to_device(c, ct, dst, false);
}
extern "C" fhs_status fhs_ciphertext_from_device_async(fhs_context* c, const void* src, int ncomp, int ci, double scale,
                                                       fhs_ciphertext** out) {
    ENTER(c);
    return from_device(c, src, ncomp, ci, scale, out, false);
}
extern "C" fhs_status fhs_context_stream(fhs_context* c, void** stream) {
    ENTER(c);
    if (!stream) return fail(FHS_ERR_INVALID, "null argument");
    *stream = (void*)c->st;
    return FHS_OK;
}

// x (any 64-bit value, or a value < 2m when canonical is asked) congruent to want (< m)?
static bool x_ok(uint64_t x, uint64_t want, uint64_t m, bool lt2m) {
    return (!lt2m || x < 2 * m) && x % m == want;
}
// The ModUp X form's arithmetic on the host (the same __host__ __device__ routines the kernels run):
// y3 (residues of a 3-prime digit q3, after the inverse-hat scaling) -> the centred digit value mod m.
// For a 59-bit target the kernels' convert3x_b59 (folded and unfolded) must give congruent values.
extern "C" fhs_status fhs_debug_modup_xform(const uint64_t* q3, const uint64_t* y3, uint64_t m, uint64_t* out) {
    if (!q3 || !y3 || !out) return FHS_ERR_INVALID;
    const uint64_t w = pm_word(m, 14);
    if (!w || !conv_pm_ok(m, 3)) return fail(FHS_ERR_INVALID, "debug_modup_xform: target not on the pseudo-Mersenne fold");
    for (int u = 0; u < 3; ++u)   // centered_x_pack has three rounding thresholds: S < 3 Q_S needs y < q
        if (y3[u] >= q3[u]) return fail(FHS_ERR_INVALID, "debug_modup_xform: residues must be < q");
    const uint64_t pr[4] = {q3[0], q3[1], q3[2], m};
    uint64_t xd[32] = {0}, xt[16] = {0};
    modup_xform_tables(pr, 4, 3, 1, xd, xt);
    uint64_t words[3];
    centered_x_pack(y3, xd, words);
    const uint64_t* t = xt + 12;
    if (t[0] >= (1ull << 30)) return fail(FHS_ERR_INVALID, "debug_modup_xform: 2^60 mod m >= 2^30 (no X form)");
    const uint64_t x = convert3x_value(words[0], words[1], words[2], (uint32_t)t[0], unpack30(t[1]), t[2],
                                       (unsigned)(w & 127), (unsigned)(w >> 8));
    if (x >= 2 * m) return fail(FHS_ERR_INVALID, "debug_modup_xform: result above 2m");
    *out = x >= m ? x - m : x;
    if (b59_prime(m)) {
        const uint32_t d = (uint32_t)((1ull << 59) - m);
        for (int canon = 0; canon < 2; ++canon)
            if (!x_ok(convert3x_b59(words[0], words[1], words[2], (uint32_t)t[0], unpack30(t[1]), t[2], d, canon), *out,
                      m, canon))
                return fail(FHS_ERR_INVALID, "debug_modup_xform: convert3x_b59 disagrees");
    }
    return FHS_OK;
}
// ModDown's X form on the host (k_special_x + moddown_convert3x arithmetic): y3 (special residues < p_k,
// already scaled by inv(P/p_k)) -> (sum_k y_k P/p_k) mod q, the fast base conversion's value.
extern "C" fhs_status fhs_debug_moddown_xform(const uint64_t* p3, const uint64_t* y3, uint64_t q, uint64_t* out) {
    if (!p3 || !y3 || !out) return FHS_ERR_INVALID;
    const uint64_t w = pm_word(q, 14);
    if (!w || !conv_pm_ok(q, 3)) return fail(FHS_ERR_INVALID, "debug_moddown_xform: target not on the pseudo-Mersenne fold");
    for (int k = 0; k < 3; ++k)
        if (p3[k] >= (1ull << 59)) return fail(FHS_ERR_INVALID, "debug_moddown_xform: special primes must be < 2^59");
    for (int k = 0; k < 3; ++k)
        if (y3[k] >= p3[k]) return fail(FHS_ERR_INVALID, "debug_moddown_xform: residues must be < p");
    uint64_t xd[32] = {0}, xt[4] = {0};
    for (int u = 0; u < 3; ++u) {   // as fhs_context_create's md_xd
        const hu128 h = (hu128)p3[(u + 1) % 3] * p3[(u + 2) % 3];
        xd[2 * u] = (uint64_t)h;
        xd[2 * u + 1] = (uint64_t)(h >> 64);
    }
    for (int i = 6; i < 15; ++i) xd[i] = ~0ull;
    modup_xform_tables(&q, 1, 0, 0, xd, xt);   // the target's weights only (no digit rows: L0 = 0)
    if (xt[0] >= (1ull << 30)) return fail(FHS_ERR_INVALID, "debug_moddown_xform: 2^60 mod q >= 2^30");
    uint64_t words[3];
    centered_x_pack(y3, xd, words);
    const uint64_t x = convert3x_value(words[0], words[1], words[2], (uint32_t)xt[0], unpack30(xt[1]), 0,
                                       (unsigned)(w & 127), (unsigned)(w >> 8));
    if (x >= 2 * q) return fail(FHS_ERR_INVALID, "debug_moddown_xform: result above 2q");
    *out = x >= q ? x - q : x;
    if (b59_prime(q)) {
        const uint32_t d = (uint32_t)((1ull << 59) - q);
        for (int canon = 0; canon < 2; ++canon)
            if (!x_ok(convert3x_b59(words[0], words[1], words[2], (uint32_t)xt[0], unpack30(xt[1]), 0, d, canon), *out,
                      q, canon))
                return fail(FHS_ERR_INVALID, "debug_moddown_xform: convert3x_b59 disagrees");
    }
    return FHS_OK;
}
extern "C" fhs_status fhs_debug_reduce128(uint64_t q, uint64_t lo, uint64_t hi, uint64_t* out, int* pm_used) {
    if (!out || q < 3) return FHS_ERR_INVALID;
    const uint64_t w = pm_word(q, 14);
    if (pm_used) *pm_used = w != 0;
    *out = w ? pm_reduce128(lo, hi, q, (unsigned)(w & 127), (unsigned)(w >> 8))
             : (uint64_t)((((hu128)hi << 64) | lo) % q);
    return FHS_OK;
}
