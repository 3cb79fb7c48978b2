// context.hip -- error string, per-device and private contexts, thread binding, the staging ring, per-thread copy streams, the device-memory pool,
// kh_dev_*, kh_sync, kh_trim, counters and timings.
#include <stdlib.h>
#include <algorithm>
#include <atomic>

#include "api_internal.hpp"
#include "env.hpp"

namespace kh {

static thread_local std::string g_err;
void set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
    g_err = buf;
}

// One context per device, created on first use and never destroyed (a destructor running after the HIP runtime has shut
// down would call into it).  A single process can therefore hold Vesta on GPU 0 and Pallas on GPU 1 (BASELINE config 5)
// or shard one MSM over all GPUs of the node (config 4) from its own threads; one-process-per-GPU works as before.
static Context* g_ctx[KH_MAX_DEVICES];
static std::mutex g_ctx_mu;
static int g_default_dev = -1;                 // first device initialised (guarded by g_ctx_mu)
static thread_local int tl_dev = -1;           // this thread's choice (kh_set_device / kh_init / DeviceScope); -1: process default
static thread_local int tl_hip_dev = -1;       // what this thread last passed to hipSetDevice

// A prover thread may take a context of its OWN for a stretch of work (kh_private_context_begin / _end; kh_prove does): own main stream, pipeline slots,
// workspaces and lock, so that several provers in one process neither queue their vector steps on one stream nor serialise their launches on one mutex
// (four single-prover processes: 177 proofs/s, four threads on the shared context: 128).  Private contexts are pooled per device and never destroyed,
// like the shared ones.  What belongs to an SRS HANDLE (its Lagrange-basis map, the claims on its openings' workspaces) has its own locks (kh_srs).
static thread_local Context* tl_private[KH_MAX_DEVICES];
static std::vector<Context*> g_private_pool[KH_MAX_DEVICES];           // idle private contexts (guarded by g_ctx_mu)
static std::atomic<int> g_private_made[KH_MAX_DEVICES];                 // private contexts ever created per device (they are never destroyed)
static int g_private_active[KH_MAX_DEVICES];                             // threads between kh_private_context_begin and _end per device (guarded by g_ctx_mu)
// a thread keeps the context it used last (its workspaces and staging ring stay warm for its next proof) and hands it to the pool when it
// exits -- no HIP call in the destructor, only the list
struct ThreadContextCache {
    Context* c[KH_MAX_DEVICES] = {nullptr};
    ~ThreadContextCache();
};
static thread_local ThreadContextCache tl_ctx_cache;

ThreadContextCache::~ThreadContextCache() {
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    for (int d = 0; d < KH_MAX_DEVICES; d++) if (c[d]) { g_private_pool[d].push_back(c[d]); c[d] = nullptr; }
}
static int current_device() {
    if (tl_dev >= 0) return tl_dev;
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    return g_default_dev;
}
static Context& shared_ctx_of(int dev) {
    if (dev < 0 || dev >= KH_MAX_DEVICES) dev = 0;
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    if (!g_ctx[dev]) g_ctx[dev] = new Context;
    return *g_ctx[dev];
}
static Context& ctx_of(int dev) {
    if (dev < 0 || dev >= KH_MAX_DEVICES) dev = 0;
    if (tl_private[dev]) return *tl_private[dev];
    return shared_ctx_of(dev);
}
Context& ctx() { return ctx_of(current_device()); }

// Small host -> device uploads as a KERNEL whose argument block carries the data (<= 3.5 KB by value): queueing an asynchronous copy costs the host ~10 us
// against ~5 us for a launch, and the vector steps of a proof -- token programs, pointer tables, constants: 20 such uploads before the opening -- are
// bound by the host's submission rate (tools/proof_timeline.py: ~10 us of idle GPU in front of every small copy).
namespace {
struct StageBlob { uint32_t w[896]; };
__global__ void k_stage_put(uint32_t* __restrict__ dst, StageBlob b, uint32_t nwords) {
    for (uint32_t i = threadIdx.x; i < nwords; i += blockDim.x) dst[i] = b.w[i];
}
__global__ void k_zero_words(uint32_t* __restrict__ dst, size_t nwords) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nwords) dst[i] = 0u;
}
__global__ void k_fill_elements(uint64_t* __restrict__ dst, uint64_t v0, uint64_t v1, uint64_t v2, uint64_t v3, size_t count) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) { dst[4 * i] = v0; dst[4 * i + 1] = v1; dst[4 * i + 2] = v2; dst[4 * i + 3] = v3; }
}
}  // namespace
int Context::stage_upload(void* dst_dev, std::initializer_list<std::pair<const void*, size_t>> parts) {
    size_t total = 0;
    for (const auto& pr : parts) total += pr.second;
    if (total == 0) return KH_OK;
    static const bool put_kernel = env_flag("KH_STAGE_PUT", true);
    if (put_kernel && total <= sizeof(StageBlob) && total % 4 == 0 && ((uintptr_t)dst_dev & 3) == 0) {
        StageBlob b;
        size_t o = 0;
        for (const auto& pr : parts) { if (pr.second) memcpy((char*)b.w + o, pr.first, pr.second); o += pr.second; }
        hipLaunchKernelGGL(k_stage_put, dim3(1), dim3(256), 0, stream, (uint32_t*)dst_dev, b, (uint32_t)(total / 4));
        KH_HIP(hipGetLastError());
        return KH_OK;
    }
    const size_t need = (total + 63) & ~(size_t)63;
    if (need > stage_cap / 4) {                       // a large table, or no ring yet: make room for many calls per turn
        const size_t cap = std::max<size_t>((size_t)1 << 20, 8 * need);
        if (cap > stage_cap) {
            KH_HIP(hipStreamSynchronize(stream));     // nothing in flight reads the old ring any more
            if (stage) (void)hipHostFree(stage);
            stage = nullptr; stage_cap = 0; stage_cur = 0;
            KH_HIP(hipHostMalloc((void**)&stage, cap, hipHostMallocDefault));
            stage_cap = cap;
        }
    }
    if (stage_cur + need > stage_cap) { KH_HIP(hipStreamSynchronize(stream)); stage_cur = 0; }
    char* h = stage + stage_cur;
    size_t o = 0;
    for (const auto& pr : parts) { if (pr.second) memcpy(h + o, pr.first, pr.second); o += pr.second; }
    stage_cur += need;
    KH_HIP(hipMemcpyAsync(dst_dev, h, total, hipMemcpyHostToDevice, stream));
    return KH_OK;
}

static int bind_thread(int dev) {
    if (tl_hip_dev != dev) { KH_HIP(hipSetDevice(dev)); tl_hip_dev = dev; }
    return KH_OK;
}
std::atomic<uint64_t>& counter(CounterId id) { static std::atomic<uint64_t> c[CNT_COUNT]; return c[id]; }
DeviceScope::DeviceScope(int device) : prev(tl_dev) {
    if (device >= 0) { tl_dev = device; if (tl_hip_dev != device && hipSetDevice(device) == hipSuccess) tl_hip_dev = device; }
}
DeviceScope::~DeviceScope() { tl_dev = prev; }

// streams, events and device facts of one context (the calling thread is bound to device_id, C.mu held or C not yet published)
static int init_context(Context& C, int device_id) {
    if (C.ready) return KH_OK;
    for (int i = 0; i < MSM_SLOTS; i++) {
        KH_HIP(hipStreamCreateWithFlags(&C.slot[i].stream, hipStreamNonBlocking));
        KH_HIP(hipEventCreateWithFlags(&C.slot[i].done, hipEventDisableTiming));
        int rc2 = C.slot[i].timer.init(); if (rc2) return rc2;
    }
    C.stream = C.slot[0].stream;         // four streams = the four hardware queues HIP gives a process by default; a fifth would share one
    KH_HIP(hipEventCreateWithFlags(&C.order_ev, hipEventDisableTiming));
    hipDeviceProp_t prop;
    KH_HIP(hipGetDeviceProperties(&prop, device_id));
    C.num_cus = prop.multiProcessorCount;
    C.lds_per_cu = prop.maxSharedMemoryPerMultiProcessor ? (size_t)prop.maxSharedMemoryPerMultiProcessor : (size_t)64 << 10;
    C.lds_per_block = prop.sharedMemPerBlock ? (size_t)prop.sharedMemPerBlock : (size_t)64 << 10;
    int rc = C.timer.init(); if (rc) return rc;
    C.device = device_id;
    C.ready = true;
    return KH_OK;
}
static int do_init(int device_id) {
    if (!(__builtin_cpu_supports("bmi2") && __builtin_cpu_supports("adx"))) {      // the host code is built with -mbmi2 -madx (__graft_entry__.py)
        set_error("this build needs a host CPU with BMI2 and ADX"); return KH_E_DEVICE;
    }
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        set_error("no HIP device available (%s); libkimchi_hip has no CPU fallback", e == hipSuccess ? "count=0" : hipGetErrorString(e));
        return KH_E_DEVICE;
    }
    if (device_id < 0) device_id = current_device();
    if (device_id < 0) {
        const char* lr = getenv("LOCAL_RANK");
        device_id = lr ? atoi(lr) % count : 0;
    }
    KH_REQUIRE(device_id < count && device_id < KH_MAX_DEVICES, "device %d out of range (count=%d)", device_id, count);
    Context& C = ctx_of(device_id);
    std::lock_guard<std::mutex> lk(C.mu);
    int rc = bind_thread(device_id); if (rc) return rc;
    if ((rc = init_context(C, device_id))) return rc;
    {
        std::lock_guard<std::mutex> g(g_ctx_mu);
        if (g_default_dev < 0) g_default_dev = device_id;
    }
    return KH_OK;
}
int ensure_init() {
    const int dev = current_device();
    if (dev < 0 || !ctx_of(dev).ready) return do_init(dev);
    return bind_thread(dev);
}

void collect_timings(Context& C, PhaseTimer& T) {
    C.last.clear();
    if (!T.created || !T.enabled) return;
    for (int i = 0; i < T.n; i++) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, T.ev[i], T.ev[i + 1]) == hipSuccess) C.last.emplace_back(T.names[i], ms);
    }
    float kms = 0.f;
    if (T.kname && hipEventElapsedTime(&kms, T.k0, T.k1) == hipSuccess) C.last.emplace_back(T.kname, kms);
}

}  // namespace kh

using namespace kh;

// one non-blocking copy stream per (host thread, device), created on first use
// (destroyed with the thread: a pool of short-lived worker threads must not leak a stream each)
struct ThreadCopyStreams {
    hipStream_t s[KH_MAX_DEVICES] = {nullptr};
    ~ThreadCopyStreams() {
        for (int d = 0; d < KH_MAX_DEVICES; d++)
            if (s[d]) { int cur = -1; if (hipGetDevice(&cur) == hipSuccess) { (void)hipSetDevice(d); (void)hipStreamDestroy(s[d]); (void)hipSetDevice(cur); } }
    }
};
hipStream_t kh::thread_copy_stream() {
    static thread_local ThreadCopyStreams tl;
    const int d = kh::ctx().device >= 0 && kh::ctx().device < KH_MAX_DEVICES ? kh::ctx().device : 0;
    if (!tl.s[d] && hipStreamCreateWithFlags(&tl.s[d], hipStreamNonBlocking) != hipSuccess) { kh::set_error("hipStreamCreate for a copy stream failed"); return nullptr; }
    return tl.s[d];
}

// the event behind the scalar upload of kh_msm_submit_host, per (host thread, device)
struct ThreadUploadEvents {
    hipEvent_t e[KH_MAX_DEVICES] = {nullptr};
    ~ThreadUploadEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};
hipEvent_t kh::thread_upload_event() {
    static thread_local ThreadUploadEvents tl;
    const int d = kh::ctx().device >= 0 && kh::ctx().device < KH_MAX_DEVICES ? kh::ctx().device : 0;
    if (!tl.e[d] && hipEventCreateWithFlags(&tl.e[d], hipEventDisableTiming) != hipSuccess) { kh::set_error("hipEventCreate for an upload event failed"); return nullptr; }
    return tl.e[d];
}

// kh_dev_alloc / kh_dev_free go through a small caching pool: hipFree synchronises the device and takes ~0.25 ms, and a prover frees
// ~15 column buffers per proof (3.8 ms of a 16 ms proof, measured with cProfile on proof_systems_amd/prover.py).  Freed blocks are
// kept per device, keyed by their (4 KiB-rounded) size, and handed out again to a request of nearly that size.  Within ONE context reuse is
// safe because every consumer of such buffers is either synchronous or ordered on that context's main stream.  Across contexts
// (kh_private_context_begin gives every prover thread its own streams) it is not: thread A may free a block with work still queued on its
// main stream and thread B would write into it from another stream.  A cached block therefore remembers the context that freed it; a request
// prefers a block of its own context, and one that takes another context's block first makes its main stream wait for an event recorded on
// the previous owner's main stream (everything that owner queued before the free precedes the event).  kh_trim empties the pool;
// KH_POOL_MAX_MB (default 2048: a 2^16 proof cycles ~0.6 GiB of column buffers) bounds what it may hold, KH_POOL_MAX_MB=0 disables it.
// A co-tenant of the process (PyTorch's allocator) that runs short of memory can ask for the cached blocks back with kh_trim(); the
// library itself trims before reporting an allocation failure.
namespace {
struct DevPool {
    std::mutex mu;
    struct Block { void* p; kh::Context* owner; };
    std::multimap<size_t, Block> free_blocks[KH_MAX_DEVICES];
    std::map<void*, std::pair<int, size_t>> live;          // pointer -> (device, rounded size)
    size_t cached[KH_MAX_DEVICES] = {0};
};
DevPool& dev_pool() { static DevPool p; return p; }
size_t pool_limit() { static const size_t lim = (size_t)env_int("KH_POOL_MAX_MB", 2048) << 20; return lim; }
}  // namespace
static void dev_pool_trim(int device) {
    DevPool& P = dev_pool();
    std::lock_guard<std::mutex> lk(P.mu);
    const int d = device >= 0 && device < KH_MAX_DEVICES ? device : 0;
    for (auto& kv : P.free_blocks[d]) (void)hipFree(kv.second.p);
    P.free_blocks[d].clear(); P.cached[d] = 0;
}

extern "C" {

int kh_device_count(void) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) return 0;
    return count;
}
int kh_init(int device_id) {
    int rc = do_init(device_id); if (rc) return rc;
    if (device_id >= 0) tl_dev = device_id;          // an explicit choice also becomes this thread's current device
    return KH_OK;
}
int kh_set_device(int device_id) {
    KH_REQUIRE(device_id >= 0, "kh_set_device: negative device id");
    int rc = do_init(device_id); if (rc) return rc;
    tl_dev = device_id;
    return KH_OK;
}
int kh_get_device(void) { return current_device(); }
// releases the caches a long-lived process accumulates on the current device: twiddle tables, LDE / scan / expression
// scratch, the slots' MSM workspaces (everything is re-created on demand)
int kh_trim(void) {
    int rc = ensure_init(); if (rc) return rc;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    for (int i = 0; i < MSM_SLOTS; i++) {
        KH_REQUIRE(!C.slot[i].busy, "kh_trim: an MSM is in flight (kh_msm_wait first)");
        KH_HIP(hipStreamSynchronize(C.slot[i].stream));
    }
    for (int i = 0; i < MSM_SLOTS; i++) {
        MsmSlot& S = C.slot[i];
        for (DevBuf* b : {&S.ws_scalars, &S.ws_digits, &S.ws_hist, &S.ws_cnt, &S.ws_off, &S.ws_ntask, &S.ws_toff, &S.ws_entries, &S.ws_partial, &S.ws_buckets,
                          &S.ws_seg, &S.ws_out, &S.ws_scan_tmp, &S.ws_biglist, &S.ws_points, &S.ws_order, &S.ws_chunks, &S.ws_handed, &S.ws_sync, &S.ws_mid,
                          &S.ws_b29, &S.ws_a1, &S.ws_l2, &S.ws_a2, &S.ws_xlist}) b->release();
    }
    C.ws_ntt_a.release(); C.ws_ntt_b.release();
    xfer_trim(C.device);
    dev_pool_trim(C.device);
    C.trim_scratch();
    // The twiddle tables belong to the DEVICE and are shared by every context on it: a private context of another thread may be between two
    // passes of a transform that reads them, and this call holds only its own context's lock.  They are dropped only while no private context
    // is ACTIVE on the device, and the registry lock is held across the free so that none can begin meanwhile (the old test --
    // "no private context was ever created" -- never became true again after the first kh_prove).
    {
        std::lock_guard<std::mutex> lk2(g_ctx_mu);
        if (g_private_active[C.device >= 0 && C.device < KH_MAX_DEVICES ? C.device : 0] == 0) ntt_trim(C);
    }
    return KH_OK;
}

int kh_private_context_begin(void) {
    int rc = ensure_init(); if (rc) return rc;
    const int dev = current_device();
    KH_REQUIRE(dev >= 0 && dev < KH_MAX_DEVICES, "no current device");
    KH_REQUIRE(!tl_private[dev], "kh_private_context_begin: this thread already has a private context on device %d", dev);
    Context& S = shared_ctx_of(dev);
    Context* c = tl_ctx_cache.c[dev];
    tl_ctx_cache.c[dev] = nullptr;
    if (!c) {
        std::lock_guard<std::mutex> lk(g_ctx_mu);
        if (!g_private_pool[dev].empty()) { c = g_private_pool[dev].back(); g_private_pool[dev].pop_back(); }
    }
    if (!c) {
        c = new (std::nothrow) Context;
        KH_REQUIRE(c, "out of memory");
        g_private_made[dev]++;
    }
    // init_context is idempotent (C.ready): a context that came back from the pool or the thread's cache half-initialised -- an earlier begin failed
    // part-way -- is completed here instead of being used with null streams.  Whatever fails below, the context goes back to the pool (never lost).
    auto give_back = [&](int status) { std::lock_guard<std::mutex> lk(g_ctx_mu); g_private_pool[dev].push_back(c); return status; };
    if ((rc = bind_thread(dev)) || (rc = init_context(*c, dev))) return give_back(rc);
    {   // whatever the caller queued on the shared context's main stream (uploads, index columns) is ordered before this context's work
        std::lock_guard<std::mutex> lk(S.mu);
        hipError_t e = hipEventRecord(S.order_ev, S.stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, S.order_ev, 0);
        if (e != hipSuccess) { set_error("kh_private_context_begin: ordering behind the shared context failed: %s", hipGetErrorString(e)); return give_back(KH_E_DEVICE); }
    }
    c->mark_async();                                      // ... and this context's side slots wait for its main stream in turn
    tl_private[dev] = c;
    { std::lock_guard<std::mutex> lk(g_ctx_mu); g_private_active[dev]++; }
    return KH_OK;
}
// Per-phase HIP events (kh_last_timings) on the calling thread's current context (its private one between kh_private_context_begin and _end).  OFF by
// default since round 5: an event recorded between two kernels costs the stream ~6-10 us of idle time (tools/proof_timeline.py) -- a proof queued ~60
// of them (10.2 -> 9.9 ms without), the pipelined MSM loop lost 1-4 %.  The Python binding's init() switches them on (its users are tools and tests).
int kh_set_phase_timers(int on) {
    int rc = ensure_init(); if (rc) return rc;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    C.timer.enabled = on != 0; C.timer.n = 0;
    for (int i = 0; i < MSM_SLOTS; i++) { C.slot[i].timer.enabled = on != 0; C.slot[i].timer.n = 0; }
    return KH_OK;
}
int kh_private_context_active(void) {
    const int dev = current_device();
    return dev >= 0 && dev < KH_MAX_DEVICES && tl_private[dev] != nullptr;
}
int kh_private_context_end(void) {
    const int dev = current_device();
    if (dev < 0 || dev >= KH_MAX_DEVICES || !tl_private[dev]) return KH_OK;
    Context* c = tl_private[dev];
    hipError_t e = hipSuccess;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        for (int i = 0; i < MSM_SLOTS && e == hipSuccess; i++) e = hipStreamSynchronize(c->slot[i].stream);      // nothing of this stretch is in flight afterwards
        c->main_dirty = false;
    }
    tl_private[dev] = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_ctx_mu);
        g_private_active[dev]--;
        if (!tl_ctx_cache.c[dev]) tl_ctx_cache.c[dev] = c; else g_private_pool[dev].push_back(c);
    }
    if (e != hipSuccess) { set_error("hipStreamSynchronize failed: %s", hipGetErrorString(e)); return KH_E_DEVICE; }
    return KH_OK;
}
const char* kh_last_error(void) { return g_err.c_str(); }

// ---------------------------------------------------------------------------------- device memory helpers
int kh_dev_alloc(void** ptr, size_t bytes) {
    KH_REQUIRE(ptr, "null ptr");
    int rc = ensure_init(); if (rc) return rc;
    const size_t want = ((bytes ? bytes : 1) + 4095) & ~(size_t)4095;
    const int d = ctx().device >= 0 && ctx().device < KH_MAX_DEVICES ? ctx().device : 0;
    DevPool& P = dev_pool();
    {
        Context* const me = &ctx_of(d);
        Context* prev = nullptr;
        std::unique_lock<std::mutex> lk(P.mu);
        auto lo = P.free_blocks[d].lower_bound(want), it = P.free_blocks[d].end();
        for (auto c = lo; c != P.free_blocks[d].end() && c->first <= want + want / 4; ++c) {
            if (it == P.free_blocks[d].end()) it = c;                      // the tightest fit, unless a block of this context fits too
            if (c->second.owner == me) { it = c; break; }
        }
        if (it != P.free_blocks[d].end()) {
            *ptr = it->second.p; prev = it->second.owner; P.live[*ptr] = {d, it->first}; P.cached[d] -= it->first;
            P.free_blocks[d].erase(it);
            lk.unlock();
            if (prev && prev != me) {                                      // another context's block: order this context behind that one's queued work
                // (behind its MAIN stream: a buffer handed to kh_msm_submit must not be freed before the ticket is waited for -- the side slots' streams
                //  are not part of the hand-over.)  A failure here gives the block back to the pool and leaves *ptr null.
                static thread_local hipEvent_t hand_over[KH_MAX_DEVICES] = {nullptr};
                hipError_t e = hipSuccess;
                if (!hand_over[d]) e = hipEventCreateWithFlags(&hand_over[d], hipEventDisableTiming);
                if (e == hipSuccess) {
                    std::lock_guard<std::mutex> g(me->mu);
                    e = hipEventRecord(hand_over[d], prev->stream);
                    if (e == hipSuccess) e = hipStreamWaitEvent(me->stream, hand_over[d], 0);
                    if (e == hipSuccess) me->mark_async();                  // ... and this context's side slots behind its main stream
                }
                if (e != hipSuccess) {
                    std::lock_guard<std::mutex> g2(P.mu);
                    auto lv = P.live.find(*ptr);
                    if (lv != P.live.end()) { P.free_blocks[d].emplace(lv->second.second, DevPool::Block{*ptr, prev}); P.cached[d] += lv->second.second; P.live.erase(lv); }
                    *ptr = nullptr;
                    set_error("kh_dev_alloc: ordering behind the previous owner of a pooled block failed: %s", hipGetErrorString(e));
                    return KH_E_DEVICE;
                }
            }
            return KH_OK;
        }
    }
    hipError_t e = hipMalloc(ptr, want);
    if (e != hipSuccess) {                                  // give the cached blocks back and retry once
        (void)hipGetLastError();
        dev_pool_trim(d);
        KH_HIP(hipMalloc(ptr, want));
    }
    std::lock_guard<std::mutex> lk(P.mu);
    P.live[*ptr] = {d, want};
    return KH_OK;
}
int kh_dev_free(void* ptr) {
    if (!ptr) return KH_OK;
    DevPool& P = dev_pool();
    {
        std::lock_guard<std::mutex> lk(P.mu);
        auto it = P.live.find(ptr);
        if (it != P.live.end()) {
            const int d = it->second.first; const size_t sz = it->second.second;
            P.live.erase(it);
            if (P.cached[d] + sz <= pool_limit()) { P.free_blocks[d].emplace(sz, DevPool::Block{ptr, &ctx_of(d)}); P.cached[d] += sz; return KH_OK; }
        }
    }
    KH_HIP(hipFree(ptr));
    return KH_OK;
}
// device-to-device copy on the main stream (ordered with kh_ntt_dev / kh_lde_dev / the vector steps; asynchronous)
int kh_dev_copy(void* dst_dev, const void* src_dev, size_t bytes) {
    int rc = ensure_init(); if (rc) return rc;
    if (bytes == 0) return KH_OK;
    KH_REQUIRE(dst_dev && src_dev, "kh_dev_copy: null pointer");
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    KH_HIP(hipMemcpyAsync(dst_dev, src_dev, bytes, hipMemcpyDeviceToDevice, C.stream));
    if (hipEventRecord(C.order_ev, C.stream) == hipSuccess) C.main_dirty = true;
    return KH_OK;
}
int kh_dev_memset_zero(void* dst_dev, size_t bytes) {
    int rc = ensure_init(); if (rc) return rc;
    if (bytes == 0) return KH_OK;
    KH_REQUIRE(dst_dev, "kh_dev_memset_zero: null pointer");
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    if (bytes <= ((size_t)1 << 16) && bytes % 4 == 0 && ((uintptr_t)dst_dev & 3) == 0) {       // small: a launch is cheaper to queue than a memset node
        hipLaunchKernelGGL(k_zero_words, dim3((unsigned)((bytes / 4 + 255) / 256)), dim3(256), 0, C.stream, (uint32_t*)dst_dev, bytes / 4);
        KH_HIP(hipGetLastError());
    } else KH_HIP(hipMemsetAsync(dst_dev, 0, bytes, C.stream));
    if (hipEventRecord(C.order_ev, C.stream) == hipSuccess) C.main_dirty = true;
    return KH_OK;
}
// count field elements (or any 32-byte records) set to `value`, queued on the main stream: the value travels in the kernel's arguments (no staging copy)
int kh_dev_fill_elements(uint64_t* dst_dev, const uint64_t value[4], size_t count) {
    int rc = ensure_init(); if (rc) return rc;
    if (count == 0) return KH_OK;
    KH_REQUIRE(dst_dev && value, "kh_dev_fill_elements: null pointer");
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    hipLaunchKernelGGL(k_fill_elements, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, C.stream, dst_dev, value[0], value[1], value[2], value[3], count);
    KH_HIP(hipGetLastError());
    C.mark_async();
    return KH_OK;
}
// The library's streams are non-blocking (they do not synchronise with the null stream hipMemcpy uses), so both copies
// first wait for the main stream: an asynchronous kh_ntt_dev / kh_lde_dev on this buffer is complete before it is read
// or overwritten.
// The copies themselves run on a per-thread non-blocking stream, not on the legacy stream.
int kh_dev_upload(void* dst_dev, const void* src_host, size_t bytes) {
    int rc = ensure_init(); if (rc) return rc;
    if (bytes == 0) return KH_OK;
    hipStream_t cs = thread_copy_stream(); if (!cs) return KH_E_DEVICE;
    KH_HIP(hipStreamSynchronize(ctx().stream));
    KH_HIP(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, cs));
    KH_HIP(hipStreamSynchronize(cs));
    return KH_OK;
}
int kh_dev_upload_2d(void* dst_dev, size_t dst_pitch, const void* src_host, size_t src_pitch, size_t width, size_t rows) {
    int rc = ensure_init(); if (rc) return rc;
    if (width == 0 || rows == 0) return KH_OK;
    KH_REQUIRE(dst_dev && src_host && dst_pitch >= width && src_pitch >= width, "kh_dev_upload_2d: bad argument");
    hipStream_t cs = thread_copy_stream(); if (!cs) return KH_E_DEVICE;
    KH_HIP(hipStreamSynchronize(ctx().stream));
    KH_HIP(hipMemcpy2DAsync(dst_dev, dst_pitch, src_host, src_pitch, width, rows, hipMemcpyHostToDevice, cs));
    KH_HIP(hipStreamSynchronize(cs));
    return KH_OK;
}
int kh_dev_upload_2d_unordered(void* dst_dev, size_t dst_pitch, const void* src_host, size_t src_pitch, size_t width, size_t rows) {
    int rc = ensure_init(); if (rc) return rc;
    if (width == 0 || rows == 0) return KH_OK;
    KH_REQUIRE(dst_dev && src_host && dst_pitch >= width && src_pitch >= width, "kh_dev_upload_2d_unordered: bad argument");
    hipStream_t cs = thread_copy_stream(); if (!cs) return KH_E_DEVICE;
    KH_HIP(hipMemcpy2DAsync(dst_dev, dst_pitch, src_host, src_pitch, width, rows, hipMemcpyHostToDevice, cs));
    KH_HIP(hipStreamSynchronize(cs));
    return KH_OK;
}
int kh_dev_download(void* dst_host, const void* src_dev, size_t bytes) {
    int rc = ensure_init(); if (rc) return rc;
    if (bytes == 0) return KH_OK;
    hipStream_t cs = thread_copy_stream(); if (!cs) return KH_E_DEVICE;
    KH_HIP(hipStreamSynchronize(ctx().stream));
    KH_HIP(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, cs));
    KH_HIP(hipStreamSynchronize(cs));
    return KH_OK;
}
int kh_sync(void) {
    int rc = ensure_init(); if (rc) return rc;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    for (int i = 0; i < MSM_SLOTS; i++) KH_HIP(hipStreamSynchronize(C.slot[i].stream));
    C.main_dirty = false;
    if (C.timer.n > 0) collect_timings(C, C.timer);
    C.timer.n = 0;
    return KH_OK;
}
uint64_t kh_counter(const char* name) {
    if (!name) return 0;
    for (int i = 0; i < CNT_COUNT; i++) if (!strcmp(name, COUNTER_NAMES[i])) return counter((CounterId)i).load(std::memory_order_relaxed);
    return 0;
}
int kh_last_timings(const char** names, float* ms, int cap) {
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    int n = 0;
    for (auto& kv : C.last) { if (n >= cap) break; names[n] = kv.first; ms[n] = kv.second; n++; }     // string literals: valid forever
    return n;
}
}  // extern "C"
