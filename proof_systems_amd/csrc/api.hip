// api.hip -- the extern "C" boundary declared in include/kimchi_hip.h.
#include <stdlib.h>
#include <algorithm>
#include <chrono>
#include <atomic>
#include <map>
#include <memory>

#include "common.hpp"
#include "host_ec.hpp"
#include "msm.hpp"

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
// like the shared ones.  What belongs to an SRS HANDLE (its Lagrange-basis map, the one opening it can run at a time) has its own locks (kh_srs).
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
    static const bool put_kernel = !(getenv("KH_STAGE_PUT") && atoi(getenv("KH_STAGE_PUT")) == 0);
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

struct LagrangeChunk { DevBuf pts; DevBuf inf; bool has_inf = false; size_t n = 0; int precomp_c = 0; };
}  // namespace kh

using namespace kh;

struct kh_srs {
    int curve = 0;
    int device = -1;          // the device its tables live on: every entry point taking this handle runs there
    size_t n = 0;
    DevBuf g;                 // window tables of g_stride = n + 2 points: g[0..n), then the slots of H and U
    size_t g_stride = 0;      // (the two extra bases of the opening rounds, written by kh_ipa_begin)
    int g_precomp_c = 0;
    DevBuf g_wide; int g_wide_c = 0;   // second table set with wide windows (MSM_WIDE_C) for bases of >= msm_wide_min_n() points: big single MSMs
    bool ipa_live = false;    // the U slot belongs to one opening at a time
    std::thread::id ipa_owner;   // ... begun by this thread (a second opening from ANOTHER thread waits for it: SRS::open is re-entrant on &self)
    // workspace of the opening rounds, kept across openings (hipMalloc / hipFree cost ~0.1 ms each: 1 ms per proof)
    DevBuf ipa_a[2], ipa_b[2], ipa_coef[2], ipa_sc, ipa_partial, ipa_sg;
    hipEvent_t ipa_ev = nullptr;
    // the late rounds' materialised folded basis (csrc/rebase.hip): its window tables, the materialisation's workspaces, a low-priority side stream, the
    // events that order it against the rounds, a pinned "an output was the identity" word
    DevBuf ipa_rb_tab, ipa_rb_B, ipa_rb_part, ipa_rb_lists, ipa_rb_scratch;
    hipStream_t ipa_rb_stream = nullptr;
    hipEvent_t ipa_rb_go = nullptr, ipa_rb_snap = nullptr, ipa_rb_done = nullptr;
    uint32_t* ipa_rb_fail = nullptr;
    uint64_t h[8];
    // fixed-base table of the blinding base: h_table[i * 255 + (j - 1)] = j * 2^(8 i) * h (XYZZ), built on first use:
    // SRS::mask_custom is one scalar multiplication by h per chunk (ipa.rs:605-622) -- 32 additions instead of 255
    // doublings + ~128 additions (a proof masks 23 commitments: 3.5 ms of host time otherwise)
    std::vector<khost::xyzz> h_table;
    std::vector<uint64_t> h_multiples;     // 2^(c w) * h for the W windows (affine, 8 words each): slots of the opening's MSMs
    // second table set for the opening ROUNDS (KH_IPA_C, window width c2 < 16): a round's two MSMs are latency-bound in the bucket
    // reduction (2^15 buckets for 2^20 entries), so narrower windows -- more accumulation work, 8-16x fewer buckets -- shorten the round
    DevBuf g2; int g2_c = 0;
    std::vector<uint64_t> h_multiples2;
    std::mutex h_mu;
    // handle-level locks (callers may be on different contexts, kh_private_context_begin): the basis map, and the one opening a handle runs at a time
    std::mutex map_mu;
    std::mutex ipa_mu; std::condition_variable ipa_cv;
    std::map<unsigned, std::vector<std::unique_ptr<LagrangeChunk>>> lagrange;
    ~kh_srs() {                                                     // the DevBufs free themselves
        if (ipa_ev) (void)hipEventDestroy(ipa_ev);
        if (ipa_rb_go) (void)hipEventDestroy(ipa_rb_go);
        if (ipa_rb_snap) (void)hipEventDestroy(ipa_rb_snap);
        if (ipa_rb_done) (void)hipEventDestroy(ipa_rb_done);
        if (ipa_rb_stream) { (void)hipStreamSynchronize(ipa_rb_stream); (void)hipStreamDestroy(ipa_rb_stream); }
        if (ipa_rb_fail) (void)hipHostFree(ipa_rb_fail);
    }
};
#define KH_ON_DEVICE_OF(srs) kh::DeviceScope dev_scope_((srs) ? (srs)->device : -1)

struct EndoPair { uint64_t q[4], r[4]; };
static const EndoPair& cached_endos(int curve) {
    static EndoPair E[2]; static std::once_flag once[2];
    std::call_once(once[curve & 1], [curve] { curve_endos(curve & 1, E[curve & 1].q, E[curve & 1].r); });
    return E[curve & 1];
}

static int resolve_basis(kh_srs_t* srs, int basis, unsigned chunk, MsmBasis& out) {
    KH_REQUIRE(srs != nullptr, "null SRS handle");
    if (basis == KH_BASIS_G) {
        KH_REQUIRE(chunk == 0, "chunk must be 0 for the monomial basis");
        out.pts = srs->g.p; out.inf = nullptr; out.n = srs->n; out.stride = srs->g_stride; out.precomp_c = srs->g_precomp_c;
        out.wide_pts = srs->g_wide_c ? srs->g_wide.p : nullptr; out.wide_c = srs->g_wide_c;
        return KH_OK;
    }
    std::lock_guard<std::mutex> ml(srs->map_mu);
    auto it = srs->lagrange.find((unsigned)basis);
    if (it == srs->lagrange.end() || chunk >= it->second.size() || !it->second[chunk]) {
        set_error("Lagrange basis for domain 2^%d chunk %u is not registered on this SRS", basis, chunk);
        return KH_E_NOTFOUND;
    }
    LagrangeChunk& L = *it->second[chunk];
    out.pts = L.pts.p; out.inf = L.has_inf ? L.inf.as<uint8_t>() : nullptr; out.n = L.n; out.precomp_c = L.precomp_c;
    return KH_OK;
}

// one non-blocking copy stream per (host thread, device), created on first use
// (destroyed with the thread: a pool of short-lived worker threads must not leak a stream each)
struct ThreadCopyStreams {
    hipStream_t s[KH_MAX_DEVICES] = {nullptr};
    ~ThreadCopyStreams() {
        for (int d = 0; d < KH_MAX_DEVICES; d++)
            if (s[d]) { int cur = -1; if (hipGetDevice(&cur) == hipSuccess) { (void)hipSetDevice(d); (void)hipStreamDestroy(s[d]); (void)hipSetDevice(cur); } }
    }
};
static hipStream_t thread_copy_stream() {
    static thread_local ThreadCopyStreams tl;
    const int d = kh::ctx().device >= 0 && kh::ctx().device < KH_MAX_DEVICES ? kh::ctx().device : 0;
    if (!tl.s[d] && hipStreamCreateWithFlags(&tl.s[d], hipStreamNonBlocking) != hipSuccess) { kh::set_error("hipStreamCreate for a copy stream failed"); return nullptr; }
    return tl.s[d];
}

// events of the chunked scalar upload (MsmHostScalars), per (host thread, device)
static constexpr int UPLOAD_CHUNKS = 8;
struct ThreadUploadEvents {
    hipEvent_t e[KH_MAX_DEVICES][UPLOAD_CHUNKS] = {{nullptr}};
    ~ThreadUploadEvents() { for (auto& row : e) for (hipEvent_t x : row) if (x) (void)hipEventDestroy(x); }
};
static hipEvent_t* thread_upload_events() {
    static thread_local ThreadUploadEvents tl;
    const int d = kh::ctx().device >= 0 && kh::ctx().device < KH_MAX_DEVICES ? kh::ctx().device : 0;
    for (int i = 0; i < UPLOAD_CHUNKS; i++)
        if (!tl.e[d][i] && hipEventCreateWithFlags(&tl.e[d][i], hipEventDisableTiming) != hipSuccess) { kh::set_error("hipEventCreate for an upload event failed"); return nullptr; }
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
size_t pool_limit() { static const size_t lim = (getenv("KH_POOL_MAX_MB") ? (size_t)atol(getenv("KH_POOL_MAX_MB")) : 2048) << 20; return lim; }
}  // namespace
// transfer buffers of the host-pointer transforms (kh_ntt / kh_lde: host_transform below)
struct XferPair { DevBuf in, out; bool busy = false, owned = false; };
static std::mutex g_xfer_mu;
static std::vector<std::unique_ptr<XferPair>>& xfer_registry(int d) {     // (never destroyed: no hipFree from a static destructor after the runtime has gone)
    static auto* r = new std::vector<std::unique_ptr<XferPair>>[KH_MAX_DEVICES];
    return r[d];
}
struct ThreadXfer {
    XferPair* p[KH_MAX_DEVICES] = {nullptr};
    ~ThreadXfer() { std::lock_guard<std::mutex> lk(g_xfer_mu); for (XferPair* q : p) if (q) { q->owned = false; q->busy = false; } }
};
static XferPair* xfer_acquire(int d) {
    static thread_local ThreadXfer tl;
    std::lock_guard<std::mutex> lk(g_xfer_mu);
    if (!tl.p[d]) {
        for (auto& q : xfer_registry(d)) if (!q->owned) { tl.p[d] = q.get(); break; }
        if (!tl.p[d]) { xfer_registry(d).emplace_back(new XferPair); tl.p[d] = xfer_registry(d).back().get(); }
        tl.p[d]->owned = true;
    }
    tl.p[d]->busy = true;
    return tl.p[d];
}
static void xfer_release(XferPair* q) { std::lock_guard<std::mutex> lk(g_xfer_mu); q->busy = false; }
struct XferGuard { XferPair* q; ~XferGuard() { xfer_release(q); } };
static void xfer_trim(int d) {              // kh_trim: every pair that is not inside a call right now gives its memory back
    if (d < 0 || d >= KH_MAX_DEVICES) return;
    std::lock_guard<std::mutex> lk(g_xfer_mu);
    for (auto& q : xfer_registry(d)) if (!q->busy) { q->in.release(); q->out.release(); }
}
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
int kh_srs_device(const kh_srs_t* srs) { return srs ? srs->device : -1; }
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
                          &S.ws_b29, &S.ws_a1, &S.ws_a2, &S.ws_xlist}) b->release();
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

// the wide-window table set of a big basis (table 0 = a copy of the basis; H / U slots unused).  It is a throughput optimisation on top of the narrow tables
// (+13/16 of their memory: 832 MiB at 2^20 points, 3.3 GiB at 2^22), so a handle whose second set does not fit is still a working handle: `required` = false
// gives the memory back, clears the error and leaves the narrow tables to serve every MSM.
static int build_wide_tables(Context& C, kh_srs* s, bool required) {
    if (s->g_wide_c) return KH_OK;
    if (!s->g_precomp_c || (!required && s->n < msm_wide_min_n())) return KH_OK;
    const int W = (256 + MSM_WIDE_C - 1) / MSM_WIDE_C;
    int rc = s->g_wide.reserve(s->g_stride * 64 * (size_t)W);
    if (!rc) {
        hipError_t e = hipMemcpyAsync(s->g_wide.p, s->g.p, s->g_stride * 64, hipMemcpyDeviceToDevice, C.stream);
        if (e != hipSuccess) { set_error("hipMemcpyAsync failed: %s", hipGetErrorString(e)); rc = KH_E_DEVICE; }
    }
    if (!rc) rc = msm_precompute(C, s->curve, s->g_wide.p, nullptr, s->g_stride, MSM_WIDE_C);
    if (rc) {
        (void)hipStreamSynchronize(C.stream);
        s->g_wide.release(); s->g_wide_c = 0;
        if (required || rc != KH_E_NOMEM) return rc;
        (void)hipGetLastError();              // an allocation that did not fit is not an error of the handle
        set_error("");
        return KH_OK;
    }
    s->g_wide_c = MSM_WIDE_C;
    return KH_OK;
}
int kh_srs_has_wide_tables(const kh_srs_t* srs) { return srs && srs->g_wide_c ? 1 : 0; }
int kh_srs_set_wide_tables(kh_srs_t* srs, int on) {
    KH_ON_DEVICE_OF(srs);
    KH_REQUIRE(srs != nullptr, "null SRS handle");
    int rc = ensure_init(); if (rc) return rc;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    if (on) {
        KH_REQUIRE(srs->g_precomp_c, "kh_srs_set_wide_tables: the handle has no window tables (fewer than %d points)", (int)MSM_PRECOMP_MIN_N);
        if ((rc = build_wide_tables(C, srs, true))) return rc;
        KH_HIP(hipStreamSynchronize(C.stream));
        return KH_OK;
    }
    for (int i = 0; i < MSM_SLOTS; i++) {
        KH_REQUIRE(!C.slot[i].busy, "kh_srs_set_wide_tables: an MSM is in flight (kh_msm_wait first)");
        if (C.slot[i].stream) KH_HIP(hipStreamSynchronize(C.slot[i].stream));
    }
    srs->g_wide_c = 0;
    srs->g_wide.release();
    return KH_OK;
}
int kh_msm_set_wide_min_n(size_t n) { msm_set_wide_min_n(n); return KH_OK; }
int kh_msm_set_sort_staging(unsigned entries, unsigned max_passes) {
    if (max_passes > 8) { set_error("kh_msm_set_sort_staging: at most 8 passes (got %u)", max_passes); return KH_E_INVALID; }
    msm_set_sort_staging(entries, max_passes); return KH_OK;
}
int kh_srs_create(int curve, const uint64_t* g_xy, size_t n, kh_srs_t** out) {
    KH_REQUIRE(out && g_xy && n > 0, "kh_srs_create: null argument or n == 0");
    KH_REQUIRE(curve == KH_CURVE_VESTA || curve == KH_CURVE_PALLAS, "unknown curve id %d", curve);
    int rc = ensure_init(); if (rc) return rc;
    std::unique_ptr<kh_srs> s(new kh_srs);
    s->curve = curve; s->n = n;
    Context& C = ctx();
    s->device = C.device;
    std::lock_guard<std::mutex> lk(C.mu);
    const bool pre = n >= MSM_PRECOMP_MIN_N && !getenv("KH_NO_PRECOMP");
    const int W = (256 + MSM_PRECOMP_C - 1) / MSM_PRECOMP_C;
    s->g_stride = n + 2;
    if ((rc = s->g.reserve(s->g_stride * 64 * (pre ? W : 1)))) return rc;
    KH_HIP(hipMemcpy(s->g.p, g_xy, n * 64, hipMemcpyHostToDevice));
    KH_HIP(hipMemcpy((char*)s->g.p + n * 64, g_xy, 64, hipMemcpyHostToDevice));          // placeholders: valid points
    KH_HIP(hipMemcpy((char*)s->g.p + (n + 1) * 64, g_xy, 64, hipMemcpyHostToDevice));
    if (pre) {
        if ((rc = msm_precompute(C, curve, s->g.p, nullptr, s->g_stride, MSM_PRECOMP_C))) return rc;
        s->g_precomp_c = MSM_PRECOMP_C;
        if ((rc = build_wide_tables(C, s.get(), false))) return rc;
    }
    // tables are per HANDLE, streams per context: another context (kh_private_context_begin on another thread) may use the handle at once, so it is
    // handed out complete (a one-time cost)
    KH_HIP(hipStreamSynchronize(C.stream));
    if ((rc = kh_srs_h(curve, s->h))) return rc;
    *out = s.release();
    return KH_OK;
}
int kh_srs_create_device(int curve, size_t depth, kh_srs_t** out) { return kh_srs_create_device_range(curve, 0, depth, out); }
int kh_srs_create_device_range(int curve, size_t start, size_t depth, kh_srs_t** out) {
    KH_REQUIRE(out && depth > 0, "kh_srs_create_device: null argument or depth == 0");
    KH_REQUIRE(curve == KH_CURVE_VESTA || curve == KH_CURVE_PALLAS, "unknown curve id %d", curve);
    KH_REQUIRE(start + depth <= ((size_t)1 << 32), "SRS index must fit u32 (ipa.rs:758)");
    int rc = ensure_init(); if (rc) return rc;
    std::unique_ptr<kh_srs> s(new kh_srs);
    s->curve = curve; s->n = depth;
    Context& C = ctx();
    s->device = C.device;
    std::lock_guard<std::mutex> lk(C.mu);
    const bool pre = depth >= MSM_PRECOMP_MIN_N && !getenv("KH_NO_PRECOMP");
    const int W = (256 + MSM_PRECOMP_C - 1) / MSM_PRECOMP_C;
    s->g_stride = depth + 2;
    if ((rc = s->g.reserve(s->g_stride * 64 * (pre ? W : 1)))) return rc;
    if ((rc = srs_generate_device(C, curve, start, depth, s->g.p))) return rc;
    KH_HIP(hipMemcpyAsync((char*)s->g.p + depth * 64, s->g.p, 64, hipMemcpyDeviceToDevice, C.stream));
    KH_HIP(hipMemcpyAsync((char*)s->g.p + (depth + 1) * 64, s->g.p, 64, hipMemcpyDeviceToDevice, C.stream));
    if (pre) {
        if ((rc = msm_precompute(C, curve, s->g.p, nullptr, s->g_stride, MSM_PRECOMP_C))) return rc;
        s->g_precomp_c = MSM_PRECOMP_C;
        if ((rc = build_wide_tables(C, s.get(), false))) return rc;
    }
    // tables are per HANDLE, streams per context: another context (kh_private_context_begin on another thread) may use the handle at once, so it is
    // handed out complete (a one-time cost)
    KH_HIP(hipStreamSynchronize(C.stream));
    if ((rc = kh_srs_h(curve, s->h))) return rc;
    *out = s.release();
    return KH_OK;
}
int kh_srs_get_g(kh_srs_t* srs, size_t offset, size_t count, uint64_t* out_xy) {
    KH_ON_DEVICE_OF(srs);
    KH_REQUIRE(srs && (out_xy || count == 0), "kh_srs_get_g: null argument");
    KH_REQUIRE(offset + count <= srs->n, "range [%zu, %zu) beyond the SRS size %zu", offset, offset + count, srs->n);
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    if (count) KH_HIP(hipMemcpy(out_xy, (const char*)srs->g.p + offset * 64, count * 64, hipMemcpyDeviceToHost));
    return KH_OK;
}
void kh_srs_free(kh_srs_t* srs) {
    if (!srs) return;
    KH_ON_DEVICE_OF(srs);
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    for (int i = 0; i < MSM_SLOTS; i++) if (C.slot[i].stream) (void)hipStreamSynchronize(C.slot[i].stream);   // nothing may still read its tables
    delete srs;                       // the handle's buffers (tables, Lagrange chunks, opening workspace) free themselves
}
size_t kh_srs_size(const kh_srs_t* srs) { return srs ? srs->n : 0; }
int kh_srs_curve(const kh_srs_t* srs) { return srs ? srs->curve : -1; }

int kh_srs_set_lagrange(kh_srs_t* srs, unsigned log2_domain, unsigned chunk, const uint64_t* xy, const uint8_t* inf, size_t n) {
    KH_ON_DEVICE_OF(srs);
    KH_REQUIRE(srs && xy, "kh_srs_set_lagrange: null argument");
    KH_REQUIRE(log2_domain <= 32 && n == ((size_t)1 << log2_domain), "basis must have 2^log2_domain = %zu points, got %zu", (size_t)1 << log2_domain, n);
    int rc = ensure_init(); if (rc) return rc;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    std::lock_guard<std::mutex> ml(srs->map_mu);
    auto& vec = srs->lagrange[log2_domain];
    if (vec.size() <= chunk) vec.resize(chunk + 1);
    std::unique_ptr<LagrangeChunk> L(new LagrangeChunk);
    L->n = n;
    const bool pre = n >= MSM_PRECOMP_MIN_N && !getenv("KH_NO_PRECOMP");
    const int W = (256 + MSM_PRECOMP_C - 1) / MSM_PRECOMP_C;
    if ((rc = L->pts.reserve(n * 64 * (pre ? W : 1)))) return rc;
    KH_HIP(hipMemcpy(L->pts.p, xy, n * 64, hipMemcpyHostToDevice));
    if (inf) {
        bool any = false;
        for (size_t i = 0; i < n; i++) any |= inf[i] != 0;
        if (any) {
            if ((rc = L->inf.reserve(n))) return rc;
            KH_HIP(hipMemcpy(L->inf.p, inf, n, hipMemcpyHostToDevice));
            L->has_inf = true;
        }
    }
    if (pre) {
        if ((rc = msm_precompute(C, srs->curve, L->pts.p, L->has_inf ? L->inf.as<uint8_t>() : nullptr, n, MSM_PRECOMP_C))) return rc;
        L->precomp_c = MSM_PRECOMP_C;
    }
    KH_HIP(hipStreamSynchronize(C.stream));              // published complete (callers of other contexts resolve the basis without this stream)
    vec[chunk] = std::move(L);
    return KH_OK;
}
int kh_srs_lagrange_chunks(const kh_srs_t* srs, unsigned log2_domain) {
    if (!srs) return 0;
    KH_ON_DEVICE_OF(srs);
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    std::lock_guard<std::mutex> ml(const_cast<kh_srs_t*>(srs)->map_mu);      // kh_srs_set_lagrange / kh_srs_compute_lagrange mutate the map under it
    auto it = srs->lagrange.find(log2_domain);
    return it == srs->lagrange.end() ? 0 : (int)it->second.size();
}
int kh_srs_compute_lagrange(kh_srs_t* srs, unsigned log2_domain) {
    KH_ON_DEVICE_OF(srs);
    KH_REQUIRE(srs, "null SRS handle");
    KH_REQUIRE(log2_domain <= 28, "log2_domain = %u too large", log2_domain);
    int rc = ensure_init(); if (rc) return rc;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    std::lock_guard<std::mutex> ml(srs->map_mu);
    const size_t n = (size_t)1 << log2_domain;
    const unsigned num_chunks = (unsigned)((n + srs->n - 1) / srs->n);            // ipa.rs:1143-1144
    auto& vec = srs->lagrange[log2_domain];
    // idempotent: the reference's get_lagrange_basis is a cache lookup (ipa.rs:780-795) that 15 rayon workers hit at once on the first
    // proof; a second computation would free the tables behind an MSM that has already resolved them
    if (vec.size() == num_chunks) {
        bool all = true;
        for (auto& c : vec) if (!c) all = false;
        if (all) return KH_OK;
    }
    vec.clear(); vec.resize(num_chunks);
    const bool pre = n >= MSM_PRECOMP_MIN_N && !getenv("KH_NO_PRECOMP");
    const int W = (256 + MSM_PRECOMP_C - 1) / MSM_PRECOMP_C;
    for (unsigned c = 0; c < num_chunks; c++) {
        std::unique_ptr<LagrangeChunk> L(new LagrangeChunk);
        L->n = n;
        if ((rc = L->pts.reserve(n * 64 * (pre ? W : 1)))) return rc;
        if ((rc = L->inf.reserve(n))) return rc;
        if ((rc = lagrange_run(C, srs->curve, srs->g.p, srs->n, log2_domain, c, L->pts.p, L->inf.as<uint8_t>()))) return rc;
        std::vector<uint8_t> hinf(n);
        KH_HIP(hipMemcpy(hinf.data(), L->inf.p, n, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; i++) if (hinf[i]) { L->has_inf = true; break; }
        if (pre) {
            if ((rc = msm_precompute(C, srs->curve, L->pts.p, L->has_inf ? L->inf.as<uint8_t>() : nullptr, n, MSM_PRECOMP_C))) return rc;
            L->precomp_c = MSM_PRECOMP_C;
        }
        KH_HIP(hipStreamSynchronize(C.stream));          // published complete (callers of other contexts resolve the basis without this stream)
        vec[c] = std::move(L);
    }
    return KH_OK;
}
int kh_srs_get_lagrange(kh_srs_t* srs, unsigned log2_domain, unsigned chunk, uint64_t* out_xy, uint8_t* out_inf) {
    KH_ON_DEVICE_OF(srs);
    KH_REQUIRE(srs && out_xy, "kh_srs_get_lagrange: null argument");
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    MsmBasis b; int rc = resolve_basis(srs, (int)log2_domain, chunk, b); if (rc) return rc;
    KH_HIP(hipMemcpy(out_xy, b.pts, b.n * 64, hipMemcpyDeviceToHost));
    if (out_inf) {
        if (b.inf) KH_HIP(hipMemcpy(out_inf, b.inf, b.n, hipMemcpyDeviceToHost));
        else memset(out_inf, 0, b.n);
    }
    return KH_OK;
}

// ---------------------------------------------------------------------------------- MSM
static int free_slot(Context& C) {
    for (int i = 0; i < MSM_SLOTS; i++) if (!C.slot[i].busy) return i;
    return -1;
}
// a caller may wait for a slot that another thread is blocked on (it will be released) or that holds ANOTHER thread's un-waited
// kh_msm_submit ticket (more provers than slots: that thread is on its way to kh_msm_wait) -- the latter for two seconds at most, in case
// the tickets' owners are themselves waiting here; with only the caller's own un-waited tickets busy the answer is -1 at once
// side_first: take a slot other than the main stream's when one is free (the opening rounds: their MSM then runs beside, not behind,
// the work other host threads queue on the main stream)
// Back-pressure, not a time-out: the caller blocks until a slot is released (an oversubscribed rayon pool must see a slow call, not
// a spurious error).  The one case that can never resolve is refused at once: every busy slot holds an un-waited ticket whose owner
// is itself blocked in here (or is the caller) -- nobody is left to call kh_msm_wait.
static int acquire_slot(std::unique_lock<std::mutex>* lk, Context& C, bool side_first = false) {
    const auto me = std::this_thread::get_id();
    auto t_start = std::chrono::steady_clock::now();
    uint64_t seen = ~(uint64_t)0;                          // what the slots looked like at the last look: the deadline counts time WITHOUT progress
    for (;;) {
        uint64_t sig = C.next_ticket;
        for (int i = 0; i < MSM_SLOTS; i++) sig = sig * 1315423911ull + (C.slot[i].busy ? C.slot[i].ticket + 1 : 0);
        if (sig != seen) { seen = sig; t_start = std::chrono::steady_clock::now(); }
        int si = -1;
        if (side_first) for (int i = MSM_SLOTS - 1; i >= 1; i--) if (!C.slot[i].busy) { si = i; break; }
        if (si < 0) si = free_slot(C);
        if (si >= 0 || !lk) return si;
        if (C.sync_inflight == 0) {
            bool progress = false;                          // some ticket owner is still free to reach kh_msm_wait
            for (int i = 0; i < MSM_SLOTS; i++)
                if (C.slot[i].busy && C.slot[i].owner != me && !C.blocked_owners.count(C.slot[i].owner)) progress = true;
            if (!progress) return -1;
        }
        // A slot whose owner leaked its ticket (an exception between kh_msm_submit and kh_msm_wait, a thread that exited) never frees: after a
        // long deadline -- far beyond any MSM, KH_SLOT_WAIT_S, default 30 s -- give up with an error instead of hanging every later caller.
        static const long slot_wait_s = getenv("KH_SLOT_WAIT_S") ? atol(getenv("KH_SLOT_WAIT_S")) : 30;
        if (std::chrono::steady_clock::now() - t_start > std::chrono::seconds(slot_wait_s)) return -2;
        C.blocked_owners.insert(me);
        C.cv.wait_for(*lk, std::chrono::milliseconds(50));  // (the time-out re-evaluates the deadlock test and the deadline)
        C.blocked_owners.erase(C.blocked_owners.find(me));
    }
}
static const char* slot_error(int si) {
    return si == -2 ? "no MSM pipeline slot came free and none changed hands for KH_SLOT_WAIT_S (default 30 s): a kh_msm_submit ticket was leaked (its owner never called kh_msm_wait)"
                    : "every MSM pipeline slot holds an un-waited kh_msm_submit ticket of this thread (or of threads blocked behind it): kh_msm_wait first";
}
// enqueue on a free slot; returns the slot index through *slot_out
static int msm_submit_locked(Context& C, kh_srs_t* srs, int basis, unsigned chunk, size_t offset, const uint64_t* scalars,
                             bool scalars_on_device, size_t n, size_t k, int mont, int* slot_out, std::unique_lock<std::mutex>* lk = nullptr,
                             bool host_async = false) {
    MsmBasis b; int rc = resolve_basis(srs, basis, chunk, b); if (rc) return rc;
    KH_REQUIRE(offset <= b.n, "offset %zu beyond basis length %zu", offset, b.n);
    size_t use = n < b.n - offset ? n : b.n - offset;      // msm_bigint semantics: min(len) pairs
    int si = acquire_slot(lk, C);
    KH_REQUIRE(si >= 0, "%s", slot_error(si));
    if (lk && (rc = resolve_basis(srs, basis, chunk, b))) return rc;     // acquire_slot may have dropped the lock: the basis map can have changed
    MsmSlot& S = C.slot[si];
    const uint64_t* sdev = scalars;
    // a big single MSM from host scalars: upload and digit pass in chunks on the calling thread's copy stream (MsmHostScalars) -- the other slots' jobs keep
    // the GPU busy meanwhile (kh_msm_submit_host: two in flight hide the whole upload), and a lone MSM hides its digit pass
    // (KH_HOST_CHUNK_MIN=n switches it on for MSMs of >= n scalars; off by default: at 2^20 the chunked upload measured level with the single copy -- what
    // pipelines the PCIe transfer under the neighbouring job's accumulation is kh_msm_submit_host itself, not the chunking: profiles/r06_host_msm*.txt)
    static const size_t chunked_min = getenv("KH_HOST_CHUNK_MIN") ? (size_t)atol(getenv("KH_HOST_CHUNK_MIN")) : 0;     // scalars; 0 = never
    MsmHostScalars hs{}; const MsmHostScalars* hsp = nullptr;
    if (!scalars_on_device && k == 1 && chunked_min && use >= chunked_min) {
        if ((rc = S.ws_scalars.reserve(use * 32))) return rc;
        hs.host = scalars; hs.cs = thread_copy_stream(); hs.ev = thread_upload_events();
        if (!hs.cs || !hs.ev) return KH_E_DEVICE;
        hs.nev = (int)std::min<size_t>(UPLOAD_CHUNKS, std::max<size_t>(1, use >> 16));       // >= 2 MB per chunk
        hsp = &hs; sdev = S.ws_scalars.as<uint64_t>();
    } else
    if (!scalars_on_device && use > 0 && k > 0) {
        if ((rc = S.ws_scalars.reserve(k * use * 32))) return rc;
        // (host_async: kh_msm_submit_host returns while the job runs -- its copies go on the calling thread's copy stream, which that call waits for)
        hipStream_t up = S.stream; hipEvent_t* uev = nullptr;
        if (host_async) { up = thread_copy_stream(); uev = thread_upload_events(); if (!up || !uev) return KH_E_DEVICE; }
        if (use == n) KH_HIP(hipMemcpyAsync(S.ws_scalars.p, scalars, k * n * 32, hipMemcpyHostToDevice, up));
        else for (size_t j = 0; j < k; j++)
            KH_HIP(hipMemcpyAsync((char*)S.ws_scalars.p + j * use * 32, scalars + j * n * 4, use * 32, hipMemcpyHostToDevice, up));
        if (host_async) { KH_HIP(hipEventRecord(uev[0], up)); KH_HIP(hipStreamWaitEvent(S.stream, uev[0], 0)); }
        sdev = S.ws_scalars.as<uint64_t>();
    } else if (scalars_on_device) {
        KH_REQUIRE(use == n || k == 1, "device-resident batched scalars must not exceed the basis window");
        // the scalars may be the output of an asynchronous kh_ntt_dev / kh_lde_dev still running on the main stream: wait for
        // the event recorded right behind the last such producer (NOT for whatever else slot 0's stream has queued since)
        if (C.main_dirty && S.stream != C.stream) KH_HIP(hipStreamWaitEvent(S.stream, C.order_ev, 0));
    }
    rc = msm_enqueue(C, S, srs->curve, b, offset, sdev, use, k, mont, 0, hsp);
    if (rc) {
        if (hsp) (void)hipStreamSynchronize(hs.cs);      // a caller that sees an error may free its scalars at once: no copy may still be reading them
        return rc;
    }
    *slot_out = si;
    return KH_OK;
}
// The GPU wait happens WITHOUT the library lock: the slot stays busy (nobody else can take it), other threads can
// enqueue on the remaining slots meanwhile (15 rayon workers call into the reference's SRS at once, prover.rs:329-351;
// two provers can run their opening rounds side by side).  The short host part runs under the lock again.
static thread_local double tl_last_wait_us = 0;           // spin / block part of the last wait_then_finish on this thread
static int wait_then_finish(std::unique_lock<std::mutex>& lk, Context& C, MsmSlot& S, uint64_t* out_xy, uint8_t* out_inf) {
    hipEvent_t ev = S.done;
    // completion by flag (MsmSlot::done_flag): what the job's last kernel will store, read while the context is still locked
    const bool by_flag = S.job.done_by_flag && S.done_flag;
    const uint32_t expect = S.done_expect;
    C.sync_inflight++;
    lk.unlock();
    const auto tw0 = std::chrono::steady_clock::now();
    // a synchronous caller is latency-bound (an opening round is ~0.4 ms of GPU time, then ~40 us of transcript on this thread):
    // poll for up to a millisecond before blocking -- the blocking wait's wake-up alone costs 10-20 us
    static const long spin_us = getenv("KH_SPIN_US") ? atol(getenv("KH_SPIN_US")) : 1000;
    hipError_t e = hipErrorNotReady;
    bool flag_seen = false;
    if (spin_us > 0) {
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned it = 0;; it++) {
            if (by_flag) {                                 // the last kernel's own store (MsmSlot::done_flag); the event is looked at now and then, for errors
                if (__atomic_load_n((const uint32_t*)S.done_flag, __ATOMIC_ACQUIRE) == expect) { flag_seen = true; e = hipSuccess; break; }
                if ((it & 1023u) != 1023u) { __builtin_ia32_pause(); continue; }
            }
            e = hipEventQuery(ev);
            if (e != hipErrorNotReady) break;
            if (std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() > spin_us) break;
            __builtin_ia32_pause();
        }
    }
    if (e == hipErrorNotReady) { (void)hipGetLastError(); e = hipEventSynchronize(ev); }
    tl_last_wait_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tw0).count();
    lk.lock();
    C.sync_inflight--;
    // the job ended by its event without the completion word ever showing its launch count: the host's count had run ahead of the device's (an enqueue
    // that failed after counting, a job whose last kernel was not the flagged one) -- take the device's, or every later wait would go by the event
    if (by_flag && !flag_seen && e == hipSuccess) S.done_expect = __atomic_load_n((const uint32_t*)S.done_flag, __ATOMIC_ACQUIRE);
    int rc;
    if (e != hipSuccess) { set_error("hipEventSynchronize: %s", hipGetErrorString(e)); S.busy = false; rc = KH_E_DEVICE; }
    else rc = msm_finish(C, S, out_xy, out_inf, flag_seen);
    C.cv.notify_all();
    return rc;
}
// Coalescing of concurrent synchronous callers.  The reference commits its 15 witness columns from 15 rayon workers at
// once (prover.rs:329-351), each calling SRS::commit_evaluations_non_hiding -> one MSM over the SAME basis.  Fifteen
// separate launches queue on four pipeline slots and pay the latency-bound tail kernels fifteen times; one batched launch
// of k = 15 shares them (0.9 ms against ~0.46 ms EACH).  So: host-buffer, single-MSM calls with the same (handle, basis,
// chunk, offset, length, scalar form) that arrive while a group is still collecting are merged into ONE msm_enqueue(k = #callers);
// every caller gets its own result.  A group collects only when calls are arriving in a burst (another call on this
// context within the last 200 us): a lone sequential caller never waits.
struct CoalesceMember { const uint64_t* scalars; uint64_t* out_xy; uint8_t* out_inf; };
struct CoalesceGroup {
    kh_srs_t* srs; int basis; unsigned chunk; size_t offset, n; int mont;
    std::vector<CoalesceMember> members;
    bool closed = false, done = false;
    int rc = KH_OK;
    std::string err;
    std::condition_variable cv;
};
static constexpr size_t COALESCE_MAX = 32;
static std::vector<std::shared_ptr<CoalesceGroup>>& coalesce_groups(Context& C) {      // per device context, guarded by C.mu
    static std::map<Context*, std::vector<std::shared_ptr<CoalesceGroup>>> G; static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    return G[&C];
}

static int msm_common(kh_srs_t* srs, int basis, unsigned chunk, size_t offset, const uint64_t* scalars, bool scalars_on_device,
                      size_t n, size_t k, int mont, uint64_t* out_xy, uint8_t* out_inf) {
    KH_ON_DEVICE_OF(srs);
    KH_REQUIRE(out_xy && out_inf, "null output pointer");
    KH_REQUIRE(scalars || n == 0 || k == 0, "null scalars");
    int rc = ensure_init(); if (rc) return rc;
    Context& C = ctx();
    std::unique_lock<std::mutex> lk(C.mu);
    static const bool coalesce_on = !(getenv("KH_NO_COALESCE") && atoi(getenv("KH_NO_COALESCE")) != 0);
    const auto now = std::chrono::steady_clock::now();
    const bool burst = C.last_sync_msm_arrival.time_since_epoch().count() != 0 &&
                       std::chrono::duration_cast<std::chrono::microseconds>(now - C.last_sync_msm_arrival).count() < 200;
    C.last_sync_msm_arrival = now;
    // KH_HOST_SPLIT_MIN=n (experiment, off by default): a lone host-scalar MSM of >= n scalars as TWO half-range MSMs on two slots, each with its own upload.
    // Measured (round 6, profiles/r06_host_msm*.txt): no gain -- 1.91-1.98 ms either way at 2^20.  The host thread stages the two uploads one after the
    // other (~0.45 ms each incl. the pinning of the pageable pages), so the second half's kernels cannot start before ~1.2 ms and then need 0.75 ms: the
    // bound is (all uploads) + (the last piece's whole pipeline), and an uneven cut would reach ~1.75 ms at best.
    static const size_t split_min = getenv("KH_HOST_SPLIT_MIN") ? (size_t)atol(getenv("KH_HOST_SPLIT_MIN")) : 0;
    if (!scalars_on_device && k == 1 && srs != nullptr && !burst && split_min && n >= split_min) {
        MsmBasis b;
        if (resolve_basis(srs, basis, chunk, b) == KH_OK && offset <= b.n && b.precomp_c) {
            const size_t use = n < b.n - offset ? n : b.n - offset, h = use / 2;
            if (h >= MSM_PRECOMP_MIN_N) {
                int s0 = -1, s1 = -1;
                if ((rc = msm_submit_locked(C, srs, basis, chunk, offset, scalars, false, h, 1, mont, &s0, &lk))) return rc;
                uint64_t xy[16]; uint8_t inf[2] = {1, 1};
                rc = msm_submit_locked(C, srs, basis, chunk, offset + h, scalars + 4 * h, false, use - h, 1, mont, &s1, &lk);
                const int rc0 = wait_then_finish(lk, C, C.slot[s0], xy, inf);          // (whatever the second submit said: the first job is in flight)
                if (rc) return rc;
                if ((rc = wait_then_finish(lk, C, C.slot[s1], xy + 8, inf + 1))) return rc;
                if (rc0) return rc0;
                lk.unlock();
                return kh_points_sum(srs->curve, xy, inf, 2, out_xy, out_inf);
            }
        }
    }
    bool eligible = coalesce_on && !scalars_on_device && k == 1 && n >= MSM_PRECOMP_MIN_N && srs != nullptr;
    if (eligible) {                                       // whole-window MSMs only (the ragged tail of a chunked polynomial goes alone)
        MsmBasis b; if (resolve_basis(srs, basis, chunk, b) != KH_OK || offset > b.n || n > b.n - offset) eligible = false;
    }
    if (!eligible) {
        int si = -1;
        if ((rc = msm_submit_locked(C, srs, basis, chunk, offset, scalars, scalars_on_device, n, k, mont, &si, &lk))) return rc;
        return wait_then_finish(lk, C, C.slot[si], out_xy, out_inf);
    }
    auto& groups = coalesce_groups(C);
    for (auto& g : groups)
        if (!g->closed && g->members.size() < COALESCE_MAX && g->srs == srs && g->basis == basis && g->chunk == chunk && g->offset == offset && g->n == n && g->mont == mont) {
            std::shared_ptr<CoalesceGroup> grp = g;       // follower: hand the pointers to the leader, sleep until it has the results
            grp->members.push_back({scalars, out_xy, out_inf});
            grp->cv.notify_all();
            grp->cv.wait(lk, [&] { return grp->done; });
            if (grp->rc) set_error("%s", grp->err.c_str());
            return grp->rc;
        }
    std::shared_ptr<CoalesceGroup> grp(new CoalesceGroup);
    grp->srs = srs; grp->basis = basis; grp->chunk = chunk; grp->offset = offset; grp->n = n; grp->mont = mont;
    grp->members.push_back({scalars, out_xy, out_inf});
    groups.push_back(grp);
    if (burst) {                                          // leader: collect while callers keep arriving (40 us of silence closes the group)
        const auto deadline = now + std::chrono::microseconds(400);
        size_t seen = 1;
        for (;;) {
            grp->cv.wait_for(lk, std::chrono::microseconds(40));
            if (grp->members.size() == seen || grp->members.size() >= COALESCE_MAX || std::chrono::steady_clock::now() >= deadline) break;
            seen = grp->members.size();
        }
    }
    grp->closed = true;
    groups.erase(std::find(groups.begin(), groups.end(), grp));
    const size_t kk = grp->members.size();
    std::vector<uint64_t> res(8 * kk); std::vector<uint8_t> rinf(kk);
    auto run = [&]() -> int {
        MsmBasis b; int r;
        int si = acquire_slot(&lk, C);
        KH_REQUIRE(si >= 0, "%s", slot_error(si));
        if ((r = resolve_basis(srs, basis, chunk, b))) return r;         // after the wait: the lock was dropped meanwhile
        MsmSlot& S = C.slot[si];
        if ((r = S.ws_scalars.reserve(kk * n * 32))) return r;
        for (size_t j = 0; j < kk; j++)
            KH_HIP(hipMemcpyAsync((char*)S.ws_scalars.p + j * n * 32, grp->members[j].scalars, n * 32, hipMemcpyHostToDevice, S.stream));
        if ((r = msm_enqueue(C, S, srs->curve, b, offset, S.ws_scalars.as<uint64_t>(), n, kk, mont))) return r;
        return wait_then_finish(lk, C, S, res.data(), rinf.data());
    };
    rc = run();
    if (rc == KH_OK)
        for (size_t j = 0; j < kk; j++) { memcpy(grp->members[j].out_xy, &res[8 * j], 64); *grp->members[j].out_inf = rinf[j]; }
    else grp->err = kh_last_error();
    grp->rc = rc; grp->done = true;
    grp->cv.notify_all();
    return rc;
}

int kh_msm_submit(kh_srs_t* srs, int basis, unsigned chunk, size_t offset, const uint64_t* scalars_dev, size_t n, size_t k,
                  int scalars_are_montgomery, uint64_t* ticket) {
    KH_ON_DEVICE_OF(srs);
    KH_REQUIRE(ticket, "null ticket pointer");
    KH_REQUIRE(scalars_dev || n == 0 || k == 0, "null scalars");
    int rc = ensure_init(); if (rc) return rc;
    Context& C = ctx();
    std::unique_lock<std::mutex> lk(C.mu);
    int si = -1;
    if ((rc = msm_submit_locked(C, srs, basis, chunk, offset, scalars_dev, true, n, k, scalars_are_montgomery, &si, &lk))) return rc;
    *ticket = C.slot[si].ticket | ((uint64_t)C.device << 56);      // the device rides in the top byte: kh_msm_wait may run on any thread
    return KH_OK;
}
int kh_msm_submit_host(kh_srs_t* srs, int basis, unsigned chunk, size_t offset, const uint64_t* scalars, size_t n, size_t k,
                       int scalars_are_montgomery, uint64_t* ticket) {
    KH_ON_DEVICE_OF(srs);
    KH_REQUIRE(ticket, "null ticket pointer");
    KH_REQUIRE(scalars || n == 0 || k == 0, "null scalars");
    int rc = ensure_init(); if (rc) return rc;
    Context& C = ctx();
    std::unique_lock<std::mutex> lk(C.mu);
    int si = -1;
    rc = msm_submit_locked(C, srs, basis, chunk, offset, scalars, false, n, k, scalars_are_montgomery, &si, &lk, true);
    if (rc) { lk.unlock(); hipStream_t cs0 = thread_copy_stream(); if (cs0) (void)hipStreamSynchronize(cs0); return rc; }
    *ticket = C.slot[si].ticket | ((uint64_t)C.device << 56);
    lk.unlock();
    // The scalars belong to the caller again when this returns: hipMemcpyAsync from pageable memory returns once the runtime has taken the data, but a
    // caller may hand over pinned (hipHostMalloc / hipHostRegister) memory, whose copies are truly asynchronous -- so wait for the calling thread's copy
    // stream, which carried every upload of this call (the kernels queued behind them on the slot's stream keep running).
    hipStream_t cs = thread_copy_stream();
    if (cs) KH_HIP(hipStreamSynchronize(cs));
    return KH_OK;
}
int kh_msm_wait(uint64_t ticket, uint64_t* out_xy, uint8_t* out_is_inf) {
    KH_REQUIRE(out_xy && out_is_inf, "null output pointer");
    kh::DeviceScope dev_scope_((int)(ticket >> 56));
    int rc = ensure_init(); if (rc) return rc;
    Context& C = ctx();
    std::unique_lock<std::mutex> lk(C.mu);
    const uint64_t seq = ticket & (((uint64_t)1 << 56) - 1);
    for (int i = 0; i < MSM_SLOTS; i++)
        if (C.slot[i].busy && C.slot[i].ticket == seq) return wait_then_finish(lk, C, C.slot[i], out_xy, out_is_inf);
    set_error("unknown or already waited MSM ticket %llu", (unsigned long long)ticket);
    return KH_E_INVALID;
}

// ---- point-range sharding over several handles / devices (BASELINE config 4 inside the library)
int kh_msm_sharded_dev(kh_srs_t* const* shards, size_t R, const uint64_t* const* scalars_dev, const size_t* counts, int scalars_are_montgomery,
                       uint64_t out_xy[8], uint8_t* out_is_inf) {
    KH_REQUIRE(shards && scalars_dev && counts && out_xy && out_is_inf && R > 0, "kh_msm_sharded_dev: null argument");
    KH_REQUIRE(R <= 64, "at most 64 shards (got %zu)", R);
    for (size_t r = 0; r < R; r++) {
        KH_REQUIRE(shards[r], "shard %zu is null", r);
        KH_REQUIRE(shards[r]->curve == shards[0]->curve, "shard %zu is on another curve", r);
        KH_REQUIRE(counts[r] <= shards[r]->n, "shard %zu: %zu scalars for %zu points", r, counts[r], shards[r]->n);
    }
    std::vector<uint64_t> tickets(R, 0), part(8 * R, 0);
    std::vector<uint8_t> pinf(R, 1);
    std::vector<size_t> pending;                                // submitted, not yet waited for (oldest first)
    int rc = KH_OK;
    auto wait_oldest = [&]() {
        const size_t r = pending.front(); pending.erase(pending.begin());
        int w = kh_msm_wait(tickets[r], &part[8 * r], &pinf[r]);
        if (rc == KH_OK) rc = w;
    };
    for (size_t r = 0; r < R && rc == KH_OK; r++) {            // as much as the pipeline slots allow is in flight before the first wait
        if (counts[r] == 0) continue;
        for (;;) {
            int s_ = kh_msm_submit(shards[r], KH_BASIS_G, 0, 0, scalars_dev[r], counts[r], 1, scalars_are_montgomery, &tickets[r]);
            if (s_ == KH_OK) { pending.push_back(r); break; }
            if (s_ == KH_E_INVALID && !pending.empty()) { wait_oldest(); if (rc) break; continue; }   // several shards on one device: its four slots are ours
            rc = s_; break;
        }
    }
    while (!pending.empty()) wait_oldest();                     // (also after an error: no ticket may be left un-waited)
    if (rc) return rc;
    return kh_points_sum(shards[0]->curve, part.data(), pinf.data(), R, out_xy, out_is_inf);
}
int kh_msm_sharded(kh_srs_t* const* shards, size_t R, const uint64_t* scalars, size_t n, int scalars_are_montgomery, uint64_t out_xy[8], uint8_t* out_is_inf) {
    KH_REQUIRE(shards && out_xy && out_is_inf && R > 0 && (scalars || n == 0), "kh_msm_sharded: null argument");
    KH_REQUIRE(R <= 64, "at most 64 shards (got %zu)", R);
    size_t total = 0;
    for (size_t r = 0; r < R; r++) { KH_REQUIRE(shards[r], "shard %zu is null", r); total += shards[r]->n; }
    KH_REQUIRE(n <= total, "%zu scalars for %zu points", n, total);
    // the slices go up from R host threads at once, each bound to its shard's device (kh_msm: upload + MSM + affine result)
    std::vector<uint64_t> part(8 * R, 0);
    std::vector<uint8_t> pinf(R, 1);
    std::vector<int> rcs(R, KH_OK);
    std::vector<std::string> errs(R);
    std::vector<std::thread> th;
    size_t off = 0;
    for (size_t r = 0; r < R; r++) {
        const size_t cnt = off >= n ? 0 : std::min(shards[r]->n, n - off);
        if (cnt) th.emplace_back([&, r, off, cnt] {
            rcs[r] = kh_msm(shards[r], KH_BASIS_G, 0, 0, scalars + 4 * off, cnt, scalars_are_montgomery, &part[8 * r], &pinf[r]);
            if (rcs[r]) errs[r] = kh_last_error();               // (the message is thread-local)
        });
        off += shards[r]->n;
    }
    for (auto& t : th) t.join();
    for (size_t r = 0; r < R; r++) if (rcs[r]) { set_error("shard %zu: %s", r, errs[r].c_str()); return rcs[r]; }
    return kh_points_sum(shards[0]->curve, part.data(), pinf.data(), R, out_xy, out_is_inf);
}

int kh_msm(kh_srs_t* srs, int basis, unsigned chunk, size_t offset, const uint64_t* scalars, size_t n,
           int scalars_are_montgomery, uint64_t out_xy[8], uint8_t* out_is_inf) {
    return msm_common(srs, basis, chunk, offset, scalars, false, n, 1, scalars_are_montgomery, out_xy, out_is_inf);
}
int kh_msm_batch(kh_srs_t* srs, int basis, unsigned chunk, size_t offset, const uint64_t* scalars, size_t n, size_t k,
                 int scalars_are_montgomery, uint64_t* out_xy, uint8_t* out_is_inf) {
    return msm_common(srs, basis, chunk, offset, scalars, false, n, k, scalars_are_montgomery, out_xy, out_is_inf);
}
int kh_msm_batch_dev(kh_srs_t* srs, int basis, unsigned chunk, size_t offset, const uint64_t* scalars_dev, size_t n, size_t k,
                     int scalars_are_montgomery, uint64_t* out_xy, uint8_t* out_is_inf) {
    return msm_common(srs, basis, chunk, offset, scalars_dev, true, n, k, scalars_are_montgomery, out_xy, out_is_inf);
}
int kh_msm_points_batch(int curve, const uint64_t* xy, const uint8_t* inf, const uint64_t* scalars, size_t n, size_t k,
                        int scalars_are_montgomery, uint64_t* out_xy, uint8_t* out_is_inf) {
    KH_REQUIRE(out_xy && out_is_inf, "null output pointer");
    KH_REQUIRE(curve == KH_CURVE_VESTA || curve == KH_CURVE_PALLAS, "unknown curve id %d", curve);
    KH_REQUIRE((xy && scalars) || n == 0 || k == 0, "null input");
    int rc = ensure_init(); if (rc) return rc;
    Context& C = ctx();
    std::unique_lock<std::mutex> lk(C.mu);
    if (n == 0 || k == 0) { for (size_t j = 0; j < k; j++) { memset(out_xy + 8 * j, 0, 64); out_is_inf[j] = 1; } return KH_OK; }
    const size_t tot = n * k;
    int si = acquire_slot(&lk, C);
    KH_REQUIRE(si >= 0, "%s", slot_error(si));
    MsmSlot& S = C.slot[si];
    if ((rc = S.ws_points.reserve(tot * 64 + tot))) return rc;
    if ((rc = S.ws_scalars.reserve(tot * 32))) return rc;
    KH_HIP(hipMemcpyAsync(S.ws_points.p, xy, tot * 64, hipMemcpyHostToDevice, S.stream));
    MsmBasis b; b.pts = S.ws_points.p; b.n = tot; b.inf = nullptr; b.batch_stride = k > 1 ? n : 0;
    if (inf) {
        KH_HIP(hipMemcpyAsync((char*)S.ws_points.p + tot * 64, inf, tot, hipMemcpyHostToDevice, S.stream));
        b.inf = (const uint8_t*)S.ws_points.p + tot * 64;
    }
    KH_HIP(hipMemcpyAsync(S.ws_scalars.p, scalars, tot * 32, hipMemcpyHostToDevice, S.stream));
    if ((rc = msm_enqueue(C, S, curve, b, 0, S.ws_scalars.as<uint64_t>(), n, k, scalars_are_montgomery))) return rc;
    return wait_then_finish(lk, C, S, out_xy, out_is_inf);
}
int kh_msm_points(int curve, const uint64_t* xy, const uint8_t* inf, const uint64_t* scalars, size_t n,
                  int scalars_are_montgomery, uint64_t out_xy[8], uint8_t* out_is_inf) {
    return kh_msm_points_batch(curve, xy, inf, scalars, n, 1, scalars_are_montgomery, out_xy, out_is_inf);
}

// PolyComm::multi_scalar_mul (commitment.rs:350-394): chunk j of the result = sum over the commitments that HAVE a
// chunk j of scalar_i * com_i.chunks[j].  Ragged chunk lists become one batched MSM with the missing chunks flagged
// as points at infinity (which contribute nothing, exactly like the reference's filter_map).
int kh_polycomm_multi_scalar_mul(int curve, const uint64_t* chunks_xy, const uint8_t* chunks_inf, const size_t* num_chunks, size_t m,
                                 const uint64_t* scalars, uint64_t* out_xy, uint8_t* out_inf, size_t* out_count) {
    KH_REQUIRE(curve == KH_CURVE_VESTA || curve == KH_CURVE_PALLAS, "unknown curve id %d", curve);
    KH_REQUIRE(out_xy && out_inf && out_count, "kh_polycomm_multi_scalar_mul: null output");
    if (m == 0) { memset(out_xy, 0, 64); out_inf[0] = 1; *out_count = 1; return KH_OK; }      // vec![C::zero()]
    KH_REQUIRE(chunks_xy && num_chunks && scalars, "kh_polycomm_multi_scalar_mul: null input");
    size_t width = 0, total = 0;
    for (size_t i = 0; i < m; i++) { width = std::max(width, num_chunks[i]); total += num_chunks[i]; }
    if (width == 0) { *out_count = 0; return KH_OK; }
    std::vector<uint64_t> pts(width * m * 8, 0), sc(width * m * 4);
    std::vector<uint8_t> inf(width * m, 1);
    size_t pos = 0;
    for (size_t i = 0; i < m; i++) {
        for (size_t j = 0; j < num_chunks[i]; j++, pos++) {
            memcpy(&pts[(j * m + i) * 8], chunks_xy + 8 * pos, 64);
            inf[j * m + i] = chunks_inf ? chunks_inf[pos] : 0;
        }
        for (size_t j = 0; j < width; j++) memcpy(&sc[(j * m + i) * 4], scalars + 4 * i, 32);
    }
    (void)total;
    int rc = kh_msm_points_batch(curve, pts.data(), inf.data(), sc.data(), m, width, 1, out_xy, out_inf);
    if (rc) return rc;
    *out_count = width;
    return KH_OK;
}

// ---------------------------------------------------------------------------------- commitment wrappers
static bool limbs_zero(const uint64_t* p) { return (p[0] | p[1] | p[2] | p[3]) == 0; }

int kh_commit_non_hiding(kh_srs_t* srs, const uint64_t* coeffs, size_t len, size_t num_chunks,
                         uint64_t* out_xy, uint8_t* out_inf, size_t* out_count) {
    KH_ON_DEVICE_OF(srs);
    KH_REQUIRE(srs && out_xy && out_inf && out_count, "kh_commit_non_hiding: null argument");
    KH_REQUIRE(coeffs || len == 0, "null coefficients");
    while (len > 0 && limbs_zero(coeffs + 4 * (len - 1))) len--;       // DensePolynomial drops leading zero coefficients
    size_t written = 0;
    const size_t gsz = srs->n;
    if (len == 0) {                                                     // is_zero -> vec![G::zero()]
        memset(out_xy, 0, 64); out_inf[0] = 1; written = 1;
    } else {
        size_t full = len / gsz, rem = len % gsz;
        if (full > 0) {                                                 // whole chunks share the basis window [0, gsz)
            int rc = kh_msm_batch(srs, KH_BASIS_G, 0, 0, coeffs, gsz, full, 1, out_xy, out_inf);
            if (rc) return rc;
            written = full;
        }
        if (rem > 0) {                                                  // ragged last chunk: msm(&g[..rem], ..)
            int rc = kh_msm(srs, KH_BASIS_G, 0, 0, coeffs + 4 * full * gsz, rem, 1, out_xy + 8 * written, out_inf + written);
            if (rc) return rc;
            written++;
        }
    }
    for (; written < num_chunks; written++) { memset(out_xy + 8 * written, 0, 64); out_inf[written] = 1; }
    *out_count = written;
    return KH_OK;
}

int kh_commit_evaluations_non_hiding(kh_srs_t* srs, unsigned log2_domain, const uint64_t* evals, size_t evals_len,
                                     uint64_t* out_xy, uint8_t* out_inf, size_t* out_count) {
    KH_ON_DEVICE_OF(srs);
    KH_REQUIRE(srs && evals && out_xy && out_inf && out_count, "kh_commit_evaluations_non_hiding: null argument");
    const size_t n = (size_t)1 << log2_domain;
    KH_REQUIRE(evals_len >= n, "desired commitment domain size (%zu) greater than evaluations' domain size (%zu)", n, evals_len);
    KH_REQUIRE((evals_len & (evals_len - 1)) == 0, "evaluation domain size %zu is not a power of two", evals_len);
    int chunks = kh_srs_lagrange_chunks(srs, log2_domain);
    if (chunks <= 0) { set_error("Lagrange basis for domain 2^%u is not registered on this SRS", log2_domain); return KH_E_NOTFOUND; }
    const size_t stride = evals_len / n;
    std::vector<uint64_t> sub;
    const uint64_t* v = evals;
    if (stride > 1) {
        sub.resize(n * 4);
        for (size_t i = 0; i < n; i++) memcpy(&sub[4 * i], evals + 4 * stride * i, 32);
        v = sub.data();
    }
    for (int c = 0; c < chunks; c++) {
        int rc = kh_msm(srs, (int)log2_domain, (unsigned)c, 0, v, n, 1, out_xy + 8 * c, out_inf + c);
        if (rc) return rc;
    }
    *out_count = (size_t)chunks;
    return KH_OK;
}

int kh_srs_set_blinding_base(kh_srs_t* srs, const uint64_t h_xy[8]) {
    KH_REQUIRE(srs && h_xy, "null argument");
    std::lock_guard<std::mutex> lk(srs->h_mu);
    memcpy(srs->h, h_xy, 64);
    srs->h_table.clear(); srs->h_multiples.clear();
    return KH_OK;
}
int kh_srs_get_blinding_base(const kh_srs_t* srs, uint64_t h_xy[8]) {
    KH_REQUIRE(srs && h_xy, "null argument");
    memcpy(h_xy, srs->h, 64);
    return KH_OK;
}
// XYZZ -> affine for a list of points with ONE field inversion (Montgomery's trick over the ZZZ's)
static void xyzz_to_affine_batch(const khost::Crv& crv, const std::vector<khost::xyzz>& acc, uint64_t* out_xy, uint8_t* out_inf) {
    const khost::Fld& F = crv.F;
    const size_t k = acc.size();
    std::vector<khost::fe> pre(k + 1);
    pre[0] = F.f.one;
    for (size_t j = 0; j < k; j++) pre[j + 1] = crv.is_identity(acc[j]) ? pre[j] : F.mul(pre[j], acc[j].zzz);
    khost::fe inv = F.inv(pre[k]);
    for (size_t j = k; j-- > 0;) {
        if (crv.is_identity(acc[j])) { memset(out_xy + 8 * j, 0, 64); out_inf[j] = 1; continue; }
        const khost::fe izzz = F.mul(inv, pre[j]);
        inv = F.mul(inv, acc[j].zzz);
        const khost::fe izz = F.sqr(F.mul(izzz, acc[j].zz));
        const khost::fe x = F.mul(acc[j].x, izz), y = F.mul(acc[j].y, izzz);
        memcpy(out_xy + 8 * j, &x, 32); memcpy(out_xy + 8 * j + 4, &y, 32);
        out_inf[j] = 0;
    }
}
int kh_mask_custom(kh_srs_t* srs, const uint64_t* com_xy, const uint8_t* com_inf, size_t com_len,
                   const uint64_t* blinders, size_t blinders_len, uint64_t* out_xy, uint8_t* out_inf) {
    KH_REQUIRE(srs && com_xy && blinders && out_xy && out_inf, "kh_mask_custom: null argument");
    if (com_len != blinders_len) { set_error("BlindersDontMatch(%zu, %zu)", blinders_len, com_len); return KH_E_BLINDERS; }
    khost::Crv crv(srs->curve);
    khost::Fld SF(khost::scalar_field_id(srs->curve));
    {
        std::lock_guard<std::mutex> lk(srs->h_mu);
        if (srs->h_table.empty()) {
            khost::aff h; memcpy(&h, srs->h, 64);
            std::vector<khost::xyzz> T(32 * 255);
            khost::xyzz base = crv.from_affine(h);
            for (int i = 0; i < 32; i++) {
                T[i * 255] = base;
                for (int j = 1; j < 255; j++) T[i * 255 + j] = crv.add(T[i * 255 + j - 1], base);
                base = crv.add(T[i * 255 + 254], base);            // 256 * base
            }
            srs->h_table.swap(T);
        }
    }
    const khost::xyzz* T = srs->h_table.data();
    std::vector<khost::xyzz> acc(com_len);
    for (size_t j = 0; j < com_len; j++) {
        khost::fe w; memcpy(&w, blinders + 4 * j, 32);
        w = SF.from_mont(w);
        khost::xyzz s = crv.identity();
        for (int i = 0; i < 32; i++) {
            const unsigned byte = (unsigned)((w.l[i >> 3] >> (8 * (i & 7))) & 0xff);
            if (byte) s = crv.add(s, T[i * 255 + byte - 1]);
        }
        if (!(com_inf && com_inf[j])) { khost::aff c; memcpy(&c, com_xy + 8 * j, 64); s = crv.add(s, crv.from_affine(c)); }
        acc[j] = s;
    }
    xyzz_to_affine_batch(crv, acc, out_xy, out_inf);
    return KH_OK;
}

// ---------------------------------------------------------------------------------- host-side group sum
int kh_points_sum(int curve, const uint64_t* xy, const uint8_t* inf, size_t n, uint64_t out_xy[8], uint8_t* out_is_inf) {
    KH_REQUIRE(curve == KH_CURVE_VESTA || curve == KH_CURVE_PALLAS, "unknown curve id %d", curve);
    KH_REQUIRE(out_xy && out_is_inf && (xy || n == 0), "null argument");
    khost::Crv crv(curve);
    khost::xyzz acc = crv.identity();
    for (size_t i = 0; i < n; i++) {
        if (inf && inf[i]) continue;
        khost::aff p; memcpy(&p, xy + 8 * i, 64);
        acc = crv.add(acc, crv.from_affine(p));
    }
    khost::aff r; bool isinf = crv.to_affine(acc, r);
    memcpy(out_xy, &r, 64); *out_is_inf = isinf ? 1 : 0;
    return KH_OK;
}

// out_j = a_j + b_j for n pairs of affine points on the host, one field inversion in all: the second half of a masking whose blinding points
// [r_j] H (kh_mask_custom over commitments at infinity) were computed while the device was still busy with the commitment itself
int kh_points_add(int curve, const uint64_t* a_xy, const uint8_t* a_inf, const uint64_t* b_xy, const uint8_t* b_inf, size_t n, uint64_t* out_xy, uint8_t* out_inf) {
    KH_REQUIRE(curve == KH_CURVE_VESTA || curve == KH_CURVE_PALLAS, "unknown curve id %d", curve);
    KH_REQUIRE(n == 0 || (a_xy && b_xy && out_xy && out_inf), "kh_points_add: null argument");
    khost::Crv crv(curve);
    std::vector<khost::xyzz> acc(n);
    for (size_t j = 0; j < n; j++) {
        khost::xyzz s = crv.identity();
        if (!(a_inf && a_inf[j])) { khost::aff p; memcpy(&p, a_xy + 8 * j, 64); s = crv.from_affine(p); }
        if (!(b_inf && b_inf[j])) { khost::aff p; memcpy(&p, b_xy + 8 * j, 64); s = crv.add(s, crv.from_affine(p)); }
        acc[j] = s;
    }
    xyzz_to_affine_batch(crv, acc, out_xy, out_inf);
    return KH_OK;
}

// ---------------------------------------------------------------------------------- IPA round vector operations
int kh_ipa_fold_scalars(int field, const uint64_t* lo, const uint64_t* hi, const uint64_t u[4], size_t n, uint64_t* out) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    KH_REQUIRE((lo && hi && u && out) || n == 0, "null argument");
    int rc = ensure_init(); if (rc) return rc;
    if (n == 0) return KH_OK;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    return ipa_fold_scalars(C, field, lo, hi, u, n, out);
}
int kh_inner_product(int field, const uint64_t* a, const uint64_t* b, size_t n, uint64_t out[4]) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    KH_REQUIRE(out && ((a && b) || n == 0), "null argument");
    int rc = ensure_init(); if (rc) return rc;
    if (n == 0) { memset(out, 0, 32); return KH_OK; }
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    return ipa_inner_product(C, field, a, b, n, out);
}
int kh_ipa_fold_points(int curve, const uint64_t* g_lo, const uint64_t* g_hi, const uint64_t u[4], size_t n, uint64_t* out_xy, uint8_t* out_inf) {
    KH_REQUIRE(curve == KH_CURVE_VESTA || curve == KH_CURVE_PALLAS, "unknown curve id %d", curve);
    KH_REQUIRE((g_lo && g_hi && u && out_xy && out_inf) || n == 0, "null argument");
    int rc = ensure_init(); if (rc) return rc;
    if (n == 0) return KH_OK;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    return ipa_fold_points(C, curve, g_lo, g_hi, u, n, out_xy, out_inf);
}

int kh_ipa_fold_points_endo(int curve, const uint64_t* g_lo, const uint64_t* g_hi, const uint64_t chal[2], size_t n, uint64_t* out_xy, uint8_t* out_inf) {
    KH_REQUIRE(curve == KH_CURVE_VESTA || curve == KH_CURVE_PALLAS, "unknown curve id %d", curve);
    KH_REQUIRE((g_lo && g_hi && out_xy && out_inf) || n == 0, "null argument");
    KH_REQUIRE(chal, "null challenge");
    int rc = ensure_init(); if (rc) return rc;
    if (n == 0) return KH_OK;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    return ipa_fold_points_endo(C, curve, g_lo, g_hi, chal, n, out_xy, out_inf);
}
int kh_endos(int curve, uint64_t endo_q[4], uint64_t endo_r[4]) {
    KH_REQUIRE(curve == KH_CURVE_VESTA || curve == KH_CURVE_PALLAS, "unknown curve id %d", curve);
    KH_REQUIRE(endo_q && endo_r, "null argument");
    const EndoPair& e = cached_endos(curve);
    memcpy(endo_q, e.q, 32); memcpy(endo_r, e.r, 32);
    return KH_OK;
}

int kh_scalar_challenge_to_field(int curve, const uint64_t chal[2], uint64_t out[4]) {
    KH_REQUIRE(curve == KH_CURVE_VESTA || curve == KH_CURVE_PALLAS, "unknown curve id %d", curve);
    KH_REQUIRE(chal && out, "null argument");
    scalar_challenge_to_field(khost::scalar_field_id(curve), chal, cached_endos(curve).r, out);
    return KH_OK;
}

// ---------------------------------------------------------------------------------- coefficient-vector operations around the opening
int kh_combine_polys_dev(int field, const uint64_t* const* polys_dev, const size_t* lens, const size_t* num_chunks, size_t m,
                         const uint64_t polyscale[4], size_t srs_length, uint64_t* out_dev, size_t* out_len) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    KH_REQUIRE(out_dev && polyscale && srs_length > 0 && (m == 0 || (polys_dev && lens && num_chunks)), "kh_combine_polys_dev: bad argument");
    int rc = ensure_init(); if (rc) return rc;
    khost::Fld F(field);
    khost::fe ps; memcpy(&ps, polyscale, 32);
    khost::fe scale = F.f.one;
    std::vector<const uint64_t*> segs; std::vector<size_t> slen; std::vector<khost::fe> scales;
    size_t longest = 0;
    for (size_t i = 0; i < m; i++) {                                  // utils.rs:164-176
        size_t offset = 0;
        for (size_t c = 0; c < num_chunks[i]; c++) {
            const size_t lo = std::min(offset, lens[i]), hi = std::min(offset + srs_length, lens[i]);
            if (hi > lo) { segs.push_back(polys_dev[i] + 4 * lo); slen.push_back(hi - lo); scales.push_back(scale); longest = std::max(longest, hi - lo); }
            scale = F.mul(scale, ps);
            offset += srs_length;
        }
    }
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    if ((rc = poly_lincomb(C, field, segs.data(), slen.data(), (const uint64_t*)scales.data(), segs.size(), out_dev, srs_length))) return rc;
    C.mark_async();
    if (out_len) *out_len = longest;
    return KH_OK;
}
int kh_poly_lincomb_dev(int field, const uint64_t* const* polys_dev, const size_t* lens, const uint64_t* scalars, size_t m,
                        uint64_t* out_dev, size_t out_len) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    KH_REQUIRE((out_dev || out_len == 0) && (m == 0 || (polys_dev && lens && scalars)), "kh_poly_lincomb_dev: null argument");
    for (size_t i = 0; i < m; i++) KH_REQUIRE(lens[i] <= out_len, "polynomial %zu has %zu coefficients, the output %zu", i, lens[i], out_len);
    int rc = ensure_init(); if (rc) return rc;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    rc = poly_lincomb(C, field, polys_dev, lens, scalars, m, out_dev, out_len);
    if (rc == KH_OK) C.mark_async();
    return rc;
}
int kh_b_init_dev(int field, const uint64_t* elm, size_t k, const uint64_t evalscale[4], size_t padded_len, uint64_t* out_dev) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    KH_REQUIRE(out_dev && evalscale && (elm || k == 0), "kh_b_init_dev: null argument");
    int rc = ensure_init(); if (rc) return rc;
    khost::Fld F(field);
    khost::fe es; memcpy(&es, evalscale, 32);
    std::vector<khost::fe> scales(k);
    khost::fe sc = F.f.one;
    for (size_t i = 0; i < k; i++) { scales[i] = sc; sc = F.mul(sc, es); }
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    rc = poly_b_init(C, field, elm, (const uint64_t*)scales.data(), k, padded_len, out_dev);
    if (rc == KH_OK) C.mark_async();
    return rc;
}
int kh_evaluate_chunks_batch_dev(int field, const uint64_t* const* polys_dev, const size_t* lens, const size_t* num_chunks, size_t m,
                                 size_t chunk_size, const uint64_t* points, size_t npts, uint64_t* out) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    KH_REQUIRE(chunk_size > 0 && (m == 0 || (polys_dev && lens && num_chunks)) && (points || npts == 0), "kh_evaluate_chunks_batch_dev: bad argument");
    size_t total = 0;
    for (size_t j = 0; j < m; j++) {
        KH_REQUIRE(polys_dev[j] || lens[j] == 0, "polynomial %zu: null pointer", j);
        KH_REQUIRE((lens[j] + chunk_size - 1) / chunk_size <= num_chunks[j], "polynomial %zu: %zu coefficients need more than %zu chunks of %zu (assert_eq at utils/src/dense_polynomial.rs:63)", j, lens[j], num_chunks[j], chunk_size);
        total += num_chunks[j];
    }
    KH_REQUIRE(out || total * npts == 0, "null output");
    int rc = ensure_init(); if (rc) return rc;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    return poly_eval_chunks(C, field, polys_dev, lens, num_chunks, m, chunk_size, points, npts, out);
}
int kh_evaluate_chunks_dev(int field, const uint64_t* coeffs_dev, size_t len, size_t chunk_size, size_t num_chunks,
                           const uint64_t* points, size_t npts, uint64_t* out) {
    return kh_evaluate_chunks_batch_dev(field, &coeffs_dev, &len, &num_chunks, 1, chunk_size, points, npts, out);
}
int kh_divide_by_vanishing_poly_dev(int field, const uint64_t* f_dev, size_t len, unsigned log2_n, uint64_t* q_dev, uint64_t* r_dev) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    KH_REQUIRE(log2_n <= 32 && r_dev && (f_dev || len == 0), "kh_divide_by_vanishing_poly_dev: bad argument");
    const size_t n = (size_t)1 << log2_n;
    KH_REQUIRE(q_dev || len <= n, "null quotient buffer");
    int rc = ensure_init(); if (rc) return rc;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    rc = poly_div_vanishing(C, field, f_dev, len, n, q_dev, r_dev);
    if (rc == KH_OK) C.mark_async();
    return rc;
}

int kh_field_scan_dev(int field, int op, int reverse, uint64_t* data_dev, size_t n) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    KH_REQUIRE((op == KH_SCAN_ADD || op == KH_SCAN_MUL) && (data_dev || n == 0), "kh_field_scan_dev: bad argument");
    int rc = ensure_init(); if (rc) return rc;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    rc = poly_scan(C, field, op, reverse ? 1 : 0, data_dev, n);
    if (rc == KH_OK) C.mark_async();
    return rc;
}
int kh_batch_inversion_dev(int field, uint64_t* v_dev, size_t n) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    KH_REQUIRE(v_dev || n == 0, "null vector");
    int rc = ensure_init(); if (rc) return rc;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    rc = poly_batch_inversion(C, field, v_dev, n);
    if (rc == KH_OK) C.mark_async();
    return rc;
}
int kh_divide_by_linear_dev(int field, const uint64_t* f_dev, size_t len, const uint64_t a[4], uint64_t* q_dev, uint64_t rem[4]) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    KH_REQUIRE(a && rem && (f_dev || len == 0) && (q_dev || len <= 1), "kh_divide_by_linear_dev: null argument");
    int rc = ensure_init(); if (rc) return rc;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    return poly_divide_by_linear(C, field, f_dev, len, a, q_dev, rem);
}
int kh_divide_by_linear_async_dev(int field, const uint64_t* f_dev, size_t len, const uint64_t a[4], uint64_t* q_dev, uint64_t* rem_dev) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    KH_REQUIRE(a && (f_dev || len == 0) && (q_dev || len <= 1), "kh_divide_by_linear_async_dev: null argument");
    int rc = ensure_init(); if (rc) return rc;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    rc = poly_divide_by_linear(C, field, f_dev, len, a, q_dev, nullptr, rem_dev);
    if (rc == KH_OK) C.mark_async();
    return rc;
}
int kh_check_equal_dev(const uint64_t* v_dev, size_t n, const uint64_t* expect, uint32_t* flags_dev, unsigned bit) {
    KH_REQUIRE((v_dev || n == 0) && flags_dev && bit < 32, "kh_check_equal_dev: bad argument");
    int rc = ensure_init(); if (rc) return rc;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    rc = poly_check_equal(C, v_dev, n, expect, flags_dev, bit);
    if (rc == KH_OK) C.mark_async();
    return rc;
}
int kh_expr_evaluations_dev(int field, const uint32_t* tokens, size_t ntok, const uint64_t* const* cols_dev, const size_t* col_len, size_t ncols,
                            const uint64_t* constants, size_t nconsts, size_t rows, unsigned stride, unsigned next_shift, int accumulate,
                            uint64_t* out_dev) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    KH_REQUIRE(tokens && ntok > 0 && (out_dev || rows == 0) && stride > 0, "kh_expr_evaluations_dev: bad argument");
    KH_REQUIRE((ncols == 0 || (cols_dev && col_len)) && (nconsts == 0 || constants), "kh_expr_evaluations_dev: null table");
    int rc = ensure_init(); if (rc) return rc;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    rc = expr_run(C, field, tokens, ntok, cols_dev, col_len, ncols, constants, nconsts, rows, stride, next_shift, accumulate, out_dev);
    if (rc == KH_OK) C.mark_async();
    return rc;
}

int kh_gate_count(void) { return gate_count(); }
const char* kh_gate_name(int gate) { return gate_name(gate); }
int kh_gate_num_constants(int gate) { return gate_num_constants(gate); }
int kh_gate_constants(int field, int gate, const uint64_t alpha[4], const uint64_t endo[4], const uint64_t* params, size_t nparams, uint64_t* out) {
    KH_REQUIRE(out, "kh_gate_constants: null output");
    return gate_constants(field, gate, alpha, endo, params, nparams, out);
}
int kh_gate_evaluations_dev(int field, int gate, const uint64_t* const* cols_dev, size_t col_len, const uint64_t* constants, size_t nconsts, size_t rows,
                            unsigned stride, unsigned next_shift, int accumulate, uint64_t* out_dev) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    KH_REQUIRE(cols_dev && constants && (out_dev || rows == 0) && stride > 0, "kh_gate_evaluations_dev: bad argument");
    int rc = ensure_init(); if (rc) return rc;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    rc = gate_run(C, field, gate, cols_dev, col_len, constants, nconsts, rows, stride, next_shift, accumulate, out_dev);
    if (rc == KH_OK) C.mark_async();
    return rc;
}

// ---------------------------------------------------------------------------------- challenge polynomials (verifier side)
#define g_bp_chals (kh::ctx().scratch("bp_chals"))
#define g_bp_out (kh::ctx().scratch("bp_out"))
static std::mutex g_bp_mu;      // the coefficient buffer is shared: one challenge-polynomial call at a time
static int bpoly_to_device(Context& C, int field, const uint64_t* chals, unsigned rounds, size_t k, const uint64_t* rs, bool reduce) {
    const size_t len = (size_t)1 << rounds;
    int rc;
    if ((rc = g_bp_chals.reserve((k * rounds + k + 1) * 32))) return rc;
    if ((rc = g_bp_out.reserve((reduce ? 1 : k) * len * 32))) return rc;
    hipStream_t s = C.stream;
    if (k * rounds) KH_HIP(hipMemcpyAsync(g_bp_chals.p, chals, k * rounds * 32, hipMemcpyHostToDevice, s));
    uint64_t* rs_dev = nullptr;
    if (rs) { rs_dev = g_bp_chals.as<uint64_t>() + 4 * k * rounds; KH_HIP(hipMemcpyAsync(rs_dev, rs, k * 32, hipMemcpyHostToDevice, s)); }
    if ((rc = bpoly_run(s, field, g_bp_chals.as<uint64_t>(), rounds, k, rs_dev, g_bp_out.as<uint64_t>()))) return rc;
    KH_HIP(hipStreamSynchronize(s));                       // callers' buffers are released; the MSM may run on another slot's stream
    return KH_OK;
}
int kh_b_poly_coefficients(int field, const uint64_t* chals, unsigned rounds, size_t k, uint64_t* out) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    KH_REQUIRE(rounds <= 28, "2^%u coefficients is beyond any SRS", rounds);
    KH_REQUIRE(out && (chals || rounds == 0 || k == 0), "null argument");
    if (k == 0) return KH_OK;
    int rc = ensure_init(); if (rc) return rc;
    std::lock_guard<std::mutex> bl(g_bp_mu);
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    if ((rc = bpoly_to_device(C, field, chals, rounds, k, nullptr, false))) return rc;
    KH_HIP(hipMemcpy(out, g_bp_out.p, (k << rounds) * 32, hipMemcpyDeviceToHost));
    return KH_OK;
}
int kh_batch_dlog_accumulator_generate(kh_srs_t* srs, size_t num_comms, const uint64_t* chals, size_t chals_len, uint64_t* out_xy, uint8_t* out_inf) {
    KH_ON_DEVICE_OF(srs);
    KH_REQUIRE(srs, "null SRS handle");
    if (num_comms == 0) { KH_REQUIRE(chals_len == 0, "chals must be empty when num_comms is 0 (utils.rs:290-293)"); return KH_OK; }
    KH_REQUIRE(chals && out_xy && out_inf, "null argument");
    const size_t rounds = chals_len / num_comms;
    KH_REQUIRE(rounds > 0 && rounds <= 28 && rounds * num_comms == chals_len, "chals.len() = %zu is not a multiple of the round count (utils.rs:295-296)", chals_len);
    const size_t len = (size_t)1 << rounds;
    int rc = ensure_init(); if (rc) return rc;
    std::lock_guard<std::mutex> bl(g_bp_mu);
    {
        Context& C = ctx();
        std::lock_guard<std::mutex> lk(C.mu);
        if ((rc = bpoly_to_device(C, khost::scalar_field_id(srs->curve), chals, (unsigned)rounds, num_comms, nullptr, false))) return rc;
    }
    // msm_bigint pairs min(|g|, 2^rounds) terms; the k coefficient vectors are k x len contiguous on the device
    if (len <= srs->n) return kh_msm_batch_dev(srs, KH_BASIS_G, 0, 0, g_bp_out.as<uint64_t>(), len, num_comms, 1, out_xy, out_inf);
    for (size_t j = 0; j < num_comms; j++)
        if ((rc = kh_msm_batch_dev(srs, KH_BASIS_G, 0, 0, g_bp_out.as<uint64_t>() + 4 * j * len, srs->n, 1, 1, out_xy + 8 * j, out_inf + j))) return rc;
    return KH_OK;
}
int kh_batch_dlog_accumulator_check(kh_srs_t* srs, const uint64_t* comms_xy, const uint8_t* comms_inf, size_t k,
                                    const uint64_t* chals, size_t chals_len, const uint64_t r[4], int* ok) {
    KH_ON_DEVICE_OF(srs);
    KH_REQUIRE(srs && ok, "null argument");
    if (k == 0) { KH_REQUIRE(chals_len == 0, "chals must be empty without commitments (utils.rs:219-222)"); *ok = 1; return KH_OK; }
    KH_REQUIRE(comms_xy && chals && r, "null argument");
    const size_t rounds = chals_len / k;
    KH_REQUIRE(rounds > 0 && rounds <= 28 && rounds * k == chals_len, "chals.len() = %zu is not a multiple of the round count (utils.rs:224-225)", chals_len);
    KH_REQUIRE(((size_t)1 << rounds) == srs->n, "2^rounds = %zu terms against an SRS of %zu (assert_eq at utils.rs:264)", (size_t)1 << rounds, srs->n);
    int rc = ensure_init(); if (rc) return rc;
    const int field = khost::scalar_field_id(srs->curve);
    khost::Fld F(field);
    std::vector<khost::fe> rs(k);
    rs[0] = F.f.one;
    khost::fe rr; memcpy(&rr, r, 32);
    for (size_t i = 1; i < k; i++) rs[i] = F.mul(rs[i - 1], rr);
    std::vector<khost::fe> neg(k);
    for (size_t i = 0; i < k; i++) neg[i] = F.neg(rs[i]);
    std::lock_guard<std::mutex> bl(g_bp_mu);
    {
        Context& C = ctx();
        std::lock_guard<std::mutex> lk(C.mu);
        if ((rc = bpoly_to_device(C, field, chals, (unsigned)rounds, k, (const uint64_t*)neg.data(), true))) return rc;
    }
    uint64_t part[16]; uint8_t pinf[2];
    if ((rc = kh_msm_batch_dev(srs, KH_BASIS_G, 0, 0, g_bp_out.as<uint64_t>(), srs->n, 1, 1, part, pinf))) return rc;        // - sum_j r^j <s_j, G>
    if ((rc = kh_msm_points(srs->curve, comms_xy, comms_inf, (const uint64_t*)rs.data(), k, 1, part + 8, pinf + 1))) return rc; // + sum_j r^j C_j
    uint64_t tot[8]; uint8_t tinf = 0;
    if ((rc = kh_points_sum(srs->curve, part, pinf, 2, tot, &tinf))) return rc;
    *ok = tinf ? 1 : 0;
    return KH_OK;
}

// The one MSM of the batch verifier (SRS::verify, ipa.rs:301-502): sum_i w_i <s_i, g> over the resident tables, with the
// s_i = b_poly_coefficients(chals_i) built on the device, plus the proof-specific points (H, sg, U, L/R, commitments,
// delta with the scalars of ipa.rs:405-470) as an ad-hoc MSM; *is_zero = the verifier's `msm_res == zero` test.
int kh_ipa_verify_msm(kh_srs_t* srs, const uint64_t* chals, size_t chals_len, const uint64_t* sg_weights, size_t k,
                      const uint64_t* extra_xy, const uint8_t* extra_inf, const uint64_t* extra_scalars, size_t m, int* is_zero) {
    KH_ON_DEVICE_OF(srs);
    KH_REQUIRE(srs && is_zero, "null argument");
    KH_REQUIRE(k == 0 || (chals && sg_weights), "null challenges");
    KH_REQUIRE(m == 0 || (extra_xy && extra_scalars), "null extra points");
    int rc = ensure_init(); if (rc) return rc;
    uint64_t part[16]; uint8_t pinf[2] = {1, 1};
    memset(part, 0, sizeof(part));
    if (k) {
        const size_t rounds = chals_len / k;
        KH_REQUIRE(rounds > 0 && rounds <= 28 && rounds * k == chals_len, "chals_len = %zu is not k x rounds", chals_len);
        KH_REQUIRE(((size_t)1 << rounds) == srs->n, "2^rounds = %zu against an SRS of %zu (padded_length, ipa.rs:340-345)", (size_t)1 << rounds, srs->n);
        std::lock_guard<std::mutex> bl(g_bp_mu);
        {
            Context& C = ctx();
            std::lock_guard<std::mutex> lk(C.mu);
            if ((rc = bpoly_to_device(C, khost::scalar_field_id(srs->curve), chals, (unsigned)rounds, k, sg_weights, true))) return rc;
        }
        if ((rc = kh_msm_batch_dev(srs, KH_BASIS_G, 0, 0, g_bp_out.as<uint64_t>(), srs->n, 1, 1, part, pinf))) return rc;
    }
    if (m && (rc = kh_msm_points(srs->curve, extra_xy, extra_inf, extra_scalars, m, 1, part + 8, pinf + 1))) return rc;
    uint64_t tot[8]; uint8_t tinf = 0;
    if ((rc = kh_points_sum(srs->curve, part, pinf, 2, tot, &tinf))) return rc;
    *is_zero = tinf ? 1 : 0;
    return KH_OK;
}

// ---------------------------------------------------------------------------------- device-resident opening rounds
struct kh_ipa {
    kh_srs_t* srs = nullptr;
    int curve = 0, field = 0;
    size_t n = 0, cur = 0, ncoef = 1;     // basis size, current vector length N_j, challenge tensor length 2^j
    DevBuf *a = nullptr, *b = nullptr, *coef = nullptr;   // the SRS handle's workspace (ping-pong pairs)
    DevBuf *sc = nullptr, *partial = nullptr;             // srs->ipa_sc / ipa_partial
    int pp = 0;
    hipEvent_t ev = nullptr;              // orders the fold (library stream) before the next round's MSM (slot stream)
    bool lr_done = false;
    bool pending = false;                 // a recorded, not yet applied fold (kh_ipa_round_fold): the next round's step kernel applies it
    uint64_t u_p[4] = {0, 0, 0, 0}, ui_p[4] = {0, 0, 0, 0};
    size_t partial_words = 0;             // u64 words of `partial` before the step kernel's block counter
    std::vector<uint64_t> tab;            // H / U window multiples staged for the asynchronous upload of kh_ipa_begin
    int sg_slot = -1;                     // pipeline slot holding the two half-sums of sg launched during the last round (kh_ipa_open), -1: none
    bool sg_want = false;                 // kh_ipa_open asks the last kh_ipa_round_lr to launch them
    bool spread_broken = false;           // a round's MSM disproved MSM_SPREAD_SCALARS (MsmJob::spread_rerun): the later rounds run without the hint
    bool rb_glv = false;                          // the folded basis's tables are GLV tables (half the doubling chain; MsmBasis::glv)
    void* round_tab = nullptr; int round_c = 0;   // table set the round MSMs run over (the SRS's own, or its narrower-window second set)
    size_t tab_stride = 0;                        // points per window table of that set (the SRS's g_stride; N + 2 after the rebase)
    // Rebase (csrc/rebase.hip): after rb_j0 rounds the folded basis of rb_N = n / 2^rb_j0 points is materialised on a side stream while the rounds go on
    // over the original tables; the first round that finds it ready switches over (n, ncoef, round_tab, round_c, tab_stride change; a, b, coef do not).
    int rb_state = 0;                             // 0: not planned, 1: planned (launch behind round rb_j0 + 1's step kernel), 2: running, 3: switched, -1: abandoned
    unsigned rb_j0 = 0, round_no = 0;             // round_no: kh_ipa_round_lr calls so far
    size_t rb_N = 0; int rb_c = 0;
    uint64_t u_xy[8] = {0};                       // the U base of this opening (its multiples go into the rebased tables' last slot)
    uint64_t hu_stage[16] = {0};                  // H | U, staged for the asynchronous upload into those tables (lives as long as the opening)
};

static int ipa_begin_common(kh_srs_t* srs, const uint64_t* a, size_t a_len, const uint64_t* b, size_t b_len, const uint64_t u_base_xy[8], kh_ipa_t** out,
                            hipMemcpyKind kind) {
    KH_ON_DEVICE_OF(srs);
    KH_REQUIRE(srs && out && a && b && u_base_xy, "kh_ipa_begin: null argument");
    const size_t n = srs->n;
    KH_REQUIRE((n & (n - 1)) == 0, "the opening rounds need a power-of-two SRS (size %zu)", n);
    KH_REQUIRE(a_len <= n && a_len > 0, "polynomial of %zu coefficients does not fit the SRS (%zu)", a_len, n);
    KH_REQUIRE(b_len == n, "b must hold padded_length = %zu evaluation-point powers (got %zu)", n, b_len);
    int rc = ensure_init(); if (rc) return rc;
    // the reference's SRS::open takes &self and is called from several threads on clones of one SRS (GpuSrs is Clone + Sync): a second
    // opening on the same handle waits for the first to be freed; only the SAME thread beginning twice is a programming error.  The claim is
    // the HANDLE's (its own lock: the callers may be on different contexts) and is given back by kh_ipa_free -- or here, if beginning fails.
    {
        std::unique_lock<std::mutex> hl(srs->ipa_mu);
        KH_REQUIRE(!(srs->ipa_live && srs->ipa_owner == std::this_thread::get_id()), "another opening is in progress on this SRS in this thread (kh_ipa_free it first)");
        srs->ipa_cv.wait(hl, [&] { return !srs->ipa_live; });
        srs->ipa_live = true; srs->ipa_owner = std::this_thread::get_id();
    }
    struct Claim {
        kh_srs_t* s; bool keep = false;
        ~Claim() { if (!keep) { { std::lock_guard<std::mutex> hl(s->ipa_mu); s->ipa_live = false; } s->ipa_cv.notify_all(); } }
    } claim{srs};
    Context& C = ctx();
    std::unique_lock<std::mutex> lk(C.mu);
    static const bool begin_timing = getenv("KH_IPA_TIMING") != nullptr;
    const auto b1_ = std::chrono::steady_clock::now();
    std::unique_ptr<kh_ipa> st(new kh_ipa);
    st->srs = srs; st->curve = srs->curve; st->field = khost::scalar_field_id(srs->curve); st->n = n; st->cur = n;
    for (int i = 0; i < 2; i++) {
        if ((rc = srs->ipa_a[i].reserve(n * 32))) return rc;
        if ((rc = srs->ipa_b[i].reserve(n * 32))) return rc;
        if ((rc = srs->ipa_coef[i].reserve(n * 32))) return rc;
    }
    if ((rc = srs->ipa_sc.reserve(2 * (n + 2) * 32))) return rc;
    if ((rc = srs->ipa_sg.reserve(2 * n * 32))) return rc;             // scalars of the two halves of sg (kh_ipa_open)
    const size_t partial_bytes = 2 * (n / 512 + 1) * 32;               // block sums of the two inner products, then the last-block counter
    if ((rc = srs->ipa_partial.reserve(partial_bytes + 64))) return rc;
    KH_HIP(hipMemsetAsync((uint8_t*)srs->ipa_partial.p + partial_bytes, 0, 64, C.stream));
    if (!srs->ipa_ev) KH_HIP(hipEventCreateWithFlags(&srs->ipa_ev, hipEventDisableTiming));
    st->a = srs->ipa_a; st->b = srs->ipa_b; st->coef = srs->ipa_coef; st->sc = &srs->ipa_sc; st->partial = &srs->ipa_partial; st->ev = srs->ipa_ev; st->partial_words = partial_bytes / 8;
    // H and U into the two extra slots of every window table
    // the rounds' table set: the SRS's own (c = 16) or, with KH_IPA_C = c2, a second set with narrower windows built on first use
    static const int ipa_c = getenv("KH_IPA_C") ? atoi(getenv("KH_IPA_C")) : IPA_ROUND_C;
    const bool second = srs->g_precomp_c && ipa_c >= 12 && ipa_c < srs->g_precomp_c && n >= 4096;
    if (second && srs->g2_c != ipa_c) {
        const int W2 = (256 + ipa_c - 1) / ipa_c;
        if ((rc = srs->g2.reserve(srs->g_stride * 64 * W2))) return rc;
        KH_HIP(hipMemcpyAsync(srs->g2.p, srs->g.p, srs->g_stride * 64, hipMemcpyDeviceToDevice, C.stream));
        if ((rc = msm_precompute(C, srs->curve, srs->g2.p, nullptr, srs->g_stride, ipa_c))) return rc;
        KH_HIP(hipStreamSynchronize(C.stream));
        srs->g2_c = ipa_c; srs->h_multiples2.clear();
    }
    const int rc_c = second ? srs->g2_c : srs->g_precomp_c;                        // window width of the rounds' tables
    void* const round_tab = second ? srs->g2.p : srs->g.p;
    std::vector<uint64_t>& hm = second ? srs->h_multiples2 : srs->h_multiples;
    st->round_tab = round_tab; st->round_c = rc_c; st->tab_stride = srs->g_stride;
    memcpy(st->u_xy, u_base_xy, 64);
    // Plan the rebase (csrc/rebase.hip): the folded basis of N = 2^KH_IPA_REBASE_LOGN points (default 2^11; at least three rounds folded into it, at least 64
    // points) with window tables of KH_IPA_REBASE_C bits (default 13: 20 windows, 2^12 buckets), materialised from the c = 16 tables.  KH_IPA_REBASE=0: never.
    {
        static const bool rb_on = !(getenv("KH_IPA_REBASE") && atoi(getenv("KH_IPA_REBASE")) == 0);
        static const unsigned rb_logn = getenv("KH_IPA_REBASE_LOGN") ? (unsigned)atoi(getenv("KH_IPA_REBASE_LOGN")) : 11u;     // 2^16 proof, opening: 5.39 (off) / 5.26 (2^9) / 5.17 (2^10) / 5.11 (2^11) / 5.34 (2^12) ms: profiles/r06_rebase_sweep.txt
        static const int rb_c = getenv("KH_IPA_REBASE_C") ? std::min(16, std::max(7, atoi(getenv("KH_IPA_REBASE_C")))) : 13;     // 13: 20 windows, the top one still 8 bits wide (12, 14: a 3-bit top window = hot buckets)
        unsigned logn = 0; while (((size_t)1 << logn) < n) logn++;
        if (rb_on && !second && srs->g_precomp_c == 16 && logn >= 9) {
            const unsigned ln = std::max(6u, std::min(rb_logn, logn - 3));
            const size_t N = (size_t)1 << ln, Q = n >> ln;
            // KH_IPA_REBASE_GLV (default on): tables for the lower 128 bits and phi of them; off when the generated constants' eigenvalue is not this curve's endo_r
            static const bool glv_env = !(getenv("KH_IPA_REBASE_GLV") && atoi(getenv("KH_IPA_REBASE_GLV")) == 0);
            bool glv_ok = glv_env;
            if (glv_ok) {
                khost::Fld SFc(khost::scalar_field_id(srs->curve));
                khost::fe er; memcpy(&er, cached_endos(srs->curve).r, 32);
                const khost::fe can = SFc.from_mont(er);
                glv_ok = memcmp(can.l, msm_glv_lambda(khost::scalar_field_id(srs->curve)), 32) == 0;
            }
            st->rb_glv = glv_ok;
            const int W2 = std::max((256 + rb_c - 1) / rb_c, 2 * ((128 + rb_c - 1) / rb_c));
            bool ok = srs->ipa_rb_tab.reserve((N + 2) * 64 * (size_t)W2) == KH_OK && srs->ipa_rb_B.reserve(rebase_bucket_bytes(N)) == KH_OK &&
                      srs->ipa_rb_part.reserve(rebase_part_bytes(N)) == KH_OK && srs->ipa_rb_lists.reserve(rebase_list_bytes(Q) + 256) == KH_OK &&       // (+ H | U, affine)
                      srs->ipa_rb_scratch.reserve((size_t)W2 * (N + 2) * 128) == KH_OK;
            if (ok && !srs->ipa_rb_stream) {
                int lo = 0, hi = 0;
                (void)hipDeviceGetStreamPriorityRange(&lo, &hi);                 // lo = the numerically largest = the LEAST urgent
                // KH_IPA_REBASE_CUS=k: the side stream may only use the first k compute units (a CU-masked stream), so that the rounds' own kernels find
                // the rest of the chip untouched; 0 (default): no mask, lowest stream priority
                static const unsigned rb_cus = getenv("KH_IPA_REBASE_CUS") ? (unsigned)atoi(getenv("KH_IPA_REBASE_CUS")) : 0u;
                bool made = false;
                if (rb_cus > 0 && rb_cus < (unsigned)C.num_cus) {
                    std::vector<uint32_t> mask(((size_t)C.num_cus + 31) / 32, 0u);
                    for (unsigned cu = 0; cu < rb_cus; cu++) mask[cu / 32] |= 1u << (cu % 32);
                    made = hipExtStreamCreateWithCUMask(&srs->ipa_rb_stream, (uint32_t)mask.size(), mask.data()) == hipSuccess;
                    if (!made) { (void)hipGetLastError(); srs->ipa_rb_stream = nullptr; }
                }
                ok = (made || hipStreamCreateWithPriority(&srs->ipa_rb_stream, hipStreamNonBlocking, lo) == hipSuccess) &&
                     hipEventCreateWithFlags(&srs->ipa_rb_go, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&srs->ipa_rb_snap, hipEventDisableTiming) == hipSuccess &&
                     hipEventCreateWithFlags(&srs->ipa_rb_done, hipEventDisableTiming) == hipSuccess &&
                     hipHostMalloc((void**)&srs->ipa_rb_fail, 64, hipHostMallocCoherent | hipHostMallocMapped) == hipSuccess;
            }
            if (ok) { *srs->ipa_rb_fail = 0; st->rb_state = 1; st->rb_j0 = logn - ln; st->rb_N = N; st->rb_c = rb_c; }
            else { (void)hipGetLastError(); set_error(""); }                     // no memory for it: the rounds stay on the original tables
        }
    }
    const int W = rc_c ? (256 + rc_c - 1) / rc_c : 1;
    std::vector<uint64_t>& tab = st->tab;                  // lives as long as the opening: no synchronisation before returning
    std::vector<uint64_t> col((size_t)W * 8);
    tab.resize((size_t)W * 16);
    if (hm.size() != (size_t)W * 8) {                      // H is the SRS's: its window multiples are computed once
        hm.resize((size_t)W * 8);
        host_window_multiples(srs->curve, srs->h, W, rc_c, hm.data());
    }
    for (int w = 0; w < W; w++) memcpy(&tab[16 * w], &hm[8 * w], 64);
    const auto b2_ = std::chrono::steady_clock::now();
    host_window_multiples(srs->curve, u_base_xy, W, rc_c, col.data());
    const auto b3_ = std::chrono::steady_clock::now();
    for (int w = 0; w < W; w++) memcpy(&tab[16 * w + 8], &col[8 * w], 64);
    hipStream_t s = C.stream;
    KH_HIP(hipMemcpy2DAsync((char*)round_tab + n * 64, srs->g_stride * 64, tab.data(), 128, 128, W, hipMemcpyHostToDevice, s));
    if (a_len < n) KH_HIP(hipMemsetAsync((char*)st->a[0].p + a_len * 32, 0, (n - a_len) * 32, s));
    KH_HIP(hipMemcpyAsync(st->a[0].p, a, a_len * 32, kind, s));
    KH_HIP(hipMemcpyAsync(st->b[0].p, b, n * 32, kind, s));
    static const khost::fe ones[2] = {khost::field(0).one, khost::field(1).one};
    KH_HIP(hipMemcpyAsync(st->coef[0].p, &ones[st->field & 1], 32, hipMemcpyHostToDevice, s));
    if (kind != hipMemcpyDeviceToDevice) KH_HIP(hipStreamSynchronize(s));      // host inputs may be the caller's temporaries
    KH_HIP(hipEventRecord(st->ev, s));
    if (begin_timing) {
        auto us = [](std::chrono::steady_clock::time_point x, std::chrono::steady_clock::time_point y) { return std::chrono::duration<double, std::micro>(y - x).count(); };
        fprintf(stderr, "kh_ipa_begin: workspace %.0f us, U multiples %.0f, uploads + copies %.0f\n", us(b1_, b2_), us(b2_, b3_), us(b3_, std::chrono::steady_clock::now()));
    }
    claim.keep = true;
    *out = st.release();
    return KH_OK;
}
int kh_ipa_begin(kh_srs_t* srs, const uint64_t* a, size_t a_len, const uint64_t* b, size_t b_len, const uint64_t u_base_xy[8], kh_ipa_t** out) {
    return ipa_begin_common(srs, a, a_len, b, b_len, u_base_xy, out, hipMemcpyHostToDevice);
}
int kh_ipa_begin_dev(kh_srs_t* srs, const uint64_t* a_dev, size_t a_len, const uint64_t* b_dev, size_t b_len, const uint64_t u_base_xy[8], kh_ipa_t** out) {
    return ipa_begin_common(srs, a_dev, a_len, b_dev, b_len, u_base_xy, out, hipMemcpyDeviceToDevice);
}
int kh_ipa_rounds_left(const kh_ipa_t* st) {
    if (!st) return -1;
    int r = 0; for (size_t c = st->cur; c > 1; c >>= 1) r++;
    return r;
}
// During the LAST round of an opening: the two halves of sg (ipa.hip: k_sg_split) as one batch of two MSMs on a side slot.  They need only the
// challenges of the earlier rounds, so they run underneath the last round instead of after it (0.39 ms of every opening); queued right
// behind the round's own launches, so that their ~15 launches overlap its execution.  `p` / `had_fold`: the challenge tensor as it
// was BEFORE the round's step kernel (which only reads it).  Quietly does nothing when no other slot is free: kh_ipa_open then computes
// sg the plain way.  Called with the library lock held.
static void ipa_sg_prelaunch_locked(kh_ipa_t* st, Context& C, int p, bool had_fold) {
    int si = -1;
    for (int i = MSM_SLOTS - 1; i >= 1; i--) if (!C.slot[i].busy) { si = i; break; }
    if (si < 0) return;
    MsmSlot& S = C.slot[si];
    kh_srs_t* srs = st->srs;
    if (hipStreamWaitEvent(S.stream, st->ev, 0) != hipSuccess) return;
    if (ipa_sg_split(S.stream, st->field, st->coef[p].as<uint64_t>(), st->n, had_fold ? 1 : 0, st->u_p, srs->ipa_sg.as<uint64_t>())) return;
    MsmBasis bs; bs.pts = srs->g.p; bs.inf = nullptr; bs.n = srs->n; bs.stride = srs->g_stride; bs.precomp_c = srs->g_precomp_c;
    if (st->rb_state == 3) { bs.pts = st->round_tab; bs.n = st->n; bs.stride = st->tab_stride; bs.precomp_c = st->round_c; bs.glv = st->rb_glv; }     // sg = <coef_rel, g'>
    if (msm_enqueue(C, S, st->curve, bs, 0, srs->ipa_sg.as<uint64_t>(), st->n, 2, 1)) return;
    st->sg_slot = si;
}
// KH_IPA_TIMING: where a round's host time goes (accumulated per thread, printed and reset by kh_ipa_open)
struct IpaRoundProf { double slot = 0, step = 0, enqueue = 0, wait = 0, finish = 0; };
static thread_local IpaRoundProf tl_round_prof;
int kh_ipa_round_lr(kh_ipa_t* st, const uint64_t rand_l[4], const uint64_t rand_r[4], uint64_t lr_xy[16], uint8_t lr_inf[2]) {
    kh::DeviceScope dev_scope_((st && st->srs) ? st->srs->device : -1);
    KH_REQUIRE(st && rand_l && rand_r && lr_xy && lr_inf, "kh_ipa_round_lr: null argument");
    KH_REQUIRE(st->cur > 1, "no round left: the vectors are folded to length 1");
    KH_REQUIRE(!st->lr_done, "kh_ipa_round_fold must follow kh_ipa_round_lr");
    static const bool prof = getenv("KH_IPA_TIMING") != nullptr;
    const auto pt0 = std::chrono::steady_clock::now();
    auto us_since = [](std::chrono::steady_clock::time_point a) { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - a).count(); };
    Context& C = ctx();
    std::unique_lock<std::mutex> lk(C.mu);
    int si = acquire_slot(&lk, C, /*side_first=*/true);
    KH_REQUIRE(si >= 0, "%s", slot_error(si));
    MsmSlot& S = C.slot[si];
    KH_HIP(hipStreamWaitEvent(S.stream, st->ev, 0));
    kh_srs_t* const srs = st->srs;
    st->round_no++;
    // the rebase (csrc/rebase.hip): switch to the materialised folded basis as soon as its tables are complete
    if (st->rb_state == 2) {
        static const bool rb_wait = getenv("KH_IPA_REBASE_WAIT") && atoi(getenv("KH_IPA_REBASE_WAIT")) != 0;      // tests: the earliest possible switch, deterministically
        if (rb_wait) KH_HIP(hipEventSynchronize(srs->ipa_rb_done));
        const hipError_t qe = hipEventQuery(srs->ipa_rb_done);
        if (qe == hipSuccess) {
            if (__atomic_load_n(srs->ipa_rb_fail, __ATOMIC_ACQUIRE) != 0) { st->rb_state = -1; counter(CNT_REBASE_ABANDON)++; }
            else {
                KH_HIP(hipStreamWaitEvent(S.stream, srs->ipa_rb_done, 0));
                st->n = st->rb_N; st->ncoef >>= st->rb_j0;
                st->round_tab = srs->ipa_rb_tab.p; st->round_c = st->rb_c; st->tab_stride = st->rb_N + 2;
                st->rb_state = 3; counter(CNT_REBASE_SWITCH)++;
                static const bool rb_say = getenv("KH_IPA_TIMING") != nullptr;
                if (rb_say) fprintf(stderr, "kh_ipa: round %u runs over the rebased tables (%zu points, c = %d, %u rounds folded in)\n", st->round_no, st->rb_N, st->rb_c, st->rb_j0);
            }
        } else if (qe != hipErrorNotReady) { KH_HIP(qe); }
        else (void)hipGetLastError();
        // the step kernel of round j0 + 3 is the first to overwrite the challenge tensor the plan kernel reads (ping-pong buffers): order it behind the plan
        if (st->rb_state == 2 && st->round_no == st->rb_j0 + 3) KH_HIP(hipStreamWaitEvent(S.stream, srs->ipa_rb_snap, 0));
    }
    if (st->rb_state == 3) counter(CNT_REBASED_ROUNDS)++;
    const int p = st->pp, q = p ^ 1;
    const bool had_fold = st->pending;
    const auto pt1 = std::chrono::steady_clock::now();
    // one launch: the recorded fold of the previous round (if any), this round's inner products and expanded scalars
    // (round 5 also wrote the MSM's window digits from this kernel, saving the k_digits launch: measured, opening 5.76 vs 5.76 ms -- not kept)
    int rc = ipa_round_step(S.stream, st->field, st->pending ? 1 : 0, st->a[p].as<uint64_t>(), st->b[p].as<uint64_t>(), st->coef[p].as<uint64_t>(),
                            st->n, st->cur, st->pending ? st->ncoef / 2 : st->ncoef, st->u_p, st->ui_p,
                            st->a[q].as<uint64_t>(), st->b[q].as<uint64_t>(), st->coef[q].as<uint64_t>(), rand_l, rand_r,
                            st->sc->as<uint64_t>(), st->partial->as<uint64_t>(), (unsigned*)(st->partial->as<uint64_t>() + st->partial_words));
    if (rc) return rc;
    const auto pt2 = std::chrono::steady_clock::now();
    if (st->pending) { st->pp = q; st->pending = false; }
    if (st->rb_state == 1 && st->round_no == st->rb_j0 + 1) {
        // this round's step kernel has just written the tensor of the first j0 challenges (2^j0 entries, st->coef[st->pp]): materialise the folded basis
        // and its window tables behind it on the side stream, H and U in the two extra slots
        const size_t N = st->rb_N, Q = (size_t)1 << st->rb_j0;
        hipStream_t rs = srs->ipa_rb_stream;
        bool ok = hipEventRecord(srs->ipa_rb_go, S.stream) == hipSuccess && hipStreamWaitEvent(rs, srs->ipa_rb_go, 0) == hipSuccess;
        uint32_t* const lists = srs->ipa_rb_lists.as<uint32_t>();
        if (ok) ok = rebase_points(rs, st->curve, st->coef[st->pp].as<uint64_t>(), Q, srs->g.p, srs->g_stride, N, srs->ipa_rb_B.p, srs->ipa_rb_part.p, lists,
                                   srs->ipa_rb_snap) == KH_OK;                   // (ipa_rb_snap: behind the plan kernel, the tensor's only reader)
        memcpy(st->hu_stage, srs->h, 64); memcpy(st->hu_stage + 8, st->u_xy, 64);       // (H | U travel in the table kernel's arguments: rebase.hip, RbExtra)
        if (ok) ok = rebase_tables(rs, st->curve, srs->ipa_rb_part.p, N, st->hu_stage, 2, st->rb_c, srs->ipa_rb_scratch.p, srs->ipa_rb_tab.p, srs->ipa_rb_fail,
                                   st->rb_glv ? cached_endos(st->curve).q : nullptr) == KH_OK;
        if (ok) ok = hipEventRecord(srs->ipa_rb_done, rs) == hipSuccess;
        if (ok) { st->rb_state = 2; counter(CNT_REBASE_LAUNCH)++; }
        else { (void)hipGetLastError(); (void)hipStreamSynchronize(rs); st->rb_state = -1; counter(CNT_REBASE_ABANDON)++; }
    }
    MsmBasis bs; bs.pts = st->round_tab; bs.inf = nullptr; bs.n = st->tab_stride; bs.stride = st->tab_stride; bs.precomp_c = st->round_c; bs.glv = st->rb_state == 3 && st->rb_glv;
    // The round's MSM is six launches (digits, one-launch sort, accumulation, bucket sums, two reduction kernels) which the host queues in ~25 us while
    // the step kernel runs.  Its scalars are products with Fiat-Shamir challenges (MSM_SPREAD_SCALARS) until a round of this opening proves otherwise.
    const int round_flags = (st->spread_broken ? 0 : MSM_SPREAD_SCALARS) | MSM_LATENCY;
    if ((rc = msm_enqueue(C, S, st->curve, bs, 0, st->sc->as<uint64_t>(), st->n + 2, 2, 1, round_flags))) return rc;
    if (st->sg_want && st->cur == 2) { st->sg_want = false; ipa_sg_prelaunch_locked(st, C, p, had_fold); }
    const auto pt3 = std::chrono::steady_clock::now();
    if ((rc = wait_then_finish(lk, C, S, lr_xy, lr_inf))) return rc;
    if (S.job.spread_rerun) st->spread_broken = true;     // (the lock is held again: the slot's job is still this round's)
    if (prof) {
        IpaRoundProf& P = tl_round_prof;
        const double total_wait_finish = us_since(pt3);
        P.slot += std::chrono::duration<double, std::micro>(pt1 - pt0).count(); P.step += std::chrono::duration<double, std::micro>(pt2 - pt1).count();
        P.enqueue += std::chrono::duration<double, std::micro>(pt3 - pt2).count(); P.wait += tl_last_wait_us; P.finish += total_wait_finish - tl_last_wait_us;
    }
    st->lr_done = true;
    return KH_OK;
}
int kh_ipa_round_fold(kh_ipa_t* st, const uint64_t chal[2], uint64_t u_out[4], uint64_t u_inv_out[4]) {
    kh::DeviceScope dev_scope_((st && st->srs) ? st->srs->device : -1);
    KH_REQUIRE(st && chal, "kh_ipa_round_fold: null argument");
    KH_REQUIRE(st->lr_done, "kh_ipa_round_lr must precede kh_ipa_round_fold");
    uint64_t u[4], ui[4];
    scalar_challenge_to_field(st->field, chal, cached_endos(st->curve).r, u);
    KH_REQUIRE((u[0] | u[1] | u[2] | u[3]) != 0, "challenge maps to zero (u.inverse().unwrap() in ipa.rs:975)");
    host_field_inverse(st->field, u, ui);
    // recorded only: the next round's step kernel (or kh_ipa_finish) applies it -- one launch per round instead of four
    memcpy(st->u_p, u, 32); memcpy(st->ui_p, ui, 32);
    st->pending = true; st->cur /= 2; st->ncoef *= 2; st->lr_done = false;
    if (u_out) memcpy(u_out, u, 32);
    if (u_inv_out) memcpy(u_inv_out, ui, 32);
    return KH_OK;
}
// sg_xy == nullptr: only the last fold and a0, b0 (the caller has the halves of sg in flight on st->sg_slot)
static int ipa_finish_impl(kh_ipa_t* st, uint64_t a0[4], uint64_t b0[4], uint64_t* sg_xy, uint8_t* sg_inf) {
    kh::DeviceScope dev_scope_((st && st->srs) ? st->srs->device : -1);
    KH_REQUIRE(st->cur == 1, "%d rounds still to run", kh_ipa_rounds_left(st));
    Context& C = ctx();
    std::unique_lock<std::mutex> lk(C.mu);
    int si = acquire_slot(&lk, C);
    KH_REQUIRE(si >= 0, "%s", slot_error(si));
    MsmSlot& S = C.slot[si];
    KH_HIP(hipStreamWaitEvent(S.stream, st->ev, 0));
    int rc;
    if (st->pending) {                                     // the last round's fold (vectors of length 2 -> 1, the full challenge tensor)
        const int p0 = st->pp, q0 = p0 ^ 1;
        // With the halves of sg in flight (sg_xy == nullptr) the full tensor is not needed -- and must not be written: it would land in the
        // buffer k_sg_split reads on the side slot's stream, which nothing orders before this fold when the GPU is busy with other provers.
        if ((rc = ipa_round_fold(S.stream, st->field, st->a[p0].as<uint64_t>(), st->b[p0].as<uint64_t>(), st->coef[p0].as<uint64_t>(), 2 * st->cur, sg_xy ? st->ncoef / 2 : 0,
                                 st->u_p, st->ui_p, st->a[q0].as<uint64_t>(), st->b[q0].as<uint64_t>(), st->coef[q0].as<uint64_t>()))) return rc;
        st->pp = q0; st->pending = false;
    }
    const int p = st->pp;
    KH_HIP(hipMemcpyAsync(a0, st->a[p].p, 32, hipMemcpyDeviceToHost, S.stream));
    KH_HIP(hipMemcpyAsync(b0, st->b[p].p, 32, hipMemcpyDeviceToHost, S.stream));
    kh_srs_t* srs = st->srs;
    MsmBasis bs; bs.pts = srs->g.p; bs.inf = nullptr; bs.n = srs->n; bs.stride = srs->g_stride; bs.precomp_c = srs->g_precomp_c;
    if (st->rb_state == 3) { bs.pts = st->round_tab; bs.n = st->n; bs.stride = st->tab_stride; bs.precomp_c = st->round_c; bs.glv = st->rb_glv; }     // sg = <coef_rel, g'>
    if (!sg_xy) { KH_HIP(hipStreamSynchronize(S.stream)); return KH_OK; }
    if ((rc = msm_enqueue(C, S, st->curve, bs, 0, st->coef[p].as<uint64_t>(), st->n, 1, 1))) return rc;   // sg = <coef, G>
    return wait_then_finish(lk, C, S, sg_xy, sg_inf);
}
int kh_ipa_finish(kh_ipa_t* st, uint64_t a0[4], uint64_t b0[4], uint64_t sg_xy[8], uint8_t* sg_inf) {
    KH_REQUIRE(st && a0 && b0 && sg_xy && sg_inf, "kh_ipa_finish: null argument");
    return ipa_finish_impl(st, a0, b0, sg_xy, sg_inf);
}
// [u] B for u = scalar_challenge_to_field(chal) = a * endo_r + b with a, b < 2^67 (poseidon/src/sponge.rs:190-226): [a] phi(B) + [b] B,
// phi(x, y) = (endo_q x, y), as one joint double-and-add of 67 steps instead of a 255-bit ladder (0.10 -> 0.03 ms on the host).
// That [endo_r] P = phi(P) for the pair kh_endos returns is checked once per curve on the first point; if it ever failed the plain ladder runs.
static khost::xyzz endo_challenge_mul(const khost::Crv& crv, int curve, const khost::aff& B, const uint64_t chal[2], const uint64_t u[4]) {
    khost::Fld SF(khost::scalar_field_id(curve));
    const EndoPair& e = cached_endos(curve);
    khost::fe eq; memcpy(&eq, e.q, 32);
    khost::aff PB = B; PB.x = crv.F.mul(B.x, eq);
    const khost::xyzz P1 = crv.from_affine(B), P2 = crv.from_affine(PB);
    static int endo_ok[2] = {-1, -1};
    static std::mutex once_mu;
    {
        std::lock_guard<std::mutex> lk(once_mu);
        if (endo_ok[curve & 1] < 0) {
            khost::fe er; memcpy(&er, e.r, 32);
            khost::aff lhs; const bool inf = crv.to_affine(crv.mul_plain(P1, SF.from_mont(er)), lhs);
            endo_ok[curve & 1] = (!inf && memcmp(&lhs, &PB, 64) == 0) ? 1 : 0;
        }
    }
    if (endo_ok[curve & 1] != 1) { khost::fe uu; memcpy(&uu, u, 32); return crv.mul_plain(P1, SF.from_mont(uu)); }
    unsigned __int128 a = 2, b = 2;
    for (int i = 63; i >= 0; i--) {
        a <<= 1; b <<= 1;
        const uint64_t w = chal[i >> 5]; const int sh = 2 * (i & 31);
        const bool plus = (w >> sh) & 1;
        if ((w >> (sh + 1)) & 1) { if (plus) a += 1; else a -= 1; } else { if (plus) b += 1; else b -= 1; }
    }
    const khost::xyzz P12 = crv.add(P1, P2);
    khost::xyzz acc = crv.identity();
    for (int i = 67; i >= 0; i--) {
        acc = crv.dbl(acc);
        const int ba = (int)((a >> i) & 1), bb = (int)((b >> i) & 1);
        if (ba && bb) acc = crv.add(acc, P12); else if (ba) acc = crv.add(acc, P2); else if (bb) acc = crv.add(acc, P1);
    }
    return acc;
}
// A + [u] B from the two halves (affine, st->sg_slot) -> sg
static int ipa_sg_collect(kh_ipa_t* st, const uint64_t chal_last[2], const uint64_t u_last[4], uint64_t sg_xy[8], uint8_t* sg_inf) {
    kh::DeviceScope dev_scope_(st->srs->device);
    uint64_t ab[16]; uint8_t abi[2];
    {
        Context& C = ctx();
        std::unique_lock<std::mutex> lk(C.mu);
        const int si = st->sg_slot; st->sg_slot = -1;
        int rc = wait_then_finish(lk, C, C.slot[si], ab, abi); if (rc) return rc;
    }
    khost::Crv crv(st->curve);
    khost::xyzz acc = crv.identity();
    if (!abi[1]) {
        khost::aff B; memcpy(&B, ab + 8, 64);
        acc = endo_challenge_mul(crv, st->curve, B, chal_last, u_last);
    }
    if (!abi[0]) { khost::aff A; memcpy(&A, ab, 64); acc = crv.add(acc, crv.from_affine(A)); }
    khost::aff out; const bool inf = crv.to_affine(acc, out);
    memset(sg_xy, 0, 64); if (!inf) memcpy(sg_xy, &out, 64);
    *sg_inf = inf ? 1 : 0;
    return KH_OK;
}
void kh_ipa_free(kh_ipa_t* st) {
    if (!st) return;
    kh::DeviceScope dev_scope_(st->srs ? st->srs->device : -1);
    Context& C = ctx();
    if (st->sg_slot >= 0) {                                // an opening that failed after launching the halves of sg: release their slot
        uint64_t ab[16]; uint8_t abi[2];
        std::unique_lock<std::mutex> ul(C.mu);
        const int si = st->sg_slot; st->sg_slot = -1;
        (void)wait_then_finish(ul, C, C.slot[si], ab, abi);
    }
    std::lock_guard<std::mutex> lk(C.mu);
    (void)hipStreamSynchronize(C.stream);                 // a fold may still be in flight on the library stream
    kh_srs_t* const srs = st->srs;
    if (srs && st->rb_state >= 2 && srs->ipa_rb_stream) (void)hipStreamSynchronize(srs->ipa_rb_stream);      // a materialisation that was never switched to: the handle's next opening reuses its buffers
    delete st;
    if (srs) {                                            // an opening another thread wants to begin on this handle can start
        { std::lock_guard<std::mutex> hl(srs->ipa_mu); srs->ipa_live = false; }
        srs->ipa_cv.notify_all();
    }
    C.cv.notify_all();
}

// The whole tail of SRS::open (ipa.rs:898-1060) in one call, so that a device-resident prover has no per-round host
// language overhead: absorb the shifted combined inner product, U = to_group(challenge_fq), log2(n) rounds (L / R on the
// device, absorb, challenge, folds), then delta, c, z1, z2.  `blinders` = the values the reference draws from its RNG, in
// its order: (rand_l, rand_r) per round, then d, r_delta.  The sponge is advanced exactly as the reference advances it.
int kh_ipa_open(kh_srs_t* srs, const uint64_t* a_dev, size_t a_len, const uint64_t* b_dev, size_t b_len, const uint64_t combined_inner_product[4],
                const uint64_t blinding_factor[4], kh_sponge_t* sponge, const uint64_t* blinders, size_t blinders_len,
                uint64_t* lr_xy, uint8_t* lr_inf, uint64_t delta_xy[8], uint8_t* delta_inf, uint64_t z1[4], uint64_t z2[4], uint64_t sg_xy[8], uint8_t* sg_inf) {
    KH_REQUIRE(srs && a_dev && b_dev && combined_inner_product && blinding_factor && sponge && blinders && lr_xy && lr_inf && delta_xy && delta_inf && z1 && z2 && sg_xy && sg_inf,
               "kh_ipa_open: null argument");
    KH_ON_DEVICE_OF(srs);
    const size_t n = srs->n;
    KH_REQUIRE(n > 1 && (n & (n - 1)) == 0, "the opening needs a power-of-two SRS (size %zu)", n);
    size_t rounds = 0; while (((size_t)1 << rounds) < n) rounds++;
    KH_REQUIRE(blinders_len == 2 * rounds + 2, "kh_ipa_open: %zu blinders given, 2 * %zu rounds + 2 needed", blinders_len, rounds);
    const int curve = srs->curve, sfield = khost::scalar_field_id(curve);
    khost::Fld SF(sfield), BF(khost::base_field_id(curve));
    khost::Crv crv(curve);
    auto fe_of = [](const uint64_t* p) { khost::fe v; memcpy(&v, p, 32); return v; };
    // shift_scalar (commitment.rs:273-288) of the combined inner product, absorbed before U is squeezed (ipa.rs:898-913)
    {
        khost::fe two = SF.add(SF.f.one, SF.f.one), acc = SF.f.one;
        for (int i = 0; i < 255; i++) acc = SF.add(acc, acc);            // 2^255 = 2^(modulus bits) as a field element
        const khost::fe cip = fe_of(combined_inner_product);
        khost::fe sh;
        if (!khost::geq(SF.f.p, BF.f.p)) sh = SF.mul(SF.sub(cip, SF.add(acc, SF.f.one)), SF.inv(two));
        else sh = SF.sub(cip, acc);
        int rc = kh_sponge_absorb_fr(sponge, sh.l, 1); if (rc) return rc;
    }
    static const bool ipa_timing = getenv("KH_IPA_TIMING") != nullptr;      // phase split of one opening on stderr
    const auto tp0 = std::chrono::steady_clock::now();
    uint64_t t[4], u_base[8];
    int rc = kh_sponge_squeeze_field(sponge, t); if (rc) return rc;
    if ((rc = kh_group_map_to_group(curve, t, u_base))) return rc;
    kh_ipa_t* st = nullptr;
    const auto tp_map = std::chrono::steady_clock::now();
    if ((rc = kh_ipa_begin_dev(srs, a_dev, a_len, b_dev, b_len, u_base, &st))) return rc;
    struct Guard { kh_ipa_t* s; ~Guard() { kh_ipa_free(s); } } guard{st};
    khost::fe r_prime = fe_of(blinding_factor);
    const auto tp1 = std::chrono::steady_clock::now();
    double t_lr = 0, t_sponge = 0, t_fold = 0, per_round_us[32] = {0};
    static const bool sg_split = getenv("KH_NO_SG_SPLIT") == nullptr;
    uint64_t u_last[4] = {0, 0, 0, 0}, chal_last[2] = {0, 0};
    for (size_t r = 0; r < rounds; r++) {
        const uint64_t* rl = blinders + 8 * r; const uint64_t* rr = rl + 4;
        const auto q0 = std::chrono::steady_clock::now();
        if (r + 1 == rounds && sg_split) st->sg_want = true;
        if ((rc = kh_ipa_round_lr(st, rl, rr, lr_xy + 16 * r, lr_inf + 2 * r))) return rc;
        const auto q1 = std::chrono::steady_clock::now();
        if ((rc = kh_sponge_absorb_g(sponge, lr_xy + 16 * r, lr_inf + 2 * r, 2))) return rc;
        uint64_t chal[2], u[4], ui[4];
        if ((rc = kh_sponge_challenge(sponge, chal))) return rc;
        const auto q2 = std::chrono::steady_clock::now();
        if ((rc = kh_ipa_round_fold(st, chal, u, ui))) return rc;
        memcpy(u_last, u, 32); chal_last[0] = chal[0]; chal_last[1] = chal[1];
        if (ipa_timing) {
            const auto q3 = std::chrono::steady_clock::now();
            if (r < 32) per_round_us[r] = std::chrono::duration<double, std::micro>(q1 - q0).count();
            t_lr += std::chrono::duration<double, std::micro>(q1 - q0).count(); t_sponge += std::chrono::duration<double, std::micro>(q2 - q1).count();
            t_fold += std::chrono::duration<double, std::micro>(q3 - q2).count();
        }
        r_prime = SF.add(r_prime, SF.add(SF.mul(fe_of(rl), fe_of(ui)), SF.mul(fe_of(rr), fe_of(u))));       // ipa.rs:1021-1027
    }
    const auto tp2 = std::chrono::steady_clock::now();
    uint64_t a0[4], b0[4];
    if (st->sg_slot >= 0) {
        if ((rc = ipa_finish_impl(st, a0, b0, nullptr, nullptr))) return rc;
        if ((rc = ipa_sg_collect(st, chal_last, u_last, sg_xy, sg_inf))) return rc;
    } else if ((rc = kh_ipa_finish(st, a0, b0, sg_xy, sg_inf))) return rc;
    const auto tp3 = std::chrono::steady_clock::now();
    // delta = (g0 + [b0] U) * d + [r_delta] H  (ipa.rs:1036-1041), on the host: three scalar multiplications
    const khost::fe d = fe_of(blinders + 8 * rounds), r_delta = fe_of(blinders + 8 * rounds + 4);
    // [d] g0 + [b0 d] U by one joint double-and-add (Shamir's trick: 256 doublings shared), then + [r_delta] H through the fixed-base
    // table of kh_mask_custom (32 additions): 0.19 -> 0.09 ms against three separate 255-bit ladders
    {
        const khost::fe k1 = SF.from_mont(d), k2 = SF.from_mont(SF.mul(fe_of(b0), d));
        khost::aff ub; memcpy(&ub, u_base, 64);
        const khost::xyzz P2 = crv.from_affine(ub);
        khost::xyzz P1 = crv.identity(), P12 = P2;
        if (!*sg_inf) { khost::aff g0; memcpy(&g0, sg_xy, 64); P1 = crv.from_affine(g0); P12 = crv.add(P1, P2); }
        khost::xyzz acc = crv.identity();
        for (int i = 255; i >= 0; i--) {
            acc = crv.dbl(acc);
            const int b1 = (int)((k1.l[i >> 6] >> (i & 63)) & 1) & (*sg_inf ? 0 : 1), b2 = (int)((k2.l[i >> 6] >> (i & 63)) & 1);
            if (b1 && b2) acc = crv.add(acc, P12); else if (b1) acc = crv.add(acc, P1); else if (b2) acc = crv.add(acc, P2);
        }
        khost::aff pa; const bool pinf = crv.to_affine(acc, pa);
        uint64_t pxy[8]; uint8_t pi = pinf ? 1 : 0; memset(pxy, 0, 64); if (!pinf) memcpy(pxy, &pa, 64);
        if ((rc = kh_mask_custom(srs, pxy, &pi, 1, r_delta.l, 1, delta_xy, delta_inf))) return rc;
    }
    if ((rc = kh_sponge_absorb_g(sponge, delta_xy, delta_inf, 1))) return rc;
    uint64_t cc[2], c[4];
    if ((rc = kh_sponge_challenge(sponge, cc))) return rc;
    scalar_challenge_to_field(sfield, cc, cached_endos(curve).r, c);
    const khost::fe z1v = SF.add(SF.mul(fe_of(a0), fe_of(c)), d), z2v = SF.add(SF.mul(r_prime, fe_of(c)), r_delta);
    memcpy(z1, &z1v, 32); memcpy(z2, &z2v, 32);
    if (ipa_timing) {
        auto us = [](std::chrono::steady_clock::time_point x, std::chrono::steady_clock::time_point y) { return std::chrono::duration<double, std::micro>(y - x).count(); };
        { const IpaRoundProf P = tl_round_prof; tl_round_prof = IpaRoundProf();
          fprintf(stderr, "kh_ipa_open: per round inside launch + wait + finish: slot %.1f us, step kernel launch %.1f, MSM enqueue %.1f, wait %.1f, finish %.1f\n",
                  P.slot / rounds, P.step / rounds, P.enqueue / rounds, P.wait / rounds, P.finish / rounds); }
        { char line[512]; int o = 0; for (size_t r = 0; r < rounds && r < 32; r++) o += snprintf(line + o, sizeof line - o, " %.0f", per_round_us[r]);
          fprintf(stderr, "kh_ipa_open: launch + wait + finish per round, us:%s\n", line); }
        fprintf(stderr, "kh_ipa_open: begin %.0f us (of which shift + squeeze + to_group %.0f), %zu rounds %.0f us (per round: launch + wait + finish %.0f, sponge %.0f, to_field + inverse %.0f), sg %.0f us, delta / z1 / z2 %.0f us\n",
                us(tp0, tp1), us(tp0, tp_map), rounds, us(tp1, tp2), t_lr / rounds, t_sponge / rounds, t_fold / rounds, us(tp2, tp3), us(tp3, std::chrono::steady_clock::now()));
    }
    return KH_OK;
}

// ---------------------------------------------------------------------------------- NTT
int kh_domain_generator(int field, unsigned log2_n, uint64_t out[4]) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    KH_REQUIRE(log2_n <= 32 && out, "log2_n must be <= 32 (two-adicity of the Pasta fields)");
    khost::fe w = kh::ntt_host_root(field, log2_n, 0);
    memcpy(out, &w, 32);
    return KH_OK;
}
int kh_ntt_dev(int field, uint64_t* data_dev, unsigned log2_n, int inverse, size_t batch) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    KH_REQUIRE(log2_n <= 28, "log2_n = %u too large", log2_n);
    KH_REQUIRE(data_dev || batch == 0, "null data");
    int rc = ensure_init(); if (rc) return rc;
    if (batch == 0) return KH_OK;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    rc = ntt_run(C, field, data_dev, log2_n, inverse, batch);
    if (rc == KH_OK && hipEventRecord(C.order_ev, C.stream) == hipSuccess) C.main_dirty = true;   // a later MSM on another slot waits for this point
    return rc;
}
int kh_lde_dev(int field, const uint64_t* coeffs_dev, unsigned log2_n, unsigned log2_blowup, uint64_t* out_dev, size_t batch) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    KH_REQUIRE(log2_n + log2_blowup <= 28, "log2 size %u too large", log2_n + log2_blowup);
    KH_REQUIRE((coeffs_dev && out_dev) || batch == 0, "null data");
    int rc = ensure_init(); if (rc) return rc;
    if (batch == 0) return KH_OK;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    rc = lde_run(C, field, coeffs_dev, log2_n, log2_blowup, out_dev, batch);
    if (rc == KH_OK && hipEventRecord(C.order_ev, C.stream) == hipSuccess) C.main_dirty = true;
    return rc;
}
int kh_coset_ntt_dev(int field, const uint64_t* coeffs_dev, unsigned log2_n, const uint64_t shift[4], uint64_t* out_dev, size_t batch) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    KH_REQUIRE(log2_n <= 28 && shift, "kh_coset_ntt_dev: bad argument");
    KH_REQUIRE((coeffs_dev && out_dev) || batch == 0, "null data");
    int rc = ensure_init(); if (rc) return rc;
    if (batch == 0) return KH_OK;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    rc = poly_coset_ntt(C, field, coeffs_dev, log2_n, shift, out_dev, batch);
    if (rc == KH_OK && hipEventRecord(C.order_ev, C.stream) == hipSuccess) C.main_dirty = true;
    return rc;
}
// Host-pointer transforms (what the ark-poly patch calls: interpolate -> kh_ntt, evaluate_over_domain_by_ref -> kh_lde).  The reference calls them from
// 15 / 16 rayon workers at once (prover.rs:370-381, constraints.rs:488-494), one column each, and each call moves 2 + 2 (or 2 + 16) MB over PCIe around
// ~10-50 us of kernels.  Until round 4 a call held the library lock across upload, transform, download and a stream synchronisation on the one shared
// workspace: sixteen callers ran strictly one after the other at ~27 GB/s (profiles/r04_pcie_inclusive.txt).  Now a call uses the calling thread's own device buffers, moves its data
// on the calling thread's own copy stream WITHOUT the lock (uploads, downloads and their pageable-memory staging of different callers overlap, and PCIe
// runs both directions at once), and takes the lock only to queue its kernels on the main stream, ordered by events.  (A call owns the calling thread's
// transfer buffers, not blocks of the shared pool.)  A batched call is cut into column
// groups that go through the same three stages, so that group i's download runs under group i + 1's transform.
}  // extern "C"
namespace {
struct HostXferEvents {
    hipEvent_t up[KH_MAX_DEVICES] = {nullptr}, done[KH_MAX_DEVICES] = {nullptr};
    ~HostXferEvents() { for (int d = 0; d < KH_MAX_DEVICES; d++) { if (up[d]) (void)hipEventDestroy(up[d]); if (done[d]) (void)hipEventDestroy(done[d]); } }
};
// The calling thread's own device buffers for these transfers, per device, grown on demand: the shared block pool is the wrong place for them -- once a
// prover's buffers have filled it to its limit, a freed 16 MB block went back to the driver (hipFree synchronises the device) and the next call allocated
// afresh: 16 concurrent extensions took 11.6 ms inside bench.py's process against 5.2 ms in a fresh one.  The buffers live in a per-device REGISTRY, not in
// thread-local storage: a thread holds a pair while it exists (a rayon worker lives as long as its pool) and hands it back at exit without
// freeing anything (no hipFree from a TLS destructor); the next new thread adopts it; kh_trim frees every pair that is not inside a call at that moment.
static size_t xfer_keep_bytes() {          // per buffer, per thread; KH_XFER_KEEP_MB overrides.  64 MB holds what the reference's callers hand over one column at
    static const size_t v = getenv("KH_XFER_KEEP_MB") ? (size_t)atol(getenv("KH_XFER_KEEP_MB")) << 20 : (size_t)64 << 20;   // a time (2 MB in, 16 MB out at 2^16 -> 2^19) and a
    return v;                              // few columns batched; a 16-column batched extension (268 MB out) pays its allocation each time (~5 ms of PCIe beside it)
}
// in -> [upload] -> din -> run(din, dout, columns) -> dout -> [download] -> out, `batch` columns of in_col / out_col bytes, in groups
template <class Run>
int host_transform(const uint64_t* in, size_t in_col, uint64_t* out, size_t out_col, size_t batch, bool in_place, Run run) {
    static thread_local HostXferEvents ev;
    Context& C = ctx();
    const int d = C.device >= 0 && C.device < KH_MAX_DEVICES ? C.device : 0;
    hipStream_t cs = thread_copy_stream(); if (!cs) return KH_E_DEVICE;
    if (!ev.up[d]) { KH_HIP(hipEventCreateWithFlags(&ev.up[d], hipEventDisableTiming)); KH_HIP(hipEventCreateWithFlags(&ev.done[d], hipEventDisableTiming)); }
    // column groups: at most four, at least ~4 MB of output each (a group costs three stream hand-overs)
    size_t groups = batch < 4 ? batch : 4;
    while (groups > 1 && (batch / groups) * out_col < ((size_t)4 << 20)) groups--;
    XferPair* const bufs = xfer_acquire(d);
    XferGuard guard{bufs};
    int rc;
    if ((rc = bufs->in.reserve(batch * in_col))) return rc;
    if (!in_place && (rc = bufs->out.reserve(batch * out_col))) return rc;
    char* const di = (char*)bufs->in.p; char* const dst_dev = in_place ? di : (char*)bufs->out.p;
    // (the queueing in a lambda: whatever fails, the copy stream is drained before this returns -- a caller that sees an error may free `in` / `out`
    // at once, and a copy queued earlier in the call may still be reading or writing them)
    auto queue_all = [&]() -> int {
        size_t c0 = 0;
        for (size_t g = 0; g < groups; g++) {
            const size_t c1 = batch * (g + 1) / groups, cols = c1 - c0;
            KH_HIP(hipMemcpyAsync(di + c0 * in_col, (const char*)in + c0 * in_col, cols * in_col, hipMemcpyHostToDevice, cs));
            KH_HIP(hipEventRecord(ev.up[d], cs));
            {
                std::lock_guard<std::mutex> lk(C.mu);
                KH_HIP(hipStreamWaitEvent(C.stream, ev.up[d], 0));
                int rr;
                if ((rr = run(C, (uint64_t*)(di + c0 * in_col), (uint64_t*)(dst_dev + c0 * out_col), cols))) return rr;
                KH_HIP(hipEventRecord(ev.done[d], C.stream));
                C.mark_async();
            }
            KH_HIP(hipStreamWaitEvent(cs, ev.done[d], 0));
            KH_HIP(hipMemcpyAsync((char*)out + c0 * out_col, dst_dev + c0 * out_col, cols * out_col, hipMemcpyDeviceToHost, cs));
            c0 = c1;
        }
        return KH_OK;
    };
    rc = queue_all();
    const hipError_t drained = hipStreamSynchronize(cs);  // everything this call queued anywhere has finished: the buffers are free for the thread's next call
    if (rc == KH_OK && drained != hipSuccess) { set_error("hipStreamSynchronize (transfer stream): %s", hipGetErrorString(drained)); rc = KH_E_DEVICE; }
    if (rc != KH_OK) {                                     // the transform kernels of a failed call may still be queued on the library stream, reading the buffers
        std::lock_guard<std::mutex> lk(C.mu);
        (void)hipStreamSynchronize(C.stream);
    }
    // a thread keeps its two buffers for its next call -- up to a bound: after a huge batch they go back (the PCIe time of such a call dwarfs an allocation)
    if (bufs->in.cap > xfer_keep_bytes()) bufs->in.release();
    if (bufs->out.cap > xfer_keep_bytes()) bufs->out.release();
    if (rc != KH_OK) return rc;
    {
        std::lock_guard<std::mutex> lk(C.mu);
        collect_timings(C, C.timer);                       // (the phases of the LAST transform queued on this context: exact for a lone caller)
    }
    return KH_OK;
}
}  // namespace
extern "C" {
int kh_ntt_set_max_logr(unsigned max_logr) { return ntt_set_max_logr(max_logr); }
int kh_ntt(int field, uint64_t* data, unsigned log2_n, int inverse, size_t batch) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    KH_REQUIRE(log2_n <= 28, "log2_n = %u too large", log2_n);
    KH_REQUIRE(data || batch == 0, "null data");
    int rc = ensure_init(); if (rc) return rc;
    if (batch == 0) return KH_OK;
    const size_t col = ((size_t)1 << log2_n) * 32;
    return host_transform(data, col, data, col, batch, true,
                          [&](Context& C, uint64_t* din, uint64_t*, size_t cols) { return ntt_run(C, field, din, log2_n, inverse, cols); });
}
int kh_lde(int field, const uint64_t* coeffs, unsigned log2_n, unsigned log2_blowup, uint64_t* out, size_t batch) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    KH_REQUIRE(log2_n + log2_blowup <= 28, "log2 size %u too large", log2_n + log2_blowup);
    KH_REQUIRE((coeffs && out) || batch == 0, "null data");
    int rc = ensure_init(); if (rc) return rc;
    if (batch == 0) return KH_OK;
    const size_t in_col = ((size_t)1 << log2_n) * 32, out_col = in_col << log2_blowup;
    return host_transform(coeffs, in_col, out, out_col, batch, false,
                          [&](Context& C, uint64_t* din, uint64_t* dout, size_t cols) { return lde_run(C, field, din, log2_n, log2_blowup, dout, cols); });
}

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

// ---------------------------------------------------------------------------------- test hooks
// test hook of csrc/rebase.hip: g'[i] = sum_{q < Q} coef[q] * g[q N + i], i < N = n / Q, from the handle's c = 16 window tables (affine out)
int kh_debug_rebase_points(kh_srs_t* srs, const uint64_t* coef, size_t Q, uint64_t* out_xy, uint32_t* out_fail) {
    KH_ON_DEVICE_OF(srs);
    KH_REQUIRE(srs && coef && out_xy && out_fail, "kh_debug_rebase_points: null argument");
    KH_REQUIRE(srs->g_precomp_c == 16, "the handle has no c = 16 window tables");
    KH_REQUIRE(Q >= 1 && srs->n % Q == 0 && (srs->n / Q) % 64 == 0, "Q = %zu must divide the SRS size %zu into a multiple of 64", Q, srs->n);
    int rc = ensure_init(); if (rc) return rc;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    const size_t N = srs->n / Q;
    DevBuf B, part, lists, out, dcoef, fail, scratch;
    if ((rc = B.reserve(rebase_bucket_bytes(N))) || (rc = part.reserve(rebase_part_bytes(N))) || (rc = lists.reserve(rebase_list_bytes(Q))) || (rc = out.reserve(N * 64)) ||
        (rc = dcoef.reserve(Q * 32)) || (rc = fail.reserve(64)) || (rc = scratch.reserve(N * 128))) return rc;
    KH_HIP(hipMemcpyAsync(dcoef.p, coef, Q * 32, hipMemcpyHostToDevice, C.stream));
    KH_HIP(hipMemsetAsync(fail.p, 0, 64, C.stream));
    if ((rc = rebase_points(C.stream, srs->curve, dcoef.as<uint64_t>(), Q, srs->g.p, srs->g_stride, N, B.p, part.p, lists.p))) return rc;
    if ((rc = rebase_tables(C.stream, srs->curve, part.p, N, nullptr, 0, 256, scratch.p, out.p, fail.as<uint32_t>()))) return rc;      // (c = 256: one level = the points themselves, affine)
    KH_HIP(hipMemcpyAsync(out_xy, out.p, N * 64, hipMemcpyDeviceToHost, C.stream));
    KH_HIP(hipMemcpyAsync(out_fail, fail.p, 4, hipMemcpyDeviceToHost, C.stream));
    KH_HIP(hipStreamSynchronize(C.stream));
    return KH_OK;
}
int kh_debug_glv_split(int scalar_field, const uint64_t* scalars, size_t n, uint32_t* out) {
    KH_REQUIRE(scalar_field == KH_FIELD_FP || scalar_field == KH_FIELD_FQ, "unknown field id %d", scalar_field);
    KH_REQUIRE(scalars && out, "kh_debug_glv_split: null argument");
    int rc = ensure_init(); if (rc) return rc;
    if (n == 0) return KH_OK;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    DevBuf din, dout;
    if ((rc = din.reserve(n * 32)) || (rc = dout.reserve(n * 40))) return rc;
    KH_HIP(hipMemcpyAsync(din.p, scalars, n * 32, hipMemcpyHostToDevice, C.stream));
    if ((rc = msm_debug_glv_split(C.stream, scalar_field, din.as<uint64_t>(), n, dout.as<uint32_t>()))) return rc;
    KH_HIP(hipMemcpyAsync(out, dout.p, n * 40, hipMemcpyDeviceToHost, C.stream));
    KH_HIP(hipStreamSynchronize(C.stream));
    return KH_OK;
}
int kh_debug_field_op(int field, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
    KH_REQUIRE(a && out, "null argument");
    int rc = ensure_init(); if (rc) return rc;
    if (n == 0) return KH_OK;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    void *da = nullptr, *db = nullptr, *dout = nullptr;
    KH_HIP(hipMalloc(&da, n * 32)); KH_HIP(hipMalloc(&dout, n * 32));
    KH_HIP(hipMemcpy(da, a, n * 32, hipMemcpyHostToDevice));
    if (b) { KH_HIP(hipMalloc(&db, n * 32)); KH_HIP(hipMemcpy(db, b, n * 32, hipMemcpyHostToDevice)); }
    rc = debug_field_op(C, field, op, (const uint64_t*)da, (const uint64_t*)db, (uint64_t*)dout, n);
    if (rc == KH_OK) { KH_HIP(hipStreamSynchronize(C.stream)); KH_HIP(hipMemcpy(out, dout, n * 32, hipMemcpyDeviceToHost)); }
    (void)hipFree(da); (void)hipFree(dout); if (db) (void)hipFree(db);
    return rc;
}
int kh_debug_point_op(int curve, int op, const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* q_xy, const uint8_t* q_inf,
                      uint64_t* out_xy, uint8_t* out_inf, size_t n) {
    KH_REQUIRE(p_xy && q_xy && out_xy && out_inf, "null argument");
    int rc = ensure_init(); if (rc) return rc;
    if (n == 0) return KH_OK;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    void *dp, *dq, *dpi = nullptr, *dqi = nullptr, *dout;
    KH_HIP(hipMalloc(&dp, n * 64)); KH_HIP(hipMalloc(&dq, n * 64)); KH_HIP(hipMalloc(&dout, n * 128));
    KH_HIP(hipMemcpy(dp, p_xy, n * 64, hipMemcpyHostToDevice)); KH_HIP(hipMemcpy(dq, q_xy, n * 64, hipMemcpyHostToDevice));
    if (p_inf) { KH_HIP(hipMalloc(&dpi, n)); KH_HIP(hipMemcpy(dpi, p_inf, n, hipMemcpyHostToDevice)); }
    if (q_inf) { KH_HIP(hipMalloc(&dqi, n)); KH_HIP(hipMemcpy(dqi, q_inf, n, hipMemcpyHostToDevice)); }
    rc = debug_point_op(C, curve, op, (const uint64_t*)dp, (const uint8_t*)dpi, (const uint64_t*)dq, (const uint8_t*)dqi, (uint8_t*)dout, n);
    if (rc == KH_OK) {
        std::vector<khost::xyzz> res(n);
        KH_HIP(hipStreamSynchronize(C.stream));
        KH_HIP(hipMemcpy(res.data(), dout, n * 128, hipMemcpyDeviceToHost));
        khost::Crv crv(curve);
        for (size_t i = 0; i < n; i++) {
            const unsigned char* raw = (const unsigned char*)&res[i];
            bool handed = true;                                   // op 6: a record of 0xff bytes = madd29 declined (exceptional case possible)
            for (int k = 0; k < 128; k++) handed &= raw[k] == 0xff;
            if (handed) { memset(out_xy + 8 * i, 0, 64); out_inf[i] = 2; continue; }
            khost::aff a; bool inf = crv.to_affine(res[i], a);
            memcpy(out_xy + 8 * i, &a, 64); out_inf[i] = inf ? 1 : 0;
        }
    }
    (void)hipFree(dp); (void)hipFree(dq); (void)hipFree(dout); if (dpi) (void)hipFree(dpi); if (dqi) (void)hipFree(dqi);
    return rc;
}

}  // extern "C"

namespace kh {
// the column pass of kh_prover_index_create (csrc/prover.cpp; kernel in poly.hip): queued on the main stream like kh_ntt_dev
int index_columns_dev(int field, const uint8_t* selcol_dev, const uint32_t* wires_dev, const uint64_t* coeffs_dev, size_t n_gates, size_t n,
                      size_t zk_rows, const uint64_t* shifts, size_t ncol, uint64_t* d1_dev) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    KH_REQUIRE(d1_dev && shifts && (n_gates == 0 || (selcol_dev && wires_dev && coeffs_dev)), "index_columns_dev: null argument");
    int rc = ensure_init(); if (rc) return rc;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    rc = poly_index_columns(C, field, selcol_dev, wires_dev, coeffs_dev, n_gates, n, zk_rows, shifts, ncol, d1_dev);
    if (rc == KH_OK) C.mark_async();
    return rc;
}
}  // namespace kh
