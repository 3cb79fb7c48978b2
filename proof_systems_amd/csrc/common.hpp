// common.hpp -- context, error reporting and workspace management shared by the
// translation units of libkimchi_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <initializer_list>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "../../include/kimchi_hip.h"
#include "msm_plan.hpp"

namespace kh {

void set_error(const char* fmt, ...);

#define KH_HIP(expr)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            kh::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return KH_E_DEVICE;                                                              \
        }                                                                                    \
    } while (0)

#define KH_REQUIRE(cond, ...)                 \
    do {                                      \
        if (!(cond)) {                        \
            kh::set_error(__VA_ARGS__);       \
            return KH_E_INVALID;              \
        }                                     \
    } while (0)

// A grow-only device buffer (workspace), owning its allocation (move-only; freed with its owner).  Not thread-safe
// by itself: the owner (Context / SRS handle) serialises users with its mutex.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
    ~DevBuf() { release(); }
    int reserve(size_t bytes) {
        if (bytes <= cap) return KH_OK;
        if (p) { hipError_t e = hipFree(p); (void)e; p = nullptr; cap = 0; }
        size_t want = bytes + bytes / 8;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { set_error("hipMalloc(%zu) failed: %s", want, hipGetErrorString(e)); p = nullptr; return KH_E_NOMEM; }
        cap = want;
        return KH_OK;
    }
    void release() { if (p) { hipError_t e = hipFree(p); (void)e; } p = nullptr; cap = 0; }
    template <class T> T* as() const { return (T*)p; }
};

struct PhaseTimer {
    static constexpr int MAXP = 24;
    hipEvent_t k0 = nullptr, k1 = nullptr;    // start / stop of ONE kernel of interest (hipExtLaunchKernelGGL): its own duration,
    const char* kname = nullptr;              // without the barrier / dispatch gaps an event pair around the launch includes
    hipEvent_t ev[MAXP + 1];
    const char* names[MAXP];
    int n = 0;
    bool created = false;
    bool enabled = false;                     // kh_set_phase_timers: an event between two kernels costs the stream 6-10 us of idle time
    int init() {
        if (created) return KH_OK;
        for (int i = 0; i <= MAXP; i++) KH_HIP(hipEventCreate(&ev[i]));
        KH_HIP(hipEventCreate(&k0)); KH_HIP(hipEventCreate(&k1));
        created = true;
        return KH_OK;
    }
    void begin(hipStream_t s) { n = 0; kname = nullptr; if (enabled && created) (void)hipEventRecord(ev[0], s); }
    void mark(const char* name, hipStream_t s) {
        if (!enabled || !created || n >= MAXP) return;
        names[n] = name; n++;
        (void)hipEventRecord(ev[n], s);
    }
};

struct MsmBasis {
    const void* pts = nullptr;       // device, n x 64 B affine x||y (Montgomery); with precomp: W tables of n points
    const uint8_t* inf = nullptr;    // device, nullable per-point infinity flags
    size_t n = 0;                    // points per table
    int precomp_c = 0;               // 0: plain basis; else window width of the precomputed tables
    size_t stride = 0;               // points between consecutive window tables (0: = n)
    size_t batch_stride = 0;         // >0: MSM j of a batch uses points [j*batch_stride, ...) (independent bases)
    const void* wide_pts = nullptr;  // a second table set of the SAME basis with wide windows (same stride), used for big single MSMs
    int wide_c = 0;
    bool glv = false;                // the tables hold 2^(c w) P for the lower 128 bits and phi(2^(c w) P) behind them: scalars are split k = k1 + k2 lambda (rebase.hip)
};

// The job a slot has in flight: assigned once by msm_enqueue, read by msm_finish
struct MsmJob {
    // the inputs (msm_finish re-runs the job from them when the fused sort gave up or the spread hint did not hold)
    MsmBasis basis;
    size_t offset = 0;
    const uint64_t* scalars = nullptr;
    size_t n = 0, k = 0;
    int mont = 0, curve = 0;
    // every decision of msm_enqueue (msm_plan.hpp): msm_finish folds by it.  plan.ngroups == 0: nothing was launched (n == 0 or k == 0), the results are k identities
    MsmPlan plan;
    bool done_by_flag = false;         // the last kernel stores the slot's launch count into done_flag (MsmSlot)
    bool spread_rerun = false;         // set by msm_finish: the spread hint did not hold and the job was re-run without it
};

// One MSM pipeline slot: its own stream, workspace and result staging, so that several MSMs can be in
// flight (kh_msm_submit / kh_msm_wait).  k_accumulate29 is held to 112 VGPRs so that the sort kernels
// (4-16 VGPRs) of the NEXT job fit beside its 4 waves per SIMD: with three slots the sort of job i+2
// and the latency-bound tail of job i both run underneath the accumulation of job i+1.
struct MsmSlot {
    hipStream_t stream = nullptr;
    PhaseTimer timer;
    DevBuf ws_scalars, ws_digits, ws_hist, ws_cnt, ws_off, ws_ntask, ws_toff, ws_entries, ws_partial,
        ws_buckets, ws_seg, ws_out, ws_scan_tmp, ws_biglist, ws_points, ws_order, ws_chunks, ws_handed, ws_sync, ws_mid,
        ws_b29, ws_a1, ws_l2, ws_a2, ws_xlist;                       // wide windows (c = 20): lazy buckets, chunk sums (level one), run sums (level two), the 2 x 2^lo marginals
    void* pinned = nullptr; size_t pinned_cap = 0;      // host staging of the group sums (XYZZ)
    hipEvent_t done = nullptr;
    bool busy = false;                 // a job is pending (set by enqueue, cleared by finish)
    std::thread::id owner;             // the host thread that queued the pending job (acquire_slot: another thread's ticket will be waited for)
    uint64_t ticket = 0;
    MsmJob job;
    std::shared_ptr<std::atomic<int>> handle_jobs;     // the pending job counts among an SRS handle's jobs in flight (kh_srs::jobs); dropped when the slot is released
    // the one-launch sort (k_sort_fused) spins on grid barriers and needs all its blocks resident at once; if another PROCESS shares the
    // GPU they may never be -- its barriers then give up after a bounded spin, set this host-visible word, and msm_finish re-runs the job
    // with the multi-launch sort and disables the fused path for the process
    volatile uint32_t* host_abort = nullptr;          // pinned host memory, written by the kernel
    // MSM_SPREAD_SCALARS was a wrong promise: k_bucket_sum_q met a bucket with more task partials than a quad may sum in sequence, stored this word
    // (pinned) and left the bucket empty; msm_finish re-runs the job with the hot-bucket kernels (and reports it: MsmJob::spread_rerun)
    volatile uint32_t* spread_abort = nullptr;
    bool flag_unavailable = false;                     // no coherent host allocation for done_flag / pinned: completion by event
    bool pinned_coherent = false;
    // Completion by flag (round 5): when a job's LAST kernel is k_marginal_fin_q (it writes the result into `pinned` itself), the last block of that
    // kernel to finish also stores the slot's launch count into done_flag (pinned).  A synchronous waiter polls that word instead of hipEventQuery:
    // the host has the result ~5 us earlier (tools/latency/launch_latency.hip: 0.2 against 5.3 us after the kernel's last store).
    volatile uint32_t* done_flag = nullptr;           // pinned host memory
    DevBuf ws_done;                                    // [0] blocks finished in the running launch, [1] launches finished
    uint32_t done_expect = 0;                          // launches enqueued with the flag so far (what done_flag shows when the newest one has ended)
};
static constexpr int MSM_SLOTS = 4;

struct Context {
    std::mutex mu;            // serialises the host side of the C ABI (GPU waits happen outside it)
    std::condition_variable cv;        // a synchronous caller that finds every slot busy waits here for one to finish
    int sync_inflight = 0;             // slots some thread is currently blocked on (they WILL free up)
    std::multiset<std::thread::id> blocked_owners;   // threads waiting in acquire_slot (deadlock test: see there)
    int device = -1;
    bool ready = false;
    hipStream_t stream = nullptr;      // = slot[0].stream: the library's main stream (NTT / LDE / vector steps / opening folds)
    bool main_dirty = false;           // asynchronous work was queued on the main stream since the last kh_sync
    hipEvent_t order_ev = nullptr;     // orders device-resident producers on the main stream before an MSM on another slot's stream
    int num_cus = 256;
    size_t lds_per_cu = (size_t)160 << 10, lds_per_block = (size_t)64 << 10;    // hipDeviceProp: what holds k_acc_wide29 to a block count per CU
    bool fused_disabled = false;       // a k_sort_fused launch could not get all its blocks resident (shared GPU): multi-launch sort from then on
    PhaseTimer timer;                  // NTT / LDE phases (MSM phases are per slot)
    // last timings (filled after a sync)
    std::vector<std::pair<const char*, float>> last;      // names are string literals (kh_last_timings hands them out)
    MsmSlot slot[MSM_SLOTS];
    uint64_t next_ticket = 1;
    std::chrono::steady_clock::time_point last_sync_msm_arrival{};     // burst detection of the caller coalescing (msm_api.cpp: msm_common)
    // NTT workspace
    DevBuf ws_ntt_a, ws_ntt_b;
    void* pinned = nullptr; size_t pinned_cap = 0;
    // Pinned staging ring for the small argument tables of the vector steps (token programs, pointer tables, constants): a copy
    // from pageable memory drains the stream first, one from pinned memory is just another stream operation -- so kh_expr_* /
    // kh_poly_* can be queued back to back like kh_ntt_dev.  A slice is reused only after a full turn of the ring, which waits
    // for the main stream.  Guarded by `mu`.
    char* stage = nullptr; size_t stage_cap = 0, stage_cur = 0;
    // copies the parts back to back into the ring and queues ONE host-to-device copy of them to dst_dev on the main stream
    int stage_upload(void* dst_dev, std::initializer_list<std::pair<const void*, size_t>> parts);
    // asynchronous work was queued on the main stream: a later MSM on another slot's stream waits for this point
    void mark_async() { if (hipEventRecord(order_ev, stream) == hipSuccess) main_dirty = true; }
    // named scratch buffers / one-time flags of the other translation units (what used to be function-local statics:
    // a static is process-wide, these belong to ONE device).  References stay valid (std::map nodes do not move).
    std::mutex scratch_mu;
    std::map<std::string, DevBuf> scratch_bufs;
    std::set<std::string> done_flags;
    DevBuf& scratch(const char* name) { std::lock_guard<std::mutex> lk(scratch_mu); return scratch_bufs[name]; }
    bool once(const char* name) { std::lock_guard<std::mutex> lk(scratch_mu); return done_flags.insert(name).second; }   // true the first time
    void trim_scratch() { std::lock_guard<std::mutex> lk(scratch_mu); for (auto& kv : scratch_bufs) kv.second.release(); }
};
static constexpr int KH_MAX_DEVICES = 16;

// The context of the calling thread's CURRENT device: the one an enclosing DeviceScope selected (entry points that
// take an SRS / opening handle run on the handle's device), else the thread's kh_set_device / kh_init choice, else
// the process default (the first device initialised).
Context& ctx();
// initialises the current device's context on first use and binds the calling thread to it (hipSetDevice is
// per-thread state: every entry point must do this, not just the thread that ran kh_init)
int ensure_init();
struct DeviceScope {               // run the rest of this scope on `device` (no-op for device < 0)
    int prev;
    explicit DeviceScope(int device);
    ~DeviceScope();
};
void collect_timings(Context& c, PhaseTimer& t);
// process-wide event counters behind kh_counter (tests and tools read them: how often a rare path ran).  `name` must be one of COUNTER_NAMES.
enum CounterId { CNT_SPREAD_RETRY = 0, CNT_FUSED_RETRY, CNT_REBASE_LAUNCH, CNT_REBASE_SWITCH, CNT_REBASE_ABANDON, CNT_REBASED_ROUNDS, CNT_LOOKUP_SORTED_DEV, CNT_IPA_CONCURRENT, CNT_IPA_WAITED, CNT_TABLE_STAGED_WORDS, CNT_POINT_CODEC_LAUNCHES, CNT_POINT_CODEC_ENCODE_LAUNCHES, CNT_COUNT };
static constexpr const char* COUNTER_NAMES[CNT_COUNT] = {"spread_retry", "fused_retry", "rebase_launch", "rebase_switch", "rebase_abandon", "rebased_rounds", "lookup_sorted_dev", "ipa_concurrent", "ipa_waited", "table_staged_words", "point_codec_launches", "point_codec_encode_launches"};
std::atomic<uint64_t>& counter(CounterId id);

// device exclusive scan of n u32 values (in may alias out); tmp is workspace
int exclusive_scan_u32(const uint32_t* in, uint32_t* out, size_t n, DevBuf& tmp, hipStream_t s);

}  // namespace kh

// How a field id selects a kernel instantiation, for every launch that is keyed by the FIELD.  KERNEL names the instantiation with F for the field's
// parameters, in parentheses when it holds a comma:
//     KH_FIELD_LAUNCH(field, k_lincomb<F>, grid, block, 0, s, args...);      KH_FIELD_LAUNCH(field, (k_chain<F, true>), ...);
// The arguments are written once; a launch that fails returns KH_E_DEVICE from the calling function, like KH_HIP.
#define KH_FIELD_LAUNCH(field, KERNEL, grid, block, lds, stream, ...)                                                        \
    do {                                                                                                                     \
        if ((field) == KH_FIELD_FP) { using F = kh::FpParams; hipLaunchKernelGGL((KERNEL), grid, block, lds, stream, __VA_ARGS__); } \
        else { using F = kh::FqParams; hipLaunchKernelGGL((KERNEL), grid, block, lds, stream, __VA_ARGS__); }               \
        KH_HIP(hipGetLastError());                                                                                           \
    } while (0)
// The same for a launch keyed by the CURVE (the MSM side): F is the curve's BASE field, Fq for Vesta and Fp for Pallas (msm.hip: VestaCfg / PallasCfg).
// (rebase.hip and lagrange.hip dispatch whole functions templated on both fields instead.)
#define KH_CURVE_LAUNCH(curve, KERNEL, grid, block, lds, stream, ...)                                                        \
    do {                                                                                                                     \
        if ((curve) == KH_CURVE_VESTA) { using F = kh::FqParams; hipLaunchKernelGGL((KERNEL), grid, block, lds, stream, __VA_ARGS__); } \
        else { using F = kh::FpParams; hipLaunchKernelGGL((KERNEL), grid, block, lds, stream, __VA_ARGS__); }               \
        KH_HIP(hipGetLastError());                                                                                           \
    } while (0)
