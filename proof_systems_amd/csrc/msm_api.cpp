// msm_api.cpp -- MSM pipeline slots, submission and waiting, caller coalescing, kh_msm*, sharded MSM, kh_msm_points*, kh_commit_*.
#include <stdlib.h>
#include <algorithm>
#include <chrono>

#include "api_internal.hpp"
#include "env.hpp"

using namespace kh;

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
int kh::acquire_slot(std::unique_lock<std::mutex>* lk, Context& C, bool side_first) {
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
        static const long slot_wait_s = (long)env_int("KH_SLOT_WAIT_S", 30);
        if (std::chrono::steady_clock::now() - t_start > std::chrono::seconds(slot_wait_s)) return -2;
        C.blocked_owners.insert(me);
        C.cv.wait_for(*lk, std::chrono::milliseconds(50));  // (the time-out re-evaluates the deadlock test and the deadline)
        C.blocked_owners.erase(C.blocked_owners.find(me));
    }
}
const char* kh::slot_error(int si) {
    return si == -2 ? "no MSM pipeline slot came free and none changed hands for KH_SLOT_WAIT_S (default 30 s): a kh_msm_submit ticket was leaked (its owner never called kh_msm_wait)"
                    : "every MSM pipeline slot holds an un-waited kh_msm_submit ticket of this thread (or of threads blocked behind it): kh_msm_wait first";
}
// The basis a job on slot S will run with, and the job counted among the handle's jobs in flight (kh_srs::jobs) in the same step: kh_srs_set_wide_tables(srs, 0)
// on another thread -- another context, another lock -- either sees the job or has taken the wide set away before it was resolved.  The count is dropped when
// the slot is released (wait_then_finish), or by the guard when the job is never enqueued.
static void uncount_handle_job(MsmSlot& S) { if (S.handle_jobs) { (*S.handle_jobs)--; S.handle_jobs.reset(); } }
static int resolve_counted(kh_srs_t* srs, int basis, unsigned chunk, MsmBasis& b, MsmSlot& S) {
    KH_REQUIRE(srs != nullptr, "null SRS handle");
    std::lock_guard<std::mutex> wl(srs->wide_mu);
    int rc = resolve_basis(srs, basis, chunk, b); if (rc) return rc;
    S.handle_jobs = srs->jobs;
    (*S.handle_jobs)++;
    return KH_OK;
}
struct HandleJobGuard { MsmSlot& S; bool keep = false; ~HandleJobGuard() { if (!keep) uncount_handle_job(S); } };
// enqueue on a free slot; returns the slot index through *slot_out
static int msm_submit_locked(Context& C, kh_srs_t* srs, int basis, unsigned chunk, size_t offset, const uint64_t* scalars,
                             bool scalars_on_device, size_t n, size_t k, int mont, int* slot_out, std::unique_lock<std::mutex>* lk = nullptr,
                             bool host_async = false) {
    MsmBasis b; int rc = resolve_basis(srs, basis, chunk, b); if (rc) return rc;
    KH_REQUIRE(offset <= b.n, "offset %zu beyond basis length %zu", offset, b.n);
    size_t use = n < b.n - offset ? n : b.n - offset;      // msm_bigint semantics: min(len) pairs
    int si = acquire_slot(lk, C);
    KH_REQUIRE(si >= 0, "%s", slot_error(si));
    MsmSlot& S = C.slot[si];
    if ((rc = resolve_counted(srs, basis, chunk, b, S))) return rc;      // (again: acquire_slot may have dropped the lock, the basis map can have changed)
    HandleJobGuard counted{S};
    const uint64_t* sdev = scalars;
    if (!scalars_on_device && use > 0 && k > 0) {
        if ((rc = S.ws_scalars.reserve(k * use * 32))) return rc;
        // (host_async: kh_msm_submit_host returns while the job runs -- its copies go on the calling thread's copy stream, which that call waits for)
        hipStream_t up = S.stream; hipEvent_t uev = nullptr;
        if (host_async) { up = thread_copy_stream(); uev = thread_upload_event(); if (!up || !uev) return KH_E_DEVICE; }
        if (use == n) KH_HIP(hipMemcpyAsync(S.ws_scalars.p, scalars, k * n * 32, hipMemcpyHostToDevice, up));
        else for (size_t j = 0; j < k; j++)
            KH_HIP(hipMemcpyAsync((char*)S.ws_scalars.p + j * use * 32, scalars + j * n * 4, use * 32, hipMemcpyHostToDevice, up));
        if (host_async) { KH_HIP(hipEventRecord(uev, up)); KH_HIP(hipStreamWaitEvent(S.stream, uev, 0)); }
        sdev = S.ws_scalars.as<uint64_t>();
    } else if (scalars_on_device) {
        KH_REQUIRE(use == n || k == 1, "device-resident batched scalars must not exceed the basis window");
        // the scalars may be the output of an asynchronous kh_ntt_dev / kh_lde_dev still running on the main stream: wait for
        // the event recorded right behind the last such producer (NOT for whatever else slot 0's stream has queued since)
        if (C.main_dirty && S.stream != C.stream) KH_HIP(hipStreamWaitEvent(S.stream, C.order_ev, 0));
    }
    if ((rc = msm_enqueue(C, S, srs->curve, b, offset, sdev, use, k, mont))) return rc;
    counted.keep = true;
    *slot_out = si;
    return KH_OK;
}
// The GPU wait happens WITHOUT the library lock: the slot stays busy (nobody else can take it), other threads can
// enqueue on the remaining slots meanwhile (15 rayon workers call into the reference's SRS at once, prover.rs:329-351;
// two provers can run their opening rounds side by side).  The short host part runs under the lock again.
static thread_local double tl_last_wait_us = 0;           // spin / block part of the last wait_then_finish on this thread
double kh::last_wait_us() { return tl_last_wait_us; }
int kh::wait_then_finish(std::unique_lock<std::mutex>& lk, Context& C, MsmSlot& S, uint64_t* out_xy, uint8_t* out_inf) {
    hipEvent_t ev = S.done;
    // completion by flag (MsmSlot::done_flag): what the job's last kernel will store, read while the context is still locked
    const bool by_flag = S.job.done_by_flag && S.done_flag;
    const uint32_t expect = S.done_expect;
    C.sync_inflight++;
    lk.unlock();
    const auto tw0 = std::chrono::steady_clock::now();
    // a synchronous caller is latency-bound (an opening round is ~0.4 ms of GPU time, then ~40 us of transcript on this thread):
    // poll for up to a millisecond before blocking -- the blocking wait's wake-up alone costs 10-20 us
    static const long spin_us = (long)env_int("KH_SPIN_US", 1000);
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
    // the job (and any re-run of it inside msm_finish) reads its handle's tables no more -- or its wait failed (e != hipSuccess: a device error, after
    // which it is not known to have ended; the slot is given up all the same, and so is the count: srs.cpp, kh_srs_set_wide_tables)
    uncount_handle_job(S);
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
    static const bool coalesce_on = !env_flag("KH_NO_COALESCE", false);
    const auto now = std::chrono::steady_clock::now();
    const bool burst = C.last_sync_msm_arrival.time_since_epoch().count() != 0 &&
                       std::chrono::duration_cast<std::chrono::microseconds>(now - C.last_sync_msm_arrival).count() < 200;
    C.last_sync_msm_arrival = now;
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
        MsmSlot& S = C.slot[si];
        if ((r = resolve_counted(srs, basis, chunk, b, S))) return r;    // after the wait: the lock was dropped meanwhile
        HandleJobGuard counted{S};
        if ((r = S.ws_scalars.reserve(kk * n * 32))) return r;
        for (size_t j = 0; j < kk; j++)
            KH_HIP(hipMemcpyAsync((char*)S.ws_scalars.p + j * n * 32, grp->members[j].scalars, n * 32, hipMemcpyHostToDevice, S.stream));
        if ((r = msm_enqueue(C, S, srs->curve, b, offset, S.ws_scalars.as<uint64_t>(), n, kk, mont))) return r;
        counted.keep = true;
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

extern "C" {

int kh_msm_set_wide_min_n(size_t n) { msm_set_wide_min_n(n); return KH_OK; }
int kh_msm_set_sort_staging(unsigned entries, unsigned max_passes) {
    if (max_passes > 8) { set_error("kh_msm_set_sort_staging: at most 8 passes (got %u)", max_passes); return KH_E_INVALID; }
    msm_set_sort_staging(entries, max_passes); return KH_OK;
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

}  // extern "C"
