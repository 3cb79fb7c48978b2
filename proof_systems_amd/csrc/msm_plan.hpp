// msm_plan.hpp -- what an MSM of a given shape runs: the window and the table set, the sort path, every grid-deciding size and the geometry structs the
// kernels of msm.hip take by value.  msm_plan() is a pure function of MsmShape (the shape, the basis' facts, the device's sizes, the knobs as values):
// standard C++ only, no HIP and nothing of the library, so tests/cpp/test_msm_plan.cpp holds it to the kernels' conditions on the host.  msm.hip fills the
// shape (it reads the environment and the atomics), reserves the workspaces from the plan (msm_reserve) and launches from it (msm_enqueue_t).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

namespace kh {

typedef uint32_t u32;

// ------------------------------------------------------------------------------------ constants shared by the kernels and the plan
// flags of msm_enqueue: MSM_SPREAD_SCALARS (below, "the caller vouches ..."), MSM_LATENCY
static constexpr int MSM_SPREAD_SCALARS = 2;
static constexpr int MSM_LATENCY = 4;                              // the caller's critical path: the accumulation runs above the default wave priority too
constexpr int windows_of(int c) { return (256 + c - 1) / c; }      // windows of c bits that cover a 256-bit scalar = tables of a set
// the partitioned sort (msm.hip, "partitioned sort"): threads per block, partitions (pass A: the top 8 bits of the bucket), low bucket bits of pass B
static constexpr int PART_T = 1024, PART_P = 256, PART_LOW = 7;
static constexpr u32 PART2_MAXLOW = 11, PART2_MAXPASS = 8;  // (array bound; the launch's max_pass decides: 2 by default)
static constexpr u32 MAX_K = 256;           // upper bound of the task length (length bins of the task ordering)
static constexpr int FUSED_T = 1024, FUSED_KPT = 2, FUSED_G = 16, FUSED_B = 64;      // chunks per job <= FUSED_G, blocks <= FUSED_B
static constexpr int FUSED_V = 17, FUSED_C = 16;        // int4's of digits / cursors per thread (registers)
static constexpr u32 WIDE_XB = 32, WIDE_HOT_NT = 16;       // (a split bucket with more partials than WIDE_HOT_NT is summed by many waves)
static constexpr u32 CHUNK = 128;            // partials per chunk item = 8 per quad of a wave (cooperative additions)
static constexpr u32 SUM_PER_T = 2, SUM_BLK = 256 * SUM_PER_T;
static constexpr size_t B29_BYTES = 144;     // a lazy XYZZ point in memory (field29.cuh, "B29 record")
// MSM_SPREAD_SCALARS: the caller vouches that the scalars are spread like random ones (the opening rounds: products with Fiat-Shamir challenges), so
// no bucket collects a large share of the entries: the two-phase hot-bucket kernels are not launched (two empty dependent launches per MSM, ~20 us of
// the ~340 us of an opening round) and a bucket's quad sums however many task partials it finds -- correct for any input, slow for a skewed one.
// The promise is checked, not trusted: a bucket with more than SPREAD_MAX_NT task partials (a constant or sparse polynomial from a
// degenerate or adversarial witness puts n / K of them into one bucket per window) is left empty and reported through a pinned word; msm_finish re-runs
// the job with the hot-bucket kernels and reports it (MsmJob::spread_rerun): the opening passes the hint no more.
static constexpr u32 SPREAD_MAX_NT = 256;
// wide-path constants (measured best, tools/wide_sweep.py): ranks of one partition side by side in the accumulation order; blocks of the
// accumulation per CU (held down with dynamic LDS); log2 of the chunk length of the first reduction level
static constexpr u32 wide_og = 16, wide_acc_blocks = 3, wide_rlog = 4;
// k_part2_sort interleaves `og` consecutive ranks of a partition: og must divide the 2^(c - 9) buckets of a partition; k_wide_a1 cuts both digit
// planes into chunks of 2^rlog buckets and k_wide_l2 the chunks of a marginal into runs of 2^flog, flog = max(lo - rlog - 4, 1), which leaves a marginal at most 16 runs -- for every wide c (> 16)
static_assert((wide_og & (wide_og - 1)) == 0 && wide_og <= (1u << (17 - 9)) && wide_rlog >= 1 && wide_rlog + 2 <= 17 / 2, "wide-path constants");

// ------------------------------------------------------------------------------------ kernel arguments the plan fills
struct SortGeom {
    size_t n;       // scalars per MSM
    u32 nb;         // buckets per group = 2^(c-1)
    int S;          // slices per (window, msm)
    int W;          // windows
    int precomp;    // 1: all windows of an MSM share one bucket group
    size_t pt_stride;   // precomp: points per window table
    size_t pt_offset;   // first basis point used
    size_t pt_batch;    // index step between the bases of consecutive MSMs of a batch (0: shared basis)
};
struct KTab { uint8_t k[48]; };             // the task length per quarter octave of entries per bucket (msm.hip, pick_K; task_length_table below)
struct FusedGeom {
    u32 n, nb, W, k, bpg, split, sub, kpt, nkeys, room, kmin;     // sub = nb / split buckets per block
    KTab ktab;
    size_t pt_stride, pt_offset, pt_batch;
};
struct WideTasks { u32 room, kmin, nkeys; KTab ktab; };
struct MargGeom { u32 nb; u32 sh[3]; u32 wd[3]; };
struct WideGeom { u32 nb, lo, hi, rlog, flog; };      // buckets, the two digit widths, log2 of the chunk (level one) and of the run of chunks (level two)

// ------------------------------------------------------------------------------------ which bucket a lane reads: the kernels' index formulas, testable on the host
#if defined(__HIPCC__)                                       // (__forceinline__ spelled out, as in lookup_hash.hpp: not every file that gets here includes a HIP header)
#define KH_PLAN_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define KH_PLAN_FN inline
#endif
// the bucket whose digit j (field g.sh[j], g.wd[j] bits wide) is v and whose other bits are e, e < g.nb >> g.wd[j]: bucket e with the digit spliced in
KH_PLAN_FN u32 marginal_bucket(const MargGeom& g, u32 j, u32 v, u32 e) {
    const u32 s = g.sh[j], f = g.wd[j];
    return ((e >> s) << (s + f)) | (v << s) | (e & ((1u << s) - 1u));
}
// the three digit fields of a `bits`-bit bucket index, low to high, each at most 5 bits wide for bits <= 15 (k_marginals*: 32 blocks in x)
inline MargGeom marginal_geometry(u32 bits) {
    const u32 f0 = (bits + 2) / 3, f1 = (bits - f0 + 1) / 2, f2 = bits - f0 - f1;
    MargGeom mg;
    mg.nb = 1u << bits; mg.sh[0] = 0; mg.wd[0] = f0; mg.sh[1] = f0; mg.wd[1] = f1; mg.sh[2] = f0 + f1; mg.wd[2] = f2;
    return mg;
}
// room of the hot-bucket lists (msm.hip, list_hot_bucket) for nkeys buckets of at most max_tasks partials: big buckets <= nkeys; chunk items <= tasks / CHUNK + nkeys
inline size_t hot_list_cap(size_t nkeys, size_t max_tasks) { return nkeys + max_tasks / CHUNK + 2; }
// work item `out` of a group of k_wide_a1 (the index of its output record): first bucket and bucket stride of its chunk of 2^rlog buckets
KH_PLAN_FN void wide_a1_item(const WideGeom& g, u32 out, u32& t0, u32& tstride) {
    const u32 per = g.nb >> g.rlog;                        // items per plane
    if (out < per) { t0 = out << g.rlog; tstride = 1u; return; }
    const u32 cpm = (1u << g.hi) >> g.rlog, v = out - per, b = v / cpm, s = v - b * cpm;      // chunks per lo-digit marginal
    t0 = ((s << g.rlog) << g.lo) + b; tstride = 1u << g.lo;
}

// ------------------------------------------------------------------------------------ the plan
struct MsmShape {
    size_t n = 0, k = 0, offset = 0;       // scalars per MSM, MSMs, first basis point used
    int flags = 0;                         // MSM_SPREAD_SCALARS | MSM_LATENCY
    // the basis (MsmBasis)
    int precomp_c = 0;                     // 0: plain basis; else window width of the precomputed tables
    bool has_wide = false; int wide_c = 0; // a second table set with wide windows
    bool glv = false;
    size_t stride = 0, basis_n = 0, batch_stride = 0;
    // the device (Context)
    int num_cus = 256;
    size_t lds_per_cu = (size_t)160 << 10, lds_per_block = (size_t)64 << 10;
    // the knobs, as values
    size_t wide_min_n = ~(size_t)0;        // msm_wide_min_n()
    u32 stage_entries = 0, stage_maxpass = 0;      // msm_set_sort_staging
    bool fused_off = false;                // KH_NO_FUSED_SORT or Context::fused_disabled
    bool flag_off = false;                 // KH_NO_DONE_FLAG
    bool fin_quad = true;                  // !KH_NO_FIN_QUAD
};

enum MsmSort { SORT_PLAIN = 0, SORT_FUSED, SORT_PARTITIONED };     // k_hist .. k_scatter | k_sort_fused | k_part_*

struct MsmPlan {
    bool wide = false, glv = false;
    int precomp = 0, c = 0, W = 0;
    u32 nb = 0;                            // buckets per group = 2^(c-1)
    int S = 0, Sq = 0;                     // slices per (window, msm); histogram slices per key
    size_t ngroups = 0;                    // bucket groups; 0: nothing was launched (MsmJob)
    size_t nkeys = 0, M = 0, tot_e = 0;    // buckets of all groups; upper bound on entries; digits per MSM = W n
    bool few_groups = false, quad_sum = false, spread = false;
    u32 room = 0, kmin = 0; KTab ktab{};   // K = clamp(ceil(entries / room), kmin, MAX_K), on the device (pick_K)
    size_t max_tasks = 0, bigcap = 0, slist_off = 0;       // slist_off: words of ws_xlist in front of the split buckets' keys
    u32 acc_prio = 0;
    MsmSort sort = SORT_PLAIN;
    SortGeom g{};
    FusedGeom fg{};
    u32 part_low = 0, part_nblk = 0; size_t part_size = 0;
    WideGeom wg{};
    size_t wide_acc_lds = 0;
    u32 stage_now = 0, part2_maxpass = 0; size_t part2_lds = 0;        // k_part2_sort's staged scatter
    u32 acc_blocks = 0, wide_items = 0, wide_runs = 0;     // grids: the accumulation; threads of k_wide_a1; of k_wide_l2
    u32 m = 0, nseg = 0, nblk1 = 0, planes = 0;
    MargGeom mg{};
    size_t tail_groups = 0, nout = 0;
    bool direct_out = false;               // the last kernel writes the result to host memory itself (k_marginal_fin_q)
    bool want_flag = false;                // completion by flag, if the slot can have it (msm_reserve)
};

inline int msm_pick_window(size_t n) {
    int lg = 0; while (((size_t)1 << (lg + 1)) <= n) lg++;
    int c = lg - 3;
    if (c < 4) c = 4;
    if (c > 16) c = 16;
    return c;
}

// the task-length table of pick_K for a launch with `nkeys` buckets on `cus` compute units (cached per bucket count)
inline KTab task_length_table(size_t nkeys, u32 cus) {
    static std::mutex mu;
    static std::map<std::pair<size_t, u32>, KTab> cache;
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find({nkeys, cus});
    if (it != cache.end()) return it->second;
    KTab t{};
    for (int idx = 0; idx < 48; idx++) {
        const double m = pow(2.0, (idx - 8) / 4.0);
        std::vector<double> p(1, exp(-m));                                   // Poisson(m), up to the far tail
        for (int c = 1; c < (int)(m + 12 * sqrt(m) + 24); c++) p.push_back(p.back() * m / c);
        auto tasks_per_bucket = [&](int K) { double s = 0; for (size_t c = 1; c < p.size(); c++) s += p[c] * (double)((c + K - 1) / K); return s; };
        if (ceil(ceil((double)nkeys * tasks_per_bucket(8) / 256.0) / cus) > 6) { t.k[idx] = 0; continue; }     // a big job: the total decides
        double best = 1e300; int bk = 8;
        for (int K = 4; K <= 32; K++) {
            const double tpb = tasks_per_bucket(K);
            const double blocks = ceil((double)nkeys * tpb / 256.0);
            const double len = std::min<double>(K, m + 2.3 * sqrt(m));
            const double cost = ceil(blocks / cus) * len + 2.0 * tpb;
            if (cost < best - 1e-9) { best = cost; bk = K; }
        }
        t.k[idx] = (uint8_t)bk;
    }
    cache[{nkeys, cus}] = t;
    return t;
}

// Every decision of an MSM, before anything is reserved or launched.  Returns non-zero and says why for a shape the kernels cannot index.
inline int msm_plan(const MsmShape& sh, MsmPlan& P, const char** why) {
    const size_t n = sh.n, k = sh.k;
    P = MsmPlan{};
    // wide windows (a second table set, c = 20: msm.hpp) for big single MSMs: 13 instead of 16 additions per scalar.  Needs the wide sort's
    // record (<= 65,536 digits per pass-A block, <= 1024 blocks).
    const bool wide = P.wide = sh.has_wide && sh.wide_c > 16 && sh.wide_c - 9 <= (int)PART2_MAXLOW && n >= sh.wide_min_n && k <= 4 &&
                               (size_t)windows_of(sh.wide_c) * n <= ((size_t)1 << 26);
    const int c = P.c = wide ? sh.wide_c : (sh.precomp_c ? sh.precomp_c : msm_pick_window(n));
    P.glv = sh.glv && !wide && sh.precomp_c != 0;      // rows 0 .. W/2-1: 2^(c w) P, rows W/2 .. W-1: phi of them (csrc/rebase.hip)
    const int W = P.W = P.glv ? 2 * ((128 + c - 1) / c) : windows_of(c);
    const u32 nb = P.nb = 1u << (c - 1);
    const int precomp = P.precomp = (wide || sh.precomp_c) ? 1 : 0;
    // slices per (window, msm): enough blocks to fill the chip (~512), no more -- the per-slice histograms
    // cost nkeys x W x S words of traffic in k_key_totals, which dominates the sort of a batch
    int S = (int)(n / 32768); if (S < 1) S = 1; if (S > 16) S = 16;
    { int want = (int)(512 / ((size_t)W * k)); if (want < 1) want = 1; if (S > want) S = want; }
    P.S = S;
    const size_t tab_stride = sh.stride ? sh.stride : sh.basis_n;
    P.g = SortGeom{n, nb, S, W, precomp, tab_stride, sh.offset, sh.batch_stride};
    const size_t ngroups = P.ngroups = precomp ? k : k * (size_t)W;
    // few groups: the latency path of the bucket sums and marginals, lane-cooperative additions (coop.cuh)
    P.few_groups = ngroups <= 8;                            // 5 / 7 / 8 MSMs of 2^16: 0.94 / 1.09 / 1.14 -> 0.85 / 1.05 / 1.09 ms against 4
    P.quad_sum = !wide && precomp && P.few_groups;          // k_bucket_sum_q, the only bucket-sum kernel that takes the spread hint
    P.spread = P.quad_sum && (sh.flags & MSM_SPREAD_SCALARS) != 0;
    P.acc_prio = (sh.flags & MSM_LATENCY) ? 1u : 0u;
    P.Sq = precomp ? W * S : S;
    const size_t nkeys = P.nkeys = ngroups * nb;
    const size_t M = P.M = n * (size_t)W * k;           // upper bound on entries
    P.tot_e = (size_t)W * n;
    // Task size: the accumulation is one long dependent chain per thread, so a launch that needs
    // 1.1 "rounds" of resident threads pays a whole extra chain at 10 % occupancy (measured: 1.80 ms
    // instead of 1.72 ms at 2^20).  Size K so that all tasks are resident at once (4 waves/SIMD =
    // 1024 threads per CU) whenever the bucket count allows it.
    const size_t cap = (size_t)sh.num_cus * 256 * 4;
    size_t room_sz = cap / 4;                              // many buckets: about one task per bucket anyway
    if (nkeys < cap / 2) room_sz = cap - cap / 16 - nkeys / 2;   // ~ half of the buckets add a remainder task
    P.room = (u32)room_sz;                                  // K = clamp(ceil(entries / room), 8, MAX_K), on the device
    P.kmin = 8;
    P.ktab = precomp ? task_length_table(nkeys, (u32)sh.num_cus) : KTab{};
    const size_t max_tasks = P.max_tasks = M / 4 + nkeys + 1;          // bound for the smallest K (the table's entries are >= 4)
    if (!(M < ((size_t)1 << 31) && (tab_stride * (size_t)(precomp ? W : 1) + sh.batch_stride * k) < ((size_t)1 << 31))) {
        *why = "MSM too large for 31-bit entry indices";
        return 1;
    }
    P.bigcap = hot_list_cap(nkeys, max_tasks);
    P.slist_off = 2 + 2 * max_tasks;                        // (key, chunk) pairs of the extra chunks, then the split buckets' keys
    P.acc_blocks = wide ? (u32)(nkeys / 256) : (u32)((max_tasks + 255) / 256);      // wide: thread per bucket; else thread per task
    // dynamic LDS that leaves room for exactly wide_acc_blocks blocks on a CU, from the device's own LDS size (160 KB on gfx950), never more than one block
    // may ask for: where the request cannot hold the count down the kernel simply runs at its register-limited occupancy
    P.wide_acc_lds = (sh.lds_per_cu / (wide_acc_blocks + 1) + 1024) & ~(size_t)1023;
    if (P.wide_acc_lds > sh.lds_per_block) P.wide_acc_lds = sh.lds_per_block & ~(size_t)1023;
    if (wide) {                                                                         // bucket = (hi digit, lo digit)
        WideGeom& wg = P.wg;
        wg.nb = nb; wg.lo = (u32)c / 2; wg.hi = (u32)(c - 1) - wg.lo; wg.rlog = wide_rlog;
        // level two leaves k_wide_a2 sixteen run records per hi-digit marginal (c = 20: runs of 4 chunks, 16 + 8 records).  Runs of 8 halve k_wide_a2's work again,
        // but their seven additions in sequence made the synchronous MSM 8 us longer than it was with one level; runs of 4 leave it as it was (NOTES 7)
        wg.flog = wg.lo > wg.rlog + 5 ? wg.lo - wg.rlog - 4 : 1;
        P.wide_items = 2u * (nb >> wg.rlog) * (u32)ngroups;
        // (one-wave blocks: the 256 waves per MSM each carry a chain of 2^flog - 1 additions, and a wave alone on its SIMD runs it fastest)
        P.wide_runs = 2u * (nb >> (wg.rlog + wg.flog)) * (u32)ngroups;
    }
    // segment length of the weighted reduction: one bucket per thread (a 15-bit double-and-add each)
    // is the shortest chain, but its work grows with the bucket count -- for batches use running
    // sums over m buckets (2 additions per bucket + one double-and-add per segment), keeping about
    // one wave per SIMD busy
    u32 m = 1;
    while (m < 16 && (ngroups * (size_t)nb) / m > 65536) m <<= 1;
    if (!precomp && m < 4) m = 4;
    if (nb < m) m = nb;
    P.m = m;
    P.nseg = nb / m;
    P.nblk1 = (P.nseg + SUM_BLK - 1) / SUM_BLK;
    // one to four MSMs over the tables: digit marginals instead (k_marginals), three fields of <= 5 bits
    P.planes = wide ? 3u : ((precomp && ngroups <= 4096 && c >= 7 && c <= 16) ? 3u : 0u);
    if (P.planes) P.mg = marginal_geometry(wide ? P.wg.lo : (u32)c - 1);      // (wide: the tail runs over the two marginal groups of 2^lo slots each, k_wide_a2)
    P.tail_groups = wide ? 2 * ngroups : ngroups;
    P.nout = P.planes ? P.tail_groups * P.planes : ngroups;
    // small jobs over the tables: the whole sort in one launch (k_sort_fused)
    // (co-residency of the spinning blocks is what makes the grid barriers safe: 64 blocks x 4 jobs in flight need 128 CUs -- not in a partitioned mode)
    bool fused = precomp && !wide && !sh.fused_off && k <= 4 && M < ((size_t)1 << 22) && nb >= 2048 && sh.num_cus >= 128;
    if (fused) {
        FusedGeom& fg = P.fg;
        fg.n = (u32)n; fg.nb = nb; fg.W = (u32)W; fg.k = (u32)k; fg.bpg = (u32)std::min<size_t>(FUSED_G, FUSED_B / (2 * k)); fg.nkeys = (u32)nkeys;
        fg.split = 2; fg.sub = nb / fg.split;              // 64 blocks of 64 KB LDS: two per CU, so four (even eight) jobs in flight stay co-resident
        fg.room = P.room; fg.kmin = P.kmin; fg.ktab = P.ktab; fg.pt_stride = tab_stride; fg.pt_offset = sh.offset; fg.pt_batch = sh.batch_stride;
        const size_t threads = (size_t)fg.bpg * k * fg.split * FUSED_T;
        fg.kpt = (u32)((nkeys + 1 + threads - 1) / threads);
        const size_t tot4 = P.tot_e / 4, chunk4 = (tot4 + fg.bpg - 1) / fg.bpg + 1;
        if (fg.kpt > (u32)FUSED_KPT || n < 4 || P.tot_e % 4 || chunk4 > (size_t)FUSED_V * FUSED_T || fg.sub > (u32)FUSED_C * FUSED_T) { fused = false; fg = FusedGeom{}; }
    }
    // large jobs over the tables: the two-pass partitioned sort (k_part_*)
    const bool part = wide || (precomp && !fused && nb == ((u32)PART_P << PART_LOW) && n <= ((size_t)1 << 20) && W <= 16 && M >= ((size_t)1 << 21));
    P.sort = fused ? SORT_FUSED : (part ? SORT_PARTITIONED : SORT_PLAIN);
    P.part_low = wide ? (u32)c - 9 : (u32)PART_LOW;
    P.part_nblk = wide ? (u32)std::max<size_t>(std::max<size_t>(1, std::min<size_t>(256, 512 / k)), (P.tot_e + 65535) / 65536)
                       : (part ? (u32)std::max<size_t>(1, std::min<size_t>(256, 512 / k)) : 0);
    P.part_size = (size_t)k * PART_P * P.part_nblk;
    if (wide) {
        // staged scatter (round 6): stage_entries = entries per pass in LDS (0: the direct scatter); the dynamic LDS also holds the planning phase's lists
        P.part2_maxpass = std::min<u32>(PART2_MAXPASS, sh.stage_maxpass);
        // (clamped to the 128 KB the attribute asks for; an MSM whose partitions cannot make it in max_pass passes does not ask for the LDS at all)
        u32 stage_now = std::min<u32>(sh.stage_entries, (131072u - (1u << PART2_MAXLOW)) / 4u);
        if (stage_now <= 2048u || P.tot_e / PART_P > (size_t)P.part2_maxpass * (stage_now - 1024u)) stage_now = 0;
        const u32 stage_words = std::max<u32>(stage_now, 3u << PART2_MAXLOW);
        P.stage_now = stage_now;
        P.part2_lds = (size_t)stage_words * 4 + (stage_now ? ((size_t)1 << PART2_MAXLOW) : 0);
    }
    // the weighted tail is 3 x ngroups blocks however many MSMs there are: a pure latency chain (10 additions deep), so it takes the
    // lane-cooperative kernel for batches too (15 witness columns: 96 -> 35 us); it writes straight into the pinned host staging
    P.direct_out = wide || (P.planes && (P.few_groups || sh.fin_quad));
    // completion by flag (MsmSlot::done_flag): every such job ends in k_marginal_fin_q
    P.want_flag = !sh.flag_off && (wide || P.planes);
    return 0;
}

}  // namespace kh
