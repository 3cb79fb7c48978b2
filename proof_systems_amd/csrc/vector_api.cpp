// vector_api.cpp -- vector steps (kh_poly_*, kh_expr_*, kh_gate_*, kh_poseidon_*, scans, divisions), kh_ntt* / kh_lde* / kh_coset_ntt_dev and the host-pointer transforms.  (The gadget and wire steps, kh_*_witness_dev, are in witness_steps.cpp.)
#include <stdlib.h>

#include "api_internal.hpp"
#include "env.hpp"

using namespace kh;

namespace {
#include "poseidon_params.inc"      // the round constants kh_poseidon_gate_coefficients hands out (the host sponge and the device kernels have the same table)
}

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
void kh::xfer_trim(int d) {              // kh_trim: every pair that is not inside a call right now gives its memory back
    if (d < 0 || d >= KH_MAX_DEVICES) return;
    std::lock_guard<std::mutex> lk(g_xfer_mu);
    for (auto& q : xfer_registry(d)) if (!q->busy) { q->in.release(); q->out.release(); }
}

extern "C" {

// ---------------------------------------------------------------------------------- coefficient-vector operations around the opening
int kh_combine_polys_dev(int field, const uint64_t* const* polys_dev, const size_t* lens, const size_t* num_chunks, size_t m,
                         const uint64_t polyscale[4], size_t srs_length, uint64_t* out_dev, size_t* out_len) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    KH_REQUIRE(out_dev && polyscale && srs_length > 0 && (m == 0 || (polys_dev && lens && num_chunks)), "kh_combine_polys_dev: bad argument");
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
    const int rc = queue_step([&](Context& C) { return poly_lincomb(C, field, segs.data(), slen.data(), (const uint64_t*)scales.data(), segs.size(), out_dev, srs_length); });
    if (rc == KH_OK && out_len) *out_len = longest;
    return rc;
}
int kh_poly_lincomb_dev(int field, const uint64_t* const* polys_dev, const size_t* lens, const uint64_t* scalars, size_t m,
                        uint64_t* out_dev, size_t out_len) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    KH_REQUIRE((out_dev || out_len == 0) && (m == 0 || (polys_dev && lens && scalars)), "kh_poly_lincomb_dev: null argument");
    for (size_t i = 0; i < m; i++) KH_REQUIRE(lens[i] <= out_len, "polynomial %zu has %zu coefficients, the output %zu", i, lens[i], out_len);
    return queue_step([&](Context& C) { return poly_lincomb(C, field, polys_dev, lens, scalars, m, out_dev, out_len); });
}
int kh_b_init_dev(int field, const uint64_t* elm, size_t k, const uint64_t evalscale[4], size_t padded_len, uint64_t* out_dev) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    KH_REQUIRE(out_dev && evalscale && (elm || k == 0), "kh_b_init_dev: null argument");
    khost::Fld F(field);
    khost::fe es; memcpy(&es, evalscale, 32);
    std::vector<khost::fe> scales(k);
    khost::fe sc = F.f.one;
    for (size_t i = 0; i < k; i++) { scales[i] = sc; sc = F.mul(sc, es); }
    return queue_step([&](Context& C) { return poly_b_init(C, field, elm, (const uint64_t*)scales.data(), k, padded_len, out_dev); });
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
    return queue_step([&](Context& C) { return poly_div_vanishing(C, field, f_dev, len, n, q_dev, r_dev); });
}

int kh_field_scan_dev(int field, int op, int reverse, uint64_t* data_dev, size_t n) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    KH_REQUIRE((op == KH_SCAN_ADD || op == KH_SCAN_MUL) && (data_dev || n == 0), "kh_field_scan_dev: bad argument");
    return queue_step([&](Context& C) { return poly_scan(C, field, op, reverse ? 1 : 0, data_dev, n); });
}
int kh_batch_inversion_dev(int field, uint64_t* v_dev, size_t n) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    KH_REQUIRE(v_dev || n == 0, "null vector");
    return queue_step([&](Context& C) { return poly_batch_inversion(C, field, v_dev, n); });
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
    return queue_step([&](Context& C) { return poly_divide_by_linear(C, field, f_dev, len, a, q_dev, nullptr, rem_dev); });
}
int kh_check_equal_dev(const uint64_t* v_dev, size_t n, const uint64_t* expect, uint32_t* flags_dev, unsigned bit) {
    KH_REQUIRE((v_dev || n == 0) && flags_dev && bit < 32, "kh_check_equal_dev: bad argument");
    return queue_step([&](Context& C) { return poly_check_equal(C, v_dev, n, expect, flags_dev, bit); });
}
int kh_expr_evaluations_dev(int field, const uint32_t* tokens, size_t ntok, const uint64_t* const* cols_dev, const size_t* col_len, size_t ncols,
                            const uint64_t* constants, size_t nconsts, size_t rows, unsigned stride, unsigned next_shift, int accumulate,
                            uint64_t* out_dev) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    KH_REQUIRE(tokens && ntok > 0 && (out_dev || rows == 0) && stride > 0, "kh_expr_evaluations_dev: bad argument");
    KH_REQUIRE((ncols == 0 || (cols_dev && col_len)) && (nconsts == 0 || constants), "kh_expr_evaluations_dev: null table");
    return queue_step([&](Context& C) { return expr_run(C, field, tokens, ntok, cols_dev, col_len, ncols, constants, nconsts, rows, stride, next_shift, accumulate, out_dev); });
}

// The `sorted` step of the lookup argument on the device (kernels in lookup_sorted.hip).  The scratch block comes from the kh_dev_alloc pool (taken before the
// context's lock: the pool may order this context behind a block's previous owner); the one wait is the read-back of the status words, outside the lock.
int kh_lookup_sorted_dev(const uint64_t* table_dev, size_t lookup_rows, const uint64_t* values_dev, size_t value_stride, size_t max_per_row, uint64_t* out_dev,
                         size_t out_stride, size_t* bad_row) {
    KH_REQUIRE(table_dev && values_dev && out_dev && lookup_rows > 0 && max_per_row > 0 && value_stride >= lookup_rows && out_stride >= lookup_rows + 1,
               "kh_lookup_sorted_dev: bad argument");
    KH_REQUIRE((((uintptr_t)table_dev | (uintptr_t)values_dev | (uintptr_t)out_dev) & 15) == 0, "kh_lookup_sorted_dev: pointers must be 16-byte aligned");
    KH_REQUIRE(max_per_row < ((size_t)1 << 31) && lookup_rows < ((size_t)1 << 31) && (max_per_row + 1) * lookup_rows < ((size_t)1 << 31),
               "kh_lookup_sorted_dev: (max_per_row + 1) * lookup_rows = (%zu + 1) * %zu does not fit 31 bits", max_per_row, lookup_rows);
    int rc = ensure_init(); if (rc) return rc;
    if (bad_row) *bad_row = (size_t)-1;
    PoolBlock scratch;
    if ((rc = kh_dev_alloc(&scratch.p, lookup_sorted_scratch_words(lookup_rows) * sizeof(uint32_t)))) return rc;
    {
        Context& C = ctx();
        std::lock_guard<std::mutex> lk(C.mu);
        rc = lookup_sorted_run(C, table_dev, lookup_rows, values_dev, value_stride, max_per_row, out_dev, out_stride, scratch.as<uint32_t>());
        C.mark_async();
        if (rc) return rc;
    }
    uint32_t status[2] = {0, 0};
    if ((rc = kh_dev_download(status, scratch.as<uint32_t>() + lookup_sorted_status_offset(lookup_rows), sizeof(status)))) return rc;
    if (status[0] != 0xffffffffu) {                         // a looked-up value that is not in the table (constraints.rs:137-141)
        const size_t s = status[0] / lookup_rows, r = status[0] % lookup_rows;
        if (bad_row) *bad_row = r;
        set_error("lookup in row %zu (slot %zu): the value is not in the table", r, s);
        return KH_E_INVALID;
    }
    KH_REQUIRE(status[1] == (max_per_row + 1) * lookup_rows, "kh_lookup_sorted_dev: %u values for %zu places", status[1], (max_per_row + 1) * lookup_rows);
    counter(CNT_LOOKUP_SORTED_DEV)++;
    return KH_OK;
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
    return queue_step([&](Context& C) { return gate_run(C, field, gate, cols_dev, col_len, constants, nconsts, rows, stride, next_shift, accumulate, out_dev); });
}

// ---------------------------------------------------------------------------------- Poseidon on the device (kernels in poseidon.hip)
int kh_poseidon_gate_coefficients(int field, uint64_t* out) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    KH_REQUIRE(out, "kh_poseidon_gate_coefficients: null output");
    const khost::fe (*rc)[3] = field == KH_FIELD_FP ? POSEIDON_RC_FP : POSEIDON_RC_FQ;
    for (size_t r = 0; r < 11; r++)
        for (size_t c = 0; c < 15; c++) memcpy(out + 4 * (15 * r + c), &rc[5 * r + c / 3][c % 3], 32);
    return KH_OK;
}
#define KH_POSEIDON_ALIGNED(p) ((((uintptr_t)(p)) & 15) == 0)
int kh_poseidon_permute_dev(int field, uint64_t* states_dev, size_t n) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    KH_REQUIRE(states_dev || n == 0, "kh_poseidon_permute_dev: null states");
    KH_REQUIRE(KH_POSEIDON_ALIGNED(states_dev), "kh_poseidon_permute_dev: states_dev must be 16-byte aligned");
    KH_REQUIRE(n <= WAVE_BLOCK_MAX_N, "kh_poseidon_permute_dev: %zu states are more than the %zu one call takes", n, WAVE_BLOCK_MAX_N);
    if (n == 0) return ensure_init();
    return queue_step([&](Context& C) { return poseidon_permute(C, field, states_dev, n); });
}
int kh_poseidon_hash_dev(int field, const uint64_t* msgs_dev, size_t msg_len, size_t n, const uint64_t* init, uint64_t* digests_dev) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    KH_REQUIRE(n == 0 || (digests_dev && (msgs_dev || msg_len == 0)), "kh_poseidon_hash_dev: null %s", digests_dev ? "messages" : "digests");
    KH_REQUIRE(KH_POSEIDON_ALIGNED(msgs_dev) && KH_POSEIDON_ALIGNED(digests_dev), "kh_poseidon_hash_dev: msgs_dev and digests_dev must be 16-byte aligned");
    KH_REQUIRE(n <= WAVE_BLOCK_MAX_N && (msg_len == 0 || n <= (SIZE_MAX / 32) / msg_len),
               "kh_poseidon_hash_dev: %zu messages of %zu elements overflow the byte count", n, msg_len);
    if (n == 0) return ensure_init();
    return queue_step([&](Context& C) { return poseidon_hash(C, field, msgs_dev, msg_len, n, init, digests_dev); });
}
#undef KH_POSEIDON_ALIGNED
int kh_poseidon_set_split_max_n(size_t n) { poseidon_set_split_max_n(n); return KH_OK; }

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
    if (batch == 0) return ensure_init();
    return queue_step([&](Context& C) { return ntt_run(C, field, data_dev, log2_n, inverse, batch); });
}
int kh_lde_dev(int field, const uint64_t* coeffs_dev, unsigned log2_n, unsigned log2_blowup, uint64_t* out_dev, size_t batch) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    KH_REQUIRE(log2_n + log2_blowup <= 28, "log2 size %u too large", log2_n + log2_blowup);
    KH_REQUIRE((coeffs_dev && out_dev) || batch == 0, "null data");
    if (batch == 0) return ensure_init();
    return queue_step([&](Context& C) { return lde_run(C, field, coeffs_dev, log2_n, log2_blowup, out_dev, batch); });
}
int kh_coset_ntt_dev(int field, const uint64_t* coeffs_dev, unsigned log2_n, const uint64_t shift[4], uint64_t* out_dev, size_t batch) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    KH_REQUIRE(log2_n <= 28 && shift, "kh_coset_ntt_dev: bad argument");
    KH_REQUIRE((coeffs_dev && out_dev) || batch == 0, "null data");
    if (batch == 0) return ensure_init();
    return queue_step([&](Context& C) { return poly_coset_ntt(C, field, coeffs_dev, log2_n, shift, out_dev, batch); });
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
    static const size_t v = (size_t)env_int("KH_XFER_KEEP_MB", 64) << 20;   // a time (2 MB in, 16 MB out at 2^16 -> 2^19) and a
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

}  // extern "C"

namespace kh {
// the column pass of kh_prover_index_create (csrc/prover.cpp; kernel in poly.hip): queued on the main stream like kh_ntt_dev
int index_columns_dev(int field, const uint8_t* selcol_dev, const uint32_t* wires_dev, const uint64_t* coeffs_dev, size_t n_gates, size_t n,
                      size_t zk_rows, const uint64_t* shifts, size_t ncol, uint64_t* d1_dev) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    KH_REQUIRE(d1_dev && shifts && (n_gates == 0 || (selcol_dev && wires_dev && coeffs_dev)), "index_columns_dev: null argument");
    return queue_step([&](Context& C) { return poly_index_columns(C, field, selcol_dev, wires_dev, coeffs_dev, n_gates, n, zk_rows, shifts, ncol, d1_dev); });
}
// the lookup passes of kh_prover_index_create_lookup (kernels in lookup_index.hip), queued on the main stream
int lookup_selectors_dev(int field, const uint8_t* code_dev, size_t n_gates, size_t n, const int* patterns, size_t npat, uint64_t* out_dev) {
    KH_REQUIRE(code_dev && patterns && out_dev, "lookup_selectors_dev: null argument");
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    return queue_step([&](Context& C) { return lookup_selector_columns(C, field, code_dev, n_gates, n, patterns, npat, out_dev); });
}
int lookup_tables_dev(int field, const uint64_t* segs_dev, const uint64_t* seg_starts, size_t nseg, const uint64_t* data_dev, size_t n, size_t width, uint64_t* tcols_dev,
                      uint64_t* ids_dev, uint64_t* rtsel_dev, size_t rt_offset, size_t rt_len, size_t zk_rows) {
    KH_REQUIRE(segs_dev && seg_starts && tcols_dev, "lookup_tables_dev: null argument");
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    return queue_step([&](Context& C) { return lookup_table_columns(C, field, segs_dev, seg_starts, nseg, data_dev, n, width, tcols_dev, ids_dev, rtsel_dev, rt_offset, rt_len, zk_rows); });
}
int lookup_atom_denominators_dev(int field, const uint64_t* x8_dev, size_t n, size_t zk_rows, const uint64_t a[4], const uint64_t omega[4], uint64_t* atoms_dev) {
    KH_REQUIRE(x8_dev && a && omega && atoms_dev, "lookup_atom_denominators_dev: null argument");
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    return queue_step([&](Context& C) { return lookup_atom_denominators(C, field, x8_dev, n, zk_rows, a, omega, atoms_dev); });
}
int lookup_atom_finish_dev(int field, size_t n, size_t zk_rows, const uint64_t zh8[32], const uint64_t lim0[4], const uint64_t limf[4], uint64_t* atoms_dev) {
    KH_REQUIRE(zh8 && lim0 && limf && atoms_dev, "lookup_atom_finish_dev: null argument");
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "unknown field id %d", field);
    return queue_step([&](Context& C) { return lookup_atom_finish(C, field, n, zk_rows, zh8, lim0, limf, atoms_dev); });
}
// the gate part of the constant term of a batch of proofs (csrc/verifier.cpp; kernels in gates.hip), queued on the main stream
int verifier_gate_terms_dev(int field, const uint64_t* cols_host, size_t ncols, size_t items, const GateBatchLaunch* launches, size_t nl, uint64_t* out_dev,
                            const uint64_t** cols_dev) {
    return queue_step([&](Context& C) { return gate_batch_run(C, field, cols_host, ncols, items, launches, nl, out_dev, cols_dev); });
}
// the kernels of kh_witness_check (csrc/prover.cpp; witness_check.hip).  The scratch block comes from the kh_dev_alloc pool, taken before the context's lock like
// kh_lookup_sorted_dev's; the read-back of the four status words, outside the lock, is the call's only wait.  lookups: what to check of them, or NULL.
int witness_check_dev(int field, const uint64_t* witness_dev, const uint64_t* d1_dev, size_t n, const int* sel_col, size_t ngate_ids, size_t public_inputs,
                      const uint64_t endo[4], const uint32_t* wires_dev, size_t n_gates, const WitnessLookups* lookups, uint64_t status[4]) {
    KH_REQUIRE(status, "witness_check_dev: null argument");
    int rc = ensure_init(); if (rc) return rc;
    PoolBlock scratch;
    if ((rc = kh_dev_alloc(&scratch.p, witness_check_scratch_bytes() + (lookups ? witness_check_lookup_scratch_bytes(lookups->L, lookups->W, lookups->rt_len) : 0)))) return rc;
    {
        Context& C = ctx();
        std::lock_guard<std::mutex> lk(C.mu);
        rc = witness_check_run(C, field, witness_dev, d1_dev, n, sel_col, ngate_ids, public_inputs, endo, wires_dev, n_gates, lookups, scratch.p);
        C.mark_async();
        if (rc) return rc;
    }
    return kh_dev_download(status, scratch.p, 4 * sizeof(uint64_t));
}
}  // namespace kh
