// opening.cpp -- point and fold helpers, challenge polynomials, the accumulator check, kh_ipa_verify_msm and the device-resident opening (kh_ipa_*).
#include <stdlib.h>
#include <algorithm>
#include <chrono>

#include "api_internal.hpp"
#include "env.hpp"

using namespace kh;

// KH_IPA_TIMING: the phase split of every opening on stderr
static bool ipa_timing() { static const bool v = env_flag("KH_IPA_TIMING", false); return v; }

struct EndoPair { uint64_t q[4], r[4]; };
static const EndoPair& cached_endos(int curve) {
    static EndoPair E[2]; static std::once_flag once[2];
    std::call_once(once[curve & 1], [curve] { curve_endos(curve & 1, E[curve & 1].q, E[curve & 1].r); });
    return E[curve & 1];
}

extern "C" {

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
    IpaWorkspace* ws = nullptr;           // the workspace this opening claimed on the handle (given back by kh_ipa_free)
    DevBuf *a = nullptr, *b = nullptr, *coef = nullptr;   // its ping-pong pairs
    DevBuf *sc = nullptr, *partial = nullptr;             // ws->sc / ws->partial
    unsigned extra = 0, uslot = 0;        // of the table set the rounds run over: slots behind the n points, and which U slot is this opening's (ipa.hip, k_ipa_step)
    int pp = 0;
    hipEvent_t ev = nullptr;              // orders the fold (library stream) before the next round's MSM (slot stream)
    bool lr_done = false;
    bool pending = false;                 // a recorded, not yet applied fold (kh_ipa_round_fold): the next round's step kernel applies it
    uint64_t u_p[4] = {0, 0, 0, 0}, ui_p[4] = {0, 0, 0, 0};
    size_t partial_words = 0;             // u64 words of `partial` before the step kernel's block counter
    std::vector<uint64_t> tab;            // U's window multiples staged for the asynchronous upload of kh_ipa_begin
    int sg_slot = -1;                     // pipeline slot holding the two half-sums of sg launched during the last round (kh_ipa_open), -1: none
    bool sg_want = false;                 // kh_ipa_open asks the last kh_ipa_round_lr to launch them
    bool spread_broken = false;           // a round's MSM disproved MSM_SPREAD_SCALARS (MsmJob::spread_rerun): the later rounds run without the hint
    bool rb_glv = false;                          // the folded basis's tables are GLV tables (half the doubling chain; MsmBasis::glv)
    void* round_tab = nullptr; int round_c = 0;   // table set the round MSMs run over (the SRS's own, or the rebased one)
    size_t tab_stride = 0;                        // points per window table of that set (the SRS's g_stride; N + 2 after the rebase: the folded basis, H, U)
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
    // the reference's SRS::open takes &self and is called from several threads on clones of one SRS (GpuSrs is Clone + Sync): every opening claims one of
    // the handle's KH_IPA_OPENINGS workspaces (its buffers, its U slot in the handle's tables) and runs beside the others; with all of them claimed a further
    // one waits for a kh_ipa_free; only the SAME thread beginning twice is a programming error.  The claim is the HANDLE's (its own lock: the callers may be
    // on different contexts) and is given back by kh_ipa_free -- or here, if beginning fails.
    IpaWorkspace* wsp = nullptr;
    {
        std::unique_lock<std::mutex> hl(srs->ipa_mu);
        const auto me = std::this_thread::get_id();
        bool others = false;
        for (auto& w : srs->ipa_ws) if (w && w->live) {
            KH_REQUIRE(w->owner != me, "another opening is in progress on this SRS in this thread (kh_ipa_free it first)");
            others = true;
        }
        auto find_free = [&]() -> int {                    // a workspace that exists before one that would have to be allocated
            for (int j = 0; j < KH_IPA_OPENINGS; j++) if (srs->ipa_ws[j] && !srs->ipa_ws[j]->live) return j;
            for (int j = 0; j < KH_IPA_OPENINGS; j++) if (!srs->ipa_ws[j]) return j;
            return -1;
        };
        int j = find_free();
        if (j < 0) {
            counter(CNT_IPA_WAITED)++;                     // (before the wait: a test can see a blocked begin)
            srs->ipa_cv.wait(hl, [&] { return (j = find_free()) >= 0; });
        } else if (others) counter(CNT_IPA_CONCURRENT)++;
        if (!srs->ipa_ws[j]) { srs->ipa_ws[j].reset(new IpaWorkspace); srs->ipa_ws[j]->index = j; }
        wsp = srs->ipa_ws[j].get();
        wsp->live = true; wsp->owner = me;
    }
    IpaWorkspace& ws = *wsp;
    struct Claim {
        kh_srs_t* s; IpaWorkspace* w; bool keep = false;
        ~Claim() { if (!keep) { { std::lock_guard<std::mutex> hl(s->ipa_mu); w->live = false; } s->ipa_cv.notify_all(); } }
    } claim{srs, wsp};
    Context& C = ctx();
    std::unique_lock<std::mutex> lk(C.mu);
    const auto b1_ = std::chrono::steady_clock::now();
    std::unique_ptr<kh_ipa> st(new kh_ipa);
    st->srs = srs; st->ws = wsp; st->curve = srs->curve; st->field = khost::scalar_field_id(srs->curve); st->n = n; st->cur = n;
    for (int i = 0; i < 2; i++) {
        if ((rc = ws.a[i].reserve(n * 32))) return rc;
        if ((rc = ws.b[i].reserve(n * 32))) return rc;
        if ((rc = ws.coef[i].reserve(n * 32))) return rc;
    }
    if ((rc = ws.sc.reserve(2 * srs->g_stride * 32))) return rc;       // two scalar vectors over the handle's tables: the points, H, every workspace's U
    if ((rc = ws.sg.reserve(2 * n * 32))) return rc;                   // scalars of the two halves of sg (kh_ipa_open)
    const size_t partial_bytes = 2 * (n / 512 + 1) * 32;               // block sums of the two inner products, then the last-block counter
    if ((rc = ws.partial.reserve(partial_bytes + 64))) return rc;
    KH_HIP(hipMemsetAsync((uint8_t*)ws.partial.p + partial_bytes, 0, 64, C.stream));
    // the scalars of the OTHER workspaces' U slots are zero: a zero digit makes no entry in the MSM's sort, so a slot another opening is rewriting is never
    // fetched.  The step kernel writes only H's and this opening's entries; the rest is zeroed here (a reused buffer may hold a rebased round's scalars).
    for (int side = 0; side < 2; side++)
        KH_HIP(hipMemsetAsync(ws.sc.as<uint8_t>() + ((size_t)side * srs->g_stride + n) * 32, 0, (srs->g_stride - n) * 32, C.stream));
    if (!ws.ev) KH_HIP(hipEventCreateWithFlags(&ws.ev, hipEventDisableTiming));
    st->a = ws.a; st->b = ws.b; st->coef = ws.coef; st->sc = &ws.sc; st->partial = &ws.partial; st->ev = ws.ev; st->partial_words = partial_bytes / 8;
    st->extra = (unsigned)(srs->g_stride - n); st->uslot = (unsigned)ws.index;
    // U into this workspace's slot of every window table of the SRS, H into its slot if it is not there yet (the rounds run over them until the rebase switches)
    const int rc_c = srs->g_precomp_c;                                             // window width of the rounds' tables
    void* const round_tab = srs->g.p;
    st->round_tab = round_tab; st->round_c = rc_c; st->tab_stride = srs->g_stride;
    memcpy(st->u_xy, u_base_xy, 64);
    // Plan the rebase (csrc/rebase.hip): the folded basis of N = 2^KH_IPA_REBASE_LOGN points (default 2^11; at least three rounds folded into it, at least 64
    // points) with window tables of KH_IPA_REBASE_C bits (default 13: 20 windows, 2^12 buckets), materialised from the c = 16 tables.  KH_IPA_REBASE=0: never.
    {
        static const bool rb_on = env_flag("KH_IPA_REBASE", true);
        static const unsigned rb_logn = (unsigned)env_int("KH_IPA_REBASE_LOGN", 11);     // 2^16 proof, opening: 5.39 (off) / 5.26 (2^9) / 5.17 (2^10) / 5.11 (2^11) / 5.34 (2^12) ms: profiles/r06_rebase_sweep.txt
        static const int rb_c = (int)std::min(16ll, std::max(7ll, env_int("KH_IPA_REBASE_C", 13)));     // 13: 20 windows, the top one still 8 bits wide (12, 14: a 3-bit top window = hot buckets)
        unsigned logn = 0; while (((size_t)1 << logn) < n) logn++;
        if (rb_on && srs->g_precomp_c == 16 && logn >= 9) {
            const unsigned ln = std::max(6u, std::min(rb_logn, logn - 3));
            const size_t N = (size_t)1 << ln, Q = n >> ln;
            // KH_IPA_REBASE_GLV (default on): tables for the lower 128 bits and phi of them; off when the generated constants' eigenvalue is not this curve's endo_r
            static const bool glv_env = env_flag("KH_IPA_REBASE_GLV", true);
            bool glv_ok = glv_env;
            if (glv_ok) {
                khost::Fld SFc(khost::scalar_field_id(srs->curve));
                khost::fe er; memcpy(&er, cached_endos(srs->curve).r, 32);
                const khost::fe can = SFc.from_mont(er);
                glv_ok = memcmp(can.l, msm_glv_lambda(khost::scalar_field_id(srs->curve)), 32) == 0;
            }
            st->rb_glv = glv_ok;
            const int W2 = std::max(windows_of(rb_c), 2 * ((128 + rb_c - 1) / rb_c));
            bool ok = ws.rb_tab.reserve((N + 2) * 64 * (size_t)W2) == KH_OK && ws.rb_B.reserve(rebase_bucket_bytes(N)) == KH_OK &&
                      ws.rb_part.reserve(rebase_part_bytes(N)) == KH_OK && ws.rb_lists.reserve(rebase_list_bytes(Q) + 256) == KH_OK &&       // (+ H | U, affine)
                      ws.rb_scratch.reserve((size_t)W2 * (N + 2) * 128) == KH_OK;
            if (ok && !ws.rb_stream) {
                int lo = 0, hi = 0;
                (void)hipDeviceGetStreamPriorityRange(&lo, &hi);                 // lo = the numerically largest = the LEAST urgent
                ok = hipStreamCreateWithPriority(&ws.rb_stream, hipStreamNonBlocking, lo) == hipSuccess &&
                     hipEventCreateWithFlags(&ws.rb_go, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&ws.rb_snap, hipEventDisableTiming) == hipSuccess &&
                     hipEventCreateWithFlags(&ws.rb_done, hipEventDisableTiming) == hipSuccess &&
                     hipHostMalloc((void**)&ws.rb_fail, 64, hipHostMallocCoherent | hipHostMallocMapped) == hipSuccess;
            }
            if (ok) { *ws.rb_fail = 0; st->rb_state = 1; st->rb_j0 = logn - ln; st->rb_N = N; st->rb_c = rb_c; }
            else { (void)hipGetLastError(); set_error(""); }                     // no memory for it: the rounds stay on the original tables
        }
    }
    const int W = rc_c ? windows_of(rc_c) : 1;
    std::vector<uint64_t>& tab = st->tab;                  // lives as long as the opening: no synchronisation before returning
    tab.resize((size_t)W * 8);
    hipStream_t s = C.stream;
    {
        // H is the SRS's: its window multiples are computed and written into slot n once per handle (and again after kh_srs_set_blinding_base, which no
        // live opening allows).  Openings of other contexts read the slot through streams of their own, so the one upload is complete before h_mu is let go.
        std::lock_guard<std::mutex> hk(srs->h_mu);
        std::vector<uint64_t>& hm = srs->h_multiples;
        if (hm.size() != (size_t)W * 8 || !srs->h_in_tables) {
            hm.resize((size_t)W * 8);
            host_window_multiples(srs->curve, srs->h, W, rc_c, hm.data());
            KH_HIP(hipMemcpy2DAsync((char*)round_tab + n * 64, srs->g_stride * 64, hm.data(), 64, 64, W, hipMemcpyHostToDevice, s));
            KH_HIP(hipStreamSynchronize(s));
            srs->h_in_tables = true;
        }
    }
    const auto b2_ = std::chrono::steady_clock::now();
    host_window_multiples(srs->curve, u_base_xy, W, rc_c, tab.data());
    const auto b3_ = std::chrono::steady_clock::now();
    KH_HIP(hipMemcpy2DAsync((char*)round_tab + (n + 1 + st->uslot) * 64, srs->g_stride * 64, tab.data(), 64, 64, W, hipMemcpyHostToDevice, s));
    if (a_len < n) KH_HIP(hipMemsetAsync((char*)st->a[0].p + a_len * 32, 0, (n - a_len) * 32, s));
    KH_HIP(hipMemcpyAsync(st->a[0].p, a, a_len * 32, kind, s));
    KH_HIP(hipMemcpyAsync(st->b[0].p, b, n * 32, kind, s));
    static const khost::fe ones[2] = {khost::field(0).one, khost::field(1).one};
    KH_HIP(hipMemcpyAsync(st->coef[0].p, &ones[st->field & 1], 32, hipMemcpyHostToDevice, s));
    if (kind != hipMemcpyDeviceToDevice) KH_HIP(hipStreamSynchronize(s));      // host inputs may be the caller's temporaries
    KH_HIP(hipEventRecord(st->ev, s));
    if (ipa_timing()) {
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
    if (ipa_sg_split(S.stream, st->field, st->coef[p].as<uint64_t>(), st->n, had_fold ? 1 : 0, st->u_p, st->ws->sg.as<uint64_t>())) return;
    MsmBasis bs; bs.pts = srs->g.p; bs.inf = nullptr; bs.n = srs->n; bs.stride = srs->g_stride; bs.precomp_c = srs->g_precomp_c;
    if (st->rb_state == 3) { bs.pts = st->round_tab; bs.n = st->n; bs.stride = st->tab_stride; bs.precomp_c = st->round_c; bs.glv = st->rb_glv; }     // sg = <coef_rel, g'>
    if (msm_enqueue(C, S, st->curve, bs, 0, st->ws->sg.as<uint64_t>(), st->n, 2, 1)) return;
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
    const bool prof = ipa_timing();
    const auto pt0 = std::chrono::steady_clock::now();
    auto us_since = [](std::chrono::steady_clock::time_point a) { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - a).count(); };
    Context& C = ctx();
    std::unique_lock<std::mutex> lk(C.mu);
    int si = acquire_slot(&lk, C, /*side_first=*/true);
    KH_REQUIRE(si >= 0, "%s", slot_error(si));
    MsmSlot& S = C.slot[si];
    KH_HIP(hipStreamWaitEvent(S.stream, st->ev, 0));
    kh_srs_t* const srs = st->srs;
    IpaWorkspace& ws = *st->ws;
    st->round_no++;
    // the rebase (csrc/rebase.hip): switch to the materialised folded basis as soon as its tables are complete
    if (st->rb_state == 2) {
        static const bool rb_wait = env_flag("KH_IPA_REBASE_WAIT", false);      // tests: the earliest possible switch, deterministically
        if (rb_wait) KH_HIP(hipEventSynchronize(ws.rb_done));
        const hipError_t qe = hipEventQuery(ws.rb_done);
        if (qe == hipSuccess) {
            if (__atomic_load_n(ws.rb_fail, __ATOMIC_ACQUIRE) != 0) { st->rb_state = -1; counter(CNT_REBASE_ABANDON)++; }
            else {
                KH_HIP(hipStreamWaitEvent(S.stream, ws.rb_done, 0));
                st->n = st->rb_N; st->ncoef >>= st->rb_j0;
                st->round_tab = ws.rb_tab.p; st->round_c = st->rb_c; st->tab_stride = st->rb_N + 2;
                st->extra = 2; st->uslot = 0;              // the rebased tables are this opening's own: the folded basis, H, U
                st->rb_state = 3; counter(CNT_REBASE_SWITCH)++;
                if (ipa_timing()) fprintf(stderr, "kh_ipa: round %u runs over the rebased tables (%zu points, c = %d, %u rounds folded in)\n", st->round_no, st->rb_N, st->rb_c, st->rb_j0);
            }
        } else if (qe != hipErrorNotReady) { KH_HIP(qe); }
        else (void)hipGetLastError();
        // the step kernel of round j0 + 3 is the first to overwrite the challenge tensor the plan kernel reads (ping-pong buffers): order it behind the plan
        if (st->rb_state == 2 && st->round_no == st->rb_j0 + 3) KH_HIP(hipStreamWaitEvent(S.stream, ws.rb_snap, 0));
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
                            st->sc->as<uint64_t>(), st->partial->as<uint64_t>(), (unsigned*)(st->partial->as<uint64_t>() + st->partial_words), st->extra, st->uslot);
    if (rc) return rc;
    const auto pt2 = std::chrono::steady_clock::now();
    if (st->pending) { st->pp = q; st->pending = false; }
    if (st->rb_state == 1 && st->round_no == st->rb_j0 + 1) {
        // this round's step kernel has just written the tensor of the first j0 challenges (2^j0 entries, st->coef[st->pp]): materialise the folded basis
        // and its window tables behind it on the side stream, H and U in the two extra slots
        const size_t N = st->rb_N, Q = (size_t)1 << st->rb_j0;
        hipStream_t rs = ws.rb_stream;
        bool ok = hipEventRecord(ws.rb_go, S.stream) == hipSuccess && hipStreamWaitEvent(rs, ws.rb_go, 0) == hipSuccess;
        uint32_t* const lists = ws.rb_lists.as<uint32_t>();
        if (ok) ok = rebase_points(rs, st->curve, st->coef[st->pp].as<uint64_t>(), Q, srs->g.p, srs->g_stride, N, ws.rb_B.p, ws.rb_part.p, lists,
                                   ws.rb_snap) == KH_OK;                   // (rb_snap: behind the plan kernel, the tensor's only reader)
        memcpy(st->hu_stage, srs->h, 64); memcpy(st->hu_stage + 8, st->u_xy, 64);       // (H | U travel in the table kernel's arguments: rebase.hip, RbExtra)
        if (ok) ok = rebase_tables(rs, st->curve, ws.rb_part.p, N, st->hu_stage, 2, st->rb_c, ws.rb_scratch.p, ws.rb_tab.p, ws.rb_fail,
                                   st->rb_glv ? cached_endos(st->curve).q : nullptr) == KH_OK;
        if (ok) ok = hipEventRecord(ws.rb_done, rs) == hipSuccess;
        if (ok) { st->rb_state = 2; counter(CNT_REBASE_LAUNCH)++; }
        else { (void)hipGetLastError(); (void)hipStreamSynchronize(rs); st->rb_state = -1; counter(CNT_REBASE_ABANDON)++; }
    }
    MsmBasis bs; bs.pts = st->round_tab; bs.inf = nullptr; bs.n = st->tab_stride; bs.stride = st->tab_stride; bs.precomp_c = st->round_c; bs.glv = st->rb_state == 3 && st->rb_glv;
    // The round's MSM is six launches (digits, one-launch sort, accumulation, bucket sums, two reduction kernels) which the host queues in ~25 us while
    // the step kernel runs.  Its scalars are products with Fiat-Shamir challenges (MSM_SPREAD_SCALARS) until a round of this opening proves otherwise.
    const int round_flags = (st->spread_broken ? 0 : MSM_SPREAD_SCALARS) | MSM_LATENCY;
    if ((rc = msm_enqueue(C, S, st->curve, bs, 0, st->sc->as<uint64_t>(), st->tab_stride, 2, 1, round_flags))) return rc;
    if (st->sg_want && st->cur == 2) { st->sg_want = false; ipa_sg_prelaunch_locked(st, C, p, had_fold); }
    const auto pt3 = std::chrono::steady_clock::now();
    if ((rc = wait_then_finish(lk, C, S, lr_xy, lr_inf))) return rc;
    if (S.job.spread_rerun) st->spread_broken = true;     // (the lock is held again: the slot's job is still this round's)
    if (prof) {
        IpaRoundProf& P = tl_round_prof;
        const double total_wait_finish = us_since(pt3);
        P.slot += std::chrono::duration<double, std::micro>(pt1 - pt0).count(); P.step += std::chrono::duration<double, std::micro>(pt2 - pt1).count();
        P.enqueue += std::chrono::duration<double, std::micro>(pt3 - pt2).count(); P.wait += last_wait_us(); P.finish += total_wait_finish - last_wait_us();
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
    IpaWorkspace* const ws = st->ws;
    if (ws && st->rb_state >= 2 && ws->rb_stream) (void)hipStreamSynchronize(ws->rb_stream);      // a materialisation that was never switched to: the workspace's next opening reuses its buffers
    delete st;
    if (srs && ws) {                                      // the workspace is free again: an opening waiting for one on this handle can start
        { std::lock_guard<std::mutex> hl(srs->ipa_mu); ws->live = false; }
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
    uint64_t u_last[4] = {0, 0, 0, 0}, chal_last[2] = {0, 0};
    for (size_t r = 0; r < rounds; r++) {
        const uint64_t* rl = blinders + 8 * r; const uint64_t* rr = rl + 4;
        const auto q0 = std::chrono::steady_clock::now();
        if (r + 1 == rounds) st->sg_want = true;
        if ((rc = kh_ipa_round_lr(st, rl, rr, lr_xy + 16 * r, lr_inf + 2 * r))) return rc;
        const auto q1 = std::chrono::steady_clock::now();
        if ((rc = kh_sponge_absorb_g(sponge, lr_xy + 16 * r, lr_inf + 2 * r, 2))) return rc;
        uint64_t chal[2], u[4], ui[4];
        if ((rc = kh_sponge_challenge(sponge, chal))) return rc;
        const auto q2 = std::chrono::steady_clock::now();
        if ((rc = kh_ipa_round_fold(st, chal, u, ui))) return rc;
        memcpy(u_last, u, 32); chal_last[0] = chal[0]; chal_last[1] = chal[1];
        if (ipa_timing()) {
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
    if (ipa_timing()) {
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

}  // extern "C"
