// srs.cpp -- SRS handles: creation, window tables, Lagrange bases, the blinding base and kh_mask_custom.
#include <stdlib.h>

#include "api_internal.hpp"
#include "srs_file.hpp"

using namespace kh;

int kh::resolve_basis(kh_srs_t* srs, int basis, unsigned chunk, MsmBasis& out) {
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

// XYZZ -> affine for a list of points with ONE field inversion (Montgomery's trick over the ZZZ's)
void kh::xyzz_to_affine_batch(const khost::Crv& crv, const std::vector<khost::xyzz>& acc, uint64_t* out_xy, uint8_t* out_inf) {
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

// the wide-window table set of a big basis (table 0 = a copy of the basis; the slots of H and U unused).  It is a throughput optimisation on top of the narrow tables
// (+13/16 of their memory: 832 MiB at 2^20 points, 3.3 GiB at 2^22), so a handle whose second set does not fit is still a working handle: `required` = false
// gives the memory back, clears the error and leaves the narrow tables to serve every MSM.
static int build_wide_tables(Context& C, kh_srs* s, bool required) {
    if (s->g_wide_c) return KH_OK;
    if (!s->g_precomp_c || (!required && s->n < msm_wide_min_n())) return KH_OK;
    int rc = s->g_wide.reserve(s->g_stride * 64 * (size_t)windows_of(MSM_WIDE_C));
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
// The narrow window tables of a point buffer of `stride` points per table (the basis of n points and, for an SRS, the slots of H and U).
// table_width: the window width a basis of n points gets; 0 = none, smaller bases keep the plain per-window path.  table_bytes: what the buffer must
// hold before its table 0 is filled.
static int table_width(size_t n) { return n >= MSM_PRECOMP_MIN_N ? MSM_PRECOMP_C : 0; }
static size_t table_bytes(size_t n, size_t stride) { return stride * 64 * (table_width(n) ? windows_of(table_width(n)) : 1); }
// builds them in place on C.stream, behind table 0; *c_built = the window width built (0 for none)
static int build_tables(Context& C, int curve, void* tables, const uint8_t* inf, size_t n, size_t stride, int* c_built) {
    const int c = table_width(n);
    if (c) { int rc = msm_precompute(C, curve, tables, inf, stride, c); if (rc) return rc; }
    *c_built = c;
    return KH_OK;
}
// kh_srs_create / kh_srs_create_device_range: `fill` brings the first n points into table 0 (complete, or queued on C.stream)
template <class Fill>
static int srs_create(int curve, size_t n, kh_srs_t** out, Fill fill) {
    int rc = ensure_init(); if (rc) return rc;
    std::unique_ptr<kh_srs> s(new kh_srs);
    s->curve = curve; s->n = n;
    Context& C = ctx();
    s->device = C.device;
    std::lock_guard<std::mutex> lk(C.mu);
    s->g_stride = n + 1 + KH_IPA_OPENINGS;              // behind the basis: H, then one slot of U per opening workspace (kh_ipa_begin)
    if ((rc = s->g.reserve(table_bytes(n, s->g_stride)))) return rc;
    if ((rc = fill(C, s->g.p))) return rc;
    for (size_t i = n; i < s->g_stride; i++)            // placeholders: valid points
        KH_HIP(hipMemcpyAsync((char*)s->g.p + i * 64, s->g.p, 64, hipMemcpyDeviceToDevice, C.stream));
    if ((rc = build_tables(C, curve, s->g.p, nullptr, n, s->g_stride, &s->g_precomp_c))) return rc;
    if ((rc = build_wide_tables(C, s.get(), false))) return rc;
    // tables are per HANDLE, streams per context: another context (kh_private_context_begin on another thread) may use the handle at once, so it is
    // handed out complete (a one-time cost)
    KH_HIP(hipStreamSynchronize(C.stream));
    if ((rc = kh_srs_h(curve, s->h))) return rc;
    *out = s.release();
    return KH_OK;
}

extern "C" {

int kh_srs_has_wide_tables(const kh_srs_t* srs) { return srs && srs->g_wide_c ? 1 : 0; }
int kh_srs_set_wide_tables(kh_srs_t* srs, int on) {
    KH_ON_DEVICE_OF(srs);
    KH_REQUIRE(srs != nullptr, "null SRS handle");
    int rc = ensure_init(); if (rc) return rc;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    if (on) {
        KH_REQUIRE(srs->g_precomp_c, "kh_srs_set_wide_tables: the handle has no window tables (fewer than %d points)", (int)MSM_PRECOMP_MIN_N);
        // another context may resolve the handle's basis at any time (msm_api.cpp: resolve_counted, under wide_mu): the set is built aside and published --
        // g_wide_c -- only when it is complete on the device
        std::lock_guard<std::mutex> wl(srs->wide_mu);
        if (srs->g_wide_c) return KH_OK;
        if ((rc = build_wide_tables(C, srs, true))) return rc;
        const int built = srs->g_wide_c;
        srs->g_wide_c = 0;
        const hipError_t e = hipStreamSynchronize(C.stream);
        if (e != hipSuccess) { srs->g_wide.release(); KH_HIP(e); }
        srs->g_wide_c = built;
        return KH_OK;
    }
    // the handle is shared between contexts: what counts is the handle's own tally of jobs in flight (kh_srs::jobs), not the calling context's slots.  A job
    // that was counted has finished on the device by the time it is counted out (wait_then_finish waited for its event), so nothing is left to wait for --
    // except a job whose wait itself failed (a device error: it is counted out without having been seen to end; every later call on that device fails too).
    std::lock_guard<std::mutex> wl(srs->wide_mu);
    KH_REQUIRE(srs->jobs->load() == 0, "kh_srs_set_wide_tables: an MSM is in flight (kh_msm_wait first)");
    srs->g_wide_c = 0;
    srs->g_wide.release();
    return KH_OK;
}
int kh_srs_create(int curve, const uint64_t* g_xy, size_t n, kh_srs_t** out) {
    KH_REQUIRE(out && g_xy && n > 0, "kh_srs_create: null argument or n == 0");
    KH_REQUIRE(curve == KH_CURVE_VESTA || curve == KH_CURVE_PALLAS, "unknown curve id %d", curve);
    return srs_create(curve, n, out, [&](Context&, void* g) -> int { KH_HIP(hipMemcpy(g, g_xy, n * 64, hipMemcpyHostToDevice)); return KH_OK; });
}
int kh_srs_create_device(int curve, size_t depth, kh_srs_t** out) { return kh_srs_create_device_range(curve, 0, depth, out); }
int kh_srs_create_device_range(int curve, size_t start, size_t depth, kh_srs_t** out) {
    KH_REQUIRE(out && depth > 0, "kh_srs_create_device: null argument or depth == 0");
    KH_REQUIRE(curve == KH_CURVE_VESTA || curve == KH_CURVE_PALLAS, "unknown curve id %d", curve);
    KH_REQUIRE(start + depth <= ((size_t)1 << 32), "SRS index must fit u32 (ipa.rs:758)");
    return srs_create(curve, depth, out, [&](Context& C, void* g) { return srs_generate_device(C, curve, start, depth, g); });
}
// n records of g and (nullable) the record of h, decoded by ONE launch straight into table 0: h lands in the slot behind the basis, which is H's own
// and holds a placeholder until the first opening, and is read back from there
int kh_srs_create_compressed(int curve, const uint8_t* g_bytes, size_t n, const uint8_t* h_bytes, kh_srs_t** out) {
    KH_REQUIRE(out && g_bytes && n > 0, "kh_srs_create_compressed: null argument or n == 0");
    KH_REQUIRE(curve == KH_CURVE_VESTA || curve == KH_CURVE_PALLAS, "unknown curve id %d", curve);
    KH_REQUIRE(n < ((size_t)1 << 32), "kh_srs_create_compressed: %zu records, the limit is 2^32 - 1", n);
    const size_t m = n + (h_bytes ? 1 : 0);
    uint64_t h_xy[8];
    kh_srs_t* srs = nullptr;
    int rc = srs_create(curve, n, &srs, [&](Context& C, void* g) -> int {
        DevBuf &rec = C.scratch("point_codec_bytes"), &inf = C.scratch("point_codec_inf"), &st = C.scratch("point_codec_status");
        int r;
        if ((r = rec.reserve(m * KH_POINT_BYTES)) || (r = inf.reserve(m)) || (r = st.reserve(m))) return r;
        KH_HIP(hipMemcpyAsync(rec.p, g_bytes, n * KH_POINT_BYTES, hipMemcpyHostToDevice, C.stream));
        if (h_bytes) KH_HIP(hipMemcpyAsync(rec.as<uint8_t>() + n * KH_POINT_BYTES, h_bytes, KH_POINT_BYTES, hipMemcpyHostToDevice, C.stream));
        if ((r = points_decompress_launch(C, curve, rec.as<uint8_t>(), m, (uint64_t*)g, inf.as<uint8_t>(), st.as<uint8_t>(), nullptr, 0))) return r;
        std::vector<uint8_t> status(m);
        KH_HIP(hipMemcpyAsync(status.data(), st.p, m, hipMemcpyDeviceToHost, C.stream));
        if (h_bytes) KH_HIP(hipMemcpyAsync(h_xy, (const char*)g + n * 64, 64, hipMemcpyDeviceToHost, C.stream));
        KH_HIP(hipStreamSynchronize(C.stream));
        for (size_t i = 0; i < m; i++) {
            if (status[i] == KH_POINT_OK) continue;
            if (i < n) set_error("kh_srs_create_compressed: record %zu is %s: a basis point must be a point", i, point_status_name(status[i]));
            else set_error("kh_srs_create_compressed: the record of the blinding base is %s", point_status_name(status[i]));
            return KH_E_INVALID;
        }
        return KH_OK;
    });
    if (rc) return rc;
    if (h_bytes && (rc = kh_srs_set_blinding_base(srs, h_xy))) { kh_srs_free(srs); return rc; }
    *out = srs;
    return KH_OK;
}
int kh_srs_get_g_compressed(kh_srs_t* srs, size_t offset, size_t count, uint8_t* out) {
    KH_ON_DEVICE_OF(srs);
    KH_REQUIRE(srs && (out || count == 0), "kh_srs_get_g_compressed: null argument");
    KH_REQUIRE(offset <= srs->n && count <= srs->n - offset, "range [%zu, %zu) beyond the SRS size %zu", offset, offset + count, srs->n);
    if (count == 0) return KH_OK;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    DevBuf& rec = C.scratch("point_codec_bytes");
    int rc = rec.reserve(count * KH_POINT_BYTES); if (rc) return rc;
    if ((rc = points_compress_launch(C, srs->curve, (const uint64_t*)((const char*)srs->g.p + offset * 64), nullptr, count, rec.as<uint8_t>()))) return rc;
    KH_HIP(hipMemcpyAsync(out, rec.p, count * KH_POINT_BYTES, hipMemcpyDeviceToHost, C.stream));
    KH_HIP(hipStreamSynchronize(C.stream));
    return KH_OK;
}
size_t kh_srs_file_bytes(size_t n) { return kh_srs_file::file_bytes(n); }
int kh_srs_write_file(kh_srs_t* srs, uint8_t* out, size_t cap) {
    KH_REQUIRE(srs && out, "kh_srs_write_file: null argument");
    const size_t want = kh_srs_file::file_bytes(srs->n);
    KH_REQUIRE(want && cap >= want, "kh_srs_write_file: %zu points need %zu bytes, the buffer has %zu", srs->n, want, cap);
    std::vector<uint8_t> records(srs->n * KH_POINT_BYTES);
    uint8_t h_record[KH_POINT_BYTES];
    uint64_t h_xy[8] __attribute__((aligned(16)));
    int rc = kh_srs_get_g_compressed(srs, 0, srs->n, records.data()); if (rc) return rc;
    if ((rc = kh_srs_get_blinding_base(srs, h_xy))) return rc;
    {
        KH_ON_DEVICE_OF(srs);
        if ((rc = kh_points_compress(srs->curve, h_xy, nullptr, 1, h_record))) return rc;
    }
    char err[192];
    if (kh_srs_file::write(records.data(), srs->n, h_record, out, cap, err, sizeof err)) { set_error("kh_srs_write_file: %s", err); return KH_E_INVALID; }
    return KH_OK;
}
int kh_srs_create_from_file(int curve, const uint8_t* file, size_t len, size_t limit, kh_srs_t** out) {
    KH_REQUIRE(out && file, "kh_srs_create_from_file: null argument");
    KH_REQUIRE(curve == KH_CURVE_VESTA || curve == KH_CURVE_PALLAS, "unknown curve id %d", curve);
    kh_srs_file::View v;
    char err[192];
    if (kh_srs_file::parse(file, len, &v, err, sizeof err)) { set_error("kh_srs_create_from_file: %s", err); return KH_E_INVALID; }
    const size_t n = limit && limit < v.count ? limit : v.count;
    KH_REQUIRE(n > 0, "kh_srs_create_from_file: the file holds no point");
    std::vector<uint8_t> records(n * KH_POINT_BYTES);                        // the items without their markers
    for (size_t i = 0; i < n; i++) memcpy(records.data() + i * KH_POINT_BYTES, v.record(i), KH_POINT_BYTES);
    return kh_srs_create_compressed(curve, records.data(), n, v.record(v.count), out);
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
int kh_srs_device(const kh_srs_t* srs) { return srs ? srs->device : -1; }

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
    if ((rc = L->pts.reserve(table_bytes(n, n)))) return rc;
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
    if ((rc = build_tables(C, srs->curve, L->pts.p, L->has_inf ? L->inf.as<uint8_t>() : nullptr, n, n, &L->precomp_c))) return rc;
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
    for (unsigned c = 0; c < num_chunks; c++) {
        std::unique_ptr<LagrangeChunk> L(new LagrangeChunk);
        L->n = n;
        if ((rc = L->pts.reserve(table_bytes(n, n)))) return rc;
        if ((rc = L->inf.reserve(n))) return rc;
        if ((rc = lagrange_run(C, srs->curve, srs->g.p, srs->n, log2_domain, c, L->pts.p, L->inf.as<uint8_t>()))) return rc;
        std::vector<uint8_t> hinf(n);
        KH_HIP(hipMemcpy(hinf.data(), L->inf.p, n, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; i++) if (hinf[i]) { L->has_inf = true; break; }
        if ((rc = build_tables(C, srs->curve, L->pts.p, L->has_inf ? L->inf.as<uint8_t>() : nullptr, n, n, &L->precomp_c))) return rc;
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

int kh_srs_set_blinding_base(kh_srs_t* srs, const uint64_t h_xy[8]) {
    KH_REQUIRE(srs && h_xy, "null argument");
    // the rounds of a live opening read H from the handle's tables: no opening may be live, and none may begin before the new H is in place (ipa_mu is held
    // throughout; kh_ipa_begin takes h_mu only after it has let go of ipa_mu)
    std::lock_guard<std::mutex> il(srs->ipa_mu);
    for (auto& w : srs->ipa_ws)
        KH_REQUIRE(!(w && w->live), "kh_srs_set_blinding_base: an opening is in progress on this SRS (kh_ipa_free it first)");
    std::lock_guard<std::mutex> lk(srs->h_mu);
    memcpy(srs->h, h_xy, 64);
    srs->h_table.clear(); srs->h_multiples.clear(); srs->h_in_tables = false;      // the next opening writes the new H into the tables
    return KH_OK;
}
int kh_srs_get_blinding_base(const kh_srs_t* srs, uint64_t h_xy[8]) {
    KH_REQUIRE(srs && h_xy, "null argument");
    memcpy(h_xy, srs->h, 64);
    return KH_OK;
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

}  // extern "C"
