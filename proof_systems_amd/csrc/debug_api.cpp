// debug_api.cpp -- test hooks (kh_debug_*).
#include "api_internal.hpp"

using namespace kh;

extern "C" {

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
int kh_debug_field29_op(int field, int op, int spread, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out, size_t n) {
    KH_REQUIRE(a && c && out && (op == 1 || b), "null argument");
    KH_REQUIRE((op == 0 || op == 1) && spread >= 0 && spread <= 2, "kh_debug_field29_op: op %d / spread %d unknown", op, spread);
    int rc = ensure_init(); if (rc) return rc;
    if (n == 0) return KH_OK;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    DevBuf da, db, dc, dout;
    if ((rc = da.reserve(n * 36)) || (rc = db.reserve(n * 36)) || (rc = dc.reserve(n * 36)) || (rc = dout.reserve(n * 36))) return rc;
    KH_HIP(hipMemcpyAsync(da.p, a, n * 36, hipMemcpyHostToDevice, C.stream));
    if (op == 0) KH_HIP(hipMemcpyAsync(db.p, b, n * 36, hipMemcpyHostToDevice, C.stream));
    KH_HIP(hipMemcpyAsync(dc.p, c, n * 36, hipMemcpyHostToDevice, C.stream));
    if ((rc = debug_field29_op(C, field, op, spread, da.as<uint32_t>(), db.as<uint32_t>(), dc.as<uint32_t>(), dout.as<uint32_t>(), n))) return rc;
    KH_HIP(hipMemcpyAsync(out, dout.p, n * 36, hipMemcpyDeviceToHost, C.stream));
    KH_HIP(hipStreamSynchronize(C.stream));
    return KH_OK;
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
// n XYZZ records of the device -> affine points and infinity bytes, after everything queued on the context stream
static int download_points(Context& C, int curve, const DevBuf& dev, size_t n, uint64_t* out_xy, uint8_t* out_inf) {
    std::vector<khost::xyzz> res(n);
    KH_HIP(hipMemcpyAsync(res.data(), dev.p, n * 128, hipMemcpyDeviceToHost, C.stream));
    KH_HIP(hipStreamSynchronize(C.stream));
    khost::Crv crv(curve);
    for (size_t i = 0; i < n; i++) {
        khost::aff a; const bool inf = crv.to_affine(res[i], a);
        memcpy(out_xy + 8 * i, &a, 64); out_inf[i] = inf ? 1 : 0;
    }
    return KH_OK;
}
int kh_debug_bucket_tail(int curve, int tail, int fin, unsigned c_or_nb, unsigned m, size_t groups, const uint64_t* buckets, uint64_t* out_xy, uint8_t* out_inf) {
    KH_REQUIRE(curve == KH_CURVE_VESTA || curve == KH_CURVE_PALLAS, "unknown curve id %d", curve);
    KH_REQUIRE(buckets && out_xy && out_inf, "kh_debug_bucket_tail: null argument");
    size_t nin = 0, nseg = 0, nout = 0;
    int rc = debug_bucket_tail_sizes(tail, fin, c_or_nb, m, groups, &nin, &nseg, &nout); if (rc) return rc;
    if ((rc = ensure_init())) return rc;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    DevBuf din, dseg, dout;
    if ((rc = din.reserve(nin * 128)) || (rc = dseg.reserve(nseg * 128)) || (rc = dout.reserve(nout * 128))) return rc;
    KH_HIP(hipMemcpyAsync(din.p, buckets, nin * 128, hipMemcpyHostToDevice, C.stream));
    if ((rc = debug_bucket_tail(C, curve, tail, fin, c_or_nb, m, groups, din.as<uint8_t>(), dseg.as<uint8_t>(), dout.as<uint8_t>()))) return rc;
    return download_points(C, curve, dout, nout, out_xy, out_inf);
}
int kh_debug_bucket_sums(int curve, int kind, size_t nkeys, const uint32_t* toff, const uint64_t* partial, uint64_t* out_xy, uint8_t* out_inf) {
    KH_REQUIRE(curve == KH_CURVE_VESTA || curve == KH_CURVE_PALLAS, "unknown curve id %d", curve);
    KH_REQUIRE(toff && out_xy && out_inf, "kh_debug_bucket_sums: null argument");
    KH_REQUIRE(kind >= 0 && kind <= 2, "kh_debug_bucket_sums: kind %d unknown", kind);
    KH_REQUIRE(nkeys >= 1 && nkeys <= ((size_t)1 << 24), "kh_debug_bucket_sums: %zu buckets (1 .. 2^24)", nkeys);
    KH_REQUIRE(toff[0] == 0, "kh_debug_bucket_sums: toff[0] = %u, the first list starts at 0", toff[0]);
    for (size_t i = 0; i < nkeys; i++) KH_REQUIRE(toff[i] <= toff[i + 1], "kh_debug_bucket_sums: toff[%zu] = %u > toff[%zu] = %u", i, toff[i], i + 1, toff[i + 1]);
    const size_t ntasks = toff[nkeys];
    KH_REQUIRE(ntasks < ((size_t)1 << 24) && (ntasks == 0 || partial), "kh_debug_bucket_sums: %zu partials (below 2^24, and not NULL)", ntasks);
    int rc = ensure_init(); if (rc) return rc;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    const size_t cap = debug_bucket_sums_cap(nkeys, ntasks);
    DevBuf dtoff, dpart, dbuckets, dbig, dchunks;
    if ((rc = dtoff.reserve((nkeys + 1) * 4)) || (rc = dpart.reserve(std::max<size_t>(ntasks, 1) * 128)) || (rc = dbuckets.reserve(nkeys * 128)) ||
        (rc = dbig.reserve((2 + 4 * cap) * 4)) || (rc = dchunks.reserve(cap * 128))) return rc;
    KH_HIP(hipMemcpyAsync(dtoff.p, toff, (nkeys + 1) * 4, hipMemcpyHostToDevice, C.stream));
    if (ntasks) KH_HIP(hipMemcpyAsync(dpart.p, partial, ntasks * 128, hipMemcpyHostToDevice, C.stream));
    if ((rc = debug_bucket_sums(C, curve, kind, nkeys, dtoff.as<uint32_t>(), dpart.as<uint8_t>(), dbuckets.as<uint8_t>(), dbig.as<uint32_t>(), cap, dchunks.as<uint8_t>()))) return rc;
    return download_points(C, curve, dbuckets, nkeys, out_xy, out_inf);
}
int kh_debug_msm_sort(const kh_msm_sort_args_t* args, kh_msm_sort_echo_t* echo, const kh_msm_sort_out_t* out) {
    KH_REQUIRE(args && echo && args->scalars, "kh_debug_msm_sort: null argument");
    const kh_msm_sort_args_t& a = *args;
    const size_t lim = (size_t)1 << 26;
    KH_REQUIRE(a.curve == KH_CURVE_VESTA || a.curve == KH_CURVE_PALLAS, "unknown curve id %d", a.curve);
    KH_REQUIRE(a.n >= 1 && a.n <= lim && a.k >= 1 && a.k <= 8, "kh_debug_msm_sort: n = %zu (1 .. 2^26), k = %zu (1 .. 8)", (size_t)a.n, (size_t)a.k);
    KH_REQUIRE(a.precomp_c == 0 || (a.precomp_c >= 7 && a.precomp_c <= 16), "kh_debug_msm_sort: precomp_c = %d (0 or 7 .. 16)", a.precomp_c);
    KH_REQUIRE(!a.glv || a.precomp_c, "kh_debug_msm_sort: glv needs window tables (precomp_c)");
    KH_REQUIRE(!(a.wide && a.glv), "kh_debug_msm_sort: no wide table set over a glv basis");
    KH_REQUIRE(a.num_cus <= 1024, "kh_debug_msm_sort: num_cus = %u (at most 1024)", a.num_cus);
    KH_REQUIRE(a.offset <= lim && a.batch_stride <= lim && a.stride <= ((size_t)1 << 30), "kh_debug_msm_sort: offset, stride or batch_stride beyond any basis");
    KH_REQUIRE(a.stride == 0 || a.stride >= a.offset + a.n, "kh_debug_msm_sort: stride %zu below offset + n = %zu", (size_t)a.stride, (size_t)(a.offset + a.n));
    KH_REQUIRE(!a.inf || a.inf_len >= a.offset + (a.k - 1) * a.batch_stride + a.n, "kh_debug_msm_sort: %zu infinity bytes, the digits read %zu", (size_t)a.inf_len,
               (size_t)(a.offset + (a.k - 1) * a.batch_stride + a.n));
    int rc = ensure_init(); if (rc) return rc;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    MsmShape sh; MsmPlan P;
    if ((rc = debug_msm_sort_plan(C, a, sh, P, echo))) return rc;
    if (!out) return KH_OK;
    const int si = acquire_slot(nullptr, C);               // (no waiting: a test hook, called with nothing in flight)
    KH_REQUIRE(si >= 0, "kh_debug_msm_sort: no free MSM pipeline slot");
    return debug_msm_sort_run(C, C.slot[si], a, sh, P, *echo, *out);
}

}  // extern "C"
