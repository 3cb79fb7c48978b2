// point_codec.hip -- the 33-byte compressed point record of the reference (ark-serialize; SURVEY A.1, oracle/pasta.py: Curve.compress / decompress) on the
// device, for kh_points_compress(_dev), kh_points_decompress(_dev), kh_srs_create_compressed (srs.cpp) and kh_proofs_from_wire: x as 32 little-endian bytes
// of the canonical integer, then a flag byte -- 0x80: y > (p - 1) / 2, 0x40: infinity, else 0.  F is the curve's BASE field, b = 5 on both curves.
// Blocks of one wave, one lane per record, a tail guard on n, no LDS, no per-lane scratch memory, no atomics but the flag word's one per wave.
//
//   k_points_decompress   flag and x < p on the integer, x -> Montgomery, rhs = x^3 + 5, fe_sqrt of field_sqrt.cuh (the root ark-ff returns, every loop
//                         bounded), y negated when its sign is not the flag's.  About 600 products per lane, nearly all of them the root: the 33 bytes at
//                         an unaligned stride are read byte by byte into registers and do not matter next to it.  The lanes of a wave take different
//                         numbers of Tonelli-Shanks rounds; the wave takes the longest of them.
//   k_points_compress     x and y out of Montgomery form, the flag from y, 33 byte stores.
#include <vector>

#include "common.hpp"
#include "field.cuh"
#include "field_sqrt.cuh"
#include "api_internal.hpp"
#include "wire_handles.hpp"

namespace kh {

__device__ __forceinline__ void raise_point_flag(u32* flags, u32 bit, bool bad) {
    if (flags && __any(bad) && (threadIdx.x & 63u) == 0) atomicOr(flags, 1u << bit);
}

// word i of (p - 1) / 2: p - 1 has the words [0, P1, P2, P3, 0, 0, 0, 2^30]
template <class F>
__device__ __forceinline__ u32 half_pm1(int i) {
    const u32 lo = i == 0 ? 0u : Fe<F>::pw(i), hi = i < 7 ? Fe<F>::pw(i + 1) : 0u;
    return (lo >> 1) | (hi << 31);
}
// a < p on plain integers: a - p borrows
template <class F>
__device__ __forceinline__ bool below_p(const Fe<F>& a) {
    u32 br = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) br = (u32)(((u64)a.v[k] - Fe<F>::pw(k) - br) >> 63);
    return br != 0;
}
// a > (p - 1) / 2 on plain integers: (p - 1) / 2 - a borrows
template <class F>
__device__ __forceinline__ bool above_half(const Fe<F>& a) {
    u32 br = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) br = (u32)(((u64)half_pm1<F>(k) - a.v[k] - br) >> 63);
    return br != 0;
}

template <class F>
__global__ void __launch_bounds__(WAVE_BLOCK)
k_points_decompress(const uint8_t* __restrict__ bytes, size_t n, SqrtParams P, u64* __restrict__ out_xy, uint8_t* __restrict__ out_inf,
                    uint8_t* __restrict__ status, u32* __restrict__ flags, u32 bit) {
    const size_t i = (size_t)blockIdx.x * WAVE_BLOCK + threadIdx.x;
    bool bad = false;
    if (i < n) {
        const uint8_t* const rec = bytes + KH_POINT_BYTES * i;              // any alignment: byte loads, every index a constant
        Fe<F> x;
#pragma unroll
        for (int k = 0; k < 8; k++)
            x.v[k] = (u32)rec[4 * k] | ((u32)rec[4 * k + 1] << 8) | ((u32)rec[4 * k + 2] << 16) | ((u32)rec[4 * k + 3] << 24);
        const u32 flag = rec[32];
        u32 st = KH_POINT_OK;
        if ((flag & 0x3fu) || flag == 0xc0u || (flag == 0x40u && !x.is_zero())) st = KH_POINT_BAD_FLAGS;
        else if (flag == 0x40u) st = KH_POINT_INFINITY;
        else if (!below_p<F>(x)) st = KH_POINT_NOT_CANONICAL;
        Fe<F> xm = Fe<F>::zero(), y = Fe<F>::zero();
        if (st == KH_POINT_OK) {
            Fe<F> five = Fe<F>::zero();
            five.v[0] = 5;
            xm = to_mont<F>(x);
            const Fe<F> rhs = add<F>(mul<F>(sqr<F>(xm), xm), to_mont<F>(five));
            // y = 0 cannot occur: it would be a point of order 2, and both curves have odd prime order.  No branch for it.
            if (fe_sqrt<F>(rhs, P, y)) {
                if (above_half<F>(from_mont<F>(y)) != (flag == 0x80u)) y = neg<F>(y);
            } else {
                st = KH_POINT_NOT_ON_CURVE;
                xm = Fe<F>::zero();
            }
        }
        xm.store(out_xy + 8 * i);
        y.store(out_xy + 8 * i + 4);
        out_inf[i] = st == KH_POINT_INFINITY ? 1 : 0;
        if (status) status[i] = (uint8_t)st;
        bad = st != KH_POINT_OK && st != KH_POINT_INFINITY;
    }
    raise_point_flag(flags, bit, bad);
}

template <class F>
__global__ void __launch_bounds__(WAVE_BLOCK)
k_points_compress(const u64* __restrict__ xy, const uint8_t* __restrict__ inf, size_t n, uint8_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * WAVE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const bool is_inf = inf && inf[i];
    Fe<F> x = from_mont<F>(Fe<F>::load(xy + 8 * i));
    const Fe<F> y = from_mont<F>(Fe<F>::load(xy + 8 * i + 4));
    if (is_inf) x = Fe<F>::zero();                                          // whatever xy holds
    uint8_t* const rec = out + KH_POINT_BYTES * i;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        rec[4 * k] = (uint8_t)x.v[k]; rec[4 * k + 1] = (uint8_t)(x.v[k] >> 8); rec[4 * k + 2] = (uint8_t)(x.v[k] >> 16); rec[4 * k + 3] = (uint8_t)(x.v[k] >> 24);
    }
    rec[32] = is_inf ? 0x40 : above_half<F>(y) ? 0x80 : 0x00;
}

int points_compress_launch(Context& C, int curve, const uint64_t* xy_dev, const uint8_t* inf_dev, size_t n, uint8_t* out_dev) {
    C.timer.begin(C.stream);
    KH_CURVE_LAUNCH(curve, k_points_compress<F>, blocks_of(n, WAVE_BLOCK), dim3(WAVE_BLOCK), 0, C.stream, (const u64*)xy_dev, inf_dev, n, out_dev);
    C.timer.mark("points_compress", C.stream);
    counter(CNT_POINT_CODEC_ENCODE_LAUNCHES)++;
    return KH_OK;
}
int points_decompress_launch(Context& C, int curve, const uint8_t* bytes_dev, size_t n, uint64_t* out_xy_dev, uint8_t* out_inf_dev, uint8_t* status_dev,
                             uint32_t* flags_dev, unsigned bit) {
    const SqrtParams P = sqrt_params(khost::Fld(khost::base_field_id(curve)));
    C.timer.begin(C.stream);
    KH_CURVE_LAUNCH(curve, k_points_decompress<F>, blocks_of(n, WAVE_BLOCK), dim3(WAVE_BLOCK), 0, C.stream, bytes_dev, n, P, (u64*)out_xy_dev, out_inf_dev,
                    status_dev, flags_dev, (u32)bit);
    C.timer.mark("points_decompress", C.stream);
    counter(CNT_POINT_CODEC_LAUNCHES)++;
    return KH_OK;
}

const char* point_status_name(unsigned status) {
    static const char* const NAMES[] = {"KH_POINT_OK", "KH_POINT_INFINITY", "KH_POINT_BAD_FLAGS", "KH_POINT_NOT_CANONICAL", "KH_POINT_NOT_ON_CURVE"};
    return status <= KH_POINT_NOT_ON_CURVE ? NAMES[status] : "an unknown status";
}

int points_decompress_staged(int curve, const uint8_t* bytes, size_t n, uint64_t* out_xy, uint8_t* out_inf, uint8_t* status) {
    int rc = ensure_init(); if (rc) return rc;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    DevBuf &rec = C.scratch("point_codec_bytes"), &xy = C.scratch("point_codec_xy"), &inf = C.scratch("point_codec_inf"), &st = C.scratch("point_codec_status");
    if ((rc = rec.reserve(n * KH_POINT_BYTES)) || (rc = xy.reserve(n * 64)) || (rc = inf.reserve(n)) || (rc = st.reserve(n))) return rc;
    KH_HIP(hipMemcpyAsync(rec.p, bytes, n * KH_POINT_BYTES, hipMemcpyHostToDevice, C.stream));
    if ((rc = points_decompress_launch(C, curve, rec.as<uint8_t>(), n, xy.as<uint64_t>(), inf.as<uint8_t>(), st.as<uint8_t>(), nullptr, 0))) return rc;
    KH_HIP(hipMemcpyAsync(out_xy, xy.p, n * 64, hipMemcpyDeviceToHost, C.stream));
    KH_HIP(hipMemcpyAsync(out_inf, inf.p, n, hipMemcpyDeviceToHost, C.stream));
    KH_HIP(hipMemcpyAsync(status, st.p, n, hipMemcpyDeviceToHost, C.stream));
    KH_HIP(hipStreamSynchronize(C.stream));
    return KH_OK;
}

}  // namespace kh

using namespace kh;

namespace {
// what the four point calls refuse alike, before anything is launched
int codec_validate(const char* call, int curve, size_t n, const void* xy, std::initializer_list<const void*> required) {
    KH_REQUIRE(curve == KH_CURVE_VESTA || curve == KH_CURVE_PALLAS, "%s: unknown curve id %d", call, curve);
    KH_REQUIRE(n < ((size_t)1 << 32), "%s: %zu records, the limit is 2^32 - 1", call, n);
    for (const void* p : required) KH_REQUIRE(p || n == 0, "%s: null argument", call);
    KH_REQUIRE((((uintptr_t)xy) & 15) == 0, "%s: the xy array must be 16-byte aligned", call);
    return KH_OK;
}
bool point_section(size_t s) {             // kh_proof_from_sections' rule
    return s <= KH_PROOF_PUBLIC_COMM || s == KH_PROOF_LR || s == KH_PROOF_DELTA || s == KH_PROOF_SG || s >= KH_PROOF_LOOKUP_SORTED_COMM;
}
}  // namespace

namespace kh {
// kh_proofs_from_wire.  extra (nullable): one more list of point records per proof -- the previous-challenge commitments of a serialised proof --, slot
// n_sections of the proof: decoded in the same launch, handed back in extra_xy[p] / extra_inf[p] and not to kh_proof_from_sections.
int proofs_from_wire(const char* call, int curve, const kh_wire_section_t* sections, size_t n_sections, size_t k, const kh_wire_section_t* extra,
                     std::vector<uint64_t>* extra_xy, std::vector<uint8_t>* extra_inf, kh_proof_t** out) {
    KH_REQUIRE(curve == KH_CURVE_VESTA || curve == KH_CURVE_PALLAS, "%s: unknown curve id %d", call, curve);
    KH_REQUIRE(sections && out && k > 0 && n_sections > 0 && n_sections <= KH_PROOF_LOOKUP_RUNTIME_COMM + 1, "%s: null argument, no proof or more than %d sections",
               call, KH_PROOF_LOOKUP_RUNTIME_COMM + 1);
    KH_REQUIRE(!extra || (extra_xy && extra_inf), "%s: null argument", call);
    const size_t slots = n_sections + 1;                                    // per proof: its sections, then the extra list
    KH_REQUIRE(k < ((size_t)1 << 32) / slots, "%s: %zu proofs", call, k);
    auto ignored = [&](size_t s) { return s == KH_PROOF_PUBLIC_COMM || s == KH_PROOF_CHALLENGES; };
    auto is_points = [&](size_t s) { return s == n_sections || point_section(s); };
    auto slot = [&](size_t j) -> kh_wire_section_t {
        const size_t p = j / slots, s = j % slots;
        if (s == n_sections) return extra ? extra[p] : kh_wire_section_t{nullptr, 0};
        return sections[p * n_sections + s];
    };
    // every point of every proof, in (proof, section) order: first[j] = where the records of slot j begin
    std::vector<size_t> first(k * slots + 1, 0);
    size_t n_elems = 0;
    for (size_t j = 0; j < k * slots; j++) {
        const kh_wire_section_t in = slot(j);
        const size_t s = j % slots;
        KH_REQUIRE(in.bytes || !in.count || ignored(s), "%s: proof %zu section %zu has %zu entries and no bytes", call, j / slots, s, in.count);
        KH_REQUIRE(in.count < ((size_t)1 << 32), "%s: proof %zu section %zu has %zu entries", call, j / slots, s, in.count);
        const size_t cnt = ignored(s) ? 0 : in.count;
        first[j + 1] = first[j] + (is_points(s) ? cnt : 0);
        if (!is_points(s)) n_elems += cnt;
    }
    const size_t n_points = first.back();
    KH_REQUIRE(n_points < ((size_t)1 << 32), "%s: %zu points, the limit is 2^32 - 1", call, n_points);
    // the elements: little-endian canonical integers -> Montgomery limbs
    const khost::Fld SF(khost::scalar_field_id(curve));
    std::vector<uint64_t> elems(4 * n_elems);
    std::vector<size_t> elem_first(k * slots, 0);
    size_t e = 0;
    for (size_t j = 0; j < k * slots; j++) {
        const size_t s = j % slots;
        elem_first[j] = e;
        if (is_points(s) || ignored(s)) continue;
        const kh_wire_section_t in = slot(j);
        for (size_t i = 0; i < in.count; i++, e++) {
            khost::fe v;
            memcpy(v.l, in.bytes + 32 * i, 32);
            KH_REQUIRE(!khost::geq(v, SF.f.p), "%s: proof %zu section %zu element %zu is not a canonical field element (>= p)", call, j / slots, s, i);
            v = SF.to_mont(v);
            memcpy(elems.data() + 4 * e, v.l, 32);
        }
    }
    // the points: gathered, decoded in one launch
    std::vector<uint8_t> records(n_points * KH_POINT_BYTES), inf(n_points), status(n_points);
    std::vector<uint64_t> xy(8 * n_points);
    for (size_t j = 0; j < k * slots; j++)
        if (first[j + 1] > first[j]) memcpy(records.data() + first[j] * KH_POINT_BYTES, slot(j).bytes, (first[j + 1] - first[j]) * KH_POINT_BYTES);
    int rc = ensure_init(); if (rc) return rc;
    if (n_points && (rc = points_decompress_staged(curve, records.data(), n_points, xy.data(), inf.data(), status.data()))) return rc;
    for (size_t j = 0; j < k * slots; j++)
        for (size_t i = first[j]; i < first[j + 1]; i++) {
            if (status[i] == KH_POINT_OK || status[i] == KH_POINT_INFINITY) continue;
            if (j % slots == n_sections) set_error("%s: proof %zu previous-challenge commitment point %zu is %s", call, j / slots, i - first[j], point_status_name(status[i]));
            else set_error("%s: proof %zu section %zu point %zu is %s", call, j / slots, j % slots, i - first[j], point_status_name(status[i]));
            return KH_E_INVALID;
        }
    std::vector<kh_proof_t*> made(k, nullptr);
    for (size_t p = 0; p < k && !rc; p++) {
        kh_section_t secs[KH_PROOF_LOOKUP_RUNTIME_COMM + 1] = {};
        for (size_t s = 0; s < n_sections; s++) {
            const size_t j = p * slots + s;
            const size_t cnt = sections[p * n_sections + s].count;
            if (ignored(s) || !cnt) continue;
            if (point_section(s)) secs[s] = kh_section_t{xy.data() + 8 * first[j], inf.data() + first[j], cnt};
            else secs[s] = kh_section_t{elems.data() + 4 * elem_first[j], nullptr, cnt};
        }
        rc = kh_proof_from_sections(secs, n_sections, &made[p]);
    }
    if (rc) { for (kh_proof_t* p : made) kh_proof_free(p); return rc; }
    for (size_t p = 0; p < k && extra; p++) {
        const size_t j = p * slots + n_sections;
        extra_xy[p].assign(xy.begin() + 8 * first[j], xy.begin() + 8 * first[j + 1]);
        extra_inf[p].assign(inf.begin() + first[j], inf.begin() + first[j + 1]);
    }
    for (size_t p = 0; p < k; p++) out[p] = made[p];
    return KH_OK;
}
}  // namespace kh

extern "C" {

int kh_points_compress(int curve, const uint64_t* xy, const uint8_t* inf, size_t n, uint8_t* out) {
    int rc = codec_validate("kh_points_compress", curve, n, xy, {xy, out});
    if (rc) return rc;
    if ((rc = ensure_init()) || n == 0) return rc;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    DevBuf &rec = C.scratch("point_codec_bytes"), &pts = C.scratch("point_codec_xy"), &fl = C.scratch("point_codec_inf");
    if ((rc = rec.reserve(n * KH_POINT_BYTES)) || (rc = pts.reserve(n * 64)) || (inf && (rc = fl.reserve(n)))) return rc;
    KH_HIP(hipMemcpyAsync(pts.p, xy, n * 64, hipMemcpyHostToDevice, C.stream));
    if (inf) KH_HIP(hipMemcpyAsync(fl.p, inf, n, hipMemcpyHostToDevice, C.stream));
    if ((rc = points_compress_launch(C, curve, pts.as<uint64_t>(), inf ? fl.as<uint8_t>() : nullptr, n, rec.as<uint8_t>()))) return rc;
    KH_HIP(hipMemcpyAsync(out, rec.p, n * KH_POINT_BYTES, hipMemcpyDeviceToHost, C.stream));
    KH_HIP(hipStreamSynchronize(C.stream));
    return KH_OK;
}

int kh_points_decompress(int curve, const uint8_t* bytes, size_t n, uint64_t* out_xy, uint8_t* out_inf, uint8_t* status, size_t* first_bad) {
    int rc = codec_validate("kh_points_decompress", curve, n, out_xy, {bytes, out_xy, out_inf});
    if (rc) return rc;
    if (n == 0) return ensure_init();
    std::vector<uint8_t> own;
    if (!status) { own.resize(n); status = own.data(); }
    if ((rc = points_decompress_staged(curve, bytes, n, out_xy, out_inf, status))) return rc;
    for (size_t i = 0; i < n; i++)
        if (status[i] != KH_POINT_OK && status[i] != KH_POINT_INFINITY) {
            if (first_bad) *first_bad = i;
            set_error("kh_points_decompress: record %zu is %s", i, point_status_name(status[i]));
            return KH_E_INVALID;
        }
    return KH_OK;
}

int kh_points_compress_dev(int curve, const uint64_t* xy_dev, const uint8_t* inf_dev, size_t n, uint8_t* out_dev) {
    int rc = codec_validate("kh_points_compress_dev", curve, n, xy_dev, {xy_dev, out_dev});
    if (rc) return rc;
    if (n == 0) return ensure_init();
    return queue_step([&](Context& C) { return points_compress_launch(C, curve, xy_dev, inf_dev, n, out_dev); });
}

int kh_points_decompress_dev(int curve, const uint8_t* bytes_dev, size_t n, uint64_t* out_xy_dev, uint8_t* out_inf_dev, uint8_t* status_dev,
                             uint32_t* flags_dev, unsigned bit) {
    int rc = codec_validate("kh_points_decompress_dev", curve, n, out_xy_dev, {bytes_dev, out_xy_dev, out_inf_dev});
    if (rc) return rc;
    KH_REQUIRE(bit < 32 && (((uintptr_t)flags_dev) & 3) == 0, "kh_points_decompress_dev: flag bit %u of a word at %p", bit, (const void*)flags_dev);
    if (n == 0) return ensure_init();
    return queue_step([&](Context& C) { return points_decompress_launch(C, curve, bytes_dev, n, out_xy_dev, out_inf_dev, status_dev, flags_dev, bit); });
}

int kh_proofs_from_wire(int curve, const kh_wire_section_t* sections, size_t n_sections, size_t k, kh_proof_t** out) {
    return proofs_from_wire("kh_proofs_from_wire", curve, sections, n_sections, k, nullptr, nullptr, nullptr, out);
}

}  // extern "C"
