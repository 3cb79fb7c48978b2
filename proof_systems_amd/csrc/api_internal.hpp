// api_internal.hpp -- what crosses a file boundary between the translation units of the extern "C" boundary (context.hip, srs.cpp, msm_api.cpp,
// opening.cpp, vector_api.cpp, witness_schedule.cpp, debug_api.cpp).  State stays private to the file that owns it: only types and functions are declared here.
#pragma once
#include <atomic>
#include <map>
#include <memory>

#include "common.hpp"
#include "host_ec.hpp"
#include "msm.hpp"

namespace kh {
struct LagrangeChunk { DevBuf pts; DevBuf inf; bool has_inf = false; size_t n = 0; int precomp_c = 0; };
}  // namespace kh

namespace kh {
// Everything one opening needs besides the handle's tables: a handle owns up to KH_IPA_OPENINGS of them (kh_srs::ipa_ws), each allocated the first time an
// opening claims it and kept across openings (hipMalloc / hipFree cost ~0.1 ms each: 1 ms per proof).  Workspace j writes U into slot n + 1 + j of the
// handle's window tables.  `live` / `owner` are guarded by the handle's ipa_mu; the rest belongs to the opening that holds the claim.
struct IpaWorkspace {
    int index = 0;            // j: which U slot of the handle's tables is this workspace's
    bool live = false;        // claimed by an opening (kh_ipa_begin .. kh_ipa_free)
    std::thread::id owner;    // ... begun by this thread (the SAME thread beginning a second one is a programming error)
    DevBuf a[2], b[2], coef[2], sc, partial, sg;
    hipEvent_t ev = nullptr;
    // the late rounds' materialised folded basis (csrc/rebase.hip): its window tables, the materialisation's workspaces, a low-priority side stream, the
    // events that order it against the rounds, a pinned "an output was the identity" word
    DevBuf rb_tab, rb_B, rb_part, rb_lists, rb_scratch;
    hipStream_t rb_stream = nullptr;
    hipEvent_t rb_go = nullptr, rb_snap = nullptr, rb_done = nullptr;
    uint32_t* rb_fail = nullptr;
    ~IpaWorkspace() {                                               // the DevBufs free themselves
        if (ev) (void)hipEventDestroy(ev);
        if (rb_go) (void)hipEventDestroy(rb_go);
        if (rb_snap) (void)hipEventDestroy(rb_snap);
        if (rb_done) (void)hipEventDestroy(rb_done);
        if (rb_stream) { (void)hipStreamSynchronize(rb_stream); (void)hipStreamDestroy(rb_stream); }
        if (rb_fail) (void)hipHostFree(rb_fail);
    }
};
}  // namespace kh

struct kh_srs {
    int curve = 0;
    int device = -1;          // the device its tables live on: every entry point taking this handle runs there
    size_t n = 0;
    kh::DevBuf g;                 // window tables of g_stride = n + 1 + KH_IPA_OPENINGS points: g[0..n), the slot of H, then one slot of U per opening workspace
    size_t g_stride = 0;      // (the extra bases of the opening rounds: H written once per handle, U by every kh_ipa_begin into its workspace's slot)
    int g_precomp_c = 0;
    kh::DevBuf g_wide; int g_wide_c = 0;   // second table set with wide windows (MSM_WIDE_C) for bases of >= msm_wide_min_n() points: big single MSMs
    // MSM jobs in flight that were resolved against this handle (kh::resolve_basis: the ones that may read the wide set), whatever context queued them:
    // counted under wide_mu together with the resolution (msm_api.cpp: resolve_counted), so that kh_srs_set_wide_tables(srs, 0) on another thread never frees tables a job reads.
    // Shared with the pipeline slots (MsmSlot::handle_jobs): a ticket may be waited for after the handle is gone.
    std::shared_ptr<std::atomic<int>> jobs = std::make_shared<std::atomic<int>>(0);
    std::mutex wide_mu;
    // the openings' workspaces (guarded by ipa_mu; allocated on first need, lowest index first: a handle used by one thread at a time only ever has [0])
    std::unique_ptr<kh::IpaWorkspace> ipa_ws[KH_IPA_OPENINGS];
    uint64_t h[8];
    // fixed-base table of the blinding base: h_table[i * 255 + (j - 1)] = j * 2^(8 i) * h (XYZZ), built on first use:
    // SRS::mask_custom is one scalar multiplication by h per chunk (ipa.rs:605-622) -- 32 additions instead of 255
    // doublings + ~128 additions (a proof masks 23 commitments: 3.5 ms of host time otherwise)
    std::vector<khost::xyzz> h_table;
    std::vector<uint64_t> h_multiples;     // 2^(c w) * h for the W windows (affine, 8 words each): slot n of the handle's tables
    bool h_in_tables = false;              // ... and they are there (uploaded by the first opening after creation / kh_srs_set_blinding_base)
    std::mutex h_mu;                       // h_table, h_multiples, h_in_tables
    // handle-level locks (callers may be on different contexts, kh_private_context_begin): the basis map, and the claims on the openings' workspaces
    std::mutex map_mu;
    std::mutex ipa_mu; std::condition_variable ipa_cv;
    std::map<unsigned, std::vector<std::unique_ptr<kh::LagrangeChunk>>> lagrange;
};
#define KH_ON_DEVICE_OF(srs) kh::DeviceScope dev_scope_((srs) ? (srs)->device : -1)

namespace kh {
// srs.cpp
int resolve_basis(kh_srs_t* srs, int basis, unsigned chunk, MsmBasis& out);
void xyzz_to_affine_batch(const khost::Crv& crv, const std::vector<khost::xyzz>& acc, uint64_t* out_xy, uint8_t* out_inf);
// context.hip: per (host thread, device)
hipStream_t thread_copy_stream();
hipEvent_t thread_upload_event();          // kh_msm_submit_host: orders the job's first kernel behind the upload on the copy stream
// msm_api.cpp
int acquire_slot(std::unique_lock<std::mutex>* lk, Context& C, bool side_first = false);
const char* slot_error(int si);
int wait_then_finish(std::unique_lock<std::mutex>& lk, Context& C, MsmSlot& S, uint64_t* out_xy, uint8_t* out_inf);
double last_wait_us();           // spin / block part of the last wait_then_finish on this thread
// vector_api.cpp
void xfer_trim(int d);
// Blocks of the kh_dev_alloc pool that go back to it when the call returns (work queued on the main stream before that precedes their next use).
struct PoolBlock {
    void* p = nullptr;
    ~PoolBlock() { if (p) (void)kh_dev_free(p); }
    template <class T> T* as() const { return (T*)p; }
};
// Where instance i of a gadget lands in the 15 witness columns (kh_poseidon_gate_witness_dev and the curve gates' kh_*_witness_dev): it starts at row
// rows[i], or row0 + i row_stride when rows is null; column c of the witness starts at witness + 4 c col_stride.  The entry points validate it against
// col_len (place_validate below) and hand it on with `rows` on the device; the kernels take it by value.
struct WitnessPlace {
    const uint32_t* rows;
    size_t row0, row_stride;
    uint64_t* witness;
    size_t col_stride;
    __host__ __device__ size_t start_row(size_t i) const { return rows ? (size_t)rows[i] : row0 + i * row_stride; }
    __host__ __device__ size_t offset(size_t r, size_t c) const { return 4 * (c * col_stride + r); }                  // words from a cell to the one r rows down, c columns on
    __host__ __device__ uint64_t* cell(size_t r, size_t c) const { return witness + offset(r, c); }                  // column c at row r
};
// Both files launch one lane per instance in blocks of ONE wave: a circuit's worth of instances is a few waves (5461 Poseidon gadgets in 2^16 rows: 86
// waves for 1024 SIMDs), which spread over the CUs only in blocks that small.  Up to WAVE_BLOCK_MAX_N instances per call the grid stays inside 31 bits.
static constexpr int WAVE_BLOCK = 64;
static constexpr size_t WAVE_BLOCK_MAX_N = (size_t)1 << 36;
inline dim3 blocks_of(size_t n, size_t per) { return dim3((unsigned)((n + per - 1) / per)); }      // the grid of n lanes in blocks of `per`
// poseidon.hip: the launchers of kh_poseidon_*_dev, queued on C.stream (arguments validated by the entry points; n >= 1)
int poseidon_permute(Context& C, int field, uint64_t* states_dev, size_t n);
int poseidon_hash(Context& C, int field, const uint64_t* msgs_dev, size_t msg_len, size_t n, const uint64_t* init, uint64_t* digests_dev);
int poseidon_gate_rows(Context& C, int field, const uint64_t* states_dev, size_t n, const WitnessPlace& at, uint64_t* out_states_dev);
void poseidon_set_split_max_n(size_t n);
// curve_gadgets.hip: the launchers of kh_complete_add_witness_dev, kh_endomul_scalar_witness_dev, kh_varbasemul_witness_dev and kh_endomul_witness_dev,
// queued on C.stream (arguments validated by the entry points; n >= 1).  chain_rows (VarBaseMul, or EndoMul with is_endo) works through the batch in
// slices over a scratch block of chain_scratch_bytes (chain_slice instances; the knob kh_curve_witness_set_slice_elements may move between the
// entry point's question and the launch, so the launcher is told what it got), which the entry point takes from the kh_dev_alloc pool.
int complete_add_rows(Context& C, int field, const uint64_t* p1_dev, const uint64_t* p2_dev, size_t n, const WitnessPlace& at, uint64_t* out_dev);
int endomul_scalar_rows(Context& C, int field, const uint64_t* chals_dev, unsigned num_bits, size_t n, const WitnessPlace& at, const uint64_t* endo_scalar,
                        uint64_t* out_dev);
size_t chain_slice(bool is_endo, unsigned num_bits, size_t n);
size_t chain_scratch_bytes(bool is_endo, unsigned num_bits, size_t n);
int chain_rows(Context& C, int field, bool is_endo, const uint64_t* endo, const uint64_t* base_dev, const uint64_t* acc0_dev, const uint64_t* scalars_dev,
               unsigned num_bits, size_t n, const WitnessPlace& at, uint64_t* out_acc_dev, uint64_t* out_n_dev, uint32_t* flags_dev, unsigned bit,
               uint64_t* scratch_dev, size_t scratch_bytes);
void chain_set_slice_elements(size_t elems);
// limb_gadgets.hip: the launchers of kh_range_check_witness_dev, kh_xor_witness_dev, kh_rot64_witness_dev, kh_foreign_field_add_witness_dev and
// kh_foreign_field_mul_witness_dev, queued on C.stream (arguments validated by the entry points; n >= 1, n times the instance's rows <= WAVE_BLOCK_MAX_N;
// modulus: 3 limbs of two u64 on the host, non-zero, each < 2^88).  ff_negated_modulus is host only: the limbs of 2^264 - f.
int range_check_rows(Context& C, int field, const uint64_t* limbs_dev, size_t n, int compact, const WitnessPlace& at, uint32_t* flags_dev, unsigned bit);
int xor_rows(Context& C, int field, const uint64_t* in1_dev, const uint64_t* in2_dev, unsigned bits, size_t n, const WitnessPlace& at, uint64_t* out_dev,
             uint32_t* flags_dev, unsigned bit);
int rot64_rows(Context& C, int field, const uint64_t* words_dev, unsigned rot, size_t n, const WitnessPlace& at, uint64_t* out_dev);
int ff_add_rows(Context& C, int field, const uint64_t* modulus, const uint64_t* left_dev, const uint64_t* right_dev, int sign, size_t n, const WitnessPlace& at,
                uint64_t* out_dev, uint32_t* flags_dev, unsigned bit);
int ff_mul_rows(Context& C, int field, const uint64_t* modulus, const uint64_t* a_dev, const uint64_t* b_dev, size_t n, const WitnessPlace& at,
                uint64_t* out_checks_dev, uint32_t* flags_dev, unsigned bit);
void ff_negated_modulus(const uint64_t* modulus, uint64_t* nf_out);
// wiring.hip: the launchers of kh_witness_gather_dev, kh_witness_scatter_dev and kh_generic_witness_dev, queued on C.stream (arguments validated by the
// entry points; n >= 1; cells_dev: n (row, column) pairs on the device, every one inside the columns; format: a KH_CELL_* value; coeffs: the half's five
// coefficients l r o m c on the host, Montgomery -- generic_rows divides by -c_o there, once per call; half: 0 or 1)
int cell_gather(Context& C, int field, const uint64_t* witness_dev, size_t col_stride, const uint32_t* cells_dev, size_t n, int format, uint64_t* out_dev,
                uint32_t* flags_dev, unsigned bit);
int cell_scatter(Context& C, int field, const uint64_t* values_dev, int format, const uint32_t* cells_dev, size_t n, uint64_t* witness_dev, size_t col_stride,
                 uint32_t* flags_dev, unsigned bit);
int generic_rows(Context& C, int field, const uint64_t* coeffs, int half, const uint64_t* l_dev, const uint64_t* r_dev, size_t n, const WitnessPlace& at,
                 uint64_t* out_dev);
// What the launchers of kh_generic_witness_dev and kh_foreign_field_mul_witness_dev compute on the host per call, as a step of its own: a witness
// schedule (witness_schedule.cpp) takes it once, at create, and launches through the *_prepared halves; the per-call launchers above are
// prepare + *_prepared.  GenericHalf: c_l c_r c_m c_c, each over -c_o (all zero when c_o = 0).  FfMulConst: the modulus with its Barrett constant
// (limb_gadgets.hip owns the layout).
struct GenericHalf { uint64_t l[4][4]; };
GenericHalf generic_fold(int field, const uint64_t* coeffs);
int generic_rows_prepared(Context& C, int field, const GenericHalf& co, int half, const uint64_t* l_dev, const uint64_t* r_dev, size_t n, const WitnessPlace& at,
                          uint64_t* out_dev);
struct FfMulConst;
std::shared_ptr<const FfMulConst> ff_mul_prepare(const uint64_t* modulus);
int ff_mul_rows_prepared(Context& C, int field, const FfMulConst& m, const uint64_t* a_dev, const uint64_t* b_dev, size_t n, const WitnessPlace& at,
                         uint64_t* out_checks_dev, uint32_t* flags_dev, unsigned bit);
// A group of wire steps of a witness schedule in one launch (k_cell_moves): one resident 16-byte record per cell.  The dense side of every move is
// the run's arena, `dense` words of 8 bytes from its start; flag: the step's bit, or CELL_MOVE_NO_FLAG.
struct CellMove { uint32_t row, meta, dense_lo, dense_hi; };
static constexpr uint32_t CELL_MOVE_NO_FLAG = 63;
inline CellMove cell_move(uint32_t row, uint32_t col, int format, uint32_t flag, uint64_t dense) {
    return CellMove{row, col | ((uint32_t)format << 4) | (flag << 8), (uint32_t)dense, (uint32_t)(dense >> 32)};
}
int cell_moves(Context& C, int field, bool scatter, const CellMove* moves_dev, size_t n, uint64_t* witness_dev, size_t col_stride, uint64_t* arena_dev,
               uint32_t* flags_dev);

// ------------------------------------------------------------------ what the entry points of the gadget and wire calls refuse (vector_api.cpp), shared
// with kh_witness_schedule_create (witness_schedule.cpp), which validates a step through the function its direct call uses: `call` names the call, or
// the step.
// How a vector step is queued on the main stream: under the context's lock, and when run(C) has queued it, the point is marked that a later MSM on
// another slot's stream waits for.  The entry points check their arguments in front of this.
template <class Run>
int queue_step(Run run) {
    int rc = ensure_init(); if (rc) return rc;
    Context& C = ctx();
    std::lock_guard<std::mutex> lk(C.mu);
    rc = run(C);
    if (rc == KH_OK) C.mark_async();
    return rc;
}
// what the 15 witness columns of a call that takes n instances (or cells) are refused for: a null or misaligned witness, columns that overlap or whose
// byte count overflows
inline int columns_validate(const char* call, const void* witness, size_t col_stride, size_t col_len, size_t n) {
    KH_REQUIRE(witness || n == 0, "%s: null witness_dev", call);
    KH_REQUIRE((((uintptr_t)witness) & 15) == 0, "%s: witness_dev must be 16-byte aligned", call);
    KH_REQUIRE(col_stride >= col_len, "%s: col_stride %zu is less than col_len %zu", call, col_stride, col_len);
    KH_REQUIRE(n <= WAVE_BLOCK_MAX_N && col_stride <= SIZE_MAX / (32 * 15), "%s: %zu instances in columns %zu elements apart overflow the byte count", call, n,
               col_stride);
    return KH_OK;
}
// what a placement (WitnessPlace, rows still on the host) is refused for: its columns, instances of inst_rows rows that do not fit col_len rows
inline int place_validate(const char* call, const WitnessPlace& at, size_t n, size_t col_len, size_t inst_rows) {
    int rc = columns_validate(call, at.witness, at.col_stride, col_len, n);
    if (rc) return rc;
    if (n > 0 && at.rows) {
        for (size_t i = 0; i < n; i++)
            KH_REQUIRE(col_len >= inst_rows && at.rows[i] <= col_len - inst_rows, "%s: instance %zu at row %u does not fit %zu rows (%zu rows each)", call, i,
                       at.rows[i], col_len, inst_rows);
    } else if (n > 0) {
        KH_REQUIRE(at.row_stride >= inst_rows, "%s: row_stride %zu is less than the %zu rows of an instance", call, at.row_stride, inst_rows);
        KH_REQUIRE(col_len >= inst_rows && at.row0 <= col_len - inst_rows && (n - 1) <= (col_len - inst_rows - at.row0) / at.row_stride,
                   "%s: %zu instances from row %zu, %zu rows apart, do not fit %zu rows", call, n, at.row0, at.row_stride, col_len);
    }
    return KH_OK;
}
struct GadgetPtr { const char* name; const void* p; bool required; unsigned align = 16; };
// what the gadget calls refuse alike: the field, null / misaligned device pointers, a placement that does not hold
inline int gadget_validate(const char* call, int field, std::initializer_list<GadgetPtr> ptrs, size_t n, const WitnessPlace& at, size_t col_len, size_t inst_rows) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "%s: unknown field id %d", call, field);
    for (const GadgetPtr& a : ptrs) {
        KH_REQUIRE(a.p || !a.required || n == 0, "%s: null %s", call, a.name);
        KH_REQUIRE((((uintptr_t)a.p) & (a.align - 1)) == 0, "%s: %s must be %u-byte aligned", call, a.name, a.align);
    }
    return place_validate(call, at, n, col_len, inst_rows);
}
// what the five limb gadgets refuse alike after their own arguments: gadget_validate's list, more lanes (one per instance and row) than a grid takes, a
// flag word that is misaligned or a bit that is not one
inline int limb_validate(const char* call, int field, std::initializer_list<GadgetPtr> ptrs, size_t n, const WitnessPlace& at, size_t col_len, size_t inst_rows,
                         const uint32_t* flags_dev = nullptr, unsigned bit = 0) {
    int rc = gadget_validate(call, field, ptrs, n, at, col_len, inst_rows);
    if (rc) return rc;
    KH_REQUIRE(n <= WAVE_BLOCK_MAX_N / inst_rows, "%s: %zu instances of %zu rows overflow the byte count", call, n, inst_rows);
    KH_REQUIRE(bit < 32 && (((uintptr_t)flags_dev) & 3) == 0, "%s: flag bit %u of a word at %p", call, bit, (const void*)flags_dev);
    return KH_OK;
}
// a foreign modulus: three limbs of two u64 on the host, each < 2^88, not all zero
inline int modulus_validate(const char* call, const uint64_t* modulus, size_t n) {
    KH_REQUIRE(modulus || n == 0, "%s: null modulus", call);
    if (!modulus) return KH_OK;
    KH_REQUIRE((modulus[1] | modulus[3] | modulus[5]) >> 24 == 0, "%s: a modulus limb is 2^88 or more", call);
    KH_REQUIRE((modulus[0] | modulus[1] | modulus[2] | modulus[3] | modulus[4] | modulus[5]) != 0, "%s: the modulus is zero", call);
    return KH_OK;
}
// what the two cell calls refuse alike: the field and the format, their columns, the dense buffer (`data`: out_dev / values_dev, aligned to its
// format's access), the flag word, a cell outside the 15 columns of col_len rows
inline int cells_validate(const char* call, int field, int format, const void* witness, size_t col_stride, size_t col_len, const uint32_t* cells, size_t n,
                          const char* data_name, const void* data, const uint32_t* flags_dev, unsigned bit) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "%s: unknown field id %d", call, field);
    KH_REQUIRE(format >= KH_CELL_FIELD && format <= KH_CELL_U64, "%s: unknown cell format %d", call, format);
    int rc = columns_validate(call, witness, col_stride, col_len, n);
    if (rc) return rc;
    const unsigned align = format == KH_CELL_U64 ? 8 : 16;
    KH_REQUIRE((cells && data) || n == 0, "%s: null %s", call, cells ? data_name : "cells");
    KH_REQUIRE((((uintptr_t)data) & (align - 1)) == 0, "%s: %s must be %u-byte aligned", call, data_name, align);
    KH_REQUIRE(bit < 32 && (((uintptr_t)flags_dev) & 3) == 0, "%s: flag bit %u of a word at %p", call, bit, (const void*)flags_dev);
    for (size_t i = 0; i < n; i++)
        KH_REQUIRE(cells[2 * i] < col_len && cells[2 * i + 1] < 15, "%s: cell %zu at (row %u, column %u) is outside the 15 columns of %zu rows", call, i, cells[2 * i],
                   cells[2 * i + 1], col_len);
    return KH_OK;
}
// ... and each gadget call's own list, in the order the call has always checked it
inline int poseidon_gate_validate(const char* call, int field, const void* states_dev, size_t n, const WitnessPlace& at, size_t col_len, const void* out_states_dev) {
    return gadget_validate(call, field, {{"states_dev", states_dev, true}, {"out_states_dev", out_states_dev, false}}, n, at, col_len, 12);
}
inline int complete_add_validate(const char* call, int field, const void* p1_dev, const void* p2_dev, size_t n, const WitnessPlace& at, size_t col_len,
                                 const void* out_dev) {
    return gadget_validate(call, field, {{"p1_dev", p1_dev, true}, {"p2_dev", p2_dev, true}, {"out_dev", out_dev, false}}, n, at, col_len, 1);
}
inline int endomul_scalar_validate(const char* call, int field, const void* chals_dev, unsigned num_bits, size_t n, const WitnessPlace& at, size_t col_len,
                                   const uint64_t* endo_scalar, const void* out_dev) {
    KH_REQUIRE(num_bits >= 16 && num_bits <= 128 && num_bits % 16 == 0, "%s: num_bits %u is not a multiple of 16 from 16 to 128", call, num_bits);
    int rc = gadget_validate(call, field, {{"chals_dev", chals_dev, true}, {"out_dev", out_dev, false}}, n, at, col_len, num_bits / 16);
    if (rc) return rc;
    KH_REQUIRE(endo_scalar || !out_dev || n == 0, "%s: null endo_scalar with an out_dev", call);
    return KH_OK;
}
// VarBaseMul (endo == nullptr, scalars of 4 limbs) and EndoMul (challenges of 2 limbs) share everything but their row counts
inline int chain_validate(const char* call, int field, bool is_endo, const uint64_t* endo, const void* base_dev, const void* acc0_dev, const void* scalars_dev,
                          unsigned num_bits, size_t n, const WitnessPlace& at, size_t col_len, const void* out_acc_dev, const void* out_n_dev,
                          const uint32_t* flags_dev, unsigned bit) {
    if (is_endo) KH_REQUIRE(num_bits >= 4 && num_bits <= 128 && num_bits % 4 == 0, "%s: num_bits %u is not a multiple of 4 from 4 to 128", call, num_bits);
    else KH_REQUIRE(num_bits >= 5 && num_bits <= 255 && num_bits % 5 == 0, "%s: num_bits %u is not a multiple of 5 from 5 to 255", call, num_bits);
    int rc = gadget_validate(call, field, {{"base_dev", base_dev, true}, {"acc0_dev", acc0_dev, true}, {is_endo ? "chals_dev" : "scalars_dev", scalars_dev, true},
                             {"out_acc_dev", out_acc_dev, false}, {"out_n_dev", out_n_dev, false}},
                             n, at, col_len, is_endo ? num_bits / 4 + 1 : 2 * num_bits / 5);
    if (rc) return rc;
    KH_REQUIRE(!is_endo || endo || n == 0, "%s: null endo", call);
    KH_REQUIRE(bit < 32 && (((uintptr_t)flags_dev) & 3) == 0, "%s: flag bit %u of a word at %p", call, bit, (void*)flags_dev);
    return KH_OK;
}
inline int range_check_validate(const char* call, int field, const void* limbs_dev, size_t n, int compact, const WitnessPlace& at, size_t col_len,
                                const uint32_t* flags_dev, unsigned bit) {
    KH_REQUIRE(compact == 0 || compact == 1, "%s: compact is %d, not 0 or 1", call, compact);
    return limb_validate(call, field, {{"limbs_dev", limbs_dev, true}}, n, at, col_len, 4, flags_dev, bit);
}
inline int xor_validate(const char* call, int field, const void* in1_dev, const void* in2_dev, unsigned bits, size_t n, const WitnessPlace& at, size_t col_len,
                        const void* out_dev, const uint32_t* flags_dev, unsigned bit) {
    KH_REQUIRE(bits >= 1 && bits <= 254, "%s: bits %u is not from 1 to 254", call, bits);
    return limb_validate(call, field, {{"in1_dev", in1_dev, true}, {"in2_dev", in2_dev, true}, {"out_dev", out_dev, false}}, n, at, col_len, (bits + 15) / 16 + 1,
                         flags_dev, bit);
}
inline int rot64_validate(const char* call, int field, const void* words_dev, unsigned rot, size_t n, const WitnessPlace& at, size_t col_len, const void* out_dev) {
    KH_REQUIRE(rot <= 63, "%s: rot %u is not from 0 to 63", call, rot);
    return limb_validate(call, field, {{"words_dev", words_dev, true, 8}, {"out_dev", out_dev, false, 8}}, n, at, col_len, 3);
}
inline int ff_add_validate(const char* call, int field, const uint64_t* modulus, const void* left_dev, const void* right_dev, int sign, size_t n,
                           const WitnessPlace& at, size_t col_len, const void* out_dev, const uint32_t* flags_dev, unsigned bit) {
    KH_REQUIRE(sign == 1 || sign == -1, "%s: sign is %d, not +1 or -1", call, sign);
    int rc = modulus_validate(call, modulus, n);
    if (rc) return rc;
    return limb_validate(call, field, {{"left_dev", left_dev, true}, {"right_dev", right_dev, true}, {"out_dev", out_dev, false}}, n, at, col_len, 2, flags_dev, bit);
}
inline int ff_mul_validate(const char* call, int field, const uint64_t* modulus, const void* a_dev, const void* b_dev, size_t n, const WitnessPlace& at,
                           size_t col_len, const void* out_checks_dev, const uint32_t* flags_dev, unsigned bit) {
    int rc = modulus_validate(call, modulus, n);
    if (rc) return rc;
    return limb_validate(call, field, {{"a_dev", a_dev, true}, {"b_dev", b_dev, true}, {"out_checks_dev", out_checks_dev, false}}, n, at, col_len, 2, flags_dev, bit);
}
inline int generic_validate(const char* call, int field, const uint64_t* coeffs, int half, const void* l_dev, const void* r_dev, size_t n, const WitnessPlace& at,
                            size_t col_len, const void* out_dev) {
    KH_REQUIRE(half == 0 || half == 1, "%s: half is %d, not 0 or 1", call, half);
    int rc = gadget_validate(call, field, {{"l_dev", l_dev, true}, {"r_dev", r_dev, false}, {"out_dev", out_dev, false}}, n, at, col_len, 1);
    if (rc) return rc;
    KH_REQUIRE(coeffs || n == 0, "%s: null coeffs", call);
    return KH_OK;
}
}  // namespace kh
