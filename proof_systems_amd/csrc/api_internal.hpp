// api_internal.hpp -- what crosses a file boundary between the translation units of the extern "C" boundary (context.hip, srs.cpp, msm_api.cpp,
// opening.cpp, vector_api.cpp, witness_steps.cpp, witness_schedule.cpp, debug_api.cpp).  State stays private to the file that owns it: only types and functions are declared here.
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
// col_len (place_validate in witness_steps.cpp) and hand it on with `rows` on the device; the kernels take it by value.
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
void ff_negated_modulus(const uint64_t* modulus, uint64_t* nf_out);
// wiring.hip: the launchers of kh_witness_gather_dev, kh_witness_scatter_dev and kh_generic_witness_dev, queued on C.stream (arguments validated by the
// entry points; n >= 1; cells_dev: n (row, column) pairs on the device, every one inside the columns; format: a KH_CELL_* value; coeffs: the half's five
// coefficients l r o m c on the host, Montgomery -- generic_fold divides by -c_o there; half: 0 or 1)
int cell_gather(Context& C, int field, const uint64_t* witness_dev, size_t col_stride, const uint32_t* cells_dev, size_t n, int format, uint64_t* out_dev,
                uint32_t* flags_dev, unsigned bit);
int cell_scatter(Context& C, int field, const uint64_t* values_dev, int format, const uint32_t* cells_dev, size_t n, uint64_t* witness_dev, size_t col_stride,
                 uint32_t* flags_dev, unsigned bit);
// What kh_generic_witness_dev and kh_foreign_field_mul_witness_dev compute on the host, as a step of its own in front of the launch (StepPrepared
// below).  GenericHalf: c_l c_r c_m c_c, each over -c_o (all zero when c_o = 0).  FfMulConst: the modulus with its Barrett constant (limb_gadgets.hip
// owns the layout).
struct GenericHalf { uint64_t l[4][4]; };
GenericHalf generic_fold(int field, const uint64_t* coeffs);
int generic_rows_prepared(Context& C, int field, const GenericHalf& co, int half, const uint64_t* l_dev, const uint64_t* r_dev, size_t n, const WitnessPlace& at,
                          uint64_t* out_dev);
struct FfMulConst;
std::shared_ptr<const FfMulConst> ff_mul_prepare(const uint64_t* modulus);
int ff_mul_rows_prepared(Context& C, int field, const FfMulConst& m, const uint64_t* a_dev, const uint64_t* b_dev, size_t n, const WitnessPlace& at,
                         uint64_t* out_checks_dev, uint32_t* flags_dev, unsigned bit);
// lookup_rows.hip: the launcher of kh_lookup_witness_dev, queued on C.stream (arguments validated by the entry point; n >= 1, 3 n <= WAVE_BLOCK_MAX_N,
// 1 <= table_len < 2^31; table_id: 4 Montgomery limbs on the host).  The hash set over the table's keys is built per call in slots_dev, a block of
// lookup_rows_slot_bytes(table_len) that the entry point takes from the kh_dev_alloc pool.
size_t lookup_rows_slot_bytes(size_t table_len);
int lookup_rows(Context& C, const uint64_t* table_id, const uint64_t* table_keys_dev, const uint64_t* table_values_dev, size_t table_len,
                const uint64_t* keys_dev, size_t n, const WitnessPlace& at, uint64_t* out_values_dev, uint32_t* flags_dev, unsigned bit, uint32_t* slots_dev,
                size_t scratch_bytes);
// value_steps.hip: the launchers of kh_field_inverse_dev, kh_field_sqrt_dev and kh_field_bits_dev, queued on C.stream (arguments validated by the entry
// points; n >= 1, n <= WAVE_BLOCK_MAX_N; format: a KH_CELL_* value; 1 <= num_bits <= 255).  The inverse's division of the work: a lane inverts a
// run of INV_RUN elements with ONE Fermat chain (3 (INV_RUN - 1) products beside it), a launch has at most INV_MAX_BLOCKS blocks of one wave -- four
// waves for each of the chip's 1024 SIMDs --, and from INV_MAX_BLOCKS * WAVE_BLOCK * INV_RUN elements on every lane works through several runs.
static constexpr int INV_RUN = 4;
static constexpr size_t INV_MAX_BLOCKS = 4096;
int field_inverse(Context& C, int field, const uint64_t* in_dev, size_t n, uint64_t* out_dev, uint32_t* flags_dev, unsigned bit);
int field_sqrt(Context& C, int field, const uint64_t* in_dev, size_t n, uint64_t* out_dev, uint64_t* out_is_square_dev, uint32_t* flags_dev, unsigned bit);
int field_bits(Context& C, int field, const uint64_t* in_dev, int format, unsigned num_bits, size_t n, uint64_t* out_dev, uint32_t* flags_dev, unsigned bit);
// point_codec.hip: the 33-byte compressed record (include/kimchi_hip.h).  The launchers are queued on C.stream (arguments validated by the entry points;
// 1 <= n < 2^32; inf_dev, status_dev and flags_dev nullable) and the decoder counts its launch (CNT_POINT_CODEC_LAUNCHES).  points_decompress_staged is
// the host-memory route of kh_points_decompress and kh_proofs_from_wire: it takes the context's lock, stages the records through the context's
// scratch, launches once and waits; out_xy (n x 8), out_inf and status (n each) are host arrays.  (kh_srs_create_compressed in srs.cpp launches into
// the handle's table 0 itself, under the lock srs_create holds.)
int points_compress_launch(Context& C, int curve, const uint64_t* xy_dev, const uint8_t* inf_dev, size_t n, uint8_t* out_dev);
int points_decompress_launch(Context& C, int curve, const uint8_t* bytes_dev, size_t n, uint64_t* out_xy_dev, uint8_t* out_inf_dev, uint8_t* status_dev,
                             uint32_t* flags_dev, unsigned bit);
int points_decompress_staged(int curve, const uint8_t* bytes, size_t n, uint64_t* out_xy, uint8_t* out_inf, uint8_t* status);
const char* point_status_name(unsigned status);
// A group of wire steps of a witness schedule in one launch (k_cell_moves): one resident 16-byte record per cell.  The dense side of every move is
// the run's arena, `dense` words of 8 bytes from its start; flag: the step's bit, or CELL_MOVE_NO_FLAG.
struct CellMove { uint32_t row, meta, dense_lo, dense_hi; };
static constexpr uint32_t CELL_MOVE_NO_FLAG = 63;
inline CellMove cell_move(uint32_t row, uint32_t col, int format, uint32_t flag, uint64_t dense) {
    return CellMove{row, col | ((uint32_t)format << 4) | (flag << 8), (uint32_t)dense, (uint32_t)(dense >> 32)};
}
int cell_moves(Context& C, int field, bool scatter, const CellMove* moves_dev, size_t n, uint64_t* witness_dev, size_t col_stride, uint64_t* arena_dev,
               uint32_t* flags_dev);

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
// `words` uint32_t of a host table (start rows, cells, a schedule's resident block) into dst_dev, through the pinned staging ring in pieces that leave
// the ring its size: the caller's array is not read after this returns
inline int stage_words(Context& C, uint32_t* dst_dev, const uint32_t* src, size_t words) {
    const size_t piece = (size_t)1 << 15;
    counter(CNT_TABLE_STAGED_WORDS) += words;
    for (size_t i = 0; i < words; i += piece) {
        const int up = C.stage_upload(dst_dev + i, {{src + i, std::min(piece, words - i) * sizeof(uint32_t)}});
        if (up) return up;
    }
    return KH_OK;
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

// ------------------------------------------------------------------ one gadget, wire or value step with its arguments resolved (witness_steps.cpp): what a
// direct call (kh_*_witness_dev, kh_witness_gather_dev, kh_witness_scatter_dev, kh_field_*_dev) builds from its arguments and a witness schedule
// (witness_schedule.cpp) from a kh_witness_step_t.  Which argument of which call sits in in[] / out[] / param / consts is the table above KH_STEP_* in
// include/kimchi_hip.h.  at.rows and cells are on the host while validating and on the device when launching; consts stays on the host.
struct StepArgs {
    int op;                                   // KH_STEP_*
    size_t n;
    WitnessPlace at;                          // the wire steps use its witness and col_stride alone
    const void* in[3];
    void* out[2];
    unsigned param;
    const uint64_t* consts;
    uint32_t* flags; unsigned bit;            // (calls without a flag leave them 0)
    int sign;
    const uint32_t* cells; int format;
};
struct OpInfo {
    const char* name;
    int n_in, n_out;
    unsigned in_bytes[3], out_bytes[2];       // per instance; 0: the cell format decides (GATHER / SCATTER)
    bool tabled_cells;                        // the table is `cells` (2 n words), not `at.rows` (n words)
    int n_consts;                             // uint64_t words behind `consts`
    unsigned table_in = 0;                    // bit k: in[k] is a table of `param` elements of in_bytes[k], not one of them per instance (LOOKUP)
    unsigned param_out = 0;                   // bit k: out[k] holds `param` elements of out_bytes[k] per instance (BITS)
    bool value = false;                       // a value step: dense arrays in and out, no placement -- rows, row0, row_stride and cells are ignored
};
const OpInfo* step_op(int op);                // null: no such op
// What a step computes on the host before it can be launched: a generic half's c_l c_r c_m c_c over -c_o (all zero when c_o = 0), ForeignFieldMul's
// modulus with its Barrett constant.  A direct call takes it per call, a schedule once, at create.
struct StepPrepared { GenericHalf generic; std::shared_ptr<const FfMulConst> ff_mul; };
// step_validate: everything the step's direct call refuses, in that call's order and words; `call` names the call, or the schedule's step.
// step_prepare: for n >= 1 (at n = 0 coeffs / modulus may be null).  step_scratch_bytes: what VarBaseMul / EndoMul (at the current slice knob) and
// Lookup (the slots of its table's hash set) need from the kh_dev_alloc pool, 0 for every other step and at n = 0.  step_launch: queued on
// C.stream, n >= 1.
int step_validate(const char* call, int field, size_t col_len, const StepArgs& a);
StepPrepared step_prepare(int field, const StepArgs& a);
size_t step_scratch_bytes(const StepArgs& a);
int step_launch(Context& C, int field, const StepArgs& a, const StepPrepared& prepared, uint64_t* scratch_dev, size_t scratch_bytes);
}  // namespace kh
