// witness_schedule.cpp -- kh_witness_schedule_*: the list of gadget and wire calls that writes a circuit's witness, compiled once and run per proof.
// Create does what depends on the circuit alone: every step goes through the validator of its direct call (api_internal.hpp) with stand-in pointers
// that carry the refs' nullness and alignment, the rows[] / cells tables go into one resident device block, the host-side constants are prepared
// (generic_fold, ff_mul_prepare), and consecutive wire steps over the arena are merged into groups of one launch each (wiring.hip: k_cell_moves).
// A run resolves the refs against this run's buffers and arena and calls the same launchers as the direct calls, under one hold of the context's
// lock: O(steps) host work, nothing staged, nothing validated per cell.
#include <string.h>
#include <iterator>
#include <unordered_set>

#include "api_internal.hpp"

using namespace kh;

namespace {
struct OpInfo {
    const char* name;
    int n_in, n_out;
    unsigned in_bytes[3], out_bytes[2];       // per instance; 0: the cell format decides (GATHER / SCATTER)
    bool tabled_cells;                        // the table is `cells` (2 n words), not `rows` (n words)
    int n_consts;                             // uint64_t words copied from `consts`
};
constexpr OpInfo OPS[] = {
    {"KH_STEP_GATHER", 0, 1, {0, 0, 0}, {0, 0}, true, 0},
    {"KH_STEP_SCATTER", 1, 0, {0, 0, 0}, {0, 0}, true, 0},
    {"KH_STEP_GENERIC", 2, 1, {32, 32, 0}, {32, 0}, false, 20},
    {"KH_STEP_POSEIDON", 1, 1, {96, 0, 0}, {96, 0}, false, 0},
    {"KH_STEP_COMPLETE_ADD", 2, 1, {64, 64, 0}, {64, 0}, false, 0},
    {"KH_STEP_VARBASEMUL", 3, 2, {64, 64, 32}, {64, 32}, false, 0},
    {"KH_STEP_ENDOMUL", 3, 2, {64, 64, 16}, {64, 32}, false, 4},
    {"KH_STEP_ENDOMUL_SCALAR", 1, 1, {16, 0, 0}, {32, 0}, false, 4},
    {"KH_STEP_RANGE_CHECK", 1, 0, {48, 0, 0}, {0, 0}, false, 0},
    {"KH_STEP_XOR", 2, 1, {32, 32, 0}, {32, 0}, false, 0},
    {"KH_STEP_ROT64", 1, 1, {8, 0, 0}, {8, 0}, false, 0},
    {"KH_STEP_FF_ADD", 2, 1, {48, 48, 0}, {48, 0}, false, 6},
    {"KH_STEP_FF_MUL", 2, 1, {48, 48, 0}, {144, 0}, false, 6},
};
constexpr int N_OPS = sizeof(OPS) / sizeof(OPS[0]);
size_t format_bytes(int format) { return format == KH_CELL_FIELD || format == KH_CELL_INT256 ? 32 : format == KH_CELL_U64 ? 8 : 16; }

struct Step {
    kh_witness_step_t s;                      // rows / cells / consts are null here: the tables are resident, the constants below
    size_t table = 0;                         // word offset of the step's rows[] / cells in the resident block
    bool has_table = false, has_consts = false;
    uint64_t consts[20];
    GenericHalf generic;
    std::shared_ptr<const FfMulConst> ff_mul;
};
// one launcher invocation of a run: a step, or a group of wire steps [first, last] as n_moves records at word offset `moves`
struct Launch { bool fused, scatter; size_t first, moves, n_moves; };

// the stand-in of a ref for the direct calls' validators: null when absent, else an address with the ref's alignment (a bound buffer and the arena
// are 16-byte aligned: kh_witness_schedule_run checks the buffers, the pool aligns the arena)
const void* stand_in(const kh_witness_ref_t& r) { return r.buf == KH_REF_NONE ? nullptr : (const void*)(uintptr_t)(4096 + (r.offset & 4095)); }
}  // namespace

struct kh_witness_schedule {
    int field = 0, device = -1;
    size_t col_len = 0, arena_bytes = 0, n_bufs = 0, resident_bytes = 0;
    std::vector<Step> steps;
    std::vector<Launch> launches;
    DevBuf resident;
};

namespace {
// a ref of step `call`: a known buffer, and inside the arena when it is there (`bytes` per instance)
int ref_validate(const char* call, const char* what, int k, const kh_witness_ref_t& r, size_t bytes, size_t n, size_t arena_bytes, size_t n_bufs) {
    KH_REQUIRE(r.buf >= KH_REF_NONE && (r.buf < 0 || (size_t)r.buf < n_bufs), "%s: %s[%d] names buffer %d of %zu", call, what, k, r.buf, n_bufs);
    if (r.buf == KH_REF_ARENA)
        KH_REQUIRE(r.offset <= arena_bytes && n <= (arena_bytes - r.offset) / bytes, "%s: %s[%d] at arena offset %zu, %zu x %zu bytes, ends past the arena's %zu bytes",
                   call, what, k, r.offset, n, bytes, arena_bytes);
    return KH_OK;
}

// every check of the step's direct call, through that call's validator
int step_validate(const char* call, int field, size_t col_len, const kh_witness_step_t& s, size_t arena_bytes, size_t n_bufs) {
    const OpInfo& op = OPS[s.op];
    KH_REQUIRE(s.flag_bit < 32 || s.flag_bit == KH_STEP_NO_FLAG, "%s: flag_bit %u is neither below 32 nor KH_STEP_NO_FLAG", call, s.flag_bit);
    const uint32_t* const flags = s.flag_bit == KH_STEP_NO_FLAG ? nullptr : (const uint32_t*)(uintptr_t)4096;
    const unsigned bit = s.flag_bit == KH_STEP_NO_FLAG ? 0 : s.flag_bit;
    const WitnessPlace at{s.rows, s.row0, s.row_stride, (uint64_t*)(uintptr_t)4096, col_len};
    const void* in[3] = {stand_in(s.in[0]), stand_in(s.in[1]), stand_in(s.in[2])};
    const void* out[2] = {stand_in(s.out[0]), stand_in(s.out[1])};
    int rc = KH_OK;
    switch (s.op) {
    case KH_STEP_GATHER:
        rc = cells_validate(call, field, s.format, at.witness, col_len, col_len, s.cells, s.n, "out_dev", out[0], flags, bit); break;
    case KH_STEP_SCATTER:
        rc = cells_validate(call, field, s.format, at.witness, col_len, col_len, s.cells, s.n, "values_dev", in[0], flags, bit); break;
    case KH_STEP_GENERIC:
        rc = generic_validate(call, field, s.consts, (int)s.param, in[0], in[1], s.n, at, col_len, out[0]); break;
    case KH_STEP_POSEIDON:
        rc = poseidon_gate_validate(call, field, in[0], s.n, at, col_len, out[0]); break;
    case KH_STEP_COMPLETE_ADD:
        rc = complete_add_validate(call, field, in[0], in[1], s.n, at, col_len, out[0]); break;
    case KH_STEP_VARBASEMUL:
        rc = chain_validate(call, field, false, nullptr, in[0], in[1], in[2], s.param, s.n, at, col_len, out[0], out[1], flags, bit); break;
    case KH_STEP_ENDOMUL:
        rc = chain_validate(call, field, true, s.consts, in[0], in[1], in[2], s.param, s.n, at, col_len, out[0], out[1], flags, bit); break;
    case KH_STEP_ENDOMUL_SCALAR:
        rc = endomul_scalar_validate(call, field, in[0], s.param, s.n, at, col_len, s.consts, out[0]); break;
    case KH_STEP_RANGE_CHECK:
        rc = range_check_validate(call, field, in[0], s.n, (int)s.param, at, col_len, flags, bit); break;
    case KH_STEP_XOR:
        rc = xor_validate(call, field, in[0], in[1], s.param, s.n, at, col_len, out[0], flags, bit); break;
    case KH_STEP_ROT64:
        rc = rot64_validate(call, field, in[0], s.param, s.n, at, col_len, out[0]); break;
    case KH_STEP_FF_ADD:
        rc = ff_add_validate(call, field, s.consts, in[0], in[1], s.sign, s.n, at, col_len, out[0], flags, bit); break;
    case KH_STEP_FF_MUL:
        rc = ff_mul_validate(call, field, s.consts, in[0], in[1], s.n, at, col_len, out[0], flags, bit); break;
    }
    if (rc) return rc;
    // (after the call's own list: n is known to be small enough for the extents, the format to be one)
    const size_t cell_bytes = op.tabled_cells ? format_bytes(s.format) : 0;
    for (int k = 0; k < op.n_in; k++)
        if ((rc = ref_validate(call, "in", k, s.in[k], op.in_bytes[k] ? op.in_bytes[k] : cell_bytes, s.n, arena_bytes, n_bufs))) return rc;
    for (int k = 0; k < op.n_out; k++)
        if ((rc = ref_validate(call, "out", k, s.out[k], op.out_bytes[k] ? op.out_bytes[k] : cell_bytes, s.n, arena_bytes, n_bufs))) return rc;
    return KH_OK;
}

// the wire steps of a group so far: what a further step must not touch to join it
struct Group {
    bool open = false, scatter = false;
    std::map<size_t, size_t> extents;                   // gathers: arena [begin, end) of the outputs, disjoint
    std::unordered_set<uint64_t> targets;               // scatters: (row, column) of the cells written
    bool takes(const kh_witness_step_t& s) const {
        if (!open || scatter != (s.op == KH_STEP_SCATTER)) return false;
        if (!scatter) {
            const size_t b = s.out[0].offset, e = b + s.n * format_bytes(s.format);
            auto it = extents.lower_bound(b);           // the first extent that begins at or after b, and the one before it
            if (it != extents.end() && it->first < e) return false;
            if (it != extents.begin() && std::prev(it)->second > b) return false;
            return true;
        }
        for (size_t i = 0; i < s.n; i++)
            if (targets.count(((uint64_t)s.cells[2 * i] << 4) | s.cells[2 * i + 1])) return false;
        return true;
    }
    void add(const kh_witness_step_t& s) {
        open = true; scatter = s.op == KH_STEP_SCATTER;
        if (!scatter) extents[s.out[0].offset] = s.out[0].offset + s.n * format_bytes(s.format);
        else for (size_t i = 0; i < s.n; i++) targets.insert(((uint64_t)s.cells[2 * i] << 4) | s.cells[2 * i + 1]);
    }
    void close() { open = false; extents.clear(); targets.clear(); }
};

template <class T>
T* resolve(const kh_witness_ref_t& r, void* const* bufs, void* arena) {
    if (r.buf == KH_REF_NONE) return nullptr;
    return (T*)((char*)(r.buf == KH_REF_ARENA ? arena : bufs[r.buf]) + r.offset);
}
bool is_chain(const Step& st) { return (st.s.op == KH_STEP_VARBASEMUL || st.s.op == KH_STEP_ENDOMUL) && st.s.n > 0; }
}  // namespace

extern "C" {

int kh_witness_schedule_create(int field, size_t col_len, const kh_witness_step_t* steps, size_t n_steps, size_t arena_bytes, size_t n_bufs,
                               kh_witness_schedule_t** out) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "kh_witness_schedule_create: unknown field id %d", field);
    KH_REQUIRE(out && (steps || n_steps == 0), "kh_witness_schedule_create: null %s", out ? "steps" : "out");
    KH_REQUIRE(n_bufs <= (size_t)INT32_MAX && col_len <= SIZE_MAX / (32 * 15), "kh_witness_schedule_create: %zu buffers, columns of %zu rows", n_bufs, col_len);
    std::unique_ptr<kh_witness_schedule> S(new (std::nothrow) kh_witness_schedule);
    KH_REQUIRE(S, "out of memory");
    S->field = field; S->col_len = col_len; S->arena_bytes = arena_bytes; S->n_bufs = n_bufs;
    S->steps.resize(n_steps);
    std::vector<uint32_t> table;                        // the resident block on the host: every table starts at a multiple of 16 bytes
    Group group;
    char call[96];
    for (size_t i = 0; i < n_steps; i++) {
        const kh_witness_step_t& s = steps[i];
        KH_REQUIRE(s.op >= 0 && s.op < N_OPS, "kh_witness_schedule_create: step %zu: unknown op %d", i, s.op);
        const OpInfo& op = OPS[s.op];
        snprintf(call, sizeof(call), "kh_witness_schedule_create: step %zu (%s)", i, op.name);
        int rc = step_validate(call, field, col_len, s, arena_bytes, n_bufs);
        if (rc) return rc;
        Step& st = S->steps[i];
        st.s = s;
        st.s.rows = nullptr; st.s.cells = nullptr; st.s.consts = nullptr;
        for (int k = op.n_in; k < 3; k++) st.s.in[k] = kh_witness_ref_t{KH_REF_NONE, 0};       // refs the call does not have are ignored, whatever they hold
        for (int k = op.n_out; k < 2; k++) st.s.out[k] = kh_witness_ref_t{KH_REF_NONE, 0};
        if (s.n == 0) continue;                         // the direct call launches nothing
        if (op.n_consts && s.consts) { memcpy(st.consts, s.consts, op.n_consts * sizeof(uint64_t)); st.has_consts = true; }
        if (s.op == KH_STEP_GENERIC) st.generic = generic_fold(field, s.consts);
        if (s.op == KH_STEP_FF_MUL) st.ff_mul = ff_mul_prepare(s.consts);
        const bool wire = op.tabled_cells;
        const kh_witness_ref_t& dense = s.op == KH_STEP_GATHER ? s.out[0] : s.in[0];
        if (wire && dense.buf == KH_REF_ARENA) {        // a fused move per cell
            if (!group.takes(s)) { group.close(); S->launches.push_back(Launch{true, s.op == KH_STEP_SCATTER, i, table.size(), 0}); }
            group.add(s);
            const size_t words = format_bytes(s.format) / 8;
            const uint32_t flag = s.flag_bit == KH_STEP_NO_FLAG ? CELL_MOVE_NO_FLAG : s.flag_bit;
            for (size_t k = 0; k < s.n; k++) {
                const CellMove m = cell_move(s.cells[2 * k], s.cells[2 * k + 1], s.format, flag, dense.offset / 8 + words * k);
                table.insert(table.end(), {m.row, m.meta, m.dense_lo, m.dense_hi});
            }
            S->launches.back().n_moves += s.n;
            continue;
        }
        group.close();
        const uint32_t* const src = wire ? s.cells : s.rows;
        if (src) {
            st.has_table = true; st.table = table.size();
            table.insert(table.end(), src, src + (wire ? 2 : 1) * s.n);
            table.resize((table.size() + 3) & ~(size_t)3);
        }
        S->launches.push_back(Launch{false, false, i, 0, 0});
    }
    int rc = ensure_init(); if (rc) return rc;
    S->device = ctx().device;
    S->resident_bytes = table.size() * sizeof(uint32_t);
    if (!table.empty()) {
        if ((rc = S->resident.reserve(S->resident_bytes))) return rc;
        rc = queue_step([&](Context& C) -> int {        // through the staging ring in pieces that leave it its size, like a direct call's table; then waited for
            const size_t piece = (size_t)1 << 15;
            counter(CNT_TABLE_STAGED_WORDS) += table.size();
            for (size_t i = 0; i < table.size(); i += piece) {
                const int up = C.stage_upload(S->resident.as<uint32_t>() + i, {{table.data() + i, std::min(piece, table.size() - i) * sizeof(uint32_t)}});
                if (up) return up;
            }
            KH_HIP(hipStreamSynchronize(C.stream));
            return KH_OK;
        });
        if (rc) return rc;
    }
    *out = S.release();
    return KH_OK;
}

int kh_witness_schedule_run(const kh_witness_schedule_t* s, void* const* bufs_dev, size_t n_bufs, uint64_t* witness_dev, size_t col_stride, uint32_t* flags_dev) {
    KH_REQUIRE(s, "kh_witness_schedule_run: null schedule");
    KH_REQUIRE(n_bufs == s->n_bufs && (bufs_dev || n_bufs == 0), "kh_witness_schedule_run: %zu buffers at %p, the schedule binds %zu", n_bufs, (const void*)bufs_dev,
               s->n_bufs);
    for (size_t k = 0; k < n_bufs; k++)
        KH_REQUIRE(bufs_dev[k] && (((uintptr_t)bufs_dev[k]) & 15) == 0, "kh_witness_schedule_run: bufs_dev[%zu] = %p must be a 16-byte aligned device address", k,
                   bufs_dev[k]);
    int rc = columns_validate("kh_witness_schedule_run", witness_dev, col_stride, s->col_len, 1);
    if (rc) return rc;
    KH_REQUIRE((((uintptr_t)flags_dev) & 3) == 0, "kh_witness_schedule_run: the flag word at %p is misaligned", (void*)flags_dev);
    DeviceScope on_device(s->device);
    if ((rc = ensure_init())) return rc;
    // what the run owns: the arena and the chain steps' scratch, from the pool (before the context's lock, like kh_lookup_sorted_dev's scratch)
    PoolBlock arena;
    if (s->arena_bytes && (rc = kh_dev_alloc(&arena.p, s->arena_bytes))) return rc;
    size_t n_chain = 0;
    for (const Step& st : s->steps) n_chain += is_chain(st);
    std::vector<PoolBlock> scratch(n_chain);
    std::vector<size_t> scratch_bytes(n_chain);
    n_chain = 0;
    for (const Step& st : s->steps)
        if (is_chain(st)) {
            scratch_bytes[n_chain] = chain_scratch_bytes(st.s.op == KH_STEP_ENDOMUL, st.s.param, st.s.n);
            if ((rc = kh_dev_alloc(&scratch[n_chain].p, scratch_bytes[n_chain]))) return rc;
            n_chain++;
        }
    const uint32_t* const resident = s->resident.as<uint32_t>();
    const int field = s->field;
    return queue_step([&](Context& C) -> int {
        size_t chain = 0;
        for (const Launch& L : s->launches) {
            int r;
            if (L.fused) {
                r = cell_moves(C, field, L.scatter, (const CellMove*)(resident + L.moves), L.n_moves, witness_dev, col_stride, arena.as<uint64_t>(), flags_dev);
                if (r) return r;
                continue;
            }
            const Step& st = s->steps[L.first];
            const kh_witness_step_t& p = st.s;
            const uint32_t* const tab = st.has_table ? resident + st.table : nullptr;
            const WitnessPlace at{tab, p.row0, p.row_stride, witness_dev, col_stride};
            const uint64_t* const in0 = resolve<const uint64_t>(p.in[0], bufs_dev, arena.p);
            const uint64_t* const in1 = resolve<const uint64_t>(p.in[1], bufs_dev, arena.p);
            const uint64_t* const in2 = resolve<const uint64_t>(p.in[2], bufs_dev, arena.p);
            uint64_t* const out0 = resolve<uint64_t>(p.out[0], bufs_dev, arena.p);
            uint64_t* const out1 = resolve<uint64_t>(p.out[1], bufs_dev, arena.p);
            uint32_t* const flags = p.flag_bit == KH_STEP_NO_FLAG ? nullptr : flags_dev;
            const unsigned bit = p.flag_bit == KH_STEP_NO_FLAG ? 0 : p.flag_bit;
            const uint64_t* const consts = st.has_consts ? st.consts : nullptr;
            switch (p.op) {
            case KH_STEP_GATHER: r = cell_gather(C, field, witness_dev, col_stride, tab, p.n, p.format, out0, flags, bit); break;
            case KH_STEP_SCATTER: r = cell_scatter(C, field, in0, p.format, tab, p.n, witness_dev, col_stride, flags, bit); break;
            case KH_STEP_GENERIC: r = generic_rows_prepared(C, field, st.generic, (int)p.param, in0, in1, p.n, at, out0); break;
            case KH_STEP_POSEIDON: r = poseidon_gate_rows(C, field, in0, p.n, at, out0); break;
            case KH_STEP_COMPLETE_ADD: r = complete_add_rows(C, field, in0, in1, p.n, at, out0); break;
            case KH_STEP_VARBASEMUL:
            case KH_STEP_ENDOMUL:
                r = chain_rows(C, field, p.op == KH_STEP_ENDOMUL, consts, in0, in1, in2, p.param, p.n, at, out0, out1, flags, bit, scratch[chain].as<uint64_t>(),
                               scratch_bytes[chain]);
                chain++;
                break;
            case KH_STEP_ENDOMUL_SCALAR: r = endomul_scalar_rows(C, field, in0, p.param, p.n, at, consts, out0); break;
            case KH_STEP_RANGE_CHECK: r = range_check_rows(C, field, in0, p.n, (int)p.param, at, flags, bit); break;
            case KH_STEP_XOR: r = xor_rows(C, field, in0, in1, p.param, p.n, at, out0, flags, bit); break;
            case KH_STEP_ROT64: r = rot64_rows(C, field, in0, p.param, p.n, at, out0); break;
            case KH_STEP_FF_ADD: r = ff_add_rows(C, field, consts, in0, in1, p.sign, p.n, at, out0, flags, bit); break;
            case KH_STEP_FF_MUL: r = ff_mul_rows_prepared(C, field, *st.ff_mul, in0, in1, p.n, at, out0, flags, bit); break;
            default: set_error("kh_witness_schedule_run: step %zu has op %d", L.first, p.op); return KH_E_INVALID;
            }
            if (r) return r;
        }
        return KH_OK;
    });
}

int kh_witness_schedule_info(const kh_witness_schedule_t* s, size_t* steps, size_t* launch_groups, size_t* resident_bytes, size_t* run_bytes) {
    KH_REQUIRE(s, "kh_witness_schedule_info: null schedule");
    if (steps) *steps = s->steps.size();
    if (launch_groups) *launch_groups = s->launches.size();
    if (resident_bytes) *resident_bytes = s->resident_bytes;
    if (run_bytes) {
        *run_bytes = s->arena_bytes;
        for (const Step& st : s->steps)
            if (is_chain(st)) *run_bytes += chain_scratch_bytes(st.s.op == KH_STEP_ENDOMUL, st.s.param, st.s.n);
    }
    return KH_OK;
}

void kh_witness_schedule_free(kh_witness_schedule_t* s) {
    if (!s) return;
    DeviceScope on_device(s->device);
    delete s;                                           // (the resident block's hipFree waits for the device: no queued run still reads it)
}

}  // extern "C"
