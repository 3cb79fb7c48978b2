// witness_schedule.cpp -- kh_witness_schedule_*: the list of gadget and wire calls that writes a circuit's witness, compiled once and run per proof.
// Create does what depends on the circuit alone: every step becomes the record of its direct call (StepArgs; witness_steps.cpp) with stand-in
// pointers that carry the refs' nullness and alignment and goes through step_validate and step_prepare, the rows[] / cells tables go into one
// resident device block, and consecutive wire steps over the arena are merged into groups of one launch each (wiring.hip: k_cell_moves).
// A run resolves the refs against this run's buffers and arena and hands each record to step_launch, as a direct call does, under one hold of the
// context's lock: O(steps) host work, nothing staged, nothing validated per cell.
#include <string.h>
#include <iterator>
#include <unordered_set>

#include "api_internal.hpp"

using namespace kh;

namespace {
size_t format_bytes(int format) { return format == KH_CELL_FIELD || format == KH_CELL_INT256 ? 32 : format == KH_CELL_U64 ? 8 : 16; }

struct Step {
    StepArgs a;                               // what no run changes; every pointer is null here: the tables are resident, the constants below, the rest per run
    kh_witness_ref_t in[3], out[2];
    bool flagged = false;                     // the run's flags_dev is the step's
    size_t table = 0;                         // word offset of the step's rows[] / cells in the resident block
    bool has_table = false, has_consts = false;
    int scratch = -1;                         // which of the run's scratch blocks is the step's (VarBaseMul / EndoMul / Lookup), or none
    uint64_t consts[20];
    StepPrepared prepared;
};
// one launcher invocation of a run: a step, or a group of wire steps [first, last] as n_moves records at word offset `moves`
struct Launch { bool fused, scatter; size_t first, moves, n_moves; };

// the stand-in of a ref for step_validate: null when absent, else an address with the ref's alignment (a bound buffer and the arena
// are 16-byte aligned: kh_witness_schedule_run checks the buffers, the pool aligns the arena)
void* stand_in(const kh_witness_ref_t& r) { return r.buf == KH_REF_NONE ? nullptr : (void*)(uintptr_t)(4096 + (r.offset & 4095)); }
}  // namespace

struct kh_witness_schedule {
    int field = 0, device = -1;
    size_t col_len = 0, arena_bytes = 0, n_bufs = 0, resident_bytes = 0, n_scratch = 0;
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

// the refs of step `call` that its op has, against the arena (after the call's own list: n is known to be small enough for the extents, the format to be one).
// An input that is a table (OpInfo::table_in: the Lookup step's two columns) extends over `param` elements, whatever n is; an output of `param`
// elements per instance (OpInfo::param_out: the bits of BITS) over n * param of them.
int refs_validate(const char* call, const OpInfo& op, const kh_witness_step_t& s, size_t arena_bytes, size_t n_bufs) {
    const size_t cell_bytes = format_bytes(s.format);                // (for the refs whose size the format decides: GATHER / SCATTER, the input of BITS)
    int rc;
    for (int k = 0; k < op.n_in; k++)
        if ((rc = ref_validate(call, "in", k, s.in[k], op.in_bytes[k] ? op.in_bytes[k] : cell_bytes, (op.table_in >> k & 1) ? (size_t)s.param : s.n, arena_bytes, n_bufs)))
            return rc;
    for (int k = 0; k < op.n_out; k++)
        if ((rc = ref_validate(call, "out", k, s.out[k], (op.out_bytes[k] ? op.out_bytes[k] : cell_bytes) * ((op.param_out >> k & 1) ? (size_t)s.param : 1), s.n, arena_bytes,
                               n_bufs)))
            return rc;
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

void* resolve(const kh_witness_ref_t& r, void* const* bufs, void* arena) {
    if (r.buf == KH_REF_NONE) return nullptr;
    return (char*)(r.buf == KH_REF_ARENA ? arena : bufs[r.buf]) + r.offset;
}
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
        KH_REQUIRE(step_op(s.op), "kh_witness_schedule_create: step %zu: unknown op %d", i, s.op);
        const OpInfo& op = *step_op(s.op);
        snprintf(call, sizeof(call), "kh_witness_schedule_create: step %zu (%s)", i, op.name);
        KH_REQUIRE(s.flag_bit < 32 || s.flag_bit == KH_STEP_NO_FLAG, "%s: flag_bit %u is neither below 32 nor KH_STEP_NO_FLAG", call, s.flag_bit);
        Step& st = S->steps[i];
        st.flagged = s.flag_bit != KH_STEP_NO_FLAG;
        const StepArgs a{s.op, s.n, {s.rows, s.row0, s.row_stride, (uint64_t*)(uintptr_t)4096, col_len}, {stand_in(s.in[0]), stand_in(s.in[1]), stand_in(s.in[2])},
                         {stand_in(s.out[0]), stand_in(s.out[1])}, s.param, s.consts, st.flagged ? (uint32_t*)(uintptr_t)4096 : nullptr,
                         st.flagged ? s.flag_bit : 0, s.sign, s.cells, s.format};
        int rc = step_validate(call, field, col_len, a);
        if (rc || (rc = refs_validate(call, op, s, arena_bytes, n_bufs))) return rc;
        st.a = StepArgs{s.op, s.n, {nullptr, s.row0, s.row_stride, nullptr, 0}, {}, {}, s.param, nullptr, nullptr, a.bit, s.sign, nullptr, s.format};
        for (int k = 0; k < 3; k++) st.in[k] = k < op.n_in ? s.in[k] : kh_witness_ref_t{KH_REF_NONE, 0};        // refs the call does not have are ignored, whatever they hold
        for (int k = 0; k < 2; k++) st.out[k] = k < op.n_out ? s.out[k] : kh_witness_ref_t{KH_REF_NONE, 0};
        if (s.n == 0) continue;                         // the direct call launches nothing
        if (op.n_consts && s.consts) { memcpy(st.consts, s.consts, op.n_consts * sizeof(uint64_t)); st.has_consts = true; }
        st.prepared = step_prepare(field, a);
        if (step_scratch_bytes(a)) st.scratch = (int)S->n_scratch++;
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
        const uint32_t* const src = op.value ? nullptr : wire ? s.cells : s.rows;        // (a value step has no placement: its rows are ignored)
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
        rc = queue_step([&](Context& C) -> int {        // through the staging ring like a direct call's table; then waited for
            const int up = stage_words(C, S->resident.as<uint32_t>(), table.data(), table.size());
            if (up) return up;
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
    // what the run owns: the arena, the chain steps' scratch and the Lookup steps' slots, from the pool (before the context's lock, like kh_lookup_sorted_dev's scratch)
    PoolBlock arena;
    if (s->arena_bytes && (rc = kh_dev_alloc(&arena.p, s->arena_bytes))) return rc;
    std::vector<PoolBlock> scratch(s->n_scratch);
    std::vector<size_t> scratch_bytes(s->n_scratch);
    for (const Step& st : s->steps)
        if (st.scratch >= 0) {
            scratch_bytes[st.scratch] = step_scratch_bytes(st.a);
            if ((rc = kh_dev_alloc(&scratch[st.scratch].p, scratch_bytes[st.scratch]))) return rc;
        }
    const uint32_t* const resident = s->resident.as<uint32_t>();
    const int field = s->field;
    return queue_step([&](Context& C) -> int {
        for (const Launch& L : s->launches) {
            int r;
            if (L.fused) {
                r = cell_moves(C, field, L.scatter, (const CellMove*)(resident + L.moves), L.n_moves, witness_dev, col_stride, arena.as<uint64_t>(), flags_dev);
                if (r) return r;
                continue;
            }
            const Step& st = s->steps[L.first];
            StepArgs a = st.a;
            (step_op(a.op)->tabled_cells ? a.cells : a.at.rows) = st.has_table ? resident + st.table : nullptr;
            a.at.witness = witness_dev; a.at.col_stride = col_stride;
            for (int k = 0; k < 3; k++) a.in[k] = resolve(st.in[k], bufs_dev, arena.p);
            for (int k = 0; k < 2; k++) a.out[k] = resolve(st.out[k], bufs_dev, arena.p);
            a.consts = st.has_consts ? st.consts : nullptr;
            a.flags = st.flagged ? flags_dev : nullptr;
            const int k = st.scratch;
            r = step_launch(C, field, a, st.prepared, k < 0 ? nullptr : scratch[k].as<uint64_t>(), k < 0 ? 0 : scratch_bytes[k]);
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
        for (const Step& st : s->steps) *run_bytes += step_scratch_bytes(st.a);
    }
    return KH_OK;
}

void kh_witness_schedule_free(kh_witness_schedule_t* s) {
    if (!s) return;
    DeviceScope on_device(s->device);
    delete s;                                           // (the resident block's hipFree waits for the device: no queued run still reads it)
}

}  // extern "C"
