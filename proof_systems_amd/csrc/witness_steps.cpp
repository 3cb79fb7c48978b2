// witness_steps.cpp -- the gadget, wire and value steps (kh_*_witness_dev, kh_lookup_witness_dev, kh_witness_gather_dev, kh_witness_scatter_dev, kh_field_*_dev): the one list of them.  A step is a
// StepArgs record (api_internal.hpp); OPS[] says what each op takes, step_validate what it refuses, step_prepare what it computes on the host,
// step_launch which launcher it runs.  A direct call fills the record from its arguments and goes through direct_step; a witness schedule
// (witness_schedule.cpp) fills it from a kh_witness_step_t and goes through the same three functions, so the two cannot differ.
#include <string.h>

#include "api_internal.hpp"

using namespace kh;

namespace {
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
    {nullptr, 0, 0, {0, 0, 0}, {0, 0}, false, 0},                   // 13: unassigned (include/kimchi_hip.h), refused as an unknown op
    {"KH_STEP_LOOKUP", 3, 1, {96, 32, 32}, {96, 0}, false, 4, 6},    // in[1], in[2]: the table's two columns, `param` elements each
    {"KH_STEP_INVERSE", 1, 1, {32, 0, 0}, {32, 0}, false, 0, 0, 0, true},
    {"KH_STEP_SQRT", 1, 2, {32, 0, 0}, {32, 32}, false, 0, 0, 0, true},
    {"KH_STEP_BITS", 1, 1, {0, 0, 0}, {32, 0}, false, 0, 0, 1, true},    // in[0]: the format decides; out[0]: `param` = num_bits elements per instance
};
constexpr int N_OPS = sizeof(OPS) / sizeof(OPS[0]);

// what a placement (WitnessPlace, rows still on the host) is refused for: its columns, instances of inst_rows rows that do not fit col_len rows
int place_validate(const char* call, const WitnessPlace& at, size_t n, size_t col_len, size_t inst_rows) {
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
// the field, null / misaligned device pointers
int pointers_validate(const char* call, int field, std::initializer_list<GadgetPtr> ptrs, size_t n) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "%s: unknown field id %d", call, field);
    for (const GadgetPtr& p : ptrs) {
        KH_REQUIRE(p.p || !p.required || n == 0, "%s: null %s", call, p.name);
        KH_REQUIRE((((uintptr_t)p.p) & (p.align - 1)) == 0, "%s: %s must be %u-byte aligned", call, p.name, p.align);
    }
    return KH_OK;
}
// what the gadget calls refuse alike: the field, null / misaligned device pointers, a placement that does not hold
int gadget_validate(const char* call, int field, std::initializer_list<GadgetPtr> ptrs, const StepArgs& a, size_t col_len, size_t inst_rows) {
    int rc = pointers_validate(call, field, ptrs, a.n);
    if (rc) return rc;
    return place_validate(call, a.at, a.n, col_len, inst_rows);
}
// a flag word that is misaligned or a bit that is not one
int flag_validate(const char* call, const StepArgs& a) {
    KH_REQUIRE(a.bit < 32 && (((uintptr_t)a.flags) & 3) == 0, "%s: flag bit %u of a word at %p", call, a.bit, (const void*)a.flags);
    return KH_OK;
}
// what the value calls refuse alike: the same pointer checks with no placement, more elements than a grid of one lane each takes, the flag
int value_validate(const char* call, int field, std::initializer_list<GadgetPtr> ptrs, const StepArgs& a) {
    int rc = pointers_validate(call, field, ptrs, a.n);
    if (rc) return rc;
    KH_REQUIRE(a.n <= WAVE_BLOCK_MAX_N, "%s: %zu elements overflow the grid", call, a.n);
    return flag_validate(call, a);
}
// what the five limb gadgets refuse alike after their own arguments: gadget_validate's list, more lanes (one per instance and row) than a grid takes, the
// flag
int limb_validate(const char* call, int field, std::initializer_list<GadgetPtr> ptrs, const StepArgs& a, size_t col_len, size_t inst_rows) {
    int rc = gadget_validate(call, field, ptrs, a, col_len, inst_rows);
    if (rc) return rc;
    KH_REQUIRE(a.n <= WAVE_BLOCK_MAX_N / inst_rows, "%s: %zu instances of %zu rows overflow the byte count", call, a.n, inst_rows);
    return flag_validate(call, a);
}
// a foreign modulus: three limbs of two u64 on the host, each < 2^88, not all zero
int modulus_validate(const char* call, const uint64_t* modulus, size_t n) {
    KH_REQUIRE(modulus || n == 0, "%s: null modulus", call);
    if (!modulus) return KH_OK;
    KH_REQUIRE((modulus[1] | modulus[3] | modulus[5]) >> 24 == 0, "%s: a modulus limb is 2^88 or more", call);
    KH_REQUIRE((modulus[0] | modulus[1] | modulus[2] | modulus[3] | modulus[4] | modulus[5]) != 0, "%s: the modulus is zero", call);
    return KH_OK;
}
}  // namespace

namespace kh {
const OpInfo* step_op(int op) { return op >= 0 && op < N_OPS && OPS[op].name ? &OPS[op] : nullptr; }

// each call's own list, in the order the call has always checked it
int step_validate(const char* call, int field, size_t col_len, const StepArgs& a) {
    const void* const* in = a.in;
    void* const* out = a.out;
    const size_t n = a.n;
    int rc;
    switch (a.op) {
    case KH_STEP_GATHER:
    case KH_STEP_SCATTER: {
        // the two cell calls: the field and the format, their columns, the dense buffer (aligned to its format's access), the flag word, a cell outside
        // the 15 columns of col_len rows
        const char* const data_name = OPS[a.op].n_out ? "out_dev" : "values_dev";
        const void* const data = OPS[a.op].n_out ? out[0] : in[0];
        KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "%s: unknown field id %d", call, field);
        KH_REQUIRE(a.format >= KH_CELL_FIELD && a.format <= KH_CELL_U64, "%s: unknown cell format %d", call, a.format);
        if ((rc = columns_validate(call, a.at.witness, a.at.col_stride, col_len, n))) return rc;
        const unsigned align = a.format == KH_CELL_U64 ? 8 : 16;
        KH_REQUIRE((a.cells && data) || n == 0, "%s: null %s", call, a.cells ? data_name : "cells");
        KH_REQUIRE((((uintptr_t)data) & (align - 1)) == 0, "%s: %s must be %u-byte aligned", call, data_name, align);
        if ((rc = flag_validate(call, a))) return rc;
        for (size_t i = 0; i < n; i++)
            KH_REQUIRE(a.cells[2 * i] < col_len && a.cells[2 * i + 1] < 15, "%s: cell %zu at (row %u, column %u) is outside the 15 columns of %zu rows", call, i,
                       a.cells[2 * i], a.cells[2 * i + 1], col_len);
        return KH_OK;
    }
    case KH_STEP_GENERIC:
        KH_REQUIRE((int)a.param == 0 || (int)a.param == 1, "%s: half is %d, not 0 or 1", call, (int)a.param);
        if ((rc = gadget_validate(call, field, {{"l_dev", in[0], true}, {"r_dev", in[1], false}, {"out_dev", out[0], false}}, a, col_len, 1))) return rc;
        KH_REQUIRE(a.consts || n == 0, "%s: null coeffs", call);
        return KH_OK;
    case KH_STEP_POSEIDON:
        return gadget_validate(call, field, {{"states_dev", in[0], true}, {"out_states_dev", out[0], false}}, a, col_len, 12);
    case KH_STEP_COMPLETE_ADD:
        return gadget_validate(call, field, {{"p1_dev", in[0], true}, {"p2_dev", in[1], true}, {"out_dev", out[0], false}}, a, col_len, 1);
    case KH_STEP_VARBASEMUL:                 // VarBaseMul (scalars of 4 limbs) and EndoMul (challenges of 2 limbs) share everything but their row counts
    case KH_STEP_ENDOMUL: {
        const bool is_endo = a.op == KH_STEP_ENDOMUL;
        const unsigned num_bits = a.param;
        if (is_endo) KH_REQUIRE(num_bits >= 4 && num_bits <= 128 && num_bits % 4 == 0, "%s: num_bits %u is not a multiple of 4 from 4 to 128", call, num_bits);
        else KH_REQUIRE(num_bits >= 5 && num_bits <= 255 && num_bits % 5 == 0, "%s: num_bits %u is not a multiple of 5 from 5 to 255", call, num_bits);
        rc = gadget_validate(call, field, {{"base_dev", in[0], true}, {"acc0_dev", in[1], true}, {is_endo ? "chals_dev" : "scalars_dev", in[2], true},
                             {"out_acc_dev", out[0], false}, {"out_n_dev", out[1], false}},
                             a, col_len, is_endo ? num_bits / 4 + 1 : 2 * num_bits / 5);
        if (rc) return rc;
        KH_REQUIRE(!is_endo || a.consts || n == 0, "%s: null endo", call);
        return flag_validate(call, a);
    }
    case KH_STEP_ENDOMUL_SCALAR:
        KH_REQUIRE(a.param >= 16 && a.param <= 128 && a.param % 16 == 0, "%s: num_bits %u is not a multiple of 16 from 16 to 128", call, a.param);
        if ((rc = gadget_validate(call, field, {{"chals_dev", in[0], true}, {"out_dev", out[0], false}}, a, col_len, a.param / 16))) return rc;
        KH_REQUIRE(a.consts || !out[0] || n == 0, "%s: null endo_scalar with an out_dev", call);
        return KH_OK;
    case KH_STEP_RANGE_CHECK:
        KH_REQUIRE((int)a.param == 0 || (int)a.param == 1, "%s: compact is %d, not 0 or 1", call, (int)a.param);
        return limb_validate(call, field, {{"limbs_dev", in[0], true}}, a, col_len, 4);
    case KH_STEP_XOR:
        KH_REQUIRE(a.param >= 1 && a.param <= 254, "%s: bits %u is not from 1 to 254", call, a.param);
        return limb_validate(call, field, {{"in1_dev", in[0], true}, {"in2_dev", in[1], true}, {"out_dev", out[0], false}}, a, col_len, (a.param + 15) / 16 + 1);
    case KH_STEP_ROT64:
        KH_REQUIRE(a.param <= 63, "%s: rot %u is not from 0 to 63", call, a.param);
        return limb_validate(call, field, {{"words_dev", in[0], true, 8}, {"out_dev", out[0], false, 8}}, a, col_len, 3);
    case KH_STEP_FF_ADD:
        KH_REQUIRE(a.sign == 1 || a.sign == -1, "%s: sign is %d, not +1 or -1", call, a.sign);
        if ((rc = modulus_validate(call, a.consts, n))) return rc;
        return limb_validate(call, field, {{"left_dev", in[0], true}, {"right_dev", in[1], true}, {"out_dev", out[0], false}}, a, col_len, 2);
    case KH_STEP_FF_MUL:
        if ((rc = modulus_validate(call, a.consts, n))) return rc;
        return limb_validate(call, field, {{"a_dev", in[0], true}, {"b_dev", in[1], true}, {"out_checks_dev", out[0], false}}, a, col_len, 2);
    case KH_STEP_LOOKUP: {
        // gadget_validate's list for an instance of ONE row; the table id; the table's length and columns; one lane per (slot, instance); the flag
        if ((rc = gadget_validate(call, field, {{"keys_dev", in[0], true}, {"out_values_dev", out[0], false}}, a, col_len, 1))) return rc;
        KH_REQUIRE(a.consts || n == 0, "%s: null table_id", call);
        khost::fe id{{0, 0, 0, 0}};
        if (a.consts) memcpy(id.l, a.consts, sizeof(id.l));
        KH_REQUIRE(!khost::geq(id, khost::Fld(field).f.p), "%s: table_id is not a canonical field element (>= p)", call);
        KH_REQUIRE(a.param >= 1 && a.param < (1u << 31), "%s: table_len %u is not from 1 to 2^31 - 1", call, a.param);
        for (const GadgetPtr& p : {GadgetPtr{"table_keys_dev", in[1], true}, GadgetPtr{"table_values_dev", in[2], true}}) {
            KH_REQUIRE(p.p || n == 0, "%s: null %s", call, p.name);
            KH_REQUIRE((((uintptr_t)p.p) & 15) == 0, "%s: %s must be 16-byte aligned", call, p.name);
        }
        KH_REQUIRE(n <= WAVE_BLOCK_MAX_N / 3, "%s: %zu instances of 3 lookups overflow the grid", call, n);
        return flag_validate(call, a);
    }
    case KH_STEP_INVERSE:
        return value_validate(call, field, {{"in_dev", in[0], true}, {"out_dev", out[0], true}}, a);
    case KH_STEP_SQRT:
        return value_validate(call, field, {{"in_dev", in[0], true}, {"out_dev", out[0], true}, {"out_is_square_dev", out[1], false}}, a);
    case KH_STEP_BITS: {
        // the field and the format first: the format decides the input's alignment and how many bits it has
        KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "%s: unknown field id %d", call, field);
        KH_REQUIRE(a.format >= KH_CELL_FIELD && a.format <= KH_CELL_U64, "%s: unknown cell format %d", call, a.format);
        const unsigned words = a.format == KH_CELL_FIELD || a.format == KH_CELL_INT256 ? 4 : a.format == KH_CELL_U64 ? 1 : 2;
        KH_REQUIRE(a.param >= 1 && a.param <= 255, "%s: num_bits %u is not from 1 to 255", call, a.param);
        KH_REQUIRE(a.param <= 64 * words, "%s: num_bits %u is more than the %u bits of cell format %d", call, a.param, 64 * words, a.format);
        return value_validate(call, field, {{"in_dev", in[0], true, a.format == KH_CELL_U64 ? 8u : 16u}, {"out_dev", out[0], true}}, a);
    }
    }
    set_error("%s: unknown op %d", call, a.op);
    return KH_E_INVALID;
}

StepPrepared step_prepare(int field, const StepArgs& a) {
    StepPrepared p{};
    if (a.op == KH_STEP_GENERIC) p.generic = generic_fold(field, a.consts);
    if (a.op == KH_STEP_FF_MUL) p.ff_mul = ff_mul_prepare(a.consts);
    return p;
}

size_t step_scratch_bytes(const StepArgs& a) {
    if (a.op == KH_STEP_LOOKUP) return a.n > 0 ? lookup_rows_slot_bytes(a.param) : 0;
    return (a.op == KH_STEP_VARBASEMUL || a.op == KH_STEP_ENDOMUL) && a.n > 0 ? chain_scratch_bytes(a.op == KH_STEP_ENDOMUL, a.param, a.n) : 0;
}

int step_launch(Context& C, int field, const StepArgs& a, const StepPrepared& prepared, uint64_t* scratch_dev, size_t scratch_bytes) {
    const uint64_t* const in0 = (const uint64_t*)a.in[0];
    const uint64_t* const in1 = (const uint64_t*)a.in[1];
    const uint64_t* const in2 = (const uint64_t*)a.in[2];
    uint64_t* const out0 = (uint64_t*)a.out[0];
    uint64_t* const out1 = (uint64_t*)a.out[1];
    switch (a.op) {
    case KH_STEP_GATHER: return cell_gather(C, field, a.at.witness, a.at.col_stride, a.cells, a.n, a.format, out0, a.flags, a.bit);
    case KH_STEP_SCATTER: return cell_scatter(C, field, in0, a.format, a.cells, a.n, a.at.witness, a.at.col_stride, a.flags, a.bit);
    case KH_STEP_GENERIC: return generic_rows_prepared(C, field, prepared.generic, (int)a.param, in0, in1, a.n, a.at, out0);
    case KH_STEP_POSEIDON: return poseidon_gate_rows(C, field, in0, a.n, a.at, out0);
    case KH_STEP_COMPLETE_ADD: return complete_add_rows(C, field, in0, in1, a.n, a.at, out0);
    case KH_STEP_VARBASEMUL:
    case KH_STEP_ENDOMUL:
        return chain_rows(C, field, a.op == KH_STEP_ENDOMUL, a.consts, in0, in1, in2, a.param, a.n, a.at, out0, out1, a.flags, a.bit, scratch_dev, scratch_bytes);
    case KH_STEP_ENDOMUL_SCALAR: return endomul_scalar_rows(C, field, in0, a.param, a.n, a.at, a.consts, out0);
    case KH_STEP_RANGE_CHECK: return range_check_rows(C, field, in0, a.n, (int)a.param, a.at, a.flags, a.bit);
    case KH_STEP_XOR: return xor_rows(C, field, in0, in1, a.param, a.n, a.at, out0, a.flags, a.bit);
    case KH_STEP_ROT64: return rot64_rows(C, field, in0, a.param, a.n, a.at, out0);
    case KH_STEP_FF_ADD: return ff_add_rows(C, field, a.consts, in0, in1, a.sign, a.n, a.at, out0, a.flags, a.bit);
    case KH_STEP_FF_MUL: return ff_mul_rows_prepared(C, field, *prepared.ff_mul, in0, in1, a.n, a.at, out0, a.flags, a.bit);
    case KH_STEP_LOOKUP: return lookup_rows(C, a.consts, in1, in2, a.param, in0, a.n, a.at, out0, a.flags, a.bit, (uint32_t*)scratch_dev, scratch_bytes);
    case KH_STEP_INVERSE: return field_inverse(C, field, in0, a.n, out0, a.flags, a.bit);
    case KH_STEP_SQRT: return field_sqrt(C, field, in0, a.n, out0, out1, a.flags, a.bit);
    case KH_STEP_BITS: return field_bits(C, field, in0, a.format, a.param, a.n, out0, a.flags, a.bit);
    }
    set_error("step_launch: unknown op %d", a.op);
    return KH_E_INVALID;
}
}  // namespace kh

namespace {
// A direct call.  Arguments first, before anything touches the device; the host-side constants; then what the call takes from the kh_dev_alloc pool
// (before the context's lock, like kh_lookup_sorted_dev's scratch: the pool may order this context behind a block's previous owner) -- the chain
// steps' scratch or the Lookup step's slots, and a block for the host table (start rows, or cells; nullable) --; then, under one hold of the lock, the table through the staging
// ring and the launch with the table on the device.  The caller's arrays are not read after this returns, and nothing waits for the device.
int direct_step(const char* call, int field, size_t col_len, StepArgs a) {
    int rc = step_validate(call, field, col_len, a);
    if (rc) return rc;
    if (a.n == 0) return ensure_init();
    const StepPrepared prepared = step_prepare(field, a);
    PoolBlock scratch, table_dev;
    const size_t scratch_bytes = step_scratch_bytes(a);
    if (scratch_bytes && (rc = kh_dev_alloc(&scratch.p, scratch_bytes))) return rc;
    const uint32_t*& table = OPS[a.op].tabled_cells ? a.cells : a.at.rows;
    const size_t words = (OPS[a.op].tabled_cells ? 2 : 1) * a.n;
    if (table && (rc = kh_dev_alloc(&table_dev.p, words * sizeof(uint32_t)))) return rc;
    return queue_step([&](Context& C) {
        if (table) {
            const int up = stage_words(C, table_dev.as<uint32_t>(), table, words);
            if (up) return up;
            table = table_dev.as<uint32_t>();
        }
        return step_launch(C, field, a, prepared, scratch.as<uint64_t>(), scratch_bytes);
    });
}
}  // namespace

extern "C" {

// ---------------------------------------------------------------------------------- gadget witnesses on the device (kernels in poseidon.hip, curve_gadgets.hip)
int kh_poseidon_gate_witness_dev(int field, const uint64_t* states_dev, size_t n, const uint32_t* rows, size_t row0, size_t row_stride,
                                 uint64_t* witness_dev, size_t col_stride, size_t col_len, uint64_t* out_states_dev) {
    return direct_step("kh_poseidon_gate_witness_dev", field, col_len,
                       {KH_STEP_POSEIDON, n, {rows, row0, row_stride, witness_dev, col_stride}, {states_dev}, {out_states_dev}});
}
int kh_complete_add_witness_dev(int field, const uint64_t* p1_dev, const uint64_t* p2_dev, size_t n, const uint32_t* rows, size_t row0, size_t row_stride,
                                uint64_t* witness_dev, size_t col_stride, size_t col_len, uint64_t* out_dev) {
    return direct_step("kh_complete_add_witness_dev", field, col_len,
                       {KH_STEP_COMPLETE_ADD, n, {rows, row0, row_stride, witness_dev, col_stride}, {p1_dev, p2_dev}, {out_dev}});
}
int kh_endomul_scalar_witness_dev(int field, const uint64_t* chals_dev, unsigned num_bits, size_t n, const uint32_t* rows, size_t row0, size_t row_stride,
                                  uint64_t* witness_dev, size_t col_stride, size_t col_len, const uint64_t endo_scalar[4], uint64_t* out_dev) {
    return direct_step("kh_endomul_scalar_witness_dev", field, col_len,
                       {KH_STEP_ENDOMUL_SCALAR, n, {rows, row0, row_stride, witness_dev, col_stride}, {chals_dev}, {out_dev}, num_bits, endo_scalar});
}
int kh_varbasemul_witness_dev(int field, const uint64_t* base_dev, const uint64_t* acc0_dev, const uint64_t* scalars_dev, unsigned num_bits, size_t n,
                              const uint32_t* rows, size_t row0, size_t row_stride, uint64_t* witness_dev, size_t col_stride, size_t col_len,
                              uint64_t* out_acc_dev, uint64_t* out_n_dev, uint32_t* flags_dev, unsigned bit) {
    return direct_step("kh_varbasemul_witness_dev", field, col_len,
                       {KH_STEP_VARBASEMUL, n, {rows, row0, row_stride, witness_dev, col_stride}, {base_dev, acc0_dev, scalars_dev}, {out_acc_dev, out_n_dev}, num_bits,
                        nullptr, flags_dev, bit});
}
int kh_endomul_witness_dev(int field, const uint64_t endo[4], const uint64_t* base_dev, const uint64_t* acc0_dev, const uint64_t* chals_dev, unsigned num_bits,
                           size_t n, const uint32_t* rows, size_t row0, size_t row_stride, uint64_t* witness_dev, size_t col_stride, size_t col_len,
                           uint64_t* out_acc_dev, uint64_t* out_n_dev, uint32_t* flags_dev, unsigned bit) {
    return direct_step("kh_endomul_witness_dev", field, col_len,
                       {KH_STEP_ENDOMUL, n, {rows, row0, row_stride, witness_dev, col_stride}, {base_dev, acc0_dev, chals_dev}, {out_acc_dev, out_n_dev}, num_bits, endo,
                        flags_dev, bit});
}
int kh_curve_witness_set_slice_elements(size_t elements) { chain_set_slice_elements(elements); return KH_OK; }

// ---------------------------------------------------------------------------------- the optional gates' witnesses (kernels in limb_gadgets.hip)
int kh_foreign_field_gate_coefficients(int field, const uint64_t modulus[6], uint64_t* out) {
    KH_REQUIRE(field == KH_FIELD_FP || field == KH_FIELD_FQ, "kh_foreign_field_gate_coefficients: unknown field id %d", field);
    KH_REQUIRE(out, "kh_foreign_field_gate_coefficients: null output");
    int rc = modulus_validate("kh_foreign_field_gate_coefficients", modulus, 1);
    if (rc) return rc;
    uint64_t nf[6];
    ff_negated_modulus(modulus, nf);
    const khost::Fld F(field);
    const uint64_t* const src[7] = {modulus + 4, nf, nf + 2, nf + 4, modulus, modulus + 2, modulus + 4};       // f2 nf0 nf1 nf2 | f0 f1 f2
    for (size_t k = 0; k < 7; k++) {
        const khost::fe v = F.to_mont(khost::fe{{src[k][0], src[k][1], 0, 0}});
        memcpy(out + 4 * k, v.l, 32);
    }
    return KH_OK;
}
int kh_range_check_witness_dev(int field, const uint64_t* limbs_dev, size_t n, int compact, const uint32_t* rows, size_t row0, size_t row_stride,
                               uint64_t* witness_dev, size_t col_stride, size_t col_len, uint32_t* flags_dev, unsigned bit) {
    return direct_step("kh_range_check_witness_dev", field, col_len,
                       {KH_STEP_RANGE_CHECK, n, {rows, row0, row_stride, witness_dev, col_stride}, {limbs_dev}, {}, (unsigned)compact, nullptr, flags_dev, bit});
}
int kh_xor_witness_dev(int field, const uint64_t* in1_dev, const uint64_t* in2_dev, unsigned bits, size_t n, const uint32_t* rows, size_t row0,
                       size_t row_stride, uint64_t* witness_dev, size_t col_stride, size_t col_len, uint64_t* out_dev, uint32_t* flags_dev, unsigned bit) {
    return direct_step("kh_xor_witness_dev", field, col_len,
                       {KH_STEP_XOR, n, {rows, row0, row_stride, witness_dev, col_stride}, {in1_dev, in2_dev}, {out_dev}, bits, nullptr, flags_dev, bit});
}
int kh_rot64_witness_dev(int field, const uint64_t* words_dev, unsigned rot, size_t n, const uint32_t* rows, size_t row0, size_t row_stride,
                         uint64_t* witness_dev, size_t col_stride, size_t col_len, uint64_t* out_dev) {
    return direct_step("kh_rot64_witness_dev", field, col_len, {KH_STEP_ROT64, n, {rows, row0, row_stride, witness_dev, col_stride}, {words_dev}, {out_dev}, rot});
}
int kh_foreign_field_add_witness_dev(int field, const uint64_t modulus[6], const uint64_t* left_dev, const uint64_t* right_dev, int sign, size_t n,
                                     const uint32_t* rows, size_t row0, size_t row_stride, uint64_t* witness_dev, size_t col_stride, size_t col_len,
                                     uint64_t* out_dev, uint32_t* flags_dev, unsigned bit) {
    return direct_step("kh_foreign_field_add_witness_dev", field, col_len,
                       {KH_STEP_FF_ADD, n, {rows, row0, row_stride, witness_dev, col_stride}, {left_dev, right_dev}, {out_dev}, 0, modulus, flags_dev, bit, sign});
}
int kh_foreign_field_mul_witness_dev(int field, const uint64_t modulus[6], const uint64_t* a_dev, const uint64_t* b_dev, size_t n, const uint32_t* rows,
                                     size_t row0, size_t row_stride, uint64_t* witness_dev, size_t col_stride, size_t col_len, uint64_t* out_checks_dev,
                                     uint32_t* flags_dev, unsigned bit) {
    return direct_step("kh_foreign_field_mul_witness_dev", field, col_len,
                       {KH_STEP_FF_MUL, n, {rows, row0, row_stride, witness_dev, col_stride}, {a_dev, b_dev}, {out_checks_dev}, 0, modulus, flags_dev, bit});
}

// ---------------------------------------------------------------------------------- GateType::Lookup rows (kernels in lookup_rows.hip)
int kh_lookup_witness_dev(int field, const uint64_t table_id[4], const uint64_t* table_keys_dev, const uint64_t* table_values_dev, size_t table_len,
                          const uint64_t* keys_dev, size_t n, const uint32_t* rows, size_t row0, size_t row_stride, uint64_t* witness_dev, size_t col_stride,
                          size_t col_len, uint64_t* out_values_dev, uint32_t* flags_dev, unsigned bit) {
    const unsigned len = table_len < ((size_t)1 << 31) ? (unsigned)table_len : 1u << 31;        // (a step's param is 32 bits: every refused length as one refused value)
    return direct_step("kh_lookup_witness_dev", field, col_len,
                       {KH_STEP_LOOKUP, n, {rows, row0, row_stride, witness_dev, col_stride}, {keys_dev, table_keys_dev, table_values_dev}, {out_values_dev}, len,
                        table_id, flags_dev, bit});
}

// ---------------------------------------------------------------------------------- advice values (kernels in value_steps.hip): no witness, no placement
int kh_field_inverse_dev(int field, const uint64_t* in_dev, size_t n, uint64_t* out_dev, uint32_t* flags_dev, unsigned bit) {
    return direct_step("kh_field_inverse_dev", field, 0, {KH_STEP_INVERSE, n, {}, {in_dev}, {out_dev}, 0, nullptr, flags_dev, bit});
}
int kh_field_sqrt_dev(int field, const uint64_t* in_dev, size_t n, uint64_t* out_dev, uint64_t* out_is_square_dev, uint32_t* flags_dev, unsigned bit) {
    return direct_step("kh_field_sqrt_dev", field, 0, {KH_STEP_SQRT, n, {}, {in_dev}, {out_dev, out_is_square_dev}, 0, nullptr, flags_dev, bit});
}
int kh_field_bits_dev(int field, const uint64_t* in_dev, int format, unsigned num_bits, size_t n, uint64_t* out_dev, uint32_t* flags_dev, unsigned bit) {
    return direct_step("kh_field_bits_dev", field, 0, {KH_STEP_BITS, n, {}, {in_dev}, {out_dev}, num_bits, nullptr, flags_dev, bit, 0, nullptr, format});
}

// ---------------------------------------------------------------------------------- wires between the gadgets (kernels in wiring.hip)
int kh_witness_gather_dev(int field, const uint64_t* witness_dev, size_t col_stride, size_t col_len, const uint32_t* cells, size_t n, int format,
                          uint64_t* out_dev, uint32_t* flags_dev, unsigned bit) {
    return direct_step("kh_witness_gather_dev", field, col_len,
                       {KH_STEP_GATHER, n, {nullptr, 0, 0, (uint64_t*)witness_dev, col_stride}, {}, {out_dev}, 0, nullptr, flags_dev, bit, 0, cells, format});
}
int kh_witness_scatter_dev(int field, const uint64_t* values_dev, int format, const uint32_t* cells, size_t n, uint64_t* witness_dev, size_t col_stride,
                           size_t col_len, uint32_t* flags_dev, unsigned bit) {
    return direct_step("kh_witness_scatter_dev", field, col_len,
                       {KH_STEP_SCATTER, n, {nullptr, 0, 0, witness_dev, col_stride}, {values_dev}, {}, 0, nullptr, flags_dev, bit, 0, cells, format});
}
int kh_generic_witness_dev(int field, const uint64_t coeffs[20], int half, const uint64_t* l_dev, const uint64_t* r_dev, size_t n, const uint32_t* rows,
                           size_t row0, size_t row_stride, uint64_t* witness_dev, size_t col_stride, size_t col_len, uint64_t* out_dev) {
    return direct_step("kh_generic_witness_dev", field, col_len,
                       {KH_STEP_GENERIC, n, {rows, row0, row_stride, witness_dev, col_stride}, {l_dev, r_dev}, {out_dev}, (unsigned)half, coeffs});
}

}  // extern "C"
