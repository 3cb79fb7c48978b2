// msm.hpp -- internal interface between the extern "C" boundary (context.hip, srs.cpp, msm_api.cpp, opening.cpp, vector_api.cpp, debug_api.cpp) and the kernel files
#pragma once
#include "common.hpp"
#include "host_ec.hpp"
#include "gate_batch.hpp"
#include "witness_lookup.hpp"

namespace kh {

// builds the window tables 2^(c*w) * P_i in place: `tables` holds W x n x 64 B with table 0 = the basis
int msm_precompute(Context& C, int curve, void* tables, const uint8_t* inf, size_t n, int c);
// rebase.hip: the folded basis of the opening's late rounds, materialised from the c = 16 tables (see there)
int rebase_points(hipStream_t s, int curve, const uint64_t* coef, size_t Q, const void* tables, size_t stride, size_t N, void* B, void* part, void* lists,
                  hipEvent_t after_plan = nullptr);
int rebase_tables(hipStream_t s, int curve, const void* part, size_t N, const void* extra_affine_host, size_t extra, int c, void* scratch, void* tables, uint32_t* fail,
                  const uint64_t* glv_beta = nullptr);      // glv_beta (Montgomery, base field): build W/2 levels and phi of them
int msm_debug_glv_split(hipStream_t s, int field, const uint64_t* scalars_dev, size_t n, uint32_t* out_dev);
const uint32_t* msm_glv_lambda(int scalar_field);         // the eigenvalue the split's constants were generated for (canonical, 8 x 32-bit limbs)
size_t rebase_bucket_bytes(size_t N);
size_t rebase_part_bytes(size_t N);
size_t rebase_list_bytes(size_t Q);
static constexpr int MSM_PRECOMP_C = 16;          // window width of the precomputed tables
// (windows_of(c): the windows of c bits that cover a 256-bit scalar = tables of a set -- msm_plan.hpp)
static constexpr int MSM_WIDE_C = 20;             // ... of the second table set big bases get: 13 windows, 2^19 buckets (msm.hip, "wide windows")
void msm_set_wide_min_n(size_t n);
void msm_set_sort_staging(unsigned entries, unsigned max_passes);   // k_part2_sort's staged scatter (kh_msm_set_sort_staging)
size_t msm_wide_min_n();                          // MSMs of at least this many points take the wide tables (KH_WIDE_MIN_N, default 2^19; 0 = never)
                                                  // measured (tools/wide_ab.py, pipelined Mscalar/s narrow -> wide): 2^17 537 -> 400, 2^18 655 -> 685, 2^19 746 -> 815,
                                                  // 2^20 896 -> 960..1000, 2^21 770 -> 976, 2^22 861 -> 992
static constexpr size_t MSM_PRECOMP_MIN_N = 1024; // smaller bases keep the plain per-window path
// enqueue all device work of k MSMs on slot S (returns immediately); msm_finish waits for it and does the host part
// flags: MSM_SPREAD_SCALARS, MSM_LATENCY (msm_plan.hpp)
int msm_enqueue(Context& C, MsmSlot& S, int curve, const MsmBasis& basis, size_t offset, const uint64_t* scalars_dev, size_t n, size_t k, int mont,
                int flags = 0);
// flag_seen: the caller has read the job's launch count from S.done_flag (the result is in S.pinned): no wait on the event
int msm_finish(Context& C, MsmSlot& S, uint64_t* out_xy, uint8_t* out_inf, bool flag_seen = false);
int debug_field_op(Context& C, int field, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
int debug_field29_op(Context& C, int field, int op, int spread, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out, size_t n);
int debug_point_op(Context& C, int curve, int op, const uint64_t* p, const uint8_t* pinf, const uint64_t* q, const uint8_t* qinf, uint8_t* out, size_t n);
// kh_debug_bucket_tail: the records (128 B) of its input, scratch and output, or why no plan has such a tail; then the launches, on C.stream, nothing waits
int debug_bucket_tail_sizes(int tail, int fin, unsigned c_or_nb, unsigned m, size_t groups, size_t* in_records, size_t* seg_records, size_t* out_records);
int debug_bucket_tail(Context& C, int curve, int tail, int fin, unsigned c_or_nb, unsigned m, size_t groups, const uint8_t* buckets, uint8_t* seg, uint8_t* out);
// kh_debug_bucket_sums: room of the hot-bucket lists (big: 2 + 4 cap words, zeroed by the call; chunks: cap records); then the launches, as above
size_t debug_bucket_sums_cap(size_t nkeys, size_t ntasks);
int debug_bucket_sums(Context& C, int curve, int kind, size_t nkeys, const uint32_t* toff, const uint8_t* partial, uint8_t* buckets, uint32_t* big, size_t bigcap,
                      uint8_t* chunks);
// kh_debug_msm_sort: the shape and plan of the caller's job with the echo (pure: nothing is reserved); then reservation, poison, the launches of
// msm_launch_sort on slot S, the wait and the downloads
int debug_msm_sort_plan(Context& C, const kh_msm_sort_args_t& a, MsmShape& sh, MsmPlan& P, kh_msm_sort_echo_t* echo);
int debug_msm_sort_run(Context& C, MsmSlot& S, const kh_msm_sort_args_t& a, const MsmShape& sh, const MsmPlan& P, const kh_msm_sort_echo_t& echo, const kh_msm_sort_out_t& out);

// ntt.hip
int ntt_build_twiddles(Context& C, int field, unsigned logn, int inverse, uint64_t* tab);
void ntt_trim(Context& C);
// ipa.hip
int ipa_fold_scalars(Context& C, int field, const uint64_t* lo, const uint64_t* hi, const uint64_t u[4], size_t n, uint64_t* out);
int ipa_inner_product(Context& C, int field, const uint64_t* a, const uint64_t* b, size_t n, uint64_t out[4]);
int ipa_fold_points_endo(Context& C, int curve, const uint64_t* g_lo, const uint64_t* g_hi, const uint64_t chal[2], size_t n, uint64_t* out_xy, uint8_t* out_inf);
int ipa_round_step(hipStream_t s, int field, int has_fold, const uint64_t* a, const uint64_t* b, const uint64_t* coef, size_t n, size_t cur2, size_t ncoef,
                   const uint64_t u[4], const uint64_t uinv[4], uint64_t* a2, uint64_t* b2, uint64_t* coef2,
                   const uint64_t rand_l[4], const uint64_t rand_r[4], uint64_t* sc, uint64_t* partial, unsigned* counter, unsigned extra, unsigned uslot);
// (extra: scalar entries behind the n points of each side = slots behind the points of the table set; uslot: which U slot is the opening's -- ipa.hip, k_ipa_step)
int ipa_round_fold(hipStream_t s, int field, const uint64_t* a, const uint64_t* b, const uint64_t* coef, size_t Nj, size_t ncoef,
                   const uint64_t u[4], const uint64_t uinv[4], uint64_t* a2, uint64_t* b2, uint64_t* coef2);
int ipa_sg_split(hipStream_t s, int field, const uint64_t* coef, size_t n, int has_fold, const uint64_t u[4], uint64_t* out);
int bpoly_run(hipStream_t s, int field, const uint64_t* chals_dev, unsigned rounds, size_t k, const uint64_t* rs_dev, uint64_t* out_dev);
// poly.hip
int poly_lincomb(Context& C, int field, const uint64_t* const* segs_dev, const size_t* lens, const uint64_t* scales, size_t m, uint64_t* out_dev, size_t out_len);
int poly_b_init(Context& C, int field, const uint64_t* elm, const uint64_t* scales, size_t k, size_t n, uint64_t* out_dev);
int poly_eval_chunks(Context& C, int field, const uint64_t* const* polys_dev, const size_t* lens, const size_t* num_chunks, size_t m, size_t chunk,
                     const uint64_t* points, size_t npts, uint64_t* out);
int poly_div_vanishing(Context& C, int field, const uint64_t* f_dev, size_t len, size_t n, uint64_t* q_dev, uint64_t* r_dev);
int poly_coset_ntt(Context& C, int field, const uint64_t* coeffs_dev, unsigned log2_n, const uint64_t shift[4], uint64_t* out_dev, size_t batch);
int poly_scan(Context& C, int field, int op, int rev, uint64_t* data_dev, size_t n);
int poly_batch_inversion(Context& C, int field, uint64_t* v_dev, size_t n);
int poly_divide_by_linear(Context& C, int field, const uint64_t* f_dev, size_t len, const uint64_t a[4], uint64_t* q_dev, uint64_t rem[4], uint64_t* rem_dev = nullptr);
int poly_check_equal(Context& C, const uint64_t* v_dev, size_t n, const uint64_t* expect, uint32_t* flags_dev, unsigned bit);
int poly_index_columns(Context& C, int field, const uint8_t* selcol_dev, const uint32_t* wires_dev, const uint64_t* coeffs_dev, size_t n_gates,
                       size_t n, size_t zk_rows, const uint64_t* shifts, size_t ncol, uint64_t* d1_dev);
// lookup_index.hip: the lookup index's columns and row-set atoms (kh_prover_index_create_lookup)
int lookup_selector_columns(Context& C, int field, const uint8_t* code_dev, size_t n_gates, size_t n, const int* patterns, size_t npat, uint64_t* out_dev);
int lookup_table_columns(Context& C, int field, const uint64_t* segs_dev, const uint64_t* seg_starts /* host: first row per segment */, size_t nseg, const uint64_t* data_dev, size_t n, size_t width,
                         uint64_t* tcols_dev, uint64_t* ids_dev, uint64_t* rtsel_dev, size_t rt_offset, size_t rt_len, size_t zk_rows);
int lookup_atom_denominators(Context& C, int field, const uint64_t* x8_dev, size_t n, size_t zk_rows, const uint64_t a[4], const uint64_t omega[4],
                             uint64_t* atoms_dev);
int lookup_atom_finish(Context& C, int field, size_t n, size_t zk_rows, const uint64_t zh8[32], const uint64_t lim0[4], const uint64_t limf[4],
                       uint64_t* atoms_dev);
// lookup_sorted.hip: the `sorted` step of the lookup argument (kh_lookup_sorted_dev).  scratch_dev: lookup_sorted_scratch_words(L) 32-bit words, of which
// the two at lookup_sorted_status_offset(L) end up as [lowest s * L + r of a value that is not in the table, or 0xffffffff | size of the sorted multiset]
size_t lookup_sorted_scratch_words(size_t L);
size_t lookup_sorted_status_offset(size_t L);
int lookup_sorted_run(Context& C, const uint64_t* table_dev, size_t L, const uint64_t* values_dev, size_t value_stride, size_t mpr, uint64_t* out_dev,
                      size_t out_stride, uint32_t* scratch_dev);
// expr.hip
// the gate library as compiled kernels (gates.hip; generated from the same expression DAGs as the token programs)
int gate_count();
const char* gate_name(int gate);
int gate_num_constants(int gate);
int gate_constants(int field, int gate, const uint64_t* alpha, const uint64_t* endo, const uint64_t* params, size_t nparams, uint64_t* out);
int gate_fixed_constants(int field, int gate, const uint64_t* endo, uint64_t* out);      // the literal and endo slots of that table alone
int gate_run(Context& C, int field, int gate, const uint64_t* const* cols_dev, size_t len, const uint64_t* consts, size_t nconsts, size_t rows,
             unsigned stride, unsigned next_shift, int accumulate, uint64_t* out_dev);
// the verifier's constant term for a batch of proofs (kh_batch_verify): the same bodies with one constants table per item (gates.hip)
int gate_batch_run(Context& C, int field, const uint64_t* cols_host, size_t ncols, size_t items, const GateBatchLaunch* launches, size_t nl, uint64_t* out_dev,
                   const uint64_t** cols_dev);
// witness_check.hip: the gate constraints of every row one by one, the copy constraints and (lk != NULL) the lookups (kh_witness_check,
// kh_witness_check_full).  scratch_dev: witness_check_scratch_bytes() (+ witness_check_lookup_scratch_bytes with lookups), whose first four 64-bit words
// end up as [lowest (row * 64 + sub) << 32 | detail, or ~0 | rows with a violated gate | disconnected cells | lookups that are in no table]
size_t witness_check_scratch_bytes();
size_t witness_check_lookup_scratch_bytes(size_t L, size_t W, size_t rt_len);
int witness_check_num_constraints(int gate);
int witness_check_run(Context& C, int field, const uint64_t* witness_dev, const uint64_t* d1_dev, size_t n, const int* sel_col, size_t ngate_ids,
                      size_t public_inputs, const uint64_t endo[4], const uint32_t* wires_dev, size_t n_gates, const WitnessLookups* lk, void* scratch_dev);
int expr_run(Context& C, int field, const uint32_t* prog, size_t ntok, const uint64_t* const* cols_dev, const size_t* col_len, size_t ncols,
             const uint64_t* consts, size_t nconsts, size_t rows, unsigned stride, unsigned next_shift, int accumulate, uint64_t* out_dev);
// host_srs.cpp
void scalar_challenge_to_field(int field, const uint64_t chal[2], const uint64_t endo[4], uint64_t out[4]);
void host_window_multiples(int curve, const uint64_t xy[8], int W, int c, uint64_t* out_xy);   // out[w] = 2^(c w) P, affine
void host_field_inverse(int field, const uint64_t a[4], uint64_t out[4]);
void endo_coefficient(int field, uint64_t out[4]);
void curve_endos(int curve, uint64_t endo_q[4], uint64_t endo_r[4]);
int ipa_fold_points(Context& C, int curve, const uint64_t* g_lo, const uint64_t* g_hi, const uint64_t u[4], size_t n, uint64_t* out_xy, uint8_t* out_inf);
// srs_gen.hip
int srs_generate_device(Context& C, int curve, size_t start, size_t count, void* out_xy_dev);
// lagrange.hip
int lagrange_run(Context& C, int curve, const void* g_dev, size_t srs_size, unsigned log_n, unsigned chunk, void* out_xy_dev, uint8_t* out_inf_dev);
khost::fe ntt_host_root(int field, unsigned logn, int inverse);   // omega_{2^logn} (or its inverse), Montgomery
int ntt_set_max_logr(unsigned v);            // 4..10, 0 = default (kh_ntt_set_max_logr)
int ntt_run(Context& C, int field, uint64_t* data_dev, unsigned log2_n, int inverse, size_t batch);
int lde_run(Context& C, int field, const uint64_t* coeffs_dev, unsigned log2_n, unsigned log2_blowup, uint64_t* out_dev, size_t batch);

}  // namespace kh
