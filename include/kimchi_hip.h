/*
 * kimchi_hip.h -- C ABI of the MI355X-native MSM + NTT hot path for Kimchi.
 *
 * This is the drop-in boundary: a Rust shim crate implements
 * poly-commitment's `trait SRS<G>` / `trait OpenProof<G>` by delegating the MSMs to
 * the kh_msm* entry points, and kimchi's evaluation-domain transforms by delegating
 * to kh_ntt / kh_lde.  Plain C, no exceptions, no torch types.  Every function
 * returns 0 on success or a negative KH_E_* code; kh_last_error() describes the last
 * failure on the calling thread.  All functions are thread-safe (the reference calls
 * SRS::commit_evaluations_non_hiding from 15 rayon workers at once,
 * kimchi/src/prover.rs:329-351).
 *
 * Wire format (zero-copy from Rust):
 *   field element = 4 x uint64_t little-endian limbs in Montgomery form, R = 2^256,
 *                   i.e. ark-ff's in-memory Fp256<MontBackend<_,4>> (the reference
 *                   itself reinterprets Fp as [u64;4]: kimchi/src/cached_prover_index.rs:502-539);
 *   affine point  = x || y = 8 limbs (64 bytes), infinity passed out of band
 *                   (ark-ec Affine{x,y,infinity} has no stable layout: the shim packs it);
 *   curve id      : 0 = Vesta  (coordinates in Fq, scalars in Fp)
 *                   1 = Pallas (coordinates in Fp, scalars in Fq)
 *   field id      : 0 = Fp, 1 = Fq.
 * Results are returned affine because the Fiat-Shamir sponge absorbs affine
 * coordinates (poly-commitment/src/commitment.rs:503-514).
 */
#ifndef KIMCHI_HIP_H
#define KIMCHI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KH_OK 0
#define KH_E_INVALID (-1)    /* bad argument (null pointer, size, id) */
#define KH_E_DEVICE (-2)     /* HIP runtime error / no device */
#define KH_E_NOTFOUND (-3)   /* basis not registered on this SRS */
#define KH_E_NOMEM (-4)

#define KH_CURVE_VESTA 0
#define KH_CURVE_PALLAS 1
#define KH_FIELD_FP 0
#define KH_FIELD_FQ 1
#define KH_BASIS_G (-1)      /* the monomial basis g of the SRS */

typedef struct kh_srs kh_srs_t;
typedef struct kh_sponge kh_sponge_t;      /* host-side Fiat-Shamir sponge, see the end of this file */

/* ---- device ------------------------------------------------------------- */
int kh_device_count(void);
/* Initialises a device (streams, workspaces) and makes it the calling thread's current device; the FIRST device
 * initialised is also the process default, i.e. what every other thread uses until it chooses otherwise.  Idempotent;
 * kh_init(-1) picks the current choice, else LOCAL_RANK, else device 0.  One process per GPU (torch.distributed
 * ranks) needs nothing else.  A single process may also drive SEVERAL GPUs: each device has its own context (streams,
 * four MSM pipeline slots, caches); an SRS handle lives on the device that was current when it was created and every
 * entry point taking a handle (kh_msm*, kh_commit*, kh_ipa_*, ...) runs on the handle's device whatever the calling
 * thread's current device is -- a Rust prover holds Vesta on GPU 0 and Pallas on GPU 1 (BASELINE config 5), or shards
 * one MSM over 8 handles created with kh_srs_create_device_range (config 4), from ordinary rayon threads.  Entry points
 * WITHOUT a handle (kh_ntt*, kh_lde*, kh_dev_alloc, the vector steps) use the calling thread's current device. */
int kh_init(int device_id);
int kh_set_device(int device_id);     /* thread-local: this thread's current device from now on (initialised on first use) */
int kh_get_device(void);              /* the calling thread's current device (-1 before any initialisation) */
/* Several prover threads in one process: between _begin and _end the calling thread works on a library context of its own on its current device -- own
 * main stream, MSM pipeline slots, workspaces and lock -- instead of the device's shared one, so that independent provers neither queue their vector steps
 * on one stream nor serialise their launches on one mutex (measured: four provers 150 -> 165-176 proofs/s; four processes: 177).  Everything the thread
 * queues in between is complete when _end returns; tickets of kh_msm_submit must be waited for before _end; work the thread queued on the shared context
 * before _begin is ordered in front.  SRS handles, device buffers and indexes are process-wide as before: one handle and one index serve every prover thread (up to
 * KH_IPA_OPENINGS openings run over a handle's tables at once, see kh_ipa_begin).
 * kh_prove* do this themselves.  Contexts are pooled per device and reused. */
int kh_private_context_begin(void);
int kh_private_context_end(void);
int kh_private_context_active(void);   /* 1 if the calling thread is between _begin and _end on its current device */
/* per-phase HIP events behind kh_last_timings on the calling thread's current context (the private one between _begin and _end): OFF by default -- an event
 * between two kernels costs the stream 6-10 us of idle time; tools that read kh_last_timings switch them on */
int kh_set_phase_timers(int on);
int kh_trim(void);                    /* current device: free cached twiddle tables, scratch and idle MSM workspaces (rebuilt on demand) */
const char *kh_last_error(void);

/* ---- SRS: device-resident bases ------------------------------------------
 * Replaces the `g: Vec<G>` half of `ipa::SRS<G>` (poly-commitment/src/ipa.rs:53-75):
 * uploads the n monomial-basis points once; Rust keeps owning its own copy. */
int kh_srs_create(int curve, const uint64_t *g_xy /* n x 8 limbs */, size_t n, kh_srs_t **out);
/* Tuning knob (process-wide): bases of at least n points get a SECOND window-table set with 20-bit windows when they are created (13 instead of 16
 * table additions per scalar, 2^19 buckets, +13/16 of the table memory), and single MSMs of at least n scalars over them take it.  Default 2^19
 * (KH_WIDE_MIN_N), 0 = never.  Results are the same group elements either way; the tests lower it to run the wide path at small sizes. */
int kh_msm_set_wide_min_n(size_t n);
/* Tuning knob (process-wide) of the wide path's sort: the second sorting pass collects a partition's entries in LDS and writes them out as coalesced runs, in
 * at most `max_passes` passes of `entries` entries each (default 28,672 and 2: KH_PART2_STAGE / KH_PART2_MAXPASS); a partition that would need more passes, or
 * entries = 0, takes the direct scatter.  Same results under every setting; the tests shrink it to run the multi-pass and the fallback branches at small sizes. */
int kh_msm_set_sort_staging(unsigned entries, unsigned max_passes);
/* The wide set is OPTIONAL: if it does not fit in device memory when the handle is created, the handle is created without it (the narrow tables serve every
 * MSM, ~8 % slower at 2^20) and no error is reported.  kh_srs_set_wide_tables(srs, 0) gives an existing wide set back (832 MiB at 2^20 points, 3.3 GiB at
 * 2^22) -- KH_E_INVALID while an MSM over the handle is in flight, submitted by ANY thread or context (the handle counts them) --, (srs, 1) builds it now whatever the threshold says and fails with KH_E_NOMEM if it
 * does not fit; kh_srs_has_wide_tables tells which state the handle is in. */
int kh_srs_set_wide_tables(kh_srs_t *srs, int on);
int kh_srs_has_wide_tables(const kh_srs_t *srs);
void kh_srs_free(kh_srs_t *srs);
size_t kh_srs_size(const kh_srs_t *srs);
int kh_srs_curve(const kh_srs_t *srs);    /* KH_CURVE_VESTA / KH_CURVE_PALLAS */
int kh_srs_device(const kh_srs_t *srs);   /* the device the handle's tables live on */

/* SRS::create (poly-commitment/src/ipa.rs:751-778) on the host: g_start .. g_{start+count-1}
 * (Blake2b-512 of the big-endian u32 index -> Shallue-van de Woestijne map, groupmap/src/lib.rs:74-189)
 * and the blinding base h (ipa.rs:765-772).  Affine x||y, Montgomery.  threads <= 0: all host cores. */
int kh_srs_generate(int curve, size_t start, size_t count, uint64_t *out_xy, int threads);
int kh_srs_h(int curve, uint64_t out_xy[8]);
/* GroupMap::to_group (groupmap/src/lib.rs:167-189): the U base of SRS::open / verify, u_base = to_group(sponge.challenge_fq())
 * (ipa.rs:909-913).  t: a base-field element, Montgomery limbs.  Host code. */
int kh_group_map_to_group(int curve, const uint64_t t[4], uint64_t out_xy[8]);

/* SRS::create(depth) entirely on the device (csrc/srs_gen.hip: Blake2b + group map + Tonelli-Shanks per
 * thread; ~15 ms for 2^20 points), already expanded to the MSM window tables; kh_srs_get_g reads
 * g[offset .. offset+count) back for the caller's own `g: Vec<G>`. */
int kh_srs_create_device(int curve, size_t depth, kh_srs_t **out);
/* the slice g[start .. start+count) of a larger SRS (one rank of a point-range-sharded MSM) */
int kh_srs_create_device_range(int curve, size_t start, size_t count, kh_srs_t **out);
int kh_srs_get_g(kh_srs_t *srs, size_t offset, size_t count, uint64_t *out_xy);

/* Registers chunk `chunk` of the Lagrange basis for the domain of size 2^log2_domain
 * (`SRS::get_lagrange_basis`, ipa.rs:780-801; entries computed by ipa.rs:1065-1172):
 * n = 2^log2_domain points, `inf` nullable per-point infinity flags. */
int kh_srs_set_lagrange(kh_srs_t *srs, unsigned log2_domain, unsigned chunk,
                        const uint64_t *xy, const uint8_t *inf, size_t n);
/* Computes the same basis on the device from g (group iNTT + batch normalisation,
 * ipa.rs:1065-1172) and registers every chunk.  Optional read-back via
 * kh_srs_get_lagrange (out_xy: n x 8 limbs, out_inf: n bytes). */
int kh_srs_compute_lagrange(kh_srs_t *srs, unsigned log2_domain);
int kh_srs_get_lagrange(kh_srs_t *srs, unsigned log2_domain, unsigned chunk,
                        uint64_t *out_xy, uint8_t *out_inf);
int kh_srs_lagrange_chunks(const kh_srs_t *srs, unsigned log2_domain);   /* 0 if not registered */

/* ---- MSM ------------------------------------------------------------------
 * Replaces ark_ec::VariableBaseMSM::{msm, msm_bigint} at the call sites
 * poly-commitment/src/ipa.rs:649,658-659,672 (commit_non_hiding) and
 * commitment.rs:382 (PolyComm::multi_scalar_mul, reached from
 * commit_evaluations_non_hiding ipa.rs:706-728).
 *
 * basis = KH_BASIS_G: out = sum_{i<n} scalars[i] * g[offset + i]
 * basis = log2_domain: out = sum_{i<n} scalars[i] * L_{offset+i}[chunk]
 * scalars: n x 4 limbs; scalars_are_montgomery selects Fp-in-memory (1) vs
 * into_bigint() canonical form (0, what msm_bigint receives).  Like msm_bigint,
 * uses min(n, basis_len - offset) pairs.  Result affine + infinity flag. */
int kh_msm(kh_srs_t *srs, int basis, unsigned chunk, size_t offset,
           const uint64_t *scalars, size_t n, int scalars_are_montgomery,
           uint64_t out_xy[8], uint8_t *out_is_inf);

/* k MSMs over the same basis window [offset, offset+n), scalars = k x n x 4 limbs
 * (the 15 witness-column commits of prover.rs:329-351, the 7 chunk commits of
 * ipa.rs:663-676 with per-chunk offsets handled by the host mirror). */
int kh_msm_batch(kh_srs_t *srs, int basis, unsigned chunk, size_t offset,
                 const uint64_t *scalars, size_t n, size_t k, int scalars_are_montgomery,
                 uint64_t *out_xy /* k x 8 */, uint8_t *out_is_inf /* k */);

/* Ad-hoc bases (IPA rounds ipa.rs:943-961, batch verifier ipa.rs:474-499). */
int kh_msm_points(int curve, const uint64_t *xy /* n x 8 */, const uint8_t *inf /* nullable */,
                  const uint64_t *scalars, size_t n, int scalars_are_montgomery,
                  uint64_t out_xy[8], uint8_t *out_is_inf);

/* k independent MSMs of the same length n with their own bases (xy: k x n x 8, inf: k x n or NULL,
 * scalars: k x n x 4) in one pass -- the L and R commitments of an IPA round (ipa.rs:943-961) are
 * two such MSMs that do not depend on each other. */
int kh_msm_points_batch(int curve, const uint64_t *xy, const uint8_t *inf, const uint64_t *scalars,
                        size_t n, size_t k, int scalars_are_montgomery,
                        uint64_t *out_xy /* k x 8 */, uint8_t *out_is_inf /* k */);

/* Sum of n affine points on the host (a handful of group additions): the fold of the per-GPU partial
 * sums of a point-range-sharded MSM after the all-gather, or `(r1 + r2).into_affine()` of ipa.rs:661. */
int kh_points_sum(int curve, const uint64_t *xy, const uint8_t *inf, size_t n, uint64_t out_xy[8], uint8_t *out_is_inf);
/* out_j = a_j + b_j for n pairs of affine points on the host (one field inversion in all; NULL flags = no point at infinity).  With
 * kh_mask_custom over commitments at infinity -- the blinding points [r_j] H, which do not depend on the commitment -- this is SRS::mask_custom
 * (ipa.rs:605-622) in two halves: the scalar multiplications run while the device computes the commitment, only n additions follow its result. */
int kh_points_add(int curve, const uint64_t *a_xy, const uint8_t *a_inf, const uint64_t *b_xy, const uint8_t *b_inf, size_t n,
                  uint64_t *out_xy /* n x 8 */, uint8_t *out_is_inf /* n */);

/* One MSM over a basis sharded by POINT RANGE over R handles (BASELINE config 4): shard r holds g[o_r, o_r + n_r), o_r =
 * n_0 + ... + n_(r-1), n_r = kh_srs_size(shards[r]), on whatever device it was created on (kh_srs_create_device_range after
 * kh_set_device: one shard per GPU, or several per GPU).  Each shard reduces its slice of the scalars with the full single-GPU
 * pipeline on its own device, concurrently; the R partial sums are folded on the host (kh_points_sum: RCCL has no group-addition
 * reduction, and R x 64 bytes do not need one).  `scalars`: host, N x 4 limbs, N = sum n_r (fewer: the tail shards get the rest / nothing).
 * This is the whole of config 4 for a one-process caller (the Rust shim); one-process-per-GPU deployments all-gather the partials
 * instead (proof_systems_amd/sharded.py over torch.distributed / RCCL). */
int kh_msm_sharded(kh_srs_t *const *shards, size_t R, const uint64_t *scalars, size_t n, int scalars_are_montgomery,
                   uint64_t out_xy[8], uint8_t *out_is_inf);
/* The same with the scalars already resident: scalars_dev[r] = shard r's slice (counts[r] <= n_r elements) on shard r's device.
 * All R jobs are submitted before the first is waited for. */
int kh_msm_sharded_dev(kh_srs_t *const *shards, size_t R, const uint64_t *const *scalars_dev, const size_t *counts,
                       int scalars_are_montgomery, uint64_t out_xy[8], uint8_t *out_is_inf);

/* ---- IPA round vector operations (poly-commitment/src/ipa.rs:980-1006) -----
 * out[i] = lo[i] + u * hi[i]      (a' = a_lo + u^-1 a_hi with u := u^-1; b' = b_lo + u b_hi)          */
int kh_ipa_fold_scalars(int field, const uint64_t *lo, const uint64_t *hi, const uint64_t u[4], size_t n, uint64_t *out);
/* <a, b> = sum a_i b_i (utils/src/field_helpers.rs:273-279) */
int kh_inner_product(int field, const uint64_t *a, const uint64_t *b, size_t n, uint64_t out[4]);
/* g'[i] = g_lo[i] + [u] g_hi[i], affine: CommitmentCurve::combine_one (commitment.rs:576-579); the
 * endo variant used by the prover (combine_one_endo, ipa.rs:1006) yields the same group elements for
 * u = u_pre.to_field(endo_r).  u: Montgomery limbs of the scalar field. */
int kh_ipa_fold_points(int curve, const uint64_t *g_lo_xy, const uint64_t *g_hi_xy, const uint64_t u[4], size_t n,
                       uint64_t *out_xy, uint8_t *out_inf);
/* CommitmentCurve::combine_one_endo (commitment.rs:581-589 -> combine.rs:292-340; prover call site
 * ipa.rs:1006): g'[i] = g_lo[i] + [chal.to_field(endo_r)] g_hi[i] by the Halo endo ladder -- 64 x
 * (doubling + mixed addition with +-g_hi or +-phi(g_hi)) instead of a 255-bit double-and-add.
 * chal: the 128-bit ScalarChallenge prechallenge as two canonical (non-Montgomery) LE limbs. */
int kh_ipa_fold_points_endo(int curve, const uint64_t *g_lo_xy, const uint64_t *g_hi_xy, const uint64_t chal[2], size_t n,
                            uint64_t *out_xy, uint8_t *out_inf);
/* endos::<G>() (ipa.rs:214-231): endo_q in the base field, endo_r in the scalar field (Montgomery limbs)
 * with phi(P) = (endo_q x, y) = [endo_r] P.  Host-only, needs no device. */
int kh_endos(int curve, uint64_t endo_q[4], uint64_t endo_r[4]);
/* ScalarChallenge::to_field(&endo_r) (poseidon/src/sponge.rs:190-226) for the curve's scalar field:
 * chal = the 128-bit prechallenge (two canonical LE limbs), out = Montgomery limbs.  Host-only. */
int kh_scalar_challenge_to_field(int curve, const uint64_t chal[2], uint64_t out[4]);

/* ---- coefficient vectors between the transforms / commitments and the opening, device-resident ----
 * kh_combine_polys_dev = combine_polys for polynomials in coefficient form (poly-commitment/src/utils.rs:103-206):
 *   polynomial i (device pointer, lens[i] coefficients) is cut into num_chunks[i] chunks of srs_length (the length
 *   of its blinder PolyComm); chunk number t overall is scaled by polyscale^t; out_dev receives srs_length
 *   coefficients (zero above *out_len = the longest chunk), ready for kh_ipa_begin_dev.  The combined blinder
 *   (a sum of m scalars) stays with the caller.
 * kh_b_init_dev: b[j] = sum_i evalscale^i elm_i^j, j < padded_len (poly-commitment/src/ipa.rs:863-888).
 * kh_evaluate_chunks_dev: to_chunked_polynomial(num_chunks, chunk_size).evaluate_chunks(x) for each of npts points
 *   (utils/src/dense_polynomial.rs:50-69, chunked_polynomial.rs:21-28; the zeta / zeta*omega evaluations of
 *   kimchi/src/prover.rs:1000-1170): out[p][c] = chunk_c(points[p]), npts x num_chunks x 4 limbs on the host.
 * kh_divide_by_vanishing_poly_dev: f = q (x^n - 1) + r (kimchi/src/prover.rs:903): q_dev gets len - n coefficients
 *   (none if len <= n), r_dev n coefficients. */
int kh_combine_polys_dev(int field, const uint64_t *const *polys_dev, const size_t *lens, const size_t *num_chunks, size_t m,
                         const uint64_t polyscale[4], size_t srs_length, uint64_t *out_dev, size_t *out_len);
/* out[i] = sum_j scalars[j] * poly_j[i], i < out_len (lens[j] <= out_len): the linearisation / ft polynomial of
 * kimchi/src/prover.rs:1180-1260 (f = sum of evaluated-constant x column polynomial terms, minus Z_H(zeta) t). */
int kh_poly_lincomb_dev(int field, const uint64_t *const *polys_dev, const size_t *lens, const uint64_t *scalars, size_t m,
                        uint64_t *out_dev, size_t out_len);
int kh_b_init_dev(int field, const uint64_t *elm, size_t k, const uint64_t evalscale[4], size_t padded_len, uint64_t *out_dev);
int kh_evaluate_chunks_dev(int field, const uint64_t *coeffs_dev, size_t len, size_t chunk_size, size_t num_chunks,
                           const uint64_t *points, size_t npts, uint64_t *out);
/* all polynomials of a proof in one launch: polynomial j has lens[j] coefficients and num_chunks[j] chunks; out receives, polynomial
 * after polynomial, npts x num_chunks[j] values (out_j[p][c]). */
int kh_evaluate_chunks_batch_dev(int field, const uint64_t *const *polys_dev, const size_t *lens, const size_t *num_chunks, size_t m,
                                 size_t chunk_size, const uint64_t *points, size_t npts, uint64_t *out);
int kh_divide_by_vanishing_poly_dev(int field, const uint64_t *f_dev, size_t len, unsigned log2_n, uint64_t *q_dev, uint64_t *r_dev);

/* ---- constraint expressions over resident columns (first slice) ----
 * kh_expr_evaluations_dev = Expr::evaluations (kimchi/src/circuits/expr.rs:1938-2190) for an expression lowered to the
 * reference's reverse Polish form (PolishToken, expr.rs:815-836, produced by Expr::to_polish); the machine is
 * PolishToken::evaluate (expr.rs:856-937) run per row.  tokens: ntok pairs (opcode, argument):
 *   KH_TOK_CONST k   push constants[k]     (Literal / Challenge / Mds / EndoCoefficient, resolved by the caller)
 *   KH_TOK_CELL  a   push column[a >> 1] at this row (a & 1 = 0, Curr) or the next one (a & 1 = 1, Next):
 *                    element (stride * i + next * next_shift) mod col_len  (the SubEvals rule, expr.rs:1972-1987;
 *                    d8 columns into a d8 result: stride 1, next_shift 8; into a d4 result: stride 2, next_shift 8)
 *                    -- VanishesOnZeroKnowledgeAndPreviousRows and UnnormalizedLagrangeBasis(i) are such columns
 *   KH_TOK_DUP, KH_TOK_POW n, KH_TOK_ADD, KH_TOK_MUL, KH_TOK_SUB, KH_TOK_STORE, KH_TOK_LOAD i   as in the reference
 *   (SkipIf / SkipIfNot are resolved by the caller: feature flags are fixed per index).
 * out_dev[i] (= or +=, `accumulate`) the value of the expression on row i, i < rows.  A malformed program (stack
 * underflow, Load before Store, final stack length != 1: ExprError::EmptyStack / the assert at expr.rs:935) returns
 * KH_E_INVALID before anything is launched. */
enum { KH_TOK_CONST = 0, KH_TOK_CELL = 1, KH_TOK_DUP = 2, KH_TOK_POW = 3, KH_TOK_ADD = 4, KH_TOK_MUL = 5, KH_TOK_SUB = 6,
       KH_TOK_STORE = 7, KH_TOK_LOAD = 8 };
int kh_expr_evaluations_dev(int field, const uint32_t *tokens, size_t ntok, const uint64_t *const *cols_dev, const size_t *col_len,
                            size_t ncols, const uint64_t *constants, size_t nconsts, size_t rows, unsigned stride,
                            unsigned next_shift, int accumulate, uint64_t *out_dev);

/* The gate library (kimchi/src/circuits/polynomials/{poseidon,complete_add,varbasemul,endosclmul,endomul_scalar,xor,rot}.rs, range_check/, foreign_field_add/,
 * foreign_field_mul/) as COMPILED kernels: index(gate) * sum_i alpha^i constraint_i per row (prover.rs:824-868), the same value the token program of that gate
 * gives through kh_expr_evaluations_dev, several times faster (no operand stack in LDS).  cols_dev: 31 device columns of col_len elements -- witness 0..14,
 * coefficients 15..29, the gate's selector 30 --, addressed like KH_TOK_CELL (stride, next_shift); constants: the table the caller builds for the gate
 * (literals, MDS entries, the endo coefficient, powers of alpha: kh_gate_num_constants entries, layout fixed per gate at build time by
 * tools/gen_gate_kernels.py -- proof_systems_amd/polish.py::gate_program returns it).  Gates are numbered 0 .. kh_gate_count() - 1; kh_gate_name gives the
 * reference's GateType name.  Two more ids follow the library, for the arguments every circuit has: "Generic" (generic.rs:100-131; witness 0..5, coefficients
 * 15..24, the generic selector 30; constants [1, alpha]) and "Permutation" (permutation.rs:225-288: alpha0 zkpm (z prod_i (w_i + gamma + x beta shift_i) -
 * z(xw) prod_i (w_i + gamma + sigma_i beta)); witness 0..6, sigma_i at 15 + i, z 22, x 23, zkpm 24; constants [gamma, beta, alpha0, beta shift_0..6]).
 * Columns an expression does not read may be any valid pointer. */
int kh_gate_count(void);
const char *kh_gate_name(int gate);
int kh_gate_num_constants(int gate);
/* The constants table of `gate` for one proof, built on the host (no device call): the protocol's literals and Poseidon MDS entries, alpha^i for the
 * gate's constraints (alpha: Montgomery limbs; may be NULL for "Generic" / "Permutation"), the endo coefficient (endo: VerifierIndex::endo, NULL if
 * the gate has none), and for "Generic" / "Permutation" the caller's per-proof values `params` in the order given above.  out: kh_gate_num_constants x 4 limbs. */
int kh_gate_constants(int field, int gate, const uint64_t alpha[4], const uint64_t endo[4], const uint64_t *params, size_t nparams, uint64_t *out);
int kh_gate_evaluations_dev(int field, int gate, const uint64_t *const *cols_dev, size_t col_len, const uint64_t *constants, size_t nconsts,
                            size_t rows, unsigned stride, unsigned next_shift, int accumulate, uint64_t *out_dev);

/* ---- Poseidon on the device (csrc/poseidon.hip) ----
 * Kimchi Poseidon (PlonkSpongeConstantsKimchi, poseidon/src/constants.rs:29-41: width 3, rate 2, 55 full rounds of x^7, the 3 x 3 MDS, + round constants,
 * no initial round-constant addition; poseidon/src/permutation.rs full_round) as a batch operation: many permutations, many sponge hashes, and the witness
 * rows of the Poseidon gadget (11 gate rows + the output row) written straight into the witness_dev columns kh_witness_check and kh_prove consume -- so
 * that a circuit made of Poseidon gadgets needs neither a host pass over its rows nor their transfer.  One lane per permutation (three for small batches
 * of gadget rows, kh_poseidon_set_split_max_n); every value is the canonical Montgomery element the reference computes, bit for bit.  Inputs are canonical Montgomery elements (< p); they are not checked.
 * The three *_dev calls are vector steps like the ones above: queued on the main stream of the calling thread's current context (the private one between
 * kh_private_context_begin and _end), they return when queued and are ordered against every other call of the library -- a producer followed by a consumer
 * needs no kh_sync.  n == 0 is KH_OK with nothing launched.  KH_E_INVALID with a kh_last_error text, before anything is launched and with nothing written:
 * an unknown field, a null pointer with n > 0, a device pointer that is not 16-byte aligned, sizes whose byte counts overflow, and for
 * kh_poseidon_gate_witness_dev an instance that does not fit (rows[i] + 12 > col_len, naming i; rows == NULL with row_stride < 12 or
 * row0 + (n - 1) row_stride + 12 > col_len) or col_stride < col_len.  Instances that overlap in `rows` are the caller's responsibility: they are not
 * checked, and which instance's values the shared cells end up with is undefined. */
/* host only, no device: the 11 coefficient rows of a Poseidon gadget, out[(15 r + c)] = round constant (5 r + c / 3)[c % 3]
 * (poseidon.rs:239-290), 11 x 15 x 4 Montgomery limbs -- what a gate list for kh_prover_index_create carries on its Poseidon rows */
int kh_poseidon_gate_coefficients(int field, uint64_t *out);

/* n permutations in place: states_dev = n x 3 x 4 limbs */
int kh_poseidon_permute_dev(int field, uint64_t *states_dev, size_t n);

/* n sponge hashes of msg_len elements each (msgs_dev: n x msg_len x 4 limbs, message after message): state = init (3 elements on the
 * host, NULL = zero), absorb the message, squeeze once (poseidon/src/poseidon.rs:60-175) -> digests_dev: n x 4 limbs.
 * msg_len == 0 is allowed (msgs_dev may be NULL): max(1, ceil(msg_len / 2)) permutations per hash */
int kh_poseidon_hash_dev(int field, const uint64_t *msgs_dev, size_t msg_len, size_t n, const uint64_t *init, uint64_t *digests_dev);

/* The witness of n Poseidon gadgets (kimchi/src/circuits/polynomials/poseidon.rs:239-290, state order :65-80): instance i starts at row
 * rows[i] (host array, copied before the call returns), or at row0 + i * row_stride when rows == NULL (row_stride >= 12).
 * witness_dev: 15 columns, column c at witness_dev + 4 * c * col_stride, col_len rows each -- the layout kh_prove / kh_witness_check take
 * with col_stride = n.  Written per instance: all 15 cells of rows r .. r + 10 (round 5 j + t of row r + j in columns
 * 3 * {0, 2, 3, 4, 1}[t] + k) and cells 0..2 of row r + 11 (the final state).  NOTHING else is written.
 * out_states_dev (nullable; may equal states_dev): the n final states. */
int kh_poseidon_gate_witness_dev(int field, const uint64_t *states_dev, size_t n, const uint32_t *rows, size_t row0, size_t row_stride,
                                 uint64_t *witness_dev, size_t col_stride, size_t col_len, uint64_t *out_states_dev);
/* Tuning knob (process-wide): kh_poseidon_gate_witness_dev spreads a permutation over three lanes (7 products in sequence per round instead of 21, three
 * times the waves) for up to n instances, and takes one lane per permutation above; default 43008 (two three-lane waves per SIMD), 0 = never.  The same
 * values are written either way; the tests set it to run both kernels at small sizes. */
int kh_poseidon_set_split_max_n(size_t n);

/* ---- The curve gates' witness on the device (csrc/curve_gadgets.hip) ----
 * CompleteAdd, VarBaseMul, EndoMul and EndoMulScalar: with kh_poseidon_gate_witness_dev, the witness of every always-present library gate, written in
 * place from a few inputs per instance.  The conventions are those of the Poseidon block above.  witness_dev: 15 columns, column c at
 * witness_dev + 4 * c * col_stride, col_len rows each.  Instance i starts at row rows[i] (host array, copied before the call returns), or at
 * row0 + i * row_stride when rows == NULL.  The calls are vector steps: queued on the main stream of the calling thread's current context (the private
 * one between kh_private_context_begin and _end) and ordered against every other call of the library -- a producer followed by a consumer needs no
 * kh_sync.  (kh_varbasemul_witness_dev and kh_endomul_witness_dev wait for the stream once per slice, see below: they invert one element on the host,
 * like kh_batch_inversion_dev.)  n == 0 is KH_OK with nothing launched.  KH_E_INVALID with a kh_last_error text, before anything is launched and with
 * nothing written: an unknown field, a null pointer with n > 0, a device pointer that is not 16-byte aligned, byte counts that overflow, an instance
 * that does not fit col_len (naming it), row_stride smaller than an instance's row count, col_stride < col_len, a bad num_bits.
 * `field` is the circuit's field; points are affine x || y in that field (8 limbs, Montgomery), as the gates see them, and are not checked to be on a
 * curve.  Every value is the canonical Montgomery element the reference's generator computes, bit for bit, and each call writes exactly the cells that
 * generator assigns: NOTHING else (not column 6 of a VarBaseMul base row, columns 12..14 of its bit row, column 3 of an EndoMul row, columns 11..14 of
 * CompleteAdd).  Overlapping instances are the caller's responsibility. */

/* complete_add.rs witness: one row per instance, cells 0..10 = x1 y1 x2 y2 x3 y3 inf same_x s inf_z x21_inv: the generic sum, the doubling when
 * p1 == p2, inf = 1 (x3, y3 as the formulas give them) for P + (-P).  out_dev (nullable): n x 8 limbs, (x3, y3) as written. */
int kh_complete_add_witness_dev(int field, const uint64_t *p1_dev, const uint64_t *p2_dev, size_t n, const uint32_t *rows, size_t row0, size_t row_stride,
                                uint64_t *witness_dev, size_t col_stride, size_t col_len, uint64_t *out_dev);

/* varbasemul.rs witness(): acc <- (acc + Q) + acc for the bits num_bits - 1 .. 0 of scalars_dev[i] (n x 4 canonical little-endian limbs, plain integers;
 * higher bits are ignored), Q = base if the bit is 1 and -base otherwise, starting from acc0; 5 bits per pair of rows, 2 * num_bits / 5 rows per instance
 * (num_bits a multiple of 5 from 5 to 255).  out_acc_dev (nullable, n x 8): the final accumulator; out_n_dev (nullable, n x 4, Montgomery): the final
 * n_acc, the scalar's num_bits bits mod p.
 * Zero denominators (the reference's generator panics: x_i == x_Q or R == -acc at some bit): flags_dev (nullable) is a caller-zeroed uint32_t on the
 * device, as for kh_check_equal_dev; bit `bit` (< 32) of it is set when any instance met one, and is not touched otherwise.  Such an instance's own
 * cells are unspecified (inside its own rows); every other instance of the call is exact.
 * No lane inverts per bit: one lane per instance walks the accumulator in XYZZ coordinates, one batch inversion over (instance, bit) yields the affine
 * accumulators and the slopes, one lane per (instance, bit) writes the cells.  Scratch comes from the kh_dev_alloc pool for the time of the call:
 * 160 bytes per (instance, bit + 1) -- 41 KB per 255-bit instance --, for at most 2^22 / (num_bits + 1) instances at a time (16384 at 255 bits,
 * 0.67 GB); a larger batch is worked through in slices of that many, so n is bounded only by the grid (2^36). */
int kh_varbasemul_witness_dev(int field, const uint64_t *base_dev, const uint64_t *acc0_dev, const uint64_t *scalars_dev, unsigned num_bits, size_t n,
                              const uint32_t *rows, size_t row0, size_t row_stride, uint64_t *witness_dev, size_t col_stride, size_t col_len,
                              uint64_t *out_acc_dev, uint64_t *out_n_dev, uint32_t *flags_dev, unsigned bit);

/* endosclmul.rs gen_witness: 4 bits of chals_dev[i] (n x 2 canonical limbs) per row, most significant of the num_bits first (a multiple of 4 from 4 to
 * 128), num_bits / 4 rows + the closing row (cells 0, 1, 4, 5, 6) per instance.  endo: 4 host limbs, VerifierIndex::endo (what kh_gate_constants takes).
 * out_acc_dev, out_n_dev, flags_dev, bit as above; the zero denominators are the two of each half-step and (x_p - x_r)(x_r - x_s).  Scratch as above
 * with num_bits / 2 + 1 accumulators and num_bits / 4 more inversions per instance: 11.4 KB per 128-bit instance. */
int kh_endomul_witness_dev(int field, const uint64_t endo[4], const uint64_t *base_dev, const uint64_t *acc0_dev, const uint64_t *chals_dev,
                           unsigned num_bits, size_t n, const uint32_t *rows, size_t row0, size_t row_stride, uint64_t *witness_dev, size_t col_stride,
                           size_t col_len, uint64_t *out_acc_dev, uint64_t *out_n_dev, uint32_t *flags_dev, unsigned bit);

/* Tuning knob (process-wide): kh_varbasemul_witness_dev and kh_endomul_witness_dev take as many instances at a time as keep the slice's batch inversion
 * within `elements` field elements; default and maximum 2^22 (what one scan takes), 0 = the default.  The same values are written either way; the tests
 * set it to run several slices at small sizes. */
int kh_curve_witness_set_slice_elements(size_t elements);

/* endomul_scalar.rs gen_witness: 16 bits of chals_dev[i] (n x 2 canonical limbs) per row, most significant of the num_bits first (a multiple of 16 from
 * 16 to 128), num_bits / 16 rows per instance, cells 0..13 = n0 n8 a0 b0 a8 b8 x0..x7.  out_dev (nullable, n x 4): a * endo_scalar + b, the scalar the
 * challenge stands for; endo_scalar: 4 host limbs (Montgomery), required with out_dev.  One lane per instance, additions only. */
int kh_endomul_scalar_witness_dev(int field, const uint64_t *chals_dev, unsigned num_bits, size_t n, const uint32_t *rows, size_t row0, size_t row_stride,
                                  uint64_t *witness_dev, size_t col_stride, size_t col_len, const uint64_t endo_scalar[4], uint64_t *out_dev);

/* ---- The optional gates' witness on the device (csrc/limb_gadgets.hip) ----
 * RangeCheck0 / RangeCheck1 (the multi-range-check), Xor16, Rot64, ForeignFieldAdd and ForeignFieldMul: with the two blocks above, the witness of every
 * gate of the library, written in place from 8 to 96 bytes of input per instance.  The conventions are those of the Poseidon and curve-gate blocks.
 * witness_dev: 15 columns, column c at witness_dev + 4 * c * col_stride, col_len rows each.  Instance i starts at row rows[i] (host array, copied
 * before the call returns), or at row0 + i * row_stride when rows == NULL.  The calls are vector steps: queued on the main stream of the calling
 * thread's current context and ordered against every other call of the library -- a producer followed by a consumer needs no kh_sync; none of them
 * waits for the device.  n == 0 is KH_OK with nothing launched.  KH_E_INVALID with a kh_last_error text that names the call, before anything is
 * launched and with nothing written: an unknown field, a null pointer with n > 0, a misaligned device pointer, byte counts that overflow, an
 * instance that does not fit col_len (naming it), row_stride smaller than the instance's row count when rows == NULL, col_stride < col_len, a bad
 * compact, bits, rot, sign or modulus.  Overlapping instances are the caller's responsibility.
 * Inputs are plain integers, not field elements: an 88-bit limb is two uint64_t, little-endian, 16-byte aligned; a foreign element or a range-check
 * triple is three limbs (48 bytes, least significant limb first); Rot64 words are one uint64_t each (8-byte aligned); Xor operands are 4 uint64_t,
 * little-endian (16-byte aligned).  Every cell written is the canonical Montgomery element of the integer the tables below give (a negative one reduced
 * mod p: carry = -1 is p - 1).  bits(v, lo, hi) is bits lo .. hi - 1 of v, L = 2^88.
 * flags_dev, bit: as for kh_check_equal_dev and kh_varbasemul_witness_dev -- bit `bit` (< 32) of a caller-zeroed device uint32_t (nullable) is set
 * when any instance's input is out of range, and is not touched otherwise.  That instance's own cells are unspecified (inside its own rows); every
 * other instance of the call is exact.
 * One lane per (instance, row): a wave's store to a column covers consecutive rows when the instances are packed densely. */

/* host only, no device: the coefficients a gate list for kh_prover_index_create* carries on the foreign-field rows of the modulus f (3 limbs of two
 * uint64_t, not zero, each < 2^88; nf = 2^264 - f in limbs) -- ForeignFieldMul's four (f2, nf0, nf1, nf2), then ForeignFieldAdd's three (f0, f1, f2;
 * the caller appends the sign); out: 7 x 4 Montgomery limbs */
int kh_foreign_field_gate_coefficients(int field, const uint64_t modulus[6], uint64_t *out);

/* The multi-range-check (range_check/witness.rs): limbs_dev = n x 3 limbs v0 v1 v2; 4 rows per instance -- RangeCheck0, RangeCheck0, RangeCheck1,
 * Zero --, all 60 cells written.  The rows carry (x0, x1, x2) = (v0, v1, v2), or (v2, v0, v1) when compact == 1 (the gate list's second row then has
 * coefficient 0 = 1).
 *   rows 0, 1 (x = x0, x1):  col 0 = x;  col 1 + k = bits(x, 76 - 12 k, 88 - 12 k), k = 0..5;  col 7 + k = bits(x, 14 - 2 k, 16 - 2 k), k = 0..7
 *   row 2:  col 0 = x2;  col 1 = 0, or v0 + L v1 when compact;  col 2 = bits(x2, 86, 88);  col 3 + k = bits(x2, 74 - 12 k, 86 - 12 k), k = 0..3;
 *           col 7 + k = bits(x2, 36 - 2 k, 38 - 2 k), k = 0..7
 *   row 3:  cols 0, 1, 2 = bits(x2, 20, 22), bits(x2, 18, 20), bits(x2, 16, 18);  cols 3, 4 = row 0's cols 1, 2;  cols 5, 6 = row 1's cols 1, 2;
 *           col 7 + k = bits(x2, 14 - 2 k, 16 - 2 k), k = 0..7
 * The flag is set when a limb is >= 2^88. */
int kh_range_check_witness_dev(int field, const uint64_t *limbs_dev, size_t n, int compact, const uint32_t *rows, size_t row0, size_t row_stride,
                               uint64_t *witness_dev, size_t col_stride, size_t col_len, uint32_t *flags_dev, unsigned bit);

/* xor.rs create_xor_witness: in1_dev, in2_dev = n x 4 words; bits from 1 to 254; ceil(bits / 16) Xor16 rows + the closing row per instance, all 15
 * cells of each written, the closing row zero.  Row i: cols 0, 1, 2 = in1 >> 16 i, in2 >> 16 i, (in1 ^ in2) >> 16 i; cols 3..6, 7..10, 11..14 = the
 * four low nybbles of each of those, lowest first.  out_dev (nullable): n x 4 words, in1 ^ in2.  The flag is set when an operand is >= 2^bits. */
int kh_xor_witness_dev(int field, const uint64_t *in1_dev, const uint64_t *in2_dev, unsigned bits, size_t n, const uint32_t *rows, size_t row0,
                       size_t row_stride, uint64_t *witness_dev, size_t col_stride, size_t col_len, uint64_t *out_dev, uint32_t *flags_dev, unsigned bit);

/* rot.rs create_witness: words_dev = n words, rotated left by rot (0..63; the gate list's Rot64 row has coefficient 0 = 2^rot); 3 rows per instance,
 * all 45 cells written.  excess = (w << rot) >> 64, shifted = (w << rot) mod 2^64, rotated = shifted + excess, bound = excess - 2^rot + 2^64.
 *   row 0 (Rot64):  cols 0, 1, 2 = w, rotated, excess;  col 3 + k = bits(bound, 52 - 12 k, 64 - 12 k), k = 0..3;
 *                   col 7 + k = bits(bound, 14 - 2 k, 16 - 2 k), k = 0..7
 *   rows 1, 2:      the RangeCheck0 rows of shifted and of excess, as rows 0, 1 of kh_range_check_witness_dev
 * out_dev (nullable): n words, rotated. */
int kh_rot64_witness_dev(int field, const uint64_t *words_dev, unsigned rot, size_t n, const uint32_t *rows, size_t row0, size_t row_stride,
                         uint64_t *witness_dev, size_t col_stride, size_t col_len, uint64_t *out_dev);

/* foreign_field_add/witness.rs, one operation per instance: left_dev, right_dev = n x 3 limbs; sign = +1 or -1.  r = left + sign right - overflow f
 * with overflow in {0, sign} such that 0 <= r < f; carry = (lo(left) + sign lo(right) - overflow lo(f) - lo(r)) / 2^176 with lo(x) = x0 + L x1, one
 * of -1, 0, 1.  Written: cells 0..7 of the gate row -- left limbs, right limbs, overflow, carry -- and cells 0..2 of the next row, the limbs of r.
 * NOTHING else.  An instance counts as 2 rows; a chain whose operations share their result rows is placed through rows[].  out_dev (nullable):
 * n x 3 limbs, r.  The flag is set when no such r exists: an operand >= f, or a limb >= 2^88.  (The final bound row of the reference's chain gadget
 * is not written by this call.) */
int kh_foreign_field_add_witness_dev(int field, const uint64_t modulus[6], const uint64_t *left_dev, const uint64_t *right_dev, int sign, size_t n,
                                     const uint32_t *rows, size_t row0, size_t row_stride, uint64_t *witness_dev, size_t col_stride, size_t col_len,
                                     uint64_t *out_dev, uint32_t *flags_dev, unsigned bit);

/* foreign_field_mul/witness.rs: a_dev, b_dev = n x 3 limbs; 2 rows per instance, ForeignFieldMul and Zero.  (q, r) = divmod(a b, f), exact;
 * nf = 2^264 - f in limbs;  p0 = a0 b0 + q0 nf0,  p1 = a0 b1 + a1 b0 + q0 nf1 + q1 nf0,  p2 = a0 b2 + a2 b0 + a1 b1 + q0 nf2 + q2 nf0 + q1 nf1;
 * p1_lo = p1 mod L, p1_hi = p1 >> 88, p1_hi0 = p1_hi mod L, p1_hi1 = p1_hi >> 88;  carry0 = (p0 + L p1_lo - r0 - L r1) >> 176;
 * carry1 = (p2 + p1_hi + carry0 - r2) >> 88.
 *   gate row, all 15 cells:  cols 0..2 = a;  cols 3..5 = b;  col 6 = p1_lo;  col 7 + k = bits(carry1, 12 k, 12 k + 12), k = 0..3;
 *                            cols 11, 12, 13 = bits(carry1, 84, 86), (86, 88), (88, 90);  col 14 = bits(carry1, 90, 91)
 *   next row, cells 0..11:   col 0 = r0 + L r1;  col 1 = r2;  cols 2..4 = q;  col 5 = q2 + L - f2 - 1;  col 6 = p1_hi0;  col 7 = p1_hi1;
 *                            col 8 + k = bits(carry1, 48 + 12 k, 60 + 12 k), k = 0..2;  col 11 = carry0.  Cells 12..14 are NOT written.
 * out_checks_dev (nullable): n x 9 limbs -- (q0, q1, q2), (r0, r1, r2), (q2 + L - f2 - 1, p1_lo, p1_hi0) --, three triples in the input format of
 * kh_range_check_witness_dev: the gate's external range checks are one call of that with 3 n instances and no host round trip.
 * The flag is set when an input limb is >= 2^88 or a value does not fit its cell: q >= 2^264, carry0 >= 4, p1_hi1 >= 4, carry1 >= 2^91.
 * The division is Barrett's, with mu = floor(2^528 / f) computed on the host per call and the full product: a fixed trip count, no lane diverges. */
int kh_foreign_field_mul_witness_dev(int field, const uint64_t modulus[6], const uint64_t *a_dev, const uint64_t *b_dev, size_t n, const uint32_t *rows,
                                     size_t row0, size_t row_stride, uint64_t *witness_dev, size_t col_stride, size_t col_len, uint64_t *out_checks_dev,
                                     uint32_t *flags_dev, unsigned bit);

/* ---- Wires between the gadgets on the device (csrc/wiring.hip) ----
 * A gadget leaves its result in a witness cell as a Montgomery element; the next one takes its input in a format of its own.  Two cell-level calls
 * convert between cells and every input format of the three blocks above, and one writes the generic rows between gadgets, so that a circuit's
 * witness is chained on the device without a download, a host conversion, an upload and a kh_sync per hop.
 * cells: a host array of n (row, column) pairs, in the order of `wires` in kh_prover_index_create, copied before the call returns.  Any of the 15
 * columns is allowed; only columns 0..6 carry copy constraints.  witness_dev, col_stride, col_len as above.  The calls are vector steps: queued on the
 * main stream of the calling thread's current context and ordered against every other call of the library; none of them waits for the device.
 * n == 0 is KH_OK with nothing launched.  KH_E_INVALID with a kh_last_error text that names the call, before anything is launched and with nothing
 * written: an unknown field or format, half not 0 or 1, a null pointer with n > 0, a misaligned device pointer (16 bytes; 8 for KH_CELL_U64 data),
 * byte counts that overflow, col_stride < col_len, a cell with row >= col_len or column >= 15 (naming its index), a generic instance that does not fit.
 * flags_dev, bit: as for kh_check_equal_dev and the limb gadgets -- bit `bit` (< 32) of a caller-zeroed device uint32_t (nullable) is set when any
 * value of the call does not fit its format, and is not touched otherwise.  Every other value of the call is exact.
 * One lane per cell or instance: a cell is one 32-byte access wherever it lies, the dense side is consecutive across the wave. */
enum { KH_CELL_FIELD = 0,   /* 4 words: the cell as it is, a Montgomery element                          */
       KH_CELL_INT256 = 1,  /* 4 words: the canonical integer (< p) -- scalars_dev, Xor operands         */
       KH_CELL_INT128 = 2,  /* 2 words -- chals_dev of EndoMul / EndoMulScalar                           */
       KH_CELL_LIMB88 = 3,  /* 2 words, value < 2^88 -- the limb of the range-check / foreign-field calls */
       KH_CELL_U64 = 4 };   /* 1 word -- the Rot64 word                                                  */

/* out_dev[i] = cell i in `format`, packed densely (4, 4, 2, 2 or 1 words each).  KH_CELL_FIELD copies the four limbs: no arithmetic, never a flag.
 * The other formats deliver v, the canonical integer the cell stands for (one Montgomery product by 1 and the final reduction): KH_CELL_INT256 all of
 * it; KH_CELL_INT128, KH_CELL_LIMB88 and KH_CELL_U64 its low 128, 88 or 64 bits -- exactly those, also when the flag is set, which it is when
 * v >= 2^128, 2^88 or 2^64.  Cells may repeat.  The witness is not written; out_dev must not overlap it.  Cells are assumed canonical (< p) and are
 * not checked. */
int kh_witness_gather_dev(int field, const uint64_t *witness_dev, size_t col_stride, size_t col_len,
                          const uint32_t *cells /* host, n x 2: (row, column) */, size_t n, int format,
                          uint64_t *out_dev, uint32_t *flags_dev, unsigned bit);

/* Cell i becomes the canonical Montgomery element of values_dev[i] (KH_CELL_FIELD: copied as it is).  The flag is set by a KH_CELL_INT256 value >= p
 * and by a KH_CELL_LIMB88 value >= 2^88; such a cell is unspecified.  NOTHING else is written.  Target cells that repeat are the caller's
 * responsibility.  A cell-to-cell copy is a KH_CELL_FIELD gather followed by a KH_CELL_FIELD scatter. */
int kh_witness_scatter_dev(int field, const uint64_t *values_dev, int format,
                           const uint32_t *cells /* host, n x 2 */, size_t n,
                           uint64_t *witness_dev, size_t col_stride, size_t col_len,
                           uint32_t *flags_dev, unsigned bit);

/* generic.rs: one half of a double generic row per instance, an instance being ONE row placed like a gadget's (rows[i], or row0 + i * row_stride).
 * half 0 writes cells 0, 1, 2, half 1 cells 3, 4, 5: l, r and o = -(c_l l + c_r r + c_m l r + c_c) / c_o, NOTHING else -- two calls with half 0 and 1
 * may target the same rows.  coeffs: that half's five coefficients in generic.rs order, l r o m c (coefficients 5 * half .. 5 * half + 4 of the gate
 * row), canonical Montgomery limbs on the host.  1 / c_o is computed once per call on the host: no lane inverts.  c_o = 0 (a constant or a public
 * input: the row constrains l and defines nothing) writes o = 0, as the reference's generators leave it.  l_dev, r_dev: n x 4 Montgomery limbs
 * (r_dev nullable: r = 0).  out_dev (nullable): the n values of o, Montgomery. */
int kh_generic_witness_dev(int field, const uint64_t coeffs[20] /* host: l r o m c, Montgomery */, int half,
                           const uint64_t *l_dev, const uint64_t *r_dev /* nullable: r = 0 */, size_t n,
                           const uint32_t *rows, size_t row0, size_t row_stride,
                           uint64_t *witness_dev, size_t col_stride, size_t col_len, uint64_t *out_dev /* nullable */);

/* ---- GateType::Lookup rows on the device: the values a circuit reads from a ROM / RAM table (csrc/lookup_rows.hip) ----
 * A Lookup row holds (table id, key, value, key, value, key, value).  The circuit knows the keys; the values are what the table holds at them, and
 * in a runtime table they arrive with each proof.  An instance is ONE row, placed like every gadget's (rows[i], or row0 + i * row_stride with
 * row_stride >= 1).  table_keys_dev, table_values_dev: table_len elements each, two columns of a table's rows -- typically column 0 and column 1 of
 * the combined table at that table's rows (kh_prover_index_lookup_table), or a runtime table's first column and the caller's own runtime values.
 * keys_dev: n x 3 elements.  For instance i and slot k = 0, 1, 2: t = the LOWEST index with table_keys_dev[t] == keys_dev[3 i + k] (elements are
 * compared as 32-byte strings: canonical Montgomery limbs are unique; inputs are assumed canonical and are not checked), the value is
 * table_values_dev[t].  Written per instance: cell 0 = table_id, cell 2 k + 1 = the key, cell 2 k + 2 = the value, NOTHING else -- cells 7..14 stay
 * as they are.  out_values_dev (nullable): n x 3 elements, the values.  The Lookup pattern always makes three lookups per row: a row that needs
 * fewer repeats a key.
 * A key that is in no row of the table sets bit `bit` of *flags_dev (the rules of the limb gadgets: a caller-zeroed device uint32_t, nullable, not
 * touched otherwise) and gets the zero element as its value, in the cell and in out_values_dev; every other slot and instance is exact.
 * The call reads only the two columns it is given.  On a table wider than two columns the row satisfies the pattern only where the further columns
 * are zero at row t, and table_id must be that table's id: both are the caller's responsibility, no flag is raised for them, and
 * kh_witness_check_full (KH_WITNESS_LOOKUPS) names a row that gets either wrong.
 * A vector step like the gadget calls: queued on the main stream of the calling thread's current context, ordered against every other call, and it
 * does not wait for the device; n == 0 is KH_OK with nothing launched.  The hash set over the table's keys is built per call in a block of the
 * kh_dev_alloc pool (a power of two of at least 2 table_len 32-bit slots).  KH_E_INVALID with a kh_last_error text that names the call, before
 * anything is launched and with nothing written: what the gadget calls refuse (field, null / misaligned device pointers, col_stride < col_len, byte
 * counts, an instance outside col_len rows), a null table_id or one >= p, table_len == 0 or >= 2^31, null or misaligned (16 bytes) table columns,
 * 3 n lanes that overflow a grid, a misaligned flag word or bit >= 32. */
int kh_lookup_witness_dev(int field, const uint64_t table_id[4] /* host, Montgomery, < p */,
                          const uint64_t *table_keys_dev, const uint64_t *table_values_dev, size_t table_len,
                          const uint64_t *keys_dev /* n x 3 x 4 limbs */, size_t n,
                          const uint32_t *rows, size_t row0, size_t row_stride,
                          uint64_t *witness_dev, size_t col_stride, size_t col_len,
                          uint64_t *out_values_dev /* nullable, n x 3 x 4 */, uint32_t *flags_dev, unsigned bit);

/* ---- Witness advice on the device: the inverse of a value, a square root, the bits of a value (csrc/value_steps.hip) ----
 * The witness values that no gate computes and the prover supplies: the inverse behind every is_zero / equals / division, the square root of a point
 * decompression or an is_square, the bits behind range and comparison logic.  A VALUE step reads a dense device array and writes a dense device
 * array: it writes no witness cell and has no placement; a KH_CELL_FIELD scatter, a generic row (l_dev / r_dev) or a gadget call consumes the result.
 * Elements are 4 x u64 Montgomery limbs.  Inputs are assumed canonical (< p) and are not compared with p, like witness_dev: a non-canonical input
 * gives an unspecified value for that element only, and every kernel ends whatever it is given (every loop has a constant trip bound).
 * flags_dev, bit: the rules of the gadget calls -- bit `bit` (< 32) of a caller-zeroed device uint32_t (nullable) is set with one atomicOr per wave,
 * and only by a wave in which some lane raises it; it is not touched otherwise.
 * Vector steps: queued on the main stream of the calling thread's current context and ordered against every other call; NONE of them waits for the
 * device (kh_batch_inversion_dev does, for its host turn).  n == 0 is KH_OK with nothing launched.  KH_E_INVALID with a kh_last_error text that names
 * the call, before anything is launched and with nothing written: an unknown field, a null in_dev / out_dev with n > 0, a misaligned device pointer
 * (16 bytes; 8 for KH_CELL_U64 data), an unknown format, num_bits outside 1..255 or above 64 x the format's words, n > 2^36 (the grid), a flag bit
 * >= 32 or a misaligned flag word.  No pool scratch, no LDS, no per-lane scratch memory.
 *
 * kh_field_inverse_dev: out[i] = in[i]^-1.  A zero input gives zero AND raises the bit: that is the "inverse or zero" advice of is_zero, whose caller
 * passes flags_dev = NULL (KH_STEP_NO_FLAG in a schedule).  out_dev == in_dev is allowed; any other overlap is the caller's responsibility.  Each
 * lane inverts a run of 4 elements with Montgomery's trick and ONE Fermat chain: about 85 products per element instead of 330.
 *
 * kh_field_sqrt_dev: out[i] = the root ark-ff's Tonelli-Shanks returns for in[i] (SqrtPrecomputation::TonelliShanks; no sign normalisation -- the
 * function the SRS generator uses).  Zero gives zero, a success that raises nothing.  A non-residue gives zero and raises the bit.
 * out_is_square_dev (nullable): n elements, the Montgomery 1 or 0; zero counts as a square.  out_dev == in_dev is allowed.
 *
 * kh_field_bits_dev: in_dev holds n values in `format`, exactly as kh_witness_gather_dev delivers them: KH_CELL_FIELD a Montgomery element, whose
 * canonical integer is taken; the other formats plain integers of 4, 2, 2 or 1 words.  out_dev receives num_bits x n elements, BIT-MAJOR: bit k
 * (least significant first) of value i is element k n + i, the Montgomery 0 or 1 -- "bit k of every value" is a contiguous n-array that a generic
 * row takes as l_dev / r_dev and a scatter puts into one column of cells.  A value >= 2^num_bits raises the bit; its low num_bits bits are written
 * regardless.  out_dev must not overlap in_dev. */
int kh_field_inverse_dev(int field, const uint64_t *in_dev, size_t n, uint64_t *out_dev, uint32_t *flags_dev, unsigned bit);
int kh_field_sqrt_dev(int field, const uint64_t *in_dev, size_t n, uint64_t *out_dev,
                      uint64_t *out_is_square_dev /* nullable */, uint32_t *flags_dev, unsigned bit);
int kh_field_bits_dev(int field, const uint64_t *in_dev, int format, unsigned num_bits, size_t n,
                      uint64_t *out_dev /* num_bits x n x 4 limbs */, uint32_t *flags_dev, unsigned bit);

/* ---- Witness schedule: a circuit's gadget and wire steps compiled once, run per proof (csrc/witness_schedule.cpp, csrc/wiring.hip) ----
 * The circuit is fixed when its index is created and only the inputs change from proof to proof.  A schedule is the witness-side counterpart of
 * kh_prover_index_create: the list of direct calls above that writes a circuit's witness, described once.  kh_witness_schedule_create does everything
 * that depends only on the circuit -- every check of the direct calls, against col_len; the rows[] and cells tables uploaded into ONE resident device
 * block; the host-side constants (a generic half's coefficients over -c_o, ForeignFieldMul's Barrett constant) -- and kh_witness_schedule_run produces
 * one proof's witness_dev with one call that uploads nothing and checks nothing per cell.
 * A step is ONE direct call and means exactly what that call means with these arguments: same cells written, same values, same flag rules, NOTHING
 * else is written.  n, rows / row0 / row_stride, cells / format, sign are the direct call's; a device pointer of the direct call is a kh_witness_ref_t:
 * buf >= 0 is bufs_dev[buf] + offset bytes of the run, KH_REF_ARENA the run's own scratch arena + offset, KH_REF_NONE a nullable argument left out.
 * in[] are the call's device inputs in their order, out[] its nullable device outputs in their order; rows, cells and consts are host arrays copied
 * at create.
 *   op                       direct call                          in[0]       in[1]     in[2]        out[0]          out[1]     param     consts
 *   KH_STEP_GATHER           kh_witness_gather_dev                -           -         -            out_dev (req.)  -          -         -
 *   KH_STEP_SCATTER          kh_witness_scatter_dev               values_dev  -         -            -               -          -         -
 *   KH_STEP_GENERIC          kh_generic_witness_dev               l_dev       r_dev *   -            out_dev         -          half      coeffs[20]
 *   KH_STEP_POSEIDON         kh_poseidon_gate_witness_dev         states_dev  -         -            out_states_dev  -          -         -
 *   KH_STEP_COMPLETE_ADD     kh_complete_add_witness_dev          p1_dev      p2_dev    -            out_dev         -          -         -
 *   KH_STEP_VARBASEMUL       kh_varbasemul_witness_dev            base_dev    acc0_dev  scalars_dev  out_acc_dev     out_n_dev  num_bits  -
 *   KH_STEP_ENDOMUL          kh_endomul_witness_dev               base_dev    acc0_dev  chals_dev    out_acc_dev     out_n_dev  num_bits  endo[4]
 *   KH_STEP_ENDOMUL_SCALAR   kh_endomul_scalar_witness_dev        chals_dev   -         -            out_dev         -          num_bits  endo_scalar[4] *
 *   KH_STEP_RANGE_CHECK      kh_range_check_witness_dev           limbs_dev   -         -            -               -          compact   -
 *   KH_STEP_XOR              kh_xor_witness_dev                   in1_dev     in2_dev   -            out_dev         -          bits      -
 *   KH_STEP_ROT64            kh_rot64_witness_dev                 words_dev   -         -            out_dev         -          rot       -
 *   KH_STEP_FF_ADD           kh_foreign_field_add_witness_dev     left_dev    right_dev -            out_dev         -          -         modulus[6]
 *   KH_STEP_FF_MUL           kh_foreign_field_mul_witness_dev     a_dev       b_dev     -            out_checks_dev  -          -         modulus[6]
 *   KH_STEP_LOOKUP           kh_lookup_witness_dev                keys_dev    table_keys_dev  table_values_dev  out_values_dev  -  table_len  table_id[4]
 *   KH_STEP_INVERSE          kh_field_inverse_dev                 in_dev      -         -            out_dev (req.)  -          -         -
 *   KH_STEP_SQRT             kh_field_sqrt_dev                    in_dev      -         -            out_dev (req.)  out_is_square_dev  -  -
 *   KH_STEP_BITS             kh_field_bits_dev                    in_dev      -         -            out_dev (req.)  -          num_bits  -          (format: the input's)
 * (* nullable as in the direct call; every out[] but the gather's and the value steps' out[0] is nullable; refs and fields a call does not have are ignored.)  flag_bit: the
 * direct call's `bit` on the run's flags_dev, or KH_STEP_NO_FLAG for a step that passes flags_dev = NULL; calls without a flag ignore it.
 * An arena extent is n instances of the argument's size, except the Lookup step's in[1] and in[2], which are its table: table_len x 32 bytes
 * whatever n is (normally bound buffers: the pointers of kh_prover_index_lookup_table, the run's runtime values), and the BITS step's out[0]:
 * n x num_bits x 32 bytes.  The three value steps (kh_field_*_dev) write no witness cell and have no placement: rows, row0, row_stride and cells are
 * ignored.  Each is one launch group and, like every step that is not a wire step, ends a fused group.
 * A run is equivalent to the direct calls issued in step order on the calling thread's current context: a vector step like them, queued on that
 * context's main stream and ordered against every other call -- a consumer (kh_witness_check, kh_prove) needs no kh_sync --, and it waits for the
 * device only where they do (once per slice in VarBaseMul / EndoMul steps).  The arena (arena_bytes, not zeroed), the chain steps' scratch and the
 * Lookup steps' slots come from the kh_dev_alloc pool for the time of the run, so a schedule is immutable after create and may be run from several threads and contexts of its
 * device at once.
 * Wire steps are many and tiny.  Consecutive KH_STEP_GATHER steps whose out[0] is in the arena run as ONE launch (k_cell_moves, one lane per cell, formats
 * and flag bits mixed inside a wave), and likewise consecutive KH_STEP_SCATTER steps whose in[0] is; a step starts a new group where fusing would
 * change the result of running the steps one after another: a gather whose output extent overlaps an earlier output of the group, a scatter with a
 * target cell the group already targets.  A wire step on a caller buffer runs on its own like the direct call.
 * kh_witness_schedule_create: KH_E_INVALID, *out untouched, with a kh_last_error text that names the step and, for a table entry, its index
 * ("kh_witness_schedule_create: step 7 (KH_STEP_GATHER): cell 3 at (row 300, column 0) is outside ...") for everything the direct call refuses, and
 * for a ref: buf >= n_bufs or below KH_REF_NONE, an offset not aligned as the direct call demands of that pointer, an arena extent past arena_bytes, a
 * required ref that is KH_REF_NONE; an unknown op; flag_bit >= 32 that is not KH_STEP_NO_FLAG.  It waits for its upload: the schedule is ready when
 * it returns.
 * kh_witness_schedule_run checks only what changes between runs -- n_bufs is the schedule's, bufs_dev[k] / witness_dev non-null and 16-byte aligned,
 * flags_dev 4-byte aligned (nullable: no step raises a flag), col_stride >= col_len, byte counts -- and returns KH_E_INVALID before anything is
 * launched and with nothing written.  Its host work is O(steps); nothing goes through the staging ring (kh_counter("table_staged_words")).
 * kh_witness_schedule_info: steps; launch_groups = the launcher invocations a run makes (a fused group counts once, a step with n = 0 not at all);
 * resident_bytes = the device block holding the tables; run_bytes = what a run takes from the pool (arena + chain scratch at the current slice knob
 * + the Lookup steps' slots).
 * kh_witness_schedule_free: no run of the schedule may be in progress on another thread; queued device work is waited for. */
typedef struct kh_witness_schedule kh_witness_schedule_t;
#define KH_REF_NONE  (-2)   /* a nullable argument that is absent */
#define KH_REF_ARENA (-1)   /* the run's own scratch arena */
#define KH_STEP_NO_FLAG 255 /* flag_bit of a step that raises no flag */
enum { KH_STEP_GATHER = 0, KH_STEP_SCATTER = 1, KH_STEP_GENERIC = 2, KH_STEP_POSEIDON = 3, KH_STEP_COMPLETE_ADD = 4, KH_STEP_VARBASEMUL = 5,
       KH_STEP_ENDOMUL = 6, KH_STEP_ENDOMUL_SCALAR = 7, KH_STEP_RANGE_CHECK = 8, KH_STEP_XOR = 9, KH_STEP_ROT64 = 10, KH_STEP_FF_ADD = 11,
       KH_STEP_FF_MUL = 12,
       /* 13 stays unassigned: it is refused as an unknown op (the tests of the schedule use it as the op that does not exist) */
       KH_STEP_LOOKUP = 14,
       KH_STEP_INVERSE = 15, KH_STEP_SQRT = 16, KH_STEP_BITS = 17 };   /* the value steps: rows, row0, row_stride and cells are ignored */
typedef struct kh_witness_ref kh_witness_ref_t;
typedef struct kh_witness_step kh_witness_step_t;
struct kh_witness_ref { int buf; size_t offset; };   /* buf >= 0: bufs_dev[buf] of the run; offset in bytes */
struct kh_witness_step {
    int op;                                   /* KH_STEP_* */
    size_t n;                                 /* instances; cells for GATHER / SCATTER */
    const uint32_t *rows; size_t row0, row_stride;   /* placement of a gadget step, exactly as in the direct call */
    const uint32_t *cells; int format;        /* GATHER / SCATTER: n (row, column) pairs, KH_CELL_*; BITS: the format of in[0] */
    unsigned param;                           /* num_bits | bits | rot | compact | half | table_len, as the direct call names it */
    int sign;                                 /* ForeignFieldAdd */
    const uint64_t *consts;                   /* host, copied at create: endo[4] | endo_scalar[4] | modulus[6] | coeffs[20] | table_id[4] | Poseidon none */
    kh_witness_ref_t in[3], out[2];
    unsigned flag_bit;                        /* < 32, or KH_STEP_NO_FLAG */
};
int kh_witness_schedule_create(int field, size_t col_len, const kh_witness_step_t *steps, size_t n_steps,
                               size_t arena_bytes, size_t n_bufs, kh_witness_schedule_t **out);
int kh_witness_schedule_run(const kh_witness_schedule_t *s, void *const *bufs_dev, size_t n_bufs,
                            uint64_t *witness_dev, size_t col_stride, uint32_t *flags_dev);
int kh_witness_schedule_info(const kh_witness_schedule_t *s, size_t *steps, size_t *launch_groups,
                             size_t *resident_bytes, size_t *run_bytes);
void kh_witness_schedule_free(kh_witness_schedule_t *s);

/* ---- scans, batch inversion, division by a linear factor: the permutation argument's vector steps ----
 * kh_field_scan_dev: in-place inclusive prefix (reverse = 0) or suffix (reverse = 1) scan under + or *
 *   (the running product z[j+1] = z[j] * ..., kimchi/src/circuits/polynomials/permutation.rs:556-563).
 * kh_batch_inversion_dev = ark_ff::batch_inversion (permutation.rs:533): non-zero entries inverted, zeros kept.
 * kh_divide_by_linear_dev: f = q (x - a) + rem (the two boundary quotients (z - 1)/(x - 1), (z - 1)/(x - sid[n - zk])
 *   of perm_quot, permutation.rs:300-327): q_dev gets len - 1 coefficients, rem = f(a) comes back to the host
 *   (the reference returns an error when it is non-zero). */
enum { KH_SCAN_ADD = 0, KH_SCAN_MUL = 1 };
int kh_field_scan_dev(int field, int op, int reverse, uint64_t *data_dev, size_t n);
int kh_batch_inversion_dev(int field, uint64_t *v_dev, size_t n);
int kh_divide_by_linear_dev(int field, const uint64_t *f_dev, size_t len, const uint64_t a[4], uint64_t *q_dev, uint64_t rem[4]);
/* The same division with the remainder left ON THE DEVICE (rem_dev: 4 limbs, nullable) -- nothing waits for the stream -- and a deferred check:
 * kh_check_equal_dev sets bit `bit` of *flags_dev (a uint32_t in device memory the caller zeroed) when any of the n elements at v_dev differs
 * from `expect` (4 limbs; NULL = zero).  A device-resident prover queues its invariants (remainders are zero, the accumulators end at 1:
 * prover.rs:913-917, permutation.rs:301-321, 566-568) behind the steps that produce them and reads the one word at the end of the proof, instead
 * of stalling the stream once per check; both are asynchronous on the library's main stream like the other vector steps. */
int kh_divide_by_linear_async_dev(int field, const uint64_t *f_dev, size_t len, const uint64_t a[4], uint64_t *q_dev, uint64_t *rem_dev);
int kh_check_equal_dev(const uint64_t *v_dev, size_t n, const uint64_t *expect, uint32_t *flags_dev, unsigned bit);

/* ---- challenge polynomials (verifier side) ----
 * kh_b_poly_coefficients = b_poly_coefficients (poly-commitment/src/commitment.rs:464-476) for k challenge sets of
 * `rounds` challenges each (k x rounds x 4 limbs, Montgomery): out[j][i] = prod_{bit b of i} chals[j][rounds-1-b],
 * k x 2^rounds x 4 limbs.
 * kh_batch_dlog_accumulator_generate (utils.rs:282-312): comms[j] = <b_poly_coefficients(chals_j), g>, coefficient
 * vectors built and consumed on the device (one batched MSM over the resident tables).
 * kh_batch_dlog_accumulator_check (utils.rs:212-273): *ok = [ sum_j r^j (C_j - <s_j, g>) == 0 ]; the reference draws
 * r from OsRng inside the function, here the caller passes it (Montgomery limbs).  Size mismatches that are
 * assert!s in the reference return KH_E_INVALID. */
int kh_b_poly_coefficients(int field, const uint64_t *chals, unsigned rounds, size_t k, uint64_t *out);
int kh_batch_dlog_accumulator_generate(kh_srs_t *srs, size_t num_comms, const uint64_t *chals, size_t chals_len,
                                       uint64_t *out_xy, uint8_t *out_inf);
int kh_batch_dlog_accumulator_check(kh_srs_t *srs, const uint64_t *comms_xy, const uint8_t *comms_inf, size_t k,
                                    const uint64_t *chals, size_t chals_len, const uint64_t r[4], int *ok);
/* The single MSM of the batch verifier SRS::verify (poly-commitment/src/ipa.rs:301-502):
 *   sum_i sg_weights[i] <b_poly_coefficients(chals_i), g>  +  sum_j extra_scalars[j] extra_j   == 0 ?
 * The k challenge polynomials (k x rounds challenges, 2^rounds = SRS size) are expanded on the device and multiplied
 * into the resident tables (ipa.rs:402-420); the proof-specific terms (H, sg, U, L/R, the commitments, delta with the
 * scalars of ipa.rs:405-470, all computed by the caller next to its sponge) go through the ad-hoc MSM. */
int kh_ipa_verify_msm(kh_srs_t *srs, const uint64_t *chals, size_t chals_len, const uint64_t *sg_weights, size_t k,
                      const uint64_t *extra_xy, const uint8_t *extra_inf, const uint64_t *extra_scalars, size_t m, int *is_zero);

/* ---- the folding loop of SRS::open on the device (poly-commitment/src/ipa.rs:929-1007) ----
 * The caller keeps the sponge and the RNG (ipa.rs:940-941, 966-971); everything between two squeezes runs here
 * on device-resident vectors, so a round costs one host<->device hop of 2 points + 1 challenge:
 *
 *   kh_ipa_begin(srs, a = p.coeffs (a_len <= srs size, zero-padded as ipa.rs:918-920), b = b_init
 *                (padded_length entries), u_base = U)                                  -> state
 *   per round:  kh_ipa_round_lr(state, rand_l, rand_r) -> (L, R)      ipa.rs:943-961
 *               kh_ipa_round_fold(state, u_pre)        -> (u, u^-1)   ipa.rs:972-1006, u = u_pre.to_field(endo_r)
 *   kh_ipa_finish(state) -> a0 = a[0], b0 = b[0], sg = g[0]                             ipa.rs:1009-1018
 *
 * L, R and sg are the reference's group elements (bit-identical affine coordinates); the basis is never folded:
 * round j's L / R are MSMs over the SRS's resident window tables with the scalars a (x) (challenge tensor), and
 * sg = <challenge tensor, G>.  The blinding base H is the handle's (kh_srs_set_blinding_base);
 * the SRS size must be a power of two.  Up to KH_IPA_OPENINGS openings begun by DIFFERENT threads run over one handle's tables at the same time (each has
 * its own workspace on the handle and its own slot for U in the handle's tables); a further kh_ipa_begin waits until one of them is freed.  A thread
 * that begins a second opening on a handle before freeing its first gets KH_E_INVALID.
 * All field elements Montgomery limbs; u_pre as in kh_ipa_fold_points_endo. */
#define KH_IPA_OPENINGS 4          /* = KH_MSM_SLOTS: more openings than pipeline slots could not overlap anyway */
typedef struct kh_ipa kh_ipa_t;
int kh_ipa_begin(kh_srs_t *srs, const uint64_t *a, size_t a_len, const uint64_t *b, size_t b_len,
                 const uint64_t u_base_xy[8], kh_ipa_t **out);
/* same with a and b already in device memory (e.g. the outputs of kh_combine_polys_dev / kh_b_init_dev) */
int kh_ipa_begin_dev(kh_srs_t *srs, const uint64_t *a_dev, size_t a_len, const uint64_t *b_dev, size_t b_len,
                     const uint64_t u_base_xy[8], kh_ipa_t **out);
int kh_ipa_rounds_left(const kh_ipa_t *st);
int kh_ipa_round_lr(kh_ipa_t *st, const uint64_t rand_l[4], const uint64_t rand_r[4], uint64_t lr_xy[16], uint8_t lr_inf[2]);
int kh_ipa_round_fold(kh_ipa_t *st, const uint64_t chal[2], uint64_t u_out[4], uint64_t u_inv_out[4]);
int kh_ipa_finish(kh_ipa_t *st, uint64_t a0[4], uint64_t b0[4], uint64_t sg_xy[8], uint8_t *sg_inf);
void kh_ipa_free(kh_ipa_t *st);
/* Everything SRS::open does after combine_polys / b_init (ipa.rs:898-1060) in ONE call: absorbs shift_scalar(<a, b>), derives
 * U = to_group(challenge_fq()), runs the log2(n) rounds (L / R MSMs on the device, absorb, challenge, folds of a, b and of the
 * challenge tensor), then delta, c, z1, z2.  `sponge`: the prover's Fq-sponge (fq_sponge_before_evaluations, prover.rs:1193),
 * advanced exactly as the reference advances it.  `blinders`: what the reference draws from its RNG, in its order -- (rand_l,
 * rand_r) per round, then d, r_delta -- 2 log2(n) + 2 scalar-field elements.  blinding_factor: the combined blinder returned
 * by combine_polys.  Outputs: lr (log2(n) x 2 points), delta, z1, z2, sg: the OpeningProof (ipa.rs:1175-1191). */
int kh_ipa_open(kh_srs_t *srs, const uint64_t *a_dev, size_t a_len, const uint64_t *b_dev, size_t b_len, const uint64_t combined_inner_product[4],
                const uint64_t blinding_factor[4], kh_sponge_t *sponge, const uint64_t *blinders, size_t blinders_len,
                uint64_t *lr_xy, uint8_t *lr_inf, uint64_t delta_xy[8], uint8_t *delta_inf, uint64_t z1[4], uint64_t z2[4], uint64_t sg_xy[8], uint8_t *sg_inf);

/* PolyComm::multi_scalar_mul (poly-commitment/src/commitment.rs:350-394): m commitments with num_chunks[i] chunks each
 * (chunks_xy / chunks_inf: the chunk lists concatenated, sum(num_chunks) points), m scalars (Montgomery).
 * out chunk j = sum_{i : num_chunks[i] > j} scalars[i] * com_i.chunks[j]; *out_count = max(num_chunks), or 1 point
 * at infinity when m == 0 (the reference's empty case).  out_xy / out_inf need room for max(num_chunks, 1) points. */
int kh_polycomm_multi_scalar_mul(int curve, const uint64_t *chunks_xy, const uint8_t *chunks_inf, const size_t *num_chunks, size_t m,
                                 const uint64_t *scalars, uint64_t *out_xy, uint8_t *out_inf, size_t *out_count);

/* ---- commitment wrappers (host logic of the SRS trait over the MSM kernels) ----
 * kh_commit_non_hiding = SRS::commit_non_hiding (poly-commitment/src/ipa.rs:638-683):
 * coefficients (len x 4 limbs, Montgomery) are split into ceil(len / srs_size) chunks,
 * chunk j = sum_i coeffs[j*srs_size + i] * g[i]; the zero polynomial (all coefficients zero or
 * len == 0) commits to ONE point at infinity; the result is padded with infinities up to
 * num_chunks (never truncated).  out_xy / out_inf must have room for
 * max(num_chunks, ceil(len / srs_size), 1) entries; *out_count receives the number written. */
int kh_commit_non_hiding(kh_srs_t *srs, const uint64_t *coeffs, size_t len, size_t num_chunks,
                         uint64_t *out_xy, uint8_t *out_inf, size_t *out_count);
/* kh_commit_evaluations_non_hiding = SRS::commit_evaluations_non_hiding (ipa.rs:706-728 +
 * PolyComm::multi_scalar_mul, commitment.rs:350-394): evals live on a domain of size evals_len
 * (a power of two, >= 2^log2_domain; sub-sampled with stride evals_len >> log2_domain), and are
 * committed against the registered Lagrange basis; one output point per basis chunk.
 * A domain larger than the evaluations' domain is the reference's panic: returns KH_E_INVALID. */
int kh_commit_evaluations_non_hiding(kh_srs_t *srs, unsigned log2_domain, const uint64_t *evals, size_t evals_len,
                                     uint64_t *out_xy, uint8_t *out_inf, size_t *out_count);
/* Blinding base h of the SRS (ipa::SRS::h); defaults to SRS::create's h (ipa.rs:765-772).  Setting it while an opening is live on the handle
 * (between kh_ipa_begin and kh_ipa_free, on any thread) is refused with KH_E_INVALID: the openings' rounds read H from the handle's tables. */
int kh_srs_set_blinding_base(kh_srs_t *srs, const uint64_t h_xy[8]);
int kh_srs_get_blinding_base(const kh_srs_t *srs, uint64_t h_xy[8]);
/* kh_mask_custom = SRS::mask_custom (ipa.rs:605-622): out_j = blinders_j * h + com_j on the host
 * (one scalar multiplication per chunk: "negligible, stays on host").  A length mismatch is
 * CommitmentError::BlindersDontMatch: returns KH_E_BLINDERS. */
#define KH_E_BLINDERS (-5)
int kh_mask_custom(kh_srs_t *srs, const uint64_t *com_xy, const uint8_t *com_inf, size_t com_len,
                   const uint64_t *blinders /* Montgomery */, size_t blinders_len,
                   uint64_t *out_xy, uint8_t *out_inf);
/* omega_{2^k} of Radix2EvaluationDomain::new(2^k) (kimchi/src/circuits/domains.rs:40-69), Montgomery. */
int kh_domain_generator(int field, unsigned log2_n, uint64_t out[4]);

/* ---- NTT -------------------------------------------------------------------
 * Replaces Radix2EvaluationDomain::{fft_in_place, ifft_in_place} behind
 * Evaluations::interpolate[_by_ref] (kimchi/src/prover.rs:289,377,433,567,614,665,
 * 907,1163; circuits/polynomials/permutation.rs:571; poly-commitment/src/utils.rs:195-196).
 * data: batch x 2^log2_n x 4 limbs, Montgomery, natural order in and out, in place;
 * inverse != 0 includes the 1/N scaling (ark-poly ifft). */
int kh_ntt(int field, uint64_t *data, unsigned log2_n, int inverse, size_t batch);
/* Tuning knob (process-wide): the largest sub-transform of one pass is 2^max_logr points (4..10; 0 = the default, 9; KH_NTT_MAX_LOGR at start-up).
 * A transform of 2^k points runs in ceil(k / max_logr) passes; results are identical for every setting (the tests run the parity cases under 8, 9, 10). */
int kh_ntt_set_max_logr(unsigned max_logr);

/* DensePolynomial::evaluate_over_domain_by_ref(d8/d4) (kimchi/src/circuits/
 * constraints.rs:490-495; prover.rs:436,617,668): n = 2^log2_n coefficients,
 * zero-extended to n << log2_blowup and forward-transformed.
 * coeffs: batch x n x 4 limbs; out: batch x (n << log2_blowup) x 4 limbs. */
int kh_lde(int field, const uint64_t *coeffs, unsigned log2_n, unsigned log2_blowup,
           uint64_t *out, size_t batch);

/* ---- device-resident variants (no PCIe in the loop) -----------------------
 * Same operations on buffers that already live in HBM (hipMalloc'd by the caller or by
 * kh_dev_alloc).  These are what the benchmark times ("inputs already resident in HBM")
 * and what a prover that keeps witness columns on the device would call.
 * Ordering: kh_ntt_dev / kh_lde_dev / kh_coset_ntt_dev / kh_dev_copy and the vector steps whose result stays on the device
 * (kh_expr_evaluations_dev, kh_poly_lincomb_dev, kh_combine_polys_dev, kh_b_init_dev, kh_field_scan_dev, kh_batch_inversion_dev,
 * kh_divide_by_vanishing_poly_dev) return as soon as their kernels are queued on the library's main stream; their host
 * arguments (token programs, pointer tables, constants) are copied before the call returns.  Every
 * other entry point that consumes a device buffer either runs on that same stream or waits for it on the device
 * (MSMs on another pipeline slot's stream wait for an event recorded on the main stream), so a producer followed by a
 * consumer needs no kh_sync in between.  Host-visible results (points, evaluations) are complete when the call
 * returns; kh_sync() is only needed before the HOST reads a device buffer through its own means. */
int kh_dev_alloc(void **ptr, size_t bytes);
int kh_dev_free(void *ptr);
int kh_dev_copy(void *dst_dev, const void *src_dev, size_t bytes);   /* device-to-device, asynchronous on the library's main stream */
int kh_dev_memset_zero(void *dst_dev, size_t bytes);
int kh_dev_upload(void *dst_dev, const void *src_host, size_t bytes);
int kh_dev_download(void *dst_host, const void *src_dev, size_t bytes);
/* count 32-byte records (field elements) at dst_dev set to `value`; asynchronous on the main stream, the value travels in the kernel's arguments */
int kh_dev_fill_elements(uint64_t *dst_dev, const uint64_t value[4], size_t count);
/* `rows` runs of `width` bytes, `src_pitch` / `dst_pitch` bytes apart: the witness columns of a prover ([Vec<F>; 15], each shorter than
 * the domain: kimchi/src/prover.rs:254-266) go into their padded device columns in one transfer. */
int kh_dev_upload_2d(void *dst_dev, size_t dst_pitch, const void *src_host, size_t src_pitch, size_t width, size_t rows);
/* The same transfer WITHOUT waiting for the work queued on the main stream first: for a destination that nothing queued reads or writes (a freshly allocated
 * column).  Returns when the bytes are on the device; kernels queued earlier keep running underneath it -- kh_prove sends the witness in column groups this way,
 * each group's interpolation and extension running under the next group's transfer. */
int kh_dev_upload_2d_unordered(void *dst_dev, size_t dst_pitch, const void *src_host, size_t src_pitch, size_t width, size_t rows);
int kh_msm_batch_dev(kh_srs_t *srs, int basis, unsigned chunk, size_t offset,
                     const uint64_t *scalars_dev, size_t n, size_t k, int scalars_are_montgomery,
                     uint64_t *out_xy /* host, k x 8 */, uint8_t *out_is_inf /* host, k */);
/* Pipelined form of kh_msm_batch_dev: kh_msm_submit enqueues all device work on one of the
 * library's four MSM pipeline slots and returns at once; kh_msm_wait blocks for that job and
 * finishes it (XYZZ -> affine on the host).  With jobs in flight the sort of one MSM and the
 * latency-bound tail (bucket reduction) of another run underneath the bucket accumulation of a third.
 * At most KH_MSM_SLOTS (4) un-waited tickets: a further submit by the thread that holds them all returns KH_E_INVALID at once; when
 * some of them are OTHER threads' (more provers than slots) it BLOCKS until one of those is waited for (back-pressure, no time-out);
 * only when every busy slot's owner is itself blocked in a submit -- nobody left to call kh_msm_wait -- it returns KH_E_INVALID. */
#define KH_MSM_SLOTS 4
int kh_msm_submit(kh_srs_t *srs, int basis, unsigned chunk, size_t offset,
                  const uint64_t *scalars_dev, size_t n, size_t k, int scalars_are_montgomery,
                  uint64_t *ticket);
int kh_msm_wait(uint64_t ticket, uint64_t *out_xy /* host, k x 8 */, uint8_t *out_is_inf /* host, k */);
/* The same pipeline from HOST scalars -- what SRS::commit_non_hiding(&DensePolynomial) hands over (poly-commitment/src/ipa.rs:638-683): one asynchronous
 * upload on the calling thread's copy stream, and the job's first kernel waits for it, so with two MSMs in flight the PCIe transfer of MSM i + 1 runs
 * underneath the accumulation of MSM i.  Returns when the scalars have been taken (pageable or pinned memory: the caller may reuse the buffer at once);
 * the job itself keeps running; kh_msm_wait collects it. */
int kh_msm_submit_host(kh_srs_t *srs, int basis, unsigned chunk, size_t offset,
                       const uint64_t *scalars /* host, k x n x 4 limbs */, size_t n, size_t k, int scalars_are_montgomery,
                       uint64_t *ticket);
int kh_ntt_dev(int field, uint64_t *data_dev, unsigned log2_n, int inverse, size_t batch);
int kh_lde_dev(int field, const uint64_t *coeffs_dev, unsigned log2_n, unsigned log2_blowup,
               uint64_t *out_dev, size_t batch);
/* One coset of an extension: out[r][i] = f_r(shift * w_n^i), i < n = 2^log2_n, for `batch` coefficient vectors (out may
 * alias coeffs).  The d8 extension of kh_lde_dev is 8 such cosets interleaved, lde[8 i + r] = coset_r[i] with
 * shift = w_{8n}^r: with one coset per GPU every later row-wise step of the quotient (expressions, z(x w) = the next row
 * of the same coset) stays local to a GPU.  Asynchronous on the main stream like kh_ntt_dev. */
int kh_coset_ntt_dev(int field, const uint64_t *coeffs_dev, unsigned log2_n, const uint64_t shift[4], uint64_t *out_dev, size_t batch);
int kh_sync(void);

/* ---- instrumentation -------------------------------------------------------
 * Device time (ms, HIP events on the library's own stream) of the last kh_msm*_dev /
 * kh_ntt*_dev / kh_lde*_dev call on this thread, split per phase.  names/ms arrays of
 * capacity cap; returns the number of phases written. */
int kh_last_timings(const char **names, float *ms, int cap);
/* Process-wide event counters (how often a path ran): "spread_retry" (an opening round's MSM met a hot bucket and was re-run with the hot-bucket
 * kernels), "fused_retry" (the one-launch sort gave up), "rebase_launch" / "rebase_switch" / "rebase_abandon" (openings that started
 * materialising the folded basis of their late rounds, switched over to it, gave it up), "rebased_rounds" (rounds that ran over a materialised
 * basis), "lookup_sorted_dev" (successful kh_lookup_sorted_dev calls; kh_prove makes one per proof with lookups), "ipa_concurrent" (kh_ipa_begin calls
 * that found another opening live on the same handle and went ahead beside it), "ipa_waited" (kh_ipa_begin calls that found every workspace of the handle
 * claimed; counted before the wait starts), "table_staged_words" (the uint32_t words of rows[] / cells tables that the gadget and wire calls and
 * kh_witness_schedule_create sent through the staging ring; kh_witness_schedule_run adds none), "point_codec_launches" (launches of the point
 * decompression kernel: one per kh_points_decompress(_dev), kh_srs_create_compressed, kh_proofs_from_wire, kh_proofs_from_msgpack and kh_verifier_index_from_msgpack call that got past its checks),
 * "point_codec_encode_launches" (launches of the point compression kernel: one per kh_points_compress(_dev), kh_srs_get_g_compressed / kh_srs_write_file and
 * per kh_proof_to_wire / kh_proof_to_msgpack / kh_verifier_index_to_msgpack call that writes).  Unknown names read 0. */
uint64_t kh_counter(const char *name);

/* Test hooks (field ops on the device; op: 0 mul, 1 add, 2 sub, 3 to_mont, 4 from_mont,
 * 5 sqr, 6 neg).  Used by the parity tests to pin the device arithmetic itself. */
int kh_debug_field_op(int field, int op, const uint64_t *a, const uint64_t *b, uint64_t *out, size_t n);
/* Test hook of the two product scans that subtract (csrc/field29.cuh: the accumulation's 29-bit-limb arithmetic), on the caller's limbs as they are:
 * every element is nine uint32_t limbs, nothing is converted.  op 0 (mulsub29): out = a b / 2^261 - c + K p; op 1 (sqrsub29, b unused, may be NULL):
 * out = a a / 2^261 - c + K p; both in normalised limbs.  spread picks K p as the additions spread it over the limbs: 0 = (K, J) = (7, 1), 1 = (5, 1),
 * 2 = (4, 4); the caller keeps c_i <= J (2^29 - 1), c_8 <= (K p)_8 - J and the limb magnitudes of a, b within the scan's column bound. */
int kh_debug_field29_op(int field, int op, int spread, const uint32_t *a, const uint32_t *b, const uint32_t *c, uint32_t *out, size_t n);
/* Test hook of the opening's rebase (csrc/rebase.hip; the folded basis of poly-commitment/src/ipa.rs:985-1003 after several rounds at once):
 * out[i] = sum_{q < Q} coef[q] * g[q N + i] for i < N = n / Q (N a multiple of 64), from the handle's c = 16 window tables; coef Montgomery, out affine.
 * *out_fail != 0: an output was the point at infinity (the rebase is then abandoned; out is incomplete). */
int kh_debug_rebase_points(kh_srs_t *srs, const uint64_t *coef, size_t Q, uint64_t *out_xy, uint32_t *out_fail);
/* Test hook of the GLV split the folded basis's MSMs use (csrc/msm.hip glv_split; constants: tools/gen_glv_params.py): for n CANONICAL scalars of the given
 * scalar field, out[10 i .. 10 i + 9] = |k1| (4 x 32-bit limbs), |k2| (4), sign of k1, sign of k2 with k = k1 + k2 lambda (mod r), lambda = the scalar-field
 * endomorphism eigenvalue of kh_endos (endo_r).  kh_scalar_challenge_to_field's curve ids pick the field: KH_FIELD_FP = Vesta's scalars, KH_FIELD_FQ = Pallas's. */
int kh_debug_glv_split(int scalar_field, const uint64_t *scalars, size_t n, uint32_t *out);
/* Point ops on the device through the XYZZ formulas: op 0 = P + Q (affine in, affine out),
 * op 1 = 2P, op 2 = P + Q via the mixed addition. inf flags in/out. */
int kh_debug_point_op(int curve, int op, const uint64_t *p_xy, const uint8_t *p_inf,
                      const uint64_t *q_xy, const uint8_t *q_inf,
                      uint64_t *out_xy, uint8_t *out_inf, size_t n);
/* Test hooks of the MSM's last two stages over narrow windows (csrc/msm.hip, "6 bucket sums" and "7 reduce"), on the caller's records and through the
 * launches an MSM makes.  A record is 128 bytes, x | y | zz | zzz in Montgomery limbs (the point (x / zz, y / zzz)); sixteen zero limbs are the identity.
 * Results are affine with an infinity byte, as kh_debug_point_op gives them.  Neither call takes an MSM slot; each returns when its result has arrived.
 *
 * kh_debug_bucket_tail: sum_t (t + 1) B_t over each of `groups` arrays of nb buckets.  tail 0 / 1 / 2 = the marginal sums by k_marginals (one wave per
 * marginal) / k_marginals_q / k_marginals_h, then k_marginal_fin (fin 0) or k_marginal_fin_q (fin 1): c_or_nb is the window width c, 7 .. 16, nb = 2^(c-1),
 * a bucket index is three digit fields as the plan cuts them (bits = c - 1, f0 = (bits + 2) / 3, f1 = (bits - f0 + 1) / 2, f2 = the rest; m is unused), and
 * out holds three points per group, plane j = sum_t (digit_j(t) + [j == 0]) B_t; the weighted sum is 2^(f0+f1) out[2] + 2^f0 out[1] + out[0].  tail 2 needs
 * nb >> f0 >= 256, as the plan does.  tail 3 = k_reduce_seg, k_sum_level, k_sum_final: c_or_nb is nb itself, a power of two up to 2^15, m the segment
 * length (a power of two up to 16 that divides nb, or nb), fin is unused, and out holds one point per group.
 *
 * kh_debug_bucket_sums: bucket i = the sum of the records partial[toff[i]] .. partial[toff[i + 1] - 1], i < nkeys (toff: nkeys + 1 ascending offsets from 0).
 * kind 0 / 1 = k_bucket_sum, lists of more than 4 / 16 records through k_bucket_chunk and k_bucket_big; kind 2 = k_bucket_sum_q, more than 16. */
int kh_debug_bucket_tail(int curve, int tail, int fin, unsigned c_or_nb, unsigned m, size_t groups, const uint64_t *buckets, uint64_t *out_xy, uint8_t *out_inf);
int kh_debug_bucket_sums(int curve, int kind, size_t nkeys, const uint32_t *toff, const uint64_t *partial, uint64_t *out_xy, uint8_t *out_inf);
/* Test hook of the MSM's front half (csrc/msm.hip, steps 1 - 4 and "tasks"): the digits, the sort and the task plan of one job, through the function an MSM
 * launches them with (msm_launch_sort), and nothing behind it: no accumulation, no tail.  The caller gives scalars and the facts of a basis; every geometry
 * value a kernel gets comes from the library's plan for that shape and every workspace from its reservation, as for a real job.  No SRS handle and no tables:
 * the sort does index arithmetic on point numbers only.
 *
 * args (host memory): k n scalars of the curve's scalar field, Montgomery (mont != 0) or canonical with at most one excess p.  inf (nullable): infinity bytes
 * indexed as a basis' are, inf[offset + j batch_stride + i] for scalar i of MSM j, inf_len >= offset + (k - 1) batch_stride + n of them.  offset, stride (0 =
 * offset + n; else at least that), batch_stride: first point used, points between window tables, points between the bases of a batch.  precomp_c: 0 = a plain
 * basis, 7 .. 16 = window tables of that width; glv: they hold phi(2^(c w) P) too; wide: a second table set of 20-bit windows that every size takes.
 * fused_off: no one-launch sort.  stage_entries, stage_maxpass: the values of kh_msm_set_sort_staging.  num_cus: 0 = the device's own.
 * Refused with KH_E_INVALID before anything is reserved: an unknown curve, n = 0, k outside 1 .. 8, precomp_c outside {0, 7 .. 16}, glv without precomp_c, wide
 * with glv, num_cus above 1024, an infinity mask that is too short, a stride below offset + n, n W k above 2^26, and whatever the plan itself refuses.
 *
 * echo: what the plan decided.  sort: 0 = k_hist .. k_scatter, 1 = k_sort_fused, 2 = the partitioned sort (wide != 0: its wide form); ranked: 0 = the tasks
 * keep the key order, 1 = all keys are ranked by task length (order / rnt / roff), 2 = the wide path's per-partition ranking, interleaved in `order`.
 * out = NULL: the echo alone, nothing is launched; the caller sizes the outputs from it --
 *   digits [k][W][n] (int32 in two's complement), off and toff nkeys + 1, entries max_entries, order nkeys, rnt and roff nkeys + 1 (ranked 1; order also for
 *   ranked 2), counts 8 words; wide only: ptot 256 k, xpairs 2 max_tasks, slist, big_keys and big_arrivals nkeys each, b29_zero nkeys bytes.
 * counts: [0] handed[0], [1] [2] the hot-bucket list's two counters, [3] the extra chunks of split buckets, [4] the split buckets, [5] off[nkeys] = entries,
 * [6] toff[nkeys] = tasks.  xpairs: (key, chunk) per extra chunk; b29_zero[g nb + t] = 1 when the lazy bucket record of true bucket t of MSM g is all zero
 * (the records are set to 0x01 bytes before the launch).  Keys are the sort's own: permuted per MSM on the wide path, (t & 255) << part_low | t >> 8.
 * Before the launch every array the sort hands on -- digits, off, toff, the task counts, entries, order / rnt / roff, the pairs and keys of the split list -- is
 * set to 0xff bytes, so a word of the result that still reads 0xffffffff was not written by this job.  Takes a free MSM slot for the duration of the call.
 * KH_E_SORT_GAVE_UP: k_sort_fused gave up at a grid barrier (its blocks were not co-resident); nothing is retried on another path. */
#define KH_E_SORT_GAVE_UP (-6)
struct kh_msm_sort_args {
    int curve, mont;
    size_t n, k;
    const uint64_t *scalars;
    const uint8_t *inf; size_t inf_len;
    size_t offset, stride, batch_stride;
    int precomp_c, glv, wide, fused_off;
    unsigned stage_entries, stage_maxpass, num_cus;
};
struct kh_msm_sort_echo {
    uint32_t c, W, nb, precomp, glv, wide, sort, S, ngroups, nkeys, part_low, part_nblk, room, kmin, wide_og, bigcap, hot_nt, stage_now, part2_maxpass, ranked;
    uint32_t max_tasks, max_entries;
    uint8_t ktab[48];
};
struct kh_msm_sort_out {
    uint32_t *digits; uint32_t *off; uint32_t *entries; uint32_t *toff; uint32_t *order; uint32_t *rnt; uint32_t *roff; uint32_t *counts;
    uint32_t *ptot; uint32_t *xpairs; uint32_t *slist; uint32_t *big_keys; uint32_t *big_arrivals;
    uint8_t *b29_zero;
};
typedef struct kh_msm_sort_args kh_msm_sort_args_t;
typedef struct kh_msm_sort_echo kh_msm_sort_echo_t;
typedef struct kh_msm_sort_out kh_msm_sort_out_t;
int kh_debug_msm_sort(const kh_msm_sort_args_t *args, kh_msm_sort_echo_t *echo, const kh_msm_sort_out_t *out);

/* ---- one process per GPU: the path's only collective, over RCCL / xGMI ----
 * A point-range-sharded MSM (BASELINE config 4) exchanges ONE partial point per rank: RCCL has no elliptic-curve reduction, so the "all-reduce" is an
 * all-gather of the partials and a local fold on every rank.  kh_comm_unique_id on one rank, its 128 bytes handed to the others by any means (file,
 * socket, the launcher's store), then kh_comm_init on every rank (collective; binds the communicator to the calling thread's current device).
 * librccl.so is loaded with dlopen at that point -- single-GPU users never need it (KH_E_NOTFOUND if it is absent).
 * kh_comm_allgather_points: out = rank 0's k points, rank 1's k points, ... (host buffers).  kh_msm_allreduce: this rank's shard (its kh_srs_t over its
 * point range, kh_srs_create_device_range) times its slice of the scalars, all-gathered and folded: every rank gets the whole MSM. */
typedef struct kh_comm kh_comm_t;
#define KH_COMM_ID_BYTES 128
int kh_comm_unique_id(uint8_t id[128]);
int kh_comm_init(int world_size, int rank, const uint8_t id[128], kh_comm_t **out);
void kh_comm_free(kh_comm_t *comm);
int kh_comm_world_size(const kh_comm_t *comm);
int kh_comm_rank(const kh_comm_t *comm);
int kh_comm_allgather_points(kh_comm_t *comm, const uint64_t *xy, const uint8_t *inf, size_t k, uint64_t *out_xy, uint8_t *out_inf);
int kh_msm_allreduce(kh_comm_t *comm, kh_srs_t *shard, const uint64_t *scalars, size_t n, int scalars_are_montgomery, uint64_t out_xy[8],
                     uint8_t *out_is_inf);

/* ---- the lookup argument's `sorted` step (kimchi/src/circuits/lookup/constraints.rs:90-194) ----
 * Two entry points with one result.  kh_lookup_sorted is the host one: host vectors in, host vectors out, one thread, a HashMap walk as in the
 * reference; it serves callers whose columns live on the host and is the reference the device path is tested against.  kh_lookup_sorted_dev runs the
 * same hash join and the expansion on the device (csrc/lookup_sorted.hip) over device-resident columns: it is the path kh_prove takes -- the
 * looked-up values and the combined table never leave the card -- and the one for any device-resident caller.
 *
 * table: the first lookup_rows = n - zk_rows - 1 entries of the combined table (4 limbs each, host memory); values: max_per_row columns of looked-up
 * joint values, column s at values + 4 s value_stride, lookup_rows entries each (a row with fewer lookups than max_per_row holds the dummy value 0 in
 * the remaining slots).  out: max_per_row + 1 columns of lookup_rows + 1 values: every table entry repeated (times looked up + 1), in table order,
 * snake layout (consecutive columns share one element, odd columns reversed).  A value that is not in the table: KH_E_INVALID and *bad_row = its row. */
int kh_lookup_sorted(const uint64_t *table, size_t lookup_rows, const uint64_t *values, size_t value_stride, size_t max_per_row, uint64_t *out,
                     size_t *bad_row);
/* The same on the device, queued on the main stream of the calling thread's current context.  table_dev / values_dev as above, in device memory (rows
 * from lookup_rows on are not looked at); column k of the result starts at out_dev + 4 k out_stride and exactly lookup_rows + 1 elements of it are
 * written: every other element of out_dev is left untouched (a prover points it at its padded n-element columns, out_stride = n, and fills the
 * zero-knowledge rows itself).  The same 32-byte values as kh_lookup_sorted, position for position.  A value that is not in the table: KH_E_INVALID,
 * *bad_row = the row the host function would report (lowest slot, then lowest row), the same text in kh_last_error, out_dev untouched.  The call waits
 * once, for one status word; on KH_OK out_dev is ordered on the main stream like the results of the other vector steps (no kh_sync before a consumer on
 * the library's stream).  KH_E_INVALID before anything is launched: a null pointer (bad_row may be null), pointers that are not 16-byte aligned,
 * lookup_rows == 0, max_per_row == 0, value_stride < lookup_rows, out_stride < lookup_rows + 1, (max_per_row + 1) lookup_rows >= 2^31.
 * Scratch (hash slots, counts, offsets) comes from the kh_dev_alloc pool. */
int kh_lookup_sorted_dev(const uint64_t *table_dev, size_t lookup_rows, const uint64_t *values_dev, size_t value_stride, size_t max_per_row,
                         uint64_t *out_dev, size_t out_stride, size_t *bad_row);

/* ---- ProverProof::create as ONE native call (kimchi/src/prover.rs:187-1515, the part this library accelerates end to end) ----
 * The host loop of the prover -- witness columns -> commitments -> z -> quotient -> evaluations -> opening, with the transcript -- written
 * against the entry points above, so that a Rust / C caller pays neither an interpreter nor 60 FFI crossings per proof.  Scope: everything
 * create_recursive takes: generic + the five library gates + the optional gates (RangeCheck0/1, Rot64, Xor16
 * as a plain gate, ForeignFieldAdd/Mul), public inputs, any num_chunks, previous challenges (kh_prove_recursive), lookups into fixed and runtime tables (kh_prover_index_attach_lookup, kh_prover_index_attach_runtime_tables, kh_prove_full).  (proof_systems_amd/prover.py runs the same protocol from Python and
 * covers lookups / runtime tables / recursion; tests/test_gpu_native_prover.py: both give the same proof, field element for field element.)
 *
 * kh_prover_index_new: the caller has built the index columns on the device (ProverIndex of prover_index.rs:30-70; column order below) on the
 * device of `srs`, whose Lagrange basis for 2^log2_n is registered (kh_srs_compute_lagrange).  Three blocks of columns of n = 2^log2_n
 * (d1_dev: evaluations on the domain; dc_dev: coefficient forms) resp. 8n (d8_dev: evaluations on the 8x extended domain) elements:
 *     column 0..14 coefficients | 15 generic selector | 16 sid (omega^j) | 17..23 sigma_0..6 | 24..28 selectors of Poseidon, CompleteAdd,
 *     VarBaseMul, EndoMul, EndoMulScalar | 29.. the n_optional optional-gate selectors (optional_gates: their kh_gate ids, in column order);
 *     dc_dev / d8_dev hold two more columns after those: x and the permutation vanishing polynomial (permutation.rs:107-118).
 *   live_mask: bit k set = the circuit HAS rows of the k-th selector column after the generic one (24 + k): only those gates' constraints are
 *   evaluated unless KH_PROVE_ALL_GATES asks for the reference's behaviour (prover.rs:824-868 evaluates every always-present gate type).
 *   shifts: the 7 permutation shifts (Shifts::new); digest: VerifierIndex::digest (an element of the curve's base field).
 *   The index keeps the pointers (no copy): they must outlive it.
 * kh_prove: witness = 15 columns x rows x 4 Montgomery limbs on the host (rows + zk_rows <= n; the zero-knowledge rows are drawn here), or
 *   witness_dev = the padded 15 x n columns already on the device (then no zero-knowledge rows are drawn: the caller has).
 *   randomness: the field elements the reference draws from its RNG, IN ITS ORDER (kh_prove_randomness_count of them; uniform scalar-field
 *   elements, Montgomery limbs) -- zero-knowledge rows per column from the last row backwards (prover.rs:254-266, host witness only), 15 x
 *   num_chunks witness blinders, z's two random rows, num_chunks blinders of z, 7 num_chunks of t, then the opening's (rand_l, rand_r) per round,
 *   d, r_delta (ipa.rs:940-941, 1036) -- or NULL: drawn from the operating system's generator (getrandom).
 * kh_proof_section: a view into the proof (valid until kh_proof_free).  Point sections give limbs = count x 8 (affine x | y) and flags =
 *   count infinity flags; element sections give limbs = count x 4 and flags = NULL. */
typedef struct kh_prover_index kh_prover_index_t;
typedef struct kh_proof kh_proof_t;
#define KH_PROVE_CHECK 1          /* assert the intermediate invariants (z ends at 1, zero remainders) */
#define KH_PROVE_ALL_GATES 2      /* evaluate the constraints of every always-present gate type, as the reference does */
#define KH_PROVE_EAGER_CHECK 8    /* with KH_PROVE_CHECK: read every invariant back where it is produced and fail THERE, as the reference's ProverError returns do
                                   * (prover.rs:913-917, permutation.rs:566-568, lookup/constraints.rs:325-331) -- one stream stall per check; by default the checks
                                   * ride on the device and are read once after the opening (same errors, reported at the end of the call) */
#define KH_PROVE_SHARED_CONTEXT 4 /* stay on the device's shared library context (default: a private one for the call, kh_private_context_begin) */
#define KH_PROOF_W_COMM 0         /* 15 x num_chunks points */
#define KH_PROOF_Z_COMM 1         /* num_chunks points */
#define KH_PROOF_T_COMM 2         /* 7 num_chunks points */
#define KH_PROOF_PUBLIC_COMM 3    /* num_chunks points (verifier side; not part of the serialised proof) */
#define KH_PROOF_EVALS 4          /* per polynomial num_chunks values at zeta, then num_chunks at zeta omega; polynomials: z, generic selector, the five
                                     selectors, w x 15, coefficients x 15, sigma x 6, the optional selectors in column order */
#define KH_PROOF_PUBLIC_EVALS 5   /* num_chunks at zeta, num_chunks at zeta omega */
#define KH_PROOF_FT_EVAL1 6
#define KH_PROOF_LR 7             /* (L, R) per round: 2 log2(srs size) points */
#define KH_PROOF_DELTA 8
#define KH_PROOF_Z1_Z2 9
#define KH_PROOF_SG 10
#define KH_PROOF_CHALLENGES 11    /* beta, gamma, alpha, zeta, v (polyscale), u (evalscale); with lookups a seventh: the joint combiner */
#define KH_PROOF_LOOKUP_SORTED_COMM 12   /* (max lookups per row + 1) x num_chunks points; empty without lookups */
#define KH_PROOF_LOOKUP_AGGREG_COMM 13   /* num_chunks points */
#define KH_PROOF_LOOKUP_RUNTIME_COMM 14  /* num_chunks points; empty without runtime tables */
int kh_prover_index_new(kh_srs_t *srs, unsigned log2_n, unsigned zk_rows, unsigned public_inputs, const uint64_t *d1_dev, const uint64_t *dc_dev,
                        const uint64_t *d8_dev, const int *optional_gates, size_t n_optional, unsigned live_mask, const uint64_t *shifts,
                        const uint64_t digest[4], kh_prover_index_t **out);
/* Adds the lookup constraint system of the index (LookupConstraintSystem, lookup/index.rs:189-311; fixed tables, no runtime tables): patterns = the
 * ids of the lookup patterns the circuit uses -- 0 Xor, 1 Lookup, 2 RangeCheck, 3 ForeignFieldMul --, increasing; per pattern its selector column as
 * d1 evaluations, coefficient form and d8 evaluations; the concatenated table columns and (nullable) the table-id column as d1 evaluations; and the d8
 * evaluations of the three row-set atoms the constraints use (expr.rs:883-893): VanishesOnZeroKnowledgeAndPreviousRows, UnnormalizedLagrangeBasis(0),
 * UnnormalizedLagrangeBasis(-zk_rows - 1).  The digest given to kh_prover_index_new must cover the lookup index.  kh_prove then runs the lookup argument
 * (joint combiner, combined table, sorted columns on the device via kh_lookup_sorted_dev, aggregation, the lookup constraints on d8, the extra evaluations and openings);
 * KH_PROOF_EVALS carries, after the polynomials listed above: sorted x (max_per_row + 1), aggregation, combined table, one selector per pattern;
 * the randomness grows by (max_per_row + 1) (zk_rows + num_chunks) after the witness blinders and zk_rows + num_chunks before z's two rows. */
int kh_prover_index_attach_lookup(kh_prover_index_t *index, const int *patterns, size_t n_patterns, const uint64_t *const *selectors_d1_dev,
                                  const uint64_t *const *selectors_c_dev, const uint64_t *const *selectors_d8_dev,
                                  const uint64_t *const *table_cols_d1_dev, size_t n_table_cols, const uint64_t *table_ids_d1_dev,
                                  const uint64_t *const *atoms_d8_dev);
/* Runtime tables (lookup/runtime_tables.rs, index.rs:241-311): `length` rows of the combined table, starting at row `offset`, whose second column arrives
 * with each proof (kh_prove_full: runtime_values, all runtime tables' data concatenated in the index's order); selector = the runtime-table selector column
 * (1 outside the runtime rows, 0 on them and on the zero-knowledge rows) as d1 evaluations, coefficient form, d8 evaluations.  After
 * kh_prover_index_attach_lookup.  KH_PROOF_EVALS then carries runtime table + runtime selector between the combined table and the pattern selectors; the
 * randomness grows by zk_rows + num_chunks right after the witness blinders. */
int kh_prover_index_attach_runtime_tables(kh_prover_index_t *index, const uint64_t *selector_d1_dev, const uint64_t *selector_c_dev,
                                          const uint64_t *selector_d8_dev, size_t offset, size_t length);
/* ---- the index from a gate list: ConstraintSystem::create(gates).public(k).build() + ProverIndex::verifier_index() (constraints.rs, prover_index.rs,
 * verifier_index.rs:175-300, 405-540) as one call, for circuits WITHOUT a lookup argument ----
 * kh_permutation_shifts: Shifts::new (permutation.rs:140-199) for the domain of 2^log2_n rows: shift_0 = 1, then six quadratic non-residues r with
 *   r^n != 1, no repeats, each the first 248 bits (little-endian, 31 bytes) of Blake2b-512(big-endian u32 counter), counter 8, 9, ...
 *   out: 7 x 4 Montgomery limbs.  Host code; needs no device.
 * kh_prover_index_create: n_gates records, one per row, as CircuitGate (gate.rs): gate_types[i] = a kh_gate_name id or KH_GATE_ZERO (a row without gate
 *   constraints); wires[14 i .. 14 i + 13] = the 7 (row, col) pairs the row's cells are wired to (identity: (i, c)); coeffs[60 i .. 60 i + 59] = 15
 *   Montgomery elements, zero-padded.  The domain is the smallest 2^k with n_gates + zk_rows <= 2^k, where zk_rows and the number of chunks follow
 *   each other with the SRS size as max_poly_size (constraints.rs:769-771, 946-999); rows n_gates .. n - 1 are Zero rows wired to themselves.  The
 *   Lagrange basis of the domain is computed on `srs` if it is not registered yet.  The call builds on the device of `srs`: the d1 columns in the
 *   layout of kh_prover_index_new (coefficients, generic selector, sid, sigma with sigma_c[r] = shift[col] omega^row for the cell (row, col) that
 *   cell (r, c) is wired to -- zero on rows n + 2 - zk_rows .. n - 2 --, the five library selectors, then ForeignFieldAdd's when the circuit has
 *   such rows), their coefficient forms and d8 evaluations, x and the permutation vanishing polynomial; then the verifier index: every column
 *   committed over the Lagrange basis, the generic and the five library selector commitments masked with blinder 1 (an absent gate type gives h
 *   per chunk), the optional selectors non-hiding, and the digest (the base-field sponge over sigma, coefficients, generic, the five selectors, the
 *   optional ones).  The result is a kh_prover_index_t for kh_prove / kh_prove_recursive / kh_prove_full that OWNS its device columns
 *   (kh_prover_index_free releases them); the caller's arrays are not kept.  public_inputs: the number of public inputs (the first rows of
 *   witness column 0).
 *   Refused with KH_E_INVALID before any device work: a gate type with a lookup pattern (Xor16, RangeCheck0, RangeCheck1, Rot64, ForeignFieldMul --
 *   their digest covers the lookup index: kh_prover_index_create_lookup below, or kh_prover_index_new + kh_prover_index_attach_lookup, is their path), Permutation, an unknown id, a wire
 *   with row >= n or col >= 7, a coefficient >= p, n_gates < 2, public_inputs >= n - zk_rows.  kh_prover_index_attach_lookup and
 *   kh_prover_index_attach_runtime_tables refuse a created index.
 * kh_prover_index_shape: the domain (log2_n), zk_rows and num_chunks of any index (NULL outputs are skipped).
 * kh_verifier_index_section: a view into the verifier index of a created index (valid until kh_prover_index_free), laid out as kh_proof_section:
 *   point sections give limbs = count x 8 (affine x | y) and flags = count infinity flags, element sections limbs = count x 4 and flags = NULL.
 *   An index from kh_prover_index_new gives its shifts and digest; its commitment sections are KH_E_NOTFOUND. */
#define KH_GATE_ZERO (-1)                  /* a row without gate constraints (GateType::Zero) */
#define KH_VINDEX_SIGMA_COMM 0             /* 7 x num_chunks points */
#define KH_VINDEX_COEFFICIENTS_COMM 1      /* 15 x num_chunks points */
#define KH_VINDEX_GENERIC_COMM 2           /* num_chunks points */
#define KH_VINDEX_SELECTOR_COMM 3          /* Poseidon (psm), CompleteAdd, VarBaseMul (mul), EndoMul (emul), EndoMulScalar: 5 x num_chunks points */
#define KH_VINDEX_OPTIONAL_COMM 4          /* num_chunks points per optional gate present, in column order (here: ForeignFieldAdd or nothing) */
#define KH_VINDEX_SHIFTS 5                 /* 7 elements */
#define KH_VINDEX_DIGEST 6                 /* 1 base-field element: VerifierIndex::digest */
int kh_permutation_shifts(int field, unsigned log2_n, uint64_t *out);
int kh_prover_index_create(kh_srs_t *srs, size_t n_gates, const int *gate_types, const uint32_t *wires, const uint64_t *coeffs,
                           unsigned public_inputs, kh_prover_index_t **out);
/* ---- the same call for circuits WITH a lookup argument: + LookupConstraintSystem::create (lookup/index.rs:188-430, lookups.rs:176-264, 500-513) and the
 * lookup side of the verifier index (verifier_index.rs:189-216, 482-530) ----
 * kh_prover_index_create_lookup takes the gate records of kh_prover_index_create, where a gate type may now also be RangeCheck0, RangeCheck1, Rot64,
 *   ForeignFieldMul, Xor16 or KH_GATE_LOOKUP (GateType::Lookup); the caller's fixed lookup tables (LookupTable: id, `width` columns of `len` entries,
 *   column-major, Montgomery limbs); and the runtime-table configurations (RuntimeTableCfg: id and first column; the second column arrives with each
 *   proof, kh_prove_full's runtime_values, all tables concatenated in this order).  n_runtime > 0 is `runtime_tables: Some(..)` of the reference.
 *   (The reference's `Some(vec![])` -- runtime tables enabled, none configured: a runtime selector and uses_runtime_tables without any runtime row --
 *   cannot be expressed here: n_runtime = 0 is `None`.)
 *   Domain: the smallest 2^k with max(n_gates, lookup_domain_size + 1) + zk_rows <= 2^k, lookup_domain_size = the fixed tables' entries + the runtime
 *   tables' + 4096 if a gate has the RangeCheck or ForeignFieldMul pattern + 256 if one has the Xor pattern + 1 if no fixed table has id 0
 *   (constraints.rs:883-945); zk_rows and the chunks as for kh_prover_index_create.
 *   Patterns (LookupPattern::from_gate): Xor16 -> Xor on its row; KH_GATE_LOOKUP -> Lookup on its row; RangeCheck0, Rot64 -> RangeCheck on their
 *   row; RangeCheck1 -> RangeCheck on its row and the next; ForeignFieldMul -> ForeignFieldMul on its row and the next.
 *   Optional gate selector columns 29..: RangeCheck0, RangeCheck1, ForeignFieldAdd, ForeignFieldMul, Xor16, Rot64, those the circuit has, in that order.
 *   The combined table: the caller's tables in their order, then the gate tables the patterns need (the 12-bit range-check table, id 1, before the
 *   4-bit XOR table, id 0), then the runtime tables (first column fixed, second zero); max(table widths, largest joint lookup) columns, zero rows up
 *   to n; a table-id column when some id is not 0; with runtime tables the runtime selector (1 outside the runtime rows, 0 on them and on the
 *   zero-knowledge rows).  All of these, the pattern selectors and the three row-set atoms of the lookup constraints are produced on the device from
 *   the gate types and the raw table data (csrc/lookup_index.hip); table columns and ids are committed and masked with blinder 1, the pattern
 *   selectors and the runtime selector committed non-hiding, and the digest absorbs, after the optional gates (in verifier_index.rs's order:
 *   range_check0, range_check1, foreign_field_mul, foreign_field_add, xor, rot): tables, ids, runtime selector, pattern selectors.
 *   The result is a created index like kh_prover_index_create's (it owns its columns; kh_prover_index_attach_* refuse it); kh_prove* run the lookup
 *   argument on it as after kh_prover_index_attach_lookup / _attach_runtime_tables.  Without any lookup pattern the call gives what
 *   kh_prover_index_create gives (tables, if any, still count for the domain, as in the reference).
 *   Refused with KH_E_INVALID before any device work, besides kh_prover_index_create's refusals: two tables (fixed, gate or runtime) with the same id,
 *   a runtime id configured twice, a table with id 0 without an all-zero entry, entries >= n - zk_rows - 1, a table value >= p, a table without
 *   columns (or more than 128), runtime tables for a circuit without a lookup pattern.
 * KH_VINDEX_LOOKUP_*: the lookup sections of kh_verifier_index_section; empty (count 0) for an index without a lookup argument. */
#define KH_GATE_LOOKUP (-2)                /* GateType::Lookup: a row without gate constraints that carries the Lookup pattern */
#define KH_VINDEX_LOOKUP_TABLE_COMM 7      /* one commitment per table column: width x num_chunks points */
#define KH_VINDEX_LOOKUP_TABLE_IDS_COMM 8  /* num_chunks points, or none when every table id is 0 */
#define KH_VINDEX_LOOKUP_SELECTOR_COMM 9   /* num_chunks points per pattern present, in the order xor, lookup, range_check, foreign_field_mul */
#define KH_VINDEX_LOOKUP_RUNTIME_SELECTOR_COMM 10   /* num_chunks points, or none without runtime tables */
#define KH_VINDEX_LOOKUP_INFO 11           /* NOT field elements: 2 records of 4 plain 64-bit words, flags = NULL: max_per_row, max_joint_size, joint_lookup_used,
                                              uses_runtime_tables | patterns present (bit k = pattern id k), table columns, first runtime row, runtime rows */
typedef struct { int id; size_t width, len; const uint64_t *data; } kh_lookup_table_t;
typedef struct { int id; size_t len; const uint64_t *first_column; } kh_runtime_table_cfg_t;
int kh_prover_index_create_lookup(kh_srs_t *srs, size_t n_gates, const int *gate_types, const uint32_t *wires, const uint64_t *coeffs,
                                  unsigned public_inputs, const kh_lookup_table_t *tables, size_t n_tables,
                                  const kh_runtime_table_cfg_t *runtime, size_t n_runtime, kh_prover_index_t **out);
/* Debug view of the lookup columns an index carries (built by kh_prover_index_create_lookup or attached): the device address and the element count
 * (n, or 8n for d8 columns) of column k of a block; KH_E_NOTFOUND where the index has none.  The memory belongs to the index (or its caller). */
#define KH_LOOKUP_COL_SELECTOR_D1 0        /* k-th pattern selector: evaluations on the domain */
#define KH_LOOKUP_COL_SELECTOR_C 1         /* ... its coefficient form */
#define KH_LOOKUP_COL_SELECTOR_D8 2        /* ... its evaluations on d8 */
#define KH_LOOKUP_COL_TABLE_D1 3           /* k-th column of the combined table */
#define KH_LOOKUP_COL_TABLE_IDS_D1 4       /* the table-id column (k = 0) */
#define KH_LOOKUP_COL_ATOM_D8 5            /* k = 0 VanishesOnZeroKnowledgeAndPreviousRows, 1 UnnormalizedLagrangeBasis(0), 2 UnnormalizedLagrangeBasis(-zk_rows - 1) */
#define KH_LOOKUP_COL_RUNTIME_SELECTOR 6   /* the runtime-table selector: k = 0 evaluations, 1 coefficient form, 2 d8 */
int kh_debug_lookup_column(const kh_prover_index_t *index, int block, size_t k, const uint64_t **dev, size_t *elems);
/* Where a lookup table sits in an index from kh_prover_index_create_lookup: the rows [first_row, first_row + len) of the combined table that hold
 * table `table_id` -- one of the caller's fixed tables, a gate table (range check: id 1, XOR: id 0) or a runtime table, each under the id it was
 * created with.  keys_dev = column 0 of the combined table at first_row, values_dev = column 1 at first_row (NULL when the combined table has one
 * column): the two columns kh_lookup_witness_dev / KH_STEP_LOOKUP read.  For a runtime table column 1 is the index's fixed zero column: is_runtime
 * is 1 (else 0), runtime_first is the table's first element inside the concatenated runtime values (else 0), and the caller passes
 * its_runtime_values_dev + 4 * runtime_first as the value column.  NULL outputs are skipped; the memory belongs to the index.
 * KH_E_NOTFOUND: an id the index does not have, an index without a lookup index, an index from kh_prover_index_new / _attach_lookup (whose tables
 * are the caller's own). */
int kh_prover_index_lookup_table(const kh_prover_index_t *index, int table_id, size_t *first_row, size_t *len, int *is_runtime,
                                 size_t *runtime_first, const uint64_t **keys_dev, const uint64_t **values_dev);
int kh_prover_index_shape(const kh_prover_index_t *index, unsigned *log2_n, unsigned *zk_rows, size_t *num_chunks);
int kh_verifier_index_section(const kh_prover_index_t *index, int section, const uint64_t **limbs, const uint8_t **flags, size_t *count);
/* wall-clock seconds of kh_prover_index_create(_lookup)'s phases (the lookup columns count under the first, their transforms and atoms under the second), each ended by a device synchronisation: validation + upload + column kernel, transforms
 * (coefficient forms, d8), commitments, masking + digest; zeros for an index from kh_prover_index_new.  Returns the number of phases (4). */
int kh_prover_index_phase_seconds(const kh_prover_index_t *index, double *seconds, size_t cap);
void kh_prover_index_free(kh_prover_index_t *index);
size_t kh_prove_randomness_count(const kh_prover_index_t *index, int witness_on_host);
int kh_prove(kh_prover_index_t *index, const uint64_t *witness, size_t rows, const uint64_t *witness_dev, const uint64_t *randomness,
             size_t n_random, unsigned flags, kh_proof_t **out);
/* create_recursive with previous challenges (RecursionChallenge, proof.rs:117-131; prover.rs:276-279, 1212-1262): n_prev accumulators, the j-th with
 * prev_rounds[j] challenges (prev_chals: all of them concatenated, Montgomery limbs) and a commitment of prev_comm_chunks[j] chunks (prev_comm_xy /
 * prev_comm_inf: all chunks concatenated).  2^rounds must be the SRS size (one chunk) or twice it (two chunks). */
int kh_prove_recursive(kh_prover_index_t *index, const uint64_t *witness, size_t rows, const uint64_t *witness_dev, const uint64_t *randomness,
                       size_t n_random, unsigned flags, const uint64_t *prev_chals, const unsigned *prev_rounds, const uint64_t *prev_comm_xy,
                       const uint8_t *prev_comm_inf, const size_t *prev_comm_chunks, size_t n_prev, kh_proof_t **out);
/* everything create_recursive takes: previous challenges and (n_runtime = the index's runtime rows, else 0) the runtime tables' second column */
int kh_prove_full(kh_prover_index_t *index, const uint64_t *witness, size_t rows, const uint64_t *witness_dev, const uint64_t *randomness, size_t n_random,
                  unsigned flags, const uint64_t *prev_chals, const unsigned *prev_rounds, const uint64_t *prev_comm_xy, const uint8_t *prev_comm_inf,
                  const size_t *prev_comm_chunks, size_t n_prev, const uint64_t *runtime_values, size_t n_runtime, kh_proof_t **out);
/* kh_prove_full with the runtime tables' second column in DEVICE memory (16-byte aligned; n_runtime elements): same meaning and same refusals, but the
 * values are read in stream order -- a producer on this thread's context needs no kh_sync -- and, like witness_dev, are not checked against p.  The
 * runtime column is assembled on the device (zeros, a device copy at the runtime rows, the drawn zero-knowledge rows) and the randomness is drawn in
 * kh_prove_full's order: with the same index, witness, randomness and values every proof section is byte-identical. */
int kh_prove_full_runtime_dev(kh_prover_index_t *index, const uint64_t *witness, size_t rows, const uint64_t *witness_dev, const uint64_t *randomness,
                              size_t n_random, unsigned flags, const uint64_t *prev_chals, const unsigned *prev_rounds, const uint64_t *prev_comm_xy,
                              const uint8_t *prev_comm_inf, const size_t *prev_comm_chunks, size_t n_prev, const uint64_t *runtime_values_dev,
                              size_t n_runtime, kh_proof_t **out);
/* ---- the witness against the circuit, row by row: ProverIndex::verify / ConstraintSystem::verify (kimchi/src/circuits/constraints.rs) ----
 * kh_prove with KH_PROVE_CHECK runs the whole proof before it says that the witness does not satisfy the constraints, and names no row.
 * kh_witness_check says which row and why, in tens of microseconds of kernels (csrc/witness_check.hip) over what is resident already: the index's d1
 * columns (coefficients, selectors), the wires of the gate list, the witness.  It is a deterministic check: every constraint of every row is evaluated
 * on its own and compared with zero exactly -- no alpha, no random combination.
 *   The witness is given as to kh_prove: witness = 15 columns x rows x 4 Montgomery limbs on the host (rows + zk_rows <= n; padded with zeros to n
 *   on the device -- no zero-knowledge rows and no randomness are drawn, the call is deterministic), or witness_dev = the padded 15 x n columns on the
 *   device, checked as given (`rows` is not read).
 *   flags: KH_WITNESS_GATES -- the constraints of every row's gate: the double generic gate (2 constraints; on rows r < public_inputs the public
 *   input, by definition the witness's own cell w[0][r], is subtracted from the first), the five library gates, the optional gates.  `next` of row
 *   n - 1 is row 0.  Works on every index (one from kh_prover_index_new has the selector columns too; its library gates are those of live_mask).
 *   KH_WITNESS_WIRES -- the copy constraints: every cell (r, c < 7) of the gate list holds the value of the cell it is wired to.  Needs the gate
 *   list: an index from kh_prover_index_create(_lookup), which keeps its wires on the device; any other index: KH_E_INVALID with a message.
 *   Returns KH_OK for a satisfied AND for a violated witness; out->kind says which.  Errors are for bad arguments only -- a null pointer, both or
 *   neither witness pointer, rows + zk_rows > n, flags == 0 or an unknown flag, KH_WITNESS_WIRES without wires -- and leave *out untouched.
 *   The report names the FIRST violation in the reference's order: every violation has the key row * 64 + sub, sub = 0..6 for a disconnected cell of
 *   that column, 7 for the row's gate, and the lowest key is reported -- the lowest row, within a row the wires by column before the gate.
 *     KH_WITNESS_DISCONNECTED (GateError::DisconnectedWires): (row, col) and the cell (wired_row, wired_col) it is wired to hold different values.
 *     KH_WITNESS_GATE (GateError::Custom { row, .. }): gate = the kh_gate_name id of the row's gate, constraints = bit i set iff constraint i of that
 *     row is not zero; constraint i is the one that carries alpha^i in the gate's combined expression (Argument::constraint_checks's order).
 *     gate_rows_violated, cells_disconnected: how many rows have a violated gate / how many (row, column) cells are disconnected, over the whole circuit.
 *   Not checked: the reference's index-side condition IncorrectPublic (a public row that is not a Generic gate with coefficients 1, 0, 0, ...), a
 *   property of the gate list, not of the witness.  Lookups are checked by kh_witness_check_full with KH_WITNESS_LOOKUPS (kh_witness_check refuses
 *   that flag):
 * kh_witness_check_full: kh_witness_check + the lookups.  With KH_WITNESS_GATES / KH_WITNESS_WIRES alone it is kh_witness_check (the runtime arguments
 *   are not read; lookup_out, if given, gets an empty record).  KH_WITNESS_LOOKUPS -- exact, without a joint combiner:
 *     The table is a set of tuples.  With L = n - zk_rows - 1, every row t < L of the index's combined table gives (id_t, c_0[t], .., c_{W-1}[t]): its W
 *     columns on the domain and the table-id column, id_t = 0 when the index has no id column.  On the runtime rows column 1 is the call's
 *     runtime_values (all runtime tables' second columns concatenated in the index's order, as for kh_prove_full; the fixed second column is zero there).
 *     Only rows r < L are checked.  For every lookup-pattern selector that is 1 on row r (the `next` rows of RangeCheck1 / ForeignFieldMul are in
 *     the selector columns), each joint lookup s of the pattern (LookupPattern::lookups, lookups.rs:417-487) gives the tuple (id, w[cells[0]][r], ..,
 *     w[cells[ncell - 1]][r], 0, .., 0) padded with zeros to W entries, id = the pattern's constant table id or w[0][r] (Lookup), and that tuple must
 *     equal a table tuple in all W + 1 components (compared as 32-byte strings: canonical Montgomery limbs are unique).
 *     This is the statement the lookup constraints enforce, and it is strictly tighter than the sorted step of kh_prove in one case: when the index
 *     has no table-id column the prover multiplies the looked-up id by 0, so a Lookup row whose w[0] names a table that does not exist passes there;
 *     here it is reported.  Rows with fewer lookups than max_per_row and the dummy entry are properties of the index and are not checked.
 *     A miss has the key row * 64 + 8 + s, after the wires (0..6) and the gate (7) of its row: the report is the lowest key over everything that was
 *     asked for, kind KH_WITNESS_LOOKUP with out->row set (kh_prove names the first miss in slot-major order instead, under its random combiner).
 *     lookup_out is always filled: lookups_missing = the (row, pattern, joint lookup) triples over the whole circuit whose tuple is in no table; for kind
 *     KH_WITNESS_LOOKUP also the pattern, the joint lookup, its witness columns and what the row looked up (read back from the witness at that row);
 *     otherwise pattern = slot = -1 and the rest is zero.
 *     Works on created and on attached indexes.  KH_E_INVALID with a message, *out and *lookup_out untouched: kh_witness_check's refusals, and with
 *     KH_WITNESS_LOOKUPS an index without a lookup index, lookup_out NULL, n_runtime different from the index's runtime rows (or runtime_values NULL
 *     with runtime rows), runtime values given for an index without runtime tables, a runtime value >= p.
 * kh_witness_lookup_message: report + lookup record as one line, "row 37: lookup 2 of pattern RangeCheck (column 5), table id 1: the value is not in
 *   the table (3 lookups missing)" ("columns 1, 2", "1 lookup missing"); for every other kind the line of kh_witness_report_message.  The record does
 *   not say which field its limbs belong to, so the table id is printed by a heuristic: the limbs are taken out of Montgomery form under Fp, then Fq, and
 *   the first result below 2^32 is the id (a table id is a small number; the other field's reading is a 255-bit value except by a 2^-220 accident);
 *   if neither is, the limbs are printed in hexadecimal.  NUL-terminated and cut at cap; returns the length of the whole line.
 * kh_witness_report_message: the report as one line ("row 37: gate Poseidon, constraints 3, 4 of 15 are not zero (412 rows violated)", "row 12, column
 *   0 is wired to (12, 4) but holds a different value (3 cells disconnected)", "the witness satisfies the circuit"; for KH_WITNESS_LOOKUP the short
 *   "row 37: a looked-up value is in no table (kh_witness_lookup_message names it)"), NUL-terminated and cut at cap;
 *   returns the length of the whole line (as snprintf), or KH_E_INVALID. */
#define KH_WITNESS_GATES 1
#define KH_WITNESS_WIRES 2
#define KH_WITNESS_LOOKUPS 4        /* kh_witness_check_full only */
#define KH_WITNESS_OK 0
#define KH_WITNESS_DISCONNECTED 1   /* GateError::DisconnectedWires */
#define KH_WITNESS_GATE 2           /* GateError::Custom { row, .. } */
#define KH_WITNESS_LOOKUP 3         /* report kind: a looked-up tuple is in no table */
typedef struct {
    int kind;                 /* KH_WITNESS_* */
    int gate;                 /* KH_WITNESS_GATE: kh_gate_name id of the row's gate */
    uint32_t constraints;     /* KH_WITNESS_GATE: bit i = constraint i of that row is non-zero */
    int col, wired_col;       /* KH_WITNESS_DISCONNECTED: the cell and the cell it is wired to */
    size_t row, wired_row;
    size_t gate_rows_violated, cells_disconnected;   /* over the whole circuit */
} kh_witness_report_t;
int kh_witness_check(kh_prover_index_t *index, const uint64_t *witness, size_t rows, const uint64_t *witness_dev, unsigned flags,
                     kh_witness_report_t *out);
int kh_witness_report_message(const kh_witness_report_t *r, char *buf, size_t cap);
typedef struct {
    int pattern, slot, ncells;       /* 0 Xor, 1 Lookup, 2 RangeCheck, 3 ForeignFieldMul; joint lookup 0..3 of the row; 1..3 */
    int cols[3];                     /* the witness columns of the tuple */
    uint64_t table_id[4], entry[3][4];   /* Montgomery limbs of what the row looked up */
    size_t lookups_missing;          /* over the whole circuit */
} kh_witness_lookup_t;
int kh_witness_check_full(kh_prover_index_t *index, const uint64_t *witness, size_t rows, const uint64_t *witness_dev,
                          const uint64_t *runtime_values, size_t n_runtime, unsigned flags, kh_witness_report_t *out,
                          kh_witness_lookup_t *lookup_out);
/* kh_witness_check_full with the runtime values in DEVICE memory (16-byte aligned): same meaning and refusals, read in stream order and not checked
 * against p (a value >= p equals no canonical cell). */
int kh_witness_check_full_runtime_dev(kh_prover_index_t *index, const uint64_t *witness, size_t rows, const uint64_t *witness_dev,
                                      const uint64_t *runtime_values_dev, size_t n_runtime, unsigned flags, kh_witness_report_t *out,
                                      kh_witness_lookup_t *lookup_out);
int kh_witness_lookup_message(const kh_witness_report_t *r, const kh_witness_lookup_t *l, char *buf, size_t cap);
int kh_proof_section(const kh_proof_t *proof, int section, const uint64_t **limbs, const uint8_t **flags, size_t *count);
int kh_proof_phase_seconds(const kh_proof_t *proof, double *seconds, size_t cap);   /* witness_upload, witness_commit, z, quotient, evaluations, opening */
void kh_proof_free(kh_proof_t *proof);

/* ---- kimchi::verifier::verify / batch_verify as ONE native call (kimchi/src/verifier.rs:126-640, 781-1200, 1275-1373; the scalar side of SRS::verify,
 * poly-commitment/src/ipa.rs:301-470) ----
 * The host loop of the verifier (csrc/verifier.cpp), written against the entry points above as kh_prove is: per proof the Fiat-Shamir replay (kh_sponge_*),
 * the public commitment (kh_msm over the registered Lagrange basis, negated, masked with blinder 1; the basis is computed on first use), ft_eval0, the
 * evaluation list in opening order with its combined inner product, and the scalars of SRS::verify; for the whole batch ONE evaluation of the
 * linearisation's constant terms on the device (the compiled gate constraints with one constants table per proof, one launch per gate type present in the
 * batch; the lookup constraints as a token program per proof that has them) and ONE final MSM (kh_ipa_verify_msm).  f_comm, ft_comm and the combined lookup
 * table are linear in commitments the final MSM takes anyway: their scalars are multiplied out on the host and no group operation runs there.
 * Scope: everything kh_prove_full produces and everything the reference's stored proofs contain -- both curves, any num_chunks, public inputs, previous
 * challenges (one or two chunks), the five library gates, the six optional gates, the lookup argument with table ids and runtime tables.
 *
 * kh_verifier_index_of: the verifier index of an index from kh_prover_index_create(_lookup) (KH_E_NOTFOUND for one from kh_prover_index_new, whose
 *   commitments are the caller's): a copy that outlives the prover index, not the SRS handle.  A prover index carries no number of previous challenges
 *   (kh_prove_recursive takes any): neither does this verifier index, which accepts any n_prev.
 * kh_verifier_index_new: from a caller's own data (a deserialised VerifierIndex, verifier_index.rs:59-158): sections[] indexed by KH_VINDEX_*, in exactly
 *   the layout kh_verifier_index_section gives (missing / count 0 = absent; flags NULL = no point at infinity); optional_gates = the kh_gate ids of
 *   KH_VINDEX_OPTIONAL_COMM's entries in column order (RangeCheck0, RangeCheck1, ForeignFieldAdd, ForeignFieldMul, Xor16, Rot64, those present); shifts and
 *   digest are computed when their sections are absent (kh_permutation_shifts; the base-field sponge in verifier_index.rs's order).  A lookup index is
 *   present iff KH_VINDEX_LOOKUP_TABLE_COMM is; it needs KH_VINDEX_LOOKUP_INFO.  Host code: no device work.  KH_E_INVALID with a message: null pointers, a
 *   domain that is no multiple of the SRS size, a section with the wrong number of points, a point off the curve, an element >= p, an unknown or
 *   out-of-order optional gate, inconsistent lookup sections.
 * kh_verifier_index_digest: VerifierIndex::digest as the index holds it (given or computed), an element of the curve's base field.
 * kh_proof_from_sections: a proof from a caller's own data: sections[] indexed by KH_PROOF_* in the layout kh_proof_section gives.  KH_PROOF_PUBLIC_COMM and
 *   KH_PROOF_CHALLENGES are ignored (the verifier derives both); KH_PROOF_PUBLIC_EVALS may be absent for a one-chunk proof (then they are computed from the
 *   public inputs, verifier.rs:336-386).  The sections are copied; their contents are checked by kh_verify, which knows the curve.
 * kh_batch_verify / kh_verify: KH_OK with *ok = 1 / 0 for well-formed proofs that are accepted / of which one at least is rejected.  KH_E_INVALID, with a
 *   kh_last_error text naming the item and the check, BEFORE any device work, for anything malformed: null pointers, k == 0, items over different SRS
 *   handles, rand containing a zero element, a limb vector that is not a canonical field element (>= p), a point that is not on the curve, and the
 *   reference's structural errors (verifier.rs:781-830, check_proof_evals_len): a commitment or evaluation with the wrong number of chunks, n_public or
 *   n_prev different from the index's, an L / R count different from log2(SRS size), lookup sections present without a lookup index or missing with one,
 *   an optional-gate selector evaluation without its commitment.  *ok and trace are untouched on error.
 *   rand: rand_base, sg_rand_base (ipa.rs:330-331; the reference draws them inside) as 2 x 4 Montgomery limbs, NULL = from the operating system.
 *   The call runs on the SRS's device, on a library context of its own like kh_prove (kh_private_context_begin) unless the thread is inside one.
 * kh_verify_last_phase_seconds: wall-clock seconds of the calling thread's last kh_batch_verify, for tools: transcript (validation, Fiat-Shamir, public
 *   commitments), constant term (upload, launches, download), scalars (ft_eval0, combined inner products, the terms of SRS::verify), final MSM.  Returns 4. */
typedef struct kh_verifier_index kh_verifier_index_t;
typedef struct kh_section { const uint64_t *limbs; const uint8_t *flags; size_t count; } kh_section_t;   /* the layout kh_*_section returns */
int kh_verifier_index_of(const kh_prover_index_t *index, kh_verifier_index_t **out);
int kh_verifier_index_new(kh_srs_t *srs, unsigned log2_n, unsigned zk_rows, unsigned public_inputs, unsigned prev_challenges,
                          const int *optional_gates, size_t n_optional, const kh_section_t *sections, size_t n_sections, kh_verifier_index_t **out);
int kh_verifier_index_digest(const kh_verifier_index_t *vix, uint64_t out[4]);
void kh_verifier_index_free(kh_verifier_index_t *vix);
int kh_proof_from_sections(const kh_section_t *sections, size_t n_sections, kh_proof_t **out);
typedef struct kh_verify_item {
    const kh_verifier_index_t *index;               /* the items of one call may use different indexes over ONE SRS handle (batch_verify's rule) */
    const kh_proof_t *proof;
    const uint64_t *public_inputs; size_t n_public; /* Montgomery limbs */
    const uint64_t *prev_chals; const unsigned *prev_rounds; const uint64_t *prev_comm_xy; const uint8_t *prev_comm_inf;
    const size_t *prev_comm_chunks; size_t n_prev;  /* as for kh_prove_recursive */
} kh_verify_item_t;
typedef struct kh_verify_trace {                     /* what the verifier derived for one item: for tests and for a caller hunting a rejection */
    uint64_t challenges[7][4];                       /* as KH_PROOF_CHALLENGES (the seventh is zero without lookups) */
    uint64_t constant_term[4], ft_eval0[4], combined_inner_product[4];
} kh_verify_trace_t;
int kh_batch_verify(const kh_verify_item_t *items, size_t k, const uint64_t *rand, int *ok, kh_verify_trace_t *trace /* k records, nullable */);
int kh_verify(const kh_verify_item_t *item, int *ok, kh_verify_trace_t *trace);
int kh_verify_last_phase_seconds(double *seconds, size_t cap);

/* ---- Compressed points: the 33-byte record the reference stores and sends (csrc/point_codec.hip, csrc/srs_file.hpp) ----
 * A record is x as 32 little-endian bytes of the CANONICAL integer plus one flag byte: 0x80 when y > (p - 1) / 2, 0x40 for the point at infinity (x = 0),
 * 0x00 otherwise (ark-serialize's compressed short-Weierstrass form; p = the curve's base field).  The srs/ files, the stored proofs and every commitment of a
 * serialised ProverProof / VerifierIndex hold it.  Decoding is one square root per point (Tonelli-Shanks, the function of kh_field_sqrt_dev), one lane
 * per record; encoding is two conversions out of Montgomery form.  No LDS, no pool scratch, no per-lane scratch memory.
 *
 * Statuses of a decoded record (one byte each).  The first two are valid records; a record with any other status gives xy = 0 and inf = 0, and every other
 * record of the call is exact.  For valid records the result is the reference's; the classification of malformed ones is this library's own contract:
 *   KH_POINT_OK             a point: x || y in Montgomery limbs, inf = 0
 *   KH_POINT_INFINITY       flag exactly 0x40 and x = 0: xy = 0, inf = 1
 *   KH_POINT_BAD_FLAGS      0x80 and 0x40 both set, one of the low six bits set, or 0x40 with x != 0 (checked first)
 *   KH_POINT_NOT_CANONICAL  x >= p
 *   KH_POINT_NOT_ON_CURVE   x^3 + 5 is not a square
 *
 * kh_points_compress / kh_points_decompress: arrays in host memory; staged through the context, the same kernels, and the call waits.  inf = NULL: no point
 *   at infinity; a set infinity byte gives 32 zero bytes and 0x40 whatever xy holds.  kh_points_decompress returns KH_OK when every record is valid;
 *   otherwise KH_E_INVALID with a kh_last_error text naming the lowest bad index and its status and *first_bad set to it -- out_xy, out_inf and status are
 *   written for all n records all the same.
 * kh_points_compress_dev / kh_points_decompress_dev: vector steps like kh_field_sqrt_dev -- queued on the main stream of the calling thread's current
 *   context, ordered against every other call, not waiting for the device; n == 0 is KH_OK with nothing launched.  flags_dev, bit: the rule of the gadget
 *   calls (nullable word, one atomicOr per wave that has something to raise); the bit is raised by any status other than OK and INFINITY.
 * Every one of the four refuses with KH_E_INVALID, before anything is launched and with nothing written: an unknown curve, a null pointer with n > 0 (other
 *   than the nullable ones), an xy pointer that is not 16-byte aligned, bit >= 32 or a misaligned flag word, n >= 2^32 (the record index is 32 bits in the
 *   SRS file; no byte count overflows below it).
 *
 * kh_srs_create_compressed: kh_srs_create from n records in host memory: the bytes are uploaded and decoded straight into the handle's tables, no affine
 *   copy exists on the host.  A basis point must be a point: a record that is not KH_POINT_OK (an infinity record too) is KH_E_INVALID naming its index, and
 *   no handle is made.  h_bytes (nullable): the blinding base as one record through the same launch, set as kh_srs_set_blinding_base does.
 * kh_srs_get_g_compressed: g[offset .. offset + count) as records (the product writes the bytes the golden SRS digests are defined on).
 * The SRS file: 0x92, 0xdd + the count as a big-endian u32, count x (0xc4 0x21 + record), 0xc4 0x21 + the record of h: kh_srs_file_bytes(n) =
 *   6 + 35 (n + 1) bytes (0 if that overflows).  kh_srs_write_file writes the handle's g and blinding base (KH_E_INVALID when cap is too small);
 *   kh_srs_create_from_file reads one: limit (0 = all) keeps the first `limit` points, h is always the file's last record.  A short buffer, a wrong marker
 *   or a count that disagrees with len is KH_E_INVALID with the byte offset in the message; every length is checked before a read.
 *
 * kh_proofs_from_wire: k proofs from the byte strings of k serialised ProverProofs: sections[p * n_sections + s] is section s (KH_PROOF_*) of proof p.  A
 *   point section is count x 33 records, an element section count x 32 little-endian canonical integers (converted to Montgomery limbs on the host;
 *   KH_E_INVALID when >= p); KH_PROOF_PUBLIC_COMM and KH_PROOF_CHALLENGES are ignored as by kh_proof_from_sections.  The points of ALL k proofs are decoded
 *   in ONE launch and handed to kh_proof_from_sections: the proofs are the ones affine sections would have given.  A bad record is KH_E_INVALID naming
 *   proof, section, index and status; no proof is made and out is left untouched.  The caller's serde still walks the msgpack structure.
 */
#define KH_POINT_BYTES 33
#define KH_POINT_OK 0
#define KH_POINT_INFINITY 1
#define KH_POINT_BAD_FLAGS 2
#define KH_POINT_NOT_CANONICAL 3
#define KH_POINT_NOT_ON_CURVE 4
int kh_points_compress(int curve, const uint64_t *xy, const uint8_t *inf /* nullable */, size_t n, uint8_t *out /* n x 33 */);
int kh_points_decompress(int curve, const uint8_t *bytes, size_t n, uint64_t *out_xy, uint8_t *out_inf,
                         uint8_t *status /* nullable */, size_t *first_bad /* nullable */);
int kh_points_compress_dev(int curve, const uint64_t *xy_dev, const uint8_t *inf_dev /* nullable */, size_t n, uint8_t *out_dev);
int kh_points_decompress_dev(int curve, const uint8_t *bytes_dev, size_t n, uint64_t *out_xy_dev, uint8_t *out_inf_dev,
                             uint8_t *status_dev /* nullable */, uint32_t *flags_dev, unsigned bit);
int kh_srs_create_compressed(int curve, const uint8_t *g_bytes /* n x 33, host */, size_t n, const uint8_t *h_bytes /* 33, nullable */, kh_srs_t **out);
int kh_srs_get_g_compressed(kh_srs_t *srs, size_t offset, size_t count, uint8_t *out /* host, count x 33 */);
size_t kh_srs_file_bytes(size_t n);
int kh_srs_write_file(kh_srs_t *srs, uint8_t *out, size_t cap);
int kh_srs_create_from_file(int curve, const uint8_t *file, size_t len, size_t limit /* 0 = all */, kh_srs_t **out);
typedef struct kh_wire_section kh_wire_section_t;
struct kh_wire_section { const uint8_t *bytes; size_t count; };   /* count records of 33 bytes, or count elements of 32 */
int kh_proofs_from_wire(int curve, const kh_wire_section_t *sections /* k x n_sections */, size_t n_sections, size_t k, kh_proof_t **out /* k */);

/* ---- Serialised proofs and verifier indexes (rmp-serde msgpack) -----------------
 * The bytes the reference sends and stores: `rmp_serde::to_vec` of a ProverProof (kimchi/src/proof.rs:134-195) and of a VerifierIndex
 * (kimchi/src/verifier_index.rs:59-158) -- structs as arrays in declaration order, Option::None as nil, a point as a 33-byte bin (the record above), a
 * field element as a 32-byte little-endian bin, the domain as one 236-byte bin.  The framing (csrc/msgpack_wire.hpp) reads nil, bool, positive fixint,
 * uint8/16/32/64, bin8/16/32, fixarray and array16/32 and refuses every other type byte; it writes the shortest encoding, which is what rmp-serde writes:
 * a file of the reference is reproduced byte for byte.  The RawFixture container of the reference's test files is not read here.
 *
 * Reading.  The structure is walked on the host first (csrc/proof_wire.hpp) and everything malformed is KH_E_INVALID before any device work, with *out (every
 *   out[p]) set to NULL, the byte offset in the message ("offset 17: expected an array, found type byte 0xc4") and no launch counted: a short or overlong
 *   buffer, a foreign type byte, a length beyond the bytes that remain, nesting deeper than 8, a wrong arity (15 w, 6 s, 15 coefficients, 5 lookup_sorted
 *   slots, (L, R) pairs, ...), a bin that is not 32 / 33 bytes, evaluations whose zeta and zeta-omega lengths differ or differ from the proof's first
 *   evaluation, witness commitments of unequal chunk counts, lookup evaluations that do not match the lookup commitments; for an index also size != 2^log_size,
 *   a domain element that is not the library's own (n, 1/n, kh_domain_generator, its inverse, 1, 1, 1), max_poly_size != kh_srs_size(srs), joint_lookup_used
 *   stated twice with different values, a lookup selector commitment present / absent against its feature bit, a runtime selector against uses_runtime_tables.
 *   Then the points of the WHOLE call -- all k proofs with their previous-challenge commitments; all commitments of an index -- are decoded in ONE launch
 *   (kh_counter("point_codec_launches") moves by exactly one per successful call); a bad record is KH_E_INVALID naming section, index and status, an element
 *   >= p is KH_E_INVALID, and no handle is made.  What needs the other file (chunk counts and lookups against the index, rounds against the SRS) stays with
 *   kh_verify.  kh_verifier_index_from_msgpack keeps the file's shifts and computes the digest, as kh_verifier_index_new does without one.
 * The shape of a proof: ProofEvaluations is full of Options, so writing needs to know which are there (optional gates, lookup patterns, runtime tables,
 *   lookups per row).  kh_prove* and kh_proofs_from_msgpack record it in the handle, and kh_prove_recursive / kh_prove_full(_runtime_dev) keep a copy of the
 *   previous challenges there too (kh_proof_prev_challenges: the arrays kh_verify_item_t and kh_prove_recursive take, valid until kh_proof_free; n_prev = 0
 *   when none).  A handle from kh_proof_from_sections or kh_proofs_from_wire has neither: give `shape`, an index of the proof's circuit.  Neither known, or
 *   both and they disagree: KH_E_INVALID.
 * Writing.  *len always receives the size needed; out == NULL is a size query (KH_OK, nothing launched); cap too small is KH_E_INVALID with nothing written.
 *   Every point of the handle goes through ONE launch of the encoder: kh_counter("point_codec_encode_launches") (launches of the compression kernel, from
 *   any caller) moves by one per call that writes.  kh_proof_to_wire: the proof's sections as kh_proofs_from_wire takes them, back to back in `out`,
 *   sections[s] pointing into it (KH_PROOF_PUBLIC_COMM and KH_PROOF_CHALLENGES included when the handle has them).  kh_verifier_index_to_msgpack: an index
 *   from kh_verifier_index_of carries no number of previous challenges, so the argument is written; any other index requires the argument to equal its own. */
int kh_proofs_from_msgpack(int curve, const uint8_t *const *bytes, const size_t *lens, size_t k, kh_proof_t **out /* k */);
int kh_proof_prev_challenges(const kh_proof_t *proof, const uint64_t **chals, const unsigned **rounds, const uint64_t **comm_xy, const uint8_t **comm_inf,
                             const size_t **comm_chunks, size_t *n_prev);
int kh_proof_to_wire(int curve, const kh_proof_t *proof, uint8_t *out, size_t cap, size_t *len, kh_wire_section_t *sections /* KH_PROOF_LOOKUP_RUNTIME_COMM + 1 */);
int kh_proof_to_msgpack(int curve, const kh_proof_t *proof, const kh_verifier_index_t *shape /* nullable */, uint8_t *out, size_t cap, size_t *len);
int kh_verifier_index_from_msgpack(kh_srs_t *srs, const uint8_t *bytes, size_t len, kh_verifier_index_t **out);
int kh_verifier_index_to_msgpack(const kh_verifier_index_t *vix, unsigned prev_challenges, uint8_t *out, size_t cap, size_t *len);

/* ---- Fiat-Shamir sponges (host side) --------------------------------------
 * The transcript of kimchi's prover / verifier: Kimchi Poseidon (width 3, rate 2, 55 full rounds, x^7) under
 * DefaultFqSponge (poseidon/src/sponge.rs:228-412) and DefaultFrSponge (kimchi/src/plonk_sponge.rs:36-57).  Host code, no
 * GPU needed.  kind KH_SPONGE_FQ = the sponge over `curve`'s BASE field that absorbs commitments and squeezes challenges of
 * the scalar field; KH_SPONGE_FR = the sponge over `curve`'s SCALAR field that absorbs evaluations.  Field elements are
 * 4 Montgomery limbs as everywhere; a challenge is the raw 128-bit value (2 limbs), to be mapped with
 * kh_scalar_challenge_to_field where the reference wraps it in a ScalarChallenge. */
#define KH_SPONGE_FQ 0
#define KH_SPONGE_FR 1
int kh_sponge_new(int kind, int curve, kh_sponge_t **out);
int kh_sponge_clone(const kh_sponge_t *s, kh_sponge_t **out);           /* fq_sponge.clone() (prover.rs:1193) */
void kh_sponge_free(kh_sponge_t *s);
int kh_sponge_absorb_g(kh_sponge_t *s, const uint64_t *xy, const uint8_t *inf /*nullable*/, size_t n);   /* FqSponge::absorb_g */
int kh_sponge_absorb(kh_sponge_t *s, const uint64_t *x, size_t n);      /* elements of the sponge's own field: absorb_fq / FrSponge::absorb(_multiple) */
int kh_sponge_absorb_fr(kh_sponge_t *s, const uint64_t *x, size_t n);   /* FqSponge::absorb_fr: scalar-field elements into the base-field sponge */
int kh_sponge_challenge(kh_sponge_t *s, uint64_t chal[2]);              /* 128-bit challenge, raw */
int kh_sponge_challenge_field(kh_sponge_t *s, uint64_t out[4]);         /* the same as a scalar-field element (beta, gamma) */
int kh_sponge_squeeze_field(kh_sponge_t *s, uint64_t out[4]);           /* challenge_fq / digest_fq / FrSponge::digest */
int kh_sponge_digest(kh_sponge_t *s, uint64_t out[4]);                  /* FqSponge::digest: as a scalar-field element, 0 if it does not fit */

#ifdef __cplusplus
}
#endif
#endif /* KIMCHI_HIP_H */
