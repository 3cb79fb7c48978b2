// poseidon.hip -- Kimchi Poseidon on the device (PlonkSpongeConstantsKimchi, poseidon/src/constants.rs:29-41: width 3, rate 2, 55 full rounds of
// x^7, the 3 x 3 MDS, + round constants, no initial round-constant addition; poseidon/src/permutation.rs full_round), for kh_poseidon_permute_dev,
// kh_poseidon_hash_dev and kh_poseidon_gate_witness_dev (csrc/vector_api.cpp, csrc/witness_steps.cpp).
//
//   k_poseidon_permute     n states of 3 elements, in place
//   k_poseidon_hash        ArithmeticSponge (poseidon.rs:60-175): state = init, absorb msg_len elements at rate 2, squeeze once; one message per lane
//   k_poseidon_gate_rows   the witness of the Poseidon gadget (kimchi/src/circuits/polynomials/poseidon.rs:239-290): the state before each of the 55
//                          rounds into the cells of 11 rows, the final state into the first three cells of the twelfth
//   k_poseidon_gate_rows3  the same rows with three lanes per permutation, for batches too small to fill the machine with one lane each (see there)
// Both gate-rows kernels take where their instances land as one WitnessPlace (api_internal.hpp) and address every cell through its members.
// One lane per permutation (except in k_poseidon_gate_rows3), blocks of ONE wave: the work is 1155 Montgomery products per lane that touch no memory (VALU issue), and a batch of a few
// thousand permutations -- one 2^16-row circuit holds 5461 gadgets: 86 waves for 1024 SIMDs -- spreads over the CUs only in blocks that small.
// The one-lane kernels share one round body: s_k <- s_k^7 as x^2, x^4, x^6 = x^4 x^2, x^7 = x^6 x (2 squarings + 2 products), then s_j <- sum_k mds[j][k] s_k +
// rc[r][j]: 21 products per round.  The loop over the rounds stays rolled (21 inlined product blocks are ~40 KB of code; unrolled it would be 55 times
// that); the state and the S-box results are named values, never an indexed array.  MDS and round constants live in constant memory: the round index
// is the same in every lane, so they arrive through scalar loads and are copied into vector registers where a product reads them.
#include "common.hpp"
#include "field.cuh"
#include "api_internal.hpp"

namespace kh {

#include "poseidon_dev_params.inc"

static constexpr int POSEIDON_ROUNDS = 55;
struct PoseidonConsts { u32 mds[3][3][8]; u32 rc[POSEIDON_ROUNDS][3][8]; };
__constant__ PoseidonConsts POSEIDON_DEV_FP = KH_POSEIDON_DEV_FP;
__constant__ PoseidonConsts POSEIDON_DEV_FQ = KH_POSEIDON_DEV_FQ;
template <class F> __device__ __forceinline__ const PoseidonConsts& poseidon_consts();
template <> __device__ __forceinline__ const PoseidonConsts& poseidon_consts<FpParams>() { return POSEIDON_DEV_FP; }
template <> __device__ __forceinline__ const PoseidonConsts& poseidon_consts<FqParams>() { return POSEIDON_DEV_FQ; }

template <class F>
__device__ __forceinline__ Fe<F> const_elem(const u32* w) {
    Fe<F> r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = w[i];
    return r;
}
// (inlined: as one __noinline__ function called three times per round the kernels were 0.5-2.8 % slower and took 95 VGPRs, profiles/poseidon_dev.txt)
template <class F>
__device__ __forceinline__ Fe<F> sbox7(const Fe<F>& x) {
    const Fe<F> x2 = sqr<F>(x), x4 = sqr<F>(x2), x6 = mul<F>(x4, x2);
    return mul<F>(x6, x);
}
template <class F>
__device__ __forceinline__ Fe<F> mds_row(const u32 (*m)[8], const u32* rc, const Fe<F>& t0, const Fe<F>& t1, const Fe<F>& t2) {
    Fe<F> a = mul<F>(const_elem<F>(m[0]), t0);
    a = add<F>(a, mul<F>(const_elem<F>(m[1]), t1));
    a = add<F>(a, mul<F>(const_elem<F>(m[2]), t2));
    return add<F>(a, const_elem<F>(rc));
}
template <class F>
__device__ __forceinline__ void poseidon_round(Fe<F>& s0, Fe<F>& s1, Fe<F>& s2, int r) {
    const PoseidonConsts& K = poseidon_consts<F>();
    const Fe<F> t0 = sbox7<F>(s0), t1 = sbox7<F>(s1), t2 = sbox7<F>(s2);
    s0 = mds_row<F>(K.mds[0], K.rc[r][0], t0, t1, t2);
    s1 = mds_row<F>(K.mds[1], K.rc[r][1], t0, t1, t2);
    s2 = mds_row<F>(K.mds[2], K.rc[r][2], t0, t1, t2);
}
template <class F>
__device__ __forceinline__ void poseidon_permutation(Fe<F>& s0, Fe<F>& s1, Fe<F>& s2) {
#pragma unroll 1
    for (int r = 0; r < POSEIDON_ROUNDS; r++) poseidon_round<F>(s0, s1, s2, r);
}

template <class F>
__global__ void __launch_bounds__(WAVE_BLOCK)
k_poseidon_permute(u64* __restrict__ states, size_t n) {
    const size_t i = (size_t)blockIdx.x * WAVE_BLOCK + threadIdx.x;
    if (i >= n) return;
    u64* const st = states + 12 * i;
    Fe<F> s0 = Fe<F>::load(st), s1 = Fe<F>::load(st + 4), s2 = Fe<F>::load(st + 8);
    poseidon_permutation<F>(s0, s1, s2);
    s0.store(st); s1.store(st + 4); s2.store(st + 8);
}

// Message i is msgs[msg_len i .. msg_len (i + 1)).  The sponge starts in the absorbing state with nothing absorbed: elements go into s0, s1 alternately, a
// permutation runs before the third, fifth, ... element and once more for the squeeze, which returns s0: max(1, ceil(msg_len / 2)) permutations.
struct PoseidonInit { u64 s[12]; };
template <class F>
__global__ void __launch_bounds__(WAVE_BLOCK)
k_poseidon_hash(const u64* __restrict__ msgs, size_t msg_len, size_t n, PoseidonInit init, u64* __restrict__ digests) {
    const size_t i = (size_t)blockIdx.x * WAVE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u64* const m = msgs + 4 * msg_len * i;
    Fe<F> s0 = Fe<F>::load(init.s), s1 = Fe<F>::load(init.s + 4), s2 = Fe<F>::load(init.s + 8);
    size_t j = 0;
    do {
        if (j < msg_len) s0 = add<F>(s0, Fe<F>::load(m + 4 * j));
        if (j + 1 < msg_len) s1 = add<F>(s1, Fe<F>::load(m + 4 * (j + 1)));
        j += 2;
        poseidon_permutation<F>(s0, s1, s2);
    } while (j < msg_len);
    s0.store(digests + 4 * i);
}

// Instance i starts at row at.start_row(i) (WitnessPlace, api_internal.hpp).  Round 5 j + t reads its state from row + j, columns 3 c .. 3 c + 2 with
// c = {0, 2, 3, 4, 1}[t] (the gate's state order, poseidon.rs:65-80).
template <class F>
__global__ void __launch_bounds__(WAVE_BLOCK)
k_poseidon_gate_rows(const u64* states, size_t n, WitnessPlace at, u64* out_states) {          // (out_states may be states: a lane reads its state before it writes anything)
    const size_t i = (size_t)blockIdx.x * WAVE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u64* const st = states + 12 * i;
    Fe<F> s0 = Fe<F>::load(st), s1 = Fe<F>::load(st + 4), s2 = Fe<F>::load(st + 8);
    u64* cell = at.cell(at.start_row(i), 0);           // column 0 of the instance's current row
    int t = 0;
#pragma unroll 1
    for (int r = 0; r < POSEIDON_ROUNDS; r++) {
        const size_t c = t == 0 ? 0 : t == 4 ? 1 : (size_t)t + 1;
        s0.store(cell + at.offset(0, 3 * c)); s1.store(cell + at.offset(0, 3 * c + 1)); s2.store(cell + at.offset(0, 3 * c + 2));
        poseidon_round<F>(s0, s1, s2, r);
        if (++t == 5) { t = 0; cell += at.offset(1, 0); }
    }
    s0.store(cell); s1.store(cell + at.offset(0, 1)); s2.store(cell + at.offset(0, 2));
    if (out_states) { u64* const o = out_states + 12 * i; s0.store(o); s1.store(o + 4); s2.store(o + 8); }
}

// The same rows with one permutation spread over THREE neighbouring lanes, for batches that cannot fill the machine with one lane each (a 2^16-row
// circuit's 5461 gadgets are 86 waves for 1024 SIMDs, and such a wave's time is its own chain of 55 x 21 products).  Lane 3 q + k of a wave holds element
// k of the state of the wave's q-th instance: it raises it to the 7th power, fetches the other two S-box results from its neighbours by wave shuffles and
// computes row k of the MDS product -- 7 products in sequence per round instead of 21, three times the waves.  21 instances per wave; lane 63, and the
// lanes behind the last instance, shadow the wave's first instance (every lane takes part in the shuffles) and store nothing.  MDS row and round constant
// differ from lane to lane here: they are vector loads (the row once, in the rotated order of the lane's operands: a sum mod p does not depend on it).
static constexpr int POSEIDON_SPLIT = 21;          // instances per wave of k_poseidon_gate_rows3
template <class F>
__device__ __forceinline__ Fe<F> shuffle_elem(const Fe<F>& a, int src) {
    Fe<F> r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = (u32)__shfl((int)a.v[i], src, 64);
    return r;
}
template <class F>
__global__ void __launch_bounds__(WAVE_BLOCK)
k_poseidon_gate_rows3(const u64* states, size_t n, WitnessPlace at, u64* out_states) {
    const u32 lane = threadIdx.x, q = lane / 3, k = lane - 3 * q;
    size_t i = (size_t)blockIdx.x * POSEIDON_SPLIT + q;
    const bool live = q < POSEIDON_SPLIT && i < n;
    if (!live) i = (size_t)blockIdx.x * POSEIDON_SPLIT;
    const u32 k1 = k == 2 ? 0 : k + 1, k2 = k1 == 2 ? 0 : k1 + 1;
    const int src1 = q < POSEIDON_SPLIT ? (int)(3 * q + k1) : (int)lane, src2 = q < POSEIDON_SPLIT ? (int)(3 * q + k2) : (int)lane;
    const PoseidonConsts& K = poseidon_consts<F>();
    const Fe<F> m0 = const_elem<F>(K.mds[k][k]), m1 = const_elem<F>(K.mds[k][k1]), m2 = const_elem<F>(K.mds[k][k2]);
    Fe<F> s = Fe<F>::load(states + 12 * i + 4 * k);
    u64* cell = at.cell(at.start_row(i), k);           // column k of the instance's current row
    int t = 0;
#pragma unroll 1
    for (int r = 0; r < POSEIDON_ROUNDS; r++) {
        const size_t c = t == 0 ? 0 : t == 4 ? 1 : (size_t)t + 1;
        if (live) s.store(cell + at.offset(0, 3 * c));
        const Fe<F> u0 = sbox7<F>(s), u1 = shuffle_elem<F>(u0, src1), u2 = shuffle_elem<F>(u0, src2);
        Fe<F> a = mul<F>(m0, u0);
        a = add<F>(a, mul<F>(m1, u1));
        a = add<F>(a, mul<F>(m2, u2));
        s = add<F>(a, const_elem<F>(K.rc[r][k]));
        if (++t == 5) { t = 0; cell += at.offset(1, 0); }
    }
    if (live) {
        s.store(cell);
        if (out_states) s.store(out_states + 12 * i + 4 * k);
    }
}

// (the phase of kh_last_timings carries the kernel's name without the k_: poseidon_permute, poseidon_hash, poseidon_gate_rows, poseidon_gate_rows3)
// kh_poseidon_gate_witness_dev takes the three-lane kernel up to this many instances (kh_poseidon_set_split_max_n): up to two of its waves per SIMD.
// A batch takes about ceil(waves / 1024) wave times, 0.18 ms for a three-lane wave of 21 instances and 0.5 ms for a one-lane wave of 64: measured, three
// lanes win up to 53,760 instances (0.545 against 0.599 ms; 0.380 against 0.532 at 43,008), lose at 2^16 (0.71 against 0.61) and by 2 % at 2^20.
static std::atomic<size_t> g_split_max_n{(size_t)POSEIDON_SPLIT * 2048};

// (the callers in vector_api.cpp and witness_steps.cpp have validated pointers and sizes: n <= WAVE_BLOCK_MAX_N keeps the grid inside 31 bits)
int poseidon_permute(Context& C, int field, uint64_t* states_dev, size_t n) {
    C.timer.begin(C.stream);
    KH_FIELD_LAUNCH(field, k_poseidon_permute<F>, blocks_of(n, WAVE_BLOCK), dim3(WAVE_BLOCK), 0, C.stream, states_dev, n);
    C.timer.mark("poseidon_permute", C.stream);
    return KH_OK;
}
int poseidon_hash(Context& C, int field, const uint64_t* msgs_dev, size_t msg_len, size_t n, const uint64_t* init, uint64_t* digests_dev) {
    PoseidonInit st; memset(&st, 0, sizeof(st));
    if (init) memcpy(st.s, init, sizeof(st.s));
    C.timer.begin(C.stream);
    KH_FIELD_LAUNCH(field, k_poseidon_hash<F>, blocks_of(n, WAVE_BLOCK), dim3(WAVE_BLOCK), 0, C.stream, msgs_dev, msg_len, n, st, digests_dev);
    C.timer.mark("poseidon_hash", C.stream);
    return KH_OK;
}
int poseidon_gate_rows(Context& C, int field, const uint64_t* states_dev, size_t n, const WitnessPlace& at, uint64_t* out_states_dev) {
    const bool split = n <= g_split_max_n.load(std::memory_order_relaxed);
    C.timer.begin(C.stream);
    if (split) KH_FIELD_LAUNCH(field, k_poseidon_gate_rows3<F>, blocks_of(n, POSEIDON_SPLIT), dim3(WAVE_BLOCK), 0, C.stream, states_dev, n, at, out_states_dev);
    else KH_FIELD_LAUNCH(field, k_poseidon_gate_rows<F>, blocks_of(n, WAVE_BLOCK), dim3(WAVE_BLOCK), 0, C.stream, states_dev, n, at, out_states_dev);
    C.timer.mark(split ? "poseidon_gate_rows3" : "poseidon_gate_rows", C.stream);
    return KH_OK;
}
void poseidon_set_split_max_n(size_t n) { g_split_max_n.store(n, std::memory_order_relaxed); }

}  // namespace kh
