"""Value steps (csrc/value_steps.hip): kh_field_inverse_dev, kh_field_sqrt_dev, kh_field_bits_dev as direct calls and as KH_STEP_INVERSE / KH_STEP_SQRT /
KH_STEP_BITS of a witness schedule.  Every comparison is exact equality of limbs against oracle.pasta (pow(x, -1, p), Field.sqrt, Field.is_square) and
Python integers; the circuits at the end go from bound device inputs to an accepted proof through ONE kh_witness_schedule_run."""
import ctypes as C
import os
import random
import re
import sys

import numpy as np
import pytest

from oracle import circuit as CC
from oracle import pasta as P

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_gpu_limb_gadgets_dev import SENTINEL, SIZES, flag_word, mont, plain, sentinel_buf  # noqa: E402
from test_gpu_wiring_dev import FIELD, FORMATS, INT128, INT256, LIMB88, U64, WORDS, records, some_cells, witness_limbs, random_witness  # noqa: E402

pytestmark = pytest.mark.gpu
FIELDS = (P.Fp, P.Fq)
WAVE = 64
PRESET, BIT = 0xa5a5005a, 7                                        # a flag word with other bits set; bit 7 is clear


def launcher_constants():
    """INV_RUN and INV_MAX_BLOCKS of csrc/api_internal.hpp: the sizes below are placed around what they make of n"""
    src = open(os.path.join(os.path.dirname(HERE), "proof_systems_amd", "csrc", "api_internal.hpp")).read()
    return int(re.search(r"INV_RUN = (\d+);", src).group(1)), int(re.search(r"INV_MAX_BLOCKS = (\d+);", src).group(1))


INV_RUN, INV_MAX_BLOCKS = launcher_constants()
# a lane's run is longer than one element from WAVE + 1 on (65 below); one size just above each further threshold:
INV_TWO_BLOCKS = WAVE * INV_RUN + 1                                # more than one block
INV_RUN_GROWS = WAVE * INV_RUN * INV_MAX_BLOCKS + 1                # the grid is full: every lane works through a second run
INV_SIZES = (1, 63, 64, 65, 130, INV_TWO_BLOCKS, 4099, 70001, INV_RUN_GROWS)
POOL = 70001                                                       # distinct elements with an oracle inverse; larger inputs repeat them


@pytest.fixture(scope="module")
def khip():
    import proof_systems_amd.khip as k
    k.init(0)
    return k


def arena(offset):
    return (-1, offset)


def free_all(*bufs):
    for b in bufs:
        b.free()


def unmont(F, limbs):
    rinv = pow(1 << 256, -1, F.p)
    return [int.from_bytes(x.tobytes(), "little") * rinv % F.p for x in np.ascontiguousarray(limbs).reshape(-1, 4)]


def guarded(khip, limbs, guard=4):
    """the elements followed by `guard` sentinel elements, on the device"""
    return khip.DevBuf(32 * (len(limbs) + guard)).upload(np.concatenate([limbs.reshape(-1, 4), np.tile(SENTINEL, (guard, 1))]))


def guard_intact(buf, n, guard=4):
    return np.array_equal(buf.download((n + guard, 4))[n:], np.tile(SENTINEL, (guard, 1)))


def test_constants_are_the_header_s(khip):
    assert (khip.STEP_LOOKUP, khip.STEP_INVERSE, khip.STEP_SQRT, khip.STEP_BITS) == (14, 15, 16, 17)
    assert (INV_RUN, INV_MAX_BLOCKS) == (4, 4096) and INV_SIZES[-1] == 1048577


# ------------------------------------------------------------------------------------------------------------ 1. inverse
@pytest.fixture(scope="module")
def inverse_pool():
    """per field: POOL non-zero elements (1, 2, p - 1, (p + 1) / 2 at indices 1..4) and their oracle inverses, as Montgomery limbs -- computed once"""
    pools = []
    for fid, F in enumerate(FIELDS):
        rnd = random.Random(7100 + fid)
        vals = [rnd.randrange(1, F.p) for _ in range(POOL)]
        vals[1:5] = [1, 2, F.p - 1, (F.p + 1) // 2]
        invs = [pow(x, -1, F.p) for x in vals]
        assert invs[1:5] == [1, (F.p + 1) // 2, F.p - 1, 2]
        x, y = mont(F, vals), mont(F, invs)
        x.setflags(write=False); y.setflags(write=False)
        pools.append((x, y))
    return pools


def inverse_case(pool, n, zeros):
    """(inputs, expected outputs) of n elements; with `zeros`: a zero at index 0, 63, 64 and n - 1 and one whole wave of them"""
    x, y = (np.resize(a, (n, 4)).copy() for a in pool)               # (np.resize repeats the pool's rows)
    if zeros:
        at = [i for i in (0, 63, 64, n - 1) if i < n] + [i for i in range(128, 192) if i < n]
        x[at] = 0; y[at] = 0
    return x, y


@pytest.mark.parametrize("fid", [0, 1])
def test_inverse(khip, fid, inverse_pool):
    for n in INV_SIZES:
        big = n > POOL
        for zeros, in_place in ((True, False), (False, True)) if big else ((True, False), (True, True), (False, True), (False, False)):
            x, want = inverse_case(inverse_pool[fid], n, zeros)
            src = guarded(khip, x)
            dst = src if in_place else sentinel_buf(khip, n + 4)
            flags = khip.DevBuf(4).upload(np.array([PRESET], dtype=np.uint32))
            khip.field_inverse_dev(fid, src, n, dst, flags=flags, bit=BIT)
            got = dst.download((n + 4, 4))
            bad = np.argwhere((got[:n] != want).any(axis=1))
            assert bad.size == 0, (n, zeros, in_place, "elements that differ from the oracle's inverse", bad[:8].ravel().tolist())
            assert np.array_equal(got[n:], np.tile(SENTINEL, (4, 1))), (n, "the guard behind out")
            if not in_place:
                assert np.array_equal(src.download((n, 4)), x), (n, "the input was written")
            assert flag_word(flags) == (PRESET | (1 << BIT) if zeros else PRESET), (n, zeros, in_place)
            free_all(*{src, dst, flags})
    # no flag word: the "inverse or zero" of is_zero
    for n in (65, 130):
        x, want = inverse_case(inverse_pool[fid], n, True)
        src, dst = guarded(khip, x), sentinel_buf(khip, n + 4)
        khip.field_inverse_dev(fid, src, n, dst)
        assert np.array_equal(dst.download((n, 4)), want) and guard_intact(dst, n)
        free_all(src, dst)
    # every element zero
    src, dst, flags = khip.DevBuf(32 * 130).zero(), sentinel_buf(khip, 134), khip.DevBuf(4).zero()
    khip.field_inverse_dev(fid, src, 130, dst, flags=flags, bit=31)
    assert not dst.download((130, 4)).any() and guard_intact(dst, 130) and flag_word(flags) == 1 << 31
    # n == 0: nothing launched, nothing needed
    assert khip.raw().kh_field_inverse_dev(fid, None, 0, None, None, 0) == 0
    free_all(src, dst, flags)


# ------------------------------------------------------------------------------------------------------------ 2. square root
SQRT_SIZES = (1, 63, 64, 65, 130, 1031)


def sqrt_specials(F):
    """(name, element): 0, 1, p - 1, the non-residue 5, and the deepest cases found against the oracle (z = 5^T: z^2 takes 17 rounds in Fp, 19 in Fq)"""
    z = F.two_adic_root
    return [("z^2", z * z % F.p), ("0", 0), ("1", 1), ("p - 1", F.p - 1), ("5", 5), ("z^(2 * 0x7fffffff)", pow(z, 2 * 0x7fffffff, F.p)), ("z^6", pow(z, 6, F.p))]


def sqrt_mix(F, rnd, n):
    """n inputs: the specials, then squares r^2, non-residues 5 r^2 and zeros in turn -- every wave holds every kind"""
    vals = [v for _name, v in sqrt_specials(F)][:n]
    while len(vals) < n:
        r = rnd.randrange(1, F.p)
        vals.append((r * r % F.p, 5 * r * r % F.p, r * r % F.p, 0 if len(vals) % 16 == 3 else pow(r, 4, F.p))[len(vals) % 4])
    return vals


def sqrt_expect(F, vals):
    roots = [F.sqrt(v) for v in vals]
    for v, r in zip(vals, roots):
        assert (r is None) == (not F.is_square(v)) and (r is None or r * r % F.p == v)
    return mont(F, [r or 0 for r in roots]), mont(F, [int(F.is_square(v)) for v in vals]), any(r is None for r in roots)


@pytest.mark.parametrize("fid", [0, 1])
def test_sqrt(khip, fid):
    F = FIELDS[fid]
    rnd = random.Random(7200 + fid)
    z = F.two_adic_root
    assert not F.is_square(5) and F.is_square(F.p - 1) and F.sqrt(1) == 1 and F.sqrt(z * z % F.p) == z
    cases = [(n, sqrt_mix(F, rnd, n)) for n in SQRT_SIZES] + [(1, [v]) for _name, v in sqrt_specials(F)] + [(64, [rnd.randrange(1, F.p) ** 2 % F.p for _ in range(64)])]
    kinds = cases[2][1]
    assert cases[2][0] == 64 and 0 in kinds and any(not F.is_square(v) for v in kinds) and sum(F.is_square(v) for v in kinds) > 16       # the mixed wave
    for k, (n, vals) in enumerate(cases):
        x = mont(F, vals)
        want, want_sq, any_bad = sqrt_expect(F, vals)
        with_sq, in_place = k % 2 == 0, k % 3 == 1
        src = guarded(khip, x)
        dst = src if in_place else sentinel_buf(khip, n + 4)
        sq = sentinel_buf(khip, n + 4) if with_sq else None
        flags = khip.DevBuf(4).upload(np.array([PRESET], dtype=np.uint32))
        khip.field_sqrt_dev(fid, src, n, dst, out_is_square=sq, flags=flags, bit=BIT)
        got = dst.download((n + 4, 4))
        bad = np.argwhere((got[:n] != want).any(axis=1))
        assert bad.size == 0, (n, "roots that are not the oracle's", bad[:8].ravel().tolist())
        assert np.array_equal(got[n:], np.tile(SENTINEL, (4, 1)))
        if with_sq:
            assert np.array_equal(sq.download((n, 4)), want_sq) and guard_intact(sq, n), n
        assert flag_word(flags) == (PRESET | (1 << BIT) if any_bad else PRESET), (n, any_bad)
        free_all(*({src, dst, flags} | ({sq} if with_sq else set())))
    # no flag word
    vals = sqrt_mix(F, rnd, 65)
    src, dst = guarded(khip, mont(F, vals)), sentinel_buf(khip, 69)
    khip.field_sqrt_dev(fid, src, 65, dst)
    assert np.array_equal(dst.download((65, 4)), sqrt_expect(F, vals)[0]) and guard_intact(dst, 65)
    assert khip.raw().kh_field_sqrt_dev(fid, None, 0, None, None, None, 0) == 0
    free_all(src, dst)


# ------------------------------------------------------------------------------------------------------------ 3. bits
NUM_BITS = (1, 8, 64, 88, 128, 254, 255)


def bits_input(F, fmt, vals):
    return mont(F, vals) if fmt == FIELD else plain(vals, WORDS[fmt])


def bits_expect(F, vals, num_bits):
    """(num_bits * n, 4): bit k of value i at k n + i, as Montgomery 0 / 1"""
    zero_one = mont(F, [0, 1])
    idx = np.array([[(v >> k) & 1 for v in vals] for k in range(num_bits)], dtype=np.int64).reshape(-1)
    return zero_one[idx]


def run_bits(khip, fid, fmt, num_bits, vals, flagged):
    F, n = FIELDS[fid], len(vals)
    data = bits_input(F, fmt, vals)
    src = khip.DevBuf(data.nbytes).upload(data)
    dst = sentinel_buf(khip, num_bits * n + 4)
    flags = khip.DevBuf(4).upload(np.array([PRESET], dtype=np.uint32))
    khip.field_bits_dev(fid, src, fmt, num_bits, n, dst, flags=flags, bit=BIT)
    got = dst.download((num_bits * n + 4, 4))
    bad = np.argwhere((got[:num_bits * n] != bits_expect(F, vals, num_bits)).any(axis=1))
    assert bad.size == 0, (fmt, num_bits, n, "elements k n + i that differ", bad[:8].ravel().tolist())
    assert np.array_equal(got[num_bits * n:], np.tile(SENTINEL, (4, 1))), (fmt, num_bits, n, "the guard behind out")
    assert flag_word(flags) == (PRESET | (1 << BIT) if flagged else PRESET), (fmt, num_bits, n, flagged)
    assert np.array_equal(src.download(data.shape), data)
    free_all(src, dst, flags)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("fid", [0, 1])
def test_bits(khip, fid, fmt):
    F = FIELDS[fid]
    rnd = random.Random(7300 + 10 * fid + fmt)
    width = 64 * WORDS[fmt]
    top = F.p if fmt == FIELD else 1 << width                      # values of the format are below this
    allowed = [b for b in NUM_BITS if b <= width]
    assert allowed == {FIELD: list(NUM_BITS), INT256: list(NUM_BITS), INT128: [1, 8, 64, 88, 128], LIMB88: [1, 8, 64, 88, 128], U64: [1, 8, 64]}[fmt]
    for num_bits in allowed:
        for n in SIZES:
            run_bits(khip, fid, fmt, num_bits, [rnd.randrange(min(top, 1 << num_bits)) for _ in range(n)], False)
        # exactly 2^num_bits (where the format holds it) and the all-ones value: the flag, and the low bits regardless
        fits = [rnd.randrange(min(top, 1 << num_bits)) for _ in range(65)]
        if (1 << num_bits) < top:
            for at in (0, 64):
                run_bits(khip, fid, fmt, num_bits, fits[:at] + [1 << num_bits] + fits[at + 1:], True)
        ones = top - 1
        run_bits(khip, fid, fmt, num_bits, fits[:63] + [ones] + fits[64:], ones >> num_bits != 0)
    src, dst = khip.DevBuf(8 * WORDS[fmt] * 65).zero(), sentinel_buf(khip, 65 * 8 + 4)
    khip.field_bits_dev(fid, src, fmt, 8, 65, dst)                 # no flag word
    assert not dst.download((65 * 8, 4)).any() and guard_intact(dst, 65 * 8)
    assert khip.raw().kh_field_bits_dev(fid, None, fmt, 8, 0, None, None, 0) == 0
    free_all(src, dst)


# ------------------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_of_the_direct_calls(khip):
    lib, vp = khip.raw(), C.c_void_p
    n = 3
    a, b, c, flags = sentinel_buf(khip, 8 * n + 1), sentinel_buf(khip, 8 * n + 1), sentinel_buf(khip, n + 1), sentinel_buf(khip, 1)
    A, B, Cq, Fl = a.ptr, b.ptr, c.ptr, flags.ptr

    def refused(name, rc, *needles):
        assert rc == khip.E_INVALID, (name, needles)
        text = lib.kh_last_error().decode()
        for needle in (name,) + needles:
            assert needle in text, (needles, text)

    inv = lambda field=0, i=A, n_=n, o=B, f=Fl, bit=0: lib.kh_field_inverse_dev(field, vp(i), n_, vp(o), vp(f), bit)
    sqrt = lambda field=0, i=A, n_=n, o=B, s=Cq, f=Fl, bit=0: lib.kh_field_sqrt_dev(field, vp(i), n_, vp(o), vp(s), vp(f), bit)
    bits = lambda field=0, i=A, fmt=FIELD, nb=8, n_=n, o=B, f=Fl, bit=0: lib.kh_field_bits_dev(field, vp(i), fmt, nb, n_, vp(o), vp(f), bit)
    for name, call in (("kh_field_inverse_dev", inv), ("kh_field_sqrt_dev", sqrt), ("kh_field_bits_dev", bits)):
        refused(name, call(field=2), "unknown field id 2")
        refused(name, call(i=None), "null in_dev")
        refused(name, call(o=None), "null out_dev")
        refused(name, call(i=A + 8), "in_dev must be 16-byte aligned")
        refused(name, call(o=B + 8), "out_dev must be 16-byte aligned")
        refused(name, call(bit=32), "flag bit 32")
        refused(name, call(f=Fl + 2), "flag bit 0")
        refused(name, call(n_=(1 << 36) + 1), "overflow the grid")
    refused("kh_field_sqrt_dev", sqrt(s=Cq + 8), "out_is_square_dev must be 16-byte aligned")
    assert sqrt(n_=0, i=None, o=None, s=None) == 0
    refused("kh_field_bits_dev", bits(fmt=5), "unknown cell format 5")
    refused("kh_field_bits_dev", bits(fmt=-1), "unknown cell format -1")
    refused("kh_field_bits_dev", bits(nb=0), "num_bits 0")
    refused("kh_field_bits_dev", bits(nb=256), "num_bits 256")
    refused("kh_field_bits_dev", bits(fmt=U64, nb=65), "num_bits 65", "64 bits")
    refused("kh_field_bits_dev", bits(fmt=INT128, nb=129), "num_bits 129", "128 bits")
    refused("kh_field_bits_dev", bits(fmt=LIMB88, nb=129), "num_bits 129")
    refused("kh_field_bits_dev", bits(fmt=U64, i=A + 4), "in_dev must be 8-byte aligned")
    refused("kh_field_bits_dev", bits(fmt=INT128, i=A + 8), "in_dev must be 16-byte aligned")
    assert bits(fmt=U64, i=A + 8, n_=0) == 0
    for buf, elems in ((a, 8 * n + 1), (b, 8 * n + 1), (c, n + 1), (flags, 1)):
        assert np.array_equal(buf.download((elems, 4)), np.tile(SENTINEL, (elems, 1))), "a refused call wrote"
    free_all(a, b, c, flags)


def test_refusals_of_the_steps_at_create(khip):
    K, lib = khip, khip.raw()
    UNTOUCHED = 0x5a5a5a5a

    def refused(steps, needles, field=0, arena_bytes=1024, n_bufs=1):
        arr, _keep = K.WitnessSchedule.pack(steps)
        h = C.c_void_p(UNTOUCHED)
        assert lib.kh_witness_schedule_create(field, 40, arr, len(steps), arena_bytes, n_bufs, C.byref(h)) == K.E_INVALID, needles
        text = lib.kh_last_error().decode()
        for needle in ("kh_witness_schedule_create",) + tuple(needles):
            assert needle in text, (needles, text)
        assert h.value == UNTOUCHED, "*out was written"

    inv = lambda **kw: dict(dict(op=K.STEP_INVERSE, n=4, out=[arena(128)], **{"in": [arena(0)]}), **kw)
    sqrt = lambda **kw: dict(dict(op=K.STEP_SQRT, n=4, out=[arena(128), arena(256)], **{"in": [arena(0)]}), **kw)
    bits = lambda **kw: dict(dict(op=K.STEP_BITS, n=4, format=FIELD, param=4, out=[arena(128)], **{"in": [arena(0)]}), **kw)
    for name, step in (("KH_STEP_INVERSE", inv), ("KH_STEP_SQRT", sqrt), ("KH_STEP_BITS", bits)):
        prefix = f"step 1 ({name})"
        ok = inv()
        refused([ok, step()], ["unknown field id 2"], field=2)
        refused([ok, step(**{"in": [None]})], [prefix, "null in_dev"])
        refused([ok, step(out=[None])], [prefix, "null out_dev"])
        refused([ok, step(**{"in": [arena(8)]})], [prefix, "in_dev must be 16-byte aligned"])
        refused([ok, step(out=[(0, 24)])], [prefix, "out_dev must be 16-byte aligned"])
        refused([ok, step(flag_bit=32)], [prefix, "flag_bit 32"])
        refused([ok, step(**{"in": [(1, 0)]})], [prefix, "in[0]", "buffer 1 of 1"])
        refused([ok, step(**{"in": [arena(1024 - 96)]})], [prefix, "in[0]", "past the arena"])
        refused([ok, step(out=[arena(1024 - 96)])], [prefix, "out[0]", "past the arena"])
    refused([sqrt(out=[arena(128), arena(1000)])], ["step 0 (KH_STEP_SQRT)", "out_is_square_dev must be 16-byte aligned"])
    refused([sqrt(out=[arena(128), arena(1024 - 96)])], ["step 0 (KH_STEP_SQRT)", "out[1]", "past the arena"])
    refused([bits(format=5)], ["step 0 (KH_STEP_BITS)", "unknown cell format 5"])
    refused([bits(param=0)], ["step 0 (KH_STEP_BITS)", "num_bits 0"])
    refused([bits(param=256)], ["step 0 (KH_STEP_BITS)", "num_bits 256"])
    refused([bits(format=U64, param=65)], ["step 0 (KH_STEP_BITS)", "num_bits 65"])
    refused([bits(format=U64, **{"in": [arena(4)]})], ["step 0 (KH_STEP_BITS)", "in_dev must be 8-byte aligned"])
    # the extent of the bits: n x num_bits x 32 bytes -- 4 x 7 elements from offset 128 end at 1024, 4 x 8 do not
    refused([bits(param=8)], ["step 0 (KH_STEP_BITS)", "out[0]", "past the arena"])
    refused([bits(format=U64, param=7, **{"in": [arena(1000)]})], ["step 0 (KH_STEP_BITS)", "in[0]", "past the arena"])       # 4 x 8 bytes from 1000
    # what is allowed: the exact fit; rows, row0, row_stride and cells of a value step are ignored
    s = K.WitnessSchedule.create(0, 40, [bits(param=7, format=U64, rows=[99, 99, 99, 99], row0=1000, row_stride=0, **{"in": [arena(992)]}), inv(n=0, out=[None])],
                                 arena_bytes=1024, n_bufs=1)
    assert s.info() == dict(steps=2, launch_groups=1, resident_bytes=0, run_bytes=1024)
    s.free()


# ------------------------------------------------------------------------------------------------------------ 5. a schedule is its direct calls
COL_LEN, COL_STRIDE, ROWS_SRC = 128, 131, 10
N5, BITS5 = 65, 16


def value_chain_cells():
    rnd = random.Random(7500)
    src = some_cells(rnd, N5, col_len=ROWS_SRC, repeats=False)
    free = [(r, c) for r in range(16, COL_LEN) for c in range(15)]
    take = lambda k: [free.pop(0) for _ in range(k)]
    return src, take(N5), take(N5), take(N5), take(BITS5 * N5)


def value_chain_steps(K):
    src, t_inv, t_root, t_sq, t_bits = value_chain_cells()
    e = 32 * N5
    return [dict(op=K.STEP_GATHER, cells=src, format=FIELD, out=[arena(0)]),
            dict(op=K.STEP_INVERSE, n=N5, out=[arena(e)], flag_bit=1, **{"in": [arena(0)]}),
            dict(op=K.STEP_SQRT, n=N5, out=[arena(2 * e), arena(3 * e)], flag_bit=2, **{"in": [arena(e)]}),
            dict(op=K.STEP_BITS, n=N5, format=FIELD, param=BITS5, out=[arena(4 * e)], flag_bit=3, **{"in": [arena(2 * e)]}),
            dict(op=K.STEP_SCATTER, cells=t_inv, format=FIELD, **{"in": [arena(e)]}),
            dict(op=K.STEP_SCATTER, cells=t_root, format=FIELD, **{"in": [arena(2 * e)]}),
            dict(op=K.STEP_SCATTER, cells=t_sq, format=FIELD, **{"in": [arena(3 * e)]}),
            dict(op=K.STEP_SCATTER, cells=t_bits, format=FIELD, **{"in": [arena(4 * e)]})], (4 + BITS5) * e


def value_chain_direct(K, fid, wit, flags):
    src, t_inv, t_root, t_sq, t_bits = value_chain_cells()
    x, inv, root, sq, bits = [K.DevBuf(32 * N5) for _ in range(4)] + [K.DevBuf(32 * N5 * BITS5)]
    K.witness_gather_dev(fid, wit, COL_STRIDE, COL_LEN, src, FIELD, x)
    K.field_inverse_dev(fid, x, N5, inv, flags=flags, bit=1)
    K.field_sqrt_dev(fid, inv, N5, root, out_is_square=sq, flags=flags, bit=2)
    K.field_bits_dev(fid, root, FIELD, BITS5, N5, bits, flags=flags, bit=3)
    for buf, cells in ((inv, t_inv), (root, t_root), (sq, t_sq), (bits, t_bits)):
        K.witness_scatter_dev(fid, buf, FIELD, cells, wit, COL_STRIDE, COL_LEN)
    return [x, inv, root, sq, bits]


@pytest.mark.parametrize("fid", [0, 1])
def test_schedule_equals_the_direct_calls(khip, fid):
    K, F = khip, FIELDS[fid]
    steps, arena_bytes = value_chain_steps(K)
    sched = K.WitnessSchedule.create(fid, COL_LEN, steps, arena_bytes=arena_bytes, n_bufs=0)
    info = sched.info()
    assert (info["steps"], info["launch_groups"], info["run_bytes"]) == (8, 1 + 3 + 1, arena_bytes), info      # a gather, three value steps, four scatters as one
    src_cells = value_chain_cells()[0]
    seen = []
    for run in range(2):
        rnd = random.Random(7510 + 2 * fid + run)
        vals = random_witness(F, rnd, COL_STRIDE)
        for k, (r, c) in enumerate(src_cells):                     # inverses of squares and of non-residues, small roots, a zero
            w = rnd.randrange(1, 1 << (BITS5 if k % 3 == 0 else 200))
            vals[c][r] = 0 if k == 7 + run else pow(w * w * (5 if k % 5 == 1 else 1), -1, F.p)
        before = np.tile(SENTINEL, (15, COL_STRIDE, 1))
        before[:, :ROWS_SRC] = witness_limbs(F, vals)[:, :ROWS_SRC]
        w1, w2 = K.DevBuf(before.nbytes).upload(before), K.DevBuf(before.nbytes).upload(before)
        f1, f2 = (K.DevBuf(4).upload(np.array([PRESET & ~0xe], dtype=np.uint32)) for _ in range(2))
        s0 = K.counter("table_staged_words")
        sched.run([], w1, col_stride=COL_STRIDE, flags=f1)
        assert K.counter("table_staged_words") == s0, "a run staged a table"
        scratch = value_chain_direct(K, fid, w2, f2)
        assert K.counter("table_staged_words") > s0               # (the direct calls stage their cells)
        got = w1.download(before.shape)
        assert np.array_equal(got, w2.download(before.shape)), run
        assert flag_word(f1) == flag_word(f2) == (PRESET & ~0xe) | 0xe, run      # a zero, a non-residue, a root of more than 16 bits
        # ... and the values, against the oracle: the inverse cells of the first instances
        _src, t_inv, t_root, _t_sq, t_bits = value_chain_cells()
        for k in range(8):
            x = vals[src_cells[k][1]][src_cells[k][0]]
            inv = pow(x, -1, F.p) if x else 0
            root = F.sqrt(inv) or 0
            assert unmont(F, got[t_inv[k][1], t_inv[k][0]]) == [inv] and unmont(F, got[t_root[k][1], t_root[k][0]]) == [root]
            for j in range(BITS5):
                r, c = t_bits[j * N5 + k]
                assert unmont(F, got[c, r]) == [(root >> j) & 1], (k, j)
        seen.append(got)
        free_all(w1, w2, f1, f2, *scratch)
    assert not np.array_equal(seen[0], seen[1])
    sched.free()
    # a value step between two arena gathers: two groups and the step; without it the gathers are one launch
    g = lambda off: dict(op=K.STEP_GATHER, cells=[(0, 0), (1, 1)], format=FIELD, out=[arena(off)])
    value = dict(op=K.STEP_INVERSE, n=2, out=[arena(64)], **{"in": [arena(0)]})
    for steps, groups in (([g(0), value, g(128)], 3), ([g(0), g(128)], 1)):
        s = K.WitnessSchedule.create(fid, COL_LEN, steps, arena_bytes=192, n_bufs=0)
        assert s.info()["launch_groups"] == groups
        s.free()


# ------------------------------------------------------------------------------------------------------------ 6. device inputs to an accepted proof
def wire(gates, pairs):
    for a, b in pairs:
        CC.connect_cell_pair(gates, a, b)


def proved(khip, fid, gates, steps, arena_bytes, bufs, rows, broken=None):
    """The witness by ONE run from the bound buffers; kh_witness_check on the device; a proof from witness_dev with no kh_sync, verified; the download
    against the oracle's verify_witness.  broken = (steps, bufs): the same circuit with a step replaced -- returns that run's report as well."""
    from proof_systems_amd import prover
    K, F = khip, FIELDS[fid]
    cs = CC.build(F, gates)
    n = cs["n"]
    assert n <= 1 << 9
    srs = K.Srs.create(fid, n)
    ix = prover.CreatedIndex(srs, *records(F, gates), public=0)
    assert ix.n == n
    sched = K.WitnessSchedule.create(fid, n, steps, arena_bytes=arena_bytes, n_bufs=len(bufs))
    wit, flags = K.DevBuf(32 * 15 * n).zero(), K.DevBuf(4).zero()
    sched.run(bufs, wit, flags=flags)
    both = K.WITNESS_GATES | K.WITNESS_WIRES
    rep = ix.native.witness_check(witness_dev=wit, flags=both)
    assert rep.kind == K.WITNESS_OK, K.witness_report_message(rep)
    sections, _ph = ix.native.prove(witness_dev=wit, flags=K.PROVE_CHECK)
    vix = K.VerifierIndex.of(ix.native)
    proof = K.Proof(sections)
    ok, _trace = K.verify(vix, proof)
    assert ok
    assert flag_word(flags) == 0
    got = wit.download((15, n, 4))
    assert not got[:, rows:].any()
    vals = unmont(F, got[:, :rows])
    cols = [vals[rows * c:rows * (c + 1)] for c in range(15)]
    CC.verify_witness(cs, cols)
    bad_rep = None
    if broken is not None:
        bsched = K.WitnessSchedule.create(fid, n, broken[0], arena_bytes=arena_bytes, n_bufs=len(broken[1]))
        bwit = K.DevBuf(32 * 15 * n).zero()
        bsched.run(broken[1], bwit)
        bad_rep = ix.native.witness_check(witness_dev=bwit, flags=both)
        bsched.free(); bwit.free()
    proof.free(); vix.free(); ix.free(); srs.close(); sched.free()
    free_all(wit, flags)
    return cols, bad_rep


@pytest.mark.parametrize("fid", [0, 1])
def test_is_zero_circuit(khip, fid):
    """b = 1 - x y and x b = 0 as the two halves of one generic row per instance, y = the INVERSE step's "inverse or zero" with no flag"""
    K, F, n = khip, FIELDS[fid], 65
    p = F.p
    rnd = random.Random(7600 + fid)
    xs = [0, 0, 0] + [rnd.randrange(1, p) for _ in range(n - 5)] + [0, 1]
    first_nonzero = 3
    half0, half1 = [0, 0, 1, 1, -1 % p], [0, 0, 0, 1, 0]
    gates = [CC.generic_gadget(p, i, half0, half1) for i in range(n)]
    wire(gates, [((i, 0), (i, 3)) for i in range(n)] + [((i, 2), (i, 4)) for i in range(n)])
    e = 32 * n

    def steps(y):
        return [dict(op=K.STEP_GENERIC, n=n, row0=0, row_stride=1, param=0, consts=mont(F, half0), out=[arena(e)], **{"in": [(0, 0), y]}),
                dict(op=K.STEP_GENERIC, n=n, row0=0, row_stride=1, param=1, consts=mont(F, half1), **{"in": [(0, 0), arena(e)]})]

    inverse = dict(op=K.STEP_INVERSE, n=n, out=[arena(0)], **{"in": [(0, 0)]})          # flag_bit: KH_STEP_NO_FLAG
    x, zeros = K.DevBuf(e).upload(mont(F, xs)), K.DevBuf(e).zero()
    cols, bad = proved(K, fid, gates, [inverse] + steps(arena(0)), 2 * e, [x], n, broken=(steps((1, 0)), [x, zeros]))
    assert cols[0] == xs and cols[1] == [pow(v, -1, p) if v else 0 for v in xs] and cols[2] == [int(v == 0) for v in xs]
    # without the inverse (y = 0: b = 1) the first instance with x != 0 fails x b = 0
    assert bad.kind == K.WITNESS_GATE and bad.row == first_nonzero, K.witness_report_message(bad)
    assert bad.gate_rows_violated == sum(1 for v in xs if v)
    free_all(x, zeros)


@pytest.mark.parametrize("fid", [0, 1])
def test_decompression_circuit(khip, fid):
    """y from x: generic rows compute x^3 + 5, the SQRT step gives y, a generic y * y row is wired to the x^3 + 5 cell"""
    K, F, n = khip, FIELDS[fid], 65
    p = F.p
    crv = P.CURVES[1 - fid]                                        # the curve over this field
    assert crv.base is F
    rnd = random.Random(7700 + fid)
    pts = [crv.mul(crv.gen, rnd.randrange(1, 1 << 64)) for _ in range(n)]
    xs = [pt[0] for pt in pts]
    mul, cube5 = CC.generic_spec(p, "Mul"), [0, 0, -1 % p, 1, 5]
    gates = []
    for i in range(n):
        gates += [CC.generic_gadget(p, 2 * i, mul, cube5), CC.generic_gadget(p, 2 * i + 1, mul)]
    for i in range(n):
        a, b = 2 * i, 2 * i + 1
        wire(gates, [((a, 0), (a, 1)), ((a, 0), (a, 4)), ((a, 2), (a, 3)), ((a, 5), (b, 2)), ((b, 0), (b, 1))])
    e = 32 * n
    steps = [dict(op=K.STEP_GENERIC, n=n, row0=0, row_stride=2, param=0, consts=mont(F, mul), out=[arena(0)], **{"in": [(0, 0), (0, 0)]}),
             dict(op=K.STEP_GENERIC, n=n, row0=0, row_stride=2, param=1, consts=mont(F, cube5), out=[arena(e)], **{"in": [arena(0), (0, 0)]}),
             dict(op=K.STEP_SQRT, n=n, out=[arena(2 * e)], flag_bit=0, **{"in": [arena(e)]}),
             dict(op=K.STEP_GENERIC, n=n, row0=1, row_stride=2, param=0, consts=mont(F, mul), **{"in": [arena(2 * e), arena(2 * e)]})]
    x = K.DevBuf(e).upload(mont(F, xs))
    cols, _ = proved(K, fid, gates, steps, 3 * e, [x], 2 * n)
    ys = cols[0][1::2]
    assert ys == [F.sqrt((v ** 3 + 5) % p) for v in xs] and all(y in (pt[1], p - pt[1]) for y, pt in zip(ys, pts))
    x.free()


@pytest.mark.parametrize("fid", [0, 1])
def test_bit_decomposition_circuit(khip, fid):
    """8 bits of 33 values: the BITS step, a booleanity half per bit, an accumulating chain of generic halves wired back to the value.
    Instance i takes rows 8 i .. 8 i + 7; row j: cells 0..2 = (b_j, b_j, 0) with b^2 - b = 0; cells 3..5 = (v, 0, 0) unconstrained for j = 0,
    (acc_{j-1}, b_j, acc_j = acc_{j-1} + 2^j b_j) after it (acc_0 = b_0); acc_7 is wired to v."""
    K, F, n, nb = khip, FIELDS[fid], 33, 8
    p = F.p
    rnd = random.Random(7800 + fid)
    vs = [0, 255, 1, 128] + [rnd.randrange(256) for _ in range(n - 4)]
    boolean, free = [-1 % p, 0, 0, 1, 0], [0, 0, 0, 0, 0]
    acc = lambda j: [1, 1 << j, -1 % p, 0, 0]
    gates = [CC.generic_gadget(p, nb * i + j, boolean, acc(j) if j else free) for i in range(n) for j in range(nb)]
    for i in range(n):
        r = nb * i
        wire(gates, [((r, 0), (r, 1)), ((r, 0), (r + 1, 3))])
        for j in range(1, nb):
            wire(gates, [((r + j, 0), (r + j, 1)), ((r + j, 0), (r + j, 4))])
        wire(gates, [((r + j, 5), (r + j + 1, 3)) for j in range(1, nb - 1)] + [((r + nb - 1, 5), (r, 3))])
    e = 32 * n
    bit = lambda j: arena(e * j)
    accs = lambda j: arena(e * (nb + j))
    steps = [dict(op=K.STEP_BITS, n=n, format=FIELD, param=nb, out=[arena(0)], flag_bit=0, **{"in": [(0, 0)]})]
    steps += [dict(op=K.STEP_GENERIC, n=n, row0=j, row_stride=nb, param=0, consts=mont(F, boolean), **{"in": [bit(j), bit(j)]}) for j in range(nb)]
    steps += [dict(op=K.STEP_GENERIC, n=n, row0=0, row_stride=nb, param=1, consts=mont(F, free), **{"in": [(0, 0)]})]
    steps += [dict(op=K.STEP_GENERIC, n=n, row0=j, row_stride=nb, param=1, consts=mont(F, acc(j)), out=[accs(j)], **{"in": [bit(0) if j == 1 else accs(j - 1), bit(j)]})
              for j in range(1, nb)]
    v = K.DevBuf(e).upload(mont(F, vs))
    cols, _ = proved(K, fid, gates, steps, 2 * nb * e, [v], nb * n)
    assert [cols[0][nb * i + j] for i in range(n) for j in range(nb)] == [(x >> j) & 1 for x in vs for j in range(nb)]
    assert cols[5][nb - 1::nb] == vs and cols[3][0::nb] == vs
    v.free()
