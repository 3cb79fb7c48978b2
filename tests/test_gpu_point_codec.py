"""Compressed points on the device (csrc/point_codec.hip, csrc/srs_file.hpp): kh_points_compress / kh_points_decompress and their _dev vector steps,
the SRS from records and from a file, kh_proofs_from_wire.  Exact equality everywhere: the encoder against cref.compress byte for byte, the decoder
against the encoder's inputs and against oracle.pasta.Curve.decompress, the 2^16 SRS against the golden digests with the product doing the encoding.
The statuses of malformed records are the library's own contract (include/kimchi_hip.h), checked as stated there."""
import hashlib
import os
import sys

import numpy as np
import pytest

from oracle import cref
from oracle import pasta as P
from oracle import views as V

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

CURVES = ["vesta", "pallas"]
SIZES = [1, 63, 64, 65, 257]
GUARD = 64


@pytest.fixture(scope="module")
def khip():
    import proof_systems_amd.khip as k
    k.init(0)
    return k


@pytest.fixture(scope="module")
def basis():
    """{curve id: 1024 SRS points}: computed once, shared, never written"""
    out = {cid: cref.srs_generate(cid, 0, 1 << 10, threads=8) for cid in (0, 1)}
    for g in out.values():
        g.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def srs16(khip):
    made = {}

    def get(cid):
        if cid not in made:
            made[cid] = khip.Srs.create(cid, 1 << 16)
        return made[cid]
    yield get
    for s in made.values():
        s.close()


def case(basis, cid, n):
    """n points with infinity bytes at 0, 63, 64 and n - 1, and the records cref.compress gives for them"""
    xy = np.ascontiguousarray(basis[cid][:n])
    inf = np.zeros(n, dtype=np.uint8)
    for i in (0, 63, 64, n - 1):
        if i < n:
            inf[i] = 1
    return xy, inf, cref.compress(cid, xy, inf)


def non_residue_x(c):
    """the smallest x >= 2 with x^3 + 5 a non-residue of the curve's base field"""
    x = 2
    while c.base.is_square((x * x * x + c.b) % c.base.p):
        x += 1
    return x


def record(x: int, flag: int):
    return np.frombuffer(x.to_bytes(32, "little") + bytes([flag]), dtype=np.uint8)


def counter(khip):
    return khip.counter("point_codec_launches")


# ---------------------------------------------------------------------------------------------------- 1. encode
@pytest.mark.parametrize("name", CURVES)
@pytest.mark.parametrize("n", SIZES)
def test_compress_equals_the_oracle_byte_for_byte(khip, basis, name, n):
    cid = P.CURVES[name].cid
    xy, inf, want = case(basis, cid, n)
    if n >= 63:         # both sign flags inside one wave, beside the infinity records
        assert {0x00, 0x80, 0x40} <= set(int(f) for f in want[:64, 32])
    # host arrays, with a guard region behind `out`
    out = np.full(n * 33 + GUARD, 0xA5, dtype=np.uint8)
    lib = khip.raw()
    assert lib.kh_points_compress(cid, khip._p64(xy), khip._p8(inf), n, khip._p8(out)) == 0
    assert np.array_equal(out[:n * 33].reshape(n, 33), want) and np.all(out[n * 33:] == 0xA5)
    assert np.array_equal(khip.points_compress(cid, xy, inf), want)
    # no infinity bytes: the same records as an all-zero array of them
    assert np.array_equal(khip.points_compress(cid, xy), cref.compress(cid, xy))
    # an infinity byte wins over whatever xy holds
    assert np.array_equal(khip.points_compress(cid, xy, np.ones(n, np.uint8)), np.tile(record(0, 0x40), (n, 1)))
    # the vector step
    dxy = khip.DevBuf(n * 64).upload(xy); dinf = khip.DevBuf(n).upload(inf)
    dout = khip.DevBuf(n * 33 + GUARD).upload(np.full(n * 33 + GUARD, 0xA5, dtype=np.uint8))
    khip.points_compress_dev(cid, dxy, dinf, n, dout)
    got = dout.download((n * 33 + GUARD,), np.uint8)
    assert np.array_equal(got[:n * 33].reshape(n, 33), want) and np.all(got[n * 33:] == 0xA5)
    khip.points_compress_dev(cid, dxy, None, n, dout)
    assert np.array_equal(dout.download((n, 33), np.uint8), cref.compress(cid, xy))
    for b in (dxy, dinf, dout):
        b.free()


# ---------------------------------------------------------------------------------------------------- 2. decode
@pytest.mark.parametrize("name", CURVES)
@pytest.mark.parametrize("n", SIZES)
def test_decompress_gives_the_points_back(khip, basis, name, n):
    c = P.CURVES[name]; cid = c.cid
    xy, inf, rec = case(basis, cid, n)
    want_xy = xy.copy(); want_xy[inf != 0] = 0          # xy of an infinity record is zero
    want_st = np.where(inf != 0, khip.POINT_INFINITY, khip.POINT_OK).astype(np.uint8)
    rc, gxy, ginf, gst, first = khip.points_decompress_raw(cid, rec)
    assert rc == 0 and first is None
    assert np.array_equal(gxy, want_xy) and np.array_equal(ginf, inf) and np.array_equal(gst, want_st)
    # the vector step, with guard regions behind every output
    drec = khip.DevBuf(n * 33).upload(rec)
    dxy = khip.DevBuf(n * 64 + GUARD).upload(np.full(n * 64 + GUARD, 0xA5, dtype=np.uint8))
    dinf = khip.DevBuf(n + GUARD).upload(np.full(n + GUARD, 0xA5, dtype=np.uint8))
    dst = khip.DevBuf(n + GUARD).upload(np.full(n + GUARD, 0xA5, dtype=np.uint8))
    flags = khip.DevBuf(4).upload(np.array([0x5], dtype=np.uint32))
    khip.points_decompress_dev(cid, drec, n, dxy, dinf, dst, flags, 4)
    bxy = dxy.download((n * 64 + GUARD,), np.uint8)
    assert np.array_equal(bxy[:n * 64].view(np.uint64).reshape(n, 8), want_xy) and np.all(bxy[n * 64:] == 0xA5)
    binf, bst = dinf.download((n + GUARD,), np.uint8), dst.download((n + GUARD,), np.uint8)
    assert np.array_equal(binf[:n], inf) and np.all(binf[n:] == 0xA5)
    assert np.array_equal(bst[:n], want_st) and np.all(bst[n:] == 0xA5)
    assert int(flags.download((1,), np.uint32)[0]) == 0x5, "a call with no bad record touched the flag word"
    # status_dev is nullable
    khip.points_decompress_dev(cid, drec, n, dxy, dinf, None, None, 0)
    assert np.array_equal(dxy.download((n, 8)), want_xy)
    for b in (drec, dxy, dinf, dst, flags):
        b.free()
    # tied to the oracle's decoder, not only to the library's own encoder
    for i in range(min(n, 64)):
        pt = c.decompress(bytes(rec[i]))
        if pt is None:
            assert ginf[i] == 1
        else:
            got = tuple(c.base.from_mont(P.from_limbs(gxy[i, 4 * k:4 * k + 4])) for k in (0, 1))
            assert got == pt and ginf[i] == 0, i


# ---------------------------------------------------------------------------------------------------- 3. malformed records
def malformed(khip, c):
    p = c.base.p
    return [(3, record(p, 0x00), khip.POINT_NOT_CANONICAL), (10, record((1 << 256) - 1, 0x80), khip.POINT_NOT_CANONICAL),
            (17, None, khip.POINT_BAD_FLAGS),            # flag 0xC0 on a valid x
            (30, None, khip.POINT_BAD_FLAGS),            # flag 0x01 on a valid x
            (45, record(1, 0x40), khip.POINT_BAD_FLAGS), (60, record(non_residue_x(c), 0x00), khip.POINT_NOT_ON_CURVE)]


@pytest.mark.parametrize("name", CURVES)
def test_malformed_records_get_their_status_and_spare_their_neighbours(khip, basis, name):
    c = P.CURVES[name]; cid = c.cid
    n = 70                                                  # the bad records share the first wave with valid ones; the second wave has none
    xy, inf, good = case(basis, cid, n)
    rec = good.copy()
    bad = malformed(khip, c)
    for i, r, _st in bad:
        if r is not None:
            rec[i] = r
    rec[17, 32] = 0xC0
    rec[30, 32] = 0x01
    want_xy = xy.copy(); want_xy[inf != 0] = 0
    want_inf = inf.copy()
    want_st = np.where(inf != 0, khip.POINT_INFINITY, khip.POINT_OK).astype(np.uint8)
    for i, _r, st in bad:
        want_xy[i] = 0; want_inf[i] = 0; want_st[i] = st
    rc, gxy, ginf, gst, first = khip.points_decompress_raw(cid, rec)
    assert rc == khip.E_INVALID and first == 3
    msg = khip.raw().kh_last_error().decode()
    assert "record 3 " in msg and "KH_POINT_NOT_CANONICAL" in msg
    assert np.array_equal(gst, want_st) and np.array_equal(gxy, want_xy) and np.array_equal(ginf, want_inf)
    with pytest.raises(khip.KhError):
        khip.points_decompress(cid, rec)
    # status = NULL and first_bad = NULL: the same return code and outputs
    oxy = np.zeros((n, 8), np.uint64); oinf = np.zeros(n, np.uint8)
    assert khip.raw().kh_points_decompress(cid, khip._p8(rec), n, khip._p64(oxy), khip._p8(oinf), None, None) == khip.E_INVALID
    assert np.array_equal(oxy, want_xy) and np.array_equal(oinf, want_inf)
    # the vector step: the bit is raised, the other bits of a preset flag word stay
    drec = khip.DevBuf(n * 33).upload(rec); dxy = khip.DevBuf(n * 64); dinf = khip.DevBuf(n); dst = khip.DevBuf(n)
    flags = khip.DevBuf(4).upload(np.array([0x5], dtype=np.uint32))
    khip.points_decompress_dev(cid, drec, n, dxy, dinf, dst, flags, 4)
    assert int(flags.download((1,), np.uint32)[0]) == 0x15
    assert np.array_equal(dxy.download((n, 8)), want_xy) and np.array_equal(dinf.download((n,), np.uint8), want_inf)
    assert np.array_equal(dst.download((n,), np.uint8), want_st)
    # flags_dev = NULL is accepted
    dst.upload(np.zeros(n, np.uint8))
    khip.points_decompress_dev(cid, drec, n, dxy, dinf, dst, None, 0)
    assert np.array_equal(dst.download((n,), np.uint8), want_st)
    # a call with no bad record leaves the flag word as it is
    drec.upload(good); flags.upload(np.array([0x5], dtype=np.uint32))
    khip.points_decompress_dev(cid, drec, n, dxy, dinf, dst, flags, 4)
    assert int(flags.download((1,), np.uint32)[0]) == 0x5
    for b in (drec, dxy, dinf, dst, flags):
        b.free()


# ---------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_happen_before_any_launch(khip, basis):
    lib = khip.raw()
    n = 8
    xy, inf, rec = case(basis, 0, n)
    rec = np.ascontiguousarray(rec)
    oxy = np.full((n + 1, 8), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64); oinf = np.full(n, 0xA5, np.uint8); ost = np.full(n, 0xA5, np.uint8)
    obytes = np.full((n, 33), 0xA5, np.uint8)
    assert oxy.ctypes.data % 16 == 0
    odd_out = (oxy.reshape(-1)[1:]).ctypes.data_as(khip.U64P)          # 8 bytes past a 16-byte boundary
    odd_in = np.concatenate([np.zeros(1, np.uint64), xy.reshape(-1)])
    odd_in = odd_in[1:] if odd_in.ctypes.data % 16 == 0 else odd_in[:-1]
    assert odd_in.ctypes.data % 16 == 8
    drec = khip.DevBuf(n * 33).upload(rec); dxy = khip.DevBuf(n * 64 + 64).upload(oxy); dinf = khip.DevBuf(n).upload(oinf); dst = khip.DevBuf(n).upload(ost)
    dbytes = khip.DevBuf(n * 33).upload(obytes)
    flags = khip.DevBuf(4).upload(np.array([0], dtype=np.uint32))
    vp = khip.C.c_void_p
    before = counter(khip)
    r8, x64, i8, s8 = khip._p8(rec), khip._p64(oxy), khip._p8(oinf), khip._p8(ost)
    refused = [
        lib.kh_points_decompress(2, r8, n, x64, i8, s8, None), lib.kh_points_decompress(-1, r8, n, x64, i8, s8, None),
        lib.kh_points_decompress(0, None, n, x64, i8, s8, None), lib.kh_points_decompress(0, r8, n, None, i8, s8, None),
        lib.kh_points_decompress(0, r8, n, x64, None, s8, None), lib.kh_points_decompress(0, r8, n, odd_out, i8, s8, None),
        lib.kh_points_decompress(0, r8, 1 << 32, x64, i8, s8, None), lib.kh_points_decompress(0, r8, 1 << 63, x64, i8, s8, None),
        lib.kh_points_decompress_dev(2, vp(drec.ptr), n, vp(dxy.ptr), vp(dinf.ptr), vp(dst.ptr), vp(flags.ptr), 0),
        lib.kh_points_decompress_dev(0, vp(0), n, vp(dxy.ptr), vp(dinf.ptr), vp(dst.ptr), vp(flags.ptr), 0),
        lib.kh_points_decompress_dev(0, vp(drec.ptr), n, vp(0), vp(dinf.ptr), vp(dst.ptr), vp(flags.ptr), 0),
        lib.kh_points_decompress_dev(0, vp(drec.ptr), n, vp(dxy.ptr), vp(0), vp(dst.ptr), vp(flags.ptr), 0),
        lib.kh_points_decompress_dev(0, vp(drec.ptr), n, vp(dxy.ptr + 8), vp(dinf.ptr), vp(dst.ptr), vp(flags.ptr), 0),
        lib.kh_points_decompress_dev(0, vp(drec.ptr), n, vp(dxy.ptr), vp(dinf.ptr), vp(dst.ptr), vp(flags.ptr), 32),
        lib.kh_points_decompress_dev(0, vp(drec.ptr), 1 << 32, vp(dxy.ptr), vp(dinf.ptr), vp(dst.ptr), vp(flags.ptr), 0),
        lib.kh_points_compress(2, khip._p64(xy), None, n, khip._p8(obytes)), lib.kh_points_compress(0, None, None, n, khip._p8(obytes)),
        lib.kh_points_compress(0, khip._p64(xy), None, n, None), lib.kh_points_compress(0, khip._p64(odd_in), None, n, khip._p8(obytes)),
        lib.kh_points_compress(0, khip._p64(xy), None, 1 << 32, khip._p8(obytes)),
        lib.kh_points_compress_dev(2, vp(dxy.ptr), vp(0), n, vp(dbytes.ptr)), lib.kh_points_compress_dev(0, vp(0), vp(0), n, vp(dbytes.ptr)),
        lib.kh_points_compress_dev(0, vp(dxy.ptr), vp(0), n, vp(0)), lib.kh_points_compress_dev(0, vp(dxy.ptr + 8), vp(0), n, vp(dbytes.ptr)),
        lib.kh_points_compress_dev(0, vp(dxy.ptr), vp(0), 1 << 32, vp(dbytes.ptr)),
    ]
    assert refused == [khip.E_INVALID] * len(refused)
    assert counter(khip) == before, "a refused call launched"
    khip.sync()
    assert np.all(oxy == 0xA5A5A5A5A5A5A5A5) and np.all(oinf == 0xA5) and np.all(ost == 0xA5) and np.all(obytes == 0xA5)
    assert np.all(dxy.download((n + 1, 8)) == 0xA5A5A5A5A5A5A5A5) and np.all(dinf.download((n,), np.uint8) == 0xA5) and np.all(dst.download((n,), np.uint8) == 0xA5)
    assert np.all(dbytes.download((n, 33), np.uint8) == 0xA5) and int(flags.download((1,), np.uint32)[0]) == 0
    # n == 0 is KH_OK with nothing launched
    assert lib.kh_points_decompress_dev(0, vp(0), 0, vp(0), vp(0), vp(0), vp(0), 0) == 0 and lib.kh_points_compress_dev(0, vp(0), vp(0), 0, vp(0)) == 0
    assert lib.kh_points_decompress(0, None, 0, None, None, None, None) == 0 and lib.kh_points_compress(0, None, None, 0, None) == 0
    assert counter(khip) == before
    # and an accepted call counts one launch
    khip.points_decompress_dev(0, drec, n, dxy, dinf, dst, flags, 0)
    assert counter(khip) == before + 1
    for b in (drec, dxy, dinf, dst, dbytes, flags):
        b.free()


# ---------------------------------------------------------------------------------------------------- 5. the SRS from records
def scalars(n, seed):
    sc = np.random.default_rng(seed).integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    sc[:, 3] &= np.uint64((1 << 61) - 1)
    return sc


@pytest.mark.parametrize("name", CURVES)
def test_srs_from_compressed_records(khip, basis, name):
    c = P.CURVES[name]; cid = c.cid
    n = 1 << 10
    g = basis[cid]
    rec = cref.compress(cid, g)
    before = counter(khip)
    srs = khip.Srs.from_compressed(cid, rec)
    assert counter(khip) == before + 1
    assert srs.n == n and np.array_equal(srs.get_g(), g)
    sc = scalars(n, 5)
    want = cref.msm(cid, g, sc, threads=8)
    got = srs.msm(sc)
    assert got[1] == want[1] and np.array_equal(got[0], want[0])
    assert np.array_equal(srs.blinding_commitment(), cref.srs_h(cid))          # without h_bytes: the curve's own
    assert np.array_equal(srs.get_g_compressed(5, 100), rec[5:105])
    srs.close()
    # with h_bytes: the blinding base is that point
    h = cref.srs_generate(cid, 7777, 1)
    srs = khip.Srs.from_compressed(cid, rec.tobytes(), cref.compress(cid, h).tobytes())
    assert np.array_equal(srs.blinding_commitment(), h[0]) and np.array_equal(srs.get_g(), g)
    got = srs.msm(sc)
    assert got[1] == want[1] and np.array_equal(got[0], want[0])
    srs.close()
    # a bad record names its index; an infinity record is no basis point; a bad h is refused too
    for r, status in ((record(non_residue_x(c), 0x80), "KH_POINT_NOT_ON_CURVE"), (record(c.base.p, 0), "KH_POINT_NOT_CANONICAL"), (record(0, 0x40), "KH_POINT_INFINITY")):
        bad = rec.copy(); bad[700] = r
        with pytest.raises(khip.KhError) as e:
            khip.Srs.from_compressed(cid, bad)
        assert e.value.code == khip.E_INVALID and "record 700 " in str(e.value) and status in str(e.value)
    with pytest.raises(khip.KhError) as e:
        khip.Srs.from_compressed(cid, rec, record(0, 0x40))
    assert e.value.code == khip.E_INVALID and "blinding base" in str(e.value)


@pytest.mark.parametrize("name", CURVES)
def test_device_srs_encodes_to_the_golden_digest(khip, srs16, golden, name):
    """the existing SRS parity test with the product doing the encoding"""
    cid = P.CURVES[name].cid
    comp = srs16(cid).get_g_compressed()
    assert comp.shape == (1 << 16, 33)
    assert hashlib.blake2b(comp.tobytes(), digest_size=32).hexdigest() == golden["srs"][name]["prefix_digest_blake2b256"]["16"]
    for idx, hx in golden["srs"][name]["samples"].items():
        assert bytes(comp[int(idx)]).hex() == hx


# ---------------------------------------------------------------------------------------------------- 6. the SRS file
@pytest.mark.parametrize("name", CURVES)
def test_srs_file_round_trip(khip, basis, srs16, golden, tmp_path, name):
    c = P.CURVES[name]; cid = c.cid
    n = 1 << 16
    data = srs16(cid).to_file_bytes()
    assert len(data) == 6 + 35 * (n + 1) == khip.raw().kh_srs_file_bytes(n)
    assert data[:6] == bytes([0x92, 0xdd, 0x00, 0x01, 0x00, 0x00])
    items = np.frombuffer(data, dtype=np.uint8, offset=6).reshape(n + 1, 35)
    assert np.all(items[:, 0] == 0xc4) and np.all(items[:, 1] == 0x21)
    assert hashlib.blake2b(items[:n, 2:].tobytes(), digest_size=32).hexdigest() == golden["srs"][name]["prefix_digest_blake2b256"]["16"]
    assert bytes(items[n, 2:]).hex() == golden["srs"][name]["h"]
    path = tmp_path / (name + ".srs")
    path.write_bytes(data)
    pts, h = P.read_srs_file(str(path), c, limit=8)
    assert pts == [bytes(r) for r in cref.compress(cid, basis[cid][:8])] and h == bytes(cref.compress(cid, cref.srs_h(cid).reshape(1, 8))[0])
    # read back, limited to 2^10 points: commits like the handle made from the records
    srs = khip.Srs.from_file_bytes(cid, data, limit=1 << 10)
    assert srs.n == 1 << 10 and np.array_equal(srs.get_g(), basis[cid]) and np.array_equal(srs.blinding_commitment(), cref.srs_h(cid))
    sc = scalars(1 << 10, 5)
    want = cref.msm(cid, basis[cid], sc, threads=8)
    got = srs.msm(sc)
    assert got[1] == want[1] and np.array_equal(got[0], want[0])
    srs.close()
    # a limit beyond the count keeps all; h still comes from the end
    small = data[:2] + (16).to_bytes(4, "big") + data[6:6 + 35 * 16] + data[-35:]
    srs = khip.Srs.from_file_bytes(cid, small, limit=100)
    assert srs.n == 16 and np.array_equal(srs.get_g(), basis[cid][:16]) and np.array_equal(srs.blinding_commitment(), cref.srs_h(cid))
    assert srs.to_file_bytes() == small
    srs.close()
    # broken files: no handle, KH_E_INVALID with the offset
    before = counter(khip)
    broken = [data[:cut] for cut in (0, 5, 6, 40, len(data) - 1)]
    broken.append(b"\x93" + data[1:])                                           # a wrong first marker
    broken.append(data[:2] + (n + 1).to_bytes(4, "big") + data[6:])             # a count one too large
    broken.append(small[:6 + 35 * 3] + b"\xc5" + small[6 + 35 * 3 + 1:])        # a wrong item marker
    for b in broken:
        with pytest.raises(khip.KhError) as e:
            khip.Srs.from_file_bytes(cid, b)
        assert e.value.code == khip.E_INVALID and "offset" in str(e.value), str(e.value)
    assert counter(khip) == before
    out = np.zeros(len(small) - 1, dtype=np.uint8)
    handle = khip.Srs.from_file_bytes(cid, small)
    assert khip.raw().kh_srs_write_file(handle._h, khip._p8(out), out.size) == khip.E_INVALID and not out.any()
    handle.close()


# ---------------------------------------------------------------------------------------------------- 7. proof intake
ELEMENTS = ("evals", "public_evals", "ft_eval1", "z1_z2", "challenges")
IGNORED = ("public_comm", "challenges")


@pytest.fixture(scope="module")
def fixture_proof(khip):
    """the proof of fixture bench_vesta_2_10 from kh_prove (test_gpu_index_create holds it to the committed bytes), its index and verifier index"""
    from test_gpu_index_create import fixture_case
    rec, _want, C_, ix, wit, prev = fixture_case(khip, "bench_vesta_2_10")
    F, nx = ix.F, ix.native
    rnd = F.limbs_many(F.rand_many(V.RefRng(P.StdRng(bytes.fromhex(rec["seed_hex"]))), nx.randomness_count(True)))
    sections = nx.prove(witness=wit, randomness=rnd, prev=prev)[0]
    vix = khip.VerifierIndex.of(nx)
    yield C_, ix, vix, sections
    vix.free(); ix.free()


def to_wire(cid, F, sections):
    """{section: bytes} as a serialised proof holds them: 33-byte records, 32-byte little-endian canonical scalars"""
    out = {}
    for name, v in sections.items():
        if isinstance(v, tuple):
            out[name] = bytearray(cref.compress(cid, v[0], v[1]).tobytes())
        else:
            out[name] = bytearray(b"".join(int(x).to_bytes(32, "little") for x in F.values(v)))
    return out


def same_sections(a, b, names):
    for name in names:
        x, y = a[name], b[name]
        if isinstance(x, tuple):
            if not (np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])):
                return False
        elif not np.array_equal(x, y):
            return False
    return True


def test_one_proof_from_wire_is_the_proof_from_affine_sections(khip, fixture_proof):
    C_, ix, vix, sections = fixture_proof
    wire = to_wire(C_.cid, ix.F, sections)
    before = counter(khip)
    proof, = khip.proofs_from_wire(C_.cid, [wire])
    assert counter(khip) == before + 1
    got = proof.sections()
    ref = khip.Proof(sections)
    assert same_sections(got, ref.sections(), khip.PROOF_SECTIONS)                # indistinguishable from a proof built from affine sections
    assert same_sections(got, sections, [s for s in khip.PROOF_SECTIONS if s not in IGNORED])
    ok, _trace = khip.verify(vix, proof)
    assert ok
    proof.free(); ref.free()


def test_three_proofs_from_wire_take_one_launch(khip, fixture_proof):
    C_, ix, vix, sections = fixture_proof
    wire = to_wire(C_.cid, ix.F, sections)
    flipped = {k: bytearray(v) for k, v in wire.items()}
    flipped["w_comm"][33 * 4 + 32] ^= 0x80                # the sign flag of one commitment: another point of the curve
    before = counter(khip)
    proofs = khip.proofs_from_wire(C_.cid, [wire, {k: bytearray(v) for k, v in wire.items()}, flipped])
    assert counter(khip) == before + 1, "the points of all the proofs go through ONE launch"
    ok, _tr = khip.batch_verify([(vix, p) for p in proofs])
    assert not ok
    assert [khip.verify(vix, p)[0] for p in proofs] == [True, True, False]
    third = proofs[2].sections()
    assert np.array_equal(third["w_comm"][0][4, :4], sections["w_comm"][0][4, :4]) and not np.array_equal(third["w_comm"][0][4, 4:], sections["w_comm"][0][4, 4:])
    for p in proofs:
        p.free()


def test_bad_wire_input_makes_no_proof(khip, fixture_proof):
    C_, ix, vix, sections = fixture_proof
    wire = to_wire(C_.cid, ix.F, sections)
    marker = 0x1234
    # an x with x^3 + 5 a non-residue in t_comm of the second proof
    bad = {k: bytearray(v) for k, v in wire.items()}
    bad["t_comm"][33 * 2:33 * 3] = bytes(record(non_residue_x(C_), 0x00))
    rc, out = khip.proofs_from_wire_raw(C_.cid, [wire, bad], out_before=marker)
    msg = khip.raw().kh_last_error().decode()
    assert rc == khip.E_INVALID and out == [marker, marker]
    assert "proof 1 section %d point 2 " % khip.PROOF_SECTIONS["t_comm"] in msg and "KH_POINT_NOT_ON_CURVE" in msg
    # an element >= p
    bad = {k: bytearray(v) for k, v in wire.items()}
    bad["evals"][32 * 3:32 * 4] = C_.scalar.p.to_bytes(32, "little")
    before = counter(khip)
    rc, out = khip.proofs_from_wire_raw(C_.cid, [bad, wire], out_before=marker)
    msg = khip.raw().kh_last_error().decode()
    assert rc == khip.E_INVALID and out == [marker, marker] and counter(khip) == before
    assert "proof 0 section %d element 3 " % khip.PROOF_SECTIONS["evals"] in msg
    # an unknown curve, no proofs
    assert khip.proofs_from_wire_raw(2, [wire], out_before=marker) == (khip.E_INVALID, [marker])
    assert khip.proofs_from_wire_raw(C_.cid, [], out_before=marker)[0] == khip.E_INVALID
