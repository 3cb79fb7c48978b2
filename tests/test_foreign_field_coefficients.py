"""kh_foreign_field_gate_coefficients (host only, no device): the coefficients a gate list carries on its ForeignFieldMul and ForeignFieldAdd rows --
f2, then the limbs of 2^264 - f; then f0, f1, f2 -- against Python's integers, both fields, and the moduli it refuses."""
import ctypes as C

import numpy as np
import pytest

from oracle import pasta as P

L = 1 << 88
MODULI = ((1 << 256) - (1 << 32) - 977, P.Fp.p, (1 << 259) - 1, 1, 3, (1 << 264) - 1, 1 << 263, L, L * L + 5)


def limbs3(x):
    return [x % L, (x >> 88) % L, x >> 176]


@pytest.fixture(scope="module")
def khip():
    import proof_systems_amd.khip as k
    return k


@pytest.mark.parametrize("fid", [0, 1])
def test_coefficients_are_the_limbs_of_f_and_of_its_negation(khip, fid):
    F = (P.Fp, P.Fq)[fid]
    R = 1 << 256
    for f in MODULI:
        got = khip.foreign_field_gate_coefficients(fid, f)
        fl, nf = limbs3(f), limbs3((1 << 264) - f)
        want = [fl[2]] + nf + fl
        assert got.shape == (7, 4)
        assert [int.from_bytes(g.tobytes(), "little") for g in got] == [v * R % F.p for v in want], hex(f)


def test_refusals(khip):
    lib = khip.raw()
    out = np.full((7, 4), 0x5a5a5a5a5a5a5a5a, dtype=np.uint64)
    keep = out.copy()
    po = out.ctypes.data_as(C.POINTER(C.c_uint64))
    mod_t = C.c_uint64 * 6
    good = mod_t(1, 0, 0, 0, 0, 0)
    for what, args in (("f = 0", (0, mod_t(0, 0, 0, 0, 0, 0), po)), ("limb 0 = 2^88", (0, mod_t(0, 1 << 24, 0, 0, 0, 0), po)),
                       ("limb 2 = 2^88", (1, mod_t(5, 0, 0, 0, 0, 1 << 24), po)), ("limb 1 high word", (1, mod_t(5, 0, 0, 1 << 63, 0, 0), po)),
                       ("unknown field", (2, good, po)), ("null modulus", (0, None, po)), ("null output", (0, good, None))):
        assert lib.kh_foreign_field_gate_coefficients(*args) == khip.E_INVALID, what
        assert "kh_foreign_field_gate_coefficients" in lib.kh_last_error().decode(), what
        assert np.array_equal(out, keep), what
    with pytest.raises(khip.KhError):
        khip.foreign_field_gate_coefficients(0, 0)
    assert lib.kh_foreign_field_gate_coefficients(0, good, po) == 0 and not np.array_equal(out, keep)
