"""Poseidon on the device, the part that needs no GPU: the coefficient rows kh_poseidon_gate_coefficients hands a gate list (host code), and
the generated constants of csrc/poseidon.hip.  Both come from tests/golden/poseidon_kimchi_params.json, the reference's fp_kimchi.rs / fq_kimchi.rs."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import gates as G
from oracle import pasta as P
from oracle import poseidon as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def khip():
    import proof_systems_amd.khip as k
    return k


@pytest.mark.parametrize("fid", [0, 1])
def test_gate_coefficients_are_the_oracles_coefficient_rows(khip, fid):
    """out[15 r + c] = round constant (5 r + c / 3)[c % 3]: exactly the 11 coefficient rows oracle.gates.poseidon_witness gives the gadget (its twelfth,
    the output row, has none), as canonical Montgomery limbs."""
    F = (P.Fp, P.Fq)[fid]
    par = S.params(("fp", "fq")[fid])
    _w, co, _out = G.poseidon_witness(F, [1, 2, 3], par["mds"], par["rc"], 11)
    assert len(co) == 12 and not any(co[11])
    want = np.array([[P.to_limbs(F.to_mont(v)) for v in row] for row in co[:11]], dtype=np.uint64)
    got = khip.poseidon_gate_coefficients(fid)
    assert got.shape == (11, 15, 4) and np.array_equal(got, want)
    assert len({tuple(x) for x in got.reshape(-1, 4).tolist()}) == 165              # 55 x 3 different constants, none repeated or dropped


def test_unknown_field_and_null_output_are_refused(khip):
    out = np.zeros((11, 15, 4), dtype=np.uint64)
    lib = khip.raw()
    assert lib.kh_poseidon_gate_coefficients(2, out.ctypes.data_as(khip.U64P)) == khip.E_INVALID and lib.kh_last_error()
    assert lib.kh_poseidon_gate_coefficients(0, None) == khip.E_INVALID and lib.kh_last_error()
    assert not out.any()


def test_generated_constants_are_fresh():
    """csrc/poseidon_params.inc (host sponge) and csrc/poseidon_dev_params.inc (device kernels) are what tools/gen_poseidon_params.py renders now."""
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_poseidon_params.py"), "--check"], cwd=ROOT).returncode == 0


def test_device_table_holds_the_reference_constants():
    """The device table read back from the generated text, word by word: 9 + 165 elements per field, each the Montgomery form of the JSON's integer."""
    import re
    txt = open(os.path.join(ROOT, "proof_systems_amd", "csrc", "poseidon_dev_params.inc")).read()
    for name, F in (("FP", P.Fp), ("FQ", P.Fq)):
        body = txt.split("#define KH_POSEIDON_DEV_" + name)[1].split("#define")[0]
        words = [int(w, 16) for w in re.findall(r"0x([0-9a-f]{8})u", body)]
        assert len(words) == 8 * (9 + 165)
        vals = [F.from_mont(sum(w << (32 * i) for i, w in enumerate(words[8 * k:8 * k + 8]))) for k in range(9 + 165)]
        par = S.params(name.lower())
        assert vals[:9] == [x for row in par["mds"] for x in row] and vals[9:] == [x for row in par["rc"] for x in row]
