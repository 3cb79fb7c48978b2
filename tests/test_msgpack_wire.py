"""csrc/msgpack_wire.hpp and csrc/proof_wire.hpp, the framing and the structure walk behind kh_proofs_from_msgpack, kh_proof_to_msgpack and
kh_verifier_index_from_msgpack / _to_msgpack, on the host alone: tests/cpp/test_msgpack_wire.cpp round-trips the inner ProverProof and VerifierIndex bytes
of three stored reference proofs (a plain one, one with runtime lookup tables, the recursive one), walks every truncation length and every type byte
replaced by a foreign one over heap blocks of exactly the length the reader is told, and provokes each arity and consistency refusal by a minimal edit.
Built with g++ under AddressSanitizer and UBSan here -- host code only, no GPU, no library, nothing preloaded."""
import os
import subprocess

import msgpack

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURES = ("test_generic_gate", "test_runtime_table", "test_recursion")


def inner_bytes(name):
    """(ProverProof bytes, VerifierIndex bytes) of a stored RawFixture: both are arrays of small integers there (oracle/fixtures.py)"""
    raw = msgpack.unpackb(open(os.path.join(HERE, "golden", "ref_fixtures", name + ".bin"), "rb").read(), raw=True, strict_map_key=False)
    return bytes(raw[0]), bytes(raw[1])


def test_the_framing_and_the_structure_walk_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_msgpack_wire")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_msgpack_wire.cpp"), "-o", exe])
    files = []
    for name in FIXTURES:
        for kind, data in zip(("proof", "index"), inner_bytes(name)):
            files.append(str(tmp_path / f"{name}.{kind}"))
            with open(files[-1], "wb") as f:
                f.write(data)
    run = subprocess.run([exe] + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert run.returncode == 0 and "msgpack_wire OK" in run.stdout, (run.stdout[-3000:], run.stderr[-3000:])
