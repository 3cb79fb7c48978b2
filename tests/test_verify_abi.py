"""The verifier's section of the C ABI (include/kimchi_hip.h: kh_verifier_index_*, kh_proof_from_sections, kh_verify, kh_batch_verify) without a GPU:
the symbols are exported and bound with the header's prototypes, the three records a caller fills in have the layout the C compiler gives them,
null arguments are refused before anything touches a device, and the generated Rust bindings are fresh."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VERIFIER_SYMBOLS = ["kh_verifier_index_of", "kh_verifier_index_new", "kh_verifier_index_digest", "kh_verifier_index_free", "kh_proof_from_sections",
                    "kh_batch_verify", "kh_verify", "kh_verify_last_phase_seconds"]


@pytest.fixture(scope="module")
def khip():
    import proof_systems_amd.khip as k
    return k


def test_symbols_are_exported_and_bound_with_the_headers_prototypes(khip):
    lib = khip.raw()
    P = ctypes.POINTER
    for s in VERIFIER_SYMBOLS:
        assert s in khip.SYMBOLS and getattr(lib, s).argtypes is not None, s
    assert lib.kh_verifier_index_of.argtypes == [ctypes.c_void_p, P(ctypes.c_void_p)]
    assert lib.kh_verifier_index_new.argtypes == [ctypes.c_void_p, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, P(ctypes.c_int), ctypes.c_size_t,
                                                  P(khip.SectionC), ctypes.c_size_t, P(ctypes.c_void_p)]
    assert lib.kh_proof_from_sections.argtypes == [P(khip.SectionC), ctypes.c_size_t, P(ctypes.c_void_p)]
    assert lib.kh_batch_verify.argtypes == [P(khip.VerifyItemC), ctypes.c_size_t, P(ctypes.c_uint64), P(ctypes.c_int), P(khip.VerifyTraceC)]
    assert lib.kh_verify.argtypes == [P(khip.VerifyItemC), P(ctypes.c_int), P(khip.VerifyTraceC)]
    assert lib.kh_verify.restype is ctypes.c_int and lib.kh_verifier_index_free.restype is None


def test_records_have_the_layout_of_the_header(khip, tmp_path):
    classes = {"kh_section_t": khip.SectionC, "kh_verify_item_t": khip.VerifyItemC, "kh_verify_trace_t": khip.VerifyTraceC}
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kimchi_hip.h")).read(), flags=re.S)
    typedefs = dict((name, body) for body, name in re.findall(r"typedef\s+struct\s+kh_[a-z_]+\s*\{([^}]*)\}\s*(kh_[a-z_0-9]+)\s*;", src))
    assert sorted(typedefs) == sorted(classes)
    c = tmp_path / "sizes.c"
    c.write_text('#include <stdio.h>\n#include "kimchi_hip.h"\nint main(void) { printf("%zu %zu %zu\\n", ' + ", ".join(f"sizeof({n})" for n in classes) + "); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(c)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    for (name, cls), size in zip(classes.items(), sizes):
        fields = [f for decl in typedefs[name].split(";") for f in re.findall(r"(\w+)\s*(?:\[\d+\]\s*)*(?:,|$)", decl.strip())]
        assert [f for f, _t in cls._fields_] == fields, name
        assert ctypes.sizeof(cls) == size, f"{name}: ctypes {ctypes.sizeof(cls)} bytes, gcc {size}"
    assert ctypes.sizeof(khip.VerifyTraceC) == 10 * 32


def test_null_arguments_are_refused_without_a_device(khip):
    """kh_verify(NULL, ..) and an item without index or proof: KH_E_INVALID with a message, *ok untouched -- in a process that never initialised a device
    (kh_get_device() stays -1)."""
    code = ("import ctypes as C, proof_systems_amd.khip as k\n"
            "lib = k.raw(); ok = C.c_int(7)\n"
            "assert lib.kh_verify(None, C.byref(ok), None) == k.E_INVALID and ok.value == 7 and b'null' in lib.kh_last_error()\n"
            "item = (k.VerifyItemC * 1)()\n"
            "assert lib.kh_verify(item, None, None) == k.E_INVALID\n"
            "assert lib.kh_verify(item, C.byref(ok), None) == k.E_INVALID and ok.value == 7 and b'item 0' in lib.kh_last_error()\n"
            "assert lib.kh_batch_verify(item, 0, None, C.byref(ok), None) == k.E_INVALID and ok.value == 7\n"
            "out = C.c_void_p()\n"
            "assert lib.kh_verifier_index_of(None, C.byref(out)) == k.E_INVALID and lib.kh_proof_from_sections(None, 0, C.byref(out)) == k.E_INVALID\n"
            "assert lib.kh_verifier_index_new(None, 5, 3, 0, 0, None, 0, None, 0, C.byref(out)) == k.E_INVALID and not out.value\n"
            "assert lib.kh_get_device() == -1\n"
            "print('refused')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "refused" in r.stdout, r.stdout + r.stderr


def test_generated_rust_bindings_are_fresh():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_sys
    text = open(os.path.join(ROOT, "rust", "kimchi-hip-sys", "src", "lib.rs")).read()
    assert text == gen_rust_sys.render(), "rust/kimchi-hip-sys/src/lib.rs is stale: run tools/gen_rust_sys.py"
    for s in VERIFIER_SYMBOLS:
        assert f"pub fn {s}(" in text, s
    assert "pub struct kh_verify_item_t {" in text and "pub struct kh_verifier_index_t {" in text
