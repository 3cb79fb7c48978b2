"""CPU-side checks of the drop-in boundary: the C-ABI library builds for gfx950, loads, and
exports every symbol include/kimchi_hip.h declares; and it fails loudly (no CPU fallback)
when no GPU is present.  No compute calls here."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def khip():
    import __graft_entry__ as ge
    ge.build()                      # no-op when libkimchi_hip.so is up to date
    import proof_systems_amd.khip as k
    return k


def _declared_functions():
    src = open(os.path.join(ROOT, "include", "kimchi_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(kh_[a-z_0-9]+)\s*\(", src)))


def test_header_symbols_exported(khip):
    decl = _declared_functions()
    assert len(decl) >= 20
    lib = ctypes.CDLL(khip.LIB_PATH)
    for name in decl:
        assert hasattr(lib, name), f"{name} declared in kimchi_hip.h but not exported"
    assert sorted(khip.SYMBOLS) == decl


def _header_source():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kimchi_hip.h")).read(), flags=re.S)


BY_VALUE = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "size_t": ctypes.c_size_t, "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32,
            "uint8_t": ctypes.c_uint8, "double": ctypes.c_double, "float": ctypes.c_float}


def _is_pointer_type(t):
    return t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer))


def test_binding_declares_the_argument_types_of_every_function(khip):
    """ctypes passes an undeclared Python int as a 32-bit C int: a function with a size_t / uint64_t / pointer parameter that the binding calls without
    `argtypes` gets garbage in the upper halves (round 6: kh_msm_submit_host asked hipMalloc for 6.6 EB).  EVERY function of the header has its argument
    list declared with the header's arity, every by-value position with exactly the header's type, every pointer position as a pointer, and the header's
    return type.  (The header is parsed here with this test's own regexes, not with the binding's parser.)"""
    decls = {m.group(2): (m.group(1).strip(), m.group(3)) for m in re.finditer(r"([A-Za-z_][\w \*]*?)\b(kh_[a-z_0-9]+)\s*\(([^;{}]*?)\)\s*;", _header_source())}
    assert sorted(decls) == _declared_functions()
    restypes = {"int": ctypes.c_int, "void": None, "size_t": ctypes.c_size_t, "uint64_t": ctypes.c_uint64, "const char *": ctypes.c_char_p}
    lib = khip.raw()
    for name, (ret, args) in sorted(decls.items()):
        fn = getattr(lib, name)
        assert fn.restype is restypes[ret], f"{name}: restype {fn.restype} for `{ret}`"
        params = [] if args.strip() in ("", "void") else [" ".join(a.split()) for a in args.split(",")]
        at = fn.argtypes
        assert at is not None, f"{name}({args}): argtypes not declared"
        assert len(at) == len(params), f"{name}: {len(at)} argtypes for ({args})"
        for t, param in zip(at, params):
            if "*" in param or "[" in param:
                assert _is_pointer_type(t), f"{name}: `{param}` declared as {t}"
            else:
                base, = [w for w in param.split()[:-1] if w != "const"]
                assert t is BY_VALUE[base], f"{name}: `{param}` declared as {t}"
    # the pointer rule, pinned: a device address takes a Python int, a host array of device addresses an array of them, host data its element type
    P = ctypes.POINTER
    assert lib.kh_msm_batch_dev.argtypes[4] is ctypes.c_void_p                                   # const uint64_t *scalars_dev
    assert lib.kh_prover_index_attach_runtime_tables.argtypes[1:4] == [ctypes.c_void_p] * 3     # const uint64_t *selector_*_dev
    assert lib.kh_gate_evaluations_dev.argtypes[2] is P(ctypes.c_void_p)                        # const uint64_t *const *cols_dev
    assert lib.kh_prover_index_attach_lookup.argtypes[3] is P(ctypes.c_void_p)                  # const uint64_t *const *selectors_d1_dev
    assert lib.kh_srs_create.argtypes == [ctypes.c_int, P(ctypes.c_uint64), ctypes.c_size_t, P(ctypes.c_void_p)]      # handle out-parameter
    assert lib.kh_comm_init.argtypes[2] is P(ctypes.c_uint8)                                     # const uint8_t id[128]
    assert lib.kh_dev_upload.argtypes[:2] == [ctypes.c_void_p, ctypes.c_void_p]                  # void *dst_dev, const void *src_host
    assert lib.kh_last_timings.argtypes[0] is P(ctypes.c_char_p) and lib.kh_counter.argtypes == [ctypes.c_char_p]
    assert lib.kh_witness_check.argtypes[5] is P(khip.WitnessReportC) and lib.kh_debug_lookup_column.argtypes[3] is P(P(ctypes.c_uint64))


def test_structures_have_the_layout_of_the_header(khip, tmp_path):
    """The four records a caller fills in: the binding's Structure classes have the typedefs' field names in order and the size the C compiler gives them."""
    import subprocess
    classes = {"kh_lookup_table_t": khip.LookupTableC, "kh_runtime_table_cfg_t": khip.RuntimeTableCfgC, "kh_witness_report_t": khip.WitnessReportC,
               "kh_witness_lookup_t": khip.WitnessLookupC}
    typedefs = dict((name, body) for body, name in re.findall(r"typedef\s+struct\s*\{([^}]*)\}\s*(kh_[a-z_0-9]+)\s*;", _header_source()))
    assert sorted(typedefs) == sorted(classes)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "kimchi_hip.h"\nint main(void) { printf("' + " ".join(["%zu"] * len(classes)) + '\\n", '
                   + ", ".join(f"sizeof({n})" for n in classes) + "); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    for (name, cls), size in zip(classes.items(), sizes):
        fields = [f for decl in typedefs[name].split(";") for f in re.findall(r"(\w+)\s*(?:\[\d+\]\s*)*(?:,|$)", decl.strip())]      # `size_t width, len`, `entry[3][4]`
        assert [f for f, _t in cls._fields_] == fields, name
        assert ctypes.sizeof(cls) == size, f"{name}: ctypes {ctypes.sizeof(cls)} bytes, gcc {size}"


def test_every_constant_of_the_header_is_in_the_binding(khip):
    """KH_X of the header (#define or anonymous enum) is khip.X, with the header's value; the short names and the section tables are those constants."""
    src = _header_source()
    consts = dict(re.findall(r"#define\s+(KH_[A-Z0-9_]+)\s+\(?(-?\d+)\)?", src))
    for body in re.findall(r"enum\s*\{([^}]*)\}", src):
        consts.update(re.findall(r"(KH_[A-Z0-9_]+)\s*=\s*(-?\d+)", body))
    assert len(consts) >= 73
    for name, value in consts.items():
        assert getattr(khip, name[3:]) == int(value), name
    assert (khip.VESTA, khip.PALLAS, khip.FP, khip.FQ, khip.Sponge.FQ, khip.Sponge.FR) == tuple(
        int(consts["KH_" + n]) for n in ("CURVE_VESTA", "CURVE_PALLAS", "FIELD_FP", "FIELD_FQ", "SPONGE_FQ", "SPONGE_FR"))
    for table, prefix in ((khip.PROOF_SECTIONS, "KH_PROOF_"), (khip.VINDEX_SECTIONS, "KH_VINDEX_"), (khip.LOOKUP_COLUMN_BLOCKS, "KH_LOOKUP_COL_")):
        assert table == {n[len(prefix):].lower(): int(v) for n, v in consts.items() if n.startswith(prefix)} and len(table) >= 7


def test_missing_header_is_an_import_error(khip, tmp_path):
    """The binding is declared from the header: a copy of the package without include/kimchi_hip.h beside it fails to import and names the path (it does
    not come up with undeclared functions).  Its own process: the import must fail as a user's would."""
    import shutil
    import subprocess
    import sys
    pkg = tmp_path / "proof_systems_amd"
    pkg.mkdir()
    for f in ("__init__.py", "_abi.py", "khip.py"):
        shutil.copy(os.path.join(ROOT, "proof_systems_amd", f), pkg / f)
    r = subprocess.run([sys.executable, "-c", "import proof_systems_amd.khip"], cwd=tmp_path, env=dict(os.environ, KH_LIB=khip.LIB_PATH, PYTHONPATH=str(tmp_path)),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "ImportError" in r.stderr and str(tmp_path / "include" / "kimchi_hip.h") in r.stderr, r.stderr[-2000:]


def test_no_oracle_in_product():
    """The product path must never route through the oracle or any CPU fallback."""
    pkg = os.path.join(ROOT, "proof_systems_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cuh", ".inc", ".h")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "pasta_ref" not in txt and "from oracle" not in txt and "import oracle" not in txt, f


def test_fails_loudly_without_gpu(khip):
    if khip.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(khip.KhError) as e:
        khip.init(0)
    assert "no CPU fallback" in str(e.value)
    import numpy as np
    with pytest.raises(khip.KhError):
        khip.ntt(khip.FP, np.zeros((4, 4), np.uint64), 2)


def test_header_is_plain_c99(tmp_path):
    """The drop-in boundary is a C ABI: include/kimchi_hip.h must compile as strict C99 (a cgo / bindgen / ctypes consumer
    sees exactly this file)."""
    import subprocess
    src = tmp_path / "hdr.c"
    src.write_text('#include "kimchi_hip.h"\nint main(void) { return KH_OK + KH_TOK_LOAD - KH_TOK_LOAD + KH_SCAN_ADD; }\n')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(root, "include"), "-fsyntax-only", str(src)])


def test_integration_build_line_names_every_source():
    """INTEGRATION.md spells the manual build out as csrc/{...}.hip csrc/{...}.cpp: the two lists are exactly __graft_entry__.SOURCES."""
    import __graft_entry__ as ge
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    named = []
    for stems, ext in re.findall(r"csrc/\{([a-z_0-9,]+)\}\.(hip|cpp)", txt):
        named += [s + "." + ext for s in stems.split(",")]
    assert sorted(named) == sorted(ge.SOURCES)
