"""csrc/gates_check_gen.inc, the per-constraint check functions of kh_witness_check, is the output of tools/gen_gate_kernels.py::render_check for the
expressions of proof_systems_amd/polish.py as they are now; the generator's first output is untouched by its second."""
import os
import re
import sys

from oracle import gates as G
from proof_systems_amd import polish as OP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_gate_kernels as GK  # noqa: E402

CSRC = os.path.join(ROOT, "proof_systems_amd", "csrc")


def test_generated_check_functions_are_current():
    assert open(os.path.join(CSRC, "gates_check_gen.inc")).read() == GK.render_check()


def test_the_combined_gate_kernels_are_unchanged():
    assert open(os.path.join(CSRC, "gates_gen.inc")).read() == GK.render()


def test_every_check_function_declares_its_gates_constraints():
    src = open(os.path.join(CSRC, "gates_check_gen.inc")).read()
    want = {name: count for name, (_fn, count) in OP.GATES.items()}
    assert want == G.ROW_MACHINES
    want["Generic"] = 2
    declared = {m.group(1): int(m.group(2)) for m in re.finditer(r"^// (\w+): (\d+) constraints", src, flags=re.M)}
    assert declared == want
    for name, count in want.items():
        body = src[src.index("uint32_t gate_check_%s(" % name):]
        body = body[:body.index("\n}\n")]
        assert re.findall(r"<< (\d+);", body) == [str(i) for i in range(count)], name      # one comparison per constraint, in order
    counts = re.search(r"GATE_CHECK_NCONSTRAINTS\[GATE_CHECK_COUNT\] = \{([^}]*)\}", src).group(1)
    assert [int(x) for x in counts.split(",")] == [want[n] for n in list(OP.GATES) + ["Generic"]]
    # no alpha, no per-proof value: literals (kind 0) and the endo coefficient (kind 2) only
    assert set(re.findall(r"^    \{(\d), ", src, flags=re.M)) <= {"0", "2"}
