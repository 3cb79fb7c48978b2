"""The KH_* environment switches of the library: one reader (csrc/env.hpp), one table ("Environment switches"), and the reader's
semantics.  Host code only: no device work."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "proof_systems_amd", "csrc")


def _sources():
    return {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".cpp", ".hpp", ".cuh", ".inc"))}


def test_the_library_reads_its_environment_through_one_reader():
    """getenv( occurs in env.hpp, and once more for the launcher's LOCAL_RANK."""
    sites = [(f, line.strip()) for f, src in _sources().items() if f != "env.hpp" for line in src.split("\n") if "getenv(" in line]
    assert len(sites) == 1 and sites[0][0] == "context.hip" and 'getenv("LOCAL_RANK")' in sites[0][1], sites
    assert _sources()["env.hpp"].count("getenv(") == 2          # env_flag, env_int


def test_the_table_of_switches_matches_the_code():
    """Every name passed to env_flag / env_int has a row in INTEGRATION.md's table with that type, and every row names a switch the code reads."""
    in_code = {}
    for f, src in _sources().items():
        for kind, name in re.findall(r'\benv_(flag|int)\(\s*"([^"]+)"', src):
            assert in_code.setdefault(name, kind) == kind, f"{name} is read both as a flag and as an int"
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = doc[doc.index("Environment switches"):]
    in_table = dict((name, kind) for name, kind in re.findall(r"^\| `(KH_[A-Z0-9_]+)` \| (flag|int) \|", section, flags=re.M))
    assert len(in_code) >= 20 and all(n.startswith("KH_") for n in in_code)
    assert in_table == in_code, (sorted(set(in_code) - set(in_table)), sorted(set(in_table) - set(in_code)),
                                 sorted(n for n in set(in_code) & set(in_table) if in_code[n] != in_table[n]))


@pytest.fixture(scope="module")
def reader(tmp_path_factory):
    d = tmp_path_factory.mktemp("env_reader")
    src = d / "reader.cpp"
    src.write_text('#include <stdio.h>\n'
                   '#include "env.hpp"\n'
                   'int main() {\n'
                   '    printf("%d %d %lld\\n", (int)kh::env_flag("KH_T", false), (int)kh::env_flag("KH_T", true), kh::env_int("KH_T", 7));\n'
                   '    return 0;\n'
                   '}\n')
    exe = d / "reader"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", str(exe), str(src)])

    def run(value):
        env = {k: v for k, v in os.environ.items() if k != "KH_T"}
        if value is not None:
            env["KH_T"] = value
        return [int(x) for x in subprocess.check_output([str(exe)], env=env).split()]
    return run


@pytest.mark.parametrize("value, flag_default_off, flag_default_on, number",
                         [(None, 0, 1, 7), ("", 0, 1, 7), ("0", 0, 0, 0), ("1", 1, 1, 1), ("yes", 1, 1, 7), ("12", 1, 1, 12), ("0x10", 1, 1, 16), ("abc", 1, 1, 7)])
def test_reader_semantics(reader, value, flag_default_off, flag_default_on, number):
    """env_flag: unset or empty = the default, exactly "0" = off, anything else = on.  env_int: unset, empty or not a number = the default (7 here),
    otherwise strtoll with base 0."""
    assert reader(value) == [flag_default_off, flag_default_on, number]
