"""CPU checks of the eight-limb (32-bit) field arithmetic of csrc/field_mulasm.inc: the four generated instruction streams
(Montgomery product, squaring, modular add, modular sub) are interpreted by tools/field_model.py and compared with Python
big integers on the definition; every instruction that writes VCC is driven to 0 and to 1 by a directed operand set or is
on a list of unreachable sites whose arithmetic bound the model asserts; and the checked-in .inc files must be what their
generators emit, so that these are checks of the code that is compiled."""
import importlib.util
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


fm = _load("field_model")
gen = fm.gen
cols = _load("gen_field_cols")

CASES = [(s, f) for f in fm.PRIMES for s in fm.STREAMS]


def test_generated_files_are_current():
    assert open(gen.INC_PATH).read() == gen.render()
    assert open(cols.INC_PATH).read() == cols.render()


def test_importing_the_generators_has_no_side_effect():
    """a fresh interpreter imports both generators: nothing printed, neither .inc rewritten"""
    before = [os.stat(m.INC_PATH).st_mtime_ns for m in (gen, cols)]
    code = ("import importlib.util, os\n"
            "for n in ('gen_field_asm', 'gen_field_cols'):\n"
            "    s = importlib.util.spec_from_file_location(n, os.path.join(%r, 'tools', n + '.py'))\n"
            "    m = importlib.util.module_from_spec(s); s.loader.exec_module(m)\n" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True)
    assert out.stdout == "" and out.stderr == ""
    assert [os.stat(m.INC_PATH).st_mtime_ns for m in (gen, cols)] == before


def test_stream_shapes():
    """the instruction counts DESIGN.md quotes, and the carry sites: one per MAC, one per v_addc behind it, eight per chain"""
    n = {s: len(fm.stream(s).prog) for s in fm.STREAMS}
    assert n == {"mul": 254, "sqr": 211, "add": 24, "sub": 22}
    mads = lambda s: sum(op == "v_mad_u64_u32" for op, _ in fm.stream(s).prog)
    assert mads("mul") == 104 and len(fm.stream("mul").sites) == 2 * 104 + 8
    assert mads("sqr") == 76 and len(fm.stream("sqr").sites) == 2 * 76 + 8
    assert len(fm.stream("add").sites) == 16 and len(fm.stream("sub").sites) == 16


def _edge_and_random(stream, p, nrand, seed):
    e = fm.edge_values(p)
    rnd = random.Random(seed)
    pairs = [(x, y) for x in e for y in e] + [(rnd.randrange(p), rnd.randrange(p)) for _ in range(nrand)]
    return [(x, x) for x, _ in pairs] if stream == "sqr" else pairs


@pytest.mark.parametrize("stream,field", CASES)
def test_streams_equal_big_integers(stream, field):
    """edge values pairwise (the 17 of test_gpu_parity.edge_fe: 289 pairs), 3000 random pairs and the directed set, with the
    accumulator bounds asserted on the way"""
    p = fm.PRIMES[field]
    for a, b in _edge_and_random(stream, p, 3000, 5):
        assert fm.evaluate(stream, p, a, b, check=True) == fm.reference(stream, p, a, b), (hex(a), hex(b))
    for v in fm.directed(stream, field):
        assert fm.evaluate(stream, p, v.a, v.b, check=v.canonical) == fm.reference(stream, p, v.a, v.b), v


@pytest.mark.parametrize("stream,field", CASES)
def test_directed_set_is_deterministic_and_holds_the_named_cases(stream, field):
    fm.directed.cache_clear()
    first = [(v.a, v.b, v.note) for v in fm.directed(stream, field)]
    fm.directed.cache_clear()
    assert [(v.a, v.b, v.note) for v in fm.directed(stream, field)] == first
    p = fm.PRIMES[field]
    vecs = fm.directed(stream, field)
    if stream in ("mul", "sqr"):
        ts = {fm.mont_t(p, v.a, v.b)[0] for v in vecs}
        assert {p - 1, p, p + 1, 0} <= ts
        if stream == "mul":
            assert 2 * p - 1 in ts
        else:                                               # a < 2^255 keeps t below 2^254 + p < 2p - 1
            assert (2 * p - max(ts)) * 1000 < p and (1 << 255) - 1 in {v.a for v in vecs}
            assert p - 1 in {v.a for v in vecs}
            for j in range(2, 8):
                assert any(fm.limbs(v.a)[j - 1] >> 31 for v in vecs)
        assert any(v.a and v.b and fm.reference(stream, p, v.a, v.b) == 0 for v in vecs)          # result 0 through t = p
        for k in range(8):                                  # m_k = 0 with non-zero operands
            assert any(v.a and v.b and (fm.mont_t(p, v.a, v.b)[1] >> (32 * k)) & fm.M32 == 0 for v in vecs), k
        plow = p % (1 << 128)
        for top in (1 << 30, (1 << 30) + 1):                # limbs 4..6 zero under an incoming borrow, both sides of p
            assert any(t >> 224 == top and (t >> 128) % (1 << 96) == 0 and t % (1 << 128) < plow for t in ts), top
    elif stream == "add":
        assert {p - 1, p, p + 1, 2 * p - 2} <= {v.a + v.b for v in vecs}
    else:
        assert any(v.a == v.b != 0 for v in vecs) and any(v.a == v.b - 1 for v in vecs) and any(v.a == 0 != v.b for v in vecs)


@pytest.mark.parametrize("stream,field", CASES)
def test_every_carry_site_is_toggled_or_bounded(stream, field):
    """Every instruction that writes VCC produces 0 and 1 somewhere in the directed set (canonical operands only), or is on
    the unreachable list -- never neither, never both.  The list is derived from operand bounds alone (field_model.site_bounds)
    and test_streams_equal_big_integers asserts those bounds on every vector.  Measured: product 98 toggled + 118 bounded (all
    104 third-word v_addc; both MACs of column 0; the first MAC of columns 1 and 7..12, which adds onto a pair whose high word
    is the small carry count; every MAC of columns 13 and 14), squaring 70 + 90 (76 v_addc and the same MACs plus the first of
    column 2), add 15 + 1 (limb 7: a + b < 2^255), sub 16 + 0."""
    S = fm.stream(stream)
    p = fm.PRIMES[field]
    cov = fm.coverage(stream, field)
    un = fm.unreachable(S, p)
    assert set(cov) == set(S.sites)
    for i in S.sites:
        assert 0 in cov[i], (i, S.lines[i])
        if i in un:
            assert 1 not in cov[i], f"site {i} ({S.lines[i]}) is listed unreachable ({un[i]}) but a vector toggles it"
        else:
            assert 1 in cov[i], f"site {i} ({S.lines[i]}) is neither toggled nor on the unreachable list"
    # the same over edge + random operands: nothing may ever toggle a bounded site
    tr = {}
    for a, b in _edge_and_random(stream, p, 300, 9):
        fm.run(S, S.operand_map(p, a, b), trace=tr)
    assert not [i for i in un if 1 in tr.get(i, ())]


def _missed_by(stream, p, pairs):
    """the reachable mutants that a plain operand list does not notice"""
    S = fm.stream(stream)
    un = fm.unreachable(S, p)
    want = [fm.reference(stream, p, a, b) for a, b in pairs]
    missed = []
    for c, site in fm.mutants(stream).items():
        if site in un:
            continue
        if all(fm.evaluate(stream, p, a, b, mutate=c) == w for (a, b), w in zip(pairs, want)):
            missed.append(c)
    return missed


@pytest.mark.parametrize("stream,field", CASES)
def test_directed_vectors_catch_every_reachable_mutant(stream, field):
    """Every carry-consuming instruction (the v_addc behind a MAC, the v_subb / v_subbrev / v_addc links of the chains, each
    v_cndmask of the selection) is run in its non-carry form, one at a time, on the vectors tagged with the site whose carry it
    consumes: at least one of them must come out wrong.  Consumers of a bounded site are exempt (their carry is never 1).

    Measured with _missed_by on the 289 edge pairs + 3000 random pairs (seed 5) that test_streams_equal_big_integers also runs --
    the shape of operand set the suite had before this file -- for either prime: that set misses 7 of the 105 reachable product
    mutants (the v_addc behind the m_k * 1 MAC of columns 1..7: its carry needs a high word of exactly 0xffffffff), 14 of the 77
    squaring mutants (the same seven, the v_addc behind the first MAC of columns 3, 4, 5, and four links of the trial subtraction:
    t_0 = 0 and limbs 4..6 zero under a borrow), and none of the 22 add and 15 sub mutants (the edge values already ripple)."""
    S = fm.stream(stream)
    p = fm.PRIMES[field]
    un = fm.unreachable(S, p)
    vecs = fm.directed(stream, field)
    n = 0
    for c, site in fm.mutants(stream).items():
        if site in un:
            continue
        n += 1
        mine = [v for v in vecs if site in v.tags and v.canonical]
        assert mine, (c, S.lines[c])
        assert any(fm.evaluate(stream, p, v.a, v.b, mutate=c) != fm.reference(stream, p, v.a, v.b) for v in mine), \
            f"mutant of {c} ({S.lines[c]}) survives its {len(mine)} vectors"
    assert n >= {"mul": 100, "sqr": 70, "add": 20, "sub": 15}[stream]
