"""csrc/lookup_hash.hpp on the host against its Python mirror (tests/lookup_collisions.py): hash(Key), hash(Tuple) and lookup_slots, output for output.
The tests of the lookup tables build keys that collide under the MIRROR; this test is what makes them collide in the library: the header is the only
place the hash is written, the three device tables and host_lookup.cpp compile it, and tests/cpp/test_lookup_hash.cpp prints it.  Built with g++ under
AddressSanitizer and UBSan here -- host code only, no GPU, no library."""
import os
import random
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import lookup_collisions as LC  # noqa: E402

ONES = (1 << 64) - 1
SIZES = (1, 7, 8, 9, 64, 65, 4096, 4097, 1 << 20)


def make_requests():
    rnd = random.Random(20)
    key = lambda: tuple(rnd.getrandbits(64) for _ in range(4))
    keys = [key() for _ in range(2000)] + [(0, 0, 0, 0), (ONES,) * 4]
    keys += [tuple(v if j == limb else 0 for j in range(4)) for limb in range(4) for v in (1, ONES)]
    tuples = [tuple(key() for _ in range(4)) for _ in range(500)]
    a, b, c = key(), key(), key()
    tuples += [((0, 0, 0, 0), a, b, c),                            # a zero id
               (a, b, (0, 0, 0, 0), (0, 0, 0, 0)),                 # a zero tail
               (a, b, c, (0, 0, 0, 0)),
               (a, a, a, a), ((0, 0, 0, 0),) * 4, ((ONES,) * 4,) * 4]   # all parts equal
    return [("K", k) for k in keys] + [("T", t) for t in tuples] + [("L", n) for n in SIZES]


def test_the_header_and_the_python_mirror_agree(tmp_path):
    exe = str(tmp_path / "test_lookup_hash")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_lookup_hash.cpp"), "-o", exe])
    reqs = make_requests()
    assert len(reqs) == 2000 + 2 + 8 + 500 + 6 + len(SIZES)
    lines = []
    for op, v in reqs:
        limbs = v if op == "K" else [x for k in v for x in k] if op == "T" else [v]
        lines.append(" ".join([op] + ["%x" % x for x in limbs]))
    run = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    out = [int(x, 16) for x in run.stdout.split()]
    assert len(out) == len(reqs)
    for (op, v), got in zip(reqs, out):
        want = LC.key_hash(v) if op == "K" else LC.tuple_hash(*v) if op == "T" else LC.slots(v)
        assert got == want, (op, v, hex(got), hex(want))
    # the pinned rule itself, in numbers: 16 slots up to 8 entries, then the next power of two of at least 2 L
    assert [LC.slots(n) for n in SIZES] == [16, 16, 16, 32, 128, 256, 8192, 16384, 1 << 21]
    # the hash is not constant on what the searches vary (a mirror and a header that both returned 0 would agree, too)
    assert len({LC.key_hash(v) for op, v in reqs if op == "K"}) == 2010 and len({LC.tuple_hash(*v) for op, v in reqs if op == "T"}) == 506


def test_the_collider_search_and_the_run_model():
    """what the directed tests rely on, on small numbers: colliders are canonical, distinct, in order and in the target slots; longest_run"""
    from oracle import pasta as P
    for F in (P.Fp, P.Fq):
        L = 48
        cap = LC.slots(L)
        assert cap == 128
        xs = LC.colliders(F, L, {cap - 2, cap - 1}, L)
        assert xs == sorted(set(xs)) and 1 <= xs[0] and xs[-1] < F.p and len(xs) == L
        assert all(LC.home(LC.mont_limbs(F, x), L) in (cap - 2, cap - 1) for x in xs)
        below = [x for x in range(1, xs[-1]) if LC.home(LC.mont_limbs(F, x), L) in (cap - 2, cap - 1)]
        assert below == xs[:-1], "the search skipped an element"
        more = LC.colliders(F, L, {3}, 2, exclude=xs)
        assert not set(more) & set(xs) and all(LC.home(LC.mont_limbs(F, x), L) == 3 for x in more)
        assert LC.colliders(F, L, {cap - 2, cap - 1}, 5, exclude=xs[:3]) == xs[3:8]
        ts = LC.tuple_colliders(F, 9, 508, {1022, 1023}, 6)
        assert ts == sorted(set(ts))
        assert all(LC.tuple_home(LC.mont_limbs(F, 9), LC.mont_limbs(F, x), LC.mont_limbs(F, x * x + 3), (0, 0, 0, 0), 508) in (1022, 1023) for x in ts)
    run = LC.longest_run([14, 15, 15, 14, 15], 16)
    assert run == ([14, 15, 0, 1, 2], True, 3, frozenset({14, 15, 0, 1, 2}))
    assert LC.longest_run([15], 16)[:3] == ([15], True, 0) and LC.longest_run([14], 16)[:3] == ([14], False, 0)
    assert LC.longest_run([14, 15], 16)[:3] == ([14, 15], False, 0) and LC.longest_run([15, 15], 16)[:3] == ([15, 0], True, 1)
    two = LC.longest_run([12, 13, 14, 15, 0, 1, 12, 0], 16)                 # two clusters that merge: the second one's keys are pushed behind the first's overflow
    assert two.slots == [12, 13, 14, 15, 0, 1, 2, 3] and two.wraps and two.displacement == 6
    assert LC.longest_run([3, 3, 9], 16)[:3] == ([3, 4], False, 1)
