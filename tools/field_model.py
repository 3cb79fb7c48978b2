#!/usr/bin/env python3
"""CPU model of the eight-limb (32-bit) field arithmetic of proof_systems_amd/csrc/field_mulasm.inc.

The four instruction streams that tools/gen_field_asm.py emits (Montgomery product, squaring, modular add, modular sub)
are interpreted instruction by instruction on 32-bit registers with the VCC semantics of every opcode, and compared with
Python big integers on the definition (a b R^-1 mod p, a^2 R^-1 mod p, a +- b mod p, R = 2^256).  On top of that:

  * carry-site coverage: every instruction that WRITES VCC is a site; run() records which values each site produced;
  * a static bound per site (site_bounds): the true (unwrapped) value of the 96-bit column accumulator at every MAC, from
    the operand bounds alone.  A site whose bound stays below the wrap point can never produce VCC = 1: that is the
    explicit list of unreachable sites, and run(check=True) asserts every one of the bounds on every vector it executes;
  * directed(): a deterministic operand set per stream and prime that drives every other site to both values (the rare
    ones by solving for one limb through the model), plus the named edge cases listed in directed();
  * mutants(): the carry-consuming instructions, for the mutation check of tests/test_field_model.py.

python3 tools/field_model.py prints the coverage table.
"""
import functools
import importlib.util
import os
import random
from math import gcd

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("gen_field_asm", os.path.join(_HERE, "gen_field_asm.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

P_FP = 0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001
P_FQ = 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001
PRIMES = {"Fp": P_FP, "Fq": P_FQ}
W = 1 << 32
M32 = W - 1
R = 1 << 256
STREAMS = ("mul", "sqr", "add", "sub")


def limbs(x):
    return [(x >> (32 * i)) & M32 for i in range(8)]


def value(l):
    return sum(x << (32 * i) for i, x in enumerate(l))


def reference(stream, p, a, b):
    """The definition, on big integers."""
    if stream == "mul":
        return a * b * pow(R, -1, p) % p
    if stream == "sqr":
        return a * a * pow(R, -1, p) % p
    return (a + b) % p if stream == "add" else (a - b) % p


def mont_t(p, a, b):
    """(t, m) of the product scan: t = (a b + m p) / R is the value BEFORE the conditional subtraction."""
    m = -a * b * pow(p, -1, R) % R
    return (a * b + m * p) >> 256, m


# ----------------------------------------------------------------------------------------------- the streams
class Stream:
    """One generated instruction list, parsed: sites (VCC writers), consumers (VCC readers) and the column structure."""

    def __init__(self, name):
        self.name = name
        self.lines = {"mul": gen.gen_mul, "sqr": gen.gen_sqr, "add": gen.gen_add, "sub": gen.gen_sub}[name]()
        self.prog = []
        for ln in self.lines:
            op, rest = ln.split(None, 1)
            self.prog.append((op, [x.strip() for x in rest.split(",")]))
        self.sites = [i for i, (op, a) in enumerate(self.prog) if len(a) > 1 and a[1] == "vcc"]
        # consumer index -> the site whose VCC it reads
        self.consumers = {}
        last = None
        for i, (op, a) in enumerate(self.prog):
            if a[-1] == "vcc" and (op.startswith("v_cndmask") or len(a) == 5 and op != "v_mad_u64_u32"):
                self.consumers[i] = last
            if i in self.sites:
                last = i
        # column structure of the product scan: col[i] = column of instruction i, closing[k] = index of the m_k * 1 MAC
        self.col, self.closing, self.switch = {}, {}, set()
        if name in ("mul", "sqr"):
            k = 0
            for i, (op, a) in enumerate(self.prog):
                self.col[i] = k
                if op == "v_sub_u32":
                    self.closing[k] = i + 1
                if op == "v_mov_b32" and a[0] in ("v2", "v4") and a[1] in ("v3", "v5"):     # lo(Y) <- hi(X): next column
                    self.switch.add(i)
                    k += 1
                if op == "v_subrev_co_u32":
                    break
            self.tail = i                                  # first instruction of the conditional subtraction
            for j in range(i, len(self.prog)):
                self.col[j] = None

    def operand_map(self, p, a, b=None):
        """The registers as field.cuh binds them."""
        pl = limbs(p)
        regs = {f"%{8 + i}": x for i, x in enumerate(limbs(a))}
        if self.name == "sqr":
            regs.update({"%16": pl[1], "%17": pl[2], "%18": pl[3]})
        else:
            regs.update({f"%{16 + i}": x for i, x in enumerate(limbs(b))})
            regs.update({"%24": pl[1], "%25": pl[2], "%26": pl[3]})
        return regs


@functools.lru_cache(None)
def stream(name):
    return Stream(name)


def _const(tok):
    return {"0": 0, "1": 1, "-1": M32, "31": 31, "2.0": 0x40000000}.get(tok)


def site_bounds(S, p):
    """Static upper bounds, from the operand bounds alone (canonical operands: every limb <= 2^32 - 1, the top limb <= 2^30
    because a, b < p < 2^254 + 2^126; m_k <= 2^32 - 1; P1..P3 and 2^30 as they are).

    mul / sqr, per column: U = the true (unwrapped, 96-bit) value of the accumulator after each MAC
        = (U of the previous column) >> 32  +  sum of the products so far, each at its largest.
      A v_mad_u64_u32 whose U < 2^64 cannot carry out of the pair.  The v_addc_co_u32 behind every MAC adds that carry to the
      third word, which therefore never exceeds the number of MACs of its column (<= 13 < 2^32): none of them can carry out.
    add: a_7 + b_7 + carry <= 2^31 + 1 < 2^32 (limb 7 of the first chain).
    Returns {site: (kind, bound)}: ("acc", U) for a MAC, ("third", n) for its v_addc, ("limb", U) for add's limb 7."""
    out = {}
    if S.name == "add":
        out[7] = ("limb", 2 * (1 << 30) + 1)
        return out
    if S.name == "sub":
        return out
    pl = limbs(p)
    ub = {}
    for i in range(8):
        ub[f"%{8 + i}"] = M32 if i < 7 else 1 << 30
    if S.name == "mul":
        for i in range(8):
            ub[f"%{16 + i}"] = M32 if i < 7 else 1 << 30
        ub.update({"%24": pl[1], "%25": pl[2], "%26": pl[3]})
    else:
        ub.update({"%16": pl[1], "%17": pl[2], "%18": pl[3]})
    for k in range(8):
        ub[gen.M[k]] = M32
    U, n = 0, 0
    for i, (op, a) in enumerate(S.prog[:S.tail]):
        if op == "v_lshlrev_b32":                          # E = a_j << 1
            ub[a[0]] = min(M32 - 1, ub[a[2]] << 1)
        elif op == "v_alignbit_b32":                       # D_j = (a_j << 1) | (a_(j-1) >> 31)
            ub[a[0]] = min(M32, (ub[a[1]] << 1) | 1)
        elif op == "v_mad_u64_u32":
            x = ub[a[2]] if _const(a[2]) is None else _const(a[2])
            y = ub[a[3]] if _const(a[3]) is None else _const(a[3])
            U = (0 if a[4] == "0" else U) + x * y
            n += 1
            out[i] = ("acc", U)
            out[i + 1] = ("third", n)
        elif i in S.switch:
            U >>= 32
            n = 0
    return out


def unreachable(S, p):
    """The sites that can never produce VCC = 1, each with the bound that says so (see site_bounds)."""
    out = {}
    for i, (kind, bound) in site_bounds(S, p).items():
        if kind == "acc" and bound < (1 << 64):
            out[i] = f"accumulator <= {bound:#x} < 2^64"
        elif kind == "third":
            out[i] = f"third word <= {bound} MACs of the column"
        elif kind == "limb":
            out[i] = f"limb sum <= {bound:#x} < 2^32"
    return out


def run(S, regs, trace=None, mutate=None, snap=None, bounds=None):
    """Interprets S on regs (dict name -> 32-bit value; modified and returned).
    trace  : dict site -> set of VCC values, updated.
    mutate : index of ONE carry-consuming instruction executed in its non-carry form (the VCC input read as 0).
    snap   : index; a copy of the registers BEFORE that instruction is stored in regs['snap'].
    bounds : site_bounds(S, p): asserted on the way, together with the consistency of the 96-bit accumulator
             (pair = true value mod 2^64, third word = true value >> 64)."""
    vcc = 0
    tot = 0                                                # the true value of the column accumulator (mul / sqr)
    get = regs.__getitem__

    def val(tok):
        c = _const(tok)
        return get(tok) if c is None else c

    for idx, (op, a) in enumerate(S.prog):
        if idx == snap:
            regs["snap"] = dict(regs)
        cin = 0 if idx == mutate else vcc
        if op == "v_mad_u64_u32":
            d = a[0]
            lo, hi = ("v2", "v3") if d == "v[2:3]" else ("v4", "v5")
            add = 0 if a[4] == "0" else (regs[lo] | (regs[hi] << 32))
            v = val(a[2]) * val(a[3]) + add
            vcc = v >> 64
            regs[lo], regs[hi] = v & M32, (v >> 32) & M32
            if bounds is not None:
                tot = (0 if a[4] == "0" else tot) + val(a[2]) * val(a[3])
                assert tot <= bounds[idx][1], (S.name, idx, "accumulator bound")
                assert tot & ((1 << 64) - 1) == v & ((1 << 64) - 1)
        elif op == "v_addc_co_u32":
            v = val(a[2]) + val(a[3]) + cin
            vcc = v >> 32
            regs[a[0]] = v & M32
            if bounds is not None and idx in bounds:
                kind, bnd = bounds[idx]
                assert v <= bnd, (S.name, idx, kind)
                if kind == "third":
                    assert v == tot >> 64, (S.name, idx, "third word")
        elif op == "v_add_co_u32":
            v = val(a[2]) + val(a[3])
            vcc = v >> 32
            regs[a[0]] = v & M32
        elif op == "v_sub_u32":
            regs[a[0]] = (val(a[1]) - val(a[2])) & M32
        elif op == "v_sub_co_u32":
            v = val(a[2]) - val(a[3])
            vcc = 1 if v < 0 else 0
            regs[a[0]] = v & M32
        elif op == "v_subrev_co_u32":
            v = val(a[3]) - val(a[2])
            vcc = 1 if v < 0 else 0
            regs[a[0]] = v & M32
        elif op == "v_subb_co_u32":
            v = val(a[2]) - val(a[3]) - cin
            vcc = 1 if v < 0 else 0
            regs[a[0]] = v & M32
        elif op == "v_subbrev_co_u32":
            v = val(a[3]) - val(a[2]) - cin
            vcc = 1 if v < 0 else 0
            regs[a[0]] = v & M32
        elif op in ("v_cndmask_b32", "v_cndmask_b32_e64"):
            regs[a[0]] = val(a[2]) if cin else val(a[1])
        elif op == "v_and_b32":
            regs[a[0]] = val(a[1]) & val(a[2])
        elif op == "v_mov_b32":
            regs[a[0]] = val(a[1])
            if bounds is not None and idx in S.switch:
                tot >>= 32
        elif op == "v_lshlrev_b32":
            regs[a[0]] = (val(a[2]) << val(a[1])) & M32
        elif op == "v_alignbit_b32":
            regs[a[0]] = (((val(a[1]) << 32) | val(a[2])) >> val(a[3])) & M32
        else:
            raise ValueError(op)
        if trace is not None and len(a) > 1 and a[1] == "vcc":
            trace.setdefault(idx, set()).add(vcc)
    return regs


def evaluate(name, p, a, b=None, trace=None, mutate=None, check=False):
    """The result of stream `name` on the integers a, b (b ignored by sqr), as an integer."""
    S = stream(name)
    regs = S.operand_map(p, a, b)
    run(S, regs, trace=trace, mutate=mutate, bounds=site_bounds(S, p) if check else None)
    return value([regs[f"%{i}"] for i in range(8)])


# ----------------------------------------------------------------------------------------------- operand construction
def sqrt_mod(a, p):
    """Tonelli-Shanks (p - 1 = 2^32 * odd for both primes); None when a is not a square."""
    a %= p
    if a == 0:
        return 0
    if pow(a, (p - 1) // 2, p) != 1:
        return None
    q, s = p - 1, 0
    while q % 2 == 0:
        q //= 2; s += 1
    z = 2
    while pow(z, (p - 1) // 2, p) != p - 1:
        z += 1
    m, c, t, r = s, pow(z, q, p), pow(a, q, p), pow(a, (q + 1) // 2, p)
    while t != 1:
        i, tt = 0, t
        while tt != 1:
            tt = tt * tt % p; i += 1
        bb = pow(c, 1 << (m - i - 1), p)
        m, c = i, bb * bb % p
        t, r = t * c % p, r * bb % p
    return r


def solve_mul_t(p, T, a, blimit):
    """b < blimit with a b + m p = T R for some 0 <= m < R, i.e. the product scan of (a, b) arrives at exactly t = T; or None.
    m = T R / p (mod a) fixes m modulo a; every further a in m takes p off b."""
    if gcd(a, p) != 1:
        return None
    m0 = T * R * pow(p, -1, a) % a
    num = T * R - m0 * p
    if num < 0:
        return None
    b = num // a
    if b >= blimit:                                        # the largest b below blimit in the progression
        b -= -(-(b - blimit + 1) // p) * p
    if b < 0:
        return None
    return b if mont_t(p, a, b)[0] == T else None


def solve_sqr_t(p, T, alimit):
    """a < alimit whose squaring arrives at t = T before the conditional subtraction, or None."""
    s = sqrt_mod(T * R, p)
    if s is None:
        return None
    for a in sorted({s, p - s, p + s, 2 * p - s}):
        if a < alimit and mont_t(p, a, a)[0] == T:
            return a
    return None


HEAVY = (M32, M32, M32, M32 - 1, 1 << 31, (1 << 31) - 1, 0, 0, 1, 2)


def heavy_operand(rnd, p):
    """A canonical operand whose limbs favour the extremes."""
    while True:
        l = [rnd.choice(HEAVY) if rnd.random() < 0.7 else rnd.getrandbits(32) for _ in range(8)]
        l[7] = rnd.choice((0, 1, (1 << 30) - 1, rnd.getrandbits(30), rnd.getrandbits(30)))
        if value(l) < p:
            return value(l)


class Vector:
    __slots__ = ("a", "b", "note", "canonical", "tags")

    def __init__(self, a, b, note, canonical=True):
        self.a, self.b, self.note, self.canonical, self.tags = a, b, note, canonical, frozenset()

    def __repr__(self):
        return f"Vector({self.a:#x}, {self.b:#x}, {self.note!r})"


def _pair_at(S, p, a, b, idx):
    """The 64-bit pair that the MAC at idx adds onto, and the registers there."""
    regs = S.operand_map(p, a, b)
    run(S, regs, snap=idx)
    sn = regs["snap"]
    d = S.prog[idx][1][0]
    lo, hi = ("v2", "v3") if d == "v[2:3]" else ("v4", "v5")
    return sn[lo] | (sn[hi] << 32), sn


def _with_limb(x, k, v):
    l = limbs(x)
    l[k] = v
    return value(l)


def steer_column(S, p, rnd, k, idx, want, tries=64):
    """Operands for which the pair entering the MAC at idx (a MAC of column k <= 7, not the column's first) satisfies
    want(pair).  Limb k of the second operand (mul: b_k, sqr: a_k) enters column k through ONE product with a_0 and no
    earlier column at all, so the pair is C + g v (mod 2^64) in that limb v: solve for v, then confirm through the model.
    want = "carry": pair >= 2^64 - 2^32 + 1 (high word all ones, low word non-zero: any MAC >= 2^32 - lo carries out);
    want = "zero" : low word 0 (m_k = 0)."""
    sq = S.name == "sqr"
    for _ in range(tries):
        a = heavy_operand(rnd, p) if rnd.random() < 0.5 else rnd.randrange(p)
        a = _with_limb(a, 0, rnd.getrandbits(32) | 0x80000001)            # a_0 odd and large: steps below 2^32 cover 2^64
        if a >= p:
            continue
        b = a if sq else rnd.randrange(p)
        set_k = (lambda v: (_with_limb(a, k, v),) * 2) if sq else (lambda v: (a, _with_limb(b, k, v)))
        if sq and k == 0:
            return None
        c0, _ = _pair_at(S, p, *set_k(0), idx)
        c1, _ = _pair_at(S, p, *set_k(1), idx)
        g = (c1 - c0) % (1 << 64)
        if g == 0:
            continue
        if want == "carry":
            v = -(-((((M32 << 32) + 1) - c0) % (1 << 64)) // g)
        else:
            g32, c32 = g % W, c0 % W
            d = gcd(g32, W)
            if c32 % d:
                continue
            v = (-c32 // d) * pow(g32 // d, -1, W // d) % (W // d)
        if v >= (1 << 30 if k == 7 else (1 << 31 if sq else W)):
            continue
        x, y = set_k(v)
        if x >= p or y >= p:
            continue
        pair, _ = _pair_at(S, p, x, y, idx)
        if (want == "carry" and pair >> 32 == M32 and pair & M32) or (want == "zero" and pair & M32 == 0):
            return x, y
    return None


def edge_values(p):
    """The edge values of tests/test_gpu_parity.py edge_fe."""
    R1, R2 = R % p, R * R % p
    vals = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, 1 << 254, R1, R2, (1 << 32) - 1, 1 << 32, (1 << 64) - 1,
            1 << 64, (1 << 128) - 1, (1 << 192) + 5, p - (1 << 32), p - (1 << 200)]
    return [v % p for v in vals]


def _named_mul(S, p, rnd):
    """The named cases of the product / squaring."""
    sq = S.name == "sqr"
    out = []
    plow = p & ((1 << 128) - 1)

    def for_t(T, note, canonical_only=False):
        """operands that arrive at t = T before the conditional subtraction; canonical if there are any"""
        if sq:
            a = solve_sqr_t(p, T, p)
            if a is not None:
                out.append(Vector(a, a, note)); return True
            a = None if canonical_only else solve_sqr_t(p, T, 1 << 255)
            if a is not None:
                out.append(Vector(a, a, note + " (operand >= p)", canonical=False)); return True
            return False
        for _ in range(16):
            a = rnd.randrange(p // 2, p)
            b = solve_mul_t(p, T, a, p)
            if b is not None:
                out.append(Vector(a, b, note)); return True
        if canonical_only:
            return False
        for a in (p, (1 << 256) - 189, (1 << 256) - 1):
            b = solve_mul_t(p, T, a, 1 << 256)
            if b is not None:
                out.append(Vector(a, b, note + " (operand >= p)", canonical=False)); return True
        return False

    # t = p - 1, p, p + 1, 2p - 1.  Canonical operands give t < p (p / R + 1) < 1.25 p and t = p only for an operand that is a
    # multiple of p, so p and 2p - 1 take an operand >= p (the stream only needs t < 2p).  The squaring also needs a < 2^255,
    # hence t < 2^254 + p < 2p - 1: there the largest t among the 4096 operands just below 2^255 stands in (t > 2p - p / 1000).
    for T, note in ((p - 1, "t = p - 1"), (p, "t = p"), (p + 1, "t = p + 1")):
        assert for_t(T, note), note
    if not sq:
        assert for_t(2 * p - 1, "t = 2p - 1")
    else:
        a = max(range((1 << 255) - 4096, 1 << 255), key=lambda x: mont_t(p, x, x)[0])
        out.append(Vector(a, a, "largest t of the operands 2^255 - 4096 .. 2^255 - 1 (operand >= p)", canonical=False))
    out.append(Vector(0, 0, "result 0 from t = 0"))
    # t with limbs 4, 5, 6 zero under an incoming borrow (low four limbs below p's), top limb 2^30 (t < p) and 2^30 + 1 (t >= p);
    # t_0 = 0 (the first link borrows) with and without the rest of the chain
    n = 0
    while n < 4:
        low = rnd.randrange(plow)
        for top in ((1 << 30), (1 << 30) + 1):
            n += for_t((top << 224) | low, f"t limbs 4..6 zero under a borrow, t_7 = {top:#x}", canonical_only=True)
    n = 0
    while n < 4:
        T = rnd.randrange(p + p // 8) & ~M32
        n += for_t(T, "t_0 = 0", canonical_only=True)
        n += for_t((1 << 254) | (T & ((1 << 128) - 1)), "t_0 = 0, limbs 4..6 zero", canonical_only=True)
    if sq:
        for j in range(2, 8):                               # bit 31 of a_(j-1) feeds D_j
            l = [rnd.getrandbits(32) for _ in range(7)] + [rnd.getrandbits(29)]
            l[j - 1] |= 1 << 31
            out.append(Vector(value(l), value(l), f"bit 31 of a_{j - 1} set (D_{j})"))
            l = [0] * 8
            l[j - 1] = 1 << 31; l[0] |= 1
            out.append(Vector(value(l), value(l), f"only bit 31 of a_{j - 1} and a_0 = 1 (D_{j})"))
        out.append(Vector(p - 1, p - 1, "a = p - 1"))
        out.append(Vector((1 << 254) + plow - 1, (1 << 254) + plow - 1, "a_7 at its maximum 2^30, limbs 4..6 zero"))
        out.append(Vector((1 << 254) - 1, (1 << 254) - 1, "a = 2^254 - 1: every D_j all ones"))
        out.append(Vector((1 << 255) - 1, (1 << 255) - 1, "a = 2^255 - 1 (operand >= p): a_7 at the stream's own maximum", canonical=False))
    return out


def _named_addsub(S, p, rnd):
    out = []
    ones = lambda lo, hi: sum(M32 << (32 * i) for i in range(lo, hi))
    if S.name == "add":
        for s, note in ((p - 1, "a + b = p - 1"), (p, "a + b = p"), (p + 1, "a + b = p + 1"), (2 * p - 2, "a + b = 2p - 2")):
            for _ in range(3):
                a = rnd.randrange(max(0, s - p + 1), min(p, s + 1))
                out.append(Vector(a, s - a, note))
        out.append(Vector(p - 1, p - 1, "a = b = p - 1"))
        out.append(Vector(0, 0, "0 + 0"))
        # carries that ripple through all-ones limbs: a = ones in limbs 0..j-1, b = 1
        for j in range(1, 8):
            out.append(Vector(ones(0, j), 1, f"carry ripples through limbs 0..{j - 1}"))
            out.append(Vector(1, ones(0, j), f"carry ripples through limbs 0..{j - 1} (swapped)"))
        out.append(Vector(ones(0, 7) | ((1 << 29) << 224), ones(0, 7) | ((1 << 29) << 224), "all-ones limbs doubled"))
        # the sum with limbs 4..6 zero under a borrow of the trial subtraction, both sides of p; sum limb 0 = 0
        plow = p & ((1 << 128) - 1)
        for top in ((1 << 30), (1 << 30) + 1):
            s = (top << 224) | rnd.randrange(plow)
            a = rnd.randrange(s - p + 1, p)
            out.append(Vector(a, s - a, f"sum limbs 4..6 zero under a borrow, top limb {top:#x}"))
        for s in ((1 << 254), (1 << 254) + (5 << 32), rnd.randrange(p) & ~M32):
            a = rnd.randrange(max(0, s - p + 1), min(p, s + 1))
            out.append(Vector(a, s - a, "sum limb 0 = 0"))
    else:
        for _ in range(3):
            b = rnd.randrange(1, p)
            out += [Vector(b, b, "a = b"), Vector(b - 1, b, "a = b - 1"), Vector(0, b, "a = 0"), Vector(b, 0, "b = 0")]
        out += [Vector(0, 0, "0 - 0"), Vector(0, 1, "0 - 1"), Vector(0, p - 1, "0 - (p - 1)"), Vector(p - 1, 0, "(p - 1) - 0")]
        for j in range(1, 8):                               # borrows that ripple through zero limbs
            out.append(Vector(1 << (32 * j), 1, f"borrow ripples through zero limbs 0..{j - 1}"))
            out.append(Vector((1 << (32 * j)) + 5, 7, f"borrow ripples through zero limbs 1..{j - 1}"))
        # an add-back whose carry ripples through limbs 4..6: a - b + 2^256 = d with limbs 4..6 all ones and a carry out of limb 3
        plow = p & ((1 << 128) - 1)
        for _ in range(4):
            dlow = rnd.randrange((1 << 128) - plow, 1 << 128)       # dlow + plow >= 2^128
            d = (rnd.randrange((3 << 30), 1 << 32) << 224) | ones(4, 7) | dlow
            diff = (1 << 256) - d                                    # b - a
            if diff >= p:
                continue
            a = rnd.randrange(0, p - diff)
            out.append(Vector(a, a + diff, "add-back carry ripples through limbs 4..6"))
        for _ in range(2):                                           # ... and the same with limb 0 = 0xffffffff alone (first link)
            diff = rnd.randrange(1, p) & ~M32 | 1
            a = rnd.randrange(0, p - diff)
            out.append(Vector(a, a + diff, "difference limb 0 = 0xffffffff: the add-back's first link carries"))
    return out


@functools.lru_cache(None)
def directed(name, pname):
    """The directed operand set of one stream for one prime: a deterministic function of (stream, prime).
    1. the named cases (_named_mul / _named_addsub);
    2. operands with extreme limbs, kept when they show a (site, VCC value) not seen before;
    3. for every site of the product scan still missing a value: solve for the one limb that steers its column;
       m_k = 0 for every k the same way.
    Every vector is tagged with the sites at which it produces VCC = 1.  Coverage counts canonical vectors only."""
    p = PRIMES[pname]
    S = stream(name)
    rnd = random.Random(f"{name}/{pname}")
    vecs = _named_mul(S, p, rnd) if name in ("mul", "sqr") else _named_addsub(S, p, rnd)
    bounds = site_bounds(S, p)
    seen = set()

    def tags_of(v, check=True):
        tr = {}
        regs = S.operand_map(p, v.a, v.b)
        run(S, regs, trace=tr, bounds=bounds if (check and v.canonical) else None)
        got = value([regs[f"%{i}"] for i in range(8)])
        assert got == reference(name, p, v.a, v.b), (name, pname, v)
        v.tags = frozenset(i for i, s in tr.items() if 1 in s)
        return {(i, x) for i, s in tr.items() for x in s}

    def offer(v, always=False):
        new = tags_of(v) - seen
        if v.canonical and (new or always):
            seen.update(new)
        if new and v.canonical or always:
            vecs.append(v)
        return bool(new)

    named, vecs = vecs, []
    for v in named:
        offer(v, always=True)
    all_pairs = {(i, x) for i in S.sites for x in (0, 1)}
    idle = 0
    while idle < 300 and all_pairs - seen - {(i, 1) for i in unreachable(S, p)}:      # until 300 in a row show nothing new
        a = heavy_operand(rnd, p)
        b = a if name == "sqr" else heavy_operand(rnd, p)
        idle = 0 if offer(Vector(a, b, "extreme limbs")) else idle + 1
    if name in ("mul", "sqr"):
        for k in range(8):                                  # m_k = 0
            r = steer_column(S, p, rnd, k, S.closing[k], "zero") if not (name == "sqr" and k == 0) else (1 << 16, 1 << 16)
            assert r is not None, (name, pname, "m_k = 0", k)
            offer(Vector(r[0], r[1], f"m_{k} = 0"), always=True)
        for (i, x) in sorted(all_pairs - seen):
            if x == 0 or i in unreachable(S, p) or S.col.get(i) is None or S.col[i] > 7 or S.prog[i][0] != "v_mad_u64_u32":
                continue
            r = steer_column(S, p, rnd, S.col[i], i, "carry")
            if r is not None:
                offer(Vector(r[0], r[1], f"carry out of the MAC at {i} (column {S.col[i]})"))
    return tuple(vecs)


def coverage(name, pname, vectors=None):
    """{site: set of VCC values} over the canonical vectors."""
    p = PRIMES[pname]
    S = stream(name)
    tr = {i: set() for i in S.sites}
    for v in (directed(name, pname) if vectors is None else vectors):
        if v.canonical:
            run(S, S.operand_map(p, v.a, v.b), trace=tr)
    return tr


def mutants(name):
    """{consumer index: producing site}: every instruction that reads VCC, to be executed in its non-carry form."""
    return dict(stream(name).consumers)


def main():
    for pname in PRIMES:
        for name in STREAMS:
            S = stream(name)
            cov = coverage(name, pname)
            un = unreachable(S, PRIMES[pname])
            missing = [i for i in S.sites if len(cov[i]) < 2 and i not in un]
            both = [i for i in S.sites if len(cov[i]) == 2]
            print(f"{pname} {name}: {len(S.prog)} instructions, {len(S.sites)} carry sites, {len(directed(name, pname))} vectors: "
                  f"{len(both)} toggled, {len(un)} unreachable, {len(missing)} open {missing}")


if __name__ == "__main__":
    main()
