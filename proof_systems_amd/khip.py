"""ctypes binding of include/kimchi_hip.h (numpy uint64 limb arrays in, numpy out).

The header is the only description of the ABI: at import it is parsed (_abi.py) and every function the library exports gets its
argtypes and restype from its prototype, the caller-filled structs become ctypes Structures and every KH_* constant a module
attribute (`_ctype` below is the whole mapping).  A new entry point needs its prototype in the header and its wrapper here.

No fallback: if libkimchi_hip.so has not been built this module raises ImportError, and
every call raises KhError when the library reports a failure (e.g. no GPU).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KH_LIB") or os.path.join(_HERE, "libkimchi_hip.so")      # KH_LIB: another build of the library (same-box A/B of two builds)

if not os.path.exists(LIB_PATH):
    raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(hipcc --offload-arch=gfx950); there is no CPU fallback")
try:
    _PROTOTYPES, _STRUCTS, _CONSTANTS = _abi.parse()
except OSError as e:
    raise ImportError(f"{_abi.HEADER} is missing: the binding is declared from it ({e})") from e

_lib = C.CDLL(LIB_PATH)

SYMBOLS = list(_PROTOTYPES)          # every function include/kimchi_hip.h declares

def __getattr__(name: str):
    """Every constant of the header is an attribute of this module under its name without the KH_ prefix (khip.TOK_CONST, khip.SCAN_MUL, khip.E_BLINDERS,
    khip.MSM_SLOTS, khip.GATE_ZERO, khip.GATE_LOOKUP, ...).  The ones this module uses itself, and the short names, are spelled out below."""
    try:
        return _CONSTANTS["KH_" + name]
    except KeyError:
        raise AttributeError(f"module {__name__!r} has no attribute {name!r}") from None


VESTA, PALLAS = _CONSTANTS["KH_CURVE_VESTA"], _CONSTANTS["KH_CURVE_PALLAS"]
FP, FQ = _CONSTANTS["KH_FIELD_FP"], _CONSTANTS["KH_FIELD_FQ"]
BASIS_G = _CONSTANTS["KH_BASIS_G"]
PROVE_CHECK = _CONSTANTS["KH_PROVE_CHECK"]
WITNESS_GATES, WITNESS_WIRES, WITNESS_LOOKUPS = _CONSTANTS["KH_WITNESS_GATES"], _CONSTANTS["KH_WITNESS_WIRES"], _CONSTANTS["KH_WITNESS_LOOKUPS"]


def _sections(prefix: str):
    """{"w_comm": KH_PROOF_W_COMM, ...}: the constants of one prefix, in the header's order"""
    return {name[len(prefix):].lower(): value for name, value in _CONSTANTS.items() if name.startswith(prefix)}


_BY_VALUE = {"int": C.c_int, "unsigned": C.c_uint, "size_t": C.c_size_t, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "uint8_t": C.c_uint8,
             "double": C.c_double, "float": C.c_float}
_STRUCTURES = {}                     # kh_lookup_table_t -> LookupTableC, ...


def _ctype(ctype: str, name: str = ""):
    """The ctypes type of a C type of the header.  By value: the matching ctypes (void: None).  A device address (a parameter named *_dev), an opaque
    handle (kh_srs_t *) and void * are c_void_p -- callers pass integers --, char * is c_char_p; one more level of either is a POINTER to that.  Every
    other T * (arrays arrive as T *) is POINTER(T), so a numpy array of the wrong element type is refused before the call."""
    toks = ctype.replace("*", " * ").split()
    depth = toks.count("*")
    base, = [t for t in toks if t not in ("const", "*")]
    if depth and (name.endswith("_dev") or base == "void" or (base.startswith("kh_") and base not in _STRUCTURES)):
        t, depth = C.c_void_p, depth - 1
    elif depth and base == "char":
        t, depth = C.c_char_p, depth - 1
    else:
        t = None if base == "void" else _STRUCTURES.get(base) or _BY_VALUE[base]
    for _ in range(depth):
        t = C.POINTER(t)
    return t


def _structure(name: str, fields):
    """kh_lookup_table_t -> class LookupTableC(ctypes.Structure) with the typedef's fields.  A pointer field keeps its pointee type (`data` takes
    arr.ctypes.data_as(U64P)): no name is given to _ctype, its *_dev rule is for parameters."""
    members = []
    for field, ctype, dims in fields:
        t = _ctype(ctype)
        for d in reversed(dims):               # entry[3][4] -> (c_uint64 * 4) * 3
            t = t * d
        members.append((field, t))
    return type("".join(w.capitalize() for w in name[3:-2].split("_")) + "C", (C.Structure,), {"__doc__": name, "_fields_": members})


for _name, _fields in _STRUCTS.items():
    _STRUCTURES[_name] = _structure(_name, _fields)
LookupTableC, RuntimeTableCfgC = _STRUCTURES["kh_lookup_table_t"], _STRUCTURES["kh_runtime_table_cfg_t"]
WitnessReportC, WitnessLookupC = _STRUCTURES["kh_witness_report_t"], _STRUCTURES["kh_witness_lookup_t"]
SectionC, VerifyItemC, VerifyTraceC = _STRUCTURES["kh_section_t"], _STRUCTURES["kh_verify_item_t"], _STRUCTURES["kh_verify_trace_t"]

# ctypes passes an undeclared Python int as a 32-bit C int (round 6: kh_msm_submit_host, called with a bare int for its size_t n, asked hipMalloc for
# 6.6 EB), so nothing is left undeclared.  A function an older build (KH_LIB) lacks is skipped; tests/test_abi.py holds the in-tree build to all of them.
for _name, (_ret, _params) in _PROTOTYPES.items():
    _fn = getattr(_lib, _name, None)
    if _fn is not None:
        _fn.restype = _ctype(_ret)
        _fn.argtypes = [_ctype(_t, _p) for _t, _p in _params]

U64P = C.POINTER(C.c_uint64)
U8P = C.POINTER(C.c_uint8)


class KhError(RuntimeError):
    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


def _check(rc: int):
    if rc != 0:
        raise KhError(f"kimchi_hip error {rc}: {_lib.kh_last_error().decode()}", rc)


def _p64(a):
    return a.ctypes.data_as(U64P)


def _p8(a):
    return None if a is None else a.ctypes.data_as(U8P)


def _c64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a if shape is None else a.reshape(shape)


def raw():
    return _lib


def device_count() -> int:
    return _lib.kh_device_count()


def init(device: int = -1, timers: bool = True):
    """kh_init; timers: switch the per-phase HIP events behind last_timings() on for the device's shared context (the library's default is off: they cost
    the stream a few microseconds each; this binding's users are tools and tests that read them)"""
    _check(_lib.kh_init(device))
    if timers:
        _check(_lib.kh_set_phase_timers(1))


def set_device(device: int):
    """This THREAD's current device from now on (kh_set_device); handles keep running on the device they were created on."""
    _check(_lib.kh_set_device(device))


def get_device() -> int:
    return _lib.kh_get_device()


def trim():
    _check(_lib.kh_trim())


def set_phase_timers(on: bool):
    """per-phase HIP events behind last_timings() on the calling thread's current context (kh_set_phase_timers)"""
    _check(_lib.kh_set_phase_timers(int(bool(on))))


def set_sort_staging(entries: int = 28672, max_passes: int = 2):
    """The wide path's staged scatter (kh_msm_set_sort_staging): entries per pass in LDS (0 = direct scatter) and the most passes a partition may take."""
    _check(_lib.kh_msm_set_sort_staging(entries, max_passes))


def glv_split(scalar_field: int, scalars):
    """kh_debug_glv_split: for canonical scalars (n, 4) u64 -> (|k1|, |k2|) as Python ints and their signs, k = k1 + k2 lambda (mod r)."""
    a = np.ascontiguousarray(scalars, dtype=np.uint64)
    n = a.shape[0]
    out = np.zeros((n, 10), np.uint32)
    _check(_lib.kh_debug_glv_split(scalar_field, _p64(a), n, out.ctypes.data_as(C.POINTER(C.c_uint32))))
    res = []
    for row in out:
        m1 = sum(int(row[t]) << (32 * t) for t in range(4)); m2 = sum(int(row[4 + t]) << (32 * t) for t in range(4))
        res.append((-m1 if row[8] else m1, -m2 if row[9] else m2))
    return res


def set_wide_min_n(n: int):
    """Bases of >= n points created from now on get the 20-bit-window table set, single MSMs of >= n scalars take it (kh_msm_set_wide_min_n; 0 = never)."""
    _check(_lib.kh_msm_set_wide_min_n(n))


POINT_BYTES = _CONSTANTS["KH_POINT_BYTES"]
POINT_OK, POINT_INFINITY, POINT_BAD_FLAGS, POINT_NOT_CANONICAL, POINT_NOT_ON_CURVE = (_CONSTANTS["KH_POINT_" + _n] for _n in (
    "OK", "INFINITY", "BAD_FLAGS", "NOT_CANONICAL", "NOT_ON_CURVE"))


def _records(b):
    """compressed points as a C-contiguous (n, 33) uint8 array: from bytes, a list of 33-byte strings or an array"""
    if isinstance(b, (bytes, bytearray, memoryview)):
        b = np.frombuffer(bytes(b), dtype=np.uint8)
    elif isinstance(b, (list, tuple)):
        b = np.frombuffer(b"".join(bytes(r) for r in b), dtype=np.uint8)
    return np.ascontiguousarray(b, dtype=np.uint8).reshape(-1, POINT_BYTES)


def points_compress(curve: int, xy, inf=None):
    """kh_points_compress: (n, 8) affine Montgomery limbs (+ infinity bytes) -> (n, 33) compressed records, encoded on the device"""
    xy = _c64(xy, (-1, 8))
    if inf is not None:
        inf = np.ascontiguousarray(inf, dtype=np.uint8).reshape(-1)
    out = np.zeros((xy.shape[0], POINT_BYTES), dtype=np.uint8)
    _check(_lib.kh_points_compress(curve, _p64(xy), _p8(inf), xy.shape[0], _p8(out)))
    return out


def points_decompress_raw(curve: int, records):
    """kh_points_decompress without raising: (return code, xy (n, 8), inf (n,), status (n,), first bad index or None)"""
    rec = _records(records)
    n = rec.shape[0]
    xy = np.zeros((n, 8), dtype=np.uint64); inf = np.zeros(n, dtype=np.uint8); status = np.zeros(n, dtype=np.uint8)
    first = C.c_size_t(n)
    rc = _lib.kh_points_decompress(curve, _p8(rec), n, _p64(xy), _p8(inf), _p8(status), C.byref(first))
    return rc, xy, inf, status, (first.value if first.value < n else None)


def points_decompress(curve: int, records):
    """kh_points_decompress: (n, 33) records -> (xy (n, 8), inf (n,)); a malformed record raises KhError naming the first one"""
    rc, xy, inf, _status, _first = points_decompress_raw(curve, records)
    _check(rc)
    return xy, inf


def points_compress_dev(curve: int, xy, inf, n: int, out):
    """kh_points_compress_dev: n points in a DevBuf (64 bytes each; inf: a DevBuf of n bytes or None) -> n x 33 bytes in `out`; a queued vector step"""
    _check(_lib.kh_points_compress_dev(curve, _ptr(xy), _ptr(inf), n, _ptr(out)))


def points_decompress_dev(curve: int, records, n: int, out_xy, out_inf, status=None, flags=None, bit: int = 0):
    """kh_points_decompress_dev: n x 33 bytes in a DevBuf -> out_xy (n x 64 bytes), out_inf and (nullable) status (n bytes each); the flag bit is raised
    by any record that is neither a point nor the point at infinity; a queued vector step"""
    _check(_lib.kh_points_decompress_dev(curve, _ptr(records), n, _ptr(out_xy), _ptr(out_inf), _ptr(status), _ptr(flags), bit))


class Srs:
    """Device-resident SRS bases (the g half of ipa::SRS<G>, poly-commitment/src/ipa.rs:53-75)."""

    def __init__(self, curve: int, g_xy=None, depth: int = 0, start: int = 0):
        """Upload the bases g_xy, or (g_xy is None) run SRS::create on the device for g[start, start+depth)."""
        self.curve = curve
        self._h = C.c_void_p()
        if g_xy is None:
            self.n = depth
            _check(_lib.kh_srs_create_device_range(curve, start, depth, C.byref(self._h)))
        else:
            g = _c64(g_xy, (-1, 8))
            self.n = g.shape[0]
            _check(_lib.kh_srs_create(curve, _p64(g), self.n, C.byref(self._h)))

    @classmethod
    def create(cls, curve: int, depth: int, start: int = 0):
        """SRS::create(depth) (ipa.rs:751-778) on the device; start > 0 gives the slice g[start, start+depth)."""
        return cls(curve, None, depth, start)

    @classmethod
    def _adopt(cls, curve: int, handle):
        self = cls.__new__(cls)
        self.curve, self._h, self.n = curve, handle, int(_lib.kh_srs_size(handle))
        return self

    @classmethod
    def from_compressed(cls, curve: int, g_bytes, h_bytes=None):
        """kh_srs_create_compressed: the bases from (n, 33) compressed records, decoded on the device straight into the handle's tables; h_bytes: the
        blinding base as one record.  A record that is not a point (an infinity record too) raises KhError naming its index."""
        g = _records(g_bytes)
        h = _records(h_bytes) if h_bytes is not None else None
        handle = C.c_void_p()
        _check(_lib.kh_srs_create_compressed(curve, _p8(g), g.shape[0], _p8(h), C.byref(handle)))
        return cls._adopt(curve, handle)

    @classmethod
    def from_file_bytes(cls, curve: int, data: bytes, limit: int = 0):
        """kh_srs_create_from_file: the contents of an srs/*.srs file; limit (0 = all) keeps the first `limit` points, h is the file's last record."""
        buf = np.frombuffer(bytes(data) + b"\0", dtype=np.uint8)               # (never a null pointer, whatever the length)
        handle = C.c_void_p()
        _check(_lib.kh_srs_create_from_file(curve, buf.ctypes.data_as(U8P), buf.size - 1, limit, C.byref(handle)))
        return cls._adopt(curve, handle)

    def to_file_bytes(self) -> bytes:
        """kh_srs_write_file: the handle's bases and blinding base in the layout of the srs/*.srs files"""
        out = np.zeros(int(_lib.kh_srs_file_bytes(self.n)), dtype=np.uint8)
        _check(_lib.kh_srs_write_file(self._h, _p8(out), out.size))
        return out.tobytes()

    def get_g(self, offset: int = 0, count: int = None):
        count = self.n - offset if count is None else count
        out = np.zeros((count, 8), dtype=np.uint64)
        _check(_lib.kh_srs_get_g(self._h, offset, count, _p64(out)))
        return out

    def get_g_compressed(self, offset: int = 0, count: int = None):
        """kh_srs_get_g_compressed: g[offset, offset + count) as (count, 33) compressed records, encoded on the device"""
        count = self.n - offset if count is None else count
        out = np.zeros((count, POINT_BYTES), dtype=np.uint8)
        _check(_lib.kh_srs_get_g_compressed(self._h, offset, count, _p8(out)))
        return out

    def debug_rebase_points(self, coef):
        """kh_debug_rebase_points: the folded basis sum_q coef[q] g[q N + i] (csrc/rebase.hip), affine; raises if an output was the identity."""
        c = _c64(coef, (-1, 4))
        N = self.n // c.shape[0]
        out = np.zeros((N, 8), dtype=np.uint64); fail = C.c_uint32(0)
        _check(_lib.kh_debug_rebase_points(self._h, _p64(c), c.shape[0], _p64(out), C.byref(fail)))
        if fail.value:
            raise KhError("rebase: an output is the point at infinity")
        return out

    def has_wide_tables(self) -> bool:
        return bool(_lib.kh_srs_has_wide_tables(self._h))

    def set_wide_tables(self, on: bool):
        """Build (True) or give back (False) the optional 20-bit-window table set of this handle (kh_srs_set_wide_tables)."""
        _check(_lib.kh_srs_set_wide_tables(self._h, int(on)))

    def close(self):
        if self._h:
            _lib.kh_srs_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_lagrange(self, log2_domain: int, xy, inf=None, chunk: int = 0):
        xy = _c64(xy, (-1, 8))
        if inf is not None:
            inf = np.ascontiguousarray(inf, dtype=np.uint8)
        _check(_lib.kh_srs_set_lagrange(self._h, log2_domain, chunk, _p64(xy), _p8(inf), xy.shape[0]))

    def compute_lagrange(self, log2_domain: int):
        _check(_lib.kh_srs_compute_lagrange(self._h, log2_domain))

    def get_lagrange(self, log2_domain: int, chunk: int = 0):
        n = 1 << log2_domain
        xy = np.zeros((n, 8), dtype=np.uint64)
        inf = np.zeros(n, dtype=np.uint8)
        _check(_lib.kh_srs_get_lagrange(self._h, log2_domain, chunk, _p64(xy), _p8(inf)))
        return xy, inf

    def lagrange_chunks(self, log2_domain: int) -> int:
        return _lib.kh_srs_lagrange_chunks(self._h, log2_domain)

    # ---- the SRS trait surface (poly-commitment/src/lib.rs:61-241) over the kernels
    def max_poly_size(self) -> int:
        return self.n

    def blinding_commitment(self):
        out = np.zeros(8, dtype=np.uint64)
        _check(_lib.kh_srs_get_blinding_base(self._h, _p64(out)))
        return out

    def set_blinding_base(self, h_xy):
        h = _c64(h_xy, (8,))
        _check(_lib.kh_srs_set_blinding_base(self._h, _p64(h)))

    def commit_non_hiding(self, coeffs, num_chunks: int):
        """SRS::commit_non_hiding (ipa.rs:638-683) -> (chunks x 8 limbs, inf flags)."""
        c = _c64(coeffs, (-1, 4))
        cap = max(num_chunks, -(-c.shape[0] // self.n), 1)
        out = np.zeros((cap, 8), dtype=np.uint64)
        inf = np.zeros(cap, dtype=np.uint8)
        cnt = C.c_size_t(0)
        _check(_lib.kh_commit_non_hiding(self._h, _p64(c), c.shape[0], num_chunks, _p64(out), _p8(inf), C.byref(cnt)))
        return out[:cnt.value], inf[:cnt.value]

    def commit_evaluations_non_hiding(self, log2_domain: int, evals):
        """SRS::commit_evaluations_non_hiding (ipa.rs:706-728)."""
        e = _c64(evals, (-1, 4))
        cap = max(1, self.lagrange_chunks(log2_domain))
        out = np.zeros((cap, 8), dtype=np.uint64)
        inf = np.zeros(cap, dtype=np.uint8)
        cnt = C.c_size_t(0)
        _check(_lib.kh_commit_evaluations_non_hiding(self._h, log2_domain, _p64(e), e.shape[0], _p64(out), _p8(inf), C.byref(cnt)))
        return out[:cnt.value], inf[:cnt.value]

    def mask_custom(self, com_xy, com_inf, blinders):
        """SRS::mask_custom (ipa.rs:605-622); raises KhError(code=E_BLINDERS) on BlindersDontMatch."""
        com = _c64(com_xy, (-1, 8)); bl = _c64(blinders, (-1, 4))
        ci = np.ascontiguousarray(com_inf, dtype=np.uint8)
        out = np.zeros((com.shape[0], 8), dtype=np.uint64)
        inf = np.zeros(com.shape[0], dtype=np.uint8)
        _check(_lib.kh_mask_custom(self._h, _p64(com), _p8(ci), com.shape[0], _p64(bl), bl.shape[0], _p64(out), _p8(inf)))
        return out, inf

    def commit_custom(self, coeffs, num_chunks: int, blinders):
        """SRS::commit_custom (ipa.rs:686-693) = mask_custom(commit_non_hiding(..), blinders)."""
        com, inf = self.commit_non_hiding(coeffs, num_chunks)
        return self.mask_custom(com, inf, blinders)

    def msm(self, scalars, basis: int = BASIS_G, chunk: int = 0, offset: int = 0, mont: bool = True):
        sc = _c64(scalars, (-1, 4))
        out = np.zeros(8, dtype=np.uint64)
        inf = np.zeros(1, dtype=np.uint8)
        _check(_lib.kh_msm(self._h, basis, chunk, offset, _p64(sc), sc.shape[0], int(mont), _p64(out), _p8(inf)))
        return out, bool(inf[0])

    def msm_batch(self, scalars, basis: int = BASIS_G, chunk: int = 0, offset: int = 0, mont: bool = True):
        sc = _c64(scalars)
        assert sc.ndim == 3 and sc.shape[2] == 4
        k, n = sc.shape[0], sc.shape[1]
        out = np.zeros((k, 8), dtype=np.uint64)
        inf = np.zeros(k, dtype=np.uint8)
        _check(_lib.kh_msm_batch(self._h, basis, chunk, offset, _p64(sc), n, k, int(mont), _p64(out), _p8(inf)))
        return out, inf

    def msm_submit(self, scalars_dev: int, n: int, k: int, basis: int = BASIS_G, chunk: int = 0, offset: int = 0, mont: bool = True):
        """Enqueue k MSMs (device-resident scalars) on a free pipeline slot; returns a ticket for msm_wait."""
        t = C.c_uint64(0)
        _check(_lib.kh_msm_submit(self._h, basis, chunk, offset, C.c_void_p(scalars_dev), n, k, int(mont), C.byref(t)))
        return (t.value, k)

    def msm_submit_host(self, scalars, k: int = 1, basis: int = BASIS_G, chunk: int = 0, offset: int = 0, mont: bool = True):
        """kh_msm_submit_host: the same pipeline from HOST scalars (k x n x 4 limbs); the buffer is the caller's again when this returns."""
        sc = _c64(scalars, (k, -1, 4))
        t = C.c_uint64(0)
        _check(_lib.kh_msm_submit_host(self._h, basis, chunk, offset, _p64(sc), sc.shape[1], k, int(mont), C.byref(t)))
        return (t.value, k)

    @staticmethod
    def msm_wait(ticket):
        t, k = ticket
        out = np.zeros((k, 8), dtype=np.uint64)
        inf = np.zeros(k, dtype=np.uint8)
        _check(_lib.kh_msm_wait(t, _p64(out), _p8(inf)))
        return out, inf

    def msm_batch_dev(self, scalars_dev: int, n: int, k: int, basis: int = BASIS_G, chunk: int = 0, offset: int = 0, mont: bool = True):
        out = np.zeros((k, 8), dtype=np.uint64)
        inf = np.zeros(k, dtype=np.uint8)
        _check(_lib.kh_msm_batch_dev(self._h, basis, chunk, offset, C.c_void_p(scalars_dev), n, k, int(mont), _p64(out), _p8(inf)))
        return out, inf


def msm_sharded(shards, scalars, mont: bool = True):
    """kh_msm_sharded: ONE MSM over a basis sharded by point range over the Srs handles `shards` (each on its own device): the slices
    of the host scalars go to their shards' devices concurrently, the partial sums are folded on the host."""
    sc = _c64(scalars, (-1, 4))
    hs = (C.c_void_p * len(shards))(*[s._h for s in shards])
    out = np.zeros(8, dtype=np.uint64); inf = np.zeros(1, dtype=np.uint8)
    _check(_lib.kh_msm_sharded(hs, len(shards), _p64(sc), sc.shape[0], int(mont), _p64(out), _p8(inf)))
    return out, bool(inf[0])


def msm_sharded_dev(shards, bufs, counts, mont: bool = True):
    """kh_msm_sharded_dev: bufs[r] = DevBuf on shard r's device holding its counts[r] scalars."""
    hs = (C.c_void_p * len(shards))(*[s._h for s in shards])
    ps = (C.c_void_p * len(shards))(*[C.c_void_p(b.ptr) for b in bufs])
    cs = (C.c_size_t * len(shards))(*counts)
    out = np.zeros(8, dtype=np.uint64); inf = np.zeros(1, dtype=np.uint8)
    _check(_lib.kh_msm_sharded_dev(hs, len(shards), ps, cs, int(mont), _p64(out), _p8(inf)))
    return out, bool(inf[0])


def srs_generate(curve: int, start: int, count: int, threads: int = 0):
    """SRS::create(depth).g[start:start+count] (host-side hash-to-curve, ipa.rs:751-778)."""
    out = np.empty((count, 8), dtype=np.uint64)
    _check(_lib.kh_srs_generate(curve, start, count, _p64(out), threads))
    return out


def srs_h(curve: int):
    out = np.empty(8, dtype=np.uint64)
    _check(_lib.kh_srs_h(curve, _p64(out)))
    return out


def msm_points(curve: int, xy, scalars, inf=None, mont: bool = True):
    xy = _c64(xy, (-1, 8))
    sc = _c64(scalars, (-1, 4))
    n = min(xy.shape[0], sc.shape[0])
    if inf is not None:
        inf = np.ascontiguousarray(inf, dtype=np.uint8)
    out = np.zeros(8, dtype=np.uint64)
    oinf = np.zeros(1, dtype=np.uint8)
    _check(_lib.kh_msm_points(curve, _p64(xy), _p8(inf), _p64(sc), n, int(mont), _p64(out), _p8(oinf)))
    return out, bool(oinf[0])


def msm_points_batch(curve: int, xy, scalars, inf=None, mont: bool = True):
    """k independent MSMs: xy (k, n, 8), scalars (k, n, 4), inf (k, n) or None."""
    xy = _c64(xy); sc = _c64(scalars)
    assert xy.ndim == 3 and sc.ndim == 3 and xy.shape[:2] == sc.shape[:2]
    k, n = xy.shape[0], xy.shape[1]
    if inf is not None:
        inf = np.ascontiguousarray(inf, dtype=np.uint8)
    out = np.zeros((k, 8), dtype=np.uint64)
    oinf = np.zeros(k, dtype=np.uint8)
    _check(_lib.kh_msm_points_batch(curve, _p64(xy), _p8(inf), _p64(sc), n, k, int(mont), _p64(out), _p8(oinf)))
    return out, oinf


def counter(name: str) -> int:
    """Process-wide event counter of the library (kh_counter): spread_retry, fused_retry, rebase_launch, rebase_switch, rebase_abandon, rebased_rounds, lookup_sorted_dev,
    ipa_concurrent, ipa_waited, table_staged_words, point_codec_launches, point_codec_encode_launches."""
    return int(_lib.kh_counter(name.encode()))


def set_ntt_max_logr(v: int):
    """Largest sub-transform of an NTT pass = 2^v points (kh_ntt_set_max_logr: 4..10, 0 = default); same results under every setting."""
    _check(_lib.kh_ntt_set_max_logr(v))


def ntt(field: int, data, log2_n: int, inverse: bool = False, in_place: bool = False):
    """in_place: transform `data` itself (a C-contiguous uint64 array) -- what ark-poly's ifft_in_place does to the caller's Vec"""
    if in_place:
        assert data.dtype == np.uint64 and data.flags["C_CONTIGUOUS"]
        d = data.reshape(-1, 1 << log2_n, 4)
    else:
        d = np.array(data, dtype=np.uint64, copy=True).reshape(-1, 1 << log2_n, 4)
    _check(_lib.kh_ntt(field, _p64(d), log2_n, int(inverse), d.shape[0]))
    return d


def lde(field: int, coeffs, log2_n: int, log2_blowup: int, out=None):
    c = _c64(coeffs, (-1, 1 << log2_n, 4))
    if out is None:
        out = np.zeros((c.shape[0], 1 << (log2_n + log2_blowup), 4), dtype=np.uint64)
    assert out.dtype == np.uint64 and out.flags["C_CONTIGUOUS"] and out.size == c.shape[0] * (4 << (log2_n + log2_blowup))
    _check(_lib.kh_lde(field, _p64(c), log2_n, log2_blowup, _p64(out), c.shape[0]))
    return out


class DevBuf:
    """A raw HBM allocation (kh_dev_alloc) for the device-resident entry points."""

    def __init__(self, nbytes: int):
        self.nbytes = nbytes
        p = C.c_void_p()
        _check(_lib.kh_dev_alloc(C.byref(p), nbytes))
        self.ptr = p.value

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        _check(_lib.kh_dev_upload(C.c_void_p(self.ptr), arr.ctypes.data_as(C.c_void_p), arr.nbytes))
        return self

    def download(self, shape, dtype=np.uint64):
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        _check(_lib.kh_dev_download(out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr), out.nbytes))
        return out

    def free(self):
        if self.ptr:
            _check(_lib.kh_dev_free(C.c_void_p(self.ptr)))
            self.ptr = None

    def view(self, offset_bytes: int):
        """A non-owning alias of this allocation starting `offset_bytes` in (anything with a .ptr is accepted as a column)."""
        return DevView(self.ptr + offset_bytes)

    def upload_at(self, offset_bytes: int, arr):
        arr = np.ascontiguousarray(arr)
        assert offset_bytes + arr.nbytes <= self.nbytes
        _check(_lib.kh_dev_upload(C.c_void_p(self.ptr + offset_bytes), arr.ctypes.data_as(C.c_void_p), arr.nbytes))

    def upload_2d(self, offset_bytes: int, dst_pitch: int, arr2d):
        """arr2d: (rows, ...) C-contiguous; row r goes to offset_bytes + r * dst_pitch."""
        a = np.ascontiguousarray(arr2d)
        rows = a.shape[0]; width = a.nbytes // rows
        assert offset_bytes + (rows - 1) * dst_pitch + width <= self.nbytes
        _check(_lib.kh_dev_upload_2d(C.c_void_p(self.ptr + offset_bytes), dst_pitch, a.ctypes.data_as(C.c_void_p), width, width, rows))

    def download_at(self, offset_bytes: int, shape, dtype=np.uint64):
        out = np.empty(shape, dtype=dtype)
        assert offset_bytes + out.nbytes <= self.nbytes
        _check(_lib.kh_dev_download(out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr + offset_bytes), out.nbytes))
        return out

    def zero(self):
        _check(_lib.kh_dev_memset_zero(C.c_void_p(self.ptr), self.nbytes))
        return self

    def fill_elements(self, offset_elems: int, value, count: int):
        """count 32-byte records from element offset_elems on set to `value` (4 limbs), queued on the main stream (kh_dev_fill_elements)"""
        assert (offset_elems + count) * 32 <= self.nbytes
        _check(_lib.kh_dev_fill_elements(C.c_void_p(self.ptr + 32 * offset_elems), _p64(_c64(value, (4,))), count))
        return self


class DevView:
    def __init__(self, ptr: int):
        self.ptr = ptr

    def view(self, offset_bytes: int):
        return DevView(self.ptr + offset_bytes)


def dev_copy(dst_ptr: int, src_ptr: int, nbytes: int):
    _check(_lib.kh_dev_copy(C.c_void_p(dst_ptr), C.c_void_p(src_ptr), nbytes))


def dev_memset_zero(dst_ptr: int, nbytes: int):
    _check(_lib.kh_dev_memset_zero(C.c_void_p(dst_ptr), nbytes))


def group_map_to_group(curve: int, t):
    out = np.zeros(8, dtype=np.uint64)
    _check(_lib.kh_group_map_to_group(curve, _p64(_c64(t, (4,))), _p64(out)))
    return out


def ntt_dev(field: int, buf: DevBuf, log2_n: int, inverse: bool, batch: int):
    _check(_lib.kh_ntt_dev(field, C.c_void_p(buf.ptr), log2_n, int(inverse), batch))


def coset_ntt_dev(field: int, src: DevBuf, log2_n: int, shift, dst: DevBuf, batch: int):
    _check(_lib.kh_coset_ntt_dev(field, C.c_void_p(src.ptr), log2_n, _p64(_c64(shift, (4,))), C.c_void_p(dst.ptr), batch))


def lde_dev(field: int, src: DevBuf, log2_n: int, log2_blowup: int, dst: DevBuf, batch: int):
    _check(_lib.kh_lde_dev(field, C.c_void_p(src.ptr), log2_n, log2_blowup, C.c_void_p(dst.ptr), batch))


def points_sum(curve: int, xy, inf=None):
    """Host-side sum of a few affine points (fold of per-GPU partial MSM results)."""
    xy = _c64(xy, (-1, 8))
    if inf is not None:
        inf = np.ascontiguousarray(inf, dtype=np.uint8)
    out = np.zeros(8, dtype=np.uint64); oinf = np.zeros(1, dtype=np.uint8)
    _check(_lib.kh_points_sum(curve, _p64(xy), _p8(inf), xy.shape[0], _p64(out), _p8(oinf)))
    return out, bool(oinf[0])


def points_add(curve: int, a_xy, a_inf, b_xy, b_inf):
    """Pairwise host sums a_j + b_j of affine points (the second half of a masking whose blinding points were computed ahead)."""
    a_xy = _c64(a_xy, (-1, 8)); b_xy = _c64(b_xy, (-1, 8))
    n = a_xy.shape[0]
    a_inf = None if a_inf is None else np.ascontiguousarray(a_inf, dtype=np.uint8)
    b_inf = None if b_inf is None else np.ascontiguousarray(b_inf, dtype=np.uint8)
    out = np.zeros((n, 8), dtype=np.uint64); oinf = np.zeros(n, dtype=np.uint8)
    _check(_lib.kh_points_add(curve, _p64(a_xy), _p8(a_inf), _p64(b_xy), _p8(b_inf), n, _p64(out), _p8(oinf)))
    return out, oinf


def ipa_fold_scalars(field: int, lo, hi, u):
    lo = _c64(lo, (-1, 4)); hi = _c64(hi, (-1, 4)); u = _c64(u, (4,))
    out = np.zeros_like(lo)
    _check(_lib.kh_ipa_fold_scalars(field, _p64(lo), _p64(hi), _p64(u), lo.shape[0], _p64(out)))
    return out


def inner_product(field: int, a, b):
    a = _c64(a, (-1, 4)); b = _c64(b, (-1, 4))
    out = np.zeros(4, dtype=np.uint64)
    _check(_lib.kh_inner_product(field, _p64(a), _p64(b), a.shape[0], _p64(out)))
    return out


def ipa_fold_points(curve: int, g_lo, g_hi, u):
    g_lo = _c64(g_lo, (-1, 8)); g_hi = _c64(g_hi, (-1, 8)); u = _c64(u, (4,))
    out = np.zeros_like(g_lo); inf = np.zeros(g_lo.shape[0], dtype=np.uint8)
    _check(_lib.kh_ipa_fold_points(curve, _p64(g_lo), _p64(g_hi), _p64(u), g_lo.shape[0], _p64(out), _p8(inf)))
    return out, inf


def ipa_fold_points_endo(curve: int, g_lo, g_hi, chal: int):
    """combine_one_endo: chal is the 128-bit prechallenge as a Python int."""
    g_lo = _c64(g_lo, (-1, 8)); g_hi = _c64(g_hi, (-1, 8))
    c = np.array([chal & (2**64 - 1), (chal >> 64) & (2**64 - 1)], dtype=np.uint64)
    out = np.zeros_like(g_lo); inf = np.zeros(g_lo.shape[0], dtype=np.uint8)
    _check(_lib.kh_ipa_fold_points_endo(curve, _p64(g_lo), _p64(g_hi), _p64(c), g_lo.shape[0], _p64(out), _p8(inf)))
    return out, inf


def field_scan_dev(field: int, op: int, buf, n: int, reverse: bool = False, offset: int = 0):
    """In-place inclusive scan of n elements starting `offset` elements into the DevBuf."""
    _check(_lib.kh_field_scan_dev(field, op, int(reverse), C.c_void_p(buf.ptr + 32 * offset), n))


def batch_inversion_dev(field: int, buf, n: int, offset: int = 0):
    _check(_lib.kh_batch_inversion_dev(field, C.c_void_p(buf.ptr + 32 * offset), n))


def divide_by_linear_dev(field: int, f, length: int, a, q):
    rem = np.zeros(4, dtype=np.uint64)
    _check(_lib.kh_divide_by_linear_dev(field, C.c_void_p(f.ptr), length, _p64(_c64(a, (4,))), C.c_void_p(q.ptr if q is not None else 0), _p64(rem)))
    return rem


def divide_by_linear_async_dev(field: int, f, length: int, a, q, rem_dev):
    """kh_divide_by_linear_async_dev: quotient into q, remainder into the DevBuf rem_dev (4 limbs); nothing waits."""
    _check(_lib.kh_divide_by_linear_async_dev(field, C.c_void_p(f.ptr), length, _p64(_c64(a, (4,))), C.c_void_p(q.ptr if q is not None else 0),
                                              C.c_void_p(rem_dev.ptr if rem_dev is not None else 0)))


def check_equal_dev(v, n: int, expect, flags, bit: int, offset: int = 0):
    """kh_check_equal_dev: flags (a DevBuf holding a uint32) |= 1 << bit when any of the n elements at v (+ offset elements) differs from expect (None: zero)."""
    e = None if expect is None else _c64(expect, (4,))
    _check(_lib.kh_check_equal_dev(C.c_void_p(v.ptr + 32 * offset), n, _p64(e) if e is not None else None, C.c_void_p(flags.ptr), bit))


def expr_evaluations_dev(field: int, tokens, cols, col_len, constants, rows: int, out, stride: int = 1, next_shift: int = 8, accumulate: bool = False,
                         out_offset: int = 0):
    """tokens: list of (opcode, arg); cols: list of DevBuf; constants: (k, 4) Montgomery limbs; out: DevBuf receiving `rows`
    elements starting `out_offset` elements in."""
    tk = np.ascontiguousarray(np.array(tokens, dtype=np.uint32).reshape(-1, 2))
    m = len(cols)
    ptrs = (C.c_void_p * max(m, 1))(*[C.c_void_p(c.ptr) for c in cols])
    lens = (C.c_size_t * max(m, 1))(*col_len)
    cs = _c64(constants, (-1, 4))
    _check(_lib.kh_expr_evaluations_dev(field, tk.ctypes.data_as(C.POINTER(C.c_uint32)), tk.shape[0], ptrs, lens, m, _p64(cs), cs.shape[0],
                                        rows, stride, next_shift, int(accumulate), C.c_void_p(out.ptr + 32 * out_offset)))


_GATE_IDS = {}


def gate_ids():
    """{name: id} of the compiled kernels (kh_gate_evaluations_dev): the gate library's GateType names, "Generic", "Permutation"."""
    if not _GATE_IDS:
        _GATE_IDS.update({_lib.kh_gate_name(g).decode(): g for g in range(_lib.kh_gate_count())})
    return _GATE_IDS


def gate_num_constants(gate: int) -> int:
    return _lib.kh_gate_num_constants(gate)


def gate_constants(field: int, gate: int, alpha=None, endo=None, params=None):
    """kh_gate_constants: the (k, 4) constants table of a compiled gate kernel for one proof (host only)."""
    k = gate_num_constants(gate)
    out = np.zeros((k, 4), dtype=np.uint64)
    a = _c64(alpha, (4,)) if alpha is not None else None
    e = _c64(endo, (4,)) if endo is not None else None
    ps = _c64(params, (-1, 4)) if params is not None else None
    _check(_lib.kh_gate_constants(field, gate, _p64(a) if a is not None else None, _p64(e) if e is not None else None,
                                  _p64(ps) if ps is not None else None, ps.shape[0] if ps is not None else 0, _p64(out)))
    return out


def gate_evaluations_dev(field: int, gate: int, cols, col_len: int, constants, rows: int, out, stride: int = 1, next_shift: int = 8, accumulate: bool = False,
                         out_offset: int = 0):
    """kh_gate_evaluations_dev: cols = 31 DevBuf (witness 0..14, coefficients 15..29, the gate's selector); constants (k, 4) Montgomery limbs."""
    assert len(cols) == 31
    ptrs = (C.c_void_p * 31)(*[C.c_void_p(c.ptr) for c in cols])
    cs = _c64(constants, (-1, 4))
    _check(_lib.kh_gate_evaluations_dev(field, gate, ptrs, col_len, _p64(cs), cs.shape[0], rows,
                                        stride, next_shift, int(accumulate), C.c_void_p(out.ptr + 32 * out_offset)))


def lookup_sorted(table, lookup_rows: int, values, max_per_row: int):
    """kh_lookup_sorted: table (>= lookup_rows, 4) limbs, values (max_per_row, stride, 4) limbs -> (max_per_row + 1, lookup_rows + 1, 4).
    Raises ValueError(row) for a value that is not in the table."""
    t = _c64(table, (-1, 4)); v = _c64(values, (max_per_row, -1, 4))
    out = np.zeros((max_per_row + 1, lookup_rows + 1, 4), dtype=np.uint64)
    bad = C.c_size_t(0)
    rc = _lib.kh_lookup_sorted(_p64(t), lookup_rows, _p64(v), v.shape[1], max_per_row, _p64(out), C.byref(bad))
    if rc != 0 and bad.value != C.c_size_t(-1).value:
        raise ValueError(bad.value)
    _check(rc)
    return out


def lookup_sorted_dev(table, lookup_rows: int, values, value_stride: int, max_per_row: int, out, out_stride: int):
    """kh_lookup_sorted_dev: the same over device buffers (anything with a .ptr), queued on the main stream.  table: >= lookup_rows elements; values:
    max_per_row columns, value_stride elements apart; out: max_per_row + 1 columns, out_stride elements apart, of which elements 0 .. lookup_rows are
    written and nothing else.  Raises ValueError(row) for a value that is not in the table (out is then untouched)."""
    bad = C.c_size_t(0)
    rc = _lib.kh_lookup_sorted_dev(C.c_void_p(table.ptr), lookup_rows, C.c_void_p(values.ptr), value_stride, max_per_row,
                                   C.c_void_p(out.ptr), out_stride, C.byref(bad))
    if rc != 0 and bad.value != C.c_size_t(-1).value:
        raise ValueError(bad.value)
    _check(rc)


def poseidon_gate_coefficients(field: int):
    """kh_poseidon_gate_coefficients: the (11, 15, 4) coefficient rows of a Poseidon gadget (host only)."""
    out = np.zeros((11, 15, 4), dtype=np.uint64)
    _check(_lib.kh_poseidon_gate_coefficients(field, _p64(out)))
    return out


def poseidon_permute_dev(field: int, states, n: int):
    """kh_poseidon_permute_dev: n states of 3 elements at `states` (anything with a .ptr) permuted in place, queued on the main stream."""
    _check(_lib.kh_poseidon_permute_dev(field, C.c_void_p(states.ptr), n))


def poseidon_hash_dev(field: int, msgs, msg_len: int, n: int, digests, init=None):
    """kh_poseidon_hash_dev: n messages of msg_len elements at `msgs` (None when msg_len == 0) -> n digests at `digests`; init: (3, 4) limbs or None (zero)."""
    st = None if init is None else _c64(init, (3, 4))
    _check(_lib.kh_poseidon_hash_dev(field, C.c_void_p(msgs.ptr if msgs is not None else 0), msg_len, n, _p64(st) if st is not None else None,
                                     C.c_void_p(digests.ptr)))


def poseidon_gate_witness_dev(field: int, states, n: int, witness, col_stride: int, col_len: int, rows=None, row0: int = 0, row_stride: int = 12,
                              out_states=None):
    """kh_poseidon_gate_witness_dev: the witness rows of n Poseidon gadgets into the 15 columns at `witness`, instance i at row rows[i] (a sequence of
    ints) or row0 + i * row_stride; out_states (nullable, may be `states`): the n final states."""
    r = None if rows is None else np.ascontiguousarray(rows, dtype=np.uint32)
    _check(_lib.kh_poseidon_gate_witness_dev(field, C.c_void_p(states.ptr), n, r.ctypes.data_as(C.POINTER(C.c_uint32)) if r is not None else None, row0,
                                             row_stride, C.c_void_p(witness.ptr), col_stride, col_len,
                                             C.c_void_p(out_states.ptr if out_states is not None else 0)))


def poseidon_set_split_max_n(n: int = 43008):
    """kh_poseidon_set_split_max_n: up to n instances poseidon_gate_witness_dev runs its three-lanes-per-permutation kernel (0: never)"""
    _check(_lib.kh_poseidon_set_split_max_n(n))


def _rows32(rows):
    r = None if rows is None else np.ascontiguousarray(rows, dtype=np.uint32)
    return r, (r.ctypes.data_as(C.POINTER(C.c_uint32)) if r is not None else None)


def _ptr(buf):
    return C.c_void_p(buf.ptr if buf is not None else 0)


def complete_add_witness_dev(field: int, p1, p2, n: int, witness, col_stride: int, col_len: int, rows=None, row0: int = 0, row_stride: int = 1, out=None):
    """kh_complete_add_witness_dev: the CompleteAdd row of n pairs of affine points (n x 8 limbs at p1, p2) into the 15 columns at `witness`, instance i at
    row rows[i] or row0 + i * row_stride; out (nullable): the n sums."""
    _r, rp = _rows32(rows)
    _check(_lib.kh_complete_add_witness_dev(field, _ptr(p1), _ptr(p2), n, rp, row0, row_stride, _ptr(witness), col_stride, col_len, _ptr(out)))


def varbasemul_witness_dev(field: int, base, acc0, scalars, num_bits: int, n: int, witness, col_stride: int, col_len: int, rows=None, row0: int = 0,
                           row_stride: int = None, out_acc=None, out_n=None, flags=None, bit: int = 0):
    """kh_varbasemul_witness_dev: the 2 * num_bits / 5 VarBaseMul rows of n scalar multiplications (base, acc0: n x 8 limbs; scalars: n x 4 canonical
    limbs, bits num_bits - 1 .. 0); out_acc / out_n (nullable): the final accumulators / n; flags (a DevBuf holding a zeroed uint32) gets bit `bit` set
    when an instance met a zero denominator."""
    _r, rp = _rows32(rows)
    _check(_lib.kh_varbasemul_witness_dev(field, _ptr(base), _ptr(acc0), _ptr(scalars), num_bits, n, rp, row0,
                                          2 * num_bits // 5 if row_stride is None else row_stride, _ptr(witness), col_stride, col_len, _ptr(out_acc),
                                          _ptr(out_n), _ptr(flags), bit))


def endomul_witness_dev(field: int, endo, base, acc0, chals, num_bits: int, n: int, witness, col_stride: int, col_len: int, rows=None, row0: int = 0,
                        row_stride: int = None, out_acc=None, out_n=None, flags=None, bit: int = 0):
    """kh_endomul_witness_dev: the num_bits / 4 EndoMul rows + the closing row of n endo-scaled multiplications (endo: 4 Montgomery limbs, endos(curve)[0]
    of the curve whose base field is `field`; chals: n x 2 canonical limbs); outputs and flags as varbasemul_witness_dev."""
    _r, rp = _rows32(rows)
    _check(_lib.kh_endomul_witness_dev(field, _p64(_c64(endo, (4,))), _ptr(base), _ptr(acc0), _ptr(chals), num_bits, n, rp, row0,
                                       num_bits // 4 + 1 if row_stride is None else row_stride, _ptr(witness), col_stride, col_len, _ptr(out_acc),
                                       _ptr(out_n), _ptr(flags), bit))


def curve_witness_set_slice_elements(elements: int = 0):
    """kh_curve_witness_set_slice_elements: the batch-inversion length that bounds a slice of varbasemul_witness_dev / endomul_witness_dev (0: the default, 2^22)"""
    _check(_lib.kh_curve_witness_set_slice_elements(elements))


def endomul_scalar_witness_dev(field: int, chals, num_bits: int, n: int, witness, col_stride: int, col_len: int, rows=None, row0: int = 0,
                               row_stride: int = None, endo_scalar=None, out=None):
    """kh_endomul_scalar_witness_dev: the num_bits / 16 EndoMulScalar rows of n challenges (n x 2 canonical limbs); out (nullable, needs endo_scalar:
    4 Montgomery limbs): the n scalars a * endo_scalar + b."""
    _r, rp = _rows32(rows)
    es = None if endo_scalar is None else _c64(endo_scalar, (4,))
    _check(_lib.kh_endomul_scalar_witness_dev(field, _ptr(chals), num_bits, n, rp, row0, num_bits // 16 if row_stride is None else row_stride,
                                              _ptr(witness), col_stride, col_len, _p64(es) if es is not None else None, _ptr(out)))


def _modulus6(modulus: int):
    """a foreign modulus as the calls take it: three 88-bit limbs of two uint64 each"""
    L = 1 << 88
    limbs = [(modulus >> (88 * k)) % L if k < 2 else modulus >> 176 for k in range(3)]
    if modulus < 0 or limbs[2] >= 1 << 128:
        raise ValueError("foreign modulus out of range")
    return np.array([w for v in limbs for w in (v & ((1 << 64) - 1), v >> 64)], dtype=np.uint64)


def foreign_field_gate_coefficients(field: int, modulus: int):
    """kh_foreign_field_gate_coefficients (host only): (7, 4) Montgomery limbs -- ForeignFieldMul's f2, nf0, nf1, nf2, then ForeignFieldAdd's f0, f1, f2."""
    out = np.zeros((7, 4), dtype=np.uint64)
    _check(_lib.kh_foreign_field_gate_coefficients(field, _p64(_modulus6(modulus)), _p64(out)))
    return out


def range_check_witness_dev(field: int, limbs, n: int, witness, col_stride: int, col_len: int, compact: bool = False, rows=None, row0: int = 0,
                            row_stride: int = 4, flags=None, bit: int = 0):
    """kh_range_check_witness_dev: the 4 multi-range-check rows of n triples of 88-bit limbs (n x 3 x 2 uint64 at `limbs`) into the 15 columns at
    `witness`, instance i at row rows[i] or row0 + i * row_stride; flags (a DevBuf holding a zeroed uint32) gets bit `bit` set when a limb is >= 2^88."""
    _r, rp = _rows32(rows)
    _check(_lib.kh_range_check_witness_dev(field, _ptr(limbs), n, int(compact), rp, row0, row_stride, _ptr(witness), col_stride, col_len, _ptr(flags), bit))


def xor_witness_dev(field: int, in1, in2, bits: int, n: int, witness, col_stride: int, col_len: int, rows=None, row0: int = 0, row_stride: int = None,
                    out=None, flags=None, bit: int = 0):
    """kh_xor_witness_dev: the ceil(bits / 16) Xor16 rows + the zero row of n pairs of operands (n x 4 uint64 each); out (nullable): in1 ^ in2; the flag
    is set when an operand is >= 2^bits."""
    _r, rp = _rows32(rows)
    _check(_lib.kh_xor_witness_dev(field, _ptr(in1), _ptr(in2), bits, n, rp, row0, (bits + 15) // 16 + 1 if row_stride is None else row_stride,
                                   _ptr(witness), col_stride, col_len, _ptr(out), _ptr(flags), bit))


def rot64_witness_dev(field: int, words, rot: int, n: int, witness, col_stride: int, col_len: int, rows=None, row0: int = 0, row_stride: int = 3, out=None):
    """kh_rot64_witness_dev: the Rot64 row and the two RangeCheck0 rows of n words rotated left by rot; out (nullable): the n rotated words."""
    _r, rp = _rows32(rows)
    _check(_lib.kh_rot64_witness_dev(field, _ptr(words), rot, n, rp, row0, row_stride, _ptr(witness), col_stride, col_len, _ptr(out)))


def foreign_field_add_witness_dev(field: int, modulus: int, left, right, sign: int, n: int, witness, col_stride: int, col_len: int, rows=None,
                                  row0: int = 0, row_stride: int = 2, out=None, flags=None, bit: int = 0):
    """kh_foreign_field_add_witness_dev: cells 0..7 of the ForeignFieldAdd row and 0..2 of the next of n operations left + sign * right mod `modulus`
    (operands n x 3 x 2 uint64); out (nullable): the results' limbs; the flag is set when an operand is >= modulus."""
    _r, rp = _rows32(rows)
    _check(_lib.kh_foreign_field_add_witness_dev(field, _p64(_modulus6(modulus)), _ptr(left), _ptr(right), sign, n, rp, row0, row_stride, _ptr(witness),
                                                 col_stride, col_len, _ptr(out), _ptr(flags), bit))


def foreign_field_mul_witness_dev(field: int, modulus: int, a, b, n: int, witness, col_stride: int, col_len: int, rows=None, row0: int = 0,
                                  row_stride: int = 2, out_checks=None, flags=None, bit: int = 0):
    """kh_foreign_field_mul_witness_dev: the ForeignFieldMul row and cells 0..11 of the next of n products a * b mod `modulus`; out_checks (nullable,
    n x 9 limbs): quotient, remainder and (bound, p1_lo, p1_hi0), three range-check triples per instance for range_check_witness_dev."""
    _r, rp = _rows32(rows)
    _check(_lib.kh_foreign_field_mul_witness_dev(field, _p64(_modulus6(modulus)), _ptr(a), _ptr(b), n, rp, row0, row_stride, _ptr(witness), col_stride,
                                                 col_len, _ptr(out_checks), _ptr(flags), bit))


CELL_WORDS = {_CONSTANTS["KH_CELL_FIELD"]: 4, _CONSTANTS["KH_CELL_INT256"]: 4, _CONSTANTS["KH_CELL_INT128"]: 2, _CONSTANTS["KH_CELL_LIMB88"]: 2,
              _CONSTANTS["KH_CELL_U64"]: 1}          # uint64 words per value of each KH_CELL_* format


def _cells32(cells):
    c = np.ascontiguousarray(cells, dtype=np.uint32).reshape(-1, 2)
    return c, c.ctypes.data_as(C.POINTER(C.c_uint32))


def witness_gather_dev(field: int, witness, col_stride: int, col_len: int, cells, fmt: int, out, flags=None, bit: int = 0):
    """kh_witness_gather_dev: out[i] = the cell cells[i] = (row, column) of the 15 columns at `witness` in the format `fmt` (CELL_FIELD, CELL_INT256,
    CELL_INT128, CELL_LIMB88, CELL_U64: CELL_WORDS[fmt] uint64 each); the flag is set when a cell does not fit a narrow format."""
    c, cp = _cells32(cells)
    _check(_lib.kh_witness_gather_dev(field, _ptr(witness), col_stride, col_len, cp, len(c), fmt, _ptr(out), _ptr(flags), bit))


def witness_scatter_dev(field: int, values, fmt: int, cells, witness, col_stride: int, col_len: int, flags=None, bit: int = 0):
    """kh_witness_scatter_dev: the cell cells[i] = (row, column) becomes the Montgomery element of values[i], read in the format `fmt`; the flag is set
    by a CELL_INT256 value >= p and by a CELL_LIMB88 value >= 2^88."""
    c, cp = _cells32(cells)
    _check(_lib.kh_witness_scatter_dev(field, _ptr(values), fmt, cp, len(c), _ptr(witness), col_stride, col_len, _ptr(flags), bit))


def generic_witness_dev(field: int, coeffs, half: int, l, r, n: int, witness, col_stride: int, col_len: int, rows=None, row0: int = 0, row_stride: int = 1,
                        out=None):
    """kh_generic_witness_dev: cells 3 * half .. 3 * half + 2 of n generic rows = l, r (n x 4 Montgomery limbs each; r nullable: 0) and
    o = -(c_l l + c_r r + c_m l r + c_c) / c_o for the half's coefficients `coeffs` = (5, 4) Montgomery limbs l r o m c; out (nullable): the n values o."""
    _r, rp = _rows32(rows)
    _check(_lib.kh_generic_witness_dev(field, _p64(_c64(coeffs, (5, 4))), half, _ptr(l), _ptr(r), n, rp, row0, row_stride, _ptr(witness), col_stride, col_len,
                                       _ptr(out)))


def lookup_witness_dev(field: int, table_id, table_keys, table_values, table_len: int, keys, n: int, witness, col_stride: int, col_len: int, rows=None,
                       row0: int = 0, row_stride: int = 1, out_values=None, flags=None, bit: int = 0):
    """kh_lookup_witness_dev: cells 0..6 of n Lookup rows = (table_id, key, value, key, value, key, value) for the n x 3 keys at `keys`, each value
    read from `table_values` at the lowest row of `table_keys` that holds the key (two device columns of table_len elements: DevBufs, views or what
    NativeProverIndex.lookup_table returns).  table_id: 4 Montgomery limbs.  out_values (nullable): the n x 3 values; the flag is set by a key that
    is in no row of the table, whose value is then zero."""
    _r, rp = _rows32(rows)
    _check(_lib.kh_lookup_witness_dev(field, _p64(_c64(table_id, (4,))), _ptr(table_keys), _ptr(table_values), table_len, _ptr(keys), n, rp, row0, row_stride,
                                      _ptr(witness), col_stride, col_len, _ptr(out_values), _ptr(flags), bit))


def field_inverse_dev(field: int, values, n: int, out, flags=None, bit: int = 0):
    """kh_field_inverse_dev: out[i] = values[i]^-1 for n Montgomery elements (DevBufs or views; out may be `values`); a zero gives zero and sets the flag
    -- the "inverse or zero" advice of is_zero, whose caller passes no flags."""
    _check(_lib.kh_field_inverse_dev(field, _ptr(values), n, _ptr(out), _ptr(flags), bit))


def field_sqrt_dev(field: int, values, n: int, out, out_is_square=None, flags=None, bit: int = 0):
    """kh_field_sqrt_dev: out[i] = the square root ark-ff's Tonelli-Shanks returns for values[i] (out may be `values`); zero gives zero; a non-residue
    gives zero and sets the flag.  out_is_square (nullable): n elements, the Montgomery 1 or 0."""
    _check(_lib.kh_field_sqrt_dev(field, _ptr(values), n, _ptr(out), _ptr(out_is_square), _ptr(flags), bit))


def field_bits_dev(field: int, values, fmt: int, num_bits: int, n: int, out, flags=None, bit: int = 0):
    """kh_field_bits_dev: the low num_bits bits of n values in the format `fmt` (CELL_WORDS[fmt] uint64 each, as witness_gather_dev delivers them) as
    Montgomery 0 / 1, bit-major: bit k of value i is element k * n + i of out (num_bits x n elements); the flag is set by a value >= 2^num_bits."""
    _check(_lib.kh_field_bits_dev(field, _ptr(values), fmt, num_bits, n, _ptr(out), _ptr(flags), bit))


WitnessRefC, WitnessStepC = _STRUCTURES["kh_witness_ref_t"], _STRUCTURES["kh_witness_step_t"]
REF_NONE, REF_ARENA, STEP_NO_FLAG = _CONSTANTS["KH_REF_NONE"], _CONSTANTS["KH_REF_ARENA"], _CONSTANTS["KH_STEP_NO_FLAG"]
(STEP_GATHER, STEP_SCATTER, STEP_GENERIC, STEP_POSEIDON, STEP_COMPLETE_ADD, STEP_VARBASEMUL, STEP_ENDOMUL, STEP_ENDOMUL_SCALAR, STEP_RANGE_CHECK, STEP_XOR,
 STEP_ROT64, STEP_FF_ADD, STEP_FF_MUL, STEP_LOOKUP, STEP_INVERSE, STEP_SQRT, STEP_BITS) = (_CONSTANTS["KH_STEP_" + _n] for _n in (
     "GATHER", "SCATTER", "GENERIC", "POSEIDON", "COMPLETE_ADD", "VARBASEMUL", "ENDOMUL", "ENDOMUL_SCALAR", "RANGE_CHECK", "XOR", "ROT64", "FF_ADD", "FF_MUL",
     "LOOKUP", "INVERSE", "SQRT", "BITS"))
_STEP_FIELDS = ("op", "n", "rows", "row0", "row_stride", "cells", "format", "param", "sign", "consts", "in", "out", "flag_bit")     # kh_witness_step_t's order


def _witness_ref(ref):
    """None -> absent; (buf, offset) with buf = REF_ARENA or the index of a bound buffer; a bare int is (buf, 0)"""
    if ref is None:
        return WitnessRefC(REF_NONE, 0)
    return WitnessRefC(int(ref), 0) if isinstance(ref, (int, np.integer)) else WitnessRefC(int(ref[0]), int(ref[1]))


class WitnessSchedule:
    """kh_witness_schedule_*: a circuit's gadget and wire steps, validated and uploaded once (`create`), run per proof (`run`).  A step is a dict with
    the fields of kh_witness_step_t (or a tuple in their order: op, n, rows, row0, row_stride, cells, format, param, sign, consts, in, out, flag_bit);
    what a dict leaves out is 0 / None, n defaults to the number of cells, flag_bit to STEP_NO_FLAG.  in / out: lists of refs -- None, (REF_ARENA,
    offset), (index of a bound buffer, offset).  consts: uint64 limbs as the direct call takes them (STEP_LOOKUP: the table id's 4 Montgomery limbs, with
    param = table_len and in = [keys, table keys, table values]), or the modulus as an int for the foreign-field steps.  The value steps (STEP_INVERSE,
    STEP_SQRT, STEP_BITS) take n, in = [values], out = [result] (STEP_SQRT: [root, is_square or None]) and, for STEP_BITS, format and param = num_bits."""

    def __init__(self, handle, n_bufs: int, col_len: int):
        self.handle, self.n_bufs, self.col_len = handle, n_bufs, col_len

    @staticmethod
    def pack(steps):
        """(a kh_witness_step_t array of the steps, the host arrays it points to: to be kept until create has returned)"""
        arr = (WitnessStepC * max(1, len(steps)))()
        keep = []                                                  # the host arrays the structs point to, until create has copied them
        for st, src in zip(arr, steps):
            d = dict(zip(_STEP_FIELDS, src)) if isinstance(src, (tuple, list)) else dict(src)
            unknown = set(d) - set(_STEP_FIELDS)
            if unknown:
                raise ValueError(f"step fields {sorted(unknown)} are not kh_witness_step_t's")
            st.op = d["op"]
            if d.get("cells") is not None:
                c, st.cells = _cells32(d["cells"]); keep.append(c)
                st.n = len(c)
            if d.get("rows") is not None:
                r, st.rows = _rows32(d["rows"]); keep.append(r)
            if d.get("n") is not None:
                st.n = d["n"]
            st.row0, st.row_stride = d.get("row0") or 0, d.get("row_stride") or 0
            st.format, st.param, st.sign = d.get("format") or 0, d.get("param") or 0, d.get("sign") or 0
            consts = d.get("consts")
            if consts is not None:
                k = _modulus6(consts) if isinstance(consts, int) else _c64(consts).reshape(-1)
                keep.append(k)
                st.consts = _p64(k)
            for name, count in (("in", 3), ("out", 2)):
                refs = list(d.get(name) or ())
                if len(refs) > count:
                    raise ValueError(f"a step has {count} `{name}` refs at most")
                setattr(st, name, (WitnessRefC * count)(*[_witness_ref(r) for r in refs + [None] * (count - len(refs))]))
            st.flag_bit = STEP_NO_FLAG if d.get("flag_bit") is None else d["flag_bit"]
        return arr, keep

    @classmethod
    def create(cls, field: int, col_len: int, steps, arena_bytes: int = 0, n_bufs: int = 0):
        arr, _keep = cls.pack(steps)
        h = C.c_void_p()
        _check(_lib.kh_witness_schedule_create(field, col_len, arr, len(steps), arena_bytes, n_bufs, C.byref(h)))
        return cls(h, n_bufs, col_len)

    def run(self, bufs, witness, col_stride: int = None, flags=None):
        """one proof's witness into the 15 columns at `witness` (col_stride: col_len unless given) from the bound buffers `bufs` (DevBufs, views or
        addresses, as many as the schedule binds); flags: a DevBuf holding the run's flag word"""
        ptrs = (C.c_void_p * max(1, len(bufs)))(*[b if isinstance(b, int) else b.ptr for b in bufs])
        _check(_lib.kh_witness_schedule_run(self.handle, ptrs, len(bufs), _ptr(witness), self.col_len if col_stride is None else col_stride, _ptr(flags)))

    def info(self):
        """{"steps", "launch_groups", "resident_bytes", "run_bytes"}"""
        v = [C.c_size_t() for _ in range(4)]
        _check(_lib.kh_witness_schedule_info(self.handle, *[C.byref(x) for x in v]))
        return dict(zip(("steps", "launch_groups", "resident_bytes", "run_bytes"), (x.value for x in v)))

    def free(self):
        if self.handle:
            _lib.kh_witness_schedule_free(self.handle)
            self.handle = None


class Comm:
    """kh_comm_*: the in-library RCCL communicator of the one-process-per-GPU deployment (no torch).  Comm.unique_id() on one rank, the bytes to
    the others, Comm(world, rank, id) on every rank."""

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        _check(_lib.kh_comm_unique_id(buf))
        return bytes(buf)

    def __init__(self, world: int, rank: int, uid: bytes):
        self._h = C.c_void_p()
        buf = (C.c_uint8 * 128)(*uid)
        _check(_lib.kh_comm_init(world, rank, buf, C.byref(self._h)))
        self.world, self.rank = world, rank

    def allgather_points(self, xy, inf):
        xy = _c64(xy, (-1, 8)); i8 = np.ascontiguousarray(inf, dtype=np.uint8).reshape(-1)
        k = xy.shape[0]
        out = np.zeros((self.world * k, 8), dtype=np.uint64); oinf = np.zeros(self.world * k, dtype=np.uint8)
        _check(_lib.kh_comm_allgather_points(self._h, _p64(xy), _p8(i8), k, _p64(out), _p8(oinf)))
        return out, oinf

    def msm_allreduce(self, shard, scalars, mont: bool = True):
        sc = _c64(scalars, (-1, 4))
        out = np.zeros(8, dtype=np.uint64); inf = np.zeros(1, dtype=np.uint8)
        _check(_lib.kh_msm_allreduce(self._h, shard._h, _p64(sc), sc.shape[0], int(mont), _p64(out), _p8(inf)))
        return out, bool(inf[0])

    def free(self):
        if self._h:
            _lib.kh_comm_free(self._h); self._h = C.c_void_p()


PROOF_SECTIONS = _sections("KH_PROOF_")
LOOKUP_PATTERN_IDS = {"Xor": 0, "Lookup": 1, "RangeCheck": 2, "ForeignFieldMul": 3}
PROOF_PHASES = ("witness_upload", "witness_commit", "z", "quotient", "evaluations", "opening")
VINDEX_SECTIONS = _sections("KH_VINDEX_")
LOOKUP_COLUMN_BLOCKS = _sections("KH_LOOKUP_COL_")
LOOKUP_INFO_FIELDS = ("max_per_row", "max_joint_size", "joint_lookup_used", "uses_runtime_tables", "pattern_mask", "table_columns", "runtime_offset", "runtime_len")
INDEX_PHASES = ("columns", "transforms", "commitments", "digest")


def witness_report_message(report: "WitnessReportC", cap: int = 512) -> str:
    """kh_witness_report_message: the report as one line, cut at cap - 1 characters."""
    buf = C.create_string_buffer(max(cap, 1))
    rc = _lib.kh_witness_report_message(C.byref(report), buf, cap)
    if rc < 0:
        _check(rc)
    return buf.value.decode()


def witness_check(index, witness=None, witness_dev=None, flags: int = WITNESS_GATES | WITNESS_WIRES) -> "WitnessReportC":
    """kh_witness_check on a NativeProverIndex: witness (15, rows, 4) Montgomery limbs on the host, or witness_dev: a DevBuf with the padded 15 x n
    columns.  Returns the filled kh_witness_report_t (kind WITNESS_OK / WITNESS_DISCONNECTED / WITNESS_GATE); bad arguments raise KhError."""
    w = _c64(witness, (15, -1, 4)) if witness is not None else None
    rep = WitnessReportC()
    _check(_lib.kh_witness_check(index._h, _p64(w) if w is not None else None, w.shape[1] if w is not None else 0,
                                 C.c_void_p(witness_dev.ptr) if witness_dev is not None else None, flags, C.byref(rep)))
    return rep


def witness_check_full(index, witness=None, witness_dev=None, runtime=None, flags: int = WITNESS_GATES | WITNESS_WIRES | WITNESS_LOOKUPS, runtime_dev=None):
    """kh_witness_check_full on a NativeProverIndex: as witness_check, + the lookups (WITNESS_LOOKUPS; runtime: (k, 4) limbs, the runtime tables' second
    column, as for prove -- or runtime_dev = (a DevBuf or view holding them, k): kh_witness_check_full_runtime_dev).  Returns (kh_witness_report_t,
    kh_witness_lookup_t), both filled; bad arguments raise KhError."""
    w = _c64(witness, (15, -1, 4)) if witness is not None else None
    rtv = _c64(runtime, (-1, 4)) if runtime is not None else None
    rep, lk = WitnessReportC(), WitnessLookupC()
    if runtime_dev is not None:
        if runtime is not None:
            raise ValueError("runtime values either on the host or on the device")
        _check(_lib.kh_witness_check_full_runtime_dev(index._h, _p64(w) if w is not None else None, w.shape[1] if w is not None else 0,
                                                      C.c_void_p(witness_dev.ptr) if witness_dev is not None else None, _ptr(runtime_dev[0]), runtime_dev[1],
                                                      flags, C.byref(rep), C.byref(lk)))
        return rep, lk
    _check(_lib.kh_witness_check_full(index._h, _p64(w) if w is not None else None, w.shape[1] if w is not None else 0,
                                      C.c_void_p(witness_dev.ptr) if witness_dev is not None else None, _p64(rtv) if rtv is not None else None,
                                      rtv.shape[0] if rtv is not None else 0, flags, C.byref(rep), C.byref(lk)))
    return rep, lk


def witness_lookup_message(report: "WitnessReportC", lookup: "WitnessLookupC", cap: int = 512) -> str:
    """kh_witness_lookup_message: report and lookup record as one line, cut at cap - 1 characters."""
    buf = C.create_string_buffer(max(cap, 1))
    rc = _lib.kh_witness_lookup_message(C.byref(report), C.byref(lookup), buf, cap)
    if rc < 0:
        _check(rc)
    return buf.value.decode()


def _proof_sections(pr):
    """{section name: (xy (k, 8), inf (k,)) | (k, 4) limbs} of a proof handle: copies of what kh_proof_section shows"""
    out = {}
    for name, sid in PROOF_SECTIONS.items():
        lp = C.POINTER(C.c_uint64)(); fp = C.POINTER(C.c_uint8)(); cnt = C.c_size_t(0)
        _check(_lib.kh_proof_section(pr, sid, C.byref(lp), C.byref(fp), C.byref(cnt)))
        k = cnt.value
        if fp:                                    # points
            out[name] = (np.ctypeslib.as_array(lp, shape=(k, 8)).copy() if k else np.zeros((0, 8), np.uint64),
                         np.ctypeslib.as_array(fp, shape=(k,)).copy() if k else np.zeros(0, np.uint8))
        else:
            out[name] = np.ctypeslib.as_array(lp, shape=(k, 4)).copy() if k else np.zeros((0, 4), np.uint64)
    return out


class NativeProverIndex:
    """kh_prover_index_new: the C++ prover's view of device-resident index columns (they must outlive the handle); or, NativeProverIndex.create,
    kh_prover_index_create: an index built from gate records that owns its columns."""

    def __init__(self, srs, log2_n: int, zk_rows: int, public: int, d1, dc, d8, optional_gate_ids, live_mask: int, shifts, digest):
        self._h = C.c_void_p()
        opt = (C.c_int * max(len(optional_gate_ids), 1))(*optional_gate_ids)
        sh = _c64(shifts, (7, 4)); dg = _c64(digest, (4,))
        _check(_lib.kh_prover_index_new(srs._h, log2_n, zk_rows, public, C.c_void_p(d1.ptr), C.c_void_p(dc.ptr), C.c_void_p(d8.ptr),
                                        opt, len(optional_gate_ids), live_mask, _p64(sh), _p64(dg), C.byref(self._h)))
        self._keep = (srs, d1, dc, d8)

    @classmethod
    def create(cls, srs, gate_types, wires, coeffs, public: int = 0):
        """kh_prover_index_create: the index (columns owned by the handle) and its verifier index from gate records -- gate_types: one kh gate id
        per row (GATE_ZERO: no constraints); wires: (rows, 7, 2) (row, col) pairs; coeffs: (rows, 15, 4) Montgomery limbs."""
        self = cls.__new__(cls)
        types = np.ascontiguousarray(gate_types, dtype=np.int32).reshape(-1)
        rows = types.shape[0]
        w = np.ascontiguousarray(wires, dtype=np.uint32).reshape(rows, 7, 2)
        co = _c64(coeffs, (rows, 15, 4))
        self._h = C.c_void_p()
        _check(_lib.kh_prover_index_create(srs._h, rows, types.ctypes.data_as(C.POINTER(C.c_int)), w.ctypes.data_as(C.POINTER(C.c_uint32)),
                                           _p64(co), public, C.byref(self._h)))
        self._keep = (srs,)
        return self

    @classmethod
    def create_lookup(cls, srs, gate_types, wires, coeffs, public: int = 0, tables=(), runtime_tables=()):
        """kh_prover_index_create_lookup: as `create`, for circuits with a lookup argument (gate_types may hold the lookup gates and GATE_LOOKUP).
        tables: [(id, data (width, len, 4) Montgomery limbs)]; runtime_tables: [(id, first column (len, 4) limbs)] (RuntimeTableCfg)."""
        self = cls.__new__(cls)
        types = np.ascontiguousarray(gate_types, dtype=np.int32).reshape(-1)
        rows = types.shape[0]
        w = np.ascontiguousarray(wires, dtype=np.uint32).reshape(rows, 7, 2)
        co = _c64(coeffs, (rows, 15, 4))
        tdata = [np.ascontiguousarray(d, dtype=np.uint64) for _i, d in tables]
        assert all(d.ndim == 3 and d.shape[2] == 4 for d in tdata), "table data: (width, len, 4) limbs"
        rdata = [_c64(d, (-1, 4)) for _i, d in runtime_tables]
        tc = (LookupTableC * max(len(tdata), 1))(*[LookupTableC(int(i), d.shape[0], d.shape[1], _p64(d)) for (i, _d), d in zip(tables, tdata)])
        rc = (RuntimeTableCfgC * max(len(rdata), 1))(*[RuntimeTableCfgC(int(i), d.shape[0], _p64(d)) for (i, _d), d in zip(runtime_tables, rdata)])
        self._h = C.c_void_p()
        _check(_lib.kh_prover_index_create_lookup(srs._h, rows, types.ctypes.data_as(C.POINTER(C.c_int)), w.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                  _p64(co), public, tc, len(tdata), rc, len(rdata), C.byref(self._h)))
        self._keep = (srs,)
        return self

    def shape(self):
        """(log2_n, zk_rows, num_chunks)"""
        ln, zk, nch = C.c_uint(0), C.c_uint(0), C.c_size_t(0)
        _check(_lib.kh_prover_index_shape(self._h, C.byref(ln), C.byref(zk), C.byref(nch)))
        return ln.value, zk.value, nch.value

    def verifier_index(self):
        """kh_verifier_index_section for every section: {name: (xy (k, 8), inf (k,))} for commitments, {name: (k, 4) limbs} for shifts / digest."""
        out = {}
        for name, sid in VINDEX_SECTIONS.items():
            lp = C.POINTER(C.c_uint64)(); fp = C.POINTER(C.c_uint8)(); cnt = C.c_size_t(0)
            _check(_lib.kh_verifier_index_section(self._h, sid, C.byref(lp), C.byref(fp), C.byref(cnt)))
            k = cnt.value
            if fp:
                out[name] = (np.ctypeslib.as_array(lp, shape=(k, 8)).copy() if k else np.zeros((0, 8), np.uint64),
                             np.ctypeslib.as_array(fp, shape=(k,)).copy() if k else np.zeros(0, np.uint8))
            elif name in ("shifts", "digest"):
                out[name] = np.ctypeslib.as_array(lp, shape=(k, 4)).copy()
            elif name == "lookup_info":               # plain integers, None for an index without a lookup argument
                out[name] = dict(zip(LOOKUP_INFO_FIELDS, (int(x) for x in np.ctypeslib.as_array(lp, shape=(4 * k,))))) if k else None
            else:                                     # a commitment section with no entries (no optional gate)
                out[name] = (np.zeros((0, 8), np.uint64), np.zeros(0, np.uint8))
        return out

    def lookup_table(self, table_id: int):
        """kh_prover_index_lookup_table: {"first_row", "len", "is_runtime", "runtime_first", "keys", "values"} of the table with this id in an index
        from create_lookup -- keys / values: DevViews of columns 0 and 1 of the combined table at first_row (values None for a one-column table), the
        index's memory --, or None where the index has no such table (KH_E_NOTFOUND)."""
        fr, ln, rf, rt = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_int(0)
        kd, vd = C.c_void_p(), C.c_void_p()
        rc = _lib.kh_prover_index_lookup_table(self._h, table_id, C.byref(fr), C.byref(ln), C.byref(rt), C.byref(rf), C.byref(kd), C.byref(vd))
        if rc == _CONSTANTS["KH_E_NOTFOUND"]:
            return None
        _check(rc)
        return {"first_row": fr.value, "len": ln.value, "is_runtime": bool(rt.value), "runtime_first": rf.value, "keys": DevView(kd.value),
                "values": DevView(vd.value) if vd.value else None}

    def lookup_column(self, block: str, k: int = 0):
        """kh_debug_lookup_column, downloaded: (elems, 4) limbs of column k of a block of LOOKUP_COLUMN_BLOCKS, or None where the index has none."""
        dev = U64P(); cnt = C.c_size_t(0)
        if _lib.kh_debug_lookup_column(self._h, LOOKUP_COLUMN_BLOCKS[block], k, C.byref(dev), C.byref(cnt)) != 0:
            return None
        out = np.zeros((cnt.value, 4), dtype=np.uint64)
        sync()
        _check(_lib.kh_dev_download(_p64(out), C.cast(dev, C.c_void_p), out.nbytes))
        return out

    def phase_seconds(self):
        """kh_prover_index_phase_seconds: {phase: seconds} of kh_prover_index_create"""
        ph = (C.c_double * 4)()
        _check(min(0, _lib.kh_prover_index_phase_seconds(self._h, ph, 4)))
        return dict(zip(INDEX_PHASES, list(ph)))

    def attach_lookup(self, patterns, sel_d1, sel_c, sel_d8, table_cols, table_ids, atoms8):
        """kh_prover_index_attach_lookup: patterns = names in the reference's order; per pattern three DevBufs; table columns / ids / atoms: DevBufs."""
        m = len(patterns)
        arr = lambda bufs: (C.c_void_p * max(len(bufs), 1))(*[C.c_void_p(b.ptr) for b in bufs])
        ids = (C.c_int * m)(*[LOOKUP_PATTERN_IDS[q] for q in patterns])
        _check(_lib.kh_prover_index_attach_lookup(self._h, ids, m, arr(sel_d1), arr(sel_c), arr(sel_d8), arr(table_cols), len(table_cols),
                                                  C.c_void_p(table_ids.ptr) if table_ids is not None else None, arr(atoms8)))
        self._keep += (sel_d1, sel_c, sel_d8, table_cols, table_ids, atoms8)

    def attach_runtime_tables(self, sel_d1, sel_c, sel_d8, offset: int, length: int):
        _check(_lib.kh_prover_index_attach_runtime_tables(self._h, C.c_void_p(sel_d1.ptr), C.c_void_p(sel_c.ptr), C.c_void_p(sel_d8.ptr), offset, length))
        self._keep += (sel_d1, sel_c, sel_d8)

    def witness_check(self, witness=None, witness_dev=None, flags: int = WITNESS_GATES | WITNESS_WIRES):
        """kh_witness_check (see witness_check)"""
        return witness_check(self, witness, witness_dev, flags)

    def witness_check_full(self, witness=None, witness_dev=None, runtime=None, flags: int = WITNESS_GATES | WITNESS_WIRES | WITNESS_LOOKUPS, runtime_dev=None):
        """kh_witness_check_full / kh_witness_check_full_runtime_dev (see witness_check_full)"""
        return witness_check_full(self, witness, witness_dev, runtime, flags, runtime_dev)

    def randomness_count(self, witness_on_host: bool) -> int:
        return _lib.kh_prove_randomness_count(self._h, int(witness_on_host))

    def prove(self, witness=None, witness_dev=None, randomness=None, flags: int = PROVE_CHECK, prev=(), runtime=None, runtime_dev=None):
        """kh_prove_full (runtime: (k, 4) limbs, the runtime tables' second column; or runtime_dev = (a DevBuf or view holding them, k):
        kh_prove_full_runtime_dev, read in stream order).  witness: (15, rows, 4) limbs on the host, or witness_dev: DevBuf with the padded columns.  randomness:
        (k, 4) limbs in the reference's draw order, or None (the library draws from the OS).  prev: [(chals (k, 4) limbs, (xy (chunks, 8), inf
        (chunks,)))].  Returns ({section: limbs[, flags]}, {phase: seconds})."""
        pr = self._prove(witness, witness_dev, randomness, flags, prev, runtime, runtime_dev)
        try:
            out = _proof_sections(pr)
            ph = (C.c_double * 6)()
            _lib.kh_proof_phase_seconds(pr, ph, 6)
            return out, dict(zip(PROOF_PHASES, list(ph)))
        finally:
            _lib.kh_proof_free(pr)

    def prove_handle(self, witness=None, witness_dev=None, randomness=None, flags: int = PROVE_CHECK, prev=(), runtime=None, runtime_dev=None):
        """`prove`, returning the proof as a Proof handle: it carries its shape and previous challenges, so Proof.to_msgpack needs nothing else"""
        pr = Proof.__new__(Proof)
        pr._h = self._prove(witness, witness_dev, randomness, flags, prev, runtime, runtime_dev)
        return pr

    def _prove(self, witness, witness_dev, randomness, flags, prev, runtime, runtime_dev):
        pr = C.c_void_p()
        w = _c64(witness, (15, -1, 4)) if witness is not None else None
        rnd = _c64(randomness, (-1, 4)) if randomness is not None else None
        m = len(prev)
        chals = _c64(np.concatenate([np.asarray(c, dtype=np.uint64).reshape(-1, 4) for c, _ in prev]), (-1, 4)) if m else None
        rounds = (C.c_uint * max(m, 1))(*[np.asarray(c).reshape(-1, 4).shape[0] for c, _ in prev])
        cxy = np.ascontiguousarray(np.concatenate([np.asarray(cm[0], dtype=np.uint64).reshape(-1, 8) for _, cm in prev])) if m else None
        cinf = np.ascontiguousarray(np.concatenate([np.asarray(cm[1], dtype=np.uint8).reshape(-1) for _, cm in prev])) if m else None
        cch = (C.c_size_t * max(m, 1))(*[np.asarray(cm[1]).reshape(-1).shape[0] for _, cm in prev])
        rtv = _c64(runtime, (-1, 4)) if runtime is not None else None
        if runtime_dev is not None and runtime is not None:
            raise ValueError("runtime values either on the host or on the device")
        fn = _lib.kh_prove_full if runtime_dev is None else _lib.kh_prove_full_runtime_dev
        rt_args = (_p64(rtv) if rtv is not None else None, rtv.shape[0] if rtv is not None else 0) if runtime_dev is None else (_ptr(runtime_dev[0]), runtime_dev[1])
        _check(fn(self._h, _p64(w) if w is not None else None, w.shape[1] if w is not None else 0,
                  C.c_void_p(witness_dev.ptr) if witness_dev is not None else None, _p64(rnd) if rnd is not None else None,
                  rnd.shape[0] if rnd is not None else 0, flags, _p64(chals) if m else None, rounds,
                  _p64(cxy) if m else None, _p8(cinf) if m else None, cch, m, *rt_args, C.byref(pr)))
        return pr

    def free(self):
        if self._h:
            _lib.kh_prover_index_free(self._h); self._h = C.c_void_p()


# ---------------------------------------------------------------------------------------------------- the native verifier
VERIFY_PHASES = ("transcript", "constant_term", "scalars", "final_msm")


def _section_array(sections: dict, names: dict):
    """{name: (xy (k, 8), inf (k,)) | (k, 4) limbs | 8 plain words (lookup_info: a dict or a sequence) | None} -> kh_section_t[len(names)] + what keeps it alive"""
    arr = (SectionC * len(names))()
    keep = []
    for name, sid in names.items():
        v = sections.get(name)
        if v is None:
            continue
        if name == "lookup_info":
            w = np.ascontiguousarray([v[f] for f in LOOKUP_INFO_FIELDS] if isinstance(v, dict) else list(v), dtype=np.uint64).reshape(8)
            keep.append(w)
            arr[sid] = SectionC(_p64(w), None, 2)
        elif isinstance(v, tuple):
            xy = _c64(v[0], (-1, 8)); inf = np.ascontiguousarray(v[1], dtype=np.uint8).reshape(-1) if v[1] is not None else None
            keep += [xy, inf]
            if xy.shape[0]:
                arr[sid] = SectionC(_p64(xy), _p8(inf) if inf is not None else None, xy.shape[0])
        else:
            e = _c64(v, (-1, 4))
            keep.append(e)
            if e.shape[0]:
                arr[sid] = SectionC(_p64(e), None, e.shape[0])
    return arr, keep


def _sized(call, as_array: bool = False):
    """the calling convention of the writers (out, cap, len): a size query (out = NULL), then the call that writes into exactly that many bytes"""
    ln = C.c_size_t(0)
    _check(call(None, 0, C.byref(ln)))
    buf = np.zeros(max(ln.value, 1), dtype=np.uint8)
    _check(call(buf.ctypes.data_as(U8P), ln.value, C.byref(ln)))
    return buf[:ln.value] if as_array else buf[:ln.value].tobytes()


def proofs_from_msgpack_raw(curve: int, blobs, out_before: int = 0):
    """kh_proofs_from_msgpack without raising: (return code, the k entries of `out` afterwards)"""
    k = len(blobs)
    arrs = [np.frombuffer(bytes(b), dtype=np.uint8) if len(b) else np.zeros(1, np.uint8) for b in blobs]
    ptrs = (U8P * max(k, 1))(*[a.ctypes.data_as(U8P) for a in arrs])
    lens = (C.c_size_t * max(k, 1))(*[len(b) for b in blobs])
    out = (C.c_void_p * max(k, 1))(*([out_before] * max(k, 1)))
    rc = _lib.kh_proofs_from_msgpack(curve, ptrs, lens, k, out)
    return rc, [out[p] or 0 for p in range(k)]


class VerifierIndex:
    """kh_verifier_index_new: a verifier index from sections in the layout NativeProverIndex.verifier_index() returns (absent / None = not there; shifts and
    digest are computed when absent); VerifierIndex.of(native_index): kh_verifier_index_of."""

    def __init__(self, srs, log2_n: int, zk_rows: int, public: int, prev_challenges: int, optional_gate_ids, sections: dict):
        self._h = C.c_void_p()
        opt = (C.c_int * max(len(optional_gate_ids), 1))(*optional_gate_ids)
        arr, _keep = _section_array(sections, VINDEX_SECTIONS)
        _check(_lib.kh_verifier_index_new(srs._h, log2_n, zk_rows, public, prev_challenges, opt, len(optional_gate_ids), arr, len(arr), C.byref(self._h)))
        self._keep = (srs,)

    @classmethod
    def of(cls, index: "NativeProverIndex"):
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        _check(_lib.kh_verifier_index_of(index._h, C.byref(self._h)))
        self._keep = index._keep[:1]
        return self

    @classmethod
    def from_msgpack(cls, srs, data: bytes):
        """kh_verifier_index_from_msgpack: the index a serialised VerifierIndex (rmp-serde) describes, over `srs`; its commitments decoded in one launch"""
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        b = np.frombuffer(bytes(data), dtype=np.uint8)
        _check(_lib.kh_verifier_index_from_msgpack(srs._h, b.ctypes.data_as(U8P), b.size, C.byref(self._h)))
        self._keep = (srs,)
        return self

    def to_msgpack(self, prev_challenges: int = 0) -> bytes:
        """kh_verifier_index_to_msgpack: the bytes the reference writes for this index (a size query, then the call that writes)"""
        return _sized(lambda out, cap, ln: _lib.kh_verifier_index_to_msgpack(self._h, prev_challenges, out, cap, ln))

    def digest(self):
        out = np.zeros(4, dtype=np.uint64)
        _check(_lib.kh_verifier_index_digest(self._h, _p64(out)))
        return out

    def free(self):
        if self._h:
            _lib.kh_verifier_index_free(self._h); self._h = C.c_void_p()


class Proof:
    """kh_proof_from_sections: a proof handle from the sections NativeProverIndex.prove returns (or a caller's own, same layout)."""

    def __init__(self, sections: dict):
        self._h = C.c_void_p()
        arr, _keep = _section_array(sections, PROOF_SECTIONS)
        _check(_lib.kh_proof_from_sections(arr, len(arr), C.byref(self._h)))

    def sections(self):
        """the proof's sections as NativeProverIndex.prove returns them (kh_proof_section)"""
        return _proof_sections(self._h)

    @classmethod
    def from_msgpack(cls, curve: int, data):
        """kh_proofs_from_msgpack: a Proof from the bytes of one serialised ProverProof, or [Proof] from a list of them -- then the points of all of them are
        decoded in one launch.  Malformed bytes raise KhError naming the byte offset, or section, index and status; no proof is made."""
        many = isinstance(data, (list, tuple))
        rc, handles = proofs_from_msgpack_raw(curve, list(data) if many else [data])
        _check(rc)
        made = []
        for h in handles:
            pr = cls.__new__(cls)
            pr._h = C.c_void_p(h)
            made.append(pr)
        return made if many else made[0]

    def to_msgpack(self, curve: int, shape: "VerifierIndex" = None) -> bytes:
        """kh_proof_to_msgpack: the bytes the reference writes for this proof.  shape: an index of the proof's circuit, needed by a handle that does not know
        which optional evaluations it has (one from sections or from wire bytes)."""
        return _sized(lambda out, cap, ln: _lib.kh_proof_to_msgpack(curve, self._h, shape._h if shape is not None else None, out, cap, ln))

    def to_wire(self, curve: int):
        """kh_proof_to_wire: {section name: bytes} in the form proofs_from_wire takes (count x 33 compressed records / count x 32 little-endian integers)"""
        secs = (WireSectionC * len(PROOF_SECTIONS))()
        buf = _sized(lambda out, cap, ln: _lib.kh_proof_to_wire(curve, self._h, out, cap, ln, secs), as_array=True)
        base = buf.ctypes.data
        out = {}
        for name, sid in PROOF_SECTIONS.items():
            width = 32 if name in _ELEMENT_SECTIONS else POINT_BYTES
            off = C.cast(secs[sid].bytes, C.c_void_p).value
            out[name] = bytes(buf[off - base: off - base + width * secs[sid].count]) if secs[sid].count else b""
        return out

    def prev_challenges(self):
        """kh_proof_prev_challenges: [(chals (rounds, 4) limbs, (xy (chunks, 8), inf (chunks,)))] as `prove` and `verify` take them"""
        ch, xy = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()
        rounds, inf, chunks, n = C.POINTER(C.c_uint)(), C.POINTER(C.c_uint8)(), C.POINTER(C.c_size_t)(), C.c_size_t(0)
        _check(_lib.kh_proof_prev_challenges(self._h, C.byref(ch), C.byref(rounds), C.byref(xy), C.byref(inf), C.byref(chunks), C.byref(n)))
        out, cpos, ppos = [], 0, 0
        for j in range(n.value):
            r, c = rounds[j], chunks[j]
            out.append((np.array([[ch[4 * (cpos + i) + l] for l in range(4)] for i in range(r)], dtype=np.uint64).reshape(r, 4),
                        (np.array([[xy[8 * (ppos + i) + l] for l in range(8)] for i in range(c)], dtype=np.uint64).reshape(c, 8),
                         np.array([inf[ppos + i] for i in range(c)], dtype=np.uint8))))
            cpos += r; ppos += c
        return out

    def free(self):
        if self._h:
            _lib.kh_proof_free(self._h); self._h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


WireSectionC = _STRUCTURES["kh_wire_section_t"]
_ELEMENT_SECTIONS = ("evals", "public_evals", "ft_eval1", "z1_z2", "challenges")      # count x 32 bytes; every other section is points


def proofs_from_wire_raw(curve: int, proofs, out_before: int = 0):
    """kh_proofs_from_wire without raising: (return code, the k entries of `out` afterwards -- out_before where the call left them alone)"""
    k, ns = len(proofs), len(PROOF_SECTIONS)
    arr = (WireSectionC * max(k * ns, 1))()
    keep = []
    for p, sections in enumerate(proofs):
        for name, sid in PROOF_SECTIONS.items():
            v = sections.get(name)
            if v is None:
                continue
            b = np.ascontiguousarray(np.frombuffer(bytes(v), dtype=np.uint8) if isinstance(v, (bytes, bytearray, memoryview)) else v, dtype=np.uint8).reshape(-1)
            width = 32 if name in _ELEMENT_SECTIONS else POINT_BYTES
            assert b.size % width == 0, f"section {name}: {b.size} bytes are no multiple of {width}"
            keep.append(b)
            if b.size:
                arr[p * ns + sid] = WireSectionC(b.ctypes.data_as(U8P), b.size // width)
    out = (C.c_void_p * max(k, 1))(*([out_before] * max(k, 1)))
    rc = _lib.kh_proofs_from_wire(curve, arr, ns, k, out)
    return rc, [out[p] or 0 for p in range(k)]


def proofs_from_wire(curve: int, proofs):
    """kh_proofs_from_wire: [Proof] from a list of {section name: bytes-like} in the serialised form -- point sections count x 33 compressed records, element
    sections count x 32 little-endian canonical integers; every point of every proof is decoded in one launch.  A bad record or element raises KhError
    naming proof, section and index, and no proof is made."""
    rc, handles = proofs_from_wire_raw(curve, proofs)
    _check(rc)
    made = []
    for h in handles:
        pr = Proof.__new__(Proof)
        pr._h = C.c_void_p(h)
        made.append(pr)
    return made


def _trace(t: "VerifyTraceC"):
    a = lambda x: np.ctypeslib.as_array(x).copy()
    return {"challenges": a(t.challenges), "constant_term": a(t.constant_term), "ft_eval0": a(t.ft_eval0), "combined_inner_product": a(t.combined_inner_product)}


def batch_verify_raw(items, rand=None, ok_before: int = -1, count=None):
    """kh_batch_verify without raising: (return code, *ok afterwards (ok_before if the call left it alone), [trace dict per item]).  items: [(VerifierIndex,
    Proof, public (k, 4) limbs or None, prev)] with prev as for NativeProverIndex.prove; count: the k handed to the library (default: len(items))."""
    k = len(items)
    arr = (VerifyItemC * max(k, 1))()
    keep = []
    for i, item in enumerate(items):
        vix, proof = item[0], item[1]
        public = item[2] if len(item) > 2 else None
        prev = item[3] if len(item) > 3 else ()
        arr[i].index = vix._h.value if vix is not None else None
        arr[i].proof = proof._h.value if proof is not None else None
        if public is not None and len(public):
            pub = _c64(public, (-1, 4)); keep.append(pub)
            arr[i].public_inputs = _p64(pub); arr[i].n_public = pub.shape[0]
        m = len(prev)
        if m:
            chals = _c64(np.concatenate([np.asarray(c, dtype=np.uint64).reshape(-1, 4) for c, _ in prev]), (-1, 4))
            rounds = (C.c_uint * m)(*[np.asarray(c).reshape(-1, 4).shape[0] for c, _ in prev])
            cxy = np.ascontiguousarray(np.concatenate([np.asarray(cm[0], dtype=np.uint64).reshape(-1, 8) for _, cm in prev]))
            cinf = np.ascontiguousarray(np.concatenate([np.asarray(cm[1], dtype=np.uint8).reshape(-1) for _, cm in prev]))
            cch = (C.c_size_t * m)(*[np.asarray(cm[1]).reshape(-1).shape[0] for _, cm in prev])
            keep += [chals, rounds, cxy, cinf, cch]
            arr[i].prev_chals = _p64(chals); arr[i].prev_rounds = rounds; arr[i].prev_comm_xy = _p64(cxy); arr[i].prev_comm_inf = _p8(cinf)
            arr[i].prev_comm_chunks = cch; arr[i].n_prev = m
    rnd = _c64(rand, (2, 4)) if rand is not None else None
    ok = C.c_int(ok_before)
    tr = (VerifyTraceC * max(k, 1))()
    rc = _lib.kh_batch_verify(arr, k if count is None else count, _p64(rnd) if rnd is not None else None, C.byref(ok), tr)
    return rc, ok.value, [_trace(tr[i]) for i in range(k)] if rc == 0 else None


def batch_verify(items, rand=None):
    """kh_batch_verify: (ok, [trace dict per item]); a malformed item raises KhError (code E_INVALID).  rand: (2, 4) limbs (rand_base, sg_rand_base) or
    None (drawn from the operating system)."""
    rc, ok, tr = batch_verify_raw(items, rand)
    _check(rc)
    return ok == 1, tr


def verify(vix, proof, public=None, prev=()):
    """kh_verify: (ok, trace)"""
    ok, tr = batch_verify([(vix, proof, public, prev)])
    return ok, tr[0]


def verify_last_phase_seconds():
    """kh_verify_last_phase_seconds: {phase: seconds} of this thread's last batch_verify"""
    ph = (C.c_double * 4)()
    _check(min(0, _lib.kh_verify_last_phase_seconds(ph, 4)))
    return dict(zip(VERIFY_PHASES, list(ph)))


def polycomm_multi_scalar_mul(curve: int, comms, scalars):
    """comms: list of (chunks (k_i, 8) limbs, inf (k_i,) flags); scalars (m, 4).  Returns (chunks, inf)."""
    m = len(comms)
    counts = [np.asarray(c[0]).reshape(-1, 8).shape[0] for c in comms]
    xy = np.concatenate([np.asarray(c[0], dtype=np.uint64).reshape(-1, 8) for c in comms]) if m else np.zeros((0, 8), np.uint64)
    inf = np.concatenate([np.asarray(c[1], dtype=np.uint8).reshape(-1) for c in comms]) if m else np.zeros(0, np.uint8)
    xy = np.ascontiguousarray(xy); inf = np.ascontiguousarray(inf)
    sc = _c64(scalars, (-1, 4))
    width = max(counts + [1])
    out = np.zeros((width, 8), dtype=np.uint64); oinf = np.zeros(width, dtype=np.uint8)
    cnt = C.c_size_t(0)
    nc = (C.c_size_t * max(m, 1))(*counts)
    _check(_lib.kh_polycomm_multi_scalar_mul(curve, _p64(xy), _p8(inf), nc, m, _p64(sc), _p64(out), _p8(oinf), C.byref(cnt)))
    return out[:cnt.value], oinf[:cnt.value]


def combine_polys_dev(field: int, polys, lens, num_chunks, polyscale, srs_length: int, out):
    """polys: list of DevBuf; out: DevBuf of srs_length elements.  Returns the length of the combined polynomial."""
    m = len(polys)
    ptrs = (C.c_void_p * max(m, 1))(*[C.c_void_p(p.ptr) for p in polys])
    ls = (C.c_size_t * max(m, 1))(*lens); cs = (C.c_size_t * max(m, 1))(*num_chunks)
    ol = C.c_size_t(0)
    _check(_lib.kh_combine_polys_dev(field, ptrs, ls, cs, m, _p64(_c64(polyscale, (4,))), srs_length, C.c_void_p(out.ptr), C.byref(ol)))
    return ol.value


def poly_lincomb_dev(field: int, polys, lens, scalars, out, out_len: int):
    m = len(polys)
    ptrs = (C.c_void_p * max(m, 1))(*[C.c_void_p(p.ptr) for p in polys])
    ls = (C.c_size_t * max(m, 1))(*lens)
    _check(_lib.kh_poly_lincomb_dev(field, ptrs, ls, _p64(_c64(scalars, (-1, 4))), m, C.c_void_p(out.ptr), out_len))


def b_init_dev(field: int, elm, evalscale, padded_len: int, out):
    e = _c64(elm, (-1, 4))
    _check(_lib.kh_b_init_dev(field, _p64(e), e.shape[0], _p64(_c64(evalscale, (4,))), padded_len, C.c_void_p(out.ptr)))


def evaluate_chunks_dev(field: int, coeffs, length: int, chunk_size: int, num_chunks: int, points):
    pts = _c64(points, (-1, 4))
    out = np.zeros((pts.shape[0], num_chunks, 4), dtype=np.uint64)
    _check(_lib.kh_evaluate_chunks_dev(field, C.c_void_p(coeffs.ptr), length, chunk_size, num_chunks, _p64(pts), pts.shape[0], _p64(out)))
    return out


def evaluate_chunks_batch_dev(field: int, polys, lens, num_chunks, chunk_size: int, points):
    """Returns a list of (npts, num_chunks[j], 4) arrays, one per polynomial."""
    pts = _c64(points, (-1, 4)); m = len(polys)
    ptrs = (C.c_void_p * max(m, 1))(*[C.c_void_p(p.ptr) for p in polys])
    ls = (C.c_size_t * max(m, 1))(*lens); cs = (C.c_size_t * max(m, 1))(*num_chunks)
    out = np.zeros((pts.shape[0] * sum(num_chunks), 4), dtype=np.uint64)
    _check(_lib.kh_evaluate_chunks_batch_dev(field, ptrs, ls, cs, m, chunk_size, _p64(pts), pts.shape[0], _p64(out)))
    res, pos = [], 0
    for c in num_chunks:
        res.append(out[pos:pos + pts.shape[0] * c].reshape(pts.shape[0], c, 4)); pos += pts.shape[0] * c
    return res


def divide_by_vanishing_poly_dev(field: int, f, length: int, log2_n: int, q, r):
    _check(_lib.kh_divide_by_vanishing_poly_dev(field, C.c_void_p(f.ptr), length, log2_n, C.c_void_p(q.ptr if q is not None else 0), C.c_void_p(r.ptr)))


def b_poly_coefficients(field: int, chals, rounds: int):
    """chals: (k * rounds, 4) Montgomery limbs -> (k, 2^rounds, 4)."""
    ch = _c64(chals, (-1, 4))
    k = ch.shape[0] // rounds if rounds else 1
    out = np.zeros((k, 1 << rounds, 4), dtype=np.uint64)
    _check(_lib.kh_b_poly_coefficients(field, _p64(ch), rounds, k, _p64(out)))
    return out


def batch_dlog_accumulator_generate(srs, num_comms: int, chals):
    ch = _c64(chals, (-1, 4))
    out = np.zeros((num_comms, 8), dtype=np.uint64); inf = np.zeros(num_comms, dtype=np.uint8)
    _check(_lib.kh_batch_dlog_accumulator_generate(srs._h, num_comms, _p64(ch), ch.shape[0], _p64(out), _p8(inf)))
    return out, inf


def batch_dlog_accumulator_check(srs, comms, chals, r, inf=None) -> bool:
    cm = _c64(comms, (-1, 8)); ch = _c64(chals, (-1, 4)); r = _c64(r, (4,))
    if inf is None:
        inf = np.zeros(cm.shape[0], dtype=np.uint8)
    ok = C.c_int(0)
    _check(_lib.kh_batch_dlog_accumulator_check(srs._h, _p64(cm), _p8(inf), cm.shape[0], _p64(ch), ch.shape[0], _p64(r), C.byref(ok)))
    return bool(ok.value)


def ipa_verify_msm(srs, chals, sg_weights, extra_xy, extra_scalars, extra_inf=None) -> bool:
    ch = _c64(chals, (-1, 4)); w = _c64(sg_weights, (-1, 4)); ex = _c64(extra_xy, (-1, 8)); es = _c64(extra_scalars, (-1, 4))
    if extra_inf is None:
        extra_inf = np.zeros(ex.shape[0], dtype=np.uint8)
    z = C.c_int(0)
    _check(_lib.kh_ipa_verify_msm(srs._h, _p64(ch), ch.shape[0], _p64(w), w.shape[0], _p64(ex), _p8(np.ascontiguousarray(extra_inf, dtype=np.uint8)),
                                  _p64(es), ex.shape[0], C.byref(z)))
    return bool(z.value)


def _chal_limbs(chal: int):
    return np.array([chal & (2**64 - 1), (chal >> 64) & (2**64 - 1)], dtype=np.uint64)


def scalar_challenge_to_field(curve: int, chal: int):
    out = np.zeros(4, dtype=np.uint64)
    _check(_lib.kh_scalar_challenge_to_field(curve, _p64(_chal_limbs(chal)), _p64(out)))
    return out


class IpaOpening:
    """The folding loop of SRS::open (ipa.rs:929-1007) on device-resident vectors; see include/kimchi_hip.h."""

    def __init__(self, srs, a, b, u_base, a_len: int = None, b_len: int = None):
        """a, b: host limb arrays, or DevBuf objects with a_len / b_len elements (kh_ipa_begin_dev)."""
        u_base = _c64(u_base, (8,))
        h = C.c_void_p()
        if isinstance(a, DevBuf):
            _check(_lib.kh_ipa_begin_dev(srs._h, C.c_void_p(a.ptr), a_len, C.c_void_p(b.ptr), b_len, _p64(u_base), C.byref(h)))
        else:
            a = _c64(a, (-1, 4)); b = _c64(b, (-1, 4))
            _check(_lib.kh_ipa_begin(srs._h, _p64(a), a.shape[0], _p64(b), b.shape[0], _p64(u_base), C.byref(h)))
        self._h = h

    def rounds_left(self) -> int:
        return _lib.kh_ipa_rounds_left(self._h)

    def round_lr(self, rand_l, rand_r):
        rand_l = _c64(rand_l, (4,)); rand_r = _c64(rand_r, (4,))
        xy = np.zeros((2, 8), dtype=np.uint64); inf = np.zeros(2, dtype=np.uint8)
        _check(_lib.kh_ipa_round_lr(self._h, _p64(rand_l), _p64(rand_r), _p64(xy), _p8(inf)))
        return xy, inf

    def round_fold(self, chal: int):
        u = np.zeros(4, dtype=np.uint64); ui = np.zeros(4, dtype=np.uint64)
        _check(_lib.kh_ipa_round_fold(self._h, _p64(_chal_limbs(chal)), _p64(u), _p64(ui)))
        return u, ui

    def finish(self):
        a0 = np.zeros(4, dtype=np.uint64); b0 = np.zeros(4, dtype=np.uint64)
        sg = np.zeros(8, dtype=np.uint64); inf = np.zeros(1, dtype=np.uint8)
        _check(_lib.kh_ipa_finish(self._h, _p64(a0), _p64(b0), _p64(sg), _p8(inf)))
        return a0, b0, sg, bool(inf[0])

    def free(self):
        if self._h:
            _lib.kh_ipa_free(self._h); self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def ipa_open(srs, a_dev, b_dev, n: int, combined_inner_product, blinding_factor, sponge, blinders):
    """kh_ipa_open: the rounds and the Schnorr tail of SRS::open in one native call.  Returns (lr_xy (k, 2, 8), lr_inf (k, 2),
    delta_xy, delta_inf, z1, z2, sg_xy, sg_inf)."""
    bl = _c64(blinders, (-1, 4))
    k = (bl.shape[0] - 2) // 2
    lr = np.zeros((k, 2, 8), dtype=np.uint64); lri = np.zeros((k, 2), dtype=np.uint8)
    delta = np.zeros(8, dtype=np.uint64); dinf = np.zeros(1, dtype=np.uint8)
    z1 = np.zeros(4, dtype=np.uint64); z2 = np.zeros(4, dtype=np.uint64)
    sg = np.zeros(8, dtype=np.uint64); sginf = np.zeros(1, dtype=np.uint8)
    _check(_lib.kh_ipa_open(srs._h, C.c_void_p(a_dev.ptr), n, C.c_void_p(b_dev.ptr), n, _p64(_c64(combined_inner_product, (4,))), _p64(_c64(blinding_factor, (4,))),
                            sponge._h, _p64(bl), bl.shape[0], _p64(lr), _p8(lri), _p64(delta), _p8(dinf), _p64(z1), _p64(z2), _p64(sg), _p8(sginf)))
    return lr, lri, delta, bool(dinf[0]), z1, z2, sg, bool(sginf[0])


def endos(curve: int):
    """(endo_q, endo_r) as Montgomery limb arrays; host-only."""
    q = np.zeros(4, dtype=np.uint64); r = np.zeros(4, dtype=np.uint64)
    _check(_lib.kh_endos(curve, _p64(q), _p64(r)))
    return q, r


def domain_generator(field: int, log2_n: int):
    out = np.zeros(4, dtype=np.uint64)
    _check(_lib.kh_domain_generator(field, log2_n, _p64(out)))
    return out


def permutation_shifts(field: int, log2_n: int):
    """kh_permutation_shifts: Shifts::new for 2^log2_n rows, (7, 4) Montgomery limbs (host code, no device)."""
    out = np.zeros((7, 4), dtype=np.uint64)
    _check(_lib.kh_permutation_shifts(field, log2_n, _p64(out)))
    return out


class Sponge:
    """kh_sponge_*: the host-side Fiat-Shamir sponges (FQ: DefaultFqSponge of `curve`, FR: DefaultFrSponge of `curve`)."""
    FQ, FR = _CONSTANTS["KH_SPONGE_FQ"], _CONSTANTS["KH_SPONGE_FR"]

    def __init__(self, kind: int, curve: int, _h=None):
        self.kind, self.curve = kind, curve
        self._h = C.c_void_p()
        if _h is None:
            _check(_lib.kh_sponge_new(kind, curve, C.byref(self._h)))
        else:
            self._h = _h

    def clone(self):
        h = C.c_void_p()
        _check(_lib.kh_sponge_clone(self._h, C.byref(h)))
        return Sponge(self.kind, self.curve, h)

    def absorb_g(self, xy, inf=None):
        xy = _c64(xy, (-1, 8))
        i8 = None if inf is None else np.ascontiguousarray(inf, dtype=np.uint8)
        _check(_lib.kh_sponge_absorb_g(self._h, _p64(xy), _p8(i8), xy.shape[0]))

    def absorb(self, x):
        x = _c64(x, (-1, 4))
        _check(_lib.kh_sponge_absorb(self._h, _p64(x), x.shape[0]))

    def absorb_fr(self, x):
        x = _c64(x, (-1, 4))
        _check(_lib.kh_sponge_absorb_fr(self._h, _p64(x), x.shape[0]))

    def challenge(self) -> int:
        c = np.zeros(2, dtype=np.uint64)
        _check(_lib.kh_sponge_challenge(self._h, _p64(c)))
        return int(c[0]) | (int(c[1]) << 64)

    def challenge_field(self):
        out = np.zeros(4, dtype=np.uint64)
        _check(_lib.kh_sponge_challenge_field(self._h, _p64(out)))
        return out

    def squeeze_field(self):
        out = np.zeros(4, dtype=np.uint64)
        _check(_lib.kh_sponge_squeeze_field(self._h, _p64(out)))
        return out

    def digest(self):
        out = np.zeros(4, dtype=np.uint64)
        _check(_lib.kh_sponge_digest(self._h, _p64(out)))
        return out

    def free(self):
        if self._h:
            _lib.kh_sponge_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def sync():
    _check(_lib.kh_sync())


def last_timings():
    names = (C.c_char_p * 32)()
    ms = (C.c_float * 32)()
    n = _lib.kh_last_timings(names, ms, 32)
    return [(names[i].decode(), float(ms[i])) for i in range(n)]


def debug_field_op(field: int, op: str, a, b=None):
    ops = {"mul": 0, "add": 1, "sub": 2, "to_mont": 3, "from_mont": 4, "sqr": 5, "neg": 6,
           "mul29": 7, "sqr29": 8, "pack29": 9, "mul29_32x": 10}      # field29.cuh (nine 29-bit limbs, lazy reduction)
    a = _c64(a, (-1, 4))
    bb = None if b is None else _c64(b, (-1, 4))
    out = np.zeros_like(a)
    _check(_lib.kh_debug_field_op(field, ops[op], _p64(a), None if bb is None else _p64(bb), _p64(out), a.shape[0]))
    return out


def debug_field29_op(field: int, op: str, spread: str, a, b, c):
    """mulsub29 / sqrsub29 (field29.cuh) on limbs as given: (n, 9) uint32 each, b None for sqrsub29; spread "s71", "s51" or "s44"."""
    U32P = C.POINTER(C.c_uint32)
    a, c = (np.ascontiguousarray(v, dtype=np.uint32).reshape(-1, 9) for v in (a, c))
    b = None if b is None else np.ascontiguousarray(b, dtype=np.uint32).reshape(-1, 9)
    out = np.zeros_like(a)
    _check(_lib.kh_debug_field29_op(field, {"mulsub29": 0, "sqrsub29": 1}[op], {"s71": 0, "s51": 1, "s44": 2}[spread], a.ctypes.data_as(U32P),
                                    None if b is None else b.ctypes.data_as(U32P), c.ctypes.data_as(U32P), out.ctypes.data_as(U32P), a.shape[0]))
    return out


def debug_point_op(curve: int, op: int, p, q, p_inf=None, q_inf=None):
    p = _c64(p, (-1, 8)); q = _c64(q, (-1, 8))
    n = p.shape[0]
    pi = None if p_inf is None else np.ascontiguousarray(p_inf, dtype=np.uint8)
    qi = None if q_inf is None else np.ascontiguousarray(q_inf, dtype=np.uint8)
    out = np.zeros((n, 8), dtype=np.uint64)
    oinf = np.zeros(n, dtype=np.uint8)
    _check(_lib.kh_debug_point_op(curve, op, _p64(p), _p8(pi), _p64(q), _p8(qi), _p64(out), _p8(oinf), n))
    return out, oinf


def debug_bucket_tail(curve: int, tail: int, fin: int, c_or_nb: int, m: int, groups: int, buckets):
    """kh_debug_bucket_tail: one reduction tail of the MSM over `groups` arrays of XYZZ records, (groups * nb, 16) uint64.  tail 0 / 1 / 2: k_marginals /
    _q / _h and k_marginal_fin (fin 0) or _fin_q (fin 1) at window width c_or_nb -> (groups, 3, 8) affine plane sums and (groups, 3) infinity bytes;
    tail 3: the segment kernels over nb = c_or_nb buckets in segments of m -> (groups, 8) and (groups,)."""
    b = _c64(buckets, (-1, 16))
    shape = (groups,) if tail == 3 else (groups, 3)
    out = np.zeros(shape + (8,), dtype=np.uint64)
    oinf = np.zeros(shape, dtype=np.uint8)
    nb = c_or_nb if tail == 3 else 1 << max(c_or_nb - 1, 0)
    if b.shape[0] != groups * nb:
        raise ValueError(f"{b.shape[0]} records for {groups} groups of {nb} buckets")
    _check(_lib.kh_debug_bucket_tail(curve, tail, fin, c_or_nb, m, groups, _p64(b), _p64(out), _p8(oinf)))
    return out, oinf


def debug_bucket_sums(curve: int, kind: int, toff, partial):
    """kh_debug_bucket_sums: bucket i = the sum of the XYZZ records partial[toff[i]:toff[i + 1]] ((n, 16) uint64) by k_bucket_sum with SMALL_NT 4 (kind 0) or 16
    (kind 1) or by k_bucket_sum_q (kind 2), each with k_bucket_chunk and k_bucket_big behind it -> (nkeys, 8) affine and (nkeys,) infinity bytes."""
    t = np.ascontiguousarray(toff, dtype=np.uint32)
    nkeys = t.shape[0] - 1
    p = _c64(partial, (-1, 16))
    if nkeys < 1 or p.shape[0] != int(t[-1]):
        raise ValueError(f"{p.shape[0]} records for offsets that end at {int(t[-1]) if t.size else None}")
    out = np.zeros((nkeys, 8), dtype=np.uint64)
    oinf = np.zeros(nkeys, dtype=np.uint8)
    _check(_lib.kh_debug_bucket_sums(curve, kind, nkeys, t.ctypes.data_as(C.POINTER(C.c_uint32)), _p64(p), _p64(out), _p8(oinf)))
    return out, oinf


MsmSortArgsC, MsmSortEchoC, MsmSortOutC = _STRUCTURES["kh_msm_sort_args_t"], _STRUCTURES["kh_msm_sort_echo_t"], _STRUCTURES["kh_msm_sort_out_t"]


def debug_msm_sort(curve: int, scalars, k: int = 1, mont: bool = False, inf=None, offset: int = 0, stride: int = 0, batch_stride: int = 0, precomp_c: int = 0,
                   glv: bool = False, wide: bool = False, fused_off: bool = False, stage_entries: int = 28672, stage_maxpass: int = 2, num_cus: int = 0,
                   echo_only: bool = False):
    """kh_debug_msm_sort: digits, sort and task plan of one job over `scalars` ((k * n, 4) uint64), nothing behind them.  Two calls: the first returns the
    plan's echo, which sizes the outputs of the second.  -> dict: the echo's fields (ktab as a uint8 array), and unless echo_only: digits (k, W, n) int32,
    off, toff, entries[:off[nkeys]], counts (8,), order / rnt / roff where ranked == 1, and for wide plans order, ptot, xpairs (counts[3], 2), slist,
    big_keys, big_arrivals, b29_zero."""
    sc = _c64(scalars, (-1, 4))
    n = sc.shape[0] // k if k > 0 else 0                   # (k = 0 goes through: the library refuses it)
    if k > 0 and n * k != sc.shape[0]:
        raise ValueError(f"{sc.shape[0]} scalars for {k} MSMs")
    a = MsmSortArgsC(curve=curve, mont=int(bool(mont)), n=n, k=k, scalars=_p64(sc), offset=offset, stride=stride, batch_stride=batch_stride, precomp_c=precomp_c,
                     glv=int(bool(glv)), wide=int(bool(wide)), fused_off=int(bool(fused_off)), stage_entries=stage_entries, stage_maxpass=stage_maxpass, num_cus=num_cus)
    if inf is not None:
        inf = np.ascontiguousarray(inf, dtype=np.uint8)
        a.inf, a.inf_len = _p8(inf), inf.size
    e = MsmSortEchoC()
    _check(_lib.kh_debug_msm_sort(C.byref(a), C.byref(e), None))
    res = {f: getattr(e, f) for f, _t in MsmSortEchoC._fields_ if f != "ktab"}
    res["ktab"] = np.array(list(e.ktab), np.uint8)
    if echo_only:
        return res
    U32P = C.POINTER(C.c_uint32)
    nkeys, W = e.nkeys, e.W
    sizes = {"digits": k * W * n, "off": nkeys + 1, "entries": e.max_entries, "toff": nkeys + 1, "counts": 8}
    if e.ranked == 1:
        sizes.update(order=nkeys, rnt=nkeys + 1, roff=nkeys + 1)
    if e.wide:
        sizes.update(order=nkeys, ptot=256 * k, xpairs=2 * e.max_tasks, slist=nkeys, big_keys=nkeys, big_arrivals=nkeys)
    bufs = {name: np.zeros(size, np.uint32) for name, size in sizes.items()}
    o = MsmSortOutC(**{name: b.ctypes.data_as(U32P) for name, b in bufs.items()})
    if e.wide:
        bufs["b29_zero"] = np.zeros(nkeys, np.uint8)
        o.b29_zero = _p8(bufs["b29_zero"])
    e2 = MsmSortEchoC()
    _check(_lib.kh_debug_msm_sort(C.byref(a), C.byref(e2), C.byref(o)))
    if bytes(e2) != bytes(e):
        raise KhError("kh_debug_msm_sort: the plan changed between the sizing call and the run")
    cnt = bufs["counts"]
    res.update(bufs)
    res["digits"] = bufs["digits"].view(np.int32).reshape(k, W, n)
    res["entries"] = bufs["entries"][:min(int(cnt[5]), e.max_entries)]
    if e.wide:
        res["xpairs"] = bufs["xpairs"][:2 * min(int(cnt[3]), e.max_tasks)].reshape(-1, 2)
        res["slist"] = bufs["slist"][:min(int(cnt[4]), nkeys)]
        res["big_keys"] = bufs["big_keys"][:min(int(cnt[1]), nkeys)]
        res["big_arrivals"] = bufs["big_arrivals"][:min(int(cnt[1]), nkeys)]
    return res
