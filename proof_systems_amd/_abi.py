"""include/kimchi_hip.h as plain data: the one parser of the header.  khip.py declares the ctypes binding from it at import and
tools/gen_rust_sys.py renders the Rust -sys crate from it, so a new entry point is written once, in the header.  Needs neither
ctypes nor the library."""
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kimchi_hip.h")

_NAME = r"[A-Za-z_][A-Za-z0-9_]*"


def parse(path=HEADER):
    """(prototypes, structs, constants), each in the header's order:
    prototypes  {name: (return type, [(C type, parameter name)])}; an array parameter `uint64_t out[4]` has the type `uint64_t *`
    structs     {name: [(field, C type, [array dimensions])]} of the records a caller fills in, under their typedef names
    constants   {name: int} of the `#define KH_*` lines, then of the anonymous enums (token opcodes, scan operators)"""
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    prototypes = {}
    for ret, name, args in re.findall(r"([A-Za-z_][A-Za-z0-9_ \*]*?)\b(kh_[a-z_0-9]+)\s*\(([^;{}]*?)\)\s*;", src):
        args = " ".join(args.split())
        params = []
        for decl in [] if args in ("", "void") else args.split(","):
            m = re.match(r"(.*?)(%s)\s*(\[\d*\])?$" % _NAME, decl.strip())
            params.append((m.group(1).strip() + (" *" if m.group(3) else ""), m.group(2)))
        prototypes[name] = (ret.strip(), params)
    structs = {}
    # `typedef struct [tag] { ... } kh_name_t;`, or `struct kh_name { ... };` with its `typedef struct kh_name kh_name_t;` elsewhere
    later = dict(re.findall(r"typedef\s+struct\s+(kh_[a-z_0-9]+)\s+(kh_[a-z_0-9]+)\s*;", src))
    records = re.findall(r"(?:typedef\s+)?struct\s*(kh_[a-z_0-9]+)?\s*\{([^}]*)\}\s*(kh_[a-z_0-9]+)?\s*;", src)
    for body, name in [(b, n or later[tag]) for tag, b, n in records]:
        declarator = _NAME + r"(?:\s*\[\d+\])*"                                   # a field, or an array field: entry[3][4]
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            m = re.match(r"(.*?)(%s(?:\s*,\s*%s)*)$" % (declarator, declarator), decl)
            for f in m.group(2).split(","):
                fields.append((re.match(_NAME, f.strip()).group(), m.group(1).strip(), [int(d) for d in re.findall(r"\[(\d+)\]", f)]))
        structs[name] = fields
    constants = re.findall(r"#define\s+(KH_[A-Z0-9_]+)\s+\(?(-?\d+)\)?", src)
    for body in re.findall(r"enum\s*\{([^}]*)\}", src):
        constants += re.findall(r"(KH_[A-Z0-9_]+)\s*=\s*(-?\d+)", body)
    return prototypes, structs, {name: int(value) for name, value in constants}
