"""Reader of include/aerognn.h: the constants, structs and prototypes of the C-ABI as ctypes.

Not a C parser. It reads the subset the header uses between `extern "C" {` and its `}`: block
comments, `#define AGN_X <int>`, anonymous enums of `AGN_X = <int>`, `typedef struct { .. } agn_x;`
without nesting or bit-fields, and prototypes with named parameters. A pointer is c_void_p, except
a parameter that points to one of the header's structs in host memory (POINTER(ThatStruct)); a
parameter named `*_device` points to device memory and stays c_void_p. Any other declaration there
raises HeaderError with its line, so an edit outside the subset fails at import, on the CPU.
"""
import ctypes as C
import re

SCALARS = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "long": C.c_long,
           "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
POINTEES = set(SCALARS) | {"void", "char", "uint8_t", "unsigned long long"}  # and the header's structs

_INT = r"\(?\s*(-?\d+)\s*\)?"
_DEFINE = re.compile(r"#define\s+(AGN_\w+)\s+" + _INT)
_ENUM = re.compile(r"enum\s*\{(.*)\}", re.S)
_ENUM_ITEM = re.compile(r"(AGN_\w+)\s*=\s*" + _INT)
_STRUCT = re.compile(r"typedef\s+struct\s*\{([^{}]*)\}\s*(agn_\w+)")
_PROTO = re.compile(r"([\w\s]+?\*?)\s*\b(agn_\w+)\s*\(([^()]*)\)")
# [const] type [* [const]].. name [\[n\]]: a space or a star keeps the type and the name apart
_DECL = re.compile(r"(?:const\s+)?(\w+(?:\s+\w+)*?)\s*((?:\*\s*(?:const\s*)?)*)(?<!\w)(\w+)(?:\[(\w+)\])?")
_SPACE = re.compile(r"\s*")


class HeaderError(ValueError):
    pass


def camel(cname):
    """agn_mlp_fwd_args -> MlpFwdArgs"""
    return "".join(w.capitalize() for w in cname[4:].split("_"))


def parse(text, path="<header>"):
    """(constants {AGN_X: int}, structs {agn_x: ctypes.Structure class}, prototypes
    {agn_x: (restype, [argtypes])}) of a header text, each in the header's order."""
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group().count("\n"), text, flags=re.S)
    consts, structs, protos = {}, {}, {}

    def bad(pos, what):
        shown = " ".join(text[pos:].split(";")[0].split())[:80]
        raise HeaderError(f"{path}:{text.count(chr(10), 0, pos) + 1}: cannot read {what}: {shown!r}")

    def ctype(pos, base, stars, dim=None, untyped=False):
        if stars and (base in POINTEES or base in structs):
            t = C.POINTER(structs[base]) if base in structs and not untyped else C.c_void_p
        elif not stars and (base in SCALARS or base in structs):
            t = SCALARS.get(base) or structs[base]
        else:
            bad(pos, f"type {base!r} of")
        if dim is None:
            return t
        if not (dim.isdigit() or dim in consts):
            bad(pos, f"array length {dim!r} of")
        return t * int(consts.get(dim, dim))

    def fields(pos, body):
        out = []
        for m in re.finditer(r"\s*([^;]+);|\S", body):  # `int a, b;` declares two fields
            at = pos + (m.start(1) if m[1] else m.start())
            first, *more = (m[1] or "").split(",")
            d = _DECL.fullmatch(first.strip())
            if not d or not all(re.fullmatch(r"\s*\w+\s*", n) for n in more):
                bad(at, "field")
            out.append((d[3], ctype(at, d[1], d[2], d[4], untyped=True)))
            out += [(n.strip(), ctype(at, d[1], d[2], untyped=True)) for n in more]
        return out

    m = re.search(r'extern\s+"C"\s*\{', text)
    if not m:
        bad(0, 'a header without `extern "C" {`')
    pos = m.end()
    while True:
        pos = _SPACE.match(text, pos).end()
        if pos >= len(text):
            bad(pos, '`extern "C" {` without its `}`')
        if text[pos] == "}":
            return consts, structs, protos
        if text[pos] == "#":
            line = text[pos:].split("\n")[0].strip()
            d = _DEFINE.fullmatch(line)
            if d:
                consts[d[1]] = int(d[2])
            elif line not in ("#ifdef __cplusplus", "#endif"):
                bad(pos, "directive")
            pos += len(line)
            continue
        end, depth = pos, 0  # one statement: up to its `;` outside braces
        while end < len(text) and (text[end] != ";" or depth):
            depth += (text[end] == "{") - (text[end] == "}")
            end += 1
        stmt = text[pos:end].strip()
        if (m := _ENUM.fullmatch(stmt)):
            for item in m[1].split(","):
                e = _ENUM_ITEM.fullmatch(item.strip())
                if not e:
                    bad(pos, "enum item in")
                consts[e[1]] = int(e[2])
        elif (m := _STRUCT.fullmatch(stmt)):
            structs[m[2]] = type(camel(m[2]), (C.Structure,), {"_fields_": fields(pos + m.start(1), m[1])})
        elif (m := _PROTO.fullmatch(stmt)):
            ret = " ".join(m[1].split())
            if ret != "const char*" and ret not in SCALARS:
                bad(pos, f"return type {ret!r} of")
            args = []
            for p in ([] if m[3].strip() == "void" else m[3].split(",")):
                d = _DECL.fullmatch(p.strip())
                if not d or d[4]:
                    bad(pos, f"parameter {' '.join(p.split())!r} of")
                # a `*_device` table of structs is passed as a device address, not as a ctypes pointer
                args.append(ctype(pos, d[1], d[2], untyped=d[3].endswith("_device")))
            protos[m[2]] = (C.c_char_p if ret == "const char*" else SCALARS[ret], args)
        else:
            bad(pos, "declaration")
        pos = end + 1
