"""The one reader of include/finenv.h for the tests: its prototypes, structs and constants, and the ctypes
declaration each of them calls for.  The header is regular C, so a few regexes read it; every function
takes the header text as an optional argument so that a test can hand in an edited copy."""
import ctypes as C
import functools
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "finenv.h")

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64,
           "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}


@functools.lru_cache(maxsize=None)
def source():
    """The header as written, comments included (for the tests that hold its prose to something)."""
    with open(HEADER) as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def text(src=None):
    """The header without its comments (src: header text, default the file)."""
    return re.sub(r"/\*.*?\*/|//[^\n]*", " ", source() if src is None else src, flags=re.S)


def _decl(decl):
    """'const float  * obs' -> ('const float *', 'obs'): single spaces, one before the stars."""
    m = re.fullmatch(r"\s*(.*?)(\w+)\s*", decl, flags=re.S)
    words = m.group(1).replace("*", " * ").split()
    return (" ".join(w for w in words if w != "*") + " " + "*" * words.count("*")).strip(), m.group(2)


@functools.lru_cache(maxsize=None)
def prototypes(src=None):
    """{function: (return type, [(argument type, argument name), ...])} in header order."""
    out = {}
    for ret, name, args in re.findall(r"^([a-z][\w \t]*?[ \t*]+)(finenv_\w+)\s*\(([^)]*)\)\s*;", text(src),
                                      flags=re.M):
        assert name not in out, f"{name} is declared twice"
        args = [] if args.strip() == "void" else [_decl(a) for a in args.split(",")]
        out[name] = (_decl(ret + "_")[0], args)
    return out


@functools.lru_cache(maxsize=None)
def structs(src=None):
    """{struct: [(field type, field name), ...]} of every `typedef struct finenv_x { ... } finenv_x;`."""
    out = {}
    for name, body, alias in re.findall(r"typedef\s+struct\s+(finenv_\w+)\s*\{(.*?)\}\s*(\w+)\s*;", text(src),
                                        flags=re.S):
        assert name == alias and name not in out, name
        out[name] = []
        for decl in filter(str.strip, body.split(";")):          # `double a, b;` declares two fields
            first, *more = decl.split(",")
            ctype, field = _decl(first)
            out[name] += [(ctype, field)] + [_decl(ctype.rstrip(" *") + " " + m) for m in more]
    return out


@functools.lru_cache(maxsize=None)
def opaque(src=None):
    """The handle types: `typedef struct finenv_x finenv_x;`."""
    return {a for a, b in re.findall(r"typedef\s+struct\s+(finenv_\w+)\s+(finenv_\w+)\s*;", text(src)) if a == b}


@functools.lru_cache(maxsize=None)
def enums(src=None):
    """Every `enum { ... };` as a list of (name, value) in order."""
    out = []
    for body in re.findall(r"\benum\s*\{(.*?)\}\s*;", text(src), flags=re.S):
        items, nxt = [], 0
        for item in filter(None, (i.strip() for i in body.split(","))):
            name, _, value = (p.strip() for p in item.partition("="))
            nxt = int(value, 0) if value else nxt
            items.append((name, nxt))
            nxt += 1
        out.append(items)
    return out


@functools.lru_cache(maxsize=None)
def constants(src=None):
    """{name: int} of every enumerator and every `#define FINENV_X <int>`."""
    out = {}
    for name, value in [i for e in enums(src) for i in e] + \
            [(n, int(v, 0)) for n, v in re.findall(r"^[ \t]*#define[ \t]+(FINENV_\w+)[ \t]+(-?\w+)[ \t]*$",
                                                   text(src), flags=re.M)]:
        assert name not in out, f"{name} is defined twice"
        out[name] = value
    return out


def enum(count_name, src=None):
    """The enumerator names, in order, of the enum that `count_name` closes (count_name is the last one).
    The values must count up from 0."""
    (found,) = [e for e in enums(src) if e[-1][0] == count_name]
    assert [v for _, v in found] == list(range(len(found))), f"{count_name}: values do not count from 0"
    return [n for n, _ in found]


def fields(count_name, src=None):
    """The lower-case field names of that enum without their FINENV_<XX>_ prefix:
    fields('FINENV_STOCK_F64_FIELDS') -> ('cash', 'cost', ...)."""
    names = enum(count_name, src)[:-1]
    prefixes = {re.match(r"FINENV_[A-Z0-9]+_", n).group() for n in names}
    assert len(prefixes) == 1, f"{count_name}: mixed prefixes {sorted(prefixes)}"
    (prefix,) = prefixes
    return tuple(n[len(prefix):].lower() for n in names)


def expected_ctype(ctype, classes, handles, ret=False):
    """The rule of the binding: the ctypes class a C type is declared as.  `classes` maps a struct's C
    name to its ctypes class, `handles` is opaque()."""
    base, stars = ctype.replace("const ", "").rstrip(" *"), ctype.count("*")
    if ret and ctype in ("void", "const char *"):
        return None if ctype == "void" else C.c_char_p
    if stars == 0:
        return SCALARS[base]
    if base in handles and stars <= 2:
        return C.c_void_p if stars == 1 else C.POINTER(C.c_void_p)
    if base in classes and stars == 1:
        return C.POINTER(classes[base])
    return C.c_void_p


def expected_signature(name, classes, src=None):
    """(restype, argtypes) the rule gives function `name`."""
    ret, args = prototypes(src)[name]
    handles = opaque(src)
    return (expected_ctype(ret, classes, handles, ret=True),
            [expected_ctype(t, classes, handles) for t, _ in args])


def expected_fields(name, src=None):
    """The ctypes _fields_ the rule gives struct `name`: a pointer is c_void_p, a scalar its class."""
    return [(f, C.c_void_p if t.endswith("*") else SCALARS[t]) for t, f in structs(src)[name]]


# finrl_amd._native's tuples of field names; tuple X mirrors the enum that FINENV_X closes
FIELD_TUPLES = ("STOCK_F64_FIELDS", "STOCK_I32_FIELDS", "STOCK_LAST_FIELDS", "STOCK_HISTORY_METRICS",
                "PORTFOLIO_F64_FIELDS", "PORTFOLIO_I32_FIELDS", "PORTFOLIO_LAST_FIELDS",
                "CRYPTO_F64_FIELDS", "CRYPTO_I32_FIELDS", "STOCKNP_F64_FIELDS", "STOCKNP_I32_FIELDS",
                "CASHPENALTY_F64_FIELDS", "CASHPENALTY_I32_FIELDS", "STOPLOSS_F64_FIELDS", "STOPLOSS_BOOKS",
                "STOPLOSS_I32_FIELDS", "BTC_F64_FIELDS", "BTC_I32_FIELDS")


def _names(xs):
    return [getattr(x, "__name__", x) for x in xs]


def binding_errors(nat, src=None):
    """Every disagreement between the tables of finrl_amd._native (`nat`) and the header, one message
    each, beginning with the function, struct or tuple it is about."""
    errs = []
    protos, decls = prototypes(src), structs(src)
    classes = {cname: cls for cname, _, cls in nat.STRUCTS}
    for table, mine, theirs in (("SIGNATURES", nat.SIGNATURES, protos), ("STRUCTS", classes, decls)):
        errs += [f"{n}: in the header, not in {table}" for n in theirs if n not in mine]
        errs += [f"{n}: in {table}, not in the header" for n in mine if n not in theirs]
    for name in protos:
        if name in nat.SIGNATURES:
            (res, args), (want_res, want_args) = nat.SIGNATURES[name], expected_signature(name, classes, src)
            if res is not want_res or list(args) != want_args:
                errs.append(f"{name}: the header gives {_names([want_res] + want_args)}, "
                            f"SIGNATURES {_names([res] + list(args))}")
    for name in decls:
        if name in classes and classes[name]._fields_ != expected_fields(name, src):
            errs.append(f"{name}: the header gives {[(f, t.__name__) for f, t in expected_fields(name, src)]}, "
                        f"{classes[name].__name__} {[(f, t.__name__) for f, t in classes[name]._fields_]}")
    for tup in FIELD_TUPLES:
        if getattr(nat, tup) != fields("FINENV_" + tup, src):
            errs.append(f"{tup}: the header gives {fields('FINENV_' + tup, src)}, the binding {getattr(nat, tup)}")
    return errs
