"""What the host tests share about the C ABI: the text and the prototypes of a header of include/, an entry of the built library bound the way the
registry (crnerf_amd._lib.HEADER_SIGNATURES) says, and check_header, which holds one header's table to its prototypes parameter by parameter."""
import ctypes
import os
import re

from crnerf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
UNORDERED = {"crnerf.h"}          # its table is not in header order: compared as a set

SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64,
           "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
RESTYPES = dict(SCALARS, **{"constchar*": ctypes.c_char_p})
# The parameters the type rule of expected_argtype does not cover: host arrays ctypes converts itself.
HOST_FLOATS = [("crnerf_rays_from_directions_f32", "c2w_host"), ("crnerf_generate_rays_f32", "intrinsics_host"), ("crnerf_generate_rays_f32", "c2w_host"),
               ("crnerf_generate_rays_fmanorm_f32", "intrinsics_host"), ("crnerf_generate_rays_fmanorm_f32", "c2w_host")]
EXCEPTIONS = dict([(k, ctypes.POINTER(ctypes.c_float)) for k in HOST_FLOATS]
                  + [(("crnerf_peer_window_create", "handle_out64"), ctypes.c_char_p), (("crnerf_peer_window_open", "handle64"), ctypes.c_char_p),
                     (("crnerf_peer_window_status", "status"), ctypes.POINTER(ctypes.c_int))])


def header_text(name):
    with open(os.path.join(INCLUDE, name)) as f:
        return f.read()


def _code(text):
    """`text` without its comments, both styles."""
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def prototypes(name):
    """{symbol: (return type, [parameter declarations])} of every prototype of include/`name`, in header order; types without their blanks."""
    protos = {}
    for m in re.finditer(r"^\s*([A-Za-z_][\w\s\*]*?)\b(crnerf_\w+)\s*\(([^)]*)\)\s*;", _code(header_text(name)), flags=re.M):
        params = [" ".join(p.split()) for p in m.group(3).split(",")]
        protos[m.group(2)] = ("".join(m.group(1).split()), [] if params in ([""], ["void"]) else params)
    return protos


def structs():
    """{C name: ctypes.Structure subclass} of every struct _lib declares; the class's docstring names the C struct."""
    found = {}
    for cls in vars(_lib).values():
        if isinstance(cls, type) and issubclass(cls, ctypes.Structure) and cls is not ctypes.Structure:
            found[re.search(r"struct (crnerf_\w+)", cls.__doc__).group(1)] = cls
    return found


def struct_fields(c_name):
    """[(type without blanks, field name, array length or None)] of `typedef struct ... c_name;`, looked for in every header."""
    for header in sorted(os.listdir(INCLUDE)):
        m = re.search(r"typedef struct(?: %s)? \{([^}]*)\} %s;" % (c_name, c_name), _code(header_text(header)))
        if m:
            break
    else:
        raise AssertionError("no header declares %s" % c_name)
    fields = []
    for decl in (d.strip() for d in m.group(1).split(";")):
        if decl:
            base, rest = re.match(r"((?:const\s+)?\w+)(.*)$", decl, flags=re.S).groups()
            for item in rest.split(","):
                stars, field, n = re.fullmatch(r"\s*([\s\*const]*?)\s*(\w+)\s*(?:\[(\d+)\])?\s*", item).groups()
                fields.append(("".join((base + stars).split()), field, int(n) if n else None))
    return fields


def expected_ctype(c_type):
    """The one ctypes type of a C type: a scalar by its width, `const crnerf_X*` the struct, an array of pointers, any other data pointer."""
    if "*" not in c_type:
        return SCALARS[c_type]
    if c_type.endswith("*const*") or c_type.endswith("**"):
        return ctypes.POINTER(ctypes.c_void_p)
    m = re.fullmatch(r"const(crnerf_\w+)\*", c_type)
    return ctypes.POINTER(structs()[m.group(1)]) if m else ctypes.c_void_p


def expected_argtype(symbol, decl):
    c_type, param = re.fullmatch(r"(.*?)(\w+)", decl).groups()
    return EXCEPTIONS.get((symbol, param)) or expected_ctype("".join(c_type.split()))


def check_header(name):
    """The table of `name` against the header: the same symbols (in the same order, but for crnerf.h), every return type, every parameter."""
    protos, table = prototypes(name), _lib.HEADER_SIGNATURES[name]
    assert sorted(protos) == sorted(table), set(protos) ^ set(table)
    if name not in UNORDERED:
        assert list(protos) == list(table)
    for symbol, (ret, params) in protos.items():
        restype, argtypes = table[symbol]
        assert restype is RESTYPES[ret], "%s returns %s, the table says %s" % (symbol, ret, restype)
        assert len(argtypes) == len(params), "%s: %d argtypes for %d parameters" % (symbol, len(argtypes), len(params))
        for k, (decl, argtype) in enumerate(zip(params, argtypes)):
            assert argtype is expected_argtype(symbol, decl), "%s, parameter %d (%s): the table says %s" % (symbol, k, decl, argtype)


def bound(name):
    """Entry `name` of the built library on a handle of its own, with the registry's restype / argtypes."""
    assert os.path.exists(_lib.LIB_PATH), "libcrnerf_hip.so missing: run __graft_entry__.build()"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, name), "%s is not exported" % name
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = _lib.ALL_SIGNATURES[name]
    return fn


def last_error():
    return bound("crnerf_last_error")()
