"""CPU tests: the C-ABI library loads and exports every symbol include/bp_c_api.h declares
(no compute without a GPU), and the host mirror fails loudly instead of falling back."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import geometry_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    """include/bp_c_api.h without its comments."""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bp_c_api.h")).read(), flags=re.S)


HEADER = _header()
PROTOTYPES = GC.api_prototypes(HEADER)
RETURNS = GC.api_return_types(HEADER)
DEFINES = {k: int(eval(v, {"__builtins__": {}})) for k, v in re.findall(r"^#define (BP_\w+) +(\S.*?)\s*$", HEADER, re.M)}
ENUMS = {k: int(v) for body in re.findall(r"enum\s*\{([^}]*)\}", HEADER) for k, v in re.findall(r"(BP_\w+)\s*=\s*(-?\d+)", body)}
# typedef struct NAME { body } NAME;  and the opaque  typedef struct NAME NAME;
STRUCT_BODIES = dict(re.findall(r"typedef struct (\w+) \{(.*?)\} \1;", HEADER, flags=re.S))
OPAQUE = re.findall(r"typedef struct (\w+) \1;", HEADER)
# C scalar -> (ctypes type, numpy format); size and natural alignment are ctypes.sizeof of it (pointers: those of void *)
SCALARS = {"int": (C.c_int, "i4"), "float": (C.c_float, "f4"), "double": (C.c_double, "f8"), "int64_t": (C.c_int64, "i8"),
           "uint64_t": (C.c_uint64, "u8"), "uint32_t": (C.c_uint32, "u4"), "unsigned": (C.c_uint32, "u4"), "size_t": (C.c_size_t, "u8"),
           "uint8_t": (C.c_uint8, "u1"), "unsigned char": (C.c_ubyte, "u1")}


def _declarator(text):
    """(base type, pointer depth, array length or None, name) of one C declarator with its type: const dropped, `x[n]` an array."""
    text = re.sub(r"\bconst\b", " ", text)
    depth = text.count("*")
    m = re.search(r"\[(\w+)\]", text)
    length = None if m is None else DEFINES[m.group(1)] if m.group(1) in DEFINES else int(m.group(1))
    words = re.sub(r"\[\w+\]", " ", text.replace("*", " ")).split()
    return " ".join(words[:-1]), depth, length, words[-1]


def _struct_fields(name):
    """[(field, base type, pointer depth, array length)] of a header struct, in order; `int a, *b;` shares its base type."""
    out = []
    for decl in STRUCT_BODIES[name].split(";"):
        if decl.strip():
            first, *rest = decl.split(",")
            base, depth, length, field = _declarator(first)
            out.append((field, base, depth, length))
            for r in rest:
                _, depth, length, field = _declarator(base + " " + r)
                out.append((field, base, depth, length))
    return out


def _ctype(pkg, base, depth, length=None, param=False):
    """The ctypes type the binding must use for a header type.  Parameters: `x[n]` is a pointer; a pointer to a struct follows the
    ABI table -- POINTER(mirror), or c_void_p for a numpy-held block and for what Python never builds."""
    A = pkg._abi
    if param and length is not None:
        depth, length = depth + 1, None
    if depth and base in A.STRUCTS:
        t, depth = C.POINTER(A.STRUCTS[base]), depth - 1
    elif depth and (base == "void" or base in A.DTYPES or base in A.NOT_MIRRORED):
        t, depth = C.c_void_p, depth - 1
    elif depth and base == "char":
        t, depth = C.c_char_p, depth - 1
    else:
        t = SCALARS[base][0]
    for _ in range(depth):
        t = C.POINTER(t)
    return t if length is None else t * length


def _natural_layout(fields):
    """([offset of every field], size) by natural C alignment: each member aligned to its scalar, the struct to its widest."""
    offsets, end, widest = [], 0, 1
    for _, base, depth, length in fields:
        size = C.sizeof(C.c_void_p) if depth else C.sizeof(SCALARS[base][0])
        end = -(-end // size) * size
        offsets.append(end)
        end += size * (length or 1)
        widest = max(widest, size)
    return offsets, -(-end // widest) * widest


def _check_struct(pkg, name):
    A = pkg._abi
    assert (name in A.STRUCTS) + (name in A.DTYPES) + (name in A.NOT_MIRRORED) == 1, "%s: listed once in _abi" % name
    if name in A.NOT_MIRRORED:
        assert A.NOT_MIRRORED[name], "%s: give the reason" % name
        return
    assert name in STRUCT_BODIES, "%s is opaque in the header" % name
    fields = _struct_fields(name)
    offsets, size = _natural_layout(fields)
    if name in A.STRUCTS:
        cls = A.STRUCTS[name]
        assert [f[0] for f in cls._fields_] == [f[0] for f in fields]
        for (field, base, depth, length), off, (_, ctype) in zip(fields, offsets, cls._fields_):
            assert ctype is _ctype(pkg, base, depth, length), "%s.%s" % (name, field)
            assert getattr(cls, field).offset == off, "%s.%s" % (name, field)
        assert C.sizeof(cls) == size
    else:
        dt = A.DTYPES[name]
        assert list(dt.names) == [f[0] for f in fields]
        for (field, base, depth, length), off in zip(fields, offsets):
            sub, at = dt.fields[field][:2]
            assert not depth and at == off, "%s.%s" % (name, field)
            assert sub.base == np.dtype(SCALARS[base][1]) and sub.shape == (() if length is None else (length,)), "%s.%s" % (name, field)
        assert dt.itemsize == size


def test_library_exports_every_declared_symbol(pkg):
    if not os.path.exists(pkg.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = pkg.load_library()
    decl = sorted(PROTOTYPES)
    assert len(decl) >= 15
    for s in decl:
        assert hasattr(lib, s), "missing export %s" % s
    assert sorted(pkg.ABI_SYMBOLS) == decl
    assert lib.bp_build_target() == b"gfx950"
    assert lib.bp_abi_version() == 5


def test_config_struct_matches_header(pkg):
    _check_struct(pkg, "bp_config")


@pytest.mark.parametrize("name", sorted((set(STRUCT_BODIES) | set(OPAQUE)) - {"bp_config"}))
def test_struct_matches_header(pkg, name):
    """Every typedef struct of the header: the Structure mirror or numpy dtype _abi.py names for it has the header's field names in
    order, scalar types, array lengths, pointers, offsets and size (natural C alignment); one never built in Python has its reason."""
    _check_struct(pkg, name)


def test_abi_lists_no_struct_the_header_lacks(pkg):
    A = pkg._abi
    assert set(A.STRUCTS) | set(A.DTYPES) | set(A.NOT_MIRRORED) == set(STRUCT_BODIES) | set(OPAQUE)
    assert set(A.NOT_MIRRORED) == set(OPAQUE)


@pytest.mark.parametrize("symbol", sorted(PROTOTYPES))
def test_signature_matches_header(pkg, symbol):
    """Every prototype: the table's argtypes have the header's parameter count and, per parameter, the ctypes type of its C type;
    the return type is the default (int) or c_char_p (const char *)."""
    A = pkg._abi
    text = PROTOTYPES[symbol].strip()
    params = [] if text in ("", "void") else [_declarator(t) for t in text.split(",")]
    assert len(A.ABI[symbol]) == len(params)
    for k, ((base, depth, length, name), got) in enumerate(zip(params, A.ABI[symbol])):
        assert got is _ctype(pkg, base, depth, length, param=True), "%s: parameter %d (%s)" % (symbol, k, name)
    assert A.ABI_RESTYPES.get(symbol, C.c_int) is {"int": C.c_int, "const char *": C.c_char_p}[RETURNS[symbol]]


def test_loaded_library_carries_the_table(pkg):
    if not os.path.exists(pkg.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib, A = pkg.load_library(), pkg._abi
    for symbol, argtypes in A.ABI.items():
        fn = getattr(lib, symbol)
        assert list(fn.argtypes or []) == list(argtypes) and fn.restype is A.ABI_RESTYPES.get(symbol, C.c_int), symbol


def test_constants_match_header_enums(pkg):
    """A Python constant X stands for the header's BP_X (enum or #define): the same value.  At least the ones the wrappers pass."""
    both = {k[3:]: v for k, v in dict(ENUMS, **DEFINES).items() if isinstance(getattr(pkg, k[3:], None), int)}
    assert len(both) >= 25 and {"MAXLAYER", "WAVE_MASK", "MIX_LPS_IBM", "SCORE_SISDR", "NOISE_SPP", "GV_DEP", "RIR_MAX_IMAGES"} <= set(both)
    for k, v in both.items():
        assert getattr(pkg, k) == v, k
    assert len(pkg._abi.PROF_KINDS) == ENUMS["BP_PROF_KINDS"]


def test_no_cpu_fallback_without_gpu(pkg):
    torch = pytest.importorskip("torch")
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    w = [None, np.zeros((4, 3), np.float32), np.zeros((3, 2), np.float32)]
    b = [None, np.zeros(3, np.float32), np.zeros(2, np.float32)]
    with pytest.raises(pkg.BPError):
        pkg.BP_GPU(1, 3, [4, 3, 2], 4, 1.0, 0.5, 0.0, w, b)


def test_product_does_not_import_oracle():
    """The oracle is test infrastructure: nothing under the package or include/ may reference it."""
    bad = []
    for base in ("dnn-for-speech-enhancement_amd", "include"):
        for dp, _, fns in os.walk(os.path.join(ROOT, base)):
            for fn in fns:
                if fn.endswith((".py", ".h", ".hip", ".cpp", ".cc")):
                    txt = open(os.path.join(dp, fn), errors="ignore").read()
                    if re.search(r"(import\s+oracle|from\s+oracle|oracle/|bp_oracle|libbp_oracle)", txt):
                        bad.append(os.path.join(dp, fn))
    assert not bad, bad
