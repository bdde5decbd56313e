"""hvc.PROTOTYPES, the binding's one table of the ABI, held to include/hvc_jpeg.h for every function the header declares:
a function without argtypes takes a Python int as a C int, so a pointer or a size_t would be cut to 32 bits silently.
No GPU and no context: the table is read as it stands, and the library is only loaded to see the table applied."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_prototypes():
    """[(name, return type, [parameter declarations])] of every HVC_API function, comments stripped"""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hvc_jpeg.h")).read(), flags=re.S)
    out = []
    for ret, name, args in re.findall(r"HVC_API\s+([\w\s\*]+?)\b(hvc_\w+)\s*\(([^;]*?)\)\s*;", hdr, flags=re.S):
        args = " ".join(args.split())
        out.append((name, " ".join(ret.split()), [] if args in ("", "void") else [a.strip() for a in args.split(",")]))
    return out


PROTOS = declared_prototypes()


def is_pointer_type(t):
    return t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer))


def is_unsigned_8_bytes(t):
    """by size and signedness: c_size_t is c_uint64 (or c_ulong) depending on the platform"""
    return isinstance(t, type) and issubclass(t, C._SimpleCData) and C.sizeof(t) == 8 and t(-1).value == 2 ** 64 - 1


def param_matches(decl, t):
    """one parameter declaration of the header against one ctypes type; (ok, what was expected)"""
    if "*" in decl or "[" in decl:
        return is_pointer_type(t), "a pointer type"
    base = " ".join(w for w in decl.split()[:-1] if w != "const")
    if base == "int":
        return t is C.c_int, "c_int"
    if base in ("size_t", "uint64_t"):
        return is_unsigned_8_bytes(t), "an 8-byte unsigned integer"
    return False, "a mapping for the by-value type %r (none yet)" % base


def test_the_header_declares_142_functions_and_the_table_lists_exactly_those():
    from video_coding_amd import hvc
    names = [name for name, _, _ in PROTOS]
    assert len(names) == len(set(names)) == 142
    assert sorted(hvc.PROTOTYPES) == sorted(names)
    assert sorted(hvc.SYMBOLS) == sorted(names)


@pytest.mark.parametrize("name,ret,params", PROTOS, ids=[p[0] for p in PROTOS])
def test_table_entry_matches_the_header(name, ret, params):
    from video_coding_amd import hvc
    proto = hvc.PROTOTYPES[name]
    assert 1 <= len(proto) <= 2
    argtypes = list(proto[0])
    assert len(argtypes) == len(params), (name, params, argtypes)
    for k, (decl, t) in enumerate(zip(params, argtypes)):
        ok, want = param_matches(decl, t)
        assert ok, "%s, parameter %d (%s): %r is not %s" % (name, k, decl, t, want)
    restype = proto[1] if len(proto) > 1 else C.c_int
    assert ret in ("int", "const char *", "void"), (name, ret)
    assert restype is {"int": C.c_int, "const char *": C.c_char_p, "void": None}[ret], (name, ret, restype)


def test_the_loaded_library_carries_the_table():
    """after lib(): no declared function is left without argtypes, and each has the table's types"""
    import video_coding_amd as hvc
    hvc.build()
    L = hvc.lib()
    for name, ret, _ in PROTOS:
        fn = getattr(L, name)
        proto = hvc.hvc.PROTOTYPES[name]
        assert fn.argtypes is not None, name
        assert list(fn.argtypes) == list(proto[0]), name
        assert fn.restype is (proto[1] if len(proto) > 1 else C.c_int), name


def test_a_library_without_a_declared_symbol_fails_at_load_and_names_it(tmp_path):
    """header and library come from one tree: a library that lacks a function of the table is refused by name (a child process:
    the library of this one is loaded already)"""
    import subprocess
    import sys
    src = tmp_path / "empty.c"
    src.write_text("int hvc_create(void **out, int device) { (void)out; (void)device; return -2; }\n")
    so = tmp_path / "libhvc_empty.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)])
    code = "\n".join(["import sys", "sys.path.insert(0, %r)" % ROOT, "import video_coding_amd as hvc",
                      "try:", "    hvc.lib()", "except ImportError as e:", "    print('REFUSED', e)"])
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, HVC_JPEG_LIB=str(so)))
    assert r.returncode == 0 and "REFUSED" in r.stdout and "hvc_destroy" in r.stdout, (r.stdout, r.stderr[-2000:])
