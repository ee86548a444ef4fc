"""The C-ABI library loads without a GPU and exports exactly what include/reloc.h declares; compute
entry points fail loudly (no CPU fallback) when no device is usable."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = open(os.path.join(ROOT, "include", "reloc.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(reloc_[a-z0-9_]+)\s*\(", txt)) - {"reloc_ctx"})


def test_header_binding_and_library_agree():
    from nclt_slam_project_amd import _native as N
    declared = _declared()
    assert len(declared) >= 35
    assert sorted(N.SIGNATURES) == declared, "include/reloc.h and _native.SIGNATURES differ"
    assert os.path.exists(N.LIB_PATH), "build the library first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(N.LIB_PATH)
    missing = [s for s in declared if not hasattr(lib, s)]
    assert not missing, f"libreloc_hip.so lacks {missing}"
    N.load(strict=True)


_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
            "float": ctypes.c_float, "double": ctypes.c_double}


def _header():
    """include/reloc.h without comments, preprocessor lines and the opening of its extern "C" block"""
    txt = open(os.path.join(ROOT, "include", "reloc.h")).read()
    txt = re.sub(r"/\*.*?\*/|//[^\n]*", " ", txt, flags=re.S)
    return re.sub(r'^\s*#.*$|extern\s+"C"\s*\{', "", txt, flags=re.M)


def _ctype(decl, N, ret=False):
    """the ctypes twin of one C parameter (with its name) or return type, by the rules of the binding"""
    decl = " ".join(decl.replace("*", " * ").replace("[", " [").split())
    words = [t for t in decl.split() if t != "const"]
    if "*" in words or "[" in decl:
        if words[0] == "reloc_ctx" and words.count("*") == 1 and "[" not in decl:
            return N.c_ctx
        if ret:
            return ctypes.c_char_p if words[0] == "char" else ctypes.c_void_p
        return N.P
    base = words[0] if ret else " ".join(words[:-1])         # a parameter carries its name behind the type
    return None if ret and base == "void" else _SCALARS[base]


def test_signatures_match_the_header_type_by_type():
    """every declaration of include/reloc.h against _native.SIGNATURES: return type and each parameter; the fields of
    reloc_params against RelocParams._fields_.  No declaration is left out."""
    from nclt_slam_project_amd import _native as N
    txt = _header()
    struct = re.search(r"typedef\s+struct\s+reloc_params\s*\{(.*?)\}\s*reloc_params\s*;", txt, flags=re.S)
    fields = [tuple(f.split()) for f in struct.group(1).split(";") if f.strip()]
    assert [(name, _SCALARS[ty]) for ty, name in fields] == list(N.RelocParams._fields_)
    compared = []
    for stmt in (txt[:struct.start()] + txt[struct.end():]).split(";"):
        m = re.fullmatch(r"\s*(.*?)\b(reloc_[a-z0-9_]+)\s*\((.*)\)\s*", stmt, flags=re.S)
        if m is None:
            continue
        ret, name, params = m.groups()
        params = [] if params.strip() in ("", "void") else params.split(",")
        got = (_ctype(ret, N, ret=True), [_ctype(p, N) for p in params])
        assert got == (N.SIGNATURES[name][0], list(N.SIGNATURES[name][1])), f"{name}: the header says {got}"
        compared.append(name)
    assert sorted(compared) == _declared() and len(compared) == len(set(compared))


def test_no_cpu_fallback_without_device():
    from nclt_slam_project_amd import _native as N
    from nclt_slam_project_amd.engine import Engine
    lib = N.load()
    if lib.reloc_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(N.RelocError, match="no HIP device"):
        Engine()
    import nclt_slam_project_amd.cv2_shim as shim
    shim._default = None
    with pytest.raises(shim.error):
        shim.cvtColor(np.zeros((8, 8, 3), np.uint8), shim.COLOR_BGR2GRAY)


def test_product_never_imports_the_oracle():
    """the shipped path must not route through the CPU oracle in any form"""
    pkg = os.path.join(ROOT, "nclt-slam-project_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                txt = open(os.path.join(dirpath, f)).read()
                for needle in ("import oracle", "from oracle", "libreloc_oracle", "orc_"):
                    assert needle not in txt, f"{f} mentions {needle}"
