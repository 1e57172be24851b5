"""C-ABI checks that need no GPU: the library loads, exports every symbol include/magic_hip.h declares, the ctypes signatures the
binding took from the header (host/abi.py) agree with a second, independent reading of it argument by argument, and the ctypes
structs agree with what a C compiler makes of the same header, field by field."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

import magic_amd  # noqa: F401
from magic_amd.host import abi
from magic_amd.host import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "magic_hip.h")


def parse_header():
    src = open(os.path.join(ROOT, "include", "magic_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = {}
    for m in re.finditer(r"\bint\s+(magic_\w+)\s*\(([^)]*)\)\s*;", src, flags=re.S):
        name, args = m.group(1), m.group(2).strip()
        types = []
        if args and args != "void":
            for a in args.split(","):
                a = " ".join(a.split())
                if "*" in a:
                    types.append(L.vp)
                elif a.startswith("long long"):
                    types.append(L.i64)
                elif a.startswith("float"):
                    types.append(L.f32)
                elif a.startswith("unsigned long long"):
                    types.append(L.u64)
                elif a.startswith("unsigned"):
                    types.append(L.u32)
                elif a.startswith("int"):
                    types.append(L.i32)
                else:
                    raise AssertionError(f"unparsed arg {a!r} in {name}")
        protos[name] = types
    return protos


def test_header_and_ctypes_signatures_agree():
    protos = parse_header()
    assert set(protos) == set(L.SIGNATURES)
    for name, types in protos.items():
        assert types == L.SIGNATURES[name], name


def test_library_exports_every_declared_symbol():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in parse_header():
        assert hasattr(lib, name), name
    assert lib.magic_abi_version() == 1


def test_library_carries_the_id_of_this_source_tree(monkeypatch):
    """magic_build_id() == csrc/build_id.py's content hash of the sources: the binary under test is the binary of this tree; a library
    whose id differs is refused at load"""
    L.load()
    assert L.library_build_id() == L.source_build_id() and len(L.library_build_id()) == 16
    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setattr(L, "source_build_id", lambda: "0" * 16)
    with pytest.raises(L.MagicHipError, match="other sources"):
        L.load()


def test_missing_library_fails_loudly(monkeypatch):
    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setattr(L, "LIB_PATH", "/nonexistent/libmagic_hip.so")
    with pytest.raises(L.MagicHipError):
        L.load()


def test_fastcall_extension_binds_the_same_library_and_checks_arity():
    """the generated CPython marshalling layer (csrc/gen_fastcall.py): built, bound to the SAME libmagic_hip.so, one wrapper per
    entry point without struct arguments, argument count and types enforced before the C call"""
    L.load()
    assert os.path.exists(L.FAST_PATH), "csrc/Makefile builds _magic_fastcall.so next to libmagic_hip.so"
    fast = {n for n, f in L._FN.items() if type(f).__name__ == "builtin_function_or_method"}
    slow = set(L.SIGNATURES) - fast
    assert slow == {"magic_device_info", "magic_build_id", "magic_gemm_dw_grouped", "magic_gemm_dw_ws_need", "magic_mse_multi"}, slow
    assert L._FN["magic_abi_version"]() == L.load().magic_abi_version() == 1
    for args in ((1, 64, 80, 80), (0, 64, 600, 80), (1, 48, 80, 80), (1, 64, 5000, 80)):       # pure host function: both bindings agree
        assert L._FN["magic_attn_supported"](*args) == L.load().magic_attn_supported(*args)
    assert L._FN["magic_gemm_last_form"]() == L.load().magic_gemm_last_form()               # host state only: both bindings read the same word
    with pytest.raises(TypeError):
        L._FN["magic_attn_supported"](1, 64, 80)
    with pytest.raises(TypeError):
        L._FN["magic_attn_supported"](1, 64, 80, "80")
    n = len(L.SIGNATURES["magic_gemm"])
    assert L._FN["magic_gemm"](*([1, 0, 1, 1, 0, 128, 128] + [None if L.SIGNATURES["magic_gemm"][i] is L.vp else 0 for i in range(7, n)])) == -1   # M = 0 -> MAGIC_ERR_ARG


def layout_c(classes):
    """a C file that compiles only if every class has its struct's size and every field its offset and size"""
    out = ["#include <stddef.h>", '#include "magic_hip.h"']
    for name, cls in classes.items():
        out.append(f'_Static_assert(sizeof({name}) == {ctypes.sizeof(cls)}, "sizeof {name}");')
        for f, _ in cls._fields_:
            d = getattr(cls, f)
            out.append(f'_Static_assert(offsetof({name}, {f}) == {d.offset} && sizeof((({name}*)0)->{f}) == {d.size}, "{name}.{f}");')
    return "\n".join(out) + "\n"


def compiles(src, tmp_path, tag):
    (tmp_path / f"{tag}.c").write_text(src)
    r = subprocess.run(["gcc", "-std=c11", "-c", "-I", os.path.dirname(HEADER), f"{tag}.c", "-o", f"{tag}.o"], cwd=tmp_path, capture_output=True, text=True)
    return r.returncode == 0, r.stderr


def test_ctypes_struct_layouts_agree_with_the_c_compiler(tmp_path):
    """every struct of the header, as the binding built it, against gcc's layout of the header; and the check can fail: a class with two
    pointer fields of equal size swapped, and one with a field dropped, do not compile"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert len(L.STRUCTS) == len(re.findall(r"\btypedef\s+struct\b", text)) == 21           # a struct the reader skipped is a failure
    assert all(issubclass(c, ctypes.Structure) and c._fields_ for c in L.STRUCTS.values())
    ok, err = compiles(layout_c(L.STRUCTS), tmp_path, "layout")
    assert ok, err
    for name in ("magic_dw_desc", "magic_rowbwd_seg"):
        fields = list(L.STRUCTS[name]._fields_)
        i = next(j for j in range(len(fields) - 1) if fields[j][1] is fields[j + 1][1] is L.vp)
        swapped = fields[:i] + [fields[i + 1], fields[i]] + fields[i + 2:]
        dropped = fields[:i] + fields[i + 1:]
        for tag, fl in (("swapped", swapped), ("dropped", dropped)):
            ok, err = compiles(layout_c({name: type(name, (ctypes.Structure,), {"_fields_": fl})}), tmp_path, f"{name}_{tag}")
            assert not ok and "static assertion failed" in err, (name, tag, err)


@pytest.mark.parametrize("bad", ["int (*done)(int);", "unsigned flags : 3;", "double x;", "magic_rowbwd_seg later;", "void v;", "int n[];"])
def test_header_reader_refuses_a_member_outside_its_dialect(bad):
    text = open(HEADER).read()
    assert abi.parse(text)[1].keys() == L.STRUCTS.keys()
    marker = "typedef struct magic_dw_desc { "
    assert text.count(marker) == 1
    with pytest.raises(ValueError, match="dialect"):
        abi.parse(text.replace(marker, marker + bad + " "))


@pytest.mark.parametrize("bad", ["void magic_no_status(int x);", "int magic_cb(int (*f)(int));", "struct loose { int a; };", "int magic_global;"])
def test_header_reader_refuses_a_declaration_outside_its_dialect(bad):
    text = open(HEADER).read()
    marker = "int magic_group_begin(void);"
    assert text.count(marker) == 1
    with pytest.raises(ValueError, match="dialect"):
        abi.parse(text.replace(marker, marker + "\n" + bad))


@pytest.mark.parametrize("content", [None, "int magic_abi_version(void);\nint magic_x(double v);\n"])
def test_missing_or_unparsable_header_fails_loudly(tmp_path, content):
    """no fallback table: the binding refuses to import, naming the header it could not read"""
    path = tmp_path / "magic_hip.h"
    if content is not None:
        path.write_text(content)
    code = f"import sys; sys.path.insert(0, {ROOT!r}); import magic_amd; from magic_amd.host import abi; abi.HEADER = {str(path)!r}; from magic_amd.host import lib"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode != 0 and "MagicHipError" in r.stderr and str(path) in r.stderr, r.stderr
