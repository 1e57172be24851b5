"""The C ABI as Python tables, read from include/magic_hip.h: the ONE definition the kernels (csrc/common.hpp includes it), the ctypes
binding (host/lib.py) and the generated CPython wrappers (csrc/gen_fastcall.py) share.  No torch import: the build runs this file too.

The header is written in a narrow dialect and this reader supports exactly that, raising ValueError on anything else: comments,
preprocessor lines, the `extern "C"` braces, `typedef struct [tag] { members } name;` and `int magic_*(arguments);`.  A member / argument
is [const] <base> then declarators `[*[const]]... name [\\[N\\]]` separated by commas; <base> is one of BASE or an earlier struct's name.
Every pointer becomes c_void_p (device and host addresses are passed as integers).
"""
import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "include", "magic_hip.h")
BASE = {"int": C.c_int, "unsigned": C.c_uint, "float": C.c_float, "long long": C.c_longlong, "unsigned long long": C.c_ulonglong,
        "char": C.c_char, "unsigned char": C.c_ubyte, "void": None}
_DECL = re.compile(r"(?:const\s+)?(%s|magic_\w+)\b(.*)" % "|".join(sorted(BASE, key=len, reverse=True)), re.S)
_DECLARATOR = re.compile(r"\s*((?:\*\s*(?:const\b\s*)?)*)(\w+)\s*(?:\[(\d+)\])?\s*")


def _decl(text, structs):
    """`const void *qkv, *P` / `int mod[3]` / `magic_enc_layer L[6]` -> [(name, ctype), ...]"""
    m = _DECL.fullmatch(text.strip())
    if not m:
        raise ValueError(f"declaration outside the header's dialect: {text.strip()!r}")
    base = BASE[m.group(1)] if m.group(1) in BASE else structs.get(m.group(1))
    out = []
    for d in m.group(2).split(","):
        dm = _DECLARATOR.fullmatch(d)
        if not dm or (base is None and not dm.group(1)):          # (also: void by value, a struct that is not defined yet)
            raise ValueError(f"declaration outside the header's dialect: {text.strip()!r}")
        t = C.c_void_p if dm.group(1) else base
        out.append((dm.group(2), t * int(dm.group(3)) if dm.group(3) else t))
    return out


def parse(text):
    """header text -> ({entry point: [argument ctypes]}, {struct name: ctypes.Structure class}), both in the header's order"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    structs, sigs = {}, {}

    def struct(m):
        fields = [f for member in m.group(1).split(";") if member.strip() for f in _decl(member, structs)]
        structs[m.group(2)] = type(m.group(2), (C.Structure,), {"_fields_": fields, "__doc__": f"`{m.group(2)}` of include/magic_hip.h"})
        return " "

    def proto(m):
        args = m.group(2).strip()
        sigs[m.group(1)] = [] if args == "void" else [_decl(a, structs)[0][1] for a in args.split(",")]
        return " "
    text = re.sub(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    text = re.sub(r"\bint\s+(magic_\w+)\s*\(([^()]*)\)\s*;", proto, text)
    rest = re.sub(r'^\s*#.*$|extern\s+"C"\s*\{|\}', " ", text, flags=re.M).strip()
    if rest or not sigs:
        raise ValueError(f"outside the header's dialect: {rest[:80]!r}" if rest else "no entry point found")
    return sigs, structs


def load(path=None):
    with open(path or HEADER) as f:
        return parse(f.read())
