"""include/mmw.h as data, for tests/test_abi.py and the tests that pin a size beside the compiler's answer: the structs as a C
compiler lays them out, the prototypes by argument class, the integer macros -- and the two comparisons that hold
mmwave_msc_amd._lib's mirrors to them."""
import ast
import ctypes as C
import functools
import operator
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


@functools.lru_cache(maxsize=None)
def header_code():
    """include/mmw.h without its comments."""
    with open(os.path.join(INCLUDE, "mmw.h")) as fh:
        return re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)


@functools.lru_cache(maxsize=None)
def header_structs():
    """{struct name: [field names in order]} of every `typedef struct mmw_x { ... } mmw_x;` (the opaque mmw_ctx has no body)."""
    out = {}
    for name, body in re.findall(r"typedef\s+struct\s+(mmw_\w+)\s*\{(.*?)\}\s*\1\s*;", header_code(), flags=re.S):
        decls = [d for d in (d.strip() for d in body.split(";")) if d]
        out[name] = [re.search(r"(\w+)\s*(?:\[[^\]]*\]\s*)*$", part).group(1) for d in decls for part in d.split(",")]
    return out


@functools.lru_cache(maxsize=None)
def c_layout():
    """{struct: {"size", "align", "fields": {field: (offset, bytes)}}} as a C compiler lays out include/mmw.h: ONE program for
    every struct of the header, compiled once per session."""
    import pytest
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    structs = header_structs()
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "mmw.h"\nint main(void){\n'
    for s, fields in structs.items():
        src += 'printf("%s %%zu %%zu\\n", sizeof(%s), (size_t)_Alignof(%s));\n' % (s, s, s)
        for f in fields:
            src += 'printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));\n' % (s, f, s, f, s, f)
    src += "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "layout.c"), "w") as fh:
            fh.write(src)
        exe = os.path.join(d, "layout")
        subprocess.run([cc, "-std=c11", "-I", INCLUDE, os.path.join(d, "layout.c"), "-o", exe], check=True, capture_output=True)
        lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    out = {}
    for key, a, b in (ln.split() for ln in lines if ln):
        if "." in key:
            s, f = key.split(".")
            out[s]["fields"][f] = (int(a), int(b))
        else:
            out[key] = {"size": int(a), "align": int(b), "fields": {}}
    return out


def _arg_class(decl):
    """pointer (x[4] included), i32, i64, size or f64 of one C parameter declaration."""
    if "*" in decl or "[" in decl:
        return "ptr"
    words = [w for w in decl.split() if w != "const"]
    return {"int": "i32", "int32_t": "i32", "int64_t": "i64", "size_t": "size", "double": "f64"}[" ".join(words[:-1])]


@functools.lru_cache(maxsize=None)
def header_prototypes():
    """{entry: (return class, [argument classes])} of every `int|const char * mmw_x(args);` of the header."""
    out = {}
    for ret, name, args in re.findall(r"^(int|const\s+char\s*\*)\s*(mmw_\w+)\s*\(([^)]*)\)\s*;", header_code(), flags=re.M):
        args = " ".join(args.split())
        out[name] = ("i32" if ret == "int" else "ptr", [] if args in ("", "void") else [_arg_class(a.strip()) for a in args.split(",")])
    return out


_OPS = {ast.Add: operator.add, ast.Sub: operator.sub, ast.Mult: operator.mul}


def int_expr(text):
    """The value of an expression of integers, + - * and parentheses; anything else is a ValueError."""
    def ev(n):
        if isinstance(n, ast.Constant) and type(n.value) is int:
            return n.value
        if isinstance(n, ast.UnaryOp) and isinstance(n.op, (ast.USub, ast.UAdd)):
            return -ev(n.operand) if isinstance(n.op, ast.USub) else ev(n.operand)
        if isinstance(n, ast.BinOp) and type(n.op) in _OPS:
            return _OPS[type(n.op)](ev(n.left), ev(n.right))
        raise ValueError(f"not an integer expression: {text!r}")
    return ev(ast.parse(text.strip(), mode="eval").body)


@functools.lru_cache(maxsize=None)
def header_defines():
    """{MMW_NAME: value} of every `#define MMW_NAME <integer or parenthesised integer expression>`."""
    found = re.findall(r"^#define[ \t]+(MMW_\w+)[ \t]+(.+?)[ \t]*$", header_code(), flags=re.M)
    return {name: int_expr(val) for name, val in found if re.fullmatch(r"[\d\s()+*-]+", val)}


def lib_name(macro):
    """The name mmwave_msc_amd._lib gives a header macro: the MMW_ prefix dropped, MMW_OK as it is."""
    return macro if macro == "MMW_OK" else macro[len("MMW_"):]


def mirror_layout(mirror):
    """A Python mirror (numpy dtype or ctypes.Structure) in c_layout's form."""
    if isinstance(mirror, np.dtype):
        return {"size": mirror.itemsize, "align": mirror.alignment,
                "fields": {f: (mirror.fields[f][1], mirror.fields[f][0].itemsize) for f in mirror.names}}
    return {"size": C.sizeof(mirror), "align": C.alignment(mirror),
            "fields": {f: (getattr(mirror, f).offset, getattr(mirror, f).size) for f, *_ in mirror._fields_}}


def struct_mismatches(cname, mirror, layout):
    """What differs between a mirror and the compiler's layout of struct `cname`, one line each (none: [])."""
    got, want = mirror_layout(mirror), layout
    bad = [f"{cname}: {k} {got[k]}, the header's is {want[k]}" for k in ("size", "align") if got[k] != want[k]]
    mine, theirs = list(got["fields"]), list(want["fields"])
    if len(mine) != len(theirs):
        bad.append(f"{cname}: {len(mine)} fields, the header's has {len(theirs)}: not in both {sorted(set(mine) ^ set(theirs))}")
    bad += [f"{cname}: field {i} is {m}, the header's is {t}" for i, (m, t) in enumerate(zip(mine, theirs)) if m != t]
    bad += [f"{cname}.{f}: (offset, bytes) {got['fields'][f]}, the header's is {want['fields'][f]}"
            for f in want["fields"] if f in got["fields"] and got["fields"][f] != want["fields"][f]]
    return bad


def ctype_class(t):
    """The argument class (_arg_class's) of a ctypes restype / argtype."""
    if t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, (C._Pointer, C.Array))):
        return "ptr"
    return {C.c_int32: "i32", C.c_int64: "i64", C.c_size_t: "size", C.c_double: "f64"}.get(t, repr(t))


def prototype_mismatches(name, entry, proto):
    """What differs between a `_lib.sig` entry (restype, argtypes) and the header's prototype, one line each (none: [])."""
    res, args = entry
    got = (ctype_class(res), [ctype_class(a) for a in args])
    bad = []
    if got[0] != proto[0]:
        bad.append(f"{name}: returns {got[0]}, the header says {proto[0]}")
    if len(got[1]) != len(proto[1]):
        bad.append(f"{name}: {len(got[1])} arguments, the header declares {len(proto[1])}")
    bad += [f"{name}: argument {i} is {g}, the header says {w}" for i, (g, w) in enumerate(zip(got[1], proto[1])) if g != w]
    return bad
