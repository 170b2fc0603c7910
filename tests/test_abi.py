"""mmwave_msc_amd._lib mirrors include/mmw.h in three tables -- ABI_STRUCTS, sig, the constants -- and this is the one place that
holds all three to the header (tests/_abi.py reads it): every struct's size, alignment and every field's offset and byte size
are the C compiler's, every prototype has the header's arity and argument classes and is exported by the library, every
integer macro has its value.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from mmwave_msc_amd import _lib
from tests import _abi

STRUCTS = sorted(_abi.header_structs())
ENTRIES = sorted(_abi.header_prototypes())
MACROS = sorted(_abi.header_defines())


def test_the_tables_cover_the_header_and_nothing_else():
    # (what the header held when this was written, counted by hand: the parsers have not gone blind to a family since)
    assert len(STRUCTS) >= 17 and len(ENTRIES) >= 108 and len(MACROS) >= 57, (len(STRUCTS), len(ENTRIES), len(MACROS))
    assert sorted(_lib.ABI_STRUCTS) == STRUCTS, "ABI_STRUCTS and the header's structs disagree"
    assert sorted(_lib.sig) == ENTRIES, "sig and the header's prototypes disagree"
    assert _lib.EXPORTS == list(_lib.sig)
    # every `mmw_x(` of the header is one of the prototypes read: none escaped the parser
    assert sorted(set(re.findall(r"\b(mmw_[a-z0-9_]+)\s*\(", _abi.header_code()))) == ENTRIES


@pytest.mark.parametrize("cname", STRUCTS)
def test_struct_mirror_has_the_compilers_layout(cname):
    assert cname in _lib.ABI_STRUCTS, f"{cname}: no mirror in _lib.ABI_STRUCTS"
    layout = _abi.c_layout()[cname]
    assert list(layout["fields"]) == _abi.header_structs()[cname] and layout["size"] > 0
    bad = _abi.struct_mismatches(cname, _lib.ABI_STRUCTS[cname], layout)
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("name", ENTRIES)
def test_prototype_is_the_headers_and_the_library_exports_it(name):
    assert os.path.isfile(_lib.LIB_PATH), "libmmw_hip.so missing: run __graft_entry__.build()"
    assert name in _lib.sig, f"{name}: declared in include/mmw.h, no prototype in _lib.sig"
    bad = _abi.prototype_mismatches(name, _lib.sig[name], _abi.header_prototypes()[name])
    assert not bad, "; ".join(bad)
    assert hasattr(C.CDLL(_lib.LIB_PATH), name), f"{name} declared in include/mmw.h but not exported"
    fn = getattr(_lib.load(), name)
    assert (fn.restype, list(fn.argtypes)) == (_lib.sig[name][0], list(_lib.sig[name][1])), f"{name}: load() declared another prototype"


@pytest.mark.parametrize("macro", MACROS)
def test_integer_macro_has_its_lib_name_and_value(macro):
    want, name = _abi.header_defines()[macro], _abi.lib_name(macro)
    assert hasattr(_lib, name), f"{macro}: no _lib.{name}"
    got = getattr(_lib, name)
    assert type(got) is int and got == want, f"{macro} = {want} in the header, _lib.{name} = {got!r}"


def test_the_comparisons_report_a_swapped_field_and_a_widened_argument():
    """The checks above cannot pass vacuously: the same comparisons, fed a mirror that is wrong, say so."""
    dt = _lib.TRACK_REPORT_DTYPE
    names = list(dt.names)
    i, j = names.index("slot"), names.index("uid")   # adjacent, both int32: size and every other offset stay right
    names[i], names[j] = names[j], names[i]
    swapped = np.dtype([(f,) + tuple(dt.fields[f][0].subdtype or (dt.fields[f][0],)) for f in names], align=True)
    assert swapped.itemsize == dt.itemsize
    bad = _abi.struct_mismatches("mmw_track_report", swapped, _abi.c_layout()["mmw_track_report"])
    assert any("mmw_track_report.slot" in b for b in bad) and any("mmw_track_report.uid" in b for b in bad), bad
    res, args = _lib.sig["mmw_report_async"]
    k = args.index(C.c_int32)
    wide = list(args[:k]) + [C.c_int64] + list(args[k + 1:])
    bad = _abi.prototype_mismatches("mmw_report_async", (res, wide), _abi.header_prototypes()["mmw_report_async"])
    assert bad == [f"mmw_report_async: argument {k} is i64, the header says i32"], bad
    # ... and a field the mirror lacks, an argument it lacks, an expression that is no integer arithmetic
    short = np.dtype([(f,) + tuple(dt.fields[f][0].subdtype or (dt.fields[f][0],)) for f in dt.names[:-1]], align=True)
    assert any("fields" in b for b in _abi.struct_mismatches("mmw_track_report", short, _abi.c_layout()["mmw_track_report"]))
    assert any("arguments" in b for b in _abi.prototype_mismatches("mmw_report_async", (res, args[:-1]), _abi.header_prototypes()["mmw_report_async"]))
    assert _abi.int_expr("(5 + 2 * (7 - 3) * 4)") == 37 and _abi.int_expr("(-3)") == -3
    for text in ("__import__('os')", "1 / 2", "2 ** 3", "(void *)1", "x + 1"):
        with pytest.raises((ValueError, SyntaxError)):
            _abi.int_expr(text)
