"""The device-resident radar readers (mmw_uart_*, include/mmw.h) as far as a machine without a GPU can check them: the status
values are the ones pinned here (tests/test_abi.py holds entries, macros and layouts to the header), the kernel file is part of
the build, every entry refuses a NULL context, and the kernels of csrc/k_uart.hip compile without scratch or spilled registers."""
import ctypes as C
import os
import re

from mmwave_msc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MACROS = (("MMW_UART_NONE", 0), ("MMW_UART_POINTS", 1), ("MMW_UART_PACKET", 2), ("MMW_UART_OVERFLOW", 3), ("MMW_UART_RAISED", 4),
          ("MMW_UART_SKIPPED", 5), ("MMW_UART_BADCHUNK", 6), ("MMW_UART_CHUNK_DROPPED", 256), ("MMW_UART_BUFFER", 32768))


def test_header_binding_and_library_agree_on_the_reader_entries():
    for macro, val in MACROS:   # (the values the kernels and the callers were written against; tests/test_abi.py holds them to the header)
        assert getattr(_lib, macro[4:]) == val, macro
    # the kernel file is part of the build, its launchers are declared where every other launcher is
    csrc = os.path.join(ROOT, "mmwave_msc_amd", "csrc")
    assert re.search(r"^SRCS\s*=.*\bk_uart\.hip\b", open(os.path.join(csrc, "Makefile")).read(), flags=re.M)
    decl = open(os.path.join(csrc, "mmw_kernels.hpp")).read()
    assert "void launch_uart_read(" in decl and "void launch_uart_set_time(" in decl


def test_every_reader_entry_refuses_a_null_context():
    L = _lib.load()   # (declares every prototype: AttributeError if one is missing)
    buf = (C.c_uint8 * _lib.UART_BUFFER)()
    n, t = C.c_int32(7), C.c_double(3.0)
    cfg = _lib.MmwUartCfg(0.04, 0.12, 16, 0)
    assert L.mmw_uart_open(None, C.byref(cfg), 1, 0.0) == _lib.E_ARG
    assert L.mmw_uart_close(None) == _lib.E_ARG
    assert L.mmw_uart_read(None, None, None, 0, None, 0.0, None, None, None, None, None) == _lib.E_ARG
    assert L.mmw_uart_get_state(None, 0, buf, C.byref(n), C.byref(t)) == _lib.E_ARG
    assert (n.value, t.value) == (7, 3.0)
    assert L.mmw_uart_set_state(None, 0, buf, 0, 0.0) == _lib.E_ARG
    assert L.mmw_uart_set_time(None, None, 0.0) == _lib.E_ARG


def test_reader_kernels_use_no_scratch_and_spill_nothing():
    from tests._isa import _device_isa, _kernel_report, assert_clean, kernel_body
    rep, asm = _device_isa(("k_uart",))["k_uart"]
    rows = _kernel_report(rep)
    names = [k[0] for k in rows]
    # k_uart_read<R, SITE, LOG>: 1, 2, 4 rows per thread of the plain kernel, of SITE = true, and of either with LOG = true
    flags = [re.match(r"_ZN3mmw11k_uart_readILi\dELb([01])ELb([01])EEEv", n) for n in names]
    flags = [m.groups() for m in flags if m]
    assert flags.count(("0", "0")) == 3 and flags.count(("1", "0")) == 3, names
    assert flags.count(("0", "1")) == 3 and flags.count(("1", "1")) == 3, names
    assert sum("k_uart_set_time" in n for n in names) == 1, names
    assert_clean(rows)
    for name, scratch, vspill, vgprs, occ, sspill in rows:
        body = kernel_body(asm, name, ".Lfunc_end")
        assert "scratch_" not in body, name
        if "k_uart_read" in name:
            # the moves store the buffer in aligned 16-byte pieces and fetch a piece's source with one wide load
            assert "global_store_dwordx4" in body and "global_load_dwordx4" in body and "v_alignbyte_b32" in body, name
            assert occ >= 4, (name, occ)
    # the decode and the normalisation are the ones k_normalize_tlv runs: called, not restated
    src = open(os.path.join(ROOT, "mmwave_msc_amd", "csrc", "k_uart.hip")).read()
    misc = open(os.path.join(ROOT, "mmwave_msc_amd", "csrc", "k_misc.hip")).read()
    for fn in ("normalize_rows<R>(", "decode_tlv_object("):
        assert fn in src and fn in misc, fn
