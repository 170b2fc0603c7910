"""The site instantiations of csrc/k_misc.hip (SITE = true of k_normalize, k_normalize_tlv, k_features, k_table), read from
the compiler's resource report and the ISA the way tests/test_cabi_exports.py reads them for the step kernels: no spilled
VGPR, no scratch; and the mounting of k_normalize<., ., true> / k_normalize_tlv<., true> arrives as scalar operands (one
workgroup is one scene), not as a per-lane load."""
import re

from tests._isa import _device_isa, _kernel_report, assert_clean, kernel_body

# _ZN3mmw<len><name>I<template arguments>EEv...: SITE is the last template argument, a bool (Lb1E = true, Lb0E = false)
SITE_KERNEL = re.compile(r"_ZN3mmw\d+(k_normalize|k_normalize_tlv|k_features|k_table)I(.*?)Lb1EEEv")


def test_site_kernels_use_no_scratch_and_read_the_mounting_through_the_scalar_cache():
    rep, asm = _device_isa(("k_misc",))["k_misc"]
    rows = [k for k in _kernel_report(rep) if SITE_KERNEL.match(k[0])]
    families = [SITE_KERNEL.match(k[0]).group(1) for k in rows]
    assert families.count("k_normalize") == 6      # fp64 / fp32 raw rows x 1, 2, 4 rows per thread
    assert families.count("k_normalize_tlv") == 3
    assert families.count("k_features") == 1 and families.count("k_table") == 1
    assert_clean(rows)
    for name, scratch, vspill, vgprs, occ, sspill in rows:
        body = kernel_body(asm, name)
        assert "scratch_" not in body, name
        if "k_normalize" in name:
            # the site variant adds no vector load to the plain kernel's: the three doubles of the mounting come by s_load from the
            # table (in place of the plain kernel's six dwords of kernel arguments), plus the two dwords of the table's pointer
            # the plain kernel: the same name and template arguments with SITE = false
            m = SITE_KERNEL.match(name)
            twins = [k[0] for k in _kernel_report(rep) if k[0].startswith("_ZN3mmw%d%sI%sLb0EEEv" % (len(m.group(1)), m.group(1), m.group(2)))]
            assert len(twins) == 1, (name, twins)
            twin = twins[0]
            tb = kernel_body(asm, twin)
            vload = lambda b: len(re.findall(r"\b(global|flat|buffer)_load_", b))
            sload = lambda b: sum({"": 1, "x2": 2, "x4": 4, "x8": 8, "x16": 16}[m] for m in re.findall(r"\bs_load_dword(x\d+)?\b", b))
            assert vload(body) == vload(tb), (name, vload(body), vload(tb))
            assert sload(body) >= sload(tb) + 2, (name, sload(body), sload(tb))
