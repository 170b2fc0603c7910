"""The site instantiations of csrc/k_misc.hip (k_normalize_site, k_normalize_tlv_site, k_features_site, k_table_site), read from
the compiler's resource report and the ISA the way tests/test_cabi_exports.py reads them for the step kernels: no spilled
VGPR, no scratch; and the mounting of k_normalize_site / k_normalize_tlv_site arrives as scalar operands (one workgroup is
one scene), not as a per-lane load."""
import re

from tests._isa import _device_isa, _kernel_report, assert_clean, kernel_body


def test_site_kernels_use_no_scratch_and_read_the_mounting_through_the_scalar_cache():
    rep, asm = _device_isa(("k_misc",))["k_misc"]
    rows = [k for k in _kernel_report(rep) if "_site" in k[0]]
    names = [k[0] for k in rows]
    assert sum("k_normalize_siteI" in n for n in names) == 6      # fp64 / fp32 raw rows x 1, 2, 4 rows per thread
    assert sum("k_normalize_tlv_siteI" in n for n in names) == 3
    assert sum("k_features_site" in n for n in names) == 1 and sum("k_table_site" in n for n in names) == 1
    assert_clean(rows)
    for name, scratch, vspill, vgprs, occ, sspill in rows:
        body = kernel_body(asm, name)
        assert "scratch_" not in body, name
        if "k_normalize" in name:
            # the site variant adds no vector load to its plain twin's: the three doubles of the mounting come by s_load from the
            # table (in place of the twin's six dwords of kernel arguments), plus the two dwords of the table's pointer
            # the plain twin: the same kernel name without "_site", the same template arguments (_ZN3mmw<len><name>I<args>E...)
            m = re.match(r"_ZN3mmw\d+(k_normalize(?:_tlv)?)_siteI(.*?)EEv", name)
            assert m, name
            plain = m.group(1)
            twins = [k[0] for k in _kernel_report(rep) if k[0].startswith("_ZN3mmw%d%sI%sEEv" % (len(plain), plain, m.group(2)))]
            assert len(twins) == 1, (name, twins)
            twin = twins[0]
            tb = kernel_body(asm, twin)
            vload = lambda b: len(re.findall(r"\b(global|flat|buffer)_load_", b))
            sload = lambda b: sum({"": 1, "x2": 2, "x4": 4, "x8": 8, "x16": 16}[m] for m in re.findall(r"\bs_load_dword(x\d+)?\b", b))
            assert vload(body) == vload(tb), (name, vload(body), vload(tb))
            assert sload(body) >= sload(tb) + 2, (name, sload(body), sload(tb))
