"""What the tests that read the compiler's output share: the resource report and the ISA of a csrc/*.hip file for gfx950 with the
product's flags, a kernel's body in that ISA, and the "no scratch, nothing spilled" assertion."""
_ISA_CACHE = {}


def _device_isa(names):
    """(resource report, ISA text) of csrc/<name>.hip for gfx950 with the product's flags: ONE device-only compile per file gives
    both (the remarks on stderr, the assembly on stdout); files compile side by side and are cached for the session."""
    import os
    import shutil
    import subprocess
    from concurrent.futures import ThreadPoolExecutor
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        import pytest
        pytest.skip("hipcc not available")
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mmwave_msc_amd", "csrc")

    def one(name):
        out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "--cuda-device-only",
                              "-Rpass-analysis=kernel-resource-usage", "-S", "-c", os.path.join(root, name + ".hip"), "-o", "-"],
                             capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-2000:]
        return out.stderr, out.stdout

    todo = [n for n in names if n not in _ISA_CACHE]
    with ThreadPoolExecutor(max_workers=4) as ex:
        for n, r in zip(todo, ex.map(one, todo)):
            _ISA_CACHE[n] = r
    return {n: _ISA_CACHE[n] for n in names}


def _kernel_report(rep):
    """[(mangled name, scratch bytes per lane, spilled VGPRs, VGPRs, waves per SIMD, spilled SGPRs)] from -Rpass-analysis=kernel-resource-usage."""
    import re
    out = []
    for blk in re.split(r"remark: Function Name: ", rep)[1:]:
        name = blk.split()[0]
        f = lambda pat: int(re.search(pat, blk).group(1))
        out.append((name, f(r"ScratchSize \[bytes/lane\]: (\d+)"), f(r"VGPRs Spill: (\d+)"), f(r" VGPRs: (\d+)"), f(r"Occupancy \[waves/SIMD\]: (\d+)"),
                    f(r"SGPRs Spill: (\d+)")))
    return out


def kernel_body(asm, name, end="s_endpgm"):
    """The ISA of kernel `name` from its label to the first `end` behind it (".Lfunc_end" for the whole kernel: one that returns
    early has more than one s_endpgm)."""
    body = asm[asm.index("\n" + name + ":"):]
    return body[: body.index(end)]


def assert_clean(rows, sgpr_spill=0):
    """No scratch, no spilled VGPR and at most `sgpr_spill` spilled SGPRs in every row of `_kernel_report` given."""
    for name, scratch, vspill, vgprs, occ, sspill in rows:
        assert scratch == 0 and vspill == 0 and sspill <= sgpr_spill, (name, scratch, vspill, sspill)
