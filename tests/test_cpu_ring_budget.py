"""No instantiation of k6_ring may use scratch memory or spill, and each must fit 256 registers (two waves per SIMD: the loader, the comm
wave and six consumers of a workgroup share a CU). The consumer waves hold every record they can in registers (ring_v6.hip, `Pre`), so the
budget is the first thing a change to the takes breaks: tools/check_ring_regs.sh prints these numbers, this test asserts them. The check
compiles ring_v6.hip for gfx950 (device side only, no GPU needed) with the script's flags and reads the kernel metadata hipcc emits."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_ring_kernels_fit_the_register_file(tmp_path):
    src = os.path.join(ROOT, "rwkv.cpp_amd", "csrc", "ring_v6.hip")
    out = str(tmp_path / "ring.s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-DRWKV_SHARED", "-DRWKV_BUILD",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rwkv.cpp_amd", "csrc"), "-S", "--cuda-device-only", src, "-o", out]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels"):]
    seen = 0
    for m in re.finditer(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", meta, re.S):
        name, private, vgprs, spills = m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4))
        if "k6_ring" in name:
            seen += 1
            assert private == 0, (name, private, vgprs, spills)
            assert spills == 0, (name, private, vgprs, spills)
            assert vgprs <= 256, (name, vgprs)
    assert seen >= 15, seen
