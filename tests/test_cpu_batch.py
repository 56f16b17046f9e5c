"""Batched decode without a GPU: the library exports the rwkv_mi_batch_* entry points, the Python binding declares them, and no row kernel
of csrc/kernels.hip uses scratch memory (the same metadata read as test_cpu_kernel_budget.py)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SYMBOLS = ("rwkv_mi_batch_create", "rwkv_mi_batch_free", "rwkv_mi_batch_state_load", "rwkv_mi_batch_state_store",
           "rwkv_mi_batch_state_from_context", "rwkv_mi_batch_state_to_context", "rwkv_mi_batch_eval", "rwkv_mi_batch_decode_greedy")


def _pkg():
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    pkg = graft.load_package()
    pkg.build_library()
    return pkg


def test_library_exports_batch_symbols():
    pkg = _pkg()
    so = ctypes.CDLL(pkg.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(so, name), name


def test_binding_declares_batch_symbols():
    pkg = _pkg()
    lib = pkg.load_rwkv_shared_library()
    for name in SYMBOLS:
        f = getattr(lib.library, name)
        assert f.argtypes is not None, name
    assert lib.library.rwkv_mi_batch_eval.restype is ctypes.c_bool
    assert lib.library.rwkv_mi_batch_create.restype is ctypes.c_void_p
    for meth in ("state_load", "state_store", "from_context", "to_context", "eval", "decode_greedy", "free"):
        assert callable(getattr(pkg.RWKVBatch, meth)), meth


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_row_entry_points_have_no_private_segment(tmp_path):
    src = os.path.join(ROOT, "rwkv.cpp_amd", "csrc", "kernels.hip")
    out = str(tmp_path / "kernels.s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-DRWKV_SHARED", "-DRWKV_BUILD",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rwkv.cpp_amd", "csrc"), "-S", "--cuda-device-only", src, "-o", out]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels"):]
    seen = set()
    for m in re.finditer(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", meta, re.S):
        name, private, vgprs, spills = m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4))
        if "_rows" in name or "k_argmax" in name:
            seen.add(name)
            assert private == 0 and spills == 0, (name, private, vgprs, spills)
    # k_mix_rows, k_wkv4_rows, k_wkv6_rows<64/32/16/8> + generic, k_wkv7_rows<64/32> + generic, k_argmax (one workgroup per row)
    assert len(seen) >= 11, sorted(seen)
    for k in ("k_mix_rows", "k_wkv4_rows", "k_wkv6_rows", "k_wkv7_rows", "k_argmax", "k_wkv6_rows_generic", "k_wkv7_rows_generic"):
        assert any(k in n for n in seen), k
