"""Ragged batch passes without a GPU: the library exports the two entry points, the Python binding declares them, RWKVBatch has the two
methods, and no segment kernel of csrc/kernels.hip uses scratch memory (the same metadata read as test_cpu_batch.py)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SYMBOLS = ("rwkv_mi_batch_eval_ragged", "rwkv_mi_batch_eval_ragged_sample")


def _pkg():
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    pkg = graft.load_package()
    pkg.build_library()
    return pkg


def test_library_exports_ragged_symbols():
    pkg = _pkg()
    so = ctypes.CDLL(pkg.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(so, name), name


def test_binding_declares_ragged_symbols():
    pkg = _pkg()
    lib = pkg.load_rwkv_shared_library()
    for name in SYMBOLS:
        f = getattr(lib.library, name)
        assert f.argtypes is not None, name
        assert f.restype is ctypes.c_bool, name
    # slots, lens, tokens, n, [params, sampled_out,] logits_out
    assert len(lib.library.rwkv_mi_batch_eval_ragged.argtypes) == 6
    assert len(lib.library.rwkv_mi_batch_eval_ragged_sample.argtypes) == 8
    for meth in ("eval_ragged", "eval_ragged_sample"):
        assert callable(getattr(pkg.RWKVBatch, meth)), meth


def test_header_declares_ragged_calls():
    text = open(os.path.join(ROOT, "include", "rwkv_mi355x.h")).read()
    for name in SYMBOLS:
        assert re.search(r"RWKV_API bool " + name + r"\(", text), name


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_segment_entry_points_have_no_private_segment(tmp_path):
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
        if "_segs" in name or "k_layernorm_gather" in name:
            seen.add(name)
            assert private == 0 and spills == 0, (name, private, vgprs, spills)
    # k_mix_segs, k_wkv4_segs, k_wkv6_segs<64/32/16/8> + generic, k_wkv7_segs<64/32> + generic, k_layernorm_gather (the head's rows)
    assert len(seen) >= 11, sorted(seen)
    for k in ("k_mix_segs", "k_wkv4_segs", "k_wkv6_segs", "k_wkv7_segs", "k_wkv6_segs_generic", "k_wkv7_segs_generic", "k_layernorm_gather"):
        assert any(k in n for n in seen), k
