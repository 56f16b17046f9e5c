"""Per-position scoring (rwkv_mi_score_resident / rwkv_mi_batch_score_ragged), without a GPU: the three libraries export the two entry points
and the kernel's test hook, the headers declare them, the Python binding declares their argument types, and the scoring kernel
(csrc/score.hip: k_score_rows) keeps within the budget of its 1024-thread workgroup: 128 registers per thread, no private segment, no spills."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SYMBOLS = ("rwkv_mi_score_resident", "rwkv_mi_batch_score_ragged")
HOOK = "rwkv_test_score_rows"


def _pkg():
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    pkg = graft.load_package()
    pkg.build_library()
    return pkg


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    return set(re.findall(r"RWKV_API[^;(]*?\b(rwkv_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


def test_libraries_export_the_scoring_symbols():
    pkg = _pkg()
    for path in (pkg.LIB_PATH, pkg.HOOKS_LIB_PATH, pkg.SAMPLE_HOOKS_LIB_PATH):
        so = ctypes.CDLL(path)
        for name in SYMBOLS:
            assert hasattr(so, name), (path, name)
    # the kernel's hook: the sampler hooks' library only
    assert hasattr(ctypes.CDLL(pkg.SAMPLE_HOOKS_LIB_PATH), HOOK)
    assert not hasattr(ctypes.CDLL(pkg.LIB_PATH), HOOK) and not hasattr(ctypes.CDLL(pkg.HOOKS_LIB_PATH), HOOK)


def test_headers_declare_them():
    assert set(SYMBOLS) <= _declared("rwkv_mi355x.h")
    assert _declared("rwkv_testhooks_score.h") == {HOOK}
    header = open(os.path.join(ROOT, "include", "rwkv_mi355x.h")).read()
    assert re.search(r"#define\s+RWKV_MI_NO_TARGET\s+UINT32_MAX", header)


def test_binding_declares_the_scoring_symbols():
    pkg = _pkg()
    lib = pkg.load_rwkv_shared_library()
    for name in SYMBOLS:
        f = getattr(lib.library, name)
        assert f.argtypes is not None, name
        assert f.restype is ctypes.c_bool, name
    assert len(lib.library.rwkv_mi_score_resident.argtypes) == 7 and len(lib.library.rwkv_mi_batch_score_ragged.argtypes) == 8
    hooks = pkg.RWKVSharedLibrary(pkg.SAMPLE_HOOKS_LIB_PATH)
    assert hooks.library.rwkv_test_score_rows.argtypes is not None and hooks.library.rwkv_test_score_rows.restype is ctypes.c_bool
    for meth in ("score_resident", "perplexity"):
        assert callable(getattr(pkg.RWKVModel, meth)), meth
    assert callable(pkg.RWKVBatch.score_ragged)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_the_scoring_kernel_keeps_the_budget(tmp_path):
    src = os.path.join(ROOT, "rwkv.cpp_amd", "csrc", "score.hip")
    out = str(tmp_path / "score.s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-DRWKV_SHARED", "-DRWKV_BUILD",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rwkv.cpp_amd", "csrc"), "-S", "--cuda-device-only", src, "-o", out]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels"):]
    seen = []
    for m in re.finditer(r"\.max_flat_workgroup_size:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", meta, re.S):
        wg, name, private, vgprs, spills = int(m.group(1)), m.group(2), int(m.group(3)), int(m.group(4)), int(m.group(5))
        if re.search(r"\dk_score_rowsEPKf", name):   # (mangled: ...12k_score_rowsEPKfiPKjPfPj)
            seen.append(name)
            assert wg == 1024, (name, wg)
            assert private == 0 and spills == 0, (name, private, vgprs, spills)
            assert vgprs <= 128, (name, vgprs, "1024 threads per workgroup leave 128 registers per thread")
    assert len(seen) == 1, seen
