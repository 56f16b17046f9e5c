"""Sampling in batched decode without a GPU: the libraries export the entry points and the test hook, the Python binding declares them
(and lays the parameter struct out as the C header does), and neither entry point of the sampler kernel (csrc/sampling.hip: k_sample,
k_sample_rows) uses a private segment or spills.

The test hook lives in lib/librwkv_testhooks_sample.so (include/rwkv_testhooks_sample.h), not in librwkv_testhooks.so: the surface of that
library is pinned to the nine entry points of include/rwkv_testhooks.h by tests/test_cpu_library.py."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SYMBOLS = ("rwkv_mi_batch_eval_sample", "rwkv_mi_batch_decode_sample", "rwkv_mi_batch_rng_seek")
HOOK = "rwkv_mi_test_sample_rows"


def _pkg():
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    pkg = graft.load_package()
    pkg.build_library()
    return pkg


def test_libraries_export_the_sampling_symbols():
    pkg = _pkg()
    so = ctypes.CDLL(pkg.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(so, name), name
    assert not hasattr(so, HOOK), "the product library exports a test hook"
    assert not hasattr(ctypes.CDLL(pkg.HOOKS_LIB_PATH), HOOK), "the surface of librwkv_testhooks.so is rwkv_testhooks.h"
    hooks = ctypes.CDLL(pkg.SAMPLE_HOOKS_LIB_PATH)
    for name in SYMBOLS + (HOOK,):
        assert hasattr(hooks, name), name
    header = open(os.path.join(ROOT, "include", "rwkv_testhooks_sample.h")).read()
    assert re.findall(r"RWKV_API[^;(]*?\b(rwkv_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)) == [HOOK]


def test_binding_declares_the_sampling_symbols():
    pkg = _pkg()
    lib = pkg.load_rwkv_shared_library()
    for name in SYMBOLS:
        f = getattr(lib.library, name)
        assert f.argtypes is not None, name
        assert f.restype is ctypes.c_bool, name
    hooks = pkg.RWKVSharedLibrary(pkg.SAMPLE_HOOKS_LIB_PATH)
    f = getattr(hooks.library, HOOK)
    assert f.argtypes is not None and len(f.argtypes) == 7 and f.restype is ctypes.c_bool
    # struct rwkv_mi_sample_params { float temperature; float top_p; float u; uint64_t seed; }
    assert ctypes.sizeof(pkg.SampleParams) == 24
    assert [pkg.SampleParams.temperature.offset, pkg.SampleParams.top_p.offset, pkg.SampleParams.u.offset, pkg.SampleParams.seed.offset] == [0, 4, 8, 16]
    for meth in ("eval_sample", "decode_sample", "rng_seek"):
        assert callable(getattr(pkg.RWKVBatch, meth)), meth


def test_parameter_rows_take_scalars_or_sequences():
    pkg = _pkg()
    rows = pkg.sample_params(3, 0.7, [0.5, 0.8, 1.0], seed=[1, 2, 1 << 40])
    assert [(round(r.temperature, 6), round(r.top_p, 6), r.u, r.seed) for r in rows] == [(0.7, 0.5, -1.0, 1), (0.7, 0.8, -1.0, 2), (0.7, 1.0, -1.0, 1 << 40)]
    with pytest.raises(ValueError):
        pkg.sample_params(3, [0.7, 0.8], 0.5)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_sampler_entry_points_have_no_private_segment(tmp_path):
    src = os.path.join(ROOT, "rwkv.cpp_amd", "csrc", "sampling.hip")
    out = str(tmp_path / "sampling.s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-DRWKV_SHARED", "-DRWKV_BUILD",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rwkv.cpp_amd", "csrc"), "-S", "--cuda-device-only", src, "-o", out]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels"):]
    seen = {}
    for m in re.finditer(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", meta, re.S):
        name, private, vgprs, spills = m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4))
        for k in ("k_sample_rows", "k_sample"):
            if re.search(k + r"E?[Pv]", name) or name.endswith(k):   # (mangled: ...8k_sampleEPKf..., ...13k_sample_rowsEPKf...)
                seen[k] = name
                assert private == 0 and spills == 0, (name, private, vgprs, spills)
                assert vgprs <= 128, (name, vgprs, "1024 threads per workgroup leave 128 registers per thread")
                break
    assert set(seen) == {"k_sample", "k_sample_rows"}, seen
