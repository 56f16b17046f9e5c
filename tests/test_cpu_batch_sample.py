"""Sampling in batched decode without a GPU: the libraries export the entry points and the test hook, the Python binding declares them
(and lays the parameter struct out as the C header does), and neither entry point of the sampler kernel (csrc/sampling.hip: k_draw<plain, 0>,
k_draw_rows<plain, 0, 0>) uses a private segment or spills.

The test hook lives in lib/librwkv_testhooks_sample.so (include/rwkv_testhooks_sample.h), not in librwkv_testhooks.so: the surface of that
library is pinned to the nine entry points of include/rwkv_testhooks.h by tests/test_cpu_library.py."""
import ctypes
import os
import re

import pytest

import kernel_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


@pytest.mark.skipif(not kernel_meta.have_hipcc(), reason="needs hipcc")
def test_sampler_entry_points_have_no_private_segment():
    # the two entry points of the plain draw with no other axis set: k_sample and k_sample_rows before the draws had one body
    kernel_meta.budget("sampling.hip", (("k_draw", (0, 0)), ("k_draw_rows", (0, 0, 0))))
