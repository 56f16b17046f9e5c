"""Ragged batch passes without a GPU: the library exports the two entry points, the Python binding declares them, RWKVBatch has the two
methods, and no segment kernel of csrc/recur.hip uses scratch memory (the same metadata read as test_cpu_batch.py)."""
import ctypes
import os
import re

import pytest

import kernel_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


@pytest.mark.skipif(not kernel_meta.have_hipcc(), reason="needs hipcc")
def test_segment_entry_points_have_no_private_segment():
    """the SEGS form of every recurrence, and the gathered layer norm in front of the head (the segments' last rows)"""
    kernel_meta.no_scratch("recur.hip", kernel_meta.recurrence_entry_points(kernel_meta.FORM_SEGS))
    kernel_meta.no_scratch("kernels.hip", ("k_layernorm_gather",))
