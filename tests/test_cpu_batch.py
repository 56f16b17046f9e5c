"""Batched decode without a GPU: the library exports the rwkv_mi_batch_* entry points, the Python binding declares them, and no row kernel
of csrc/recur.hip uses scratch memory (the same metadata read as test_cpu_kernel_budget.py)."""
import ctypes
import os

import pytest

import kernel_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


@pytest.mark.skipif(not kernel_meta.have_hipcc(), reason="needs hipcc")
def test_row_entry_points_have_no_private_segment():
    """the ROWS form of every recurrence, and the argmax kernels of the greedy loops (one workgroup per row)"""
    kernel_meta.no_scratch("recur.hip", kernel_meta.recurrence_entry_points(kernel_meta.FORM_ROWS))
    kernel_meta.no_scratch("kernels.hip", ("k_argmax", "k_argmax_live"))
