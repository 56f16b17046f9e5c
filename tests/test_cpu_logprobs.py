"""The log-prob report (rwkv_mi_*set_logprobs / _logprobs_shape / _logprobs_store), without a GPU: the header declares the calls, the
libraries export them, the binding wires their argument types, the kernel's test hook lives in the sample-hooks library only, and the ordering
reference the GPU tests hold the device to orders a hand-written row as the header states."""
import ctypes
import os
import re

import numpy as np

from logprobs_ref import NO_TOKEN, f64_logprobs, top_ids

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rwkv_mi_batch_set_logprobs", "rwkv_mi_batch_logprobs_shape", "rwkv_mi_batch_logprobs_store",
           "rwkv_mi_set_logprobs", "rwkv_mi_logprobs_shape", "rwkv_mi_logprobs_store")
HOOK = "rwkv_test_logprob_rows"


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


def test_headers_declare_the_calls():
    assert set(SYMBOLS) <= _declared("rwkv_mi355x.h")
    assert _declared("rwkv_testhooks_logprobs.h") == {HOOK}
    header = open(os.path.join(ROOT, "include", "rwkv_mi355x.h")).read()
    assert re.search(r"#define\s+RWKV_MI_TOP_MAX\s+20\b", header)


def test_libraries_export_them_and_the_hook_stays_out_of_the_product():
    pkg = _pkg()
    for path in (pkg.LIB_PATH, pkg.HOOKS_LIB_PATH, pkg.SAMPLE_HOOKS_LIB_PATH):
        so = ctypes.CDLL(path)
        for name in SYMBOLS:
            assert hasattr(so, name), (path, name)
    assert hasattr(ctypes.CDLL(pkg.SAMPLE_HOOKS_LIB_PATH), HOOK)
    assert not hasattr(ctypes.CDLL(pkg.LIB_PATH), HOOK) and not hasattr(ctypes.CDLL(pkg.HOOKS_LIB_PATH), HOOK)


def test_binding_wires_the_argument_types():
    pkg = _pkg()
    lib = pkg.load_rwkv_shared_library()
    for name in SYMBOLS:
        f = getattr(lib.library, name)
        assert f.argtypes is not None and f.restype is ctypes.c_bool, name
        assert len(f.argtypes) == (3 if name.endswith("set_logprobs") else 4 if name.endswith("shape") else 5), name
    hooks = pkg.RWKVSharedLibrary(pkg.SAMPLE_HOOKS_LIB_PATH)
    assert len(hooks.library.rwkv_test_logprob_rows.argtypes) == 8 and hooks.library.rwkv_test_logprob_rows.restype is ctypes.c_bool
    for cls in (pkg.RWKVModel, pkg.RWKVBatch):
        assert callable(cls.set_logprobs) and callable(cls.logprobs), cls


def test_the_ordering_reference_on_a_hand_written_row():
    nan, inf = float("nan"), float("inf")
    #        0     1    2     3    4     5    6     7     8     9
    row = [1.0, nan, 3.0, -inf, 3.0, -0.0, 0.0, -inf, nan, 2.5]
    # value descending, index ascending among equals; -0 ties with +0; -inf last among the rest; a NaN never ranks
    want = [2, 4, 9, 0, 5, 6, 3, 7]
    assert top_ids(row, 8).tolist() == want
    assert top_ids(row, 3).tolist() == want[:3]
    assert top_ids(row, 0).tolist() == []
    assert top_ids(row, 10).tolist() == want + [NO_TOKEN, NO_TOKEN]
    assert top_ids([nan, nan], 2).tolist() == [NO_TOKEN, NO_TOKEN]
    # the float64 log-probs of a row without NaN: exp of them adds up to 1; NO_TOKEN and -inf give -inf
    clean = np.array([1.0, 3.0, -inf, 3.0, 0.0], dtype=np.float32)
    lp = f64_logprobs(clean, [0, 1, 2, 3, 4, NO_TOKEN])
    assert abs(np.exp(lp[:5]).sum() - 1.0) < 1e-12 and lp[2] == -inf and lp[5] == -inf and lp[1] == lp[3]
