"""Top-k and min-p in the device sampler (rwkv_mi_*truncation_set / _get), without a GPU: the libraries export the four entry points, the test
hook lives in a library of its own whose header declares exactly that one entry, the binding declares everything, tests/cut_ref.py -- the host
statement tests/test_gpu_truncation.py holds the device to -- gives the hand-written answers, and every kernel of csrc/sampling.hip that
takes the truncation argument keeps within a 1024-thread workgroup's budget."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import kernel_meta

import cut_ref as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"rwkv_mi_batch_truncation_set": 4, "rwkv_mi_batch_truncation_get": 4, "rwkv_mi_truncation_set": 3, "rwkv_mi_truncation_get": 3}
HOOK = "rwkv_mi_test_cut_rows"
# the truncating forms (CUT = 1) of k_draw<SRC, CUT> and k_draw_rows<SRC, CUT, GUIDED> on the plain (0) and the penalised (1) source -- what
# k_cut_sample, k_cut_sample_rows, k_cut_pen_sample, k_cut_pen_sample_rows, k_guided_sample_rows and k_guided_pen_sample_rows were -- and the
# three families of the draft walk that were there when the setting came
KERNELS = (("k_draw", (0, 1)), ("k_draw_rows", (0, 1, 0)), ("k_draw", (1, 1)), ("k_draw_rows", (1, 1, 0)), ("k_draw_rows", (0, 1, 1)), ("k_draw_rows", (1, 1, 1)),
           ("k_draft_accept_rows", (0,)), ("k_draft_accept_rows", (1,)), ("k_draft_accept_rows", (2,)))


def _pkg():
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    pkg = graft.load_package()
    pkg.build_library()
    return pkg


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"RWKV_API[^;(]*?\b(rwkv_\w+)\s*\(([^;]*)\)\s*;", text)}


def test_header_and_product_library_have_the_four_symbols():
    pkg = _pkg()
    declared = _declared("rwkv_mi355x.h")
    so = ctypes.CDLL(pkg.LIB_PATH)
    for name, n_args in SYMBOLS.items():
        assert name in declared and len(declared[name].split(",")) == n_args, name
        assert hasattr(so, name), name


def test_only_the_cut_library_exports_the_hook():
    pkg = _pkg()
    assert os.path.dirname(pkg.CUT_HOOKS_LIB_PATH) == os.path.dirname(pkg.LIB_PATH)
    for path in (pkg.LIB_PATH, pkg.HOOKS_LIB_PATH, pkg.SAMPLE_HOOKS_LIB_PATH, pkg.GUIDE_HOOKS_LIB_PATH):
        assert not hasattr(ctypes.CDLL(path), HOOK), path
    assert list(_declared("rwkv_testhooks_cut.h")) == [HOOK]
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.CUT_HOOKS_LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert exported == set(_declared("rwkv.h")) | set(_declared("rwkv_mi355x.h")) | {HOOK}


def test_binding_declares_everything():
    pkg = _pkg()
    lib = pkg.load_rwkv_shared_library()
    for name, n_args in SYMBOLS.items():
        f = getattr(lib.library, name)
        assert f.restype is ctypes.c_bool and len(f.argtypes) == n_args, name
    hooks = pkg.RWKVSharedLibrary(pkg.CUT_HOOKS_LIB_PATH)
    f = getattr(hooks.library, HOOK)
    assert f.restype is ctypes.c_bool and len(f.argtypes) == len(_declared("rwkv_testhooks_cut.h")[HOOK].split(",")) == 9
    # struct rwkv_mi_test_cut { uint32_t top_k; float min_p; }
    assert ctypes.sizeof(pkg.CutParams) == 8 and [pkg.CutParams.top_k.offset, pkg.CutParams.min_p.offset] == [0, 4]
    for cls in (pkg.RWKVBatch, pkg.RWKVModel):
        for meth in ("set_truncation", "truncation"):
            assert callable(getattr(cls, meth)), (cls, meth)


def test_cut_ref_on_hand_written_cases():
    inf, nan = np.inf, np.nan
    # all equal: the lowest indices
    assert np.flatnonzero(C.top_k_mask(np.full(20, 0.25, dtype=np.float32), 7)).tolist() == list(range(7))
    # twin maxima, k = 1: the lower index
    v = np.array([0.0, 3.0, 1.0, 3.0, 2.0], dtype=np.float32)
    assert np.flatnonzero(C.top_k_mask(v, 1)).tolist() == [1]
    assert np.flatnonzero(C.top_k_mask(v, 3)).tolist() == [1, 3, 4]
    # a NaN in the top is skipped
    v = np.array([1.0, nan, 5.0, 4.0, -1.0], dtype=np.float32)
    assert np.flatnonzero(C.top_k_mask(v, 2)).tolist() == [2, 3]
    assert C.rank_order(v).tolist() == [2, 3, 0, 4]
    m = C.masked(v, 2)
    assert m.dtype == np.float32 and m.tolist() == [-inf, -inf, 5.0, 4.0, -inf]
    # -inf fills up last, by index; +0 and -0 are one value
    v = np.array([-inf, 2.0, -inf, 1.0, -inf], dtype=np.float32)
    assert np.flatnonzero(C.top_k_mask(v, 4)).tolist() == [0, 1, 2, 3]
    v = np.array([-0.0, 0.0, -1.0, 0.0], dtype=np.float32)
    assert np.flatnonzero(C.top_k_mask(v, 2)).tolist() == [0, 1]
    # k >= n and k == 0 keep all
    v = np.array([1.0, 2.0, 3.0], dtype=np.float32)
    for k in (0, 3, 4, 1 << 31):
        assert C.top_k_mask(v, k).all()


def test_reference_distribution_takes_both_thresholds_on_the_survivors():
    lg = np.log(np.array([0.4, 0.3, 0.15, 0.1, 0.05])).astype(np.float32)
    # top-k 3: {0.4, 0.3, 0.15} / 0.85; top-p 0.8 on THAT distribution keeps 0.4706 + 0.3529 (cumulative 0.8235 first exceeds 0.8)
    p = C.ref_distribution_cut(lg, 1.0, 0.8, 3, 0.0)
    assert np.flatnonzero(p).tolist() == [0, 1] and abs(p[0] - 4.0 / 7.0) < 1e-6
    # min-p 0.3: p >= 0.3 * p_max = 0.12 keeps three; intersected with top-p 0.6 (keeps two)
    assert np.flatnonzero(C.ref_distribution_cut(lg, 1.0, 1.0, 0, 0.3)).tolist() == [0, 1, 2]
    assert np.flatnonzero(C.ref_distribution_cut(lg, 1.0, 0.6, 0, 0.3)).tolist() == [0, 1]
    # the temperature comes last: the support does not move, the weights do
    q = C.ref_distribution_cut(lg, 0.5, 1.0, 0, 0.3)
    assert np.flatnonzero(q).tolist() == [0, 1, 2] and abs(q[0] / q[1] - (0.4 / 0.3) ** 2) < 1e-5
    assert C.ref_distribution_cut(lg, 0.0, 0.5, 2, 0.5).tolist() == [1.0, 0.0, 0.0, 0.0, 0.0]
    # a min_p in a gap is clear of every ratio; a row of equal values has no gap
    mp = C.min_p_in_a_gap(lg, 0.2)
    assert 0.125 < mp < 0.25 and C.clearance(lg, mp) > 1e-4
    assert C.min_p_in_a_gap(np.full(9, 0.25, dtype=np.float32), 0.05) is None


@pytest.mark.skipif(not kernel_meta.have_hipcc(), reason="needs hipcc")
def test_truncating_entry_points_keep_the_budget():
    kernel_meta.budget("sampling.hip", KERNELS)
