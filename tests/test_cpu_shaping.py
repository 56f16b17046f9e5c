"""Typical-p and top-n-sigma in the device sampler (rwkv_mi_*shaping_set / _get), without a GPU: the libraries export the four entry points,
the test hook lives in a library of its own whose header declares exactly that one entry, the binding declares everything,
tests/shape_ref.py -- the host statement tests/test_gpu_shaping.py holds the device to -- gives the hand-written answers, every case of the
device's table lies clear of the decisions the device takes in f32, and the kernels that got the two stages keep within a 1024-thread
workgroup's budget."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import kernel_meta
import shape_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"rwkv_mi_batch_shaping_set": 4, "rwkv_mi_batch_shaping_get": 4, "rwkv_mi_shaping_set": 3, "rwkv_mi_shaping_get": 3}
HOOK = "rwkv_mi_test_shape_rows"
# every form of k_draw<SRC, CUT> and k_draw_rows<SRC, CUT, GUIDED> with CUT = 1, and the three drawing families of the draft walk
KERNELS = (*(("k_draw", (src, 1)) for src in (0, 1, 2)), *(("k_draw_rows", (src, 1, g)) for src in (0, 1, 2) for g in (0, 1)),
           *(("k_draft_accept_rows", (f,)) for f in (1, 2, 3)))


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


def test_symbols_hook_library_and_binding():
    pkg = _pkg()
    declared = _declared("rwkv_mi355x.h")
    lib = pkg.load_rwkv_shared_library()
    for name, n_args in SYMBOLS.items():
        assert name in declared and len(declared[name].split(",")) == n_args, name
        f = getattr(lib.library, name)
        assert f.restype is ctypes.c_bool and len(f.argtypes) == n_args, name
    # only the shape library exports the hook, beside exactly the product's surface
    assert os.path.dirname(pkg.SHAPE_HOOKS_LIB_PATH) == os.path.dirname(pkg.LIB_PATH)
    for path in (pkg.LIB_PATH, pkg.HOOKS_LIB_PATH, pkg.SAMPLE_HOOKS_LIB_PATH, pkg.GUIDE_HOOKS_LIB_PATH, pkg.CUT_HOOKS_LIB_PATH, pkg.DECAY_HOOKS_LIB_PATH):
        assert not hasattr(ctypes.CDLL(path), HOOK), path
    assert list(_declared("rwkv_testhooks_shape.h")) == [HOOK]
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.SHAPE_HOOKS_LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert exported == set(_declared("rwkv.h")) | set(declared) | {HOOK}
    f = getattr(pkg.RWKVSharedLibrary(pkg.SHAPE_HOOKS_LIB_PATH).library, HOOK)
    assert f.restype is ctypes.c_bool and len(f.argtypes) == len(_declared("rwkv_testhooks_shape.h")[HOOK].split(",")) == 9
    # struct rwkv_mi_test_shape { uint32_t top_k; float min_p; float typical_p; float n_sigma; }
    assert ctypes.sizeof(pkg.ShapeParams) == 16 and [getattr(pkg.ShapeParams, n).offset for n, _ in pkg.ShapeParams._fields_] == [0, 4, 8, 12]
    for cls in (pkg.RWKVBatch, pkg.RWKVModel):
        for meth in ("set_shaping", "shaping"):
            assert callable(getattr(cls, meth)), (cls, meth)


def test_shape_ref_on_hand_written_cases():
    inf, nan = np.inf, np.nan
    p, s = S.typical_keys(S.HAND)
    H = float(-(p * np.log(p)).sum())
    assert abs(H - 1.392) < 1e-3 and np.allclose(s, [0.476, 0.188, 0.505, 0.910, 1.603], atol=1e-3)
    # the most typical token is not the most probable one
    for tp, want in ((0.2, [1]), (0.5, [0, 1]), (0.75, [0, 1, 2])):
        assert np.flatnonzero(S.typical_mask(S.HAND, tp)).tolist() == want, tp
    m = S.masked(S.HAND, 0, 0.2, 0.0)
    assert m.dtype == np.float32 and m.tolist() == [-inf, float(S.HAND[1]), -inf, -inf, -inf]
    # equal keys at the boundary stay together: the twins 1 and 3 lie nearest the entropy, and 0.1 is exceeded only by both
    v = np.log(np.array([0.5, 0.2, 0.1, 0.2])).astype(np.float32)
    assert np.flatnonzero(S.typical_mask(v, 0.1)).tolist() == [1, 3]
    # a row of equal values has one key
    for tp in (0.01, 0.5, 0.99):
        assert S.typical_mask(np.full(9, 0.25, dtype=np.float32), tp).all()
    # -inf and NaN: no mass and no key; {0, 0} and typical_p = 1 keep all
    v = np.array([S.HAND[0], -inf, S.HAND[1], nan, S.HAND[2], S.HAND[3], S.HAND[4]], dtype=np.float32)
    assert np.flatnonzero(S.typical_mask(v, 0.5)).tolist() == [0, 2]
    for tp, ns in ((0.0, 0.0), (1.0, 0.0)):
        assert S.kept(v, 0, tp, ns).all()
    # n-sigma: the statistics are the finite values' -- max 4, mean 2, sigma sqrt(2) -- whatever else the row holds
    v = np.array([4.0, -inf, 3.0, nan, 2.0, 1.0, 0.0, inf], dtype=np.float32)
    assert abs(S.n_sigma_floor(v, 1.0) - (4.0 - np.sqrt(2.0))) < 1e-12
    assert np.flatnonzero(S.n_sigma_mask(v, 1.0)).tolist() == [0, 2, 7] and np.flatnonzero(S.n_sigma_mask(v, 1.5)).tolist() == [0, 2, 4, 7]
    assert S.n_sigma_mask(np.full(7, -1.5, dtype=np.float32), 3.0).all()
    # the floor is taken before top-k and typical-p on what both leave: floor {4, 3}, top-k 1 {4}; the floor and top-k commute
    assert np.flatnonzero(S.kept(v[:7], 1, 0.0, 1.0)).tolist() == [0]
    assert np.flatnonzero(S.kept(S.HAND, 3, 0.75, 0.0)).tolist() == [0, 1]   # (of {0.4, 0.3, 0.15} / 0.85: keys 0.27, 0.01, 0.71)


@pytest.mark.parametrize("name,row", S.cases(), ids=[c[0] for c in S.cases()])
def test_every_device_case_is_clear_of_its_decisions(name, row):
    """The condition on the inputs that lets tests/test_gpu_shaping.py compare exactly: the device takes the floor, the masses and the keys
    in f32 (relative error some 1e-6), so a case is admitted only when every decision has 1e-3 to spare."""
    for setting in S.SETTINGS:
        assert min(S.case_clearances(row, setting)) >= 1e-3, (name, setting, S.case_clearances(row, setting))
        assert S.kept(row, setting[0], setting[2], setting[3]).any()


@pytest.mark.skipif(not kernel_meta.have_hipcc(), reason="needs hipcc")
def test_shaping_entry_points_keep_the_budget():
    found = kernel_meta.budget("sampling.hip", KERNELS)
    # the stages' LDS -- 16 histograms of 256 64-bit bins and three bodies -- fits a workgroup's 64 KB
    assert all(32768 < k.lds <= 65536 for k in found.values()), found
