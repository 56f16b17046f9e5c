"""Penalty decay and repetition penalty in the device sampler (rwkv_mi_*repetition_set / _get, rwkv_mi_*counts_store_f32), without a GPU: the
libraries export the six entry points, the test hooks live in a library of their own whose header declares exactly those, the binding declares
everything, tests/decay_ref.py -- the host statements tests/test_gpu_decay.py holds the device to -- gives the hand-written answers, and every
new entry point of csrc/sampling.hip keeps within a 1024-thread workgroup's budget."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import kernel_meta

import decay_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"rwkv_mi_batch_repetition_set": 4, "rwkv_mi_batch_repetition_get": 4, "rwkv_mi_batch_counts_store_f32": 3,
           "rwkv_mi_repetition_set": 3, "rwkv_mi_repetition_get": 3, "rwkv_mi_counts_store_f32": 2}
HOOKS = {"rwkv_mi_test_decay_rows": 11, "rwkv_mi_test_decay_counts_add": 5}
# the repetition source (SRC = 2) of k_draw<SRC, CUT>, k_draw_rows<SRC, CUT, GUIDED> and the draft walk (FAMILY = 1 + SRC): what k_rep_pen_sample,
# k_rep_pen_sample_rows, k_guided_rep_pen_sample_rows and k_rep_draft_accept_rows were
KERNELS = (("k_draw", (2, 1)), ("k_draw_rows", (2, 1, 0)), ("k_draw_rows", (2, 1, 1)), ("k_draft_accept_rows", (3,)))
F = np.float32


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


def test_header_and_product_library_have_the_six_symbols():
    pkg = _pkg()
    declared = _declared("rwkv_mi355x.h")
    so = ctypes.CDLL(pkg.LIB_PATH)
    for name, n_args in SYMBOLS.items():
        assert name in declared and len(declared[name].split(",")) == n_args, name
        assert hasattr(so, name), name


def test_only_the_decay_library_exports_the_hooks():
    pkg = _pkg()
    assert os.path.dirname(pkg.DECAY_HOOKS_LIB_PATH) == os.path.dirname(pkg.LIB_PATH)
    for path in (pkg.LIB_PATH, pkg.HOOKS_LIB_PATH, pkg.SAMPLE_HOOKS_LIB_PATH, pkg.GUIDE_HOOKS_LIB_PATH, pkg.CUT_HOOKS_LIB_PATH):
        so = ctypes.CDLL(path)
        for hook in HOOKS:
            assert not hasattr(so, hook), (path, hook)
    assert set(_declared("rwkv_testhooks_decay.h")) == set(HOOKS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.DECAY_HOOKS_LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert exported == set(_declared("rwkv.h")) | set(_declared("rwkv_mi355x.h")) | set(HOOKS)


def test_binding_declares_everything():
    pkg = _pkg()
    lib = pkg.load_rwkv_shared_library()
    for name, n_args in SYMBOLS.items():
        f = getattr(lib.library, name)
        assert f.restype is ctypes.c_bool and len(f.argtypes) == n_args, name
    hooks = pkg.RWKVSharedLibrary(pkg.DECAY_HOOKS_LIB_PATH)
    declared = _declared("rwkv_testhooks_decay.h")
    for hook, n_args in HOOKS.items():
        f = getattr(hooks.library, hook)
        assert f.restype is ctypes.c_bool and len(f.argtypes) == len(declared[hook].split(",")) == n_args, hook
    # struct rwkv_mi_test_rep { float decay; float repetition; }
    assert ctypes.sizeof(pkg.RepParams) == 8 and [pkg.RepParams.decay.offset, pkg.RepParams.repetition.offset] == [0, 4]
    for cls in (pkg.RWKVBatch, pkg.RWKVModel):
        for meth in ("set_repetition", "repetition", "counts_f32"):
            assert callable(getattr(cls, meth)), (cls, meth)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def test_decay_ref_on_hand_written_cases():
    inf, nan = np.inf, np.nan
    # positive divides, everything else multiplies; the penalty follows; a token that has not occurred keeps its logit
    l = np.array([2.0, -2.0, 0.0, -0.0, -inf, nan, 3.0, 2.0], dtype=np.float32)
    o = D.words_of(np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 2.5], dtype=np.float32))
    a = D.adjusted(l, o, 0.5, 0.25, 0.5, 2.0)
    # 2 / 2 - (0.5 + 0.25);  -2 * 2 - 0.75;  0 * 2 - 0.75;  -0 * 2 - 0.75;  -inf;  NaN;  untouched;  2 / 2 - (0.5 + 2.5 * 0.25)
    want = np.array([0.25, -4.75, -0.75, -0.75, -inf, nan, 3.0, -0.125], dtype=np.float32)
    assert np.array_equal(_bits(a), _bits(want)), a.tolist()
    # the bias comes last, on every token
    b = D.adjusted(l, o, 0.5, 0.25, 0.5, 2.0, bias=np.full(8, 1.0, dtype=np.float32))
    assert np.array_equal(_bits(b[[0, 6]]), _bits(np.array([1.25, 4.0], dtype=np.float32)))
    # the setting none on a row of counts is the penalised draw: l - (presence + count * frequency)
    c = np.array([0, 3, 1, 0, 0, 0, 0, 0], dtype=np.uint32)
    n = D.adjusted(l, c, 0.2, 0.2, 1.0, 1.0)
    ref = l.copy()
    ref[1] = F(-2.0) - (F(0.2) + F(3.0) * F(0.2))
    ref[2] = F(0.0) - (F(0.2) + F(1.0) * F(0.2))
    assert np.array_equal(_bits(n), _bits(ref))
    # every operation is rounded to float32 on its own: 1/3 * 3 in float32, not in double
    x = D.adjusted(np.array([1.0], dtype=np.float32), D.words_of(np.array([3.0], dtype=np.float32)), 0.0, 1.0 / 3.0, 0.5, 3.0)
    assert x[0] == F(F(1.0) / F(3.0)) - (F(0.0) + F(3.0) * F(1.0 / 3.0))
    # a subnormal occurrence is an occurrence: it takes the presence penalty (and a frequency term that rounds away)
    tiny = np.array([1], dtype=np.uint32)   # the smallest subnormal, 2^-149
    s = D.adjusted(np.array([1.0], dtype=np.float32), tiny, 0.5, 0.25, 0.5, 1.0)
    assert D.occurrences(tiny, 0.5)[0] > 0 and s[0] == F(0.5)
    # ... and one that has underflowed to 0 is a token that has not occurred
    assert D.adjusted(np.array([1.0], dtype=np.float32), np.array([0], dtype=np.uint32), 0.5, 0.25, 0.5, 2.0)[0] == F(1.0)
    # 2^24 as a count and as a float: the same value; as a count it no longer grows as a float, as a float + 1 is absorbed
    big = np.array([1 << 24], dtype=np.uint32)
    assert D.occurrences(big, 1.0)[0] == F(16777216.0) == D.occurrences(D.words_of(np.array([16777216.0], dtype=np.float32)), 0.5)[0]
    assert D.recorded(big, 1.0, 0)[0] == (1 << 24) + 1
    assert D.recorded(D.words_of(np.array([16777216.0], dtype=np.float32)), 0.999, 0).view(np.float32)[0] == F(F(16777216.0) * F(0.999)) + F(1.0)


def test_decay_ref_table_rules():
    # a recorded draw decays every entry, then counts the pick; one that does not record leaves the row alone
    o = D.words_of(np.array([1.0, 0.0, 2.0], dtype=np.float32))
    r = D.recorded(o, 0.5, 1).view(np.float32)
    assert r.tolist() == [0.5, 1.0, 1.0]
    assert np.array_equal(D.recorded(o, 0.5, 1, record=False), o)
    assert D.recorded(np.array([4, 0, 1], dtype=np.uint32), 1.0, 2).tolist() == [4, 0, 2]
    # decay 0 keeps only the last token
    assert D.recorded(o, 0.0, 2).view(np.float32).tolist() == [0.0, 0.0, 1.0]
    # counts_add is the draws in order: 0.996 three times is not 0.996 ** 3 in one rounding
    w = D.counts_add(np.zeros(4, dtype=np.uint32), 0.996, [2, 2, 1, 3]).view(np.float32)
    d = F(0.996)
    assert w[2] == ((F(1.0) * d + F(1.0)) * d) * d and w[1] == F(1.0) * d and w[3] == F(1.0) and w[0] == F(0.0)
    # 200 halvings pass through the subnormals to 0: 1 -> 2^-149 after 149 more tokens, 0 after 150
    row = D.counts_add(np.zeros(8, dtype=np.uint32), 0.5, [5] + [0] * 149).view(np.float32)
    assert row[5] == F(2.0 ** -149) and row.view(np.uint32)[5] == 1
    row = D.counts_add(D.words_of(row), 0.5, [0]).view(np.float32)
    assert row[5] == F(0.0) and row[0] > F(1.99)


@pytest.mark.skipif(not kernel_meta.have_hipcc(), reason="needs hipcc")
def test_new_entry_points_keep_the_budget():
    kernel_meta.budget("sampling.hip", KERNELS)
    # the decaying count kernel: one thread per entry
    assert re.search(r"\dk_count_add_decayEPf", kernel_meta.kernels("sampling.hip")["k_count_add_decay"].name)
