"""Guided decoding (rwkv_mi_batch_guide_*), without a GPU: the header declares the four entry points and their limits, the libraries export
them, the binding declares them with the header's argument counts, the guided sampler's test hook lives in a library of its own whose header
declares exactly that one entry, csrc/sampling.hip's two guided row kernels and k_guide_expand keep within a 1024-thread workgroup's budget,
and tests/guide_ref.py -- the host statement of a guide that tests/test_gpu_guide.py holds the device to -- is consistent with itself."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import kernel_meta

import guide_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"rwkv_mi_batch_guide_create": 6, "rwkv_mi_batch_guide_free": 2, "rwkv_mi_batch_guide_attach": 4, "rwkv_mi_batch_guide_state": 5}
HOOK = "rwkv_mi_test_guided_rows"
# the guided forms of k_draw_rows<SRC, CUT, GUIDED> on the plain (0) and the penalised (1) source: what k_guided_sample_rows and
# k_guided_pen_sample_rows were
KERNELS = (("k_draw_rows", (0, 1, 1)), ("k_draw_rows", (1, 1, 1)))


def _pkg():
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    pkg = graft.load_package()
    pkg.build_library()
    return pkg


@pytest.fixture(autouse=True, scope="module")
def _guide_symbols():
    """Everything here, the host statement included, is about the guide calls: a library without them fails every test of this file."""
    so = ctypes.CDLL(_pkg().LIB_PATH)
    missing = [name for name in SYMBOLS if not hasattr(so, name)]
    assert not missing, missing


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"RWKV_API[^;(]*?\b(rwkv_\w+)\s*\(([^;]*)\)\s*;", text)}


def test_header_declares_the_guide_symbols_and_limits():
    declared = _declared("rwkv_mi355x.h")
    for name, n_args in SYMBOLS.items():
        assert name in declared, name
        assert len(declared[name].split(",")) == n_args, (name, declared[name])
    header = open(os.path.join(ROOT, "include", "rwkv_mi355x.h")).read()
    for macro, value in (("RWKV_MI_GUIDE_MAX", "16"), ("RWKV_MI_GUIDE_MAX_STATES", "65535"), ("RWKV_MI_NO_GUIDE", "UINT32_MAX")):
        assert re.search(r"#define\s+" + macro + r"\s+" + value + r"\b", header), macro


def test_libraries_export_the_guide_symbols_and_only_the_guide_library_the_hook():
    pkg = _pkg()
    for path in (pkg.LIB_PATH, pkg.HOOKS_LIB_PATH, pkg.SAMPLE_HOOKS_LIB_PATH, pkg.GUIDE_HOOKS_LIB_PATH):
        so = ctypes.CDLL(path)
        for name in SYMBOLS:
            assert hasattr(so, name), (path, name)
    assert os.path.dirname(pkg.GUIDE_HOOKS_LIB_PATH) == os.path.dirname(pkg.SAMPLE_HOOKS_LIB_PATH)
    assert hasattr(ctypes.CDLL(pkg.GUIDE_HOOKS_LIB_PATH), HOOK)
    for path in (pkg.LIB_PATH, pkg.HOOKS_LIB_PATH, pkg.SAMPLE_HOOKS_LIB_PATH):
        assert not hasattr(ctypes.CDLL(path), HOOK), path
    # the hook's header declares exactly its one entry
    hook = _declared("rwkv_testhooks_guide.h")
    assert list(hook) == [HOOK], sorted(hook)
    # the guide library: the declared surface and that entry, nothing else
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.GUIDE_HOOKS_LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert exported == set(_declared("rwkv.h")) | set(_declared("rwkv_mi355x.h")) | {HOOK}


def test_binding_declares_the_guide_symbols():
    pkg = _pkg()
    lib = pkg.load_rwkv_shared_library()
    for name, n_args in SYMBOLS.items():
        f = getattr(lib.library, name)
        assert f.restype is ctypes.c_bool and len(f.argtypes) == n_args, name
    hooks = pkg.RWKVSharedLibrary(pkg.GUIDE_HOOKS_LIB_PATH)
    f = getattr(hooks.library, HOOK)
    assert f.restype is ctypes.c_bool and len(f.argtypes) == len(_declared("rwkv_testhooks_guide.h")[HOOK].split(",")) == 18
    assert (pkg.NO_GUIDE, pkg.GUIDE_MAX, pkg.GUIDE_MAX_STATES) == (0xFFFFFFFF, 16, 65535)
    for meth in ("create_guide", "free_guide", "attach_guide", "detach_guide", "guide_state"):
        assert callable(getattr(pkg.RWKVBatch, meth)), meth
    # the binding's CSR form is the reference's
    g = G.random_guide(97, 5, seed=3)
    for a, b in zip(pkg.guide_edges(g.edges), g.csr()):
        assert a.dtype == np.uint32 and np.array_equal(a, b)


def test_random_guide_has_an_edge_in_every_state_and_is_seeded():
    for V, S, allow in ((1000, 7, 0.5), (50, 3, 0.0), (65536, 2, 0.5)):
        g = G.random_guide(V, S, seed=11, allow=allow)
        G.check(g)
        assert g.n_states == S and all(len(e) >= 1 for e in g.edges)
        assert g.edges == G.random_guide(V, S, seed=11, allow=allow).edges
        assert g.edges != G.random_guide(V, S, seed=12, allow=allow).edges
        if allow == 0.5:
            assert all(0.4 * V < len(e) < 0.6 * V for e in g.edges)


def test_mask_step_walk_and_tables_agree():
    g = G.random_guide(300, 6, seed=5)
    begin, toks, nxt = g.csr()
    dense = g.dense()
    assert begin[0] == 0 and begin.size == g.n_states + 1 and toks.size == nxt.size == begin[-1]
    for s in range(g.n_states):
        m = g.mask(s)
        mine = toks[begin[s]:begin[s + 1]]
        assert np.all(np.diff(mine.astype(np.int64)) > 0), "tokens strictly ascending"
        assert np.array_equal(np.flatnonzero(m), mine)
        assert np.array_equal(dense[s] != 0xFFFF, m)
        assert np.array_equal(dense[s][m], nxt[begin[s]:begin[s + 1]])
        for t in (0, 1, 150, 299):
            to, miss = g.step(s, t)
            assert (to, miss) == ((int(dense[s, t]), 0) if m[t] else (s, 1))
    s0 = 2
    allowed = []
    s = s0
    for _ in range(20):   # a walk over allowed tokens never misses ...
        t = min(g.edges[s])
        allowed.append(t)
        s = g.edges[s][t]
    assert g.walk(s0, allowed) == (s, 0)
    dead = next(t for t in range(300) if not g.mask(s0)[t])
    assert g.walk(s0, [dead, dead]) == (s0, 2)   # ... a dead token stays and counts


def test_chain_guide_forces_its_string():
    text = [5, 0, 299, 5, 17]
    g = G.chain_guide(300, text)
    assert g.n_states == len(text)
    s = 0
    for i in range(3 * len(text)):
        m = g.mask(s)
        assert m.sum() == 1 and m[text[i % len(text)]]
        s, miss = g.step(s, text[i % len(text)])
        assert miss == 0 and s == (i + 1) % len(text)


def test_all_allowed_guide_masks_nothing():
    g = G.all_allowed_guide(50, 3)
    for s in range(3):
        assert g.mask(s).all()
        assert g.step(s, 7) == ((s + 7) % 3, 0)
    assert (g.dense() != 0xFFFF).all()


def test_bad_guides_fail_the_check():
    with pytest.raises(AssertionError):
        G.Guide([{1: 0}, {}], 10)          # a state without an edge
    with pytest.raises(AssertionError):
        G.Guide([{10: 0}], 10)             # a token out of range
    with pytest.raises(AssertionError):
        G.Guide([{1: 1}], 10)              # a next state out of range


@pytest.mark.skipif(not kernel_meta.have_hipcc(), reason="needs hipcc")
def test_guided_entry_points_keep_the_budget():
    kernel_meta.budget("sampling.hip", KERNELS)
    kernel_meta.budget("sampling.hip", ("k_guide_expand",), wg=256)
