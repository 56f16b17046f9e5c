"""Speculative decoding (rwkv_mi_batch_eval_draft), without a GPU: the header declares the entry point and its limit, all four libraries export
it, the binding declares it with the header's argument count, lookup_draft -- the prompt-lookup drafter the binding offers callers -- does what
its statement says on hand-written histories, and the device-only compile of csrc/sampling.hip and csrc/kernels.hip shows the accept kernel and
every replay kernel without a private segment or spills, the accept kernel within a 1024-thread workgroup's 128 registers."""
import ctypes
import os
import re

import pytest

import kernel_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL, N_ARGS = "rwkv_mi_batch_eval_draft", 11
ACCEPT = "k_draft_accept_rows"
REPLAY = ("k_wkv4_replay", "k_wkv6_replay", "k_wkv6_replay_generic", "k_wkv7_replay", "k_wkv7_replay_generic", "k_draft_carry", "k_draft_stash")


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


def test_header_declares_the_draft_call_and_its_limit():
    declared = _declared("rwkv_mi355x.h")
    assert SYMBOL in declared
    assert len(declared[SYMBOL].split(",")) == N_ARGS, declared[SYMBOL]
    header = open(os.path.join(ROOT, "include", "rwkv_mi355x.h")).read()
    assert re.search(r"#define\s+RWKV_MI_DRAFT_MAX\s+8\b", header)


def test_all_four_libraries_export_the_draft_call():
    pkg = _pkg()
    for path in (pkg.LIB_PATH, pkg.HOOKS_LIB_PATH, pkg.SAMPLE_HOOKS_LIB_PATH, pkg.GUIDE_HOOKS_LIB_PATH):
        assert hasattr(ctypes.CDLL(path), SYMBOL), path


def test_binding_declares_the_draft_call():
    pkg = _pkg()
    lib = pkg.load_rwkv_shared_library()
    f = getattr(lib.library, SYMBOL)
    assert f.restype is ctypes.c_bool and len(f.argtypes) == N_ARGS
    assert callable(pkg.RWKVBatch.eval_draft)
    assert pkg.DRAFT_MAX == 8


def test_lookup_draft_on_hand_written_histories():
    pkg = _pkg()
    look = pkg.lookup_draft
    # a repeat is found: the tail 1 2 3 occurred before, followed by 4 5 6
    assert look([1, 2, 3, 4, 5, 6, 7, 1, 2, 3], 3) == [4, 5, 6]
    assert look([1, 2, 3, 4, 5, 6, 7, 1, 2, 3], 8) == [4, 5, 6, 7, 1, 2, 3]
    # the most recent earlier occurrence wins
    assert look([1, 2, 3, 9, 9, 1, 2, 3, 8, 8, 1, 2, 3], 2) == [8, 8]
    # shorter than k where the history ends first
    assert look([5, 6, 7, 1, 5, 6, 7], 4) == [1, 5, 6, 7]
    assert look([5, 6, 7, 5, 6, 7], 4) == [5, 6, 7]
    assert look([4, 4, 4, 4], 8, ngram=3) == [4]          # (overlapping occurrences: the one that starts one token earlier)
    # another n-gram length
    assert look([1, 2, 9, 3, 2], 2, ngram=1) == [9, 3]
    assert look([1, 2, 9, 3, 2], 2, ngram=2) == []
    # no match, too short a history, nothing asked for
    assert look([1, 2, 3, 4, 5, 6], 4) == []
    assert look([1, 2, 3], 4) == []
    assert look([1, 2], 4) == []
    assert look([], 4) == []
    assert look([1, 2, 3, 4, 1, 2, 3], 0) == []
    # a draft is a list of ints whatever the history was
    import numpy as np
    d = look(np.array([1, 2, 3, 4, 1, 2, 3], dtype=np.uint32), 1)
    assert d == [4] and type(d[0]) is int


@pytest.mark.skipif(not kernel_meta.have_hipcc(), reason="needs hipcc")
def test_accept_kernel_keeps_the_budget():
    """the families of k_draft_accept_rows -- greedy, sampled, penalised and (the fourth, k_rep_draft_accept_rows before the walk was one
    template) penalised with a repetition setting: 1024 threads, so 128 registers per thread, no spills, no private segment"""
    families = kernel_meta.named("sampling.hip", ACCEPT)
    assert set(families) == {(0,), (1,), (2,), (3,)}, families
    kernel_meta.budget("sampling.hip", tuple((ACCEPT, f) for f in families))


@pytest.mark.skipif(not kernel_meta.have_hipcc(), reason="needs hipcc")
def test_replay_kernels_have_no_private_segment_and_no_spills():
    """every entry point of the replay -- the fourth over each WKV body, templated and generic -- and the two copy kernels beside them"""
    seen = {k: kernel_meta.named("kernels.hip", k) for k in REPLAY}
    for k, forms in seen.items():
        assert forms, (k, seen)
        for kern in forms.values():
            print(kern)
            assert kern.private == 0 and kern.spills == 0, kern
    assert len(seen["k_wkv6_replay"]) == 4 and len(seen["k_wkv7_replay"]) == 2, seen   # head sizes 64, 32, 16, 8 and 64, 32
