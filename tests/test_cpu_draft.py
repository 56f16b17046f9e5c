"""Speculative decoding (rwkv_mi_batch_eval_draft), without a GPU: the header declares the entry point and its limit, all four libraries export
it, the binding declares it with the header's argument count, lookup_draft -- the prompt-lookup drafter the binding offers callers -- does what
its statement says on hand-written histories, and the device-only compile of csrc/sampling.hip and csrc/kernels.hip shows the accept kernel and
every replay kernel without a private segment or spills, the accept kernel within a 1024-thread workgroup's 128 registers."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
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


def _kernel_meta(src_name, tmp_path):
    src = os.path.join(ROOT, "rwkv.cpp_amd", "csrc", src_name)
    out = str(tmp_path / (src_name + ".s"))
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-DRWKV_SHARED", "-DRWKV_BUILD",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rwkv.cpp_amd", "csrc"), "-S", "--cuda-device-only", src, "-o", out]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels"):]
    rows = []
    for m in re.finditer(r"\.max_flat_workgroup_size:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)",
                         meta, re.S):
        rows.append((m.group(2), int(m.group(1)), int(m.group(3)), int(m.group(4)), int(m.group(5))))
    return rows


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_accept_kernel_keeps_the_budget(tmp_path):
    """the three families of k_draft_accept_rows: 1024 threads, so 128 registers per thread, no spills, no private segment"""
    seen = set()
    for name, wg, private, vgprs, spills in _kernel_meta("sampling.hip", tmp_path):
        m = re.search(r"\d" + ACCEPT + r"ILi(\d)EEEv", name)
        if not m:
            continue
        seen.add(int(m.group(1)))
        print(name, wg, private, vgprs, spills)
        assert private == 0 and spills == 0, (name, private, vgprs, spills)
        assert vgprs <= 128, (name, vgprs, "1024 threads per workgroup leave 128 registers per thread")
        assert wg == 1024, (name, wg)
    assert seen == {0, 1, 2}, seen


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_replay_kernels_have_no_private_segment_and_no_spills(tmp_path):
    """every entry point of the replay -- the fourth over each WKV body, templated and generic -- and the two copy kernels beside them"""
    seen = {}
    for name, wg, private, vgprs, spills in _kernel_meta("kernels.hip", tmp_path):
        for k in REPLAY:
            if re.search(r"\d" + k + r"(ILi\d+EEEv|E[Pv]|ENS_)", name):
                seen.setdefault(k, []).append(name)
                print(name, wg, private, vgprs, spills)
                assert private == 0 and spills == 0, (name, private, vgprs, spills)
    assert set(seen) == set(REPLAY), seen
    assert len(seen["k_wkv6_replay"]) == 4 and len(seen["k_wkv7_replay"]) == 2, seen   # head sizes 64, 32, 16, 8 and 64, 32
