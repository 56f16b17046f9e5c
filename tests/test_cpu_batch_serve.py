"""Continuous batching (rwkv_mi_batch_serve), without a GPU: the scheduling rule restated in Python and pinned on hand-written cases, the
request-table builder of the binding, the exported symbol and its declaration, and the two kernels of csrc/sampling.hip from their code
objects -- k_serve_rows and k_serve_reset keep within their launch bounds' register budget without scratch, and the draw entry points and
k_stop_rows keep the registers they had.

serve_rule() and pass_bound() below are the rules of include/rwkv_mi355x.h; tests/test_gpu_batch_serve.py imports them as its scheduler."""
import ctypes
import os
import re

import numpy as np
import pytest

import kernel_meta
from test_cpu_batch_until import PARENT_REGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rwkv_mi_batch_serve",)
NO_SLOT = 0xFFFFFFFF
# k_serve_rows<DRAWS>: the scheduler of a drawing family and of the greedy one; k_serve_reset<VEC>: the 16-byte and the word form of the copy
SERVE_ROWS = {(0,), (1,)}
SERVE_RESET = {(0,), (1,)}
# (sgpr_count, vgpr_count) of k_stop_rows as the commit before rwkv_mi_batch_serve compiled it for gfx950: the scheduler does not share its body
STOP_ROWS_REGS = (33, 23)


def serve_rule(prompt_lens, emitted_lens, n):
    """(lane, start_pass, passes) of a queue served by n lanes: request q occupies its lane for prompt_lens[q] - 1 + emitted_lens[q] passes from
    start_pass[q] on. Lane r starts with request r at pass 0; a lane whose request retires after pass i takes the next request not yet taken
    at pass i + 1, lanes that retire in the same pass in ascending lane order. passes: the passes up to and including the last retirement."""
    R = len(prompt_lens)
    assert R >= n >= 1 and len(emitted_lens) == R
    lane, start = [None] * R, [None] * R
    free_at = [0] * n
    q = 0
    while q < R:
        p = min(free_at)
        for r in range(n):
            if free_at[r] == p and q < R:
                assert prompt_lens[q] >= 1 and emitted_lens[q] >= 1
                lane[q], start[q] = r, p
                free_at[r] = p + prompt_lens[q] - 1 + emitted_lens[q]
                q += 1
    return lane, start, max(free_at)


def pass_bound(prompt_lens, max_tokens):
    """the passes the host enqueues at most: a lane with work advances its request by one pass, so no schedule needs more"""
    return sum(L - 1 + b for L, b in zip(prompt_lens, max_tokens))


def _pkg():
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    pkg = graft.load_package()
    pkg.build_library()
    return pkg


# ---- the rule ----

def test_lanes_that_retire_together_take_requests_in_lane_order():
    # three lanes, the first two retire after pass 1: lane 0 takes request 3, lane 1 request 4, both from pass 2 on
    lane, start, passes = serve_rule([1, 1, 1, 1, 1], [2, 2, 5, 1, 1], 3)
    assert lane == [0, 1, 2, 0, 1] and start == [0, 0, 0, 2, 2] and passes == 5
    # the other way round in time: lane 2 retires first and takes the next request, whatever its number
    lane, start, passes = serve_rule([1, 1, 1, 1, 1], [4, 4, 2, 3, 1], 3)
    assert lane == [0, 1, 2, 2, 0] and start == [0, 0, 0, 2, 4] and passes == 5
    # a prompt occupies its lane: L - 1 passes without a token, then one pass per token
    lane, start, passes = serve_rule([3, 1, 2], [2, 1, 1], 2)
    assert lane == [0, 1, 1] and start == [0, 0, 1] and passes == 4


def test_a_request_of_one_prompt_token_and_one_token_is_retired_by_the_pass_that_admitted_it():
    # request 2 is fed at pass 1 and retires after it: lane 1 admits again at pass 2
    lane, start, passes = serve_rule([1, 1, 1, 1], [5, 1, 1, 2], 2)
    assert lane == [0, 1, 1, 1] and start == [0, 0, 1, 2] and passes == 5
    # one lane: the queue in order, back to back
    lane, start, passes = serve_rule([1, 1, 1], [1, 1, 1], 1)
    assert lane == [0, 0, 0] and start == [0, 1, 2] and passes == 3


def test_as_many_requests_as_lanes_is_decode_until():
    lane, start, passes = serve_rule([1, 1, 1], [4, 2, 7], 3)
    assert lane == [0, 1, 2] and start == [0, 0, 0] and passes == 7
    with pytest.raises(AssertionError):
        serve_rule([1, 1], [1, 1], 3)   # fewer requests than lanes


def test_the_pass_bound_covers_every_schedule():
    rng = np.random.default_rng(5)
    for _ in range(200):
        n = int(rng.integers(1, 6))
        R = n + int(rng.integers(0, 12))
        L = [int(v) for v in rng.integers(1, 7, R)]
        budget = [int(v) for v in rng.integers(1, 10, R)]
        emitted = [int(rng.integers(1, b + 1)) for b in budget]
        lane, start, passes = serve_rule(L, emitted, n)
        assert passes <= pass_bound(L, budget)
        assert sorted(q for q in range(R) if start[q] == 0) == list(range(n))
        # a lane serves one request at a time, and requests are taken in the order of the queue
        assert start == sorted(start)
        for r in range(n):
            mine = [q for q in range(R) if lane[q] == r]
            for a, b in zip(mine, mine[1:]):
                assert start[b] == start[a] + L[a] - 1 + emitted[a]
    assert pass_bound([1], [1]) == 1 and pass_bound([5, 1], [9, 1]) == 14
    # one lane meets the bound when every request runs to its budget
    assert serve_rule([3, 2], [4, 5], 1)[2] == pass_bound([3, 2], [4, 5])


# ---- the binding ----

def test_libraries_export_the_serve_symbol():
    pkg = _pkg()
    for path in (pkg.LIB_PATH, pkg.HOOKS_LIB_PATH, pkg.SAMPLE_HOOKS_LIB_PATH):
        so = ctypes.CDLL(path)
        for name in SYMBOLS:
            assert hasattr(so, name), (path, name)
    header = open(os.path.join(ROOT, "include", "rwkv_mi355x.h")).read()
    declared = re.findall(r"RWKV_API[^;(]*?\b(rwkv_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert set(SYMBOLS) <= set(declared)
    for macro, value in (("RWKV_MI_NO_SLOT", "UINT32_MAX"), ("RWKV_MI_SERVE_GREEDY", "0"), ("RWKV_MI_SERVE_SAMPLE", "1"), ("RWKV_MI_SERVE_PENALIZED", "2")):
        assert re.search(r"#define\s+" + macro + r"\s+" + value + r"\b", header), macro


def test_binding_declares_the_call_and_lays_the_request_out_as_the_header_does():
    pkg = _pkg()
    lib = pkg.load_rwkv_shared_library()
    f = lib.library.rwkv_mi_batch_serve
    assert f.restype is ctypes.c_bool and len(f.argtypes) == 17
    R = pkg.ServeRequest
    # struct rwkv_mi_serve_request { u32 prompt_len, from_slot; sample_params (24, 8-aligned); penalty_params (12); u32 top_k; f32 min_p, decay,
    # repetition; stop_params (8); u32 reserved }
    assert ctypes.sizeof(R) == 72
    assert [R.prompt_len.offset, R.from_slot.offset, R.sample.offset, R.penalty.offset, R.top_k.offset, R.min_p.offset, R.decay.offset, R.repetition.offset,
            R.stop.offset, R.reserved.offset] == [0, 4, 8, 32, 44, 48, 52, 56, 60, 68]
    assert pkg.NO_SLOT == NO_SLOT and (pkg.SERVE_GREEDY, pkg.SERVE_SAMPLE, pkg.SERVE_PENALIZED) == (0, 1, 2)
    assert callable(pkg.RWKVBatch.serve)


def test_request_builder_layout_defaults_and_errors():
    pkg = _pkg()
    arr, prompts, seq_lens, seq_tokens = pkg.serve_requests([
        dict(prompt=[5, 6, 7], max_tokens=9, stop=[[1], [2, 3]], from_slot=4, temperature=1.5, top_p=0.9, seed=11, presence=0.25, frequency=0.5, top_k=7,
             min_p=0.05, decay=0.996, repetition=1.1),
        dict(prompt=[8], max_tokens=1),
        dict(prompt=(9, 10), max_tokens=3, stop=[[4, 4, 4]]),
    ])
    assert len(arr) == 3
    assert prompts.dtype == np.uint32 and prompts.tolist() == [5, 6, 7, 8, 9, 10]
    assert seq_lens.dtype == np.uint32 and seq_lens.tolist() == [1, 2, 3] and seq_tokens.tolist() == [1, 2, 3, 4, 4, 4]
    a = arr[0]
    assert (a.prompt_len, a.from_slot, a.stop.max_tokens, a.stop.n_seqs, a.top_k, a.sample.seed, a.reserved) == (3, 4, 9, 2, 7, 11, 0)
    f32 = lambda v: float(np.float32(v))   # noqa: E731
    assert (a.sample.temperature, a.sample.top_p, a.sample.u) == (1.5, f32(0.9), -1.0)
    assert (a.penalty.presence, a.penalty.frequency, a.penalty.record) == (0.25, 0.5, 1)
    assert (a.min_p, a.decay, a.repetition) == (f32(0.05), f32(0.996), f32(1.1))
    d = arr[1]   # the defaults: the fresh state, no sequences, no truncation, no repetition setting
    assert (d.prompt_len, d.from_slot, d.stop.max_tokens, d.stop.n_seqs, d.top_k, d.min_p, d.decay, d.repetition) == (1, NO_SLOT, 1, 0, 0, 0.0, 1.0, 1.0)
    assert (d.sample.temperature, d.sample.top_p, d.sample.u, d.sample.seed) == (1.0, f32(0.8), -1.0, 0)
    assert (arr[2].prompt_len, arr[2].stop.n_seqs) == (2, 1)
    empty = pkg.serve_requests([])
    assert len(empty[0]) == 0 and empty[1].size == 0 and empty[2].size == 0 and empty[3].size == 0
    with pytest.raises(ValueError):
        pkg.serve_requests([dict(prompt=[], max_tokens=3)])
    with pytest.raises(KeyError):
        pkg.serve_requests([dict(prompt=[1])])
    with pytest.raises(ValueError):
        pkg.serve_requests([dict(prompt=[1], max_tokens=3, temprature=1.0)])   # (a misspelt key is not dropped silently)


# ---- the kernels ----

@pytest.mark.skipif(not kernel_meta.have_hipcc(), reason="needs hipcc")
def test_serve_kernels_keep_their_budget_and_the_old_entry_points_their_registers():
    assert set(kernel_meta.named("sampling.hip", "k_serve_rows")) == SERVE_ROWS
    assert set(kernel_meta.named("sampling.hip", "k_serve_reset")) == SERVE_RESET
    kernel_meta.budget("sampling.hip", tuple(("k_serve_rows", a) for a in sorted(SERVE_ROWS)))
    kernel_meta.budget("sampling.hip", tuple(("k_serve_reset", a) for a in sorted(SERVE_RESET)), wg=256)
    drawn = kernel_meta.budget("sampling.hip", tuple(PARENT_REGS))
    for key, k in drawn.items():
        assert (k.sgprs, k.vgprs) == PARENT_REGS[key], (key, k, PARENT_REGS[key])
    stop = kernel_meta.budget("sampling.hip", ("k_stop_rows",), wg=64)["k_stop_rows"]
    assert (stop.sgprs, stop.vgprs) == STOP_ROWS_REGS, stop
