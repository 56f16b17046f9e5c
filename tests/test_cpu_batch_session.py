"""Serve sessions (rwkv_mi_batch_serve_open .. _close), without a GPU: the protocol restated in Python pass by pass and pinned on hand-written
cases, the exported symbols and the binding's structs, the new scheduler kernel from its code object, and the two host-only pieces -- the
session's staged-table layout (csrc/call_layout.h, SessionLayout) and its bookkeeping (csrc/session_book.h) -- exercised by stand-alone
programs, the second under the address and undefined-behaviour sanitizers.

session_rule() below is the protocol of include/rwkv_mi355x.h; tests/test_gpu_batch_session.py imports it as its scheduler."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import kernel_meta
from test_cpu_batch_serve import SERVE_RESET, SERVE_ROWS, serve_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rwkv_mi_batch_serve_open", "rwkv_mi_batch_serve_submit", "rwkv_mi_batch_serve_cancel", "rwkv_mi_batch_serve_poll", "rwkv_mi_batch_serve_stats",
           "rwkv_mi_batch_serve_close")
SESSION_ROWS = {(0,), (1,)}   # k_session_rows<DRAWS>: the scheduler of the greedy family and of a drawing one


def session_rule(arrive_block, cancel_block, prompt_lens, natural_lens, n, K):
    """(lane, start_pass, emitted_len, reason_is_cancel) per request of a session of n lanes and blocks of K passes. Request q is submitted when
    arrive_block[q] blocks have been enqueued (so block arrive_block[q] is the first whose launches carry it; ids are in submit order, the
    numbers ascending), cancelled when cancel_block[q] have been (None: never), and emits natural_lens[q] tokens when left alone.
    Pass by pass: in front of the first pass P = b K of block b the idle lanes take, in lane order, the requests that have arrived, from pass P
    on. After every pass a lane with a request counts a token when the pass fed the last prompt token or a later one; the request retires
    when that is its natural end; otherwise, when its cancel has arrived with this block or an earlier one, it retires cancelled -- in its
    prompt phase with nothing emitted. Then the lanes without a request, the ones that have just retired theirs included, take what has
    arrived in lane order, from the next pass on."""
    R = len(prompt_lens)
    assert len(arrive_block) == len(cancel_block) == len(natural_lens) == R and list(arrive_block) == sorted(arrive_block)
    lane, start, emitted, cancelled = [None] * R, [None] * R, [0] * R, [False] * R
    ran = [0] * R
    on = [None] * n
    head, finished, P = 0, 0, 0
    while finished < R:
        b = P // K
        tail = sum(1 for a in arrive_block if a <= b)

        def admit(at):
            nonlocal head
            for r in range(n):
                if on[r] is None and head < tail:
                    on[r], lane[head], start[head] = head, r, at
                    head += 1

        if P % K == 0:
            admit(P)
        for r in range(n):
            q = on[r]
            if q is None:
                continue
            ran[q] += 1
            ended = False
            if ran[q] >= prompt_lens[q]:
                emitted[q] += 1
                ended = emitted[q] == natural_lens[q]
            if not ended and cancel_block[q] is not None and cancel_block[q] <= b:
                cancelled[q] = ended = True
            if ended:
                on[r] = None
                finished += 1
        admit(P + 1)
        P += 1
        assert P < 1 << 20, "the rule does not end"
    return lane, start, emitted, cancelled


def _pkg():
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    pkg = graft.load_package()
    pkg.build_library()
    return pkg


# ---- the rule ----

def test_everything_submitted_up_front_is_the_closed_call():
    rng = np.random.default_rng(5)
    for _ in range(200):
        n = int(rng.integers(1, 6))
        R = n + int(rng.integers(0, 12))
        L = [int(v) for v in rng.integers(1, 7, R)]
        emitted = [int(v) for v in rng.integers(1, 10, R)]
        K = int(rng.integers(1, 18))
        lane, start, lens, cancelled = session_rule([0] * R, [None] * R, L, emitted, n, K)
        want_lane, want_start, _ = serve_rule(L, emitted, n)
        assert (lane, start, lens) == (want_lane, want_start, emitted) and not any(cancelled), (n, K, L, emitted)


def test_an_arrival_with_all_lanes_idle_starts_at_its_block():
    for K in (1, 3, 16):
        # request 0 is over long before block 2; request 1 arrives there and starts at the block's first pass, on the lowest lane
        lane, start, lens, _ = session_rule([0, 2], [None, None], [1, 2], [1, 3], 3, K)
        assert lane == [0, 0] and start == [0, 2 * K] and lens == [1, 3], (K, lane, start)


def test_the_lowest_idle_lane_takes_an_arrival():
    # lane 0 is busy through block 1, lanes 1 and 2 are idle when request 3 arrives
    lane, start, _, _ = session_rule([0, 0, 0, 1], [None] * 4, [1, 1, 1, 1], [9, 1, 1, 2], 3, 4)
    assert lane == [0, 1, 2, 1] and start == [0, 0, 0, 4]
    # two arrivals, two idle lanes: in lane order
    lane, start, _, _ = session_rule([0, 0, 0, 1, 1], [None] * 5, [1, 1, 1, 1, 1], [9, 1, 1, 2, 2], 3, 4)
    assert lane == [0, 1, 2, 1, 2] and start == [0, 0, 0, 4, 4]
    # more arrivals than idle lanes: the rest waits for a retirement, and takes the lane at the pass after it
    lane, start, _, _ = session_rule([0, 1, 1], [None] * 3, [1, 1, 1], [9, 2, 1], 2, 4)
    assert lane == [0, 1, 1] and start == [0, 4, 6]
    # ... and when both lanes retire after the same pass, the lowest one takes it
    lane, start, _, _ = session_rule([0, 1, 1], [None] * 3, [1, 1, 1], [6, 2, 1], 2, 4)
    assert lane == [0, 1, 0] and start == [0, 4, 6]


def test_cancel_in_the_prompt_phase_gives_length_zero():
    # a prompt of 9 tokens from pass 0; the cancel arrives with block 1 (K = 4): the request retires after pass 4 with nothing emitted
    lane, start, lens, cancelled = session_rule([0], [1], [9], [5], 1, 4)
    assert (lane, start, lens, cancelled) == ([0], [0], [0], [True])
    # the freed lane serves the next request from the pass after that
    lane, start, lens, cancelled = session_rule([0, 0], [1, None], [9, 1], [5, 2], 1, 4)
    assert start == [0, 5] and lens == [0, 2] and cancelled == [True, False]


def test_cancel_in_decode_keeps_the_draws_up_to_the_first_pass_of_its_block():
    # one prompt token: pass p draws token p. The cancel arrives with block 2 (K = 3): passes 0 .. 6 have drawn, 7 tokens
    _, _, lens, cancelled = session_rule([0], [2], [1], [50], 1, 3)
    assert lens == [7] and cancelled == [True]
    # a natural end in that same pass wins
    _, _, lens, cancelled = session_rule([0], [2], [1], [7], 1, 3)
    assert lens == [7] and cancelled == [False]
    # ... and one a pass later does not
    _, _, lens, cancelled = session_rule([0], [2], [1], [8], 1, 3)
    assert lens == [7] and cancelled == [True]


def test_a_request_cancelled_while_queued_costs_one_lane_pass():
    # one lane; request 1 waits behind request 0 and is cancelled meanwhile: admitted at pass 6, retired after it, request 2 from pass 7 on
    lane, start, lens, cancelled = session_rule([0, 0, 0], [None, 1, None], [1, 3, 1], [6, 4, 2], 1, 2)
    assert start == [0, 6, 7] and lens == [6, 0, 2] and cancelled == [False, True, False]
    # with a one-token prompt its one pass draws a token, which is kept; with a budget of one that is its natural end
    _, _, lens, cancelled = session_rule([0, 0], [None, 1], [1, 1], [6, 4], 1, 2)
    assert lens == [6, 1] and cancelled == [False, True]
    _, _, lens, cancelled = session_rule([0, 0], [None, 1], [1, 1], [6, 1], 1, 2)
    assert lens == [6, 1] and cancelled == [False, False]


# ---- the binding ----

def test_libraries_export_the_session_symbols_and_the_header_declares_them():
    pkg = _pkg()
    for path in (pkg.LIB_PATH, pkg.HOOKS_LIB_PATH, pkg.SAMPLE_HOOKS_LIB_PATH):
        so = ctypes.CDLL(path)
        for name in SYMBOLS:
            assert hasattr(so, name), (path, name)
    header = open(os.path.join(ROOT, "include", "rwkv_mi355x.h")).read()
    declared = re.findall(r"RWKV_API[^;(]*?\b(rwkv_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert set(SYMBOLS) <= set(declared)
    for macro, value in (("RWKV_MI_STOP_CANCELLED", r"\(UINT32_MAX - 1u\)"), ("RWKV_MI_SERVE_CUT", "1u"), ("RWKV_MI_SERVE_REP", "2u"), ("RWKV_MI_SERVE_GUIDED", "4u"),
                         ("RWKV_MI_POLL_DRAIN", "1u")):
        assert re.search(r"#define\s+" + macro + r"\s+" + value, header), macro
    for text in ("the log-prob report inside a session", "chunked prompt ingestion", "priorities or reordering of the queue", "compacting idle lanes"):
        assert text in header, text   # (what is out of scope is said where the calls are declared)


def test_binding_lays_the_limits_and_the_event_out_as_the_header_does():
    pkg = _pkg()
    lib = pkg.load_rwkv_shared_library().library
    Lm, Ev = pkg.ServeLimits, pkg.ServeEvent
    # struct rwkv_mi_serve_limits { u32 capacity, max_prompt, stride, max_seqs, max_seq_tokens, features, reserved }
    assert ctypes.sizeof(Lm) == 28
    assert [getattr(Lm, f).offset for f in ("capacity", "max_prompt", "stride", "max_seqs", "max_seq_tokens", "features", "reserved")] == [0, 4, 8, 12, 16, 20, 24]
    # struct rwkv_mi_serve_event { u32 id, first, n_new, finished, stopped_by, lane, start_pass, guide_state, guide_misses }
    assert ctypes.sizeof(Ev) == 36
    assert [getattr(Ev, f).offset for f in ("id", "first", "n_new", "finished", "stopped_by", "lane", "start_pass", "guide_state", "guide_misses")] == list(range(0, 36, 4))
    header = open(os.path.join(ROOT, "include", "rwkv_mi355x.h")).read()
    for name, fields in (("rwkv_mi_serve_limits", Lm._fields_), ("rwkv_mi_serve_event", Ev._fields_)):
        body = re.search(r"struct " + name + r" \{(.*?)\n\};", header, flags=re.S).group(1)
        assert re.findall(r"uint32_t (\w+);", body) == [f for f, _ in fields], name
    assert (pkg.STOP_CANCELLED, pkg.SERVE_CUT, pkg.SERVE_REP, pkg.SERVE_GUIDED, pkg.POLL_DRAIN) == (0xFFFFFFFE, 1, 2, 4, 1)
    assert lib.rwkv_mi_batch_serve_open.restype is ctypes.c_void_p and len(lib.rwkv_mi_batch_serve_open.argtypes) == 5
    assert [len(getattr(lib, name).argtypes) for name in SYMBOLS[1:]] == [7, 2, 8, 5, 2]
    assert all(getattr(lib, name).restype is ctypes.c_bool for name in SYMBOLS[1:])
    assert callable(pkg.RWKVBatch.serve_open) and all(callable(getattr(pkg.ServeSession, f)) for f in ("submit", "cancel", "poll", "stats", "close", "__enter__", "__exit__"))


def test_a_misspelt_request_key_raises_before_anything_is_called():
    pkg = _pkg()
    s = object.__new__(pkg.ServeSession)   # (no batch behind it: the key is looked at first)
    s._ptr, s._L = 1, None
    with pytest.raises(ValueError, match="unknown keys"):
        s.submit(prompt=[1], max_tokens=3, temprature=1.0)
    with pytest.raises(KeyError):
        s.submit(prompt=[1])
    s._ptr = None
    with pytest.raises(ValueError, match="closed"):
        s.submit(prompt=[1], max_tokens=3)


# ---- the kernels ----

@pytest.mark.skipif(not kernel_meta.have_hipcc(), reason="needs hipcc")
def test_the_session_scheduler_keeps_its_budget_and_the_serve_kernels_their_instantiations():
    assert set(kernel_meta.named("sampling.hip", "k_session_rows")) == SESSION_ROWS
    kernel_meta.budget("sampling.hip", (("k_session_rows", (0,)), ("k_session_rows", (1,))))
    assert set(kernel_meta.named("sampling.hip", "k_serve_rows")) == SERVE_ROWS
    assert set(kernel_meta.named("sampling.hip", "k_serve_reset")) == SERVE_RESET


# ---- the host-only pieces ----

def _build_and_run(tmp_path, name, flags, says):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-O1", *flags, "-I", os.path.join(ROOT, "rwkv.cpp_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert says in r.stdout


def test_session_layout_invariants(tmp_path):
    _build_and_run(tmp_path, "session_layout_check", [], "session layout OK")


def test_session_bookkeeping_under_the_sanitizers(tmp_path):
    _build_and_run(tmp_path, "session_book_check", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "session book OK")
