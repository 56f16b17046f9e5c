"""Speculative decoding in the batch (rwkv_mi_batch_eval_draft; csrc/sampling.hip k_draft_accept_rows, csrc/kernels.hip k_wkvX_replay). The
guarantee is that speculation never changes what is emitted, only how many passes it takes, so everything here is bit for bit: the emitted
tokens, lens_out, the slot's state as the bytes of state_store, its occurrence table, and -- a draw counter cannot be read back -- the token
one further generator draw gives, against the PLAIN loop of the same family run for lens_out steps from the same start:
    greedy      decode_greedy
    sampled     the host loop of eval_sample with u = -1, the slot's counter continuing
    penalised   decode_sample_penalized (it continues, every step records)
Drafts are cut from the reference's own continuation and corrupted at a chosen position j: d(j+1) = (e_j + 1) % n_vocab, so exactly j draft
tokens stand."""
import ctypes
import os

import numpy as np
import pytest

from gpu_lib import ROOT, library, model, pkg, synth

pytestmark = pytest.mark.gpu

ARGS = 1 << 8   # RWKV_ERROR_ARGS
NO_TOKEN = 0xFFFFFFFF
GOLDEN = os.path.join(ROOT, "tests", "golden")
# one tiny fixture of every architecture in a float and a quantised format (RWKV-6 ships quantised only: its float format is the synthetic
# FP32 below), and the synthetic configurations with head size 64, so that the templated AND the generic replay kernels run
TINY = ["tiny-rwkv-4v0-660K-FP32", "tiny-rwkv-4v0-660K-Q5_1", "tiny-rwkv-5v1-730K-FP16", "tiny-rwkv-5v1-730K-Q5_0", "tiny-rwkv-5v2-730K-FP32",
        "tiny-rwkv-5v2-730K-Q5_1", "tiny-rwkv-6v0-3m-Q5_0", "tiny-rwkv-6v0-3m-Q5_1", "tiny-rwkv-7v0-834K-FP16", "tiny-rwkv-7v0-834K-Q5_1"]
SYNTH = [("test-v6", "Q5_1"), ("test-v6", "FP32"), ("test-v7", "Q5_1"), ("test-v5.1", "Q5_1"), ("test-v4", "Q8_0")]
MODELS = [("golden", n) for n in TINY if os.path.exists(os.path.join(GOLDEN, n + ".bin"))] + [("synth",) + s for s in SYNTH]
PROMPT = [34, 105, 110, 7, 92]
X0 = 61
P_U32 = ctypes.POINTER(ctypes.c_uint32)
P_F32 = ctypes.POINTER(ctypes.c_float)


def _path(tmp_path, spec):
    library()
    if spec[0] == "golden":
        return os.path.join(GOLDEN, spec[1] + ".bin")
    p = str(tmp_path / f"{spec[1]}-{spec[2]}.bin")
    synth.write_model(p, synth.CONFIGS[spec[1]], spec[2], seed=7)
    return p


def _id(spec):
    return "-".join(spec[1:])


class Bench:
    """A model, a batch of `slots` slots, and per slot a start state: the state after PROMPT (+ the slot index, so the slots differ)."""

    def __init__(self, path, slots=6):
        self.m = model(path)
        self.V = self.m.n_vocab
        self.B = pkg.RWKVBatch(self.m, slots)
        self.start = []
        for s in range(slots):
            self.B.state_load(s, None)
            self.B.eval_ragged([s], [[(t + s) % self.V for t in PROMPT]], want_logits=False)
            self.start.append(self.B.state_store(s))

    def reset(self, slot, counter=0, counts=()):
        self.B.state_load(slot, self.start[slot])
        self.B.rng_seek(slot, counter)
        if counts is not None:
            self.B.counts_reset(slot)
            self.B.counts_add(slot, list(counts))

    def bytes(self, slot):
        return self.B.state_store(slot).tobytes()

    def close(self):
        self.B.free()
        self.m.free()


def _corrupt(true, k, j, V):
    """the draft d1 .. dk from the true continuation e0 .., with d(j+1) wrong when j < k: exactly min(j, k) tokens stand"""
    d = [int(t) for t in true[:k]]
    if j < k:
        d[j] = (d[j] + 1) % V
    return d


# ---- greedy: every architecture, every draft length, every mismatch position ----

@pytest.mark.parametrize("spec", MODELS, ids=_id)
def test_greedy_draft_keeps_exactly_the_true_prefix(tmp_path, spec):
    b = Bench(_path(tmp_path, spec), slots=2)
    try:
        ref = {}
        for n in range(1, 10):
            b.reset(0, counts=None)
            toks, _ = b.B.decode_greedy([0], [X0], n)
            ref[n] = (toks[0].tolist(), b.bytes(0))
        true = ref[9][0]
        for n in range(1, 10):
            assert ref[n][0] == true[:n]
        other = b.bytes(1)
        for k in (1, 4, 8):
            for j in range(k + 1):
                b.reset(0, counts=None)
                emitted, lens = b.B.eval_draft([0], [[X0] + _corrupt(true, k, j, b.V)])
                assert int(lens[0]) == j + 1, (k, j, lens)
                assert emitted[0] == true[:j + 1], (k, j)
                assert b.bytes(0) == ref[j + 1][1], (k, j)
        assert b.bytes(1) == other
    finally:
        b.close()


# ---- a mixed call: rows of 1, 3 and 9 tokens with different mismatch positions, and a slot the call does not name ----

@pytest.mark.parametrize("spec", [("synth", "test-v6", "Q5_1"), ("synth", "test-v7", "Q5_1"), ("golden", "tiny-rwkv-5v2-730K-Q5_1")], ids=_id)
@pytest.mark.parametrize("big", [False, True], ids=["T13", "T49"])
def test_mixed_call_gives_every_row_what_it_gets_alone(tmp_path, spec, big):
    """T = 13 stays below the matrix-core threshold of a quantised file; four more rows of 9 tokens (T = 49 with them) cross it"""
    b = Bench(_path(tmp_path, spec), slots=8)
    try:
        # (slot, k, mismatch position); slot 7 is not named
        plan = [(0, 0, 0), (1, 2, 1), (2, 8, 5)] + ([(3, 8, 8), (4, 8, 0), (5, 8, 3), (6, 8, 7)] if big else [])
        ref, rows = {}, {}
        for slot, k, j in plan:
            b.reset(slot, counts=None)
            true = b.B.decode_greedy([slot], [X0 + slot], 9)[0][0].tolist()
            b.reset(slot, counts=None)
            toks = b.B.decode_greedy([slot], [X0 + slot], min(j, k) + 1)[0][0].tolist()
            ref[slot] = (toks, b.bytes(slot))
            rows[slot] = [X0 + slot] + _corrupt(true, k, j, b.V)
        alone = {}
        for slot, k, j in plan:
            b.reset(slot, counts=None)
            emitted, lens = b.B.eval_draft([slot], [rows[slot]])
            alone[slot] = (emitted[0], int(lens[0]), b.bytes(slot))
        for slot, _, _ in plan:
            b.reset(slot, counts=None)
        untouched = b.bytes(7)
        slots = [p[0] for p in plan]
        assert sum(len(rows[s]) for s in slots) == (49 if big else 13)
        emitted, lens = b.B.eval_draft(slots, [rows[s] for s in slots])
        for i, (slot, k, j) in enumerate(plan):
            got = (emitted[i], int(lens[i]), b.bytes(slot))
            assert got[1] == min(j, k) + 1, (slot, got[1])
            assert got[:2] == alone[slot][:2] and got[2] == alone[slot][2], slot
            assert got[0] == ref[slot][0] and got[2] == ref[slot][1], slot
        assert b.bytes(7) == untouched
    finally:
        b.close()


# ---- sampled: the host loop of eval_sample with u = -1, the counter continuing ----

def _sampled_reference(b, slot, x0, n, temperature, top_p, seed):
    toks, tok = [], x0
    for _ in range(n):
        tok = int(b.B.eval_sample([slot], [tok], temperature, top_p, -1.0, seed)[0])
        toks.append(tok)
    return toks


@pytest.mark.parametrize("spec", [("synth", "test-v6", "Q5_1"), ("synth", "test-v7", "Q5_1"), ("golden", "tiny-rwkv-4v0-660K-FP32")], ids=_id)
@pytest.mark.parametrize("temperature", [1.0, 0.0])
def test_sampled_draft_equals_the_host_loop(tmp_path, spec, temperature):
    b = Bench(_path(tmp_path, spec), slots=3)
    try:
        plan = [(0, 8, 3, 11, 5), (1, 4, 4, 12, 0), (2, 8, 0, 13, 40)]   # slot, k, mismatch position, seed, the slot's counter before the call
        ref, rows = {}, {}
        for slot, k, j, seed, ctr in plan:
            b.reset(slot, ctr, counts=None)
            true = _sampled_reference(b, slot, X0, 9, temperature, 0.9, seed)
            a = min(j, k)
            b.reset(slot, ctr, counts=None)
            toks = _sampled_reference(b, slot, X0, a + 1, temperature, 0.9, seed)
            assert toks == true[:a + 1]
            state = b.bytes(slot)
            nxt = int(b.B.eval_sample([slot], [toks[-1]], 1.0, 0.9, -1.0, seed)[0])   # the draw counter, shown by what it decides
            ref[slot] = (toks, state, nxt, b.bytes(slot))
            rows[slot] = [X0] + _corrupt(true, k, j, b.V)
        for slot, k, j, seed, ctr in plan:
            b.reset(slot, ctr, counts=None)
        slots = [p[0] for p in plan]
        params = pkg.sample_params(len(plan), temperature, 0.9, 0.5, [p[3] for p in plan])   # (u is not read: the generator draws)
        emitted, lens = b.B.eval_draft(slots, [rows[s] for s in slots], params=params)
        for i, (slot, k, j, seed, ctr) in enumerate(plan):
            assert int(lens[i]) == min(j, k) + 1 and emitted[i] == ref[slot][0], (slot, emitted[i], ref[slot][0])
            assert b.bytes(slot) == ref[slot][1], slot
            nxt = int(b.B.eval_sample([slot], [emitted[i][-1]], 1.0, 0.9, -1.0, seed)[0])
            assert nxt == ref[slot][2] and b.bytes(slot) == ref[slot][3], slot
    finally:
        b.close()


# ---- penalised: decode_sample_penalized, counts and all ----

@pytest.mark.parametrize("spec", [("synth", "test-v6", "Q5_1"), ("synth", "test-v7", "Q5_1"), ("golden", "tiny-rwkv-5v1-730K-Q5_0")], ids=_id)
def test_penalised_draft_equals_the_penalised_loop(tmp_path, spec):
    b = Bench(_path(tmp_path, spec), slots=3)
    try:
        plan = [(0, 8, 4, 21, 3), (1, 8, 8, 22, 0), (2, 3, 1, 23, 9)]   # slot, k, mismatch position, seed, counter
        before = {0: [X0, 5, 5, 9], 1: [], 2: [1, 2, 3]}
        ref, rows = {}, {}
        for slot, k, j, seed, ctr in plan:
            b.reset(slot, ctr, before[slot])
            true = b.B.decode_sample_penalized([slot], [X0], 9, 1.0, 0.9, seed, 0.2, 0.2)[0][0].tolist()
            if slot == 0:
                b.B.set_logit_bias(0, {int(true[0]): -999999999.0, 17: 1.5})   # the row with a bias: its first token is forbidden from now on
                b.reset(slot, ctr, before[slot])
                true = b.B.decode_sample_penalized([slot], [X0], 9, 1.0, 0.9, seed, 0.2, 0.2)[0][0].tolist()
            a = min(j, k)
            b.reset(slot, ctr, before[slot])
            toks = b.B.decode_sample_penalized([slot], [X0], a + 1, 1.0, 0.9, seed, 0.2, 0.2)[0][0].tolist()
            assert toks == true[:a + 1]
            ref[slot] = (toks, b.bytes(slot), b.B.counts(slot).copy())
            nxt = int(b.B.eval_sample([slot], [toks[-1]], 1.0, 0.9, -1.0, seed)[0])
            ref[slot] += (nxt,)
            rows[slot] = [X0] + _corrupt(true, k, j, b.V)
        for slot, k, j, seed, ctr in plan:
            b.reset(slot, ctr, before[slot])
        slots = [p[0] for p in plan]
        params = pkg.sample_params(len(plan), 1.0, 0.9, 0.25, [p[3] for p in plan])
        pens = pkg.penalty_params(len(plan), 0.2, 0.2, False)   # (record is not read: every emitted token is recorded)
        emitted, lens = b.B.eval_draft(slots, [rows[s] for s in slots], params=params, penalties=pens)
        for i, (slot, k, j, seed, ctr) in enumerate(plan):
            assert int(lens[i]) == min(j, k) + 1 and emitted[i] == ref[slot][0], (slot, emitted[i], ref[slot][0])
            assert b.bytes(slot) == ref[slot][1], slot
            assert np.array_equal(b.B.counts(slot), ref[slot][2]), slot
            assert int(b.B.counts(slot).sum()) == len(before[slot]) + int(lens[i])
            assert int(b.B.eval_sample([slot], [emitted[i][-1]], 1.0, 0.9, -1.0, seed)[0]) == ref[slot][3], slot
    finally:
        b.close()


# ---- continuation, and a drafter in the loop ----

@pytest.mark.parametrize("spec", [("synth", "test-v6", "Q5_1"), ("golden", "tiny-rwkv-7v0-834K-FP16")], ids=_id)
def test_two_draft_calls_equal_the_plain_loop_of_the_summed_length(tmp_path, spec):
    b = Bench(_path(tmp_path, spec), slots=2)
    try:
        # greedy in slot 0, sampled in slot 1
        b.reset(0, counts=None)
        g_true = b.B.decode_greedy([0], [X0], 12)[0][0].tolist()
        b.reset(1, 2, counts=None)
        s_true = _sampled_reference(b, 1, X0, 12, 1.0, 0.9, 77)
        for slot, true, params in ((0, g_true, None), (1, s_true, pkg.sample_params(1, 1.0, 0.9, -1.0, 77))):
            b.reset(slot, 2, counts=None)
            e1, l1 = b.B.eval_draft([slot], [[X0] + _corrupt(true, 6, 3, b.V)], params=params)          # 3 stand: 4 emitted
            e2, l2 = b.B.eval_draft([slot], [[e1[0][-1]] + [int(t) for t in true[4:9]]], params=params)   # all 5 stand: 6 emitted
            assert (int(l1[0]), int(l2[0])) == (4, 6) and e1[0] + e2[0] == true[:10], slot
            got = b.bytes(slot)
            b.reset(slot, 2, counts=None)
            if params is None:
                assert b.B.decode_greedy([slot], [X0], 10)[0][0].tolist() == true[:10]
            else:
                assert _sampled_reference(b, slot, X0, 10, 1.0, 0.9, 77) == true[:10]
            assert got == b.bytes(slot), slot
    finally:
        b.close()


def test_lookup_draft_in_a_greedy_loop_emits_the_plain_stream(tmp_path):
    """the drafter callers get: whatever lookup_draft proposes, the stream is the greedy loop's, in no more passes than tokens"""
    b = Bench(_path(tmp_path, ("synth", "test-v6", "Q5_1")), slots=1)
    try:
        b.reset(0, counts=None)
        true = b.B.decode_greedy([0], [X0], 48)[0][0].tolist()
        b.reset(0, counts=None)
        history, out, tok, passes = list(PROMPT) + [X0], [], X0, 0
        while len(out) < 40:
            emitted, _ = b.B.eval_draft([0], [[tok] + pkg.lookup_draft(history, pkg.DRAFT_MAX)])
            out += emitted[0]
            history += emitted[0]
            tok = emitted[0][-1]
            passes += 1
        assert out == true[:len(out)] and passes <= len(out)
    finally:
        b.close()


# ---- logits_out: the logits the last emitted token was chosen from ----

@pytest.mark.parametrize("spec", [("synth", "test-v6", "Q5_1"), ("synth", "test-v7", "Q5_1"), ("golden", "tiny-rwkv-4v0-660K-Q5_1")], ids=_id)
def test_logits_out_are_the_logits_of_that_step(tmp_path, spec):
    b = Bench(_path(tmp_path, spec), slots=3)
    try:
        plan = [(0, 8, 2), (1, 5, 5), (2, 0, 0)]
        rows, want = {}, {}
        for slot, k, j in plan:
            b.reset(slot, counts=None)
            true = b.B.decode_greedy([slot], [X0], 9)[0][0].tolist()
            b.reset(slot, counts=None)
            fed = [X0] + true[:min(j, k)]
            for t in fed:
                logits = b.B.eval([slot], [t])[0]
            want[slot] = logits.copy()
            rows[slot] = [X0] + _corrupt(true, k, j, b.V)
            b.reset(slot, counts=None)
        slots = [p[0] for p in plan]
        emitted, lens, logits = b.B.eval_draft(slots, [rows[s] for s in slots], want_logits=True)
        for i, (slot, k, j) in enumerate(plan):
            assert logits[i].tobytes() == want[slot].tobytes(), slot
            assert int(np.argmax(logits[i])) == emitted[i][-1]
    finally:
        b.close()


# ---- rejections: RWKV_ERROR_ARGS, and nothing has changed ----

def _raw(b, slots, rows, params=None, pens=None, stride=None, tokens_out=True, lens_out=True, lens=None):
    s = np.asarray(slots, dtype=np.uint32)
    ln = np.asarray([len(r) for r in rows] if lens is None else lens, dtype=np.uint32)
    toks = np.asarray([t for r in rows for t in r], dtype=np.uint32)
    stride = max([len(r) for r in rows] + [1]) if stride is None else stride
    out = np.full((max(len(rows), 1), max(stride, 16)), 0xABABABAB, dtype=np.uint32)
    kept = np.full(max(len(rows), 1), 0xABABABAB, dtype=np.uint32)
    ok = b.B._L.rwkv_mi_batch_eval_draft(b.B._ptr, s.ctypes.data_as(P_U32), ln.ctypes.data_as(P_U32), toks.ctypes.data_as(P_U32), len(slots), params, pens, stride,
                                        out.ctypes.data_as(P_U32) if tokens_out else None, kept.ctypes.data_as(P_U32) if lens_out else None, None)
    return ok, b.m._library.rwkv_get_last_error(b.m._ctx), out, kept


def test_rejections_change_nothing(tmp_path):
    b = Bench(_path(tmp_path, ("synth", "test-v6", "Q5_1")), slots=3)
    try:
        V = b.V
        for s in range(3):
            b.reset(s, 4, [X0, 3, 3])
        guide = b.B.create_guide([{t: 0 for t in range(0, V, 2)}])
        b.B.attach_guide(2, guide, 0)
        b.B.set_logprobs(2)
        b.B.eval_sample([0, 1], [X0, X0], 1.0, 0.9, -1.0, [1, 2])   # a report to keep
        shape = [ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_uint32(0)]
        assert b.B._L.rwkv_mi_batch_logprobs_shape(b.B._ptr, *[ctypes.byref(x) for x in shape])
        shape0 = [int(x.value) for x in shape]
        report0 = [a.tobytes() for a in b.B.logprobs()]
        states = [b.bytes(s) for s in range(3)]
        counts = [b.B.counts(s).copy() for s in range(3)]
        sp = lambda n, **kw: pkg.sample_params(n, kw.get("t", 1.0), kw.get("p", 0.9), kw.get("u", -1.0), 5)   # noqa: E731
        pp = lambda n, **kw: pkg.penalty_params(n, kw.get("pr", 0.2), kw.get("fr", 0.2), True)                # noqa: E731
        row = [X0, 1, 2]
        cases = {
            "what eval_ragged rejects: n == 0": dict(slots=[], rows=[]),
            "a slot out of range": dict(slots=[3], rows=[row]),
            "a slot named twice": dict(slots=[0, 0], rows=[row, row]),
            "a length of 0": dict(slots=[0, 1], rows=[row, []]),
            "a token out of range": dict(slots=[0], rows=[[X0, V]]),
            "a draft above DRAFT_MAX": dict(slots=[0], rows=[[X0] + [1] * 9]),
            "tokens_out NULL": dict(slots=[0], rows=[row], tokens_out=False),
            "lens_out NULL": dict(slots=[0], rows=[row], lens_out=False),
            "stride below the longest row": dict(slots=[0, 1], rows=[row, [X0]], stride=2),
            "penalties without params": dict(slots=[0], rows=[row], pens=pp(1)),
            "a negative temperature": dict(slots=[0], rows=[row], params=sp(1, t=-1.0)),
            "top_p above 1": dict(slots=[0], rows=[row], params=sp(1, p=1.5)),
            "a NaN temperature": dict(slots=[0], rows=[row], params=sp(1, t=float("nan"))),
            "a presence that is not finite": dict(slots=[0], rows=[row], params=sp(1), pens=pp(1, pr=float("inf"))),
            "a NaN frequency": dict(slots=[0], rows=[row], params=sp(1), pens=pp(1, fr=float("nan"))),
            "a guided slot, greedy": dict(slots=[0, 2], rows=[row, row]),
            "a guided slot, sampled": dict(slots=[2], rows=[row], params=sp(1)),
            "a guided slot, penalised": dict(slots=[1, 2], rows=[row, row], params=sp(2), pens=pp(2)),
        }
        for what, kw in cases.items():
            ok, err, out, kept = _raw(b, **kw)
            assert not ok and err & ARGS, what
            assert (out == 0xABABABAB).all() and (kept == 0xABABABAB).all(), what
            for s in range(3):
                assert b.bytes(s) == states[s], (what, s)
                assert np.array_equal(b.B.counts(s), counts[s]), (what, s)
            assert b.B.guide_state(2) == (guide, 0, 0), what
            assert b.B._L.rwkv_mi_batch_logprobs_shape(b.B._ptr, *[ctypes.byref(x) for x in shape]) and [int(x.value) for x in shape] == shape0, what
        assert [a.tobytes() for a in b.B.logprobs()] == report0
        # the next draw of every slot is the one a twin that never saw a rejected call makes
        b.B.detach_guide(2)
        got = b.B.eval_sample([0, 1, 2], [X0, X0, X0], 1.0, 0.9, -1.0, [1, 2, 3]).tolist()
        twin = Bench(_path(tmp_path, ("synth", "test-v6", "Q5_1")), slots=3)
        try:
            for s in range(3):
                twin.reset(s, 4, [X0, 3, 3])
            twin.B.eval_sample([0, 1], [X0, X0], 1.0, 0.9, -1.0, [1, 2])
            assert twin.B.eval_sample([0, 1, 2], [X0, X0, X0], 1.0, 0.9, -1.0, [1, 2, 3]).tolist() == got
        finally:
            twin.close()
        # a valid call leaves the report of the call before it alone, too
        b.B.set_logprobs(2)
        b.B.eval_sample([0], [X0], 1.0, 0.9, -1.0, 1)
        kept_report = [a.tobytes() for a in b.B.logprobs()]
        b.B.eval_draft([0, 1], [[X0, 1, 2], [X0]])
        assert [a.tobytes() for a in b.B.logprobs()] == kept_report
    finally:
        b.close()
