"""Continuous batching in the batch device loop (rwkv_mi_batch_serve; csrc/sampling.hip k_serve_rows / k_serve_reset behind the draw kernels
and k_argmax_live). The oracle is the call's own guarantee: every request alone on a one-slot twin batch through the existing calls --
state_load (fresh, or the prefix slot's state), rng_seek 0, counts_reset, the request's truncation and repetition settings, eval of all but
the last prompt token, decode_until from the last one. Tokens, lengths, reasons, lanes' end states, counts, parities and draw counters must be
equal; lane and start pass must be what test_cpu_batch_serve.serve_rule gives for the observed lengths. Every comparison is exact.

A slot's draw counter cannot be read back; it is pinned through what it decides: one more generator draw (u < 0) must give the twin's token."""
import ctypes
import os

import numpy as np
import pytest

from gpu_lib import library, model, pkg, synth
from test_cpu_batch_serve import pass_bound, serve_rule
from test_cpu_batch_until import NO_TOKEN, stop_rule

pytestmark = pytest.mark.gpu

ARGS = 1 << 8   # RWKV_ERROR_ARGS
MODELS = [("test-v4", "Q8_0"), ("test-v6", "Q5_1"), ("test-v7", "Q5_1")]
FAMILIES = ("greedy", "sample", "pen")
FAMILY_ID = {"greedy": 0, "sample": 1, "pen": 2}
N_SLOTS = 6
LANES = [4, 0, 2]    # (scrambled; slots 1 and 3 are not named)
PREFIX_SLOT = 5      # a 6-token prefix that two requests share
R = 8
PROMPT_LENS = [1, 1, 2, 5, 3, 1, 4, 2]
BUDGETS = [2, 2, 7, 9, 3, 1, 5, 8]       # requests 0 and 1 retire after the same pass; request 5 is one prompt token and one token
FROM_PREFIX = (3, 6)
STOPPED = 3                              # the request that gets a two-token stop sequence from its own stream
K = 16
P_U32 = ctypes.POINTER(ctypes.c_uint32)


def _tok(i, j, V):
    return (37 * i + 11 * j + 5) % V


def _synth(tmp_path, name, fmt, seed=17):
    library()
    p = str(tmp_path / f"{name}-{fmt}.bin")
    synth.write_model(p, synth.CONFIGS[name], fmt, seed=seed)
    return p


def _requests(V):
    """The queue without its stop sequences: distinct seeds, temperatures at or above 1, and one request each with top-k, min-p, a decay and a
    repetition penalty (the last two are read by the penalised family only)."""
    reqs = []
    for q in range(R):
        reqs.append(dict(prompt=[_tok(q, j, V) for j in range(PROMPT_LENS[q])], max_tokens=BUDGETS[q], from_slot=PREFIX_SLOT if q in FROM_PREFIX else None,
                         temperature=1.0 + 0.15 * q, top_p=[0.9, 1.0, 0.95, 1.0, 0.85, 1.0, 0.9, 1.0][q], seed=21 + q,
                         presence=[0.2, 0.25, 0.0, 1.5, 0.2, 0.7, 0.3, 0.4][q], frequency=[0.2, 0.5, 0.3, 0.0, 0.2, 0.1, 0.3, 0.2][q]))
    reqs[2]["top_k"] = 5
    reqs[4]["min_p"] = 0.05
    reqs[6]["decay"] = 0.996
    reqs[7]["repetition"] = 1.1
    reqs[3]["top_k"], reqs[3]["repetition"] = 40, 1.1
    return reqs


def _prepare(b, V):
    """What the batch starts from: a token in every slot, a second one in three of them (the lanes have mixed parities), the prefix slot on
    the odd buffer with six tokens from the fresh state, and a draw counter and a history on every slot that an admission has to clear."""
    every = list(range(N_SLOTS))
    b.eval(every, [_tok(1, s, V) for s in every], want_logits=False)
    b.eval([0, 3], [_tok(2, s, V) for s in (0, 3)], want_logits=False)
    b.state_load(PREFIX_SLOT, None)
    for j in range(6):
        b.eval([PREFIX_SLOT], [_tok(9, j, V)], want_logits=False)
    for s in every:
        b.rng_seek(s, 3 * s + 1)


def _dirty_counts(b, V):
    for s in range(N_SLOTS):
        b.counts_add(s, [(5 * s + 3 * i) % min(V, 50) for i in range(12)])


def _fresh(m, family):
    b = pkg.RWKVBatch(m, N_SLOTS)
    _prepare(b, m.n_vocab)
    if family == "pen":
        _dirty_counts(b, m.n_vocab)
    return b


def _twin(m, family, rq, prefix_state):
    """The request alone, through the existing calls, on a batch of one slot: (twin batch, tokens, stopped_by)."""
    tw = pkg.RWKVBatch(m, 1)
    tw.state_load(0, prefix_state if rq.get("from_slot") is not None else None)
    tw.rng_seek(0, 0)
    if family == "pen":
        tw.counts_reset(0)
    tw.set_truncation(0, rq.get("top_k", 0), rq.get("min_p", 0.0))
    tw.set_repetition(0, rq.get("decay", 1.0), rq.get("repetition", 1.0))
    for t in rq["prompt"][:-1]:
        tw.eval([0], [t], want_logits=False)
    kw = {}
    if family != "greedy":
        kw.update(temperature=rq["temperature"], top_p=rq["top_p"], seed=rq["seed"])
    if family == "pen":
        kw.update(presence=rq["presence"], frequency=rq["frequency"])
    toks, why, _ = tw.decode_until([0], [rq["prompt"][-1]], rq["max_tokens"], stop=rq.get("stop") or None, **kw)
    return tw, toks[0], int(why[0])


def _queue_with_stop(m, family, prefix_state):
    """The queue, request STOPPED with a two-token sequence cut from what its twin emits without one (so it certainly occurs)."""
    reqs = _requests(m.n_vocab)
    tw, full, _ = _twin(m, family, reqs[STOPPED], prefix_state)
    tw.free()
    full = [int(t) for t in full]
    assert len(full) == BUDGETS[STOPPED]
    seq = full[3:5]
    reqs[STOPPED]["stop"] = [[m.n_vocab - 1, m.n_vocab - 2, m.n_vocab - 3], seq]
    want = stop_rule(full, BUDGETS[STOPPED], reqs[STOPPED]["stop"])
    assert want[1] == 1 and want[0] <= 5, (full, want)
    return reqs


def _raw_counts(b, slot, decaying):
    """the words of a slot's occurrence row as they lie in memory (a decaying row holds floats)"""
    return b.counts_f32(slot).view(np.uint32) if decaying else b.counts(slot)


def _check_serve(m, family, name, lanes=LANES):
    V = m.n_vocab
    n = len(lanes)
    b = _fresh(m, family)
    prefix_state = b.state_store(PREFIX_SLOT)
    bystanders = {s: b.state_store(s) for s in range(N_SLOTS) if s not in lanes}
    reqs = _queue_with_stop(m, family, prefix_state)
    twins = [_twin(m, family, rq, prefix_state) for rq in reqs]
    got = b.serve(lanes, reqs, FAMILY_ID[family])
    lens = [len(t) for t in got["tokens"]]
    for q in range(R):
        tw, toks, why = twins[q]
        assert np.array_equal(got["tokens"][q], toks), (name, family, q, got["tokens"][q], toks)
        assert int(got["stopped_by"][q]) == why, (name, family, q, got["stopped_by"][q], why)
    assert lens[5] == 1 and int(got["stopped_by"][STOPPED]) == 1 and lens[STOPPED] < BUDGETS[STOPPED], (lens, got["stopped_by"])
    lane_want, start_want, passes_want = serve_rule(PROMPT_LENS, lens, n)
    assert got["lane"].tolist() == lane_want and got["start_pass"].tolist() == start_want, (name, family, got["lane"], lane_want, got["start_pass"], start_want)
    ends = [start_want[q] + PROMPT_LENS[q] - 1 + lens[q] for q in range(R)]
    assert len(set(ends)) < R, ("two requests must retire after the same pass", ends)
    assert passes_want <= b.last_loop_passes() <= min(passes_want + 2 * K, pass_bound(PROMPT_LENS, BUDGETS)), (b.last_loop_passes(), passes_want)
    last_want = [max(q for q in range(R) if lane_want[q] == r) for r in range(n)]
    assert got["last_request"].tolist() == last_want, (got["last_request"], last_want)
    # the slots the call did not name as lanes: the prefix slot and the bystanders
    for s, before in bystanders.items():
        assert np.array_equal(b.state_store(s), before), (name, family, s, "a slot that is no lane")
    # what each lane is left with: its last request's twin
    for r, slot in enumerate(lanes):
        q = last_want[r]
        tw, toks, _ = twins[q]
        assert np.array_equal(b.state_store(slot), tw.state_store(0)), (name, family, r, q, "state")
        if family == "pen":
            decaying = reqs[q].get("decay", 1.0) != 1.0
            assert np.array_equal(b.counts(slot), _raw_counts(tw, 0, decaying)), (name, family, r, q, "occurrence row")
        # parity: one more eval of the last token reads the buffer the batch's parity names
        assert np.array_equal(b.eval([slot], [int(toks[-1])]), tw.eval([0], [int(toks[-1])])), (name, family, r, q, "parity")
        # the draw counter: one more generator draw (the lane slot has no truncation setting: the twin's is cleared for it)
        tw.set_truncation(0, 0, 0.0)
        a = ([int(toks[-1])], 1.0, 1.0, -1.0, 77 + r)
        assert np.array_equal(b.eval_sample([slot], *a), tw.eval_sample([0], *a)), (name, family, r, q, "draw counter")
    for tw, _, _ in twins:
        tw.free()
    b.free()
    return got, lens


# ---- 1. the guarantee, three architectures, three families ----

@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name,fmt", MODELS)
def test_every_request_is_the_request_alone_and_every_lane_its_last_request(tmp_path, name, fmt, family):
    m = model(_synth(tmp_path, name, fmt))
    _check_serve(m, family, name)
    m.free()


# ---- 2. a real vocabulary width through the occurrence reset; a vocabulary that is no multiple of four through the word form of the reset ----

@pytest.mark.parametrize("name,fmt", [("mega-v6-2048-v64k", "Q4_0"), ("slice-v4-768", "Q8_0")])
def test_penalised_queue_on_real_vocabulary_widths(tmp_path, name, fmt):
    m = model(_synth(tmp_path, name, fmt))
    _check_serve(m, "pen", name)
    m.free()


# ---- 3. the block of the loop cannot be seen in the results ----

def test_loop_block_of_one_and_sixteen_give_the_same(tmp_path):
    m = model(_synth(tmp_path, "test-v6", "Q5_1"))
    family = "sample"
    results = {}
    saved = os.environ.get("RWKV_MI_LOOP_BLOCK")
    try:
        for block in (1, 16):
            os.environ["RWKV_MI_LOOP_BLOCK"] = str(block)   # (read at the call)
            b = _fresh(m, family)
            reqs = _queue_with_stop(m, family, b.state_store(PREFIX_SLOT))
            got = b.serve(LANES, reqs, FAMILY_ID[family])
            lens = [len(t) for t in got["tokens"]]
            need = serve_rule(PROMPT_LENS, lens, len(LANES))[2]
            assert need <= b.last_loop_passes() <= need + 2 * block, (block, b.last_loop_passes(), need)
            results[block] = (got, [b.state_store(s) for s in range(N_SLOTS)])
            b.free()
    finally:
        if saved is None:
            os.environ.pop("RWKV_MI_LOOP_BLOCK", None)
        else:
            os.environ["RWKV_MI_LOOP_BLOCK"] = saved
    (g1, s1), (g16, s16) = results[1], results[16]
    assert all(np.array_equal(a, c) for a, c in zip(g1["tokens"], g16["tokens"]))
    for key in ("stopped_by", "lane", "start_pass", "last_request"):
        assert np.array_equal(g1[key], g16[key]), key
    assert all(np.array_equal(a, c) for a, c in zip(s1, s16))
    m.free()


# ---- 4. as many requests as lanes, one prompt token each: decode_until after the same resets ----

@pytest.mark.parametrize("family", FAMILIES)
def test_one_request_per_lane_is_decode_until(tmp_path, family):
    m = model(_synth(tmp_path, "test-v6", "Q5_1"))
    V = m.n_vocab
    n = len(LANES)
    budgets = [6, 3, 9]
    reqs = [dict(prompt=[_tok(0, r, V)], max_tokens=budgets[r], temperature=1.0 + 0.25 * r, top_p=[0.9, 1.0, 0.95][r], seed=40 + r,
                 presence=[0.2, 0.0, 1.5][r], frequency=[0.2, 0.3, 0.0][r]) for r in range(n)]
    b, tw = _fresh(m, family), _fresh(m, family)
    got = b.serve(LANES, reqs, FAMILY_ID[family])
    for s in LANES:
        tw.state_load(s, None)
        tw.rng_seek(s, 0)
        if family == "pen":
            tw.counts_reset(s)
    kw = {}
    if family != "greedy":
        kw.update(temperature=[rq["temperature"] for rq in reqs], top_p=[rq["top_p"] for rq in reqs], seed=[rq["seed"] for rq in reqs])
    if family == "pen":
        kw.update(presence=[rq["presence"] for rq in reqs], frequency=[rq["frequency"] for rq in reqs])
    toks, why, _ = tw.decode_until(LANES, [rq["prompt"][0] for rq in reqs], budgets, **kw)
    for r in range(n):
        assert np.array_equal(got["tokens"][r], toks[r]) and int(got["stopped_by"][r]) == int(why[r]) == NO_TOKEN, (family, r)
    assert got["lane"].tolist() == [0, 1, 2] and got["start_pass"].tolist() == [0, 0, 0] and got["last_request"].tolist() == [0, 1, 2]
    for s in range(N_SLOTS):
        assert np.array_equal(b.state_store(s), tw.state_store(s)), (family, s)
        if family == "pen":
            assert np.array_equal(b.counts(s), tw.counts(s)), (family, s)
    last = [int(t[-1]) for t in toks]
    assert np.array_equal(b.eval(LANES, last), tw.eval(LANES, last)), (family, "parity")
    b.free()
    tw.free()
    m.free()


# ---- 5. rejections ----

def _raw(b, lanes, family, arr, prompts, seq_lens, seq_tokens, stride, override=None):
    """rwkv_mi_batch_serve through the C ABI with every output given; override: arguments to replace (a number, or a pointer by None)."""
    s = np.asarray(lanes, dtype=np.uint32)
    Rn = max(len(arr), 1)
    outs = dict(tokens_out=np.zeros((Rn, max(stride, 1)), dtype=np.uint32), lens_out=np.zeros(Rn, dtype=np.uint32), why_out=np.zeros(Rn, dtype=np.uint32),
                lane_out=np.zeros(Rn, dtype=np.uint32), start_out=np.zeros(Rn, dtype=np.uint32), last_out=np.zeros(max(s.size, 1), dtype=np.uint32))
    a = dict(lanes=s.ctypes.data_as(P_U32), n=s.size, family=family, requests=arr, n_requests=len(arr), prompts=prompts.ctypes.data_as(P_U32),
             seq_lens=seq_lens.ctypes.data_as(P_U32), seq_tokens=seq_tokens.ctypes.data_as(P_U32), stride=stride)
    a.update({k: v.ctypes.data_as(P_U32) for k, v in outs.items()})
    a.update(override or {})
    ok = b._L.rwkv_mi_batch_serve(b._ptr, a["lanes"], a["n"], a["family"], a["requests"], a["n_requests"], a["prompts"], a["seq_lens"], a["seq_tokens"],
                                  a["stride"], a["tokens_out"], a["lens_out"], a["why_out"], a["lane_out"], a["start_out"], a["last_out"], None)
    return bool(ok), outs


def test_rejections_change_nothing(tmp_path):
    m = model(_synth(tmp_path, "test-v6", "Q5_1"))
    V = m.n_vocab
    b, tw = _fresh(m, "pen"), _fresh(m, "pen")
    u32 = lambda v: np.asarray(v, dtype=np.uint32)   # noqa: E731

    def queue(**change):
        reqs = _requests(V)
        reqs[STOPPED]["stop"] = [[1], [2, 3]]
        for q, kv in change.items():
            reqs[int(q[1:])].update(kv)
        return reqs

    def rejected(what, lanes=LANES, family=2, reqs=None, stride=9, mutate=None, null=()):
        arr, prompts, seq_lens, seq_tokens = pkg.serve_requests(queue() if reqs is None else reqs)
        if mutate:
            arr, prompts, seq_lens, seq_tokens = mutate(arr, prompts, seq_lens, seq_tokens)
        ok, _ = _raw(b, lanes, family, arr, prompts, seq_lens, seq_tokens, stride, {name: None for name in null})
        err = m._library.rwkv_get_last_error(m._ctx)
        assert not ok and err & ARGS, (what, ok, err)

    def zero_len(arr, p, sl, st):
        arr[2].prompt_len = 0
        return arr, p, sl, st

    def many_seqs(arr, p, sl, st):
        arr[STOPPED].stop.n_seqs = 17
        return arr, p, u32([1] * 17), u32([1] * 17)

    rejected("fewer requests than lanes", reqs=queue()[:2])
    rejected("n == 0", lanes=[])
    rejected("n > n_slots", lanes=[0, 1, 2, 3, 4, 5, 0])
    rejected("a lane out of range", lanes=[4, 0, N_SLOTS])
    rejected("a lane twice", lanes=[4, 0, 4])
    rejected("an unknown family", family=3)
    rejected("an empty prompt", mutate=zero_len)
    rejected("a prompt token out of range", reqs=queue(q4=dict(prompt=[1, V, 2])))
    rejected("a from_slot that is a lane", reqs=queue(q6=dict(from_slot=LANES[1])))
    rejected("a from_slot out of range", reqs=queue(q6=dict(from_slot=N_SLOTS)))
    rejected("lanes NULL", null=("lanes",))
    rejected("requests NULL", null=("requests",))
    rejected("prompt_tokens NULL", null=("prompts",))
    rejected("lens_out NULL", null=("lens_out",))
    # what decode_until rejects for the same fields
    rejected("a negative temperature", reqs=queue(q1=dict(temperature=-1.0)))
    rejected("a top_p above 1", reqs=queue(q1=dict(top_p=1.5)))
    rejected("a penalty that is not finite", reqs=queue(q1=dict(presence=float("inf"))))
    rejected("a max_tokens of 0", reqs=queue(q1=dict(max_tokens=0)))
    rejected("stride below the largest max_tokens", stride=8)
    rejected("n_seqs above the limit", mutate=many_seqs)
    rejected("seq_lens NULL", null=("seq_lens",))
    rejected("seq_tokens NULL", null=("seq_tokens",))
    rejected("a sequence of length 0", reqs=queue(q3=dict(stop=[[1], []])))
    rejected("a sequence longer than the limit", reqs=queue(q3=dict(stop=[[1] * 9])))
    rejected("a sequence token out of range", reqs=queue(q3=dict(stop=[[1, V]])))
    # what the two settings reject
    rejected("min_p above 1", reqs=queue(q1=dict(min_p=1.5)))
    rejected("min_p NaN", reqs=queue(q1=dict(min_p=float("nan"))))
    rejected("decay above 1", reqs=queue(q1=dict(decay=1.5)))
    rejected("decay below 0", reqs=queue(q1=dict(decay=-0.1)))
    rejected("repetition 0", reqs=queue(q1=dict(repetition=0.0)))
    rejected("repetition infinite", reqs=queue(q1=dict(repetition=float("inf"))))
    # a lane with a bias, a lane with a guide, a batch that reports
    b.set_logit_bias(LANES[0], {3: 2.0})
    rejected("a lane with a bias set")
    b.set_logit_bias(LANES[0], {})
    g = b.create_guide([{t: 0 for t in range(8)}])
    b.attach_guide(LANES[2], g, 0)
    rejected("a lane with a guide attached")
    b.detach_guide(LANES[2])
    b.free_guide(g)
    b.set_logprobs(2)
    rejected("a batch with the report on")
    b.set_logprobs(0, enabled=False)
    # nothing moved: state, counts and the next generator draw of every slot
    every = list(range(N_SLOTS))
    for s in every:
        assert np.array_equal(b.state_store(s), tw.state_store(s)), s
        assert np.array_equal(b.counts(s), tw.counts(s)), s
    a = (every, [_tok(3, s, V) for s in every], 1.0, 1.0, -1.0, list(range(50, 50 + N_SLOTS)), 0.2, 0.2, False)
    assert np.array_equal(b.eval_sample_penalized(*a), tw.eval_sample_penalized(*a))
    # ... and the same call with nothing wrong goes through
    arr, prompts, seq_lens, seq_tokens = pkg.serve_requests(queue())
    ok, outs = _raw(b, LANES, 2, arr, prompts, seq_lens, seq_tokens, 9)
    assert ok and (outs["lens_out"] >= 1).all() and (outs["lens_out"] <= np.asarray(BUDGETS)).all()
    for q in range(R):
        assert (outs["tokens_out"][q, outs["lens_out"][q]:] == NO_TOKEN).all(), (q, "no token past the request's length")
    b.free()
    tw.free()
    m.free()
