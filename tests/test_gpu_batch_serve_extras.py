"""Served requests with a guide, a logit bias and the log-prob report (rwkv_mi_batch_serve_ex; the guide words in csrc/sampling.hip
k_serve_rows, csrc/score.hip k_logprob_rows_serve). The oracle is the call's own guarantee: every request alone on a one-slot twin batch
through the existing calls -- state_load, rng_seek 0, counts_reset, the two settings, guide_attach, logit_bias_set, set_logprobs, eval of all
but the last prompt token, decode_until from the last one. Tokens, lengths, reasons, guide state, miss count and report rows must be equal,
lane and start pass what test_cpu_batch_serve.serve_rule gives for the observed lengths. Every comparison is exact (floats by their bits)."""
import ctypes
import os

import numpy as np
import pytest

from gpu_lib import library, model, pkg, synth
from test_cpu_batch_serve import serve_rule
from test_cpu_batch_until import NO_TOKEN

pytestmark = pytest.mark.gpu

ARGS = 1 << 8   # RWKV_ERROR_ARGS
NO_GUIDE = NO_SLOT = 0xFFFFFFFF
FAMILY_ID = {"greedy": 0, "sample": 1, "pen": 2}
N_SLOTS = 8
LANES = [4, 0, 2]        # (scrambled)
PREFIX_SLOT = 5          # a 6-token prefix that one request starts from
BIAS_SLOTS = (1, 3)      # bystanders whose bias tables the requests read
P_U32 = ctypes.POINTER(ctypes.c_uint32)
# the mixed queue: prompts of 1 .. 4 tokens, budgets of 2 .. 9, no stop sequence (every request runs to its budget, so the schedule is known)
PROMPT_LENS = [1, 1, 2, 2, 1, 3, 1, 4, 2]
BUDGETS = [2, 3, 4, 3, 5, 2, 9, 6, 7]
R = len(BUDGETS)
#          guide, guide_state, bias_slot (None: the key is absent)
EXTRAS = [(0, 0, None), (None, None, None), (1, 1, 1), (None, None, None), (0, 2, None), (None, None, None), (None, None, 3), (1, 0, 1), (None, None, None)]


def _tok(i, j, V):
    return (37 * i + 11 * j + 5) % V


def _synth(tmp_path, name, fmt, seed=17):
    library()
    p = str(tmp_path / f"{name}-{fmt}.bin")
    synth.write_model(p, synth.CONFIGS[name], fmt, seed=seed)
    return p


def _guides(V):
    """guide 0: three states, state s allows the tokens j = s (mod 3) and moves by j // 3; guide 1: the even tokens, then the tokens below 64"""
    return [[{j: (s + j // 3) % 3 for j in range(s, V, 3)} for s in range(3)],
            [{j: 1 for j in range(0, V, 2)}, {j: 0 for j in range(64)}]]


def _biases(V):
    return {1: {7: 5.0, 8: float("-inf"), 100: 3.0, 101: -2.5, V - 1: 1.25}, 3: {(3 * i + 1) % V: 2.0 + 0.5 * i for i in range(10)}}


def _queue(V, family, extras=EXTRAS, prompt_lens=PROMPT_LENS, budgets=BUDGETS):
    reqs = []
    for q, (g, gs, bs) in enumerate(extras):
        rq = dict(prompt=[_tok(q, j, V) for j in range(prompt_lens[q])], max_tokens=budgets[q], from_slot=PREFIX_SLOT if q == 8 else None,
                  temperature=1.0 + 0.15 * q, top_p=[0.9, 1.0, 0.95, 1.0, 0.85, 1.0, 0.9, 1.0, 0.95][q % 9], seed=21 + q,
                  presence=[0.2, 0.25, 0.0, 1.5, 0.2, 0.7, 0.3, 0.4, 0.1][q % 9], frequency=[0.2, 0.5, 0.3, 0.0, 0.2, 0.1, 0.3, 0.2, 0.4][q % 9])
        if g is not None and family != "greedy":
            rq.update(guide=g, guide_state=gs)
        if bs is not None and family == "pen":   # (only the penalised family reads a bias)
            rq.update(bias_slot=bs)
        reqs.append(rq)
    reqs[3]["top_k"] = 5
    if len(reqs) > 4:
        reqs[4]["repetition"] = 1.1   # (read by the penalised family only)
    return reqs


def _fresh(m, family, guides=None, biases=None):
    """A batch whose slots all have a past an admission has to clear: states on mixed parities, draw counters, counts; the prefix slot with six
    tokens from the fresh state; the guides; the bias tables of the two bias slots (penalised family)."""
    V = m.n_vocab
    b = pkg.RWKVBatch(m, N_SLOTS)
    every = list(range(N_SLOTS))
    b.eval(every, [_tok(1, s, V) for s in every], want_logits=False)
    b.eval([0, 3], [_tok(2, s, V) for s in (0, 3)], want_logits=False)
    b.state_load(PREFIX_SLOT, None)
    for j in range(6):
        b.eval([PREFIX_SLOT], [_tok(9, j, V)], want_logits=False)
    for s in every:
        b.rng_seek(s, 3 * s + 1)
    if family == "pen":
        for s in every:
            b.counts_add(s, [(5 * s + 3 * i) % min(V, 50) for i in range(12)])
        for s, table in (_biases(V) if biases is None else biases).items():
            b.set_logit_bias(s, table)
    ids = [b.create_guide(g) for g in (_guides(V) if guides is None else guides)]
    assert ids == list(range(len(ids)))
    return b


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _twin(m, family, rq, prefix_state, guides, biases, top_n):
    """The request alone, through the existing calls, on a batch of one slot. top_n None: the report is off."""
    tw = pkg.RWKVBatch(m, 1)
    tw.state_load(0, prefix_state if rq.get("from_slot") is not None else None)
    tw.rng_seek(0, 0)
    if family == "pen":
        tw.counts_reset(0)
    tw.set_truncation(0, rq.get("top_k", 0), rq.get("min_p", 0.0))
    tw.set_repetition(0, rq.get("decay", 1.0), rq.get("repetition", 1.0))
    if rq.get("guide") is not None:
        ids = [tw.create_guide(g) for g in guides]
        tw.attach_guide(0, ids[rq["guide"]], rq.get("guide_state", 0))
    if rq.get("bias_slot") is not None:
        tw.set_logit_bias(0, biases[rq["bias_slot"]])
    if top_n is not None:
        tw.set_logprobs(top_n)
    for t in rq["prompt"][:-1]:
        tw.eval([0], [t], want_logits=False)
    kw = {}
    if family != "greedy":
        kw.update(temperature=rq["temperature"], top_p=rq["top_p"], seed=rq["seed"])
    if family == "pen":
        kw.update(presence=rq["presence"], frequency=rq["frequency"])
    toks, why, _ = tw.decode_until([0], [rq["prompt"][-1]], rq["max_tokens"], stop=rq.get("stop") or None, **kw)
    _, g_state, g_misses = tw.guide_state(0)
    out = dict(tokens=toks[0], why=int(why[0]), guide_state=g_state, guide_misses=g_misses)
    if top_n is not None:
        chosen, ids, vals = tw.logprobs()
        n = len(toks[0])
        out.update(chosen=chosen[0, :n], ids=ids[0, :n], vals=vals[0, :n])
    tw.free()
    return out


def _check_against_twins(m, b, got, reqs, family, guides, biases, top_n, prefix_state, n_lanes=len(LANES)):
    """every request of `got` against its twin; the report of the batch against the twins' rows, and empty behind every length"""
    Rn = len(reqs)
    lens = [len(t) for t in got["tokens"]]
    report = b.logprobs() if top_n is not None else None
    if report is not None:
        stride = max(rq["max_tokens"] for rq in reqs)
        assert report[0].shape == (Rn, stride) and report[1].shape == report[2].shape == (Rn, stride, top_n)
    for q, rq in enumerate(reqs):
        tw = _twin(m, family, rq, prefix_state, guides, biases, top_n)
        where = (family, top_n, q)
        assert np.array_equal(got["tokens"][q], tw["tokens"]), (where, got["tokens"][q], tw["tokens"])
        assert int(got["stopped_by"][q]) == tw["why"], (where, got["stopped_by"][q], tw["why"])
        assert (int(got["guide_state"][q]), int(got["guide_misses"][q])) == (tw["guide_state"], tw["guide_misses"]), (where, got["guide_state"][q], got["guide_misses"][q], tw)
        if rq.get("guide") is None:
            assert (int(got["guide_state"][q]), int(got["guide_misses"][q])) == (0, 0), where
        if report is None:
            continue
        chosen, ids, vals = (a[q] for a in report)
        n = lens[q]
        assert np.array_equal(_bits(chosen[:n]), _bits(tw["chosen"])), (where, chosen[:n], tw["chosen"])
        assert np.array_equal(ids[:n], tw["ids"]) and np.array_equal(_bits(vals[:n]), _bits(tw["vals"])), (where, "top-N")
        assert (chosen[n:] == 0.0).all() and (ids[n:] == NO_TOKEN).all() and np.isneginf(vals[n:]).all(), (where, "behind the length")
    lane_want, start_want, _ = serve_rule([len(rq["prompt"]) for rq in reqs], lens, n_lanes)
    assert got["lane"].tolist() == lane_want and got["start_pass"].tolist() == start_want, (family, got["lane"], lane_want, got["start_pass"], start_want)
    return lens, lane_want


def _followers(lane, has):
    """(has[a], has[b]) of every two requests that follow each other on a lane"""
    pairs = set()
    for r in set(lane):
        mine = [q for q in range(len(lane)) if lane[q] == r]
        pairs |= {(has[a], has[b]) for a, b in zip(mine, mine[1:])}
    return pairs


# ---- 1. the guarantee on a mixed queue ----

@pytest.mark.parametrize("top_n", [None, 0, 3])
@pytest.mark.parametrize("family", ["sample", "pen"])
def test_every_request_of_a_mixed_queue_is_the_request_alone(tmp_path, family, top_n):
    m = model(_synth(tmp_path, "test-v6", "Q5_1"))
    V = m.n_vocab
    guides, biases = _guides(V), _biases(V)
    b = _fresh(m, family)
    prefix_state = b.state_store(PREFIX_SLOT)
    slot_words = [b.guide_state(s) for s in range(N_SLOTS)]
    reqs = _queue(V, family)
    if top_n is not None:
        b.set_logprobs(top_n)
    got = b.serve(LANES, reqs, FAMILY_ID[family], report=top_n is not None)
    lens, lane = _check_against_twins(m, b, got, reqs, family, guides, biases, top_n, prefix_state)
    assert lens == BUDGETS
    # the queue is ordered so that the lanes see every hand-over that could leave something behind
    guided, biased = [rq.get("guide") is not None for rq in reqs], [rq.get("bias_slot") is not None for rq in reqs]
    assert {(True, False), (False, True)} <= _followers(lane, guided)
    if family == "pen":
        assert (True, False) in _followers(lane, biased)
    # the lane slots' own guide words are neither read nor written
    assert [b.guide_state(s) for s in range(N_SLOTS)] == slot_words == [(NO_GUIDE, 0, 0)] * N_SLOTS
    b.free()
    m.free()


# ---- 2. the same as the plain call ----

def _raw_ex(b, lanes, family, reqs, extras="build", stride=None, override=None):
    """rwkv_mi_batch_serve_ex through the C ABI with every output given; extras: "build" (serve_extras of the queue), None, or a table;
    override: arguments to replace (a number, or a pointer by None). (ok, outputs)"""
    arr, prompts, seq_lens, seq_tokens = pkg.serve_requests(reqs)
    if extras == "build":
        extras = pkg.serve_extras(reqs)
    s = np.asarray(lanes, dtype=np.uint32)
    Rn = max(len(arr), 1)
    stride = max([int(r.stop.max_tokens) for r in arr], default=0) if stride is None else stride
    names = ("tokens_out", "lens_out", "why_out", "lane_out", "start_out", "last_out", "g_state_out", "g_misses_out")
    outs = {k: np.zeros(Rn, dtype=np.uint32) for k in names}
    outs["tokens_out"] = np.zeros((Rn, max(stride, 1)), dtype=np.uint32)
    outs["last_out"] = np.zeros(max(s.size, 1), dtype=np.uint32)
    a = dict(lanes=s.ctypes.data_as(P_U32), n=s.size, family=family, requests=arr, n_requests=len(arr), prompts=prompts.ctypes.data_as(P_U32),
             seq_lens=seq_lens.ctypes.data_as(P_U32), seq_tokens=seq_tokens.ctypes.data_as(P_U32), stride=stride, extras=extras)
    a.update({k: v.ctypes.data_as(P_U32) for k, v in outs.items()})
    a.update(override or {})
    ok = b._L.rwkv_mi_batch_serve_ex(b._ptr, a["lanes"], a["n"], a["family"], a["requests"], a["n_requests"], a["prompts"], a["seq_lens"], a["seq_tokens"],
                                     a["stride"], a["tokens_out"], a["lens_out"], a["why_out"], a["lane_out"], a["start_out"], a["last_out"], None,
                                     a["extras"], a["g_state_out"], a["g_misses_out"])
    return bool(ok), outs


@pytest.mark.parametrize("family", ["sample", "pen"])
def test_unguided_unbiased_requests_draw_what_they_draw_through_the_plain_call(tmp_path, family):
    m = model(_synth(tmp_path, "test-v6", "Q5_1"))
    V = m.n_vocab
    reqs = _queue(V, family)
    plain = [{k: v for k, v in rq.items() if k not in ("guide", "guide_state", "bias_slot")} for rq in reqs]
    assert pkg.serve_extras(reqs) is not None and pkg.serve_extras(plain) is None
    b, p = _fresh(m, family), _fresh(m, family)
    got = b.serve(LANES, reqs, FAMILY_ID[family])
    want = p.serve(LANES, plain, FAMILY_ID[family])   # (rwkv_mi_batch_serve: no request names an extra)
    # no stop sequence: every request runs to its budget in both, so the two schedules are one
    assert got["lane"].tolist() == want["lane"].tolist() and got["start_pass"].tolist() == want["start_pass"].tolist()
    same = [q for q in range(R) if reqs[q] == plain[q]]
    assert len(same) >= 4
    for q in same:
        assert np.array_equal(got["tokens"][q], want["tokens"][q]), (family, q)
    assert any(not np.array_equal(got["tokens"][q], want["tokens"][q]) for q in range(R) if q not in same), "no guide or bias changed a draw"
    b.free()
    p.free()
    m.free()


@pytest.mark.parametrize("family", ["greedy", "pen"])
def test_without_extras_and_report_the_call_is_the_plain_call(tmp_path, family):
    m = model(_synth(tmp_path, "test-v6", "Q5_1"))
    V = m.n_vocab
    plain = [{k: v for k, v in rq.items() if k not in ("guide", "guide_state", "bias_slot")} for rq in _queue(V, family)]
    b, p = _fresh(m, family), _fresh(m, family)
    ok, outs = _raw_ex(b, LANES, FAMILY_ID[family], plain, extras=None)
    assert ok
    want = p.serve(LANES, plain, FAMILY_ID[family])
    assert b.last_loop_passes() == p.last_loop_passes()
    for q in range(R):
        n = int(outs["lens_out"][q])
        assert np.array_equal(outs["tokens_out"][q, :n], want["tokens"][q]) and (outs["tokens_out"][q, n:] == NO_TOKEN).all(), (family, q)
    for key, name in (("why_out", "stopped_by"), ("lane_out", "lane"), ("start_out", "start_pass"), ("last_out", "last_request")):
        assert np.array_equal(outs[key], want[name]), (family, key)
    assert not outs["g_state_out"].any() and not outs["g_misses_out"].any()
    for s in range(N_SLOTS):
        assert np.array_equal(b.state_store(s), p.state_store(s)), (family, s)
    b.free()
    p.free()
    m.free()


# ---- 3. `chosen` against the scorer ----

def test_chosen_is_the_scorers_log_prob_and_a_successor_on_the_lane_leaves_the_rows_alone(tmp_path):
    m = model(_synth(tmp_path, "test-v6", "Q5_1"))
    V = m.n_vocab
    family = "pen"
    b = _fresh(m, family)
    reqs = _queue(V, family)
    b.set_logprobs(3)
    got = b.serve(LANES, reqs, FAMILY_ID[family], report=True)
    chosen, ids, vals = b.logprobs()
    lane = got["lane"].tolist()
    # request 0 and the request that took its lane after it: the first one's rows were written long before the second one's
    first, second = 0, min(q for q in range(1, R) if lane[q] == lane[0])
    assert int(got["start_pass"][second]) > 0
    scorer = pkg.RWKVBatch(m, 1)
    for q in (first, second):
        emitted = [int(t) for t in got["tokens"][q]]
        prompt, n = reqs[q]["prompt"], len(emitted)
        scorer.state_load(0, None)
        targets = [NO_SLOT] * (len(prompt) - 1) + emitted   # (NO_TARGET: the prompt's own positions are not scored)
        lp, _ = scorer.score_ragged([0], [prompt + emitted[:-1]], [targets], want_argmax=False)
        assert np.array_equal(_bits(chosen[q, :n]), _bits(lp[0][len(prompt) - 1:])), (q, chosen[q, :n], lp[0])
        assert (chosen[q, n:] == 0.0).all() and (ids[q, n:] == NO_TOKEN).all() and np.isneginf(vals[q, n:]).all(), q
        # the top-N is of the model's logits: descending, its first entry the largest log-prob of the step
        assert (np.diff(vals[q, :n], axis=1) <= 0).all() and (vals[q, :n, 0] >= chosen[q, :n]).all(), q
    scorer.free()
    b.free()
    m.free()


# ---- 4. a guide that drives the stop ----

def test_a_chain_guide_ends_its_request_by_the_stop_sequence_and_hands_the_lane_on(tmp_path):
    m = model(_synth(tmp_path, "test-v6", "Q5_1"))
    V = m.n_vocab
    family = "sample"
    chain = [41, 7, 300, 12]
    # state i allows chain[i] alone; the last state (every state must allow a token) goes round on the last token
    guide = [{chain[i]: i + 1} for i in range(len(chain))] + [{chain[-1]: len(chain)}]
    extras = [(None, None, None), (0, 0, None), (None, None, None), (None, None, None), (None, None, None)]
    reqs = _queue(V, family, extras, [1, 2, 1, 3, 1], [7, 9, 3, 4, 2])
    reqs[1]["stop"] = [[V - 1, V - 2], [chain[-1]]]
    b = _fresh(m, family, guides=[guide])
    got = b.serve(LANES, reqs, FAMILY_ID[family])
    assert got["tokens"][1].tolist() == chain and int(got["stopped_by"][1]) == 1
    assert (int(got["guide_state"][1]), int(got["guide_misses"][1])) == (len(chain), 0)
    lens = [len(t) for t in got["tokens"]]
    assert lens == [7, len(chain), 3, 4, 2]
    lane_want, start_want, _ = serve_rule([1, 2, 1, 3, 1], lens, len(LANES))
    assert got["lane"].tolist() == lane_want and got["start_pass"].tolist() == start_want
    # lane 1 is free after the pass that drew the chain's last token: 1 prompt pass + 4 tokens
    assert lane_want[4] == 1 and start_want[4] == 1 + len(chain)
    _check_against_twins(m, b, got, reqs, family, [guide], {}, None, None)
    b.free()
    m.free()


# ---- 5. misses ----

def test_a_bias_that_forbids_every_allowed_token_counts_misses_and_leaves_the_state(tmp_path):
    m = model(_synth(tmp_path, "test-v6", "Q5_1"))
    V = m.n_vocab
    family = "pen"
    # state 1 allows three tokens, all of them biased to -inf: every draw from it is a dead pick
    guide = [{j: 1 for j in range(V)}, {3: 0, 5: 0, 9: 0}]
    biases = {1: {3: float("-inf"), 5: float("-inf"), 9: float("-inf")}, 3: {2: 1.0}}
    extras = [(None, None, None), (0, 1, 1), (None, None, None), (0, 0, 1)]
    reqs = _queue(V, family, extras, [1, 2, 1, 1], [4, 6, 2, 5])
    b = _fresh(m, family, guides=[guide], biases=biases)
    got = b.serve(LANES, reqs, FAMILY_ID[family])
    assert (int(got["guide_state"][1]), int(got["guide_misses"][1])) == (1, 6)
    assert (int(got["guide_state"][3]), int(got["guide_misses"][3])) == (1, 4)   # (one live draw into state 1, then four dead ones)
    _check_against_twins(m, b, got, reqs, family, [guide], biases, None, None)
    b.free()
    m.free()


# ---- 6. the greedy family reports ----

def test_the_greedy_family_reports_what_greedy_decode_until_reports(tmp_path):
    m = model(_synth(tmp_path, "test-v6", "Q5_1"))
    V = m.n_vocab
    family = "greedy"
    b = _fresh(m, family)
    prefix_state = b.state_store(PREFIX_SLOT)
    reqs = _queue(V, family)
    assert pkg.serve_extras(reqs) is None
    b.set_logprobs(2)
    got = b.serve(LANES, reqs, FAMILY_ID[family], report=True)
    _check_against_twins(m, b, got, reqs, family, [], {}, 2, prefix_state)
    # the greedy token is the first of its step's top-N
    chosen, ids, vals = b.logprobs()
    for q in range(R):
        assert np.array_equal(ids[q, :BUDGETS[q], 0], got["tokens"][q]) and np.array_equal(_bits(vals[q, :BUDGETS[q], 0]), _bits(chosen[q, :BUDGETS[q]])), q
    b.free()
    m.free()


# ---- 7. the block of the loop cannot be seen in the results ----

def test_loop_block_of_one_and_sixteen_give_the_same(tmp_path):
    m = model(_synth(tmp_path, "test-v6", "Q5_1"))
    V = m.n_vocab
    family = "pen"
    results = {}
    saved = os.environ.get("RWKV_MI_LOOP_BLOCK")
    try:
        for block in (1, 16):
            os.environ["RWKV_MI_LOOP_BLOCK"] = str(block)   # (read at the call)
            b = _fresh(m, family)
            b.set_logprobs(3)
            got = b.serve(LANES, _queue(V, family), FAMILY_ID[family], report=True)
            need = serve_rule(PROMPT_LENS, [len(t) for t in got["tokens"]], len(LANES))[2]
            assert need <= b.last_loop_passes() <= need + 2 * block, (block, b.last_loop_passes(), need)
            results[block] = (got, b.logprobs(), [b.state_store(s) for s in range(N_SLOTS)])
            b.free()
    finally:
        if saved is None:
            os.environ.pop("RWKV_MI_LOOP_BLOCK", None)
        else:
            os.environ["RWKV_MI_LOOP_BLOCK"] = saved
    (g1, r1, s1), (g16, r16, s16) = results[1], results[16]
    assert all(np.array_equal(a, c) for a, c in zip(g1["tokens"], g16["tokens"]))
    for key in ("stopped_by", "lane", "start_pass", "last_request", "guide_state", "guide_misses"):
        assert np.array_equal(g1[key], g16[key]), key
    assert np.array_equal(_bits(r1[0]), _bits(r16[0])) and np.array_equal(r1[1], r16[1]) and np.array_equal(_bits(r1[2]), _bits(r16[2]))
    assert all(np.array_equal(a, c) for a, c in zip(s1, s16))
    m.free()


# ---- 8. a vocabulary that is no multiple of four: the word form of the reset, a guide table of that width ----

def test_guided_queue_on_a_vocabulary_of_50277_tokens(tmp_path):
    m = model(_synth(tmp_path, "slice-v4-768", "Q8_0"))
    V = m.n_vocab
    assert V == 50277
    family = "pen"
    # the odd row length puts every state's row of the 2-byte table on another alignment
    guide = [{j: 1 + (j // 2) % 2 for j in range(0, V, 2)}, {j: 0 for j in range(1, V, 5)}, {j: (j // 7) % 3 for j in range(0, V, 7)}]
    biases = {1: {V - 1: 4.0, 10: float("-inf"), 50000: 2.5}, 3: {0: 1.0}}
    extras = [(0, 2, 1), (None, None, None), (0, 0, None), (None, None, 1), (0, 1, None)]
    reqs = _queue(V, family, extras, [1, 2, 1, 1, 3], [3, 2, 4, 2, 3])
    b = _fresh(m, family, guides=[guide], biases=biases)
    prefix_state = b.state_store(PREFIX_SLOT)
    b.set_logprobs(3)
    got = b.serve(LANES, reqs, FAMILY_ID[family], report=True)
    _check_against_twins(m, b, got, reqs, family, [guide], biases, 3, prefix_state)
    b.free()
    m.free()


# ---- 9. rejections ----

def test_rejections_change_nothing(tmp_path):
    m = model(_synth(tmp_path, "test-v6", "Q5_1"))
    V = m.n_vocab
    family = "pen"

    def prepared():
        """a batch with a guide attached to a bystander (its words exist and are not zero) and a report of its own"""
        x = _fresh(m, family)
        x.attach_guide(6, 0, 2)
        x.set_logprobs(2)
        x.decode_until([7], [3], 4, temperature=1.0, top_p=0.9, seed=5, presence=0.1, frequency=0.1)
        return x

    b, tw = prepared(), prepared()
    every = list(range(N_SLOTS))

    def words():
        """what a rejected call must leave: state, counts and guide words of every slot, and the current report, by their bits"""
        per_slot = [(b.state_store(s).tobytes(), b.counts(s).tobytes(), b.guide_state(s)) for s in every]
        return per_slot, [a.tobytes() for a in b.logprobs()]

    def rejected(what, lanes=LANES, fam=2, change=None, extras="build", stride=None, null=(), mutate=None):
        reqs = _queue(V, "pen" if fam == 2 else "sample" if fam == 1 else "greedy")
        for q, kv in (change or {}).items():
            reqs[q].update(kv)
        if mutate:
            extras = mutate(pkg.serve_extras(reqs))
        before = words()
        ok, _ = _raw_ex(b, lanes, fam, reqs, extras=extras, stride=stride, override={name: None for name in null})
        err = m._library.rwkv_get_last_error(m._ctx)
        assert not ok and err & ARGS, (what, ok, err)
        assert words() == before, (what, "a rejected call changed something")

    def reserved(ex):
        ex[5].reserved = 1
        return ex

    # what rwkv_mi_batch_serve rejects -- but for the report, which is on throughout
    rejected("a lane twice", lanes=[4, 0, 4])
    rejected("a lane out of range", lanes=[4, 0, N_SLOTS])
    rejected("an unknown family", fam=3)
    rejected("a from_slot that is a lane", change={6: dict(from_slot=LANES[1])})
    rejected("lens_out NULL", null=("lens_out",))
    rejected("a max_tokens of 0", change={1: dict(max_tokens=0)})
    rejected("stride below the largest max_tokens", stride=8)
    b.set_logit_bias(LANES[0], {3: 2.0})
    rejected("a lane whose slot has a bias set")
    b.set_logit_bias(LANES[0], {})
    b.attach_guide(LANES[2], 1, 0)
    rejected("a lane whose slot has a guide attached")
    b.detach_guide(LANES[2])
    tw.attach_guide(LANES[2], 1, 0)   # (attach and detach zero the slot's words: the same on the twin)
    tw.detach_guide(LANES[2])
    # what the extras add
    rejected("a guide that names no guide", change={0: dict(guide=2)})
    rejected("a guide beyond the batch's limit", change={0: dict(guide=pkg.GUIDE_MAX)})
    rejected("a guide_state that is no state", change={0: dict(guide_state=3)})
    rejected("a bias_slot out of range", change={6: dict(bias_slot=N_SLOTS)})
    rejected("a bias_slot that is a lane", change={6: dict(bias_slot=LANES[0])})
    rejected("a bias_slot with no bias set", change={6: dict(bias_slot=7)})
    rejected("a guided request in the greedy family", fam=0, change={0: dict(guide=0, guide_state=0)})
    rejected("a bias_slot in the sampled family", fam=1, change={6: dict(bias_slot=3)})
    rejected("a bias_slot in the greedy family", fam=0, change={6: dict(bias_slot=3)})
    rejected("reserved that is not 0", mutate=reserved)
    rejected("the report on and a stride of 0", stride=0)
    # nothing moved since the start either -- against a batch that saw none of the calls -- and the draw counters stand: the next generator draw
    for s in every:
        assert np.array_equal(b.state_store(s), tw.state_store(s)), s
        assert np.array_equal(b.counts(s), tw.counts(s)), s
        assert b.guide_state(s) == tw.guide_state(s) == ((0, 2, 0) if s == 6 else (NO_GUIDE, 0, 0)), s
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(b.logprobs(), tw.logprobs()))
    a = (every, [_tok(3, s, V) for s in every], 1.0, 1.0, -1.0, list(range(50, 50 + N_SLOTS)), 0.2, 0.2, False)
    assert np.array_equal(b.eval_sample_penalized(*a), tw.eval_sample_penalized(*a))
    # ... and the same call with nothing wrong goes through
    ok, outs = _raw_ex(b, LANES, 2, _queue(V, "pen"))
    assert ok and outs["lens_out"].tolist() == BUDGETS
    b.free()
    tw.free()
    m.free()
