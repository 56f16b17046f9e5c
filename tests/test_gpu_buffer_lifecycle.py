"""The life of the buffers a context and a batch own (csrc/devmem.h): grown, reused, grown again, left alone by a rejected call, released
with their owner -- seen through what the calls compute. Every result is held against the CPU oracle (tests/oracle_lib.py) run from the same
states: np.array_equal on tokens, ids, logits and states; the log-probs with the one tolerance of tests/test_gpu_score.py (check_logprob,
check_rows) and tests/test_gpu_logprobs.py (check_against_f64). Nothing is compared with an earlier output of the library.

Files: the RWKV-4 FP16 and the RWKV-6 Q5_1 tiny models of tests/golden. Sizes: a batch's token words start at n_slots (4) and its segment
tables at nothing, so passes of 3, 70 (one segment of 33: a sequence kernel's), 3 and 150 tokens grow both, reuse them and grow them again;
the report buffers grow with steps * rows * top_n (2 steps, 40 steps, then top_n 2 -> 5), the scoring words past their first 1024 rows never
in a test this small -- what grows there is the token words under them (5, then 100 positions). The staged tables of the queue, the stop
words, the beam words and the draft words (csrc/call_layout.h) on one batch, one call after the other: a queue of 4 requests with 4 tokens
a request, one of 12 with 16 (the table grows), a rejected one, the first again (the table is reused), one with a guided request (the guide
fields appear), then decode_until, decode_beam, eval_draft and a ragged pass of 70 tokens. The requests are held against the oracle's
greedy walk under tests/test_cpu_batch_until.py's stop rule and tests/guide_ref.py's masks, the schedule against
tests/test_cpu_batch_serve.py's model of it, the beam against tests/test_gpu_beam.py's host-driven search run on the oracle."""
import ctypes

import numpy as np
import pytest

import guide_ref as G
import oracle_lib as O
import reference_constants as R
from gpu_lib import model, pkg
from logprobs_ref import f64_logprobs, top_ids
from test_cpu_batch_serve import serve_rule
from test_cpu_batch_until import NO_TOKEN, stop_rule
from test_gpu_beam import bits32, bits64, host_search
from test_gpu_logprobs import check_against_f64
from test_gpu_score import check_rows

pytestmark = pytest.mark.gpu

ARGS = 1 << 8   # RWKV_ERROR_ARGS
P_UINT32 = ctypes.POINTER(ctypes.c_uint32)
FILES = [("4v0-660K", "FP16"), ("6v0-3m", "Q5_1")]
N_SLOTS = 4


def _tokens(call, slot, n, V):
    return [(41 * call + 13 * slot + 23 * j + 3) % V for j in range(n)]


def _open(golden_dir, version, fmt):
    path = R.fixture_path(golden_dir, version, fmt)
    return model(path), O.OracleModel(path)


def _fresh(om):
    return {s: om.init_state() for s in range(N_SLOTS)}


def _load(b, ost):
    for s, st in ost.items():
        b.state_load(s, st)


def _same_states(b, ost, what):
    for s, st in ost.items():
        assert np.array_equal(b.state_store(s), st), (what, "state of slot", s)


def _ragged_pass(b, om, ost, call, lens, what):
    """one eval_ragged of the given lengths on slots 0 ..: logits and every slot's state against the oracle (ost advanced in place)"""
    slots = list(range(len(lens)))
    rows = [_tokens(call, s, n, om.n_vocab) for s, n in zip(slots, lens)]
    got = b.eval_ragged(slots, rows)
    for s in slots:
        want, ost[s] = om.eval_sequence(rows[s], ost[s])
        assert np.array_equal(got[s], want), (what, "logits of slot", s)
    _same_states(b, ost, what)


def _oracle_greedy(om, state, first, steps):
    """(tokens [steps], logits [steps][V], state after) of the greedy loop from `state`"""
    toks, logits, tok = [], [], first
    for _ in range(steps):
        lg, state = om.eval(tok, state)
        tok = int(np.argmax(lg))
        toks.append(tok); logits.append(lg)
    return np.asarray(toks, dtype=np.uint32), np.stack(logits), state


def _greedy_loop(b, om, ost, slots, firsts, steps, top_n, what):
    """one decode_greedy with the report on: tokens, top ids, chosen and top log-probs and the slots' states against the oracle"""
    toks, _ = b.decode_greedy(slots, firsts, steps)
    chosen, ids, lps = b.logprobs()
    assert chosen.shape == (len(slots), steps) and ids.shape == (len(slots), steps, top_n) and lps.shape == ids.shape, what
    for r, s in enumerate(slots):
        want, logits, ost[s] = _oracle_greedy(om, ost[s], firsts[r], steps)
        assert np.array_equal(toks[r], want), (what, "tokens of slot", s)
        for i in range(steps):
            assert np.array_equal(ids[r, i], top_ids(logits[i], top_n)), (what, "top ids", s, i)
            ref = f64_logprobs(logits[i], np.concatenate([[want[i]], ids[r, i]]))
            check_against_f64(chosen[r, i], ref[0], (what, "chosen", s, i))
            for k in range(top_n):
                check_against_f64(lps[r, i, k], ref[1 + k], (what, "top", s, i, k))
    _same_states(b, ost, what)


def _score(b, om, ost, call, lens, what):
    """one score_ragged of the given lengths on slots 0 ..: log-probs, argmax and the slots' states against the oracle"""
    V = om.n_vocab
    slots = list(range(len(lens)))
    rows = [_tokens(call, s, n, V) for s, n in zip(slots, lens)]
    tgts = [_tokens(call + 1, s, n, V) for s, n in zip(slots, lens)]
    lps, ams = b.score_ragged(slots, rows, tgts)
    for s in slots:
        logits = []
        for t in rows[s]:
            lg, ost[s] = om.eval(t, ost[s])
            logits.append(lg)
        check_rows(np.stack(logits), tgts[s], lps[s], ams[s], (what, "slot", s))
    _same_states(b, ost, what)


@pytest.mark.parametrize("version,fmt", FILES)
def test_ragged_tables_grow_are_reused_and_grow_again(golden_dir, version, fmt):
    m, om = _open(golden_dir, version, fmt)
    b = pkg.RWKVBatch(m, N_SLOTS)
    ost = _fresh(om)
    for call, lens in enumerate([(1, 1, 1), (33, 30, 5, 2), (1, 1, 1), (40, 70, 39, 1)]):
        _ragged_pass(b, om, ost, call, lens, (version, fmt, "pass of", sum(lens)))
    b.free(); m.free()


@pytest.mark.parametrize("version,fmt", FILES)
def test_report_and_score_buffers_grow_are_reused_and_grow_again(golden_dir, version, fmt):
    m, om = _open(golden_dir, version, fmt)
    b = pkg.RWKVBatch(m, N_SLOTS)
    ost = _fresh(om)
    slots, firsts = [0, 1, 2], [34, 105, 110]
    b.set_logprobs(2)
    _greedy_loop(b, om, ost, slots, firsts, 2, 2, (version, fmt, "2 steps"))
    _greedy_loop(b, om, ost, slots, firsts, 40, 2, (version, fmt, "40 steps"))
    b.set_logprobs(5)
    _greedy_loop(b, om, ost, slots, firsts, 2, 5, (version, fmt, "2 steps, top 5"))
    _score(b, om, ost, 7, (2, 3), (version, fmt, "5 positions"))
    _score(b, om, ost, 9, (60, 40), (version, fmt, "100 positions"))
    # the context's own report and scoring words, the same pattern: draws at temperature 0 are the argmax
    m.set_logprobs(2)
    st = om.init_state()
    m.state_load(None)
    for steps in (2, 40):
        toks, _ = m.decode_sample(34, steps, temperature=0.0)
        chosen, ids, lps = m.logprobs()
        want, logits, st = _oracle_greedy(om, st, 34, steps)
        assert np.array_equal(toks, want), (version, fmt, "context loop", steps)
        for i in range(steps):
            assert np.array_equal(ids[0, i], top_ids(logits[i], 2)), (version, fmt, "context top ids", steps, i)
            check_against_f64(chosen[0, i], f64_logprobs(logits[i], [want[i]])[0], (version, fmt, "context chosen", steps, i))
        assert np.array_equal(m.state_store(), st), (version, fmt, "context state", steps)
    for n in (5, 100):
        rows, tg = _tokens(11, n, n, om.n_vocab), _tokens(12, n, n, om.n_vocab)
        lp, am, _ = m.score_resident(rows, tg)
        logits = []
        for t in rows:
            lg, st = om.eval(t, st)
            logits.append(lg)
        check_rows(np.stack(logits), tg, lp, am, (version, fmt, "context score", n))
        assert np.array_equal(m.state_store(), st), (version, fmt, "context state after score", n)
    b.free(); m.free()


def _touch_every_family(m, b, om):
    """one call of every family that allocates on first use, on a context and a batch; what is cheap to hold against the oracle is held"""
    V = om.n_vocab
    lg, st = om.eval(34, om.init_state())
    top = int(np.argmax(lg))
    assert np.array_equal(m.eval(34, None)[0], lg)
    assert m.sample(temperature=0.0) == top                                       # sampler scratch, draw counter
    m.counts_add([top, top, 5])                                                   # occurrence and bias tables
    want_counts = np.zeros(V, dtype=np.uint32); want_counts[top] = 2; want_counts[5] = 1
    assert np.array_equal(m.counts(), want_counts)
    m.set_logit_bias({top: -1e30})
    second = int(top_ids(lg, 2)[1])
    assert m.sample_penalized(temperature=0.0, presence=0.0, frequency=0.0, record=False) == second   # (the bias forbids the argmax)
    m.set_logprobs(2)                                                             # report
    assert m.sample(temperature=0.0) == top
    assert np.array_equal(m.logprobs()[1][0, 0], top_ids(lg, 2))
    lp, am, _ = m.score_resident([105, 110], [1, 2])                              # scoring words
    l1, st = om.eval(105, st); l2, st = om.eval(110, st)
    check_rows(np.stack([l1, l2]), [1, 2], lp, am, "context score")
    # the batch
    ost = _fresh(om)
    slots, toks = [0, 1], [34, 105]
    rl = {}
    for s, t in zip(slots, toks):
        rl[s], ost[s] = om.eval(t, ost[s])
    got = b.eval_sample(slots, toks, temperature=0.0)                             # sampler scratch and row table
    assert np.array_equal(got, [int(np.argmax(rl[s])) for s in slots])
    for s, t in zip(slots, toks):
        rl[s], ost[s] = om.eval(t, ost[s])
    b.counts_add(0, [7, 7]); b.set_logit_bias(0, {int(np.argmax(rl[0])): -1e30})  # occurrence and bias tables (the bias forbids row 0's argmax)
    want_counts = np.zeros(V, dtype=np.uint32); want_counts[7] = 2
    assert np.array_equal(b.counts(0), want_counts)
    got = b.eval_sample_penalized(slots, toks, temperature=0.0, presence=0.0, frequency=0.0, record=False)   # penalised row table
    assert np.array_equal(got, [int(top_ids(rl[0], 2)[1]), int(np.argmax(rl[1]))])
    rows = [_tokens(3, 0, 33, V), _tokens(3, 1, 2, V)]                            # segment tables, token words
    got = b.eval_ragged(slots, rows)
    for s in slots:
        want, ost[s] = om.eval_sequence(rows[s], ost[s])
        assert np.array_equal(got[s], want)
    want, _, ost[2] = _oracle_greedy(om, ost[2], 34, 6)                           # stop tables: slot 2 stops at its own third token
    out, why, _ = b.decode_until([2], [34], 6, stop=[[int(want[2])]])
    n = int(np.flatnonzero(want == want[2])[0]) + 1
    assert np.array_equal(out[0], want[:n]) and int(why[0]) == 0
    _, _, ost[2] = _oracle_greedy(om, om.init_state(), 34, n)
    b.set_logprobs(2)                                                             # report
    _greedy_loop(b, om, ost, [3], [110], 3, 2, "batch report")
    _score(b, om, ost, 5, (3, 2), "batch score")                                  # scoring words


@pytest.mark.parametrize("version,fmt", FILES)
def test_every_lazy_family_on_one_object_then_free_and_create_again(golden_dir, version, fmt):
    m, om = _open(golden_dir, version, fmt)
    b = pkg.RWKVBatch(m, N_SLOTS)
    _touch_every_family(m, b, om)
    b.free(); m.free()
    # a double free, or a buffer released under a stream still using it, is a HIP error on the next calls: the device must be as usable as before
    m, _ = _open(golden_dir, version, fmt)
    b = pkg.RWKVBatch(m, N_SLOTS)
    want, logits, st = _oracle_greedy(om, om.init_state(), 34, 1)
    toks, _ = b.decode_greedy([0], [34], 1)
    assert np.array_equal(toks[0], want) and np.array_equal(b.state_store(0), st), (version, fmt)
    lg, s2 = m.eval(34, None)
    assert np.array_equal(lg, logits[0]) and np.array_equal(s2, st), (version, fmt)
    b.free(); m.free()


@pytest.mark.parametrize("version,fmt", FILES)
def test_a_rejected_call_leaves_the_buffers_as_they_were(golden_dir, version, fmt):
    m, om = _open(golden_dir, version, fmt)
    b = pkg.RWKVBatch(m, N_SLOTS)
    L = m._library.library
    u32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.uint32)).ctypes.data_as(P_UINT32)
    # a ragged pass; a call whose lengths add up past the limit (rejected before anything grows); the same pass from the same states again
    start = _fresh(om)
    for attempt in range(2):
        ost = {s: st.copy() for s, st in start.items()}
        _load(b, ost)
        _ragged_pass(b, om, ost, 1, (33, 30, 5, 2), (version, fmt, "ragged, attempt", attempt))
        if attempt == 0:
            assert not L.rwkv_mi_batch_eval_ragged(b._ptr, u32([0, 1]), u32([0x7FFFFFFF, 2]), u32([1, 2, 3]), 2, None)
            assert m._library.rwkv_get_last_error(m._ctx) & ARGS
            _same_states(b, ost, (version, fmt, "after the rejected ragged call"))
    # a reporting loop; top_n above RWKV_MI_TOP_MAX (rejected: the report stays as it was set); the same loop from the same states again
    b.set_logprobs(2)
    for attempt in range(2):
        ost = {s: st.copy() for s, st in start.items()}
        _load(b, ost)
        _greedy_loop(b, om, ost, [0, 1, 2], [34, 105, 110], 4, 2, (version, fmt, "loop, attempt", attempt))
        if attempt == 0:
            with pytest.raises(ValueError):
                b.set_logprobs(pkg.TOP_MAX + 1)
            assert b.last_error & ARGS
    b.free(); m.free()


def _oracle_request(om, state, prompt, max_tokens, stop=(), guide=None, g_state=0):
    """(tokens, stopped_by, state after, guide state, misses) of a request alone: the prompt fed from `state`, then every step's argmax -- under
    `guide`, of the tokens it allows (guide_ref) -- fed in turn, ended by stop_rule. The last token is not fed: the state is that of the plain
    loop of the request's length. A row of decode_until is the request whose prompt is the row's first token, from the slot's state."""
    for t in prompt:
        lg, state = om.eval(t, state)
    toks, states, words = [], [], [(g_state, 0)]
    for _ in range(max_tokens):
        tok = int(np.argmax(lg if guide is None else np.where(guide.mask(words[-1][0]), lg, -np.inf)))
        if guide is not None:
            nxt, miss = guide.step(words[-1][0], tok)
            words.append((nxt, words[-1][1] + miss))
        toks.append(tok); states.append(state)
        lg, state = om.eval(tok, state)
    n, why = stop_rule(toks, max_tokens, stop)
    return np.asarray(toks[:n], dtype=np.uint32), why, states[n - 1], words[n if guide is not None else 0]


def _serve(b, om, ost, lanes, reqs, what, family=pkg.SERVE_GREEDY, guides=None):
    """one serve call: every request against the request alone from the fresh state, the lanes and start passes against serve_rule, the guide
    words against the guide's walk, and every slot's state -- a lane holds the end state of its last request, no other slot changes"""
    got = b.serve(lanes, reqs, family=family)
    want = [_oracle_request(om, om.init_state(), rq["prompt"], rq["max_tokens"], rq.get("stop") or [],
                            None if rq.get("guide") is None else guides[rq["guide"]], rq.get("guide_state", 0)) for rq in reqs]
    lane, start, _ = serve_rule([len(rq["prompt"]) for rq in reqs], [len(w[0]) for w in want], len(lanes))
    for q, w in enumerate(want):
        assert np.array_equal(got["tokens"][q], w[0]), (what, "tokens of request", q)
    assert np.array_equal(got["stopped_by"], [w[1] for w in want]), (what, "reasons")
    assert np.array_equal(got["lane"], lane) and np.array_equal(got["start_pass"], start), (what, "lanes and start passes")
    assert np.array_equal(got["guide_state"], [w[3][0] for w in want]) and np.array_equal(got["guide_misses"], [w[3][1] for w in want]), (what, "guide words")
    last = [max(q for q in range(len(reqs)) if lane[q] == r) for r in range(len(lanes))]
    assert np.array_equal(got["last_request"], last), (what, "last requests")
    for r, s in enumerate(lanes):
        ost[s] = want[last[r]][2]
    _same_states(b, ost, what)


class _OracleSlots:
    """the slots of a batch on the CPU oracle: what host_search (tests/test_gpu_beam.py) drives in place of a second batch"""

    def __init__(self, om, ost):
        self.om, self.ost = om, ost

    def state_store(self, s):
        return self.ost[s].copy()

    def state_load(self, s, st):
        self.ost[s] = np.array(st, dtype=np.float32)

    def eval(self, slots, tokens):
        out = []
        for s, t in zip(slots, tokens):
            lg, self.ost[s] = self.om.eval(t, self.ost[s])
            out.append(lg)
        return np.stack(out)


@pytest.mark.parametrize("version,fmt", FILES)
def test_staged_tables_grow_are_reused_and_outlive_a_rejected_call(golden_dir, version, fmt):
    m, om = _open(golden_dir, version, fmt)
    b = pkg.RWKVBatch(m, N_SLOTS)
    ost = _fresh(om)
    V = om.n_vocab
    small = [{"prompt": _tokens(1, q, 1 + q % 2, V), "max_tokens": 2 + q % 3} for q in range(4)]            # at most 4 tokens: stride 4
    big = [{"prompt": _tokens(2, q, 1 + q % 3, V), "max_tokens": 1 + 5 * q % 16} for q in range(12)]         # request 3 has 16: stride 16
    stream = _oracle_request(om, om.init_state(), big[4]["prompt"], big[4]["max_tokens"])[0]
    big[4]["stop"] = [[int(stream[1]), int(stream[2])]]                                                     # (its own second and third token)
    # 1, 2: the table of the first call, then a larger one
    _serve(b, om, ost, [2, 0], small, (version, fmt, "4 requests"))
    _serve(b, om, ost, [1, 3, 0], big, (version, fmt, "12 requests"))
    # 3: a lane named twice is rejected and changes nothing; 4: the first queue again, in the table the second one left
    with pytest.raises(ValueError):
        b.serve([1, 1], small)
    assert b.last_error & ARGS
    _same_states(b, ost, (version, fmt, "after the rejected queue"))
    _serve(b, om, ost, [2, 0], small, (version, fmt, "4 requests again"))
    # 5: a guided request among plain ones (guided greedy is temperature 0 of the sampled family): the guide fields of the table appear
    guide = G.random_guide(V, 3, seed=5)
    gid = b.create_guide(guide.edges)
    guided = [dict(rq, temperature=0.0) for rq in small]
    guided[1].update(guide=gid, guide_state=2)
    _serve(b, om, ost, [2, 0], guided, (version, fmt, "a guided request"), family=pkg.SERVE_SAMPLE, guides={gid: guide})
    # 6: decode_until: slot 1 ends at its own third token, slot 3 at its budget
    first, budgets = [34, 105], [6, 5]
    third = int(_oracle_request(om, ost[1], [first[0]], budgets[0])[0][2])
    stops = [[[third]], []]
    out, why, _ = b.decode_until([1, 3], first, budgets, stop=stops)
    for r, s in enumerate([1, 3]):
        toks, reason, ost[s], _ = _oracle_request(om, ost[s], [first[r]], budgets[r], stops[r])
        assert np.array_equal(out[r], toks) and int(why[r]) == reason, (version, fmt, "until, slot", s)
    assert int(why[0]) == 0 and int(why[1]) == NO_TOKEN and len(out[0]) <= 3 and len(out[1]) == 5, (version, fmt, "until", why)
    _same_states(b, ost, (version, fmt, "until"))
    # 7: decode_beam, one group of width 2 from slot 2's state, against the host-driven search on the oracle (which leaves ost where the call
    # leaves the slots: without end tokens every hypothesis is unfinished)
    tokens, lens, scores, lps, _ = b.decode_beam([[2, 0]], [110], 2, 4)
    wt, wl, ws, wlp, wfin = host_search(_OracleSlots(om, ost), [[2, 0]], [110], 2, 4, [])
    assert np.array_equal(tokens, wt) and np.array_equal(lens, wl), (version, fmt, "beam", tokens.tolist(), wt.tolist())
    assert np.array_equal(bits32(lps), bits32(wlp)) and np.array_equal(bits64(scores), bits64(ws)), (version, fmt, "beam scores")
    assert not wfin.any()
    _same_states(b, ost, (version, fmt, "beam"))
    # 8: eval_draft, a draft of 2 per row: slot 1's second draft token is wrong (one stands), slot 3's both stand
    rows = []
    for s, x0, wrong in ((1, 34, True), (3, 105, False)):
        true = _oracle_greedy(om, ost[s], x0, 3)[0]
        rows.append((s, x0, wrong, true))
    emitted, kept = b.eval_draft([1, 3], [[x0, int(true[0]), (int(true[1]) + (1 if wrong else 0)) % V] for _, x0, wrong, true in rows])
    for r, (s, x0, wrong, true) in enumerate(rows):
        n = 2 if wrong else 3
        assert int(kept[r]) == n and np.array_equal(emitted[r], true[:n]), (version, fmt, "draft, slot", s)
        ost[s] = _oracle_greedy(om, ost[s], x0, n)[2]
    _same_states(b, ost, (version, fmt, "draft"))
    # 9: a ragged pass of 70 tokens after all of them
    _ragged_pass(b, om, ost, 9, (33, 30, 5, 2), (version, fmt, "ragged pass of 70"))
    b.free(); m.free()
