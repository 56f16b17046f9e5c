"""Serve sessions (rwkv_mi_batch_serve_open .. _close; csrc/sampling.hip k_session_rows): the device loop of rwkv_mi_batch_serve kept open
between host calls. The oracle is the guarantee itself: every request alone on a one-slot twin batch (test_gpu_batch_serve._twin), whenever it
was submitted; a cancelled request gives a prefix of its twin's tokens. Who runs where and when -- lane, start pass, the length of a cancelled
request -- must be what test_cpu_batch_session.session_rule gives for the blocks counted at each submit and cancel. Every comparison is exact,
every case a legal call sequence."""
import os

import numpy as np
import pytest

import test_gpu_batch_serve_extras as X
from gpu_lib import model, pkg
from test_cpu_batch_session import session_rule
from test_gpu_batch_serve import (BUDGETS, FAMILIES, FAMILY_ID, LANES, MODELS, N_SLOTS, PREFIX_SLOT, PROMPT_LENS, R, _fresh, _queue_with_stop, _raw_counts, _requests, _synth,
                                  _twin)

pytestmark = pytest.mark.gpu

ARGS = 1 << 8   # RWKV_ERROR_ARGS
NO_TOKEN = 0xFFFFFFFF
CANCELLED = 0xFFFFFFFE
LIMITS = dict(capacity=R, max_prompt=max(PROMPT_LENS), stride=max(BUDGETS), max_seqs=2, max_seq_tokens=5)


def _features(family):
    return {"greedy": 0, "sample": pkg.SERVE_CUT, "pen": pkg.SERVE_CUT | pkg.SERVE_REP}[family]


class _block:
    """RWKV_MI_LOOP_BLOCK for the sessions opened inside (it is read at open)"""

    def __init__(self, K):
        self.K = K

    def __enter__(self):
        self.saved = os.environ.get("RWKV_MI_LOOP_BLOCK")
        os.environ["RWKV_MI_LOOP_BLOCK"] = str(self.K)

    def __exit__(self, *exc):
        if self.saved is None:
            os.environ.pop("RWKV_MI_LOOP_BLOCK", None)
        else:
            os.environ["RWKV_MI_LOOP_BLOCK"] = self.saved


class _Client:
    """Submits, cancels and polls, and keeps what a client would: the blocks counted at every submit and cancel, the tokens of every request as
    its events bring them -- each event must continue where the last one ended -- and its `finished` event, which must come once."""

    def __init__(self, sess):
        self.sess = sess
        self.tokens, self.end, self.arrive, self.cancel_at, self.events = {}, {}, {}, {}, 0

    def submit(self, rq):
        at = self.sess.stats()["blocks"]
        rid = self.sess.submit(**rq)
        assert rid == len(self.arrive), (rid, len(self.arrive))   # (ids count up from 0 in submit order)
        self.arrive[rid], self.tokens[rid] = at, []
        return rid

    def cancel(self, rid):
        at = self.sess.stats()["blocks"]
        ok = self.sess.cancel(rid)
        if ok:
            self.cancel_at.setdefault(rid, at)
        return ok

    def poll(self, **kw):
        events = self.sess.poll(**kw)
        for e in events:
            rid = e["id"]
            assert rid not in self.end, (rid, "an event after the request's end")
            assert e["first"] == len(self.tokens[rid]), (rid, e["first"], len(self.tokens[rid]))
            self.tokens[rid].extend(int(t) for t in e["tokens"])
            if e["finished"]:
                self.end[rid] = e
        self.events += len(events)
        return events

    def drain(self, **kw):
        """polls until a poll enqueues nothing and brings nothing: the session is not busy and everything read has been delivered"""
        for _ in range(100000):
            before = self.sess.stats()["blocks"]
            if not self.poll(drain=True, **kw) and self.sess.stats()["blocks"] == before:
                return
        raise AssertionError("the session does not come to rest")

    def check_rule(self, reqs, natural, n, K):
        """lane, start pass, and the length and reason of what was cancelled, against the protocol restated in Python"""
        ids = sorted(self.arrive)
        assert set(self.end) == set(ids), (sorted(self.end), ids)
        lane, start, lens, cancelled = session_rule([self.arrive[i] for i in ids], [self.cancel_at.get(i) for i in ids], [len(reqs[i]["prompt"]) for i in ids],
                                                    [natural[i] for i in ids], n, K)
        got = [(self.end[i]["lane"], self.end[i]["start_pass"], len(self.tokens[i]), self.end[i]["stopped_by"] == CANCELLED) for i in ids]
        assert got == list(zip(lane, start, lens, cancelled)), (got, list(zip(lane, start, lens, cancelled)))


def _work_end(c, reqs, ids):
    """the passes up to and including the last retirement of the requests `ids`, none of them cancelled: a request that starts at pass s
    runs its prompt but the last token, then one pass per token"""
    return max(c.end[i]["start_pass"] + len(reqs[i]["prompt"]) - 1 + len(c.tokens[i]) for i in ids)


def _open(b, family, **over):
    return b.serve_open(LANES, FAMILY_ID[family], **{**LIMITS, "features": _features(family), **over})


def _check_twin(client, rid, twin, where):
    _, toks, why = twin
    assert np.array_equal(client.tokens[rid], toks), (where, rid, client.tokens[rid], toks)
    assert client.end[rid]["stopped_by"] == why, (where, rid, client.end[rid]["stopped_by"], why)


# ---- 1. everything submitted before the first poll: the closed call ----

def _check_upfront(m, family, name):
    b1, b2 = _fresh(m, family), _fresh(m, family)
    reqs = _queue_with_stop(m, family, b1.state_store(PREFIX_SLOT))
    want = b1.serve(LANES, reqs, FAMILY_ID[family])
    sess = _open(b2, family)
    c = _Client(sess)
    for rq in reqs:
        c.submit(rq)
    assert sess.stats() == dict(passes=0, blocks=0, in_flight=R, room=0)   # (nothing is enqueued by open or by submit)
    c.drain()
    assert sess.stats()["in_flight"] == 0 and sess.stats()["room"] == R
    last = sess.close()
    for q in range(R):
        assert np.array_equal(c.tokens[q], want["tokens"][q]), (name, family, q, c.tokens[q], want["tokens"][q])
        e = c.end[q]
        assert (e["stopped_by"], e["lane"], e["start_pass"]) == (int(want["stopped_by"][q]), int(want["lane"][q]), int(want["start_pass"][q])), (name, family, q, e)
    assert last.tolist() == want["last_request"].tolist()
    for r, slot in enumerate(LANES):
        q = int(last[r])
        assert np.array_equal(b2.state_store(slot), b1.state_store(slot)), (name, family, r, "state")
        if family == "pen":
            decaying = reqs[q].get("decay", 1.0) != 1.0
            assert np.array_equal(_raw_counts(b2, slot, decaying), _raw_counts(b1, slot, decaying)), (name, family, r, "occurrence row")
        a = ([int(want["tokens"][q][-1])], 1.0, 1.0, -1.0, 77 + r)   # (parity and draw counter: one more generator draw)
        assert np.array_equal(b2.eval_sample([slot], *a), b1.eval_sample([slot], *a)), (name, family, r, "draw counter")
    for s in range(N_SLOTS):
        if s not in LANES:
            assert np.array_equal(b2.state_store(s), b1.state_store(s)), (name, family, s, "a slot that is no lane")
    b1.free()
    b2.free()


@pytest.mark.parametrize("family", FAMILIES)
def test_upfront_equals_serve_in_every_family(tmp_path, family):
    m = model(_synth(tmp_path, "test-v6", "Q5_1"))
    _check_upfront(m, family, "test-v6")
    m.free()


@pytest.mark.parametrize("name,fmt", [mf for mf in MODELS if mf[0] != "test-v6"])
def test_upfront_equals_serve_on_every_architecture(tmp_path, name, fmt):
    m = model(_synth(tmp_path, name, fmt))
    _check_upfront(m, "sample", name)
    m.free()


# ---- 7. vocabulary widths: the float4 and the word form of the admission copy ----

@pytest.mark.parametrize("name,fmt", [("mega-v6-2048-v64k", "Q4_0"), ("slice-v4-768", "Q8_0")])
def test_penalised_queue_on_real_vocabulary_widths(tmp_path, name, fmt):
    m = model(_synth(tmp_path, name, fmt))
    _check_upfront(m, "pen", name)
    m.free()


# ---- 2. arrivals and revival ----

@pytest.mark.parametrize("K", [1, 3, 16])
def test_arrivals_find_idle_lanes_and_every_request_is_its_twin(tmp_path, K):
    m = model(_synth(tmp_path, "test-v6", "Q5_1"))
    family = "sample"
    b = _fresh(m, family)
    prefix_state = b.state_store(PREFIX_SLOT)
    reqs = _queue_with_stop(m, family, prefix_state)
    twins = [_twin(m, family, rq, prefix_state) for rq in reqs]
    with _block(K):
        sess = _open(b, family)
    c = _Client(sess)
    for rq in reqs[:2]:      # (fewer requests than lanes: the closed call rejects that)
        c.submit(rq)
    c.poll()
    for rq in reqs[2:5]:
        c.submit(rq)
    c.drain()
    assert set(c.end) == set(range(5))
    at_rest = sess.stats()
    assert sess.poll() == [] and sess.poll(drain=True) == [] and sess.stats() == at_rest, (at_rest, sess.stats())
    # at most two blocks of dead passes lie behind the end of the work
    assert _work_end(c, reqs, range(5)) <= at_rest["passes"] <= _work_end(c, reqs, range(5)) + 2 * K, (at_rest, _work_end(c, reqs, range(5)))
    for rq in reqs[5:]:      # (every lane is idle by now: these are revivals)
        c.submit(rq)
    c.drain()
    assert _work_end(c, reqs, range(R)) <= sess.stats()["passes"] <= _work_end(c, reqs, range(R)) + 2 * K, (sess.stats(), _work_end(c, reqs, range(R)))
    last = sess.close()
    for q in range(R):
        _check_twin(c, q, twins[q], ("arrivals", K))
    c.check_rule(reqs, [len(t[1]) for t in twins], len(LANES), K)
    assert at_rest["passes"] == at_rest["blocks"] * K
    # after close each lane holds its last request's end: one more token gives the twin's logits (the parity is right)
    for r, slot in enumerate(LANES):
        q = int(last[r])
        assert q == max(i for i in range(R) if c.end[i]["lane"] == r), (r, q)
        tw, toks, _ = twins[q]
        assert np.array_equal(b.state_store(slot), tw.state_store(0)), (K, r, q, "state")
        assert np.array_equal(b.eval([slot], [int(toks[-1])]), tw.eval([0], [int(toks[-1])])), (K, r, q, "parity")
    for tw, _, _ in twins:
        tw.free()
    b.free()
    m.free()


@pytest.mark.parametrize("K", [1, 4])
def test_polling_without_drain_comes_to_rest_within_two_blocks_of_the_end(tmp_path, K):
    m = model(_synth(tmp_path, "test-v6", "Q5_1"))
    family = "sample"
    b = _fresh(m, family)
    prefix_state = b.state_store(PREFIX_SLOT)
    reqs = _queue_with_stop(m, family, prefix_state)
    twins = [_twin(m, family, rq, prefix_state) for rq in reqs]
    with _block(K):
        sess = _open(b, family)
    c = _Client(sess)
    for rq in reqs:
        c.submit(rq)
    for polls in range(1, 10000):
        before = sess.stats()["blocks"]
        events = c.poll()                 # (never RWKV_MI_POLL_DRAIN: a server's loop)
        if sess.stats()["blocks"] == before and not events:
            break
    assert set(c.end) == set(range(R)), sorted(c.end)
    at_rest = sess.stats()
    end = _work_end(c, reqs, range(R))
    assert end <= at_rest["passes"] <= end + 2 * K and at_rest["passes"] == at_rest["blocks"] * K, (at_rest, end, polls)
    assert at_rest["in_flight"] == 0 and at_rest["room"] == R
    for _ in range(3):
        assert sess.poll() == [] and sess.stats() == at_rest, (at_rest, sess.stats())
    for q in range(R):
        _check_twin(c, q, twins[q], ("no drain", K))
    # a submit wakes it, and it rests again
    rid = c.submit(reqs[0])
    for _ in range(10000):
        before = sess.stats()["blocks"]
        if not c.poll() and sess.stats()["blocks"] == before:
            break
    assert np.array_equal(c.tokens[rid], twins[0][1]) and c.end[rid]["start_pass"] == at_rest["passes"], (c.end[rid], at_rest)
    woke = sess.stats()
    end = c.end[rid]["start_pass"] + len(reqs[0]["prompt"]) - 1 + len(c.tokens[rid])
    assert end <= woke["passes"] <= end + 2 * K and sess.poll() == [] and sess.stats() == woke, (woke, end)
    sess.close()
    for tw, _, _ in twins:
        tw.free()
    b.free()
    m.free()


# ---- 3. the ring ----

def test_a_ring_of_four_serves_eleven_requests_and_a_full_ring_rejects(tmp_path, capfd):
    m = model(_synth(tmp_path, "test-v6", "Q5_1"))
    m._library.rwkv_set_print_errors(m._ctx, True)   # (the rejection's message is read below)
    family = "pen"
    b = _fresh(m, family)
    prefix_state = b.state_store(PREFIX_SLOT)
    reqs = _queue_with_stop(m, family, prefix_state)
    reqs += [dict(rq, seed=rq["seed"] + 100) for rq in reqs[:3]]
    twins = [_twin(m, family, rq, prefix_state) for rq in reqs]
    with _block(3):
        sess = _open(b, family, capacity=4)
    c = _Client(sess)
    todo = list(reqs)
    full_seen = 0
    taken_at = {}   # id -> the ids whose end had been delivered when the ring took it
    for _ in range(1000):
        while todo and sess.stats()["room"] > 0:
            rid = c.submit(todo.pop(0))
            taken_at[rid] = set(c.end)
        # what the ring says about itself is what a ring of four says: id q waits for the end of id q - 4 to have been delivered, so the
        # room is four less the ids from the oldest undelivered one on
        st = sess.stats()
        issued = len(c.arrive)
        oldest = min((i for i in range(issued) if i not in c.end), default=issued)
        assert st["room"] == 4 - (issued - oldest) and st["in_flight"] == issued - len(c.end) <= 4, (st, issued, oldest, sorted(c.end))
        if todo and st["room"] == 0:
            capfd.readouterr()
            with pytest.raises(ValueError):
                sess.submit(**todo[0])
            assert "full" in capfd.readouterr().err
            assert b.last_error & ARGS and sess.stats() == st, (b.last_error, st, sess.stats())
            full_seen += 1
        c.poll(drain=True)
        if not todo and len(c.end) == len(reqs):
            break
    assert full_seen >= 1 and len(c.end) == 11
    # every entry has been used at least twice, and never by two requests at once: id q was taken only after id q - 4 had been delivered
    assert sorted(taken_at) == list(range(11)) and all(q - 4 in taken_at[q] for q in range(4, 11)), taken_at
    for q in range(11):
        _check_twin(c, q, twins[q], "ring")
    c.check_rule(reqs, [len(t[1]) for t in twins], len(LANES), 3)
    sess.close()
    for tw, _, _ in twins:
        tw.free()
    b.free()
    m.free()


# ---- 4. cancel ----

def test_cancel_in_the_prompt_in_decode_and_in_the_queue(tmp_path):
    m = model(_synth(tmp_path, "test-v6", "Q5_1"))
    family, K = "sample", 3
    b = _fresh(m, family)
    prefix_state = b.state_store(PREFIX_SLOT)
    reqs = _requests(m.n_vocab)
    twins = [_twin(m, family, rq, prefix_state) for rq in reqs]
    natural = [len(t[1]) for t in twins]
    with _block(K):
        sess = _open(b, family)
    c = _Client(sess)
    for rq in reqs:
        c.submit(rq)
    assert c.cancel(7)                      # queued: it waits behind the others
    assert not c.cancel(R) and not c.cancel(NO_TOKEN)   # never issued
    c.poll()                                # block 0: passes 0 .. 2
    # request 2 (two prompt tokens, on lane 2 from pass 0) draws from pass 1 on; request 3 (five prompt tokens) starts at pass 2, when
    # requests 0 and 1 have spent their budget of two: both cancels arrive with block 1, whose first pass is pass 3
    assert c.cancel(2) and c.cancel(3)
    assert c.cancel(2)                      # (again, while in flight: true, and nothing more happens)
    c.drain()
    assert 0 in c.end and not c.cancel(0)   # its end has been delivered
    c.check_rule(reqs, natural, len(LANES), K)
    for q in (2, 3, 7):
        assert c.end[q]["stopped_by"] == CANCELLED, (q, c.end[q])
        assert c.tokens[q] == [int(t) for t in twins[q][1][: len(c.tokens[q])]], (q, "a prefix of the twin's tokens")
    assert len(c.tokens[3]) == 0 and len(c.tokens[7]) == 0 and 0 < len(c.tokens[2]) < natural[2], [len(c.tokens[q]) for q in (2, 3, 7)]
    for q in (0, 1, 4, 5, 6):
        _check_twin(c, q, twins[q], "beside a cancel")
    # the lane request 3 gave up serves the next request from the pass after its retirement
    after = [q for q in range(R) if c.end[q]["lane"] == c.end[3]["lane"] and c.end[q]["start_pass"] > c.end[3]["start_pass"]]
    assert after and min(c.end[q]["start_pass"] for q in after) == c.end[3]['start_pass'] + 2, (after, [c.end[q] for q in after])
    sess.close()
    for tw, _, _ in twins:
        tw.free()
    b.free()
    m.free()


# ---- 5. streaming ----

def test_events_stream_the_tokens_once_each(tmp_path):
    m = model(_synth(tmp_path, "test-v6", "Q5_1"))
    family = "sample"
    b = _fresh(m, family)
    prefix_state = b.state_store(PREFIX_SLOT)
    reqs = _queue_with_stop(m, family, prefix_state)
    twins = [_twin(m, family, rq, prefix_state) for rq in reqs]
    with _block(2):
        sess = _open(b, family)
    c = _Client(sess)
    for rq in reqs:
        c.submit(rq)
    for _ in range(1000):
        events = c.poll(max_events=1, max_tokens=2)
        assert len(events) <= 1 and sum(len(e["tokens"]) for e in events) <= 2
        if len(c.end) == R:
            break
    for q in range(R):
        _check_twin(c, q, twins[q], "streamed")     # (the client has checked every `first`: nothing lost, nothing twice)
    assert c.events > R, (c.events, "a request's tokens arrive in more than one event")
    assert sess.poll(drain=True) == []
    sess.close()
    for tw, _, _ in twins:
        tw.free()
    b.free()
    m.free()


# ---- 6. guides and bias per request ----

@pytest.mark.parametrize("family", ["sample", "pen"])
def test_guides_and_bias_come_with_requests(tmp_path, family):
    m = model(_synth(tmp_path, "test-v6", "Q5_1"))
    V = m.n_vocab
    guides, biases = X._guides(V), X._biases(V)
    # the sampled family hands lanes over guided -> unguided -> guided; the penalised one biased -> unbiased, without guides
    extras = X.EXTRAS if family == "sample" else [(None, None, bs) for _, _, bs in X.EXTRAS]
    reqs = X._queue(V, family, extras=extras)
    b = X._fresh(m, family, guides, biases)
    prefix_state = b.state_store(X.PREFIX_SLOT)
    features = pkg.SERVE_GUIDED if family == "sample" else pkg.SERVE_REP | pkg.SERVE_CUT
    with _block(3):
        sess = b.serve_open(X.LANES, FAMILY_ID[family], capacity=len(reqs), max_prompt=max(X.PROMPT_LENS), stride=max(X.BUDGETS), max_seqs=0, max_seq_tokens=0,
                            features=features)
    c = _Client(sess)
    for rq in reqs[:4]:
        c.submit(rq)
    c.poll()
    for rq in reqs[4:]:
        c.submit(rq)
    # a request that needs what the session did not declare: a guide in the penalised session, which declared none
    if family == "pen":
        before = sess.stats()
        with pytest.raises(ValueError):
            sess.submit(**dict(reqs[0], guide=0, guide_state=0))
        assert b.last_error & ARGS and sess.stats() == before
    c.drain()
    has = [(rq.get("guide") is not None, rq.get("bias_slot") is not None) for rq in reqs]
    for q, rq in enumerate(reqs):
        tw = X._twin(m, family, rq, prefix_state, guides, biases, None)
        assert np.array_equal(c.tokens[q], tw["tokens"]) and c.end[q]["stopped_by"] == tw["why"], (family, q, c.tokens[q], tw["tokens"])
        assert (c.end[q]["guide_state"], c.end[q]["guide_misses"]) == (tw["guide_state"], tw["guide_misses"]), (family, q, c.end[q], tw)
    # the hand-overs the case is about did happen on some lane
    pairs = set()
    for r in range(len(X.LANES)):
        mine = sorted((c.end[q]["start_pass"], q) for q in range(len(reqs)) if c.end[q]["lane"] == r)
        pairs |= {(has[a], has[bq]) for (_, a), (_, bq) in zip(mine, mine[1:])}
    k = 0 if family == "sample" else 1
    assert any(a[k] and not bq[k] for a, bq in pairs) and any(not a[k] and bq[k] for a, bq in pairs), pairs
    sess.close()
    b.free()
    m.free()


def test_a_session_without_features_rejects_a_truncating_request(tmp_path):
    m = model(_synth(tmp_path, "test-v6", "Q5_1"))
    b = _fresh(m, "sample")
    reqs = _requests(m.n_vocab)
    sess = _open(b, "sample", features=0)
    with pytest.raises(ValueError):
        sess.submit(**reqs[2])            # top_k 5
    assert b.last_error & ARGS and sess.stats()["in_flight"] == 0
    assert sess.submit(**reqs[0]) == 0    # (a request with no setting is taken, and gets the first id)
    sess.close()
    b.free()
    m.free()


# ---- 8. rejections change nothing ----

def test_rejections_change_nothing(tmp_path):
    m = model(_synth(tmp_path, "test-v6", "Q5_1"))
    V = m.n_vocab
    family = "pen"
    b = _fresh(m, family)
    prefix_state = b.state_store(PREFIX_SLOT)
    reqs = _queue_with_stop(m, family, prefix_state)
    twins = [_twin(m, family, rq, prefix_state) for rq in reqs]
    before = [b.state_store(s) for s in range(N_SLOTS)]

    def no_open(what, lanes=LANES, fam=2, **over):
        with pytest.raises(ValueError):
            b.serve_open(lanes, fam, **{**LIMITS, "features": _features(family), **over})
        assert b.last_error & ARGS, (what, b.last_error)

    no_open("n == 0", lanes=[])
    no_open("a lane out of range", lanes=[4, 0, N_SLOTS])
    no_open("a lane twice", lanes=[4, 0, 4])
    no_open("an unknown family", fam=3)
    no_open("capacity 0", capacity=0)
    no_open("stride 0", stride=0)
    no_open("max_prompt 0", max_prompt=0)
    no_open("too many sequences", max_seqs=17)
    no_open("unknown feature bits", features=8)
    no_open("guides in the greedy family", fam=0, features=pkg.SERVE_GUIDED)
    with pytest.raises(ValueError):
        pkg.ServeSession(b, LANES, 2, pkg.ServeLimits(R, 5, 9, 2, 5, 0, 1))
    assert b.last_error & ARGS, "reserved != 0"
    b.set_logit_bias(LANES[0], {3: 2.0})
    no_open("a lane with a bias set")
    b.set_logit_bias(LANES[0], {})
    g = b.create_guide([{t: 0 for t in range(8)}])
    b.attach_guide(LANES[2], g, 0)
    no_open("a lane with a guide attached")
    b.detach_guide(LANES[2])
    b.free_guide(g)
    b.set_logprobs(2)
    no_open("a batch with the report on")
    b.set_logprobs(0, enabled=False)

    sess = _open(b, family)
    c = _Client(sess)
    no_open("a second session")

    def no_submit(what, **change):
        at = sess.stats()
        with pytest.raises(ValueError):
            sess.submit(**{**reqs[1], **change})
        assert b.last_error & ARGS and sess.stats() == at, (what, b.last_error)

    no_submit("a prompt over max_prompt", prompt=[1] * 6)
    no_submit("max_tokens over stride", max_tokens=10)
    no_submit("too many sequences", stop=[[1], [2], [3]])
    no_submit("too many sequence tokens", stop=[[1, 2, 3], [4, 5, 6]])
    no_submit("a from_slot that is a lane", from_slot=LANES[1])
    no_submit("a from_slot out of range", from_slot=N_SLOTS)
    no_submit("a prompt token out of range", prompt=[1, V])
    no_submit("max_tokens 0", max_tokens=0)
    no_submit("a top_p above 1", top_p=1.5)
    no_submit("repetition 0", repetition=0.0)
    no_submit("a bias_slot without a bias", bias_slot=1)
    for rq in reqs[:4]:
        c.submit(rq)
    c.poll()

    def no_call(what, f):
        with pytest.raises(ValueError):
            f()
        assert b.last_error & ARGS, (what, b.last_error)

    no_call("eval", lambda: b.eval([1], [3]))
    no_call("decode_until", lambda: b.decode_until([1], [3], 2))
    no_call("serve", lambda: b.serve(LANES, reqs, 2))
    no_call("set_logprobs", lambda: b.set_logprobs(2))
    # what runs no pass stays legal on a slot that is no lane
    assert np.array_equal(b.state_store(1), before[1])
    b.set_logit_bias(3, {5: 1.0})
    b.set_logit_bias(3, {})
    for rq in reqs[4:]:
        c.submit(rq)
    c.drain()
    for q in range(R):
        _check_twin(c, q, twins[q], "after the rejections")   # (the session still yields its twins)
    sess.close()
    for s in range(N_SLOTS):
        if s not in LANES:
            assert np.array_equal(b.state_store(s), before[s]), s
    for tw, _, _ in twins:
        tw.free()
    b.free()
    m.free()


# ---- 9. close with work in flight ----

def test_close_with_work_in_flight_hands_the_batch_back(tmp_path):
    m = model(_synth(tmp_path, "test-v6", "Q5_1"))
    family = "sample"
    b = _fresh(m, family)
    prefix_state = b.state_store(PREFIX_SLOT)
    reqs = _queue_with_stop(m, family, prefix_state)
    twins = [_twin(m, family, rq, prefix_state) for rq in reqs]
    with _block(2), b.serve_open(LANES, FAMILY_ID[family], **{**LIMITS, "features": _features(family)}) as sess:
        c = _Client(sess)
        for rq in reqs:
            c.submit(rq)
        c.poll()
        c.poll()
        c.poll()
        assert sess.stats()["in_flight"] > 0
    assert sess.last_request is not None and not sess._ptr
    # what had been delivered by then is consistent: prefixes of the twins, whole where an end came
    for q in range(R):
        toks = [int(t) for t in twins[q][1]]
        assert c.tokens[q] == toks[: len(c.tokens[q])], (q, c.tokens[q], toks)
        if q in c.end:
            assert c.tokens[q] == toks and c.end[q]["stopped_by"] == twins[q][2], (q, c.end[q])
    # the batch is usable as before: the closed call on the same queue gives the twins, and a pass runs
    got = b.serve(LANES, reqs, FAMILY_ID[family])
    for q in range(R):
        assert np.array_equal(got["tokens"][q], twins[q][1]) and int(got["stopped_by"][q]) == twins[q][2], q
    tw = twins[int(got["last_request"][0])]
    assert np.array_equal(b.eval([LANES[0]], [int(tw[1][-1])]), tw[0].eval([0], [int(tw[1][-1])]))
    for t, _, _ in twins:
        t.free()
    b.free()
    m.free()
