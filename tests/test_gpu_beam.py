"""Beam search in the batch (rwkv_mi_batch_decode_beam, csrc/score.hip k_beam_rows / k_beam_select) and the slot-to-slot copy
(rwkv_mi_batch_state_copy).

Everything is held exactly. The selection of a step against tests/beam_ref.py working from the per-row lists the report kernel gives on the same
logits (rwkv_test_logprob_rows at top_n = W: the two kernels share one body, so the lists are the same bits): tokens, parents, finished words
and float32 log-probs array_equal, the float64 scores bit-equal. The whole call against a search the HOST drives with existing calls only --
eval with the logits to the host, the same lists through the hook, beam_ref, the states permuted with state_store / state_load. W = 1 against
the greedy loop. The log-probs a step chooses also stay within the ONE tolerance of tests/test_gpu_score.py (check_logprob) of NumPy float64."""
import ctypes

import numpy as np
import pytest

import beam_ref
import reference_constants as R
from beam_ref import NO_TOKEN
from gpu_lib import model, pkg
from logprobs_ref import f64_logprobs
from test_gpu_logprobs import check_against_f64, logprob_rows
from test_gpu_score import _crafted, _hooks

pytestmark = pytest.mark.gpu

ARGS = 1 << 8   # RWKV_ERROR_ARGS
P_UINT32 = ctypes.POINTER(ctypes.c_uint32)
P_FLOAT = ctypes.POINTER(ctypes.c_float)
P_DOUBLE = ctypes.POINTER(ctypes.c_double)
GOLDEN = [(v, "Q5_1") for v in R.VERSIONS] + [(v, "FP16") for v in R.HAVE_FP32_FP16]
FIRST = (34, 105, 110)


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- 1. the two kernels of a step on crafted logits, through the hook ----

def beam_step(logits, scores, finished, W, ends):
    """k_beam_rows + k_beam_select through the test hook on logits [G * W][V]: tokens, parents, log-probs, scores, finished words [G * W]."""
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    rows, V = logits.shape
    sc = np.ascontiguousarray(scores, dtype=np.float64)
    fin = np.ascontiguousarray(finished, dtype=np.uint32)
    e = np.ascontiguousarray(ends, dtype=np.uint32)
    tok = np.full(rows, 0xDEAD, dtype=np.uint32)
    par = np.full(rows, 0xDEAD, dtype=np.uint32)
    lp = np.full(rows, np.nan, dtype=np.float32)
    so = np.full(rows, np.nan, dtype=np.float64)
    fo = np.full(rows, 0xDEAD, dtype=np.uint32)
    ok = _hooks().rwkv_test_beam_step(logits.ctypes.data_as(P_FLOAT), rows // W, V, sc.ctypes.data_as(P_DOUBLE), fin.ctypes.data_as(P_UINT32), W,
                                      e.ctypes.data_as(P_UINT32) if e.size else None, e.size, tok.ctypes.data_as(P_UINT32), par.ctypes.data_as(P_UINT32),
                                      lp.ctypes.data_as(P_FLOAT), so.ctypes.data_as(P_DOUBLE), fo.ctypes.data_as(P_UINT32))
    assert ok, "rwkv_test_beam_step failed"
    return tok, par, lp, so, fo


_pools = {}


def _pool(V):
    """test_gpu_score.py's crafted rows (model-like / wide / narrow spreads, V equal logits, a dominant logit, +-1e4, exact ties) and the rows the
    beam needs: all NaN, a tenth -inf, all but three -inf"""
    if V not in _pools:
        rng = np.random.default_rng(77 + V)
        rows = list(_crafted(V, 991 + V)[0])
        ninf = rng.standard_normal(V).astype(np.float32)
        ninf[rng.random(V) < 0.1] = -np.inf
        few = np.full(V, -np.inf, dtype=np.float32)
        few[rng.choice(V, size=3, replace=False)] = (0.5, -1.5, 0.5)
        _pools[V] = {"rows": np.stack(rows), "nan": np.full(V, np.nan, dtype=np.float32), "ninf": ninf, "few": few, "equal": rows[6]}
    return _pools[V]


def _groups(V, W, seed):
    """the groups of the file: (name, rows [W][V], scores [W], finished [W])"""
    p = _pool(V)
    rng = np.random.default_rng(seed)
    pool = p["rows"]

    def pick(k):
        return np.stack([pool[(k + 3 * j) % len(pool)] for j in range(W)])
    live = np.zeros(W, dtype=np.uint32)
    start = np.full(W, -np.inf)
    start[0] = 0.0
    out = [("step 0", pick(0), start, live)]                                                     # must yield row 0's W candidates in rank order
    out.append(("identical rows, identical scores", np.stack([pool[1]] * W), np.full(W, -1.5), live))   # the parent decides every tie
    out.append(("equal logits inside the rows", np.stack([p["equal"]] * W), np.full(W, -0.25), live))   # W * W equal candidates: parent 0's, by rank
    out.append(("equal logits beside ties", np.stack([p["equal"], pool[12]] * W)[:W], np.full(W, -0.25), live))
    mixed = pick(2)
    mixed[W // 2] = p["nan"]                                                                     # a row of all NaN offers nothing
    mixed[W - 1] = p["ninf"]
    mixed[0] = p["few"]                                                                          # three candidates, then -inf log-probs: not offered
    out.append(("NaN, -inf and random scores", mixed, -rng.random(W) * 8.0, live))
    out.append(("all NaN", np.stack([p["nan"]] * W), np.full(W, -2.0), live))                    # every hypothesis dead
    out.append(("all finished", pick(4), -np.arange(W, dtype=np.float64) - 0.5, np.ones(W, dtype=np.uint32)))   # unchanged
    fin_last = live.copy()
    fin_last[W - 1] = 1
    wins = -rng.random(W) * 4.0 - 1.0
    wins[W - 1] = 0.0                                                                            # a finished hypothesis above every live candidate ...
    out.append(("a finished hypothesis wins", pick(5), wins, fin_last))
    loses = wins.copy()
    loses[W - 1] = -1e9                                                                          # ... and one below all of them
    out.append(("a finished hypothesis loses", pick(6), loses, fin_last))
    return out


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("W", [1, 2, 5, 20])
@pytest.mark.parametrize("V", [1000, 50277, 65536])
def test_a_step_through_the_hook(V, W, G):
    groups = _groups(V, W, 5 * V + W)
    while len(groups) % G:
        groups.append(groups[len(groups) % 3])
    for c0 in range(0, len(groups), G):
        chunk = groups[c0:c0 + G]
        logits = np.concatenate([g[1] for g in chunk])
        scores = np.concatenate([g[2] for g in chunk])
        finished = np.concatenate([g[3] for g in chunk])
        # the per-row lists: the report kernel on the same logits
        _, ids, lps = logprob_rows(logits, np.zeros(G * W, dtype=np.int64), W)
        # end tokens that do finish something: the best token of the chunk's first row and the second best of its last
        ends = sorted({int(t) for t in (ids[0, 0], ids[-1, min(1, W - 1)]) if int(t) != NO_TOKEN})
        tok, par, lp, sc, fin = beam_step(logits, scores, finished, W, ends)
        for g, (name, rows, s_in, f_in) in enumerate(chunk):
            at = slice(g * W, (g + 1) * W)
            what = (V, W, G, name)
            wt, wp, wl, ws, wf, _ = beam_ref.step(ids[at], lps[at], s_in, f_in, np.zeros(W, dtype=np.uint32), ends)
            assert np.array_equal(tok[at], wt), (what, tok[at].tolist(), wt.tolist())
            assert np.array_equal(par[at], wp), (what, par[at].tolist(), wp.tolist())
            assert np.array_equal(fin[at], wf), (what, fin[at].tolist(), wf.tolist())
            assert np.array_equal(bits32(lp[at]), bits32(wl)), what
            assert np.array_equal(bits64(sc[at]), bits64(ws)), (what, sc[at].tolist(), ws.tolist())
            # the chosen log-probs against NumPy float64 on the parent's row
            for j in range(W):
                if int(tok[at][j]) != NO_TOKEN:
                    ref = f64_logprobs(rows[int(par[at][j])], [int(tok[at][j])])[0]
                    check_against_f64(lp[at][j], ref, (what, j))
            # what the issue states of the named groups, apart from the reference
            if name == "step 0":
                n = int((ids[g * W] != NO_TOKEN).sum())
                assert np.array_equal(tok[at], ids[g * W]) and np.all(par[at][:n] == 0) and np.array_equal(bits32(lp[at][:n]), bits32(lps[g * W][:n])), what
            if name == "equal logits inside the rows":
                assert np.all(par[at] == 0) and np.array_equal(tok[at], np.arange(W)), what
            if name == "all finished":
                assert np.all(tok[at] == NO_TOKEN) and np.array_equal(par[at], np.arange(W)) and np.array_equal(bits64(sc[at]), bits64(s_in)) and np.all(fin[at] == 1), what
            if name == "all NaN":
                assert np.all(tok[at] == NO_TOKEN) and np.all(np.isneginf(sc[at])) and np.all(fin[at] == 1) and np.array_equal(par[at], np.arange(W)), what
            if name == "a finished hypothesis wins":
                assert int(par[at][0]) == W - 1 and int(tok[at][0]) == NO_TOKEN and sc[at][0] == 0.0 and fin[at][0] == 1, what
            if name == "a finished hypothesis loses" and W > 1:
                assert not np.any((par[at] == W - 1) & (tok[at] == NO_TOKEN)), what
            if name == "identical rows, identical scores" and W > 1 and lps[g * W, 0] > lps[g * W, 1]:
                # W equal best candidates, one per parent, above everything else: the parents in ascending order, the same token each
                assert np.array_equal(par[at], np.arange(W)) and np.all(tok[at] == ids[g * W, 0]) and np.all(sc[at] == sc[at][0]), what


# ---- the host-driven search: existing calls only ----

def host_search(tw, slots, first, W, n_tokens, ends):
    """The search of G groups on the batch `tw`, driven from the host: eval, the report kernel's lists through the hook, beam_ref, the states
    permuted through the host. slots: [G][W]. Returns what decode_beam returns (without the time) and the finished words [G][W]."""
    slots = np.asarray(slots)
    G = slots.shape[0]
    flat = slots.reshape(-1).tolist()
    for g in range(G):
        s0 = tw.state_store(int(slots[g, 0]))
        for j in range(1, W):
            tw.state_load(int(slots[g, j]), s0)
    words = [beam_ref.start(W) for _ in range(G)]
    fed = np.repeat(np.asarray(first, dtype=np.uint32), W)
    hist = [([], [], []) for _ in range(G)]
    for _ in range(n_tokens):
        logits = tw.eval(flat, fed.tolist())
        _, ids, lps = logprob_rows(logits, np.zeros(G * W, dtype=np.int64), W)
        states = [tw.state_store(s) for s in flat]
        for g in range(G):
            at = slice(g * W, (g + 1) * W)
            tok, par, lp, sc, fin, ln = beam_ref.step(ids[at], lps[at], *words[g], ends)
            words[g] = (sc, fin, ln)
            fed[at] = np.where(tok != NO_TOKEN, tok, fed[at][par])
            for h, x in zip(hist[g], (tok, par, lp)):
                h.append(x)
            for j in range(W):
                if int(par[j]) != j:
                    tw.state_load(flat[g * W + j], states[g * W + int(par[j])])
        if all(w[1].all() for w in words):
            break
    out = [beam_ref.backtrace(*hist[g], words[g][0], n_tokens) for g in range(G)]
    for g in range(G):
        assert np.array_equal(out[g][1], words[g][2])
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([w[0] for w in words]), np.stack([o[2] for o in out]),
            np.stack([w[1] for w in words]))


def _prompted(m, n_slots, prompt_slots, seed=1):
    """a batch whose prompt slots have read a few tokens of their own (so the groups start from different states)"""
    b = pkg.RWKVBatch(m, n_slots)
    rng = np.random.default_rng(seed)
    for _ in range(3):
        b.eval(prompt_slots, rng.integers(0, m.n_vocab, size=len(prompt_slots)).tolist())
    return b


def _check_against_the_host(m, G, W, n_tokens, ends, first, what):
    slots = np.arange(G * W).reshape(G, W)
    b = _prompted(m, G * W, slots[:, 0].tolist())
    tw = _prompted(m, G * W, slots[:, 0].tolist())
    tokens, lens, scores, lps, _ = b.decode_beam(slots, first, W, n_tokens, ends)
    wt, wl, ws, wlp, wfin = host_search(tw, slots, first, W, n_tokens, ends)
    assert np.array_equal(tokens, wt), (what, tokens.tolist(), wt.tolist())
    assert np.array_equal(lens, wl), (what, lens.tolist(), wl.tolist())
    assert np.array_equal(bits32(lps), bits32(wlp)), what
    assert np.array_equal(bits64(scores), bits64(ws)), (what, scores.tolist(), ws.tolist())
    assert b.last_loop_passes() >= int(lens.max()) and np.all(lens <= n_tokens), what
    # every unfinished hypothesis: its slot holds the state the host's search holds, and goes on from it (the parity is right)
    open_rows = [(g, j) for g in range(G) for j in range(W) if not wfin[g, j]]
    for g, j in open_rows:
        assert np.array_equal(b.state_store(int(slots[g, j])), tw.state_store(int(slots[g, j]))), (what, "state", g, j)
    if open_rows:
        sl = [int(slots[g, j]) for g, j in open_rows]
        last = [int(tokens[g, j, lens[g, j] - 1]) for g, j in open_rows]
        assert np.array_equal(b.eval(sl, last), tw.eval(sl, last)), (what, "the next pass")
    b.free(); tw.free()
    return tokens, lens, wfin


def _greedy_token(m, G, W, first, step):
    """the token the greedy run of group 0 emits at `step`, from the same prompted state"""
    slots = np.arange(G * W).reshape(G, W)
    g = _prompted(m, G * W, slots[:, 0].tolist())
    toks, _ = g.decode_greedy(slots[:, 0].tolist(), list(first), step + 1)
    g.free()
    return int(toks[0, step])


# ---- 2. W = 1 is the greedy loop ----

@pytest.mark.parametrize("n_tokens", [8, 9])
@pytest.mark.parametrize("version,fmt", GOLDEN)
def test_width_one_is_the_greedy_loop(golden_dir, version, fmt, n_tokens):
    m = model(R.fixture_path(golden_dir, version, fmt))
    b, tw = _prompted(m, 3, [0, 1, 2]), _prompted(m, 3, [0, 1, 2])
    tokens, lens, scores, lps, _ = b.decode_beam([[0], [1], [2]], FIRST, 1, n_tokens)
    greedy, _ = tw.decode_greedy([0, 1, 2], FIRST, n_tokens)
    assert np.array_equal(tokens[:, 0, :], greedy), (version, fmt)
    assert np.all(lens == n_tokens) and b.last_loop_passes() == n_tokens
    for s in range(3):
        assert np.array_equal(b.state_store(s), tw.state_store(s)), (version, fmt, s)
    assert np.array_equal(b.eval([0, 1, 2], greedy[:, -1].tolist()), tw.eval([0, 1, 2], greedy[:, -1].tolist()))
    # the score is the sum of the step's log-probs, added in order as doubles
    for g in range(3):
        acc = np.float64(0.0)
        for x in lps[g, 0]:
            acc = acc + np.float64(x)
        assert bits64(scores[g, 0]) == bits64(acc)
    b.free(); tw.free(); m.free()


# ---- 3. the whole call against the host-driven search ----

@pytest.mark.parametrize("version,fmt", GOLDEN)
def test_the_call_is_the_host_driven_search(golden_dir, version, fmt):
    m = model(R.fixture_path(golden_dir, version, fmt))
    first = FIRST[:2]
    end = _greedy_token(m, 2, 3, first, 3)
    finished_somewhere = False
    for n_tokens, ends in ((9, [end]), (8, [end]), (9, [])):
        _, _, fin = _check_against_the_host(m, 2, 3, n_tokens, ends, first, (version, fmt, n_tokens, ends))
        finished_somewhere |= bool(ends) and bool(fin.any())
    assert finished_somewhere, (version, fmt, "no hypothesis reached the end token")
    m.free()


# ---- 4. 33 rows: the pass takes the matrix-core products ----

def test_thirty_three_rows(golden_dir):
    m = model(R.fixture_path(golden_dir, "6v0-3m", "Q5_1"))
    first = [(7 * g + 3) % m.n_vocab for g in range(11)]
    _check_against_the_host(m, 11, 3, 3, [], first, "33 rows")
    m.free()


# ---- 5. the best hypothesis' log-probs are score_ragged's ----

@pytest.mark.parametrize("version,fmt", [("6v0-3m", "Q5_1"), ("7v0-834K", "FP16")])
def test_logprobs_are_what_score_ragged_scores(golden_dir, version, fmt):
    m = model(R.fixture_path(golden_dir, version, fmt))
    slots = np.arange(6).reshape(2, 3)
    b, sc = _prompted(m, 6, [0, 3]), _prompted(m, 6, [0, 3])
    tokens, lens, scores, lps, _ = b.decode_beam(slots, FIRST[:2], 3, 7)
    for g in range(2):
        text = tokens[g, 0, :lens[g, 0]].tolist()
        assert len(text) == 7
        want, _ = sc.score_ragged([int(slots[g, 0])], [[FIRST[g]] + text[:-1]], [text])
        assert np.array_equal(bits32(lps[g, 0, :len(text)]), bits32(want[0])), (version, fmt, g)
    b.free(); sc.free(); m.free()


# ---- 6. neighbours ----

def test_neighbours_are_untouched_and_the_report_changes_nothing(golden_dir):
    m = model(R.fixture_path(golden_dir, "6v0-3m", "Q5_1"))
    slots = np.arange(4).reshape(2, 2)

    def prepared():
        x = _prompted(m, 5, [0, 2, 4])
        for s in range(5):
            x.rng_seek(s, 10 + s)
        x.counts_add(1, [3, 3, 9]); x.counts_add(4, [5])
        return x
    b, rep, tw = prepared(), prepared(), prepared()
    idle = b.state_store(4)
    out = b.decode_beam(slots, FIRST[:2], 2, 6)
    assert np.array_equal(b.state_store(4), idle)
    for s in range(5):
        assert np.array_equal(b.counts(s), tw.counts(s)), s
    # the report on: the same tokens, lengths, scores, log-probs and states
    rep.set_logprobs(5)
    out2 = rep.decode_beam(slots, FIRST[:2], 2, 6)
    for x, y in zip(out[:4], out2[:4]):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
    for s in range(5):
        assert np.array_equal(b.state_store(s), rep.state_store(s)), s
    rep.set_logprobs(enabled=False)
    # the draw counters: from equal states, one generator draw per slot is the twin's
    for x in (b, rep, tw):
        for s in range(5):
            x.state_load(s, idle)
    draws = [x.eval_sample(list(range(5)), [1, 2, 3, 4, 5], 1.0, 1.0, -1.0, [11, 22, 33, 44, 55]) for x in (b, rep, tw)]
    assert np.array_equal(draws[0], draws[2]) and np.array_equal(draws[1], draws[2])
    b.free(); rep.free(); tw.free(); m.free()


# ---- 7. rwkv_mi_batch_state_copy ----

def test_state_copy(golden_dir):
    m = model(R.fixture_path(golden_dir, "6v0-3m", "Q5_1"))

    def prepared():
        x = _prompted(m, 3, [0])          # slot 0 after three passes: its parity differs from slot 1's
        x.counts_add(0, [3, 3, 9]); x.rng_seek(0, 7); x.set_logit_bias(0, {5: 4.0})
        return x
    for counter, counts, bias in ((False, False, False), (True, False, False), (False, True, False), (False, False, True), (True, True, True)):
        b, tw = prepared(), prepared()
        b.copy_state(1, 0, counter=counter, counts=counts, bias=bias)
        assert np.array_equal(b.state_store(1), b.state_store(0)) and np.array_equal(b.state_store(0), tw.state_store(0))
        # the twin gets by hand exactly what was asked for
        tw.state_load(1, tw.state_store(0))
        if counter:
            tw.rng_seek(1, 7)
        if counts:
            tw.counts_add(1, [3, 3, 9])
        if bias:
            tw.set_logit_bias(1, {5: 4.0})
        what = (counter, counts, bias)
        assert np.array_equal(b.counts(1), tw.counts(1)) and np.array_equal(b.counts(2), tw.counts(2)), what
        t1, _ = b.decode_sample_penalized([0, 1, 2], [9, 9, 9], 8, 1.0, 1.0, 5, 0.5, 0.5)
        t2, _ = tw.decode_sample_penalized([0, 1, 2], [9, 9, 9], 8, 1.0, 1.0, 5, 0.5, 0.5)
        assert np.array_equal(t1, t2), what
        if counter and counts and bias:
            assert np.array_equal(t1[0], t1[1]), "the copy and the original continue identically"
            assert np.array_equal(b.state_store(0), b.state_store(1))
        b.free(); tw.free()
    # dst == src does nothing
    b, tw = prepared(), prepared()
    b.copy_state(0, 0, counter=True, counts=True, bias=True)
    assert np.array_equal(b.state_store(0), tw.state_store(0)) and np.array_equal(b.counts(0), tw.counts(0))
    assert np.array_equal(b.eval([0, 1], [4, 4]), tw.eval([0, 1], [4, 4]))
    b.free(); tw.free(); m.free()


# ---- 8. rejections ----

def test_rejections_change_nothing(golden_dir):
    m = model(R.fixture_path(golden_dir, "6v0-3m", "Q5_1"))
    lib = m._library
    L = lib.library
    V = m.n_vocab
    b, tw = _prompted(m, 4, [0, 1, 2, 3]), _prompted(m, 4, [0, 1, 2, 3])
    lib.rwkv_set_print_errors(m._ctx, False)

    def beam(slots, first, G, W, n_tokens, ends, n_end=None):
        s = np.asarray(slots, dtype=np.uint32); f = np.asarray(first, dtype=np.uint32); e = np.asarray(ends, dtype=np.uint32)
        p = pkg.BeamParams(W, len(ends) if n_end is None else n_end, e.ctypes.data_as(P_UINT32) if e.size else None)
        tok = np.empty(max(1, G * max(W, 1) * max(n_tokens, 1)), dtype=np.uint32)
        lens = np.empty(max(1, G * max(W, 1)), dtype=np.uint32)
        return L.rwkv_mi_batch_decode_beam(b._ptr, s.ctypes.data_as(P_UINT32), f.ctypes.data_as(P_UINT32), G, ctypes.byref(p), n_tokens,
                                           tok.ctypes.data_as(P_UINT32), lens.ctypes.data_as(P_UINT32), None, None, None)
    nine = list(range(9))
    cases = {
        "a slot out of range": lambda: beam([0, 4], [1], 1, 2, 3, []),
        "a slot named twice": lambda: beam([0, 1, 2, 1], [1, 2], 2, 2, 3, []),
        "width 0": lambda: beam([0], [1], 1, 0, 3, []),
        "width above RWKV_MI_TOP_MAX": lambda: beam(list(range(21)), [1], 1, 21, 3, []),
        "more than 8 end tokens": lambda: beam([0, 1], [1], 1, 2, 3, nine),
        "an end token >= n_vocab": lambda: beam([0, 1], [1], 1, 2, 3, [3, V]),
        "end_tokens NULL with n_end 2": lambda: beam([0, 1], [1], 1, 2, 3, [], n_end=2),
        "n_tokens 0": lambda: beam([0, 1], [1], 1, 2, 0, []),
        "n_groups 0": lambda: beam([0, 1], [1], 0, 2, 3, []),
        "more rows than slots": lambda: beam([0, 1, 2, 3, 0, 1], [1, 2, 3], 3, 2, 3, []),
        "a first token >= n_vocab": lambda: beam([0, 1, 2, 3], [1, V], 2, 2, 3, []),
        "copy: dst out of range": lambda: L.rwkv_mi_batch_state_copy(b._ptr, 4, 0, 1),
        "copy: src out of range": lambda: L.rwkv_mi_batch_state_copy(b._ptr, 0, 4, 1),
        "copy: an unknown bit": lambda: L.rwkv_mi_batch_state_copy(b._ptr, 1, 0, 16),
    }
    for what, call in cases.items():
        assert not call(), what
        assert lib.rwkv_get_last_error(m._ctx) & ARGS, what
        for s in range(4):
            assert np.array_equal(b.state_store(s), tw.state_store(s)), (what, s)
    lib.rwkv_set_print_errors(m._ctx, True)
    # states, parities and counters are as before: the next pass and the next draw are the twin's
    assert np.array_equal(b.eval([0, 1, 2, 3], [5, 6, 7, 8]), tw.eval([0, 1, 2, 3], [5, 6, 7, 8]))
    assert np.array_equal(b.eval_sample([0, 1, 2, 3], [1, 2, 3, 4], 1.0, 1.0, -1.0, [11, 22, 33, 44]), tw.eval_sample([0, 1, 2, 3], [1, 2, 3, 4], 1.0, 1.0, -1.0, [11, 22, 33, 44]))
    # ... and a valid call still runs
    assert beam([0, 1, 2, 3], [1, 2], 2, 2, 3, [])
    b.free(); tw.free(); m.free()
