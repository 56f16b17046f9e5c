"""Presence / frequency penalties and logit bias in the device sampler (rwkv_mi_*_penalized, csrc/sampling.hip k_draw<pen, 0> /
k_draw_rows<pen, 0, 0>). The penalised draw is pinned three ways: bit for bit to the existing sampler fed the adjusted logits computed on the
host in float32 (the statement of include/rwkv_mi355x.h, operation by operation); to the existing calls when the penalties are zero; and
to the reference's own statement (chat_with_bot.py:246-247, then sampling.py's sample_probs restated in float64). Loops, single steps and
bursts are compared with each other, rows with contexts that run that sequence alone. Tokens, states, counts and draw counters are
compared exactly.

A slot's draw counter cannot be read back; it is pinned through what it decides: a generator draw (u < 0) from known logits with the
expected counter, made by the existing sampler through its test hook, must give the token the slot gives."""
import numpy as np
import pytest

import reference_constants as R
from gpu_lib import library, model, pkg, synth
from test_gpu_batch import _tok
from test_gpu_batch_sample import _descending_cumsum, _sample_rows, _top_p_clear_of_the_cumsums
from test_gpu_sampling import ref_distribution

pytestmark = pytest.mark.gpu

ARGS = 1 << 8   # RWKV_ERROR_ARGS
MODELS = [("test-v4", "Q8_0"), ("test-v6", "Q5_1"), ("test-v7", "Q5_1"), ("mega-v6-2048-v64k", "Q4_0")]
NEG = -999999999.0   # (the chat program's new_line_logit_bias)


def _synth(tmp_path, name, fmt, seed=7):
    library()
    p = str(tmp_path / f"{name}-{fmt}.bin")
    synth.write_model(p, synth.CONFIGS[name], fmt, seed=seed)
    return p


def _bias_row(V, bias):
    """The bias table of a slot as the device holds it: float32 [V], zero where nothing is set; None without a bias."""
    if not bias:
        return None
    row = np.zeros(V, dtype=np.float32)
    for k, v in bias.items():
        row[k] = np.float32(v)
    return row


def _adjust(logits, counts, presence, frequency, bias_row):
    """adj[j] = (l[j] - (presence + (float) count[j] * frequency)) + bias[j], every operation rounded to float32 in that order; the penalty
    where count[j] > 0 (the reference's loop runs over the tokens that have occurred), the bias add skipped without a bias."""
    l = np.ascontiguousarray(logits, dtype=np.float32)
    c = counts.astype(np.float32)
    pen = np.float32(presence) + c * np.float32(frequency)
    assert pen.dtype == np.float32
    adj = np.where(counts > 0, l - pen, l).astype(np.float32)
    if bias_row is not None:
        adj = adj + bias_row
    assert adj.dtype == np.float32
    return adj


def _reference_adjust(logits, token_counts, presence, frequency, bias):
    """chat_with_bot.py:246-247 on the reference's float32 array, with Python floats as it has them, then the logit bias."""
    out = np.array(logits, dtype=np.float32)
    for n in token_counts:
        out[n] -= presence + token_counts[n] * frequency
    for k, v in (bias or {}).items():
        out[k] += v
    return out


def _counts_of(V, tokens):
    return np.bincount(np.asarray(tokens, dtype=np.int64), minlength=V).astype(np.uint32)


def _oracle_draw(adj_rows, T, P, U, seeds, counters):
    """The existing sampler (plain k_draw_rows<plain, 0, 0> through its test hook) on the adjusted logits: tokens and the counters afterwards."""
    n = len(adj_rows)
    table = pkg.sample_params(n, T, P, U, seeds)
    return _sample_rows(np.stack(adj_rows), table, np.asarray(counters, dtype=np.uint64), 1)


# ---- 1. bit for bit against the existing sampler on the adjusted logits ----

@pytest.mark.parametrize("name,fmt", MODELS)
def test_penalised_draw_is_the_plain_sampler_on_the_adjusted_logits(tmp_path, name, fmt):
    p = _synth(tmp_path, name, fmt, seed=11)
    m = model(p)
    V = m.n_vocab
    b, twin = pkg.RWKVBatch(m, 7), pkg.RWKVBatch(m, 7)
    slots = [4, 1, 5, 0, 2, 6]
    n = len(slots)
    T = [0.0, 1.0, 0.7, 1.5, 1.0, 0.3]
    P = [0.8, 0.9, 0.5, 1.0, 0.0, 0.95]
    U = [-1.0, -1.0, 0.37, -1.0, 0.81, -1.0]
    seeds = [7, 8, 9, 10, 11, 12]
    presence = [0.2, 0.25, 0.0, 1.5, 0.2, 0.7]
    frequency = [0.2, 0.5, 0.3, 0.0, 0.2, 0.1]
    record = [True, True, False, True, True, True]
    bias = {4: {3: NEG, 17: 2.0}, 5: {V - 1: -np.inf, 0: 0.5}, 2: {9: -3.25}}
    rng = np.random.default_rng(5)
    counts = {s: np.zeros(V, dtype=np.uint32) for s in slots}
    counters = {s: 3 * s + 1 for s in slots}
    for s in slots:
        b.rng_seek(s, counters[s])
        if s != 0:   # (slot 0 starts without a history)
            pre = rng.integers(0, min(V, 40), size=25).tolist() + [V - 2] * 3
            b.counts_add(s, pre)
            counts[s] += _counts_of(V, pre)
        assert np.array_equal(b.counts(s), counts[s]), (name, s)
        if s in bias:
            b.set_logit_bias(s, bias[s])
    toks = [_tok(0, s, V) for s in slots]
    for step in range(3):
        out, lg = b.eval_sample_penalized(slots, toks, T, P, U, seeds, presence, frequency, record, want_logits=True)
        assert np.array_equal(lg, twin.eval(slots, toks)), (name, step, "the returned logits are the model's")
        adj = [_adjust(lg[i], counts[s], presence[i], frequency[i], _bias_row(V, bias.get(s))) for i, s in enumerate(slots)]
        want, ctr = _oracle_draw(adj, T, P, U, seeds, [counters[s] for s in slots])
        assert np.array_equal(out, want), (name, step, out.tolist(), want.tolist())
        for i, s in enumerate(slots):
            counters[s] = int(ctr[i])
            if record[i]:
                counts[s][int(out[i])] += 1
            assert np.array_equal(b.counts(s), counts[s]), (name, step, s)
            assert np.array_equal(b.state_store(s), twin.state_store(s)), (name, step, s)
        toks = [int(t) for t in out]
    # the draw counters after the last step: one more generator draw on every row (no argmax) against the oracle with the expected counters
    out, lg = b.eval_sample_penalized(slots, toks, 1.0, 1.0, -1.0, seeds, presence, frequency, False, want_logits=True)
    adj = [_adjust(lg[i], counts[s], presence[i], frequency[i], _bias_row(V, bias.get(s))) for i, s in enumerate(slots)]
    want, _ = _oracle_draw(adj, [1.0] * n, [1.0] * n, [-1.0] * n, seeds, [counters[s] for s in slots])
    assert np.array_equal(out, want), (name, "draw counters", out.tolist(), want.tolist())
    b.free()
    twin.free()
    m.free()


# ---- 2. zero is plain ----

def test_zero_penalties_are_the_plain_calls(golden_dir):
    path = R.fixture_path(golden_dir, "6v0-3m", "Q5_0")
    m = model(path)
    V = m.n_vocab
    b, twin = pkg.RWKVBatch(m, 6), pkg.RWKVBatch(m, 6)
    slots = [5, 2, 4, 0, 1, 3]
    T = [1.0, 0.7, 1.5, 0.0, 1.0, 0.3]
    P = [0.8, 0.95, 1.0, 0.5, 0.0, 0.8]
    seeds = [3, 4, 5, 6, 7, 8]
    record = [True, False, True, False, True, False]
    b.counts_add(2, [1, 1, 2, 3])   # (counts do not matter at zero penalties: count * 0 is 0)
    toks = [_tok(0, s, V) for s in slots]
    for step in range(4):
        got = b.eval_sample_penalized(slots, toks, T, P, -1.0, seeds, 0.0, 0.0, record)
        want = twin.eval_sample(slots, toks, T, P, -1.0, seeds)
        assert np.array_equal(got, want), (step, got.tolist(), want.tolist())   # (equal streams from step 1 on: equal draw counters)
        toks = [int(t) for t in got]
    rows = [[_tok(9, s, V), _tok(10, s, V), _tok(11, s, V)][: 1 + i % 3] for i, s in enumerate(slots)]
    got = b.eval_ragged_sample_penalized(slots, rows, T, P, -1.0, seeds, 0.0, 0.0, record)
    want = twin.eval_ragged_sample(slots, rows, T, P, -1.0, seeds)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    got = b.eval_sample_penalized(slots, [int(t) for t in got], 1.0, 1.0, -1.0, seeds, 0.0, 0.0, record)
    want = twin.eval_sample(slots, [int(t) for t in want], 1.0, 1.0, -1.0, seeds)
    assert np.array_equal(got, want), ("draw counters after the ragged pass", got.tolist(), want.tolist())
    for s in slots:
        assert np.array_equal(b.state_store(s), twin.state_store(s)), s
    # the loop: after rng_seek(slot, 0) it is decode_sample (which resets the counters itself)
    for s in slots:
        b.rng_seek(s, 0)
    first = [int(t) for t in got]
    la, _ = b.decode_sample_penalized(slots, first, 16, T, P, seeds, 0.0, 0.0)
    lb, _ = twin.decode_sample(slots, first, 16, T, P, seeds)
    assert np.array_equal(la, lb), (la.tolist(), lb.tolist())
    for s in slots:
        assert np.array_equal(b.state_store(s), twin.state_store(s)), s
    # ... and on a context
    c = m.clone()
    c.state_load(None)
    a1, _ = c.decode_sample(7, 16, 1.0, 0.9, 42)
    st = c.state_store()
    c.state_load(None)
    c.rng_seek(0)
    a2, _ = c.decode_sample_penalized(7, 16, 1.0, 0.9, 42, 0.0, 0.0)
    assert np.array_equal(a1, a2) and np.array_equal(c.state_store(), st)
    c.free()
    b.free()
    twin.free()
    m.free()


# ---- 3. the reference's statement ----

@pytest.mark.parametrize("name,fmt", MODELS)
def test_penalised_draw_follows_the_reference_statement(tmp_path, name, fmt):
    p = _synth(tmp_path, name, fmt, seed=13)
    m = model(p)
    V = m.n_vocab
    presence, frequency = 0.25, 0.5   # (dyadic: the reference's double-precision penalty is exact in float32)
    bias = {5: NEG, 21: 2.0}
    history = [3, 3, 3, 9, 21, 40, 40, V - 1, 7, 7, 7, 7]
    token_counts = {}
    for t in history:
        token_counts[t] = token_counts.get(t, 0) + 1
    logits, st0 = m.eval(7, None)
    ref_adj = _reference_adjust(logits, token_counts, presence, frequency, bias)
    # the reference's adjusted logits are the statement's, bit for bit
    assert np.array_equal(ref_adj, _adjust(logits, _counts_of(V, history), presence, frequency, _bias_row(V, bias)))
    cases = [(1.0, 0.3), (0.7, 0.8), (1.5, 0.9), (0.0, 0.0), (1.0, 1.0), (0.3, 0.5)]
    params = [(t, _top_p_clear_of_the_cumsums(ref_adj, q) if 0.0 < q < 1.0 else q) for t, q in cases]
    for t, q in params:   # condition on the reference alone: where top_p cuts, no descending cumulative sum lies within 1e-5 of it
        if 0.0 < q < 1.0:
            d = float(np.abs(_descending_cumsum(ref_adj) - q).min())
            assert d > 1e-5, (name, t, q, d)
    ref = [ref_distribution(ref_adj, t, q) for t, q in params]
    cdf = [np.cumsum(pr) for pr in ref]
    n = len(params)
    b = pkg.RWKVBatch(m, n)
    slots = list(range(n))
    for s in slots:
        b.counts_add(s, history)
        b.set_logit_bias(s, bias)
    m.counts_add(history)
    m.set_logit_bias(bias)
    T, P = [q[0] for q in params], [q[1] for q in params]
    for u in np.linspace(0.001, 0.999, 41):
        for s in slots:
            b.state_load(s, None)
        out, lg = b.eval_sample_penalized(slots, [7] * n, T, P, float(u), 0, presence, frequency, False, want_logits=True)
        assert np.array_equal(lg[0], logits)
        for r in range(n):
            tok, pr = int(out[r]), ref[r]
            assert tok < V and tok != 5 and pr[tok] > 0.0, (name, params[r], u, tok)
            lo = cdf[r][tok] - pr[tok]
            assert lo - 1e-4 <= u <= cdf[r][tok] + 1e-4, (name, params[r], u, tok, lo, cdf[r][tok])
            # the single entry point on the context's own logits (those of m.eval above): the same token
            assert m.sample_penalized(T[r], P[r], float(u), 0, presence, frequency, record=False) == tok, (name, params[r], u)
    assert np.array_equal(m.counts(), _counts_of(V, history)), "record=False counted a token"
    assert np.array_equal(m.logits_store(), logits), "the sampler changed the logits"
    b.free()
    m.free()


# ---- 4. loop = steps = bursts ----

@pytest.mark.parametrize("name,fmt", [("test-v6", "Q5_1"), ("mega-v6-2048-v64k", "Q4_0")])
def test_loop_equals_bursts_equals_steps(tmp_path, name, fmt):
    p = _synth(tmp_path, name, fmt, seed=17)
    m = model(p)
    V = m.n_vocab
    b = pkg.RWKVBatch(m, 6)
    T, P, seeds = [1.0, 0.8], [0.9, 1.0], [101, 202]
    presence, frequency = [0.2, 0.5], [0.2, 0.25]
    bias = {0: {11: NEG, 30: 1.0}, 1: None}
    pre = [4, 4, 8, 15, 16, 23, 42]
    groups = {"loop": [0, 1], "bursts": [2, 3], "steps": [4, 5]}
    for sl in groups.values():
        for i, s in enumerate(sl):
            b.state_load(s, None)
            b.counts_reset(s)
            b.counts_add(s, pre)
            b.rng_seek(s, 5)
            if bias[i]:
                b.set_logit_bias(s, bias[i])
    first = [3, 9]
    loop, ms = b.decode_sample_penalized(groups["loop"], first, 32, T, P, seeds, presence, frequency)
    assert loop.shape == (2, 32) and ms > 0.0
    b1, _ = b.decode_sample_penalized(groups["bursts"], first, 16, T, P, seeds, presence, frequency)
    b2, _ = b.decode_sample_penalized(groups["bursts"], [int(t) for t in b1[:, -1]], 16, T, P, seeds, presence, frequency)
    bursts = np.concatenate([b1, b2], axis=1)
    steps, toks = [], list(first)
    for _ in range(32):
        out = b.eval_sample_penalized(groups["steps"], toks, T, P, -1.0, seeds, presence, frequency, True)
        steps.append(out)
        toks = [int(t) for t in out]
    steps = np.stack(steps, axis=1)
    assert np.array_equal(loop, bursts), (name, loop.tolist(), bursts.tolist())
    assert np.array_equal(loop, steps), (name, loop.tolist(), steps.tolist())
    for i in range(2):
        want = _counts_of(V, pre) + _counts_of(V, loop[i])
        states = [b.state_store(sl[i]) for sl in groups.values()]
        for k, sl in enumerate(groups.values()):
            assert np.array_equal(b.counts(sl[i]), want), (name, i, k)
            assert np.array_equal(states[k], states[0]), (name, i, k)
    # the draw counters: 5 + 32 in every group (no row is an argmax) -- one more generator draw each, against the oracle with that counter
    every = groups["loop"] + groups["bursts"] + groups["steps"]
    nxt = [int(loop[i % 2, -1]) for i in range(6)]
    out, lg = b.eval_sample_penalized(every, nxt, 1.0, 1.0, -1.0, seeds * 3, presence * 3, frequency * 3, False, want_logits=True)
    adj = [_adjust(lg[k], _counts_of(V, pre) + _counts_of(V, loop[k % 2]), presence[k % 2], frequency[k % 2], _bias_row(V, bias[k % 2])) for k in range(6)]
    want, _ = _oracle_draw(adj, [1.0] * 6, [1.0] * 6, [-1.0] * 6, seeds * 3, [37] * 6)
    assert np.array_equal(out, want), (name, out.tolist(), want.tolist())
    b.free()
    m.free()


# ---- 5. a row is its sequence alone ----

@pytest.mark.parametrize("name,fmt", [("test-v7", "Q5_1"), ("test-v4", "Q8_0"), ("mega-v6-2048-v64k", "Q4_0")])
def test_rows_of_the_penalised_loop_equal_the_context_alone(tmp_path, name, fmt):
    p = _synth(tmp_path, name, fmt, seed=19)
    m = model(p)
    V = m.n_vocab
    b = pkg.RWKVBatch(m, 8)
    spec = {   # slot: (temperature, top_p, seed, presence, frequency, bias, counts_add, rng_seek)
        6: (1.0, 0.9, 11, 0.2, 0.2, {2: NEG}, [1, 2, 3], 0),
        1: (0.7, 1.0, 12, 0.5, 0.0, None, [], 7),
        3: (0.0, 0.8, 13, 1.0, 0.5, {8: 4.0, 1: -1.0}, [9, 9, 9], 2),
        0: (1.5, 0.5, 14, 0.0, 0.75, None, [5] * 20, 100),
        5: (1.0, 0.0, 15, 0.25, 0.25, {V - 1: 3.0}, [V - 1], 1 << 33),
    }
    ctx = m.clone()
    alone = {}
    for s, (t, q, seed, pr, fr, bias, pre, ctr) in spec.items():
        ctx.state_load(None)
        ctx.eval_resident([_tok(1, s, V)], want_logits=False)
        start = ctx.state_store()
        ctx.counts_reset()
        ctx.counts_add(pre)
        ctx.set_logit_bias(bias or {})
        ctx.rng_seek(ctr)
        toks, _ = ctx.decode_sample_penalized(_tok(2, s, V), 16, t, q, seed, pr, fr)
        alone[s] = (start, toks, ctx.state_store(), ctx.counts())
        assert np.array_equal(alone[s][3], _counts_of(V, pre) + _counts_of(V, toks)), (name, s)
    for order in ([6, 1, 3, 0, 5], [5, 0, 3, 1, 6], [3, 6], [1, 5, 0]):
        for s in order:
            t, q, seed, pr, fr, bias, pre, ctr = spec[s]
            b.state_load(s, alone[s][0])
            b.counts_reset(s)
            b.counts_add(s, pre)
            b.set_logit_bias(s, bias or {})
            b.rng_seek(s, ctr)
        col = lambda k: [spec[s][k] for s in order]   # noqa: E731
        got, _ = b.decode_sample_penalized(order, [_tok(2, s, V) for s in order], 16, col(0), col(1), col(2), col(3), col(4))
        for i, s in enumerate(order):
            assert np.array_equal(got[i], alone[s][1]), (name, order, s, got[i].tolist(), alone[s][1].tolist())
            assert np.array_equal(b.state_store(s), alone[s][2]), (name, order, s)
            assert np.array_equal(b.counts(s), alone[s][3]), (name, order, s)
    ctx.free()
    b.free()
    m.free()


# ---- 6. ragged: a prompt in chunks ----

def test_chunked_prompt_leaves_counts_and_counters_as_the_whole_prompt(golden_dir):
    path = R.fixture_path(golden_dir, "6v0-3m", "Q5_0")
    m = model(path)
    V = m.n_vocab
    b = pkg.RWKVBatch(m, 4)
    prompt = [(13 * j + 1) % V for j in range(40)]
    pre = [2, 2, 50]
    bias = {60: NEG, 61: 1.5}
    t, q, seed, pr, fr = 1.0, 0.9, 77, 0.5, 0.25
    for s in (0, 1, 2, 3):
        b.rng_seek(s, 4)
        b.counts_add(s, pre)
        b.set_logit_bias(s, bias)
    # slot 0: the whole prompt in one call, with a decode row beside it; slot 1: chunks of 16, 16 and 8 (non-final: argmax, not recorded)
    whole = b.eval_ragged_sample_penalized([0, 2], [prompt, [9]], [t, 1.0], [q, 1.0], -1.0, [seed, 5], pr, fr, True)
    c1 = b.eval_ragged_sample_penalized([3, 1], [[9], prompt[:16]], [1.0, 0.0], [1.0, q], -1.0, [5, seed], pr, fr, [True, False])
    assert np.array_equal(b.counts(1), _counts_of(V, pre)), "a chunk with record == 0 counted its token"
    b.eval_ragged_sample_penalized([1], [prompt[16:32]], 0.0, q, -1.0, seed, pr, fr, False)
    last = b.eval_ragged_sample_penalized([1], [prompt[32:]], t, q, -1.0, seed, pr, fr, True)
    assert int(last[0]) == int(whole[0]) and int(c1[0]) == int(whole[1])
    # step 1's oracle: the existing sampler on the adjusted logits of the prompt's last token, with the draw counter the slot was given
    logits, state = m.eval_sequence(prompt, None)
    adj = _adjust(logits, _counts_of(V, pre), pr, fr, _bias_row(V, bias))
    want, _ = _oracle_draw([adj], [t], [q], [-1.0], [seed], [4])
    assert int(last[0]) == int(want[0]), (int(last[0]), int(want[0]))
    for s in (0, 1):
        assert np.array_equal(b.counts(s), _counts_of(V, pre) + _counts_of(V, [int(whole[0])])), s
        assert np.array_equal(b.state_store(s), state), s
    # the draw counters of both: 5 -- the next generator draw of each is the other's, and the oracle's with that counter
    out, lg = b.eval_sample_penalized([1, 0], [int(last[0])] * 2, 1.0, 1.0, -1.0, seed, pr, fr, True, want_logits=True)
    adj = _adjust(lg[0], b.counts(1) - _counts_of(V, [int(out[0])]), pr, fr, _bias_row(V, bias))
    want, _ = _oracle_draw([adj], [1.0], [1.0], [-1.0], [seed], [5])
    assert int(out[0]) == int(out[1]) == int(want[0]), (out.tolist(), want.tolist())
    b.free()
    m.free()


# ---- 7. rejected calls change nothing ----

def test_rejected_penalty_calls_change_nothing(golden_dir):
    path = R.fixture_path(golden_dir, "6v0-3m", "Q5_0")
    m = model(path)
    V = m.n_vocab
    b, twin = pkg.RWKVBatch(m, 4), pkg.RWKVBatch(m, 4)
    slots = [2, 0, 3, 1]
    good = dict(temperature=[1.0, 0.7, 1.5, 1.0], top_p=[0.8, 0.95, 1.0, 0.0], u=-1.0, seed=[3, 4, 5, 6], presence=0.5, frequency=0.25)
    bias = {7: NEG, 8: 2.0}
    for x in (b, twin):
        for s in slots:
            x.counts_add(s, [1, 2, 2, s])
            x.set_logit_bias(s, bias)
        first = x.eval_sample_penalized(slots, [_tok(0, s, V) for s in slots], **good)
    snapshot = {s: (b.state_store(s), b.counts(s)) for s in slots}
    nan, inf = float("nan"), float("inf")
    L, ptr = b._L, b._ptr

    def rejected(call):
        b.last_error = 0
        with pytest.raises(ValueError):
            call()
        assert b.last_error & ARGS, b.last_error

    # what the plain counterparts reject, and the penalties
    for kw in (dict(presence=nan), dict(frequency=[0.1, inf, 0.1, 0.1]), dict(presence=[0.0, 0.0, -inf, 0.0]), dict(frequency=nan),
               dict(temperature=-1.0), dict(top_p=1.5), dict(u=1.0)):
        a = dict(good)
        a.update(kw)
        rejected(lambda: b.eval_sample_penalized(slots, [1, 2, 3, 4], **a))
        rejected(lambda: b.eval_ragged_sample_penalized(slots, [[1], [2, 3], [4], [5]], **a))
        if "u" not in kw:
            a.pop("u")
            rejected(lambda: b.decode_sample_penalized(slots, [1, 2, 3, 4], 3, **a))
    for sl, tk in (([1, 1], [3, 4]), ([4], [3]), ([0], [V]), ([], [])):
        rejected(lambda: b.eval_sample_penalized(sl, tk, 1.0, 0.8, -1.0, 1, 0.2, 0.2))
        rejected(lambda: b.decode_sample_penalized(sl, tk, 3, 1.0, 0.8, 1, 0.2, 0.2))
        rejected(lambda: b.eval_ragged_sample_penalized(sl, [[t] for t in tk], 1.0, 0.8, -1.0, 1, 0.2, 0.2))
    rejected(lambda: b.eval_ragged_sample_penalized([0], [[]], 1.0, 0.8, -1.0, 1, 0.2, 0.2))
    # penalties == NULL (through the C entry points: the binding always passes a table)
    s32, t32 = pkg.rwkv_cpp._u32([0]), pkg.rwkv_cpp._u32([1])
    P32 = pkg.rwkv_cpp.P_UINT32
    sp = pkg.sample_params(1, 1.0, 0.8, -1.0, 1)
    out = np.zeros(4, dtype=np.uint32)
    lib = m._library
    for call in (lambda: L.rwkv_mi_batch_eval_sample_penalized(ptr, s32.ctypes.data_as(P32), t32.ctypes.data_as(P32), 1, sp, None, out.ctypes.data_as(P32), None),
                 lambda: L.rwkv_mi_batch_eval_ragged_sample_penalized(ptr, s32.ctypes.data_as(P32), t32.ctypes.data_as(P32), t32.ctypes.data_as(P32), 1, sp, None,
                                                                      out.ctypes.data_as(P32), None),
                 lambda: L.rwkv_mi_batch_decode_sample_penalized(ptr, s32.ctypes.data_as(P32), t32.ctypes.data_as(P32), 1, 2, sp, None, out.ctypes.data_as(P32), None)):
        assert not call()
        assert lib.rwkv_get_last_error(m._ctx) & ARGS
    # the tables' own calls
    rejected(lambda: b.set_logit_bias(0, {V: 1.0}))
    rejected(lambda: b.set_logit_bias(0, {3: nan}))
    rejected(lambda: b.set_logit_bias(0, {3: 1.0, 4: inf}))
    ids, vals = pkg.rwkv_cpp._u32([3, 9, 3]), np.array([1.0, 2.0, 3.0], dtype=np.float32)
    assert not L.rwkv_mi_batch_logit_bias_set(ptr, 0, ids.ctypes.data_as(P32), vals.ctypes.data_as(pkg.rwkv_cpp.P_FLOAT), 3)   # (a repeated id)
    assert lib.rwkv_get_last_error(m._ctx) & ARGS
    rejected(lambda: b.counts_add(0, [1, V]))
    rejected(lambda: b.counts_add(4, [1]))
    rejected(lambda: b.counts_reset(4))
    rejected(lambda: b.counts(9))
    rejected(lambda: b.set_logit_bias(4, {1: 1.0}))
    # ... and the context's
    c = m.clone()
    lg, _ = c.eval(3, None)
    fav = int(np.argmax(lg))
    cbias = {fav: NEG, (fav + 1) % V: 2.0}
    c.counts_add([1, 1, 5])
    c.set_logit_bias(cbias)
    for call in (lambda: c.counts_add([V]), lambda: c.set_logit_bias({V + 3: 0.0}), lambda: c.set_logit_bias({1: nan}), lambda: c.set_logit_bias({1: inf}),
                 lambda: c.sample_penalized(1.0, 0.8, 0.5, 0, nan, 0.2), lambda: c.sample_penalized(1.0, 0.8, 0.5, 0, 0.2, inf),
                 lambda: c.sample_penalized(-1.0, 0.8, 0.5, 0, 0.2, 0.2), lambda: c.decode_sample_penalized(V, 3, 1.0, 0.8, 0, 0.2, 0.2),
                 lambda: c.decode_sample_penalized(1, 3, 1.0, 0.8, 0, nan, 0.2), lambda: c.decode_sample_penalized(1, 0, 1.0, 0.8, 0, 0.2, 0.2)):
        c.last_error = 0
        with pytest.raises(ValueError):
            call()
        assert c.last_error & ARGS, c.last_error
    assert np.array_equal(c.counts(), _counts_of(V, [1, 1, 5]))
    # (the previous bias still holds: the argmax of the context's logits under it, not the favourite)
    want = int(np.argmax(_adjust(lg, _counts_of(V, [1, 1, 5]), 0.5, 0.25, _bias_row(V, cbias))))
    assert want != fav and c.sample_penalized(0.0, 1.0, 0.5, 0, 0.5, 0.25, record=False) == want
    c.free()
    # nothing moved: states and counts now, and parities, draw counters and the bias through what the next valid calls return
    for s in slots:
        assert np.array_equal(b.state_store(s), snapshot[s][0]), s
        assert np.array_equal(b.counts(s), snapshot[s][1]), s
    nxt = [int(t) for t in first]
    assert np.array_equal(b.eval_sample_penalized(slots, nxt, **good), twin.eval_sample_penalized(slots, nxt, **good))
    la, _ = b.decode_sample_penalized([3, 0], [9, 10], 6, 1.0, 0.9, [21, 22], 0.5, 0.25)
    lb, _ = twin.decode_sample_penalized([3, 0], [9, 10], 6, 1.0, 0.9, [21, 22], 0.5, 0.25)
    assert np.array_equal(la, lb) and not np.isin(la, [7]).any()
    for s in slots:
        assert np.array_equal(b.state_store(s), twin.state_store(s)), s
        assert np.array_equal(b.counts(s), twin.counts(s)), s
    b.free()
    twin.free()
    m.free()


def test_bias_is_replaced_and_cleared(golden_dir):
    path = R.fixture_path(golden_dir, "6v0-3m", "Q5_0")
    m = model(path)
    V = m.n_vocab
    b = pkg.RWKVBatch(m, 2)
    lg = b.eval([0], [3])[0]
    top = np.argsort(lg)[::-1]
    a, c, d = int(top[0]), int(top[1]), int(top[2])

    def argmax_now():
        b.state_load(0, None)
        return int(b.eval_sample_penalized([0], [3], 0.0, 1.0, 0.5, 0, 0.0, 0.0, False)[0])

    assert argmax_now() == a
    b.set_logit_bias(0, {a: NEG})
    assert argmax_now() == c
    b.set_logit_bias(0, {c: -np.inf})   # replaces: a is back
    assert argmax_now() == a
    b.set_logit_bias(0, {a: NEG, c: NEG})
    assert argmax_now() == d
    b.set_logit_bias(0, {})             # cleared
    assert argmax_now() == a
    # the penalty itself: enough occurrences of the favourite and the next one wins; the presence penalty alone does it when the margin is small
    b.counts_add(0, [a] * 3)
    gap = float(lg[a] - lg[c])
    b.state_load(0, None)
    assert int(b.eval_sample_penalized([0], [3], 0.0, 1.0, 0.5, 0, 0.0, gap, False)[0]) == c   # (3 x gap > gap)
    b.state_load(0, None)
    assert int(b.eval_sample_penalized([0], [3], 0.0, 1.0, 0.5, 0, 2.0 * gap, 0.0, False)[0]) == c
    b.counts_reset(0)
    assert not b.counts(0).any() and argmax_now() == a
    b.free()
    m.free()


# ---- 8. beside the persistent kernel ----

def test_penalised_loop_next_to_persistent_kernel(tmp_path, monkeypatch):
    monkeypatch.setenv("RWKV_MI_NO_AUTOTUNE", "1")
    p = _synth(tmp_path, "mega-v6-4096", "Q4_0", seed=21)
    m = model(p)
    assert m.decode_path() == 2, m.persist_info()
    V = m.n_vocab
    b = pkg.RWKVBatch(m, 8)
    slots = list(range(8))
    T = [0.0, 0.3, 0.7, 1.0, 1.5, 0.0, 1.0, 0.7]
    seeds = [s + 1 for s in slots]
    pre = [5, 5, 6]

    def fresh():
        m.state_load(None)
        for s in slots:
            b.state_load(s, None)
            b.counts_reset(s)
            b.counts_add(s, pre)
            b.rng_seek(s, 0)
            b.set_logit_bias(s, {10 + s: NEG} if s % 2 else {})

    def batch_round(first):
        return b.decode_sample_penalized(slots, first, 4, T, 0.9, seeds, 0.2, 0.2)[0]

    # solo: the context's greedy rounds, then the batch's penalised rounds
    fresh()
    solo_ctx, tok = [], 3
    for _ in range(3):
        toks, _ = m.decode_greedy(tok, 4)
        solo_ctx.append(toks)
        tok = int(toks[-1])
    solo_ctx_state = m.state_store()
    solo_b, first = [], [_tok(0, s, V) for s in slots]
    for _ in range(3):
        out = batch_round(first)
        solo_b.append(out)
        first = [int(t) for t in out[:, -1]]
    solo_counts = [b.counts(s) for s in slots]
    solo_states = [b.state_store(s) for s in slots]
    # interleaved in one process
    fresh()
    tok, first = 3, [_tok(0, s, V) for s in slots]
    for rnd in range(3):
        toks, _ = m.decode_greedy(tok, 4)
        assert np.array_equal(toks, solo_ctx[rnd]), (rnd, list(toks), list(solo_ctx[rnd]))
        tok = int(toks[-1])
        out = batch_round(first)
        assert np.array_equal(out, solo_b[rnd]), (rnd, out.tolist(), solo_b[rnd].tolist())
        first = [int(t) for t in out[:, -1]]
        assert m.healthy()
    assert np.array_equal(m.state_store(), solo_ctx_state)
    for s in slots:
        assert np.array_equal(b.counts(s), solo_counts[s]), s
        assert np.array_equal(b.state_store(s), solo_states[s]), s
        assert np.array_equal(b.counts(s), _counts_of(V, pre) + _counts_of(V, np.concatenate([r[s] for r in solo_b]))), s
    assert m.decode_path() == 2 and m.healthy()
    b.free()
    m.free()
