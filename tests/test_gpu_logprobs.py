"""The log-prob report on the device (rwkv_mi_*set_logprobs, csrc/score.hip k_logprob_rows): the log-prob of every emitted token and the
top-N alternatives of its step, taken from the model's logits inside the calls that emit.

What is exact is held exactly: the ids against np.lexsort((index, -logit)) of the entries that are not NaN (logprobs_ref.top_ids); every
log-prob, bit for bit, against the scoring kernel (rwkv_test_score_rows / score_ragged) on the same logits with that id as target -- the two
kernels share one body; tokens, states, draw counters and counts against the same call with the report off. A slot's draw counter cannot be
read back; it is pinned through what it decides: one more generator draw must give the token the twin gives.
The log-probs have the ONE tolerance of tests/test_gpu_score.py, derived there and not measured: |dev - float32(ref)| <= ulp32(ref) + 2^-32
against NumPy float64 on the same f32 logits."""
import ctypes
import os

import numpy as np
import pytest

import reference_constants as R
from gpu_lib import library, model, pkg, synth
from logprobs_ref import NO_TOKEN, f64_logprobs, top_ids
from test_gpu_score import _crafted, check_logprob, score_rows, _hooks

pytestmark = pytest.mark.gpu

ARGS = 1 << 8   # RWKV_ERROR_ARGS
P_UINT32 = ctypes.POINTER(ctypes.c_uint32)
P_FLOAT = ctypes.POINTER(ctypes.c_float)
# every architecture's tiny model in one quantised and (where shipped) one float format
GOLDEN = [(v, "Q5_1") for v in R.VERSIONS] + [(v, "FP16") for v in R.HAVE_FP32_FP16]
SEEDS = (11, 22, 33)
FIRST = (34, 105, 110)
SLOTS = [0, 1, 2]


def logprob_rows(logits, tokens, top_n):
    """k_logprob_rows through the test hook on logits [rows][V]: chosen [rows], ids [rows][top_n], log-probs [rows][top_n]."""
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    rows, V = logits.shape
    tk = np.ascontiguousarray(np.asarray(tokens, dtype=np.int64).astype(np.uint32))
    ch = np.full(rows, np.nan, dtype=np.float32)
    ids = np.full((rows, top_n), 0xDEAD, dtype=np.uint32)
    lp = np.full((rows, top_n), np.nan, dtype=np.float32)
    ok = _hooks().rwkv_test_logprob_rows(logits.ctypes.data_as(P_FLOAT), rows, V, tk.ctypes.data_as(P_UINT32), top_n, ch.ctypes.data_as(P_FLOAT),
                                         ids.ctypes.data_as(P_UINT32) if top_n else None, lp.ctypes.data_as(P_FLOAT) if top_n else None)
    assert ok, "rwkv_test_logprob_rows failed"
    return ch, ids, lp


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_against_f64(dev, ref, what):
    """the file's one tolerance where the reference is finite; where it is not (a -inf logit, a row with a NaN) the value itself"""
    if np.isnan(ref):
        assert np.isnan(dev), (what, float(dev))
    elif np.isinf(ref):
        assert float(dev) == ref, (what, float(dev), ref)
    else:
        check_logprob(dev, ref, what)


# ---- 1. the kernel on crafted logits ----

def _rows_for(V, seed):
    """test_gpu_score.py's crafted families (model-like / wide / narrow spreads, equal logits, one dominant logit, magnitudes of +-1e4, exact ties
    at 5, 63, 64, V // 2, 1025 % V, V - 1) with an emitted token per row, and the rows the ordering rule needs."""
    logits, targets = _crafted(V, seed)
    tokens = [int(t) if int(t) < V else 0 for t in targets]
    rows = list(logits)
    rng = np.random.default_rng(seed + 1)

    def add(l, t):
        rows.append(np.asarray(l, dtype=np.float32)); tokens.append(int(t))
    g = min(30, V - 3)                                   # a tie group wider than every top_n of the file (21 of the 24 of the tiny row)
    top = rng.standard_normal(V).astype(np.float32)
    idx = rng.choice(V, size=g, replace=False)
    idx[:4] = (5, V - 1, 64 % V, (1024 + 5) % V) if V > 1100 else (5, V - 1, 16 % V, 17 % V)   # (across lane, wave and 1024-stride boundaries)
    idx = np.unique(idx)
    top[idx] = top.max() + 2.0
    add(top, idx[-1])                                    # the tie group at the top: it straddles the N-th place for N = 1, 5, 20
    below = top.copy()
    free = np.setdiff1d(np.arange(V), idx)[:3]
    below[free] = top.max() + np.array([3.0, 1.0, 2.0], dtype=np.float32)
    add(below, free[1])                                  # ... and behind three larger logits: it straddles for N = 5 and 20
    ninf = rng.standard_normal(V).astype(np.float32)
    ninf[rng.random(V) < 0.1] = -np.inf
    add(ninf, int(np.argmax(ninf)))                      # some -inf
    few = np.full(V, -np.inf, dtype=np.float32)
    keep = rng.choice(V, size=3, replace=False)
    few[keep] = (0.5, -1.5, 0.5)
    add(few, keep[1])                                    # all but three -inf: -inf ranks behind them, by index
    zeros = -np.abs(rng.standard_normal(V)).astype(np.float32) - 1.0
    z = rng.choice(V, size=6, replace=False)
    zeros[z] = (0.0, -0.0, -0.0, 0.0, -0.0, 0.0)
    add(zeros, z[2])                                     # -0 ties with +0
    nans = np.full(V, np.nan, dtype=np.float32)
    k3 = rng.choice(V, size=3, replace=False)
    nans[k3] = (1.0, -np.inf, 2.0)
    add(nans, k3[0])                                     # fewer than top_n entries that are not NaN
    return np.stack(rows), np.asarray(tokens, dtype=np.int64)


@pytest.mark.parametrize("V", [24, 1000, 50277, 65536])
def test_crafted_logits_through_the_hook(V):
    logits, tokens = _rows_for(V, 4321 + V)
    rows = logits.shape[0]
    ch, ids, lp = logprob_rows(logits, tokens, 20)
    # the ids: exactly the lexsort
    want = np.stack([top_ids(logits[r], 20) for r in range(rows)])
    assert np.array_equal(ids, want), [(r, ids[r].tolist(), want[r].tolist()) for r in range(rows) if not np.array_equal(ids[r], want[r])][:2]
    # chosen and every top log-prob: the scoring kernel's bits on the same row with that id as target
    sc, am = score_rows(logits, tokens)
    assert np.array_equal(bits(ch), bits(sc))
    some = np.array([np.any(logits[r] > -np.inf) for r in range(rows)])
    assert np.array_equal(ids[some, 0], am[some])        # top_ids[0] is the token k_argmax picks
    for k in range(20):
        valid = ids[:, k] != NO_TOKEN
        sk, _ = score_rows(logits, np.where(valid, ids[:, k], 0), want_argmax=False)
        assert np.array_equal(bits(lp[valid, k]), bits(sk[valid])), (V, k)
        assert np.all(np.isneginf(lp[~valid, k])), (V, k)
    # ... and within the derived tolerance of NumPy float64
    for r in range(rows):
        ref = f64_logprobs(logits[r], np.concatenate([[tokens[r]], ids[r]]))
        check_against_f64(ch[r], ref[0], ("chosen", V, r))
        for k in range(20):
            check_against_f64(lp[r, k], ref[1 + k], ("top", V, r, k))
    # every top_n is a prefix of the longest; chosen does not depend on it
    for n in (0, 1, 5):
        c2, i2, l2 = logprob_rows(logits, tokens, n)
        assert np.array_equal(bits(c2), bits(ch)) and np.array_equal(i2, ids[:, :n]) and np.array_equal(bits(l2), bits(lp[:, :n])), (V, n)
    # two runs are equal, and a row alone equals the same row among others
    c3, i3, l3 = logprob_rows(logits, tokens, 20)
    assert np.array_equal(bits(c3), bits(ch)) and np.array_equal(i3, ids) and np.array_equal(bits(l3), bits(lp))
    for r in (0, 12, rows - 5, rows - 1):
        c1, i1, l1 = logprob_rows(logits[r:r + 1], tokens[r:r + 1], 20)
        assert np.array_equal(bits(c1), bits(ch[r:r + 1])) and np.array_equal(i1[0], ids[r]) and np.array_equal(bits(l1[0]), bits(lp[r])), (V, r)


# ---- 2. / 3. end to end: the report of every call shape ----

def _batches(m, k):
    return [pkg.RWKVBatch(m, 3) for _ in range(k)]


def _same_slots(a, b, what):
    for s in SLOTS:
        assert np.array_equal(a.state_store(s), b.state_store(s)), (what, "state", s)


def _same_counters(a, b, what):
    """one more generator draw per slot from both (the report off in both by then): the draw counters decide it"""
    ta = a.eval_sample(SLOTS, [1, 2, 3], 1.0, 1.0, -1.0, SEEDS)
    tb = b.eval_sample(SLOTS, [1, 2, 3], 1.0, 1.0, -1.0, SEEDS)
    assert np.array_equal(ta, tb), (what, "draw counter")


def _check_loop(m, toks, rep, what, top_n=5):
    """the report of a loop that started from fresh slots with FIRST and emitted toks [3][steps], against score_ragged and eval on fresh copies"""
    chosen, ids, lps = rep
    steps = toks.shape[1]
    assert chosen.shape == (3, steps) and ids.shape == (3, steps, top_n) and lps.shape == (3, steps, top_n), what
    sc, ev = _batches(m, 2)
    fed = [[FIRST[r]] + toks[r, :-1].tolist() for r in range(3)]
    lp_rows, am_rows = sc.score_ragged(SLOTS, fed, [toks[r].tolist() for r in range(3)])
    for r in range(3):
        assert np.array_equal(bits(chosen[r]), bits(lp_rows[r])), (what, "chosen", r)
        assert np.array_equal(ids[r, :, 0], am_rows[r]), (what, "argmax", r)
    cur = list(FIRST)
    for i in range(steps):
        lg = ev.eval(SLOTS, cur)
        for r in range(3):
            assert np.array_equal(ids[r, i], top_ids(lg[r], top_n)), (what, "top ids", r, i)
            ref = f64_logprobs(lg[r], ids[r, i])
            for k in range(top_n):
                check_against_f64(lps[r, i, k], ref[k], (what, r, i, k))
        cur = toks[:, i].tolist()
    sc.free(); ev.free()


@pytest.mark.parametrize("version,fmt", GOLDEN)
def test_decode_sample_reports_what_score_ragged_scores(golden_dir, version, fmt):
    m = model(R.fixture_path(golden_dir, version, fmt))
    b, tw = _batches(m, 2)
    b.set_logprobs(5)
    toks, _ = b.decode_sample(SLOTS, FIRST, 8, 1.0, 0.9, SEEDS)
    plain, _ = tw.decode_sample(SLOTS, FIRST, 8, 1.0, 0.9, SEEDS)
    assert np.array_equal(toks, plain), (version, fmt)
    _same_slots(b, tw, (version, fmt))
    _check_loop(m, toks, b.logprobs(), (version, fmt))
    b.set_logprobs(enabled=False)
    _same_counters(b, tw, (version, fmt))
    b.free(); tw.free(); m.free()


SHAPES = [("6v0-3m", "Q5_1"), ("7v0-834K", "FP16")]


@pytest.mark.parametrize("version,fmt", SHAPES)
def test_the_greedy_and_the_penalised_loop(golden_dir, version, fmt):
    m = model(R.fixture_path(golden_dir, version, fmt))
    b, tw = _batches(m, 2)
    b.set_logprobs(5)
    toks, _ = b.decode_greedy(SLOTS, FIRST, 8)
    plain, _ = tw.decode_greedy(SLOTS, FIRST, 8)
    assert np.array_equal(toks, plain)
    _same_slots(b, tw, "greedy")
    rep = b.logprobs()
    assert np.array_equal(rep[1][:, :, 0], toks)          # the greedy token is the first alternative
    _check_loop(m, toks, rep, (version, fmt, "greedy"))
    b.free(); tw.free()
    # penalised: presence / frequency 0.5 and a bias; the report is still the model's distribution
    b, tw = _batches(m, 2)
    for x in (b, tw):
        x.set_logit_bias(1, {int(plain[1, 0]): -30.0, 7: 4.0})
    b.set_logprobs(5)
    toks, _ = b.decode_sample_penalized(SLOTS, FIRST, 8, 1.0, 0.9, SEEDS, 0.5, 0.5)
    ptoks, _ = tw.decode_sample_penalized(SLOTS, FIRST, 8, 1.0, 0.9, SEEDS, 0.5, 0.5)
    assert np.array_equal(toks, ptoks)
    _same_slots(b, tw, "penalised")
    for s in SLOTS:
        assert np.array_equal(b.counts(s), tw.counts(s)), s
    _check_loop(m, toks, b.logprobs(), (version, fmt, "penalised"))
    b.set_logprobs(enabled=False)
    _same_counters(b, tw, "penalised")
    b.free(); tw.free(); m.free()


@pytest.mark.parametrize("version,fmt", SHAPES)
def test_the_single_passes(golden_dir, version, fmt):
    m = model(R.fixture_path(golden_dir, version, fmt))
    V = m.n_vocab
    rng = np.random.default_rng(5)
    ragged = [rng.integers(0, V, size=n).tolist() for n in (1, 3, 33)]   # 33: the pass reaches the matrix-core path
    calls = {
        "eval_sample": lambda x: x.eval_sample(SLOTS, FIRST, 1.0, 0.9, [0.1, 0.5, 0.9], SEEDS, want_logits=True),
        "eval_sample_penalized": lambda x: x.eval_sample_penalized(SLOTS, FIRST, 1.0, 0.9, -1.0, SEEDS, 0.5, 0.5, True, want_logits=True),
        "eval_ragged_sample": lambda x: x.eval_ragged_sample(SLOTS, ragged, 1.0, 0.9, -1.0, SEEDS, want_logits=True),
        "eval_ragged_sample_penalized": lambda x: x.eval_ragged_sample_penalized(SLOTS, ragged, [1.0, 0.0, 1.0], 0.9, -1.0, SEEDS, 0.5, 0.5, True, want_logits=True),
    }
    for what, call in calls.items():
        b, tw = _batches(m, 2)
        if "penalized" in what:
            for x in (b, tw):
                x.counts_add(0, [3, 3, 9]); x.set_logit_bias(2, {5: 6.0})
        b.set_logprobs(5)
        tok, lg = call(b)
        ptok, plg = call(tw)
        assert np.array_equal(tok, ptok) and np.array_equal(lg, plg), what
        _same_slots(b, tw, what)
        chosen, ids, lps = b.logprobs()
        assert chosen.shape == (3, 1) and ids.shape == (3, 1, 5), what
        sc, _ = score_rows(lg, tok, want_argmax=False)
        assert np.array_equal(bits(chosen[:, 0]), bits(sc)), what
        for r in range(3):
            assert np.array_equal(ids[r, 0], top_ids(lg[r], 5)), (what, r)
            sk, _ = score_rows(np.repeat(lg[r:r + 1], 5, axis=0), ids[r, 0], want_argmax=False)
            assert np.array_equal(bits(lps[r, 0]), bits(sk)), (what, r)
        if "penalized" in what:
            for s in SLOTS:
                assert np.array_equal(b.counts(s), tw.counts(s)), (what, s)
        b.set_logprobs(enabled=False)
        _same_counters(b, tw, what)
        b.free(); tw.free()
    m.free()


@pytest.mark.parametrize("version,fmt", SHAPES)
def test_a_context_reports_what_a_batch_row_reports(golden_dir, version, fmt):
    m = model(R.fixture_path(golden_dir, version, fmt))
    tw = m.clone()
    b, = _batches(m, 1)
    b.set_logprobs(5)
    m.set_logprobs(5)
    # the sampled loop
    m.state_load(None); tw.state_load(None)
    toks, _ = m.decode_sample(FIRST[0], 8, 1.0, 0.9, SEEDS[0])
    plain, _ = tw.decode_sample(FIRST[0], 8, 1.0, 0.9, SEEDS[0])
    rows, _ = b.decode_sample([0], [FIRST[0]], 8, 1.0, 0.9, SEEDS[0])
    assert np.array_equal(toks, plain) and np.array_equal(toks, rows[0]) and np.array_equal(m.state_store(), tw.state_store())
    for mine, theirs in zip(m.logprobs(), b.logprobs()):
        assert mine.shape == theirs.shape and mine.shape[:2] == (1, 8) and np.array_equal(bits(mine), bits(theirs))
    # the penalised loop (it continues: counts and draw counters from where they are, in all three)
    for x in (m, tw):
        x.state_load(None); x.counts_reset(); x.rng_seek(0); x.set_logit_bias({9: 3.0})
    b.state_load(0); b.counts_reset(0); b.rng_seek(0, 0); b.set_logit_bias(0, {9: 3.0})
    toks, _ = m.decode_sample_penalized(FIRST[1], 8, 1.0, 0.9, SEEDS[1], 0.5, 0.5)
    plain, _ = tw.decode_sample_penalized(FIRST[1], 8, 1.0, 0.9, SEEDS[1], 0.5, 0.5)
    rows, _ = b.decode_sample_penalized([0], [FIRST[1]], 8, 1.0, 0.9, SEEDS[1], 0.5, 0.5)
    assert np.array_equal(toks, plain) and np.array_equal(toks, rows[0]) and np.array_equal(m.state_store(), tw.state_store())
    assert np.array_equal(m.counts(), tw.counts())
    for mine, theirs in zip(m.logprobs(), b.logprobs()):
        assert np.array_equal(bits(mine), bits(theirs))
    # one draw from the logits of the last evaluation, plain and penalised: the scoring kernel on those logits
    for pen in (False, True):
        lg = m.eval_resident([FIRST[2]]); tw.eval_resident([FIRST[2]])
        draw = (lambda x: x.sample_penalized(1.0, 0.9, 0.3, 0, 0.5, 0.5, True)) if pen else (lambda x: x.sample(1.0, 0.9, 0.3, 0))
        tok = draw(m)
        assert tok == draw(tw)
        chosen, ids, lps = m.logprobs()
        assert chosen.shape == (1, 1) and ids.shape == (1, 1, 5)
        sc, _ = score_rows(lg[None, :], [tok], want_argmax=False)
        assert bits(chosen)[0, 0] == bits(sc)[0] and np.array_equal(ids[0, 0], top_ids(lg, 5))
        sk, _ = score_rows(np.repeat(lg[None, :], 5, axis=0), ids[0, 0], want_argmax=False)
        assert np.array_equal(bits(lps[0, 0]), bits(sk))
        assert np.array_equal(m.logits_store(), lg)
    b.free(); tw.free(); m.free()


# ---- 4. rwkv_mi_batch_decode_until ----

@pytest.mark.parametrize("version,fmt", SHAPES)
def test_decode_until_reports_each_row_up_to_its_end(golden_dir, version, fmt):
    m = model(R.fixture_path(golden_dir, version, fmt))
    ref, = _batches(m, 1)
    plain, _ = ref.decode_sample(SLOTS, FIRST, 7, 1.0, 0.9, SEEDS)
    ref.free()
    stop_tok = int(plain[2, 2])                                   # row 2 stops at the first occurrence of its third token
    want_len = [1, 4, int(np.flatnonzero(plain[2] == stop_tok)[0]) + 1]
    results = []
    for block in (None, "2"):
        if block:
            os.environ["RWKV_MI_LOOP_BLOCK"] = block
        try:
            b, = _batches(m, 1)
            b.set_logprobs(5)
            outs, why, _ = b.decode_until(SLOTS, FIRST, [1, 4, 7], stop=[[], [], [[stop_tok]]], temperature=1.0, top_p=0.9, seed=SEEDS)
            rep = b.logprobs()
            passes = b.last_loop_passes()
            b.free()
        finally:
            os.environ.pop("RWKV_MI_LOOP_BLOCK", None)
        assert [len(o) for o in outs] == want_len and int(why[2]) == 0 and int(why[0]) == NO_TOKEN
        chosen, ids, lps = rep
        assert chosen.shape == (3, passes) and ids.shape == (3, passes, 5) and passes >= max(want_len)
        results.append((outs, chosen[:, :max(want_len)], ids[:, :max(want_len)], lps[:, :max(want_len)]))
        for r in range(3):
            L = want_len[r]
            # the plain loop of the row's own length, alone, in the same slot
            p, = _batches(m, 1)
            p.set_logprobs(5)
            ptoks, _ = p.decode_sample([r], [FIRST[r]], L, 1.0, 0.9, SEEDS[r])
            pc, pi, pl = p.logprobs()
            p.free()
            assert np.array_equal(outs[r], ptoks[0])
            assert np.array_equal(bits(chosen[r, :L]), bits(pc[0])) and np.array_equal(ids[r, :L], pi[0]) and np.array_equal(bits(lps[r, :L]), bits(pl[0])), r
            # the retiring step is there ...
            assert np.isfinite(chosen[r, L - 1]) and chosen[r, L - 1] <= 0.0 and ids[r, L - 1, 0] != NO_TOKEN, r
            # ... and behind it the fill values
            assert np.all(bits(chosen[r, L:]) == 0) and np.all(ids[r, L:] == NO_TOKEN) and np.all(np.isneginf(lps[r, L:])), r
    (o0, *a), (o1, *c) = results
    assert all(np.array_equal(x, y) for x, y in zip(o0, o1)) and all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, c))
    m.free()


# ---- 5. rejections and lifetime ----

def test_rejections_change_nothing(golden_dir, tmp_path):
    m = model(R.fixture_path(golden_dir, "6v0-3m", "Q5_1"))
    lib = m._library
    L = lib.library
    V = m.n_vocab
    b, tw = _batches(m, 2)
    rows, steps, top_n = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_uint32()
    buf = (ctypes.c_float * 64)()
    lib.rwkv_set_print_errors(m._ctx, False)

    def rejected(ok, what):
        assert not ok, what
        assert lib.rwkv_get_last_error(m._ctx) & ARGS, what

    # nothing reported yet: _shape and _store refuse
    b.set_logprobs(5)
    rejected(L.rwkv_mi_batch_logprobs_shape(b._ptr, ctypes.byref(rows), ctypes.byref(steps), ctypes.byref(top_n)), "shape before a call")
    rejected(L.rwkv_mi_batch_logprobs_store(b._ptr, 8, buf, None, None), "store before a call")
    toks, _ = b.decode_sample(SLOTS, FIRST, 4, 1.0, 0.9, SEEDS)
    tw.decode_sample(SLOTS, FIRST, 4, 1.0, 0.9, SEEDS)
    before = b.logprobs()
    states = [b.state_store(s) for s in SLOTS]

    def unchanged(what):
        for x, y in zip(b.logprobs(), before):
            assert np.array_equal(bits(x), bits(y)), what
        for s in SLOTS:
            assert np.array_equal(b.state_store(s), states[s]), what

    rejected(L.rwkv_mi_batch_set_logprobs(b._ptr, True, 21), "top_n above RWKV_MI_TOP_MAX")
    unchanged("top_n above RWKV_MI_TOP_MAX")
    rejected(L.rwkv_mi_batch_logprobs_store(b._ptr, 3, buf, None, None), "stride < steps")
    unchanged("stride < steps")
    bad = np.array([1, V, 3], dtype=np.uint32)
    sl = np.array(SLOTS, dtype=np.uint32)
    out = np.empty((3, 4), dtype=np.uint32)
    rejected(L.rwkv_mi_batch_decode_sample(b._ptr, sl.ctypes.data_as(P_UINT32), bad.ctypes.data_as(P_UINT32), 3, 4, pkg.sample_params(3, 1.0, 0.9), out.ctypes.data_as(P_UINT32), None),
             "a token >= n_vocab in an emitting call")
    unchanged("a token >= n_vocab in an emitting call")
    rejected(L.rwkv_mi_batch_eval_sample(b._ptr, sl.ctypes.data_as(P_UINT32), bad.ctypes.data_as(P_UINT32), 3, None, out.ctypes.data_as(P_UINT32), None), "params NULL")
    unchanged("params NULL")
    # the report is still the loop's (top_n still 5) after a call that emits nothing
    b.eval(SLOTS, toks[:, -1].tolist()); tw.eval(SLOTS, toks[:, -1].tolist())
    for x, y in zip(b.logprobs(), before):
        assert x.shape == y.shape and np.array_equal(bits(x), bits(y))
    # each output pointer of _store may be NULL
    assert L.rwkv_mi_batch_logprobs_store(b._ptr, 4, None, None, None)
    # off: a loop reports nothing, _store refuses; tokens, states and counters go on as in the twin all along
    b.set_logprobs(enabled=False)
    rejected(L.rwkv_mi_batch_logprobs_store(b._ptr, 8, buf, None, None), "store after set_logprobs")
    t1, _ = b.decode_greedy(SLOTS, [1, 2, 3], 3)
    t2, _ = tw.decode_greedy(SLOTS, [1, 2, 3], 3)
    assert np.array_equal(t1, t2)
    rejected(L.rwkv_mi_batch_logprobs_shape(b._ptr, ctypes.byref(rows), ctypes.byref(steps), ctypes.byref(top_n)), "shape with the report off")
    _same_slots(b, tw, "off")
    _same_counters(b, tw, "off")
    # the context: before a call, and a top_n out of range
    rejected(L.rwkv_mi_logprobs_store(m._ctx.ptr, 8, buf, None, None), "context store before a call")
    rejected(L.rwkv_mi_set_logprobs(m._ctx.ptr, True, 21), "context top_n")
    lib.rwkv_set_print_errors(m._ctx, True)
    b.free(); tw.free(); m.free()
    # a chain context has no report
    p = str(tmp_path / "m.bin")
    synth.write_model(p, synth.CONFIGS["test-v6"], "Q5_1", seed=3)
    os.environ["RWKV_MI_DEVICES"] = "0,0"
    try:
        c = model(p)
    finally:
        del os.environ["RWKV_MI_DEVICES"]
    lib.rwkv_set_print_errors(c._ctx, False)
    for what, ok in (("set", L.rwkv_mi_set_logprobs(c._ctx.ptr, True, 5)), ("store", L.rwkv_mi_logprobs_store(c._ctx.ptr, 8, buf, None, None)),
                     ("shape", L.rwkv_mi_logprobs_shape(c._ctx.ptr, None, None, None))):
        assert not ok, what
    assert lib.rwkv_get_last_error(c._ctx) & ARGS
    lib.rwkv_set_print_errors(c._ctx, True)
    c.free()
