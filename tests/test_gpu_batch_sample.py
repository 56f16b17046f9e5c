"""Sampling in batched decode (rwkv_mi_batch_eval_sample / _decode_sample / _rng_seek, csrc/sampling.hip k_draw_rows<plain, 0, 0>): every row is pinned
to the single-context sampler (rwkv_mi_sample / rwkv_mi_decode_sample on a context that steps that sequence alone), and both entry points of
the kernel to the float64 restatement of the reference's sample_probs (test_gpu_sampling.ref_distribution). Tokens, states and draw counters
are compared exactly."""
import ctypes

import numpy as np
import pytest

import oracle_lib as O
import reference_constants as R
from gpu_lib import library, model, pkg, synth
from test_gpu_batch import _tok
from test_gpu_sampling import ref_distribution

pytestmark = pytest.mark.gpu

ARGS = 1 << 8   # RWKV_ERROR_ARGS
TEMPERATURES = (0.0, 0.3, 0.7, 1.0, 1.5)
TOP_PS = (0.0, 0.5, 0.8, 0.95, 1.0)
SUBSETS = ([3, 0, 5], [1], [5, 2, 4, 0, 1, 3], [2, 4], [4, 2], [0, 5, 1])
BAD_CALLS = lambda V: [([1, 1], [3, 4]), ([6], [3]), ([0, 9], [1, 2]), ([2], [V]), ([], []), (list(range(6)) + [0], [1] * 7)]   # noqa: E731


def _synth(tmp_path, name, fmt, seed=7):
    library()
    p = str(tmp_path / f"{name}-{fmt}.bin")
    synth.write_model(p, synth.CONFIGS[name], fmt, seed=seed)
    return p


def _row_params(i, n):
    """(temperature, top_p, seed) of row i of an n-row call: the 25 pairs in an order that depends on n (7 is coprime to 25: rows
    0 .. 24 are all different pairs); from row 25 on a pair comes back with another seed."""
    k = (7 * i + n) % 25
    return TEMPERATURES[k % 5], TOP_PS[k // 5], 1000 + 17 * i


@pytest.mark.parametrize("name,fmt", [("test-v6", "Q5_1"), ("test-v7", "Q5_1"), ("test-v4", "Q8_0"), ("mega-v6-2048-v64k", "Q4_0")])
def test_sampling_loop_rows_equal_the_sequence_alone(tmp_path, name, fmt):
    p = _synth(tmp_path, name, fmt, seed=9)
    m = model(p)
    V = m.n_vocab
    b = pkg.RWKVBatch(m, 33)
    for n in (1, 4, 33):
        slots = list(range(n))[::-1]
        for s in slots:
            b.state_load(s, None)
        b.eval(slots, [_tok(1, s, V) for s in slots], want_logits=False)   # every slot from its own state
        start = {s: b.state_store(s) for s in slots}
        first = [_tok(2, s, V) for s in slots]
        params = [_row_params(i, n) for i in range(n)]
        assert len(set(params)) == n
        toks, ms = b.decode_sample(slots, first, 16, [q[0] for q in params], [q[1] for q in params], [q[2] for q in params])
        assert toks.shape == (n, 16) and ms > 0.0
        for i, s in enumerate(slots):
            m.state_load(start[s])
            ref, _ = m.decode_sample(first[i], 16, *params[i])
            assert np.array_equal(toks[i], ref), (name, fmt, n, s, params[i], list(toks[i]), list(ref))
            assert np.array_equal(b.state_store(s), m.state_store()), (name, fmt, n, s)
            if params[i][0] == 0.0:
                m.state_load(start[s])
                g, _ = m.decode_greedy(first[i], 16)
                assert np.array_equal(toks[i], g), (name, fmt, n, s, "temperature 0 is the argmax")
    # the seeds reach the rows: the same state, first token, temperature and top-p in four slots, two seeds
    for s in range(4):
        b.state_load(s, start[0])
    toks, _ = b.decode_sample([0, 1, 2, 3], [first[-1]] * 4, 16, 1.0, 1.0, [5, 6, 5, 6])
    assert np.array_equal(toks[0], toks[2]) and np.array_equal(toks[1], toks[3]), (name, fmt)
    assert not np.array_equal(toks[0], toks[1]), (name, fmt, list(toks[0]))
    b.free()
    m.free()


def test_steps_equal_the_sequence_alone_and_the_counter_belongs_to_the_slot(golden_dir):
    path = R.fixture_path(golden_dir, "6v0-3m", "Q5_0")
    m = model(path)
    b = pkg.RWKVBatch(m, 6)
    temperature = [1.0, 0.7, 1.5, 0.3, 1.0, 0.7]
    top_p = [0.8, 0.95, 1.0, 0.5, 0.0, 0.8]
    seed = [100 + s for s in range(6)]
    ctx = {s: m.clone() for s in range(6)}       # a fresh context per slot: its own draw counter, from 0
    cst = {s: None for s in range(6)}            # that sequence's state, stepped alone through rwkv_eval
    fed = {s: [] for s in range(6)}
    drawn = {s: [] for s in range(6)}

    def alone(s, tok):
        _, cst[s] = ctx[s].eval(tok, cst[s])
        return ctx[s].sample(temperature[s], top_p[s], -1.0, seed[s])

    for step, slots in enumerate(SUBSETS):
        before = {s: b.state_store(s) for s in range(6)}
        toks = [_tok(step, s, 128) for s in slots]
        out = b.eval_sample(slots, toks, [temperature[s] for s in slots], [top_p[s] for s in slots], -1.0, [seed[s] for s in slots])
        for i, s in enumerate(slots):
            ref = alone(s, toks[i])
            assert int(out[i]) == ref, (step, slots, s, int(out[i]), ref)
            fed[s].append(toks[i])
            drawn[s].append(int(out[i]))
        for s in range(6):
            after = b.state_store(s)
            assert np.array_equal(after, cst[s] if s in slots else before[s]), (step, s)
    # rng_seek(slot, 0), the same steps from the same state: the same tokens
    keep = b.state_store(5)
    b.state_load(5, None)
    b.rng_seek(5, 0)
    again = [int(b.eval_sample([5], [t], temperature[5], top_p[5], -1.0, seed[5])[0]) for t in fed[5]]
    assert again == drawn[5] and len(again) == 3, (again, drawn[5])
    assert np.array_equal(b.state_store(5), keep)
    # ... and seeking to a recorded count resumes there: the third draw alone
    b.state_load(5, None)
    for t in fed[5][:2]:
        b.eval([5], [t], want_logits=False)
    b.rng_seek(5, 2)
    assert int(b.eval_sample([5], [fed[5][2]], temperature[5], top_p[5], -1.0, seed[5])[0]) == drawn[5][2]
    # decode_sample after eval_sample calls gives what it gives on a fresh batch
    twin = pkg.RWKVBatch(m, 6)
    for s in (1, 3):
        twin.state_load(s, b.state_store(s))
    args = ([3, 1], [7, 9], 8, [temperature[3], temperature[1]], [top_p[3], top_p[1]], [seed[3], seed[1]])
    got, _ = b.decode_sample(*args)
    want, _ = twin.decode_sample(*args)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    for s in (1, 3):
        assert np.array_equal(b.state_store(s), twin.state_store(s)), s
    # ... and a slot it did not name continues its stream where it was
    for s in (0, 2):
        out = b.eval_sample([s], [11 + s], temperature[s], top_p[s], -1.0, seed[s])
        assert int(out[0]) == alone(s, 11 + s), s
    twin.free()
    b.free()
    for c in ctx.values():
        c.free()
    m.free()


def test_rejected_calls_change_nothing(golden_dir):
    path = R.fixture_path(golden_dir, "6v0-3m", "Q5_0")
    m = model(path)
    V = m.n_vocab
    b, twin = pkg.RWKVBatch(m, 6), pkg.RWKVBatch(m, 6)
    good = dict(temperature=[1.0, 0.7, 1.5, 0.3, 1.0, 0.7], top_p=[0.8, 0.95, 1.0, 0.5, 0.0, 0.8], u=-1.0, seed=[3, 4, 5, 6, 7, 8])
    slots6, toks6 = [5, 2, 4, 0, 1, 3], [_tok(0, s, 128) for s in range(6)]
    first = b.eval_sample(slots6, toks6, **good)
    assert np.array_equal(first, twin.eval_sample(slots6, toks6, **good))
    snapshot = {s: b.state_store(s) for s in range(6)}
    nan = float("nan")
    bad = [(sl, tk, {}) for sl, tk in BAD_CALLS(V)]
    bad += [([0, 1], [3, 4], kw) for kw in (dict(temperature=-1.0), dict(temperature=[1.0, -1.0]), dict(top_p=1.5), dict(top_p=[0.5, -0.1]),
                                           dict(temperature=nan), dict(top_p=[0.5, nan]))]
    bad_u = [([0, 1], [3, 4], kw) for kw in (dict(u=1.0), dict(u=[0.5, 1.5]), dict(u=[nan, 0.5]))]
    for sl, tk, kw in bad + bad_u:
        a = dict(temperature=1.0, top_p=0.8, u=-1.0, seed=1)
        a.update(kw)
        b.last_error = 0
        with pytest.raises(ValueError):
            b.eval_sample(sl, tk, **a)
        assert b.last_error & ARGS, (sl, tk, kw, b.last_error)
    for sl, tk, kw in bad:   # (the loop takes no u: the generator draws)
        a = dict(temperature=1.0, top_p=0.8, seed=1)
        a.update(kw)
        b.last_error = 0
        with pytest.raises(ValueError):
            b.decode_sample(sl, tk, 3, **a)
        assert b.last_error & ARGS, (sl, tk, kw, b.last_error)
    for s in range(6):
        assert np.array_equal(b.state_store(s), snapshot[s]), ("a rejected call changed a slot", s)
    # no parity and no draw counter moved either: the next valid calls return what a batch that never saw the bad ones returns
    nxt = [int(t) % 128 for t in first]
    assert np.array_equal(b.eval_sample(slots6, nxt, **good), twin.eval_sample(slots6, nxt, **good))
    la, _ = b.decode_sample([4, 1], [9, 10], 5, 1.0, 0.9, [21, 22])
    lb, _ = twin.decode_sample([4, 1], [9, 10], 5, 1.0, 0.9, [21, 22])
    assert np.array_equal(la, lb)
    for s in range(6):
        assert np.array_equal(b.state_store(s), twin.state_store(s)), s
    b.free()
    twin.free()
    m.free()


# ---- both entry points of the kernel on crafted logits (the test hook) ----

_sample_hooks = None


def _sample_hooks_library():
    """lib/librwkv_testhooks_sample.so: the product objects + the sampler's test entry point (include/rwkv_testhooks_sample.h)."""
    global _sample_hooks
    if _sample_hooks is None:
        library()   # (builds; and HIP is initialised in the order gpu_lib keeps)
        _sample_hooks = pkg.RWKVSharedLibrary(pkg.SAMPLE_HOOKS_LIB_PATH)
    return _sample_hooks


def _sample_rows(logits, params, counters, rows_kernel):
    L = _sample_hooks_library().library
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    n_rows, n_vocab = logits.shape
    ctr = None if counters is None else np.ascontiguousarray(counters, dtype=np.uint64).copy()
    out = np.empty(n_rows, dtype=np.uint32)
    ok = L.rwkv_mi_test_sample_rows(logits.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), n_rows, n_vocab, params,
                                    None if ctr is None else ctr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), rows_kernel,
                                    out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    assert ok, "rwkv_mi_test_sample_rows failed"
    return out, ctr


def _descending_cumsum(logits):
    x = logits.astype(np.float64)
    e = np.exp(x - x.max())
    return np.cumsum(np.sort(e / e.sum())[::-1])


def _top_p_clear_of_the_cumsums(logits, target):
    """A top_p (as the float32 the kernel receives) near `target` that lies in the middle of a gap of the reference's descending cumulative
    sums wide enough for the condition below: from the gap that holds the target towards the larger probabilities, the first such gap."""
    cum = np.concatenate([[0.0], _descending_cumsum(logits)])
    k = int(np.searchsorted(cum, target))
    while k > 0:
        if cum[k] - cum[k - 1] > 4e-5:
            return float(np.float32(0.5 * (cum[k] + cum[k - 1])))
        k -= 1
    raise AssertionError("no gap of the cumulative sums is wide enough")


def _crafted_rows(V, rng):
    """8 rows of logits and (temperature, top_p) of each."""
    g = lambda scale: (rng.standard_normal(V) * scale).astype(np.float32)   # noqa: E731
    rows = [g(1.0), g(4.0)]
    spike = g(1.0); spike[V // 3] = spike.max() + 30.0
    rows.append(spike)
    twins = g(1.0); twins[V // 5] = twins[(4 * V) // 5] = twins.max() + 1.0       # two exactly equal maxima: the argmax rule (first index)
    rows.append(twins)
    rows.append(np.full(V, 0.25, dtype=np.float32))
    holes = g(1.0); holes[rng.random(V) < 0.5] = -np.inf
    rows.append(holes)
    twins4 = g(4.0); twins4[V // 7] = twins4[(6 * V) // 7] = twins4.max() + 0.5    # ... and as two equally likely draws
    rows.append(twins4)
    rows.append(g(4.0))
    logits = np.stack(rows)
    # (all equal: the cumulative sums are k / V, 1.5e-5 apart at 65 536 -- no top_p below 1 is clear of them there)
    params = [(1.0, _top_p_clear_of_the_cumsums(rows[0], 0.3)), (0.7, _top_p_clear_of_the_cumsums(rows[1], 0.8)),
              (1.5, _top_p_clear_of_the_cumsums(rows[2], 0.9)), (0.0, 0.0),
              (1.0, 0.8005 if V == 1000 else 1.0), (0.3, _top_p_clear_of_the_cumsums(rows[5], 0.5)),
              (1.0, 1.0), (1.5, 0.0)]
    return logits, params


@pytest.mark.parametrize("V", [1000, 50277, 65536])
def test_both_entry_points_on_crafted_logits(V):
    rng = np.random.default_rng(V)
    logits, params = _crafted_rows(V, rng)
    # condition on the inputs, on the reference alone: where top_p cuts, no descending cumulative sum lies within 1e-5 of it
    for r, (t, p) in enumerate(params):
        if 0.0 < p < 1.0:
            d = float(np.abs(_descending_cumsum(logits[r]) - p).min())
            assert d > 1e-5, (V, r, p, d)
    ref = [ref_distribution(logits[r], t, p) for r, (t, p) in enumerate(params)]
    cdf = [np.cumsum(pr) for pr in ref]
    T, P = [q[0] for q in params], [q[1] for q in params]
    for u in np.linspace(0.001, 0.999, 41):
        table = pkg.sample_params(8, T, P, float(u), 0)
        ctr_in = np.arange(8, dtype=np.uint64) * 3
        rows, rows_ctr = _sample_rows(logits, table, ctr_in, 1)
        one, one_ctr = _sample_rows(logits, table, ctr_in, 0)
        assert np.array_equal(rows, one), (V, u, rows.tolist(), one.tolist())
        assert np.array_equal(rows_ctr, one_ctr), (V, u)
        for r in range(8):
            tok, pr = int(rows[r]), ref[r]
            assert tok < V and pr[tok] > 0.0, (V, r, params[r], u, tok)
            lo = cdf[r][tok] - pr[tok]
            assert lo - 1e-4 <= u <= cdf[r][tok] + 1e-4, (V, r, params[r], u, tok, lo, cdf[r][tok])
    # the generator: each row draws with its own seed and counter; a draw that is not an argmax advances the counter by one
    table = pkg.sample_params(8, T, P, -1.0, [40 + r for r in range(8)])
    ctr_in = np.array([0, 1, 2, 3, 4, 5, 1 << 33, 7], dtype=np.uint64)
    rows, rows_ctr = _sample_rows(logits, table, ctr_in, 1)
    one, one_ctr = _sample_rows(logits, table, ctr_in, 0)
    assert np.array_equal(rows, one) and np.array_equal(rows_ctr, one_ctr), (V, rows.tolist(), one.tolist())
    assert np.array_equal(rows_ctr, ctr_in + np.array([t != 0.0 for t in T], dtype=np.uint64)), (V, rows_ctr.tolist())
    assert all(ref[r][int(rows[r])] > 0.0 for r in range(8))
    none, _ = _sample_rows(logits, table, None, 1)   # counters == NULL: zero
    zero, _ = _sample_rows(logits, table, np.zeros(8, dtype=np.uint64), 0)
    assert np.array_equal(none, zero)


def test_logits_on_request(golden_dir):
    path = R.fixture_path(golden_dir, "6v0-3m", "Q5_0")
    m = model(path)
    b, twin = pkg.RWKVBatch(m, 4), pkg.RWKVBatch(m, 4)
    slots = [2, 0, 3]
    T, P, U = [0.7, 1.0, 0.0], [0.5, 0.95, 0.8], [0.11, 0.62, 0.97]
    states = {s: None for s in slots}
    for step in range(3):
        toks = [_tok(step, s, 128) for s in slots]
        out, lg = b.eval_sample(slots, toks, T, P, U, 0, want_logits=True)
        assert lg.shape == (3, m.n_vocab) and out.shape == (3,)
        assert np.array_equal(lg, twin.eval(slots, toks)), step
        for i, s in enumerate(slots):
            cl, states[s] = m.eval(toks[i], states[s])
            assert np.array_equal(lg[i], cl), (step, s)
            assert int(out[i]) == m.sample(T[i], P[i], U[i]), (step, s)
    assert b.eval_sample([1], [5], 1.0, 0.8, 0.5).shape == (1,)   # (without the logits: the tokens alone)
    b.free()
    twin.free()
    m.free()


def test_sampling_next_to_persistent_kernel(tmp_path, monkeypatch):
    monkeypatch.setenv("RWKV_MI_NO_AUTOTUNE", "1")
    p = _synth(tmp_path, "mega-v6-4096", "Q4_0", seed=21)
    m = model(p)
    assert m.decode_path() == 2, m.persist_info()
    om = O.OracleModel(p)
    V = m.n_vocab
    b = pkg.RWKVBatch(m, 8)
    slots = list(range(8))
    T = [0.0, 0.3, 0.7, 1.0, 1.5, 0.0, 1.0, 0.7]
    ost = {s: om.init_state() for s in slots}
    cst, tok = om.init_state(), 3
    for rnd in range(3):
        toks, _ = m.decode_greedy(tok, 4)
        ref = []
        for _ in range(4):
            ol, cst = om.eval(tok, cst)
            tok = int(np.argmax(ol))
            ref.append(tok)
        assert list(toks) == ref, (rnd, list(toks), ref)
        fed = [_tok(rnd, s, V) for s in slots]
        out, lg = b.eval_sample(slots, fed, T, 0.9, -1.0, [s + 1 for s in slots], want_logits=True)
        for i, s in enumerate(slots):
            ol, ost[s] = om.eval(fed[i], ost[s])
            assert np.array_equal(lg[i], ol), ("beside path 2", rnd, s)
            assert int(out[i]) < V
            if T[i] == 0.0:
                assert int(out[i]) == int(np.argmax(ol)), (rnd, s)
        assert m.healthy()
    assert np.array_equal(m.state_store(), cst)
    assert m.decode_path() == 2 and m.healthy()
    b.free()
    m.free()
    om.free()
