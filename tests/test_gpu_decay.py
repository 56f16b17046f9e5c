"""Penalty decay and repetition penalty in the device sampler (rwkv_mi_*repetition_set, csrc/sampling.hip RepetitionLogits / the SRC_REP forms of k_draw, k_draw_rows and the draft walk): the
draw is held, bit for bit, to the existing sampler on logits adjusted on the host by tests/decay_ref.py, the occurrence row to decay_ref's as
uint32 bit patterns; "none" to the calls without a setting; every device loop to the host-driven loop of single steps; every caller to the
plain loop. No tolerance anywhere: the new draw is the existing sampler on adjusted values."""
import ctypes
import os

import numpy as np
import pytest

import cut_ref as C
import decay_ref as D
import reference_constants as R
from gpu_lib import library, model, pkg, synth
from test_gpu_batch import _tok
from test_gpu_batch_sample import _sample_rows

pytestmark = pytest.mark.gpu

ARGS = 1 << 8   # RWKV_ERROR_ARGS
F = np.float32
P_F, P_U32, P_U64 = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)

_decay_hooks = None


def _hooks():
    """lib/librwkv_testhooks_decay.so: the product objects + the test entry points of include/rwkv_testhooks_decay.h."""
    global _decay_hooks
    if _decay_hooks is None:
        library()   # (builds; and HIP is initialised in the order gpu_lib keeps)
        _decay_hooks = pkg.RWKVSharedLibrary(pkg.DECAY_HOOKS_LIB_PATH)
    return _decay_hooks.library


def _decay_rows(logits, params, pens, reps, occ, bias, counters, rows_kernel):
    """the hook: (tokens, counters, occurrence rows afterwards)"""
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    n_rows, n_vocab = logits.shape
    table = (pkg.RepParams * n_rows)(*[pkg.RepParams(float(d), float(r)) for d, r in reps])
    occ = np.ascontiguousarray(occ, dtype=np.uint32).copy()
    bias = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
    ctr = None if counters is None else np.ascontiguousarray(counters, dtype=np.uint64).copy()
    out = np.empty(n_rows, dtype=np.uint32)
    ok = _hooks().rwkv_mi_test_decay_rows(logits.ctypes.data_as(P_F), n_rows, n_vocab, params, pens, table, occ.ctypes.data_as(P_U32),
                                          None if bias is None else bias.ctypes.data_as(P_F), None if ctr is None else ctr.ctypes.data_as(P_U64),
                                          rows_kernel, out.ctypes.data_as(P_U32))
    assert ok, "rwkv_mi_test_decay_rows failed"
    return out, ctr, occ


def _hook_counts_add(occ_f32, tokens, decay):
    occ = np.ascontiguousarray(occ_f32, dtype=np.float32).copy()
    t = np.ascontiguousarray(tokens, dtype=np.uint32)
    assert _hooks().rwkv_mi_test_decay_counts_add(occ.ctypes.data_as(P_F), occ.size, t.ctypes.data_as(P_U32), t.size, float(decay))
    return occ


# ---- 1. source and sweep ----

DECAYS = (1.0, 0.996, 0.5, 0.0)
REPS = (1.0, 1.1, 2.0)
PENS = ((0.0, 0.0), (0.2, 0.2))
SUBNORMAL = np.array([1], dtype=np.uint32).view(np.float32)[0]   # 2^-149


def _matrix(V):
    """One row per (decay, repetition, penalties, record, occurrence kind): logits with positive, negative, zero and -inf values at occurred
    tokens; occurrence rows all zero or crafted -- integers, fractions, the smallest subnormal and 2^24 on a decaying row, counts up to 2^24 on
    any other. The occurred tokens lie in the first, a middle and the last thread chunk."""
    rng = np.random.default_rng(V + 1)
    base = [(rng.standard_normal(V) * s).astype(np.float32) for s in (1.0, 2.0, 4.0, 1.0)]
    C_ = -(-V // 1024)
    at = np.unique(np.concatenate([np.arange(0, 12), rng.choice(V, 40, replace=False), np.arange(V - 12, V), [C_ - 1, C_, 7 * C_ + 1]]) % V)
    rows = []
    for decay in DECAYS:
        for rep in REPS:
            for pen in PENS:
                for record in (0, 1):
                    for crafted in (0, 1):
                        rows.append((decay, rep, pen, record, crafted))
    n = len(rows)
    logits = np.empty((n, V), dtype=np.float32)
    occ = np.zeros((n, V), dtype=np.uint32)
    T, P = [], []
    for r, (decay, rep, pen, record, crafted) in enumerate(rows):
        lg = base[r % 4].copy()
        kinds = rng.integers(0, 4, at.size)
        lg[at[kinds == 0]] = np.abs(lg[at[kinds == 0]]) + F(0.5)     # positive: divided
        lg[at[kinds == 1]] = -np.abs(lg[at[kinds == 1]]) - F(0.5)    # negative: multiplied
        lg[at[kinds == 2]] = F(0.0)
        lg[at[kinds == 3]] = -np.inf
        lg[at[0]] = lg.max() + F(3.0)                                # a likely token that has occurred: the penalty moves the draw
        logits[r] = lg
        if crafted:
            if D.is_decaying(decay):
                o = np.zeros(V, dtype=np.float32)
                vals = np.array([1.0, 2.0, 7.0, 0.996, 0.5, 1.984063, 3.25e-3, SUBNORMAL, 16777216.0], dtype=np.float32)
                o[at] = vals[np.arange(at.size) % vals.size]
                occ[r] = D.words_of(o)
            else:
                vals = np.array([1, 2, 7, 1, 3, 40, 1 << 24], dtype=np.uint32)
                occ[r][at] = vals[np.arange(at.size) % vals.size]
        T.append((1.0, 0.7, 0.0, 1.3)[(r // 2) % 4])
        P.append((1.0, 0.9, 0.0, 0.5)[(r // 8) % 4])
    bias = (rng.standard_normal((n, V)) * 0.5).astype(np.float32)
    bias[:, at[1]] = -np.inf   # (a forbidden token among the occurred ones)
    return rows, logits, occ, bias, T, P, at


@pytest.mark.parametrize("V", [1000, 50277, 65536])
def test_source_and_sweep_against_the_reference(V):
    rows, logits, occ, bias, T, P, at = _matrix(V)
    n = len(rows)
    assert n == 96 and any(t == 0.0 for t in T)
    reps = [(r[0], r[1]) for r in rows]
    pens = pkg.penalty_params(n, [r[2][0] for r in rows], [r[2][1] for r in rows], [bool(r[3]) for r in rows])
    ctr_in = np.arange(n, dtype=np.uint64) * 3 + 1
    for b in (None, bias):
        adj = np.stack([D.adjusted(logits[r], occ[r], rows[r][2][0], rows[r][2][1], rows[r][0], rows[r][1], None if b is None else b[r]) for r in range(n)])
        # the matrix does what it is for: a repetition penalty changes what is read at the occurred tokens of a crafted row, and nowhere else
        for r in range(n):
            if b is None and rows[r][4] and rows[r][1] != 1.0:
                moved = adj[r].view(np.uint32) != logits[r].view(np.uint32)
                assert moved[at].any() and not np.delete(moved, at).any(), r
        for form in (1, 0):
            for u in (-1.0, 0.001, 0.37, 0.999):
                table = pkg.sample_params(n, T, P, float(u), [50 + r for r in range(n)])
                got, got_ctr, occ_out = _decay_rows(logits, table, pens, reps, occ, b, ctr_in, form)
                ref, ref_ctr = _sample_rows(adj, table, ctr_in, form)
                assert np.array_equal(got, ref), (V, b is not None, form, u, np.flatnonzero(got != ref).tolist())
                assert np.array_equal(got_ctr, ref_ctr), (V, form, u)
                for r in range(n):
                    want = D.recorded(occ[r], rows[r][0], int(got[r]), bool(rows[r][3]))
                    assert np.array_equal(occ_out[r], want), (V, form, u, r, rows[r], np.flatnonzero(occ_out[r] != want)[:8].tolist())


# ---- 3. underflow ----

def test_two_hundred_halvings_pass_through_the_subnormals_to_zero():
    V = 1000
    rng = np.random.default_rng(3)
    tokens = np.concatenate([[5, 6, 7, 999], rng.integers(100, 900, 196)]).astype(np.uint32)   # 5, 6, 7 and 999 never come again
    start = np.zeros(V, dtype=np.float32)
    got = _hook_counts_add(start, tokens, 0.5)
    want = D.counts_add(np.zeros(V, dtype=np.uint32), 0.5, tokens)
    assert np.array_equal(got.view(np.uint32), want), np.flatnonzero(got.view(np.uint32) != want).tolist()
    # the four first tokens have been halved 199 .. 196 times: 0; and every partial run passes through the subnormals exactly as NumPy does
    assert (got[[5, 6, 7, 999]] == 0.0).all() and (got[tokens[-3:]] > 0).all()
    for n in (127, 140, 149, 150, 151):
        part = _hook_counts_add(start, tokens[:n], 0.5)
        ref = D.counts_add(np.zeros(V, dtype=np.uint32), 0.5, tokens[:n])
        assert np.array_equal(part.view(np.uint32), ref), n
    part = _hook_counts_add(start, tokens[:150], 0.5).view(np.uint32)
    assert part[5] == 1 and part[6] == 2, "2^-149 and 2^-148: subnormals are kept"
    # the draw that follows takes no presence penalty where the entry reached 0: token 5 leads by 0.1, a penalty of 0.5 would hand the
    # argmax to token 3, which has not occurred
    lg = np.full((1, V), -4.0, dtype=np.float32)
    lg[0, 5], lg[0, 3] = 5.0, 4.9
    pens = pkg.penalty_params(1, 0.5, 0.5, True)
    for form in (1, 0):
        tok, _, occ_out = _decay_rows(lg, pkg.sample_params(1, 0.0, 1.0, 0.5, 0), pens, [(0.5, 1.0)], want[None, :], None, None, form)
        assert int(tok[0]) == 5, (form, tok)
        assert np.array_equal(occ_out[0], D.recorded(want, 0.5, 5))
    # ... while an entry that is still subnormal is an occurrence: the same draw on the row of 150 tokens goes to token 3
    tok, _, _ = _decay_rows(lg, pkg.sample_params(1, 0.0, 1.0, 0.5, 0), pens, [(0.5, 1.0)], part[None, :], None, None, 1)
    assert int(tok[0]) == 3


# ---- helpers of the model tests ----

SETTINGS = [(1.0, 1.0), (0.996, 1.0), (1.0, 1.1), (0.9, 1.3)]   # slot s: none, decay only, repetition only, both
T4, P4, SEEDS = [1.0, 0.8, 1.3, 1.0], [1.0, 0.9, 0.95, 0.5], [11, 12, 13, 14]
PRES, FREQ = 0.4, 0.3


def _table(x, s):
    """the slot's occurrence row as words, whichever kind it is"""
    d, _ = x.repetition(s)
    return x.counts_f32(s).view(np.uint32) if D.is_decaying(d) else x.counts(s)


def _fresh(b, slots, V, salt, settings=SETTINGS):
    """every named slot from a state of its own, its setting, its draw counter at 0, its table empty; the states"""
    for s in slots:
        b.state_load(s, None)
        b.set_repetition(s, *settings[s])
    b.eval(slots, [_tok(salt, s, V) for s in slots], want_logits=False)
    for s in slots:
        b.rng_seek(s, 0)
        b.counts_reset(s)
    return {s: b.state_store(s) for s in slots}


def _like(twin, b, slots, states, settings=SETTINGS):
    for s in slots:
        twin.state_load(s, states[s])
        twin.set_repetition(s, *settings[s])
        twin.rng_seek(s, 0)
        twin.counts_reset(s)


def _steps(b, slots, first, n, T, P, seeds):
    """n single penalised passes with the generator drawing and every step recorded: tokens [len(slots)][n]"""
    out = np.empty((len(slots), n), dtype=np.uint32)
    feed = list(first)
    for j in range(n):
        got = b.eval_sample_penalized(slots, feed, T, P, -1.0, seeds, PRES, FREQ, True)
        out[:, j] = got
        feed = [int(t) for t in got]
    return out


def _host_loop(b, slots, first, n, settings, bias):
    """The host-driven loop: per token one eval, decay_ref on the downloaded logits, the PLAIN sampler (the sample hook, the generator drawing
    from the host's counters), decay_ref on the host's tables. Returns (tokens [len(slots)][n], tables, counters)."""
    V = b._n_vocab
    tables = [np.zeros(V, dtype=np.uint32) for _ in slots]
    ctr = np.zeros(len(slots), dtype=np.uint64)
    out = np.empty((len(slots), n), dtype=np.uint32)
    feed = list(first)
    params = pkg.sample_params(len(slots), T4, P4, -1.0, SEEDS)
    for j in range(n):
        lg = b.eval(slots, feed)
        adj = np.stack([D.adjusted(lg[i], tables[i], PRES, FREQ, settings[s][0], settings[s][1], bias.get(s)) for i, s in enumerate(slots)])
        got, ctr = _sample_rows(adj, params, ctr, 1)
        for i, s in enumerate(slots):
            tables[i] = D.recorded(tables[i], settings[s][0], int(got[i]))
        out[:, j] = got
        feed = [int(t) for t in got]
    return out, tables, ctr


# ---- 4. loops ----

@pytest.mark.parametrize("version,fmt", [("4v0-660K", "Q5_0"), ("6v0-3m", "Q5_0"), ("7v0-834K", "Q5_0")])
def test_penalised_loop_is_the_host_driven_loop(golden_dir, version, fmt):
    m = model(R.fixture_path(golden_dir, version, fmt))
    V = m.n_vocab
    b, twin = pkg.RWKVBatch(m, 4), pkg.RWKVBatch(m, 4)
    slots = [2, 0, 3, 1]
    first = [_tok(2, s, V) for s in slots]
    bias_row = np.zeros(V, dtype=np.float32)
    bias_row[[3, 17]] = [-np.inf, 1.5]
    bias = {3: bias_row}
    st = _fresh(b, slots, V, 1)
    _like(twin, b, slots, st)
    for x in (b, twin):
        x.set_logit_bias(3, {3: -np.inf, 17: 1.5})
    loop, _ = b.decode_sample_penalized(slots, first, 24, T4, P4, SEEDS, PRES, FREQ)
    host, tables, ctr = _host_loop(twin, slots, first, 24, SETTINGS, bias)
    assert np.array_equal(loop, host), (version, loop.tolist(), host.tolist())
    for i, s in enumerate(slots):
        assert np.array_equal(b.state_store(s), twin.state_store(s)), (version, s)
        assert np.array_equal(_table(b, s), tables[i]), (version, s, SETTINGS[s])
    # the settings act: the decayed tables differ from counts, and at least one row's tokens from the loop without settings
    assert not np.array_equal(D.occurrences(tables[slots.index(1)], 0.996), np.round(D.occurrences(tables[slots.index(1)], 0.996)))
    # the draw counters: one more draw from the same logits agrees with the host's counters
    nxt = [int(t) for t in loop[:, -1]]
    more = b.eval_sample_penalized(slots, nxt, T4, P4, -1.0, SEEDS, PRES, FREQ, False, want_logits=True)
    adj = np.stack([D.adjusted(more[1][i], tables[i], PRES, FREQ, SETTINGS[s][0], SETTINGS[s][1], bias.get(s)) for i, s in enumerate(slots)])
    ref, _ = _sample_rows(adj, pkg.sample_params(4, T4, P4, -1.0, SEEDS), ctr, 1)
    assert np.array_equal(more[0], ref), (version, "the draw counters")
    for i, s in enumerate(slots):
        assert np.array_equal(_table(b, s), tables[i]), (version, s, "a row that does not record neither decays nor counts")
    # 12 + 12 is 24
    _like(twin, b, slots, st)
    a1, _ = twin.decode_sample_penalized(slots, first, 12, T4, P4, SEEDS, PRES, FREQ)
    a2, _ = twin.decode_sample_penalized(slots, [int(t) for t in a1[:, -1]], 12, T4, P4, SEEDS, PRES, FREQ)
    assert np.array_equal(a1, loop[:, :12])
    # (the second call feeds the 12th token, which the 24-step loop fed as its 13th pass: its outputs are steps 13 .. 24)
    assert np.array_equal(a2, loop[:, 12:]), (version, a2.tolist(), loop[:, 12:].tolist())
    for i, s in enumerate(slots):
        assert np.array_equal(_table(twin, s), tables[i]), (version, s)
    # a context decoding alone with the same setting equals its slot
    for i, s in enumerate(slots):
        m.state_load(st[s])
        m.set_repetition(*SETTINGS[s])
        m.counts_reset()
        m.rng_seek(0)
        m.set_logit_bias({3: -np.inf, 17: 1.5} if s == 3 else {})
        ref, _ = m.decode_sample_penalized(first[i], 24, T4[i], P4[i], SEEDS[i], PRES, FREQ)
        assert np.array_equal(ref, loop[i]), (version, s, SETTINGS[s])
        words = m.counts_f32().view(np.uint32) if D.is_decaying(SETTINGS[s][0]) else m.counts()
        assert np.array_equal(words, tables[i]), (version, s)
        assert m.repetition() == b.repetition(s)
    m.set_repetition(1.0, 1.0)
    m.set_logit_bias({})
    twin.free()
    b.free()
    m.free()


# ---- 2. none is none ----

def test_none_is_none(golden_dir):
    m = model(R.fixture_path(golden_dir, "6v0-3m", "Q5_0"))
    V = m.n_vocab
    b, twin = pkg.RWKVBatch(m, 4), pkg.RWKVBatch(m, 4)   # twin never hears of a setting
    slots = [3, 1, 0, 2]
    first = [_tok(5, s, V) for s in slots]
    none = [(1.0, 1.0)] * 4
    mixed = [(1.0, 1.0), (1.0, 1.0), (0.9, 1.2), (1.0, 1.0)]   # slot 2 has a setting: the pass runs the new kernels on every row

    def twin_like(st):
        for s in slots:
            twin.state_load(s, st[s]); twin.rng_seek(s, 0); twin.counts_reset(s)

    for what, settings, same in (("none", none, slots), ("mixed", mixed, [3, 1, 0])):
        idx = [slots.index(s) for s in same]
        # single passes
        st = _fresh(b, slots, V, 1, settings)
        twin_like(st)
        for x in (b, twin):
            for s in slots:
                x.counts_add(s, [first[0], first[1], 9, 9])
        x1 = b.eval_sample_penalized(slots, first, T4, P4, 0.3, SEEDS, PRES, FREQ, [True, False, True, True])
        y1 = twin.eval_sample_penalized(slots, first, T4, P4, 0.3, SEEDS, PRES, FREQ, [True, False, True, True])
        assert np.array_equal(x1[idx], y1[idx]), what
        x2 = b.eval_ragged_sample_penalized(slots, [[7, 8, 9], [4], [5, 6], [1, 2, 3, 4]], T4, P4, -1.0, SEEDS, PRES, FREQ, True)
        y2 = twin.eval_ragged_sample_penalized(slots, [[7, 8, 9], [4], [5, 6], [1, 2, 3, 4]], T4, P4, -1.0, SEEDS, PRES, FREQ, True)
        assert np.array_equal(x2[idx], y2[idx]), what
        # the loop, decode_until and the draft walk
        x3, _ = b.decode_sample_penalized(slots, first, 10, T4, P4, SEEDS, PRES, FREQ)
        y3, _ = twin.decode_sample_penalized(slots, first, 10, T4, P4, SEEDS, PRES, FREQ)
        assert np.array_equal(x3[idx], y3[idx]), what
        x4, w4, _ = b.decode_until(slots, first, [4, 9, 6, 7], temperature=T4, top_p=P4, seed=SEEDS, presence=PRES, frequency=FREQ)
        y4, v4, _ = twin.decode_until(slots, first, [4, 9, 6, 7], temperature=T4, top_p=P4, seed=SEEDS, presence=PRES, frequency=FREQ)
        for i in idx:
            assert np.array_equal(x4[i], y4[i]) and w4[i] == v4[i], (what, i)
        params, pens = pkg.sample_params(4, T4, P4, -1.0, SEEDS), pkg.penalty_params(4, PRES, FREQ, True)
        draft = [[first[i], int(x3[i][0]), int(x3[i][1])] for i in range(4)]
        x5, k5 = b.eval_draft(slots, draft, params=params, penalties=pens)
        y5, l5 = twin.eval_draft(slots, draft, params=params, penalties=pens)
        for i in idx:
            assert x5[i] == y5[i] and k5[i] == l5[i], (what, i)
        for s in same:
            assert np.array_equal(b.state_store(s), twin.state_store(s)), (what, s)
            assert np.array_equal(b.counts(s), twin.counts(s)), (what, s)
            assert np.array_equal(b.counts_f32(s), twin.counts(s).astype(np.float32)), (what, s)
        # the draw counters: the next generator draws agree
        nx = b.eval_sample_penalized(slots, first, T4, P4, -1.0, SEEDS, 0.0, 0.0, False)
        ny = twin.eval_sample_penalized(slots, first, T4, P4, -1.0, SEEDS, 0.0, 0.0, False)
        assert np.array_equal(nx[idx], ny[idx]), what
    # the context
    c = m.clone()
    lg, _ = m.eval(11, None)
    c.eval(11, None)
    m.set_repetition(1.0, 1.0)
    for x in (m, c):
        x.counts_reset(); x.counts_add([int(np.argmax(lg)), 4, 4]); x.rng_seek(0)
    assert [m.sample_penalized(1.0, 0.9, u, 0, PRES, FREQ, True) for u in (0.1, 0.5, 0.9)] == [c.sample_penalized(1.0, 0.9, u, 0, PRES, FREQ, True) for u in (0.1, 0.5, 0.9)]
    assert np.array_equal(m.counts(), c.counts())
    m.state_load(None); c.state_load(None)
    la, _ = m.decode_sample_penalized(7, 10, 1.0, 0.9, 5, PRES, FREQ)
    lb, _ = c.decode_sample_penalized(7, 10, 1.0, 0.9, 5, PRES, FREQ)
    assert np.array_equal(la, lb) and np.array_equal(m.counts(), c.counts()) and np.array_equal(m.state_store(), c.state_store())
    c.free()
    twin.free()
    b.free()
    m.free()


# ---- 5. decode_until ----

def test_decode_until_leaves_every_row_where_the_plain_loop_of_its_length_does(golden_dir):
    m = model(R.fixture_path(golden_dir, "6v0-3m", "Q5_0"))
    V = m.n_vocab
    b, twin = pkg.RWKVBatch(m, 4), pkg.RWKVBatch(m, 4)
    slots = [3, 1, 0, 2]
    first = [_tok(5, s, V) for s in slots]
    st = _fresh(b, slots, V, 3)
    _like(twin, b, slots, st)
    loop, _ = twin.decode_sample_penalized(slots, first, 16, T4, P4, SEEDS, PRES, FREQ)
    # row 0 stops at a sequence (its tokens 5 and 6 of the plain loop), the others at budgets of their own
    stops = [[[int(loop[0][4]), int(loop[0][5])]], [], [], []]
    budgets = [16, 1, 11, 16]
    rows, why, _ = b.decode_until(slots, first, budgets, stop=stops, temperature=T4, top_p=P4, seed=SEEDS, presence=PRES, frequency=FREQ)
    cut0 = next(j + 1 for j in range(1, 16) if [int(loop[0][j - 1]), int(loop[0][j])] == stops[0][0])
    lens = [cut0, 1, 11, 16]
    assert 2 <= cut0 <= 6, lens   # (four different lengths)
    for i, s in enumerate(slots):
        assert list(rows[i]) == list(loop[i][:lens[i]]), (i, list(rows[i]), loop[i].tolist())
        assert int(why[i]) == (0 if i == 0 else pkg.NO_TOKEN)
        # the plain loop of the row's own length, alone
        twin.state_load(s, st[s]); twin.rng_seek(s, 0); twin.counts_reset(s)
        alone, _ = twin.decode_sample_penalized([s], [first[i]], lens[i], T4[i], P4[i], SEEDS[i], PRES, FREQ)
        assert np.array_equal(alone[0], rows[i])
        assert np.array_equal(_table(b, s), _table(twin, s)), (s, SETTINGS[s], "the table of a retired row")
        assert np.array_equal(b.state_store(s), twin.state_store(s)), s
    twin.free()
    b.free()
    m.free()


# ---- 6. eval_draft ----

def test_draft_walk_on_decaying_slots_is_the_plain_loop(golden_dir):
    m = model(R.fixture_path(golden_dir, "6v0-3m", "Q5_0"))
    V = m.n_vocab
    b, twin = pkg.RWKVBatch(m, 4), pkg.RWKVBatch(m, 4)
    slots = [3, 1, 0, 2]
    settings = [(0.5, 1.0), (0.996, 1.0), (0.9, 1.2), (0.996, 2.0)]   # every slot decays
    first = [_tok(5, s, V) for s in slots]
    st = _fresh(b, slots, V, 4, settings)
    _like(twin, b, slots, st, settings)
    e = _steps(twin, slots, first, 6, T4, P4, SEEDS)   # what the plain loop emits: e0 .. e5
    # a draft that stands, one that fails at once, one that fails in the middle, one empty
    drafts = [[int(t) for t in e[0][:4]], [(int(e[1][0]) + 1) % V, int(e[1][1])], [int(e[2][0]), int(e[2][1]), (int(e[2][2]) + 1) % V, int(e[2][3])], []]
    keep = [5, 1, 3, 1]
    params, pens = pkg.sample_params(4, T4, P4, -1.0, SEEDS), pkg.penalty_params(4, PRES, FREQ, True)
    emitted, lens = b.eval_draft(slots, [[first[i]] + drafts[i] for i in range(4)], params=params, penalties=pens)
    assert lens.tolist() == keep, lens.tolist()
    for i in range(4):
        assert list(emitted[i]) == [int(t) for t in e[i][:keep[i]]], (i, list(emitted[i]), e[i].tolist())
    # every slot is where the plain loop of keep[i] steps leaves it: state, table, counter (the next draws agree)
    _like(twin, b, slots, st, settings)
    for i, s in enumerate(slots):
        _steps(twin, [s], [first[i]], keep[i], [T4[i]], [P4[i]], [SEEDS[i]])
    for s in slots:
        assert np.array_equal(b.state_store(s), twin.state_store(s)), s
        assert np.array_equal(_table(b, s), _table(twin, s)), (s, settings[s])
    nxt = [int(emitted[i][-1]) for i in range(4)]
    assert np.array_equal(_steps(b, slots, nxt, 2, T4, P4, SEEDS), _steps(twin, slots, nxt, 2, T4, P4, SEEDS))
    twin.free()
    b.free()
    m.free()


# ---- 7. composition ----

def test_guided_truncating_repeating_slot_is_the_hooks_composed_on_the_host(golden_dir):
    import guide_ref as G
    m = model(R.fixture_path(golden_dir, "6v0-3m", "Q5_0"))
    V = m.n_vocab
    b = pkg.RWKVBatch(m, 2)
    g = G.random_guide(V, 4, seed=3)
    gid = b.create_guide(g.edges)
    b.attach_guide(0, gid, 1)
    settings = [(0.9, 1.5), (1.0, 1.25)]
    for s in (0, 1):
        b.set_truncation(s, 6, 0.0)
        b.set_repetition(s, *settings[s])
        b.counts_reset(s)
    tables = [np.zeros(V, dtype=np.uint32), np.zeros(V, dtype=np.uint32)]
    state, feed = 1, [7, 9]
    for step, u in enumerate((0.03, 0.31, 0.55, 0.78, 0.97, 0.5, 0.2, 0.66)):
        out, lg = b.eval_sample_penalized([0, 1], feed, [1.0, 0.8], [1.0, 0.9], float(u), 0, PRES, FREQ, True, want_logits=True)
        host = np.stack([D.adjusted(lg[s], tables[s], PRES, FREQ, *settings[s]) for s in (0, 1)])   # the penalised source ...
        host[0][~g.mask(state)] = -np.inf                                                             # ... the guide's mask ...
        host = np.stack([C.masked(host[0], 6), C.masked(host[1], 6)])                                 # ... then top-k
        ref, _ = _sample_rows(host, pkg.sample_params(2, [1.0, 0.8], [1.0, 0.9], float(u), 0), None, 1)
        assert np.array_equal(out, ref), (step, u, out.tolist(), ref.tolist())
        for s in (0, 1):
            tables[s] = D.recorded(tables[s], settings[s][0], int(out[s]))
            assert np.array_equal(_table(b, s), tables[s]), (step, s)
        state, miss = g.step(state, int(out[0]))
        assert miss == 0 and b.guide_state(0) == (gid, state, 0), (step, b.guide_state(0))
        feed = [int(t) for t in out]
    b.detach_guide(0)
    b.free_guide(gid)
    b.free()
    m.free()


# ---- 8. table rules, 9. argument checks ----

def test_table_rules(golden_dir):
    m = model(R.fixture_path(golden_dir, "6v0-3m", "Q5_0"))
    V = m.n_vocab
    b = pkg.RWKVBatch(m, 4)
    toks = [5, 9, 5, 200 % V, 5]
    assert all(b.repetition(s) == (1.0, 1.0) for s in range(4)) and m.repetition() == (1.0, 1.0)
    b.counts_add(0, toks)
    # a set that does not flip the kind keeps the row; counts_store_f32 on an integer slot returns the counts
    b.set_repetition(0, 1.0, 1.3)
    assert b.counts(0)[5] == 3 and b.counts(0).sum() == 5
    assert np.array_equal(b.counts_f32(0), b.counts(0).astype(np.float32)) and b.counts_f32(0).dtype == np.float32
    # one that flips it zeroes the row; counts_add then decays per token, in order
    b.set_repetition(0, 0.996, 1.3)
    assert not b.counts_f32(0).any()
    b.counts_add(0, toks)
    want = D.counts_add(np.zeros(V, dtype=np.uint32), 0.996, toks)
    assert np.array_equal(b.counts_f32(0).view(np.uint32), want)
    b.set_repetition(0, 0.5, 1.0)   # decaying before and after: kept
    assert np.array_equal(b.counts_f32(0).view(np.uint32), want)
    b.counts_add(0, [9])
    want = D.counts_add(want, 0.5, [9])
    assert np.array_equal(b.counts_f32(0).view(np.uint32), want)
    # counts_store on a decaying slot
    b.last_error = 0
    with pytest.raises(ValueError):
        b.counts(0)
    assert b.last_error & ARGS
    # state_copy(.., COUNTS) between like slots copies; between unlike slots it is refused and nothing changes
    b.set_repetition(1, 0.9, 1.0)
    b.copy_state(1, 0, counts=True)
    assert np.array_equal(b.counts_f32(1).view(np.uint32), want) and b.repetition(1) == (float(np.float32(0.9)), 1.0)
    b.counts_add(2, [1, 1, 2])
    b.state_load(2, None); b.eval([2], [3], want_logits=False)
    before = (b.state_store(2), b.counts(2), b.state_store(0))
    b.last_error = 0
    for dst, src in ((2, 0), (0, 2)):
        with pytest.raises(ValueError):
            b.copy_state(dst, src, counts=True)
        assert b.last_error & ARGS
    assert np.array_equal(b.state_store(2), before[0]) and np.array_equal(b.counts(2), before[1]) and np.array_equal(b.state_store(0), before[2])
    assert np.array_equal(b.counts_f32(0).view(np.uint32), want)
    b.copy_state(2, 0)   # (without the counts bit the kinds do not matter)
    b.copy_state(3, 2, counts=True)
    assert np.array_equal(b.counts(3), before[1])
    # reset zeroes a decaying row; flipping back zeroes again
    b.counts_reset(0)
    assert not b.counts_f32(0).any()
    b.counts_add(0, [4]); b.set_repetition(0, 1.0, 1.0)
    assert not b.counts(0).any()
    # the context: the same rules, and a clone starts with none
    m.set_repetition(0.996, 1.1)
    m.counts_add(toks)
    assert np.array_equal(m.counts_f32().view(np.uint32), D.counts_add(np.zeros(V, dtype=np.uint32), 0.996, toks))
    with pytest.raises(ValueError):
        m.counts()
    assert m.last_error & ARGS
    c = m.clone()
    assert c.repetition() == (1.0, 1.0), "a cloned context starts with none"
    c.free()
    m.set_repetition(1.0, 1.0)
    assert not m.counts().any()
    b.free()
    m.free()


def test_rejections_change_nothing(golden_dir, tmp_path):
    m = model(R.fixture_path(golden_dir, "6v0-3m", "Q5_0"))
    b, twin = pkg.RWKVBatch(m, 3), pkg.RWKVBatch(m, 3)
    for x in (b, twin):
        x.set_repetition(1, 0.996, 1.2)
        x.counts_add(1, [3, 4, 3])
        x.counts_add(0, [8])
    slots, toks = [0, 1, 2], [3, 4, 5]
    b.eval(slots, toks, want_logits=False); twin.eval(slots, toks, want_logits=False)
    snapshot = {s: b.state_store(s) for s in range(3)}
    inf, nan = float("inf"), float("nan")
    bad = ((1, nan, 1.0), (1, -0.01, 1.0), (1, 1.0001, 1.0), (1, 0.5, nan), (1, 0.5, 0.0), (1, 0.5, -1.0), (1, 0.5, inf), (0, 0.5, -inf), (3, 0.5, 1.0), (1 << 40, 1.0, 1.0))
    for slot, d, r in bad:
        b.last_error = 0
        with pytest.raises(ValueError):
            b.set_repetition(slot, d, r)
        assert b.last_error & ARGS, (slot, d, r, b.last_error)
    for call in (lambda: b.repetition(3), lambda: b.counts_f32(3)):
        b.last_error = 0
        with pytest.raises(ValueError):
            call()
        assert b.last_error & ARGS
    m.set_repetition(0.9, 1.5)
    for d, r in ((nan, 1.0), (-1.0, 1.0), (2.0, 1.0), (0.5, 0.0), (0.5, nan), (0.5, inf)):
        with pytest.raises(ValueError):
            m.set_repetition(d, r)
        assert m.last_error & ARGS, (d, r)
    assert m.repetition() == (float(np.float32(0.9)), 1.5) and b.repetition(1) == (float(np.float32(0.996)), float(np.float32(1.2))) and b.repetition(0) == (1.0, 1.0)
    m.set_repetition(1.0, 1.0)
    # setting, table, parity and counters as they were: everything that follows equals a batch that never saw the bad calls
    for s in range(3):
        assert np.array_equal(b.state_store(s), snapshot[s]), s
    assert np.array_equal(b.counts_f32(1), twin.counts_f32(1)) and np.array_equal(b.counts(0), twin.counts(0)) and not b.counts(2).any()
    la, _ = b.decode_sample_penalized(slots, toks, 6, 1.0, 0.9, [5, 6, 7], 0.3, 0.2)
    lb, _ = twin.decode_sample_penalized(slots, toks, 6, 1.0, 0.9, [5, 6, 7], 0.3, 0.2)
    assert np.array_equal(la, lb)
    for s in range(3):
        assert np.array_equal(b.state_store(s), twin.state_store(s)), s
        assert np.array_equal(b.counts_f32(s), twin.counts_f32(s)), s
    twin.free()
    b.free()
    m.free()
    # the context forms on a chain of stages, as the penalised context calls
    p = str(tmp_path / "m.bin")
    synth.write_model(p, synth.CONFIGS["test-v6"], "Q5_1", seed=3)
    os.environ["RWKV_MI_DEVICES"] = "0,0"
    try:
        c = model(p)
    finally:
        del os.environ["RWKV_MI_DEVICES"]
    library().rwkv_set_print_errors(c._ctx, False)
    for call in (lambda: c.set_repetition(0.996, 1.1), lambda: c.repetition(), lambda: c.counts_f32()):
        c.last_error = 0
        with pytest.raises(ValueError):
            call()
        assert c.last_error & ARGS
    library().rwkv_set_print_errors(c._ctx, True)
    c.free()
