"""Top-k and min-p in the device sampler (rwkv_mi_*truncation_set, csrc/sampling.hip select_stage / cut_sample): top-k is held, bit for bit,
to the existing sampler on logits masked on the host (tests/cut_ref.py); "none" to the existing sampler on the same logits; min-p to the
float64 restatement; every row of the batch to a context decoding alone; every caller of the sampler to single steps with the same setting.

Where the issue's wording and its semantics part: a row with temperature 0 is an argmax and skips the select stage, so the vector its draw
leaves in the scratch is the untruncated softmax -- for such a row "weights > 0 is a subset of the mask" cannot hold and is not what the
semantics state; the row's TOKEN must lie in the mask instead (it is the maximum at its lowest index)."""
import ctypes

import numpy as np
import pytest

import cut_ref as C
import reference_constants as R
from gpu_lib import library, model, pkg, synth
from test_gpu_batch import _tok
from test_gpu_batch_sample import _crafted_rows, _descending_cumsum, _sample_rows, _top_p_clear_of_the_cumsums

pytestmark = pytest.mark.gpu

ARGS = 1 << 8   # RWKV_ERROR_ARGS
US = np.linspace(0.001, 0.999, 41)

_cut_hooks = None


def _cut_hooks_library():
    """lib/librwkv_testhooks_cut.so: the product objects + the truncating sampler's test entry point (include/rwkv_testhooks_cut.h)."""
    global _cut_hooks
    if _cut_hooks is None:
        library()   # (builds; and HIP is initialised in the order gpu_lib keeps)
        _cut_hooks = pkg.RWKVSharedLibrary(pkg.CUT_HOOKS_LIB_PATH)
    return _cut_hooks


def _cut_rows(logits, params, cuts, counters, rows_kernel, want_weights=False):
    L = _cut_hooks_library().library
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    n_rows, n_vocab = logits.shape
    table = (pkg.CutParams * n_rows)(*[pkg.CutParams(int(k), float(p)) for k, p in cuts])
    ctr = None if counters is None else np.ascontiguousarray(counters, dtype=np.uint64).copy()
    out = np.empty(n_rows, dtype=np.uint32)
    w = np.empty((n_rows, n_vocab), dtype=np.float32) if want_weights else None
    ok = L.rwkv_mi_test_cut_rows(logits.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), n_rows, n_vocab, params, table,
                                 None if ctr is None else ctr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), rows_kernel,
                                 out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                 None if w is None else w.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    assert ok, "rwkv_mi_test_cut_rows failed"
    return out, ctr, w


_rows_cache = {}


def _rows(V):
    """The eight crafted rows of test_gpu_batch_sample with their (temperature, top_p), and three more for the select stage: a plateau of 200
    exactly equal values at scattered indices (several thread chunks) that a k cuts through, a NaN among the largest values, and a row that is
    half -inf. Computed once per V and never written."""
    if V not in _rows_cache:
        rng = np.random.default_rng(V)
        logits, params = _crafted_rows(V, rng)
        g = rng.standard_normal(V).astype(np.float32)
        plateau = g.copy()
        at = np.sort(rng.choice(V, 200, replace=False))
        plateau[at] = np.float32(2.5)            # (some 6 of 1000, 300 of 50 277, 400 of 65 536 standard normals lie above: see _plateau_k)
        nanrow = g.copy()
        top = np.argsort(-nanrow)[:5]
        nanrow[top[2]] = np.nan
        half = g.copy()
        half[rng.permutation(V)[:V // 2]] = -np.inf
        logits = np.concatenate([logits, np.stack([plateau, nanrow, half])])
        params = list(params) + [(1.0, 1.0), (0.7, 1.0), (1.0, _top_p_clear_of_the_cumsums(half, 0.9))]
        logits.setflags(write=False)
        _rows_cache[V] = (logits, params, at)
    return _rows_cache[V]


def _plateau_k(logits_row, at):
    """A k that cuts through the middle of the plateau: everything above it, and half of it."""
    return int((logits_row > np.float32(2.5)).sum()) + at.size // 2


# ---- 1. top-k is the mask, bit for bit ----

@pytest.mark.parametrize("V", [1000, 50277, 65536])
def test_top_k_is_the_mask_bit_for_bit(V):
    logits, params, at = _rows(V)
    n = logits.shape[0]
    T, P = [q[0] for q in params], [q[1] for q in params]
    ctr_in = np.arange(n, dtype=np.uint64) * 3
    kp = _plateau_k(logits[8], at)
    assert (logits[8] == np.float32(2.5)).sum() == 200 and at[-1] // -(-V // 1024) - at[0] // -(-V // 1024) >= 3, "the plateau spans thread chunks"
    assert np.isfinite(logits[10]).sum() < V - 1
    for k in (1, 2, 7, 40, V - 1, kp):
        ks = [k] * n
        want = np.stack([C.top_k_mask(logits[r], ks[r]) for r in range(n)])
        ref_logits = np.stack([C.masked(logits[r], ks[r]) for r in range(n)])
        if k == kp:   # the cut goes through the plateau: its first hundred members by index stay
            assert want[8][at[:100]].all() and not want[8][at[100:]].any()
        if k == V - 1:
            assert not want[9][np.isnan(logits[9])].any() and want[10].sum() == V - 1   # (the NaN never ranks; -inf fills up, by index)
        for form in (1, 0):
            for i, u in enumerate(US):
                table = pkg.sample_params(n, T, P, float(u), 0)
                got, got_ctr, w = _cut_rows(logits, table, [(kk, 0.0) for kk in ks], ctr_in, form, want_weights=(i == 0))
                ref, ref_ctr = _sample_rows(ref_logits, table, ctr_in, form)
                assert np.array_equal(got, ref), (V, k, form, u, got.tolist(), ref.tolist())
                assert np.array_equal(got_ctr, ref_ctr), (V, k, form, u)
                if w is not None:
                    for r in range(n):
                        if T[r] != 0.0:
                            assert not (w[r] > 0.0)[~want[r]].any(), (V, k, form, r, "a weight outside the mask")
                            assert (w[r] > 0.0).any(), (V, k, form, r)
                        else:
                            assert want[r][int(got[r])], (V, k, form, r, "the argmax lies in the mask")


# ---- 2. off is today's sampler ----

@pytest.mark.parametrize("V", [1000, 50277, 65536])
def test_off_is_the_sampler_without_a_setting(V):
    logits, params, _ = _rows(V)
    base = logits[:8]   # (without a mask the NaN row is the old sampler's all-NaN case; it is compared as well, below)
    T, P = [q[0] for q in params], [q[1] for q in params]
    for rows, n in ((base, 8), (logits, 11)):
        ctr_in = np.arange(n, dtype=np.uint64) * 5 + 1
        for cut in ((0, 0.0), (V, 0.0), (V + 7, 0.0)):
            for form in (1, 0):
                for u in (-1.0, 0.001, 0.37, 0.999):
                    table = pkg.sample_params(n, T[:n], P[:n], float(u), [70 + r for r in range(n)])
                    got, got_ctr, _ = _cut_rows(rows, table, [cut] * n, ctr_in, form)
                    ref, ref_ctr = _sample_rows(rows, table, ctr_in, form)
                    assert np.array_equal(got, ref) and np.array_equal(got_ctr, ref_ctr), (V, cut, form, u, got.tolist(), ref.tolist())


# ---- 3. min-p ----

NO_CLEAR_MIN_P = {4: "all values equal: every ratio is 1, no threshold below 1 lies in a gap"}


@pytest.mark.parametrize("V", [1000, 50277, 65536])
def test_min_p_against_the_reference(V):
    logits, params, _ = _rows(V)
    rows = [r for r in range(8) if r not in NO_CLEAR_MIN_P]
    assert len(rows) >= 6
    lg = logits[rows]
    n = len(rows)
    T = [params[r][0] if params[r][0] != 0.0 else 1.0 for r in rows]   # (an argmax row draws no vector: it gets temperature 1 here)
    targets = [0.05, 0.2, 3e-14, 0.05, 0.2, 0.05, 0.5]   # (the spike row: every other token lies 30 below the maximum)
    mp = [C.min_p_in_a_gap(lg[i], targets[i]) for i in range(n)]
    # the condition, on the reference alone, before the device runs
    for i in range(n):
        assert mp[i] is not None and 0.0 < mp[i] < 1.0, (V, rows[i])
        assert C.clearance(lg[i], mp[i]) > 1e-4, (V, rows[i], mp[i], C.clearance(lg[i], mp[i]))
    cases = []
    # alone; with a clear top-p (taken on the full distribution: no top-k); with a top-k
    cases.append(([1.0] * n, [0] * n))
    cases.append(([_top_p_clear_of_the_cumsums(lg[i], 0.9) for i in range(n)], [0] * n))
    cases.append(([1.0] * n, [40] * n))
    for P, K in cases:
        for i in range(n):
            if 0.0 < P[i] < 1.0:
                assert float(np.abs(_descending_cumsum(lg[i]) - P[i]).min()) > 1e-5, (V, rows[i], P[i])
        ref = [C.ref_distribution_cut(lg[i], T[i], P[i], K[i], mp[i]) for i in range(n)]
        cdf = [np.cumsum(p) for p in ref]
        cuts = [(K[i], mp[i]) for i in range(n)]
        for form in (1, 0):
            for j, u in enumerate(US):
                table = pkg.sample_params(n, T, P, float(u), 0)
                got, _, w = _cut_rows(lg, table, cuts, None, form, want_weights=(j == 0))
                if w is not None:
                    for i in range(n):
                        assert np.array_equal(w[i] > 0.0, ref[i] > 0.0), (V, rows[i], P[i], K[i], mp[i], int((w[i] > 0).sum()), int((ref[i] > 0).sum()))
                for i in range(n):
                    tok, pr = int(got[i]), ref[i]
                    assert tok < V and pr[tok] > 0.0, (V, rows[i], u, tok)
                    lo = cdf[i][tok] - pr[tok]
                    assert lo - 1e-4 <= u <= cdf[i][tok] + 1e-4, (V, rows[i], P[i], K[i], mp[i], u, tok, lo, cdf[i][tok])


# ---- 4. rows equal the sequence alone ----

def _synth(tmp_path, name, fmt, seed=7):
    library()
    p = str(tmp_path / f"{name}-{fmt}.bin")
    synth.write_model(p, synth.CONFIGS[name], fmt, seed=seed)
    return p


SETTINGS = [(0, 0.0), (5, 0.0), (0, 0.1), (40, 0.05)]


@pytest.mark.parametrize("name,fmt", [("test-v6", "Q5_1"), ("test-v7", "Q5_1"), ("test-v4", "Q8_0"), ("mega-v6-2048-v64k", "Q4_0")])
def test_rows_equal_the_sequence_alone(tmp_path, name, fmt):
    p = _synth(tmp_path, name, fmt, seed=9)
    m = model(p)
    V = m.n_vocab
    b = pkg.RWKVBatch(m, 4)
    slots = [2, 0, 3, 1]
    for s in slots:
        b.state_load(s, None)
        b.set_truncation(s, *SETTINGS[s])
    b.eval(slots, [_tok(1, s, V) for s in slots], want_logits=False)   # every slot from its own state
    start = {s: b.state_store(s) for s in slots}
    first = [_tok(2, s, V) for s in slots]
    T, P, seeds = [1.0, 0.8, 1.3, 1.0], [1.0, 0.9, 0.95, 0.0], [11, 12, 13, 14]
    toks, _ = b.decode_sample(slots, first, 24, T, P, seeds)
    more = b.eval_sample(slots, [int(t) for t in toks[:, -1]], T, P, -1.0, seeds)   # (one more draw: the counters stand where the context's does)
    for i, s in enumerate(slots):
        m.state_load(start[s])
        m.set_truncation(*SETTINGS[s])
        ref, _ = m.decode_sample(first[i], 24, T[i], P[i], seeds[i])
        assert np.array_equal(toks[i], ref), (name, fmt, s, SETTINGS[s], list(toks[i]), list(ref))
        # the state and the counter: the context steps the 25th token alone and draws again from its generator
        _, st = m.eval(int(ref[-1]), m.state_store())
        assert np.array_equal(b.state_store(s), st), (name, fmt, s)
        assert int(more[i]) == m.sample(T[i], P[i], -1.0, seeds[i]), (name, fmt, s, "the draw counter")
        assert m.truncation() == b.truncation(s)
    m.set_truncation(0, 0.0)
    b.free()
    m.free()


# ---- 5. every caller honours the setting, bit for bit against steps ----

def _fresh(m, b, slots, V, salt):
    """every named slot from a state of its own, its draw counter at 0, its counts empty; the states"""
    for s in slots:
        b.state_load(s, None)
    b.eval(slots, [_tok(salt, s, V) for s in slots], want_logits=False)
    for s in slots:
        b.rng_seek(s, 0)
    return {s: b.state_store(s) for s in slots}


def _steps(b, slots, first, n, T, P, seeds, pen=None):
    """n single passes with the generator drawing (penalised and recording when pen = (presence, frequency)): tokens [len(slots)][n]"""
    out = np.empty((len(slots), n), dtype=np.uint32)
    feed = list(first)
    for j in range(n):
        if pen is None:
            got = b.eval_sample(slots, feed, T, P, -1.0, seeds)
        else:
            got = b.eval_sample_penalized(slots, feed, T, P, -1.0, seeds, pen[0], pen[1], True)
        out[:, j] = got
        feed = [int(t) for t in got]
    return out


def test_every_caller_honours_the_setting(golden_dir):
    path = R.fixture_path(golden_dir, "6v0-3m", "Q5_0")
    m = model(path)
    V = m.n_vocab
    b, twin = pkg.RWKVBatch(m, 4), pkg.RWKVBatch(m, 4)
    slots = [3, 1, 0, 2]
    T, P, seeds = [1.0, 0.9, 1.2, 1.0], [1.0, 0.95, 0.9, 0.0], [21, 22, 23, 24]
    first = [_tok(5, s, V) for s in slots]
    for x in (b, twin):
        for s in slots:
            x.set_truncation(s, *SETTINGS[s])

    def both(salt):
        st = _fresh(m, b, slots, V, salt)
        for s in slots:
            twin.state_load(s, st[s])
            twin.rng_seek(s, 0)
            for x in (b, twin):
                x.counts_reset(s)
        return st

    def same_states(what):
        for s in slots:
            assert np.array_equal(b.state_store(s), twin.state_store(s)), (what, s)

    # the sampled loop is its steps
    both(1)
    loop, _ = b.decode_sample(slots, first, 16, T, P, seeds)
    steps = _steps(twin, slots, first, 16, T, P, seeds)
    assert np.array_equal(loop, steps), (loop.tolist(), steps.tolist())
    # (the loop feeds 16 tokens, the steps 16 as well: the last token of either is not fed)
    same_states("decode_sample")
    # ... and the setting acts: without it the same loop emits other tokens
    both(1)
    for s in slots:
        b.set_truncation(s, 0, 0.0)
    plain, _ = b.decode_sample(slots, first, 16, T, P, seeds)
    for s in slots:
        b.set_truncation(s, *SETTINGS[s])
    assert np.array_equal(plain[slots.index(0)], loop[slots.index(0)]) and not np.array_equal(plain, loop)
    # the penalised loop is its steps
    both(2)
    loop, _ = b.decode_sample_penalized(slots, first, 16, T, P, seeds, 0.4, 0.3)
    steps = _steps(twin, slots, first, 16, T, P, seeds, pen=(0.4, 0.3))
    assert np.array_equal(loop, steps), (loop.tolist(), steps.tolist())
    same_states("decode_sample_penalized")
    for s in slots:
        assert np.array_equal(b.counts(s), twin.counts(s)), s
    # decode_until is the plain loop cut at the stop
    both(3)
    loop, _ = b.decode_sample(slots, first, 16, T, P, seeds)
    stops = [[[int(loop[i][6]), int(loop[i][7])]] for i in range(4)]
    both(3)
    rows, why, _ = b.decode_until(slots, first, 16, stop=stops, temperature=T, top_p=P, seed=seeds)
    for i in range(4):
        seq = stops[i][0]
        cut = next(j + 1 for j in range(1, 16) if [int(loop[i][j - 1]), int(loop[i][j])] == seq)
        assert cut <= 8 and list(rows[i]) == list(loop[i][:cut]) and int(why[i]) == 0, (i, cut, list(rows[i]), list(loop[i]))
    # eval_draft, sampled and penalised: a draft that stands, one that fails at once, one that fails in the middle, one empty
    for pen in (None, (0.4, 0.3)):
        st = both(4)
        e = _steps(twin, slots, first, 6, T, P, seeds, pen=pen)   # what the plain loop emits: e0 .. e5
        drafts = [[int(t) for t in e[0][:4]], [(int(e[1][0]) + 1) % V, int(e[1][1])], [int(e[2][0]), int(e[2][1]), (int(e[2][2]) + 1) % V, int(e[2][3])], []]
        keep = [5, 1, 3, 1]
        params = pkg.sample_params(4, T, P, -1.0, seeds)
        pens = None if pen is None else pkg.penalty_params(4, pen[0], pen[1], True)
        emitted, lens = b.eval_draft(slots, [[first[i]] + drafts[i] for i in range(4)], params=params, penalties=pens)
        assert lens.tolist() == keep, (pen, lens.tolist())
        for i, s in enumerate(slots):
            assert list(emitted[i]) == [int(t) for t in e[i][:keep[i]]], (pen, i, list(emitted[i]), e[i].tolist())
        # every slot is where the plain loop of keep[i] steps leaves it: state, counter (the next draws agree), counts
        for s in slots:
            twin.state_load(s, st[s]); twin.rng_seek(s, 0); twin.counts_reset(s)
        for i, s in enumerate(slots):
            _steps(twin, [s], [first[i]], keep[i], [T[i]], [P[i]], [seeds[i]], pen=pen)
        same_states(("eval_draft", pen))
        nxt = [int(emitted[i][-1]) for i in range(4)]
        assert np.array_equal(_steps(b, slots, nxt, 2, T, P, seeds, pen=pen), _steps(twin, slots, nxt, 2, T, P, seeds, pen=pen)), pen
        if pen is not None:
            for s in slots:
                assert np.array_equal(b.counts(s), twin.counts(s)), s
    twin.free()
    b.free()
    m.free()


def test_guided_slot_with_top_k_is_the_hook_on_host_masked_logits(golden_dir):
    import guide_ref as G
    path = R.fixture_path(golden_dir, "6v0-3m", "Q5_0")
    m = model(path)
    V = m.n_vocab
    b = pkg.RWKVBatch(m, 2)
    g = G.random_guide(V, 4, seed=3)
    gid = b.create_guide(g.edges)
    b.attach_guide(0, gid, 1)
    b.set_truncation(0, 6, 0.0)
    b.set_truncation(1, 6, 0.0)
    state = 1
    feed = [7, 9]
    for step, u in enumerate((0.03, 0.31, 0.55, 0.78, 0.97, 0.5)):
        out, lg = b.eval_sample([0, 1], feed, [1.0, 0.8], [1.0, 0.9], float(u), 0, want_logits=True)
        host = lg.copy()
        host[0][~g.mask(state)] = -np.inf                               # the guide's mask, then top-k
        host = np.stack([C.masked(host[0], 6), C.masked(host[1], 6)])
        ref, _ = _sample_rows(host, pkg.sample_params(2, [1.0, 0.8], [1.0, 0.9], float(u), 0), None, 1)
        assert np.array_equal(out, ref), (step, u, out.tolist(), ref.tolist())
        assert g.mask(state)[int(out[0])] and C.top_k_mask(lg[1], 6)[int(out[1])]
        state, miss = g.step(state, int(out[0]))
        assert miss == 0 and b.guide_state(0) == (gid, state, 0), (step, b.guide_state(0))
        feed = [int(t) for t in out]
    b.detach_guide(0)
    b.free_guide(gid)
    b.free()
    m.free()


# ---- 6. top_k = 1 at temperature 1 ----

def test_top_k_1_emits_the_greedy_tokens_and_advances_the_counter(golden_dir):
    path = R.fixture_path(golden_dir, "6v0-3m", "Q5_0")
    m = model(path)
    V = m.n_vocab
    b, twin = pkg.RWKVBatch(m, 3), pkg.RWKVBatch(m, 3)
    slots = [0, 1, 2]
    st = _fresh(m, b, slots, V, 6)
    first = [_tok(7, s, V) for s in slots]
    greedy, _ = b.decode_greedy(slots, first, 16)
    for s in slots:
        b.state_load(s, st[s])
        b.set_truncation(s, 1, 0.0)
    toks, _ = b.decode_sample(slots, first, 16, 1.0, 1.0, [31, 32, 33])
    assert np.array_equal(toks, greedy), (toks.tolist(), greedy.tolist())
    # one advance per step: the slots continue the stream of a counter at 16, not at 0
    for s in slots:
        b.set_truncation(s, 0, 0.0)
    nxt = [int(t) for t in toks[:, -1]]
    cont = _steps(b, slots, nxt, 8, 1.0, 1.0, [31, 32, 33])
    for ctr, same in ((16, True), (0, False)):
        for s in slots:
            twin.state_load(s, st[s])
        twin.decode_greedy(slots, first, 16)
        for s in slots:
            twin.rng_seek(s, ctr)
        assert np.array_equal(_steps(twin, slots, nxt, 8, 1.0, 1.0, [31, 32, 33]), cont) == same, ctr
    twin.free()
    b.free()
    m.free()


# ---- 7. settings stick and rejections change nothing ----

def test_settings_stick_and_rejections_change_nothing(golden_dir):
    path = R.fixture_path(golden_dir, "6v0-3m", "Q5_0")
    m = model(path)
    V = m.n_vocab
    b, twin = pkg.RWKVBatch(m, 3), pkg.RWKVBatch(m, 3)
    assert all(b.truncation(s) == (0, 0.0) for s in range(3)) and m.truncation() == (0, 0.0)
    b.set_truncation(1, 40, 0.25)
    b.set_truncation(2, V + 5, 1.0)
    assert b.truncation(0) == (0, 0.0) and b.truncation(1) == (40, 0.25) and b.truncation(2) == (V + 5, 1.0)
    b.set_truncation(2, 0, 0.0)
    assert b.truncation(2) == (0, 0.0)
    m.set_truncation(3, 0.5)
    assert m.truncation() == (3, 0.5)
    c = m.clone()
    assert c.truncation() == (0, 0.0), "a cloned context starts with none"
    c.free()
    twin.set_truncation(1, 40, 0.25)
    slots, toks = [0, 1, 2], [3, 4, 5]
    args = ([1.0, 0.9, 1.0], [0.9, 1.0, 0.0], -1.0, [1, 2, 3])
    assert np.array_equal(b.eval_sample(slots, toks, *args), twin.eval_sample(slots, toks, *args))
    snapshot = {s: b.state_store(s) for s in range(3)}
    for slot, k, p in ((1, 7, float("nan")), (1, 7, -0.01), (1, 7, 1.5), (3, 7, 0.1), (1 << 40, 0, 0.0)):
        b.last_error = 0
        with pytest.raises(ValueError):
            b.set_truncation(slot, k, p)
        assert b.last_error & ARGS, (slot, k, p, b.last_error)
    b.last_error = 0
    with pytest.raises(ValueError):
        b.truncation(3)
    assert b.last_error & ARGS
    for p in (float("nan"), -1.0, 1.0001):
        with pytest.raises(ValueError):
            m.set_truncation(9, p)
        assert m.last_error & ARGS, p
    assert m.truncation() == (3, 0.5) and b.truncation(1) == (40, 0.25) and b.truncation(0) == (0, 0.0)
    for s in range(3):
        assert np.array_equal(b.state_store(s), snapshot[s]), s
    # no counter moved: the next calls return what a batch that never saw the bad ones returns
    la, _ = b.decode_sample_penalized(slots, toks, 6, 1.0, 0.9, [5, 6, 7], 0.3, 0.2)
    lb, _ = twin.decode_sample_penalized(slots, toks, 6, 1.0, 0.9, [5, 6, 7], 0.3, 0.2)
    assert np.array_equal(la, lb)
    for s in range(3):
        assert np.array_equal(b.state_store(s), twin.state_store(s)), s
    # copy_state carries no setting: the destination keeps its own
    b.copy_state(0, 1, counter=True)
    assert b.truncation(0) == (0, 0.0) and b.truncation(1) == (40, 0.25)
    # the context's setting reaches its draws: top_k = 1 is the argmax at any u
    m.set_truncation(1, 0.0)
    lg, _ = m.eval(11, None)
    assert all(m.sample(1.0, 1.0, u) == int(np.argmax(lg)) for u in (0.0, 0.5, 0.999))
    assert m.sample_penalized(1.0, 1.0, 0.7, 0, 0.0, 0.0, False) == int(np.argmax(lg))
    m.set_truncation(0, 0.0)
    twin.free()
    b.free()
    m.free()
