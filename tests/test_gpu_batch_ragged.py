"""Ragged batch passes (rwkv_mi_batch_eval_ragged / _eval_ragged_sample): row i feeds lens[i] consecutive tokens to its slot, all rows in one
pass over the weights. Every row is held to the sequence stepped alone -- the CPU oracle (OracleModel.eval, token by token) and a
rwkv_context of the same file fed the same tokens -- with np.array_equal, logits and stored states. Another batch call is the reference
only where a test says "twin"."""
import ctypes

import numpy as np
import pytest

import oracle_lib as O
import reference_constants as R
from gpu_lib import library, model, pkg, synth
from test_gpu_api_semantics import CASES

pytestmark = pytest.mark.gpu

ARGS = 1 << 8   # RWKV_ERROR_ARGS
P_UINT32 = ctypes.POINTER(ctypes.c_uint32)
P_FLOAT = ctypes.POINTER(ctypes.c_float)


def _synth(tmp_path, name, fmt, seed=7):
    library()
    p = str(tmp_path / f"{name}-{fmt}.bin")
    synth.write_model(p, synth.CONFIGS[name], fmt, seed=seed)
    return p


def _toks(call, slot, n, V):
    return [(37 * call + 11 * slot + 29 * j + 5) % V for j in range(n)]


def _oracle_row(om, state, toks):
    """The oracle stepping one sequence alone, token by token: (last logits, state)."""
    lg = None
    for t in toks:
        lg, state = om.eval(t, state)
    return lg, state


def _check_ragged(om, b, slots, rows, ost, what, check_states=True):
    """One ragged call; each row against the oracle stepping that slot alone (ost: slot -> oracle state, advanced in place)."""
    lg = b.eval_ragged(slots, rows)
    assert lg.shape == (len(slots), om.n_vocab)
    for i, (s, r) in enumerate(zip(slots, rows)):
        ol, ost[s] = _oracle_row(om, ost[s], r)
        assert np.array_equal(lg[i], ol), (what, "logits", i, s, len(r), float(np.abs(lg[i] - ol).max()))
    if check_states:
        for s in slots:
            assert np.array_equal(b.state_store(s), ost[s]), (what, "state", s)
    return lg


@pytest.mark.parametrize("version,fmt", CASES)
def test_golden_every_architecture(golden_dir, version, fmt):
    path = R.fixture_path(golden_dir, version, fmt)
    m = model(path)
    om = O.OracleModel(path)
    V = min(m.n_vocab, 128)
    prompts = [[], [72], [104, 101, 108], [84, 104, 105, 115, 32, 105, 115], [97] * 11]
    b = pkg.RWKVBatch(m, 5)
    ost, gst = {}, {}
    for s, pr in enumerate(prompts):
        st = om.init_state()
        for t in pr:
            _, st = om.eval(t, st)
        ost[s], gst[s] = st, st.copy()
        b.state_load(s, st if pr else None)
    for call, lens in enumerate(([1, 3, 7, 1, 11], [11, 1, 3, 7, 1], [7, 11, 1, 1, 3])):
        slots = list(range(5))
        rows = [_toks(call, s, lens[s], V) for s in slots]
        lg = _check_ragged(om, b, slots, rows, ost, (version, fmt, call))
        for i, s in enumerate(slots):   # rwkv_eval_sequence on a context fed the same tokens
            cl, gst[s] = m.eval_sequence(rows[i], gst[s])
            assert np.array_equal(lg[i], cl), (version, fmt, call, s)
            assert np.array_equal(b.state_store(s), gst[s]), (version, fmt, call, s)
    b.free()
    m.free()
    om.free()


# T = 31 (vector products), 32 and 33 (matrix cores), 200: len-1 rows, a segment of exactly 32 tokens, of 40, of 31, many 2-token segments --
# the _segs entry points alone, the *_seq kernels on a sub-range of the pass, and both in one pass
MIXES = [
    [1] * 3 + [2] * 14,
    [1, 31],
    [32, 1],
    [32],
    [1, 1, 32, 40, 31, 1] + [2] * 47,
]


@pytest.mark.parametrize("name,fmt", [("test-v4", "Q5_1"), ("test-v5.2", "FP16"), ("test-v6", "Q4_0"), ("test-v6", "Q8_0"), ("test-v7", "Q5_1")])
def test_both_product_paths_and_both_recurrence_routes(tmp_path, name, fmt):
    p = _synth(tmp_path, name, fmt)
    m = model(p)
    om = O.OracleModel(p)
    V = m.n_vocab
    b = pkg.RWKVBatch(m, 64)
    assert [sum(x) for x in MIXES] == [31, 32, 33, 32, 200]
    for k, lens in enumerate(MIXES):
        n = len(lens)
        slots = list(range(64 - n, 64))[::-1] if k % 2 else list(range(n))
        for s in slots:
            b.state_load(s, None)
        ost = {s: om.init_state() for s in slots}
        _check_ragged(om, b, slots, [_toks(k, s, ln, V) for s, ln in zip(slots, lens)], ost, (name, fmt, "mix", k))
        # ... and once more from the states that call left, the lengths moved round the slots
        lens2 = lens[1:] + lens[:1]
        _check_ragged(om, b, slots, [_toks(k + 9, s, ln, V) for s, ln in zip(slots, lens2)], ost, (name, fmt, "mix", k, "second call"))
    b.free()
    m.free()
    om.free()


@pytest.mark.parametrize("name,fmt", [("test-v6", "Q4_0"), ("test-v7", "Q5_1"), ("test-v4", "Q5_1"), ("test-v5.2", "FP16")])
def test_chunking_invariance(tmp_path, name, fmt):
    p = _synth(tmp_path, name, fmt, seed=11)
    m = model(p)
    om = O.OracleModel(p)
    V = m.n_vocab
    prompt = [(17 * i + 3) % V for i in range(75)]
    whole, cut = pkg.RWKVBatch(m, 4), pkg.RWKVBatch(m, 4)
    lw = whole.eval_ragged([1], [prompt])[0]
    ost = {s: om.init_state() for s in range(4)}
    # 32 + 1 + 42 over three calls that also carry other rows
    _check_ragged(om, cut, [0, 1, 2], [[5], prompt[:32], [7, 8, 9]], ost, (name, fmt, "chunk 1"))
    _check_ragged(om, cut, [1, 3], [prompt[32:33], _toks(1, 3, 40, V)], ost, (name, fmt, "chunk 2"))
    lc = _check_ragged(om, cut, [2, 0, 1], [[4], [6, 7], prompt[33:]], ost, (name, fmt, "chunk 3"))[2]
    assert np.array_equal(lw, lc), (name, fmt, float(np.abs(lw - lc).max()))
    assert np.array_equal(whole.state_store(1), cut.state_store(1)), (name, fmt)
    ol, os_ = _oracle_row(om, om.init_state(), prompt)
    assert np.array_equal(lw, ol) and np.array_equal(whole.state_store(1), os_), (name, fmt)
    whole.free()
    cut.free()
    m.free()
    om.free()


def test_twin_all_lengths_one_equals_batch_eval(golden_dir, tmp_path):
    for path, n in ((R.fixture_path(golden_dir, "6v0-3m", "Q5_0"), 6), (_synth(tmp_path, "test-v7", "Q5_1"), 33), (_synth(tmp_path, "test-v4", "Q5_1"), 33)):
        m = model(path)
        V = min(m.n_vocab, 128)
        b, twin = pkg.RWKVBatch(m, n), pkg.RWKVBatch(m, n)
        for call in range(3):
            slots = list(range(n))[::-1] if call % 2 else list(range(n))
            toks = [_toks(call, s, 1, V)[0] for s in slots]
            got = b.eval_ragged(slots, [[t] for t in toks])
            want = twin.eval(slots, toks)
            assert np.array_equal(got, want), (path, call)
            for s in slots:
                assert np.array_equal(b.state_store(s), twin.state_store(s)), (path, call, s)
        b.free()
        twin.free()
        m.free()


@pytest.mark.parametrize("name,fmt", [("mega-v6-4096", "Q4_0"), ("slice-v7-2560", "Q5_1"), ("slice-v4-768", "Q5_1")])
def test_real_geometry(tmp_path, name, fmt):
    p = _synth(tmp_path, name, fmt, seed=3)
    m = model(p)
    om = O.OracleModel(p)
    V = m.n_vocab
    b = pkg.RWKVBatch(m, 9)
    ost = {s: om.init_state() for s in range(9)}
    # 8 decode rows + one 96-token segment in one pass (the segment in the middle of the call)
    slots = [0, 1, 2, 3, 8, 4, 5, 6, 7]
    rows = [[(x * 97) % V for x in _toks(0, s, 96 if s == 8 else 1, V)] for s in slots]
    _check_ragged(om, b, slots, rows, ost, (name, fmt))
    # the slots go on as decode rows of the existing call
    toks = [(_toks(1, s, 1, V)[0] * 97) % V for s in slots]
    lg = b.eval(slots, toks)
    for i, s in enumerate(slots):
        ol, ost[s] = om.eval(toks[i], ost[s])
        assert np.array_equal(lg[i], ol), (name, fmt, "decode after the ragged pass", s)
    b.free()
    m.free()
    om.free()


SUBSETS = ([3, 0, 5], [1], [5, 2, 4, 0, 1, 3], [2, 4], [4, 2], [0, 5, 1])


def test_slots_not_named_are_untouched_any_subset_any_order(golden_dir):
    path = R.fixture_path(golden_dir, "6v0-3m", "Q5_0")
    m = model(path)
    om = O.OracleModel(path)
    b = pkg.RWKVBatch(m, 6)
    ost = {s: om.init_state() for s in range(6)}
    for call, slots in enumerate(SUBSETS):
        before = {s: b.state_store(s) for s in range(6)}
        rows = [_toks(call, s, 1 + (3 * s + 5 * call) % 9, 128) for s in slots]
        _check_ragged(om, b, slots, rows, ost, ("subset", call, slots))
        for s in range(6):
            if s not in slots:
                assert np.array_equal(b.state_store(s), before[s]), ("slot not named but changed", call, s)
    b.free()
    m.free()
    om.free()


def test_rejected_calls_change_nothing(golden_dir):
    path = R.fixture_path(golden_dir, "6v0-3m", "Q5_0")
    m = model(path)
    om = O.OracleModel(path)
    V = m.n_vocab
    b, twin = pkg.RWKVBatch(m, 6), pkg.RWKVBatch(m, 6)
    good = dict(temperature=[1.0, 0.7, 1.5, 0.3, 1.0, 0.7], top_p=[0.8, 0.95, 1.0, 0.5, 0.0, 0.8], u=-1.0, seed=[3, 4, 5, 6, 7, 8])
    slots6 = [5, 2, 4, 0, 1, 3]
    rows6 = [_toks(0, s, 1 + s, 128) for s in slots6]
    first = b.eval_ragged_sample(slots6, rows6, **good)
    assert np.array_equal(first, twin.eval_ragged_sample(slots6, rows6, **good))   # (twin: the batch that never sees a bad call)
    snapshot = {s: b.state_store(s) for s in range(6)}
    long_bad = _toks(1, 0, 40, 128)
    long_bad[23] = V                                     # a token >= n_vocab in the middle of a long segment
    bad = [
        ([0, 1], [[3], []]),                             # a zero length
        ([1, 1], [[3, 4], [5]]),                         # a repeated slot
        ([6], [[3, 4]]),                                 # a slot out of range
        ([0, 9], [[1], [2, 3]]),
        ([2, 3], [[1, 2], long_bad]),
        ([2], [[V]]),
        ([], []),                                        # n = 0
        (list(range(6)) + [0], [[1, 2]] * 7),            # n > n_slots
    ]
    for slots, rows in bad:
        b.last_error = 0
        with pytest.raises(ValueError):
            b.eval_ragged(slots, rows)
        assert b.last_error & ARGS, (slots, rows, b.last_error)
        b.last_error = 0
        with pytest.raises(ValueError):
            b.eval_ragged_sample(slots, rows, 1.0, 0.8, -1.0, 1)
        assert b.last_error & ARGS, (slots, rows, b.last_error)
    # lens == NULL (the binding always passes one: the entry points directly)
    L, lib = b._L, library()
    s2 = np.array([0, 1], dtype=np.uint32)
    t2 = np.array([3, 4, 5], dtype=np.uint32)
    out = np.empty((2, V), dtype=np.float32)
    ok = L.rwkv_mi_batch_eval_ragged(b._ptr, s2.ctypes.data_as(P_UINT32), None, t2.ctypes.data_as(P_UINT32), 2, out.ctypes.data_as(P_FLOAT))
    assert not ok and lib.rwkv_get_last_error(m._ctx) & ARGS
    params = pkg.sample_params(2, 1.0, 0.8, -1.0, 1)
    drawn = np.empty(2, dtype=np.uint32)
    ok = L.rwkv_mi_batch_eval_ragged_sample(b._ptr, s2.ctypes.data_as(P_UINT32), None, t2.ctypes.data_as(P_UINT32), 2, params,
                                            drawn.ctypes.data_as(P_UINT32), None)
    assert not ok and lib.rwkv_get_last_error(m._ctx) & ARGS
    # bad sampling arguments are rejected as eval_sample rejects them
    for kw in (dict(temperature=-1.0), dict(top_p=[0.5, 1.5]), dict(u=1.0), dict(temperature=float("nan"))):
        a = dict(temperature=1.0, top_p=0.8, u=-1.0, seed=1)
        a.update(kw)
        b.last_error = 0
        with pytest.raises(ValueError):
            b.eval_ragged_sample([0, 1], [[3, 4], [5]], **a)
        assert b.last_error & ARGS, (kw, b.last_error)
    for s in range(6):
        assert np.array_equal(b.state_store(s), snapshot[s]), ("a rejected call changed a slot", s)
    # no parity and no draw counter moved either: the next draw of every slot is what the twin draws
    nxt = [[int(t) % 128, 7, 9] for t in first]
    assert np.array_equal(b.eval_ragged_sample(slots6, nxt, **good), twin.eval_ragged_sample(slots6, nxt, **good))
    for s in range(6):
        assert np.array_equal(b.state_store(s), twin.state_store(s)), s
    # and the batch still works, against the oracle
    ost = {s: b.state_store(s) for s in range(6)}
    _check_ragged(om, b, [2, 0], [[9, 10, 11], [12]], ost, "after rejected calls")
    b.free()
    twin.free()
    m.free()
    om.free()


def test_sampling_rows_equal_the_sequence_alone(golden_dir):
    path = R.fixture_path(golden_dir, "6v0-3m", "Q5_0")
    m = model(path)
    b = pkg.RWKVBatch(m, 6)
    temperature = [1.0, 0.7, 1.5, 0.3, 1.0, 0.7]
    top_p = [0.8, 0.95, 1.0, 0.5, 0.0, 0.8]
    seed = [100 + s for s in range(6)]
    ctx = {s: m.clone() for s in range(6)}       # a fresh context per slot: its own draw counter, from 0
    cst = {s: None for s in range(6)}            # that sequence's state, fed alone through rwkv_eval_sequence

    def alone(s, toks, temp):
        lg, cst[s] = ctx[s].eval_sequence(toks, cst[s])
        if temp == 0.0:
            return int(np.argmax(lg))            # (no draw on the context: its counter stays, as the slot's must)
        return ctx[s].sample(temp, top_p[s], -1.0, seed[s])

    for call, slots in enumerate(SUBSETS + ([0, 1, 2, 3, 4, 5],)):
        rows = [_toks(call, s, 1 + (2 * s + 3 * call) % 7, 128) for s in slots]
        # a row that is a non-final prompt chunk is given temperature 0: here every third (call + slot)
        temps = [0.0 if (call + s) % 3 == 0 else temperature[s] for s in slots]
        out, lg = b.eval_ragged_sample(slots, rows, temps, [top_p[s] for s in slots], -1.0, [seed[s] for s in slots], want_logits=True)
        for i, s in enumerate(slots):
            ref = alone(s, rows[i], temps[i])
            assert int(out[i]) == ref, (call, slots, s, temps[i], int(out[i]), ref)
            if temps[i] == 0.0:
                assert int(out[i]) == int(np.argmax(lg[i])), (call, s)
            assert np.array_equal(b.state_store(s), cst[s]), (call, s)
    # every slot has had argmax rows between its draws: the draws above matched contexts whose counters the argmax rows never moved.
    # Once more, explicitly: an argmax row, then the slot's next draw equals the counter-unchanged draw of its context
    for s in range(6):
        out = b.eval_ragged_sample([s], [[3, 4, 5]], 0.0, top_p[s], -1.0, seed[s])
        assert int(out[0]) == alone(s, [3, 4, 5], 0.0), s
        out = b.eval_ragged_sample([s], [[6, 7]], temperature[s], top_p[s], -1.0, seed[s])
        assert int(out[0]) == alone(s, [6, 7], temperature[s]), s
    b.free()
    for c in ctx.values():
        c.free()
    m.free()


def test_next_to_persistent_kernel(tmp_path, monkeypatch):
    if "PERSISTENT_DECODE=unavailable" in library().rwkv_get_system_info_string():
        pytest.skip("no persistent decode kernel on this device")
    monkeypatch.setenv("RWKV_MI_NO_AUTOTUNE", "1")
    p = _synth(tmp_path, "mega-v6-4096", "Q4_0", seed=21)
    m = model(p)
    assert m.decode_path() == 2, m.persist_info()
    om = O.OracleModel(p)
    V = m.n_vocab
    b = pkg.RWKVBatch(m, 8)
    slots = list(range(8))
    ost = {s: om.init_state() for s in slots}
    cst, tok = om.init_state(), 3
    for rnd, lens in enumerate(([1, 1, 5, 1, 1, 1, 1, 1], [1, 33, 1, 1, 2, 1, 1, 1], [1] * 8)):
        toks, _ = m.decode_greedy(tok, 4)
        ref = []
        for _ in range(4):
            ol, cst = om.eval(tok, cst)
            tok = int(np.argmax(ol))
            ref.append(tok)
        assert list(toks) == ref, (rnd, list(toks), ref)
        _check_ragged(om, b, slots, [_toks(rnd, s, ln, V) for s, ln in zip(slots, lens)], ost, ("beside path 2", rnd), check_states=False)
        assert m.healthy()
    assert np.array_equal(m.state_store(), cst)
    for s in (1, 2):
        assert np.array_equal(b.state_store(s), ost[s]), s
    assert m.decode_path() == 2 and m.healthy()
    b.free()
    m.free()
    om.free()
