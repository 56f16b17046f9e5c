"""Batched decode (rwkv_mi_batch_*): N sequences per pass over the weights, each row bit-identical to that sequence stepped alone -- against
the CPU oracle and against rwkv_eval / rwkv_mi_decode_greedy on a context. Every comparison is np.array_equal."""
import numpy as np
import pytest

import oracle_lib as O
import reference_constants as R
from gpu_lib import library, model, pkg, synth
from test_gpu_api_semantics import CASES

pytestmark = pytest.mark.gpu

ARGS = 1 << 8   # RWKV_ERROR_ARGS


def _synth(tmp_path, name, fmt, seed=7):
    library()
    p = str(tmp_path / f"{name}-{fmt}.bin")
    synth.write_model(p, synth.CONFIGS[name], fmt, seed=seed)
    return p


def _tok(step, row, V):
    return (37 * step + 11 * row + 5) % V


def _check_rows(om, b, slots, tokens, ostates, what):
    """One batch call; each row against the oracle stepping that slot alone (ostates: slot -> oracle state, advanced in place)."""
    lg = b.eval(slots, tokens)
    for i, (s, t) in enumerate(zip(slots, tokens)):
        ol, ostates[s] = om.eval(t, ostates[s])
        assert np.array_equal(lg[i], ol), (what, i, s, float(np.abs(lg[i] - ol).max()))
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
    for step in range(6):
        slots = list(range(5))
        toks = [_tok(step, s, V) for s in slots]
        lg = _check_rows(om, b, slots, toks, ost, (version, fmt, step))
        for i, s in enumerate(slots):   # rwkv_eval on a context doing the same
            cl, gst[s] = m.eval(toks[i], gst[s])
            assert np.array_equal(lg[i], cl), (version, fmt, step, s)
    for s in range(5):
        st = b.state_store(s)
        assert np.array_equal(st, ost[s]) and np.array_equal(st, gst[s]), (version, fmt, s)
    b.free()
    m.free()
    om.free()


def test_subsets_order_and_rejected_calls(golden_dir):
    path = R.fixture_path(golden_dir, "6v0-3m", "Q5_0")
    m = model(path)
    om = O.OracleModel(path)
    V = m.n_vocab
    b = pkg.RWKVBatch(m, 6)
    ost = {s: om.init_state() for s in range(6)}
    step = 0
    for slots in ([3, 0, 5], [1], [5, 2, 4, 0, 1, 3], [2, 4], [4, 2], [0, 5, 1]):
        before = {s: b.state_store(s) for s in range(6)}
        toks = [_tok(step, s, 128) for s in slots]
        _check_rows(om, b, slots, toks, ost, ("subset", step, slots))
        for s in range(6):
            after = b.state_store(s)
            if s in slots:
                assert np.array_equal(after, ost[s]), (step, s)
            else:
                assert np.array_equal(after, before[s]), ("slot not named but changed", step, s)
        step += 1
    snapshot = {s: b.state_store(s) for s in range(6)}
    bad = [([1, 1], [3, 4]), ([6], [3]), ([0, 9], [1, 2]), ([2], [V]), ([], []), (list(range(6)) + [0], [1] * 7)]
    for slots, toks in bad:
        b.last_error = 0
        with pytest.raises(ValueError):
            b.eval(slots, toks)
        assert b.last_error & ARGS, (slots, toks, b.last_error)
        with pytest.raises(ValueError):
            b.decode_greedy(slots, toks, 3)
        assert b.last_error & ARGS, (slots, toks, b.last_error)
    for s in range(6):
        assert np.array_equal(b.state_store(s), snapshot[s]), ("a rejected call changed a slot", s)
    # and the batch still works afterwards
    _check_rows(om, b, [2, 0], [9, 10], ost, "after rejected calls")
    b.free()
    m.free()
    om.free()


@pytest.mark.parametrize("name,fmt", [("test-v4", "Q5_1"), ("test-v5.2", "FP16"), ("test-v6", "Q4_0"), ("test-v6", "Q8_0"), ("test-v7", "Q5_1")])
def test_both_product_paths(tmp_path, name, fmt):
    # n < 32: k_mvq_tn / k_mvf; n >= 32: k_mmq_mfma / k_mmfx_seq
    p = _synth(tmp_path, name, fmt)
    m = model(p)
    om = O.OracleModel(p)
    V = m.n_vocab
    b = pkg.RWKVBatch(m, 64)
    for n in (1, 31, 32, 33, 64):
        slots = list(range(64 - n, 64))[::-1] if n % 2 else list(range(n))
        for s in slots:
            b.state_load(s, None)
        ost = {s: om.init_state() for s in slots}
        for step in range(3):
            _check_rows(om, b, slots, [_tok(step + n, s, V) for s in slots], ost, (name, fmt, n, step))
        for s in slots[:: max(1, n // 8)]:
            assert np.array_equal(b.state_store(s), ost[s]), (name, fmt, n, s)
    b.free()
    m.free()
    om.free()


@pytest.mark.parametrize("name,fmt", [("mega-v6-4096", "Q4_0"), ("slice-v7-2560", "Q5_1"), ("slice-v4-768", "Q5_1")])
def test_real_geometry(tmp_path, name, fmt):
    p = _synth(tmp_path, name, fmt, seed=3)
    m = model(p)
    om = O.OracleModel(p)
    V = m.n_vocab
    b = pkg.RWKVBatch(m, 48)
    for n in (8, 48):
        slots = list(range(n))
        for s in slots:
            b.state_load(s, None)
        ost = {s: om.init_state() for s in slots}
        for step in range(3):
            _check_rows(om, b, slots, [(_tok(step, s, V) * 97) % V for s in slots], ost, (name, fmt, n, step))
        for s in (0, n - 1):
            assert np.array_equal(b.state_store(s), ost[s]), (name, fmt, n, s)
    b.free()
    m.free()
    om.free()


@pytest.mark.parametrize("name,fmt", [("test-v6", "Q5_1"), ("test-v7", "Q5_1"), ("test-v4", "Q8_0"), ("mega-v6-2048-v64k", "Q4_0")])
def test_greedy_loop(tmp_path, name, fmt):
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
        toks, ms = b.decode_greedy(slots, first, 16)
        assert toks.shape == (n, 16) and ms > 0.0
        for i, s in enumerate(slots):
            m.state_load(start[s])
            ref, _ = m.decode_greedy(first[i], 16)
            assert np.array_equal(toks[i], ref), (name, fmt, n, s, list(toks[i]), list(ref))
            assert np.array_equal(b.state_store(s), m.state_store()), (name, fmt, n, s)
    b.free()
    m.free()


@pytest.mark.parametrize("name,fmt", [("test-v6", "Q5_1"), ("test-v7", "Q4_0")])
def test_context_interop(tmp_path, name, fmt):
    p = _synth(tmp_path, name, fmt, seed=13)
    m = model(p)
    om = O.OracleModel(p)
    V = m.n_vocab
    prompt = [(17 * i + 3) % V for i in range(40)]
    b = pkg.RWKVBatch(m, 4)
    m.eval_sequence(prompt, None)          # prefill on the context: its resident state
    b.from_context(2, m)
    _, ost = om.eval_sequence(prompt, om.init_state())
    o0 = om.init_state()
    for step, (ta, tb) in enumerate([(5, 6), (7, 8), (9, 10)]):
        lg = b.eval([0, 2], [ta, tb])
        ol0, o0 = om.eval(ta, o0)
        ol2, ost = om.eval(tb, ost)
        assert np.array_equal(lg[0], ol0) and np.array_equal(lg[1], ol2), (name, step)
    b.to_context(2, m)
    toks, _ = m.decode_greedy(11, 12)
    tok, ref = 11, []
    for _ in range(12):
        ol, ost = om.eval(tok, ost)
        tok = int(np.argmax(ol))
        ref.append(tok)
    assert list(toks) == ref, (list(toks), ref)
    assert np.array_equal(m.state_store(), ost)
    b.free()
    m.free()
    om.free()


def test_next_to_persistent_kernel(tmp_path, monkeypatch):
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
    for rnd in range(3):
        toks, _ = m.decode_greedy(tok, 4)
        ref = []
        for _ in range(4):
            ol, cst = om.eval(tok, cst)
            tok = int(np.argmax(ol))
            ref.append(tok)
        assert list(toks) == ref, (rnd, list(toks), ref)
        _check_rows(om, b, slots, [_tok(rnd, s, V) for s in slots], ost, ("beside path 2", rnd))
        assert m.healthy()
    assert np.array_equal(m.state_store(), cst)
    assert m.decode_path() == 2 and m.healthy()
    b.free()
    m.free()
    om.free()
