"""The ragged form of per-position scoring (rwkv_mi_batch_score_ragged): row i feeds lens[i] tokens to its slot, all rows in one pass, and
every token of the pass gets its log-prob / argmax. Every slot is held, bit for bit (np.array_equal / identical bytes), to
rwkv_mi_score_resident of its tokens alone on a context, and its state to the CPU oracle stepping that sequence alone. The log-prob's own
accuracy against float64 is held in tests/test_gpu_score.py; here nothing has a tolerance."""
import ctypes

import numpy as np
import pytest

import oracle_lib as O
import reference_constants as R
from gpu_lib import library, model, pkg, synth

pytestmark = pytest.mark.gpu

ARGS = 1 << 8   # RWKV_ERROR_ARGS
NO_TARGET = 0xFFFFFFFF
P_UINT32 = ctypes.POINTER(ctypes.c_uint32)
P_FLOAT = ctypes.POINTER(ctypes.c_float)
LENS = (1, 2, 31, 40, 33)


def _toks(call, slot, n, V):
    return [(37 * call + 11 * slot + 29 * j + 5) % V for j in range(n)]


def _targets(call, slot, n, V):
    t = [(53 * call + 7 * slot + 31 * j + 2) % V for j in range(n)]
    if n > 2:
        t[n // 2] = NO_TARGET
    return t


def _oracle_state(om, state, toks):
    for t in toks:
        _, state = om.eval(t, state)
    return state


def _alone(m, state, toks, tgts):
    """score_resident of one sequence alone on the context, from `state`"""
    m.state_load(state)
    lp, am, _ = m.score_resident(toks, tgts)
    return lp, am


def _check_call(m, om, b, slots, rows, tgts, ost, what):
    """One score_ragged call; each row against the context alone and the oracle's state (ost: slot -> oracle state, advanced in place)."""
    lps, ams = b.score_ragged(slots, rows, tgts)
    assert len(lps) == len(ams) == len(slots)
    for i, s in enumerate(slots):
        lp, am = _alone(m, ost[s], rows[i], tgts[i])
        assert lps[i].tobytes() == lp.tobytes(), (what, "logprobs", i, s, len(rows[i]))
        assert np.array_equal(ams[i], am), (what, "argmax", i, s, len(rows[i]))
        ost[s] = _oracle_state(om, ost[s], rows[i])
        assert np.array_equal(m.state_store(), ost[s]), (what, "context state", s)
        assert np.array_equal(b.state_store(s), ost[s]), (what, "slot state", s)
    return lps, ams


def _synth(tmp_path, name, fmt, seed=7):
    library()
    p = str(tmp_path / f"{name}-{fmt}.bin")
    synth.write_model(p, synth.CONFIGS[name], fmt, seed=seed)
    return p


def _golden_or_synth(golden_dir, tmp_path, name, fmt):
    return R.fixture_path(golden_dir, name, fmt) if name[0].isdigit() else _synth(tmp_path, name, fmt)


@pytest.mark.parametrize("name,fmt", [("6v0-3m", "Q5_1"), ("7v0-834K", "FP16"), ("4v0-660K", "Q5_0"), ("5v2-730K", "FP32"), ("test-v6", "Q4_0"), ("test-v7", "Q5_1")])
def test_each_slot_equals_the_sequence_alone(golden_dir, tmp_path, name, fmt):
    path = _golden_or_synth(golden_dir, tmp_path, name, fmt)
    m = model(path)
    om = O.OracleModel(path)
    V = m.n_vocab
    b = pkg.RWKVBatch(m, 8)
    untouched = {s: b.state_store(s) for s in (5, 6, 7)}
    ost = {s: om.init_state() for s in range(8)}
    slots = [3, 0, 4, 1, 2]
    rows = [_toks(0, s, n, V) for s, n in zip(slots, LENS)]
    tgts = [_targets(0, s, n, V) for s, n in zip(slots, LENS)]
    assert sum(LENS) == 107
    _check_call(m, om, b, slots, rows, tgts, ost, (name, fmt, "first call"))
    for s in untouched:   # slots not named are untouched
        assert np.array_equal(b.state_store(s), untouched[s]), (name, fmt, "slot not named but changed", s)
    # the parity rule: a second call continues from what the first one left, the lengths moved round the slots
    lens2 = LENS[2:] + LENS[:2]
    rows2 = [_toks(1, s, n, V) for s, n in zip(slots, lens2)]
    tgts2 = [_targets(1, s, n, V) for s, n in zip(slots, lens2)]
    _check_call(m, om, b, slots, rows2, tgts2, ost, (name, fmt, "second call"))
    for s in untouched:
        assert np.array_equal(b.state_store(s), untouched[s]), (name, fmt, "slot not named but changed", s)
    # ... and the plain ragged pass continues from a scoring pass as from any other
    lg = b.eval_ragged([0], [[9, 8, 7]])
    m.state_load(ost[0])
    assert np.array_equal(lg[0], m.eval_resident([9, 8, 7]))
    # argmax alone, log-probs alone: the same values
    twin = pkg.RWKVBatch(m, 8)
    lps, ams = twin.score_ragged(slots, rows, tgts)
    twin2 = pkg.RWKVBatch(m, 8)
    none, ams2 = twin2.score_ragged(slots, rows)
    assert none is None and all(np.array_equal(a, c) for a, c in zip(ams, ams2))
    twin3 = pkg.RWKVBatch(m, 8)
    lps3, none = twin3.score_ragged(slots, rows, tgts, want_argmax=False)
    assert none is None and all(a.tobytes() == c.tobytes() for a, c in zip(lps, lps3))
    for t in (twin, twin2, twin3):
        t.free()
    b.free()
    m.free()
    om.free()


@pytest.mark.parametrize("name,fmt", [("test-v6", "Q4_0"), ("test-v7", "Q5_1"), ("test-v4", "Q5_1"), ("test-v5.2", "FP16")])
def test_a_sequence_cut_over_three_calls_equals_the_whole(tmp_path, name, fmt):
    p = _synth(tmp_path, name, fmt, seed=11)
    m = model(p)
    om = O.OracleModel(p)
    V = m.n_vocab
    prompt = [(17 * i + 3) % V for i in range(75)]
    ptg = [(19 * i + 1) % V for i in range(75)]
    whole, cut = pkg.RWKVBatch(m, 4), pkg.RWKVBatch(m, 4)
    wl, wa = whole.score_ragged([1], [prompt], [ptg])
    ost = {s: om.init_state() for s in range(4)}
    # 32 + 1 + 42 over three calls that also carry other rows
    c1 = _check_call(m, om, cut, [0, 1, 2], [[5], prompt[:32], [7, 8, 9]], [[1], ptg[:32], [2, 3, 4]], ost, (name, fmt, "chunk 1"))
    c2 = _check_call(m, om, cut, [1, 3], [prompt[32:33], _toks(1, 3, 40, V)], [ptg[32:33], _targets(1, 3, 40, V)], ost, (name, fmt, "chunk 2"))
    c3 = _check_call(m, om, cut, [2, 0, 1], [[4], [6, 7], prompt[33:]], [[5], [6, 7], ptg[33:]], ost, (name, fmt, "chunk 3"))
    assert np.concatenate([c1[0][1], c2[0][0], c3[0][2]]).tobytes() == wl[0].tobytes(), (name, fmt, "logprobs")
    assert np.array_equal(np.concatenate([c1[1][1], c2[1][0], c3[1][2]]), wa[0]), (name, fmt, "argmax")
    assert np.array_equal(whole.state_store(1), cut.state_store(1)), (name, fmt)
    # ... and the whole equals the context alone
    lp, am = _alone(m, None, prompt, ptg)
    assert lp.tobytes() == wl[0].tobytes() and np.array_equal(am, wa[0])
    whole.free()
    cut.free()
    m.free()
    om.free()


def test_rejected_calls_change_nothing(golden_dir):
    path = R.fixture_path(golden_dir, "6v0-3m", "Q5_0")
    m = model(path)
    V = m.n_vocab
    b = pkg.RWKVBatch(m, 6)
    slots6 = [5, 2, 4, 0, 1, 3]
    rows6 = [_toks(0, s, 1 + s, 128) for s in slots6]
    b.score_ragged(slots6, rows6, [_targets(0, s, 1 + s, 128) for s in slots6])
    snapshot = {s: b.state_store(s) for s in range(6)}
    long_bad = _toks(1, 0, 40, 128)
    long_bad[23] = V                                     # a token >= n_vocab in the middle of a long segment
    ok40 = _toks(1, 0, 40, 128)
    bad_target = _targets(1, 0, 40, 128)
    bad_target[23] = V                                   # a target >= n_vocab that is not NO_TARGET
    bad = [
        ([0, 1], [[3], []], [[3], []]),                  # a zero length
        ([1, 1], [[3, 4], [5]], [[3, 4], [5]]),          # a repeated slot
        ([6], [[3, 4]], [[3, 4]]),                       # a slot out of range
        ([0, 9], [[1], [2, 3]], [[1], [2, 3]]),
        ([2, 3], [[1, 2], long_bad], [[1, 2], ok40]),
        ([2], [[V]], [[1]]),
        ([], [], []),                                    # n = 0
        (list(range(6)) + [0], [[1, 2]] * 7, [[1, 2]] * 7),   # n > n_slots
        ([2, 3], [[1, 2], ok40], [[1, 2], bad_target]),
        ([2], [[1]], [[V]]),
        ([2], [[1]], [[0xFFFFFFFE]]),
    ]
    for slots, rows, tgts in bad:
        b.last_error = 0
        with pytest.raises(ValueError):
            b.score_ragged(slots, rows, tgts)
        assert b.last_error & ARGS, (slots, rows, tgts, b.last_error)
    # a bad target is rejected when only the argmax is asked for as well; log-probs without targets; lens == NULL (the entry point directly)
    L, lib = b._L, library()
    s2 = np.array([0, 1], dtype=np.uint32)
    l2 = np.array([1, 2], dtype=np.uint32)
    t2 = np.array([3, 4, 5], dtype=np.uint32)
    g2 = np.array([3, V, 5], dtype=np.uint32)
    lp = np.empty(3, dtype=np.float32)
    am = np.empty(3, dtype=np.uint32)
    u32 = lambda a: a.ctypes.data_as(P_UINT32)   # noqa: E731
    for what, args in {
        "bad target, argmax only": (u32(s2), u32(l2), u32(t2), u32(g2), 2, None, u32(am)),
        "log-probs without targets": (u32(s2), u32(l2), u32(t2), None, 2, lp.ctypes.data_as(P_FLOAT), u32(am)),
        "lens == NULL": (u32(s2), None, u32(t2), u32(t2), 2, lp.ctypes.data_as(P_FLOAT), u32(am)),
        "tokens == NULL": (u32(s2), u32(l2), None, u32(t2), 2, lp.ctypes.data_as(P_FLOAT), u32(am)),
    }.items():
        lib.rwkv_set_print_errors(m._ctx, False)
        ok = L.rwkv_mi_batch_score_ragged(b._ptr, *args)
        lib.rwkv_set_print_errors(m._ctx, True)
        assert not ok and lib.rwkv_get_last_error(m._ctx) & ARGS, what
    for s in range(6):
        assert np.array_equal(b.state_store(s), snapshot[s]), ("a rejected call changed slot", s)
    # the batch goes on as if the bad calls had never been made: against a twin that never saw them
    twin = pkg.RWKVBatch(m, 6)
    twin.score_ragged(slots6, rows6, [_targets(0, s, 1 + s, 128) for s in slots6])
    rows = [_toks(2, s, 3 + s, 128) for s in slots6]
    tg = [_targets(2, s, 3 + s, 128) for s in slots6]
    a, c = b.score_ragged(slots6, rows, tg), twin.score_ragged(slots6, rows, tg)
    for k in range(2):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[k], c[k]))
    for s in range(6):
        assert np.array_equal(b.state_store(s), twin.state_store(s))
    # both outputs NULL: rwkv_mi_batch_eval_ragged(.., NULL)
    assert L.rwkv_mi_batch_score_ragged(b._ptr, u32(s2), u32(l2), u32(t2), None, 2, None, None)
    twin.eval_ragged([0, 1], [[3], [4, 5]], want_logits=False)
    for s in (0, 1):
        assert np.array_equal(b.state_store(s), twin.state_store(s))
    twin.free()
    b.free()
    m.free()
