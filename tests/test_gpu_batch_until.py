"""Stop sequences and per-row token budgets in the batch decode loops (rwkv_mi_batch_decode_until; csrc/sampling.hip k_draw_rows<plain, 0, 0> and
k_draw_rows<pen, 0, 0> behind their live words, k_stop_rows; csrc/kernels.hip k_argmax_live). The oracle is the unchanged plain loop of the same family plus matching
on the host: the plain loop runs on a twin batch for the full budget, each row's expected length and reason are computed from its tokens by
test_cpu_batch_until.stop_rule, and the plain loop runs again on fresh twins with n_tokens = len[r] for what the slot must hold. Every
comparison is exact.

A slot's draw counter cannot be read back; it is pinned through what it decides: one more generator draw (u < 0) must give the token the twin gives."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_lib import library, model, pkg, synth
from test_cpu_batch_until import NO_TOKEN, stop_rule

pytestmark = pytest.mark.gpu

ARGS = 1 << 8   # RWKV_ERROR_ARGS
MODELS = [("test-v4", "Q8_0"), ("test-v6", "Q5_1"), ("test-v7", "Q5_1"), ("mega-v6-2048-v64k", "Q4_0")]
FAMILIES = ("greedy", "sample", "pen")
NEG = -999999999.0
N_SLOTS = 7
SLOTS = [4, 1, 5, 0, 2, 6]   # (slot 3 is not named)
BUDGET = 24
K = 16                       # the default block of the loop
# one row of parameters per row of SLOTS; temperatures at or above 1: the rows' tokens differ
T = [1.0, 1.2, 1.5, 1.0, 2.0, 1.3]
P = [0.9, 1.0, 0.95, 0.0, 1.0, 0.85]
SEEDS = [7, 8, 9, 10, 11, 12]
PRESENCE = [0.2, 0.25, 0.0, 1.5, 0.2, 0.7]
FREQUENCY = [0.2, 0.5, 0.3, 0.0, 0.2, 0.1]
P_U32 = ctypes.POINTER(ctypes.c_uint32)


def _tok(step, row, V):
    return (37 * step + 11 * row + 5) % V


def _synth(tmp_path, name, fmt, seed=17):
    library()
    p = str(tmp_path / f"{name}-{fmt}.bin")
    synth.write_model(p, synth.CONFIGS[name], fmt, seed=seed)
    return p


def _prepare(b, family, V):
    """What every batch of a comparison starts from: a token in every slot, a second one in three of them (mixed parities), and for the
    penalised family a history, a draw counter and, on one slot, a bias."""
    every = list(range(N_SLOTS))
    b.eval(every, [_tok(1, s, V) for s in every], want_logits=False)
    b.eval([1, 5, 3], [_tok(2, s, V) for s in (1, 5, 3)], want_logits=False)
    if family == "pen":
        for s in every:
            b.counts_add(s, [(5 * s + 3 * i) % min(V, 50) for i in range(12)])
            b.rng_seek(s, 3 * s + 1)
        b.set_logit_bias(4, {3: NEG, 17: 2.0})


def _fresh(m, family):
    b = pkg.RWKVBatch(m, N_SLOTS)
    _prepare(b, family, m.n_vocab)
    return b


def _rows_of(rows, v):
    return [v[i] for i in rows]


def _plain(b, family, rows, first, n_tokens):
    """The plain loop of the family on the rows `rows` (indices into SLOTS and the parameter rows): tokens [len(rows)][n_tokens]."""
    slots = _rows_of(rows, SLOTS)
    if family == "greedy":
        return b.decode_greedy(slots, first, n_tokens)[0]
    if family == "sample":
        return b.decode_sample(slots, first, n_tokens, _rows_of(rows, T), _rows_of(rows, P), _rows_of(rows, SEEDS))[0]
    return b.decode_sample_penalized(slots, first, n_tokens, _rows_of(rows, T), _rows_of(rows, P), _rows_of(rows, SEEDS), _rows_of(rows, PRESENCE),
                                     _rows_of(rows, FREQUENCY))[0]


def _family_args(family, rows):
    n = len(rows)
    params = None if family == "greedy" else pkg.sample_params(n, _rows_of(rows, T), _rows_of(rows, P), -1.0, _rows_of(rows, SEEDS))
    pens = pkg.penalty_params(n, _rows_of(rows, PRESENCE), _rows_of(rows, FREQUENCY), True) if family == "pen" else None
    return params, pens


def _call(b, slots, first, params, pens, sp, seq_lens, seq_tokens, stride, override=None):
    """rwkv_mi_batch_decode_until through the C ABI with every output given: (ok, tokens [n][stride], lens [n], stopped_by [n]). override:
    arguments to replace (n, stride, or a pointer by None)."""
    s, t = np.asarray(slots, dtype=np.uint32), np.asarray(first, dtype=np.uint32)
    n = s.size
    toks = np.zeros((max(n, 1), max(stride, 1)), dtype=np.uint32)
    lens = np.zeros(max(n, 1), dtype=np.uint32)
    why = np.zeros(max(n, 1), dtype=np.uint32)
    a = dict(slots=s.ctypes.data_as(P_U32), first=t.ctypes.data_as(P_U32), n=n, params=params, pens=pens, sp=sp,
             seq_lens=seq_lens.ctypes.data_as(P_U32), seq_tokens=seq_tokens.ctypes.data_as(P_U32), stride=stride,
             tokens_out=toks.ctypes.data_as(P_U32), lens_out=lens.ctypes.data_as(P_U32), why_out=why.ctypes.data_as(P_U32))
    a.update(override or {})
    ok = b._L.rwkv_mi_batch_decode_until(b._ptr, a["slots"], a["first"], a["n"], a["params"], a["pens"], a["sp"], a["seq_lens"], a["seq_tokens"],
                                         a["stride"], a["tokens_out"], a["lens_out"], a["why_out"], None)
    return bool(ok), toks, lens, why


def _until(b, family, slots, first, max_tokens, stop, stride=None, rows=None):
    """decode_until of the family on the named slots (rows: their rows of the parameter tables; default: SLOTS' order): tokens [n][stride]
    as the library wrote them, lens, stopped_by."""
    rows = list(range(len(slots))) if rows is None else rows
    params, pens = _family_args(family, rows)
    sp, seq_lens, seq_tokens = pkg.stop_params(len(slots), max_tokens, stop)
    stride = max(r.max_tokens for r in sp) if stride is None else stride
    ok, toks, lens, why = _call(b, slots, first, params, pens, sp, seq_lens, seq_tokens, stride)
    assert ok, "rwkv_mi_batch_decode_until failed"
    return toks, lens, why


def _window(row, width, parity, avoid):
    """The `width`-token window of a row's stream whose stop_rule length has the given parity, is not in `avoid` and is the largest such up
    to 13 (streams of tiny models can be periodic: a window then matches long before the place it was cut from); any window failing that."""
    best = None
    for end in range(width, BUDGET):
        q = row[end - width: end]
        L = stop_rule(row, BUDGET, [q])[0]
        if L & 1 == parity and L not in avoid and L <= 13 and (best is None or L > best[0]):
            best = (L, q)
    return best[1] if best else row[4: 4 + width]


def _choose_stops(full, V, every_row_stops=False):
    """Per-row stop lists chosen from what the full-budget plain loop emitted (full: [6][BUDGET]): row 0 retires after pass 0; row 1 by a
    two-token sequence, at an even length; row 2 by a three-token sequence, at an odd one; row 3 by an overlapping one ([a, a] where its
    stream repeats a token, else two sequences that match at the same step); row 4 meets only its budget; row 5 has a stop token that
    never occurs. every_row_stops: rows 4 and 5 get a stop from the end of their streams as well (every row retires by pass BUDGET)."""
    f = [[int(t) for t in r] for r in full]
    stop = [[[f[0][0]]], [_window(f[1], 2, 0, (1, BUDGET))]]
    stop.append([_window(f[2], 3, 1, (1, BUDGET))])
    rep = [i for i in range(1, BUDGET) if f[3][i] == f[3][i - 1]]
    stop.append([[f[3][rep[0]]] * 2] if rep else [[f[3][10], f[3][11]], [f[3][11]]])
    absent = next(t for t in range(V) if t not in f[5])
    stop.append([[f[4][BUDGET - 1]]] if every_row_stops else [])
    stop.append([[absent], [f[5][BUDGET - 2], f[5][BUDGET - 1]]] if every_row_stops else [[absent]])
    return stop


def _expected(full, max_tokens, stop):
    want = [stop_rule(full[r], max_tokens[r] if isinstance(max_tokens, list) else max_tokens, stop[r]) for r in range(len(stop))]
    return [w[0] for w in want], [w[1] for w in want]


def _assert_spread(lens):
    assert len(set(lens)) >= 4 and len({l & 1 for l in lens}) == 2, ("the rows must retire at four distinct lengths of both parities", lens)


def _twins_by_length(m, family, first, lens):
    """{length: (twin batch, rows)}: a fresh batch per distinct length on which the plain loop of that length has run the rows of that length."""
    out = {}
    for L in sorted(set(lens)):
        rows = [r for r in range(len(lens)) if lens[r] == L]
        tw = _fresh(m, family)
        toks = _plain(tw, family, rows, _rows_of(rows, first), L)
        out[L] = (tw, rows, toks)
    return out


def _check_guarantee(m, family, name, draws):
    V = m.n_vocab
    first = [_tok(0, s, V) for s in SLOTS]
    every = list(range(len(SLOTS)))
    ref = _fresh(m, family)
    full = _plain(ref, family, every, first, BUDGET)
    ref.free()
    stop = _choose_stops(full, V)
    lens_want, why_want = _expected(full, BUDGET, stop)
    _assert_spread(lens_want)
    assert lens_want[0] == 1 and why_want[4] == NO_TOKEN and lens_want[4] == BUDGET and lens_want[5] == BUDGET, (lens_want, why_want)
    b = _fresh(m, family)
    untouched = b.state_store(3)
    toks, lens, why = _until(b, family, SLOTS, first, BUDGET, stop)
    assert lens.tolist() == lens_want and why.tolist() == why_want, (name, family, lens.tolist(), lens_want, why.tolist(), why_want)
    assert b.last_loop_passes() == BUDGET
    for r in every:
        assert np.array_equal(toks[r, : lens[r]], full[r, : lens[r]]), (name, family, r)
        assert (toks[r, lens[r]:] == NO_TOKEN).all(), (name, family, r, "no token past the row's length")
    assert np.array_equal(b.state_store(3), untouched), (name, family, "the slot that was not named")
    twins = _twins_by_length(m, family, first, lens_want)
    for L, (tw, rows, ptoks) in twins.items():
        slots = _rows_of(rows, SLOTS)
        for i, r in enumerate(rows):
            assert np.array_equal(ptoks[i], toks[r, :L]), (name, family, r, L)
            assert np.array_equal(b.state_store(SLOTS[r]), tw.state_store(SLOTS[r])), (name, family, r, L, "state")
            if family == "pen":
                assert np.array_equal(b.counts(SLOTS[r]), tw.counts(SLOTS[r])), (name, family, r, L, "a retired row must not record")
        last = [int(toks[r, L - 1]) for r in rows]
        if not draws:
            # continuing by one eval of the last token: the batch reads the buffer its parity names
            assert np.array_equal(b.eval(slots, last), tw.eval(slots, last)), (name, family, L, "parity")
        elif family == "sample":
            got = b.eval_sample(slots, last, 1.0, 1.0, -1.0, _rows_of(rows, SEEDS))
            assert np.array_equal(got, tw.eval_sample(slots, last, 1.0, 1.0, -1.0, _rows_of(rows, SEEDS))), (name, family, L, "draw counter")
        elif family == "pen":
            a = (slots, last, 1.0, 1.0, -1.0, _rows_of(rows, SEEDS), _rows_of(rows, PRESENCE), _rows_of(rows, FREQUENCY), False)
            assert np.array_equal(b.eval_sample_penalized(*a), tw.eval_sample_penalized(*a)), (name, family, L, "draw counter")
        tw.free()
    b.free()


# ---- 1. the guarantee ----

@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name,fmt", MODELS)
def test_retired_rows_are_what_the_plain_loop_of_their_length_leaves(tmp_path, name, fmt, family):
    m = model(_synth(tmp_path, name, fmt))
    _check_guarantee(m, family, name, draws=False)
    m.free()


# ---- 2. the draw counter and the counts survive retirement ----

@pytest.mark.parametrize("family", ("sample", "pen"))
def test_draw_counters_and_counts_survive_retirement(tmp_path, family):
    m = model(_synth(tmp_path, "test-v6", "Q5_1"))
    _check_guarantee(m, family, "test-v6", draws=True)
    m.free()


# ---- 3. no sequences, equal budgets: the plain loop ----

def test_without_sequences_the_call_is_the_plain_loop(tmp_path):
    m = model(_synth(tmp_path, "test-v6", "Q5_1"))
    V = m.n_vocab
    first = [_tok(0, s, V) for s in SLOTS]
    every = list(range(len(SLOTS)))
    n_tokens = K + 1   # (odd, and one pass into the second block)
    results = {}
    for family in FAMILIES:
        b, tw = _fresh(m, family), _fresh(m, family)
        toks, lens, why = _until(b, family, SLOTS, first, n_tokens, None)
        want = _plain(tw, family, every, first, n_tokens)
        assert lens.tolist() == [n_tokens] * len(SLOTS) and why.tolist() == [NO_TOKEN] * len(SLOTS), (family, lens, why)
        assert np.array_equal(toks, want), family
        for s in range(N_SLOTS):
            assert np.array_equal(b.state_store(s), tw.state_store(s)), (family, s)
        results[family] = toks
        b.free()
        tw.free()
    # penalties zero and no bias: the penalised form is the sampled form (the draw counters start from 0 in both)
    b = _fresh(m, "sample")
    params = pkg.sample_params(len(SLOTS), T, P, -1.0, SEEDS)
    sp, seq_lens, seq_tokens = pkg.stop_params(len(SLOTS), n_tokens, None)
    ok, toks, lens, why = _call(b, SLOTS, first, params, pkg.penalty_params(len(SLOTS), 0.0, 0.0, True), sp, seq_lens, seq_tokens, n_tokens)
    assert ok and np.array_equal(toks, results["sample"])
    b.free()
    m.free()


# ---- 4. ending early ----

def _spec(family, first, max_tokens, stop, stride):
    return dict(family=family, slots=SLOTS, first=first, max_tokens=max_tokens, stop=stop, stride=stride)


def test_the_loop_ends_when_every_row_has_retired(tmp_path):
    path = _synth(tmp_path, "test-v6", "Q5_1")
    m = model(path)
    V = m.n_vocab
    family = "sample"
    first = [_tok(0, s, V) for s in SLOTS]
    ref = _fresh(m, family)
    full = _plain(ref, family, list(range(len(SLOTS))), first, BUDGET)
    ref.free()
    stop = _choose_stops(full, V, every_row_stops=True)
    lens_want, why_want = _expected(full, 4096, stop)
    assert max(lens_want) <= BUDGET and NO_TOKEN not in why_want, (lens_want, why_want)
    b = _fresh(m, family)
    os.environ.pop("RWKV_MI_LOOP_BLOCK", None)
    toks, lens, why = _until(b, family, SLOTS, first, 4096, stop, stride=4096)
    passes = b.last_loop_passes()
    assert lens.tolist() == lens_want and why.tolist() == why_want, (lens.tolist(), lens_want, why.tolist(), why_want)
    assert passes <= max(lens_want) + 2 * K, (passes, lens_want)
    states = np.stack([b.state_store(s) for s in SLOTS])
    b.free()
    m.free()
    # the same call in blocks of one pass, in a fresh process
    spec, out = str(tmp_path / "spec.json"), str(tmp_path / "out.npz")
    json.dump(_spec(family, first, 4096, stop, 4096), open(spec, "w"))
    env = dict(os.environ, RWKV_MI_LOOP_BLOCK="1")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "until_worker.py")
    subprocess.run([sys.executable, worker, path, spec, out], check=True, env=env, timeout=300)
    got = np.load(out)
    assert int(got["passes"]) <= max(lens_want) + 2, (int(got["passes"]), lens_want)
    assert np.array_equal(got["tokens"], toks) and np.array_equal(got["lens"], lens) and np.array_equal(got["why"], why)
    assert np.array_equal(got["states"], states)


# ---- 5. independence of company ----

def test_a_row_alone_is_the_row_in_company(tmp_path):
    m = model(_synth(tmp_path, "test-v6", "Q5_1"))
    V = m.n_vocab
    family = "pen"
    first = [_tok(0, s, V) for s in SLOTS]
    ref = _fresh(m, family)
    full = _plain(ref, family, list(range(len(SLOTS))), first, BUDGET)
    ref.free()
    stop = _choose_stops(full, V)
    b = _fresh(m, family)
    toks, lens, why = _until(b, family, SLOTS, first, BUDGET, stop)
    for r, s in enumerate(SLOTS):
        solo = _fresh(m, family)
        t1, l1, w1 = _until(solo, family, [s], [first[r]], BUDGET, [stop[r]], rows=[r])
        assert int(l1[0]) == int(lens[r]) and int(w1[0]) == int(why[r]) and np.array_equal(t1[0], toks[r]), (r, l1, lens[r])
        assert np.array_equal(solo.state_store(s), b.state_store(s)) and np.array_equal(solo.counts(s), b.counts(s)), r
        solo.free()
    b.free()
    m.free()


# ---- 6. rejections ----

def test_rejections_change_nothing(tmp_path):
    m = model(_synth(tmp_path, "test-v6", "Q5_1"))
    V = m.n_vocab
    n = len(SLOTS)
    b, tw = _fresh(m, "pen"), _fresh(m, "pen")
    first = [_tok(0, s, V) for s in SLOTS]
    params, pens = _family_args("pen", list(range(n)))
    stop = [[[1], [2, 3]]] + [[]] * (n - 1)
    sp, seq_lens, seq_tokens = pkg.stop_params(n, 8, stop)
    u32 = lambda v: np.asarray(v, dtype=np.uint32)   # noqa: E731

    def stops(max_tokens=8, n_seqs0=2):
        arr = (pkg.StopParams * n)()
        for i in range(n):
            arr[i] = pkg.StopParams(max_tokens[i] if isinstance(max_tokens, list) else max_tokens, n_seqs0 if i == 0 else 0)
        return arr

    def rejected(what, slots=SLOTS, first_=first, params_=params, pens_=pens, sp_=sp, sl=seq_lens, st=seq_tokens, stride=8, **override):
        ok, _, _, _ = _call(b, slots, first_, params_, pens_, sp_, sl, st, stride, override)
        err = m._library.rwkv_get_last_error(m._ctx)
        assert not ok and err & ARGS, (what, ok, err)

    # what the plain loops reject
    rejected("n == 0", n=0)
    rejected("n > n_slots", n=N_SLOTS + 1)
    rejected("a slot out of range", slots=[4, 1, 5, 0, 2, N_SLOTS])
    rejected("a slot twice", slots=[4, 1, 5, 0, 2, 4])
    rejected("a token out of range", first_=first[:-1] + [V])
    rejected("a negative temperature", params_=pkg.sample_params(n, [1.0] * (n - 1) + [-1.0], 0.8, -1.0, 0))
    rejected("a top_p above 1", params_=pkg.sample_params(n, 1.0, [0.8] * (n - 1) + [1.5], -1.0, 0))
    rejected("a penalty that is not finite", pens_=pkg.penalty_params(n, [0.2] * (n - 1) + [float("inf")], 0.2, True))
    # what this call adds
    rejected("stops NULL", sp=None)
    rejected("lens_out NULL", lens_out=None)
    rejected("penalties without params", params_=None)
    rejected("a max_tokens of 0", sp_=stops([8, 8, 0, 8, 8, 8]))
    rejected("stride below the largest max_tokens", sp_=stops([8, 8, 9, 8, 8, 8]))
    rejected("stride below max_tokens", stride=7)
    rejected("n_seqs above the limit", sp_=stops(8, 17), sl=u32([1] * 17), st=u32([1] * 17))
    rejected("seq_lens NULL", seq_lens=None)
    rejected("seq_tokens NULL", seq_tokens=None)
    rejected("a sequence of length 0", sl=u32([1, 0]))
    rejected("a sequence longer than the limit", sl=u32([1, 9]), st=u32([1] * 10))
    rejected("a sequence token out of range", st=u32([1, 2, V]))
    # nothing moved: state, counts and the next generator draw of the named slots
    for s in SLOTS:
        assert np.array_equal(b.state_store(s), tw.state_store(s)), s
        assert np.array_equal(b.counts(s), tw.counts(s)), s
    a = (SLOTS, first, 1.0, 1.0, -1.0, SEEDS, PRESENCE, FREQUENCY, False)
    assert np.array_equal(b.eval_sample_penalized(*a), tw.eval_sample_penalized(*a))
    # ... and the same call with nothing wrong goes through
    ok, _, lens, _ = _call(b, SLOTS, [int(t) for t in first], params, pens, sp, seq_lens, seq_tokens, 8)
    assert ok and (lens >= 1).all() and (lens <= 8).all()
    b.free()
    tw.free()
    m.free()
