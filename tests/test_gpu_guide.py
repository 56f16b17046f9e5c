"""Guided decoding (rwkv_mi_batch_guide_*; csrc/sampling.hip k_draw_rows<plain, 1, 1>, k_draw_rows<pen, 1, 1>, k_guide_expand). Everything is
bit for bit. At the kernel level the oracle is the EXISTING sampler (rwkv_mi_test_sample_rows) on the same logits -- for the penalised entry
the adjusted logits of tests/test_gpu_batch_penalty.py -- with -inf written at the positions the guide forbids. At the model level it is
the host-driven loop a caller had to write before: per step, rwkv_mi_batch_logit_bias_set with -inf off the mask, one
rwkv_mi_batch_eval_sample_penalized, the token read back, the automaton stepped on the host (tests/guide_ref.py).

A slot's draw counter cannot be read back; it is pinned through what it decides: one more generator draw must give the token the twin gives."""
import ctypes

import numpy as np
import pytest

import guide_ref as G
from gpu_lib import library, model, pkg
from test_gpu_batch_penalty import NEG, _adjust, _counts_of, _synth
from test_gpu_batch_sample import _sample_rows

pytestmark = pytest.mark.gpu

ARGS = 1 << 8   # RWKV_ERROR_ARGS
NO_GUIDE = 0xFFFFFFFF
SMALL = [("test-v6", "Q5_1"), ("test-v7", "Q5_1"), ("test-v4", "Q8_0")]
MODELS = SMALL + [("mega-v6-2048-v64k", "Q4_0")]
STEPS = 32
P_U32 = ctypes.POINTER(ctypes.c_uint32)
P_F32 = ctypes.POINTER(ctypes.c_float)

_guide_hooks = None


def _guide_hooks_library():
    """lib/librwkv_testhooks_guide.so: the product objects + the guided sampler's test entry point (include/rwkv_testhooks_guide.h)."""
    global _guide_hooks
    if _guide_hooks is None:
        library()   # (builds; and HIP is initialised in the order gpu_lib keeps)
        _guide_hooks = pkg.RWKVSharedLibrary(pkg.GUIDE_HOOKS_LIB_PATH)
    return _guide_hooks


def _guided_rows(logits, guides, row_guide, row_state, params, counters, penalties=None, counts=None, bias=None):
    """rwkv_mi_test_guided_rows: (tokens, states, misses, counters, counts) after one launch of the plain (penalties None) or penalised entry."""
    L = _guide_hooks_library().library
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    R, V = logits.shape
    parts = [g.csr() for g in guides]
    cat = lambda k: np.ascontiguousarray(np.concatenate([p[k] for p in parts]).astype(np.uint32))   # noqa: E731
    begin, toks, nxt = cat(0), cat(1), cat(2)
    n_states = np.asarray([g.n_states for g in guides], dtype=np.uint32)
    rg, rs = np.asarray(row_guide, dtype=np.uint32), np.asarray(row_state, dtype=np.uint32)
    ctr = np.ascontiguousarray(counters, dtype=np.uint64).copy()
    cnt = None if counts is None else np.ascontiguousarray(counts, dtype=np.uint32).copy()
    bs = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
    out, st, ms = (np.empty(R, dtype=np.uint32) for _ in range(3))
    u32 = lambda a: None if a is None else a.ctypes.data_as(P_U32)   # noqa: E731
    ok = L.rwkv_mi_test_guided_rows(logits.ctypes.data_as(P_F32), R, V, len(guides), u32(n_states), u32(begin), u32(toks), u32(nxt), u32(rg), u32(rs), params,
                                    penalties, u32(cnt), None if bs is None else bs.ctypes.data_as(P_F32), ctr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                    u32(out), u32(st), u32(ms))
    assert ok, "rwkv_mi_test_guided_rows failed"
    return out, st, ms, ctr, cnt


def _masked(values, mask):
    """the values a guided row reads: its own where the guide allows the token, -inf elsewhere"""
    return np.where(mask, values, np.float32(-np.inf)).astype(np.float32)


# ---- the two guided row kernels on crafted logits (the test hook) ----

def _hand_built(V):
    """Guide A of the kernel test, three states over a vocabulary the 1024 threads cut into chunks of C tokens. State 0 allows token 0, token
    V - 1 and the first and the last token of some threads' chunks (the first thread's, one in the middle, the last one that holds tokens) and a
    sprinkling of others; state 1 is a single-token state: the first token of a chunk; state 2 allows a random half."""
    C = (V + 1023) // 1024
    last_thread = (V - 1) // C
    special = sorted({0, V - 1, C - 1, C, 37 * C, 37 * C + C - 1, last_thread * C, last_thread * C - 1} & set(range(V)))
    rng = np.random.default_rng(V)
    others = rng.choice(V, size=40, replace=False).tolist()
    s0 = {int(t): int(i % 3) for i, t in enumerate(sorted(set(special) | set(others)))}
    s1 = {500 * C if 500 * C < V else 5 * C: 2}
    s2 = {int(t): int(t % 3) for t in np.flatnonzero(rng.random(V) < 0.5)}
    return G.Guide([s0, s1, s2], V), special


KERNEL_CASES = [(0.0, 1.0), (1.0, 1.0), (0.7, 0.8)]


@pytest.mark.parametrize("V", [1000, 50277, 65536])
@pytest.mark.parametrize("penalised", [False, True], ids=["plain", "pen"])
def test_guided_rows_are_the_sampler_on_masked_logits(V, penalised):
    gA, special = _hand_built(V)
    gB = G.random_guide(V, 3, seed=V + 1)
    gC = G.all_allowed_guide(V, 2)
    guides = [gA, gB, gC]
    row_guide = [0, 0, 1, 2, NO_GUIDE]
    row_state = [0, 1, 2, 1, 0]
    R = 5
    rng = np.random.default_rng(3 * V + int(penalised))
    seeds = [11, 12, 13, 14, 15]
    presence, frequency = [0.2, 0.5, 0.0, 1.5, 0.25], [0.2, 0.25, 0.3, 0.0, 0.5]
    record = [True, True, False, True, True]
    for case, (t, q) in enumerate(KERNEL_CASES):
        logits = (rng.standard_normal((R, V)) * 2.0).astype(np.float32)
        # row 0's favourite is one of the special tokens of its state, another one in every case; an allowed and a forbidden token of rows 1 and 2
        # get a lift as well, so that the mask and not the logits decides
        logits[0, special[(case * 3 + int(penalised)) % len(special)]] += 9.0
        logits[1, 7] += 9.0
        logits[2, int(np.flatnonzero(~gB.mask(2))[0])] += 9.0
        counters = np.asarray([5, 0, 9, 1 << 33, 2], dtype=np.uint64)
        params = pkg.sample_params(R, t, q, -1.0, seeds)
        masks = [guides[g].mask(s) if g != NO_GUIDE else np.ones(V, dtype=bool) for g, s in zip(row_guide, row_state)]
        assert masks[3].all() and masks[1].sum() == 1
        if penalised:
            counts = np.stack([_counts_of(V, rng.integers(0, V, size=30).tolist() + [int(np.argmax(logits[r]))] * 2) for r in range(R)])
            bias = np.zeros((R, V), dtype=np.float32)
            bias[0, special[0]] = 2.0
            bias[2, 5] = NEG
            pens = pkg.penalty_params(R, presence, frequency, record)
            values = np.stack([_adjust(logits[r], counts[r], presence[r], frequency[r], bias[r]) for r in range(R)])
            got, st, ms, ctr, cnt = _guided_rows(logits, guides, row_guide, row_state, params, counters, pens, counts, bias)
        else:
            values = logits
            got, st, ms, ctr, cnt = _guided_rows(logits, guides, row_guide, row_state, params, counters)
        want, want_ctr = _sample_rows(np.stack([_masked(values[r], masks[r]) for r in range(R)]), params, counters, 1)
        print(V, penalised, (t, q), "tokens", got.tolist(), "oracle", want.tolist(), "states", st.tolist(), "misses", ms.tolist())
        assert np.array_equal(got, want), (V, penalised, t, q, got.tolist(), want.tolist())
        assert np.array_equal(ctr, want_ctr), (V, penalised, t, q, ctr.tolist(), want_ctr.tolist())
        # the all-allowed row and the unguided row: the unguided sampler on the untouched values
        free, _ = _sample_rows(values[3:], pkg.sample_params(2, t, q, -1.0, seeds[3:]), counters[3:], 1)
        assert np.array_equal(got[3:], free), (V, penalised, t, q)
        for r in range(R):
            g, s = row_guide[r], row_state[r]
            assert masks[r][got[r]], (V, penalised, t, q, r, "a forbidden token")
            assert (int(st[r]), int(ms[r])) == ((guides[g].step(s, got[r])[0], 0) if g != NO_GUIDE else (s, 0)), (V, penalised, t, q, r)
        if penalised:
            for r in range(R):
                expect = counts[r].copy()
                expect[got[r]] += 1 if record[r] else 0
                assert np.array_equal(cnt[r], expect), (V, r, "counts")


@pytest.mark.parametrize("V", [1000, 65536])
@pytest.mark.parametrize("penalised", [False, True], ids=["plain", "pen"])
def test_all_nan_logits_miss_and_leave_the_state(V, penalised):
    """All-NaN logits are ordinary data for the sampler: its token is 0. On a guided row whose state forbids token 0 that pick is dead: the state
    stays and the miss counter goes up by one."""
    g = G.Guide([{3: 1, V - 1: 0}, {5: 0}], V)
    logits = np.full((2, V), np.nan, dtype=np.float32)
    logits[1] = np.random.default_rng(V).standard_normal(V).astype(np.float32)
    for t in (0.0, 1.0):
        params = pkg.sample_params(2, t, 0.8, -1.0, [1, 2])
        pens = pkg.penalty_params(2, 0.2, 0.2, True) if penalised else None
        counts = np.zeros((2, V), dtype=np.uint32) if penalised else None
        got, st, ms, _, cnt = _guided_rows(logits, [g], [0, 0], [0, 1], params, [0, 0], pens, counts)
        assert (int(got[0]), int(st[0]), int(ms[0])) == (0, 0, 1), (V, penalised, t, got.tolist(), st.tolist(), ms.tolist())
        assert (int(got[1]), int(st[1]), int(ms[1])) == (5, 0, 0), (V, penalised, t, got.tolist(), st.tolist(), ms.tolist())


# ---- model level ----

T = [1.0, 0.7, 1.3, 1.0]
P = [0.9, 1.0, 0.8, 0.0]
SEEDS = [21, 22, 23, 24]
PRESENCE = FREQUENCY = 0.2
SLOTS = [2, 0, 3, 1]
PRE = [4, 4, 8, 15, 16, 23, 42]
START_CTR = 5


def _guides_for(V, seed):
    """two random guides that allow half the vocabulary per state; SLOTS' rows: A / state 1, A / state 3, B / state 0, none"""
    return [G.random_guide(V, 4, seed=seed), G.random_guide(V, 3, seed=seed + 1)], [(0, 1), (0, 3), (1, 0), None]


def _fresh(m, guides, attach, user_bias=None):
    """A 4-slot batch: a token in every slot and a second one in two of them (mixed parities), a history and a draw counter per slot, the
    guides created, SLOTS[i] attached as attach[i] says ((guide index, state) or None)."""
    V = m.n_vocab
    b = pkg.RWKVBatch(m, 4)
    b.eval([0, 1, 2, 3], [(11 * s + 5) % V for s in range(4)], want_logits=False)
    b.eval([1, 3], [(7 * s + 1) % V for s in (1, 3)], want_logits=False)
    ids = [b.create_guide(g.edges) for g in guides]
    for i, s in enumerate(SLOTS):
        b.counts_add(s, PRE)
        b.rng_seek(s, START_CTR)
        if user_bias and user_bias.get(i):
            b.set_logit_bias(s, user_bias[i])
        if attach[i] is not None:
            b.attach_guide(s, ids[attach[i][0]], attach[i][1])
    return b, ids


def _host_loop(m, guides, attach, first, steps, penalised, user_bias=None):
    """The reference: the loop a caller drives from the host, one pass per token. Before every step each guided slot's bias is set to -inf off
    its mask (merged with the slot's own bias), then one eval_sample_penalized (u < 0, the slot's seed; the plain family: zero penalties, nothing
    recorded, the draw counters from 0 as decode_sample starts them), then the automaton steps on the host. Returns (tokens [4][steps],
    the batch, the guide (state, misses) per row)."""
    V = m.n_vocab
    b, _ = _fresh(m, [], [None] * 4)
    where = [None if a is None else [a[1], 0] for a in attach]
    if not penalised:
        for s in SLOTS:
            b.rng_seek(s, 0)
    toks, out = list(first), []
    for _ in range(steps):
        for i, s in enumerate(SLOTS):
            bias = dict((user_bias or {}).get(i) or {})
            if where[i] is not None:
                allowed = guides[attach[i][0]].mask(where[i][0])
                bias = {**{int(t): -np.inf for t in np.flatnonzero(~allowed)}, **{k: v for k, v in bias.items() if allowed[k]}}
            b.set_logit_bias(s, bias)
        pr = PRESENCE if penalised else 0.0
        got = b.eval_sample_penalized(SLOTS, toks, T, P, -1.0, SEEDS, pr, pr, penalised)
        for i in range(4):
            if where[i] is not None:
                st, miss = guides[attach[i][0]].step(where[i][0], got[i])
                where[i] = [st, where[i][1] + miss]
        out.append(got)
        toks = [int(t) for t in got]
    return np.stack(out, axis=1), b, where


def _same_slots(b, ref, what):
    for s in SLOTS:
        assert np.array_equal(b.state_store(s), ref.state_store(s)), (what, s, "state")
        assert np.array_equal(b.counts(s), ref.counts(s)), (what, s, "counts")


def _guide_words(b, ids, attach, where, what):
    for i, s in enumerate(SLOTS):
        want = (NO_GUIDE, 0, 0) if attach[i] is None else (ids[attach[i][0]], where[i][0], where[i][1])
        assert b.guide_state(s) == want, (what, s, b.guide_state(s), want)


def _same_counters(b, ref, what):
    """one more generator draw on every slot of both (unguided in neither: the guides are detached first)"""
    for s in SLOTS:
        b.detach_guide(s)
        b.set_logit_bias(s, {})
        ref.set_logit_bias(s, {})
    a = b.eval_sample_penalized(SLOTS, [1, 2, 3, 4], 1.0, 1.0, -1.0, SEEDS, 0.0, 0.0, False)
    c = ref.eval_sample_penalized(SLOTS, [1, 2, 3, 4], 1.0, 1.0, -1.0, SEEDS, 0.0, 0.0, False)
    assert np.array_equal(a, c), (what, "draw counters", a.tolist(), c.tolist())


@pytest.mark.parametrize("name,fmt", MODELS)
def test_guided_loops_equal_the_host_driven_loop(tmp_path, name, fmt):
    m = model(_synth(tmp_path, name, fmt, seed=23))
    V = m.n_vocab
    guides, attach = _guides_for(V, seed=31)
    first = [(13 * i + 3) % V for i in range(4)]
    # a user bias on a guided row (merged into the reference's mask) and on the unguided one
    allowed = np.flatnonzero(guides[0].mask(3))
    user_bias = {1: {int(allowed[0]): 2.0, int(allowed[1]): NEG, int(np.flatnonzero(~guides[0].mask(3))[0]): 4.0}, 3: {9: -3.25}}
    # (the 64k-token model once per family: its reference uploads 32k bias entries per guided row and step)
    variants = ((False, None), (True, None), (True, user_bias)) if V < 4096 else ((False, None), (True, user_bias))
    for penalised, bias in variants:
        want, ref, where = _host_loop(m, guides, attach, first, STEPS, penalised, bias)
        calls = {"loop": lambda b: (b.decode_sample_penalized(SLOTS, first, STEPS, T, P, SEEDS, PRESENCE, FREQUENCY)[0] if penalised
                                    else b.decode_sample(SLOTS, first, STEPS, T, P, SEEDS)[0]),
                 "until": lambda b: np.stack(b.decode_until(SLOTS, first, STEPS, None, T, P, SEEDS, PRESENCE if penalised else None,
                                                            FREQUENCY if penalised else None)[0])}
        for what, call in calls.items():
            b, ids = _fresh(m, guides, attach, bias)
            got = call(b)
            tag = (name, "pen" if penalised else "plain", "bias" if bias else "", what)
            assert np.array_equal(got, want), (tag, got.tolist(), want.tolist())
            _guide_words(b, ids, attach, where, tag)
            if not penalised:   # (the reference's zero-penalty passes ran on the model's logits plus the mask: no counts moved in either)
                for s in SLOTS:
                    assert np.array_equal(b.counts(s), _counts_of(V, PRE)), (tag, s)
            _same_slots(b, ref, tag)
            if what == "until":
                _same_counters(b, ref, tag)
            b.free()
        ref.free()
    m.free()


@pytest.mark.parametrize("name,fmt", SMALL)
def test_chain_guide_forces_its_string_whatever_the_seed(tmp_path, name, fmt):
    m = model(_synth(tmp_path, name, fmt, seed=25))
    V = m.n_vocab
    text = [V - 1, 0, 17, 17, V // 2, 3, 1023 % V, 5]
    chain = G.chain_guide(V, text)
    for seeds in ([1, 2, 3, 4], [901, 902, 903, 904]):
        b, ids = _fresh(m, [chain], [(0, 0), (0, 3), (0, 7), (0, 5)])
        got, _ = b.decode_sample(SLOTS, [7, 8, 9, 10], STEPS, 1.0, [0.9, 1.0, 0.5, 0.0], seeds)
        for i, start in enumerate((0, 3, 7, 5)):
            want = [text[(start + k) % len(text)] for k in range(STEPS)]
            assert got[i].tolist() == want, (name, seeds, i, got[i].tolist(), want)
            assert b.guide_state(SLOTS[i]) == (ids[0], (start + STEPS) % len(text), 0), (name, i)
        b.free()
    m.free()


@pytest.mark.parametrize("name,fmt", SMALL)
def test_every_token_is_allowed_in_the_state_it_was_drawn_in(tmp_path, name, fmt):
    m = model(_synth(tmp_path, name, fmt, seed=27))
    V = m.n_vocab
    guides, attach = _guides_for(V, seed=41)
    attach[3] = (1, 2)
    b, ids = _fresh(m, guides, attach)
    temps = [0.0, 1.0, 1.5, 0.7]   # (temperature 0: guided greedy)
    got, _ = b.decode_sample_penalized(SLOTS, [3, 4, 5, 6], STEPS, temps, [0.9, 1.0, 1.0, 0.8], SEEDS, PRESENCE, FREQUENCY)
    for i, s in enumerate(SLOTS):
        g, st = guides[attach[i][0]], attach[i][1]
        for k, t in enumerate(got[i]):
            assert g.mask(st)[t], (name, i, k, int(t), "not allowed in state", st)
            st = g.step(st, t)[0]
        assert b.guide_state(s) == (ids[attach[i][0]], st, 0), (name, i, b.guide_state(s), st)
        assert np.array_equal(b.counts(s), _counts_of(V, PRE) + _counts_of(V, got[i])), (name, i)
    b.free()
    m.free()


@pytest.mark.parametrize("name,fmt", SMALL)
def test_loop_equals_bursts_equals_steps(tmp_path, name, fmt):
    m = model(_synth(tmp_path, name, fmt, seed=29))
    V = m.n_vocab
    guides, _ = _guides_for(V, seed=51)
    g = guides[0]
    rows = [(0, 1), (0, 2)]
    t2, p2, seeds2 = [1.0, 0.8], [0.9, 1.0], [101, 202]
    first = [3, 9]
    # SLOTS[0:2] run the loop, SLOTS[2:4] the same two sequences in pieces
    b, ids = _fresh(m, guides, rows + rows)
    for s in SLOTS:   # (the same start for both groups)
        b.state_load(s, None)
    loop_s, part_s = SLOTS[:2], SLOTS[2:]
    # the penalised family: 16 + 16 = 32, the counts and the draw counters continue
    loop, _ = b.decode_sample_penalized(loop_s, first, STEPS, t2, p2, seeds2, PRESENCE, FREQUENCY)
    b1, _ = b.decode_sample_penalized(part_s, first, 16, t2, p2, seeds2, PRESENCE, FREQUENCY)
    for i, s in enumerate(part_s):
        assert b.guide_state(s) == (ids[0], g.walk(rows[i][1], b1[i])[0], 0), (name, "after the first burst", i)
    b2, _ = b.decode_sample_penalized(part_s, [int(t) for t in b1[:, -1]], 16, t2, p2, seeds2, PRESENCE, FREQUENCY)
    assert np.array_equal(loop, np.concatenate([b1, b2], axis=1)), (name, "pen", loop.tolist(), b1.tolist(), b2.tolist())
    for i in range(2):
        assert b.guide_state(loop_s[i]) == b.guide_state(part_s[i]) == (ids[0], g.walk(rows[i][1], loop[i])[0], 0), (name, "pen", i)
        assert np.array_equal(b.state_store(loop_s[i]), b.state_store(part_s[i])), (name, "pen", i)
        assert np.array_equal(b.counts(loop_s[i]), b.counts(part_s[i])), (name, "pen", i)
    # the plain family: the loop starts the draw counters from 0; 32 single passes after rng_seek(slot, 0) are its stream
    for i, s in enumerate(SLOTS):
        b.state_load(s, None)
        b.rng_seek(s, 0)
        b.attach_guide(s, ids[0], rows[i % 2][1])
    loop, _ = b.decode_sample(loop_s, first, STEPS, t2, p2, seeds2)
    steps, toks = [], list(first)
    for k in range(STEPS):
        out = b.eval_sample(part_s, toks, t2, p2, -1.0, seeds2)
        steps.append(out)
        toks = [int(t) for t in out]
        for i, s in enumerate(part_s):
            assert b.guide_state(s) == (ids[0], g.walk(rows[i][1], loop[i][: k + 1])[0], 0), (name, "plain", k, i)
    assert np.array_equal(loop, np.stack(steps, axis=1)), (name, "plain")
    for i in range(2):
        assert b.guide_state(loop_s[i]) == b.guide_state(part_s[i]), (name, "plain", i)
        assert np.array_equal(b.state_store(loop_s[i]), b.state_store(part_s[i])), (name, "plain", i)
    b.free()
    m.free()


@pytest.mark.parametrize("name,fmt", SMALL)
def test_unguided_rows_of_a_guided_call_are_untouched(tmp_path, name, fmt):
    m = model(_synth(tmp_path, name, fmt, seed=33))
    V = m.n_vocab
    guides, _ = _guides_for(V, seed=61)
    attach = [(0, 1), None, (1, 2), None]
    free_rows = [1, 3]
    b, _ = _fresh(m, guides, attach)
    twin, _ = _fresh(m, [], [None] * 4)
    first = [5, 6, 7, 8]
    calls = [("pen loop", lambda x: x.decode_sample_penalized(SLOTS, first, 12, T, P, SEEDS, PRESENCE, FREQUENCY)[0]),
             ("pass", lambda x: x.eval_sample(SLOTS, first, T, P, -1.0, SEEDS).reshape(4, 1)),
             ("pen pass", lambda x: x.eval_sample_penalized(SLOTS, first, T, P, [0.3, 0.4, 0.5, 0.6], SEEDS, PRESENCE, FREQUENCY, True).reshape(4, 1)),
             ("until", lambda x: np.stack(x.decode_until(SLOTS, first, 9, None, T, P, SEEDS, PRESENCE, FREQUENCY)[0])),
             ("loop", lambda x: x.decode_sample(SLOTS, first, 12, T, P, SEEDS)[0])]
    for what, call in calls:
        got, want = call(b), call(twin)
        for i in free_rows:
            s = SLOTS[i]
            assert np.array_equal(got[i], want[i]), (name, what, i, got[i].tolist(), want[i].tolist())
            assert np.array_equal(b.state_store(s), twin.state_store(s)), (name, what, i)
            assert np.array_equal(b.counts(s), twin.counts(s)), (name, what, i)
            assert b.guide_state(s) == (NO_GUIDE, 0, 0)
    # the draw counters of the unguided slots: one more generator draw in a call that names only them
    fs = [SLOTS[i] for i in free_rows]
    a = b.eval_sample(fs, [1, 2], 1.0, 1.0, -1.0, [7, 8])
    c = twin.eval_sample(fs, [1, 2], 1.0, 1.0, -1.0, [7, 8])
    assert np.array_equal(a, c), (name, a.tolist(), c.tolist())
    b.free()
    twin.free()
    m.free()


@pytest.mark.parametrize("name,fmt", SMALL)
@pytest.mark.parametrize("penalised", [False, True], ids=["sample", "pen"])
def test_until_leaves_each_slot_as_the_plain_guided_loop_of_its_length(tmp_path, name, fmt, penalised):
    m = model(_synth(tmp_path, name, fmt, seed=35))
    V = m.n_vocab
    # a chain that reaches, after its last forced token, the accepting state, which allows token 0 alone; and a guide whose free state sends a
    # quarter of its tokens to such an accepting state
    forced = [9, V - 1, 4, 4, 100, 7, 300, 2, 11, 64]
    chain = G.Guide([{t: i + 1} for i, t in enumerate(forced)] + [{0: len(forced)}], V)
    rng = np.random.default_rng(5)
    free_tokens = [int(t) for t in np.flatnonzero(rng.random(V) < 0.5) if t != 0]
    loose = G.Guide([{t: (1 if rng.random() < 0.25 else 0) for t in free_tokens}, {0: 1}], V)
    guides = [chain, loose]
    attach = [(0, 2), (0, 6), (1, 0), None]
    budgets = [96, 96, 96, 7]
    first = [5, 6, 7, 8]
    pr = PRESENCE if penalised else None
    b, ids = _fresh(m, guides, attach)
    toks, why, _ = b.decode_until(SLOTS, first, budgets, [[0]], T, P, SEEDS, pr, pr)
    lens = [len(t) for t in toks]
    print(name, penalised, "lens", lens, "stopped_by", why.tolist(), "passes", b.last_loop_passes())
    # the chain rows: the rest of the forced string, then token 0, which stops them
    assert toks[0].tolist() == forced[2:] + [0] and toks[1].tolist() == forced[6:] + [0] and why[:2].tolist() == [0, 0]
    assert lens[3] == 7 or toks[3][-1] == 0
    assert lens[2] < 96 and toks[2][-1] == 0 and loose.walk(0, toks[2][:-1])[0] == 1, (lens, "the loose row ends through its accepting state")
    assert b.last_loop_passes() <= max(lens) + 2 * 16 and b.last_loop_passes() <= 96, (b.last_loop_passes(), lens)
    for i, s in enumerate(SLOTS):
        # the plain guided loop of lens[i] steps, this slot alone
        twin, tids = _fresh(m, guides, attach)
        if penalised:
            want, _ = twin.decode_sample_penalized([s], [first[i]], lens[i], T[i], P[i], SEEDS[i], PRESENCE, FREQUENCY)
        else:
            want, _ = twin.decode_sample([s], [first[i]], lens[i], T[i], P[i], SEEDS[i])
        assert np.array_equal(toks[i], want[0]), (name, penalised, i, toks[i].tolist(), want[0].tolist())
        assert np.array_equal(b.state_store(s), twin.state_store(s)), (name, penalised, i, "state")
        assert np.array_equal(b.counts(s), twin.counts(s)), (name, penalised, i, "counts")
        assert b.guide_state(s) == twin.guide_state(s), (name, penalised, i, b.guide_state(s), twin.guide_state(s))
        if attach[i] is not None:
            assert b.guide_state(s) == (ids[attach[i][0]],) + guides[attach[i][0]].walk(attach[i][1], toks[i]), (name, penalised, i)
        # the draw counter: one more generator draw, in the state each is in
        a = b.eval_sample([s], [1], 1.0, 1.0, -1.0, SEEDS[i])
        c = twin.eval_sample([s], [1], 1.0, 1.0, -1.0, SEEDS[i])
        assert np.array_equal(a, c), (name, penalised, i, "draw counter")
        twin.free()
    b.free()
    m.free()


@pytest.mark.parametrize("name,fmt", SMALL)
def test_ragged_prompt_in_chunks_attaches_before_the_final_chunk(tmp_path, name, fmt):
    m = model(_synth(tmp_path, name, fmt, seed=37))
    V = m.n_vocab
    guides, _ = _guides_for(V, seed=71)
    g = guides[1]
    b, ids = _fresh(m, guides, [None] * 4)
    prompt = [(13 * j + 1) % V for j in range(40)]
    for s in (0, 1):
        b.state_load(s, None)
        b.rng_seek(s, 4)
    # slot 0: the guide attached, the whole prompt in one pass, a decode row beside it
    b.attach_guide(0, ids[1], 2)
    whole = b.eval_ragged_sample([0, 2], [prompt, [9]], [1.0, 1.0], [0.9, 1.0], -1.0, [77, 5])
    # slot 1: a non-final chunk without the guide (an argmax: the draw counter stays), the guide attached, the final chunk
    b.eval_ragged_sample([1], [prompt[:24]], 0.0, 0.9, -1.0, 77)
    assert b.guide_state(1) == (NO_GUIDE, 0, 0)
    b.attach_guide(1, ids[1], 2)
    last = b.eval_ragged_sample([3, 1], [[9], prompt[24:]], [1.0, 1.0], [1.0, 0.9], -1.0, [5, 77])
    assert int(last[1]) == int(whole[0]), (name, last.tolist(), whole.tolist())
    assert g.mask(2)[whole[0]]
    assert b.guide_state(0) == b.guide_state(1) == (ids[1], g.step(2, whole[0])[0], 0), (name, b.guide_state(0), b.guide_state(1))
    assert np.array_equal(b.state_store(0), b.state_store(1))
    # the penalised ragged pass honours the guide as well: the host-driven reference of one step
    b.state_load(0, None)
    b.attach_guide(0, ids[1], 1)
    tok, lg = b.eval_ragged_sample_penalized([0], [prompt], 1.0, 0.9, -1.0, 77, 0.5, 0.25, True, want_logits=True)
    counts = b.counts(0)
    counts[tok[0]] -= 1
    want, _ = _sample_rows(_masked(_adjust(lg[0], counts, 0.5, 0.25, None), g.mask(1))[None, :], pkg.sample_params(1, 1.0, 0.9, -1.0, 77), [5], 1)
    assert int(tok[0]) == int(want[0]) and b.guide_state(0) == (ids[1], g.step(1, tok[0])[0], 0), (name, tok.tolist(), want.tolist())
    b.free()
    m.free()


def test_rejected_guide_calls_change_nothing(tmp_path):
    m = model(_synth(tmp_path, "test-v6", "Q5_1", seed=39))
    V = m.n_vocab
    guides, attach = _guides_for(V, seed=81)
    b, ids = _fresh(m, guides, attach)
    twin, _ = _fresh(m, guides, attach)
    first = b.decode_sample_penalized(SLOTS, [1, 2, 3, 4], 3, T, P, SEEDS, PRESENCE, FREQUENCY)[0][:, -1]
    twin.decode_sample_penalized(SLOTS, [1, 2, 3, 4], 3, T, P, SEEDS, PRESENCE, FREQUENCY)
    snapshot = {s: (b.state_store(s), b.counts(s), b.guide_state(s)) for s in SLOTS}
    L, ptr, lib = b._L, b._ptr, m._library

    def rejected(call):
        b.last_error = 0
        with pytest.raises(ValueError):
            call()
        assert b.last_error == ARGS, b.last_error   # (RWKV_ERROR_ARGS and nothing else)

    def create(n_states, begin, toks, nxt, out=True):
        a = [np.asarray(x, dtype=np.uint32) for x in (begin, toks, nxt)]
        gid = ctypes.c_uint32(12345)
        ok = L.rwkv_mi_batch_guide_create(ptr, n_states, *[x.ctypes.data_as(P_U32) for x in a], ctypes.byref(gid) if out else None)
        err = lib.rwkv_get_last_error(m._ctx)
        assert not ok and err == ARGS and gid.value == 12345, (n_states, begin, toks, nxt, ok, err, gid.value)

    # every rule of guide_create
    create(0, [0], [1], [0])                                  # no state
    create(65536, [0, 1], [1], [0])                           # too many states
    create(2, [0, 1, 1], [1], [0])                            # a state without an edge
    create(2, [1, 2, 3], [1, 2, 3], [0, 0, 0])                # edge_begin does not start at 0
    create(2, [0, 2, 1], [1, 2], [0, 0])                      # edge_begin decreases
    create(1, [0, 2], [1, V], [0, 0])                         # a token out of range
    create(1, [0, 2], [2, 2], [0, 0])                         # tokens not strictly ascending
    create(1, [0, 2], [3, 2], [0, 0])
    create(2, [0, 1, 2], [1, 2], [0, 2])                      # a next state out of range
    create(1, [0, 1], [1], [0], out=False)                    # guide_out is NULL
    assert not L.rwkv_mi_batch_guide_create(ptr, 1, None, None, None, ctypes.byref(ctypes.c_uint32(0))) and lib.rwkv_get_last_error(m._ctx) == ARGS
    # free and attach
    rejected(lambda: b.free_guide(7))                         # no such guide
    rejected(lambda: b.free_guide(16))
    rejected(lambda: b.free_guide(NO_GUIDE))
    rejected(lambda: b.free_guide(ids[0]))                    # still attached
    rejected(lambda: b.attach_guide(4, ids[0], 0))            # a slot out of range
    rejected(lambda: b.attach_guide(0, 9, 0))                 # no such guide
    rejected(lambda: b.attach_guide(0, ids[1], 3))            # a state out of range (3 states)
    rejected(lambda: b.guide_state(4))
    # the greedy family and beam search on a guided slot
    rejected(lambda: b.decode_greedy(SLOTS, [1, 2, 3, 4], 4))
    rejected(lambda: b.decode_greedy([SLOTS[0]], [1], 4))
    rejected(lambda: b.decode_until(SLOTS, [1, 2, 3, 4], 4))
    rejected(lambda: b.decode_beam([SLOTS[3], SLOTS[0]], [1], 2, 4))
    # a 17th guide: fourteen more fit, then none -- and the batch is as it was
    extra = [b.create_guide([{1: 0}]) for _ in range(14)]
    assert sorted(ids + extra) == list(range(16))
    rejected(lambda: b.create_guide([{1: 0}]))
    for gid in extra:
        b.free_guide(gid)
    assert b.create_guide([{2: 0}]) == min(extra)             # a freed id is given out again
    b.free_guide(min(extra))
    # nothing moved: states, counts and guide words now; parities, draw counters and guides through what the next valid calls return
    for s in SLOTS:
        assert np.array_equal(b.state_store(s), snapshot[s][0]) and np.array_equal(b.counts(s), snapshot[s][1]) and b.guide_state(s) == snapshot[s][2], s
    nxt = [int(t) for t in first]
    la = b.decode_sample_penalized(SLOTS, nxt, 6, T, P, SEEDS, PRESENCE, FREQUENCY)[0]
    lb = twin.decode_sample_penalized(SLOTS, nxt, 6, T, P, SEEDS, PRESENCE, FREQUENCY)[0]
    assert np.array_equal(la, lb), (la.tolist(), lb.tolist())
    _same_slots(b, twin, "after the rejected calls")
    for s in SLOTS:
        assert b.guide_state(s) == twin.guide_state(s), s
    # the unguided slot still runs the greedy family; a detached slot as well; a guide nobody has attached can be freed
    b.decode_greedy([SLOTS[3]], [1], 2)
    b.detach_guide(SLOTS[2])
    assert b.guide_state(SLOTS[2]) == (NO_GUIDE, 0, 0)
    b.decode_greedy([SLOTS[2], SLOTS[3]], [1, 2], 2)
    b.free_guide(ids[1])
    b.free()
    twin.free()
    m.free()


# ---- beside the persistent kernel ----

def test_guided_loop_next_to_persistent_kernel(tmp_path, monkeypatch):
    monkeypatch.setenv("RWKV_MI_NO_AUTOTUNE", "1")
    m = model(_synth(tmp_path, "mega-v6-4096", "Q4_0", seed=21))
    assert m.decode_path() == 2, m.persist_info()
    V = m.n_vocab
    b = pkg.RWKVBatch(m, 8)
    slots = list(range(8))
    temps = [0.0, 0.3, 0.7, 1.0, 1.5, 0.0, 1.0, 0.7]
    seeds = [s + 1 for s in slots]
    guide = G.random_guide(V, 5, seed=91)
    gid = b.create_guide(guide.edges)

    def fresh():
        m.state_load(None)
        for s in slots:
            b.state_load(s, None)
            b.counts_reset(s)
            b.counts_add(s, [5, 5, 6])
            b.rng_seek(s, 0)
            if s % 4 == 3:
                b.detach_guide(s)
            else:
                b.attach_guide(s, gid, s % 5)

    def batch_round(first):
        return b.decode_sample_penalized(slots, first, 4, temps, 0.9, seeds, 0.2, 0.2)[0]

    # solo: the context's greedy rounds, then the batch's guided rounds
    fresh()
    solo_ctx, tok = [], 3
    for _ in range(3):
        toks, _ = m.decode_greedy(tok, 4)
        solo_ctx.append(toks)
        tok = int(toks[-1])
    solo_ctx_state = m.state_store()
    solo_b, first = [], [(11 * s + 5) % V for s in slots]
    for _ in range(3):
        out = batch_round(first)
        solo_b.append(out)
        first = [int(t) for t in out[:, -1]]
    solo_states = [b.state_store(s) for s in slots]
    solo_guides = [b.guide_state(s) for s in slots]
    for s in slots:
        if s % 4 != 3:
            assert solo_guides[s] == (gid,) + guide.walk(s % 5, np.concatenate([r[s] for r in solo_b])), s
    # interleaved in one process
    fresh()
    tok, first = 3, [(11 * s + 5) % V for s in slots]
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
        assert np.array_equal(b.state_store(s), solo_states[s]), s
        assert b.guide_state(s) == solo_guides[s], s
    assert m.decode_path() == 2 and m.healthy()
    b.free()
    m.free()
