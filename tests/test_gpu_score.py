"""Per-position scoring on the device (rwkv_mi_score_resident, csrc/score.hip k_score_rows): log-prob of a target and argmax after EVERY token
of one pass.

What is exact is held exactly (np.array_equal): the logits of every position against the CPU oracle's per-token rwkv_eval, the argmax
against the first maximum of those, the state, and every split / chunking / run-to-run comparison, log-probs included.
The log-prob itself has ONE tolerance, derived and not measured: the reference is NumPy float64 on the oracle's f32 logits,
    ref = l[target] - (m + log(sum(exp(l - m)))),   m = max(l);
the device's float64 sum of V <= 2^17 positive terms (each exp good to a few f64 ulp) is off by less than about V * 2^-52 <= 2^-35 relative,
log carries that over as an absolute error, and the single rounding to f32 adds half an f32 ulp of the result:
    |dev - float32(ref)| <= ulp32(ref) + 2^-32
(the 2^-32 term, 8 x the derived bound, matters where the log-prob is near 0 and an f32 ulp is smaller than the f64 error)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import reference_constants as R
from gpu_lib import ROOT, library, model, pkg, synth

pytestmark = pytest.mark.gpu

ARGS = 1 << 8   # RWKV_ERROR_ARGS
NO_TARGET = 0xFFFFFFFF
P_UINT32 = ctypes.POINTER(ctypes.c_uint32)
P_FLOAT = ctypes.POINTER(ctypes.c_float)
GOLDEN = [(v, f) for v in R.VERSIONS for f in ("FP32", "FP16", "Q5_0", "Q5_1") if v in R.HAVE_FP32_FP16 or f.startswith("Q")]
LENGTHS = (1, 2, 31, 32, 33, 200, 1064)

_sample_hooks = None


def _hooks():
    global _sample_hooks
    if _sample_hooks is None:
        library()
        _sample_hooks = pkg.RWKVSharedLibrary(pkg.SAMPLE_HOOKS_LIB_PATH)
    return _sample_hooks.library


def score_rows(logits, targets, want_logprobs=True, want_argmax=True):
    """k_score_rows through the test hook on logits [rows][V]."""
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    rows, V = logits.shape
    tg = None if targets is None else np.ascontiguousarray(np.asarray(targets, dtype=np.int64).astype(np.uint32))
    lp = np.full(rows, np.nan, dtype=np.float32) if want_logprobs else None
    am = np.full(rows, 0xFFFFFFFF, dtype=np.uint32) if want_argmax else None
    ok = _hooks().rwkv_test_score_rows(logits.ctypes.data_as(P_FLOAT), rows, V, None if tg is None else tg.ctypes.data_as(P_UINT32),
                                       None if lp is None else lp.ctypes.data_as(P_FLOAT), None if am is None else am.ctypes.data_as(P_UINT32))
    assert ok, "rwkv_test_score_rows failed"
    return lp, am


def ref_logprob(l, target):
    """float64 on the f32 logits"""
    l = np.asarray(l, dtype=np.float32).astype(np.float64)
    m = l.max()
    return float(l[int(target)] - (m + np.log(np.exp(l - m).sum())))


def check_logprob(dev, ref, what):
    """the one tolerance of this file (module docstring); every figure is printed before it is asserted"""
    r32 = np.float32(ref)
    tol = float(np.spacing(np.abs(r32))) + 2.0 ** -32
    err = abs(float(dev) - float(r32))
    if err > tol or not float(dev) <= 0.0:
        print("logprob", what, "dev", float(dev), "ref", ref, "err", err, "tol", tol)
    assert err <= tol, (what, float(dev), ref, err, tol)
    assert float(dev) <= 0.0, (what, float(dev))


def check_rows(logits, targets, lp, am, what):
    for r in range(logits.shape[0]):
        if am is not None:
            assert int(am[r]) == int(np.argmax(logits[r])), (what, r, int(am[r]), int(np.argmax(logits[r])))
        if lp is None:
            continue
        if int(targets[r]) == NO_TARGET:
            assert float(lp[r]) == 0.0, (what, r, float(lp[r]))
        else:
            check_logprob(lp[r], ref_logprob(logits[r], targets[r]), (what, r))


# ---- the kernel on crafted logits ----

def _crafted(V, seed):
    rng = np.random.default_rng(seed)
    rows, targets = [], []

    def add(l, t):
        rows.append(np.asarray(l, dtype=np.float32)); targets.append(int(t))
    for k in range(6):   # random rows: model-like spread, wide, narrow
        add(rng.standard_normal(V) * (1.0, 4.0, 0.05)[k % 3] + (0.0, -7.0)[k % 2], rng.integers(V))
    add(np.full(V, 1.25), V // 3)                                   # V equal logits: -log V, argmax 0
    dom = rng.standard_normal(V); d = int(rng.integers(1, V)); dom[d] = dom.max() + 30.0
    add(dom, d)                                                     # one dominant logit, the target on it ...
    add(dom, (d + 7) % V)                                           # ... and elsewhere
    big = np.where(rng.random(V) < 0.5, 1e4, -1e4) + rng.standard_normal(V)
    add(big, int(np.argmax(big)))                                   # magnitudes of +-1e4: the max subtraction keeps exp in range
    add(big, int(np.argmin(big)))
    add(-big, rng.integers(V))
    ties = rng.standard_normal(V).astype(np.float32)
    idx = sorted({int(i) for i in (V - 1, V // 2, 1025 % V, 64 % V, 63 % V, 5)})
    ties[idx] = ties.max() + 1.0                                    # exact ties at several indices: the lowest wins
    add(ties, idx[-1])
    ties2 = ties.copy(); ties2[idx[0]] = ties2.min()                # ... and with the first of them gone
    add(ties2, idx[1])
    add(rng.standard_normal(V), NO_TARGET)                          # rows without a target return 0
    add(np.full(V, -3.0), NO_TARGET)
    return np.stack(rows), np.asarray(targets, dtype=np.int64)


@pytest.mark.parametrize("V", [1000, 50277, 65536])
def test_crafted_logits_through_the_hook(V):
    logits, targets = _crafted(V, 1234 + V)
    lp, am = score_rows(logits, targets)
    check_rows(logits, targets, lp, am, ("crafted", V))
    eq = 6   # the row of equal logits
    assert int(am[eq]) == 0   # (its log-prob, -log V, has been held to the tolerance with the other rows)
    # the same buffer twice: identical bytes; each output alone: the same values; one row alone: the same values (nothing depends on the launch)
    lp2, am2 = score_rows(logits, targets)
    assert lp.tobytes() == lp2.tobytes() and am.tobytes() == am2.tobytes()
    lp3, none = score_rows(logits, targets, want_argmax=False)
    assert none is None and lp3.tobytes() == lp.tobytes()
    none, am3 = score_rows(logits, None, want_logprobs=False)
    assert none is None and np.array_equal(am3, am)
    for r in (0, 7, len(targets) - 1):
        l1, a1 = score_rows(logits[r:r + 1], targets[r:r + 1])
        assert l1.tobytes() == lp[r:r + 1].tobytes() and a1[0] == am[r]
    # log-probs asked for without targets: every row is a row without a target
    lp4, _ = score_rows(logits, None)
    assert np.array_equal(lp4, np.zeros(len(targets), dtype=np.float32))


def test_argmax_rule_is_k_argmax(tmp_path):
    """the same rows through the greedy loop's k_argmax (the first token of decode_greedy is the argmax of the step's logits) and through
    sample(temperature = 0) -- on a model's real logits, where the hook's argmax must name the same token"""
    p = str(tmp_path / "m.bin")
    library()
    synth.write_model(p, synth.CONFIGS["test-v6"], "Q4_0", seed=5)
    m = model(p)
    for tok in (3, 77, 500):
        m.state_load(None)
        lg = m.eval_resident([tok])
        _, am = score_rows(lg[None, :], None, want_logprobs=False)
        assert m.sample(temperature=0.0) == int(am[0])
        m.state_load(None)
        toks, _ = m.decode_greedy(tok, 1)
        assert int(toks[0]) == int(am[0]) == int(np.argmax(lg))
    m.free()


# ---- every golden architecture and format against the oracle at every position ----

def _tokens(n, V, seed):
    return np.random.default_rng(seed).integers(0, V, size=n).astype(np.uint32)


def _oracle_positions(om, tokens, keep_states=()):
    """The oracle stepping token by token from a fresh state: logits [n][V] and the states after the prefixes named in keep_states."""
    st = om.init_state()
    logits = np.empty((len(tokens), om.n_vocab), dtype=np.float32)
    states = {}
    for i, t in enumerate(tokens):
        logits[i], st = om.eval(int(t), st)
        if i + 1 in keep_states:
            states[i + 1] = st
    return logits, states


def _check_call(m, tokens, targets, ol, ostate, what):
    lp, am, lg = m.score_resident(tokens, targets, want_argmax=True, want_logits=True)
    assert np.array_equal(lg, ol), (what, "logits", float(np.abs(lg - ol).max()))
    check_rows(ol, targets, lp, am, what)
    assert np.array_equal(m.state_store(), ostate), (what, "state")
    assert np.array_equal(m.logits_store(), ol[-1]), (what, "logits_store")
    assert m.sample(temperature=0.0) == int(am[-1]), (what, "sample")
    return lp, am, lg


@pytest.mark.parametrize("version,fmt", GOLDEN)
def test_golden_every_position(golden_dir, version, fmt):
    path = R.fixture_path(golden_dir, version, fmt)
    m = model(path)
    om = O.OracleModel(path)
    V = m.n_vocab
    tokens = _tokens(max(LENGTHS), V, 20240 + len(version) + len(fmt))
    targets_all = np.concatenate([tokens[1:], _tokens(1, V, 9)]).astype(np.int64)
    targets_all[5::17] = NO_TARGET
    ol, ostates = _oracle_positions(om, tokens, set(LENGTHS) | {T - 1 for T in LENGTHS})
    for T in LENGTHS:
        m.state_load(None)
        lp, am, _ = _check_call(m, tokens[:T], targets_all[:T], ol[:T], ostates[T], (version, fmt, T))
        # k_argmax through the greedy loop: from the state before the last token, its first token is the argmax of that step
        m.state_load(ostates[T - 1] if T > 1 else None)
        toks, _ = m.decode_greedy(int(tokens[T - 1]), 1)
        assert int(toks[0]) == int(am[-1]), (version, fmt, T, "k_argmax")
        # each output alone: the same bytes
        m.state_load(None)
        lp2, none, none2 = m.score_resident(tokens[:T], targets_all[:T], want_argmax=False)
        assert none is None and none2 is None and lp2.tobytes() == lp.tobytes(), (version, fmt, T)
        m.state_load(None)
        none, am2, none2 = m.score_resident(tokens[:T])
        assert none is None and np.array_equal(am2, am), (version, fmt, T)
    m.free()
    om.free()


# ---- chunking is invisible ----

def _child(path, tokens, tmp_path, env_extra):
    tp, out = str(tmp_path / "tokens.npy"), str(tmp_path / "out.npz")
    np.save(tp, tokens)
    env = dict(os.environ)
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "score_worker.py"), path, tp, out], cwd=os.path.join(ROOT, "tests"), env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return np.load(out)


@pytest.mark.parametrize("name,fmt", [("test-v6", "Q4_0"), ("test-v7", "Q5_1"), ("test-v4", "FP16")])
def test_head_chunks_of_32_rows_give_the_same_bytes(tmp_path, name, fmt):
    """RWKV_MI_SCORE_ROWS=32 in a fresh child process (seven chunks, the last of 8 rows on the vector kernels) against the default (one
    chunk on the matrix cores), and against the oracle"""
    p = str(tmp_path / "m.bin")
    library()
    synth.write_model(p, synth.CONFIGS[name], fmt, seed=13)
    om = O.OracleModel(p)
    tokens = _tokens(200, om.n_vocab, 77)
    targets = np.concatenate([tokens[1:], [NO_TARGET]]).astype(np.int64)
    small = _child(p, tokens, tmp_path, {"RWKV_MI_SCORE_ROWS": "32"})
    m = model(p)
    lp, am, lg = m.score_resident(tokens, targets, want_argmax=True, want_logits=True)
    for key, mine in (("logprobs", lp), ("argmax", am), ("logits", lg), ("state", m.state_store()), ("last", m.logits_store())):
        assert small[key].tobytes() == mine.tobytes(), (name, fmt, key)
    ol, ostates = _oracle_positions(om, tokens, (200,))
    assert np.array_equal(lg, ol) and np.array_equal(m.state_store(), ostates[200])
    check_rows(ol, targets, lp, am, (name, fmt))
    m.free()
    om.free()


@pytest.mark.parametrize("version,fmt", [("6v0-3m", "Q5_1"), ("7v0-834K", "FP16"), ("4v0-660K", "Q5_0"), ("5v2-730K", "FP32")])
def test_a_call_cut_in_three_equals_the_whole(golden_dir, version, fmt):
    path = R.fixture_path(golden_dir, version, fmt)
    m = model(path)
    V = m.n_vocab
    tokens = _tokens(75, V, 31)
    targets = _tokens(75, V, 32).astype(np.int64)
    whole = m.score_resident(tokens, targets, want_argmax=True, want_logits=True)
    state = m.state_store()
    m.state_load(None)
    parts = [m.score_resident(tokens[a:b], targets[a:b], want_argmax=True, want_logits=True) for a, b in ((0, 32), (32, 33), (33, 75))]
    for k, what in enumerate(("logprobs", "argmax", "logits")):
        assert np.concatenate([p[k] for p in parts]).tobytes() == whole[k].tobytes(), (version, fmt, what)
    assert np.array_equal(m.state_store(), state)
    m.free()


# ---- rejections ----

def test_rejections_change_nothing(golden_dir, tmp_path):
    path = R.fixture_path(golden_dir, "6v0-3m", "Q5_1")
    m = model(path)
    lib = m._library
    L = lib.library
    V = m.n_vocab
    m.eval_resident([1, 2, 3])
    before, lbefore = m.state_store(), m.logits_store()
    good = (ctypes.c_uint32 * 4)(1, 2, 3, 4)
    bad = (ctypes.c_uint32 * 4)(1, 2, V, 4)
    badt = (ctypes.c_uint32 * 4)(1, 2, V, 4)
    okt = (ctypes.c_uint32 * 4)(1, NO_TARGET, V - 1, 0)
    lp = (ctypes.c_float * 4)()
    am = (ctypes.c_uint32 * 4)()
    lib.rwkv_set_print_errors(m._ctx, False)
    cases = {
        "NULL tokens": (None, 4, okt, lp, am),
        "n = 0": (good, 0, okt, lp, am),
        "token >= V": (bad, 4, okt, lp, am),
        "target >= V": (good, 4, badt, lp, am),
        "target >= V, argmax only": (good, 4, badt, None, am),
        "log-probs without targets": (good, 4, None, lp, am),
    }
    for what, (tk, n, tg, lpo, amo) in cases.items():
        assert not L.rwkv_mi_score_resident(m._ctx.ptr, tk, n, tg, lpo, amo, None), what
        assert lib.rwkv_get_last_error(m._ctx) & ARGS, what
        assert np.array_equal(m.state_store(), before) and np.array_equal(m.logits_store(), lbefore), what
    lib.rwkv_set_print_errors(m._ctx, True)
    # ... and the accepted form of the same call still works afterwards
    assert L.rwkv_mi_score_resident(m._ctx.ptr, good, 4, okt, lp, am, None)
    assert lp[1] == 0.0 and not np.array_equal(m.state_store(), before)
    # every output NULL: rwkv_mi_eval_resident(.., NULL)
    m.state_load(before)
    assert L.rwkv_mi_score_resident(m._ctx.ptr, good, 4, None, None, None, None)
    after = m.state_store()
    m.state_load(before)
    m.eval_resident([1, 2, 3, 4], want_logits=False)
    assert np.array_equal(m.state_store(), after)
    m.free()
    # a chain context
    p = str(tmp_path / "m.bin")
    synth.write_model(p, synth.CONFIGS["test-v6"], "Q5_1", seed=3)
    os.environ["RWKV_MI_DEVICES"] = "0,0"
    try:
        c = model(p)
    finally:
        del os.environ["RWKV_MI_DEVICES"]
    c.eval_sequence([1, 2, 3], None)
    c.state_load(None)
    sbefore = c.state_store()
    lib.rwkv_set_print_errors(c._ctx, False)
    assert not L.rwkv_mi_score_resident(c._ctx.ptr, good, 4, okt, lp, am, None)
    assert lib.rwkv_get_last_error(c._ctx) & ARGS
    lib.rwkv_set_print_errors(c._ctx, True)
    assert np.array_equal(c.state_store(), sbefore)
    c.free()


# ---- perplexity ----

@pytest.mark.parametrize("version,fmt", [("6v0-3m", "Q5_0"), ("4v0-660K", "FP16")])
def test_perplexity_is_the_reference_loop(golden_dir, version, fmt):
    """measure_pexplexity.py:71-85: feed tokens[:-1]; position i is scored against tokens[i + 1] and counts when ignore_first_n_tokens == 0
    or i + 1 >= ignore_first_n_tokens; float64 mean. The bound on the mean is the mean of the per-term tolerances ulp32(ref_i) + 2^-32 (an
    error of a mean is at most the mean of the errors); nothing is added for the difference between ref_i and float32(ref_i)."""
    path = R.fixture_path(golden_dir, version, fmt)
    m = model(path)
    om = O.OracleModel(path)
    tokens = _tokens(200, m.n_vocab, 4242)
    ol, _ = _oracle_positions(om, tokens[:-1])
    ref = np.array([ref_logprob(ol[i], tokens[i + 1]) for i in range(199)])
    for ignore in (0, 1, 10):
        counted = np.array([ignore == 0 or i + 1 >= ignore for i in range(199)])
        want = float(-ref[counted].sum() / counted.sum())
        tol = float(np.mean([float(np.spacing(np.abs(np.float32(r)))) + 2.0 ** -32 for r in ref[counted]]))
        m.state_load(None)
        loss, ppl = m.perplexity(tokens, ignore_first_n_tokens=ignore)
        print("perplexity", version, fmt, ignore, "loss", loss, "ref", want, "err", abs(loss - want), "tol", tol)
        assert abs(loss - want) <= tol, (version, fmt, ignore, loss, want, tol)
        assert ppl == float(np.exp(loss))
    m.free()
    om.free()


# ---- real geometry ----

def test_world_vocabulary_multi_chunk_head(tmp_path):
    """D = 2048, V = 65536, one layer (tests/test_gpu_real_geometry.py's World-vocabulary slice), Q4_0 with its F16 head, T = 300: two
    chunks of the default R = 256 rows, the second one short (44 rows), the F16 head on the matrix-core sequence kernel -- every position
    against the oracle."""
    os.environ["RWKV_MI_NO_AUTOTUNE"] = "1"
    try:
        library()
        p = str(tmp_path / "m.bin")
        spec = synth.CONFIGS["mega-v6-2048-v64k"]
        synth.write_model(p, spec, "Q4_0", seed=71)
        om = O.OracleModel(p)
        m = model(p)
        tokens = _tokens(300, spec.n_vocab, 99)
        targets = np.concatenate([tokens[1:], [NO_TARGET]]).astype(np.int64)
        ol, ostates = _oracle_positions(om, tokens, (300,))
        _check_call(m, tokens, targets, ol, ostates[300], "world vocabulary")
        m.free(); om.free()
    finally:
        del os.environ["RWKV_MI_NO_AUTOTUNE"]
