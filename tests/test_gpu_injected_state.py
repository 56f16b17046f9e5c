"""Every decode path from states it did not produce itself, on plain and on stressed decay vectors (tests/stress_lib.py), against the CPU
oracle run from the same state: np.array_equal on logits and on the whole state at every step a call exposes. The oracle's own worth on
these inputs is held in tests/test_cpu_stress_reference.py.

Files: the D = 256 file of every architecture as Q5_1 and FP16, a plain and a stressed copy of each, with every family of
stress_lib.state_families; and the geometries the persistent kernels are built for, stressed copy only, families normal / large / long-run
(+ half-fresh on RWKV-4): mega-v6-2048 Q4_0 under RWKV_MI_PERSIST=ring and =regs, slice-v7-2560 Q5_1, slice-v4-768 Q5_1.

Paths, each asserted with decode_path() / persist_kind() where a test claims it:
  per-op      RWKV_MI_NO_FUSED=1, decode_path() == 0                     every case
  fused       RWKV_MI_NO_MEGA=1, decode_path() == 1                      quantised RWKV-4 / 6 / 7
  persistent  decode_path() == 2, persist_kind() == 3 (k47)              quantised RWKV-4 / 7 (D = 256 included)
              persist_kind() == 2 (ring) / 1 (regs)                      mega-v6-2048
Per case: the plain ABI (4 tokens of eval(token, state_in)) and the resident loops (state_load, decode_greedy, state_store,
decode_sample at temperature 0) on every path of the case; the sequence kernels (40 tokens at once and in chunks of 33: both sides of the
32-token threshold of the sequence recurrences, then one eval from the returned state); rows and segments (RWKVBatch: 3 eval passes, one
ragged pass of lengths 1, 3, 33, 40, 2, one score_ragged on the same lists).

The log-probs of score_ragged have the one tolerance of tests/test_gpu_score.py (derived there; tests/test_gpu_batch_score.py holds the
ragged form to that scorer bit for bit): |dev - float32(ref)| <= ulp32(ref) + 2^-32, ref = logprobs_ref.f64_logprobs on the oracle's logits.

What the file sees that the fresh-state suite does not (one-line mutations of one copy of a recurrence each, on a side build; the suite
without this file passed on both):
  wkv4_body (kernels.hip), e1 taken as 0 when pp - qq < -10     18 tests here fail, every RWKV-4 case: plain ABI (5), resident loops (4),
                                                                sequence (4), rows and segments (5)
  k6_ring (ring_v6.hip), the decay clamped to >= 1e-6           3 fail: plain ABI, resident loops and the eval after a sequence, ring case
Thresholds much further out are not mutations in f32 and no finite state of these families shows them: e1 < exp(-20) changes a = e1 aa + e2 v
by under an ulp, and that ulp goes into the output only, where the next projection rounds its operand to fp16 or 8 bits (an FP32 file and the
`large` family would show it down to exp(-20)); a decay floor of 1e-20 under a state of 1e3 is 1e-17 beside k v.
"""
import os
import shutil

import numpy as np
import pytest

import oracle_lib as O
import stress_lib as S
from gpu_lib import library, model, pkg, synth
from logprobs_ref import f64_logprobs

pytestmark = pytest.mark.gpu

SEED = 7
ARCH_OF = {"test-v4": "4", "test-v5.1": "5.1", "test-v5.2": "5.2", "test-v6": "6", "test-v7": "7",
           "mega-v6-2048": "6", "slice-v7-2560": "7", "slice-v4-768": "4"}
ENV = ("RWKV_MI_NO_AUTOTUNE", "RWKV_MI_NO_FUSED", "RWKV_MI_NO_MEGA", "RWKV_MI_PERSIST", "RWKV_MI_SEQ_Q", "RWKV_MI_SEQ_F16")
N_SEQ, CHUNK, N_ABI, N_GREEDY, FIRST, FOLLOW = 40, 33, 4, 6, 5, 7
SEG_LENS = (1, 3, 33, 40, 2)
N_PASSES = 3


def _case(name, fmt, weights, persist=None):
    """(file key, [(path label, environment, decode_path(), persist_kind())]), the path a model of the file takes by default last"""
    quant, arch = fmt not in ("FP16", "FP32"), ARCH_OF[name]
    paths = [("per-op", {"RWKV_MI_NO_FUSED": "1"}, 0, 0)]
    if quant and arch in ("4", "6", "7"):
        paths.append(("fused", {"RWKV_MI_NO_MEGA": "1"}, 1, 0))
    if persist is not None:
        paths.append(("persistent", {"RWKV_MI_PERSIST": persist} if persist in ("ring", "regs") else {}, 2, {"ring": 2, "regs": 1, "k47": 3}[persist]))
    return (name, fmt, weights), paths[-1:] if persist == "regs" else paths   # (the ring case has run the file's other two paths)


SMALL = [(n, f, w, "k47" if f == "Q5_1" and ARCH_OF[n] in ("4", "7") else None)
         for n in ("test-v4", "test-v5.1", "test-v5.2", "test-v6", "test-v7") for f in ("Q5_1", "FP16") for w in ("plain", "stress")]
BIG = [("mega-v6-2048", "Q4_0", "stress", "ring"), ("mega-v6-2048", "Q4_0", "stress", "regs"),
       ("slice-v7-2560", "Q5_1", "stress", "k47"), ("slice-v4-768", "Q5_1", "stress", "k47")]
BIG_FAMILIES = ("normal", "large", "long-run", "half-fresh")
CASES = [_case(*c) for c in SMALL + BIG]
IDS = ["-".join(c[:3]) + (f"-{c[3]}" if c[3] else "") for c in SMALL + BIG]


@pytest.fixture(autouse=True)
def _env():
    keep = {k: os.environ.get(k) for k in ENV}
    os.environ.update({"RWKV_MI_NO_AUTOTUNE": "1", "RWKV_MI_SEQ_Q": "exact", "RWKV_MI_SEQ_F16": "valu"})   # (the exact sequence arms: tests/conftest.py)
    for k in ("RWKV_MI_NO_FUSED", "RWKV_MI_NO_MEGA", "RWKV_MI_PERSIST"):
        os.environ.pop(k, None)
    yield
    for k, v in keep.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def _open(path, paths, which):
    """A model of the file on the named path ("top": the last of the case's paths), the path asserted."""
    label, env, want_path, want_kind = paths[-1] if which == "top" else next(p for p in paths if p[0] == which)
    os.environ.update(env)
    try:
        m = model(path)
    finally:
        for k in env:
            del os.environ[k]
    assert m.decode_path() == want_path and (want_path != 2 or m.persist_kind() == want_kind), (label, m.decode_path(), m.persist_kind(), m.persist_info())
    return m


def _row_tokens(call, slot, n, V):
    return [(37 * call + 11 * slot + 29 * j + 5) % V for j in range(n)]


def _row_targets(slot, n, V):
    return [(53 + 7 * slot + 31 * j + 2) % V for j in range(n)]


class _Reference:
    """What the oracle computes from every injected state of one file, computed once and read by every test of the file."""

    def __init__(self, path, families):
        om = O.OracleModel(path)
        self.V = V = om.n_vocab
        fam = S.state_families(om, SEED)
        self.states = {k: s for k, s in fam.items() if families is None or k in families}
        self.tokens = S.lcg_tokens(V, N_SEQ, start=S.PROMPT_LEN)
        self.serial, self.seq, self.follow, self.greedy = {}, {}, {}, {}
        for k, s0 in self.states.items():
            st, steps = s0, []
            for t in self.tokens[:N_ABI]:
                lg, st = om.eval(t, st)
                steps.append((lg, st))
            # (the oracle's sequence call is its serial loop with the projections of all tokens taken together: tests/test_cpu_f64_reference.py)
            self.serial[k], self.seq[k] = steps, om.eval_sequence(self.tokens[N_ABI:], st)
            self.follow[k] = om.eval(FOLLOW, self.seq[k][1])
            st, tok, out = s0, FIRST, []
            for _ in range(N_GREEDY):
                lg, st = om.eval(tok, st)
                tok = int(np.argmax(lg))
                out.append(tok)
            self.greedy[k] = (out, st)
        # rows and segments: slot i starts from the i-th family (cycling) and runs alone
        names = list(self.states)
        self.slot_family = [names[i % len(names)] for i in range(len(SEG_LENS))]
        self.rows = []
        for slot, n in enumerate(SEG_LENS):
            st, r = self.states[self.slot_family[slot]], {"passes": []}
            for p in range(N_PASSES):
                lg, st = om.eval(_row_tokens(p, slot, 1, V)[0], st)
                r["passes"].append(lg)
            r["state_passes"] = st
            r["segment"] = _row_tokens(N_PASSES, slot, n, V)
            r["ragged"] = lg, st = om.eval_sequence(r["segment"], st)
            r["targets"] = _row_targets(slot, n, V)
            am, lp = [], []
            for t, g in zip(r["segment"], r["targets"]):
                lg, st = om.eval(t, st)
                am.append(int(np.argmax(lg)))
                lp.append(float(f64_logprobs(lg, [g])[0]))
            r["score"] = (np.array(am, dtype=np.uint32), np.array(lp), st)
            self.rows.append(r)
        om.free()
        for k in self.states:
            self.states[k].setflags(write=False)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """(name, fmt, weights) -> (path, _Reference): each file is written once per module, the stressed one as a rewritten copy of the plain one."""
    library()
    O.lib().orc_set_fast(1)     # (the AVX row kernels: bit-identical to the scalar oracle, tests/test_oracle_golden.py)
    base = tmp_path_factory.mktemp("injected")
    plain, made = {}, {}

    def get(key):
        name, fmt, weights = key
        if key not in made:
            if (name, fmt) not in plain:
                plain[(name, fmt)] = str(base / f"{name}-{fmt}-plain.bin")
                synth.write_model(plain[(name, fmt)], synth.CONFIGS[name], fmt, seed=SEED)
            p = plain[(name, fmt)]
            if weights == "stress":
                p = str(base / f"{name}-{fmt}-stress.bin")
                shutil.copyfile(plain[(name, fmt)], p)
                done = S.rewrite_f32_vectors(p, S.stress_vectors(ARCH_OF[name], SEED))
                assert set(done) == S.expected_names(ARCH_OF[name], synth.CONFIGS[name].n_layer)
            made[key] = (p, _Reference(p, None if name.startswith("test-") else BIG_FAMILIES))
        return made[key]
    yield get
    O.lib().orc_set_fast(0)
    for p in set(plain.values()) | {p for p, _ in made.values()}:
        os.remove(p)


def _same(got, want, *what):
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(got, want), what + (int((got != want).sum()), "differ; first at", int((got != want).argmax()),
                                              float(got.reshape(-1)[(got != want).argmax()]), float(want.reshape(-1)[(got != want).argmax()]))


@pytest.mark.parametrize("key,paths", CASES, ids=IDS)
def test_plain_abi_from_an_injected_state_on_every_path(files, key, paths):
    path, ref = files(key)
    for label, *_ in paths:
        m = _open(path, paths, label)
        for family, s0 in ref.states.items():
            st = s0.copy()
            for i, (ol, ost) in enumerate(ref.serial[family]):
                lg, st = m.eval(ref.tokens[i], st)
                _same(st, ost, key, label, family, i, "state")
                _same(lg, ol, key, label, family, i, "logits")
        assert m.healthy()
        m.free()


@pytest.mark.parametrize("key,paths", CASES, ids=IDS)
def test_resident_loops_from_a_loaded_state_on_every_path(files, key, paths):
    path, ref = files(key)
    for label, *_ in paths:
        m = _open(path, paths, label)
        for family, s0 in ref.states.items():
            want, ost = ref.greedy[family]
            m.state_load(s0.copy())
            toks, _ = m.decode_greedy(FIRST, N_GREEDY)
            assert list(toks) == want, (key, label, family, list(toks), want)
            _same(m.state_store(), ost, key, label, family, "state after decode_greedy")
            m.state_load(s0.copy())
            toks, _ = m.decode_sample(FIRST, N_GREEDY, temperature=0.0, top_p=0.9, seed=1)
            assert list(toks) == want, (key, label, family, "decode_sample(temperature=0)", list(toks), want)
            _same(m.state_store(), ost, key, label, family, "state after decode_sample")
        assert m.healthy()
        m.free()


@pytest.mark.parametrize("key,paths", CASES, ids=IDS)
def test_sequence_kernels_from_an_injected_state(files, key, paths):
    path, ref = files(key)
    m = _open(path, paths, "top")
    for family, s0 in ref.states.items():
        ol, ost = ref.seq[family]
        for what, (lg, st) in (("eval_sequence", m.eval_sequence(ref.tokens, s0.copy())),
                               ("eval_sequence_in_chunks", m.eval_sequence_in_chunks(ref.tokens, s0.copy(), chunk_size=CHUNK))):
            _same(st, ost, key, family, what, "state")
            _same(lg, ol, key, family, what, "logits")
            lg, st = m.eval(FOLLOW, st)
            _same(st, ref.follow[family][1], key, family, what, "state of the eval that follows")
            _same(lg, ref.follow[family][0], key, family, what, "logits of the eval that follows")
    m.free()


@pytest.mark.parametrize("key,paths", CASES, ids=IDS)
def test_rows_and_segments_from_injected_states(files, key, paths):
    path, ref = files(key)
    m = _open(path, paths, "top")
    V, slots = ref.V, list(range(len(SEG_LENS)))
    b = pkg.RWKVBatch(m, len(slots))
    for s in slots:
        b.state_load(s, ref.states[ref.slot_family[s]].copy())
    for p in range(N_PASSES):
        lg = b.eval(slots, [_row_tokens(p, s, 1, V)[0] for s in slots])
        for s in slots:
            _same(lg[s], ref.rows[s]["passes"][p], key, "eval pass", p, "slot", s, ref.slot_family[s])
    for s in slots:
        _same(b.state_store(s), ref.rows[s]["state_passes"], key, "state after the eval passes, slot", s, ref.slot_family[s])
    lg = b.eval_ragged(slots, [ref.rows[s]["segment"] for s in slots])
    for s in slots:
        _same(b.state_store(s), ref.rows[s]["ragged"][1], key, "state after eval_ragged, slot", s, ref.slot_family[s])
        _same(lg[s], ref.rows[s]["ragged"][0], key, "eval_ragged, slot", s, ref.slot_family[s])
    lps, ams = b.score_ragged(slots, [ref.rows[s]["segment"] for s in slots], [ref.rows[s]["targets"] for s in slots])
    for s in slots:
        am, lp, ost = ref.rows[s]["score"]
        _same(b.state_store(s), ost, key, "state after score_ragged, slot", s, ref.slot_family[s])
        _same(ams[s], am, key, "argmax of score_ragged, slot", s, ref.slot_family[s])
        r32 = lp.astype(np.float32)
        err, tol = np.abs(lps[s].astype(np.float64) - r32.astype(np.float64)), np.spacing(np.abs(r32)).astype(np.float64) + 2.0 ** -32
        assert (err <= tol).all(), (key, "log-probs of score_ragged, slot", s, float((err - tol).max()))
    b.free()
    m.free()
