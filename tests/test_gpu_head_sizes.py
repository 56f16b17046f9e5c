"""Every form of the RWKV-5 / 6 / 7 recurrences at head sizes other than 64 (tests/heads_lib.py: S = 16, 32, 96, 128, 512), against the CPU
oracle run from the same state: np.array_equal on logits and on the whole state at every step a call exposes. The oracle's own worth on
these files is held in tests/test_cpu_head_sizes.py. The log-probs of score_ragged have the one tolerance of tests/test_gpu_score.py
(check_logprob, imported).

Per row of the table, format (Q5_1, FP16) and weights (plain, stressed; the D = 1024 rows: stressed, forms a - c), from the `normal`, `large`
and `long-run` states of stress_lib.state_families and from the fresh state -- an injected random state shows a transposed or mis-strided
state index at the first token, a fresh one only later:
  a  a default context: decode_path() == 0 and persist_kind() == 0 (the fused and the persistent paths decline every S != 64); 4 tokens of
     eval(token, state_in); state_load, decode_greedy, state_store, decode_sample at temperature 0
  b  40 tokens with eval_sequence at once and in chunks of 33, then one eval from the returned state; serial == sequence bit for bit
  c  rows: an RWKVBatch of 5 slots from different states, 3 eval passes
  d  segments: one eval_ragged of lengths (1, 3, 33, 40, 2), one score_ragged on the same lists
  e  replay: one eval_draft over four slots with drafts of 4, 6, 5 and 8 tokens cut from the oracle's greedy continuation with one token
     changed, so that they keep the whole draft, a proper prefix of 3, the first draft token only, and x0 alone; every slot's state
     afterwards is the oracle's after exactly the kept tokens
  f  the fast quantised sequence arm (RWKV_MI_SEQ_Q=force, T = 97) on the S = 96 row of RWKV-6 and RWKV-7, Q5_1: held to float64 with the
     criterion and the constant of tests/test_gpu_f64_reference.py, the launch counter showing that the arm ran

Which kernel of csrc/kernels.hip each case launches (seq: a, b; rows: c; segs: d; replay: e -- b with 40 tokens is also the T >= 32 sequence
pass that skips the lane-pipelined launch_wkv6_seq / launch_wkv7_seq, d the ragged pass that keeps every segment in the short launch, and
every case the group norm without its quantising sequence form):
  k_wkv6<32> / _rows / _segs / _replay               v5.1-D256-S32 (u and w per head), v6-D256-S32 (w per token)
  k_wkv6<16> / _rows / _segs / _replay               v5.2-D256-S16 (u and w per channel)
  k_wkv6_generic / _rows_ / _segs_ / _replay_generic v6-D768-S96, v6-D256-S128; v6-D1024-S512 (seq and rows; the 256-thread loop twice)
  k_wkv7<32> / _rows / _segs / _replay               v7-D256-S32
  k_wkv7_generic / _rows_ / _segs_ / _replay_generic v7-D256-S16, v7-D768-S96, v7-D256-S128; v7-D1024-S512 (seq and rows)
  k_groupnorm, k_v7_kprep off one element per lane   S = 16, 32 (idle lanes), 96 (uneven), 128 (two), 512 (eight), every case of the row
tests/test_gpu_recur_kernels.py runs the same kernels on caller-supplied arrays at the head sizes no file can have.

What the two files see that the suite before them does not (one-line mutations of csrc/kernels.hip on a side build, the whole GPU suite run
once on each; "before": the 1357 GPU tests that existed before these two files, of which 1353 pass and 4 skip on the unmutated build):
  wkv6_body_generic reads sin[h S S + j S + i]        61 tests here and in test_gpu_recur_kernels.py fail: every form of the ten generic
  for sin[h S S + i S + j]                            RWKV-6 cases (plain ABI 10, sequence 10, rows 10, segments 8, replay 8), the fast arm of
                                                      RWKV-6, test_wkv6_in_its_three_forms at every generic S (14). Before: 0 fail
  wkv7_body_generic reads state_in at every token,    57 fail: sequence 14, segments 12, replay 12 (every generic RWKV-7 case), the fast arm of
  not at the first only                               RWKV-7, test_wkv7_in_its_three_forms at every generic S (18). The plain ABI and the rows
                                                      run one token per launch and cannot see it. Before: 0 fail
  k_groupnorm divides the sum by 64 for the mean,     202 fail: every case of a - e (40, 40, 40, 36, 36) and test_groupnorm at every S but 64
  not by S                                            (10); the fast arm (f) is a tolerance and passes. Before: 49 fail, all of them on the tiny
                                                      golden files with head size 8 (test_gpu_tiny_rwkv, the golden cases of test_gpu_batch*,
                                                      test_gpu_score, test_gpu_buffer_lifecycle, test_gpu_reference_*): a divisor fixed at 64
                                                      was not invisible before, one that is right at 8 and 64 alone would have been
"""
import os

import numpy as np
import pytest

import f64_model as F
import heads_lib as HL
import oracle_lib as O
import stress_lib as S
from gpu_lib import library, model, pkg, synth
from logprobs_ref import f64_logprobs
from test_gpu_f64_reference import C_FAST, _counter, _err
from test_gpu_injected_state import CHUNK, FIRST, FOLLOW, N_ABI, N_GREEDY, N_PASSES, N_SEQ, SEG_LENS, _row_targets, _row_tokens, _same
from test_gpu_score import check_logprob

pytestmark = pytest.mark.gpu

ENV = ("RWKV_MI_NO_AUTOTUNE", "RWKV_MI_NO_FUSED", "RWKV_MI_NO_MEGA", "RWKV_MI_PERSIST", "RWKV_MI_SEQ_Q", "RWKV_MI_SEQ_F16")
FAMILIES = ("normal", "large", "long-run")
# replay: (draft length k, mismatch position j): min(j, k) draft tokens stand
DRAFTS = ((4, 4), (6, 3), (5, 1), (8, 0))
X0 = 61

KEYS = [(row, fmt, w) for row in HL.ROWS for fmt in HL.FORMATS for w in HL.weights_of(row)]
SMALL_KEYS = [k for k in KEYS if not HL.is_big(k[0])]


def _id(key):
    return f"{HL.row_id(key[0])}-{key[1]}-{key[2]}"


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


class _Reference:
    """What the oracle computes from every start state of one file, computed once and read by every test of the file."""

    def __init__(self, path, big):
        om = O.OracleModel(path)
        self.V = V = om.n_vocab
        fam = S.state_families(om, HL.SEED)
        self.states = {"fresh": om.init_state(), **{k: fam[k] for k in FAMILIES}}
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
            self.greedy[k] = self._greedy(om, s0, FIRST, N_GREEDY)
        # rows, segments and drafts: every slot starts from another state -- the last one from `normal` of another seed -- and runs alone
        pool = {**self.states, "normal-2": S.state_families(om, HL.SEED + 1)["normal"]}
        self.slot_family = ["normal", "large", "long-run", "fresh", "normal-2"]
        self.slot_state = [pool[f] for f in self.slot_family]
        self.rows, self.drafts = [], []
        for slot, n in enumerate(SEG_LENS):
            st, r = self.slot_state[slot], {"passes": []}
            for p in range(N_PASSES):
                lg, st = om.eval(_row_tokens(p, slot, 1, V)[0], st)
                r["passes"].append(lg)
            r["state_passes"] = st
            self.rows.append(r)
            if big:
                continue
            r["segment"] = _row_tokens(N_PASSES, slot, n, V)
            r["ragged"] = lg, st = om.eval_sequence(r["segment"], st)
            r["targets"] = _row_targets(slot, n, V)
            am, lp = [], []
            for t, g in zip(r["segment"], r["targets"]):
                lg, st = om.eval(t, st)
                am.append(int(np.argmax(lg)))
                lp.append(float(f64_logprobs(lg, [g])[0]))
            r["score"] = (np.array(am, dtype=np.uint32), np.array(lp), st)
        if not big:
            for slot, (k, j) in enumerate(DRAFTS):
                s0 = self.slot_state[slot]
                true, _ = self._greedy(om, s0, X0 + slot, k + 1)
                kept = min(j, k)
                draft = [int(t) for t in true[:k]]
                if j < k:
                    draft[j] = (draft[j] + 1) % V
                emitted, st = self._greedy(om, s0, X0 + slot, kept + 1)
                assert emitted == true[:kept + 1]
                self.drafts.append({"row": [X0 + slot] + draft, "emitted": emitted, "state": st})
        om.free()
        for s in self.states.values():
            s.setflags(write=False)

    @staticmethod
    def _greedy(om, st, tok, n):
        out = []
        for _ in range(n):
            lg, st = om.eval(tok, st)
            tok = int(np.argmax(lg))
            out.append(tok)
        return out, st


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """(row, fmt, weights) -> (path, _Reference): each file is written once per module."""
    library()
    O.lib().orc_set_fast(1)     # (the AVX row kernels: bit-identical to the scalar oracle, tests/test_oracle_golden.py)
    made, refs = HL.Files(synth, tmp_path_factory.mktemp("heads")), {}

    def get(key):
        if key not in refs:
            refs[key] = (made(*key), _Reference(made(*key), HL.is_big(key[0])))
        return refs[key]
    yield get
    O.lib().orc_set_fast(0)
    made.close()


def _open(path, key, **kw):
    """A default context of the file: the fused and the persistent paths must decline a head size other than 64, not run with a wrong geometry."""
    m = model(path, **kw)
    assert m.decode_path() == 0 and m.persist_kind() == 0, (key, m.decode_path(), m.persist_kind(), m.persist_info())
    return m


@pytest.mark.parametrize("key", KEYS, ids=_id)
def test_plain_abi_and_resident_loops(files, key):
    """(a)"""
    path, ref = files(key)
    m = _open(path, key)
    assert (m.n_embed, m.n_layer) == (key[0][1], 3 if key[0][0] == "7" else 2)
    for family, s0 in ref.states.items():
        st = s0.copy()
        for i, (ol, ost) in enumerate(ref.serial[family]):
            lg, st = m.eval(ref.tokens[i], st)
            _same(st, ost, key, family, i, "state")
            _same(lg, ol, key, family, i, "logits")
        want, ost = ref.greedy[family]
        m.state_load(s0.copy())
        toks, _ = m.decode_greedy(FIRST, N_GREEDY)
        assert list(toks) == want, (key, family, list(toks), want)
        _same(m.state_store(), ost, key, family, "state after decode_greedy")
        m.state_load(s0.copy())
        toks, _ = m.decode_sample(FIRST, N_GREEDY, temperature=0.0, top_p=0.9, seed=1)
        assert list(toks) == want, (key, family, "decode_sample(temperature=0)", list(toks), want)
        _same(m.state_store(), ost, key, family, "state after decode_sample")
    assert m.healthy()
    m.free()


@pytest.mark.parametrize("key", KEYS, ids=_id)
def test_sequence_forms(files, key):
    """(b)"""
    path, ref = files(key)
    m = _open(path, key)
    for family, s0 in ref.states.items():
        ol, ost = ref.seq[family]
        for what, (lg, st) in (("eval_sequence", m.eval_sequence(ref.tokens, s0.copy())),
                               ("eval_sequence_in_chunks", m.eval_sequence_in_chunks(ref.tokens, s0.copy(), chunk_size=CHUNK))):
            _same(st, ost, key, family, what, "state")
            _same(lg, ol, key, family, what, "logits")
            lg, st = m.eval(FOLLOW, st)
            _same(st, ref.follow[family][1], key, family, what, "state of the eval that follows")
            _same(lg, ref.follow[family][0], key, family, what, "logits of the eval that follows")
        # serial == sequence, bit for bit: the same 40 tokens one eval at a time
        st = s0.copy()
        for t in ref.tokens:
            lg, st = m.eval(t, st)
        _same(st, ost, key, family, "serial", "state")
        _same(lg, ol, key, family, "serial", "logits")
    m.free()


def _batch(m, ref, n):
    b = pkg.RWKVBatch(m, n)
    for s in range(n):
        b.state_load(s, ref.slot_state[s].copy())
    return b


@pytest.mark.parametrize("key", KEYS, ids=_id)
def test_rows(files, key):
    """(c)"""
    path, ref = files(key)
    m = _open(path, key)
    slots = list(range(len(SEG_LENS)))
    b = _batch(m, ref, len(slots))
    for p in range(N_PASSES):
        lg = b.eval(slots, [_row_tokens(p, s, 1, ref.V)[0] for s in slots])
        for s in slots:
            _same(lg[s], ref.rows[s]["passes"][p], key, "eval pass", p, "slot", s, ref.slot_family[s])
    for s in slots:
        _same(b.state_store(s), ref.rows[s]["state_passes"], key, "state after the eval passes, slot", s, ref.slot_family[s])
    b.free()
    m.free()


@pytest.mark.parametrize("key", SMALL_KEYS, ids=_id)
def test_segments(files, key):
    """(d)"""
    path, ref = files(key)
    m = _open(path, key)
    slots = list(range(len(SEG_LENS)))
    b = _batch(m, ref, len(slots))
    for s in slots:
        b.state_load(s, ref.rows[s]["state_passes"].copy())
    lg = b.eval_ragged(slots, [ref.rows[s]["segment"] for s in slots])
    for s in slots:
        _same(b.state_store(s), ref.rows[s]["ragged"][1], key, "state after eval_ragged, slot", s, ref.slot_family[s])
        _same(lg[s], ref.rows[s]["ragged"][0], key, "eval_ragged, slot", s, ref.slot_family[s])
    lps, ams = b.score_ragged(slots, [ref.rows[s]["segment"] for s in slots], [ref.rows[s]["targets"] for s in slots])
    for s in slots:
        am, lp, ost = ref.rows[s]["score"]
        _same(b.state_store(s), ost, key, "state after score_ragged, slot", s, ref.slot_family[s])
        _same(ams[s], am, key, "argmax of score_ragged, slot", s, ref.slot_family[s])
        for i in range(len(lp)):
            check_logprob(lps[s][i], lp[i], (key, "score_ragged, slot", s, "position", i))
    b.free()
    m.free()


@pytest.mark.parametrize("key", SMALL_KEYS, ids=_id)
def test_replay(files, key):
    """(e)"""
    path, ref = files(key)
    m = _open(path, key)
    n = len(DRAFTS)
    b = _batch(m, ref, n + 1)
    untouched = b.state_store(n)
    emitted, lens = b.eval_draft(list(range(n)), [d["row"] for d in ref.drafts])
    for s, d in enumerate(ref.drafts):
        assert emitted[s] == d["emitted"] and int(lens[s]) == min(DRAFTS[s][1], DRAFTS[s][0]) + 1, (key, "slot", s, emitted[s], d["emitted"], int(lens[s]))
        _same(b.state_store(s), d["state"], key, "state after eval_draft, slot", s, ref.slot_family[s], "kept", len(d["emitted"]))
    _same(b.state_store(n), untouched, key, "the slot the call does not name")
    b.free()
    m.free()


@pytest.mark.parametrize("arch", ["6", "7"])
def test_fast_sequence_arm_against_float64(files, arch):
    """(f)"""
    T, key = 97, ((arch, 768, 96), "Q5_1", "plain")
    p = files(key)[0]
    toks = S.lcg_tokens(512, T)
    fl, fs = F.F64Model(p).eval_sequence(toks, None)
    om = O.OracleModel(p)
    ol, ost = om.eval_sequence(toks, om.init_state())
    om.free()
    os.environ["RWKV_MI_SEQ_Q"] = "force"
    m = _open(p, key, hooks=True)
    before = _counter("rwkv_mi_test_mmq_fast_launches")
    gl, gs = m.eval_sequence(toks, None)
    assert _counter("rwkv_mi_test_mmq_fast_launches") > before, "rwkv_mi_test_mmq_fast_launches: the fast arm did not run"
    m.free()
    for what, fast, orc, refv in (("logits", gl, ol, fl), ("state", gs, ost, fs)):
        e_fast, e_orc = _err(fast, refv), _err(orc, refv)
        print(f"v{arch} S96 Q5_1 T{T} {what}: e_oracle {e_orc:.2e} e_fast {e_fast:.2e} ratio {e_fast / max(e_orc, 1e-30):.2f}")
        assert np.isfinite(fast).all() and e_fast <= C_FAST * e_orc + 1e-6, (arch, what, e_fast, e_orc)
