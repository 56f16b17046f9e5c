"""k6_ring with records topped up into registers when a gather completes (take_landed, RWKV_MI_RING_TOPUP): every mask computes what
the CPU oracle computes, bit for bit. The mask only chooses WHEN a landed record leaves the ring for the register buffer that waits
for it: bit 0 in front of prologue A (W1 + r/k/v/g records), bit 1 in front of prologue F (ffn key + receptance records), bit 2 in
front of the kq hand-over (ffn value records, where they are held in registers at all).
Models: the smallest on which the buffer logic differs -- D = 4096 Q4_0 (NPK 5, NPG 3), Q8_0 (NPK 2, NPG 1, no value records ahead,
records lap the ring), Q5_1 (NPK 4), D = 2048 Q4_0 (16 key sets, consumer waves 4 and 5 outside the prologues), and a vocabulary
whose head is folded in behind the last layer."""
import os

import numpy as np
import pytest

import oracle_lib as O
from gpu_lib import library, model, synth

pytestmark = pytest.mark.gpu

TOKENS = [1, 2, 3, 400, 5, 77, 300, 9, 11, 12]   # (every test vocabulary has at least 512 entries)
MODELS = [("mega-v6-4096", "Q4_0"), ("mega-v6-4096", "Q8_0"), ("mega-v6-4096", "Q5_1"), ("mega-v6-2048", "Q4_0"), ("mega-v6-4096-v4k", "Q4_0")]
MASKS = [0, 1, 2, 3, 7]

_ref = {}


@pytest.fixture
def reference(tmp_path_factory):
    """The model file and the oracle's results, computed once per model and shared by its masks (never written to afterwards)."""
    def get(name, fmt):
        if (name, fmt) not in _ref:
            p = str(tmp_path_factory.mktemp("topup") / f"{name}-{fmt}.bin")
            synth.write_model(p, synth.CONFIGS[name], fmt, seed=13)
            om = O.OracleModel(p)
            ost, logits, states = om.init_state(), [], []
            for t in TOKENS:
                ol, ost = om.eval(t, ost)
                logits.append(ol.copy()); states.append(ost.copy())
            ost, tok, greedy = om.init_state(), 5, []
            for _ in range(8):
                ol, ost = om.eval(tok, ost)
                tok = int(np.argmax(ol))
                greedy.append(tok)
            om.free()
            for a in logits + states: a.setflags(write=False)
            gstate = ost.copy(); gstate.setflags(write=False)
            _ref[(name, fmt)] = (p, logits, states, greedy, gstate)
        return _ref[(name, fmt)]
    return get


@pytest.fixture
def ring_env():
    keep = {k: os.environ.get(k) for k in ("RWKV_MI_PERSIST", "RWKV_MI_NO_AUTOTUNE", "RWKV_MI_RING_TOPUP")}
    os.environ["RWKV_MI_PERSIST"] = "ring"
    os.environ["RWKV_MI_NO_AUTOTUNE"] = "1"
    yield
    for k, v in keep.items():
        if v is None: os.environ.pop(k, None)
        else: os.environ[k] = v


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("name,fmt", MODELS)
def test_topup_mask_matches_oracle(reference, ring_env, name, fmt, mask):
    library()
    p, logits, states, greedy, gstate = reference(name, fmt)
    os.environ["RWKV_MI_RING_TOPUP"] = str(mask)      # (read when the context is created)
    m = model(p)
    assert m.decode_path() == 2 and m.persist_kind() == 2, "ring kernel not selected"
    st = None
    for i, t in enumerate(TOKENS):
        lg, st = m.eval(t, st)
        assert np.array_equal(lg, logits[i]), (name, fmt, mask, i, float(np.abs(lg - logits[i]).max()))
        assert np.array_equal(st, states[i]), (name, fmt, mask, i, float(np.abs(st - states[i]).max()))
    m.state_load(None)
    toks, _ = m.decode_greedy(5, 8)
    assert list(toks) == greedy, (name, fmt, mask)
    assert np.array_equal(m.state_store(), gstate), (name, fmt, mask)
    assert m.healthy()
    m.free()
