"""k6_ring exists twice: the product instantiation (no stamp, no trace store, no RWKV_MI_RING_DBG branch compiled in) and the instrumented
one (ring_v6_instr.hip), which the host launches exactly while a trace slot is bound. Both compute what the CPU oracle computes, bit for
bit, and a context may change from one to the other between two tokens: the hand-over generation in the control words runs on.

Ten tokens are decoded one by one; with `trace` set, rwkv_mi_trace_phases is called behind the third and behind the seventh token. The call
binds the slot, runs two tokens of its own through the instrumented kernel and unbinds it, so the sequence goes product -> instrumented ->
product twice (the serial evaluation passes its state in with every token: what the call did to the context's own state does not matter).
Logits and state behind every token must equal the oracle's -- with and without the trace calls, i.e. the two runs give the same arrays --
and so must a greedy decode behind them. The stamps the call returns must be monotonic per wave.
Models: those of test_gpu_ring_topup.py -- D = 4096 Q4_0 / Q8_0 / Q5_1, D = 2048 Q4_0 (16 key sets, consumer waves 4 and 5 outside the
prologues), and a vocabulary whose head is folded in behind the last layer."""
import ctypes
import os

import numpy as np
import pytest

import oracle_lib as O
from gpu_lib import library, model, synth

pytestmark = pytest.mark.gpu

TOKENS = [1, 2, 3, 400, 5, 77, 300, 9, 11, 12]   # (every test vocabulary has at least 512 entries)
MODELS = [("mega-v6-4096", "Q4_0"), ("mega-v6-4096", "Q8_0"), ("mega-v6-4096", "Q5_1"), ("mega-v6-2048", "Q4_0"), ("mega-v6-4096-v4k", "Q4_0")]
TRACE_BEHIND = (3, 7)                            # tokens decoded when rwkv_mi_trace_phases is called

_ref = {}


@pytest.fixture
def reference(tmp_path_factory):
    """The model file and the oracle's results, computed once per model and shared by both runs (never written to afterwards)."""
    def get(name, fmt):
        if (name, fmt) not in _ref:
            p = str(tmp_path_factory.mktemp("variants") / f"{name}-{fmt}.bin")
            synth.write_model(p, synth.CONFIGS[name], fmt, seed=29)
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
    keep = {k: os.environ.get(k) for k in ("RWKV_MI_PERSIST", "RWKV_MI_NO_AUTOTUNE")}
    os.environ["RWKV_MI_PERSIST"] = "ring"
    os.environ["RWKV_MI_NO_AUTOTUNE"] = "1"
    yield
    for k, v in keep.items():
        if v is None: os.environ.pop(k, None)
        else: os.environ[k] = v


def _trace(lib, m):
    L = lib.library
    L.rwkv_mi_trace_phases.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L.rwkv_mi_trace_phases.restype = ctypes.c_bool
    out = np.zeros(256 * 8 * 32, dtype=np.int64)
    assert L.rwkv_mi_trace_phases(m._ctx.ptr, 5, 1, 2, out.ctypes.data)
    t = out.reshape(256, 8, 32)
    assert (np.diff(t[:, 2:, :14], axis=2) >= 0).all() and (t[:, 2:, 13] > t[:, 2:, 0]).all()   # consumer waves
    assert (np.diff(t[:, 1, :12], axis=1) >= 0).all()                                              # comm wave
    assert (t[:, 0, 1] > t[:, 0, 0]).all()                                                         # loader: start / end


@pytest.mark.parametrize("trace", [False, True])
@pytest.mark.parametrize("name,fmt", MODELS)
def test_product_and_instrumented_kernel_match_oracle(reference, ring_env, name, fmt, trace):
    lib = library()
    p, logits, states, greedy, gstate = reference(name, fmt)
    m = model(p)
    assert m.decode_path() == 2 and m.persist_kind() == 2, "ring kernel not selected"
    st = None
    for i, t in enumerate(TOKENS):
        lg, st = m.eval(t, st)
        assert np.array_equal(lg, logits[i]), (name, fmt, trace, i, float(np.abs(lg - logits[i]).max()))
        assert np.array_equal(st, states[i]), (name, fmt, trace, i, float(np.abs(st - states[i]).max()))
        if trace and i + 1 in TRACE_BEHIND:
            _trace(lib, m)
    m.state_load(None)
    toks, _ = m.decode_greedy(5, 8)
    assert list(toks) == greedy, (name, fmt, trace)
    assert np.array_equal(m.state_store(), gstate), (name, fmt, trace)
    assert m.healthy()
    m.free()
