"""k6_ring's row sums through wave_sum_scatter (ring_v6.hip): the same halving trees as wave_sum_n, every node formed once.

(a) The hook (include/rwkv_testhooks_rowsum.h) runs both forms on the same 64 x N values in one wave, for every N from 2 to 16 -- the
    kernel instantiates N = 2, 3, 4, 6, 8 and 12 ((TF + 1) * R of the row phases of the three geometries, and the comm wave's 2 * KCOMM)
    -- and both results must be the same 32-bit patterns. NaN: where the butterfly's total is a NaN the scatter's must be a NaN; the
    payload is left out of the comparison (which NaN survives an addition of two NaNs follows the operand order, and the two lanes of a
    pair add in opposite orders).
(b) The whole kernel against the CPU oracle, bit for bit, on the models of tests/test_gpu_ring_topup.py (the smallest on which the row
    paths differ) plus the 2560-wide geometry where synth.CONFIGS has a small one."""
import ctypes
import os

import numpy as np
import pytest

import oracle_lib as O
import gpu_lib
from gpu_lib import library, model, synth

pytestmark = pytest.mark.gpu

NS = list(range(2, 17))
INSTANTIATED = (2, 3, 4, 6, 8, 12)

_hook = []


def hook():
    if not _hook:
        library()                                        # (torch first, the libraries built)
        L = gpu_lib.pkg.RWKVSharedLibrary(gpu_lib.pkg.SAMPLE_HOOKS_LIB_PATH).library
        L.rwkv_test_ring_rowsum.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
        L.rwkv_test_ring_rowsum.restype = ctypes.c_bool
        _hook.append(L)
    return _hook[0]


def both(values):
    """values [n][64] float32 -> (butterfly [n][64], scatter's total of value i in every lane that holds it [n][lanes])"""
    n = values.shape[0]
    v = np.ascontiguousarray(values, dtype=np.float32)
    bf, sc, lanes = np.empty((n, 64), np.float32), np.empty(64, np.float32), ctypes.c_int(0)
    assert hook().rwkv_test_ring_rowsum(n, v.ctypes.data, bf.ctypes.data, sc.ctypes.data, ctypes.byref(lanes))
    w = lanes.value
    assert w * n <= 64 and w in (4, 8, 16, 32)
    return bf, sc[:n * w].reshape(n, w), w


def cases(n):
    rng = np.random.default_rng(1000 + n)
    normal = rng.standard_normal((n, 64)).astype(np.float32)
    spread = (10.0 ** rng.uniform(-30, 30, (n, 64)) * rng.choice([-1.0, 1.0], (n, 64))).astype(np.float32)
    tiny = (rng.integers(0, 1 << 23, (n, 64)).astype(np.uint32) | (rng.integers(0, 2, (n, 64)).astype(np.uint32) << 31)).view(np.float32).copy()   # denormals
    tiny[:, ::5] = 0.0
    tiny[:, 1::7] = -0.0
    zeros = np.where(rng.integers(0, 2, (n, 64)) == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    zeros[0] = -0.0                                      # (a sum of -0 only stays -0)
    inf = normal.copy()
    inf[np.arange(n), (7 * np.arange(n) + 3) % 64] = np.inf
    nan = normal.copy()
    nan[np.arange(n), (11 * np.arange(n) + 5) % 64] = np.nan
    return {"normal": normal, "spread": spread, "denormal": tiny, "zeros": zeros, "inf": inf, "nan": nan}


@pytest.mark.parametrize("n", NS)
def test_scatter_forms_the_butterflys_bits(n):
    assert set(INSTANTIATED) <= set(NS)
    for name, v in cases(n).items():
        bf, sc, w = both(v)
        for i in range(n):
            ref = bf[i, i * w:(i + 1) * w]               # the butterfly's total in the lanes that hold the scatter's
            a, b = ref.view(np.uint32), sc[i].view(np.uint32)
            if name == "nan":
                assert np.isnan(bf[i]).all() and np.isnan(sc[i]).all(), (name, n, i)
                continue
            assert np.array_equal(a, b), (name, n, i, ref[0], sc[i][0])
            assert (bf[i].view(np.uint32) == a[0]).all(), (name, n, i)          # (every lane of the butterfly holds the same total)
        if name == "inf":
            assert np.isposinf(sc).all()
        if name == "zeros":
            assert np.signbit(sc[0]).all() and (sc == 0).all()


TOKENS = [1, 2, 3, 400, 5, 77, 300, 9, 11, 12]   # (every test vocabulary has at least 512 entries)
MODELS = [("mega-v6-4096", "Q4_0"), ("mega-v6-4096", "Q8_0"), ("mega-v6-4096", "Q5_1"), ("mega-v6-2048", "Q4_0"), ("mega-v6-4096-v4k", "Q4_0")]
MODELS += [(k, "Q4_0") for k in ("mega-v6-2560",) if k in synth.CONFIGS]

_ref = {}


@pytest.fixture
def reference(tmp_path_factory):
    """The model file and the oracle's results, computed once per model (never written to afterwards)."""
    def get(name, fmt):
        if (name, fmt) not in _ref:
            p = str(tmp_path_factory.mktemp("rowsum") / f"{name}-{fmt}.bin")
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
    keep = {k: os.environ.get(k) for k in ("RWKV_MI_PERSIST", "RWKV_MI_NO_AUTOTUNE")}
    os.environ["RWKV_MI_PERSIST"] = "ring"
    os.environ["RWKV_MI_NO_AUTOTUNE"] = "1"
    yield
    for k, v in keep.items():
        if v is None: os.environ.pop(k, None)
        else: os.environ[k] = v


@pytest.mark.parametrize("name,fmt", MODELS)
def test_ring_matches_oracle_bit_for_bit(reference, ring_env, name, fmt):
    library()
    p, logits, states, greedy, gstate = reference(name, fmt)
    m = model(p)
    assert m.decode_path() == 2 and m.persist_kind() == 2, "ring kernel not selected"
    st = None
    for i, t in enumerate(TOKENS):
        lg, st = m.eval(t, st)
        assert np.array_equal(lg, logits[i]), (name, fmt, i, float(np.abs(lg - logits[i]).max()))
        assert np.array_equal(st, states[i]), (name, fmt, i, float(np.abs(st - states[i]).max()))
    m.state_load(None)
    toks, _ = m.decode_greedy(5, 8)
    assert list(toks) == greedy, (name, fmt)
    assert np.array_equal(m.state_store(), gstate), (name, fmt)
    assert m.healthy()
    m.free()
