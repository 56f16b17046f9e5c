"""k_mmf_rows (csrc/rows_mf.hip), the F16 / F32 product for 5 .. 31 tokens, through lib/librwkv_testhooks_rows_mf.so (librwkv_testhooks.so + the
launch counter). Kernel level: the operands of tests/fx_lib.py; (K, N) = (32, 37): one slice of a 128-step, three absent, a ragged panel; (160, 37):
a tail of one slice; (2112, 70): many chunks, a tail of two, past k_mvf's 2048-element tile; T at the edges of one and two token tiles. Model level:
synth D = 256, an FP16 file and a Q5_1 one (F16 head and low-rank stages).

The float64 bound: K / 32 + 5 roundings on any path of the pinned order, so |y - sum| <= (K / 32 + 5) (2^-24 sum |w x| + 2^-149), held wherever the
float64 sum is finite and sum |w x| < 2^127 -- inside float32's range; finite in float64 alone would admit the `huge` weight row, whose
float32 sums overflow to inf and NaN in the oracle too. The oracle's own worst ratio on these operands is 0.51."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import fx_lib as X
import oracle_lib as O
from gpu_lib import pkg, synth

pytestmark = pytest.mark.gpu

SEED = 7


@functools.lru_cache(None)
def hooks():
    pkg.build_library()
    lib = pkg.RWKVSharedLibrary(os.path.join(os.path.dirname(pkg.LIB_PATH), "librwkv_testhooks_rows_mf.so"))
    lib.library.rwkv_mi_test_mul_mat.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    lib.library.rwkv_mi_test_mul_mat.restype = ctypes.c_bool
    lib.library.rwkv_mi_test_mmf_rows_launches.restype = ctypes.c_uint64
    return lib


def launches():
    return int(hooks().library.rwkv_mi_test_mmf_rows_launches())


def gpu_mul_mat(t, w, K, N, x):
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, K)
    y = np.empty((x.shape[0], N), dtype=np.float32)
    assert hooks().library.rwkv_mi_test_mul_mat(t, np.ascontiguousarray(w).ctypes.data, K, N, x.ctypes.data, x.shape[0], y.ctypes.data)
    return y


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(y, ref):
    """isnan positions equal, bit patterns equal everywhere else"""
    ny, nr = np.isnan(y), np.isnan(ref)
    return np.array_equal(ny, nr) and np.array_equal(_bits(y)[~ny], _bits(ref)[~nr])


def _operands(fmt, K, N, T):
    """(type, payload bytes, the rows behind them, x): N fx_lib weight rows from row T on and one rotation of the activation families"""
    t = X.TYPE_NAMES[fmt]
    w = X.weight_rows(t, K, SEED)[0]
    wb, idx = X.take_rows(w, T, N)
    ops = X.token_operands(K, T, SEED)
    return t, wb, w[idx], ops[(T + K // 32) % len(ops)][0]


@pytest.mark.parametrize("T", [5, 15, 16, 17, 31])
@pytest.mark.parametrize("K,N", [(32, 37), (160, 37), (2112, 70)])
@pytest.mark.parametrize("fmt", list(X.TYPE_NAMES))
def test_product_is_k_mvf_token_by_token(fmt, K, N, T):
    t, wb, rows, x = _operands(fmt, K, N, T)
    before = launches()
    y = gpu_mul_mat(t, wb, K, N, x)
    assert launches() == before + 1, "k_mmf_rows did not run exactly once"
    assert _same(y, O.mul_mat(t, wb, K, N, x)), (fmt, K, N, T, "oracle")
    alone = np.concatenate([gpu_mul_mat(t, wb, K, N, x[i]) for i in range(T)])
    assert launches() == before + 1 and _same(y, alone), (fmt, K, N, T, "token by token")
    ref, mag = X.float64_sum(t, rows, x)
    ok = np.isfinite(ref) & (mag < 2.0 ** 127)
    with np.errstate(all="ignore"):
        ratio = np.nan_to_num((np.abs(y.astype(np.float64) - ref) / ((K / 32 + 5) * (2.0 ** -24 * mag + 2.0 ** -149)))[ok], nan=np.inf).max()
    print("ROWS-MF", fmt, K, N, T, f"float64 bound: worst ratio {ratio:.3f} over {int(ok.sum())} outputs")
    assert ok.any() and ratio <= 1.0, (fmt, K, N, T, ratio)


@pytest.mark.parametrize("T", [4, 32])
def test_gate_leaves_four_and_thirty_two_tokens_alone(T):
    t, wb, _, x = _operands("FP16", 160, 37, T)
    before = launches()
    assert _same(gpu_mul_mat(t, wb, 160, 37, x), O.mul_mat(t, wb, 160, 37, x)) and launches() == before


@pytest.mark.parametrize("K", [32, 160])
def test_negative_underflow_keeps_its_sign(K):
    """F32 weights 1e-30 against activations -1e-30: every product underflows to -0; an absent slice of the tail must leave it -0."""
    w, x = np.full((37, K), 1e-30, dtype=np.float32), np.full((17, K), -1e-30, dtype=np.float32)
    before = launches()
    y = gpu_mul_mat(X.F32, w.view(np.uint8).reshape(-1), K, 37, x)
    assert launches() == before + 1 and (_bits(y) == 0x80000000).all(), (K, sorted({hex(int(v)) for v in _bits(y).reshape(-1)}))


def test_switch_keeps_the_token_tiles(tmp_path):
    """RWKV_MI_ROWS_MF=valu in a fresh process (the switch is read once): the same bits, the counter stays at zero."""
    t, wb, _, x = _operands("FP16", 2112, 70, 17)
    np.save(tmp_path / "y.npy", gpu_mul_mat(t, wb, 2112, 70, x))
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import test_gpu_rows_mf as M; t, wb, _, x = M._operands('FP16', 2112, 70, 17); "
            "y = M.gpu_mul_mat(t, wb, 2112, 70, x); assert M.launches() == 0, M.launches(); "
            "assert M._same(y, np.load(%r))" % (os.path.dirname(__file__), str(tmp_path / "y.npy")))
    subprocess.run([sys.executable, "-c", code], env=dict(os.environ, RWKV_MI_ROWS_MF="valu"), check=True, timeout=300)


MODELS = [("test-v6", "FP16"), ("test-v7", "Q5_1")]


@pytest.fixture(scope="module", params=MODELS, ids=["-".join(m) for m in MODELS])
def model(request, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("rows_mf") / "-".join(request.param))
    synth.write_model(p, synth.CONFIGS[request.param[0]], request.param[1], seed=SEED)
    m = pkg.RWKVModel(hooks(), p, thread_count=2, gpu_layer_count=0)
    yield m
    m.free()
    os.remove(p)


def _tok(m, s, p):
    return (7 + 13 * s + 5 * p) % m.n_vocab


def _alone(m, s, n, greedy=0):
    """rwkv_eval of sequence s alone: n tokens of _tok, then `greedy` tokens of its own choice -> (logits after the n, state, the choices)"""
    state, tok, out = None, _tok(m, s, n), []
    for p in range(n):
        lg, state = m.eval(_tok(m, s, p), state)
    for _ in range(greedy):
        l2, state = m.eval(tok, state)
        tok = int(np.argmax(l2))
        out.append(tok)
    return lg, state, out


@pytest.mark.parametrize("n", [5, 16, 17])
def test_batch_rows_equal_each_sequence_alone(model, n):
    m, slots = model, list(range(n))
    b = pkg.RWKVBatch(m, n)
    for s in slots:
        b.state_load(s, None)
    before = launches()
    for p in range(2):
        lg = b.eval(slots, [_tok(m, s, p) for s in slots])
    toks, _ = b.decode_greedy(slots, [_tok(m, s, 2) for s in slots], 3)
    assert launches() > before, "k_mmf_rows did not run"
    for s in slots:
        ref_lg, st, want = _alone(m, s, 2, greedy=3)
        assert np.array_equal(_bits(lg[s]), _bits(ref_lg)) and list(toks[s]) == want and np.array_equal(_bits(b.state_store(s)), _bits(st)), (n, s)
    b.free()


def test_sequence_and_ragged_pass_equal_serial_eval(model):
    m, before = model, launches()
    lg, st = m.eval_sequence([_tok(m, 3, p) for p in range(17)], None)
    assert launches() > before, "k_mmf_rows did not run in eval_sequence"
    ref_lg, ref_st, _ = _alone(m, 3, 17)
    assert np.array_equal(_bits(lg), _bits(ref_lg)) and np.array_equal(_bits(st), _bits(ref_st))
    b = pkg.RWKVBatch(m, 3)
    for s in range(3):
        b.state_load(s, None)
    before = launches()
    lg = b.eval_ragged([0, 1, 2], [[_tok(m, s, p) for p in range(n)] for s, n in enumerate((1, 9, 3))])
    assert launches() > before, "k_mmf_rows did not run in eval_ragged"
    for s, n in enumerate((1, 9, 3)):
        ref_lg, ref_st, _ = _alone(m, s, n)
        assert np.array_equal(_bits(lg[s]), _bits(ref_lg)) and np.array_equal(_bits(b.state_store(s)), _bits(ref_st)), s
    b.free()
