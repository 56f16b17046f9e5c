"""k_mmq_rows (csrc/rows_mm.hip), the quantised product for 2 .. 31 tokens, through lib/librwkv_testhooks_rows_mm.so (librwkv_testhooks.so + the
launch counter). Kernel level: hand-built blocks (tests/blocks_lib.py), all formats; (K, N) = (64, 37): 62 empty leaves, a ragged panel; (2080, 130):
leaf 0 holds two blocks; (4160, 37): chains of 3 and 2; T at the edges of one and two token tiles. Model level: synth D = 256."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import blocks_lib as B
import f64_model as F
import oracle_lib as O
from gpu_lib import pkg, synth
from test_cpu_f64_reference import QUANT_TOL, _err

pytestmark = pytest.mark.gpu

SEED = 7


@functools.lru_cache(None)
def hooks():
    pkg.build_library()
    lib = pkg.RWKVSharedLibrary(os.path.join(os.path.dirname(pkg.LIB_PATH), "librwkv_testhooks_rows_mm.so"))
    lib.library.rwkv_mi_test_mul_mat.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    lib.library.rwkv_mi_test_mul_mat.restype = ctypes.c_bool
    lib.library.rwkv_mi_test_mmq_rows_launches.restype = ctypes.c_uint64
    return lib


def launches():
    return int(hooks().library.rwkv_mi_test_mmq_rows_launches())


def gpu_mul_mat(t, w, K, N, x):
    """gpu_lib.gpu_mul_mat through the library that carries the counter."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, K)
    y = np.empty((x.shape[0], N), dtype=np.float32)
    assert hooks().library.rwkv_mi_test_mul_mat(t, np.ascontiguousarray(w).ctypes.data, K, N, x.ctypes.data, x.shape[0], y.ctypes.data)
    return y


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _operands(fmt, K, N, T):
    t = B.QTYPES[fmt]
    w, _ = B.take_rows(B.weight_rows(t, K, SEED)[0], t, K, T, N)
    ops = B.token_operands(K, T, SEED)
    return t, w, ops[(T + K // 32) % len(ops)][0]


@pytest.mark.parametrize("T", [2, 15, 16, 17, 31])
@pytest.mark.parametrize("K,N", [(64, 37), (2080, 130), (4160, 37)])
@pytest.mark.parametrize("fmt", list(B.QTYPES))
def test_product_is_the_single_token_kernel_token_by_token(fmt, K, N, T):
    t, w, x = _operands(fmt, K, N, T)
    before = launches()
    y = gpu_mul_mat(t, w, K, N, x)
    assert launches() == before + 1, "k_mmq_rows did not run exactly once"
    ref = O.mul_mat(t, w, K, N, x)
    bad = _bits(y) != _bits(ref)
    assert not bad.any(), (fmt, K, N, T, int(bad.sum()), [(int(i), int(j), float(y[i, j]), float(ref[i, j])) for i, j in zip(*np.nonzero(bad))][:8])
    alone = np.concatenate([gpu_mul_mat(t, w, K, N, x[i]) for i in range(T)])
    assert launches() == before + 1 and np.array_equal(_bits(y), _bits(alone)), (fmt, K, N, T)
    e = _err(y, F._Matrix(t, (K, N), w.tobytes())(x))
    print("ROWS-MM", fmt, K, N, T, f"float64 criterion {e:.3e}")
    assert np.isfinite(y).all() and e <= QUANT_TOL, (fmt, K, N, T, e)


def test_switch_keeps_the_token_tiled_kernel(tmp_path):
    """RWKV_MI_ROWS_MM=tn in a fresh process (the switch is read once): the same bits, the counter stays at zero."""
    t, w, x = _operands("Q5_1", 2080, 130, 17)
    np.save(tmp_path / "y.npy", gpu_mul_mat(t, w, 2080, 130, x))
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import test_gpu_rows_mm as M; t, w, x = M._operands('Q5_1', 2080, 130, 17); "
            "y = M.gpu_mul_mat(t, w, 2080, 130, x); assert M.launches() == 0, M.launches(); "
            "assert np.array_equal(y.view(np.uint32), np.load(%r).view(np.uint32))" % (os.path.dirname(__file__), str(tmp_path / "y.npy")))
    subprocess.run([sys.executable, "-c", code], env=dict(os.environ, RWKV_MI_ROWS_MM="tn"), check=True, timeout=300)


MODELS = [("test-v6", "Q4_0"), ("test-v6", "Q8_0"), ("test-v7", "Q5_1"), ("test-v4", "Q4_1")]


@pytest.fixture(scope="module", params=MODELS, ids=["-".join(m) for m in MODELS])
def model(request, tmp_path_factory):
    name, fmt = request.param
    p = str(tmp_path_factory.mktemp("rows_mm") / f"{name}-{fmt}.bin")
    synth.write_model(p, synth.CONFIGS[name], fmt, seed=SEED)
    m = pkg.RWKVModel(hooks(), p, thread_count=2, gpu_layer_count=0)
    yield m
    m.free()
    os.remove(p)


def _alone(m, tokens, state=None):
    """rwkv_eval of one sequence: (logits of the last token, state)."""
    lg = None
    for tok in tokens:
        lg, state = m.eval(int(tok), state)
    return lg, state


def _tok(m, s, p):
    return (7 + 13 * s + 5 * p) % m.n_vocab


@pytest.mark.parametrize("n", [2, 16, 17])
def test_batch_rows_equal_each_sequence_alone(model, n):
    m, slots = model, list(range(n))
    b = pkg.RWKVBatch(m, n)
    for s in slots:
        b.state_load(s, None)
    before = launches()
    for p in range(2):
        lg = b.eval(slots, [_tok(m, s, p) for s in slots])
    toks, _ = b.decode_greedy(slots, [_tok(m, s, 2) for s in slots], 3)
    assert launches() > before, "k_mmq_rows did not run"
    for s in slots:
        ref_lg, st = _alone(m, [_tok(m, s, 0), _tok(m, s, 1)])
        assert np.array_equal(_bits(lg[s]), _bits(ref_lg)), (n, s, "logits")
        tok, want = _tok(m, s, 2), []
        for _ in range(3):
            l2, st = m.eval(tok, st)
            tok = int(np.argmax(l2))
            want.append(tok)
        assert list(toks[s]) == want and np.array_equal(_bits(b.state_store(s)), _bits(st)), (n, s, "decode_greedy")
    b.free()


def test_sequence_and_ragged_pass_equal_serial_eval(model):
    m = model
    seq = [_tok(m, 3, p) for p in range(17)]
    before = launches()
    lg, st = m.eval_sequence(seq, None)
    assert launches() > before, "k_mmq_rows did not run"
    ref_lg, ref_st = _alone(m, seq)
    assert np.array_equal(_bits(lg), _bits(ref_lg)) and np.array_equal(_bits(st), _bits(ref_st))
    rows = [[_tok(m, s, p) for p in range(n)] for s, n in enumerate((1, 9, 3))]
    b = pkg.RWKVBatch(m, 3)
    for s in range(3):
        b.state_load(s, None)
    lg = b.eval_ragged([0, 1, 2], rows)
    for s in range(3):
        ref_lg, ref_st = _alone(m, rows[s])
        assert np.array_equal(_bits(lg[s]), _bits(ref_lg)) and np.array_equal(_bits(b.state_store(s)), _bits(ref_st)), s
    b.free()
