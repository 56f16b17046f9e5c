"""The quantising row producers (csrc/rows_q.hip: k_mix_rows_q, k_v6_mix2_rows_q, k_groupnorm_rows_q) through lib/librwkv_testhooks_rows_q.so
(librwkv_testhooks.so + the two launch counters). Model level: synth files of two layers, V = 512, D = 256 and -- RWKV-6 -- D = 320: ten blocks
per row, a ragged wave of the block-per-lane split and five heads over workgroups of four waves."""
import ctypes
import dataclasses
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import f64_model as F
from gpu_lib import pkg, synth
from test_cpu_f64_reference import QUANT_TOL, _err

pytestmark = pytest.mark.gpu

SEED = 7
# Stand-alone launch_quantize_act calls per layer of a row or segment pass below 32 tokens (Runner, csrc/engine.hip; emb / head are F16 in these files,
# so the head quantises nothing). What stays with the kernels:
#   RWKV-6:  tanh(decay_w1 . xw), the input of time_decay_w2; relu(k)^2, the input of ffn.value
#   RWKV-5:  relu(k)^2, the input of ffn.value
#   RWKV-4:  the WKV output, the input of att.output (no group norm); relu(k)^2, the input of ffn.value
#   RWKV-7:  the inputs of att.receptance, att.key, att.value (the six-output mix) and of att.output (the group norm with the bonus term);
#            relu(k)^2, the input of ffn.value
LEFT = {"6": 2, "5.2": 1, "4": 2, "7": 5}
PLAIN_V6 = 11   # without them, every quantised product's input: maa_w1, r k v g, decay_w1, decay_w2, att.output, ffn k r v
MODELS = [("test-v6", "Q4_0", 256), ("test-v5.2", "Q5_1", 256), ("test-v4", "Q8_0", 256), ("test-v7", "Q4_0", 256), ("test-v6", "Q5_1", 320)]


@functools.lru_cache(None)
def hooks():
    pkg.build_library()
    lib = pkg.RWKVSharedLibrary(os.path.join(os.path.dirname(pkg.LIB_PATH), "librwkv_testhooks_rows_q.so"))
    lib.library.rwkv_mi_test_quant_act_launches.restype = lib.library.rwkv_mi_test_rows_q_launches.restype = ctypes.c_uint64
    return lib


def launches():
    """(stand-alone quantiser launches, launches of the new kernels) of this process"""
    return int(hooks().library.rwkv_mi_test_quant_act_launches()), int(hooks().library.rwkv_mi_test_rows_q_launches())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _open(d, name, fmt, D):
    """(model, path, architecture) of the two-layer file of (name, fmt, D) in directory d"""
    spec = dataclasses.replace(synth.CONFIGS[name], n_layer=2, n_vocab=512, n_embed=D, ffn=D * 7 // 2)
    p = os.path.join(str(d), f"{name}-{fmt}-{D}.bin")
    if not os.path.exists(p):
        synth.write_model(p, spec, fmt, seed=SEED)
    return pkg.RWKVModel(hooks(), p, thread_count=2, gpu_layer_count=0), p, spec.arch


@pytest.fixture(scope="module", params=MODELS, ids=["-".join(map(str, m)) for m in MODELS])
def model(request, tmp_path_factory):
    m, p, arch = _open(tmp_path_factory.mktemp("rows_q"), *request.param)
    yield m, p, arch
    m.free()


def _alone(m, tokens, state=None):
    """rwkv_eval of one sequence: (logits of the last token, state)."""
    lg = None
    for tok in tokens:
        lg, state = m.eval(int(tok), state)
    return lg, state


def _tok(m, s, p):
    return (7 + 13 * s + 5 * p) % m.n_vocab


def _two_passes(m, n):
    """two eval passes over n fresh slots: the batch, the logits of both passes and the counters' growth over each"""
    b = pkg.RWKVBatch(m, n)
    for s in range(n):
        b.state_load(s, None)
    lgs, grew = [], []
    for p in range(2):
        q0, k0 = launches()
        lgs.append(b.eval(list(range(n)), [_tok(m, s, p) for s in range(n)]))
        grew.append((launches()[0] - q0, launches()[1] - k0))
    return b, lgs, grew


@pytest.mark.parametrize("n", [2, 17])
def test_batch_rows_equal_each_sequence_alone(model, n):
    (m, path, arch), slots = model, list(range(n))
    b, lgs, grew = _two_passes(m, n)
    q0 = launches()[0]
    toks, _ = b.decode_greedy(slots, [_tok(m, s, 2) for s in slots], 3)
    assert all(k > 0 for _, k in grew), "the quantising row producers did not run"
    assert [q for q, _ in grew] == [LEFT[arch] * 2] * 2 and launches()[0] - q0 == 3 * LEFT[arch] * 2, (arch, grew, "stand-alone quantiser launches per pass")
    f64 = F.F64Model(path)
    errs = [_err(lgs[0][s], f64.eval(_tok(m, s, 0), None)[0]) for s in slots]
    print("ROWS-Q", os.path.basename(path), n, f"float64 criterion {max(errs):.3e}")
    assert np.isfinite(lgs[0]).all() and max(errs) <= QUANT_TOL, (n, errs)
    for s in slots:
        st = None
        for p in range(2):
            ref_lg, st = m.eval(_tok(m, s, p), st)
            assert np.array_equal(_bits(lgs[p][s]), _bits(ref_lg)), (n, s, p, "logits")
        tok, want = _tok(m, s, 2), []
        for _ in range(3):
            l2, st = m.eval(tok, st)
            tok = int(np.argmax(l2))
            want.append(tok)
        assert list(toks[s]) == want and np.array_equal(_bits(b.state_store(s)), _bits(st)), (n, s, "decode_greedy")
    b.free()


@pytest.mark.parametrize("name,fmt", [("test-v6", "Q4_0"), ("test-v5.2", "Q5_1")])
def test_ragged_pass_equals_serial_eval(tmp_path, name, fmt):
    """segments of 1, 9 and 3 tokens on slots that hold one evaluated token: the carry from the slot at t0 and the carry inside a segment"""
    m, _, _ = _open(tmp_path, name, fmt, 256)
    b = pkg.RWKVBatch(m, 3)
    for s in range(3):
        b.state_load(s, None)
    b.eval([0, 1, 2], [_tok(m, s, 0) for s in range(3)])
    rows = [[_tok(m, s, 1 + p) for p in range(n)] for s, n in enumerate((1, 9, 3))]
    k0 = launches()[1]
    lg = b.eval_ragged([0, 1, 2], rows)
    assert launches()[1] > k0, "the quantising segment producers did not run"
    for s in range(3):
        ref_lg, ref_st = _alone(m, [_tok(m, s, 0)] + rows[s])
        assert np.array_equal(_bits(lg[s]), _bits(ref_lg)) and np.array_equal(_bits(b.state_store(s)), _bits(ref_st)), s
    b.free()
    m.free()


def test_switch_keeps_the_stand_alone_quantiser(tmp_path):
    """RWKV_MI_ROWS_Q=plain in a fresh process (the switch is read once): the same bits, the new counter stays at zero, every quantised product's
    input goes through the stand-alone quantiser."""
    m, _, arch = _open(tmp_path, "test-v6", "Q5_1", 320)
    b, lgs, _ = _two_passes(m, 17)
    np.save(tmp_path / "y.npy", np.concatenate([lgs[1].ravel(), b.state_store(16)]))
    b.free()
    m.free()
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import test_gpu_rows_q as M; m, _, arch = M._open(%r, 'test-v6', 'Q5_1', 320); "
            "b, lgs, grew = M._two_passes(m, 17); assert grew == [(M.PLAIN_V6 * 2, 0)] * 2, grew; "
            "y = np.concatenate([lgs[1].ravel(), b.state_store(16)]); assert np.array_equal(y.view(np.uint32), np.load(%r).view(np.uint32))"
            % (os.path.dirname(__file__), str(tmp_path), str(tmp_path / "y.npy")))
    subprocess.run([sys.executable, "-c", code], env=dict(os.environ, RWKV_MI_ROWS_Q="plain"), check=True, timeout=300)
