"""The weight quantiser on the device (csrc/quant_w.hip) against the host quantiser (csrc/quantize.cpp), bit for bit: the file
rwkv_mi_quantize_model_file writes is the file rwkv_quantize_model_file writes, and a context of rwkv_mi_init_from_file_as is the context of
that file. Every comparison is bitwise: there is no tolerance."""
import filecmp
import os

import numpy as np
import pytest

import blocks_lib as B
import f64_model as F
import reference_constants as R
import stress_lib as S
from gpu_lib import library, model, synth

pytestmark = pytest.mark.gpu

SOURCES = ("FP32", "FP16")
TINY = ("4v0-660K", "5v2-730K", "7v0-834K")      # the fixtures that exist as FP32 / FP16; RWKV-6 is synth's test-v6
ARCHS = TINY + ("test-v6",)


def palette():
    """The stress blocks, (n, 32) float16 -- every value is exact in binary16, so the FP32 file holds the same numbers."""
    ramp = np.arange(32, dtype=np.float64)
    rows = []
    rows.append(np.zeros(32))                                              # all zeros: d = -0.0, stored 0x8000
    r = ramp / 64; r[3], r[7] = -1.0, 1.0; rows.append(r)                  # |a| twice, the negative first
    r = ramp / 64; r[3], r[7] = 1.0, -1.0; rows.append(r)                  # ... the positive first
    r = ramp / 32; r[31] = -2.0; rows.append(r)                            # the maximum at index 31
    r = -ramp / 32; r[0] = 1.0; rows.append(r)                             # a positive maximum: its code is clamped
    rows.append(np.full(32, 0.75))                                         # constant: d = 0 in Q4_1 / Q5_1
    halves = np.concatenate([np.arange(-7.5, 8.0), np.arange(-7.5, 8.0)])[:30]
    rows.append(np.concatenate([[-8.0, 0.0], halves]))                     # Q4_0: d = 1, x id + 8.5 is an integer
    rows.append(np.concatenate([[-16.0], np.arange(-15.5, 15.5)]))         # Q5_0 likewise
    rows.append(np.concatenate([[0.0, 15.0], np.arange(0.5, 15.0), np.arange(0.5, 15.0)]))   # Q4_1: d = 1, m = 0
    rows.append(np.concatenate([[0.0, 31.0], np.arange(0.5, 30.5)]))       # Q5_1 likewise
    rows.append(np.concatenate([[127.0, -126.5], np.arange(-14.5, 15.5)])) # Q8_0: d = 1, roundf sees ties
    r = ramp * 2.0 ** -20; r[0] = -2.0 ** -14; rows.append(r)              # d = 2^-17: subnormal in binary16
    r = ramp * 1024.0; r[5], r[9] = 65504.0, -65504.0; rows.append(r)      # the largest binary16 magnitude
    p = np.array(rows)
    assert p.shape[1] == 32 and np.isfinite(p).all() and np.array_equal(p.astype(np.float16).astype(np.float64), p)
    return p.astype(np.float16)


def _tile(dims, dtype):
    p = palette()
    n = int(np.prod(dims))
    return np.resize(p.reshape(-1), n).reshape(dims[1], dims[0]).astype(dtype)


@pytest.fixture(scope="module")
def files(tmp_path_factory, golden_dir):
    """source(name, "FP32" | "FP16") and host(name, source, fmt): the source files and, made once each, what the host quantiser writes."""
    tmp = tmp_path_factory.mktemp("quant_device")
    lib = library()
    made = {}

    def source(name, src):
        if name in TINY:
            return R.fixture_path(golden_dir, name, src)
        path = str(tmp / f"{name}-{src}.bin")
        if path not in made:
            synth.write_model(path, synth.CONFIGS["test-v6"], src, seed=5)
            # the stress file: every matrix is the palette, over and over
            B.rewrite_f16_matrices(path, lambda n, dims, w: _tile(dims, np.float16))
            S.rewrite_f32_vectors(path, lambda n, dims, old: _tile(dims, np.float32) if old is not None and len(dims) == 2 else None)
            made[path] = True
        return path

    def host(name, src, fmt):
        path = str(tmp / f"{name}-{src}-{fmt}-host.bin")
        if path not in made:
            lib.rwkv_quantize_model_file(source(name, src), path, fmt)
            if name == "test-v6":   # the host quantiser reads the palette without a non-finite value
                blob = open(path, "rb").read()
                for tname, ty, dims, at, nbytes in B.quantised_tensors(path):
                    q, d, m = F.block_parts(ty, blob[at:at + nbytes], int(np.prod(dims)))
                    assert np.isfinite(d).all() and (m is None or np.isfinite(m).all()), (tname, fmt)
            made[path] = True
        return path

    lib.rwkv_set_print_errors(None, False)
    yield source, host, tmp
    lib.rwkv_set_print_errors(None, True)


@pytest.mark.parametrize("src", SOURCES)
@pytest.mark.parametrize("fmt", R.QUANT_FORMATS)
def test_device_file_is_the_host_file(files, fmt, src):
    source, host, tmp = files
    for name in ARCHS:
        out = str(tmp / "device.bin")
        library().rwkv_mi_quantize_model_file(source(name, src), out, fmt)
        assert filecmp.cmp(out, host(name, src, fmt), shallow=False), (name, src, fmt)


def _run(m):
    """(logits, state) after rwkv_eval of 3 tokens, then after rwkv_eval_sequence of 40, the weight bytes and the decode path"""
    lib = m._library.library
    n_vocab = m.n_vocab
    a = R.PROMPT if n_vocab > max(R.PROMPT) else [1, 2, 3]
    state, logits = None, None
    for t in a:
        logits, state = m.eval(t, state)
    seq_logits, seq_state = m.eval_sequence(S.lcg_tokens(n_vocab, 40), None)
    return (logits.copy(), state.copy(), seq_logits.copy(), seq_state.copy()), int(lib.rwkv_mi_weight_bytes(m._ctx.ptr)), m.decode_path()


def _same_context(monkeypatch, src_path, fmt, host_path):
    # (the decode path as the model's format and geometry decide it, not as a timing of six tokens on a shared device does)
    monkeypatch.setenv("RWKV_MI_NO_AUTOTUNE", "1")
    a = model(src_path, load_as=fmt)
    b = model(host_path)
    try:
        (xa, wa, pa), (xb, wb, pb) = _run(a), _run(b)
    finally:
        a.free()
        b.free()
    assert wa == wb and pa == pb, (wa, wb, pa, pb)
    for got, want, what in zip(xa, xb, ("logits", "state", "sequence logits", "sequence state")):
        assert np.array_equal(got, want), (what, fmt, float(np.abs(got - want).max()))


@pytest.mark.parametrize("name", ARCHS)
@pytest.mark.parametrize("fmt", R.QUANT_FORMATS)
def test_load_as_is_the_load_of_the_host_file(files, monkeypatch, fmt, name):
    source, host, _ = files
    if name == "test-v6":   # (a model to evaluate, not the stress file: its logits must stay finite)
        src = str(files[2] / "v6-FP16.bin")
        hq = str(files[2] / f"v6-FP16-{fmt}.bin")
        if not os.path.exists(src):
            synth.write_model(src, synth.CONFIGS["test-v6"], "FP16", seed=6)
        library().rwkv_quantize_model_file(src, hq, fmt)
        _same_context(monkeypatch, src, fmt, hq)
    else:
        _same_context(monkeypatch, source(name, "FP16"), fmt, host(name, "FP16", fmt))


@pytest.mark.parametrize("fmt", ("Q4_0", "Q5_1"))
def test_tensors_of_more_than_one_piece(files, monkeypatch, fmt):
    """One RWKV-6 layer at D = 2048 in FP32: ffn.key and ffn.value are 56 MiB each -- two pieces of the load pipeline, the second short."""
    tmp = files[2]
    src, hq, dq = str(tmp / "wide-FP32.bin"), str(tmp / f"wide-{fmt}-host.bin"), str(tmp / "wide-device.bin")
    if not os.path.exists(src):
        synth.write_model(src, synth.CONFIGS["mega-v6-2048"], "FP32", seed=7, limit_layers=1)
    lib = library()
    lib.rwkv_quantize_model_file(src, hq, fmt)
    lib.rwkv_mi_quantize_model_file(src, dq, fmt)
    assert filecmp.cmp(dq, hq, shallow=False), fmt
    _same_context(monkeypatch, src, fmt, hq)
