"""The arms that are not bit-identical to anything, held to the float64 forward pass (tests/f64_model.py), and the argmax tie rule.

  fast sequence arms   k_mmq_fast (RWKV_MI_SEQ_Q=fast / force) and k_mmf16_seq (RWKV_MI_SEQ_F16=mfma) on one- and two-layer slices of the
                       BASELINE geometries: e_x = max |x - f64| / (1 + max |f64|); e_fast <= C e_oracle + 1e-6 with C = 8 on logits and state.
                       The fast arm may add its f32 terms in another order, not be much worse than f32 arithmetic in ggml's order. (The
                       conftest's model-level gate, 1e-2 (1 + max |oracle|), is far looser.)
  sampler              at the shipped vocabularies (50277, 65536) against the float64 distribution of the context's own logits.
  ties                 three bit-identical head rows carry the largest logit: every greedy path returns the smallest index.
"""
import ctypes
import dataclasses
import os

import numpy as np
import pytest

import f64_model as F
import oracle_lib as O
from gpu_lib import hooks_library, library, model, pkg, synth
from test_gpu_sampling import ref_distribution

pytestmark = pytest.mark.gpu

C_FAST = 8.0


def _err(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / (1.0 + np.abs(want).max()))


def _counter(name):
    f = getattr(hooks_library().library, name)
    f.restype = ctypes.c_uint64
    return int(f())


@pytest.fixture(autouse=True)
def _env():
    keep = {k: os.environ.get(k) for k in ("RWKV_MI_SEQ_Q", "RWKV_MI_SEQ_F16", "RWKV_MI_NO_AUTOTUNE", "RWKV_MI_NO_MEGA", "RWKV_MI_NO_FUSED", "RWKV_MI_PERSIST")}
    O.lib().orc_set_fast(1)
    yield
    O.lib().orc_set_fast(0)
    for k, v in keep.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


# (config, format, layers, T, sequence arm setting, F16 arm setting, launch counter that proves the arm ran)
FAST_CASES = [("rwkv6-1b6", "Q4_0", 1, 130, "force", "valu", "rwkv_mi_test_mmq_fast_launches"),
              ("rwkv6-1b6", "Q5_1", 2, 97, "force", "valu", "rwkv_mi_test_mmq_fast_launches"),
              ("rwkv7-2b9", "Q5_1", 1, 97, "force", "valu", "rwkv_mi_test_mmq_fast_launches"),
              ("rwkv7-2b9", "FP16", 2, 130, "exact", "mfma", "rwkv_mi_test_mmf16_launches"),
              ("rwkv4-169m", "Q5_0", 2, 130, "force", "valu", "rwkv_mi_test_mmq_fast_launches")]


@pytest.mark.parametrize("name,fmt,layers,T,seq_q,seq_f16,counter", FAST_CASES)
def test_fast_sequence_arms_against_float64(tmp_path, name, fmt, layers, T, seq_q, seq_f16, counter):
    p = str(tmp_path / "m.bin")
    spec = dataclasses.replace(synth.CONFIGS[name], n_vocab=4096)
    synth.write_model(p, spec, fmt, seed=67, limit_layers=layers)
    toks = [int((1103515245 * i + 12345) % spec.n_vocab) for i in range(T)]
    fl, fs = F.F64Model(p).eval_sequence(toks, None)
    om = O.OracleModel(p)
    ol, ost = om.eval_sequence(toks, om.init_state())
    om.free()
    os.environ["RWKV_MI_SEQ_Q"], os.environ["RWKV_MI_SEQ_F16"] = seq_q, seq_f16
    m = model(p, hooks=True)
    before = _counter(counter)
    gl, gs = m.eval_sequence(toks, None)
    assert _counter(counter) > before, f"{counter}: the fast arm did not run"
    cl, cs = m.eval_sequence_in_chunks(toks, None, chunk_size=max(64, 3 * T // 5))
    m.free()
    for what, fast, orc, ref in (("logits", gl, ol, fl), ("state", gs, ost, fs), ("chunked logits", cl, ol, fl), ("chunked state", cs, ost, fs)):
        e_fast, e_orc = _err(fast, ref), _err(orc, ref)
        print(f"{name} {fmt} L{layers} T{T} {what}: e_oracle {e_orc:.2e} e_fast {e_fast:.2e} ratio {e_fast / max(e_orc, 1e-30):.2f}")
        assert np.isfinite(fast).all() and e_fast <= C_FAST * e_orc + 1e-6, (name, fmt, what, e_fast, e_orc)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the sampler at the shipped vocabularies
# ---------------------------------------------------------------------------------------------------------------------------------------

SAMPLE_GRID = [(1.0, 0.8), (0.7, 0.5), (1.5, 1.0), (1.0, 0.0), (0.0, 0.8), (0.3, 0.95),
               (0.05, 0.8), (5.0, 1.0), (1.0, 1e-6), (1.0, 0.999999)]


def _slack(V):
    """sampling.hip gives each of 1024 threads a contiguous chunk of ceil(V / 1024) logits. A token's cumulative probability is then a
    chain of <= ceil(V / 1024) f32 additions inside the thread, plus an inclusive scan over the 1024 thread sums (log2 1024 = 10 levels,
    each adding one rounding to the running sum and one to the partial it adds), plus the normalisation, the temperature power and the
    comparison with u (<= 4 more roundings). Every rounding is at most 2^-24 of the total mass, which is 1 after normalisation."""
    return (-(-V // 1024) + 2 * 10 + 4) * 2.0 ** -24


@pytest.fixture(scope="module", params=["slice-v4-768", "mega-v6-2048-v64k"])
def vocab_ctx(request, tmp_path_factory):
    library()
    p = str(tmp_path_factory.mktemp("v") / "m.bin")
    synth.write_model(p, synth.CONFIGS[request.param], "Q8_0", seed=5, limit_layers=1)
    m = model(p)
    yield m
    m.free()


@pytest.mark.parametrize("temperature,top_p", SAMPLE_GRID)
def test_sampler_at_real_vocabularies(vocab_ctx, temperature, top_p):
    m = vocab_ctx
    logits, _ = m.eval(7, None)
    V = logits.size
    assert V in (50277, 65536)
    pr = ref_distribution(logits, temperature, top_p)
    cdf = np.cumsum(pr)
    slack = _slack(V)
    for u in np.linspace(0.001, 0.999, 41):
        tok = m.sample(temperature, top_p, u=float(u))
        lo, hi = cdf[tok] - pr[tok], cdf[tok]
        assert pr[tok] > 0.0, (temperature, top_p, u, tok)
        assert lo - slack <= u <= hi + slack, (V, temperature, top_p, float(u), tok, lo, hi, slack)


# ---------------------------------------------------------------------------------------------------------------------------------------
# argmax ties: greater value, then smaller index
# ---------------------------------------------------------------------------------------------------------------------------------------

def _make_tie(path, rows):
    """Rewrites head.weight and ln_out in place: ln_out.weight small, ln_out.bias a fixed +-0.5 pattern, and the given head rows all equal
    to (160 / D) x the bias (bit-identical rows): their logit is ~40, every other row's ~1, for every input."""
    _, t = F.read_file(path)
    D = len(t["ln_out.bias"][2]) // 4
    bias = np.where(np.arange(D) % 3 == 0, -0.5, 0.5).astype(np.float32)
    ty_h = t["head.weight"][0]
    row = ((160.0 / D) * bias).astype(np.float32 if ty_h == F.F32 else np.float16)   # tied logit ~40: the three rows hold all the mass
    offsets = {}
    with open(path, "rb") as f:
        blob = f.read()
    for name in ("ln_out.weight", "ln_out.bias", "head.weight"):
        mv = t[name][2]
        offsets[name] = blob.find(bytes(mv[:64]))
        assert offsets[name] > 0 and blob[offsets[name]:offsets[name] + len(mv)] == bytes(mv), name
    with open(path, "r+b") as f:
        f.seek(offsets["ln_out.weight"])
        f.write(np.full(D, 0.01, np.float32).tobytes())
        f.seek(offsets["ln_out.bias"])
        f.write(bias.tobytes())
        for r in rows:
            f.seek(offsets["head.weight"] + r * D * row.itemsize)
            f.write(row.tobytes())


TIE_CASES = [("mega-v6-2048-v64k", "Q4_0", (5, 4097, 65530), 2),
             ("slice-v7-2560", "Q5_1", (70, 1100, 4000), 3),
             ("slice-v4-768", "Q5_1", (3, 777, 50270), 3)]


@pytest.mark.parametrize("name,fmt,rows,kind", TIE_CASES)
def test_every_greedy_path_breaks_ties_to_the_smallest_index(tmp_path, name, fmt, rows, kind):
    library()
    p = str(tmp_path / "m.bin")
    synth.write_model(p, synth.CONFIGS[name], fmt, seed=13)
    _make_tie(p, rows)
    want = min(rows)
    om = O.OracleModel(p)
    st = om.init_state()
    for t in (5, 9, 300):
        ol, st = om.eval(t, st)
        top = np.flatnonzero(ol == ol.max())
        assert sorted(top) == sorted(rows) and int(np.argmax(ol)) == want, (name, top)
    om.free()

    def greedy(m):
        m.state_load(None)
        toks, _ = m.decode_greedy(5, 4)
        return list(toks)

    os.environ["RWKV_MI_NO_AUTOTUNE"] = "1"
    if kind == 2:
        os.environ["RWKV_MI_PERSIST"] = "ring"
    os.environ["RWKV_MI_NO_FUSED"] = "1"
    per_op = model(p)
    assert greedy(per_op) == [want] * 4, "per-op"
    per_op.free()
    del os.environ["RWKV_MI_NO_FUSED"]
    os.environ["RWKV_MI_NO_MEGA"] = "1"
    fused = model(p)
    assert fused.decode_path() == 1 and greedy(fused) == [want] * 4, "fused"
    fused.free()
    del os.environ["RWKV_MI_NO_MEGA"]
    m = model(p)
    assert m.decode_path() == 2 and m.persist_kind() == kind, (m.decode_path(), m.persist_kind())
    assert greedy(m) == [want] * 4, "persistent"
    m.state_load(None)
    z, _ = m.decode_sample(5, 4, temperature=0.0, top_p=0.9, seed=1)
    assert list(z) == [want] * 4, "decode_sample(temperature=0)"
    # sample(): temperature 0 is the argmax; a top_p whose cut-off falls on the tied probabilities keeps exactly the three rows
    m.state_load(None)
    m.eval(5, None)
    assert m.sample(0.0, 0.8, u=0.5) == want
    got = {m.sample(1.0, 0.5, u=float(u)) for u in np.linspace(0.001, 0.999, 41)}
    assert got == set(rows), got
    for n in (4, 33):
        b = pkg.RWKVBatch(m, n)
        for s in range(n):
            b.state_load(s, None)
        toks, _ = b.decode_greedy(list(range(n)), [5 + 11 * s for s in range(n)], 3)
        b.free()
        assert np.all(toks == want), ("batch", n, toks)
    m.free()
