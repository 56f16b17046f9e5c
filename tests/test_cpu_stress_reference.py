"""tests/stress_lib.py does what it claims, and the CPU oracle stays finite and stays the reference on it. CPU-only.

tests/test_gpu_injected_state.py holds every GPU path to the oracle, bit for bit, on stress weights and from injected states; that is worth
what the oracle is worth there. Here the oracle runs 40 tokens from every state family, on the plain and on the stressed copy of the D = 256
file of every architecture, and is held to the float64 pass (tests/f64_model.py) from the same state with the criterion and the gates of
tests/test_cpu_f64_reference.py, unchanged: e = max |oracle - f64| / (1 + max |f64|) on every step's logits and on the final state,
e <= TAU = 1e-4 (FP32), 1e-3 (FP16), QUANT_TOL = 1e-2 (Q5_1).

Every cell met its gate as stress_lib states it: no range had to be narrowed. The figures are in the docstring of
test_oracle_is_finite_and_the_reference_from_every_state.
"""
import os
import shutil

import numpy as np
import pytest

import f64_model as F
import oracle_lib as O
import stress_lib as S
from test_cpu_f64_reference import QUANT_TOL, TOL, _err, synth

SEED = 7
ARCHS = {"test-v4": "4", "test-v5.1": "5.1", "test-v5.2": "5.2", "test-v6": "6", "test-v7": "7"}
FORMATS = ("FP32", "FP16", "Q5_1")
N_TOKENS = 40


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    made = {}
    base = tmp_path_factory.mktemp("stress")

    def get(name, fmt, weights):
        if (name, fmt, "plain") not in made:
            p = str(base / f"{name}-{fmt}-plain.bin")
            synth.write_model(p, synth.CONFIGS[name], fmt, seed=SEED)
            made[(name, fmt, "plain")] = (p, [])
        if (name, fmt, weights) not in made:
            p = str(base / f"{name}-{fmt}-stress.bin")
            shutil.copyfile(made[(name, fmt, "plain")][0], p)
            made[(name, fmt, weights)] = (p, S.rewrite_f32_vectors(p, S.stress_vectors(ARCHS[name], SEED)))
        return made[(name, fmt, weights)]
    yield get
    for p, _ in made.values():
        os.remove(p)


@pytest.fixture(autouse=True, scope="module")
def _oracle_row_kernels():
    O.lib().orc_set_fast(1)     # (the AVX row kernels: bit-identical to the scalar oracle, tests/test_oracle_golden.py)
    yield
    O.lib().orc_set_fast(0)


@pytest.mark.parametrize("fmt", ["FP16", "Q5_1"])
@pytest.mark.parametrize("name", list(ARCHS))
def test_stress_vectors_reach_the_ends(files, name, fmt):
    arch, spec = ARCHS[name], synth.CONFIGS[name]
    plain, _ = files(name, fmt, "plain")
    path, names = files(name, fmt, "stress")
    assert set(names) == S.expected_names(arch, spec.n_layer) and len(names) == len(set(names)), (name, sorted(names))
    _, before = F.read_file(plain)
    _, after = F.read_file(path)
    assert list(before) == list(after)
    for key in before:   # nothing else moved, and every rewritten tensor did
        same = bytes(before[key][2]) == bytes(after[key][2])
        assert same == (key not in names) and before[key][:2] == after[key][:2], key
    vec = lambda key: np.concatenate([np.frombuffer(bytes(after[f"blocks.{i}.att.{key}"][2]), dtype="<f4") for i in range(spec.n_layer)])  # noqa: E731
    if arch == "4":
        w = vec("time_decay")
        print(name, "time_decay", float(w.min()), float(w.max()))
        assert w.min() < -20.0 and w.max() > -1e-3 and (w < 0).all()
        u = vec("time_first")
        assert u.min() < -11.0 and u.max() > 11.0
    elif arch in ("5.1", "5.2", "6"):
        # the per-token factor that reaches the recurrence: the stored value (RWKV-5), f32 exp(-exp(w)) of the rewritten base (RWKV-6)
        w = vec("time_decay")
        if arch == "6":
            with np.errstate(under="ignore"):
                w = np.exp(-np.exp(w.astype(np.float32))).astype(np.float32)
        print(name, "decay", float(w.min()), float(w.max()), int((w == 0).sum()), "zeros")
        assert (w == 0.0).any() and w.max() >= 1.0 - 1e-6 and w.max() <= 1.0 and w.min() >= 0.0
        if arch != "6":
            assert (w == 1.0).any() and (w == np.float32(1e-30)).any()
    else:
        w = vec("w0")
        assert w.min() < -13.0 and w.max() > 7.0
    if arch != "4":
        g = vec("ln_x.weight")
        assert g.min() < -2.9 and g.max() > 2.9


def test_state_families_are_what_they_claim(files):
    for name in ("test-v4", "test-v6"):
        path, _ = files(name, "Q5_1", "stress")
        om = O.OracleModel(path)
        fam = S.state_families(om, SEED)
        again = S.state_families(om, SEED)
        assert all(np.array_equal(fam[k], again[k]) for k in fam)
        assert set(fam) == {"normal", "large", "tiny", "long-run"} | ({"half-fresh", "pp-high"} if name == "test-v4" else set())
        tiny = np.abs(fam["tiny"][fam["tiny"] != 0]) if name != "test-v4" else np.abs(fam["tiny"].reshape(om.n_layer, 5, -1)[:, :4]).reshape(-1)
        assert tiny.max() < np.finfo(np.float32).tiny and (tiny > 0).sum() > tiny.size // 2   # denormals, and not flushed by the cast
        assert 100.0 < np.abs(fam["large"]).max() < 1000.0
        if name == "test-v4":
            v = {k: s.reshape(om.n_layer, 5, om.n_embed) for k, s in fam.items()}
            fresh = om.init_state().reshape(om.n_layer, 5, om.n_embed)
            for k in ("normal", "large", "tiny", "pp-high"):
                assert (v[k][:, 3] > 0).all() and np.abs(v[k][:, 4]).max() <= 80.0
            assert v["pp-high"][:, 4].min() >= 40.0 and (v["normal"][:, 4] < 0).any() and (v["normal"][:, 4] > 0).any()
            assert np.array_equal(v["half-fresh"][:, :, 0::2], fresh[:, :, 0::2]) and np.array_equal(v["half-fresh"][:, :, 1::2], v["normal"][:, :, 1::2])
            assert (fresh[:, 4] == np.float32(-1e30)).all()
        om.free()


@pytest.mark.parametrize("weights", ["plain", "stress"])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", list(ARCHS))
def test_oracle_is_finite_and_the_reference_from_every_state(files, name, fmt, weights):
    """40 tokens from the fresh state and from every family of stress_lib.state_families: logits of every step and the final state finite
    and within the format's gate of the float64 pass run from the same state.

    Measured (seed 7), the worst e over the five architectures and all families (fresh, normal, large, tiny, long-run; half-fresh and
    pp-high on RWKV-4), logits of any step / final state, and the cell it was seen in:
      FP32  plain   6.8e-7 (v5.1 large)     / 1.9e-6 (v4 pp-high)      gate 1e-4
      FP32  stress  8.4e-7 (v5.1 large)     / 1.9e-6 (v4 pp-high)
      FP16  plain   2.8e-4 (v5.1 large)     / 1.1e-4 (v5.2 normal)     gate 1e-3
      FP16  stress  6.3e-4 (v5.1 long-run)  / 1.4e-4 (v5.1 normal)
      Q5_1  plain   4.3e-3 (v7 normal)      / 4.8e-3 (v6 fresh)        gate 1e-2
      Q5_1  stress  6.4e-3 (v7 large)       / 4.9e-3 (v6 fresh)
    The stressed vectors cost the oracle nothing beyond f32 rounding (FP32: 8.4e-7 against 6.8e-7). The FP16 and Q5_1 figures are the
    operand-grid steps tests/test_cpu_f64_reference.py describes, a little larger where ln_x.weight in U(-3, 3) amplifies them. On RWKV-5 / 6 / 7
    the `tiny` family gives the figures of the fresh state: a state of 1e-41 is the zero state to within any rounding here. No cell was
    narrowed.
    """
    tol = TOL.get(fmt, QUANT_TOL)
    path, _ = files(name, fmt, weights)
    om, fm = O.OracleModel(path), F.F64Model(path)
    toks = S.lcg_tokens(om.n_vocab, N_TOKENS, start=S.PROMPT_LEN)
    states = {"fresh": om.init_state(), **S.state_families(om, SEED)}
    errs = {}
    for family, s0 in states.items():
        st, ol = s0.copy(), []
        for t in toks:
            lg, st = om.eval(t, st)
            ol.append(lg)
        ol = np.stack(ol)
        assert np.isfinite(ol).all() and np.isfinite(st).all(), (name, fmt, weights, family)
        fl, fst = fm.forward(toks, s0)
        assert np.isfinite(fl).all() and np.isfinite(fst).all(), (name, fmt, weights, family, "float64")
        errs[family] = (max(_err(ol[i], fl[i]) for i in range(N_TOKENS)), _err(st, fst))
    om.free()
    print("STRESS", name, fmt, weights, " ".join(f"{k} {a:.1e}/{b:.1e}" for k, (a, b) in errs.items()))
    assert all(max(e) <= tol for e in errs.values()), (name, fmt, weights, tol, errs)
