"""The CPU oracle against an independent float64 forward pass (tests/f64_model.py), CPU-only.

test_oracle_golden.py pins the oracle to the reference's recorded logits, but only on tiny fixtures; the RWKV-7 one has a single head, so a
per-head reduction and a whole-vector one give the same logits there. Here the float64 pass is first pinned to the same golden data, then
the oracle is held to it on two-layer slices of the production geometries (40 / 64 / 32 heads of 64), and the float64 pass's known-wrong
RWKV-7 variants show that the comparison tells per-head from whole-vector reductions.

Criterion: e = max |oracle - f64| / (1 + max |f64|), on logits and on the state vector.
  FP32 files  e <= TAU = 1e-4: the oracle differs from float64 by f32 rounding only (measured <= 6.5e-6, mostly <= 1e-6, on every slice).
              A whole-vector reduction in place of a per-head one costs >= 1e-2 (the teeth test below: 107 to 2800 TAU).
  FP16 files  e <= 1e-3, quantised files e <= 1e-2: ggml rounds every matrix operand to fp16 / to 8-bit codes. That rounding is a step
              function of the activation, and the f32 and float64 activations differ by ~1e-7 relative, so some operands land one grid
              step apart; perturbing the float64 pass's activations by 1e-7 moves its logits by 1.4e-4 on an FP16 file. Measured: 1e-4 to
              3.2e-4 (FP16), 1.6e-3 to 4.9e-3 (quantised). These checks catch gross format errors; per-head reductions are pinned by FP32.
"""
import dataclasses
import os

import numpy as np
import pytest

import f64_model as F
import oracle_lib as O
import reference_constants as R
import __graft_entry__ as graft  # (tests/conftest.py puts the repository root on sys.path)

graft.load_package()
from rwkv_cpp_amd import synth  # noqa: E402

TAU = 1e-4
TOL = {"FP32": TAU, "FP16": 1e-3}
QUANT_TOL = 1e-2


def _err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / (1.0 + np.abs(want).max()))


# ---------------------------------------------------------------------------------------------------------------------------------------
# self-pin: the float64 pass's own reader and dequantiser, and the golden data
# ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["FP16", "Q4_0", "Q4_1", "Q5_0", "Q5_1", "Q8_0"])
def test_dequantiser_matches_the_oracle_byte_for_byte(fmt):
    rng = np.random.default_rng(3)
    t = O.TYPE_IDS[fmt]
    x = np.concatenate([rng.standard_normal(32 * 40).astype(np.float32) * s for s in (1e-3, 1.0, 50.0)])
    x[:32] = 0.0                                                   # an all-zero block (d = 0)
    x[32:64] = np.linspace(-1, 1, 32, dtype=np.float32)
    raw = O.quantize_row(t, x)
    got = F.dequantize(t, raw.tobytes(), x.size).astype(np.float32)
    want = O.dequantize_row(t, raw, x.size)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), fmt


def test_reader_sees_the_oracle_geometry(golden_dir):
    for version in R.VERSIONS:
        for fmt in ("FP32", "Q5_1"):
            p = R.fixture_path(golden_dir, version, fmt)
            if not os.path.exists(p):
                continue
            m, om = F.F64Model(p), O.OracleModel(p)
            assert (m.arch, m.n_vocab, m.n_embed, m.n_layer, m.head_count, m.head_size, m.state_len) == \
                   ((om.arch_major, om.arch_minor), om.n_vocab, om.n_embed, om.n_layer, om.head_count, om.head_size, om.state_len), p
            assert np.array_equal(m.init_state(), om.init_state().astype(np.float64))
            om.free()


def _golden_diff(path, golden_dir, version, wrong=None):
    exp = R.expected_logits(golden_dir, version).astype(np.float64)
    lg, _ = F.F64Model(path, wrong=wrong).eval_sequence(R.PROMPT, None)
    d = lg - exp
    return float(d.sum()), float(np.abs(d).max())


@pytest.mark.parametrize("version", R.HAVE_FP32_FP16)
def test_f64_meets_the_fp32_golden_bounds(golden_dir, version):
    # the bounds the oracle meets (test_oracle_golden.py): |sum| <= 1.05e-3 and max-abs <= 1e-5; measured max-abs of the float64 pass:
    # 1.5e-6 (4v0), 1.6e-6 (5v1), 3.1e-6 (5v2), 3.7e-7 (7v0) -- the recorded logits are f32 results of ggml's f32 arithmetic
    s, mx = _golden_diff(R.fixture_path(golden_dir, version, "FP32"), golden_dir, version)
    print(f"{version} FP32: sum {s:+.3e} max {mx:.3e}")
    assert abs(s) <= 0.001 * R.TOLERANCE_FACTOR
    assert mx <= 1e-5


# Two fixtures sit on an operand-rounding boundary: the float64 pass puts one activation on the other side of a rounding step of ggml's
# operand grid than ggml's f32 arithmetic did (5v1 FP16: an activation 7.6e-6 of an fp16 ulp from a rounding midpoint; 5v2 Q5_0: an
# activation 1.8e-7 of a Q8 step from one), and the recorded sum of the reference, which is the sum over 65536 logits of a tiny model, moves
# past its 5 % margin (-0.332 vs -0.290; 27.6 vs 25.3). Every other FP16 / Q5 fixture meets its recorded threshold.
ON_A_BOUNDARY = {("5v1-730K", "FP16"), ("5v2-730K", "Q5_0")}
GOLDEN_OTHER = [(v, "FP16", abs(R.FULL[v]["FP16"])) for v in R.HAVE_FP32_FP16] + \
               [(v, f, abs(R.SHIPPED_Q5[v][f])) for v in R.SHIPPED_Q5 for f in ("Q5_0", "Q5_1")] + \
               [("7v0-834K", f, abs(R.FROM_FP32["7v0-834K"][R.QUANT_FORMATS.index(f)])) for f in ("Q5_0", "Q5_1")]


@pytest.mark.parametrize("version,fmt,recorded", GOLDEN_OTHER)
def test_f64_meets_the_recorded_thresholds(golden_dir, version, fmt, recorded):
    s, mx = _golden_diff(R.fixture_path(golden_dir, version, fmt), golden_dir, version)
    print(f"{version} {fmt}: sum {s:+.4f} recorded {recorded:.4f} max {mx:.3e}")
    if (version, fmt) in ON_A_BOUNDARY:
        # the sum is off by the one operand step, not by a wrong reading of the model: it stays within 1.5x the recorded sum
        assert abs(s) <= 1.5 * recorded
    else:
        assert abs(s) <= recorded * R.TOLERANCE_FACTOR


def test_wrong_variants_still_pass_the_single_head_golden_fixture(golden_dir):
    """The gap this file closes: on 7v0 (one head of 64) every whole-vector variant meets the golden bounds the correct pass meets."""
    for wrong in F.WRONG_VARIANTS:
        s, mx = _golden_diff(R.fixture_path(golden_dir, "7v0-834K", "FP32"), golden_dir, "7v0-834K", wrong=wrong)
        assert abs(s) <= 0.001 * R.TOLERANCE_FACTOR and mx <= 1e-5, (wrong, s, mx)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the oracle at production geometry
# ---------------------------------------------------------------------------------------------------------------------------------------

def _spec(name):
    if name == "v5.1-2048":
        return dataclasses.replace(synth.CONFIGS["test-v5.1"], n_embed=2048, ffn=7168, n_vocab=4096, name=name)
    if name == "v5.2-2048":
        return dataclasses.replace(synth.CONFIGS["test-v5.2"], n_embed=2048, ffn=7168, n_vocab=4096, name=name)
    return dataclasses.replace(synth.CONFIGS[name], n_layer=2)


QUANT_OF = {"slice-v7-2560": "Q5_1", "mega-v6-4096": "Q4_0", "v5.1-2048": "Q5_0", "v5.2-2048": "Q8_0", "slice-v4-768": "Q4_1"}
SLICES = list(QUANT_OF)
TOKENS = [int((1103515245 * i + 12345) % 512) for i in range(80)]   # (every slice has >= 512 tokens)


@pytest.fixture(scope="module")
def slice_file(tmp_path_factory):
    made = {}

    def get(name, fmt):
        if (name, fmt) not in made:
            p = str(tmp_path_factory.getbasetemp() / f"{name}-{fmt}.bin")
            synth.write_model(p, _spec(name), fmt, seed=11)
            made[(name, fmt)] = p
        return made[(name, fmt)]
    yield get
    for p in made.values():
        os.remove(p)


@pytest.fixture(autouse=True, scope="module")
def _oracle_row_kernels():
    O.lib().orc_set_fast(1)     # (the AVX row kernels: bit-identical to the scalar oracle, tests/test_oracle_golden.py)
    yield
    O.lib().orc_set_fast(0)


@pytest.mark.parametrize("fmt", ["FP32", "FP16", "quant"])
@pytest.mark.parametrize("name", SLICES)
def test_oracle_against_float64_at_production_geometry(slice_file, name, fmt):
    fmt = QUANT_OF[name] if fmt == "quant" else fmt
    tol = TOL.get(fmt, QUANT_TOL)
    p = slice_file(name, fmt)
    om, fm = O.OracleModel(p), F.F64Model(p)
    assert fm.head_count == om.head_count and (fm.head_count == 0 or fm.head_size == 64)
    errs = {}
    # 16 serial tokens from the initial state: every step's logits, and the state
    st, ol = om.init_state(), []
    for t in TOKENS[:16]:
        lg, st = om.eval(t, st)
        ol.append(lg)
    fl, fst = fm.forward(TOKENS[:16], None)
    errs["serial logits"] = max(_err(ol[i], fl[i]) for i in range(16))
    errs["serial state"] = _err(st, fst)
    # one 64-token sequence from the initial state and one from the state the serial run left (oracle's f32 state, fed to both)
    for label, s0 in (("init", None), ("warm", st)):
        lg, so = om.eval_sequence(TOKENS[16:80], om.init_state() if s0 is None else s0)
        flg, fso = fm.eval_sequence(TOKENS[16:80], s0)
        errs[f"seq/{label} logits"], errs[f"seq/{label} state"] = _err(lg, flg), _err(so, fso)
    om.free()
    print(name, fmt, " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v <= tol for v in errs.values()), (name, fmt, tol, errs)


@pytest.mark.parametrize("wrong", F.WRONG_VARIANTS)
def test_wrong_variants_are_rejected_at_forty_heads(slice_file, wrong):
    """The same comparison with a whole-vector reduction in the float64 pass: the oracle (per head) misses it by >= 100 TAU."""
    p = slice_file("slice-v7-2560", "FP32")
    om, fm = O.OracleModel(p), F.F64Model(p, wrong=wrong)
    st, ol = om.init_state(), []
    for t in TOKENS[:16]:
        lg, st = om.eval(t, st)
        ol.append(lg)
    fl, fst = fm.forward(TOKENS[:16], None)
    e_logits, e_state = max(_err(ol[i], fl[i]) for i in range(16)), _err(st, fst)
    om.free()
    print(wrong, f"logits {e_logits:.2e} state {e_state:.2e} ({e_logits / TAU:.0f} / {e_state / TAU:.0f} TAU)")
    assert e_logits >= 100 * TAU and e_state >= 100 * TAU, (wrong, e_logits, e_state)
