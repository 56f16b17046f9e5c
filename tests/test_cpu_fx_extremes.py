"""tests/fx_lib.py does what it claims, and the CPU oracle is the reference for the F16 / F32 products on it. CPU-only.

tests/test_gpu_fx_extremes.py holds k_mvf and k_mmfx_seq to the oracle bit for bit (NaN by position) on hand-built operands: binary16
subnormal weights, f32 denormals, products that underflow to a signed zero, infinities, every edge of the binary16 rounding of the
activations. That is worth what the oracle is worth there, so here

  * an emulation that shares nothing with oracle/ -- one fma32 built from fractions.Fraction with a single round-to-nearest-even into
    binary32 (subnormals, overflow, signed zeros, inf and NaN), the 32 chains k % 32 and the fold 16 / 8 / 4 / (0 + 1) + (2 + 3), the
    activations through NumPy's float16 under F16 weights -- must give the oracle's bits on every weight row x every activation row of both
    types at K = 160;
  * orc_f32_to_f16 must be NumPy's float16 cast on every activation element;
  * the AVX row kernels must be the scalar oracle in bits at every shape the GPU file uses;
  * the oracle's outputs are non-finite ONLY where the weight row or the activation row is a declared non-finite family (fx_lib), and finite
    everywhere else: that is what keeps "NaN by position" from hiding anything;
  * every finite F16 output lies within the project's bound 2e-6 sum |w fp16(x)| + 1e-30 of the float64 sum (tests/test_gpu_seq_f16.py).
The measured figures are in the docstrings of the tests.
"""
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import blocks_lib as B
import fx_lib as X
import oracle_lib as O
from test_cpu_f64_reference import synth

SEED = 7
TYPES = ["FP16", "FP32"]
KS = [32, 128, 160, 2112]           # the row lengths of tests/test_gpu_fx_extremes.py

_TWO128 = Fraction(2) ** 128


def _round32(v):
    """A non-zero Fraction to the nearest binary32 (ties to even; subnormals: quantum 2^-149; |v| rounding to 2^128: inf), as a float."""
    neg, m = v < 0, abs(v)
    e = m.numerator.bit_length() - m.denominator.bit_length()       # 2^(e-1) < m < 2^(e+1)
    if m < Fraction(2) ** e:
        e -= 1
    quantum = Fraction(2) ** (max(e, -126) - 23)
    q = m / quantum
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    r = n * quantum
    out = math.inf if r >= _TWO128 else float(r)                     # (exact: at most 24 bits, exponent within double's)
    return -out if neg else out


def fma32(a, b, c):
    """round32(a b + c) of three binary32 values held in Python floats: ONE rounding, IEEE 754 fusedMultiplyAdd."""
    if math.isnan(a) or math.isnan(b) or math.isnan(c):
        return math.nan
    psign = (math.copysign(1.0, a) < 0) != (math.copysign(1.0, b) < 0)
    if math.isinf(a) or math.isinf(b):
        if a == 0 or b == 0 or (math.isinf(c) and (c < 0) != psign):
            return math.nan
        return -math.inf if psign else math.inf
    if math.isinf(c):
        return c
    v = Fraction(a) * Fraction(b) + Fraction(c)
    if v == 0:      # an exact zero sum is +0 unless both addends are -0 (a zero product has the sign of its factors)
        return -0.0 if (a == 0 or b == 0) and c == 0 and psign and math.copysign(1.0, c) < 0 else 0.0
    return _round32(v)


def add32(a, b):
    return fma32(a, 1.0, b)


def emulate_row(w, x):
    """One output in ggml's order: chain p = fma32(w[k], x[k], .) over k = p, p + 32, ...; then the fold."""
    ps = [0.0] * 32
    for k in range(len(w)):
        ps[k & 31] = fma32(w[k], x[k], ps[k & 31])
    for width in (16, 8, 4):
        for i in range(width):
            ps[i] = add32(ps[i], ps[i + width])
    return add32(add32(ps[0], ps[1]), add32(ps[2], ps[3]))


def test_fma32_is_a_single_rounding():
    f = np.float32
    assert fma32(1.0, 1.0, 1.0) == 2.0
    assert fma32(float(f(1) + f(2.0 ** -23)), float(f(1) - f(2.0 ** -24)), -1.0) == 2.0 ** -23 - 2.0 ** -24 - 2.0 ** -47      # exact: the product keeps all its bits
    assert fma32(float(f(1e-30)), float(f(-1e-30)), 0.0) == 0.0 and math.copysign(1.0, fma32(float(f(1e-30)), float(f(-1e-30)), 0.0)) < 0   # underflow keeps the sign
    assert math.copysign(1.0, fma32(0.0, 0.0, -0.0)) > 0 and math.copysign(1.0, fma32(0.0, -0.0, -0.0)) < 0 and math.copysign(1.0, fma32(0.0, -0.0, 0.0)) > 0
    assert math.copysign(1.0, fma32(1.0, 1.0, -1.0)) > 0
    assert fma32(2.0 ** -149, 0.5, 0.0) == 0.0 and fma32(2.0 ** -149, 0.75, 0.0) == 2.0 ** -149 and fma32(3 * 2.0 ** -149, 0.5, 0.0) == 2 * 2.0 ** -149   # ties to even below the smallest denormal
    big = float(np.finfo(f).max)
    assert fma32(big, 1.0, 2.0 ** 102) == big and fma32(big, 1.0, 2.0 ** 103) == math.inf and fma32(big, 2.0, -big) == big    # overflow is judged after the one rounding
    assert math.isnan(fma32(math.inf, 0.0, 1.0)) and math.isnan(fma32(math.inf, 1.0, -math.inf)) and fma32(-math.inf, 2.0, 5.0) == -math.inf
    rng = np.random.default_rng(3)
    a, b, c = (rng.standard_normal(2000).astype(f) * f(10.0) ** rng.integers(-12, 12, 2000).astype(f) for _ in range(3))
    want = (a.astype(np.float64) * b.astype(np.float64)).astype(f)      # a product of two binary32 is exact in binary64: one rounding
    assert all(fma32(float(p), float(q), 0.0) == float(r) for p, q, r in zip(a, b, want))
    s = (a.astype(np.float64) + c.astype(np.float64)).astype(f)         # the sum of two binary32 rounded twice is the sum rounded once (Figueroa)
    assert all(add32(float(p), float(q)) == float(r) for p, q, r in zip(a, c, s))


def _same_bits(a, b):
    """isnan positions equal, bit patterns equal everywhere else."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return ~((np.isnan(a) & np.isnan(b)) | (~np.isnan(a) & ~np.isnan(b) & (a.view(np.uint32) == b.view(np.uint32))))


def _payload(w):
    return np.ascontiguousarray(w).view(np.uint8).reshape(-1)


def test_families_are_what_they_claim():
    for K in KS:
        for t in (X.F16, X.F32):
            w, names = X.weight_rows(t, K, SEED)
            row = {n: w[i].astype(np.float64) for i, n in enumerate(names)}
            assert len(set(names)) == len(names) == w.shape[0] == len(X.families(t)) + X.N_MIXED and w.dtype == X.DTYPE[t]
            assert np.isfinite(w).all()
            assert not row["zeros"].any() and not np.signbit(row["zeros"]).any() and np.signbit(row["negzero"]).all() and not row["negzero"].any()
            assert (row["+sub"] == 2.0 ** -24).all() and (row["maxsub"] == 1023 * 2.0 ** -24).all() and (row["minnorm"] == 2.0 ** -14).all()
            sr = row["subrand"] * 2.0 ** 24
            assert (sr == np.round(sr)).all() and (np.abs(sr) >= 1).all() and (np.abs(sr) <= 1023).all() and (sr < 0).any() and (sr > 0).any()
            assert (np.abs(row["altmax"]) == 65504).all() and row["altmax"][0] == -row["altmax"][1]
            assert (row["alt32max"][:32] == 65504).all() and (K == 32 or (row["alt32max"][32:64] == -65504).all())
            assert row["ramp"].min() == 2.0 ** -24 and row["ramp"].max() == 2.0 ** 5
            lb = (row["lowbits"] - 1) * 1024
            assert (lb == np.round(lb)).all() and lb.max() < 1024 and len(np.unique(lb)) >= min(K, 1024) // 2
            assert (row["spike"] != 0).sum() == 1 and row["spike"][(7 * names.index("spike")) % K] != 0
            if t == X.F32:
                tiny = float(np.finfo(np.float32).tiny)
                assert row["denorm"].any() and np.abs(row["denorm"]).max() < tiny
                assert float(np.float32(1e-30)) * float(np.float32(1e-30)) < 2.0 ** -150        # the product of tiny and negtiny underflows to a zero
                assert (w[names.index("allbits")].view(np.uint32) & 0x7FFFFF == 0x7FFFFF).all() and (row["huge"] > 2.9e38).all()
        x, an = X.activation_rows(K, SEED)
        a = {n: x[i] for i, n in enumerate(an)}
        assert len(set(an)) == len(an) and x.dtype == np.float32
        assert set(X.NONFINITE_ACTS[X.F32]) <= set(an) and set(X.NONFINITE_ACTS[X.F16]) <= set(an)
        h = X.round_trip_f16(x)
        h = {n: h[i] for i, n in enumerate(an)}
        assert np.signbit(a["negzero"][:32]).all() and not a["negzero"][:32].any()
        assert set(np.unique(np.abs(h["n6e-8"]))) >= {0.0, 2.0 ** -24} and h["n6e-8"][9] == 0 and a["n6e-8"][9] == 2.0 ** -25   # the tie at 2^-25 goes to even: 0
        assert np.array_equal(h["ties"][:4], np.array([1, 1, 1 + 2.0 ** -10, 1 + 2.0 ** -9], dtype=np.float32)) and (a["ties"][:4] != h["ties"][:4]).sum() == 2
        assert (np.abs(h["r65519"]) == 65504).all() and np.isinf(h["r65520"]).all() and (h["max"] == 65504).all() and np.isinf(h["big"]).all()
        assert ((h["n1e-3"] != 0) & (np.abs(h["n1e-3"]) < 2.0 ** -14)).any()
        assert a["denorm"].any() and np.abs(a["denorm"]).max() < np.finfo(np.float32).tiny and not h["denorm"].any()
        assert np.signbit(h["negtiny"]).all() and not h["negtiny"].any()
        assert np.isinf(a["inf"]).all() and np.isnan(a["nan"]).sum() == K // 32
        finite = [n for n in an if n not in ("inf", "nan")]
        assert all(np.isfinite(a[n]).all() for n in finite)
    for T in (1, 3, 31, 32, 65):
        ops = X.token_operands(32, T, SEED)
        rows, names = X.activation_rows(32, SEED)
        for pos in {0, 31, 32, T - 1}:
            if pos < T:
                assert sorted(int(fam[pos]) for _, fam in ops) == list(range(len(names))), (T, pos)
        for x, fam in ops:
            assert np.array_equal(x.view(np.uint32), rows[fam].view(np.uint32))


def test_oracle_conversion_is_numpys_float16():
    L = O.lib()
    for K in KS:
        x, names = X.activation_rows(K, SEED)
        with np.errstate(over="ignore"):
            want = x.astype(np.float16)
        for i, n in enumerate(names):
            got = np.array([L.orc_f32_to_f16(float(v)) for v in x[i]], dtype=np.uint16)
            w16 = want[i].view(np.uint16)
            nan = np.isnan(x[i])
            assert np.array_equal(got[~nan], w16[~nan]), (K, n)
            assert ((got[nan] & 0x7C00) == 0x7C00).all() and (got[nan] & 0x3FF).all(), (K, n)          # a NaN stays a NaN
            back = np.array([L.orc_f16_to_f32(int(v)) for v in got[~nan]], dtype=np.float32)
            assert np.array_equal(back.view(np.uint32), want[i][~nan].astype(np.float32).view(np.uint32)), (K, n)


@pytest.mark.parametrize("fmt", TYPES)
def test_oracle_is_the_exact_emulation(fmt):
    """K = 160 (five links per chain, the tail of a 128-element step), every weight row x every activation row: the oracle's bits are those
    of the Fraction emulation, NaN by position. The predicted signed zero is among them: tiny x negtiny is 0x80000000."""
    t, K = X.TYPE_NAMES[fmt], 160
    w, wn = X.weight_rows(t, K, SEED)
    x, an = X.activation_rows(K, SEED)
    O.lib().orc_set_fast(0)
    y = O.mul_mat(t, _payload(w), K, w.shape[0], x)
    xs = X.round_trip_f16(x) if t == X.F16 else x
    wl, xl = [[float(v) for v in r] for r in w.astype(np.float64)], [[float(v) for v in r] for r in xs.astype(np.float64)]
    emu = np.array([[emulate_row(wr, xr) for wr in wl] for xr in xl], dtype=np.float64).astype(np.float32)
    bad = _same_bits(y, emu)
    assert not bad.any(), (fmt, [(an[i], wn[j], float(y[i, j]), float(emu[i, j])) for i, j in zip(*np.nonzero(bad))][:8])
    if t == X.F32:
        assert y[an.index("negtiny"), wn.index("tiny")].view(np.uint32) == 0x80000000
        assert y[an.index("negtiny"), wn.index("negtiny")].view(np.uint32) == 0x00000000


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("fmt", TYPES)
def test_oracle_on_hand_built_operands(fmt, K):
    """Every weight row x every activation row at every K of the GPU file: the AVX row kernels are the scalar oracle in bits (NaN by
    position); an output is non-finite only where its weight row or its activation row is a declared non-finite family, and finite
    everywhere else; every finite F16 output is within 2e-6 sum |w fp16(x)| + 1e-30 of the float64 sum.

    Measured (seed 7), the largest |oracle - f64| / bound over the finite F16 outputs at K = 32 / 128 / 160 / 2112:
      0.061 (max x ramp) / 0.026 (spike x altmax) / 0.032 (ties x ramp) / 0.242 (ties x maxsub); 84 of the 336 outputs are non-finite,
      all in declared families. For F32 weights the same figure against sum |w x| is printed and not asserted (no bound is claimed for
      them; the emulation above is exact): 0.065 / 0.029 / 0.043 / 0.320 (big x maxsub), 60 - 61 of 416 outputs non-finite.
    """
    t = X.TYPE_NAMES[fmt]
    w, wn = X.weight_rows(t, K, SEED)
    x, an = X.activation_rows(K, SEED)
    O.lib().orc_set_fast(0)
    y = O.mul_mat(t, _payload(w), K, w.shape[0], x)
    O.lib().orc_set_fast(1)
    try:
        y_fast = O.mul_mat(t, _payload(w), K, w.shape[0], x)
    finally:
        O.lib().orc_set_fast(0)
    bad = _same_bits(y, y_fast)
    assert not bad.any(), (fmt, K, "scalar oracle != AVX rows", [(an[i], wn[j], float(y[i, j]), float(y_fast[i, j])) for i, j in zip(*np.nonzero(bad))][:8])
    declared = np.array([n in X.NONFINITE_ACTS[t] for n in an])[:, None] | np.array([n in X.NONFINITE_WEIGHTS for n in wn])[None, :]
    stray = ~np.isfinite(y) & ~declared
    assert not stray.any(), (fmt, K, "non-finite outside the declared families", [(an[i], wn[j], float(y[i, j])) for i, j in zip(*np.nonzero(stray))][:8])
    ref, A = X.float64_sum(t, w, x)
    held = np.isfinite(y) & np.isfinite(A)
    assert held[~declared].all()
    bound = 2e-6 * A + 1e-30
    with np.errstate(all="ignore"):
        ratio = np.where(held, np.abs(y.astype(np.float64) - ref) / bound, 0.0)
    i, j = np.unravel_index(int(ratio.argmax()), ratio.shape)
    print("FX-ORACLE", fmt, K, f"ratio {float(ratio.max()):.4f} at {an[i]} x {wn[j]}; non-finite outputs {int((~np.isfinite(y)).sum())} of {y.size}")
    if t == X.F16:
        assert float(ratio.max()) <= 1.0, (fmt, K, float(ratio.max()), an[i], wn[j])
    if t == X.F32:      # the predicted signed zero, at every K, scalar and AVX rows alike
        assert y[an.index("negtiny"), wn.index("tiny")].view(np.uint32) == 0x80000000 == y_fast[an.index("negtiny"), wn.index("tiny")].view(np.uint32)


def test_probe_reads_back_the_rounded_activations():
    """The oracle on the identity: fp16(x) (F16) / x (F32) by value on every token without a non-finite element (a -0 summed with +0 terms is
    +0), NaN everywhere on the others (0 x inf)."""
    K = 160
    x, an = X.activation_rows(K, SEED)
    for t in (X.F16, X.F32):
        y = O.mul_mat(t, X.probe(t, K), K, K, x)
        want = X.round_trip_f16(x) if t == X.F16 else x
        for i, n in enumerate(an):
            if np.isfinite(want[i]).all():
                assert np.array_equal(y[i], want[i]), (t, n)
                nz = want[i] != 0
                assert np.array_equal(y[i][nz].view(np.uint32), want[i][nz].view(np.uint32)), (t, n)
            else:
                assert np.isnan(y[i]).all(), (t, n)


# ---------------------------------------------------------------------------------------------------------------------------------------
# model files: the F16 palette
# ---------------------------------------------------------------------------------------------------------------------------------------

def test_f16_rewriter_changes_the_f16_matrices_only(tmp_path):
    import f64_model as F
    for name, fmt in (("test-v7", "Q5_1"), ("test-v6", "FP16")):
        path, plain = str(tmp_path / "p.bin"), str(tmp_path / "plain.bin")
        counts = B.write_f16_palette_model(synth, path, name, fmt, SEED)
        synth.write_model(plain, synth.CONFIGS[name], fmt, seed=SEED)
        _, before = F.read_file(plain)
        _, after = F.read_file(path)
        assert list(before) == list(after) and os.path.getsize(plain) == os.path.getsize(path)
        f16 = {k for k, (ty, dims, _) in before.items() if ty == F.F16 and len(dims) == 2}
        assert f16 == set(counts) and {"emb.weight", "head.weight"} <= f16
        assert ("blocks.1.att.w1" in f16) == (name == "test-v7") and ("blocks.0.ffn.key.weight" in f16) == (fmt == "FP16")
        for key in before:
            assert before[key][:2] == after[key][:2]
            assert (bytes(before[key][2]) == bytes(after[key][2])) == (key not in counts), key
        tot = {k: sum(c[k] for c in counts.values()) for k in B.F16_PALETTE}
        n = sum(tot.values())
        for k, share in (("keep", 0.60), ("neg", 0.10), ("zero", 0.08), ("subnormal", 0.10), ("minnorm", 0.04), ("lowbits", 0.08)):
            assert abs(tot[k] / n - share) < 0.01, (k, tot[k] / n)
        ty, dims, raw = after["head.weight"]
        old = np.frombuffer(bytes(before["head.weight"][2]), dtype=np.float16).astype(np.float64)
        new = np.frombuffer(bytes(raw), dtype=np.float16).astype(np.float64)
        assert np.isfinite(new).all() and np.abs(new).max() <= np.abs(old).max()
        assert ((new != 0) & (np.abs(new) < 2.0 ** -14)).mean() > 0.08 and (np.signbit(new) & (new == 0)).any() and (new == 2.0 ** -14).any()
        assert np.abs(new.reshape(dims[1], dims[0])).max(axis=1).min() > 0                         # no row is entirely zero


@pytest.mark.parametrize("name,fmt", [(n, "FP16") for n in ("test-v4", "test-v5.2", "test-v6", "test-v7")] + [("test-v7", "Q5_1"), ("test-v6", "Q4_0")])
def test_oracle_is_finite_and_the_reference_on_f16_palette_files(tmp_path, name, fmt):
    """40 tokens from the fresh state on the D = 256 file whose F16 matrices are redrawn with blocks_lib.f16_palette: logits of every step and
    the final state finite and within the gate of tests/test_cpu_f64_reference.py, unchanged (FP16 files 1e-3, quantised files 1e-2), of the
    float64 pass, e = max |oracle - f64| / (1 + max |f64|).

    Measured (seed 7), worst e over the steps' logits / final state; max |logit| 2.5 - 3.4:
      FP16   test-v4 1.4e-4 / 1.2e-4   test-v5.2 2.1e-4 / 1.1e-4   test-v6 1.9e-4 / 7.9e-5   test-v7 3.3e-4 / 1.5e-4
      test-v7 Q5_1 3.9e-3 / 3.6e-3     test-v6 Q4_0 1.0e-3 / 1.5e-4
    """
    import f64_model as F
    import stress_lib as S
    from test_cpu_f64_reference import QUANT_TOL, TOL, _err
    path = str(tmp_path / "m.bin")
    B.write_f16_palette_model(synth, path, name, fmt, SEED)
    O.lib().orc_set_fast(1)     # (the AVX rows: the scalar oracle in bits, test_oracle_on_hand_built_operands)
    try:
        om, fm = O.OracleModel(path), F.F64Model(path)
        toks = S.lcg_tokens(om.n_vocab, 40)
        st, ol = om.init_state(), []
        for tok in toks:
            lg, st = om.eval(tok, st)
            ol.append(lg)
        om.free()
    finally:
        O.lib().orc_set_fast(0)
    ol = np.stack(ol)
    assert np.isfinite(ol).all() and np.isfinite(st).all(), (name, fmt)
    fl, fst = fm.forward(toks, None)
    e = (max(_err(ol[i], fl[i]) for i in range(len(toks))), _err(st, fst))
    print("F16-PALETTE", name, fmt, f"{e[0]:.1e} / {e[1]:.1e}", f"max |logit| {float(np.abs(ol).max()):.2f}")
    assert max(e) <= TOL.get(fmt, QUANT_TOL), (name, fmt, e)
