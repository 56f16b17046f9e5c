"""tests/blocks_lib.py does what it claims, and the CPU oracle stays finite and stays the reference on it. CPU-only.

tests/test_gpu_block_extremes.py holds every quantised product of the GPU library to the oracle, bit for bit, on hand-built blocks (codes at
the ends of the format; scales 0, fp16-subnormal, 1, +-65504, of either sign; m of either sign and far larger than d) and on activation rows
that reach every branch of the activation quantiser. That is worth what the oracle is worth there. Here the scalar oracle is held to its
AVX row kernels bit for bit and to a float64 evaluation (f64_model._Matrix: the same codes and fp16 scales, every product and sum in
float64) within the rounding bound of two f32 sums of nb block terms,

    |oracle - f64| <= (2 nb + 8) 2^-24 A,   A = sum_k |x_q[k]| |q_w[k] d_w| + sum_b |s_x[b]| |m_w[b]|   (exact, per output),

which is the bound of tests/test_gpu_prefill_fast.py without its factor 1.5 and without Cauchy-Schwarz. At model level the D = 256 files
are redrawn with blocks_lib.model_palette and the oracle is held to tests/f64_model.py with the criterion and the QUANT_TOL gate of
tests/test_cpu_f64_reference.py, unchanged. The measured figures are in the docstrings of the two tests.
"""
import os

import numpy as np
import pytest

import blocks_lib as B
import f64_model as F
import oracle_lib as O
import stress_lib as S
from test_cpu_f64_reference import QUANT_TOL, _err, synth

SEED = 7
FORMATS = list(B.QTYPES)
N_TOKENS = 40


def _random_parts(t, n, rng):
    codes = rng.integers(B.CODE_MIN[t], B.CODE_MAX[t] + 1, size=(n, 32))
    vals = np.array(list(B.SCALES.values()), dtype=np.float16)
    d = vals[rng.integers(len(vals), size=n)]
    m = vals[rng.integers(len(vals), size=n)] if t in B.HAS_M else None
    return codes, d, m


@pytest.mark.parametrize("fmt", FORMATS)
def test_pack_blocks_is_the_inverse_of_block_parts(fmt):
    t, rng = B.QTYPES[fmt], np.random.default_rng(1)
    for codes, d, m in [_random_parts(t, 300, rng)] + [(B.family_codes(t, f, 11, rng), np.array(list(B.SCALES.values()), dtype=np.float16),
                                                         np.array(list(B.SCALES.values())[::-1], dtype=np.float16) if t in B.HAS_M else None)
                                                        for f in B.code_families(t)]:
        raw = B.pack_blocks(t, codes, d, m)
        assert raw.dtype == np.uint8 and raw.size == codes.shape[0] * F.BLOCK_BYTES[t]
        q, d2, m2 = F.block_parts(t, raw.tobytes(), codes.size)
        assert np.array_equal(B.stored_codes(t, q), codes), fmt
        assert np.array_equal(d2, d.astype(np.float64)) and (m is None) == (m2 is None), fmt
        assert m is None or np.array_equal(m2, m.astype(np.float64)), fmt
    if t in (B.Q5_0, B.Q5_1):   # bit j of qh is element j's fifth bit; low nibble of byte j is element j, high nibble element 16 + j
        codes = np.zeros((1, 32), dtype=np.int64)
        codes[0, 3], codes[0, 20] = 0x1A, 0x15
        raw = B.pack_blocks(t, codes, np.ones(1, dtype=np.float16), np.ones(1, dtype=np.float16) if t in B.HAS_M else None)
        pos = 4 if t in B.HAS_M else 2
        assert int(raw[pos:pos + 4].view("<u4")[0]) == (1 << 3) | (1 << 20) and raw[pos + 4 + 3] == 0x0A and raw[pos + 4 + 4] == 0x50


@pytest.mark.parametrize("fmt", FORMATS)
def test_oracle_dequantises_packed_rows_exactly(fmt):
    t, K = B.QTYPES[fmt], 768
    wb, names = B.weight_rows(t, K, SEED)
    n = K * len(names)
    q, d, m = F.block_parts(t, wb.tobytes(), n)
    want = q * d[:, None]                                          # exact in float64 (<= 8 + 11 bits), the sign of a zero kept
    if m is not None:
        want = want + m[:, None]                                  # one addition, exact in float64; the cast rounds once, as the oracle's f32 sum
    got = O.dequantize_row(t, wb, n)
    assert np.isfinite(got).all()
    assert np.array_equal(got.view(np.uint32), want.reshape(-1).astype(np.float32).view(np.uint32)), fmt


@pytest.mark.parametrize("fmt", FORMATS)
def test_pack_blocks_reproduces_the_reference_quantiser(fmt):
    t, rng = B.QTYPES[fmt], np.random.default_rng(5)
    acts, _ = B.activation_rows(768, SEED)
    x = np.concatenate([acts[np.abs(acts).max(axis=1) < 1e4].reshape(-1)] + [rng.standard_normal(32 * 64).astype(np.float32) * s for s in (1e-3, 0.05, 1.0, 50.0)])
    raw = O.quantize_row(t, x)
    q, d, m = F.block_parts(t, raw.tobytes(), x.size)
    assert np.array_equal(B.pack_blocks(t, B.stored_codes(t, q), d.astype(np.float16), None if m is None else m.astype(np.float16)), raw), fmt
    if t in (B.Q4_0, B.Q5_0):   # the reference quantiser writes a negative d for the blocks whose largest magnitude is positive
        assert 0.3 < (d < 0).mean() < 0.7, (fmt, float((d < 0).mean()))


def test_token_operands_put_every_family_on_every_tile_edge():
    rows, names = B.activation_rows(64, SEED)
    assert len(set(names)) == len(names) == rows.shape[0] and rows.dtype == np.float32 and np.isfinite(rows).all()
    for T in (1, 5, 31, 32, 65):
        ops = B.token_operands(64, T, SEED)
        for pos in {0, 31, 32, T - 1}:
            if pos < T:
                assert sorted(int(fam[pos]) for _, fam in ops) == list(range(len(names))), (T, pos)
        for x, fam in ops:
            assert x.shape == (T, 64) and np.array_equal(x.view(np.uint32), rows[fam].view(np.uint32))


def test_activation_rows_are_what_they_claim():
    for K in (64, 768, 2560):
        x, names = B.activation_rows(K, SEED)
        row = {n: x[i] for i, n in enumerate(names)}
        q, d, s = (dict(zip(names, v)) for v in zip(*(O.quantize_act(r) for r in x)))
        assert not row["zeros"].any() and not np.signbit(row["zeros"]).any()
        nz = row["negzero"].reshape(-1, 32)
        assert np.signbit(nz[0]).all() and not nz[0].any() and (K == 64 or (np.signbit(nz[2]).sum() == 16 and not nz[2].any()))
        for n in ("+127", "-127", "alt127"):
            assert (d[n] == 1.0).all() and (np.abs(q[n]) == 127).all()
        assert (q["+127"] == 127).all() and (q["-127"] == -127).all() and (s["alt127"] == 0).all() and (s["+127"] == 32 * 127).all()
        assert (d["ties"] == 0.5).all() and (d["halves"] == 1.0).all()
        h = row["halves"].reshape(-1, 32)[:, 1:]
        assert ((h - np.floor(h)) == 0.5).all()                       # every code of the row but the first of a block is a rounding tie ...
        assert np.array_equal(q["halves"].reshape(-1, 32)[:, 1:], np.where(h > 0, np.ceil(h), np.floor(h)).astype(np.int8))   # ... rounded away from zero
        assert ((row["spike"].reshape(-1, 32) != 0).sum(axis=1) == 1).all() and len(set(np.argmax(row["spike"].reshape(-1, 32) != 0, axis=1)[:32])) == min(32, K // 32)
        g = row["negmax"].reshape(-1, 32)
        assert (g[np.arange(g.shape[0]), np.abs(g).argmax(axis=1)] < 0).all() and (q["negmax"].reshape(-1, 32).min(axis=1) == -127).all()
        sub = 2.0 ** -14
        assert (d["n1e-3"] > 100 * 2.0 ** -24).all() and (d["n1e-3"] < sub).all()                   # fp16 subnormals
        assert set(np.unique(d["n2e-6"])) <= {0.0, 2.0 ** -24} and (K == 64 or len(np.unique(d["n2e-6"])) == 2)
        for n in ("n1e-6", "n3e-8"):
            assert (d[n] == 0).all() and s[n].any() and (np.abs(s[n]) <= 256 * 2.0 ** -24).all() and (np.abs(q[n]).reshape(-1, 32).max(axis=1) == 127).all()
        assert (d["n1e-40"] == 0).all() and (s["n1e-40"] == 0).all() and row["n1e-40"].any() and np.abs(row["n1e-40"]).max() < np.finfo(np.float32).tiny
        assert set(np.unique(d["alt8e6"])) <= {62976.0, 63008.0} and (s["alt8e6"] == 0).all()
        assert (s["c2000"] == 64000.0).all() and (q["c2000"] == 127).all()


@pytest.mark.parametrize("K", [64, 768, 2560])
@pytest.mark.parametrize("fmt", FORMATS)
def test_oracle_on_hand_built_blocks(fmt, K):
    """Every weight row x every activation row: the scalar oracle and its AVX row kernels agree bit for bit, everything is finite, the
    oracle is within (2 nb + 8) 2^-24 A of float64, the zero row and the 1e-40 row (d_x = s_x = 0 whatever the codes are) give exact
    zeros, and the largest block sum the format allows is reached (computed from the codes).

    Measured (seed 7): the worst |oracle - f64| / bound over all outputs, and max |y|, per format at K = 64 / 768 / 2560 (the share of the
    bound falls with K because the bound grows with nb and the error of a sum of nb terms with sqrt(nb) at most):
      Q4_0  0.097 / 0.019 / 0.010      2.5e14 / 3.0e15 / 1.0e16
      Q4_1  0.125 / 0.052 / 0.010      2.5e14 / 3.0e15 / 1.0e16
      Q5_0  0.119 / 0.025 / 0.012      5.2e14 / 6.2e15 / 2.1e16
      Q5_1  0.147 / 0.044 / 0.014      5.2e14 / 6.2e15 / 2.1e16
      Q8_0  0.132 / 0.017 / 0.007      4.3e15 / 5.1e16 / 1.7e17
    """
    t, nb = B.QTYPES[fmt], K // 32
    wb, wnames = B.weight_rows(t, K, SEED)
    x, anames = B.activation_rows(K, SEED)
    R = len(wnames)
    O.lib().orc_set_fast(0)
    y = O.mul_mat(t, wb, K, R, x)
    O.lib().orc_set_fast(1)
    try:
        y_fast = O.mul_mat(t, wb, K, R, x)
    finally:
        O.lib().orc_set_fast(0)
    assert np.array_equal(y.view(np.uint32), y_fast.view(np.uint32)), (fmt, K, "scalar oracle != AVX row kernels")
    assert np.isfinite(y).all(), (fmt, K)
    assert not y[anames.index("zeros")].any() and not y[anames.index("n1e-40")].any()
    mat = F._Matrix(t, (K, R), wb.tobytes())
    ref = mat(x.astype(np.float64))
    xq, sx, qx = np.empty(x.shape), np.empty((x.shape[0], nb)), np.empty(x.shape)
    for i in range(x.shape[0]):
        q, d, s = O.quantize_act(x[i])
        qx[i] = q
        xq[i] = (q.astype(np.float64).reshape(-1, 32) * d.astype(np.float64)[:, None]).reshape(-1)
        sx[i] = s
    A = np.abs(xq) @ np.abs(mat.w.astype(np.float64)).T
    if mat.m is not None:
        A += np.abs(sx) @ np.abs(mat.m).T
    bound = (2 * nb + 8) * 2.0 ** -24 * A
    err = np.abs(y.astype(np.float64) - ref)
    ratio = float((err[A > 0] / bound[A > 0]).max())
    print("BLOCKS", fmt, K, f"ratio {ratio:.4f} max|y| {float(np.abs(y).max()):.2e}")
    assert (err <= bound).all(), (fmt, K, ratio, [(anames[i], wnames[j]) for i, j in zip(*np.nonzero(err > bound))][:5])
    # the block sums these operands reach, from the codes
    qw, _, _ = F.block_parts(t, wb.tobytes(), K * R)
    isum = np.einsum("abj,rbj->arb", qx.reshape(-1, nb, 32), qw.reshape(R, nb, 32))
    assert np.abs(isum).max() == B.ISUM_MAX[t] and (t != B.Q8_0 or B.ISUM_MAX[t] == 32 * 127 * 128), (fmt, K, float(np.abs(isum).max()), B.ISUM_MAX[t])


CELLS = [(n, f) for n in ("test-v4", "test-v5.2", "test-v6", "test-v7") for f in ("Q4_0", "Q5_1")] + [("test-v6", f) for f in ("Q4_1", "Q5_0", "Q8_0")]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    base, made = tmp_path_factory.mktemp("blocks"), {}

    def get(name, fmt):
        if (name, fmt) not in made:
            p = str(base / f"{name}-{fmt}-palette.bin")
            made[(name, fmt)] = (p, B.write_palette_model(synth, p, name, fmt, SEED))
        return made[(name, fmt)]
    yield get
    for p, _ in made.values():
        os.remove(p)


def test_rewriter_changes_the_quantised_tensors_only(files, tmp_path):
    name, fmt = "test-v6", "Q5_1"
    path, counts = files(name, fmt)
    plain = str(tmp_path / "plain.bin")
    synth.write_model(plain, synth.CONFIGS[name], fmt, seed=SEED)
    _, before = F.read_file(plain)
    _, after = F.read_file(path)
    assert list(before) == list(after) and os.path.getsize(plain) == os.path.getsize(path)
    for key in before:
        assert before[key][:2] == after[key][:2]
        assert (bytes(before[key][2]) == bytes(after[key][2])) == (key not in counts), key
    quant = {k for k, (ty, dims, _) in before.items() if ty in F.BLOCK_BYTES}
    assert quant == set(counts) and "blocks.0.ffn.value.weight" in quant and "emb.weight" not in quant
    # the shares of the palette, and what the families are
    tot = {k: sum(c.get(k, 0) for c in counts.values()) for k in B.PALETTE_1}
    n = sum(tot.values())
    for k, share in (("keep", 0.50), ("neg", 0.15), ("subnormal", 0.10), ("codes", 0.10)):
        assert abs(tot[k] / n - share) < 0.02, (k, tot[k] / n)
    assert abs((tot["zero"] + tot["zero-both"]) / n - 0.10) < 0.02 and abs((tot["m-zero"] + tot["m-scaled"]) / n - 0.05) < 0.02
    ty, dims, raw = after["blocks.1.ffn.key.weight"]
    q, d, m = F.block_parts(ty, bytes(raw), int(np.prod(dims)))
    d, m = d.reshape(dims[1], -1), m.reshape(dims[1], -1)
    first = B.ZERO_KEY_ROWS[1]
    assert not d[first:first + 64].any() and not m[first:first + 64].any() and d[first - 1].any() and d[first + 64].any()
    assert (d < 0).any() and (m > 0).any() and ((d == 0) & (m != 0)).any() and (np.abs(d[d != 0]) < 2.0 ** -14).any()
    ty, dims, raw = after["blocks.0.att.key.weight"]
    _, d0, _ = F.block_parts(ty, bytes(before["blocks.0.att.key.weight"][2]), int(np.prod(dims)))
    _, d1, m1 = F.block_parts(ty, bytes(raw), int(np.prod(dims)))
    assert abs((d1 == -d0).mean() - 0.15) < 0.02 and (np.abs(m1) > 4 * np.abs(d0) * 16).sum() == 0   # |m| stays within 4 x its old value (16 d)


@pytest.mark.parametrize("name,fmt", CELLS)
def test_oracle_is_finite_and_the_reference_on_palette_files(files, name, fmt):
    """40 tokens from the fresh state on the D = 256 file redrawn with model_palette: logits of every step and the final state finite and
    within QUANT_TOL = 1e-2 of the float64 pass, e = max |oracle - f64| / (1 + max |f64|).

    Measured (seed 7), worst e over the steps' logits / final state:
      test-v4    Q4_0 2.1e-5 / 5.4e-7    Q5_1 1.5e-3 / 5.4e-7
      test-v5.2  Q4_0 1.1e-3 / 2.4e-4    Q5_1 1.6e-3 / 1.6e-7
      test-v6    Q4_0 1.0e-3 / 1.2e-4    Q5_1 2.2e-3 / 5.6e-5    Q4_1 2.1e-3 / 1.7e-4    Q5_0 1.9e-3 / 2.1e-3    Q8_0 1.4e-3 / 8.8e-4
      test-v7    Q4_0 3.4e-3 / 2.1e-3    Q5_1 5.7e-3 / 1.1e-3
    max |logit| stays between 1.8 and 2.5. Every cell met the gate on the palette as blocks_lib.model_palette states it: none was narrowed.
    """
    path, _ = files(name, fmt)
    O.lib().orc_set_fast(1)     # (the AVX row kernels: bit-identical to the scalar oracle, test_oracle_on_hand_built_blocks)
    try:
        om, fm = O.OracleModel(path), F.F64Model(path)
        toks = S.lcg_tokens(om.n_vocab, N_TOKENS)
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
    assert np.isfinite(fl).all() and np.isfinite(fst).all(), (name, fmt, "float64")
    e = (max(_err(ol[i], fl[i]) for i in range(N_TOKENS)), _err(st, fst))
    print("PALETTE", name, fmt, f"{e[0]:.1e} / {e[1]:.1e}", f"max |logit| {float(np.abs(ol).max()):.2f}")
    assert max(e) <= QUANT_TOL, (name, fmt, e)
