"""The CPU oracle at head sizes other than 64 (tests/heads_lib.py), CPU-only: it and the float64 pass (tests/f64_model.py) read the
intended geometry off every file, and the oracle is held to the float64 pass with the criterion and the gates of
tests/test_cpu_f64_reference.py, unchanged: e = max |oracle - f64| / (1 + max |f64|) on every step's logits and on the final state,
e <= 1e-3 (FP16), QUANT_TOL = 1e-2 (Q5_1). This is what makes the oracle worth comparing against in tests/test_gpu_head_sizes.py.

The figures are in the docstring of test_oracle_is_the_reference_at_every_head_size.
"""
import numpy as np
import pytest

import f64_model as F
import heads_lib as HL
import oracle_lib as O
import stress_lib as S
from test_cpu_f64_reference import QUANT_TOL, TOL, _err, synth

N_TOKENS = 40
FAMILIES = ("normal", "large", "tiny", "long-run")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    f = HL.Files(synth, tmp_path_factory.mktemp("heads"))
    yield f
    f.close()


@pytest.fixture(autouse=True, scope="module")
def _oracle_row_kernels():
    O.lib().orc_set_fast(1)     # (the AVX row kernels: bit-identical to the scalar oracle, tests/test_oracle_golden.py)
    yield
    O.lib().orc_set_fast(0)


@pytest.mark.parametrize("fmt", HL.FORMATS)
@pytest.mark.parametrize("row", HL.ROWS, ids=HL.row_id)
def test_both_readers_see_the_geometry_of_the_table(files, row, fmt):
    arch, D, S_ = row
    L = 3 if arch == "7" else 2
    major, minor = (int(arch[0]), int(arch[2:]) if len(arch) > 1 else 0)
    want = ((major, minor), 512, D, L, D // S_, S_, L * D * (2 + S_))
    p = files(row, fmt, HL.weights_of(row)[0])
    m, om = F.F64Model(p), O.OracleModel(p)
    got_f = (tuple(m.arch), m.n_vocab, m.n_embed, m.n_layer, m.head_count, m.head_size, m.state_len)
    got_o = ((om.arch_major, om.arch_minor), om.n_vocab, om.n_embed, om.n_layer, om.head_count, om.head_size, om.state_len)
    om.free()
    assert got_f == want, (row, fmt, "float64 pass", got_f)
    assert got_o == want, (row, fmt, "oracle", got_o)


@pytest.mark.parametrize("fmt", HL.FORMATS)
@pytest.mark.parametrize("row", HL.ROWS, ids=HL.row_id)
def test_oracle_is_the_reference_at_every_head_size(files, row, fmt):
    """40 tokens of lcg_tokens from the normal, large, tiny and long-run states, on the plain and the stressed copy (the D = 1024 rows: the
    stressed copy): logits of every step and the final state finite and within the format's gate of the float64 pass run from the same state.

    Measured (seed 7), the worst e of each row over both copies and the four families, logits of any step / final state:
                        Q5_1 (gate 1e-2)        FP16 (gate 1e-3)
      v5.1 D256  S32    2.9e-3 / 1.3e-3         4.0e-4 / 1.6e-4
      v5.2 D256  S16    1.8e-3 / 8.1e-4         2.1e-4 / 1.3e-4
      v6   D256  S32    4.0e-3 / 4.5e-3         3.2e-4 / 9.0e-5
      v6   D768  S96    3.2e-3 / 1.7e-3         2.1e-4 / 1.0e-4
      v6   D256  S128   5.3e-3 / 4.7e-3         2.4e-4 / 1.0e-4
      v6   D1024 S512   3.1e-3 / 4.2e-3         4.1e-4 / 1.2e-4
      v7   D256  S32    4.9e-3 / 4.3e-3         2.6e-4 / 1.1e-4
      v7   D256  S16    7.2e-3 / 4.2e-3         3.1e-4 / 2.6e-4
      v7   D768  S96    3.9e-3 / 4.3e-3         2.3e-4 / 1.8e-4
      v7   D256  S128   5.3e-3 / 4.7e-3         2.3e-4 / 1.1e-4
      v7   D1024 S512   3.9e-3 / 4.4e-3         2.5e-4 / 1.3e-4
    The worst cell of all is 7.2e-3 (Q5_1) and 4.1e-4 (FP16). No input range had to be narrowed.
    """
    tol = TOL.get(fmt, QUANT_TOL)
    worst = [0.0, 0.0]
    for weights in HL.weights_of(row):
        path = files(row, fmt, weights)
        om, fm = O.OracleModel(path), F.F64Model(path)
        toks = S.lcg_tokens(om.n_vocab, N_TOKENS, start=S.PROMPT_LEN)
        fam = S.state_families(om, HL.SEED)
        errs = {}
        for family in FAMILIES:
            s0 = fam[family]
            st, ol = s0.copy(), []
            for t in toks:
                lg, st = om.eval(t, st)
                ol.append(lg)
            ol = np.stack(ol)
            assert np.isfinite(ol).all() and np.isfinite(st).all(), (row, fmt, weights, family)
            fl, fst = fm.forward(toks, s0)
            assert np.isfinite(fl).all() and np.isfinite(fst).all(), (row, fmt, weights, family, "float64")
            errs[family] = (max(_err(ol[i], fl[i]) for i in range(N_TOKENS)), _err(st, fst))
        om.free()
        print("HEADS", HL.row_id(row), fmt, weights, " ".join(f"{k} {a:.1e}/{b:.1e}" for k, (a, b) in errs.items()))
        assert all(max(e) <= tol for e in errs.values()), (row, fmt, weights, tol, errs)
        worst = [max(worst[0], max(e[0] for e in errs.values())), max(worst[1], max(e[1] for e in errs.values()))]
    print("HEADS-WORST", HL.row_id(row), fmt, f"{worst[0]:.1e} / {worst[1]:.1e}")
