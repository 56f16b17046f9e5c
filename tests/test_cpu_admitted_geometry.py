"""The case table of tests/geometry_lib.py and the CPU oracle on its files, CPU-only.

1. The table builds what it claims: per case the tensor shapes synth.write_model writes (n_embed, blocks of an F-long row, F % 128, mix and
   decay rank, the RWKV-7 ranks and their per-layer sums) against figures written out here by hand, and the expected path against the
   predicates re-derived in geometry_lib (ring_admits, mega_admits): a ring / regs row is inside its predicate, an `outside` row is
   outside both kernels its switch could pick.
2. The oracle is worth comparing against on these files: for the first row of every (architecture, n_embed) of the table, the oracle is
   held to the float64 pass (tests/f64_model.py) with the criterion and the gate of tests/test_cpu_f64_reference.py, unchanged:
   e = max |oracle - f64| / (1 + max |f64|) on every step's logits and on the state, e <= QUANT_TOL = 1e-2 (every file here is quantised).
   The figures are in the docstring of test_oracle_is_the_reference_on_the_admitted_geometries.
"""
import os

import numpy as np
import pytest

import f64_model as F
import geometry_lib as G
import oracle_lib as O
import stress_lib as S
from test_cpu_f64_reference import QUANT_TOL, _err, synth

SEED = 7
N_SERIAL, N_SEQ = 8, 24

# id -> (n_embed, blocks of an F-long row, F % 128, mix rank, decay rank), RWKV-6
V6 = {
    "ring-2048-F6176": (2048, 193, 32, 32, 64), "ring-2048-F7200": (2048, 225, 32, 32, 64), "ring-2048-F8192": (2048, 256, 0, 32, 64),
    "ring-2048-F7168-R64": (2048, 224, 0, 64, 64), "ring-2560-F8256": (2560, 258, 64, 32, 64), "ring-2560-F9536": (2560, 298, 64, 32, 64),
    "ring-2560-F8960-R64": (2560, 280, 0, 64, 64), "ring-4096-F12352": (4096, 386, 64, 64, 128), "ring-4096-F14272": (4096, 446, 64, 64, 128),
    "ring-4096-F14336-R32": (4096, 448, 0, 32, 128), "ring-2048-F6176-Q8_0": (2048, 193, 32, 32, 64), "ring-2560-F9536-Q5_1": (2560, 298, 64, 32, 64),
    "ring-4096-F12352-Q5_0": (4096, 386, 64, 64, 128), "ring-2048-F7200-V4096": (2048, 225, 32, 32, 64),
    "regs-2048-F1024": (2048, 32, 0, 32, 64), "regs-2048-F7200": (2048, 225, 32, 32, 64), "regs-2048-F7488": (2048, 234, 64, 32, 64),
    "regs-2048-F7168-R64": (2048, 224, 0, 64, 64), "regs-4096-F8224": (4096, 257, 32, 64, 128), "regs-4096-F14304": (4096, 447, 96, 64, 128),
    "regs-2048-F32": (2048, 1, 32, 32, 64),
    "outside-2048-F6144-ring": (2048, 192, 0, 32, 64), "outside-2048-F8224-ring": (2048, 257, 32, 32, 64), "outside-2048-F8224-regs": (2048, 257, 32, 32, 64),
    "outside-2560-F8288": (2560, 259, 96, 32, 64), "outside-4096-DR64-ring": (4096, 448, 0, 64, 64), "outside-4096-DR64-regs": (4096, 448, 0, 64, 64),
    "fused-v6-512-F1824-R48-DR128": (512, 57, 32, 48, 128), "fused-v6-1280-F4544-R256": (1280, 142, 64, 256, 64),
    "fused-v6-512-R260-declines": (512, 57, 32, 260, 64), "fused-v6-512-DR32-declines": (512, 57, 32, 32, 32),
}
# id -> (n_embed, F, layers, (w, a, g, v), sum on layer 0 (no v1), sum on the other layers), RWKV-7
V7 = {
    "k47-v7-256-r32": (256, 1024, 2, (32, 32, 32, 32), 96, 128), "k47-v7-256-sum256": (256, 1024, 2, (32, 64, 128, 32), 224, 256),
    "k47-v7-256-one-layer": (256, 1024, 1, (64, 64, 96, 32), 224, None), "k47-v7-256-g160-outside": (256, 1024, 2, (32, 32, 160, 32), 224, 256),
    "k47-v7-256-w96-outside": (256, 1024, 2, (96, 32, 32, 32), 160, 192), "k47-v7-256-F896-outside": (256, 896, 2, (64, 64, 96, 32), 224, 256),
    "k47-v7-2560-r32": (2560, 10240, 2, (32, 32, 32, 32), 96, 128), "k47-v7-2560-sum480": (2560, 10240, 2, (64, 96, 288, 32), 448, 480),
    "k47-v7-2560-g352-outside": (2560, 10240, 2, (96, 96, 352, 64), 544, 608),
    "fused-v7-512-F1056": (512, 1056, 2, (128, 64, 256, 96), 448, 544), "fused-v7-1024-w512": (1024, 4096, 2, (512, 32, 32, 32), 576, 608),
    "fused-v7-512-w544-declines": (512, 1056, 2, (544, 64, 256, 96), 864, 960), "fused-v7-512-one-layer": (512, 1056, 1, (128, 64, 256, 96), 448, None),
}
# id -> (n_embed, F, F % 128), RWKV-4 and RWKV-5
OTHER = {"k47-v4-768-F3104-outside": (768, 3104, 32), "fused-v4-512-F2048": (512, 2048, 0), "fused-v4-1280-F3104": (1280, 3104, 32),
         "perop-v5.1-512-F1824": (512, 1824, 32), "perop-v5.2-512-F1824": (512, 1824, 32)}


def test_every_row_has_its_figures():
    assert set(V6) | set(V7) | set(OTHER) == set(G.BY_ID) and len(V6) + len(V7) + len(OTHER) == len(G.CASES)
    assert G.CASES[-1].id == "regs-2048-F32"      # (the bottom of mega_variant runs last)
    assert all(c.fmt in synth.BLOCK_BYTES for c in G.CASES)


@pytest.mark.parametrize("case", G.CASES, ids=[c.id for c in G.CASES])
def test_the_table_builds_what_it_claims(case):
    spec = G.spec(synth, case)
    dims = {k: d for k, d, _ in synth._tensor_list(spec)}
    D, L = spec.n_embed, spec.n_layer
    assert dims["emb.weight"] == (D, spec.n_vocab) and spec.n_vocab == (4096 if case.id.endswith("V4096") else 512)
    assert D % 256 == 0 and (case.arch == "4" or (spec.head_size == 64 and D % 64 == 0))
    F_ = dims["blocks.0.ffn.key.weight"][1]
    assert dims[f"blocks.{L - 1}.ffn.value.weight"] == (F_, D) and f"blocks.{L}.ln1.weight" not in dims
    if case.arch == "6":
        want_D, nb, f128, R, DR = V6[case.id]
        got = (D, F_ // 32, F_ % 128, dims["blocks.0.att.time_maa_w1"][1] // 5, dims["blocks.0.att.time_decay_w1"][1])
        assert F_ % 32 == 0 and got == (want_D, nb, f128, R, DR) and dims["blocks.0.att.time_maa_w2"] == (R, D, 5), (case.id, got)
        ring, regs = G.ring_admits(D, F_, DR, R), G.mega_admits(D, F_, DR, R)
        if case.group == "ring":
            assert ring and (case.path, case.kind) == (2, 2) and dict(case.env) == G.RING
        elif case.group == "regs":
            assert regs and (case.path, case.kind) == (2, 1) and dict(case.env) == G.REGS
        elif case.group == "outside":
            assert not (ring if dict(case.env) == G.RING else regs) and (case.path, case.kind) == (1, 0)
            assert DR in (64, 128) and R <= 256    # (what fused_v6_supported asks: the fused launches take it)
        else:
            assert dict(case.env) == G.NO_MEGA and case.path == (1 if DR in (64, 128) and R <= 256 else 0)
    elif case.arch == "7":
        want_D, want_F, want_L, ranks, sum0, sum1 = V7[case.id]
        got = tuple(dims[f"blocks.0.att.{n}1"][1] for n in "wag") + (dims["blocks.1.att.v1"][1] if L > 1 else spec.v7_rank_v,)
        assert (D, F_, L) == (want_D, want_F, want_L) and got == ranks, (case.id, got)
        assert "blocks.0.att.v1" not in dims and sum(ranks[:3]) == sum0 and (L == 1 or sum(ranks) == sum1)
        w, a, g, v = ranks
        fused = all(r % 32 == 0 and r <= 512 for r in ranks) and F_ % 32 == 0
        cap = {256: (128, 64, 256), 2560: (320, 96, 576)}.get(D)
        k47 = fused and cap is not None and F_ == 4 * D and g <= cap[0] and max(w, a, v if L > 1 else 0) <= cap[1] and (sum1 if L > 1 else sum0) <= cap[2]
        want = (2, 3) if (k47 and dict(case.env) == G.DEFAULT) else ((1, 0) if fused else (0, 0))
        assert (case.path, case.kind) == want, (case.id, want)
        if case.id == "k47-v7-2560-sum480":
            assert sum1 % 64 == 32 and sum0 % 64 == 0
    else:
        want_D, want_F, f128 = OTHER[case.id]
        assert (D, F_, F_ % 128) == (want_D, want_F, f128) and F_ % 32 == 0
        if case.arch == "4":
            assert (case.path, case.kind) == (1, 0) and (dict(case.env) == G.NO_MEGA or F_ != 4 * D)
        else:
            assert (case.path, case.kind, case.other) == (0, 0, None)


@pytest.fixture(autouse=True, scope="module")
def _oracle_row_kernels():
    O.lib().orc_set_fast(1)     # (the AVX row kernels: bit-identical to the scalar oracle, tests/test_oracle_golden.py)
    yield
    O.lib().orc_set_fast(0)


REPS = G.representatives()


@pytest.mark.parametrize("case", REPS, ids=[c.id for c in REPS])
def test_oracle_is_the_reference_on_the_admitted_geometries(tmp_path, case):
    """8 serial tokens from the fresh state, then 24 tokens at once from the `normal` state of stress_lib.state_families: logits of every
    step and the state finite and within QUANT_TOL = 1e-2 of the float64 pass run from the same state. The file read back has the n_embed,
    ffn size and layer count of the row.

    Measured (seed of the row), serial logits / serial state / sequence logits / sequence state:
      ring-2048-F6176               v6 D 2048  2.0e-3 / 2.5e-3 / 1.4e-3 / 3.4e-3
      ring-2560-F8256               v6 D 2560  1.8e-3 / 2.6e-3 / 2.0e-3 / 3.5e-3
      ring-4096-F12352              v6 D 4096  1.5e-3 / 3.6e-3 / 2.1e-3 / 3.3e-3
      k47-v7-256-r32                v7 D 256   1.0e-3 / 3.1e-7 / 6.6e-8 / 2.2e-6
      k47-v7-2560-r32               v7 D 2560  6.5e-4 / 7.5e-7 / 2.3e-3 / 1.4e-3
      k47-v4-768-F3104-outside      v4 D 768   5.3e-6 / 1.3e-7 / 7.9e-8 / 7.5e-7
      fused-v6-512-F1824-R48-DR128  v6 D 512   2.5e-3 / 1.6e-3 / 6.4e-8 / 2.3e-7
      fused-v6-1280-F4544-R256      v6 D 1280  3.7e-4 / 1.5e-7 / 7.7e-4 / 1.0e-3
      fused-v7-512-F1056            v7 D 512   1.7e-3 / 8.4e-4 / 5.9e-8 / 2.3e-6
      fused-v7-1024-w512            v7 D 1024  1.9e-3 / 1.0e-3 / 9.0e-4 / 7.8e-4
      fused-v4-512-F2048            v4 D 512   1.2e-5 / 1.4e-7 / 1.0e-3 / 5.5e-4
      fused-v4-1280-F3104           v4 D 1280  1.9e-5 / 1.4e-7 / 5.1e-4 / 2.3e-4
      perop-v5.1-512-F1824          v5.1 D 512 7.6e-8 / 1.3e-7 / 7.1e-8 / 2.1e-7
      perop-v5.2-512-F1824          v5.2 D 512 6.6e-6 / 1.6e-7 / 4.5e-5 / 1.6e-7
    The worst cell is 3.6e-3, under the gate of 1e-2. (Where an N(0, 1) state makes the logits large the criterion, relative to max |f64|,
    reads 1e-7: the error there is the f32 rounding of the state's contribution.)
    """
    p = str(tmp_path / "m.bin")
    spec = G.spec(synth, case)
    synth.write_model(p, spec, case.fmt, seed=case.seed)
    hdr, tensors = F.read_file(p)
    assert (hdr["n_embed"], hdr["n_layer"], hdr["n_vocab"]) == (spec.n_embed, spec.n_layer, spec.n_vocab)
    assert tensors["blocks.0.ffn.key.weight"][1] == (spec.n_embed, spec.ffn) and tensors["blocks.0.ffn.key.weight"][0] == O.TYPE_IDS[case.fmt]
    om, fm = O.OracleModel(p), F.F64Model(p)
    assert (fm.n_embed, fm.n_layer, fm.state_len) == (om.n_embed, om.n_layer, om.state_len)
    toks = S.lcg_tokens(om.n_vocab, N_SERIAL + N_SEQ, start=S.PROMPT_LEN)
    errs = {}
    st, ol = om.init_state(), []
    for t in toks[:N_SERIAL]:
        lg, st = om.eval(t, st)
        ol.append(lg)
    fl, fst = fm.forward(toks[:N_SERIAL], None)
    assert np.isfinite(np.stack(ol)).all() and np.isfinite(st).all()
    errs["serial logits"], errs["serial state"] = max(_err(ol[i], fl[i]) for i in range(N_SERIAL)), _err(st, fst)
    s0 = S.state_families(om, SEED, long_run=False)["normal"]
    lg, so = om.eval_sequence(toks[N_SERIAL:], s0.copy())
    flg, fso = fm.eval_sequence(toks[N_SERIAL:], s0)
    assert np.isfinite(lg).all() and np.isfinite(so).all()
    errs["seq logits"], errs["seq state"] = _err(lg, flg), _err(so, fso)
    om.free()
    os.remove(p)
    print("ADMITTED", case.id, case.fmt, " / ".join(f"{v:.1e}" for v in errs.values()))
    assert all(v <= QUANT_TOL for v in errs.values()), (case.id, QUANT_TOL, errs)
