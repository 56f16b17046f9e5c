"""Every decode path at the geometries it ADMITS (tests/geometry_lib.py), not only at the handful it was tuned on, against the CPU oracle:
np.array_equal on logits and on the whole state. The oracle's own worth on these files is held in tests/test_cpu_admitted_geometry.py; the
host-side stream layout of the ring kernel on all 117 admitted (D, F) pairs in tests/cpp/ring_geom_check.cpp and ring_wave_check.cpp.

A path takes a model or declines it at load time (ring_variant, mega_variant, p47_variant, fused_v6 / v7 / v4_supported) and each predicate
admits a range: before this file nothing launched k6_ring at an F other than 7168 / 8960 / 14336, k6_mega other than 7168 / 14336, k47 at a
rank set other than the two released ones, or a fused kernel at an F that is no multiple of 128. Every case ASSERTS decode_path() and
persist_kind() of the context it runs on (geometry_lib.CASES, written by hand from the predicates), so none passes by falling back; the
persistent cases also assert healthy() at the end, because a poll time-out drops a context to the per-layer launches, which are exact too.

Per case, on the context under test (and the first item also on a second context one path below, where the row names one):
  - ten single tokens from the fresh state; decode_greedy of 8 with state_store; a 97-token eval_sequence and its chunks-of-40 form; the
    opt-in fast sequence arms within FAST_ARM_REL_TOL (tests/conftest.py: the one tolerance of this file) -- all of it _check of
    tests/test_gpu_real_geometry.py, called, not copied
  - four tokens from an injected `normal` state of stress_lib.state_families (a mis-strided index shows at the first token only from a
    state that is not fresh)
  - one RWKVBatch of three slots (fresh, normal, normal scaled by 1/2), two eval passes

Which admitted edge each case sits on:
  ring (RWKV_MI_PERSIST=ring, kind 2)
    ring-2048-F6176         193 blocks, the lowest: three 64-block steps + ONE block; 63 workgroups own no key group (k_has false)
    ring-2048-F7200         225 blocks, F % 128 = 32: the sub-16-byte tail of qvec_stage
    ring-2048-F8192         256 blocks, the top: a key group on every workgroup; dim_ffn = 4 D, what a default-trained file has
    ring-2048-F7168-R64     the tuned F at the other mix rank (320 rows of time_maa_w1: 64 workgroups carry two)
    ring-2560-F8256         258 blocks, the lowest; ring-2560-F9536: 298 blocks, the top (894 of 896 gather units); -F8960-R64: mix rank 64
    ring-4096-F12352        386 blocks, the lowest: a two-block seventh step; ring-4096-F14272: 446 blocks; -F14336-R32: mix rank 32
    -Q8_0 / -Q5_1 / -Q5_0   another format at a non-tuned F of each D;  ring-2048-F7200-V4096: the folded head behind a non-tuned stream
  regs (RWKV_MI_PERSIST=regs, kind 1)
    regs-2048-F1024 / F7200 / F7488 (702 of 704 units, the top) / F7168-R64;  regs-4096-F8224 (257 blocks, the lowest) / F14304 (447 blocks,
    odd: the ring declines it);  regs-2048-F32: the bottom of the predicate, the LAST row, run last and alone (-k regs-2048-F32)
  outside (path 1 under the same switch, exact there): 2048 / F 6144 (192 blocks: three steps, the ring declines) . 2048 / F 8224 (257 blocks:
    ring and regs both decline) . 2560 / F 8288 (259 blocks, odd at two key groups per workgroup) . 4096 at decay rank 64 (ring and regs)
  k47 (the default path, kind 3): v7 D 256 ranks (32, 32, 32, 32) . (32, 64, 128, 32) (sum 256, the top) . one layer (no v1 / v2); outside: g 160,
    w 96, F = 3.5 D.  v7 D 2560 (32, 32, 32, 32) . (64, 96, 288, 32): lr1 of 480 on layer 1 = 7.5 poll slots of 64 (layer 0, without v1, has
    448 = 7 whole slots: only a layer with v1 has the partial slot); outside: g 352.  v4 D 768 / F 3104 != 4 D: fused
  fused (RWKV_MI_NO_MEGA=1, path 1) with per-op (RWKV_MI_NO_FUSED=1, path 0) on the same file: v6 D 512 / F 1824 (57 blocks, F % 128 = 32)
    ranks (48, 128) . D 1280 / F 4544 (F % 128 = 64) mix rank 256 . mix rank 260 and decay rank 32: fused declines, path 0.  v7 D 512 / F 1056
    ranks (128, 64, 256, 96) . D 1024 with w 512 . w 544 declines . one layer.  v4 D 512 / F 2048 . D 1280 / F 3104.  RWKV-5.1 / 5.2: per-op only

Result: all 49 cases pass as the kernels stood -- no kernel and no predicate changed, and no row of the table had to be corrected.

What the file sees that the suite before it does not (one-line mutations of csrc/fused_blocks.h on a side build, arithmetic on loaded values
only; "before": the 1648 GPU tests that existed before this file, of which 1644 pass and 4 skip on the unmutated build):
  qvec_stage without its word tail (the last           22 of the 49 cases here fail: every file with F % 128 != 0 in a format whose product reads
  qvec_bytes(K) % 16 bytes of a staged activation      the integer block sums (Q4_0, Q5_0; the Q8_0 and Q5_1 files pass) -- 5 fused, 1 k47-outside,
  image: integer block sums of the last blocks)        3 outside, and 5 regs + 8 ring cases through the fused context a persistent case runs
                                                       beside its kernel (only the fused kernels stage with qvec_stage).
                                                       Before: 0 fail (every F in the tree was a multiple of 128)
  batch_consume counts the clamped blocks past nb      44 fail: every case with a fused, k47 or regs context (the five that pass are the per-op
  as live (valid = true)                               ones: RWKV-5, and the files the fused path declines).
                                                       Before: 197 fail -- a clamp that is wrong at every row shorter than a step was never invisible
k6_ring itself is reached by neither (k6_mega and k47 by the second): it stages and consumes through its own code (ring_v6.hip), and
there the one arithmetic-only candidate of this kind -- counting the blocks past the end of a short last step -- changes nothing, because
those blocks are zero bytes in the stream (d = 0). A mutation of the ring that shows only at the new shapes would have to move an address, a trip count or a hand-over (k_has, the
key-group deal, the gather slots), which is not done on a shared device; what holds the ring here is the comparison itself at 14 shapes it
had never run at, with its path asserted before and after.
"""
import os

import numpy as np
import pytest

import geometry_lib as G
import oracle_lib as O
import stress_lib as S
from gpu_lib import pkg, synth
from test_gpu_injected_state import _row_tokens, _same
from test_gpu_real_geometry import _check

pytestmark = pytest.mark.gpu

ENV = ("RWKV_MI_NO_AUTOTUNE", "RWKV_MI_NO_FUSED", "RWKV_MI_NO_MEGA", "RWKV_MI_PERSIST", "RWKV_MI_SEQ_Q", "RWKV_MI_SEQ_F16")
SEED = 7
N_INJECTED, N_SLOTS, N_PASSES = 4, 3, 2


@pytest.fixture(autouse=True)
def _env():
    keep = {k: os.environ.get(k) for k in ENV}
    os.environ.update({"RWKV_MI_NO_AUTOTUNE": "1", "RWKV_MI_SEQ_Q": "exact", "RWKV_MI_SEQ_F16": "valu"})   # (the exact sequence arms: tests/conftest.py)
    for k in ("RWKV_MI_NO_FUSED", "RWKV_MI_NO_MEGA", "RWKV_MI_PERSIST"):
        os.environ.pop(k, None)
    O.lib().orc_set_fast(1)     # (the AVX row kernels: bit-identical to the scalar oracle, tests/test_oracle_golden.py)
    yield
    O.lib().orc_set_fast(0)
    for k, v in keep.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def _more(case):
    def more(m, g, om, spec):
        V = spec.n_vocab
        assert m.persist_kind() == case.kind, (case.id, m.persist_kind(), m.persist_info())
        assert g is m or (g.decode_path() == case.other_path and g.persist_kind() == 0), (case.id, g.decode_path())
        # from an injected state
        s0 = S.state_families(om, SEED, long_run=False)["normal"]
        toks = S.lcg_tokens(V, N_INJECTED, start=S.PROMPT_LEN)
        ost, st = s0, s0.copy()
        for i, t in enumerate(toks):
            ol, ost = om.eval(t, ost)
            lg, st = m.eval(t, st)
            _same(st, ost, case.id, "injected", i, "state")
            _same(lg, ol, case.id, "injected", i, "logits")
        # rows: three slots from three states, two passes
        starts = [None, s0, (s0 * np.float32(0.5)).astype(np.float32)]
        b = pkg.RWKVBatch(m, N_SLOTS)
        slots = list(range(N_SLOTS))
        refs = [om.init_state() if s is None else s for s in starts]
        for s in slots:
            b.state_load(s, None if starts[s] is None else starts[s].copy())
        for p in range(N_PASSES):
            toks = [_row_tokens(p, s, 1, V)[0] for s in slots]
            lg = b.eval(slots, toks)
            for s in slots:
                ol, refs[s] = om.eval(toks[s], refs[s])
                _same(lg[s], ol, case.id, "batch pass", p, "slot", s)
        for s in slots:
            _same(b.state_store(s), refs[s], case.id, "batch state, slot", s)
        b.free()
        if case.path == 2:
            assert m.healthy(), (case.id, m.persist_info())
            assert m.decode_path() == 2 and m.persist_kind() == case.kind, (case.id, "after the loops", m.decode_path(), m.persist_kind())
    return more


@pytest.mark.parametrize("case", G.CASES, ids=[c.id for c in G.CASES])
def test_admitted_geometry_against_the_oracle(tmp_path, case):
    _check(tmp_path, case.id, case.fmt, case.seed, case.path, None if case.other is None else dict(case.other), dict(case.env),
           spec=G.spec(synth, case), more=_more(case))
