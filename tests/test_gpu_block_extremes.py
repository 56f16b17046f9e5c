"""Every quantised product on hand-built blocks (tests/blocks_lib.py), against the CPU oracle: np.array_equal on the bit patterns wherever
a kernel promises ggml's addition order. The oracle's own worth on these operands is held in tests/test_cpu_block_extremes.py.

Kernel level (rwkv_mi_test_mul_mat of librwkv_testhooks.so; all five formats; (K, N) = (64, 37), (768, 130), (2560, 37); T = 1, 5, 31, 32,
65; per case one call for every rotation of the activation families over the tokens, each with the next N weight rows -- every family
lands on token 0, 31, 32 and T - 1, and every weight row is used, both asserted):
  T < 32    k_quant_act + the matvec (T = 1) and its token-tiled form: the hook takes launch_quantize_act + launch_matvec_q below
            k_mfma_min_tokens = 32 (csrc/testhooks.cpp)
  T >= 32   the tile quantiser (quantize_tile_unit) + k_mmq_mfma, the exact walk; with K = 2560 (80 blocks >= 64) and so few tiles its
            split walk + k_mmq_combine (launch_mmq_mfma cuts the walk only for rows of >= 64 blocks). One shape of 8 x 4 tiles at K = 768
            (N = 1024, T = 256, Q4_0 and Q5_0) runs the unsplit grid. The counter of k_mmq_fast launches stays put: the exact arm ran.
  plain-order arm  RWKV_MI_SEQ_Q=force at (512, 256, 128) and (2560, 136, 100): k_mmq_fast, asserted by its launch counter; the bound of
            tests/test_gpu_prefill_fast.py with A as defined there; the exact arm on the same operands bit-identical, counter unchanged.
  rwkv_mi_test_quantize_act (k_quant_act)  d, s everywhere; q and isum where amax >= 2^-100 (below, the reference's reciprocal overflows).
  A Q8_0 probe matrix (row n: code 1 at element n, d = 1) returns d_x q_x[n] of every token: one case of its own on both quantisers, and
  the failure message of the product tests names the activation codes that differ by position.

Model level (files of synth redrawn with blocks_lib.model_palette; every family present in every tensor, asserted where the file is made),
with _case / _open of tests/test_gpu_injected_state.py -- decode_path() and persist_kind() asserted there for every model opened:
  per-op (decode_path 0), fused (1), k47 (2, kind 3)   D = 256: Q4_0 and Q5_1 of RWKV-4, 5.2, 6, 7; Q4_1, Q5_0, Q8_0 of RWKV-6
  ring (2, kind 2) and regs (2, kind 1)                mega-v6-2048 Q4_0 under RWKV_MI_PERSIST=ring / =regs
  k47                                                  slice-v7-2560 Q5_1, slice-v4-768 Q5_1
Per case, from the fresh state, logits and whole state with np.array_equal: 4 tokens of eval and decode_greedy of 6 on every path of the
case; eval_sequence of 40 tokens and the same in chunks of 33; an RWKVBatch of 3 slots: two eval passes, then eval_ragged of lengths 1, 33, 3.

What the file sees (one-line mutations of a side build each; the whole GPU suite was run on every build: failures here / in the rest):
  quantize_tile_unit (prefill.hip), roundf -> rintf        50 here (30 products with T >= 32, both unsplit grids, all 10 plain-order cases,
                                                           the probe at T = 65, 5 sequence and 2 batch cases) / 115 in the rest: at the
                                                           sizes of test_gpu_prefill*.py (20 + 13 fail) Gaussian rows hold ties by chance
  unpack_raw (kdev.h), sign of the weight scale dropped    105 here (45 products with T < 32 -- every format, shape and T --, every model
                                                           case on every call) / 104 in the rest, all in tests that run reference-quantised
                                                           weights on the per-op and fused kernels (test_gpu_mul_mat 36, test_gpu_prefill 20,
                                                           test_gpu_tiny_rwkv 12, test_gpu_synthetic 10, ...); none in test_gpu_injected_state,
                                                           test_gpu_mega, test_gpu_persist_v47 or test_gpu_ring_*: no persistent kernel had a negative d
  k6_ring (ring_v6.hip), |d| after its own unpack          2 here (eval and decode_greedy of the ring case) / 0: the rest of the suite passes
  k47 (persist_v47.hip rows_issue), m -> -|m|              8 here (eval and decode_greedy of the four Q5_1 k47 cases) / 0: the rest passes
  quant_vec4 (persist.h), roundf -> rintf                  1 here (eval, slice-v7-2560) / 29 in the rest (test_gpu_mega, test_gpu_ring_variants,
                                                           test_gpu_persist_v47, ...): not invisible at model level -- at D >= 2048 a few
                                                           LayerNorm outputs land on a tie by chance; no palette steers one there
The sequence and batch cases of the k47 / ring files pass under the two persistent-kernel mutations: those calls run the sequence and
per-op kernels, which the mutations leave alone.
"""
import ctypes
import os

import numpy as np
import pytest

import blocks_lib as B
import f64_model as F
import oracle_lib as O
import stress_lib as S
from gpu_lib import gpu_mul_mat, gpu_quantize_act, hooks_library, library, pkg, synth
from test_gpu_injected_state import ARCH_OF, _case, _env, _open, _row_tokens, _same  # noqa: F401  (_env: the autouse fixture of that file)

pytestmark = pytest.mark.gpu

SEED = 7
FORMATS = list(B.QTYPES)
SHAPES = [(64, 37), (768, 130), (2560, 37)]
TOKENS = [1, 5, 31, 32, 65]


@pytest.fixture(autouse=True, scope="module")
def _oracle_row_kernels():
    O.lib().orc_set_fast(1)     # (the AVX row kernels: bit-identical to the scalar oracle on these operands, tests/test_cpu_block_extremes.py)
    O.lib().orc_set_threads(min(16, os.cpu_count() or 1))
    yield
    O.lib().orc_set_fast(0)


def _launches():
    L = hooks_library().library
    L.rwkv_mi_test_mmq_fast_launches.restype = ctypes.c_uint64
    return int(L.rwkv_mi_test_mmq_fast_launches())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


_cache = {}


def _weights(t, K):
    if ("w", t, K) not in _cache:
        _cache[("w", t, K)] = B.weight_rows(t, K, SEED)
    return _cache[("w", t, K)]


def _operands(K, T):
    if ("x", K, T) not in _cache:
        _cache[("x", K, T)] = B.token_operands(K, T, SEED)
    return _cache[("x", K, T)]


def _wrong_codes(K, x):
    """Through the Q8_0 probe matrix: [(token, element, device d_x q_x, oracle d_x q_x)] of the activation codes the device got wrong."""
    got = gpu_mul_mat(B.Q8_0, B.probe_q8_0(K), K, K, x)
    out = []
    for i in range(x.shape[0]):
        q, d, _ = O.quantize_act(x[i])
        want = q.astype(np.float32) * np.repeat(d, 32)
        out += [(i, int(k), float(got[i, k]), float(want[k])) for k in np.nonzero(got[i] != want)[0]]
    return out


@pytest.mark.parametrize("T", TOKENS)
@pytest.mark.parametrize("K,N", SHAPES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_products_on_hand_built_blocks(fmt, K, N, T):
    t = B.QTYPES[fmt]
    wb, wnames = _weights(t, K)
    _, anames = B.activation_rows(K, SEED)
    ops = _operands(K, T)
    used, at = set(), {p: set() for p in {0, 31, 32, T - 1} if p < T}
    before = _launches()
    for r, (x, fam) in enumerate(ops):
        w, idx = B.take_rows(wb, t, K, r * N, N)
        used.update(int(i) for i in idx)
        for p in at:
            at[p].add(int(fam[p]))
        y, ref = gpu_mul_mat(t, w, K, N, x), O.mul_mat(t, w, K, N, x)
        assert np.isfinite(ref).all()
        bad = _bits(y) != _bits(ref)
        if bad.any():
            pairs = [(int(i), anames[fam[i]], wnames[idx[j]], float(y[i, j]), float(ref[i, j])) for i, j in zip(*np.nonzero(bad))]
            codes = _wrong_codes(K, x) if K <= 768 else "(probe not run at this K)"
            raise AssertionError((fmt, K, N, T, "rotation", r, int(bad.sum()), "outputs differ (token, activation family, weight row, device, oracle):",
                                  pairs[:8], "activation codes that differ (token, element, device, oracle):", codes if isinstance(codes, str) else codes[:8]))
    assert _launches() == before, "k_mmq_fast ran: not the exact arm"
    assert used == set(range(len(wnames))) and all(v == set(range(len(anames))) for v in at.values()), (len(used), len(wnames), at)


@pytest.mark.parametrize("fmt", ["Q4_0", "Q5_0"])
def test_exact_gemm_on_an_unsplit_grid(fmt):
    t, K, N, T = B.QTYPES[fmt], 768, 1024, 256
    wb, _ = _weights(t, K)
    w, _ = B.take_rows(wb, t, K, 0, N)
    x, _ = B.token_operands(K, T, SEED)[0]
    before = _launches()
    y, ref = gpu_mul_mat(t, w, K, N, x), O.mul_mat(t, w, K, N, x)
    assert _launches() == before
    assert np.array_equal(_bits(y), _bits(ref)), (fmt, int((_bits(y) != _bits(ref)).sum()))


@pytest.mark.parametrize("K,N,T", [(512, 256, 128), (2560, 136, 100)])
@pytest.mark.parametrize("fmt", FORMATS)
def test_plain_order_arm_on_hand_built_blocks(fmt, K, N, T):
    """k_mmq_fast within 1.5 (2 nb + 8) 2^-24 A of the oracle, A = |x_q|_2 |w_deq|_2 as in tests/test_gpu_prefill_fast.py, plus one term that
    bound leaves out. It rests on A >= sum_k |x_q[k]| |w_deq[k]| covering the size of every block term, which fails for an activation block
    whose fp16 d_x is 0 while its s_x is not (rows n1e-6 and n3e-8: s_x is rounded from the f32 product): there x_q = 0, A has nothing, and
    the terms m_w s_x are still added, in another order than the oracle's. With A alone the rows of Q4_1 with m = 65504 against n1e-6 gave
    |y - oracle| = 7.5e-9 under a bound of 1e-30. So for Q4_1 / Q5_1 the blocks with d_x = 0 add |s_x| |m_w| to A, and nothing else changes:
    every output with no such block has the bound of that file to the bit."""
    t = B.QTYPES[fmt]
    wb, _ = _weights(t, K)
    w, _ = B.take_rows(wb, t, K, 0, N)
    x, _ = B.token_operands(K, T, SEED)[3]
    ref = O.mul_mat(t, w, K, N, x)
    os.environ["RWKV_MI_SEQ_Q"] = "force"
    try:
        before = _launches()
        y = gpu_mul_mat(t, w, K, N, x)
        assert _launches() == before + 1, "k_mmq_fast did not run"
    finally:
        os.environ["RWKV_MI_SEQ_Q"] = "exact"
    rb = w.size // N
    wd = np.stack([O.dequantize_row(t, w[n * rb:(n + 1) * rb], K) for n in range(N)]).astype(np.float64)
    xq, dx, sx = np.empty((T, K)), np.empty((T, K // 32)), np.empty((T, K // 32))
    for i in range(T):
        q, dx[i], sx[i] = O.quantize_act(x[i])
        xq[i] = q.astype(np.float64) * np.repeat(dx[i], 32)
    A = np.sqrt((xq * xq).sum(axis=1))[:, None] * np.sqrt((wd * wd).sum(axis=1))[None, :]
    if t in B.HAS_M:
        _, _, mw = F.block_parts(t, w.tobytes(), K * N)
        A = A + np.where(dx == 0, np.abs(sx), 0.0) @ np.abs(mw.reshape(N, K // 32)).T
    bound = 1.5 * (2 * (K // 32) + 8) * 2.0 ** -24 * A + 1e-30
    assert np.isfinite(y).all()
    ratio = float((np.abs(y.astype(np.float64) - ref.astype(np.float64)) / bound).max())
    print("PLAIN-ORDER", fmt, K, N, T, f"ratio {ratio:.4f}")
    assert ratio <= 1.0, (fmt, K, N, T, ratio)
    before = _launches()
    assert np.array_equal(_bits(gpu_mul_mat(t, w, K, N, x)), _bits(ref))
    assert _launches() == before


@pytest.mark.parametrize("K", [64, 768, 2560])
def test_activation_quantiser_on_every_family(K):
    x, names = B.activation_rows(K, SEED)
    q, d, s, isum = gpu_quantize_act(x.reshape(-1))
    oq, od, os_ = O.quantize_act(x.reshape(-1))
    blocks = [f"{n}[{b}]" for n in names for b in range(K // 32)]
    held = np.abs(x.reshape(-1, 32)).max(axis=1) >= 2.0 ** -100
    nb = K // 32
    assert not held[names.index("n1e-40") * nb:][:nb].any() and all(held[names.index(n) * nb:][:nb].all() for n in names if n not in ("zeros", "negzero", "n1e-40"))
    for what, a, b in (("d", d, od), ("s", s, os_)):
        # values everywhere; bit patterns where the codes are defined (s_x = fp16(sum d): below, the sign of a zero s_x is the sign of an undefined sum)
        bad = np.nonzero((a != b) | (held & (_bits(a) != _bits(b))))[0]
        assert bad.size == 0, (what, [(blocks[i], float(a[i]), float(b[i])) for i in bad[:8]])
    bad = np.nonzero((q.reshape(-1, 32) != oq.reshape(-1, 32)).any(axis=1) & held)[0]
    assert bad.size == 0, ("q", [(blocks[i], q.reshape(-1, 32)[i].tolist(), oq.reshape(-1, 32)[i].tolist()) for i in bad[:3]])
    want = oq.reshape(-1, 32).astype(np.int32).sum(axis=1)
    assert np.array_equal(isum[held], want[held]), ("isum", [blocks[i] for i in np.nonzero((isum != want) & held)[0][:8]])


@pytest.mark.parametrize("T", [5, 65])
def test_probe_matrix_reads_back_the_activation_codes(T):
    """y[t][n] = d_x q_x[n]: k_quant_act (T = 5) and the tile quantiser (T = 65), every code of every family by position."""
    K = 768
    w = B.probe_q8_0(K)
    for x, _ in _operands(K, T)[::4]:
        y = gpu_mul_mat(B.Q8_0, w, K, K, x)
        for i in range(T):
            q, d, _ = O.quantize_act(x[i])
            want = q.astype(np.float32) * np.repeat(d, 32)
            bad = np.nonzero(y[i] != want)[0]      # (by value: the row sum of a -0 term and zeros is +0)
            assert bad.size == 0, (T, "token", i, [(int(k), float(y[i, k]), float(want[k])) for k in bad[:8]])


# ---------------------------------------------------------------------------------------------------------------------------------------
# model level (the four _check_* bodies and _Reference also serve tests/test_gpu_fx_extremes.py, on files whose F16 matrices are redrawn)
# ---------------------------------------------------------------------------------------------------------------------------------------

N_SEQ, CHUNK, N_ABI, N_GREEDY, FIRST = 40, 33, 4, 6, 5
SEG_LENS = (1, 33, 3)
N_PASSES = 2

SMALL = [(n, f, "palette", "k47" if ARCH_OF[n] in ("4", "7") else None) for n in ("test-v4", "test-v5.2", "test-v6", "test-v7") for f in ("Q4_0", "Q5_1")] + \
        [("test-v6", f, "palette", None) for f in ("Q4_1", "Q5_0", "Q8_0")]
BIG = [("mega-v6-2048", "Q4_0", "palette", "ring"), ("mega-v6-2048", "Q4_0", "palette", "regs"),
       ("slice-v7-2560", "Q5_1", "palette", "k47"), ("slice-v4-768", "Q5_1", "palette", "k47")]
CASES = [_case(*c) for c in SMALL + BIG]
IDS = ["-".join(c[:2]) + (f"-{c[3]}" if c[3] else "") for c in SMALL + BIG]


class _Reference:
    """What the oracle computes on one file from the fresh state, computed once and read by every test of the file."""

    def __init__(self, path):
        om = O.OracleModel(path)
        self.V = V = om.n_vocab
        self.fresh = om.init_state()
        self.tokens = S.lcg_tokens(V, N_SEQ)
        st, self.serial = self.fresh, []
        for t in self.tokens[:N_ABI]:
            lg, st = om.eval(t, st)
            self.serial.append((lg, st))
        self.seq = om.eval_sequence(self.tokens, self.fresh)
        st, tok, out = self.fresh, FIRST, []
        for _ in range(N_GREEDY):
            lg, st = om.eval(tok, st)
            tok = int(np.argmax(lg))
            out.append(tok)
        self.greedy = (out, st)
        self.rows = []
        for slot, n in enumerate(SEG_LENS):
            st, r = self.fresh, {"passes": []}
            for p in range(N_PASSES):
                lg, st = om.eval(_row_tokens(p, slot, 1, V)[0], st)
                r["passes"].append(lg)
            r["state_passes"] = st
            r["segment"] = _row_tokens(N_PASSES, slot, n, V)
            r["ragged"] = om.eval_sequence(r["segment"], st)
            self.rows.append(r)
        om.free()
        assert all(np.isfinite(lg).all() and np.isfinite(st).all() for lg, st in self.serial + [self.seq]), path
        self.fresh.setflags(write=False)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """(name, fmt, "palette") -> (path, _Reference): each file is written and redrawn once per module."""
    library()
    base, made = tmp_path_factory.mktemp("blocks"), {}

    def get(key):
        if key not in made:
            name, fmt, _ = key
            p = str(base / f"{name}-{fmt}-palette.bin")
            B.write_palette_model(synth, p, name, fmt, SEED)
            made[key] = (p, _Reference(p))
        return made[key]
    yield get
    for p, _ in made.values():
        os.remove(p)


@pytest.mark.parametrize("key,paths", CASES, ids=IDS)
def test_eval_on_palette_blocks_on_every_path(files, key, paths):
    _check_eval_on_every_path(*files(key), key, paths)


def _check_eval_on_every_path(path, ref, key, paths):
    for label, *_ in paths:
        m = _open(path, paths, label)
        st = None
        for i, (ol, ost) in enumerate(ref.serial):
            lg, st = m.eval(ref.tokens[i], st)
            _same(st, ost, key, label, i, "state")
            _same(lg, ol, key, label, i, "logits")
        assert m.healthy()
        m.free()


@pytest.mark.parametrize("key,paths", CASES, ids=IDS)
def test_decode_greedy_on_palette_blocks_on_every_path(files, key, paths):
    _check_decode_greedy_on_every_path(*files(key), key, paths)


def _check_decode_greedy_on_every_path(path, ref, key, paths):
    for label, *_ in paths:
        m = _open(path, paths, label)
        want, ost = ref.greedy
        m.state_load(ref.fresh.copy())
        toks, _ = m.decode_greedy(FIRST, N_GREEDY)
        assert list(toks) == want, (key, label, list(toks), want)
        _same(m.state_store(), ost, key, label, "state after decode_greedy")
        assert m.healthy()
        m.free()


@pytest.mark.parametrize("key,paths", CASES, ids=IDS)
def test_sequence_kernels_on_palette_blocks(files, key, paths):
    _check_sequence_kernels(*files(key), key, paths)


def _check_sequence_kernels(path, ref, key, paths):
    m = _open(path, paths, "top")
    ol, ost = ref.seq
    for what, (lg, st) in (("eval_sequence", m.eval_sequence(ref.tokens, None)),
                           ("eval_sequence_in_chunks", m.eval_sequence_in_chunks(ref.tokens, None, chunk_size=CHUNK))):
        _same(st, ost, key, what, "state")
        _same(lg, ol, key, what, "logits")
    m.free()


@pytest.mark.parametrize("key,paths", CASES, ids=IDS)
def test_rows_and_segments_on_palette_blocks(files, key, paths):
    _check_rows_and_segments(*files(key), key, paths)


def _check_rows_and_segments(path, ref, key, paths):
    m = _open(path, paths, "top")
    V, slots = ref.V, list(range(len(SEG_LENS)))
    b = pkg.RWKVBatch(m, len(slots))
    for s in slots:
        b.state_load(s, ref.fresh.copy())
    for p in range(N_PASSES):
        lg = b.eval(slots, [_row_tokens(p, s, 1, V)[0] for s in slots])
        for s in slots:
            _same(lg[s], ref.rows[s]["passes"][p], key, "eval pass", p, "slot", s)
    for s in slots:
        _same(b.state_store(s), ref.rows[s]["state_passes"], key, "state after the eval passes, slot", s)
    lg = b.eval_ragged(slots, [ref.rows[s]["segment"] for s in slots])
    for s in slots:
        _same(b.state_store(s), ref.rows[s]["ragged"][1], key, "state after eval_ragged, slot", s)
        _same(lg[s], ref.rows[s]["ragged"][0], key, "eval_ragged, slot", s)
    b.free()
    m.free()
