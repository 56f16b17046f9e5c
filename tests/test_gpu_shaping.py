"""Typical-p and top-n-sigma in the device sampler (rwkv_mi_*shaping_set, csrc/sampling.hip sigma_floor / typical_stage / cut_sample): the
kept set and the token are held, bit for bit, to the truncating sampler on logits masked on the host by tests/shape_ref.py (float64), on the
table of cases tests/test_cpu_shaping.py has shown clear of every f32 decision; the public interface to a host loop of passes and the hook
on the downloaded logits."""
import ctypes

import numpy as np
import pytest

import reference_constants as R
import shape_ref as S
from gpu_lib import library, model, pkg
from test_gpu_batch import _tok
from test_gpu_truncation import _cut_rows, _fresh

pytestmark = pytest.mark.gpu

ARGS = 1 << 8   # RWKV_ERROR_ARGS
US = (0.02, 0.3, 0.5, 0.77, 0.98)
NONE = (0, 0.0, 0.0, 0.0)

_hooks = None


def _shape_rows(logits, params, settings, counters, rows_kernel, want_weights=False):
    """rwkv_mi_test_shape_rows (lib/librwkv_testhooks_shape.so): tokens [rows], counters after, weights [rows][n_vocab] or None"""
    global _hooks
    if _hooks is None:
        library()   # (builds; and HIP is initialised in the order gpu_lib keeps)
        _hooks = pkg.RWKVSharedLibrary(pkg.SHAPE_HOOKS_LIB_PATH)
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    n_rows, n_vocab = logits.shape
    table = (pkg.ShapeParams * n_rows)(*[pkg.ShapeParams(int(k), float(mp), float(tp), float(ns)) for k, mp, tp, ns in settings])
    ctr = None if counters is None else np.ascontiguousarray(counters, dtype=np.uint64).copy()
    out = np.empty(n_rows, dtype=np.uint32)
    w = np.empty((n_rows, n_vocab), dtype=np.float32) if want_weights else None
    ok = _hooks.library.rwkv_mi_test_shape_rows(logits.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), n_rows, n_vocab, params, table,
                                                None if ctr is None else ctr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), rows_kernel,
                                                out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                                None if w is None else w.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    assert ok, "rwkv_mi_test_shape_rows failed"
    return out, ctr, w


@pytest.mark.parametrize("rows_kernel", [1, 0])
@pytest.mark.parametrize("name,row", S.cases(), ids=[c[0] for c in S.cases()])
def test_kept_set_and_token_are_the_sampler_on_host_masked_logits(name, row, rows_kernel):
    """One launch of the row kernel (or one context launch per row) over the same row of logits under every setting of the table, one row
    with no setting -- the plain draw -- and one with temperature 0, which ignores its setting."""
    settings = S.SETTINGS + [NONE, (0, 0.0, 0.2, 1.0)]
    n = len(settings)
    T = [1.0, 0.8] * (n // 2) + [0.0]
    P = [1.0, 1.0, 0.9] * (n // 3) + [1.0] * (n - 3 * (n // 3))
    logits = np.tile(row, (n, 1))
    want = np.stack([S.kept(row, k, tp, ns) for k, _, tp, ns in settings[:-1]] + [np.ones(row.size, dtype=bool)])
    ref_logits = np.where(want, logits, S.NEG).astype(np.float32)
    assert want[n - 2].all() and not want[:n - 2].all(axis=1).any(), "every setting of the table cuts something"
    for i, u in enumerate(US):
        table = pkg.sample_params(n, T, P, float(u), 0)
        got, _, w = _shape_rows(logits, table, settings, None, rows_kernel, want_weights=(i == 0))
        # (top-k is in the mask already; min-p is the body's in both draws)
        ref, _, rw = _cut_rows(ref_logits, table, [(0, mp) for _, mp, _, _ in settings], None, rows_kernel, want_weights=(i == 0))
        assert np.array_equal(got, ref), (name, rows_kernel, u, got.tolist(), ref.tolist())
        assert want[np.arange(n), got].all(), (name, rows_kernel, u, got.tolist())
        if w is not None:
            assert np.array_equal(w[:-1] > 0.0, rw[:-1] > 0.0), (name, rows_kernel, [(int((a > 0).sum()), int((b > 0).sum())) for a, b in zip(w, rw)])
            assert not (w[:-1] > 0.0)[~want[:-1]].any() and (w[:-1] > 0.0).any(axis=1).all()
    assert int(got[-1]) == int(np.argmax(row)), "a row with temperature 0 is the argmax, whatever its setting"


def _host_loop(b, slots, first, n, T, P, seeds, settings):
    """n passes of eval with the logits downloaded; each row's token from the hook on them, its draw counter the step: tokens [rows][n]"""
    out = np.empty((len(slots), n), dtype=np.uint32)
    feed = list(first)
    for j in range(n):
        lg = b.eval(slots, feed)
        got, _, _ = _shape_rows(lg, pkg.sample_params(len(slots), T, P, -1.0, seeds), settings, np.full(len(slots), j, dtype=np.uint64), 1)
        out[:, j] = got
        feed = [int(t) for t in got]
    return out


def test_through_the_public_interface(golden_dir):
    m = model(R.fixture_path(golden_dir, "6v0-3m", "Q5_0"))
    V = m.n_vocab
    b, twin = pkg.RWKVBatch(m, 2), pkg.RWKVBatch(m, 2)
    slots, T, P, seeds = [0, 1], [1.0, 0.9], [1.0, 0.95], [41, 42]
    first = [_tok(3, s, V) for s in slots]
    shape = (0.625, 1.5)
    assert b.shaping(0) == (0.0, 0.0) and m.shaping() == (0.0, 0.0)
    b.set_shaping(0, *shape)
    assert b.shaping(0) == shape and b.shaping(1) == (0.0, 0.0)

    def start(x):
        return _fresh(m, x, slots, V, 1)

    # the loop: the shaped slot is the host loop with the hook, the other slot the run with no setting anywhere
    st = start(b)
    loop, _ = b.decode_sample(slots, first, 8, T, P, seeds)
    start(twin)
    plain, _ = twin.decode_sample(slots, first, 8, T, P, seeds)
    start(twin)
    host = _host_loop(twin, slots, first, 8, T, P, seeds, [(0, 0.0, *shape), NONE])
    assert np.array_equal(loop, host), (loop.tolist(), host.tolist())
    assert np.array_equal(loop[1], plain[1]) and not np.array_equal(loop[0], plain[0]), (loop.tolist(), plain.tolist())
    # a context with the setting: the same loop from slot 0's state
    m.state_load(st[0])
    m.set_shaping(*shape)
    assert m.shaping() == shape
    alone, _ = m.decode_sample(first[0], 8, T[0], P[0], seeds[0])
    assert np.array_equal(alone, loop[0]), (alone.tolist(), loop[0].tolist())
    c = m.clone()
    assert c.shaping() == (0.0, 0.0), "a cloned context starts with none"
    c.free()
    m.set_shaping(0.0, 0.0)
    # eval_draft, sampled: a draft that stands and one that fails in the middle emit what the loop emitted
    start(b)
    drafts = [[int(t) for t in loop[0][:4]], [int(loop[1][0]), (int(loop[1][1]) + 1) % V, int(loop[1][2])]]
    emitted, lens = b.eval_draft(slots, [[first[i]] + drafts[i] for i in range(2)], params=pkg.sample_params(2, T, P, -1.0, seeds))
    assert lens.tolist() == [5, 2] and all(list(emitted[i]) == [int(t) for t in loop[i][:lens[i]]] for i in range(2)), (lens.tolist(), emitted, loop.tolist())
    twin.free()
    b.free()
    m.free()


def test_rejections_change_nothing(golden_dir):
    m = model(R.fixture_path(golden_dir, "6v0-3m", "Q5_0"))
    b = pkg.RWKVBatch(m, 2)
    b.set_shaping(1, 0.875, 2.0)
    m.set_shaping(0.5, 0.0)
    for slot, tp, ns in ((1, 1.5, 0.0), (1, -0.1, 0.0), (1, float("nan"), 0.0), (1, 0.5, -1.0), (1, 0.5, float("nan")), (1, 0.5, float("inf")), (2, 0.5, 1.0)):
        b.last_error = 0
        with pytest.raises(ValueError):
            b.set_shaping(slot, tp, ns)
        assert b.last_error & ARGS, (slot, tp, ns, b.last_error)
    for tp, ns in ((1.0001, 0.0), (float("nan"), 1.0), (0.5, -0.5), (0.5, float("nan"))):
        with pytest.raises(ValueError):
            m.set_shaping(tp, ns)
        assert m.last_error & ARGS, (tp, ns)
    with b.serve_open([0], pkg.SERVE_SAMPLE):
        b.last_error = 0
        with pytest.raises(ValueError):
            b.set_shaping(1, 0.3, 0.0)
        assert b.last_error & ARGS
    assert b.shaping(1) == (0.875, 2.0) and b.shaping(0) == (0.0, 0.0) and m.shaping() == (0.5, 0.0)
    b.set_shaping(1, 1.0, 0.0)   # (typical_p = 1 is accepted: none)
    m.set_shaping(0.0, 0.0)
    b.free()
    m.free()
