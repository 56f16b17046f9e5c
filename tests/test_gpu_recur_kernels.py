"""The recurrence kernels of csrc/kernels.hip and csrc/prefill.hip on caller-supplied arrays (lib/librwkv_testhooks_recur.so,
include/rwkv_testhooks_recur.h), at head sizes no model file can have, against the float32 rendering of the oracle's statements
(tests/recur_ref.py; tests/test_cpu_recur_ref.py holds that rendering to float64): np.array_equal on the outputs and on the whole out-state.
The out-buffers go in filled with a sentinel, so a slot no row or segment names, and a token no segment covers, must come back as they went in.

  launch_wkv6 / launch_wkv7   S in {8, 16, 20, 32, 40, 64, 96, 100, 128, 256, 320} (20, 100: no multiple of 8; 40, 96, 100: no power of two; 320:
                              the 256-thread loop of the generic bodies taken twice), H in {1, 3}; RWKV-5 / 6: (u_per_chan, w_mode) in
                              {(0, 0), (1, 1), (1, 2)}
     sequence                 T in {1, 2, 5}                                                                  k_wkvX<S>, k_wkvX_generic
     rows                     4 rows over 6 slots in a permuted order, two slots unused                       k_wkvX_rows<S>, k_wkvX_rows_generic
     segments                 9 tokens; segments of 1, 4 and 2 tokens that start at 2, 5 and 3, on slots 4, 0, 2  k_wkvX_segs<S>, k_wkvX_segs_generic
                              (templated: wkv6 S = 8, 16, 32, 64; wkv7 S = 32, 64; every other S generic)
  launch_wkvX_seq             S = 64, T in {32, 33, 64, 65, 97}, H in {1, 2, 5}: against the rendering and against launch_wkvX on the same input
  launch_groupnorm            the same S, T * H in {1, 5, 9} (a partial last workgroup of four waves), with and without the gate and the RWKV-7
                              bonus, eps 1e-5 and 64e-5                                                        k_groupnorm
  launch_v7_kprep             the same S and T * H                                                             k_v7_kprep
"""
import ctypes

import numpy as np
import pytest

import recur_ref as RR
from gpu_lib import RecurStates, recur_hooks_library

pytestmark = pytest.mark.gpu

F = np.float32
ARGS = 1 << 8   # RWKV_ERROR_ARGS
SIZES = (8, 16, 20, 32, 40, 64, 96, 100, 128, 256, 320)
HEADS = (1, 3)
MODES = ((0, 0), (1, 1), (1, 2))
SENTINEL = F(-777.25)
N_SLOTS = 6
# form -> (T, slots, t0, t1)
ROWS = (4, (3, 0, 5, 1), None, None)
SEGS = (9, (4, 0, 2), (2, 5, 3), (3, 9, 5))


def _L():
    return recur_hooks_library().library


def _p(a):
    return None if a is None else a.ctypes.data


def _c(a):
    return np.ascontiguousarray(a, dtype=F)


def _states(state_in, form, slots, t0, t1):
    """(struct, the arrays it points to -- state_out filled with the sentinel)"""
    keep = {"in": _c(state_in), "out": np.full(state_in.shape, SENTINEL, dtype=F), "slots": np.asarray(slots, dtype=np.uint32),
            "t0": None if t0 is None else np.asarray(t0, dtype=np.int32), "t1": None if t1 is None else np.asarray(t1, dtype=np.int32)}
    st = RecurStates(_p(keep["in"]), _p(keep["out"]), state_in.shape[0], form, len(slots), _p(keep["slots"]), _p(keep["t0"]), _p(keep["t1"]))
    return st, keep


def _gpu_wkv6(d, mode, state_in, form, slots, t0=None, t1=None):
    T, H, S = d["r"].shape
    u = _c(d["u_chan"] if mode[0] else d["u_head"])
    w = _c((d["w_head"], d["w_chan"], d["w_tok"])[mode[1]])
    st, keep = _states(state_in, form, slots, t0, t1)
    out = np.full((T, H, S), SENTINEL, dtype=F)
    ok = _L().rwkv_mi_test_wkv6(_p(d["r"]), _p(d["k"]), _p(d["v"]), _p(u), mode[0], _p(w), mode[1], ctypes.byref(st), _p(out), T, H, S)
    assert ok, "rwkv_mi_test_wkv6 failed"
    return out, keep["out"]


def _gpu_wkv7(d, state_in, form, slots, t0=None, t1=None):
    T, H, S = d["r"].shape
    st, keep = _states(state_in, form, slots, t0, t1)
    out = np.full((T, H, S), SENTINEL, dtype=F)
    ok = _L().rwkv_mi_test_wkv7(_p(d["r"]), _p(d["w7"]), _p(d["k"]), _p(d["v"]), _p(d["a"]), _p(d["b"]), ctypes.byref(st), _p(out), T, H, S)
    assert ok, "rwkv_mi_test_wkv7 failed"
    return out, keep["out"]


def _ref(arch, d, mode, state_in, form, slots, t0, t1):
    """the rendering of the same call: (out, state_out) with the sentinel wherever the call writes nothing"""
    T, H, S = d["r"].shape
    out, so = np.full((T, H, S), SENTINEL, dtype=F), np.full(state_in.shape, SENTINEL, dtype=F)
    ranges = [(0, T)] if form == 0 else [(t, t + 1) for t in range(T)] if form == 1 else list(zip(t0, t1))
    for slot, (a, b) in zip(slots, ranges):
        if arch == 6:
            u = d["u_chan"] if mode[0] else d["u_head"]
            w = (d["w_head"], d["w_chan"], d["w_tok"][a:b])[mode[1]]
            o, s = RR.wkv6(state_in[slot], d["r"][a:b], d["k"][a:b], d["v"][a:b], u, mode[0], w, mode[1], F)
        else:
            o, s = RR.wkv7(state_in[slot], *(d[x][a:b] for x in ("r", "w7", "k", "v", "a", "b")), F)
        out[a:b], so[slot] = o, s.reshape(-1)
    return out, so


def _same(got, want, *what):
    bad = got != want
    assert np.array_equal(got, want), what + (int(bad.sum()), "differ; first at", int(bad.reshape(-1).argmax()), float(got.reshape(-1)[bad.reshape(-1).argmax()]),
                                              float(want.reshape(-1)[bad.reshape(-1).argmax()]))


def _state_in(S, H, seed):
    return np.random.default_rng([seed, S, H]).standard_normal((N_SLOTS, H * S * S)).astype(F)


def _forms():
    for T in (1, 2, 5):
        yield "sequence", 0, T, (2,), None, None
    yield "rows", 1, ROWS[0], ROWS[1], None, None
    yield "segments", 2, SEGS[0], SEGS[1], SEGS[2], SEGS[3]


@pytest.mark.parametrize("H", HEADS)
@pytest.mark.parametrize("S", SIZES)
def test_wkv6_in_its_three_forms(S, H):
    state_in = _state_in(S, H, 11)
    for what, form, T, slots, t0, t1 in _forms():
        d = RR.draw(21, T, H, S)
        for mode in MODES:
            out, so = _gpu_wkv6(d, mode, state_in, form, slots, t0, t1)
            want_out, want_so = _ref(6, d, mode, state_in, form, slots, t0, t1)
            _same(so, want_so, "wkv6 state", what, "T", T, "S", S, "H", H, mode)
            _same(out, want_out, "wkv6 out", what, "T", T, "S", S, "H", H, mode)


@pytest.mark.parametrize("H", HEADS)
@pytest.mark.parametrize("S", SIZES)
def test_wkv7_in_its_three_forms(S, H):
    state_in = _state_in(S, H, 12)
    for what, form, T, slots, t0, t1 in _forms():
        d = RR.draw(22, T, H, S)
        out, so = _gpu_wkv7(d, state_in, form, slots, t0, t1)
        want_out, want_so = _ref(7, d, None, state_in, form, slots, t0, t1)
        _same(so, want_so, "wkv7 state", what, "T", T, "S", S, "H", H)
        _same(out, want_out, "wkv7 out", what, "T", T, "S", S, "H", H)


@pytest.mark.parametrize("H", (1, 2, 5))
@pytest.mark.parametrize("T", (32, 33, 64, 65, 97))
def test_wkv6_seq_is_the_rendering_and_the_per_head_kernel(T, H):
    S = 64
    d = RR.draw(23, T, H, S)
    state_in = _state_in(S, H, 13)
    for mode in MODES:
        u = _c(d["u_chan"] if mode[0] else d["u_head"])
        w = _c((d["w_head"], d["w_chan"], d["w_tok"])[mode[1]])
        out, so = np.full((T, H, S), SENTINEL, dtype=F), np.full(H * S * S, SENTINEL, dtype=F)
        sin = _c(state_in[1])
        assert _L().rwkv_mi_test_wkv6_seq(_p(d["r"]), _p(d["k"]), _p(d["v"]), _p(u), mode[0], _p(w), mode[1], _p(sin), _p(so), _p(out), T, H, S)
        want_out, want_so = _ref(6, d, mode, state_in, 0, (1,), None, None)
        _same(so, want_so[1], "wkv6_seq state", "T", T, "H", H, mode)
        _same(out, want_out, "wkv6_seq out", "T", T, "H", H, mode)
        k_out, k_so = _gpu_wkv6(d, mode, state_in, 0, (1,))
        _same(so, k_so[1], "wkv6_seq state against k_wkv6<64>", "T", T, "H", H, mode)
        _same(out, k_out, "wkv6_seq out against k_wkv6<64>", "T", T, "H", H, mode)


@pytest.mark.parametrize("H", (1, 2, 5))
@pytest.mark.parametrize("T", (32, 33, 64, 65, 97))
def test_wkv7_seq_is_the_rendering_and_the_per_head_kernel(T, H):
    S = 64
    d = RR.draw(24, T, H, S)
    state_in = _state_in(S, H, 14)
    out, so = np.full((T, H, S), SENTINEL, dtype=F), np.full(H * S * S, SENTINEL, dtype=F)
    sin = _c(state_in[1])
    assert _L().rwkv_mi_test_wkv7_seq(_p(d["r"]), _p(d["w7"]), _p(d["k"]), _p(d["v"]), _p(d["a"]), _p(d["b"]), _p(sin), _p(so), _p(out), T, H, S)
    want_out, want_so = _ref(7, d, None, state_in, 0, (1,), None, None)
    _same(so, want_so[1], "wkv7_seq state", "T", T, "H", H)
    _same(out, want_out, "wkv7_seq out", "T", T, "H", H)
    k_out, k_so = _gpu_wkv7(d, state_in, 0, (1,))
    _same(so, k_so[1], "wkv7_seq state against k_wkv7<64>", "T", T, "H", H)
    _same(out, k_out, "wkv7_seq out against k_wkv7<64>", "T", T, "H", H)


@pytest.mark.parametrize("S", SIZES)
def test_groupnorm(S):
    for T, H in ((1, 1), (5, 1), (3, 3)):
        d = RR.draw(25, T, H, S)
        bonus = (d["k"], d["r"], d["v"], d["r_k"])
        for eps in (1e-5, 64e-5):
            for gate in (None, d["gate"]):
                for v7 in (None, bonus):
                    x = d["x"].copy()
                    args = [_p(x), _p(d["lw"]), _p(d["lb"]), eps, _p(gate)] + [_p(a) for a in (v7 or (None,) * 4)]
                    assert _L().rwkv_mi_test_groupnorm(*args, T, H, S), "rwkv_mi_test_groupnorm failed"
                    want = RR.group_norm(d["x"], d["lw"], d["lb"], eps, F, gate=gate, v7=v7)
                    _same(x, want, "groupnorm", "S", S, "T", T, "H", H, "eps", eps, "gate", gate is not None, "bonus", v7 is not None)


@pytest.mark.parametrize("S", SIZES)
def test_v7_kprep(S):
    for T, H in ((1, 1), (5, 1), (3, 3)):
        d = RR.draw(26, T, H, S)
        outs = [np.full((T, H, S), SENTINEL, dtype=F) for _ in range(3)]
        assert _L().rwkv_mi_test_v7_kprep(_p(d["k"]), _p(d["gate"]), _p(d["k_k"]), _p(d["k_a"]), *[_p(o) for o in outs], T, H, S), "rwkv_mi_test_v7_kprep failed"
        want = RR.v7_kprep(d["k"], d["gate"], d["k_k"], d["k_a"], F)
        for name, got, w in zip(("k'", "-kk", "kk a"), outs, want):
            _same(got, w, "v7_kprep", name, "S", S, "T", T, "H", H)


def test_refusals_launch_nothing():
    L = recur_hooks_library()
    T, H = 33, 1
    # the lane-pipelined forms exist for S = 64 only, from 32 tokens on
    for S, T_ in ((32, T), (96, T), (64, 31)):
        d = RR.draw(27, T_, H, S)
        sin, so, out = _c(_state_in(S, H, 15)[0]), np.full(H * S * S, SENTINEL, dtype=F), np.full((T_, H, S), SENTINEL, dtype=F)
        assert not L.library.rwkv_mi_test_wkv6_seq(_p(d["r"]), _p(d["k"]), _p(d["v"]), _p(d["u_chan"]), 1, _p(d["w_tok"]), 2, _p(sin), _p(so), _p(out), T_, H, S)
        assert L.rwkv_get_last_error(None) & ARGS
        assert not L.library.rwkv_mi_test_wkv7_seq(_p(d["r"]), _p(d["w7"]), _p(d["k"]), _p(d["v"]), _p(d["a"]), _p(d["b"]), _p(sin), _p(so), _p(out), T_, H, S)
        assert L.rwkv_get_last_error(None) & ARGS
        assert (so == SENTINEL).all() and (out == SENTINEL).all()
    # a slot named twice, a slot out of range, a segment past T, overlapping segments, rows that are not T
    S, T = 16, 9
    d = RR.draw(28, T, H, S)
    state_in = _state_in(S, H, 16)
    for form, slots, t0, t1 in ((2, (1, 1), (0, 3), (3, 5)), (2, (1, 6), (0, 3), (3, 5)), (2, (1, 2), (0, 3), (3, 10)), (2, (1, 2), (0, 3), (4, 5)),
                                (1, (0, 1, 2), None, None), (0, (0, 1), None, None)):
        st, keep = _states(state_in, form, slots, t0, t1)
        out = np.full((T, H, S), SENTINEL, dtype=F)
        assert not L.library.rwkv_mi_test_wkv7(_p(d["r"]), _p(d["w7"]), _p(d["k"]), _p(d["v"]), _p(d["a"]), _p(d["b"]), ctypes.byref(st), _p(out), T, H, S)
        assert L.rwkv_get_last_error(None) & ARGS, (form, slots, t0, t1)
        assert (keep["out"] == SENTINEL).all() and (out == SENTINEL).all()
