"""tests/recur_ref.py without a GPU: its vector statements are the oracle's scalar loops, its float32 rendering is held to its float64 one,
and the hook library tests/test_gpu_recur_kernels.py drives exports exactly what include/rwkv_testhooks_recur.h declares.

Criterion of tests/test_cpu_f64_reference.py, its FP32 gate unchanged: e = max |f32 - f64| / (1 + max |f64|) <= TOL["FP32"] = 1e-4, on the
outputs and on the state, with the inputs of recur_ref.draw (r, k, v ~ N(0, 1) / sqrt(S), decays in (0, 1) with exact 0 and 1 entries,
a = -kk with |kk| = 1, states ~ N(0, 1)). No cell needed narrower inputs; the worst figures are in the tests' docstrings.

Not here: the float32 rendering against the oracle's own state after one token of an S = 96 file (every recurrence input recomputed from the
file). tests/test_gpu_head_sizes.py ties the kernels to the oracle on whole files, tests/test_gpu_recur_kernels.py ties them to this rendering.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import recur_ref as RR
from test_cpu_f64_reference import TOL, _err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = {"rwkv_mi_test_wkv6": 12, "rwkv_mi_test_wkv7": 11, "rwkv_mi_test_wkv6_seq": 13, "rwkv_mi_test_wkv7_seq": 12,
         "rwkv_mi_test_groupnorm": 12, "rwkv_mi_test_v7_kprep": 10}
SIZES = (8, 20, 64, 96, 100, 320)
F = np.float32


def _pkg():
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    pkg = graft.load_package()
    pkg.build_library()
    return pkg


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"RWKV_API[^;(]*?\b(rwkv_\w+)\s*\(([^;]*)\)\s*;", text)}


def test_only_the_recur_library_exports_the_hooks():
    pkg = _pkg()
    lib_dir = os.path.dirname(pkg.LIB_PATH)
    path = os.path.join(lib_dir, "librwkv_testhooks_recur.so")
    for other in (pkg.LIB_PATH, pkg.HOOKS_LIB_PATH, pkg.SAMPLE_HOOKS_LIB_PATH, pkg.GUIDE_HOOKS_LIB_PATH, pkg.CUT_HOOKS_LIB_PATH, pkg.DECAY_HOOKS_LIB_PATH):
        so = ctypes.CDLL(other)
        for hook in HOOKS:
            assert not hasattr(so, hook), (other, hook)
    declared = _declared("rwkv_testhooks_recur.h")
    assert set(declared) == set(HOOKS)
    for hook, n_args in HOOKS.items():
        assert len(declared[hook].split(",")) == n_args, hook
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert exported == set(_declared("rwkv.h")) | set(_declared("rwkv_mi355x.h")) | set(HOOKS)


# ---- the vector statements are the scalar loops ----

def _wkv6_scalar(state, r, k, v, u, w):
    """wkv6_token of oracle/rwkv_oracle.c, one head, float32 scalars"""
    S = r.size
    o = np.zeros(S, dtype=F)
    for i in range(S):
        for j in range(S):
            kv = F(v[j] * k[i])
            prev = state[i, j]
            temp = F(F(kv * u[i]) + prev)
            o[j] = F(o[j] + F(temp * r[i]))
            state[i, j] = F(F(prev * w[i]) + kv)
    return o


def _wkv7_scalar(state, r, w, k, v, a, b):
    S = r.size
    out = np.zeros(S, dtype=F)
    for i in range(S):
        sa = F(0.0)
        for j in range(S):
            sa = F(sa + F(a[j] * state[i, j]))
        res = F(0.0)
        for j in range(S):
            kv = F(v[i] * k[j])
            ns = F(F(F(state[i, j] * w[j]) + kv) + F(sa * b[j]))
            state[i, j] = ns
            res = F(res + F(ns * r[j]))
        out[i] = res
    return out


def test_vector_statements_are_the_scalar_loops():
    S, H = 5, 2
    d = RR.draw(1, 1, H, S)
    st = np.random.default_rng(2).standard_normal((H, S, S)).astype(F)
    a, b = st.copy(), st.copy()
    got = RR.wkv6_token(a, d["r"][0], d["k"][0], d["v"][0], d["u_chan"], d["w_tok"][0], F)
    want = np.stack([_wkv6_scalar(b[h], d["r"][0, h], d["k"][0, h], d["v"][0, h], d["u_chan"][h], d["w_tok"][0, h]) for h in range(H)])
    assert np.array_equal(got, want) and np.array_equal(a, b)
    a, b = st.copy(), st.copy()
    got = RR.wkv7_token(a, d["r"][0], d["w7"][0], d["k"][0], d["v"][0], d["a"][0], d["b"][0], F)
    want = np.stack([_wkv7_scalar(b[h], d["r"][0, h], d["w7"][0, h], d["k"][0, h], d["v"][0, h], d["a"][0, h], d["b"][0, h]) for h in range(H)])
    assert np.array_equal(got, want) and np.array_equal(a, b)


def test_partial_sums_follow_the_oracle_order():
    """element j to partial j % 64, ascending; then the halving tree 32, 16, .. 1 -- on values whose float32 sum depends on the order"""
    x = np.zeros(130, dtype=F)
    x[0], x[64], x[128] = 1.0, 2.0 ** -24, 2.0 ** -24      # partial 0: (1 + 2^-24) + 2^-24 = 1 in float32, not 1 + 2^-23
    x[32] = -1.0                                            # the first fold adds partial 32 to partial 0
    x[1] = 2.0 ** -30
    assert RR._fold(RR._partials(x[None], F))[0] == F(2.0 ** -30)
    assert RR._fold(RR._partials(x[None], np.float64))[0] == 2.0 ** -23 + 2.0 ** -30
    ps = np.arange(64, dtype=np.float64)[None]
    want = ps[0].copy()
    for o in (32, 16, 8, 4, 2, 1):
        want[:o] += want[o:2 * o]
    assert RR._fold(ps)[0] == want[0] == 2016.0


# ---- float32 against float64 ----

@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("mode", [(0, 0), (1, 1), (1, 2)], ids=["head", "chan", "token"])
def test_wkv6_float32_against_float64(S, mode):
    """worst e measured over these cells: 4.3e-7 (out, S = 320, per head) and 1.5e-7 (state)"""
    T, H = 5, 3
    d = RR.draw(3, T, H, S)
    st = np.random.default_rng(4).standard_normal((H, S, S)).astype(F)
    u = d["u_chan"] if mode[0] else d["u_head"]
    w = (d["w_head"], d["w_chan"], d["w_tok"])[mode[1]]
    o32, s32 = RR.wkv6(st, d["r"], d["k"], d["v"], u, mode[0], w, mode[1], F)
    o64, s64 = RR.wkv6(st, d["r"], d["k"], d["v"], u, mode[0], w, mode[1], np.float64)
    assert o32.dtype == F and s32.dtype == F and o64.dtype == np.float64
    print("RECUR wkv6", S, mode, f"out {_err(o32, o64):.1e} state {_err(s32, s64):.1e}")
    assert _err(o32, o64) <= TOL["FP32"] and _err(s32, s64) <= TOL["FP32"]


@pytest.mark.parametrize("S", SIZES)
def test_wkv7_float32_against_float64(S):
    """worst e measured over these cells: 4.5e-7 (out, S = 320) and 1.2e-7 (state)"""
    T, H = 5, 3
    d = RR.draw(5, T, H, S)
    st = np.random.default_rng(6).standard_normal((H, S, S)).astype(F)
    args = (st, d["r"], d["w7"], d["k"], d["v"], d["a"], d["b"])
    o32, s32 = RR.wkv7(*args, F)
    o64, s64 = RR.wkv7(*args, np.float64)
    assert o32.dtype == F and s32.dtype == F
    print("RECUR wkv7", S, f"out {_err(o32, o64):.1e} state {_err(s32, s64):.1e}")
    assert _err(o32, o64) <= TOL["FP32"] and _err(s32, s64) <= TOL["FP32"]


@pytest.mark.parametrize("S", SIZES)
def test_group_norm_and_kprep_float32_against_float64(S):
    """worst e measured over these cells: 1.6e-7 (group norm, S = 8, gate, eps 64e-5) and 3.1e-8 (key preparation)"""
    T, H = 3, 3
    d = RR.draw(7, T, H, S)
    errs = {}
    for what, kw in (("plain", {}), ("gate", {"gate": d["gate"]}), ("bonus", {"v7": (d["k"], d["r"], d["v"], d["r_k"])}),
                     ("bonus+gate", {"gate": d["gate"], "v7": (d["k"], d["r"], d["v"], d["r_k"])})):
        for eps in (1e-5, 64e-5):
            y32, y64 = RR.group_norm(d["x"], d["lw"], d["lb"], eps, F, **kw), RR.group_norm(d["x"], d["lw"], d["lb"], eps, np.float64, **kw)
            assert y32.dtype == F
            errs[(what, eps)] = _err(y32, y64)
    k32, k64 = RR.v7_kprep(d["k"], d["gate"], d["k_k"], d["k_a"], F), RR.v7_kprep(d["k"], d["gate"], d["k_k"], d["k_a"], np.float64)
    for name, a, b in zip(("k'", "-kk", "kk a"), k32, k64):
        assert a.dtype == F
        errs[name] = _err(a, b)
    print("RECUR norm", S, " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= TOL["FP32"], errs
