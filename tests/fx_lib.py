"""Hand-built operands of the UNQUANTISED products (F16 / F32 matrices): weight rows and activation rows that reach every end of binary16 and
binary32, the counterpart of tests/blocks_lib.py for k_mvf, k_mmfx_seq and k_mmf16_seq (csrc/kernels.hip). TEST INFRASTRUCTURE ONLY
(tests/test_cpu_fx_extremes.py holds the oracle to an exact emulation on everything made here, tests/test_gpu_fx_extremes.py holds the GPU
products to the oracle; the model-level palette of F16 elements is blocks_lib.f16_palette).

A weight ROW is one family of K elements, and so is an activation row. Patterns that depend on the position are functions of k % 32 (the
partial sum of ggml's order an element belongs to) and k // 32 (its link in that chain; four links are one 128-element step of k_mmfx_seq), so
a family sits differently in the 32 chains and in the steps.

  weight rows      weight_rows(type, K, seed): F16_FAMILIES for an F16 matrix, + F32_ONLY for an F32 one, + four `mixed` rows (a family per
                   32-element run)
  activation rows  activation_rows(K, seed), f32; token_operands rotates them over the tokens exactly as blocks_lib.token_operands does
  probe            probe(type, K): the K x K identity; y[t][n] is what the product made of x[t][n]

Declared NON-FINITE families (the only ones whose outputs may be inf or NaN, asserted per output in tests/test_cpu_fx_extremes.py): the weight
row `huge`; the activation rows `r65520`, `inf`, `nan`; and `big` under F16 weights, where 1e30 rounds to inf. Everything else stays finite at
every K used. NaN payloads and signs are outside what is held: NaN is compared by position.
"""
import numpy as np

import f64_model as F
from blocks_lib import SUB, _rng

F16, F32 = F.F16, F.F32
DTYPE = {F16: np.float16, F32: np.float32}
TYPE_NAMES = {"FP16": F16, "FP32": F32}
H_MAX = 65504.0

F16_FAMILIES = ("zeros", "negzero", "+sub", "-sub", "maxsub", "subrand", "minnorm", "+1", "-1", "+max", "-max", "altmax", "alt32max", "ramp",
                "lowbits", "normal", "spike")
F32_ONLY = ("denorm", "tiny", "negtiny", "allbits", "huge")
N_MIXED = 4
NONFINITE_WEIGHTS = ("huge",)
NONFINITE_ACTS = {F16: ("r65520", "inf", "nan", "big"), F32: ("r65520", "inf", "nan")}


def families(type_id):
    return F16_FAMILIES + (F32_ONLY if type_id == F32 else ())


def _family_row(type_id, family, K, row, rng):
    """K elements of one family, float64 (every value exact in the type), or uint32 bit patterns for `allbits`."""
    k = np.arange(K)
    const = {"zeros": 0.0, "negzero": -0.0, "+sub": SUB, "-sub": -SUB, "maxsub": 1023 * SUB, "minnorm": 2.0 ** -14, "+1": 1.0, "-1": -1.0,
             "+max": H_MAX, "-max": -H_MAX, "tiny": 1e-30, "negtiny": -1e-30, "huge": 3e38}
    if family in const:
        return np.full(K, const[family])
    if family == "subrand":
        return rng.integers(1, 1024, size=K) * SUB * np.where(rng.random(K) < 0.5, -1.0, 1.0)
    if family == "altmax":
        return np.where(k % 2 == 0, H_MAX, -H_MAX)
    if family == "alt32max":                                         # every chain k % 32 alternates along k: it cancels link by link
        return np.where((k // 32) % 2 == 0, H_MAX, -H_MAX)
    if family == "ramp":
        return 2.0 ** ((k % 30) - 24.0)
    if family == "lowbits":
        return 1.0 + ((37 * (k % 32) + k // 32) % 1024) * 2.0 ** -10
    if family == "normal":
        return 0.05 * rng.standard_normal(K)
    if family == "spike":
        v = np.zeros(K)
        v[(7 * row) % K] = -1.5
        return v
    if family == "denorm":
        return 1e-40 * rng.standard_normal(K)
    assert family == "allbits", family
    bits = (rng.integers(0, 2, size=K).astype(np.uint32) << 31) | ((127 + rng.integers(-20, 21, size=K)).astype(np.uint32) << 23) | 0x7FFFFF
    return bits.view(np.float32).astype(np.float64)


def weight_rows(type_id, K, seed):
    """(w (R, K) np.float16 / np.float32, names): one row per family of the type, then N_MIXED rows that draw a FINITE family per 32-element
    run. The payload of a call is take_rows(w, ...) viewed as bytes."""
    rng = _rng(seed, "fx-weights", type_id, K)
    names = list(families(type_id))
    rows = [_family_row(type_id, f, K, r, rng) for r, f in enumerate(names)]
    pool = [f for f in names if f not in NONFINITE_WEIGHTS and f != "spike"]
    for r in range(N_MIXED):
        v = np.empty(K)
        for b in range(K // 32):
            v[32 * b:32 * b + 32] = _family_row(type_id, pool[rng.integers(len(pool))], K, r, rng)[32 * b:32 * b + 32]
        rows.append(v)
        names.append(f"mixed{r}")
    with np.errstate(under="ignore"):
        w = np.stack(rows).astype(DTYPE[type_id])
    if type_id == F16:
        assert np.array_equal(w.astype(np.float64)[:len(F16_FAMILIES) - 2], np.stack(rows)[:len(F16_FAMILIES) - 2])   # all but normal / spike: exact in binary16
    return w, names


def take_rows(w, start, N):
    """N rows of a weight_rows matrix from row `start` on, cyclically: (payload bytes uint8, row indices)."""
    idx = (start + np.arange(N)) % w.shape[0]
    return np.ascontiguousarray(w[idx]).view(np.uint8).reshape(-1), idx


def probe(type_id, K):
    """The K x K identity as payload bytes: y[t][n] = fp16(x[t][n]) (F16) or x[t][n] (F32), so a rounding edge shows by its position."""
    return np.eye(K, dtype=DTYPE[type_id]).view(np.uint8).reshape(-1)


def activation_rows(K, seed):
    """(x float32 (R, K), names): one row per family.

      zeros     +0.0                                   negzero  runs of -0.0, of N(0, 1), and of -0.0 / +0.0 alternating, in turn
      normal    N(0, 1)                                n1e-3    N(0, 1) 1e-3: binary16 subnormals of many steps among them
      n6e-8     N(0, 1) 6e-8: straddles 2^-25, where binary16 rounds to 0 or to 2^-24 (and 2^-25 itself, a tie, at k % 32 == 9)
      ties      1 + (k mod 4) 2^-11: exact, tie to even down, exact, tie to even up
      max       65504                                  r65519   +-65519 by element: the largest f32 that rounds to 65504, not to inf
      alt2000   +-2000 alternating by element          spike    one non-zero element per run, at position b mod 32, signs alternating
      denorm    N(0, 1) 1e-40: f32 denormals           negtiny  -1e-30: against 1e-30 every product underflows to -0
      big       1e30 (F16 weights: inf)                r65520   65520, the smallest f32 that rounds to inf, negative at k % 3 == 0
      inf       +inf                                   nan      N(0, 1) with one NaN per run, at position b mod 32
    """
    nb, rng = K // 32, _rng(seed, "fx-activations", K)
    n = lambda: rng.standard_normal((nb, 32))                        # noqa: E731
    j, b = np.arange(32), np.arange(nb)
    k = np.arange(K).reshape(nb, 32)
    sign = np.where(j % 2 == 0, 1.0, -1.0)
    rows = {"zeros": np.zeros((nb, 32))}
    z = n()
    z[b % 3 == 0] = -0.0
    z[b % 3 == 2] = np.where(j % 2 == 0, -0.0, 0.0)
    rows["negzero"] = z
    rows["normal"], rows["n1e-3"] = n(), n() * 1e-3
    e = n() * 6e-8
    e[:, 9] = 2.0 ** -25 * np.where(b % 2 == 0, 1.0, -1.0)
    rows["n6e-8"] = e
    rows["ties"] = 1.0 + (k % 4) * 2.0 ** -11
    rows["max"] = np.full((nb, 32), H_MAX)
    rows["r65519"] = np.broadcast_to(65519.0 * sign, (nb, 32)).copy()
    rows["alt2000"] = np.broadcast_to(2000.0 * sign, (nb, 32)).copy()
    s = np.zeros((nb, 32))
    s[b, b % 32] = np.where(b % 2 == 0, 1.0, -1.0) * 3.7 * (1 + b % 7)
    rows["spike"] = s
    rows["denorm"] = n() * 1e-40
    rows["negtiny"] = np.full((nb, 32), -1e-30)
    rows["big"] = np.full((nb, 32), 1e30)
    rows["r65520"] = np.where(k % 3 == 0, -65520.0, 65520.0)
    rows["inf"] = np.full((nb, 32), np.inf)
    g = n()
    g[b, b % 32] = np.nan
    rows["nan"] = g
    with np.errstate(under="ignore"):
        x = np.stack([v.reshape(-1) for v in rows.values()]).astype(np.float32)
    return x, list(rows)


def token_operands(K, T, seed):
    """As blocks_lib.token_operands: one operand per rotation r of the R activation rows, token t of operand r holding row (t + r) mod R.
    Returns [(x (T, K), family index of every token)]."""
    rows, _ = activation_rows(K, seed)
    R = rows.shape[0]
    return [(np.ascontiguousarray(rows[(np.arange(T) + r) % R]), (np.arange(T) + r) % R) for r in range(R)]


def round_trip_f16(x):
    """fp16(x) as f32, by NumPy's cast (round to nearest even, subnormals kept, overflow to inf)."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


def float64_sum(type_id, w, x):
    """(sum_k w[n][k] x'[t][k], sum_k |w[n][k] x'[t][k]|) in float64, x' = fp16(x) under F16 weights: the reference and the size A of the
    project's bound 2e-6 A + 1e-30 (tests/test_gpu_seq_f16.py). Rows with a non-finite operand give non-finite figures."""
    xs = (round_trip_f16(x) if type_id == F16 else np.asarray(x, dtype=np.float32)).astype(np.float64)
    wd = np.asarray(w).astype(np.float64)
    with np.errstate(all="ignore"):
        return xs @ wd.T, np.abs(xs) @ np.abs(wd).T
