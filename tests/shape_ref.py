"""The shaping settings of the device sampler (rwkv_mi_*shaping_set: typical-p and top-n-sigma), restated on the host in NumPy / float64: what
tests/test_gpu_shaping.py holds the device to. The order of a draw is n-sigma floor -> top-k -> typical-p -> softmax -> top-p and min-p ->
temperature; everything from the softmax on is the sampler's and is not restated here.

Beside the two cuts, two plain measures of how far a case lies from a decision the device takes in f32 (the clearances), and the table of
cases the device is held to, which tests/test_cpu_shaping.py checks against them without a GPU."""
import numpy as np

import cut_ref as C

NEG = np.float32(-np.inf)


def n_sigma_floor(values_f32, n_sigma):
    """M - n_sigma * sigma over the finite values (the population's standard deviation); -inf when none is finite."""
    v = np.asarray(values_f32, dtype=np.float32).astype(np.float64)
    v = v[np.isfinite(v)]
    if v.size == 0:
        return -np.inf
    return float(v.max() - float(n_sigma) * np.sqrt(np.mean((v - v.mean()) ** 2)))


def n_sigma_mask(values_f32, n_sigma):
    """bool [n]: the values the floor leaves as they are. n_sigma == 0: all; else a NaN is never kept."""
    v = np.asarray(values_f32, dtype=np.float32)
    if n_sigma == 0.0:
        return np.ones(v.size, dtype=bool)
    with np.errstate(invalid="ignore"):
        return v.astype(np.float64) >= n_sigma_floor(v, n_sigma)


def typical_keys(values_f32):
    """(p, s) in float64: the softmax of the values (a NaN reads -inf) and the keys |-ln p - H|, inf where p is 0."""
    w = np.asarray(values_f32, dtype=np.float32).astype(np.float64)
    w = np.where(np.isnan(w), -np.inf, w)
    e = np.exp(w - w.max())
    p = e / e.sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        lnp = np.log(p)
        H = -np.sum(np.where(p > 0.0, p * lnp, 0.0))
        s = np.where(p > 0.0, np.abs(-lnp - H), np.inf)
    return p, s


def _crossing(values_f32, typical_p):
    """(keys ascending without repeats, the mass at or below each, the index of S* among them or None)"""
    p, s = typical_keys(values_f32)
    keys = np.unique(s)
    mass = np.array([p[s <= k].sum() for k in keys])
    over = np.flatnonzero(mass > typical_p)
    return keys, mass, (int(over[0]) if over.size else None)


def typical_mask(values_f32, typical_p):
    """bool [n]: the values the typical stage leaves as they are. typical_p == 0 or 1: all."""
    v = np.asarray(values_f32, dtype=np.float32)
    if not (0.0 < typical_p < 1.0) or not np.isfinite(np.nanmax(np.where(np.isnan(v), -np.inf, v))):
        return np.ones(v.size, dtype=bool)
    keys, _, at = _crossing(v, typical_p)
    if at is None:
        return np.ones(v.size, dtype=bool)
    return typical_keys(v)[1] <= keys[at]


def kept(values_f32, top_k, typical_p, n_sigma):
    """bool [n]: the tokens whose value the body reads as it is, after floor -> top-k -> typical-p."""
    v = np.asarray(values_f32, dtype=np.float32)
    keep = n_sigma_mask(v, n_sigma)
    keep &= C.top_k_mask(np.where(keep, v, NEG), top_k)
    keep &= typical_mask(np.where(keep, v, NEG), typical_p)
    return keep


def masked(values_f32, top_k, typical_p, n_sigma):
    """The values the body reads: float32, -inf outside the kept set."""
    v = np.asarray(values_f32, dtype=np.float32)
    return np.where(kept(v, top_k, typical_p, n_sigma), v, NEG).astype(np.float32)


def floor_clearance(values_f32, n_sigma):
    """The relative gap between the floor and the nearest finite value on either side (inf: no floor)."""
    if n_sigma == 0.0:
        return np.inf
    v = np.asarray(values_f32, dtype=np.float32).astype(np.float64)
    f = n_sigma_floor(values_f32, n_sigma)
    return float(np.abs(v[np.isfinite(v)] - f).min() / abs(f))


def typical_clearance(values_f32, typical_p):
    """(the gap between typical_p and the cumulative mass on either side of the crossing, the relative gap between S* and the next key);
    (inf, inf) when the stage is off."""
    if not (0.0 < typical_p < 1.0):
        return np.inf, np.inf
    keys, mass, at = _crossing(values_f32, typical_p)
    before = mass[at - 1] if at else 0.0
    nxt = keys[at + 1] if at + 1 < keys.size else np.inf
    return float(min(typical_p - before, mass[at] - typical_p)), float(1.0 if np.isinf(nxt) else (nxt - keys[at]) / nxt)


# ---- the cases of tests/test_gpu_shaping.py ----

HAND = np.log(np.array([0.4, 0.3, 0.15, 0.1, 0.05])).astype(np.float32)
GAUSS = (np.random.default_rng(20).standard_normal(24) * 2.0).astype(np.float32)
FAR = np.float32(-30.0)   # "far below": finite, so it enters the n-sigma statistics, with no mass a float can hold beside the row's
VOCABS = (5, 1025, 65536)   # below one chunk of the 1024 threads, a ragged last chunk, the full vocabulary
# (top_k, min_p, typical_p, n_sigma): typical-p alone, n-sigma alone, both -- each plain, with top-k 3 and with min-p
SETTINGS = [(k, mp, tp, ns) for tp, ns in ((0.5, 0.0), (0.0, 1.0), (0.75, 1.5)) for k, mp in ((0, 0.0), (3, 0.0), (0, 0.1))]


def embed(base, n_vocab, fill):
    """The row [n_vocab]: the first values of `base` that fit, spread evenly from token 0 to the last one, `fill` everywhere else."""
    vals = base[:min(base.size, n_vocab)]
    row = np.full(n_vocab, fill, dtype=np.float32)
    row[np.linspace(0, n_vocab - 1, vals.size).astype(np.int64)] = vals
    return row


def cases():
    """[(name, row)]: the hand vector and the Gaussian row at every vocabulary, the rest (there is none at 5) -inf and far below."""
    out = []
    for bname, base in (("hand", HAND), ("gauss", GAUSS)):
        out.append((f"{bname}-{VOCABS[0]}", embed(base, VOCABS[0], NEG)))
        out += [(f"{bname}-{V}-{fname}", embed(base, V, fill)) for V in VOCABS[1:] for fname, fill in (("inf", NEG), ("far", FAR))]
    return out


def case_clearances(row, setting):
    """(floor, mass, key) clearances of one row under one setting, each stage on what the stages before it leave."""
    top_k, _, tp, ns = setting
    v = np.where(n_sigma_mask(row, ns), row, NEG)
    v = C.masked(v, top_k)
    return (floor_clearance(row, ns), *typical_clearance(v, tp))
