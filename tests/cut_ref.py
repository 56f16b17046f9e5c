"""The truncation settings of the device sampler (rwkv_mi_*truncation_set: top-k and min-p), restated on the host in NumPy / float64: what
tests/test_gpu_truncation.py holds the device to. The order is mask -> softmax -> top-p and min-p, intersected -> temperature.

top-k is a mask on the VALUES the draw reads (float32, compared as such): the tokens are ranked by (value descending, index ascending), a
NaN never ranks, -inf ranks last, +0 and -0 are equal; everything outside the first k reads -inf. k == 0 or k >= n: no top-k."""
import numpy as np


def rank_order(values_f32):
    """The indices of the values that rank, in the order (value descending, index ascending); NaNs are left out."""
    v = np.asarray(values_f32, dtype=np.float32)
    idx = np.flatnonzero(~np.isnan(v))
    return idx[np.argsort(-v[idx].astype(np.float64), kind="stable")]


def top_k_mask(values_f32, k):
    """bool [n]: the tokens whose value the draw reads as it is. Exact."""
    v = np.asarray(values_f32, dtype=np.float32)
    n = v.size
    if k == 0 or k >= n:
        return np.ones(n, dtype=bool)
    keep = np.zeros(n, dtype=bool)
    keep[rank_order(v)[:k]] = True
    return keep


def masked(values_f32, k):
    """The values the draw reads under top_k = k: float32, -inf outside the mask."""
    v = np.asarray(values_f32, dtype=np.float32)
    return np.where(top_k_mask(v, k), v, np.float32(-np.inf)).astype(np.float32)


def ref_distribution_cut(logits, temperature, top_p, top_k, min_p):
    """The probabilities the draw is taken from, float64 [n]: test_gpu_sampling.ref_distribution with the two truncations."""
    x = masked(logits, top_k).astype(np.float64)
    x = x - x.max()
    e = np.exp(x)
    probs = e / e.sum()
    if top_p == 0.0:
        top_p = 1.0
    if temperature == 0.0:
        out = np.zeros_like(probs)
        out[int(np.argmax(probs))] = 1.0
        return out
    keep = np.ones(probs.size, dtype=bool)
    if top_p < 1.0:
        sp = np.sort(probs)[::-1]
        keep &= probs >= float(sp[np.argmax(np.cumsum(sp) > top_p)])
    if min_p != 0.0:
        keep &= probs >= float(min_p) * probs.max()
    probs = np.where(keep, probs, 0.0)
    if temperature != 1.0:
        probs = np.power(probs, 1.0 / temperature)
    return probs / probs.sum()


def ratios(logits):
    """exp(l - max) of the values that are neither NaN nor -inf, float64, sorted ascending: p / p_max of every token with a probability."""
    x = np.asarray(logits, dtype=np.float32).astype(np.float64)
    x = x[np.isfinite(x)]
    return np.sort(np.exp(x - x.max()))


def min_p_in_a_gap(logits, target):
    """A min_p (as the float32 the kernel receives) near `target` that no token's p / p_max is near: the geometric midpoint of the first
    gap between two neighbouring ratios, from the one that holds the target upwards, whose ends differ by more than 2e-4 relative (so the
    result can lie below the target by less than that one gap). None when there is no such gap (all values equal)."""
    r = ratios(logits)
    i = max(int(np.searchsorted(r, target)), 1)
    while i < r.size:
        lo, hi = r[i - 1], r[i]
        if lo > 0.0 and hi / lo - 1.0 > 2e-4:
            return float(np.float32(np.sqrt(lo * hi)))
        i += 1
    return None


def clearance(logits, min_p):
    """How far, relative, the nearest p / p_max is from min_p."""
    return float(np.abs(ratios(logits) / float(min_p) - 1.0).min())
