"""The reference of the log-prob report's ordering (tests/test_cpu_logprobs.py checks it on a hand-written row, tests/test_gpu_logprobs.py
holds the device to it): the top_n logits that are not NaN, by value descending, then by index ascending."""
import numpy as np

NO_TOKEN = 0xFFFFFFFF


def top_ids(logits, top_n):
    """uint32 [top_n]: np.lexsort((index, -logit))[:top_n] over the entries that are not NaN (-inf ranks last among them, -0 ties with +0),
    padded with NO_TOKEN where fewer rank."""
    l = np.asarray(logits, dtype=np.float32)
    index = np.flatnonzero(~np.isnan(l))
    order = index[np.lexsort((index, -l[index]))][:top_n]
    out = np.full(top_n, NO_TOKEN, dtype=np.uint32)
    out[:order.size] = order
    return out


def f64_logprobs(logits, ids):
    """float64 on the f32 logits: l[id] - (m + log(sum(exp(l - m)))) for each id; -inf for NO_TOKEN."""
    l = np.asarray(logits, dtype=np.float32).astype(np.float64)
    m = np.nanmax(l) if not np.isnan(l).all() else np.nan
    with np.errstate(all="ignore"):
        lse = m + np.log(np.exp(l - m).sum())
        return np.array([-np.inf if int(i) == NO_TOKEN else l[int(i)] - lse for i in ids], dtype=np.float64)
