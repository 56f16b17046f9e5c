"""Plain numpy renderings of the recurrences of the CPU oracle (oracle/rwkv_oracle.c), statement for statement: wkv6_token, wkv7_token,
group_norm / norm_row(np = 64) with the RWKV-7 bonus and the gate, and the RWKV-7 key preparation of att_v7. TEST INFRASTRUCTURE ONLY (a helper
module; tests/test_cpu_recur_ref.py holds the float32 rendering to the float64 one, tests/test_gpu_recur_kernels.py holds the kernels to the
float32 one bit for bit).

Every function takes the precision `dt`. With dt = numpy.float32 every operation rounds to float32, as the oracle's C statements do and as
the kernels do (both are built with -ffp-contract=off: no fused multiply-add); the partial sums of norm_row are doubles in the oracle and
stay doubles. With dt = numpy.float64 the same statements are the high-precision side. The loops over the independent index (the value
column of wkv6, the value row of wkv7, the rows of a norm) are numpy vectors; the loops whose order the oracle fixes (the key index of a
sum, the 64 partial sums and their halving tree) are Python loops in that order."""
import numpy as np

NP = 64   # partial sums of a per-head reduction: element j goes to partial j % 64 (one per lane of a wave), folded by a halving tree


def _fold(ps):
    """fold_d / fold_f over the last axis of ps [..., 64]"""
    ps = ps.copy()
    o = ps.shape[-1] // 2
    while o > 0:
        ps[..., :o] = ps[..., :o] + ps[..., o:2 * o]
        o //= 2
    return ps[..., 0]


def _partials(x, acc):
    """ps[j % 64] += x[..., j], j ascending, in the precision `acc`"""
    ps = np.zeros(x.shape[:-1] + (NP,), dtype=acc)
    for c in range(0, x.shape[-1], NP):
        chunk = x[..., c:c + NP].astype(acc)
        ps[..., :chunk.shape[-1]] = ps[..., :chunk.shape[-1]] + chunk
    return ps


def wkv6_token(state, r, k, v, u, w, dt):
    """wkv6_token on state [H][S(i: key)][S(j: value)], changed in place; r, k, v, u, w: [H][S] (a per-head u or w repeated along S). -> out [H][S]"""
    H, S = r.shape
    o = np.zeros((H, S), dtype=dt)
    for i in range(S):
        kv = v * k[:, i:i + 1]
        prev = state[:, i, :].copy()
        temp = kv * u[:, i:i + 1] + prev
        o = o + temp * r[:, i:i + 1]
        state[:, i, :] = prev * w[:, i:i + 1] + kv
    return o


def wkv6(state, r, k, v, u, u_per_chan, w, w_mode, dt):
    """tokens [0, T) of one sequence. r, k, v: [T][H][S]; u: [H] or [H][S]; w: [H], [H][S] or [T][H][S]. -> (out [T][H][S], state afterwards)"""
    T, H, S = r.shape
    c = lambda x: np.asarray(x).astype(dt)   # noqa: E731
    state, r, k, v = c(state).reshape(H, S, S).copy(), c(r), c(k), c(v)
    u = c(u).reshape(H, S) if u_per_chan else np.repeat(c(u).reshape(H, 1), S, axis=1)
    w = c(w).reshape(T, H, S) if w_mode == 2 else c(w).reshape(H, S) if w_mode == 1 else np.repeat(c(w).reshape(H, 1), S, axis=1)
    out = np.empty((T, H, S), dtype=dt)
    for t in range(T):
        out[t] = wkv6_token(state, r[t], k[t], v[t], u, w[t] if w_mode == 2 else w, dt)
    return out, state


def wkv7_token(state, r, w, k, v, a, b, dt):
    """wkv7_token on state [H][S(i: value)][S(j: key)], changed in place; the six inputs [H][S]. -> out [H][S]"""
    H, S = r.shape
    sa = np.zeros((H, S), dtype=dt)
    for j in range(S):
        sa = sa + a[:, j:j + 1] * state[:, :, j]
    res = np.zeros((H, S), dtype=dt)
    for j in range(S):
        kv = v * k[:, j:j + 1]
        ns = (state[:, :, j] * w[:, j:j + 1] + kv) + sa * b[:, j:j + 1]
        state[:, :, j] = ns
        res = res + ns * r[:, j:j + 1]
    return res


def wkv7(state, r, w, k, v, a, b, dt):
    """tokens [0, T) of one sequence, every input [T][H][S]. -> (out [T][H][S], state afterwards)"""
    T, H, S = r.shape
    c = lambda x: np.asarray(x).astype(dt)   # noqa: E731
    state, r, w, k, v, a, b = c(state).reshape(H, S, S).copy(), c(r), c(w), c(k), c(v), c(a), c(b)
    out = np.empty((T, H, S), dtype=dt)
    for t in range(T):
        out[t] = wkv7_token(state, r[t], w[t], k[t], v[t], a[t], b[t], dt)
    return out, state


def group_norm(x, lw, lb, eps, dt, gate=None, v7=None):
    """group_norm (norm_row(np = 64), * ln_x.w + ln_x.b), then the RWKV-7 bonus (v7 = (k, r, v [T][H][S], r_k [H][S]): + v * sum_head(k r r_k))
    and the gate. x: [T][H][S]; lw, lb: [H][S]. -> y [T][H][S]"""
    c = lambda z: np.asarray(z).astype(dt)   # noqa: E731
    acc = np.float64
    x, lw, lb = c(x), c(lw), c(lb)
    n = x.shape[-1]
    mean = (_fold(_partials(x, acc)) / acc(n)).astype(dt)[..., None]
    d = x - mean
    variance = (_fold(_partials(d * d, acc)) / acc(n)).astype(dt)[..., None]
    scale = dt(1.0) / np.sqrt(variance + dt(eps))
    y = d * scale
    y = y * lw
    y = y + lb
    if v7 is not None:
        vk, vr, vv, rk = (c(z) for z in v7)
        s = _fold(_partials((vk * vr) * rk, dt))[..., None]
        y = y + vv * s
    if gate is not None:
        y = y * c(gate)
    return y


def v7_kprep(k, a, k_k, k_a, dt):
    """the key path of att_v7: kk = l2norm_head(k * k_k); k' = k + (a * k * k_a - k * k_a). k, a: [T][H][S]; k_k, k_a: [H][S].
    -> (k', -kk, kk * a)"""
    c = lambda z: np.asarray(z).astype(dt)   # noqa: E731
    k, a, k_k, k_a = c(k), c(a), c(k_k), c(k_a)
    t = k * k_k
    s = _fold(_partials(t * t, dt))[..., None]
    scale = dt(1.0) / np.maximum(np.sqrt(s), dt(1e-12))
    kk = t * scale
    ka = k * k_a
    return k + (a * ka - ka), -kk, kk * a


# ---- inputs as a model would produce them ----

def draw(seed, T, H, S):
    """r, k, v ~ N(0, 1) / sqrt(S); decays in (0, 1) with exact 0 and 1 entries; kk of unit norm per head, a gate in (0, 1); states ~ N(0, 1).
    Every array float32; the per-token ones [T][H][S], the vectors [H][S] (and [H] for the per-head forms)."""
    rng = np.random.default_rng([int(seed), T, H, S])
    f = np.float32
    n = lambda *shape: rng.standard_normal(shape).astype(f)   # noqa: E731
    d = {x: n(T, H, S) / f(np.sqrt(S)) for x in ("r", "k", "v")}
    for name, shape in (("w_tok", (T, H, S)), ("w_chan", (H, S)), ("w_head", (H,))):
        w = rng.uniform(0.0, 1.0, shape).astype(f)
        flat = w.reshape(-1)
        flat[0::5], flat[1::7] = 0.0, 1.0
        d[name] = w
    d["w_head"][...] = rng.uniform(0.5, 1.0, (H,)).astype(f)
    if H > 1:
        d["w_head"][0] = 1.0
    d["u_chan"], d["u_head"] = n(H, S), n(H)
    kk = n(T, H, S)
    kk = (kk / np.sqrt((kk.astype(np.float64) ** 2).sum(-1, keepdims=True))).astype(f)
    gate = rng.uniform(0.0, 1.0, (T, H, S)).astype(f)
    d["a"], d["b"], d["gate"] = -kk, kk * gate, gate
    d["w7"] = np.exp(-0.606531 * rng.uniform(0.0, 1.0, (T, H, S))).astype(f)
    d["w7"].reshape(-1)[1::7] = 1.0
    d["lw"], d["lb"], d["k_k"], d["k_a"], d["r_k"] = rng.uniform(-3.0, 3.0, (H, S)).astype(f), n(H, S), n(H, S), rng.uniform(0.0, 1.0, (H, S)).astype(f), n(H, S)
    d["x"] = n(T, H, S)
    return d
