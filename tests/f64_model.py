"""An independent float64 forward pass of the rwkv.cpp model file (architectures 4, 5.1, 5.2, 6 and 7). TEST INFRASTRUCTURE ONLY.

The CPU oracle (oracle/rwkv_oracle.c) restates ggml's f32 arithmetic in one fixed order, and the GPU kernels are held to it bit for bit;
this module is the yardstick for the oracle itself and for the arms that are not bit-identical to anything. It shares no code with the
oracle: its own file reader, its own NumPy dequantiser of Q4_0 / Q4_1 / Q5_0 / Q5_1 / Q8_0 (F16 and F32 widened exactly), and the graph of
the reference restated in NumPy (rwkv_graph.inc:84-543, rwkv_operators.inc:40-97, rwkv_operators_wkv_v7.inc:37-107, ggml_rwkv_wkv6).
Everything is computed in float64; the projections of all T tokens are one matmul, only the token shift and the recurrences loop over tokens.

What ggml's mul_mat does to its operands is kept, because it is part of what the model computes:
  * F16 weights: the activation is rounded to fp16 first (ggml converts src1 to the weight's vec_dot_type); products and sums in float64.
  * quantised weights: the activation is quantised per 32-block to Q8_0 (Q4_0 / Q5_0 / Q8_0 weights) or Q8_1 (Q4_1 / Q5_1): the codes q_x,
    the fp16 scale d_x and the fp16 block sum s_x come from ``oracle_lib.quantize_act`` -- the ONE step shared with the oracle (that
    quantiser is pinned bit-exact to the GPU's by test_activation_quantiser_bit_exact). The product is then formed in float64:
    y = sum_b d_w d_x isum_b (+ m_w s_x), evaluated as sum_k (d_w q_w[k]) (d_x q_x[k]) + sum_b m_w s_x (each term exact in float64).

``wrong=`` selects deliberately wrong RWKV-7 variants (each per-head reduction taken over the whole vector) that exist only to show
that the tests built on this module can tell a per-head reduction from a whole-vector one:
  "kk"   -- kk l2-normalised over D,   "r_k" -- the r_k bonus summed over D,   "ln_x" -- ln_x normalised as one group.
"""
import struct

import numpy as np

import oracle_lib as O

F32, F16, Q4_0, Q4_1, Q5_0, Q5_1, Q8_0 = 0, 1, 2, 3, 7, 8, 9
BLOCK_BYTES = {Q4_0: 18, Q4_1: 20, Q5_0: 22, Q5_1: 24, Q8_0: 34}
WRONG_VARIANTS = ("kk", "r_k", "ln_x")


def _f16(b):
    """fp16 bytes (..., 2) -> float64, exact."""
    return np.ascontiguousarray(b).view(np.float16)[..., 0].astype(np.float64)


def block_parts(type_id, raw, n):
    """Decodes n elements of a quantised payload: (codes q (n//32, 32) float64, scale d (n//32,), offset m (n//32,) or None).
    The element value is q * d (+ m)."""
    bb = BLOCK_BYTES[type_id]
    blk = np.frombuffer(raw, dtype=np.uint8, count=(n // 32) * bb).reshape(-1, bb)
    d = _f16(blk[:, 0:2].copy())
    m = None
    if type_id in (Q4_1, Q5_1):
        m = _f16(blk[:, 2:4].copy())
    if type_id == Q8_0:
        return blk[:, 2:34].copy().view(np.int8).astype(np.float64), d, m
    pos = {Q4_0: 2, Q4_1: 4, Q5_0: 6, Q5_1: 8}[type_id]
    qs = blk[:, pos:pos + 16].astype(np.int64)
    q = np.concatenate([qs & 0x0F, qs >> 4], axis=1)            # element j: low nibble of byte j; element 16 + j: high nibble of byte j
    if type_id in (Q5_0, Q5_1):
        qh = blk[:, pos - 4:pos].copy().view("<u4")[:, 0].astype(np.int64)
        q |= ((qh[:, None] >> np.arange(32)) & 1) << 4        # bit j of qh is the fifth bit of element j
    if type_id in (Q4_0, Q5_0):
        q -= 8 if type_id == Q4_0 else 16
    return q.astype(np.float64), d, m


def dequantize(type_id, raw, n):
    """The payload as float64 values (F32 / F16 widened exactly; blocks as q * d (+ m))."""
    if type_id == F32:
        return np.frombuffer(raw, dtype="<f4", count=n).astype(np.float64)
    if type_id == F16:
        return np.frombuffer(raw, dtype="<f2", count=n).astype(np.float64)
    q, d, m = block_parts(type_id, raw, n)
    y = q * d[:, None]
    if m is not None:
        y = y + m[:, None]
    return y.reshape(-1)


def _type_bytes(type_id, n):
    return n * 4 if type_id == F32 else n * 2 if type_id == F16 else (n // 32) * BLOCK_BYTES[type_id]


def read_file(path):
    """rwkv.cpp file: header (magic, version, n_vocab, n_embed, n_layer, data type), then per tensor: n_dims, key length, type, dims, key,
    payload. Returns (header dict, {name: (type, dims, raw bytes)})."""
    with open(path, "rb") as f:
        blob = f.read()
    magic, version, n_vocab, n_embed, n_layer, data_type = struct.unpack_from("<6I", blob, 0)
    assert magic == 0x67676D66, "not an rwkv.cpp file"
    hdr = dict(version=version, n_vocab=n_vocab, n_embed=n_embed, n_layer=n_layer, data_type=data_type)
    tensors, p = {}, 24
    while p < len(blob):
        nd, kl, ty = struct.unpack_from("<3I", blob, p)
        p += 12
        dims = struct.unpack_from(f"<{nd}I", blob, p)
        p += 4 * nd
        name = blob[p:p + kl].decode()
        p += kl
        nb = _type_bytes(ty, int(np.prod(dims)))
        tensors[name] = (ty, tuple(dims), memoryview(blob)[p:p + nb])
        p += nb
    return hdr, tensors


class _Matrix:
    """A 2-D weight (ggml dims (K, N): N rows of K) as ggml's mul_mat sees it."""

    def __init__(self, ty, dims, raw):
        self.type, (self.K, self.N) = ty, dims
        if ty in (F32, F16):
            self.w = dequantize(ty, raw, self.K * self.N).astype(np.float32).reshape(self.N, self.K)   # exact in f32
            self.m = None
        else:
            q, d, m = block_parts(ty, raw, self.K * self.N)
            self.w = (q * d[:, None]).astype(np.float32).reshape(self.N, self.K)  # d_w q_w: <= 19 significant bits, exact in f32
            self.m = None if m is None else m.reshape(self.N, self.K // 32)

    def __call__(self, x):
        """x (T, K) float64 -> (T, N) float64."""
        x = np.asarray(x, dtype=np.float64).reshape(-1, self.K)
        if self.type == F32:
            return x @ self.w.T.astype(np.float64)
        if self.type == F16:
            xh = x.astype(np.float32).astype(np.float16).astype(np.float64)
            return xh @ self.w.T.astype(np.float64)
        xq = np.empty_like(x)
        sx = np.empty((x.shape[0], self.K // 32))
        for t in range(x.shape[0]):
            q, d, s = O.quantize_act(x[t].astype(np.float32))
            xq[t] = (q.astype(np.float64).reshape(-1, 32) * d.astype(np.float64)[:, None]).reshape(-1)
            sx[t] = s
        y = xq @ self.w.T.astype(np.float64)
        if self.m is not None:
            y += sx @ self.m.T
        return y


def _layer_norm(x, w, b, eps=1e-5):
    mu = x.mean(axis=-1, keepdims=True)
    c = x - mu
    return c / np.sqrt((c * c).mean(axis=-1, keepdims=True) + eps) * w + b


def _norm(x, eps):
    mu = x.mean(axis=-1, keepdims=True)
    c = x - mu
    return c / np.sqrt((c * c).mean(axis=-1, keepdims=True) + eps)


def _sigmoid(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def _shift(xn, carry):
    """x_prev of every token: the carried vector, then the sequence shifted by one."""
    return np.concatenate([carry[None, :], xn[:-1]], axis=0)


class F64Model:
    def __init__(self, path, wrong=None):
        assert wrong in (None,) + WRONG_VARIANTS, wrong
        self.wrong = wrong
        hdr, t = read_file(path)
        self.n_vocab, self.n_embed, self.n_layer = hdr["n_vocab"], hdr["n_embed"], hdr["n_layer"]
        self._t = t
        # architecture by the tensors present (rwkv_model_loading.inc)
        if "blocks.0.att.r_k" in t:
            self.arch = (7, 0)
        elif "blocks.0.att.time_maa_x" in t:
            self.arch = (6, 0)
        elif "blocks.0.att.ln_x.weight" in t:
            self.arch = (5, 2 if "blocks.0.att.gate.weight" in t else 1)
        else:
            self.arch = (4, 0)
        D = self.n_embed
        if self.arch[0] == 7:
            self.head_count = t["blocks.0.att.r_k"][1][1]
        elif self.arch[0] >= 5:
            self.head_count = t["blocks.0.att.time_decay"][1][-1]
        else:
            self.head_count = 0
        self.head_size = D // self.head_count if self.head_count else 0
        self.per_layer = D * (2 + self.head_size) if self.arch[0] >= 5 else 5 * D
        self.state_len = self.per_layer * self.n_layer
        self._mats = {}
        self._vecs = {}

    # parameters, decoded on first use
    def vec(self, name):
        if name not in self._vecs:
            ty, dims, raw = self._t[name]
            self._vecs[name] = dequantize(ty, raw, int(np.prod(dims)))
        return self._vecs[name]

    def mat(self, name):
        if name not in self._mats:
            ty, dims, raw = self._t[name]
            self._mats[name] = _Matrix(ty, dims, raw)
        return self._mats[name]

    def has(self, name):
        return name in self._t

    def init_state(self):
        s = np.zeros(self.state_len)
        if self.arch[0] == 4:
            s.reshape(self.n_layer, 5, self.n_embed)[:, 4] = float(np.float32(-1e30))   # pp: -1e30f (rwkv_eval.inc:224-241)
        return s

    def eval(self, token, state_in):
        logits, state = self.forward([token], state_in)
        return logits[-1], state

    def eval_sequence(self, tokens, state_in):
        logits, state = self.forward(tokens, state_in, all_logits=False)
        return logits[-1], state

    def forward(self, tokens, state_in, all_logits=True):
        """Runs the tokens from state_in (None: the initial state). Returns (logits (T, V) -- or (1, V) of the last token when not
        all_logits --, state) in float64; the state in the oracle's layout."""
        D = self.n_embed
        state = self.init_state() if state_in is None else np.array(state_in, dtype=np.float64)
        emb_ty, _, emb_raw = self._t["emb.weight"]
        row_bytes = _type_bytes(emb_ty, D)
        x = np.stack([dequantize(emb_ty, emb_raw[tok * row_bytes:(tok + 1) * row_bytes], D) for tok in tokens])
        x = _layer_norm(x, self.vec("blocks.0.ln0.weight"), self.vec("blocks.0.ln0.bias"))
        self._v_first = None
        for i in range(self.n_layer):
            st = state[i * self.per_layer:(i + 1) * self.per_layer]
            x = x + getattr(self, f"_att_v{self.arch[0]}")(i, x, st)
            x = x + self._ffn(i, x, st)
        if not all_logits:
            x = x[-1:]
        xo = _layer_norm(x, self.vec("ln_out.weight"), self.vec("ln_out.bias"))
        return self.mat("head.weight")(xo), state

    # time mixing (rwkv_graph.inc:84-482); st is the layer's slice of the state, updated in place
    def _carry(self, i, x, st, ln, off):
        D = self.n_embed
        xn = _layer_norm(x, self.vec(f"blocks.{i}.{ln}.weight"), self.vec(f"blocks.{i}.{ln}.bias"))
        xp = _shift(xn, st[off * D:(off + 1) * D].copy())
        st[off * D:(off + 1) * D] = xn[-1]
        return xn, xp

    def _lerp(self, i, xn, xp, name):
        mix = self.vec(f"blocks.{i}.{name}")
        return xn * mix + (xp - xp * mix)

    def _att_v4(self, i, x, st):
        D, p = self.n_embed, f"blocks.{i}.att."
        xn, xp = self._carry(i, x, st, "ln1", 1)
        r = _sigmoid(self.mat(p + "receptance.weight")(self._lerp(i, xn, xp, "att.time_mix_r")))
        k = self.mat(p + "key.weight")(self._lerp(i, xn, xp, "att.time_mix_k"))
        v = self.mat(p + "value.weight")(self._lerp(i, xn, xp, "att.time_mix_v"))
        tf, td = self.vec(p + "time_first"), self.vec(p + "time_decay")
        aa, bb, pp = st[2 * D:3 * D].copy(), st[3 * D:4 * D].copy(), st[4 * D:5 * D].copy()
        wkv = np.empty_like(k)
        for t in range(k.shape[0]):
            ww = tf + k[t]
            qq = np.maximum(pp, ww)
            e1, e2 = np.exp(pp - qq), np.exp(ww - qq)
            wkv[t] = (e1 * aa + e2 * v[t]) / (e1 * bb + e2)
            ww = pp + td
            qq = np.maximum(ww, k[t])
            e1, e2 = np.exp(ww - qq), np.exp(k[t] - qq)
            aa, bb, pp = e1 * aa + e2 * v[t], e1 * bb + e2, qq
        st[2 * D:3 * D], st[3 * D:4 * D], st[4 * D:5 * D] = aa, bb, pp
        return self.mat(p + "output.weight")(r * wkv)

    def _wkv6(self, st, r, k, v, u, w):
        """ggml_rwkv_wkv6: per head, S[i][j] (i: key, j: value); out_j = sum_i r_i (u_i k_i v_j + S_ij); S_ij <- S_ij w_i + k_i v_j.
        u (H, S); w (T, H, S)."""
        D, H, S = self.n_embed, self.head_count, self.head_size
        s = st[2 * D:].reshape(H, S, S).copy()
        out = np.empty_like(r)
        for t in range(r.shape[0]):
            rt, kt, vt = r[t].reshape(H, S), k[t].reshape(H, S), v[t].reshape(H, S)
            kv = kt[:, :, None] * vt[:, None, :]
            out[t] = np.einsum("hi,hij->hj", rt, u[:, :, None] * kv + s).reshape(-1)
            s = s * w[t].reshape(H, S)[:, :, None] + kv
        st[2 * D:] = s.reshape(-1)
        return out

    def _group_norm(self, i, y, eps):
        H, S = self.head_count, self.head_size
        if self.wrong == "ln_x":
            n = _norm(y, eps)
        else:
            n = _norm(y.reshape(-1, H, S), eps).reshape(y.shape)
        return n * self.vec(f"blocks.{i}.att.ln_x.weight") + self.vec(f"blocks.{i}.att.ln_x.bias")

    def _att_v5(self, i, x, st):
        H, S, p = self.head_count, self.head_size, f"blocks.{i}.att."
        xn, xp = self._carry(i, x, st, "ln1", 1)
        r = self.mat(p + "receptance.weight")(self._lerp(i, xn, xp, "att.time_mix_r"))
        k = self.mat(p + "key.weight")(self._lerp(i, xn, xp, "att.time_mix_k"))
        v = self.mat(p + "value.weight")(self._lerp(i, xn, xp, "att.time_mix_v"))
        if self.arch[1] >= 2:
            g = self.mat(p + "gate.weight")(self._lerp(i, xn, xp, "att.time_mix_g"))
            g = g * _sigmoid(g)
            u = self.vec(p + "time_faaaa").reshape(H, S)
            w = self.vec(p + "time_decay").reshape(H, S)
        else:   # 5.1: one time_first / time_decay per head, repeated over the head (rwkv_graph.inc:257-262)
            u = np.repeat(self.vec(p + "time_first").reshape(H, 1), S, axis=1)
            w = np.repeat(self.vec(p + "time_decay").reshape(H, 1), S, axis=1)
        y = self._wkv6(st, r, k, v, u, np.broadcast_to(w, (r.shape[0], H, S)))
        y = self._group_norm(i, y, float(np.float32(1e-5)))
        if self.arch[1] >= 2:
            y = y * g
        return self.mat(p + "output.weight")(y)

    def _att_v6(self, i, x, st):
        D, H, S, p = self.n_embed, self.head_count, self.head_size, f"blocks.{i}.att."
        xn, xp = self._carry(i, x, st, "ln1", 1)
        sx = xp - xn
        xxx = np.tanh(self.mat(p + "time_maa_w1")(xn + sx * self.vec(p + "time_maa_x")))
        T = xn.shape[0]
        ty, (R, _, _), raw = self._t[p + "time_maa_w2"]
        w2 = dequantize(ty, raw, 5 * D * R).reshape(5, D, R)
        lanes = {}
        for f, c in enumerate("wkvrg"):   # slice order w, k, v, r, g (rwkv_graph.inc:336-340)
            mf = xxx[:, f * R:(f + 1) * R] @ w2[f].T
            lanes[c] = (mf + self.vec(p + f"time_maa_{c}")) * sx + xn
        r = self.mat(p + "receptance.weight")(lanes["r"])
        k = self.mat(p + "key.weight")(lanes["k"])
        v = self.mat(p + "value.weight")(lanes["v"])
        g = self.mat(p + "gate.weight")(lanes["g"])
        g = g * _sigmoid(g)
        w = self.mat(p + "time_decay_w2")(np.tanh(self.mat(p + "time_decay_w1")(lanes["w"]))) + self.vec(p + "time_decay")
        w = np.exp(-np.exp(w))
        y = self._wkv6(st, r, k, v, self.vec(p + "time_faaaa").reshape(H, S), w.reshape(T, H, S))
        y = self._group_norm(i, y, float(np.float32(64e-5)))
        return self.mat(p + "output.weight")(y * g)

    def _att_v7(self, i, x, st):
        D, H, S, p = self.n_embed, self.head_count, self.head_size, f"blocks.{i}.att."
        T = x.shape[0]
        xn, xp = self._carry(i, x, st, "ln1", 1)
        sx = xp - xn
        mix = self.vec(p + "x_rwkvag").reshape(6, D)
        xr, xw, xk, xv, xa, xg = (xn + sx * mix[f] for f in range(6))
        r = self.mat(p + "receptance.weight")(xr)
        g = self.mat(p + "g2")(_sigmoid(self.mat(p + "g1")(xg)))
        a = _sigmoid(self.mat(p + "a2")(self.mat(p + "a1")(xa)) + self.vec(p + "a0"))
        w = self.mat(p + "w2")(np.tanh(self.mat(p + "w1")(xw))) + self.vec(p + "w0")
        w = np.exp(_sigmoid(w) * float(np.float32(-0.606531)))
        k = self.mat(p + "key.weight")(xk)
        kk = k * self.vec(p + "k_k")
        if self.wrong == "kk":
            kk = kk / np.maximum(np.sqrt((kk * kk).sum(axis=-1, keepdims=True)), 1e-12)
        else:
            kh = kk.reshape(T, H, S)
            kk = (kh / np.maximum(np.sqrt((kh * kh).sum(axis=-1, keepdims=True)), 1e-12)).reshape(T, D)
        ka = k * self.vec(p + "k_a")
        k = k + (a * ka - ka)
        v = self.mat(p + "value.weight")(xv)
        if self._v_first is None:
            self._v_first = v
        else:
            v = v + (self._v_first - v) * _sigmoid(self.mat(p + "v2")(self.mat(p + "v1")(xv)) + self.vec(p + "v0"))
        # rwkv_wkv_v7 with a = -kk, b = kk * a: per head, S[i][j] (i: value, j: key);
        # sa_i = sum_j a_j S_ij; S_ij <- S_ij w_j + v_i k_j + sa_i b_j; out_i = sum_j S_ij r_j
        s = st[2 * D:].reshape(H, S, S).copy()
        y = np.empty_like(r)
        na, nb = -kk, kk * a
        for t in range(T):
            rt, wt, kt, vt, at, bt = (z[t].reshape(H, S) for z in (r, w, k, v, na, nb))
            sa = np.einsum("hj,hij->hi", at, s)
            s = s * wt[:, None, :] + vt[:, :, None] * kt[:, None, :] + sa[:, :, None] * bt[:, None, :]
            y[t] = np.einsum("hij,hj->hi", s, rt).reshape(-1)
        st[2 * D:] = s.reshape(-1)
        y = self._group_norm(i, y, float(np.float32(64e-5)))
        krr = k * r * self.vec(p + "r_k")
        if self.wrong == "r_k":
            bonus = v * krr.sum(axis=-1, keepdims=True)
        else:
            bonus = (v.reshape(T, H, S) * krr.reshape(T, H, S).sum(axis=-1, keepdims=True)).reshape(T, D)
        return self.mat(p + "output.weight")((y + bonus) * g)

    # channel mixing (rwkv_graph.inc:484-543)
    def _ffn(self, i, x, st):
        p = f"blocks.{i}.ffn."
        xn, xp = self._carry(i, x, st, "ln2", 0)
        if self.arch[0] <= 5:
            xk, xr = self._lerp(i, xn, xp, "ffn.time_mix_k"), self._lerp(i, xn, xp, "ffn.time_mix_r")
        elif self.arch[0] == 6:
            sx = xp - xn
            xk, xr = xn + sx * self.vec(p + "time_maa_k"), xn + sx * self.vec(p + "time_maa_r")
        else:
            xk, xr = xn + (xp - xn) * self.vec(p + "x_k"), None
        k = np.maximum(self.mat(p + "key.weight")(xk), 0.0)
        out = self.mat(p + "value.weight")(k * k)
        if self.arch[0] == 7:
            return out
        return _sigmoid(self.mat(p + "receptance.weight")(xr)) * out
