"""Hand-built operands of the quantised products: blocks whose codes and scales sit at the ends of the format, activation rows that
reach every branch of the activation quantiser, and model files whose blocks are redrawn from such families. TEST INFRASTRUCTURE ONLY
(tests/test_cpu_block_extremes.py holds the oracle to float64 on everything made here, tests/test_gpu_block_extremes.py holds every GPU
product to the oracle).

The operands of every other test come from one family: N(0, 0.05^2) weights through the reference quantiser or synth._direct_blocks
(d > 0 near 0.02, m = -d levels / 2), N(0, 1) activations. Here a weight ROW is one family -- next to a block of scale 65504 a block of
scale 2^-24 vanishes in f32 rounding, and a kernel that mishandles it would still match bit for bit -- and so is an activation row.

  weight rows      code family x scale class of d (x scale class of m): weight_rows
  activation rows  one per family: activation_rows; token_operands rotates them over the tokens of a T-token operand
  model files      rewrite_quantised_blocks(path, model_palette(seed)): per block a seeded draw of a family (model_palette)
  F16 matrices     rewrite_f16_matrices(path, f16_palette(seed)): per ELEMENT a seeded draw (emb, head, RWKV-7's low-rank stages; every matrix
                   of an FP16 file). The kernel-level families of the unquantised products (F16 / F32 weight rows, f32 activation rows at the
                   edges of binary16 and binary32) are in tests/fx_lib.py, held by tests/test_{cpu,gpu}_fx_extremes.py.

No scale is inf or NaN (such a file is corrupt). Outside what is held (numerics): activations with amax / 127 > 65504, same-sign
blocks whose fp16 block sum s_x overflows under Q4_1 / Q5_1 (constant 2000 is the largest constant row: s_x = 64000), and the CODES of
activation blocks with amax < 2^-100 (the reference's reciprocal overflows; their d_x and s_x are 0 and are held).
"""
import struct
import zlib

import numpy as np

import f64_model as F

Q4_0, Q4_1, Q5_0, Q5_1, Q8_0 = F.Q4_0, F.Q4_1, F.Q5_0, F.Q5_1, F.Q8_0
QTYPES = {"Q4_0": Q4_0, "Q4_1": Q4_1, "Q5_0": Q5_0, "Q5_1": Q5_1, "Q8_0": Q8_0}
HAS_M = (Q4_1, Q5_1)
CODE_MIN = {Q4_0: 0, Q4_1: 0, Q5_0: 0, Q5_1: 0, Q8_0: -128}       # as stored
CODE_MAX = {Q4_0: 15, Q4_1: 15, Q5_0: 31, Q5_1: 31, Q8_0: 127}
CODE_BIAS = {Q4_0: 8, Q4_1: 0, Q5_0: 16, Q5_1: 0, Q8_0: 0}        # element value = (stored - bias) d (+ m); block_parts returns stored - bias
# the largest |sum_j q_w[j] q_x[j]| of a block: |q_x| <= 127, and the stored code furthest from the bias
ISUM_MAX = {t: 32 * 127 * max(CODE_MAX[t] - CODE_BIAS[t], CODE_BIAS[t] - CODE_MIN[t]) for t in CODE_MIN}

SUB = 2.0 ** -24                                                   # the smallest fp16 subnormal
SCALES = {"0": 0.0, "+sub": SUB, "-sub": -SUB, "maxsub": 1023 * SUB, "minnorm": 2.0 ** -14, "+1": 1.0, "-1": -1.0,
          "+max": 65504.0, "-max": -65504.0, "+0.02": 0.02, "-0.02": -0.02}
QH_PATTERNS = {"qh0": 0x00000000, "qhF": 0xFFFFFFFF, "qhlo": 0x0000FFFF, "qhhi": 0xFFFF0000, "qhA": 0xAAAAAAAA}


def stored_codes(type_id, q):
    """Codes as block_parts returns them (bias removed) -> as stored."""
    return np.asarray(q).astype(np.int64) + CODE_BIAS[type_id]


def pack_blocks(type_id, codes, d, m=None):
    """File-layout blocks, the inverse of f64_model.block_parts: codes (n_blocks, 32) AS STORED (0..15, 0..31, int8 for Q8_0), d and m
    np.float16 (n_blocks,). Returns uint8 (n_blocks * block bytes,). Low nibble of byte j: element j; high nibble: element 16 + j; bit j of
    qh: the fifth bit of element j."""
    codes = np.asarray(codes).astype(np.int64).reshape(-1, 32)
    n = codes.shape[0]
    assert codes.min() >= CODE_MIN[type_id] and codes.max() <= CODE_MAX[type_id], (type_id, int(codes.min()), int(codes.max()))
    d = np.asarray(d)
    assert d.dtype == np.float16 and d.shape == (n,), (d.dtype, d.shape)
    assert (m is not None) == (type_id in HAS_M)
    bb = F.BLOCK_BYTES[type_id]
    out = np.zeros((n, bb), dtype=np.uint8)
    out[:, 0:2] = d.view(np.uint8).reshape(n, 2)
    pos = 2
    if m is not None:
        m = np.asarray(m)
        assert m.dtype == np.float16 and m.shape == (n,), (m.dtype, m.shape)
        out[:, 2:4] = m.view(np.uint8).reshape(n, 2)
        pos = 4
    if type_id == Q8_0:
        out[:, 2:34] = codes.astype(np.int8).view(np.uint8)
        return out.reshape(-1)
    if type_id in (Q5_0, Q5_1):
        qh = (((codes >> 4) & 1) << np.arange(32)).sum(axis=1).astype("<u4")
        out[:, pos:pos + 4] = qh.view(np.uint8).reshape(n, 4)
        pos += 4
    out[:, pos:pos + 16] = ((codes[:, :16] & 0x0F) | ((codes[:, 16:] & 0x0F) << 4)).astype(np.uint8)
    return out.reshape(-1)


def _rng(seed, *what):
    return np.random.default_rng([int(seed)] + [zlib.crc32(str(w).encode()) for w in what])


def code_families(type_id):
    """The names of the code families of a format, in a fixed order."""
    return ["min", "max", "alt", "ramp", "random"] + (list(QH_PATTERNS) if type_id in (Q5_0, Q5_1) else [])


def family_codes(type_id, family, n_blocks, rng):
    """(n_blocks, 32) stored codes of one family. `min` of Q8_0 is -128 in every element, a code the reference quantiser never writes."""
    lo, hi = CODE_MIN[type_id], CODE_MAX[type_id]
    j = np.arange(32)
    if family == "min":
        row = np.full(32, lo)
    elif family == "max":
        row = np.full(32, hi)
    elif family == "alt":
        row = np.where(j % 2 == 0, lo, hi)
    elif family == "ramp":
        row = lo + (j * (hi - lo)) // 31
    elif family == "random":
        return rng.integers(lo, hi + 1, size=(n_blocks, 32))
    else:                                                            # Q5: a fixed qh word over random low nibbles
        low = rng.integers(0, 16, size=(n_blocks, 32))
        return low | (((QH_PATTERNS[family] >> j) & 1) << 4)
    return np.broadcast_to(row, (n_blocks, 32)).copy()


def weight_rows(type_id, K, seed):
    """(bytes uint8 (R * row bytes,), names): R rows of K elements. Every row but the last four is homogeneous: one code family, one class
    of d, one class of m in all its blocks. Q4_0 / Q5_0 / Q8_0: every code family x every class of d. Q4_1 / Q5_1: every class of d x
    every class of m (d = 0 with m != 0, m = 0, m > 0 and |m| >> |d| among them), the code family cycling over the pairs so that every code
    family meets every class of d. The last four rows draw family and classes per block."""
    nb, rng = K // 32, _rng(seed, "weights", type_id, K)
    fams, classes = code_families(type_id), list(SCALES)
    f16 = lambda name: np.full(nb, SCALES[name], dtype=np.float16)   # noqa: E731
    rows, names = [], []
    if type_id in HAS_M:
        for i, dn in enumerate(classes):
            for k, mn in enumerate(classes):
                fam = fams[(i + k) % len(fams)]
                rows.append(pack_blocks(type_id, family_codes(type_id, fam, nb, rng), f16(dn), f16(mn)))
                names.append(f"{fam}/d{dn}/m{mn}")
    else:
        for fam in fams:
            for dn in classes:
                rows.append(pack_blocks(type_id, family_codes(type_id, fam, nb, rng), f16(dn)))
                names.append(f"{fam}/d{dn}")
    vals = np.array([SCALES[c] for c in classes], dtype=np.float16)
    for r in range(4):
        codes = np.concatenate([family_codes(type_id, fams[rng.integers(len(fams))], 1, rng) for _ in range(nb)])
        m = vals[rng.integers(len(vals), size=nb)] if type_id in HAS_M else None
        rows.append(pack_blocks(type_id, codes, vals[rng.integers(len(vals), size=nb)], m))
        names.append(f"mixed{r}")
    return np.concatenate(rows), names


def take_rows(w_bytes, type_id, K, start, N):
    """N rows of a weight_rows payload from row `start` on, cyclically: (bytes, row indices)."""
    rb = (K // 32) * F.BLOCK_BYTES[type_id]
    rows = w_bytes.reshape(-1, rb)
    idx = (start + np.arange(N)) % rows.shape[0]
    return np.ascontiguousarray(rows[idx]).reshape(-1), idx


def probe_q8_0(K):
    """The Q8_0 matrix with N = K, row n: code 1 at element n, d = 1. y[t][n] = d_x q_x[n] of token t exactly: a wrong activation code
    shows by its position."""
    codes = np.zeros((K, K), dtype=np.int64)
    codes[np.arange(K), np.arange(K)] = 1
    return pack_blocks(Q8_0, codes.reshape(-1, 32), np.ones(K * K // 32, dtype=np.float16))


def tie_row(K):
    """The half-integer row of tests/test_gpu_det_math.py: block b holds ((32 b + j) mod 255 - 127) / 2, element 0 is 63.5."""
    t = np.arange(K, dtype=np.float64).reshape(-1, 32) % 255 - 127.0
    t[:, 0] = 127.0
    return (t * 0.5).reshape(-1)


def activation_rows(K, seed):
    """(x float32 (R, K), names): one row per family.

      zeros        +0.0
      negzero      blocks of -0.0, of N(0, 1), and of -0.0 / +0.0 alternating, in turn
      +127 -127    constant: d_x = 1, every code +-127         alt127   +-127 alternating: the same codes, s_x = 0
      ties         tie_row(K): d_x = 0.5, x / d_x integers      halves   element 0 is 127 (d_x = 1), the others k + 0.5: every code a rounding tie
      spike        one non-zero element per block, at position b mod 32, signs alternating
      negmax       N(0, 1) with one element of -5 per block: the largest magnitude is negative
      n1e-3        N(0, 1) 1e-3: d_x an fp16 subnormal of many steps
      n2e-6        N(0, 1) 1.8e-6: amax / 127 near 2^-25, d_x rounds to 2^-24 or to 0
      n1e-6 n3e-8  N(0, 1) 1e-6 and 3e-8: d_x = 0 under codes that reach +-127 (they come from the f32 quotient); s_x, rounded from the f32
                   product, is not 0: up to 221 and 7 times 2^-24
      n1e-40       f32 denormals: d_x = s_x = 0               alt8e6   +-8e6 alternating: d_x = 62976 or 63008, s_x = 0
      c2000        constant 2000: s_x = 64000                 normal   N(0, 1)
    """
    nb, rng = K // 32, _rng(seed, "activations", K)
    n = lambda: rng.standard_normal((nb, 32))                        # noqa: E731
    j, b = np.arange(32), np.arange(nb)
    sign = np.where(j % 2 == 0, 1.0, -1.0)
    rows = {"zeros": np.zeros((nb, 32))}
    z = n()
    z[b % 3 == 0] = -0.0
    z[b % 3 == 2] = np.where(j % 2 == 0, -0.0, 0.0)
    rows["negzero"] = z
    rows["+127"] = np.full((nb, 32), 127.0)
    rows["-127"] = np.full((nb, 32), -127.0)
    rows["alt127"] = np.broadcast_to(127.0 * sign, (nb, 32)).copy()
    rows["ties"] = tie_row(K).reshape(nb, 32)
    h = (rng.integers(-127, 127, size=(nb, 32)) + 0.5)
    h[:, 0] = 127.0
    rows["halves"] = h
    s = np.zeros((nb, 32))
    s[b, b % 32] = np.where(b % 2 == 0, 1.0, -1.0) * 3.7 * (1 + b % 7)
    rows["spike"] = s
    g = n()
    g[b, (5 * b + 3) % 32] = -5.0 - np.abs(g[b, 0])
    rows["negmax"] = g
    rows["n1e-3"], rows["n2e-6"], rows["n1e-6"], rows["n3e-8"] = n() * 1e-3, n() * 1.8e-6, n() * 1e-6, n() * 3e-8
    rows["n1e-40"] = n() * 1e-40
    rows["alt8e6"] = np.broadcast_to(8e6 * sign, (nb, 32)).copy()
    rows["c2000"] = np.full((nb, 32), 2000.0)
    rows["normal"] = n()
    with np.errstate(under="ignore"):
        x = np.stack([v.reshape(-1) for v in rows.values()]).astype(np.float32)
    return x, list(rows)


def token_operands(K, T, seed):
    """The T-token operands of one shape: one per rotation r of the R activation rows, token t of operand r holding row (t + r) mod R. Over
    the R operands every family lands on every token, token 0, 31, 32 and T - 1 among them (the tile quantiser owns 32 tokens per wave and
    16 elements per lane). Returns [(x (T, K), family index of every token)]."""
    rows, _ = activation_rows(K, seed)
    R = rows.shape[0]
    return [(np.ascontiguousarray(rows[(np.arange(T) + r) % R]), (np.arange(T) + r) % R) for r in range(R)]


# ---------------------------------------------------------------------------------------------------------------------------------------
# model files
# ---------------------------------------------------------------------------------------------------------------------------------------

def quantised_tensors(path):
    """[(name, type, dims, byte offset of the payload, payload bytes)] of the quantised 2-D tensors of a model file."""
    with open(path, "rb") as f:
        blob = f.read()
    out, p = [], 24
    while p < len(blob):
        nd, kl, ty = struct.unpack_from("<3I", blob, p)
        p += 12
        dims = struct.unpack_from(f"<{nd}I", blob, p)
        p += 4 * nd
        name = blob[p:p + kl].decode()
        p += kl
        n = int(np.prod(dims))
        nbytes = n * 4 if ty == F.F32 else n * 2 if ty == F.F16 else (n // 32) * F.BLOCK_BYTES[ty]
        if ty in F.BLOCK_BYTES and nd == 2:
            out.append((name, ty, tuple(dims), p, nbytes))
        p += nbytes
    return out


def rewrite_quantised_blocks(path, fn):
    """The counterpart of stress_lib.rewrite_f32_vectors for the quantised 2-D tensors of a written model file: for each,
    fn(name, type, codes (N, K / 32, 32) as stored, d float16 (N, K / 32), m float16 (N, K / 32) or None) -> (codes, d, m) of the same
    shapes, or None (left alone), packed over the old payload in place (a (K, N) tensor is N rows of K / 32 blocks). Returns
    {name: per-family block counts} for the tensors rewritten, the counts as fn.counts[name] gives them ({} where fn keeps none)."""
    with open(path, "rb") as f:
        blob = bytearray(f.read())
    done = {}
    for name, ty, dims, at, nbytes in quantised_tensors(path):
        n = int(np.prod(dims))
        q, d, m = F.block_parts(ty, bytes(blob[at:at + nbytes]), n)
        codes, d16 = stored_codes(ty, q), d.astype(np.float16)
        m16 = None if m is None else m.astype(np.float16)
        assert np.array_equal(pack_blocks(ty, codes, d16, m16), np.frombuffer(bytes(blob[at:at + nbytes]), dtype=np.uint8)), name
        shape = (dims[1], dims[0] // 32)
        new = fn(name, ty, codes.reshape(shape + (32,)), d16.reshape(shape), None if m16 is None else m16.reshape(shape))
        if new is None:
            continue
        raw = pack_blocks(ty, new[0].reshape(-1, 32), new[1].reshape(-1), None if new[2] is None else new[2].reshape(-1))
        assert raw.size == nbytes, (name, raw.size, nbytes)
        blob[at:at + nbytes] = raw.tobytes()
        done[name] = dict(getattr(fn, "counts", {}).get(name, {}))
    with open(path, "wb") as f:
        f.write(blob)
    return done


PALETTE_0 = ("keep", "neg", "zero", "subnormal", "codes")
PALETTE_1 = PALETTE_0 + ("zero-both", "m-zero", "m-scaled")
ZERO_KEY_ROWS = {0: 64, 1: 48}     # layer -> first of 64 consecutive ffn.key rows zeroed (layer 1: not on a block edge of the ffn.value input)


def palette_families(type_id, name):
    fams = PALETTE_1 if type_id in HAS_M else PALETTE_0
    return fams + (("key-rows-zero",) if _zero_key_layer(name) is not None else ())


def _zero_key_layer(name):
    parts = name.split(".")
    if len(parts) == 5 and parts[0] == "blocks" and parts[2:] == ["ffn", "key", "weight"] and int(parts[1]) in ZERO_KEY_ROWS:
        return int(parts[1])
    return None


def model_palette(seed):
    """The fn of rewrite_quantised_blocks used at model level. Per block, by a draw u ~ U(0, 1) seeded by (seed, tensor name):

      u < .50   keep
      u < .65   neg        d -> -d; Q4_1 / Q5_1: m -> -m too (a positive m of the same magnitudes)
      u < .75   zero       d = 0; Q4_1 / Q5_1: m kept for two in three (zero), both 0 for the third (zero-both)
      u < .85   subnormal  d = 2^-24, -2^-24 or 1023 2^-24 (m kept)
      u < .95   codes      all-min, all-max or alternating codes, d (and m) kept
      rest      Q4_0 / Q5_0 / Q8_0: keep; Q4_1 / Q5_1: m = 0 (m-zero) or m times U(-4, 4) (m-scaled)
    In layers 0 and 1, 64 consecutive rows of ffn.key.weight get d = 0 (and m = 0): relu(k)^2 hands exact zero blocks to the ffn.value
    product through each path's own activation quantiser (key-rows-zero). The large scale classes stay at kernel level: logits stay
    finite. fn.counts[name] holds the blocks of every family of a tensor."""
    def fn(name, ty, codes, d, m):
        rng = _rng(seed, "palette", name)
        shape, n = d.shape, d.size
        codes, d = codes.reshape(n, 32), d.reshape(n)
        m = None if m is None else m.reshape(n)
        u, pick, v = rng.random(n), rng.integers(0, 3, size=n), rng.uniform(-4.0, 4.0, size=n)
        codes, d = codes.copy(), d.copy()
        m = None if m is None else m.copy()
        fam = np.full(n, "keep", dtype=object)
        s = (u >= 0.50) & (u < 0.65)
        fam[s] = "neg"
        d[s] = -d[s]
        if m is not None:
            m[s] = -m[s]
        s = (u >= 0.65) & (u < 0.75)
        fam[s] = "zero"
        d[s] = 0
        if m is not None:
            both = s & (pick == 2)
            fam[both] = "zero-both"
            m[both] = 0
        s = (u >= 0.75) & (u < 0.85)
        fam[s] = "subnormal"
        d[s] = np.array([SUB, -SUB, 1023 * SUB], dtype=np.float16)[pick[s]]
        s = (u >= 0.85) & (u < 0.95)
        fam[s] = "codes"
        lo, hi = CODE_MIN[ty], CODE_MAX[ty]
        pats = np.stack([np.full(32, lo), np.full(32, hi), np.where(np.arange(32) % 2 == 0, lo, hi)])
        codes[s] = pats[pick[s]]
        if m is not None:
            s = u >= 0.95
            z = s & (pick == 0)
            fam[z] = "m-zero"
            m[z] = 0
            sc = s & (pick != 0)
            fam[sc] = "m-scaled"
            m[sc] = (m[sc].astype(np.float64) * v[sc]).astype(np.float16)
        layer = _zero_key_layer(name)
        codes, d = codes.reshape(shape + (32,)), d.reshape(shape)
        m = None if m is None else m.reshape(shape)
        if layer is not None:
            rows = slice(ZERO_KEY_ROWS[layer], ZERO_KEY_ROWS[layer] + 64)
            fam.reshape(shape)[rows] = "key-rows-zero"
            d[rows] = 0
            if m is not None:
                m[rows] = 0
        fn.counts[name] = {k: int((fam == k).sum()) for k in palette_families(ty, name)}
        return codes, d, m
    fn.counts = {}
    return fn



def write_palette_model(synth, path, name, fmt, seed):
    """Writes synth.CONFIGS[name] as `fmt` and redraws its quantised tensors with model_palette(seed). Every family must occur in every
    rewritten tensor (asserted). Returns {tensor: counts}."""
    synth.write_model(path, synth.CONFIGS[name], fmt, seed=seed)
    want = [t[0] for t in quantised_tensors(path)]
    counts = rewrite_quantised_blocks(path, model_palette(seed))
    assert want and list(counts) == want, (name, fmt, want, list(counts))
    for tensor, c in counts.items():
        assert set(c) == set(palette_families(QTYPES[fmt], tensor)) and min(c.values()) >= 1, (name, fmt, tensor, c)
        if "key-rows-zero" in c:
            assert c["key-rows-zero"] == 64 * synth.CONFIGS[name].n_embed // 32, (tensor, c)
    assert sum("key-rows-zero" in c for c in counts.values()) == 2, (name, fmt)
    return counts


# ---------------------------------------------------------------------------------------------------------------------------------------
# model files: the F16 matrices (every matrix of an FP16 file; emb, head and RWKV-7's low-rank stages of a quantised one)
# ---------------------------------------------------------------------------------------------------------------------------------------

def f16_matrices(path):
    """[(name, dims, byte offset of the payload, payload bytes)] of the F16 2-D tensors of a model file."""
    with open(path, "rb") as f:
        blob = f.read()
    out, p = [], 24
    while p < len(blob):
        nd, kl, ty = struct.unpack_from("<3I", blob, p)
        p += 12
        dims = struct.unpack_from(f"<{nd}I", blob, p)
        p += 4 * nd
        name = blob[p:p + kl].decode()
        p += kl
        n = int(np.prod(dims))
        nbytes = n * 4 if ty == F.F32 else n * 2 if ty == F.F16 else (n // 32) * F.BLOCK_BYTES[ty]
        if ty == F.F16 and nd == 2:
            out.append((name, tuple(dims), p, nbytes))
        p += nbytes
    return out


def rewrite_f16_matrices(path, fn):
    """The counterpart of rewrite_quantised_blocks for the F16 2-D tensors of a written model file: for each,
    fn(name, dims, w float16 (N, K)) -> float16 (N, K), or None (left alone), written over the old payload in place (a (K, N) tensor is N
    rows of K elements). Returns {name: per-family element counts} for the tensors rewritten, as fn.counts[name] gives them."""
    with open(path, "rb") as f:
        blob = bytearray(f.read())
    done = {}
    for name, dims, at, nbytes in f16_matrices(path):
        w = np.frombuffer(bytes(blob[at:at + nbytes]), dtype=np.float16).reshape(dims[1], dims[0])
        new = fn(name, dims, w)
        if new is None:
            continue
        assert new.dtype == np.float16 and new.shape == w.shape, (name, new.dtype, new.shape)
        blob[at:at + nbytes] = np.ascontiguousarray(new).tobytes()
        done[name] = dict(getattr(fn, "counts", {}).get(name, {}))
    with open(path, "wb") as f:
        f.write(blob)
    return done


F16_PALETTE = ("keep", "neg", "zero", "subnormal", "minnorm", "lowbits")


def f16_palette(seed):
    """The fn of rewrite_f16_matrices used at model level. Per ELEMENT, by a draw u ~ U(0, 1) seeded by (seed, tensor name):

      u < .60   keep
      u < .70   neg        w -> -w
      u < .78   zero       +0 or -0
      u < .88   subnormal  +-j 2^-24, j uniform in 1 .. 1023
      u < .92   minnorm    2^-14, the smallest normal
      rest      lowbits    +-s (1 + j 2^-10), j uniform in 0 .. 1023: every mantissa bit in use; s the largest power of two with 2 s <= the
                           tensor's largest magnitude (tests/fx_lib.py has the family at s = 1; here no value may leave the tensor's range)
    No value is inf or NaN or larger than the tensor's own largest magnitude, and no row is entirely zero (both asserted): logits stay finite.
    fn.counts[name] holds the elements of every family of a tensor."""
    def fn(name, dims, w):
        rng = _rng(seed, "f16-palette", name)
        shape, n = w.shape, w.size
        w = w.reshape(n).copy()
        top = float(np.abs(w.astype(np.float64)).max())
        assert np.isfinite(top) and top >= 2.0 ** -13, (name, top)
        u, neg, j = rng.random(n), rng.random(n) < 0.5, rng.integers(0, 1024, size=n)
        sgn = np.where(neg, -1.0, 1.0)
        fam = np.zeros(n, dtype=np.uint8)                               # index into F16_PALETTE
        s = (u >= 0.60) & (u < 0.70)
        fam[s] = 1
        w[s] = -w[s]
        s = (u >= 0.70) & (u < 0.78)
        fam[s] = 2
        w[s] = (0.0 * sgn[s]).astype(np.float16)
        s = (u >= 0.78) & (u < 0.88)
        fam[s] = 3
        w[s] = (sgn[s] * np.maximum(j[s], 1) * SUB).astype(np.float16)
        s = (u >= 0.88) & (u < 0.92)
        fam[s] = 4
        w[s] = np.float16(2.0 ** -14)
        s = u >= 0.92
        fam[s] = 5
        scale = 2.0 ** (np.floor(np.log2(top)) - 1)
        w[s] = (sgn[s] * scale * (1.0 + j[s] * 2.0 ** -10)).astype(np.float16)
        w64 = w.astype(np.float64)
        assert np.isfinite(w64).all() and np.abs(w64).max() <= top, (name, float(np.abs(w64).max()), top)
        assert np.abs(w64.reshape(shape)).max(axis=1).min() > 0, (name, "a row is entirely zero")
        fn.counts[name] = dict(zip(F16_PALETTE, (int(c) for c in np.bincount(fam, minlength=len(F16_PALETTE)))))
        return w.reshape(shape)
    fn.counts = {}
    return fn


def write_f16_palette_model(synth, path, name, fmt, seed):
    """Writes synth.CONFIGS[name] as `fmt` and redraws its F16 matrices with f16_palette(seed); the quantised blocks (and the f32 tensors)
    stay as synth wrote them, so a failure points at F16. Every family must occur in every rewritten tensor (asserted). Returns
    {tensor: counts}."""
    synth.write_model(path, synth.CONFIGS[name], fmt, seed=seed)
    want = [t[0] for t in f16_matrices(path)]
    counts = rewrite_f16_matrices(path, f16_palette(seed))
    assert {"emb.weight", "head.weight"} <= set(want) and list(counts) == want, (name, fmt, want, list(counts))
    for tensor, c in counts.items():
        assert set(c) == set(F16_PALETTE) and min(c.values()) >= 1, (name, fmt, tensor, c)
    return counts
