"""Stress inputs of the recurrences: model files whose decay vectors reach their ends, and states that no kernel produced itself.
TEST INFRASTRUCTURE ONLY (a helper module; tests/test_cpu_stress_reference.py holds the oracle to float64 on everything made here,
tests/test_gpu_injected_state.py holds every GPU path to the oracle).

synth.py draws the vectors that drive the recurrences from narrow ranges (RWKV-4 time_decay in -exp(U(-5, 1)), RWKV-5 decay in
[0.9, 0.999], RWKV-6 / 7 decay base in [-6, -1], time_first / time_faaaa within +-1 or +-0.1), and every parity test starts from the fresh
state. `stress_vectors` rewrites those vectors of a written file, `state_families` makes the states to inject.

  arch   tensor                          values
  4      att.time_decay                  -exp(U(-9, 3.5))                       (-33 .. -1.2e-4)
  4      att.time_first                  U(-12, 12)
  5.x    att.time_decay (stored as the   U(0.5, 1); of every five entries the first is exactly 0, the second exactly 1, the third 1e-30
         per-token factor)
  5.x    att.time_first / time_faaaa     U(-4, 4)
  6      att.time_decay                  U(-14, 4); of every sixteen entries the first is 6 and the second -14. U(-14, 4) alone ends at
                                         exp(-exp(4)) = 2e-24, not at 0: f32 exp(-exp(w)) is exactly 0 only from w = 4.65 on. The pinned 6 gives
                                         exp(-403) = 0 whatever the data-dependent part (|.| < 1 on these files) adds; the pinned -14 gives 1 - 8.3e-7.
  6      att.time_faaaa                  U(-4, 4)
  7      att.w0                          U(-14, 8)   (the factor exp(-0.606531 sigmoid(w)) spans 1 - 5e-7 .. 0.5455: RWKV-7 has no zero decay)
  5.x-7  att.ln_x.weight                 U(-3, 3)
"""
import zlib

import numpy as np

import f64_model as F

PROMPT_LEN = 300   # tokens behind the `long-run` state


def lcg_tokens(n_vocab, n, start=0):
    """The prompt used across the suite: (1103515245 i + 12345) mod n_vocab."""
    return [int((1103515245 * i + 12345) % n_vocab) for i in range(start, start + n)]


def rewrite_f32_vectors(path, fn):
    """For every tensor of the file, fn(name, dims, old float32 values) -> None or a new float32 array of the same size, written over the
    old one in place. A tensor is located by its bytes: the match must be unique and the tensor F32. Returns the names rewritten."""
    _, tensors = F.read_file(path)
    with open(path, "rb") as f:
        blob = bytearray(f.read())
    done = []
    for name, (ty, dims, mv) in tensors.items():
        old = np.frombuffer(bytes(mv), dtype="<f4").copy() if ty == F.F32 else None
        new = fn(name, dims, old)
        if new is None:
            continue
        assert ty == F.F32, (name, "is not F32", ty)
        new = np.ascontiguousarray(new, dtype="<f4").reshape(-1)
        assert new.size == old.size, (name, new.size, old.size)
        raw = bytes(mv)
        at = blob.find(raw)
        assert at > 0 and blob.find(raw, at + 1) < 0, (name, "is not unique by its bytes")
        blob[at:at + len(raw)] = new.tobytes()
        done.append(name)
    with open(path, "wb") as f:
        f.write(blob)
    return done


def _rng(seed, name):
    return np.random.default_rng([int(seed), zlib.crc32(name.encode())])


def stress_vectors(arch, seed):
    """The fn of rewrite_f32_vectors that spreads the recurrence's own parameters of an `arch` ("4", "5.1", "5.2", "6", "7") file to their
    ends (module docstring). Each tensor's values depend on (seed, its name) only."""
    assert arch in ("4", "5.1", "5.2", "6", "7"), arch

    def fn(name, dims, old):
        if not name.startswith("blocks."):
            return None
        key = name.split(".", 2)[2]
        n = int(np.prod(dims))
        rng = _rng(seed, name)
        if key == "att.ln_x.weight":
            return rng.uniform(-3.0, 3.0, n).astype(np.float32)
        if arch == "4":
            if key == "att.time_decay":
                return (-np.exp(rng.uniform(-9.0, 3.5, n))).astype(np.float32)
            if key == "att.time_first":
                return rng.uniform(-12.0, 12.0, n).astype(np.float32)
        elif arch in ("5.1", "5.2"):
            if key == "att.time_decay":
                w = rng.uniform(0.5, 1.0, n).astype(np.float32)
                w[0::5], w[1::5], w[2::5] = 0.0, 1.0, 1e-30
                return w
            if key in ("att.time_first", "att.time_faaaa"):
                return rng.uniform(-4.0, 4.0, n).astype(np.float32)
        elif arch == "6":
            if key == "att.time_decay":
                w = rng.uniform(-14.0, 4.0, n).astype(np.float32)
                w[0::16], w[1::16] = 6.0, -14.0
                return w
            if key == "att.time_faaaa":
                return rng.uniform(-4.0, 4.0, n).astype(np.float32)
        elif key == "att.w0":
            return rng.uniform(-14.0, 8.0, n).astype(np.float32)
        return None
    return fn


def expected_names(arch, n_layer):
    """The names stress_vectors(arch, .) rewrites in a file of n_layer layers."""
    keys = {"4": ("att.time_decay", "att.time_first"), "5.1": ("att.time_decay", "att.time_first", "att.ln_x.weight"),
            "5.2": ("att.time_decay", "att.time_faaaa", "att.ln_x.weight"), "6": ("att.time_decay", "att.time_faaaa", "att.ln_x.weight"),
            "7": ("att.w0", "att.ln_x.weight")}[arch]
    return {f"blocks.{i}.{k}" for i in range(n_layer) for k in keys}


def state_families(om, seed, long_run=True):
    """{family: float32 state in the oracle's layout} for the file `om` (an oracle_lib.OracleModel) has loaded. All values are finite.

      normal      N(0, 1) everywhere
      large       N(0, 64^2) everywhere
      tiny        N(0, (1e-41)^2) everywhere: denormals
      long-run    the oracle's own state after PROMPT_LEN tokens of lcg_tokens
      half-fresh  RWKV-4 only: even channels as in init_state() (aa = bb = 0, pp = -1e30, shifts 0), odd channels as in `normal`
      pp-high     RWKV-4 only: `normal` with pp ~ U(40, 80)
    RWKV-4 (per layer: ffn shift, att shift, aa, bb, pp): in every drawn family bb = |drawn| + 0.5 (`tiny`: + 1e-40) and pp ~ U(-60, 60).
    long_run=False leaves `long-run` out (300 oracle tokens: seconds at D = 4096); the drawn families are the same values either way."""
    rng = np.random.default_rng([int(seed), om.arch_major, om.arch_minor, om.n_embed])
    n, v4 = om.state_len, om.arch_major == 4
    out = {}
    for family, sd, floor in (("normal", 1.0, 0.5), ("large", 64.0, 0.5), ("tiny", 1e-41, 1e-40)):
        s = (rng.standard_normal(n) * sd).astype(np.float32)
        if v4:
            v = s.reshape(om.n_layer, 5, om.n_embed)
            v[:, 3] = (np.abs(v[:, 3].astype(np.float64)) + floor).astype(np.float32)
            v[:, 4] = rng.uniform(-60.0, 60.0, v[:, 4].shape).astype(np.float32)
        out[family] = s
    if long_run:
        _, out["long-run"] = om.eval_sequence(lcg_tokens(om.n_vocab, PROMPT_LEN), om.init_state(), want_logits=False)
    if v4:
        s = out["normal"].copy()
        s.reshape(om.n_layer, 5, om.n_embed)[:, :, 0::2] = om.init_state().reshape(om.n_layer, 5, om.n_embed)[:, :, 0::2]
        out["half-fresh"] = s
        s = out["normal"].copy()
        pp = s.reshape(om.n_layer, 5, om.n_embed)[:, 4]
        pp[...] = rng.uniform(40.0, 80.0, pp.shape).astype(np.float32)
        out["pp-high"] = s
    for family, s in out.items():
        assert s.dtype == np.float32 and s.shape == (n,) and np.isfinite(s).all(), family
    return out
