"""The geometries every fast decode path ADMITS, beside the ones it was tuned on. TEST INFRASTRUCTURE ONLY (a helper module;
tests/test_cpu_admitted_geometry.py holds the oracle to float64 on these files and checks that each file is what its row says,
tests/test_gpu_admitted_geometry.py holds every decode path to the oracle on them).

Each path decides at load time whether it takes a model: ring_variant -> rg_variant_key (csrc/ring_geom.h), mega_variant
(csrc/mega_v6.hip), p47_variant (csrc/persist_v47.hip), fused_v6_supported, fused_v7_supported, fused_v4_supported. What they admit:

  k6_ring  D 2048   F 6176 .. 8192 in steps of 32 (193 .. 256 blocks), mix rank 32 | 64, decay rank 64
           D 2560   F 8256 .. 9536 in steps of 64, mix rank 32 | 64, decay rank 64
           D 4096   F 12352 .. 14336 in steps of 64, mix rank 32 | 64, decay rank 128
  k6_mega  D 2048   F 32 .. 7488 in steps of 32 (3 F / 32 <= 704 units), decay rank 64
           D 4096   F 8224 .. 14336 in steps of 32 (two key groups per workgroup, 3 F / 32 <= 1344), decay rank 128
  k47 v7   D 256    F = 4 D; ranks % 32 = 0, g <= 128, w / a / v <= 64, widest layer's sum <= 256
           D 2560   F = 4 D; g <= 320, w / a / v <= 96, sum <= 576
  k47 v4   D 256 | 768, F = 4 D
  fused    v6: D % 256 = 0, F % 32 = 0, mix rank <= 256, decay rank 64 | 128;  v7: D % 256 = 0, F % 32 = 0, every rank % 32 = 0 and <= 512;
           v4: D % 256 = 0, F % 32 = 0;  RWKV-5: none

CASES has one row per case: the spec (dataclasses.replace of a synth.CONFIGS entry: two layers and V = 512 unless the row says otherwise),
the format, the environment the context is created under, and the decode_path() / persist_kind() that context must report -- written by
hand from the predicates above and ASSERTED by both test files' users, so that no case passes by falling back to another path.
`other` is the environment of a second context of the same file on a slower path (None: there is none below the expected one).

The rows sit on these edges (F / 32 = blocks of an F-long row; a step = 64 blocks):
  ring   2048: F 6176 the lowest (193 blocks = three steps + one block; 63 workgroups own no key group) . F 7200 (F % 128 = 32: the
         sub-16-byte tail of qvec_stage) . F 8192 the top (256 blocks: a key group on every workgroup) . F 7168 at mix rank 64
         2560: F 8256 the lowest (258 blocks) . F 9536 the top (298 blocks, 894 of 896 gather units) . F 8960 at mix rank 64
         4096: F 12352 the lowest (386 blocks: a two-block seventh step) . F 14272 (446 blocks) . F 14336 at mix rank 32
         one format other than Q4_0 at a non-tuned F per D, and F 7200 behind a folded head (V = 4096)
  regs   2048: F 1024 . F 7200 . F 7488 the top (702 of 704 units) . F 7168 at mix rank 64 . F 32 the bottom (LAST: see below)
         4096: F 8224 the lowest (257 blocks) . F 14304 (447 blocks, odd: the ring declines it)
  outside (one step past an edge; the fused launches, path 1): 2048 / F 6144 under =ring . 2048 / F 8224 (both decline) .
         2560 / F 8288 (259 blocks, odd at two groups per workgroup) . 4096 at decay rank 64
  k47    v7 256: ranks (w, a, g, v) = (32, 32, 32, 32) . (32, 64, 128, 32), sum 256, the top . one layer (no v1 / v2 anywhere);
         outside: g 160 . w 96 . F = 3.5 D.   v7 2560: (32, 32, 32, 32) . (64, 96, 288, 32): 480 on layers >= 1 is 7.5 64-unit poll
         slots of the lr1 vector (layer 0, without v1, has 448 = 7 whole ones); outside: g 352.   v4 768 with F != 4 D: fused
  fused  v6: D 512 / F 1824 (57 blocks, F % 128 = 32) ranks (48, 128) . D 1280 / F 4544 (F % 128 = 64) mix rank 256 . mix rank 260 and
         decay rank 32 decline (per-op).   v7: D 512 / F 1056 ranks (128, 64, 256, 96) . D 1024 with w 512 . w 544 declines . one layer.
         v4: D 512 / F 2048 . D 1280 / F 3104 (F % 128 = 32).   RWKV-5.1 / 5.2: D 512 / F 1824, per-op only

The F = 32 row of k6_mega (one block per ffn.value row, one key group in the whole grid) is the last row of CASES: the shape furthest
from anything the kernel had run at, so that on a shared device it can be selected last and alone (`-k regs-2048-F32`)."""
import dataclasses

RING = {"RWKV_MI_PERSIST": "ring"}
REGS = {"RWKV_MI_PERSIST": "regs"}
NO_MEGA = {"RWKV_MI_NO_MEGA": "1"}
NO_FUSED = {"RWKV_MI_NO_FUSED": "1"}
DEFAULT = {}

V6_BASE = {2048: "mega-v6-2048", 2560: "mega-v6-2560", 4096: "mega-v6-4096"}


@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    group: str          # ring | regs | outside | k47 | fused
    arch: str
    spec: tuple         # (base name in synth.CONFIGS, ((field, value), ...)) -- see spec()
    fmt: str
    env: tuple          # ((name, value), ...): the environment of the context under test
    path: int           # decode_path() it must report: 0 per-op, 1 fused launches, 2 one persistent launch
    kind: int           # persist_kind(): 0 none, 1 regs (k6_mega), 2 ring (k6_ring), 3 k47
    other: tuple        # environment of the second context (a slower path), or None
    other_path: int
    seed: int


def _row(id_, group, arch, base, fmt, env, path, kind, other, other_path, **fields):
    fields.setdefault("n_layer", 2)
    fields.setdefault("n_vocab", 512)
    n = len(_ROWS)
    _ROWS.append(Case(id_, group, arch, (base, tuple(sorted(fields.items()))), fmt, tuple(sorted(env.items())), path, kind,
                      None if other is None else tuple(sorted(other.items())), other_path, 101 + n))


_ROWS = []


def _v6(id_, group, D, F, env, path, kind, fmt="Q4_0", **more):
    # a persistent case is held beside the fused launches, a fused one beside the per-op path
    other, other_path = (NO_MEGA, 1) if path == 2 else (NO_FUSED, 0)
    _row(id_, group, "6", V6_BASE[D], fmt, env, path, kind, other, other_path, ffn=F, **more)


# ---- k6_ring ----
_v6("ring-2048-F6176", "ring", 2048, 6176, RING, 2, 2)
_v6("ring-2048-F7200", "ring", 2048, 7200, RING, 2, 2)
_v6("ring-2048-F8192", "ring", 2048, 8192, RING, 2, 2)
_v6("ring-2048-F7168-R64", "ring", 2048, 7168, RING, 2, 2, mix_rank=64)
_v6("ring-2560-F8256", "ring", 2560, 8256, RING, 2, 2)
_v6("ring-2560-F9536", "ring", 2560, 9536, RING, 2, 2)
_v6("ring-2560-F8960-R64", "ring", 2560, 8960, RING, 2, 2, mix_rank=64)
_v6("ring-4096-F12352", "ring", 4096, 12352, RING, 2, 2)
_v6("ring-4096-F14272", "ring", 4096, 14272, RING, 2, 2)
_v6("ring-4096-F14336-R32", "ring", 4096, 14336, RING, 2, 2, mix_rank=32)
_v6("ring-2048-F6176-Q8_0", "ring", 2048, 6176, RING, 2, 2, fmt="Q8_0")
_v6("ring-2560-F9536-Q5_1", "ring", 2560, 9536, RING, 2, 2, fmt="Q5_1")
_v6("ring-4096-F12352-Q5_0", "ring", 4096, 12352, RING, 2, 2, fmt="Q5_0")
_v6("ring-2048-F7200-V4096", "ring", 2048, 7200, RING, 2, 2, n_vocab=4096)
# ---- k6_mega ----
_v6("regs-2048-F1024", "regs", 2048, 1024, REGS, 2, 1)
_v6("regs-2048-F7200", "regs", 2048, 7200, REGS, 2, 1)
_v6("regs-2048-F7488", "regs", 2048, 7488, REGS, 2, 1)
_v6("regs-2048-F7168-R64", "regs", 2048, 7168, REGS, 2, 1, mix_rank=64)
_v6("regs-4096-F8224", "regs", 4096, 8224, REGS, 2, 1)
_v6("regs-4096-F14304", "regs", 4096, 14304, REGS, 2, 1)
# ---- one step outside the RWKV-6 persistent kernels ----
_v6("outside-2048-F6144-ring", "outside", 2048, 6144, RING, 1, 0)
_v6("outside-2048-F8224-ring", "outside", 2048, 8224, RING, 1, 0)
_v6("outside-2048-F8224-regs", "outside", 2048, 8224, REGS, 1, 0)
_v6("outside-2560-F8288", "outside", 2560, 8288, RING, 1, 0)
_v6("outside-4096-DR64-ring", "outside", 4096, 14336, RING, 1, 0, decay_rank=64)
_v6("outside-4096-DR64-regs", "outside", 4096, 14336, REGS, 1, 0, decay_rank=64)


# ---- k47 ----
def _v7(id_, group, base, env, path, kind, w, a, g, v, other=NO_MEGA, other_path=1, **more):
    _row(id_, group, "7", base, "Q4_0", env, path, kind, other, other_path, v7_rank_w=w, v7_rank_a=a, v7_rank_g=g, v7_rank_v=v, **more)


_v7("k47-v7-256-r32", "k47", "test-v7", DEFAULT, 2, 3, 32, 32, 32, 32)
_v7("k47-v7-256-sum256", "k47", "test-v7", DEFAULT, 2, 3, 32, 64, 128, 32)
_v7("k47-v7-256-one-layer", "k47", "test-v7", DEFAULT, 2, 3, 64, 64, 96, 32, n_layer=1)
_v7("k47-v7-256-g160-outside", "k47", "test-v7", DEFAULT, 1, 0, 32, 32, 160, 32, other=NO_FUSED, other_path=0)
_v7("k47-v7-256-w96-outside", "k47", "test-v7", DEFAULT, 1, 0, 96, 32, 32, 32, other=NO_FUSED, other_path=0)
_v7("k47-v7-256-F896-outside", "k47", "test-v7", DEFAULT, 1, 0, 64, 64, 96, 32, other=NO_FUSED, other_path=0, ffn=896)
_v7("k47-v7-2560-r32", "k47", "slice-v7-2560", DEFAULT, 2, 3, 32, 32, 32, 32)
_v7("k47-v7-2560-sum480", "k47", "slice-v7-2560", DEFAULT, 2, 3, 64, 96, 288, 32)
_v7("k47-v7-2560-g352-outside", "k47", "slice-v7-2560", DEFAULT, 1, 0, 96, 96, 352, 64, other=NO_FUSED, other_path=0)
_row("k47-v4-768-F3104-outside", "k47", "4", "slice-v4-768", "Q4_0", DEFAULT, 1, 0, NO_FUSED, 0, ffn=3104)
# ---- the fused launches, and the per-op path on the same file ----
_row("fused-v6-512-F1824-R48-DR128", "fused", "6", "test-v6", "Q4_0", NO_MEGA, 1, 0, NO_FUSED, 0, n_embed=512, ffn=1824, mix_rank=48, decay_rank=128)
_row("fused-v6-1280-F4544-R256", "fused", "6", "test-v6", "Q4_0", NO_MEGA, 1, 0, NO_FUSED, 0, n_embed=1280, ffn=4544, mix_rank=256)
_row("fused-v6-512-R260-declines", "fused", "6", "test-v6", "Q4_0", NO_MEGA, 0, 0, None, 0, n_embed=512, ffn=1824, mix_rank=260)
_row("fused-v6-512-DR32-declines", "fused", "6", "test-v6", "Q4_0", NO_MEGA, 0, 0, None, 0, n_embed=512, ffn=1824, decay_rank=32)
_v7("fused-v7-512-F1056", "fused", "test-v7", NO_MEGA, 1, 0, 128, 64, 256, 96, other=NO_FUSED, other_path=0, n_embed=512, ffn=1056)
_v7("fused-v7-1024-w512", "fused", "test-v7", NO_MEGA, 1, 0, 512, 32, 32, 32, other=NO_FUSED, other_path=0, n_embed=1024, ffn=4096)
_v7("fused-v7-512-w544-declines", "fused", "test-v7", NO_MEGA, 0, 0, 544, 64, 256, 96, other=None, other_path=0, n_embed=512, ffn=1056)
_v7("fused-v7-512-one-layer", "fused", "test-v7", NO_MEGA, 1, 0, 128, 64, 256, 96, other=NO_FUSED, other_path=0, n_embed=512, ffn=1056, n_layer=1)
_row("fused-v4-512-F2048", "fused", "4", "test-v4", "Q4_0", NO_MEGA, 1, 0, NO_FUSED, 0, n_embed=512, ffn=2048)
_row("fused-v4-1280-F3104", "fused", "4", "test-v4", "Q4_0", NO_MEGA, 1, 0, NO_FUSED, 0, n_embed=1280, ffn=3104)
_row("perop-v5.1-512-F1824", "fused", "5.1", "test-v5.1", "Q4_0", NO_MEGA, 0, 0, None, 0, n_embed=512, ffn=1824)
_row("perop-v5.2-512-F1824", "fused", "5.2", "test-v5.2", "Q4_0", NO_MEGA, 0, 0, None, 0, n_embed=512, ffn=1824)
# ---- the bottom of mega_variant: last, and run alone ----
_v6("regs-2048-F32", "regs", 2048, 32, REGS, 2, 1)

CASES = tuple(_ROWS)
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def spec(synth, case):
    base, fields = case.spec
    s = dataclasses.replace(synth.CONFIGS[base], name=case.id, **dict(fields))
    assert s.arch == case.arch
    return s


def representatives():
    """The first row of every (architecture, n_embed) of the table."""
    seen, out = set(), []
    for c in CASES:
        key = (c.arch, dict(c.spec[1]).get("n_embed", c.spec[0]))
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


def ring_admits(D, F, DR, R):
    """csrc/ring_geom.h rg_variant_key, re-derived from the variant table: blocks per F-long row inside the instantiation's step count and
    its gather slots, whole key groups, at most two of them per workgroup."""
    nb = F // 32
    lo, hi, even, dr = {2048: (193, 256, False, 64), 2560: (257, 298, True, 64), 4096: (385, 448, True, 128)}.get(D, (1, 0, False, 0))
    return F % 32 == 0 and lo <= nb <= hi and (not even or nb % 2 == 0) and DR == dr and R in (32, 64)


def mega_admits(D, F, DR, R):
    nb = F // 32
    lo, hi, dr = {2048: (1, 234, 64), 4096: (257, 448, 128)}.get(D, (1, 0, 0))
    return F % 32 == 0 and lo <= nb <= hi and DR == dr and R in (32, 64)
