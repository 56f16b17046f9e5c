"""Model files with head sizes other than 64. TEST INFRASTRUCTURE ONLY (a helper module; tests/test_cpu_head_sizes.py holds the oracle to
float64 on every file made here, tests/test_gpu_head_sizes.py holds every recurrence form of the GPU to the oracle on them).

synth.CONFIGS has head size 64 only and the tiny golden files have (H, S) = (8, 8), (16, 8) and (1, 64). The loader takes head_size =
n_embed / head_count from the shape of att.time_decay or att.r_k, so a file of any S that divides D loads; ROWS are the shapes that reach
the S = 32 and S = 16 instantiations of the recurrence kernels and their generic forms (csrc/kernels.hip: launch_wkv6, launch_wkv7,
launch_draft_replay):

  arch  D     S    H   what it reaches
  5.1   256   32   8   wkv6<32>, u and w per head (u_per_chan 0, w_mode 0)
  5.2   256   16   16  wkv6<16>, per channel (1 / 1)
  6     256   32   8   wkv6<32>, w_mode 2
  6     768   96   8   generic; S no power of two; the lanes of the group norm unevenly loaded (32 lanes carry two elements, 32 one)
  6     256   128  2   generic; two elements per lane
  6     1024  512  2   generic with the 256-thread loop taken twice
  7     256   32   8   wkv7<32>
  7     256   16   16  generic (RWKV-7 has no 16 instantiation)
  7     768   96   8   generic, the kprep / bonus sums over 96
  7     256   128  2   generic
  7     1024  512  2   generic, strided

ffn is the base configuration's ffn * D / 256, every other rank that of test-v6 / test-v7, the vocabulary 512; 2 layers, 3 on RWKV-7 so that
v_first is used. The two D = 1024 rows are `big`: stressed weights only, and only the plain, sequence and row forms."""
import dataclasses
import os
import shutil

import stress_lib as S

SEED = 7
FORMATS = ("Q5_1", "FP16")
BASE = {"5.1": "test-v5.1", "5.2": "test-v5.2", "6": "test-v6", "7": "test-v7"}
# (arch, D, S)
ROWS = [("5.1", 256, 32), ("5.2", 256, 16),
        ("6", 256, 32), ("6", 768, 96), ("6", 256, 128), ("6", 1024, 512),
        ("7", 256, 32), ("7", 256, 16), ("7", 768, 96), ("7", 256, 128), ("7", 1024, 512)]


def is_big(row):
    return row[1] == 1024


def row_id(row):
    return f"v{row[0]}-D{row[1]}-S{row[2]}"


def weights_of(row):
    return ("stress",) if is_big(row) else ("plain", "stress")


def spec(synth, row):
    arch, D, S_ = row
    base = synth.CONFIGS[BASE[arch]]
    assert base.n_embed == 256 and D % S_ == 0 and (base.ffn * D) % 256 == 0
    return dataclasses.replace(base, n_embed=D, head_size=S_, ffn=base.ffn * D // 256, n_layer=3 if arch == "7" else 2, n_vocab=512, name=row_id(row))


class Files:
    """(row, fmt, weights) -> path: each file is written once, the stressed one as a rewritten copy of the plain one; close() removes them."""

    def __init__(self, synth, base):
        self.synth, self.base, self.made = synth, str(base), {}

    def __call__(self, row, fmt, weights):
        plain = (row, fmt, "plain")
        if plain not in self.made:
            p = os.path.join(self.base, f"{row_id(row)}-{fmt}-plain.bin")
            self.synth.write_model(p, spec(self.synth, row), fmt, seed=SEED)
            self.made[plain] = p
        if (row, fmt, weights) not in self.made:
            p = os.path.join(self.base, f"{row_id(row)}-{fmt}-stress.bin")
            shutil.copyfile(self.made[plain], p)
            done = S.rewrite_f32_vectors(p, S.stress_vectors(row[0], SEED))
            assert set(done) == S.expected_names(row[0], spec(self.synth, row).n_layer), (row, sorted(done))
            self.made[(row, fmt, weights)] = p
        return self.made[(row, fmt, weights)]

    def close(self):
        for p in self.made.values():
            os.remove(p)
        self.made = {}
