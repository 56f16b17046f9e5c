"""Child process of tests/test_gpu_batch_until.py: one sampled rwkv_mi_batch_decode_until call on a fresh batch in a fresh process
(RWKV_MI_LOOP_BLOCK is read at the call; the parent sets it in this process's environment).
usage: until_worker.py MODEL SPEC.json OUT.npz     (SPEC: what test_gpu_batch_until._spec() wrote)"""
import json
import sys

import numpy as np

from gpu_lib import model, pkg
from test_gpu_batch_until import N_SLOTS, _prepare, _until


def main():
    path, spec_path, out = sys.argv[1:4]
    spec = json.load(open(spec_path))
    m = model(path)
    b = pkg.RWKVBatch(m, N_SLOTS)
    _prepare(b, spec["family"], m.n_vocab)
    toks, lens, why = _until(b, spec["family"], spec["slots"], spec["first"], spec["max_tokens"], spec["stop"], stride=spec["stride"])
    np.savez(out, tokens=toks, lens=lens, why=why, passes=b.last_loop_passes(), states=np.stack([b.state_store(s) for s in spec["slots"]]))
    b.free()
    m.free()


if __name__ == "__main__":
    main()
