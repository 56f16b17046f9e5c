"""Child process of tests/test_gpu_score.py: one rwkv_mi_score_resident call on a fresh context in a fresh process (RWKV_MI_SCORE_ROWS is read
when a context's first scoring call allocates the head's chunk, so the parent sets it in this process's environment).
usage: score_worker.py MODEL TOKENS.npy OUT.npz     (the targets are the tokens moved on by one, the last position is not scored)"""
import sys

import numpy as np

from gpu_lib import model, pkg


def main():
    path, tokens_path, out = sys.argv[1:4]
    tokens = np.load(tokens_path).astype(np.uint32)
    targets = np.concatenate([tokens[1:], np.array([pkg.NO_TARGET], dtype=np.uint32)])
    m = model(path)
    logprobs, argmax, logits = m.score_resident(tokens, targets, want_argmax=True, want_logits=True)
    np.savez(out, logprobs=logprobs, argmax=argmax, logits=logits, state=m.state_store(), last=m.logits_store())
    m.free()


if __name__ == "__main__":
    main()
