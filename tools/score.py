#!/usr/bin/env python3
"""Per-position scoring (rwkv_mi_score_resident / rwkv_mi_batch_score_ragged) timed against what there was before it.

    python tools/score.py MODEL_PATH [--config rwkv6-1b6] [--dtype Q4_0] [--T 1024] [--reps 3] [--loop-tokens 128] [--short 32x24] [--out FILE.jsonl]
    python tools/score.py MODEL_PATH --tokens FILE.npy [--ignore-first 0]

MODEL_PATH is written with synth.write_model (seed 42) unless it exists with its ".ok" marker. Host clock around complete calls (each ends
with its stream drained), the smallest of --reps runs after one warm-up run of the same shape, every arm in this process and run. One JSON
record per line, also appended to --out:
  mode score_pass    T tokens from a fresh state three ways:
        score_ms       rwkv_mi_score_resident with targets: log-prob and argmax of every position (8 T bytes come back)
        plain_ms       rwkv_mi_eval_resident of the same T with the last token's logits -- score_ms - plain_ms is what the all-position head costs
        loop_ms        the only way before: one-token rwkv_mi_eval_resident steps with the logits to the host and a NumPy log-softmax there,
                       timed over --loop-tokens tokens and scaled to T (loop_ms_per_token is what was measured)
  mode score_ragged  N short sequences of L tokens (--short NxL): one rwkv_mi_batch_score_ragged pass against N rwkv_mi_score_resident calls
--tokens FILE.npy scores real token ids instead (RWKVModel.perplexity) and prints loss and perplexity with the time of the pass."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("model_path")
    ap.add_argument("--config", default="rwkv6-1b6")
    ap.add_argument("--dtype", default="Q4_0")
    ap.add_argument("--T", type=int, default=1024, help="tokens of the timed pass")
    ap.add_argument("--reps", type=int, default=3, help="timed runs of each arm (the smallest is reported)")
    ap.add_argument("--loop-tokens", type=int, default=128, help="tokens the one-token loop is timed over")
    ap.add_argument("--short", default="32x24", help="NxL: N short sequences of L tokens for the ragged arm (0x0 skips it)")
    ap.add_argument("--tokens", default=None, help="a .npy file of token ids: print their loss and perplexity instead")
    ap.add_argument("--ignore-first", type=int, default=0, help="--tokens: ignore_first_n_tokens of the reference's script")
    ap.add_argument("--out", default=None, help="also append the records to this file")
    args = ap.parse_args()

    import numpy as np
    import __graft_entry__ as graft
    pkg = graft.load_package()
    from rwkv_cpp_amd import synth

    marker = args.model_path + ".ok"
    if not args.tokens and not (os.path.exists(args.model_path) and os.path.exists(marker)):
        t = time.time()
        info = synth.write_model(args.model_path, synth.CONFIGS[args.config], args.dtype, seed=42)
        with open(marker, "w") as f:
            f.write(json.dumps(info))
        print(f"[score] wrote {args.model_path}: {info['bytes'] / 1e9:.2f} GB in {time.time() - t:.1f}s", file=sys.stderr)

    pkg.build_library()
    lib = pkg.load_rwkv_shared_library()
    m = pkg.RWKVModel(lib, args.model_path, thread_count=1, gpu_layer_count=99)
    V = m.n_vocab

    def emit(rec):
        rec.update({"reps": args.reps, "config": args.config, "dtype": args.dtype, "n_vocab": V})
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    def best(run, reset):
        times = []
        for k in range(args.reps + 1):   # (run 0: warm-up -- tile-major weight images, scratch growth, the scoring buffers)
            reset()
            t0 = time.perf_counter()
            run()
            times.append((time.perf_counter() - t0) * 1e3)
        return min(times[1:])

    if args.tokens:
        ids = np.load(args.tokens).astype(np.int64).reshape(-1)
        m.state_load(None)
        t0 = time.perf_counter()
        loss, ppl = m.perplexity(ids, ignore_first_n_tokens=args.ignore_first)
        ms = (time.perf_counter() - t0) * 1e3
        emit({"mode": "perplexity", "tokens": int(ids.size), "ignore_first_n_tokens": args.ignore_first, "loss": loss, "perplexity": ppl,
              "ms": round(ms, 3), "tokens_per_s": round((ids.size - 1) / (ms / 1e3), 1)})
        m.free()
        return

    T = args.T
    toks = np.array([(7 * j + 13) % V for j in range(T + 1)], dtype=np.uint32)
    feed, targets = toks[:-1], toks[1:]

    def fresh():
        m.state_load(None)

    score_ms = best(lambda: m.score_resident(feed, targets), fresh)
    plain_ms = best(lambda: m.eval_resident(feed, want_logits=True), fresh)

    def token_loop():
        total = 0.0
        for i in range(min(args.loop_tokens, T)):
            lg = m.eval_resident(feed[i:i + 1], want_logits=True).astype(np.float64)
            mx = lg.max()
            total += lg[targets[i]] - (mx + np.log(np.exp(lg - mx).sum()))
        return total

    n_loop = min(args.loop_tokens, T)
    loop_ms = best(token_loop, fresh) / n_loop
    # the three arms agree on what they compute: the loop's sum of log-probs against the pass's (float64 host softmax vs the kernel's f32 results)
    m.state_load(None)
    lp, _, _ = m.score_resident(feed, targets)
    m.state_load(None)
    loop_sum = token_loop()
    emit({"mode": "score_pass", "T": T, "score_ms": round(score_ms, 3), "plain_ms": round(plain_ms, 3), "head_all_positions_ms": round(score_ms - plain_ms, 3),
          "loop_ms_per_token": round(loop_ms, 4), "loop_tokens": n_loop, "loop_ms": round(loop_ms * T, 3),
          "score_tokens_per_s": round(T / (score_ms / 1e3), 1), "plain_tokens_per_s": round(T / (plain_ms / 1e3), 1),
          "loop_tokens_per_s": round(1e3 / loop_ms, 1), "score_over_loop": round(loop_ms * T / score_ms, 2),
          "sum_logprob_first_loop_tokens": float(lp[:n_loop].astype(np.float64).sum()), "sum_logprob_loop": float(loop_sum), "decode_path": m.decode_path()})

    N, L = (int(x) for x in args.short.split("x"))
    if N and L:
        seqs = [np.array([(11 * i + 7 * j + 3) % V for j in range(L + 1)], dtype=np.uint32) for i in range(N)]
        b = pkg.RWKVBatch(m, N)
        slots = list(range(N))

        def fresh_slots():
            for s in slots:
                b.state_load(s, None)

        def one_by_one():
            for s in seqs:
                m.state_load(None)
                m.score_resident(s[:-1], s[1:])

        r_ms = best(lambda: b.score_ragged(slots, [s[:-1] for s in seqs], [s[1:] for s in seqs]), fresh_slots)
        s_ms = best(one_by_one, fresh)
        emit({"mode": "score_ragged", "N": N, "L": L, "T": N * L, "ragged_ms": round(r_ms, 3), "separate_ms": round(s_ms, 3),
              "separate_over_ragged": round(s_ms / r_ms, 2), "ragged_tokens_per_s": round(N * L / (r_ms / 1e3), 1)})
        b.free()
    m.free()


if __name__ == "__main__":
    main()
