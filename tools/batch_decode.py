#!/usr/bin/env python3
"""Batched greedy decode (rwkv_mi_batch_decode_greedy) swept over the batch size, against single-stream rwkv_mi_decode_greedy.

    python tools/batch_decode.py MODEL_PATH [--config rwkv6-7b] [--dtype Q4_0] [--n 1,2,4,...] [--tokens 32] [--warmup 4]

MODEL_PATH is written with synth.write_model (seed 42) unless it exists with its ".ok" marker. Prints one JSON record per n:
  ms_per_step           one batched step (n tokens, one pass over the weights), from HIP events around the device loop
  tokens_per_s          aggregate n / step time; per_seq_tokens_per_s = 1 / step time
  alg_bytes_per_step    weights once + n x (state read + write + embedding row + logits), from shapes
  step_fraction_of_8TBs that figure over the step time, as a fraction of 8 TB/s -- a figure of the whole step, not of one kernel
and first one record with the single-stream rate measured in the same process.

--sample adds, beside each greedy record, the sampling loop two ways (temperature 1.0, top-p 0.8, seed = row, the same number of steps):
  mode batch_sample        rwkv_mi_batch_decode_sample, the loop on the device (HIP events, as the greedy loop); sampler_ms_per_step is
                           its step minus the greedy step of the same n
  mode batch_host_sample   what has to be done without it: RWKVBatch.eval with the logits to the host, then sample_probs of the
                           reference's python/sampling.py restated in NumPy on each row; host clock around the loop

--sample --penalties adds two more arms in the same run, shapes and n (presence 0.2, frequency 0.2 -- the reference chat program's defaults --
every step recorded), and appends its records to --out when given:
  mode batch_sample_penalized       rwkv_mi_batch_decode_sample_penalized, the loop on the device; penalty_ms_per_step is its step minus the
                                    plain sampled step of the same n and run
  mode batch_host_sample_penalized  the host path doing the same job: the logits to the host, chat_with_bot.py:246-247 on each row, then
                                    sample_probs in NumPy; host clock around the loop

--ragged times the ragged pass (rwkv_mi_batch_eval_ragged*) instead, host clock around complete calls (each ends with its stream drained),
the smallest of --reps runs after one warm-up run of the same shape, both sides in this process and run; records also go to --out:
  mode ragged_ingest   N prompts of L tokens: one ragged pass (logits of every prompt's last token to the host) against the way without
                       it, N x (rwkv_mi_eval_resident on a context with its logits, then rwkv_mi_batch_state_from_context)
  mode ragged_join     a 64-row decode step (sampled on the device, temperature 0) that also carries prompt chunks, against the same
                       decode step alone plus the chunks pre-filled on a context and copied in

--until times rwkv_mi_batch_decode_until (sampled family: temperature 1.0, top-p 0.8, seed = row) against the unchanged plain loop in the same
process, HIP events around each device loop, the smallest of --reps runs, --tokens steps (the budget); records also go to --out:
  mode until_no_stop      (a) no stop met, every budget = --tokens, for RWKV_MI_LOOP_BLOCK in 4, 16, 64: ms per step against
                          rwkv_mi_batch_decode_sample's -- the price of the live words, the stop kernel and the block hand-shake
  mode until_half_retire  (b) every second row retires at a quarter of the budget, against (a) at the default block: what dead rows cost
  mode until_all_retire   (c) every row retires at a quarter of the budget, against the plain loop of the full budget, with last_loop_passes
  mode until_eval_sample  the way without either loop: one synchronising rwkv_mi_batch_eval_sample call per token, host clock

--serve times rwkv_mi_batch_serve (sampled family: temperature 1.0, top-p 0.8, seed = request) on a fixed, seeded queue of 4 n requests with
budgets spread over 16 .. 256 and prompts of 1 .. 32 tokens, for every n of --n (give --n 8,64), the smallest of --reps runs after a warm-up
run, everything in this process and run; records also go to --out:
  mode serve            the queue on n lanes: host clock around the call (and the HIP events' figure), useful tokens/s, passes enqueued
  mode serve_waves      the same queue statically batched, n requests at a time: rwkv_mi_batch_eval_ragged of the prompts but their last
                        tokens, then rwkv_mi_batch_decode_until until the slowest has ended; host clock around those calls
  mode serve_admission  the mean time of a pass that admits (every lane, every pass: one prompt token, a budget of one) against one that
                        does not (n requests of the same number of passes), and the difference per admission
--session times the serve session (rwkv_mi_batch_serve_open ..) on the same queue: the whole queue submitted before the first poll against
serve (modes serve, session_upfront), and the queue revealed in groups of n -- group g + 1 at the poll that delivers the end of half of
group g -- against one closed serve call per group (modes closed_groups, session_arrivals); both arms emit the same tokens
(same_tokens_as_serve), and every record of a session carries the bytes it fetches per block and the median host time of a poll.
--serve --guide and --serve --logprobs N time rwkv_mi_batch_serve_ex on the same queue -- every request under a guide of four states, each
allowing a random half of the vocabulary, or the batch's report on at top_n N (both flags: both) -- against the same waves with the guide
attached to the lanes or the report on, the only way to either before that call; no admission record:
  mode serve_guide / serve_logprobs [/ serve_guide_logprobs]   as mode serve
  mode ..._waves        as mode serve_waves, with same_tokens_as_serve and, with the report, same_chosen_as_serve (the log-probs, bit for bit)

--sample --logprobs N[,N...] times the sampled loop (temperature 1.0, top-p 0.8, seed = row) with and without the report of the emitted tokens
(rwkv_mi_batch_set_logprobs) in the same process, HIP events around each device loop, the smallest of --reps runs, --tokens steps, for every
top_n of the list; records also go to --out:
  mode logprobs_report   ms per step with the report at this top_n, the same run's step without it, and their difference
  mode logprobs_host     the way without it: RWKVBatch.eval with the logits to the host, then a float64 log-softmax and np.argpartition for
                         the largest top_n of the list on each row, the token taken as its argmax; host clock around the loop

--sample --guide times the sampled loop (temperature 1.0, top-p 0.8, seed = row) three ways in the same process, --tokens steps, the smallest of
--reps runs (the plain loop also with its largest run: the run-to-run spread of the box), under a guide of 4 states that each allow a random half
of the vocabulary; records also go to --out:
  mode guide_plain    (a) rwkv_mi_batch_decode_sample with no guide attached, HIP events around the device loop -- the only arm when the library
                      loaded through RWKV_LIB_DIR is a build without guides
  mode guide_device   (b) the same loop with the guide attached to every row; guide_ms_per_step is its step minus (a)'s
  mode guide_host     (c) the way without guides: per token and row rwkv_mi_batch_logit_bias_set with -inf on every forbidden id, one
                      rwkv_mi_batch_eval_sample_penalized pass, the token read back, the automaton stepped on the host; host clock

--sample --cut K[,K...] times the sampled loop (temperature 1.0, top-p 0.8, seed = row) under truncation settings (rwkv_mi_batch_truncation_set)
in the same process, --tokens steps, HIP events around each device loop, the smallest of --reps runs (the loop without a setting also with its
largest run: the run-to-run spread of the box); sampler_ms_per_step is a loop's step minus the greedy loop's of the same n and run; records
also go to --out:
  mode cut_plain    rwkv_mi_batch_decode_sample with no setting on any slot -- the only arm when the library loaded through RWKV_LIB_DIR is a
                    build without the settings
  mode cut_device   the same loop with every slot set to {K, 0} for each K of the list, to {0, 0.05}, and to {the first K, 0.05}
  mode cut_host     the host path doing the same job: RWKVBatch.eval with the logits to the host, then in NumPy the top-k mask (argpartition),
                    softmax, the top-p cut-off intersected with min-p, the draw; host clock around the loop

--sample --penalties --decay D[,D...] [--repetition R] times the penalised loop (temperature 1.0, top-p 0.8, seed = row, presence 0.2, frequency
0.2, every step recorded) under repetition settings (rwkv_mi_batch_repetition_set) in the same process, --tokens steps, HIP events around each
device loop, the smallest of --reps runs (the loop without a setting also with its largest run: the run-to-run spread of the box); records also
go to --out:
  mode decay_plain    rwkv_mi_batch_decode_sample_penalized with no setting on any slot -- the only arm when the library loaded through
                      RWKV_LIB_DIR is a build without the settings
  mode decay_device   the same loop with every slot set to {D, 1} for each D of the list, to {1, R}, and to {the first D, R}; setting_ms_per_step
                      is its step minus decay_plain's
  mode decay_host     the host path doing the same job: RWKVBatch.eval with the logits to the host, then in NumPy the decayed float table, the
                      repetition and presence / frequency penalty on it, sample_probs; host clock around the loop

--beam W[,W...] times rwkv_mi_batch_decode_beam (no end tokens, --tokens steps) for every width of the list, G = rows // W groups at the largest
row count of --n, HIP events around each device loop, the smallest of --reps runs; records also go to --out:
  mode beam        ms per step of the beam loop beside the greedy loop's at the same row count from the same run, and their difference
  mode beam_host   the search driven from the host with the calls that existed before: RWKVBatch.eval with the logits to the host, a float64
                   log-softmax and the W best of each row, the selection, the states permuted with state_store / state_load; host clock

--draft K[,K...] times rwkv_mi_batch_eval_draft for every draft length of the list and every n, greedy and sampled (temperature 1.0, top-p 0.8,
seed = row), host clock around complete calls (each ends with its stream drained), the smallest of --reps runs after a warm-up run, everything
in this process and run; records also go to --out. Drafts are cut from the true continuation, computed ahead with the plain loop, and corrupted
so that exactly a tokens per row stand -- synthetic weights give no meaningful natural acceptance rate:
  mode draft_plain      the plain device loops of the same n (HIP events): what the draft call has to beat
  mode draft_overhead   one call of n rows of 1 + K tokens, every draft standing (nothing replayed) and none standing (every row replayed),
                        against rwkv_mi_batch_eval_ragged_sample of the same shape -- the only arm when the library loaded through RWKV_LIB_DIR
                        is a build without the call: the difference is the stash, the head on every token, the choice and the replay
  mode draft_accept     --tokens successive calls with a in 0, 1, 2, 4, 8 (a <= K) tokens standing per row: tokens/s against the plain loop's,
                        and break_even_a = call time / plain step time - 1, the acceptance from which the call wins
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_BS = 8.0e12


def host_sample(logits, temperature, top_p, rng):
    """The reference's sample_probs on one row of logits (softmax, top-p cut-off, temperature power, renormalise, draw), NumPy on the host."""
    import numpy as np
    x = logits - logits.max()
    probs = np.exp(x)
    probs /= probs.sum()
    if top_p == 0.0:
        top_p = 1.0
    if temperature == 0.0:
        return int(np.argmax(probs))
    if top_p < 1.0:
        sorted_probs = np.sort(probs)[::-1]
        cutoff = float(sorted_probs[np.argmax(np.cumsum(sorted_probs) > top_p)])
        probs[probs < cutoff] = 0
    if temperature != 1.0:
        probs = np.power(probs, 1.0 / temperature)
    probs = probs / probs.sum()
    return int(rng.choice(a=len(probs), p=probs))


def ragged(pkg, m, args):
    V = m.n_vocab
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        rec.update({"reps": args.reps, "config": args.config, "dtype": args.dtype})
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def prompt(i, L):
        return [(7 * i + 13 * j + 1) % V for j in range(L)]

    def best(run, reset):
        times = []
        for k in range(args.reps + 1):   # (run 0: warm-up -- tile-major weight images, scratch growth)
            reset()
            t0 = time.perf_counter()
            run()
            times.append((time.perf_counter() - t0) * 1e3)
        return min(times[1:])

    def prefill_and_copy(b, slot, toks):
        m.eval_resident(toks, want_logits=True)
        b.from_context(slot, m)

    b = pkg.RWKVBatch(m, 66)
    for N in (1, 8, 32):
        for L in (16, 128, 512):
            slots = list(range(N))
            prompts = [prompt(i, L) for i in slots]

            def fresh():
                for s in slots:
                    b.state_load(s, None)
                m.state_load(None)

            def separate():
                for i in slots:
                    if i:
                        m.state_load(None)   # (a new request starts from the fresh state; part of this way of doing it)
                    prefill_and_copy(b, i, prompts[i])

            r_ms = best(lambda: b.eval_ragged(slots, prompts), fresh)
            s_ms = best(separate, fresh)
            emit({"mode": "ragged_ingest", "N": N, "L": L, "T": N * L, "ragged_ms": round(r_ms, 3), "separate_ms": round(s_ms, 3),
                  "separate_over_ragged": round(s_ms / r_ms, 2), "ragged_tokens_per_s": round(N * L / (r_ms / 1e3), 1)})

    dec = list(range(64))
    dec_toks = [(7 * i + 1) % V for i in dec]

    def fresh_all():
        for s in range(66):
            b.state_load(s, None)
        m.state_load(None)

    d_ms = best(lambda: b.eval_sample(dec, dec_toks, 0.0, 0.8, -1.0, 0), fresh_all)
    for chunks in ([64], [512], [64, 512]):
        extra = list(range(64, 64 + len(chunks)))
        rows = [[t] for t in dec_toks] + [prompt(s, L) for s, L in zip(extra, chunks)]

        def separate():
            b.eval_sample(dec, dec_toks, 0.0, 0.8, -1.0, 0)
            for s, L in zip(extra, chunks):
                if s != extra[0]:
                    m.state_load(None)
                prefill_and_copy(b, s, prompt(s, L))

        r_ms = best(lambda: b.eval_ragged_sample(dec + extra, rows, 0.0, 0.8, -1.0, 0), fresh_all)
        s_ms = best(separate, fresh_all)
        emit({"mode": "ragged_join", "decode_rows": 64, "chunks": chunks, "T": 64 + sum(chunks), "decode_step_alone_ms": round(d_ms, 3),
              "ragged_ms": round(r_ms, 3), "chunk_cost_in_the_pass_ms": round(r_ms - d_ms, 3), "separate_ms": round(s_ms, 3),
              "chunk_cost_separate_ms": round(s_ms - d_ms, 3), "separate_over_ragged": round(s_ms / r_ms, 2)})
    b.free()
    if sink:
        sink.close()


def until(pkg, m, args):
    V = m.n_vocab
    sink = open(args.out, "a") if args.out else None
    steps = args.tokens
    quarter = max(1, steps // 4)

    def emit(rec):
        rec.update({"steps": steps, "reps": args.reps, "temperature": 1.0, "top_p": 0.8, "config": args.config, "dtype": args.dtype})
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    ns = [int(x) for x in args.n.split(",")]
    b = pkg.RWKVBatch(m, max(ns))
    for n in ns:
        slots = list(range(n))
        first = [(7 * i + 1) % V for i in slots]

        def best(run):
            out = []
            for k in range(args.reps + 1):   # (run 0: warm-up -- buffers of the first call, tile-major weight images)
                for s in slots:
                    b.state_load(s, None)
                out.append(run())
            return min(out[1:])

        plain_ms = best(lambda: b.decode_sample(slots, first, steps, 1.0, 0.8, slots)[1])
        by_block = {}
        for block in (4, 16, 64):
            os.environ["RWKV_MI_LOOP_BLOCK"] = str(block)
            by_block[block] = best(lambda: b.decode_until(slots, first, steps, None, 1.0, 0.8, slots)[2])
            emit({"mode": "until_no_stop", "n": n, "block": block, "ms_per_step": round(by_block[block] / steps, 4),
                  "plain_ms_per_step": round(plain_ms / steps, 4), "until_over_plain": round(by_block[block] / plain_ms, 4), "passes": b.last_loop_passes()})
        os.environ.pop("RWKV_MI_LOOP_BLOCK", None)
        half = [quarter if i % 2 else steps for i in slots]
        half_ms = best(lambda: b.decode_until(slots, first, half, None, 1.0, 0.8, slots)[2])
        emit({"mode": "until_half_retire", "n": n, "retire_at": quarter, "retiring_rows": sum(1 for i in slots if i % 2), "ms_per_step": round(half_ms / steps, 4),
              "no_stop_ms_per_step": round(by_block[16] / steps, 4), "half_over_no_stop": round(half_ms / by_block[16], 4), "passes": b.last_loop_passes()})
        all_ms = best(lambda: b.decode_until(slots, first, quarter, None, 1.0, 0.8, slots)[2])
        emit({"mode": "until_all_retire", "n": n, "retire_at": quarter, "ms": round(all_ms, 3), "plain_full_budget_ms": round(plain_ms, 3),
              "plain_over_until": round(plain_ms / all_ms, 2), "passes": b.last_loop_passes()})

        def per_token():
            toks = list(first)
            t0 = time.perf_counter()
            for _ in range(steps):
                toks = [int(t) for t in b.eval_sample(slots, toks, 1.0, 0.8, -1.0, slots)]
            return (time.perf_counter() - t0) * 1e3

        call_ms = best(per_token)
        emit({"mode": "until_eval_sample", "n": n, "ms_per_step": round(call_ms / steps, 4), "until_ms_per_step": round(by_block[16] / steps, 4),
              "per_token_calls_over_until": round(call_ms / by_block[16], 3)})
    b.free()
    if sink:
        sink.close()


def serve(pkg, m, args):
    import numpy as np
    V = m.n_vocab
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        rec.update({"reps": args.reps, "temperature": 1.0, "top_p": 0.8, "config": args.config, "dtype": args.dtype})
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def best(run):
        out = [run() for _ in range(args.reps + 1)]   # (run 0: warm-up -- buffers of the first call, tile-major weight images)
        return min(out[1:], key=lambda r: r[0])

    # the arm: the plain queue, or -- what only waves of decode_until gave before rwkv_mi_batch_serve_ex -- every request under a guide
    # (--guide: a few states, each allowing a random half of the vocabulary, as --sample --guide builds it) or the batch's report on
    # (--logprobs N)
    guided = bool(args.guide)
    top_n = int(args.logprobs.split(",")[0]) if args.logprobs else None
    arm = "serve" + ("_guide" if guided else "") + ("_logprobs" if top_n is not None else "")
    n_states = 4
    grng = np.random.default_rng(7)
    edges = [{int(t): int(grng.integers(0, n_states)) for t in np.flatnonzero(grng.random(V) < 0.5)} for _ in range(n_states)] if guided else None

    for n in [int(x) for x in args.n.split(",")]:
        R = 4 * n
        rng = np.random.default_rng(1000 + n)   # the queue is fixed by n
        budgets = [int(v) for v in rng.integers(16, 257, R)]
        prompts = [[int(t) for t in rng.integers(0, V, int(L))] for L in rng.integers(1, 33, R)]
        reqs = [dict(prompt=prompts[q], max_tokens=budgets[q], temperature=1.0, top_p=0.8, seed=q) for q in range(R)]
        useful = sum(budgets)   # (no stop sequences: every request runs to its budget, in both arms)
        lanes = list(range(n))
        b = pkg.RWKVBatch(m, n)
        if guided:
            gid = b.create_guide(edges)
            for q in range(R):
                reqs[q].update(guide=gid, guide_state=q % n_states)
        if top_n is not None:
            b.set_logprobs(top_n)

        def served():
            for s in lanes:
                if guided:
                    b.detach_guide(s)   # (the waves attach: a lane brings no guide of its own)
            t0 = time.perf_counter()
            got = b.serve(lanes, reqs, pkg.SERVE_SAMPLE, report=top_n is not None)
            host = (time.perf_counter() - t0) * 1e3
            assert [len(t) for t in got["tokens"]] == budgets
            chosen = [row[:budgets[q]] for q, row in enumerate(b.logprobs()[0])] if top_n is not None else []
            return host, got["elapsed_ms"], b.last_loop_passes(), got["tokens"], chosen

        def waves():
            # the same queue statically batched: n requests at a time, prompts in one ragged pass, then the loop until the slowest has ended
            host, passes, toks, chosen = 0.0, 0, [], []
            for w in range(0, R, n):
                for s in lanes:
                    b.state_load(s, None)
                    if guided:
                        b.attach_guide(s, gid, (w + s) % n_states)
                t0 = time.perf_counter()
                long = [s for s in lanes if len(prompts[w + s]) > 1]
                if long:
                    b.eval_ragged(long, [prompts[w + s][:-1] for s in long], want_logits=False)
                    passes += 1
                out, _, _ = b.decode_until(lanes, [prompts[w + s][-1] for s in lanes], budgets[w: w + n], None, 1.0, 0.8, list(range(w, w + n)))
                host += (time.perf_counter() - t0) * 1e3
                passes += b.last_loop_passes()
                toks.extend(out)
                if top_n is not None:
                    chosen.extend(row[:budgets[w + s]] for s, row in enumerate(b.logprobs()[0]))
            return host, passes, toks, chosen

        s_host, s_dev, s_passes, s_toks, s_chosen = best(served)
        w_host, w_passes, w_toks, w_chosen = best(waves)
        same = all(np.array_equal(a, c) for a, c in zip(s_toks, w_toks))
        extra = {}
        if top_n is not None:
            extra = {"top_n": top_n, "same_chosen_as_serve": bool(all(np.array_equal(a.view(np.uint32), c.view(np.uint32)) for a, c in zip(s_chosen, w_chosen)))}
        emit({"mode": arm, "n": n, "requests": R, "useful_tokens": useful, "total_ms": round(s_host, 3), "device_ms": round(s_dev, 3), "passes": s_passes,
              "useful_tokens_per_s": round(useful / s_host * 1e3, 1), "ms_per_pass": round(s_dev / s_passes, 4)})
        emit({"mode": arm + "_waves", "n": n, "requests": R, "useful_tokens": useful, "total_ms": round(w_host, 3), "passes": w_passes,
              "useful_tokens_per_s": round(useful / w_host * 1e3, 1), "waves_over_serve": round(w_host / s_host, 3), "same_tokens_as_serve": bool(same), **extra})
        if arm != "serve":
            b.free()
            continue

        # what an admission costs: a queue in which EVERY pass admits all n lanes (one prompt token, one token) against a call of n requests
        # that admits none after the first pass. Both retire their last request after pass steps - 1, so both enqueue the same passes (the dead
        # ones behind the last retirement included, which cost what a pass without an admission costs): the difference is the admissions'
        steps = 32
        churn = [dict(prompt=[(7 * q + 1) % V], max_tokens=1, temperature=1.0, top_p=0.8, seed=q) for q in range(steps * n)]
        steady = [dict(prompt=[(7 * q + 1) % V], max_tokens=steps, temperature=1.0, top_p=0.8, seed=q) for q in range(n)]

        def timed(queue):
            def run():
                got = b.serve(lanes, queue, pkg.SERVE_SAMPLE)
                return got["elapsed_ms"], b.last_loop_passes()
            return best(run)

        (admit_ms, admit_passes), (plain_ms, plain_passes) = timed(churn), timed(steady)
        assert admit_passes == plain_passes, (admit_passes, plain_passes)
        plain_pass = plain_ms / plain_passes
        emit({"mode": "serve_admission", "n": n, "admitting_passes": steps, "passes": plain_passes, "plain_pass_ms": round(plain_pass, 4),
              "admitting_pass_ms": round(plain_pass + (admit_ms - plain_ms) / steps, 4), "ms_per_admission": round((admit_ms - plain_ms) / (steps * n), 5),
              "state_mb": round(m.state_len * 4 / 1e6, 2)})
        b.free()
    if sink:
        sink.close()


def session(pkg, m, args):
    """--session: the serve session (rwkv_mi_batch_serve_open ..) on the queue of --serve, two arms per n. `session_upfront`: the whole queue
    submitted before the first poll, against `serve` on the same queue. `session_arrivals`: the queue revealed in groups of n, group g + 1
    submitted at the poll that delivers the end of half of group g, against one closed `serve` call per group, each after the one before
    has returned (`closed_groups`). Passes from submit to first token: the pass that draws a request's first token minus the passes
    enqueued when it was submitted (closed arm: when half of the group before had ended)."""
    import numpy as np
    V = m.n_vocab
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        rec.update({"reps": args.reps, "temperature": 1.0, "top_p": 0.8, "config": args.config, "dtype": args.dtype, "loop_block": int(os.environ.get("RWKV_MI_LOOP_BLOCK", 16))})
        if args.run:
            rec["run"] = args.run
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def best(run):
        out = [run() for _ in range(args.reps + 1)]   # (run 0: warm-up)
        return min(out[1:], key=lambda r: r[0])

    for n in [int(x) for x in args.n.split(",")]:
        R = 4 * n
        rng = np.random.default_rng(1000 + n)   # the queue of --serve
        budgets = [int(v) for v in rng.integers(16, 257, R)]
        prompts = [[int(t) for t in rng.integers(0, V, int(L))] for L in rng.integers(1, 33, R)]
        reqs = [dict(prompt=prompts[q], max_tokens=budgets[q], temperature=1.0, top_p=0.8, seed=q) for q in range(R)]
        useful = sum(budgets)
        lanes = list(range(n))
        b = pkg.RWKVBatch(m, n)
        limits = dict(capacity=R, max_prompt=32, stride=256, max_seqs=0, max_seq_tokens=0, features=0)
        fetch_bytes = 4 * (2 + n + R * (8 + 256))

        def in_session(groups):
            """groups: lists of request numbers; group g + 1 is submitted at the poll that delivers the end of half of group g"""
            toks, first_at, submit_at, ended, poll_ms = {}, {}, {}, set(), []
            t0 = time.perf_counter()
            with b.serve_open(lanes, pkg.SERVE_SAMPLE, **limits) as s:
                nxt = 0
                while len(ended) < R:
                    while nxt < len(groups) and (nxt == 0 or 2 * len(ended & set(groups[nxt - 1])) >= len(groups[nxt - 1])):
                        at = s.stats()["passes"]
                        for q in groups[nxt]:
                            assert s.submit(**reqs[q]) == len(submit_at)
                            submit_at[q] = at
                        nxt += 1
                    order = [q for g in groups[:nxt] for q in g]   # (id -> request number)
                    p0 = time.perf_counter()
                    events = s.poll()
                    poll_ms.append((time.perf_counter() - p0) * 1e3)
                    for e in events:
                        q = order[e["id"]]
                        toks.setdefault(q, []).extend(e["tokens"].tolist())
                        first_at.setdefault(q, e["start_pass"] + len(prompts[q]) - 1)
                        if e["finished"]:
                            ended.add(q)
                passes = s.stats()["passes"]
            host = (time.perf_counter() - t0) * 1e3
            assert [len(toks[q]) for q in range(R)] == budgets
            wait = float(np.mean([first_at[q] - submit_at[q] + 1 for q in range(R)]))
            return host, passes, [toks[q] for q in range(R)], wait, float(np.median(poll_ms)), len(poll_ms)

        def closed(groups):
            host, base, toks, first_at, submit_at, half = 0.0, 0, {}, {}, {}, 0
            for g in groups:
                t0 = time.perf_counter()
                got = b.serve(lanes, [reqs[q] for q in g], pkg.SERVE_SAMPLE)
                host += (time.perf_counter() - t0) * 1e3
                ends = []
                for i, q in enumerate(g):
                    toks[q] = got["tokens"][i].tolist()
                    submit_at[q] = half
                    first_at[q] = base + int(got["start_pass"][i]) + len(prompts[q]) - 1
                    ends.append(base + int(got["start_pass"][i]) + len(prompts[q]) - 1 + len(toks[q]))
                half = sorted(ends)[(len(g) + 1) // 2 - 1]   # the passes enqueued when half of this group had ended: the next group exists from then on
                base += b.last_loop_passes()
            wait = float(np.mean([first_at[q] - submit_at[q] + 1 for q in range(R)]))
            return host, base, [toks[q] for q in range(R)], wait

        whole, groups = [list(range(R))], [list(range(g, g + n)) for g in range(0, R, n)]
        s_host, s_passes, s_toks, s_wait = best(lambda: closed(whole))
        u_host, u_passes, u_toks, u_wait, u_poll, u_polls = best(lambda: in_session(whole))
        emit({"mode": "serve", "n": n, "requests": R, "useful_tokens": useful, "total_ms": round(s_host, 3), "passes": s_passes, "useful_tokens_per_s": round(useful / s_host * 1e3, 1)})
        emit({"mode": "session_upfront", "n": n, "requests": R, "useful_tokens": useful, "total_ms": round(u_host, 3), "passes": u_passes,
              "useful_tokens_per_s": round(useful / u_host * 1e3, 1), "session_over_serve": round(u_host / s_host, 4), "same_tokens_as_serve": bool(u_toks == s_toks),
              "fetch_bytes_per_block": fetch_bytes, "poll_ms_median": round(u_poll, 4), "polls": u_polls})
        c_host, c_passes, c_toks, c_wait = best(lambda: closed(groups))
        a_host, a_passes, a_toks, a_wait, a_poll, a_polls = best(lambda: in_session(groups))
        emit({"mode": "closed_groups", "n": n, "requests": R, "groups": len(groups), "useful_tokens": useful, "total_ms": round(c_host, 3), "passes": c_passes,
              "useful_tokens_per_s": round(useful / c_host * 1e3, 1), "passes_to_first_token": round(c_wait, 2), "same_tokens_as_serve": bool(c_toks == s_toks)})
        emit({"mode": "session_arrivals", "n": n, "requests": R, "groups": len(groups), "useful_tokens": useful, "total_ms": round(a_host, 3), "passes": a_passes,
              "useful_tokens_per_s": round(useful / a_host * 1e3, 1), "passes_to_first_token": round(a_wait, 2), "same_tokens_as_serve": bool(a_toks == s_toks),
              "closed_over_session": round(c_host / a_host, 3), "fetch_bytes_per_block": fetch_bytes, "poll_ms_median": round(a_poll, 4), "polls": a_polls})
        b.free()
    if sink:
        sink.close()


def logprobs(pkg, m, args):
    import numpy as np
    V = m.n_vocab
    sink = open(args.out, "a") if args.out else None
    steps = args.tokens
    tops = [int(x) for x in args.logprobs.split(",")]

    def emit(rec):
        rec.update({"steps": steps, "reps": args.reps, "temperature": 1.0, "top_p": 0.8, "config": args.config, "dtype": args.dtype})
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    ns = [int(x) for x in args.n.split(",")]
    b = pkg.RWKVBatch(m, max(ns))
    for n in ns:
        slots = list(range(n))
        first = [(7 * i + 1) % V for i in slots]

        def best(run):
            out = []
            for k in range(args.reps + 1):   # (run 0: warm-up -- buffers of the first call, tile-major weight images)
                for s in slots:
                    b.state_load(s, None)
                out.append(run())
            return min(out[1:])

        b.set_logprobs(enabled=False)
        plain_ms = best(lambda: b.decode_sample(slots, first, steps, 1.0, 0.8, slots)[1])
        for top_n in tops:
            b.set_logprobs(top_n)
            rep_ms = best(lambda: b.decode_sample(slots, first, steps, 1.0, 0.8, slots)[1])
            t0 = time.perf_counter()
            b.logprobs()
            store_ms = (time.perf_counter() - t0) * 1e3
            emit({"mode": "logprobs_report", "n": n, "top_n": top_n, "ms_per_step": round(rep_ms / steps, 4), "plain_ms_per_step": round(plain_ms / steps, 4),
                  "report_ms_per_step": round((rep_ms - plain_ms) / steps, 4), "report_over_plain": round(rep_ms / plain_ms, 4),
                  "store_ms_per_call": round(store_ms, 3), "report_bytes_per_step": 4 * n * (1 + 2 * top_n)})
        b.set_logprobs(enabled=False)
        top = max(tops)

        def host():
            toks = list(first)
            t0 = time.perf_counter()
            for _ in range(steps):
                lg = b.eval(slots, toks).astype(np.float64)
                mx = lg.max(axis=1, keepdims=True)
                lp = lg - (mx + np.log(np.exp(lg - mx).sum(axis=1, keepdims=True)))
                if top:
                    part = np.argpartition(-lp, top - 1, axis=1)[:, :top]
                    np.take_along_axis(lp, part, axis=1)
                toks = lp.argmax(axis=1).tolist()
            return (time.perf_counter() - t0) * 1e3

        host_ms = best(host)
        emit({"mode": "logprobs_host", "n": n, "top_n": top, "ms_per_step": round(host_ms / steps, 4), "plain_ms_per_step": round(plain_ms / steps, 4),
              "host_over_plain": round(host_ms / plain_ms, 2), "logits_bytes_per_step": 4 * n * V})
    b.free()
    if sink:
        sink.close()


def beam(pkg, m, args):
    import numpy as np
    V = m.n_vocab
    sink = open(args.out, "a") if args.out else None
    steps = args.tokens
    widths = [int(x) for x in args.beam.split(",")]
    rows_wanted = max(int(x) for x in args.n.split(","))

    def emit(rec):
        rec.update({"steps": steps, "reps": args.reps, "config": args.config, "dtype": args.dtype})
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    b = pkg.RWKVBatch(m, rows_wanted)
    for W in widths:
        G = max(1, rows_wanted // W)
        n = G * W
        slots = list(range(n))
        first = [(7 * g + 1) % V for g in range(G)]

        def best(run):
            out = []
            for k in range(args.reps + 1):   # (run 0: warm-up -- buffers of the first call, tile-major weight images)
                for s in slots:
                    b.state_load(s, None)
                out.append(run())
            return min(out[1:])

        greedy_ms = best(lambda: b.decode_greedy(slots, [first[r // W] for r in range(n)], steps)[1])
        beam_ms = best(lambda: b.decode_beam(slots, first, W, steps)[4])
        emit({"mode": "beam", "width": W, "groups": G, "rows": n, "ms_per_step": round(beam_ms / steps, 4), "greedy_ms_per_step": round(greedy_ms / steps, 4),
              "beam_step_minus_greedy_ms": round((beam_ms - greedy_ms) / steps, 4), "beam_over_greedy": round(beam_ms / greedy_ms, 4), "passes": b.last_loop_passes()})

        def host():
            # the search driven from the host with calls that existed before: the logits to the host, a float64 log-softmax and the W best
            # of each row there, the selection, the states permuted with state_store / state_load
            score = np.where(np.arange(n) % W == 0, 0.0, -np.inf)
            fed = [first[r // W] for r in range(n)]
            for s in slots:
                if s % W:
                    b.state_load(s, b.state_store(s - s % W))
            t0 = time.perf_counter()
            for _ in range(steps):
                lg = b.eval(slots, fed).astype(np.float64)
                mx = lg.max(axis=1, keepdims=True)
                lp = lg - (mx + np.log(np.exp(lg - mx).sum(axis=1, keepdims=True)))
                top = np.argpartition(-lp, W - 1, axis=1)[:, :W] if W < V else np.tile(np.arange(V), (n, 1))
                top = np.take_along_axis(top, np.argsort(-np.take_along_axis(lp, top, axis=1), axis=1, kind="stable"), axis=1)
                cand = score[:, None] + np.take_along_axis(lp, top, axis=1)
                states = None
                for g in range(G):
                    flat = cand[g * W:(g + 1) * W].reshape(-1)
                    pick = np.argsort(-flat, kind="stable")[:W]
                    parents = pick // W
                    if np.any(parents != np.arange(W)):
                        if states is None:
                            states = {}
                        for j in range(W):
                            p = g * W + int(parents[j])
                            if p != g * W + j and p not in states:
                                states[p] = b.state_store(p)
                        for j in range(W):
                            p = g * W + int(parents[j])
                            if p != g * W + j:
                                b.state_load(g * W + j, states[p])
                    score[g * W:(g + 1) * W] = flat[pick]
                    for j in range(W):
                        fed[g * W + j] = int(top[g * W + int(parents[j]), int(pick[j]) % W])
            return (time.perf_counter() - t0) * 1e3

        host_ms = best(host)
        emit({"mode": "beam_host", "width": W, "groups": G, "rows": n, "ms_per_step": round(host_ms / steps, 4), "beam_ms_per_step": round(beam_ms / steps, 4),
              "host_over_device": round(host_ms / beam_ms, 2), "logits_bytes_per_step": 4 * n * V, "state_bytes": 4 * m.state_len})
    b.free()
    if sink:
        sink.close()


def host_sample_cut(logits, temperature, top_p, top_k, min_p, rng):
    """host_sample with the two truncations in the device's order: mask -> softmax -> top-p and min-p, intersected -> temperature."""
    import numpy as np
    x = logits.copy()
    if 0 < top_k < x.size:
        x[np.argpartition(x, x.size - top_k)[:x.size - top_k]] = -np.inf
    x -= x.max()
    probs = np.exp(x)
    probs /= probs.sum()
    cutoff = 0.0
    if 0.0 < top_p < 1.0:
        sorted_probs = np.sort(probs)[::-1]
        cutoff = float(sorted_probs[np.argmax(np.cumsum(sorted_probs) > top_p)])
    if min_p:
        cutoff = max(cutoff, min_p * float(probs.max()))
    probs[probs < cutoff] = 0
    if temperature != 1.0:
        probs = np.power(probs, 1.0 / temperature)
    probs = probs / probs.sum()
    return int(rng.choice(a=len(probs), p=probs))


def cut(pkg, m, args):
    import numpy as np
    V = m.n_vocab
    L = m._library.library
    sink = open(args.out, "a") if args.out else None
    steps = args.tokens
    have_cut = hasattr(L, "rwkv_mi_batch_truncation_set")   # (an older build loaded through RWKV_LIB_DIR: the plain loop only)
    ks = [int(x) for x in args.cut.split(",")]
    settings = [(k, 0.0) for k in ks] + [(0, 0.05), (ks[0], 0.05)]

    def emit(rec):
        rec.update({"steps": steps, "reps": args.reps, "temperature": 1.0, "top_p": 0.8, "config": args.config, "dtype": args.dtype,
                    "truncation_in_library": have_cut})
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    ns = [int(x) for x in args.n.split(",")]
    b = pkg.RWKVBatch(m, max(ns))
    for n in ns:
        slots = list(range(n))
        first = [(7 * i + 1) % V for i in slots]

        def runs(run, setting):
            out = []
            for k in range(args.reps + 1):   # (run 0: warm-up -- buffers of the first call, tile-major weight images)
                for s in slots:
                    b.state_load(s, None)
                    if have_cut:
                        b.set_truncation(s, *setting)
                out.append(run())
            return out[1:]

        greedy_ms = min(runs(lambda: b.decode_greedy(slots, first, steps)[1], (0, 0.0)))
        plain = runs(lambda: b.decode_sample(slots, first, steps, 1.0, 0.8, slots)[1], (0, 0.0))
        plain_ms = min(plain)
        emit({"mode": "cut_plain", "n": n, "ms_per_step": round(plain_ms / steps, 4), "ms_per_step_max": round(max(plain) / steps, 4),
              "spread": round(max(plain) / plain_ms - 1.0, 4), "greedy_ms_per_step": round(greedy_ms / steps, 4),
              "sampler_ms_per_step": round((plain_ms - greedy_ms) / steps, 4)})
        if not have_cut:
            continue
        for top_k, min_p in settings:
            dev_ms = min(runs(lambda: b.decode_sample(slots, first, steps, 1.0, 0.8, slots)[1], (top_k, min_p)))
            emit({"mode": "cut_device", "n": n, "top_k": top_k, "min_p": min_p, "ms_per_step": round(dev_ms / steps, 4),
                  "plain_ms_per_step": round(plain_ms / steps, 4), "sampler_ms_per_step": round((dev_ms - greedy_ms) / steps, 4),
                  "cut_ms_per_step": round((dev_ms - plain_ms) / steps, 4), "cut_over_plain": round(dev_ms / plain_ms, 4)})
        top_k, min_p = settings[-1]
        rngs = [np.random.default_rng(i) for i in range(n)]

        def host():
            toks = list(first)
            t0 = time.perf_counter()
            for _ in range(steps):
                lg = b.eval(slots, toks)
                toks = [host_sample_cut(lg[i], 1.0, 0.8, top_k, min_p, rngs[i]) for i in range(n)]
            return (time.perf_counter() - t0) * 1e3

        host_ms = min(runs(host, (0, 0.0)))
        emit({"mode": "cut_host", "n": n, "top_k": top_k, "min_p": min_p, "ms_per_step": round(host_ms / steps, 4), "logits_bytes_per_step": 4 * n * V})
    b.free()
    if sink:
        sink.close()


def guide(pkg, m, args):
    import ctypes

    import numpy as np
    V = m.n_vocab
    L = m._library.library
    sink = open(args.out, "a") if args.out else None
    steps = args.tokens
    have_guides = hasattr(L, "rwkv_mi_batch_guide_create")   # (an older build loaded through RWKV_LIB_DIR: the plain loop only)
    n_states = 4

    def emit(rec):
        rec.update({"steps": steps, "reps": args.reps, "temperature": 1.0, "top_p": 0.8, "config": args.config, "dtype": args.dtype})
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    # a guide of a few states, each allowing a random half of the vocabulary; for the host-driven loop, per state, the ids it forbids with
    # their -inf values as rwkv_mi_batch_logit_bias_set takes them, and the dense transition table to step on the host
    rng = np.random.default_rng(7)
    allowed = [np.flatnonzero(rng.random(V) < 0.5) for _ in range(n_states)]
    nxt = np.full((n_states, V), 0xFFFF, dtype=np.uint16)
    for s, a in enumerate(allowed):
        nxt[s, a] = rng.integers(0, n_states, size=a.size)
    off_ids = [np.ascontiguousarray(np.flatnonzero(nxt[s] == 0xFFFF).astype(np.uint32)) for s in range(n_states)]
    off_vals = [np.full(ids.size, -np.inf, dtype=np.float32) for ids in off_ids]
    P_U32, P_F32 = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_float)

    ns = [int(x) for x in args.n.split(",")]
    b = pkg.RWKVBatch(m, max(ns))
    gid = b.create_guide([{int(t): int(nxt[s, t]) for t in a} for s, a in enumerate(allowed)]) if have_guides else None
    for n in ns:
        slots = list(range(n))
        first = [(7 * i + 1) % V for i in slots]

        def runs(run, guided):
            out = []
            for k in range(args.reps + 1):   # (run 0: warm-up -- buffers of the first call, tile-major weight images)
                for s in slots:
                    b.state_load(s, None)
                    if have_guides:
                        b.attach_guide(s, gid if guided else pkg.NO_GUIDE, s % n_states if guided else 0)
                out.append(run())
            return out[1:]

        plain = runs(lambda: b.decode_sample(slots, first, steps, 1.0, 0.8, slots)[1], False)
        plain_ms = min(plain)
        emit({"mode": "guide_plain", "n": n, "ms_per_step": round(plain_ms / steps, 4), "ms_per_step_max": round(max(plain) / steps, 4),
              "spread": round(max(plain) / plain_ms - 1.0, 4), "guides_in_library": have_guides})
        if not have_guides:
            continue
        dev_ms = min(runs(lambda: b.decode_sample(slots, first, steps, 1.0, 0.8, slots)[1], True))
        assert all(b.guide_state(s)[2] == 0 for s in slots), "a guided row missed"
        emit({"mode": "guide_device", "n": n, "ms_per_step": round(dev_ms / steps, 4), "plain_ms_per_step": round(plain_ms / steps, 4),
              "guide_ms_per_step": round((dev_ms - plain_ms) / steps, 4), "guided_over_plain": round(dev_ms / plain_ms, 4), "states": n_states,
              "table_bytes": int(nxt.nbytes)})

        def host():
            # the way without guides: before every token each row's mask goes up as a bias of -inf, one synchronising pass samples, the token
            # comes back and the automaton steps on the host
            state = [s % n_states for s in slots]
            toks = list(first)
            for s in slots:
                b.rng_seek(s, 0)
            t0 = time.perf_counter()
            for _ in range(steps):
                for i, s in enumerate(slots):
                    ids, vals = off_ids[state[i]], off_vals[state[i]]
                    if not L.rwkv_mi_batch_logit_bias_set(b._ptr, s, ids.ctypes.data_as(P_U32), vals.ctypes.data_as(P_F32), ids.size):
                        raise RuntimeError("rwkv_mi_batch_logit_bias_set failed")
                toks = [int(t) for t in b.eval_sample_penalized(slots, toks, 1.0, 0.8, -1.0, slots, 0.0, 0.0, False)]
                state = [int(nxt[state[i], toks[i]]) for i in range(n)]
            ms = (time.perf_counter() - t0) * 1e3
            for s in slots:
                b.set_logit_bias(s, {})
            return ms

        host_ms = min(runs(host, False))
        emit({"mode": "guide_host", "n": n, "ms_per_step": round(host_ms / steps, 4), "device_ms_per_step": round(dev_ms / steps, 4),
              "host_over_device": round(host_ms / dev_ms, 2), "bias_entries_per_row_and_step": int(np.mean([ids.size for ids in off_ids]))})
    b.free()
    if sink:
        sink.close()


def decay(pkg, m, args):
    import numpy as np
    V = m.n_vocab
    have = hasattr(m._library.library, "rwkv_mi_batch_repetition_set")   # (an older build loaded through RWKV_LIB_DIR: the plain arm only)
    sink = open(args.out, "a") if args.out else None
    ns = [int(x) for x in args.n.split(",")]
    decays = [float(x) for x in args.decay.split(",")]
    steps, presence, frequency = args.tokens, 0.2, 0.2

    def emit(rec):
        rec.update({"steps": steps, "reps": args.reps, "presence": presence, "frequency": frequency, "temperature": 1.0, "top_p": 0.8,
                    "config": args.config, "dtype": args.dtype, "settings_in_library": have})
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    b = pkg.RWKVBatch(m, max(ns))
    for n in ns:
        slots = list(range(n))
        first = [(7 * i + 1) % V for i in slots]

        def device(setting):
            out = []
            for r in range(args.reps + 1):   # (run 0: warm-up -- tables, rows and tile-major weight images of the first call)
                for s in slots:
                    b.state_load(s, None)
                    if have:
                        b.set_repetition(s, *setting)
                    b.counts_reset(s)
                    b.rng_seek(s, 0)
                out.append(b.decode_sample_penalized(slots, first, args.warmup if r == 0 else steps, 1.0, 0.8, slots, presence, frequency)[1])
            return out[1:]

        plain = device((1.0, 1.0))
        plain_ms = min(plain)
        emit({"mode": "decay_plain", "n": n, "ms_per_step": round(plain_ms / steps, 4), "ms_per_step_max": round(max(plain) / steps, 4),
              "spread": round(max(plain) / plain_ms - 1.0, 4)})
        if not have:
            continue
        for setting in [(d, 1.0) for d in decays] + [(1.0, args.repetition), (decays[0], args.repetition)]:
            ms = min(device(setting))
            emit({"mode": "decay_device", "n": n, "decay": setting[0], "repetition": setting[1], "ms_per_step": round(ms / steps, 4),
                  "plain_ms_per_step": round(plain_ms / steps, 4), "setting_ms_per_step": round((ms - plain_ms) / steps, 4),
                  "table_store_bytes_per_step": 4 * V * n if setting[0] != 1.0 else 0})
        for s in slots:
            b.set_repetition(s, 1.0, 1.0)
        # the way without the settings: per token the logits to the host, the demos' recipe on a float table in NumPy, sample_probs
        d32, r32, p32, f32 = np.float32(decays[0]), np.float32(args.repetition), np.float32(presence), np.float32(frequency)
        rngs = [np.random.default_rng(i) for i in range(n)]
        for s in slots:
            b.state_load(s, None)
        toks = list(first)
        for timed in (False, True):
            occ = np.zeros((n, V), dtype=np.float32)
            t0 = time.perf_counter()
            for _ in range(steps if timed else args.warmup):
                lg = b.eval(slots, toks)
                for i in range(n):
                    row, o = lg[i], occ[i]
                    at = np.flatnonzero(o > 0)
                    v = row[at]
                    v = np.where(v > 0, v / r32, v * r32)
                    row[at] = v - (p32 + o[at] * f32)
                    toks[i] = host_sample(row, 1.0, 0.8, rngs[i])
                    o *= d32
                    o[toks[i]] += np.float32(1.0)
            host_ms = (time.perf_counter() - t0) * 1e3 / steps
        dev_ms = min(device((decays[0], args.repetition))) / steps
        emit({"mode": "decay_host", "n": n, "decay": decays[0], "repetition": args.repetition, "ms_per_step": round(host_ms, 4),
              "device_ms_per_step": round(dev_ms, 4), "host_over_device": round(host_ms / dev_ms, 2), "logits_bytes_per_step": 4 * n * V})
        for s in slots:
            b.set_repetition(s, 1.0, 1.0)
    b.free()
    if sink:
        sink.close()


def draft(pkg, m, args):
    import numpy as np
    V = m.n_vocab
    L = m._library.library
    have_draft = hasattr(L, "rwkv_mi_batch_eval_draft")   # (an older build loaded through RWKV_LIB_DIR: the ragged pass and the plain loops only)
    sink = open(args.out, "a") if args.out else None
    ks = [int(x) for x in args.draft.split(",")]
    ns = [int(x) for x in args.n.split(",")]
    passes = args.tokens
    accepts = (0, 1, 2, 4, 8)

    def emit(rec):
        rec.update({"reps": args.reps, "temperature": 1.0, "top_p": 0.8, "config": args.config, "dtype": args.dtype, "draft_in_library": have_draft})
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def corrupt(true_row, k, a):
        d = [int(t) for t in true_row[:k]]
        if a < k:
            d[a] = (d[a] + 1) % V
        return d

    b = pkg.RWKVBatch(m, max(ns))
    for n in ns:
        slots = list(range(n))
        first = [(7 * i + 1) % V for i in slots]

        def fresh():
            for s in slots:
                b.state_load(s, None)
                b.rng_seek(s, 0)

        def best(run):
            out = []
            for _ in range(args.reps + 1):   # (run 0: warm-up -- buffers of the first call, tile-major weight images)
                fresh()
                out.append(run())
            return min(out[1:])

        def clocked(call):
            def run():
                t0 = time.perf_counter()
                call()
                return (time.perf_counter() - t0) * 1e3
            return run

        need = passes * (max(accepts) + 1) + max(ks) + 1
        plain = {"greedy": best(lambda: b.decode_greedy(slots, first, 32)[1]) / 32,
                 "sampled": best(lambda: b.decode_sample(slots, first, 32, 1.0, 0.8, slots)[1]) / 32}
        emit({"mode": "draft_plain", "n": n, "greedy_ms_per_step": round(plain["greedy"], 4), "sampled_ms_per_step": round(plain["sampled"], 4), "steps": 32})
        for family in ("greedy", "sampled"):
            fresh()
            true = (b.decode_greedy(slots, first, need) if family == "greedy" else b.decode_sample(slots, first, need, 1.0, 0.8, slots))[0]
            params = None if family == "greedy" else pkg.sample_params(n, 1.0, 0.8, -1.0, slots)
            temperature = 0.0 if family == "greedy" else 1.0
            for k in ks:
                # 1. the call's overhead: one call of n rows of 1 + k tokens against the ragged pass of the same shape that samples each row's last
                # token -- what is added is the stash, the head on every token, the sequential choice and (where a draft falls) the replay
                rows_all = [[first[i]] + corrupt(true[i], k, k) for i in slots]
                rows_none = [[first[i]] + corrupt(true[i], k, 0) for i in slots]
                ragged_ms = best(clocked(lambda: b.eval_ragged_sample(slots, rows_all, temperature, 0.8, -1.0, slots)))
                rec = {"mode": "draft_overhead", "family": family, "n": n, "k": k, "T": n * (k + 1), "ragged_sample_ms": round(ragged_ms, 4)}
                if have_draft:
                    all_ms = best(clocked(lambda: b.eval_draft(slots, rows_all, params=params)))
                    none_ms = best(clocked(lambda: b.eval_draft(slots, rows_none, params=params)))
                    rec.update({"draft_all_accepted_ms": round(all_ms, 4), "draft_none_accepted_ms": round(none_ms, 4),
                                "overhead_all_accepted_ms": round(all_ms - ragged_ms, 4), "overhead_none_accepted_ms": round(none_ms - ragged_ms, 4)})
                emit(rec)
                if not have_draft:
                    continue
                # 2. tokens/s as a function of acceptance: `passes` successive calls whose drafts are cut from the true continuation and corrupted
                # so that exactly a tokens per row stand, the rows built ahead of the clock; each call emits a + 1 tokens per row
                for a in [x for x in accepts if x <= k]:
                    calls, pos, x0 = [], 0, list(first)
                    for _ in range(passes):
                        calls.append([[x0[i]] + corrupt(true[i][pos:], k, a) for i in slots])
                        pos += a + 1
                        x0 = [int(true[i][pos - 1]) for i in slots]

                    def run():
                        t0 = time.perf_counter()
                        for rows in calls:
                            _, lens = b.eval_draft(slots, rows, params=params)
                            assert (lens == a + 1).all(), (a, lens)
                        return (time.perf_counter() - t0) * 1e3
                    call_ms = best(run) / passes
                    plain_ms = plain[family]
                    emit({"mode": "draft_accept", "family": family, "n": n, "k": k, "a": a, "passes": passes, "ms_per_call": round(call_ms, 4),
                          "tokens_per_s": round(n * (a + 1) / (call_ms / 1e3), 1), "plain_ms_per_step": round(plain_ms, 4),
                          "plain_tokens_per_s": round(n / (plain_ms / 1e3), 1), "speedup": round((a + 1) * plain_ms / call_ms, 3),
                          "break_even_a": round(call_ms / plain_ms - 1.0, 3)})
    b.free()
    if sink:
        sink.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("model_path")
    ap.add_argument("--config", default="rwkv6-7b")
    ap.add_argument("--dtype", default="Q4_0")
    ap.add_argument("--n", default="1,2,4,8,16,32,64,128")
    ap.add_argument("--tokens", type=int, default=32, help="steps of each timed loop")
    ap.add_argument("--warmup", type=int, default=4, help="steps of the warm-up loop of every n")
    ap.add_argument("--sample", action="store_true", help="also time the sampling loop: on the device, and through the host")
    ap.add_argument("--penalties", action="store_true", help="with --sample: also time the penalised sampling loop, on the device and through the host")
    ap.add_argument("--ragged", action="store_true", help="time the ragged pass: prompt ingestion and joining a decode step (see above)")
    ap.add_argument("--until", action="store_true", help="time rwkv_mi_batch_decode_until against the plain sampled loop (see above)")
    ap.add_argument("--serve", action="store_true", help="time rwkv_mi_batch_serve on a fixed queue of 4 n requests against the same queue in waves of decode_until; with --guide and / or --logprobs N: rwkv_mi_batch_serve_ex with every request guided, the report on (see above)")
    ap.add_argument("--session", action="store_true", help="time the serve session on the queue of --serve: the whole queue up front against serve, and arrivals in groups of n against one closed serve call per group")
    ap.add_argument("--run", default=None, help="--session: an identifier of this process run, written into every record")
    ap.add_argument("--logprobs", default=None, metavar="N[,N...]",
                    help="with --sample: time the sampled loop with and without the report of the emitted tokens, for each top_n of the list (see above)")
    ap.add_argument("--beam", default=None, metavar="W[,W...]",
                    help="time rwkv_mi_batch_decode_beam for each width of the list at the largest row count of --n, against the greedy loop and the host-driven search")
    ap.add_argument("--guide", action="store_true",
                    help="with --sample: time the sampled loop plain, guided on the device, and masked from the host before every token (see above)")
    ap.add_argument("--cut", default=None, metavar="K[,K...]",
                    help="with --sample: time the sampled loop with no truncation setting, with top_k = each K, with min_p = 0.05, and with both (see above)")
    ap.add_argument("--decay", default=None, metavar="D[,D...]",
                    help="with --sample --penalties: time the penalised loop with no repetition setting, with decay = each D, with --repetition, and with both (see above)")
    ap.add_argument("--repetition", type=float, default=1.1, help="--decay: the repetition penalty of the arms that have one")
    ap.add_argument("--draft", default=None, metavar="K[,K...]",
                    help="time rwkv_mi_batch_eval_draft for each draft length of the list: its overhead over the ragged pass, tokens/s by acceptance (see above)")
    ap.add_argument("--reps", type=int, default=3, help="--draft, --ragged, --until, --logprobs, --beam, --guide, --cut, --decay: timed runs of each shape (the smallest is reported)")
    ap.add_argument("--out", default=None, help="--draft, --ragged, --penalties, --until, --logprobs, --beam, --guide, --cut, --decay: also append the records to this file")
    args = ap.parse_args()

    import __graft_entry__ as graft
    pkg = graft.load_package()
    from rwkv_cpp_amd import synth

    spec = synth.CONFIGS[args.config]
    marker = args.model_path + ".ok"
    if not (os.path.exists(args.model_path) and os.path.exists(marker)):
        t = time.time()
        info = synth.write_model(args.model_path, spec, args.dtype, seed=42)
        with open(marker, "w") as f:
            f.write(json.dumps(info))
        print(f"[batch_decode] wrote {args.model_path}: {info['bytes'] / 1e9:.2f} GB in {time.time() - t:.1f}s", file=sys.stderr)

    pkg.build_library()
    lib = pkg.load_rwkv_shared_library()
    m = pkg.RWKVModel(lib, args.model_path, thread_count=1, gpu_layer_count=99)
    if args.ragged:
        ragged(pkg, m, args)
        m.free()
        return
    if args.until:
        until(pkg, m, args)
        m.free()
        return
    if args.session:
        session(pkg, m, args)
        m.free()
        return
    if args.serve:
        serve(pkg, m, args)
        m.free()
        return
    if args.beam is not None:
        beam(pkg, m, args)
        m.free()
        return
    if args.draft is not None:
        draft(pkg, m, args)
        m.free()
        return
    if args.guide:
        if not args.sample:
            ap.error("--guide times the sampled loop: give --sample with it")
        guide(pkg, m, args)
        m.free()
        return
    if args.cut is not None:
        if not args.sample:
            ap.error("--cut times the sampled loop: give --sample with it")
        cut(pkg, m, args)
        m.free()
        return
    if args.decay is not None:
        if not (args.sample and args.penalties):
            ap.error("--decay times the penalised sampled loop: give --sample --penalties with it")
        decay(pkg, m, args)
        m.free()
        return
    if args.logprobs is not None:
        if not args.sample:
            ap.error("--logprobs times the sampled loop: give --sample with it")
        logprobs(pkg, m, args)
        m.free()
        return
    ns = [int(x) for x in args.n.split(",")]
    V, D, state_len = m.n_vocab, m.n_embed, m.state_len
    weight_bytes = int(lib.library.rwkv_mi_weight_bytes(m._ctx.ptr))
    emb_row = 2 * D                                   # F16 embedding row
    per_seq = 2 * 4 * state_len + emb_row + 4 * V     # state read + write, embedding row, logits
    weights_once = weight_bytes - V * emb_row         # every matrix once; of the embedding only the rows the tokens select

    # single stream, same process
    m.state_load(None)
    m.decode_greedy(1, args.warmup)
    _, ms1 = m.decode_greedy(2, args.tokens)
    single = args.tokens / (ms1 / 1e3)
    print(json.dumps({"mode": "single_stream", "decode_path": m.decode_path(), "ms_per_token": round(ms1 / args.tokens, 4),
                      "tokens_per_s": round(single, 1)}), flush=True)

    b = pkg.RWKVBatch(m, max(ns))
    for n in ns:   # warm-up of every n first (tile-major weight images, scratch growth)
        b.decode_greedy(list(range(n)), [(7 * i + 1) % V for i in range(n)], args.warmup)
    for n in ns:
        slots = list(range(n))
        for s in slots:
            b.state_load(s, None)
        _, ms = b.decode_greedy(slots, [(7 * i + 1) % V for i in range(n)], args.tokens)
        step_ms = ms / args.tokens
        alg = weights_once + n * per_seq
        rec = {"mode": "batch", "n": n, "ms_per_step": round(step_ms, 4), "tokens_per_s": round(n / (step_ms / 1e3), 1),
               "per_seq_tokens_per_s": round(1e3 / step_ms, 1), "vs_single_stream": round(n / (step_ms / 1e3) / single, 3),
               "alg_bytes_per_step": alg, "step_fraction_of_8TBs": round(alg / (step_ms / 1e3) / HBM_PEAK_BS, 4),
               "steps": args.tokens, "config": args.config, "dtype": args.dtype}
        print(json.dumps(rec), flush=True)
        if not args.sample:
            continue
        import numpy as np
        first = [(7 * i + 1) % V for i in range(n)]
        for s in slots:
            b.state_load(s, None)
        b.decode_sample(slots, first, args.warmup, 1.0, 0.8, slots)   # (the first sampling call allocates the sampler's scratch)
        for s in slots:
            b.state_load(s, None)
        _, ms_s = b.decode_sample(slots, first, args.tokens, 1.0, 0.8, slots)
        dev_ms = ms_s / args.tokens
        print(json.dumps({"mode": "batch_sample", "n": n, "ms_per_step": round(dev_ms, 4), "greedy_ms_per_step": round(step_ms, 4),
                          "sampler_ms_per_step": round(dev_ms - step_ms, 4), "tokens_per_s": round(n / (dev_ms / 1e3), 1),
                          "temperature": 1.0, "top_p": 0.8, "steps": args.tokens, "config": args.config, "dtype": args.dtype}), flush=True)
        rngs = [np.random.default_rng(i) for i in range(n)]
        for s in slots:
            b.state_load(s, None)
        toks = list(first)
        for timed in (False, True):
            t0 = time.perf_counter()
            for _ in range(args.tokens if timed else args.warmup):
                lg = b.eval(slots, toks)
                toks = [host_sample(lg[i], 1.0, 0.8, rngs[i]) for i in range(n)]
            host_ms = (time.perf_counter() - t0) * 1e3 / args.tokens
        print(json.dumps({"mode": "batch_host_sample", "n": n, "ms_per_step": round(host_ms, 4), "device_sample_ms_per_step": round(dev_ms, 4),
                          "host_over_device": round(host_ms / dev_ms, 2), "logits_bytes_per_step": 4 * n * V,
                          "temperature": 1.0, "top_p": 0.8, "steps": args.tokens, "config": args.config, "dtype": args.dtype}), flush=True)
        if not args.penalties:
            continue
        presence, frequency = 0.2, 0.2   # (chat_with_bot.py:31-33)

        def new_request():
            for s in slots:
                b.state_load(s, None)
                b.counts_reset(s)
                b.rng_seek(s, 0)

        new_request()
        b.decode_sample_penalized(slots, first, args.warmup, 1.0, 0.8, slots, presence, frequency)   # (the first call allocates the tables)
        new_request()
        _, ms_p = b.decode_sample_penalized(slots, first, args.tokens, 1.0, 0.8, slots, presence, frequency)
        pen_ms = ms_p / args.tokens
        recs = [{"mode": "batch_sample_penalized", "n": n, "ms_per_step": round(pen_ms, 4), "sampled_ms_per_step": round(dev_ms, 4),
                 "penalty_ms_per_step": round(pen_ms - dev_ms, 4), "greedy_ms_per_step": round(step_ms, 4), "tokens_per_s": round(n / (pen_ms / 1e3), 1)}]
        rngs = [np.random.default_rng(i) for i in range(n)]
        for s in slots:
            b.state_load(s, None)
        toks = list(first)
        for timed in (False, True):
            token_counts = [{} for _ in range(n)]
            t0 = time.perf_counter()
            for _ in range(args.tokens if timed else args.warmup):
                lg = b.eval(slots, toks)
                for i in range(n):
                    row, tc = lg[i], token_counts[i]
                    for k in tc:
                        row[k] -= presence + tc[k] * frequency
                    toks[i] = host_sample(row, 1.0, 0.8, rngs[i])
                    tc[toks[i]] = tc.get(toks[i], 0) + 1
            host_p_ms = (time.perf_counter() - t0) * 1e3 / args.tokens
        recs.append({"mode": "batch_host_sample_penalized", "n": n, "ms_per_step": round(host_p_ms, 4), "device_ms_per_step": round(pen_ms, 4),
                     "host_over_device": round(host_p_ms / pen_ms, 2), "logits_bytes_per_step": 4 * n * V})
        for rec in recs:
            rec.update({"presence": presence, "frequency": frequency, "temperature": 1.0, "top_p": 0.8, "steps": args.tokens,
                        "config": args.config, "dtype": args.dtype})
            line = json.dumps(rec)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
    b.free()
    m.free()


if __name__ == "__main__":
    main()
