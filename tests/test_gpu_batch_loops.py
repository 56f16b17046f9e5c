"""The four device loops of a batch on ONE batch, in any order of first use (rwkv_mi_batch_decode_until, rwkv_mi_batch_serve,
rwkv_mi_batch_decode_beam, rwkv_mi_batch_decode_greedy). The three polled loops share the pinned live counts and the two block events of their
batch, whichever of them runs first creates them, and the greedy loop must never need them. The oracle is the call itself on a fresh batch
of its own that starts from the same slot states (state_load): tokens, lengths, reasons, the states of the named slots and the number of
passes enqueued must be equal. Every comparison is exact.

RWKV_MI_LOOP_BLOCK is 2 for every call: each polled loop then spans at least three blocks, so the wait on the block before the last one
enqueued is taken."""
import os

import numpy as np
import pytest

from gpu_lib import ROOT, library, model, pkg

pytestmark = pytest.mark.gpu

MODELS = [("tiny-rwkv-6v0-3m", "Q5_1"), ("tiny-rwkv-4v0-660K", "Q5_1")]
ORDERS = [("until", "serve", "beam", "greedy"), ("beam", "serve", "until", "greedy"), ("serve", "greedy", "beam", "until")]
N_SLOTS = 4
BLOCK = 2
# the slots each call names: every slot is named by two calls, so each call but the first starts from what another loop left
SLOTS = {"until": [2, 0], "serve": [1, 3], "beam": [3, 0], "greedy": [1, 2]}


def _tok(i, j, V):
    return (37 * i + 11 * j + 5) % V


def _requests(V):
    return [dict(prompt=[_tok(3, 0, V)], max_tokens=2), dict(prompt=[_tok(4, 0, V), _tok(4, 1, V)], max_tokens=3),
            dict(prompt=[_tok(5, 0, V), _tok(5, 1, V)], max_tokens=3)]


def _run(b, call, V):
    """One of the four calls on its slots: everything it returns but the elapsed time, as a list of arrays."""
    slots = SLOTS[call]
    if call == "until":
        toks, why, _ = b.decode_until(slots, [_tok(1, 0, V), _tok(1, 1, V)], [5, 3])
        assert [len(t) for t in toks] == [5, 3]
        return list(toks) + [why]
    if call == "serve":
        got = b.serve(slots, _requests(V))
        assert [len(t) for t in got["tokens"]] == [2, 3, 3]
        return list(got["tokens"]) + [got[k] for k in ("stopped_by", "lane", "start_pass", "last_request")]
    if call == "beam":
        tokens, lens, scores, lps, _ = b.decode_beam([slots], [_tok(2, 0, V)], 2, 5)
        return [tokens, lens, scores, lps]
    return [b.decode_greedy(slots, [_tok(6, 0, V), _tok(6, 1, V)], 5)[0]]


def _same(a, c):
    return len(a) == len(c) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, c))


@pytest.mark.parametrize("order", ORDERS, ids=["-".join(o) for o in ORDERS])
@pytest.mark.parametrize("name,fmt", MODELS)
def test_each_loop_on_a_shared_batch_is_the_loop_on_a_batch_of_its_own(name, fmt, order):
    library()
    m = model(os.path.join(ROOT, "tests", "golden", f"{name}-{fmt}.bin"))
    V = m.n_vocab
    every = list(range(N_SLOTS))
    saved = os.environ.get("RWKV_MI_LOOP_BLOCK")
    batches = []   # freed on every exit, the twins and the shared batch before the model

    def batch():
        batches.append(pkg.RWKVBatch(m, N_SLOTS))
        return batches[-1]

    try:
        os.environ["RWKV_MI_LOOP_BLOCK"] = str(BLOCK)   # (read at the call)
        b = batch()
        # distinct states, mixed parities
        b.eval(every, [_tok(0, s, V) for s in every], want_logits=False)
        b.eval([1, 2], [_tok(7, s, V) for s in (1, 2)], want_logits=False)
        for call in order:
            tw = batch()
            for s in every:
                tw.state_load(s, b.state_store(s))
            got, want = _run(b, call, V), _run(tw, call, V)
            assert _same(got, want), (name, order, call, got, want)
            assert b.last_loop_passes() == tw.last_loop_passes(), (name, order, call, b.last_loop_passes(), tw.last_loop_passes())
            if call != "greedy":
                assert b.last_loop_passes() > 2 * BLOCK, (name, order, call, "the loop must span three blocks")
            for s in SLOTS[call]:
                assert np.array_equal(b.state_store(s), tw.state_store(s)), (name, order, call, s)
            tw.free()
    finally:
        if saved is None:
            os.environ.pop("RWKV_MI_LOOP_BLOCK", None)
        else:
            os.environ["RWKV_MI_LOOP_BLOCK"] = saved
        for x in batches:
            x.free()   # (a second free of a twin does nothing)
        m.free()
