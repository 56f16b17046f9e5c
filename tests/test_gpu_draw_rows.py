"""One row table per call (csrc/model.h DrawRow, filled by DrawState::row): every row of a batch call carries ALL its slot's draw settings, so the
thing only this layout can get wrong is a field of one row reaching another. Six slots with different settings -- none, truncation, a guide,
repetition, everything at once, none again -- go through one penalised loop together, in either order, and through the plain loop; each slot
must end exactly where it ends when it is the only slot its call names. Exact equality throughout: no tolerance is involved."""
import os

import numpy as np
import pytest

from gpu_lib import model, pkg

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny-rwkv-6v0-3m-Q5_0.bin")
STEPS = 8
N = 6
FIRST = [17, 101, 5, 240, 66, 17]
SEEDS = [11, 22, 33, 44, 55, 66]
TEMPERATURE = [1.0, 0.8, 1.2, 1.0, 0.9, 1.1]
TOP_P = [0.9, 1.0, 0.8, 0.95, 1.0, 0.9]
PRESENCE = [0.2, 0.1, 0.3, 0.2, 0.4, 0.2]
FREQUENCY = [0.2, 0.3, 0.1, 0.2, 0.1, 0.2]
# a 3-state guide that allows six tokens per state
GUIDE = [{20 + 7 * s + 13 * j: (s + j) % 3 for j in range(6)} for s in range(3)]


def _settings(b, slot, guide):
    """slot i of the issue's list, 0-based: 0 none, 1 truncation, 2 guide, 3 repetition, 4 decay + repetition + truncation + guide, 5 none"""
    if slot in (1, 4):
        b.set_truncation(slot, 5, 0.05)
    if slot in (2, 4):
        b.attach_guide(slot, guide, 0)
    if slot == 3:
        b.set_repetition(slot, 1.0, 1.3)
    if slot == 4:
        b.set_repetition(slot, 0.9, 1.3)


def _run(m, slots, penalised):
    """A fresh batch with the settings of `slots` only, one loop of STEPS steps over them in that order: per slot what it ends with"""
    b = pkg.RWKVBatch(m, N)
    guide = b.create_guide(GUIDE)
    for s in slots:
        _settings(b, s, guide)
    pick = lambda v: [v[s] for s in slots]
    if penalised:
        toks, _ = b.decode_sample_penalized(slots, pick(FIRST), STEPS, pick(TEMPERATURE), pick(TOP_P), pick(SEEDS), pick(PRESENCE), pick(FREQUENCY))
    else:
        toks, _ = b.decode_sample(slots, pick(FIRST), STEPS, pick(TEMPERATURE), pick(TOP_P), pick(SEEDS))
    end = {}
    for i, s in enumerate(slots):
        words = b.guide_state(s)[1:]
        occ = b.counts_f32(s)
        # the draw counter has no getter: one more generator draw of the slot alone, from a state and with settings checked equal, shows it
        after = b.eval_sample([s], [int(toks[i][-1])], 1.0, 1.0, -1.0, SEEDS[s])
        end[s] = {"tokens": toks[i].tolist(), "occurrences": occ.view(np.uint32).tolist(), "guide words": words, "state": b.state_store(s).view(np.uint32).tolist(),
                  "next draw": after.tolist()}
    b.free()
    return end


@pytest.fixture(scope="module")
def alone():
    """each slot as the only one named: {(slot, penalised): its end}, computed once"""
    m = model(GOLDEN)
    return m, {(s, pen): _run(m, [s], pen)[s] for pen in (True, False) for s in (range(N) if pen else (0, 1, 2, 5))}


@pytest.mark.parametrize("order, penalised", [(list(range(N)), True), (list(range(N))[::-1], True), ([0, 1, 2, 5], False)],
                         ids=["penalised", "penalised-reversed", "plain"])
def test_every_slot_ends_as_it_does_alone(alone, order, penalised):
    m, ref = alone
    got = _run(m, order, penalised)
    for s in order:
        for what, want in ref[(s, penalised)].items():
            assert got[s][what] == want, (s, what)
    # (the settings did something: the guided slots drew from their guide, and the slots differ)
    for s in (2, 4) if penalised else (2,):
        assert all(t in set().union(*GUIDE) for t in got[s]["tokens"]), (s, got[s]["tokens"])
    assert got[0]["tokens"] != got[5]["tokens"]
