"""The beam search's selection rule (tests/beam_ref.py, the reference tests/test_gpu_beam.py holds the device to) on a hand-written table, the
answers worked out below, and -- without a GPU -- that the header declares the two calls, the libraries export them and the binding wires them.

The "model" has five tokens and its log-probs depend on the last token only; every number is a multiple of 1/4, so every sum is exact and the
ties are exact ties. Token 4 ends a hypothesis. The ranked lists (id, log-prob) after each token:
    after 0:  (1, -1)     (2, -1)     (3, -2)
    after 1:  (4, -0.5)   (3, -1.5)   (0, -3)
    after 2:  (3, -0.5)   (0, -1)     (4, -4)
    after 3:  (4, -0.25)  (1, -2)     (2, -2)
    after 4:  never asked for: a hypothesis that ends in 4 has finished
A beam of W uses the first W entries of a list. The first token is 0."""
import ctypes
import os
import re

import numpy as np

import beam_ref
from beam_ref import NO_TOKEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rwkv_mi_batch_state_copy", "rwkv_mi_batch_decode_beam")
HOOK = "rwkv_test_beam_step"
END = 4
TABLE = {0: [(1, -1.0), (2, -1.0), (3, -2.0)],
         1: [(4, -0.5), (3, -1.5), (0, -3.0)],
         2: [(3, -0.5), (0, -1.0), (4, -4.0)],
         3: [(4, -0.25), (1, -2.0), (2, -2.0)]}
X = NO_TOKEN


def _model(table, W, asked=None):
    def candidates(fed, parents, live):
        ids = np.full((W, W), NO_TOKEN, dtype=np.uint32)
        lps = np.full((W, W), -np.inf, dtype=np.float32)
        for j in range(W):
            if not live[j]:
                continue          # (a finished or dead row is never asked: its lists stay unusable)
            if asked is not None:
                asked.append(int(fed[j]))
            for k, (t, l) in enumerate(table[int(fed[j])][:W]):
                ids[j, k], lps[j, k] = t, l
        return ids, lps
    return candidates


def test_width_two_ties_by_rank_then_by_parent_then_a_finished_hypothesis_survives_and_the_group_ends_early():
    # step 0: only hypothesis 0 has a finite score. It offers (1, -1) at rank 0 and (2, -1) at rank 1: equal scores, one parent -- the RANK
    #         decides.                                                         -> h0 = [1] -1, h1 = [2] -1
    # step 1: h0 (after 1) offers (4, -1.5), (3, -2.5); h1 (after 2) offers (3, -1.5), (0, -2). The two best tie at -1.5 with rank 0 each -- the
    #         PARENT decides: parent 0 first. Its token is 4, so it finishes.     -> h0 = [1 4] -1.5 finished, h1 = [2 3] -1.5
    # step 2: h0 offers itself at -1.5; h1 (after 3) offers (4, -1.75), (1, -3.5). The finished one survives by its score, in front.
    #                                                                            -> h0 = [1 4] -1.5, h1 = [2 3 4] -1.75, both finished
    # the group has ended after 3 of the 6 steps allowed.
    asked = []
    tokens, lens, scores, lps, steps, _, fin = beam_ref.search(_model(TABLE, 2, asked), 0, 2, 6, [END])
    assert steps == 3 and fin.tolist() == [1, 1]
    assert tokens.tolist() == [[1, 4, X, X, X, X], [2, 3, 4, X, X, X]]
    assert lens.tolist() == [2, 3] and scores.tolist() == [-1.5, -1.75]
    assert lps.tolist() == [[-1.0, -0.5, 0, 0, 0, 0], [-1.0, -0.5, -0.25, 0, 0, 0]]
    assert asked == [0, 1, 2, 3]          # step 0 asks row 0 only (row 1 starts at -inf); step 2 does not ask the finished row


def test_width_three_to_the_end_and_cut_short():
    # step 0: (1, -1), (2, -1), (3, -2)                                          -> h0 = [1] -1, h1 = [2] -1, h2 = [3] -2
    # step 1: h0: (4, -1.5) (3, -2.5) (0, -4);  h1: (3, -1.5) (0, -2) (4, -5);  h2: (4, -2.25) (1, -4) (2, -4)
    #         best three: -1.5 parent 0 (token 4: finished), -1.5 parent 1, -2 parent 1 rank 1
    #                                                                            -> h0 = [1 4] -1.5 F, h1 = [2 3] -1.5, h2 = [2 0] -2
    # step 2: h0 itself -1.5;  h1 (after 3): (4, -1.75) (1, -3.5) (2, -3.5);  h2 (after 0): (1, -3) (2, -3) (3, -4)
    #                                                                            -> h0 = [1 4] -1.5 F, h1 = [2 3 4] -1.75 F, h2 = [2 0 1] -3
    # step 3: h0 -1.5; h1 -1.75;  h2 (after 1): (4, -3.5) (3, -4.5) (0, -6)      -> h2 = [2 0 1 4] -3.5 F: all finished after 4 steps
    tokens, lens, scores, lps, steps, _, fin = beam_ref.search(_model(TABLE, 3), 0, 3, 6, [END])
    assert steps == 4 and fin.tolist() == [1, 1, 1]
    assert tokens.tolist() == [[1, 4, X, X, X, X], [2, 3, 4, X, X, X], [2, 0, 1, 4, X, X]]
    assert lens.tolist() == [2, 3, 4] and scores.tolist() == [-1.5, -1.75, -3.5]
    assert lps[2].tolist() == [-1.0, -1.0, -1.0, -0.5, 0, 0]          # (2 after 0, 0 after 2, 1 after 0, 4 after 1: they add up to -3.5)
    # cut at 3 steps: hypothesis 2 is still open, its last parent is itself
    tokens, lens, scores, _, steps, par, fin = beam_ref.search(_model(TABLE, 3), 0, 3, 3, [END])
    assert steps == 3 and fin.tolist() == [1, 1, 0] and par.tolist() == [0, 1, 2]
    assert tokens.tolist() == [[1, 4, X], [2, 3, 4], [2, 0, 1]] and lens.tolist() == [2, 3, 3] and scores.tolist() == [-1.5, -1.75, -3.0]
    # without end tokens nothing finishes: token 4 is a token like the others, and "after 4" is asked for
    table = dict(TABLE)
    table[4] = [(0, -1.0), (1, -1.0), (2, -1.0)]
    tokens, lens, scores, _, steps, _, fin = beam_ref.search(_model(table, 2), 0, 2, 3)
    # step 1 as above without finishing: h0 = [1 4] -1.5, h1 = [2 3] -1.5; step 2: h0 (after 4): (0, -2.5) (1, -2.5); h1 (after 3): (4, -1.75) (1, -3.5)
    assert steps == 3 and not fin.any() and tokens.tolist() == [[2, 3, 4], [1, 4, 0]] and scores.tolist() == [-1.75, -2.5] and lens.tolist() == [3, 3]


def test_a_group_with_too_few_candidates_has_dead_hypotheses():
    # after 0 only one entry ranks (the other is without a token); after 1 two do
    table = {0: [(1, -1.0), (NO_TOKEN, -np.inf)], 1: [(2, -1.0), (3, -2.0)], 2: [(0, -1.0), (1, -1.0)], 3: [(0, -1.0), (1, -1.0)]}
    ids, lps = _model(table, 2)(np.array([0, 0]), None, [True, False])
    sc, fin, ln = beam_ref.start(2)
    tok, par, lp, sc, fin, ln = beam_ref.step(ids, lps, sc, fin, ln)
    # h1 is dead: no token, parent itself, score -inf, finished, length 0
    assert tok.tolist() == [1, X] and par.tolist() == [0, 1] and sc.tolist() == [-1.0, -np.inf] and fin.tolist() == [0, 1] and ln.tolist() == [1, 0]
    # ... and offers nothing; the next step fills both places from h0
    ids, lps = _model(table, 2)(np.array([1, 0]), par, [True, False])
    tok, par, lp, sc, fin, ln = beam_ref.step(ids, lps, sc, fin, ln)
    assert tok.tolist() == [2, 3] and par.tolist() == [0, 0] and sc.tolist() == [-2.0, -3.0] and fin.tolist() == [0, 0] and ln.tolist() == [2, 2]
    # a log-prob of -inf or NaN is not offered either; nothing at all leaves the whole group dead
    ids = np.array([[1, 2], [3, 4]], dtype=np.uint32)
    lps = np.array([[-np.inf, np.nan], [-1.0, -1.0]], dtype=np.float32)
    tok, par, lp, sc, fin, ln = beam_ref.step(ids, lps, *beam_ref.start(2))
    assert tok.tolist() == [X, X] and par.tolist() == [0, 1] and np.isneginf(sc).all() and fin.tolist() == [1, 1] and lp.tolist() == [0.0, 0.0]
    tokens, lens, _ = beam_ref.backtrace([tok], [par], [lp], sc, 2)
    assert tokens.tolist() == [[X, X], [X, X]] and lens.tolist() == [0, 0]
    # an all-finished group is unchanged by a step, whatever its lists hold
    tok, par, lp, sc2, fin, ln = beam_ref.step(ids, lps, [-1.0, -1.0], [1, 1], [3, 2])
    assert tok.tolist() == [X, X] and par.tolist() == [0, 1] and sc2.tolist() == [-1.0, -1.0] and fin.tolist() == [1, 1] and ln.tolist() == [3, 2]


# ---- the surface ----

def _pkg():
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    pkg = graft.load_package()
    pkg.build_library()
    return pkg


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    return set(re.findall(r"RWKV_API[^;(]*?\b(rwkv_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


def test_headers_declare_the_calls():
    assert set(SYMBOLS) <= _declared("rwkv_mi355x.h")
    assert _declared("rwkv_testhooks_beam.h") == {HOOK}
    header = open(os.path.join(ROOT, "include", "rwkv_mi355x.h")).read()
    for name, value in (("STATE", 1), ("COUNTER", 2), ("COUNTS", 4), ("BIAS", 8)):
        assert re.search(r"#define\s+RWKV_MI_COPY_%s\s+%du\b" % (name, value), header), name


def test_libraries_export_them_and_the_hook_stays_out_of_the_product():
    pkg = _pkg()
    for path in (pkg.LIB_PATH, pkg.HOOKS_LIB_PATH, pkg.SAMPLE_HOOKS_LIB_PATH):
        so = ctypes.CDLL(path)
        for name in SYMBOLS:
            assert hasattr(so, name), (path, name)
    assert hasattr(ctypes.CDLL(pkg.SAMPLE_HOOKS_LIB_PATH), HOOK)
    assert not hasattr(ctypes.CDLL(pkg.LIB_PATH), HOOK) and not hasattr(ctypes.CDLL(pkg.HOOKS_LIB_PATH), HOOK)


def test_binding_wires_the_argument_types():
    pkg = _pkg()
    lib = pkg.load_rwkv_shared_library()
    assert len(lib.library.rwkv_mi_batch_state_copy.argtypes) == 4 and len(lib.library.rwkv_mi_batch_decode_beam.argtypes) == 11
    for name in SYMBOLS:
        assert getattr(lib.library, name).restype is ctypes.c_bool, name
    assert ctypes.sizeof(pkg.BeamParams) == 16
    hooks = pkg.RWKVSharedLibrary(pkg.SAMPLE_HOOKS_LIB_PATH)
    assert len(hooks.library.rwkv_test_beam_step.argtypes) == 13 and hooks.library.rwkv_test_beam_step.restype is ctypes.c_bool
    assert callable(pkg.RWKVBatch.decode_beam) and callable(pkg.RWKVBatch.copy_state)
