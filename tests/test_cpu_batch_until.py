"""Stop sequences and per-row token budgets in the batch decode loops (rwkv_mi_batch_decode_until), without a GPU: the libraries export the
two entry points, the header and the binding declare them, struct rwkv_mi_stop_params is laid out as the C header has it, decode_until's
arguments are shaped as documented, and csrc/sampling.hip has exactly its four draw entry points and the stop test k_stop_rows: all five keep
within the budget of a 1024-thread workgroup, and the four draw entry points -- the two row forms now take the live words of decode_until as
a last argument that may be NULL -- keep the registers they had before that argument.

stop_rule() below is the stop rule of include/rwkv_mi355x.h restated in Python; tests/test_gpu_batch_until.py imports it as its matcher."""
import ctypes
import os
import re

import numpy as np
import pytest

import kernel_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rwkv_mi_batch_decode_until", "rwkv_mi_batch_last_loop_passes")
NO_TOKEN = 0xFFFFFFFF
# (sgpr_count, vgpr_count) of the four draw entry points as the commit before decode_until compiled them for gfx950: they must not move. They
# were k_sample, k_sample_rows, k_pen_sample, k_pen_sample_rows then; now the plain and the penalised source of k_draw<SRC, CUT> and
# k_draw_rows<SRC, CUT, GUIDED> with no other axis set
PARENT_REGS = {("k_draw", (0, 0)): (48, 39), ("k_draw_rows", (0, 0, 0)): (52, 39), ("k_draw", (1, 0)): (50, 39), ("k_draw_rows", (1, 0, 0)): (54, 39)}
NEW_KERNELS = ("k_stop_rows",)


def stop_rule(tokens, max_tokens, seqs):
    """(length, stopped_by) of a row that emits `tokens` (at least max_tokens of them, the tokens of THIS call only) under a budget of
    max_tokens and the stop sequences `seqs`: the row retires after the first pass i at which tokens[0..i] end with one of the sequences --
    the lowest index among those that match, also at the budget's last step -- or i + 1 == max_tokens (stopped_by NO_TOKEN)."""
    tokens = [int(t) for t in tokens]
    for i in range(max_tokens):
        for k, q in enumerate(seqs):
            q = [int(t) for t in q]
            if len(q) <= i + 1 and tokens[i + 1 - len(q): i + 1] == q:
                return i + 1, k
    return max_tokens, NO_TOKEN


def _pkg():
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    pkg = graft.load_package()
    pkg.build_library()
    return pkg


def test_libraries_export_the_until_symbols():
    pkg = _pkg()
    for path in (pkg.LIB_PATH, pkg.HOOKS_LIB_PATH, pkg.SAMPLE_HOOKS_LIB_PATH):
        so = ctypes.CDLL(path)
        for name in SYMBOLS:
            assert hasattr(so, name), (path, name)
    header = open(os.path.join(ROOT, "include", "rwkv_mi355x.h")).read()
    declared = re.findall(r"RWKV_API[^;(]*?\b(rwkv_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert set(SYMBOLS) <= set(declared), sorted(set(SYMBOLS) - set(declared))
    for macro, value in (("RWKV_MI_STOP_MAX_SEQS", "16"), ("RWKV_MI_STOP_MAX_LEN", "8"), ("RWKV_MI_NO_TOKEN", "UINT32_MAX")):
        assert re.search(r"#define\s+" + macro + r"\s+" + value + r"\b", header), macro


def test_binding_declares_the_until_symbols():
    pkg = _pkg()
    lib = pkg.load_rwkv_shared_library()
    f = lib.library.rwkv_mi_batch_decode_until
    assert f.restype is ctypes.c_bool and len(f.argtypes) == 14
    g = lib.library.rwkv_mi_batch_last_loop_passes
    assert g.restype is ctypes.c_size_t and len(g.argtypes) == 1
    # struct rwkv_mi_stop_params { uint32_t max_tokens; uint32_t n_seqs; }
    assert ctypes.sizeof(pkg.StopParams) == 8
    assert [pkg.StopParams.max_tokens.offset, pkg.StopParams.n_seqs.offset] == [0, 4]
    assert pkg.NO_TOKEN == NO_TOKEN
    for meth in ("decode_until", "last_loop_passes"):
        assert callable(getattr(pkg.RWKVBatch, meth)), meth


def test_stop_arguments_take_scalars_or_rows():
    pkg = _pkg()

    def shaped(n, max_tokens, stop):
        rows, lens, toks = pkg.stop_params(n, max_tokens, stop)
        return [(r.max_tokens, r.n_seqs) for r in rows], lens.tolist(), toks.tolist()

    # a scalar budget, no sequences
    assert shaped(3, 24, None) == ([(24, 0)] * 3, [], [])
    # one list of sequences for all rows
    assert shaped(2, 24, [[0], [187, 187]]) == ([(24, 2), (24, 2)], [1, 2, 1, 2], [0, 187, 187, 0, 187, 187])
    # a budget per row, a list per row (one of them empty)
    assert shaped(3, [4, 5, 6], [[[0]], [], [[187, 187], [535], [1, 2, 3]]]) == ([(4, 1), (5, 0), (6, 3)], [1, 2, 1, 3], [0, 187, 187, 535, 1, 2, 3])
    # n empty lists: no row has a sequence
    assert shaped(2, 7, [[], []]) == ([(7, 0), (7, 0)], [], [])
    assert pkg.stop_params(2, 7, [[0]])[1].dtype == np.uint32 and pkg.stop_params(2, 7, [[0]])[2].dtype == np.uint32
    with pytest.raises(ValueError):
        pkg.stop_params(3, [4, 5], None)
    with pytest.raises(ValueError):
        pkg.stop_params(3, 8, [[[0]], [[1]]])   # (per-row lists for two rows of three)


def test_stop_rule_hand_written_cases():
    a, b, c = 5, 6, 7
    # a stop token: emitted, then the row ends
    assert stop_rule([b, a, c, c], 4, [[a]]) == (2, 0)
    # after pass 0
    assert stop_rule([a, b, c], 3, [[a]]) == (1, 0)
    # the budget, nothing matched
    assert stop_rule([b, b, b, b], 3, [[a]]) == (3, NO_TOKEN)
    assert stop_rule([b, b, b, b], 3, []) == (3, NO_TOKEN)
    # the lowest index wins when two match at the same step ...
    assert stop_rule([c, a, b], 3, [[a, b], [b]]) == (3, 0)
    assert stop_rule([c, a, b], 3, [[b], [a, b]]) == (3, 0)
    # ... but an earlier step wins over a lower index
    assert stop_rule([c, a, b], 3, [[a, b], [a]]) == (2, 1)
    # a match at the budget's last step reports the match
    assert stop_rule([c, c, a, a], 3, [[c, a]]) == (3, 0)
    # the window is this call's tokens only: [a, b] cannot match at the first token, whatever was fed
    assert stop_rule([b, c, c], 3, [[a, b]]) == (3, NO_TOKEN)
    assert stop_rule([b, a, b], 4, [[a, b]]) == (3, 0)
    # overlapping: [a, a] on a a a retires at the second token
    assert stop_rule([a, a, a], 3, [[a, a]]) == (2, 0)
    # a sequence longer than the budget never matches
    assert stop_rule([a, b, c], 2, [[a, b, c]]) == (2, NO_TOKEN)
    # three tokens
    assert stop_rule([c, a, b, c, a], 5, [[a, b, c]]) == (4, 0)


@pytest.mark.skipif(not kernel_meta.have_hipcc(), reason="needs hipcc")
def test_draw_entry_points_and_stop_test_keep_the_budget_and_the_four_their_registers():
    drawn = kernel_meta.budget("sampling.hip", tuple(PARENT_REGS))
    kernel_meta.budget("sampling.hip", NEW_KERNELS, wg=64)
    for key, k in drawn.items():
        assert (k.sgprs, k.vgprs) == PARENT_REGS[key], (key, k, PARENT_REGS[key])
