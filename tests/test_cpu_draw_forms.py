"""The draw kernels of csrc/sampling.hip, without a GPU: every entry point is an instantiation of one body (draw_row) on three compile-time
axes, and a launcher's switch decides which exist. The compiled file holds EXACTLY the forms a call can name -- a stray instantiation is what
the one-body design invites, and each costs compile time and code size for a kernel nothing launches."""
import pytest

import kernel_meta

PLAIN, PEN, REP = 0, 1, 2   # SRC: what the draw reads (model.h)
# k_draw<SRC, CUT>: a context's draw
CONTEXT = {(PLAIN, 0), (PLAIN, 1), (PEN, 0), (PEN, 1), (REP, 1)}
# k_draw_rows<SRC, CUT, GUIDED>: a batch pass's; the repetition and the guided forms exist with CUT only
ROWS = {(PLAIN, 0, 0), (PLAIN, 1, 0), (PLAIN, 1, 1), (PEN, 0, 0), (PEN, 1, 0), (PEN, 1, 1), (REP, 1, 0), (REP, 1, 1)}
# k_draft_accept_rows<FAMILY>: 0 the greedy walk, 1 + SRC a drawing one
WALK = {(0,), (1 + PLAIN,), (1 + PEN,), (1 + REP,)}


@pytest.mark.skipif(not kernel_meta.have_hipcc(), reason="needs hipcc")
def test_exactly_the_seventeen_draw_kernels_are_compiled():
    assert set(kernel_meta.named("sampling.hip", "k_draw")) == CONTEXT
    assert set(kernel_meta.named("sampling.hip", "k_draw_rows")) == ROWS
    assert set(kernel_meta.named("sampling.hip", "k_draft_accept_rows")) == WALK
    # ... and nothing else in the file draws: every other kernel is one of the helpers around them
    others = {key for key in kernel_meta.kernels("sampling.hip") if not isinstance(key, tuple)}
    assert others == {"k_stop_rows", "k_guide_expand", "k_count_add", "k_count_add_decay", "k_bias_scatter", "k_sample_seek_rows"}, others
