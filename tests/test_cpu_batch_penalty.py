"""Presence / frequency penalties and logit bias in the device sampler, without a GPU: the libraries export the entry points of
include/rwkv_mi355x.h's penalty family, the Python binding declares them (and lays struct rwkv_mi_penalty_params out as the C header does),
and the four entry points of the sampler kernel (csrc/sampling.hip: k_draw<plain, 0>, k_draw_rows<plain, 0, 0> and the penalised k_draw<pen, 0>,
k_draw_rows<pen, 0, 0>) keep within the budget of a 1024-thread workgroup: 128 registers per thread, no private segment, no spills."""
import ctypes
import os
import re

import pytest

import kernel_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rwkv_mi_batch_counts_reset", "rwkv_mi_batch_counts_add", "rwkv_mi_batch_counts_store", "rwkv_mi_batch_logit_bias_set",
           "rwkv_mi_batch_eval_sample_penalized", "rwkv_mi_batch_eval_ragged_sample_penalized", "rwkv_mi_batch_decode_sample_penalized",
           "rwkv_mi_counts_reset", "rwkv_mi_counts_add", "rwkv_mi_counts_store", "rwkv_mi_logit_bias_set", "rwkv_mi_rng_seek",
           "rwkv_mi_sample_penalized", "rwkv_mi_decode_sample_penalized")
# k_draw<SRC, CUT> and k_draw_rows<SRC, CUT, GUIDED> on the plain (0) and the penalised (1) source, no other axis set: what k_sample,
# k_sample_rows, k_pen_sample and k_pen_sample_rows were
KERNELS = (("k_draw", (0, 0)), ("k_draw_rows", (0, 0, 0)), ("k_draw", (1, 0)), ("k_draw_rows", (1, 0, 0)))


def _pkg():
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    pkg = graft.load_package()
    pkg.build_library()
    return pkg


def test_libraries_export_the_penalty_symbols():
    pkg = _pkg()
    for path in (pkg.LIB_PATH, pkg.HOOKS_LIB_PATH, pkg.SAMPLE_HOOKS_LIB_PATH):
        so = ctypes.CDLL(path)
        for name in SYMBOLS:
            assert hasattr(so, name), (path, name)
    header = open(os.path.join(ROOT, "include", "rwkv_mi355x.h")).read()
    declared = re.findall(r"RWKV_API[^;(]*?\b(rwkv_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert set(SYMBOLS) <= set(declared), sorted(set(SYMBOLS) - set(declared))


def test_binding_declares_the_penalty_symbols():
    pkg = _pkg()
    lib = pkg.load_rwkv_shared_library()
    for name in SYMBOLS:
        f = getattr(lib.library, name)
        assert f.argtypes is not None, name
        assert f.restype is ctypes.c_bool, name
    # struct rwkv_mi_penalty_params { float presence; float frequency; uint32_t record; }
    assert ctypes.sizeof(pkg.PenaltyParams) == 12
    assert [pkg.PenaltyParams.presence.offset, pkg.PenaltyParams.frequency.offset, pkg.PenaltyParams.record.offset] == [0, 4, 8]
    for meth in ("eval_sample_penalized", "eval_ragged_sample_penalized", "decode_sample_penalized", "counts_reset", "counts_add", "counts",
                 "set_logit_bias"):
        assert callable(getattr(pkg.RWKVBatch, meth)), meth
    for meth in ("sample_penalized", "decode_sample_penalized", "counts_reset", "counts_add", "counts", "set_logit_bias", "rng_seek"):
        assert callable(getattr(pkg.RWKVModel, meth)), meth


def test_penalty_rows_take_scalars_or_sequences():
    pkg = _pkg()
    rows = pkg.penalty_params(3, 0.25, [0.5, 0.0, 1.0])
    assert [(r.presence, r.frequency, r.record) for r in rows] == [(0.25, 0.5, 1), (0.25, 0.0, 1), (0.25, 1.0, 1)]
    rows = pkg.penalty_params(3, [0.0, 0.5, 2.0], 0.5, record=[True, False, True])
    assert [(r.presence, r.frequency, r.record) for r in rows] == [(0.0, 0.5, 1), (0.5, 0.5, 0), (2.0, 0.5, 1)]
    assert [r.record for r in pkg.penalty_params(2, 0.0, 0.0, record=False)] == [0, 0]
    with pytest.raises(ValueError):
        pkg.penalty_params(3, [0.25, 0.5], 0.5)
    with pytest.raises(ValueError):
        pkg.penalty_params(3, 0.25, 0.5, record=[True, False])


@pytest.mark.skipif(not kernel_meta.have_hipcc(), reason="needs hipcc")
def test_penalised_and_plain_entry_points_keep_the_budget():
    kernel_meta.budget("sampling.hip", KERNELS)
