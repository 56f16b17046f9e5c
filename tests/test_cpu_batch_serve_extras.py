"""Served requests with a guide, a bias and the report (rwkv_mi_batch_serve_ex), without a GPU: the exported symbol and its declaration, the
16-byte extras struct and its builder in the binding, the request builder as it was, and the kernels from their code objects -- the scheduler
k_serve_rows is still two instantiations within a 1024-thread workgroup's budget, and the report's serve entry point of csrc/score.hip has
the shape of the entry points beside it."""
import ctypes
import os
import re

import pytest

import kernel_meta
from test_cpu_batch_serve import SERVE_ROWS, _pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_GUIDE = NO_SLOT = 0xFFFFFFFF


def test_libraries_export_the_symbol_and_the_header_declares_it():
    pkg = _pkg()
    for path in (pkg.LIB_PATH, pkg.HOOKS_LIB_PATH, pkg.SAMPLE_HOOKS_LIB_PATH):
        assert hasattr(ctypes.CDLL(path), "rwkv_mi_batch_serve_ex"), path
    header = open(os.path.join(ROOT, "include", "rwkv_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert "rwkv_mi_batch_serve_ex" in re.findall(r"RWKV_API[^;(]*?\b(rwkv_\w+)\s*\(", code)
    fields = re.search(r"struct\s+rwkv_mi_serve_extra\s*\{(.*?)\}", code, re.S).group(1)
    assert re.findall(r"uint32_t\s+(\w+)\s*;", fields) == ["guide", "guide_state", "bias_slot", "reserved"]
    # the 17 arguments of rwkv_mi_batch_serve, then extras and the two guide outputs
    decl = lambda name: re.search(r"RWKV_API\s+bool\s+" + name + r"\s*\((.*?)\)\s*;", code, re.S).group(1)   # noqa: E731
    old, new = [a.strip() for a in decl("rwkv_mi_batch_serve").split(",")], [a.strip() for a in decl("rwkv_mi_batch_serve_ex").split(",")]
    assert len(old) == 17 and new[:17] == old
    assert [re.sub(r"\s+", " ", a) for a in new[17:]] == ["const struct rwkv_mi_serve_extra * extras", "uint32_t * guide_state_out", "uint32_t * guide_misses_out"]


def test_binding_declares_the_call_and_lays_the_extra_out_as_the_header_does():
    pkg = _pkg()
    lib = pkg.load_rwkv_shared_library()
    f, old = lib.library.rwkv_mi_batch_serve_ex, lib.library.rwkv_mi_batch_serve
    assert f.restype is ctypes.c_bool and len(f.argtypes) == 20 and len(old.argtypes) == 17
    assert list(f.argtypes[:17]) == list(old.argtypes)
    assert f.argtypes[17] is ctypes.POINTER(pkg.ServeExtra)
    E = pkg.ServeExtra
    assert ctypes.sizeof(E) == 16
    assert [E.guide.offset, E.guide_state.offset, E.bias_slot.offset, E.reserved.offset] == [0, 4, 8, 12]
    assert pkg.NO_GUIDE == NO_GUIDE and pkg.NO_SLOT == NO_SLOT


def test_extras_builder_defaults_and_none_for_a_queue_without_extras():
    pkg = _pkg()
    plain = [dict(prompt=[1, 2], max_tokens=3), dict(prompt=[4], max_tokens=1, top_k=5)]
    assert pkg.serve_extras(plain) is None and pkg.serve_extras([]) is None
    queue = [dict(prompt=[1, 2], max_tokens=3), dict(prompt=[4], max_tokens=2, guide=1, guide_state=7), dict(prompt=[5], max_tokens=2, bias_slot=3),
             dict(prompt=[6], max_tokens=2, guide=0, bias_slot=4), dict(prompt=[7], max_tokens=2, guide=None, bias_slot=None)]
    ex = pkg.serve_extras(queue)
    assert len(ex) == len(queue)
    words = [(e.guide, e.guide_state, e.bias_slot, e.reserved) for e in ex]
    assert words == [(NO_GUIDE, 0, NO_SLOT, 0), (1, 7, NO_SLOT, 0), (NO_GUIDE, 0, 3, 0), (0, 0, 4, 0), (NO_GUIDE, 0, NO_SLOT, 0)]
    # one request that names a key is enough for a table, the others get the defaults
    ex = pkg.serve_extras(plain + [dict(prompt=[1], max_tokens=1, guide_state=2)])
    assert [(e.guide, e.guide_state, e.bias_slot, e.reserved) for e in ex] == [(NO_GUIDE, 0, NO_SLOT, 0)] * 2 + [(NO_GUIDE, 2, NO_SLOT, 0)]


def test_request_builder_returns_what_it_returned_and_takes_the_new_keys():
    pkg = _pkg()
    old = [dict(prompt=[5, 6, 7], max_tokens=9, stop=[[1], [2, 3]], from_slot=4, temperature=1.5, top_p=0.9, seed=11, presence=0.25, frequency=0.5, top_k=7,
                min_p=0.05, decay=0.996, repetition=1.1), dict(prompt=[8], max_tokens=1)]
    new = [dict(old[0], guide=2, guide_state=1), dict(old[1], bias_slot=3)]
    a, b = pkg.serve_requests(old), pkg.serve_requests(new)
    assert len(a) == len(b) == 4
    assert bytes(a[0]) == bytes(b[0]) and ctypes.sizeof(a[0]) == 2 * 72
    for x, y in zip(a[1:], b[1:]):
        assert x.dtype == y.dtype and x.tolist() == y.tolist()
    assert a[1].tolist() == [5, 6, 7, 8] and a[2].tolist() == [1, 2] and a[3].tolist() == [1, 2, 3]
    with pytest.raises(ValueError):
        pkg.serve_requests([dict(prompt=[1], max_tokens=3, giude=1)])   # (a misspelt key is not dropped silently)
    with pytest.raises(ValueError):
        pkg.serve_requests([dict(prompt=[1], max_tokens=3, guide=1, temprature=1.0)])


@pytest.mark.skipif(not kernel_meta.have_hipcc(), reason="needs hipcc")
def test_scheduler_is_still_two_instantiations_and_the_report_entry_point_has_the_shape_of_its_neighbours():
    assert set(kernel_meta.named("sampling.hip", "k_serve_rows")) == SERVE_ROWS == {(0,), (1,)}
    kernel_meta.budget("sampling.hip", tuple(("k_serve_rows", a) for a in sorted(SERVE_ROWS)))
    # 1024 threads, no private segment, no spills, at most 128 registers per thread
    kernel_meta.budget("score.hip", ("k_logprob_rows_serve", "k_logprob_rows", "k_logprob_rows_live"))
