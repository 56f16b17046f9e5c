"""What the device weight quantiser (csrc/quant_w.hip: rwkv_mi_init_from_file_as, rwkv_mi_quantize_model_file) shows without a GPU: its
declarations, its argument errors, that it refuses to run on the host, and the register budget of its kernels."""
import os
import re

import pytest

import kernel_meta as K
import reference_constants as R
from gpu_lib import ROOT, library

ARGS, FILE, CTX = 1 << 8, 2 << 8, 6 << 8
DATA_TYPE, UNSUPPORTED = 8, 9
T_F32, T_F16 = 0, 1
Q_TYPES = (2, 3, 7, 8, 9)   # Q4_0, Q4_1, Q5_0, Q5_1, Q8_0 (csrc/common.h, DType)


def test_header_and_binding_declare_both_functions():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rwkv_mi355x.h")).read(), flags=re.S)
    L = library().library
    for name, n_args in (("rwkv_mi_init_from_file_as", 4), ("rwkv_mi_quantize_model_file", 3)):
        m = re.search(r"RWKV_API[^;(]*\b" + name + r"\s*\(([^)]*)\)", text)
        assert m and len(m.group(1).split(",")) == n_args, name
        assert len(getattr(L, name).argtypes) == n_args, name


@pytest.fixture
def quiet():
    lib = library()
    lib.rwkv_set_print_errors(None, False)
    yield lib
    lib.rwkv_set_print_errors(None, True)


def test_argument_errors_need_no_device(quiet, golden_dir, tmp_path):
    L = quiet.library
    src, out = R.fixture_path(golden_dir, "5v2-730K", "FP32").encode(), str(tmp_path / "x.bin").encode()
    for bad in (b"Q4_3", b"FP16", b"nonsense"):
        assert not L.rwkv_mi_init_from_file_as(src, 1, 0, bad)
        assert quiet.rwkv_get_last_error(None) == ARGS | DATA_TYPE, bad
        assert not L.rwkv_mi_quantize_model_file(src, out, bad)
        assert quiet.rwkv_get_last_error(None) == ARGS | DATA_TYPE, bad
    assert not L.rwkv_mi_init_from_file_as(None, 1, 0, b"Q4_0") and quiet.rwkv_get_last_error(None) == ARGS
    assert not L.rwkv_mi_init_from_file_as(src, 1, 0, None) and quiet.rwkv_get_last_error(None) == ARGS
    assert not L.rwkv_mi_quantize_model_file(None, out, b"Q4_0") and quiet.rwkv_get_last_error(None) == ARGS
    assert not L.rwkv_mi_quantize_model_file(src, None, b"Q4_0") and quiet.rwkv_get_last_error(None) == ARGS
    assert not os.path.exists(out)
    # an already quantised file: FILE, as the host quantiser answers
    q = R.fixture_path(golden_dir, "5v2-730K", "Q5_0").encode()
    assert not L.rwkv_mi_init_from_file_as(q, 1, 0, b"Q4_0") and quiet.rwkv_get_last_error(None) == FILE
    assert not L.rwkv_mi_quantize_model_file(q, out, b"Q4_0") and quiet.rwkv_get_last_error(None) == FILE


def test_no_host_fallback_without_a_gpu(quiet, golden_dir, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    L = quiet.library
    src, out = R.fixture_path(golden_dir, "5v2-730K", "FP16").encode(), str(tmp_path / "x.bin")
    assert not L.rwkv_mi_init_from_file_as(src, 1, 0, b"Q5_1")
    err = quiet.rwkv_get_last_error(None)
    assert err & CTX == CTX and (err & 0xFF) == UNSUPPORTED
    assert not L.rwkv_mi_quantize_model_file(src, out.encode(), b"Q5_1")
    err = quiet.rwkv_get_last_error(None)
    assert err & CTX == CTX and (err & 0xFF) == UNSUPPORTED and not os.path.exists(out)


@pytest.mark.skipif(not K.have_hipcc(), reason="hipcc is not installed")
def test_kernels_have_no_private_segment_and_no_spills():
    """k_quant_w<source, format, form>: the lane's 32 elements and its codes live in registers"""
    keys = [("k_quant_w", (s, t, form)) for s in (T_F32, T_F16) for t in Q_TYPES for form in (0, 1)]
    found = K.no_scratch("quant_w.hip", keys)
    assert set(K.named("quant_w.hip", "k_quant_w")) == {k[1] for k in keys}
    for k in found.values():
        assert k.wg == 256 and k.lds <= 48 * 1024, k
