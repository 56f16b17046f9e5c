"""Host-side mirror of the reference's Python binding on top of the C ABI of librwkv.so.

Mirrors python/rwkv_cpp/rwkv_cpp_shared_library.py (RWKVSharedLibrary: one method per rwkv.h entry point, same
names and argument meaning, ValueError on failure) and python/rwkv_cpp/rwkv_cpp_model.py (RWKVModel: eval /
eval_sequence / eval_sequence_in_chunks returning (logits, state)) of RWKV/rwkv.cpp @ 2025-02-19, plus the rwkv_mi_*
extensions. The reference's own wrapper also works unchanged against this library.

There is no fallback: if librwkv.so is missing or no MI355X is visible, loading / init raises.
"""
import ctypes
import os
import subprocess
from typing import List, Optional, Tuple

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# RWKV_LIB_DIR selects an alternative in-tree build directory (A/B variants built with `make LIBDIR=... OBJDIR=... EXTRA=-D...`)
LIB_PATH = os.path.join(PKG_DIR, os.environ.get("RWKV_LIB_DIR", "lib"), "librwkv.so")
# tests/ only: the same objects + csrc/testhooks.cpp (include/rwkv_testhooks.h); the product library does not export test entry points
HOOKS_LIB_PATH = os.path.join(PKG_DIR, os.environ.get("RWKV_LIB_DIR", "lib"), "librwkv_testhooks.so")
# tests/ only: the same objects + csrc/testhooks_sample.cpp (include/rwkv_testhooks_sample.h): the sampler kernel on caller-supplied logits
SAMPLE_HOOKS_LIB_PATH = os.path.join(PKG_DIR, os.environ.get("RWKV_LIB_DIR", "lib"), "librwkv_testhooks_sample.so")
# tests/ only: the same objects + csrc/testhooks_guide.cpp (include/rwkv_testhooks_guide.h): the guided sampler kernels on caller-supplied logits
GUIDE_HOOKS_LIB_PATH = os.path.join(PKG_DIR, os.environ.get("RWKV_LIB_DIR", "lib"), "librwkv_testhooks_guide.so")
# tests/ only: the same objects + csrc/testhooks_cut.cpp (include/rwkv_testhooks_cut.h): the plain sampler with a truncation setting per row
CUT_HOOKS_LIB_PATH = os.path.join(PKG_DIR, os.environ.get("RWKV_LIB_DIR", "lib"), "librwkv_testhooks_cut.so")

# tests/ only: the same objects + csrc/testhooks_decay.cpp (include/rwkv_testhooks_decay.h): the penalised sampler with a repetition setting per row
DECAY_HOOKS_LIB_PATH = os.path.join(PKG_DIR, os.environ.get("RWKV_LIB_DIR", "lib"), "librwkv_testhooks_decay.so")

QUANTIZED_FORMAT_NAMES =("Q4_0", "Q4_1", "Q5_0", "Q5_1", "Q8_0")
PENALTY_SYMBOLS = ("rwkv_mi_batch_counts_reset", "rwkv_mi_batch_counts_add", "rwkv_mi_batch_counts_store", "rwkv_mi_batch_logit_bias_set",
                   "rwkv_mi_batch_eval_sample_penalized", "rwkv_mi_batch_eval_ragged_sample_penalized", "rwkv_mi_batch_decode_sample_penalized",
                   "rwkv_mi_counts_reset", "rwkv_mi_counts_add", "rwkv_mi_counts_store", "rwkv_mi_logit_bias_set", "rwkv_mi_rng_seek",
                   "rwkv_mi_sample_penalized", "rwkv_mi_decode_sample_penalized")
SCORE_SYMBOLS = ("rwkv_mi_score_resident", "rwkv_mi_batch_score_ragged")
UNTIL_SYMBOLS = ("rwkv_mi_batch_decode_until", "rwkv_mi_batch_last_loop_passes")
SERVE_SYMBOLS = ("rwkv_mi_batch_serve", "rwkv_mi_batch_serve_ex")
LOGPROBS_SYMBOLS = ("rwkv_mi_batch_set_logprobs", "rwkv_mi_batch_logprobs_shape", "rwkv_mi_batch_logprobs_store",
                    "rwkv_mi_set_logprobs", "rwkv_mi_logprobs_shape", "rwkv_mi_logprobs_store")
BEAM_SYMBOLS = ("rwkv_mi_batch_state_copy", "rwkv_mi_batch_decode_beam")
GUIDE_SYMBOLS = ("rwkv_mi_batch_guide_create", "rwkv_mi_batch_guide_free", "rwkv_mi_batch_guide_attach", "rwkv_mi_batch_guide_state")
GUIDE_MAX = 16              # RWKV_MI_GUIDE_MAX: guides per batch
GUIDE_MAX_STATES = 65535    # RWKV_MI_GUIDE_MAX_STATES: states per guide
NO_GUIDE = 0xFFFFFFFF       # RWKV_MI_NO_GUIDE: a slot without a guide
DRAFT_SYMBOLS = ("rwkv_mi_batch_eval_draft",)
TRUNCATION_SYMBOLS = ("rwkv_mi_batch_truncation_set", "rwkv_mi_batch_truncation_get", "rwkv_mi_truncation_set", "rwkv_mi_truncation_get")
REPETITION_SYMBOLS = ("rwkv_mi_batch_repetition_set", "rwkv_mi_batch_repetition_get", "rwkv_mi_batch_counts_store_f32",
                      "rwkv_mi_repetition_set", "rwkv_mi_repetition_get", "rwkv_mi_counts_store_f32")
DRAFT_MAX = 8               # RWKV_MI_DRAFT_MAX: draft tokens per row of RWKVBatch.eval_draft
COPY_STATE, COPY_COUNTER, COPY_COUNTS, COPY_BIAS = 1, 2, 4, 8  # RWKV_MI_COPY_*: the bits of rwkv_mi_batch_state_copy's `what`
TOP_MAX = 20             # RWKV_MI_TOP_MAX: the most alternatives a report holds per token, and the widest beam
NO_TARGET = 0xFFFFFFFF   # RWKV_MI_NO_TARGET: a position that is not scored (its log-prob is 0)
NO_TOKEN = 0xFFFFFFFF    # RWKV_MI_NO_TOKEN: no token (past a row's length), no stop sequence (the budget ended the row)
STOP_MAX_SEQS = 16       # RWKV_MI_STOP_MAX_SEQS
STOP_MAX_LEN = 8         # RWKV_MI_STOP_MAX_LEN
NO_SLOT = 0xFFFFFFFF     # RWKV_MI_NO_SLOT
SERVE_GREEDY, SERVE_SAMPLE, SERVE_PENALIZED = 0, 1, 2   # RWKV_MI_SERVE_*
SERVE_EXTRA_KEYS = ("guide", "guide_state", "bias_slot")   # the keys of a request dict that serve_extras reads (struct rwkv_mi_serve_extra)
P_FLOAT = ctypes.POINTER(ctypes.c_float)
P_UINT32 = ctypes.POINTER(ctypes.c_uint32)


class SampleParams(ctypes.Structure):
    """struct rwkv_mi_sample_params (include/rwkv_mi355x.h): one row's sampling parameters, 24 bytes."""
    _fields_ = [("temperature", ctypes.c_float), ("top_p", ctypes.c_float), ("u", ctypes.c_float), ("seed", ctypes.c_uint64)]


P_SAMPLE_PARAMS = ctypes.POINTER(SampleParams)


class PenaltyParams(ctypes.Structure):
    """struct rwkv_mi_penalty_params (include/rwkv_mi355x.h): one row's presence / frequency penalty and its record flag, 12 bytes."""
    _fields_ = [("presence", ctypes.c_float), ("frequency", ctypes.c_float), ("record", ctypes.c_uint32)]


P_PENALTY_PARAMS = ctypes.POINTER(PenaltyParams)


class StopParams(ctypes.Structure):
    """struct rwkv_mi_stop_params (include/rwkv_mi355x.h): one row's token budget and the number of its stop sequences, 8 bytes."""
    _fields_ = [("max_tokens", ctypes.c_uint32), ("n_seqs", ctypes.c_uint32)]


P_STOP_PARAMS = ctypes.POINTER(StopParams)


class ServeRequest(ctypes.Structure):
    """struct rwkv_mi_serve_request (include/rwkv_mi355x.h): one request of RWKVBatch.serve -- prompt length, start slot, draw settings, budget and
    number of stop sequences -- 72 bytes."""
    _fields_ = [("prompt_len", ctypes.c_uint32), ("from_slot", ctypes.c_uint32), ("sample", SampleParams), ("penalty", PenaltyParams),
                ("top_k", ctypes.c_uint32), ("min_p", ctypes.c_float), ("decay", ctypes.c_float), ("repetition", ctypes.c_float),
                ("stop", StopParams), ("reserved", ctypes.c_uint32)]


P_SERVE_REQUEST = ctypes.POINTER(ServeRequest)


class ServeExtra(ctypes.Structure):
    """struct rwkv_mi_serve_extra (include/rwkv_mi355x.h): what a request of RWKVBatch.serve carries beyond its ServeRequest -- its guide and the
    state it enters it in, the slot whose bias table it reads -- 16 bytes."""
    _fields_ = [("guide", ctypes.c_uint32), ("guide_state", ctypes.c_uint32), ("bias_slot", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


P_SERVE_EXTRA = ctypes.POINTER(ServeExtra)

SESSION_SYMBOLS = ("rwkv_mi_batch_serve_open", "rwkv_mi_batch_serve_submit", "rwkv_mi_batch_serve_cancel", "rwkv_mi_batch_serve_poll",
                   "rwkv_mi_batch_serve_stats", "rwkv_mi_batch_serve_close")
STOP_CANCELLED = 0xFFFFFFFE                            # RWKV_MI_STOP_CANCELLED: stopped_by of a request that was cancelled
SERVE_CUT, SERVE_REP, SERVE_GUIDED = 1, 2, 4           # RWKV_MI_SERVE_*: the features of a serve session
POLL_DRAIN = 1                                         # RWKV_MI_POLL_DRAIN


class ServeLimits(ctypes.Structure):
    """struct rwkv_mi_serve_limits (include/rwkv_mi355x.h): the ring and the per-request limits of a serve session, 28 bytes."""
    _fields_ = [("capacity", ctypes.c_uint32), ("max_prompt", ctypes.c_uint32), ("stride", ctypes.c_uint32), ("max_seqs", ctypes.c_uint32),
                ("max_seq_tokens", ctypes.c_uint32), ("features", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class ServeEvent(ctypes.Structure):
    """struct rwkv_mi_serve_event (include/rwkv_mi355x.h): what a poll of a serve session delivers for one request, 36 bytes."""
    _fields_ = [("id", ctypes.c_uint32), ("first", ctypes.c_uint32), ("n_new", ctypes.c_uint32), ("finished", ctypes.c_uint32),
                ("stopped_by", ctypes.c_uint32), ("lane", ctypes.c_uint32), ("start_pass", ctypes.c_uint32), ("guide_state", ctypes.c_uint32),
                ("guide_misses", ctypes.c_uint32)]


class CutParams(ctypes.Structure):
    """struct rwkv_mi_test_cut (include/rwkv_testhooks_cut.h): one row's truncation setting as the test hook takes it, 8 bytes."""
    _fields_ = [("top_k", ctypes.c_uint32), ("min_p", ctypes.c_float)]


class RepParams(ctypes.Structure):
    """struct rwkv_mi_test_rep (include/rwkv_testhooks_decay.h): one row's repetition setting as the test hook takes it, 8 bytes."""
    _fields_ = [("decay", ctypes.c_float), ("repetition", ctypes.c_float)]


class BeamParams(ctypes.Structure):
    """struct rwkv_mi_beam_params (include/rwkv_mi355x.h): the beam width and the ids that finish a hypothesis, 16 bytes."""
    _fields_ = [("width", ctypes.c_uint32), ("n_end", ctypes.c_uint32), ("end_tokens", P_UINT32)]


def build_library(force: bool = False) -> str:
    """Compiles every HIP/C++ source for gfx950 into rwkv.cpp_amd/lib/librwkv.so (hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", PKG_DIR, "-j8"]
    if force:
        args.append("-B")
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return LIB_PATH


class RWKVContext:
    def __init__(self, ptr) -> None:
        self.ptr = ptr


class RWKVSharedLibrary:
    """ctypes declarations of every symbol include/rwkv.h and include/rwkv_mi355x.h export."""

    def __init__(self, shared_library_path: str = LIB_PATH) -> None:
        if not os.path.isfile(shared_library_path):
            raise FileNotFoundError(f"{shared_library_path} not found: build it with __graft_entry__.build() (no CPU fallback exists)")
        self.library = L = ctypes.cdll.LoadLibrary(shared_library_path)
        c_ctx = ctypes.c_void_p

        L.rwkv_init_from_file.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32]
        L.rwkv_init_from_file.restype = c_ctx
        L.rwkv_clone_context.argtypes = [c_ctx, ctypes.c_uint32]
        L.rwkv_clone_context.restype = c_ctx
        L.rwkv_eval.argtypes = [c_ctx, ctypes.c_int32, P_FLOAT, P_FLOAT, P_FLOAT]
        L.rwkv_eval.restype = ctypes.c_bool
        L.rwkv_eval_sequence.argtypes = [c_ctx, P_UINT32, ctypes.c_size_t, P_FLOAT, P_FLOAT, P_FLOAT]
        L.rwkv_eval_sequence.restype = ctypes.c_bool
        L.rwkv_eval_sequence_in_chunks.argtypes = [c_ctx, P_UINT32, ctypes.c_size_t, ctypes.c_size_t, P_FLOAT, P_FLOAT, P_FLOAT]
        L.rwkv_eval_sequence_in_chunks.restype = ctypes.c_bool
        for name in ("rwkv_get_n_vocab", "rwkv_get_n_embed", "rwkv_get_n_layer", "rwkv_get_state_len", "rwkv_get_logits_len"):
            getattr(L, name).argtypes = [c_ctx]
            getattr(L, name).restype = ctypes.c_size_t
        for name in ("rwkv_get_state_buffer_element_count", "rwkv_get_logits_buffer_element_count"):
            getattr(L, name).argtypes = [c_ctx]
            getattr(L, name).restype = ctypes.c_uint32
        L.rwkv_init_state.argtypes = [c_ctx, P_FLOAT]
        L.rwkv_init_state.restype = None
        L.rwkv_free.argtypes = [c_ctx]
        L.rwkv_free.restype = None
        L.rwkv_quantize_model_file.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]
        L.rwkv_quantize_model_file.restype = ctypes.c_bool
        L.rwkv_get_system_info_string.argtypes = []
        L.rwkv_get_system_info_string.restype = ctypes.c_char_p
        L.rwkv_set_print_errors.argtypes = [c_ctx, ctypes.c_bool]
        L.rwkv_set_print_errors.restype = None
        L.rwkv_get_print_errors.argtypes = [c_ctx]
        L.rwkv_get_print_errors.restype = ctypes.c_bool
        L.rwkv_get_last_error.argtypes = [c_ctx]
        L.rwkv_get_last_error.restype = ctypes.c_int
        # extensions
        L.rwkv_mi_state_load.argtypes = [c_ctx, P_FLOAT]
        L.rwkv_mi_state_load.restype = ctypes.c_bool
        L.rwkv_mi_state_store.argtypes = [c_ctx, P_FLOAT]
        L.rwkv_mi_state_store.restype = ctypes.c_bool
        L.rwkv_mi_eval_resident.argtypes = [c_ctx, P_UINT32, ctypes.c_size_t, P_FLOAT]
        L.rwkv_mi_eval_resident.restype = ctypes.c_bool
        L.rwkv_mi_decode_greedy.argtypes = [c_ctx, ctypes.c_uint32, ctypes.c_size_t, P_UINT32, P_FLOAT]
        L.rwkv_mi_decode_greedy.restype = ctypes.c_bool
        L.rwkv_mi_profile_decode.argtypes = [c_ctx, ctypes.c_uint32, ctypes.c_size_t, ctypes.POINTER(ctypes.c_double)]
        L.rwkv_mi_profile_decode.restype = ctypes.c_bool
        L.rwkv_mi_profile_prefill.argtypes = [c_ctx, P_UINT32, ctypes.c_size_t, ctypes.POINTER(ctypes.c_double)]
        L.rwkv_mi_profile_prefill.restype = ctypes.c_bool
        L.rwkv_mi_bytes_per_token.argtypes = [c_ctx]
        L.rwkv_mi_bytes_per_token.restype = ctypes.c_uint64
        L.rwkv_mi_weight_bytes.argtypes = [c_ctx]
        L.rwkv_mi_weight_bytes.restype = ctypes.c_uint64
        L.rwkv_mi_prefill_flops.argtypes = [c_ctx, ctypes.c_size_t]
        L.rwkv_mi_prefill_flops.restype = ctypes.c_uint64
        L.rwkv_mi_get_arch.argtypes = [c_ctx, P_UINT32, P_UINT32, P_UINT32, P_UINT32]
        L.rwkv_mi_get_arch.restype = None
        L.rwkv_mi_init_stage.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
        L.rwkv_mi_init_stage.restype = c_ctx
        L.rwkv_mi_set_stream.argtypes = [c_ctx, ctypes.c_void_p]
        L.rwkv_mi_set_stream.restype = ctypes.c_bool
        L.rwkv_mi_handoff_len.argtypes = [c_ctx]
        L.rwkv_mi_handoff_len.restype = ctypes.c_size_t
        L.rwkv_mi_stage_step.argtypes = [c_ctx, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.rwkv_mi_stage_step.restype = ctypes.c_bool
        L.rwkv_mi_logits_store.argtypes = [c_ctx, P_FLOAT]
        L.rwkv_mi_logits_store.restype = ctypes.c_bool
        L.rwkv_mi_logits_device_ptr.argtypes = [c_ctx]
        L.rwkv_mi_logits_device_ptr.restype = ctypes.c_void_p
        L.rwkv_mi_set_graph_enabled.argtypes = [c_ctx, ctypes.c_bool]
        L.rwkv_mi_set_graph_enabled.restype = None
        L.rwkv_mi_decode_path.argtypes = [c_ctx]
        L.rwkv_mi_decode_path.restype = ctypes.c_int
        L.rwkv_mi_persist_kind.argtypes = [c_ctx]
        L.rwkv_mi_persist_kind.restype = ctypes.c_int
        if hasattr(L, "rwkv_mi_persist_info"):   # (absent from older A/B builds loaded through RWKV_LIB_DIR)
            L.rwkv_mi_persist_info.argtypes = [c_ctx]
            L.rwkv_mi_persist_info.restype = ctypes.c_char_p
        L.rwkv_mi_load_stats.argtypes = [c_ctx, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64)]
        L.rwkv_mi_load_stats.restype = None
        L.rwkv_mi_decode_healthy.argtypes = [c_ctx]
        L.rwkv_mi_decode_healthy.restype = ctypes.c_bool
        L.rwkv_mi_sample.argtypes = [c_ctx, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_uint64, P_UINT32]
        L.rwkv_mi_sample.restype = ctypes.c_bool
        L.rwkv_mi_decode_sample.argtypes = [c_ctx, ctypes.c_uint32, ctypes.c_size_t, ctypes.c_float, ctypes.c_float, ctypes.c_uint64, P_UINT32, P_FLOAT]
        L.rwkv_mi_decode_sample.restype = ctypes.c_bool
        L.rwkv_mi_decode_generation.argtypes = [c_ctx]
        L.rwkv_mi_decode_generation.restype = ctypes.c_uint32
        if hasattr(L, "rwkv_mi_test_set_tag"):   # (librwkv_testhooks.so only)
            L.rwkv_mi_test_set_tag.argtypes = [c_ctx, ctypes.c_uint32]
            L.rwkv_mi_test_set_tag.restype = ctypes.c_bool
        # the C++ decode loop of a pipeline (runner.cpp)
        L.rwkv_mi_decode_greedy_streams.argtypes = [ctypes.POINTER(c_ctx), ctypes.c_size_t, P_UINT32, ctypes.c_size_t, P_UINT32, P_FLOAT]
        L.rwkv_mi_decode_greedy_streams.restype = ctypes.c_bool
        L.rwkv_mi_comm_available.argtypes = []
        L.rwkv_mi_comm_available.restype = ctypes.c_bool
        L.rwkv_mi_comm_unique_id.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
        L.rwkv_mi_comm_unique_id.restype = ctypes.c_bool
        L.rwkv_mi_comm_init.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        L.rwkv_mi_comm_init.restype = ctypes.c_void_p
        if hasattr(L, "rwkv_mi_comm_init_ipc"):   # (absent from older A/B builds loaded through RWKV_LIB_DIR)
            L.rwkv_mi_comm_init_ipc.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
            L.rwkv_mi_comm_init_ipc.restype = ctypes.c_void_p
        L.rwkv_mi_comm_free.argtypes = [ctypes.c_void_p]
        L.rwkv_mi_comm_free.restype = None
        L.rwkv_mi_stage_run.argtypes = [ctypes.POINTER(c_ctx), ctypes.c_size_t, P_UINT32, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                        P_UINT32, P_FLOAT]
        L.rwkv_mi_stage_run.restype = ctypes.c_bool
        # batched decode (rwkv_mi_batch_*)
        c_batch = ctypes.c_void_p
        L.rwkv_mi_batch_create.argtypes = [c_ctx, ctypes.c_size_t]
        L.rwkv_mi_batch_create.restype = c_batch
        L.rwkv_mi_batch_free.argtypes = [c_batch]
        L.rwkv_mi_batch_free.restype = None
        L.rwkv_mi_batch_state_load.argtypes = [c_batch, ctypes.c_size_t, P_FLOAT]
        L.rwkv_mi_batch_state_load.restype = ctypes.c_bool
        L.rwkv_mi_batch_state_store.argtypes = [c_batch, ctypes.c_size_t, P_FLOAT]
        L.rwkv_mi_batch_state_store.restype = ctypes.c_bool
        L.rwkv_mi_batch_state_from_context.argtypes = [c_batch, ctypes.c_size_t, c_ctx]
        L.rwkv_mi_batch_state_from_context.restype = ctypes.c_bool
        L.rwkv_mi_batch_state_to_context.argtypes = [c_batch, ctypes.c_size_t, c_ctx]
        L.rwkv_mi_batch_state_to_context.restype = ctypes.c_bool
        L.rwkv_mi_batch_eval.argtypes = [c_batch, P_UINT32, P_UINT32, ctypes.c_size_t, P_FLOAT]
        L.rwkv_mi_batch_eval.restype = ctypes.c_bool
        L.rwkv_mi_batch_decode_greedy.argtypes = [c_batch, P_UINT32, P_UINT32, ctypes.c_size_t, ctypes.c_size_t, P_UINT32, P_FLOAT]
        L.rwkv_mi_batch_decode_greedy.restype = ctypes.c_bool
        L.rwkv_mi_batch_eval_sample.argtypes = [c_batch, P_UINT32, P_UINT32, ctypes.c_size_t, P_SAMPLE_PARAMS, P_UINT32, P_FLOAT]
        L.rwkv_mi_batch_eval_sample.restype = ctypes.c_bool
        L.rwkv_mi_batch_decode_sample.argtypes = [c_batch, P_UINT32, P_UINT32, ctypes.c_size_t, ctypes.c_size_t, P_SAMPLE_PARAMS, P_UINT32, P_FLOAT]
        L.rwkv_mi_batch_decode_sample.restype = ctypes.c_bool
        L.rwkv_mi_batch_rng_seek.argtypes = [c_batch, ctypes.c_size_t, ctypes.c_uint64]
        L.rwkv_mi_batch_rng_seek.restype = ctypes.c_bool
        L.rwkv_mi_batch_eval_ragged.argtypes = [c_batch, P_UINT32, P_UINT32, P_UINT32, ctypes.c_size_t, P_FLOAT]
        L.rwkv_mi_batch_eval_ragged.restype = ctypes.c_bool
        L.rwkv_mi_batch_eval_ragged_sample.argtypes = [c_batch, P_UINT32, P_UINT32, P_UINT32, ctypes.c_size_t, P_SAMPLE_PARAMS, P_UINT32, P_FLOAT]
        L.rwkv_mi_batch_eval_ragged_sample.restype = ctypes.c_bool
        # penalised sampling: per-slot / per-context occurrence and bias tables
        L.rwkv_mi_batch_counts_reset.argtypes = [c_batch, ctypes.c_size_t]
        L.rwkv_mi_batch_counts_add.argtypes = [c_batch, ctypes.c_size_t, P_UINT32, ctypes.c_size_t]
        L.rwkv_mi_batch_counts_store.argtypes = [c_batch, ctypes.c_size_t, P_UINT32]
        L.rwkv_mi_batch_logit_bias_set.argtypes = [c_batch, ctypes.c_size_t, P_UINT32, P_FLOAT, ctypes.c_size_t]
        L.rwkv_mi_batch_eval_sample_penalized.argtypes = [c_batch, P_UINT32, P_UINT32, ctypes.c_size_t, P_SAMPLE_PARAMS, P_PENALTY_PARAMS, P_UINT32, P_FLOAT]
        L.rwkv_mi_batch_eval_ragged_sample_penalized.argtypes = [c_batch, P_UINT32, P_UINT32, P_UINT32, ctypes.c_size_t, P_SAMPLE_PARAMS, P_PENALTY_PARAMS,
                                                                 P_UINT32, P_FLOAT]
        L.rwkv_mi_batch_decode_sample_penalized.argtypes = [c_batch, P_UINT32, P_UINT32, ctypes.c_size_t, ctypes.c_size_t, P_SAMPLE_PARAMS, P_PENALTY_PARAMS,
                                                            P_UINT32, P_FLOAT]
        L.rwkv_mi_counts_reset.argtypes = [c_ctx]
        L.rwkv_mi_counts_add.argtypes = [c_ctx, P_UINT32, ctypes.c_size_t]
        L.rwkv_mi_counts_store.argtypes = [c_ctx, P_UINT32]
        L.rwkv_mi_logit_bias_set.argtypes = [c_ctx, P_UINT32, P_FLOAT, ctypes.c_size_t]
        L.rwkv_mi_rng_seek.argtypes = [c_ctx, ctypes.c_uint64]
        L.rwkv_mi_sample_penalized.argtypes = [c_ctx, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_uint64, ctypes.c_float, ctypes.c_float,
                                               ctypes.c_uint32, P_UINT32]
        L.rwkv_mi_decode_sample_penalized.argtypes = [c_ctx, ctypes.c_uint32, ctypes.c_size_t, ctypes.c_float, ctypes.c_float, ctypes.c_uint64,
                                                      ctypes.c_float, ctypes.c_float, P_UINT32, P_FLOAT]
        for name in PENALTY_SYMBOLS:
            getattr(L, name).restype = ctypes.c_bool
        # scoring: log-prob / argmax at every position
        if hasattr(L, "rwkv_mi_score_resident"):   # (absent from older A/B builds loaded through RWKV_LIB_DIR)
            L.rwkv_mi_score_resident.argtypes = [c_ctx, P_UINT32, ctypes.c_size_t, P_UINT32, P_FLOAT, P_UINT32, P_FLOAT]
            L.rwkv_mi_batch_score_ragged.argtypes = [c_batch, P_UINT32, P_UINT32, P_UINT32, P_UINT32, ctypes.c_size_t, P_FLOAT, P_UINT32]
            for name in SCORE_SYMBOLS:
                getattr(L, name).restype = ctypes.c_bool
        # device loops in which every row ends by itself: stop sequences and per-row budgets
        if hasattr(L, "rwkv_mi_batch_decode_until"):   # (absent from older A/B builds loaded through RWKV_LIB_DIR)
            L.rwkv_mi_batch_decode_until.argtypes = [c_batch, P_UINT32, P_UINT32, ctypes.c_size_t, P_SAMPLE_PARAMS, P_PENALTY_PARAMS, P_STOP_PARAMS,
                                                     P_UINT32, P_UINT32, ctypes.c_size_t, P_UINT32, P_UINT32, P_UINT32, P_FLOAT]
            L.rwkv_mi_batch_decode_until.restype = ctypes.c_bool
            L.rwkv_mi_batch_last_loop_passes.argtypes = [c_batch]
            L.rwkv_mi_batch_last_loop_passes.restype = ctypes.c_size_t
        # continuous batching: a queue of requests behind the lanes of one device loop
        if hasattr(L, "rwkv_mi_batch_serve"):   # (absent from older A/B builds loaded through RWKV_LIB_DIR)
            L.rwkv_mi_batch_serve.argtypes = [c_batch, P_UINT32, ctypes.c_size_t, ctypes.c_int, P_SERVE_REQUEST, ctypes.c_size_t, P_UINT32, P_UINT32, P_UINT32,
                                              ctypes.c_size_t, P_UINT32, P_UINT32, P_UINT32, P_UINT32, P_UINT32, P_UINT32, P_FLOAT]
            L.rwkv_mi_batch_serve.restype = ctypes.c_bool
        # ... whose requests carry a guide and a bias, and which fills the report
        if hasattr(L, "rwkv_mi_batch_serve_ex"):   # (absent from older A/B builds loaded through RWKV_LIB_DIR)
            L.rwkv_mi_batch_serve_ex.argtypes = list(L.rwkv_mi_batch_serve.argtypes) + [P_SERVE_EXTRA, P_UINT32, P_UINT32]
            L.rwkv_mi_batch_serve_ex.restype = ctypes.c_bool
        # serve sessions: the same loop kept open between host calls
        if hasattr(L, "rwkv_mi_batch_serve_open"):   # (absent from older A/B builds loaded through RWKV_LIB_DIR)
            c_session = ctypes.c_void_p
            P_SIZE_T = ctypes.POINTER(ctypes.c_size_t)
            L.rwkv_mi_batch_serve_open.argtypes = [c_batch, P_UINT32, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ServeLimits)]
            L.rwkv_mi_batch_serve_open.restype = c_session
            L.rwkv_mi_batch_serve_submit.argtypes = [c_session, P_SERVE_REQUEST, P_UINT32, P_UINT32, P_UINT32, P_SERVE_EXTRA, P_UINT32]
            L.rwkv_mi_batch_serve_cancel.argtypes = [c_session, ctypes.c_uint32]
            L.rwkv_mi_batch_serve_poll.argtypes = [c_session, ctypes.c_uint32, ctypes.POINTER(ServeEvent), ctypes.c_size_t, P_UINT32, ctypes.c_size_t, P_SIZE_T, P_SIZE_T]
            L.rwkv_mi_batch_serve_stats.argtypes = [c_session, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), P_UINT32, P_UINT32]
            L.rwkv_mi_batch_serve_close.argtypes = [c_session, P_UINT32]
            for name in SESSION_SYMBOLS[1:]:
                getattr(L, name).restype = ctypes.c_bool
        # the report: log-probs and top-N alternatives of every emitted token
        if hasattr(L, "rwkv_mi_batch_set_logprobs"):   # (absent from older A/B builds loaded through RWKV_LIB_DIR)
            P_SIZE = ctypes.POINTER(ctypes.c_size_t)
            for handle, prefix in ((c_batch, "rwkv_mi_batch_"), (c_ctx, "rwkv_mi_")):
                getattr(L, prefix + "set_logprobs").argtypes = [handle, ctypes.c_bool, ctypes.c_uint32]
                getattr(L, prefix + "logprobs_shape").argtypes = [handle, P_SIZE, P_SIZE, P_UINT32]
                getattr(L, prefix + "logprobs_store").argtypes = [handle, ctypes.c_size_t, P_FLOAT, P_UINT32, P_FLOAT]
            for name in LOGPROBS_SYMBOLS:
                getattr(L, name).restype = ctypes.c_bool
        # slot-to-slot copy and beam search
        if hasattr(L, "rwkv_mi_batch_decode_beam"):   # (absent from older A/B builds loaded through RWKV_LIB_DIR)
            L.rwkv_mi_batch_state_copy.argtypes = [c_batch, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32]
            L.rwkv_mi_batch_decode_beam.argtypes = [c_batch, P_UINT32, P_UINT32, ctypes.c_size_t, ctypes.POINTER(BeamParams), ctypes.c_size_t, P_UINT32, P_UINT32,
                                                    ctypes.POINTER(ctypes.c_double), P_FLOAT, P_FLOAT]
            for name in BEAM_SYMBOLS:
                getattr(L, name).restype = ctypes.c_bool
        # guided decoding: token automata that mask the device sampler per slot
        if hasattr(L, "rwkv_mi_batch_guide_create"):   # (absent from older A/B builds loaded through RWKV_LIB_DIR)
            L.rwkv_mi_batch_guide_create.argtypes = [c_batch, ctypes.c_uint32, P_UINT32, P_UINT32, P_UINT32, P_UINT32]
            L.rwkv_mi_batch_guide_free.argtypes = [c_batch, ctypes.c_uint32]
            L.rwkv_mi_batch_guide_attach.argtypes = [c_batch, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32]
            L.rwkv_mi_batch_guide_state.argtypes = [c_batch, ctypes.c_size_t, P_UINT32, P_UINT32, P_UINT32]
            for name in GUIDE_SYMBOLS:
                getattr(L, name).restype = ctypes.c_bool
        # speculative decoding: verify a draft in one pass, keep its prefix
        if hasattr(L, "rwkv_mi_batch_eval_draft"):   # (absent from older A/B builds loaded through RWKV_LIB_DIR)
            L.rwkv_mi_batch_eval_draft.argtypes = [c_batch, P_UINT32, P_UINT32, P_UINT32, ctypes.c_size_t, P_SAMPLE_PARAMS, P_PENALTY_PARAMS, ctypes.c_size_t,
                                                   P_UINT32, P_UINT32, P_FLOAT]
            for name in DRAFT_SYMBOLS:
                getattr(L, name).restype = ctypes.c_bool
        # top-k and min-p: per-sequence truncation settings of the device sampler
        if hasattr(L, "rwkv_mi_batch_truncation_set"):   # (absent from older A/B builds loaded through RWKV_LIB_DIR)
            L.rwkv_mi_batch_truncation_set.argtypes = [c_batch, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_float]
            L.rwkv_mi_batch_truncation_get.argtypes = [c_batch, ctypes.c_size_t, P_UINT32, P_FLOAT]
            L.rwkv_mi_truncation_set.argtypes = [c_ctx, ctypes.c_uint32, ctypes.c_float]
            L.rwkv_mi_truncation_get.argtypes = [c_ctx, P_UINT32, P_FLOAT]
            for name in TRUNCATION_SYMBOLS:
                getattr(L, name).restype = ctypes.c_bool
        # penalty decay and repetition penalty: per-sequence repetition settings of the penalised draws
        if hasattr(L, "rwkv_mi_batch_repetition_set"):   # (absent from older A/B builds loaded through RWKV_LIB_DIR)
            L.rwkv_mi_batch_repetition_set.argtypes = [c_batch, ctypes.c_size_t, ctypes.c_float, ctypes.c_float]
            L.rwkv_mi_batch_repetition_get.argtypes = [c_batch, ctypes.c_size_t, P_FLOAT, P_FLOAT]
            L.rwkv_mi_batch_counts_store_f32.argtypes = [c_batch, ctypes.c_size_t, P_FLOAT]
            L.rwkv_mi_repetition_set.argtypes = [c_ctx, ctypes.c_float, ctypes.c_float]
            L.rwkv_mi_repetition_get.argtypes = [c_ctx, P_FLOAT, P_FLOAT]
            L.rwkv_mi_counts_store_f32.argtypes = [c_ctx, P_FLOAT]
            for name in REPETITION_SYMBOLS:
                getattr(L, name).restype = ctypes.c_bool
        if hasattr(L, "rwkv_mi_test_decay_rows"):   # (librwkv_testhooks_decay.so only)
            L.rwkv_mi_test_decay_rows.argtypes = [P_FLOAT, ctypes.c_int64, ctypes.c_int64, P_SAMPLE_PARAMS, P_PENALTY_PARAMS, ctypes.POINTER(RepParams), P_UINT32,
                                                  P_FLOAT, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int, P_UINT32]
            L.rwkv_mi_test_decay_rows.restype = ctypes.c_bool
            L.rwkv_mi_test_decay_counts_add.argtypes = [P_FLOAT, ctypes.c_int64, P_UINT32, ctypes.c_int64, ctypes.c_float]
            L.rwkv_mi_test_decay_counts_add.restype = ctypes.c_bool
        if hasattr(L, "rwkv_mi_test_cut_rows"):   # (librwkv_testhooks_cut.so only)
            L.rwkv_mi_test_cut_rows.argtypes = [P_FLOAT, ctypes.c_int64, ctypes.c_int64, P_SAMPLE_PARAMS, ctypes.POINTER(CutParams), ctypes.POINTER(ctypes.c_uint64),
                                                ctypes.c_int, P_UINT32, P_FLOAT]
            L.rwkv_mi_test_cut_rows.restype = ctypes.c_bool
        if hasattr(L, "rwkv_mi_test_guided_rows"):   # (librwkv_testhooks_guide.so only)
            L.rwkv_mi_test_guided_rows.argtypes = [P_FLOAT, ctypes.c_int64, ctypes.c_int64, ctypes.c_uint32, P_UINT32, P_UINT32, P_UINT32, P_UINT32, P_UINT32, P_UINT32,
                                                   P_SAMPLE_PARAMS, P_PENALTY_PARAMS, P_UINT32, P_FLOAT, ctypes.POINTER(ctypes.c_uint64), P_UINT32, P_UINT32, P_UINT32]
            L.rwkv_mi_test_guided_rows.restype = ctypes.c_bool
        if hasattr(L, "rwkv_test_beam_step"):   # (librwkv_testhooks_sample.so only)
            L.rwkv_test_beam_step.argtypes = [P_FLOAT, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_double), P_UINT32, ctypes.c_uint32, P_UINT32,
                                              ctypes.c_uint32, P_UINT32, P_UINT32, P_FLOAT, ctypes.POINTER(ctypes.c_double), P_UINT32]
            L.rwkv_test_beam_step.restype = ctypes.c_bool
        if hasattr(L, "rwkv_test_logprob_rows"):   # (librwkv_testhooks_sample.so only)
            L.rwkv_test_logprob_rows.argtypes = [P_FLOAT, ctypes.c_int64, ctypes.c_int64, P_UINT32, ctypes.c_uint32, P_FLOAT, P_UINT32, P_FLOAT]
            L.rwkv_test_logprob_rows.restype = ctypes.c_bool
        if hasattr(L, "rwkv_test_score_rows"):   # (librwkv_testhooks_sample.so only)
            L.rwkv_test_score_rows.argtypes = [P_FLOAT, ctypes.c_int64, ctypes.c_int64, P_UINT32, P_FLOAT, P_UINT32]
            L.rwkv_test_score_rows.restype = ctypes.c_bool
        if hasattr(L, "rwkv_mi_test_sample_rows"):   # (librwkv_testhooks_sample.so only)
            L.rwkv_mi_test_sample_rows.argtypes = [P_FLOAT, ctypes.c_int64, ctypes.c_int64, P_SAMPLE_PARAMS, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int, P_UINT32]
            L.rwkv_mi_test_sample_rows.restype = ctypes.c_bool

    # --- rwkv.h ---------------------------------------------------------------------------------------------

    def rwkv_init_from_file(self, model_file_path: str, thread_count: int, offload_layers: int) -> RWKVContext:
        ptr = self.library.rwkv_init_from_file(model_file_path.encode("utf-8"), ctypes.c_uint32(thread_count), ctypes.c_uint32(offload_layers))
        if not ptr:
            raise ValueError("rwkv_init_from_file failed, check stderr")
        return RWKVContext(ptr)

    def rwkv_clone_context(self, ctx: RWKVContext, thread_count: int) -> RWKVContext:
        ptr = self.library.rwkv_clone_context(ctx.ptr, ctypes.c_uint32(thread_count))
        if not ptr:
            raise ValueError("rwkv_clone_context failed, check stderr")
        return RWKVContext(ptr)

    def rwkv_eval(self, ctx: RWKVContext, token: int, state_in_address: Optional[int], state_out_address: int, logits_out_address: int) -> None:
        if not self.library.rwkv_eval(ctx.ptr, ctypes.c_int32(token), ctypes.cast(state_in_address or 0, P_FLOAT),
                                      ctypes.cast(state_out_address or 0, P_FLOAT), ctypes.cast(logits_out_address or 0, P_FLOAT)):
            raise ValueError("rwkv_eval failed, check stderr")

    def rwkv_eval_sequence(self, ctx: RWKVContext, tokens: List[int], state_in_address: Optional[int], state_out_address: int, logits_out_address: int) -> None:
        arr = (ctypes.c_uint32 * len(tokens))(*tokens)
        if not self.library.rwkv_eval_sequence(ctx.ptr, arr, ctypes.c_size_t(len(tokens)), ctypes.cast(state_in_address or 0, P_FLOAT),
                                               ctypes.cast(state_out_address or 0, P_FLOAT), ctypes.cast(logits_out_address or 0, P_FLOAT)):
            raise ValueError("rwkv_eval_sequence failed, check stderr")

    def rwkv_eval_sequence_in_chunks(self, ctx: RWKVContext, tokens: List[int], chunk_size: int, state_in_address: Optional[int],
                                     state_out_address: int, logits_out_address: int) -> None:
        arr = (ctypes.c_uint32 * len(tokens))(*tokens)
        if not self.library.rwkv_eval_sequence_in_chunks(ctx.ptr, arr, ctypes.c_size_t(len(tokens)), ctypes.c_size_t(chunk_size),
                                                         ctypes.cast(state_in_address or 0, P_FLOAT), ctypes.cast(state_out_address or 0, P_FLOAT),
                                                         ctypes.cast(logits_out_address or 0, P_FLOAT)):
            raise ValueError("rwkv_eval_sequence_in_chunks failed, check stderr")

    def rwkv_get_n_vocab(self, ctx: RWKVContext) -> int:
        return self.library.rwkv_get_n_vocab(ctx.ptr)

    def rwkv_get_n_embed(self, ctx: RWKVContext) -> int:
        return self.library.rwkv_get_n_embed(ctx.ptr)

    def rwkv_get_n_layer(self, ctx: RWKVContext) -> int:
        return self.library.rwkv_get_n_layer(ctx.ptr)

    def rwkv_get_state_buffer_element_count(self, ctx: RWKVContext) -> int:
        return self.library.rwkv_get_state_buffer_element_count(ctx.ptr)

    def rwkv_get_logits_buffer_element_count(self, ctx: RWKVContext) -> int:
        return self.library.rwkv_get_logits_buffer_element_count(ctx.ptr)

    def rwkv_init_state(self, ctx: RWKVContext, state_address: int) -> None:
        self.library.rwkv_init_state(ctx.ptr, ctypes.cast(state_address, P_FLOAT))

    def rwkv_free(self, ctx: RWKVContext) -> None:
        self.library.rwkv_free(ctx.ptr)
        ctx.ptr = ctypes.cast(0, ctypes.c_void_p)

    def rwkv_quantize_model_file(self, model_file_path_in: str, model_file_path_out: str, format_name: str) -> None:
        if format_name not in QUANTIZED_FORMAT_NAMES:
            raise ValueError(f"Unknown format name {format_name}, use one of {QUANTIZED_FORMAT_NAMES}")
        if not self.library.rwkv_quantize_model_file(model_file_path_in.encode("utf-8"), model_file_path_out.encode("utf-8"), format_name.encode("utf-8")):
            raise ValueError("rwkv_quantize_model_file failed, check stderr")

    def rwkv_get_system_info_string(self) -> str:
        return self.library.rwkv_get_system_info_string().decode("utf-8")

    def rwkv_set_print_errors(self, ctx: Optional[RWKVContext], print_errors: bool) -> None:
        self.library.rwkv_set_print_errors(ctx.ptr if ctx else None, print_errors)

    def rwkv_get_last_error(self, ctx: Optional[RWKVContext]) -> int:
        return int(self.library.rwkv_get_last_error(ctx.ptr if ctx else None))


def load_rwkv_shared_library() -> RWKVSharedLibrary:
    return RWKVSharedLibrary(LIB_PATH)


def _report(L, prefix: str, handle):
    """The last report of a batch or a context (rwkv_mi_*logprobs_shape / _store) as (chosen [rows][steps] float32, top_ids [rows][steps][top_n]
    uint32, top_logprobs [rows][steps][top_n] float32); None when the library refuses (no report yet)."""
    rows, steps, top_n = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_uint32(0)
    if not getattr(L, prefix + "logprobs_shape")(handle, ctypes.byref(rows), ctypes.byref(steps), ctypes.byref(top_n)):
        return None
    r, s, k = int(rows.value), int(steps.value), int(top_n.value)
    chosen = np.empty((r, s), dtype=np.float32)
    ids = np.empty((r, s, k), dtype=np.uint32)
    vals = np.empty((r, s, k), dtype=np.float32)
    if not getattr(L, prefix + "logprobs_store")(handle, s, ctypes.cast(_ptr(chosen), P_FLOAT), ctypes.cast(_ptr(ids) if k else 0, P_UINT32),
                                                 ctypes.cast(_ptr(vals) if k else 0, P_FLOAT)):
        return None
    return chosen, ids, vals


def _ptr(a: Optional[np.ndarray]) -> int:
    return 0 if a is None else a.ctypes.data


class RWKVModel:
    """numpy flavour of the reference's RWKVModel (python/rwkv_cpp/rwkv_cpp_model.py:22-364)."""

    def __init__(self, shared_library: RWKVSharedLibrary, model_path: str, thread_count: int = 1, gpu_layer_count: int = 0, **kwargs) -> None:
        if "gpu_layers_count" in kwargs:
            gpu_layer_count = kwargs["gpu_layers_count"]
        if not os.path.isfile(model_path):
            raise ValueError(f"{model_path} is not a file")
        if thread_count <= 0:
            raise ValueError("Thread count must be > 0")
        self._library = shared_library
        self._ctx = shared_library.rwkv_init_from_file(model_path, thread_count, gpu_layer_count)
        self._state_buffer_element_count = shared_library.rwkv_get_state_buffer_element_count(self._ctx)
        self._logits_buffer_element_count = shared_library.rwkv_get_logits_buffer_element_count(self._ctx)
        self._valid = True

    @property
    def n_vocab(self) -> int:
        return self._library.rwkv_get_n_vocab(self._ctx)

    @property
    def n_embed(self) -> int:
        return self._library.rwkv_get_n_embed(self._ctx)

    @property
    def n_layer(self) -> int:
        return self._library.rwkv_get_n_layer(self._ctx)

    @property
    def state_len(self) -> int:
        return self._state_buffer_element_count

    def arch(self) -> Tuple[int, int, int, int]:
        v = [ctypes.c_uint32() for _ in range(4)]
        self._library.library.rwkv_mi_get_arch(self._ctx.ptr, *[ctypes.byref(x) for x in v])
        return tuple(int(x.value) for x in v)

    def _check(self, a: Optional[np.ndarray], name: str, size: int) -> None:
        if a is None:
            return
        if a.dtype != np.float32 or not a.flags["C_CONTIGUOUS"] or a.shape != (size,):
            raise ValueError(f"{name} must be a contiguous float32 array of shape ({size},)")

    def _outputs(self, state_out, logits_out):
        self._check(state_out, "state_out", self._state_buffer_element_count)
        self._check(logits_out, "logits_out", self._logits_buffer_element_count)
        if state_out is None:
            state_out = np.zeros(self._state_buffer_element_count, dtype=np.float32)
        if logits_out is None:
            logits_out = np.zeros(self._logits_buffer_element_count, dtype=np.float32)
        return state_out, logits_out

    def init_state(self) -> np.ndarray:
        s = np.empty(self._state_buffer_element_count, dtype=np.float32)
        self._library.rwkv_init_state(self._ctx, s.ctypes.data)
        return s

    def eval(self, token: int, state_in: Optional[np.ndarray], state_out: Optional[np.ndarray] = None,
             logits_out: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
        if not self._valid:
            raise ValueError("Model was freed")
        self._check(state_in, "state_in", self._state_buffer_element_count)
        state_out, logits_out = self._outputs(state_out, logits_out)
        self._library.rwkv_eval(self._ctx, token, _ptr(state_in), _ptr(state_out), _ptr(logits_out))
        return logits_out, state_out

    def eval_sequence(self, tokens: List[int], state_in: Optional[np.ndarray], state_out: Optional[np.ndarray] = None,
                      logits_out: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
        if not self._valid:
            raise ValueError("Model was freed")
        self._check(state_in, "state_in", self._state_buffer_element_count)
        state_out, logits_out = self._outputs(state_out, logits_out)
        self._library.rwkv_eval_sequence(self._ctx, list(tokens), _ptr(state_in), _ptr(state_out), _ptr(logits_out))
        return logits_out, state_out

    def eval_sequence_in_chunks(self, tokens: List[int], state_in: Optional[np.ndarray], state_out: Optional[np.ndarray] = None,
                                logits_out: Optional[np.ndarray] = None, chunk_size: int = 16) -> Tuple[np.ndarray, np.ndarray]:
        if not self._valid:
            raise ValueError("Model was freed")
        self._check(state_in, "state_in", self._state_buffer_element_count)
        state_out, logits_out = self._outputs(state_out, logits_out)
        self._library.rwkv_eval_sequence_in_chunks(self._ctx, list(tokens), chunk_size, _ptr(state_in), _ptr(state_out), _ptr(logits_out))
        return logits_out, state_out

    # --- rwkv_mi_* extensions: state resident in HBM ------------------------------------------------------

    def state_load(self, state_in: Optional[np.ndarray]) -> None:
        self._check(state_in, "state_in", self._state_buffer_element_count)
        if not self._library.library.rwkv_mi_state_load(self._ctx.ptr, ctypes.cast(_ptr(state_in), P_FLOAT)):
            raise ValueError("rwkv_mi_state_load failed")

    def state_store(self) -> np.ndarray:
        s = np.empty(self._state_buffer_element_count, dtype=np.float32)
        if not self._library.library.rwkv_mi_state_store(self._ctx.ptr, ctypes.cast(s.ctypes.data, P_FLOAT)):
            raise ValueError("rwkv_mi_state_store failed")
        return s

    def logits_store(self) -> np.ndarray:
        """Logits of the last step that produced any (device -> host; synchronises the context's stream)."""
        lg = np.empty(self._logits_buffer_element_count, dtype=np.float32)
        if not self._library.library.rwkv_mi_logits_store(self._ctx.ptr, ctypes.cast(_ptr(lg), P_FLOAT)):
            raise ValueError("rwkv_mi_logits_store failed")
        return lg

    def eval_resident(self, tokens: List[int], want_logits: bool = True) -> Optional[np.ndarray]:
        arr = (ctypes.c_uint32 * len(tokens))(*tokens)
        logits = np.empty(self._logits_buffer_element_count, dtype=np.float32) if want_logits else None
        if not self._library.library.rwkv_mi_eval_resident(self._ctx.ptr, arr, len(tokens), ctypes.cast(_ptr(logits), P_FLOAT)):
            raise ValueError("rwkv_mi_eval_resident failed")
        return logits

    def score_resident(self, tokens: List[int], targets: Optional[List[int]] = None, want_argmax: bool = True, want_logits: bool = False):
        """Feeds `tokens` from the resident state (as eval_resident) and reports the prediction after EACH of them, from one pass:
        (logprobs, argmax, logits). logprobs[t] = log P(targets[t] | tokens[..t]) as float32 (0 where targets[t] is NO_TARGET; None without
        targets), argmax[t] the most likely next token (None unless want_argmax), logits [n][n_vocab] (None unless want_logits)."""
        t = _u32(tokens).reshape(-1)
        tg = None if targets is None else _u32(targets).reshape(-1)
        if tg is not None and tg.size != t.size:
            raise ValueError("tokens and targets differ in length")
        logprobs = np.empty(t.size, dtype=np.float32) if tg is not None else None
        argmax = np.empty(t.size, dtype=np.uint32) if want_argmax else None
        logits = np.empty((t.size, self._logits_buffer_element_count), dtype=np.float32) if want_logits else None
        self._mi("rwkv_mi_score_resident", t.ctypes.data_as(P_UINT32), t.size, ctypes.cast(_ptr(tg), P_UINT32), ctypes.cast(_ptr(logprobs), P_FLOAT),
                 ctypes.cast(_ptr(argmax), P_UINT32), ctypes.cast(_ptr(logits), P_FLOAT))
        return logprobs, argmax, logits

    def perplexity(self, tokens: List[int], ignore_first_n_tokens: int = 0) -> Tuple[float, float]:
        """(mean loss, exp(mean loss)) of `tokens` from the resident state -- the loop of the reference's measure_pexplexity.py:71-85 in one
        pass: tokens[:-1] are fed, position i is scored against tokens[i + 1] and counts when ignore_first_n_tokens == 0 or
        i + 1 >= ignore_first_n_tokens; the mean is taken in float64 on the host."""
        t = _u32(tokens).reshape(-1)
        if t.size < 2:
            raise ValueError("perplexity needs at least two tokens")
        logprobs, _, _ = self.score_resident(t[:-1], t[1:], want_argmax=False)
        i = np.arange(t.size - 1)
        counted = (i + 1 >= ignore_first_n_tokens) if ignore_first_n_tokens else np.ones(t.size - 1, dtype=bool)
        if not counted.any():
            raise ValueError("ignore_first_n_tokens leaves no position to count")
        loss = float(-(logprobs[counted].astype(np.float64)).sum() / int(counted.sum()))
        return loss, float(np.exp(loss))

    def decode_greedy(self, first_token: int, n_tokens: int) -> Tuple[np.ndarray, float]:
        out = np.empty(n_tokens, dtype=np.uint32)
        ms = ctypes.c_float(0.0)
        if not self._library.library.rwkv_mi_decode_greedy(self._ctx.ptr, first_token, n_tokens, ctypes.cast(out.ctypes.data, P_UINT32), ctypes.byref(ms)):
            raise ValueError("rwkv_mi_decode_greedy failed")
        return out, float(ms.value)

    @staticmethod
    def decode_greedy_streams(models: List["RWKVModel"], first_tokens: List[int], n_tokens: int) -> Tuple[np.ndarray, float]:
        """Greedy decode of several resident-state contexts (a model and its clones; RWKV_MI_DEVICES chains included) interleaved by the
        library's C++ loop: tokens [n_streams][n_tokens], wall milliseconds."""
        n = len(models)
        L = models[0]._library.library
        arr = (ctypes.c_void_p * n)(*[m._ctx.ptr for m in models])
        first = (ctypes.c_uint32 * n)(*first_tokens)
        out = np.empty((n, n_tokens), dtype=np.uint32)
        ms = ctypes.c_float(0.0)
        if not L.rwkv_mi_decode_greedy_streams(arr, n, first, n_tokens, ctypes.cast(out.ctypes.data, P_UINT32), ctypes.byref(ms)):
            raise ValueError("rwkv_mi_decode_greedy_streams failed")
        return out, float(ms.value)

    def sample(self, temperature: float = 1.0, top_p: float = 0.8, u: float = -1.0, seed: int = 0) -> int:
        """Samples from the logits of the last evaluation on the device (mirror of the reference's sampling.sample_logits)."""
        tok = ctypes.c_uint32(0)
        if not self._library.library.rwkv_mi_sample(self._ctx.ptr, temperature, top_p, u, seed, ctypes.byref(tok)):
            raise ValueError("rwkv_mi_sample failed")
        return int(tok.value)

    def decode_sample(self, first_token: int, n_tokens: int, temperature: float = 1.0, top_p: float = 0.8, seed: int = 0) -> Tuple[np.ndarray, float]:
        out = np.empty(n_tokens, dtype=np.uint32)
        ms = ctypes.c_float(0.0)
        if not self._library.library.rwkv_mi_decode_sample(self._ctx.ptr, first_token, n_tokens, temperature, top_p, seed,
                                                           ctypes.cast(out.ctypes.data, P_UINT32), ctypes.byref(ms)):
            raise ValueError("rwkv_mi_decode_sample failed")
        return out, float(ms.value)

    # --- penalised sampling: the context's occurrence table and bias table (include/rwkv_mi355x.h) ---

    def _mi(self, name: str, *args) -> None:
        if not getattr(self._library.library, name)(self._ctx.ptr, *args):
            self.last_error = self._library.rwkv_get_last_error(self._ctx)
            raise ValueError(f"{name} failed (error flags {self.last_error})")

    def counts_reset(self) -> None:
        self._mi("rwkv_mi_counts_reset")

    def counts_add(self, tokens: List[int]) -> None:
        """count[t] += 1 for every t of `tokens` (resuming a recorded response)."""
        t = _u32(tokens).reshape(-1)
        self._mi("rwkv_mi_counts_add", t.ctypes.data_as(P_UINT32), t.size)

    def counts(self) -> np.ndarray:
        """The context's occurrence table, uint32 [n_vocab]."""
        out = np.empty(self.n_vocab, dtype=np.uint32)
        self._mi("rwkv_mi_counts_store", out.ctypes.data_as(P_UINT32))
        return out

    def set_logit_bias(self, bias: dict) -> None:
        """Replaces the context's logit bias by {token id: value}; an empty dict clears it (sampling.py's logit_bias)."""
        ids, values = _bias_arrays(bias)
        self._mi("rwkv_mi_logit_bias_set", ids.ctypes.data_as(P_UINT32), values.ctypes.data_as(P_FLOAT), ids.size)

    def rng_seek(self, counter: int) -> None:
        """Sets the context's draw counter (0 for a new request)."""
        self._mi("rwkv_mi_rng_seek", counter)

    def set_truncation(self, top_k: int = 0, min_p: float = 0.0) -> None:
        """The context's truncation setting, read by every draw from now on: top_k (0: off) masks all but the top_k largest values the draw
        reads to -inf before the softmax; min_p (0: off) cuts the probabilities below min_p * the largest, beside top-p. (0, 0) clears."""
        self._mi("rwkv_mi_truncation_set", int(top_k), float(min_p))

    def truncation(self) -> Tuple[int, float]:
        """The context's truncation setting (top_k, min_p); (0, 0.0) is none."""
        k, p = ctypes.c_uint32(0), ctypes.c_float(0.0)
        self._mi("rwkv_mi_truncation_get", ctypes.byref(k), ctypes.byref(p))
        return int(k.value), float(p.value)

    def set_repetition(self, decay: float = 1.0, repetition: float = 1.0) -> None:
        """The context's repetition setting, read by every PENALISED draw from now on: repetition (1: off) divides the positive and multiplies
        the other logits of the tokens that have occurred; decay (1: off) makes the occurrence table a float table that every recorded draw
        multiplies by decay before it counts its token. (1, 1) clears. A set that turns decay on or off zeroes the table."""
        self._mi("rwkv_mi_repetition_set", float(decay), float(repetition))

    def repetition(self) -> Tuple[float, float]:
        """The context's repetition setting (decay, repetition); (1.0, 1.0) is none."""
        d, r = ctypes.c_float(0.0), ctypes.c_float(0.0)
        self._mi("rwkv_mi_repetition_get", ctypes.byref(d), ctypes.byref(r))
        return float(d.value), float(r.value)

    def counts_f32(self) -> np.ndarray:
        """The context's occurrence table as float32 [n_vocab]: the decayed occurrences of a decaying context, the counts of any other."""
        out = np.empty(self.n_vocab, dtype=np.float32)
        self._mi("rwkv_mi_counts_store_f32", out.ctypes.data_as(P_FLOAT))
        return out

    def sample_penalized(self, temperature: float = 1.0, top_p: float = 0.8, u: float = -1.0, seed: int = 0, presence: float = 0.2,
                         frequency: float = 0.2, record: bool = True) -> int:
        """sample() on the logits less presence + count * frequency, plus the bias; the chosen token is counted when `record`."""
        tok = ctypes.c_uint32(0)
        self._mi("rwkv_mi_sample_penalized", temperature, top_p, u, seed, presence, frequency, 1 if record else 0, ctypes.byref(tok))
        return int(tok.value)

    def decode_sample_penalized(self, first_token: int, n_tokens: int, temperature: float = 1.0, top_p: float = 0.8, seed: int = 0,
                                presence: float = 0.2, frequency: float = 0.2) -> Tuple[np.ndarray, float]:
        """decode_sample() with the penalised draw, every step recorded. It continues: call counts_reset() and rng_seek(0) for a new request."""
        out = np.empty(n_tokens, dtype=np.uint32)
        ms = ctypes.c_float(0.0)
        self._mi("rwkv_mi_decode_sample_penalized", first_token, n_tokens, temperature, top_p, seed, presence, frequency,
                 ctypes.cast(out.ctypes.data, P_UINT32), ctypes.byref(ms))
        return out, float(ms.value)

    # --- the report: log-probs and top-N alternatives of every emitted token (include/rwkv_mi355x.h) ---

    def set_logprobs(self, top_n: int = 0, enabled: bool = True) -> None:
        """Turns the report of the context's draws (sample, sample_penalized, decode_sample, decode_sample_penalized) on, with top_n <= TOP_MAX
        alternatives per token, or off. decode_greedy is not covered: greedy with a report is decode_sample at temperature 0."""
        self._mi("rwkv_mi_set_logprobs", bool(enabled), int(top_n))

    def logprobs(self):
        """The report of the last draw or loop: (chosen [1][steps], top_ids [1][steps][top_n], top_logprobs [1][steps][top_n]), taken from the
        model's logits (not the penalised ones); chosen equals score_resident's log-prob of the emitted token, bit for bit."""
        out = _report(self._library.library, "rwkv_mi_", self._ctx.ptr)
        if out is None:
            self.last_error = self._library.rwkv_get_last_error(self._ctx)
            raise ValueError(f"rwkv_mi_logprobs_store failed (error flags {self.last_error})")
        return out

    def profile_decode(self, first_token: int, n_tokens: int) -> dict:
        out = (ctypes.c_double * 4)()
        if not self._library.library.rwkv_mi_profile_decode(self._ctx.ptr, first_token, n_tokens, out):
            raise ValueError("rwkv_mi_profile_decode failed")
        return {"kernel_ms": out[0], "launches": int(out[1]), "bytes": int(out[2]), "wall_ms": out[3]}

    def profile_prefill(self, tokens: List[int]) -> dict:
        arr = (ctypes.c_uint32 * len(tokens))(*tokens)
        out = (ctypes.c_double * 4)()
        if not self._library.library.rwkv_mi_profile_prefill(self._ctx.ptr, arr, len(tokens), out):
            raise ValueError("rwkv_mi_profile_prefill failed")
        return {"kernel_ms": out[0], "launches": int(out[1]), "ops": int(out[2]), "wall_ms": out[3]}

    def bytes_per_token(self) -> int:
        return int(self._library.library.rwkv_mi_bytes_per_token(self._ctx.ptr))

    def prefill_flops(self, n_tokens: int) -> int:
        return int(self._library.library.rwkv_mi_prefill_flops(self._ctx.ptr, n_tokens))

    def set_graph_enabled(self, enabled: bool) -> None:
        self._library.library.rwkv_mi_set_graph_enabled(self._ctx.ptr, enabled)

    def decode_path(self) -> int:
        """0 = per-op kernels, 1 = fused RWKV-6 layer, 2 = persistent whole-stage kernel."""
        return int(self._library.library.rwkv_mi_decode_path(self._ctx.ptr))

    def persist_kind(self) -> int:
        """Persistent kernel behind decode path 2: 2 = LDS-DMA weight ring, 1 = register prefetch, 0 = none."""
        return int(self._library.library.rwkv_mi_persist_kind(self._ctx.ptr))

    def load_stats(self) -> Tuple[float, int]:
        """(seconds, bytes) of the model file's payload on its way to HBM at creation."""
        sec, b = ctypes.c_double(0.0), ctypes.c_uint64(0)
        self._library.library.rwkv_mi_load_stats(self._ctx.ptr, ctypes.byref(sec), ctypes.byref(b))
        return float(sec.value), int(b.value)

    def persist_info(self) -> str:
        """"persist: ring|regs|k47|none; <what decided it>" (rwkv_mi_persist_info)."""
        return self._library.library.rwkv_mi_persist_info(self._ctx.ptr).decode("utf-8")

    def healthy(self) -> bool:
        return bool(self._library.library.rwkv_mi_decode_healthy(self._ctx.ptr))

    def decode_generation(self) -> int:
        """Hand-over generation the persistent kernel's next launch starts from (advances 8 per layer and launch; 0: path 2 is off)."""
        return int(self._library.library.rwkv_mi_decode_generation(self._ctx.ptr))

    def test_set_tag(self, base: int) -> bool:
        """Test hook (a model opened through librwkv_testhooks.so only): presets the persistent kernel's rolling hand-over tag."""
        return bool(self._library.library.rwkv_mi_test_set_tag(self._ctx.ptr, base & 0xFFFFFFFF))

    def clone(self, thread_count: int = 1) -> "RWKVModel":
        other = object.__new__(RWKVModel)
        other._library = self._library
        other._ctx = self._library.rwkv_clone_context(self._ctx, thread_count)
        other._state_buffer_element_count = self._state_buffer_element_count
        other._logits_buffer_element_count = self._logits_buffer_element_count
        other._valid = True
        return other

    def free(self) -> None:
        if not self._valid:
            raise ValueError("Already freed")
        self._valid = False
        self._library.rwkv_free(self._ctx)

    def __del__(self) -> None:
        if hasattr(self, "_valid") and self._valid:
            self.free()


def _u32(values) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(values, dtype=np.int64).astype(np.uint32))


def _rows(n: int, v, what: str) -> list:
    a = np.asarray(v)
    if a.ndim == 0:
        return [a.item()] * n
    if a.shape != (n,):
        raise ValueError(f"{what} must be a scalar or a sequence of length {n}")
    return a.tolist()


def sample_params(n: int, temperature, top_p, u=-1.0, seed=0):
    """[n] struct rwkv_mi_sample_params; each argument is a scalar (every row) or a sequence of length n."""
    t, p, us, sd = _rows(n, temperature, "temperature"), _rows(n, top_p, "top_p"), _rows(n, u, "u"), _rows(n, seed, "seed")
    arr = (SampleParams * n)()
    for i in range(n):
        arr[i] = SampleParams(float(t[i]), float(p[i]), float(us[i]), int(sd[i]) & 0xFFFFFFFFFFFFFFFF)
    return arr


def penalty_params(n: int, presence, frequency, record=True):
    """[n] struct rwkv_mi_penalty_params; each argument is a scalar (every row) or a sequence of length n."""
    pr, fr, rec = _rows(n, presence, "presence"), _rows(n, frequency, "frequency"), _rows(n, record, "record")
    arr = (PenaltyParams * n)()
    for i in range(n):
        arr[i] = PenaltyParams(float(pr[i]), float(fr[i]), 1 if rec[i] else 0)
    return arr


def stop_params(n: int, max_tokens, stop=None):
    """The stop arguments of RWKVBatch.decode_until for n rows: ([n] struct rwkv_mi_stop_params, seq_lens, seq_tokens), the rows' sequences back
    to back. max_tokens: a scalar (every row) or one value per row. stop: None, a list of token-id sequences for all rows ([[0], [187, 187]]), or
    one such list per row ([[[0]], [], [[187, 187], [535]]]: a list whose elements' elements are sequences)."""
    mt = _rows(n, max_tokens, "max_tokens")
    if stop is None:
        per_row = [[] for _ in range(n)]
    else:
        stop = [list(s) for s in stop]
        if any(len(s) and isinstance(s[0], (list, tuple, np.ndarray)) for s in stop) or (len(stop) == n and all(len(s) == 0 for s in stop) and n > 0):
            if len(stop) != n:
                raise ValueError(f"stop must be a list of sequences or one such list per row ({n} rows)")
            per_row = [[list(q) for q in s] for s in stop]
        else:
            per_row = [stop] * n
    arr = (StopParams * n)()
    lens, toks = [], []
    for i in range(n):
        arr[i] = StopParams(int(mt[i]), len(per_row[i]))
        for q in per_row[i]:
            lens.append(len(q))
            toks.extend(int(t) for t in q)
    return arr, _u32(lens).reshape(-1), _u32(toks).reshape(-1)


def serve_requests(requests):
    """The request table of RWKVBatch.serve from one dict per request: ([R] struct rwkv_mi_serve_request, prompt_tokens, seq_lens, seq_tokens), the
    requests' prompts and stop sequences back to back. Keys: prompt (token ids, at least one), max_tokens; optional from_slot (None: the fresh
    state), stop (a list of token-id sequences), temperature (1.0), top_p (0.8), seed (0), presence (0.0), frequency (0.0), top_k (0), min_p (0.0),
    decay (1.0), repetition (1.0). The keys of serve_extras -- guide, guide_state, bias_slot -- are accepted and not read here."""
    requests = list(requests)
    arr = (ServeRequest * len(requests))()
    prompts, lens, toks = [], [], []
    for i, rq in enumerate(requests):
        unknown = set(rq) - {"prompt", "max_tokens", "from_slot", "stop", "temperature", "top_p", "seed", "presence", "frequency", "top_k", "min_p", "decay", "repetition"}
        unknown -= set(SERVE_EXTRA_KEYS)
        if unknown:
            raise ValueError(f"request {i}: unknown keys {sorted(unknown)}")
        prompt = [int(t) for t in rq["prompt"]]
        if not prompt:
            raise ValueError(f"request {i}: the prompt is empty")
        stop = [[int(t) for t in q] for q in rq.get("stop") or []]
        from_slot = rq.get("from_slot")
        arr[i] = ServeRequest(len(prompt), NO_SLOT if from_slot is None else int(from_slot),
                              SampleParams(float(rq.get("temperature", 1.0)), float(rq.get("top_p", 0.8)), -1.0, int(rq.get("seed", 0)) & 0xFFFFFFFFFFFFFFFF),
                              PenaltyParams(float(rq.get("presence", 0.0)), float(rq.get("frequency", 0.0)), 1),
                              int(rq.get("top_k", 0)), float(rq.get("min_p", 0.0)), float(rq.get("decay", 1.0)), float(rq.get("repetition", 1.0)),
                              StopParams(int(rq["max_tokens"]), len(stop)), 0)
        prompts.extend(prompt)
        for q in stop:
            lens.append(len(q))
            toks.extend(q)
    return arr, _u32(prompts).reshape(-1), _u32(lens).reshape(-1), _u32(toks).reshape(-1)


def serve_extras(requests):
    """The extras table of RWKVBatch.serve ([R] struct rwkv_mi_serve_extra) from the same dicts serve_requests takes, or None when no request
    names one of the optional keys guide (a guide id; None: NO_GUIDE), guide_state (0), bias_slot (a slot whose bias table the request reads;
    None: NO_SLOT)."""
    requests = list(requests)
    if not any(k in rq for rq in requests for k in SERVE_EXTRA_KEYS):
        return None
    arr = (ServeExtra * len(requests))()
    for i, rq in enumerate(requests):
        guide, bias_slot = rq.get("guide"), rq.get("bias_slot")
        arr[i] = ServeExtra(NO_GUIDE if guide is None else int(guide), int(rq.get("guide_state", 0)), NO_SLOT if bias_slot is None else int(bias_slot), 0)
    return arr


def guide_edges(edges):
    """A guide in the CSR form of rwkv_mi_batch_guide_create from one {token: next_state} dict per state: (edge_begin [n_states + 1],
    edge_tokens, edge_next), each state's tokens ascending."""
    begin, toks, nxt = [0], [], []
    for e in edges:
        for t in sorted(int(k) for k in e):
            toks.append(t)
            nxt.append(int(e[t]))
        begin.append(len(toks))
    return _u32(begin).reshape(-1), _u32(toks).reshape(-1), _u32(nxt).reshape(-1)


def lookup_draft(history, k: int, ngram: int = 3) -> List[int]:
    """Prompt-lookup drafting: the (at most k) tokens that followed the most recent EARLIER occurrence of the last `ngram` tokens of
    `history`; fewer where the history ends first, none where there is no such occurrence or the history is shorter than ngram + 1."""
    h = [int(t) for t in history]
    k, ngram = int(k), int(ngram)
    if k <= 0 or ngram <= 0 or len(h) <= ngram:
        return []
    tail = h[-ngram:]
    for start in range(len(h) - ngram - 1, -1, -1):   # (the occurrence that is the tail itself is not an earlier one)
        if h[start:start + ngram] == tail:
            return h[start + ngram:start + ngram + k]
    return []


def _bias_arrays(bias: dict):
    ids = _u32(list(bias.keys())).reshape(-1)
    values = np.ascontiguousarray(np.asarray(list(bias.values()), dtype=np.float64).astype(np.float32)).reshape(-1)
    return ids, values


class ServeSession:
    """A serve session of a RWKVBatch (rwkv_mi_batch_serve_open ..; RWKVBatch.serve_open creates it). submit(**request) takes the keys of
    serve_requests and serve_extras and returns the request's id; poll() enqueues one block of passes when there is work and returns what
    the blocks before it emitted; cancel(id) drops a request; close() cancels what is in flight and hands the batch back. Every request's
    tokens are what it gives alone, whenever it was submitted."""

    def __init__(self, batch: "RWKVBatch", lanes: List[int], family: int, limits: ServeLimits) -> None:
        self._batch = batch
        self._L = batch._L
        self._ptr = None
        s = _u32(lanes).reshape(-1)
        self.n_lanes = int(s.size)
        self.limits = limits
        ptr = self._L.rwkv_mi_batch_serve_open(batch._ptr, s.ctypes.data_as(P_UINT32), s.size, int(family), ctypes.byref(limits))
        if not ptr:
            batch._fail("rwkv_mi_batch_serve_open")
        self._ptr = ptr
        batch._session = self
        self.last_request = None
        self._events = (ServeEvent * max(int(limits.capacity), 1))()
        self._tokens = np.empty(max(int(limits.capacity) * int(limits.stride), 1), dtype=np.uint32)

    def _open(self):
        if not self._ptr:
            raise ValueError("the session is closed")

    def submit(self, **request) -> int:
        """One request (prompt, max_tokens, and the optional keys of serve_requests / serve_extras); a misspelt key raises. Returns its id."""
        self._open()
        arr, prompts, seq_lens, seq_tokens = serve_requests([request])
        extras = serve_extras([request])
        rid = ctypes.c_uint32(0)
        if not self._L.rwkv_mi_batch_serve_submit(self._ptr, arr, prompts.ctypes.data_as(P_UINT32), seq_lens.ctypes.data_as(P_UINT32),
                                                  seq_tokens.ctypes.data_as(P_UINT32), extras, ctypes.byref(rid)):
            self._batch._fail("rwkv_mi_batch_serve_submit")
        return int(rid.value)

    def cancel(self, rid: int) -> bool:
        self._open()
        return bool(self._L.rwkv_mi_batch_serve_cancel(self._ptr, int(rid)))

    def poll(self, drain: bool = False, max_events: Optional[int] = None, max_tokens: Optional[int] = None):
        """One poll: a list of dict(id, first, tokens, finished, stopped_by, lane, start_pass, guide_state, guide_misses), one per request with
        new tokens or a newly known end. drain: the block this poll enqueued is waited for as well. max_events / max_tokens bound what one
        call delivers (the rest comes with the next)."""
        self._open()
        me = len(self._events) if max_events is None else min(int(max_events), len(self._events))
        mt = self._tokens.size if max_tokens is None else min(int(max_tokens), self._tokens.size)
        ne, nt = ctypes.c_size_t(0), ctypes.c_size_t(0)
        if not self._L.rwkv_mi_batch_serve_poll(self._ptr, POLL_DRAIN if drain else 0, self._events, me, self._tokens.ctypes.data_as(P_UINT32), mt,
                                                ctypes.byref(ne), ctypes.byref(nt)):
            self._batch._fail("rwkv_mi_batch_serve_poll")
        out, at = [], 0
        for i in range(ne.value):
            e = self._events[i]
            out.append(dict(id=int(e.id), first=int(e.first), tokens=self._tokens[at: at + e.n_new].copy(), finished=bool(e.finished), stopped_by=int(e.stopped_by),
                            lane=int(e.lane), start_pass=int(e.start_pass), guide_state=int(e.guide_state), guide_misses=int(e.guide_misses)))
            at += e.n_new
        return out

    def stats(self):
        """dict(passes, blocks, in_flight, room): passes and blocks enqueued so far, requests in flight, submits the ring has room for."""
        self._open()
        passes, blocks, in_flight, room = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
        self._L.rwkv_mi_batch_serve_stats(self._ptr, ctypes.byref(passes), ctypes.byref(blocks), ctypes.byref(in_flight), ctypes.byref(room))
        return dict(passes=int(passes.value), blocks=int(blocks.value), in_flight=int(in_flight.value), room=int(room.value))

    def close(self):
        """Cancels what is in flight, drains and frees the session; the batch is usable as before. Returns last_request [n_lanes]: the id each
        lane served last (NO_TOKEN: none)."""
        if not self._ptr:
            return self.last_request
        last = np.empty(self.n_lanes, dtype=np.uint32)
        ptr, self._ptr = self._ptr, None
        self._batch._session = None
        ok = self._L.rwkv_mi_batch_serve_close(ptr, last.ctypes.data_as(P_UINT32))
        self.last_request = last
        if not ok:
            self._batch._fail("rwkv_mi_batch_serve_close")
        return last

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class RWKVBatch:
    """n_slots device-resident sequences of one model advanced together, one pass over the weights per step (rwkv_mi_batch_*).

    Row i of a call is slot slots[i] fed tokens[i]; every row equals rwkv_eval of that sequence alone, bit for bit. Bound to `model`'s
    context (a single-device one); free it before the model. Not thread-safe."""

    def __init__(self, model: RWKVModel, n_slots: int) -> None:
        self._model = model
        self._L = model._library.library
        self.n_slots = int(n_slots)
        self._ptr = self._L.rwkv_mi_batch_create(model._ctx.ptr, self.n_slots)
        if not self._ptr:
            raise ValueError(f"rwkv_mi_batch_create failed (error flags {model._library.rwkv_get_last_error(model._ctx)})")
        self._state_len = model.state_len
        self._n_vocab = model.n_vocab
        self.last_error = 0

    def _fail(self, what: str):
        self.last_error = self._model._library.rwkv_get_last_error(self._model._ctx)   # (reported on the model's context)
        raise ValueError(f"{what} failed (error flags {self.last_error})")

    def state_load(self, slot: int, state_in: Optional[np.ndarray] = None) -> None:
        self._model._check(state_in, "state_in", self._state_len)
        if not self._L.rwkv_mi_batch_state_load(self._ptr, slot, ctypes.cast(_ptr(state_in), P_FLOAT)):
            self._fail("rwkv_mi_batch_state_load")

    def state_store(self, slot: int) -> np.ndarray:
        s = np.empty(self._state_len, dtype=np.float32)
        if not self._L.rwkv_mi_batch_state_store(self._ptr, slot, ctypes.cast(s.ctypes.data, P_FLOAT)):
            self._fail("rwkv_mi_batch_state_store")
        return s

    def from_context(self, slot: int, model: RWKVModel) -> None:
        """The resident state of `model`'s context (e.g. after a prefill) into a slot, device to device."""
        if not self._L.rwkv_mi_batch_state_from_context(self._ptr, slot, model._ctx.ptr):
            self._fail("rwkv_mi_batch_state_from_context")

    def to_context(self, slot: int, model: RWKVModel) -> None:
        """A slot into the resident state of `model`'s context, device to device."""
        if not self._L.rwkv_mi_batch_state_to_context(self._ptr, slot, model._ctx.ptr):
            self._fail("rwkv_mi_batch_state_to_context")

    @staticmethod
    def _slot_tokens(slots, tokens, what: str):
        """slots and one token per slot (the argument named `what`) as uint32 arrays of one length"""
        s, t = _u32(slots), _u32(tokens)
        if s.size != t.size:
            raise ValueError(f"slots and {what} differ in length")
        return s, t

    def _sampled(self, name: str, n: int, want_logits: bool, *args):
        """The single pass `name`(batch, *args, sampled_out, logits_out): tokens [n], with the logits [n][n_vocab] when want_logits."""
        out = np.empty(n, dtype=np.uint32)
        logits = np.empty((n, self._n_vocab), dtype=np.float32) if want_logits else None
        if not getattr(self._L, name)(self._ptr, *args, out.ctypes.data_as(P_UINT32), ctypes.cast(_ptr(logits), P_FLOAT)):
            self._fail(name)
        return (out, logits) if want_logits else out

    def _loop(self, name: str, n: int, n_tokens: int, *args) -> Tuple[np.ndarray, float]:
        """The device loop `name`(batch, *args, tokens_out, elapsed_ms): tokens [n][n_tokens], elapsed milliseconds."""
        out = np.empty((n, n_tokens), dtype=np.uint32)
        ms = ctypes.c_float(0.0)
        if not getattr(self._L, name)(self._ptr, *args, ctypes.cast(out.ctypes.data, P_UINT32), ctypes.byref(ms)):
            self._fail(name)
        return out, float(ms.value)

    def eval(self, slots: List[int], tokens: List[int], want_logits: bool = True) -> Optional[np.ndarray]:
        """One token per named slot in one pass; logits [n][n_vocab] in call order (None when want_logits is False)."""
        s, t = self._slot_tokens(slots, tokens, "tokens")
        out = np.empty((s.size, self._n_vocab), dtype=np.float32) if want_logits else None
        if not self._L.rwkv_mi_batch_eval(self._ptr, s.ctypes.data_as(P_UINT32), t.ctypes.data_as(P_UINT32), s.size, ctypes.cast(_ptr(out), P_FLOAT)):
            self._fail("rwkv_mi_batch_eval")
        return out

    def decode_greedy(self, slots: List[int], first_tokens: List[int], n_tokens: int) -> Tuple[np.ndarray, float]:
        """Greedy loop on the device for every named slot: tokens [n][n_tokens], elapsed milliseconds."""
        s, t = self._slot_tokens(slots, first_tokens, "first_tokens")
        return self._loop("rwkv_mi_batch_decode_greedy", s.size, n_tokens, s.ctypes.data_as(P_UINT32), t.ctypes.data_as(P_UINT32), s.size, n_tokens)

    def eval_sample(self, slots: List[int], tokens: List[int], temperature=1.0, top_p=0.8, u=-1.0, seed=0, want_logits: bool = False):
        """One token per named slot in one pass, then one token sampled per row on the device: tokens [n] (and the logits [n][n_vocab]
        when want_logits). temperature, top_p, u, seed: a scalar (every row) or a sequence of length n. u < 0 draws from the slot's
        own stream uniform01(seed, counter of the slot)."""
        s, t = self._slot_tokens(slots, tokens, "tokens")
        return self._sampled("rwkv_mi_batch_eval_sample", s.size, want_logits, s.ctypes.data_as(P_UINT32), t.ctypes.data_as(P_UINT32), s.size,
                             sample_params(s.size, temperature, top_p, u, seed))

    def decode_sample(self, slots: List[int], first_tokens: List[int], n_tokens: int, temperature=1.0, top_p=0.8, seed=0) -> Tuple[np.ndarray, float]:
        """Sampling loop on the device for every named slot (their draw counters start from 0): tokens [n][n_tokens], elapsed milliseconds."""
        s, t = self._slot_tokens(slots, first_tokens, "first_tokens")
        return self._loop("rwkv_mi_batch_decode_sample", s.size, n_tokens, s.ctypes.data_as(P_UINT32), t.ctypes.data_as(P_UINT32), s.size, n_tokens,
                          sample_params(s.size, temperature, top_p, -1.0, seed))

    @staticmethod
    def _ragged(slots, token_lists):
        """slots, lens and the rows' tokens back to back (the lengths are passed on as they are: an empty row is rejected by the library)"""
        s = _u32(slots)
        rows = [_u32(r).reshape(-1) for r in token_lists]
        if s.size != len(rows):
            raise ValueError("slots and token_lists differ in length")
        lens = _u32([r.size for r in rows])
        toks = np.ascontiguousarray(np.concatenate(rows)) if rows else _u32([])
        return s, lens, toks

    def eval_ragged(self, slots: List[int], token_lists: List[List[int]], want_logits: bool = True) -> Optional[np.ndarray]:
        """token_lists[i] (one token or many: a prompt, or a chunk of one) to slot slots[i], all rows in ONE pass over the weights; logits
        [n][n_vocab] of each row's last token in call order (None when want_logits is False). Every row equals rwkv_eval_sequence of its
        tokens alone, bit for bit."""
        s, lens, toks = self._ragged(slots, token_lists)
        out = np.empty((s.size, self._n_vocab), dtype=np.float32) if want_logits else None
        if not self._L.rwkv_mi_batch_eval_ragged(self._ptr, s.ctypes.data_as(P_UINT32), lens.ctypes.data_as(P_UINT32), toks.ctypes.data_as(P_UINT32),
                                                 s.size, ctypes.cast(_ptr(out), P_FLOAT)):
            self._fail("rwkv_mi_batch_eval_ragged")
        return out

    def eval_ragged_sample(self, slots: List[int], token_lists: List[List[int]], temperature=1.0, top_p=0.8, u=-1.0, seed=0, want_logits: bool = False):
        """As eval_ragged, then one token sampled per row from its last-token logits on the device: tokens [n] (and the logits when
        want_logits). The parameters as eval_sample takes them. Every row is sampled: give a non-final prompt chunk temperature 0 (an
        argmax, which leaves the slot's draw counter where it was)."""
        s, lens, toks = self._ragged(slots, token_lists)
        return self._sampled("rwkv_mi_batch_eval_ragged_sample", s.size, want_logits, s.ctypes.data_as(P_UINT32), lens.ctypes.data_as(P_UINT32),
                             toks.ctypes.data_as(P_UINT32), s.size, sample_params(s.size, temperature, top_p, u, seed))

    def score_ragged(self, slots: List[int], token_lists: List[List[int]], target_lists: Optional[List[List[int]]] = None, want_argmax: bool = True):
        """token_lists[i] to slot slots[i], all rows in ONE pass (as eval_ragged), with the prediction after EVERY token: (list of logprob
        arrays, list of argmax arrays), one array per row; target_lists[i][t] is scored against the logits after token_lists[i][t]. Each row
        equals RWKVModel.score_resident of its tokens alone, bit for bit. A list is None when it was not asked for."""
        s, lens, toks = self._ragged(slots, token_lists)
        tg = None
        if target_lists is not None:
            rows = [_u32(r).reshape(-1) for r in target_lists]
            if [r.size for r in rows] != lens.tolist():
                raise ValueError("token_lists and target_lists differ in shape")
            tg = np.ascontiguousarray(np.concatenate(rows)) if rows else _u32([])
        logprobs = np.empty(toks.size, dtype=np.float32) if tg is not None else None
        argmax = np.empty(toks.size, dtype=np.uint32) if want_argmax else None
        if not self._L.rwkv_mi_batch_score_ragged(self._ptr, s.ctypes.data_as(P_UINT32), lens.ctypes.data_as(P_UINT32), toks.ctypes.data_as(P_UINT32),
                                                  ctypes.cast(_ptr(tg), P_UINT32), s.size, ctypes.cast(_ptr(logprobs), P_FLOAT), ctypes.cast(_ptr(argmax), P_UINT32)):
            self._fail("rwkv_mi_batch_score_ragged")
        cuts = np.cumsum(lens.astype(np.int64))[:-1]
        return (None if logprobs is None else np.split(logprobs, cuts)), (None if argmax is None else np.split(argmax, cuts))

    def rng_seek(self, slot: int, counter: int) -> None:
        """Sets a slot's draw counter (0 for a new request in a reused slot)."""
        if not self._L.rwkv_mi_batch_rng_seek(self._ptr, slot, counter):
            self._fail("rwkv_mi_batch_rng_seek")

    def set_truncation(self, slot: int, top_k: int = 0, min_p: float = 0.0) -> None:
        """The slot's truncation setting, read by every draw of the slot from now on (eval_sample, the ragged and penalised forms, the
        loops, decode_until, eval_draft; guided or not): top_k (0: off) masks all but the top_k largest values the draw reads to -inf before
        the softmax; min_p (0: off) cuts the probabilities below min_p * the largest, beside top-p. (0, 0) clears. copy_state does not
        carry it: set it on the destination slot."""
        if not self._L.rwkv_mi_batch_truncation_set(self._ptr, slot, int(top_k), float(min_p)):
            self._fail("rwkv_mi_batch_truncation_set")

    def truncation(self, slot: int) -> Tuple[int, float]:
        """The slot's truncation setting (top_k, min_p); (0, 0.0) is none."""
        k, p = ctypes.c_uint32(0), ctypes.c_float(0.0)
        if not self._L.rwkv_mi_batch_truncation_get(self._ptr, slot, ctypes.byref(k), ctypes.byref(p)):
            self._fail("rwkv_mi_batch_truncation_get")
        return int(k.value), float(p.value)

    def set_repetition(self, slot: int, decay: float = 1.0, repetition: float = 1.0) -> None:
        """The slot's repetition setting, read by every PENALISED draw of the slot from now on (eval_sample_penalized, the ragged form, the
        penalised loop, decode_until and eval_draft with penalties; guided or truncating or not): repetition (1: off) divides the positive and
        multiplies the other logits of the tokens that have occurred; decay (1: off) makes the slot's occurrence row a float row that every
        recorded draw multiplies by decay before it counts its token. (1, 1) clears. A set that turns decay on or off zeroes the row.
        copy_state does not carry the setting: set it on the destination slot."""
        if not self._L.rwkv_mi_batch_repetition_set(self._ptr, slot, float(decay), float(repetition)):
            self._fail("rwkv_mi_batch_repetition_set")

    def repetition(self, slot: int) -> Tuple[float, float]:
        """The slot's repetition setting (decay, repetition); (1.0, 1.0) is none."""
        d, r = ctypes.c_float(0.0), ctypes.c_float(0.0)
        if not self._L.rwkv_mi_batch_repetition_get(self._ptr, slot, ctypes.byref(d), ctypes.byref(r)):
            self._fail("rwkv_mi_batch_repetition_get")
        return float(d.value), float(r.value)

    def counts_f32(self, slot: int) -> np.ndarray:
        """The slot's occurrence row as float32 [n_vocab]: the decayed occurrences of a decaying slot, the counts of any other."""
        out = np.empty(self._n_vocab, dtype=np.float32)
        if not self._L.rwkv_mi_batch_counts_store_f32(self._ptr, slot, out.ctypes.data_as(P_FLOAT)):
            self._fail("rwkv_mi_batch_counts_store_f32")
        return out

    # --- penalised sampling: one occurrence table and one bias table per slot (include/rwkv_mi355x.h) ---

    def counts_reset(self, slot: int) -> None:
        if not self._L.rwkv_mi_batch_counts_reset(self._ptr, slot):
            self._fail("rwkv_mi_batch_counts_reset")

    def counts_add(self, slot: int, tokens: List[int]) -> None:
        """count[t] += 1 in the slot's occurrence table for every t of `tokens` (resuming a recorded response)."""
        t = _u32(tokens).reshape(-1)
        if not self._L.rwkv_mi_batch_counts_add(self._ptr, slot, t.ctypes.data_as(P_UINT32), t.size):
            self._fail("rwkv_mi_batch_counts_add")

    def counts(self, slot: int) -> np.ndarray:
        """The slot's occurrence table, uint32 [n_vocab]."""
        out = np.empty(self._n_vocab, dtype=np.uint32)
        if not self._L.rwkv_mi_batch_counts_store(self._ptr, slot, out.ctypes.data_as(P_UINT32)):
            self._fail("rwkv_mi_batch_counts_store")
        return out

    def set_logit_bias(self, slot: int, bias: dict) -> None:
        """Replaces the slot's logit bias by {token id: value}; an empty dict clears it."""
        ids, values = _bias_arrays(bias)
        if not self._L.rwkv_mi_batch_logit_bias_set(self._ptr, slot, ids.ctypes.data_as(P_UINT32), values.ctypes.data_as(P_FLOAT), ids.size):
            self._fail("rwkv_mi_batch_logit_bias_set")

    def eval_sample_penalized(self, slots: List[int], tokens: List[int], temperature=1.0, top_p=0.8, u=-1.0, seed=0, presence=0.2, frequency=0.2,
                              record=True, want_logits: bool = False):
        """eval_sample with each row's logits less presence + count * frequency of its slot, plus the slot's bias; a row with `record`
        counts its token afterwards. presence, frequency, record: a scalar (every row) or a sequence of length n."""
        s, t = self._slot_tokens(slots, tokens, "tokens")
        return self._sampled("rwkv_mi_batch_eval_sample_penalized", s.size, want_logits, s.ctypes.data_as(P_UINT32), t.ctypes.data_as(P_UINT32), s.size,
                             sample_params(s.size, temperature, top_p, u, seed), penalty_params(s.size, presence, frequency, record))

    def eval_ragged_sample_penalized(self, slots: List[int], token_lists: List[List[int]], temperature=1.0, top_p=0.8, u=-1.0, seed=0, presence=0.2,
                                     frequency=0.2, record=True, want_logits: bool = False):
        """eval_ragged_sample with the penalised draw. Give a non-final prompt chunk temperature 0 AND record False: nothing of the slot's
        draw counter or counts moves then."""
        s, lens, toks = self._ragged(slots, token_lists)
        return self._sampled("rwkv_mi_batch_eval_ragged_sample_penalized", s.size, want_logits, s.ctypes.data_as(P_UINT32), lens.ctypes.data_as(P_UINT32),
                             toks.ctypes.data_as(P_UINT32), s.size, sample_params(s.size, temperature, top_p, u, seed),
                             penalty_params(s.size, presence, frequency, record))

    def decode_sample_penalized(self, slots: List[int], first_tokens: List[int], n_tokens: int, temperature=1.0, top_p=0.8, seed=0, presence=0.2,
                                frequency=0.2) -> Tuple[np.ndarray, float]:
        """decode_sample with the penalised draw, every step recorded: tokens [n][n_tokens], elapsed milliseconds. It continues -- neither
        the counts nor the draw counters are reset; call counts_reset(slot) and rng_seek(slot, 0) for a new request."""
        s, t = self._slot_tokens(slots, first_tokens, "first_tokens")
        return self._loop("rwkv_mi_batch_decode_sample_penalized", s.size, n_tokens, s.ctypes.data_as(P_UINT32), t.ctypes.data_as(P_UINT32), s.size, n_tokens,
                          sample_params(s.size, temperature, top_p, -1.0, seed), penalty_params(s.size, presence, frequency, True))

    def decode_until(self, slots: List[int], first_tokens: List[int], max_tokens, stop=None, temperature=None, top_p=0.8, seed=0, presence=None,
                     frequency=None):
        """The device loop in which every row ends by itself: at one of its stop sequences (token ids; `stop` as stop_params takes it) or after
        max_tokens tokens (a scalar or one value per row). temperature None: the greedy loop; a temperature: decode_sample (the slots' draw
        counters start from 0); with presence or frequency given: decode_sample_penalized (it continues, every step records). Returns (list of
        n uint32 arrays, each of its row's own length; stopped_by [n]: the index of the row's matching sequence, or NO_TOKEN when the budget
        ended it; elapsed milliseconds). Each slot is left exactly as the plain loop of its row's length leaves it."""
        s, t = self._slot_tokens(slots, first_tokens, "first_tokens")
        n = s.size
        sp, seq_lens, seq_tokens = stop_params(n, max_tokens, stop)
        penalised = presence is not None or frequency is not None
        if penalised and temperature is None:
            raise ValueError("penalties need a temperature (the greedy loop has no penalised form)")
        params = None if temperature is None else sample_params(n, temperature, top_p, -1.0, seed)
        pens = penalty_params(n, 0.0 if presence is None else presence, 0.0 if frequency is None else frequency, True) if penalised else None
        stride = max([int(r.max_tokens) for r in sp], default=0)
        out = np.empty((n, stride), dtype=np.uint32)
        lens = np.zeros(n, dtype=np.uint32)
        why = np.empty(n, dtype=np.uint32)
        ms = ctypes.c_float(0.0)
        if not self._L.rwkv_mi_batch_decode_until(self._ptr, s.ctypes.data_as(P_UINT32), t.ctypes.data_as(P_UINT32), n, params, pens, sp,
                                                  seq_lens.ctypes.data_as(P_UINT32), seq_tokens.ctypes.data_as(P_UINT32), stride,
                                                  ctypes.cast(out.ctypes.data, P_UINT32), lens.ctypes.data_as(P_UINT32), why.ctypes.data_as(P_UINT32),
                                                  ctypes.byref(ms)):
            self._fail("rwkv_mi_batch_decode_until")
        return [out[i, : int(lens[i])].copy() for i in range(n)], why, float(ms.value)

    def serve(self, lanes: List[int], requests, family: int = SERVE_GREEDY, report: bool = False):
        """Continuous batching: the slots `lanes` serve the queue `requests` (dicts, as serve_requests takes them; at least as many as lanes) in
        one device loop -- lane r starts with request r, and a lane whose request has ended takes the next one not yet taken on the following
        pass, in lane order. A request starts from the fresh state or from its from_slot's (never a lane), is fed its prompt one token a pass and
        then decodes as a row of decode_until with its own settings; family: SERVE_GREEDY, SERVE_SAMPLE or SERVE_PENALIZED, the call's. Returns
        a dict: tokens (one uint32 array per request, of its own length), stopped_by [R], lane [R] (index into lanes), start_pass [R],
        last_request [n] (the request whose end state each lane holds), elapsed_ms, guide_state [R] and guide_misses [R] (0 for a request
        without a guide). Every request's tokens are what it gives alone.
        A request may carry a guide (keys guide, guide_state) and, in the penalised family, the slot whose bias table it reads (bias_slot; set
        it with set_logit_bias first; never a lane). report: the batch has the report on (set_logprobs) and the call fills it per request --
        read it with logprobs(), [R][stride]. Either goes through rwkv_mi_batch_serve_ex; a queue with neither through rwkv_mi_batch_serve."""
        requests = list(requests)
        s = _u32(lanes).reshape(-1)
        arr, prompts, seq_lens, seq_tokens = serve_requests(requests)
        extras = serve_extras(requests)
        n, R = s.size, len(arr)
        stride = max([int(r.stop.max_tokens) for r in arr], default=0)
        out = np.empty((R, stride), dtype=np.uint32)
        lens = np.zeros(R, dtype=np.uint32)
        why, lane, start = (np.empty(R, dtype=np.uint32) for _ in range(3))
        last = np.empty(n, dtype=np.uint32)
        g_state, g_misses = np.zeros(R, dtype=np.uint32), np.zeros(R, dtype=np.uint32)
        ms = ctypes.c_float(0.0)
        args = (self._ptr, s.ctypes.data_as(P_UINT32), n, int(family), arr, R, prompts.ctypes.data_as(P_UINT32),
                seq_lens.ctypes.data_as(P_UINT32), seq_tokens.ctypes.data_as(P_UINT32), stride,
                ctypes.cast(out.ctypes.data, P_UINT32), lens.ctypes.data_as(P_UINT32), why.ctypes.data_as(P_UINT32),
                lane.ctypes.data_as(P_UINT32), start.ctypes.data_as(P_UINT32), last.ctypes.data_as(P_UINT32), ctypes.byref(ms))
        if extras is not None or report:
            if not self._L.rwkv_mi_batch_serve_ex(*args, extras, g_state.ctypes.data_as(P_UINT32), g_misses.ctypes.data_as(P_UINT32)):
                self._fail("rwkv_mi_batch_serve_ex")
        elif not self._L.rwkv_mi_batch_serve(*args):
            self._fail("rwkv_mi_batch_serve")
        return {"tokens": [out[q, : int(lens[q])].copy() for q in range(R)], "stopped_by": why, "lane": lane, "start_pass": start,
                "last_request": last, "elapsed_ms": float(ms.value), "guide_state": g_state, "guide_misses": g_misses}

    def serve_open(self, lanes: List[int], family: int = SERVE_GREEDY, capacity: int = 16, max_prompt: int = 64, stride: int = 64,
                   max_seqs: int = STOP_MAX_SEQS, max_seq_tokens: int = STOP_MAX_SEQS * STOP_MAX_LEN, features: int = 0) -> "ServeSession":
        """A serve session on the slots `lanes`: serve()'s device loop kept open between host calls -- submit requests, poll their tokens as
        they are emitted, cancel them. capacity: the entries of the request ring (requests in flight); max_prompt, stride (every max_tokens
        <= stride), max_seqs, max_seq_tokens: per request; features: SERVE_CUT | SERVE_REP | SERVE_GUIDED, what a request may ask for. While
        the session is open the batch runs no other pass. Use it as a context manager, or close() it."""
        return ServeSession(self, lanes, family, ServeLimits(int(capacity), int(max_prompt), int(stride), int(max_seqs), int(max_seq_tokens), int(features), 0))

    # --- speculative decoding (include/rwkv_mi355x.h) ---

    def eval_draft(self, slots: List[int], rows: List[List[int]], params=None, penalties=None, want_logits: bool = False):
        """rows[i] = [x0, d1 .. dk] (k <= DRAFT_MAX) to slot slots[i], all rows in ONE pass: x0 is the token not yet fed, d1 .. dk a draft of what
        follows. Returns (emitted: one list per row -- the accepted draft tokens, then the correction or bonus token --, lens uint32 [n]), with
        the logits [n][n_vocab] each row's last token was chosen from as a third element when want_logits. params None: greedy; sample_params(..):
        sampled, the slots' draw counters continuing; with penalty_params(..) as well: penalised, every emitted token recorded. What is emitted,
        and every slot's state, draw counter and counts, are those of the plain loop of len(emitted[i]) steps: continue by feeding
        emitted[i][-1] as the next x0."""
        s, lens, toks = self._ragged(slots, rows)
        n = s.size
        stride = max(int(lens.max()) if n else 0, 1)
        out = np.empty((n, stride), dtype=np.uint32)
        kept = np.zeros(n, dtype=np.uint32)
        logits = np.empty((n, self._n_vocab), dtype=np.float32) if want_logits else None
        if not self._L.rwkv_mi_batch_eval_draft(self._ptr, s.ctypes.data_as(P_UINT32), lens.ctypes.data_as(P_UINT32), toks.ctypes.data_as(P_UINT32), n,
                                                params, penalties, stride, ctypes.cast(out.ctypes.data, P_UINT32), kept.ctypes.data_as(P_UINT32),
                                                ctypes.cast(_ptr(logits), P_FLOAT)):
            self._fail("rwkv_mi_batch_eval_draft")
        emitted = [out[i, : int(kept[i])].tolist() for i in range(n)]
        return (emitted, kept, logits) if want_logits else (emitted, kept)

    # --- slot-to-slot copy and beam search (include/rwkv_mi355x.h) ---

    def copy_state(self, dst: int, src: int, counter: bool = False, counts: bool = False, bias: bool = False) -> None:
        """Slot src's state into slot dst, device to device (n samples of one prompt: prefill once, copy n - 1 times); with counter, counts, bias:
        the slot's draw counter, occurrence table, bias table as well. dst == src does nothing."""
        what = COPY_STATE | (COPY_COUNTER if counter else 0) | (COPY_COUNTS if counts else 0) | (COPY_BIAS if bias else 0)
        if not self._L.rwkv_mi_batch_state_copy(self._ptr, dst, src, what):
            self._fail("rwkv_mi_batch_state_copy")

    def decode_beam(self, slots, first_tokens: List[int], width: int, n_tokens: int, end_tokens=(), want_logprobs: bool = True):
        """Beam search on the device: G groups of `width` hypotheses. slots: [G][width] distinct slots (a flat list of G * width is taken too);
        group g starts from the state of slots[g][0] -- which is consumed: keep a prompt with copy_state -- and first_tokens[g]. A hypothesis
        finishes at one of end_tokens (at most 8 ids). Returns (tokens [G][width][n_tokens] with NO_TOKEN past a hypothesis' length, lens
        [G][width], scores float64 [G][width], logprobs float32 [G][width][n_tokens] or None, elapsed milliseconds); hypothesis 0 is the best.
        Afterwards slots[g][j] continues an unfinished hypothesis j as a greedy loop's slot would: eval its last token."""
        s = _u32(slots).reshape(-1)
        t = _u32(first_tokens).reshape(-1)
        width = int(width)
        if width < 1 or s.size != t.size * width:
            raise ValueError("slots must hold width slots per first token")
        G = t.size
        ends = _u32(list(end_tokens)).reshape(-1)
        params = BeamParams(width, ends.size, ends.ctypes.data_as(P_UINT32) if ends.size else None)
        tokens = np.empty((G, width, n_tokens), dtype=np.uint32)
        lens = np.zeros((G, width), dtype=np.uint32)
        scores = np.empty((G, width), dtype=np.float64)
        lps = np.empty((G, width, n_tokens), dtype=np.float32) if want_logprobs else None
        ms = ctypes.c_float(0.0)
        if not self._L.rwkv_mi_batch_decode_beam(self._ptr, s.ctypes.data_as(P_UINT32), t.ctypes.data_as(P_UINT32), G, ctypes.byref(params), n_tokens,
                                                 ctypes.cast(tokens.ctypes.data, P_UINT32), lens.ctypes.data_as(P_UINT32),
                                                 scores.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.cast(_ptr(lps), P_FLOAT), ctypes.byref(ms)):
            self._fail("rwkv_mi_batch_decode_beam")
        return tokens, lens, scores, lps, float(ms.value)

    # --- guided decoding: token automata that mask the device sampler per slot (include/rwkv_mi355x.h) ---

    def create_guide(self, edges) -> int:
        """A guide from one {token: next_state} dict per state (every state allows at least one token): its id. The batch holds up to GUIDE_MAX
        guides, shared by its slots."""
        begin, toks, nxt = guide_edges(edges)
        out = ctypes.c_uint32(NO_GUIDE)
        if not self._L.rwkv_mi_batch_guide_create(self._ptr, begin.size - 1, begin.ctypes.data_as(P_UINT32), toks.ctypes.data_as(P_UINT32),
                                                  nxt.ctypes.data_as(P_UINT32), ctypes.byref(out)):
            self._fail("rwkv_mi_batch_guide_create")
        return int(out.value)

    def free_guide(self, guide: int) -> None:
        """Releases a guide that no slot has attached."""
        if not self._L.rwkv_mi_batch_guide_free(self._ptr, guide):
            self._fail("rwkv_mi_batch_guide_free")

    def attach_guide(self, slot: int, guide: int, state: int = 0) -> None:
        """From now on the sampled and penalised calls draw the slot's tokens under `guide`, starting in `state`; the slot's miss counter
        starts from 0. The greedy loops and decode_beam reject a slot with a guide."""
        if not self._L.rwkv_mi_batch_guide_attach(self._ptr, slot, guide, state):
            self._fail("rwkv_mi_batch_guide_attach")

    def detach_guide(self, slot: int) -> None:
        if not self._L.rwkv_mi_batch_guide_attach(self._ptr, slot, NO_GUIDE, 0):
            self._fail("rwkv_mi_batch_guide_attach")

    def guide_state(self, slot: int) -> Tuple[int, int, int]:
        """(guide, state, misses) of a slot; guide is NO_GUIDE for a slot without one. misses: the draws whose token the guide did not allow
        (all-NaN logits, or a bias of -inf on every allowed token)."""
        g, s, m = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
        if not self._L.rwkv_mi_batch_guide_state(self._ptr, slot, ctypes.byref(g), ctypes.byref(s), ctypes.byref(m)):
            self._fail("rwkv_mi_batch_guide_state")
        return int(g.value), int(s.value), int(m.value)

    # --- the report: log-probs and top-N alternatives of every emitted token (include/rwkv_mi355x.h) ---

    def set_logprobs(self, top_n: int = 0, enabled: bool = True) -> None:
        """Turns the report on, with top_n <= TOP_MAX alternatives per token, or off. While it is on, every call that emits tokens (the sampled
        passes, the device loops -- the greedy one included -- and decode_until) records each emitted token's log-prob and the top_n of its step."""
        if not self._L.rwkv_mi_batch_set_logprobs(self._ptr, bool(enabled), int(top_n)):
            self._fail("rwkv_mi_batch_set_logprobs")

    def logprobs(self):
        """The report of the last emitting call, rows in its order: (chosen [rows][steps], top_ids [rows][steps][top_n], top_logprobs
        [rows][steps][top_n]), from the MODEL'S logits (a penalised or biased row's token need not be among its top_n). chosen equals
        score_ragged's log-prob of the emitted token, bit for bit. After decode_until a row's entries behind its length are 0 / NO_TOKEN / -inf."""
        out = _report(self._L, "rwkv_mi_batch_", self._ptr)
        if out is None:
            self._fail("rwkv_mi_batch_logprobs_store")
        return out

    def last_loop_passes(self) -> int:
        """Passes the batch's last device loop enqueued (decode_until stops at most two blocks after its last row has retired)."""
        return int(self._L.rwkv_mi_batch_last_loop_passes(self._ptr))

    def free(self) -> None:
        if self._ptr:
            session = getattr(self, "_session", None)
            if session is not None:
                session._ptr = None   # (rwkv_mi_batch_free closes it)
                self._session = None
            self._L.rwkv_mi_batch_free(self._ptr)
            self._ptr = None

    def __del__(self) -> None:
        if getattr(self, "_ptr", None):
            self.free()
