/* rwkv_testhooks_score.h -- the scoring kernel's entry point for tests/ ONLY. It is compiled into lib/librwkv_testhooks_sample.so with the
 * sampler's hook (csrc/testhooks_sample.cpp); it is declared here because rwkv_testhooks_sample.h is pinned to the sampler's one entry point
 * (tests/test_cpu_batch_sample.py). Neither librwkv.so nor librwkv_testhooks.so exports it. */
#ifndef RWKV_TESTHOOKS_SCORE_H
#define RWKV_TESTHOOKS_SCORE_H

#include "rwkv.h"
#include "rwkv_mi355x.h"

#if defined(__cplusplus)
extern "C" {
#endif

/* Test hook (used by tests/ only): k_score_rows (csrc/score.hip) in one launch on caller-supplied logits [rows][n_vocab]. targets [rows]
 * (an entry of RWKV_MI_NO_TARGET, or any entry >= n_vocab, gives 0), logprobs_out [rows] and argmax_out [rows] may each be NULL. */
RWKV_API bool rwkv_test_score_rows(const float * logits, int64_t rows, int64_t n_vocab, const uint32_t * targets, float * logprobs_out, uint32_t * argmax_out);

#if defined(__cplusplus)
}
#endif

#endif
