/*
 * rwkv_testhooks_logprobs.h -- the report kernel's entry point for tests/ ONLY, exported by lib/librwkv_testhooks_sample.so (never by
 * librwkv.so): k_logprob_rows (score.hip) on caller-supplied logits, without a model.
 */
#ifndef RWKV_TESTHOOKS_LOGPROBS_H
#define RWKV_TESTHOOKS_LOGPROBS_H

#include "rwkv.h"

#if defined(__cplusplus)
extern "C" {
#endif

/* logits: [rows][n_vocab]; tokens: [rows], the emitted token of each row (< n_vocab); top_n <= RWKV_MI_TOP_MAX and <= n_vocab.
 * chosen_out [rows], top_ids_out / top_logprobs_out [rows][top_n]: each may be NULL. */
RWKV_API bool rwkv_test_logprob_rows(const float * logits, int64_t rows, int64_t n_vocab, const uint32_t * tokens, uint32_t top_n,
                                     float * chosen_out, uint32_t * top_ids_out, float * top_logprobs_out);

#if defined(__cplusplus)
}
#endif

#endif
