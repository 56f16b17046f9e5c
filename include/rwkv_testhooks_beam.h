/*
 * rwkv_testhooks_beam.h -- the beam step's entry point for tests/ ONLY, exported by lib/librwkv_testhooks_sample.so (never by librwkv.so):
 * k_beam_rows and k_beam_select (score.hip), the two kernels of one step of rwkv_mi_batch_decode_beam, on caller-supplied logits, scores and
 * finished words, without a model.
 */
#ifndef RWKV_TESTHOOKS_BEAM_H
#define RWKV_TESTHOOKS_BEAM_H

#include "rwkv.h"

#if defined(__cplusplus)
extern "C" {
#endif

/* logits: [groups * width][n_vocab]; scores_in (double) and finished_in: [groups * width]; 1 <= width <= RWKV_MI_TOP_MAX and <= n_vocab;
 * end_tokens: n_end <= 8 ids < n_vocab (NULL when n_end is 0). Row g * width + j of the outputs is hypothesis j of group g after the step:
 * tokens_out (RWKV_MI_NO_TOKEN: none), parents_out (the index within the group), logprobs_out (0 where there is no token), scores_out (double),
 * finished_out. Each output may be NULL. */
RWKV_API bool rwkv_test_beam_step(const float * logits, int64_t groups, int64_t n_vocab, const double * scores_in, const uint32_t * finished_in,
                                  uint32_t width, const uint32_t * end_tokens, uint32_t n_end, uint32_t * tokens_out, uint32_t * parents_out,
                                  float * logprobs_out, double * scores_out, uint32_t * finished_out);

#if defined(__cplusplus)
}
#endif

#endif
