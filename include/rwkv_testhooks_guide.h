/* rwkv_testhooks_guide.h -- the guided sampler's entry point for tests/ ONLY, in a library of its own: lib/librwkv_testhooks_guide.so (the
 * product objects + csrc/testhooks_guide.cpp). The surface of librwkv_testhooks.so is pinned (tests/test_cpu_library.py: exactly the entry
 * points of rwkv_testhooks.h); librwkv.so exports no test entry point. */
#ifndef RWKV_TESTHOOKS_GUIDE_H
#define RWKV_TESTHOOKS_GUIDE_H

#include "rwkv.h"
#include "rwkv_mi355x.h"

#if defined(__cplusplus)
extern "C" {
#endif

/* Test hook (used by tests/ only): k_draw_rows<plain, 1, 1> (penalties == NULL) or k_draw_rows<pen, 1, 1> in ONE launch on caller-supplied logits
 * [n_rows][n_vocab], after k_guide_expand has built the tables of n_guides guides. Guide g has n_states[g] states; the guides' edges are given
 * back to back in the CSR form of rwkv_mi_batch_guide_create: edge_begin holds sum(n_states[g] + 1) words, each guide's own run starting at 0,
 * edge_tokens / edge_next the edges of guide 0, then guide 1, ... . Row r draws with params[r] and counters[r] ([n_rows] in / out; NULL: zero,
 * not returned) on guide row_guide[r] (RWKV_MI_NO_GUIDE: none) from state row_state[r]; penalised, with penalties[r] on counts[r] ([n_rows][n_vocab]
 * in / out) and bias[r] ([n_rows][n_vocab]; NULL: no row has a bias). tokens_out, states_out, misses_out: [n_rows]; a row's miss counter starts
 * from 0, a row without a guide returns its row_state and 0. */
RWKV_API bool rwkv_mi_test_guided_rows(const float * logits, int64_t n_rows, int64_t n_vocab, uint32_t n_guides, const uint32_t * n_states,
                                       const uint32_t * edge_begin, const uint32_t * edge_tokens, const uint32_t * edge_next,
                                       const uint32_t * row_guide, const uint32_t * row_state, const struct rwkv_mi_sample_params * params,
                                       const struct rwkv_mi_penalty_params * penalties, uint32_t * counts, const float * bias, uint64_t * counters,
                                       uint32_t * tokens_out, uint32_t * states_out, uint32_t * misses_out);

#if defined(__cplusplus)
}
#endif

#endif
