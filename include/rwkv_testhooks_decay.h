/* rwkv_testhooks_decay.h -- the entry points of the penalised sampler with a repetition setting for tests/ ONLY, in a library of its own:
 * lib/librwkv_testhooks_decay.so (the product objects + csrc/testhooks_decay.cpp). The surfaces of the other hook libraries are pinned by their
 * tests; librwkv.so exports no test entry point. */
#ifndef RWKV_TESTHOOKS_DECAY_H
#define RWKV_TESTHOOKS_DECAY_H

#include "rwkv.h"
#include "rwkv_mi355x.h"

#if defined(__cplusplus)
extern "C" {
#endif

/* one row's repetition setting, the two words of rwkv_mi_batch_repetition_set: {1, 1} is none */
struct rwkv_mi_test_rep { float decay; float repetition; };

/* Test hook (used by tests/ only): the penalised sampler with a repetition setting per row on caller-supplied logits [n_rows][n_vocab]. Row r
 * draws with params[r], penalties[r] (record included), reps[r] and counters[r] ([n_rows] in / out; NULL: zero, not returned) on the occurrence
 * row occ[r] ([n_rows][n_vocab] 4-byte words in / out: floats where reps[r].decay != 1, uint32 counts elsewhere) and bias[r] ([n_rows][n_vocab];
 * NULL: no row has a bias). rows_kernel != 0: k_draw_rows<rep, 1, 0> in ONE launch with the settings as its table, a row with {1, 1} included;
 * 0: row after row, each with its setting by value (k_draw<rep, 1>; k_draw<pen, 0> where it is {1, 1}). tokens_out: [n_rows]. */
RWKV_API bool rwkv_mi_test_decay_rows(const float * logits, int64_t n_rows, int64_t n_vocab, const struct rwkv_mi_sample_params * params,
                                      const struct rwkv_mi_penalty_params * penalties, const struct rwkv_mi_test_rep * reps, uint32_t * occ,
                                      const float * bias, uint64_t * counters, int rows_kernel, uint32_t * tokens_out);

/* Test hook (used by tests/ only): k_count_add_decay, what rwkv_mi_*counts_add launches on a decaying sequence, on a caller-supplied row occ
 * ([n_vocab] floats in / out): per token of the list, in its order, every entry * decay, then the token's entry + 1.0f. */
RWKV_API bool rwkv_mi_test_decay_counts_add(float * occ, int64_t n_vocab, const uint32_t * tokens, int64_t n_tokens, float decay);

#if defined(__cplusplus)
}
#endif

#endif
