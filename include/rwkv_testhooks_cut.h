/* rwkv_testhooks_cut.h -- the truncating sampler's entry point for tests/ ONLY, in a library of its own: lib/librwkv_testhooks_cut.so (the
 * product objects + csrc/testhooks_cut.cpp). The surfaces of the other hook libraries are pinned by their tests; librwkv.so exports no test
 * entry point. */
#ifndef RWKV_TESTHOOKS_CUT_H
#define RWKV_TESTHOOKS_CUT_H

#include "rwkv.h"
#include "rwkv_mi355x.h"

#if defined(__cplusplus)
extern "C" {
#endif

/* one row's truncation setting, the two words of rwkv_mi_batch_truncation_set: {0, 0} is none */
struct rwkv_mi_test_cut { uint32_t top_k; float min_p; };

/* Test hook (used by tests/ only): the plain sampler with a truncation setting per row on caller-supplied logits [n_rows][n_vocab]. Row r
 * draws with params[r], cuts[r] and counters[r] ([n_rows] in / out; NULL: zero, not returned). rows_kernel != 0: k_draw_rows<plain, 1, 0> in ONE launch
 * with the settings as its row table; 0: row after row, each with its setting by value (k_draw<plain, 1>; k_draw<plain, 0> where it is {0, 0}). tokens_out: [n_rows]. weights_out
 * ([n_rows][n_vocab], or NULL): the vector the draw ran over -- the body's scratch after the draw, copied out in TOKEN order (the kernel keeps
 * it transposed): the unnormalised weight of every token, 0 where a truncation cut it. */
RWKV_API bool rwkv_mi_test_cut_rows(const float * logits, int64_t n_rows, int64_t n_vocab, const struct rwkv_mi_sample_params * params,
                                    const struct rwkv_mi_test_cut * cuts, uint64_t * counters, int rows_kernel, uint32_t * tokens_out,
                                    float * weights_out);

#if defined(__cplusplus)
}
#endif

#endif
