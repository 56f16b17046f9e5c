/* rwkv_testhooks_sample.h -- the sampler's entry point for tests/ ONLY, in a library of its own: lib/librwkv_testhooks_sample.so (the
 * product objects + csrc/testhooks_sample.cpp). It is kept out of librwkv_testhooks.so because the surface of that library is pinned
 * (tests/test_cpu_library.py: exactly the entry points of rwkv_testhooks.h); librwkv.so exports neither. */
#ifndef RWKV_TESTHOOKS_SAMPLE_H
#define RWKV_TESTHOOKS_SAMPLE_H

#include "rwkv.h"
#include "rwkv_mi355x.h"

#if defined(__cplusplus)
extern "C" {
#endif

/* Test hook (used by tests/ only): k_draw_rows<plain, 0, 0> in one launch (rows_kernel != 0), or k_draw<plain, 0> row after row (rows_kernel == 0), on
 * caller-supplied logits [n_rows][n_vocab]; counters: [n_rows] in / out (NULL: zero, not returned). */
RWKV_API bool rwkv_mi_test_sample_rows(const float * logits, int64_t n_rows, int64_t n_vocab, const struct rwkv_mi_sample_params * params,
                                       uint64_t * counters, int rows_kernel, uint32_t * tokens_out);

#if defined(__cplusplus)
}
#endif

#endif
