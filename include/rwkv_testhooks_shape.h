/* rwkv_testhooks_shape.h -- the shaping sampler's entry point for tests/ ONLY, in a library of its own: lib/librwkv_testhooks_shape.so (the
 * product objects + csrc/testhooks_shape.cpp). The surfaces of the other hook libraries are pinned by their tests; librwkv.so exports no test
 * entry point. */
#ifndef RWKV_TESTHOOKS_SHAPE_H
#define RWKV_TESTHOOKS_SHAPE_H

#include "rwkv.h"
#include "rwkv_mi355x.h"

#if defined(__cplusplus)
extern "C" {
#endif

/* one row's settings: the two words of rwkv_mi_batch_truncation_set and the two of rwkv_mi_batch_shaping_set; {0, 0, 0, 0} is none */
struct rwkv_mi_test_shape { uint32_t top_k; float min_p; float typical_p; float n_sigma; };

/* Test hook (used by tests/ only): the plain sampler with a truncation and a shaping setting per row on caller-supplied logits
 * [n_rows][n_vocab]. Row r draws with params[r], shapes[r] and counters[r] ([n_rows] in / out; NULL: zero, not returned). rows_kernel != 0:
 * k_draw_rows<plain, 1, 0> in ONE launch with the settings as its row table; 0: row after row, each with its settings by value
 * (k_draw<plain, 1>; k_draw<plain, 0> where they are all 0). tokens_out: [n_rows]. weights_out ([n_rows][n_vocab], or NULL): the vector the
 * draw ran over -- the body's scratch after the draw, copied out in TOKEN order (the kernel keeps it transposed): the unnormalised weight
 * of every token, 0 where a stage or a threshold cut it. */
RWKV_API bool rwkv_mi_test_shape_rows(const float * logits, int64_t n_rows, int64_t n_vocab, const struct rwkv_mi_sample_params * params,
                                      const struct rwkv_mi_test_shape * shapes, uint64_t * counters, int rows_kernel, uint32_t * tokens_out,
                                      float * weights_out);

#if defined(__cplusplus)
}
#endif

#endif
