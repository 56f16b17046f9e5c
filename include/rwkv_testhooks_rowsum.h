/* rwkv_testhooks_rowsum.h -- the ring kernel's row-sum reductions for tests/ ONLY, exported by lib/librwkv_testhooks_sample.so (never by
 * librwkv.so or librwkv_testhooks.so, whose surfaces are pinned); csrc/testhooks_rowsum.cpp. */
#ifndef RWKV_TESTHOOKS_ROWSUM_H
#define RWKV_TESTHOOKS_ROWSUM_H

#include "rwkv.h"

#if defined(__cplusplus)
extern "C" {
#endif

/* Test hook (used by tests/ only): one wave of 64 lanes runs wave_sum_n<n> (n xor-butterflies: the definition) and wave_sum_scatter<n>
 * (the same trees, every node once) of ring_v6.hip on values[n][64] (value i of lane l at values[i * 64 + l]), n in 1..16.
 * butterfly_out[n][64]: what every lane holds of value i afterwards (the total, in all 64). scatter_out[64]: the one register the scatter
 * returns; value i's total stands in lanes [i * lanes, (i + 1) * lanes), lanes = *lanes_per_value. */
RWKV_API bool rwkv_test_ring_rowsum(int n, const float * values, float * butterfly_out, float * scatter_out, int * lanes_per_value);

#if defined(__cplusplus)
}
#endif

#endif
