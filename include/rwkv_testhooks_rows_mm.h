/* rwkv_testhooks_rows_mm.h -- entry point of lib/librwkv_testhooks_rows_mm.so, for tests/ ONLY. That library is librwkv_testhooks.so (every
 * entry point of rwkv_testhooks.h, rwkv_mi_test_mul_mat among them) plus the one below; librwkv.so and librwkv_testhooks.so do not export it. */
#ifndef RWKV_TESTHOOKS_ROWS_MM_H
#define RWKV_TESTHOOKS_ROWS_MM_H

#include "rwkv_testhooks.h"

#if defined(__cplusplus)
extern "C" {
#endif

/* Test hook (used by tests/ only): launches of k_mmq_rows, the quantised product for 2 .. 31 tokens on the matrix cores (csrc/rows_mm.hip),
 * by this process through this library so far. RWKV_MI_ROWS_MM=tn keeps it at zero. */
RWKV_API uint64_t rwkv_mi_test_mmq_rows_launches(void);

#if defined(__cplusplus)
}
#endif

#endif
