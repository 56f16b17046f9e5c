/* rwkv_testhooks_rows_mf.h -- entry point of lib/librwkv_testhooks_rows_mf.so, for tests/ ONLY. That library is librwkv_testhooks.so (every
 * entry point of rwkv_testhooks.h, rwkv_mi_test_mul_mat among them) plus the one below; librwkv.so and librwkv_testhooks.so do not export it. */
#ifndef RWKV_TESTHOOKS_ROWS_MF_H
#define RWKV_TESTHOOKS_ROWS_MF_H

#include "rwkv_testhooks.h"

#if defined(__cplusplus)
extern "C" {
#endif

/* Test hook (used by tests/ only): launches of k_mmf_rows, the F16 / F32 product for 5 .. 31 tokens on the matrix cores (csrc/rows_mf.hip),
 * by this process through this library so far. RWKV_MI_ROWS_MF=valu keeps it at zero. */
RWKV_API uint64_t rwkv_mi_test_mmf_rows_launches(void);

#if defined(__cplusplus)
}
#endif

#endif
