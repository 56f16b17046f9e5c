/* rwkv_testhooks_rows_q.h -- entry points of lib/librwkv_testhooks_rows_q.so, for tests/ ONLY. That library is librwkv_testhooks.so (every
 * entry point of rwkv_testhooks.h) plus the two below; librwkv.so and librwkv_testhooks.so do not export them. */
#ifndef RWKV_TESTHOOKS_ROWS_Q_H
#define RWKV_TESTHOOKS_ROWS_Q_H

#include "rwkv_testhooks.h"

#if defined(__cplusplus)
extern "C" {
#endif

/* Test hook (used by tests/ only): stand-alone launches of the activation quantiser (launch_quantize_act, csrc/matvec.hip) by this process
 * through this library so far. */
RWKV_API uint64_t rwkv_mi_test_quant_act_launches(void);

/* Test hook (used by tests/ only): launches of the quantising row producers (k_mix_rows_q, k_v6_mix2_rows_q, k_groupnorm_rows_q,
 * csrc/rows_q.hip) by this process through this library so far. RWKV_MI_ROWS_Q=plain keeps it at zero. */
RWKV_API uint64_t rwkv_mi_test_rows_q_launches(void);

#if defined(__cplusplus)
}
#endif

#endif
