// testhooks_rows_q.cpp -- for tests/ ONLY: the launch counters of the quantising row producers (rows_q.hip) and of the stand-alone activation
// quantiser (matvec.hip). lib/librwkv_testhooks_rows_q.so = every product object + csrc/testhooks.cpp + this file, so the models a test runs
// through that library are the ones the counters see.
#include "kernels.h"
#include "rwkv_testhooks_rows_q.h"

extern "C" {

RWKV_API uint64_t rwkv_mi_test_quant_act_launches(void) { return (uint64_t) rwkvmi::g_quant_act_launches.load(); }
RWKV_API uint64_t rwkv_mi_test_rows_q_launches(void) { return (uint64_t) rwkvmi::g_rows_q_launches.load(); }

}  // extern "C"
