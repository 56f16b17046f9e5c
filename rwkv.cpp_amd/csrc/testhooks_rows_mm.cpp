// testhooks_rows_mm.cpp -- for tests/ ONLY: the launch counter of k_mmq_rows (rows_mm.hip). lib/librwkv_testhooks_rows_mm.so = every product
// object + csrc/testhooks.cpp + this file, so the products and models a test runs through that library are the ones the counter sees.
#include "kernels.h"
#include "rwkv_testhooks_rows_mm.h"

extern "C" {

RWKV_API uint64_t rwkv_mi_test_mmq_rows_launches(void) { return (uint64_t) rwkvmi::g_mmq_rows_launches.load(); }

}  // extern "C"
