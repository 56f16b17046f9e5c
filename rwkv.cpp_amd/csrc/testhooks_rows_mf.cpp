// testhooks_rows_mf.cpp -- for tests/ ONLY: the launch counter of k_mmf_rows (rows_mf.hip). lib/librwkv_testhooks_rows_mf.so = every product
// object + csrc/testhooks.cpp + this file, so the products and models a test runs through that library are the ones the counter sees.
#include "kernels.h"
#include "rwkv_testhooks_rows_mf.h"

extern "C" {

RWKV_API uint64_t rwkv_mi_test_mmf_rows_launches(void) { return (uint64_t) rwkvmi::g_mmf_rows_launches.load(); }

}  // extern "C"
