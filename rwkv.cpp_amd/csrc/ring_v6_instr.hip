// ring_v6_instr.hip -- the instrumented instantiations of k6_ring (phase stamps, trace stores, the RWKV_MI_RING_DBG timing experiments): the
// same body as the product kernels of ring_v6.hip, compiled with INS = true, in a translation unit of its own so that `make -j` builds
// the two halves side by side. The host launches these exactly when a trace slot is bound (rwkv_mi_trace_phases) or RWKV_MI_RING_DBG is
// non-zero (RingV6::forward_range); results are bit-identical to the product kernels'.
#define R6_INSTR_TU 1
#include "ring_v6.hip"
