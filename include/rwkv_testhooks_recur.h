/* rwkv_testhooks_recur.h -- the launchers of the RWKV-5 / 6 / 7 recurrences, the group norm and the RWKV-7 key preparation for tests/ ONLY, in
 * a library of its own: lib/librwkv_testhooks_recur.so (the product objects + csrc/testhooks_recur.cpp). The model-level tests can only have
 * head sizes that divide an embedding width the projections accept; the kernels take any head size S. The surfaces of the other hook libraries
 * are pinned by their tests; librwkv.so exports no test entry point.
 *
 * Every array is the caller's, on the host. A hook returns false with the last error set (RWKV_ERROR_ARGS) on bad arguments and launches
 * nothing. */
#ifndef RWKV_TESTHOOKS_RECUR_H
#define RWKV_TESTHOOKS_RECUR_H

#include "rwkv.h"

#if defined(__cplusplus)
extern "C" {
#endif

/* Where the states of a launch_wkv6 / launch_wkv7 call are, and which form of StateRef it takes. state_in: [n_slots][H*S*S], only read;
 * state_out: [n_slots][H*S*S] in / out -- the caller prefills it, the hook uploads it, launches, and returns it, so a slot the call does not
 * name comes back as it went in. On the device both buffers sit behind 2*H*S floats that the StateRef skips with its offset, as a layer's WKV
 * state sits behind its two token-shift rows.
 *   form 0, sequence   n == 1: tokens [0, T) of one sequence on slot slots[0]                      (k_wkvX)
 *   form 1, rows       n == T: row t is its own sequence on slot slots[t], a RowState table        (k_wkvX_rows)
 *   form 2, segments   n segments: tokens [t0[i], t1[i]) on slot slots[i], a SegState table        (k_wkvX_segs)
 * Slots are distinct and below n_slots; segments are not empty, lie in [0, T) and do not overlap. t0 / t1 are read in form 2 only. */
struct rwkv_mi_test_recur_states {
    const float * state_in; float * state_out; int64_t n_slots;
    int form; int64_t n; const uint32_t * slots; const int32_t * t0; const int32_t * t1;
};

/* launch_wkv6 (RWKV-5 / 6). r, k, v: [T][H*S]; u: [H] (u_per_chan 0) or [H*S]; w: [H] (w_mode 0), [H*S] (1) or [T][H*S] (2);
 * out: [T][H*S] in / out (a token no segment covers comes back as it went in). */
RWKV_API bool rwkv_mi_test_wkv6(const float * r, const float * k, const float * v, const float * u, int u_per_chan, const float * w, int w_mode,
                                const struct rwkv_mi_test_recur_states * states, float * out, int64_t T, int64_t H, int64_t S);

/* launch_wkv7. r, w, k, v, a, b: [T][H*S]; out as above. */
RWKV_API bool rwkv_mi_test_wkv7(const float * r, const float * w, const float * k, const float * v, const float * a, const float * b,
                                const struct rwkv_mi_test_recur_states * states, float * out, int64_t T, int64_t H, int64_t S);

/* launch_wkv6_seq / launch_wkv7_seq, the lane-pipelined sequence forms: one sequence of T tokens, state_in -> state_out ([H*S*S] each).
 * They exist for S == 64 and the engine takes them from 32 tokens on: any other S, or T < 32, is refused. */
RWKV_API bool rwkv_mi_test_wkv6_seq(const float * r, const float * k, const float * v, const float * u, int u_per_chan, const float * w, int w_mode,
                                    const float * state_in, float * state_out, float * out, int64_t T, int64_t H, int64_t S);
RWKV_API bool rwkv_mi_test_wkv7_seq(const float * r, const float * w, const float * k, const float * v, const float * a, const float * b,
                                    const float * state_in, float * state_out, float * out, int64_t T, int64_t H, int64_t S);

/* launch_groupnorm, in place on x [T][H*S]. lw, lb: [H*S]. gate: [T][H*S] or NULL. v7_k, v7_r, v7_v: [T][H*S] and v7_rk: [H*S], all four or
 * none (the RWKV-7 bonus). */
RWKV_API bool rwkv_mi_test_groupnorm(float * x, const float * lw, const float * lb, float eps, const float * gate, const float * v7_k,
                                     const float * v7_r, const float * v7_v, const float * v7_rk, int64_t T, int64_t H, int64_t S);

/* launch_v7_kprep. k, a: [T][H*S]; k_k, k_a: [H*S]; k_out, neg_kk, kk_a: [T][H*S], written. */
RWKV_API bool rwkv_mi_test_v7_kprep(const float * k, const float * a, const float * k_k, const float * k_a, float * k_out, float * neg_kk,
                                    float * kk_a, int64_t T, int64_t H, int64_t S);

#if defined(__cplusplus)
}
#endif

#endif
