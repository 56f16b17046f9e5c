// score.hip -- per-row log-probability and argmax of a [rows][n_vocab] logits buffer (rwkv_mi_score_resident, rwkv_mi_batch_score_ragged):
// what perplexity and scoring of given text need from the prediction at EVERY position, without shipping n_vocab floats per token to the
// host (the reference's measure_pexplexity.py:71-85 downloads the logits of one rwkv_eval per token and takes the cross entropy there).
// One workgroup of 1024 threads per row:
//   argmax[row]  = index of the largest logit, the lowest index among equals; NaN never wins; 0 when nothing compares greater than -inf
//                  (the rule of k_argmax, kernels.hip, statement by statement);
//   logprob[row] = (float) ((double) l[target] - ((double) m + log(S))),   m = the row maximum (exact),
//                  S = sum_j exp((double) l[j] - (double) m)   in float64, rounded to f32 once at the end.
// The order of the sum is fixed: thread i adds j = i, i + 1024, ... in ascending order into one accumulator, the 64 lanes of a wave are
// combined by the xor butterfly (32, 16, ... 1), the waves in ascending order by every thread; no atomics. A row's results therefore
// depend on its logits and its target alone -- not on the chunk of the head it came in, not on the other rows of the launch, not on the run.
// Shape: the row is read twice (maximum, then sum); it is NOT kept in registers between the two. 64 floats per thread would fit the 128
// registers a 1024-thread workgroup leaves, but only for rows of at most 65536 logits and with the f64 exp's own registers on top; the
// second read of a 256 KB row comes from L2 / the memory-side cache the head product has just written, and the kernel's time is the
// rows * n_vocab float64 exps either way (about 1 % of the head product it follows).
#include "kdev.h"
#include "model.h"

namespace rwkvmi {

__global__ __launch_bounds__(1024) void k_score_rows(const float * __restrict__ logits_all, int n, const uint32_t * __restrict__ targets /* may be NULL */,
                                                     float * __restrict__ logprobs /* may be NULL */, uint32_t * __restrict__ argmax /* may be NULL */) {
    __shared__ float l_v[16];
    __shared__ int l_i[16];
    __shared__ double l_s[16];
    __shared__ float l_m;
    const int64_t row = blockIdx.x;
    const float * __restrict__ logits = logits_all + row * (int64_t) n;
    const int NT = blockDim.x;
    // ---- maximum and its first index (k_argmax) ----
    float best = -INFINITY;
    int bi = 0x7fffffff;
    int i = threadIdx.x;
    for (; i + 7 * NT < n; i += 8 * NT) {   // 8 loads in flight per trip
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = logits[i + u * NT];
#pragma unroll
        for (int u = 0; u < 8; u++) if (v[u] > best) { best = v[u]; bi = i + u * NT; }
    }
    for (; i < n; i += NT) {
        const float v = logits[i];
        if (v > best) { best = v; bi = i; }   // strided scan keeps the smallest index per thread for ties
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, WAVE);
        const int oi = __shfl_xor(bi, o, WAVE);
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { l_v[wave] = best; l_i[wave] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (NT >> 6); w++)
            if (l_v[w] > best || (l_v[w] == best && l_i[w] < bi)) { best = l_v[w]; bi = l_i[w]; }
        l_m = best;
        if (argmax) argmax[row] = bi == 0x7fffffff ? 0u : (uint32_t) bi;
    }
    if (!logprobs) return;
    // ---- log-probability of the target (the branch is uniform over the workgroup) ----
    const uint32_t target = targets ? targets[row] : UINT32_MAX;
    if (target >= (uint32_t) n) {   // RWKV_MI_NO_TARGET (an index behind the row is never read)
        if (threadIdx.x == 0) logprobs[row] = 0.0f;
        return;
    }
    __syncthreads();
    const double m = (double) l_m;
    double acc = 0.0;
    i = threadIdx.x;
    for (; i + 3 * NT < n; i += 4 * NT) {   // 4 loads in flight per trip, added in the order of j
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) v[u] = logits[i + u * NT];
#pragma unroll
        for (int u = 0; u < 4; u++) acc += exp((double) v[u] - m);
    }
    for (; i < n; i += NT) acc += exp((double) logits[i] - m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, WAVE);
    if (lane == 0) l_s[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double S = 0.0;
        for (int w = 0; w < (NT >> 6); w++) S += l_s[w];
        logprobs[row] = (float) ((double) logits[target] - (m + log(S)));
    }
}

void launch_score_rows(const float * logits, int64_t rows, int n, const uint32_t * targets, float * logprobs, uint32_t * argmax, hipStream_t st) {
    if (rows > 0 && (logprobs || argmax)) hipLaunchKernelGGL(k_score_rows, dim3((unsigned) rows), dim3(1024), 0, st, logits, n, targets, logprobs, argmax);
}

}  // namespace rwkvmi
