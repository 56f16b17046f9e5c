// kernels.hip -- hand-written gfx950 (CDNA4, wave64) kernels of the RWKV hot path: embedding + ln0, the layer norms, the elementwise
// helpers, argmax and the two load-time kernels. The matrix products and their dispatch are matvec.hip, the recurrences recur.hip; the
// launchers of all three are declared in kernels.h.
//
// Numerics contract of the three files (DESIGN.md "Numerics"):
//  * Projections with quantised weights follow ggml's CPU mul_mat: activations are quantised per
//    32-element block to int8 (d = amax/127 stored fp16-rounded), the dot is an exact integer dot (v_dot4_i32_i8),
//    and blocks are accumulated in f32:  acc = fma(d_w*d_x, isum, acc) [+ fma(m_w, s_x, acc)].
//  * Lane l of the wave that owns an output row accumulates blocks l, l+64, l+128, ... in that order; the 64 partials
//    are folded by an xor-butterfly (32,16,8,4,2,1). The single-token kernel and the token-tiled (sequence) kernel use
//    the SAME order, so rwkv_eval_sequence is bit-identical to repeated rwkv_eval (reference test
//    tests/test_eval_sequence_in_chunks.c:54 checks this with memcmp).
//  * F16 weights: activations are rounded to fp16 first (what ggml does), products/accumulation in f32.
//  * Norm statistics are accumulated in double (ggml_norm), with a fixed reduction tree.
//  * Everything outside the dot products is ONE ROUNDING PER ggml GRAPH OP (the reference evaluates mul, add, sub ...
//    as separate graph nodes), so these files are compiled with -ffp-contract=off and fused multiply-adds appear only as
//    explicit fmaf() inside dot products. exp / tanh are the deterministic double-precision routines of kdev.h. Together
//    with the fixed reduction orders this makes the GPU results bit-identical to the CPU oracle (oracle/rwkv_oracle.c),
//    which the tests assert with array_equal.
#include "kdev.h"

namespace rwkvmi {

// ---------------------------------------------------------------------------------------------------------------
// Embedding gather + LayerNorm, LayerNorm. One 256-thread block per token; the row lives in LDS.
// ---------------------------------------------------------------------------------------------------------------

struct EmbView {
    int type;
    const void * data;
    const uint8_t * qs;
    const uint32_t * qh;
    const void * sc;
    int64_t rows;      // n_vocab: a token id that comes from device memory (on-device argmax / sampling, a pipeline's feedback) is clamped to it
};

__device__ __forceinline__ float emb_elem(const EmbView & e, int64_t row, int64_t D, int64_t k) {
    switch (e.type) {
        case T_F32: return reinterpret_cast<const float *>(e.data)[row * D + k];
        case T_F16: return h2f_bits(reinterpret_cast<const uint16_t *>(e.data)[row * D + k]);
        default: break;
    }
    // quantised embedding (never produced by the reference quantiser, supported for completeness)
    const int64_t blk = row * (D / 32) + k / 32;
    const int j = (int)(k & 31);
    float d, m = 0.0f;
    int code;
    if (e.type == T_Q8_0) {
        code = reinterpret_cast<const int8_t *>(e.qs)[blk * 32 + j];
        d = h2f_bits(reinterpret_cast<const uint16_t *>(e.sc)[blk]);
        return code * d;
    }
    const uint8_t byte = e.qs[blk * 16 + (j & 15)];
    code = (j < 16) ? (byte & 0x0F) : (byte >> 4);
    if (e.type == T_Q5_0 || e.type == T_Q5_1) code |= (int)((e.qh[blk] >> j) & 1u) << 4;
    if (e.type == T_Q4_1 || e.type == T_Q5_1) {
        const uint32_t dm = reinterpret_cast<const uint32_t *>(e.sc)[blk];
        d = h2f_bits((uint16_t)(dm & 0xFFFF)); m = h2f_bits((uint16_t)(dm >> 16));
        return code * d + m;
    }
    d = h2f_bits(reinterpret_cast<const uint16_t *>(e.sc)[blk]);
    return (code - (e.type == T_Q4_0 ? 8 : 16)) * d;
}

// normalises the row held in l_row (D floats): ((x - mean) * scale) * w + b, one rounding per step, written to out
__device__ __forceinline__ void block_layernorm(float * l_row, int64_t D, const float * __restrict__ w, const float * __restrict__ b,
                                                float eps, float * __restrict__ out, double * red) {
    double s = 0.0;
    s = ln_partial_sum(l_row, D);
    const float mean = (float)(block_sum_d(s, red) / (double) D);
    double s2 = 0.0;
    s2 = ln_partial_var(l_row, D, mean);
    const float var = (float)(block_sum_d(s2, red) / (double) D);
    const float scale = 1.0f / sqrtf(var + eps);
    int64_t i = threadIdx.x;
    for (; i + 3 * 256 < D; i += 4 * 256) {
        float wv[4], bv[4];
#pragma unroll
        for (int u = 0; u < 4; u++) { wv[u] = w[i + u * 256]; bv[u] = b[i + u * 256]; }
#pragma unroll
        for (int u = 0; u < 4; u++) { const float y = l_row[i + u * 256] * scale; const float yw = y * wv[u]; out[i + u * 256] = yw + bv[u]; }
    }
    for (; i < D; i += 256) { const float y = l_row[i] * scale; const float yw = y * w[i]; out[i] = yw + b[i]; }
}

__global__ __launch_bounds__(256) void k_embed_ln0(EmbView emb, const uint32_t * __restrict__ tokens, int64_t D,
                                                   const float * __restrict__ w, const float * __restrict__ b, float * __restrict__ x) {
    extern __shared__ __attribute__((aligned(16))) float l_row[];
    __shared__ double red[257];
    const int64_t t = blockIdx.x;
    const int64_t tok = tokens[t];
    const int64_t row = tok < emb.rows ? tok : 0;     // (host-side token ids are range-checked by the API; this guards device-side ones)
    int64_t i = threadIdx.x;
    if (emb.type == T_F16 || emb.type == T_F32) {
        for (; i + 3 * 256 < D; i += 4 * 256) {   // 4 loads in flight per trip
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) v[u] = emb_elem(emb, row, D, i + u * 256);
#pragma unroll
            for (int u = 0; u < 4; u++) l_row[i + u * 256] = v[u];
        }
    }
    for (; i < D; i += 256) l_row[i] = emb_elem(emb, row, D, i);
    __syncthreads();
    block_layernorm(l_row, D, w, b, 1e-5f, x + t * D, red);
}

__global__ __launch_bounds__(256) void k_layernorm(const float * __restrict__ x, int64_t D, const float * __restrict__ w,
                                                   const float * __restrict__ b, float * __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) float l_row[];
    __shared__ double red[257];
    const int64_t t = blockIdx.x;
    int64_t i = threadIdx.x;
    for (; i + 3 * 256 < D; i += 4 * 256) {   // 4 loads in flight per trip
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) v[u] = x[t * D + i + u * 256];
#pragma unroll
        for (int u = 0; u < 4; u++) l_row[i + u * 256] = v[u];
    }
    for (; i < D; i += 256) l_row[i] = x[t * D + i];
    __syncthreads();
    block_layernorm(l_row, D, w, b, 1e-5f, y + t * D, red);
}

// n gathered rows of x (ragged pass: the last token of each segment): row idx[i] -> y[i]
__global__ __launch_bounds__(256) void k_layernorm_gather(const float * __restrict__ x, const int32_t * __restrict__ idx, int64_t D,
                                                          const float * __restrict__ w, const float * __restrict__ b, float * __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) float l_row[];
    __shared__ double red[257];
    const int64_t t = idx[blockIdx.x];
    for (int64_t i = threadIdx.x; i < D; i += 256) l_row[i] = x[t * D + i];
    __syncthreads();
    block_layernorm(l_row, D, w, b, 1e-5f, y + (int64_t) blockIdx.x * D, red);
}

void launch_embed_ln0(const DevTensor & emb, const uint32_t * tokens, int64_t T, int64_t D, const float * w, const float * b, float * x, hipStream_t st) {
    EmbView e{emb.type, emb.data, emb.qs, emb.qh, emb.sc, emb.rows()};
    hipLaunchKernelGGL(k_embed_ln0, dim3((unsigned) T), dim3(256), (size_t) D * sizeof(float), st, e, tokens, D, w, b, x);
}

void launch_layernorm(const float * x, int64_t T, int64_t D, const float * w, const float * b, float * y, hipStream_t st) {
    hipLaunchKernelGGL(k_layernorm, dim3((unsigned) T), dim3(256), (size_t) D * sizeof(float), st, x, D, w, b, y);
}

void launch_layernorm_gather(const float * x, const int32_t * idx, int64_t n, int64_t D, const float * w, const float * b, float * y, hipStream_t st) {
    hipLaunchKernelGGL(k_layernorm_gather, dim3((unsigned) n), dim3(256), (size_t) D * sizeof(float), st, x, idx, D, w, b, y);
}

// ---------------------------------------------------------------------------------------------------------------
// Small elementwise kernels, argmax, the load-time transpose
// ---------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_mul(float * __restrict__ y, const float * __restrict__ a, const float * __restrict__ b, int64_t n) {
    for (int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t) gridDim.x * 256) y[i] = a[i] * b[i];
}
void launch_mul(float * y, const float * a, const float * b, int64_t n, hipStream_t st) {
    const unsigned grid = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(k_mul, dim3(grid), dim3(256), 0, st, y, a, b, n);
}

__global__ __launch_bounds__(256) void k_copy(float * __restrict__ dst, const float * __restrict__ src, int64_t n) {
    for (int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t) gridDim.x * 256) dst[i] = src[i];
}
void launch_copy_f32(float * dst, const float * src, int64_t n, hipStream_t st) {
    const unsigned grid = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(k_copy, dim3(grid), dim3(256), 0, st, dst, src, n);
}

__global__ __launch_bounds__(256) void k_fill_state_v4(float * __restrict__ state, int64_t n_layer, int64_t D) {
    const int64_t n = n_layer * 5 * D;
    for (int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t) gridDim.x * 256) state[i] = ((i / D) % 5 == 4) ? -1e30f : 0.0f;
}
void launch_fill_state_v4(float * state, int64_t n_layer, int64_t D, hipStream_t st) {
    const int64_t n = n_layer * 5 * D;
    const unsigned grid = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(k_fill_state_v4, dim3(grid), dim3(256), 0, st, state, n_layer, D);
}

// one workgroup per row of logits[rows][n]
__device__ __forceinline__ void argmax_row(const float * __restrict__ logits_all, int64_t n, uint32_t * __restrict__ out, uint32_t * __restrict__ hist) {
    __shared__ float l_v[16];
    __shared__ int l_i[16];
    const int64_t row = blockIdx.x;
    const float * __restrict__ logits = logits_all + row * n;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    int64_t i = threadIdx.x;
    for (; i + 7 * (int64_t) blockDim.x < n; i += 8 * (int64_t) blockDim.x) {   // 8 loads in flight per trip
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = logits[i + u * (int64_t) blockDim.x];
#pragma unroll
        for (int u = 0; u < 8; u++) if (v[u] > best) { best = v[u]; bi = (int) (i + u * (int64_t) blockDim.x); }
    }
    for (; i < n; i += blockDim.x) {
        const float v = logits[i];
        if (v > best) { best = v; bi = (int) i; }  // strided scan keeps the smallest index per thread for ties
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
        for (int w = 1; w < (int)(blockDim.x >> 6); w++)
            if (l_v[w] > best || (l_v[w] == best && l_i[w] < bi)) { best = l_v[w]; bi = l_i[w]; }
        // (no element compared greater than -inf: every logit is NaN or -inf, e.g. after a poll time-out of the persistent kernel on a
        //  shared GPU. The token feeds the next embedding lookup on the device: it must stay a row of the table.)
        const uint32_t tok = bi == 0x7fffffff ? 0u : (uint32_t) bi;
        out[row] = tok;
        if (hist) hist[row] = tok;
    }
}
__global__ __launch_bounds__(1024) void k_argmax(const float * __restrict__ logits_all, int64_t n, uint32_t * __restrict__ out, uint32_t * __restrict__ hist) {
    argmax_row(logits_all, n, out, hist);
}
// the same row behind its live word (rwkv_mi_batch_decode_until, greedy): a retired row reads no logit and writes no token
__global__ __launch_bounds__(1024) void k_argmax_live(const float * __restrict__ logits_all, int64_t n, uint32_t * __restrict__ out, uint32_t * __restrict__ hist,
                                                      const uint32_t * __restrict__ live) {
    if (!live[blockIdx.x]) return;
    argmax_row(logits_all, n, out, hist);
}
void launch_argmax(const float * logits, int64_t rows, int64_t n, uint32_t * out, uint32_t * hist, hipStream_t st) {
    hipLaunchKernelGGL(k_argmax, dim3((unsigned) rows), dim3(1024), 0, st, logits, n, out, hist);
}
void launch_argmax_live(const float * logits, int64_t rows, int64_t n, uint32_t * out, uint32_t * hist, const uint32_t * live, hipStream_t st) {
    hipLaunchKernelGGL(k_argmax_live, dim3((unsigned) rows), dim3(1024), 0, st, logits, n, out, hist, live);
}

// load-time transpose of the v6 mix matrix: [5][D][R] (file) -> [5][R][D], so that lanes read consecutive d
__global__ __launch_bounds__(256) void k_transpose_w2(const float * __restrict__ src, float * __restrict__ dst, int64_t D, int64_t R) {
    const int64_t n = 5 * D * R;
    for (int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t) gridDim.x * 256) {
        const int64_t d = i % D, m = (i / D) % R, f = i / (D * R);
        dst[i] = src[(f * D + d) * R + m];
    }
}
void launch_transpose_w2(const float * src, float * dst, int64_t D, int64_t R, hipStream_t st) {
    hipLaunchKernelGGL(k_transpose_w2, dim3(1024), dim3(256), 0, st, src, dst, D, R);
}

// ---------------------------------------------------------------------------------------------------------------
// Load-time re-pack: file blocks (d [m] [qh] qs) -> planes. One thread per block.
// ---------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_repack(int type, const uint8_t * __restrict__ raw, int64_t n_blocks, uint8_t * __restrict__ qs,
                                                uint32_t * __restrict__ qh, uint8_t * __restrict__ sc) {
    const int64_t b = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (b >= n_blocks) return;
    int bsz, qoff, qbytes, scb, hoff = -1;
    switch (type) {
        case T_Q4_0: bsz = 18; scb = 2; qoff = 2; qbytes = 16; break;
        case T_Q4_1: bsz = 20; scb = 4; qoff = 4; qbytes = 16; break;
        case T_Q5_0: bsz = 22; scb = 2; hoff = 2; qoff = 6; qbytes = 16; break;
        case T_Q5_1: bsz = 24; scb = 4; hoff = 4; qoff = 8; qbytes = 16; break;
        default:     bsz = 34; scb = 2; qoff = 2; qbytes = 32; break;  // Q8_0
    }
    const uint8_t * src = raw + b * bsz;
    for (int i = 0; i < scb; i++) sc[b * scb + i] = src[i];
    if (hoff >= 0) qh[b] = (uint32_t) src[hoff] | ((uint32_t) src[hoff + 1] << 8) | ((uint32_t) src[hoff + 2] << 16) | ((uint32_t) src[hoff + 3] << 24);
    for (int i = 0; i < qbytes; i++) qs[b * qbytes + i] = src[qoff + i];
}

void launch_repack(int type, const uint8_t * raw, int64_t n_blocks, uint8_t * qs, uint32_t * qh, void * sc, hipStream_t st) {
    hipLaunchKernelGGL(k_repack, dim3((unsigned)((n_blocks + 255) / 256)), dim3(256), 0, st, type, raw, n_blocks, qs, qh, (uint8_t *) sc);
}

}  // namespace rwkvmi
