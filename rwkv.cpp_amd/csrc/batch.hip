// batch.hip -- the row kernels of batched decode: T rows of one pass are T DIFFERENT sequences, each with its own recurrent state.
//
// The per-op Runner (engine.hip) runs T rows through every layer; its products and elementwise kernels already treat every row on its own.
// What ties the rows of a sequence together is the token-shift carry (k_mix: row t reads row t-1) and the WKV state carried across rows
// (k_wkv4 / k_wkv6 / k_wkv7). Here each row reads its carry and its state from its own slot and writes its own slot back: a table of
// {in, out} base pointers per row (RowState, device memory) plus the offset of the state component inside the slot.
//
// Exactness: every kernel below performs the statements of the T = 1 iteration of its single-token counterpart in kernels.hip, in the same
// order, compiled with the same -ffp-contract=off. A row therefore equals one single-token step of its sequence bit for bit.
#include "kdev.h"

namespace rwkvmi {

// ---------------------------------------------------------------------------------------------------------------
// Token-shift mix: k_mix with x_prev = carry_in(row)[d] and carry_out(row)[d] = x (every row is the last row of its sequence).
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mix_rows(MixArgs a, const RowState * __restrict__ rows, int64_t co, int64_t T, int64_t D) {
    const int64_t n = T * D;
    for (int64_t idx = (int64_t) blockIdx.x * 256 + threadIdx.x; idx < n; idx += (int64_t) gridDim.x * 256) {
        const int64_t t = idx / D, d = idx - t * D;
        const float x = a.xn[idx];
        const float xp = rows[t].in[co + d];
        if (a.mode == 0) {
            for (int f = 0; f < a.n_out; f++) { const float c = a.coef[f][d]; const float xc = x * c, pc = xp * c; a.out[f][idx] = xc + (xp - pc); }
        } else {
            const float sx = xp - x;
            if (a.sx) a.sx[idx] = sx;
            for (int f = 0; f < a.n_out; f++) { const float sc = sx * a.coef[f][d]; a.out[f][idx] = sc + x; }
        }
        rows[t].out[co + d] = x;
    }
}

void launch_mix_rows(const MixArgs & a, const RowState * rows, int64_t co, int64_t T, int64_t D, hipStream_t st) {
    const int64_t n = T * D;
    const unsigned grid = (unsigned) ((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(k_mix_rows, dim3(grid), dim3(256), 0, st, a, rows, co, T, D);
}

// ---------------------------------------------------------------------------------------------------------------
// RWKV-4: one thread per (channel, row). State of a row at so: aa [so, so + D), bb [so + D, ...), pp [so + 2 D, ...).
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_wkv4_rows(const float * __restrict__ k, const float * __restrict__ v, const float * __restrict__ r,
                                                   const float * __restrict__ tf, const float * __restrict__ td, const RowState * __restrict__ rows,
                                                   int64_t so, float * __restrict__ out, int64_t D) {
    const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
    const int64_t t = blockIdx.y;
    if (i >= D) return;
    const float * sin = rows[t].in + so;
    float * sout = rows[t].out + so;
    float aa = sin[i], bb = sin[D + i], pp = sin[2 * D + i];
    const float u = tf[i], w = td[i];
    const float kk = k[t * D + i], vv = v[t * D + i];
    float ww = u + kk;
    float qq = fmaxf(pp, ww);
    float e1 = det_expf(pp - qq), e2 = det_expf(ww - qq);
    const float a = e1 * aa + e2 * vv;
    const float b = e1 * bb + e2;
    ww = pp + w;
    qq = fmaxf(ww, kk);
    e1 = det_expf(ww - qq); e2 = det_expf(kk - qq);
    aa = e1 * aa + e2 * vv;
    bb = e1 * bb + e2;
    pp = qq;
    out[t * D + i] = r[t * D + i] * (a / b);
    sout[i] = aa; sout[D + i] = bb; sout[2 * D + i] = pp;
}

void launch_wkv4_rows(const float * k, const float * v, const float * r, const float * time_first, const float * time_decay,
                      const RowState * rows, int64_t so, float * out, int64_t T, int64_t D, hipStream_t st) {
    hipLaunchKernelGGL(k_wkv4_rows, dim3((unsigned) ((D + 255) / 256), (unsigned) T), dim3(256), 0, st, k, v, r, time_first, time_decay, rows, so, out, D);
}

// ---------------------------------------------------------------------------------------------------------------
// RWKV-5/6: one wave per (head, row), lane j owns value column j of state[h][:, j] (k_wkv6's layout and order).
// ---------------------------------------------------------------------------------------------------------------
template <int S>
__global__ __launch_bounds__(64) void k_wkv6_rows(const float * __restrict__ r, const float * __restrict__ k, const float * __restrict__ v,
                                                  const float * __restrict__ u, int u_per_chan, const float * __restrict__ w, int w_mode,
                                                  const RowState * __restrict__ rows, int64_t so, float * __restrict__ out, int64_t H) {
    __shared__ float l_r[S], l_k[S], l_u[S], l_w[S];
    const int64_t h = blockIdx.x, t = blockIdx.y;
    const int j = threadIdx.x;
    const int64_t D = H * S;
    const float * state_in = rows[t].in + so;
    float * state_out = rows[t].out + so;
    float s[S];
    if (j < S) {
#pragma unroll
        for (int i = 0; i < S; i++) s[i] = state_in[h * S * S + i * S + j];
    }
    if (j < S) {
        l_u[j] = u_per_chan ? u[h * S + j] : u[h];
        if (w_mode < 2) l_w[j] = (w_mode == 1) ? w[h * S + j] : w[h];
    }
    __syncthreads();
    if (j < S) {
        l_r[j] = r[t * D + h * S + j];
        l_k[j] = k[t * D + h * S + j];
        if (w_mode == 2) l_w[j] = w[t * D + h * S + j];
    }
    __syncthreads();
    if (j < S) {
        const float vj = v[t * D + h * S + j];
        float o = 0.0f;
#pragma unroll
        for (int i = 0; i < S; i++) {
            const float kv = vj * l_k[i];
            const float prev = s[i];
            const float temp = kv * l_u[i] + prev;
            o += temp * l_r[i];
            s[i] = prev * l_w[i] + kv;
        }
        out[t * D + h * S + j] = o;
#pragma unroll
        for (int i = 0; i < S; i++) state_out[h * S * S + i * S + j] = s[i];
    }
}

// head sizes without a template: the state column stays in memory (k_wkv6_generic's order)
__global__ __launch_bounds__(256) void k_wkv6_rows_generic(const float * __restrict__ r, const float * __restrict__ k, const float * __restrict__ v,
                                                           const float * __restrict__ u, int u_per_chan, const float * __restrict__ w, int w_mode,
                                                           const RowState * __restrict__ rows, int64_t so, float * __restrict__ out, int64_t H, int64_t S) {
    const int64_t h = blockIdx.x, t = blockIdx.y;
    const int64_t D = H * S;
    const float * sin = rows[t].in + so;
    float * sout = rows[t].out + so;
    for (int64_t j = threadIdx.x; j < S; j += blockDim.x) {
        const float vj = v[t * D + h * S + j];
        float o = 0.0f;
        for (int64_t i = 0; i < S; i++) {
            const float ki = k[t * D + h * S + i], ri = r[t * D + h * S + i];
            const float ui = u_per_chan ? u[h * S + i] : u[h];
            const float wi = (w_mode == 2) ? w[t * D + h * S + i] : (w_mode == 1 ? w[h * S + i] : w[h]);
            const float kv = vj * ki;
            const float prev = sin[h * S * S + i * S + j];
            const float temp = kv * ui + prev;
            o += temp * ri;
            sout[h * S * S + i * S + j] = prev * wi + kv;
        }
        out[t * D + h * S + j] = o;
    }
}

void launch_wkv6_rows(const float * r, const float * k, const float * v, const float * u, int u_per_chan, const float * w, int w_mode,
                      const RowState * rows, int64_t so, float * out, int64_t T, int64_t H, int64_t S, hipStream_t st) {
    const dim3 grid((unsigned) H, (unsigned) T);
    switch (S) {
        case 64: hipLaunchKernelGGL((k_wkv6_rows<64>), grid, dim3(64), 0, st, r, k, v, u, u_per_chan, w, w_mode, rows, so, out, H); break;
        case 32: hipLaunchKernelGGL((k_wkv6_rows<32>), grid, dim3(64), 0, st, r, k, v, u, u_per_chan, w, w_mode, rows, so, out, H); break;
        case 16: hipLaunchKernelGGL((k_wkv6_rows<16>), grid, dim3(64), 0, st, r, k, v, u, u_per_chan, w, w_mode, rows, so, out, H); break;
        case 8:  hipLaunchKernelGGL((k_wkv6_rows<8>),  grid, dim3(64), 0, st, r, k, v, u, u_per_chan, w, w_mode, rows, so, out, H); break;
        default: hipLaunchKernelGGL(k_wkv6_rows_generic, grid, dim3(256), 0, st, r, k, v, u, u_per_chan, w, w_mode, rows, so, out, H, S); break;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// RWKV-7: one wave per (head, row), lane i owns value row i of state[h][i, :] (k_wkv7's layout and order).
// ---------------------------------------------------------------------------------------------------------------
template <int S>
__global__ __launch_bounds__(64) void k_wkv7_rows(const float * __restrict__ r, const float * __restrict__ w, const float * __restrict__ k,
                                                  const float * __restrict__ v, const float * __restrict__ a, const float * __restrict__ b,
                                                  const RowState * __restrict__ rows, int64_t so, float * __restrict__ out, int64_t H) {
    __shared__ float l_r[S], l_w[S], l_k[S], l_a[S], l_b[S];
    const int64_t h = blockIdx.x, t = blockIdx.y;
    const int i = threadIdx.x;
    const int64_t D = H * S;
    const float * state_in = rows[t].in + so;
    float * state_out = rows[t].out + so;
    float s[S];
    if (i < S) {
#pragma unroll
        for (int j = 0; j < S; j += 4) {
            const float4 q = *reinterpret_cast<const float4 *>(state_in + h * S * S + (int64_t) i * S + j);
            s[j] = q.x; s[j + 1] = q.y; s[j + 2] = q.z; s[j + 3] = q.w;
        }
    }
    if (i < S) {
        const int64_t o = t * D + h * S + i;
        l_r[i] = r[o]; l_w[i] = w[o]; l_k[i] = k[o]; l_a[i] = a[o]; l_b[i] = b[o];
    }
    __syncthreads();
    if (i < S) {
        const float vi = v[t * D + h * S + i];
        float sa = 0.0f;
#pragma unroll
        for (int j = 0; j < S; j++) sa += l_a[j] * s[j];
        float res = 0.0f;
#pragma unroll
        for (int j = 0; j < S; j++) {
            const float kv = vi * l_k[j];
            const float ns = (s[j] * l_w[j] + kv) + sa * l_b[j];
            s[j] = ns;
            res += ns * l_r[j];
        }
        out[t * D + h * S + i] = res;
#pragma unroll
        for (int j = 0; j < S; j += 4)
            *reinterpret_cast<float4 *>(state_out + h * S * S + (int64_t) i * S + j) = make_float4(s[j], s[j + 1], s[j + 2], s[j + 3]);
    }
}

__global__ __launch_bounds__(256) void k_wkv7_rows_generic(const float * __restrict__ r, const float * __restrict__ w, const float * __restrict__ k,
                                                           const float * __restrict__ v, const float * __restrict__ a, const float * __restrict__ b,
                                                           const RowState * __restrict__ rows, int64_t so, float * __restrict__ out, int64_t H, int64_t S) {
    const int64_t h = blockIdx.x, t = blockIdx.y;
    const int64_t D = H * S;
    const float * sin = rows[t].in + so;
    float * sout = rows[t].out + so;
    for (int64_t i = threadIdx.x; i < S; i += blockDim.x) {
        const int64_t base = t * D + h * S;
        const float vi = v[base + i];
        float sa = 0.0f;
        for (int64_t j = 0; j < S; j++) sa += a[base + j] * sin[h * S * S + i * S + j];
        float res = 0.0f;
        for (int64_t j = 0; j < S; j++) {
            const float kv = vi * k[base + j];
            const float ns = (sin[h * S * S + i * S + j] * w[base + j] + kv) + sa * b[base + j];
            sout[h * S * S + i * S + j] = ns;
            res += ns * r[base + j];
        }
        out[base + i] = res;
    }
}

void launch_wkv7_rows(const float * r, const float * w, const float * k, const float * v, const float * a, const float * b,
                      const RowState * rows, int64_t so, float * out, int64_t T, int64_t H, int64_t S, hipStream_t st) {
    const dim3 grid((unsigned) H, (unsigned) T);
    switch (S) {
        case 64: hipLaunchKernelGGL((k_wkv7_rows<64>), grid, dim3(64), 0, st, r, w, k, v, a, b, rows, so, out, H); break;
        case 32: hipLaunchKernelGGL((k_wkv7_rows<32>), grid, dim3(64), 0, st, r, w, k, v, a, b, rows, so, out, H); break;
        default: hipLaunchKernelGGL(k_wkv7_rows_generic, grid, dim3(256), 0, st, r, w, k, v, a, b, rows, so, out, H, S); break;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Greedy pick of every row: one workgroup per row, k_argmax's scan and tie rule (greater value, then smaller index; NaN never wins).
// The token lands in out[row] (where the next step's embedding lookup reads it) and in hist[row] when given.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_argmax_rows(const float * __restrict__ logits_all, int64_t n, uint32_t * __restrict__ out, uint32_t * __restrict__ hist) {
    __shared__ float l_v[16];
    __shared__ int l_i[16];
    const int64_t row = blockIdx.x;
    const float * __restrict__ logits = logits_all + row * n;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    int64_t i = threadIdx.x;
    for (; i + 7 * (int64_t) blockDim.x < n; i += 8 * (int64_t) blockDim.x) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = logits[i + u * (int64_t) blockDim.x];
#pragma unroll
        for (int u = 0; u < 8; u++) if (v[u] > best) { best = v[u]; bi = (int) (i + u * (int64_t) blockDim.x); }
    }
    for (; i < n; i += blockDim.x) {
        const float v = logits[i];
        if (v > best) { best = v; bi = (int) i; }
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
        // (every logit NaN or -inf: the token feeds the next embedding lookup on the device, it must stay a row of the table)
        const uint32_t tok = bi == 0x7fffffff ? 0u : (uint32_t) bi;
        out[row] = tok;
        if (hist) hist[row] = tok;
    }
}

void launch_argmax_rows(const float * logits, int64_t T, int64_t n, uint32_t * out, uint32_t * hist, hipStream_t st) {
    hipLaunchKernelGGL(k_argmax_rows, dim3((unsigned) T), dim3(1024), 0, st, logits, n, out, hist);
}

}  // namespace rwkvmi
