// rows_q.hip -- the quantising row and segment forms of the producers whose only consumers are quantised products, for passes below
// k_mfma_min_tokens tokens (batched decode, serve, beam, draft and short ragged passes): the token-shift mix, the RWKV-6 data-dependent mix
// and the RWKV-5 / 6 group norm (+ gate) write the plain QAct of launch_quantize_act (kernels.h: codes, fp16-rounded scale, the code sum, and
// for Q8_1 consumers scale * sum) that k_mmq_rows and k_mvq_* read, instead of an f32 vector for a quantiser launch of its own.
//
// Numerics: the f32 value of an element is made by the statements of the unfused kernel (mix_lerp_*, v6_mix2_elem, groupnorm_elem: kdev.h, shared
// with recur.hip; the group norm keeps k_groupnorm's lane partials and wave_sum_d), the block's statements are k_quant_act's: amax (order-free)
// -> d = amax / 127 -> id = 1 / d -> roundf(v * id) per element -> the integer sum (order-free). So the QAct holds k_quant_act's bits of the
// value the unfused kernel would have stored, and every product behind it its bits of today.
//
// Work split, the mix: one LANE owns one 32-element block of one (token, output) -- the block's x, x_prev and the 32 mixed values live in its
// registers; amax and the sum are loops over its own registers, the codes leave as two 16-byte stores. No
// LDS, no lane exchange, no barrier. Workgroup = one wave = 64 consecutive blocks of (blockIdx.y = output, blockIdx.z = token): the output and
// the token -- and with it the slot or segment the carry comes from -- are uniform in the wave, a wave's loads are contiguous 8 KB runs of the
// token's row, its code stores a contiguous 2 KB run. The lanes of output 0 also write the carry (the row's x into its slot's out buffer) and,
// RWKV-6, sx. The group norm: one wave per (token, head) as k_groupnorm, lane = element; behind the head's statistics the lane's value stays in
// its register and the two half-waves reduce their block's amax and sum (half_max_f / half_sum_i, DPP), as k_quant_act does. The data-dependent
// mix likewise, lane = element as in k_v6_mix2: an element is a walk over R rows of W2 that only lanes on consecutive channels read coalesced
// (a block per lane was measured: 52.7 us per launch at n = 8 on the 7B against 29.8 for k_v6_mix2).
#include "kdev.h"
#include "model.h"

#include <cstdlib>
#include <cstring>

namespace rwkvmi {

std::atomic<unsigned long long> g_rows_q_launches{0};

struct RowsQOut { QAct x[ROWS_Q_BATCH]; bool q81; };   // q81: the consumers read s (Q4_1 / Q5_1 weights)

// k_quant_act's block in one lane: the 32 values v of block blk
__device__ __forceinline__ void quant_block_store(const float (&v)[32], int64_t blk, const QAct & o, bool q81) {
    float amax = 0.0f;
#pragma unroll
    for (int j = 0; j < 32; j++) amax = fmaxf(amax, fabsf(v[j]));
    const float dd = amax / 127.0f;
    const float id = dd != 0.0f ? 1.0f / dd : 0.0f;
    int sum = 0;
    int w8[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        int w = 0;
#pragma unroll
        for (int e = 0; e < 4; e++) { const int qi = (int) roundf(v[4 * j + e] * id); sum += qi; w |= (qi & 0xFF) << (8 * e); }
        w8[j] = w;
    }
    int4 * q = reinterpret_cast<int4 *>(o.q + blk * 32);
    q[0] = make_int4(w8[0], w8[1], w8[2], w8[3]);
    q[1] = make_int4(w8[4], w8[5], w8[6], w8[7]);
    o.d[blk] = round_f16(dd);
    if (q81) o.s[blk] = round_f16((float) sum * dd);
    o.isum[blk] = sum;
}

__device__ __forceinline__ void load32(float (&v)[32], const float * p) {
    const float4 * p4 = reinterpret_cast<const float4 *>(p);
#pragma unroll
    for (int j = 0; j < 8; j++) { const float4 f = p4[j]; v[4 * j] = f.x; v[4 * j + 1] = f.y; v[4 * j + 2] = f.z; v[4 * j + 3] = f.w; }
}
__device__ __forceinline__ void store32(float * p, const float (&v)[32]) {
    float4 * p4 = reinterpret_cast<float4 *>(p);
#pragma unroll
    for (int j = 0; j < 8; j++) p4[j] = make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
}

// ---------------------------------------------------------------------------------------------------------------
// Token-shift mix -> QAct. grid (ceil(nb / 64), n_out, T), nb = D / 32. a.out is not read: nothing but the QActs, the carry and sx is written.
// ---------------------------------------------------------------------------------------------------------------
template <int FORM>
__global__ __launch_bounds__(64) void k_mix_rows_q(MixArgs a, RowsQOut o, int nb, StateRef s) {
    static_assert(FORM == FORM_ROWS || FORM == FORM_SEGS, "a sequence takes k_mix or k_mix_seq_q");
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= nb) return;
    const int f = blockIdx.y;
    const int64_t t = blockIdx.z, D = (int64_t) nb * 32, d0 = (int64_t) b * 32, co = s.off + d0;
    const float * xrow = a.xn + t * D + d0;
    const float * prev;
    float * carry = nullptr;
    if constexpr (FORM == FORM_ROWS) {
        // every row is the last token of its sequence (k_mix, FORM_ROWS)
        prev = s.rows[t].in + co;
        carry = s.rows[t].out + co;
    } else {
        // the segment's first token continues from the slot, its last one leaves the carry there (k_mix, FORM_SEGS)
        const SegState seg = s.segs[s.seg_of[t]];
        prev = t == seg.t0 ? seg.in + co : xrow - D;
        if (t == seg.t1 - 1) carry = seg.out + co;
    }
    float x[32], xp[32], val[32];
    load32(x, xrow);
    load32(xp, prev);
    if (f == 0 && carry) store32(carry, x);
    load32(val, a.coef[f] + d0);
    if (a.mode == 0) {
#pragma unroll
        for (int j = 0; j < 32; j++) val[j] = mix_lerp_v4(x[j], xp[j], val[j]);
    } else {
#pragma unroll
        for (int j = 0; j < 32; j++) { xp[j] = xp[j] - x[j]; val[j] = mix_lerp_v6(x[j], xp[j], val[j]); }
        if (f == 0 && a.sx) store32(a.sx + t * D + d0, xp);
    }
    quant_block_store(val, t * nb + b, o.x[f], o.q81);
}

// ---------------------------------------------------------------------------------------------------------------
// RWKV-6 data-dependent mix -> five QActs. One thread per element (t, f, d) in k_v6_mix2's order; 32 consecutive threads are one block of output f
// (D % 32 == 0), reduced as k_quant_act reduces it. No grid stride: whole waves stay in the reductions.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_v6_mix2_rows_q(V6Mix2Args a, RowsQOut o, int64_t T, int64_t D, int64_t R) {
    const int64_t idx = (int64_t) blockIdx.x * 256 + threadIdx.x;
    const bool live = idx < T * 5 * D;
    const int64_t i = live ? idx : 0;
    const int64_t d = i % D, f = (i / D) % 5, t = i / (5 * D);
    const float v = live ? v6_mix2_elem(a, t, f, d, D, R) : 0.0f;
    const float amax = half_max_f(fabsf(v));
    const float dd = amax / 127.0f;
    const float id = dd != 0.0f ? 1.0f / dd : 0.0f;
    const int qi = (int) roundf(v * id);
    const int sum = half_sum_i(qi);
    if (!live) return;
    const QAct & q = o.x[f];
    const int64_t e = t * D + d;
    q.q[e] = (int8_t) qi;
    if ((threadIdx.x & 31) == 0) {
        q.d[e >> 5] = round_f16(dd);
        if (o.q81) q.s[e >> 5] = round_f16((float) sum * dd);
        q.isum[e >> 5] = sum;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Group norm (+ gate) -> QAct, S % 32 == 0. One wave per (token, head), four per workgroup: k_groupnorm's statements up to the element's value
// (lane l sums elements l, l + 64, ... in double, wave_sum_d), x is only read. In a trip of 64 elements a half-wave is one block, whole or empty.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_groupnorm_rows_q(const float * __restrict__ x, const float * __restrict__ lw, const float * __restrict__ lb, float eps,
                                                          const float * __restrict__ gate, QAct o, bool q81, int64_t TH, int64_t H, int64_t S) {
    const int lane = threadIdx.x & 63;
    const int64_t th = (int64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
    if (th >= TH) return;
    const int64_t h = th % H;
    const int64_t base = th * S;  // == t*D + h*S
    double s = 0.0;
    for (int64_t j = lane; j < S; j += WAVE) s += (double) x[base + j];
    const float mean = (float)(wave_sum_d(s) / (double) S);
    double s2 = 0.0;
    for (int64_t j = lane; j < S; j += WAVE) { const float v = x[base + j] - mean; s2 += (double)(v * v); }
    const float var = (float)(wave_sum_d(s2) / (double) S);
    const float scale = 1.0f / sqrtf(var + eps);
    for (int64_t j0 = 0; j0 < S; j0 += WAVE) {
        const int64_t j = j0 + lane;
        const bool live = j < S;   // (whole waves stay in the reductions below)
        float y = 0.0f;
        if (live) {
            y = groupnorm_elem(x[base + j], mean, scale, lw[h * S + j], lb[h * S + j]);
            if (gate) y *= gate[base + j];
        }
        const float amax = half_max_f(fabsf(y));
        const float dd = amax / 127.0f;
        const float id = dd != 0.0f ? 1.0f / dd : 0.0f;
        const int qi = (int) roundf(y * id);
        const int sum = half_sum_i(qi);
        if (!live) continue;
        o.q[base + j] = (int8_t) qi;
        if ((lane & 31) == 0) {
            const int64_t blk = (base + j) >> 5;
            o.d[blk] = round_f16(dd);
            if (q81) o.s[blk] = round_f16((float) sum * dd);
            o.isum[blk] = sum;
        }
    }
}

// RWKV_MI_ROWS_Q = plain: the unfused producers and k_quant_act for the whole process, as before these kernels (A/B, tests). = nomix2: the same
// for the data-dependent mix alone, the one producer with five outputs (A/B of that kernel by itself). Read once.
static int rows_q_off() {
    static const int off = [] { const char * e = getenv("RWKV_MI_ROWS_Q"); return !e ? 0 : strcmp(e, "plain") == 0 ? 2 : strcmp(e, "nomix2") == 0 ? 1 : 0; }();
    return off;
}

// The gate, whole: a pass of rows or segments below k_mfma_min_tokens tokens whose producer feeds n products of row length K, every one
// quantised and of one activation kind (Q8_1: the weights carry a minimum, the product reads s; Q8_0 otherwise), and no per-launch profile of
// the products running. Everything it does not admit runs the unfused producer and launch_quantize_act as before.
bool rows_q_admits(int n, const int * wtypes, int64_t T, int64_t K, bool rows_or_segs, bool prof_on) {
    if (!rows_or_segs || prof_on || n < 1 || n > ROWS_Q_BATCH || T < 1 || T >= k_mfma_min_tokens || K < 32 || K % 32 != 0 || rows_q_off() == 2 || (rows_q_off() == 1 && n == 5)) return false;
    for (int i = 0; i < n; i++) if (!dtype_quantized(wtypes[i]) || rows_q_is_q81(wtypes[i]) != rows_q_is_q81(wtypes[0])) return false;
    return true;
}

static RowsQOut rows_q_out(int n, const QAct * outs, bool q81) {
    RowsQOut o{};
    for (int i = 0; i < n; i++) o.x[i] = outs[i];
    o.q81 = q81;
    return o;
}

void launch_mix_rows_q(const MixArgs & a, const StateRef & s, int64_t T, int64_t D, const QAct * outs, bool q81, hipStream_t st) {
    const int nb = (int) (D / 32);
    const dim3 grid((unsigned) ((nb + 63) / 64), (unsigned) a.n_out, (unsigned) T);
    const RowsQOut o = rows_q_out(a.n_out, outs, q81);
    g_rows_q_launches.fetch_add(1, std::memory_order_relaxed);
    if (s.segs) hipLaunchKernelGGL(k_mix_rows_q<FORM_SEGS>, grid, dim3(64), 0, st, a, o, nb, s);
    else hipLaunchKernelGGL(k_mix_rows_q<FORM_ROWS>, grid, dim3(64), 0, st, a, o, nb, s);
}

void launch_v6_mix2_rows_q(const V6Mix2Args & a, int64_t T, int64_t D, int64_t R, const QAct * outs, bool q81, hipStream_t st) {
    const int64_t n = T * 5 * D;
    g_rows_q_launches.fetch_add(1, std::memory_order_relaxed);
    hipLaunchKernelGGL(k_v6_mix2_rows_q, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, st, a, rows_q_out(5, outs, q81), T, D, R);
}

bool launch_groupnorm_rows_q(const float * x, const float * lw, const float * lb, float eps, const float * gate, int64_t T, int64_t H, int64_t S,
                             const QAct & out, bool q81, hipStream_t st) {
    if (S % 32 != 0) return false;   // (a block would hold parts of several heads: k_groupnorm + k_quant_act)
    const int64_t TH = T * H;
    g_rows_q_launches.fetch_add(1, std::memory_order_relaxed);
    hipLaunchKernelGGL(k_groupnorm_rows_q, dim3((unsigned) ((TH + 3) / 4)), dim3(256), 0, st, x, lw, lb, eps, gate, out, q81, TH, H, S);
    return true;
}

}  // namespace rwkvmi
