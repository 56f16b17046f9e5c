// rows_mm.hip -- k_mmq_rows<FMT, NT>: y[T][N] = epi(W[N][K] . x[T][K]) for quantised W and 2 <= T < k_mfma_min_tokens on the matrix cores:
// the product of batched decode (rwkv_mi_batch_*, serve, beam, draft passes) and of short sequence / ragged passes. It reads the DECODE
// layout (the row-major planes W.qs / W.qh / W.sc) and the plain QAct of launch_quantize_act; every weight byte leaves HBM once per product.
//
// Numerics: bit-identical to k_mvq_t1 on each token alone (matvec.hip). 64 partials P[l], l = b mod 64, each the chain of blk_fma
// (kdev.h) over its blocks in increasing b, then the xor butterfly 32, 16, 8, 4, 2, 1; leaves without blocks are +0.0. The tree's last two
// levels pair the leaves by l & 3: root = (s0 + s2) + (s1 + s3), s_w = the sum of the subtree l & 3 == w. Wave w of the workgroup owns that
// subtree: its 16 leaves l = w + 4 m are 16 accumulators per output, so K is walked in PLAIN order (block b goes to wave b & 3, accumulator
// (b >> 2) & 15) -- the row-major planes are read as contiguous row pieces, no second image of the matrix, no stack. At the end a lane folds
// its 16 accumulators (m with m + 8, + 4, + 2, + 1: the levels 32, 16, 8, 4) and the four waves meet through LDS.
//
// Work split: a workgroup = 4 waves owns a panel of 16 weight rows (RM_R) and ALL T tokens; blockIdx.y = up to 4 products of one shape (the r / k /
// v / g projections of a layer in one launch). K walks in chunks of 16 blocks: per chunk the 256 threads load the panel's codes (16 rows x
// 256 contiguous bytes, 512 for Q8_0; 16 bytes per thread, non-temporal: one reader), its scales and fifth bits, and the tokens' codes and
// scales (from L2) into registers, RM_PF chunks ahead of their use, and store them into one of two LDS buffers a chunk ahead; one barrier per
// chunk. v_mfma_i32_16x16x32_i8 has K = 32 = one quantisation block: A = the 16 rows (lane = row l % 16, k-group l / 16 = elements 8 g .. 8 g + 7
// of the block -- for the nibble formats the low (g < 2) or high nibbles of 8 code bytes, so no byte shuffle), B = 16 tokens in the same k
// order, D = the exact integer sums, lane (token l % 16, rows 4 (l / 16) .. + 3). T <= 16 is one token tile (NT = 1), 17 .. 31 two tiles that
// share the A operand. 4- and 5-bit codes stay unsigned, the format's offset goes through the activation sum as in blk_fma. The fold per
// (row, token, block) is blk_fma's statement: P = fma(d_w * d_x, (float) isum, P) [+ fma(m_w, s_x, P)]. Dead token columns are zeros in LDS
// and never stored; rows past N are clamped on load and never stored.
#include "kdev.h"
#include "model.h"

#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace rwkvmi {

std::atomic<unsigned long long> g_mmq_rows_launches{0};

typedef int rm_v4i __attribute__((ext_vector_type(4)));

// Panel height: 16 rows (4 waves). -DRWKV_ROWS_MM_R=32 builds the 32-row panel that was measured against it (8 waves, waves 4 .. 7 on the
// second row tile, the token operands shared through LDS): DESIGN.md section 6.7 has the figures; 16 won.
#ifndef RWKV_ROWS_MM_R
#define RWKV_ROWS_MM_R 16
#endif
constexpr int RM_R = RWKV_ROWS_MM_R;             // weight rows per workgroup
constexpr int RM_RT = RM_R / 16, RM_NTH = 256 * RM_RT;
static_assert(RM_R == 16 || RM_R == 32, "one or two row tiles");
constexpr int RM_CB = 16;      // blocks of K per chunk
constexpr int RM_PF = 4;       // chunks in flight (register stages)

struct RowsMmArgs {
    const uint8_t * qs[ROWS_MM_BATCH]; const uint32_t * qh[ROWS_MM_BATCH]; const void * sc[ROWS_MM_BATCH];
    QAct x[ROWS_MM_BATCH]; float * y[ROWS_MM_BATCH]; Epi epi[ROWS_MM_BATCH];
    int64_t N, ldy;
    int T, nb;
};

// One chunk in LDS: weight codes [row][16 blocks] on a pitch 16 bytes past the row (the 16 rows of an operand read start 4 banks apart),
// token codes [token][16 blocks][32 B] likewise, then the small arrays [block][row] / [block][token] as floats / words.
template <int FMT, int NT> struct RmLds {
    static constexpr int  QS = QF<FMT>::QS;
    static constexpr bool QH = QF<FMT>::QH, HM = QF<FMT>::HM, XI = QF<FMT>::OFF != 0;
    static constexpr int  TP = 16 * NT;
    static constexpr int  W_PITCH = RM_CB * QS + 16, X_PITCH = RM_CB * 32 + 16;
    static constexpr int  O_W = 0, O_X = O_W + RM_R * W_PITCH, O_DW = O_X + TP * X_PITCH, O_MW = O_DW + RM_CB * RM_R * 4,
                          O_QH = O_MW + (HM ? RM_CB * RM_R * 4 : 0), O_DX = O_QH + (QH ? RM_CB * RM_R * 4 : 0), O_SX = O_DX + RM_CB * TP * 4,
                          O_XI = O_SX + (HM ? RM_CB * TP * 4 : 0), BUF = O_XI + (XI ? RM_CB * TP * 4 : 0);
    static constexpr int  BYTES = 2 * BUF;
    static_assert(BYTES <= (RM_R == 16 ? 64 : 160) * 1024 && BYTES >= 4 * RM_RT * NT * 4 * 64 * 4, "LDS budget; the waves' exchange at the end reuses the buffers");
};

template <int FMT, int NT>
__global__ __launch_bounds__(RM_NTH) void k_mmq_rows(RowsMmArgs A) {
    typedef RmLds<FMT, NT> L;
    constexpr int QS = L::QS, TP = L::TP, OFF = QF<FMT>::OFF;
    constexpr int NWQ = QS / 16;                 // 16-byte pieces of weight codes per thread and chunk
    constexpr int PPR = RM_CB * QS / 16;         // pieces per row and chunk (16 or 32)
    constexpr int NXQ = 2 * NT / RM_RT;          // 16-byte pieces of token codes per thread and chunk
    constexpr int NXS = (NT + RM_RT - 1) / RM_RT, XS_ALL = 256 * NT;   // token scales per thread and chunk; entries per chunk
    __shared__ __attribute__((aligned(16))) unsigned char lds[L::BYTES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i16 = lane & 15, g = lane >> 4;
    const int wl = wave & 3, r0 = (wave >> 2) * 16;      // the wave's subtree and the first row of its row tile
    const int bz = blockIdx.y;
    const int64_t N = A.N, n0 = (int64_t) blockIdx.x * RM_R;
    const int T = A.T, nb = A.nb;
    const uint8_t * __restrict__ const qs = A.qs[bz];
    const uint32_t * __restrict__ const qh = A.qh[bz];
    const void * __restrict__ const sc = A.sc[bz];
    const QAct x = A.x[bz];
    const int nq = (nb + RM_CB - 1) / RM_CB;

    // ---- a chunk on its way: global memory -> registers (fetch) -> LDS (stash). Blocks past the row end are clamped onto its last block
    //      and never used; tokens past T are zeros ----
    struct Stage { int4 wq[NWQ]; unsigned sc, qh; int4 xq[NXQ]; float xd[NXS], xs[NXS]; int xi[NXS]; };
    Stage stage[RM_PF];
    auto fetch = [&](Stage & s, int q) {
        const int b0 = q * RM_CB;
#pragma unroll
        for (int p = 0; p < NWQ; p++) {
            const int idx = tid + RM_NTH * p, row = idx / PPR, piece = idx % PPR;
            int blk = b0 + piece / NWQ; blk = blk < nb ? blk : nb - 1;
            const int64_t rowc = n0 + row < N ? n0 + row : N - 1;
            s.wq[p] = ldw16(qs + (rowc * nb + blk) * QS + (piece % NWQ) * 16);
        }
        {
            const int row = tid >> 4;
            int blk = b0 + (tid & 15); blk = blk < nb ? blk : nb - 1;
            const int64_t rowc = n0 + row < N ? n0 + row : N - 1;
            if constexpr (L::HM) s.sc = ldw4(reinterpret_cast<const uint32_t *>(sc) + rowc * nb + blk);
            else s.sc = ldw2(reinterpret_cast<const uint16_t *>(sc) + rowc * nb + blk);
            if constexpr (L::QH) s.qh = ldw4(qh + rowc * nb + blk);
        }
#pragma unroll
        for (int p = 0; p < NXQ; p++) {
            const int idx = tid + RM_NTH * p, tok = idx >> 5, piece = idx & 31;
            int blk = b0 + (piece >> 1); blk = blk < nb ? blk : nb - 1;
            s.xq[p] = tok < T ? *reinterpret_cast<const int4 *>(x.q + ((int64_t) tok * nb + blk) * 32 + (piece & 1) * 16) : make_int4(0, 0, 0, 0);
        }
#pragma unroll
        for (int p = 0; p < NXS; p++) {
            const int idx = tid + RM_NTH * p, tok = idx >> 4;
            int blk = b0 + (idx & 15); blk = blk < nb ? blk : nb - 1;
            const bool live = tok < T && idx < XS_ALL;
            const int64_t at = (int64_t) (live ? tok : 0) * nb + blk;
            s.xd[p] = live ? x.d[at] : 0.0f;
            if constexpr (L::HM) s.xs[p] = live ? x.s[at] : 0.0f;
            if constexpr (L::XI) s.xi[p] = live ? x.isum[at] : 0;
        }
    };
    auto stash = [&](const Stage & s, int buf) {
        unsigned char * const B = lds + buf * L::BUF;
#pragma unroll
        for (int p = 0; p < NWQ; p++) {
            const int idx = tid + RM_NTH * p, row = idx / PPR, piece = idx % PPR;
            *reinterpret_cast<int4 *>(B + L::O_W + row * L::W_PITCH + piece * 16) = s.wq[p];
        }
        {
            const int at = ((tid & 15) * RM_R + (tid >> 4)) * 4;      // [block][row]
            *reinterpret_cast<float *>(B + L::O_DW + at) = h2f_bits((uint16_t) (s.sc & 0xFFFFu));
            if constexpr (L::HM) *reinterpret_cast<float *>(B + L::O_MW + at) = h2f_bits((uint16_t) (s.sc >> 16));
            if constexpr (L::QH) *reinterpret_cast<unsigned *>(B + L::O_QH + at) = s.qh;
        }
#pragma unroll
        for (int p = 0; p < NXQ; p++) {
            const int idx = tid + RM_NTH * p, tok = idx >> 5, piece = idx & 31;
            *reinterpret_cast<int4 *>(B + L::O_X + tok * L::X_PITCH + piece * 16) = s.xq[p];
        }
#pragma unroll
        for (int p = 0; p < NXS; p++) {
            const int idx = tid + RM_NTH * p;
            if (idx >= XS_ALL) continue;
            const int at = ((idx & 15) * TP + (idx >> 4)) * 4;        // [block][token]
            *reinterpret_cast<float *>(B + L::O_DX + at) = s.xd[p];
            if constexpr (L::HM) *reinterpret_cast<float *>(B + L::O_SX + at) = s.xs[p];
            if constexpr (L::XI) *reinterpret_cast<int *>(B + L::O_XI + at) = s.xi[p];
        }
    };

    // acc[m][tile][r]: leaf l = wave + 4 m of output (row 4 g + r, token 16 tile + i16)
    float acc[16][NT][4];
#pragma unroll
    for (int m = 0; m < 16; m++)
#pragma unroll
        for (int tl = 0; tl < NT; tl++)
#pragma unroll
            for (int r = 0; r < 4; r++) acc[m][tl][r] = 0.0f;

    // the wave's four blocks of chunk q (c = wave + 4 mm): leaves m = 4 (q & 3) + mm
    auto compute = [&](int q, int buf, auto sub_tag) {
        constexpr int SUB = decltype(sub_tag)::value;
        const unsigned char * const B = lds + buf * L::BUF;
#pragma unroll
        for (int mm = 0; mm < 4; mm++) {
            const int c = wl + 4 * mm;
            if (q * RM_CB + c >= nb) continue;                           // (wave-uniform)
            int a0, a1;
            if constexpr (QS == 32) {
                const int2 raw = *reinterpret_cast<const int2 *>(B + L::O_W + (r0 + i16) * L::W_PITCH + c * 32 + g * 8);
                a0 = raw.x; a1 = raw.y;
            } else {
                const int2 raw = *reinterpret_cast<const int2 *>(B + L::O_W + (r0 + i16) * L::W_PITCH + c * 16 + (g & 1) * 8);
                const int sh = (g >> 1) * 4;
                a0 = (raw.x >> sh) & 0x0F0F0F0F; a1 = (raw.y >> sh) & 0x0F0F0F0F;
                if constexpr (L::QH) {
                    // bit e of the word = the fifth bit of element e; this lane's elements are 8 g .. 8 g + 7
                    const unsigned hb = (*reinterpret_cast<const unsigned *>(B + L::O_QH + (c * RM_R + r0 + i16) * 4) >> (8 * g)) & 0xFFu;
                    a0 |= (int) ((((hb & 0xFu) * 0x00204081u) & 0x01010101u) << 4);
                    a1 |= (int) ((((hb >> 4) * 0x00204081u) & 0x01010101u) << 4);
                }
            }
            const long aop = (long) (((unsigned long long) (unsigned) a1 << 32) | (unsigned) a0);
            const float4 dw4 = *reinterpret_cast<const float4 *>(B + L::O_DW + (c * RM_R + r0 + 4 * g) * 4);
            const float dw[4] = {dw4.x, dw4.y, dw4.z, dw4.w};
            float mw[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if constexpr (L::HM) {
                const float4 mw4 = *reinterpret_cast<const float4 *>(B + L::O_MW + (c * RM_R + r0 + 4 * g) * 4);
                mw[0] = mw4.x; mw[1] = mw4.y; mw[2] = mw4.z; mw[3] = mw4.w;
            }
#pragma unroll
            for (int tl = 0; tl < NT; tl++) {
                const int2 braw = *reinterpret_cast<const int2 *>(B + L::O_X + (tl * 16 + i16) * L::X_PITCH + c * 32 + g * 8);
                const long bop = (long) (((unsigned long long) (unsigned) braw.y << 32) | (unsigned) braw.x);
                const int sat = (c * TP + tl * 16 + i16) * 4;
                const float dx = *reinterpret_cast<const float *>(B + L::O_DX + sat);
                float sx = 0.0f;
                int oa = 0;
                if constexpr (L::HM) sx = *reinterpret_cast<const float *>(B + L::O_SX + sat);
                if constexpr (L::XI) oa = OFF * *reinterpret_cast<const int *>(B + L::O_XI + sat);
                const rm_v4i zero = {0, 0, 0, 0};
                const rm_v4i sums = __builtin_amdgcn_mfma_i32_16x16x32_i8(aop, bop, zero, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int s = sums[r] - oa;
                    const float dd = dw[r] * dx;
                    float P = acc[4 * SUB + mm][tl][r];
                    P = fmaf(dd, (float) s, P);
                    if constexpr (L::HM) P = fmaf(mw[r], sx, P);
                    acc[4 * SUB + mm][tl][r] = P;
                }
            }
        }
    };

    // ---- the walk: chunk q is computed from LDS buffer q & 1 while chunk q + 1 goes from its registers into the other buffer and chunk
    //      q + 1 + RM_PF is requested into the registers that this frees ----
    static_assert(RM_PF == 4, "the register stage of chunk q is q & 3: a compile-time index in the loop unrolled by four");
    fetch(stage[0], 0);
    stash(stage[0], 0);
    if (1 < nq) fetch(stage[1], 1);
    if (2 < nq) fetch(stage[2], 2);
    if (3 < nq) fetch(stage[3], 3);
    if (4 < nq) fetch(stage[0], 4);
    __syncthreads();
    auto round = [&](int q, auto sub_tag) {
        constexpr int SUB = decltype(sub_tag)::value, NX = (SUB + 1) & 3;
        if (q >= nq) return;                                             // (workgroup-uniform)
        compute(q, SUB & 1, sub_tag);
        if (q + 1 < nq) stash(stage[NX], NX & 1);
        if (q + 1 + RM_PF < nq) fetch(stage[NX], q + 1 + RM_PF);
        __syncthreads();
    };
#pragma unroll 1
    for (int q0 = 0; q0 < nq; q0 += 4) {
        static_for<RM_PF>([&](auto sub_tag) { round(q0 + decltype(sub_tag)::value, sub_tag); });
    }

    // ---- the wave's subtree: leaves l and l ^ 32 (m, m + 8), then ^ 16, ^ 8, ^ 4; the four subtrees meet in LDS as (s0 + s2) + (s1 + s3) ----
    float * const ex = reinterpret_cast<float *>(lds);                   // [wave][tile][r][lane]; every wave is behind the walk's last barrier
#pragma unroll
    for (int tl = 0; tl < NT; tl++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
#pragma unroll
            for (int w = 8; w >= 1; w >>= 1)
#pragma unroll
                for (int m = 0; m < w; m++) acc[m][tl][r] = acc[m][tl][r] + acc[m + w][tl][r];
            ex[((wave * NT + tl) * 4 + r) * 64 + lane] = acc[0][tl][r];
        }
    __syncthreads();
    float * __restrict__ const y = A.y[bz];
    const Epi epi = A.epi[bz];
#pragma unroll
    for (int p = 0; p < NT; p++) {
        const int o = tid + RM_NTH * p, row = o % RM_R, tok = o / RM_R;   // consecutive threads = consecutive rows of one token
        const int at = (row >> 4) * 4 * NT * 256 + ((tok >> 4) * 4 + (row & 3)) * 64 + ((row & 15) >> 2) * 16 + (tok & 15);
        const float s0 = ex[at], s1 = ex[NT * 256 + at], s2 = ex[2 * NT * 256 + at], s3 = ex[3 * NT * 256 + at];
        const float v = (s0 + s2) + (s1 + s3);
        const int64_t n = n0 + row;
        if (n < N && tok < T) y[(int64_t) tok * A.ldy + n] = apply_epi(epi, v, tok, n, A.ldy);
    }
}

// RWKV_MI_ROWS_MM = tn: the token-tiled VALU kernel (k_mvq_tn) for the whole process, as before this kernel (A/B, tests). Read once.
static bool rows_mm_off() {
    static const bool off = [] { const char * e = getenv("RWKV_MI_ROWS_MM"); return e && strcmp(e, "tn") == 0; }();
    return off;
}

// The gate, whole: everything it does not admit runs k_mvq_t1 / k_mvq_tn / the sequence GEMM as before. No lower bound on N or K: a panel
// clamps its rows, a chunk its blocks.
bool mmq_rows_admits(int wtype, int64_t T, int64_t K) {
    return dtype_quantized(wtype) && T >= 2 && T < k_mfma_min_tokens && K >= 32 && K % 32 == 0 && !rows_mm_off();
}

template <int FMT>
static void launch_mmq_rows_fmt(const RowsMmArgs & a, int n, hipStream_t st) {
    const dim3 grid((unsigned) ((a.N + RM_R - 1) / RM_R), (unsigned) n);
    if (a.T <= 16) hipLaunchKernelGGL((k_mmq_rows<FMT, 1>), grid, dim3(RM_NTH), 0, st, a);
    else hipLaunchKernelGGL((k_mmq_rows<FMT, 2>), grid, dim3(RM_NTH), 0, st, a);
}

void launch_mmq_rows(int n, const DevTensor * const * Ws, const QAct * xs, float * const * ys, const Epi * epis, int64_t T, int64_t ldy, hipStream_t st) {
    RowsMmArgs a{};
    for (int i = 0; i < n; i++) { a.qs[i] = Ws[i]->qs; a.qh[i] = Ws[i]->qh; a.sc[i] = Ws[i]->sc; a.x[i] = xs[i]; a.y[i] = ys[i]; a.epi[i] = epis[i]; }
    a.N = Ws[0]->rows(); a.ldy = ldy; a.T = (int) T; a.nb = (int) (Ws[0]->cols() / 32);
    g_mmq_rows_launches.fetch_add(1, std::memory_order_relaxed);
    switch (Ws[0]->type) {
        case T_Q4_0: launch_mmq_rows_fmt<T_Q4_0>(a, n, st); break;
        case T_Q4_1: launch_mmq_rows_fmt<T_Q4_1>(a, n, st); break;
        case T_Q5_0: launch_mmq_rows_fmt<T_Q5_0>(a, n, st); break;
        case T_Q5_1: launch_mmq_rows_fmt<T_Q5_1>(a, n, st); break;
        case T_Q8_0: launch_mmq_rows_fmt<T_Q8_0>(a, n, st); break;
        default: break;
    }
}

}  // namespace rwkvmi
