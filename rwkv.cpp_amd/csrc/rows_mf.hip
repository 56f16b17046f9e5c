// rows_mf.hip -- k_mmf_rows<F16, NT>: y[T][N] = epi(W[N][K] . x[T][K]) for F16 / F32 W and 5 <= T < k_mfma_min_tokens on the matrix cores: the
// unquantised product of batched decode (rwkv_mi_batch_*, serve, beam, draft passes) and of short sequence / ragged passes -- the head of every
// model, every matrix of an FP16 / FP32 file, the low-rank stages of RWKV-7. Every weight byte leaves HBM once per product (k_mvf's token tiles
// of four walk the matrix ceil(T / 4) times).
//
// Numerics: bit-identical to k_mvf on each token alone (matvec.hip, "Projection, F32 / F16 weights"). ggml's vec_dot order: 32 partials,
// partial p the chain fmaf(w[k], x[k], .) over k = p, p + 32, p + 64, ... in increasing k; then ps[i] += ps[i + 16], += ps[i + 8], += ps[i + 4],
// (ps0 + ps1) + (ps2 + ps3). v_mfma_f32_16x16x4_f32 adds its four k slices onto the accumulator as a chain of single fused multiply-adds in k
// order (tools/mfma_f32_chain.hip), so ONE instruction with the slices p, p + 32, p + 64, p + 96 of a 128-element step is four links of partial
// p's chain for a 16-token x 16-row tile (k_mmfx_seq's head comment). F16 weights: the activations are rounded to fp16 first, as ggml feeds an
// F16 matrix, and both sides are widened to f32 for the f32 instruction (the f16 MFMA shapes add in another order). An absent k slice of a tail
// (K % 32 == 0, not % 128) is +0 in the activations against -0 in the weights: fma(+0, -0, a) = a for EVERY a, a = -0 included.
//
// Work split: a workgroup = 4 waves owns a panel of 16 weight rows (MF_R) and ALL T tokens; T <= 16 is one token tile (NT = 1), 17 .. 31 two tiles
// that share the weight operand. The 32 partials are independent until the fold, so wave w owns partials 8 w .. 8 w + 7 (k_mvf gives them to
// lane q of a row): 8 NT accumulators of 4 registers. In a 128-element step its lane (slice j = lane / 16, row or token i = lane % 16) needs
// elements 32 j + 8 w .. + 7 of its row: 16 contiguous bytes of halfs or 32 of floats, and every staged element is read by exactly ONE wave.
//
// Movement: K walks in chunks of 512 bytes per row in LDS whatever the type (256 elements = two steps for F16 weights, where the rounded
// activations are kept as the halfs they are; 128 = one step for F32). Per chunk the 256 threads load the panel (16 rows x 512 contiguous
// bytes, 16 bytes per thread and piece, non-temporal: one reader) and the tokens' floats (from L2) into registers four chunks (three: F16, two tiles) ahead of their
// use, and store them into one of two LDS buffers a chunk ahead -- the activations rounded and packed on the way; one barrier per chunk. Rows
// sit on a pitch of 528 bytes: the 16 rows of an operand read start 4 banks apart, 16-byte reads are conflict-free. Halfs are widened by the
// wave that reads them (one reader per element: as many conversions as on the way in, half the LDS traffic). Token columns past T are zeros in
// LDS and never stored; rows past N are clamped on load and never stored.
//
// The fold: behind the walk's last barrier waves 2 and 3 hand their partials to waves 0 and 1 through LDS (ps[i] += ps[i + 16]), wave 1 hands
// its sums to wave 0 (+= ps[i + 8]); += ps[i + 4] and (ps0 + ps1) + (ps2 + ps3) stay inside the lane of wave 0, which stores.
#include "kdev.h"
#include "model.h"

#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <utility>

namespace rwkvmi {

std::atomic<unsigned long long> g_mmf_rows_launches{0};

typedef float mfr_f4 __attribute__((ext_vector_type(4)));

constexpr int MF_R = 16;         // weight rows per workgroup
constexpr int MF_ROWB = 512;     // bytes of a row's chunk in LDS, weights and activations alike
constexpr int MF_PITCH = MF_ROWB + 16;

template <bool F16, int NT> struct MfrCfg {
    static constexpr int ES = F16 ? 2 : 4;               // bytes per element in LDS
    static constexpr int KC = MF_ROWB / ES;              // elements of K per chunk
    static constexpr int KS = KC / 128;                  // steps of 128 elements (8 NT instructions per wave) per chunk
    static constexpr int EP = 16 / ES;                   // elements of a 16-byte piece
    static constexpr int TP = 16 * NT;
    static constexpr int PF = F16 && NT == 2 ? 3 : 4;    // chunks in flight (register stages): 40 registers per stage for F16 x two tiles, 16 .. 24 otherwise
    static constexpr int NWP = 2, NXP = 2 * NT;          // 16-byte pieces per thread and chunk: weights, activations (as they sit in LDS)
    static constexpr int O_W = 0, O_X = MF_R * MF_PITCH, BUF = O_X + TP * MF_PITCH, BYTES = 2 * BUF;
    static_assert(BYTES <= 64 * 1024 && BYTES >= 2 * 8 * NT * 64 * 16, "LDS budget; the waves' exchange at the end reuses the buffers");
};

template <bool F16, int NT>
__global__ __launch_bounds__(256) void k_mmf_rows(const void * __restrict__ W, int64_t N, int64_t K, const float * __restrict__ x, int64_t ldx,
                                                  int T, float * __restrict__ y, int64_t ldy, Epi epi) {
    typedef MfrCfg<F16, NT> C;
    constexpr int ES = C::ES, KC = C::KC, KS = C::KS, EP = C::EP, PF = C::PF, NWP = C::NWP, NXP = C::NXP;
    __shared__ __attribute__((aligned(16))) unsigned char lds[C::BYTES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i16 = lane & 15, j = lane >> 4;
    const int64_t n0 = (int64_t) blockIdx.x * MF_R;
    const int nq = (int) ((K + KC - 1) / KC);
    const unsigned char * __restrict__ const Wb = reinterpret_cast<const unsigned char *>(W);

    // ---- a chunk on its way: global memory -> registers (fetch) -> LDS (stash). Piece idx = tid + 256 p is 16 bytes of LDS: row or token idx / 32,
    //      elements EP (idx % 32) .. of the chunk. Pieces past K are -0 (weights) against +0 (activations); tokens past T are +0.
    //      (The loads are predicated, and the compiler, which cannot count loads behind a branch, waits for ALL loads in flight before every stash.
    //      A walk whose loads are all unconditional -- addresses clamped, padding chosen at the stash, a cached line requested past the last
    //      chunk -- gets exact wait counts and was measured SLOWER; this form is the faster of the two.) ----
    constexpr int NEG0 = F16 ? (int) 0x80008000u : (int) 0x80000000u;
    struct Stage { int4 w[NWP]; float4 x[NXP][F16 ? 2 : 1]; };
    Stage stage[PF];
    auto fetch = [&](Stage & s, int q) {
        const int64_t k0 = (int64_t) q * KC;
#pragma unroll
        for (int p = 0; p < NWP; p++) {
            const int idx = tid + 256 * p, row = idx >> 5;
            const int64_t k = k0 + EP * (idx & 31);
            const int64_t rowc = n0 + row < N ? n0 + row : N - 1;
            s.w[p] = k < K ? ldw16(Wb + (rowc * K + k) * ES) : make_int4(NEG0, NEG0, NEG0, NEG0);
        }
#pragma unroll
        for (int p = 0; p < NXP; p++) {
            const int idx = tid + 256 * p, tok = idx >> 5;
            const int64_t k = k0 + EP * (idx & 31);
            const bool live = tok < T && k < K;
            const float * const src = x + (int64_t) (live ? tok : 0) * ldx + (live ? k : 0);
#pragma unroll
            for (int h = 0; h < (F16 ? 2 : 1); h++) s.x[p][h] = live ? *reinterpret_cast<const float4 *>(src + 4 * h) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto stash = [&](const Stage & s, int buf) {
        unsigned char * const B = lds + buf * C::BUF;
#pragma unroll
        for (int p = 0; p < NWP; p++) {
            const int idx = tid + 256 * p;
            *reinterpret_cast<int4 *>(B + C::O_W + (idx >> 5) * MF_PITCH + (idx & 31) * 16) = s.w[p];
        }
#pragma unroll
        for (int p = 0; p < NXP; p++) {
            const int idx = tid + 256 * p;
            unsigned char * const dst = B + C::O_X + (idx >> 5) * MF_PITCH + (idx & 31) * 16;
            if constexpr (F16) {
                // what ggml feeds an F16 matrix: the fp16 value of the activation, kept as the half it is (h2f_bits gives round_f16's float back)
                const float f[8] = {s.x[p][0].x, s.x[p][0].y, s.x[p][0].z, s.x[p][0].w, s.x[p][1].x, s.x[p][1].y, s.x[p][1].z, s.x[p][1].w};
                unsigned u[4];
#pragma unroll
                for (int e = 0; e < 4; e++)
                    u[e] = (unsigned) __half_as_ushort(__float2half_rn(f[2 * e])) | ((unsigned) __half_as_ushort(__float2half_rn(f[2 * e + 1])) << 16);
                *reinterpret_cast<int4 *>(dst) = make_int4((int) u[0], (int) u[1], (int) u[2], (int) u[3]);
            } else {
                *reinterpret_cast<float4 *>(dst) = s.x[p][0];
            }
        }
    };
    // elements 32 j + 8 wave .. + 7 of step kk of a row's chunk, as floats
    auto operand = [&](const unsigned char * rowp, int kk, float (&o)[8]) {
        const unsigned char * const src = rowp + (128 * kk + 32 * j + 8 * wave) * ES;
        if constexpr (F16) {
            const int4 raw = *reinterpret_cast<const int4 *>(src);
            const unsigned u[4] = {(unsigned) raw.x, (unsigned) raw.y, (unsigned) raw.z, (unsigned) raw.w};
#pragma unroll
            for (int e = 0; e < 4; e++) { o[2 * e] = h2f_bits((uint16_t) (u[e] & 0xFFFFu)); o[2 * e + 1] = h2f_bits((uint16_t) (u[e] >> 16)); }
        } else {
            const float4 a = *reinterpret_cast<const float4 *>(src), b = *reinterpret_cast<const float4 *>(src + 16);
            o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
        }
    };

    // acc[tile][e]: partial 8 wave + e of the outputs (token 16 tile + 4 j + register, row i16)
    mfr_f4 acc[NT][8];
#pragma unroll
    for (int tl = 0; tl < NT; tl++)
#pragma unroll
        for (int e = 0; e < 8; e++) acc[tl][e] = (mfr_f4){0.0f, 0.0f, 0.0f, 0.0f};

    auto compute = [&](int q, int buf) {
        const unsigned char * const B = lds + buf * C::BUF;
#pragma unroll
        for (int kk = 0; kk < KS; kk++) {
            if ((int64_t) q * KC + 128 * kk >= K) break;                      // (workgroup-uniform) a step wholly past K adds nothing
            float wb[8];
            operand(B + C::O_W + i16 * MF_PITCH, kk, wb);
#pragma unroll
            for (int tl = 0; tl < NT; tl++) {
                float xa[8];
                operand(B + C::O_X + (16 * tl + i16) * MF_PITCH, kk, xa);
                // D[token][row] += A[token][k] B[k][row]: the instruction of partial 8 wave + e adds the links k = 128 step + 8 wave + e, + 32, + 64, + 96
#pragma unroll
                for (int e = 0; e < 8; e++) acc[tl][e] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[e], wb[e], acc[tl][e], 0, 0, 0);
            }
        }
    };

    // ---- the walk: chunk q is computed from LDS buffer q & 1 while chunk q + 1 goes from its registers (stage (q + 1) % PF) into the other buffer
    //      and chunk q + 1 + PF is requested into the registers that this frees ----
    fetch(stage[0], 0);
    stash(stage[0], 0);
    static_for<PF>([&](auto s) { constexpr int S = decltype(s)::value; if (S >= 1 && S < nq) fetch(stage[S], S); });
    if (PF < nq) fetch(stage[0], PF);
    __syncthreads();
#pragma unroll 1
    for (int q0 = 0; q0 < nq; q0 += PF) {
        static_for<PF>([&](auto s) {
            constexpr int S = decltype(s)::value, NX = (S + 1) % PF;
            const int q = q0 + S;
            if (q < nq) {                                                     // (workgroup-uniform)
                compute(q, q & 1);
                if (q + 1 < nq) stash(stage[NX], (q + 1) & 1);
                if (q + 1 + PF < nq) fetch(stage[NX], q + 1 + PF);
                __syncthreads();
            }
        });
    }

    // ---- the fold of k_mvf. Every wave is behind the walk's last barrier: the buffers are free. xch[wave & 1][tile][e][lane] ----
    mfr_f4 * const xch = reinterpret_cast<mfr_f4 *>(lds) + (size_t) (wave & 1) * NT * 8 * 64;
    if (wave >= 2) {
#pragma unroll
        for (int tl = 0; tl < NT; tl++)
#pragma unroll
            for (int e = 0; e < 8; e++) xch[(tl * 8 + e) * 64 + lane] = acc[tl][e];
    }
    __syncthreads();
    if (wave < 2) {
#pragma unroll
        for (int tl = 0; tl < NT; tl++)
#pragma unroll
            for (int e = 0; e < 8; e++) acc[tl][e] = acc[tl][e] + xch[(tl * 8 + e) * 64 + lane];        // ps[i] += ps[i + 16]
    }
    if (wave == 1) {                                                          // (its own region: nobody else reads it)
#pragma unroll
        for (int tl = 0; tl < NT; tl++)
#pragma unroll
            for (int e = 0; e < 8; e++) xch[(tl * 8 + e) * 64 + lane] = acc[tl][e];
    }
    __syncthreads();
    if (wave != 0) return;
    const mfr_f4 * const up = reinterpret_cast<const mfr_f4 *>(lds) + (size_t) NT * 8 * 64;
    // C / D layout: column (= weight row) lane % 16, row (= token) 4 (lane / 16) + register
    const int64_t n = n0 + i16;
#pragma unroll
    for (int tl = 0; tl < NT; tl++) {
#pragma unroll
        for (int e = 0; e < 8; e++) acc[tl][e] = acc[tl][e] + up[(tl * 8 + e) * 64 + lane];            // ps[i] += ps[i + 8]
#pragma unroll
        for (int e = 0; e < 4; e++) acc[tl][e] = acc[tl][e] + acc[tl][e + 4];
        const mfr_f4 res = (acc[tl][0] + acc[tl][1]) + (acc[tl][2] + acc[tl][3]);
        if (n < N) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int t = 16 * tl + 4 * j + r;
                if (t < T) y[(int64_t) t * ldy + n] = apply_epi(epi, res[r], t, n, ldy);
            }
        }
    }
}

// RWKV_MI_ROWS_MF = valu: k_mvf's token tiles of four for the whole process, as before this kernel (A/B, tests). Read once.
static bool rows_mf_off() {
    static const bool off = [] { const char * e = getenv("RWKV_MI_ROWS_MF"); return e && strcmp(e, "valu") == 0; }();
    return off;
}

// The gate, whole: everything it does not admit runs k_mvf as before. Up to TT = 4 tokens k_mvf already reads each byte once, hence T > 4.
// No lower bound on N or K: a panel clamps its rows, a chunk pads its pieces.
bool mmf_rows_admits(int wtype, int64_t T, int64_t K, int64_t ldx) {
    return (wtype == T_F16 || wtype == T_F32) && T > 4 && T < k_mfma_min_tokens && K >= 32 && K % 32 == 0 && ldx % 4 == 0 && !rows_mf_off();
}

template <bool F16>
static void launch_mmf_rows_t(const DevTensor & W, const float * x, int64_t ldx, int64_t T, float * y, int64_t ldy, const Epi & epi, hipStream_t st) {
    const int64_t N = W.rows(), K = W.cols();
    const dim3 grid((unsigned) ((N + MF_R - 1) / MF_R));
    if (T <= 16) hipLaunchKernelGGL((k_mmf_rows<F16, 1>), grid, dim3(256), 0, st, W.data, N, K, x, ldx, (int) T, y, ldy, epi);
    else hipLaunchKernelGGL((k_mmf_rows<F16, 2>), grid, dim3(256), 0, st, W.data, N, K, x, ldx, (int) T, y, ldy, epi);
}

void launch_mmf_rows(const DevTensor & W, const float * x, int64_t ldx, int64_t T, float * y, int64_t ldy, const Epi & epi, hipStream_t st) {
    g_mmf_rows_launches.fetch_add(1, std::memory_order_relaxed);
    if (W.type == T_F16) launch_mmf_rows_t<true>(W, x, ldx, T, y, ldy, epi, st);
    else launch_mmf_rows_t<false>(W, x, ldx, T, y, ldy, epi, st);
}

}  // namespace rwkvmi
