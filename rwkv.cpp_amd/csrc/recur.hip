// recur.hip -- the recurrences of the per-op path: the token-shift mixes, the WKV bodies of RWKV-4 / 5-6 / 7 in their sequence, row, segment
// and replay forms, the group norm and the RWKV-7 key preparation. The numerics contract is the one at the head of kernels.hip.
#include "kdev.h"

namespace rwkvmi {

// ---------------------------------------------------------------------------------------------------------------
// The forms of a recurrence (kernels.h, StateRef). An entry point is its body's kernel at one FORM, an int template parameter; it gets the
// launcher's StateRef by value and takes from it where its block's state goes in -> out and which tokens [t0, t1) the block runs:
//   FORM_SEQ   (grid.y 1): one sequence, s.in -> s.out, tokens [0, T);
//   FORM_ROWS  (grid.y T): row t = blockIdx.y is its own sequence (batched decode), rows[t].in -> rows[t].out, tokens [t, t + 1);
//   FORM_SEGS  (grid.y n_segs): segment blockIdx.y is tokens [t0, t1) of its own sequence (ragged pass), segs[i].in -> segs[i].out.
// The StateRef is the LAST kernel argument: what a form reads together (out and H; off and rows or segs) then lies together in the argument
// block and comes in as many scalar loads as a kernel of that form alone would need.
// ---------------------------------------------------------------------------------------------------------------
// (the enum itself: kdev.h, the quantising row forms of rows_q.hip take the same parameter)

struct FormSpan { const float * in; float * out; int64_t t0, t1; };
template <int FORM> __device__ __forceinline__ FormSpan form_span(const StateRef & s, int64_t T) {
    if constexpr (FORM == FORM_ROWS) {
        const int64_t t = blockIdx.y;
        return {s.rows[t].in + s.off, s.rows[t].out + s.off, t, t + 1};
    } else if constexpr (FORM == FORM_SEGS) {
        const SegState seg = s.segs[blockIdx.y];
        return {seg.in + s.off, seg.out + s.off, seg.t0, seg.t1};
    } else {
        return {s.in + s.off, s.out + s.off, 0, T};
    }
}

// f(integral_constant<int, FORM>) of the form `s` asks for, and the grid.y of that form
template <class F> static void with_form(const StateRef & s, F && f) {
    if (s.segs) f(std::integral_constant<int, FORM_SEGS>{});
    else if (s.rows) f(std::integral_constant<int, FORM_ROWS>{});
    else f(std::integral_constant<int, FORM_SEQ>{});
}
static unsigned form_grid_y(const StateRef & s, int64_t T) { return s.segs ? (unsigned) s.n_segs : s.rows ? (unsigned) T : 1u; }

// ---------------------------------------------------------------------------------------------------------------
// Token-shift mixes
// ---------------------------------------------------------------------------------------------------------------

// the lerps of element idx (channel d) given x and x_prev; the forms of k_mix differ only in where x_prev comes from and the carry goes
__device__ __forceinline__ void mix_elem(const MixArgs & a, int64_t idx, int64_t d, float x, float xp) {
    if (a.mode == 0) {
        for (int f = 0; f < a.n_out; f++) a.out[f][idx] = mix_lerp_v4(x, xp, a.coef[f][d]);
    } else {
        const float sx = xp - x;
        if (a.sx) a.sx[idx] = sx;
        for (int f = 0; f < a.n_out; f++) a.out[f][idx] = mix_lerp_v6(x, sx, a.coef[f][d]);
    }
}

// launched over tokens, not over sequences: the form decides x_prev and the carry per element
template <int FORM>
__global__ __launch_bounds__(256) void k_mix(MixArgs a, int64_t T, int64_t D, StateRef s) {
    const int64_t n = T * D, co = s.off;
    for (int64_t idx = (int64_t) blockIdx.x * 256 + threadIdx.x; idx < n; idx += (int64_t) gridDim.x * 256) {
        const int64_t t = idx / D, d = idx - t * D;
        const float x = a.xn[idx];
        if constexpr (FORM == FORM_ROWS) {
            // every row is the last token of its sequence: x_prev = rows[t].in[co + d], and rows[t].out[co + d] = x
            mix_elem(a, idx, d, x, s.rows[t].in[co + d]);
            s.rows[t].out[co + d] = x;
        } else if constexpr (FORM == FORM_SEGS) {
            // token t belongs to seg = segs[seg_of[t]]; its first token continues from the slot, its last one leaves the carry there
            const SegState seg = s.segs[s.seg_of[t]];
            mix_elem(a, idx, d, x, (t == seg.t0) ? seg.in[co + d] : a.xn[idx - D]);
            if (t == seg.t1 - 1) seg.out[co + d] = x;
        } else {
            mix_elem(a, idx, d, x, (t == 0) ? s.in[co + d] : a.xn[idx - D]);
            if (t == T - 1) s.out[co + d] = x;
        }
    }
}

void launch_mix(MixArgs a, const StateRef & s, int64_t T, int64_t D, hipStream_t st) {
    const int64_t n = T * D;
    const unsigned grid = (unsigned) ((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    with_form(s, [&](auto form) { hipLaunchKernelGGL(k_mix<decltype(form)::value>, dim3(grid), dim3(256), 0, st, a, T, D, s); });
}

__global__ __launch_bounds__(256) void k_v6_mix2(V6Mix2Args a, int64_t T, int64_t D, int64_t R) {
    const int64_t n = T * 5 * D;
    for (int64_t idx = (int64_t) blockIdx.x * 256 + threadIdx.x; idx < n; idx += (int64_t) gridDim.x * 256) {
        const int64_t d = idx % D;
        const int64_t f = (idx / D) % 5;
        const int64_t t = idx / (5 * D);
        a.out[f][t * D + d] = v6_mix2_elem(a, t, f, d, D, R);
    }
}

void launch_v6_mix2(const V6Mix2Args & a, int64_t T, int64_t D, int64_t R, hipStream_t st) {
    const int64_t n = T * 5 * D;
    const unsigned grid = (unsigned) ((n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192);
    hipLaunchKernelGGL(k_v6_mix2, dim3(grid), dim3(256), 0, st, a, T, D, R);
}

// ---------------------------------------------------------------------------------------------------------------
// WKV recurrences. Sequential in t inside the kernel; the state stays in registers across the tokens of a call.
// Each recurrence is one __device__ body over tokens [t0, t1) from state_in to state_out, with two entry points:
//   k_wkvX<.., FORM> (grid (H, form_grid_y), channel blocks for H with RWKV-4): body(f.in, f.out, f.t0, f.t1), f = form_span<FORM>(s, T) --
//                one sequence, one sequence per row or one per segment (RWKV-5 / 6: k_wkv6 / k_wkv6_rows / k_wkv6_segs, one kernel per
//                form with the same three statements, see there);
//   k_wkvX_replay (grid (H, n_segs, layers), rwkv_mi_batch_eval_draft): every layer of segment i again over its first keep[i] tokens, on the
//                inputs the pass stashed, body(segs[i].in + so, segs[i].out + so, t0, t0 + keep[i]) -- see "Replay" below.
// A row therefore performs exactly the statements of one single-token step, in the same order. The bodies' pointers are plain: the
// entry points' per-token parameters carry __restrict__, the slot pointers read out of rows[] / segs[] do not (on the row form's slot
// pointers it raised the 64-wide RWKV-7 kernel from 86 to 126 VGPRs).
// ---------------------------------------------------------------------------------------------------------------

// RWKV-4: one thread per channel i; the state is aa, bb, pp at [0, D), [D, 2 D), [2 D, 3 D)
__device__ __forceinline__ void wkv4_body(const float * k, const float * v, const float * r, const float * tf, const float * td,
                                          const float * state_in, float * state_out, float * out, int64_t t0, int64_t t1, int64_t D) {
    const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (i >= D) return;
    float aa = state_in[i], bb = state_in[D + i], pp = state_in[2 * D + i];
    const float u = tf[i], w = td[i];
    for (int64_t t = t0; t < t1; t++) {
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
    }
    state_out[i] = aa; state_out[D + i] = bb; state_out[2 * D + i] = pp;
}

template <int FORM>
__global__ __launch_bounds__(256) void k_wkv4(const float * __restrict__ k, const float * __restrict__ v, const float * __restrict__ r,
                                              const float * __restrict__ tf, const float * __restrict__ td, float * __restrict__ out,
                                              int64_t T, int64_t D, StateRef s) {
    const FormSpan f = form_span<FORM>(s, T);
    wkv4_body(k, v, r, tf, td, f.in, f.out, out, f.t0, f.t1, D);
}

void launch_wkv4(const float * k, const float * v, const float * r, const float * time_first, const float * time_decay,
                 const StateRef & s, float * out, int64_t T, int64_t D, hipStream_t st) {
    const dim3 grid((unsigned) ((D + 255) / 256), form_grid_y(s, T));
    with_form(s, [&](auto form) {
        hipLaunchKernelGGL(k_wkv4<decltype(form)::value>, grid, dim3(256), 0, st, k, v, r, time_first, time_decay, out, T, D, s);
    });
}

// wkv6: one wave per head, lane j owns value column j of state[h][:, j] (SREG = S when S is a supported compile-time
// size, else the state column is kept in global memory -- generic path for unusual head sizes).
template <int S>
__device__ __forceinline__ void wkv6_body(const float * r, const float * k, const float * v, const float * u, int u_per_chan, const float * w, int w_mode,
                                          const float * state_in, float * state_out, float * out, int64_t t0, int64_t t1, int64_t H) {
    __shared__ float l_r[S], l_k[S], l_u[S], l_w[S];
    const int64_t h = blockIdx.x;
    const int j = threadIdx.x;
    const int64_t D = H * S;
    float s[S];
    if (j < S) {
#pragma unroll
        for (int i = 0; i < S; i++) s[i] = state_in[h * S * S + i * S + j];
    }
    if (j < S) {
        l_u[j] = u_per_chan ? u[h * S + j] : u[h];
        if (w_mode < 2) l_w[j] = (w_mode == 1) ? w[h * S + j] : w[h];
    }
    for (int64_t t = t0; t < t1; t++) {
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
        }
    }
    if (j < S) {
#pragma unroll
        for (int i = 0; i < S; i++) state_out[h * S * S + i * S + j] = s[i];
    }
}

__device__ __forceinline__ void wkv6_body_generic(const float * r, const float * k, const float * v, const float * u, int u_per_chan,
                                                  const float * w, int w_mode,
                                                  const float * state_in, float * state_out, float * out, int64_t t0, int64_t t1, int64_t H, int64_t S) {
    const int64_t h = blockIdx.x;
    const int64_t D = H * S;
    for (int64_t j = threadIdx.x; j < S; j += blockDim.x) {
        for (int64_t t = t0; t < t1; t++) {
            const float * sin = (t == t0) ? state_in : state_out;
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
                state_out[h * S * S + i * S + j] = prev * wi + kv;
            }
            out[t * D + h * S + j] = o;
        }
    }
}

// This body keeps one entry point per form and does not take the StateRef: as k_wkv6<S, FORM> its segment form at S = 64 measured 0.2 us
// (0.5 %) per launch over k_wkv6_segs<64>, instruction for instruction the same kernel (profiles/kernels_split_parent_vs_commit_7b_q4_0.jsonl).
template <int S>
__global__ __launch_bounds__(64) void k_wkv6(const float * __restrict__ r, const float * __restrict__ k, const float * __restrict__ v,
                                             const float * __restrict__ u, int u_per_chan, const float * __restrict__ w, int w_mode,
                                             const float * __restrict__ state_in, float * __restrict__ state_out, float * __restrict__ out,
                                             int64_t T, int64_t H) {
    wkv6_body<S>(r, k, v, u, u_per_chan, w, w_mode, state_in, state_out, out, 0, T, H);
}

template <int S>
__global__ __launch_bounds__(64) void k_wkv6_rows(const float * __restrict__ r, const float * __restrict__ k, const float * __restrict__ v,
                                                  const float * __restrict__ u, int u_per_chan, const float * __restrict__ w, int w_mode,
                                                  const RowState * __restrict__ rows, int64_t so, float * __restrict__ out, int64_t H) {
    const int64_t t = blockIdx.y;
    wkv6_body<S>(r, k, v, u, u_per_chan, w, w_mode, rows[t].in + so, rows[t].out + so, out, t, t + 1, H);
}

__global__ __launch_bounds__(256) void k_wkv6_generic(const float * __restrict__ r, const float * __restrict__ k, const float * __restrict__ v,
                                                      const float * __restrict__ u, int u_per_chan, const float * __restrict__ w, int w_mode,
                                                      const float * __restrict__ state_in, float * __restrict__ state_out, float * __restrict__ out,
                                                      int64_t T, int64_t H, int64_t S) {
    wkv6_body_generic(r, k, v, u, u_per_chan, w, w_mode, state_in, state_out, out, 0, T, H, S);
}

__global__ __launch_bounds__(256) void k_wkv6_rows_generic(const float * __restrict__ r, const float * __restrict__ k, const float * __restrict__ v,
                                                           const float * __restrict__ u, int u_per_chan, const float * __restrict__ w, int w_mode,
                                                           const RowState * __restrict__ rows, int64_t so, float * __restrict__ out, int64_t H, int64_t S) {
    const int64_t t = blockIdx.y;
    wkv6_body_generic(r, k, v, u, u_per_chan, w, w_mode, rows[t].in + so, rows[t].out + so, out, t, t + 1, H, S);
}

template <int S>
__global__ __launch_bounds__(64) void k_wkv6_segs(const float * __restrict__ r, const float * __restrict__ k, const float * __restrict__ v,
                                                  const float * __restrict__ u, int u_per_chan, const float * __restrict__ w, int w_mode,
                                                  const SegState * __restrict__ segs, int64_t so, float * __restrict__ out, int64_t H) {
    const SegState seg = segs[blockIdx.y];
    wkv6_body<S>(r, k, v, u, u_per_chan, w, w_mode, seg.in + so, seg.out + so, out, seg.t0, seg.t1, H);
}

__global__ __launch_bounds__(256) void k_wkv6_segs_generic(const float * __restrict__ r, const float * __restrict__ k, const float * __restrict__ v,
                                                           const float * __restrict__ u, int u_per_chan, const float * __restrict__ w, int w_mode,
                                                           const SegState * __restrict__ segs, int64_t so, float * __restrict__ out, int64_t H, int64_t S) {
    const SegState seg = segs[blockIdx.y];
    wkv6_body_generic(r, k, v, u, u_per_chan, w, w_mode, seg.in + so, seg.out + so, out, seg.t0, seg.t1, H, S);
}

void launch_wkv6(const float * r, const float * k, const float * v, const float * u, int u_per_chan, const float * w, int w_mode,
                 const StateRef & s, float * out, int64_t T, int64_t H, int64_t S, hipStream_t st) {
    if (s.segs) {
        const dim3 sgrid((unsigned) H, (unsigned) s.n_segs);
        auto go = [&](auto kern, unsigned block, auto... generic_s) {
            hipLaunchKernelGGL(kern, sgrid, dim3(block), 0, st, r, k, v, u, u_per_chan, w, w_mode, s.segs, s.off, out, H, generic_s...);
        };
        switch (S) {
            case 64: go(k_wkv6_segs<64>, 64); break;
            case 32: go(k_wkv6_segs<32>, 64); break;
            case 16: go(k_wkv6_segs<16>, 64); break;
            case 8:  go(k_wkv6_segs<8>, 64); break;
            default: go(k_wkv6_segs_generic, 256, S); break;
        }
        return;
    }
    const dim3 grid((unsigned) H, s.rows ? (unsigned) T : 1u);
    auto go = [&](auto seq, auto row, unsigned block, auto... generic_s) {
        if (s.rows) hipLaunchKernelGGL(row, grid, dim3(block), 0, st, r, k, v, u, u_per_chan, w, w_mode, s.rows, s.off, out, H, generic_s...);
        else hipLaunchKernelGGL(seq, grid, dim3(block), 0, st, r, k, v, u, u_per_chan, w, w_mode, s.in + s.off, s.out + s.off, out, T, H, generic_s...);
    };
    switch (S) {
        case 64: go(k_wkv6<64>, k_wkv6_rows<64>, 64); break;
        case 32: go(k_wkv6<32>, k_wkv6_rows<32>, 64); break;
        case 16: go(k_wkv6<16>, k_wkv6_rows<16>, 64); break;
        case 8:  go(k_wkv6<8>, k_wkv6_rows<8>, 64); break;
        default: go(k_wkv6_generic, k_wkv6_rows_generic, 256, S); break;
    }
}

// wkv7: one wave per head, lane i owns value row i of state[h][i, :].
template <int S>
__device__ __forceinline__ void wkv7_body(const float * r, const float * w, const float * k, const float * v, const float * a, const float * b,
                                          const float * state_in, float * state_out, float * out, int64_t t0, int64_t t1, int64_t H) {
    __shared__ float l_r[S], l_w[S], l_k[S], l_a[S], l_b[S];
    const int64_t h = blockIdx.x;
    const int i = threadIdx.x;
    const int64_t D = H * S;
    float s[S];
    if (i < S) {
#pragma unroll
        for (int j = 0; j < S; j += 4) {
            const float4 q = *reinterpret_cast<const float4 *>(state_in + h * S * S + (int64_t) i * S + j);
            s[j] = q.x; s[j + 1] = q.y; s[j + 2] = q.z; s[j + 3] = q.w;
        }
    }
    for (int64_t t = t0; t < t1; t++) {
        __syncthreads();
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
        }
    }
    if (i < S) {
#pragma unroll
        for (int j = 0; j < S; j += 4)
            *reinterpret_cast<float4 *>(state_out + h * S * S + (int64_t) i * S + j) = make_float4(s[j], s[j + 1], s[j + 2], s[j + 3]);
    }
}

__device__ __forceinline__ void wkv7_body_generic(const float * r, const float * w, const float * k, const float * v, const float * a, const float * b,
                                                  const float * state_in, float * state_out, float * out, int64_t t0, int64_t t1, int64_t H, int64_t S) {
    const int64_t h = blockIdx.x;
    const int64_t D = H * S;
    for (int64_t i = threadIdx.x; i < S; i += blockDim.x) {
        for (int64_t t = t0; t < t1; t++) {
            const float * sin = (t == t0) ? state_in : state_out;
            const int64_t base = t * D + h * S;
            const float vi = v[base + i];
            float sa = 0.0f;
            for (int64_t j = 0; j < S; j++) sa += a[base + j] * sin[h * S * S + i * S + j];
            float res = 0.0f;
            for (int64_t j = 0; j < S; j++) {
                const float kv = vi * k[base + j];
                const float ns = (sin[h * S * S + i * S + j] * w[base + j] + kv) + sa * b[base + j];
                state_out[h * S * S + i * S + j] = ns;
                res += ns * r[base + j];
            }
            out[base + i] = res;
        }
    }
}

template <int S, int FORM>
__global__ __launch_bounds__(64) void k_wkv7(const float * __restrict__ r, const float * __restrict__ w, const float * __restrict__ k,
                                             const float * __restrict__ v, const float * __restrict__ a, const float * __restrict__ b,
                                             float * __restrict__ out, int64_t H, int64_t T, StateRef s) {
    const FormSpan f = form_span<FORM>(s, T);
    wkv7_body<S>(r, w, k, v, a, b, f.in, f.out, out, f.t0, f.t1, H);
}

template <int FORM>
__global__ __launch_bounds__(256) void k_wkv7_generic(const float * __restrict__ r, const float * __restrict__ w, const float * __restrict__ k,
                                                      const float * __restrict__ v, const float * __restrict__ a, const float * __restrict__ b,
                                                      float * __restrict__ out, int64_t H, int64_t T, int64_t S, StateRef s) {
    const FormSpan f = form_span<FORM>(s, T);
    wkv7_body_generic(r, w, k, v, a, b, f.in, f.out, out, f.t0, f.t1, H, S);
}

void launch_wkv7(const float * r, const float * w, const float * k, const float * v, const float * a, const float * b,
                 const StateRef & s, float * out, int64_t T, int64_t H, int64_t S, hipStream_t st) {
    const dim3 grid((unsigned) H, form_grid_y(s, T));
    with_form(s, [&](auto form) {
        constexpr int F = decltype(form)::value;
        auto go = [&](auto kern, unsigned block, auto... generic_s) {
            hipLaunchKernelGGL(kern, grid, dim3(block), 0, st, r, w, k, v, a, b, out, H, T, generic_s..., s);
        };
        switch (S) {
            case 64: go(k_wkv7<64, F>, 64); break;
            case 32: go(k_wkv7<32, F>, 64); break;
            default: go(k_wkv7_generic<F>, 256, S); break;
        }
    });
}

// ---------------------------------------------------------------------------------------------------------------
// Replay (rwkv_mi_batch_eval_draft). A recurrent state cannot be cut back: after a ragged pass over x0 d1 .. dk a slot's other buffer holds
// the state after dk, and when only keep < 1 + k of those tokens stand it is of no use. The pass therefore stashes, per layer and token, what
// its recurrences read (DraftStash: the inputs of the layer's WKV body and the two token-shift inputs), and once keep[i] is known on the
// device the replay entry point of each body runs segment i's first keep[i] tokens again from the slot's CURRENT buffer, which the pass has
// not touched, into the other one: exactly the statements of a ragged pass over those tokens. A segment whose whole draft stands returns at
// once -- the pass has left the right state. The bodies' per-token output goes to a plane of the stash nobody reads.
// ---------------------------------------------------------------------------------------------------------------

// src[i][0 .. plane) -> dst + i * plane, i < n: the planes of a layer the pass is about to overwrite
__global__ __launch_bounds__(256) void k_draft_stash(DraftStashSrc s, float * __restrict__ dst, int64_t plane) {
    for (int64_t idx = (int64_t) blockIdx.x * 256 + threadIdx.x; idx < plane; idx += (int64_t) gridDim.x * 256)
        for (int i = 0; i < s.n; i++) dst[(int64_t) i * plane + idx] = s.src[i][idx];
}

void launch_draft_stash(const DraftStashSrc & s, float * dst, int64_t plane, hipStream_t st) {
    const unsigned grid = (unsigned) ((plane + 255) / 256 < 4096 ? (plane + 255) / 256 : 4096);
    hipLaunchKernelGGL(k_draft_stash, dim3(grid), dim3(256), 0, st, s, dst, plane);
}

// what a replay block works on: its segment, how much of it stands (0: nothing to do), its layer's planes
struct ReplayBlock { SegState seg; int64_t t1; const float * in; float * sink; int64_t so; };
__device__ __forceinline__ ReplayBlock replay_block(const DraftStash & d, const SegState * __restrict__ segs, const uint32_t * __restrict__ keep) {
    ReplayBlock b;
    b.seg = segs[blockIdx.y];
    const int64_t kp = keep[blockIdx.y];
    b.t1 = kp < (int64_t) (b.seg.t1 - b.seg.t0) ? b.seg.t0 + kp : 0;   // (the whole workgroup takes the same way: no barrier is left waiting)
    b.in = d.base + (int64_t) blockIdx.z * d.planes() * d.plane;
    b.sink = const_cast<float *>(b.in) + (int64_t) (d.n_in + 2) * d.plane;
    b.so = (d.layer0 + (int64_t) blockIdx.z) * d.per_layer;
    return b;
}

__global__ __launch_bounds__(256) void k_wkv4_replay(DraftStash d, const DraftLayer * __restrict__ lw, const SegState * __restrict__ segs,
                                                     const uint32_t * __restrict__ keep, int64_t D) {
    const ReplayBlock b = replay_block(d, segs, keep);
    if (!b.t1) return;
    const DraftLayer w = lw[blockIdx.z];
    wkv4_body(b.in, b.in + d.plane, b.in + 2 * d.plane, w.u, w.w, b.seg.in + b.so + 2 * D, b.seg.out + b.so + 2 * D, b.sink, b.seg.t0, b.t1, D);
}

// RWKV-5: r, k, v stashed, u and w the layer's vectors (w_mode < 2); RWKV-6: w stashed as the fourth plane (w_mode 2)
template <int S>
__global__ __launch_bounds__(64) void k_wkv6_replay(DraftStash d, const DraftLayer * __restrict__ lw, int u_per_chan, int w_mode,
                                                    const SegState * __restrict__ segs, const uint32_t * __restrict__ keep, int64_t H) {
    const ReplayBlock b = replay_block(d, segs, keep);
    if (!b.t1) return;
    const DraftLayer w = lw[blockIdx.z];
    const int64_t so = b.so + 2 * H * S;
    wkv6_body<S>(b.in, b.in + d.plane, b.in + 2 * d.plane, w.u, u_per_chan, w_mode == 2 ? b.in + 3 * d.plane : w.w, w_mode,
                 b.seg.in + so, b.seg.out + so, b.sink, b.seg.t0, b.t1, H);
}

__global__ __launch_bounds__(256) void k_wkv6_replay_generic(DraftStash d, const DraftLayer * __restrict__ lw, int u_per_chan, int w_mode,
                                                             const SegState * __restrict__ segs, const uint32_t * __restrict__ keep, int64_t H, int64_t S) {
    const ReplayBlock b = replay_block(d, segs, keep);
    if (!b.t1) return;
    const DraftLayer w = lw[blockIdx.z];
    const int64_t so = b.so + 2 * H * S;
    wkv6_body_generic(b.in, b.in + d.plane, b.in + 2 * d.plane, w.u, u_per_chan, w_mode == 2 ? b.in + 3 * d.plane : w.w, w_mode,
                      b.seg.in + so, b.seg.out + so, b.sink, b.seg.t0, b.t1, H, S);
}

template <int S>
__global__ __launch_bounds__(64) void k_wkv7_replay(DraftStash d, const SegState * __restrict__ segs, const uint32_t * __restrict__ keep, int64_t H) {
    const ReplayBlock b = replay_block(d, segs, keep);
    if (!b.t1) return;
    const int64_t so = b.so + 2 * H * S;
    wkv7_body<S>(b.in, b.in + d.plane, b.in + 2 * d.plane, b.in + 3 * d.plane, b.in + 4 * d.plane, b.in + 5 * d.plane,
                 b.seg.in + so, b.seg.out + so, b.sink, b.seg.t0, b.t1, H);
}

__global__ __launch_bounds__(256) void k_wkv7_replay_generic(DraftStash d, const SegState * __restrict__ segs, const uint32_t * __restrict__ keep,
                                                             int64_t H, int64_t S) {
    const ReplayBlock b = replay_block(d, segs, keep);
    if (!b.t1) return;
    const int64_t so = b.so + 2 * H * S;
    wkv7_body_generic(b.in, b.in + d.plane, b.in + 2 * d.plane, b.in + 3 * d.plane, b.in + 4 * d.plane, b.in + 5 * d.plane,
                      b.seg.in + so, b.seg.out + so, b.sink, b.seg.t0, b.t1, H, S);
}

// the two token-shift carries of a replayed segment: what the segment form of k_mix leaves at a segment's last token, for token t0 + keep - 1 -- the ffn
// mix's input at so, the att mix's at so + D
__global__ __launch_bounds__(256) void k_draft_carry(DraftStash d, const SegState * __restrict__ segs, const uint32_t * __restrict__ keep, int64_t D) {
    const ReplayBlock b = replay_block(d, segs, keep);
    const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (!b.t1 || i >= D) return;
    const int64_t at = (b.t1 - 1) * D + i;
    b.seg.out[b.so + i] = b.in[(int64_t) (d.n_in + 1) * d.plane + at];
    b.seg.out[b.so + D + i] = b.in[(int64_t) d.n_in * d.plane + at];
}

void launch_draft_replay(const DraftStash & d, const DraftLayer * lw, int arch_major, int arch_minor, const SegState * segs, int64_t n_segs,
                         const uint32_t * keep, int64_t n_layers, int64_t D, int64_t H, int64_t S, hipStream_t st) {
    const unsigned n = (unsigned) n_segs, L = (unsigned) n_layers;
    if (arch_major == 4) {
        hipLaunchKernelGGL(k_wkv4_replay, dim3((unsigned) ((D + 255) / 256), n, L), dim3(256), 0, st, d, lw, segs, keep, D);
    } else if (arch_major <= 6) {
        const int u_per_chan = (arch_major == 6 || arch_minor >= 2) ? 1 : 0, w_mode = arch_major == 6 ? 2 : u_per_chan;
        const dim3 grid((unsigned) H, n, L);
        auto go = [&](auto kern, unsigned block, auto... generic_s) {
            hipLaunchKernelGGL(kern, grid, dim3(block), 0, st, d, lw, u_per_chan, w_mode, segs, keep, H, generic_s...);
        };
        switch (S) {
            case 64: go(k_wkv6_replay<64>, 64); break;
            case 32: go(k_wkv6_replay<32>, 64); break;
            case 16: go(k_wkv6_replay<16>, 64); break;
            case 8:  go(k_wkv6_replay<8>, 64); break;
            default: go(k_wkv6_replay_generic, 256, S); break;
        }
    } else {
        const dim3 grid((unsigned) H, n, L);
        auto go = [&](auto kern, unsigned block, auto... generic_s) { hipLaunchKernelGGL(kern, grid, dim3(block), 0, st, d, segs, keep, H, generic_s...); };
        switch (S) {
            case 64: go(k_wkv7_replay<64>, 64); break;
            case 32: go(k_wkv7_replay<32>, 64); break;
            default: go(k_wkv7_replay_generic, 256, S); break;
        }
    }
    hipLaunchKernelGGL(k_draft_carry, dim3((unsigned) ((D + 255) / 256), n, L), dim3(256), 0, st, d, segs, keep, D);
}

// ---------------------------------------------------------------------------------------------------------------
// Group norm (+ v7 bonus, + gate), v7 key prep: one wave per (token, head). The v7 value mix.
// ---------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_groupnorm(float * __restrict__ x, const float * __restrict__ lw, const float * __restrict__ lb, float eps,
                                                   const float * __restrict__ gate, const float * __restrict__ v7_k, const float * __restrict__ v7_r,
                                                   const float * __restrict__ v7_v, const float * __restrict__ v7_rk, int64_t TH, int64_t H, int64_t S) {
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
    float bonus = 0.0f;
    if (v7_k) {
        float p = 0.0f;
        for (int64_t j = lane; j < S; j += WAVE) p += (v7_k[base + j] * v7_r[base + j]) * v7_rk[h * S + j];
        bonus = wave_sum_f(p);
    }
    for (int64_t j = lane; j < S; j += WAVE) {
        float y = groupnorm_elem(x[base + j], mean, scale, lw[h * S + j], lb[h * S + j]);
        if (v7_k) y += v7_v[base + j] * bonus;
        if (gate) y *= gate[base + j];
        x[base + j] = y;
    }
}

void launch_groupnorm(float * x, const float * lw, const float * lb, float eps, const float * gate,
                      const float * v7_k, const float * v7_r, const float * v7_v, const float * v7_rk,
                      int64_t T, int64_t H, int64_t S, hipStream_t st) {
    const int64_t TH = T * H;
    hipLaunchKernelGGL(k_groupnorm, dim3((unsigned)((TH + 3) / 4)), dim3(256), 0, st, x, lw, lb, eps, gate, v7_k, v7_r, v7_v, v7_rk, TH, H, S);
}

__global__ __launch_bounds__(256) void k_v7_kprep(const float * __restrict__ k, const float * __restrict__ a, const float * __restrict__ k_k,
                                                  const float * __restrict__ k_a, float * __restrict__ k_out, float * __restrict__ neg_kk,
                                                  float * __restrict__ kk_a, int64_t TH, int64_t H, int64_t S) {
    const int lane = threadIdx.x & 63;
    const int64_t th = (int64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
    if (th >= TH) return;
    const int64_t h = th % H;
    const int64_t base = th * S;
    float p = 0.0f;
    for (int64_t j = lane; j < S; j += WAVE) { const float t = k[base + j] * k_k[h * S + j]; p += t * t; }
    const float sum = wave_sum_f(p);
    const float scale = 1.0f / fmaxf(sqrtf(sum), 1e-12f);
    for (int64_t j = lane; j < S; j += WAVE) {
        const float kv = k[base + j], av = a[base + j];
        const float kk = (kv * k_k[h * S + j]) * scale;
        const float ka = kv * k_a[h * S + j];
        const float aka = av * ka;
        k_out[base + j] = kv + (aka - ka);
        neg_kk[base + j] = -kk;
        kk_a[base + j] = kk * av;
    }
}

void launch_v7_kprep(const float * k, const float * a, const float * k_k, const float * k_a, float * k_out, float * neg_kk, float * kk_a,
                     int64_t T, int64_t H, int64_t S, hipStream_t st) {
    const int64_t TH = T * H;
    hipLaunchKernelGGL(k_v7_kprep, dim3((unsigned)((TH + 3) / 4)), dim3(256), 0, st, k, a, k_k, k_a, k_out, neg_kk, kk_a, TH, H, S);
}

__global__ __launch_bounds__(256) void k_v7_vmix(float * __restrict__ v, const float * __restrict__ v_first, const float * __restrict__ gate, int64_t n) {
    for (int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t) gridDim.x * 256) { const float dv = (v_first[i] - v[i]) * gate[i]; v[i] = v[i] + dv; }
}
void launch_v7_vmix(float * v, const float * v_first, const float * gate, int64_t n, hipStream_t st) {
    const unsigned grid = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(k_v7_vmix, dim3(grid), dim3(256), 0, st, v, v_first, gate, n);
}

}  // namespace rwkvmi
