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
// k_logprob_rows (rwkv_mi_*set_logprobs) is the same reduction for the token a draw has just emitted, plus the row's top-N: see below.
#include "kdev.h"
#include "model.h"

namespace rwkvmi {

// One body, several entry points (the convention of sampling.hip and kernels.hip): k_score_rows and k_logprob_rows both reduce a row through
// these two functions, so the log-prob a draw reports for its token is, bit for bit, the one k_score_rows gives that row with that target.

// The row maximum and its first index (k_argmax). Thread 0 returns the index (0x7fffffff when nothing compares greater than -inf) and has
// written the maximum to *l_m; the other threads read it behind the barrier score_row_lse starts with.
__device__ __forceinline__ int score_row_max(const float * __restrict__ logits, int n, float * l_m) {
    __shared__ float l_v[16];
    __shared__ int l_i[16];
    const int NT = blockDim.x;
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
        *l_m = best;
    }
    return bi;
}

// m + log(S), S = sum_j exp((double) l[j] - m) in the fixed order of the file's head; the value is thread 0's (the others return 0).
// Called by the whole workgroup after score_row_max.
__device__ __forceinline__ double score_row_lse(const float * __restrict__ logits, int n, const float * l_m) {
    __shared__ double l_s[16];
    const int NT = blockDim.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    const double m = (double) *l_m;
    double acc = 0.0;
    int i = threadIdx.x;
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
    if (threadIdx.x != 0) return 0.0;
    double S = 0.0;
    for (int w = 0; w < (NT >> 6); w++) S += l_s[w];
    return m + log(S);
}

// the log-prob of a logit of the row, rounded to f32 once
__device__ __forceinline__ float score_logprob(float l, double lse) { return (float) ((double) l - lse); }

__global__ __launch_bounds__(1024) void k_score_rows(const float * __restrict__ logits_all, int n, const uint32_t * __restrict__ targets /* may be NULL */,
                                                     float * __restrict__ logprobs /* may be NULL */, uint32_t * __restrict__ argmax /* may be NULL */) {
    __shared__ float l_m;
    const int64_t row = blockIdx.x;
    const float * __restrict__ logits = logits_all + row * (int64_t) n;
    const int bi = score_row_max(logits, n, &l_m);
    if (threadIdx.x == 0 && argmax) argmax[row] = bi == 0x7fffffff ? 0u : (uint32_t) bi;
    if (!logprobs) return;
    // ---- log-probability of the target (the branch is uniform over the workgroup) ----
    const uint32_t target = targets ? targets[row] : UINT32_MAX;
    if (target >= (uint32_t) n) {   // RWKV_MI_NO_TARGET (an index behind the row is never read)
        if (threadIdx.x == 0) logprobs[row] = 0.0f;
        return;
    }
    const double lse = score_row_lse(logits, n, &l_m);
    if (threadIdx.x == 0) logprobs[row] = score_logprob(logits[target], lse);
}

// ---- the report of a draw (rwkv_mi_*set_logprobs): the log-prob of the token a row has just emitted and the row's top_n alternatives ----
// Where a logit ranks: by value descending, then by index ascending; a NaN never ranks (key 0), -inf ranks last among the rest, -0 ranks
// as +0. The key is the logit's bit pattern made monotone in the upper word and the complement of the index in the lower one: the keys
// of a row are distinct, a larger key ranks earlier, and the largest key of all is the token k_argmax picks.
__device__ __forceinline__ unsigned long long rank_key(float v, int j) {
    if (v != v) return 0ull;
    if (v == 0.0f) v = 0.0f;
    uint32_t u = __float_as_uint(v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long) u << 32) | (unsigned long long) (0xFFFFFFFFu - (uint32_t) j);
}

// One body for k_logprob_rows and its live form. chosen = the score of the row's token (the word the draw has just written), by the two
// functions k_score_rows is made of. Then top_n sweeps over the row: sweep k finds the largest key below the key sweep k - 1 found --
// per thread over j = i, i + 1024, ..., the 64 lanes by the xor butterfly, the waves through LDS (two buffers in turn: one barrier per
// sweep). A maximum of distinct integers is the same in any order, so the selection is exact and depends on the row's logits alone; no
// atomics. A sweep that finds nothing ends the list: the remaining entries are RWKV_MI_NO_TOKEN / -inf.
// Cost: the row is read 2 + top_n times, from L2 after the first; the float64 exps of the sum are one read's worth of 64 per thread.
__device__ __forceinline__ void logprob_row_body(const float * __restrict__ logits, int n, uint32_t token, int top_n,
                                                 float * __restrict__ chosen, uint32_t * __restrict__ top_ids, float * __restrict__ top_lp) {
    __shared__ float l_m;
    __shared__ unsigned long long l_k[2][16];
    (void) score_row_max(logits, n, &l_m);
    const double lse = score_row_lse(logits, n, &l_m);
    const int tid = threadIdx.x, NT = blockDim.x;
    if (tid == 0) *chosen = token < (uint32_t) n ? score_logprob(logits[token], lse) : 0.0f;   // (an index behind the row is never read)
    unsigned long long bound = ~0ull;
    int k = 0;
    for (; k < top_n; k++) {
        unsigned long long best = 0ull;
        int i = tid;
        for (; i + 7 * NT < n; i += 8 * NT) {   // 8 loads in flight per trip
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) v[u] = logits[i + u * NT];
#pragma unroll
            for (int u = 0; u < 8; u++) { const unsigned long long key = rank_key(v[u], i + u * NT); if (key < bound && key > best) best = key; }
        }
        for (; i < n; i += NT) { const unsigned long long key = rank_key(logits[i], i); if (key < bound && key > best) best = key; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const unsigned long long ok = __shfl_xor(best, o, WAVE); if (ok > best) best = ok; }
        if ((tid & 63) == 0) l_k[k & 1][tid >> 6] = best;
        __syncthreads();
        for (int w = 0; w < (NT >> 6); w++) { const unsigned long long wk = l_k[k & 1][w]; if (wk > best) best = wk; }
        if (best == 0ull) break;   // (uniform: every thread holds the workgroup's maximum)
        bound = best;
        if (tid == 0) {
            const uint32_t id = 0xFFFFFFFFu - (uint32_t) (best & 0xFFFFFFFFull);
            top_ids[k] = id;
            top_lp[k] = score_logprob(logits[id], lse);
        }
    }
    if (tid == 0) for (; k < top_n; k++) { top_ids[k] = UINT32_MAX; top_lp[k] = -INFINITY; }
}

// Row form: grid = rows, one workgroup per row; row r's token is tokens[r], its record goes to chosen[r], top_ids[r][top_n], top_lp[r][top_n].
__global__ __launch_bounds__(1024) void k_logprob_rows(const float * __restrict__ logits_all, int n, const uint32_t * __restrict__ tokens, int top_n,
                                                       float * __restrict__ chosen, uint32_t * __restrict__ top_ids, float * __restrict__ top_lp) {
    const size_t r = blockIdx.x;
    logprob_row_body(logits_all + r * (size_t) n, n, tokens[r], top_n, chosen + r, top_ids + r * (size_t) top_n, top_lp + r * (size_t) top_n);
}

// ... and behind the row's LIVE WORD (rwkv_mi_batch_decode_until; as the row samplers' live argument): a retired row writes nothing. The launch
// sits between the draw and k_stop_rows, so the step at which a row retires is reported. The whole workgroup takes the branch together.
__global__ __launch_bounds__(1024) void k_logprob_rows_live(const float * __restrict__ logits_all, int n, const uint32_t * __restrict__ tokens, int top_n,
                                                            float * __restrict__ chosen, uint32_t * __restrict__ top_ids, float * __restrict__ top_lp,
                                                            const uint32_t * __restrict__ live) {
    const size_t r = blockIdx.x;
    if (!live[r]) return;
    logprob_row_body(logits_all + r * (size_t) n, n, tokens[r], top_n, chosen + r, top_ids + r * (size_t) top_n, top_lp + r * (size_t) top_n);
}

// ... and behind a LANE of rwkv_mi_batch_serve_ex (model.h, ServeTables), between the choice and the scheduler: a lane whose draw word is 0 --
// it is fed a prompt token, or is dead -- writes nothing. The others serve request q = req[r], which has emitted j = lens[q] tokens before
// this one (the scheduler behind this launch is what advances lens): the record goes to entry (j, q) of buffers laid out [position][request],
// so the requests that follow each other on a lane never meet. A position the request's token row does not hold (j >= stride) is not
// reported. The whole workgroup takes each branch together.
__global__ __launch_bounds__(1024) void k_logprob_rows_serve(const float * __restrict__ logits_all, int n, const uint32_t * __restrict__ tokens, int top_n,
                                                             float * __restrict__ chosen, uint32_t * __restrict__ top_ids, float * __restrict__ top_lp,
                                                             const uint32_t * __restrict__ draw, const uint32_t * __restrict__ req,
                                                             const uint32_t * __restrict__ lens, uint32_t stride, uint32_t n_requests) {
    const size_t r = blockIdx.x;
    if (!draw[r]) return;
    const uint32_t q = req[r];
    if (q >= n_requests) return;   // (a lane that draws has a request; a word that names none is never used as an index)
    const uint32_t j = lens[q];
    if (j >= stride) return;
    const size_t at = (size_t) j * n_requests + q;
    logprob_row_body(logits_all + r * (size_t) n, n, tokens[r], top_n, chosen + at, top_ids + at * (size_t) top_n, top_lp + at * (size_t) top_n);
}

// ---- one step of the beam search (rwkv_mi_batch_decode_beam): the rows' candidates, then the selection of each group ----
// The candidates of a row are the report's top-N at N = the beam width, through the report's body: ids and f32 log-probs in the report's order,
// bit for bit what k_logprob_rows gives the row. Behind the row's own words (the pattern of the _live kernels): a finished hypothesis, and one
// whose score is -inf, offers nothing of its logits and its workgroup returns before it reads one. (The body's `chosen` is asked for no token:
// it writes the 0 of an index behind the row into a word nobody reads.)
__global__ __launch_bounds__(1024) void k_beam_rows(const float * __restrict__ logits_all, int n, int width, const double * __restrict__ score,
                                                    const uint32_t * __restrict__ finished, float * __restrict__ chosen, uint32_t * __restrict__ cand_ids,
                                                    float * __restrict__ cand_lp) {
    const size_t r = blockIdx.x;
    if (finished[r] || !(score[r] > -INFINITY)) return;
    logprob_row_body(logits_all + r * (size_t) n, n, UINT32_MAX, width, chosen + r, cand_ids + r * (size_t) width, cand_lp + r * (size_t) width);
}

// The selection, one wave per group of W = t.width hypotheses (rows g W .. g W + W - 1); lane i < W holds hypothesis i.
// Candidates, numbered c = parent * W + rank: a live parent with a finite score offers its W (id, lp) pairs with the cumulative score
// (double) score[parent] + (double) lp, kept as double -- not the pairs without a token or whose lp is not above -inf (-inf, or the NaN of a
// row that holds one); a finished parent with a finite score offers itself once, at rank 0, with its score and no token; a score of -inf
// offers nothing. The W best by score descending, then c ascending (parent, then rank) -- a total order on distinct c, so the result does not
// depend on the order of execution: round j finds the best candidate behind the one round j - 1 found, per lane over c = lane, lane + 64, ...,
// the 64 lanes by the xor butterfly (32, 16, ... 1), and lane j keeps it. Every lane reads what it needs of the group into registers before any
// lane writes (the words are rewritten in place).
// Hypothesis j then becomes selection j: its token goes to tokens[row] (where the row's next embedding lookup reads it) and to the history;
// a finished one is fed the token it was fed before (a dead step) and records no token; one for which no candidate is left is dead: score
// -inf, parent itself, finished, length 0. other[row].in = used[row of the parent].out re-parents the next pass; other[row].out stays.
// live_count moves by the change of the group's unfinished hypotheses: an integer sum, the same in any order.
__global__ __launch_bounds__(64) void k_beam_select(BeamTables t, size_t rows, uint32_t * tokens, uint32_t step, const RowState * used, RowState * other) {
    constexpr int Q = (RWKV_MI_TOP_MAX * RWKV_MI_TOP_MAX + 63) / 64;   // candidates per lane
    const int W = (int) t.width, lane = threadIdx.x;
    const size_t r0 = (size_t) blockIdx.x * (size_t) W;
    const bool mine = lane < W;
    double sc = -INFINITY;
    uint32_t fin = 1u, len = 0u, fed = 0u;
    if (mine) { sc = t.score[r0 + lane]; fin = t.finished[r0 + lane]; len = t.len[r0 + lane]; fed = tokens[r0 + lane]; }
    double cs[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) {
        const int c = lane + 64 * q;
        const bool in = c < W * W;
        const int p = in ? c / W : 0, k = in ? c % W : 0;
        const double ps = __shfl(sc, p, WAVE);
        const uint32_t pf = __shfl(fin, p, WAVE);
        cs[q] = -INFINITY;
        if (!in || !(ps > -INFINITY)) continue;
        if (pf) { if (k == 0) cs[q] = ps; continue; }
        const size_t at = (r0 + (size_t) p) * (size_t) W + (size_t) k;
        const float lp = t.cand_lp[at];
        if (t.cand_ids[at] != UINT32_MAX && lp > -INFINITY) cs[q] = ps + (double) lp;
    }
    double prev_s = INFINITY, my_s = -INFINITY;
    int prev_c = -1, my_c = 0x7fffffff;
    for (int j = 0; j < W; j++) {
        double bs = -INFINITY;
        int bc = 0x7fffffff;
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const int c = lane + 64 * q;
            const double s = cs[q];
            if (!(s > -INFINITY) || !(s < prev_s || (s == prev_s && c > prev_c))) continue;
            if (s > bs || (s == bs && c < bc)) { bs = s; bc = c; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double os = __shfl_xor(bs, o, WAVE);
            const int oc = __shfl_xor(bc, o, WAVE);
            if (os > bs || (os == bs && oc < bc)) { bs = os; bc = oc; }
        }
        if (lane == j) { my_s = bs; my_c = bc; }
        if (bc == 0x7fffffff) break;   // (uniform: every lane holds the wave's best; nothing is left for the later rounds either)
        prev_s = bs; prev_c = bc;
    }
    const bool dead = my_c == 0x7fffffff;
    const int parent = dead ? (mine ? lane : 0) : my_c / W;
    const uint32_t p_fin = __shfl(fin, parent, WAVE), p_len = __shfl(len, parent, WAVE), p_fed = __shfl(fed, parent, WAVE);
    uint32_t tok = UINT32_MAX, n_fin = 1u, n_len = 0u, n_fed = fed;
    float lp = 0.0f;
    if (mine && !dead) {
        n_fed = p_fed; n_len = p_len;
        if (!p_fin) {
            const size_t at = (r0 + (size_t) parent) * (size_t) W + (size_t) (my_c % W);
            tok = t.cand_ids[at]; lp = t.cand_lp[at];
            n_fed = tok; n_len = p_len + 1u; n_fin = 0u;
            for (uint32_t e = 0; e < t.n_end; e++) if (tok == t.end_tokens[e]) n_fin = 1u;
        }
    }
    const int before = __popcll(__ballot(mine && !fin)), after = __popcll(__ballot(mine && !n_fin));
    if (lane == 0 && t.live_count && after != before) atomicAdd(t.live_count, (uint32_t) (after - before));
    if (!mine) return;
    const size_t r = r0 + (size_t) lane, h = (size_t) step * rows + r;
    t.score[r] = dead ? -INFINITY : my_s; t.finished[r] = n_fin; t.len[r] = n_len;
    tokens[r] = n_fed;
    t.hist_tok[h] = tok; t.hist_parent[h] = (uint32_t) parent; t.hist_lp[h] = lp;
    if (other) other[r].in = used[r0 + (size_t) parent].out;
}

void launch_beam_rows(const float * logits, int64_t rows, int n, const BeamTables & t, hipStream_t st) {
    if (rows > 0) hipLaunchKernelGGL(k_beam_rows, dim3((unsigned) rows), dim3(1024), 0, st, logits, n, (int) t.width, t.score, t.finished, t.chosen, t.cand_ids, t.cand_lp);
}

void launch_beam_select(const BeamTables & t, int64_t groups, uint32_t * tokens, uint32_t step, const RowState * used, RowState * other, hipStream_t st) {
    if (groups > 0) hipLaunchKernelGGL(k_beam_select, dim3((unsigned) groups), dim3(64), 0, st, t, (size_t) groups * t.width, tokens, step, used, other);
}

void launch_score_rows(const float * logits, int64_t rows, int n, const uint32_t * targets, float * logprobs, uint32_t * argmax, hipStream_t st) {
    if (rows > 0 && (logprobs || argmax)) hipLaunchKernelGGL(k_score_rows, dim3((unsigned) rows), dim3(1024), 0, st, logits, n, targets, logprobs, argmax);
}

void launch_logprob_rows(const float * logits, int64_t rows, int n, const uint32_t * tokens, int top_n, float * chosen, uint32_t * top_ids, float * top_lp,
                         const uint32_t * live, hipStream_t st) {
    if (rows <= 0) return;
    if (live) hipLaunchKernelGGL(k_logprob_rows_live, dim3((unsigned) rows), dim3(1024), 0, st, logits, n, tokens, top_n, chosen, top_ids, top_lp, live);
    else hipLaunchKernelGGL(k_logprob_rows, dim3((unsigned) rows), dim3(1024), 0, st, logits, n, tokens, top_n, chosen, top_ids, top_lp);
}

void launch_logprob_rows_serve(const float * logits, int64_t lanes, int n, const uint32_t * tokens, int top_n, float * chosen, uint32_t * top_ids, float * top_lp,
                               const uint32_t * draw, const uint32_t * req, const uint32_t * lens, uint32_t stride, uint32_t n_requests, hipStream_t st) {
    if (lanes <= 0) return;
    hipLaunchKernelGGL(k_logprob_rows_serve, dim3((unsigned) lanes), dim3(1024), 0, st, logits, n, tokens, top_n, chosen, top_ids, top_lp, draw, req, lens, stride,
                       n_requests);
}

}  // namespace rwkvmi
