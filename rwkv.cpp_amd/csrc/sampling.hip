// sampling.hip -- temperature / top-k / top-p / min-p sampling on the device (the reference samples on the host from downloaded logits,
// python/sampling.py:10-52): [top-k mask,] softmax, nucleus cut-off [and min-p], p^(1/temperature), renormalise, draw -- one launch of one workgroup on the
// logits that are already in HBM; the chosen token lands where the next embedding lookup reads it, so a sampling decode loop
// never leaves the device (rwkv_mi_decode_sample). Semantics follow sample_probs() statement by statement:
//   probs = softmax(logits);  top_p == 0 -> 1;  temperature == 0 -> argmax;
//   top_p < 1: cutoff = the probability at which the descending cumulative sum first exceeds top_p; probs < cutoff -> 0;
//   temperature != 1: probs = (probs / max probs)^(1/temperature);  probs /= sum;  token = first index whose cumulative probability exceeds u.
// The cut-off is found without sorting: the largest threshold t (bisection over the float bit pattern, 31 reductions) with
// sum{p >= t} > top_p is exactly that probability. Sums are f32 in a fixed order (per-thread contiguous chunks, then a tree): runs
// are reproducible; against numpy's sequential cumsum the result can differ only when u or top_p falls within rounding of a boundary.
// Every draw is ONE body, draw_row, on ONE description of a row, DrawRow (model.h): the sampler's parameters, the draw counter of the row's
// sequence, its penalty and tables, its guide, its truncation and repetition settings. The body has three compile-time axes, and an entry
// point is an instantiation of them -- a call launches the one its DrawForm (model.h) names, so a call that uses none of a feature runs the
// code of before that feature, registers and all (tests/test_cpu_batch_until.py pins the four unset forms; DESIGN.md 6.15 has the table):
//   SRC     what the draw reads instead of the logit l[j]. PLAIN: l[j]. PEN (rwkv_mi_*_penalized):
//             adj[j] = (l[j] - (presence + (float) count[j] * frequency)) + bias[j]      where count[j] > 0;      l[j] + bias[j] elsewhere
//           (the reference's chat program, chat_with_bot.py:246-247 -- its loop runs over the tokens that have occurred -- then sample_logits'
//           logit_bias, sampling.py:27-36; every operation rounded to f32 in that order) from the sequence's occurrence table count[n] and its
//           optional bias table; a draw that records counts the chosen token afterwards. REP (rwkv_mi_*repetition_set; RepetitionLogits): the
//           penalised draw of a call that names a sequence with a setting {decay, repetition} -- the logit of an occurred token is divided or
//           multiplied by `repetition` in front of the penalty, and a sequence with decay != 1 keeps its occurrence row as floats that every
//           recorded draw multiplies by decay before it counts the pick. A row with {1, 1} draws as PEN does.
//   CUT     the row's truncation setting {top_k, min_p} is read (rwkv_mi_*truncation_set; cut_sample): mask -> softmax -> top-p and min-p,
//           intersected -> temperature. A row with top-k on runs select_stage in front of the body -- of the values above, all but the first
//           top_k in the order (value descending, index ascending) read -inf -- and the body on the stash; min-p is one more threshold of the
//           body, p >= (float) (min_p * p_max), combined with the top-p cut-off as the larger bit pattern. A row with {0, 0} draws as the form
//           without CUT does, statement for statement. The REP and GUIDED forms exist with CUT only.
//   GUIDED  (the row form only; rwkv_mi_batch_guide_*) a row whose slot has a guide attached, in state s, reads -inf instead of the value
//           above wherever the guide's next(s, j) is dead, and moves its state to next(s, token) afterwards; a row without one draws as the
//           unguided form does.
// The entry points: k_draw<SRC, CUT>, one workgroup on a context's logits; k_draw_rows<SRC, CUT, GUIDED>, one workgroup per row of a batch
// pass (rwkv_mi_batch_eval_sample / _decode_sample and their kin), behind the row's live word in rwkv_mi_batch_decode_until, whose k_stop_rows
// retires a row -- stop sequence or budget -- by rewriting its entries of the two row tables on the device; k_draft_accept_rows<FAMILY>, the
// walk of rwkv_mi_batch_eval_draft, which draws once per position. The logits themselves are never written. rwkv_mi_batch_serve puts a queue
// of requests behind the rows: k_serve_rows<DRAWS>, the scheduler that follows each pass's draw (the rows' live words are its draw words), and
// k_serve_reset<VEC>, which copies an admitted request's start state in; neither draws.
#include "kdev.h"
#include "model.h"

namespace rwkvmi {

__device__ __forceinline__ float block_sum_f(float v, float * red /* [32] */) {
    v = wave_sum_f(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float t = 0.0f;
    for (int w = 0; w < (int) (blockDim.x >> 6); w++) t += red[w];
    return t;
}

// splitmix64 -> uniform in [0, 1) with 24 bits
__device__ __forceinline__ float uniform01(unsigned long long seed, unsigned long long counter) {
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (counter + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return (float) (z >> 40) * (1.0f / 16777216.0f);
}

// f(j) over a thread's chunk, in the order of j
template <class F>
__device__ __forceinline__ void for_chunk(int cnt, F && f) { for (int j = 0; j < cnt; j++) f(j); }

// A thread's view of the scratch vector: element j of its chunk (the layout is explained at sample_body).
struct ProbVec {
    float * mem; int nt;
    __device__ __forceinline__ float get(int j) const { return mem[(size_t) j * nt]; }
    __device__ __forceinline__ void set(int j, float v) const { mem[(size_t) j * nt] = v; }
};

// Where sample_body takes the logit of element j of the thread's chunk from: first() in the pass that finds the maximum, again() in the
// pass that exponentiates. The plain source loads the logit both times.
struct PlainLogits {
    static constexpr bool stashes = false;   // (whether first() leaves the value in the scratch vector: the select stage stores it where not)
    const float * lg;
    __device__ __forceinline__ float first(int j, const ProbVec &) const { return lg[j]; }
    __device__ __forceinline__ float again(int j, const ProbVec &) const { return lg[j]; }
};
// The penalised source: first() computes the adjusted logit and STASHES it in the scratch vector, again() reads it back (the pass that
// exponentiates overwrites the element it has just read). Against recomputing it in the second pass: a thread's chunk is contiguous in
// the three tables, so the 64 lanes of a load touch 64 cache lines each time, while the scratch is laid out for the passes -- the stash
// costs one coalesced store and load per element and saves three such loads; the arithmetic is the same either way.
struct PenalisedLogits {
    static constexpr bool stashes = true;
    const float * lg; const uint32_t * count; const float * bias /* may be NULL */; float presence, frequency;
    __device__ __forceinline__ float first(int j, const ProbVec & pr) const {
        float a = lg[j];
        const uint32_t c = count[j];
        if (c) a = a - (presence + (float) c * frequency);   // (the reference's loop runs over the tokens that have occurred)
        if (bias) a = a + bias[j];
        pr.set(j, a);
        return a;
    }
    __device__ __forceinline__ float again(int j, const ProbVec & pr) const { return pr.get(j); }
};

// The penalised source of a sequence with a repetition setting (rwkv_mi_*repetition_set; model.h, DrawRow): the row's occurrence word o[j] is a
// float where the sequence is decaying (is_float), else (float) count[j], and the value is, every operation rounded to f32 in this order,
//   a = l[j];   o[j] > 0:  a = a > 0 ? a / repetition : a * repetition;  a = a - (presence + o[j] * frequency);      bias:  a = a + bias[j]
// ({1, 1}: the penalised source's adj[j], statement for statement). It stashes like the penalised source, so the guided source and the select
// stage take it unchanged. It only reads the row: what a recorded draw does to it follows the draw (rep_record).
struct RepetitionLogits {
    static constexpr bool stashes = true;
    const float * lg; const uint32_t * occ; const float * bias /* may be NULL */; float presence, frequency, repetition; bool is_float;
    __device__ __forceinline__ float first(int j, const ProbVec & pr) const {
        float a = lg[j];
        const uint32_t w = occ[j];
        const float o = is_float ? __uint_as_float(w) : (float) w;
        if (o > 0.0f) {
            a = a > 0.0f ? a / repetition : a * repetition;   // (0, -0, NaN and -inf take the multiply)
            a = a - (presence + o * frequency);
        }
        if (bias) a = a + bias[j];
        pr.set(j, a);
        return a;
    }
    __device__ __forceinline__ float again(int j, const ProbVec & pr) const { return pr.get(j); }
};

// make_src of a row with the setting `rep`: occ is the row's table
__device__ __forceinline__ auto rep_source(const float * lg, const uint32_t * occ, const float * bias, float presence, float frequency, const RepRow & rep) {
    const bool is_float = rep.decay != 1.0f;
    const float repetition = rep.repetition;
    return [=](int i0) { return RepetitionLogits{lg + i0, occ + i0, bias ? bias + i0 : nullptr, presence, frequency, repetition, is_float}; };
}

// What follows the draw of such a row when it records (every thread calls it: record is the row's). A decaying row is swept by the whole
// workgroup, o[j] = o[j] * decay in a pass of its own over the row in index order -- consecutive lanes, consecutive words, where the draw's
// reads of the table are a chunk per thread: riding the sweep on those reads cost 0.06-0.08 ms a step on the 7B, this pass DESIGN 6.14's
// figure -- and behind a barrier thread 0 adds 1.0f to the pick's entry; any other row counts + 1u. The body's barriers lie between the last
// read of the row in first() and the sweep.
__device__ __forceinline__ void rep_record(uint32_t * occ, int n, const RepRow & rep, uint32_t record, int pick) {
    if (!record) return;
    if (rep.decay == 1.0f) { if (threadIdx.x == 0) occ[pick] += 1u; return; }
    for (int j = threadIdx.x; j < n; j += blockDim.x) occ[j] = __float_as_uint(__uint_as_float(occ[j]) * rep.decay);
    __syncthreads();
    if (threadIdx.x == 0) occ[pick] = __float_as_uint(__uint_as_float(occ[pick]) + 1.0f);
}

// The guided source (the GUIDED forms of k_draw_rows): the value the row's draw would read anyway -- Inner is any of the three sources
// above -- with the mask applied LAST: -inf where the guide's transition from the row's state is dead. nx: the thread's chunk of
// the state's row of the dense table, contiguous like its chunk of the count table; NULL: the row has no guide and reads what Inner reads.
// first() stashes the value as the penalised source does, so again() neither reads the table a second time nor derives the value again.
template <class Inner>
struct GuidedLogits {
    static constexpr bool stashes = true;
    Inner in; const uint16_t * nx /* may be NULL */;
    __device__ __forceinline__ float first(int j, const ProbVec & pr) const {
        float a = in.first(j, pr);
        if (nx && nx[j] == GUIDE_DEAD) a = -INFINITY;
        pr.set(j, a);
        return a;
    }
    __device__ __forceinline__ float again(int j, const ProbVec & pr) const { return pr.get(j); }
};

// What sample_body reads behind the select stage: the scratch vector in both passes (the stage has left the masked values there).
struct StashedLogits {
    __device__ __forceinline__ float first(int j, const ProbVec & pr) const { return pr.get(j); }
    __device__ __forceinline__ float again(int j, const ProbVec & pr) const { return pr.get(j); }
};

// The order of top-k as an unsigned key: a larger value has a larger key, equal values (+0 and -0 among them) the same one, -inf the
// smallest key a number has, and a NaN -- which never ranks -- 0, below all of them.
__device__ __forceinline__ uint32_t rank_key(float a) {
    if (a != a) return 0u;
    if (a == 0.0f) return 0x80000000u;
    const uint32_t b = __float_as_uint(a);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// The select stage of a row with top-k on (0 < k < n), in front of sample_body: the values the draw would read -- src.first() over the
// thread's chunk, stashed in the scratch vector -- are ranked by (value descending, index ascending), and every one outside the first k is
// overwritten with -inf. The k-th largest key is found exactly by a byte-radix select, most significant byte first: a 256-bin histogram in
// LDS of the keys that share the prefix found so far (integer atomics: the counts do not depend on the order of arrival), from which wave
// 0 takes the bin that holds the k-th largest and the number of keys above it. The keys above the k-th largest number k - need, so `need`
// of the tied class survive: its members get ranks by index -- a thread's chunk is a contiguous ascending range, so a per-thread count, an
// exclusive scan over the threads and a walk of the chunk give them -- unless the whole class survives, when no rank is needed. A NaN is
// always dropped. Every thread takes the same branches (k and the LDS words are uniform); the stage ends behind a barrier, so its LDS
// words are fenced from the body's.
template <class Src>
__device__ __forceinline__ void select_stage(const Src & src, int cnt, uint32_t k, const ProbVec & pr) {
    __shared__ uint32_t c_hist[256];
    __shared__ uint32_t c_wave[16];
    __shared__ uint32_t c_digit, c_above, c_class;
    const int tid = threadIdx.x;
    for_chunk(cnt, [&](int j) { const float a = src.first(j, pr); if (!Src::stashes) pr.set(j, a); });
    uint32_t kth = 0u, need = k, tied = 0u;   // kth: the prefix of the k-th largest key; need: how many of the keys with that prefix survive
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) c_hist[tid] = 0u;
        __syncthreads();
        const uint32_t above_mask = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
        for_chunk(cnt, [&](int j) {
            const uint32_t key = rank_key(pr.get(j));
            if ((key & above_mask) == kth) atomicAdd(&c_hist[(key >> shift) & 255u], 1u);
        });
        __syncthreads();
        if (tid < 64) {
            // lane l holds bins 4 l .. 4 l + 3; suf: the keys in the bins of the lanes from l on, above: in those of the lanes behind l
            uint32_t h[4];
            for (int b = 0; b < 4; b++) h[b] = c_hist[4 * tid + b];
            const uint32_t own = h[0] + h[1] + h[2] + h[3];
            uint32_t suf = own;
            for (int o = 1; o < 64; o <<= 1) { const uint32_t v = __shfl_down(suf, o, WAVE); if (tid + o < 64) suf += v; }
            uint32_t above = suf - own;
            if (above < need && suf >= need) {   // (exactly one lane: the keys with the prefix number at least need >= 1)
                int b = 3;
                while (b > 0 && above + h[b] < need) { above += h[b]; b--; }
                c_digit = (uint32_t) (4 * tid + b); c_above = above; c_class = h[b];
            }
        }
        __syncthreads();
        kth |= c_digit << shift;
        need -= c_above;
        tied = c_class;
    }
    // need of the `tied` keys equal to kth survive, the lowest indices first
    uint32_t rank = 0u;
    if (tied != need) {
        uint32_t mine = 0u;
        for_chunk(cnt, [&](int j) { mine += rank_key(pr.get(j)) == kth ? 1u : 0u; });
        uint32_t inc = mine;
        for (int o = 1; o < 64; o <<= 1) { const uint32_t v = __shfl_up(inc, o, WAVE); if ((tid & 63) >= o) inc += v; }
        if ((tid & 63) == 63) c_wave[tid >> 6] = inc;
        __syncthreads();
        rank = inc - mine;
        for (int w = 0; w < (tid >> 6); w++) rank += c_wave[w];
    }
    for_chunk(cnt, [&](int j) {
        const uint32_t key = rank_key(pr.get(j));
        bool keep = key > kth;
        if (key == kth) { keep = rank < need; rank++; }
        if (!keep || key == 0u) pr.set(j, -INFINITY);
    });
    __syncthreads();
}

// What thread 0 does to a guided row's words after the draw (where the penalised rows count the token): the state moves along the picked
// token's transition; a dead pick -- all-NaN logits, or a caller's -inf bias on every allowed token -- leaves it and counts a miss. The
// state word is only ever written from the table (or by rwkv_mi_batch_guide_attach, which checks it), so it always indexes inside it.
__device__ __forceinline__ void guide_advance(const DrawRow & g, const uint16_t * state_row, int pick) {
    const uint16_t to = state_row[pick];
    if (to != GUIDE_DEAD) *g.state = to; else *g.misses += 1u;
}

// The sampler proper, shared by every entry point (the convention of the recurrence kernels and their row forms): k_draw hands it a context's
// row, k_draw_rows the row of blockIdx.x. Everything the workgroup does -- chunks, summation order, bisection, scan, draw -- is this
// function, so a row of the batch picks bit for bit the token the single-context sampler picks from the same logits.
// The scratch vector is laid out for the passes, not for the reader: token i0 + j of thread tid lives at probs[j * 1024 + tid], so the 64 lanes
// of a load touch two cache lines instead of 64 (a thread's chunk is contiguous in the logits; ~35 passes run over the probabilities).
// make_src(i0): the logit source of the thread whose chunk starts at token i0 (PlainLogits or PenalisedLogits).
template <class MakeSrc>
__device__ __forceinline__ int sample_body(MakeSrc && make_src, int n, float temperature, float top_p, float min_p /* 0: none */, float u_in,
                                           unsigned long long seed, unsigned long long * counter /* read and advanced by thread 0; may be NULL */,
                                           float * __restrict__ probs /* scratch of C * 1024 >= n floats, C = ceil(n / 1024) */,
                                           uint32_t * __restrict__ out_token, uint32_t * __restrict__ hist_word /* may be NULL */) {
    __shared__ float red[32];
    __shared__ float l_scan[1024];
    __shared__ int l_pick, l_last;
    __shared__ unsigned long long l_ctr;
    const int tid = threadIdx.x, NT = blockDim.x;
    const int C = (n + NT - 1) / NT;                 // contiguous chunk per thread
    const int i0 = tid * C, i1 = i0 + C < n ? i0 + C : n;
    const int cnt = i1 - i0;                         // (<= 0 for the threads behind the end)
    const ProbVec pr{probs + tid, NT};
    const auto src = make_src(i0);
    // softmax
    float m = -INFINITY;
    for_chunk(cnt, [&](int j) { m = fmaxf(m, src.first(j, pr)); });
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, WAVE));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    for (int w = 0; w < (NT >> 6); w++) m = fmaxf(m, red[w]);
    float part = 0.0f;
    for_chunk(cnt, [&](int j) { const float e = det_expf(src.again(j, pr) - m); pr.set(j, e); part += e; });
    const float total = block_sum_f(part, red);
    const float inv = 1.0f / total;
    for_chunk(cnt, [&](int j) { pr.set(j, pr.get(j) * inv); });
    if (top_p == 0.0f) top_p = 1.0f;
    int pick = -1;
    if (temperature == 0.0f) {
        // argmax, first index of the maximum
        float best = -1.0f; int bi = 0x7fffffff;
        for_chunk(cnt, [&](int j) { const float p = pr.get(j); if (p > best) { best = p; bi = i0 + j; } });
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(best, o, WAVE); const int oi = __shfl_xor(bi, o, WAVE);
            if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
        }
        __shared__ float l_bv[16]; __shared__ int l_bi[16];
        if ((tid & 63) == 0) { l_bv[tid >> 6] = best; l_bi[tid >> 6] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < (NT >> 6); w++) if (l_bv[w] > best || (l_bv[w] == best && l_bi[w] < bi)) { best = l_bv[w]; bi = l_bi[w]; }
            l_pick = bi;
        }
        __syncthreads();
        pick = l_pick;
    } else {
        unsigned cutoff_bits = 0u;
        if (top_p < 1.0f) {
            // largest bit pattern T with sum{p : bits(p) >= T} > top_p  (probabilities are non-negative floats: bit order = value order)
            unsigned T = 0u;
            // (when not even the sum over ALL probabilities exceeds top_p -- float rounding of the softmax -- the reference's
            //  argmax over an all-false mask is 0: the cut-off is the LARGEST probability, i.e. 1 * inv)
            float g0 = 0.0f;
            for_chunk(cnt, [&](int j) { g0 += pr.get(j); });
            g0 = block_sum_f(g0, red);
            const bool none = !(g0 > top_p);
            for (int bit = 30; bit >= 0; bit--) {
                const unsigned cand = T | (1u << bit);
                float g = 0.0f;
                for_chunk(cnt, [&](int j) { const float p = pr.get(j); g += __float_as_uint(p) >= cand ? p : 0.0f; });
                g = block_sum_f(g, red);
                if (g > top_p) T = cand;
            }
            cutoff_bits = none ? __float_as_uint(1.0f * inv) : T;
        }
        if (min_p != 0.0f) {
            // min-p, on the same distribution as the top-p cut-off: p survives where p >= (float) (min_p * p_max) as well -- the larger of
            // the two thresholds' bit patterns (non-negative floats: bit order = value order) in front of the pass below
            float pm = 0.0f;
            for_chunk(cnt, [&](int j) { pm = fmaxf(pm, pr.get(j)); });
            for (int o = 32; o > 0; o >>= 1) pm = fmaxf(pm, __shfl_xor(pm, o, WAVE));
            __syncthreads();
            if ((tid & 63) == 0) red[tid >> 6] = pm;
            __syncthreads();
            for (int w = 0; w < (NT >> 6); w++) pm = fmaxf(pm, red[w]);
            const unsigned floor_bits = __float_as_uint(min_p * pm);
            if (floor_bits > cutoff_bits) cutoff_bits = floor_bits;
        }
        const float it = 1.0f / temperature;
        part = 0.0f;
        for_chunk(cnt, [&](int j) {
            float p = pr.get(j);
            if (__float_as_uint(p) < cutoff_bits) p = 0.0f;
            // (p * total = p / p_max: the power of the probability relative to the largest one -- the same distribution after the
            //  renormalisation below, without p^(1/temperature) underflowing to zero for every token at a low temperature and a large vocabulary)
            else if (temperature != 1.0f) p = p > 0.0f ? powf(p * total, it) : 0.0f;
            pr.set(j, p);
            part += p;
        });
        // inclusive scan of the per-thread sums (Hillis-Steele), then the thread whose range holds u * total walks its chunk
        l_scan[tid] = part;
        __syncthreads();
        for (int o = 1; o < NT; o <<= 1) {
            const float add = tid >= o ? l_scan[tid - o] : 0.0f;
            __syncthreads();
            l_scan[tid] += add;
            __syncthreads();
        }
        const float all = l_scan[NT - 1];
        if (tid == 0) { l_ctr = counter ? *counter : 0ull; l_pick = 0x7fffffff; l_last = 0; }
        __syncthreads();
        const unsigned long long ctr = l_ctr;
        const float u = (u_in >= 0.0f ? u_in : uniform01(seed, ctr)) * all;
        const float before = tid ? l_scan[tid - 1] : 0.0f;
        if (i0 < i1 && before <= u && u < l_scan[tid]) {
            // (float prefix sums of a Hillis-Steele scan need not be monotone: more than one thread may see u in its interval -- the
            //  lowest candidate index wins)
            float acc = before;
            int found = -1, last_pos = -1;
            for_chunk(cnt, [&](int j) { const float p = pr.get(j); acc += p; if (p > 0.0f) last_pos = i0 + j; if (found < 0 && acc > u) found = i0 + j; });
            const int cand = found >= 0 ? found : last_pos;   // (acc can fall short of l_scan[tid] by rounding: the chunk's last candidate)
            if (cand >= 0) atomicMin(&l_pick, cand);
        }
        __syncthreads();
        if (l_pick == 0x7fffffff) {
            // u landed on / beyond the total through rounding: the last token with non-zero probability (0 when there is none)
            int lp = -1;
            for_chunk(cnt, [&](int j) { if (pr.get(j) > 0.0f) lp = i0 + j; });
            if (lp > 0) atomicMax(&l_last, lp);
            __syncthreads();
            pick = l_last;
        } else pick = l_pick;
        if (tid == 0 && counter) *counter = ctr + 1;
    }
    if (pick < 0 || pick >= n) pick = 0;   // (all-NaN probabilities: the token must stay a row of the embedding table)
    if (tid == 0) { *out_token = (uint32_t) pick; if (hist_word) *hist_word = (uint32_t) pick; }
    return pick;
}

// The draw of a sequence with the truncation setting `cut` (model.h, DrawRow): a row with top-k on runs the select stage on its source and
// then the body on the stash; every other row runs the body on its source, exactly as before there were settings -- {0, 0} is that draw,
// statement for statement. min-p is the body's. A row with temperature 0 is an argmax, which both truncations keep: it skips the stage
// (and never reaches the body's min-p). The setting is the row's, so the whole workgroup takes one branch.
template <class MakeSrc>
__device__ __forceinline__ int cut_sample(MakeSrc && make_src, const CutRow & cut, int n, float temperature, float top_p, float u_in,
                                          unsigned long long seed, unsigned long long * counter, float * __restrict__ probs,
                                          uint32_t * __restrict__ out_token, uint32_t * __restrict__ hist_word) {
    if (cut.top_k == 0u || cut.top_k >= (uint32_t) n || temperature == 0.0f)
        return sample_body(make_src, n, temperature, top_p, cut.min_p, u_in, seed, counter, probs, out_token, hist_word);
    const int tid = threadIdx.x, NT = blockDim.x;
    const int C = (n + NT - 1) / NT;   // (the body's chunks)
    const int i0 = tid * C, i1 = i0 + C < n ? i0 + C : n;
    select_stage(make_src(i0), i1 - i0, cut.top_k, ProbVec{probs + tid, NT});
    return sample_body([](int) { return StashedLogits{}; }, n, temperature, top_p, cut.min_p, u_in, seed, counter, probs, out_token, hist_word);
}

// The draw of one row by its workgroup, the pick returned to every thread: the source of SRC on the row's tables -- behind the guide's mask
// when GUIDED: the row reads its slot's state word s, every thread, before the body's first barrier, and draws through GuidedLogits on row s
// of the guide's table (next == NULL: no guide, and the pick of the unguided form, bit for bit) -- then cut_sample with the row's setting
// when CUT, else the body itself with no min-p; then what follows a draw: with `record` the pick is counted (thread 0, argmax or not: the
// draw of step i has seen the counts of the steps before it; rep_record for SRC_REP), and thread 0 moves the guide, after the last barrier.
// Only the fields the instantiation names are read: a form without a feature compiles to the code it was before the row had the field.
template <int SRC, bool CUT, bool GUIDED>
__device__ __forceinline__ int draw_row(const float * lg, int n, const DrawRow & row, uint32_t record, float * __restrict__ probs,
                                        uint32_t * __restrict__ out_token, uint32_t * __restrict__ hist_word) {
    static_assert(CUT || (SRC != SRC_REP && !GUIDED), "the repetition and guided forms go through cut_sample");
    const uint16_t * srow = nullptr;
    if constexpr (GUIDED) srow = row.next ? row.next + (size_t) *row.state * (size_t) n : nullptr;
    const auto inner = [&] {
        if constexpr (SRC == SRC_PLAIN) return [=](int i0) { return PlainLogits{lg + i0}; };
        else if constexpr (SRC == SRC_PEN) {
            uint32_t * count = row.count; const float * bias = row.bias; const float presence = row.presence, frequency = row.frequency;
            return [=](int i0) { return PenalisedLogits{lg + i0, count + i0, bias ? bias + i0 : nullptr, presence, frequency}; };
        } else return rep_source(lg, row.count, row.bias, row.presence, row.frequency, RepRow{row.decay, row.repetition});
    }();
    const auto make_src = [=](int i0) {
        if constexpr (GUIDED) return GuidedLogits<decltype(inner(0))>{inner(i0), srow ? srow + i0 : nullptr};
        else return inner(i0);
    };
    const rwkv_mi_sample_params & p = row.p;
    int pick;
    if constexpr (CUT) pick = cut_sample(make_src, CutRow{row.top_k, row.min_p}, n, p.temperature, p.top_p, p.u, p.seed, row.counter, probs, out_token, hist_word);
    else pick = sample_body(make_src, n, p.temperature, p.top_p, 0.0f, p.u, p.seed, row.counter, probs, out_token, hist_word);
    if constexpr (SRC == SRC_PEN) { if (threadIdx.x == 0 && record) row.count[pick] += 1u; }
    if constexpr (SRC == SRC_REP) rep_record(row.count, n, RepRow{row.decay, row.repetition}, record, pick);
    if constexpr (GUIDED) { if (threadIdx.x == 0 && srow) guide_advance(row, srow, pick); }
    return pick;
}

// The single-context entry: the row of a context is host words, so it arrives as SCALAR kernel arguments and is assembled here (a DrawRow by
// value costs the two unset forms 4 SGPRs over their pinned counts; an argument an instantiation does not read costs it nothing).
template <int SRC, bool CUT>
__global__ __launch_bounds__(1024) void k_draw(const float * __restrict__ logits, int n, float temperature, float top_p, float u_in, unsigned long long seed,
                                               unsigned long long * counter, float presence, float frequency, uint32_t record, uint32_t * count,
                                               const float * __restrict__ bias, CutRow cut, RepRow rep, float * __restrict__ probs,
                                               uint32_t * __restrict__ out_token, uint32_t * __restrict__ hist, int hist_pos) {
    const DrawRow row{{temperature, top_p, u_in, seed}, counter, presence, frequency, record, count, bias, nullptr, nullptr, nullptr, cut.top_k, cut.min_p,
                      rep.decay, rep.repetition};
    draw_row<SRC, CUT, false>(logits, n, row, record, probs, out_token, hist ? hist + hist_pos : nullptr);
}

// The row entry: grid = rows, one workgroup per row of logits[rows][n] with table[r]; row r's probabilities in its own stretch of the scratch
// (stride floats apart, the batch owns it), its token in tokens[r] and, with a history, hist[r].
// live (rwkv_mi_batch_decode_until; NULL: every row draws): a row whose LIVE WORD is 0 has retired and returns before it reads anything -- no
// draw, no counter advance, no count or sweep, no guide step, no token or history word. The whole workgroup takes the branch together: no
// barrier is left waiting.
template <int SRC, bool CUT, bool GUIDED>
__global__ __launch_bounds__(1024) void k_draw_rows(const float * __restrict__ logits, int n, const DrawRow * __restrict__ table, float * __restrict__ probs,
                                                    size_t stride, uint32_t * __restrict__ tokens, uint32_t * __restrict__ hist,
                                                    const uint32_t * __restrict__ live) {
    const size_t r = blockIdx.x;
    if (live && !live[r]) return;
    const DrawRow row = table[r];
    draw_row<SRC, CUT, GUIDED>(logits + r * (size_t) n, n, row, row.record, probs + r * stride, tokens + r, hist ? hist + r : nullptr);
}

// The greedy loops' choice for one row by the whole workgroup, returned to every thread: the largest logit, the lowest index among equals; a
// NaN never wins, and where nothing compares greater than -inf the token is 0 -- the rule of k_argmax / k_argmax_live and of the scoring kernel.
__device__ __forceinline__ int draft_argmax(const float * lg, int n) {
    __shared__ float l_v[16];
    __shared__ int l_i[16], l_res;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < n; i += blockDim.x) { const float v = lg[i]; if (v > best) { best = v; bi = i; } }
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, WAVE); const int oi = __shfl_xor(bi, o, WAVE);
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if ((threadIdx.x & 63) == 0) { l_v[threadIdx.x >> 6] = best; l_i[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int) (blockDim.x >> 6); w++) if (l_v[w] > best || (l_v[w] == best && l_i[w] < bi)) { best = l_v[w]; bi = l_i[w]; }
        l_res = bi == 0x7fffffff ? 0 : bi;
    }
    __syncthreads();
    return l_res;
}

// rwkv_mi_batch_eval_draft: which tokens of a row's draft stand. One workgroup per row r = segment segs[r] of the pass, whose tokens
// [t0, t1) are x0 d1 .. dk and whose logits (of EVERY token: logits[T][n]) are in HBM. Position j = 0 .. k chooses e_j from the logits after
// token t0 + j exactly as the plain loop of the family chooses it -- FAMILY 0: the greedy argmax; 1 + SRC: draw_row<SRC, true, false> on
// table[r], recording (a row without a truncation setting carries {0, 0}) -- and writes it to out[r][j]; the walk ends after the first j with
// j == k or e_j != d(j+1). Then keep[r] = j + 1, out[r][j + 1 .. out_stride) = RWKV_MI_NO_TOKEN and the logits of position j go to row r of
// logits_row. The draw counter and the occurrence row advance once per position walked -- a decaying row sweeps and counts each time -- so they
// end where the plain loop of keep[r] steps leaves them: nothing is rolled back. The pick comes back to every thread: the whole workgroup
// leaves the walk together. Between two positions a fence and a barrier: the next one reads the counter and the count thread 0 has just
// written, and reuses the body's LDS words.
template <int FAMILY>
__global__ __launch_bounds__(1024) void k_draft_accept_rows(const float * __restrict__ logits, int n, const SegState * __restrict__ segs,
                                                            const uint32_t * __restrict__ tokens, const DrawRow * __restrict__ table /* FAMILY 0: unread */,
                                                            float * __restrict__ probs, size_t stride, uint32_t * __restrict__ out, int out_stride,
                                                            uint32_t * __restrict__ keep, float * __restrict__ logits_row) {
    const size_t r = blockIdx.x;
    const SegState seg = segs[r];
    const int k = seg.t1 - seg.t0 - 1;
    uint32_t * o = out + r * (size_t) out_stride;
    int j = 0;
    for (;;) {
        const float * lg = logits + (size_t) (seg.t0 + j) * (size_t) n;
        int pick;
        if constexpr (FAMILY == 0) {
            pick = draft_argmax(lg, n);
            if (threadIdx.x == 0) o[j] = (uint32_t) pick;
        } else {
            const DrawRow row = table[r];
            pick = draw_row<FAMILY - 1, true, false>(lg, n, row, 1u, probs + r * stride, o + j, nullptr);
        }
        if (j == k || (uint32_t) pick != tokens[seg.t0 + j + 1]) break;
        j++;
        __threadfence_block();
        __syncthreads();
    }
    if (threadIdx.x == 0) keep[r] = (uint32_t) (j + 1);
    for (int i = j + 1 + (int) threadIdx.x; i < out_stride; i += blockDim.x) o[i] = RWKV_MI_NO_TOKEN;
    const float * src = logits + (size_t) (seg.t0 + j) * (size_t) n;
    float * dst = logits_row + r * (size_t) n;
    for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
}

// rwkv_mi_batch_guide_create: the dense table next[n_states][n_vocab] from the CSR edges, one workgroup per state: the dead fill of the
// state's row, then -- behind a barrier -- one 2-byte store per edge. A state's tokens are distinct, so no two stores meet.
__global__ __launch_bounds__(256) void k_guide_expand(uint16_t * __restrict__ next, int n_vocab, const uint32_t * __restrict__ edge_begin,
                                                      const uint32_t * __restrict__ edge_tokens, const uint32_t * __restrict__ edge_next) {
    uint16_t * row = next + (size_t) blockIdx.x * (size_t) n_vocab;
    for (int j = threadIdx.x; j < n_vocab; j += 256) row[j] = GUIDE_DEAD;
    __syncthreads();
    const uint32_t e1 = edge_begin[blockIdx.x + 1];
    for (size_t e = (size_t) edge_begin[blockIdx.x] + threadIdx.x; e < e1; e += 256)
        if (edge_tokens[e] < (uint32_t) n_vocab) row[edge_tokens[e]] = (uint16_t) edge_next[e];
}

// The stop test of rwkv_mi_batch_decode_until, one thread per row, after the draw of pass `step` of the call (hist: [step][n], the tokens this
// call has emitted). A live row retires when its emitted tokens end with one of its stop sequences (the lowest index wins) or when step + 1
// is its budget: its length and reason are written, its live word cleared, the live count taken down by one -- and BOTH row tables get the
// entry {in = F, out = G}, F the buffer pass `step` wrote for the row (`used`, the table of that pass, holds it as .out), G the other one.
// From the next pass on the row recomputes a dead step from F into G; F, the state of the row's last token, is never written again.
__global__ __launch_bounds__(64) void k_stop_rows(StopTables t, int n, const uint32_t * __restrict__ hist, uint32_t step, RowState * used, RowState * other) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= n || !t.live[r]) return;
    const StopRow sr = t.rows[r];
    const uint32_t * sl = t.seq_lens + sr.seq0;
    const uint32_t * tk = t.seq_tokens + sr.tok0;
    uint32_t reason = RWKV_MI_NO_TOKEN;
    for (uint32_t s = 0; s < sr.n_seqs && reason == RWKV_MI_NO_TOKEN; s++) {
        const uint32_t L = sl[s];
        bool match = L <= step + 1u;   // (the window is this call's tokens only)
        for (uint32_t k = 0; match && k < L; k++) match = hist[(size_t) (step + 1u - L + k) * (size_t) n + r] == tk[k];
        if (match) reason = s;
        tk += L;
    }
    if (reason == RWKV_MI_NO_TOKEN && step + 1u != sr.max_tokens) return;
    t.lens[r] = step + 1u;
    t.reasons[r] = reason;
    t.live[r] = 0u;
    const RowState u = used[r];
    const RowState dead{u.out, const_cast<float *>(u.in)};
    used[r] = dead;
    other[r] = dead;
    atomicSub(t.live_count, 1u);
}

// The scheduler of rwkv_mi_batch_serve (model.h, ServeTables), ONE workgroup, thread tid on lane base + tid, after the draw of pass `step`:
//   decode   (the lane's draw word is 1: the pass drew tokens[r]) the token is appended to the request's row out[q] and the stop test runs on
//            that row -- k_stop_rows' rule on a contiguous window: the lowest matching sequence, else the budget. A request that ends leaves
//            its length and reason and its lane FREE;
//   prompt   (the draw word is 0) the lane's token word gets the next prompt token; with the last one the draw word goes up;
//   free     the free lanes of the chunk are ranked in lane order -- a ballot per wave, the waves' counts through LDS -- and lane r takes
//            request next + rank(r) while the queue lasts: its words, its token word, its draw row (the request's, with the lane's counter,
//            set to 0, and the lane's occurrence row) and its admit word, for k_serve_reset. A lane the queue has nothing for goes dead as a
//            row of k_stop_rows does: {in = F, out = G} in both row tables, for good.
//   guides   (rwkv_mi_batch_serve_ex; t.guide_state NULL: the call has none, and none of this runs) a request whose row has a table is
//            guided: at its admission the row gets the LANE's guide words, set to the request's start state and no miss; at its retirement
//            the two words are left as the request's. An unguided request's row has no table, so it draws unmasked whatever its lane served.
// Who gets what follows from the words alone: next_request is read and written by this workgroup only, no atomic decides anything. Thread 0
// leaves the new head of the queue and the number of lanes that are not dead. DRAWS: the family has a draw table (the greedy one has none).
template <bool DRAWS>
__global__ __launch_bounds__(1024) void k_serve_rows(ServeTables t, int n, uint32_t * __restrict__ tokens, uint32_t step, RowState * used, RowState * other) {
    __shared__ uint32_t l_free[16], l_work[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = blockDim.x >> 6;
    uint32_t next = *t.next_request, work = 0u;
    for (int base = 0; base < n; base += blockDim.x) {
        const int r = base + tid;
        uint32_t q = r < n ? t.req[r] : RWKV_MI_NO_TOKEN;
        bool is_free = q == SERVE_FREE;
        if (q < SERVE_FREE) {
            const ServeReq & rq = t.reqs[q];
            if (t.draw[r]) {
                uint32_t len = t.lens[q];
                uint32_t * o = t.out + (size_t) q * t.stride;
                if (len < t.stride) o[len] = tokens[r];
                len++;
                const uint32_t * sl = t.seq_lens + rq.stop.seq0;
                const uint32_t * tk = t.seq_tokens + rq.stop.tok0;
                uint32_t reason = RWKV_MI_NO_TOKEN;
                for (uint32_t s = 0; s < rq.stop.n_seqs && reason == RWKV_MI_NO_TOKEN; s++) {
                    const uint32_t L = sl[s];
                    bool match = L <= len;   // (the window is the request's own tokens only)
                    for (uint32_t k = 0; match && k < L; k++) match = o[len - L + k] == tk[k];
                    if (match) reason = s;
                    tk += L;
                }
                t.lens[q] = len;
                if (reason != RWKV_MI_NO_TOKEN || len >= rq.stop.max_tokens) {
                    t.reasons[q] = reason; is_free = true;
                    if constexpr (DRAWS) {
                        // (a guided request leaves the lane's guide words, which its draws have moved, as its own)
                        if (t.guide_state && rq.row.next) { t.req_guide_state[q] = t.guide_state[r]; t.req_guide_misses[q] = t.guide_misses[r]; }
                    }
                }
            } else {
                const uint32_t pos = t.pos[r];
                tokens[r] = t.prompts[rq.prompt0 + pos];
                t.pos[r] = pos + 1u;
                if (pos + 1u == rq.prompt_len) t.draw[r] = 1u;
            }
        }
        const unsigned long long m = __ballot(is_free);
        uint32_t rank = (uint32_t) __popcll(m & ((1ull << lane) - 1ull));
        __syncthreads();   // (the chunk before has read the words)
        if (lane == 0) l_free[wave] = (uint32_t) __popcll(m);
        __syncthreads();
        uint32_t total = 0u;
        for (int w = 0; w < waves; w++) { if (w < wave) rank += l_free[w]; total += l_free[w]; }
        bool alive = q < SERVE_FREE && !is_free;
        if (r < n) t.admit[r] = 0u;
        if (is_free) {
            const uint32_t qn = next + rank;
            if (qn < t.n_requests) {
                const ServeReq & rq = t.reqs[qn];
                const uint32_t slot = t.lane_slot[r];
                t.req[r] = qn; t.last[r] = qn; t.pos[r] = 1u;
                tokens[r] = t.prompts[rq.prompt0];
                t.draw[r] = rq.prompt_len == 1u ? 1u : 0u;
                t.lane[qn] = (uint32_t) r; t.start_pass[qn] = step + 1u;
                t.counters[slot] = 0ull;
                if constexpr (DRAWS) {
                    DrawRow * row = t.rows + r;   // (the request's row, then the two words that are the lane's)
                    *row = rq.row;
                    row->counter = t.counters + slot;
                    if (rq.row.record) row->count = t.counts + (size_t) slot * t.n_vocab;
                    // (a guided request: the lane's guide words, from the request's start state and no miss; any other has no table and
                    //  no words, whatever the lane served before)
                    if (t.guide_state && rq.row.next) {
                        row->state = t.guide_state + r; row->misses = t.guide_misses + r;
                        t.guide_state[r] = t.req_guide_state[qn]; t.guide_misses[r] = 0u;
                    }
                }
                t.admit[r] = 1u;
                alive = true;
            } else {
                t.req[r] = RWKV_MI_NO_TOKEN; t.draw[r] = 0u;
                const RowState u = used[r];
                const RowState dead{u.out, const_cast<float *>(u.in)};
                used[r] = dead;
                other[r] = dead;
            }
        }
        next = next + total < t.n_requests ? next + total : t.n_requests;
        work += (uint32_t) __popcll(__ballot(alive));
    }
    if (lane == 0) l_work[wave] = work;
    __syncthreads();
    if (tid == 0) {
        uint32_t w_all = 0u;
        for (int w = 0; w < waves; w++) w_all += l_work[w];
        *t.next_request = next;
        *t.work = w_all;
    }
}

// The scheduler of a serve session (model.h, SessionTables): k_serve_rows with the queue a ring that the host keeps filling, ONE workgroup,
// thread tid on lane base + tid, after the draw of pass `step`. What differs:
//   the ring   the lane's word t.req[r] is the ENTRY of its request, id % capacity, and every per-request word is indexed by it; ids are
//              handed out from next_request while they are below `tail`, the kernel argument that says how far the host has uploaded;
//   idle       a lane the queue has nothing for is IDLE, not dead: its two row-table entries become {in = F, out = G} ONCE, when its request
//              retires with nothing to take, and it stays a candidate of every later step. An admission to an idle lane restores the
//              mirror (other[r] = {G, F}); k_serve_reset then copies the start state into used[r].out = G, which the next pass reads;
//   cancel     a request whose cancel word is set retires with RWKV_MI_STOP_CANCELLED at the step after any of its passes, unless that
//              pass drew a token that ends it by itself (the token is appended and the natural end tested first); in its prompt phase it
//              retires with length 0;
//   admit_only the launch in front of a block's first pass: lanes that have a request are not looked at, idle ones take what has arrived.
// A retirement leaves done = 1 and the pass; an admission the id, done = 0, length 0, lane, start pass and whether the lane was idle. Thread 0
// leaves the new head of the queue and the number of lanes that have a request, with ordinary stores.
template <bool DRAWS>
__global__ __launch_bounds__(1024) void k_session_rows(SessionTables s, int n, uint32_t * __restrict__ tokens, uint32_t step, RowState * used, RowState * other) {
    __shared__ uint32_t l_free[16], l_work[16];
    const ServeTables & t = s.t;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = blockDim.x >> 6;
    uint32_t next = *t.next_request, work = 0u;
    for (int base = 0; base < n; base += blockDim.x) {
        const int r = base + tid;
        const bool in = r < n;
        const uint32_t e = in ? t.req[r] : SESSION_IDLE;
        const bool had = e != SESSION_IDLE;
        bool retired = false;
        if (had && !s.admit_only) {
            const ServeReq & rq = t.reqs[e];
            const bool cancelled = s.cancel[e] != 0u;
            bool ended = false;
            if (t.draw[r]) {
                uint32_t len = t.lens[e];
                uint32_t * o = t.out + (size_t) e * t.stride;
                if (len < t.stride) o[len] = tokens[r];
                len++;
                const uint32_t * sl = t.seq_lens + rq.stop.seq0;
                const uint32_t * tk = t.seq_tokens + rq.stop.tok0;
                uint32_t reason = RWKV_MI_NO_TOKEN;
                for (uint32_t q = 0; q < rq.stop.n_seqs && reason == RWKV_MI_NO_TOKEN; q++) {
                    const uint32_t L = sl[q];
                    bool match = L <= len;   // (the window is the request's own tokens only)
                    for (uint32_t k = 0; match && k < L; k++) match = o[len - L + k] == tk[k];
                    if (match) reason = q;
                    tk += L;
                }
                t.lens[e] = len;
                if (reason != RWKV_MI_NO_TOKEN || len >= rq.stop.max_tokens) { t.reasons[e] = reason; ended = true; }
            } else if (!cancelled) {
                const uint32_t pos = t.pos[r];
                tokens[r] = t.prompts[rq.prompt0 + pos];
                t.pos[r] = pos + 1u;
                if (pos + 1u == rq.prompt_len) t.draw[r] = 1u;
            }
            if (!ended && cancelled) { t.reasons[e] = RWKV_MI_STOP_CANCELLED; ended = true; }
            if (ended) {
                if constexpr (DRAWS) {
                    if (t.guide_state && rq.row.next) { t.req_guide_state[e] = t.guide_state[r]; t.req_guide_misses[e] = t.guide_misses[r]; }
                }
                s.end_pass[e] = step; s.done[e] = 1u;
                retired = true;
            }
        }
        const bool is_free = in && (!had || retired);
        const unsigned long long m = __ballot(is_free);
        uint32_t rank = (uint32_t) __popcll(m & ((1ull << lane) - 1ull));
        __syncthreads();   // (the chunk before has read the words)
        if (lane == 0) l_free[wave] = (uint32_t) __popcll(m);
        __syncthreads();
        uint32_t total = 0u;
        for (int w = 0; w < waves; w++) { if (w < wave) rank += l_free[w]; total += l_free[w]; }
        bool alive = had && !retired;
        if (in) t.admit[r] = 0u;
        if (is_free) {
            const uint32_t qn = next + rank;
            if (qn < s.tail) {
                const uint32_t en = qn % s.capacity;
                const ServeReq & rq = t.reqs[en];
                const uint32_t slot = t.lane_slot[r];
                t.req[r] = en; t.last[r] = qn; t.pos[r] = 1u;
                tokens[r] = t.prompts[rq.prompt0];
                t.draw[r] = rq.prompt_len == 1u ? 1u : 0u;
                t.lane[en] = (uint32_t) r; t.start_pass[en] = step + 1u;
                t.lens[en] = 0u; t.reasons[en] = RWKV_MI_NO_TOKEN;
                s.ids[en] = qn; s.done[en] = 0u; s.revived[en] = had ? 0u : 1u;
                t.counters[slot] = 0ull;
                if constexpr (DRAWS) {
                    DrawRow * row = t.rows + r;   // (the request's row, then the words that are the lane's: k_serve_rows' admission)
                    *row = rq.row;
                    row->counter = t.counters + slot;
                    if (rq.row.record) row->count = t.counts + (size_t) slot * t.n_vocab;
                    if (t.guide_state) {   // (the entry's words back are an unguided request's 0 and 0 until a guided one retires)
                        t.req_guide_state[en] = 0u; t.req_guide_misses[en] = 0u;
                        if (rq.row.next) {
                            row->state = t.guide_state + r; row->misses = t.guide_misses + r;
                            t.guide_state[r] = t.prompts[(size_t) en * s.entry_words + s.guide_word]; t.guide_misses[r] = 0u;
                        }
                    }
                }
                if (!had) {   // (idle: both entries are {F, G}; the pass that follows runs on `other` and has to read G)
                    const RowState u = used[r];
                    other[r] = RowState{u.out, const_cast<float *>(u.in)};
                }
                t.admit[r] = 1u;
                alive = true;
            } else if (had) {
                t.req[r] = SESSION_IDLE; t.draw[r] = 0u;
                const RowState u = used[r];
                const RowState idle{u.out, const_cast<float *>(u.in)};
                used[r] = idle;
                other[r] = idle;
            }
        }
        next = next + total < s.tail ? next + total : s.tail;
        work += (uint32_t) __popcll(__ballot(alive));
    }
    if (lane == 0) l_work[wave] = work;
    __syncthreads();
    if (tid == 0) {
        uint32_t w_all = 0u;
        for (int w = 0; w < waves; w++) w_all += l_work[w];
        *t.next_request = next;
        *t.work = w_all;
    }
}

// The admissions of the pass, grid = lanes x chunks: a workgroup whose lane's admit word is 0 returns at once, all of it together. The others
// stream the request's start state -- a from_slot's current buffer or the batch's fresh state: one path -- into used[r].out, the buffer the
// lane's next pass reads (a live lane's two row tables mirror each other) and zero the lane's occurrence row. VEC: 16 bytes per load and
// store -- the launcher has checked that the state length and the vocabulary are multiples of four words, so every buffer and row is aligned;
// the other form moves words.
template <bool VEC>
__global__ __launch_bounds__(256) void k_serve_reset(ServeTables t, const RowState * __restrict__ used, int64_t state_len) {
    const int r = blockIdx.x;
    if (!t.admit[r]) return;
    const float * __restrict__ src = t.reqs[t.req[r]].start;
    float * __restrict__ dst = used[r].out;
    const int64_t i0 = (int64_t) blockIdx.y * 256 + threadIdx.x, hop = (int64_t) gridDim.y * 256;
    if constexpr (VEC) {
        const float4 * __restrict__ s4 = (const float4 *) src;
        float4 * __restrict__ d4 = (float4 *) dst;
#pragma unroll 4
        for (int64_t i = i0; i < state_len / 4; i += hop) d4[i] = s4[i];
    } else {
        for (int64_t i = i0; i < state_len; i += hop) dst[i] = src[i];
    }
    if (!t.counts) return;
    uint32_t * c = t.counts + (size_t) t.lane_slot[r] * t.n_vocab;
    if constexpr (VEC) {
        uint4 * c4 = (uint4 *) c;
        for (int64_t i = i0; i < (int64_t) (t.n_vocab / 4); i += hop) c4[i] = make_uint4(0u, 0u, 0u, 0u);
    } else {
        for (int64_t i = i0; i < (int64_t) t.n_vocab; i += hop) c[i] = 0u;
    }
}

// count[tokens[i]] += 1 for a list of tokens (rwkv_mi_*counts_add: a token may come more than once)
__global__ __launch_bounds__(256) void k_count_add(uint32_t * __restrict__ count, const uint32_t * __restrict__ tokens, int64_t n, int n_vocab) {
    const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (i < n && tokens[i] < (uint32_t) n_vocab) atomicAdd(count + tokens[i], 1u);
}

// The same on the table of a decaying sequence: for every token of the list, in its order, every entry is multiplied by decay and the token's
// entry goes up by 1.0f -- what the draws that recorded these tokens would have left. One thread owns entry j from the first token to the last
// (the list is read by every thread at the same index), so the n products are rounded one after the other as the plain loop rounds them; the
// closed form decay^n is not bit-equal to that.
__global__ __launch_bounds__(256) void k_count_add_decay(float * __restrict__ occ, const uint32_t * __restrict__ tokens, int64_t n, int n_vocab, float decay) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_vocab) return;
    float o = occ[j];
    for (int64_t i = 0; i < n; i++) {
        o = o * decay;
        if (tokens[i] == (uint32_t) j) o = o + 1.0f;
    }
    occ[j] = o;
}

// bias[ids[i]] = values[i] (rwkv_mi_*logit_bias_set, into a table the caller has cleared; the ids are distinct)
__global__ __launch_bounds__(256) void k_bias_scatter(float * __restrict__ bias, const uint32_t * __restrict__ ids, const float * __restrict__ values, int64_t n, int n_vocab) {
    const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (i < n && ids[i] < (uint32_t) n_vocab) bias[ids[i]] = values[i];
}

__global__ __launch_bounds__(64) void k_sample_seek_rows(const DrawRow * __restrict__ table, int rows, unsigned long long value) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r < rows) *table[r].counter = value;
}

// From a call's form to the instantiation it launches: the one switch of each launcher is over this number. Exactly the forms listed are
// compiled (tests/test_cpu_draw_forms.py holds the file to the list); DrawForm::of makes no other, and one that arrives anyway is a bug of the
// caller's that ends the process rather than draw with another kernel.
constexpr int form_id(int src, bool cut, bool guided) { return src * 4 + (cut ? 2 : 0) + (guided ? 1 : 0); }
static int form_id(const DrawForm & f) { return form_id(f.rep ? SRC_REP : f.draw == Draw::penalized ? SRC_PEN : SRC_PLAIN, f.cut, f.guided); }
[[noreturn]] static void no_such_form(const DrawForm & f) {
    fprintf(stderr, "sampling.hip: no draw kernel of the form {draw %d, cut %d, guided %d, rep %d}\n", (int) f.draw, (int) f.cut, (int) f.guided, (int) f.rep);
    abort();
}

void launch_draw(const float * logits, int n, const DrawRow & row, const DrawForm & form, float * probs, uint32_t * out_token, uint32_t * hist, int hist_pos,
                 hipStream_t st) {
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(1), dim3(1024), 0, st, logits, n, row.p.temperature, row.p.top_p, row.p.u, (unsigned long long) row.p.seed, row.counter, row.presence,
                           row.frequency, row.record, row.count, row.bias, CutRow{row.top_k, row.min_p}, RepRow{row.decay, row.repetition}, probs, out_token, hist, hist_pos);
    };
    switch (form_id(form)) {
        case form_id(SRC_PLAIN, false, false): go(k_draw<SRC_PLAIN, false>); break;
        case form_id(SRC_PLAIN, true, false):  go(k_draw<SRC_PLAIN, true>); break;
        case form_id(SRC_PEN, false, false):   go(k_draw<SRC_PEN, false>); break;
        case form_id(SRC_PEN, true, false):    go(k_draw<SRC_PEN, true>); break;
        case form_id(SRC_REP, true, false):    go(k_draw<SRC_REP, true>); break;
        default: no_such_form(form);
    }
}

void launch_draw_rows(const float * logits, int64_t rows, int n, const DrawRow * table, const DrawForm & form, float * probs, uint32_t * tokens, uint32_t * hist,
                      const uint32_t * live, hipStream_t st) {
    auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3((unsigned) rows), dim3(1024), 0, st, logits, n, table, probs, sample_scratch_floats(n), tokens, hist, live); };
    switch (form_id(form)) {
        case form_id(SRC_PLAIN, false, false): go(k_draw_rows<SRC_PLAIN, false, false>); break;
        case form_id(SRC_PLAIN, true, false):  go(k_draw_rows<SRC_PLAIN, true, false>); break;
        case form_id(SRC_PLAIN, true, true):   go(k_draw_rows<SRC_PLAIN, true, true>); break;
        case form_id(SRC_PEN, false, false):   go(k_draw_rows<SRC_PEN, false, false>); break;
        case form_id(SRC_PEN, true, false):    go(k_draw_rows<SRC_PEN, true, false>); break;
        case form_id(SRC_PEN, true, true):     go(k_draw_rows<SRC_PEN, true, true>); break;
        case form_id(SRC_REP, true, false):    go(k_draw_rows<SRC_REP, true, false>); break;
        case form_id(SRC_REP, true, true):     go(k_draw_rows<SRC_REP, true, true>); break;
        default: no_such_form(form);
    }
}

// (the walk reads every row's truncation setting whatever form.cut says, and takes no guide: rwkv_mi_batch_eval_draft rejects a guided slot)
void launch_draft_accept_rows(const float * logits, int64_t rows, int n, const SegState * segs, const uint32_t * tokens, const DrawRow * table, const DrawForm & form,
                              float * probs, uint32_t * out, int out_stride, uint32_t * keep, float * logits_row, hipStream_t st) {
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3((unsigned) rows), dim3(1024), 0, st, logits, n, segs, tokens, table, probs, sample_scratch_floats(n), out, out_stride, keep, logits_row);
    };
    if (form.guided) no_such_form(form);
    if (form.draw == Draw::none) go(k_draft_accept_rows<0>);
    else switch (form_id(form) / 4) {
        case SRC_PLAIN: go(k_draft_accept_rows<1 + SRC_PLAIN>); break;
        case SRC_PEN:   go(k_draft_accept_rows<1 + SRC_PEN>); break;
        case SRC_REP:   go(k_draft_accept_rows<1 + SRC_REP>); break;
    }
}

void launch_guide_expand(uint16_t * next, uint32_t n_states, int n_vocab, const uint32_t * edge_begin, const uint32_t * edge_tokens, const uint32_t * edge_next,
                         hipStream_t st) {
    hipLaunchKernelGGL(k_guide_expand, dim3(n_states), dim3(256), 0, st, next, n_vocab, edge_begin, edge_tokens, edge_next);
}

void launch_stop_rows(const StopTables & t, int64_t rows, const uint32_t * hist, uint32_t step, RowState * used, RowState * other, hipStream_t st) {
    hipLaunchKernelGGL(k_stop_rows, dim3((unsigned) ((rows + 63) / 64)), dim3(64), 0, st, t, (int) rows, hist, step, used, other);
}

void launch_serve_rows(const ServeTables & t, int64_t n, uint32_t * tokens, uint32_t step, RowState * used, RowState * other, hipStream_t st) {
    const unsigned threads = n >= 1024 ? 1024u : (unsigned) ((n + 63) / 64) * 64u;
    if (t.rows) hipLaunchKernelGGL(k_serve_rows<true>, dim3(1), dim3(threads), 0, st, t, (int) n, tokens, step, used, other);
    else hipLaunchKernelGGL(k_serve_rows<false>, dim3(1), dim3(threads), 0, st, t, (int) n, tokens, step, used, other);
}

void launch_session_rows(const SessionTables & s, int64_t n, uint32_t * tokens, uint32_t step, RowState * used, RowState * other, hipStream_t st) {
    const unsigned threads = n >= 1024 ? 1024u : (unsigned) ((n + 63) / 64) * 64u;
    if (s.t.rows) hipLaunchKernelGGL(k_session_rows<true>, dim3(1), dim3(threads), 0, st, s, (int) n, tokens, step, used, other);
    else hipLaunchKernelGGL(k_session_rows<false>, dim3(1), dim3(threads), 0, st, s, (int) n, tokens, step, used, other);
}

void launch_serve_reset(const ServeTables & t, int64_t n, unsigned chunks, const RowState * used, int64_t state_len, hipStream_t st) {
    // (hipMalloc aligns the buffers themselves: a slot's state and its occurrence row are 16-byte aligned when their lengths are whole float4s)
    const bool vec = (state_len & 3) == 0 && (!t.counts || (t.n_vocab & 3u) == 0);
    if (vec) hipLaunchKernelGGL(k_serve_reset<true>, dim3((unsigned) n, chunks), dim3(256), 0, st, t, used, state_len);
    else hipLaunchKernelGGL(k_serve_reset<false>, dim3((unsigned) n, chunks), dim3(256), 0, st, t, used, state_len);
}

void launch_count_add(uint32_t * count, const uint32_t * tokens, int64_t n, int n_vocab, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_count_add, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, st, count, tokens, n, n_vocab);
}

void launch_count_add_decay(float * occ, const uint32_t * tokens, int64_t n, int n_vocab, float decay, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_count_add_decay, dim3((unsigned) ((n_vocab + 255) / 256)), dim3(256), 0, st, occ, tokens, n, n_vocab, decay);
}

void launch_bias_scatter(float * bias, const uint32_t * ids, const float * values, int64_t n, int n_vocab, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_bias_scatter, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, st, bias, ids, values, n, n_vocab);
}

void launch_sample_seek_rows(const DrawRow * table, int64_t rows, unsigned long long value, hipStream_t st) {
    hipLaunchKernelGGL(k_sample_seek_rows, dim3((unsigned) ((rows + 63) / 64)), dim3(64), 0, st, table, (int) rows, value);
}

}  // namespace rwkvmi
