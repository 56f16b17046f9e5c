// draw_state.cpp -- what a sequence carries from one draw to the next, for a context's one sequence and a batch's slots (model.h,
// DrawState), the argument rules of the calls that change it, and a guide's edges and table
#include "model.h"
#include "rwkv_mi355x.h"

#include <cinttypes>
#include <cmath>
#include <cstring>

using namespace rwkvmi;

// ---- penalised sampling (rwkv_mi_*_penalized, rwkv_mi_*counts_*, rwkv_mi_*logit_bias_set): what contexts and batches share ----

// the arguments of counts_add / logit_bias_set / a penalty (checked before anything changes; errors are reported on ctx)
bool rwkvmi::check_count_tokens(rwkv_context * ctx, const uint32_t * tokens, size_t n) {
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, tokens != nullptr || n == 0, "tokens is NULL");
    const size_t n_vocab = (size_t) ctx->model->n_vocab();
    for (size_t i = 0; i < n; i++)
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, tokens[i] < n_vocab, "Token at index %zu (%" PRIu32 ") is out of range (0 .. %zu)", i, tokens[i], n_vocab - 1);
    return true;
}

bool rwkvmi::check_bias(rwkv_context * ctx, const uint32_t * ids, const float * values, size_t n) {
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, n == 0 || (ids != nullptr && values != nullptr), "ids or values is NULL");
    const size_t n_vocab = (size_t) ctx->model->n_vocab();
    std::vector<uint8_t> seen(n ? n_vocab : 0, 0);
    for (size_t i = 0; i < n; i++) {
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, ids[i] < n_vocab, "bias id at index %zu (%" PRIu32 ") is out of range (0 .. %zu)", i, ids[i], n_vocab - 1);
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, !seen[ids[i]], "bias id %" PRIu32 " appears twice", ids[i]);
        seen[ids[i]] = 1;
        // (NaN fails the comparison; -inf and large negatives forbid a token and are allowed)
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, values[i] < INFINITY, "bias value at index %zu (%g) is NaN or +inf", i, (double) values[i]);
    }
    return true;
}

bool rwkvmi::check_penalty(rwkv_context * ctx, float presence, float frequency, size_t index) {
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, std::isfinite(presence) && std::isfinite(frequency),
                 "the penalty at index %zu is not finite (presence %g, frequency %g)", index, (double) presence, (double) frequency);
    return true;
}

// ---- the draw state of a context's sequence or of a batch's slots (model.h, DrawState) ----

bool DrawState::ensure_counters(rwkv_context * ctx, hipStream_t st) {
    if (counters) return true;
    DevBuf<unsigned long long> fresh;
    const hipError_t e = grow(want(fresh, slots));
    RW_CTX_CHECK(ctx, RWKV_ERROR_ALLOC, false, e == hipSuccess, "cannot allocate the draw counters of %zu slots: %s", slots, hipGetErrorString(e));
    HIP_CTX_OK(ctx, hipMemsetAsync(fresh.p, 0, slots * sizeof(unsigned long long), st));
    counters = std::move(fresh);
    return true;
}

bool DrawState::ensure_sampler(rwkv_context * ctx, hipStream_t st) {
    if (!ensure_counters(ctx, st)) return false;
    if (probs) return true;
    const hipError_t e = grow(want(probs, slots * sample_scratch_floats((int64_t) n_vocab)));
    RW_CTX_CHECK(ctx, RWKV_ERROR_ALLOC, false, e == hipSuccess, "cannot allocate the sampler's scratch for %zu slots: %s", slots, hipGetErrorString(e));
    return true;
}

bool DrawState::ensure_penalty(rwkv_context * ctx, hipStream_t st) {
    if (counts && bias) return true;
    const size_t words = slots * n_vocab;   // (both tables are 32-bit words)
    DevBuf<uint32_t> c;
    DevBuf<float> b;
    const hipError_t e = grow(want(c, words), want(b, words));
    RW_CTX_CHECK(ctx, RWKV_ERROR_ALLOC, false, e == hipSuccess, "cannot allocate the penalty tables of %zu slots: %s", slots, hipGetErrorString(e));
    // (a table that could not be zeroed is not kept)
    HIP_CTX_OK(ctx, hipMemsetAsync(c.p, 0, words * 4, st));
    HIP_CTX_OK(ctx, hipMemsetAsync(b.p, 0, words * 4, st));
    HIP_CTX_OK(ctx, hipStreamSynchronize(st));
    counts = std::move(c);
    bias = std::move(b);
    return true;
}

bool DrawState::seek(rwkv_context * ctx, size_t slot, unsigned long long value, hipStream_t st) {
    if (!ensure_counters(ctx, st)) return false;
    HIP_CTX_OK(ctx, hipMemcpyAsync(counter(slot), &value, sizeof(value), hipMemcpyHostToDevice, st));
    HIP_CTX_OK(ctx, hipStreamSynchronize(st));
    return true;
}

bool DrawState::counts_reset(rwkv_context * ctx, size_t slot, hipStream_t st) {
    if (!ensure_penalty(ctx, st)) return false;
    HIP_CTX_OK(ctx, hipMemsetAsync(counts_of(slot), 0, n_vocab * sizeof(uint32_t), st));
    HIP_CTX_OK(ctx, hipStreamSynchronize(st));
    return true;
}

// count[tokens[i]] += 1 on the device
bool DrawState::counts_add(rwkv_context * ctx, size_t slot, const uint32_t * tokens, size_t n, hipStream_t st) {
    if (!ensure_penalty(ctx, st)) return false;
    if (n == 0) return true;
    DevBuf<uint32_t> d;
    bool ok = d.upload(tokens, n, st);
    // (a decaying slot's row holds floats: every token of the list decays the row and counts, in the list's order)
    if (ok && decaying(slot)) launch_count_add_decay((float *) counts_of(slot), d.p, (int64_t) n, (int) n_vocab, reps[slot].decay, st);
    else if (ok) launch_count_add(counts_of(slot), d.p, (int64_t) n, (int) n_vocab, st);
    ok = ok && hipGetLastError() == hipSuccess;
    ok = hipStreamSynchronize(st) == hipSuccess && ok;
    RW_CTX_CHECK(ctx, RWKV_ERROR_GRAPH, false, ok, "HIP error: %s", hipGetErrorString(hipGetLastError()));
    return true;
}

bool DrawState::counts_store(rwkv_context * ctx, size_t slot, uint32_t * counts_out, hipStream_t st) {
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, !decaying(slot), "the slot is decaying: its occurrence row holds floats (counts_store_f32 reads it)");
    if (!ensure_penalty(ctx, st)) return false;
    HIP_CTX_OK(ctx, hipMemcpyAsync(counts_out, counts_of(slot), n_vocab * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_CTX_OK(ctx, hipStreamSynchronize(st));
    return true;
}

// the row as floats: a decaying slot's words as they are, the counts of any other converted (exact below 2^24)
bool DrawState::counts_store_f32(rwkv_context * ctx, size_t slot, float * out, hipStream_t st) {
    if (!ensure_penalty(ctx, st)) return false;
    HIP_CTX_OK(ctx, hipMemcpyAsync(out, counts_of(slot), n_vocab * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_CTX_OK(ctx, hipStreamSynchronize(st));
    if (!decaying(slot))
        for (size_t j = 0; j < n_vocab; j++) { uint32_t c; memcpy(&c, out + j, sizeof(c)); out[j] = (float) c; }
    return true;
}

// bias = 0, then bias[ids[i]] = values[i] on the device
bool DrawState::bias_set(rwkv_context * ctx, size_t slot, const uint32_t * ids, const float * values, size_t n, hipStream_t st) {
    if (!ensure_penalty(ctx, st)) return false;
    if (n == 0) { HIP_CTX_OK(ctx, hipStreamSynchronize(st)); has_bias[slot] = 0; return true; }
    has_bias[slot] = 1;   // (a failure below leaves a table that is cleared or half written: it is not read as "no bias")
    float * table = bias.p + slot * n_vocab;
    DevBuf<uint32_t> di;
    DevBuf<float> dv;
    bool ok = di.upload(ids, n, st) && dv.upload(values, n, st) && hipMemsetAsync(table, 0, n_vocab * sizeof(float), st) == hipSuccess;
    if (ok) launch_bias_scatter(table, di.p, dv.p, (int64_t) n, (int) n_vocab, st);
    ok = ok && hipGetLastError() == hipSuccess;
    ok = hipStreamSynchronize(st) == hipSuccess && ok;
    RW_CTX_CHECK(ctx, RWKV_ERROR_GRAPH, false, ok, "HIP error: %s", hipGetErrorString(hipGetLastError()));
    return true;
}

bool DrawState::ensure_guides(rwkv_context * ctx, hipStream_t st) {
    if (guide_state && guide_misses) return true;
    DevBuf<uint32_t> s, m;
    const hipError_t e = grow(want(s, slots), want(m, slots));
    RW_CTX_CHECK(ctx, RWKV_ERROR_ALLOC, false, e == hipSuccess, "cannot allocate the guide words of %zu slots: %s", slots, hipGetErrorString(e));
    // (words that could not be zeroed are not kept)
    HIP_CTX_OK(ctx, hipMemsetAsync(s.p, 0, slots * sizeof(uint32_t), st));
    HIP_CTX_OK(ctx, hipMemsetAsync(m.p, 0, slots * sizeof(uint32_t), st));
    HIP_CTX_OK(ctx, hipStreamSynchronize(st));
    guide_state = std::move(s);
    guide_misses = std::move(m);
    return true;
}

bool DrawState::guide_attach(rwkv_context * ctx, size_t slot, uint32_t guide, uint32_t state, hipStream_t st) {
    const bool detach = guide == RWKV_MI_NO_GUIDE;
    if (detach && !guide_state) { HIP_CTX_OK(ctx, hipStreamSynchronize(st)); guide_of[slot] = guide; return true; }   // (never attached: no words exist)
    if (!ensure_guides(ctx, st)) return false;
    const uint32_t words[2] = {detach ? 0u : state, 0u};
    HIP_CTX_OK(ctx, hipMemcpyAsync(guide_state.p + slot, &words[0], sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_CTX_OK(ctx, hipMemcpyAsync(guide_misses.p + slot, &words[1], sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_CTX_OK(ctx, hipStreamSynchronize(st));
    guide_of[slot] = guide;
    return true;
}

bool DrawState::guide_words(rwkv_context * ctx, size_t slot, uint32_t * state_out, uint32_t * misses_out, hipStream_t st) {
    uint32_t words[2] = {0u, 0u};
    if (guide_of[slot] != RWKV_MI_NO_GUIDE) {
        HIP_CTX_OK(ctx, hipMemcpyAsync(&words[0], guide_state.p + slot, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_CTX_OK(ctx, hipMemcpyAsync(&words[1], guide_misses.p + slot, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_CTX_OK(ctx, hipStreamSynchronize(st));
    }
    if (state_out) *state_out = words[0];
    if (misses_out) *misses_out = words[1];
    return true;
}

// the truncation setting of a slot: host words, read by every draw of the slot from the next call on
bool DrawState::cut_set(rwkv_context * ctx, size_t slot, uint32_t top_k, float min_p) {
    // (written so that a NaN fails the comparison)
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, min_p >= 0.0f && min_p <= 1.0f, "min_p (%g) must be in 0 .. 1", (double) min_p);
    cuts[slot] = CutRow{top_k, min_p};
    return true;
}

// the repetition setting of a slot: host words, read by every penalised draw of the slot from the next call on. The words of the slot's
// occurrence row are floats exactly while decay != 1: a set that changes that zeroes the row (a table not yet allocated is zero already)
bool DrawState::rep_set(rwkv_context * ctx, size_t slot, float decay, float repetition, hipStream_t st) {
    // (written so that a NaN fails the comparison)
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, decay >= 0.0f && decay <= 1.0f, "decay (%g) must be in 0 .. 1", (double) decay);
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, repetition > 0.0f && repetition < INFINITY, "repetition (%g) must be finite and above 0", (double) repetition);
    if ((decay != 1.0f) != decaying(slot) && counts) {
        HIP_CTX_OK(ctx, hipMemsetAsync(counts_of(slot), 0, n_vocab * sizeof(uint32_t), st));
        HIP_CTX_OK(ctx, hipStreamSynchronize(st));
    }
    reps[slot] = RepRow{decay, repetition};
    return true;
}

// ---- a guide's edges and its table on the device (rwkv_mi_batch_guide_create; model.h) ----
namespace rwkvmi {

const char * guide_edges_fault(size_t n_vocab, uint32_t n_states, const uint32_t * edge_begin, const uint32_t * edge_tokens, const uint32_t * edge_next) {
    if (!edge_begin || !edge_tokens || !edge_next) return "edge_begin, edge_tokens or edge_next is NULL";
    if (n_states == 0 || n_states > RWKV_MI_GUIDE_MAX_STATES) return "n_states is 0 or above RWKV_MI_GUIDE_MAX_STATES";
    if (edge_begin[0] != 0) return "edge_begin does not start at 0";
    for (uint32_t s = 0; s < n_states; s++) {
        if (edge_begin[s + 1] < edge_begin[s]) return "edge_begin decreases";
        if (edge_begin[s + 1] == edge_begin[s]) return "a state has no edge";
    }
    for (uint32_t s = 0; s < n_states; s++)
        for (size_t e = edge_begin[s]; e < edge_begin[s + 1]; e++) {
            if (edge_tokens[e] >= n_vocab) return "an edge's token is out of range";
            if (e > edge_begin[s] && edge_tokens[e] <= edge_tokens[e - 1]) return "a state's tokens are not strictly ascending";
            if (edge_next[e] >= n_states) return "an edge's next state is out of range";
        }
    return nullptr;
}

hipError_t guide_table_build(DevBuf<uint16_t> & table, size_t n_vocab, uint32_t n_states, const uint32_t * edge_begin, const uint32_t * edge_tokens,
                             const uint32_t * edge_next, hipStream_t st, bool * alloc_failed) {
    const size_t n_edges = edge_begin[n_states];
    DevBuf<uint16_t> fresh;
    DevBuf<uint32_t> d_begin, d_tokens, d_next;
    *alloc_failed = true;
    hipError_t e = grow(want(fresh, (size_t) n_states * n_vocab), want(d_begin, (size_t) n_states + 1), want(d_tokens, n_edges), want(d_next, n_edges));
    if (e != hipSuccess) return e;
    *alloc_failed = false;
    e = hipMemcpyAsync(d_begin.p, edge_begin, ((size_t) n_states + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_tokens.p, edge_tokens, n_edges * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_next.p, edge_next, n_edges * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) { launch_guide_expand(fresh.p, n_states, (int) n_vocab, d_begin.p, d_tokens.p, d_next.p, st); e = hipGetLastError(); }
    const hipError_t es = hipStreamSynchronize(st);   // (the edges are read until here, also after a failure)
    if (e == hipSuccess) e = es;
    if (e == hipSuccess) table = std::move(fresh);
    return e;
}

}  // namespace rwkvmi
