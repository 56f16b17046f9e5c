// batch.cpp -- the batch engine behind the rwkv_mi_batch_* calls (include/rwkv_mi355x.h): the batch and its staged tables, the checks and
// uploads of a call, the pass, the draft pass, the loop driver with its four loops, and the entry points. Nothing outside this file names a
// member of rwkv_mi_batch.
#include "model.h"
#include "rwkv_mi355x.h"
#include "call_layout.h"
#include "session_book.h"

#include <cinttypes>
#include <cmath>
#include <cstring>

using namespace rwkvmi;

// ---------------------------------------------------------------------------------------------------------------
// Batched decode (rwkv_mi_batch_*): n sequences per pass over the weights. The slots' states are [2][n_slots][state_len] in HBM with a
// parity per slot; a pass reads slot s at buffer parity[s] and writes buffer parity[s] ^ 1 through a row table ({in, out} per row,
// uploaded through pinned staging). The pass itself is the per-op Runner in row mode on the batch's own context (engine.hip forward_rows).
// ---------------------------------------------------------------------------------------------------------------

// What the host of a polled device loop reads between two blocks of passes (batch_run_passes): the polled word of the last two blocks in
// pinned memory, each behind its event. Created by the first polled loop of a batch, whichever it is; destroyed with the batch, whose free
// function has drained the stream and made the device current.
struct BlockPoll {
    PinBuf<uint32_t> count;   // [2]
    hipEvent_t ev[2] = {nullptr, nullptr};   // (not copyable: `count` is not)
    ~BlockPoll() { for (hipEvent_t e : ev) if (e) (void) hipEventDestroy(e); }
    // a failure leaves what exists as it was and clears the sticky HIP error
    hipError_t ensure() {
        hipError_t e = count ? hipSuccess : count.alloc(2);
        for (hipEvent_t & v : ev) if (e == hipSuccess && !v) e = hipEventCreateWithFlags(&v, hipEventDisableTiming);
        if (e != hipSuccess) (void) hipGetLastError();
        return e;
    }
};

struct rwkv_mi_batch {
    rwkv_context * ctx = nullptr;      // the caller's context: model, device, error word
    rwkv_context * run = nullptr;      // the batch's own context (stream, scratch, tokens, logits)
    size_t n_slots = 0;
    int64_t state_len = 0;
    DevBuf<float> states;              // [2][n_slots][state_len]
    std::vector<uint8_t> parity;
    // The words of a call travel in staged tables (devmem.h, Staged): one device buffer with its pinned staging, the five
    // untyped ones laid out by call_layout.h. Who allocates each, and when it grows, is said where it is done (batch_ensure_*).
    StagedRows<RowState> rows;         // [2][n_slots]: the row tables of a call (a device loop alternates between the two)
    DrawState draw;                    // the slots' draw state: counters (zero at creation), sampler scratch, occurrence and bias tables
    // the row table of a drawing call, [n_slots] (rows.h, DrawRow: filled by DrawState::row) -- allocated with the sampler's buffers by the
    // first drawing call -- and the form of the current call's kernel
    StagedRows<DrawRow> draw_rows;
    DrawForm form;
    // guided decoding (rwkv_mi_batch_guide_*): the guides' dense tables next[n_states][n_vocab], shared by the slots (which guide a slot has, and
    // its state and miss words, are the draw state's)
    DevBuf<uint16_t> guides[RWKV_MI_GUIDE_MAX];
    uint32_t guide_states[RWKV_MI_GUIDE_MAX] = {};   // n_states of each (0: the id is free)
    // ragged passes (rwkv_mi_batch_eval_ragged*): the tables of a call (SegLayout); the long segments stay on the host
    Staged seg;
    std::vector<SegState> long_segs;
    SegPass pass;
    // the device loops (batch_run_passes): what the polled ones read between blocks -- allocated by the first of them -- and the passes the
    // last loop enqueued
    BlockPoll poll;
    size_t last_loop_passes = 0;
    // rwkv_mi_batch_decode_until: the stop words of a call (StopLayout), the device pointers of the current call and where its lengths and
    // reasons, which come back, lie
    Staged stop_words;
    StopTables stop{};
    Field<uint32_t> stop_lens, stop_reasons;
    // rwkv_mi_batch_decode_beam: the per-row words of a call (BeamLayout)
    Staged beam;
    // rwkv_mi_batch_eval_draft: the logits of every token of a pass [T][n_vocab] and the stash of its recurrences' inputs (kernels.h, DraftStash),
    // both grown to the largest call so far; the layers' vectors and the words a pass leaves (DraftLayout) -- allocated by the first draft call
    DevBuf<float> d_draft_logits;
    DevBuf<float> d_draft_stash;
    DevBuf<DraftLayer> d_draft_layers;
    Staged draft_words;
    // rwkv_mi_batch_serve: the words of a call (ServeLayout); the fresh state every request without a from_slot starts from, filled once --
    // allocated by the first call
    Staged serve;
    DevBuf<float> serve_fresh;          // [state_len]
    LogprobReport lp;                   // the report of the batch's emitting calls (rwkv_mi_batch_set_logprobs)
    // the serve session open on the batch (rwkv_mi_batch_serve_open; owned by its handle until close, or closed by rwkv_mi_batch_free):
    // while there is one, batch_begin rejects every call that runs a pass
    rwkv_mi_serve_session * session = nullptr;

    float * slot_buf(size_t slot, int p) const { return states.p + ((size_t) p * n_slots + slot) * (size_t) state_len; }
};

struct rwkv_mi_serve_session;

// errors of the batch's own context are reported on the caller's
static bool batch_fail_through(rwkv_mi_batch * B) { B->ctx->last_error |= B->run->last_error; B->run->last_error = 0; return false; }

#define BATCH_HIP_OK(B, CALL) \
    do { hipError_t e_ = (CALL); RW_CTX_CHECK((B)->ctx, RWKV_ERROR_GRAPH, false, e_ == hipSuccess, "HIP error: %s", hipGetErrorString(e_)); } while (0)

// what every body starts with, before it looks at an argument: no error yet, the batch's own context prints as the caller's does, the
// batch's device is current
static bool batch_begin(rwkv_mi_batch * B) {
    B->ctx->last_error = RWKV_ERROR_NONE;
    RW_CTX_CHECK(B->ctx, RWKV_ERROR_ARGS, false, B->session == nullptr, "a serve session is open on this batch (rwkv_mi_batch_serve_close ends it)");
    B->run->print_errors = B->ctx->print_errors;
    BATCH_HIP_OK(B, hipSetDevice(B->ctx->model->device));
    return true;
}

// What a batch call is: a point on three axes. The input -- one token per row, or a segment per row (lens); the draw -- none,
// the sampler, or the penalised sampler; the repeat -- one pass (batch_pass, batch_draft) or a device loop. The loops are one driver
// (batch_run_passes: the passes, their blocks, the poll that ends them) and what each body adds to it: batch_loop n_tokens steps (no draw
// means the greedy argmax), batch_until every row ending by itself, batch_serve a queue of requests behind the rows, batch_beam (its own
// description, BeamCall) a selection behind every pass. Every entry point fills in this description and calls one body. The REPORT
//  is a fourth property, the batch's own: a call that emits tokens -- a draw, or a loop's argmax -- records them when
// B->lp.enabled; the bodies branch on that and on `emits`, never on who called.
struct BatchCall {
    const uint32_t * slots, * tokens;   // row i is slot slots[i] fed tokens[i] ...
    size_t n;
    // ... or the next lens[i] of tokens. `ragged` says only that lens is REQUIRED: batch_check_rows picks its NULL-argument message by it and
    // nothing else reads it -- past that check ragged == (lens != NULL), and everything branches on lens
    bool ragged = false;
    const uint32_t * lens = nullptr;
    Draw draw = Draw::none;
    const rwkv_mi_sample_params * params = nullptr;        // [n], with a draw
    const rwkv_mi_penalty_params * penalties = nullptr;    // [n], with the penalised draw
    // what a single pass reports: the logits of each row's last token; the sampled tokens (with a draw); per-token scores (ragged, no draw)
    float * logits_out = nullptr;
    uint32_t * sampled_out = nullptr;
    const uint32_t * targets = nullptr;
    float * logprobs_out = nullptr;
    uint32_t * argmax_out = nullptr;
    // rwkv_mi_batch_decode_until (until: the call is one; batch_until is its body): a budget and stop sequences per row, the rows' sequences back
    // to back in seq_lens / seq_tokens; tokens_out is [n][stride]
    bool until = false;
    const rwkv_mi_stop_params * stops = nullptr;
    const uint32_t * seq_lens = nullptr, * seq_tokens = nullptr;
    size_t stride = 0;
    uint32_t * lens_out = nullptr;
    uint32_t * stopped_by_out = nullptr;
    // rwkv_mi_batch_serve (batch_serve is its body): slots are the call's lanes, tokens is unused; the queue of n_requests requests with their
    // prompts back to back, their sequences in seq_lens / seq_tokens; tokens_out, lens_out and stopped_by_out are per request
    const rwkv_mi_serve_request * requests = nullptr;
    size_t n_requests = 0;
    const uint32_t * prompts = nullptr;
    uint32_t * lane_out = nullptr, * start_pass_out = nullptr, * last_request_out = nullptr;
    // rwkv_mi_batch_serve_ex (serve_ex: the call is one; the same body): what a request carries beyond its struct -- a guide with its start
    // state, the slot whose bias table it reads -- and its final guide words back; on a reporting batch the call fills the report
    bool serve_ex = false;
    const rwkv_mi_serve_extra * extras = nullptr;
    uint32_t * guide_state_out = nullptr, * guide_misses_out = nullptr;
};

// n, slots, lens and tokens of a call: no slot changes when they are rejected. Row i feeds lens[i] consecutive tokens to slot slots[i]; the
// form without lens has every length 1 and checks tokens[i] with its row. *T_out = the tokens of the pass.
static bool batch_check_rows(rwkv_mi_batch * B, const BatchCall & c, size_t * T_out) {
    rwkv_context * ctx = B->ctx;
    if (c.ragged) RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, c.slots != nullptr && c.lens != nullptr && c.tokens != nullptr, "slots, lens or tokens is NULL");
    else RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, c.slots != nullptr && c.tokens != nullptr, "slots or tokens is NULL");
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, c.n > 0 && c.n <= B->n_slots, "n (%zu) must be in 1 .. %zu", c.n, B->n_slots);
    const size_t n_vocab = (size_t) ctx->model->n_vocab();
    std::vector<uint8_t> seen(B->n_slots, 0);
    uint64_t T = 0;
    for (size_t i = 0; i < c.n; i++) {
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, c.slots[i] < B->n_slots, "slot %" PRIu32 " at index %zu is out of range (0 .. %zu)", c.slots[i], i, B->n_slots - 1);
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, !seen[c.slots[i]], "slot %" PRIu32 " appears twice", c.slots[i]);
        seen[c.slots[i]] = 1;
        if (!c.lens) {
            RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, c.tokens[i] < n_vocab, "Token at index %zu (%" PRIu32 ") is out of range (0 .. %zu)", i, c.tokens[i], n_vocab - 1);
            T++;
            continue;
        }
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, c.lens[i] > 0, "lens[%zu] is 0", i);
        T += c.lens[i];
        // (token positions are 32-bit words of the segment table)
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, T <= (uint64_t) INT32_MAX, "the lengths add up to more than %d tokens", INT32_MAX);
    }
    for (size_t t = 0; c.lens && t < (size_t) T; t++)
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, c.tokens[t] < n_vocab, "Token at index %zu (%" PRIu32 ") is out of range (0 .. %zu)", t, c.tokens[t], n_vocab - 1);
    *T_out = (size_t) T;
    return true;
}

// row tables of the n named slots into the staging (the stream has been drained): table 0 takes a slot from its current buffer into the
// other one, table 1 -- what the odd passes of a loop run on -- is the reverse
static void batch_stage_rows(rwkv_mi_batch * B, const uint32_t * slots, size_t n, int tables) {
    for (int tb = 0; tb < tables; tb++)
        for (size_t i = 0; i < n; i++) {
            const int p = B->parity[slots[i]] ^ tb;
            B->rows.h()[(size_t) tb * B->n_slots + i] = RowState{B->slot_buf(slots[i], p), B->slot_buf(slots[i], p ^ 1)};
        }
}

// the first n rows of the staged tables, whoever staged them, to the device
static bool batch_upload_rows(rwkv_mi_batch * B, size_t n, int tables) {
    for (int tb = 0; tb < tables; tb++)
        BATCH_HIP_OK(B, B->rows.upload_rows((size_t) tb * B->n_slots, (size_t) tb * B->n_slots + n, B->run->stream));
    return true;
}

// row tables of the n named slots and the tokens into the batch's device words
static bool batch_upload(rwkv_mi_batch * B, const BatchCall & c, int tables) {
    rwkv_context * run = B->run;
    BATCH_HIP_OK(B, hipStreamSynchronize(run->stream));   // (the previous call's copies may still read the staging)
    batch_stage_rows(B, c.slots, c.n, tables);
    memcpy(run->h_tokens.p, c.tokens, c.n * sizeof(uint32_t));
    if (!batch_upload_rows(B, c.n, tables)) return false;
    BATCH_HIP_OK(B, hipMemcpyAsync(run->d_tokens.p, run->h_tokens.p, c.n * sizeof(uint32_t), hipMemcpyHostToDevice, run->stream));
    return true;
}

// the sampling arguments of a call (checked after batch_check_rows, before anything changes)
static bool batch_check_params(rwkv_mi_batch * B, const rwkv_mi_sample_params * params, size_t n, bool u_used) {
    rwkv_context * ctx = B->ctx;
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, params != nullptr, "params is NULL");
    for (size_t i = 0; i < n; i++) {
        const rwkv_mi_sample_params & p = params[i];
        // (written so that a NaN fails each comparison)
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, p.temperature >= 0.0f && p.top_p >= 0.0f && p.top_p <= 1.0f && (!u_used || p.u < 1.0f),
                     "bad sampling arguments at index %zu (temperature %g, top_p %g, u %g)", i, (double) p.temperature, (double) p.top_p, (double) p.u);
    }
    return true;
}

// the penalties of a call (checked with the other arguments, before anything changes)
static bool batch_check_penalties(rwkv_mi_batch * B, const rwkv_mi_penalty_params * penalties, size_t n) {
    RW_CTX_CHECK(B->ctx, RWKV_ERROR_ARGS, false, penalties != nullptr, "penalties is NULL");
    for (size_t i = 0; i < n; i++) if (!check_penalty(B->ctx, penalties[i].presence, penalties[i].frequency, i)) return false;
    return true;
}

// ---- guided decoding: which calls see a guide (rwkv_mi_batch_guide_*) ----

// whether a call names a slot with a guide attached (its slots have been checked)
static bool batch_names_guided(const rwkv_mi_batch * B, const uint32_t * slots, size_t n) {
    for (size_t i = 0; i < n; i++) if (B->draw.guide_of[slots[i]] != RWKV_MI_NO_GUIDE) return true;
    return false;
}

// the greedy family has no sampler to mask: a call of it that names a guided slot is rejected with its other arguments
static bool batch_check_unguided(rwkv_mi_batch * B, const uint32_t * slots, size_t n, const char * call) {
    RW_CTX_CHECK(B->ctx, RWKV_ERROR_ARGS, false, !batch_names_guided(B, slots, n),
                 "%s takes no slot with a guide attached (guided greedy is temperature 0 of the sampled calls)", call);
    return true;
}

// what the calls on one slot's draw state start with
static bool batch_slot_call(rwkv_mi_batch * B, size_t slot) {
    rwkv_context * ctx = B->ctx;
    ctx->last_error = RWKV_ERROR_NONE;
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, slot < B->n_slots, "slot %zu is out of range", slot);
    return true;
}

// ---- ragged passes: row i feeds lens[i] consecutive tokens to slot slots[i] ----

// the token words and the tables of a ragged call, grown where needed (new buffers first: a failure leaves the batch as it was), then
// filled and uploaded: one copy for the tables, one for the tokens
static bool batch_upload_ragged(rwkv_mi_batch * B, const BatchCall & c, size_t T) {
    rwkv_context * ctx = B->ctx;
    rwkv_context * run = B->run;
    const uint32_t * slots = c.slots, * lens = c.lens;
    const size_t n = c.n;
    const Model & m = *ctx->model;
    BATCH_HIP_OK(B, hipStreamSynchronize(run->stream));   // (the previous call's copies may still read the staging)
    if (T > run->d_tokens.count) {
        const hipError_t e = grow(want(run->d_tokens, T), want(run->h_tokens, T));
        RW_CTX_CHECK(ctx, RWKV_ERROR_ALLOC, false, e == hipSuccess, "cannot allocate the token words of %zu tokens: %s", T, hipGetErrorString(e));
    }
    size_t n_short = 0;
    for (size_t i = 0; i < n; i++) if (!seg_takes_seq_kernel(m, lens[i])) n_short++;
    const SegLayout L(n, n_short, T);
    if (L.bytes > B->seg.bytes()) {   // (grown to the largest call so far)
        const hipError_t e = grow(want(B->seg, L.bytes));
        RW_CTX_CHECK(ctx, RWKV_ERROR_ALLOC, false, e == hipSuccess, "cannot allocate the segment tables of %zu tokens: %s", T, hipGetErrorString(e));
    }
    SegState * segs = B->seg.h(L.segs), * shorts = B->seg.h(L.shorts);
    int32_t * seg_of = B->seg.h(L.seg_of), * last = B->seg.h(L.last);
    B->long_segs.clear();
    int32_t t = 0;
    size_t k = 0;
    for (size_t i = 0; i < n; i++) {
        const int p = B->parity[slots[i]];
        const SegState g{B->slot_buf(slots[i], p), B->slot_buf(slots[i], p ^ 1), t, t + (int32_t) lens[i]};
        segs[i] = g;
        if (seg_takes_seq_kernel(m, lens[i])) B->long_segs.push_back(g); else shorts[k++] = g;
        for (int32_t j = g.t0; j < g.t1; j++) seg_of[j] = (int32_t) i;
        last[i] = g.t1 - 1;
        t = g.t1;
    }
    memcpy(run->h_tokens.p, c.tokens, T * sizeof(uint32_t));
    BATCH_HIP_OK(B, B->seg.upload(0, L.bytes, run->stream));
    BATCH_HIP_OK(B, hipMemcpyAsync(run->d_tokens.p, run->h_tokens.p, T * sizeof(uint32_t), hipMemcpyHostToDevice, run->stream));
    SegPass & ps = B->pass;
    ps.d_segs = B->seg.d(L.segs); ps.d_short = B->seg.d(L.shorts);
    ps.d_seg_of = B->seg.d(L.seg_of); ps.d_last = B->seg.d(L.last);
    ps.h_long = B->long_segs.data();
    ps.n = (int64_t) n; ps.n_short = (int64_t) n_short; ps.n_long = (int64_t) B->long_segs.size();
    return true;
}

// ---- stop sequences and budgets (rwkv_mi_batch_decode_until) ----

// the budgets and stop sequences of `n` rows (or requests), checked with the other arguments, before anything changes
static bool batch_check_stops(rwkv_mi_batch * B, const rwkv_mi_stop_params * stops, size_t n, const uint32_t * seq_lens, const uint32_t * seq_tokens, size_t stride,
                              const uint32_t * lens_out) {
    rwkv_context * ctx = B->ctx;
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, stops != nullptr && lens_out != nullptr, "stops or lens_out is NULL");
    const size_t n_vocab = (size_t) ctx->model->n_vocab();
    size_t n_seqs = 0, n_toks = 0;
    for (size_t i = 0; i < n; i++) {
        const rwkv_mi_stop_params & sp = stops[i];
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, sp.max_tokens > 0, "max_tokens at index %zu is 0", i);
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, (size_t) sp.max_tokens <= stride, "stride (%zu) is less than max_tokens at index %zu (%" PRIu32 ")", stride, i, sp.max_tokens);
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, sp.n_seqs <= RWKV_MI_STOP_MAX_SEQS, "n_seqs at index %zu (%" PRIu32 ") is above %d", i, sp.n_seqs, RWKV_MI_STOP_MAX_SEQS);
        n_seqs += sp.n_seqs;
    }
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, n_seqs == 0 || seq_lens != nullptr, "seq_lens is NULL");
    for (size_t s = 0; s < n_seqs; s++) {
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, seq_lens[s] > 0 && seq_lens[s] <= RWKV_MI_STOP_MAX_LEN, "the length of stop sequence %zu (%" PRIu32 ") must be in 1 .. %d",
                     s, seq_lens[s], RWKV_MI_STOP_MAX_LEN);
        n_toks += seq_lens[s];
    }
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, n_toks == 0 || seq_tokens != nullptr, "seq_tokens is NULL");
    for (size_t t = 0; t < n_toks; t++)
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, seq_tokens[t] < n_vocab, "stop token at index %zu (%" PRIu32 ") is out of range (0 .. %zu)", t, seq_tokens[t], n_vocab - 1);
    return true;
}

// The next row of a call's StopRow table: its parameters and where its sequences start in the flat tables. *n_seqs and *n_toks are the
// sequences and tokens of the rows before it on entry, with it on return (after the last row: the call's totals).
static StopRow stop_row(const rwkv_mi_stop_params & sp, const uint32_t * seq_lens, size_t * n_seqs, size_t * n_toks) {
    const StopRow row{sp.max_tokens, sp.n_seqs, (uint32_t) *n_seqs, (uint32_t) *n_toks};
    for (uint32_t s = 0; s < sp.n_seqs; s++) *n_toks += seq_lens[*n_seqs + s];
    *n_seqs += sp.n_seqs;
    return row;
}

// the poll words of the batch and the stop words: on the first call of the family, for the largest call there is (n_slots rows of
// RWKV_MI_STOP_MAX_SEQS sequences of RWKV_MI_STOP_MAX_LEN tokens)
static bool batch_ensure_stop(rwkv_mi_batch * B) {
    const size_t bytes = StopLayout(B->n_slots, B->n_slots * RWKV_MI_STOP_MAX_SEQS, B->n_slots * RWKV_MI_STOP_MAX_SEQS * RWKV_MI_STOP_MAX_LEN).bytes;
    hipError_t e = B->poll.ensure();
    if (e == hipSuccess && !B->stop_words) e = grow(want(B->stop_words, bytes));
    RW_CTX_CHECK(B->ctx, RWKV_ERROR_ALLOC, false, e == hipSuccess, "cannot allocate the stop tables of %zu slots: %s", B->n_slots, hipGetErrorString(e));
    return true;
}

// the stop words of the n rows, one upload per call (after batch_upload: the stream has been drained, the staging is free): every row live,
// no length, no reason, n rows to go
static bool batch_upload_stops(rwkv_mi_batch * B, const BatchCall & c) {
    const size_t n = c.n;
    size_t n_seqs = 0, n_toks = 0;
    const Staged & w = B->stop_words;
    for (size_t i = 0; i < n; i++) (void) stop_row(c.stops[i], c.seq_lens, &n_seqs, &n_toks);   // (the call's totals: the layout needs them)
    const StopLayout L(n, n_seqs, n_toks);
    size_t seq0 = 0, tok0 = 0;
    for (size_t i = 0; i < n; i++) w.h(L.rows)[i] = stop_row(c.stops[i], c.seq_lens, &seq0, &tok0);
    for (size_t i = 0; i < n; i++) { w.h(L.live)[i] = 1u; w.h(L.lens)[i] = 0u; w.h(L.reasons)[i] = RWKV_MI_NO_TOKEN; }
    *w.h(L.count) = (uint32_t) n;
    if (n_seqs) memcpy(w.h(L.seq_lens), c.seq_lens, L.seq_lens.bytes());
    if (n_toks) memcpy(w.h(L.seq_tokens), c.seq_tokens, L.seq_tokens.bytes());
    BATCH_HIP_OK(B, w.upload(0, L.bytes, B->run->stream));
    B->stop = StopTables{w.d(L.rows), w.d(L.seq_lens), w.d(L.seq_tokens), w.d(L.live), w.d(L.lens), w.d(L.reasons), w.d(L.count)};
    B->stop_lens = L.lens; B->stop_reasons = L.reasons;
    return true;
}

// ---- the bodies of the batch calls ----

// every argument of a call, nothing changed yet, in the order the entry points report them: rows, targets, params, penalties. u_used: the rows'
// u is read (a single pass; in a loop the generator draws)
static bool batch_check_args(rwkv_mi_batch * B, const BatchCall & c, bool u_used, size_t * T_out) {
    if (!batch_check_rows(B, c, T_out) || !check_targets(B->ctx, c.targets, *T_out, c.logprobs_out)) return false;
    if (c.draw != Draw::none && !batch_check_params(B, c.params, c.n, u_used)) return false;
    if (c.draw == Draw::penalized && !batch_check_penalties(B, c.penalties, c.n)) return false;
    return !c.until || batch_check_stops(B, c.stops, c.n, c.seq_lens, c.seq_tokens, c.stride, c.lens_out);
}

// the form of the call's draw kernel -- decided here, once, from the slots the call names; everything after reads B->form -- and the buffers
// the call needs: the stop tables; for a drawing call the row table with its pinned staging, on the first one, then the slots' own buffers
// (B->draw; the plain sampler allocates none of the penalty tables)
static bool batch_ensure_draw(rwkv_mi_batch * B, const BatchCall & c) {
    B->form = B->draw.form(c.draw, c.slots, c.n);
    if (c.until && !batch_ensure_stop(B)) return false;
    if (c.draw == Draw::none) return true;
    const size_t n = B->n_slots;
    const hipError_t e = grow(want(B->draw_rows, B->draw_rows ? 0 : n));
    RW_CTX_CHECK(B->ctx, RWKV_ERROR_ALLOC, false, e == hipSuccess, "cannot allocate the sampler's row tables for %zu slots: %s", n, hipGetErrorString(e));
    return B->draw.ensure_sampler(B->ctx, B->run->stream) && (c.draw != Draw::penalized || B->draw.ensure_penalty(B->ctx, B->run->stream));
}

// the row table of the n named slots, one upload per call (after batch_upload*: the stream has been drained, the staging is free). loop: the
// generator draws and every step records
static bool batch_upload_draw_rows(rwkv_mi_batch * B, const BatchCall & c, bool loop) {
    const bool pen = c.draw == Draw::penalized;
    for (size_t i = 0; i < c.n; i++) {
        DrawRow & r = B->draw_rows.h()[i];
        r = B->draw.row(c.slots[i], c.params[i], pen ? &c.penalties[i] : nullptr, loop ? 1u : pen ? c.penalties[i].record : 0u, B->guides);
        if (loop) r.p.u = -1.0f;
    }
    BATCH_HIP_OK(B, B->draw_rows.upload_rows(0, c.n, B->run->stream));
    return true;
}

// the rows or the segments of a call (that drains the stream first), then its stop words and its sampler table. loop: both row tables
static bool batch_upload_call(rwkv_mi_batch * B, const BatchCall & c, size_t T, bool loop) {
    if (!(c.lens ? batch_upload_ragged(B, c, T) : batch_upload(B, c, loop ? 2 : 1))) return false;
    if (c.until && !batch_upload_stops(B, c)) return false;
    return c.draw == Draw::none || batch_upload_draw_rows(B, c, loop);
}

// what follows the head of the call's passes (model.h, RowSampler): its draw, the call's whole history and, when it reports, report buffers;
// a loop sets the step
static RowSampler batch_sampler(rwkv_mi_batch * B, uint32_t * hist, const RowReport * report) {
    RowSampler s;
    s.form = B->form; s.rows = B->draw_rows.d(); s.probs = B->draw.probs.p;
    s.hist = hist; s.report = report;
    return s;
}

// a pass that could not be launched: the stream is drained before the call returns (what it had enqueued reads the staging)
static bool batch_fail_drained(rwkv_mi_batch * B) { (void) hipStreamSynchronize(B->run->stream); return batch_fail_through(B); }

static void batch_flip(rwkv_mi_batch * B, const BatchCall & c) { for (size_t i = 0; i < c.n; i++) B->parity[c.slots[i]] ^= 1; }

// One pass: every named slot advances by its token or its segment, then what the call asked for goes back to the host.
static bool batch_pass(rwkv_mi_batch * B, const BatchCall & c) {
    rwkv_context * ctx = B->ctx;
    rwkv_context * run = B->run;
    size_t T = 0;
    if (!batch_begin(B) || !batch_check_args(B, c, true, &T)) return false;
    const bool drawn = c.draw != Draw::none, scoring = c.logprobs_out || c.argmax_out;
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, !drawn || c.sampled_out != nullptr, "sampled_out is NULL");
    if (!batch_ensure_draw(B, c)) return false;
    if (scoring && !ensure_score(run, (int64_t) T)) return batch_fail_through(B);
    const bool report = drawn && B->lp.enabled;   // (a pass emits where it draws)
    if (report && !B->lp.begin(B->ctx, B->run->stream, c.n)) return false;
    if (!batch_upload_call(B, c, T, false)) return false;   // (drains the stream: the staging of the targets is free as well)
    if (c.logprobs_out) {
        memcpy(run->h_score_targets.p, c.targets, T * sizeof(uint32_t));
        BATCH_HIP_OK(B, hipMemcpyAsync(run->d_score_targets.p, run->h_score_targets.p, T * sizeof(uint32_t), hipMemcpyHostToDevice, run->stream));
    }
    // Row i's token lands in the batch's token word i (a ragged pass has read all T of them by then): the 4 n bytes that go back to the host.
    const RowReport rep = B->lp.buffers();
    const RowSampler sampler = batch_sampler(B, nullptr, report ? &rep : nullptr);
    // scoring is the ragged pass with the head on every token (engine.hip, ScorePass): T rows of log-probs / argmax in token order
    ScorePass sp;
    sp.targets = sp.logprobs = c.logprobs_out != nullptr;
    sp.argmax = c.argmax_out != nullptr;
    const bool want_logits = drawn || scoring || c.logits_out;
    const bool ok = c.lens ? forward_segs(run, B->pass, (int64_t) T, want_logits, drawn ? &sampler : nullptr, scoring ? &sp : nullptr)
                           : forward_rows(run, B->rows.d(), (int64_t) c.n, want_logits, drawn ? &sampler : nullptr);
    if (!ok) return batch_fail_drained(B);
    if (drawn) BATCH_HIP_OK(B, hipMemcpyAsync(run->h_tokens.p, run->d_tokens.p, c.n * sizeof(uint32_t), hipMemcpyDeviceToHost, run->stream));
    if (c.logits_out) BATCH_HIP_OK(B, hipMemcpyAsync(c.logits_out, run->d_logits.p, c.n * (size_t) ctx->model->n_vocab() * sizeof(float), hipMemcpyDeviceToHost, run->stream));
    if (c.logprobs_out) BATCH_HIP_OK(B, hipMemcpyAsync(c.logprobs_out, run->d_score_logprobs.p, T * sizeof(float), hipMemcpyDeviceToHost, run->stream));
    if (c.argmax_out) BATCH_HIP_OK(B, hipMemcpyAsync(c.argmax_out, run->d_score_argmax.p, T * sizeof(uint32_t), hipMemcpyDeviceToHost, run->stream));
    BATCH_HIP_OK(B, hipStreamSynchronize(run->stream));
    if (drawn) memcpy(c.sampled_out, run->h_tokens.p, c.n * sizeof(uint32_t));
    batch_flip(B, c);
    if (report) B->lp.done(c.n, 1, nullptr);
    return true;
}

// ---- speculative decoding (rwkv_mi_batch_eval_draft) ----

// what the call checks beyond the rows, params and penalties of its family (nothing changed yet)
static bool batch_check_draft(rwkv_mi_batch * B, const BatchCall & c, const uint32_t * tokens_out) {
    rwkv_context * ctx = B->ctx;
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, tokens_out != nullptr && c.lens_out != nullptr, "tokens_out or lens_out is NULL");
    for (size_t i = 0; i < c.n; i++) {
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, c.lens[i] <= 1u + RWKV_MI_DRAFT_MAX, "lens[%zu] (%" PRIu32 ") is above 1 + RWKV_MI_DRAFT_MAX (%d)", i, c.lens[i], 1 + RWKV_MI_DRAFT_MAX);
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, (size_t) c.lens[i] <= c.stride, "stride (%zu) is less than lens[%zu] (%" PRIu32 ")", c.stride, i, c.lens[i]);
    }
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, !batch_names_guided(B, c.slots, c.n), "rwkv_mi_batch_eval_draft takes no slot with a guide attached");
    return true;
}

// the call's buffers for a pass of T tokens: one decision, a failure leaves every buffer as it was. The layers' vectors are uploaded with the
// first allocation (the stream is drained by the upload that follows)
static bool batch_ensure_draft(rwkv_mi_batch * B, size_t T) {
    rwkv_context * ctx = B->ctx;
    const Model & m = *ctx->model;
    const size_t V = (size_t) m.n_vocab(), D = (size_t) m.n_embed(), L = (size_t) (m.layer_end - m.layer_begin);
    const size_t logits = T * V, stash = L * (size_t) (draft_stash_inputs(m) + 3) * T * D, words = DraftLayout(B->n_slots).bytes;
    const bool first = !B->d_draft_layers;
    if (logits > B->d_draft_logits.count || stash > B->d_draft_stash.count) BATCH_HIP_OK(B, hipStreamSynchronize(B->run->stream));   // (an earlier call may still read the old ones)
    const hipError_t e = grow(want(B->d_draft_logits, logits > B->d_draft_logits.count ? logits : 0), want(B->d_draft_stash, stash > B->d_draft_stash.count ? stash : 0),
                              want(B->d_draft_layers, first ? L : 0), want(B->draft_words, first ? words : 0));
    RW_CTX_CHECK(ctx, RWKV_ERROR_ALLOC, false, e == hipSuccess, "cannot allocate the draft buffers of %zu tokens: %s", T, hipGetErrorString(e));
    if (first) {
        std::vector<DraftLayer> lw(L);
        auto f = [](const DevTensor * t) { return t ? (const float *) t->data : nullptr; };
        for (size_t i = 0; i < L; i++) {
            const LayerW & w = m.layers[m.layer_begin + i];
            const bool faaaa = m.arch_major == 6 || (m.arch_major == 5 && m.arch_minor >= 2);
            lw[i] = DraftLayer{m.arch_major == 7 ? nullptr : f(faaaa ? w.att_time_faaaa : w.att_time_first), m.arch_major >= 6 ? nullptr : f(w.att_time_decay)};
        }
        const hipError_t eu = hipMemcpy(B->d_draft_layers.p, lw.data(), L * sizeof(DraftLayer), hipMemcpyHostToDevice);
        if (eu != hipSuccess) { B->d_draft_layers.reset(); B->draft_words.reset(); }
        BATCH_HIP_OK(B, eu);
    }
    return true;
}

// One draft pass (engine.hip forward_draft): every named slot is fed x0 and its draft in one walk over the weights; the device then decides how
// much of each draft the plain loop of the call's family would have emitted, and puts the slots whose draft did not stand in full back to the
// state after what did. The host learns lens_out and tokens_out after one synchronisation; `keep` never leaves the device in between.
static bool batch_draft(rwkv_mi_batch * B, const BatchCall & c, uint32_t * tokens_out) {
    rwkv_context * ctx = B->ctx;
    rwkv_context * run = B->run;
    size_t T = 0;
    if (!batch_begin(B) || !batch_check_args(B, c, false, &T) || !batch_check_draft(B, c, tokens_out)) return false;
    if (!batch_ensure_draw(B, c) || !batch_ensure_draft(B, T)) return false;
    if (!batch_upload_call(B, c, T, true)) return false;   // (loop: the generator draws, every step records)
    const Model & m = *ctx->model;
    const int W = 1 + RWKV_MI_DRAFT_MAX;
    const DraftLayout DL(B->n_slots);
    const Staged & w = B->draft_words;
    DraftPass d;
    d.stash.base = B->d_draft_stash.p; d.stash.n_in = draft_stash_inputs(m); d.stash.plane = (int64_t) T * m.n_embed();
    d.stash.layer0 = m.layer_begin; d.stash.per_layer = m.state_per_layer();
    d.lw = B->d_draft_layers.p; d.logits_all = B->d_draft_logits.p;
    d.form = B->form; d.rows = B->draw_rows.d(); d.probs = B->draw.probs.p;
    d.keep = w.d(DL.keep); d.out = w.d(DL.out); d.out_stride = W;
    if (!forward_draft(run, B->pass, (int64_t) T, d)) return batch_fail_drained(B);
    const Field<uint32_t> keep = DL.keep.first(c.n), out = DL.out.first(c.n * (size_t) W);   // (the call's c.n rows of both)
    BATCH_HIP_OK(B, w.fetch(keep.off, keep.end(), run->stream));
    BATCH_HIP_OK(B, w.fetch(out.off, out.end(), run->stream));
    if (c.logits_out) BATCH_HIP_OK(B, hipMemcpyAsync(c.logits_out, run->d_logits.p, c.n * (size_t) m.n_vocab() * sizeof(float), hipMemcpyDeviceToHost, run->stream));
    BATCH_HIP_OK(B, hipStreamSynchronize(run->stream));
    for (size_t r = 0; r < c.n; r++) {
        c.lens_out[r] = w.h(DL.keep)[r];
        const uint32_t * e = w.h(DL.out) + r * (size_t) W;
        for (size_t j = 0; j < c.stride; j++) tokens_out[r * c.stride + j] = j < (size_t) W ? e[j] : RWKV_MI_NO_TOKEN;
    }
    batch_flip(B, c);
    return true;
}

// passes per block of a polled device loop: 16, or RWKV_MI_LOOP_BLOCK in 1 .. 1024 (read at the call)
static size_t loop_block() {
    const char * e = getenv("RWKV_MI_LOOP_BLOCK");
    if (!e || !e[0]) return 16;
    char * end = nullptr;
    const long v = strtol(e, &end, 10);
    return (*end == 0 && v >= 1 && v <= 1024) ? (size_t) v : 16;
}

// The passes of a device loop, between the two events its time is taken from. Pass i runs on row table i & 1 and reads the buffers pass i - 1
// wrote; the driver gives the sampler the pass's step and tables (used: this pass's, other: the next one's -- what the loop's kernels rewrite
// to retire, admit or re-parent a row) and `step` enqueues the pass. With a poll_word -- a device word that is 0 once no row has anything
// left to do -- the host decides when to stop enqueuing: passes go out in blocks of K; behind each block the word is copied to pinned memory
// and an event recorded; after enqueuing block b the host waits for the event of block b - 1 (which has long passed, or passes while block b
// runs: the device is never idle for it) and stops when that count is 0. Passes past the end of the work are dead steps, at most 2 K of
// them. Without one, all max_passes passes are enqueued and nothing waits. A pass that could not be launched, or a failed poll, drains the
// stream before the call returns (what has been enqueued reads the staging). B->last_loop_passes: the passes enqueued. A step may enqueue
// more than its pass: what it puts in front of pass 0 (batch_serve's first admission) lies behind ev0, inside the time the loop reports.
template <typename Step>
static bool batch_run_passes(rwkv_mi_batch * B, size_t max_passes, const uint32_t * poll_word, RowSampler & sampler, Step step) {
    rwkv_context * run = B->run;
    const size_t K = poll_word ? loop_block() : max_passes;
    BATCH_HIP_OK(B, hipEventRecord(run->ev0, run->stream));
    size_t passes = 0;
    for (size_t b = 0; passes < max_passes; b++) {
        for (const size_t end = std::min(max_passes, passes + K); passes < end; passes++) {
            sampler.step = (uint32_t) passes;
            sampler.used = B->rows.d() + (passes & 1) * B->n_slots; sampler.other = B->rows.d() + ((passes & 1) ^ 1) * B->n_slots;
            if (!step(sampler)) return batch_fail_drained(B);
        }
        if (!poll_word) break;
        hipError_t e = hipMemcpyAsync(B->poll.count.p + (b & 1), poll_word, sizeof(uint32_t), hipMemcpyDeviceToHost, run->stream);
        if (e == hipSuccess) e = hipEventRecord(B->poll.ev[b & 1], run->stream);
        if (e == hipSuccess && b > 0) e = hipEventSynchronize(B->poll.ev[(b - 1) & 1]);
        if (e != hipSuccess) { (void) hipStreamSynchronize(run->stream); BATCH_HIP_OK(B, e); }
        if (b > 0 && B->poll.count.p[(b - 1) & 1] == 0) break;
    }
    BATCH_HIP_OK(B, hipEventRecord(run->ev1, run->stream));
    B->last_loop_passes = passes;
    return true;
}

// what ends every loop, behind the copies of its results: the stream drained, the time between the driver's two events
static bool batch_passes_done(rwkv_mi_batch * B, float * elapsed_ms) {
    rwkv_context * run = B->run;
    BATCH_HIP_OK(B, hipStreamSynchronize(run->stream));
    if (elapsed_ms) BATCH_HIP_OK(B, hipEventElapsedTime(elapsed_ms, run->ev0, run->ev1));
    return true;
}

// The device loop: n_tokens passes of one token per row, each row's next token chosen on the device -- its argmax, or the call's draw.
// tokens_out: [n][n_tokens]. The plain sampled loop starts the named slots' draw counters from 0. The penalised loop CONTINUES: the named
// slots' counts and draw counters are where the caller left them, and every step records.
static bool batch_loop(rwkv_mi_batch * B, const BatchCall & c, size_t n_tokens, uint32_t * tokens_out, float * elapsed_ms) {
    rwkv_context * ctx = B->ctx;
    rwkv_context * run = B->run;
    size_t T = 0;
    if (!batch_begin(B) || !batch_check_args(B, c, false, &T)) return false;
    if (c.draw == Draw::none && !batch_check_unguided(B, c.slots, c.n, "the greedy loop")) return false;
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, n_tokens > 0, "n_tokens is 0");
    const size_t n = c.n;
    const bool drawn = c.draw != Draw::none;
    if (!batch_ensure_draw(B, c)) return false;
    DevBuf<uint32_t> hist;   // [n_tokens][n], freed on every exit
    BATCH_HIP_OK(B, hist.alloc(n_tokens * n));
    const bool report = B->lp.enabled;   // (every step of a loop emits)
    if (!B->lp.begin(B->ctx, B->run->stream, n_tokens * n)) return false;
    if (!batch_upload_call(B, c, T, true)) return false;
    if (c.draw == Draw::sample) launch_sample_seek_rows(B->draw_rows.d(), (int64_t) n, 0ull, run->stream);   // the named slots' streams start over
    const RowReport rep = B->lp.buffers();
    RowSampler sampler = batch_sampler(B, hist.p, report ? &rep : nullptr);
    // the token of each row lands where its next embedding lookup reads it: sampled inside the pass's chain bracket, or -- the greedy argmax,
    // its report directly behind it -- after the bracket: the event the device's next persistent launch waits on is recorded after both
    const auto step = [&](const RowSampler & s) {
        if (!forward_rows(run, s.used, (int64_t) n, true, drawn ? &s : nullptr)) return false;
        if (!drawn) launch_row_sampler(run, s, (int64_t) n);
        return true;
    };
    if (!batch_run_passes(B, n_tokens, nullptr, sampler, step)) return false;
    std::vector<uint32_t> h(tokens_out ? n_tokens * n : 0);
    if (tokens_out) BATCH_HIP_OK(B, hipMemcpyAsync(h.data(), hist.p, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, run->stream));
    if (!batch_passes_done(B, elapsed_ms)) return false;
    for (size_t r = 0; r < n && tokens_out; r++)
        for (size_t i = 0; i < n_tokens; i++) tokens_out[r * n_tokens + i] = h[i * n + r];
    if (n_tokens & 1) batch_flip(B, c);
    if (report) B->lp.done(n, n_tokens, nullptr);
    return true;
}

// The device loop in which every row ends by itself (rwkv_mi_batch_decode_until): batch_loop's passes, the draw behind the rows' live words and
// followed by the stop test (engine.hip launch_row_sampler, sampling.hip k_stop_rows), which retires a row ON THE DEVICE by rewriting its entries
// of the two row tables -- the model's kernels never learn of it. The driver polls the live count. Passes past a row's retirement are dead
// steps into the row's other buffer.
static bool batch_until(rwkv_mi_batch * B, const BatchCall & c, uint32_t * tokens_out, float * elapsed_ms) {
    rwkv_context * ctx = B->ctx;
    rwkv_context * run = B->run;
    size_t T = 0;
    if (!batch_begin(B) || !batch_check_args(B, c, false, &T)) return false;
    if (c.draw == Draw::none && !batch_check_unguided(B, c.slots, c.n, "the greedy loop")) return false;
    const size_t n = c.n;
    size_t budget = 0;
    for (size_t i = 0; i < n; i++) budget = std::max(budget, (size_t) c.stops[i].max_tokens);
    if (!batch_ensure_draw(B, c)) return false;
    DevBuf<uint32_t> hist;   // [budget][n], freed on every exit; a word no row wrote stays RWKV_MI_NO_TOKEN
    hipError_t he = hist.alloc(budget * n);
    if (he != hipSuccess) (void) hipGetLastError();
    RW_CTX_CHECK(ctx, RWKV_ERROR_ALLOC, false, he == hipSuccess, "cannot allocate the history of %zu steps of %zu rows: %s", budget, n, hipGetErrorString(he));
    const bool report = B->lp.enabled;   // (every step of a live row emits; a slot no row wrote is never read back: LogprobReport::store fills behind lens)
    if (!B->lp.begin(B->ctx, B->run->stream, budget * n)) return false;
    if (!batch_upload_call(B, c, T, true)) return false;
    if (c.draw == Draw::sample) launch_sample_seek_rows(B->draw_rows.d(), (int64_t) n, 0ull, run->stream);   // the named slots' streams start over
    BATCH_HIP_OK(B, hipMemsetAsync(hist.p, 0xFF, budget * n * sizeof(uint32_t), run->stream));
    const RowReport rep = B->lp.buffers();
    RowSampler sampler = batch_sampler(B, hist.p, report ? &rep : nullptr);
    sampler.stop = &B->stop;
    if (!batch_run_passes(B, budget, B->stop.live_count, sampler, [&](const RowSampler & s) { return forward_rows(run, s.used, (int64_t) n, true, &s); })) return false;
    const size_t passes = B->last_loop_passes;
    std::vector<uint32_t> h(tokens_out ? passes * n : 0);
    const uint32_t * h_lens = B->stop_words.h(B->stop_lens), * h_reasons = B->stop_words.h(B->stop_reasons);   // (adjacent: one copy)
    if (tokens_out) BATCH_HIP_OK(B, hipMemcpyAsync(h.data(), hist.p, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, run->stream));
    BATCH_HIP_OK(B, B->stop_words.fetch(B->stop_lens.off, B->stop_reasons.end(), run->stream));
    if (!batch_passes_done(B, elapsed_ms)) return false;
    // (every budget is at most `budget`, and the loop ends on a live count of 0 or at `budget`: every row has retired)
    for (size_t r = 0; r < n; r++)
        RW_CTX_CHECK(ctx, RWKV_ERROR_GRAPH, false, h_lens[r] > 0 && h_lens[r] <= passes, "row %zu did not retire (the device loop failed)", r);
    for (size_t r = 0; r < n; r++) {
        const size_t len = h_lens[r];
        c.lens_out[r] = (uint32_t) len;
        if (c.stopped_by_out) c.stopped_by_out[r] = h_reasons[r];
        for (size_t j = 0; tokens_out && j < c.stride; j++) tokens_out[r * c.stride + j] = j < len ? h[j * n + r] : RWKV_MI_NO_TOKEN;
        if (len & 1) B->parity[c.slots[r]] ^= 1;
    }
    if (report) B->lp.done(n, passes, h_lens);
    return true;
}

// ---- continuous batching (rwkv_mi_batch_serve) ----

// every argument of a serve call, nothing changed yet. *n_prompt_out = the prompt tokens of the queue
static bool batch_check_serve(rwkv_mi_batch * B, const BatchCall & c, size_t * n_prompt_out) {
    rwkv_context * ctx = B->ctx;
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, c.slots != nullptr && c.requests != nullptr && c.prompts != nullptr && c.lens_out != nullptr,
                 "lanes, requests, prompt_tokens or lens_out is NULL");
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, c.n > 0 && c.n <= B->n_slots, "n (%zu) must be in 1 .. %zu", c.n, B->n_slots);
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, c.n_requests >= c.n && c.n_requests < (size_t) SERVE_FREE, "n_requests (%zu) is below the %zu lanes (or above 2^32 - 3)", c.n_requests, c.n);
    if (!c.serve_ex) RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, !B->lp.enabled, "rwkv_mi_batch_serve takes no batch with the log-prob report on");
    else RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, !B->lp.enabled || c.stride > 0, "the log-prob report is on and stride is 0");
    std::vector<uint8_t> is_lane(B->n_slots, 0);
    for (size_t i = 0; i < c.n; i++) {
        const uint32_t s = c.slots[i];
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, s < B->n_slots, "lane slot %" PRIu32 " at index %zu is out of range (0 .. %zu)", s, i, B->n_slots - 1);
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, !is_lane[s], "lane slot %" PRIu32 " appears twice", s);
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, B->draw.guide_of[s] == RWKV_MI_NO_GUIDE && !B->draw.has_bias[s], "lane slot %" PRIu32 " has a guide attached or a bias set", s);
        is_lane[s] = 1;
    }
    const size_t R = c.n_requests, n_vocab = (size_t) ctx->model->n_vocab();
    std::vector<rwkv_mi_sample_params> sp(R);
    std::vector<rwkv_mi_penalty_params> pp(R);
    std::vector<rwkv_mi_stop_params> st(R);
    uint64_t P = 0;
    for (size_t q = 0; q < R; q++) {
        const rwkv_mi_serve_request & rq = c.requests[q];
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, rq.prompt_len > 0, "the prompt of request %zu is empty", q);
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, rq.from_slot == RWKV_MI_NO_SLOT || (rq.from_slot < B->n_slots && !is_lane[rq.from_slot]),
                     "from_slot of request %zu (%" PRIu32 ") is a lane of the call or out of range", q, rq.from_slot);
        P += rq.prompt_len;
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, P <= (uint64_t) INT32_MAX, "the prompts add up to more than %d tokens", INT32_MAX);
        // (the rules of DrawState::cut_set and rep_set, written so that a NaN fails each comparison)
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, rq.min_p >= 0.0f && rq.min_p <= 1.0f, "min_p of request %zu (%g) must be in 0 .. 1", q, (double) rq.min_p);
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, rq.decay >= 0.0f && rq.decay <= 1.0f, "decay of request %zu (%g) must be in 0 .. 1", q, (double) rq.decay);
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, rq.repetition > 0.0f && rq.repetition < INFINITY, "repetition of request %zu (%g) must be finite and above 0", q, (double) rq.repetition);
        sp[q] = rq.sample; pp[q] = rq.penalty; st[q] = rq.stop;
        if (!c.extras) continue;
        // what the request carries beyond its struct: settings come with requests, by the rules of rwkv_mi_batch_guide_attach and _logit_bias_set
        const rwkv_mi_serve_extra & ex = c.extras[q];
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, ex.reserved == 0, "reserved of the extra of request %zu is not 0", q);
        if (ex.guide != RWKV_MI_NO_GUIDE) {
            RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, ex.guide < RWKV_MI_GUIDE_MAX && B->guide_states[ex.guide], "guide of request %zu (%" PRIu32 ") names no guide", q, ex.guide);
            RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, ex.guide_state < B->guide_states[ex.guide], "guide_state of request %zu (%" PRIu32 ") is out of range (guide %" PRIu32
                         " has %" PRIu32 " states)", q, ex.guide_state, ex.guide, B->guide_states[ex.guide]);
            RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, c.draw != Draw::none, "request %zu has a guide in the greedy family (guided greedy is temperature 0 of the sampled one)", q);
        }
        if (ex.bias_slot != RWKV_MI_NO_SLOT) {
            RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, ex.bias_slot < B->n_slots && !is_lane[ex.bias_slot] && B->draw.has_bias[ex.bias_slot],
                         "bias_slot of request %zu (%" PRIu32 ") is a lane of the call, out of range or has no bias set", q, ex.bias_slot);
            RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, c.draw == Draw::penalized, "request %zu has a bias_slot in a family that reads no bias (the penalised one does)", q);
        }
    }
    for (size_t t = 0; t < (size_t) P; t++)
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, c.prompts[t] < n_vocab, "Prompt token at index %zu (%" PRIu32 ") is out of range (0 .. %zu)", t, c.prompts[t], n_vocab - 1);
    if (c.draw != Draw::none && !batch_check_params(B, sp.data(), R, false)) return false;
    if (c.draw == Draw::penalized && !batch_check_penalties(B, pp.data(), R)) return false;
    // the requests' budgets and sequences, by the rules of rwkv_mi_batch_decode_until
    if (!batch_check_stops(B, st.data(), R, c.seq_lens, c.seq_tokens, c.stride, c.lens_out)) return false;
    *n_prompt_out = (size_t) P;
    return true;
}

// the poll words of the batch; the serve buffer for `bytes` and, on the first call, the fresh state: one decision
static bool batch_ensure_serve(rwkv_mi_batch * B, size_t bytes) {
    rwkv_context * ctx = B->ctx;
    const Model & m = *ctx->model;
    hipStream_t st = B->run->stream;
    const bool more = bytes > B->serve.bytes(), first = !B->serve_fresh;   // (grown to the largest call so far)
    if (more) BATCH_HIP_OK(B, hipStreamSynchronize(st));   // (an earlier call may still read the old one)
    hipError_t e = B->poll.ensure();
    if (e == hipSuccess) e = grow(want(B->serve, more ? bytes : 0), want(B->serve_fresh, first ? (size_t) B->state_len : 0));
    RW_CTX_CHECK(ctx, RWKV_ERROR_ALLOC, false, e == hipSuccess, "cannot allocate the serve tables (%zu bytes): %s", bytes, hipGetErrorString(e));
    if (first) {
        if (m.arch_major >= 5) e = hipMemsetAsync(B->serve_fresh.p, 0, (size_t) B->state_len * sizeof(float), st);
        else { launch_fill_state_v4(B->serve_fresh.p, m.n_layer(), m.n_embed(), st); e = hipGetLastError(); }
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) B->serve_fresh.reset();   // (a fresh state that could not be filled is not kept)
        BATCH_HIP_OK(B, e);
    }
    return true;
}

// workgroups per lane of k_serve_reset: one per 128 KiB of state, at most 256
static unsigned serve_chunks(int64_t state_len) {
    const int64_t c = (state_len * (int64_t) sizeof(float) + (128 << 10) - 1) / (128 << 10);
    return (unsigned) std::min<int64_t>(std::max<int64_t>(c, 1), 256);
}

// The device loop with a queue behind it (rwkv_mi_batch_serve): the driver's passes, the draw behind the lanes' DRAW words and
// followed by the scheduler (engine.hip launch_row_sampler; sampling.hip k_serve_rows, k_serve_reset), which emits, feeds prompts, retires and
// admits ON THE DEVICE: between two passes it rewrites a lane's token word, draw row and words and has the request's start state copied into
// the buffer the lane's next pass reads. The model's kernels never learn of it. The admission in front of pass 0 is the same two kernels.
// The driver polls the number of lanes with work, and never enqueues more passes than the queue can need.
// rwkv_mi_batch_serve_ex is the same body: a request's guide table and bias table go into its draw row here, the guide words of the lanes and
// of the requests travel in the serve buffer when a request is guided, and on a reporting batch every pass reports between its choice and
// the scheduler, at (position, request). Without extras and report nothing of that exists: no byte, no launch, no copy more.
static bool batch_serve(rwkv_mi_batch * B, const BatchCall & c, uint32_t * tokens_out, float * elapsed_ms) {
    rwkv_context * ctx = B->ctx;
    rwkv_context * run = B->run;
    size_t n_prompt = 0;
    if (!batch_begin(B) || !batch_check_serve(B, c, &n_prompt)) return false;
    const Model & m = *ctx->model;
    const size_t n = c.n, R = c.n_requests, n_vocab = (size_t) m.n_vocab();
    const bool pen = c.draw == Draw::penalized;
    size_t n_seqs = 0, n_toks = 0, bound = 0;
    bool any_cut = false, any_rep = false, any_guided = false;
    std::vector<StopRow> stop_rows(R);
    for (size_t q = 0; q < R; q++) {
        const rwkv_mi_serve_request & rq = c.requests[q];
        stop_rows[q] = stop_row(rq.stop, c.seq_lens, &n_seqs, &n_toks);
        bound += (size_t) rq.prompt_len - 1 + rq.stop.max_tokens;   // (a lane with work advances its request by one pass: no schedule needs more)
        any_cut |= (rq.top_k != 0u && rq.top_k < n_vocab) || rq.min_p != 0.0f;
        any_rep |= rq.decay != 1.0f || rq.repetition != 1.0f;
        any_guided |= c.extras && c.extras[q].guide != RWKV_MI_NO_GUIDE;
    }
    BatchCall lanes{c.slots, nullptr, n};
    lanes.draw = c.draw;
    if (!batch_ensure_draw(B, lanes)) return false;   // (the draw buffers of the family; the form it derives from the lanes' own settings ...)
    B->form = DrawForm::of(c.draw, any_cut, any_guided, any_rep);   // (... is not the call's: the requests carry theirs)
    const ServeLayout L(n, R, n_prompt, n_seqs, n_toks, c.stride, any_guided);
    if (!batch_ensure_serve(B, L.bytes)) return false;
    // (the entry point that reports, on a batch that does: entry (j, q) is position j of request q -- rows = R, steps = stride)
    const bool report = c.serve_ex && B->lp.enabled;
    if (report && !B->lp.begin(B->ctx, B->run->stream, c.stride * R)) return false;
    BATCH_HIP_OK(B, hipStreamSynchronize(run->stream));   // (the previous call's copies may still read the staging)
    const Staged & w = B->serve;
    ServeReq * reqs = w.h(L.reqs);
    size_t p0 = 0;
    for (size_t q = 0; q < R; q++) {
        const rwkv_mi_serve_request & rq = c.requests[q];
        // (the row of DrawState::row for a loop: the generator draws, every penalised draw records; the counter and the occurrence row are the
        //  lane's, which the scheduler fills in)
        DrawRow row{};
        row.p = rq.sample; row.p.u = -1.0f;
        row.presence = pen ? rq.penalty.presence : 0.0f; row.frequency = pen ? rq.penalty.frequency : 0.0f; row.record = pen ? 1u : 0u;
        row.top_k = rq.top_k; row.min_p = rq.min_p; row.decay = rq.decay; row.repetition = rq.repetition;
        // (its guide's table and its bias slot's, both only read; the guide words are the lane's, which the scheduler fills in as well)
        const rwkv_mi_serve_extra ex = c.extras ? c.extras[q] : rwkv_mi_serve_extra{RWKV_MI_NO_GUIDE, 0u, RWKV_MI_NO_SLOT, 0u};
        if (ex.guide != RWKV_MI_NO_GUIDE) row.next = B->guides[ex.guide].p;
        if (pen && ex.bias_slot != RWKV_MI_NO_SLOT) row.bias = B->draw.bias_of(ex.bias_slot);
        if (any_guided) { w.h(L.req_g_state)[q] = ex.guide != RWKV_MI_NO_GUIDE ? ex.guide_state : 0u; w.h(L.req_g_misses)[q] = 0u; }
        const float * start = rq.from_slot == RWKV_MI_NO_SLOT ? B->serve_fresh.p : B->slot_buf(rq.from_slot, B->parity[rq.from_slot]);
        reqs[q] = ServeReq{row, stop_rows[q], rq.prompt_len, (uint32_t) p0, start};
        p0 += rq.prompt_len;
    }
    for (size_t r = 0; any_guided && r < n; r++) { w.h(L.g_state)[r] = 0u; w.h(L.g_misses)[r] = 0u; }
    memcpy(w.h(L.prompts), c.prompts, L.prompts.bytes());
    if (n_seqs) memcpy(w.h(L.seq_lens), c.seq_lens, L.seq_lens.bytes());
    if (n_toks) memcpy(w.h(L.seq_tokens), c.seq_tokens, L.seq_tokens.bytes());
    for (size_t r = 0; r < n; r++) { w.h(L.lane_slot)[r] = c.slots[r]; w.h(L.req)[r] = SERVE_FREE; w.h(L.pos)[r] = 0u; w.h(L.draw)[r] = 0u; w.h(L.admit)[r] = 0u; w.h(L.last)[r] = RWKV_MI_NO_TOKEN; }
    batch_stage_rows(B, c.slots, n, 2);
    *w.h(L.next) = 0u; *w.h(L.work) = (uint32_t) n;
    for (size_t q = 0; q < R; q++) { w.h(L.lens)[q] = 0u; w.h(L.reasons)[q] = RWKV_MI_NO_TOKEN; w.h(L.lane)[q] = RWKV_MI_NO_TOKEN; w.h(L.start)[q] = RWKV_MI_NO_TOKEN; }
    BATCH_HIP_OK(B, w.upload(0, L.out.off, run->stream));
    BATCH_HIP_OK(B, hipMemsetAsync(w.d(L.out), 0xFF, L.out.bytes(), run->stream));
    if (!batch_upload_rows(B, n, 2)) return false;
    RowServe serve{};
    serve.t = ServeTables{w.d(L.reqs), w.d(L.prompts), w.d(L.seq_lens), w.d(L.seq_tokens), w.d(L.out), (uint32_t) c.stride,
                          w.d(L.lens), w.d(L.reasons), w.d(L.lane), w.d(L.start), w.d(L.req), w.d(L.pos), w.d(L.draw), w.d(L.admit), w.d(L.last), w.d(L.lane_slot),
                          c.draw != Draw::none ? B->draw_rows.d() : nullptr, B->draw.counters.p, B->draw.counts.p, w.d(L.next), w.d(L.work),
                          (uint32_t) R, (uint32_t) n_vocab,
                          any_guided ? w.d(L.g_state) : nullptr, any_guided ? w.d(L.g_misses) : nullptr,
                          any_guided ? w.d(L.req_g_state) : nullptr, any_guided ? w.d(L.req_g_misses) : nullptr};
    serve.state_len = B->state_len; serve.chunks = serve_chunks(B->state_len);
    const RowReport rep = B->lp.buffers();
    RowSampler sampler = batch_sampler(B, nullptr, report ? &rep : nullptr);
    sampler.serve = &serve;
    const auto step = [&](const RowSampler & s) {
        if (s.step == 0) {
            // lane r takes request r: the admission in front of pass 0 copies into what the table of pass 1 writes, which is what pass 0 reads
            launch_serve_rows(serve.t, (int64_t) n, run->d_tokens.p, UINT32_MAX, s.other, s.used, run->stream);
            launch_serve_reset(serve.t, (int64_t) n, serve.chunks, s.other, serve.state_len, run->stream);
        }
        return forward_rows(run, s.used, (int64_t) n, true, &s);
    };
    if (!batch_run_passes(B, bound, serve.t.work, sampler, step)) return false;
    BATCH_HIP_OK(B, w.fetch(L.down, L.bytes, run->stream));
    if (!batch_passes_done(B, elapsed_ms)) return false;
    const uint32_t * lens = w.h(L.lens), * reasons = w.h(L.reasons), * lane = w.h(L.lane), * start = w.h(L.start), * last = w.h(L.last), * out = w.h(L.out);
    // (the queue's work fits the bound, and the loop ends on a work count of 0 or at the bound: every request has been served to its end)
    for (size_t q = 0; q < R; q++)
        RW_CTX_CHECK(ctx, RWKV_ERROR_GRAPH, false, lane[q] < n && lens[q] > 0 && lens[q] <= c.requests[q].stop.max_tokens &&
                     (reasons[q] != RWKV_MI_NO_TOKEN || lens[q] == c.requests[q].stop.max_tokens), "request %zu did not end (the device loop failed)", q);
    for (size_t r = 0; r < n; r++) RW_CTX_CHECK(ctx, RWKV_ERROR_GRAPH, false, last[r] < R, "lane %zu served no request (the device loop failed)", r);
    for (size_t q = 0; q < R; q++) {
        c.lens_out[q] = lens[q];
        if (c.stopped_by_out) c.stopped_by_out[q] = reasons[q];
        if (c.lane_out) c.lane_out[q] = lane[q];
        if (c.start_pass_out) c.start_pass_out[q] = start[q];
        if (tokens_out) memcpy(tokens_out + q * c.stride, out + q * c.stride, c.stride * 4);
        // (an unguided request's words are 0 and 0)
        if (c.guide_state_out) c.guide_state_out[q] = any_guided ? w.h(L.req_g_state)[q] : 0u;
        if (c.guide_misses_out) c.guide_misses_out[q] = any_guided ? w.h(L.req_g_misses)[q] : 0u;
    }
    for (size_t r = 0; r < n; r++) {
        // the lane ran one pass after the other from pass 0 to the last one of its last request: that many times its buffers changed places
        const size_t q = last[r], ran = (size_t) start[q] + c.requests[q].prompt_len - 1 + lens[q];
        if (c.last_request_out) c.last_request_out[r] = (uint32_t) q;
        if (ran & 1) B->parity[c.slots[r]] ^= 1;
    }
    if (report) B->lp.done(R, c.stride, lens);
    return true;
}

// ---- serve sessions (rwkv_mi_batch_serve_open ..) ----

// The device loop of batch_serve cut at its block boundaries and owned by a handle. The words live in one staged table (SessionLayout): a
// submit writes its ring entry into the staging, the next block carries it up; what a block brings back goes into staging of its own, one
// half per block parity, because the fetch of block b runs while the host reads what block b - 1 left. Every decision is the book's
// (session_book.h); this code enqueues, copies and waits for events.
struct rwkv_mi_serve_session {
    rwkv_mi_batch * B = nullptr;
    std::vector<uint32_t> lanes;
    std::vector<uint8_t> is_lane;           // [n_slots]
    Draw draw = Draw::none;
    DrawForm form;
    rwkv_mi_serve_limits lim{};
    SessionLayout L;
    Staged words;
    PinBuf<uint8_t> down;                   // [2][L.bytes - L.down]
    hipEvent_t ev[2] = {nullptr, nullptr};
    SessionBook book;
    RowSession dev{};
    bool failed = false;                    // a block could not be enqueued or read: only close is left
    ~rwkv_mi_serve_session() { for (hipEvent_t e : ev) if (e) (void) hipEventDestroy(e); }
};

// what every session call starts with: batch_begin without its session check
static bool session_begin(rwkv_mi_serve_session * S) {
    rwkv_mi_batch * B = S->B;
    B->ctx->last_error = RWKV_ERROR_NONE;
    B->run->print_errors = B->ctx->print_errors;
    BATCH_HIP_OK(B, hipSetDevice(B->ctx->model->device));
    RW_CTX_CHECK(B->ctx, RWKV_ERROR_GRAPH, false, !S->failed, "the session has failed (rwkv_mi_batch_serve_close frees it)");
    return true;
}

// One block: what was submitted and cancelled since the last one goes up, the admission in front of the first pass, K passes, the fetch of
// the words that come back and the block's event.
static bool session_enqueue(rwkv_mi_serve_session * S) {
    rwkv_mi_batch * B = S->B;
    rwkv_context * run = B->run;
    hipStream_t st = run->stream;
    const SessionLayout & L = S->L;
    const Staged & w = S->words;
    const size_t n = S->lanes.size();
    const SessionBook::Block b = S->book.begin_block();
    const size_t half = (size_t) (b.index & 1);
    S->failed = true;   // (until everything below has been enqueued)
    for (uint32_t id = b.upload_from; id != b.upload_to;) {
        const size_t e0 = L.entry_of(id), count = std::min<size_t>(b.upload_to - id, L.capacity - e0);
        size_t from = 0, to = 0;
        L.reqs_range(e0, e0 + count, &from, &to);
        BATCH_HIP_OK(B, w.upload(from, to, st));
        L.words_range(e0, e0 + count, &from, &to);
        BATCH_HIP_OK(B, w.upload(from, to, st));
        id += (uint32_t) count;
    }
    const Field<uint32_t> ch = L.cancel_half(half);   // (block b - 2, which read this half, has been consumed)
    memcpy(w.h(ch), S->book.cancel.data(), ch.bytes());
    BATCH_HIP_OK(B, w.upload(ch.off, ch.end(), st));
    RowSession & d = S->dev;
    d.s.tail = b.tail; d.s.cancel = w.d(ch);
    RowSampler sampler = batch_sampler(B, nullptr, nullptr);
    sampler.form = S->form; sampler.session = &d;
    const auto table = [&](uint32_t pass) { return B->rows.d() + (size_t) (pass & 1u) * B->n_slots; };
    // idle lanes take what has arrived at the block's first pass: the scheduler step "after pass first_pass - 1", admissions only
    d.s.admit_only = 1u;
    launch_session_rows(d.s, (int64_t) n, run->d_tokens.p, b.first_pass - 1u, table(b.first_pass + 1u), table(b.first_pass), st);
    launch_serve_reset(d.s.t, (int64_t) n, d.chunks, table(b.first_pass + 1u), d.state_len, st);
    d.s.admit_only = 0u;
    for (size_t i = 0; i < S->book.K; i++) {
        const uint32_t pass = b.first_pass + (uint32_t) i;
        sampler.step = pass; sampler.used = table(pass); sampler.other = table(pass + 1u);
        if (!forward_rows(run, sampler.used, (int64_t) n, true, &sampler)) return batch_fail_drained(B);
    }
    const size_t down_bytes = L.bytes - L.down;
    hipError_t e = hipMemcpyAsync(S->down.p + half * down_bytes, w.dev.p + L.down, down_bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipEventRecord(S->ev[half], st);
    if (e != hipSuccess) { (void) hipStreamSynchronize(st); BATCH_HIP_OK(B, e); }
    S->failed = false;
    return true;
}

// reads the words of the enqueued blocks below `upto`, oldest first, each behind its event
static bool session_consume(rwkv_mi_serve_session * S, uint64_t upto) {
    rwkv_mi_batch * B = S->B;
    const SessionLayout & L = S->L;
    const size_t down_bytes = L.bytes - L.down;
    while (S->book.consumed < upto) {
        const size_t half = (size_t) (S->book.consumed & 1);
        const hipError_t e = hipEventSynchronize(S->ev[half]);
        if (e != hipSuccess) { S->failed = true; (void) hipStreamSynchronize(B->run->stream); BATCH_HIP_OK(B, e); }
        const uint8_t * base = S->down.p + half * down_bytes;
        const auto at = [base, &L](const Field<uint32_t> & f) { return (const uint32_t *) (base + (f.off - L.down)); };
        const bool g = L.req_g_state.count != 0;
        S->book.consume(SessionWords{at(L.next), at(L.work), at(L.ids), at(L.done), at(L.lens), at(L.reasons), at(L.lane), at(L.start), at(L.end), at(L.revived),
                                     g ? at(L.req_g_state) : nullptr, g ? at(L.req_g_misses) : nullptr, at(L.out)});
    }
    return true;
}

// everything rwkv_mi_batch_serve_ex checks for one request, the session's limits and its features; nothing changed
static bool session_check_request(rwkv_mi_serve_session * S, const rwkv_mi_serve_request & rq, const uint32_t * prompt, const uint32_t * seq_lens,
                                  const uint32_t * seq_tokens, const rwkv_mi_serve_extra * ex) {
    rwkv_mi_batch * B = S->B;
    rwkv_context * ctx = B->ctx;
    const rwkv_mi_serve_limits & lim = S->lim;
    const size_t n_vocab = (size_t) ctx->model->n_vocab();
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, rq.prompt_len > 0, "the prompt of the request is empty");
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, rq.prompt_len <= lim.max_prompt, "prompt_len (%" PRIu32 ") is above the session's max_prompt (%" PRIu32 ")", rq.prompt_len, lim.max_prompt);
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, rq.from_slot == RWKV_MI_NO_SLOT || (rq.from_slot < B->n_slots && !S->is_lane[rq.from_slot]),
                 "from_slot of the request (%" PRIu32 ") is a lane of the session or out of range", rq.from_slot);
    for (uint32_t t = 0; t < rq.prompt_len; t++)
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, prompt[t] < n_vocab, "Prompt token at index %" PRIu32 " (%" PRIu32 ") is out of range (0 .. %zu)", t, prompt[t], n_vocab - 1);
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, rq.min_p >= 0.0f && rq.min_p <= 1.0f, "min_p of the request (%g) must be in 0 .. 1", (double) rq.min_p);
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, rq.decay >= 0.0f && rq.decay <= 1.0f, "decay of the request (%g) must be in 0 .. 1", (double) rq.decay);
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, rq.repetition > 0.0f && rq.repetition < INFINITY, "repetition of the request (%g) must be finite and above 0", (double) rq.repetition);
    bool guided = false;
    if (ex) {
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, ex->reserved == 0, "reserved of the extra of the request is not 0");
        if (ex->guide != RWKV_MI_NO_GUIDE) {
            RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, ex->guide < RWKV_MI_GUIDE_MAX && B->guide_states[ex->guide], "guide of the request (%" PRIu32 ") names no guide", ex->guide);
            RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, ex->guide_state < B->guide_states[ex->guide], "guide_state of the request (%" PRIu32 ") is out of range", ex->guide_state);
            RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, S->draw != Draw::none, "the request has a guide in the greedy family (guided greedy is temperature 0 of the sampled one)");
            guided = true;
        }
        if (ex->bias_slot != RWKV_MI_NO_SLOT) {
            RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, ex->bias_slot < B->n_slots && !S->is_lane[ex->bias_slot] && B->draw.has_bias[ex->bias_slot],
                         "bias_slot of the request (%" PRIu32 ") is a lane of the session, out of range or has no bias set", ex->bias_slot);
            RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, S->draw == Draw::penalized, "the request has a bias_slot in a family that reads no bias (the penalised one does)");
        }
    }
    if (S->draw != Draw::none && !batch_check_params(B, &rq.sample, 1, false)) return false;
    if (S->draw == Draw::penalized && !batch_check_penalties(B, &rq.penalty, 1)) return false;
    uint32_t lens_dummy = 0;
    if (!batch_check_stops(B, &rq.stop, 1, seq_lens, seq_tokens, lim.stride, &lens_dummy)) return false;
    size_t n_toks = 0;
    for (uint32_t q = 0; q < rq.stop.n_seqs; q++) n_toks += seq_lens[q];
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, rq.stop.n_seqs <= lim.max_seqs && n_toks <= lim.max_seq_tokens,
                 "the request's %" PRIu32 " stop sequences of %zu tokens are above the session's limits (%" PRIu32 ", %" PRIu32 ")", rq.stop.n_seqs, n_toks, lim.max_seqs, lim.max_seq_tokens);
    // what the request needs of the draw kernel, as batch_serve derives it from its queue
    const bool cut = S->draw != Draw::none && ((rq.top_k != 0u && rq.top_k < n_vocab) || rq.min_p != 0.0f);
    const bool rep = S->draw == Draw::penalized && (rq.decay != 1.0f || rq.repetition != 1.0f);
    // (against the session's kernel, which the features fixed: RWKV_MI_SERVE_GUIDED and _REP bring the truncating form with them)
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, (!cut || S->form.cut) && (!rep || S->form.rep) && (!guided || S->form.guided), "the request needs a feature the session did not declare (cut %d, rep %d, guided %d; features 0x%" PRIx32 ")",
                 (int) cut, (int) rep, (int) guided, lim.features);
    return true;
}

// the session's lanes, checked by batch_check_serve's rules
static bool session_check_lanes(rwkv_mi_batch * B, const uint32_t * lanes, size_t n, std::vector<uint8_t> * is_lane) {
    rwkv_context * ctx = B->ctx;
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, lanes != nullptr, "lanes is NULL");
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, n > 0 && n <= B->n_slots, "n (%zu) must be in 1 .. %zu", n, B->n_slots);
    is_lane->assign(B->n_slots, 0);
    for (size_t i = 0; i < n; i++) {
        const uint32_t s = lanes[i];
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, s < B->n_slots, "lane slot %" PRIu32 " at index %zu is out of range (0 .. %zu)", s, i, B->n_slots - 1);
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, !(*is_lane)[s], "lane slot %" PRIu32 " appears twice", s);
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, B->draw.guide_of[s] == RWKV_MI_NO_GUIDE && !B->draw.has_bias[s], "lane slot %" PRIu32 " has a guide attached or a bias set", s);
        (*is_lane)[s] = 1;
    }
    return true;
}

static rwkv_mi_serve_session * session_open(rwkv_mi_batch * B, const uint32_t * lanes, size_t n, int family, const rwkv_mi_serve_limits * lim) {
    rwkv_context * ctx = B->ctx;
    rwkv_context * run = B->run;
    ctx->last_error = RWKV_ERROR_NONE;
    RW_NO_PIPELINE(ctx, nullptr);
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, nullptr, family == RWKV_MI_SERVE_GREEDY || family == RWKV_MI_SERVE_SAMPLE || family == RWKV_MI_SERVE_PENALIZED,
                 "unknown family (%d)", family);
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, nullptr, B->session == nullptr, "a serve session is already open on this batch");
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, nullptr, !B->lp.enabled, "a serve session takes no batch with the log-prob report on");
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, nullptr, lim != nullptr, "limits is NULL");
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, nullptr, lim->reserved == 0, "reserved of the limits is not 0");
    const uint32_t known = RWKV_MI_SERVE_CUT | RWKV_MI_SERVE_REP | RWKV_MI_SERVE_GUIDED;
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, nullptr, (lim->features & ~known) == 0, "unknown bits in features (0x%" PRIx32 ")", lim->features);
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, nullptr, lim->capacity >= 1 && lim->max_prompt >= 1 && lim->stride >= 1, "capacity, max_prompt and stride must be at least 1");
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, nullptr, lim->max_seqs <= RWKV_MI_STOP_MAX_SEQS && lim->max_seq_tokens <= RWKV_MI_STOP_MAX_SEQS * RWKV_MI_STOP_MAX_LEN,
                 "max_seqs (%" PRIu32 ") or max_seq_tokens (%" PRIu32 ") is above what a request may carry (%d, %d)", lim->max_seqs, lim->max_seq_tokens, RWKV_MI_STOP_MAX_SEQS,
                 RWKV_MI_STOP_MAX_SEQS * RWKV_MI_STOP_MAX_LEN);
    const Draw draw = family == RWKV_MI_SERVE_PENALIZED ? Draw::penalized : family == RWKV_MI_SERVE_SAMPLE ? Draw::sample : Draw::none;
    const bool guided = (lim->features & RWKV_MI_SERVE_GUIDED) != 0;
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, nullptr, !guided || draw != Draw::none, "RWKV_MI_SERVE_GUIDED in the greedy family (guided greedy is temperature 0 of the sampled one)");
    std::unique_ptr<rwkv_mi_serve_session> S(new (std::nothrow) rwkv_mi_serve_session());
    RW_CTX_CHECK(ctx, RWKV_ERROR_ALLOC, nullptr, S != nullptr, "out of memory");
    if (!session_check_lanes(B, lanes, n, &S->is_lane)) return nullptr;
    const SessionLayout L(n, lim->capacity, lim->max_prompt, lim->max_seqs, lim->max_seq_tokens, lim->stride, guided);
    // (a ring entry's words are addressed by 32-bit word offsets)
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, nullptr, (uint64_t) lim->capacity * lim->stride < (1ull << 28) && L.bytes < (1ull << 31), "the session's tables are too large (%zu bytes)", L.bytes);
    run->print_errors = ctx->print_errors;
    if (hipSetDevice(ctx->model->device) != hipSuccess) { RW_CTX_CHECK(ctx, RWKV_ERROR_GRAPH, nullptr, false, "hipSetDevice failed"); }
    BatchCall lane_call{lanes, nullptr, n};
    lane_call.draw = draw;
    if (!batch_ensure_draw(B, lane_call) || !batch_ensure_serve(B, 0)) return nullptr;   // (the family's draw buffers; the fresh state)
    S->B = B; S->lanes.assign(lanes, lanes + n); S->draw = draw; S->lim = *lim; S->L = L;
    S->form = DrawForm::of(draw, (lim->features & RWKV_MI_SERVE_CUT) != 0, guided, (lim->features & RWKV_MI_SERVE_REP) != 0);
    B->form = S->form;
    hipError_t e = grow(want(S->words, L.bytes), want(S->down, 2 * (L.bytes - L.down)));
    for (hipEvent_t & v : S->ev) if (e == hipSuccess) e = hipEventCreateWithFlags(&v, hipEventDisableTiming);
    if (e != hipSuccess) (void) hipGetLastError();
    RW_CTX_CHECK(ctx, RWKV_ERROR_ALLOC, nullptr, e == hipSuccess, "cannot allocate the session's tables (%zu bytes): %s", L.bytes, hipGetErrorString(e));
    S->book.init(lim->capacity, n, lim->stride, loop_block());
    // the start values: every lane idle on {in = its slot's current buffer, out = the other one} in BOTH row tables -- an idle lane's dead
    // passes leave the slot's state alone --, a valid token word per lane, no entry admitted, an empty queue
    hipStream_t st = run->stream;
    if (hipStreamSynchronize(st) != hipSuccess) { RW_CTX_CHECK(ctx, RWKV_ERROR_GRAPH, nullptr, false, "HIP error at the session's start"); }
    const Staged & w = S->words;
    memset(w.pin.p, 0, L.bytes);
    for (size_t r = 0; r < n; r++) { w.h(L.lane_slot)[r] = lanes[r]; w.h(L.req)[r] = SESSION_IDLE; w.h(L.last)[r] = RWKV_MI_NO_TOKEN; }
    for (size_t i = 0; i < L.capacity; i++) { w.h(L.ids)[i] = RWKV_MI_NO_TOKEN; w.h(L.reasons)[i] = RWKV_MI_NO_TOKEN; }
    for (int tb = 0; tb < 2; tb++)
        for (size_t r = 0; r < n; r++) {
            const int p = B->parity[lanes[r]];
            B->rows.h()[(size_t) tb * B->n_slots + r] = RowState{B->slot_buf(lanes[r], p), B->slot_buf(lanes[r], p ^ 1)};
        }
    e = w.upload(0, L.bytes, st);
    if (e == hipSuccess) e = hipMemsetAsync(run->d_tokens.p, 0, n * sizeof(uint32_t), st);
    for (int tb = 0; tb < 2 && e == hipSuccess; tb++) e = B->rows.upload_rows((size_t) tb * B->n_slots, (size_t) tb * B->n_slots + n, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    RW_CTX_CHECK(ctx, RWKV_ERROR_GRAPH, nullptr, e == hipSuccess, "HIP error: %s", hipGetErrorString(e));
    RowSession & d = S->dev;
    uint32_t * ring = w.d(L.ring);
    d.s.t = ServeTables{w.d(L.reqs), ring, ring, ring, w.d(L.out), lim->stride,
                        w.d(L.lens), w.d(L.reasons), w.d(L.lane), w.d(L.start), w.d(L.req), w.d(L.pos), w.d(L.draw), w.d(L.admit), w.d(L.last), w.d(L.lane_slot),
                        draw != Draw::none ? B->draw_rows.d() : nullptr, B->draw.counters.p, B->draw.counts.p, w.d(L.next), w.d(L.work),
                        0u, (uint32_t) ctx->model->n_vocab(),
                        guided ? w.d(L.g_state) : nullptr, guided ? w.d(L.g_misses) : nullptr, guided ? w.d(L.req_g_state) : nullptr, guided ? w.d(L.req_g_misses) : nullptr};
    d.s.capacity = lim->capacity; d.s.tail = 0u; d.s.cancel = w.d(L.cancel_half(0));
    d.s.ids = w.d(L.ids); d.s.done = w.d(L.done); d.s.end_pass = w.d(L.end); d.s.revived = w.d(L.revived);
    d.s.entry_words = (uint32_t) L.entry_words; d.s.guide_word = (uint32_t) L.w_guide; d.s.admit_only = 0u;
    d.state_len = B->state_len; d.chunks = serve_chunks(B->state_len);
    B->session = S.get();
    return S.release();
}

// the request's ring entry into the staging: the row batch_serve builds, its words behind it
static void session_stage(rwkv_mi_serve_session * S, uint32_t id, const rwkv_mi_serve_request & rq, const uint32_t * prompt, const uint32_t * seq_lens,
                          const uint32_t * seq_tokens, const rwkv_mi_serve_extra * extra) {
    rwkv_mi_batch * B = S->B;
    const SessionLayout & L = S->L;
    const size_t e = L.entry_of(id);
    const bool pen = S->draw == Draw::penalized;
    uint32_t * ew = S->words.h(L.ring) + L.word(e, 0);
    DrawRow row{};
    row.p = rq.sample; row.p.u = -1.0f;
    row.presence = pen ? rq.penalty.presence : 0.0f; row.frequency = pen ? rq.penalty.frequency : 0.0f; row.record = pen ? 1u : 0u;
    row.top_k = rq.top_k; row.min_p = rq.min_p; row.decay = rq.decay; row.repetition = rq.repetition;
    const rwkv_mi_serve_extra ex = extra ? *extra : rwkv_mi_serve_extra{RWKV_MI_NO_GUIDE, 0u, RWKV_MI_NO_SLOT, 0u};
    if (ex.guide != RWKV_MI_NO_GUIDE) row.next = B->guides[ex.guide].p;
    if (pen && ex.bias_slot != RWKV_MI_NO_SLOT) row.bias = B->draw.bias_of(ex.bias_slot);
    const float * start = rq.from_slot == RWKV_MI_NO_SLOT ? B->serve_fresh.p : B->slot_buf(rq.from_slot, B->parity[rq.from_slot]);
    const StopRow stop{rq.stop.max_tokens, rq.stop.n_seqs, (uint32_t) L.word(e, L.w_seq_lens), (uint32_t) L.word(e, L.w_seq_tokens)};
    S->words.h(L.reqs)[e] = ServeReq{row, stop, rq.prompt_len, (uint32_t) L.word(e, L.w_prompt), start};
    memcpy(ew + L.w_prompt, prompt, (size_t) rq.prompt_len * sizeof(uint32_t));
    size_t n_toks = 0;
    for (uint32_t q = 0; q < rq.stop.n_seqs; q++) { ew[L.w_seq_lens + q] = seq_lens[q]; n_toks += seq_lens[q]; }
    if (n_toks) memcpy(ew + L.w_seq_tokens, seq_tokens, n_toks * sizeof(uint32_t));
    ew[L.w_guide] = ex.guide != RWKV_MI_NO_GUIDE ? ex.guide_state : 0u;
}

// Cancels what is in flight, drains, sets the lanes' parities and frees the session. Every request still in flight retires within one block of
// its cancel word (a queued one after one pass on a lane), so the number of blocks is bounded; a session that is still busy after them has failed.
static bool session_close(rwkv_mi_serve_session * S, uint32_t * last_request_out) {
    rwkv_mi_batch * B = S->B;
    std::unique_ptr<rwkv_mi_serve_session> owner(S);
    SessionBook & book = S->book;
    B->ctx->last_error = RWKV_ERROR_NONE;
    B->run->print_errors = B->ctx->print_errors;
    (void) hipSetDevice(B->ctx->model->device);
    bool ok = !S->failed;
    for (uint32_t id = book.oldest; id != book.submitted; id++) (void) book.cancel_request(id);
    std::vector<rwkv_mi_serve_event> ev(book.capacity);
    std::vector<uint32_t> toks(book.capacity * book.stride);
    size_t ne = 0, nt = 0;
    if (ok) ok = session_consume(S, book.enqueued);   // (what is still unread first: the blocks below are enqueued on what the device has really done)
    for (size_t blocks = 0; ok && book.busy() && blocks < book.capacity + 4; blocks++) {
        ok = session_enqueue(S) && session_consume(S, book.enqueued);
        if (ok) book.deliver(ev.data(), ev.size(), toks.data(), toks.size(), &ne, &nt);
    }
    if (ok) book.deliver(ev.data(), ev.size(), toks.data(), toks.size(), &ne, &nt);
    (void) hipStreamSynchronize(B->run->stream);   // (whatever happened: nothing of the session's is read after this)
    B->session = nullptr;
    if (ok && (book.busy() || book.in_flight != 0)) {
        ok = false;
        ctx_fail(B->ctx, RWKV_ERROR_GRAPH, __FILE__, __LINE__, "session drained", "the session did not drain (%" PRIu32 " requests in flight): the device loop failed", book.in_flight);
    }
    for (size_t r = 0; r < S->lanes.size(); r++) {
        if (ok && book.parity_flip(r)) B->parity[S->lanes[r]] ^= 1;
        if (last_request_out) last_request_out[r] = book.lane_last[r];
    }
    return ok;
}

// ---- beam search (rwkv_mi_batch_decode_beam) ----

// a call of G groups of W hypotheses: row g * W + j is slot slots[g * W + j]
struct BeamCall {
    const uint32_t * slots, * first_tokens;
    size_t G;
    const rwkv_mi_beam_params * p;
    size_t n_tokens;
};

// every argument of a beam call, nothing changed yet
static bool batch_check_beam(rwkv_mi_batch * B, const BeamCall & c) {
    rwkv_context * ctx = B->ctx;
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, c.slots != nullptr && c.first_tokens != nullptr && c.p != nullptr, "slots, first_tokens or params is NULL");
    const size_t n_vocab = (size_t) ctx->model->n_vocab(), W = c.p->width;
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, W >= 1 && W <= RWKV_MI_TOP_MAX && W <= n_vocab, "width (%zu) must be in 1 .. %d and at most n_vocab", W, RWKV_MI_TOP_MAX);
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, c.G >= 1 && c.G <= B->n_slots && c.G * W <= B->n_slots, "n_groups (%zu) x width (%zu) must be in 1 .. %zu rows", c.G, W, B->n_slots);
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, c.n_tokens > 0, "n_tokens is 0");
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, c.p->n_end <= 8 && (c.p->n_end == 0 || c.p->end_tokens != nullptr), "n_end (%" PRIu32 ") is above 8 or end_tokens is NULL", c.p->n_end);
    for (uint32_t e = 0; e < c.p->n_end; e++)
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, c.p->end_tokens[e] < n_vocab, "end token at index %" PRIu32 " (%" PRIu32 ") is out of range (0 .. %zu)", e, c.p->end_tokens[e], n_vocab - 1);
    std::vector<uint8_t> seen(B->n_slots, 0);
    for (size_t r = 0; r < c.G * W; r++) {
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, c.slots[r] < B->n_slots, "slot %" PRIu32 " at index %zu is out of range (0 .. %zu)", c.slots[r], r, B->n_slots - 1);
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, !seen[c.slots[r]], "slot %" PRIu32 " appears twice", c.slots[r]);
        seen[c.slots[r]] = 1;
    }
    for (size_t g = 0; g < c.G; g++)
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, c.first_tokens[g] < n_vocab, "Token at index %zu (%" PRIu32 ") is out of range (0 .. %zu)", g, c.first_tokens[g], n_vocab - 1);
    return batch_check_unguided(B, c.slots, c.G * W, "beam search");
}

// the poll words of the batch and the beam words: on the first beam call, for n_slots rows
static bool batch_ensure_beam(rwkv_mi_batch * B) {
    const BeamLayout L(B->n_slots);
    hipError_t e = B->poll.ensure();
    if (e == hipSuccess && !B->beam) e = grow(want(B->beam, L.bytes));
    RW_CTX_CHECK(B->ctx, RWKV_ERROR_ALLOC, false, e == hipSuccess, "cannot allocate the beam tables of %zu slots: %s", B->n_slots, hipGetErrorString(e));
    return true;
}

// The device loop of a beam search: the driver's passes, polled on the unfinished hypotheses, each pass followed by the two kernels of a step (engine.hip launch_row_sampler,
// score.hip k_beam_rows / k_beam_select). A step RE-PARENTS instead of copying: the selection writes, into the row table of the next pass, for
// every row the buffer its parent has just written as .in; .out stays the row's own slot's other buffer. Every read of a pass is of a buffer
// the pass before wrote (the first: the group's start buffer), every write goes to the other buffer of a named slot -- no pass writes what it
// or a later row of it reads, and any number of children share a parent. The only states that move are those of the last selection: a
// hypothesis that ends in another slot's buffer is copied home, device to device, into its slot's idle buffer.
static bool batch_beam(rwkv_mi_batch * B, const BeamCall & c, uint32_t * tokens_out, uint32_t * lens_out, double * scores_out, float * logprobs_out, float * elapsed_ms) {
    rwkv_context * ctx = B->ctx;
    rwkv_context * run = B->run;
    if (!batch_begin(B) || !batch_check_beam(B, c)) return false;
    const size_t W = c.p->width, n = c.G * W, n_tokens = c.n_tokens;
    if (!batch_ensure_beam(B)) return false;
    DevBuf<uint32_t> hist;   // token, parent, log-prob: [3][n_tokens][n], freed on every exit
    hipError_t he = hist.alloc(3 * n_tokens * n);
    if (he != hipSuccess) (void) hipGetLastError();
    RW_CTX_CHECK(ctx, RWKV_ERROR_ALLOC, false, he == hipSuccess, "cannot allocate the history of %zu steps of %zu rows: %s", n_tokens, n, hipGetErrorString(he));
    BATCH_HIP_OK(B, hipStreamSynchronize(run->stream));   // (the previous call's copies may still read the staging)
    // table 0: every row of a group from the group's start buffer into its own slot's other buffer; table 1: .out back into the current one
    // (its .in is written by the first selection)
    const BeamLayout L(n);
    const Staged & w = B->beam;
    double * h_score = w.h(L.score);
    uint32_t * h_fin = w.h(L.finished), * h_len = w.h(L.lens);
    for (size_t r = 0; r < n; r++) {
        const size_t s0 = c.slots[r - r % W], s = c.slots[r];
        float * cur = B->slot_buf(s, B->parity[s]), * oth = B->slot_buf(s, B->parity[s] ^ 1);
        B->rows.h()[r] = RowState{B->slot_buf(s0, B->parity[s0]), oth};
        B->rows.h()[B->n_slots + r] = RowState{oth, cur};
        run->h_tokens.p[r] = c.first_tokens[r / W];
        h_score[r] = r % W ? -INFINITY : 0.0;
        h_fin[r] = 0u; h_len[r] = 0u;
    }
    *w.h(L.count) = (uint32_t) n;
    if (!batch_upload_rows(B, n, 2)) return false;
    BATCH_HIP_OK(B, hipMemcpyAsync(run->d_tokens.p, run->h_tokens.p, n * sizeof(uint32_t), hipMemcpyHostToDevice, run->stream));
    BATCH_HIP_OK(B, w.upload(0, L.upload, run->stream));
    BeamTables t{w.d(L.score), w.d(L.finished), w.d(L.lens), w.d(L.ids), w.d(L.lp), w.d(L.chosen),
                 hist.p, hist.p + n_tokens * n, (float *) (hist.p + 2 * n_tokens * n), w.d(L.count), (uint32_t) W, c.p->n_end, {}};
    for (uint32_t e = 0; e < c.p->n_end; e++) t.end_tokens[e] = c.p->end_tokens[e];
    RowSampler sampler;
    sampler.beam = &t;
    if (!batch_run_passes(B, n_tokens, t.live_count, sampler, [&](const RowSampler & s) { return forward_rows(run, s.used, (int64_t) n, true, &s); })) return false;
    const size_t passes = B->last_loop_passes;
    std::vector<uint32_t> h(3 * passes * n);
    for (size_t a = 0; a < 3; a++)
        BATCH_HIP_OK(B, hipMemcpyAsync(h.data() + a * passes * n, hist.p + a * n_tokens * n, passes * n * sizeof(uint32_t), hipMemcpyDeviceToHost, run->stream));
    BATCH_HIP_OK(B, w.fetch(0, L.count.off, run->stream));
    if (!batch_passes_done(B, elapsed_ms)) return false;
    const uint32_t * h_tok = h.data(), * h_par = h.data() + passes * n;
    const float * h_lp = (const float *) (h.data() + 2 * passes * n);
    // the backtrace: hypothesis j of the last selection, then its parent's of the step before, ...; a step without a token (the hypothesis
    // had finished) adds nothing. A dead hypothesis (score -inf) has no text.
    std::vector<uint32_t> text(passes);
    std::vector<float> text_lp(passes);
    for (size_t r = 0; r < n; r++) {
        size_t len = 0, at = r;
        for (size_t i = passes; i-- > 0 && h_score[r] > -INFINITY;) {
            const size_t w = i * n + at;
            RW_CTX_CHECK(ctx, RWKV_ERROR_GRAPH, false, h_par[w] < W, "the history of row %zu is broken at step %zu (the device loop failed)", r, i);
            if (h_tok[w] != RWKV_MI_NO_TOKEN) { text[len] = h_tok[w]; text_lp[len] = h_lp[w]; len++; }
            at = r - r % W + h_par[w];
        }
        RW_CTX_CHECK(ctx, RWKV_ERROR_GRAPH, false, len == h_len[r], "row %zu has %zu tokens in the history and a length of %" PRIu32 " (the device loop failed)", r, len, h_len[r]);
        if (lens_out) lens_out[r] = (uint32_t) len;
        if (scores_out) scores_out[r] = h_score[r];
        for (size_t j = 0; j < n_tokens; j++) {
            if (tokens_out) tokens_out[r * n_tokens + j] = j < len ? text[len - 1 - j] : RWKV_MI_NO_TOKEN;
            if (logprobs_out) logprobs_out[r * n_tokens + j] = j < len ? text_lp[len - 1 - j] : 0.0f;
        }
    }
    // where the states are: the last pass wrote row x's into slot x's buffer parity ^ (passes & 1). An unfinished hypothesis whose last parent
    // is another row is copied from that row's buffer into its own slot's other one, which no copy reads; the parities follow
    const int odd = (int) (passes & 1);
    std::vector<uint8_t> parity(n);
    for (size_t r = 0; r < n; r++) {
        const size_t s = c.slots[r], rp = r - r % W + h_par[(passes - 1) * n + r];
        parity[r] = B->parity[s] ^ odd;
        if (h_fin[r] || rp == r) continue;   // (an unfinished row's parent has been checked by its backtrace)
        const size_t sp = c.slots[rp];
        parity[r] ^= 1;
        BATCH_HIP_OK(B, hipMemcpyAsync(B->slot_buf(s, parity[r]), B->slot_buf(sp, B->parity[sp] ^ odd), (size_t) B->state_len * sizeof(float), hipMemcpyDeviceToDevice, run->stream));
    }
    for (size_t r = 0; r < n; r++) B->parity[c.slots[r]] = parity[r];
    BATCH_HIP_OK(B, hipStreamSynchronize(run->stream));
    return true;
}

extern "C" {

RWKV_API void rwkv_mi_batch_free(struct rwkv_mi_batch * B) {
    if (!B) return;
    if (B->session) (void) session_close(B->session, nullptr);
    if (B->run) {
        (void) hipSetDevice(B->run->model->device);
        (void) hipStreamSynchronize(B->run->stream);
    }
    rwkv_context * run = B->run;
    delete B;   // its buffers and block events: after the drain above, before the batch's own context gives up its stream and its reference to the model
    batch_context_destroy(run);
}

RWKV_API struct rwkv_mi_batch * rwkv_mi_batch_create(struct rwkv_context * ctx, size_t n_slots) {
    RW_CHECK(RWKV_ERROR_ARGS, nullptr, ctx != nullptr, "ctx is NULL");
    ctx->last_error = RWKV_ERROR_NONE;
    RW_NO_PIPELINE(ctx, nullptr);
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, nullptr, n_slots > 0 && n_slots <= ((size_t) 1 << 20), "n_slots (%zu) out of range", n_slots);
    Model & m = *ctx->model;
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS | RWKV_ERROR_UNSUPPORTED, nullptr, m.has_embed && m.has_head, "a batch needs a whole model (embedding and head)");
    std::unique_ptr<rwkv_mi_batch, void (*)(rwkv_mi_batch *)> B(new (std::nothrow) rwkv_mi_batch(), rwkv_mi_batch_free);
    RW_CTX_CHECK(ctx, RWKV_ERROR_ALLOC, nullptr, B != nullptr, "out of memory");
    B->ctx = ctx;
    B->n_slots = n_slots;
    B->state_len = m.state_len();
    B->parity.assign(n_slots, 0);
    B->draw.init(n_slots, (size_t) m.n_vocab());
    RW_CTX_CHECK(ctx, RWKV_ERROR_GRAPH, nullptr, hipSetDevice(m.device) == hipSuccess, "hipSetDevice failed");
    B->run = batch_context_create(&m, (int64_t) n_slots);
    RW_CTX_CHECK(ctx, RWKV_ERROR_CTX | RWKV_ERROR_ALLOC, nullptr, B->run != nullptr, "cannot create the batch's stream / buffers (device memory?)");
    B->run->print_errors = ctx->print_errors;
    const size_t sbytes = (size_t) B->state_len * sizeof(float);
    hipError_t e = B->states.alloc(2 * n_slots * (size_t) B->state_len);
    RW_CTX_CHECK(ctx, RWKV_ERROR_ALLOC, nullptr, e == hipSuccess, "cannot allocate %zu slot states: %s", n_slots, hipGetErrorString(e));
    e = B->rows.alloc(2 * n_slots);
    RW_CTX_CHECK(ctx, RWKV_ERROR_ALLOC, nullptr, e == hipSuccess, "HIP error: %s", hipGetErrorString(e));
    if (!B->draw.ensure_counters(ctx, B->run->stream)) return nullptr;
    // every slot starts from the fresh state (both buffers: a slot's first pass reads buffer 0)
    for (size_t s = 0; s < n_slots; s++) {
        float * dst = B->slot_buf(s, 0);
        if (m.arch_major >= 5) e = hipMemsetAsync(dst, 0, sbytes, B->run->stream);
        else { launch_fill_state_v4(dst, m.n_layer(), m.n_embed(), B->run->stream); e = hipGetLastError(); }
        if (e != hipSuccess) break;
    }
    if (e == hipSuccess) e = hipStreamSynchronize(B->run->stream);
    RW_CTX_CHECK(ctx, RWKV_ERROR_GRAPH, nullptr, e == hipSuccess, "HIP error: %s", hipGetErrorString(e));
    return B.release();
}

RWKV_API bool rwkv_mi_batch_state_load(struct rwkv_mi_batch * B, size_t slot, const float * state_in) {
    rwkv_context * ctx = B->ctx;
    ctx->last_error = RWKV_ERROR_NONE;
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, slot < B->n_slots, "slot %zu is out of range", slot);
    const Model & m = *ctx->model;
    BATCH_HIP_OK(B, hipSetDevice(m.device));
    hipStream_t st = B->run->stream;
    BATCH_HIP_OK(B, hipStreamSynchronize(st));
    float * dst = B->slot_buf(slot, B->parity[slot]);
    const size_t sbytes = (size_t) B->state_len * sizeof(float);
    if (state_in) BATCH_HIP_OK(B, hipMemcpyAsync(dst, state_in, sbytes, hipMemcpyHostToDevice, st));
    else if (m.arch_major >= 5) BATCH_HIP_OK(B, hipMemsetAsync(dst, 0, sbytes, st));
    else { launch_fill_state_v4(dst, m.n_layer(), m.n_embed(), st); BATCH_HIP_OK(B, hipGetLastError()); }
    BATCH_HIP_OK(B, hipStreamSynchronize(st));
    return true;
}

RWKV_API bool rwkv_mi_batch_state_store(struct rwkv_mi_batch * B, size_t slot, float * state_out) {
    rwkv_context * ctx = B->ctx;
    ctx->last_error = RWKV_ERROR_NONE;
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, slot < B->n_slots && state_out != nullptr, "slot %zu is out of range or state_out is NULL", slot);
    BATCH_HIP_OK(B, hipSetDevice(ctx->model->device));
    hipStream_t st = B->run->stream;
    BATCH_HIP_OK(B, hipMemcpyAsync(state_out, B->slot_buf(slot, B->parity[slot]), (size_t) B->state_len * sizeof(float), hipMemcpyDeviceToHost, st));
    BATCH_HIP_OK(B, hipStreamSynchronize(st));
    return true;
}

// a context whose resident state can be exchanged with the batch's slots: one device, same device, same state size
static bool batch_peer_ok(rwkv_mi_batch * B, size_t slot, rwkv_context * other) {
    rwkv_context * ctx = B->ctx;
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, slot < B->n_slots && other != nullptr, "slot %zu is out of range or the context is NULL", slot);
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS | RWKV_ERROR_UNSUPPORTED, false, other->stages.empty(), "a RWKV_MI_DEVICES chain cannot exchange state with a batch");
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, other->model->device == ctx->model->device && other->model->state_len() == B->state_len,
                 "the context is on another device or has another state size");
    return true;
}

RWKV_API bool rwkv_mi_batch_state_from_context(struct rwkv_mi_batch * B, size_t slot, struct rwkv_context * other) {
    B->ctx->last_error = RWKV_ERROR_NONE;
    if (!batch_peer_ok(B, slot, other)) return false;
    BATCH_HIP_OK(B, hipSetDevice(other->model->device));
    BATCH_HIP_OK(B, hipStreamSynchronize(other->stream));     // (the context's last step has written its state)
    hipStream_t st = B->run->stream;
    BATCH_HIP_OK(B, hipMemcpyAsync(B->slot_buf(slot, B->parity[slot]), other->state[other->cur].p, (size_t) B->state_len * sizeof(float), hipMemcpyDeviceToDevice, st));
    BATCH_HIP_OK(B, hipStreamSynchronize(st));
    return true;
}

RWKV_API bool rwkv_mi_batch_state_to_context(struct rwkv_mi_batch * B, size_t slot, struct rwkv_context * other) {
    B->ctx->last_error = RWKV_ERROR_NONE;
    if (!batch_peer_ok(B, slot, other)) return false;
    BATCH_HIP_OK(B, hipSetDevice(other->model->device));
    hipStream_t st = B->run->stream;
    BATCH_HIP_OK(B, hipStreamSynchronize(st));
    BATCH_HIP_OK(B, hipMemcpyAsync(other->state[other->cur].p, B->slot_buf(slot, B->parity[slot]), (size_t) B->state_len * sizeof(float), hipMemcpyDeviceToDevice, other->stream));
    BATCH_HIP_OK(B, hipStreamSynchronize(other->stream));
    return true;
}

RWKV_API bool rwkv_mi_batch_eval(struct rwkv_mi_batch * B, const uint32_t * slots, const uint32_t * tokens, size_t n, float * logits_out) {
    BatchCall c{slots, tokens, n};
    c.logits_out = logits_out;
    return batch_pass(B, c);
}

RWKV_API bool rwkv_mi_batch_decode_greedy(struct rwkv_mi_batch * B, const uint32_t * slots, const uint32_t * first_tokens, size_t n,
                                          size_t n_tokens, uint32_t * tokens_out, float * elapsed_ms) {
    return batch_loop(B, BatchCall{slots, first_tokens, n}, n_tokens, tokens_out, elapsed_ms);
}

RWKV_API bool rwkv_mi_batch_eval_sample(struct rwkv_mi_batch * B, const uint32_t * slots, const uint32_t * tokens, size_t n,
                                        const struct rwkv_mi_sample_params * params, uint32_t * sampled_out, float * logits_out) {
    BatchCall c{slots, tokens, n};
    c.draw = Draw::sample; c.params = params;
    c.sampled_out = sampled_out; c.logits_out = logits_out;
    return batch_pass(B, c);
}

RWKV_API bool rwkv_mi_batch_eval_ragged(struct rwkv_mi_batch * B, const uint32_t * slots, const uint32_t * lens, const uint32_t * tokens, size_t n,
                                        float * logits_out) {
    BatchCall c{slots, tokens, n, true, lens};
    c.logits_out = logits_out;
    return batch_pass(B, c);
}

RWKV_API bool rwkv_mi_batch_score_ragged(struct rwkv_mi_batch * B, const uint32_t * slots, const uint32_t * lens, const uint32_t * tokens, const uint32_t * targets,
                                         size_t n, float * logprobs_out, uint32_t * argmax_out) {
    BatchCall c{slots, tokens, n, true, lens};
    c.targets = targets; c.logprobs_out = logprobs_out; c.argmax_out = argmax_out;
    return batch_pass(B, c);
}

RWKV_API bool rwkv_mi_batch_eval_ragged_sample(struct rwkv_mi_batch * B, const uint32_t * slots, const uint32_t * lens, const uint32_t * tokens, size_t n,
                                               const struct rwkv_mi_sample_params * params, uint32_t * sampled_out, float * logits_out) {
    BatchCall c{slots, tokens, n, true, lens};
    c.draw = Draw::sample; c.params = params;
    c.sampled_out = sampled_out; c.logits_out = logits_out;
    return batch_pass(B, c);
}

RWKV_API bool rwkv_mi_batch_decode_sample(struct rwkv_mi_batch * B, const uint32_t * slots, const uint32_t * first_tokens, size_t n,
                                          size_t n_tokens, const struct rwkv_mi_sample_params * params, uint32_t * tokens_out, float * elapsed_ms) {
    BatchCall c{slots, first_tokens, n};
    c.draw = Draw::sample; c.params = params;
    return batch_loop(B, c, n_tokens, tokens_out, elapsed_ms);
}

RWKV_API bool rwkv_mi_batch_rng_seek(struct rwkv_mi_batch * B, size_t slot, uint64_t counter) {
    return batch_slot_call(B, slot) && on_device(B->ctx) && B->draw.seek(B->ctx, slot, counter, B->run->stream);
}

RWKV_API bool rwkv_mi_batch_truncation_set(struct rwkv_mi_batch * B, size_t slot, uint32_t top_k, float min_p) {
    return batch_slot_call(B, slot) && B->draw.cut_set(B->ctx, slot, top_k, min_p);
}

RWKV_API bool rwkv_mi_batch_truncation_get(struct rwkv_mi_batch * B, size_t slot, uint32_t * top_k_out, float * min_p_out) {
    if (!batch_slot_call(B, slot)) return false;
    if (top_k_out) *top_k_out = B->draw.cuts[slot].top_k;
    if (min_p_out) *min_p_out = B->draw.cuts[slot].min_p;
    return true;
}

RWKV_API bool rwkv_mi_batch_repetition_set(struct rwkv_mi_batch * B, size_t slot, float decay, float repetition) {
    return batch_slot_call(B, slot) && on_device(B->ctx) && B->draw.rep_set(B->ctx, slot, decay, repetition, B->run->stream);
}

RWKV_API bool rwkv_mi_batch_repetition_get(struct rwkv_mi_batch * B, size_t slot, float * decay_out, float * repetition_out) {
    if (!batch_slot_call(B, slot)) return false;
    if (decay_out) *decay_out = B->draw.reps[slot].decay;
    if (repetition_out) *repetition_out = B->draw.reps[slot].repetition;
    return true;
}

RWKV_API bool rwkv_mi_batch_counts_store_f32(struct rwkv_mi_batch * B, size_t slot, float * out) {
    if (!batch_slot_call(B, slot)) return false;
    RW_CTX_CHECK(B->ctx, RWKV_ERROR_ARGS, false, out != nullptr, "out is NULL");
    return on_device(B->ctx) && B->draw.counts_store_f32(B->ctx, slot, out, B->run->stream);
}

RWKV_API bool rwkv_mi_batch_counts_reset(struct rwkv_mi_batch * B, size_t slot) {
    return batch_slot_call(B, slot) && on_device(B->ctx) && B->draw.counts_reset(B->ctx, slot, B->run->stream);
}

RWKV_API bool rwkv_mi_batch_counts_add(struct rwkv_mi_batch * B, size_t slot, const uint32_t * tokens, size_t n) {
    return batch_slot_call(B, slot) && check_count_tokens(B->ctx, tokens, n) && on_device(B->ctx) && B->draw.counts_add(B->ctx, slot, tokens, n, B->run->stream);
}

RWKV_API bool rwkv_mi_batch_counts_store(struct rwkv_mi_batch * B, size_t slot, uint32_t * counts_out) {
    if (!batch_slot_call(B, slot)) return false;
    RW_CTX_CHECK(B->ctx, RWKV_ERROR_ARGS, false, counts_out != nullptr, "counts_out is NULL");
    return on_device(B->ctx) && B->draw.counts_store(B->ctx, slot, counts_out, B->run->stream);
}

RWKV_API bool rwkv_mi_batch_logit_bias_set(struct rwkv_mi_batch * B, size_t slot, const uint32_t * ids, const float * values, size_t n) {
    return batch_slot_call(B, slot) && check_bias(B->ctx, ids, values, n) && on_device(B->ctx) && B->draw.bias_set(B->ctx, slot, ids, values, n, B->run->stream);
}

RWKV_API bool rwkv_mi_batch_eval_sample_penalized(struct rwkv_mi_batch * B, const uint32_t * slots, const uint32_t * tokens, size_t n,
                                                  const struct rwkv_mi_sample_params * params, const struct rwkv_mi_penalty_params * penalties,
                                                  uint32_t * sampled_out, float * logits_out) {
    BatchCall c{slots, tokens, n};
    c.draw = Draw::penalized; c.params = params; c.penalties = penalties;
    c.sampled_out = sampled_out; c.logits_out = logits_out;
    return batch_pass(B, c);
}

RWKV_API bool rwkv_mi_batch_eval_ragged_sample_penalized(struct rwkv_mi_batch * B, const uint32_t * slots, const uint32_t * lens, const uint32_t * tokens,
                                                         size_t n, const struct rwkv_mi_sample_params * params,
                                                         const struct rwkv_mi_penalty_params * penalties, uint32_t * sampled_out, float * logits_out) {
    BatchCall c{slots, tokens, n, true, lens};
    c.draw = Draw::penalized; c.params = params; c.penalties = penalties;
    c.sampled_out = sampled_out; c.logits_out = logits_out;
    return batch_pass(B, c);
}

RWKV_API bool rwkv_mi_batch_decode_sample_penalized(struct rwkv_mi_batch * B, const uint32_t * slots, const uint32_t * first_tokens, size_t n,
                                                    size_t n_tokens, const struct rwkv_mi_sample_params * params,
                                                    const struct rwkv_mi_penalty_params * penalties, uint32_t * tokens_out, float * elapsed_ms) {
    BatchCall c{slots, first_tokens, n};
    c.draw = Draw::penalized; c.params = params; c.penalties = penalties;
    return batch_loop(B, c, n_tokens, tokens_out, elapsed_ms);
}

RWKV_API bool rwkv_mi_batch_decode_until(struct rwkv_mi_batch * B, const uint32_t * slots, const uint32_t * first_tokens, size_t n,
                                         const struct rwkv_mi_sample_params * params, const struct rwkv_mi_penalty_params * penalties,
                                         const struct rwkv_mi_stop_params * stops, const uint32_t * seq_lens, const uint32_t * seq_tokens,
                                         size_t stride, uint32_t * tokens_out, uint32_t * lens_out, uint32_t * stopped_by_out, float * elapsed_ms) {
    B->ctx->last_error = RWKV_ERROR_NONE;
    RW_CTX_CHECK(B->ctx, RWKV_ERROR_ARGS, false, params != nullptr || penalties == nullptr, "penalties are given without params");
    BatchCall c{slots, first_tokens, n};
    c.draw = penalties ? Draw::penalized : params ? Draw::sample : Draw::none;
    c.params = params; c.penalties = penalties;
    c.until = true; c.stops = stops; c.seq_lens = seq_lens; c.seq_tokens = seq_tokens;
    c.stride = stride; c.lens_out = lens_out; c.stopped_by_out = stopped_by_out;
    return batch_until(B, c, tokens_out, elapsed_ms);
}

RWKV_API size_t rwkv_mi_batch_last_loop_passes(const struct rwkv_mi_batch * B) { return B ? B->last_loop_passes : 0; }

// both entry points of the queue: the description they share -- `ex`: the call is rwkv_mi_batch_serve_ex, which takes what follows it -- and the body
static bool serve_entry(rwkv_mi_batch * B, const uint32_t * lanes, size_t n, int family, const rwkv_mi_serve_request * requests, size_t n_requests,
                        const uint32_t * prompt_tokens, const uint32_t * seq_lens, const uint32_t * seq_tokens, size_t stride, uint32_t * tokens_out, uint32_t * lens_out,
                        uint32_t * stopped_by_out, uint32_t * lane_out, uint32_t * start_pass_out, uint32_t * last_request_out, float * elapsed_ms, bool ex,
                        const rwkv_mi_serve_extra * extras, uint32_t * guide_state_out, uint32_t * guide_misses_out) {
    B->ctx->last_error = RWKV_ERROR_NONE;
    RW_NO_PIPELINE(B->ctx, false);
    RW_CTX_CHECK(B->ctx, RWKV_ERROR_ARGS, false, family == RWKV_MI_SERVE_GREEDY || family == RWKV_MI_SERVE_SAMPLE || family == RWKV_MI_SERVE_PENALIZED,
                 "unknown family (%d)", family);
    BatchCall c{lanes, nullptr, n};
    c.draw = family == RWKV_MI_SERVE_PENALIZED ? Draw::penalized : family == RWKV_MI_SERVE_SAMPLE ? Draw::sample : Draw::none;
    c.requests = requests; c.n_requests = n_requests; c.prompts = prompt_tokens;
    c.seq_lens = seq_lens; c.seq_tokens = seq_tokens;
    c.stride = stride; c.lens_out = lens_out; c.stopped_by_out = stopped_by_out;
    c.lane_out = lane_out; c.start_pass_out = start_pass_out; c.last_request_out = last_request_out;
    c.serve_ex = ex; c.extras = extras; c.guide_state_out = guide_state_out; c.guide_misses_out = guide_misses_out;
    return batch_serve(B, c, tokens_out, elapsed_ms);
}

RWKV_API bool rwkv_mi_batch_serve(struct rwkv_mi_batch * B, const uint32_t * lanes, size_t n, int family, const struct rwkv_mi_serve_request * requests,
                                  size_t n_requests, const uint32_t * prompt_tokens, const uint32_t * seq_lens, const uint32_t * seq_tokens, size_t stride,
                                  uint32_t * tokens_out, uint32_t * lens_out, uint32_t * stopped_by_out, uint32_t * lane_out, uint32_t * start_pass_out,
                                  uint32_t * last_request_out, float * elapsed_ms) {
    return serve_entry(B, lanes, n, family, requests, n_requests, prompt_tokens, seq_lens, seq_tokens, stride, tokens_out, lens_out, stopped_by_out, lane_out,
                       start_pass_out, last_request_out, elapsed_ms, false, nullptr, nullptr, nullptr);
}

RWKV_API bool rwkv_mi_batch_serve_ex(struct rwkv_mi_batch * B, const uint32_t * lanes, size_t n, int family, const struct rwkv_mi_serve_request * requests,
                                     size_t n_requests, const uint32_t * prompt_tokens, const uint32_t * seq_lens, const uint32_t * seq_tokens, size_t stride,
                                     uint32_t * tokens_out, uint32_t * lens_out, uint32_t * stopped_by_out, uint32_t * lane_out, uint32_t * start_pass_out,
                                     uint32_t * last_request_out, float * elapsed_ms, const struct rwkv_mi_serve_extra * extras, uint32_t * guide_state_out,
                                     uint32_t * guide_misses_out) {
    return serve_entry(B, lanes, n, family, requests, n_requests, prompt_tokens, seq_lens, seq_tokens, stride, tokens_out, lens_out, stopped_by_out, lane_out,
                       start_pass_out, last_request_out, elapsed_ms, true, extras, guide_state_out, guide_misses_out);
}

// ---- serve sessions (include/rwkv_mi355x.h) ----

RWKV_API struct rwkv_mi_serve_session * rwkv_mi_batch_serve_open(struct rwkv_mi_batch * B, const uint32_t * lanes, size_t n, int family,
                                                                 const struct rwkv_mi_serve_limits * limits) {
    return B ? session_open(B, lanes, n, family, limits) : nullptr;
}

RWKV_API bool rwkv_mi_batch_serve_submit(struct rwkv_mi_serve_session * S, const struct rwkv_mi_serve_request * request, const uint32_t * prompt_tokens,
                                         const uint32_t * seq_lens, const uint32_t * seq_tokens, const struct rwkv_mi_serve_extra * extra, uint32_t * id_out) {
    if (!S || !session_begin(S)) return false;
    rwkv_context * ctx = S->B->ctx;
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, request != nullptr && prompt_tokens != nullptr && id_out != nullptr, "request, prompt_tokens or id_out is NULL");
    if (!session_check_request(S, *request, prompt_tokens, seq_lens, seq_tokens, extra)) return false;
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, S->book.room() > 0 && S->book.submitted < SERVE_FREE - 1u,
                 "the request ring is full (%" PRIu32 " requests in flight, capacity %" PRIu32 "): poll until an end has been delivered", S->book.in_flight, S->lim.capacity);
    const uint32_t id = S->book.submit();
    session_stage(S, id, *request, prompt_tokens, seq_lens, seq_tokens, extra);
    *id_out = id;
    return true;
}

RWKV_API bool rwkv_mi_batch_serve_cancel(struct rwkv_mi_serve_session * S, uint32_t id) {
    if (!S) return false;
    S->B->ctx->last_error = RWKV_ERROR_NONE;
    return S->book.cancel_request(id);
}

RWKV_API bool rwkv_mi_batch_serve_poll(struct rwkv_mi_serve_session * S, uint32_t flags, struct rwkv_mi_serve_event * events_out, size_t max_events,
                                       uint32_t * tokens_out, size_t max_tokens, size_t * n_events, size_t * n_tokens) {
    if (!S || !session_begin(S)) return false;
    rwkv_context * ctx = S->B->ctx;
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, (flags & ~RWKV_MI_POLL_DRAIN) == 0, "unknown bits in flags (0x%" PRIx32 ")", flags);
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, n_events != nullptr && n_tokens != nullptr && (events_out != nullptr || max_events == 0) && (tokens_out != nullptr || max_tokens == 0),
                 "n_events or n_tokens is NULL, or events_out / tokens_out is NULL with a maximum above 0");
    SessionBook & book = S->book;
    // (a busy session whose last block read left no work and no queue has a block of dead passes unread: it is read, not followed by another)
    const bool enqueue = book.busy() && book.wants_block();
    if (enqueue && !session_enqueue(S)) return false;
    const uint64_t upto = ((flags & RWKV_MI_POLL_DRAIN) || !enqueue) ? book.enqueued : book.enqueued - 1;
    if (!session_consume(S, upto)) return false;
    book.deliver(events_out, max_events, tokens_out, max_tokens, n_events, n_tokens);
    return true;
}

RWKV_API bool rwkv_mi_batch_serve_stats(struct rwkv_mi_serve_session * S, uint64_t * passes, uint64_t * blocks, uint32_t * in_flight, uint32_t * room) {
    if (!S) return false;
    S->B->ctx->last_error = RWKV_ERROR_NONE;
    if (passes) *passes = S->book.passes;
    if (blocks) *blocks = S->book.enqueued;
    if (in_flight) *in_flight = S->book.in_flight;
    if (room) *room = S->book.room();
    return true;
}

RWKV_API bool rwkv_mi_batch_serve_close(struct rwkv_mi_serve_session * S, uint32_t * last_request_out) {
    return S ? session_close(S, last_request_out) : false;
}

RWKV_API bool rwkv_mi_batch_eval_draft(struct rwkv_mi_batch * B, const uint32_t * slots, const uint32_t * lens, const uint32_t * tokens, size_t n,
                                       const struct rwkv_mi_sample_params * params, const struct rwkv_mi_penalty_params * penalties,
                                       size_t stride, uint32_t * tokens_out, uint32_t * lens_out, float * logits_out) {
    B->ctx->last_error = RWKV_ERROR_NONE;
    RW_CTX_CHECK(B->ctx, RWKV_ERROR_ARGS, false, params != nullptr || penalties == nullptr, "penalties are given without params");
    BatchCall c{slots, tokens, n};
    c.ragged = true; c.lens = lens;
    c.draw = penalties ? Draw::penalized : params ? Draw::sample : Draw::none;
    c.params = params; c.penalties = penalties;
    c.stride = stride; c.lens_out = lens_out; c.logits_out = logits_out;
    return batch_draft(B, c, tokens_out);
}

RWKV_API bool rwkv_mi_batch_state_copy(struct rwkv_mi_batch * B, size_t dst_slot, size_t src_slot, uint32_t what) {
    rwkv_context * ctx = B->ctx;
    ctx->last_error = RWKV_ERROR_NONE;
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, dst_slot < B->n_slots && src_slot < B->n_slots, "slot %zu or %zu is out of range", dst_slot, src_slot);
    // (no bit for the truncation setting: it is two host words the caller sets on the destination slot themselves)
    const uint32_t known = RWKV_MI_COPY_STATE | RWKV_MI_COPY_COUNTER | RWKV_MI_COPY_COUNTS | RWKV_MI_COPY_BIAS;
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, (what & ~known) == 0, "unknown bits in what (0x%" PRIx32 ")", what);
    // (nor one for the repetition setting; but a row of floats is not a row of counts: the copy is between slots of one kind)
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, !(what & RWKV_MI_COPY_COUNTS) || B->draw.decaying(dst_slot) == B->draw.decaying(src_slot),
                 "RWKV_MI_COPY_COUNTS between a decaying slot and one that is not (%zu, %zu)", dst_slot, src_slot);
    if (dst_slot == src_slot) return true;
    BATCH_HIP_OK(B, hipSetDevice(ctx->model->device));
    hipStream_t st = B->run->stream;
    DrawState & d = B->draw;
    BATCH_HIP_OK(B, hipMemcpyAsync(B->slot_buf(dst_slot, B->parity[dst_slot]), B->slot_buf(src_slot, B->parity[src_slot]), (size_t) B->state_len * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (what & RWKV_MI_COPY_COUNTER)
        BATCH_HIP_OK(B, hipMemcpyAsync(d.counter(dst_slot), d.counter(src_slot), sizeof(unsigned long long), hipMemcpyDeviceToDevice, st));
    // (a batch without the penalty tables has every count 0 and no bias: there is nothing to copy)
    if ((what & RWKV_MI_COPY_COUNTS) && d.counts)
        BATCH_HIP_OK(B, hipMemcpyAsync(d.counts_of(dst_slot), d.counts_of(src_slot), d.n_vocab * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    if ((what & RWKV_MI_COPY_BIAS) && d.bias) {
        BATCH_HIP_OK(B, hipMemcpyAsync(d.bias.p + dst_slot * d.n_vocab, d.bias.p + src_slot * d.n_vocab, d.n_vocab * sizeof(float), hipMemcpyDeviceToDevice, st));
        d.has_bias[dst_slot] = d.has_bias[src_slot];
    }
    BATCH_HIP_OK(B, hipStreamSynchronize(st));
    return true;
}

RWKV_API bool rwkv_mi_batch_decode_beam(struct rwkv_mi_batch * B, const uint32_t * slots, const uint32_t * first_tokens, size_t n_groups,
                                        const struct rwkv_mi_beam_params * params, size_t n_tokens, uint32_t * tokens_out, uint32_t * lens_out,
                                        double * scores_out, float * logprobs_out, float * elapsed_ms) {
    return batch_beam(B, BeamCall{slots, first_tokens, n_groups, params, n_tokens}, tokens_out, lens_out, scores_out, logprobs_out, elapsed_ms);
}

RWKV_API bool rwkv_mi_batch_set_logprobs(struct rwkv_mi_batch * B, bool enabled, uint32_t top_n) {
    B->ctx->last_error = RWKV_ERROR_NONE;
    RW_CTX_CHECK(B->ctx, RWKV_ERROR_ARGS, false, B->session == nullptr, "a serve session is open on this batch (it takes no log-prob report)");
    return B->lp.set(B->ctx, enabled, top_n);
}

RWKV_API bool rwkv_mi_batch_logprobs_shape(struct rwkv_mi_batch * B, size_t * rows, size_t * steps, uint32_t * top_n) {
    B->ctx->last_error = RWKV_ERROR_NONE;
    return B->lp.shape(B->ctx, rows, steps, top_n);
}

RWKV_API bool rwkv_mi_batch_logprobs_store(struct rwkv_mi_batch * B, size_t stride, float * chosen_out, uint32_t * top_ids_out, float * top_logprobs_out) {
    B->ctx->last_error = RWKV_ERROR_NONE;
    BATCH_HIP_OK(B, hipSetDevice(B->ctx->model->device));
    return B->lp.store(B->ctx, B->run->stream, stride, chosen_out, top_ids_out, top_logprobs_out);
}

// ---- guided decoding (include/rwkv_mi355x.h): the guides of a batch and the guide words of its slots ----

RWKV_API bool rwkv_mi_batch_guide_create(struct rwkv_mi_batch * B, uint32_t n_states, const uint32_t * edge_begin, const uint32_t * edge_tokens,
                                         const uint32_t * edge_next, uint32_t * guide_out) {
    rwkv_context * ctx = B->ctx;
    ctx->last_error = RWKV_ERROR_NONE;
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, guide_out != nullptr, "guide_out is NULL");
    const size_t n_vocab = (size_t) ctx->model->n_vocab();
    const char * fault = guide_edges_fault(n_vocab, n_states, edge_begin, edge_tokens, edge_next);
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, fault == nullptr, "bad guide: %s", fault);
    uint32_t id = 0;
    while (id < RWKV_MI_GUIDE_MAX && B->guide_states[id]) id++;
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, id < RWKV_MI_GUIDE_MAX, "the batch already holds %d guides", RWKV_MI_GUIDE_MAX);
    BATCH_HIP_OK(B, hipSetDevice(ctx->model->device));
    bool alloc_failed = false;
    const hipError_t e = guide_table_build(B->guides[id], n_vocab, n_states, edge_begin, edge_tokens, edge_next, B->run->stream, &alloc_failed);
    RW_CTX_CHECK(ctx, RWKV_ERROR_ALLOC, false, !alloc_failed, "cannot allocate the table of a guide of %" PRIu32 " states (%zu bytes): %s", n_states,
                 (size_t) n_states * n_vocab * sizeof(uint16_t), hipGetErrorString(e));
    BATCH_HIP_OK(B, e);
    B->guide_states[id] = n_states;
    *guide_out = id;
    return true;
}

RWKV_API bool rwkv_mi_batch_guide_free(struct rwkv_mi_batch * B, uint32_t guide) {
    rwkv_context * ctx = B->ctx;
    ctx->last_error = RWKV_ERROR_NONE;
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, guide < RWKV_MI_GUIDE_MAX && B->guide_states[guide], "%" PRIu32 " names no guide", guide);
    for (size_t s = 0; s < B->n_slots; s++)
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, B->draw.guide_of[s] != guide, "guide %" PRIu32 " is still attached to slot %zu", guide, s);
    BATCH_HIP_OK(B, hipSetDevice(ctx->model->device));
    BATCH_HIP_OK(B, hipStreamSynchronize(B->run->stream));
    B->guides[guide].reset();
    B->guide_states[guide] = 0;
    return true;
}

RWKV_API bool rwkv_mi_batch_guide_attach(struct rwkv_mi_batch * B, size_t slot, uint32_t guide, uint32_t state) {
    if (!batch_slot_call(B, slot)) return false;
    rwkv_context * ctx = B->ctx;
    if (guide != RWKV_MI_NO_GUIDE) {
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, guide < RWKV_MI_GUIDE_MAX && B->guide_states[guide], "%" PRIu32 " names no guide", guide);
        RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, state < B->guide_states[guide], "state %" PRIu32 " is out of range (guide %" PRIu32 " has %" PRIu32 " states)", state, guide,
                     B->guide_states[guide]);
    }
    return on_device(ctx) && B->draw.guide_attach(ctx, slot, guide, state, B->run->stream);
}

RWKV_API bool rwkv_mi_batch_guide_state(struct rwkv_mi_batch * B, size_t slot, uint32_t * guide_out, uint32_t * state_out, uint32_t * misses_out) {
    if (!batch_slot_call(B, slot)) return false;
    if (guide_out) *guide_out = B->draw.guide_of[slot];
    return on_device(B->ctx) && B->draw.guide_words(B->ctx, slot, state_out, misses_out, B->run->stream);
}

}  // extern "C"
