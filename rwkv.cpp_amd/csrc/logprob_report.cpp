// logprob_report.cpp -- the report of the emitted tokens (rwkv_mi_*set_logprobs / _logprobs_shape / _logprobs_store): what contexts and
// batches share (model.h, LogprobReport)
#include "model.h"
#include "rwkv_mi355x.h"

#include <cinttypes>
#include <cmath>

using namespace rwkvmi;

bool LogprobReport::set(rwkv_context * ctx, bool enabled, uint32_t top_n) {
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, top_n <= RWKV_MI_TOP_MAX && (size_t) top_n <= (size_t) ctx->model->n_vocab(),
                 "top_n (%" PRIu32 ") is above %d or above n_vocab", top_n, RWKV_MI_TOP_MAX);
    this->enabled = enabled;
    this->top_n = enabled ? top_n : 0;
    valid = false;
    return true;
}

// buffers for `entries` = steps * rows records of the current top_n (grown as one group: a failure leaves the report as it was). The caller
// has drained the stream the previous report was written on.
bool LogprobReport::ensure(rwkv_context * ctx, size_t entries) {
    const size_t top = entries * top_n;
    const bool more = entries > d_chosen.count, more_top = top > d_ids.count;
    const hipError_t e = grow(want(d_chosen, more ? entries : 0), want(d_ids, more_top ? top : 0), want(d_vals, more_top ? top : 0));
    RW_CTX_CHECK(ctx, RWKV_ERROR_ALLOC, false, e == hipSuccess, "cannot allocate the log-prob report of %zu tokens: %s", entries, hipGetErrorString(e));
    if (more || more_top) valid = false;
    return true;
}

bool LogprobReport::begin(rwkv_context * ctx, hipStream_t st, size_t entries) {
    if (!enabled) return true;
    HIP_CTX_OK(ctx, hipStreamSynchronize(st));
    if (!ensure(ctx, entries)) return false;
    valid = false;
    return true;
}

// what a reporting call that succeeded leaves: its shape and, per row, the steps the row wrote (lens == nullptr: all of them)
void LogprobReport::done(size_t rows, size_t steps, const uint32_t * lens) {
    this->rows = rows; this->steps = steps; last_top_n = top_n; valid = true;
    this->lens.assign(rows, (uint32_t) steps);
    for (size_t r = 0; lens && r < rows; r++) this->lens[r] = lens[r];
}

bool LogprobReport::shape(rwkv_context * ctx, size_t * rows, size_t * steps, uint32_t * top_n) const {
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, valid, "there is no log-prob report (no reporting call yet, or rwkv_mi_*set_logprobs since)");
    if (rows) *rows = this->rows;
    if (steps) *steps = this->steps;
    if (top_n) *top_n = last_top_n;
    return true;
}

// [steps][rows] on the device -> [rows][stride] on the host, the way the loops' tokens_out is transposed; an entry behind a row's length
// is 0 / RWKV_MI_NO_TOKEN / -inf
bool LogprobReport::store(rwkv_context * ctx, hipStream_t st, size_t stride, float * chosen_out, uint32_t * top_ids_out, float * top_logprobs_out) const {
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, valid, "there is no log-prob report (no reporting call yet, or rwkv_mi_*set_logprobs since)");
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, stride >= steps, "stride (%zu) is less than the report's steps (%zu)", stride, steps);
    const size_t R = rows, S = steps, N = last_top_n, E = R * S;
    const bool tops = N > 0 && (top_ids_out || top_logprobs_out);
    std::vector<float> hc(chosen_out ? E : 0), hv(tops && top_logprobs_out ? E * N : 0);
    std::vector<uint32_t> hi(tops && top_ids_out ? E * N : 0);
    if (!hc.empty()) HIP_CTX_OK(ctx, hipMemcpyAsync(hc.data(), d_chosen.p, E * sizeof(float), hipMemcpyDeviceToHost, st));
    if (!hi.empty()) HIP_CTX_OK(ctx, hipMemcpyAsync(hi.data(), d_ids.p, E * N * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (!hv.empty()) HIP_CTX_OK(ctx, hipMemcpyAsync(hv.data(), d_vals.p, E * N * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_CTX_OK(ctx, hipStreamSynchronize(st));
    for (size_t r = 0; r < R; r++)
        for (size_t j = 0; j < stride; j++) {
            const bool in = j < lens[r];
            const size_t src = j * R + r, dst = r * stride + j;
            if (chosen_out) chosen_out[dst] = in ? hc[src] : 0.0f;
            for (size_t k = 0; k < N; k++) {
                if (top_ids_out) top_ids_out[dst * N + k] = in ? hi[src * N + k] : RWKV_MI_NO_TOKEN;
                if (top_logprobs_out) top_logprobs_out[dst * N + k] = in ? hv[src * N + k] : -INFINITY;
            }
        }
    return true;
}
