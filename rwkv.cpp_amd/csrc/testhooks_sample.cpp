// testhooks_sample.cpp -- the sampler's entry point for tests/ ONLY (include/rwkv_testhooks_sample.h), the scoring kernel's
// (include/rwkv_testhooks_score.h), the report kernel's (include/rwkv_testhooks_logprobs.h) and the beam step's
// (include/rwkv_testhooks_beam.h). `make` links it with every product
// object into a third library, lib/librwkv_testhooks_sample.so; neither librwkv.so nor librwkv_testhooks.so carries it.
#include "testhooks_draw.h"
#include "rwkv_mi355x.h"
#include "rwkv_testhooks_sample.h"
#include "rwkv_testhooks_score.h"
#include "rwkv_testhooks_logprobs.h"
#include "rwkv_testhooks_beam.h"

#include <vector>

using namespace rwkvmi;

extern "C" {

// Test hook: both entry points of the sampler on standalone logits; row r draws with counters[r].
RWKV_API bool rwkv_mi_test_sample_rows(const float * logits, int64_t n_rows, int64_t n_vocab, const struct rwkv_mi_sample_params * params,
                                       uint64_t * counters, int rows_kernel, uint32_t * tokens_out) {
    g_last_error = RWKV_ERROR_NONE;
    RW_CHECK(RWKV_ERROR_ARGS, false, logits && params && tokens_out && n_rows > 0 && n_rows <= 65535 && n_vocab > 0 && n_vocab <= (int64_t) 1 << 24, "bad arguments");
    DrawHook h;
    const bool ok = h.init(logits, n_rows, n_vocab, params, counters, nullptr, nullptr) &&
                    h.run(DrawForm::of(Draw::sample, false, false, false), rows_kernel != 0, tokens_out, counters, nullptr);
    RW_CHECK(RWKV_ERROR_GRAPH, false, ok, "HIP error: %s", hipGetErrorString(hipGetLastError()));
    return true;
}

// Test hook: the scoring kernel on standalone logits.
RWKV_API bool rwkv_test_score_rows(const float * logits, int64_t rows, int64_t n_vocab, const uint32_t * targets, float * logprobs_out, uint32_t * argmax_out) {
    g_last_error = RWKV_ERROR_NONE;
    RW_CHECK(RWKV_ERROR_ARGS, false, logits && rows > 0 && rows <= 65535 && n_vocab > 0 && n_vocab <= (int64_t) 1 << 24, "bad arguments");
    const size_t R = (size_t) rows, V = (size_t) n_vocab;
    DevBuf<float> logits_buf, lp_buf;
    DevBuf<uint32_t> tgt_buf, am_buf;
    bool ok = logits_buf.alloc(R * V) == hipSuccess && lp_buf.alloc(R) == hipSuccess && tgt_buf.alloc(R) == hipSuccess && am_buf.alloc(R) == hipSuccess;
    float * d_logits = logits_buf.p, * d_lp = lp_buf.p;
    uint32_t * d_tgt = tgt_buf.p, * d_am = am_buf.p;
    ok = ok && hipMemcpy(d_logits, logits, R * V * 4, hipMemcpyHostToDevice) == hipSuccess &&
              (!targets || hipMemcpy(d_tgt, targets, R * 4, hipMemcpyHostToDevice) == hipSuccess);
    if (ok) {
        launch_score_rows(d_logits, rows, (int) n_vocab, targets ? d_tgt : nullptr, logprobs_out ? d_lp : nullptr, argmax_out ? d_am : nullptr, nullptr);
        ok = hipDeviceSynchronize() == hipSuccess &&
             (!logprobs_out || hipMemcpy(logprobs_out, d_lp, R * 4, hipMemcpyDeviceToHost) == hipSuccess) &&
             (!argmax_out || hipMemcpy(argmax_out, d_am, R * 4, hipMemcpyDeviceToHost) == hipSuccess);
    }
    RW_CHECK(RWKV_ERROR_GRAPH, false, ok, "HIP error: %s", hipGetErrorString(hipGetLastError()));
    return true;
}

// Test hook: the report kernel on standalone logits, row r's emitted token tokens[r].
RWKV_API bool rwkv_test_logprob_rows(const float * logits, int64_t rows, int64_t n_vocab, const uint32_t * tokens, uint32_t top_n,
                                     float * chosen_out, uint32_t * top_ids_out, float * top_logprobs_out) {
    g_last_error = RWKV_ERROR_NONE;
    RW_CHECK(RWKV_ERROR_ARGS, false, logits && tokens && rows > 0 && rows <= 65535 && n_vocab > 0 && n_vocab <= (int64_t) 1 << 24 &&
             top_n <= RWKV_MI_TOP_MAX && (int64_t) top_n <= n_vocab, "bad arguments");
    for (int64_t r = 0; r < rows; r++) RW_CHECK(RWKV_ERROR_ARGS, false, (int64_t) tokens[r] < n_vocab, "token %lld is out of range", (long long) r);
    const size_t R = (size_t) rows, V = (size_t) n_vocab, N = top_n ? top_n : 1;   // (top_n == 0: one unused word per row)
    DevBuf<float> logits_buf, ch_buf, lp_buf;
    DevBuf<uint32_t> tok_buf, ids_buf;
    bool ok = logits_buf.alloc(R * V) == hipSuccess && ch_buf.alloc(R) == hipSuccess && tok_buf.alloc(R) == hipSuccess &&
              ids_buf.alloc(R * N) == hipSuccess && lp_buf.alloc(R * N) == hipSuccess;
    float * d_logits = logits_buf.p, * d_ch = ch_buf.p, * d_lp = lp_buf.p;
    uint32_t * d_tok = tok_buf.p, * d_ids = ids_buf.p;
    ok = ok && hipMemcpy(d_logits, logits, R * V * 4, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(d_tok, tokens, R * 4, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        launch_logprob_rows(d_logits, rows, (int) n_vocab, d_tok, (int) top_n, d_ch, d_ids, d_lp, nullptr, nullptr);
        ok = hipDeviceSynchronize() == hipSuccess &&
             (!chosen_out || hipMemcpy(chosen_out, d_ch, R * 4, hipMemcpyDeviceToHost) == hipSuccess) &&
             (!top_ids_out || !top_n || hipMemcpy(top_ids_out, d_ids, R * top_n * 4, hipMemcpyDeviceToHost) == hipSuccess) &&
             (!top_logprobs_out || !top_n || hipMemcpy(top_logprobs_out, d_lp, R * top_n * 4, hipMemcpyDeviceToHost) == hipSuccess);
    }
    RW_CHECK(RWKV_ERROR_GRAPH, false, ok, "HIP error: %s", hipGetErrorString(hipGetLastError()));
    return true;
}

// Test hook: the two kernels of one beam step on standalone logits, scores and finished words.
RWKV_API bool rwkv_test_beam_step(const float * logits, int64_t groups, int64_t n_vocab, const double * scores_in, const uint32_t * finished_in,
                                  uint32_t width, const uint32_t * end_tokens, uint32_t n_end, uint32_t * tokens_out, uint32_t * parents_out,
                                  float * logprobs_out, double * scores_out, uint32_t * finished_out) {
    g_last_error = RWKV_ERROR_NONE;
    RW_CHECK(RWKV_ERROR_ARGS, false, logits && scores_in && finished_in && groups > 0 && n_vocab > 0 && n_vocab <= (int64_t) 1 << 24 &&
             width >= 1 && width <= RWKV_MI_TOP_MAX && (int64_t) width <= n_vocab && groups * (int64_t) width <= 65535 && n_end <= 8 && (!n_end || end_tokens),
             "bad arguments");
    for (uint32_t e = 0; e < n_end; e++) RW_CHECK(RWKV_ERROR_ARGS, false, (int64_t) end_tokens[e] < n_vocab, "end token %u is out of range", e);
    const size_t R = (size_t) groups * width, V = (size_t) n_vocab;
    DevBuf<float> logits_buf, lp_buf, ch_buf, hlp_buf;
    DevBuf<double> score_buf;
    DevBuf<uint32_t> fin_buf, len_buf, ids_buf, tok_buf, htok_buf, hpar_buf;
    bool ok = logits_buf.alloc(R * V) == hipSuccess && lp_buf.alloc(R * width) == hipSuccess && ch_buf.alloc(R) == hipSuccess && hlp_buf.alloc(R) == hipSuccess &&
              score_buf.alloc(R) == hipSuccess && fin_buf.alloc(R) == hipSuccess && len_buf.alloc(R) == hipSuccess && ids_buf.alloc(R * width) == hipSuccess &&
              tok_buf.alloc(R) == hipSuccess && htok_buf.alloc(R) == hipSuccess && hpar_buf.alloc(R) == hipSuccess;
    ok = ok && hipMemcpy(logits_buf.p, logits, R * V * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(score_buf.p, scores_in, R * 8, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(fin_buf.p, finished_in, R * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemset(len_buf.p, 0, R * 4) == hipSuccess && hipMemset(tok_buf.p, 0, R * 4) == hipSuccess;
    if (ok) {
        BeamTables t{score_buf.p, fin_buf.p, len_buf.p, ids_buf.p, lp_buf.p, ch_buf.p, htok_buf.p, hpar_buf.p, hlp_buf.p, nullptr, width, n_end, {}};
        for (uint32_t e = 0; e < n_end; e++) t.end_tokens[e] = end_tokens[e];
        launch_beam_rows(logits_buf.p, (int64_t) R, (int) n_vocab, t, nullptr);
        launch_beam_select(t, groups, tok_buf.p, 0u, nullptr, nullptr, nullptr);
        ok = hipDeviceSynchronize() == hipSuccess &&
             (!tokens_out || hipMemcpy(tokens_out, htok_buf.p, R * 4, hipMemcpyDeviceToHost) == hipSuccess) &&
             (!parents_out || hipMemcpy(parents_out, hpar_buf.p, R * 4, hipMemcpyDeviceToHost) == hipSuccess) &&
             (!logprobs_out || hipMemcpy(logprobs_out, hlp_buf.p, R * 4, hipMemcpyDeviceToHost) == hipSuccess) &&
             (!scores_out || hipMemcpy(scores_out, score_buf.p, R * 8, hipMemcpyDeviceToHost) == hipSuccess) &&
             (!finished_out || hipMemcpy(finished_out, fin_buf.p, R * 4, hipMemcpyDeviceToHost) == hipSuccess);
    }
    RW_CHECK(RWKV_ERROR_GRAPH, false, ok, "HIP error: %s", hipGetErrorString(hipGetLastError()));
    return true;
}

}  // extern "C"
