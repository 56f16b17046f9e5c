// testhooks_decay.cpp -- the entry points of the penalised sampler with a repetition setting for tests/ ONLY (include/rwkv_testhooks_decay.h).
// `make` links it with every product object into a library of its own, lib/librwkv_testhooks_decay.so; no other library carries it.
#include "testhooks_draw.h"
#include "rwkv_mi355x.h"
#include "rwkv_testhooks_decay.h"

#include <cmath>

using namespace rwkvmi;

extern "C" {

// Test hook: both entry forms of the penalised sampler with a repetition setting per row on standalone logits and occurrence rows.
RWKV_API bool rwkv_mi_test_decay_rows(const float * logits, int64_t n_rows, int64_t n_vocab, const struct rwkv_mi_sample_params * params,
                                      const struct rwkv_mi_penalty_params * penalties, const struct rwkv_mi_test_rep * reps, uint32_t * occ,
                                      const float * bias, uint64_t * counters, int rows_kernel, uint32_t * tokens_out) {
    g_last_error = RWKV_ERROR_NONE;
    RW_CHECK(RWKV_ERROR_ARGS, false, logits && params && penalties && reps && occ && tokens_out && n_rows > 0 && n_rows <= 65535 && n_vocab > 0 &&
             n_vocab <= (int64_t) 1 << 24, "bad arguments");
    for (size_t r = 0; r < (size_t) n_rows; r++)
        RW_CHECK(RWKV_ERROR_ARGS, false, reps[r].decay >= 0.0f && reps[r].decay <= 1.0f && reps[r].repetition > 0.0f && std::isfinite(reps[r].repetition),
                 "bad setting of row %zu", r);
    DrawHook h;
    bool ok = h.init(logits, n_rows, n_vocab, params, counters, occ, bias);
    for (size_t r = 0; ok && r < h.R; r++) { h.penalise(r, penalties[r]); h.rows[r].decay = reps[r].decay; h.rows[r].repetition = reps[r].repetition; }
    // (the row kernel in its repetition form whatever the settings)
    ok = ok && h.run(DrawForm::of(Draw::penalized, false, false, true), rows_kernel != 0, tokens_out, counters, occ);
    RW_CHECK(RWKV_ERROR_GRAPH, false, ok, "HIP error: %s", hipGetErrorString(hipGetLastError()));
    return true;
}

// Test hook: k_count_add_decay on a standalone row.
RWKV_API bool rwkv_mi_test_decay_counts_add(float * occ, int64_t n_vocab, const uint32_t * tokens, int64_t n_tokens, float decay) {
    g_last_error = RWKV_ERROR_NONE;
    RW_CHECK(RWKV_ERROR_ARGS, false, occ && tokens && n_vocab > 0 && n_vocab <= (int64_t) 1 << 24 && n_tokens > 0 && decay >= 0.0f && decay <= 1.0f, "bad arguments");
    for (int64_t i = 0; i < n_tokens; i++) RW_CHECK(RWKV_ERROR_ARGS, false, tokens[i] < (uint64_t) n_vocab, "token %lld is out of range", (long long) i);
    DevBuf<float> occ_buf;
    DevBuf<uint32_t> tok_buf;
    bool ok = occ_buf.alloc((size_t) n_vocab) == hipSuccess && tok_buf.alloc((size_t) n_tokens) == hipSuccess &&
              hipMemcpy(occ_buf.p, occ, (size_t) n_vocab * 4, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(tok_buf.p, tokens, (size_t) n_tokens * 4, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        launch_count_add_decay(occ_buf.p, tok_buf.p, n_tokens, (int) n_vocab, decay, nullptr);
        ok = hipDeviceSynchronize() == hipSuccess && hipMemcpy(occ, occ_buf.p, (size_t) n_vocab * 4, hipMemcpyDeviceToHost) == hipSuccess;
    }
    RW_CHECK(RWKV_ERROR_GRAPH, false, ok, "HIP error: %s", hipGetErrorString(hipGetLastError()));
    return true;
}

}  // extern "C"
