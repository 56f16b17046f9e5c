// testhooks_cut.cpp -- the truncating sampler's entry point for tests/ ONLY (include/rwkv_testhooks_cut.h). `make` links it with every product
// object into a library of its own, lib/librwkv_testhooks_cut.so; no other library carries it.
#include "testhooks_draw.h"
#include "rwkv_mi355x.h"
#include "rwkv_testhooks_cut.h"

using namespace rwkvmi;

extern "C" {

// Test hook: both entry points of the plain sampler on standalone logits with a truncation setting per row; row r draws with counters[r].
RWKV_API bool rwkv_mi_test_cut_rows(const float * logits, int64_t n_rows, int64_t n_vocab, const struct rwkv_mi_sample_params * params,
                                    const struct rwkv_mi_test_cut * cuts, uint64_t * counters, int rows_kernel, uint32_t * tokens_out,
                                    float * weights_out) {
    g_last_error = RWKV_ERROR_NONE;
    RW_CHECK(RWKV_ERROR_ARGS, false, logits && params && cuts && tokens_out && n_rows > 0 && n_rows <= 65535 && n_vocab > 0 && n_vocab <= (int64_t) 1 << 24,
             "bad arguments");
    for (int64_t r = 0; r < n_rows; r++)
        RW_CHECK(RWKV_ERROR_ARGS, false, cuts[r].min_p >= 0.0f && cuts[r].min_p <= 1.0f, "bad min_p of row %zu", (size_t) r);
    DrawHook h;
    bool ok = h.init(logits, n_rows, n_vocab, params, counters, nullptr, nullptr);
    for (size_t r = 0; ok && r < h.R; r++) { h.rows[r].top_k = cuts[r].top_k; h.rows[r].min_p = cuts[r].min_p; }
    // (the row kernel in its truncating form whatever the settings; weights_out reads each row's stretch of the scratch after the draw)
    ok = ok && h.run(DrawForm::of(Draw::sample, true, false, false), rows_kernel != 0, tokens_out, counters, nullptr) && (!weights_out || h.weights(weights_out));
    RW_CHECK(RWKV_ERROR_GRAPH, false, ok, "HIP error: %s", hipGetErrorString(hipGetLastError()));
    return true;
}

}  // extern "C"
