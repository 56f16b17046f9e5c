// testhooks_cut.cpp -- the truncating sampler's entry point for tests/ ONLY (include/rwkv_testhooks_cut.h). `make` links it with every product
// object into a library of its own, lib/librwkv_testhooks_cut.so; no other library carries it.
#include "model.h"
#include "rwkv_mi355x.h"
#include "rwkv_testhooks_cut.h"

#include <vector>

using namespace rwkvmi;

extern "C" {

// Test hook: both entry points of the plain sampler on standalone logits with a truncation setting per row; row r draws with counters[r].
RWKV_API bool rwkv_mi_test_cut_rows(const float * logits, int64_t n_rows, int64_t n_vocab, const struct rwkv_mi_sample_params * params,
                                    const struct rwkv_mi_test_cut * cuts, uint64_t * counters, int rows_kernel, uint32_t * tokens_out,
                                    float * weights_out) {
    g_last_error = RWKV_ERROR_NONE;
    RW_CHECK(RWKV_ERROR_ARGS, false, logits && params && cuts && tokens_out && n_rows > 0 && n_rows <= 65535 && n_vocab > 0 && n_vocab <= (int64_t) 1 << 24,
             "bad arguments");
    const size_t R = (size_t) n_rows, V = (size_t) n_vocab, S = sample_scratch_floats(n_vocab);
    for (size_t r = 0; r < R; r++)
        RW_CHECK(RWKV_ERROR_ARGS, false, cuts[r].min_p >= 0.0f && cuts[r].min_p <= 1.0f, "bad min_p of row %zu", r);
    DevBuf<float> logits_buf, probs_buf;
    DevBuf<unsigned long long> ctr_buf;
    DevBuf<SampleRow> table_buf;
    DevBuf<CutRow> cut_buf;
    DevBuf<uint32_t> tok_buf;
    std::vector<SampleRow> table(R);
    std::vector<CutRow> crows(R);
    bool ok = logits_buf.alloc(R * V) == hipSuccess && probs_buf.alloc(R * S) == hipSuccess && ctr_buf.alloc(R) == hipSuccess &&
              table_buf.alloc(R) == hipSuccess && cut_buf.alloc(R) == hipSuccess && tok_buf.alloc(R) == hipSuccess;
    ok = ok && hipMemcpy(logits_buf.p, logits, R * V * 4, hipMemcpyHostToDevice) == hipSuccess &&
         (counters ? hipMemcpy(ctr_buf.p, counters, R * 8, hipMemcpyHostToDevice) : hipMemset(ctr_buf.p, 0, R * 8)) == hipSuccess;
    if (ok) {
        for (size_t r = 0; r < R; r++) { table[r] = SampleRow{params[r], ctr_buf.p + r}; crows[r] = CutRow{cuts[r].top_k, cuts[r].min_p}; }
        ok = hipMemcpy(table_buf.p, table.data(), R * sizeof(SampleRow), hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(cut_buf.p, crows.data(), R * sizeof(CutRow), hipMemcpyHostToDevice) == hipSuccess;
    }
    if (ok) {
        // (every row has its own stretch of the scratch in both forms: weights_out reads it after the draw)
        if (rows_kernel) launch_sample_rows(logits_buf.p, n_rows, (int) n_vocab, table_buf.p, cut_buf.p, probs_buf.p, tok_buf.p, nullptr, nullptr, nullptr);
        else for (size_t r = 0; r < R; r++)
            launch_sample(logits_buf.p + r * V, (int) n_vocab, params[r].temperature, params[r].top_p, params[r].u, params[r].seed, ctr_buf.p + r, crows[r],
                          probs_buf.p + r * S, tok_buf.p + r, nullptr, 0, nullptr);
        ok = hipDeviceSynchronize() == hipSuccess && hipMemcpy(tokens_out, tok_buf.p, R * 4, hipMemcpyDeviceToHost) == hipSuccess &&
             (!counters || hipMemcpy(counters, ctr_buf.p, R * 8, hipMemcpyDeviceToHost) == hipSuccess);
    }
    if (ok && weights_out) {
        // token t = i0 + j of thread tid, i0 = tid * C, lives at scratch[j * 1024 + tid] (sampling.hip, sample_body)
        std::vector<float> scratch(R * S);
        ok = hipMemcpy(scratch.data(), probs_buf.p, R * S * 4, hipMemcpyDeviceToHost) == hipSuccess;
        const size_t C = S / 1024;
        for (size_t r = 0; ok && r < R; r++)
            for (size_t t = 0; t < V; t++) weights_out[r * V + t] = scratch[r * S + (t % C) * 1024 + t / C];
    }
    RW_CHECK(RWKV_ERROR_GRAPH, false, ok, "HIP error: %s", hipGetErrorString(hipGetLastError()));
    return true;
}

}  // extern "C"
