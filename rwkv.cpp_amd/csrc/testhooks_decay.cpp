// testhooks_decay.cpp -- the entry points of the penalised sampler with a repetition setting for tests/ ONLY (include/rwkv_testhooks_decay.h).
// `make` links it with every product object into a library of its own, lib/librwkv_testhooks_decay.so; no other library carries it.
#include "model.h"
#include "rwkv_mi355x.h"
#include "rwkv_testhooks_decay.h"

#include <cmath>
#include <vector>

using namespace rwkvmi;

extern "C" {

// Test hook: both entry forms of the penalised sampler with a repetition setting per row on standalone logits and occurrence rows.
RWKV_API bool rwkv_mi_test_decay_rows(const float * logits, int64_t n_rows, int64_t n_vocab, const struct rwkv_mi_sample_params * params,
                                      const struct rwkv_mi_penalty_params * penalties, const struct rwkv_mi_test_rep * reps, uint32_t * occ,
                                      const float * bias, uint64_t * counters, int rows_kernel, uint32_t * tokens_out) {
    g_last_error = RWKV_ERROR_NONE;
    RW_CHECK(RWKV_ERROR_ARGS, false, logits && params && penalties && reps && occ && tokens_out && n_rows > 0 && n_rows <= 65535 && n_vocab > 0 &&
             n_vocab <= (int64_t) 1 << 24, "bad arguments");
    const size_t R = (size_t) n_rows, V = (size_t) n_vocab, S = sample_scratch_floats(n_vocab);
    for (size_t r = 0; r < R; r++)
        RW_CHECK(RWKV_ERROR_ARGS, false, reps[r].decay >= 0.0f && reps[r].decay <= 1.0f && reps[r].repetition > 0.0f && std::isfinite(reps[r].repetition),
                 "bad setting of row %zu", r);
    DevBuf<float> logits_buf, probs_buf, bias_buf;
    DevBuf<unsigned long long> ctr_buf;
    DevBuf<PenaltyRow> table_buf;
    DevBuf<RepRow> rep_buf;
    DevBuf<uint32_t> tok_buf, occ_buf;
    std::vector<PenaltyRow> table(R);
    std::vector<RepRow> rrows(R);
    bool ok = logits_buf.alloc(R * V) == hipSuccess && probs_buf.alloc(R * S) == hipSuccess && ctr_buf.alloc(R) == hipSuccess && table_buf.alloc(R) == hipSuccess &&
              rep_buf.alloc(R) == hipSuccess && tok_buf.alloc(R) == hipSuccess && occ_buf.alloc(R * V) == hipSuccess && (!bias || bias_buf.alloc(R * V) == hipSuccess);
    ok = ok && hipMemcpy(logits_buf.p, logits, R * V * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(occ_buf.p, occ, R * V * 4, hipMemcpyHostToDevice) == hipSuccess &&
         (!bias || hipMemcpy(bias_buf.p, bias, R * V * 4, hipMemcpyHostToDevice) == hipSuccess) &&
         (counters ? hipMemcpy(ctr_buf.p, counters, R * 8, hipMemcpyHostToDevice) : hipMemset(ctr_buf.p, 0, R * 8)) == hipSuccess;
    if (ok) {
        for (size_t r = 0; r < R; r++) {
            table[r] = PenaltyRow{params[r], ctr_buf.p + r, penalties[r].presence, penalties[r].frequency, penalties[r].record, occ_buf.p + r * V,
                                  bias ? bias_buf.p + r * V : nullptr};
            rrows[r] = RepRow{reps[r].decay, reps[r].repetition};
        }
        ok = hipMemcpy(table_buf.p, table.data(), R * sizeof(PenaltyRow), hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(rep_buf.p, rrows.data(), R * sizeof(RepRow), hipMemcpyHostToDevice) == hipSuccess;
    }
    if (ok) {
        if (rows_kernel) launch_pen_sample_rows(logits_buf.p, n_rows, (int) n_vocab, table_buf.p, nullptr, rep_buf.p, probs_buf.p, tok_buf.p, nullptr, nullptr, nullptr);
        else for (size_t r = 0; r < R; r++)
            launch_pen_sample(logits_buf.p + r * V, (int) n_vocab, params[r].temperature, params[r].top_p, params[r].u, params[r].seed, ctr_buf.p + r,
                              penalties[r].presence, penalties[r].frequency, penalties[r].record, occ_buf.p + r * V, table[r].bias, CutRow{0u, 0.0f}, rrows[r],
                              probs_buf.p + r * S, tok_buf.p + r, nullptr, 0, nullptr);
        ok = hipDeviceSynchronize() == hipSuccess && hipMemcpy(tokens_out, tok_buf.p, R * 4, hipMemcpyDeviceToHost) == hipSuccess &&
             hipMemcpy(occ, occ_buf.p, R * V * 4, hipMemcpyDeviceToHost) == hipSuccess &&
             (!counters || hipMemcpy(counters, ctr_buf.p, R * 8, hipMemcpyDeviceToHost) == hipSuccess);
    }
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
