// testhooks_guide.cpp -- the guided sampler's entry point for tests/ ONLY (include/rwkv_testhooks_guide.h). `make` links it with every product
// object into a library of its own, lib/librwkv_testhooks_guide.so; no other library carries it.
#include "testhooks_draw.h"
#include "rwkv_mi355x.h"
#include "rwkv_testhooks_guide.h"

#include <vector>

using namespace rwkvmi;

extern "C" {

// Test hook: the two guided row kernels on standalone logits, guides built by k_guide_expand from the caller's edges.
RWKV_API bool rwkv_mi_test_guided_rows(const float * logits, int64_t n_rows, int64_t n_vocab, uint32_t n_guides, const uint32_t * n_states,
                                       const uint32_t * edge_begin, const uint32_t * edge_tokens, const uint32_t * edge_next,
                                       const uint32_t * row_guide, const uint32_t * row_state, const struct rwkv_mi_sample_params * params,
                                       const struct rwkv_mi_penalty_params * penalties, uint32_t * counts, const float * bias, uint64_t * counters,
                                       uint32_t * tokens_out, uint32_t * states_out, uint32_t * misses_out) {
    g_last_error = RWKV_ERROR_NONE;
    RW_CHECK(RWKV_ERROR_ARGS, false, logits && params && row_guide && row_state && tokens_out && states_out && misses_out && n_rows > 0 && n_rows <= 65535 &&
             n_vocab > 0 && n_vocab <= (int64_t) 1 << 24 && n_guides <= RWKV_MI_GUIDE_MAX && (!n_guides || n_states) && (!penalties || counts), "bad arguments");
    const size_t R = (size_t) n_rows, V = (size_t) n_vocab;
    // where each guide's edges start, every rule of rwkv_mi_batch_guide_create on them, every row's guide and state
    std::vector<size_t> begin_at(n_guides), edge_at(n_guides);
    size_t nb = 0, ne = 0;
    for (uint32_t g = 0; g < n_guides; g++) {
        begin_at[g] = nb; edge_at[g] = ne;
        RW_CHECK(RWKV_ERROR_ARGS, false, edge_begin && n_states[g] > 0 && n_states[g] <= RWKV_MI_GUIDE_MAX_STATES, "bad n_states of guide %u", g);
        const char * fault = guide_edges_fault(V, n_states[g], edge_begin + nb, edge_tokens ? edge_tokens + ne : nullptr, edge_next ? edge_next + ne : nullptr);
        RW_CHECK(RWKV_ERROR_ARGS, false, fault == nullptr, "bad guide %u: %s", g, fault);
        ne += edge_begin[nb + n_states[g]];
        nb += (size_t) n_states[g] + 1;
    }
    for (size_t r = 0; r < R; r++)
        RW_CHECK(RWKV_ERROR_ARGS, false, row_guide[r] == RWKV_MI_NO_GUIDE || (row_guide[r] < n_guides && row_state[r] < n_states[row_guide[r]]),
                 "bad guide or state of row %zu", r);
    std::vector<DevBuf<uint16_t>> tables(n_guides);
    DevBuf<uint32_t> state_buf, miss_buf;
    DrawHook h;
    bool ok = h.init(logits, n_rows, n_vocab, params, counters, penalties ? counts : nullptr, penalties ? bias : nullptr) && state_buf.alloc(R) == hipSuccess &&
              miss_buf.alloc(R) == hipSuccess;
    for (uint32_t g = 0; ok && g < n_guides; g++) {
        bool alloc_failed = false;
        ok = guide_table_build(tables[g], V, n_states[g], edge_begin + begin_at[g], edge_tokens + edge_at[g], edge_next + edge_at[g], nullptr, &alloc_failed) == hipSuccess;
    }
    ok = ok && hipMemcpy(state_buf.p, row_state, R * 4, hipMemcpyHostToDevice) == hipSuccess && hipMemset(miss_buf.p, 0, R * 4) == hipSuccess;
    for (size_t r = 0; ok && r < R; r++) {
        if (penalties) h.penalise(r, penalties[r]);
        h.rows[r].next = row_guide[r] == RWKV_MI_NO_GUIDE ? nullptr : tables[row_guide[r]].p;
        h.rows[r].state = state_buf.p + r; h.rows[r].misses = miss_buf.p + r;
    }
    // (the row kernel in its guided form whatever the rows' guides)
    ok = ok && h.run(DrawForm::of(penalties ? Draw::penalized : Draw::sample, false, true, false), true, tokens_out, counters, penalties ? counts : nullptr) &&
         hipMemcpy(states_out, state_buf.p, R * 4, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(misses_out, miss_buf.p, R * 4, hipMemcpyDeviceToHost) == hipSuccess;
    RW_CHECK(RWKV_ERROR_GRAPH, false, ok, "HIP error: %s", hipGetErrorString(hipGetLastError()));
    return true;
}

}  // extern "C"
