// testhooks_draw.h -- what the sampler's test hooks share (testhooks_sample / _guide / _cut / _decay.cpp, tests/ ONLY): R standalone rows of
// logits on the device with a draw counter, a stretch of the scratch and a token word each, optional occurrence and bias rows, and their
// DrawRow table; the draw in either entry form; what comes back. No product object includes it.
#pragma once
#include "model.h"

#include <vector>

namespace rwkvmi {

struct DrawHook {
    size_t R = 0, V = 0, S = 0;   // rows, vocabulary, floats of a row's scratch
    DevBuf<float> logits, probs, bias;
    DevBuf<unsigned long long> ctr;
    DevBuf<uint32_t> tok, occ;
    DevBuf<DrawRow> table;
    std::vector<DrawRow> rows;    // the host's rows: plain draws after init(), then what the hook sets

    // the buffers, uploaded: logits [R][V]; counters [R] (NULL: zero); occurrence and bias rows [R][V] (NULL: none, and the rows' pointers stay NULL)
    bool init(const float * h_logits, int64_t n_rows, int64_t n_vocab, const rwkv_mi_sample_params * params, const uint64_t * counters, const uint32_t * h_occ,
              const float * h_bias) {
        R = (size_t) n_rows; V = (size_t) n_vocab; S = sample_scratch_floats(n_vocab);
        bool ok = logits.alloc(R * V) == hipSuccess && probs.alloc(R * S) == hipSuccess && ctr.alloc(R) == hipSuccess && tok.alloc(R) == hipSuccess &&
                  table.alloc(R) == hipSuccess && (!h_occ || occ.alloc(R * V) == hipSuccess) && (!h_bias || bias.alloc(R * V) == hipSuccess);
        ok = ok && hipMemcpy(logits.p, h_logits, R * V * 4, hipMemcpyHostToDevice) == hipSuccess &&
             (counters ? hipMemcpy(ctr.p, counters, R * 8, hipMemcpyHostToDevice) : hipMemset(ctr.p, 0, R * 8)) == hipSuccess &&
             (!h_occ || hipMemcpy(occ.p, h_occ, R * V * 4, hipMemcpyHostToDevice) == hipSuccess) &&
             (!h_bias || hipMemcpy(bias.p, h_bias, R * V * 4, hipMemcpyHostToDevice) == hipSuccess);
        rows.resize(R);
        for (size_t r = 0; ok && r < R; r++)
            rows[r] = DrawRow{params[r], ctr.p + r, 0.0f, 0.0f, 0u, nullptr, nullptr, nullptr, nullptr, nullptr, 0u, 0.0f, 1.0f, 1.0f};
        return ok;
    }
    // row r draws penalised from its occurrence row and, where there is one, its bias row
    void penalise(size_t r, const rwkv_mi_penalty_params & pen) {
        rows[r].presence = pen.presence; rows[r].frequency = pen.frequency; rows[r].record = pen.record;
        rows[r].count = occ.p + r * V; rows[r].bias = bias ? bias.p + r * V : nullptr;
    }
    // The draw, every row on its own stretch of the scratch: the row kernel once in `form`, or the context kernel once per row in the form a
    // context with that row's settings launches. Then the tokens [R] and, where asked for, the counters [R] and the occurrence rows [R][V]
    bool run(const DrawForm & form, bool rows_kernel, uint32_t * tokens_out, uint64_t * counters_out, uint32_t * occ_out) {
        if (hipMemcpy(table.p, rows.data(), R * sizeof(DrawRow), hipMemcpyHostToDevice) != hipSuccess) return false;
        if (rows_kernel) launch_draw_rows(logits.p, (int64_t) R, (int) V, table.p, form, probs.p, tok.p, nullptr, nullptr, nullptr);
        else for (size_t r = 0; r < R; r++)
            launch_draw(logits.p + r * V, (int) V, rows[r], DrawForm::of_row(form.draw, rows[r]), probs.p + r * S, tok.p + r, nullptr, 0, nullptr);
        return hipDeviceSynchronize() == hipSuccess && hipMemcpy(tokens_out, tok.p, R * 4, hipMemcpyDeviceToHost) == hipSuccess &&
               (!counters_out || hipMemcpy(counters_out, ctr.p, R * 8, hipMemcpyDeviceToHost) == hipSuccess) &&
               (!occ_out || hipMemcpy(occ_out, occ.p, R * V * 4, hipMemcpyDeviceToHost) == hipSuccess);
    }
    // what the draw left in the scratch, in token order [R][V]: token t = i0 + j of thread tid, i0 = tid * C, lives at scratch[j * 1024 + tid]
    // (sampling.hip, sample_body)
    bool weights(float * weights_out) {
        std::vector<float> scratch(R * S);
        if (hipMemcpy(scratch.data(), probs.p, R * S * 4, hipMemcpyDeviceToHost) != hipSuccess) return false;
        const size_t C = S / 1024;
        for (size_t r = 0; r < R; r++)
            for (size_t t = 0; t < V; t++) weights_out[r * V + t] = scratch[r * S + (t % C) * 1024 + t / C];
        return true;
    }
};

}  // namespace rwkvmi
