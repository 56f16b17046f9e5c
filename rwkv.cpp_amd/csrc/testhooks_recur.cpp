// testhooks_recur.cpp -- the launchers of the RWKV-5 / 6 / 7 recurrences, the group norm and the RWKV-7 key preparation on caller-supplied host
// arrays, for tests/ ONLY (include/rwkv_testhooks_recur.h). `make` links it with every product object into a library of its own,
// lib/librwkv_testhooks_recur.so; no other library carries it.
#include "model.h"
#include "kernels.h"
#include "devmem.h"
#include "rwkv_mi355x.h"
#include "rwkv_testhooks_recur.h"

#include <vector>

using namespace rwkvmi;

namespace {

constexpr int64_t MAX_T = 4096, MAX_H = 1024, MAX_S = 1024, MAX_SLOTS = 4096;

bool shape_ok(int64_t T, int64_t H, int64_t S) { return T > 0 && T <= MAX_T && H > 0 && H <= MAX_H && S > 0 && S <= MAX_S; }

struct Up {
    bool ok = true;
    bool operator()(DevBuf<float> & b, const float * src, size_t n, size_t pad = 0) {
        ok = ok && b.alloc(pad + n) == hipSuccess && (pad == 0 || hipMemset(b.p, 0, pad * 4) == hipSuccess) &&
             hipMemcpy(b.p + pad, src, n * 4, hipMemcpyHostToDevice) == hipSuccess;
        return ok;
    }
};

// the device side of a rwkv_mi_test_recur_states: both buffers behind `pad` floats, and the table of the form
struct States {
    DevBuf<float> in, out;
    DevBuf<RowState> rows;
    DevBuf<SegState> segs;
    StateRef ref;
    size_t pad = 0, per_slot = 0, n_slots = 0;

    static bool valid(const rwkv_mi_test_recur_states * s, int64_t T) {
        if (!s || !s->state_in || !s->state_out || !s->slots || s->n_slots <= 0 || s->n_slots > MAX_SLOTS || s->n <= 0 || s->n > s->n_slots) return false;
        if (s->form < 0 || s->form > 2 || (s->form == 0 && s->n != 1) || (s->form == 1 && s->n != T) || (s->form == 2 && (!s->t0 || !s->t1))) return false;
        std::vector<char> slot_used((size_t) s->n_slots, 0), tok_used((size_t) T, 0);
        for (int64_t i = 0; i < s->n; i++) {
            if (s->slots[i] >= (uint64_t) s->n_slots || slot_used[s->slots[i]]) return false;
            slot_used[s->slots[i]] = 1;
            if (s->form != 2) continue;
            if (s->t0[i] < 0 || s->t1[i] <= s->t0[i] || s->t1[i] > T) return false;
            for (int32_t t = s->t0[i]; t < s->t1[i]; t++) { if (tok_used[(size_t) t]) return false; tok_used[(size_t) t] = 1; }
        }
        return true;
    }

    bool build(const rwkv_mi_test_recur_states * s, int64_t H, int64_t S) {
        pad = (size_t) (2 * H * S); per_slot = (size_t) (H * S * S); n_slots = (size_t) s->n_slots;
        Up up;
        if (!up(in, s->state_in, n_slots * per_slot, pad) || !up(out, s->state_out, n_slots * per_slot, pad)) return false;
        ref.off = (int64_t) pad;
        if (s->form == 0) {
            ref.in = in.p + s->slots[0] * per_slot; ref.out = out.p + s->slots[0] * per_slot;
        } else if (s->form == 1) {
            std::vector<RowState> t((size_t) s->n);
            for (size_t i = 0; i < t.size(); i++) t[i] = RowState{in.p + s->slots[i] * per_slot, out.p + s->slots[i] * per_slot};
            if (!rows.upload(t.data(), t.size(), nullptr) || hipStreamSynchronize(nullptr) != hipSuccess) return false;
            ref.rows = rows.p;
        } else {
            std::vector<SegState> t((size_t) s->n);
            for (size_t i = 0; i < t.size(); i++) t[i] = SegState{in.p + s->slots[i] * per_slot, out.p + s->slots[i] * per_slot, s->t0[i], s->t1[i]};
            if (!segs.upload(t.data(), t.size(), nullptr) || hipStreamSynchronize(nullptr) != hipSuccess) return false;
            ref.segs = segs.p; ref.n_segs = s->n;
        }
        return true;
    }

    bool fetch(float * state_out) const { return hipMemcpy(state_out, out.p + pad, n_slots * per_slot * 4, hipMemcpyDeviceToHost) == hipSuccess; }
};

bool finish(bool ok) {
    ok = ok && hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess;
    RW_CHECK(RWKV_ERROR_GRAPH, false, ok, "HIP error: %s", hipGetErrorString(hipGetLastError()));
    return true;
}

}  // namespace

extern "C" {

RWKV_API bool rwkv_mi_test_wkv6(const float * r, const float * k, const float * v, const float * u, int u_per_chan, const float * w, int w_mode,
                                const struct rwkv_mi_test_recur_states * states, float * out, int64_t T, int64_t H, int64_t S) {
    g_last_error = RWKV_ERROR_NONE;
    RW_CHECK(RWKV_ERROR_ARGS, false, r && k && v && u && w && out && shape_ok(T, H, S) && (u_per_chan == 0 || u_per_chan == 1) && w_mode >= 0 && w_mode <= 2 &&
             States::valid(states, T), "bad arguments");
    const size_t n = (size_t) (T * H * S), hs = (size_t) (H * S);
    DevBuf<float> d_r, d_k, d_v, d_u, d_w, d_out;
    States st;
    Up up;
    bool ok = up(d_r, r, n) && up(d_k, k, n) && up(d_v, v, n) && up(d_u, u, u_per_chan ? hs : (size_t) H) &&
              up(d_w, w, w_mode == 2 ? n : w_mode == 1 ? hs : (size_t) H) && up(d_out, out, n) && st.build(states, H, S);
    if (ok) launch_wkv6(d_r.p, d_k.p, d_v.p, d_u.p, u_per_chan, d_w.p, w_mode, st.ref, d_out.p, T, H, S, nullptr);
    if (!finish(ok)) return false;
    ok = st.fetch(states->state_out) && hipMemcpy(out, d_out.p, n * 4, hipMemcpyDeviceToHost) == hipSuccess;
    RW_CHECK(RWKV_ERROR_GRAPH, false, ok, "HIP error: %s", hipGetErrorString(hipGetLastError()));
    return true;
}

RWKV_API bool rwkv_mi_test_wkv7(const float * r, const float * w, const float * k, const float * v, const float * a, const float * b,
                                const struct rwkv_mi_test_recur_states * states, float * out, int64_t T, int64_t H, int64_t S) {
    g_last_error = RWKV_ERROR_NONE;
    RW_CHECK(RWKV_ERROR_ARGS, false, r && w && k && v && a && b && out && shape_ok(T, H, S) && States::valid(states, T), "bad arguments");
    const size_t n = (size_t) (T * H * S);
    DevBuf<float> d_r, d_w, d_k, d_v, d_a, d_b, d_out;
    States st;
    Up up;
    bool ok = up(d_r, r, n) && up(d_w, w, n) && up(d_k, k, n) && up(d_v, v, n) && up(d_a, a, n) && up(d_b, b, n) && up(d_out, out, n) && st.build(states, H, S);
    if (ok) launch_wkv7(d_r.p, d_w.p, d_k.p, d_v.p, d_a.p, d_b.p, st.ref, d_out.p, T, H, S, nullptr);
    if (!finish(ok)) return false;
    ok = st.fetch(states->state_out) && hipMemcpy(out, d_out.p, n * 4, hipMemcpyDeviceToHost) == hipSuccess;
    RW_CHECK(RWKV_ERROR_GRAPH, false, ok, "HIP error: %s", hipGetErrorString(hipGetLastError()));
    return true;
}

RWKV_API bool rwkv_mi_test_wkv6_seq(const float * r, const float * k, const float * v, const float * u, int u_per_chan, const float * w, int w_mode,
                                    const float * state_in, float * state_out, float * out, int64_t T, int64_t H, int64_t S) {
    g_last_error = RWKV_ERROR_NONE;
    RW_CHECK(RWKV_ERROR_ARGS, false, r && k && v && u && w && state_in && state_out && out && shape_ok(T, H, S) && (u_per_chan == 0 || u_per_chan == 1) &&
             w_mode >= 0 && w_mode <= 2, "bad arguments");
    RW_CHECK(RWKV_ERROR_ARGS, false, S == 64 && T >= k_mfma_min_tokens, "the lane-pipelined sequence form is for head size 64 and at least %d tokens", (int) k_mfma_min_tokens);
    const size_t n = (size_t) (T * H * S), hs = (size_t) (H * S), ns = (size_t) (H * S * S);
    DevBuf<float> d_r, d_k, d_v, d_u, d_w, d_in, d_st, d_out;
    Up up;
    bool ok = up(d_r, r, n) && up(d_k, k, n) && up(d_v, v, n) && up(d_u, u, u_per_chan ? hs : (size_t) H) &&
              up(d_w, w, w_mode == 2 ? n : w_mode == 1 ? hs : (size_t) H) && up(d_in, state_in, ns) && up(d_st, state_out, ns) && up(d_out, out, n);
    ok = ok && launch_wkv6_seq(d_r.p, d_k.p, d_v.p, d_u.p, u_per_chan, d_w.p, w_mode, d_in.p, d_st.p, d_out.p, T, H, nullptr);
    if (!finish(ok)) return false;
    ok = hipMemcpy(state_out, d_st.p, ns * 4, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(out, d_out.p, n * 4, hipMemcpyDeviceToHost) == hipSuccess;
    RW_CHECK(RWKV_ERROR_GRAPH, false, ok, "HIP error: %s", hipGetErrorString(hipGetLastError()));
    return true;
}

RWKV_API bool rwkv_mi_test_wkv7_seq(const float * r, const float * w, const float * k, const float * v, const float * a, const float * b,
                                    const float * state_in, float * state_out, float * out, int64_t T, int64_t H, int64_t S) {
    g_last_error = RWKV_ERROR_NONE;
    RW_CHECK(RWKV_ERROR_ARGS, false, r && w && k && v && a && b && state_in && state_out && out && shape_ok(T, H, S), "bad arguments");
    RW_CHECK(RWKV_ERROR_ARGS, false, S == 64 && T >= k_mfma_min_tokens, "the lane-pipelined sequence form is for head size 64 and at least %d tokens", (int) k_mfma_min_tokens);
    const size_t n = (size_t) (T * H * S), ns = (size_t) (H * S * S);
    DevBuf<float> d_r, d_w, d_k, d_v, d_a, d_b, d_in, d_st, d_out;
    Up up;
    bool ok = up(d_r, r, n) && up(d_w, w, n) && up(d_k, k, n) && up(d_v, v, n) && up(d_a, a, n) && up(d_b, b, n) && up(d_in, state_in, ns) &&
              up(d_st, state_out, ns) && up(d_out, out, n);
    ok = ok && launch_wkv7_seq(d_r.p, d_w.p, d_k.p, d_v.p, d_a.p, d_b.p, d_in.p, d_st.p, d_out.p, T, H, nullptr);
    if (!finish(ok)) return false;
    ok = hipMemcpy(state_out, d_st.p, ns * 4, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(out, d_out.p, n * 4, hipMemcpyDeviceToHost) == hipSuccess;
    RW_CHECK(RWKV_ERROR_GRAPH, false, ok, "HIP error: %s", hipGetErrorString(hipGetLastError()));
    return true;
}

RWKV_API bool rwkv_mi_test_groupnorm(float * x, const float * lw, const float * lb, float eps, const float * gate, const float * v7_k,
                                     const float * v7_r, const float * v7_v, const float * v7_rk, int64_t T, int64_t H, int64_t S) {
    g_last_error = RWKV_ERROR_NONE;
    const bool bonus = v7_k != nullptr;
    RW_CHECK(RWKV_ERROR_ARGS, false, x && lw && lb && shape_ok(T, H, S) && eps > 0.0f && (v7_r != nullptr) == bonus && (v7_v != nullptr) == bonus &&
             (v7_rk != nullptr) == bonus, "bad arguments");
    const size_t n = (size_t) (T * H * S), hs = (size_t) (H * S);
    DevBuf<float> d_x, d_lw, d_lb, d_g, d_k, d_r, d_v, d_rk;
    Up up;
    bool ok = up(d_x, x, n) && up(d_lw, lw, hs) && up(d_lb, lb, hs) && (!gate || up(d_g, gate, n)) &&
              (!bonus || (up(d_k, v7_k, n) && up(d_r, v7_r, n) && up(d_v, v7_v, n) && up(d_rk, v7_rk, hs)));
    if (ok) launch_groupnorm(d_x.p, d_lw.p, d_lb.p, eps, d_g.p, d_k.p, d_r.p, d_v.p, d_rk.p, T, H, S, nullptr);
    if (!finish(ok)) return false;
    ok = hipMemcpy(x, d_x.p, n * 4, hipMemcpyDeviceToHost) == hipSuccess;
    RW_CHECK(RWKV_ERROR_GRAPH, false, ok, "HIP error: %s", hipGetErrorString(hipGetLastError()));
    return true;
}

RWKV_API bool rwkv_mi_test_v7_kprep(const float * k, const float * a, const float * k_k, const float * k_a, float * k_out, float * neg_kk,
                                    float * kk_a, int64_t T, int64_t H, int64_t S) {
    g_last_error = RWKV_ERROR_NONE;
    RW_CHECK(RWKV_ERROR_ARGS, false, k && a && k_k && k_a && k_out && neg_kk && kk_a && shape_ok(T, H, S), "bad arguments");
    const size_t n = (size_t) (T * H * S), hs = (size_t) (H * S);
    DevBuf<float> d_k, d_a, d_kk, d_ka, d_o0, d_o1, d_o2;
    Up up;
    bool ok = up(d_k, k, n) && up(d_a, a, n) && up(d_kk, k_k, hs) && up(d_ka, k_a, hs) && d_o0.alloc(n) == hipSuccess && d_o1.alloc(n) == hipSuccess &&
              d_o2.alloc(n) == hipSuccess;
    if (ok) launch_v7_kprep(d_k.p, d_a.p, d_kk.p, d_ka.p, d_o0.p, d_o1.p, d_o2.p, T, H, S, nullptr);
    if (!finish(ok)) return false;
    ok = hipMemcpy(k_out, d_o0.p, n * 4, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(neg_kk, d_o1.p, n * 4, hipMemcpyDeviceToHost) == hipSuccess &&
         hipMemcpy(kk_a, d_o2.p, n * 4, hipMemcpyDeviceToHost) == hipSuccess;
    RW_CHECK(RWKV_ERROR_GRAPH, false, ok, "HIP error: %s", hipGetErrorString(hipGetLastError()));
    return true;
}

}  // extern "C"
