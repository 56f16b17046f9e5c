// engine.hip -- the hand-scheduled per-layer pipeline that replaces the reference's ggml graphs
// (rwkv_build_serial_graph / rwkv_build_sequential_graph, rwkv_graph.inc:611-866). One code path serves T = 1 (decode)
// and T > 1 (sequence mode); state and weights never leave HBM between calls.
#include "model.h"

#include <condition_variable>
#include <cstdarg>
#include <cstring>
#include <mutex>
#include <thread>

namespace rwkvmi {

void ctx_fail(struct ::rwkv_context * ctx, int flags, const char * file, int line, const char * expr, const char * fmt, ...) {
    ctx->last_error |= flags;
    if (!ctx->print_errors) return;
    if (fmt && fmt[0]) {
        va_list ap;
        va_start(ap, fmt);
        vfprintf(stderr, fmt, ap);
        va_end(ap);
    }
    fprintf(stderr, "\n%s:%d: %s\n", file, line, expr);
}

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ---------------------------------------------------------------------------------------------------------------
// The persistent decode kernel needs every CU of its device at once. Two contexts of one process (rwkv_clone_context: one
// clone per thread, rwkv.h:64-68) launching it concurrently on their own streams could each become half resident and spin
// until both time out. Launches are therefore chained per device: a context's launch waits (on the device, not the host) for
// the completion event of the previous persistent launch of the process. Other processes cannot be seen from here: a poll
// time-out is recovered from by dropping to the per-layer launches (recover_from_abort).
// ---------------------------------------------------------------------------------------------------------------
static constexpr int k_max_devices = 64;
static std::mutex g_mega_mu[k_max_devices + 1];   // per device: a streamed rwkv_eval holds it across its host-blocking slice uploads, other devices go on
static hipEvent_t g_mega_last[k_max_devices] = {};
static rwkv_context * g_mega_last_owner[k_max_devices] = {};
static int g_mega_contexts[k_max_devices] = {};   // contexts of this process holding a persistent kernel, per device

static std::mutex & mega_mu(int dev) { return g_mega_mu[(dev >= 0 && dev < k_max_devices) ? dev : k_max_devices]; }
static int mega_chain_count(rwkv_context * ctx, int delta) {
    const int dev = ctx->model->device;
    std::lock_guard<std::mutex> lk(mega_mu(dev));
    if (dev < 0 || dev >= k_max_devices) return 0;
    return g_mega_contexts[dev] += delta;
}

static void mega_chain_begin(rwkv_context * ctx) {
    const int dev = ctx->model->device;
    mega_mu(dev).lock();
    // (chain_covered: a pipeline hop has already made this stream wait on exactly that launch -- one barrier packet in front of the launch, not two)
    if (dev >= 0 && dev < k_max_devices && g_mega_last[dev] && g_mega_last_owner[dev] != ctx && g_mega_last[dev] != ctx->chain_covered) (void) hipStreamWaitEvent(ctx->stream, g_mega_last[dev], 0);
}
static void mega_chain_end(rwkv_context * ctx) {
    const int dev = ctx->model->device;
    // (a single persistent context per device -- the usual case -- records nothing: no marker between graph replays)
    if (dev >= 0 && dev < k_max_devices && g_mega_contexts[dev] > 1 && ctx->mega_done && hipEventRecord(ctx->mega_done, ctx->stream) == hipSuccess) {
        g_mega_last[dev] = ctx->mega_done; g_mega_last_owner[dev] = ctx;
    }
    mega_mu(dev).unlock();
}
hipEvent_t mega_chain_marker(rwkv_context * ctx) {
    const int dev = ctx->model->device;
    if (dev < 0 || dev >= k_max_devices) return nullptr;
    std::lock_guard<std::mutex> lk(mega_mu(dev));
    return (g_mega_last_owner[dev] == ctx && g_mega_last[dev] == ctx->mega_done) ? ctx->mega_done : nullptr;
}
static void mega_chain_forget(rwkv_context * ctx) {
    const int dev = ctx->model->device;
    std::lock_guard<std::mutex> lk(mega_mu(dev));
    if (dev >= 0 && dev < k_max_devices && g_mega_last_owner[dev] == ctx) {
        if (g_mega_last[dev]) (void) hipEventSynchronize(g_mega_last[dev]);
        g_mega_last[dev] = nullptr; g_mega_last_owner[dev] = nullptr;
    }
}

// what decided a context's single-token path, in words (rwkv_mi_persist_info)
static void note(rwkv_context * ctx, const char * fmt, ...) {
    char buf[320];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    if (!ctx->persist_note.empty()) ctx->persist_note += "; ";
    ctx->persist_note += buf;
}

// Which single-token path is fastest depends on the device: the persistent kernels are bound by cross-XCD hand-over latency, the
// per-layer launches by launch boundaries (RWKV-6, measured: 1.5-1.6 ms vs 2.6 ms per token on most MI355X boxes, but on some boxes
// four of the eight XCDs lag and a chain of all-to-all hand-overs runs at their pace: 3.4 ms vs 2.9 ms). A few eager tokens settle it
// per context at creation: every persistent candidate in cand, then the per-layer launches (fused_v6.hip / fused_v7.hip), 2 warm + 6
// timed tokens each; the fastest stays in ctx->mega, the others are freed. RWKV-6 times on state zeroed once, RWKV-4 / RWKV-7 from a
// fresh state per timing. The state is (re)initialised by every caller afterwards.
static void calibrate_decode_path(rwkv_context * ctx, std::vector<std::unique_ptr<PersistentDecoder>> cand) {
    Model & m = *ctx->model;
    const bool v6 = m.arch_major == 6;
    DevBuf<uint32_t> tok;   // (the calibration's own token words, 256 bytes, in the place of the context's)
    if (tok.alloc(64) != hipSuccess) { ctx->mega = std::move(cand[0]); return; }
    const size_t sbytes = (size_t) m.state_len() * sizeof(float);
    bool ok = hipMemsetAsync(tok.p, 0, 256, ctx->stream) == hipSuccess;
    for (int i = 0; v6 && i < 2; i++) ok = ok && hipMemsetAsync(ctx->state[i].p, 0, sbytes, ctx->stream) == hipSuccess;
    std::swap(ctx->d_tokens, tok);
    // (with logits: a kernel that folds ln_out + head runs them inside its launch, the other paths as launches of their own -- part of what is compared)
    auto timed = [&](std::unique_ptr<PersistentDecoder> & h) -> float {
        ctx->mega.swap(h);
        if (!v6) { ctx->cur = 0; ok = ok && state_from_host(ctx, nullptr); }
        for (int i = 0; i < 2 && ok; i++) ok = forward(ctx, 1, m.has_head);
        ok = ok && hipEventRecord(ctx->ev0, ctx->stream) == hipSuccess;
        for (int i = 0; i < 6 && ok; i++) ok = forward(ctx, 1, m.has_head);
        ok = ok && hipEventRecord(ctx->ev1, ctx->stream) == hipSuccess && hipStreamSynchronize(ctx->stream) == hipSuccess;
        float ms = 0.0f;
        ok = ok && hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) == hipSuccess;
        ctx->mega.swap(h);
        return ms;
    };
    // a candidate whose timing failed or whose poll timed out is out: its abort word is cleared and the comparison goes on without it
    auto timed_out = [&](PersistentDecoder & h) {
        const bool bad = !ok || h.ctl.aborted(ctx->stream);
        if (bad) { if (h.ctl.aborted_cached()) (void) h.ctl.clear_abort(ctx->stream); ok = true; }
        return bad;
    };
    std::unique_ptr<PersistentDecoder> launches;   // (no persistent kernel: the per-layer launches)
    std::vector<float> t(cand.size(), 1e30f);
    std::vector<char> bad(cand.size(), 0);
    size_t best = 0;
    for (size_t i = 0; i < cand.size(); i++) {
        t[i] = timed(cand[i]);
        bad[i] = timed_out(*cand[i]);
        if (bad[i]) t[i] = 1e30f;
        if (t[i] < t[best]) best = i;
    }
    float t_fused = timed(launches);
    // RWKV-4 / RWKV-7: six tokens each on a device that may be busy: a margin under 10 % is timed once more and the smaller figures decide (the
    // choice is kept for every later context of the model)
    if (!v6 && !bad[best] && ok && fabsf(t_fused - t[best]) < 0.10f * t[best]) {
        const float p2 = timed(cand[best]);
        if (timed_out(*cand[best])) { bad[best] = 1; t[best] = 1e30f; }
        else { t[best] = p2 < t[best] ? p2 : t[best]; const float f2 = timed(launches); t_fused = f2 < t_fused ? f2 : t_fused; }
    }
    (void) hipStreamSynchronize(ctx->stream);
    std::swap(ctx->d_tokens, tok);
    ctx->cur = 0;
    ctx->last_error = 0;
    tok.reset();
    const bool keep = ok && !bad[best] && !(t_fused < 0.97f * t[best]);
    for (size_t i = 0; i < cand.size(); i++) if (bad[i]) note(ctx, "calibration: the %s kernel timed out (not every workgroup resident)", decode_path_name(cand[i]->kind()));
    if (!bad[best]) note(ctx, "calibration: %s %.3f ms / token against %.3f ms for the per-layer launches: %s", decode_path_name(cand[best]->kind()), t[best] / 6.0f, t_fused / 6.0f, keep ? "kept" : "dropped");
    if (ok) m.decode_choice.store(keep ? cand[best]->kind() : DecodePath::Launches);
    if (keep) ctx->mega = std::move(cand[best]);
    else { mega_chain_forget(ctx); mega_chain_count(ctx, -1); }
}

// The persistent kernel a new context of m starts from (nullptr: none qualifies). known: what an earlier context of the model measured.
// RWKV-6, nothing measured yet: RWKV_MI_PERSIST = ring | regs names the kernel; by default the LDS-DMA ring, else the register prefetch.
static PersistentDecoder * create_decoder(const Model & m, DecodePath known) {
    if (m.arch_major != 6) return p47_create(m);
    if (known == DecodePath::Regs) return mega_v6_create(m);
    if (known == DecodePath::Ring) return ring_v6_create(m);
    const char * pk = getenv("RWKV_MI_PERSIST");
    const bool want_ring = !(pk && strcmp(pk, "regs") == 0), want_regs = !(pk && strcmp(pk, "ring") == 0);
    if (want_ring) { PersistentDecoder * r = ring_v6_create(m); if (r || !want_regs) return r; }
    return mega_v6_create(m);
}

// After a poll time-out of the persistent kernel (the device was shared): the stream is drained, the abort word cleared, the
// persistent path and the captured graphs dropped; the context continues on the per-layer launches. The state buffer the failed
// step READ is intact (the kernel only writes the other one): the caller may flip `cur` back and repeat the step.
void recover_from_abort(rwkv_context * ctx) {
    if (!ctx->mega) return;
    note(ctx, "a poll of the %s kernel timed out at run time (not every workgroup resident: is the GPU shared?): fell back to the per-layer launches", decode_path_name(ctx->mega->kind()));
    (void) hipStreamSynchronize(ctx->stream);
    (void) ctx->mega->ctl.clear_abort(ctx->stream);
    mega_chain_forget(ctx);
    mega_chain_count(ctx, -1);
    ctx->mega.reset();
    drop_graphs(ctx);
}

rwkv_context * create_context(Model * m, uint32_t n_threads) {
    std::unique_ptr<rwkv_context> ctx(new (std::nothrow) rwkv_context());
    if (!ctx) {
        // a model that no context references yet (rwkv_init_from_file / rwkv_mi_init_stage) would be orphaned
        if (m->refcount.load() == 0) { m->refcount++; release_model(m); }
        global_fail(RWKV_ERROR_CTX | RWKV_ERROR_ALLOC, __FILE__, __LINE__, "ctx != nullptr", "Failed to allocate rwkv_context");
        return nullptr;
    }
    ctx->model = m;
    ctx->n_threads = n_threads;
    ctx->draw.init(1, (size_t) m->n_vocab());
    m->refcount++;
    auto fail = [&](hipError_t e) {
        global_fail(RWKV_ERROR_CTX | RWKV_ERROR_ALLOC, __FILE__, __LINE__, "hip allocation", "HIP error: %s", hipGetErrorString(e));
        destroy_context(ctx.release());
        return (rwkv_context *) nullptr;
    };
    hipError_t e;
    if ((e = hipSetDevice(m->device)) != hipSuccess) return fail(e);
    if ((e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess) return fail(e);
    for (int i = 0; i < 2; i++) if ((e = ctx->state[i].alloc((size_t) m->state_len())) != hipSuccess) return fail(e);
    if ((e = ctx->d_logits.alloc((size_t) m->n_vocab())) != hipSuccess) return fail(e);
    if ((e = ctx->d_next_token.alloc(16)) != hipSuccess) return fail(e);   // (64 bytes)
    if ((e = hipEventCreate(&ctx->ev0)) != hipSuccess) return fail(e);
    if ((e = hipEventCreate(&ctx->ev1)) != hipSuccess) return fail(e);
    if ((e = hipEventCreateWithFlags(&ctx->mega_done, hipEventDisableTiming)) != hipSuccess) return fail(e);
    prefill_prepare_current_device();   // dynamic-LDS limits of the sequence-mode kernels: per device
    const char * g = getenv("RWKV_MI_NO_GRAPH");
    ctx->use_graph = !(g && g[0] == '1');
    const char * nf = getenv("RWKV_MI_NO_FUSED");
    if (!(nf && nf[0] == '1')) {
        size_t bytes = 0;
        if (fused_v6_supported(*m)) { ctx->fused = FusedLayer::v6; bytes = fused_v6_scratch_bytes(*m); }
        else if (fused_v7_supported(*m)) { ctx->fused = FusedLayer::v7; bytes = fused_v7_scratch_bytes(*m); }
        else if (fused_v4_supported(*m)) { ctx->fused = FusedLayer::v4; bytes = fused_v4_scratch_bytes(*m); }
        if (ctx->fused != FusedLayer::none && (e = ctx->fused_scratch.alloc(bytes)) != hipSuccess) return fail(e);
    }
    if (ctx->fused != FusedLayer::none) {
        // one persistent launch per token where the model and the device have a variant; the fused launches stay as the fall-back
        const char * nm = getenv("RWKV_MI_NO_MEGA"), * na = getenv("RWKV_MI_NO_AUTOTUNE"), * pk = getenv("RWKV_MI_PERSIST");
        const DecodePath known = m->decode_choice.load();      // (what an earlier context of this model measured)
        std::vector<std::unique_ptr<PersistentDecoder>> cand;   // the persistent candidates, in the order they are timed
        if (!(nm && nm[0] == '1') && known != DecodePath::Launches) if (PersistentDecoder * h = create_decoder(*m, known)) cand.emplace_back(h);
        if (nm && nm[0] == '1') note(ctx.get(), "RWKV_MI_NO_MEGA=1");
        else if (known == DecodePath::Launches) note(ctx.get(), "an earlier context of this model measured the per-layer launches faster");
        else if (cand.empty()) { const char * why = persist_unavailable_reason(*m); note(ctx.get(), "%s", why ? why : "the persistent kernel could not be built (device memory?)"); }
        // a second persistent context on this device: launches the first one made while it was alone carry no completion event
        if (!cand.empty() && mega_chain_count(ctx.get(), +1) > 1) (void) hipDeviceSynchronize();
        if (!cand.empty() && known == DecodePath::Unmeasured && !(na && na[0] == '1')) {
            // (the register-prefetch kernel beside the ring only where it has been seen within 2 % of it: D = 2048 -- profiles/r04y_prefill_1b6_q4_0_kernel_stats.csv
            //  calibration rows, 710 vs 726 us; at D = 4096 / 2560 the ring wins by 10 % and more and timing a third path cost every context
            //  creation ~15 ms. RWKV_MI_PERSIST=regs still names it.)
            if (!(pk && pk[0]) && cand[0]->kind() == DecodePath::Ring && m->n_embed() == 2048) if (PersistentDecoder * h = mega_v6_create(*m)) cand.emplace_back(h);
            calibrate_decode_path(ctx.get(), std::move(cand));
        } else if (!cand.empty()) ctx->mega = std::move(cand[0]);
    }
    if (ctx->fused == FusedLayer::none) { const char * why = persist_unavailable_reason(*m); note(ctx.get(), "%s", (nf && nf[0] == '1') ? "RWKV_MI_NO_FUSED=1" : (why ? why : "no fused layer for this model")); }
    // A new context starts from the reference's fresh state (rwkv_eval.inc:224-241), whatever the calibration left behind:
    // rwkv_mi_eval_resident / rwkv_mi_decode_greedy / rwkv_mi_stage_step continue from the resident state without a load.
    ctx->cur = 0;
    if (!state_from_host(ctx.get(), nullptr) || (e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return fail(e);
    ctx->last_error = 0;
    return ctx.release();
}

void drop_graphs(rwkv_context * ctx) {
    for (int a = 0; a < 2; a++) for (int b = 0; b < 2; b++) if (ctx->graph_exec[a][b]) { (void) hipGraphExecDestroy(ctx->graph_exec[a][b]); ctx->graph_exec[a][b] = nullptr; }
}

void destroy_context(rwkv_context * ctx) {
    if (!ctx) return;
    if (ctx->stream) (void) hipStreamSynchronize(ctx->stream);
    if (ctx->abi_streamer) { abi_streamer_free(ctx->abi_streamer); ctx->abi_streamer = nullptr; }
    drop_graphs(ctx);
    if (ctx->mega) { mega_chain_forget(ctx); mega_chain_count(ctx, -1); ctx->mega.reset(); }
    if (ctx->mega_done) (void) hipEventDestroy(ctx->mega_done);
    if (ctx->ev0) (void) hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void) hipEventDestroy(ctx->ev1);
    for (hipEvent_t e : ctx->prof.events) (void) hipEventDestroy(e);
    Model * m = ctx->model;
    hipStream_t st = ctx->owns_stream ? ctx->stream : nullptr;
    // The context's buffers are its members and go here: after the drain above, before its stream is destroyed and before the model's last
    // reference can free the arena.
    delete ctx;
    if (st) { matvec_f_release_stream(st); (void) hipStreamDestroy(st); }
    release_model(m);
}

// Scratch for T tokens: one allocation carved into named activations.
bool ensure_scratch(rwkv_context * ctx, int64_t T) {
    if (T <= ctx->scratch_T) return true;
    Model & m = *ctx->model;
    const size_t D = (size_t) m.n_embed(), F = (size_t) m.ffn_size;
    const size_t LR = (size_t)(m.max_lowrank > 0 ? m.max_lowrank : 32);
    const size_t KQ = D > F ? D : F;  // widest quantised activation row
    auto fsz = [&](size_t n) { return align_up((size_t) T * n * sizeof(float), 256); };
    const size_t n_D = 3 + 6 + 6 + 3 + 1 + 1;  // x xn sx | m[6] | r k v g w a | t0 t1 t2 | out | v_first
    size_t total = n_D * fsz(D) + fsz(F) + 2 * fsz(LR) + align_up(D * sizeof(float), 256);
    total += align_up((size_t) T * KQ, 256) + 3 * align_up((size_t) T * (KQ / 32) * 4, 256);
    constexpr size_t k_ws_part = (size_t) 16 << 20;   // split-walk partial sums: up to 64 tiles x 8 parts x 32 KiB
    constexpr int    k_ws_counters = 1024;
    if (T >= k_mfma_min_tokens) total += align_up(tile_act_bytes(T, (int64_t) KQ), 256) + 5 * align_up(tile_act_bytes(T, (int64_t) D), 256) + k_ws_part + k_ws_counters * sizeof(int);
    // (the old scratch goes BEFORE the new one is allocated, unlike every grow(): it is the context's largest buffer)
    if (ctx->scratch) { HIP_CTX_OK(ctx, hipStreamSynchronize(ctx->stream)); ctx->scratch.reset(); ctx->scratch_T = 0; }
    drop_graphs(ctx);
    HIP_CTX_OK(ctx, ctx->scratch.alloc(total));
    uint8_t * p = ctx->scratch.p;
    auto takef = [&](size_t n) { float * r = (float *) p; p += fsz(n); return r; };
    auto & b = ctx->b;
    b.x = takef(D); b.xn = takef(D); b.sx = takef(D);
    for (int i = 0; i < 6; i++) b.m[i] = takef(D);
    b.r = takef(D); b.k = takef(D); b.v = takef(D); b.g = takef(D); b.w = takef(D); b.a = takef(D);
    b.t0 = takef(D); b.t1 = takef(D); b.t2 = takef(D); b.out = takef(D); b.v_first = takef(D);
    b.ffk = takef(F); b.lr1 = takef(LR); b.lr2 = takef(LR);
    b.xlast = (float *) p; p += align_up(D * sizeof(float), 256);
    b.qa.q = (int8_t *) p; p += align_up((size_t) T * KQ, 256);
    b.qa.d = (float *) p; p += align_up((size_t) T * (KQ / 32) * 4, 256);
    b.qa.s = (float *) p; p += align_up((size_t) T * (KQ / 32) * 4, 256);
    b.qa.isum = (int *) p; p += align_up((size_t) T * (KQ / 32) * 4, 256);
    b.tile = nullptr;
    b.ws = MmqWs();
    for (int i = 0; i < 5; i++) b.tiles[i] = nullptr;
    if (T >= k_mfma_min_tokens) {
        b.tile = p; p += align_up(tile_act_bytes(T, (int64_t) KQ), 256);
        for (int i = 0; i < 5; i++) { b.tiles[i] = p; p += align_up(tile_act_bytes(T, (int64_t) D), 256); }
        b.ws.part = (float *) p; b.ws.part_bytes = k_ws_part; p += k_ws_part;
        b.ws.counters = (int *) p; b.ws.n_counters = k_ws_counters; p += k_ws_counters * sizeof(int);
        HIP_CTX_OK(ctx, hipMemsetAsync(b.ws.counters, 0, k_ws_counters * sizeof(int), ctx->stream));
    }
    ctx->scratch_T = T;
    return true;
}

// Scoring buffers of a context (model.h, ScorePass): everything new is allocated before anything old is released.
bool ensure_score(rwkv_context * ctx, int64_t rows) {
    const size_t V = (size_t) ctx->model->n_vocab();
    int64_t R = ctx->score_R;
    const bool first = !ctx->d_score;
    if (first) {
        R = (int64_t) (((size_t) 64 << 20) / (4 * V));
        R = R < 32 ? 32 : (R > 1024 ? 1024 : R);
        // (read here, once per context: tests force many chunks on small models with it)
        if (const char * v = getenv("RWKV_MI_SCORE_ROWS")) { const long long n = atoll(v); if (n >= 1) R = (int64_t) n; }
    }
    const int64_t cap = rows < 1024 ? 1024 : rows;
    const size_t words = rows > ctx->score_cap ? (size_t) cap : 0;
    hipError_t e = hipSuccess;
    if (words && ctx->score_cap) e = hipStreamSynchronize(ctx->stream);   // (an earlier call's copies may still use the old words)
    if (e != hipSuccess) (void) hipGetLastError();
    else e = grow(want(ctx->d_score, first ? (size_t) R * V : 0), want(ctx->d_score_targets, words), want(ctx->h_score_targets, words),
                  want(ctx->d_score_logprobs, words), want(ctx->d_score_argmax, words));
    RW_CTX_CHECK(ctx, RWKV_ERROR_ALLOC, false, e == hipSuccess, "cannot allocate the scoring buffers (%lld rows of %zu logits): %s", (long long) R, V, hipGetErrorString(e));
    if (first) ctx->score_R = R;
    if (words) ctx->score_cap = cap;
    return true;
}

std::atomic<int> g_test_fail_state_init{0};   // (tests: librwkv_testhooks.so arms it; the next state initialisation fails once)

bool state_from_host(rwkv_context * ctx, const float * state_in) {
    Model & m = *ctx->model;
    if (g_test_fail_state_init.load(std::memory_order_relaxed) > 0 && g_test_fail_state_init.fetch_sub(1) > 0)
        RW_CTX_CHECK(ctx, RWKV_ERROR_GRAPH, false, false, "state initialisation failed (injected by the test hook)");
    float * dst = ctx->state[ctx->cur].p;
    if (state_in) {
        HIP_CTX_OK(ctx, hipMemcpyAsync(dst, state_in, (size_t) m.state_len() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    } else if (m.arch_major >= 5) {
        HIP_CTX_OK(ctx, hipMemsetAsync(dst, 0, (size_t) m.state_len() * sizeof(float), ctx->stream));
    } else {
        launch_fill_state_v4(dst, m.n_layer(), m.n_embed(), ctx->stream);
    }
    return true;
}

bool state_to_host(rwkv_context * ctx, float * state_out) {
    Model & m = *ctx->model;
    HIP_CTX_OK(ctx, hipMemcpyAsync(state_out, ctx->state[ctx->cur].p, (size_t) m.state_len() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    return true;
}

// ---------------------------------------------------------------------------------------------------------------
// layer pipeline
// ---------------------------------------------------------------------------------------------------------------

namespace {

struct Runner {
    rwkv_context * ctx;
    Model & m;
    hipStream_t st;
    int64_t T, D, H, S;
    rwkv_context::Buf & b;

    bool copy_failed = false;   // score mode: a copy of the head's logits could not be enqueued
    bool failed = false;   // a launch of the pass could not be made (allocation failure): its outputs are not valid
    // The state the pass reads / writes: the context's state[cur] -> state[cur ^ 1], or in row mode (batched decode, rwkv_mi_batch_*)
    // state.rows, where row t is its own sequence. Row mode never takes the single-token paths (persistent / fused), T == 1 included.
    // Segment mode (ragged batch pass, seg != nullptr): state.segs / state.seg_of, the T tokens are seg->n runs of consecutive tokens, each
    // run on its own slot. Everything between the recurrences is per token and runs over all T tokens as in sequence mode (the product
    // path is chosen on T); the token-shift mixes take the carry per segment (k_mix_segs), the WKV recurrences run per segment. No
    // single-token path here either.
    StateRef state;
    const SegPass * seg = nullptr;
    const ScorePass * score = nullptr;   // score mode: the head runs on every row of the pass (run_head_score)
    // draft mode (segment mode only; rwkv_mi_batch_eval_draft): every layer stashes the inputs of its recurrences, the head runs on every row
    // into draft->logits_all. Without it no launch of a pass changes.
    const DraftPass * draft = nullptr;
    float * stash_plane(uint32_t layer, int i) const {
        const DraftStash & d = draft->stash;
        return d.base + ((int64_t) (layer - m.layer_begin) * d.planes() + i) * d.plane;
    }
    // after a layer's time mixing, before its channel mixing overwrites b.xn and b.r: the WKV body's inputs in the order of its arguments, then
    // the input of the att token-shift mix
    void stash_att(uint32_t layer) {
        DraftStashSrc s;
        switch (m.arch_major) {
            case 4: s.src[0] = b.k; s.src[1] = b.v; s.src[2] = b.r; s.n = 3; break;
            case 5: s.src[0] = b.r; s.src[1] = b.k; s.src[2] = b.v; s.n = 3; break;
            case 6: s.src[0] = b.r; s.src[1] = b.k; s.src[2] = b.v; s.src[3] = b.w; s.n = 4; break;
            default: s.src[0] = b.r; s.src[1] = b.w; s.src[2] = b.t0; s.src[3] = b.v; s.src[4] = b.t1; s.src[5] = b.t2; s.n = 6; break;
        }
        s.src[s.n++] = b.xn;
        launch_draft_stash(s, stash_plane(layer, 0), draft->stash.plane, st);
    }
    // after the channel mixing: the input of its token-shift mix
    void stash_ffn(uint32_t layer) {
        DraftStashSrc s; s.src[0] = b.xn; s.n = 1;
        launch_draft_stash(s, stash_plane(layer, draft->stash.n_in + 1), draft->stash.plane, st);
    }
    // the WKV state of the segments the _segs kernels run (seg->d_short), at offset so
    StateRef seg_short(int64_t so) const { StateRef s = state.at(so); s.segs = seg->d_short; s.n_segs = seg->n_short; return s; }

    // inputs quantised ahead of their products, several per launch (sequence mode): source pointer -> tile image
    struct Pre { const float * x = nullptr; int wtype = -1; int64_t K = 0; TileAct ta; } pre[5];
    void prequant(int n, const float * const * xs, int64_t K, int wtype) {
        for (auto & e : pre) e = Pre();
        if (!(dtype_quantized(wtype) && T >= k_mfma_min_tokens && b.tiles[0] && K == D && n <= 5)) return;
        TileAct tas[5];
        for (int i = 0; i < n; i++) { tas[i] = tile_act_at(b.tiles[i], T, K); pre[i].x = xs[i]; pre[i].wtype = wtype; pre[i].K = K; pre[i].ta = tas[i]; }
        launch_quantize_act_tiles_batched(n, xs, T, K, wtype, tas, st);
    }
    const TileAct * find_pre(const float * x, int64_t K, int wtype) const {
        for (auto & e : pre) if (e.x == x && e.K == K && e.wtype == wtype) return &e.ta;
        return nullptr;
    }
    void drop_pre() { for (auto & e : pre) e = Pre(); }
    // tile images for n outputs of a fused mix (sequence mode, all consumers quantised with `wtype`): registered like prequant's
    // carries: the kernel that would write them takes x_prev from the row above (k_mix_seq_q) -- it has no segment form
    bool fused_outs(int n, float * const * keys, int wtype, TileAct * tas, bool carries = true) {
        if (state.rows) return false;   // (row mode: the quantising mixes carry across rows; k_mix_rows + prequant instead)
        if (state.segs && carries) return false;   // (segment mode: k_mix_segs + prequant; the per-token quantising kernels stay)
        if (!(dtype_quantized(wtype) && T >= k_mfma_min_tokens && b.tiles[0] && D % 256 == 0 && n <= 5)) return false;
        for (auto & e : pre) e = Pre();
        for (int i = 0; i < n; i++) { tas[i] = tile_act_at(b.tiles[i], T, D); pre[i].x = keys[i]; pre[i].wtype = wtype; pre[i].K = D; pre[i].ta = tas[i]; }
        return true;
    }

    // y_i[T][N] = epi_i(W_i . x_i[T][K]) for up to 4 matrices of one shape: one launch in sequence mode when every input was quantised ahead
    void mm_batch(int n, const DevTensor * const * Ws, const float * const * xs, float * const * ys, const Epi * epis) {
        bool batched = T >= k_mfma_min_tokens && b.tile && !ctx->prof.on;
        TileAct tas[4];
        for (int i = 0; i < n && batched; i++) {
            const TileAct * ta = find_pre(xs[i], Ws[i]->cols(), Ws[i]->type);
            if (!ta || Ws[i]->type != Ws[0]->type || Ws[i]->rows() != Ws[0]->rows() || Ws[i]->cols() != Ws[0]->cols()) batched = false; else tas[i] = *ta;
        }
        if (batched && launch_mmq_mfma_batched(n, Ws, tas, ys, epis, T, Ws[0]->rows(), &b.ws, st)) return;
        for (int i = 0; i < n; i++) mm(Ws[i], xs[i], ys[i], epis[i]);
    }

    // y[T][N] = epi(W . x[T][K])    (ggml_mul_mat)
    void mm(const DevTensor * W, const float * x, float * y, const Epi & epi = Epi()) {
        const int64_t N = W->rows(), K = W->cols();
        // (also for the narrow / short low-rank matrices of RWKV-6: routing those to the token-tiled kernel was measured -- 33.6 instead of
        //  23.6 ms per 1024-token pass)
        if (dtype_quantized(W->type) && T >= k_mfma_min_tokens && b.tile) {
            // sequence mode: int8 GEMM on the matrix cores (prefill.hip), bit-identical to the single-token kernel per (row, token)
            TileAct ta;
            if (const TileAct * p = find_pre(x, K, W->type)) ta = *p;
            else { ta = tile_act_at(b.tile, T, K); launch_quantize_act_tiles(x, T, K, W->type, ta, st); }
            auto & pf = ctx->prof;
            if (pf.on) {   // live per-launch timing of the GEMM (rwkv_mi_profile_prefill): `bytes` carries the launch's integer operations
                if (pf.used * 2 + 2 > pf.events.size()) {
                    hipEvent_t a = nullptr, c = nullptr;
                    (void) hipEventCreate(&a); (void) hipEventCreate(&c);
                    pf.events.push_back(a); pf.events.push_back(c); pf.bytes.push_back(0);
                }
                pf.bytes[pf.used] = 2ull * (uint64_t) T * (uint64_t) N * (uint64_t) K;
                (void) hipEventRecord(pf.events[pf.used * 2], st);
            }
            // (the tile-major weight image or the walk table could not be allocated: the product was NOT computed -- the pass fails,
            //  forward() reports it; the f32 activations may not even exist here when the mix wrote tile images only)
            if (!launch_mmq_mfma(*W, ta, T, y, N, epi, st, &b.ws)) { ctx->last_error |= RWKV_ERROR_GRAPH | RWKV_ERROR_ALLOC; failed = true; }
            if (pf.on) { (void) hipEventRecord(pf.events[pf.used * 2 + 1], st); pf.used++; }
        } else if (dtype_quantized(W->type)) {
            launch_quantize_act(x, T, K, b.qa, st);
            auto & pf = ctx->prof;
            const bool timed = pf.on && T == 1 && W->type == (int) m.header.data_type;
            if (timed) {
                if (pf.used * 2 + 2 > pf.events.size()) {
                    hipEvent_t a = nullptr, c = nullptr;
                    (void) hipEventCreate(&a); (void) hipEventCreate(&c);
                    pf.events.push_back(a); pf.events.push_back(c); pf.bytes.push_back(0);
                }
                // algorithmic bytes of this launch: the weight rows once + the quantised activation + the outputs
                pf.bytes[pf.used] = W->nbytes + (uint64_t) K + (uint64_t)(K / 32) * 12 + (uint64_t) N * 4;
                (void) hipEventRecord(pf.events[pf.used * 2], st);
            }
            launch_matvec_q(*W, b.qa, T, y, N, epi, st);
            if (timed) { (void) hipEventRecord(pf.events[pf.used * 2 + 1], st); pf.used++; }
        } else {
            launch_matvec_f(*W, x, K, T, y, N, epi, st);
        }
    }
    // group norm (+ gate) of the WKV output and the output projection behind it; sequence mode: the norm writes the projection's quantised
    // input image itself (k_groupnorm_seq_q), the f32 values never leave the chip
    void gn_out(const LayerW & L, float eps, const float * gate) {
        TileAct ta[1]; float * keys[1] = {b.out};
        if (fused_outs(1, keys, L.att_output->type, ta, false) && !ctx->prof.on &&
            launch_groupnorm_seq_q(b.out, f(L.att_ln_x_w), f(L.att_ln_x_b), eps, gate, T, H, S, ta[0], L.att_output->type, st)) {}
        else { drop_pre(); launch_groupnorm(b.out, f(L.att_ln_x_w), f(L.att_ln_x_b), eps, gate, nullptr, nullptr, nullptr, nullptr, T, H, S, st); }
        mm(L.att_output, b.out, b.x, epi(EPI_ADD_RES, nullptr, b.x));
        drop_pre();
    }
    // WKV-5/6: long sequences on the lane-pipelined kernel (one wave per value column), otherwise one wave per head
    // (so: offset of the layer's WKV state in a state buffer)
    void wkv6(const float * r, const float * k, const float * v, const float * u, int u_per_chan, const float * w, int w_mode,
              int64_t so, float * out) {
        if (seg) {
            // segments of at least k_mfma_min_tokens tokens (head size 64): the lane-pipelined kernel on their token range, one launch each;
            // all the others in one launch of the per-head form. Both perform the serial body's statements per token, so they mix freely.
            for (int64_t i = 0; i < seg->n_long; i++) {
                const SegState & g = seg->h_long[i];
                const int64_t o = (int64_t) g.t0 * D;
                launch_wkv6_seq(r + o, k + o, v + o, u, u_per_chan, w_mode == 2 ? w + o : w, w_mode, g.in + so, g.out + so, out + o, g.t1 - g.t0, H, st);
            }
            if (seg->n_short) launch_wkv6(r, k, v, u, u_per_chan, w, w_mode, seg_short(so), out, T, H, S, st);
            return;
        }
        if (!state.rows && S == 64 && T >= k_mfma_min_tokens) launch_wkv6_seq(r, k, v, u, u_per_chan, w, w_mode, state.in + so, state.out + so, out, T, H, st);
        else launch_wkv6(r, k, v, u, u_per_chan, w, w_mode, state.at(so), out, T, H, S, st);
    }
    // token-shift mix whose carry sits at offset co of a state buffer
    void mix(const MixArgs & a, int64_t co) { launch_mix(a, state.at(co), T, D, st); }
    static const float * f(const DevTensor * t) { return (const float *) t->data; }
    static Epi epi(int op, const float * bias = nullptr, const float * res = nullptr, const float * aux = nullptr) {
        Epi e; e.op = op; e.bias = bias; e.res = res; e.aux = aux; return e;
    }

    // channel mixing (rwkv_ffn_v4_v5 :484-511, rwkv_ffn_v6 :513-531, rwkv_ffn_v7 :533-543)
    void ffn(const LayerW & L, int64_t so) {
        launch_layernorm(b.x, T, D, f(L.ln2_w), f(L.ln2_b), b.xn, st);
        MixArgs a; a.xn = b.xn;
        if (m.arch_major <= 5) { a.mode = 0; a.n_out = 2; a.coef[0] = f(L.ffn_time_mix_k); a.coef[1] = f(L.ffn_time_mix_r); }
        else if (m.arch_major == 6) { a.mode = 1; a.n_out = 2; a.coef[0] = f(L.ffn_time_maa_k); a.coef[1] = f(L.ffn_time_maa_r); }
        else { a.mode = 1; a.n_out = 1; a.coef[0] = f(L.ffn_x_k); }
        a.out[0] = b.m[0]; a.out[1] = b.m[1];
        TileAct tas[5];
        if ((m.arch_major == 7 || L.ffn_receptance->type == L.ffn_key->type) && L.ffn_key->cols() == D && fused_outs(a.n_out, a.out, L.ffn_key->type, tas)) {
            // sequence mode: the mix writes its outputs (RWKV-7: its one output) as quantised tile images (their only consumers are the products below)
            a.out[0] = nullptr; a.out[1] = nullptr; a.carry_in = state.in + so; a.carry_out = state.out + so;
            launch_mix_seq_q(a, T, D, st, tas, L.ffn_key->type);
        } else {
            mix(a, so);
            if (m.arch_major != 7) { const float * xs[2] = {b.m[0], b.m[1]}; prequant(2, xs, D, L.ffn_key->type); }
        }
        // Sequence mode, exact arm: the key product's only consumer is the value product, so its epilogue writes relu(k)^2 straight as that
        // product's quantised input image (prefill.hip MmqQOut) -- b.ffk is never written, its quantiser launch is gone. Needs the key
        // product's own input quantised ahead (its image then is not b.tile, which receives the output).
        TileAct fk; bool fkq = false;
        if (T >= k_mfma_min_tokens && b.tile && !ctx->prof.on && dtype_quantized(L.ffn_key->type) && dtype_quantized(L.ffn_value->type)) {
            // (the receptance product runs between the two: its input must be quantised ahead as well, or it would be quantised into b.tile)
            const bool rec_ok = m.arch_major == 7 || find_pre(b.m[1], L.ffn_receptance->cols(), L.ffn_receptance->type) != nullptr;
            if (const TileAct * in = rec_ok ? find_pre(b.m[0], L.ffn_key->cols(), L.ffn_key->type) : nullptr) {
                fk = tile_act_at(b.tile, T, L.ffn_key->rows());
                fkq = launch_mmq_mfma_q(*L.ffn_key, *in, T, epi(EPI_RELU_SQ), fk, L.ffn_value->type, st);
            }
        }
        if (!fkq) mm(L.ffn_key, b.m[0], b.ffk, epi(EPI_RELU_SQ));
        if (m.arch_major != 7) mm(L.ffn_receptance, b.m[1], b.r);
        drop_pre();
        if (fkq) { pre[0].x = b.ffk; pre[0].wtype = L.ffn_value->type; pre[0].K = L.ffn_value->cols(); pre[0].ta = fk; }
        if (m.arch_major == 7) mm(L.ffn_value, b.ffk, b.x, epi(EPI_ADD_RES, nullptr, b.x));
        else mm(L.ffn_value, b.ffk, b.x, epi(EPI_SIGMUL_ADD_RES, nullptr, b.x, b.r));
        drop_pre();
    }

    // rwkv_att_v4 (:163-197)
    void att_v4(const LayerW & L, int64_t so) {
        launch_layernorm(b.x, T, D, f(L.ln1_w), f(L.ln1_b), b.xn, st);
        MixArgs a; a.xn = b.xn; a.mode = 0; a.n_out = 3;
        a.coef[0] = f(L.att_time_mix_k); a.coef[1] = f(L.att_time_mix_v); a.coef[2] = f(L.att_time_mix_r);
        a.out[0] = b.m[0]; a.out[1] = b.m[1]; a.out[2] = b.m[2];
        mix(a, so + D);
        mm(L.att_receptance, b.m[2], b.r, epi(EPI_SIGMOID));
        mm(L.att_key, b.m[0], b.k);
        mm(L.att_value, b.m[1], b.v);
        launch_wkv4(b.k, b.v, b.r, f(L.att_time_first), f(L.att_time_decay), seg ? seg_short(so + 2 * D) : state.at(so + 2 * D), b.out, T, D, st);
        mm(L.att_output, b.out, b.x, epi(EPI_ADD_RES, nullptr, b.x));
    }

    // rwkv_att_v5 (:199-292)
    void att_v5(const LayerW & L, int64_t so) {
        const bool v52 = m.arch_minor >= 2;
        launch_layernorm(b.x, T, D, f(L.ln1_w), f(L.ln1_b), b.xn, st);
        MixArgs a; a.xn = b.xn; a.mode = 0; a.n_out = v52 ? 4 : 3;
        a.coef[0] = f(L.att_time_mix_k); a.coef[1] = f(L.att_time_mix_v); a.coef[2] = f(L.att_time_mix_r);
        if (v52) a.coef[3] = f(L.att_time_mix_g);
        for (int i = 0; i < 4; i++) a.out[i] = b.m[i];
        mix(a, so + D);
        mm(L.att_receptance, b.m[2], b.r);
        mm(L.att_key, b.m[0], b.k);
        mm(L.att_value, b.m[1], b.v);
        if (v52) mm(L.att_gate, b.m[3], b.g, epi(EPI_SILU));
        wkv6(b.r, b.k, b.v, v52 ? f(L.att_time_faaaa) : f(L.att_time_first), v52 ? 1 : 0, f(L.att_time_decay), v52 ? 1 : 0,
             so + 2 * D, b.out);
        gn_out(L, 1e-5f, v52 ? b.g : nullptr);
    }

    // rwkv_att_v6 (:294-385)
    void att_v6(const LayerW & L, int64_t so) {
        launch_layernorm(b.x, T, D, f(L.ln1_w), f(L.ln1_b), b.xn, st);
        MixArgs a; a.xn = b.xn; a.mode = 1; a.n_out = 1;
        a.coef[0] = f(L.att_time_maa_x); a.out[0] = b.m[5]; a.sx = b.sx;
        {
            // sequence mode: the mix's only consumer is the W1 product -- it writes that product's quantised input image (and sx, which the
            // five mixes read) instead of f32 values for a quantiser launch
            TileAct ta[1];
            if (fused_outs(1, a.out, L.att_time_maa_w1->type, ta) && getenv("RWKV_MI_NO_MIX_QUANT") == nullptr) {
                MixArgs q = a; q.out[0] = nullptr; q.carry_in = state.in + so + D; q.carry_out = state.out + so + D;
                if (!launch_mix_seq_q(q, T, D, st, ta, L.att_time_maa_w1->type)) { drop_pre(); mix(a, so + D); }
            } else { drop_pre(); mix(a, so + D); }
        }
        const int64_t R5 = L.att_time_maa_w1->ne[1], R = R5 / 5;
        mm(L.att_time_maa_w1, b.m[5], b.lr1, epi(EPI_TANH));
        drop_pre();
        V6Mix2Args v; v.w2 = f(L.att_time_maa_w2); v.tl = b.lr1; v.sx = b.sx; v.xn = b.xn;
        v.maa[0] = f(L.att_time_maa_w); v.maa[1] = f(L.att_time_maa_k); v.maa[2] = f(L.att_time_maa_v);
        v.maa[3] = f(L.att_time_maa_r); v.maa[4] = f(L.att_time_maa_g);
        for (int i = 0; i < 5; i++) v.out[i] = b.m[i];  // xw, xk, xv, xr, xg
        bool fused_q = false;
        {
            const int wt = L.att_receptance->type;
            TileAct tas[5];
            if (L.att_key->type == wt && L.att_value->type == wt && L.att_gate->type == wt && L.att_time_decay_w1->type == wt &&
                (R == 32 || R == 64) && fused_outs(5, v.out, wt, tas, false)) {
                // sequence mode: the five mixed inputs leave the kernel as quantised tile images (their only consumers are products)
                for (int i = 0; i < 5; i++) v.out[i] = nullptr;
                fused_q = launch_v6_mix2_seq(v, T, D, R, st, tas, wt);
                if (!fused_q) { drop_pre(); for (int i = 0; i < 5; i++) v.out[i] = b.m[i]; }
            }
        }
        if (!fused_q && !(T >= k_mfma_min_tokens && launch_v6_mix2_seq(v, T, D, R, st))) launch_v6_mix2(v, T, D, R, st);
        {
            // the five mixed inputs are quantised by one launch, the four D x D projections run as one launch (sequence mode)
            const float * xs[5] = {b.m[3], b.m[1], b.m[2], b.m[4], b.m[0]};
            if (!fused_q) prequant(5, xs, D, L.att_receptance->type);
            const DevTensor * Ws[4] = {L.att_receptance, L.att_key, L.att_value, L.att_gate};
            float * ys[4] = {b.r, b.k, b.v, b.g};
            const Epi es[4] = {Epi(), Epi(), Epi(), epi(EPI_SILU)};
            mm_batch(4, Ws, xs, ys, es);
        }
        mm(L.att_time_decay_w1, b.m[0], b.lr2, epi(EPI_TANH));
        drop_pre();
        // decay_w2 consumes [T][DR] rows of lr2
        mm(L.att_time_decay_w2, b.lr2, b.w, epi(EPI_V6_DECAY, f(L.att_time_decay)));
        wkv6(b.r, b.k, b.v, f(L.att_time_faaaa), 1, b.w, 2, so + 2 * D, b.out);
        gn_out(L, 64e-5f, b.g);
    }

    // rwkv_att_v7 (:387-482)
    void att_v7(const LayerW & L, int layer, int64_t so) {
        launch_layernorm(b.x, T, D, f(L.ln1_w), f(L.ln1_b), b.xn, st);
        MixArgs a; a.xn = b.xn; a.mode = 1; a.n_out = 6;
        for (int i = 0; i < 6; i++) { a.coef[i] = f(L.att_x_rwkvag) + (int64_t) i * D; a.out[i] = b.m[i]; }  // r, w, k, v, a, g
        mix(a, so + D);
        mm(L.att_receptance, b.m[0], b.r);
        mm(L.att_g1, b.m[5], b.lr1, epi(EPI_SIGMOID));
        mm(L.att_g2, b.lr1, b.g);
        mm(L.att_a1, b.m[4], b.lr1);
        mm(L.att_a2, b.lr1, b.a, epi(EPI_BIAS_SIGMOID, f(L.att_a0)));
        mm(L.att_w1, b.m[1], b.lr1, epi(EPI_TANH));
        mm(L.att_w2, b.lr1, b.w, epi(EPI_V7_DECAY, f(L.att_w0)));
        mm(L.att_key, b.m[2], b.k);
        launch_v7_kprep(b.k, b.a, f(L.att_k_k), f(L.att_k_a), b.t0 /* k' */, b.t1 /* -kk */, b.t2 /* kk*a */, T, H, S, st);
        mm(L.att_value, b.m[3], b.v);
        if (layer == 0) {
            launch_copy_f32(b.v_first, b.v, T * D, st);
        } else {
            mm(L.att_v1, b.m[3], b.lr1);
            mm(L.att_v2, b.lr1, b.sx, epi(EPI_BIAS_SIGMOID, f(L.att_v0)));
            launch_v7_vmix(b.v, b.v_first, b.sx, T * D, st);
        }
        static const bool no_seq7 = getenv("RWKV_MI_NO_WKV7_SEQ") != nullptr;   // (measurement aid: the single-token form over the whole sequence)
        if (seg) {
            for (int64_t i = 0; i < seg->n_long; i++) {   // (as wkv6: long segments on the sequence kernel, the rest in one _segs launch)
                const SegState & g = seg->h_long[i];
                const int64_t o = (int64_t) g.t0 * D;
                launch_wkv7_seq(b.r + o, b.w + o, b.t0 + o, b.v + o, b.t1 + o, b.t2 + o, g.in + so + 2 * D, g.out + so + 2 * D, b.out + o, g.t1 - g.t0, H, st);
            }
            if (seg->n_short) launch_wkv7(b.r, b.w, b.t0, b.v, b.t1, b.t2, seg_short(so + 2 * D), b.out, T, H, S, st);
        }
        else if (!state.rows && S == 64 && T >= k_mfma_min_tokens && !no_seq7) launch_wkv7_seq(b.r, b.w, b.t0, b.v, b.t1, b.t2, state.in + so + 2 * D, state.out + so + 2 * D, b.out, T, H, st);
        else launch_wkv7(b.r, b.w, b.t0, b.v, b.t1, b.t2, state.at(so + 2 * D), b.out, T, H, S, st);
        launch_groupnorm(b.out, f(L.att_ln_x_w), f(L.att_ln_x_b), 64e-5f, b.g, b.t0, b.r, b.v, f(L.att_r_k), T, H, S, st);
        mm(L.att_output, b.out, b.x, epi(EPI_ADD_RES, nullptr, b.x));
    }

    void run_embed() {
        if (!state.rows && !seg && T == 1 && ctx->mega && m.has_embed && ctx->mega->folds_embed()) return;   // inside the persistent launch
        if (m.has_embed) launch_embed_ln0(*m.emb, ctx->d_tokens.p, T, D, f(m.ln0_w), f(m.ln0_b), b.x, st);
    }
    // layers [lb, le) of the stage (absolute layer ids); returns true when the launch also produced the logits (ring kernel, last layers)
    bool run_layers(uint32_t lb, uint32_t le, bool want_logits) {
        const float * sin = ctx->state[ctx->cur].p;
        float * sout = ctx->state[ctx->cur ^ 1].p;
        state.in = sin; state.out = sout;
        const int64_t per_layer = m.state_per_layer();
        const bool one = T == 1 && !state.rows && !seg;   // (the single-token paths work on the context's own state)
        if (one && ctx->mega) {
            const bool whole = lb == m.layer_begin && le == m.layer_end;   // (only a whole-stage launch is profiled)
            const bool head_done = want_logits && m.has_head && le == m.layer_end && ctx->mega->folds_head();
            const float * s0 = sin + (int64_t) m.layer_begin * per_layer;
            float * o0 = sout + (int64_t) m.layer_begin * per_layer;
            // (the launch starts from the token id and ends with the argmax where the stage has embedding / head and the kernel folds them)
            const uint32_t * tok = (lb == m.layer_begin && m.has_embed && ctx->mega->folds_embed()) ? ctx->d_tokens.p : nullptr;
            uint32_t * ntok = ctx->ntok_out ? ctx->ntok_out : (tok ? ctx->d_tokens.p : ctx->d_next_token.p);    // the greedy loops read the next token where the embedding reads it
            ctx->mega->forward_range(b.x, b.v_first, s0, o0, st, whole ? &ctx->prof : nullptr, head_done ? ctx->d_logits.p : nullptr, (int) (lb - m.layer_begin), (int) (le - m.layer_begin), tok, ntok);
            return head_done;
        }
        for (uint32_t i = lb; i < le; i++) {
            const LayerW & L = m.layers[i];
            const int64_t so = (int64_t) i * per_layer;
            if (one && ctx->fused == FusedLayer::v6) { fused_v6_layer(m, L, b.x, sin + so, sout + so, ctx->fused_scratch.p, st, &ctx->prof); continue; }
            if (one && ctx->fused == FusedLayer::v4) { fused_v4_layer(m, L, b.x, sin + so, sout + so, ctx->fused_scratch.p, st, &ctx->prof); continue; }
            if (one && ctx->fused == FusedLayer::v7) { fused_v7_layer(m, L, (int) i, b.x, b.v_first, sin + so, sout + so, ctx->fused_scratch.p, st, &ctx->prof); continue; }
            switch (m.arch_major) {
                case 4: att_v4(L, so); break;
                case 5: att_v5(L, so); break;
                case 6: att_v6(L, so); break;
                case 7: att_v7(L, (int) i, so); break;
                default: break;
            }
            if (draft) stash_att(i);
            ffn(L, so);
            if (draft) stash_ffn(i);
        }
        return false;
    }
    // score mode (sequence and segment mode): ln_out and the head on ALL T rows, a chunk of ctx->score_R rows at a time -- the chunk's
    // logits, k_score_rows on them, optionally their copy to the host; the product is chosen on the chunk's row count like row mode's head
    void run_head_score() {
        const int64_t Tall = T, R = ctx->score_R, V = m.n_vocab();
        drop_pre();
        int64_t rows = 0;
        for (int64_t r0 = 0; r0 < Tall; r0 += R) {
            rows = Tall - r0 < R ? Tall - r0 : R;
            launch_layernorm(b.x + r0 * D, rows, D, f(m.ln_out_w), f(m.ln_out_b), b.xn, st);
            T = rows;
            mm(m.head, b.xn, ctx->d_score.p);
            T = Tall;
            launch_score_rows(ctx->d_score.p, rows, (int) V, score->targets ? ctx->d_score_targets.p + r0 : nullptr,
                              score->logprobs ? ctx->d_score_logprobs.p + r0 : nullptr, score->argmax ? ctx->d_score_argmax.p + r0 : nullptr, st);
            if (score->h_logits_all &&
                hipMemcpyAsync(score->h_logits_all + r0 * V, ctx->d_score.p, (size_t) (rows * V) * sizeof(float), hipMemcpyDeviceToHost, st) != hipSuccess) copy_failed = true;
        }
        // the context's own logits are those of the last token, as after a plain pass (the sampler and rwkv_mi_logits_store read them)
        if (score->keep_last &&
            hipMemcpyAsync(ctx->d_logits.p, ctx->d_score.p + (rows - 1) * V, (size_t) V * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) copy_failed = true;
    }
    void run_head() {
        if (score) { run_head_score(); return; }
        if (draft) {
            // draft mode: ln_out on all T rows, one product with T rows into [T][n_vocab] (per row what row mode's head computes)
            drop_pre();
            launch_layernorm(b.x, T, D, f(m.ln_out_w), f(m.ln_out_b), b.xn, st);
            mm(m.head, b.xn, draft->logits_all);
            return;
        }
        if (state.rows) {
            // row mode: every row is the last token of its sequence -- ln_out on all rows, one product with T rows into [T][n_vocab]
            launch_layernorm(b.x, T, D, f(m.ln_out_w), f(m.ln_out_b), b.xn, st);
            mm(m.head, b.xn, ctx->d_logits.p);
            return;
        }
        if (seg) {
            // segment mode: ln_out on the last token of each segment (gathered), one product with seg->n rows into [n][n_vocab]
            launch_layernorm_gather(b.x, seg->d_last, seg->n, D, f(m.ln_out_w), f(m.ln_out_b), b.xn, st);
            const int64_t Tsave = T; T = seg->n;
            mm(m.head, b.xn, ctx->d_logits.p);
            T = Tsave;
            return;
        }
        // ln_out on the last token only, then the head projection (rwkv_graph.inc:704-708, 851-854)
        launch_layernorm(b.x + (T - 1) * D, 1, D, f(m.ln_out_w), f(m.ln_out_b), b.xlast, st);
        const int64_t Tsave = T; T = 1;
        mm(m.head, b.xlast, ctx->d_logits.p);
        T = Tsave;
    }
    void run(bool want_logits) {
        run_embed();
        const bool head_done = run_layers(m.layer_begin, m.layer_end, want_logits);
        if (want_logits && m.has_head && !head_done) run_head();
    }
};

}  // namespace

// Where a single-token step that produces logits has ALSO left their argmax (persist_v47.hip folds it into the launch), or nullptr: the
// greedy loops then need no argmax launch -- and no copy when that is where their next step reads the token.
uint32_t * folded_argmax_target(const rwkv_context * ctx) {
    if (!ctx->mega || !ctx->model->has_head || !ctx->mega->folds_argmax()) return nullptr;
    return (ctx->model->has_embed && ctx->mega->folds_embed()) ? ctx->d_tokens.p : ctx->d_next_token.p;
}

int64_t handoff_len(const Model & m) { return m.arch_major == 7 ? 2 * m.n_embed() : m.n_embed(); }

bool forward(rwkv_context * ctx, int64_t T, bool want_logits, const ScorePass * score) {
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, !score || (T > 1 && ctx->d_score.p), "a scoring pass needs its buffers and at least two tokens");
    if (!ensure_scratch(ctx, T)) return false;
    Model & m = *ctx->model;
    Runner r{ctx, m, ctx->stream, T, m.n_embed(), m.head_count, m.head_size, ctx->b};
    r.score = score;
    const bool chained = T == 1 && ctx->mega;
    if (chained) mega_chain_begin(ctx);
    r.run(want_logits);
    if (chained) mega_chain_end(ctx);
    ctx->cur ^= 1;
    HIP_CTX_OK(ctx, hipGetLastError());
    RW_CTX_CHECK(ctx, RWKV_ERROR_GRAPH | RWKV_ERROR_ALLOC, false, !r.failed, "a sequence-mode product could not be launched (out of device memory for the tile-major weight image?)");
    RW_CTX_CHECK(ctx, RWKV_ERROR_GRAPH, false, !r.copy_failed, "a copy of the scoring pass's logits could not be enqueued");
    return true;
}

// ---------------------------------------------------------------------------------------------------------------
// Batched decode (batch.cpp, rwkv_mi_batch_*). The batch runs on a context of its own (batch_context_create): the model, a stream, scratch,
// token words and a [rows][n_vocab] logits buffer -- no state, no persistent kernel, no fused layers, no graphs. Growing its scratch
// therefore never drops the captured graphs of the caller's context.
// Ordering: the batch takes part in the per-device chain of persistent launches (engine.hip top). It counts as one more member, so a
// persistent context on the device records every launch's completion; each pass first waits on the device's latest persistent launch and
// then leaves its own completion as the event the next persistent launch waits on. A batch pass never runs beside a persistent kernel.
// ---------------------------------------------------------------------------------------------------------------
rwkv_context * batch_context_create(Model * m, int64_t max_rows) {
    rwkv_context * c = new (std::nothrow) rwkv_context();
    if (!c) return nullptr;
    c->model = m;
    m->refcount++;
    c->use_graph = false;
    bool ok = hipSetDevice(m->device) == hipSuccess &&
              hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess &&
              c->d_logits.alloc((size_t) max_rows * (size_t) m->n_vocab()) == hipSuccess &&
              c->d_tokens.alloc((size_t) max_rows) == hipSuccess && c->h_tokens.alloc((size_t) max_rows) == hipSuccess &&
              hipEventCreate(&c->ev0) == hipSuccess && hipEventCreate(&c->ev1) == hipSuccess &&
              hipEventCreateWithFlags(&c->mega_done, hipEventDisableTiming) == hipSuccess;
    if (!ok) { destroy_context(c); return nullptr; }
    prefill_prepare_current_device();
    // (a persistent context already on the device recorded nothing while it was alone: drain it once)
    if (mega_chain_count(c, +1) > 1) (void) hipDeviceSynchronize();
    return c;
}

void batch_context_destroy(rwkv_context * c) {
    if (!c) return;
    (void) hipSetDevice(c->model->device);
    if (c->stream) (void) hipStreamSynchronize(c->stream);
    mega_chain_forget(c);
    mega_chain_count(c, -1);
    destroy_context(c);
}

// What follows the head of a batch pass over the `rows` rows of ctx->d_logits.p (model.h, RowSampler): row r's token goes to ctx->d_tokens.p[r]
// and, with a history, into the step's row of it. Order within a step: the choice, then the report of what it wrote, then the stop test.
void launch_row_sampler(rwkv_context * ctx, const RowSampler & s, int64_t rows) {
    const int n_vocab = (int) ctx->model->n_vocab();
    const float * logits = ctx->d_logits.p;
    uint32_t * tokens = ctx->d_tokens.p;
    if (s.beam) {
        // a step of rwkv_mi_batch_decode_beam: every row's candidates, then each group's selection (which writes the rows' next tokens)
        launch_beam_rows(logits, rows, n_vocab, *s.beam, ctx->stream);
        launch_beam_select(*s.beam, rows / (int64_t) s.beam->width, tokens, s.step, s.used, s.other, ctx->stream);
        return;
    }
    if (const RowServe * sv = s.serve) {
        // a step of rwkv_mi_batch_serve: the family's choice behind the lanes' draw words (no history: the scheduler appends the token to its
        // request's row), then -- rwkv_mi_batch_serve_ex on a reporting batch -- the report of what it wrote, at the request's position (the
        // scheduler is what advances it), then the scheduler, then the admissions it decided
        if (s.form.draw != Draw::none) launch_draw_rows(logits, rows, n_vocab, s.rows, s.form, s.probs, tokens, nullptr, sv->t.draw, ctx->stream);
        else launch_argmax_live(logits, rows, n_vocab, tokens, nullptr, sv->t.draw, ctx->stream);
        if (const RowReport * rp = s.report)
            launch_logprob_rows_serve(logits, rows, n_vocab, tokens, (int) rp->top_n, rp->chosen, rp->ids, rp->vals, sv->t.draw, sv->t.req, sv->t.lens, sv->t.stride,
                                      sv->t.n_requests, ctx->stream);
        launch_serve_rows(sv->t, rows, tokens, s.step, s.used, s.other, ctx->stream);
        launch_serve_reset(sv->t, rows, sv->chunks, s.used, sv->state_len, ctx->stream);
        return;
    }
    if (const RowSession * ss = s.session) {
        // a step of a serve session: the family's choice behind the lanes' draw words, the session's scheduler, the admissions it decided
        const ServeTables & t = ss->s.t;
        if (s.form.draw != Draw::none) launch_draw_rows(logits, rows, n_vocab, s.rows, s.form, s.probs, tokens, nullptr, t.draw, ctx->stream);
        else launch_argmax_live(logits, rows, n_vocab, tokens, nullptr, t.draw, ctx->stream);
        launch_session_rows(ss->s, rows, tokens, s.step, s.used, s.other, ctx->stream);
        launch_serve_reset(t, rows, ss->chunks, s.used, ss->state_len, ctx->stream);
        return;
    }
    const size_t at = (size_t) s.step * (size_t) rows;   // the step's slot of the call's history and report buffers
    uint32_t * hist = s.hist ? s.hist + at : nullptr;
    const uint32_t * live = s.stop ? s.stop->live : nullptr;   // (rwkv_mi_batch_decode_until: everything but the stop test runs behind the live words)
    if (s.form.draw != Draw::none) launch_draw_rows(logits, rows, n_vocab, s.rows, s.form, s.probs, tokens, hist, live, ctx->stream);
    else if (live) launch_argmax_live(logits, rows, n_vocab, tokens, hist, live, ctx->stream);
    else launch_argmax(logits, rows, n_vocab, tokens, hist, ctx->stream);
    if (const RowReport * rp = s.report)
        launch_logprob_rows(logits, rows, n_vocab, tokens, (int) rp->top_n, rp->chosen + at, rp->ids + at * rp->top_n, rp->vals + at * rp->top_n, live, ctx->stream);
    if (s.stop) launch_stop_rows(*s.stop, rows, s.hist, s.step, s.used, s.other, ctx->stream);
}

// One pass of T rows, row t = one token (ctx->d_tokens.p[t]) of the sequence whose state is d_rows[t]. Logits: ctx->d_logits.p[T][n_vocab].
// sample: the T sampler workgroups (sampling.hip, k_draw_rows) follow the head INSIDE the chain bracket. Each of them is 1024 threads,
// a CU's worth of waves, so up to T CUs are taken while they run; the completion event mega_chain_end records is what the device's next
// persistent launch waits on, and with the sampler in front of it that launch still finds every CU free ("a batch pass never runs beside
// a persistent kernel" holds for the sampler too). The greedy loop's argmax stays where it was, after the bracket: batch_loop (batch.cpp) calls
// launch_row_sampler itself behind the pass for that family.
bool forward_rows(rwkv_context * ctx, const RowState * d_rows, int64_t T, bool want_logits, const RowSampler * sample) {
    if (!ensure_scratch(ctx, T)) return false;
    Model & m = *ctx->model;
    Runner r{ctx, m, ctx->stream, T, m.n_embed(), m.head_count, m.head_size, ctx->b};
    r.state.rows = d_rows;
    mega_chain_begin(ctx);
    r.run(want_logits);
    if (sample && want_logits && !r.failed) launch_row_sampler(ctx, *sample, T);
    mega_chain_end(ctx);
    HIP_CTX_OK(ctx, hipGetLastError());
    RW_CTX_CHECK(ctx, RWKV_ERROR_GRAPH | RWKV_ERROR_ALLOC, false, !r.failed, "a batched product could not be launched (out of device memory for the tile-major weight image?)");
    return true;
}

// Which recurrence a segment of `len` tokens of a ragged pass takes: the sequence kernels (k_wkv6_seq / k_wkv7_seq, head size 64) from
// k_mfma_min_tokens tokens on, as sequence mode decides for a whole call; the per-head _segs form otherwise (RWKV-4 always).
bool seg_takes_seq_kernel(const Model & m, int64_t len) {
    static const bool no_seq7 = getenv("RWKV_MI_NO_WKV7_SEQ") != nullptr;
    if (m.arch_major < 5 || m.head_size != 64 || len < k_mfma_min_tokens) return false;
    return !(m.arch_major == 7 && no_seq7);
}

// One ragged pass of T tokens (ctx->d_tokens.p) in p.n segments: segment i = tokens [t0, t1) of the sequence whose state goes
// segs[i].in -> segs[i].out. Logits: ctx->d_logits.p[n][n_vocab], those of each segment's last token. The pass takes the place in the
// per-device chain that forward_rows takes, the sampler included.
bool forward_segs(rwkv_context * ctx, const SegPass & p, int64_t T, bool want_logits, const RowSampler * sample, const ScorePass * score) {
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, !score || (!sample && ctx->d_score.p), "a scoring pass needs its buffers and takes no sampler");
    if (!ensure_scratch(ctx, T)) { (void) hipGetLastError(); ctx->last_error |= RWKV_ERROR_ALLOC; return false; }
    Model & m = *ctx->model;
    Runner r{ctx, m, ctx->stream, T, m.n_embed(), m.head_count, m.head_size, ctx->b};
    r.seg = &p;
    r.score = score;
    r.state.segs = p.d_segs; r.state.n_segs = p.n; r.state.seg_of = p.d_seg_of;
    mega_chain_begin(ctx);
    r.run(want_logits);
    if (sample && want_logits && !r.failed) launch_row_sampler(ctx, *sample, p.n);
    mega_chain_end(ctx);
    HIP_CTX_OK(ctx, hipGetLastError());
    RW_CTX_CHECK(ctx, RWKV_ERROR_GRAPH | RWKV_ERROR_ALLOC, false, !r.failed, "a product of the ragged pass could not be launched (out of device memory for the tile-major weight image?)");
    RW_CTX_CHECK(ctx, RWKV_ERROR_GRAPH, false, !r.copy_failed, "a copy of the scoring pass's logits could not be enqueued");
    return true;
}

// One draft pass (model.h, DraftPass): the ragged pass of forward_segs with the stash and the head on every token, then -- inside the pass's
// place in the per-device chain, as the samplers are -- the choice and the replay.
bool forward_draft(rwkv_context * ctx, const SegPass & p, int64_t T, const DraftPass & d) {
    Model & m = *ctx->model;
    RW_CTX_CHECK(ctx, RWKV_ERROR_ARGS, false, p.n_long == 0 && p.n_short == p.n && d.stash.base && d.logits_all, "a draft pass takes short segments and needs its buffers");
    if (!ensure_scratch(ctx, T)) { (void) hipGetLastError(); ctx->last_error |= RWKV_ERROR_ALLOC; return false; }
    Runner r{ctx, m, ctx->stream, T, m.n_embed(), m.head_count, m.head_size, ctx->b};
    r.seg = &p;
    r.draft = &d;
    r.state.segs = p.d_segs; r.state.n_segs = p.n; r.state.seg_of = p.d_seg_of;
    mega_chain_begin(ctx);
    r.run(true);
    if (!r.failed) {
        launch_draft_accept_rows(d.logits_all, p.n, (int) m.n_vocab(), p.d_segs, ctx->d_tokens.p, d.rows, d.form, d.probs, d.out, d.out_stride, d.keep, ctx->d_logits.p,
                                 ctx->stream);
        launch_draft_replay(d.stash, d.lw, m.arch_major, m.arch_minor, p.d_segs, p.n, d.keep, (int64_t) (m.layer_end - m.layer_begin), m.n_embed(), m.head_count, m.head_size,
                            ctx->stream);
    }
    mega_chain_end(ctx);
    HIP_CTX_OK(ctx, hipGetLastError());
    RW_CTX_CHECK(ctx, RWKV_ERROR_GRAPH | RWKV_ERROR_ALLOC, false, !r.failed, "a product of the draft pass could not be launched (out of device memory for the tile-major weight image?)");
    return true;
}

// ---------------------------------------------------------------------------------------------------------------
// rwkv_eval with the caller's state STREAMED (rwkv_eval.inc:2-22,38-76; rwkv.h:106-108: state_in / state_out are host buffers on
// every call). The plain form is upload (34.6 MB for the 7B) -> token -> download, serial: 2.97 ms per token against 1.54 ms with the
// state resident (round 3: 337 vs 649 tokens/s). Here the token is cut into up to eight layer groups:
//     this thread      for each group: upload its state slice (copy stream), record; the compute stream waits for THAT slice only and
//                      runs the group's layers (the ring kernel on a layer range: one launch per group; the per-layer paths: their
//                      launches), records "group done"
//     download thread  for each group: a second copy stream waits for "group done" and brings the group's new state slice back
// so the PCIe traffic of both directions runs under the layers of other groups; exposed are the first slice's upload, the last
// slice's download and the logits. Nothing is assumed about the caller's memory (pageable copies through the runtime's staging path,
// both directions at once from two threads); state_in == state_out is fine (a slice is read before its group runs, written after).
// The state on the device is complete afterwards (state[cur]): a poll time-out of the persistent kernel falls back as before.
// ---------------------------------------------------------------------------------------------------------------
constexpr int k_abi_max_groups = 32;
struct AbiStreamer {
    hipStream_t up = nullptr, down = nullptr;
    std::vector<hipEvent_t> ev_up, ev_done;
    std::thread worker;
    std::mutex mu;
    std::condition_variable cv;
    // job of the download thread
    int n_groups = 0, published = 0, finished = 0;     // groups of this call / "group done" recorded so far / downloaded so far
    bool quit = false, failed = false;
    int device = 0;
    float * h_out = nullptr; const float * d_out = nullptr;
    std::vector<std::pair<int64_t, int64_t>> slices;    // (offset, count) in floats per group
    uint64_t call = 0, seen = 0;

    void run() {
        (void) hipSetDevice(device);
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            cv.wait(lk, [&] { return quit || call != seen; });
            if (quit) return;
            seen = call;
            int g = 0;
            while (g < n_groups) {
                cv.wait(lk, [&] { return quit || published > g || g >= n_groups; });
                if (quit) return;
                if (g >= n_groups) break;       // (the call failed before this group ran)
                const auto sl = slices[(size_t) g];
                hipEvent_t ev = ev_done[(size_t) g];
                lk.unlock();
                bool ok = hipStreamWaitEvent(down, ev, 0) == hipSuccess &&
                          hipMemcpyAsync(h_out + sl.first, d_out + sl.first, (size_t) sl.second * sizeof(float), hipMemcpyDeviceToHost, down) == hipSuccess &&
                          hipStreamSynchronize(down) == hipSuccess;
                lk.lock();
                if (!ok) failed = true;
                g++;
                finished = g;
                cv.notify_all();
            }
        }
    }
};

void abi_streamer_free(void * p) {
    AbiStreamer * a = (AbiStreamer *) p;
    if (!a) return;
    { std::lock_guard<std::mutex> lk(a->mu); a->quit = true; }
    a->cv.notify_all();
    if (a->worker.joinable()) a->worker.join();
    for (hipEvent_t e : a->ev_up) (void) hipEventDestroy(e);
    for (hipEvent_t e : a->ev_done) (void) hipEventDestroy(e);
    if (a->up) (void) hipStreamDestroy(a->up);
    if (a->down) (void) hipStreamDestroy(a->down);
    delete a;
}

bool forward_streamed_eligible(const rwkv_context * ctx) {
    const char * e = getenv("RWKV_MI_ABI_STREAM");       // 0: off, 1: whatever the size of the state (tests), unset: from 4 MB of state
    if ((e && e[0] == '0') || !ctx->stages.empty() || !ctx->owns_stream) return false;
    const Model & m = *ctx->model;
    if (m.layer_end - m.layer_begin < 2 || !m.has_embed || !m.has_head) return false;
    if (ctx->mega && !ctx->mega->has_range()) return false;     // (the register-prefetch kernel has no layer-range launch)
    if (e && e[0] == '1') return true;
    return (size_t) m.state_len() * sizeof(float) >= ((size_t) 4 << 20);   // small states: the serial copies are already cheap
}

// One token (already in ctx->d_tokens.p) from the caller's state_in (nullptr: the fresh state) into the caller's state_out (nullptr: none).
// On return the streams are drained; *aborted reports a poll time-out of the persistent kernel (the caller repeats the step).
bool forward_streamed(rwkv_context * ctx, bool want_logits, const float * h_in, float * h_out, float * h_logits, bool * aborted) {
    *aborted = false;
    Model & m = *ctx->model;
    if (!ensure_scratch(ctx, 1)) return false;
    AbiStreamer * a = (AbiStreamer *) ctx->abi_streamer;
    if (!a) {
        a = new (std::nothrow) AbiStreamer();
        RW_CTX_CHECK(ctx, RWKV_ERROR_ALLOC, false, a != nullptr, "out of memory");
        a->device = m.device;
        bool ok = hipStreamCreateWithFlags(&a->up, hipStreamNonBlocking) == hipSuccess && hipStreamCreateWithFlags(&a->down, hipStreamNonBlocking) == hipSuccess;
        for (int i = 0; i < k_abi_max_groups && ok; i++) {
            hipEvent_t e1 = nullptr, e2 = nullptr;
            ok = hipEventCreateWithFlags(&e1, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&e2, hipEventDisableTiming) == hipSuccess;
            if (e1) a->ev_up.push_back(e1);
            if (e2) a->ev_done.push_back(e2);
        }
        if (!ok) { abi_streamer_free(a); RW_CTX_CHECK(ctx, RWKV_ERROR_ALLOC, false, false, "cannot create the copy streams of the streamed rwkv_eval"); }
        a->worker = std::thread([a] { a->run(); });
        ctx->abi_streamer = a;
    }
    const uint32_t L = m.layer_end - m.layer_begin;
    // Layer groups. What a call cannot hide is the upload of its FIRST slice and the download of its LAST one, so the groups are small at both
    // ends and grow towards the middle: 1 1 2 4 8 | 8 4 2 1 1 layers for 32 (round 4 cut eight even groups: 4.3 MB exposed at each end of a 7B
    // token, now 1.1 MB; two more launches). RWKV_MI_ABI_GROUPS=even restores the even cut (A/B).
    std::vector<uint32_t> gsz;
    {
        static const bool even = [] { const char * e = getenv("RWKV_MI_ABI_GROUPS"); return e && e[0] == 'e'; }();
        const char * lst = getenv("RWKV_MI_ABI_GROUPS");     // (measurement aid: an explicit list of group sizes, e.g. 1,3,12,12,3,1)
        if (lst && lst[0] >= '0' && lst[0] <= '9') {
            uint32_t sum = 0;
            for (const char * q = lst; *q && (int) gsz.size() < k_abi_max_groups;) { const uint32_t v = (uint32_t) strtoul(q, (char **) &q, 10); if (v == 0) break; gsz.push_back(v); sum += v; if (*q == ',') q++; }
            if (sum != L) gsz.clear();
        }
        if (!gsz.empty()) {}
        else if (even || L < 8) { const uint32_t G0 = L < 8 ? L : 8; for (uint32_t g = 0; g < G0; g++) gsz.push_back((uint32_t) ((uint64_t) L * (g + 1) / G0 - (uint64_t) L * g / G0)); }
        else {
            std::vector<uint32_t> left, right;
            uint32_t rest = L;
            for (uint32_t i = 0, sz = 1; rest > 0; i++) {
                const uint32_t a = sz < rest ? sz : rest; left.push_back(a); rest -= a;
                if (rest > 0) { const uint32_t b = sz < rest ? sz : rest; right.push_back(b); rest -= b; }
                if (i >= 1 && sz < 8) sz *= 2;      // 1 1 2 4 8 8 ...
                if ((int) (left.size() + right.size()) >= k_abi_max_groups - 2 && rest > 0) { left.back() += rest; rest = 0; }
            }
            gsz = left;
            for (size_t i = right.size(); i-- > 0;) gsz.push_back(right[i]);
        }
    }
    const int G = (int) gsz.size();
    const int64_t per = m.state_per_layer();
    float * sin = ctx->state[ctx->cur].p;
    float * sout = ctx->state[ctx->cur ^ 1].p;
    // every fallible step of the set-up comes BEFORE the download job is published: a return between arming the worker and the final wait
    // would leave it inside a stale job holding the caller's pointer (it then finished the NEXT call's groups twice, the second time after
    // that call had returned)
    if (!h_in) { if (!state_from_host(ctx, nullptr)) return false; }
    std::vector<std::pair<uint32_t, uint32_t>> ranges;
    {
        std::lock_guard<std::mutex> lk(a->mu);
        a->slices.clear();
        uint32_t lb = m.layer_begin;
        for (int g = 0; g < G; g++) {
            const uint32_t le = lb + gsz[(size_t) g];
            ranges.push_back({lb, le});
            a->slices.push_back({(int64_t) lb * per, (int64_t) (le - lb) * per});
            lb = le;
        }
        // (the LAST group's slice is brought back by this thread on the compute stream, right behind its layers and in front of the logits: handing
        //  it to the download thread cost a wake-up of that thread and one of this one on the only part of the call nothing overlaps)
        a->n_groups = h_out ? G - 1 : 0; a->published = 0; a->finished = 0; a->failed = false;
        a->h_out = h_out; a->d_out = sout;
        a->call++;
    }
    a->cv.notify_all();
    Runner r{ctx, m, ctx->stream, 1, m.n_embed(), m.head_count, m.head_size, ctx->b};
    r.run_embed();
    const bool chained = ctx->mega != nullptr;
    if (chained) mega_chain_begin(ctx);
    bool ok = true, head_done = false;
    for (int g = 0; g < G && ok; g++) {
        const auto sl = a->slices[(size_t) g];
        if (h_in) {
            ok = hipMemcpyAsync(sin + sl.first, h_in + sl.first, (size_t) sl.second * sizeof(float), hipMemcpyHostToDevice, a->up) == hipSuccess &&
                 hipEventRecord(a->ev_up[(size_t) g], a->up) == hipSuccess && hipStreamWaitEvent(ctx->stream, a->ev_up[(size_t) g], 0) == hipSuccess;
            if (!ok) break;
        }
        head_done = r.run_layers(ranges[(size_t) g].first, ranges[(size_t) g].second, want_logits) || head_done;
        ok = hipEventRecord(a->ev_done[(size_t) g], ctx->stream) == hipSuccess;
        if (ok && h_out && g + 1 < G) { { std::lock_guard<std::mutex> lk(a->mu); a->published = g + 1; } a->cv.notify_all(); }
    }
    if (ok && h_out) {
        const auto sl = a->slices[(size_t) (G - 1)];
        ok = hipMemcpyAsync(h_out + sl.first, sout + sl.first, (size_t) sl.second * sizeof(float), hipMemcpyDeviceToHost, ctx->stream) == hipSuccess;
    }
    if (chained) mega_chain_end(ctx);
    if (ok && want_logits && !head_done) r.run_head();
    if (ok && h_logits) ok = hipMemcpyAsync(h_logits, ctx->d_logits.p, (size_t) m.n_vocab() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream) == hipSuccess;
    const bool ctl_ok = !ctx->mega || ctx->mega->ctl.fetch(ctx->stream);
    const bool sync_ok = hipStreamSynchronize(ctx->stream) == hipSuccess;
    {   // the download thread must be done with this call whatever happened above (it holds the caller's pointer)
        std::unique_lock<std::mutex> lk(a->mu);
        if (!ok) { a->n_groups = a->published; }     // (groups that never ran are not downloaded)
        a->cv.notify_all();
        a->cv.wait(lk, [&] { return a->finished >= a->n_groups; });
        ok = ok && !a->failed;
    }
    ctx->cur ^= 1;
    RW_CTX_CHECK(ctx, RWKV_ERROR_GRAPH, false, ok && sync_ok, "HIP error in the streamed rwkv_eval: %s", hipGetErrorString(hipGetLastError()));
    RW_CTX_CHECK(ctx, RWKV_ERROR_GRAPH | RWKV_ERROR_ALLOC, false, !r.failed, "a product could not be launched");
    if (ctx->mega && (!ctl_ok || ctx->mega->ctl.aborted_cached())) { recover_from_abort(ctx); *aborted = true; }
    return true;
}

// A single-token step that is ONE persistent launch issued directly (no graph): no embedding launch in front of it (none to do, or folded)
// and no head launches behind it (none wanted, or folded). A whole model additionally folds the argmax (the greedy loops' condition since
// round 5); a pipeline stage qualifies since round 6 -- a chain of N stages paid N replays of a one-node graph per token
// (RWKV_MI_STAGE_GRAPH=1 restores that for A/B). runner.cpp relies on this: only a direct launch sees a changed set_x_out.
bool single_launch_step(const rwkv_context * ctx, bool want_logits) {
    if (!ctx->mega) return false;
    const Model & mm = *ctx->model;
    static const bool replay = getenv("RWKV_MI_STAGE_GRAPH") != nullptr;
    const bool one_launch = (!mm.has_embed || ctx->mega->folds_embed()) && (!(want_logits && mm.has_head) || ctx->mega->folds_head());
    if (!one_launch) return false;
    return (mm.has_embed && mm.has_head) ? ctx->mega->folds_argmax() : !replay;
}

// Single-token step through a captured hipGraph: one graph per (state parity, logits on/off), replayed per token so
// that the ~100 short launches of a decode step cost one graph launch on the host.
bool forward_decode(rwkv_context * ctx, bool want_logits) {
    if (!ctx->use_graph) return forward(ctx, 1, want_logits);
    // one launch per token (persist_v47.hip with embedding, head and argmax inside it): a direct launch from a busy stream costs the host
    // 3 - 5 us, the replay of a one-node graph 10 - 16 (guide row graph-replay-floor) -- at 250 us per token of the 169M that is the gap
    // Round 6: the same holds for every stage of a layer pipeline whose step is ONE persistent launch (single_launch_step below).
    if (single_launch_step(ctx, want_logits)) return forward(ctx, 1, want_logits);
    if (!ensure_scratch(ctx, 1)) return false;
    hipGraphExec_t & ge = ctx->graph_exec[ctx->cur][want_logits ? 1 : 0];
    if (!ge) {
        Model & m = *ctx->model;
        hipGraph_t graph = nullptr;
        HIP_CTX_OK(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
        Runner r{ctx, m, ctx->stream, 1, m.n_embed(), m.head_count, m.head_size, ctx->b};
        r.run(want_logits);
        HIP_CTX_OK(ctx, hipStreamEndCapture(ctx->stream, &graph));
        hipError_t e = hipGraphInstantiate(&ge, graph, nullptr, nullptr, 0);
        (void) hipGraphDestroy(graph);
        RW_CTX_CHECK(ctx, RWKV_ERROR_GRAPH, false, e == hipSuccess, "hipGraphInstantiate failed: %s", hipGetErrorString(e));
    }
    const bool chained = ctx->mega != nullptr;
    if (chained) mega_chain_begin(ctx);
    const hipError_t le = hipGraphLaunch(ge, ctx->stream);
    if (chained) mega_chain_end(ctx);
    HIP_CTX_OK(ctx, le);
    ctx->cur ^= 1;
    return true;
}

}  // namespace rwkvmi
