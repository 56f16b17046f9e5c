// persist_host.h -- the host side the persistent decode kernels share (mega_v6.hip: register prefetch; ring_v6.hip: LDS-DMA weight ring;
// persist_v47.hip: RWKV-4 / RWKV-7): which single-token path a context runs, the per-launch profile, the profiled launch, the control
// words of a launch and the object a context holds. Bodies: persist_host.cpp.
#pragma once

#include <cstdint>
#include <vector>

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "devmem.h"

namespace rwkvmi {

// The single-token path of a stage: what a handle is (Regs / Ring / K47) and what the first context of a model measured as fastest
// (Model::decode_choice; Launches = the fused per-layer launches).
enum class DecodePath : int { Unmeasured, Regs, Ring, K47, Launches };
const char * decode_path_name(DecodePath p);   // "regs" | "ring" | "k47" | "none"

// Live per-launch timing of the dominant kernel (the quantised single-token projection) with HIP events on the context's
// stream; filled by rwkv_mi_profile_decode, used by bench.py's roofline figure.
struct DecodeProf {
    bool on = false;
    std::vector<hipEvent_t> events;  // pairs
    std::vector<uint64_t> bytes;     // per pair
    size_t used = 0;
    double total_ms = 0.0;
    uint64_t launches = 0, total_bytes = 0;
};

// Launch, optionally bracketed by the kernel's own start/stop timestamps (hipExtLaunchKernelGGL events: the dispatch's
// begin/end as the profiler sees them, no host-side event overhead inside the interval). bytes == 0: never bracketed.
template <typename Kern, typename Param>
static void launch_profiled(DecodeProf * pf, uint64_t bytes, Kern kernel, dim3 grid, dim3 block, size_t shmem, hipStream_t st, const Param & prm) {
    if (pf && pf->on && bytes) {
        if (pf->used * 2 + 2 > pf->events.size()) {
            hipEvent_t a = nullptr, c = nullptr;
            (void) hipEventCreate(&a); (void) hipEventCreate(&c);
            pf->events.push_back(a); pf->events.push_back(c); pf->bytes.push_back(0);
        }
        pf->bytes[pf->used] = bytes;
        hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t) shmem, st, pf->events[pf->used * 2], pf->events[pf->used * 2 + 1], 0, prm);
        pf->used++;
    } else {
        hipLaunchKernelGGL(kernel, grid, block, shmem, st, prm);
    }
}

// Control words of a persistent kernel: dev[0] the rolling hand-over generation the next launch starts from, dev[1] the abort word (a
// poll timed out: co-residency lost or a bug; results since then are not valid), dev[2..6] the greedy history {on, position, address
// low / high, capacity}. The abort word is read through a pinned host mirror: an asynchronous copy on the caller's stream, checked after
// the caller's own stream synchronisation. (A blocking hipMemcpy would go through the legacy null stream and couple every blocking
// stream of the process.)
struct PersistCtl {
    DevBuf<unsigned> dev;
    PinBuf<unsigned> host;       // pinned mirror of dev[0..1], refreshed by fetch()

    bool alloc(unsigned generation);   // zeroed words, then {generation, 0} on the device and in the mirror
    bool fetch(hipStream_t st) const;                  // async copy of the control words into the mirror
    bool aborted_cached() const { return host.p[1] != 0; }   // the mirror's abort word (valid after the stream was synchronised)
    bool aborted(hipStream_t st) const;                // fetch + synchronise + check
    unsigned generation(hipStream_t st) const;         // fetch + synchronise; 0 on failure
    // clears the abort word (after the caller has drained the stream), so that the handle -- or the context that drops it -- is usable again
    bool clear_abort(hipStream_t st);
    // Test hook: presets the rolling tag generation (the kernel compares its low 16 bits), e.g. just below a 16-bit wrap.
    bool set_tag(unsigned base, hipStream_t st);
    // Test hook: the abort word set from the host, as a poll that timed out would set it -- the next launch drains at once, the host finds
    // the word behind it and the context falls back to the per-layer launches (engine.hip, recover_from_abort).
    bool force_abort(hipStream_t st);
    // greedy loops: the kernel appends every token it picks to hist (device memory, n entries) from position 0; nullptr switches it off
    bool set_history(uint32_t * hist, size_t n, hipStream_t st);
};

// One persistent launch per token over the layers of a stage; rwkv_context::mega owns one.
struct PersistentDecoder {
    PersistCtl ctl;

    virtual ~PersistentDecoder();
    virtual DecodePath kind() const = 0;
    virtual uint64_t bytes() const = 0;            // algorithmic bytes of one whole-stage launch
    virtual bool has_range() const { return true; }   // forward_range accepts a proper sub-range of the stage
    virtual bool folds_embed() const = 0;          // the launch starts from the token id: the caller skips its embedding + ln0 launch
    virtual bool folds_head() const = 0;           // logits != nullptr: ln_out + the head projection run inside the launch (the caller skips its own)
    virtual bool folds_argmax() const = 0;         // a launch that produces logits also writes their argmax to next_tok
    // (folds_argmax) tokens appended on the device (at most n), no copy per token; false: this kernel keeps no history
    virtual bool set_history(uint32_t * hist, size_t n, hipStream_t st) { return ctl.set_history(hist, n, st); }
    // Pipeline stages: the launch that runs the stage's last layer writes the residual stream to x_out (the NEXT stage's input buffer, on this
    // or on a peer device) instead of back into its own x; nullptr restores the in-place form. false: this kernel has no such output.
    virtual bool set_x_out(float * to) { x_out = to; return true; }
    // Layers [l0, l1) of the stage in one launch (indices into the stage's own layers; the whole stage is [0, its layer count)).
    // sin / sout: state of the stage's FIRST layer. x: the residual stream in plain memory, read by the first and written by the last
    // layer of the launch. tok (only used with l0 == 0 and folds_embed): the launch starts from the token id. logits (only used with
    // l1 == the stage's last layer and folds_head): ln_out + head inside; next_tok: where their argmax lands.
    virtual void forward_range(float * x, float * v_first, const float * sin, float * sout, hipStream_t st, DecodeProf * pf, float * logits, int l0, int l1,
                               const uint32_t * tok, uint32_t * next_tok) = 0;
    // debug: cycle stamps of one layer for the next launches (fetch = false), then their copy into out (fetch = true)
    virtual bool trace(int layer, long long * out, bool fetch) = 0;

protected:
    float * x_out = nullptr;
    DevBuf<long long> trace_buf;
    // the body of trace(): a zeroed buffer of n + extra stamps on first use, bound to the kernel's parameter slots; fetch copies the first
    // n out (extra: the ring loader's samples, dumped raw to the file RWKV_MI_RING_LTRACE names)
    bool trace_into(long long *& slot, int & slot_layer, int layer, size_t n, size_t extra, long long * out, bool fetch);
};

// ---- what the creators of the persistent kernels share (bodies: persist_host.cpp) ----

struct Model;

// The per-layer table of the RWKV-6 kernels (persist.h says why offsets): byte offsets from the parameter arena, three planes per matrix.
struct M6Off { long long qs, qh, sc; };
struct M6Layer {
    long long ln1_w, ln1_b, maa_x, maa[5], w2b /* floats into M6P::w2b */, time_decay, faaaa, lnx_w, lnx_b, ln2_w, ln2_b, fmaa_k, fmaa_r;
    M6Off w1, rkvg[4], dw1, dw2, wo, fk, fr, fv;
};

// Offsets of a model's parameters from its arena. in_arena is sticky: false once an address was null or outside the arena (the kernels
// address every weight as arena + offset, so such a model does not qualify).
struct ArenaOffsets {
    const unsigned char * base;
    uint64_t bytes;
    bool in_arena = true;
    explicit ArenaOffsets(const Model & m);
    long long off(const void * ptr);
    long long f(const DevTensor * t) { return off(t->data); }                  // a tensor the architecture always has
    long long f_opt(const DevTensor * t) { return t ? off(t->data) : 0; }      // one a layer may lack (persist_v47.hip): offset 0, no failure
    M6Off pl3(const DevTensor * t);                                            // the planes of a quantised matrix
};

// What both RWKV-6 kernels ask of a stage before their own geometry test: RWKV-6 with 64-wide heads, a non-empty layer range, the eleven
// matrices of every layer present and of the file's one format, F / DR / R5 the same in every layer. false: no persistent RWKV-6 kernel.
struct V6Shape { int64_t D, F, DR, R5, R, H; int fmt; };
bool v6_stage_shape(const Model & m, V6Shape & s);

// The layer table of the stage (layer i's blocked W2 at i * w2_layer floats), the algorithmic bytes of one launch over it -- every layer
// tensor once + the recurrent state read and written -- and whether every address was inside the arena.
struct V6Table { std::vector<M6Layer> layers; uint64_t bytes = 0; bool in_arena = true; };
V6Table v6_layer_table(const Model & m, size_t w2_layer);

// W2 ([5][R][D] floats) into the chunk-blocked layout both RWKV-6 kernels read, on the null stream (the kernel: mega_v6.hip, k_block_w2)
void launch_block_w2(const float * src, float * dst, int D, int R);

// The exchange arena of a kernel: slot i starts at unit *slots[i], the units of sizes[0 .. i) before it; returns the units of all n. The size
// lists are the kernels' own.
int64_t carve_exchange(const int64_t * sizes, int n, int * const * slots);

}  // namespace rwkvmi
