// persist_host.cpp -- the control-word protocol and the trace buffer of the persistent decode kernels (persist_host.h), written once.
#include "model.h"

#include <cstdio>
#include <cstdlib>

namespace rwkvmi {

const char * decode_path_name(DecodePath p) {
    switch (p) {
        case DecodePath::Regs: return "regs";
        case DecodePath::Ring: return "ring";
        case DecodePath::K47:  return "k47";
        default:               return "none";
    }
}

bool PersistCtl::alloc(unsigned generation) {
    bool ok = dev.alloc(64) == hipSuccess && hipMemset(dev.p, 0, 256) == hipSuccess   // (256 bytes; dev[2..6]: the greedy history words)
           && host.alloc(16) == hipSuccess;
    if (ok) { host.p[0] = generation; host.p[1] = 0u; }
    const unsigned init[2] = {generation, 0u};
    return ok && hipMemcpy(dev.p, init, sizeof(init), hipMemcpyHostToDevice) == hipSuccess;
}
bool PersistCtl::fetch(hipStream_t st) const { return hipMemcpyAsync(host.p, dev.p, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, st) == hipSuccess; }
bool PersistCtl::aborted(hipStream_t st) const {
    if (!fetch(st) || hipStreamSynchronize(st) != hipSuccess) return true;
    return aborted_cached();
}
unsigned PersistCtl::generation(hipStream_t st) const {
    if (!fetch(st) || hipStreamSynchronize(st) != hipSuccess) return 0;
    return host.p[0];
}
bool PersistCtl::clear_abort(hipStream_t st) {
    host.p[1] = 0u;
    return hipMemsetAsync(dev.p + 1, 0, sizeof(unsigned), st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
}
bool PersistCtl::set_tag(unsigned base, hipStream_t st) {
    if (hipStreamSynchronize(st) != hipSuccess) return false;
    return hipMemcpy(dev.p, &base, sizeof(unsigned), hipMemcpyHostToDevice) == hipSuccess;
}
bool PersistCtl::force_abort(hipStream_t st) {
    if (hipStreamSynchronize(st) != hipSuccess) return false;
    const unsigned one = 1u;
    return hipMemcpy(dev.p + 1, &one, sizeof(one), hipMemcpyHostToDevice) == hipSuccess;
}
bool PersistCtl::set_history(uint32_t * hist, size_t n, hipStream_t st) {
    const unsigned long long a = (unsigned long long) hist;
    const unsigned w[5] = {hist ? 1u : 0u, 0u, (unsigned) (a & 0xFFFFFFFFull), (unsigned) (a >> 32), hist ? (unsigned) (n > 0xFFFFFFFFull ? 0xFFFFFFFFull : n) : 0u};
    return hipMemcpyAsync(dev.p + 2, w, sizeof(w), hipMemcpyHostToDevice, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
}

PersistentDecoder::~PersistentDecoder() = default;

bool PersistentDecoder::trace_into(long long *& slot, int & slot_layer, int layer, size_t n, size_t extra, long long * out, bool fetch) {
    if (!trace_buf) { if (trace_buf.alloc(n + extra) != hipSuccess) return false; (void) hipMemset(trace_buf.p, 0, (n + extra) * 8); }
    slot = trace_buf.p; slot_layer = layer;
    if (!fetch) return true;
    const char * path = extra ? getenv("RWKV_MI_RING_LTRACE") : nullptr;   // measurement aid: the loader samples as raw int64 [2][512][4]
    if (path) {
        std::vector<long long> buf(extra);
        if (hipMemcpy(buf.data(), trace_buf.p + n, extra * 8, hipMemcpyDeviceToHost) == hipSuccess) {
            if (FILE * f = fopen(path, "wb")) { fwrite(buf.data(), 8, extra, f); fclose(f); }
        }
    }
    return hipMemcpy(out, trace_buf.p, n * 8, hipMemcpyDeviceToHost) == hipSuccess;
}

ArenaOffsets::ArenaOffsets(const Model & m) : base((const unsigned char *) m.arena), bytes(m.arena_bytes) {}
long long ArenaOffsets::off(const void * ptr) {
    const long long o = (const unsigned char *) ptr - base;
    if (!ptr || o < 0 || (uint64_t) o >= bytes) in_arena = false;
    return o;
}
M6Off ArenaOffsets::pl3(const DevTensor * t) { M6Off o; o.qs = off(t->qs); o.qh = t->qh ? off(t->qh) : 0; o.sc = off(t->sc); return o; }

bool v6_stage_shape(const Model & m, V6Shape & s) {
    if (m.arch_major != 6 || m.head_size != 64 || m.layer_end <= m.layer_begin) return false;
    const LayerW & L0 = m.layers[m.layer_begin];
    if (!L0.ffn_key || !L0.att_time_decay_w1 || !L0.att_time_maa_w1) return false;
    s.D = m.n_embed(); s.H = m.head_count; s.fmt = (int) m.header.data_type;
    s.F = L0.ffn_key->ne[1]; s.DR = L0.att_time_decay_w1->ne[1]; s.R5 = L0.att_time_maa_w1->ne[1]; s.R = s.R5 / 5;
    for (uint32_t i = m.layer_begin; i < m.layer_end; i++) {
        const LayerW & L = m.layers[i];
        const DevTensor * mats[] = {L.att_receptance, L.att_key, L.att_value, L.att_gate, L.att_output, L.att_time_maa_w1,
                                    L.att_time_decay_w1, L.att_time_decay_w2, L.ffn_key, L.ffn_value, L.ffn_receptance};
        for (const DevTensor * t : mats) if (!t || t->type != s.fmt) return false;
        if (L.ffn_key->ne[1] != s.F || L.att_time_decay_w1->ne[1] != s.DR || L.att_time_maa_w1->ne[1] != s.R5) return false;
    }
    return true;
}

V6Table v6_layer_table(const Model & m, size_t w2_layer) {
    V6Table t;
    ArenaOffsets a(m);
    for (uint32_t i = m.layer_begin; i < m.layer_end; i++) {
        const LayerW & L = m.layers[i];
        M6Layer d{};
        d.ln1_w = a.f(L.ln1_w); d.ln1_b = a.f(L.ln1_b); d.maa_x = a.f(L.att_time_maa_x);
        d.maa[0] = a.f(L.att_time_maa_w); d.maa[1] = a.f(L.att_time_maa_k); d.maa[2] = a.f(L.att_time_maa_v); d.maa[3] = a.f(L.att_time_maa_r); d.maa[4] = a.f(L.att_time_maa_g);
        d.w2b = (long long) (t.layers.size() * w2_layer); d.time_decay = a.f(L.att_time_decay); d.faaaa = a.f(L.att_time_faaaa);
        d.lnx_w = a.f(L.att_ln_x_w); d.lnx_b = a.f(L.att_ln_x_b); d.ln2_w = a.f(L.ln2_w); d.ln2_b = a.f(L.ln2_b);
        d.fmaa_k = a.f(L.ffn_time_maa_k); d.fmaa_r = a.f(L.ffn_time_maa_r);
        d.w1 = a.pl3(L.att_time_maa_w1);
        d.rkvg[0] = a.pl3(L.att_receptance); d.rkvg[1] = a.pl3(L.att_key); d.rkvg[2] = a.pl3(L.att_value); d.rkvg[3] = a.pl3(L.att_gate);
        d.dw1 = a.pl3(L.att_time_decay_w1); d.dw2 = a.pl3(L.att_time_decay_w2); d.wo = a.pl3(L.att_output);
        d.fk = a.pl3(L.ffn_key); d.fr = a.pl3(L.ffn_receptance); d.fv = a.pl3(L.ffn_value);
        t.layers.push_back(d);
        const DevTensor * all[] = {L.ln1_w, L.ln1_b, L.att_time_maa_x, L.att_time_maa_w, L.att_time_maa_k, L.att_time_maa_v, L.att_time_maa_r, L.att_time_maa_g,
                                   L.att_time_maa_w1, L.att_time_maa_w2, L.att_time_decay, L.att_time_faaaa, L.att_time_decay_w1, L.att_time_decay_w2,
                                   L.att_receptance, L.att_key, L.att_value, L.att_gate, L.att_output, L.att_ln_x_w, L.att_ln_x_b, L.ln2_w, L.ln2_b,
                                   L.ffn_time_maa_k, L.ffn_time_maa_r, L.ffn_key, L.ffn_value, L.ffn_receptance};
        for (const DevTensor * x : all) if (x) t.bytes += x->nbytes;
        t.bytes += 2 * (uint64_t) m.state_per_layer() * sizeof(float);
    }
    t.in_arena = a.in_arena;
    return t;
}

int64_t carve_exchange(const int64_t * sizes, int n, int * const * slots) {
    int64_t units = 0;
    for (int i = 0; i < n; i++) { *slots[i] = (int) units; units += sizes[i]; }
    return units;
}

// Why no persistent kernel serves this model on this device (nullptr: one does). The kernels give every CU one workgroup and hand vectors
// over between them inside the launch: they need all 256 CUs of an unpartitioned MI355X (a CPX / DPX partition or another part reports
// fewer), quantised matrices of one format, 64-wide heads and a geometry that has an instantiation.
const char * persist_unavailable_reason(const Model & m) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, m.device) != hipSuccess) return "the device properties could not be read";
    static thread_local char buf[160];
    if (prop.multiProcessorCount != 256) { snprintf(buf, sizeof buf, "the device reports %d CUs: the persistent kernels need all 256 of an unpartitioned MI355X (SPX mode)", prop.multiProcessorCount); return buf; }
    if (m.head_size != 64) return "head size is not 64";
    if (m.arch_major == 5) return "RWKV-5 has no persistent kernel (per-op launches)";
    const int t = (int) m.header.data_type;
    if (t == T_F32 || t == T_F16) return "FP32 / FP16 files run the per-op launches (the persistent kernels stream quantised matrices)";
    return "no instantiation for this geometry (n_embed / ffn size / ranks / vocabulary)";
}

}  // namespace rwkvmi
