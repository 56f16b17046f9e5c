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
    bool ok = hipMalloc((void **) &dev, 256) == hipSuccess && hipMemset(dev, 0, 256) == hipSuccess   // (dev[2..6]: the greedy history words)
           && hipHostMalloc((void **) &host, 64, hipHostMallocDefault) == hipSuccess;
    if (ok) { host[0] = generation; host[1] = 0u; }
    const unsigned init[2] = {generation, 0u};
    return ok && hipMemcpy(dev, init, sizeof(init), hipMemcpyHostToDevice) == hipSuccess;
}
void PersistCtl::release() {
    if (dev) (void) hipFree(dev);
    if (host) (void) hipHostFree(host);
    dev = nullptr; host = nullptr;
}
bool PersistCtl::fetch(hipStream_t st) const { return hipMemcpyAsync(host, dev, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, st) == hipSuccess; }
bool PersistCtl::aborted(hipStream_t st) const {
    if (!fetch(st) || hipStreamSynchronize(st) != hipSuccess) return true;
    return aborted_cached();
}
unsigned PersistCtl::generation(hipStream_t st) const {
    if (!fetch(st) || hipStreamSynchronize(st) != hipSuccess) return 0;
    return host[0];
}
bool PersistCtl::clear_abort(hipStream_t st) {
    host[1] = 0u;
    return hipMemsetAsync(dev + 1, 0, sizeof(unsigned), st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
}
bool PersistCtl::set_tag(unsigned base, hipStream_t st) {
    if (hipStreamSynchronize(st) != hipSuccess) return false;
    return hipMemcpy(dev, &base, sizeof(unsigned), hipMemcpyHostToDevice) == hipSuccess;
}
bool PersistCtl::force_abort(hipStream_t st) {
    if (hipStreamSynchronize(st) != hipSuccess) return false;
    const unsigned one = 1u;
    return hipMemcpy(dev + 1, &one, sizeof(one), hipMemcpyHostToDevice) == hipSuccess;
}
bool PersistCtl::set_history(uint32_t * hist, size_t n, hipStream_t st) {
    const unsigned long long a = (unsigned long long) hist;
    const unsigned w[5] = {hist ? 1u : 0u, 0u, (unsigned) (a & 0xFFFFFFFFull), (unsigned) (a >> 32), hist ? (unsigned) (n > 0xFFFFFFFFull ? 0xFFFFFFFFull : n) : 0u};
    return hipMemcpyAsync(dev + 2, w, sizeof(w), hipMemcpyHostToDevice, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
}

PersistentDecoder::~PersistentDecoder() {
    ctl.release();
    if (trace_buf) (void) hipFree(trace_buf);
}

bool PersistentDecoder::trace_into(long long *& slot, int & slot_layer, int layer, size_t n, size_t extra, long long * out, bool fetch) {
    if (!trace_buf) { if (hipMalloc((void **) &trace_buf, (n + extra) * 8) != hipSuccess) return false; (void) hipMemset(trace_buf, 0, (n + extra) * 8); }
    slot = trace_buf; slot_layer = layer;
    if (!fetch) return true;
    const char * path = extra ? getenv("RWKV_MI_RING_LTRACE") : nullptr;   // measurement aid: the loader samples as raw int64 [2][512][4]
    if (path) {
        std::vector<long long> buf(extra);
        if (hipMemcpy(buf.data(), trace_buf + n, extra * 8, hipMemcpyDeviceToHost) == hipSuccess) {
            if (FILE * f = fopen(path, "wb")) { fwrite(buf.data(), 8, extra, f); fclose(f); }
        }
    }
    return hipMemcpy(out, trace_buf, n * 8, hipMemcpyDeviceToHost) == hipSuccess;
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
