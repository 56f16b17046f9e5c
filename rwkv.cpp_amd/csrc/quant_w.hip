// quant_w.hip -- the weight quantiser on the device: FP32 / FP16 weight rows -> Q4_0 | Q4_1 | Q5_0 | Q5_1 | Q8_0 blocks, with the arithmetic
// of the host quantiser (quantize.cpp, quantize_row) operation for operation, so that both produce the same bytes. One body, two output
// forms: the planes launch_repack leaves in HBM (the loader's piece kind 3, rwkv_mi_init_from_file_as) and the file's interleaved block
// bytes (rwkv_mi_quantize_model_file, below). DESIGN.md 6.19.
//
// Split: a tile is 256 consecutive blocks (8192 weights); a workgroup of 256 lanes walks a contiguous run of tiles, one block per lane.
//   1. the tile's source bytes (32 KiB FP32, 16 KiB FP16: one contiguous span, rows are whole blocks) come in as 16-byte loads, lane after
//      lane, and are laid into LDS block by block at a pitch of the block's bytes + 16: eight consecutive lanes reading 16 bytes of their
//      own blocks then touch every bank once, which is the rate of a 128-bit LDS read;
//   2. each lane reads its 32 elements into registers and runs the host's statement in index order -- no cross-lane reduction, so the
//      first-greatest-magnitude rule of Q4_0 / Q5_0 (whose sign is the scale's sign) holds by construction;
//   3. the lane lays its codes, fifth bits and scales into a second LDS region in the layout of the destination -- per plane, or the file's
//      18..34-byte blocks -- and the workgroup writes each destination span with 16-byte stores (2-byte stores for the last bytes of a
//      short tile). No atomics, no scratch memory, nothing shared between workgroups.
#include "kernels.h"
#include "read_ring.h"

#include <cinttypes>
#include <cmath>
#include <cstring>
#include <deque>
#include <sys/stat.h>

namespace rwkvmi {

constexpr int QW_TILE = 256;             // blocks per tile == lanes per workgroup
constexpr int QW_MAX_WORKGROUPS = 1024;  // a 32 MiB FP32 piece is 1024 tiles

enum : int { QW_PLANES = 0, QW_BLOCKS = 1 };

template <int TYPE> struct QwFmt {
    static constexpr bool has_m = TYPE == T_Q4_1 || TYPE == T_Q5_1;
    static constexpr bool has_h = TYPE == T_Q5_0 || TYPE == T_Q5_1;
    static constexpr int qs_bytes = TYPE == T_Q8_0 ? 32 : 16;
    static constexpr int sc_bytes = has_m ? 4 : 2;
    static constexpr int block_bytes = sc_bytes + (has_h ? 4 : 0) + qs_bytes;
    static constexpr int words = qs_bytes / 4;
};

// round to nearest even, as the host's (_Float16) cast. The value passes through a register of its own first: left to itself the compiler
// fuses `mx / -8` and this conversion into one v_fma_mixlo_f16 (mx * -0.125 + 0), and -0.0 + 0 is +0.0 -- the all-zero block's 0x8000 lost
__device__ inline uint16_t qw_f16_bits(float f) {
    asm volatile("" : "+v"(f));
    const _Float16 h = (_Float16) f;
    return __builtin_bit_cast(uint16_t, h);
}

// l[0 .. nbytes) -> g, by the whole workgroup: 16-byte stores, then 2-byte stores for what is left (nbytes is even; both 16-byte aligned)
__device__ inline void qw_store_span(const uint8_t * l, uint8_t * __restrict__ g, int nbytes) {
    const int n16 = nbytes >> 4;
    for (int i = threadIdx.x; i < n16; i += QW_TILE) ((uint4 *) g)[i] = ((const uint4 *) l)[i];
    for (int i = n16 * 8 + threadIdx.x; i < (nbytes >> 1); i += QW_TILE) ((uint16_t *) g)[i] = ((const uint16_t *) l)[i];
}

// SRC: T_F32 / T_F16. FORM QW_PLANES: qs / qh / sc are the planes' positions of block 0; QW_BLOCKS: qs is the first block's first byte.
template <int SRC, int TYPE, int FORM>
__global__ __launch_bounds__(QW_TILE) void k_quant_w(const uint8_t * __restrict__ src, int64_t n_blocks, int64_t tiles_per_wg, uint8_t * __restrict__ qs,
                                                      uint32_t * __restrict__ qh, uint8_t * __restrict__ sc) {
    using F = QwFmt<TYPE>;
    constexpr int SRC_BLOCK = SRC == T_F32 ? 128 : 64;   // bytes of a block's 32 source elements
    constexpr int PITCH = SRC_BLOCK + 16;
    constexpr int U4 = SRC_BLOCK / 16;                   // 16-byte loads per block
    // the output region: per plane at the tile's pitch, or the tile's blocks back to back
    constexpr int OUT_QH = QW_TILE * F::qs_bytes, OUT_SC = OUT_QH + QW_TILE * 4;
    constexpr int OUT_BYTES = FORM == QW_PLANES ? OUT_SC + QW_TILE * F::sc_bytes : QW_TILE * F::block_bytes;
    __shared__ __attribute__((aligned(16))) uint8_t l_in[QW_TILE * PITCH];
    __shared__ __attribute__((aligned(16))) uint8_t l_out[OUT_BYTES];

    const int lane = threadIdx.x;
    const int64_t n_tiles = (n_blocks + QW_TILE - 1) / QW_TILE;
    const int64_t tile0 = (int64_t) blockIdx.x * tiles_per_wg;
    const int64_t tile1 = tile0 + tiles_per_wg < n_tiles ? tile0 + tiles_per_wg : n_tiles;
    for (int64_t tile = tile0; tile < tile1; tile++) {
        const int64_t b0 = tile * QW_TILE;
        const int nv = (int) (n_blocks - b0 < QW_TILE ? n_blocks - b0 : QW_TILE);   // blocks of this tile
        // 1. source -> LDS
        const uint4 * g = (const uint4 *) (src + b0 * SRC_BLOCK);
#pragma unroll
        for (int i = 0; i < U4; i++) {
            const int u = i * QW_TILE + lane;
            if (u < nv * U4) *(uint4 *) (l_in + (u / U4) * PITCH + (u % U4) * 16) = g[u];
        }
        __syncthreads();
        if (lane < nv) {
            // 2. the lane's block, in registers
            float x[32];
            const uint4 * mine = (const uint4 *) (l_in + lane * PITCH);
#pragma unroll
            for (int i = 0; i < U4; i++) {
                const uint4 v = mine[i];
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (SRC == T_F32) x[i * 4 + k] = __builtin_bit_cast(float, w[k]);
                    else {
                        x[i * 8 + 2 * k] = (float) __builtin_bit_cast(_Float16, (uint16_t) (w[k] & 0xFFFFu));
                        x[i * 8 + 2 * k + 1] = (float) __builtin_bit_cast(_Float16, (uint16_t) (w[k] >> 16));
                    }
                }
            }
            // quantize_row's statement for one block (quantize.cpp:33-94)
            uint32_t code[F::words] = {};
            uint32_t hbits = 0;
            uint16_t dh, mh = 0;
            if (TYPE == T_Q4_0 || TYPE == T_Q5_0) {
                constexpr int HALF = TYPE == T_Q4_0 ? 8 : 16, TOP = 2 * HALF - 1;
                float amax = 0.0f, mx = 0.0f;
#pragma unroll
                for (int j = 0; j < 32; j++) if (amax < fabsf(x[j])) { amax = fabsf(x[j]); mx = x[j]; }
                const float d = mx / -HALF, id = d ? 1.0f / d : 0.0f;
                dh = qw_f16_bits(d);
#pragma unroll
                for (int j = 0; j < 16; j++) {
                    const int a = (int8_t) (x[j] * id + (HALF + 0.5f)), b = (int8_t) (x[16 + j] * id + (HALF + 0.5f));
                    const uint32_t q0 = (uint8_t) (a < TOP ? a : TOP), q1 = (uint8_t) (b < TOP ? b : TOP);
                    code[j / 4] |= ((q0 & 0x0F) | ((q1 & 0x0F) << 4)) << (8 * (j % 4));
                    hbits |= ((q0 & 0x10) >> 4) << j;
                    hbits |= ((q1 & 0x10) >> 4) << (j + 16);
                }
            } else if (TYPE == T_Q4_1 || TYPE == T_Q5_1) {
                constexpr int TOP = TYPE == T_Q4_1 ? 15 : 31;
                float mn = INFINITY, mx = -INFINITY;
#pragma unroll
                for (int j = 0; j < 32; j++) { if (x[j] < mn) mn = x[j]; if (x[j] > mx) mx = x[j]; }
                const float d = (mx - mn) / TOP, id = d ? 1.0f / d : 0.0f;
                dh = qw_f16_bits(d); mh = qw_f16_bits(mn);
#pragma unroll
                for (int j = 0; j < 16; j++) {
                    uint32_t q0, q1;
                    if (TYPE == T_Q4_1) {
                        const int a = (int8_t) ((x[j] - mn) * id + 0.5f), b = (int8_t) ((x[16 + j] - mn) * id + 0.5f);
                        q0 = (uint8_t) (a < TOP ? a : TOP); q1 = (uint8_t) (b < TOP ? b : TOP);
                    } else {
                        q0 = (uint8_t) ((x[j] - mn) * id + 0.5f); q1 = (uint8_t) ((x[16 + j] - mn) * id + 0.5f);
                    }
                    code[j / 4] |= ((q0 & 0x0F) | ((q1 & 0x0F) << 4)) << (8 * (j % 4));
                    hbits |= ((q0 & 0x10) >> 4) << j;
                    hbits |= ((q1 & 0x10) >> 4) << (j + 16);
                }
            } else {   // Q8_0
                float amax = 0.0f;
#pragma unroll
                for (int j = 0; j < 32; j++) if (fabsf(x[j]) > amax) amax = fabsf(x[j]);
                const float d = amax / 127, id = d ? 1.0f / d : 0.0f;
                dh = qw_f16_bits(d);
#pragma unroll
                for (int j = 0; j < 32; j++) code[j / 4] |= (uint32_t) (uint8_t) (int8_t) roundf(x[j] * id) << (8 * (j % 4));
            }
            // 3. the block in the destination's layout
            if (FORM == QW_PLANES) {
                uint4 * q = (uint4 *) (l_out + lane * F::qs_bytes);
#pragma unroll
                for (int i = 0; i < F::words / 4; i++) q[i] = make_uint4(code[4 * i], code[4 * i + 1], code[4 * i + 2], code[4 * i + 3]);
                if (F::has_h) ((uint32_t *) (l_out + OUT_QH))[lane] = hbits;
                if (F::has_m) ((uint32_t *) (l_out + OUT_SC))[lane] = (uint32_t) dh | ((uint32_t) mh << 16);
                else ((uint16_t *) (l_out + OUT_SC))[lane] = dh;
            } else {
                uint16_t * o = (uint16_t *) (l_out + lane * F::block_bytes);   // (every field of a block starts on an even byte)
                *o++ = dh;
                if (F::has_m) *o++ = mh;
                if (F::has_h) { *o++ = (uint16_t) (hbits & 0xFFFFu); *o++ = (uint16_t) (hbits >> 16); }
#pragma unroll
                for (int i = 0; i < F::words; i++) { *o++ = (uint16_t) (code[i] & 0xFFFFu); *o++ = (uint16_t) (code[i] >> 16); }
            }
        }
        __syncthreads();
        if (FORM == QW_PLANES) {
            qw_store_span(l_out, qs + b0 * F::qs_bytes, nv * F::qs_bytes);
            if (F::has_h) qw_store_span(l_out + OUT_QH, (uint8_t *) (qh + b0), nv * 4);
            qw_store_span(l_out + OUT_SC, sc + b0 * F::sc_bytes, nv * F::sc_bytes);
        } else {
            qw_store_span(l_out, qs + b0 * F::block_bytes, nv * F::block_bytes);
        }
        // (no barrier here: the next tile's loads write l_in, which every lane left before the barrier above, and its lanes write l_out
        //  only behind the next barrier, which a lane reaches after these stores)
    }
}

template <int SRC, int TYPE, int FORM>
static void launch_one(const void * src, int64_t n_blocks, uint8_t * qs, uint32_t * qh, uint8_t * sc, hipStream_t st) {
    const int64_t n_tiles = (n_blocks + QW_TILE - 1) / QW_TILE;
    if (n_tiles == 0) return;
    const int64_t per = (n_tiles + QW_MAX_WORKGROUPS - 1) / QW_MAX_WORKGROUPS;
    hipLaunchKernelGGL((k_quant_w<SRC, TYPE, FORM>), dim3((unsigned) ((n_tiles + per - 1) / per)), dim3(QW_TILE), 0, st,
                       (const uint8_t *) src, n_blocks, per, qs, qh, sc);
}
template <int FORM>
static void launch_form(int type, int src_type, const void * src, int64_t n_blocks, uint8_t * qs, uint32_t * qh, uint8_t * sc, hipStream_t st) {
#define QW_CASE(T) case T: if (src_type == T_F32) launch_one<T_F32, T, FORM>(src, n_blocks, qs, qh, sc, st); \
                           else launch_one<T_F16, T, FORM>(src, n_blocks, qs, qh, sc, st); break
    switch (type) { QW_CASE(T_Q4_0); QW_CASE(T_Q4_1); QW_CASE(T_Q5_0); QW_CASE(T_Q5_1); default: QW_CASE(T_Q8_0); }
#undef QW_CASE
}

void launch_quant_w_planes(int type, int src_type, const void * src, int64_t n_blocks, uint8_t * qs, uint32_t * qh, void * sc, hipStream_t st) {
    launch_form<QW_PLANES>(type, src_type, src, n_blocks, qs, qh, (uint8_t *) sc, st);
}
void launch_quant_w_blocks(int type, int src_type, const void * src, int64_t n_blocks, uint8_t * blocks, hipStream_t st) {
    launch_form<QW_BLOCKS>(type, src_type, src, n_blocks, blocks, nullptr, nullptr, st);
}

}  // namespace rwkvmi

using namespace rwkvmi;

// ---------------------------------------------------------------------------------------------------------------
// rwkv_mi_quantize_model_file: rwkv_quantize_model_file (quantize.cpp) with the blocks made on the device. The file's payloads travel
// through the loader's reader ring in pieces of at most 32 MiB: a selected tensor's piece goes to the device, through the kernel's blocks
// form and back into a pinned slot; every other piece is written from the slot it was read into. This thread writes in file order and
// keeps two pieces in flight behind the one it writes.
// ---------------------------------------------------------------------------------------------------------------

namespace {

struct FileCloser { void operator()(FILE * f) const { if (f) fclose(f); } };

struct OutSlots {   // where the blocks of a piece land: a device buffer and its pinned twin per ring slot
    void * d[ReadRing::k_slots] = {}; void * h[ReadRing::k_slots] = {};
    ~OutSlots() { for (int i = 0; i < ReadRing::k_slots; i++) { if (d[i]) (void) hipFree(d[i]); if (h[i]) (void) hipHostFree(h[i]); } }
};

}  // namespace

extern "C" RWKV_API bool rwkv_mi_quantize_model_file(const char * in_path, const char * out_path, const char * type_name) {
#define QF_HIP_OK(FLAGS, CALL) do { hipError_t e_ = (CALL); RW_CHECK((FLAGS), false, e_ == hipSuccess, "HIP error: %s", hipGetErrorString(e_)); } while (0)
    g_last_error = RWKV_ERROR_NONE;
    RW_CHECK(RWKV_ERROR_ARGS, false, in_path && out_path && type_name, "NULL argument");
    const int out_type = dtype_from_name(type_name);
    RW_CHECK(RWKV_ERROR_ARGS | RWKV_ERROR_DATA_TYPE, false, out_type >= 0 && dtype_quantized(out_type), "Unsupported output data type (%s)", type_name);

    std::unique_ptr<FILE, FileCloser> in(fopen(in_path, "rb"));
    RW_CHECK(RWKV_ERROR_FILE | RWKV_ERROR_FILE_OPEN, false, in != nullptr, "Failed to open %s for reading", in_path);
    struct stat st;
    RW_CHECK(RWKV_ERROR_FILE | RWKV_ERROR_FILE_STAT, false, fstat(fileno(in.get()), &st) == 0, "failed to stat file %s", in_path);
    FileHeader hdr;
    if (!read_file_header(in.get(), hdr)) { global_fail(RWKV_ERROR_FILE, __FILE__, __LINE__, "read_file_header", "Invalid file header"); return false; }
    RW_CHECK(RWKV_ERROR_FILE, false, hdr.data_type == T_F32 || hdr.data_type == T_F16,
             "Unsupported input data type (%s); needs to be FP32 or FP16", dtype_name((int) hdr.data_type));

    // the directory, and the pieces of every payload in file order
    struct Piece { size_t tensor; int64_t nblk; uint64_t out_bytes; bool first, quant; };   // nblk > 0: blocks made on the device
    std::vector<TensorInfo> infos;
    std::vector<Piece> pieces;
    std::vector<ReadRing::Span> spans;
    while ((uint64_t) ftello(in.get()) < (uint64_t) st.st_size) {
        TensorInfo t;
        if (!read_tensor_info(in.get(), t)) { global_fail(RWKV_ERROR_MODEL_PARAMS, __FILE__, __LINE__, "read_tensor_info", "Failed to read tensor header"); return false; }
        RW_CHECK(RWKV_ERROR_MODEL_PARAMS | RWKV_ERROR_FILE_READ, false, t.file_offset + t.nbytes <= (uint64_t) st.st_size && fseeko(in.get(), (off_t) t.nbytes, SEEK_CUR) == 0,
                 "Failed to read tensor data of %s", t.name.c_str());
        const bool quantize = quantizer_selects(t);
        RW_CHECK(RWKV_ERROR_MODEL_PARAMS | RWKV_ERROR_SHAPE, false, !quantize || t.ne[0] % 32 == 0,
                 "Tensor %s has rows of %" PRId64 " elements: quantised formats need a multiple of 32", t.name.c_str(), t.ne[0]);
        // a piece of a selected tensor is a whole number of the kernel's tiles, so that every piece's blocks start 16-byte aligned
        const uint64_t unit = quantize ? 32 * dtype_block_bytes(t.type) : 1, per = ReadRing::k_piece / unit * unit;
        bool first = true;
        for (uint64_t o = 0; o < t.nbytes || first; o += per, first = false) {
            const uint64_t n = t.nbytes - o < per ? t.nbytes - o : per;
            const int64_t nblk = quantize ? (int64_t) (n / unit) : 0;
            pieces.push_back(Piece{infos.size(), nblk, quantize ? (uint64_t) nblk * dtype_block_bytes(out_type) : n, first, quantize});
            spans.push_back({t.file_offset + o, n});
        }
        infos.push_back(std::move(t));
    }

    // like the loader: no CPU path exists behind this call (rwkv_quantize_model_file is the host's)
    int n_dev = 0, device = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    RW_CHECK(RWKV_ERROR_CTX | RWKV_ERROR_UNSUPPORTED, false, e == hipSuccess && n_dev > 0,
             "No HIP device is visible: rwkv_mi_quantize_model_file runs on the GPU (%s); rwkv_quantize_model_file does not need one",
             e == hipSuccess ? "0 devices" : hipGetErrorString(e));
    QF_HIP_OK(RWKV_ERROR_CTX, hipGetDevice(&device));
    hipDeviceProp_t prop;
    QF_HIP_OK(RWKV_ERROR_CTX, hipGetDeviceProperties(&prop, device));
    RW_CHECK(RWKV_ERROR_CTX | RWKV_ERROR_UNSUPPORTED, false, strncmp(prop.gcnArchName, "gfx950", 6) == 0,
             "Device %d is %s; this library is built for gfx950 (MI355X) only", device, prop.gcnArchName);

    std::unique_ptr<FILE, FileCloser> out(fopen(out_path, "wb"));
    RW_CHECK(RWKV_ERROR_FILE | RWKV_ERROR_FILE_OPEN, false, out != nullptr, "Failed to open %s for writing", out_path);
    FileHeader oh = hdr;
    oh.version = RWKV_FILE_VERSION;
    oh.data_type = (uint32_t) out_type;
    RW_CHECK(RWKV_ERROR_FILE | RWKV_ERROR_FILE_WRITE, false, fwrite(&oh, sizeof oh, 1, out.get()) == 1, "Failed to write file header");

    // (declared before the ring: the ring's destructor drains the stream that writes into them)
    OutSlots os;
    hipEvent_t back[ReadRing::k_slots] = {};   // the copy back into os.h[slot] has landed
    struct Events { hipEvent_t * e; ~Events() { for (int i = 0; i < ReadRing::k_slots; i++) if (e[i]) (void) hipEventDestroy(e[i]); } } events{back};
    bool any_device = false;
    for (const Piece & pc : pieces) any_device = any_device || pc.nblk > 0;
    const size_t out_cap = ReadRing::k_piece / 64 * dtype_block_bytes(out_type);   // an FP16 piece holds the most blocks
    for (int i = 0; i < ReadRing::k_slots && any_device; i++) {
        QF_HIP_OK(RWKV_ERROR_MODEL | RWKV_ERROR_ALLOC, hipMalloc(&os.d[i], out_cap));
        QF_HIP_OK(RWKV_ERROR_MODEL | RWKV_ERROR_ALLOC, hipHostMalloc(&os.h[i], out_cap, hipHostMallocDefault));
        QF_HIP_OK(RWKV_ERROR_CTX, hipEventCreateWithFlags(&back[i], hipEventDisableTiming));
    }
    ReadRing ring;
    if (!ring.start(in_path, std::move(spans), any_device, device)) return false;

    std::deque<size_t> flying;   // pieces taken from the ring and not yet written
    auto write_oldest = [&]() -> bool {
        const size_t i = flying.front();
        flying.pop_front();
        const Piece & pc = pieces[i];
        const TensorInfo & t = infos[pc.tensor];
        const int slot = ReadRing::slot(i);
        if (pc.first) {
            const uint32_t th[6] = {(uint32_t) t.ndim, (uint32_t) t.name.size(), (uint32_t) (pc.quant ? out_type : t.type), (uint32_t) t.ne[0], (uint32_t) t.ne[1], (uint32_t) t.ne[2]};
            const bool ok = fwrite(th, sizeof(uint32_t), 3 + (size_t) t.ndim, out.get()) == 3 + (size_t) t.ndim && fwrite(t.name.data(), 1, t.name.size(), out.get()) == t.name.size();
            RW_CHECK(RWKV_ERROR_FILE_WRITE, false, ok, "Failed to write tensor %s", t.name.c_str());
        }
        if (pc.nblk > 0) QF_HIP_OK(RWKV_ERROR_MODEL | RWKV_ERROR_DATA, hipEventSynchronize(back[slot]));
        const void * payload = pc.nblk > 0 ? os.h[slot] : ring.h[slot];
        RW_CHECK(RWKV_ERROR_FILE_WRITE, false, pc.out_bytes == 0 || fwrite(payload, 1, pc.out_bytes, out.get()) == pc.out_bytes, "Failed to write tensor %s", t.name.c_str());
        ring.release(i);
        return true;
    };
    for (size_t i = 0; i < pieces.size(); i++) {
        const Piece & pc = pieces[i];
        const int slot = ReadRing::slot(i);
        RW_CHECK(RWKV_ERROR_MODEL_PARAMS | RWKV_ERROR_FILE_READ, false, ring.wait_read(i), "Failed to read tensor data of %s", infos[pc.tensor].name.c_str());
        if (pc.nblk > 0) {
            QF_HIP_OK(RWKV_ERROR_MODEL | RWKV_ERROR_DATA, hipMemcpyAsync(ring.d[slot], ring.h[slot], ring.spans[i].bytes, hipMemcpyHostToDevice, ring.st));
            launch_quant_w_blocks(out_type, infos[pc.tensor].type, ring.d[slot], pc.nblk, (uint8_t *) os.d[slot], ring.st);
            QF_HIP_OK(RWKV_ERROR_MODEL | RWKV_ERROR_DATA, hipMemcpyAsync(os.h[slot], os.d[slot], pc.out_bytes, hipMemcpyDeviceToHost, ring.st));
            QF_HIP_OK(RWKV_ERROR_MODEL | RWKV_ERROR_DATA, hipEventRecord(back[slot], ring.st));
            QF_HIP_OK(RWKV_ERROR_MODEL | RWKV_ERROR_DATA, ring.record(i));
        }
        flying.push_back(i);
        while (flying.size() > 2) if (!write_oldest()) return false;
    }
    while (!flying.empty()) if (!write_oldest()) return false;
    QF_HIP_OK(RWKV_ERROR_MODEL | RWKV_ERROR_DATA, hipStreamSynchronize(ring.st));
    QF_HIP_OK(RWKV_ERROR_MODEL | RWKV_ERROR_DATA, hipGetLastError());
    RW_CHECK(RWKV_ERROR_FILE_WRITE, false, fflush(out.get()) == 0, "Failed to write %s", out_path);
    return true;
#undef QF_HIP_OK
}
