// read_ring.h -- the reader ring behind the model loader (model.hip) and the device file quantiser (quant_w.hip): a file's spans, each of at
// most k_piece bytes, are pread() in order by a small pool of threads into a ring of PINNED host slots. The owner takes the spans in
// order (wait_read), enqueues its copy / kernels from the slot on `st`, records the slot's event (record) and hands the slot back (release);
// a slot is refilled when it was released and the event behind its last use has completed. Each slot has a device twin of the same size
// for payloads that a kernel reads (a real DMA needs pinned memory: a copy out of a pageable mapping is staged synchronously in the runtime).
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cerrno>
#include <condition_variable>
#include <fcntl.h>
#include <mutex>
#include <thread>
#include <unistd.h>

#include "common.h"

namespace rwkvmi {

struct ReadRing {
    static constexpr size_t k_piece = (size_t) 32 << 20;
    static constexpr int k_slots = 4, k_readers = 4;
    struct Span { uint64_t off, bytes; };

    int fd = -1;
    void * h[k_slots] = {}; void * d[k_slots] = {}; hipEvent_t ev[k_slots] = {};
    hipStream_t st = nullptr;
    std::vector<Span> spans;
    std::vector<std::thread> th;
    std::mutex mu; std::condition_variable cv;
    std::vector<int> state;          // per span: 0 not read, 1 read (slot filled), 2 released (event recorded), -1 read error
    std::atomic<size_t> next{0};
    bool stop = false;

    ~ReadRing() {
        { std::lock_guard<std::mutex> lk(mu); stop = true; }
        cv.notify_all();
        for (std::thread & t : th) if (t.joinable()) t.join();
        if (st) { (void) hipStreamSynchronize(st); (void) hipStreamDestroy(st); }
        for (int i = 0; i < k_slots; i++) { if (h[i]) (void) hipHostFree(h[i]); if (d[i]) (void) hipFree(d[i]); if (ev[i]) (void) hipEventDestroy(ev[i]); }
        if (fd >= 0) close(fd);
    }

    static int slot(size_t i) { return (int) (i % k_slots); }

    // opens the file, allocates the slots (their device twins with device_slots) and starts the readers on the current device
    bool start(const char * path, std::vector<Span> file_spans, bool device_slots, int device) {
#define RING_HIP_OK(FLAGS, CALL) do { hipError_t e_ = (CALL); RW_CHECK((FLAGS), false, e_ == hipSuccess, "HIP error: %s", hipGetErrorString(e_)); } while (0)
        spans = std::move(file_spans);
        fd = open(path, O_RDONLY);
        RW_CHECK(RWKV_ERROR_FILE | RWKV_ERROR_FILE_OPEN, false, fd >= 0, "Failed to open file %s", path);
        (void) posix_fadvise(fd, 0, 0, POSIX_FADV_SEQUENTIAL);
        RING_HIP_OK(RWKV_ERROR_CTX, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        for (int i = 0; i < k_slots && !spans.empty(); i++) {
            RING_HIP_OK(RWKV_ERROR_MODEL | RWKV_ERROR_ALLOC, hipHostMalloc(&h[i], k_piece, hipHostMallocDefault));
            if (device_slots) RING_HIP_OK(RWKV_ERROR_MODEL | RWKV_ERROR_ALLOC, hipMalloc(&d[i], k_piece));
            RING_HIP_OK(RWKV_ERROR_CTX, hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
        }
#undef RING_HIP_OK
        state.assign(spans.size(), 0);
        for (int i = 0; i < k_readers && (size_t) i < spans.size(); i++) th.emplace_back([this, device] { read_loop(device); });
        return true;
    }

    // true once span i rests in h[slot(i)]; false when it could not be read
    bool wait_read(size_t i) {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return state[i] != 0; });
        return state[i] == 1;
    }
    // after the last work on `st` that reads slot(i)
    hipError_t record(size_t i) { return hipEventRecord(ev[slot(i)], st); }
    void release(size_t i) {
        { std::lock_guard<std::mutex> g(mu); state[i] = 2; }
        cv.notify_all();
    }

private:
    void read_loop(int device) {
        (void) hipSetDevice(device);
        for (;;) {
            const size_t i = next.fetch_add(1);
            if (i >= spans.size()) return;
            const int s = slot(i);
            if (i >= (size_t) k_slots) {
                // the slot's previous span must have been released and the copy / kernel behind its event finished
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return stop || state[i - k_slots] == 2; });
                if (stop) return;
                lk.unlock();
                if (hipEventSynchronize(ev[s]) != hipSuccess) { std::lock_guard<std::mutex> g(mu); state[i] = -1; cv.notify_all(); return; }
            }
            const Span & sp = spans[i];
            uint64_t done = 0;
            bool ok = true;
            while (done < sp.bytes) {
                const ssize_t r = pread(fd, (uint8_t *) h[s] + done, sp.bytes - done, (off_t) (sp.off + done));
                if (r <= 0) { if (r < 0 && errno == EINTR) continue; ok = false; break; }
                done += (uint64_t) r;
            }
            { std::lock_guard<std::mutex> g(mu); state[i] = ok ? 1 : -1; }
            cv.notify_all();
            if (!ok) return;
        }
    }
};

}  // namespace rwkvmi
