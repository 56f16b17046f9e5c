// testhooks_rowsum.cpp -- the ring kernel's row-sum reductions for tests/ ONLY (include/rwkv_testhooks_rowsum.h). `make` links it into
// lib/librwkv_testhooks_sample.so beside testhooks_sample.cpp; neither librwkv.so nor librwkv_testhooks.so carries it.
#include "model.h"
#include "rwkv_testhooks_rowsum.h"

using namespace rwkvmi;

extern "C" {

// Test hook: wave_sum_n<n> and wave_sum_scatter<n> (ring_v6.hip) on the same n x 64 values, one wave.
RWKV_API bool rwkv_test_ring_rowsum(int n, const float * values, float * butterfly_out, float * scatter_out, int * lanes_per_value) {
    g_last_error = RWKV_ERROR_NONE;
    RW_CHECK(RWKV_ERROR_ARGS, false, values && butterfly_out && scatter_out && lanes_per_value && n >= 1 && n <= 16, "bad arguments");
    const size_t bytes = (size_t) n * 64 * 4;
    DevBuf<float> in_buf, n_buf, s_buf;
    bool ok = in_buf.alloc((size_t) n * 64) == hipSuccess && n_buf.alloc((size_t) n * 64) == hipSuccess && s_buf.alloc(64) == hipSuccess;
    float * d_in = in_buf.p, * d_n = n_buf.p, * d_s = s_buf.p;
    ok = ok && hipMemcpy(d_in, values, bytes, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        ok = launch_ring_rowsum_test(n, d_in, d_n, d_s, nullptr) && hipDeviceSynchronize() == hipSuccess &&
             hipMemcpy(butterfly_out, d_n, bytes, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(scatter_out, d_s, 64 * 4, hipMemcpyDeviceToHost) == hipSuccess;
        *lanes_per_value = ring_rowsum_lanes(n);
    }
    RW_CHECK(RWKV_ERROR_GRAPH, false, ok, "HIP error: %s", hipGetErrorString(hipGetLastError()));
    return true;
}

}  // extern "C"
