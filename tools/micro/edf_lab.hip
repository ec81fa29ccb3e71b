// lab: the EDF decode kernel (csrc/kernels_edf.h) at 1 .. 32 samples per thread, back-to-back launches under HIP events, on the
// one-hour shape of tools/time_edf_ops.py (33 signals x 256 samples x 3600 records, 19 selected): what kEdfPerThread was chosen by
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#include <algorithm>
#include "../../eeg_gnn_ssl_amd/csrc/kernels_edf.h"
using namespace eeg;
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)
template <typename T, int PER>
float run(const int16_t* p, long long rec, long long R, long long n, EdfChannels ch, T* out, int C, int reps) {
    const long long L = rec * n, tile = kEdfThreads * PER;
    dim3 grid((unsigned)((L + tile - 1) / tile), C);
    hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
    for (int i = 0; i < 5; ++i) hipLaunchKernelGGL((edf_decode_kernel<T, PER>), grid, dim3(kEdfThreads), 0, 0, p, rec, R, n, ch, out, L);
    hipEventRecord(a);
    for (int i = 0; i < reps; ++i) hipLaunchKernelGGL((edf_decode_kernel<T, PER>), grid, dim3(kEdfThreads), 0, 0, p, rec, R, n, ch, out, L);
    hipEventRecord(b); hipEventSynchronize(b);
    float ms; hipEventElapsedTime(&ms, a, b);
    if (hipGetLastError() != hipSuccess) return -1.f;
    return ms / reps * 1000.f;
}
int main() {
    const long long rec = 3600, n = 256, NS = 33, R = NS * n; const int C = 19;
    int16_t* p; double* out;
    CK(hipMalloc(&p, 2 * rec * R)); CK(hipMalloc(&out, 8 * C * rec * n));
    CK(hipMemset(p, 0x5a, 2 * rec * R));
    EdfChannels ch = {};
    for (int c = 0; c < C; ++c) { ch.off[c] = (long long)(32 - c) * n; ch.gain[c] = 0.1673 + c; ch.offset[c] = 0.0239; }
    for (int round = 0; round < 3; ++round) {
        printf("round %d  us per launch  f64: PER1 %.2f PER2 %.2f PER4 %.2f PER8 %.2f PER16 %.2f PER32 %.2f | f32: PER1 %.2f PER2 %.2f PER4 %.2f PER8 %.2f PER16 %.2f PER32 %.2f\n", round,
               run<double, 1>(p, rec, R, n, ch, out, C, 200), run<double, 2>(p, rec, R, n, ch, out, C, 200), run<double, 4>(p, rec, R, n, ch, out, C, 200),
               run<double, 8>(p, rec, R, n, ch, out, C, 200), run<double, 16>(p, rec, R, n, ch, out, C, 200), run<double, 32>(p, rec, R, n, ch, out, C, 200),
               run<float, 1>(p, rec, R, n, ch, (float*)out, C, 200), run<float, 2>(p, rec, R, n, ch, (float*)out, C, 200), run<float, 4>(p, rec, R, n, ch, (float*)out, C, 200),
               run<float, 8>(p, rec, R, n, ch, (float*)out, C, 200), run<float, 16>(p, rec, R, n, ch, (float*)out, C, 200), run<float, 32>(p, rec, R, n, ch, (float*)out, C, 200));
    }
    CK(hipDeviceSynchronize());
    hipFree(p); hipFree(out);
    return 0;
}
