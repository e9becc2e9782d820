// Test probe (tests/test_sincos_gpu.py), not part of libr2l_hip.so or its ABI: the encoder's r2l_sincos and one angle doubling
// of its result, for an array of arguments.  Built by the test with the library's own compiler flags (-ffp-contract=off).
#include <hip/hip_runtime.h>
#include "r2l_common.h"

__global__ void sincos_probe_kernel(const float* __restrict__ x, float* __restrict__ out, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s, c, s2, c2;
    r2l_sincos(x[i], s, c);
    r2l_sincos_double(s, c, s2, c2);
    out[4 * i + 0] = s;
    out[4 * i + 1] = c;
    out[4 * i + 2] = s2;
    out[4 * i + 3] = c2;
}

// out: [n][4] = sin x, cos x, then (sin 2x, cos 2x) by r2l_sincos_double.  Returns the hipError_t of the launch.
extern "C" int sincos_probe(const float* x, float* out, long long n, void* stream) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(sincos_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, out, n);
    return (int)hipGetLastError();
}
