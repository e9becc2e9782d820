// r2l_dw_tail.hip — tail weight / bias gradients (3x256) by plain reduction over the rays, and the reduce of the per-workgroup
// partials.  r2l_dw_tail_launch runs the stage.
#include "r2l_dw.h"

// =================================================================================================================
// Tail gradients: dWt[c][f] = sum_r dpre[r][c] * (x_n[r][f] + x_0[r][f]),  dbt[c] = sum_r dpre[r][c]
// =================================================================================================================
__global__ __launch_bounds__(256) void r2l_dw_tail_kernel(const float* __restrict__ dpre, const float* __restrict__ x0,
                                                          const float* __restrict__ xn, float* __restrict__ grads,
                                                          float* __restrict__ part, int n_block, int64_t N,
                                                          int64_t rays_per_wg) {
    const int f = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * rays_per_wg;
    int64_t r1 = r0 + rays_per_wg;
    if (r1 > N) r1 = N;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, b0 = 0.f, b1 = 0.f, b2 = 0.f;
    // (8 rows in flight per thread: one row per trip left this loop load-latency bound, 0.10 ms per 98 304 rays for 100 MB)
#pragma unroll 8
    for (int64_t r = r0; r < r1; ++r) {
        const float y = x0 != nullptr ? xn[r * R2L_W + f] + x0[r * R2L_W + f] : xn[r * R2L_W + f];  // x0 == nullptr: xn holds y
        const float d0 = dpre[r * 3 + 0], d1 = dpre[r * 3 + 1], d2 = dpre[r * 3 + 2];
        s0 = __builtin_fmaf(d0, y, s0);
        s1 = __builtin_fmaf(d1, y, s1);
        s2 = __builtin_fmaf(d2, y, s2);
        b0 += d0; b1 += d1; b2 += d2;
    }
    if (part != nullptr) {  // [wg][4][256]: rows 0-2 = dWt partial, row 3 = dbt partial (first 3 entries)
        float* p = part + (int64_t)blockIdx.x * (4 * R2L_W);
        p[0 * R2L_W + f] = s0;
        p[1 * R2L_W + f] = s1;
        p[2 * R2L_W + f] = s2;
        if (f == 0) { p[3 * R2L_W + 0] = b0; p[3 * R2L_W + 1] = b1; p[3 * R2L_W + 2] = b2; }
        return;
    }
    float* gw = grads + r2l_off_tail_w(n_block);
    atomicAdd(gw + 0 * R2L_W + f, s0);
    atomicAdd(gw + 1 * R2L_W + f, s1);
    atomicAdd(gw + 2 * R2L_W + f, s2);
    if (f == 0 && r0 < r1) {
        float* gb = grads + r2l_off_tail_b(n_block);
        atomicAdd(gb + 0, b0);
        atomicAdd(gb + 1, b1);
        atomicAdd(gb + 2, b2);
    }
}

// tail.0.{weight,bias} += partials of all workgroups in a fixed order: thread (f, j) adds the partials of workgroups
// w = j, j+8, ... (8 independent chains keep enough loads in flight), then the 8 sums are added in j order.
__global__ __launch_bounds__(256) void r2l_tail_reduce_kernel(const float* __restrict__ part, int64_t wgs,
                                                              float* __restrict__ grads, int n_block) {
    __shared__ float red[8][32];
    const int row = blockIdx.y, f = blockIdx.x * 32 + (threadIdx.x & 31), j = threadIdx.x >> 5;
    float s = 0.f;
#pragma unroll 8
    for (int64_t w = j; w < wgs; w += 8) s += part[w * (4 * R2L_W) + row * R2L_W + f];
    red[j][threadIdx.x & 31] = s;
    __syncthreads();
    if (j == 0) {
        float t = red[0][threadIdx.x];
#pragma unroll
        for (int k = 1; k < 8; ++k) t += red[k][threadIdx.x];
        if (row < 3) grads[r2l_off_tail_w(n_block) + row * R2L_W + f] += t;
        else if (f < 3) grads[r2l_off_tail_b(n_block) + f] += t;
    }
}

int r2l_dw_tail_launch(const float* dpre, const float* x0, const float* xn, float* grads, float* part, int n_block, int64_t N,
                       int64_t wgs, int64_t rays_per_wg, hipStream_t stream) {
    hipLaunchKernelGGL(r2l_dw_tail_kernel, dim3((unsigned)wgs), dim3(256), 0, stream, dpre, x0, xn, grads, part, n_block, N,
                       rays_per_wg);
    R2L_CHECK(hipGetLastError());
    if (part != nullptr) {
        hipLaunchKernelGGL(r2l_tail_reduce_kernel, dim3(R2L_W / 32, 4), dim3(256), 0, stream, part, wgs, grads, n_block);
        R2L_CHECK(hipGetLastError());
    }
    return 0;
}
