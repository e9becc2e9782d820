// r2l_dw_head.hip — head weight gradient on the fp32 MFMA: dW_head = G_head^T PE(rays), the 1008-d positional encoding recomputed
// on the fly (or read from a given embedding), and the reduce of its per-slice partials.  r2l_dw_head_launch runs the stage: in
// the default trio r2l_dw_head16.hip goes in front and the kernel here is its fallback.
#include "r2l_dw.h"

// =================================================================================================================
// Head weight gradient:  dWh[o][k] = sum_r Gh[r][o] * PE[r][k]   (k in 1008, padded to 1024), dbh[o] = sum_r Gh[r][o]
// The encoding is recomputed from the rays (never stored: 4 KB/ray).  Workgroup (kq, slice): kq selects 256 encoding
// columns; wave w of it owns columns kq*256 + w*64 .. +63 (two 32-column tiles) x all 256 output rows (8 tiles).
// Lane (i, h) evaluates encoding column k = base + i (+32) for ray 2s+h: one sin or cos (or the identity) per tile.
// =================================================================================================================
struct HeadStep {  // raw operands of one k-step (two rays), as loaded
    f32x4 g0, g1;
    float o0, d0, u0, o1, d1, u1;
};

// FROM_EMB / JITTER are compile-time so that the pipelined loop body is branch-free (runtime flags inside it made hipcc
// emit per-load branches, spills and vmcnt(0) drains).
template <bool FROM_EMB, bool JITTER>
__global__ __launch_bounds__(256, 1) void r2l_dw_head_kernel(const R2LDwHeadArgs a) {
    if (a.run_if != nullptr && __builtin_nontemporal_load(a.run_if) == 0u) return;  // fallback behind r2l_dw_head16_kernel
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int hh = lane >> 5, jl = lane & 31;
    const int kq = blockIdx.x & 3;
    const int64_t slice = blockIdx.x >> 2;
    const int64_t r0 = slice * a.rays_per_wg;
    int64_t r1 = r0 + a.rays_per_wg;
    if (r1 > a.N) r1 = a.N;
    if (r0 >= r1) return;
    const int kbase = kq * 256 + wave * 64;
    constexpr bool from_emb = FROM_EMB;
    constexpr bool jitter = JITTER && !FROM_EMB;
    const int k0 = kbase + jl, k1 = kbase + 32 + jl;
    const PECol c0 = pe_col(k0), c1 = pe_col(k1);
    const int e0 = k0 < R2L_IN ? k0 : R2L_IN - 1, e1 = k1 < R2L_IN ? k1 : R2L_IN - 1;  // clamped emb columns
    const float m0 = k0 < R2L_IN ? 1.f : 0.f, m1 = k1 < R2L_IN ? 1.f : 0.f;
    // sample depth z = zl + zs * t_rand: the rule of r2l_depths (r2l_student_net.h), one sample per encoding column
    const float zl0 = from_emb ? 0.f : a.ztab[c0.smp], zs0 = jitter ? a.ztab[16 + c0.smp] : 0.f;
    const float zl1 = from_emb ? 0.f : a.ztab[c1.smp], zs1 = jitter ? a.ztab[16 + c1.smp] : 0.f;

    f32x16 acc[8][2];
#pragma unroll
    for (int eo = 0; eo < 8; ++eo)
#pragma unroll
        for (int ei = 0; ei < 2; ++ei)
#pragma unroll
            for (int c = 0; c < 16; ++c) acc[eo][ei][c] = 0.f;
    f32x4 bs0 = {0.f, 0.f, 0.f, 0.f}, bs1 = {0.f, 0.f, 0.f, 0.f};

    const int64_t nfull = (r1 - r0) / 2;
    // unconditional loads of k-step s (row index clamped into the slice)
    auto ld = [&](int64_t s, HeadStep& v) {
        const int64_t sc = s < nfull ? s : (nfull > 0 ? nfull - 1 : 0);
        const int64_t r = r0 + 2 * sc + hh;
        v.g0 = *reinterpret_cast<const f32x4*>(a.gh + r * R2L_W + 4 * jl);
        v.g1 = *reinterpret_cast<const f32x4*>(a.gh + r * R2L_W + 128 + 4 * jl);
        if constexpr (from_emb) {
            v.o0 = a.emb[r * R2L_IN + e0];
            v.o1 = a.emb[r * R2L_IN + e1];
            v.d0 = v.d1 = v.u0 = v.u1 = 0.f;
        } else {
            v.o0 = a.rays_o[r * 3 + c0.ax]; v.d0 = a.rays_d[r * 3 + c0.ax];
            v.o1 = a.rays_o[r * 3 + c1.ax]; v.d1 = a.rays_d[r * 3 + c1.ax];
            if constexpr (jitter) {
                v.u0 = a.t_rand[r * 16 + c0.smp];
                v.u1 = a.t_rand[r * 16 + c1.smp];
            } else {
                v.u0 = v.u1 = 0.f;
            }
        }
    };
    auto encode = [&](const HeadStep& v, float& p0, float& p1) {
        if constexpr (from_emb) { p0 = v.o0 * m0; p1 = v.o1 * m1; return; }
        const float z0 = jitter ? zl0 + zs0 * v.u0 : zl0;
        const float z1 = jitter ? zl1 + zs1 * v.u1 : zl1;
        p0 = pe_eval(c0, v.o0 + v.d0 * z0);
        p1 = pe_eval(c1, v.o1 + v.d1 * z1);
    };
    auto kstep = [&](const f32x4& g0, const f32x4& g1, float p0, float p1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc[e][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(g0[e], p0, acc[e][0], 0, 0, 0);
            acc[e][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(g0[e], p1, acc[e][1], 0, 0, 0);
            acc[4 + e][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(g1[e], p0, acc[4 + e][0], 0, 0, 0);
            acc[4 + e][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(g1[e], p1, acc[4 + e][1], 0, 0, 0);
        }
        bs0 += g0;
        bs1 += g1;
    };
    if (nfull > 0) {
        // 4 rotating raw-operand buffers (loads three k-steps ahead); the encoding of k-step s+1 is evaluated on the
        // VALU while the 32 MFMAs of k-step s run.  16 k-steps per loop trip (hipcc drains vmcnt at loop headers).
        HeadStep hb[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) ld(k, hb[k]);
        float pa0, pa1;
        encode(hb[0], pa0, pa1);
        int64_t s = 0;
        for (; s + 16 <= nfull; s += 16) {
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const f32x4 g0 = hb[k & 3].g0, g1 = hb[k & 3].g1;
                float pn0, pn1;
                encode(hb[(k + 1) & 3], pn0, pn1);  // next k-step's columns
                kstep(g0, g1, pa0, pa1);
                ld(s + k + 4, hb[k & 3]);
                pa0 = pn0;
                pa1 = pn1;
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        for (; s < nfull; ++s) {  // remainder of the slice
            HeadStep v;
            ld(s, v);
            float p0, p1;
            encode(v, p0, p1);
            kstep(v.g0, v.g1, p0, p1);
        }
    }
    if ((r1 - r0) & 1) {  // odd tail: only the lower half-wave's ray exists
        const int64_t r = r1 - 1;
        HeadStep v;
        v.g0 = *reinterpret_cast<const f32x4*>(a.gh + r * R2L_W + 4 * jl);
        v.g1 = *reinterpret_cast<const f32x4*>(a.gh + r * R2L_W + 128 + 4 * jl);
        if constexpr (from_emb) {
            v.o0 = a.emb[r * R2L_IN + e0];
            v.o1 = a.emb[r * R2L_IN + e1];
            v.d0 = v.d1 = v.u0 = v.u1 = 0.f;
        } else {
            v.o0 = a.rays_o[r * 3 + c0.ax]; v.d0 = a.rays_d[r * 3 + c0.ax];
            v.o1 = a.rays_o[r * 3 + c1.ax]; v.d1 = a.rays_d[r * 3 + c1.ax];
            v.u0 = jitter ? a.t_rand[r * 16 + c0.smp] : 0.f;
            v.u1 = jitter ? a.t_rand[r * 16 + c1.smp] : 0.f;
        }
        float p0, p1;
        encode(v, p0, p1);
        if (hh) { v.g0 = f32x4{0.f, 0.f, 0.f, 0.f}; v.g1 = v.g0; p0 = 0.f; p1 = 0.f; }
        kstep(v.g0, v.g1, p0, p1);
    }
    // flush: output row o = half*128 + 4*ro + e, encoding column k = kbase + ei*32 + jl
    float* gw = a.grads;  // head.0.weight is first in the flat buffer, [256][1008]
    float* sl = a.slab ? a.slab + slice * (int64_t)(R2L_W * 1024) : nullptr;
#pragma unroll
    for (int eo = 0; eo < 8; ++eo)
#pragma unroll
        for (int ei = 0; ei < 2; ++ei)
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                const int ro = (c & 3) + 8 * (c >> 2) + 4 * hh;
                const int o = (eo >> 2) * 128 + 4 * ro + (eo & 3);
                const int k = kbase + ei * 32 + jl;
                if (k < R2L_IN) {
                    if (sl) sl[o * 1024 + k] = acc[eo][ei][c];  // 64 slices x 64-way same-address atomics are slow
                    else atomicAdd(gw + (int64_t)o * R2L_IN + k, acc[eo][ei][c]);
                }
            }
    if (kq == 0 && wave == 0) {
        float* gb = a.grads + r2l_off_head_b();
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float s0 = bs0[e] + __shfl_xor(bs0[e], 32);
            const float s1 = bs1[e] + __shfl_xor(bs1[e], 32);
            if (hh == 0) {
                if (sl) {  // bias partial of row o rides in the (otherwise unused) padding column 1008 of the slab row
                    sl[(4 * jl + e) * 1024 + R2L_IN] = s0;
                    sl[(128 + 4 * jl + e) * 1024 + R2L_IN] = s1;
                } else {
                    atomicAdd(gb + 4 * jl + e, s0);
                    atomicAdd(gb + 128 + 4 * jl + e, s1);
                }
            }
        }
    }
}

// dWh[o][k] += sum over slices of slab[slice][o][k] (k < 1008), dbh[o] += sum of slab[slice][o][1008]; slices are
// added in index order (deterministic)
__global__ void r2l_head_reduce_kernel(const float* __restrict__ slab, int n_slices, float* __restrict__ grads) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // over [256][1024]
    if (i >= (int64_t)R2L_W * 1024) return;
    const int o = (int)(i >> 10), k = (int)(i & 1023);
    if (k > R2L_IN) return;
    float s = 0.f;
    for (int sidx = 0; sidx < n_slices; ++sidx) s += slab[(int64_t)sidx * (R2L_W * 1024) + i];
    if (k == R2L_IN) grads[r2l_off_head_b() + o] += s;  // column 1008 carries the bias partials
    else grads[(int64_t)o * R2L_IN + k] += s;
}

int r2l_dw_head_launch(R2LDwHeadArgs a, int64_t slices, bool dw_head16, const unsigned* status, bool no_fallback,
                       hipStream_t stream) {
    const dim3 hg((unsigned)(slices * 4)), hb(256);
    if (dw_head16) {
        // default trio: the same GEMM on the fp16 matrix pipe (r2l_dw_head16.hip); the fp32 kernel behind it runs only when
        // the dX chain raised its status word (range guard / bf16x3 fallback step)
        a.run_unless = status;
        if (const int rc = r2l_dw_head16_launch(a, slices, stream)) return rc;
        a.run_unless = nullptr;
        a.run_if = status;
    }
    if (dw_head16 && no_fallback) {
    } else if (a.emb != nullptr) hipLaunchKernelGGL((r2l_dw_head_kernel<true, false>), hg, hb, 0, stream, a);
    else if (a.t_rand != nullptr) hipLaunchKernelGGL((r2l_dw_head_kernel<false, true>), hg, hb, 0, stream, a);
    else hipLaunchKernelGGL((r2l_dw_head_kernel<false, false>), hg, hb, 0, stream, a);
    R2L_CHECK(hipGetLastError());
    if (a.slab) {
        hipLaunchKernelGGL(r2l_head_reduce_kernel, dim3(R2L_W * 1024 / 256), dim3(256), 0, stream, a.slab, (int)slices, a.grads);
        R2L_CHECK(hipGetLastError());
    }
    return 0;
}
