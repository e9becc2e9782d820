// r2l_dw_body.hip — weight gradients of the 2*n_block body layers: dW[l] = G[l]^T A[l] (reduction over rays) + db, on the fp32
// MFMA (r2l_dw_body_kernel), on the bf16 matrix pipe at fp32 accuracy (r2l_dw_body3_kernel: row-major stash,
// r2l_dw_body3c_kernel: chunked stash of the bf16x3 chains) and the slab reduce all of them share with r2l_dw16.hip.
// r2l_dw_body_launch runs the stage: the kernel the plan names (the default trio: r2l_dw16.hip with r2l_dw_body3c_kernel behind
// it as fallback), then the reduce.
#include "r2l_dispatch.h"
#include "r2l_dw.h"

// =================================================================================================================
// Weight gradients of the 2*n_block body layers:   dW[l][o][i] = sum_r G_l[r][o] * A_l[r][i],   db[l][o] = sum_r G_l[r][o]
//   layer (b,0): G = gt[b]   , A = x_b    ;   layer (b,2): G = gx[b+1] , A = t_b
// One workgroup (4 waves, one per SIMD) accumulates a full 256x256 tile set: wave (wo,wi) owns output rows
// wo*128 + 4*i + e (e = 0..3: four 32-row MFMA tiles) x input columns wi*128 + 4*i' + e'.  An MFMA k-step consumes two
// rays (lanes 0-31 ray 2s, lanes 32-63 ray 2s+1); each lane feeds its 4 tiles from ONE 16-byte load per operand:
// 512 contiguous bytes per half-wave.  The (layer, ray-chunk) work list is cut into equal contiguous ranges, one per
// workgroup.  A range touches at most two layers; the workgroup stores its partial (dW, db) of each with plain coalesced
// stores into its own slab slots and r2l_dw_reduce_kernel adds the partials of a layer to the gradient in workgroup
// order: deterministic, and ~0.2 ms cheaper per step than the 65 536 scattered fp32 atomics per flush it replaced
// (which remain as the dw_slab == NULL path).  The gradient buffer is zeroed by the caller (accumulation for free).
// =================================================================================================================

__device__ __forceinline__ void dw_flush(f32x16 (&acc)[4][4], f32x4& bsum, float* __restrict__ gw, float* __restrict__ gb,
                                         int wo, int wi, int lane) {
    const int jl = lane & 31, hh = lane >> 5;
#pragma unroll
    for (int eo = 0; eo < 4; ++eo)
#pragma unroll
        for (int ei = 0; ei < 4; ++ei)
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                // D[row][col]: row = (c&3) + 8*(c>>2) + 4*hh -> output feature index within the tile, col = jl -> input
                const int ro = (c & 3) + 8 * (c >> 2) + 4 * hh;
                const int o = wo * 128 + 4 * ro + eo;
                const int i = wi * 128 + 4 * jl + ei;
                atomicAdd(gw + o * R2L_W + i, acc[eo][ei][c]);
                acc[eo][ei][c] = 0.f;
            }
    if (wi == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float s = bsum[e] + __shfl_xor(bsum[e], 32);
            if (hh == 0) atomicAdd(gb + wo * 128 + 4 * jl + e, s);
        }
    }
    bsum = f32x4{0.f, 0.f, 0.f, 0.f};
}

// Same partial tile, written with plain coalesced 16-byte stores into this workgroup's slab slot (every element exactly
// once: lanes (jl, hh) of wave (wo, wi) own rows wo*128 + 4*ro + eo, columns wi*128 + 4*jl .. +3).
__device__ __forceinline__ void dw_flush_slab(f32x16 (&acc)[4][4], f32x4& bsum, float* __restrict__ sl, int wo, int wi,
                                              int lane) {
    const int jl = lane & 31, hh = lane >> 5;
#pragma unroll
    for (int eo = 0; eo < 4; ++eo)
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const int ro = (c & 3) + 8 * (c >> 2) + 4 * hh;
            const int o = wo * 128 + 4 * ro + eo;
            const f32x4 v = {acc[eo][0][c], acc[eo][1][c], acc[eo][2][c], acc[eo][3][c]};
            *reinterpret_cast<f32x4*>(sl + o * R2L_W + wi * 128 + 4 * jl) = v;
#pragma unroll
            for (int ei = 0; ei < 4; ++ei) acc[eo][ei][c] = 0.f;
        }
    if (wi == 0) {
        f32x4 sv;
#pragma unroll
        for (int e = 0; e < 4; ++e) sv[e] = bsum[e] + __shfl_xor(bsum[e], 32);
        if (hh == 0) *reinterpret_cast<f32x4*>(sl + R2L_W * R2L_W + wo * 128 + 4 * jl) = sv;
    }
    bsum = f32x4{0.f, 0.f, 0.f, 0.f};
}

// grads[layer] += sum of the workgroup partials of that layer, added in workgroup order (deterministic).  Workgroup w
// covered units [w*upw, (w+1)*upw): its first layer is (w*upw)/upl and a layer's partial sits in slot layer - first.
__global__ __launch_bounds__(256) void r2l_dw_reduce_kernel(const float* __restrict__ slab, float* __restrict__ grads,
                                                            int64_t upl, int64_t upw, int64_t wgs, int layer0) {
    const int layer = blockIdx.y;  // relative to layer0, like the work list
    const int i4 = blockIdx.x * 256 + threadIdx.x;
    if (i4 >= DW_SLAB_FLOATS / 4) return;
    const int64_t w0 = ((int64_t)layer * upl) / upw;
    int64_t w1 = ((int64_t)(layer + 1) * upl - 1) / upw;
    if (w1 > wgs - 1) w1 = wgs - 1;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int64_t w = w0; w <= w1; ++w) {
        const int slot = layer - (int)((w * upw) / upl);
        s += *reinterpret_cast<const f32x4*>(slab + (w * 2 + slot) * (int64_t)DW_SLAB_FLOATS + 4 * i4);
    }
    f32x4* g = reinterpret_cast<f32x4*>(grads + r2l_off_body_w(layer0 + layer)) + i4;
    *g = *g + s;
}

__global__ __launch_bounds__(256, 1) void r2l_dw_body_kernel(const R2LDwArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wo = wave >> 1, wi = wave & 1;
    const int hh = lane >> 5, jl = lane & 31;
    const int64_t total = a.units_per_layer * a.n_layers;
    int64_t u0 = (int64_t)blockIdx.x * a.units_per_wg;
    int64_t u1 = u0 + a.units_per_wg;
    if (u1 > total) u1 = total;
    if (u0 >= u1) return;

    f32x16 acc[4][4];
#pragma unroll
    for (int eo = 0; eo < 4; ++eo)
#pragma unroll
        for (int ei = 0; ei < 4; ++ei)
#pragma unroll
            for (int c = 0; c < 16; ++c) acc[eo][ei][c] = 0.f;
    f32x4 bsum = {0.f, 0.f, 0.f, 0.f};

    int64_t u = u0;
    const int first_layer = a.layer0 + (int)(u0 / a.units_per_layer);
    while (u < u1) {
        const int layer = a.layer0 + (int)(u / a.units_per_layer);
        const int64_t cu = u % a.units_per_layer;
        int64_t cend = cu + (u1 - u);
        if (cend > a.units_per_layer) cend = a.units_per_layer;
        const int b = layer >> 1;
        const int64_t Np = R2L_PAD_ROWS(a.N);
        const float* G = (layer & 1) ? a.gx + (int64_t)(b + 1) * Np * R2L_W : a.gt + (int64_t)b * Np * R2L_W;
        const float* A = (layer & 1) ? a.save_t + (int64_t)b * Np * R2L_W : a.save_x + (int64_t)b * Np * R2L_W;
        const int64_t r0 = cu * DW_CHUNK;
        int64_t r1 = cend * DW_CHUNK;
        if (r1 > a.N) r1 = a.N;
        const float* gp = G + (int64_t)wo * 128 + 4 * jl;
        const float* ap = A + (int64_t)wi * 128 + 4 * jl;
        // Software pipeline without predicates: operands of k-step s+2 are loaded (row index clamped into the
        // segment, so the loads are unconditional and hipcc can use counted vmcnt waits) while k-step s computes.
        const int64_t nfull = (r1 - r0) / 2;  // k-steps with both rays present
        // operands through buffer descriptors based at the segment start (SGPR base + 32-bit offsets: the 64-bit VGPR
        // address form costs MFMA issue slots); per-lane part in voff, the k-step position in the scalar offset
        const __amdgpu_buffer_rsrc_t grs =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(G + r0 * R2L_W), 0, 0xffffffff, 0x00020000);
        const __amdgpu_buffer_rsrc_t ars =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(A + r0 * R2L_W), 0, 0xffffffff, 0x00020000);
        const unsigned gvo = (unsigned)(hh * R2L_W + wo * 128 + 4 * jl) * 4u;
        const unsigned avo = (unsigned)(hh * R2L_W + wi * 128 + 4 * jl) * 4u;
        auto ld = [&](int64_t s, f32x4& gv, f32x4& av) {
            const int64_t sc = s < nfull ? s : (nfull > 0 ? nfull - 1 : 0);
            const unsigned so = (unsigned)sc * (2u * R2L_W * 4u);
            gv = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(grs, gvo, so, 0));
            av = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ars, avo, so, 0));
        };
        auto kstep = [&](const f32x4& gv, const f32x4& av) {
#pragma unroll
            for (int eo = 0; eo < 4; ++eo)
#pragma unroll
                for (int ei = 0; ei < 4; ++ei)
                    acc[eo][ei] = __builtin_amdgcn_mfma_f32_32x32x2f32(gv[eo], av[ei], acc[eo][ei], 0, 0, 0);
            bsum += gv;
        };
        if (nfull > 0) {
            // 4 rotating operand buffers, each reloaded right after the k-step that consumed it: every load is issued
            // three k-steps (3072 MFMA cycles) before its use, with no register copies.  The loop body is a whole
            // 64-ray chunk (32 k-steps) because hipcc drains vmcnt to 0 at every loop header.
            f32x4 gb[DW_DEPTH], ab[DW_DEPTH];
#pragma unroll
            for (int k = 0; k < DW_DEPTH; ++k) ld(k, gb[k], ab[k]);
#ifdef DW_SCHED_V1  // rounds 1 - 5 (A/B builds): the buffer a k-step consumed is refilled BEHIND its 16 MFMAs
            int64_t s = 0;
            // hipcc drains vmcnt to 0 at every loop header, which exposes the full HBM latency of the newest load (~2 us):
            // long trips amortise it (one drain per 2048 / 1024 / 512 MFMAs)
#define DW_TRIPS(TRIP)                                                                       \
            for (; s + TRIP <= nfull; s += TRIP) {                                           \
                _Pragma("unroll") for (int k = 0; k < TRIP; ++k) {                           \
                    kstep(gb[k % DW_DEPTH], ab[k % DW_DEPTH]);                               \
                    ld(s + k + DW_DEPTH, gb[k % DW_DEPTH], ab[k % DW_DEPTH]);                \
                    __builtin_amdgcn_sched_barrier(0);                                       \
                }                                                                            \
            }
#else
            // Round 6.  With one wave per SIMD nothing else fills the issue port, and the round-5 loop put a k-step's two loads, its
            // clamp (a 64-bit VALU compare + three scalar ops) and the four bias adds in a lump BEHIND its 16 MFMAs (they could not go
            // earlier: the loads overwrite the operands those MFMAs read): ~130 issue cycles against the 64 the last MFMA covers —
            // the matrix pipe idled ~11 % of the kernel (PMC: 88.9 % busy at 2.39 GHz, 1152 cycles per k-step instead of 1024).
            // Now the buffer consumed ONE K-STEP AGO is refilled under this k-step's MFMAs (same look-ahead: three k-steps), the
            // clamp is one s_min_i32; the loads issue in the shadow of the previous k-step's last MFMA, the bias adds among this one's.  (The first k-step
            // of a segment refills the last prologue buffer with the data it already holds: one redundant load pair per segment.)
            const int nfull32 = (int)nfull;
            auto ldi = [&](int s32, f32x4& gv, f32x4& av) {
                const int sc = s32 < nfull32 ? s32 : nfull32 - 1;
                const unsigned so = (unsigned)sc * (2u * R2L_W * 4u);
                gv = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(grs, gvo, so, 0));
                av = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ars, avo, so, 0));
            };
            int s = 0;
            // (not pinned with sched_group_barrier: with [2 MFMA, 1 load] x 2 in front hipcc moved accumulators between VGPRs and AGPRs in
            // every k-step — 7000 v_accvgpr moves per 128 k-steps)
#define DW_TRIPS(TRIP)                                                                                                   \
            for (; s + TRIP <= nfull32; s += TRIP) {                                                                     \
                _Pragma("unroll") for (int k = 0; k < TRIP; ++k) {                                                       \
                    ldi(s + k - 1 + DW_DEPTH, gb[(k + DW_DEPTH - 1) % DW_DEPTH], ab[(k + DW_DEPTH - 1) % DW_DEPTH]);     \
                    kstep(gb[k % DW_DEPTH], ab[k % DW_DEPTH]);                                                           \
                    __builtin_amdgcn_sched_barrier(0);                                                                   \
                }                                                                                                        \
            }
#endif
            DW_TRIPS(DW_LONG_TRIP)
            DW_TRIPS(64)
            DW_TRIPS(32)
#undef DW_TRIPS
            for (; s < nfull; ++s) {  // remainder: only the last, partial chunk at the end of N
                f32x4 gv, av;
                ld(s, gv, av);
                kstep(gv, av);
            }
        }
        if ((r1 - r0) & 1) {  // odd tail (only at the very end of N): the second ray of the pair does not exist
            const int64_t r = r1 - 1;
            f32x4 gv = *reinterpret_cast<const f32x4*>(gp + r * R2L_W);
            f32x4 av = *reinterpret_cast<const f32x4*>(ap + r * R2L_W);
            if (hh) { gv = f32x4{0.f, 0.f, 0.f, 0.f}; av = gv; }
            kstep(gv, av);
        }
#ifdef DW_NO_FLUSH  // diagnostics build only
        if (a.N < 0) dw_flush_slab(acc, bsum, a.slab, wo, wi, lane);
#else
        if (a.slab != nullptr) {
            dw_flush_slab(acc, bsum, a.slab + ((int64_t)blockIdx.x * 2 + (layer - first_layer)) * DW_SLAB_FLOATS, wo, wi,
                          lane);
        } else {
            float* gw = a.grads + r2l_off_body_w(layer);
            float* gb = a.grads + r2l_off_body_b(layer);
            dw_flush(acc, bsum, gw, gb, wo, wi, lane);
        }
#endif
        u += cend - cu;
    }
}

// =================================================================================================================
// The same GEMMs on the bf16 matrix pipe at fp32 accuracy (scheme of r2l_fwd3.hip: every fp32 operand value is the exact sum
// of three bf16 numbers, six bf16 products stand for one fp32 product).  Both operands are activations, so both are split
// here, on the VALU: one k-step is 16 rays; a lane loads the 4-feature pieces of its 8 rays for both operands (16 x 16 B),
// splits the 64 values (packed v_cvt_pk_bf16_f32 + shift/mask + subtract) and issues 16 tiles x 6 = 96 MFMAs.  The rows
// past N of a slot are exact zeros in the gradient operands (the chains write zero gradients for padding rays), so the k
// loop simply runs to the padded row count: no tails, no predicates.  Work split, accumulator layout and the slab flush are
// those of r2l_dw_body_kernel.
// =================================================================================================================
typedef __bf16 dw3_bf16x8 __attribute__((ext_vector_type(8)));
struct Dw3Split {
    dw3_bf16x8 h, m, l;
};
__device__ __forceinline__ unsigned dw3_pk(float a0, float a1) {
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a0, a1}, bf16x2));
}
__device__ __forceinline__ float dw3_lo(unsigned u) { return __builtin_bit_cast(float, u << 16); }
__device__ __forceinline__ float dw3_hi(unsigned u) { return __builtin_bit_cast(float, u & 0xffff0000u); }
// component e of the eight loaded pieces (8 rays) -> bf16 (hi, mid, lo) operand registers
__device__ __forceinline__ Dw3Split dw3_split(const f32x4 (&v)[8], int e) {
    u32x4 uh, um, ul;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const float x0 = v[2 * p][e], x1 = v[2 * p + 1][e];
        const unsigned h = dw3_pk(x0, x1);
        const float r0 = x0 - dw3_lo(h), r1 = x1 - dw3_hi(h);
        const unsigned m = dw3_pk(r0, r1);
        const unsigned l = dw3_pk(r0 - dw3_lo(m), r1 - dw3_hi(m));
        uh[p] = h; um[p] = m; ul[p] = l;
    }
    Dw3Split s;
    s.h = __builtin_bit_cast(dw3_bf16x8, uh);
    s.m = __builtin_bit_cast(dw3_bf16x8, um);
    s.l = __builtin_bit_cast(dw3_bf16x8, ul);
    return s;
}

__global__ __launch_bounds__(256, 1) void r2l_dw_body3_kernel(const R2LDwArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wo = wave >> 1, wi = wave & 1;
    const int hh = lane >> 5, jl = lane & 31;
    const int64_t total = a.units_per_layer * a.n_layers;
    int64_t u0 = (int64_t)blockIdx.x * a.units_per_wg;
    int64_t u1 = u0 + a.units_per_wg;
    if (u1 > total) u1 = total;
    if (u0 >= u1) return;

    f32x16 acc[4][4];
#pragma unroll
    for (int eo = 0; eo < 4; ++eo)
#pragma unroll
        for (int ei = 0; ei < 4; ++ei)
#pragma unroll
            for (int c = 0; c < 16; ++c) acc[eo][ei][c] = 0.f;
    f32x4 bsum = {0.f, 0.f, 0.f, 0.f};
    const int64_t Np = R2L_PAD_ROWS(a.N);

    int64_t u = u0;
    const int first_layer = a.layer0 + (int)(u0 / a.units_per_layer);
    while (u < u1) {
        const int layer = a.layer0 + (int)(u / a.units_per_layer);
        const int64_t cu = u % a.units_per_layer;
        int64_t cend = cu + (u1 - u);
        if (cend > a.units_per_layer) cend = a.units_per_layer;
        const int b = layer >> 1;
        const float* G = (layer & 1) ? a.gx + (int64_t)(b + 1) * Np * R2L_W : a.gt + (int64_t)b * Np * R2L_W;
        const float* A = (layer & 1) ? a.save_t + (int64_t)b * Np * R2L_W : a.save_x + (int64_t)b * Np * R2L_W;
        const int64_t r0 = cu * DW_CHUNK;
        int64_t r1 = cend * DW_CHUNK;
        if (r1 > Np) r1 = Np;
        const int64_t nsteps = (r1 - r0) / 16;  // Np is a multiple of 32
        const __amdgpu_buffer_rsrc_t grs =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(G + r0 * R2L_W), 0, 0xffffffff, 0x00020000);
        const __amdgpu_buffer_rsrc_t ars =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(A + r0 * R2L_W), 0, 0xffffffff, 0x00020000);
        // lane (jl, hh): rays 8hh .. 8hh+7 of the 16-ray step, features 4jl .. 4jl+3 of the wave's 128-feature slice
        const unsigned gvo = (unsigned)(8 * hh * R2L_W + wo * 128 + 4 * jl) * 4u;
        const unsigned avo = (unsigned)(8 * hh * R2L_W + wi * 128 + 4 * jl) * 4u;
        auto ld = [&](int64_t s, f32x4 (&gv)[8], f32x4 (&av)[8]) {
            const int64_t sc = s < nsteps ? s : nsteps - 1;  // the prefetch behind the last step re-reads it
            const unsigned so = (unsigned)sc * (16u * R2L_W * 4u);
            // rows r < 4 via the instruction's 12-bit offset field, rows 4..7 through the scalar offset (+4096); the opaque
            // copies keep hipcc from materialising voff + const in 16 loop-invariant VGPRs
            unsigned gq = gvo, aq = avo;
            asm volatile("" : "+v"(gq), "+v"(aq));
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const unsigned ro = (unsigned)(r & 3) * (R2L_W * 4u), sx = so + (unsigned)(r >> 2) * 4096u;
                gv[r] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(grs, gq + ro, sx, 0));
                av[r] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ars, aq + ro, sx, 0));
            }
        };
        auto kstep = [&](const f32x4 (&gv)[8], const f32x4 (&av)[8]) {
            Dw3Split bs[4];
#pragma unroll
            for (int ei = 0; ei < 4; ++ei) bs[ei] = dw3_split(av, ei);
#pragma unroll
            for (int eo = 0; eo < 4; ++eo) {
                const Dw3Split as = dw3_split(gv, eo);
#pragma unroll
                for (int ei = 0; ei < 4; ++ei) acc[eo][ei] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as.l, bs[ei].h, acc[eo][ei], 0, 0, 0);
#pragma unroll
                for (int ei = 0; ei < 4; ++ei) acc[eo][ei] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as.h, bs[ei].l, acc[eo][ei], 0, 0, 0);
#pragma unroll
                for (int ei = 0; ei < 4; ++ei) acc[eo][ei] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as.m, bs[ei].m, acc[eo][ei], 0, 0, 0);
#pragma unroll
                for (int ei = 0; ei < 4; ++ei) acc[eo][ei] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as.m, bs[ei].h, acc[eo][ei], 0, 0, 0);
#pragma unroll
                for (int ei = 0; ei < 4; ++ei) acc[eo][ei] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as.h, bs[ei].m, acc[eo][ei], 0, 0, 0);
#pragma unroll
                for (int ei = 0; ei < 4; ++ei) acc[eo][ei] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as.h, bs[ei].h, acc[eo][ei], 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 8; ++r) bsum += gv[r];
        };
        if (nsteps > 0) {
            f32x4 g0[8], x0[8], g1[8], x1[8];
            ld(0, g0, x0);
            int64_t s = 0;
            for (; s + 2 <= nsteps; s += 2) {  // two steps per trip: the buffers swap roles without register copies
                ld(s + 1, g1, x1);
                kstep(g0, x0);
                ld(s + 2, g0, x0);
                kstep(g1, x1);
            }
        }
        if (a.slab != nullptr) {
            dw_flush_slab(acc, bsum, a.slab + ((int64_t)blockIdx.x * 2 + (layer - first_layer)) * DW_SLAB_FLOATS, wo, wi,
                          lane);
        } else {
            float* gw = a.grads + r2l_off_body_w(layer);
            float* gb = a.grads + r2l_off_body_b(layer);
            dw_flush(acc, bsum, gw, gb, wo, wi, lane);
        }
        u += cend - cu;
    }
}

// =================================================================================================================
// The same GEMMs fed from the CHUNKED fp32 stash of the bf16x3 chains (r2l_common.h), every operand value split ONCE per
// workgroup.  (r2l_dw_body3_kernel lets each wave load and split its own operands: every value is split by two waves, and
// the split — ~6 VALU instructions per value — is what bounds it.)
//   * one k-step = 16 rays (half a tile): per operand 32 chunks x 512 contiguous bytes.  Wave w loads chunks 8w .. 8w+7 of
//     both operands (8 x 16 B per lane: lane = (chunk parity, ray, half chunk) -> 4 consecutive features of one ray),
//     splits them into bf16 (hi, mid, lo) (packed v_cvt_pk_bf16_f32, shift / mask, subtract) and writes the three 8-byte
//     quads into the step image in LDS: [split][chunk][slot S][8 B];
//   * the MFMA operands (lane = feature, 8 consecutive rays in its 16 bytes) come out of the image through
//     ds_read_b64_tr_b16: within a 16-lane group lane L = 4*row + q supplies the address of four consecutive bf16 (ray row,
//     feature quad q) and lane l receives rows 0..3 of column l — 4 rays of feature l (measured: tools/tr_probe.hip);
//   * slot S of (ray, quad fq = 2 chunk + half) = half*16 + ((ray + 4 (chunk & 3)) & 15): the 32 lanes of a read pass (two
//     16-feature blocks x four quads x four rays) and of a write pass (16 rays x two halves) hit 32 different 8-byte slots;
//   * software pipeline per step s (two images, one barrier per step): the 4 x TERMS groups of four MFMAs of step s carry
//     along the transposing reads of step s+1 (image s+1 -> registers), the split + LDS write of step s+2 (raw registers ->
//     image s+2, which takes the buffer of image s) and the global loads of step s+3 (in place into the raw registers, one
//     step of latency cover; inline asm with hand-placed vmcnt(7) waits: hipcc would drain vmcnt to 0 at the loop header);
//   * db: the loader lanes add up their raw fp32 gradient quads (4 adds per quad); the 16 rays of a quad column are
//     combined by xor-shuffles at the flush.
// Work split, accumulators and the slab reduce are those of r2l_dw_body_kernel; tile eo of a wave's 128-feature slice is
// features 32 eo .. 32 eo + 31 here (row m of the MFMA result = feature 32 eo + m).
// (Round 1's 3-product and fp16 variants of this kernel were retired with r2l_dw16.hip.)
// =================================================================================================================
#define DW3C_OP_BYTES 24576   // one operand, one step: 3 splits x 32 chunks x 256 B
#define DW3C_BUF_BYTES 49152  // G image, A image
typedef short dw3c_s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned dw3c_u32x2 __attribute__((ext_vector_type(2)));

// 8 rays of this lane's feature: two transposing reads (rays 8hh + 0..3 at p0, 8hh + 4..7 at p1), byte offset off (a constant
// after unrolling: it ends up in the instruction's offset field)
__device__ __forceinline__ dw3_bf16x8 dw3c_read(unsigned p0, unsigned p1, unsigned off) {
    typedef __attribute__((address_space(3))) dw3c_s16x4 lds_v;
    const dw3c_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v*)(size_t)(p0 + off));
    const dw3c_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v*)(size_t)(p1 + off));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    return __builtin_bit_cast(dw3_bf16x8, s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]});
}
// the operand registers of one k-step: gs = tiles of the gradient operand (MFMA A), xs = tiles of the activation operand
struct Dw3cRegs {
    Dw3Split gs[4], xs[4];
};
// fragment F of a step (24 fragments, F < 12: activation tile F/3, split F%3, else gradient tile (F-12)/3, split (F-12)%3);
// gp / ap [t]: lane bases in the
// G / A image for ray quad t
__device__ __forceinline__ void dw3c_frag(int F, Dw3cRegs& R, const unsigned (&gp)[2], const unsigned (&ap)[2]) {
    constexpr int NS = 3;
    const bool grad = F >= 4 * NS;
    const int f = grad ? F - 4 * NS : F, e = f / NS, sp = f % NS;
    const dw3_bf16x8 val = grad ? dw3c_read(gp[0], gp[1], (unsigned)(e * 1024 + sp * 8192))
                                : dw3c_read(ap[0], ap[1], (unsigned)(e * 1024 + sp * 8192));
    Dw3Split& d = grad ? R.gs[e] : R.xs[e];
    if (sp == 0) d.h = val;
    else if (sp == 1) d.m = val;
    else d.l = val;
}
// 16-byte global load the compiler does not track (so that it does not wait for it at loop headers): the consumer waits
// with dw3c_wait7 — the loads retire in order and exactly 7 younger ones are in flight at every use
__device__ __forceinline__ void dw3c_load(f32x4& dst, u32x4 rsrc, unsigned voff, unsigned soff) {
    asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=&v"(dst) : "v"(voff), "s"(rsrc), "s"(soff) : "memory");
}
__device__ __forceinline__ void dw3c_wait7(f32x4& v) { asm volatile("s_waitcnt vmcnt(7)" : "+v"(v)::"memory"); }
__device__ __forceinline__ void dw3c_wait0(f32x4& v) { asm volatile("s_waitcnt vmcnt(0)" : "+v"(v)::"memory"); }
// split state of one raw quad (4 features of one ray)
struct Dw3cQuad {
    float r[4];
    unsigned uh[2], um[2], ul[2];
};
// part 0: hi + first residual; part 1: mid + second residual; part 2: lo
__device__ __forceinline__ void dw3c_split_part(Dw3cQuad& q, const f32x4& x, int part) {
    if (part == 0) {
        q.uh[0] = dw3_pk(x[0], x[1]);
        q.uh[1] = dw3_pk(x[2], x[3]);
        q.r[0] = x[0] - dw3_lo(q.uh[0]); q.r[1] = x[1] - dw3_hi(q.uh[0]);
        q.r[2] = x[2] - dw3_lo(q.uh[1]); q.r[3] = x[3] - dw3_hi(q.uh[1]);
    } else if (part == 1) {
        q.um[0] = dw3_pk(q.r[0], q.r[1]);
        q.um[1] = dw3_pk(q.r[2], q.r[3]);
        q.r[0] -= dw3_lo(q.um[0]); q.r[1] -= dw3_hi(q.um[0]);
        q.r[2] -= dw3_lo(q.um[1]); q.r[3] -= dw3_hi(q.um[1]);
    } else {
        q.ul[0] = dw3_pk(q.r[0], q.r[1]);
        q.ul[1] = dw3_pk(q.r[2], q.r[3]);
    }
}
__device__ __forceinline__ void dw3c_write(unsigned addr, unsigned d0, unsigned d1) {
    typedef __attribute__((address_space(3))) dw3c_u32x2 lds_u2;
    *(lds_u2*)(size_t)addr = dw3c_u32x2{d0, d1};
}

__global__ __launch_bounds__(256, 1) void r2l_dw_body3c_kernel(const R2LDwArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char img[2][DW3C_BUF_BYTES];
    constexpr int TERMS = 6;  // bf16 products per fp32 product
    if (a.run_if != nullptr && __builtin_nontemporal_load(a.run_if) == 0u) return;
    const float unscale = a.scale_dev != nullptr ? a.scale_dev[1] : a.unscale;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wo = wave >> 1, wi = wave & 1;
    const int64_t total = a.units_per_layer * a.n_layers;
    int64_t u0 = (int64_t)blockIdx.x * a.units_per_wg;
    int64_t u1 = u0 + a.units_per_wg;
    if (u1 > total) u1 = total;
    if (u0 >= u1) return;

    f32x16 acc[4][4];
#pragma unroll
    for (int eo = 0; eo < 4; ++eo)
#pragma unroll
        for (int ei = 0; ei < 4; ++ei)
#pragma unroll
            for (int c = 0; c < 16; ++c) acc[eo][ei][c] = 0.f;
    f32x4 bacc[4];  // db partials of this loader lane: gradient chunk pair kk, its 4 features, summed over its ray column
#pragma unroll
    for (int k = 0; k < 4; ++k) bacc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int64_t Np = R2L_PAD_ROWS(a.N);
    const int64_t slot = R2L_TRIO_SLOT(Np);
    const unsigned img_lds = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)&img[0][0];

    // loader lane: chunk parity cc inside the instruction's chunk pair, ray j of the half tile, half chunk hf
    const int lcc = lane >> 5, lj = (lane >> 1) & 15, lhf = lane & 1;
    const unsigned lvoff = (unsigned)(lcc * 1024 + lj * 32 + lhf * 16);
    // its write address in an operand image for instruction kk (chunk 8 wave + 2 kk + cc): [split][chunk][S][8 B];
    // (chunk & 3) = (2 kk + cc) & 3 -> two rotations, even / odd kk
    unsigned wbase[2];
#pragma unroll
    for (int par = 0; par < 2; ++par) {
        const int rot = 4 * ((2 * par + lcc) & 3);
        wbase[par] = img_lds + (unsigned)(wave * 2048 + lcc * 256 + (lhf * 16 + ((lj + rot) & 15)) * 8);
    }
    // read bases: 16-lane group (hh, par): 16-feature block parity par inside the tile, rays 8hh..; lane L = 4*row + q in it
    unsigned gb0[2], ab0[2];
    {
        const int g = lane >> 4, L = lane & 15, par = g & 1, hh = g >> 1, q = L & 3, row = L >> 2;
        const int cl = 2 * par + (q >> 1);  // chunk inside the tile's four
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int S = (q & 1) * 16 + ((8 * hh + 4 * t + row + 4 * (cl & 3)) & 15);
            const unsigned base = (unsigned)(cl * 256 + S * 8);
            gb0[t] = img_lds + base + (unsigned)wo * 4096u;
            ab0[t] = img_lds + DW3C_OP_BYTES + base + (unsigned)wi * 4096u;
        }
    }

    int64_t u = u0;
    const int first_layer = a.layer0 + (int)(u0 / a.units_per_layer);
    while (u < u1) {
        const int layer = a.layer0 + (int)(u / a.units_per_layer);
        const int64_t cu = u % a.units_per_layer;
        int64_t cend = cu + (u1 - u);
        if (cend > a.units_per_layer) cend = a.units_per_layer;
        const int b = layer >> 1;
        const float* G = (layer & 1) ? a.gx + (int64_t)(b + 1) * slot : a.gt + (int64_t)b * slot;
        const float* A = (layer & 1) ? a.save_t + (int64_t)b * slot : a.save_x + (int64_t)b * slot;
        const int64_t r0 = cu * DW_CHUNK;  // a multiple of 64 rays: two whole tiles
        int64_t r1 = cend * DW_CHUNK;
        if (r1 > Np) r1 = Np;
        const int nsteps = (int)((r1 - r0) / 16);  // Np is a multiple of 32: always even
        // descriptors based at the first tile of the segment (+ this wave's eight chunks)
        const u32x4 grs = r2l_buffer_rsrc(G + r0 * R2L_W + wave * 8 * R2L_CHUNK_PIECE);
        const u32x4 ars = r2l_buffer_rsrc(A + r0 * R2L_W + wave * 8 * R2L_CHUNK_PIECE);
        // raw quad k of a step: k < 4 gradient chunk pair k, else activation chunk pair k - 4.  Steps past the end are
        // clamped to the last one (harmless reloads: every step issues exactly 8 loads, which keeps vmcnt(7) uniform)
        f32x4 raw[8];
        auto load = [&](int s, int k) {
            const int sc = s < nsteps ? s : nsteps - 1;
            const unsigned so = (unsigned)(sc >> 1) * (unsigned)(R2L_CHUNK_TILE * 4) + (unsigned)(sc & 1) * 512u + (unsigned)(k & 3) * 2048u;
            dw3c_load(raw[k], (k < 4) ? grs : ars, lvoff, so);
        };
        Dw3cQuad qs;
        // parts of the split of raw quad k into the image in buffer `buf`; the last part writes the quads and reloads raw[k]
        // with the data of step s_next
        auto quad_part = [&](int k, int part, int buf, int s_next) {
            if (part == 0) {
                dw3c_wait7(raw[k]);
                // (raw holds step s_next - 1: a clamped reload past the end must not be counted)
                if (k < 4) bacc[k] += raw[k] * ((s_next - 1 < nsteps) ? 1.f : 0.f);
            }
            dw3c_split_part(qs, raw[k], part);
            if (part == 2) {
                const unsigned wa = wbase[k & 1] + (unsigned)buf * DW3C_BUF_BYTES + (unsigned)(k >> 2) * DW3C_OP_BYTES + (unsigned)(k & 3) * 512u;
                dw3c_write(wa, qs.uh[0], qs.uh[1]);
                dw3c_write(wa + 8192u, qs.um[0], qs.um[1]);
                dw3c_write(wa + 16384u, qs.ul[0], qs.ul[1]);
                load(s_next, k);
            }
        };
        // One k-step: 16 x TERMS MFMAs on the registers C; riding along, per group of four MFMAs: fragments of step s+1 (LDS
        // image s+1 -> registers Nx) and a part of the split of step s+2 (raw -> image s+2 in the buffer image s occupied;
        // raw reloaded with step s+3)
        auto step = [&](Dw3cRegs& C, Dw3cRegs& Nx, int s, int buf) {
            // image s+1 is complete (everybody wrote its share during step s-1) and nobody reads image s any more
            __syncthreads();
            const unsigned bo = (unsigned)(buf ^ 1) * DW3C_BUF_BYTES;  // image of step s+1
            const unsigned gp[2] = {gb0[0] + bo, gb0[1] + bo}, ap[2] = {ab0[0] + bo, ab0[1] + bo};
#pragma unroll
            for (int g = 0; g < 4 * TERMS; ++g) {
                const int eo = g / TERMS, term = g % TERMS;
                // small terms first: (l,h) (h,l) (m,m) (m,h) (h,m) (h,h)
                const int tk = term;
                const dw3_bf16x8& ga2 = (tk == 0) ? C.gs[eo].l : (tk == 2 || tk == 3) ? C.gs[eo].m : C.gs[eo].h;
#pragma unroll
                for (int ei = 0; ei < 4; ++ei) {
                    const dw3_bf16x8& xb = (tk == 1) ? C.xs[ei].l : (tk == 2 || tk == 4) ? C.xs[ei].m : C.xs[ei].h;
                    acc[eo][ei] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ga2, xb, acc[eo][ei], 0, 0, 0);
                }
                // 24 groups: 24 fragments, 8 quads x 3 parts
                dw3c_frag(g, Nx, gp, ap);
                quad_part(g / 3, g % 3, buf, s + 3);
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        if (nsteps > 0) {
            Dw3cRegs RA, RB;
            // prologue: images 0 and 1, raw = step 2 (latencies exposed once per segment)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
#pragma unroll
                for (int k = 0; k < 8; ++k) load(s, k);
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    dw3c_wait0(raw[k]);
                    if (k < 4) bacc[k] += raw[k];
#pragma unroll
                    for (int part = 0; part < 3; ++part) dw3c_split_part(qs, raw[k], part);
                    const unsigned wa = wbase[k & 1] + (unsigned)s * DW3C_BUF_BYTES + (unsigned)(k >> 2) * DW3C_OP_BYTES + (unsigned)(k & 3) * 512u;
                    dw3c_write(wa, qs.uh[0], qs.uh[1]);
                    dw3c_write(wa + 8192u, qs.um[0], qs.um[1]);
                    dw3c_write(wa + 16384u, qs.ul[0], qs.ul[1]);
                }
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) load(2, k);
            __syncthreads();
#pragma unroll
            for (int F = 0; F < 24; ++F) dw3c_frag(F, RA, gb0, ab0);  // step 0 from buffer 0
            for (int s = 0; s < nsteps; s += 2) {
                step(RA, RB, s, 0);
                step(RB, RA, s + 1, 1);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();  // the images are dead (and the clamped reloads landed) before the next segment refills them
        }
        // flush: D[m][n] of tile (eo, ei): m = 8 (c>>2) + 4 hh + (c&3) -> output feature wo*128 + 32 eo + m, n = lane & 31 ->
        // input feature wi*128 + 32 ei + n
        {
            const int n = lane & 31, hh = lane >> 5;
            float* sl = (a.slab != nullptr) ? a.slab + ((int64_t)blockIdx.x * 2 + (layer - first_layer)) * DW_SLAB_FLOATS : nullptr;
            float* gw = a.grads + r2l_off_body_w(layer);
            float* gbias = a.grads + r2l_off_body_b(layer);
            float* rowp = (sl != nullptr ? sl : gw) + (wo * 128 + 4 * hh) * R2L_W + wi * 128 + n;
            if (sl != nullptr) {
#pragma unroll
                for (int eo = 0; eo < 4; ++eo)
#pragma unroll
                    for (int ei = 0; ei < 4; ++ei)
#pragma unroll
                        for (int c = 0; c < 16; ++c) {
                            rowp[(32 * eo + 8 * (c >> 2) + (c & 3)) * R2L_W + 32 * ei] = acc[eo][ei][c] * unscale;
                            acc[eo][ei][c] = 0.f;
                        }
            } else {
#pragma unroll
                for (int eo = 0; eo < 4; ++eo)
#pragma unroll
                    for (int ei = 0; ei < 4; ++ei)
#pragma unroll
                        for (int c = 0; c < 16; ++c) {
                            atomicAdd(rowp + (32 * eo + 8 * (c >> 2) + (c & 3)) * R2L_W + 32 * ei, acc[eo][ei][c] * unscale);
                            acc[eo][ei][c] = 0.f;
                        }
            }
            // db: loader lane (cc, j, hf) holds, for kk = 0..3, features 8 (8 wave + 2 kk + cc) + 4 hf .. +3 summed over its ray
            // column j; the 16 columns sit in lane bits 1..4
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                f32x4 v = bacc[k];
#pragma unroll
                for (int m = 2; m <= 16; m <<= 1)
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] += __shfl_xor(v[e], m);
                v *= unscale;
                if (lj == 0) {
                    const int f = 8 * (8 * wave + 2 * k + lcc) + 4 * lhf;
                    if (sl != nullptr) *reinterpret_cast<f32x4*>(sl + R2L_W * R2L_W + f) = v;
                    else
#pragma unroll
                        for (int e = 0; e < 4; ++e) atomicAdd(gbias + f + e, v[e]);
                }
                bacc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
        u += cend - cu;
    }
}

int r2l_dw_body_launch(R2LDwArgs a, int dw_body, int64_t wgs, unsigned* status, bool no_fallback, hipStream_t stream) {
    const dim3 grid((unsigned)wgs), block(256);
    // bf16 matrix pipe at fp32 accuracy: operands split once per workgroup from the chunked stash of the bf16x3 chains
    // (r2l_dw_body3c), or per wave from the row-major stash of the other chains (R2L_NO_FWD3: fp32 MFMA)
    if (dw_body == R2L_DWBODY_DW16) {
        // default trio: one fp16 product per fp32 product on the fp16 stage pieces the chains stashed (r2l_dw16.hip; a.mid_off:
        // with their mid halves); when the dX chain raised its status word (this step fell back to the bf16x3 chains and their
        // fp32 stash) it returns at once and the bf16x3 kernel behind it does the work
        a.act_scale = a.save_x + R2L_STASH_FMT_WORD(a.n_block, R2L_PAD_ROWS(a.N)) + 1;  // the scale the forward stashed x, relu(t) at
        if (const int rc = r2l_dw16_launch(a, wgs, status, stream)) return rc;
        a.mid_off = 0u;
        a.act_scale = nullptr;
        a.run_if = status;
        if (!no_fallback) hipLaunchKernelGGL(r2l_dw_body3c_kernel, grid, block, 0, stream, a);
    } else if (dw_body == R2L_DWBODY_BODY3C) hipLaunchKernelGGL(r2l_dw_body3c_kernel, grid, block, 0, stream, a);
    else if (dw_body == R2L_DWBODY_BODY3) hipLaunchKernelGGL(r2l_dw_body3_kernel, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(r2l_dw_body_kernel, grid, block, 0, stream, a);
    R2L_CHECK(hipGetLastError());
    if (a.slab != nullptr) {
        hipLaunchKernelGGL(r2l_dw_reduce_kernel, dim3((DW_SLAB_FLOATS / 4 + 255) / 256, a.n_layers), dim3(256), 0, stream,
                           a.slab, a.grads, a.units_per_layer, a.units_per_wg, wgs, a.layer0);
        R2L_CHECK(hipGetLastError());
    }
    return 0;
}
