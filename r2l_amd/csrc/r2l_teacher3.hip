// r2l_teacher3.hip — the fused NeRF-teacher point network (run_network + NeRF.forward, see r2l_teacher_mlp.hip) at fp32
// accuracy on the bf16 matrix pipe: same scheme as r2l_fwd3.hip (bf16 hi/mid/lo triples, six MFMAs per product, LDS-DMA
// staged weight stream, machinery in r2l_f3.h), one wavefront = 32 consecutive sample points.
//
// Stage stream (24 KiB stages: 16 input features x 256 outputs x 3 splits; "bias" = one-MFMA-per-tile bias stage):
//   L0:   bias, 4 xyz-embedding blocks
//   4 x : t-layer (L1, L3, L5, L7): bias, [L5: 4 xyz-embedding blocks], 16 blocks of relu(x)
//         x-layer (L2, L4, L6, feature): bias, 16 blocks of relu(t)
//   views: bias, 16 blocks of the feature (no ReLU), 2 direction-embedding blocks; its 128 outputs occupy tiles 0-3 of the
//          stage, tiles 4-7 are zero padding (9 of 164 stages cost twice what they could; kept for one uniform stage routine)
// alpha (on relu(L7)) and rgb (on relu(views)) stay on the VALU as in the fp32 kernel.
// Embedding k order per half-wave h: xyz: 15 (sin, cos) pairs (frequency 5h + q/3, axis q%3), then the identity (h = 0: x,
// y; h = 1: z, pad);  direction: 6 pairs (frequency 2h + q/3), identity (x, y | z, pad), 2 pads.
#include "r2l_f3.h"
#include "r2l_teacher_net.h"

#define T3_STAGES 164

// =================================================================================================================
// pack
// =================================================================================================================
__global__ void r2l_pack_teacher3_kernel(const float* __restrict__ params, unsigned short* __restrict__ out) {
    const TOff off = t_offsets();
    const int64_t total = (int64_t)(T3_STAGES + R2L_F3_PAD_STAGES) * 8 * 64 * 8;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int s = (int)(idx & 7), lane = (int)((idx >> 3) & 63), tile = (int)((idx >> 9) & 7);
        const int g = (int)(idx >> 12);
        const int i = lane & 31, h = lane >> 5, o = 32 * tile + i;
        unsigned short* st = out + (int64_t)g * (F3_STAGE_BYTES / 2);
        // the stage: 0..144 as r2l_teacher_net.h has them, then the views layer (kind 3 feature block, 4 direction block);
        // kind -1: stream padding
        const T16Stage d = t16_body_stage(g, off);
        int kind = d.kind, layer = d.layer, kb = d.kb;
        int64_t boff = d.boff;
        bool views = false;
        if (g >= T16_BODY_STAGES && g < T3_STAGES) {
            const int r = g - T16_BODY_STAGES;
            views = true;
            if (r == 0) { kind = 0; boff = off.views_b; }
            else if (r <= 16) { kind = 3; kb = r - 1; }
            else { kind = 4; kb = r - 17; }
        }
        float w = 0.f;
        bool have = false;
        if (kind == 0) {
            if (!views || tile < 4) { w = params[boff + o]; have = true; }
        } else if (kind == 1) {
            const int col = t16_emb_col(8 * kb + s, h, 5);
            if (col >= 0) { w = layer == 5 ? params[off.w[5] + (int64_t)o * (T_W + T_XYZ) + col] : params[off.w[0] + (int64_t)o * T_XYZ + col]; have = true; }
        } else if (kind == 2) {
            const int T = kb >> 1, r = kb & 1;
            const int in = 32 * T + 8 * (2 * r + (s >> 2)) + 4 * h + (s & 3);
            if (layer == 8) w = params[off.feat_w + (int64_t)o * T_W + in];
            else if (layer == 5) w = params[off.w[5] + (int64_t)o * (T_W + T_XYZ) + T_XYZ + in];
            else w = params[off.w[layer] + (int64_t)o * T_W + in];
            have = true;
        } else if (kind == 3) {
            const int T = kb >> 1, r = kb & 1;
            const int in = 32 * T + 8 * (2 * r + (s >> 2)) + 4 * h + (s & 3);
            if (tile < 4) { w = params[off.views_w + (int64_t)o * (T_W + T_DIR) + in]; have = true; }
        } else if (kind == 4) {
            const int col = t16_emb_col(8 * kb + s, h, 2);
            if (tile < 4 && col >= 0) { w = params[off.views_w + (int64_t)o * (T_W + T_DIR) + T_W + col]; have = true; }
        }
        unsigned short v0 = 0, v1 = 0, v2 = 0;
        if (have) {
            const unsigned short hi = f3_bf16_rne(w);
            const float r1 = w - f3_bf16_to_f(hi);
            const unsigned short mid = f3_bf16_rne(r1);
            const unsigned short lo = f3_bf16_rne(r1 - f3_bf16_to_f(mid));
            if (kind == 0) {
                v0 = (h == 0) ? (s == 0 ? hi : (s == 1 ? mid : (s == 2 ? lo : (unsigned short)0))) : (unsigned short)0;
            } else {
                v0 = hi; v1 = mid; v2 = lo;
            }
        }
        const int64_t e = ((int64_t)tile * 64 + lane) * 8 + s;
        st[e] = v0;
        st[8 * 64 * 8 + e] = v1;
        st[2 * 8 * 64 * 8 + e] = v2;
    }
}

// =================================================================================================================
// kernel
// =================================================================================================================
// either of two gatherers, chosen at run time (the stage in front of a conditionally inserted group of stages)
template <class GA, class GB>
struct T3Select {
    bool first;
    GA ga;
    GB gb;
    __device__ __forceinline__ void operator()(float (&v)[4]) const {
        float w[4];
        ga(v);
        gb(w);
#pragma unroll
        for (int s = 0; s < 4; ++s) v[s] = first ? v[s] : w[s];
    }
};

// LIVE: the launch form on an index list with a device count (r2l_teacher_net.h "live form")
template <bool LIVE>
__global__ __launch_bounds__(256, 1) void r2l_teacher3_kernel(const T16Args a) {
    __shared__ __attribute__((aligned(16))) unsigned char wbuf[F3_NBUF][F3_STAGE_BYTES];
    if (a.run_if != nullptr && __builtin_nontemporal_load(a.run_if) == 0u) return;
    int64_t n_pts = a.n_pts;
    if constexpr (LIVE) {
        n_pts = t_live_count(a.count_dev, a.n_pts);
        if (t_live_workgroup_idle(n_pts)) return;
    }
    const TOff off = t_offsets();
    const int lane = threadIdx.x & 63, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t tile = (int64_t)blockIdx.x * 4 + wave;
    const int64_t pt = tile * R2L_TILE_RAYS + (lane & 31);
    bool valid = pt < n_pts;
    int64_t pc = valid ? pt : n_pts - 1;
    int live_n = 0;  // LIVE: the sample this lane stores (< 2^31: one register across the chain, not the 64-bit pair)
    if constexpr (LIVE) live_n = (int)(pc = t_live_sample(a.idx, n_pts, a.n_out, pt, valid));
    const int64_t ray = pc / a.S;

    float p[3], vd[3];
    {
        const float z = a.z[pc];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            p[k] = a.rays_o[ray * 3 + k] + a.rays_d[ray * 3 + k] * z;  // create_data.py:484, mul/add rounded separately
            vd[k] = a.viewdirs[ray * 3 + k];
        }
    }
    const float* P0 = a.params;

    F3Pipe P;
    P.init(a.stream, &wbuf[0][0], lane, wave);
    P.issue(); P.issue(); P.issue(); P.issue(); P.issue();
#pragma unroll
    for (int k = 0; k < 8; ++k) P.ones.h[k] = (__bf16)((h == 0 && k < 3) ? 1.0f : 0.0f);
    P.ones.m = P.ones.h;
    P.ones.l = P.ones.h;

    f32x16 x[R2L_NT], t[R2L_NT];
    asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
    __syncthreads();
    P.lb = P.base + lane * 16;
    {
        F3None none;
        F3Side<true, F3None> s0{P.a1, P.lb, 0, none, false, F3Dma{false, P.rs, 0u, 0u, 0u}};
#pragma unroll
        for (int i = 0; i < 6; ++i) s0.step(i);
    }
    P.sb = P.ones;

    typedef T16Emb4<5> Xyz4;
    typedef T16Emb4<2> Dir4;
    typedef F3Take4<true> Relu4;
    // ---- layer 0: x = W0 pe + b0 (pre-activation; every consumer applies the ReLU to its B values) ---------------------
    f3_stage<true, true, false>(x, P, Xyz4{p, h, 0}, Xyz4{p, h, 4});
    f3_stage<false, false, false>(x, P, Xyz4{p, h, 8}, Xyz4{p, h, 12});
    f3_stage<false, false, false>(x, P, Xyz4{p, h, 16}, Xyz4{p, h, 20});
    f3_stage<false, false, false>(x, P, Xyz4{p, h, 24}, Xyz4{p, h, 28});
    f3_stage<false, false, true>(x, P, F3None{}, F3None{});

    // ---- (L1,L2) (L3,L4) (L5,L6) (L7,feature): t = W_odd relu(x) [+ W5pe pe] + b ; x = W_even relu(t) + b -----------------
    float alpha = 0.f;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        {
            // opaque copies: keeps hipcc from hoisting the (loop-invariant) sin/cos values of the k == 2 branch out of the loop
            float pp[3] = {p[0], p[1], p[2]};
            int hh = h;
            asm volatile("" : "+v"(pp[0]), "+v"(pp[1]), "+v"(pp[2]), "+v"(hh));
            f3_stage<true, true, false>(t, P, T3Select<Xyz4, Relu4>{k == 2, Xyz4{pp, hh, 0}, Relu4{x[0], 0, nullptr, 0}},
                                        T3Select<Xyz4, Relu4>{k == 2, Xyz4{pp, hh, 4}, Relu4{x[0], 4, nullptr, 0}});
            if (k == 2) {
                f3_stage<false, false, false>(t, P, Xyz4{pp, hh, 8}, Xyz4{pp, hh, 12});
                f3_stage<false, false, false>(t, P, Xyz4{pp, hh, 16}, Xyz4{pp, hh, 20});
                f3_stage<false, false, false>(t, P, Xyz4{pp, hh, 24}, Xyz4{pp, hh, 28});
                f3_stage<false, false, false>(t, P, Relu4{x[0], 0, nullptr, 0}, Relu4{x[0], 4, nullptr, 0});
            }
        }
#pragma unroll
        for (int kb = 0; kb < 15; ++kb)
            f3_stage<false, false, false>(t, P, Relu4{x[(kb + 1) >> 1], 8 * ((kb + 1) & 1), nullptr, 0},
                                          Relu4{x[(kb + 1) >> 1], 8 * ((kb + 1) & 1) + 4, nullptr, 0});
        f3_stage<false, false, true>(t, P, F3None{}, F3None{});
        if (k == 3) {  // alpha_linear on relu(layer 7)
            float acc = 0.f;
#pragma unroll
            for (int T = 0; T < R2L_NT; ++T)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 wv = *reinterpret_cast<const f32x4*>(P0 + off.alpha_w + 32 * T + 8 * q + 4 * h);
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc = __builtin_fmaf(wv[j], fmaxf(t[T][4 * q + j], 0.f), acc);
                }
            acc += __shfl_xor(acc, 32);
            alpha = acc + P0[off.alpha_b];
        }
        f3_stage<true, true, false>(x, P, Relu4{t[0], 0, nullptr, 0}, Relu4{t[0], 4, nullptr, 0});
#pragma unroll
        for (int kb = 0; kb < 15; ++kb)
            f3_stage<false, false, false>(x, P, Relu4{t[(kb + 1) >> 1], 8 * ((kb + 1) & 1), nullptr, 0},
                                          Relu4{t[(kb + 1) >> 1], 8 * ((kb + 1) & 1) + 4, nullptr, 0});
        f3_stage<false, false, true>(x, P, F3None{}, F3None{});  // next: the next pair's (or the views layer's) bias stage
    }

    // ---- views layer: v[128] = Wv [feature, dir-embedding] + bv in tiles 0-3 of t (ReLU applied by the rgb head) ---------
    typedef F3Take4<false> Id4;
    f3_stage<true, true, false>(t, P, Id4{x[0], 0, nullptr, 0}, Id4{x[0], 4, nullptr, 0});
#pragma unroll
    for (int kb = 0; kb < 15; ++kb)
        f3_stage<false, false, false>(t, P, Id4{x[(kb + 1) >> 1], 8 * ((kb + 1) & 1), nullptr, 0},
                                      Id4{x[(kb + 1) >> 1], 8 * ((kb + 1) & 1) + 4, nullptr, 0});
    f3_stage<false, false, false>(t, P, Dir4{vd, h, 0}, Dir4{vd, h, 4});
    f3_stage<false, false, false>(t, P, Dir4{vd, h, 8}, Dir4{vd, h, 12});
    f3_stage<false, false, true>(t, P, F3None{}, F3None{});  // next: stream padding

    // rgb = Wrgb relu(v) + b
    float acc3[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int T = 0; T < 4; ++T)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f32x4 wv[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) wv[c] = *reinterpret_cast<const f32x4*>(P0 + off.rgb_w + c * T_VIEWS + 32 * T + 8 * q + 4 * h);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float y = fmaxf(t[T][4 * q + j], 0.f);
#pragma unroll
                for (int c = 0; c < 3; ++c) acc3[c] = __builtin_fmaf(wv[c][j], y, acc3[c]);
            }
        }
#pragma unroll
    for (int c = 0; c < 3; ++c) acc3[c] = acc3[c] + __shfl_xor(acc3[c], 32) + P0[off.rgb_b + c];
    if (valid && h == 0) {
        const f32x4 o4 = {acc3[0], acc3[1], acc3[2], alpha};
        *reinterpret_cast<f32x4*>(a.raw + (LIVE ? (int64_t)live_n : pt) * 4) = o4;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// host side (called from r2l_teacher_mlp.hip's C ABI entry points)
// ------------------------------------------------------------------------------------------------------------------
int64_t r2l_teacher3_stream_floats(void) { return (int64_t)(T3_STAGES + R2L_F3_PAD_STAGES) * (F3_STAGE_BYTES / 4); }

int r2l_teacher3_pack(const float* tparams, float* wstream3, hipStream_t stream) {
    hipLaunchKernelGGL(r2l_pack_teacher3_kernel, dim3(512), dim3(256), 0, stream, tparams,
                       reinterpret_cast<unsigned short*>(wstream3));
    R2L_CHECK(hipGetLastError());
    return 0;
}

int r2l_teacher3_mlp(const float* rays_o, const float* rays_d, const float* viewdirs, const float* z,
                     const float* wstream3, const float* tparams, float* raw, int64_t n_pts, int S, hipStream_t stream,
                     const unsigned* run_if, const int64_t* idx, const int64_t* count_dev, int64_t n_out) {
    T16Args a{};
    a.run_if = run_if;
    a.idx = idx; a.count_dev = count_dev; a.n_out = n_out > 0 ? n_out : n_pts;
    a.rays_o = rays_o; a.rays_d = rays_d; a.viewdirs = viewdirs; a.z = z;
    a.stream = reinterpret_cast<const unsigned char*>(wstream3); a.params = tparams; a.raw = raw; a.n_pts = n_pts; a.S = S;
    if (idx != nullptr) hipLaunchKernelGGL(r2l_teacher3_kernel<true>, dim3(t_workgroups(n_pts)), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(r2l_teacher3_kernel<false>, dim3(t_workgroups(n_pts)), dim3(256), 0, stream, a);
    R2L_CHECK(hipGetLastError());
    return 0;
}
