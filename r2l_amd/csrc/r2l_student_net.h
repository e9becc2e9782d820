// r2l_student_net.h — the R2L student, NeRF_v3_2 (16 samples x 3 axes x (2 * 10 + 1) encoding -> Linear(1008, 256) + ReLU ->
// n_block x ResMLP block -> outer residual -> Linear(256, 3) + Sigmoid), as its five forward chains (r2l_forward.hip,
// r2l_fwd2.hip, r2l_fwd3.hip, r2l_coopf_fwd.hip, r2l_coop16.hip) and five dX chains (r2l_bwd32.hip, r2l_bwd2.hip, r2l_bwd3.hip,
// r2l_coopf_bwd.hip, r2l_coop16.hip) share it.  What is a property of the network or of the ray set-up lives here once: the
// parameter census, the ray of a lane, the sample depths, the loss seed of the backward, the tail in both directions, and the
// host-side declarations between the files.  The GEMM pipelines stay in the .hip files.  Every chain takes the census and the
// launchers from here; the device helpers serve the one-wave-per-tile chains, and a kernel whose code or speed a helper was found
// to change keeps those lines of its own, with a comment that names the helper and the finding (the cooperative chains, the pose
// branches of r2l_forward.hip and r2l_fwd3.hip, the tail finish of r2l_forward.hip).
//
// The helpers are inlined into kernels that sit at the register limit: they take register arrays by reference, index them with
// compile-time constants only and select their variants with template parameters — never with a run-time flag.
#pragma once
#include "r2l_dispatch.h"
#include "r2l_pixel_ray.h"

// ---- the parameter census: flat offsets in state_dict order -----------------------------------------------------------
// head.0.{weight [256,1008], bias}, body.b.body.{0,2}.{weight [256,256], bias} (layer = 2 b + {0, 1}), tail.0.{weight [3,256], bias}
__host__ __device__ static inline int64_t r2l_off_head_b() { return (int64_t)R2L_IN * R2L_W; }
__host__ __device__ static inline int64_t r2l_off_body_w(int layer) {
    return (int64_t)R2L_IN * R2L_W + R2L_W + (int64_t)layer * (R2L_W * R2L_W + R2L_W);
}
__host__ __device__ static inline int64_t r2l_off_body_b(int layer) { return r2l_off_body_w(layer) + R2L_W * R2L_W; }
__host__ __device__ static inline int64_t r2l_off_tail_w(int n_block) { return r2l_off_body_w(2 * n_block); }
__host__ __device__ static inline int64_t r2l_off_tail_b(int n_block) { return r2l_off_tail_w(n_block) + 3 * R2L_W; }
__host__ __device__ static inline int64_t r2l_off_total(int n_block) { return r2l_off_tail_b(n_block) + 3; }

// ---- inputs and outputs every chain family takes, as they travel between the files ---------------------------------------------
// (Kernel arguments embed R2LRayIn where that leaves their layout as it was — r2l_fwd2.hip, r2l_fwd3.hip —; the other families
// keep their own order of the same members, because a moved kernel argument re-allocates the registers of the whole chain.)
struct R2LRayIn {
    const float* rays_o;   // [N,3]   rays mode
    const float* rays_d;   // [N,3]
    const float* t_rand;   // [N,16] stratified jitter U[0,1) or nullptr (perturb == 0)
    const float* ztab;     // [32]: z_lower[16], z_span[16]
    float c2w[12];         // pose mode: row-major [3,4] camera-to-world, by value
    const float* c2w_dev;  // pose mode, several frames per launch: [K][12] on the device (r2l_pose_of), else nullptr
    int H, Wimg;
    float focal;
};
struct R2LLossIO {
    const float* rgb;      // [N,3] forward output
    const float* target;   // [N,3] MSE mode: dL/drgb = grad_scale * (rgb - target), or nullptr
    const float* drgb;     // [N,3] generic mode (target == nullptr): dL/drgb given by the caller
    float grad_scale;      // = 2 * lw_rgb / (3 * N_global)
    float* dpre;           // [N,3] dL/d(tail pre-activation)
    float* sqerr_partial;  // [ceil(N/32)] per-tile sums of (rgb - target)^2, or nullptr
};
// rays mode or pose mode: a launch without explicit rays takes its rays from the pose(s)
static inline bool r2l_pose_mode(const R2LRayIn& r) { return r.rays_o == nullptr; }
// into kernel arguments that carry the members under the same names.  r2l_set_rays serves the kernels that take ONE pose per
// launch (r2l_coopf_fwd.hip, r2l_coop16.hip: no c2w_dev member), so a pose table must not reach it: forward_poses
// (r2l_forward.hip) refuses the cooperative tilings with a table, and the launchers' callers hand c2w_dev == nullptr.
template <class Args>
static inline void r2l_set_rays(Args& a, const R2LRayIn& r) {
    a.rays_o = r.rays_o; a.rays_d = r.rays_d; a.t_rand = r.t_rand; a.ztab = r.ztab;  // (r.c2w_dev: see above)
    for (int i = 0; i < 12; ++i) a.c2w[i] = r.c2w[i];
    a.H = r.H; a.Wimg = r.Wimg; a.focal = r.focal;
}
template <class Args>
static inline void r2l_set_loss(Args& a, const R2LLossIO& l) {
    a.rgb = l.rgb; a.target = l.target; a.drgb = l.drgb; a.grad_scale = l.grad_scale;
    a.dpre = l.dpre; a.sqerr_partial = l.sqerr_partial;
}

// ---- the ray of a lane ------------------------------------------------------------------------------------------------------
// pose mode: the camera of ray rc and its pixel index.  One pose by value (c2w), or — one launch over several frames
// (r2l_forward_poses: no tail round and no launch gap per frame) — a device table c2w_dev[K][12], frame = rc / (H * W)
struct R2LPoseRay { float c[12]; int64_t pix; };
__device__ __forceinline__ R2LPoseRay r2l_pose_of(const float (&c2w)[12], const float* c2w_dev, int64_t hw, int64_t rc) {
    R2LPoseRay r;
    r.pix = rc;
    if (c2w_dev != nullptr) {
        const int64_t p = rc / hw;
        r.pix = rc - p * hw;
#pragma unroll
        for (int i = 0; i < 12; ++i) r.c[i] = c2w_dev[p * 12 + i];
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i) r.c[i] = c2w[i];
    }
    return r;
}
// o, d of row rc of a lane, selected by the kernel's POSE template argument at the call site:
//     if constexpr (!POSE) r2l_ray_of_row(a.rays_o, a.rays_d, rc, o, d);
//     else r2l_ray_of_pixel<TABLE>(a.c2w, a.c2w_dev, a.H, a.Wimg, a.focal, rc, o, d);
// (two calls with plain values, not one helper that takes the kernel's arguments: a reference to the arguments in a rays-mode
// kernel makes hipcc load all of them up front, which re-allocates the registers of the chain.)  Callers: r2l_fwd2.hip in both
// modes, r2l_forward.hip and r2l_fwd3.hip in rays mode; the pose branches of those two, r2l_coopf_fwd.hip and r2l_coop16.hip keep the
// same lines of their own — each says why where it does — and tests/test_student_forward_gpu.py holds all of them to r2l_frame_rays' bits.
__device__ __forceinline__ void r2l_ray_of_row(const float* rays_o, const float* rays_d, int64_t rc, float (&o)[3], float (&d)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        o[k] = rays_o[rc * 3 + k];
        d[k] = rays_d[rc * 3 + k];
    }
}
// pose mode: the world ray of pixel rc of the frame(s) — PointSampler.__init__ / sample_test (nerf_raybased.py:80-99), the very
// pixel_ray that r2l_frame_rays writes.  TABLE: the kernel takes a pose table (else c2w_dev is not read).
template <bool TABLE>
__device__ __forceinline__ void r2l_ray_of_pixel(const float (&c2w)[12], const float* c2w_dev, int H, int Wimg, float focal,
                                                 int64_t rc, float (&o)[3], float (&d)[3]) {
    if constexpr (TABLE) {
        const R2LPoseRay pr = r2l_pose_of(c2w, c2w_dev, (int64_t)H * Wimg, rc);
        pixel_ray(pr.c, focal, H, Wimg, (int)(pr.pix / Wimg), (int)(pr.pix % Wimg), o, d);
    } else {
        pixel_ray(c2w, focal, H, Wimg, (int)(rc / Wimg), (int)(rc % Wimg), o, d);
    }
}

// ---- sample depths ----------------------------------------------------------------------------------------------------------
// z[k] of sample first + k of row rc: z_lower, or fl(z_lower + fl(z_span * t_rand)) (nerf_raybased.py:119-123; the build passes
// -ffp-contract=off), COUNT samples as 16-byte loads.  COUNT = 8, first = 8 h: the half-wave layout of r2l_forward.hip, r2l_fwd2.hip
// and r2l_fwd3.hip.  The other layouts keep this rule on their own lines and point here: r2l_coop16.hip (16 per lane),
// r2l_coopf_fwd.hip (2 per thread), and the scalar recomputations of r2l_dw_head.hip, r2l_dw_head16.hip and r2l_input_grad.hip.
template <int COUNT>
__device__ __forceinline__ void r2l_depths(const float* ztab, const float* t_rand, int64_t rc, int first, float (&z)[COUNT]) {
    static_assert(COUNT % 4 == 0, "whole 16-byte loads");
    f32x4 lo[COUNT / 4];
#pragma unroll
    for (int q = 0; q < COUNT / 4; ++q) {
        lo[q] = *reinterpret_cast<const f32x4*>(ztab + first + 4 * q);
#pragma unroll
        for (int k = 0; k < 4; ++k) z[4 * q + k] = lo[q][k];
    }
    if (t_rand != nullptr) {
#pragma unroll
        for (int q = 0; q < COUNT / 4; ++q) {
            const f32x4 sp = *reinterpret_cast<const f32x4*>(ztab + 16 + first + 4 * q);
            const f32x4 u = *reinterpret_cast<const f32x4*>(t_rand + rc * 16 + first + 4 * q);
#pragma unroll
            for (int k = 0; k < 4; ++k) z[4 * q + k] = lo[q][k] + sp[k] * u[k];
        }
    }
}

// ---- loss seed of the dX chains ---------------------------------------------------------------------------------------------
// dp = dL/d(tail pre-activation) of row rc: dL/drgb (MSE: grad_scale * (rgb - target); generic: drgb) through the sigmoid,
// 0 for the padding rays of a ragged tile.  Returns the ray's squared error (MSE mode, else 0).
__device__ __forceinline__ float r2l_loss_seed(const float* rgb, const float* target, const float* drgb, float grad_scale,
                                               int64_t rc, bool valid, float (&dp)[3]) {
    float se = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float r = rgb[rc * 3 + c];
        float dl;
        if (target != nullptr) {
            const float e = r - target[rc * 3 + c];
            se += e * e;
            dl = grad_scale * e;
        } else {
            dl = drgb[rc * 3 + c];
        }
        dp[c] = valid ? dl * (r * (1.0f - r)) : 0.f;
    }
    if (!valid) se = 0.f;
    return se;
}
__device__ __forceinline__ void r2l_dpre_store(float* dpre, int64_t ray, const float (&dp)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) dpre[ray * 3 + c] = dp[c];
}
// per-tile squared error of a 32-ray tile held by one wave: lanes 0..31 hold the 32 rays (both half-waves carry the same se)
__device__ __forceinline__ void r2l_tile_sqerr(float* sqerr_partial, int64_t tile, float se, int h, int lane) {
    if (sqerr_partial != nullptr) {
        float s = (h == 0) ? se : 0.f;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
        if (lane == 0) sqerr_partial[tile] = s;
    }
}

// ---- the tail, Linear(256, 3) + Sigmoid ---------------------------------------------------------------------------------------
// Transposed: Wt^T dp for the four features at tw (the tail weight of channel 0 at the first of them), and g = Wt^T dp for NTILE
// 32-feature tiles in fragment layout, tw = params + r2l_off_tail_w + 32 * first tile + 4 * h.  SCALED: the chain runs on
// gscale * g (a power of two, r2l_bwd2.hip): Wt^T (dp * gscale), the product formed here, at its use, as the chains always formed
// it — hipcc hoists the three multiplies.  (Handing in a pre-scaled copy of dp gives the same bits; it was tried, bought no line
// of assembly and costs every scaled caller a second array.  The fp32 chains pass SCALED = false and gscale is not read.)
template <bool SCALED>
__device__ __forceinline__ void r2l_tail_transposed4(f32x4& out, const float* tw, const float (&dp)[3], float gscale) {
    f32x4 wv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) wv[c] = *reinterpret_cast<const f32x4*>(tw + c * R2L_W);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float v = wv[0][j] * (SCALED ? dp[0] * gscale : dp[0]);
        v = __builtin_fmaf(wv[1][j], SCALED ? dp[1] * gscale : dp[1], v);
        v = __builtin_fmaf(wv[2][j], SCALED ? dp[2] * gscale : dp[2], v);
        out[j] = v;
    }
}
template <bool SCALED, int NTILE>
__device__ __forceinline__ void r2l_tail_transposed(f32x16 (&g)[NTILE], const float* tw, const float (&dp)[3], float gscale) {
#pragma unroll
    for (int T = 0; T < NTILE; ++T)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f32x4 v;
            r2l_tail_transposed4<SCALED>(v, tw + 32 * T + 8 * q, dp, gscale);
#pragma unroll
            for (int j = 0; j < 4; ++j) g[T][4 * q + j] = v[j];
        }
}
// Forward finish of a one-wave-per-tile chain: p3 = this half-wave's partial dot products of Wt (x_n + x_0); the two halves are
// added, then rgb = sigmoid(p3 (* act_s) + bias) for the lanes that `store`.  SCALED: the chain ran on y / act_s (r2l_f2.h).
template <bool SCALED>
__device__ __forceinline__ void r2l_tail_finish(float (&p3)[3], const float* bias, float act_s, float* rgb, int64_t ray, bool store) {
#pragma unroll
    for (int c = 0; c < 3; ++c) p3[c] += __shfl_xor(p3[c], 32);
    if (store) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = SCALED ? p3[c] * act_s + bias[c] : p3[c] + bias[c];
            rgb[ray * 3 + c] = 1.0f / (1.0f + expf(-v));
        }
    }
}

// ---- host side: the launchers between the files ------------------------------------------------------------------------------
// The stash / parameter / stream arguments are the C ABI's (include/r2l_hip.h); rays and loss travel as the structs above.
// forward chains
int r2l_coop16_forward(const R2LRayIn& rays, const float* wstream16, const float* params, int n_block, float* rgb,
                       float* save_x, float* save_t, int64_t N, hipStream_t stream);
int r2l_fwd2_forward(const R2LRayIn& rays, const float* wstream2, const float* params, int n_block, float* rgb,
                     float* save_x, float* save_t, int64_t N, hipStream_t stream, bool stash_mid);
// run_if: nullptr, or a device word — the launch returns at once while it is 0 (fallback behind r2l_fwd2_forward)
int r2l_fwd3_forward(const R2LRayIn& rays, const float* wstream3, const float* params, int n_block, float* rgb,
                     float* save_x, float* save_t, int64_t N, hipStream_t stream, const unsigned* run_if = nullptr,
                     const float* x0_in = nullptr);  // x0_in: body + tail from a given X_0
// cooperative fp16x2 chains (r2l_coopf_fwd.hip / r2l_coopf_bwd.hip), taken instead of r2l_fwd2_forward / r2l_bwd2_backward when
// the plan's tiling is COOPF: tiles per workgroup, mixed grid and mid halves of the stash as the plan says
int r2l_coopf_forward(const R2LRayIn& rays, const float* wstream2, const float* params, int n_block, float* rgb,
                      float* save_x, float* save_t, int64_t N, hipStream_t stream, const R2LPlan& plan);
// dX chains
int r2l_bwd32_backward(const R2LLossIO& loss, const float* save_x, const float* save_t, const float* wstream_bwd32,
                       const float* params, int n_block, float* gx, float* gt, int64_t N, hipStream_t stream);
int r2l_coop16_backward(const R2LLossIO& loss, const float* save_x, const float* save_t, const float* wstream_bwd16,
                        const float* params, int n_block, float* gx, float* gt, int64_t N, hipStream_t stream);
int r2l_bwd3_backward(const R2LLossIO& loss, const float* save_x, const float* save_t, const float* wstream_bwd3,
                      const float* params, int n_block, float* gx, float* gt, int64_t N, hipStream_t stream, float gscale = 1.0f,
                      const unsigned* run_if = nullptr, const float* scale_dev = nullptr);
// the same chain on two-way fp16 splits (r2l_bwd2.hip); status: range-guard word (behind the bwd2 stream region)
int r2l_bwd2_backward(const R2LLossIO& loss, const float* save_x, const float* save_t, const float* wstream_bwd2,
                      const float* params, int n_block, float* gx, float* gt, int64_t N, hipStream_t stream, float gscale,
                      unsigned* status, const float* scale_dev, bool stash_mid);  // stash_mid: the step stashes the mid halves too (exact dW)
int r2l_coopf_backward(const R2LLossIO& loss, const float* save_x, const float* save_t, const float* wstream_bwd2,
                       const float* params, int n_block, float* gx, float* gt, int64_t N, hipStream_t stream, float gscale,
                       unsigned* status, const float* scale_dev, const R2LPlan& plan, int b_start = -1,
                       int b_end = 0);  // blocks b_start (-1: the last) down to b_end
