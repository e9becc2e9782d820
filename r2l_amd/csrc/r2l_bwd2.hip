// r2l_bwd2.hip — the dX chain of r2l_bwd3.hip on the fp16 matrix pipe with two-way operand splits (machinery: r2l_f2.h):
// three fp16 products per fp32 product, ~2^-21 relative.  The chain runs on gscale * g (a power of two chosen from the MSE
// gradient scale, r2l_backward), which puts its values into fp16's range; a range guard raises a status word and the bf16x3
// kernel launched behind it redoes the launch.  Stage order, mask ring and stash stores are r2l_bwd3.hip's; six 16 KiB
// weight buffers fit beside the 32 KiB mask ring.  The file also owns the range control of a step of the fp16 trio: the two
// kernels that write the B2S_* status words in front of the chain (r2l_bwd_prepare_kernel, r2l_gscale_kernel; r2l_bwd2_open_step).
#include "r2l_f2.h"
#include "r2l_coopf.h"
#include "r2l_dw.h"  // r2l_bwd2_open_step

#define B3_RING 2  // mask pieces (one per block) per wave

// =================================================================================================================
// pack: stage order and element numbering of r2l_pack_bwd2_kernel, two fp16 splits per value, 16 KiB stages
// =================================================================================================================
__global__ void r2l_pack_bwd2_kernel(const float* __restrict__ params, unsigned short* __restrict__ out, int n_block) {
    const int64_t stages = r2l_bwd3_stages(n_block);
    const int64_t total = (stages + R2L_F3_PAD_STAGES) * 8 * 64 * 8;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int s = (int)(idx & 7), lane = (int)((idx >> 3) & 63), tile = (int)((idx >> 9) & 7);
        const int64_t g = idx >> 12;
        const int i = lane & 31, h = lane >> 5, o = 32 * tile + i;
        unsigned short* st = out + g * (F2_STAGE_BYTES / 2);
        unsigned short v0 = 0, v1 = 0;
        if (g < stages) {
            const int slot = (int)(g / 34), r = (int)(g % 34), b = n_block - 1 - slot;
            if (r != 0 && r != 17) {
                const int layer = r < 17 ? 2 * b + 1 : 2 * b, kb = r < 17 ? r - 1 : r - 18;
                const int T = kb >> 1, rr = kb & 1;
                const int in = 32 * T + 8 * (2 * rr + (s >> 2)) + 4 * h + (s & 3);
                const float w = params[r2l_off_body_w(layer) + (int64_t)in * R2L_W + o];  // (W^T)[o][in] = W[in][o]
                const _Float16 hi = (_Float16)w;
                const _Float16 mid = (_Float16)(w - (float)hi);
                v0 = __builtin_bit_cast(unsigned short, hi);
                v1 = __builtin_bit_cast(unsigned short, mid);
            }
        }
        const int64_t e = ((int64_t)tile * 64 + lane) * 8 + s;
        st[e] = v0;
        st[8 * 64 * 8 + e] = v1;
    }
}

// =================================================================================================================
// kernel
// =================================================================================================================
struct B2Args {
    const float* rgb;
    const float* target;
    const float* drgb;
    const float* save_x;
    const float* save_t;
    const unsigned char* stream;
    const float* params;
    int n_block;
    float grad_scale;
    float gscale, ginv;  // the chain runs on gscale * g (a power of two; what it stashes is scaled), gx[0] is scaled back
    const float* scale_dev;  // generic mode: {gscale, 1 / gscale} chosen on the device from max |drgb| (r2l_gscale_kernel), or nullptr
    unsigned* status;    // range guard: raised when a chain value leaves fp16's safe range (the bf16x3 kernel then redoes it)
    const unsigned* fmt; // stash format word of the forward (r2l_common.h): != 0 -> chunked fp32 stash (the forward fell back to
                         // the bf16x3 kernel): this launch raises *status and leaves the work to the bf16x3 chain as well
    float* dpre;
    float* gx;
    float* gt;
    float* sqerr_partial;
    int64_t N;
    unsigned stash_mid;  // != 0: also stash the mid halves of g / masked u, this many bytes behind the hi pieces (r2l_f2.h)
};

// gatherers: four B values of the next stage (+ their stash store)
// (what the weight-gradient GEMMs read of g / the masked u is the fp16 hi operand these values are converted to: stashed by
// the stage that assembles it, r2l_f2.h F2Hst — gx[b+1] and gt[b] hold fp16 stage pieces, scaled by gscale)
struct B3TakeG {  // g values (identity)
    const f32x16& frag;
    int c0;
    __device__ __forceinline__ void operator()(float (&v)[4]) const {
#pragma unroll
        for (int s = 0; s < 4; ++s) v[s] = frag[c0 + s];
    }
};
struct B3TakeU {  // u values masked by relu'(t_b) (mask words of the forward: bit (T&1)*16 + c of word T>>1)
    const f32x16& frag;
    int c0;
    int T;
    const u32x4& mb;
    __device__ __forceinline__ void operator()(float (&v)[4]) const {
        const unsigned w = mb[T >> 1] >> ((T & 1) * 16 + c0);
#pragma unroll
        for (int s = 0; s < 4; ++s) v[s] = ((w >> s) & 1u) ? frag[c0 + s] : 0.f;
    }
};

// MID: the mid halves of g / masked u are stashed too (exact weight gradients; template parameter: see r2l_fwd2.hip)
template <bool MID>
__global__ __launch_bounds__(256, 1) void r2l_bwd2_kernel(const B2Args a) {
    __shared__ __attribute__((aligned(16))) unsigned char wbuf[F2_NBUF][F2_STAGE_BYTES];
    __shared__ __attribute__((aligned(16))) unsigned char mring[4][B3_RING][1024];

    if (__builtin_nontemporal_load(a.fmt) != 0u) {  // the forward's stash is the bf16x3 trio's: so is this step's backward
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(a.status, 1u);
        return;
    }
    const float gscale = a.scale_dev != nullptr ? a.scale_dev[0] : a.gscale;
    const float ginv = a.scale_dev != nullptr ? a.scale_dev[1] : a.ginv;
    const int lane = threadIdx.x & 63, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // a wave whose tile lies past the end recomputes the last live tile (identical values to identical addresses): nothing in
    // the chain is conditional
    const int64_t n_tiles = (a.N + R2L_TILE_RAYS - 1) / R2L_TILE_RAYS;
    int64_t tile = (int64_t)blockIdx.x * 4 + wave;
    if (tile > n_tiles - 1) tile = n_tiles - 1;
    const int64_t ray = tile * R2L_TILE_RAYS + (lane & 31);
    const bool valid = ray < a.N;
    const int64_t rc = valid ? ray : a.N - 1;
    const int64_t Np = R2L_PAD_ROWS(a.N);

    // ---- loss gradient through the sigmoid, per-tile squared error; g = dy = Wt^T (gscale dpre) (tail Linear(256,3)) ----
    float dp[3];
    const float se = r2l_loss_seed(a.rgb, a.target, a.drgb, a.grad_scale, rc, valid, dp);
    if (valid && h == 0) r2l_dpre_store(a.dpre, ray, dp);
    r2l_tile_sqerr(a.sqerr_partial, tile, se, h, lane);
    f32x16 g[R2L_NT], u[R2L_NT], dy[R2L_NT];
    r2l_tail_transposed<true>(g, a.params + r2l_off_tail_w(a.n_block) + 4 * h, dp, gscale);
#pragma unroll
    for (int T = 0; T < R2L_NT; ++T) dy[T] = g[T];

    // ---- weight staging (6 buffers of 16 KiB beside the 32 KiB mask ring) ------------------------------------------------------
    F2Pipe P;
    P.init(a.stream, &wbuf[0][0], lane, wave);
#pragma unroll
    for (int k = 0; k < F2_NBUF - 1; ++k) P.issue();  // stages 0 .. F2_NBUF-2
#pragma unroll
    for (int k = 0; k < 8; ++k) P.ones.h[k] = (_Float16)((h == 0 && k < 2) ? 1.0f : 0.0f);
    P.ones.m = P.ones.h;
    if (F2_NBUF == 6) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");  // stage 0 landed
    else asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
    __syncthreads();
    P.lb = P.base + lane * 16;
    {
        F3None none;
        F2Side<true, F3None> s0{P.a1, P.lb, 0, none, false, F3Dma{false, P.rs, 0u, 0u, 0u}, P.amax};
#pragma unroll
        for (int i = 0; i < 6; ++i) s0.step(i);
    }
    P.sb = P.ones;

    // mask words of this wave's tile: one 1 KiB piece per block (64 lanes x 16 B), fetched by DMA into a two-slot LDS ring at
    // the start of the block and read when its second GEMM starts, 17 stages later
    const unsigned ring_lds = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)&mring[0][0][0] +
                              (unsigned)wave * (B3_RING * 1024u);
    const unsigned char* ring_lane = &mring[0][0][0] + wave * (B3_RING * 1024) + lane * 16;
    const int64_t slot = R2L_TRIO_SLOT(Np);
    const int64_t lane_unit = tile * R2L_H16_TILE_UNITS + lane;  // this lane's 16-byte unit of stage piece 0 in a slot
    const unsigned mvoff = (unsigned)((R2L_MASK_OFFSET(Np) + tile * 256 + lane * 4) * 4);  // byte offset of the lane's mask words

#pragma unroll 1
    for (int b = a.n_block - 1; b >= 0; --b) {
        // descriptor of save_t[b] (per block: 32-bit offsets inside the slot)
        const u32x4 trs = r2l_buffer_rsrc(a.save_t + (int64_t)b * slot);
        float* const gxr = a.gx + (int64_t)(b + 1) * slot;
        float* const gtr = a.gt + (int64_t)b * slot;
        const unsigned hvoff = (unsigned)(lane_unit * 16);
        const F3Dma no_dma{false, u32x4{0u, 0u, 0u, 0u}, 0u, 0u, 0u};
        constexpr bool mid = MID;
        const F3Dma mask_dma{true, trs, mvoff, 0u, ring_lds + (unsigned)(b & 1) * 1024u};
        // GEMM A: u = W2^T g.  stage 0 (zero stage, zero-initialises u) gathers g block 0; stage 1+kb gathers g block kb+1
        f2_stage<true, true, false>(u, P, B3TakeG{g[0], 0}, B3TakeG{g[0], 4}, mask_dma, no_dma, F2Hst{true, gxr, hvoff, 0u});
#pragma unroll
        for (int kb = 0; kb < 15; ++kb)
            f2_stage<false, false, false>(u, P, B3TakeG{g[(kb + 1) >> 1], 8 * ((kb + 1) & 1)},
                                          B3TakeG{g[(kb + 1) >> 1], 8 * ((kb + 1) & 1) + 4}, no_dma, no_dma,
                                          F2Hst{true, gxr, hvoff, 1024u * (unsigned)(kb + 1)},
                                          F2Hst{mid, gxr, hvoff, 1024u * (unsigned)kb + a.stash_mid});
        // (the mask piece was requested 16 stages ago: every stage wait since has retired all but the newest loads)
        const u32x4 mb = *reinterpret_cast<const u32x4*>(ring_lane + (b & 1) * 1024);
        f2_stage<false, false, true>(u, P, F3None{}, F3None{}, no_dma, no_dma, F2Hst{false, nullptr, 0u, 0u},
                                     F2Hst{mid, gxr, hvoff, 1024u * 15u + a.stash_mid});
        // GEMM B: g += W1^T (u . mask).  stage 17 (zero stage) gathers masked-u block 0; stage 18+kb gathers block kb+1
        f2_stage<true, false, false>(g, P, B3TakeU{u[0], 0, 0, mb}, B3TakeU{u[0], 4, 0, mb}, no_dma, no_dma, F2Hst{true, gtr, hvoff, 0u});
#pragma unroll
        for (int kb = 0; kb < 15; ++kb)
            f2_stage<false, false, false>(g, P, B3TakeU{u[(kb + 1) >> 1], 8 * ((kb + 1) & 1), (kb + 1) >> 1, mb},
                                          B3TakeU{u[(kb + 1) >> 1], 8 * ((kb + 1) & 1) + 4, (kb + 1) >> 1, mb}, no_dma, no_dma,
                                          F2Hst{true, gtr, hvoff, 1024u * (unsigned)(kb + 1)},
                                          F2Hst{mid, gtr, hvoff, 1024u * (unsigned)kb + a.stash_mid});
        // next: the zero stage of the next block (or the padding)
        f2_stage<false, false, true>(g, P, F3None{}, F3None{}, no_dma, no_dma, F2Hst{false, nullptr, 0u, 0u},
                                     F2Hst{mid, gtr, hvoff, 1024u * 15u + a.stash_mid});
    }

    f2_report_amax<B2S_AMAX>(a.status, P.amax, lane);  // AMAX (the next step's scale is chosen from it), FLAG if out of range

    // ---- head: dL/d(head pre-activation) = (g + dy) * (x_0 > 0) -> gx[0] ---------------------------------------------------------
    {
        // x_0 = relu(head): its fp16 stage pieces (slot 0 of save_x); stage kb = 2T + r holds fragment registers c = 8r .. 8r+7
        // of tile T.  Only the sign matters; fp16 rounds x_0 < 3e-8 to zero (such a unit counts as inactive).
        const u32x4* r = reinterpret_cast<const u32x4*>(a.save_x) + lane_unit;
        float* o = a.gx + ray * R2L_W + 4 * h;  // row-major fp32: the head weight gradient reads rows
#pragma unroll
        for (int T = 0; T < R2L_NT; ++T)
#pragma unroll
            for (int rr = 0; rr < 2; ++rr) {
                const f16x8 xv = __builtin_bit_cast(f16x8, r[64 * (2 * T + rr)]);
#pragma unroll
                for (int q2 = 0; q2 < 2; ++q2) {
                    f32x4 ov;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int c = 8 * rr + 4 * q2 + j;
                        ov[j] = (float)xv[4 * q2 + j] > 0.f ? (g[T][c] + dy[T][c]) * ginv : 0.f;
                    }
                    *reinterpret_cast<f32x4*>(o + 32 * T + 8 * (2 * rr + q2)) = ov;
                }
            }
    }
}

// Generic mode of the fp16 trio: the caller's dL/drgb has no known scale, so the power of two that puts the dX chain into
// fp16's range is chosen on the device: out = {gscale, 1 / gscale}, gscale = 2^(8 - e) for max |drgb| = m * 2^e — the rule
// r2l_backward_part applies on the host to the MSE gradient scale.  One workgroup (generic mode is not the training loop's).
__global__ __launch_bounds__(1024) void r2l_gscale_kernel(const float* __restrict__ drgb, int64_t n, float* __restrict__ out) {
    __shared__ float red[1024];
    float m = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += 1024) m = fmaxf(m, fabsf(drgb[i]));
    red[threadIdx.x] = m;
    __syncthreads();
    for (int k = 512; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + k]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        float g = 1.0f;
        if (red[0] > 0.f && red[0] < 3.0e38f) {
            int e = 0;
            (void)frexpf(red[0], &e);
            g = ldexpf(1.0f, 8 - e);
        }
        out[0] = g;
        out[1] = 1.0f / g;
    }
}

// The 16 status words behind the fp16 dX stream (r2l_common.h B2S_*), at the start of every step of the fp16 trio: FLAG and
// AMAX cleared, and — MSE mode — the power of two the step's dX chain runs on written to GSCALE / GINV:
//   * first step (or after a step that fell back, or a zero gradient): the a-priori rule of rounds 1 - 3, 2^(8 - e) for
//     grad_scale = m * 2^e (the seed is then <= 64 |rgb - target|), corrected by the size of the tail weights the seed goes
//     through: x 2^(-3 - e_w) for max |W_tail| = m * 2^e_w (the default init's 1/16 gives 1);
//   * afterwards the scale is KEPT while the last clean step's largest |chain value| (times grad_scale / its grad_scale: batch
//     sizes may change) lies in [2^-2, 2^13] scaled — a factor 4 below the guard (R2L_F2_RANGE) and, at the low end, still
//     2^-23 of the largest value in absolute fp16 (hi + mid) resolution — and re-centred to 2^8 when it leaves that band.
//     So nets whose gradients live where the a-priori rule expects them (default init, the trained nets measured so far) run
//     bit for bit as in round 3, and a net whose gradients drift (or start) elsewhere follows on the next step instead of
//     falling back (overflow) or silently losing bits (underflow) from then on.
// Powers of two commute with fp32 rounding: whatever the scale, the bf16x3 fallback run on it is bit-identical after unscaling.
// (A kernel, not hipMemsetAsync: a memset node captured into a hipGraph wrote a stale pattern on replay, ROCm 7.0; the history
// is device state, so captured steps adapt on replay as eager ones do.)  generic mode (mse == 0): GSCALE is r2l_gscale_kernel's.
__global__ __launch_bounds__(64) void r2l_bwd_prepare_kernel(unsigned* status, const float* __restrict__ tail_w, float grad_scale,
                                                             int mse) {
    float wm = 0.f;
    if (mse)
        for (int i = threadIdx.x; i < 3 * R2L_W; i += 64) wm = fmaxf(wm, fabsf(tail_w[i]));
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) wm = fmaxf(wm, __shfl_xor(wm, off));
    if (threadIdx.x != 0) return;
    const float gs = fabsf(grad_scale);
    const bool valid = status[B2S_MAGIC] == F2_MAGIC;
    const bool clean = valid && status[B2S_FLAG] == 0u;
    const float a_raw = valid ? __builtin_bit_cast(float, status[B2S_AMAX]) : 0.f;  // 0: the chain did not run (forward fell back)
    const float a = clean ? a_raw : 0.f;
    const float g_prev = valid ? __builtin_bit_cast(float, status[B2S_GSCALE]) : 0.f;
    const float gs_prev = valid ? __builtin_bit_cast(float, status[B2S_GS]) : 0.f;
    int ex_prev = 0;
    const bool g_ok = g_prev > 0.f && g_prev < 3.0e38f && frexpf(g_prev, &ex_prev) == 0.5f;  // a power of two: 2^(ex_prev - 1)
    float peak = valid ? __builtin_bit_cast(float, status[B2S_PEAK]) : 0.f;
    unsigned trips = valid ? status[B2S_TRIPS] : 0u;
    if (valid && status[B2S_FLAG] != 0u) ++trips;
    // a step whose CHAIN tripped the guard (round 5): its AMAX is the truth while every value stayed finite in fp32 — the guard
    // trips at 32768, the fp32 B values are tracked before their fp16 conversion — so the next step re-centres on it instead of
    // repeating the a-priori rule (and tripping again, step after step, on a net whose gradients grow through the body);
    // AMAX = inf / NaN: only "too large" is known — the scale drops by 2^8 and the following step refines it
    bool blind = false;
    if (clean && g_ok && a > 0.f && a < 3.0e38f) peak = a / g_prev;  // unscaled amax of the last clean step
    else if (!clean && valid && g_ok && a_raw > 0.f && a_raw < 3.0e38f) peak = a_raw / g_prev;
    else if (!clean && valid && g_ok && !(a_raw <= 0.f) && !(a_raw < 3.0e38f)) { blind = true; peak = 0.f; }
    else if (!clean) peak = 0.f;                                      // (a step whose forward fell back says nothing reliable)
    if (mse) {
        int ex = 0;
        const float est = (peak > 0.f && gs_prev > 0.f && gs > 0.f && g_ok) ? peak * (gs / gs_prev) : 0.f;
        if (blind) {
            ex = (ex_prev - 1) - 8;
        } else if (est > 0.f && est < 3.0e38f) {
            const float scaled = est * g_prev;
            if (scaled >= 0.25f && scaled <= 8192.f) {
                ex = ex_prev - 1;
            } else {
                (void)frexpf(est, &ex);
                ex = 8 - ex;
            }
        } else if (gs > 0.f) {
            int e = 0, ew = -3;
            (void)frexpf(gs, &e);
            if (wm > 0.f && wm < 3.0e38f) (void)frexpf(wm, &ew);
            ex = (8 - e) + (-3 - ew);
        }
        ex = ex > 120 ? 120 : (ex < -120 ? -120 : ex);
        status[B2S_GSCALE] = __builtin_bit_cast(unsigned, ldexpf(1.0f, ex));
        status[B2S_GINV] = __builtin_bit_cast(unsigned, ldexpf(1.0f, -ex));
        status[B2S_GS] = __builtin_bit_cast(unsigned, gs);
    } else {
        status[B2S_GS] = 0u;
    }
    status[B2S_PEAK] = __builtin_bit_cast(unsigned, peak);
    status[B2S_TRIPS] = trips;
    status[B2S_MAGIC] = F2_MAGIC;
    status[B2S_AMAX] = 0u;
    status[B2S_EXPANDED] = 0u;
    status[B2S_FLAG] = 0u;
}

// ------------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------------
int r2l_bwd2_pack(const float* params, int n_block, float* wstream2, hipStream_t stream) {
    hipLaunchKernelGGL(r2l_pack_bwd2_kernel, dim3(2048), dim3(256), 0, stream, params,
                       reinterpret_cast<unsigned short*>(wstream2), n_block);
    R2L_CHECK(hipGetLastError());
    return 0;
}

int r2l_bwd2_backward(const R2LLossIO& loss, const float* save_x, const float* save_t, const float* wstream_bwd2,
                      const float* params, int n_block, float* gx, float* gt, int64_t N, hipStream_t stream, float gscale,
                      unsigned* status, const float* scale_dev, bool stash_mid) {
    B2Args a{};
    r2l_set_loss(a, loss);
    a.status = status;
    a.scale_dev = scale_dev;
    a.fmt = reinterpret_cast<const unsigned*>(save_x) + R2L_STASH_FMT_WORD(n_block, R2L_PAD_ROWS(N));
    a.gscale = gscale; a.ginv = 1.0f / gscale;
    a.save_x = save_x; a.save_t = save_t;
    a.stream = reinterpret_cast<const unsigned char*>(wstream_bwd2); a.params = params; a.n_block = n_block;
    a.gx = gx; a.gt = gt; a.N = N;
    a.stash_mid = stash_mid ? (unsigned)R2L_H16_MID_BYTES(R2L_PAD_ROWS(N)) : 0u;
    const int64_t tiles = (N + R2L_TILE_RAYS - 1) / R2L_TILE_RAYS;
    if (a.stash_mid != 0u) hipLaunchKernelGGL(r2l_bwd2_kernel<true>, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(r2l_bwd2_kernel<false>, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, stream, a);
    R2L_CHECK(hipGetLastError());
    return 0;
}

// opens a step of the fp16 trio in front of its dX chain (here or r2l_coopf_bwd.hip); generic mode: drgb != nullptr
// (a kernel, not hipMemsetAsync: a memset node captured into a hipGraph wrote a stale 16-byte pattern instead of zeros on
// replay — ROCm 7.0 —, which sent every replayed step to the fallback kernels)
int r2l_bwd2_open_step(unsigned* status, const float* params, int n_block, float grad_scale, const float* drgb, int64_t N,
                       hipStream_t stream) {
    hipLaunchKernelGGL(r2l_bwd_prepare_kernel, dim3(1), dim3(64), 0, stream, status, params + r2l_off_tail_w(n_block), grad_scale,
                       drgb == nullptr ? 1 : 0);
    R2L_CHECK(hipGetLastError());
    if (drgb != nullptr) {
        hipLaunchKernelGGL(r2l_gscale_kernel, dim3(1), dim3(1024), 0, stream, drgb, 3 * N, reinterpret_cast<float*>(status + B2S_GSCALE));
        R2L_CHECK(hipGetLastError());
    }
    return 0;
}
