// r2l_input_grad.hip — the student's gradient with respect to its INPUT: dL/d(embedding) and, through the encoder and the
// sampler, dL/d(rays_o), dL/d(rays_d).  The dX chain of a step (r2l_backward_part*, R2L_BWD_CHAIN) leaves Gh = dL/d(head
// pre-activation) [N,256] fp32, unscaled and row-major, in slot 0 of gx in every kernel family (it is what the head weight
// gradient reads: r2l_dw_head.hip).  One more GEMM carries it to the input,
//     dEmb[r][k] = sum_o Gh[r][o] * Wh[o][k]          (Wh = head.0.weight [256][1008] as it lies in `params`),
// and the ray form continues with the encoder's and the sampler's derivative in the epilogue, on the accumulators:
//     x = o + d z_s,   dPts[r][s][a] = sum_f dEmb[r][(3 s + a) 21 + f] * phi'_f(x),
//     phi' = 2^f cos(2^f x) (sin columns), -2^f sin(2^f x) (cos columns), 1 (identity column),
//     dO[r][a] = sum_s dPts[r][s][a],   dD[r][a] = sum_s z_s dPts[r][s][a],
// so that the [N,1008] product (4 KB a ray) reaches memory only when the caller asks for it.
//
// Exact fp32 on the matrix pipe (v_mfma_f32_32x32x2_f32): D[column][ray] += Wh^T[column][o] * Gh^T[o][ray], the columns as
// the MFMA's rows, so that lane (j, h) ends up with ONE ray (j) and, per 32-column tile T, the columns 32 T + 8 q + 4 h + e of
// register c = 4 q + e: sixteen-byte runs of a dEmb row, and whole coordinates' worth of columns of one ray in one lane pair.
//
// Workgroup = 128 rays = four waves of one 32-ray tile each.  The 1008 columns go in four passes of 252 (= 4 samples x 3
// axes x 21: every coordinate's 21 columns lie inside one pass; eight column tiles, the last four columns of the eighth are
// padding).  Per pass the 256 x 252 block of Wh streams through LDS in eight k-slabs of 32 rows, double-buffered and shared by
// the four waves: Wh is read from L2 once per 128 rays.  Gh rows are re-read per pass (L1 / L2: 1 KB a ray).
// No atomics; every sum runs in a fixed order (MFMA k order, then registers in index order, then the two half-waves): two
// calls give the same bits, and so do the output combinations, which are one kernel with run-time switches.
#include "r2l_dw.h"

#define IG_WG_RAYS 128
#define IG_KSLAB 32                     // rows of Wh (head units o) per LDS slab
#define IG_NSLAB (R2L_W / IG_KSLAB)     // 8
#define IG_PASS_COLS 252                // columns per pass: 4 samples x 3 axes x 21
#define IG_SLAB_COLS 256                // eight 32-column tiles
#define IG_NPASS (R2L_IN / IG_PASS_COLS)  // 4
#define IG_LD (IG_KSLAB * IG_SLAB_COLS / 4 / 256)  // f32x4 loads per thread and slab: 8
static_assert(IG_NPASS * IG_PASS_COLS == R2L_IN, "the passes tile the encoding");

struct R2LInputGradArgs {
    const float* gh;      // [>= N][256] slot 0 of gx
    const float* wh;      // [256][1008]
    const float* rays_o;  // ray form (or all four nullptr)
    const float* rays_d;
    const float* t_rand;
    const float* ztab;
    float* d_emb;         // [N][1008] or nullptr
    float* d_o;           // [N][3], both or neither
    float* d_d;
    int64_t N;
    int emb_vec;          // d_emb is 16-byte aligned: rows are stored as f32x4
};

// slab (pass, ks) of Wh as this thread's IG_LD pieces: f32x4 number q = tid + 256 i of the [32][256] slab, row q / 64, columns
// 4 (q % 64) .. + 3 of the pass; pieces that reach past column 1007 are zeros (only the last pass has them)
__device__ __forceinline__ void ig_load_slab(const float* wh, int pass, int ks, int tid, f32x4 (&st)[IG_LD]) {
#pragma unroll
    for (int i = 0; i < IG_LD; ++i) {
        const int q = tid + 256 * i, row = q >> 6, c4 = (q & 63) * 4;
        const int col = pass * IG_PASS_COLS + c4;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        st[i] = col + 4 <= R2L_IN ? *reinterpret_cast<const f32x4*>(wh + (int64_t)(ks * IG_KSLAB + row) * R2L_IN + col) : zero;
    }
}

__global__ __launch_bounds__(256, 1) void r2l_input_grad_kernel(const R2LInputGradArgs a) {
    __shared__ float slab[2 * IG_KSLAB * IG_SLAB_COLS];  // 64 KiB: two k-slabs
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t tile0 = (int64_t)blockIdx.x * IG_WG_RAYS + wave * R2L_TILE_RAYS;
    const bool live = tile0 < a.N;  // wave-uniform: a wave without rays only helps to stage Wh
    const int64_t ray = tile0 + j;
    const bool mine = ray < a.N;
    const int64_t rl = mine ? ray : a.N - 1;  // rows >= N of gx are padding with undefined content: never read
    const float* grow = a.gh + rl * R2L_W + 4 * h;
    const bool want_rays = a.d_o != nullptr;
    const bool jitter = a.t_rand != nullptr;

    float ro[3] = {0.f, 0.f, 0.f}, rd[3] = {0.f, 0.f, 0.f};
    if (want_rays) {
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            ro[ax] = a.rays_o[rl * 3 + ax];
            rd[ax] = a.rays_d[rl * 3 + ax];
        }
    }
    float sum_o[3] = {0.f, 0.f, 0.f}, sum_d[3] = {0.f, 0.f, 0.f};

    f32x4 st[IG_LD];
    ig_load_slab(a.wh, 0, 0, tid, st);
#pragma unroll
    for (int i = 0; i < IG_LD; ++i) *reinterpret_cast<f32x4*>(slab + (tid + 256 * i) * 4) = st[i];
    __syncthreads();

#pragma unroll 1
    for (int pass = 0; pass < IG_NPASS; ++pass) {
        f32x16 acc[8];
#pragma unroll
        for (int T = 0; T < 8; ++T)
#pragma unroll
            for (int c = 0; c < 16; ++c) acc[T][c] = 0.f;
#pragma unroll 1
        for (int ks = 0; ks < IG_NSLAB; ++ks) {
            const int t = pass * IG_NSLAB + ks;
            const bool more = t + 1 < IG_NPASS * IG_NSLAB;
            if (more) ig_load_slab(a.wh, (t + 1) / IG_NSLAB, (t + 1) % IG_NSLAB, tid, st);
            if (live) {
                // B operands: lane (j, h) supplies Gh[ray j][32 ks + 8 g + 4 h + e] to k-step (g, e); the A operand of that
                // k-step is row 8 g + 4 h + e of the slab
                f32x4 gv[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) gv[g] = *reinterpret_cast<const f32x4*>(grow + ks * IG_KSLAB + 8 * g);
                const float* sl = slab + (t & 1) * (IG_KSLAB * IG_SLAB_COLS) + (4 * h) * IG_SLAB_COLS + j;
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int T = 0; T < 8; ++T)
                            acc[T] = __builtin_amdgcn_mfma_f32_32x32x2f32(sl[(8 * g + e) * IG_SLAB_COLS + 32 * T], gv[g][e], acc[T], 0, 0, 0);
            }
            if (more) {
                float* dst = slab + ((t + 1) & 1) * (IG_KSLAB * IG_SLAB_COLS);
#pragma unroll
                for (int i = 0; i < IG_LD; ++i) *reinterpret_cast<f32x4*>(dst + (tid + 256 * i) * 4) = st[i];
            }
            __syncthreads();  // slab t + 1 is complete; slab t may be overwritten in the next trip
        }
        if (!live) continue;

        // ---- dEmb rows: register quad (T, q) of lane (j, h) = columns 252 pass + 32 T + 8 q + 4 h .. + 3 of ray j ------------
        if (a.d_emb != nullptr && mine) {
            float* row = a.d_emb + ray * R2L_IN + pass * IG_PASS_COLS + 4 * h;
#pragma unroll
            for (int T = 0; T < 8; ++T)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int lc = 32 * T + 8 * q;  // (+ 4 h): a quad lies wholly inside the pass or wholly in its padding
                    if (lc + 4 * h >= IG_PASS_COLS) continue;
                    const f32x4 v = {acc[T][4 * q + 0], acc[T][4 * q + 1], acc[T][4 * q + 2], acc[T][4 * q + 3]};
                    if (a.emb_vec) {
                        *reinterpret_cast<f32x4*>(row + lc) = v;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) row[lc + e] = v[e];
                    }
                }
        }
        if (!want_rays) continue;

        // ---- encoder and sampler backward on the accumulators ------------------------------------------------------------------
        // the pass's four samples: depth and the twelve point coordinates of this lane's ray, formed as the forward forms them
        float z[4], x[12], dp[12];
#pragma unroll
        for (int sp = 0; sp < 4; ++sp) {
            const int s = 4 * pass + sp;
            const float zl = a.ztab[s];  // (the depth rule of r2l_depths, r2l_student_net.h; jitter is a run-time flag here)
            z[sp] = zl;
            if (jitter) z[sp] = zl + a.ztab[16 + s] * a.t_rand[rl * 16 + s];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                x[3 * sp + ax] = ro[ax] + rd[ax] * z[sp];
                dp[3 * sp + ax] = 0.f;
            }
        }
        // column lc = 32 T + 8 q + e + 4 h of the pass: coordinate lc / 21, slot lc % 21 — both known at compile time for h = 0
        // and for h = 1, the lane picks its own; a lane's columns rise with (T, c), so every coordinate's sum runs in column order
#pragma unroll
        for (int T = 0; T < 8; ++T)
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                const int lc0 = 32 * T + 8 * (c >> 2) + (c & 3), lc1 = lc0 + 4;
                if (lc0 >= IG_PASS_COLS) continue;  // (then lc1 is padding too)
                const bool ok1 = lc1 < IG_PASS_COLS;
                const int co0 = lc0 / 21, f0 = lc0 % 21;
                const int co1 = ok1 ? lc1 / 21 : co0, f1 = ok1 ? lc1 % 21 : f0;
                // slot f: f < 10 sin(2^f x) -> 2^f cos; 10 <= f < 20 cos(2^(f-10) x) -> -2^(f-10) sin; 20: x -> 1
                const float sc0 = f0 == 20 ? 1.f : (float)(1 << (f0 % 10)), sc1 = f1 == 20 ? 1.f : (float)(1 << (f1 % 10));
                const float sg0 = (f0 >= 10 && f0 < 20) ? -sc0 : sc0, sg1 = (f1 >= 10 && f1 < 20) ? -sc1 : sc1;
                const float xx = h ? x[co1] : x[co0];
                const float sc = h ? sc1 : sc0;
                float sn, cs;
                r2l_sincos(xx * sc, sn, cs);
                const float tr0 = (f0 >= 10 && f0 < 20) ? sn : cs, tr1 = (f1 >= 10 && f1 < 20) ? sn : cs;
                const float ph0 = f0 == 20 ? 1.f : tr0 * sg0, ph1 = f1 == 20 ? 1.f : tr1 * sg1;
                float v = acc[T][c] * (h ? ph1 : ph0);
                r2l_no_pack(v);
                if (co0 == co1) {
                    dp[co0] += (ok1 || h == 0) ? v : 0.f;
                } else {
                    dp[co0] += h == 0 ? v : 0.f;
                    dp[co1] += h == 1 ? v : 0.f;
                }
            }
        // the two half-waves of a ray, then the pass's four samples in order
#pragma unroll
        for (int k = 0; k < 12; ++k) dp[k] += __shfl_xor(dp[k], 32);
#pragma unroll
        for (int sp = 0; sp < 4; ++sp)
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                sum_o[ax] += dp[3 * sp + ax];
                sum_d[ax] += z[sp] * dp[3 * sp + ax];
            }
    }
    if (want_rays && live && mine && h == 0) {
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            a.d_o[ray * 3 + ax] = sum_o[ax];
            a.d_d[ray * 3 + ax] = sum_d[ax];
        }
    }
}

extern "C" int r2l_backward_input(const float* gx, const float* params, int n_block, const float* rays_o, const float* rays_d,
                                  const float* t_rand, const float* ztab, float* d_emb, float* d_rays_o, float* d_rays_d, int64_t N,
                                  void* stream_) {
    R2L_REQUIRE(d_emb != nullptr || d_rays_o != nullptr || d_rays_d != nullptr, "r2l_backward_input: no output requested (d_emb, d_rays_o and d_rays_d are all NULL)");
    R2L_REQUIRE((d_rays_o != nullptr) == (d_rays_d != nullptr), "r2l_backward_input: d_rays_o and d_rays_d go together (one of them is NULL)");
    R2L_REQUIRE(d_rays_o == nullptr || (rays_o != nullptr && rays_d != nullptr && ztab != nullptr),
                "r2l_backward_input: d_rays_o / d_rays_d need the ray form (rays_o, rays_d, ztab)");
    R2L_REQUIRE(N >= 1, "r2l_backward_input: N < 1");
    R2L_REQUIRE(n_block >= 0 && n_block <= R2L_MAX_BLOCKS, "r2l_backward_input: n_block out of range");
    R2L_REQUIRE(gx != nullptr && params != nullptr, "r2l_backward_input: gx or params is NULL");
    R2L_REQUIRE((((uintptr_t)gx | (uintptr_t)params) & 15u) == 0, "r2l_backward_input: gx and params must be 16-byte aligned");
    R2L_REQUIRE((N + IG_WG_RAYS - 1) / IG_WG_RAYS <= 0x7fffffff, "r2l_backward_input: N too large for one launch");
    R2LInputGradArgs a{};
    a.gh = gx; a.wh = params;  // head.0.weight is first in the flat buffer
    a.d_emb = d_emb; a.d_o = d_rays_o; a.d_d = d_rays_d; a.N = N;
    if (d_rays_o != nullptr) { a.rays_o = rays_o; a.rays_d = rays_d; a.t_rand = t_rand; a.ztab = ztab; }
    a.emb_vec = (((uintptr_t)d_emb) & 15u) == 0 ? 1 : 0;
    hipLaunchKernelGGL(r2l_input_grad_kernel, dim3((unsigned)((N + IG_WG_RAYS - 1) / IG_WG_RAYS)), dim3(256), 0, (hipStream_t)stream_, a);
    R2L_CHECK(hipGetLastError());
    return 0;
}
