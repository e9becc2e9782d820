// r2l_teacher_train.hip — backward pass of the NeRF teacher for training it (step 1 of the pipeline, /root/reference/main.py
// --model_name nerf: render_rays + img2mse(rgb) + img2mse(rgb0) + loss.backward(), main.py:1319-1406), exact fp32 throughout:
//   r2l_raw2outputs_backward : loss seed 2 (rgb_map - target) / (3R) and autograd of raw2outputs (main.py:556-621) -> draw
//   r2l_teacher_backward     : dX chain and weight / bias gradients of NeRF(D=8, W=256, 63+27, skips=[4], use_viewdirs)
//                              (model/nerf_raybased.py:357-401) from draw and the stash of r2l_teacher_mlp_train
//   r2l_teacher_backward_live : the same chain on the live samples of an index list, the count read on the device (occupancy grids
//                              while the teacher trains; below r2l_teacher_backward)
//   r2l_raw2outputs_backward_scaled : the first with the seed scale (or dL/drgb_map itself) an argument, and dL/d|rays_d|
//   r2l_teacher_backward_input      : the same dX chain with no weight product, on to rays_o / rays_d / viewdirs (end of file)
// The products are fp32-input MFMA (v_mfma_f32_32x32x2_f32) in one LDS-tiled GEMM kernel with loader / epilogue functors:
// the dX products G_{l-1} = (G_l W_l) * relu'(h_{l-1}) (weights read row-major, no transposed stream needed) and the weight
// products dW_l = G_l^T A_l reduced over the points in fixed-size chunks into partial slabs, summed in a fixed order by a second
// kernel (no atomics: a step is bit-reproducible).  The positional encodings (A of layer 0, of layer 5's first 63 columns and
// of the views layer's last 27) are not stored: the GEMM's loader recomputes them from (o, d, z) / viewdirs.
#include "r2l_teacher_net.h"

#define TT_BM 128
#define TT_BN 128
#define TT_BK 16
#define TT_KCHUNK 2048  // points per partial slab of a weight gradient: fixed, so the reduction order never changes

// ------------------------------------------------------------------------------------------------------------------
// raw2outputs backward (one wave per ray, S <= 256 samples staged in LDS)
// ------------------------------------------------------------------------------------------------------------------
// Forward (main.py:556-621): dists = [z_{i+1} - z_i, 1e10] * |d| ; a_i = 1 - exp(-relu(raw3_i + noise_i) dists_i) ;
// T_i = prod_{j<i} t_j with t_j = 1 - a_j + 1e-10 ; w_i = a_i T_i ; rgb_map = sum w_i sigmoid(raw_i[:3]) (+ 1 - sum w_i when
// white_bkgd).  With e_i = dL/dw_i = g . rgb_i (- sum g when white_bkgd) and g = dL/drgb_map:
//   dL/da_k = T_k (e_k - U_k),  U_k = sum_{i>k} e_i a_i prod_{k<j<i} t_j   (suffix recurrence U_k = e_{k+1} a_{k+1} + t_{k+1} U_{k+1})
// which is cumprod's backward without a division by t_k (a_k = 1 leaves t_k = 1e-10, where dividing loses the gradient).
#define TT_RB_MAXS 256
__global__ __launch_bounds__(256) void r2l_raw2outputs_bwd_kernel(const float* __restrict__ raw, const float* __restrict__ z,
                                                                  const float* __restrict__ rays_d,
                                                                  const float* __restrict__ noise, int white,
                                                                  const float* __restrict__ target,
                                                                  const float* __restrict__ gseed, float* __restrict__ draw,
                                                                  float* __restrict__ sqerr, float* __restrict__ d_len, int64_t R,
                                                                  int S, float gscale) {
    __shared__ float s_a[4][TT_RB_MAXS], s_t[4][TT_RB_MAXS], s_da[4][TT_RB_MAXS], s_e[4][TT_RB_MAXS], s_T[4][TT_RB_MAXS];
    // Only when d_len is asked for: s_dn = d a / d |d| = relu(sigma) (z_{i+1} - z_i) exp(..), and a second, accurate pair
    // (a', t') = (-expm1(-x), exp(-x) + 1e-10) for d_len's own dL/da.  The pair above is the reference's fp32 arithmetic, whose
    // 1 - a keeps three digits of t behind a nearly opaque sample (a within 1e-4 of 1): draw, measured against the ray's
    // largest entry, does not notice, but d_len of such a ray IS those small terms.
    __shared__ float s_dn[4][TT_RB_MAXS], s_ap[4][TT_RB_MAXS], s_tp[4][TT_RB_MAXS];
    __shared__ float s_rgb[4][TT_RB_MAXS][3];
    __shared__ float s_g[4][3];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + wave;
    const bool live = r < R;  // (no early return: the barriers below are block-wide)
    const int64_t rc = live ? r : R - 1;
    const float d0 = rays_d[rc * 3], d1 = rays_d[rc * 3 + 1], d2 = rays_d[rc * 3 + 2];
    const float dn = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
    const float* rr = raw + rc * S * 4;
    const float* zr = z + rc * S;
    for (int i = lane; i < S && live; i += 64) {
        const float dz = i + 1 < S ? zr[i + 1] - zr[i] : 1e10f;
        const float dist = dz * dn;
        const float sig = noise ? rr[4 * i + 3] + noise[rc * S + i] : rr[4 * i + 3];
        const float xx = fmaxf(sig, 0.f) * dist;
        const float ex = expf(-xx);
        const float a = 1.0f - ex;
        s_a[wave][i] = a;
        s_t[wave][i] = (1.0f - a) + 1e-10f;
        s_da[wave][i] = sig > 0.f ? dist * ex : 0.f;  // d a / d raw3 (relu'(0) = 0, as torch)
        if (d_len) {
            s_dn[wave][i] = sig > 0.f ? (sig * dz) * ex : 0.f;
            s_ap[wave][i] = -expm1f(-xx);
            s_tp[wave][i] = ex + 1e-10f;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) s_rgb[wave][i][c] = 1.0f / (1.0f + expf(-rr[4 * i + c]));
    }
    __syncthreads();
    if (lane == 0 && live) {
        float T = 1.0f, acc = 0.f, m[3] = {0.f, 0.f, 0.f};
        for (int i = 0; i < S; ++i) {  // cumprod order of the reference
            const float w = s_a[wave][i] * T;
            s_T[wave][i] = T;
            acc += w;
#pragma unroll
            for (int c = 0; c < 3; ++c) m[c] += w * s_rgb[wave][i][c];
            T *= s_t[wave][i];
        }
        if (d_len) {  // s_dn <- T' d a / d |d| with the accurate transmittance T' = prod t'
            float Tp = 1.0f;
            for (int i = 0; i < S; ++i) {
                s_dn[wave][i] *= Tp;
                Tp *= s_tp[wave][i];
            }
        }
        float g[3], se = 0.f, gsum = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float rgb = white ? m[c] + (1.0f - acc) : m[c];
            if (gseed) {
                g[c] = gseed[r * 3 + c];  // dL/drgb_map itself: no target, no loss
            } else {
                const float diff = rgb - target[r * 3 + c];
                se += diff * diff;
                g[c] = gscale * diff;  // d img2mse / d rgb_map = 2 (rgb - target) / (3 R) at the default scale
            }
            gsum += g[c];
            s_g[wave][c] = g[c];
        }
        if (!gseed) sqerr[r] = se;
        float U = 0.f, Up = 0.f, dl = 0.f;
        for (int k = S - 1; k >= 0; --k) {
            const float e = g[0] * s_rgb[wave][k][0] + g[1] * s_rgb[wave][k][1] + g[2] * s_rgb[wave][k][2] -
                            (white ? gsum : 0.f);
            s_e[wave][k] = s_T[wave][k] * (e - U);  // dL/da_k
            if (d_len) {  // fixed order: last sample first; dL/da'_k = T'_k (e_k - U'_k)
                dl += (e - Up) * s_dn[wave][k];
                float eap = e * s_ap[wave][k];
                r2l_no_pack(eap);
                Up = eap + s_tp[wave][k] * Up;
            }
            float ea = e * s_a[wave][k];
            r2l_no_pack(ea);  // (the two products would pair into a v_pk_mul_f32 + a swizzled v_pk_add_f32: build.py's ISA audit)
            U = ea + s_t[wave][k] * U;
        }
        if (d_len) d_len[r] = dl;
    }
    __syncthreads();
    if (!live) return;
    const float g0 = s_g[wave][0], g1 = s_g[wave][1], g2 = s_g[wave][2];
    for (int i = lane; i < S; i += 64) {
        const float w = s_a[wave][i] * s_T[wave][i];
        f32x4 o;
        const float gg[3] = {g0, g1, g2};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float sg = s_rgb[wave][i][c];
            o[c] = w * gg[c] * (sg * (1.0f - sg));
        }
        o[3] = s_e[wave][i] * s_da[wave][i];
        *reinterpret_cast<f32x4*>(draw + (r * S + i) * 4) = o;
    }
}

static int tt_raw2outputs_backward(const float* raw, const float* z, const float* rays_d, const float* noise, int white_bkgd,
                                   const float* target, const float* g, float grad_scale, float* draw, float* sqerr,
                                   float* d_len, int64_t R, int S, hipStream_t st) {
    hipLaunchKernelGGL(r2l_raw2outputs_bwd_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, st, raw, z, rays_d, noise,
                       white_bkgd, target, g, draw, sqerr, d_len, R, S, grad_scale);
    R2L_CHECK(hipGetLastError());
    return 0;
}

extern "C" int r2l_raw2outputs_backward(const float* raw, const float* z, const float* rays_d, const float* noise, int white_bkgd,
                                        const float* target, float* draw, float* sqerr, int64_t R, int S, void* stream) {
    R2L_REQUIRE(R >= 0 && S >= 1 && S <= TT_RB_MAXS, "r2l_raw2outputs_backward: need R >= 0 and 1 <= S <= 256");
    if (R == 0) return 0;
    R2L_REQUIRE(raw && z && rays_d && target && draw && sqerr, "r2l_raw2outputs_backward: a required pointer is NULL");
    return tt_raw2outputs_backward(raw, z, rays_d, noise, white_bkgd, target, nullptr, (float)(2.0 / (3.0 * (double)R)), draw,
                                   sqerr, nullptr, R, S, (hipStream_t)stream);
}

extern "C" int r2l_raw2outputs_backward_scaled(const float* raw, const float* z, const float* rays_d, const float* noise,
                                               int white_bkgd, const float* target, const float* g, float grad_scale,
                                               float* draw, float* sqerr, float* d_len, int64_t R, int S, void* stream) {
    R2L_REQUIRE(R >= 0 && S >= 1 && S <= TT_RB_MAXS, "r2l_raw2outputs_backward_scaled: need R >= 0 and 1 <= S <= 256");
    if (R == 0) return 0;
    R2L_REQUIRE(raw && z && rays_d && draw, "r2l_raw2outputs_backward_scaled: a required pointer is NULL");
    R2L_REQUIRE(g || (target && sqerr), "r2l_raw2outputs_backward_scaled: without g, target and sqerr are required");
    return tt_raw2outputs_backward(raw, z, rays_d, noise, white_bkgd, target, g, grad_scale, draw, sqerr, d_len, R, S,
                                   (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------------------------
// GEMM: C[M,N] = sum_k A[m,k] B[k,n] on v_mfma_f32_32x32x2_f32.  128 x 128 block tile, 4 waves of 64 x 64 (2 x 2 MFMA
// tiles), K staged through LDS 16 at a time.  blockIdx.z = one K chunk of `kchunk` (the weight products); the epilogue gets
// (row, col, value, chunk).  Loaders return the operand element (the caller keeps indices in range).
// ------------------------------------------------------------------------------------------------------------------
struct LdRowA {  // A[m,k] = p[m*ld + k]   (dX: the layer's output gradient, k along a row)
    const float* p;
    int ld;
    static constexpr bool KFAST = true;
    __device__ float operator()(int64_t m, int64_t k) const { return p[m * ld + k]; }
};
struct LdTransA {  // A[m,k] = p[k*ld + m]   (dW: G^T, the points are k)
    const float* p;
    int ld;
    static constexpr bool KFAST = false;
    __device__ float operator()(int64_t m, int64_t k) const { return p[k * ld + m]; }
};
struct LdWeightB {  // B[k,n] = W[k*ld + col0 + n]   (dX: row k = output feature of the layer, n = input feature)
    const float* w;
    int ld, col0;
    __device__ float operator()(int64_t k, int64_t n) const { return w[k * ld + col0 + n]; }
};
// B[k = point, n] = the input row of a layer: [PE(xyz) (nx cols)] [stashed activation (w1 cols, row stride w1)] [PE(dir) (nd)]
struct LdActB {
    const float* act;
    const float *rays_o, *rays_d, *viewdirs, *z;
    int S, nx, w1, nd;
    __device__ float operator()(int64_t p, int64_t n) const {
        if (n < nx) {  // embed xyz, helpers:24-56: [x, sin(2^0 x), cos(2^0 x), ...]
            const int64_t ray = p / S;
            const int c = (int)n;
            const int ax = c < 3 ? c : (c - 3) % 3;
            const float x = rays_o[ray * 3 + ax] + rays_d[ray * 3 + ax] * z[p];  // as the forward: mul / add rounded separately
            return tt_pe(x, c);
        }
        n -= nx;
        if (n < w1) return act[p * w1 + n];
        n -= w1;
        const int64_t ray = p / S;
        const int c = (int)n;
        return tt_pe(viewdirs[ray * 3 + (c < 3 ? c : (c - 3) % 3)], c);
    }
    // column c of the encoding of one coordinate value x (c < 3: x itself; else frequency (c-3)/6, sin for (c-3)%6 < 3)
    __device__ static float tt_pe(float x, int c) {
        if (c < 3) return x;
        const int f = (c - 3) / 6;
        float sn, cs;
        r2l_sincos(x * (float)(1 << f), sn, cs);
        return (c - 3) % 6 < 3 ? sn : cs;
    }
};
// dX epilogue: out[m*ld + n] = (v + r1a[4m] r1b[n]) * (mask[m*ld_mask + n] > 0)  (rank-1 term and mask optional)
struct EpDX {
    float* out;
    int ld;
    const float* mask;
    int mask_ld;
    const float* r1a;
    const float* r1b;
    int64_t M;
    int N;
    __device__ void operator()(int64_t m, int n, float v, int) const {
        if (m >= M || n >= N) return;
        if (r1a) v += r1a[m * 4] * r1b[n];
        if (mask && !(mask[m * mask_ld + n] > 0.f)) v = 0.f;
        out[m * ld + n] = v;
    }
};
// dW epilogue: partial slab [chunk][M][N + 1] (column N = the bias partial, written by the kernel's row sums)
struct EpSlab {
    float* slab;
    int64_t M;
    int N;
    __device__ void operator()(int64_t m, int n, float v, int z) const {
        if (m >= M || n >= N) return;
        slab[((int64_t)z * M + m) * (N + 1) + n] = v;
    }
};

// (the kernel's body as a function: the live kernels below run it behind their own read of the device count)
template <class LA, class LB, class EP>
__device__ __forceinline__ void tt_gemm_tile(const LA& la, const LB& lb, const EP& ep, int64_t M, int N, int64_t K, int64_t kchunk,
                                             float* bias_slab) {
    __shared__ float As[TT_BK][TT_BM + 1];
    __shared__ float Bs[TT_BK][TT_BN + 1];
    __shared__ float rs[2][TT_BM];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l = lane & 31;
    const int64_t m0 = (int64_t)blockIdx.y * TT_BM;
    const int n0 = blockIdx.x * TT_BN;
    const int64_t kb = (int64_t)blockIdx.z * kchunk, ke = kb + kchunk < K ? kb + kchunk : K;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    // row sums of A over this chunk (dW: the bias gradient), only in the first column block, fixed order
    const bool rowsum = bias_slab != nullptr && blockIdx.x == 0;
    float rsum = 0.f;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    for (int64_t k0 = kb; k0 < ke; k0 += TT_BK) {
#pragma unroll
        for (int r = 0; r < TT_BM * TT_BK / 256; ++r) {
            const int e = tid + 256 * r;
            const int mm = LA::KFAST ? e / TT_BK : e % TT_BM, kk = LA::KFAST ? e % TT_BK : e / TT_BM;
            As[kk][mm] = (m0 + mm < M && k0 + kk < ke) ? la(m0 + mm, k0 + kk) : 0.f;
        }
#pragma unroll
        for (int r = 0; r < TT_BN * TT_BK / 256; ++r) {
            const int e = tid + 256 * r;
            const int nn = e % TT_BN, kk = e / TT_BN;
            Bs[kk][nn] = (n0 + nn < N && k0 + kk < ke) ? lb(k0 + kk, n0 + nn) : 0.f;
        }
        __syncthreads();
        if (rowsum) {
#pragma unroll
            for (int kk = 0; kk < TT_BK / 2; ++kk) rsum += As[(tid >> 7) * (TT_BK / 2) + kk][tid & 127];
        }
#pragma unroll
        for (int kk = 0; kk < TT_BK; kk += 2) {
            const float a0 = As[kk + h][wm + l], a1 = As[kk + h][wm + 32 + l];
            const float b0 = Bs[kk + h][wn + l], b1 = Bs[kk + h][wn + 32 + l];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
    // D layout of 32x32x2: column = lane & 31, row = 8 (r / 4) + 4 (lane / 32) + r % 4
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                ep(m0 + wm + 32 * i + 8 * (r >> 2) + 4 * h + (r & 3), n0 + wn + 32 * j + l, acc[i][j][r], blockIdx.z);
    if (rowsum) {
        rs[tid >> 7][tid & 127] = rsum;
        __syncthreads();
        if (tid < TT_BM && m0 + tid < M) bias_slab[((int64_t)blockIdx.z * M + m0 + tid) * (N + 1) + N] = rs[0][tid] + rs[1][tid];
    }
}

template <class LA, class LB, class EP>
__global__ __launch_bounds__(256) void tt_gemm_kernel(const LA la, const LB lb, const EP ep, int64_t M, int N, int64_t K,
                                                      int64_t kchunk, float* bias_slab) {
    tt_gemm_tile(la, lb, ep, M, N, K, kchunk, bias_slab);
}

// ---- live form (r2l_teacher_backward_live): the points are rows 0 .. count - 1 of a launch sized for the capacity `cap`, and the
// count = min(*count_dev, cap) is read here, by every launch of the chain (an ordinary load of one address, as the forward's live form).
__device__ __forceinline__ int64_t tt_live_count(const int64_t* __restrict__ count_dev, int64_t cap) {
    const int64_t c = *count_dev;
    return c < cap ? c : cap;
}
// dX: the points are the rows.  A tile whose first row is at or past the count leaves whole, before any staging or barrier;
// a partly filled tile stores rows below the count only.
template <class LA, class LB>
__global__ __launch_bounds__(256) void tt_gemm_live_dx_kernel(const LA la, const LB lb, EpDX ep, int N, int64_t K,
                                                              const int64_t* __restrict__ count_dev, int64_t cap) {
    const int64_t cnt = tt_live_count(count_dev, cap);
    if ((int64_t)blockIdx.y * TT_BM >= cnt) return;
    ep.M = cnt;
    tt_gemm_tile(la, lb, ep, cnt, N, K, K, nullptr);
}
// dW: the points are K.  A chunk (blockIdx.z) at or past the count leaves whole and writes no slab; the last live chunk ends at
// the count, as the plain form's last chunk ends at P.
template <class LA, class LB>
__global__ __launch_bounds__(256) void tt_gemm_live_dw_kernel(const LA la, const LB lb, const EpSlab ep, int64_t M, int N,
                                                              const int64_t* __restrict__ count_dev, int64_t cap, float* bias_slab) {
    const int64_t cnt = tt_live_count(count_dev, cap);
    if ((int64_t)blockIdx.z * TT_KCHUNK >= cnt) return;
    tt_gemm_tile(la, lb, ep, M, N, cnt, TT_KCHUNK, bias_slab);
}

// grads[w_off + m*N + n] = sum_z slab[z][m][n] (n < N), grads[b_off + m] = sum_z slab[z][m][N]; z in increasing order
__global__ void tt_slab_reduce_kernel(const float* __restrict__ slab, int Z, int64_t M, int N, float* __restrict__ grads,
                                      int64_t w_off, int64_t b_off) {
    const int64_t cols = N + 1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M * cols; i += (int64_t)gridDim.x * blockDim.x) {
        float s = 0.f;
        for (int zz = 0; zz < Z; ++zz) s += slab[(int64_t)zz * M * cols + i];
        const int64_t m = i / cols;
        const int n = (int)(i % cols);
        if (n < N) grads[w_off + m * N + n] = s;
        else grads[b_off + m] = s;
    }
}

// G_views[p, j] = (sum_c drgb[p, c] W_rgb[c, j]) * (relu(v)[p, j] > 0)   (rgb_linear^T and the views layer's ReLU)
__global__ void tt_rgb_head_dx_kernel(const float* __restrict__ draw, const float* __restrict__ rgb_w,
                                      const float* __restrict__ vstash, float* __restrict__ gv, int64_t P) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P * 128; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = i >> 7;
        const int j = (int)(i & 127);
        const float v = draw[p * 4] * rgb_w[j] + draw[p * 4 + 1] * rgb_w[128 + j] + draw[p * 4 + 2] * rgb_w[256 + j];
        gv[i] = vstash[i] > 0.f ? v : 0.f;
    }
}

template <class LA, class LB, class EP>
static int tt_gemm(const LA& la, const LB& lb, const EP& ep, int64_t M, int N, int64_t K, int64_t kchunk, float* bias_slab,
                   hipStream_t st) {
    const int64_t nz = (K + kchunk - 1) / kchunk;
    R2L_REQUIRE((M + TT_BM - 1) / TT_BM < 65536 && nz < 65536, "r2l_teacher_backward: too many points for one call");
    const dim3 grid((unsigned)((N + TT_BN - 1) / TT_BN), (unsigned)((M + TT_BM - 1) / TT_BM), (unsigned)nz);
    hipLaunchKernelGGL((tt_gemm_kernel<LA, LB, EP>), grid, dim3(256), 0, st, la, lb, ep, M, N, K, kchunk, bias_slab);
    R2L_CHECK(hipGetLastError());
    return 0;
}

// dW (and db) of one layer: grads[w_off + m*N + n] = sum_p G[p, m] B[p, n], grads[b_off + m] = sum_p G[p, m]
static int tt_weight_grad(const float* G, int ldg, int64_t M, const LdActB& b, int N, int64_t P, float* slab, float* grads,
                          int64_t w_off, int64_t b_off, hipStream_t st) {
    const int Z = (int)((P + TT_KCHUNK - 1) / TT_KCHUNK);
    const EpSlab ep{slab, M, N};
    if (int rc = tt_gemm(LdTransA{G, ldg}, b, ep, M, N, P, TT_KCHUNK, slab, st)) return rc;
    const int64_t n = M * (N + 1);
    hipLaunchKernelGGL(tt_slab_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, slab, Z, M, N, grads, w_off,
                       b_off);
    R2L_CHECK(hipGetLastError());
    return 0;
}

// dX of one layer: out[P, N] = (G[P, Kout] W[Kout, col0 : col0 + N]) (+ rank-1) * relu'(mask)
static int tt_dx(const float* G, int ldg, int Kout, const float* w, int ldw, int col0, int N, float* out, const float* mask,
                 const float* r1a, const float* r1b, int64_t P, hipStream_t st) {
    const EpDX ep{out, N, mask, N, r1a, r1b, P, N};
    return tt_gemm(LdRowA{G, ldg}, LdWeightB{w, ldw, col0}, ep, P, N, Kout, Kout, nullptr, st);
}

static int64_t tt_slab_floats(int64_t P) { return ((P + TT_KCHUNK - 1) / TT_KCHUNK) * (int64_t)T_W * (T_W + T_XYZ + 1); }

extern "C" int64_t r2l_teacher_train_work_floats(int64_t P) {
    if (P < 0) return -1;
    return 2 * P * T_W + P * T_VIEWS + tt_slab_floats(P);  // G ping, G pong, G of the views layer, slabs
}

extern "C" int r2l_teacher_backward(const float* rays_o, const float* rays_d, const float* viewdirs, const float* z,
                                    const float* tparams, const float* stash, const float* draw, float* grads, float* work,
                                    int64_t R, int S, void* stream) {
    R2L_REQUIRE(R >= 0 && S >= 0, "r2l_teacher_backward: negative R / S");
    const TOff off = t_offsets();
    const int64_t P = R * (int64_t)S;
    if (P == 0) {  // no points: every gradient is zero
        R2L_REQUIRE(grads, "r2l_teacher_backward: grads is NULL");
        R2L_CHECK(hipMemsetAsync(grads, 0, sizeof(float) * off.total, (hipStream_t)stream));
        return 0;
    }
    R2L_REQUIRE(rays_o && rays_d && viewdirs && z && tparams && stash && draw && grads && work,
                "r2l_teacher_backward: a required pointer is NULL");
    const hipStream_t st = (hipStream_t)stream;
    const float* W = tparams;
    float* ga = work;
    float* gb = ga + P * T_W;
    float* gv = gb + P * T_W;
    float* slab = gv + P * T_VIEWS;
    auto slot = [&](int l) { return T_STASH_SLOT(stash, (int64_t)l, P); };
    const float* vst = slot(T_STASH_VIEWS);  // relu(views layer), [P,128]
    auto act = [&](const float* a, int nx, int w1, int nd) { return LdActB{a, rays_o, rays_d, viewdirs, z, S, nx, w1, nd}; };
    int rc;
    // heads: rgb_linear (128 -> 3) and alpha_linear (256 -> 1) weight gradients; G of the views layer
    if ((rc = tt_weight_grad(draw, 4, 3, act(vst, 0, T_VIEWS, 0), T_VIEWS, P, slab, grads, off.rgb_w, off.rgb_b, st))) return rc;
    if ((rc = tt_weight_grad(draw + 3, 4, 1, act(slot(7), 0, T_W, 0), T_W, P, slab, grads, off.alpha_w, off.alpha_b, st)))
        return rc;
    hipLaunchKernelGGL(tt_rgb_head_dx_kernel, dim3((unsigned)((P * T_VIEWS + 255) / 256 < 65536 ? (P * T_VIEWS + 255) / 256 : 65536)),
                       dim3(256), 0, st, draw, W + off.rgb_w, vst, gv, P);
    R2L_CHECK(hipGetLastError());
    // views layer: dW over [feature, PE(dir)]; dX to the feature (the direction encoding is a constant)
    if ((rc = tt_weight_grad(gv, T_VIEWS, T_VIEWS, act(slot(T_STASH_FEAT), 0, T_W, T_DIR), T_W + T_DIR, P, slab, grads, off.views_w,
                             off.views_b, st)))
        return rc;
    if ((rc = tt_dx(gv, T_VIEWS, T_VIEWS, W + off.views_w, T_W + T_DIR, 0, T_W, ga, nullptr, nullptr, nullptr, P, st))) return rc;
    // feature_linear: dW over h7; dX into h7 plus the alpha head's d sigma (x) w_alpha, then relu'(h7)
    if ((rc = tt_weight_grad(ga, T_W, T_W, act(slot(7), 0, T_W, 0), T_W, P, slab, grads, off.feat_w, off.feat_b, st)))
        return rc;
    if ((rc = tt_dx(ga, T_W, T_W, W + off.feat_w, T_W, 0, T_W, gb, slot(7), draw + 3, W + off.alpha_w, P, st))) return rc;
    // layers 7 .. 1: G (pre-activation gradient of layer l) in `cur`; layer 5's input is [PE(xyz), h4]
    float* cur = gb;
    float* nxt = ga;
    for (int l = 7; l >= 1; --l) {
        const int nx = l == 5 ? T_XYZ : 0;
        const int fin = nx + T_W;
        if ((rc = tt_weight_grad(cur, T_W, T_W, act(slot(l - 1), nx, T_W, 0), fin, P, slab, grads, off.w[l], off.b[l], st)))
            return rc;
        if ((rc = tt_dx(cur, T_W, T_W, W + off.w[l], fin, nx, T_W, nxt, slot(l - 1), nullptr, nullptr, P, st))) return rc;
        float* t = cur; cur = nxt; nxt = t;
    }
    // layer 0: dW over PE(xyz)
    return tt_weight_grad(cur, T_W, T_W, act(nullptr, T_XYZ, 0, 0), T_XYZ, P, slab, grads, off.w[0], off.b[0], st);
}

// ------------------------------------------------------------------------------------------------------------------
// The same backward on the live samples of an index list, the count left on the device (r2l_teacher_backward_live): the chain
// above with every launch sized for the capacity P and reading count = min(*count_dev, P) itself.  Point p < count is sample
// idx[p]: the stash of r2l_teacher_mlp_train_live is compact (row p), draw is gathered to [count,4] first, and the encoder operand
// reads ray idx[p] / S and z[idx[p]].  Every product then runs over rows / chunks 0 .. count - 1 exactly as the plain chain runs
// over 0 .. P - 1 on the compacted problem, so the two give the same bits.
// ------------------------------------------------------------------------------------------------------------------
// LdActB with the encodings read through idx (a number outside [0, cap) reads sample 0 in its place; its draw row is zero)
struct LdActBLive {
    const float* act;
    const float *rays_o, *rays_d, *viewdirs, *z;
    const int64_t* idx;
    int64_t cap;
    int S, nx, w1, nd;
    __device__ int64_t sample(int64_t p) const {
        const int64_t n = idx[p];
        return n >= 0 && n < cap ? n : 0;
    }
    __device__ float operator()(int64_t p, int64_t n) const {
        if (n < nx) {
            const int64_t s = sample(p), ray = s / S;
            const int c = (int)n;
            const int ax = c < 3 ? c : (c - 3) % 3;
            const float x = rays_o[ray * 3 + ax] + rays_d[ray * 3 + ax] * z[s];  // as the forward: mul / add rounded separately
            return LdActB::tt_pe(x, c);
        }
        n -= nx;
        if (n < w1) return act[p * w1 + n];
        n -= w1;
        const int64_t ray = sample(p) / S;
        const int c = (int)n;
        return LdActB::tt_pe(viewdirs[ray * 3 + (c < 3 ? c : (c - 3) % 3)], c);
    }
};

// dg[p] = draw[idx[p]] for p < count (zero for a number outside [0, cap)): one thread per float
__global__ void tt_gather_draw_kernel(const float* __restrict__ draw, const int64_t* __restrict__ idx,
                                      const int64_t* __restrict__ count_dev, int64_t cap, float* __restrict__ dg) {
    const int64_t cnt = tt_live_count(count_dev, cap);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cnt * 4; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t n = idx[i >> 2];
        dg[i] = n >= 0 && n < cap ? draw[n * 4 + (i & 3)] : 0.f;
    }
}

// tt_rgb_head_dx_kernel over the live rows
__global__ void tt_rgb_head_dx_live_kernel(const float* __restrict__ draw, const float* __restrict__ rgb_w,
                                           const float* __restrict__ vstash, float* __restrict__ gv,
                                           const int64_t* __restrict__ count_dev, int64_t cap) {
    const int64_t cnt = tt_live_count(count_dev, cap);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cnt * 128; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = i >> 7;
        const int j = (int)(i & 127);
        const float v = draw[p * 4] * rgb_w[j] + draw[p * 4 + 1] * rgb_w[128 + j] + draw[p * 4 + 2] * rgb_w[256 + j];
        gv[i] = vstash[i] > 0.f ? v : 0.f;
    }
}

// tt_slab_reduce_kernel over the live chunks, in increasing order (none: the gradient is zero)
__global__ void tt_slab_reduce_live_kernel(const float* __restrict__ slab, const int64_t* __restrict__ count_dev, int64_t cap,
                                           int64_t M, int N, float* __restrict__ grads, int64_t w_off, int64_t b_off) {
    const int64_t cnt = tt_live_count(count_dev, cap);
    const int Z = cnt > 0 ? (int)((cnt + TT_KCHUNK - 1) / TT_KCHUNK) : 0;
    const int64_t cols = N + 1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M * cols; i += (int64_t)gridDim.x * blockDim.x) {
        float s = 0.f;
        for (int zz = 0; zz < Z; ++zz) s += slab[(int64_t)zz * M * cols + i];
        const int64_t m = i / cols;
        const int n = (int)(i % cols);
        if (n < N) grads[w_off + m * N + n] = s;
        else grads[b_off + m] = s;
    }
}

struct TTLive {
    const int64_t* count_dev;
    int64_t cap;
};

static int tt_weight_grad_live(const float* G, int ldg, int64_t M, const LdActBLive& b, int N, const TTLive& lv, float* slab,
                               float* grads, int64_t w_off, int64_t b_off, hipStream_t st) {
    const int64_t nz = (lv.cap + TT_KCHUNK - 1) / TT_KCHUNK;  // (< 65536: checked by the entry point)
    const dim3 grid((unsigned)((N + TT_BN - 1) / TT_BN), (unsigned)((M + TT_BM - 1) / TT_BM), (unsigned)nz);
    hipLaunchKernelGGL((tt_gemm_live_dw_kernel<LdTransA, LdActBLive>), grid, dim3(256), 0, st, LdTransA{G, ldg}, b,
                       EpSlab{slab, M, N}, M, N, lv.count_dev, lv.cap, slab);
    R2L_CHECK(hipGetLastError());
    const int64_t n = M * (N + 1);
    hipLaunchKernelGGL(tt_slab_reduce_live_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, slab, lv.count_dev, lv.cap, M, N,
                       grads, w_off, b_off);
    R2L_CHECK(hipGetLastError());
    return 0;
}

static int tt_dx_live(const float* G, int ldg, int Kout, const float* w, int ldw, int col0, int N, float* out, const float* mask,
                      const float* r1a, const float* r1b, const TTLive& lv, hipStream_t st) {
    const EpDX ep{out, N, mask, N, r1a, r1b, lv.cap, N};  // (.M: the kernel puts the count there)
    const dim3 grid((unsigned)((N + TT_BN - 1) / TT_BN), (unsigned)((lv.cap + TT_BM - 1) / TT_BM), 1);
    hipLaunchKernelGGL((tt_gemm_live_dx_kernel<LdRowA, LdWeightB>), grid, dim3(256), 0, st, LdRowA{G, ldg}, LdWeightB{w, ldw, col0}, ep,
                       N, (int64_t)Kout, lv.count_dev, lv.cap);
    R2L_CHECK(hipGetLastError());
    return 0;
}

extern "C" int64_t r2l_teacher_train_live_work_floats(int64_t P) {
    if (P < 0) return -1;
    return r2l_teacher_train_work_floats(P) + 4 * P;  // r2l_teacher_backward's, then the gathered draw [P,4]
}

extern "C" int r2l_teacher_backward_live(const float* rays_o, const float* rays_d, const float* viewdirs, const float* z,
                                         const int64_t* idx, const int64_t* count_dev, const float* tparams, const float* stash,
                                         const float* draw, float* grads, float* work, int64_t R, int S, void* stream) {
    R2L_REQUIRE(R >= 0, "r2l_teacher_backward_live: R is negative");
    R2L_REQUIRE(S >= 1, "r2l_teacher_backward_live: S: need S >= 1");
    R2L_REQUIRE(R < ((int64_t)1 << 31) && R * (int64_t)S < (int64_t)65535 * TT_BM,
                "r2l_teacher_backward_live: R*S: too many points for one call (need R*S < 65535 * 128)");
    R2L_REQUIRE(grads != nullptr, "r2l_teacher_backward_live: grads is NULL");
    const TOff off = t_offsets();
    const int64_t P = R * (int64_t)S;
    const hipStream_t st = (hipStream_t)stream;
    if (P == 0) {  // no points: every gradient is zero
        R2L_CHECK(hipMemsetAsync(grads, 0, sizeof(float) * off.total, st));
        return 0;
    }
    R2L_REQUIRE(rays_o != nullptr, "r2l_teacher_backward_live: rays_o is NULL");
    R2L_REQUIRE(rays_d != nullptr, "r2l_teacher_backward_live: rays_d is NULL");
    R2L_REQUIRE(viewdirs != nullptr, "r2l_teacher_backward_live: viewdirs is NULL");
    R2L_REQUIRE(z != nullptr, "r2l_teacher_backward_live: z is NULL");
    R2L_REQUIRE(idx != nullptr, "r2l_teacher_backward_live: idx is NULL");
    R2L_REQUIRE(count_dev != nullptr, "r2l_teacher_backward_live: count_dev is NULL");
    R2L_REQUIRE(tparams != nullptr, "r2l_teacher_backward_live: tparams is NULL");
    R2L_REQUIRE(stash != nullptr, "r2l_teacher_backward_live: stash is NULL");
    R2L_REQUIRE(draw != nullptr, "r2l_teacher_backward_live: draw is NULL");
    R2L_REQUIRE(work != nullptr, "r2l_teacher_backward_live: work is NULL");
    const float* W = tparams;
    float* ga = work;
    float* gb = ga + P * T_W;
    float* gv = gb + P * T_W;
    float* slab = gv + P * T_VIEWS;
    float* dg = slab + tt_slab_floats(P);
    const TTLive lv{count_dev, P};
    auto slot = [&](int l) { return T_STASH_SLOT(stash, (int64_t)l, P); };  // compact rows, the slots where a stash of P points has them
    const float* vst = slot(T_STASH_VIEWS);
    auto act = [&](const float* a, int nx, int w1, int nd) { return LdActBLive{a, rays_o, rays_d, viewdirs, z, idx, P, S, nx, w1, nd}; };
    const unsigned nblk = (unsigned)((P * T_VIEWS + 255) / 256 < 65536 ? (P * T_VIEWS + 255) / 256 : 65536);
    int rc;
    hipLaunchKernelGGL(tt_gather_draw_kernel, dim3((unsigned)((P * 4 + 255) / 256 < 65536 ? (P * 4 + 255) / 256 : 65536)), dim3(256), 0, st,
                       draw, idx, count_dev, P, dg);
    R2L_CHECK(hipGetLastError());
    // from here on: r2l_teacher_backward's sequence with draw = dg and the live launches
    if ((rc = tt_weight_grad_live(dg, 4, 3, act(vst, 0, T_VIEWS, 0), T_VIEWS, lv, slab, grads, off.rgb_w, off.rgb_b, st))) return rc;
    if ((rc = tt_weight_grad_live(dg + 3, 4, 1, act(slot(7), 0, T_W, 0), T_W, lv, slab, grads, off.alpha_w, off.alpha_b, st))) return rc;
    hipLaunchKernelGGL(tt_rgb_head_dx_live_kernel, dim3(nblk), dim3(256), 0, st, dg, W + off.rgb_w, vst, gv, count_dev, P);
    R2L_CHECK(hipGetLastError());
    if ((rc = tt_weight_grad_live(gv, T_VIEWS, T_VIEWS, act(slot(T_STASH_FEAT), 0, T_W, T_DIR), T_W + T_DIR, lv, slab, grads,
                                  off.views_w, off.views_b, st)))
        return rc;
    if ((rc = tt_dx_live(gv, T_VIEWS, T_VIEWS, W + off.views_w, T_W + T_DIR, 0, T_W, ga, nullptr, nullptr, nullptr, lv, st))) return rc;
    if ((rc = tt_weight_grad_live(ga, T_W, T_W, act(slot(7), 0, T_W, 0), T_W, lv, slab, grads, off.feat_w, off.feat_b, st))) return rc;
    if ((rc = tt_dx_live(ga, T_W, T_W, W + off.feat_w, T_W, 0, T_W, gb, slot(7), dg + 3, W + off.alpha_w, lv, st))) return rc;
    float* cur = gb;
    float* nxt = ga;
    for (int l = 7; l >= 1; --l) {
        const int nx = l == 5 ? T_XYZ : 0;
        const int fin = nx + T_W;
        if ((rc = tt_weight_grad_live(cur, T_W, T_W, act(slot(l - 1), nx, T_W, 0), fin, lv, slab, grads, off.w[l], off.b[l], st)))
            return rc;
        if ((rc = tt_dx_live(cur, T_W, T_W, W + off.w[l], fin, nx, T_W, nxt, slot(l - 1), nullptr, nullptr, lv, st))) return rc;
        float* t = cur; cur = nxt; nxt = t;
    }
    return tt_weight_grad_live(cur, T_W, T_W, act(nullptr, T_XYZ, 0, 0), T_XYZ, lv, slab, grads, off.w[0], off.b[0], st);
}

// ------------------------------------------------------------------------------------------------------------------
// Backward to the rays (a frozen teacher: iNeRF-style localisation, density normals).  The dX chain above with no weight
// product and no slab, then the three input-side products
//   d_pe_xyz[P,63] = G_0 W_0 + G_5 W_5[:, 0:63]        d_pe_dir[P,27] = G_views W_views[:, 256:283]
// through the same GEMM, then one wave per ray: the encoder's derivative per point
//   d_x = g_x + sum_k 2^k (cos(2^k x) g_sin_k - sin(2^k x) g_cos_k)      (r2l_sincos at the frequency itself, as the forward)
// and the sums over the ray's samples (lane l takes samples l, l + 64, .. in order, then a fixed xor tree over the lanes).
// The per-ray pass reads whole rays, so a ray that straddles GEMM tiles needs no special case and nothing is atomic.
// ------------------------------------------------------------------------------------------------------------------
// accumulating epilogue: out[m*ld + n] += v (one thread per entry)
struct EpDXAdd {
    float* out;
    int ld;
    int64_t M;
    int N;
    __device__ void operator()(int64_t m, int n, float v, int) const {
        if (m >= M || n >= N) return;
        out[m * ld + n] += v;
    }
};

template <int L>
__device__ __forceinline__ void tt_pe_backward(const float (&x)[3], const float* __restrict__ g, float (&dx)[3]) {
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        float acc = g[ax];
#pragma unroll
        for (int k = 0; k < L; ++k) {
            const float f = (float)(1 << k);
            float sn, cs;
            r2l_sincos(x[ax] * f, sn, cs);
            acc += f * (cs * g[3 + 6 * k + ax] - sn * g[3 + 6 * k + 3 + ax]);
        }
        dx[ax] = acc;
    }
}

__device__ __forceinline__ float tt_wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__global__ __launch_bounds__(256) void tt_input_reduce_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                              const float* __restrict__ viewdirs, const float* __restrict__ z,
                                                              const float* __restrict__ dpe_x, const float* __restrict__ dpe_d,
                                                              const float* __restrict__ d_len, int fold,
                                                              float* __restrict__ d_rays_o, float* __restrict__ d_rays_d,
                                                              float* __restrict__ d_viewdirs, float* __restrict__ d_pts, int64_t R,
                                                              int S) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;  // (whole waves leave: the shuffles below are wave-wide)
    const float o[3] = {rays_o[r * 3], rays_o[r * 3 + 1], rays_o[r * 3 + 2]};
    const float d[3] = {rays_d[r * 3], rays_d[r * 3 + 1], rays_d[r * 3 + 2]};
    float so[3] = {0.f, 0.f, 0.f}, sd[3] = {0.f, 0.f, 0.f}, sv[3] = {0.f, 0.f, 0.f};
    const bool want_x = dpe_x != nullptr;
    float vd[3] = {0.f, 0.f, 0.f};
    if (dpe_d) {
        vd[0] = viewdirs[r * 3]; vd[1] = viewdirs[r * 3 + 1]; vd[2] = viewdirs[r * 3 + 2];
    }
    for (int s = lane; s < S; s += 64) {
        const int64_t p = r * S + s;
        if (want_x) {
            const float zz = z[p];
            float x[3], dx[3];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) x[ax] = o[ax] + d[ax] * zz;  // as the forward: mul / add rounded separately
            tt_pe_backward<10>(x, dpe_x + p * T_XYZ, dx);
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                if (d_pts) d_pts[p * 3 + ax] = dx[ax];
                so[ax] += dx[ax];
                sd[ax] += zz * dx[ax];
            }
        }
        if (dpe_d) {
            float dv[3];
            tt_pe_backward<4>(vd, dpe_d + p * T_DIR, dv);
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) sv[ax] += dv[ax];
        }
    }
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        so[ax] = tt_wave_sum(so[ax]);
        sd[ax] = tt_wave_sum(sd[ax]);
        sv[ax] = tt_wave_sum(sv[ax]);
    }
    if (lane != 0) return;
    if (d_viewdirs)
        for (int ax = 0; ax < 3; ++ax) d_viewdirs[r * 3 + ax] = sv[ax];
    if (!d_rays_d) return;
    if (d_len || fold) {
        const float dn = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        if (d_len) {
            const float dl = d_len[r];
            for (int ax = 0; ax < 3; ++ax) sd[ax] += dl * (d[ax] / dn);
        }
        if (fold) {  // viewdirs = rays_d / |rays_d|: the normalisation's Jacobian (I - v v^T) / |d|
            const float dot = sv[0] * vd[0] + sv[1] * vd[1] + sv[2] * vd[2];
            for (int ax = 0; ax < 3; ++ax) sd[ax] += (sv[ax] - dot * vd[ax]) / dn;
        }
    }
    for (int ax = 0; ax < 3; ++ax) {
        d_rays_o[r * 3 + ax] = so[ax];
        d_rays_d[r * 3 + ax] = sd[ax];
    }
}

extern "C" int64_t r2l_teacher_input_grad_work_floats(int64_t P) {
    if (P < 0) return -1;
    return 2 * P * T_W + P * T_VIEWS + P * T_XYZ + P * T_DIR;  // G ping, G pong, G of the views layer, d_pe_xyz, d_pe_dir
}

extern "C" int r2l_teacher_backward_input(const float* rays_o, const float* rays_d, const float* viewdirs, const float* z,
                                          const float* tparams, const float* stash, const float* draw, const float* d_len,
                                          int fold_viewdirs, float* d_rays_o, float* d_rays_d, float* d_viewdirs, float* d_pts,
                                          float* work, int64_t R, int S, void* stream) {
    R2L_REQUIRE(R >= 0 && S >= 1 && S <= TT_RB_MAXS, "r2l_teacher_backward_input: need R >= 0 and 1 <= S <= 256");
    R2L_REQUIRE(d_rays_o || d_rays_d || d_viewdirs || d_pts, "r2l_teacher_backward_input: no output requested");
    R2L_REQUIRE((d_rays_o != nullptr) == (d_rays_d != nullptr),
                "r2l_teacher_backward_input: d_rays_o and d_rays_d are given together or not at all");
    if (R == 0) return 0;
    R2L_REQUIRE(rays_o && rays_d && viewdirs && z && tparams && stash && draw && work,
                "r2l_teacher_backward_input: a required pointer is NULL");
    const TOff off = t_offsets();
    const int64_t P = R * (int64_t)S;
    const hipStream_t st = (hipStream_t)stream;
    const float* W = tparams;
    float* ga = work;
    float* gb = ga + P * T_W;
    float* gv = gb + P * T_W;
    float* dpx = gv + P * T_VIEWS;
    float* dpd = dpx + P * T_XYZ;
    auto slot = [&](int l) { return T_STASH_SLOT(stash, (int64_t)l, P); };
    const bool want_x = d_rays_d || d_pts;
    const bool want_dir = d_viewdirs || (d_rays_d && fold_viewdirs);  // the folding term needs d_viewdirs, returned or not
    int rc;
    hipLaunchKernelGGL(tt_rgb_head_dx_kernel, dim3((unsigned)((P * T_VIEWS + 255) / 256 < 65536 ? (P * T_VIEWS + 255) / 256 : 65536)),
                       dim3(256), 0, st, draw, W + off.rgb_w, slot(T_STASH_VIEWS), gv, P);
    R2L_CHECK(hipGetLastError());
    if (want_dir &&
        (rc = tt_dx(gv, T_VIEWS, T_VIEWS, W + off.views_w, T_W + T_DIR, T_W, T_DIR, dpd, nullptr, nullptr, nullptr, P, st)))
        return rc;
    if (want_x) {
        if ((rc = tt_dx(gv, T_VIEWS, T_VIEWS, W + off.views_w, T_W + T_DIR, 0, T_W, ga, nullptr, nullptr, nullptr, P, st))) return rc;
        if ((rc = tt_dx(ga, T_W, T_W, W + off.feat_w, T_W, 0, T_W, gb, slot(7), draw + 3, W + off.alpha_w, P, st))) return rc;
        float* cur = gb;
        float* nxt = ga;
        for (int l = 7; l >= 1; --l) {
            const int nx = l == 5 ? T_XYZ : 0;
            if (nx && (rc = tt_dx(cur, T_W, T_W, W + off.w[l], nx + T_W, 0, T_XYZ, dpx, nullptr, nullptr, nullptr, P, st))) return rc;
            if ((rc = tt_dx(cur, T_W, T_W, W + off.w[l], nx + T_W, nx, T_W, nxt, slot(l - 1), nullptr, nullptr, P, st))) return rc;
            float* t = cur; cur = nxt; nxt = t;
        }
        const EpDXAdd ep{dpx, T_XYZ, P, T_XYZ};  // + G_0 W_0 onto layer 5's share
        if ((rc = tt_gemm(LdRowA{cur, T_W}, LdWeightB{W + off.w[0], T_XYZ, 0}, ep, P, T_XYZ, T_W, T_W, nullptr, st))) return rc;
    }
    hipLaunchKernelGGL(tt_input_reduce_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, st, rays_o, rays_d, viewdirs, z,
                       want_x ? dpx : (const float*)nullptr, want_dir ? dpd : (const float*)nullptr, d_len, fold_viewdirs,
                       d_rays_o, d_rays_d, d_viewdirs, d_pts, R, S);
    R2L_CHECK(hipGetLastError());
    return 0;
}
