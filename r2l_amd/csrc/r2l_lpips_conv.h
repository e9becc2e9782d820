// r2l_lpips_conv.h — the kernels that the LPIPS variants share (r2l_lpips.hip: AlexNet; r2l_lpips_vgg.hip: VGG-16): the
// implicit-GEMM convolution on v_mfma_f32_32x32x2_f32 with its split-K slab reduce, the distance kernel of one layer and the
// finish kernel.  Every variant has five taps (LP_L).  Each file that includes this gets its own copies (anonymous namespace).
#pragma once
#include "r2l_common.h"

namespace {

constexpr int LP_L = 5;
constexpr int LP_BM = 128, LP_BK = 16, LP_THREADS = 256;
constexpr int LP_LDA = LP_BM + 2;                      // A is k-major in LDS; + 2: the four k-quads of a store hit 32 banks
constexpr int LP_K0 = 11 * 11 * 3, LP_ROW0 = 11 * 3;   // AlexNet layer 0 (FIRST): K = 363, 33 contiguous values per kernel row
constexpr int LP_DPOS = 64, LP_DWAVE = LP_DPOS / 4;    // positions per workgroup / per wave of the distance kernel

__global__ void lpips_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// ---- the convolutions ------------------------------------------------------------------------------------------------------
struct LpConv {
    const float* in;        // !FIRST: NHWC [images][hi][wi][cin]
    const float* img_a;     // FIRST: [K][hi][wi][3]
    const float* img_b;
    const float* rescale;   // FIRST: NULL or {min_a, max_a, min_b, max_b}
    const float* wp;        // [kpad][n]
    const float* bias;
    float* out;             // split == 1: relu(acc + bias) [M][n]; else the raw slabs [split][M][n]
    int hi, wi, ho, wo, cin, n, ks, pad;
    int M, nslab, per_split, split;
};

// FIRST: AlexNet's 11 x 11 / 4 gather from the [K,H,W,3] images.  !FIRST: any stride-1 ks x ks convolution of an NHWC map with
// cin % 16 == 0 (a 16-deep K slab is 16 contiguous channels of one tap)
template <int BN, bool FIRST>
__global__ __launch_bounds__(LP_THREADS) void lpips_conv_kernel(const LpConv p) {
    constexpr int NJ = BN / 64, LDB = BN + 4, NB4 = BN / 64;  // NB4: float4 of the B slab per thread
    __shared__ float As[LP_BK][LP_LDA];
    __shared__ __attribute__((aligned(16))) float Bs[LP_BK][LDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l = lane & 31;
    const int m0 = blockIdx.x * LP_BM, n0 = blockIdx.y * BN;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * (BN / 2);
    const int s_begin = blockIdx.z * p.per_split, s_end = min(s_begin + p.per_split, p.nslab);
    const int pos = p.ho * p.wo;

    // the rows this thread stages: FIRST one row and eight k, else two rows (64 apart) and one k-quad
    constexpr int NR = FIRST ? 1 : 2;
    bool valid[NR];
    int iy0[NR], ix0[NR];
    int64_t base[NR];  // element offset of (image, iy0, ix0, channel 0)
    float sc = 1.f, mn = 0.f;
    const float* img = nullptr;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int m = m0 + (FIRST ? (tid & (LP_BM - 1)) : (tid >> 2) + 64 * r);
        valid[r] = m < p.M;
        const int mm = valid[r] ? m : 0;
        const int im = mm / pos, rem = mm - im * pos, oy = rem / p.wo, ox = rem - oy * p.wo;
        if (FIRST) {
            iy0[r] = oy * 4 - p.pad, ix0[r] = ox * 4 - p.pad;
            img = (im & 1) ? p.img_b : p.img_a;
            base[r] = (((int64_t)(im >> 1) * p.hi + iy0[r]) * p.wi + ix0[r]) * 3;
            if (p.rescale) {  // the stack's rescale to [-1, 1] (main.py:361-363), as r2l_flip applies it
                mn = p.rescale[2 * (im & 1)];
                sc = 2.f / (p.rescale[2 * (im & 1) + 1] - mn);
            }
        } else {
            iy0[r] = oy - p.pad, ix0[r] = ox - p.pad;
            base[r] = (((int64_t)im * p.hi + iy0[r]) * p.wi + ix0[r]) * p.cin + 4 * (tid & 3);
        }
    }
    // position of slab s in K: tap (kh, kw) and first channel (!FIRST)
    int ci0 = 0, kh = 0, kw = 0;
    if (!FIRST) {
        const int k0 = s_begin * LP_BK, tap = k0 / p.cin;
        ci0 = k0 - tap * p.cin, kh = tap / p.ks, kw = tap - kh * p.ks;
    }
    f32x4 ra[2], rb[NB4];
    auto fetch = [&](int s) {
        if (FIRST) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int kk = s * LP_BK + (tid >> 7) + 2 * j;
                const int ky = kk / LP_ROW0, rem = kk - ky * LP_ROW0, kx = rem / 3, c = rem - kx * 3;
                const int iy = iy0[0] + ky, ix = ix0[0] + kx;
                float v = 0.f;
                if (valid[0] && kk < LP_K0 && (unsigned)iy < (unsigned)p.hi && (unsigned)ix < (unsigned)p.wi) {
                    v = img[base[0] + (int64_t)ky * p.wi * 3 + rem];
                    if (p.rescale) v = sc * (v - mn) - 1.f;
                    // the scaling layer: (x - shift) / scale
                    v = c == 0 ? (v + 0.030f) / 0.458f : c == 1 ? (v + 0.088f) / 0.448f : (v + 0.188f) / 0.450f;
                }
                ra[j >> 2][j & 3] = v;
            }
        } else {
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const int iy = iy0[r] + kh, ix = ix0[r] + kw;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (valid[r] && (unsigned)iy < (unsigned)p.hi && (unsigned)ix < (unsigned)p.wi)
                    v = *reinterpret_cast<const f32x4*>(p.in + base[r] + ((int64_t)kh * p.wi + kw) * p.cin + ci0);
                ra[r] = v;
            }
            ci0 += LP_BK;
            if (ci0 == p.cin) {
                ci0 = 0;
                if (++kw == p.ks) kw = 0, ++kh;
            }
        }
#pragma unroll
        for (int r = 0; r < NB4; ++r) {
            const int e = tid + LP_THREADS * r, kr = e / (BN / 4), nq = e % (BN / 4);
            rb[r] = *reinterpret_cast<const f32x4*>(p.wp + (int64_t)(s * LP_BK + kr) * p.n + n0 + 4 * nq);
        }
    };
    auto stage = [&]() {
        if (FIRST) {
#pragma unroll
            for (int j = 0; j < 8; ++j) As[(tid >> 7) + 2 * j][tid & (LP_BM - 1)] = ra[j >> 2][j & 3];
        } else {
#pragma unroll
            for (int r = 0; r < NR; ++r)
#pragma unroll
                for (int j = 0; j < 4; ++j) As[4 * (tid & 3) + j][(tid >> 2) + 64 * r] = ra[r][j];
        }
#pragma unroll
        for (int r = 0; r < NB4; ++r) {
            const int e = tid + LP_THREADS * r, kr = e / (BN / 4), nq = e % (BN / 4);
            *reinterpret_cast<f32x4*>(&Bs[kr][4 * nq]) = rb[r];
        }
    };

    f32x16 acc[2][NJ];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    if (s_begin < s_end) fetch(s_begin);
    for (int s = s_begin; s < s_end; ++s) {
        stage();
        __syncthreads();
        if (s + 1 < s_end) fetch(s + 1);
#pragma unroll
        for (int kk = 0; kk < LP_BK; kk += 2) {
            const float a0 = As[kk + h][wm + l], a1 = As[kk + h][wm + 32 + l];
            float b[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) b[j] = Bs[kk + h][wn + 32 * j + l];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b[j], acc[0][j], 0, 0, 0);
                acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b[j], acc[1][j], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // D layout of 32x32x2: column = lane & 31, row = 8 (r / 4) + 4 (lane / 32) + r % 4
    float* out = p.out + (p.split > 1 ? (int64_t)blockIdx.z * p.M * p.n : 0);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int n = n0 + wn + 32 * j + l;
        const float bias = p.split > 1 ? 0.f : p.bias[n];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm + 32 * i + 8 * (r >> 2) + 4 * h + (r & 3);
                if (m < p.M) out[(int64_t)m * p.n + n] = p.split > 1 ? acc[i][j][r] : fmaxf(acc[i][j][r] + bias, 0.f);
            }
    }
}

// out[m][n] = relu(slab_0[m][n] + slab_1[m][n] + ... + bias[n]): the K chunks in increasing order (n4: float4 per row)
__global__ void lpips_slab_reduce_kernel(const float* __restrict__ slab, int split, int64_t mn4, int n4,
                                         const float* __restrict__ bias, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= mn4) return;
    const f32x4* s = reinterpret_cast<const f32x4*>(slab);
    f32x4 v = s[i];
    for (int z = 1; z < split; ++z) v += s[(int64_t)z * mn4 + i];
    v += reinterpret_cast<const f32x4*>(bias)[i % n4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.f);
    reinterpret_cast<f32x4*>(out)[i] = v;
}

// ---- distance --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float lp_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One layer.  grid (nb, K): workgroup (b, k) handles positions 64 b .. 64 b + 63 of pair k, a wave 16 of them one after the
// other: d = sum_c w[c] (a[c] / (|a| + 1e-10) - b[c] / (|b| + 1e-10))^2.  c4 = C / 4 <= 128: two float4 per lane and image.
__global__ __launch_bounds__(256) void lpips_dist_kernel(const float* __restrict__ f, const float* __restrict__ lin, int pos, int c4,
                                                         float* __restrict__ map, int64_t map_stride,
                                                         float* __restrict__ partial, int nb_total) {
    __shared__ float red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, k = blockIdx.y;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 w[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) w[i] = lane + 64 * i < c4 ? reinterpret_cast<const f32x4*>(lin)[lane + 64 * i] : zero;
    float wsum = 0.f;
    for (int t = 0; t < LP_DWAVE; ++t) {
        const int q = blockIdx.x * LP_DPOS + wave * LP_DWAVE + t;
        if (q >= pos) break;  // (wave-uniform)
        const f32x4* fa = reinterpret_cast<const f32x4*>(f) + ((int64_t)(2 * k) * pos + q) * c4;
        const f32x4* fb = fa + (int64_t)pos * c4;
        f32x4 a[2], b[2];
        float sa = 0.f, sb = 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const bool in = lane + 64 * i < c4;
            a[i] = in ? fa[lane + 64 * i] : zero;
            b[i] = in ? fb[lane + 64 * i] : zero;
#pragma unroll
            for (int j = 0; j < 4; ++j) sa += a[i][j] * a[i][j], sb += b[i][j] * b[i][j];
        }
        const float da = sqrtf(lp_wave_sum(sa)) + 1e-10f, db = sqrtf(lp_wave_sum(sb)) + 1e-10f;
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float e = a[i][j] / da - b[i][j] / db;
                d += w[i][j] * (e * e);
            }
        d = lp_wave_sum(d);
        if (lane == 0 && map) map[(int64_t)k * map_stride + q] = d;
        wsum += d;
    }
    if (lane == 0) red[wave] = wsum;
    __syncthreads();
    if (threadIdx.x == 0) partial[(int64_t)k * nb_total + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

struct LpFinish {
    int nb[LP_L], nb_off[LP_L], nb_total;
    float count[LP_L];
};
// out[k] = v_0 + v_1 + v_2 + v_3 + v_4, v_l = (the partials of (k, l) in a fixed order) / (Ho Wo)
__global__ __launch_bounds__(256) void lpips_finish_kernel(const float* __restrict__ partial, const LpFinish fin,
                                                           float* __restrict__ per_layer, float* __restrict__ out) {
    __shared__ float red[LP_L][4];
    const float* p = partial + (int64_t)blockIdx.x * fin.nb_total;
#pragma unroll
    for (int l = 0; l < LP_L; ++l) {
        float v = 0.f;
        for (int i = threadIdx.x; i < fin.nb[l]; i += 256) v += p[fin.nb_off[l] + i];
        v = lp_wave_sum(v);
        if ((threadIdx.x & 63) == 0) red[l][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float total = 0.f;
#pragma unroll
        for (int l = 0; l < LP_L; ++l) {
            const float v = ((red[l][0] + red[l][1]) + (red[l][2] + red[l][3])) / fin.count[l];
            if (per_layer) per_layer[(int64_t)blockIdx.x * LP_L + l] = v;
            total = l == 0 ? v : total + v;
        }
        out[blockIdx.x] = total;
    }
}

template <int BN, bool FIRST>
int lp_launch_conv(const LpConv& c, hipStream_t st) {
    const dim3 grid((unsigned)((c.M + LP_BM - 1) / LP_BM), (unsigned)(c.n / BN), (unsigned)c.split);
    hipLaunchKernelGGL((lpips_conv_kernel<BN, FIRST>), grid, dim3(LP_THREADS), 0, st, c);
    R2L_CHECK(hipGetLastError());
    return 0;
}

}  // namespace
