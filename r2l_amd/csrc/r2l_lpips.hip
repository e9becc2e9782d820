// r2l_lpips.hip — LPIPS (Zhang et al., CVPR 2018; AlexNet, v0.1, eval mode) of rendered frames against their targets, as the
// test-set loop calls it (main.py:359-369): the five AlexNet feature maps of both images, per position the channel-normalised
// features' weighted squared difference, per layer its spatial mean, the five means added.
//
// The convolutions are implicit GEMMs in exact fp32 on v_mfma_f32_32x32x2_f32: M = images * Ho * Wo (both images of all K pairs
// in one launch: image 2k is a[k], 2k + 1 is b[k]), N = Cout, K = kh * kw * Cin in the order (kh, kw, ci).  Activations are
// NHWC in the work buffer, so for layers 1-4 a 16-deep K slab is 16 contiguous channels of one tap: a lane loads 16 bytes.
// Layer 0 gathers from the [K,H,W,3] images (for one kh the 33 values (kw, ci) of a row are contiguous in memory) and applies
// the stack rescale and the scaling layer while loading; a padded tap is exactly 0.  A workgroup of four waves owns a
// 128 x BN tile; the next slab is fetched into registers while the MFMAs run on the one in LDS.  The weights are packed once
// (r2l_lpips_pack) into the K-major B operand [K][Cout], layer 0's K padded with zero rows to a multiple of the slab depth.
//
// Layers 1-4 have few rows at one pair (1152 for layers 2-4 at 400x400), so their K is split into LP_SPLIT[l] chunks: every
// chunk writes a raw partial slab and a second kernel adds the slabs in increasing chunk order, then bias and ReLU.  The split
// is a constant of the layer: a row's bits depend on neither the number of pairs in the launch nor its tile.
//
// The distance kernel handles one layer: a wave per position computes both channel norms and the weighted squared difference,
// a workgroup (64 positions of ONE pair) writes one partial; the finish kernel adds the partials of every (pair, layer) in a
// fixed order, divides by Ho * Wo and adds the layers in the order 0..4.  No float atomics: the result is bit-reproducible.
#include "r2l_common.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int LP_L = 5;
constexpr int LP_CIN[LP_L] = {3, 64, 192, 384, 256};
constexpr int LP_COUT[LP_L] = {64, 192, 384, 256, 256};
constexpr int LP_KS[LP_L] = {11, 5, 3, 3, 3};
constexpr int LP_STRIDE[LP_L] = {4, 1, 1, 1, 1};
constexpr int LP_PAD[LP_L] = {2, 2, 1, 1, 1};
constexpr int LP_BN[LP_L] = {64, 64, 128, 128, 128};   // tile width: divides Cout, so there is no N tail
constexpr int LP_SPLIT[LP_L] = {1, 2, 9, 12, 12};      // K chunks (1: bias + ReLU in the GEMM's own epilogue)
constexpr int LP_BM = 128, LP_BK = 16, LP_THREADS = 256;
constexpr int LP_LDA = LP_BM + 2;                      // A is k-major in LDS; + 2: the four k-quads of a store hit 32 banks
constexpr int LP_K0 = 11 * 11 * 3, LP_ROW0 = 11 * 3;   // layer 0: K = 363, 33 contiguous values per kernel row
constexpr int LP_MIN_HW = 31;                          // 31 -> 7, 3, 1, 1, 1
constexpr int LP_DPOS = 64, LP_DWAVE = LP_DPOS / 4;    // positions per workgroup / per wave of the distance kernel
constexpr int64_t LP_PARAM_FLOATS = 2470848;

constexpr int lp_kdim(int l) { return LP_KS[l] * LP_KS[l] * LP_CIN[l]; }
constexpr int lp_kpad(int l) { return (lp_kdim(l) + LP_BK - 1) / LP_BK * LP_BK; }
constexpr bool lp_tables_ok() {
    for (int l = 0; l < LP_L; ++l) {
        if (LP_COUT[l] % LP_BN[l] != 0 || LP_COUT[l] % 4 != 0) return false;
        if (l > 0 && (LP_CIN[l] % LP_BK != 0 || LP_CIN[l] != LP_COUT[l - 1] || LP_STRIDE[l] != 1)) return false;
    }
    return lp_kpad(0) == 368;
}
static_assert(lp_tables_ok(), "layer tables: no N tail, a slab of layers 1-4 lies in one tap");

// Everything the host derives from (K, H, W): sizes of the maps and the regions of the work buffer (floats)
struct LpPlan {
    int hi[LP_L], wi[LP_L];      // input of conv l (layer 0: the image; 1, 2: the pooled map)
    int ho[LP_L], wo[LP_L];      // F_l
    int64_t f_off[LP_L];         // F_l: [2K][ho][wo][cout]
    int64_t p_off[2];            // pooled F_0, F_1
    int64_t slab_off, part_off;  // split-K slabs; partials of the distance kernel [K][nb_total]
    int nb[LP_L], nb_off[LP_L], nb_total;
    int64_t map_off[LP_L], map_floats;
    int64_t total;
};

bool lp_plan(int K, int H, int W, LpPlan* P) {
    if (K < 1 || H < LP_MIN_HW || W < LP_MIN_HW) return false;
    int h = H, w = W;
    int64_t off = 0, slab = 0;
    P->nb_total = 0;
    P->map_floats = 0;
    for (int l = 0; l < LP_L; ++l) {
        P->hi[l] = h, P->wi[l] = w;
        P->ho[l] = h = (h + 2 * LP_PAD[l] - LP_KS[l]) / LP_STRIDE[l] + 1;
        P->wo[l] = w = (w + 2 * LP_PAD[l] - LP_KS[l]) / LP_STRIDE[l] + 1;
        const int64_t pos = (int64_t)h * w, m = 2 * (int64_t)K * pos;
        P->f_off[l] = off;
        off += m * LP_COUT[l];
        if (LP_SPLIT[l] > 1 && LP_SPLIT[l] * m * LP_COUT[l] > slab) slab = LP_SPLIT[l] * m * LP_COUT[l];
        P->nb[l] = (int)((pos + LP_DPOS - 1) / LP_DPOS);
        P->nb_off[l] = P->nb_total;
        P->nb_total += P->nb[l];
        P->map_off[l] = P->map_floats;
        P->map_floats += pos;
        if (l < 2) {  // max-pool 3 / 2, no padding, floor
            h = (h - 3) / 2 + 1, w = (w - 3) / 2 + 1;
            P->p_off[l] = off;
            off += 2 * (int64_t)K * h * w * LP_COUT[l];
        }
    }
    P->slab_off = off;
    off += slab;
    P->part_off = off;
    off += ((int64_t)K * P->nb_total + 3) / 4 * 4;
    P->total = off;
    return true;
}

// ---- pack: flat parameters -> [for l: Wp_l [kpad][cout], bias_l [cout]] lin_0 .. lin_4 ------------------------------------
struct LpStream {
    int64_t w[LP_L], b[LP_L], lin[LP_L], total;      // offsets in the packed stream
    int64_t pw[LP_L], pb[LP_L], plin[LP_L];          // offsets in the flat parameters
};
LpStream lp_stream() {
    LpStream s;
    int64_t o = 0, p = 0;
    for (int l = 0; l < LP_L; ++l) {
        s.w[l] = o, o += (int64_t)lp_kpad(l) * LP_COUT[l];
        s.b[l] = o, o += LP_COUT[l];
        s.pw[l] = p, p += (int64_t)lp_kdim(l) * LP_COUT[l];
        s.pb[l] = p, p += LP_COUT[l];
    }
    for (int l = 0; l < LP_L; ++l) {
        s.lin[l] = o, o += LP_COUT[l];
        s.plin[l] = p, p += LP_COUT[l];
    }
    s.total = o;
    return s;
}

// Wp[kk][co] with kk = (kh * ks + kw) * cin + ci  <-  W[co][ci][kh][kw] (torch order); rows kdim .. kpad - 1 are zero
__global__ void lpips_pack_w_kernel(const float* __restrict__ w, float* __restrict__ wp, int cin, int cout, int ks, int kdim,
                                    int kpad) {
    const int64_t n = (int64_t)kpad * cout;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int kk = (int)(i / cout), co = (int)(i % cout);
        float v = 0.f;
        if (kk < kdim) {
            const int tap = kk / cin, ci = kk % cin, kh = tap / ks, kw = tap % ks;
            v = w[(((int64_t)co * cin + ci) * ks + kh) * ks + kw];
        }
        wp[i] = v;
    }
}
__global__ void lpips_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// ---- the convolutions ------------------------------------------------------------------------------------------------------
struct LpConv {
    const float* in;        // layers 1-4: NHWC [2K][hi][wi][cin]
    const float* img_a;     // layer 0: [K][hi][wi][3]
    const float* img_b;
    const float* rescale;   // layer 0: NULL or {min_a, max_a, min_b, max_b}
    const float* wp;        // [kpad][n]
    const float* bias;
    float* out;             // split == 1: relu(acc + bias) [M][n]; else the raw slabs [split][M][n]
    int hi, wi, ho, wo, cin, n, ks, pad;
    int M, nslab, per_split, split;
};

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
    // position of slab s in K: tap (kh, kw) and first channel (layers 1-4)
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

// max-pool 3 / 2 (no padding, floor: every tap is inside) of NHWC maps; c4: float4 per position
__global__ void lpips_pool_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t total4, int hi, int wi, int ho,
                                  int wo, int c4) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total4) return;
    const int c = (int)(i % c4);
    int64_t t = i / c4;
    const int x = (int)(t % wo);
    t /= wo;
    const int y = (int)(t % ho);
    const int64_t im = t / ho;
    const f32x4* src = reinterpret_cast<const f32x4*>(in) + ((im * hi + 2 * y) * wi + 2 * x) * c4 + c;
    f32x4 v = src[0];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const f32x4 u = src[((int64_t)dy * wi + dx) * c4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], u[j]);
        }
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

extern "C" {

int64_t r2l_lpips_param_floats(void) { return LP_PARAM_FLOATS; }

int64_t r2l_lpips_pack_floats(void) { return lp_stream().total; }

int r2l_lpips_pack(const float* params_dev, float* wpack_dev, void* stream) {
    R2L_REQUIRE(params_dev, "r2l_lpips_pack: params_dev is NULL");
    R2L_REQUIRE(wpack_dev, "r2l_lpips_pack: wpack_dev is NULL");
    R2L_REQUIRE(((uintptr_t)wpack_dev & 15) == 0, "r2l_lpips_pack: wpack_dev must be 16-byte aligned");
    const LpStream s = lp_stream();
    hipStream_t st = (hipStream_t)stream;
    for (int l = 0; l < LP_L; ++l) {
        const int64_t n = (int64_t)lp_kpad(l) * LP_COUT[l];
        hipLaunchKernelGGL(lpips_pack_w_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, params_dev + s.pw[l],
                           wpack_dev + s.w[l], LP_CIN[l], LP_COUT[l], LP_KS[l], lp_kdim(l), lp_kpad(l));
        R2L_CHECK(hipGetLastError());
        hipLaunchKernelGGL(lpips_copy_kernel, dim3((LP_COUT[l] + 255) / 256), dim3(256), 0, st, params_dev + s.pb[l],
                           wpack_dev + s.b[l], LP_COUT[l]);
        R2L_CHECK(hipGetLastError());
        hipLaunchKernelGGL(lpips_copy_kernel, dim3((LP_COUT[l] + 255) / 256), dim3(256), 0, st, params_dev + s.plin[l],
                           wpack_dev + s.lin[l], LP_COUT[l]);
        R2L_CHECK(hipGetLastError());
    }
    return 0;
}

int64_t r2l_lpips_work_floats(int K, int H, int W) {
    LpPlan P;
    return lp_plan(K, H, W, &P) ? P.total : -1;
}

int64_t r2l_lpips_map_floats(int H, int W) {
    LpPlan P;
    return lp_plan(1, H, W, &P) ? P.map_floats : -1;
}

int r2l_lpips(const float* img_a, const float* img_b, int K, int H, int W, const float* rescale_dev, const float* wpack, float* work,
              float* per_layer, float* maps, float* out, void* stream) {
    R2L_REQUIRE(K >= 1, "r2l_lpips: K must be at least 1");
    R2L_REQUIRE(H >= LP_MIN_HW && W >= LP_MIN_HW, "r2l_lpips: H and W must be at least 31 (the deepest feature map would be empty)");
    R2L_REQUIRE(H <= 16384 && W <= 16384, "r2l_lpips: H and W must be at most 16384");
    R2L_REQUIRE(img_a, "r2l_lpips: img_a is NULL");
    R2L_REQUIRE(img_b, "r2l_lpips: img_b is NULL");
    R2L_REQUIRE(wpack, "r2l_lpips: wpack is NULL");
    R2L_REQUIRE(work, "r2l_lpips: work is NULL");
    R2L_REQUIRE(out, "r2l_lpips: out is NULL");
    R2L_REQUIRE((((uintptr_t)wpack | (uintptr_t)work) & 15) == 0, "r2l_lpips: wpack and work must be 16-byte aligned");
    LpPlan P;
    lp_plan(K, H, W, &P);
    R2L_REQUIRE(K <= 65535 && 2 * (int64_t)K * P.ho[0] * P.wo[0] <= INT_MAX - LP_BM,
                "r2l_lpips: K exceeds one launch (65535 pairs, 2^31 rows of layer 0)");
    const LpStream S = lp_stream();
    hipStream_t st = (hipStream_t)stream;
    for (int l = 0; l < LP_L; ++l) {
        const int64_t M = 2 * (int64_t)K * P.ho[l] * P.wo[l];
        LpConv c;
        c.in = l == 0 ? nullptr : l < 3 ? work + P.p_off[l - 1] : work + P.f_off[l - 1];
        c.img_a = img_a, c.img_b = img_b, c.rescale = rescale_dev;
        c.wp = wpack + S.w[l], c.bias = wpack + S.b[l];
        c.split = LP_SPLIT[l];
        c.out = work + (c.split > 1 ? P.slab_off : P.f_off[l]);
        c.hi = P.hi[l], c.wi = P.wi[l], c.ho = P.ho[l], c.wo = P.wo[l];
        c.cin = LP_CIN[l], c.n = LP_COUT[l], c.ks = LP_KS[l], c.pad = LP_PAD[l];
        c.M = (int)M, c.nslab = lp_kpad(l) / LP_BK;
        c.per_split = (c.nslab + c.split - 1) / c.split;
        int rc = l == 0 ? lp_launch_conv<64, true>(c, st) : LP_BN[l] == 64 ? lp_launch_conv<64, false>(c, st)
                                                                           : lp_launch_conv<128, false>(c, st);
        if (rc) return rc;
        if (c.split > 1) {
            const int64_t mn4 = M * LP_COUT[l] / 4;
            hipLaunchKernelGGL(lpips_slab_reduce_kernel, dim3((unsigned)((mn4 + 255) / 256)), dim3(256), 0, st, work + P.slab_off,
                               c.split, mn4, LP_COUT[l] / 4, c.bias, work + P.f_off[l]);
            R2L_CHECK(hipGetLastError());
        }
        if (l < 2) {
            const int ph = (P.ho[l] - 3) / 2 + 1, pw = (P.wo[l] - 3) / 2 + 1;
            const int64_t total4 = 2 * (int64_t)K * ph * pw * (LP_COUT[l] / 4);
            hipLaunchKernelGGL(lpips_pool_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, work + P.f_off[l],
                               work + P.p_off[l], total4, P.ho[l], P.wo[l], ph, pw, LP_COUT[l] / 4);
            R2L_CHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(lpips_dist_kernel, dim3((unsigned)P.nb[l], (unsigned)K), dim3(256), 0, st, work + P.f_off[l],
                           wpack + S.lin[l], P.ho[l] * P.wo[l], LP_COUT[l] / 4, maps ? maps + P.map_off[l] : nullptr, P.map_floats,
                           work + P.part_off + P.nb_off[l], P.nb_total);
        R2L_CHECK(hipGetLastError());
    }
    LpFinish fin;
    for (int l = 0; l < LP_L; ++l) fin.nb[l] = P.nb[l], fin.nb_off[l] = P.nb_off[l], fin.count[l] = (float)(P.ho[l] * P.wo[l]);
    fin.nb_total = P.nb_total;
    hipLaunchKernelGGL(lpips_finish_kernel, dim3((unsigned)K), dim3(256), 0, st, work + P.part_off, fin, per_layer, out);
    R2L_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
