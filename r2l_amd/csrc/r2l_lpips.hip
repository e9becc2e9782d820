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
#include "r2l_lpips_conv.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int LP_CIN[LP_L] = {3, 64, 192, 384, 256};
constexpr int LP_COUT[LP_L] = {64, 192, 384, 256, 256};
constexpr int LP_KS[LP_L] = {11, 5, 3, 3, 3};
constexpr int LP_STRIDE[LP_L] = {4, 1, 1, 1, 1};
constexpr int LP_PAD[LP_L] = {2, 2, 1, 1, 1};
constexpr int LP_BN[LP_L] = {64, 64, 128, 128, 128};   // tile width: divides Cout, so there is no N tail
constexpr int LP_SPLIT[LP_L] = {1, 2, 9, 12, 12};      // K chunks (1: bias + ReLU in the GEMM's own epilogue)
constexpr int LP_MIN_HW = 31;                          // 31 -> 7, 3, 1, 1, 1
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

// (the convolution, slab-reduce, distance and finish kernels: r2l_lpips_conv.h, shared with r2l_lpips_vgg.hip)

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
