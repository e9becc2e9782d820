// r2l_lpips_vgg.hip — LPIPS (Zhang et al., CVPR 2018; VGG-16, v0.1, eval mode: lpips.LPIPS(net='vgg')) of rendered frames against
// their targets: the variant the published NeRF / R2L tables report.  Thirteen 3 x 3 / 1 / 1 convolutions with bias and ReLU in
// five stages (64, 128, 256, 512, 512 channels; a 2 x 2 / 2 max-pool, floor, between the stages), the taps are the last map of
// every stage; distance, per-layer mean and total exactly as in r2l_lpips.hip.
//
// Every convolution is an instance of lpips_conv_kernel<BN, false> (r2l_lpips_conv.h: exact fp32 on v_mfma_f32_32x32x2_f32,
// NHWC, both images of all K pairs in one launch).  Convolution 0 (Cin = 3) is too: a prologue kernel writes the image, after
// the stack rescale and the scaling layer, as NHWC with 16 channels of which 13 are zero, and the packed weights of layer 0 have
// zero rows for them (K = 144 instead of 27: 5.9 of the 196 GFLOP of a 400 x 400 pair, against a second gather loader to
// maintain).  The padding of the convolution is applied to that map, so a padded tap is exactly 0 after rescale and scaling.
//
// Tiles: BN = 64 for the 64-channel stage, 128 elsewhere.  One 400 x 400 pair has 2 * 2500 rows in stage 3 and 2 * 625 in stage
// 4 (40 and 10 row tiles of 128), so these split K: 3 chunks in stage 3 (480 workgroups), 9 in stage 4 (360); the chunks are
// added in increasing order by lpips_slab_reduce_kernel.  Stages 0-2 have 2500 / 625 / 314 workgroups without a split.  The
// split is a constant of the layer: a pair's bits depend neither on K nor on the pair's place in the launch.
//
// Work buffer: the maps are full resolution (2 * 160 000 * 64 floats for each of conv1_1 and conv1_2 of a 400 x 400 pair), so
// only three regions exist: R0 and R1 take the non-tap maps, the pooled maps and the 16-channel image in turn, T holds the
// live tap, whose distance is taken before the pool overwrites R0.  With the split-K slabs and the distance partials that is
// 235.5 MB per 400 x 400 pair and 942.1 MB per 800 x 800 pair (r2l_lpips_vgg_work_floats(1, H, W) * 4), against 345.6 / 1382.4
// MB for all thirteen maps; conv1_1 and conv1_2 alone, which must exist together, are 163.8 / 655.4 MB.
#include "r2l_lpips_conv.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int LV_N = 13;
constexpr int LV_CIN[LV_N] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
constexpr int LV_COUT[LV_N] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
constexpr int LV_STAGE[LV_N] = {0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4};
constexpr int LV_TAP[LP_L] = {1, 3, 6, 9, 12};         // conv1_2, conv2_2, conv3_3, conv4_3, conv5_3
constexpr int LV_SPLIT_OF_STAGE[LP_L] = {1, 1, 1, 3, 9};
// regions of the work buffer: 0 = R0, 1 = R1, 2 = T.  The image goes to R1, every pool writes R0.
constexpr int LV_IN[LV_N] = {1, 0, 0, 1, 0, 1, 0, 0, 1, 0, 0, 1, 0};
constexpr int LV_OUT[LV_N] = {0, 2, 1, 2, 1, 0, 2, 1, 0, 2, 1, 0, 2};
constexpr int LV_C0 = 16;                               // channels of the prologue's image map
constexpr int LV_MIN_HW = 16;                           // 16 -> 8 -> 4 -> 2 -> 1
constexpr int64_t LV_PARAM_FLOATS = 14716160;

constexpr int lv_cinp(int l) { return l == 0 ? LV_C0 : LV_CIN[l]; }
constexpr int lv_kpad(int l) { return 9 * lv_cinp(l); }
constexpr int lv_bn(int l) { return LV_COUT[l] == 64 ? 64 : 128; }
constexpr int lv_split(int l) { return LV_SPLIT_OF_STAGE[LV_STAGE[l]]; }
constexpr int64_t lv_param_floats() {
    int64_t n = 0;
    for (int l = 0; l < LV_N; ++l) n += 9 * (int64_t)LV_CIN[l] * LV_COUT[l] + LV_COUT[l];
    for (int s = 0; s < LP_L; ++s) n += LV_COUT[LV_TAP[s]];
    return n;
}
constexpr bool lv_tables_ok() {
    for (int l = 0; l < LV_N; ++l) {
        if (LV_COUT[l] % lv_bn(l) != 0 || lv_cinp(l) % LP_BK != 0 || LV_COUT[l] > 512) return false;
        if (l > 0 && LV_CIN[l] != LV_COUT[l - 1]) return false;
        if ((lv_kpad(l) / LP_BK) % lv_split(l) != 0) return false;                  // equal chunks
        if (LV_OUT[l] == LV_IN[l] || (l > 0 && LV_STAGE[l] == LV_STAGE[l - 1] && LV_IN[l] != LV_OUT[l - 1])) return false;
        if (l > 0 && LV_STAGE[l] != LV_STAGE[l - 1] && (LV_IN[l] != 0 || LV_OUT[l - 1] != 2)) return false;
    }
    for (int s = 0; s < LP_L; ++s)
        if (LV_OUT[LV_TAP[s]] != 2 || LV_STAGE[LV_TAP[s]] != s) return false;
    return LV_IN[0] == 1 && lv_param_floats() == LV_PARAM_FLOATS;
}
static_assert(lv_tables_ok(), "layer tables: no N tail, a slab lies in one tap, the regions chain, the parameter count");

// Everything the host derives from (K, H, W)
struct LvPlan {
    int h[LP_L], w[LP_L];        // the maps of stage s
    int64_t reg_off[3];          // R0, R1, T
    int64_t slab_off, part_off;
    int nb[LP_L], nb_off[LP_L], nb_total;
    int64_t map_off[LP_L], map_floats;
    int64_t total;
};

bool lv_plan(int K, int H, int W, LvPlan* P) {
    if (K < 1 || H < LV_MIN_HW || W < LV_MIN_HW) return false;
    if (2 * (int64_t)K * H * W > (int64_t)INT_MAX - LP_BM) return false;  // the kernels index rows with int
    int64_t reg[3] = {0, 0, 0}, slab = 0;
    auto use = [&](int r, int64_t n) { if (n > reg[r]) reg[r] = n; };
    P->nb_total = 0;
    P->map_floats = 0;
    for (int s = 0, h = H, w = W; s < LP_L; ++s, h /= 2, w /= 2) {
        P->h[s] = h, P->w[s] = w;
        const int64_t pos = (int64_t)h * w;
        P->nb[s] = (int)((pos + LP_DPOS - 1) / LP_DPOS);
        P->nb_off[s] = P->nb_total;
        P->nb_total += P->nb[s];
        P->map_off[s] = P->map_floats;
        P->map_floats += pos;
    }
    use(1, 2 * (int64_t)K * H * W * LV_C0);
    for (int l = 0; l < LV_N; ++l) {
        const int s = LV_STAGE[l];
        const int64_t mn = 2 * (int64_t)K * P->h[s] * P->w[s] * LV_COUT[l];
        use(LV_OUT[l], mn);
        if (lv_split(l) > 1 && lv_split(l) * mn > slab) slab = lv_split(l) * mn;
        if (l == LV_TAP[s] && s + 1 < LP_L) use(0, 2 * (int64_t)K * P->h[s + 1] * P->w[s + 1] * LV_COUT[l]);
    }
    int64_t off = 0;
    for (int r = 0; r < 3; ++r) P->reg_off[r] = off, off += reg[r];   // (multiples of 16 floats)
    P->slab_off = off;
    off += slab;
    P->part_off = off;
    off += ((int64_t)K * P->nb_total + 3) / 4 * 4;
    P->total = off;
    return true;
}

// ---- pack: flat parameters -> [for l: Wp_l [9 cinp][cout], bias_l [cout]] lin_0 .. lin_4 ----------------------------------
struct LvStream {
    int64_t w[LV_N], b[LV_N], lin[LP_L], total;      // offsets in the packed stream
    int64_t pw[LV_N], pb[LV_N], plin[LP_L];          // offsets in the flat parameters
};
LvStream lv_stream() {
    LvStream s;
    int64_t o = 0, p = 0;
    for (int l = 0; l < LV_N; ++l) {
        s.w[l] = o, o += (int64_t)lv_kpad(l) * LV_COUT[l];
        s.b[l] = o, o += LV_COUT[l];
        s.pw[l] = p, p += 9 * (int64_t)LV_CIN[l] * LV_COUT[l];
        s.pb[l] = p, p += LV_COUT[l];
    }
    for (int t = 0; t < LP_L; ++t) {
        s.lin[t] = o, o += LV_COUT[LV_TAP[t]];
        s.plin[t] = p, p += LV_COUT[LV_TAP[t]];
    }
    s.total = o;
    return s;
}

// Wp[kk][co] with kk = (kh * 3 + kw) * cinp + ci  <-  W[co][ci][kh][kw] (torch order); the rows of channels cin .. cinp - 1 are zero
__global__ void lpips_vgg_pack_w_kernel(const float* __restrict__ w, float* __restrict__ wp, int cin, int cinp, int cout) {
    const int64_t n = 9 * (int64_t)cinp * cout;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int kk = (int)(i / cout), co = (int)(i % cout);
        const int tap = kk / cinp, ci = kk % cinp, kh = tap / 3, kw = tap % 3;
        wp[i] = ci < cin ? w[(((int64_t)co * cin + ci) * 3 + kh) * 3 + kw] : 0.f;
    }
}

// ---- prologue: [K,H,W,3] x 2 -> NHWC [2K][H][W][16], image 2k = a[k], 2k + 1 = b[k]; rescale and scaling layer applied ------------
// one thread per (pixel, float4 of channels); hw = H * W; total4 = 2 K hw * 4
__global__ void lpips_vgg_image_kernel(const float* __restrict__ img_a, const float* __restrict__ img_b,
                                       const float* __restrict__ rescale, float* __restrict__ out, int64_t total4, int hw) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total4) return;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if ((i & 3) == 0) {
        const int64_t pix = i >> 2, im = pix / hw, rem = pix - im * hw;
        const float* src = ((im & 1) ? img_b : img_a) + ((im >> 1) * hw + rem) * 3;
        float x[3] = {src[0], src[1], src[2]};
        if (rescale) {  // the stack's rescale to [-1, 1] (main.py:361-363), as r2l_flip applies it
            const float mn = rescale[2 * (im & 1)], sc = 2.f / (rescale[2 * (im & 1) + 1] - mn);
#pragma unroll
            for (int c = 0; c < 3; ++c) x[c] = sc * (x[c] - mn) - 1.f;
        }
        // the scaling layer: (x - shift) / scale
        v[0] = (x[0] + 0.030f) / 0.458f, v[1] = (x[1] + 0.088f) / 0.448f, v[2] = (x[2] + 0.188f) / 0.450f;
    }
    reinterpret_cast<f32x4*>(out)[i] = v;
}

// max-pool 2 / 2 (no padding, floor: ho = hi / 2, every tap is inside) of NHWC maps; c4: float4 per position
__global__ void lpips_vgg_pool_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t total4, int hi, int wi, int ho,
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
    const f32x4 u00 = src[0], u01 = src[c4], u10 = src[(int64_t)wi * c4], u11 = src[((int64_t)wi + 1) * c4];
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = fmaxf(fmaxf(u00[j], u01[j]), fmaxf(u10[j], u11[j]));
    reinterpret_cast<f32x4*>(out)[i] = v;
}

}  // namespace

extern "C" {

int64_t r2l_lpips_vgg_param_floats(void) { return LV_PARAM_FLOATS; }

int64_t r2l_lpips_vgg_pack_floats(void) { return lv_stream().total; }

int r2l_lpips_vgg_pack(const float* params_dev, float* wpack_dev, void* stream) {
    R2L_REQUIRE(params_dev, "r2l_lpips_vgg_pack: params_dev is NULL");
    R2L_REQUIRE(wpack_dev, "r2l_lpips_vgg_pack: wpack_dev is NULL");
    R2L_REQUIRE(((uintptr_t)wpack_dev & 15) == 0, "r2l_lpips_vgg_pack: wpack_dev must be 16-byte aligned");
    const LvStream s = lv_stream();
    hipStream_t st = (hipStream_t)stream;
    for (int l = 0; l < LV_N; ++l) {
        const int64_t n = (int64_t)lv_kpad(l) * LV_COUT[l];
        hipLaunchKernelGGL(lpips_vgg_pack_w_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, params_dev + s.pw[l],
                           wpack_dev + s.w[l], LV_CIN[l], lv_cinp(l), LV_COUT[l]);
        R2L_CHECK(hipGetLastError());
        hipLaunchKernelGGL(lpips_copy_kernel, dim3((LV_COUT[l] + 255) / 256), dim3(256), 0, st, params_dev + s.pb[l],
                           wpack_dev + s.b[l], LV_COUT[l]);
        R2L_CHECK(hipGetLastError());
    }
    for (int t = 0; t < LP_L; ++t) {
        const int c = LV_COUT[LV_TAP[t]];
        hipLaunchKernelGGL(lpips_copy_kernel, dim3((c + 255) / 256), dim3(256), 0, st, params_dev + s.plin[t], wpack_dev + s.lin[t], c);
        R2L_CHECK(hipGetLastError());
    }
    return 0;
}

int64_t r2l_lpips_vgg_work_floats(int K, int H, int W) {
    LvPlan P;
    return lv_plan(K, H, W, &P) ? P.total : -1;
}

int64_t r2l_lpips_vgg_map_floats(int H, int W) {
    LvPlan P;
    return lv_plan(1, H, W, &P) ? P.map_floats : -1;
}

int r2l_lpips_vgg(const float* img_a, const float* img_b, int K, int H, int W, const float* rescale_dev, const float* wpack,
                  float* work, float* per_layer, float* maps, float* out, void* stream) {
    R2L_REQUIRE(K >= 1, "r2l_lpips_vgg: K must be at least 1");
    R2L_REQUIRE(H >= LV_MIN_HW && W >= LV_MIN_HW, "r2l_lpips_vgg: H and W must be at least 16 (the deepest feature map would be empty)");
    R2L_REQUIRE(H <= 16384 && W <= 16384, "r2l_lpips_vgg: H and W must be at most 16384");
    R2L_REQUIRE(img_a, "r2l_lpips_vgg: img_a is NULL");
    R2L_REQUIRE(img_b, "r2l_lpips_vgg: img_b is NULL");
    R2L_REQUIRE(wpack, "r2l_lpips_vgg: wpack is NULL");
    R2L_REQUIRE(work, "r2l_lpips_vgg: work is NULL");
    R2L_REQUIRE(out, "r2l_lpips_vgg: out is NULL");
    R2L_REQUIRE((((uintptr_t)wpack | (uintptr_t)work) & 15) == 0, "r2l_lpips_vgg: wpack and work must be 16-byte aligned");
    LvPlan P;
    R2L_REQUIRE(K <= 65535 && lv_plan(K, H, W, &P), "r2l_lpips_vgg: K exceeds one launch (65535 pairs, 2^31 rows of layer 0)");
    const LvStream S = lv_stream();
    hipStream_t st = (hipStream_t)stream;
    {
        const int64_t total4 = 2 * (int64_t)K * H * W * (LV_C0 / 4);
        hipLaunchKernelGGL(lpips_vgg_image_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, img_a, img_b, rescale_dev,
                           work + P.reg_off[1], total4, H * W);
        R2L_CHECK(hipGetLastError());
    }
    for (int l = 0; l < LV_N; ++l) {
        const int s = LV_STAGE[l], h = P.h[s], w = P.w[s];
        const int64_t M = 2 * (int64_t)K * h * w;
        float* dst = work + P.reg_off[LV_OUT[l]];
        LpConv c;
        c.in = work + P.reg_off[LV_IN[l]];
        c.img_a = c.img_b = c.rescale = nullptr;
        c.wp = wpack + S.w[l], c.bias = wpack + S.b[l];
        c.split = lv_split(l);
        c.out = c.split > 1 ? work + P.slab_off : dst;
        c.hi = c.ho = h, c.wi = c.wo = w;
        c.cin = lv_cinp(l), c.n = LV_COUT[l], c.ks = 3, c.pad = 1;
        c.M = (int)M, c.nslab = lv_kpad(l) / LP_BK;
        c.per_split = c.nslab / c.split;
        const int rc = lv_bn(l) == 64 ? lp_launch_conv<64, false>(c, st) : lp_launch_conv<128, false>(c, st);
        if (rc) return rc;
        if (c.split > 1) {
            const int64_t mn4 = M * LV_COUT[l] / 4;
            hipLaunchKernelGGL(lpips_slab_reduce_kernel, dim3((unsigned)((mn4 + 255) / 256)), dim3(256), 0, st, work + P.slab_off,
                               c.split, mn4, LV_COUT[l] / 4, c.bias, dst);
            R2L_CHECK(hipGetLastError());
        }
        if (l != LV_TAP[s]) continue;
        // the tap exists: its distance now, then the pool recycles R0
        hipLaunchKernelGGL(lpips_dist_kernel, dim3((unsigned)P.nb[s], (unsigned)K), dim3(256), 0, st, dst, wpack + S.lin[s], h * w,
                           LV_COUT[l] / 4, maps ? maps + P.map_off[s] : nullptr, P.map_floats, work + P.part_off + P.nb_off[s],
                           P.nb_total);
        R2L_CHECK(hipGetLastError());
        if (s + 1 < LP_L) {
            const int64_t total4 = 2 * (int64_t)K * P.h[s + 1] * P.w[s + 1] * (LV_COUT[l] / 4);
            hipLaunchKernelGGL(lpips_vgg_pool_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, dst, work + P.reg_off[0],
                               total4, h, w, P.h[s + 1], P.w[s + 1], LV_COUT[l] / 4);
            R2L_CHECK(hipGetLastError());
        }
    }
    LpFinish fin;
    for (int s = 0; s < LP_L; ++s) fin.nb[s] = P.nb[s], fin.nb_off[s] = P.nb_off[s], fin.count[s] = (float)(P.h[s] * P.w[s]);
    fin.nb_total = P.nb_total;
    hipLaunchKernelGGL(lpips_finish_kernel, dim3((unsigned)K), dim3(256), 0, st, work + P.part_off, fin, per_layer, out);
    R2L_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
