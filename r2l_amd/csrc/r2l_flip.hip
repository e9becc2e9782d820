// r2l_flip.hip — the FLIP difference map (Andersson et al., HPG 2020) of rendered frames against their targets, one fused kernel.
//
// Test-set evaluation (main.py:356-393) calls utils/flip_loss.py:70-130 on the whole stack: per image pair about 60 torch
// launches (colour transforms as view/matmul, four padded copies, 14 conv2d's with 21x21 and 19x19 windows at the standard
// 67 pixels per degree).  Here: one launch for K pairs.  A 32x8-pixel tile and its 10-pixel halo of both images are converted
// to YCxCz on load (sRGB -> linear -> XYZ / white, replicate padding by clamped coordinates, the reference's [-1,1] stack
// rescale folded in) and sit in LDS; every thread runs the spatial CSF filters (A, RG, BY) and the edge / point detectors
// of its pixel from there, then the colour pipeline (linear RGB clamp, L*a*b*, Hunt, HyAB, redistribution) and the feature
// pipeline in registers; the block reduces the map value and a second small kernel sums the per-block partials of every
// frame in a fixed order (no float atomics: the means are bit-reproducible).
//
// Every 2-D window of the reference is a sum of separable terms, so the taps are 1-D tables built on the host in double:
//   A, RG: g(x) g(y) ; BY: g1(x) g1(y) + g2(x) g2(y) ; edge: e(x) g(y) ; point: p(x) g(y)   (and transposed),
// each already carrying its share of the 2-D normaliser.  All tables live in one FL_WIN-wide frame centred at FL_R: a smaller
// radius (lower pixels per degree) is zero taps at the rim, which replicate padding makes exact.  The detectors' taps sum to
// zero, so they are applied to Y minus the centre pixel's Y: the same value, but flat regions give exactly 0 instead of the
// cancellation residue that (.)^0.5 would amplify (the reference's own fp32 run is 1e-4 off its fp64 run there).
// A wave covers two 32-pixel rows, so the 32-lane halves of a ds_read_b32 touch 32 consecutive dwords: no bank conflicts.
#include "r2l_common.h"

#include <math.h>

namespace {

constexpr int FL_R = 10, FL_WIN = 2 * FL_R + 1, FL_RF = 9;  // compiled-in maxima: CSF radius, its window, detector radius
constexpr int FL_TX = 32, FL_TY = 8, FL_THREADS = FL_TX * FL_TY;
constexpr int FL_HX = FL_TX + 2 * FL_R, FL_HY = FL_TY + 2 * FL_R;  // 52 x 28

struct FlipParams {
    float ga[FL_WIN], grg[FL_WIN], gb1[FL_WIN], gb2[FL_WIN];  // CSF: achromatic, red-green, blue-yellow (two Gaussians)
    float fg[FL_WIN], fe[FL_WIN], fp[FL_WIN];                 // detectors: Gaussian, edge, point (zero beyond their radius)
    float to_opp[9];    // linear RGB -> XYZ / white point (rows x, y, z)
    float to_rgb[9];    // XYZ / white point -> linear RGB
    float cmax, pccmax;
};

__device__ __forceinline__ float srgb_to_linear(float v) {
    v = fminf(fmaxf(v, 0.f), 1.f);
    return v > 0.04045f ? powf((v + 0.055f) / 1.055f, 2.4f) : v / 12.92f;
}

__device__ __forceinline__ float lab_f(float t) {
    return t > 0.00885f ? cbrtf(t) : t / (3.f * (6.f / 29.f) * (6.f / 29.f)) + 4.f / 29.f;
}

// filtered YCxCz -> Hunt-adjusted L*a*b* (flip_loss.py:216-221 clamp included)
__device__ __forceinline__ void opponent_to_hunt_lab(const FlipParams& P, float Y, float cx, float cz, float& L, float& a, float& b) {
    const float y = (Y + 16.f) / 116.f, x = y + cx / 500.f, z = y - cz / 200.f;
    float rgb[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = fmaf(P.to_rgb[3 * c + 2], z, fmaf(P.to_rgb[3 * c + 1], y, P.to_rgb[3 * c] * x));
        rgb[c] = fminf(fmaxf(v, 0.f), 1.f);
    }
    float f[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
        f[c] = lab_f(fmaf(P.to_opp[3 * c + 2], rgb[2], fmaf(P.to_opp[3 * c + 1], rgb[1], P.to_opp[3 * c] * rgb[0])));
    L = 116.f * f[1] - 16.f;
    const float h = 0.01f * L;
    a = h * (500.f * (f[0] - f[1]));
    b = h * (200.f * (f[1] - f[2]));
}

__global__ __launch_bounds__(FL_THREADS) void r2l_flip_kernel(const float* __restrict__ img_a, const float* __restrict__ img_b,
                                                              int H, int W, FlipParams P, const float* __restrict__ rescale,
                                                              float* __restrict__ partial, float* __restrict__ map) {
    __shared__ float s[6][FL_HY][FL_HX];  // Y, Cx, Cz of image a, then of image b
    __shared__ float red[FL_THREADS / 64];
    const int tx = threadIdx.x % FL_TX, ty = threadIdx.x / FL_TX;
    const int x0 = blockIdx.x * FL_TX, y0 = blockIdx.y * FL_TY;
    const int64_t frame = (int64_t)blockIdx.z * H * W;
    float sc[2] = {1.f, 1.f}, mn[2] = {0.f, 0.f};
    if (rescale) {  // the stack's rescale to [-1, 1] (main.py:361-363): 2 / (max - min) * (x - min) - 1
        mn[0] = rescale[0], sc[0] = 2.f / (rescale[1] - rescale[0]);
        mn[1] = rescale[2], sc[1] = 2.f / (rescale[3] - rescale[2]);
    }
    for (int i = threadIdx.x; i < FL_HY * FL_HX; i += FL_THREADS) {
        const int hy = i / FL_HX, hx = i % FL_HX;
        const int y = min(max(y0 + hy - FL_R, 0), H - 1), x = min(max(x0 + hx - FL_R, 0), W - 1);  // replicate padding
        const int64_t off = (frame + (int64_t)y * W + x) * 3;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const float* p = (m ? img_b : img_a) + off;
            float c[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float v = p[k];
                if (rescale) v = sc[m] * (v - mn[m]) - 1.f;
                c[k] = srgb_to_linear(v);
            }
            float o[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) o[k] = fmaf(P.to_opp[3 * k + 2], c[2], fmaf(P.to_opp[3 * k + 1], c[1], P.to_opp[3 * k] * c[0]));
            s[3 * m + 0][hy][hx] = 116.f * o[1] - 16.f;
            s[3 * m + 1][hy][hx] = 500.f * (o[0] - o[1]);
            s[3 * m + 2][hy][hx] = 200.f * (o[1] - o[2]);
        }
    }
    __syncthreads();
    const float yc[2] = {s[0][ty + FL_R][tx + FL_R], s[3][ty + FL_R][tx + FL_R]};
    float fa[2] = {0.f, 0.f}, frg[2] = {0.f, 0.f}, fby[2] = {0.f, 0.f};
    float ex[2] = {0.f, 0.f}, ey[2] = {0.f, 0.f}, px[2] = {0.f, 0.f}, py[2] = {0.f, 0.f};
#pragma unroll 1
    for (int i = 0; i < FL_WIN; ++i) {
        float ra[2] = {0.f, 0.f}, rrg[2] = {0.f, 0.f}, rb1[2] = {0.f, 0.f}, rb2[2] = {0.f, 0.f};
        float rg[2] = {0.f, 0.f}, re[2] = {0.f, 0.f}, rp[2] = {0.f, 0.f};
#pragma unroll
        for (int j = 0; j < FL_WIN; ++j) {
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const float Y = s[3 * m][ty + i][tx + j], cx = s[3 * m + 1][ty + i][tx + j], cz = s[3 * m + 2][ty + i][tx + j];
                const float d = Y - yc[m];
                ra[m] = fmaf(P.ga[j], Y, ra[m]);
                rrg[m] = fmaf(P.grg[j], cx, rrg[m]);
                rb1[m] = fmaf(P.gb1[j], cz, rb1[m]);
                rb2[m] = fmaf(P.gb2[j], cz, rb2[m]);
                rg[m] = fmaf(P.fg[j], d, rg[m]);
                re[m] = fmaf(P.fe[j], d, re[m]);
                rp[m] = fmaf(P.fp[j], d, rp[m]);
            }
        }
        const float wa = P.ga[i], wrg = P.grg[i], wb1 = P.gb1[i], wb2 = P.gb2[i], wg = P.fg[i], we = P.fe[i], wp = P.fp[i];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            fa[m] = fmaf(wa, ra[m], fa[m]);
            frg[m] = fmaf(wrg, rrg[m], frg[m]);
            fby[m] = fmaf(wb2, rb2[m], fmaf(wb1, rb1[m], fby[m]));
            ex[m] = fmaf(wg, re[m], ex[m]);  // edge taps along x, Gaussian along y
            ey[m] = fmaf(we, rg[m], ey[m]);  // transposed
            px[m] = fmaf(wg, rp[m], px[m]);
            py[m] = fmaf(wp, rg[m], py[m]);
        }
    }
    // colour pipeline
    float L[2], A[2], B[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) opponent_to_hunt_lab(P, fa[m], frg[m], fby[m], L[m], A[m], B[m]);
    const float da = A[0] - A[1], db = B[0] - B[1];
    const float hyab = fabsf(L[0] - L[1]) + sqrtf(da * da + db * db);
    const float pw = powf(hyab, 0.7f);
    const float dec = pw < P.pccmax ? (0.95f / P.pccmax) * pw : 0.95f + ((pw - P.pccmax) / (P.cmax - P.pccmax)) * 0.05f;
    // feature pipeline: the detectors ran on Y - Y_centre; (Y + 16) / 116 of flip_loss.py:108-109 is the factor 1 / 116
    const float de = fabsf(sqrtf(ex[0] * ex[0] + ey[0] * ey[0]) - sqrtf(ex[1] * ex[1] + ey[1] * ey[1]));
    const float dp = fabsf(sqrtf(px[0] * px[0] + py[0] * py[0]) - sqrtf(px[1] * px[1] + py[1] * py[1]));
    const float def = fminf(sqrtf(fmaxf(de, dp) * (0.70710678118654752f / 116.f)), 1.f);
    float v = powf(dec, 1.f - def);
    const int y = y0 + ty, x = x0 + tx;
    if (y < H && x < W) {
        if (map) map[frame + (int64_t)y * W + x] = v;
    } else {
        v = 0.f;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        partial[((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// out[k] = mean of frame k: its n partials summed in a fixed order
__global__ __launch_bounds__(256) void r2l_flip_finish_kernel(const float* __restrict__ partial, int64_t n, float inv_count,
                                                              float* __restrict__ out) {
    __shared__ float red[4];
    const float* p = partial + (int64_t)blockIdx.x * n;
    float v = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += 256) v += p[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = ((red[0] + red[1]) + (red[2] + red[3])) * inv_count;
}

// ---- host: the constants of flip_loss.py:137-181,259-288,324-333 in double ------------------------------------------------
void lab_hunt(const double A[9], const double white[3], const double rgb[3], double out[3]) {
    double f[3];
    for (int c = 0; c < 3; ++c) {
        const double t = (A[3 * c] * rgb[0] + A[3 * c + 1] * rgb[1] + A[3 * c + 2] * rgb[2]) / white[c];
        f[c] = t > 0.00885 ? pow(t, 1.0 / 3.0) : t / (3.0 * (6.0 / 29.0) * (6.0 / 29.0)) + 4.0 / 29.0;
    }
    out[0] = 116.0 * f[1] - 16.0;
    out[1] = 0.01 * out[0] * 500.0 * (f[0] - f[1]);
    out[2] = 0.01 * out[0] * 200.0 * (f[1] - f[2]);
}

// false: pixels_per_degree is outside what the kernel is compiled for
bool flip_params(double ppd, FlipParams* P) {
    const double PI = 3.14159265358979323846;
    if (!(ppd > 0.0) || !(ppd < 1e6)) return false;
    const int r = (int)ceil(3.0 * sqrt(0.04 / (2.0 * PI * PI)) * ppd);
    const double sd = 0.5 * 0.082 * ppd;
    const int rf = (int)ceil(3.0 * sd);
    if (r < 0 || r > FL_R || rf < 0 || rf > FL_RF) return false;
    // spatial CSFs: a * sqrt(pi / b) * exp(-pi^2 z / b) with z = (x^2 + y^2) / ppd^2, normalised by the 2-D sum
    const double b_a = 0.0047, b_rg = 0.0053, a1_by = 34.1, b1_by = 0.04, a2_by = 13.5, b2_by = 0.025;
    double g[4][FL_WIN], sum[4] = {0, 0, 0, 0};
    const double bs[4] = {b_a, b_rg, b1_by, b2_by};
    for (int t = 0; t < 4; ++t)
        for (int j = 0; j < FL_WIN; ++j) {
            const int x = j - FL_R;
            g[t][j] = abs(x) <= r ? exp(-PI * PI * (x / ppd) * (x / ppd) / bs[t]) : 0.0;
            sum[t] += g[t][j];
        }
    const double c1 = a1_by * sqrt(PI / b1_by), c2 = a2_by * sqrt(PI / b2_by);
    const double s_by = c1 * sum[2] * sum[2] + c2 * sum[3] * sum[3];
    for (int j = 0; j < FL_WIN; ++j) {
        P->ga[j] = (float)(g[0][j] / sum[0]);
        P->grg[j] = (float)(g[1][j] / sum[1]);
        P->gb1[j] = (float)(g[2][j] * sqrt(c1 / s_by));
        P->gb2[j] = (float)(g[3][j] * sqrt(c2 / s_by));
    }
    // detectors: positive taps of the 2-D window sum to +1, negative ones to -1; the sign depends on x alone
    double fg[FL_WIN], fe[FL_WIN], fp[FL_WIN], sg = 0, se = 0, spp = 0, spn = 0;
    for (int j = 0; j < FL_WIN; ++j) {
        const int x = j - FL_R;
        const bool in = abs(x) <= rf;
        fg[j] = in ? exp(-(double)(x * x) / (2.0 * sd * sd)) : 0.0;
        fe[j] = -x * fg[j];
        fp[j] = ((double)(x * x) / (sd * sd) - 1.0) * fg[j];
        sg += fg[j];
        if (fe[j] > 0) se += fe[j];
        if (fp[j] > 0) spp += fp[j];
        if (fp[j] < 0) spn -= fp[j];
    }
    for (int j = 0; j < FL_WIN; ++j) {
        P->fg[j] = (float)(fg[j] / sg);
        P->fe[j] = (float)(se > 0 ? fe[j] / se : 0.0);
        P->fp[j] = (float)(fp[j] > 0 ? fp[j] / spp : (spn > 0 ? fp[j] / spn : 0.0));
    }
    // linear RGB <-> XYZ (D65) with the white point A * (1,1,1) folded in
    const double A[9] = {10135552.0 / 24577794.0, 8788810.0 / 24577794.0, 4435075.0 / 24577794.0,
                         2613072.0 / 12288897.0,  8788810.0 / 12288897.0, 887015.0 / 12288897.0,
                         1425312.0 / 73733382.0,  8788810.0 / 73733382.0, 70074185.0 / 73733382.0};
    double white[3], M[9], inv[9];
    for (int c = 0; c < 3; ++c) {
        white[c] = A[3 * c] + A[3 * c + 1] + A[3 * c + 2];
        for (int k = 0; k < 3; ++k) M[3 * c + k] = A[3 * c + k] / white[c];
    }
    const double det = M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
    inv[0] = (M[4] * M[8] - M[5] * M[7]) / det, inv[1] = (M[2] * M[7] - M[1] * M[8]) / det, inv[2] = (M[1] * M[5] - M[2] * M[4]) / det;
    inv[3] = (M[5] * M[6] - M[3] * M[8]) / det, inv[4] = (M[0] * M[8] - M[2] * M[6]) / det, inv[5] = (M[2] * M[3] - M[0] * M[5]) / det;
    inv[6] = (M[3] * M[7] - M[4] * M[6]) / det, inv[7] = (M[1] * M[6] - M[0] * M[7]) / det, inv[8] = (M[0] * M[4] - M[1] * M[3]) / det;
    for (int k = 0; k < 9; ++k) P->to_opp[k] = (float)M[k], P->to_rgb[k] = (float)inv[k];
    // cmax = HyAB(Hunt(Lab(green)), Hunt(Lab(blue)))^0.7
    const double green[3] = {0, 1, 0}, blue[3] = {0, 0, 1};
    double lg[3], lb[3];
    lab_hunt(A, white, green, lg);
    lab_hunt(A, white, blue, lb);
    const double cmax = pow(fabs(lg[0] - lb[0]) + sqrt((lg[1] - lb[1]) * (lg[1] - lb[1]) + (lg[2] - lb[2]) * (lg[2] - lb[2])), 0.7);
    P->cmax = (float)cmax;
    P->pccmax = (float)(0.4 * cmax);
    return true;
}

}  // namespace

extern "C" {

int64_t r2l_flip_partial_count(int H, int W, int K) {
    return (int64_t)((H + FL_TY - 1) / FL_TY) * ((W + FL_TX - 1) / FL_TX) * K;
}

int r2l_flip(const float* img_a, const float* img_b, int K, int H, int W, float pixels_per_degree, const float* rescale_dev,
             float* partial, float* map, float* out, void* stream) {
    R2L_REQUIRE(K > 0 && H > 0 && W > 0, "r2l_flip: K, H and W must be positive");
    R2L_REQUIRE(K <= 65535 && (H + FL_TY - 1) / FL_TY <= 65535, "r2l_flip: K or H exceeds the launch grid (65535 frames, 524280 rows)");
    R2L_REQUIRE(img_a && img_b && partial && out, "r2l_flip: a required pointer is NULL");
    FlipParams P;
    R2L_REQUIRE(flip_params((double)pixels_per_degree, &P),
                "r2l_flip: pixels_per_degree out of range (0, 73.1]: its filter radii exceed the compiled 10 (CSF) / 9 (detectors)");
    dim3 grid((W + FL_TX - 1) / FL_TX, (H + FL_TY - 1) / FL_TY, K);
    hipLaunchKernelGGL(r2l_flip_kernel, grid, dim3(FL_THREADS), 0, (hipStream_t)stream, img_a, img_b, H, W, P, rescale_dev, partial,
                       map);
    R2L_CHECK(hipGetLastError());
    hipLaunchKernelGGL(r2l_flip_finish_kernel, dim3(K), dim3(256), 0, (hipStream_t)stream, partial, (int64_t)grid.x * grid.y,
                       1.f / ((float)H * (float)W), out);
    R2L_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
