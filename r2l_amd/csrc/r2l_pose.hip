// r2l_pose.hip — camera-pose refinement against a trained student (include/r2l_hip.h "pose refinement").
//   r2l_pose_key        : the key of pose p's pixel bijection at an iteration; host integer arithmetic
//   r2l_pose_batch      : the rays of P observed images under P current pose estimates in one launch: n distinct pixels per pose,
//                         the whole frame as window, through pixel_ray (csrc/r2l_pixel_ray.h) — the rows r2l_image_batch writes
//   r2l_pose_grad       : the segmented reduction from ray gradients to pose gradients, [N,3] x 5 -> grad [P,6], loss [P]
//   r2l_pose_update     : Adam on the 6-vector and the retraction R <- exp([w]x) R, t <- t + v, one pose per thread
//   r2l_pose_refine_step: one iteration for all P poses — batch -> [pack] -> forward with stash -> dX chain -> input gradient ->
//                         pose gradient -> update: the EXISTING kernels with their existing arguments and the three above, enqueued
//                         back to back on the caller's stream through one work buffer: no allocation, no synchronisation, no state.
//
// r2l_pose_grad.  Seven sums per pose: d x dd (3), d_o (3), |rgb - target|^2 (1).  Pose p's n rays are cut into K = ceil(n / 256)
// chunks of 256; one wave (a 64-thread workgroup) takes one chunk, a lane four of its rays:
//   vector path (n % 4 == 0 and all five inputs 16-byte aligned: every chunk then starts on a 16-byte boundary): lane l takes rays
//       4 l .. 4 l + 3 of the chunk as three 16-byte loads per input; scalar path: rays l, l + 64, l + 128, l + 192.
//   lane: (t0 + t1) + (t2 + t3), absent rays contribute 0;  wave: six xor-shuffle levels (32, 16, 8, 4, 2, 1).
//   K == 1: lane 0 writes grad / loss.  K > 1: lane 0 writes eight floats (seven sums, one 0) of a partial, and a reduce kernel —
//   one wave per 64 partials of a pose, the same six levels — runs ceil(log64 K) times, ping-pong in `work`, the last one writing
//   grad / loss.  The path, the chunking and the order depend on (P, n) and the alignment alone: two calls give the same bits.
// Additions on the longest path of a term: 1 (the cross product's own subtraction, or the two of a pixel's squared error) + 2 + 6
// + 6 per reduce level: 9 for n <= 256, 15 up to 16 384, 21 up to 2^20, 33 for any n < 2^31.
// Every grid is a count of chunks or of partial groups, P * ceil(.. n ..): one pose of 2^20 rays is 4096 waves, then 64, then 1.
#include "r2l_dispatch.h"
#include "r2l_perm.h"
#include "r2l_pixel_ray.h"
#include "r2l_hip.h"
#include <math.h>

#define R2L_POSE_SALT 0x706F73655F726566ull  // "pose_ref": r2l_pose_key (pinned in include/r2l_hip.h)
#define PG_CHUNK 256                         // rays of a wave of r2l_pose_grad
#define PG_FAN 64                            // partials of a wave of its reduce kernel
#define POSE_SERIES_THETA2 1e-4f             // Rodrigues' coefficients by their series below this squared angle (theta < 0.01)

namespace {

// Row p n + j: pixel pi(key_p, H W)(j) of image p, its world ray under c2w[p] (pixel_ray: the one definition), its colour, its id.
__global__ void r2l_pose_batch_kernel(const float* __restrict__ images, const float* __restrict__ c2w, int H, int W, float focal,
                                      unsigned long long z, int half_bits, int64_t n, int64_t N, float* __restrict__ rays_o,
                                      float* __restrict__ rays_d, float* __restrict__ target, int64_t* __restrict__ ids_out) {
    const int64_t hw = (int64_t)H * W;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < N; r += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = r / n, j = r - p * n;
        unsigned k[4];
        perm_round_keys(perm_epoch_key(z, (unsigned long long)p), k);
        const int64_t q = (int64_t)perm_at((unsigned long long)j, (unsigned long long)hw, half_bits, k);
        const int row = (int)(q / W), col = (int)(q - (int64_t)row * W);
        const int64_t g = (p * H + row) * W + col;
        float o[3], d[3];
        pixel_ray(c2w + p * 12, focal, H, W, row, col, o, d);
        const float* __restrict__ px = images + g * 3;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            rays_o[r * 3 + i] = o[i];
            rays_d[r * 3 + i] = d[i];
            target[r * 3 + i] = px[i];
        }
        if (ids_out != nullptr) ids_out[r] = g;
    }
}

// The seven terms of one ray.
__device__ __forceinline__ void pg_terms(const float (&d)[3], const float (&go)[3], const float (&gd)[3], const float (&c)[3],
                                         const float (&t)[3], float (&s)[7]) {
    s[0] = d[1] * gd[2] - d[2] * gd[1];
    s[1] = d[2] * gd[0] - d[0] * gd[2];
    s[2] = d[0] * gd[1] - d[1] * gd[0];
    s[3] = go[0]; s[4] = go[1]; s[5] = go[2];
    const float e0 = c[0] - t[0], e1 = c[1] - t[1], e2 = c[2] - t[2];
    s[6] = (e0 * e0 + e1 * e1) + e2 * e2;
}

__device__ __forceinline__ void pg_wave_sum(float (&s)[7]) {
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1)
#pragma unroll
        for (int i = 0; i < 7; ++i) s[i] += __shfl_xor(s[i], w);
}

// What lane 0 of a wave leaves: the outputs themselves (last), else partial `at` of eight floats.
__device__ __forceinline__ void pg_write(const float (&s)[7], bool last, int64_t p, int64_t at, float den, float* __restrict__ part,
                                         float* __restrict__ grad, float* __restrict__ loss) {
    if (last) {
#pragma unroll
        for (int i = 0; i < 6; ++i) grad[p * 6 + i] = s[i];
        if (loss != nullptr) loss[p] = s[6] / den;
    } else {
        float4* __restrict__ o = reinterpret_cast<float4*>(part + at * 8);
        o[0] = make_float4(s[0], s[1], s[2], s[3]);
        o[1] = make_float4(s[4], s[5], s[6], 0.f);
    }
}

// Wave (p, k) = blockIdx.x: chunk k of pose p.  den = 3 n as a float (loss = sum / den).
template <bool VEC>
__global__ __launch_bounds__(64) void r2l_pose_grad_kernel(const float* __restrict__ rays_d, const float* __restrict__ d_o,
                                                           const float* __restrict__ d_d, const float* __restrict__ rgb,
                                                           const float* __restrict__ target, int64_t n, int64_t K, float den,
                                                           float* __restrict__ part, float* __restrict__ grad,
                                                           float* __restrict__ loss) {
    const int64_t p = (int64_t)blockIdx.x / K, k = (int64_t)blockIdx.x - p * K;
    const int lane = (int)threadIdx.x;
    const int64_t first = k * PG_CHUNK;          // of the pose's rays
    const int64_t base = p * n + first;          // of all rays
    const int64_t left = n - first;              // rays of this chunk and behind it (>= 1)
    float s4[4][7];
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int i = 0; i < 7; ++i) s4[x][i] = 0.f;
    if (VEC) {
        if ((int64_t)lane * 4 < left) {  // n % 4 == 0: a lane's four rays are all present or all absent
            const int64_t w = (base + lane * 4) * 3 / 4;  // 16-byte word: (p n + first + 4 l) * 3 floats is a multiple of 4
            float v[5][12];
            const float* in[5] = {rays_d, d_o, d_d, rgb, target};
#pragma unroll
            for (int a = 0; a < 5; ++a)
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const float4 x = reinterpret_cast<const float4*>(in[a])[w + q];
                    v[a][4 * q] = x.x; v[a][4 * q + 1] = x.y; v[a][4 * q + 2] = x.z; v[a][4 * q + 3] = x.w;
                }
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                float a[5][3];
#pragma unroll
                for (int y = 0; y < 5; ++y)
#pragma unroll
                    for (int i = 0; i < 3; ++i) a[y][i] = v[y][3 * x + i];
                pg_terms(a[0], a[1], a[2], a[3], a[4], s4[x]);
            }
        }
    } else {
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const int64_t j = lane + 64 * x;
            if (j < left) {
                const int64_t at = (base + j) * 3;
                float a[5][3];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    a[0][i] = rays_d[at + i]; a[1][i] = d_o[at + i]; a[2][i] = d_d[at + i]; a[3][i] = rgb[at + i]; a[4][i] = target[at + i];
                }
                pg_terms(a[0], a[1], a[2], a[3], a[4], s4[x]);
            }
        }
    }
    float s[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) s[i] = (s4[0][i] + s4[1][i]) + (s4[2][i] + s4[3][i]);
    pg_wave_sum(s);
    if (lane == 0) pg_write(s, K == 1, p, (int64_t)blockIdx.x, den, part, grad, loss);
}

// Wave (p, g) = blockIdx.x: partials 64 g .. 64 g + 63 of pose p's K_in -> partial g of its K_out = ceil(K_in / 64), or the outputs.
__global__ __launch_bounds__(64) void r2l_pose_grad_reduce_kernel(const float* __restrict__ in, int64_t K_in, int64_t K_out, float den,
                                                                  float* __restrict__ out, float* __restrict__ grad,
                                                                  float* __restrict__ loss) {
    const int64_t p = (int64_t)blockIdx.x / K_out, g = (int64_t)blockIdx.x - p * K_out;
    const int lane = (int)threadIdx.x;
    const int64_t k = g * PG_FAN + lane;
    float s[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) s[i] = 0.f;
    if (k < K_in) {
        const float4* __restrict__ q = reinterpret_cast<const float4*>(in + (p * K_in + k) * 8);
        const float4 a = q[0], b = q[1];
        s[0] = a.x; s[1] = a.y; s[2] = a.z; s[3] = a.w; s[4] = b.x; s[5] = b.y; s[6] = b.z;
    }
    pg_wave_sum(s);
    if (lane == 0) pg_write(s, K_out == 1, p, (int64_t)blockIdx.x, den, out, grad, loss);
}

__device__ __forceinline__ void cross3(const float (&a)[3], const float (&b)[3], float (&c)[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// One pose per thread.  Adam as r2l_adam_step evaluates it (csrc/r2l_train.hip r2l_adam_one), with a step size per half of the
// 6-vector; then R <- exp([dw]x) R by Rodrigues' formula with half-angle coefficients (no 1 - cos), one modified Gram-Schmidt pass
// over the columns 0, 1, 2, and t <- t + dv.  Not all six sums finite: nothing of the pose is touched.  dw == 0: R keeps its bits.
__global__ void r2l_pose_update_kernel(float* __restrict__ c2w, float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
                                       const float* __restrict__ grad, int P, float step_rot, float step_trans, float b1, float b2,
                                       float eps, float sqrt_bc2) {
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p >= P) return;
    float g[6];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        g[i] = grad[p * 6 + i];
        ok = ok && isfinite(g[i]);
    }
    if (!ok) return;
    float dl[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const float m = exp_avg[p * 6 + i], v = exp_avg_sq[p * 6 + i];
        const float mi = m + (g[i] - m) * (1.0f - b1);
        const float vi = v * b2 + (g[i] * g[i]) * (1.0f - b2);
        exp_avg[p * 6 + i] = mi;
        exp_avg_sq[p * 6 + i] = vi;
        const float denom = sqrtf(vi) / sqrt_bc2 + eps;
        dl[i] = -((i < 3 ? step_rot : step_trans) * (mi / denom));
    }
    float* __restrict__ c = c2w + p * 12;
    if (dl[0] != 0.f || dl[1] != 0.f || dl[2] != 0.f) {
        const float w[3] = {dl[0], dl[1], dl[2]};
        const float th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
        float A, B;  // sin(th) / th, (1 - cos(th)) / th^2
        if (th2 < POSE_SERIES_THETA2) {
            A = 1.0f - th2 * (1.0f / 6.0f - th2 * (1.0f / 120.0f));
            B = 0.5f - th2 * (1.0f / 24.0f - th2 * (1.0f / 720.0f));
        } else {
            const float th = sqrtf(th2);
            float sh, ch;
            sincosf(0.5f * th, &sh, &ch);
            A = (2.0f * sh) * ch / th;
            B = (2.0f * sh) * sh / th2;
        }
        float R[3][3];  // R[col][row]
#pragma unroll
        for (int col = 0; col < 3; ++col) {
            const float r[3] = {c[col], c[4 + col], c[8 + col]};
            float k1[3], k2[3];
            cross3(w, r, k1);
            cross3(w, k1, k2);
#pragma unroll
            for (int i = 0; i < 3; ++i) R[col][i] = (r[i] + A * k1[i]) + B * k2[i];
        }
#pragma unroll
        for (int col = 0; col < 3; ++col) {
#pragma unroll
            for (int q = 0; q < col; ++q) {
                const float dot = (R[q][0] * R[col][0] + R[q][1] * R[col][1]) + R[q][2] * R[col][2];
#pragma unroll
                for (int i = 0; i < 3; ++i) R[col][i] = R[col][i] - dot * R[q][i];
            }
            const float nrm = sqrtf((R[col][0] * R[col][0] + R[col][1] * R[col][1]) + R[col][2] * R[col][2]);
#pragma unroll
            for (int i = 0; i < 3; ++i) R[col][i] = R[col][i] / nrm;
        }
#pragma unroll
        for (int col = 0; col < 3; ++col)
#pragma unroll
            for (int i = 0; i < 3; ++i) c[i * 4 + col] = R[col][i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) c[i * 4 + 3] = c[i * 4 + 3] + dl[3 + i];
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
constexpr int64_t MAX_RAYS = ((int64_t)1 << 31) - 1;
int64_t pg_chunks(int64_t n) { return (n + PG_CHUNK - 1) / PG_CHUNK; }
int64_t pg_groups(int64_t K) { return (K + PG_FAN - 1) / PG_FAN; }
int64_t round1k(int64_t n) { return (n + 1023) & ~(int64_t)1023; }

// ---- the descriptor ------------------------------------------------------------------------------------------------------------
const char* pose_desc_check(const r2l_pose_refine_step_desc* d) {
    if (d == nullptr) return "r2l_pose_refine_step_desc: desc is NULL";
    if (d->n_block < 0 || d->n_block > R2L_MAX_BLOCKS) return "r2l_pose_refine_step_desc.n_block: need 0 <= n_block <= 1024";
    if (const char* why = r2l_cfg_check(d->cfg)) return why;
    if (d->P < 1) return "r2l_pose_refine_step_desc.P: need P >= 1";
    if (d->n < 1) return "r2l_pose_refine_step_desc.n: need n >= 1";
    if (d->H < 1 || d->W < 1) return "r2l_pose_refine_step_desc.H: need H >= 1 and W >= 1";
    if ((int64_t)d->P * d->H > MAX_RAYS || (int64_t)d->P * d->H * d->W > MAX_RAYS)
        return "r2l_pose_refine_step_desc.P: need P * H * W < 2^31 pixels";
    if (d->n > (int64_t)d->H * d->W) return "r2l_pose_refine_step_desc.n: exceeds the H * W pixels of a frame";
    if (d->n > MAX_RAYS / d->P) return "r2l_pose_refine_step_desc.n: P * n must stay below 2^31 rays";
    if (!(d->focal > 0.f)) return "r2l_pose_refine_step_desc.focal: need focal > 0";
    if (d->iteration < 1 || d->iteration >= ((int64_t)1 << 60))
        return "r2l_pose_refine_step_desc.iteration: need 1 <= iteration < 2^60 (iterations count from 1)";
    if (d->pack != 0 && d->pack != 1) return "r2l_pose_refine_step_desc.pack: 0 or 1";
    if (d->reserved[0] || d->reserved[1] || d->reserved[2] || d->reserved[3]) return "r2l_pose_refine_step_desc.reserved: must be 0";
    return nullptr;
}

// The work buffer: every part starts on a 4 KiB boundary of it.
struct PoseWork {
    int64_t o, d, t, rgb, save_x, save_t, gx, gt, dpre, sqerr, d_o, d_d, grad, pg, total;
};
PoseWork pose_work(const r2l_pose_refine_step_desc* d) {
    const int64_t N = (int64_t)d->P * d->n;
    const int64_t slot = r2l_stash_slot_floats(N), nb = d->n_block;
    PoseWork w{};
    int64_t at = 0;
    auto take = [&](int64_t n) { const int64_t a = at; at += round1k(n); return a; };
    w.o = take(N * 3); w.d = take(N * 3); w.t = take(N * 3); w.rgb = take(N * 3);
    w.save_x = take((nb + 1) * slot);
    w.save_t = take((nb > 0 ? nb : 1) * slot);
    w.gx = take((nb + 1) * slot);
    w.gt = take((nb > 0 ? nb : 1) * slot);
    w.dpre = take(N * 3);
    w.sqerr = take(r2l_num_tiles(N));
    w.d_o = take(N * 3); w.d_d = take(N * 3);
    w.grad = take((int64_t)d->P * 6);
    w.pg = take(r2l_pose_grad_work_floats(d->P, d->n));
    w.total = at;
    return w;
}

}  // namespace

extern "C" int r2l_pose_key(uint64_t seed, int64_t iteration, int64_t p, uint64_t* key_out) {
    R2L_REQUIRE(iteration >= 1, "r2l_pose_key: need iteration >= 1");
    R2L_REQUIRE(p >= 0, "r2l_pose_key: p is negative");
    R2L_REQUIRE(key_out != nullptr, "r2l_pose_key: key_out is NULL");
    const unsigned long long z = perm_epoch_key(seed ^ R2L_POSE_SALT, (unsigned long long)iteration);
    *key_out = perm_epoch_key(z, (unsigned long long)p);
    return 0;
}

extern "C" int r2l_pose_batch(const float* images, const float* c2w, int P, int H, int W, float focal, uint64_t seed, int64_t iteration,
                              int64_t n, float* rays_o, float* rays_d, float* target, int64_t* ids_out, void* stream) {
    R2L_REQUIRE(P >= 0 && H >= 1 && W >= 1, "r2l_pose_batch: need P >= 0, H >= 1 and W >= 1");
    R2L_REQUIRE(focal > 0.f, "r2l_pose_batch: need focal > 0");
    R2L_REQUIRE(iteration >= 1, "r2l_pose_batch: need iteration >= 1");
    R2L_REQUIRE(n >= 0, "r2l_pose_batch: n is negative");
    const int64_t ph = (int64_t)P * H;  // < 2^62; checked before it is multiplied again
    R2L_REQUIRE(ph <= MAX_RAYS && ph * W <= MAX_RAYS, "r2l_pose_batch: need P * H * W < 2^31 pixels");
    const int64_t hw = (int64_t)H * W;
    R2L_REQUIRE(n <= hw, "r2l_pose_batch: n exceeds the H * W pixels of a frame");
    if (n == 0 || P == 0) return 0;
    R2L_REQUIRE(images && c2w && rays_o && rays_d && target,
                "r2l_pose_batch: a required pointer is NULL (images, c2w, rays_o, rays_d, target)");
    const int64_t N = (int64_t)P * n;  // <= P * H * W < 2^31
    const unsigned long long z = perm_epoch_key(seed ^ R2L_POSE_SALT, (unsigned long long)iteration);
    const int64_t blocks = (N + 255) / 256;
    hipLaunchKernelGGL(r2l_pose_batch_kernel, dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(256), 0, (hipStream_t)stream,
                       images, c2w, H, W, focal, z, perm_half_bits(hw), n, N, rays_o, rays_d, target, ids_out);
    R2L_CHECK(hipGetLastError());
    return 0;
}

// Floats of r2l_pose_grad's scratch: the partials of the first launch and of the first reduce level (later levels alternate
// between the two); 0 for n <= 256.  -1: P < 0, n < 0, or 2^31 rays or more.
extern "C" int64_t r2l_pose_grad_work_floats(int64_t P, int64_t n) {
    if (P < 0 || n < 0 || (P > 0 && n > MAX_RAYS / P)) {
        r2l_set_error_msg("r2l_pose_grad_work_floats: need P >= 0, n >= 0 and P * n < 2^31");
        return -1;
    }
    const int64_t K = pg_chunks(n);
    if (P == 0 || K <= 1) return 0;
    return round1k(P * K * 8) + round1k(P * pg_groups(K) * 8);
}

extern "C" int r2l_pose_grad(const float* rays_d, const float* d_rays_o, const float* d_rays_d, const float* rgb, const float* target,
                             int64_t P, int64_t n, float* grad, float* loss, float* work, void* stream) {
    R2L_REQUIRE(P >= 0 && n >= 0, "r2l_pose_grad: P or n is negative");
    if (P == 0) return 0;
    R2L_REQUIRE(n >= 1, "r2l_pose_grad: need n >= 1 (a pose without rays has no mean)");
    R2L_REQUIRE(n <= MAX_RAYS / P, "r2l_pose_grad: P * n must stay below 2^31 rays");
    R2L_REQUIRE(rays_d && d_rays_o && d_rays_d && rgb && target && grad,
                "r2l_pose_grad: a required pointer is NULL (rays_d, d_rays_o, d_rays_d, rgb, target, grad)");
    int64_t K = pg_chunks(n);
    R2L_REQUIRE(K == 1 || (work != nullptr && aligned16(work)), "r2l_pose_grad: work is NULL or not 16-byte aligned (n > 256)");
    const hipStream_t st = (hipStream_t)stream;
    const float den = (float)(3.0 * (double)n);
    const bool vec = n % 4 == 0 && aligned16(rays_d) && aligned16(d_rays_o) && aligned16(d_rays_d) && aligned16(rgb) && aligned16(target);
    float* a = work;
    float* b = K > 1 ? work + round1k(P * K * 8) : nullptr;
    if (vec)
        hipLaunchKernelGGL(r2l_pose_grad_kernel<true>, dim3((unsigned)(P * K)), dim3(64), 0, st, rays_d, d_rays_o, d_rays_d, rgb, target,
                           n, K, den, a, grad, loss);
    else
        hipLaunchKernelGGL(r2l_pose_grad_kernel<false>, dim3((unsigned)(P * K)), dim3(64), 0, st, rays_d, d_rays_o, d_rays_d, rgb, target,
                           n, K, den, a, grad, loss);
    R2L_CHECK(hipGetLastError());
    while (K > 1) {
        const int64_t K_out = pg_groups(K);
        hipLaunchKernelGGL(r2l_pose_grad_reduce_kernel, dim3((unsigned)(P * K_out)), dim3(64), 0, st, a, K, K_out, den, b, grad, loss);
        R2L_CHECK(hipGetLastError());
        float* const x = a; a = b; b = x;
        K = K_out;
    }
    return 0;
}

extern "C" int r2l_pose_update(float* c2w, float* exp_avg, float* exp_avg_sq, const float* grad, int P, float lr_rot, float lr_trans,
                               float beta1, float beta2, float eps, int64_t step, void* stream) {
    R2L_REQUIRE(P >= 0, "r2l_pose_update: P is negative");
    R2L_REQUIRE(step >= 1, "r2l_pose_update: need step >= 1");
    if (P == 0) return 0;
    R2L_REQUIRE(c2w && exp_avg && exp_avg_sq && grad, "r2l_pose_update: a required pointer is NULL (c2w, exp_avg, exp_avg_sq, grad)");
    // bias corrections in double from the fp32 betas, rounded once (beyond 2^31 steps the power is 0 for every beta < 1 in use)
    const double s = (double)(step > 0x7fffffff ? 0x7fffffff : step);
    const float bc1 = (float)(1.0 - pow((double)beta1, s)), sqrt_bc2 = (float)sqrt(1.0 - pow((double)beta2, s));
    hipLaunchKernelGGL(r2l_pose_update_kernel, dim3((unsigned)((P + 63) / 64)), dim3(64), 0, (hipStream_t)stream, c2w, exp_avg, exp_avg_sq,
                       grad, P, lr_rot / bc1, lr_trans / bc1, beta1, beta2, eps, sqrt_bc2);
    R2L_CHECK(hipGetLastError());
    return 0;
}

extern "C" int64_t r2l_pose_refine_work_floats(const r2l_pose_refine_step_desc* d) {
    if (const char* why = pose_desc_check(d)) {
        r2l_set_error_msg(why);
        return -1;
    }
    return pose_work(d).total;
}

extern "C" int r2l_pose_refine_step(const r2l_pose_refine_step_desc* d, const float* images, float* c2w, float* exp_avg,
                                    float* exp_avg_sq, const float* ztab, const float* params, float* wstream, float* wstream_bwd,
                                    float* loss_out, float* work, void* stream) {
    if (const char* why = pose_desc_check(d)) {
        r2l_set_error_msg(why);
        return (int)hipErrorInvalidValue;
    }
    R2L_REQUIRE(images != nullptr, "r2l_pose_refine_step: images is NULL");
    R2L_REQUIRE(c2w != nullptr, "r2l_pose_refine_step: c2w is NULL");
    R2L_REQUIRE(exp_avg != nullptr, "r2l_pose_refine_step: exp_avg is NULL");
    R2L_REQUIRE(exp_avg_sq != nullptr, "r2l_pose_refine_step: exp_avg_sq is NULL");
    R2L_REQUIRE(ztab != nullptr, "r2l_pose_refine_step: ztab is NULL");
    R2L_REQUIRE(params != nullptr, "r2l_pose_refine_step: params is NULL");
    R2L_REQUIRE(wstream != nullptr, "r2l_pose_refine_step: wstream is NULL");
    R2L_REQUIRE(wstream_bwd != nullptr, "r2l_pose_refine_step: wstream_bwd is NULL");
    R2L_REQUIRE(loss_out != nullptr, "r2l_pose_refine_step: loss_out is NULL");
    R2L_REQUIRE(work != nullptr, "r2l_pose_refine_step: work is NULL");
    R2L_REQUIRE(aligned16(work), "r2l_pose_refine_step: work must be 16-byte aligned");

    const PoseWork w = pose_work(d);
    const int nb = d->n_block;
    const int64_t N = (int64_t)d->P * d->n;
    float *const o = work + w.o, *const dd = work + w.d, *const t = work + w.t, *const rgb = work + w.rgb;
    float *const gx = work + w.gx, *const d_o = work + w.d_o, *const d_d = work + w.d_d, *const grad = work + w.grad;
    int rc;

    if ((rc = r2l_pose_batch(images, c2w, d->P, d->H, d->W, d->focal, d->seed, d->iteration, d->n, o, dd, t, nullptr, stream))) return rc;
    if (d->pack) {
        if ((rc = r2l_pack_forward_layout(params, nb, wstream, r2l_forward_layout_for_cfg(N, 1, d->cfg), stream))) return rc;
        if ((rc = r2l_pack_backward_layout(params, nb, wstream_bwd, r2l_backward_layout_for_cfg(N, d->cfg), stream))) return rc;
    }
    if ((rc = r2l_forward_rays_cfg(o, dd, nullptr, ztab, wstream, params, nb, rgb, work + w.save_x, work + w.save_t, N, stream, d->cfg)))
        return rc;
    // every pose's loss is its own mean: dL/drgb = 2 (rgb - target) / (3 n).  The chain alone never touches `grads`, which the
    // entry point wants non-NULL: dpre stands in for it, as in r2l_amd/autograd.py
    const float grad_scale = (float)(2.0 / (3.0 * (double)d->n));
    if ((rc = r2l_backward_part_cfg(o, dd, nullptr, ztab, nullptr, rgb, t, nullptr, work + w.save_x, work + w.save_t, wstream_bwd, params,
                                    nb, grad_scale, work + w.dpre, gx, work + w.gt, work + w.sqerr, work + w.dpre, nullptr, N, stream,
                                    R2L_BWD_CHAIN, 0, 2 * nb, d->cfg)))
        return rc;
    if ((rc = r2l_backward_input(gx, params, nb, o, dd, nullptr, ztab, nullptr, d_o, d_d, N, stream))) return rc;
    if ((rc = r2l_pose_grad(dd, d_o, d_d, rgb, t, d->P, d->n, grad, loss_out, work + w.pg, stream))) return rc;
    return r2l_pose_update(c2w, exp_avg, exp_avg_sq, grad, d->P, d->lr_rot, d->lr_trans, d->beta1, d->beta2, d->eps, d->iteration, stream);
}
