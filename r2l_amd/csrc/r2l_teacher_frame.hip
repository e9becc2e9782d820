// r2l_teacher_frame.hip — teacher frames from camera poses in one library call (include/r2l_hip.h "teacher frames").
//   r2l_frame_rays        : get_rays (utils/run_nerf_raybased_helpers.py:231-257) + the viewdirs of
//                           create_data.py:138-147 for K whole frames, one launch
//   r2l_ndc_rays          : ndc_rays (helpers:260-279) of explicit rays; the same arithmetic inside the frames' ray kernel
//   r2l_draw_uniform      : counter-based uniforms (Philox4x32-10), a pure function of (seed, stream_id, element index): every
//                           host of the C ABI draws the same t_rand / u, whatever its grouping of frames or chunks of rays
//   r2l_draw_normal       : standard normals by Box-Muller on the same Philox blocks (the sigma noise of teacher training,
//                           csrc/r2l_teacher_step.hip)
//   r2l_teacher_frames_cfg: rays -> stratified z -> coarse MLP -> raw2outputs -> sample_pdf + sort -> fine MLP -> raw2outputs,
//                           the EXISTING kernels of those stages enqueued back to back on the caller's stream through one work
//                           buffer the caller sized once: no allocation, no host synchronisation
//   r2l_teacher_frames_occ_cfg: the same body with each point-network launch replaced by r2l_occ_index -> r2l_teacher_mlp_live_cfg
//                           (occupancy grids, the live count read on the device): still no host synchronisation
//   r2l_teacher_frames_ert_cfg: the same body again; its LAST pass walks the samples front to back in segments and leaves out the
//                           rays whose transmittance has fallen below eps (r2l_occ_index_seg -> r2l_teacher_mlp_live_into_cfg ->
//                           r2l_ert_advance per segment), with or without grids
//   r2l_pixel_batch       : the batching mode of teacher training (main.py:1137-1162, 1199-1210) without its bank of rays:
//                           draw t takes pixel pi(epoch_key(seed, t / M), M)(t % M) of the M = n_img*H*W training pixels
//                           (csrc/r2l_perm.h, the ray store's sampler), and its ray is computed on the spot
//   r2l_image_batch       : the images mode of teacher training (main.py:1260-1302): draw j takes position pi(key, win_h*win_w)(j)
//                           of a window of ONE image — n_draw distinct pixels, what np.random.choice(.., replace=False) gives —
//                           through the per-pixel body of r2l_pixel_batch; r2l_image_draw (host arithmetic) names the image and
//                           the key of an iteration
// The kernels here move 12 - 72 bytes per ray: a thread per ray (per Philox block of four draws), no LDS.
#include "r2l_dispatch.h"
#include "r2l_perm.h"
#include "r2l_pixel_ray.h"
#include <initializer_list>
#include <math.h>
#include <stdio.h>

namespace {

// ---- Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) ---------------------------------
__device__ __forceinline__ void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        const unsigned n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// out[j] = uniform of element i0 + j, j < n.  Thread t owns Philox block (i0 >> 2) + t = elements 4 b .. 4 b + 3.
__global__ void r2l_draw_uniform_kernel(float* __restrict__ out, int64_t n, int64_t i0, unsigned long long seed,
                                        unsigned long long stream_id) {
    const int64_t b0 = i0 >> 2, nb = ((i0 + n + 3) >> 2) - b0;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nb; t += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long b = (unsigned long long)(b0 + t);
        unsigned c[4] = {(unsigned)b, (unsigned)(b >> 32), (unsigned)stream_id, (unsigned)(stream_id >> 32)};
        philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int64_t j = (int64_t)(b << 2) + w - i0;
            if (j >= 0 && j < n) out[j] = (float)(c[w] >> 8) * 5.9604644775390625e-08f;  // 2^-24: exact, in [0, 1)
        }
    }
}

// out[i] = scale * n_i, i < n: standard normals by Box-Muller on the same Philox blocks (include/r2l_hip.h).  Thread t owns block t =
// elements 4 t .. 4 t + 3: two (u1, u2) pairs, each giving r cos, r sin.  The angle is 2 pi u2 with u2 a multiple of 2^-24: 2 u2 is
// exact and sincospif reduces it exactly, where fp32(2 pi) * u2 would carry the rounding of the product into the angle (up to
// pi * 2^-24 absolute, which alone is 3 * 2^-24 r in the result; the whole kernel measures 2.4 * 2^-24 r).  logf and sqrtf are the accurate library forms (1 ulp /
// correctly rounded): a dozen of them per 16 bytes written is nothing beside the step these draws feed, and the fast forms
// (v_log_f32 is ~1 ulp in log2 only, which the 0.693 factor and the argument near 1 do not preserve) would miss the tail.
__global__ void r2l_draw_normal_kernel(float* __restrict__ out, int64_t n, unsigned long long seed, unsigned long long stream_id,
                                       float scale) {
    const int64_t nb = (n + 3) >> 2;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nb; t += (int64_t)gridDim.x * blockDim.x) {
        unsigned c[4] = {(unsigned)t, (unsigned)((unsigned long long)t >> 32), (unsigned)stream_id, (unsigned)(stream_id >> 32)};
        philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
        float v[4];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const float u1 = (float)((c[2 * p] >> 8) + 1u) * 5.9604644775390625e-08f;  // (0, 1]: exact
            const float a = (float)(c[2 * p + 1] >> 8) * 1.1920928955078125e-07f;      // 2 u2 in [0, 2): exact
            const float r = sqrtf(-2.f * logf(u1));
            float sn, cs;
            sincospif(a, &sn, &cs);
            v[2 * p] = r * cs;
            v[2 * p + 1] = r * sn;
        }
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int64_t j = (t << 2) + w;
            if (j < n) out[j] = scale * v[w];
        }
    }
}

// ndc_rays (utils/run_nerf_raybased_helpers.py:260-279) of one ray, separately rounded fp32 in the order of include/r2l_hip.h.
// o2 / d2 may alias o / d: everything is read before anything is written.
__device__ __forceinline__ void ndc_one(const float (&o)[3], const float (&d)[3], float cw, float ch, float near, float (&o2)[3],
                                        float (&d2)[3]) {
    const float t = (-(near + o[2])) / d[2];
    const float sx = o[0] + t * d[0], sy = o[1] + t * d[1], sz = o[2] + t * d[2];
    const float qx = sx / sz, qy = sy / sz, dx = d[0] / d[2], dy = d[1] / d[2];
    o2[0] = (cw * sx) / sz; o2[1] = (ch * sy) / sz; o2[2] = 1.f + (2.f * near) / sz;
    d2[0] = cw * (dx - qx); d2[1] = ch * (dy - qy); d2[2] = (-2.f * near) / sz;
}

// pixel_ray (csrc/r2l_pixel_ray.h): the world ray of a pixel, the one definition behind r2l_frame_rays and r2l_pixel_batch —
// and behind r2l_cstore_batch, which recomputes these very rays.

// (x^2 + z^2) + y^2: the association of torch.norm's reduction over a 3-vector, so that render()'s own normalisation of
// these rays_d gives these bits (tests/test_teacher_frames_gpu.py: fused = unfused)
__device__ __forceinline__ float ray_norm(const float (&d)[3]) { return sqrtf((d[0] * d[0] + d[2] * d[2]) + d[1] * d[1]); }

// Rays first .. first + n of the K*H*W rays of K frames (ray r = (k*H + row)*W + col); outputs are indexed by r - first.
// NDC: rows and viewdirs take the world ray, rays_o / rays_d its ndc_rays image at near plane 1 (create_data.py:138-152).
template <bool NDC>
__device__ __forceinline__ void frame_rays_body(const float* __restrict__ c2w, const float* __restrict__ focal_dev, float focal, int H,
                                                int W, int64_t first, int64_t n, float* __restrict__ rays_o,
                                                float* __restrict__ rays_d, float* __restrict__ viewdirs, float* __restrict__ rows,
                                                float* __restrict__ nearfar, float near, float far, float cw, float ch) {
    const int64_t hw = (int64_t)H * W;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = first + j, k = r / hw, pix = r - k * hw;
        const int row = (int)(pix / W), col = (int)(pix - (int64_t)row * W);
        float o[3], d[3];
        pixel_ray(c2w + k * 12, focal_dev != nullptr ? focal_dev[k] : focal, H, W, row, col, o, d);
        float on[3], dn[3];
        if (NDC) ndc_one(o, d, cw, ch, 1.f, on, dn);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (rays_o != nullptr) rays_o[j * 3 + i] = NDC ? on[i] : o[i];
            if (rays_d != nullptr) rays_d[j * 3 + i] = NDC ? dn[i] : d[i];
            if (rows != nullptr) { rows[j * 9 + i] = o[i]; rows[j * 9 + 3 + i] = d[i]; }
        }
        if (viewdirs != nullptr) {
            const float nrm = ray_norm(d);
#pragma unroll
            for (int i = 0; i < 3; ++i) viewdirs[j * 3 + i] = d[i] / nrm;
        }
        if (nearfar != nullptr && j == 0) { nearfar[0] = near; nearfar[1] = far; }
    }
}

__global__ void r2l_frame_rays_kernel(const float* __restrict__ c2w, const float* __restrict__ focal_dev, float focal, int H, int W,
                                      int64_t first, int64_t n, float* __restrict__ rays_o, float* __restrict__ rays_d,
                                      float* __restrict__ viewdirs, float* __restrict__ rows, float* __restrict__ nearfar, float near,
                                      float far) {
    frame_rays_body<false>(c2w, focal_dev, focal, H, W, first, n, rays_o, rays_d, viewdirs, rows, nearfar, near, far, 0.f, 0.f);
}

__global__ void r2l_frame_rays_ndc_kernel(const float* __restrict__ c2w, const float* __restrict__ focal_dev, float focal, int H,
                                          int W, int64_t first, int64_t n, float* __restrict__ rays_o, float* __restrict__ rays_d,
                                          float* __restrict__ viewdirs, float* __restrict__ rows, float* __restrict__ nearfar,
                                          float near, float far, float cw, float ch) {
    frame_rays_body<true>(c2w, focal_dev, focal, H, W, first, n, rays_o, rays_d, viewdirs, rows, nearfar, near, far, cw, ch);
}

// ndc_o / ndc_d [n,3] = ndc_rays of rays_o / rays_d [n,3]; the outputs may be the inputs (a thread reads its ray first).
// No __restrict__: the pointers may alias.
__global__ void r2l_ndc_rays_kernel(const float* rays_o, const float* rays_d, int64_t n, float cw, float ch, float near, float* ndc_o,
                                    float* ndc_d) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
        float o[3], d[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) { o[i] = rays_o[j * 3 + i]; d[i] = rays_d[j * 3 + i]; }
        ndc_one(o, d, cw, ch, near, o, d);
#pragma unroll
        for (int i = 0; i < 3; ++i) { ndc_o[j * 3 + i] = o[i]; ndc_d[j * 3 + i] = d[i]; }
    }
}

// Output row j of a pixel sampler: pixel g = (img * H + row) * W + col of the training images.  The ONE per-pixel body behind
// r2l_pixel_batch and r2l_image_batch, which differ only in how they choose (img, row, col).  NDC: viewdirs take the world ray,
// rays_o / rays_d its ndc_rays image at near plane 1 (what train_nerf.device_rays does to the selected rays).
template <bool NDC>
__device__ __forceinline__ void pixel_row(const float* __restrict__ images, const float* __restrict__ c2w, int H, int W, float focal,
                                          int64_t img, int row, int col, int64_t j, float* __restrict__ rays_o,
                                          float* __restrict__ rays_d, float* __restrict__ viewdirs, float* __restrict__ target,
                                          int64_t* __restrict__ ids_out, float cw, float ch) {
    const int64_t g = (img * H + row) * W + col;
    float o[3], d[3];
    pixel_ray(c2w + img * 12, focal, H, W, row, col, o, d);
    const float nrm = ray_norm(d);
    float on[3], dn[3];
    if (NDC) ndc_one(o, d, cw, ch, 1.f, on, dn);
    const float* __restrict__ px = images + g * 3;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        rays_o[j * 3 + i] = NDC ? on[i] : o[i];
        rays_d[j * 3 + i] = NDC ? dn[i] : d[i];
        viewdirs[j * 3 + i] = d[i] / nrm;
        target[j * 3 + i] = px[i];
    }
    if (ids_out != nullptr) ids_out[j] = g;
}

// Draw t = draw0 + j of the pixel sampler: pixel g = pi(epoch_key(seed, t / M), M)(t % M) of the M = n_img * hw training pixels,
// g = (img * H + row) * W + col.  A thread per draw; the cycle walk of perm_at diverges within a wave (~2 trips at worst on
// average).  Every index is 64-bit.
template <bool NDC>
__global__ void r2l_pixel_batch_kernel(const float* __restrict__ images, const float* __restrict__ c2w, int H, int W, float focal,
                                       int64_t M, int half_bits, int64_t draw0, int64_t n_draw, unsigned long long seed,
                                       float* __restrict__ rays_o, float* __restrict__ rays_d, float* __restrict__ viewdirs,
                                       float* __restrict__ target, int64_t* __restrict__ ids_out, float cw, float ch) {
    const int64_t hw = (int64_t)H * W;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_draw; j += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long t = (unsigned long long)(draw0 + j), epoch = t / (unsigned long long)M;
        unsigned k[4];
        perm_round_keys(perm_epoch_key(seed, epoch), k);
        const int64_t g = (int64_t)perm_at(t - epoch * (unsigned long long)M, (unsigned long long)M, half_bits, k);
        const int64_t img = g / hw, pix = g - img * hw;
        const int row = (int)(pix / W), col = (int)(pix - (int64_t)row * W);
        pixel_row<NDC>(images, c2w, H, W, focal, img, row, col, j, rays_o, rays_d, viewdirs, target, ids_out, cw, ch);
    }
}

// Draw j of the images-mode sampler: position q = pi(key, n_win)(j) of the win_h x win_w window at (row0, col0) of image img,
// row-major (n_win = win_h * win_w, j < n_draw <= n_win: a prefix of a bijection, so the pixels are distinct).  A thread per draw,
// the same cycle walk and the same body as above.
template <bool NDC>
__global__ void r2l_image_batch_kernel(const float* __restrict__ images, const float* __restrict__ c2w, int H, int W, float focal,
                                       int img, int row0, int col0, int win_w, int64_t n_win, int half_bits, int64_t n_draw,
                                       unsigned long long key, float* __restrict__ rays_o, float* __restrict__ rays_d,
                                       float* __restrict__ viewdirs, float* __restrict__ target, int64_t* __restrict__ ids_out,
                                       float cw, float ch) {
    unsigned k[4];
    perm_round_keys(key, k);  // (uniform over the grid: a few dozen integer ops)
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_draw; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t q = (int64_t)perm_at((unsigned long long)j, (unsigned long long)n_win, half_bits, k);
        const int wr = (int)(q / win_w), wc = (int)(q - (int64_t)wr * win_w);
        pixel_row<NDC>(images, c2w, H, W, focal, (int64_t)img, row0 + wr, col0 + wc, j, rays_o, rays_d, viewdirs, target, ids_out, cw,
                       ch);
    }
}

// cw (extent = W) / ch (extent = H) of ndc_rays: -1 / (extent / (2 focal)) as torch evaluates it for an fp32 tensor focal,
// where number / tensor is reciprocal(tensor) * number:  r = 1 / (2 focal);  c = -(1 / (r * extent))
float ndc_coef(int extent, float focal) {
    const float r = 1.f / (2.f * focal);
    return -(1.f / (r * (float)extent));
}

// rows[r, 6:9] = rgb[r, :]
__global__ void r2l_rows_rgb_kernel(const float* __restrict__ rgb, float* __restrict__ rows, int64_t n) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n * 3; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = e / 3;
        rows[r * 9 + 6 + (e - r * 3)] = rgb[e];
    }
}

unsigned grid_for(int64_t total) {
    const int64_t g = (total + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

int launch_draw(float* out, int64_t n, int64_t i0, uint64_t seed, uint64_t stream_id, hipStream_t stream) {
    hipLaunchKernelGGL(r2l_draw_uniform_kernel, dim3(grid_for((n + 3) / 4 + 1)), dim3(256), 0, stream, out, n, i0,
                       (unsigned long long)seed, (unsigned long long)stream_id);
    R2L_CHECK(hipGetLastError());
    return 0;
}

int launch_rays(const float* c2w, const float* focal_dev, float focal, int H, int W, int64_t first, int64_t n, float* rays_o,
                float* rays_d, float* viewdirs, float* rows, float* nearfar, float near, float far, hipStream_t stream,
                bool ndc = false, float ndc_focal = 0.f) {
    if (ndc)
        hipLaunchKernelGGL(r2l_frame_rays_ndc_kernel, dim3(grid_for(n)), dim3(256), 0, stream, c2w, focal_dev, focal, H, W, first, n,
                           rays_o, rays_d, viewdirs, rows, nearfar, near, far, ndc_coef(W, ndc_focal), ndc_coef(H, ndc_focal));
    else
        hipLaunchKernelGGL(r2l_frame_rays_kernel, dim3(grid_for(n)), dim3(256), 0, stream, c2w, focal_dev, focal, H, W, first, n,
                           rays_o, rays_d, viewdirs, rows, nearfar, near, far);
    R2L_CHECK(hipGetLastError());
    return 0;
}

// What is wrong with a descriptor, or nullptr
const char* desc_check(const r2l_teacher_frame_desc* d) {
    if (d == nullptr) return "r2l_teacher_frame_desc: desc is NULL";
    if (d->H < 1 || d->W < 1) return "r2l_teacher_frame_desc.H / .W: need H >= 1 and W >= 1";
    if (!(d->near < d->far)) return "r2l_teacher_frame_desc.near / .far: need near < far";
    if (d->N_samples < 1) return "r2l_teacher_frame_desc.N_samples: need N_samples >= 1";
    if (d->N_importance < 0) return "r2l_teacher_frame_desc.N_importance: need N_importance >= 0";
    if (d->N_importance > 0 && d->N_samples < 3) return "r2l_teacher_frame_desc.N_samples: need N_samples >= 3 with N_importance > 0";
    if ((int64_t)d->N_samples + d->N_importance > 256) return "r2l_teacher_frame_desc.N_samples + .N_importance: at most 256";
    if (d->N_importance > 0 && (d->N_samples > 64 || d->N_importance > 192))
        return "r2l_teacher_frame_desc.N_samples / .N_importance: r2l_sample_pdf_sort needs N_samples <= 64 and N_importance <= 192";
    if (d->perturb != 0 && d->perturb != 1) return "r2l_teacher_frame_desc.perturb: 0 or 1";
    if (d->raw_noise_std != 0.f) return "r2l_teacher_frame_desc.raw_noise_std: must be 0";
    if (d->chunk_rays < 0) return "r2l_teacher_frame_desc.chunk_rays: need chunk_rays >= 0";
    if (d->ndc != 0 && d->ndc != 1) return "r2l_teacher_frame_desc.ndc: 0 or 1";
    if (d->ndc == 1 && !(d->focal > 0.f)) return "r2l_teacher_frame_desc.focal: need focal > 0 with .ndc = 1 (also with focal_dev)";
    if (d->reserved[0] || d->reserved[1] || d->reserved[2]) return "r2l_teacher_frame_desc.reserved: must be 0";
    return nullptr;
}

// The work buffer: every part starts on a 16-byte boundary (the quarter-wave kernels of r2l_render.hip take aligned pointers)
struct FrameWork {
    int64_t nearfar, o, d, v, z, raw, wts, zs, zall, trand, u, rgb_c, s_c, rgb_f, s_f, total;
};
int64_t r4(int64_t n) { return (n + 3) & ~(int64_t)3; }
FrameWork frame_work(const r2l_teacher_frame_desc* d) {
    const int64_t hw = (int64_t)d->H * d->W;
    const int64_t cr = d->chunk_rays > 0 && d->chunk_rays < hw ? d->chunk_rays : hw;
    const int64_t S = d->N_samples, NI = d->N_importance, T = S + NI;
    FrameWork w{};
    int64_t at = 0;
    auto take = [&](int64_t n) { const int64_t a = at; at += r4(n); return a; };
    w.nearfar = take(2);
    w.o = take(cr * 3); w.d = take(cr * 3); w.v = take(cr * 3);
    w.z = take(cr * S);
    w.raw = take(cr * T * 4);
    w.wts = take(NI > 0 ? cr * S : 0);
    w.zs = take(cr * NI);
    w.zall = take(NI > 0 ? cr * T : 0);
    w.trand = take(d->perturb ? cr * S : 0);
    w.u = take(d->perturb ? cr * NI : 0);
    w.rgb_c = take(cr * 3); w.s_c = take(r4(cr) * 3);  // coarse rgb0 | disp0, acc0, depth0
    w.rgb_f = take(cr * 3); w.s_f = take(r4(cr) * 3);  // stand-ins for final outputs the caller passed as NULL
    w.total = at;
    return w;
}

// What the occupancy form adds behind the plain work buffer: idx (int64 per sample of the larger pass), the count, the index work
struct OccWork {
    int64_t idx, count, iwork, total;
};
OccWork occ_work(const r2l_teacher_frame_desc* d, const FrameWork& w) {
    const int64_t hw = (int64_t)d->H * d->W;
    const int64_t cr = d->chunk_rays > 0 && d->chunk_rays < hw ? d->chunk_rays : hw;
    const int64_t n = cr * ((int64_t)d->N_samples + d->N_importance);  // samples of the larger pass
    OccWork o{};
    o.idx = w.total;
    o.count = o.idx + r4(2 * n);
    o.iwork = o.count + 4;
    const int64_t ib = n < ((int64_t)1 << 31) ? r2l_occ_index_work_bytes(n) : 0;  // (a larger pass is refused by the index call)
    o.total = o.iwork + r4((ib + 3) / 4);
    return o;
}

// The grids of the occupancy form (both NULL: the early-termination form without grids) and the early termination of the last pass,
// or none: the ONE body below serves the three entry points
struct FrameOcc {
    const r2l_occ_grid *coarse, *fine;
    int64_t* live_acc;
    const r2l_ert_desc* ert;
};

// What is wrong with an early-termination descriptor, or nullptr
const char* ert_check(const r2l_ert_desc* e) {
    if (e == nullptr) return "r2l_ert_desc: ert is NULL";
    if (!(e->eps > 0.f && e->eps <= 0.1f)) return "r2l_ert_desc.eps: need 0 < eps <= 0.1";
    if (e->seg < 8) return "r2l_ert_desc.seg: need seg >= 8";
    if (e->reserved[0] || e->reserved[1]) return "r2l_ert_desc.reserved: must be 0";
    return nullptr;
}

int frames_body(const char* who, const float* c2w_dev, const float* focal_dev, int K, const r2l_teacher_frame_desc* d, const float* ttab,
                const float* u_det, const float* wstream_coarse, const float* tparams_coarse, const float* wstream_fine,
                const float* tparams_fine, float* rows, float* rgb, float* disp, float* acc, float* depth, float* rgb0, float* work,
                void* stream, const r2l_config* cfg, const FrameOcc* occ);

}  // namespace

extern "C" int r2l_draw_uniform(float* out, int64_t n, uint64_t seed, uint64_t stream_id, void* stream) {
    R2L_REQUIRE(n >= 0, "r2l_draw_uniform: n is negative");
    if (n == 0) return 0;
    R2L_REQUIRE(out != nullptr, "r2l_draw_uniform: out is NULL");
    return launch_draw(out, n, 0, seed, stream_id, (hipStream_t)stream);
}

extern "C" int r2l_draw_normal(float* out, int64_t n, uint64_t seed, uint64_t stream_id, float scale, void* stream) {
    R2L_REQUIRE(n >= 0, "r2l_draw_normal: n is negative");
    if (n == 0) return 0;
    R2L_REQUIRE(out != nullptr, "r2l_draw_normal: out is NULL");
    hipLaunchKernelGGL(r2l_draw_normal_kernel, dim3(grid_for((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, out, n,
                       (unsigned long long)seed, (unsigned long long)stream_id, scale);
    R2L_CHECK(hipGetLastError());
    return 0;
}

extern "C" int r2l_frame_rays(const float* c2w_dev, const float* focal_dev, float focal, int K, int H, int W, float* rays_o,
                              float* rays_d, float* viewdirs, float* rows, void* stream) {
    R2L_REQUIRE(K >= 0, "r2l_frame_rays: K is negative");
    R2L_REQUIRE(H >= 1 && W >= 1, "r2l_frame_rays: need H >= 1 and W >= 1");
    R2L_REQUIRE(focal_dev != nullptr || focal > 0.f, "r2l_frame_rays: need focal > 0 (or focal_dev)");
    if (K == 0) return 0;
    R2L_REQUIRE(c2w_dev != nullptr, "r2l_frame_rays: c2w_dev is NULL");
    if (!rays_o && !rays_d && !viewdirs && !rows) return 0;
    return launch_rays(c2w_dev, focal_dev, focal, H, W, 0, (int64_t)K * H * W, rays_o, rays_d, viewdirs, rows, nullptr, 0.f, 0.f,
                       (hipStream_t)stream);
}

extern "C" int r2l_ndc_rays(const float* rays_o, const float* rays_d, int64_t n, int H, int W, float focal, float near, float* ndc_o,
                            float* ndc_d, void* stream) {
    R2L_REQUIRE(n >= 0, "r2l_ndc_rays: n is negative");
    R2L_REQUIRE(H >= 1 && W >= 1, "r2l_ndc_rays: need H >= 1 and W >= 1");
    R2L_REQUIRE(focal > 0.f, "r2l_ndc_rays: need focal > 0");
    if (n == 0) return 0;
    R2L_REQUIRE(rays_o && rays_d && ndc_o && ndc_d, "r2l_ndc_rays: a pointer is NULL (rays_o, rays_d, ndc_o, ndc_d)");
    hipLaunchKernelGGL(r2l_ndc_rays_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, rays_o, rays_d, n, ndc_coef(W, focal),
                       ndc_coef(H, focal), near, ndc_o, ndc_d);
    R2L_CHECK(hipGetLastError());
    return 0;
}

extern "C" int r2l_pixel_batch(const float* images, const float* c2w, int n_img, int H, int W, float focal, int ndc, int64_t draw0,
                               int64_t n_draw, uint64_t seed, float* rays_o, float* rays_d, float* viewdirs, float* target,
                               int64_t* ids_out, void* stream) {
    R2L_REQUIRE(n_img >= 1 && H >= 1 && W >= 1, "r2l_pixel_batch: need n_img >= 1, H >= 1 and W >= 1");
    R2L_REQUIRE(focal > 0.f, "r2l_pixel_batch: need focal > 0");
    R2L_REQUIRE(ndc == 0 || ndc == 1, "r2l_pixel_batch: ndc is 0 or 1");
    R2L_REQUIRE(n_draw >= 0, "r2l_pixel_batch: n_draw is negative");
    R2L_REQUIRE(draw0 >= 0 && draw0 <= INT64_MAX - n_draw, "r2l_pixel_batch: draw0 is negative (or draw0 + n_draw overflows)");
    const int64_t nh = (int64_t)n_img * H;  // < 2^62; checked before it is multiplied again
    R2L_REQUIRE(nh <= 0x7fffffff && nh * W <= 0x7fffffff, "r2l_pixel_batch: need n_img * H * W < 2^31 pixels");
    const int64_t M = nh * W;
    R2L_REQUIRE(images && c2w && rays_o && rays_d && viewdirs && target,
                "r2l_pixel_batch: a required pointer is NULL (images, c2w, rays_o, rays_d, viewdirs, target)");
    if (n_draw == 0) return 0;
    const hipStream_t st = (hipStream_t)stream;
    if (ndc)
        hipLaunchKernelGGL(r2l_pixel_batch_kernel<true>, dim3(grid_for(n_draw)), dim3(256), 0, st, images, c2w, H, W, focal, M,
                           perm_half_bits(M), draw0, n_draw, (unsigned long long)seed, rays_o, rays_d, viewdirs, target, ids_out,
                           ndc_coef(W, focal), ndc_coef(H, focal));
    else
        hipLaunchKernelGGL(r2l_pixel_batch_kernel<false>, dim3(grid_for(n_draw)), dim3(256), 0, st, images, c2w, H, W, focal, M,
                           perm_half_bits(M), draw0, n_draw, (unsigned long long)seed, rays_o, rays_d, viewdirs, target, ids_out, 0.f,
                           0.f);
    R2L_CHECK(hipGetLastError());
    return 0;
}

extern "C" int r2l_image_batch(const float* images, const float* c2w, int n_img, int H, int W, float focal, int ndc, int img, int row0,
                               int col0, int win_h, int win_w, uint64_t key, int64_t n_draw, float* rays_o, float* rays_d,
                               float* viewdirs, float* target, int64_t* ids_out, void* stream) {
    R2L_REQUIRE(n_img >= 1 && H >= 1 && W >= 1, "r2l_image_batch: need n_img >= 1, H >= 1 and W >= 1");
    R2L_REQUIRE(focal > 0.f, "r2l_image_batch: need focal > 0");
    R2L_REQUIRE(ndc == 0 || ndc == 1, "r2l_image_batch: ndc is 0 or 1");
    R2L_REQUIRE(n_draw >= 0, "r2l_image_batch: n_draw is negative");
    const int64_t nh = (int64_t)n_img * H;  // < 2^62; checked before it is multiplied again
    R2L_REQUIRE(nh <= 0x7fffffff && nh * W <= 0x7fffffff, "r2l_image_batch: need n_img * H * W < 2^31 pixels");
    R2L_REQUIRE(img >= 0 && img < n_img, "r2l_image_batch: img is outside [0, n_img)");
    R2L_REQUIRE(win_h >= 1 && win_w >= 1, "r2l_image_batch: need win_h >= 1 and win_w >= 1");
    R2L_REQUIRE(row0 >= 0 && (int64_t)row0 + win_h <= H, "r2l_image_batch: row0 / win_h: the window leaves the frame");
    R2L_REQUIRE(col0 >= 0 && (int64_t)col0 + win_w <= W, "r2l_image_batch: col0 / win_w: the window leaves the frame");
    const int64_t n_win = (int64_t)win_h * win_w;  // <= H * W < 2^31
    R2L_REQUIRE(n_draw <= n_win, "r2l_image_batch: n_draw exceeds the win_h * win_w pixels of the window");
    R2L_REQUIRE(images && c2w && rays_o && rays_d && viewdirs && target,
                "r2l_image_batch: a required pointer is NULL (images, c2w, rays_o, rays_d, viewdirs, target)");
    if (n_draw == 0) return 0;
    const hipStream_t st = (hipStream_t)stream;
    if (ndc)
        hipLaunchKernelGGL(r2l_image_batch_kernel<true>, dim3(grid_for(n_draw)), dim3(256), 0, st, images, c2w, H, W, focal, img, row0,
                           col0, win_w, n_win, perm_half_bits(n_win), n_draw, (unsigned long long)key, rays_o, rays_d, viewdirs, target,
                           ids_out, ndc_coef(W, focal), ndc_coef(H, focal));
    else
        hipLaunchKernelGGL(r2l_image_batch_kernel<false>, dim3(grid_for(n_draw)), dim3(256), 0, st, images, c2w, H, W, focal, img, row0,
                           col0, win_w, n_win, perm_half_bits(n_win), n_draw, (unsigned long long)key, rays_o, rays_d, viewdirs, target,
                           ids_out, 0.f, 0.f);
    R2L_CHECK(hipGetLastError());
    return 0;
}

// Host arithmetic only: the image and the window key of an iteration (include/r2l_hip.h).
extern "C" int r2l_image_draw(uint64_t seed, int64_t iteration, int n_img, int* img_out, uint64_t* key_out) {
    R2L_REQUIRE(iteration >= 1, "r2l_image_draw: need iteration >= 1");
    R2L_REQUIRE(n_img >= 1, "r2l_image_draw: need n_img >= 1");
    R2L_REQUIRE(img_out != nullptr && key_out != nullptr, "r2l_image_draw: a required pointer is NULL (img_out, key_out)");
    const unsigned long long z = perm_epoch_key(seed ^ 0x696D675F6D6F6465ull, (unsigned long long)iteration);
    *img_out = (int)(((z >> 40) * (unsigned long long)n_img) >> 24);
    *key_out = perm_epoch_key(z, 0);
    return 0;
}

extern "C" int64_t r2l_teacher_frames_work_floats(const r2l_teacher_frame_desc* d) {
    if (const char* why = desc_check(d)) {
        r2l_set_error_msg(why);
        return -1;
    }
    return frame_work(d).total;
}

extern "C" int r2l_teacher_frames_cfg(const float* c2w_dev, const float* focal_dev, int K, const r2l_teacher_frame_desc* d,
                                      const float* ttab, const float* u_det, const float* wstream_coarse, const float* tparams_coarse,
                                      const float* wstream_fine, const float* tparams_fine, float* rows, float* rgb, float* disp,
                                      float* acc, float* depth, float* rgb0, float* work, void* stream, const r2l_config* cfg) {
    return frames_body("r2l_teacher_frames_cfg", c2w_dev, focal_dev, K, d, ttab, u_det, wstream_coarse, tparams_coarse, wstream_fine,
                       tparams_fine, rows, rgb, disp, acc, depth, rgb0, work, stream, cfg, nullptr);
}

extern "C" int64_t r2l_teacher_frames_occ_work_floats(const r2l_teacher_frame_desc* d) {
    if (const char* why = desc_check(d)) {
        r2l_set_error_msg(why);
        return -1;
    }
    return occ_work(d, frame_work(d)).total;
}

extern "C" int64_t r2l_teacher_frames_ert_work_floats(const r2l_teacher_frame_desc* d, const r2l_ert_desc* ert) {
    const char* why = desc_check(d);
    if (why == nullptr) why = ert_check(ert);
    if (why != nullptr) {
        r2l_set_error_msg(why);
        return -1;
    }
    const int64_t hw = (int64_t)d->H * d->W;
    const int64_t cr = d->chunk_rays > 0 && d->chunk_rays < hw ? d->chunk_rays : hw;
    return occ_work(d, frame_work(d)).total + r4(cr);  // (trans of a chunk's rays behind the occupancy form's buffer)
}

extern "C" int r2l_teacher_frames_ert_cfg(const float* c2w_dev, const float* focal_dev, int K, const r2l_teacher_frame_desc* d,
                                          const float* ttab, const float* u_det, const float* wstream_coarse,
                                          const float* tparams_coarse, const float* wstream_fine, const float* tparams_fine, float* rows,
                                          float* rgb, float* disp, float* acc, float* depth, float* rgb0,
                                          const r2l_occ_grid* grid_coarse, const r2l_occ_grid* grid_fine, int64_t* live_acc,
                                          const r2l_ert_desc* ert, float* work, void* stream, const r2l_config* cfg) {
    const char* why = desc_check(d);
    if (why == nullptr) why = ert_check(ert);
    if (why != nullptr) {
        r2l_set_error_msg(why);
        return (int)hipErrorInvalidValue;
    }
    R2L_REQUIRE(grid_coarse != nullptr || grid_fine == nullptr,
                "r2l_teacher_frames_ert_cfg: grid_fine without grid_coarse (both NULL: no grids; grid_fine NULL: grid_coarse serves both passes)");
    R2L_REQUIRE(d->ndc == 0 || grid_coarse == nullptr,
                "r2l_teacher_frames_ert_cfg: r2l_teacher_frame_desc.ndc must be 0 with a grid (the box of an occupancy grid is in world space)");
    for (const r2l_occ_grid* g : {grid_coarse, grid_fine})
        if (g != nullptr)
            if (const char* bad = r2l_occ_grid_why(g, "r2l_teacher_frames_ert_cfg: grid is NULL")) {
                r2l_set_error_msg(bad);
                return (int)hipErrorInvalidValue;
            }
    const FrameOcc occ{grid_coarse, grid_fine ? grid_fine : grid_coarse, live_acc, ert};
    return frames_body("r2l_teacher_frames_ert_cfg", c2w_dev, focal_dev, K, d, ttab, u_det, wstream_coarse, tparams_coarse, wstream_fine,
                       tparams_fine, rows, rgb, disp, acc, depth, rgb0, work, stream, cfg, &occ);
}

extern "C" int r2l_teacher_frames_occ_cfg(const float* c2w_dev, const float* focal_dev, int K, const r2l_teacher_frame_desc* d,
                                          const float* ttab, const float* u_det, const float* wstream_coarse,
                                          const float* tparams_coarse, const float* wstream_fine, const float* tparams_fine, float* rows,
                                          float* rgb, float* disp, float* acc, float* depth, float* rgb0,
                                          const r2l_occ_grid* grid_coarse, const r2l_occ_grid* grid_fine, int64_t* live_acc, float* work,
                                          void* stream, const r2l_config* cfg) {
    if (const char* why = desc_check(d)) {
        r2l_set_error_msg(why);
        return (int)hipErrorInvalidValue;
    }
    R2L_REQUIRE(d->ndc == 0, "r2l_teacher_frames_occ_cfg: r2l_teacher_frame_desc.ndc must be 0 (the box of an occupancy grid is in world space)");
    if (const char* why = r2l_occ_grid_why(grid_coarse, "r2l_teacher_frames_occ_cfg: grid_coarse is NULL")) {
        r2l_set_error_msg(why);
        return (int)hipErrorInvalidValue;
    }
    if (grid_fine != nullptr)
        if (const char* why = r2l_occ_grid_why(grid_fine, "r2l_teacher_frames_occ_cfg: grid_fine is NULL")) {
            r2l_set_error_msg(why);
            return (int)hipErrorInvalidValue;
        }
    const FrameOcc occ{grid_coarse, grid_fine ? grid_fine : grid_coarse, live_acc, nullptr};
    return frames_body("r2l_teacher_frames_occ_cfg", c2w_dev, focal_dev, K, d, ttab, u_det, wstream_coarse, tparams_coarse, wstream_fine,
                       tparams_fine, rows, rgb, disp, acc, depth, rgb0, work, stream, cfg, &occ);
}

namespace {

// a refusal of the body, named after the entry point that was called
#define FRAMES_REQUIRE(cond, msg)                                    \
    do {                                                             \
        if (!(cond)) {                                               \
            static thread_local char buf_[256];                      \
            snprintf(buf_, sizeof buf_, "%s: %s", who, msg);         \
            r2l_set_error_msg(buf_);                                 \
            return (int)hipErrorInvalidValue;                        \
        }                                                            \
    } while (0)

// The point network of one pass: the plain launch, or (occupancy form) index -> [live_acc] -> the live launch, or (the last pass
// of the early-termination form) a zero fill of raw, then per segment of consecutive sample numbers: the index of the segment
// without the rays terminated so far -> [live_acc] -> the live launch into raw -> the transmittance through the segment
int frames_mlp(const float* o, const float* dd, const float* v, const float* z, const float* wstream, const float* tparams, float* raw,
               int64_t cr, int S, void* stream, const r2l_config* cfg, const r2l_occ_grid* grid, const FrameOcc* occ, float* work,
               const OccWork& ow, bool last) {
    if (occ == nullptr) return r2l_teacher_mlp_cfg(o, dd, v, z, wstream, tparams, raw, cr, S, stream, cfg);
    int64_t* const idx = reinterpret_cast<int64_t*>(work + ow.idx);
    int64_t* const count = reinterpret_cast<int64_t*>(work + ow.count);
    int rc;
    if (occ->ert != nullptr && last) {
        float* const trans = work + ow.total;  // [chunk rays], behind the occupancy form's parts
        R2L_CHECK(hipMemsetAsync(raw, 0, (size_t)cr * S * 4 * sizeof(float), (hipStream_t)stream));
        const int seg = occ->ert->seg;
        for (int s0 = 0; s0 < S; s0 += seg) {
            const int s1 = S - s0 < seg ? S : s0 + seg;
            const int64_t cap = cr * (int64_t)(s1 - s0);
            if ((rc = r2l_occ_index_seg(grid, o, dd, z, cr, S, s0, s1, s0 == 0 ? nullptr : trans, occ->ert->eps, idx, count,
                                        work + ow.iwork, stream)))
                return rc;
            if (occ->live_acc != nullptr && (rc = r2l_occ_live_add(count, cap, occ->live_acc, stream))) return rc;
            if ((rc = r2l_teacher_mlp_live_into_cfg(o, dd, v, z, idx, count, cap, wstream, tparams, raw, cr, S, stream, cfg))) return rc;
            if (s1 < S && (rc = r2l_ert_advance(raw, z, dd, cr, S, s0, s1, trans, stream))) return rc;
        }
        return 0;
    }
    if (grid == nullptr) return r2l_teacher_mlp_cfg(o, dd, v, z, wstream, tparams, raw, cr, S, stream, cfg);
    if ((rc = r2l_occ_index(grid, o, dd, z, cr, S, idx, count, work + ow.iwork, stream))) return rc;
    if (occ->live_acc != nullptr && (rc = r2l_occ_live_add(count, cr * (int64_t)S, occ->live_acc, stream))) return rc;
    return r2l_teacher_mlp_live_cfg(o, dd, v, z, idx, count, wstream, tparams, raw, cr, S, stream, cfg);
}

int frames_body(const char* who, const float* c2w_dev, const float* focal_dev, int K, const r2l_teacher_frame_desc* d, const float* ttab,
                const float* u_det, const float* wstream_coarse, const float* tparams_coarse, const float* wstream_fine,
                const float* tparams_fine, float* rows, float* rgb, float* disp, float* acc, float* depth, float* rgb0, float* work,
                void* stream, const r2l_config* cfg, const FrameOcc* occ) {
    if (const char* why = desc_check(d)) {
        r2l_set_error_msg(why);
        return (int)hipErrorInvalidValue;
    }
    R2L_CFG_ENTER(cfg);
    FRAMES_REQUIRE(K >= 0, "K is negative");
    FRAMES_REQUIRE((wstream_fine == nullptr) == (tparams_fine == nullptr),
                "wstream_fine / tparams_fine: both or neither (NULL pair: the coarse net serves both passes)");
    FRAMES_REQUIRE(d->perturb != 0 || d->N_importance == 0 || u_det != nullptr,
                "u_det is NULL (needed with perturb == 0 and N_importance > 0)");
    FRAMES_REQUIRE(focal_dev != nullptr || d->focal > 0.f, "need r2l_teacher_frame_desc.focal > 0 (or focal_dev)");
    if (K == 0) return 0;
    FRAMES_REQUIRE(c2w_dev && ttab && wstream_coarse && tparams_coarse && work,
                "a required pointer is NULL (c2w_dev, ttab, wstream_coarse, tparams_coarse, work)");
    FRAMES_REQUIRE(((uintptr_t)work & 15) == 0, "work must be 16-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    const int S = d->N_samples, NI = d->N_importance, T = S + NI;
    const int64_t hw = (int64_t)d->H * d->W;
    const int64_t cr_max = d->chunk_rays > 0 && d->chunk_rays < hw ? d->chunk_rays : hw;
    const FrameWork w = frame_work(d);
    const OccWork ow = occ_work(d, w);  // (read by the occupancy form only)
    float* const nf = work + w.nearfar;
    float *const o = work + w.o, *const dd = work + w.d, *const v = work + w.v, *const z = work + w.z, *const raw = work + w.raw;
    const float* wfine = wstream_fine ? wstream_fine : wstream_coarse;
    const float* pfine = tparams_fine ? tparams_fine : tparams_coarse;
    int rc;
    for (int k = 0; k < K; ++k) {
        const uint64_t fid = d->frame_id0 + (uint64_t)k;
        for (int64_t r0 = 0; r0 < hw; r0 += cr_max) {
            const int64_t cr = hw - r0 < cr_max ? hw - r0 : cr_max;
            const int64_t g = (int64_t)k * hw + r0;  // first ray of this pass among the K*H*W
            // final outputs of this pass: the caller's arrays, or stand-ins in the work buffer
            float* f_rgb = rgb ? rgb + g * 3 : work + w.rgb_f;
            float* f_disp = disp ? disp + g : work + w.s_f;
            float* f_acc = acc ? acc + g : work + w.s_f + r4(cr_max);
            float* f_depth = depth ? depth + g : work + w.s_f + 2 * r4(cr_max);
            if ((rc = launch_rays(c2w_dev, focal_dev, d->focal, d->H, d->W, g, cr, o, dd, v, rows ? rows + g * 9 : nullptr, nf, d->near,
                                  d->far, st, d->ndc == 1, d->focal)))
                return rc;
            float* t_rand = nullptr;
            if (d->perturb) {
                t_rand = work + w.trand;
                if ((rc = launch_draw(t_rand, cr * S, r0 * S, d->seed, 2 * fid, st))) return rc;
            }
            if ((rc = r2l_stratified_z(nf, nf + 1, 0, ttab, t_rand, z, cr, S, stream))) return rc;
            if ((rc = frames_mlp(o, dd, v, z, wstream_coarse, tparams_coarse, raw, cr, S, stream, cfg, occ ? occ->coarse : nullptr, occ, work,
                                 ow, NI == 0)))
                return rc;
            if (NI == 0) {
                if ((rc = r2l_raw2outputs(raw, z, dd, nullptr, d->white_bkgd, f_rgb, f_disp, f_acc, nullptr, f_depth, cr, S, stream)))
                    return rc;
            } else {
                float* c_rgb = rgb0 ? rgb0 + g * 3 : work + w.rgb_c;
                float* c_s = work + w.s_c;
                if ((rc = r2l_raw2outputs(raw, z, dd, nullptr, d->white_bkgd, c_rgb, c_s, c_s + r4(cr_max), work + w.wts,
                                          c_s + 2 * r4(cr_max), cr, S, stream)))
                    return rc;
                const float* u = u_det;
                if (d->perturb) {
                    if ((rc = launch_draw(work + w.u, cr * NI, r0 * NI, d->seed, 2 * fid + 1, st))) return rc;
                    u = work + w.u;
                }
                if ((rc = r2l_sample_pdf_sort(z, work + w.wts, u, d->perturb ? NI : 0, work + w.zs, work + w.zall, nullptr, cr, S, NI,
                                              stream)))
                    return rc;
                if ((rc = frames_mlp(o, dd, v, work + w.zall, wfine, pfine, raw, cr, T, stream, cfg, occ ? occ->fine : nullptr, occ, work,
                                     ow, true)))
                    return rc;
                if ((rc = r2l_raw2outputs(raw, work + w.zall, dd, nullptr, d->white_bkgd, f_rgb, f_disp, f_acc, nullptr, f_depth, cr, T,
                                          stream)))
                    return rc;
            }
            if (rows != nullptr) {
                hipLaunchKernelGGL(r2l_rows_rgb_kernel, dim3(grid_for(cr * 3)), dim3(256), 0, st, f_rgb, rows + g * 9, cr);
                R2L_CHECK(hipGetLastError());
            }
        }
    }
    return 0;
}

}  // namespace
