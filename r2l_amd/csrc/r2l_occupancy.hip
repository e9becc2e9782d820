// Occupancy grid of the teacher's render: a bit per cell of a box says whether the trained density can be positive there, and
// the sample points of a launch that fall into an empty cell are dropped before the point network sees them (raw2outputs gives
// a sample with sigma <= 0 the weight 0 exactly, so a dropped sample whose sigma is not positive changes no bit of a frame).
// Stateless calls (include/r2l_hip.h "occupancy grid" pins the arithmetic):
//   r2l_occ_build    sigma of (G k)^3 probes through the EXISTING point-network launch (r2l_teacher_mlp_cfg, S = 1), slab by
//                    slab, a cell's bit = any of its k^3 probes above the threshold, then a box maximum (dilation);
//   r2l_occ_compact  the live samples of [R,S] in ascending order: their index and their (o, d, viewdirs, z) as S = 1 rows;
//   r2l_occ_scatter  raw of the live rows back into a zero-filled [R,S,4];
//   r2l_occ_index    r2l_occ_compact's idx and count without its row copies (the same kernels, a template switch), for the point
//                    network's live form (r2l_teacher_mlp_live_cfg), which reads the count on the device; r2l_occ_live_add sums
//                    counts in stream order;
//   r2l_occ_index_seg  r2l_occ_index over one segment of consecutive sample numbers of every ray, without the rays whose transmittance
//                    is below eps, the grid optional (one more template switch of the same kernels);
//   r2l_occ_rays     the rays that meet an occupied cell at any of T depths (a light-field student can leave out whole rays only):
//                    flag + count per 2048 rays, the scan of r2l_occ_index, placement; r2l_rays_gather and r2l_rgb_scatter_bg are the
//                    two small kernels of a culled frame (include/r2l_hip.h "whole rays");
//   r2l_ert_advance  a ray's transmittance through a segment, from the raw the point network has written (early ray termination,
//                    include/r2l_hip.h "early ray termination").
// No kernel of the point network is touched here.  Nothing here is compute-bound: build is the network's time, compact and scatter
// move 40 + 8 and 32 bytes per live sample.  Every output position comes from a scan, never from the arrival order of an
// atomic (there are no atomics in this file): the same arguments give the same bits.
#include "r2l_common.h"
#include "r2l_dispatch.h"

namespace {

struct OccGrid {  // r2l_occ_grid by value, as the kernels take it
    const uint32_t* bits;
    int G;
    float lo[3], inv[3];
};

// live = outside the box, or the cell's bit.  c = floorf((p - lo) * inv), difference and product rounded separately (the
// library is built without contraction); NaN and +-inf compare false on both sides: outside.
__device__ __forceinline__ bool occ_live(const OccGrid& g, float px, float py, float pz) {
    const float fx = floorf((px - g.lo[0]) * g.inv[0]);
    const float fy = floorf((py - g.lo[1]) * g.inv[1]);
    const float fz = floorf((pz - g.lo[2]) * g.inv[2]);
    const float fG = (float)g.G;
    const bool inside = fx >= 0.f && fx < fG && fy >= 0.f && fy < fG && fz >= 0.f && fz < fG;
    if (!inside) return true;
    const int i = ((int)fz * g.G + (int)fy) * g.G + (int)fx;  // < 512^3 = 2^27
    return (g.bits[i >> 5] >> (i & 31)) & 1u;
}

// ---- build ------------------------------------------------------------------------------------------------------------------
// A slab is a run of whole cells [c0, c0 + nc), c0 a multiple of 64; its probes are laid out cell-major (point (c - c0) k^3 + s,
// s = (jz k + jy) k + jx), so that one thread owns a cell and a wave's ballot is two words of bits.
constexpr int64_t OCC_SLAB_PROBES = (int64_t)1 << 18;
constexpr int OCC_THREADS = 256;

int64_t occ_slab_cells(int G, int k) {
    const int64_t ncell = (int64_t)G * G * G, k3 = (int64_t)k * k * k;
    const int64_t all = (ncell + 63) / 64 * 64;
    int64_t c = OCC_SLAB_PROBES / k3 / 64 * 64;
    if (c < 64) c = 64;
    return c < all ? c : all;
}
int64_t occ_words(int G) { return ((int64_t)G * G * G + 31) / 32; }

unsigned occ_blocks(int64_t n, int per_block) {
    int64_t b = (n + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

// the S = 1 rows of the slab's probes: o = probe, d = 0, viewdirs = (0, 0, 1), z = 0
__global__ __launch_bounds__(OCC_THREADS) void r2l_occ_probe_kernel(int G, int k, float lo0, float lo1, float lo2, float st0, float st1,
                                                                    float st2, int64_t c0, int64_t n_pts, float* __restrict__ o,
                                                                    float* __restrict__ d, float* __restrict__ v, float* __restrict__ z) {
    const int k3 = k * k * k;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_pts; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t cell = c0 + j / k3;
        const int s = (int)(j % k3);
        const int cx = (int)(cell % G), cy = (int)((cell / G) % G), cz = (int)(cell / ((int64_t)G * G));
        const int jx = s % k, jy = (s / k) % k, jz = s / (k * k);
        o[3 * j + 0] = lo0 + ((float)(cx * k + jx) + 0.5f) * st0;
        o[3 * j + 1] = lo1 + ((float)(cy * k + jy) + 0.5f) * st1;
        o[3 * j + 2] = lo2 + ((float)(cz * k + jz) + 0.5f) * st2;
        d[3 * j + 0] = 0.f;
        d[3 * j + 1] = 0.f;
        d[3 * j + 2] = 0.f;
        v[3 * j + 0] = 0.f;
        v[3 * j + 1] = 0.f;
        v[3 * j + 2] = 1.f;
        z[j] = 0.f;
    }
}

// one thread per cell of the slab (whole waves: nc_pad is a multiple of 64): bit = any sigma > thresh; sigma_out in probe order
__global__ __launch_bounds__(OCC_THREADS) void r2l_occ_mark_kernel(int G, int k, float thresh, int64_t c0, int64_t nc_pad, int64_t ncell,
                                                                   int64_t words, const float* __restrict__ raw,
                                                                   uint32_t* __restrict__ bits, float* __restrict__ sigma_out) {
    const int k3 = k * k * k;
    const int64_t Gk = (int64_t)G * k;
    const int lane = threadIdx.x & 63;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nc_pad; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t cell = c0 + j;
        bool occ = false;
        if (cell < ncell) {
            const int cx = (int)(cell % G), cy = (int)((cell / G) % G), cz = (int)(cell / ((int64_t)G * G));
            for (int s = 0; s < k3; ++s) {
                const float sg = raw[(j * k3 + s) * 4 + 3];
                occ = occ || sg > thresh;
                if (sigma_out != nullptr) {
                    const int jx = s % k, jy = (s / k) % k, jz = s / (k * k);
                    sigma_out[((int64_t)(cz * k + jz) * Gk + (cy * k + jy)) * Gk + (cx * k + jx)] = sg;
                }
            }
        }
        const unsigned long long m = __ballot(occ);
        const int64_t w = (cell >> 5);  // lane 0 / lane 32 hold the first cell of a word
        if (lane == 0 && w < words) bits[w] = (uint32_t)m;
        if (lane == 32 && w < words) bits[w] = (uint32_t)(m >> 32);
    }
}

// box maximum along one axis (stride 1, G or G^2 cells), clipped at the faces; the three passes make the (2 dil + 1)^3 box
__global__ __launch_bounds__(OCC_THREADS) void r2l_occ_dilate_kernel(int G, int dil, int axis, int64_t ncell, int64_t words,
                                                                     const uint32_t* __restrict__ src, uint32_t* __restrict__ dst) {
    const int64_t n_pad = (ncell + 63) / 64 * 64;
    const int lane = threadIdx.x & 63;
    const int64_t stride = axis == 0 ? 1 : (axis == 1 ? G : (int64_t)G * G);
    for (int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; cell < n_pad; cell += (int64_t)gridDim.x * blockDim.x) {
        bool occ = false;
        if (cell < ncell) {
            const int c = (int)((cell / stride) % G);
            const int a = c - dil < 0 ? 0 : c - dil, b = c + dil > G - 1 ? G - 1 : c + dil;
            for (int q = a; q <= b && !occ; ++q) {
                const int64_t i = cell + (int64_t)(q - c) * stride;
                occ = (src[i >> 5] >> (i & 31)) & 1u;
            }
        }
        const unsigned long long m = __ballot(occ);
        const int64_t w = cell >> 5;
        if (lane == 0 && w < words) dst[w] = (uint32_t)m;
        if (lane == 32 && w < words) dst[w] = (uint32_t)(m >> 32);
    }
}

// ---- compact ----------------------------------------------------------------------------------------------------------------
// Workgroup b owns the samples [b * 2048, (b + 1) * 2048), 256 at a time.  Launch 1 counts its live samples, launch 2 (one
// workgroup) turns the counts into exclusive offsets and writes the total, launch 3 evaluates the same predicate again and
// places every live sample at offset + (live samples before it in the workgroup): ascending n by construction.
constexpr int OCC_CHUNK = 2048;
constexpr int OCC_ROUNDS = OCC_CHUNK / OCC_THREADS;
constexpr int OCC_SCAN_THREADS = 1024;

struct CompactArgs {
    OccGrid g;
    const float *o, *d, *v, *z;
    int64_t n;  // R * S
    int S;
    unsigned* blk;  // [number of workgroups]: counts, then exclusive offsets
    float *out_o, *out_d, *out_v, *out_z;
    int64_t* idx;
    // SEG only (r2l_occ_index_seg): the samples s0 <= s < s0 + W of every ray; n is then R * W, and g.bits may be NULL (no grid)
    int s0, W;
    const float* trans;  // [R] or NULL: a ray with trans < eps has no live sample
    float eps;
};

// ROWS: the (o, d, viewdirs, z) row copies of r2l_occ_compact; without them the placement writes idx alone (r2l_occ_index)
// SEG: the enumeration runs over a segment of every ray (m -> ray m / W, sample s0 + m % W: ascending in n = ray * S + s), the grid
//      is optional and a terminated ray drops out (r2l_occ_index_seg); the other instantiations compile from the code they had
template <bool EMIT, bool ROWS = true, bool SEG = false>
__global__ __launch_bounds__(OCC_THREADS) void r2l_occ_compact_kernel(const CompactArgs a) {
    static_assert(!(SEG && ROWS), "the segment form writes idx alone");
    __shared__ unsigned wsum[OCC_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t base = (int64_t)blockIdx.x * OCC_CHUNK;
    unsigned running = EMIT ? a.blk[blockIdx.x] : 0u;
#pragma unroll 1
    for (int r = 0; r < OCC_ROUNDS; ++r) {
        int64_t n = base + r * OCC_THREADS + t;
        bool live = false;
        int64_t ray = 0;
        float zz = 0.f;
        if (n < a.n) {
            if constexpr (SEG) {
                ray = n / a.W;
                n = ray * a.S + a.s0 + (n - ray * a.W);  // < R * S < 2^31
                live = !(a.trans != nullptr && a.trans[ray] < a.eps);  // (a NaN transmittance keeps the ray)
            } else {
                ray = n / a.S;
                live = true;
            }
            if (!SEG || (live && a.g.bits != nullptr)) {
                zz = a.z[n];
                // the point exactly as r2l_teacher_mlp_kernel forms it: product and sum rounded separately
                const float px = a.o[ray * 3 + 0] + a.d[ray * 3 + 0] * zz;
                const float py = a.o[ray * 3 + 1] + a.d[ray * 3 + 1] * zz;
                const float pz = a.o[ray * 3 + 2] + a.d[ray * 3 + 2] * zz;
                live = occ_live(a.g, px, py, pz);
            }
        }
        const unsigned long long m = __ballot(live);
        if (!EMIT) {
            running += (unsigned)__popcll(m);  // (every lane of the wave carries the wave's count)
        } else {
            if (lane == 0) wsum[w] = (unsigned)__popcll(m);
            __syncthreads();
            unsigned before = 0, total = 0;
#pragma unroll
            for (int j = 0; j < OCC_THREADS / 64; ++j) {
                const unsigned c = wsum[j];
                if (j < w) before += c;
                total += c;
            }
            if (live) {
                const int64_t pos = (int64_t)running + before + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
                a.idx[pos] = n;
                if constexpr (ROWS) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        a.out_o[pos * 3 + c] = a.o[ray * 3 + c];
                        a.out_d[pos * 3 + c] = a.d[ray * 3 + c];
                        a.out_v[pos * 3 + c] = a.v[ray * 3 + c];
                    }
                    a.out_z[pos] = zz;
                }
            }
            running += total;
            __syncthreads();
        }
    }
    if (!EMIT) {
        if (lane == 0) wsum[w] = running;
        __syncthreads();
        if (t == 0) {
            unsigned s = 0;
            for (int j = 0; j < OCC_THREADS / 64; ++j) s += wsum[j];
            a.blk[blockIdx.x] = s;
        }
    }
}

// counts -> exclusive offsets in place, total -> *count_out.  One workgroup; thread t owns the run [t * per, (t + 1) * per).
__global__ __launch_bounds__(OCC_SCAN_THREADS) void r2l_occ_scan_kernel(unsigned* __restrict__ blk, int64_t nb, int64_t per,
                                                                        int64_t* __restrict__ count_out) {
    __shared__ unsigned wtot[OCC_SCAN_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    int64_t lo = (int64_t)t * per, hi = lo + per;
    lo = lo < nb ? lo : nb;
    hi = hi < nb ? hi : nb;
    unsigned mine = 0;
    for (int64_t i = lo; i < hi; ++i) mine += blk[i];
    unsigned s = mine;  // inclusive scan over the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned u = __shfl_up(s, off);
        if (lane >= off) s += u;
    }
    if (lane == 63) wtot[w] = s;
    __syncthreads();
    unsigned before = 0, total = 0;
    for (int j = 0; j < OCC_SCAN_THREADS / 64; ++j) {
        const unsigned c = wtot[j];
        if (j < w) before += c;
        total += c;
    }
    unsigned run = before + s - mine;
    for (int64_t i = lo; i < hi; ++i) {
        const unsigned c = blk[i];
        blk[i] = run;
        run += c;
    }
    if (t == 0) *count_out = (int64_t)total;
}

// live_acc[0] += *count, live_acc[1] += total: one thread, ordered by the stream behind the scan that wrote *count (no atomics)
__global__ void r2l_occ_live_add_kernel(const int64_t* __restrict__ count, int64_t total, int64_t* __restrict__ live_acc) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        live_acc[0] += *count;
        live_acc[1] += total;
    }
}

// ---- whole rays: does a ray meet an occupied cell? (r2l_occ_rays) -------------------------------------------------------------------
// A ray is live iff any of its T points o + d * t_j, t_j = near + ((float)j + 0.5f) * dt, is live by occ_live.  A sub-wave of
// RAY_LANES lanes owns a ray: lane l tests the depths l, l + RAY_LANES, ... and the sub-wave stops at the first round with a hit
// (the loop itself is wave-uniform: it ends when every sub-wave of the wave is done).  The lanes of a sub-wave read the same o and
// d (one address: a broadcast); the grid's bits are read where the points fall — 256 KB at 128^3, resident in L2, no LDS copy.
// Workgroup b owns the rays [b * 2048, (b + 1) * 2048), as the sample kernels above own samples: launch 1 writes a flag byte per ray
// and the workgroup's count, launch 2 is r2l_occ_scan_kernel, launch 3 places the flagged rays behind the offset (ascending r).
constexpr int RAY_LANES = 16;
constexpr int RAY_THREADS = 1024;
constexpr int RAY_PER_PASS = RAY_THREADS / RAY_LANES;  // 64 rays a pass, 32 passes a workgroup

__global__ __launch_bounds__(RAY_THREADS) void r2l_occ_rays_flag_kernel(const OccGrid g, const float* __restrict__ o,
                                                                        const float* __restrict__ d, int64_t R, float near, float dt, int T,
                                                                        uint8_t* __restrict__ flags, unsigned* __restrict__ blk) {
    __shared__ unsigned wsum[RAY_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, sub = t & (RAY_LANES - 1);
    const int shift = lane & ~(RAY_LANES - 1);  // where the sub-wave's bits sit in a ballot
    const int64_t base = (int64_t)blockIdx.x * OCC_CHUNK;
    unsigned running = 0;
#pragma unroll 1
    for (int pass = 0; pass < OCC_CHUNK / RAY_PER_PASS; ++pass) {
        const int64_t r = base + pass * RAY_PER_PASS + (t >> 4);
        const bool have = r < R;
        float ox = 0.f, oy = 0.f, oz = 0.f, dx = 0.f, dy = 0.f, dz = 0.f;
        if (have) {
            ox = o[r * 3 + 0]; oy = o[r * 3 + 1]; oz = o[r * 3 + 2];
            dx = d[r * 3 + 0]; dy = d[r * 3 + 1]; dz = d[r * 3 + 2];
        }
        bool done = !have, hit = false;
#pragma unroll 1
        for (int j0 = 0; j0 < T; j0 += RAY_LANES) {
            const int j = j0 + sub;
            bool live = false;
            if (!done && j < T) {
                const float tj = near + ((float)j + 0.5f) * dt;  // (no contraction: product and sum rounded separately)
                live = occ_live(g, ox + dx * tj, oy + dy * tj, oz + dz * tj);  // the point as r2l_occ_index forms it
            }
            const unsigned long long m = __ballot(live);
            if ((m >> shift) & ((1ull << RAY_LANES) - 1ull)) hit = done = true;
            if (__ballot(!done) == 0ull) break;  // (uniform over the wave)
        }
        const bool mine = have && sub == 0;
        if (mine) flags[r] = hit ? 1 : 0;
        running += (unsigned)__popcll(__ballot(mine && hit));  // (every lane carries the wave's count)
    }
    if (lane == 0) wsum[w] = running;
    __syncthreads();
    if (t == 0) {
        unsigned s = 0;
        for (int j = 0; j < RAY_THREADS / 64; ++j) s += wsum[j];
        blk[blockIdx.x] = s;
    }
}

// the placement of r2l_occ_compact_kernel<true> with the predicate read from the flags
__global__ __launch_bounds__(OCC_THREADS) void r2l_occ_rays_place_kernel(const uint8_t* __restrict__ flags, int64_t R,
                                                                         const unsigned* __restrict__ blk, int64_t* __restrict__ idx) {
    __shared__ unsigned wsum[OCC_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t base = (int64_t)blockIdx.x * OCC_CHUNK;
    unsigned running = blk[blockIdx.x];
#pragma unroll 1
    for (int r = 0; r < OCC_ROUNDS; ++r) {
        const int64_t n = base + r * OCC_THREADS + t;
        const bool live = n < R && flags[n] != 0;
        const unsigned long long m = __ballot(live);
        if (lane == 0) wsum[w] = (unsigned)__popcll(m);
        __syncthreads();
        unsigned before = 0, total = 0;
#pragma unroll
        for (int j = 0; j < OCC_THREADS / 64; ++j) {
            const unsigned c = wsum[j];
            if (j < w) before += c;
            total += c;
        }
        if (live) idx[(int64_t)running + before + (unsigned)__popcll(m & ((1ull << lane) - 1ull))] = n;
        running += total;
        __syncthreads();
    }
}

// out row i = row idx[i] of rays_o / rays_d; an index outside [0, R) gives a NaN row and reads nothing
__global__ __launch_bounds__(OCC_THREADS) void r2l_rays_gather_kernel(const float* __restrict__ o, const float* __restrict__ d, int64_t R,
                                                                      const int64_t* __restrict__ idx, int64_t M, float* __restrict__ out_o,
                                                                      float* __restrict__ out_d) {
    const float nan = __int_as_float(0x7fc00000);
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < M * 3; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = e / 3, n = idx[i];
        const int c = (int)(e - i * 3);
        const bool ok = n >= 0 && n < R;
        out_o[e] = ok ? o[n * 3 + c] : nan;
        out_d[e] = ok ? d[n * 3 + c] : nan;
    }
}

// thread r: a dead ray's row = bg; and, as thread i = r < M, row idx[i] = rgb_live[i].  idx lists exactly the rays with live != 0
// (one r2l_occ_rays call made both), so no row is written twice
__global__ __launch_bounds__(OCC_THREADS) void r2l_rgb_scatter_bg_kernel(const float* __restrict__ rgb_live, const int64_t* __restrict__ idx,
                                                                         int64_t M, const uint8_t* __restrict__ live, float bg,
                                                                         float* __restrict__ out, int64_t R) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < R; r += (int64_t)gridDim.x * blockDim.x) {
        if (live[r] == 0) {
            out[r * 3 + 0] = bg;
            out[r * 3 + 1] = bg;
            out[r * 3 + 2] = bg;
        }
        if (r < M) {
            const int64_t n = idx[r];
            if (n >= 0 && n < R) {
                out[n * 3 + 0] = rgb_live[r * 3 + 0];
                out[n * 3 + 1] = rgb_live[r * 3 + 1];
                out[n * 3 + 2] = rgb_live[r * 3 + 2];
            }
        }
    }
}

// ---- early ray termination: the transmittance through a segment ----------------------------------------------------------------
// trans[r] = (s0 == 0 ? 1 : trans[r]) * prod over s0 <= s < s1, in ascending s, of f_s = (1 - alpha_s) + 1e-10, alpha_s by the
// per-sample expressions of r2l_raw2outputs without noise.  A workgroup owns ERT_RAYS rays.  Phase 1: all 256 threads form the
// ERT_RAYS * W factors, consecutive threads taking consecutive samples of a ray (sigma is every fourth float of raw: a wave's loads
// cover one contiguous span instead of one line per ray), into an LDS tile whose odd row stride keeps phase 2 off one bank.
// Phase 2: thread r multiplies row r front to back — the pinned order, one rounding per product.
constexpr int ERT_RAYS = 32;
constexpr int ERT_MAX_S = 256;
constexpr int ERT_STRIDE = ERT_MAX_S + 1;

__global__ __launch_bounds__(OCC_THREADS) void r2l_ert_advance_kernel(const float* __restrict__ raw, const float* __restrict__ z,
                                                                      const float* __restrict__ rays_d, int64_t R, int S, int s0, int W,
                                                                      float* __restrict__ trans) {
    __shared__ float f[ERT_RAYS * ERT_STRIDE];
    const int t = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * ERT_RAYS;
    const int rays = R - r0 < ERT_RAYS ? (int)(R - r0) : ERT_RAYS;
    for (int e = t; e < rays * W; e += OCC_THREADS) {
        const int rl = e / W, sl = e - rl * W, s = s0 + sl;
        const int64_t ray = r0 + rl, n = ray * S + s;
        const float d0 = rays_d[ray * 3 + 0], d1 = rays_d[ray * 3 + 1], d2 = rays_d[ray * 3 + 2];
        const float dn = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);  // the association of r2l_raw2outputs
        float dist = (s + 1 < S) ? z[n + 1] - z[n] : 1e10f;
        dist = dist * dn;
        const float al = 1.0f - __expf(-fmaxf(raw[n * 4 + 3], 0.f) * dist);
        f[rl * ERT_STRIDE + sl] = (1.0f - al) + 1e-10f;
    }
    __syncthreads();
    if (t < rays) {
        float T = s0 == 0 ? 1.0f : trans[r0 + t];
        for (int sl = 0; sl < W; ++sl) T = T * f[t * ERT_STRIDE + sl];
        trans[r0 + t] = T;
    }
}

// ---- scatter ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OCC_THREADS) void r2l_occ_scatter_kernel(const float4* __restrict__ raw_live, const int64_t* __restrict__ idx,
                                                                      int64_t M, float4* __restrict__ raw_out, int64_t n_out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t n = idx[i];
        if (n >= 0 && n < n_out) raw_out[n] = raw_live[i];  // (an index out of range writes nothing)
    }
}

// what is wrong with a grid, or nullptr
const char* occ_grid_check(const r2l_occ_grid* g, const char* null_msg) {
    if (g == nullptr) return null_msg;
    if (g->bits == nullptr) return "r2l_occ_grid.bits is NULL";
    if (g->G < 1 || g->G > 512) return "r2l_occ_grid.G: need 1 <= G <= 512";
    for (int a = 0; a < 3; ++a) {
        if (!(g->lo[a] - g->lo[a] == 0.f)) return "r2l_occ_grid.lo: not finite";
        if (!(g->inv[a] > 0.f) || !(g->inv[a] - g->inv[a] == 0.f)) return "r2l_occ_grid.inv: need a positive finite value (lo < hi)";
        if (!(g->step[a] > 0.f) || !(g->step[a] - g->step[a] == 0.f)) return "r2l_occ_grid.step: need a positive finite value (lo < hi)";
    }
    if (g->reserved[0] || g->reserved[1]) return "r2l_occ_grid.reserved: must be 0";
    return nullptr;
}

OccGrid occ_dev(const r2l_occ_grid* g) {
    OccGrid d;
    d.bits = g->bits;
    d.G = g->G;
    for (int a = 0; a < 3; ++a) {
        d.lo[a] = g->lo[a];
        d.inv[a] = g->inv[a];
    }
    return d;
}

}  // namespace

extern "C" int r2l_occ_grid_init(r2l_occ_grid* grid, uint32_t* bits, int G, int k, const float* lo, const float* hi) {
    R2L_REQUIRE(grid != nullptr, "r2l_occ_grid_init: grid is NULL");
    R2L_REQUIRE(bits != nullptr, "r2l_occ_grid_init: bits is NULL");
    R2L_REQUIRE(lo != nullptr, "r2l_occ_grid_init: lo is NULL");
    R2L_REQUIRE(hi != nullptr, "r2l_occ_grid_init: hi is NULL");
    R2L_REQUIRE(G >= 1 && G <= 512, "r2l_occ_grid_init: G: need 1 <= G <= 512");
    R2L_REQUIRE(k >= 1 && k <= 4, "r2l_occ_grid_init: k: need 1 <= k <= 4");
    for (int a = 0; a < 3; ++a) {
        R2L_REQUIRE(lo[a] - lo[a] == 0.f && hi[a] - hi[a] == 0.f, "r2l_occ_grid_init: lo / hi: not finite");
        R2L_REQUIRE(lo[a] < hi[a], "r2l_occ_grid_init: lo / hi: need lo[a] < hi[a] on every axis");
    }
    r2l_occ_grid g{};
    g.bits = bits;
    g.G = G;
    for (int a = 0; a < 3; ++a) {
        const float side = hi[a] - lo[a];
        g.lo[a] = lo[a];
        g.inv[a] = (float)G / side;
        g.step[a] = side / (float)(G * k);
        R2L_REQUIRE(side - side == 0.f && g.inv[a] - g.inv[a] == 0.f && g.step[a] > 0.f,
                    "r2l_occ_grid_init: lo / hi: the side of the box is out of fp32 range");
    }
    *grid = g;
    return 0;
}

extern "C" int64_t r2l_occ_bits_words(int G) {
    if (G < 1 || G > 512) {
        r2l_set_error_msg("r2l_occ_bits_words: G: need 1 <= G <= 512");
        return -1;
    }
    return occ_words(G);
}

extern "C" int64_t r2l_occ_build_work_floats(int G, int k) {
    if (G < 1 || G > 512 || k < 1 || k > 4) {
        r2l_set_error_msg("r2l_occ_build_work_floats: need 1 <= G <= 512 and 1 <= k <= 4");
        return -1;
    }
    const int64_t P = occ_slab_cells(G, k) * k * k * k;                // probes of a slab: a multiple of 64
    return 14 * P + 2 * ((occ_words(G) + 3) / 4 * 4);                  // o, d, viewdirs [P,3], z [P], raw [P,4]; two bit planes
}

extern "C" int r2l_occ_build(r2l_occ_grid* grid, int k, int dilate, float sigma_thresh, const float* wstream, const float* tparams,
                             const r2l_config* cfg, float* work, float* sigma_out, void* stream) {
    R2L_CFG_ENTER(cfg);
    if (const char* why = occ_grid_check(grid, "r2l_occ_build: grid is NULL")) {
        r2l_set_error_msg(why);
        return (int)hipErrorInvalidValue;
    }
    R2L_REQUIRE(k >= 1 && k <= 4, "r2l_occ_build: k: need 1 <= k <= 4");
    R2L_REQUIRE(dilate >= 0, "r2l_occ_build: dilate is negative");
    R2L_REQUIRE(sigma_thresh == sigma_thresh, "r2l_occ_build: sigma_thresh is NaN");
    R2L_REQUIRE(wstream != nullptr, "r2l_occ_build: wstream is NULL");
    R2L_REQUIRE(tparams != nullptr, "r2l_occ_build: tparams is NULL");
    R2L_REQUIRE(work != nullptr, "r2l_occ_build: work is NULL");
    R2L_REQUIRE(((uintptr_t)work & 15) == 0, "r2l_occ_build: work is not 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int G = grid->G, k3 = k * k * k;
    const int64_t ncell = (int64_t)G * G * G, words = occ_words(G), slab = occ_slab_cells(G, k), P = slab * k3;
    float *o = work, *d = o + 3 * P, *v = d + 3 * P, *z = v + 3 * P, *raw = z + P;
    uint32_t* plane0 = reinterpret_cast<uint32_t*>(raw + 4 * P);
    uint32_t* plane1 = plane0 + (words + 3) / 4 * 4;
    const int dil = dilate > G - 1 ? G - 1 : dilate;  // (a wider box is clipped to the same cells)
    uint32_t* marked = dil > 0 ? plane0 : grid->bits;
    for (int64_t c0 = 0; c0 < ncell; c0 += slab) {
        const int64_t nc = ncell - c0 < slab ? ncell - c0 : slab, n_pts = nc * k3, nc_pad = (nc + 63) / 64 * 64;
        hipLaunchKernelGGL(r2l_occ_probe_kernel, dim3(occ_blocks(n_pts, OCC_THREADS)), dim3(OCC_THREADS), 0, s, G, k, grid->lo[0],
                           grid->lo[1], grid->lo[2], grid->step[0], grid->step[1], grid->step[2], c0, n_pts, o, d, v, z);
        R2L_CHECK(hipGetLastError());
        const int rc = r2l_teacher_mlp_cfg(o, d, v, z, wstream, tparams, raw, n_pts, 1, stream, cfg);
        if (rc) return rc;
        hipLaunchKernelGGL(r2l_occ_mark_kernel, dim3(occ_blocks(nc_pad, OCC_THREADS)), dim3(OCC_THREADS), 0, s, G, k, sigma_thresh, c0,
                           nc_pad, ncell, words, raw, marked, sigma_out);
        R2L_CHECK(hipGetLastError());
    }
    if (dil > 0) {
        const unsigned nb = occ_blocks((ncell + 63) / 64 * 64, OCC_THREADS);
        uint32_t* const src[3] = {plane0, plane1, plane0};
        uint32_t* const dst[3] = {plane1, plane0, grid->bits};
        for (int axis = 0; axis < 3; ++axis) {
            hipLaunchKernelGGL(r2l_occ_dilate_kernel, dim3(nb), dim3(OCC_THREADS), 0, s, G, dil, axis, ncell, words, src[axis], dst[axis]);
            R2L_CHECK(hipGetLastError());
        }
    }
    return 0;
}

extern "C" int64_t r2l_occ_compact_work_bytes(int64_t n) {
    if (n < 0 || n >= ((int64_t)1 << 31)) {
        r2l_set_error_msg("r2l_occ_compact_work_bytes: need 0 <= R*S < 2^31");
        return -1;
    }
    const int64_t nb = (n + OCC_CHUNK - 1) / OCC_CHUNK;
    return ((nb < 1 ? 1 : nb) * (int64_t)sizeof(unsigned) + 15) / 16 * 16;
}

extern "C" int r2l_occ_compact(const r2l_occ_grid* grid, const float* rays_o, const float* rays_d, const float* viewdirs, const float* z,
                               int64_t R, int S, float* out_o, float* out_d, float* out_v, float* out_z, int64_t* idx_out,
                               int64_t* count_out, void* work, void* stream) {
    if (const char* why = occ_grid_check(grid, "r2l_occ_compact: grid is NULL")) {
        r2l_set_error_msg(why);
        return (int)hipErrorInvalidValue;
    }
    R2L_REQUIRE(R >= 0, "r2l_occ_compact: R is negative");
    R2L_REQUIRE(S >= 1, "r2l_occ_compact: S: need S >= 1");
    R2L_REQUIRE(R < ((int64_t)1 << 31) && R * (int64_t)S < ((int64_t)1 << 31), "r2l_occ_compact: R*S: need R*S < 2^31");
    R2L_REQUIRE(count_out != nullptr, "r2l_occ_compact: count_out is NULL");
    hipStream_t s = (hipStream_t)stream;
    if (R == 0) {
        R2L_CHECK(hipMemsetAsync(count_out, 0, sizeof(int64_t), s));
        return 0;
    }
    R2L_REQUIRE(rays_o != nullptr, "r2l_occ_compact: rays_o is NULL");
    R2L_REQUIRE(rays_d != nullptr, "r2l_occ_compact: rays_d is NULL");
    R2L_REQUIRE(viewdirs != nullptr, "r2l_occ_compact: viewdirs is NULL");
    R2L_REQUIRE(z != nullptr, "r2l_occ_compact: z is NULL");
    R2L_REQUIRE(out_o != nullptr, "r2l_occ_compact: out_o is NULL");
    R2L_REQUIRE(out_d != nullptr, "r2l_occ_compact: out_d is NULL");
    R2L_REQUIRE(out_v != nullptr, "r2l_occ_compact: out_v is NULL");
    R2L_REQUIRE(out_z != nullptr, "r2l_occ_compact: out_z is NULL");
    R2L_REQUIRE(idx_out != nullptr, "r2l_occ_compact: idx_out is NULL");
    R2L_REQUIRE(work != nullptr, "r2l_occ_compact: work is NULL");
    R2L_REQUIRE(((uintptr_t)work & 3) == 0, "r2l_occ_compact: work is not 4-byte aligned");
    CompactArgs a;
    a.g = occ_dev(grid);
    a.o = rays_o; a.d = rays_d; a.v = viewdirs; a.z = z;
    a.n = R * (int64_t)S;
    a.S = S;
    a.blk = (unsigned*)work;
    a.out_o = out_o; a.out_d = out_d; a.out_v = out_v; a.out_z = out_z;
    a.idx = idx_out;
    const int64_t nb = (a.n + OCC_CHUNK - 1) / OCC_CHUNK;  // <= 2^20
    hipLaunchKernelGGL(r2l_occ_compact_kernel<false>, dim3((unsigned)nb), dim3(OCC_THREADS), 0, s, a);
    R2L_CHECK(hipGetLastError());
    hipLaunchKernelGGL(r2l_occ_scan_kernel, dim3(1), dim3(OCC_SCAN_THREADS), 0, s, a.blk, nb, (nb + OCC_SCAN_THREADS - 1) / OCC_SCAN_THREADS,
                       count_out);
    R2L_CHECK(hipGetLastError());
    hipLaunchKernelGGL(r2l_occ_compact_kernel<true>, dim3((unsigned)nb), dim3(OCC_THREADS), 0, s, a);
    R2L_CHECK(hipGetLastError());
    return 0;
}

extern "C" int64_t r2l_occ_index_work_bytes(int64_t n) {
    if (n < 0 || n >= ((int64_t)1 << 31)) {
        r2l_set_error_msg("r2l_occ_index_work_bytes: need 0 <= R*S < 2^31");
        return -1;
    }
    return r2l_occ_compact_work_bytes(n);  // (the same per-workgroup counts)
}

// r2l_occ_compact without its row copies: the same count / scan / placement launches, idx and the count bit for bit
extern "C" int r2l_occ_index(const r2l_occ_grid* grid, const float* rays_o, const float* rays_d, const float* z, int64_t R, int S,
                             int64_t* idx_out, int64_t* count_out, void* work, void* stream) {
    if (const char* why = occ_grid_check(grid, "r2l_occ_index: grid is NULL")) {
        r2l_set_error_msg(why);
        return (int)hipErrorInvalidValue;
    }
    R2L_REQUIRE(R >= 0, "r2l_occ_index: R is negative");
    R2L_REQUIRE(S >= 1, "r2l_occ_index: S: need S >= 1");
    R2L_REQUIRE(R < ((int64_t)1 << 31) && R * (int64_t)S < ((int64_t)1 << 31), "r2l_occ_index: R*S: need R*S < 2^31");
    R2L_REQUIRE(count_out != nullptr, "r2l_occ_index: count_out is NULL");
    hipStream_t s = (hipStream_t)stream;
    if (R == 0) {
        R2L_CHECK(hipMemsetAsync(count_out, 0, sizeof(int64_t), s));
        return 0;
    }
    R2L_REQUIRE(rays_o != nullptr, "r2l_occ_index: rays_o is NULL");
    R2L_REQUIRE(rays_d != nullptr, "r2l_occ_index: rays_d is NULL");
    R2L_REQUIRE(z != nullptr, "r2l_occ_index: z is NULL");
    R2L_REQUIRE(idx_out != nullptr, "r2l_occ_index: idx_out is NULL");
    R2L_REQUIRE(work != nullptr, "r2l_occ_index: work is NULL");
    R2L_REQUIRE(((uintptr_t)work & 3) == 0, "r2l_occ_index: work is not 4-byte aligned");
    CompactArgs a{};
    a.g = occ_dev(grid);
    a.o = rays_o; a.d = rays_d; a.z = z;
    a.n = R * (int64_t)S;
    a.S = S;
    a.blk = (unsigned*)work;
    a.idx = idx_out;
    const int64_t nb = (a.n + OCC_CHUNK - 1) / OCC_CHUNK;  // <= 2^20
    hipLaunchKernelGGL((r2l_occ_compact_kernel<false, false>), dim3((unsigned)nb), dim3(OCC_THREADS), 0, s, a);
    R2L_CHECK(hipGetLastError());
    hipLaunchKernelGGL(r2l_occ_scan_kernel, dim3(1), dim3(OCC_SCAN_THREADS), 0, s, a.blk, nb, (nb + OCC_SCAN_THREADS - 1) / OCC_SCAN_THREADS,
                       count_out);
    R2L_CHECK(hipGetLastError());
    hipLaunchKernelGGL((r2l_occ_compact_kernel<true, false>), dim3((unsigned)nb), dim3(OCC_THREADS), 0, s, a);
    R2L_CHECK(hipGetLastError());
    return 0;
}

extern "C" int64_t r2l_occ_rays_work_bytes(int64_t R) {
    if (R < 0 || R >= ((int64_t)1 << 31)) {
        r2l_set_error_msg("r2l_occ_rays_work_bytes: need 0 <= R < 2^31");
        return -1;
    }
    return r2l_occ_compact_work_bytes(R) + (R + 15) / 16 * 16;  // the per-workgroup counts, then a flag byte per ray
}

// The live rays of [R]: flag + count per 2048 rays, the scan of r2l_occ_index, placement.  The flags go to live_out when it is
// given, else into work.
extern "C" int r2l_occ_rays(const r2l_occ_grid* grid, const float* rays_o, const float* rays_d, int64_t R, float near, float far, int T,
                            int64_t* idx_out, int64_t* count_out, uint8_t* live_out, void* work, void* stream) {
    if (const char* why = occ_grid_check(grid, "r2l_occ_rays: grid is NULL")) {
        r2l_set_error_msg(why);
        return (int)hipErrorInvalidValue;
    }
    R2L_REQUIRE(R >= 0, "r2l_occ_rays: R is negative");
    R2L_REQUIRE(R < ((int64_t)1 << 31), "r2l_occ_rays: R: need R < 2^31");
    R2L_REQUIRE(T >= 1, "r2l_occ_rays: T: need T >= 1");
    R2L_REQUIRE(near - near == 0.f && far - far == 0.f, "r2l_occ_rays: near / far: not finite");
    R2L_REQUIRE(near <= far, "r2l_occ_rays: near / far: need near <= far");
    const float dt = (far - near) / (float)T;
    R2L_REQUIRE(dt - dt == 0.f, "r2l_occ_rays: near / far: far - near is out of fp32 range");
    R2L_REQUIRE(count_out != nullptr, "r2l_occ_rays: count_out is NULL");
    hipStream_t s = (hipStream_t)stream;
    if (R == 0) {
        R2L_CHECK(hipMemsetAsync(count_out, 0, sizeof(int64_t), s));
        return 0;
    }
    R2L_REQUIRE(rays_o != nullptr, "r2l_occ_rays: rays_o is NULL");
    R2L_REQUIRE(rays_d != nullptr, "r2l_occ_rays: rays_d is NULL");
    R2L_REQUIRE(idx_out != nullptr, "r2l_occ_rays: idx_out is NULL");
    R2L_REQUIRE(work != nullptr, "r2l_occ_rays: work is NULL");
    R2L_REQUIRE(((uintptr_t)work & 3) == 0, "r2l_occ_rays: work is not 4-byte aligned");
    unsigned* blk = (unsigned*)work;
    uint8_t* flags = live_out != nullptr ? live_out : (uint8_t*)work + r2l_occ_compact_work_bytes(R);
    const int64_t nb = (R + OCC_CHUNK - 1) / OCC_CHUNK;  // <= 2^20
    hipLaunchKernelGGL(r2l_occ_rays_flag_kernel, dim3((unsigned)nb), dim3(RAY_THREADS), 0, s, occ_dev(grid), rays_o, rays_d, R, near, dt, T,
                       flags, blk);
    R2L_CHECK(hipGetLastError());
    hipLaunchKernelGGL(r2l_occ_scan_kernel, dim3(1), dim3(OCC_SCAN_THREADS), 0, s, blk, nb, (nb + OCC_SCAN_THREADS - 1) / OCC_SCAN_THREADS,
                       count_out);
    R2L_CHECK(hipGetLastError());
    hipLaunchKernelGGL(r2l_occ_rays_place_kernel, dim3((unsigned)nb), dim3(OCC_THREADS), 0, s, flags, R, blk, idx_out);
    R2L_CHECK(hipGetLastError());
    return 0;
}

extern "C" int r2l_rays_gather(const float* rays_o, const float* rays_d, int64_t R, const int64_t* idx, int64_t M, float* out_o,
                               float* out_d, void* stream) {
    R2L_REQUIRE(R >= 0 && R < ((int64_t)1 << 31), "r2l_rays_gather: R: need 0 <= R < 2^31");
    R2L_REQUIRE(M >= 0 && M < ((int64_t)1 << 31), "r2l_rays_gather: M: need 0 <= M < 2^31");
    if (M == 0) return 0;
    R2L_REQUIRE(idx != nullptr, "r2l_rays_gather: idx is NULL");
    R2L_REQUIRE(out_o != nullptr, "r2l_rays_gather: out_o is NULL");
    R2L_REQUIRE(out_d != nullptr, "r2l_rays_gather: out_d is NULL");
    R2L_REQUIRE(R == 0 || rays_o != nullptr, "r2l_rays_gather: rays_o is NULL");
    R2L_REQUIRE(R == 0 || rays_d != nullptr, "r2l_rays_gather: rays_d is NULL");
    hipLaunchKernelGGL(r2l_rays_gather_kernel, dim3(occ_blocks(M * 3, OCC_THREADS)), dim3(OCC_THREADS), 0, (hipStream_t)stream, rays_o,
                       rays_d, R, idx, M, out_o, out_d);
    R2L_CHECK(hipGetLastError());
    return 0;
}

extern "C" int r2l_rgb_scatter_bg(const float* rgb_live, const int64_t* idx, int64_t M, const uint8_t* live, float bg, float* rgb_out,
                                  int64_t R, void* stream) {
    R2L_REQUIRE(R >= 0 && R < ((int64_t)1 << 31), "r2l_rgb_scatter_bg: R: need 0 <= R < 2^31");
    R2L_REQUIRE(M >= 0 && M <= R, "r2l_rgb_scatter_bg: M: need 0 <= M <= R");
    R2L_REQUIRE(bg == bg, "r2l_rgb_scatter_bg: bg is NaN");
    if (R == 0) return 0;
    R2L_REQUIRE(live != nullptr, "r2l_rgb_scatter_bg: live is NULL");
    R2L_REQUIRE(rgb_out != nullptr, "r2l_rgb_scatter_bg: rgb_out is NULL");
    R2L_REQUIRE(M == 0 || rgb_live != nullptr, "r2l_rgb_scatter_bg: rgb_live is NULL");
    R2L_REQUIRE(M == 0 || idx != nullptr, "r2l_rgb_scatter_bg: idx is NULL");
    hipLaunchKernelGGL(r2l_rgb_scatter_bg_kernel, dim3(occ_blocks(R, OCC_THREADS)), dim3(OCC_THREADS), 0, (hipStream_t)stream, rgb_live, idx,
                       M, live, bg, rgb_out, R);
    R2L_CHECK(hipGetLastError());
    return 0;
}

extern "C" int r2l_occ_live_add(const int64_t* count, int64_t total, int64_t* live_acc, void* stream) {
    R2L_REQUIRE(count != nullptr, "r2l_occ_live_add: count is NULL");
    R2L_REQUIRE(total >= 0, "r2l_occ_live_add: total is negative");
    R2L_REQUIRE(live_acc != nullptr, "r2l_occ_live_add: live_acc is NULL");
    hipLaunchKernelGGL(r2l_occ_live_add_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, count, total, live_acc);
    R2L_CHECK(hipGetLastError());
    return 0;
}

extern "C" int64_t r2l_occ_index_seg_work_bytes(int64_t n) {
    if (n < 0 || n >= ((int64_t)1 << 31)) {
        r2l_set_error_msg("r2l_occ_index_seg_work_bytes: need 0 <= R*(s1-s0) < 2^31");
        return -1;
    }
    return r2l_occ_compact_work_bytes(n);  // (the same per-workgroup counts)
}

// The index of one segment of every ray, with the terminated rays left out: the count / scan / placement launches of r2l_occ_index
// over the R * (s1 - s0) samples of the segment
extern "C" int r2l_occ_index_seg(const r2l_occ_grid* grid, const float* rays_o, const float* rays_d, const float* z, int64_t R, int S,
                                 int s0, int s1, const float* trans, float eps, int64_t* idx_out, int64_t* count_out, void* work,
                                 void* stream) {
    if (grid != nullptr)
        if (const char* why = occ_grid_check(grid, "r2l_occ_index_seg: grid is NULL")) {
            r2l_set_error_msg(why);
            return (int)hipErrorInvalidValue;
        }
    R2L_REQUIRE(R >= 0, "r2l_occ_index_seg: R is negative");
    R2L_REQUIRE(S >= 1, "r2l_occ_index_seg: S: need S >= 1");
    R2L_REQUIRE(R < ((int64_t)1 << 31) && R * (int64_t)S < ((int64_t)1 << 31), "r2l_occ_index_seg: R*S: need R*S < 2^31");
    R2L_REQUIRE(s0 >= 0 && s0 < s1 && s1 <= S, "r2l_occ_index_seg: s0 / s1: need 0 <= s0 < s1 <= S");
    R2L_REQUIRE(trans == nullptr || (eps > 0.f && eps - eps == 0.f), "r2l_occ_index_seg: eps: need a positive finite value with trans");
    R2L_REQUIRE(count_out != nullptr, "r2l_occ_index_seg: count_out is NULL");
    hipStream_t s = (hipStream_t)stream;
    if (R == 0) {
        R2L_CHECK(hipMemsetAsync(count_out, 0, sizeof(int64_t), s));
        return 0;
    }
    R2L_REQUIRE(rays_o != nullptr, "r2l_occ_index_seg: rays_o is NULL");
    R2L_REQUIRE(rays_d != nullptr, "r2l_occ_index_seg: rays_d is NULL");
    R2L_REQUIRE(z != nullptr, "r2l_occ_index_seg: z is NULL");
    R2L_REQUIRE(idx_out != nullptr, "r2l_occ_index_seg: idx_out is NULL");
    R2L_REQUIRE(work != nullptr, "r2l_occ_index_seg: work is NULL");
    R2L_REQUIRE(((uintptr_t)work & 3) == 0, "r2l_occ_index_seg: work is not 4-byte aligned");
    CompactArgs a{};
    if (grid != nullptr) a.g = occ_dev(grid);  // (else bits == NULL: every point is live by the grid rule)
    a.o = rays_o; a.d = rays_d; a.z = z;
    a.S = S;
    a.s0 = s0;
    a.W = s1 - s0;
    a.n = R * (int64_t)a.W;
    a.trans = trans;
    a.eps = eps;
    a.blk = (unsigned*)work;
    a.idx = idx_out;
    const int64_t nb = (a.n + OCC_CHUNK - 1) / OCC_CHUNK;  // <= 2^20
    hipLaunchKernelGGL((r2l_occ_compact_kernel<false, false, true>), dim3((unsigned)nb), dim3(OCC_THREADS), 0, s, a);
    R2L_CHECK(hipGetLastError());
    hipLaunchKernelGGL(r2l_occ_scan_kernel, dim3(1), dim3(OCC_SCAN_THREADS), 0, s, a.blk, nb, (nb + OCC_SCAN_THREADS - 1) / OCC_SCAN_THREADS,
                       count_out);
    R2L_CHECK(hipGetLastError());
    hipLaunchKernelGGL((r2l_occ_compact_kernel<true, false, true>), dim3((unsigned)nb), dim3(OCC_THREADS), 0, s, a);
    R2L_CHECK(hipGetLastError());
    return 0;
}

extern "C" int r2l_ert_advance(const float* raw, const float* z, const float* rays_d, int64_t R, int S, int s0, int s1, float* trans,
                               void* stream) {
    R2L_REQUIRE(R >= 0, "r2l_ert_advance: R is negative");
    R2L_REQUIRE(S >= 1 && S <= ERT_MAX_S, "r2l_ert_advance: S: need 1 <= S <= 256");
    R2L_REQUIRE(R < ((int64_t)1 << 31) && R * (int64_t)S < ((int64_t)1 << 31), "r2l_ert_advance: R*S: need R*S < 2^31");
    R2L_REQUIRE(s0 >= 0 && s0 < s1 && s1 <= S, "r2l_ert_advance: s0 / s1: need 0 <= s0 < s1 <= S");
    if (R == 0) return 0;
    R2L_REQUIRE(raw != nullptr, "r2l_ert_advance: raw is NULL");
    R2L_REQUIRE(z != nullptr, "r2l_ert_advance: z is NULL");
    R2L_REQUIRE(rays_d != nullptr, "r2l_ert_advance: rays_d is NULL");
    R2L_REQUIRE(trans != nullptr, "r2l_ert_advance: trans is NULL");
    const int64_t nb = (R + ERT_RAYS - 1) / ERT_RAYS;  // < 2^26
    hipLaunchKernelGGL(r2l_ert_advance_kernel, dim3((unsigned)nb), dim3(OCC_THREADS), 0, (hipStream_t)stream, raw, z, rays_d, R, S, s0,
                       s1 - s0, trans);
    R2L_CHECK(hipGetLastError());
    return 0;
}

// what r2l_teacher_frames_occ_cfg asks of a grid before it enqueues anything
const char* r2l_occ_grid_why(const r2l_occ_grid* g, const char* null_msg) { return occ_grid_check(g, null_msg); }

extern "C" int r2l_occ_scatter(const float* raw_live, const int64_t* idx, int64_t M, float* raw_out, int64_t R, int S, void* stream) {
    R2L_REQUIRE(R >= 0, "r2l_occ_scatter: R is negative");
    R2L_REQUIRE(S >= 1, "r2l_occ_scatter: S: need S >= 1");
    R2L_REQUIRE(R < ((int64_t)1 << 31) && R * (int64_t)S < ((int64_t)1 << 31), "r2l_occ_scatter: R*S: need R*S < 2^31");
    R2L_REQUIRE(M >= 0 && M <= R * (int64_t)S, "r2l_occ_scatter: M: need 0 <= M <= R*S");
    if (R == 0) return 0;
    R2L_REQUIRE(raw_out != nullptr, "r2l_occ_scatter: raw_out is NULL");
    R2L_REQUIRE(((uintptr_t)raw_out & 15) == 0, "r2l_occ_scatter: raw_out is not 16-byte aligned");
    R2L_REQUIRE(M == 0 || raw_live != nullptr, "r2l_occ_scatter: raw_live is NULL");
    R2L_REQUIRE(M == 0 || ((uintptr_t)raw_live & 15) == 0, "r2l_occ_scatter: raw_live is not 16-byte aligned");
    R2L_REQUIRE(M == 0 || idx != nullptr, "r2l_occ_scatter: idx is NULL");
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_out = R * (int64_t)S;
    R2L_CHECK(hipMemsetAsync(raw_out, 0, (size_t)n_out * 4 * sizeof(float), s));
    if (M == 0) return 0;
    hipLaunchKernelGGL(r2l_occ_scatter_kernel, dim3(occ_blocks(M, OCC_THREADS)), dim3(OCC_THREADS), 0, s,
                       reinterpret_cast<const float4*>(raw_live), idx, M, reinterpret_cast<float4*>(raw_out), n_out);
    R2L_CHECK(hipGetLastError());
    return 0;
}
