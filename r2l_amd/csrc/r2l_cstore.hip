// Compact ray store: 16 bytes a ray instead of 36 (include/r2l_hip.h "compact ray store").  A store that the TEACHER fills holds
// rows whose o, d are a pure function of the pose, the pose's focal and the pixel — pixel_ray of csrc/r2l_pixel_ray.h, the
// definition r2l_frame_rays computed them with — so a row keeps { rgb, id } and the batch kernel recomputes o, d per draw:
//   r2l_cstore_append: rgb[K*H*W] (any row stride >= 3) -> floor(K*H*W / rps) shards of rows { rgb[pi(i)], id = pi(i) }, pi the
//     bijection r2l_store_append shuffles by (csrc/r2l_perm.h); the K poses and focals go into the pose table, the new shards'
//     entries of shard_pose0 point at them.  One launch: a thread per output row writes one 16-byte word (coalesced); the
//     first threads of the grid also copy the 13 K floats of the pose table.
//   r2l_cstore_batch: the sampler of r2l_store_batch, then per row one 16-byte read, pixel_ray, and the 36-byte [o, d, rgb] row
//     of the plain store's batch, bit for bit.  36-byte rows are not 16-byte aligned, so a workgroup takes 1024 rows (a whole
//     number of 16-byte words: 2304), builds them in LDS — thread t takes rows t, t + 256, ...: the reads are lane-contiguous
//     words, the LDS writes have an odd stride of 9 floats (no bank conflict) — and writes the tile out as words, lane i at
//     base + 16 i, as r2l_store_batch's copy does.  16 B read + 36 B written a ray against 36 + 36.
// Built with the flags of r2l_teacher_frame.hip (r2l_amd/build.py FILE_FLAGS): the rays must reproduce.
#include "r2l_common.h"
#include "r2l_perm.h"
#include "r2l_pixel_ray.h"
#include <cstdio>

namespace {

constexpr int CS_THREADS = 256;
constexpr int CS_TILE_ROWS = 1024;  // batch rows per workgroup pass: 4 per thread, 2304 16-byte words

static_assert(sizeof(r2l_cstore) == 72, "r2l_cstore has no padding (r2l_amd/_lib.py CompactStoreDesc is its twin)");

struct CRow {  // one 16-byte row of the store
    float r, g, b;
    unsigned id;
};
static_assert(sizeof(CRow) == 16, "a compact row is one 16-byte word");

__global__ __launch_bounds__(CS_THREADS) void r2l_cstore_append_kernel(
    const float* __restrict__ rgb, int64_t rgb_stride, const float* __restrict__ c2w, const float* __restrict__ focal_dev, float focal,
    int K, uint4* __restrict__ rows_out, float* __restrict__ pose_c2w, float* __restrict__ pose_focal, int* __restrict__ shard_pose0,
    int64_t m, int first_pose, unsigned long long n_rows, int64_t n_out, int half_bits, unsigned long long key, int shuffle) {
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    unsigned k[4];
    perm_round_keys(key, k);
    for (int64_t i = t0; i < n_out; i += step) {
        const unsigned long long src = shuffle ? perm_at((unsigned long long)i, n_rows, half_bits, k) : (unsigned long long)i;
        const float* __restrict__ px = rgb + (int64_t)src * rgb_stride;
        uint4 w;
        w.x = __float_as_uint(px[0]); w.y = __float_as_uint(px[1]); w.z = __float_as_uint(px[2]);
        w.w = (unsigned)src;  // < n_rows <= 2^32 - 1 (checked by the host)
        rows_out[i] = w;
    }
    for (int64_t e = t0; e < (int64_t)K * 12; e += step) pose_c2w[e] = c2w[e];
    for (int64_t e = t0; e < K; e += step) pose_focal[e] = focal_dev != nullptr ? focal_dev[e] : focal;
    for (int64_t e = t0; e < m; e += step) shard_pose0[e] = first_pose;
}

__global__ __launch_bounds__(CS_THREADS) void r2l_cstore_batch_kernel(
    const uint4* __restrict__ rows, const float* __restrict__ pose_c2w, const float* __restrict__ pose_focal,
    const int* __restrict__ shard_pose0, int64_t capacity_poses, int H, int W, unsigned hw, float4* __restrict__ batch,
    int* __restrict__ ids_out, int64_t n_shards, int64_t rps, int64_t chunks_per_shard, int64_t draw0, int64_t n_draw,
    unsigned long long seed, int half_bits) {
    __shared__ __attribute__((aligned(16))) float tile[CS_TILE_ROWS * 9];
    const int64_t n_work = n_draw * chunks_per_shard;
    for (int64_t w = blockIdx.x; w < n_work; w += gridDim.x) {
        const int64_t j = w / chunks_per_shard;
        const int64_t c = w - j * chunks_per_shard;
        const unsigned long long t = (unsigned long long)(draw0 + j);
        const unsigned long long epoch = t / (unsigned long long)n_shards;
        unsigned k[4];
        perm_round_keys(perm_epoch_key(seed, epoch), k);  // (uniform over the workgroup, as in r2l_store_batch)
        const int64_t shard = (int64_t)perm_at(t - epoch * (unsigned long long)n_shards, (unsigned long long)n_shards, half_bits, k);
        if (ids_out != nullptr && c == 0 && threadIdx.x == 0) ids_out[j] = (int)shard;
        const int64_t r0 = c * CS_TILE_ROWS;
        const int rows_here = (int)(rps - r0 < CS_TILE_ROWS ? rps - r0 : CS_TILE_ROWS);  // a multiple of 4
        const uint4* __restrict__ src = rows + shard * rps + r0;
        const int64_t p0 = shard_pose0[shard];
#pragma unroll
        for (int q = 0; q < CS_TILE_ROWS / CS_THREADS; ++q) {
            const int r = (int)threadIdx.x + q * CS_THREADS;
            if (r < rows_here) {
                const uint4 v = src[r];
                const unsigned id = v.w, kp = id / hw, pix = id - kp * hw;  // kp * hw <= id: no wrap
                const unsigned row = pix / (unsigned)W, col = pix - row * (unsigned)W;
                const int64_t p = p0 + (int64_t)kp;
                float o[3], d[3];
                if (p >= 0 && p < capacity_poses) {
                    pixel_ray(pose_c2w + p * 12, pose_focal[p], H, W, (int)row, (int)col, o, d);
                } else {  // a row that names no pose of the table (a store nobody appended to): NaN rays, nothing is read
#pragma unroll
                    for (int i = 0; i < 3; ++i) o[i] = d[i] = __uint_as_float(0x7fc00000u);
                }
                float* __restrict__ out = tile + r * 9;
#pragma unroll
                for (int i = 0; i < 3; ++i) { out[i] = o[i]; out[3 + i] = d[i]; }
                out[6] = __uint_as_float(v.x); out[7] = __uint_as_float(v.y); out[8] = __uint_as_float(v.z);
            }
        }
        __syncthreads();
        float4* __restrict__ dst = batch + (j * rps + r0) / 4 * 9;
        const float4* __restrict__ tw = reinterpret_cast<const float4*>(tile);
        const int words_here = rows_here / 4 * 9;
        for (int x = threadIdx.x; x < words_here; x += CS_THREADS) dst[x] = tw[x];
        __syncthreads();  // tile is rewritten by the next pass
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// What is wrong with a store's description, or nullptr.  `who` is not part of the message: the callers prefix their name.
const char* store_check(const r2l_cstore* s) {
    if (s == nullptr) return "store is NULL";
    if (s->rows == nullptr || s->pose_c2w == nullptr || s->pose_focal == nullptr || s->shard_pose0 == nullptr)
        return "a pointer of the store is NULL (rows, pose_c2w, pose_focal, shard_pose0)";
    if (s->reserved[0] != 0 || s->reserved[1] != 0) return "r2l_cstore.reserved must be 0";
    if (s->H < 1 || s->W < 1) return "r2l_cstore.H / .W: need H >= 1 and W >= 1";
    if (s->rays_per_shard <= 0 || s->rays_per_shard % 4 != 0)
        return "r2l_cstore.rays_per_shard must be positive and a multiple of 4 (a shard's batch rows are a whole number of 16-byte words)";
    if (s->capacity_shards < 0 || s->capacity_shards > 0x7fffffff) return "r2l_cstore.capacity_shards: need 0 <= capacity_shards < 2^31";
    if (s->capacity_poses < 0 || s->capacity_poses > 0x7fffffff) return "r2l_cstore.capacity_poses: need 0 <= capacity_poses < 2^31";
    if (!aligned16(s->rows)) return "r2l_cstore.rows must be 16-byte aligned";
    return nullptr;
}

thread_local char g_msg[256];
int refuse(const char* who, const char* why) {
    snprintf(g_msg, sizeof(g_msg), "%s: %s", who, why);
    r2l_set_error_msg(g_msg);
    return (int)hipErrorInvalidValue;
}

}  // namespace

extern "C" int r2l_cstore_append(const r2l_cstore* store, const float* rgb, int64_t rgb_stride, const float* c2w_dev,
                                 const float* focal_dev, float focal, int K, int64_t first_shard, int64_t first_pose, uint64_t key,
                                 int shuffle, int64_t* n_written_out, void* stream) {
    if (const char* why = store_check(store)) return refuse("r2l_cstore_append", why);
    R2L_REQUIRE(rgb != nullptr && c2w_dev != nullptr && n_written_out != nullptr,
                "r2l_cstore_append: a required pointer is NULL (rgb, c2w_dev, n_written_out)");
    R2L_REQUIRE(K >= 1, "r2l_cstore_append: need K >= 1");
    R2L_REQUIRE(rgb_stride >= 3, "r2l_cstore_append: rgb_stride is the row stride of rgb in floats: at least 3");
    R2L_REQUIRE(focal_dev != nullptr || focal > 0.f, "r2l_cstore_append: need focal > 0 (or focal_dev)");
    R2L_REQUIRE(first_shard >= 0 && first_pose >= 0, "r2l_cstore_append: first_shard / first_pose is negative");
    const uint64_t kh = (uint64_t)K * (uint64_t)store->H;  // < 2^62; checked before it is multiplied again
    R2L_REQUIRE(kh <= 0xffffffffull && kh * (uint64_t)store->W <= 0xffffffffull,
                "r2l_cstore_append: K * H * W exceeds 2^32 - 1 (a row's id is 32 bits)");
    const int64_t n_rows = (int64_t)(kh * (uint64_t)store->W);
    const int64_t m = n_rows / store->rays_per_shard;
    R2L_REQUIRE(m <= store->capacity_shards && first_shard <= store->capacity_shards - m,
                "r2l_cstore_append: first_shard + floor(K*H*W / rays_per_shard) exceeds capacity_shards");
    R2L_REQUIRE(K <= store->capacity_poses && first_pose <= store->capacity_poses - K,
                "r2l_cstore_append: first_pose + K exceeds capacity_poses");
    *n_written_out = m;
    if (m == 0) return 0;  // no shard refers to these poses: nothing is enqueued
    const int64_t n_out = m * store->rays_per_shard;
    const int64_t blocks = (n_out + CS_THREADS - 1) / CS_THREADS;
    const unsigned grid = (unsigned)(blocks > 8192 ? 8192 : blocks);
    hipLaunchKernelGGL(r2l_cstore_append_kernel, dim3(grid), dim3(CS_THREADS), 0, (hipStream_t)stream, rgb, rgb_stride, c2w_dev,
                       focal_dev, focal, K, (uint4*)store->rows + first_shard * store->rays_per_shard,
                       store->pose_c2w + first_pose * 12, store->pose_focal + first_pose, store->shard_pose0 + first_shard, m,
                       (int)first_pose, (unsigned long long)n_rows, n_out, perm_half_bits(n_rows), (unsigned long long)key,
                       shuffle != 0 ? 1 : 0);
    R2L_CHECK(hipGetLastError());
    return 0;
}

extern "C" int r2l_cstore_batch(const r2l_cstore* store, int64_t n_shards, int64_t draw0, int64_t n_draw, uint64_t seed, float* batch,
                                int32_t* ids_out, void* stream) {
    if (const char* why = store_check(store)) return refuse("r2l_cstore_batch", why);
    R2L_REQUIRE(batch != nullptr, "r2l_cstore_batch: batch is NULL");
    R2L_REQUIRE(n_shards >= 1 && n_shards <= store->capacity_shards,
                "r2l_cstore_batch: need 1 <= n_shards <= capacity_shards (< 2^31: ids are int32)");
    R2L_REQUIRE(n_draw >= 0, "r2l_cstore_batch: n_draw is negative");
    R2L_REQUIRE(draw0 >= 0 && draw0 <= INT64_MAX - n_draw, "r2l_cstore_batch: draw0 is negative (or draw0 + n_draw overflows)");
    R2L_REQUIRE(aligned16(batch), "r2l_cstore_batch: batch must be 16-byte aligned");
    const uint64_t hw = (uint64_t)store->H * (uint64_t)store->W;
    R2L_REQUIRE(hw <= 0xffffffffull, "r2l_cstore_batch: H * W exceeds 2^32 - 1 (a row's id is 32 bits)");
    if (n_draw == 0) return 0;
    const int64_t rps = store->rays_per_shard;
    const int64_t chunks = (rps + CS_TILE_ROWS - 1) / CS_TILE_ROWS;
    const int64_t n_work = n_draw * chunks;
    const unsigned grid = (unsigned)(n_work > 16384 ? 16384 : n_work);
    hipLaunchKernelGGL(r2l_cstore_batch_kernel, dim3(grid), dim3(CS_THREADS), 0, (hipStream_t)stream, (const uint4*)store->rows,
                       (const float*)store->pose_c2w, (const float*)store->pose_focal, (const int*)store->shard_pose0,
                       store->capacity_poses, store->H, store->W, (unsigned)hw, (float4*)batch, (int*)ids_out, n_shards, rps, chunks,
                       draw0, n_draw, (unsigned long long)seed, perm_half_bits(n_shards));
    R2L_CHECK(hipGetLastError());
    return 0;
}
