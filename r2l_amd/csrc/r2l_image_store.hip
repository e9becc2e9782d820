// Ray store rows straight from images and poses (include/r2l_hip.h r2l_store_append_images): the real training rays of a scene
// — README step 4's converter, utils/convert_original_data_to_rays_*.py, without the files — are a pure function of K images and
// K poses, so one launch writes the shuffled [o, d, rgb] shards that r2l_frame_rays(rows) -> rgb copy into columns 6..8 ->
// r2l_store_append would have written, bit for bit, and the [K*H*W, 9] intermediate never exists.
//   Output row i = [pixel_ray of pixel r, images[r]] with r = pi(key, K*H*W)(i) (csrc/r2l_perm.h; shuffle = 0: r = i).  After the
//   shuffle the frame of a lane's ray is any of the K: the pose (12 floats) and focal are read per lane; the K poses stay in
//   cache.  12 B gathered and 36 B written a ray.  36-byte rows are not 16-byte aligned, so — as r2l_cstore_batch does — a
//   workgroup takes 1024 output rows (2304 16-byte words), builds them in LDS — thread t takes rows t, t + 256, ...: four
//   independent gathers in flight a thread, LDS writes at an odd stride of 9 floats (no bank conflict) — and writes the tile
//   out as words, lane i at base + 16 i.
// Built with the flags of r2l_teacher_frame.hip (r2l_amd/build.py FILE_FLAGS): the rays must reproduce.
#include "r2l_common.h"
#include "r2l_perm.h"
#include "r2l_pixel_ray.h"

namespace {

constexpr int IS_THREADS = 256;
constexpr int IS_TILE_ROWS = 1024;  // output rows per workgroup pass: 4 per thread, 2304 16-byte words

// SMALL: K*H*W < 2^32, the ray number splits into (frame, row, col) with 32-bit divisions
template <bool SMALL>
__global__ __launch_bounds__(IS_THREADS) void r2l_store_append_images_kernel(
    const float* __restrict__ images, const float* __restrict__ c2w, const float* __restrict__ focal_dev, float focal, int H, int W,
    unsigned long long hw, float4* __restrict__ out, unsigned long long n_rows, int64_t n_out, int half_bits, unsigned long long key,
    int shuffle) {
    __shared__ __attribute__((aligned(16))) float tile[IS_TILE_ROWS * 9];
    unsigned k[4];
    perm_round_keys(key, k);
    const int64_t n_tiles = (n_out + IS_TILE_ROWS - 1) / IS_TILE_ROWS;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t r0 = t * IS_TILE_ROWS;
        const int rows_here = (int)(n_out - r0 < IS_TILE_ROWS ? n_out - r0 : IS_TILE_ROWS);  // a multiple of 4
#pragma unroll
        for (int q = 0; q < IS_TILE_ROWS / IS_THREADS; ++q) {
            const int r = (int)threadIdx.x + q * IS_THREADS;
            if (r < rows_here) {
                const unsigned long long i = (unsigned long long)(r0 + r);
                const unsigned long long src = shuffle ? perm_at(i, n_rows, half_bits, k) : i;  // < n_rows
                int64_t kf;
                int row, col;
                if (SMALL) {
                    const unsigned s = (unsigned)src, f = s / (unsigned)hw, pix = s - f * (unsigned)hw;
                    const unsigned y = pix / (unsigned)W;
                    kf = f; row = (int)y; col = (int)(pix - y * (unsigned)W);
                } else {
                    const unsigned long long f = src / hw, pix = src - f * hw;
                    const unsigned long long y = pix / (unsigned long long)W;
                    kf = (int64_t)f; row = (int)y; col = (int)(pix - y * (unsigned long long)W);
                }
                const float* __restrict__ px = images + (int64_t)src * 3;
                const float c0 = px[0], c1 = px[1], c2 = px[2];
                float o[3], d[3];
                pixel_ray(c2w + kf * 12, focal_dev != nullptr ? focal_dev[kf] : focal, H, W, row, col, o, d);
                float* __restrict__ w = tile + r * 9;
#pragma unroll
                for (int a = 0; a < 3; ++a) { w[a] = o[a]; w[3 + a] = d[a]; }
                w[6] = c0; w[7] = c1; w[8] = c2;
            }
        }
        __syncthreads();
        float4* __restrict__ dst = out + r0 / 4 * 9;
        const float4* __restrict__ tw = reinterpret_cast<const float4*>(tile);
        const int words_here = rows_here / 4 * 9;
        for (int x = threadIdx.x; x < words_here; x += IS_THREADS) dst[x] = tw[x];
        __syncthreads();  // tile is rewritten by the next pass
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" int r2l_store_append_images(const float* images, const float* c2w_dev, const float* focal_dev, float focal, int K, int H,
                                       int W, float* store, int64_t capacity_shards, int64_t first_shard, int64_t rays_per_shard,
                                       uint64_t key, int shuffle, int64_t* n_written_out, void* stream) {
    R2L_REQUIRE(images != nullptr && c2w_dev != nullptr && store != nullptr && n_written_out != nullptr,
                "r2l_store_append_images: a required pointer is NULL (images, c2w_dev, store, n_written_out)");
    R2L_REQUIRE(K >= 1, "r2l_store_append_images: need K >= 1");
    R2L_REQUIRE(H >= 1 && W >= 1, "r2l_store_append_images: need H >= 1 and W >= 1");
    R2L_REQUIRE(focal_dev != nullptr || focal > 0.f, "r2l_store_append_images: need focal > 0 (or focal_dev)");
    R2L_REQUIRE(rays_per_shard > 0 && rays_per_shard % 4 == 0,
                "r2l_store_append_images: rays_per_shard must be positive and a multiple of 4 (a shard is a whole number of 16-byte "
                "words)");
    R2L_REQUIRE(capacity_shards >= 0 && first_shard >= 0, "r2l_store_append_images: capacity_shards / first_shard is negative");
    const uint64_t hw = (uint64_t)H * (uint64_t)W;  // < 2^62
    R2L_REQUIRE(hw <= ((uint64_t)1 << 58) / (uint64_t)K, "r2l_store_append_images: K * H * W exceeds 2^58");
    const int64_t n_rows = (int64_t)(hw * (uint64_t)K);
    const int64_t m = n_rows / rays_per_shard;
    R2L_REQUIRE(m <= capacity_shards && first_shard <= capacity_shards - m,
                "r2l_store_append_images: first_shard + floor(K*H*W / rays_per_shard) exceeds capacity_shards");
    R2L_REQUIRE(capacity_shards <= (((int64_t)1 << 58) / rays_per_shard), "r2l_store_append_images: capacity_shards * rays_per_shard "
                "exceeds 2^58");
    R2L_REQUIRE(aligned16(store), "r2l_store_append_images: store must be 16-byte aligned");
    {  // the kernel reads images through __restrict__ while it writes the store
        const uintptr_t ia = (uintptr_t)images, ib = ia + (uintptr_t)n_rows * 12u;
        const uintptr_t sa = (uintptr_t)store, sb = sa + (uintptr_t)capacity_shards * (uintptr_t)rays_per_shard * 36u;
        R2L_REQUIRE(ib <= sa || sb <= ia, "r2l_store_append_images: images overlap the store");
    }
    *n_written_out = m;
    if (m == 0) return 0;
    const int64_t n_out = m * rays_per_shard;
    const int64_t n_tiles = (n_out + IS_TILE_ROWS - 1) / IS_TILE_ROWS;
    const unsigned grid = (unsigned)(n_tiles > 16384 ? 16384 : n_tiles);
    float4* out = (float4*)(store + first_shard * rays_per_shard * 9);
    if (n_rows <= (int64_t)0xffffffffll)
        hipLaunchKernelGGL(r2l_store_append_images_kernel<true>, dim3(grid), dim3(IS_THREADS), 0, (hipStream_t)stream, images, c2w_dev,
                           focal_dev, focal, H, W, (unsigned long long)hw, out, (unsigned long long)n_rows, n_out,
                           perm_half_bits(n_rows), (unsigned long long)key, shuffle != 0 ? 1 : 0);
    else
        hipLaunchKernelGGL(r2l_store_append_images_kernel<false>, dim3(grid), dim3(IS_THREADS), 0, (hipStream_t)stream, images, c2w_dev,
                           focal_dev, focal, H, W, (unsigned long long)hw, out, (unsigned long long)n_rows, n_out,
                           perm_half_bits(n_rows), (unsigned long long)key, shuffle != 0 ? 1 : 0);
    R2L_CHECK(hipGetLastError());
    return 0;
}
