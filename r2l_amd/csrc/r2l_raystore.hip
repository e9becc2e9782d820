// Device-resident ray store: the teacher's [o, d, rgb] rows stay in HBM between create_data and training instead of going
// through [4096,9] .npy shards (reference: utils/create_data.py:854-872 writes them, main.py:759-808 reads them back).
//
// The store is caller-owned: capacity_shards * rays_per_shard rows of 9 fp32, shard s = rows [s * rps, (s+1) * rps).  Two
// stateless entry points:
//   r2l_store_append: rows_in[n_rows, 9] -> floor(n_rows / rps) shards from first_shard on; output row i = input row
//     pi(key, n_rows)(i) (csrc/r2l_perm.h, the bijection of r2l_pool_pick), the tail of the permuted sequence is dropped as
//     create_data.py:862-872 drops it.  A gather of 36-byte rows: a workgroup takes 256 output rows, evaluates the bijection
//     once per row into LDS, then writes the 2304 floats of its tile in order (lane i at base + 4 i: coalesced writes; the
//     reads are 36-byte pieces wherever the permutation sends them).
//   r2l_store_append_live: r2l_store_append of the rows rows_in[idx[0..M)] (the live rays of r2l_occ_rays) without gathering them
//     first: the same kernel, the permutation over M, the row read through idx.
//   r2l_store_batch: draw t = draw0 + j takes shard pi(epoch_key(seed, t / n_shards), n_shards)(t % n_shards) — a fresh
//     permutation of the shards per epoch, without replacement inside one (the InfiniteSampler of main.py:759-767) — and copies
//     it to rows [j * rps, (j+1) * rps) of the batch with 16-byte accesses, lane i at base + 16 i.  A pure function of
//     (seed, n_shards, t): the host uploads nothing, a resumed run needs no sampler state.
// Every row and float offset is 64-bit: a full store of 10 000 poses is 14.4 G floats.
#include "r2l_common.h"
#include "r2l_perm.h"

namespace {

constexpr int TILE_ROWS = 256;  // output rows per workgroup pass of the append (= its thread count)
constexpr int COPY_WORDS = 1024;  // 16-byte words per workgroup pass of the batch copy (4 per lane)

// LIVE (r2l_store_append_live): the permutation runs over the M entries of idx and row i comes from input row idx[pi(i)]; an
// index outside [0, n_src) gives a NaN row and reads nothing.  The plain instantiation compiles from the code it had.
template <bool LIVE>
__global__ __launch_bounds__(TILE_ROWS) void r2l_store_append_kernel(const float* __restrict__ rows_in, float* __restrict__ out,
                                                                      int64_t n_rows, int64_t n_out, int half_bits,
                                                                      unsigned long long key, int shuffle,
                                                                      const int64_t* __restrict__ idx, int64_t n_src) {
    __shared__ int64_t src[TILE_ROWS];
    unsigned k[4];
    perm_round_keys(key, k);
    const int64_t n_tiles = (n_out + TILE_ROWS - 1) / TILE_ROWS;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t row0 = tile * TILE_ROWS;
        const int rows_here = (int)(n_out - row0 < TILE_ROWS ? n_out - row0 : TILE_ROWS);
        if ((int)threadIdx.x < rows_here) {
            const int64_t i = row0 + threadIdx.x;
            int64_t at = shuffle ? (int64_t)perm_at((unsigned long long)i, (unsigned long long)n_rows, half_bits, k) : i;
            if constexpr (LIVE) {
                at = idx[at];
                if (at < 0 || at >= n_src) at = -1;
            }
            src[threadIdx.x] = at;
        }
        __syncthreads();
        float* __restrict__ dst = out + row0 * 9;
        for (int e = threadIdx.x; e < rows_here * 9; e += TILE_ROWS) {
            const int r = e / 9;
            if constexpr (LIVE) {
                const int64_t at = src[r];
                dst[e] = at < 0 ? __int_as_float(0x7fc00000) : rows_in[at * 9 + (e - r * 9)];
            } else {
                dst[e] = rows_in[src[r] * 9 + (e - r * 9)];
            }
        }
        __syncthreads();  // src is rewritten by the next tile
    }
}

__global__ __launch_bounds__(256) void r2l_store_batch_kernel(const float4* __restrict__ store, float4* __restrict__ batch,
                                                               int* __restrict__ ids_out, int64_t n_shards, int64_t words_per_shard,
                                                               int64_t chunks_per_shard, int64_t draw0, int64_t n_draw,
                                                               unsigned long long seed, int half_bits) {
    const int64_t n_work = n_draw * chunks_per_shard;
    for (int64_t w = blockIdx.x; w < n_work; w += gridDim.x) {
        const int64_t j = w / chunks_per_shard;
        const int64_t c = w - j * chunks_per_shard;
        const unsigned long long t = (unsigned long long)(draw0 + j);
        const unsigned long long epoch = t / (unsigned long long)n_shards;
        unsigned k[4];
        perm_round_keys(perm_epoch_key(seed, epoch), k);  // (uniform over the workgroup: a few dozen integer ops)
        const int64_t id = (int64_t)perm_at(t - epoch * (unsigned long long)n_shards, (unsigned long long)n_shards, half_bits, k);
        if (ids_out != nullptr && c == 0 && threadIdx.x == 0) ids_out[j] = (int)id;
        const float4* __restrict__ s = store + id * words_per_shard;
        float4* __restrict__ d = batch + j * words_per_shard;
        const int64_t w0 = c * COPY_WORDS;
        const int64_t w1 = w0 + COPY_WORDS < words_per_shard ? w0 + COPY_WORDS : words_per_shard;
        for (int64_t x = w0 + threadIdx.x; x < w1; x += 256) d[x] = s[x];
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" int r2l_store_append(const float* rows_in, int64_t n_rows, float* store, int64_t capacity_shards, int64_t first_shard,
                                int64_t rays_per_shard, uint64_t key, int shuffle, int64_t* n_written_out, void* stream) {
    R2L_REQUIRE(rows_in != nullptr && store != nullptr && n_written_out != nullptr, "r2l_store_append: a required pointer is NULL");
    R2L_REQUIRE(rays_per_shard > 0 && rays_per_shard % 4 == 0,
                "r2l_store_append: rays_per_shard must be positive and a multiple of 4 (a shard is a whole number of 16-byte words)");
    R2L_REQUIRE(n_rows >= 0 && n_rows < ((int64_t)1 << 60), "r2l_store_append: n_rows is negative");
    R2L_REQUIRE(capacity_shards >= 0 && first_shard >= 0, "r2l_store_append: capacity_shards / first_shard is negative");
    const int64_t m = n_rows / rays_per_shard;
    R2L_REQUIRE(m <= capacity_shards && first_shard <= capacity_shards - m,
                "r2l_store_append: first_shard + floor(n_rows / rays_per_shard) exceeds capacity_shards");
    *n_written_out = m;
    if (m == 0) return 0;
    const int64_t n_out = m * rays_per_shard;
    const int64_t n_tiles = (n_out + TILE_ROWS - 1) / TILE_ROWS;
    const unsigned grid = (unsigned)(n_tiles > 8192 ? 8192 : n_tiles);
    hipLaunchKernelGGL(r2l_store_append_kernel<false>, dim3(grid), dim3(TILE_ROWS), 0, (hipStream_t)stream, rows_in,
                       store + first_shard * rays_per_shard * 9, n_rows, n_out, perm_half_bits(n_rows), (unsigned long long)key,
                       shuffle != 0 ? 1 : 0, (const int64_t*)nullptr, (int64_t)0);
    R2L_CHECK(hipGetLastError());
    return 0;
}

// r2l_store_append of the M rows rows_in[idx[.]] without gathering them first: the same kernel, the permutation over M
extern "C" int r2l_store_append_live(const float* rows_in, int64_t n_rows, const int64_t* idx, int64_t M, float* store,
                                     int64_t capacity_shards, int64_t first_shard, int64_t rays_per_shard, uint64_t key, int shuffle,
                                     int64_t* n_written_out, void* stream) {
    R2L_REQUIRE(rows_in != nullptr && store != nullptr && n_written_out != nullptr, "r2l_store_append_live: a required pointer is NULL");
    R2L_REQUIRE(rays_per_shard > 0 && rays_per_shard % 4 == 0,
                "r2l_store_append_live: rays_per_shard must be positive and a multiple of 4 (a shard is a whole number of 16-byte words)");
    R2L_REQUIRE(n_rows >= 0 && n_rows < ((int64_t)1 << 60), "r2l_store_append_live: n_rows is negative");
    R2L_REQUIRE(M >= 0 && M < ((int64_t)1 << 60), "r2l_store_append_live: M is negative");
    R2L_REQUIRE(M == 0 || idx != nullptr, "r2l_store_append_live: idx is NULL");
    R2L_REQUIRE(capacity_shards >= 0 && first_shard >= 0, "r2l_store_append_live: capacity_shards / first_shard is negative");
    const int64_t m = M / rays_per_shard;
    R2L_REQUIRE(m <= capacity_shards && first_shard <= capacity_shards - m,
                "r2l_store_append_live: first_shard + floor(M / rays_per_shard) exceeds capacity_shards");
    *n_written_out = m;
    if (m == 0) return 0;
    const int64_t n_out = m * rays_per_shard;
    const int64_t n_tiles = (n_out + TILE_ROWS - 1) / TILE_ROWS;
    const unsigned grid = (unsigned)(n_tiles > 8192 ? 8192 : n_tiles);
    hipLaunchKernelGGL(r2l_store_append_kernel<true>, dim3(grid), dim3(TILE_ROWS), 0, (hipStream_t)stream, rows_in,
                       store + first_shard * rays_per_shard * 9, M, n_out, perm_half_bits(M), (unsigned long long)key,
                       shuffle != 0 ? 1 : 0, idx, n_rows);
    R2L_CHECK(hipGetLastError());
    return 0;
}

extern "C" int r2l_store_batch(const float* store, int64_t n_shards, int64_t rays_per_shard, int64_t draw0, int64_t n_draw,
                               uint64_t seed, float* batch, int32_t* ids_out, void* stream) {
    R2L_REQUIRE(store != nullptr && batch != nullptr, "r2l_store_batch: a required pointer is NULL (store / batch)");
    R2L_REQUIRE(rays_per_shard > 0 && rays_per_shard % 4 == 0,
                "r2l_store_batch: rays_per_shard must be positive and a multiple of 4 (a shard is a whole number of 16-byte words)");
    R2L_REQUIRE(n_shards >= 1 && n_shards <= 0x7fffffff, "r2l_store_batch: need 1 <= n_shards < 2^31 (ids are int32)");
    R2L_REQUIRE(n_draw >= 0, "r2l_store_batch: n_draw is negative");
    R2L_REQUIRE(draw0 >= 0 && draw0 <= INT64_MAX - n_draw, "r2l_store_batch: draw0 is negative (or draw0 + n_draw overflows)");
    R2L_REQUIRE(aligned16(store) && aligned16(batch), "r2l_store_batch: store and batch must be 16-byte aligned");
    if (n_draw == 0) return 0;
    const int64_t words = rays_per_shard / 4 * 9;  // 36 B per row
    const int64_t chunks = (words + COPY_WORDS - 1) / COPY_WORDS;
    const int64_t n_work = n_draw * chunks;
    const unsigned grid = (unsigned)(n_work > 16384 ? 16384 : n_work);
    hipLaunchKernelGGL(r2l_store_batch_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const float4*)store, (float4*)batch,
                       (int*)ids_out, n_shards, words, chunks, draw0, n_draw, (unsigned long long)seed, perm_half_bits(n_shards));
    R2L_CHECK(hipGetLastError());
    return 0;
}
