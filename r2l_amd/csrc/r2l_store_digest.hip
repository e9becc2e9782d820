// Digest of a ray store's shards (include/r2l_hip.h r2l_words_digest): what RayStore.save writes beside the rows and what
// RayStore.load recomputes before a file is trained on.  Item k of words_per_item 32-bit words gets
//   out[k] = sum over i of epoch_key(((uint64)i << 32) | word[i], salt + k)   (mod 2^64)
// with epoch_key = perm_epoch_key of csrc/r2l_perm.h (the splitmix64 finalizer the sampler keys its epochs with).  The sum is an
// integer sum, so any reduction order gives the same bits: per thread a 64-bit accumulator, then the wave (shuffles), then the
// workgroup (LDS), then ONE 64-bit atomic add per workgroup into out[k], which the entry point zero-fills first.
// Work unit = (item, slice): a slice is DG_SLICE_VEC 16-byte words of the item's aligned body.  An item starts where
// words + k * words_per_item lands, which is 16-byte aligned for the rows of a store but not for a pose table of odd length:
// the 0-3 words before the first aligned address (head) and the 0-3 words behind the last whole 16-byte word (tail) are read
// one by one by the first lanes of slice 0; every other read is one 16-byte load, lane-contiguous.  Nothing outside
// [words + k * words_per_item, words + (k + 1) * words_per_item) is read, nothing but out[0 .. n_items) is written.
#include "r2l_common.h"
#include "r2l_perm.h"

namespace {

constexpr int DG_THREADS = 256;
constexpr int DG_PASS_VEC = DG_THREADS;        // 16-byte words per workgroup pass: 1024 words of 32 bits
constexpr int DG_SLICE_VEC = 16 * DG_PASS_VEC;  // 16-byte words per work unit: 64 KiB of an item
constexpr unsigned long long DG_GOLDEN = 0x9E3779B97F4A7C15ull;

// epoch_key(x, e) with c = (e + 1) * DG_GOLDEN hoisted: perm_epoch_key(x, e) == dg_term(x, c)
__device__ __forceinline__ unsigned long long dg_term(unsigned long long i, unsigned w, unsigned long long c) {
    unsigned long long z = ((i << 32) | (unsigned long long)w) + c;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ __launch_bounds__(DG_THREADS) void r2l_words_digest_kernel(const unsigned* __restrict__ words, int64_t wpi, int64_t n_items,
                                                                      int64_t slices, unsigned long long salt,
                                                                      unsigned long long* __restrict__ out) {
    __shared__ unsigned long long part[DG_THREADS / 64];
    const int64_t n_work = n_items * slices;
    for (int64_t u = blockIdx.x; u < n_work; u += gridDim.x) {  // (uniform over the workgroup: the barriers below are too)
        const int64_t k = u / slices;
        const int64_t s = u - k * slices;
        const unsigned* __restrict__ base = words + k * wpi;
        const unsigned long long c = (salt + (unsigned long long)k + 1ull) * DG_GOLDEN;
        // head: words before the first 16-byte aligned address (the pointer is 4-byte aligned: checked by the host)
        int64_t head = (int64_t)((16u - (unsigned)((uintptr_t)base & 15u)) & 15u) >> 2;
        if (head > wpi) head = wpi;
        const int64_t n_vec = (wpi - head) >> 2;
        const int64_t tail0 = head + (n_vec << 2);  // first word behind the aligned body; wpi - tail0 is 0..3
        unsigned long long acc = 0;
        const int64_t v0 = s * DG_SLICE_VEC;
        const int64_t v1 = v0 + DG_SLICE_VEC < n_vec ? v0 + DG_SLICE_VEC : n_vec;
        const uint4* __restrict__ body = reinterpret_cast<const uint4*>(base + head);
        for (int64_t v = v0 + threadIdx.x; v < v1; v += DG_THREADS) {
            const uint4 q = body[v];
            const unsigned long long i = (unsigned long long)(head + (v << 2));
            acc += dg_term(i, q.x, c) + dg_term(i + 1, q.y, c) + dg_term(i + 2, q.z, c) + dg_term(i + 3, q.w, c);
        }
        if (s == 0) {  // lanes 0-2: the head's words, lanes 4-6: the tail's
            const int64_t t = threadIdx.x;
            if (t < head) acc += dg_term((unsigned long long)t, base[t], c);
            if (t >= 4 && tail0 + (t - 4) < wpi && t < 8) acc += dg_term((unsigned long long)(tail0 + t - 4), base[tail0 + t - 4], c);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long sum = 0;
#pragma unroll
            for (int w = 0; w < DG_THREADS / 64; ++w) sum += part[w];
            if (v1 > v0 || s == 0) atomicAdd(out + k, sum);  // (a slice past this item's body has nothing to add)
        }
        __syncthreads();  // part is rewritten by the next unit
    }
}

}  // namespace

extern "C" int r2l_words_digest(const uint32_t* words, int64_t words_per_item, int64_t n_items, uint64_t salt, uint64_t* out,
                                void* stream) {
    R2L_REQUIRE(n_items >= 0, "r2l_words_digest: n_items is negative");
    R2L_REQUIRE(words_per_item >= 1 && words_per_item <= 0xffffffffll,
                "r2l_words_digest: words_per_item must be in [1, 2^32) (the word's position is the high half of what is hashed)");
    R2L_REQUIRE(n_items == 0 || (words != nullptr && out != nullptr), "r2l_words_digest: a required pointer is NULL (words, out)");
    R2L_REQUIRE(((uintptr_t)words & 3u) == 0, "r2l_words_digest: words must be 4-byte aligned");
    R2L_REQUIRE(((uintptr_t)out & 7u) == 0, "r2l_words_digest: out must be 8-byte aligned");
    R2L_REQUIRE(n_items <= INT64_MAX / words_per_item, "r2l_words_digest: n_items * words_per_item overflows 63 bits");
    if (n_items == 0) return 0;
    R2L_CHECK(hipMemsetAsync(out, 0, (size_t)n_items * sizeof(uint64_t), (hipStream_t)stream));
    // an item's aligned body has at most ceil(words_per_item / 4) 16-byte words; at least one slice (head and tail ride on slice 0)
    const int64_t vecs = (words_per_item + 3) / 4;
    const int64_t slices = (vecs + DG_SLICE_VEC - 1) / DG_SLICE_VEC;
    const int64_t n_work = n_items * slices;  // slices <= words_per_item: no overflow (checked above)
    const unsigned grid = (unsigned)(n_work > 32768 ? 32768 : n_work);  // the rest is the kernel's stride loop
    hipLaunchKernelGGL(r2l_words_digest_kernel, dim3(grid), dim3(DG_THREADS), 0, (hipStream_t)stream, (const unsigned*)words,
                       words_per_item, n_items, slices, (unsigned long long)salt, (unsigned long long*)out);
    R2L_CHECK(hipGetLastError());
    return 0;
}
