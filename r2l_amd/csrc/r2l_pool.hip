// Hard-ray pool on the device: the three data movements of /root/reference/main.py:1325-1347 (augment: n_hard_out random pool
// rows appended to every batch) and :1410-1425 (update: the hard_ratio * B rays with the largest per-ray error enter the pool,
// replacing the rows that were handed out) as ONE kernel each, plus the row choice.
//
// The reference draws `np.random.permutation(pool_rows)[:n_out]` on the host per step (1.6 M entries at the README sizes: a
// whole MI355X training step); rounds 1 - 3 used torch.randperm on the device — a 1.6 M-key radix sort, 0.16 ms per step, the
// largest single item of the CLI loop's overhead over the bare step (profiles/r04_e2e_train.txt).  All that is needed is n_out
// DISTINCT rows, every row equally likely: r2l_pool_pick evaluates a keyed bijection of [0, n_rows) — a 4-round Feistel network
// on the next even number of bits, cycle-walked back into the range — at i = 0 .. n_out-1.  A fresh key per step (host counter
// through a mixer) gives a fresh permutation; distinctness is by construction.  HBM-bound trivia otherwise: 36 B per row.
#include "r2l_common.h"
#include "r2l_perm.h"

namespace {

__global__ void r2l_pool_pick_kernel(int64_t* __restrict__ out, int64_t n_out, int64_t n_rows, int half_bits, unsigned long long key) {
    unsigned k[4];
    perm_round_keys(key, k);  // csrc/r2l_perm.h: the bijection is shared with the ray store
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_out; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = (int64_t)perm_at((unsigned long long)i, (unsigned long long)n_rows, half_bits, k);
}

// rows [0, B): the batch; rows [B, B + n_out): pool rows idx[i]; three contiguous [B + n_out, 3] outputs
__global__ void r2l_pool_augment_kernel(const float* __restrict__ o, const float* __restrict__ d, const float* __restrict__ t, int64_t so,
                                        int64_t sd, int64_t st, const float* __restrict__ pool, const int64_t* __restrict__ idx, int64_t B,
                                        int64_t n_out, float* __restrict__ oo, float* __restrict__ od, float* __restrict__ ot) {
    const int64_t total = (B + n_out) * 9;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = e / 9;
        const int c = (int)(e - row * 9);
        float v;
        if (row < B) v = c < 3 ? o[row * so + c] : (c < 6 ? d[row * sd + c - 3] : t[row * st + c - 6]);
        else v = pool[idx[row - B] * 9 + c];
        float* dst = c < 3 ? oo : (c < 6 ? od : ot);
        dst[row * 3 + (c % 3)] = v;
    }
}

// pool[dst(i)] = [o, d, t][hard[i]]  for i < n_in;  dst(i) = dst_idx[i] or dst0 + i
__global__ void r2l_pool_store_kernel(const float* __restrict__ o, const float* __restrict__ d, const float* __restrict__ t, int64_t so,
                                      int64_t sd, int64_t st, const int64_t* __restrict__ hard, float* __restrict__ pool,
                                      const int64_t* __restrict__ dst_idx, int64_t dst0, int64_t n_in) {
    const int64_t total = n_in * 9;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = e / 9;
        const int c = (int)(e - i * 9);
        const int64_t src = hard[i];
        const float v = c < 3 ? o[src * so + c] : (c < 6 ? d[src * sd + c - 3] : t[src * st + c - 6]);
        pool[(dst_idx != nullptr ? dst_idx[i] : dst0 + i) * 9 + c] = v;
    }
}

// ---- r2l_pool_select: the k rows with the largest per-ray squared error, by radix select ---------------------------------------
// Row i < B has the key bits(e_i), e_i = (d0*d0 + d1*d1) + d2*d2 of d = rgb[i] - target[i] (separately rounded fp32: the library
// is built without contraction; e_i >= +0, so the bit pattern orders like the value; NaN -> 0xFFFFFFFF).  The threshold key T —
// the k-th largest — is found one 8-bit digit at a time from the top: a 256-bin histogram of the digit over the rows that
// match the digits found so far, then the bin that holds the wanted rank.  One ordered compaction follows: every thread owns a
// contiguous run of rows, an exclusive scan of (rows above T, rows equal to T) over the threads gives every selected row its
// place, and of the rows equal to T the first k - count_above in index order are taken.  hard_out is in ascending index order
// and no position depends on the arrival order of an atomic: atomics only count.
//
// Histogram: the errors of a trained net sit in a handful of exponents, so the top digit has two or three hot bins.  A wave
// adds the counts of its two most common digits with one LDS atomic each (ballot), the lanes left over add their own.
//
// B <= SEL_SMALL_MAX (the per-GPU batches of training, 4096 - 12 288 rows): ONE launch of one workgroup, keys in LDS.
// Larger B: the keys go to `work`, and every step is a launch of its own over up to 1024 workgroups (keys + digit 3, digits
// 2 .. 0, count, compaction); the histograms of `work` are cleared by a memset node in the call.
constexpr int SEL_SMALL_MAX = 12288;
constexpr int SEL_SMALL_THREADS = 1024;
constexpr int SEL_THREADS = 256;
constexpr int SEL_MAX_BLOCKS = 1024;

__device__ __forceinline__ unsigned sel_key(const float* __restrict__ rgb, const float* __restrict__ tgt, int64_t srgb, int64_t st,
                                            int64_t i, float& e) {
    const float* a = rgb + i * srgb;
    const float* b = tgt + i * st;
    const float d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2];
    e = (d0 * d0 + d1 * d1) + d2 * d2;
    return e != e ? 0xFFFFFFFFu : __float_as_uint(e);
}

// called by whole waves (uniform control flow); hist: 256 LDS counters
__device__ __forceinline__ void sel_hist_add(unsigned* hist, bool valid, unsigned digit) {
    const int lane = threadIdx.x & 63;
    unsigned long long rem = __ballot(valid);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (rem == 0) break;  // (wave-uniform)
        const int leader = __ffsll((long long)rem) - 1;
        const unsigned d0 = __shfl(digit, leader);
        const unsigned long long m = __ballot(valid && digit == d0) & rem;
        if (lane == leader) atomicAdd(&hist[d0], (unsigned)__popcll(m));
        rem &= ~m;
    }
    if ((rem >> lane) & 1) atomicAdd(&hist[digit], 1u);
}

// hist[256] counts a digit over the rows still in play, krem (1 <= krem <= their number) is the wanted rank from the top:
// -> the digit whose bin holds that rank, and the rank inside the bin.  Whole workgroup (>= 256 threads), sh: 8 LDS words.
__device__ __forceinline__ void sel_resolve(const unsigned* hist, unsigned* sh, unsigned& krem, unsigned& digit) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const unsigned h = t < 256 ? hist[t] : 0u;
    unsigned s = h;  // sum of the bins t .. 255: a suffix scan, first inside the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned v = __shfl_down(s, off);
        if (lane + off < 64) s += v;
    }
    if (t < 256 && lane == 0) sh[w] = s;
    __syncthreads();
    if (t < 256) {
        for (int j = w + 1; j < 4; ++j) s += sh[j];
        if (s >= krem && s - h < krem) {  // exactly one bin: s does not increase with t
            sh[4] = (unsigned)t;
            sh[5] = krem - (s - h);
        }
    }
    __syncthreads();
    digit = sh[4];
    krem = sh[5];
    __syncthreads();
}

// exclusive scan of (a, e) over the workgroup's threads (<= 1024) and the totals.  sh: 32 LDS words.
__device__ __forceinline__ void sel_scan2(unsigned a, unsigned e, unsigned* sh, unsigned& a_pre, unsigned& e_pre, unsigned& a_tot,
                                          unsigned& e_tot) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, nw = blockDim.x >> 6;
    unsigned sa = a, se = e;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned va = __shfl_up(sa, off), ve = __shfl_up(se, off);
        if (lane >= off) {
            sa += va;
            se += ve;
        }
    }
    if (lane == 63) {
        sh[2 * w] = sa;
        sh[2 * w + 1] = se;
    }
    __syncthreads();
    unsigned ba = 0, be = 0, ta = 0, te = 0;
    for (int j = 0; j < nw; ++j) {
        const unsigned ua = sh[2 * j], ue = sh[2 * j + 1];
        if (j < w) {
            ba += ua;
            be += ue;
        }
        ta += ua;
        te += ue;
    }
    a_pre = ba + sa - a;
    e_pre = be + se - e;
    a_tot = ta;
    e_tot = te;
    __syncthreads();
}

// the selected rows of [lo, hi) in index order, from place a_pre + min(e_pre, need_eq) on
__device__ __forceinline__ void sel_emit(const unsigned* keys, int64_t lo, int64_t hi, unsigned T, unsigned need_eq, unsigned a_pre,
                                         unsigned e_pre, int64_t k, int64_t* __restrict__ hard) {
    int64_t pos = (int64_t)a_pre + (e_pre < need_eq ? e_pre : need_eq);
    for (int64_t i = lo; i < hi; ++i) {
        const unsigned key = keys[i];
        bool take = key > T;
        if (key == T) take = e_pre++ < need_eq;
        if (take && pos < k) hard[pos++] = i;
    }
}

__global__ __launch_bounds__(SEL_SMALL_THREADS) void r2l_pool_select_small_kernel(const float* __restrict__ rgb,
                                                                                  const float* __restrict__ tgt, int64_t srgb,
                                                                                  int64_t st, int B, int k,
                                                                                  int64_t* __restrict__ hard, float* __restrict__ err) {
    __shared__ unsigned keys[SEL_SMALL_MAX];
    __shared__ unsigned hist[256];
    __shared__ unsigned sh[32];
    const int t = threadIdx.x;
    if (t < 256) hist[t] = 0u;
    for (int i = t; i < B; i += SEL_SMALL_THREADS) {
        float e;
        keys[i] = sel_key(rgb, tgt, srgb, st, i, e);
        if (err != nullptr) err[i] = e;
    }
    __syncthreads();
    unsigned prefix = 0u, mask = 0u, krem = (unsigned)k;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int base = 0; base < B; base += SEL_SMALL_THREADS) {
            const int i = base + t;
            const unsigned key = i < B ? keys[i] : 0u;
            sel_hist_add(hist, i < B && (key & mask) == prefix, (key >> shift) & 255u);
        }
        __syncthreads();
        unsigned digit;
        sel_resolve(hist, sh, krem, digit);
        prefix |= digit << shift;
        mask |= 255u << shift;
        if (t < 256) hist[t] = 0u;
        __syncthreads();
    }
    // prefix = T, krem = how many of the rows equal to T are taken
    const int per = (B + SEL_SMALL_THREADS - 1) / SEL_SMALL_THREADS;
    const int lo = min(t * per, B), hi = min(lo + per, B);
    unsigned a = 0, e = 0;
    for (int i = lo; i < hi; ++i) {
        a += keys[i] > prefix;
        e += keys[i] == prefix;
    }
    unsigned a_pre, e_pre, a_tot, e_tot;
    sel_scan2(a, e, sh, a_pre, e_pre, a_tot, e_tot);
    sel_emit(keys, lo, hi, prefix, krem, a_pre, e_pre, k, hard);
}

// ---- many workgroups: workgroup b owns the rows [b * chunk, (b + 1) * chunk) in every launch --------------------------------
struct SelWork {
    unsigned* keys;   // [B]
    unsigned* ghist;  // [4][256], cleared by the call
    unsigned* cnt;    // [gridDim.x][2]: rows above T / equal to T per workgroup
};

// T's digits above `shift` from the finished histograms: (prefix, mask, krem) as the one-workgroup kernel carries them
__device__ __forceinline__ void sel_resolve_upto(const unsigned* ghist, int n_pass, unsigned* sh, unsigned& prefix, unsigned& mask,
                                                 unsigned& krem) {
    prefix = 0u;
    mask = 0u;
    for (int p = 0; p < n_pass; ++p) {
        unsigned digit;
        sel_resolve(ghist + 256 * p, sh, krem, digit);
        prefix |= digit << (24 - 8 * p);
        mask |= 255u << (24 - 8 * p);
    }
}

// pass 0: keys (and err_out) + the histogram of the top digit; pass 1 .. 3: the histogram of digit 3 - pass
__global__ __launch_bounds__(SEL_THREADS) void r2l_pool_select_hist_kernel(const float* __restrict__ rgb, const float* __restrict__ tgt,
                                                                           int64_t srgb, int64_t st, int64_t B, int64_t k,
                                                                           int64_t chunk, int pass, SelWork wk, float* __restrict__ err) {
    __shared__ unsigned hist[256];
    __shared__ unsigned sh[8];
    const int t = threadIdx.x;
    hist[t] = 0u;
    unsigned prefix, mask, krem = (unsigned)k;
    sel_resolve_upto(wk.ghist, pass, sh, prefix, mask, krem);  // (its barriers also publish the cleared hist)
    if (pass == 0) __syncthreads();
    const int shift = 24 - 8 * pass;
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < B ? lo + chunk : B;
    for (int64_t base = lo; base < hi; base += SEL_THREADS) {
        const int64_t i = base + t;
        unsigned key = 0u;
        if (i < hi) {
            if (pass == 0) {
                float e;
                key = sel_key(rgb, tgt, srgb, st, i, e);
                wk.keys[i] = key;
                if (err != nullptr) err[i] = e;
            } else {
                key = wk.keys[i];
            }
        }
        sel_hist_add(hist, i < hi && (key & mask) == prefix, (key >> shift) & 255u);
    }
    __syncthreads();
    if (hist[t] != 0u) atomicAdd(&wk.ghist[256 * pass + t], hist[t]);
}

// emit == 0: this workgroup's (above, equal) counts; emit == 1: the compaction
__global__ __launch_bounds__(SEL_THREADS) void r2l_pool_select_compact_kernel(int64_t B, int64_t k, int64_t chunk, int emit, SelWork wk,
                                                                              int64_t* __restrict__ hard) {
    __shared__ unsigned sh[32];
    const int t = threadIdx.x;
    unsigned T, mask, need_eq = (unsigned)k;
    sel_resolve_upto(wk.ghist, 4, sh, T, mask, need_eq);
    const int64_t per = chunk / SEL_THREADS;
    const int64_t end = (int64_t)blockIdx.x * chunk + chunk < B ? (int64_t)blockIdx.x * chunk + chunk : B;
    int64_t lo = (int64_t)blockIdx.x * chunk + t * per;
    lo = lo < end ? lo : end;
    const int64_t hi = lo + per < end ? lo + per : end;
    unsigned a = 0, e = 0;
    for (int64_t i = lo; i < hi; ++i) {
        const unsigned key = wk.keys[i];
        a += key > T;
        e += key == T;
    }
    unsigned a_pre, e_pre, a_tot, e_tot;
    sel_scan2(a, e, sh, a_pre, e_pre, a_tot, e_tot);
    if (!emit) {
        if (t == 0) {
            wk.cnt[2 * blockIdx.x] = a_tot;
            wk.cnt[2 * blockIdx.x + 1] = e_tot;
        }
        return;
    }
    unsigned ba = 0, be = 0;  // the workgroups in front of this one
    for (int j = t; j < (int)blockIdx.x; j += SEL_THREADS) {
        ba += wk.cnt[2 * j];
        be += wk.cnt[2 * j + 1];
    }
    unsigned pa, pe, ta, te;
    sel_scan2(ba, be, sh, pa, pe, ta, te);
    sel_emit(wk.keys, lo, hi, T, need_eq, ta + a_pre, te + e_pre, k, hard);
}

int64_t sel_chunk(int64_t B) {  // rows per workgroup: a multiple of 1024, at most SEL_MAX_BLOCKS workgroups
    const int64_t c = ((B + SEL_MAX_BLOCKS - 1) / SEL_MAX_BLOCKS + 1023) / 1024 * 1024;
    return c < 1024 ? 1024 : c;
}

unsigned grid_for(int64_t total) {
    int64_t g = (total + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

}  // namespace

extern "C" int r2l_pool_pick(int64_t* idx_out, int64_t n_out, int64_t n_rows, uint64_t key, void* stream) {
    R2L_REQUIRE(n_out >= 0 && n_rows >= 0 && n_out <= n_rows && n_rows < ((int64_t)1 << 60), "r2l_pool_pick: need 0 <= n_out <= n_rows");
    if (n_out == 0) return 0;
    R2L_REQUIRE(idx_out != nullptr, "r2l_pool_pick: idx_out is NULL");
    hipLaunchKernelGGL(r2l_pool_pick_kernel, dim3(grid_for(n_out)), dim3(256), 0, (hipStream_t)stream, idx_out, n_out, n_rows,
                       perm_half_bits(n_rows), (unsigned long long)key);
    R2L_CHECK(hipGetLastError());
    return 0;
}

extern "C" int r2l_pool_augment(const float* rays_o, const float* rays_d, const float* target, int64_t stride_o, int64_t stride_d,
                                int64_t stride_t, const float* pool, const int64_t* idx, int64_t B, int64_t n_out, float* out_o,
                                float* out_d, float* out_t, void* stream) {
    R2L_REQUIRE(B >= 0 && n_out >= 0, "r2l_pool_augment: negative B / n_out");
    if (B + n_out == 0) return 0;
    R2L_REQUIRE((B == 0 || (rays_o && rays_d && target)) && (n_out == 0 || (pool && idx)) && out_o && out_d && out_t,
                "r2l_pool_augment: a required pointer is NULL");
    hipLaunchKernelGGL(r2l_pool_augment_kernel, dim3(grid_for((B + n_out) * 9)), dim3(256), 0, (hipStream_t)stream, rays_o, rays_d, target,
                       stride_o, stride_d, stride_t, pool, idx, B, n_out, out_o, out_d, out_t);
    R2L_CHECK(hipGetLastError());
    return 0;
}

extern "C" int r2l_pool_store(const float* rays_o, const float* rays_d, const float* target, int64_t stride_o, int64_t stride_d,
                              int64_t stride_t, const int64_t* hard, float* pool, const int64_t* dst_idx, int64_t dst0, int64_t n_in,
                              void* stream) {
    R2L_REQUIRE(n_in >= 0 && dst0 >= 0, "r2l_pool_store: negative n_in / dst0");
    if (n_in == 0) return 0;
    R2L_REQUIRE(rays_o && rays_d && target && hard && pool, "r2l_pool_store: a required pointer is NULL");
    hipLaunchKernelGGL(r2l_pool_store_kernel, dim3(grid_for(n_in * 9)), dim3(256), 0, (hipStream_t)stream, rays_o, rays_d, target, stride_o,
                       stride_d, stride_t, hard, pool, dst_idx, dst0, n_in);
    R2L_CHECK(hipGetLastError());
    return 0;
}

extern "C" int64_t r2l_pool_select_work_bytes(int64_t B) {
    if (B < 0 || B >= ((int64_t)1 << 31)) {
        r2l_set_error_msg("r2l_pool_select_work_bytes: need 0 <= B < 2^31");
        return -1;
    }
    if (B <= SEL_SMALL_MAX) return 16;  // (nothing is kept there: one workgroup ranks out of LDS)
    return ((B + 3) / 4 * 4 + 4 * 256 + 2 * SEL_MAX_BLOCKS) * (int64_t)sizeof(unsigned);
}

extern "C" int r2l_pool_select(const float* rgb, const float* target, int64_t stride_rgb, int64_t stride_t, int64_t B, int64_t k,
                               int64_t* hard_out, float* err_out, void* work, void* stream) {
    R2L_REQUIRE(B >= 0 && B < ((int64_t)1 << 31), "r2l_pool_select: need 0 <= B < 2^31");
    R2L_REQUIRE(k >= 0 && k <= B, "r2l_pool_select: need 0 <= k <= B");
    R2L_REQUIRE(stride_rgb >= 3, "r2l_pool_select: stride_rgb is below 3 floats");
    R2L_REQUIRE(stride_t >= 3, "r2l_pool_select: stride_t is below 3 floats");
    R2L_REQUIRE(rgb != nullptr, "r2l_pool_select: rgb is NULL");
    R2L_REQUIRE(target != nullptr, "r2l_pool_select: target is NULL");
    R2L_REQUIRE(hard_out != nullptr || k == 0, "r2l_pool_select: hard_out is NULL");
    R2L_REQUIRE(work != nullptr, "r2l_pool_select: work is NULL");
    R2L_REQUIRE(((uintptr_t)work & 15) == 0, "r2l_pool_select: work is not 16-byte aligned");
    if (B == 0 || k == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (B <= SEL_SMALL_MAX) {
        hipLaunchKernelGGL(r2l_pool_select_small_kernel, dim3(1), dim3(SEL_SMALL_THREADS), 0, s, rgb, target, stride_rgb, stride_t,
                           (int)B, (int)k, hard_out, err_out);
        R2L_CHECK(hipGetLastError());
        return 0;
    }
    const int64_t chunk = sel_chunk(B);
    const unsigned nb = (unsigned)((B + chunk - 1) / chunk);
    SelWork wk;
    wk.keys = (unsigned*)work;
    wk.ghist = wk.keys + (B + 3) / 4 * 4;
    wk.cnt = wk.ghist + 4 * 256;
    R2L_CHECK(hipMemsetAsync(wk.ghist, 0, 4 * 256 * sizeof(unsigned), s));
    for (int pass = 0; pass < 4; ++pass) {
        hipLaunchKernelGGL(r2l_pool_select_hist_kernel, dim3(nb), dim3(SEL_THREADS), 0, s, rgb, target, stride_rgb, stride_t, B, k,
                           chunk, pass, wk, err_out);
        R2L_CHECK(hipGetLastError());
    }
    for (int emit = 0; emit < 2; ++emit) {
        hipLaunchKernelGGL(r2l_pool_select_compact_kernel, dim3(nb), dim3(SEL_THREADS), 0, s, B, k, chunk, emit, wk, hard_out);
        R2L_CHECK(hipGetLastError());
    }
    return 0;
}
