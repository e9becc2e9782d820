// r2l_student_step.hip — one student training iteration in one library call (include/r2l_hip.h "one student training iteration").
//   r2l_train_batch:        the step's batch in ONE launch instead of r2l_store_batch -> r2l_pool_pick -> r2l_pool_augment: the rows of
//                           the drawn shards de-interleaved from the store's 9-float rows into contiguous o / d / t, the picked pool
//                           rows behind them.  Same sampler (pi, epoch_key of r2l_perm.h), same row choice, same bits.
//   r2l_student_train_step: the stages of r2l_amd/train_step.py (RayStore.next -> HardRayPool.augment -> draw_uniform ->
//                           R2LTrainer.step -> HardRayPool.update) in that order — batch -> jitter -> [re-pack] -> forward with stash
//                           -> zero the gradient -> backward -> loss finish -> Adam -> pool select + store — the EXISTING kernels with
//                           their existing arguments, enqueued back to back on the caller's stream through one work buffer the caller
//                           sized once: no allocation, no host synchronisation, no state.
// r2l_train_batch is the only kernel of this file.  A thread takes four consecutive rows of a shard — 36 floats = nine 16-byte words,
// aligned because a shard is a whole number of such groups — and writes three 16-byte words to each output; one thread per pool row
// behind them.  The batch is at most a few MB: the launch is latency-bound, nothing here is tuned beyond the vector accesses.
#include "r2l_common.h"
#include "r2l_dispatch.h"
#include "r2l_perm.h"

namespace {

__global__ __launch_bounds__(256) void r2l_train_batch_kernel(const float4* __restrict__ store, const float* __restrict__ pool,
                                                               float4* __restrict__ oo, float4* __restrict__ od, float4* __restrict__ ot,
                                                               int* __restrict__ ids_out, int64_t* __restrict__ idx_out, int64_t n_shards,
                                                               int64_t groups_per_shard, int64_t n_groups, int64_t draw0,
                                                               unsigned long long seed, int shard_half_bits, int64_t B, int64_t n_out,
                                                               int64_t n_pool_rows, int pool_half_bits, unsigned long long pool_key) {
    const int64_t total = n_groups + n_out;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (int64_t)gridDim.x * blockDim.x) {
        unsigned k[4];
        if (q < n_groups) {  // rows 4 g .. 4 g + 3 of draw j
            const int64_t j = q / groups_per_shard;
            const int64_t g = q - j * groups_per_shard;
            const unsigned long long t = (unsigned long long)(draw0 + j);
            const unsigned long long epoch = t / (unsigned long long)n_shards;
            perm_round_keys(perm_epoch_key(seed, epoch), k);
            const int64_t id = (int64_t)perm_at(t - epoch * (unsigned long long)n_shards, (unsigned long long)n_shards, shard_half_bits, k);
            if (ids_out != nullptr && g == 0) ids_out[j] = (int)id;
            const float4* __restrict__ s = store + (id * groups_per_shard + g) * 9;
            float f[36];
#pragma unroll
            for (int w = 0; w < 9; ++w) {
                const float4 v = s[w];
                f[4 * w] = v.x; f[4 * w + 1] = v.y; f[4 * w + 2] = v.z; f[4 * w + 3] = v.w;
            }
            const int64_t at = q * 3;  // 16-byte words: 12 floats of each output per group
#pragma unroll
            for (int w = 0; w < 3; ++w) {  // word w of an output = its floats 4 w .. 4 w + 3; float e = column e % 3 of row e / 3
                float a[4], b[4], c[4];
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    const int e = 4 * w + x, src = (e / 3) * 9 + e % 3;
                    a[x] = f[src]; b[x] = f[src + 3]; c[x] = f[src + 6];
                }
                oo[at + w] = make_float4(a[0], a[1], a[2], a[3]);
                od[at + w] = make_float4(b[0], b[1], b[2], b[3]);
                ot[at + w] = make_float4(c[0], c[1], c[2], c[3]);
            }
        } else {  // pool row i behind the batch
            const int64_t i = q - n_groups;
            perm_round_keys(pool_key, k);
            const int64_t idx = (int64_t)perm_at((unsigned long long)i, (unsigned long long)n_pool_rows, pool_half_bits, k);
            idx_out[i] = idx;
            const float* __restrict__ p = pool + idx * 9;
            float* __restrict__ o = reinterpret_cast<float*>(oo) + (B + i) * 3;
            float* __restrict__ d = reinterpret_cast<float*>(od) + (B + i) * 3;
            float* __restrict__ tt = reinterpret_cast<float*>(ot) + (B + i) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                o[c] = p[c]; d[c] = p[3 + c]; tt[c] = p[6 + c];
            }
        }
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
constexpr int64_t MAX_RAYS = ((int64_t)1 << 31) - 1;  // of a step: r2l_pool_select ranks fewer than 2^31 rows

// ---- the descriptor ------------------------------------------------------------------------------------------------------------
const char* step_desc_check(const r2l_student_step_desc* d) {
    if (d == nullptr) return "r2l_student_step_desc: desc is NULL";
    if (d->n_block < 0 || d->n_block > R2L_MAX_BLOCKS) return "r2l_student_step_desc.n_block: need 0 <= n_block <= 1024";
    if (const char* why = r2l_cfg_check(d->cfg)) return why;
    if (d->rays_per_shard < 1 || d->rays_per_shard % 4 != 0)
        return "r2l_student_step_desc.rays_per_shard: must be positive and a multiple of 4";
    if (d->n_shards < 1 || d->n_shards > 0x7fffffff) return "r2l_student_step_desc.n_shards: need 1 <= n_shards < 2^31";
    if (d->n_draw < 1) return "r2l_student_step_desc.n_draw: need n_draw >= 1";
    if (d->draw0 < 0 || d->draw0 > INT64_MAX - d->n_draw) return "r2l_student_step_desc.draw0: need draw0 >= 0";
    if (d->n_draw > MAX_RAYS / d->rays_per_shard) return "r2l_student_step_desc.n_draw: n_draw * rays_per_shard must stay below 2^31";
    if (d->perturb != 0 && d->perturb != 1) return "r2l_student_step_desc.perturb: 0 or 1";
    if (d->pack != 0 && d->pack != 1) return "r2l_student_step_desc.pack: 0 or 1";
    if (d->pool_full != 0 && d->pool_full != 1) return "r2l_student_step_desc.pool_full: 0 or 1";
    const int64_t B = d->n_draw * d->rays_per_shard;
    if (d->n_in < 0) return "r2l_student_step_desc.n_in: need n_in >= 0";
    if (d->n_out < 0 || d->n_out > MAX_RAYS - B) return "r2l_student_step_desc.n_out: need n_out >= 0 and fewer than 2^31 rays per step";
    if (d->pool_rows < 0 || d->pool_capacity_rows < 0 || d->pool_rows > d->pool_capacity_rows ||
        d->pool_capacity_rows >= ((int64_t)1 << 60))
        return "r2l_student_step_desc.pool_rows: need 0 <= pool_rows <= pool_capacity_rows";
    if (d->n_in > d->n_out) return "r2l_student_step_desc.n_in: need n_in <= n_out";
    if (d->n_in > B) return "r2l_student_step_desc.n_in: need n_in <= n_draw * rays_per_shard";
    if (!d->pool_full && d->n_in > d->pool_capacity_rows - d->pool_rows)
        return "r2l_student_step_desc.pool_rows: pool_rows + n_in exceeds pool_capacity_rows (pool not full)";
    if (d->pool_full && d->n_out > d->pool_rows) return "r2l_student_step_desc.n_out: exceeds pool_rows (pool full)";
    if (d->step < 1 || d->step >= ((int64_t)1 << 60)) return "r2l_student_step_desc.step: need 1 <= step < 2^60 (iterations count from 1)";
    if (d->reserved[0] || d->reserved[1] || d->reserved[2] || d->reserved[3]) return "r2l_student_step_desc.reserved: must be 0";
    return nullptr;
}

// The work buffer: every part starts on a 4 KiB boundary of it (the stash rows of the weight-gradient GEMMs are 1 KiB: DESIGN.md §8).
struct StepWork {
    int64_t o, d, t, trand, rgb, save_x, save_t, gx, gt, dpre, sqerr, slab, idx, hard, sel, total;
};
StepWork step_work(const r2l_student_step_desc* d) {
    const int64_t B = d->n_draw * d->rays_per_shard;
    const int64_t N = B + (d->pool_full ? d->n_out : 0);
    const int64_t slot = r2l_stash_slot_floats(N), nb = d->n_block;
    StepWork w{};
    int64_t at = 0;
    auto take = [&](int64_t n) { const int64_t a = at; at += (n + 1023) & ~(int64_t)1023; return a; };
    w.o = take(N * 3); w.d = take(N * 3); w.t = take(N * 3);
    w.trand = take(d->perturb ? N * 16 : 0);
    w.rgb = take(N * 3);
    w.save_x = take((nb + 1) * slot);
    w.save_t = take((nb > 0 ? nb : 1) * slot);
    w.gx = take((nb + 1) * slot);
    w.gt = take((nb > 0 ? nb : 1) * slot);
    w.dpre = take(N * 3);
    w.sqerr = take(r2l_num_tiles(N));
    w.slab = take(r2l_dw_slab_floats());
    w.idx = take(d->pool_full ? 2 * d->n_out : 0);  // int64
    w.hard = take(2 * d->n_in);                     // int64
    w.sel = take(d->n_in > 0 ? (r2l_pool_select_work_bytes(B) + 3) / 4 : 0);
    w.total = at;
    return w;
}

}  // namespace

extern "C" int r2l_train_batch(const float* store, int64_t n_shards, int64_t rays_per_shard, int64_t draw0, int64_t n_draw,
                               uint64_t seed, const float* pool, int64_t n_pool_rows, int64_t n_out, uint64_t pool_key, float* out_o,
                               float* out_d, float* out_t, int32_t* ids_out, int64_t* idx_out, void* stream) {
    R2L_REQUIRE(rays_per_shard > 0 && rays_per_shard % 4 == 0,
                "r2l_train_batch: rays_per_shard must be positive and a multiple of 4 (a shard is a whole number of 16-byte words)");
    R2L_REQUIRE(n_shards >= 1 && n_shards <= 0x7fffffff, "r2l_train_batch: need 1 <= n_shards < 2^31 (ids are int32)");
    R2L_REQUIRE(n_draw >= 0 && n_draw <= ((int64_t)1 << 56) / rays_per_shard, "r2l_train_batch: n_draw is negative (or the batch too large)");
    R2L_REQUIRE(draw0 >= 0 && draw0 <= INT64_MAX - n_draw, "r2l_train_batch: draw0 is negative (or draw0 + n_draw overflows)");
    R2L_REQUIRE(n_pool_rows >= 0 && n_pool_rows < ((int64_t)1 << 60) && n_out >= 0 && n_out <= n_pool_rows,
                "r2l_train_batch: need 0 <= n_out <= n_pool_rows");
    if (n_draw == 0 && n_out == 0) return 0;
    R2L_REQUIRE(out_o != nullptr && out_d != nullptr && out_t != nullptr, "r2l_train_batch: an output is NULL (out_o / out_d / out_t)");
    R2L_REQUIRE(n_draw == 0 || store != nullptr, "r2l_train_batch: store is NULL");
    R2L_REQUIRE(n_out == 0 || (pool != nullptr && idx_out != nullptr), "r2l_train_batch: pool / idx_out is NULL with n_out > 0");
    R2L_REQUIRE(aligned16(store) && aligned16(out_o) && aligned16(out_d) && aligned16(out_t),
                "r2l_train_batch: store, out_o, out_d and out_t must be 16-byte aligned");
    const int64_t gps = rays_per_shard / 4, n_groups = n_draw * gps, total = n_groups + n_out;
    const int64_t blocks = (total + 255) / 256;
    hipLaunchKernelGGL(r2l_train_batch_kernel, dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)store, pool, (float4*)out_o, (float4*)out_d, (float4*)out_t, (int*)ids_out, idx_out, n_shards, gps,
                       n_groups, draw0, (unsigned long long)seed, perm_half_bits(n_shards), n_draw * rays_per_shard, n_out, n_pool_rows,
                       perm_half_bits(n_pool_rows), (unsigned long long)pool_key);
    R2L_CHECK(hipGetLastError());
    return 0;
}

extern "C" int64_t r2l_student_step_work_floats(const r2l_student_step_desc* d) {
    if (const char* why = step_desc_check(d)) {
        r2l_set_error_msg(why);
        return -1;
    }
    return step_work(d).total;
}

extern "C" int r2l_student_train_step(const r2l_student_step_desc* d, const float* store, float* pool, const float* ztab, float* params,
                                      float* grads, float* exp_avg, float* exp_avg_sq, float* wstream, float* wstream_bwd,
                                      float* loss_out, float* rgb_out, float* work, void* stream) {
    if (const char* why = step_desc_check(d)) {
        r2l_set_error_msg(why);
        return (int)hipErrorInvalidValue;
    }
    const int64_t B = d->n_draw * d->rays_per_shard;
    const int64_t n_out = d->pool_full ? d->n_out : 0;
    const int64_t N = B + n_out;
    R2L_REQUIRE(store != nullptr, "r2l_student_train_step: store is NULL");
    R2L_REQUIRE(pool != nullptr || (n_out == 0 && d->n_in == 0), "r2l_student_train_step: pool is NULL (needed with n_in > 0, or n_out > 0 and pool_full)");
    R2L_REQUIRE(ztab != nullptr, "r2l_student_train_step: ztab is NULL");
    R2L_REQUIRE(params != nullptr, "r2l_student_train_step: params is NULL");
    R2L_REQUIRE(grads != nullptr, "r2l_student_train_step: grads is NULL");
    R2L_REQUIRE(exp_avg != nullptr, "r2l_student_train_step: exp_avg is NULL");
    R2L_REQUIRE(exp_avg_sq != nullptr, "r2l_student_train_step: exp_avg_sq is NULL");
    R2L_REQUIRE(wstream != nullptr, "r2l_student_train_step: wstream is NULL");
    R2L_REQUIRE(wstream_bwd != nullptr, "r2l_student_train_step: wstream_bwd is NULL");
    R2L_REQUIRE(loss_out != nullptr, "r2l_student_train_step: loss_out is NULL");
    R2L_REQUIRE(work != nullptr, "r2l_student_train_step: work is NULL");
    R2L_REQUIRE(((uintptr_t)work & 15) == 0, "r2l_student_train_step: work must be 16-byte aligned");
    R2L_REQUIRE(aligned16(store), "r2l_student_train_step: store must be 16-byte aligned");

    const hipStream_t st = (hipStream_t)stream;
    const StepWork w = step_work(d);
    const int nb = d->n_block;
    float *const o = work + w.o, *const dd = work + w.d, *const t = work + w.t;
    float* const rgb = rgb_out != nullptr ? rgb_out : work + w.rgb;
    int64_t* const idx = n_out > 0 ? reinterpret_cast<int64_t*>(work + w.idx) : nullptr;
    int rc;

    if ((rc = r2l_train_batch(store, d->n_shards, d->rays_per_shard, d->draw0, d->n_draw, d->store_seed, pool, d->pool_rows, n_out,
                              d->pool_key, o, dd, t, nullptr, idx, stream)))
        return rc;
    float* t_rand = nullptr;
    if (d->perturb) {
        t_rand = work + w.trand;
        if ((rc = r2l_draw_uniform(t_rand, N * 16, d->seed, d->jitter_stream, stream))) return rc;
    }
    if (d->pack) {  // in front of the step, as the trainer's lazy check does: on exit the streams hold the parameters the step READ
        if ((rc = r2l_pack_forward_layout(params, nb, wstream, r2l_forward_layout_for_cfg(N, 1, d->cfg), stream))) return rc;
        if ((rc = r2l_pack_backward_layout(params, nb, wstream_bwd, r2l_backward_layout_for_cfg(N, d->cfg), stream))) return rc;
    }
    if ((rc = r2l_forward_rays_cfg(o, dd, t_rand, ztab, wstream, params, nb, rgb, work + w.save_x, work + w.save_t, N, stream, d->cfg)))
        return rc;
    R2L_CHECK(hipMemsetAsync(grads, 0, (size_t)r2l_param_count(nb) * sizeof(float), st));
    const float grad_scale = (float)(2.0 * d->lw_rgb / (3.0 * (double)N));  // the staged path's doubles, then one rounding
    if ((rc = r2l_backward_part_cfg(o, dd, t_rand, ztab, nullptr, rgb, t, nullptr, work + w.save_x, work + w.save_t, wstream_bwd, params,
                                    nb, grad_scale, work + w.dpre, work + w.gx, work + w.gt, work + w.sqerr, grads, work + w.slab, N,
                                    stream, R2L_BWD_ALL, 0, 2 * nb, d->cfg)))
        return rc;
    if ((rc = r2l_loss_finish(work + w.sqerr, r2l_num_tiles(N), (float)(d->lw_rgb / (3.0 * (double)N)), loss_out, stream))) return rc;
    // Adam's bias corrections are 1 - beta^step: beyond 2^31 steps the power is 0 in double for every beta < 1 a run would use
    const int adam_step = d->step > 0x7fffffff ? 0x7fffffff : (int)d->step;
    if ((rc = r2l_adam_step_guarded(params, grads, exp_avg, exp_avg_sq, r2l_param_count(nb), d->lr, d->beta1, d->beta2, d->eps, adam_step,
                                    1.0f, nullptr, stream)))
        return rc;
    if (d->n_in > 0) {
        int64_t* const hard = reinterpret_cast<int64_t*>(work + w.hard);
        if ((rc = r2l_pool_select(rgb, t, 3, 3, B, d->n_in, hard, nullptr, work + w.sel, stream))) return rc;
        if ((rc = r2l_pool_store(o, dd, t, 3, 3, 3, hard, pool, d->pool_full ? idx : nullptr, d->pool_full ? 0 : d->pool_rows, d->n_in,
                                 stream)))
            return rc;
    }
    return 0;
}
