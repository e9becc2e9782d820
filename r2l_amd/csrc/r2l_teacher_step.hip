// r2l_teacher_step.hip — one teacher training step in one library call (include/r2l_hip.h "one teacher training step").
//   r2l_teacher_train_step: the stages of r2l_amd/teacher_train.py (TeacherTrainer.forward_backward + adam) in that order — stratified
//                           z -> coarse forward with stash -> raw2outputs (weights) -> sample_pdf + sort -> fine forward with stash ->
//                           raw2outputs backward + network backward + loss finish (fine, then coarse) -> Adam -> re-pack — the EXISTING
//                           kernels enqueued back to back on the caller's stream through one work buffer the caller sized once: no
//                           allocation, no host synchronisation, no state.  The random draws (t_rand, u, the sigma noise) are made
//                           here from counter-based streams of (seed, step): a C host reproduces a run, a resume needs no generator
// Two kernels of its own, one thread each: near / far into the work buffer (r2l_stratified_z reads them from the device), and the
// step's loss / psnr from the two nets' r2l_loss_finish results.
//   r2l_teacher_train_step_occ: the same body with each pass's forward replaced by r2l_occ_index -> r2l_teacher_mlp_train_live and each
//                           network backward by r2l_teacher_backward_live on the same idx / count (occupancy grids; the live counts
//                           stay on the device): still no allocation and no host synchronisation
#include "r2l_common.h"
#include <math.h>

namespace {

__global__ void r2l_step_nearfar_kernel(float* __restrict__ nf, float near, float far) {
    if (blockIdx.x == 0 && threadIdx.x == 0) { nf[0] = near; nf[1] = far; }
}

// loss = mse of the last net + mse of the coarse net (fp32, in the order of the staged path's sum), psnr of the last net;
// first == nullptr: one net
__global__ void r2l_step_loss_kernel(const float* __restrict__ last, const float* __restrict__ first, float* __restrict__ out) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        out[0] = first != nullptr ? last[0] + first[0] : last[0];
        out[1] = last[1];
    }
}

const char* step_desc_check(const r2l_teacher_step_desc* d) {
    if (d == nullptr) return "r2l_teacher_step_desc: desc is NULL";
    if (d->N_rand < 1) return "r2l_teacher_step_desc.N_rand: need N_rand >= 1";
    if (d->N_samples < 1) return "r2l_teacher_step_desc.N_samples: need N_samples >= 1";
    if (d->N_importance < 0) return "r2l_teacher_step_desc.N_importance: need N_importance >= 0";
    if (d->N_importance > 0 && d->N_samples < 3) return "r2l_teacher_step_desc.N_samples: need N_samples >= 3 with N_importance > 0";
    if ((int64_t)d->N_samples + d->N_importance > 256) return "r2l_teacher_step_desc.N_samples + .N_importance: at most 256";
    if (d->N_importance > 0 && (d->N_samples > 64 || d->N_importance > 192))
        return "r2l_teacher_step_desc.N_samples / .N_importance: r2l_sample_pdf_sort needs N_samples <= 64 and N_importance <= 192";
    if (d->perturb != 0 && d->perturb != 1) return "r2l_teacher_step_desc.perturb: 0 or 1";
    if (d->white_bkgd != 0 && d->white_bkgd != 1) return "r2l_teacher_step_desc.white_bkgd: 0 or 1";
    if (!(d->raw_noise_std >= 0.f) || !(d->raw_noise_std < INFINITY)) return "r2l_teacher_step_desc.raw_noise_std: need a finite raw_noise_std >= 0";
    if (!(d->near < d->far)) return "r2l_teacher_step_desc.near / .far: need near < far";
    if (d->step < 1 || d->step >= ((int64_t)1 << 60)) return "r2l_teacher_step_desc.step: need 1 <= step < 2^60 (iterations count from 1)";
    if (d->reserved[0] || d->reserved[1] || d->reserved[2] || d->reserved[3]) return "r2l_teacher_step_desc.reserved: must be 0";
    return nullptr;
}

// The work buffer: every part starts on a 4 KiB boundary of it.  16 bytes are what the kernels need (raw is stored as 16-byte words,
// the quarter-wave kernels of r2l_render.hip take aligned pointers, and r2l_sample_pdf_sort picks its kernel by the alignment of its
// arguments); the rest is for the GEMMs of the backward pass, whose 1 KiB stash rows should not straddle cache lines the way the
// staged path's separately allocated buffers never do.
struct StepWork {
    int64_t nearfar, z, raw_c, stash_c, rgb_c, s_c, draw, sqerr_c, sqerr_f, mse_c, mse_f, bwd, trand, noise_c;
    int64_t wts, zs, zall, raw_f, stash_f, u, noise_f, total;
    int64_t idx_c, count_c, idx_f, count_f, iwork;  // occupancy form only: int64 idx per sample and count (4) per pass, the index work
};
int64_t r4(int64_t n) { return (n + 3) & ~(int64_t)3; }
// occ: the layout of r2l_teacher_train_step_occ — the backward's scratch is r2l_teacher_backward_live's, and the parts of the two index
// lists follow the plain parts.  Without it the layout is the one r2l_teacher_train_step always had.
StepWork step_work(const r2l_teacher_step_desc* d, bool occ = false) {
    const int64_t R = d->N_rand, S = d->N_samples, NI = d->N_importance, T = S + NI;
    const bool noise = d->raw_noise_std > 0.f;
    StepWork w{};
    int64_t at = 0;
    auto take = [&](int64_t n) { const int64_t a = at; at += (n + 1023) & ~(int64_t)1023; return a; };
    w.nearfar = take(2);
    w.z = take(R * S);
    w.raw_c = take(R * S * 4);
    w.stash_c = take(r2l_teacher_stash_floats(R * S));
    w.rgb_c = take(R * 3); w.s_c = take(r4(R) * 3);  // rgb0 | disp0, acc0, depth0: r2l_raw2outputs writes them all
    w.draw = take(R * T * 4);                        // d loss / d raw of one net at a time
    w.sqerr_c = take(R); w.sqerr_f = take(NI > 0 ? R : 0);
    w.mse_c = take(2); w.mse_f = take(NI > 0 ? 2 : 0);
    w.bwd = take(occ ? r2l_teacher_train_live_work_floats(R * T) : r2l_teacher_train_work_floats(R * T));  // scratch of one net's backward at a time
    w.trand = take(d->perturb ? R * S : 0);
    w.noise_c = take(noise ? R * S : 0);
    w.wts = take(NI > 0 ? R * S : 0);
    w.zs = take(R * NI);
    w.zall = take(NI > 0 ? R * T : 0);
    w.raw_f = take(NI > 0 ? R * T * 4 : 0);
    w.stash_f = take(NI > 0 ? r2l_teacher_stash_floats(R * T) : 0);
    w.u = take(d->perturb ? R * NI : 0);
    w.noise_f = take(noise && NI > 0 ? R * T : 0);
    if (occ) {
        w.idx_c = take(2 * R * S); w.count_c = take(4);
        w.idx_f = take(NI > 0 ? 2 * R * T : 0); w.count_f = take(NI > 0 ? 4 : 0);
        w.iwork = take((r2l_occ_index_work_bytes(R * T) + 3) / 4);  // (R*T < 65535 * 128 < 2^31: step_occ_desc_check)
    }
    w.total = at;
    return w;
}

// what the occupancy form asks of a valid descriptor beyond step_desc_check, or nullptr
const char* step_occ_desc_check(const r2l_teacher_step_desc* d) {
    if (d->raw_noise_std > 0.f)
        return "r2l_teacher_train_step_occ: r2l_teacher_step_desc.raw_noise_std must be 0 (noise can lift a skipped sample above zero)";
    if ((int64_t)d->N_rand * ((int64_t)d->N_samples + d->N_importance) >= (int64_t)65535 * 128)
        return "r2l_teacher_train_step_occ: r2l_teacher_step_desc.N_rand: too many samples for one call (need N_rand * (N_samples + "
               "N_importance) < 65535 * 128)";
    return nullptr;
}

// The grids of the occupancy form, or none: the ONE body below serves both entry points
struct StepOcc {
    const r2l_occ_grid *coarse, *fine;
    int64_t* live_acc;
};

int step_body(const r2l_teacher_step_desc* d, const float* rays_o, const float* rays_d, const float* viewdirs, const float* target,
              const float* ttab, const float* u_det, float* params, float* grads, float* exp_avg, float* exp_avg_sq, float* wstream_coarse,
              float* wstream_fine, float* loss_out, float* work, void* stream, const StepOcc* occ);

// The forward with stash of one pass: the plain launch, or (occupancy form) index -> [live_acc] -> the live launch
int step_forward(const float* o, const float* dd, const float* v, const float* z, const float* wstream, const float* tparams, float* raw,
                 float* stash, int64_t R, int S, void* stream, const r2l_occ_grid* grid, const StepOcc* occ, int64_t* idx, int64_t* count,
                 void* iwork) {
    if (occ == nullptr) return r2l_teacher_mlp_train(o, dd, v, z, wstream, tparams, raw, stash, R, S, stream);
    int rc;
    if ((rc = r2l_occ_index(grid, o, dd, z, R, S, idx, count, iwork, stream))) return rc;
    if (occ->live_acc != nullptr && (rc = r2l_occ_live_add(count, R * (int64_t)S, occ->live_acc, stream))) return rc;
    return r2l_teacher_mlp_train_live(o, dd, v, z, idx, count, wstream, tparams, raw, stash, R, S, stream);
}

// The network backward of one pass: the plain chain, or the live one on the pass's idx / count
int step_backward(const float* o, const float* dd, const float* v, const float* z, const float* tparams, const float* stash,
                  const float* draw, float* grads, float* work, int64_t R, int S, void* stream, const StepOcc* occ, const int64_t* idx,
                  const int64_t* count) {
    if (occ == nullptr) return r2l_teacher_backward(o, dd, v, z, tparams, stash, draw, grads, work, R, S, stream);
    return r2l_teacher_backward_live(o, dd, v, z, idx, count, tparams, stash, draw, grads, work, R, S, stream);
}

}  // namespace

extern "C" int64_t r2l_teacher_step_work_floats(const r2l_teacher_step_desc* d) {
    if (const char* why = step_desc_check(d)) {
        r2l_set_error_msg(why);
        return -1;
    }
    return step_work(d).total;
}

extern "C" int r2l_teacher_train_step(const r2l_teacher_step_desc* d, const float* rays_o, const float* rays_d, const float* viewdirs,
                                      const float* target, const float* ttab, const float* u_det, float* params, float* grads,
                                      float* exp_avg, float* exp_avg_sq, float* wstream_coarse, float* wstream_fine, float* loss_out,
                                      float* work, void* stream) {
    return step_body(d, rays_o, rays_d, viewdirs, target, ttab, u_det, params, grads, exp_avg, exp_avg_sq, wstream_coarse, wstream_fine,
                     loss_out, work, stream, nullptr);
}

extern "C" int64_t r2l_teacher_step_occ_work_floats(const r2l_teacher_step_desc* d) {
    if (const char* why = step_desc_check(d)) {
        r2l_set_error_msg(why);
        return -1;
    }
    if (const char* why = step_occ_desc_check(d)) {
        r2l_set_error_msg(why);
        return -1;
    }
    return step_work(d, true).total;
}

extern "C" int r2l_teacher_train_step_occ(const r2l_teacher_step_desc* d, const float* rays_o, const float* rays_d, const float* viewdirs,
                                          const float* target, const float* ttab, const float* u_det, float* params, float* grads,
                                          float* exp_avg, float* exp_avg_sq, float* wstream_coarse, float* wstream_fine, float* loss_out,
                                          const r2l_occ_grid* grid_coarse, const r2l_occ_grid* grid_fine, int64_t* live_acc, float* work,
                                          void* stream) {
    if (const char* why = step_desc_check(d)) {
        r2l_set_error_msg(why);
        return (int)hipErrorInvalidValue;
    }
    if (const char* why = step_occ_desc_check(d)) {
        r2l_set_error_msg(why);
        return (int)hipErrorInvalidValue;
    }
    if (const char* why = r2l_occ_grid_why(grid_coarse, "r2l_teacher_train_step_occ: grid_coarse is NULL")) {
        r2l_set_error_msg(why);
        return (int)hipErrorInvalidValue;
    }
    if (grid_fine != nullptr) {
        if (const char* why = r2l_occ_grid_why(grid_fine, "r2l_teacher_train_step_occ: grid_fine is NULL")) {
            r2l_set_error_msg(why);
            return (int)hipErrorInvalidValue;
        }
    }
    const StepOcc occ{grid_coarse, grid_fine ? grid_fine : grid_coarse, live_acc};
    return step_body(d, rays_o, rays_d, viewdirs, target, ttab, u_det, params, grads, exp_avg, exp_avg_sq, wstream_coarse, wstream_fine,
                     loss_out, work, stream, &occ);
}

namespace {

int step_body(const r2l_teacher_step_desc* d, const float* rays_o, const float* rays_d, const float* viewdirs, const float* target,
              const float* ttab, const float* u_det, float* params, float* grads, float* exp_avg, float* exp_avg_sq, float* wstream_coarse,
              float* wstream_fine, float* loss_out, float* work, void* stream, const StepOcc* occ) {
    if (const char* why = step_desc_check(d)) {
        r2l_set_error_msg(why);
        return (int)hipErrorInvalidValue;
    }
    const int R = d->N_rand, S = d->N_samples, NI = d->N_importance, T = S + NI;
    R2L_REQUIRE(rays_o != nullptr, "r2l_teacher_train_step: rays_o is NULL");
    R2L_REQUIRE(rays_d != nullptr, "r2l_teacher_train_step: rays_d is NULL");
    R2L_REQUIRE(viewdirs != nullptr, "r2l_teacher_train_step: viewdirs is NULL");
    R2L_REQUIRE(target != nullptr, "r2l_teacher_train_step: target is NULL");
    R2L_REQUIRE(ttab != nullptr, "r2l_teacher_train_step: ttab is NULL");
    R2L_REQUIRE(d->perturb != 0 || NI == 0 || u_det != nullptr,
                "r2l_teacher_train_step: u_det is NULL (needed with perturb == 0 and N_importance > 0)");
    R2L_REQUIRE(params != nullptr, "r2l_teacher_train_step: params is NULL");
    R2L_REQUIRE(grads != nullptr, "r2l_teacher_train_step: grads is NULL");
    R2L_REQUIRE(exp_avg != nullptr, "r2l_teacher_train_step: exp_avg is NULL");
    R2L_REQUIRE(exp_avg_sq != nullptr, "r2l_teacher_train_step: exp_avg_sq is NULL");
    R2L_REQUIRE(wstream_coarse != nullptr, "r2l_teacher_train_step: wstream_coarse is NULL");
    R2L_REQUIRE(NI == 0 || wstream_fine != nullptr, "r2l_teacher_train_step: wstream_fine is NULL with N_importance > 0");
    R2L_REQUIRE(NI > 0 || wstream_fine == nullptr,
                "r2l_teacher_train_step: wstream_fine given with N_importance == 0 (the coarse net trains alone: pass NULL)");
    R2L_REQUIRE(loss_out != nullptr, "r2l_teacher_train_step: loss_out is NULL");
    R2L_REQUIRE(work != nullptr, "r2l_teacher_train_step: work is NULL");
    R2L_REQUIRE(((uintptr_t)work & 15) == 0, "r2l_teacher_train_step: work must be 16-byte aligned");

    const hipStream_t st = (hipStream_t)stream;
    const StepWork w = step_work(d, occ != nullptr);
    int64_t* const idx_c = occ ? (int64_t*)(work + w.idx_c) : nullptr;
    int64_t* const count_c = occ ? (int64_t*)(work + w.count_c) : nullptr;
    int64_t* const idx_f = occ ? (int64_t*)(work + w.idx_f) : nullptr;
    int64_t* const count_f = occ ? (int64_t*)(work + w.count_f) : nullptr;
    void* const iwork = occ ? (void*)(work + w.iwork) : nullptr;
    const int64_t n_net = r2l_teacher_param_count();
    const uint64_t sid = ((uint64_t)1 << 62) + 4 * (uint64_t)d->step;  // streams sid + 0 .. 3 of this step (include/r2l_hip.h)
    const bool noise = d->raw_noise_std > 0.f;
    float* const nf = work + w.nearfar;
    float* const z = work + w.z;
    int rc;

    hipLaunchKernelGGL(r2l_step_nearfar_kernel, dim3(1), dim3(64), 0, st, nf, d->near, d->far);
    R2L_CHECK(hipGetLastError());
    float* t_rand = nullptr;
    if (d->perturb) {
        t_rand = work + w.trand;
        if ((rc = r2l_draw_uniform(t_rand, (int64_t)R * S, d->seed, sid + 0, stream))) return rc;
    }
    if ((rc = r2l_stratified_z(nf, nf + 1, 0, ttab, t_rand, z, R, S, stream))) return rc;
    float* noise_c = nullptr;
    if (noise) {
        noise_c = work + w.noise_c;
        if ((rc = r2l_draw_normal(noise_c, (int64_t)R * S, d->seed, sid + 2, d->raw_noise_std, stream))) return rc;
    }
    if ((rc = step_forward(rays_o, rays_d, viewdirs, z, wstream_coarse, params, work + w.raw_c, work + w.stash_c, R, S, stream,
                           occ ? occ->coarse : nullptr, occ, idx_c, count_c, iwork)))
        return rc;

    const float* mse_last = work + w.mse_c;
    const float* mse_first = nullptr;
    const float inv_denom = (float)(1.0 / (double)(3 * (int64_t)R));  // the staged path's 1 / (3 R): a double, then one rounding
    if (NI > 0) {
        float* const c_s = work + w.s_c;
        if ((rc = r2l_raw2outputs(work + w.raw_c, z, rays_d, noise_c, d->white_bkgd, work + w.rgb_c, c_s, c_s + r4(R), work + w.wts,
                                  c_s + 2 * r4(R), R, S, stream)))
            return rc;
        const float* u = u_det;
        if (d->perturb) {
            if ((rc = r2l_draw_uniform(work + w.u, (int64_t)R * NI, d->seed, sid + 1, stream))) return rc;
            u = work + w.u;
        }
        float* const zall = work + w.zall;
        if ((rc = r2l_sample_pdf_sort(z, work + w.wts, u, d->perturb ? NI : 0, work + w.zs, zall, nullptr, R, S, NI, stream))) return rc;
        float* noise_f = nullptr;
        if (noise) {
            noise_f = work + w.noise_f;
            if ((rc = r2l_draw_normal(noise_f, (int64_t)R * T, d->seed, sid + 3, d->raw_noise_std, stream))) return rc;
        }
        float* const fparams = params + n_net;
        if ((rc = step_forward(rays_o, rays_d, viewdirs, zall, wstream_fine, fparams, work + w.raw_f, work + w.stash_f, R, T, stream,
                               occ ? occ->fine : nullptr, occ, idx_f, count_f, iwork)))
            return rc;
        if ((rc = r2l_raw2outputs_backward(work + w.raw_f, zall, rays_d, noise_f, d->white_bkgd, target, work + w.draw, work + w.sqerr_f,
                                           R, T, stream)))
            return rc;
        if ((rc = step_backward(rays_o, rays_d, viewdirs, zall, fparams, work + w.stash_f, work + w.draw, grads + n_net, work + w.bwd, R,
                                T, stream, occ, idx_f, count_f)))
            return rc;
        if ((rc = r2l_loss_finish(work + w.sqerr_f, R, inv_denom, work + w.mse_f, stream))) return rc;
        mse_last = work + w.mse_f;
        mse_first = work + w.mse_c;
    }
    if ((rc = r2l_raw2outputs_backward(work + w.raw_c, z, rays_d, noise_c, d->white_bkgd, target, work + w.draw, work + w.sqerr_c, R, S,
                                       stream)))
        return rc;
    if ((rc = step_backward(rays_o, rays_d, viewdirs, z, params, work + w.stash_c, work + w.draw, grads, work + w.bwd, R, S, stream, occ,
                            idx_c, count_c)))
        return rc;
    if ((rc = r2l_loss_finish(work + w.sqerr_c, R, inv_denom, work + w.mse_c, stream))) return rc;
    hipLaunchKernelGGL(r2l_step_loss_kernel, dim3(1), dim3(64), 0, st, mse_last, mse_first, loss_out);
    R2L_CHECK(hipGetLastError());

    // Adam's bias corrections are 1 - beta^step: beyond 2^31 steps the power is 0 in double for every beta < 1 a run would use
    const int adam_step = d->step > 0x7fffffff ? 0x7fffffff : (int)d->step;
    if ((rc = r2l_adam_step(params, grads, exp_avg, exp_avg_sq, n_net * (NI > 0 ? 2 : 1), d->lr, d->beta1, d->beta2, d->eps, adam_step,
                            1.0f, stream)))
        return rc;
    if ((rc = r2l_pack_teacher(params, wstream_coarse, stream))) return rc;
    if (NI > 0 && (rc = r2l_pack_teacher(params + n_net, wstream_fine, stream))) return rc;
    return 0;
}

}  // namespace
