// r2l_backward.hip — C ABI of the hand-written backward of the R2L student (replaces the autograd graph the reference's
// training loop builds: loss = mean((rgb-target)^2) * lw_rgb, loss.backward()).  Host only: this file
// contains no kernel.  r2l_backward_part_cfg checks its arguments, resolves the launch plan (r2l_dispatch.h) and runs the four
// stages of a step, each through the launcher of the file that owns its kernels:
//   1. dX chain      : r2l_bwd32.hip (fp32 MFMA), r2l_coop16.hip, r2l_bwd3.hip (bf16x3), r2l_bwd2.hip / r2l_coopf_bwd.hip (fp16x2):
//                      dL/drgb -> sigmoid' -> tail^T -> the 2*n_block transposed layers; writes the per-layer output gradients G
//                      that the weight-gradient GEMMs need.
//   2. body dW       : r2l_dw_body.hip (with r2l_dw16.hip in front in the default trio): dW[l] = G[l]^T A[l] + db.
//   3. head dW       : r2l_dw_head.hip (with r2l_dw_head16.hip in front in the default trio): dW_head = G_head^T PE(rays).
//   4. tail dW       : r2l_dw_tail.hip: tail weight / bias gradients (3x256).
#include "r2l_dispatch.h"
#include "r2l_f2.h"
#include "r2l_dw.h"
#include "r2l_hip.h"

extern "C" int64_t r2l_num_tiles(int64_t N) { return (N + R2L_TILE_RAYS - 1) / R2L_TILE_RAYS; }
extern "C" int64_t r2l_padded_rows(int64_t N) { return R2L_PAD_ROWS(N); }
// (+ 16 floats of status words behind the partials)
extern "C" int64_t r2l_dw_slab_floats(void) { return DW_TAIL_SLAB_BASE + DW_TAIL_SLAB + 16; }  // (r2l_dw.h: body | head | tail regions)
extern "C" int64_t r2l_stash_slot_floats(int64_t N) { return R2L_TRIO_SLOT(R2L_PAD_ROWS(N)); }

// May the dX chain of an N-ray step be cut into block segments (R2L_BWD_CHAIN with a layer range)?  1 when the step takes the
// cooperative fp16 chains (small launches of the default trio), else 0.
extern "C" int r2l_chain_segments_ok_cfg(int64_t N, int n_block, const r2l_config* cfg) {
    R2L_CFG_QUERY(cfg);
    return r2l_plan(cfg, N, n_block, true, false).chain_segments_ok ? 1 : 0;
}
// Device word that the fp16 dX chain raises when a step needs the bf16x3 fallback (range guard, or the forward fell back):
// 0 after a clean step.  A host that runs steps with R2L_BWD_NOFALLBACK hands it to r2l_adam_step_guarded.
extern "C" const unsigned* r2l_backward_status_word(const float* wstream_bwd, int n_block) {
    return r2l_bwd_streams(wstream_bwd, n_block).status;
}

extern "C" const unsigned* r2l_backward_status_words(const float* wstream_bwd, int n_block) {
    if (wstream_bwd == nullptr || n_block < 0 || n_block > R2L_MAX_BLOCKS) return nullptr;
    return r2l_backward_status_word(wstream_bwd, n_block);
}

extern "C" int r2l_backward(const float* rays_o, const float* rays_d, const float* t_rand, const float* ztab,
                            const float* emb, const float* rgb, const float* target, const float* drgb,
                            const float* save_x, const float* save_t,
                            const float* wstream_bwd, const float* params, int n_block, float grad_scale, float* dpre,
                            float* gx, float* gt, float* sqerr_partial, float* grads, float* dw_slab, int64_t N,
                            void* stream_) {
    return r2l_backward_part_cfg(rays_o, rays_d, t_rand, ztab, emb, rgb, target, drgb, save_x, save_t, wstream_bwd, params, n_block,
                                 grad_scale, dpre, gx, gt, sqerr_partial, grads, dw_slab, N, stream_, R2L_BWD_ALL, 0, 2 * n_block,
                                 nullptr);
}

// The same backward cut into stages, so that a data-parallel host can hand finished gradient buckets to the collective
// while the remaining stages still run: parts = OR of R2L_BWD_CHAIN (dX chain; must precede everything else of a step),
// R2L_BWD_BODY (weight / bias gradients of the body layers [layer_lo, layer_hi) of the 2*n_block, complete in `grads`
// when the call's kernels have run), R2L_BWD_HEAD, R2L_BWD_TAIL.  Stages of one step go to ONE stream (they share dw_slab).
extern "C" int r2l_backward_part(const float* rays_o, const float* rays_d, const float* t_rand, const float* ztab,
                                 const float* emb, const float* rgb, const float* target, const float* drgb,
                                 const float* save_x, const float* save_t,
                                 const float* wstream_bwd, const float* params, int n_block, float grad_scale, float* dpre,
                                 float* gx, float* gt, float* sqerr_partial, float* grads, float* dw_slab, int64_t N,
                                 void* stream_, int parts, int layer_lo, int layer_hi) {
    return r2l_backward_part_cfg(rays_o, rays_d, t_rand, ztab, emb, rgb, target, drgb, save_x, save_t, wstream_bwd, params, n_block,
                                 grad_scale, dpre, gx, gt, sqerr_partial, grads, dw_slab, N, stream_, parts, layer_lo, layer_hi,
                                 nullptr);
}

// What the stages of a call share, derived once from the plan and the arguments.
struct R2LBwdStep {
    bool split;        // the one-wave-per-tile trios (their forward wrote the stash): private stash layout, see r2l_dispatch.h R2L_STASH_*
    bool trio16;       // the default trio of those: fp16 chains + fp16 weight-gradient GEMMs on fp16 stage pieces
    bool chain_seg;    // R2L_BWD_CHAIN with a proper sub-range of the layers: ONE SEGMENT of the dX chain (include/r2l_hip.h)
    bool no_fallback;  // R2L_BWD_NOFALLBACK: the bf16x3 kernels behind the fp16 ones are not launched
    // MSE mode of the trio: the dX chain runs on gscale * g, gscale = 2^(8 - e) for grad_scale = m * 2^e (m in [0.5, 1)): the
    // seed gscale * dL/dpre is then <= 64 |rgb - target|, which puts the chain's values into fp16's range for the fp16
    // gradient kernels; powers of two commute with fp32 rounding, so the scaled chain is bit-identical after unscaling
    float gscale;
    unsigned* status;  // raised by r2l_bwd2_kernel when this step has to run on the bf16x3 kernels (range guard / the forward fell back)
    // generic mode (dL/drgb from the caller, no known scale): {gscale, 1 / gscale} are chosen on the device from max |drgb| and
    // live in words 4, 5 of the status area; every kernel of the step reads them there
    // (round 4: MSE mode as well — the step's scale is chosen on the device from the previous step's largest chain value,
    // r2l_bwd_prepare_kernel; the host-side gscale above remains the bf16x3-only trio's)
    const float* scale_dev;
};

// Small steps: the head / tail gradients BESIDE the body's (round 5).  At 4096 rays the body's weight-gradient kernel fills 172
// CUs for ~105 us and its reduce 19 us, then the head's (64 workgroups, VALU-bound: 54 us + 11 us of reduce) and the tail's
// (6 + 11 us) each run alone on a mostly idle chip.  They only share the dX chain's outputs as inputs and write disjoint ranges
// of the flat gradient and (since round 5) disjoint regions of dw_slab, so a call that does all of them puts head + tail on a
// second stream of the library's own between two events: fork behind the chain, join before returning — for the caller's
// stream nothing changes (capturable: the side stream joins the capture and leaves it at the join).  R2L_NO_DW_OVERLAP=1: off.
// The side stream and its fork / join events belong to the calling THREAD (and device): two host threads driving the same
// device never record or wait on each other's events; calls of one thread are issued in order, so a later
// call's re-record cannot be seen by an earlier call's already enqueued wait.
struct R2LSideStream {  // always joins once forked — on the error returns too (an unjoined fork would invalidate a capture
    hipStream_t on = nullptr, back = nullptr;     // in progress and let the caller's later work race with head / tail kernels)
    hipEvent_t ev = nullptr;
    int fork(hipStream_t stream) {  // (no device to ask, or one past the table: the call runs on one stream)
        static thread_local hipStream_t streams[16] = {nullptr};
        static thread_local hipEvent_t ev_fork[16], ev_join[16];
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 0;
        if (streams[dev] == nullptr) {
            hipStream_t st = nullptr;
            R2L_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
            R2L_CHECK(hipEventCreateWithFlags(&ev_fork[dev], hipEventDisableTiming));
            R2L_CHECK(hipEventCreateWithFlags(&ev_join[dev], hipEventDisableTiming));
            streams[dev] = st;  // (last: a failed creation above leaves the slot empty and the next call retries)
        }
        R2L_CHECK(hipEventRecord(ev_fork[dev], stream));
        R2L_CHECK(hipStreamWaitEvent(streams[dev], ev_fork[dev], 0));
        on = streams[dev]; back = stream; ev = ev_join[dev];
        return 0;
    }
    int join() {
        if (on == nullptr) return 0;
        const hipStream_t s = on;
        on = nullptr;
        R2L_CHECK(hipEventRecord(ev, s));
        R2L_CHECK(hipStreamWaitEvent(back, ev, 0));
        return 0;
    }
    ~R2LSideStream() { (void)join(); }
};

// Where the head's per-slice partials go: the head's region of dw_slab, else the (by now dead) gt scratch when it is large
// enough — never beside the body kernels of an overlapped call: they are still reading it on the other stream —, else
// nullptr: fp32 atomics.
static float* r2l_head_partials(float* dw_slab, float* gt, int64_t slices, int n_block, int64_t N, bool overlap) {
    if (slices <= 1) return nullptr;
    const int64_t slab_floats = slices * (int64_t)(R2L_W * 1024);
    const int64_t gt_floats = (int64_t)n_block * R2L_PAD_ROWS(N) * R2L_W;
    if (dw_slab != nullptr && slab_floats <= DW_HEAD_SLAB_MAX) return dw_slab + DW_BODY_SLAB;
    return (slab_floats <= gt_floats && !overlap) ? gt : nullptr;
}

extern "C" int r2l_backward_part_cfg(const float* rays_o, const float* rays_d, const float* t_rand, const float* ztab,
                                     const float* emb, const float* rgb, const float* target, const float* drgb,
                                     const float* save_x, const float* save_t,
                                     const float* wstream_bwd, const float* params, int n_block, float grad_scale, float* dpre,
                                     float* gx, float* gt, float* sqerr_partial, float* grads, float* dw_slab, int64_t N,
                                     void* stream_, int parts, int layer_lo, int layer_hi, const r2l_config* cfg) {
    R2L_CFG_ENTER(cfg);
    R2L_REQUIRE(N >= 0 && n_block >= 0 && n_block <= R2L_MAX_BLOCKS, "r2l_backward_part: N / n_block out of range");
    if (N <= 0) return 0;
    R2L_REQUIRE((parts & ~(R2L_BWD_ALL | R2L_BWD_NOFALLBACK)) == 0 && (parts & R2L_BWD_ALL) != 0,
                "r2l_backward_part: parts is an OR of R2L_BWD_CHAIN / BODY / HEAD / TAIL (+ R2L_BWD_NOFALLBACK)");
    R2L_REQUIRE(rgb && (target || drgb) && save_x && (save_t || n_block == 0) && wstream_bwd && params && dpre && gx &&
                    (gt || n_block == 0) && grads,
                "r2l_backward_part: a required pointer is NULL");
    R2L_REQUIRE(emb != nullptr || (rays_o && rays_d && ztab), "r2l_backward_part: needs emb, or rays_o / rays_d / ztab to recompute it");
    if (layer_lo < 0) layer_lo = 0;
    if (layer_hi > 2 * n_block) layer_hi = 2 * n_block;
    R2LBwdStep s{};
    s.chain_seg = (parts & R2L_BWD_CHAIN) && layer_hi > layer_lo && !(layer_lo == 0 && layer_hi == 2 * n_block);
    s.no_fallback = (parts & R2L_BWD_NOFALLBACK) != 0;
    if (s.chain_seg && ((layer_lo | layer_hi) & 1)) {
        r2l_set_error_msg("r2l_backward_part: a chain segment covers whole blocks (even layer bounds)");
        return (int)hipErrorInvalidValue;
    }
    hipStream_t stream = (hipStream_t)stream_;
    // what runs: the same plan the forward of this step resolved (r2l_dispatch.h)
    const R2LPlan plan = r2l_plan(cfg, N, n_block, true, emb != nullptr);
    const R2LDwGrids grid = r2l_dw_grids(plan, layer_hi - layer_lo);
    const R2LStreams w = r2l_bwd_streams(wstream_bwd, n_block);
    s.split = plan.stash != R2L_STASH_ROWMAJOR;
    s.trio16 = plan.stash == R2L_STASH_FP16;
    s.gscale = 1.0f;
    if (s.split && target != nullptr && grad_scale > 0.f) {
        int e = 0;
        (void)frexpf(grad_scale, &e);
        s.gscale = ldexpf(1.0f, 8 - e);
    }
    s.status = w.status;
    s.scale_dev = s.trio16 ? reinterpret_cast<const float*>(s.status + B2S_GSCALE) : nullptr;

    // 1. dX chain
    const R2LLossIO loss{rgb, target, drgb, grad_scale, dpre, sqerr_partial};
    if (!(parts & R2L_BWD_CHAIN)) {
    } else if (plan.chain == R2L_CHAIN_COOP16) {
        if (const int rc = r2l_coop16_backward(loss, save_x, save_t, w.w16, params, n_block, gx, gt, N, stream)) return rc;
    } else if (s.split) {
        // one-wave-per-tile dX chain.  Default trio (MSE mode: scaled chain, values in fp16's range up to the guard): two-way fp16
        // splits, 3 fp16 products per fp32 product (r2l_bwd2.hip), stashing fp16 stage pieces for r2l_dw16.hip, with the
        // bf16x3 chain behind it as fallback (returns at once unless the status word behind the bwd2 stream was raised: range
        // guard, or the forward already fell back and left an fp32 stash); otherwise the bf16x3 chain (r2l_bwd3.hip)
        if (s.chain_seg && !(plan.chain_segments_ok && s.no_fallback)) {
            r2l_set_error_msg("r2l_backward_part: chain segments need the cooperative fp16 chains (r2l_chain_segments_ok_cfg) and "
                              "R2L_BWD_NOFALLBACK");
            return (int)hipErrorInvalidValue;
        }
        if (s.trio16) {
            if (!s.chain_seg || layer_hi == 2 * n_block) {  // (the first segment opens the step)
                const float* generic = target != nullptr ? nullptr : drgb;
                if (const int rc = r2l_bwd2_open_step(s.status, params, n_block, grad_scale, generic, N, stream)) return rc;
            }
            // small launches: the cooperative chain (r2l_coopf_bwd.hip), same stream / stash / status word; only it is cut into segments
            const int rc2 = plan.tiling == R2L_TILING_COOPF
                                ? r2l_coopf_backward(loss, save_x, save_t, w.w2, params, n_block, gx, gt, N, stream, s.gscale, s.status,
                                                     s.scale_dev, plan, s.chain_seg ? layer_hi / 2 - 1 : -1, s.chain_seg ? layer_lo / 2 : 0)
                                : r2l_bwd2_backward(loss, save_x, save_t, w.w2, params, n_block, gx, gt, N, stream, s.gscale, s.status,
                                                    s.scale_dev, plan.stash_mid);
            if (rc2) return rc2;
            if (!s.no_fallback) {
                // the fallback's stream is packed in front of it, and only when it will run
                // (... and an fp16 forward stash is expanded for the bf16x3 kernels: a chain-only trip, r2l_bwd3.hip)
                if (const int rc = r2l_bwd3_pack(params, n_block, w.w3, stream, s.status, save_x, save_t, N)) return rc;
            }
        }
        if (!(s.trio16 && s.no_fallback)) {
            if (const int rc = r2l_bwd3_backward(loss, save_x, save_t, w.w3, params, n_block, gx, gt, N, stream, s.gscale,
                                                 s.trio16 ? s.status : nullptr, s.scale_dev)) return rc;
        }
    } else {
        if (const int rc = r2l_bwd32_backward(loss, save_x, save_t, w.w32, params, n_block, gx, gt, N, stream)) return rc;
    }

    // a call that does body and head of a small step: head + tail on the side stream (R2LSideStream)
    R2LSideStream side;
    if (plan.dw_overlap && (parts & R2L_BWD_BODY) && (parts & R2L_BWD_HEAD) && layer_hi > layer_lo && dw_slab != nullptr) {
        if (const int rc = side.fork(stream)) return rc;
    }
    const bool overlap = side.on != nullptr;
    const hipStream_t hstream = overlap ? side.on : stream;

    // 2. body weight gradients
    if ((parts & R2L_BWD_BODY) && layer_hi > layer_lo) {
        R2LDwArgs a{};
        a.save_x = save_x; a.save_t = save_t; a.gx = gx; a.gt = gt; a.grads = grads; a.n_block = n_block; a.N = N;
        a.layer0 = layer_lo; a.n_layers = layer_hi - layer_lo;
        a.units_per_layer = (N + DW_CHUNK - 1) / DW_CHUNK;
        const int64_t total = a.units_per_layer * a.n_layers;
        int64_t wgs = grid.body_wgs;
        if (wgs > total) wgs = total;
        a.units_per_wg = (total + wgs - 1) / wgs;
        wgs = (total + a.units_per_wg - 1) / a.units_per_wg;
        // units_per_wg <= units_per_layer whenever wgs >= n_layers (always, for n_block <= 128): a range touches <= 2 layers
        a.slab = (a.units_per_wg <= a.units_per_layer) ? dw_slab : nullptr;
        // chunked stash: the gradient operands carry the chain's power-of-two scale
        if (s.split) a.unscale = 1.0f / s.gscale;
        a.scale_dev = s.scale_dev;
        // (exact mode: the chains of this step stashed the mid halves too — the same config / environment as the forward)
        if (plan.stash_mid) a.mid_off = (unsigned)R2L_H16_MID_BYTES(R2L_PAD_ROWS(N));
        if (const int rc = r2l_dw_body_launch(a, plan.dw_body, wgs, s.status, s.no_fallback, stream)) return rc;
    }
    // 3. head weight gradient
    if (parts & R2L_BWD_HEAD) {
        R2LDwHeadArgs a{};
        a.rays_o = rays_o; a.rays_d = rays_d; a.t_rand = t_rand; a.ztab = ztab; a.emb = emb; a.gh = gx; a.grads = grads; a.N = N;
        a.rays_per_wg = grid.head_rays;
        a.slab = r2l_head_partials(dw_slab, gt, grid.head_slices, n_block, N, overlap);
        if (plan.dw_head16) {
            a.gscale = s.gscale;
            a.unscale = 1.0f / s.gscale;
            a.scale_dev = s.scale_dev;
            a.exact = plan.stash_mid;
        }
        if (const int rc = r2l_dw_head_launch(a, grid.head_slices, plan.dw_head16, s.status, s.no_fallback, hstream)) return rc;
    }
    // 4. tail gradients
    if (parts & R2L_BWD_TAIL) {
        const int64_t wgs = grid.tail_wgs;
        // partials in the tail's region of dw_slab; summed in workgroup order
        float* part = (dw_slab != nullptr && wgs * (4 * R2L_W) <= DW_TAIL_SLAB) ? dw_slab + DW_TAIL_SLAB_BASE : nullptr;
        // (chunked stash: slot n of save_x holds y = x_n + x_0)
        const float* xn = save_x + (int64_t)n_block * (s.split ? R2L_TRIO_SLOT(R2L_PAD_ROWS(N)) : R2L_PAD_ROWS(N) * (int64_t)R2L_W);
        if (const int rc = r2l_dw_tail_launch(dpre, s.split ? nullptr : save_x, xn, grads, part, n_block, N, wgs, grid.tail_rays, hstream))
            return rc;
    }
    return side.join();  // the caller's stream continues when head + tail are done as well
}
