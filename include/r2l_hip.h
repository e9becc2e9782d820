/* r2l_hip.h — C ABI of libr2l_hip.so, the MI355X (gfx950) implementation of the R2L hot path.
 *
 * The reference (snap-research/R2L) has no FFI layer: its hot path is a chain of PyTorch ops.  Each entry point
 * below replaces the reference op sequence cited beside it (paths are into /root/reference).  All pointers are
 * DEVICE pointers to contiguous row-major fp32 unless marked "host".  The library never allocates, frees or
 * retains caller memory; kernels are enqueued on the caller's HIP stream (`stream` = hipStream_t, 0 = default) with
 * no implicit synchronisation.  Every function returns 0 on success or a hipError_t code; r2l_last_error() gives
 * the text.  Nothing throws across this boundary.  INTEGRATION.md shows the ctypes stub a maintainer binds.
 */
#ifndef R2L_HIP_H
#define R2L_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

const char* r2l_last_error(void);

/* ---- explicit dispatch ------------------------------------------------------------------------------------------
 * Which kernel family serves a call is the library's choice (by ray count) unless the host says otherwise.  Hosts say so
 * with an r2l_config passed to the *_cfg form of an entry point (cfg == NULL and all-zero fields = AUTO = the plain entry
 * point).  AUTO fields still honour the R2L_* environment switches of README.md (test / A-B overrides); a non-zero field
 * wins over the environment.  A forward with a stash and the backward that consumes it must be given the same config, and
 * so must the r2l_*_layout_for_cfg queries that decide which weight-stream layout to pack for them.
 * A field outside its enum / range (or a non-zero reserved word) is an error: launch entry points return
 * hipErrorInvalidValue (r2l_last_error says which field), the host-side *_for_cfg / *_ok_cfg queries return -1.
 * (The reference has no counterpart: its dtype / device choices are torch globals; this replaces `setenv` for hosts that
 * are not this repo's Python.) */
enum { R2L_PRECISION_AUTO = 0,
       R2L_PRECISION_FP16X2 = 1,     /* 3 fp16 MFMA products per fp32 product (~2^-21), range-guarded; dW per dw_mode     */
       R2L_PRECISION_BF16X3 = 2,     /* 6 bf16 products per fp32 product (fp32-exact products) everywhere                  */
       R2L_PRECISION_FP32_MFMA = 3   /* v_mfma_f32_32x32x2_f32 everywhere                                                  */ };
enum { R2L_TILING_AUTO = 0,
       R2L_TILING_WAVE_PER_TILE = 1, /* one wavefront owns a 32-ray tile ("main")                                          */
       R2L_TILING_COOP_RETIRED = 2,  /* (rounds 1 - 4: fp32-MFMA cooperative kernels, 32-ray tiles; retired: hipErrorInvalidValue) */
       R2L_TILING_COOP16 = 3,        /* fp32-MFMA cooperative kernels, 16-ray tile per workgroup                           */
       R2L_TILING_COOPF = 4          /* fp16x2 cooperative kernels (r2l_coopf_*), coop_tiles ray tiles per workgroup       */ };
enum { R2L_DW_AUTO = 0,
       R2L_DW_FP16 = 1,              /* fp16 trio: weight-gradient GEMMs on the operands' fp16 hi halves, 1 product        */
       R2L_DW_EXACT = 2              /* fp16 trio: both operands as hi + mid (22 bits), 3 products: fp32-grade dW          */ };
typedef struct r2l_config {
    int precision;    /* R2L_PRECISION_*                                                                                  */
    int tiling;       /* R2L_TILING_*                                                                                     */
    int coop_tiles;   /* 0 auto, 1 or 2: 32-ray tiles per workgroup of the fp16x2 cooperative kernels; 3 (opt-in, never auto):
                         mixed grid (two-tile and one-tile workgroups, one per CU) for tile counts between one and two per CU */
    int reserve_cus;  /* 0 auto (R2L_RESERVE_CUS or none), n > 0: CUs the persistent weight-gradient kernels leave free
                         for collectives running beside them, -1: none                                                    */
    int dw_mode;      /* R2L_DW_*                                                                                         */
    int reserved[3];  /* must be 0                                                                                        */
} r2l_config;

/* Errors: every entry point returning int gives 0 on success, else a hipError_t value (hipErrorInvalidValue = 1 for a NULL
 * required pointer, a size / n_block (0 .. 1024) / layout / parts argument out of range, or a bad r2l_config — checked before
 * anything is launched) or R2L_ERR_RCCL_BASE + ncclResult_t; r2l_last_error() holds the text for the calling thread.  N == 0
 * (R == 0, K == 0) is a successful no-op. */

/* ---- parameter layout ------------------------------------------------------------------------------------------
 * `params` is ONE flat fp32 buffer holding NeRF_v3_2's tensors in state_dict order (model/nerf_raybased.py:500-537):
 *   head.0.weight[256,1008] head.0.bias[256] { body.b.body.0.weight[256,256] .bias[256] body.b.body.2.weight .bias }
 *   x n_block, tail.0.weight[3,256] tail.0.bias[3].          W = 256, 16 samples/ray, L = 10 are compiled in.   */
int64_t r2l_param_count(int n_block);        /* 5 917 187 for n_block = 43 (D = 88) */
int64_t r2l_fwd_stream_floats(int n_block);  /* size of the packed forward weight stream, incl. prefetch padding */
int64_t r2l_bwd_stream_floats(int n_block);  /* size of the packed transposed (dX) weight stream                */

/* Re-pack params into the MFMA A-operand weight streams the chain kernels read (call after every weight update). */
int r2l_pack_forward(const float* params, int n_block, float* wstream, void* stream);
int r2l_pack_backward(const float* params, int n_block, float* wstream_bwd, void* stream);
/* Per-layout form: layout = 32 (fp32-MFMA one-wave-per-tile kernels), 16 (16-ray cooperative
 * kernels), 3 (bf16 (hi, mid, lo) stages: r2l_fwd3.hip / r2l_bwd3.hip), 2 (fp16 (hi, mid) stages: r2l_fwd2.hip /
 * r2l_bwd2.hip and their cooperative forms r2l_coopf_*.hip; the bf16 stream behind them is their range-guard fallback and
 * is packed by the fallback launch itself when — and only when — it runs) or 0 (all parts, = r2l_pack_forward/backward).
 * r2l_variant_for(N) tells which chain variant a call with N rays will take (0 main — incl. the cooperative fp16x2 kernels
 * of small launches —, 2 coop16: layout 16; 1 named the retired 32-ray cooperative family), honouring R2L_FORCE_VARIANT
 * (main | coopf | coop16). */
int r2l_variant_for(int64_t N);
/* Within the fp16 trio (layout 2): 0 = the one-wave-per-tile chains serve a launch of N rays, 1 / 2 = the cooperative chains
 * with that many 32-ray tiles per workgroup, 3 = their MIXED grid (only when pinned; tile counts between one and two per CU:
 * tiles - n_cu two-tile workgroups + 2 n_cu - tiles one-tile ones, one workgroup on every CU) (<= 16 384 rays, and 32 769 .. 49 152 rays:
 * csrc/r2l_common.h r2l_use_coopf; R2L_FORCE_VARIANT=main|coopf and R2L_COOPF_TILES=1|2|3 pin it).  1 / 2 / 3 give
 * bit-identical results (every tile takes the same path); 0 agrees with them within rounding. */
int r2l_coop_tiles_for(int64_t N, int n_block);
int r2l_forward_layout_for(int64_t N, int with_stash); /* 16, 32, 3 = bf16x3 stage stream, 2 = fp16x2 stage stream (+ the
                                                         * bf16x3 one behind it as range-guard fallback) */
/* Same for the transposed stream r2l_backward reads for N rays (r2l_pack_backward_layout takes the value). */
int r2l_backward_layout_for(int64_t N);
/* The same four queries for calls that will be made with an r2l_config; cfg == NULL: the plain forms. */
int r2l_variant_for_cfg(int64_t N, const r2l_config* cfg);
int r2l_coop_tiles_for_cfg(int64_t N, int n_block, const r2l_config* cfg);
int r2l_forward_layout_for_cfg(int64_t N, int with_stash, const r2l_config* cfg);
int r2l_backward_layout_for_cfg(int64_t N, const r2l_config* cfg);
int r2l_pack_forward_layout(const float* params, int n_block, float* wstream, int layout, void* stream);
int r2l_pack_backward_layout(const float* params, int n_block, float* wstream, int layout, void* stream);

/* ---- student forward -------------------------------------------------------------------------------------------
 * rgb[N,3] = NeRF_v3_2.forward(PositionalEmbedder(10)(PointSampler.sample_train(rays_o, rays_d, perturb)))
 *   replaces model/nerf_raybased.py:114-126 (sample_train), :198-208 (PositionalEmbedder.__call__),
 *   :461-465 (ResMLP.forward), :539-544 (NeRF_v3_2.forward); call site main.py:1371-1374 / 220-230.
 * ztab[32] = z_lower[16] ++ z_span[16]; depth of sample s = z_lower[s] + z_span[s]*t_rand[ray,s], or z_lower[s]
 * when t_rand == NULL (perturb == 0; then z_lower = PointSampler.z_vals).
 * save_x [(n_block+1) slots] / save_t [n_block slots] of r2l_stash_slot_floats(N) floats each: optional activation stash
 * for r2l_backward (both or none); opaque to the caller (row-major fp32 [Np,256], chunked fp32 or fp16 stage pieces per slot,
 * depending on the kernel family the library picks for N and the R2L_* environment — which must be the same for this call
 * and the r2l_backward that consumes the stash; Np = r2l_padded_rows(N) = N rounded up to 32). */
int r2l_forward_rays(const float* rays_o, const float* rays_d, const float* t_rand, const float* ztab,
                     const float* wstream, const float* params, int n_block, float* rgb, float* save_x,
                     float* save_t, int64_t N, void* stream);

/* rgb[H*W,3] for a whole frame from a camera pose: PointSampler.sample_test (model/nerf_raybased.py:80-102) fused in
 * front of the same chain; call sites main.py:300-309 (render_path) and main.py:401-404 (render_func, --benchmark).
 * c2w_host12: HOST pointer to the row-major [3,4] camera-to-world matrix. */
int r2l_forward_pose(const float* c2w_host12, int H, int W, float focal, const float* ztab, const float* wstream,
                     const float* params, int n_block, float* rgb, void* stream);
/* r2l_forward_rays / r2l_forward_pose with explicit dispatch (r2l_config above; cfg == NULL: as the plain forms). */
int r2l_forward_rays_cfg(const float* rays_o, const float* rays_d, const float* t_rand, const float* ztab,
                         const float* wstream, const float* params, int n_block, float* rgb, float* save_x,
                         float* save_t, int64_t N, void* stream, const r2l_config* cfg);
int r2l_forward_pose_cfg(const float* c2w_host12, int H, int W, float focal, const float* ztab, const float* wstream,
                         const float* params, int n_block, float* rgb, void* stream, const r2l_config* cfg);
/* K frames in ONE launch — the test-set loop of main.py:300-309 (render_path renders every test pose: 200 at testskip=1)
 * without a launch and a partly filled last round of workgroups per frame: rgb[K*H*W,3], frame k from the DEVICE table
 * c2w_dev[K][3][4].  Same values as K calls of r2l_forward_pose.  One-wave-per-tile tilings only (an error otherwise). */
int r2l_forward_poses_cfg(const float* c2w_dev, int K, int H, int W, float focal, const float* ztab, const float* wstream,
                          const float* params, int n_block, float* rgb, void* stream, const r2l_config* cfg);

/* ---- range control of the fp16 kernels (precision FP16X2, the default) -----------------------------------------------------
 * fp16 ends at 65504; the reference's fp32 activations (model/nerf_raybased.py:461-465: an un-normalised 88-layer residual
 * stream) are not bounded a priori.  The library keeps them in range by itself, on the device: the forward weight stream is
 * packed for a power-of-two activation scale s (head weights and all biases divided by s — a ReLU net is positively
 * homogeneous, so every activation is divided by s and nothing else changes; the kernels multiply by s where values leave
 * the chain: exact), every launch records its largest |activation|, and r2l_pack_forward* picks s for the next launches from
 * it (s = 1 while activations stay below 8192: bit-identical to an unscaled stream).  A launch that nevertheless meets a
 * value >= 32768 is redone by the bf16x3 kernel launched behind it (no host involvement, results still exact products), the
 * stream is re-packed for a larger s by that fallback, and the NEXT launch is back on the fp16 kernels.  The training
 * backward does the same with the power-of-two scale of its gradient chain, step to step (r2l_backward_status_words).
 * Hosts only need to (a) zero-fill `wstream` / `wstream_bwd` once after allocating them (stale contents of a previous
 * instance would be taken for history: harmless, but runs are then not reproducible bit for bit) and (b) may read the
 * telemetry below, e.g. to log head-room.  Words (uint32 / float bit patterns) of the forward area:
 *   [0] guard flag of the launch in flight   [1] largest |activation| / s since the scale was last chosen (float)
 *   [2] s (float)   [3] 1 / s   [5] launches that fell back to the bf16x3 kernel   [6] largest |activation| (unscaled) of the
 *   previous epoch (float)   [7] times s changed;   others: private.
 * of the backward area: [0] flag: this step ran on the bf16x3 kernels   [4] gradient scale (float)   [8] largest |chain value|
 *   x scale of this step (float)   [10] steps that fell back   [11] largest unscaled |chain value| of the last clean step. */
const unsigned* r2l_forward_status_words(const float* wstream, int n_block);
const unsigned* r2l_backward_status_words(const float* wstream_bwd, int n_block);

/* rgb[N,3] = NeRF_v3_2.forward(emb[N,1008])  — the module-boundary form (model/nerf_raybased.py:539-544) for callers
 * that still run their own sampler/embedder. */
int r2l_forward_emb(const float* emb, const float* wstream, const float* params, int n_block, float* rgb,
                    float* save_x, float* save_t, int64_t N, void* stream);
/* ... with a config: precision = bf16x3 (fp16x2 is served by the same kernels: this path has no range-guard fallback) runs a
 * forward-only launch (save_x == save_t == NULL) as head on the fp32 MFMA -> X_0 in x0_scratch (r2l_padded_rows(N) * 256 floats,
 * caller-owned) -> body + tail on the bf16x3 chain; every other case is r2l_forward_emb (x0_scratch may then be NULL). */
int r2l_forward_emb_cfg(const float* emb, const float* wstream, const float* params, int n_block, float* rgb, float* save_x,
                        float* save_t, int64_t N, float* x0_scratch, void* stream, const r2l_config* cfg);

/* ---- student backward + optimizer ------------------------------------------------------------------------------
 * Replaces loss.backward() of main.py:1377-1404 for the R2L branch (autograd over the ops above, anomaly mode on in the
 * reference: model/nerf_raybased.py:4) by three hand-written stages: the dX chain through the transposed layers, the
 * per-layer weight-gradient GEMMs (reduction over rays) and the head gradient with the encoding recomputed.
 *   MSE mode  (target != NULL): dL/drgb = grad_scale * (rgb - target)   [grad_scale = 2*lw_rgb / (3*N_global)];
 *                               sqerr_partial[r2l_num_tiles(N)] receives per-32-ray sums of (rgb-target)^2.
 *   generic   (target == NULL): dL/drgb = drgb[N,3] supplied by the caller (autograd bridge); grad_scale is ignored (the
 *                               power-of-two scale the fp16 kernels run the chain on is derived from max |drgb| on the device).
 * Head input: emb[N,1008] if given, else recomputed from (rays_o, rays_d, t_rand, ztab) exactly as the forward did.
 * save_x/save_t: the stash written by the forward of the same N (r2l_forward_rays, or r2l_forward_emb when emb is given).
 * Scratch owned by the caller: dpre[N,3], gx[(n_block+1) slots], gt[n_block slots] (slots of r2l_stash_slot_floats(N)
 * floats, like the stash), dw_slab[r2l_dw_slab_floats()] (204 MB: per-workgroup partial body-layer gradients, per-slice head
 * partials and tail partials in disjoint regions, each summed in a fixed order: bit-reproducible; NULL selects fp32 atomics
 * instead, no scratch but run-to-run rounding differences).  A call that computes body AND head gradients of a small launch
 * (<= 16 384 rays) runs head + tail on a second stream of the library's own beside the body's, forked behind the dX chain and
 * joined before the call returns: for the caller's stream nothing changes (R2L_NO_DW_OVERLAP=1 turns it off).  Gradients are ACCUMULATED into `grads` (flat, same layout as params): zero it first unless
 * accumulation is wanted. */
int64_t r2l_num_tiles(int64_t N);
int64_t r2l_padded_rows(int64_t N);
/* Floats per stash slot: size save_x / gx as (n_block+1) * r2l_stash_slot_floats(N) floats and save_t / gt as
 * n_block * r2l_stash_slot_floats(N) (Np*264: 1 KiB per ray of data + the forward's ReLU mask words; the layout inside the
 * buffers is private to the library). */
int64_t r2l_stash_slot_floats(int64_t N);
int64_t r2l_dw_slab_floats(void);
int r2l_backward(const float* rays_o, const float* rays_d, const float* t_rand, const float* ztab, const float* emb,
                 const float* rgb, const float* target, const float* drgb, const float* save_x, const float* save_t,
                 const float* wstream_bwd, const float* params, int n_block, float grad_scale, float* dpre, float* gx,
                 float* gt, float* sqerr_partial, float* grads, float* dw_slab, int64_t N, void* stream);

/* The same backward cut into stages for data-parallel hosts (replaces nn.DataParallel's ReduceAddCoalesced after
 * loss.backward(), main.py:37-42,472-479,1404): `parts` = OR of the R2L_BWD_* bits; R2L_BWD_BODY computes the weight and
 * bias gradients of the body layers [layer_lo, layer_hi) of the 2*n_block (layer 2b = body.b.body.0, 2b+1 = body.b.body.2),
 * which are complete in `grads` once the call's kernels have run — the host can all-reduce that contiguous range of the
 * flat buffer while later stages still execute.  R2L_BWD_CHAIN must come first in a step; all stages of a step go to
 * one stream (they share dw_slab).  r2l_backward(...) == r2l_backward_part(..., R2L_BWD_ALL, 0, 2*n_block). */
#define R2L_BWD_CHAIN 1
#define R2L_BWD_BODY 2
#define R2L_BWD_HEAD 4
#define R2L_BWD_TAIL 8
#define R2L_BWD_ALL 15
int r2l_backward_part(const float* rays_o, const float* rays_d, const float* t_rand, const float* ztab, const float* emb,
                      const float* rgb, const float* target, const float* drgb, const float* save_x, const float* save_t,
                      const float* wstream_bwd, const float* params, int n_block, float grad_scale, float* dpre, float* gx,
                      float* gt, float* sqerr_partial, float* grads, float* dw_slab, int64_t N, void* stream, int parts,
                      int layer_lo, int layer_hi);
/* r2l_backward_part with explicit dispatch: the config the forward of this step was given (cfg == NULL: the plain form;
 * parts = R2L_BWD_ALL, layers [0, 2 n_block) = r2l_backward). */
int r2l_backward_part_cfg(const float* rays_o, const float* rays_d, const float* t_rand, const float* ztab, const float* emb,
                          const float* rgb, const float* target, const float* drgb, const float* save_x,
                          const float* save_t, const float* wstream_bwd, const float* params, int n_block,
                          float grad_scale, float* dpre, float* gx, float* gt, float* sqerr_partial, float* grads,
                          float* dw_slab, int64_t N, void* stream, int parts, int layer_lo, int layer_hi,
                          const r2l_config* cfg);
/* A data-parallel host with idle CUs (small per-GPU batches: the cooperative chains occupy one CU per 32 or 64 rays) can cut the
 * dX chain itself: R2L_BWD_CHAIN with a layer range [layer_lo, layer_hi) that is a proper sub-range of [0, 2 n_block) runs ONE
 * SEGMENT of the chain — whole blocks, issued from the top (layer_hi = 2 n_block first) down to layer_lo = 0, each on the same
 * stream — and the weight gradients of a finished segment (R2L_BWD_BODY over the same range, on ANOTHER stream, behind an
 * event) and their all-reduce run beside the next segment.  Results are bit-identical to the uncut chain.  Only where
 * r2l_chain_segments_ok_cfg(N, n_block, cfg) says 1, and only together with R2L_BWD_NOFALLBACK on every stage of the step:
 * the bf16x3 fallback kernels are not launched, so a step whose chain raised the status word (*r2l_backward_status_word != 0
 * afterwards: range guard, or the forward had fallen back) has NO valid gradient — r2l_adam_step_guarded skips its update on
 * the device, the host notices later (no sync) and goes back to the uncut form.  r2l_amd/train_step.py is the worked example. */
#define R2L_BWD_NOFALLBACK 16
int r2l_chain_segments_ok_cfg(int64_t N, int n_block, const r2l_config* cfg);
const unsigned* r2l_backward_status_word(const float* wstream_bwd, int n_block);

/* The gradient with respect to the student's INPUT (what autograd gives the reference's plain module for free: pose
 * refinement, localisation against a trained light field).  Call order of a step:
 *     r2l_forward_rays* / r2l_forward_emb* with the stash  ->  r2l_backward* whose parts include R2L_BWD_CHAIN  ->  this call,
 * on the same stream.  gx is that backward's gx: its slot 0 holds dL/d(head pre-activation) [N,256] once the chain has run (in
 * every kernel family: fp32, unscaled, row-major; rows >= N are padding and are not read).  params as given to that backward;
 * gx and params 16-byte aligned.
 *   d_emb    [N,1008] or NULL:  d_emb[r][k] = sum_o gh[r][o] * head.0.weight[o][k]   (exact fp32 products on the matrix pipe)
 *   d_rays_o, d_rays_d  [N,3] each, both or neither; they need the ray form (rays_o, rays_d, ztab as given to the forward;
 *            t_rand NULL when the forward had none):  with z = z_lower[s] + z_span[s] * t_rand[r,s], x = o + d z,
 *            d_pts[r][s][a] = sum_f d_emb[r][(3 s + a) 21 + f] * phi'_f(x)  (2^f cos(2^f x) for the sin columns, -2^f sin(2^f x)
 *            for the cos columns, 1 for x itself),  d_rays_o[a] = sum_s d_pts[s][a],  d_rays_d[a] = sum_s z_s d_pts[s][a].
 *            The jitter t_rand and the table ztab get no gradient.  Without d_emb the [N,1008] product never reaches memory.
 * Outputs are OVERWRITTEN (unlike `grads`), no row >= N is written, no atomics: two calls give the same bits.
 * After a step whose range guard fell back, gx is valid once the fallback kernels have run: they are stream-ordered in front of
 * this launch, nothing to do.  A R2L_BWD_NOFALLBACK step whose status word was raised has no valid gradient here either.
 * Errors (non-zero, r2l_last_error names them): no output requested; d_rays_* without rays_o / rays_d / ztab; one of the two
 * d_rays_* alone; N < 1; n_block out of range; gx / params NULL or misaligned. */
int r2l_backward_input(const float* gx, const float* params, int n_block, const float* rays_o, const float* rays_d,
                       const float* t_rand, const float* ztab, float* d_emb, float* d_rays_o, float* d_rays_d, int64_t N,
                       void* stream);

/* ---- gradient all-reduce for hosts without torch.distributed ----------------------------------------------------------
 * The one exchange of data-parallel training (replaces nn.DataParallel's ReduceAddCoalesced + parameter broadcast,
 * main.py:37-42,472-479): in-place SUM of grads[n] over the ranks, RCCL over xGMI, enqueued on the caller's stream.  RCCL
 * is dlopen'ed on first use (librccl.so.1; override with R2L_RCCL_PATH).  One communicator per process = per GPU (the
 * device current at r2l_allreduce_init).  Rank 0 makes the 128-byte id, the host hands it to the other ranks.  Ranges of
 * the flat buffer finished by r2l_backward_part can be reduced one by one (the call is asynchronous on `stream`).
 * Errors: R2L_ERR_RCCL_BASE + ncclResult_t (R2L_ERR_RCCL_BASE alone: library missing / bad arguments). */
#define R2L_ERR_RCCL_BASE 10000
typedef struct r2l_comm r2l_comm;
int r2l_allreduce_unique_id(void* id_out128);
int r2l_allreduce_init(const void* id128, int world, int rank, r2l_comm** out);
int r2l_grad_allreduce(r2l_comm* comm, float* grads, int64_t n, void* stream);
int r2l_allreduce_destroy(r2l_comm* comm);

/* torch.optim.Adam(lr, betas, eps, weight_decay 0) on flat buffers (main.py:465-467, 1406); `step` counts from 1;
 * grads are multiplied by grad_scale first (1/world_size after a sum all-reduce), before the square.
 * Contract, per entry and with u = 2^-24 (g' = g * grad_scale; every scalar the fp32 value passed here, promoted exactly):
 *   m' = m + (g' - m)(1 - beta1)   v' = v beta2 + g'^2 (1 - beta2)   p' = p - lr / (1 - beta1^step) * m' / (sqrt(v') / sqrt(1 - beta2^step) + eps)
 * evaluated in fp32, within 4 u (|m| + |g'|), 6 u v' and 8 (u (|p| + |p'|) + S u (|m| + |g'|) / D + u |p' - p|) of the fp64 value
 * (S, D: step size and denominator; tests/optim_util.py, tests/test_optimizer_gpu.py).  The weights 1 - beta are formed from the
 * fp32 beta (1.0f - 0.999f = 0.00099998713: beta + (1 - beta) = 1 exactly) and the bias corrections from the same value, where
 * torch.optim.Adam rounds the doubles beta and 1 - beta separately (0.999f beside 0.001f): against torch's fp32 Adam a step from the
 * same state differs by up to 1.29e-5 relative in v's increment, 2.2e-7 in m's, ~8e-6 in the update at small steps (measured: 1.30e-5,
 * 7e-8 of |m| + |g|, 7.8e-6) — far below what two fp32 evaluations of a gradient differ by, and not bit-equality. */
int r2l_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                  float beta1, float beta2, float eps, int step, float grad_scale, void* stream);
/* ... the same update unless *skip_if != 0 (a device word, e.g. r2l_backward_status_word of a R2L_BWD_NOFALLBACK step, or its
 * MAX over the ranks): then parameters and moments are left untouched; skip_if == NULL: r2l_adam_step. */
int r2l_adam_step_guarded(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                          float beta1, float beta2, float eps, int step, float grad_scale, const unsigned* skip_if,
                          void* stream);
/* The same update (bit for bit) with the re-pack of the fp16x2 weight streams folded in: what r2l_adam_step_guarded followed by
 * r2l_pack_forward_layout(.., 2, ..) and r2l_pack_backward_layout(.., 2, ..) leave behind — the optimizer kernel writes the body
 * weights' (hi, mid) stage pieces of both streams itself and commits the activation scale (range control), a second small kernel
 * packs the head / bias stages for it — two launches instead of four, 42 us of kernel time instead of 65.  (The trainer of this repo
 * keeps the separate packs by default: packed a step early, the backward stream is cold when the dX chain reads it, which costs
 * what the fusion saves; profiles/r05_small_step_ab.txt.)  wstream_fwd / wstream_bwd: the buffers of
 * r2l_fwd_stream_floats / r2l_bwd_stream_floats; only their fp16x2 parts are written (the other layouts stay stale until packed).
 * *skip_if != 0: nothing is touched.  The default trio's step (r2l_forward_layout_for_cfg == r2l_backward_layout_for_cfg == 2). */
int r2l_adam_step_packed(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int n_block, float lr,
                         float beta1, float beta2, float eps, int step, float grad_scale, const unsigned* skip_if,
                         float* wstream_fwd, float* wstream_bwd, void* stream);

/* out2[0] = inv_denom * sum(sqerr_partial) (= img2mse * lw_rgb, helpers:19), out2[1] = psnr (helpers:20). */
int r2l_loss_finish(const float* sqerr_partial, int64_t n_partial, float inv_denom, float* out2, void* stream);

/* ---- NeRF teacher (pseudo-data generation) --------------------------------------------------------------------------
 * tparams: flat fp32 state_dict-order buffer of NeRF(D=8, W=256, input_ch=63, input_ch_views=27, use_viewdirs=True)
 * (model/nerf_raybased.py:357-375, built at utils/create_data.py:251-265): pts_linears.{0..7}, views_linears.0,
 * feature_linear, alpha_linear, rgb_linear. */
int64_t r2l_teacher_param_count(void);     /* 595 844 */
int64_t r2l_teacher_stream_floats(void);
int r2l_pack_teacher(const float* tparams, float* wstream, void* stream);
/* Range control of the fp16 teacher kernel: same scheme and word layout as r2l_forward_status_words (zero-fill `wstream`
 * once after allocating it). */
const unsigned* r2l_teacher_status_words(const float* wstream);

/* raw[R,S,4] = network_query_fn(pts = o + d*z, viewdirs, NeRF): run_network (create_data.py:55-77: embed xyz L=10 and
 * dirs L=4, helpers:24-74; the netchunk loop disappears) + NeRF.forward (model/nerf_raybased.py:377-401), fused. */
int r2l_teacher_mlp(const float* rays_o, const float* rays_d, const float* viewdirs, const float* z,
                    const float* wstream, const float* tparams, float* raw, int64_t R, int S, void* stream);
/* ... with explicit dispatch: only cfg->precision matters (cfg == NULL: the plain form). */
int r2l_teacher_mlp_cfg(const float* rays_o, const float* rays_d, const float* viewdirs, const float* z,
                        const float* wstream, const float* tparams, float* raw, int64_t R, int S, void* stream,
                        const r2l_config* cfg);

/* ---- NeRF teacher training (exact fp32; utils/train_nerf.py) ---------------------------------------------------------
 * One step of main.py:1319-1406 for the teacher: loss = img2mse(rgb) + img2mse(rgb0) (helpers:19), gradients by hand.
 * Stash: floats of the layer outputs kept for the backward pass of P = R*S points (relu(h0..h7), the feature, relu(views)). */
int64_t r2l_teacher_stash_floats(int64_t P);
/* The fp32-MFMA chain of r2l_teacher_mlp_cfg(precision = fp32_mfma) (raw bit-identical), also writing the stash. */
int r2l_teacher_mlp_train(const float* rays_o, const float* rays_d, const float* viewdirs, const float* z,
                          const float* wstream, const float* tparams, float* raw, float* stash, int64_t R, int S, void* stream);
/* draw[R,S,4] = d loss / d raw for loss = img2mse(rgb_map, target) (helpers:19; main.py:1353-1363), through raw2outputs
 * (main.py:556-621: relu(sigma + noise), the 1e10 last dists times |d|, cumprod(1 - alpha + 1e-10), white_bkgd rgb + 1 - acc);
 * alpha = 1 is handled by suffix sums, no division by 1 - alpha.  sqerr[R] = sum_c (rgb_map - target)^2 for r2l_loss_finish
 * with inv_denom = 1/(3R).  noise[R,S] optional (already scaled by raw_noise_std).  1 <= S <= 256. */
int r2l_raw2outputs_backward(const float* raw, const float* z, const float* rays_d, const float* noise, int white_bkgd,
                             const float* target, float* draw, float* sqerr, int64_t R, int S, void* stream);
/* Scratch floats of r2l_teacher_backward for P points. */
int64_t r2l_teacher_train_work_floats(int64_t P);
/* grads[595 844] (tparams order) = d loss / d tparams from draw and the stash of r2l_teacher_mlp_train on the same points
 * (NeRF.forward, model/nerf_raybased.py:377-401, backwards; embedder helpers:24-74 recomputed).  Overwrites grads; fixed
 * reduction order, no atomics: bit-reproducible. */
int r2l_teacher_backward(const float* rays_o, const float* rays_d, const float* viewdirs, const float* z,
                         const float* tparams, const float* stash, const float* draw, float* grads, float* work, int64_t R,
                         int S, void* stream);
/* r2l_raw2outputs_backward with the seed exposed (r2l_raw2outputs_backward IS this call with g = NULL, d_len = NULL and
 * grad_scale = (float)(2.0 / (3.0 * R)), bit for bit):
 *   g == NULL: dL/drgb_map = grad_scale * (rgb_map - target), sqerr[R] written as above;
 *   g[R,3] given: it IS dL/drgb_map; target, grad_scale and sqerr play no part (may be NULL / anything).
 * d_len[R], optional: dL/d|rays_d| (raw2outputs multiplies the intervals by |rays_d|), formed from a dL/dalpha of the kernel's
 * own as sum_s dL/dalpha_s * relu(sigma_s + noise_s) * (z_{s+1} - z_s) * exp(..), summed from the last sample to the first.
 * That dL/dalpha runs the same suffix recurrence on alpha = -expm1(-x) and t = exp(-x) + 1e-10 (x = relu(sigma) dist): the
 * reference's fp32 1 - alpha, which draw keeps bit for bit, leaves three digits of the transmittance behind a nearly opaque
 * sample, and d_len of such a ray consists of those terms.  Asking for d_len changes no bit of draw or sqerr. */
int r2l_raw2outputs_backward_scaled(const float* raw, const float* z, const float* rays_d, const float* noise, int white_bkgd,
                                    const float* target, const float* g, float grad_scale, float* draw, float* sqerr,
                                    float* d_len, int64_t R, int S, void* stream);
/* Scratch floats of r2l_teacher_backward_input for P points (-1 for P < 0). */
int64_t r2l_teacher_input_grad_work_floats(int64_t P);
/* The teacher's backward to its RAYS (frozen weights): the dX chain of r2l_teacher_backward with no weight-gradient product,
 * then d_pe_xyz = G_0 W_0 + G_5 W_5[:, 0:63] and d_pe_dir = G_views W_views[:, 256:283], the derivative of the encoder
 * (helpers:24-74; L = 10 at the fp32 points o + d*z, L = 4 at viewdirs; sin / cos by the forward's own function) and the sums
 * over each ray's samples:
 *   d_pts[R,S,3]      = dL/d(o + d z)              d_rays_o[R,3] = sum_s d_pts        d_viewdirs[R,3] = sum_s d_dir
 *   d_rays_d[R,3]     = sum_s z_s d_pts  (+ d_len[r] rays_d/|rays_d| when d_len[R] is given: the term of raw2outputs' interval
 *                        scaling)  (+ (d_viewdirs - (d_viewdirs . v) v) / |rays_d| with fold_viewdirs = 1, for viewdirs v =
 *                        rays_d/|rays_d|; d_viewdirs is then formed whether or not it is returned)
 * z is a constant (the fine samples are detached, as the reference detaches z_samples).  stash: r2l_teacher_mlp_train's on the
 * same points; draw[R,S,4]; work: r2l_teacher_input_grad_work_floats(R*S) floats.  d_rays_o / d_rays_d: both or neither; each
 * of d_viewdirs, d_pts may be NULL; at least one output.  Outputs are overwritten, no row >= R is written, no atomics, fixed
 * summation order (bit-reproducible).  R == 0 is a successful no-op; 1 <= S <= 256. */
int r2l_teacher_backward_input(const float* rays_o, const float* rays_d, const float* viewdirs, const float* z,
                               const float* tparams, const float* stash, const float* draw, const float* d_len,
                               int fold_viewdirs, float* d_rays_o, float* d_rays_d, float* d_viewdirs, float* d_pts, float* work,
                               int64_t R, int S, void* stream);

/* z_out[R,S] = near*(1-t)+far*t, with stratified jitter when t_rand[R,S] != NULL (create_data.py:457-482).
 * near/far: per-ray values read at near[r*nf_stride], far[r*nf_stride]; ttab[2S] = t_vals ++ (1 - t_vals).
 * nf_stride = 1: two [R] arrays; nf_stride = 11 (8): columns 6 and 7 of [R,11] ([R,8]) ray rows, passed as rows + 6 and rows + 7;
 * nf_stride = 0: every ray reads near[0], far[0] — ONE pair shared by all rays (the frames call).  S >= 1; S = 1 gives z = near
 * (t_vals = [0]), jitter or not.  Every product and sum is rounded to fp32 on its own (no FMA), as torch's expressions are:
 * the result equals theirs bit for bit.  R == 0 is a successful no-op. */
int r2l_stratified_z(const float* near, const float* far, int nf_stride, const float* ttab, const float* t_rand,
                     float* z_out, int64_t R, int S, void* stream);

/* raw2outputs (create_data.py:335-402 == main.py:556-621 == model/nerf_raybased.py:226-295).  noise[R,S] (already
 * scaled by raw_noise_std) and weights[R,S] are optional (NULL).  1 <= S <= 256.
 * The last sample of a ray gets the interval 1e10 * |d|; S = 1 means exactly that for the one sample (alpha = 1 - exp(-relu(sigma)
 * * 1e10 |d|), weights = alpha) — the reference's own expression is degenerate there (1e10 expanded over an empty slice: no
 * sample at all) — as in r2l_raw2outputs_backward.  A ray without opacity (acc = 0) has disp = NaN (0 / 0), as the reference. */
int r2l_raw2outputs(const float* raw, const float* z, const float* rays_d, const float* noise, int white_bkgd,
                    float* rgb_map, float* disp_map, float* acc_map, float* weights, float* depth_map, int64_t R, int S,
                    void* stream);

/* Hierarchical sampling on the GPU (the reference round-trips through the CPU, create_data.py:505-515):
 *   z_samples[R,NI] = sample_pdf(.5*(z[1:]+z[:-1]), weights[:,1:-1], NI, u)     (helpers:283-330)
 *   z_all[R,S+NI]   = sort(cat[z, z_samples])  ;  z_std[R] = std(z_samples, unbiased=False)  (optional)
 * u: the uniforms, read at u[r*u_stride + i] (u_stride = 0: one shared row, e.g. det=True's linspace(0,1,NI)). */
int r2l_sample_pdf_sort(const float* z, const float* weights, const float* u, int64_t u_stride, float* z_samples,
                        float* z_all, float* z_std, int64_t R, int S, int NI, void* stream);

/* ---- teacher frames from camera poses (one library call per group of frames) ------------------------------------------------
 * What r2l_amd/render.py assembles per pose from the stages above, behind the C ABI: a host that binds this header renders a
 * teacher frame from a pose without re-implementing the ray set-up or the random draws (csrc/r2l_teacher_frame.hip).
 *
 * out[i] = (w >> 8) * 2^-24 in [0,1), w = word (i & 3) of Philox4x32-10 with
 * counter = { lo32(i>>2), hi32(i>>2), lo32(stream_id), hi32(stream_id) },
 * key = { lo32(seed), hi32(seed) }.  Pure function of (seed, stream_id, i). */
int r2l_draw_uniform(float* out, int64_t n, uint64_t seed, uint64_t stream_id, void* stream);
/* out[i] = scale * n_i (one fp32 rounding of the product), n_i standard normal by Box-Muller on the Philox4x32-10 block
 * b = i >> 2 of stream (seed, stream_id) — counter and key exactly as r2l_draw_uniform; words w0..w3:
 *   u1 = ((w0 >> 8) + 1) * 2^-24 in (0,1],  u2 = (w1 >> 8) * 2^-24 in [0,1):  r = sqrt(-2 ln u1)
 *   element 4b+0 = r cos(2 pi u2), 4b+1 = r sin(2 pi u2); elements 4b+2, 4b+3 the same from (w2, w3).
 * |n_i| <= sqrt(48 ln 2) = 5.77.  Pure function of (seed, stream_id, i).  The angle is evaluated as sincospi(2 u2) (2 u2 is exact);
 * every element is within 6 * 2^-24 * r of the real-number value (tests/test_teacher_step_gpu.py).  n == 0 is a successful no-op;
 * n < 0 or a NULL out is hipErrorInvalidValue before any launch. */
int r2l_draw_normal(float* out, int64_t n, uint64_t seed, uint64_t stream_id, float scale, void* stream);

/* Rays of K whole frames (helpers:231-257 get_rays + the viewdirs of create_data.py:138-147), one launch.
 * Ray r = (k*H + row)*W + col.  focal_dev: K device floats or NULL (focal for all).
 * Any of rays_o / rays_d / viewdirs [K*H*W,3] and rows [K*H*W,9] may be NULL; rows gets columns 0..5 = o, d.
 * Separately rounded fp32, in this order:  dirs = ((col - W*0.5)/focal, -(row - H*0.5)/focal, -1);
 * d_i = (dirs_x*R_i0 + dirs_y*R_i1) + dirs_z*R_i2;  o_i = c2w[i][3];  viewdirs = d / sqrt((d_x^2 + d_z^2) + d_y^2)
 * (the association torch.norm(d, dim=-1) uses on the GPU for a 3-vector: render() normalising these rays_d gives the same bits). */
int r2l_frame_rays(const float* c2w_dev /*[K][3][4]*/, const float* focal_dev, float focal, int K, int H, int W,
                   float* rays_o, float* rays_d, float* viewdirs, float* rows, void* stream);

/* ndc_rays (helpers:260-279) of n explicit rays [n,3]: the rays of a forward-facing (LLFF) scene in normalised device
 * coordinates.  Separately rounded fp32, in this order (extent W for cw, H for ch):
 *   r = 1/(2*focal);  cw = -(1/(r*W));  ch = -(1/(r*H))     (-1 / (W / (2 focal)) as torch evaluates it for an fp32 tensor focal:
 *                                                            number / tensor is reciprocal(tensor) * number)
 *   t  = (-(near + o_z)) / d_z;   s_i = o_i + t*d_i
 *   o' = ((cw*s_x)/s_z, (ch*s_y)/s_z, 1 + (2*near)/s_z)
 *   d' = (cw*(d_x/d_z - s_x/s_z), ch*(d_y/d_z - s_y/s_z), (-2*near)/s_z)
 * d_z == 0 gives the reference's inf / NaN.  In place is allowed (ndc_o == rays_o, ndc_d == rays_d).  n == 0 is a successful no-op;
 * n < 0, H < 1, W < 1, focal <= 0 or a NULL pointer is hipErrorInvalidValue before any launch. */
int r2l_ndc_rays(const float* rays_o, const float* rays_d, int64_t n, int H, int W, float focal, float near,
                 float* ndc_o, float* ndc_d, void* stream);

typedef struct r2l_teacher_frame_desc {
    int H, W; float focal; float near, far;
    int N_samples, N_importance;   /* N_importance 0: coarse pass only; with N_importance > 0: 3 <= N_samples <= 64,
                                      N_importance <= 192 (r2l_sample_pdf_sort); N_samples + N_importance <= 256 */
    int perturb;                   /* 0 | 1 */
    int white_bkgd; float raw_noise_std;   /* raw_noise_std must be 0 */
    int chunk_rays;                /* 0: a whole frame per pass */
    uint64_t seed, frame_id0;      /* draws of frame k: t_rand stream_id = 2*(frame_id0+k), u stream_id = 2*(frame_id0+k)+1 */
    int ndc;                       /* 0 | 1: 1 = forward-facing scenes, the stages run on the NDC image of the rays (below) */
    int reserved[3];               /* must be 0 */
} r2l_teacher_frame_desc;

/* Frame k = render(H, W, focal_k, c2w = c2w_k, ndc = False, near, far, use_viewdirs = True, ...) of create_data.py:97-176:
 * r2l_frame_rays, r2l_stratified_z, coarse r2l_teacher_mlp_cfg, r2l_raw2outputs (with weights), r2l_sample_pdf_sort, fine
 * r2l_teacher_mlp_cfg, r2l_raw2outputs — those very kernels, enqueued on `stream` with no allocation and no host
 * synchronisation; frames (and passes of chunk_rays rays within a frame) run back to back through `work`, 16-byte aligned,
 * r2l_teacher_frames_work_floats(d) floats (-1 for an invalid descriptor), sized for min(chunk_rays or H*W, H*W) rays.
 * perturb == 1: t_rand[r, s] and u[r, i] are r2l_draw_uniform elements r*N_samples + s and r*N_importance + i (r: ray within
 * its frame) of the frame's two streams, so the outputs do not depend on the grouping into calls or on chunk_rays.
 * perturb == 0: no t_rand; u_det is the one shared row of uniforms (u_stride 0).  rows[:, 6:9] receives rgb.  rgb0 (the coarse
 * pass's rgb) is written only when N_importance > 0.  K == 0 is a successful no-op.
 * ndc == 1: frame k = render(H, W, focal, rays = get_rays(H, W, focal_k, c2w_k), ndc = True, ...) (create_data.py:138-152): the ray
 * kernel writes the WORLD o, d to rows[:, 0:6] and takes viewdirs from the world d, and hands r2l_ndc_rays(o, d; near plane 1) to
 * the stages, which are the same kernels; near / far are then NDC depths (0, 1).  The NDC coefficients cw / ch take desc.focal,
 * NOT focal_dev[k]: desc.focal must be > 0 even when focal_dev is given.  That is the reference under use_rand_focal, which
 * draws rays with the scaled focal_ but calls render(H, W, focal, rays=...) with the scene's (create_data.py:816-831).  The work
 * buffer is the same size.  ndc == 0 enqueues what it always did. */
int64_t r2l_teacher_frames_work_floats(const r2l_teacher_frame_desc* d);
int r2l_teacher_frames_cfg(const float* c2w_dev, const float* focal_dev, int K, const r2l_teacher_frame_desc* d,
                           const float* ttab /*dev [2*N_samples], as r2l_stratified_z*/,
                           const float* u_det /*dev [N_importance], used when perturb == 0*/,
                           const float* wstream_coarse, const float* tparams_coarse,
                           const float* wstream_fine, const float* tparams_fine /*NULL pair: coarse net serves both passes*/,
                           float* rows /*[K*H*W,9] o,d,rgb or NULL*/, float* rgb, float* disp, float* acc, float* depth,
                           float* rgb0 /*each [K*H*W(,3)] or NULL*/, float* work, void* stream, const r2l_config* cfg);

/* ---- occupancy grid of the teacher's render (skip the samples that lie in empty space) ------------------------------------------
 * In a bounded scene most sample points of a ray lie where the trained sigma pre-activation is negative; r2l_raw2outputs turns
 * those into alpha = 0 exactly, so they add exactly nothing to a frame.  A grid of one bit per cell over a box records where sigma
 * can be positive; the samples of a launch whose cell is empty are left out of the point network (csrc/r2l_occupancy.hip):
 *   r2l_occ_compact -> r2l_teacher_mlp_cfg on the M live samples as M rows with S = 1 -> r2l_occ_scatter -> r2l_raw2outputs.
 * No point-network kernel is involved beyond being called.  All calls are stateless, check their arguments before any launch
 * (hipErrorInvalidValue, r2l_last_error names the argument), enqueue on `stream`, never synchronise and use no atomics: every
 * output position comes from a scan, and the same arguments give the same bits.  r2l_amd/occupancy.py (build_spec, compact_spec,
 * scatter_spec) restates the three calls in numpy.
 *
 * The grid is CALLER-OWNED.  bits: device, r2l_occ_bits_words(G) = ceil(G^3 / 32) words; cell (cx, cy, cz) is bit (i & 31) of word
 * (i >> 5), i = (cz*G + cy)*G + cx; the padding bits of the last word are zero.  r2l_occ_grid_init fills the fields in host fp32:
 *   inv[a] = (float)G / (hi[a] - lo[a]);   step[a] = (hi[a] - lo[a]) / (float)(G*k)      (hi - lo rounded first)
 * and refuses G < 1, G > 512, k < 1, k > 4, lo[a] >= hi[a], a value that is not finite and NULL pointers.
 * The cell of a point p is c[a] = (int)floorf((p[a] - lo[a]) * inv[a]), difference and product rounded separately (no FMA).  The
 * point is inside iff 0 <= c[a] < G on all three axes; a NaN or infinite coordinate is outside.  A point outside the box is
 * ALWAYS LIVE; a point inside is live iff its cell's bit is set.  (A point at hi[a] is outside whenever (hi - lo) * inv rounds to
 * G, which holds for the boxes whose side and G are powers of two; the rule above decides, not the real-number box.) */
typedef struct r2l_occ_grid {
    uint32_t* bits;
    int G;
    float lo[3], inv[3], step[3];
    int reserved[2];               /* must be 0 */
} r2l_occ_grid;
int64_t r2l_occ_bits_words(int G);   /* -1 outside 1 .. 512 */
int r2l_occ_grid_init(r2l_occ_grid* grid, uint32_t* bits, int G, int k, const float* lo /*host [3]*/, const float* hi /*host [3]*/);

/* Fills grid->bits from the network (wstream, tparams: as r2l_teacher_mlp_cfg; cfg picks the kernel family, NULL = default).
 * Probe (c, j), c < G, j < k, of axis a sits at lo[a] + ((float)(c*k + j) + 0.5f) * step[a] (sum, product, sum rounded separately);
 * probe (px, py, pz), p = c*k + j, has the place (pz*G*k + py)*G*k + px in PROBE ORDER.  The sigma pre-activation (raw[..., 3]) of
 * all (G k)^3 probes comes from r2l_teacher_mlp_cfg on rows with S = 1: rays_o = probe, rays_d = 0, z = 0 (the point is the probe,
 * bit for bit), viewdirs = (0, 0, 1) — sigma does not depend on the view direction.  They run in slabs of whole cells through
 * `work` (16-byte aligned, r2l_occ_build_work_floats(G, k) floats; -1 for a G or k out of range), a point's sigma does not depend
 * on the slab it is in.  A cell is occupied iff any of its k^3 probes has sigma > sigma_thresh (a NaN sigma is not above
 * anything).  The bits are then dilated by `dilate` cells: a cell's bit is the maximum over the (2 dilate + 1)^3 box of cells around
 * it, clipped at the grid's faces (three one-axis passes).  sigma_out, optional: [(G k)^3] floats in probe order, the very
 * values the bits were made from.  k must be the k given to r2l_occ_grid_init (it set step).
 * Refused: a NULL grid / bits / wstream / tparams / work, G < 1, G > 512, k < 1, k > 4, dilate < 0, a NaN sigma_thresh, inv or step
 * not positive and finite (lo >= hi), non-zero reserved, work not 16-byte aligned, an invalid cfg. */
int64_t r2l_occ_build_work_floats(int G, int k);
int r2l_occ_build(r2l_occ_grid* grid, int k, int dilate, float sigma_thresh, const float* wstream, const float* tparams,
                  const r2l_config* cfg, float* work, float* sigma_out /*[(G k)^3] or NULL*/, void* stream);

/* The live samples of rays [R] with depths z[R,S].  Sample n = r*S + s is live iff the fp32 point rays_o[r] + rays_d[r] * z[n]
 * (product and sum rounded separately, exactly as r2l_teacher_mlp_cfg forms it) is live by the rule above.  *count_out (device
 * int64) = the number M of live samples; idx_out[0..M) = their n in ASCENDING order; row i < M of out_o / out_d / out_v [.,3] and
 * out_z [.] = rays_o[r], rays_d[r], viewdirs[r] and z[n] of sample idx_out[i], copied: the arguments of r2l_teacher_mlp_cfg with
 * R = M, S = 1.  All outputs have capacity R*S; rows >= M are not written.  work: r2l_occ_compact_work_bytes(R*S) bytes (-1 for
 * R*S < 0 or >= 2^31), 4-byte aligned.  Three launches: count per 2048 samples, scan of the counts, placement.
 * R == 0 is a successful no-op that sets *count_out = 0.  Refused: a NULL grid / pointer, R < 0, S < 1, R*S >= 2^31, a grid that
 * r2l_occ_build would refuse. */
int64_t r2l_occ_compact_work_bytes(int64_t n_samples);
int r2l_occ_compact(const r2l_occ_grid* grid, const float* rays_o, const float* rays_d, const float* viewdirs, const float* z,
                    int64_t R, int S, float* out_o, float* out_d, float* out_v, float* out_z, int64_t* idx_out,
                    int64_t* count_out, void* work, void* stream);

/* raw_out[R,S,4] = 0 everywhere (a memset: sigma = +0 -> alpha = 0), then raw_out[idx[i]] = raw_live[i] for i < M (idx: distinct
 * sample numbers in [0, R*S), as r2l_occ_compact writes them; a number outside that range writes nothing).  M == 0 leaves the zero
 * fill alone; R == 0 is a successful no-op.  raw_live and raw_out 16-byte aligned.  Refused: R < 0, S < 1, R*S >= 2^31, M < 0,
 * M > R*S, a NULL or misaligned pointer. */
int r2l_occ_scatter(const float* raw_live /*[M,4]*/, const int64_t* idx /*[M]*/, int64_t M, float* raw_out, int64_t R, int S,
                    void* stream);

/* ---- occupancy inside the fused frames call: the live count stays on the device --------------------------------------------------
 * The chain above reads M on the host to size the point-network launch.  The calls below remove that read, so that empty space
 * can be skipped where nothing synchronises (r2l_teacher_frames_occ_cfg):
 *   r2l_occ_index -> r2l_teacher_mlp_live_cfg -> r2l_raw2outputs.
 * The 40 bytes a sample of copied rows, the raw_live buffer and the scatter launch of the chain above are not needed.
 *
 * idx_out[0..M) and *count_out exactly as r2l_occ_compact writes them (ascending, the same bits) and none of its row copies: the
 * same count / scan / placement kernels with the copies compiled out.  idx_out has capacity R*S; entries >= M are not written.
 * work: r2l_occ_index_work_bytes(R*S) bytes (-1 for R*S < 0 or >= 2^31), 4-byte aligned.  R == 0 is a successful no-op that sets
 * *count_out = 0.  Refused: a NULL grid / pointer, R < 0, S < 1, R*S >= 2^31, a grid that r2l_occ_build would refuse. */
int64_t r2l_occ_index_work_bytes(int64_t n_samples);
int r2l_occ_index(const r2l_occ_grid* grid, const float* rays_o, const float* rays_d, const float* z, int64_t R, int S,
                  int64_t* idx_out, int64_t* count_out, void* work, void* stream);
/* live_acc[0] += *count; live_acc[1] += total (device int64[2], caller-zeroed): one thread of one launch, ordered by `stream` behind
 * the call that wrote *count.  No atomics: calls on one stream add up exactly.  Refused: a NULL pointer, total < 0. */
int r2l_occ_live_add(const int64_t* count /*device, 1*/, int64_t total, int64_t* live_acc, void* stream);

/* ---- whole rays: does a ray meet an occupied cell? ---------------------------------------------------------------------------------
 * A light-field network cannot skip samples; whole rays are the only work it can leave out.  r2l_occ_rays asks the grid per RAY:
 * ray r is live iff any of the T points p_j = rays_o[r] + rays_d[r] * t_j, j < T, is live by the point rule pinned under
 * r2l_occ_grid above (outside the box or not finite: live; inside: the cell's bit), with
 *   dt = (far - near) / (float)T  (host fp32);   t_j = near + ((float)j + 0.5f) * dt
 * every operation rounded separately, product and sum of the point formed exactly as r2l_occ_index forms its point.  The call is
 * therefore SPECIFIED BY r2l_occ_index: with z[r, j] = t_j for all rays, ray r is live iff r2l_occ_index lists any sample n in
 * [r*T, (r+1)*T).  z[R,T] is never built: a sub-wave of 16 lanes steps a ray's depths and leaves at the first hit.
 * idx_out[0..M) = the live ray numbers in ASCENDING order (capacity R; entries >= M are not written), *count_out (device int64) = M,
 * live_out (optional, [R] bytes) = 0 or 1 per ray.  Three launches on `stream` — flag + count per 2048 rays, the scan of
 * r2l_occ_index, placement —, no atomics, no synchronisation, stateless: two calls give the same bits.  work:
 * r2l_occ_rays_work_bytes(R) bytes (-1 for R < 0 or R >= 2^31), 4-byte aligned.  R == 0 is a successful no-op that sets
 * *count_out = 0.  Refused before any launch: a NULL grid / pointer (live_out may be NULL), R < 0, R >= 2^31, T < 1, near or far not
 * finite, far < near, far - near out of fp32 range, a grid that r2l_occ_build would refuse, a misaligned work.
 *
 * WHY A DEAD RAY IS BACKGROUND (host side; r2l_amd/occupancy.py cull_steps, rays_spec).  Let the grid be dilated by at least one
 * cell and T be the smallest count with (far - near) / T * d_max <= the smallest cell side, d_max >= |rays_d[r]|.  Consecutive
 * sample points are then at most one cell side apart, so every point x of the segment [near, far] of a dead ray lies within half a
 * cell of a sample s.  s is inside the box and in a clear cell; x's cell differs from s's by at most one along each axis, so it was
 * clear BEFORE the dilation, or x is at most half a cell outside the box.  A dead ray meets no cell in which a build probe had
 * sigma > sigma_thresh: raw2outputs gives it acc = 0 and the background colour (0, or 1 - acc = 1 with white_bkgd) up to what the
 * probes missed.  For the rays of a frame d_max = sqrt(1 + (W/(2 f))^2 + (H/(2 f))^2), f the smallest focal in use. */
int64_t r2l_occ_rays_work_bytes(int64_t R);
int r2l_occ_rays(const r2l_occ_grid* grid, const float* rays_o, const float* rays_d, int64_t R, float near, float far, int T,
                 int64_t* idx_out /*[R]*/, int64_t* count_out /*device, 1*/, uint8_t* live_out /*[R] or NULL*/, void* work,
                 void* stream);
/* The two small kernels of a culled render (r2l_frame_rays -> r2l_occ_rays -> read M -> r2l_rays_gather -> r2l_forward_rays_cfg on
 * M rays -> r2l_rgb_scatter_bg), one launch each:
 *   r2l_rays_gather: out_o[i], out_d[i] = rays_o[idx[i]], rays_d[idx[i]] for i < M; an index outside [0, R) gives a NaN row and
 *     reads nothing.  M == 0 is a successful no-op.
 *   r2l_rgb_scatter_bg: rgb_out[r] = (bg, bg, bg) for every ray with live[r] == 0, and rgb_out[idx[i]] = rgb_live[i] for i < M (an
 *     index outside [0, R) writes nothing).  idx and live must come from ONE r2l_occ_rays call, so that no row is written twice;
 *     rows of live rays that idx does not list are left alone.  M == 0 needs neither rgb_live nor idx.
 * Refused: R or M negative or >= 2^31, M > R (scatter), a NaN bg, a NULL pointer that is needed. */
int r2l_rays_gather(const float* rays_o, const float* rays_d, int64_t R, const int64_t* idx, int64_t M, float* out_o /*[M,3]*/,
                    float* out_d /*[M,3]*/, void* stream);
int r2l_rgb_scatter_bg(const float* rgb_live /*[M,3]*/, const int64_t* idx /*[M]*/, int64_t M, const uint8_t* live /*[R]*/, float bg,
                       float* rgb_out /*[R,3]*/, int64_t R, void* stream);

/* The point network on an index list with a device count.  raw[R,S,4] is zero-filled first (a memset, as r2l_occ_scatter); then for
 * i < min(*count_dev, R*S) and n = idx[i]:  raw[n] = net(rays_o[n/S] + rays_d[n/S] * z[n], viewdirs[n/S]), the point formed with
 * product and sum rounded separately.  An idx[i] outside [0, R*S) reads and writes nothing at that number; nothing outside
 * raw[0 .. R*S*4) is written; a *count_dev above R*S counts as R*S, one below 1 leaves the zero fill alone.  idx has capacity R*S;
 * entries at or past the count are not read.  No host synchronisation and no atomics beyond what r2l_teacher_mlp_cfg does (the fp16x2
 * family's range control).  raw[n] has the bits r2l_teacher_mlp_cfg(..., R, S) writes at n, in every kernel family: a point is a
 * column of its tile and does not depend on its neighbours, so the call equals r2l_occ_compact -> r2l_teacher_mlp_cfg on [M,1] ->
 * r2l_occ_scatter bit for bit when idx / count_dev come from r2l_occ_index.
 * Launch: the kernels of r2l_teacher_mlp_cfg in their live instantiation (a template parameter: the plain kernels are compiled from
 * the code they always had), over a grid sized for the capacity R*S.  Tile lane i takes sample idx[i]; a workgroup (128 lanes)
 * leaves as a whole, before any LDS staging or barrier, when its first lane is at or past the count — which covers a count of 0 —,
 * and a partly filled last workgroup clamps its idle lanes to row count - 1.  The fp16x2 family keeps its range control: its live
 * kernel is followed by the rescale kernel and by the bf16x3 live kernel with run_if = GO, the dispatch of r2l_teacher_mlp_cfg;
 * cfg is consulted with the capacity (only cfg->precision matters).  The training form (r2l_teacher_mlp_train) has no live variant
 * behind THIS entry point, which writes no stash: its live form is a call of its own, r2l_teacher_mlp_train_live ("occupancy while
 * the teacher trains", below).
 * R == 0 is a successful no-op.  Refused before any launch (hipErrorInvalidValue, r2l_last_error names the argument): a NULL
 * pointer, R < 0, S < 1, R*S >= 2^31, raw not 16-byte aligned, an invalid cfg. */
int r2l_teacher_mlp_live_cfg(const float* rays_o, const float* rays_d, const float* viewdirs, const float* z /*[R,S]*/,
                             const int64_t* idx /*device, capacity R*S*/, const int64_t* count_dev /*device, 1*/,
                             const float* wstream, const float* tparams, float* raw /*[R,S,4]*/, int64_t R, int S, void* stream,
                             const r2l_config* cfg);

/* r2l_teacher_frames_cfg with each of its two r2l_teacher_mlp_cfg launches replaced by r2l_occ_index -> r2l_teacher_mlp_live_cfg on
 * the pass's grid (grid_fine NULL: grid_coarse serves both passes); every other stage, the draws and the outputs are those of
 * r2l_teacher_frames_cfg, arguments up to rgb0 included.  Still no allocation and no host synchronisation.  live_acc: NULL, or device
 * int64[2] that receives += (live samples, all samples) of every pass (r2l_occ_live_add).  work: 16-byte aligned,
 * r2l_teacher_frames_occ_work_floats(d) floats = r2l_teacher_frames_work_floats(d) + idx (2 floats per sample of the larger pass,
 * rounded up to 4) + 4 (the count) + r2l_occ_index_work_bytes of that pass in floats (rounded up to 4).  A frame equals the per-pose
 * render through r2l_occ_compact / r2l_occ_scatter on the same rays and draws bit for bit; against the frame without grids it
 * differs only on rays with a skipped sample of positive sigma.  r2l_teacher_frames_cfg itself enqueues exactly what it always did
 * and r2l_teacher_frames_work_floats is unchanged (one body serves both entry points).
 * Refused in addition to r2l_teacher_frames_cfg's refusals: a NULL grid_coarse, a grid r2l_occ_build would refuse, d->ndc == 1 (the
 * box is in world space).  The descriptor's reserved stays zero: the grids are arguments. */
int64_t r2l_teacher_frames_occ_work_floats(const r2l_teacher_frame_desc* d);
int r2l_teacher_frames_occ_cfg(const float* c2w_dev, const float* focal_dev, int K, const r2l_teacher_frame_desc* d,
                               const float* ttab, const float* u_det, const float* wstream_coarse, const float* tparams_coarse,
                               const float* wstream_fine, const float* tparams_fine, float* rows, float* rgb, float* disp, float* acc,
                               float* depth, float* rgb0, const r2l_occ_grid* grid_coarse,
                               const r2l_occ_grid* grid_fine /*NULL: grid_coarse serves both passes*/,
                               int64_t* live_acc /*device int64[2] or NULL*/, float* work, void* stream, const r2l_config* cfg);

/* ---- early ray termination: stop the teacher's rays once they are opaque ------------------------------------------------------------
 * A grid removes the samples in empty space; what it cannot remove are the samples BEHIND the first opaque surface: their cells are
 * occupied, the ray just never gets there.  Everything past the point where the transmittance T has fallen below eps adds less
 * than T to the pixel.  The LAST pass of a render (the fine pass with N_importance > 0, else the only pass) is walked front to
 * back in segments of consecutive sample numbers:
 *   zero fill of raw;  per segment [s0, s1):  r2l_occ_index_seg (without the rays whose T < eps) -> r2l_teacher_mlp_live_into_cfg
 *   -> r2l_ert_advance (T through the segment, from the raw just written);  then the unchanged r2l_raw2outputs.
 * A skipped sample keeps raw = 0, which r2l_raw2outputs turns into alpha = 0 exactly — the grids' mechanism.  The coarse pass, its
 * weights and so the fine depths are untouched bit for bit, hence for a ray terminated with transmittance T_cut (0: never):
 *   |rgb - rgb_without| <= T_cut <= eps,  the same for acc, far * that for depth
 * up to the fp32 slack of two S-term sums: the samples before the cut are identical, the skipped ones have weights that sum to at
 * most T_cut and colours in [0, 1], and white_bkgd's 1 - acc moves by the same sum the other way.
 * The calls follow the occupancy calls: stateless, arguments checked before any launch (hipErrorInvalidValue, r2l_last_error names
 * the argument), enqueued on `stream`, never synchronising, no atomics, the same arguments give the same bits, R == 0 a successful
 * no-op.  r2l_amd/ert.py (index_seg_spec, advance_spec) restates the first two in numpy.
 *
 * r2l_occ_index_seg: the index of one segment.  Sample n = r*S + s with s0 <= s < s1 is live iff
 *   (grid == NULL, or its fp32 point is live by the rule of r2l_occ_grid above)  and  (trans == NULL, or NOT (trans[r] < eps)) —
 * a NaN transmittance keeps its ray.  idx_out[0..M) = the live n in ascending order (capacity R*(s1-s0); entries >= M are not
 * written), *count_out = M.  The kernels of r2l_occ_index with one more template switch: they enumerate m in [0, R*(s1-s0)) with
 * r = m / (s1-s0), s = s0 + m % (s1-s0), which ascends in n.  work: r2l_occ_index_seg_work_bytes(R*(s1-s0)) bytes (-1 outside
 * [0, 2^31)), 4-byte aligned.  R == 0 sets *count_out = 0.  Refused: 0 <= s0 < s1 <= S violated, R < 0, S < 1, R*S >= 2^31, eps not
 * finite or <= 0 when trans != NULL, a NULL pointer other than grid / trans, a grid that r2l_occ_build would refuse. */
int64_t r2l_occ_index_seg_work_bytes(int64_t n_samples);
int r2l_occ_index_seg(const r2l_occ_grid* grid /*NULL: every point is live by the grid rule*/, const float* rays_o, const float* rays_d,
                      const float* z /*[R,S]*/, int64_t R, int S, int s0, int s1,
                      const float* trans /*device [R], or NULL: no ray is terminated*/, float eps,
                      int64_t* idx_out /*capacity R*(s1-s0)*/, int64_t* count_out, void* work, void* stream);

/* r2l_ert_advance: the transmittance through a segment.  T = 1.0f when s0 == 0 (trans is then not read), else trans[r]; for
 * s = s0 .. s1-1 in ASCENDING order T = T * f_s, one fp32 rounding per product; trans[r] = T.
 *   f_s = (1.0f - alpha_s) + 1e-10f,  alpha_s = 1.0f - __expf(-max(raw[r,s,3], 0) * dist_s),
 *   dist_s = (s == S-1 ? 1e10f : z[r,s+1] - z[r,s]) * sqrtf(d0*d0 + d1*d1 + d2*d2)  (sums left to right)
 * — the per-sample expressions of r2l_raw2outputs without noise.  The order is sequential on purpose: advance(0, a) followed by
 * advance(a, b) equals advance(0, b) bit for bit.  Refused: the range errors above, a NULL pointer, S > 256. */
int r2l_ert_advance(const float* raw /*[R,S,4]*/, const float* z /*[R,S]*/, const float* rays_d, int64_t R, int S, int s0, int s1,
                    float* trans /*[R]: read unless s0 == 0, written*/, void* stream);

/* r2l_teacher_mlp_live_cfg without its zero fill of raw, over an index list of `capacity` entries: for i < min(*count_dev, capacity)
 * and n = idx[i] in [0, R*S), raw[n] = the point network at sample n (r2l_teacher_mlp_cfg's bits there, every kernel family, the
 * fp16x2 family with its rescale and bf16x3 fallback); every other entry of raw is NOT TOUCHED.  The launch grid is sized for
 * `capacity`, not for R*S: a segment pays a segment's launch floor; cfg is consulted with the capacity.  capacity == 0 launches
 * nothing.  r2l_teacher_mlp_live_cfg is the memset plus this call with capacity = R*S.  Refused: what r2l_teacher_mlp_live_cfg
 * refuses, capacity < 0 or > R*S. */
int r2l_teacher_mlp_live_into_cfg(const float* rays_o, const float* rays_d, const float* viewdirs, const float* z /*[R,S]*/,
                                  const int64_t* idx /*device, `capacity` entries*/, const int64_t* count_dev /*device, 1*/,
                                  int64_t capacity, const float* wstream, const float* tparams, float* raw /*[R,S,4]*/, int64_t R, int S,
                                  void* stream, const r2l_config* cfg);

/* r2l_teacher_frames_occ_cfg with early termination in the last pass.  grid_coarse / grid_fine may both be NULL: the coarse pass is
 * then the plain r2l_teacher_mlp_cfg launch and the last pass skips by transmittance alone (grid_fine NULL with a grid_coarse: it
 * serves both passes, as above).  The last pass zero-fills raw once and then runs, for the segments [j*seg, min((j+1)*seg, S)):
 * r2l_occ_index_seg (trans = NULL for j = 0) -> r2l_occ_live_add (with live_acc; the total of a segment is rays*(s1-s0)) ->
 * r2l_teacher_mlp_live_into_cfg with capacity = rays*(s1-s0) -> r2l_ert_advance (not after the last segment).  Without grids the
 * coarse pass adds nothing to live_acc.  work: r2l_teacher_frames_ert_work_floats(d, ert) floats =
 * r2l_teacher_frames_occ_work_floats(d) + trans (one float per ray of a chunk, rounded up to 4).  With seg >= S of the last pass
 * there is one segment and no termination: the frame equals r2l_teacher_frames_occ_cfg's (with grids) or r2l_teacher_frames_cfg's
 * (without) bit for bit.  Refused in addition to r2l_teacher_frames_cfg's refusals (raw_noise_std is 0 there already): a NULL ert,
 * eps outside (0, 0.1], seg < 8, non-zero reserved, d->ndc == 1 WITH a grid (ndc == 1 without grids is accepted: the first way to
 * skip samples on forward-facing scenes), grid_fine without grid_coarse, a grid r2l_occ_build would refuse. */
typedef struct r2l_ert_desc {
    float eps;                     /* a ray whose transmittance is below eps at a segment boundary is terminated */
    int seg;                       /* samples per segment */
    int reserved[2];               /* must be 0 */
} r2l_ert_desc;
int64_t r2l_teacher_frames_ert_work_floats(const r2l_teacher_frame_desc* d, const r2l_ert_desc* ert);
int r2l_teacher_frames_ert_cfg(const float* c2w_dev, const float* focal_dev, int K, const r2l_teacher_frame_desc* d,
                               const float* ttab, const float* u_det, const float* wstream_coarse, const float* tparams_coarse,
                               const float* wstream_fine, const float* tparams_fine, float* rows, float* rgb, float* disp, float* acc,
                               float* depth, float* rgb0, const r2l_occ_grid* grid_coarse /*NULL: no grids*/,
                               const r2l_occ_grid* grid_fine /*NULL: grid_coarse serves both passes*/,
                               int64_t* live_acc /*device int64[2] or NULL*/, const r2l_ert_desc* ert, float* work, void* stream,
                               const r2l_config* cfg);

/* ---- test-set metric ------------------------------------------------------------------------------------------------
 * out[0] = SSIM(img1, img2): utils/ssim_torch.py:28-56,86-94 as called at main.py:46,254,334 (11x11 Gaussian sigma 1.5,
 * zero padding, C1 = 0.01^2, C2 = 0.03^2, mean over every pixel and channel), fused into one kernel + a fixed-order
 * finish.  img1/img2: device [H, W, C] fp32 (the layout render_path holds, no permute).  window_host: host pointer to
 * the 121 window values (ssim_torch.py:19-25; any 121 floats, row-major [i][j] with i along H) or NULL to have the reference's
 * computed here, bit for bit.  partial: device buffer of r2l_ssim_partial_count(H, W, C) = tilesY * tilesX * C floats with
 * tilesY = ceil(H / 16), tilesX = ceil(W / 16).  Every entry is written (none is accumulated into) on every call:
 *   partial[(c * tilesY + ty) * tilesX + tx] = sum of the SSIM map over the pixels of the 16 x 16 tile (ty, tx) of channel c
 *                                             that lie inside the image (rows 16 ty .., columns 16 tx ..)
 *   out[0] = (sum of the partials in a fixed order) * (1 / (H W C))
 * The tile sums are the finest thing this entry point exposes; tests/ssim_util.py holds each of them to an fp64 yardstick.
 * H, W, C >= 1 and C <= 65535, otherwise an error before anything is launched. */
int64_t r2l_ssim_partial_count(int H, int W, int C);
int r2l_ssim(const float* img1, const float* img2, int H, int W, int C, const float* window_host, float* partial,
             float* out, void* stream);

/* out[k] = mean over the pixels of frame k of the FLIP difference map of img_a[k] against img_b[k]: utils/flip_loss.py:70-130
 * (compute_flip: sRGB -> YCxCz, spatial CSF filters, L*a*b* + Hunt, HyAB^0.7 redistributed with pc 0.4 / pt 0.95 and
 * cmax = HyAB(green, blue)^0.7; edge and point detectors on Y; per pixel dE_c^(1 - dE_f)), replicate padding, fused into
 * one kernel + a fixed-order finish (no float atomics: bit-reproducible).  The function is symmetric in its two images.
 * img_a/img_b: device [K, H, W, 3] fp32 (the layout render_path holds, no permute); values are clamped to [0,1] first, as the
 * reference clamps them.  pixels_per_degree: main.py:373-377's standard is 0.7 * (3840 / 0.7) * pi / 180 = 67.02; the filter
 * radii ceil(0.13505 * ppd) and ceil(0.123 * ppd) are derived from it and must not exceed the compiled 10 and 9:
 * supported 0 < ppd <= 73.1, anything else is hipErrorInvalidValue.  rescale_dev: NULL (plain FLIP) or a device pointer to
 * {min_a, max_a, min_b, max_b}: each image is first mapped by 2 / (max - min) * (x - min) - 1, the [-1, 1] rescale that
 * main.py:361-363 applies to the whole stack before FLIP (a device pointer: the caller needs no host sync for the extrema).
 * map: NULL or device [K, H, W], receives the per-pixel value.  partial: device scratch of r2l_flip_partial_count(H, W, K)
 * floats.  Filter taps and constants are built on the host in double per call and passed by value. */
int64_t r2l_flip_partial_count(int H, int W, int K);
int r2l_flip(const float* img_a, const float* img_b, int K, int H, int W, float pixels_per_degree,
             const float* rescale_dev, float* partial, float* map, float* out, void* stream);

/* out[k] = LPIPS(img_a[k], img_b[k]) with the AlexNet features, version 0.1, eval mode (lpips.LPIPS(net='alex') as
 * main.py:359-369 calls it): scaling layer (x - shift) / scale, the five feature maps after their ReLUs (conv 3-64 11/4/2,
 * pool 3/2, conv 64-192 5/1/2, pool 3/2, conv 192-384, 384-256, 256-256 3/1/1; zero padding after the scaling layer), per
 * position d_l = sum_c lin_l[c] (a[c] / (|a| + 1e-10) - b[c] / (|b| + 1e-10))^2, v_l = its spatial mean, out = v_0 + .. + v_4.
 * The convolutions are exact-fp32 MFMA implicit GEMMs, the sums run in a fixed order (no float atomics): out is
 * bit-reproducible and the bits of a pair do not depend on how many pairs share the call.
 * The weights are the caller's: r2l_lpips_param_floats() = 2470848 flat floats, for l = 0..4 { conv weight [Co,Ci,kh,kw] (torch
 * order), bias [Co] }, then lin_0 .. lin_4; r2l_lpips_pack turns them once into the library-private stream wpack_dev
 * (r2l_lpips_pack_floats() floats) that r2l_lpips reads.
 * img_a/img_b: device [K, H, W, 3] fp32 (the layout render_path holds), values meant to lie in [-1, 1]; H, W >= 31.
 * rescale_dev: NULL (values used as given) or a device pointer to {min_a, max_a, min_b, max_b} as r2l_flip: each image is first
 * mapped by 2 / (max - min) * (x - min) - 1 (main.py:361-363).  work: device scratch of r2l_lpips_work_floats(K, H, W) floats
 * (-1 for K < 1 or H, W < 31).  per_layer: NULL or device [K, 5], receives v_0 .. v_4.  maps: NULL or device
 * [K, r2l_lpips_map_floats(H, W)], receives d_l(y, x): layer 0's [Ho, Wo] map first.  wpack and work must be 16-byte aligned.
 * Every argument is checked before the first launch; the call allocates and synchronises nothing and keeps no state. */
int64_t r2l_lpips_param_floats(void);
int64_t r2l_lpips_pack_floats(void);
int r2l_lpips_pack(const float* params_dev, float* wpack_dev, void* stream);
int64_t r2l_lpips_work_floats(int K, int H, int W);
int64_t r2l_lpips_map_floats(int H, int W);
int r2l_lpips(const float* img_a, const float* img_b, int K, int H, int W, const float* rescale_dev, const float* wpack,
              float* work, float* per_layer, float* maps, float* out, void* stream);

/* The VGG-16 variant (lpips.LPIPS(net='vgg'), version 0.1, eval mode: the one the published NeRF / R2L tables report), same
 * contract as r2l_lpips.  The same scaling layer, then thirteen 3/1/1 convolutions with bias and ReLU (zero padding after the
 * scaling layer): 3-64, 64-64 | 64-128, 128-128 | 128-256, 256-256, 256-256 | 256-512, 512-512, 512-512 | 512-512, 512-512,
 * 512-512, a 2/2 max-pool (floor, no padding) at each '|'; the five feature maps are the last of each group after its ReLU
 * (64, 128, 256, 512, 512 channels); d_l, v_l and out as above, lin_l with the tap's channel count.
 * r2l_lpips_vgg_param_floats() = 14716160 flat floats: for l = 0..12 { conv weight [Co,Ci,3,3] (torch order), bias [Co] }, then
 * lin_0 .. lin_4.  H, W >= 16 (16 -> 8 -> 4 -> 2 -> 1).  r2l_lpips_vgg_work_floats is -1 for K < 1, H or W < 16, or when
 * 2 K H W does not fit the kernels' int row index; the feature maps are full resolution: 236 MB per 400x400 pair (the file
 * header of csrc/r2l_lpips_vgg.hip has the plan).  maps: [K, r2l_lpips_vgg_map_floats(H, W)], layer 0's [H, W] map first. */
int64_t r2l_lpips_vgg_param_floats(void);
int64_t r2l_lpips_vgg_pack_floats(void);
int r2l_lpips_vgg_pack(const float* params_dev, float* wpack_dev, void* stream);
int64_t r2l_lpips_vgg_work_floats(int K, int H, int W);
int64_t r2l_lpips_vgg_map_floats(int H, int W);
int r2l_lpips_vgg(const float* img_a, const float* img_b, int K, int H, int W, const float* rescale_dev, const float* wpack,
                  float* work, float* per_layer, float* maps, float* out, void* stream);

/* ---- hard-ray pool (training data path) ---------------------------------------------------------------------------------
 * The three data movements of main.py:1325-1347 (n_hard_out random pool rows [o, d, rgb] appended to every batch) and
 * main.py:1410-1425 (the hard rays of the step enter the pool, appended until it is full, then replacing the rows that were
 * handed out), one kernel each, and the ranking of the per-ray errors that picks those hard rays (r2l_pool_select below): an
 * iteration needs no sort on the host's side of the ABI.
 *   r2l_pool_pick: idx_out[i], i < n_out = n_out DISTINCT rows of [0, n_rows), every row equally likely: a keyed bijection
 *     (4-round Feistel, cycle-walked) evaluated at 0 .. n_out-1 — replaces np.random.permutation(n_rows)[:n_out]; same key,
 *     same rows.
 *   r2l_pool_augment: out_{o,d,t}[B + n_out, 3] (contiguous) = the batch's rows (inputs may be column slices of a [B, 9] shard
 *     batch: row strides in floats) followed by pool rows idx[0 .. n_out).
 *   r2l_pool_store: pool[dst(i)] = [o, d, t][hard[i]], i < n_in, dst(i) = dst_idx[i] (replace) or dst0 + i (dst_idx NULL: append).
 * pool: [rows, 9] fp32 row-major.  idx / hard / dst_idx: device int64. */
int r2l_pool_pick(int64_t* idx_out, int64_t n_out, int64_t n_rows, uint64_t key, void* stream);
int r2l_pool_augment(const float* rays_o, const float* rays_d, const float* target, int64_t stride_o, int64_t stride_d,
                     int64_t stride_t, const float* pool, const int64_t* idx, int64_t B, int64_t n_out, float* out_o, float* out_d,
                     float* out_t, void* stream);
int r2l_pool_store(const float* rays_o, const float* rays_d, const float* target, int64_t stride_o, int64_t stride_d,
                   int64_t stride_t, const int64_t* hard, float* pool, const int64_t* dst_idx, int64_t dst0, int64_t n_in,
                   void* stream);

/* r2l_pool_select: the k hardest of the first B rows of a step (csrc/r2l_pool.hip: a radix select on 8-bit digits and one ordered
 * compaction; one workgroup up to 12 288 rows, up to 1024 beyond).  rgb / target: device fp32 rows of 3, row strides in floats
 * (>= 3: the step's output next to a column slice of a [B, 9] shard batch).
 *   error of row i:  e_i = fl(fl(fl(d0*d0) + fl(d1*d1)) + fl(d2*d2)),  d = rgb[i] - target[i], every operation rounded to fp32 —
 *     the SUM of squares, not the mean (dividing by 3 can merge two distinct sums into a tie).
 *   rank key:  the bit pattern of e_i as uint32 (e_i >= +0: the order of the values); any NaN -> 0xFFFFFFFF, among the hardest.
 *   result:  the rows ordered by (key descending, index ascending), the first k of them; a tie at the threshold goes to the lower
 *     index.  hard_out (device int64[k]) holds these k indices in ASCENDING INDEX order; err_out (device [B], or NULL) receives
 *     e_i of every row.
 * A pure function of its inputs: the same for every launch geometry, no position depends on the arrival order of an atomic.
 * Stateless; allocates nothing, never synchronises, enqueues on `stream`.  work: device scratch of r2l_pool_select_work_bytes B
 * bytes (-1: B < 0 or B >= 2^31), 16-byte aligned; written before it is read, so its contents on entry do not matter.
 * hipErrorInvalidValue (with r2l_last_error), checked before any launch: rgb, target, work or (with k > 0) hard_out NULL, a
 * stride below 3, B < 0, B >= 2^31, k < 0, k > B, work not 16-byte aligned.  B == 0 or k == 0 is a successful no-op.
 * r2l_amd/pool_select.py (select_spec) restates the result in numpy. */
int64_t r2l_pool_select_work_bytes(int64_t B);
int r2l_pool_select(const float* rgb, const float* target, int64_t stride_rgb, int64_t stride_t, int64_t B, int64_t k,
                    int64_t* hard_out /*[k]*/, float* err_out /*[B] or NULL*/, void* work, void* stream);

/* ---- device-resident ray store (training data path without shard files) ---------------------------------------------------
 * The teacher's [o, d, rgb] rows stay in device memory between their rendering and the student's steps, instead of being
 * written as [4096,9] .npy shards (create_data.py:854-872) and read back (main.py:759-808).  The store is CALLER-OWNED memory:
 * capacity_shards * rays_per_shard rows of 9 fp32, row-major; shard s is rows [s * rays_per_shard, (s+1) * rays_per_shard).
 * Both calls are stateless, check their arguments before any launch, enqueue one kernel on `stream` and never synchronise.
 * rays_per_shard must be a positive multiple of 4 (a shard is a whole number of 16-byte words); all offsets are 64-bit.
 *
 * pi(key, n) below is the bijection of [0, n) that the hard-ray pool's row choice evaluates (csrc/r2l_perm.h): with
 * bits = the smallest even number >= 2 with 2^bits >= n, a 4-round Feistel network F on bits/2 + bits/2 bits, round function
 * murmur3-finalizer(r ^ k[round]) masked to bits/2 bits, round keys k = mix(lo), mix(hi ^ 0x9e3779b9), mix(lo ^ 0x7f4a7c15),
 * mix(hi + 0x6a09e667) of the key's low / high 32 bits; pi(i) = the first of F(i), F(F(i)), ... that is < n (cycle walking).
 * epoch_key(seed, e) = the splitmix64 finalizer of seed + (e + 1) * 0x9E3779B97F4A7C15 (mod 2^64):
 *   z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31.
 * r2l_amd/raystore.py (perm, shard_ids) restates both in numpy.
 *
 *   r2l_store_append: writes m = floor(n_rows / rays_per_shard) shards starting at shard first_shard; output row i
 *     (i < m * rays_per_shard) is input row pi(key, n_rows)(i), the remaining n_rows mod rays_per_shard rows of the permuted
 *     sequence are dropped (create_data.py:862-872).  shuffle = 0: the identity instead of pi.  *n_written_out = m (host
 *     arithmetic).  Needs first_shard + m <= capacity_shards.  rows_in: device [n_rows, 9] fp32, must not overlap the store.
 *   r2l_store_batch: sampler and copy in one launch.  Draw t = draw0 + j, j < n_draw, takes shard
 *     id = pi(epoch_key(seed, t / n_shards), n_shards)(t % n_shards) — a fresh permutation of the shards per epoch, without
 *     replacement inside an epoch (the InfiniteSampler of main.py:759-767) — and copies it to rows
 *     [j * rays_per_shard, (j+1) * rays_per_shard) of batch.  ids_out: device int32[n_draw] receiving the ids, or NULL.
 *     A pure function of (seed, n_shards, t).  store and batch must be 16-byte aligned; n_shards >= 1 shards of the store are
 *     read (the caller keeps n_shards within what it has filled). */
int r2l_store_append(const float* rows_in, int64_t n_rows, float* store, int64_t capacity_shards, int64_t first_shard,
                     int64_t rays_per_shard, uint64_t key, int shuffle, int64_t* n_written_out, void* stream);
int r2l_store_batch(const float* store, int64_t n_shards, int64_t rays_per_shard, int64_t draw0, int64_t n_draw, uint64_t seed,
                    float* batch, int32_t* ids_out, void* stream);
/*   r2l_store_append_images: the REAL training rays of a scene as store rows, from K images and their K poses (the converters
 *     utils/convert_original_data_to_rays_*.py without the files).  With n_rows = K*H*W and m = floor(n_rows / rays_per_shard),
 *     output row i < m * rays_per_shard, counted from shard first_shard, is [o, d, rgb] of ray r = pi(key, n_rows)(i) — pi as
 *     specified for r2l_store_append above; shuffle = 0: r = i —, r = (k*H + row)*W + col:  (o, d) = the ray of pixel (row, col)
 *     under c2w_dev[k] and focal_dev[k] (NULL: focal for all) in the arithmetic pinned under r2l_frame_rays above (pixel_ray of
 *     csrc/r2l_pixel_ray.h), rgb = images[r] copied.  The tail of the permuted sequence is dropped, *n_written_out = m (host
 *     arithmetic).  BIT FOR BIT what r2l_frame_rays(rows) -> a copy of images into columns 6..8 -> r2l_store_append gives, in one
 *     launch and without the [n_rows, 9] intermediate: 12 bytes gathered and 36 written a ray.  Stateless; one kernel on `stream`,
 *     no synchronisation, 64-bit offsets; m == 0 enqueues nothing.  Refused before the launch (hipErrorInvalidValue, r2l_last_error
 *     names the argument): a NULL images / c2w_dev / store / n_written_out, K, H or W < 1, K*H*W > 2^58, focal <= 0 with a NULL
 *     focal_dev, rays_per_shard not a positive multiple of 4, a negative first_shard, first_shard + m > capacity_shards, a store
 *     that is not 16-byte aligned, images [K,H,W,3] that overlap the capacity_shards * rays_per_shard rows of the store.
 *     r2l_amd/raystore.py (append_images_spec) restates it in numpy. */
int r2l_store_append_images(const float* images /*dev [K,H,W,3]*/, const float* c2w_dev /*[K,3,4]*/,
                            const float* focal_dev /*[K] or NULL*/, float focal, int K, int H, int W,
                            float* store, int64_t capacity_shards, int64_t first_shard, int64_t rays_per_shard,
                            uint64_t key, int shuffle, int64_t* n_written_out, void* stream);
/*   r2l_store_append_live: r2l_store_append of the M rows rows_in[idx[0..M)] (idx: device, e.g. the live rays of r2l_occ_rays),
 *     without the gathered intermediate: output row i < m * rays_per_shard is input row idx[pi(key, M)(i)], m = floor(M /
 *     rays_per_shard), the tail of the permuted sequence dropped, *n_written_out = m.  BIT FOR BIT what a gather of the M rows
 *     followed by r2l_store_append(n_rows = M, key) gives, in one launch.  An index outside [0, n_rows) writes a NaN row and reads
 *     nothing.  Refused: what r2l_store_append refuses (with M in the place of its n_rows), M < 0, a NULL idx with M > 0.
 *     r2l_amd/raystore.py (append_live_spec) restates it in numpy. */
int r2l_store_append_live(const float* rows_in /*[n_rows,9]*/, int64_t n_rows, const int64_t* idx /*[M]*/, int64_t M, float* store,
                          int64_t capacity_shards, int64_t first_shard, int64_t rays_per_shard, uint64_t key, int shuffle,
                          int64_t* n_written_out, void* stream);

/* ---- compact ray store (16 bytes a ray; o and d recomputed per draw) ------------------------------------------------------------
 * A store that the TEACHER fills is redundant at 36 bytes a ray: every row of a flush group comes from r2l_teacher_frames_cfg,
 * so its o, d are a pure function of the pose's c2w, the pose's focal and the pixel — the arithmetic pinned under r2l_frame_rays
 * above (pixel_ray of csrc/r2l_pixel_ray.h, the one definition behind both).  Only rgb is information.  The compact store keeps
 * { rgb, id } per ray, 13 floats per pose and one int per shard, and r2l_cstore_batch hands out the [o, d, rgb] rows that
 * r2l_store_batch would have handed out from a plain store filled with the same groups and keys, BIT FOR BIT.
 *
 * The store is CALLER-OWNED memory described by one struct (72 bytes, no padding):
 *   rows         capacity_shards * rays_per_shard rows of 16 bytes { float rgb[3]; uint32_t id; }, 16-byte aligned; shard s is
 *                rows [s * rays_per_shard, (s+1) * rays_per_shard)
 *   pose_c2w     [capacity_poses][3][4], pose_focal [capacity_poses]: the pose table
 *   shard_pose0  [capacity_shards]: pose-table index of pose 0 of the flush group that wrote the shard
 * id is the row number inside its flush group, (k*H + row)*W + col with k the pose within the group: the ray index of
 * r2l_frame_rays / r2l_teacher_frames_cfg.  ids are unsigned 32-bit: a group of K*H*W > 2^32 - 1 rays is refused.
 * Both calls are stateless, check their arguments before any launch (hipErrorInvalidValue, r2l_last_error names the argument),
 * enqueue one kernel on `stream` and never synchronise.  r2l_amd/raystore.py (cstore_append_spec, cstore_batch_spec) restates
 * them in numpy. */
typedef struct r2l_cstore {
    void*    rows;
    float*   pose_c2w;
    float*   pose_focal;
    int32_t* shard_pose0;
    int64_t  capacity_shards, capacity_poses;   /* each < 2^31 */
    int64_t  rays_per_shard;                    /* positive multiple of 4 */
    int      H, W;                              /* the frames' size: one per store; H*W <= 2^32 - 1 */
    int      reserved[2];                       /* must be 0 */
} r2l_cstore;

/*   r2l_cstore_append: one flush group of K whole frames.  With n_rows = K*H*W and m = floor(n_rows / rays_per_shard), output row
 *     i < m * rays_per_shard of shards first_shard .. first_shard + m - 1 is { rgb[pi(key, n_rows)(i)], id = pi(key, n_rows)(i) }
 *     — pi as specified for r2l_store_append above, the tail of the permuted sequence dropped as there; shuffle = 0: the identity.
 *     rgb: device fp32, row r at rgb + r * rgb_stride (3 for the rgb output of r2l_teacher_frames_cfg, 9 for rows + 6).
 *     The K poses c2w_dev[K][3][4] and focals (focal_dev[K], or NULL: the scalar focal K times) are copied to the pose table at
 *     first_pose, shard_pose0[first_shard .. first_shard + m) = first_pose, *n_written_out = m (host arithmetic).  m == 0 enqueues
 *     nothing (no shard refers to the poses).  Refused: a NULL pointer (store, its four pointers, rgb, c2w_dev, n_written_out),
 *     K < 1, H or W < 1, K*H*W > 2^32 - 1, first_shard + m > capacity_shards, first_pose + K > capacity_poses, rays_per_shard not a
 *     positive multiple of 4, rgb_stride < 3, focal <= 0 with a NULL focal_dev, non-zero reserved, rows not 16-byte aligned.
 *   r2l_cstore_batch: draw t = draw0 + j, j < n_draw, takes the shard r2l_store_batch takes (the same sampler: a pure function
 *     of (seed, n_shards, t)); row x of that shard becomes row j * rays_per_shard + x of batch [n_draw * rays_per_shard, 9]:
 *       p = shard_pose0[shard] + id / (H*W);   row = (id % (H*W)) / W;   col = id % W
 *       [o, d] = the ray of pixel (row, col) with pose_c2w[p] and pose_focal[p], in the arithmetic of r2l_frame_rays;  rgb copied.
 *     A row whose p lies outside the pose table (a store nobody appended to) gets NaN rays; nothing outside the table is read.
 *     ids_out: device int32[n_draw] receiving the shard ids, or NULL.  batch must be 16-byte aligned; 1 <= n_shards <=
 *     capacity_shards; the other conditions are those of r2l_store_batch and of the struct.  16 bytes read and 36 written per ray. */
int r2l_cstore_append(const r2l_cstore* store, const float* rgb, int64_t rgb_stride, const float* c2w_dev, const float* focal_dev,
                      float focal, int K, int64_t first_shard, int64_t first_pose, uint64_t key, int shuffle,
                      int64_t* n_written_out, void* stream);
int r2l_cstore_batch(const r2l_cstore* store, int64_t n_shards, int64_t draw0, int64_t n_draw, uint64_t seed,
                     float* batch /*[n_draw * rays_per_shard, 9]*/, int32_t* ids_out, void* stream);

/* ---- digest of a ray store's shards (the checksums of a store file) ------------------------------------------------------------
 * r2l_words_digest (csrc/r2l_store_digest.hip): n_items items of words_per_item 32-bit words each, contiguous in device memory;
 *   out[k] = sum over i < words_per_item of epoch_key(((uint64_t)i << 32) | words[k * words_per_item + i], salt + k)   (mod 2^64)
 * with epoch_key exactly as specified for r2l_store_batch above (csrc/r2l_perm.h perm_epoch_key).  An integer sum: the result
 * does not depend on the order of the reduction, so the kernel and r2l_amd/raystore.py (words_digest_spec) agree bit for bit with
 * no order pinned.  The word's position i and the item's number k enter the hash: swapped words or swapped items change it.
 * RayStore.save / .load (r2l_amd/raystore.py; INTEGRATION.md "store file") call it with one item per shard — words_per_item =
 * rays_per_shard * 9, or * 4 for a compact store — and once per pose-table section as a single item.
 * Stateless; checks its arguments before any launch, enqueues hipMemsetAsync(out) and one kernel on `stream`, never synchronises;
 * all offsets are 64-bit.  Reads words[0 .. n_items * words_per_item), writes out[0 .. n_items) and nothing else.
 * hipErrorInvalidValue (r2l_last_error names the argument): n_items < 0, words_per_item outside [1, 2^32), words or out NULL with
 * n_items > 0, words not 4-byte aligned, out not 8-byte aligned.  n_items == 0 enqueues nothing.  Items that start on a 16-byte
 * boundary are read with 16-byte loads throughout; others through up to 3 single words at either end. */
int r2l_words_digest(const uint32_t* words, int64_t words_per_item, int64_t n_items, uint64_t salt, uint64_t* out /* dev [n_items] */,
                     void* stream);

/* r2l_train_batch: the batch of a student step in ONE launch instead of r2l_store_batch -> r2l_pool_pick -> r2l_pool_augment
 * (csrc/r2l_student_step.hip).  With B = n_draw * rays_per_shard, out_o / out_d / out_t are [B + n_out, 3] contiguous:
 *   rows [0, B):          the rows of the shards id(draw0 + j), j < n_draw — id exactly as specified for r2l_store_batch above —
 *                         de-interleaved from the store's 9-float rows [o, d, rgb];
 *   rows [B, B + n_out):  the pool rows pi(pool_key, n_pool_rows)(i), i < n_out: the index sequence of r2l_pool_pick.
 * ids_out (device int32[n_draw], or NULL) receives the shard ids, idx_out (device int64[n_out], required with n_out > 0: the
 * replace step of r2l_pool_store needs it) the picked pool rows.  n_out == 0: the shard rows alone (pool may be NULL).
 * Stateless: the arguments are checked before the launch, one kernel is enqueued on `stream`, nothing synchronises; all offsets
 * are 64-bit.  store, out_o, out_d and out_t must be 16-byte aligned (the shard words are read and the batch rows written as
 * 16-byte words).  hipErrorInvalidValue (with r2l_last_error): the conditions of r2l_store_batch, n_out < 0 or > n_pool_rows, a
 * NULL output, a NULL pool / idx_out with n_out > 0.  r2l_amd/raystore.py (train_batch_spec) restates it in numpy. */
int r2l_train_batch(const float* store, int64_t n_shards, int64_t rays_per_shard, int64_t draw0, int64_t n_draw, uint64_t seed,
                    const float* pool /*[n_pool_rows, 9]*/, int64_t n_pool_rows, int64_t n_out, uint64_t pool_key, float* out_o,
                    float* out_d, float* out_t, int32_t* ids_out, int64_t* idx_out, void* stream);

/* ---- one student training iteration in one library call --------------------------------------------------------------------
 * What r2l_amd/train_step.py and the driver's loop assemble per iteration from the stages above (RayStore.next ->
 * HardRayPool.augment -> draw_uniform -> R2LTrainer.step -> HardRayPool.update), behind the C ABI (csrc/r2l_student_step.hip): a
 * pure function of (store, pool, weights, optimizer state, descriptor).  Those very kernels with those very arguments, in this
 * order, enqueued on `stream` with no allocation and no host synchronisation; the call keeps no state.  World size 1, the uncut
 * backward (no segmented chain, no staged buckets: the all-reduce of a data-parallel step sits between 6 and 8).
 *   1. r2l_train_batch: B = n_draw * rays_per_shard shard rows + (pool_full ? n_out : 0) pool rows;  N = the sum
 *   2. r2l_draw_uniform of N*16 elements on stream `jitter_stream` of `seed` (perturb == 1; else no t_rand is passed on)
 *   3. pack == 1: r2l_pack_forward_layout / r2l_pack_backward_layout in the layouts r2l_forward_layout_for_cfg(N, 1, cfg) and
 *      r2l_backward_layout_for_cfg(N, cfg) name
 *   4. r2l_forward_rays_cfg with stash        5. hipMemsetAsync of grads
 *   6. r2l_backward_part_cfg(R2L_BWD_ALL), grad_scale = 2 lw_rgb / (3 N)      7. r2l_loss_finish, inv_denom = lw_rgb / (3 N)
 *   8. r2l_adam_step_guarded(lr, beta1, beta2, eps, step, gradient scale 1, no guard word)
 *   9. n_in > 0: r2l_pool_select of the first B rows, k = n_in, then r2l_pool_store — appended at row pool_rows while the pool is
 *      not full, replacing the rows idx_out[0 .. n_in) of step 1 once it is.
 * pack: the weight streams are packed IN FRONT of the step, as the trainer's lazy version check packs them: on exit they hold the
 * parameters the step READ, not the updated ones, and a render that follows must re-pack (r2l_amd: engine.mark_dirty()).  A host
 * that does nothing else with the weights passes pack = 0 at its first step (after packing both streams once itself) and 1 from
 * its second step on.  r2l_adam_step_packed (R2L_ADAM_PACK of the trainer) is not used by this call.  Range control and the bf16x3
 * fallback live inside the forward and backward entry points: nothing to do here.
 * The host computes pool_key (the key r2l_pool_pick would be given), jitter_stream (the trainer: 2^61 + 4096 * iteration + rank),
 * lr and the pool's fill state — plain arithmetic; passing them in is what keeps the call a pure function.
 *
 * Caller-owned: store (n_shards filled shards), pool ([pool_capacity_rows, 9]; NULL allowed when nothing is read or written:
 * n_in == 0 and no augmented rows), ztab[32], params / grads / exp_avg / exp_avg_sq (r2l_param_count(n_block) each; grads is
 * overwritten), wstream / wstream_bwd (zero-filled once after allocation, packed from params before a step with pack == 0),
 * loss_out[2] (loss, psnr), rgb_out ([N, 3], or NULL: the step's rgb then stays in the work buffer).
 * work: 16-byte aligned, r2l_student_step_work_floats(d) floats (-1 with r2l_last_error for an invalid descriptor).  Every part
 * rounded up to a multiple of 1024 floats, so that every part starts on a 4 KiB boundary; with slot = r2l_stash_slot_floats(N):
 *   o, d, t [N,3] each; t_rand [N,16] (perturb); rgb [N,3]; save_x (n_block + 1 slots), save_t (max(n_block, 1) slots), gx, gt
 *   likewise; dpre [N,3]; sqerr (r2l_num_tiles(N)); the dW slab (r2l_dw_slab_floats()); idx_out (int64 [n_out], pool_full);
 *   hard (int64 [n_in]); the scratch of r2l_pool_select (r2l_pool_select_work_bytes(B), n_in > 0).
 * hipErrorInvalidValue (with r2l_last_error naming the field or pointer) before any launch: a NULL required pointer, n_block < 0,
 * an invalid r2l_config, rays_per_shard not a positive multiple of 4, n_shards < 1, n_draw < 1, draw0 < 0, perturb / pack /
 * pool_full not 0 or 1, n_in > n_out or n_in > B, pool_rows + n_in > pool_capacity_rows while the pool is not full, pool_full with
 * n_out > pool_rows, 2^31 rays or more, step < 1, non-zero reserved, a work buffer that is not 16-byte aligned.
 * r2l_amd/train_step.py (R2LTrainer.fused_step) and tests/chost/train_host.c are the worked examples. */
typedef struct r2l_student_step_desc {
    int n_block;
    int perturb, pack, pool_full;     /* 0 | 1 */
    const r2l_config* cfg;            /* dispatch of every launch of the step; NULL = AUTO */
    int64_t rays_per_shard;           /* positive multiple of 4 */
    int64_t n_shards;                 /* FILLED shards of the store at this step, >= 1 */
    int64_t n_draw, draw0;            /* this step takes the draws draw0 .. draw0 + n_draw - 1 */
    uint64_t store_seed;              /* seed of r2l_store_batch */
    int64_t pool_capacity_rows;
    int64_t pool_rows;                /* rows filled on entry */
    int64_t n_in, n_out;              /* hard rays entering the pool per step / pool rows appended to a batch once pool_full */
    uint64_t pool_key;                /* key of r2l_pool_pick for this step (read with pool_full and n_out > 0) */
    uint64_t seed, jitter_stream;     /* r2l_draw_uniform(seed, jitter_stream) */
    double lw_rgb;
    float lr, beta1, beta2, eps;
    int64_t step;                     /* Adam's step count of this update, 1 <= step < 2^60 */
    int reserved[4];                  /* must be 0 */
} r2l_student_step_desc;
int64_t r2l_student_step_work_floats(const r2l_student_step_desc* d);   /* -1: invalid descriptor */
int r2l_student_train_step(const r2l_student_step_desc* d, const float* store, float* pool, const float* ztab, float* params,
                           float* grads, float* exp_avg, float* exp_avg_sq, float* wstream, float* wstream_bwd,
                           float* loss_out /* dev [2]: loss, psnr */, float* rgb_out /* dev [N,3] or NULL */, float* work,
                           void* stream);

/* ---- pose refinement against a trained student -------------------------------------------------------------------------------
 * Localising P observed images against a frozen student (the use r2l_backward_input names): per iteration n pixels of every image,
 * their rays under the current pose estimates, one forward and one dX chain, the ray gradients reduced to a 6-vector per pose, Adam
 * on it and a retraction onto SE(3).  (The reference has no counterpart; iNeRF-style loops do this through autograd.)  P poses, n
 * rays per pose, N = P n; ray p n + j belongs to pose p.  csrc/r2l_pose.hip; r2l_amd/pose_refine.py restates every stage in torch.
 *
 * r2l_pose_key: the key of pose p's pixel bijection at an iteration, host integer arithmetic only (no device work, no stream), with
 * epoch_key exactly as specified for r2l_store_batch above:
 *   z = epoch_key(seed ^ 0x706F73655F726566, iteration)        *key_out = epoch_key(z, p)          (iteration >= 1, p >= 0)
 *
 * r2l_pose_batch: row p n + j of rays_o / rays_d / target / ids_out is, bit for bit, row j of what r2l_image_batch writes for
 * n_img = P, img = p, the whole frame as window, ndc = 0 and the key of r2l_pose_key(seed, iteration, p): pixel pi(key, H W)(j) of
 * image p, its world ray under c2w[p] (pixel_ray of csrc/r2l_pixel_ray.h, the one definition), its colour, and its id
 * (p H + row) W + col.  n <= H W: the pixels of a pose are distinct.  One launch, arguments checked before it; n == 0 or P == 0 is a
 * successful no-op.  hipErrorInvalidValue (with r2l_last_error): a NULL required pointer (all but ids_out), P < 0, H / W < 1,
 * focal <= 0, iteration < 1, n < 0 or n > H W, P H W > 2^31 - 1.
 *
 * r2l_pose_grad: the segmented reduction, all inputs [N,3]:
 *   grad[p][0:3] = sum_j rays_d[p n + j] x d_rays_d[p n + j]    (d/dw at 0 of R <- exp([w]x) R: the rotation is about the camera
 *                                                                centre, rays_o does not move with it)
 *   grad[p][3:6] = sum_j d_rays_o[p n + j]
 *   loss[p]      = sum_j |rgb - target|^2 / (3 n)                (loss may be NULL; the divisor is the fp32 value of 3 n)
 * Outputs are OVERWRITTEN; nothing but grad, loss and work is written; no float atomics, a fixed order: two calls give the same
 * bits.  Segments need not be aligned to anything.  Every product and every difference is rounded separately (no FMA); the sums are
 * trees: four rays per lane pairwise, six shuffle levels per wave of 256 rays, then waves over 64 partials each until one is left.
 * fp32 additions on the longest path of a term: 1 + 2 + 6 + 6 ceil(log64(ceil(n / 256))) — 9 for n <= 256, 15 for n <= 16 384, 21 for
 * n <= 2^20, at most 33.  Every input is read once (16-byte loads when n % 4 == 0 and the inputs are 16-byte aligned).
 * work: r2l_pose_grad_work_floats(P, n) floats, 16-byte aligned (0 floats, and work may be NULL, for n <= 256).
 * hipErrorInvalidValue: a NULL required pointer, P < 0, n < 1 (with P > 0), P n >= 2^31, a NULL / misaligned work with n > 256.
 *
 * r2l_pose_update: per pose, with g = grad[p] and u = 2^-24:
 *   not all six g finite: pose, exp_avg and exp_avg_sq of p keep their bits (one bad query does not poison the batch).  Else
 *   m' = m + (g - m)(1 - beta1)   v' = v beta2 + g^2 (1 - beta2)   delta = -(lr / (1 - beta1^step)) (m' / (sqrt(v') / sqrt(1 - beta2^step) + eps))
 *   — torch.optim.Adam's update of a zero 6-vector, evaluated as r2l_adam_step evaluates it — lr = lr_rot for delta[0:3] = dw,
 *   lr_trans for delta[3:6] = dv;  R <- exp([dw]x) R = R + A [dw]x R + B [dw]x [dw]x R,  A = sin(th) / th = 2 sin(th/2) cos(th/2) / th,
 *   B = (1 - cos(th)) / th^2 = 2 sin^2(th/2) / th^2, and below th^2 < 1e-4 (th < 0.01) by their series A = 1 - th^2/6 + th^4/120,
 *   B = 1/2 - th^2/24 + th^4/720;  one modified Gram-Schmidt pass over the columns of R in the order 0, 1, 2;  t <- t + dv.
 *   dw == 0 exactly (a zero gradient on zero moments): R keeps its bits — the Gram-Schmidt pass belongs to the rotation.
 * c2w [P,3,4] in place; exp_avg, exp_avg_sq, grad [P,6].  hipErrorInvalidValue: a NULL pointer, P < 0, step < 1.
 *
 * r2l_pose_refine_step: one iteration for all P poses in one call — the same kernels with the same arguments in this order on
 * `stream`, no allocation, no synchronisation, no state (the mould of r2l_student_train_step):
 *   1. r2l_pose_batch at (seed, iteration)
 *   2. pack == 1: r2l_pack_forward_layout / r2l_pack_backward_layout in the layouts r2l_forward_layout_for_cfg(N, 1, cfg) and
 *      r2l_backward_layout_for_cfg(N, cfg) name (the weights are frozen: a host packs once and passes 0 afterwards)
 *   3. r2l_forward_rays_cfg with the stash, t_rand = NULL; ztab is the test-time table (z_lower = PointSampler.z_vals, z_span = 0)
 *   4. r2l_backward_part_cfg, parts = R2L_BWD_CHAIN, MSE mode, grad_scale = 2 / (3 n) — every pose's loss is its own mean; no weight-
 *      gradient stage, no slab, `grads` is not touched (dpre stands in for the pointer)
 *   5. r2l_backward_input in the ray form, without d_emb          6. r2l_pose_grad -> grad, loss_out
 *   7. r2l_pose_update with step = iteration
 * loss_out: device [P] (the host passes another row per iteration and reads them when it likes).  images: device [P,H,W,3];
 * c2w, exp_avg, exp_avg_sq as r2l_pose_update; wstream / wstream_bwd zero-filled once after allocation.
 * work: 16-byte aligned, r2l_pose_refine_work_floats(d) floats (-1 with r2l_last_error for an invalid descriptor); every part is
 * rounded up to a multiple of 1024 floats, so that every part starts on a 4 KiB boundary; with slot = r2l_stash_slot_floats(N):
 *   rays_o, rays_d, target, rgb [N,3] each; save_x (n_block + 1 slots), save_t (max(n_block, 1) slots), gx, gt likewise; dpre [N,3];
 *   sqerr (r2l_num_tiles(N)); d_rays_o, d_rays_d [N,3]; grad [P,6]; the scratch of r2l_pose_grad.
 * hipErrorInvalidValue (r2l_last_error names the field or pointer) before any launch: a NULL required pointer, n_block out of
 * range, an invalid r2l_config, P < 1, n < 1, H / W < 1, n > H W, P H W or N >= 2^31, iteration < 1, focal <= 0, pack not 0 or 1,
 * non-zero reserved, a work buffer that is not 16-byte aligned.  Range control and the bf16x3 fallback live inside the forward and
 * backward entry points.  r2l_amd/pose_refine.py (PoseRefiner.fused_step) is the worked example. */
int r2l_pose_key(uint64_t seed, int64_t iteration /*>= 1*/, int64_t p, uint64_t* key_out);
int r2l_pose_batch(const float* images /*dev [P,H,W,3]*/, const float* c2w /*dev [P,3,4]*/, int P, int H, int W, float focal,
                   uint64_t seed, int64_t iteration, int64_t n, float* rays_o, float* rays_d, float* target /*each [P*n,3]*/,
                   int64_t* ids_out /*[P*n] or NULL*/, void* stream);
int64_t r2l_pose_grad_work_floats(int64_t P, int64_t n);   /* -1: P or n negative, or P n >= 2^31 */
int r2l_pose_grad(const float* rays_d, const float* d_rays_o, const float* d_rays_d, const float* rgb, const float* target,
                  int64_t P, int64_t n, float* grad /*[P,6]*/, float* loss /*[P] or NULL*/, float* work, void* stream);
int r2l_pose_update(float* c2w /*[P,3,4]*/, float* exp_avg, float* exp_avg_sq, const float* grad /*[P,6] each*/, int P,
                    float lr_rot, float lr_trans, float beta1, float beta2, float eps, int64_t step /*>= 1*/, void* stream);
typedef struct r2l_pose_refine_step_desc {
    int n_block;
    int pack;                         /* 0 | 1 */
    const r2l_config* cfg;            /* dispatch of every launch of the step; NULL = AUTO */
    int P, H, W;                      /* poses = observed images, each H x W */
    float focal;
    int64_t n;                        /* rays per pose and iteration, 1 <= n <= H W */
    uint64_t seed;
    int64_t iteration;                /* 1-based: names the pixels and is Adam's step count; 1 <= iteration < 2^60 */
    float lr_rot, lr_trans, beta1, beta2, eps;
    int reserved[4];                  /* must be 0 */
} r2l_pose_refine_step_desc;
int64_t r2l_pose_refine_work_floats(const r2l_pose_refine_step_desc* d);   /* -1: invalid descriptor */
int r2l_pose_refine_step(const r2l_pose_refine_step_desc* d, const float* images /*dev [P,H,W,3]*/, float* c2w /*dev [P,3,4]*/,
                         float* exp_avg, float* exp_avg_sq /*dev [P,6] each*/, const float* ztab, const float* params,
                         float* wstream, float* wstream_bwd, float* loss_out /*dev [P]*/, float* work, void* stream);

/* ---- pixel sampler of teacher training (batching mode without a bank of rays) ----------------------------------------------
 * The reference's use_batching mode (main.py:1137-1162, 1199-1210) builds the rays of every pixel of every training image,
 * shuffles that bank and hands out N_rand rows per step.  Here one draw is one pixel and its ray is computed when it is drawn:
 * with M = n_img*H*W, draw t = draw0 + j, j < n_draw, takes pixel
 *   g = pi(epoch_key(seed, t / M), M)(t % M)            (pi and epoch_key exactly as specified for r2l_store_batch above)
 * — a fresh permutation of all pixels per epoch, without replacement inside an epoch, a pure function of (seed, M, t) — and
 * g = (img*H + row)*W + col.  Outputs, each [n_draw,3]:
 *   target[j]   = images[img,row,col,:]
 *   the world ray (o, d) of pixel (row, col) under c2w[img], separately rounded fp32 in the order given for r2l_frame_rays
 *   viewdirs[j] = d / sqrt((d_x^2 + d_z^2) + d_y^2)      (always of the WORLD d)
 *   rays_o[j], rays_d[j] = (o, d) with ndc == 0; with ndc == 1 their r2l_ndc_rays image at near plane 1, cw / ch from focal
 *   ids_out[j]  = g                                      (device int64[n_draw], or NULL)
 * Stateless: the arguments are checked before any launch, one kernel is enqueued on `stream`, nothing synchronises.  n_draw == 0
 * is a successful no-op.  hipErrorInvalidValue (with r2l_last_error): a NULL required pointer (all but ids_out), n_img / H / W < 1,
 * focal <= 0, draw0 < 0, n_draw < 0, ndc not 0 or 1, M > 2^31 - 1.  r2l_amd/pixel_batch.py (pixel_ids, host_batch) restates it. */
int r2l_pixel_batch(const float* images /*dev [n_img,H,W,3]*/, const float* c2w /*dev [n_img,3,4]*/, int n_img, int H, int W,
                    float focal, int ndc, int64_t draw0, int64_t n_draw, uint64_t seed, float* rays_o, float* rays_d,
                    float* viewdirs, float* target /*each [n_draw,3]*/, int64_t* ids_out /*[n_draw] or NULL*/, void* stream);

/* ---- pixel sampler of teacher training, images mode (one image and a window of it per iteration) ---------------------------
 * The reference's no_batching mode (main.py:1260-1302) draws one training image per iteration and N_rand of its pixels without
 * replacement, for the first precrop_iters iterations from a centre crop.  Here draw j < n_draw takes position
 *   q = pi(key, win_h*win_w)(j)                          (pi exactly as specified for r2l_store_append above)
 * of the win_h x win_w window whose first pixel is (row0, col0), row-major: row = row0 + q / win_w, col = col0 + q % win_w.
 * A prefix of a bijection: the n_draw <= win_h*win_w pixels are distinct.  The five outputs are, bit for bit, what r2l_pixel_batch
 * writes for pixel (img, row, col): target, the world ray, viewdirs of the world d, the r2l_ndc_rays image at near plane 1 with
 * ndc == 1, and ids_out[j] = (img*H + row)*W + col (one per-pixel body serves both kernels).
 * Stateless: the arguments are checked before any launch, one kernel is enqueued on `stream`, nothing synchronises.  n_draw == 0
 * is a successful no-op; all offsets are 64-bit.  hipErrorInvalidValue (with r2l_last_error): what r2l_pixel_batch refuses (a NULL
 * required pointer, n_img / H / W < 1, focal <= 0, n_draw < 0, ndc not 0 or 1, n_img*H*W > 2^31 - 1), img outside [0, n_img),
 * win_h < 1 or win_w < 1, a window that leaves the frame (row0 < 0, row0 + win_h > H, col0 < 0, col0 + win_w > W),
 * n_draw > win_h*win_w.  r2l_amd/image_batch.py (window_ids, host_batch) restates it.
 *
 * r2l_image_draw: the image and the key of an iteration, host integer arithmetic only (no device work, no stream).  With
 * epoch_key exactly as specified for r2l_store_batch above:
 *   z        = epoch_key(seed ^ 0x696D675F6D6F6465, iteration)            (iteration >= 1)
 *   *img_out = ((z >> 40) * n_img) >> 24                                  (the top 24 bits of z scaled to [0, n_img))
 *   *key_out = epoch_key(z, 0)
 * A pure function of (seed, iteration, n_img): a C host trains in images mode with r2l_image_draw -> r2l_image_batch ->
 * r2l_teacher_train_step and resumes with no sampler state.  hipErrorInvalidValue: iteration < 1, n_img < 1, a NULL output. */
int r2l_image_batch(const float* images /*dev [n_img,H,W,3]*/, const float* c2w /*dev [n_img,3,4]*/, int n_img, int H, int W,
                    float focal, int ndc, int img, int row0, int col0, int win_h, int win_w, uint64_t key, int64_t n_draw,
                    float* rays_o, float* rays_d, float* viewdirs, float* target /*each [n_draw,3]*/,
                    int64_t* ids_out /*[n_draw] or NULL*/, void* stream);
int r2l_image_draw(uint64_t seed, int64_t iteration /*>= 1*/, int n_img, int* img_out, uint64_t* key_out);

/* ---- one teacher training step in one library call ------------------------------------------------------------------------
 * What r2l_amd/teacher_train.py (TeacherTrainer.forward_backward + adam) assembles per step from the stages above, behind the C
 * ABI (csrc/r2l_teacher_step.hip): a pure function of (weights, optimizer state, batch, seed, step).  Those very kernels, in this
 * order, enqueued on `stream` with no allocation and no host synchronisation; the call keeps no state:
 *   r2l_stratified_z (near / far shared, nf_stride 0) -> coarse r2l_teacher_mlp_train -> r2l_raw2outputs (weights) ->
 *   r2l_sample_pdf_sort -> fine r2l_teacher_mlp_train -> r2l_raw2outputs_backward + r2l_teacher_backward + r2l_loss_finish of the
 *   fine net, then of the coarse net -> loss_out -> r2l_adam_step over [coarse | fine] -> r2l_pack_teacher of both nets.
 * N_importance == 0: the coarse net alone (no sampling, no fine pass); wstream_fine must be NULL exactly then.
 * params / grads / exp_avg / exp_avg_sq: n_nets * r2l_teacher_param_count() floats, [coarse | fine] (n_nets = 2 with
 * N_importance > 0, else 1); grads is overwritten.  On entry wstream_coarse / wstream_fine (r2l_teacher_stream_floats() each, zero-
 * filled once after allocation) must be packed from params (r2l_pack_teacher); on exit they are packed from the UPDATED params: a
 * test-set render, or the next step, follows directly.  rays_o / rays_d / viewdirs / target: device [N_rand,3].
 * loss_out (device [2]): loss_out[0] = mse_fine + mse_coarse (one fp32 add, fine first; the coarse mse alone without a fine net),
 * loss_out[1] = psnr of the fine net (of the coarse net when it is alone), each mse / psnr as r2l_loss_finish with 1/(3 N_rand).
 * Adam: r2l_adam_step(lr, beta1, beta2, eps, step, grad_scale 1); its bias corrections take min(step, 2^31 - 1).
 *
 * Draws: made inside the call, stream_id = 2^62 + 4*step + k of `seed` (the frames call uses stream ids 2*frame_id, far below;
 * the student's training loop with its device pool draws the jitter of iteration i on rank r from stream 2^61 + 4096*i + r of
 * r2l_draw_uniform, element ray*16 + sample: between the two, apart from both for any run length and rank count in use):
 *   k = 0  t_rand[r,s]      element r*N_samples + s                    of r2l_draw_uniform        (perturb == 1)
 *   k = 1  u[r,i]           element r*N_importance + i                 of r2l_draw_uniform        (perturb == 1, N_importance > 0)
 *   k = 2  coarse noise     element r*N_samples + s                    of r2l_draw_normal, scale = raw_noise_std   (raw_noise_std > 0)
 *   k = 3  fine noise       element r*(N_samples + N_importance) + j   of r2l_draw_normal, scale = raw_noise_std   (.. and N_importance > 0)
 * perturb == 0: no t_rand, and u is the one shared row u_det (u_stride 0), required exactly then (with N_importance > 0).
 * raw_noise_std == 0: no noise buffers, the kernels receive NULL.  The noise of a net is the same in its r2l_raw2outputs and its
 * r2l_raw2outputs_backward.
 *
 * work: 16-byte aligned, r2l_teacher_step_work_floats(d) floats (-1 with r2l_last_error for an invalid descriptor).  With
 * R = N_rand, S = N_samples, T = S + N_importance, every part rounded up to a multiple of 1024 floats (4 KiB), it holds
 *   near/far (2), z [R,S], coarse raw [R,S,4], coarse stash (r2l_teacher_stash_floats(R*S)), rgb [R,3] + disp, acc, depth [R] of
 *   the coarse r2l_raw2outputs, draw [R,T,4], sqerr [R] and mse/psnr (2) per net, the scratch of r2l_teacher_backward
 *   (r2l_teacher_train_work_floats(R*T)), t_rand [R,S] (perturb), coarse noise [R,S] (raw_noise_std > 0), and with N_importance > 0:
 *   weights [R,S], z_samples [R,N_importance], z_all [R,T], fine raw [R,T,4], fine stash (r2l_teacher_stash_floats(R*T)),
 *   u [R,N_importance] (perturb), fine noise [R,T] (raw_noise_std > 0).
 * hipErrorInvalidValue (with r2l_last_error naming the field or pointer) before any launch: N_rand < 1, the sample limits of
 * r2l_teacher_frame_desc, perturb / white_bkgd not 0 or 1, raw_noise_std < 0 or not finite, near >= far, step < 1 or >= 2^60,
 * non-zero reserved, a NULL required pointer, a wstream_fine that does not match N_importance (NULL with N_importance > 0, or
 * given with N_importance == 0), a missing u_det, an unaligned work.  r2l_amd/teacher_train.py (TeacherTrainer.fused_step) is the worked example. */
typedef struct r2l_teacher_step_desc {
    int N_rand;                     /* rays of this step, >= 1 */
    int N_samples, N_importance;    /* limits as r2l_teacher_frame_desc; N_importance == 0: coarse net only */
    int perturb, white_bkgd;        /* 0 | 1 */
    float raw_noise_std;            /* >= 0 */
    float near, far;                /* near < far; one pair for all rays */
    float lr, beta1, beta2, eps;
    int64_t step;                   /* 1-based iteration = Adam's step count; 1 <= step < 2^60 */
    uint64_t seed;
    int reserved[4];                /* must be 0 */
} r2l_teacher_step_desc;
int64_t r2l_teacher_step_work_floats(const r2l_teacher_step_desc* d);   /* -1: invalid descriptor */
int r2l_teacher_train_step(const r2l_teacher_step_desc* d,
        const float* rays_o, const float* rays_d, const float* viewdirs, const float* target, /* dev, each [N_rand,3] */
        const float* ttab, const float* u_det,      /* as r2l_teacher_frames_cfg; u_det needed iff perturb==0 && N_importance>0 */
        float* params, float* grads, float* exp_avg, float* exp_avg_sq,   /* [coarse | fine], r2l_teacher_param_count() each */
        float* wstream_coarse, float* wstream_fine, /* wstream_fine NULL iff N_importance == 0 */
        float* loss_out /* dev [2]: loss, psnr */, float* work, void* stream);

/* ---- occupancy while the teacher trains: the training step on the live samples -----------------------------------------------
 * With raw_noise_std == 0 a sample whose sigma pre-activation is not positive has alpha = 0 exactly in r2l_raw2outputs and an exactly
 * zero row of d loss / d raw in r2l_raw2outputs_backward (relu' = 0 on sigma, weight 0 on the colours): it adds exact zeros to every
 * weight gradient.  Leaving such samples out of the forward AND the backward changes a step by summation order only, as long as the
 * grid skips no sample of positive sigma; what a grid costs in training is its staleness between refreshes, not a biased gradient.
 * The three calls below are r2l_teacher_mlp_train, r2l_teacher_backward and r2l_teacher_train_step on an index list whose count stays
 * on the device (r2l_occ_index).  All are stateless, check their arguments before any launch (hipErrorInvalidValue, r2l_last_error
 * names the argument), enqueue on `stream`, never synchronise, use no atomics and give the same bits for the same arguments.  The plain
 * calls enqueue what they always did: the live kernels are instantiations of their own (template parameters / wrappers around the
 * one GEMM body).
 *
 * r2l_teacher_mlp_train_live: the fp32-MFMA training forward launched over the capacity P = R*S; tile lane i < count =
 * min(*count_dev, P) takes sample n = idx[i].  raw[R,S,4] is zero-filled first (a memset), then raw[n] gets the bits
 * r2l_teacher_mlp_train(..., R, S) writes at n.  The stash is COMPACT: slot l sits at the offset a stash of P points has it
 * (r2l_teacher_stash_floats(P) floats in all), and row i of a slot holds the layer output of sample idx[i], bit for bit the plain
 * call's row idx[i]; rows at or past the count are not written.  A workgroup (128 lanes) with no lane below the count leaves as a
 * whole before any staging or barrier.  An idx[i] outside [0, P) reads and writes nothing (neither raw nor its stash row).
 * R == 0 is a successful no-op.  Refused: a NULL pointer, R < 0, S < 1, R*S >= 2^31, raw or stash not 16-byte aligned. */
int r2l_teacher_mlp_train_live(const float* rays_o, const float* rays_d, const float* viewdirs, const float* z /*[R,S]*/,
                               const int64_t* idx /*device, capacity R*S*/, const int64_t* count_dev /*device, 1*/,
                               const float* wstream, const float* tparams, float* raw /*[R,S,4]*/, float* stash, int64_t R, int S,
                               void* stream);
/* r2l_teacher_backward on the live samples.  stash: r2l_teacher_mlp_train_live's on the same idx / count_dev; draw[R,S,4] as
 * r2l_raw2outputs_backward writes it.  work: r2l_teacher_train_live_work_floats(P) = r2l_teacher_train_work_floats(P) + 4 P floats
 * (-1 for P < 0); a first small kernel gathers draw[idx[p]] to [count,4] there (zero for an idx[p] outside [0, P)).  Every GEMM
 * launch of the chain is sized for the capacity and reads count = min(*count_dev, P) itself: dX tiles (128 rows) whose first row is
 * at or past the count leave whole; weight-gradient chunks (2048 points) at or past the count contribute nothing, and the slab
 * reduce sums the live chunks in increasing order.  The encoder operand reads ray idx[p] / S and z[idx[p]].
 * grads equals, BIT FOR BIT, r2l_teacher_backward on the compacted problem: rows rays_o[idx/S], rays_d[idx/S], viewdirs[idx/S] and
 * z.flat[idx] as [M,1], the stash slots gathered to the layout of M points, and draw.flat[idx].  A count of 0 gives all-zero grads;
 * a count above P counts as P; R == 0 zero-fills grads.  Refused: a NULL pointer, R < 0, S < 1, R*S >= 65535 * 128. */
int64_t r2l_teacher_train_live_work_floats(int64_t P);
int r2l_teacher_backward_live(const float* rays_o, const float* rays_d, const float* viewdirs, const float* z /*[R,S]*/,
                              const int64_t* idx, const int64_t* count_dev, const float* tparams, const float* stash,
                              const float* draw /*[R,S,4]*/, float* grads, float* work, int64_t R, int S, void* stream);
/* r2l_teacher_train_step with each pass's r2l_teacher_mlp_train replaced by r2l_occ_index -> r2l_teacher_mlp_train_live on the pass's
 * grid (grid_fine NULL: grid_coarse serves both passes) and each r2l_teacher_backward by r2l_teacher_backward_live on the same
 * idx / count; the draws, r2l_raw2outputs, r2l_sample_pdf_sort, r2l_raw2outputs_backward, the loss, Adam and the re-pack are those of
 * r2l_teacher_train_step, arguments up to loss_out included.  Still no allocation and no host synchronisation.  live_acc: NULL, or
 * device int64[2] that receives += (live samples, all samples) of every pass (r2l_occ_live_add).  work: 16-byte aligned,
 * r2l_teacher_step_occ_work_floats(d) floats (-1 with r2l_last_error for a descriptor the call would refuse): the parts of
 * r2l_teacher_step_work_floats with the backward's scratch that of r2l_teacher_backward_live, then idx (2 floats per sample) and the
 * count (4) of each pass and r2l_occ_index_work_bytes of the larger pass, every part rounded up to 4 KiB.  With all-ones grids the
 * step equals r2l_teacher_train_step bit for bit; r2l_teacher_train_step itself enqueues exactly what it always did and
 * r2l_teacher_step_work_floats is unchanged (one body serves both entry points).
 * Refused in addition to r2l_teacher_train_step's refusals: a NULL grid_coarse, a grid r2l_occ_build would refuse,
 * d->raw_noise_std > 0 (noise can lift a skipped sample above zero), N_rand * (N_samples + N_importance) >= 65535 * 128.  The
 * descriptor's reserved stays zero: the grids are arguments.  r2l_amd/teacher_train.py (TeacherTrainer.set_occupancy) is the worked
 * example. */
int64_t r2l_teacher_step_occ_work_floats(const r2l_teacher_step_desc* d);
int r2l_teacher_train_step_occ(const r2l_teacher_step_desc* d,
        const float* rays_o, const float* rays_d, const float* viewdirs, const float* target,
        const float* ttab, const float* u_det,
        float* params, float* grads, float* exp_avg, float* exp_avg_sq,
        float* wstream_coarse, float* wstream_fine,
        float* loss_out, const r2l_occ_grid* grid_coarse, const r2l_occ_grid* grid_fine /*NULL: grid_coarse serves both passes*/,
        int64_t* live_acc /*device int64[2] or NULL*/, float* work, void* stream);

/* ---- frame writer (host threads; test-set evaluation) ------------------------------------------------------------------
 * Replaces `imageio.imwrite(filename, to8b(rgb))` of every prediction / ground-truth frame in render_path (main.py:337-344):
 * a pool of encoder threads (zlib, Sub filter; lossless, so the decoded pixels are the bytes handed over).  `pixels`: HOST
 * buffer of H*W*C bytes (C = 1, 3 or 4; row-major), owned by the caller and left untouched until the job is done;
 * `ready_event`: NULL, or a hipEvent_t the worker waits for before reading `pixels` (the frame's asynchronous device-to-host
 * copy).  r2l_png_writer_wait(job): job and all earlier ones are on disk (job < 0: everything submitted); non-zero if any
 * job failed (r2l_last_error).  level: zlib 0..9 (1: ~2 ms per 400x400 frame). */
typedef struct r2l_png_writer r2l_png_writer;
int r2l_png_writer_open(int n_threads, int level, r2l_png_writer** out);
int r2l_png_writer_submit(r2l_png_writer* w, const char* path, const unsigned char* pixels, int H, int W, int C,
                          void* ready_event, int64_t* job_id);
int r2l_png_writer_wait(r2l_png_writer* w, int64_t job_id);
int r2l_png_writer_close(r2l_png_writer* w);

/* ---- ray-shard reader (host threads; --data_mode rays) ------------------------------------------------------------
 * Replaces BlenderDataset_v2.__getitem__ (dataset/load_blender.py:257-324: np.load of one [4096,9] f32 shard),
 * InfiniteSamplerWrapper (main.py:759-776: random permutations of the file list, forever) and the DataLoader's
 * batch_size=N_rand collate + pin_memory (main.py:794-806).  `slot_ptrs[depth]` are caller-owned (pinned) host buffers
 * of files_per_batch * rows * cols * 4 bytes each; reader threads pread() shard payloads straight into them.  All
 * shards must have the shape of paths[0].  Format: NumPy .npy v1/v2/v3, '<f4', C order, 2-D. */
typedef struct r2l_reader r2l_reader;
int r2l_npy_shape(const char* path, int64_t* rows, int64_t* cols);
int r2l_reader_open(const char* const* paths, int64_t n_paths, int files_per_batch, int n_threads, uint64_t seed,
                    void* const* slot_ptrs, int depth, r2l_reader** out);
int r2l_reader_info(r2l_reader* r, int64_t* rows, int64_t* cols, int64_t* files_read);
/* Blocks until the oldest scheduled batch is complete; *slot = index of the buffer holding it.  The buffer is not
 * rewritten until r2l_reader_release(slot), which queues the next batch into it. */
int r2l_reader_next(r2l_reader* r, int* slot);
int r2l_reader_release(r2l_reader* r, int slot);
int r2l_reader_close(r2l_reader* r);

#ifdef __cplusplus
}
#endif
#endif /* R2L_HIP_H */
