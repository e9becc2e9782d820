// r2l_dispatch.h — which kernels serve a call (host only; no device code).
// Four arithmetic families (fp32 MFMA, fp16x2, bf16x3, fp16-hi dW), three tilings, three stash formats and a fallback chain behind
// every fp16 launch: THE rule that picks among them is r2l_plan() (r2l_dispatch.hip).  Every *_cfg entry point checks the caller's
// config, resolves ONE R2LPlan and hands its fields down; the launchers take what they need as arguments and decide nothing.  The
// forward and the backward of a step resolve the same plan from the same inputs — that is what makes them agree on the stash
// format — and the host-side queries of include/r2l_hip.h are reads of plan fields.  A non-zero r2l_config field wins; an AUTO (0)
// field falls through to the R2L_* environment switch it replaces, all read in one function (r2l_env_read), per call.
#pragma once
#include "r2l_common.h"

// What is wrong with a caller's r2l_config, or nullptr.  Every *_cfg entry point checks before it does anything else:
// launch entry points fail with hipErrorInvalidValue (R2L_CFG_ENTER), the host-side queries return -1 (R2L_CFG_QUERY).
static inline const char* r2l_cfg_check(const r2l_config* c) {
    if (c == nullptr) return nullptr;
    if (c->precision < 0 || c->precision > R2L_PRECISION_FP32_MFMA) return "r2l_config.precision: not an R2L_PRECISION_* value";
    if (c->tiling < 0 || c->tiling > R2L_TILING_COOPF) return "r2l_config.tiling: not an R2L_TILING_* value";
    if (c->tiling == R2L_TILING_COOP_RETIRED) return "r2l_config.tiling: 2 (the 32-ray fp32-MFMA cooperative kernels) was retired in round 5 — R2L_TILING_COOP16 serves those launches";
    if (c->coop_tiles < 0 || c->coop_tiles > 3) return "r2l_config.coop_tiles: 0 (auto), 1, 2 or 3 (mixed)";
    if (c->reserve_cus < -1) return "r2l_config.reserve_cus: -1 (none), 0 (auto) or a CU count";
    if (c->dw_mode < 0 || c->dw_mode > R2L_DW_EXACT) return "r2l_config.dw_mode: not an R2L_DW_* value";
    if (c->reserved[0] || c->reserved[1] || c->reserved[2]) return "r2l_config.reserved: must be 0";
    return nullptr;
}
#define R2L_CFG_CHECK(cfg, fail)                          \
    if (const char* r2l_why_ = r2l_cfg_check(cfg)) {      \
        r2l_set_error_msg(r2l_why_);                      \
        return fail;                                      \
    }
#define R2L_CFG_ENTER(cfg) R2L_CFG_CHECK(cfg, (int)hipErrorInvalidValue)
#define R2L_CFG_QUERY(cfg) R2L_CFG_CHECK(cfg, -1)

enum { R2L_ARITH_FP32 = 0, R2L_ARITH_BF16X3 = 1, R2L_ARITH_FP16X2 = 2 };
// chain kernels (forward launch / dX chain).  FP16: r2l_fwd2 / r2l_bwd2, or r2l_coopf_* when the plan's tiling is COOPF, with
// the bf16x3 kernels launched behind them as range-guard fallback (they return at once unless the status word is raised)
enum { R2L_CHAIN_FP32 = 0, R2L_CHAIN_COOP16 = 1, R2L_CHAIN_BF16X3 = 2, R2L_CHAIN_FP16 = 3 };
// The one-wave-per-tile training trios keep their stash (save_x[0..n-1], save_t, gx[1..n], gt) in a private layout: fp16
// stage pieces (the default trio, r2l_f2.h) or the chunked fp32 layout of r2l_common.h (bf16x3 trio); slot n of save_x then
// holds y = x_n + x_0 row-major (all the tail gradient needs) and gx[0] stays row-major (head gradient).
// Every other combination (cooperative fp32 chains, fp32 chains, the pre-embedded module-boundary path) is row-major throughout.
enum { R2L_STASH_ROWMAJOR = 0, R2L_STASH_CHUNKED = 1, R2L_STASH_FP16 = 2 };
// body weight gradients: fp32 MFMA (r2l_dw_body_kernel), bf16x3 on the row-major stash (r2l_dw_body3_kernel), bf16x3 on the
// chunked stash (r2l_dw_body3c_kernel), or the fp16 GEMMs of the default trio with body3c behind them (r2l_dw16.hip)
enum { R2L_DWBODY_FP32 = 0, R2L_DWBODY_BODY3 = 1, R2L_DWBODY_BODY3C = 2, R2L_DWBODY_DW16 = 3 };

struct R2LPlan {
    int64_t N;
    int n_cu;         // CUs of the device (one device type per process; 256 when there is none to ask)
    int reserve_cus;  // CUs kept out of the weight-gradient launches (effective value: 0 .. n_cu / 2)
    // arithmetic of forward-only launches (R2L_NO_FWD3 / R2L_NO_FWD2 alone) and of a training step (all four R2L_NO_* switches)
    int arith_fwd, arith_step;
    int tiling;       // R2L_TILING_WAVE_PER_TILE, _COOP16 or _COOPF — never AUTO
    int coop_tiles;   // COOPF: ray tiles per workgroup, 1 / 2 / 3 (mixed grid); else 0
    int n_two;        // mixed grid: its two-tile workgroups (the grid has tiles - n_two workgroups); else 0
    int xcd_major;    // mixed grid: role order (R2L_MIXED_MAP, r2l_coopf.h fc_mixed_index)
    int fwd;          // R2L_CHAIN_*: the forward launch of this call (with_stash: the step's arithmetic, else the forward-only one)
    int fwd_layout, bwd_layout;  // stream layouts those launches read: 32 / 16 / 3 / 2 (include/r2l_hip.h)
    int stash;        // R2L_STASH_* of a training step
    bool stash_mid;   // fp16 stage pieces with the mid halves (exact weight gradients: dw_mode, else R2L_DW_EXACT=1)
    int chain;        // R2L_CHAIN_*: dX chain
    int dw_body;      // R2L_DWBODY_*
    bool dw_head16;   // head dW on the fp16 matrix pipe (r2l_dw_head16.hip), the fp32 head kernel behind it; else that kernel alone
    bool chain_segments_ok;  // may the dX chain be cut into block segments (the cooperative fp16 chains only)
    // what sizes the weight-gradient grids (r2l_dw_grids below)
    bool dw_overlap;  // step small enough for the head / tail gradients to run beside the body's (and R2L_NO_DW_OVERLAP unset)
    int64_t dw_overlap_max, dw_wgs_env;
};
R2LPlan r2l_plan(const r2l_config* cfg, int64_t N, int n_block, bool with_stash, bool pre_embedded);

// Grids of the weight-gradient kernels of a step, from the plan and the body layers of the call alone (r2l_dispatch.hip)
// (body: persistent workgroups, before the clip to the work list; head: ray slices of 4 workgroups each; rays per slice / workgroup)
struct R2LDwGrids { int64_t body_wgs, head_slices, head_rays, tail_wgs, tail_rays; };
R2LDwGrids r2l_dw_grids(const R2LPlan& p, int n_layers);

// a stream buffer = [32-ray-tile layout | 16-ray-tile layout | bf16x3 stages | fp16x2 stages + 16 status words]; every kernel
// finds its part here.  (The status words live in the caller's buffer, library-private contents: written through.)
struct R2LStreams { float *w32, *w16, *w3, *w2; unsigned* status; };
static inline R2LStreams r2l_streams(const float* w, int64_t n32, int64_t n16, int64_t n3, int64_t status_offset) {
    float* p = const_cast<float*>(w);
    return R2LStreams{p, p + n32, p + n32 + n16, p + n32 + n16 + n3, reinterpret_cast<unsigned*>(p + n32 + n16 + n3 + status_offset)};
}
static inline R2LStreams r2l_fwd_streams(const float* wstream, int n) {
    return r2l_streams(wstream, r2l_fwd32_stream_floats(n), r2l_fwd16_stream_floats(n), r2l_fwd3_stream_floats(n), r2l_fwd2_status_offset(n));
}
static inline R2LStreams r2l_bwd_streams(const float* wstream_bwd, int n) {
    return r2l_streams(wstream_bwd, r2l_bwd32_stream_floats(n), r2l_bwd16_stream_floats(n), r2l_bwd3_stream_floats(n), r2l_bwd2_status_offset(n));
}
