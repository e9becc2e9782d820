// r2l_dispatch.hip — the launch plan (r2l_dispatch.h): the table of environment switches, the rule that resolves a plan, and
// the grids of the weight-gradient kernels.  Host code only: this file contains no kernel.
#include "r2l_dispatch.h"
#include "r2l_dw.h"
#include <string.h>

// ---- the environment switches of the library (R2L_RCCL_PATH, r2l_allreduce.hip, is not dispatch) ------------------------------
struct R2LEnv {
    int tiling;        // R2L_FORCE_VARIANT=main|coop|coop16|coopf as R2L_TILING_*, or R2L_TILING_AUTO
    bool named_coop;   // ... it said "coop"
    bool no_fwd3, no_fwd2, no_bwd2, no_dw2, dw_exact;  // R2L_NO_FWD3 / R2L_NO_FWD2 / R2L_NO_BWD2 / R2L_NO_DW2 / R2L_DW_EXACT = 1
    int coopf_tiles, reserve_cus;                      // R2L_COOPF_TILES=1|2|3, R2L_RESERVE_CUS=n; else 0
    int64_t dw_wgs;    // R2L_DW_WGS=n: workgroups of the body weight-gradient kernel (tuning knob, tools/small_prof.sh), else 0
    int mixed_map;     // R2L_MIXED_MAP=1: XCD-major role order of the mixed coopf grid (A/B knob), else 0 = by blockIdx
    int64_t dw_overlap_max;  // R2L_DW_OVERLAP_MAX_RAYS (tuning knob, tools/run_ab.sh), else R2L_COOPF_MAX_RAYS: read once per process,
    bool no_dw_overlap;      // as is R2L_NO_DW_OVERLAP=1
};
// the switches read per call, found in ONE walk over the environment (a getenv per switch is a walk each: measurable on the
// 0.8 ms steps, whose host side is on the critical path)
enum { E_FORCE_VARIANT, E_NO_FWD3, E_NO_FWD2, E_NO_BWD2, E_NO_DW2, E_DW_EXACT, E_COOPF_TILES, E_RESERVE_CUS, E_DW_WGS, E_MIXED_MAP, E_N };
static const char* const r2l_switch_names[E_N] = {"R2L_FORCE_VARIANT", "R2L_NO_FWD3", "R2L_NO_FWD2", "R2L_NO_BWD2", "R2L_NO_DW2",
                                                   "R2L_DW_EXACT", "R2L_COOPF_TILES", "R2L_RESERVE_CUS", "R2L_DW_WGS", "R2L_MIXED_MAP"};
extern char** environ;
static bool env_on(const char* e) { return e && e[0] && e[0] != '0'; }
static R2LEnv r2l_env_read() {
    const char* val[E_N] = {};  // as getenv: the first entry of a name, or nullptr
    for (char** entry = environ; entry && *entry; ++entry) {
        const char* s = *entry;
        for (int i = 0; i < E_N && s[0] == 'R' && s[1] == '2' && s[2] == 'L' && s[3] == '_'; ++i) {
            const size_t n = strlen(r2l_switch_names[i]);
            if (val[i] == nullptr && strncmp(s, r2l_switch_names[i], n) == 0 && s[n] == '=') val[i] = s + n + 1;
        }
    }
    R2LEnv v{};  // (tiling: R2L_TILING_AUTO)
    if (const char* e = val[E_FORCE_VARIANT]; e && e[0]) {
        if (e[0] == 'm') v.tiling = R2L_TILING_WAVE_PER_TILE;
        else if (e[0] == 'c' && e[1] && e[2] && e[3] && e[4] == 'f') v.tiling = R2L_TILING_COOPF;
        else if (e[0] == 'c') {  // coop16; "coop" named the retired 32-ray family: its launches are coop16's now
            v.tiling = R2L_TILING_COOP16;
            v.named_coop = e[1] && e[2] && e[3] && !e[4];
        } else v.tiling = R2L_TILING_WAVE_PER_TILE;  // (anything else used to mean "not the cooperative fp16 kernels")
    }
    v.no_fwd3 = env_on(val[E_NO_FWD3]);
    v.no_fwd2 = env_on(val[E_NO_FWD2]);
    v.no_bwd2 = env_on(val[E_NO_BWD2]);
    v.no_dw2 = env_on(val[E_NO_DW2]);
    v.dw_exact = env_on(val[E_DW_EXACT]);
    if (const char* e = val[E_COOPF_TILES]; e && e[0] >= '1' && e[0] <= '3') v.coopf_tiles = e[0] - '0';
    if (val[E_RESERVE_CUS]) v.reserve_cus = atoi(val[E_RESERVE_CUS]);
    if (val[E_DW_WGS]) v.dw_wgs = atoll(val[E_DW_WGS]);
    if (val[E_MIXED_MAP]) v.mixed_map = val[E_MIXED_MAP][0] == '1' ? 1 : 0;
    static const char* const max_rays = getenv("R2L_DW_OVERLAP_MAX_RAYS");  // these two: read once per process
    static const int64_t overlap_max = max_rays ? (int64_t)atoll(max_rays) : (int64_t)R2L_COOPF_MAX_RAYS;
    static const bool overlap_off = env_on(getenv("R2L_NO_DW_OVERLAP"));
    v.dw_overlap_max = overlap_max, v.no_dw_overlap = overlap_off;
    return v;
}

static int r2l_n_cu() {
    static int n_cu = 0;  // one device type per process
    int dev = 0, v = 0;
    if (n_cu == 0) n_cu = (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ? v : 256;
    return n_cu;
}

// Which chain variant is fastest for N rays.  In units of one main-kernel round (1024 wave slots x 32 rays): main needs
// ceil(N/32768) rounds; coop (4 waves share a 32-ray tile, 256 workgroups) ceil(N/8192) rounds of ~0.34 (measured: fwd
// 0.81 ms at 4096 rays, 0.94 ms at 8192); coop16 (4 waves share a 16-ray tile: fills all 256 CUs from 4096 rays)
// ceil(N/4096) rounds of ~0.174 (0.47 ms at 4096 rays, 0.91 ms at 8192).
// R2L_FORCE_VARIANT=main|coop|coop16 in the environment overrides (tests, A/B).
#ifndef R2L_C16_ROUND
#define R2L_C16_ROUND 0.174
#endif
// Cooperative fp16x2 kernels (r2l_coopf.h: one 32-ray tile per WORKGROUP): a sub-family of the MAIN variant — same streams,
// stash and fallbacks as r2l_fwd2 / r2l_bwd2, taken instead of them for launches of at most R2L_COOPF_MAX_RAYS rays, and
// for launches between one and one and a half ROUNDS of the one-wave-per-tile kernels (a round = 256 CUs x 128 rays): the
// two-tile cooperative kernels then run three full rounds of 16 384 rays where those run two, the second half empty
// (measured, tools/variant_sweep.py, 49 152 rays: step 4.19 vs 4.51 ms, forward 1.44 vs 1.53 ms; 24 576: 2.55 vs 2.44,
// 65 536: 5.53 vs 5.29, 98 304: 8.20 vs 7.81 — the one-wave-per-tile kernels everywhere else)
// (R2L_FORCE_VARIANT=coopf: always; =main: never).  Only with the whole fp16 trio enabled (no R2L_NO_* switch).
#define R2L_MAIN_ROUND_RAYS 32768  // one wave per 32-ray tile, four per workgroup, one workgroup per CU, 256 CUs

R2LPlan r2l_plan(const r2l_config* cfg, int64_t N, int n_block, bool with_stash, bool pre_embedded) {
    const r2l_config c = cfg ? *cfg : r2l_config{};
    const R2LEnv env = r2l_env_read();
    R2LPlan p{};
    p.N = N, p.n_cu = r2l_n_cu();
    // Data-parallel hosts overlap the gradient all-reduce with the weight-gradient stages (r2l_backward_part).  Those kernels
    // are persistent workgroups that take every register of their CU, so a collective launched beside them would wait for
    // a whole stage to finish: R2L_RESERVE_CUS=n (set by the host when world_size > 1; r2l_amd/train_step.py uses 8) keeps n
    // CUs out of the weight-gradient launches for the RCCL kernels.  Default 0.
    p.reserve_cus = c.reserve_cus ? c.reserve_cus : env.reserve_cus;  // (-1: none)
    if (p.reserve_cus < 0 || p.reserve_cus > p.n_cu / 2) p.reserve_cus = 0;
    // ---- arithmetic.  Forward launches big enough for the one-wave-per-tile kernels take the bf16x3 kernel (R2L_NO_FWD3=1: fp32
    // MFMA), by default behind the fp16x2 one: three fp16 products per fp32 product, ~2^-21 relative (r2l_fwd2.hip), the bf16x3
    // kernel as its range-guard fallback (R2L_NO_FWD2=1: bf16x3 only).  The default TRAINING trio of one-wave-per-tile MSE-mode
    // steps: fp16x2 forward and dX chain (r2l_bwd2.hip) stashing fp16 stage pieces, and the fp16 weight-gradient GEMMs on them
    // (r2l_dw16.hip).  Any of R2L_NO_FWD3 / R2L_NO_FWD2 / R2L_NO_BWD2 / R2L_NO_DW2 = 1 puts the whole step on the bf16x3 trio
    // (r2l_fwd3 / r2l_bwd3 / r2l_dw_body3c, chunked fp32 stash) — the kernels the range guards fall back to.
    const bool use3 = c.precision ? c.precision != R2L_PRECISION_FP32_MFMA : !env.no_fwd3;
    const bool use2 = c.precision ? c.precision == R2L_PRECISION_FP16X2 : use3 && !env.no_fwd2;
    const bool trio16 = c.precision ? c.precision == R2L_PRECISION_FP16X2 : use2 && !env.no_bwd2 && !env.no_dw2;
    p.arith_fwd = use2 ? R2L_ARITH_FP16X2 : (use3 ? R2L_ARITH_BF16X3 : R2L_ARITH_FP32);
    p.arith_step = trio16 ? R2L_ARITH_FP16X2 : (use3 ? R2L_ARITH_BF16X3 : R2L_ARITH_FP32);
    // ---- tiling: cfg->tiling, else R2L_FORCE_VARIANT, else by size
    const int forced = c.tiling ? c.tiling : env.tiling;
    if (!c.tiling && env.named_coop) {  // said once per process, not silently
        static bool warned = false;
        if (!warned) {
            warned = true;
            fprintf(stderr, "libr2l_hip: R2L_FORCE_VARIANT=coop names the kernel family retired in round 5; taking coop16\n");
        }
    }
    bool coop16 = forced == R2L_TILING_COOP16;
    if (forced == R2L_TILING_AUTO && !(trio16 && N <= R2L_COOPF_MAX_RAYS)) {  // (those: served by the cooperative fp16x2 kernels)
        // (one main round on the fp16x2 kernels costs 0.30 of a round of the fp32-MFMA kernel the unit was defined on; measured,
        // tools/variant_sweep.py: 98 304-ray-style steps of 6144 rays 1.99 ms on the one-wave-per-tile kernels vs 2.11 ms on the
        // 16-ray cooperative ones, 20 480 rays 2.9 vs 5.9 ms; 4096 rays 1.94 vs 1.34 ms)
        // (round 5: the 32-ray fp32-MFMA cooperative family — 0.34 per round of 8192 rays — is retired: AUTO reached it only under a
        // pinned fp32_mfma precision, in the bands where it beat two 16-ray rounds by 2 %: profiles/r05_dispatch_table.md)
        const double main_t = (double)((N + 32767) / 32768) * (use3 ? 0.30 : 1.0);
        const double c16_t = (double)((N + 4095) / 4096) * R2L_C16_ROUND;
        coop16 = c16_t < main_t;
    }
    const bool coopf = n_block > 0 && trio16 &&
                       (forced == R2L_TILING_COOPF ||
                        (forced == R2L_TILING_AUTO &&
                         (N <= R2L_COOPF_MAX_RAYS || (N > R2L_MAIN_ROUND_RAYS && N <= R2L_MAIN_ROUND_RAYS + R2L_MAIN_ROUND_RAYS / 2))));
    p.tiling = coop16 ? R2L_TILING_COOP16 : (coopf ? R2L_TILING_COOPF : R2L_TILING_WAVE_PER_TILE);
    if (coopf) {
        // ray tiles per workgroup: 1 while that keeps the launch within one workgroup per CU, else 2; the MIXED grid (3) is
        // opt-in (r2l_coopf.h): outside its band 1 below, 2 above
        const int64_t tiles = (N + R2L_TILE_RAYS - 1) / R2L_TILE_RAYS;
        const int want = c.coop_tiles ? c.coop_tiles : env.coopf_tiles;
        if (want == 1 || want == 2) p.coop_tiles = want;
        else if (tiles <= p.n_cu) p.coop_tiles = 1;
        else if (tiles >= 2 * (int64_t)p.n_cu) p.coop_tiles = 2;
#ifndef FC_MIXED_AUTO  // (A/B builds with -DFC_MIXED_AUTO: AUTO takes the mixed grid in its band)
        else if (want == 0) p.coop_tiles = 2;
#endif
        else p.coop_tiles = 3;
        if (p.coop_tiles == 3) {
            p.n_two = (int)(tiles - p.n_cu);
            p.xcd_major = env.mixed_map;
        }
    }

    // ---- kernels
    const bool fwd16 = with_stash ? trio16 : use2;  // (with the training stash: only as part of the default fp16 trio, whose stash format it writes)
    p.fwd = coop16 ? R2L_CHAIN_COOP16 : (fwd16 ? R2L_CHAIN_FP16 : (use3 ? R2L_CHAIN_BF16X3 : R2L_CHAIN_FP32));
    p.fwd_layout = coop16 ? 16 : (fwd16 ? 2 : (use3 ? 3 : 32));
    p.bwd_layout = coop16 ? 16 : (use3 ? (trio16 ? 2 : 3) : 32);
    if (pre_embedded) {
        // module-boundary path (r2l_forward_emb_cfg): the fp32-MFMA kernel reads the caller's encoding; a config that names a
        // 16-bit precision gets the bf16x3 chain behind an fp32-MFMA head (no range-guard fallback here).  The environment is not asked.
        p.fwd = (c.precision == R2L_PRECISION_BF16X3 || c.precision == R2L_PRECISION_FP16X2) ? R2L_CHAIN_BF16X3 : R2L_CHAIN_FP32;
    }
    const bool split = !pre_embedded && N > 0 && !coop16 && use3;
    p.stash = !split ? R2L_STASH_ROWMAJOR : (trio16 ? R2L_STASH_FP16 : R2L_STASH_CHUNKED);
    p.stash_mid = p.stash == R2L_STASH_FP16 && (c.dw_mode ? c.dw_mode == R2L_DW_EXACT : env.dw_exact);
    p.chain = coop16 ? R2L_CHAIN_COOP16 : (!split ? R2L_CHAIN_FP32 : (trio16 ? R2L_CHAIN_FP16 : R2L_CHAIN_BF16X3));
    p.dw_body = split ? (trio16 ? R2L_DWBODY_DW16 : R2L_DWBODY_BODY3C) : (use3 ? R2L_DWBODY_BODY3 : R2L_DWBODY_FP32);
    p.dw_head16 = p.stash == R2L_STASH_FP16;
    p.chain_segments_ok = N > 0 && !coop16 && use3 && trio16 && coopf;
    p.dw_overlap = !env.no_dw_overlap && N <= env.dw_overlap_max;
    p.dw_overlap_max = env.dw_overlap_max, p.dw_wgs_env = env.dw_wgs;
    return p;
}

// ---- grids of the weight-gradient kernels ---------------------------------------------------------------------------------------
R2LDwGrids r2l_dw_grids(const R2LPlan& p, int n_layers) {
    R2LDwGrids g{};
    const int n_cu = p.n_cu - p.reserve_cus;
    const bool trio16 = p.dw_body == R2L_DWBODY_DW16;
    const int64_t N = p.N;
    int64_t wgs = n_cu < DW_MAX_WGS ? n_cu : DW_MAX_WGS;
    // small steps: two workgroups per layer, none across a layer boundary (one slab flush each, half the reduce): measured
    // at 4096 rays 97 + 16 us against 111 + 22 us for 251 workgroups; at 12 288 rays the full grid wins again (229 + 22
    // against 242 + 16)
    // (that is the fp16 trio's kernel, which is bound by the slab traffic at this size; the fp32-MFMA / bf16x3 kernels are bound by
    // their MFMAs — 32 units on 172 workgroups against 22 on 251 — and keep the full grid: round 6, profiles/r06_graded_step_ab.txt E)
    if (trio16 && N <= 6144 && 2 * (int64_t)n_layers <= wgs) wgs = 2 * (int64_t)n_layers;
    // above that, up to the largest step whose head / tail gradients run beside this kernel: 11/16 of the CUs.  On the full grid the
    // head kernel (VALU-bound, 4 workgroups per ray slice) queues behind the persistent workgroups and the overlap is one in name
    // only (12 288 rays: 1.251 ms with 251 workgroups = 1.285 with the overlap off; 1.231 with 176, 1.239 with 144: round 6,
    // profiles/r06_small_step_dw_grid.txt); the kernel is HBM-bound, fewer workgroups cost it little
    if (trio16 && N > 6144 && N <= p.dw_overlap_max && wgs > n_cu * 11 / 16) wgs = n_cu * 11 / 16;
    // the MFMA-bound kernels with the head / tail gradients beside them (small steps): an eighth of the CUs stays free for those,
    // or they queue behind the persistent grid (4096 rays, fp32 family: 1.358 ms with 172 workgroups, 1.367 with 251, 1.317 with 224)
    // (decided by the step size alone, not by whether THIS call overlaps: the staged form — body buckets in calls of their own —
    // must cut the same work list as the one-call form, tests: staged with one bucket == one call, bit for bit)
    if (!trio16 && N <= p.dw_overlap_max && wgs > n_cu - n_cu / 8) wgs = n_cu - n_cu / 8;
    if (p.dw_wgs_env >= n_layers && p.dw_wgs_env <= wgs) wgs = p.dw_wgs_env;
    g.body_wgs = wgs;
    int64_t slices = n_cu / 4;  // head
    if (slices > DW_HEAD_SLAB_MAX / (R2L_W * 1024)) slices = DW_HEAD_SLAB_MAX / (R2L_W * 1024);  // (what the slab region holds)
    // small launches: >= 256 rays per slice (each slice costs a 1 MB partial).  (Round 5 tried 128 and 64 rays per slice for the
    // 4096-ray step — 32 / 64 slices instead of 16: 0.789 / 0.823 ms per step against 0.789, same box: what the wider grid gains
    // the 1 MB-per-slice reduce gives back; profiles/r05_small_step_ab.txt)
    if (slices > (N + 255) / 256) slices = (N + 255) / 256;
    if (slices < 1) slices = 1;
    int64_t per = (N + slices - 1) / slices;
    per = (per + 1) & ~(int64_t)1;  // even: a k-step pairs rays 2s, 2s+1
    if (per < 2) per = 2;
    g.head_slices = (N + per - 1) / per;
    g.head_rays = per;
    wgs = 2 * n_cu;  // tail
    if (wgs > DW_TAIL_SLAB / (4 * R2L_W)) wgs = DW_TAIL_SLAB / (4 * R2L_W);  // (what the slab region holds: no switch of paths,
    per = (N + wgs - 1) / wgs;                                              //  i.e. of summation order, on a larger device)
    if (per < 1) per = 1;
    g.tail_wgs = (N + per - 1) / per;
    g.tail_rays = per;
    return g;
}
