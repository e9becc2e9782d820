// r2l_teacher_net.h — the NeRF teacher's point network, NeRF(D=8, W=256, 63+27, skips=[4], use_viewdirs), as the four files
// that implement it share it: r2l_teacher_mlp.hip (fp32 MFMA, with and without the training stash), r2l_teacher2.hip (fp16x2),
// r2l_teacher3.hip (bf16x3) and r2l_teacher_train.hip (backward).  What is a property of the network or of the library's
// private formats lives here once: the parameter census, the training stash layout, the stage order of the two 16-bit
// streams, and the host-side declarations between the files.  The arithmetic stays in the .hip files.
#pragma once
#include "r2l_common.h"

// ---- the network ------------------------------------------------------------------------------------------------------
#define T_W 256      // width of the eight body layers and of feature_linear
#define T_XYZ 63     // xyz encoding: 3 + 3 * 2 * 10
#define T_DIR 27     // direction encoding: 3 + 3 * 2 * 4
#define T_VIEWS 128  // width of the views layer

// flat parameter offsets, state_dict order
struct TOff {
    int64_t w[8], b[8], views_w, views_b, feat_w, feat_b, alpha_w, alpha_b, rgb_w, rgb_b, total;
};
__host__ __device__ static inline TOff t_offsets() {
    TOff o;
    int64_t p = 0;
    for (int i = 0; i < 8; ++i) {
        const int fin = i == 0 ? T_XYZ : (i == 5 ? T_W + T_XYZ : T_W);
        o.w[i] = p; p += (int64_t)T_W * fin;
        o.b[i] = p; p += T_W;
    }
    o.views_w = p; p += (int64_t)T_VIEWS * (T_W + T_DIR);
    o.views_b = p; p += T_VIEWS;
    o.feat_w = p; p += (int64_t)T_W * T_W;
    o.feat_b = p; p += T_W;
    o.alpha_w = p; p += T_W;
    o.alpha_b = p; p += 1;
    o.rgb_w = p; p += 3 * T_VIEWS;
    o.rgb_b = p; p += 3;
    o.total = p;
    return o;
}

// ---- training stash ---------------------------------------------------------------------------------------------------
// Written by the forward with stash (r2l_teacher_mlp_train), read by the backward: slot l of [P,256] floats for l = 0..7 holds
// relu(layer l), slot 8 the feature (no ReLU), slot 9 relu(views layer) as [P,128].  ReLU masks follow from the values.
#define T_STASH_FEAT 8
#define T_STASH_VIEWS 9
#define T_STASH_PER_POINT (9 * T_W + T_VIEWS)
// slot l of a stash of P points behind `base`: the stash itself, or a point's row in slot 0 (-> its row in slot l <= 8)
#define T_STASH_SLOT(base, l, P) ((base) + (l) * (P) * T_W)

// ---- stage order of the 16-bit streams (fp16x2, bf16x3) ---------------------------------------------------------------
// A stage is one k-block of 16 input features (8 per half-wave) for all 256 outputs.  Both streams begin with the same 145:
//   L0:   bias, 4 xyz-embedding blocks
//   4 x : t-layer (L1, L3, L5, L7): bias, [L5: 4 xyz-embedding blocks], 16 blocks of relu(x)
//         x-layer (L2, L4, L6, feature): bias, 16 blocks of relu(t)
// and end with their own layout of the views layer.  The kernels consume stages in exactly this order.
// Embedding k order per half-wave h: (sin, cos) pairs (frequency nfreq_half * h + q/3, axis q%3), then the identity (h = 0:
// x, y; h = 1: z, pad), then padding; nfreq_half = 5 (xyz) or 2 (direction).
#define T16_BODY_STAGES 145

// embedding column of value v of half h (or -1 = zero padding)
__host__ __device__ static inline int t16_emb_col(int v, int h, int nfreq_half) {
    const int ntrig = 6 * nfreq_half;
    if (v < ntrig) {
        const int q = v >> 1, fl = q / 3, ax = q % 3;
        return 3 + (nfreq_half * h + fl) * 6 + ((v & 1) ? 3 + ax : ax);
    }
    if (v == ntrig) return h ? 2 : 0;
    if (v == ntrig + 1) return h ? -1 : 1;
    return -1;
}

// Stage g of the common part: kind 0 bias (at offset boff), 1 xyz block (layer 0 or 5), 2 256->256 block (layer 8:
// feature_linear), kb its k-block; kind -1 for g >= T16_BODY_STAGES, where each pack kernel decodes its own views layer
// (kinds 3 feature block, 4 direction block).
struct T16Stage {
    int kind, layer, kb;
    int64_t boff;
};
__device__ __forceinline__ T16Stage t16_body_stage(int g, const TOff& off) {
    int kind = -1, layer = 0, kb = 0;
    int64_t boff = 0;
    if (g == 0) { kind = 0; boff = off.b[0]; }
    else if (g < 5) { kind = 1; layer = 0; kb = g - 1; }
    else if (g < T16_BODY_STAGES) {
        int r = g - 5, k = 0;
        const int psz[4] = {34, 34, 38, 34};
        while (r >= psz[k]) { r -= psz[k]; ++k; }
        const int lt = 1 + 2 * k, lx = 2 + 2 * k;  // lx == 8: feature_linear
        const int tl = (k == 2) ? 21 : 17;        // stages of the t-layer
        if (r < tl) {
            layer = lt;
            if (r == 0) { kind = 0; boff = off.b[lt]; }
            else if (k == 2 && r <= 4) { kind = 1; kb = r - 1; }
            else { kind = 2; kb = r - 1 - (k == 2 ? 4 : 0); }
        } else {
            r -= tl;
            layer = lx;
            if (r == 0) { kind = 0; boff = lx == 8 ? off.feat_b : off.b[lx]; }
            else { kind = 2; kb = r - 1; }
        }
    }
    return T16Stage{kind, layer, kb, boff};
}

// four embedding values v0 .. v0+3 of this half-wave: (sin, cos) pairs of c[axis] * 2^(NF*h + fl), then the identity
template <int NF>
struct T16Emb4 {
    const float (&c)[3];
    int h;
    int v0;
    __device__ __forceinline__ void operator()(float (&out)[4]) const {
        const float base = h ? (float)(1 << NF) : 1.0f;
#pragma unroll
        for (int j = 0; j < 4; j += 2) {
            const int v = v0 + j;
            if (v < 6 * NF) {
                const int q = v >> 1, fl = q / 3, ax = q % 3;
                r2l_sincos(c[ax] * (base * (float)(1 << fl)), out[j], out[j + 1]);
            } else if (v == 6 * NF) {
                out[j] = h ? c[2] : c[0];
                out[j + 1] = h ? 0.f : c[1];
            } else {
                out[j] = 0.f;
                out[j + 1] = 0.f;
            }
        }
    }
};

struct T16Args {
    const float* rays_o;
    const float* rays_d;
    const float* viewdirs;
    const float* z;
    const unsigned char* stream;
    union {                      // the guard word, by the name its kernel knows it under
        unsigned* status;        // r2l_teacher2_kernel: range-guard word behind the stream: != 0 -> the launch is left to bf16x3
        const unsigned* run_if;  // r2l_teacher3_kernel: nullptr, or: return at once while this word is 0 (teacher2's fallback)
    };
    const float* params;
    float* raw;
    int64_t n_pts;
    int S;
    const int64_t* idx;        // live form only (below): the sample of every tile lane, capacity n_pts
    const int64_t* count_dev;  // live form only: how many entries of idx count (device, 1)
    int64_t n_out;             // live form only: the entries of idx name samples in [0, n_out) (R*S; n_pts unless the list is shorter)
};

// ---- live form of the three forward kernels (r2l_teacher_mlp_live_cfg, include/r2l_hip.h) ------------------------------------
// The launch is sized for the capacity n_pts of the index list (R*S behind r2l_teacher_mlp_live_cfg; r2l_teacher_mlp_live_into_cfg
// names a shorter one, and then n_out = R*S bounds the sample numbers); tile lane i < count = min(*count_dev, n_pts) takes sample n = idx[i] where the
// plain form takes sample i, and stores at raw + 4 n.  LIVE is a template parameter of each kernel: the plain instantiations
// compile from the code they always had.  A point is a column of its tile, so raw[n] has the bits the plain form writes at n.
// The fp32 chain's training form (STASH) has a live instantiation too, in a kernel of its own (r2l_teacher_mlp_train_live_kernel): its
// stash is compact, tile lane i writes row i of a slot.
// The count is an ordinary load of one address by every lane (the compiler may make it a scalar load).
__device__ __forceinline__ int64_t t_live_count(const int64_t* __restrict__ count_dev, int64_t cap) {
    const int64_t c = *count_dev;
    return c < cap ? c : cap;
}
// A workgroup (4 tiles of R2L_TILE_RAYS lanes) with no lane below the count leaves as a whole, before any LDS staging or barrier;
// count <= 0 empties every workgroup, so the clamp below never sees row -1.
__device__ __forceinline__ bool t_live_workgroup_idle(int64_t count) {
    return (int64_t)blockIdx.x * (4 * R2L_TILE_RAYS) >= count;
}
// Sample of tile lane i (count >= 1).  A lane at or past the count reads row count - 1 and stores nothing, as the plain form
// clamps to its last point; an entry outside [0, cap) — cap = n_out, the samples of raw — reads sample 0 in its place and stores nothing.
__device__ __forceinline__ int64_t t_live_sample(const int64_t* __restrict__ idx, int64_t count, int64_t cap, int64_t i, bool& valid) {
    const bool below = i < count;
    const int64_t n = idx[below ? i : count - 1];
    const bool in = n >= 0 && n < cap;
    valid = below && in;
    return in ? n : 0;
}

// ---- host side --------------------------------------------------------------------------------------------------------
// workgroups (4 waves of R2L_TILE_RAYS points) of a forward launch over n_pts points
static inline unsigned t_workgroups(int64_t n_pts) {
    const int64_t tiles = (n_pts + R2L_TILE_RAYS - 1) / R2L_TILE_RAYS;
    return (unsigned)((tiles + 3) / 4);
}
// r2l_teacher3.hip: the same network on the bf16 matrix pipe (fp32-accurate); its stage stream follows the fp32 one
int64_t r2l_teacher3_stream_floats(void);
int r2l_teacher3_pack(const float* tparams, float* wstream3, hipStream_t stream);
int r2l_teacher3_mlp(const float* rays_o, const float* rays_d, const float* viewdirs, const float* z,
                     const float* wstream3, const float* tparams, float* raw, int64_t n_pts, int S, hipStream_t stream,
                     const unsigned* run_if, const int64_t* idx = nullptr, const int64_t* count_dev = nullptr, int64_t n_out = 0);
// r2l_teacher2.hip: three fp16 products per fp32 product (default), range-guarded; its stream follows the bf16x3 one
int64_t r2l_teacher2_stream_floats(void);
const unsigned* r2l_teacher2_status(const float* wstream2);
int r2l_teacher2_pack(const float* tparams, float* wstream2, hipStream_t stream);
int r2l_teacher2_mlp(const float* rays_o, const float* rays_d, const float* viewdirs, const float* z,
                     const float* wstream2, const float* tparams, float* raw, int64_t n_pts, int S, hipStream_t stream,
                     const int64_t* idx = nullptr, const int64_t* count_dev = nullptr, int64_t n_out = 0);
// (idx / count_dev: NULL pair = the plain form; else the live form over the capacity n_pts, sample numbers below n_out — 0: n_pts)
