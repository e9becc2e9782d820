// r2l_bwd32.hip — the dX chain of the student's backward on the fp32 MFMA (the exact-fp32 family; its siblings: r2l_coop16.hip,
// r2l_bwd3.hip, r2l_bwd2.hip, r2l_coopf_bwd.hip): dL/drgb -> sigmoid' -> tail^T -> the 2*n_block transposed layers,
// register-resident exactly like the forward (W^T streams packed by r2l_pack_backward); writes the per-layer output gradients G
// (row-major [N,256]) that the weight-gradient GEMMs need.
#include "r2l_dw.h"

struct R2LBwdArgs {
    const float* rgb;      // [N,3] forward output
    const float* target;   // [N,3]  MSE mode: dL/drgb = grad_scale*(rgb-target)            (or nullptr)
    const float* drgb;     // [N,3]  generic mode (target == nullptr): dL/drgb given by the caller
    const float* save_x;   // [(n_block+1),N,256]
    const float* save_t;   // [n_block,N,256]
    const float* wstream;  // packed transposed weight stream
    const float* params;   // flat params (tail weights)
    int n_block;
    float grad_scale;      // dL/drgb = grad_scale * (rgb - target);  = 2*lw_rgb / (3*N_global)
    float* dpre;           // [N,3]   dL/d(tail pre-activation)
    float* gx;             // [(n_block+1),N,256]  gx[b] = dL/dx_b ; gx[0] already includes the outer-residual branch and
                           //                      is masked by relu'(head) i.e. it is dL/d(head pre-activation)
    float* gt;             // [n_block,N,256]      dL/d(hidden pre-activation) of each block
    float* sqerr_partial;  // [ceil(N/32)] per-tile sums of (rgb-target)^2
    int64_t N;
};

// relu'(t) as 128 bits per lane: bit R2L_MASK32_BIT(T, c) of word T >> 1 belongs to fragment register (T, c) (r2l_common.h: the
// forward's mask words)
struct MaskAct {
    unsigned mb[4];
    __device__ __forceinline__ float operator()(float v, int T, int c) const {
        return ((mb[T >> 1] >> R2L_MASK32_BIT(T, c)) & 1u) ? v : 0.f;
    }
};

// GEMM A of the backward chain (u = W2^T g): g = dL/dx_{b+1} is the B operand, its store to gx[b+1] rides along (StoreHook).
// The ReLU mask of the block's hidden activation comes from the forward's mask words (r2l_common.h r2l_mask32_offset): one
// 16-byte load per lane, issued in front of the GEMM and first used behind it.  (Rounds 1 - 5 prefetched relu(t) itself, one
// 16-byte piece per group, and folded its signs: 32 loads per lane and block, all of save_t read a second time.)

__global__ __launch_bounds__(256, 1) void r2l_bwd_chain_kernel(const R2LBwdArgs a) {
    __shared__ float stash[4][R2L_NT * 16][64];  // dy of each wave's tile (outer residual branch), re-added at the head

    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int h = lane >> 5;
    const int64_t tile = (int64_t)blockIdx.x * 4 + wave;
    if (tile * R2L_TILE_RAYS >= a.N) return;
    const int64_t ray = tile * R2L_TILE_RAYS + (lane & 31);
    const bool valid = ray < a.N;
    const int64_t rc = valid ? ray : a.N - 1;

    WRing2 ws;  // 64 groups per block: ring slots are static (r2l_common.h)
    ws.init(a.wstream, lane);
    const int64_t Np = R2L_PAD_ROWS(a.N);  // rows per stash / gradient slot

    // loss gradient through the sigmoid: dpre = grad_scale*(rgb-target) * rgb*(1-rgb); per-tile squared error
    float dp[3];
    const float se = r2l_loss_seed(a.rgb, a.target, a.drgb, a.grad_scale, rc, valid, dp);
    if (valid && h == 0) r2l_dpre_store(a.dpre, ray, dp);
    r2l_tile_sqerr(a.sqerr_partial, tile, se, h, lane);

    // g = dy = Wt^T dpre   (tail Linear(256,3))
    f32x16 g[R2L_NT], u[R2L_NT];
    r2l_tail_transposed<false>(g, a.params + r2l_off_tail_w(a.n_block) + 4 * h, dp, 1.0f);
#pragma unroll
    for (int T = 0; T < R2L_NT; ++T)
#pragma unroll
        for (int c = 0; c < 16; ++c) stash[wave][T * 16 + c][lane] = g[T][c];
#pragma unroll 1
    for (int b = a.n_block - 1; b >= 0; --b) {
        // u = W2^T g (accumulators initialised by the first group, C = 0); g (= dL/dx_{b+1}) is stored to gx[b+1] along the way;
        // the ReLU mask words of the block's hidden activation are requested in front of it
        const u32x4 mw = *reinterpret_cast<const u32x4*>(a.save_t + r2l_mask32_offset(a.n_block, Np, b) + tile * 256 + lane * 4);
        {
            StoreHook hk(a.gx + (int64_t)(b + 1) * Np * R2L_W, ray, h, g);
            gemm256a<IdentityAct, 0, true>(u, g, ws, hk, IdentityAct());
        }
        const unsigned mb[4] = {mw[0], mw[1], mw[2], mw[3]};
        // g += W1^T (u . mask): the mask relu'(hidden) = (t_b > 0) is applied lazily to the B operands of each group and
        // to the pieces of u (= dL/d hidden pre-activation) stored to gt[b] along the way
        {
            const MaskAct mask{{mb[0], mb[1], mb[2], mb[3]}};
            StoreHookT<false, MaskAct> su(a.gt + (int64_t)b * Np * R2L_W, ray, h, u, mask);
            gemm256a<MaskAct, 0>(g, u, ws, su, mask);
        }
    }

    // head: dL/d(head pre-activation) = (g + dy) * (x_0 > 0)
    {
        const float* r = a.save_x + ray * R2L_W + 4 * h;
#pragma unroll
        for (int T = 0; T < R2L_NT; ++T)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 xv = *reinterpret_cast<const f32x4*>(r + 32 * T + 8 * q);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float v = g[T][4 * q + j] + stash[wave][T * 16 + 4 * q + j][lane];
                    g[T][4 * q + j] = xv[j] > 0.f ? v : 0.f;
                }
            }
    }
    store_frag(a.gx, ray, h, g);
}

int r2l_bwd32_backward(const R2LLossIO& loss, const float* save_x, const float* save_t, const float* wstream_bwd32,
                       const float* params, int n_block, float* gx, float* gt, int64_t N, hipStream_t stream) {
    R2LBwdArgs a{};
    r2l_set_loss(a, loss);
    a.save_x = save_x; a.save_t = save_t; a.wstream = wstream_bwd32;
    a.params = params; a.n_block = n_block; a.gx = gx; a.gt = gt; a.N = N;
    const int64_t tiles = (N + R2L_TILE_RAYS - 1) / R2L_TILE_RAYS;
    hipLaunchKernelGGL(r2l_bwd_chain_kernel, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, stream, a);
    R2L_CHECK(hipGetLastError());
    return 0;
}
