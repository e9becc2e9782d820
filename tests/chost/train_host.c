/* A C99 host that TRAINS: four iterations of the student through r2l_student_train_step alone (include/r2l_hip.h), on buffers read
 * from a file, the final parameters written to another.  Besides the call it needs only memory: what it computes itself per
 * iteration is the arithmetic the header leaves to the host — the pool's key and fill state, the jitter stream, the pack flag.
 * Built and run by tests/test_student_step_gpu.py (-std=c99 -pedantic -Werror), which holds its result to R2LTrainer.fused_step's.
 *
 *   usage: train_host <in> <out>
 *   in:  int64 h[16] = {magic, n_block, rays_per_shard, n_shards, n_draw, store_seed, pool_capacity_rows, n_in, n_out,
 *                       fill_rows (the pool is full once it holds this many), pool_seed, jitter_seed, perturb, 0, 0, 0},
 *        double lr, lw_rgb;  float params[r2l_param_count(n_block)], ztab[32], store[n_shards * rays_per_shard * 9]
 *   out: float params[...], loss[2] */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "r2l_hip.h"

/* the five runtime calls this host makes, declared here: the HIP headers are C++-flavoured, a C99 host needs none of them */
extern int hipMalloc(void** ptr, size_t size);
extern int hipFree(void* ptr);
extern int hipMemcpy(void* dst, const void* src, size_t size, int kind); /* 1: host to device, 2: device to host */
extern int hipMemset(void* dst, int value, size_t size);
extern int hipDeviceSynchronize(void);

#define MAGIC 0x5232534cLL
#define ITERS 4
#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            printf("FAILED line %d: %s (%s)\n", __LINE__, #cond, r2l_last_error());        \
            return 1;                                                                      \
        }                                                                                  \
    } while (0)

static float* dev_floats(int64_t n, const float* init) {
    void* p = NULL;
    int rc;
    if (hipMalloc(&p, (size_t)n * sizeof(float)) != 0) return NULL;
    if (init != NULL) rc = hipMemcpy(p, init, (size_t)n * sizeof(float), 1);
    else rc = hipMemset(p, 0, (size_t)n * sizeof(float));
    return rc == 0 ? (float*)p : NULL;
}

int main(int argc, char** argv) {
    int64_t h[16], n_param, n_store, work_floats = 0, pool_rows = 0, draws = 0, draw = 0;
    double lr_lw[2];
    float *host, *params, *ztab, *store, *pool, *grads, *m, *v, *wf, *wb, *loss, *work = NULL;
    float loss_host[2];
    int it, full = 0;
    FILE* f;
    CHECK(argc == 3);
    f = fopen(argv[1], "rb");
    CHECK(f != NULL);
    CHECK(fread(h, sizeof h, 1, f) == 1 && h[0] == MAGIC);
    CHECK(fread(lr_lw, sizeof lr_lw, 1, f) == 1);
    n_param = r2l_param_count((int)h[1]);
    n_store = h[3] * h[2] * 9;
    host = (float*)malloc((size_t)(n_param + 32 + n_store) * sizeof(float));
    CHECK(host != NULL && fread(host, sizeof(float), (size_t)(n_param + 32 + n_store), f) == (size_t)(n_param + 32 + n_store));
    fclose(f);
    params = dev_floats(n_param, host);
    ztab = dev_floats(32, host + n_param);
    store = dev_floats(n_store, host + n_param + 32);
    pool = dev_floats(h[6] * 9 + 4, NULL);
    grads = dev_floats(n_param, NULL);
    m = dev_floats(n_param, NULL);
    v = dev_floats(n_param, NULL);
    wf = dev_floats(r2l_fwd_stream_floats((int)h[1]), NULL); /* zero-filled once: the status words carry the range history */
    wb = dev_floats(r2l_bwd_stream_floats((int)h[1]), NULL);
    loss = dev_floats(2, NULL);
    CHECK(params && ztab && store && pool && grads && m && v && wf && wb && loss);
    /* the first step finds the streams packed; every later one packs them itself, in front of the step (pack = 1) */
    CHECK(r2l_pack_forward(params, (int)h[1], wf, NULL) == 0);
    CHECK(r2l_pack_backward(params, (int)h[1], wb, NULL) == 0);

    for (it = 1; it <= ITERS; ++it) {
        r2l_student_step_desc d;
        int64_t need;
        memset(&d, 0, sizeof d);
        d.n_block = (int)h[1];
        d.perturb = (int)h[12];
        d.pack = it > 1;
        d.pool_full = full;
        d.cfg = NULL;
        d.rays_per_shard = h[2];
        d.n_shards = h[3];
        d.n_draw = h[4];
        d.draw0 = draw;
        d.store_seed = (uint64_t)h[5];
        d.pool_capacity_rows = h[6];
        d.pool_rows = pool_rows;
        d.n_in = h[7];
        d.n_out = h[8];
        if (full) d.pool_key = (uint64_t)h[10] * 0x9E3779B97F4A7C15ULL + (uint64_t)(draws + 1) * 0xD1B54A32D192ED03ULL;
        d.seed = (uint64_t)h[11];
        d.jitter_stream = ((uint64_t)1 << 61) + 4096u * (uint64_t)it; /* rank 0 */
        d.lw_rgb = lr_lw[1];
        d.lr = (float)lr_lw[0];
        d.beta1 = 0.9f;
        d.beta2 = 0.999f;
        d.eps = 1e-8f;
        d.step = it;
        need = r2l_student_step_work_floats(&d);
        CHECK(need > 0);
        if (need > work_floats) { /* grows once, when the full pool starts to lengthen the batch */
            if (work != NULL) CHECK(hipDeviceSynchronize() == 0 && hipFree(work) == 0);
            work = dev_floats(need, NULL);
            CHECK(work != NULL);
            work_floats = need;
        }
        CHECK(r2l_student_train_step(&d, store, pool, ztab, params, grads, m, v, wf, wb, loss, NULL, work, NULL) == 0);
        draw += h[4];
        if (full) {
            ++draws;
        } else if (h[7] > 0) {
            pool_rows += h[7];
            full = pool_rows >= h[9];
        }
    }
    CHECK(hipDeviceSynchronize() == 0);
    CHECK(hipMemcpy(host, params, (size_t)n_param * sizeof(float), 2) == 0);
    CHECK(hipMemcpy(loss_host, loss, sizeof loss_host, 2) == 0);
    f = fopen(argv[2], "wb");
    CHECK(f != NULL);
    CHECK(fwrite(host, sizeof(float), (size_t)n_param, f) == (size_t)n_param && fwrite(loss_host, sizeof(float), 2, f) == 2);
    fclose(f);
    printf("C99 training host ok: %d iterations, loss %.6f psnr %.4f\n", ITERS, (double)loss_host[0], (double)loss_host[1]);
    return 0;
}
