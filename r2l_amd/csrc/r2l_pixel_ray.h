// World ray of one pixel: the ONE definition behind r2l_frame_rays, r2l_pixel_batch (r2l_teacher_frame.hip), the compact ray
// store's batch (r2l_cstore.hip), which recomputes the o, d that r2l_frame_rays wrote and must give the same bits, and the pose
// mode of the student's forward chains (r2l_student_net.h r2l_ray_of_pixel).  Every file that includes this is built with
// -ffp-contract=off; the store, pose and frame kernels also with -fno-slp-vectorize (r2l_amd/build.py FILE_FLAGS), the student's
// chain files with the SLP vectoriser on — which is why the two products below are kept apart by hand.  The rounding order is part
// of the interface.
#pragma once

// World ray of pixel (row, col) of an H x W frame with pose c ([3][4]) and focal f: separately rounded fp32 in the order of
// include/r2l_hip.h (the build passes -ffp-contract=off).
__device__ __forceinline__ void pixel_ray(const float* __restrict__ c, float f, int H, int W, int row, int col, float (&o)[3],
                                          float (&d)[3]) {
    const float dx = ((float)col - (float)W * .5f) / f, dy = -(((float)row - (float)H * .5f) / f), dz = -1.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float dxc = dx * c[i * 4 + 0];
        // no packed multiply + swizzled add for the pair of products (r2l_common.h r2l_no_pack): an empty asm, changes no value
        asm volatile("" : "+v"(dxc));
        d[i] = (dxc + dy * c[i * 4 + 1]) + dz * c[i * 4 + 2];
        o[i] = c[i * 4 + 3];
    }
}
