"""Times of ray culling (--r2l_ray_cull) on one GPU -> profiles/ray_cull.txt.

The protocol of profiles/occupancy_fused.txt: one process, three alternated rounds, device events, median and spread.  The scene is
the tests' trained-like pair (tests/teacher_util.py: an analytic shell at r = 1 and a blob), the student a W256 D88 network with
random weights (its time does not depend on them), the frames 400 x 400 at the lego focal, 9 poses a launch group on the r = 4 sphere.

    python tools/ray_cull_time.py [--out profiles/ray_cull.txt] [--poses 100]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import r2l_oracle as O  # noqa: E402
from r2l_amd import engine, occupancy as OC, ray_cull as RC  # noqa: E402
from r2l_amd.raystore import RayStore  # noqa: E402

DEV = torch.device("cuda:0")
H = W = 400
FOCAL = 555.5555155968841
NEAR, FAR = 2., 6.
K = 9


def poses(n, first=0):
    return torch.stack([torch.from_numpy(O.pose_spherical(-170. + 47. * (first + k), -15. - 20. * ((first + k) % 3), 4.)[:3, :4])
                        for k in range(n)], 0).float()


def timed(fns, rounds=3, reps=5):
    """{name: (median ms, spread)} of alternated rounds; every fn is warmed once."""
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / reps)
    return {k: (float(np.median(v)), float(max(v) - min(v))) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_cull.txt"))
    ap.add_argument("--poses", type=int, default=100)
    a = ap.parse_args()
    from r2l_amd.nerf_raybased import NeRF, PointSampler
    from r2l_amd.render import render_frames
    from tests.pose_refine_util import make_model
    from tests.teacher_util import trained_like_pair
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    nets = []
    for sd in trained_like_pair():
        m = NeRF(D=8, W=256, input_ch=63, output_ch=4, skips=[4], input_ch_views=27, use_viewdirs=True)
        m.load_state_dict(sd)
        nets.append(m.to(DEV).eval())
    student = make_model(n_block=43, device=DEV, state=O.make_state_dict(n_block=43, seed=0)).eval()
    ps = PointSampler(H, W, FOCAL, 16, NEAR, FAR, device=DEV)
    c2ws = poses(K)
    say("ray culling, %s, %d x %d frames, focal %.1f, near %g, far %g, %d poses a launch group; one process, three alternated rounds, "
        "device events, median (spread)" % (torch.cuda.get_device_name(0), H, W, FOCAL, NEAR, FAR, K))
    grids = {}
    for bound in (2.5, 6.0):
        g = OC.OccupancyGrid([-bound] * 3, [bound] * 3, G=128, k=2, dilate=1).build(nets[1])
        grids[bound] = RC.RayCull(g, NEAR, FAR, True)
        say("grid 128^3 x 2 x 1 over +-%g of the fine net: built in %.2f s, %.1f %% of the cells occupied, T = %d" %
            (bound, g.build_seconds, 100. * g.occupied_share(), grids[bound].steps(H, W, FOCAL)))
    words = OC.n_words(4)
    empty = RC.RayCull(OC.OccupancyGrid([-16.] * 3, [16.] * 3, G=4, k=1, dilate=1).set_bits(np.zeros(words, np.uint32), device=DEV), NEAR, FAR, True)
    full = RC.RayCull(OC.OccupancyGrid([-2.5] * 3, [2.5] * 3, G=128, k=2, dilate=1).set_bits(
        np.full(OC.n_words(128), 0xFFFFFFFF, np.uint32), device=DEV), NEAR, FAR, True)

    say("")
    say("student test loop, ms per frame without images (W256 D88):")
    for fam in ("default", "fp32_mfma"):
        engine.DEFAULT_CONFIG = {} if fam == "default" else {"precision": fam}
        with torch.no_grad():
            fns = {"off": lambda: student.render_poses(c2ws, ps)}
            for name, c in (("+-2.5", grids[2.5]), ("+-6", grids[6.0]), ("empty grid, inside rays", empty), ("full grid", full)):
                fns[name] = (lambda c=c: c.render_poses(student, c2ws, ps))
            res = timed(fns)
        for name, c in (("+-2.5", grids[2.5]), ("+-6", grids[6.0]), ("empty grid, inside rays", empty), ("full grid", full)):
            c.live_rays = c.total_rays = 0
            with torch.no_grad():
                c.render_poses(student, c2ws, ps)
            res[name] += (100. * c.live_rays / c.total_rays,)
        say("  %-9s switch off %.3f (%.3f)" % (fam, res["off"][0] / K, res["off"][1] / K))
        for name in ("+-2.5", "+-6", "empty grid, inside rays", "full grid"):
            say("  %-9s %-24s %.3f (%.3f)  = %.3f of off; live rays %.1f %%" %
                (fam, name, res[name][0] / K, res[name][1] / K, res[name][0] / res["off"][0], res[name][2]))
    engine.DEFAULT_CONFIG = {}

    say("")
    o, d = grids[2.5].frame_rays(c2ws, H, W, FOCAL, DEV)
    fns = {}
    for bound in (2.5, 6.0):
        c = grids[bound]
        fns["r2l_occ_rays +-%g, T = %d" % (bound, c.steps(H, W, FOCAL))] = (lambda c=c: c.grid.rays(o, d, NEAR, FAR, c.steps(H, W, FOCAL)))
    for name, (ms, sp) in timed(fns, reps=10).items():
        say("%s alone on %d x %d rays: %.3f ms (%.3f)" % (name, K, H * W, ms, sp))

    say("")
    chunk = 10
    n_pose = a.poses
    for bound in (2.5, 6.0):
        c = grids[bound]
        T = c.steps(H, W, FOCAL)
        cap = n_pose * H * W // 4096 + 1
        plain, culled = RayStore(cap, DEV), RayStore(cap, DEV)
        t_plain, t_cull, live = [], [], 0
        for g0 in range(0, n_pose, chunk):
            with torch.no_grad():
                rows = render_frames(poses(chunk, g0).to(DEV), H, W, FOCAL, NEAR, FAR, nets[0], nets[1], 64, 128, 1, True, seed=0,
                                     frame_id0=g0, rows=True, occupancy=(c.grid, c.grid))["rows"]
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            plain.append(rows, 1000 + g0)
            e[1].record()
            M, idx, _ = c.live_index(rows[:, 0:3], rows[:, 3:6], T)
            culled.append_live(rows, idx, M, 1000 + g0)
            e[2].record()
            torch.cuda.synchronize()
            t_plain.append(e[0].elapsed_time(e[1]))
            t_cull.append(e[1].elapsed_time(e[2]))
            live += M
        say("fill of %d poses in groups of %d, grid +-%g (both passes of the teacher skip with it): %d shards = %.3f GB without the "
            "switch, %d shards = %.3f GB with it (live rays %.1f %%); per group: append %.3f ms, r2l_occ_rays + read + append_live "
            "%.3f ms (medians)" % (n_pose, chunk, bound, plain.n_shards, plain.n_shards * 4096 * 36 / 1e9, culled.n_shards,
                                   culled.n_shards * 4096 * 36 / 1e9, 100. * live / (n_pose * H * W), float(np.median(t_plain)),
                                   float(np.median(t_cull))))
        plain.close()
        culled.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
