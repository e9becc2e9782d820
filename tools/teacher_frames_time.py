"""create_data in ms/pose with and without --r2l_fused_frames (teacher frames assembled per pose by render(), or per flush
group inside the library by r2l_teacher_frames_cfg): 400x400, 64+128 samples, the default fp16x2 teacher kernels, seeded D8
W256 teacher pair, shards shuffled and written by the background writer.  Both paths in ONE process on one box, alternated
`--repeats` times after a warm-up run of each; the table goes to stdout and, with --out, to a file.

    python tools/teacher_frames_time.py --poses 24 --repeats 3 --out profiles/teacher_frames.txt

--ndc measures something else, the cost of NDC rays (forward-facing LLFF scenes): render_frames on K frames of 378 x 504 (the
LLFF frame at factor 8), 64+64 samples, with ndc = False and ndc = True alternated, in ms per frame by device events, and
r2l_ndc_rays alone on the 190 512 rays of one frame against the 48 bytes per ray it moves.

    python tools/teacher_frames_time.py --ndc --poses 4 --repeats 5 --out profiles/llff_ndc.txt
"""
import argparse
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from model.nerf_raybased import NeRF  # noqa: E402
from r2l_amd import create_data  # noqa: E402


def forward_poses(K, seed=0):
    """K forward-facing poses [K,3,4]: rotations <= 0.35 rad about a random axis, origins within +-1 (z within +-0.3)."""
    import numpy as np
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(K):
        axis = rng.randn(3)
        axis /= np.linalg.norm(axis)
        ang = rng.uniform(-.35, .35)
        Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        R = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * (Kx @ Kx)
        out.append(np.concatenate([R, (rng.uniform(-1, 1, 3) * np.array([1., 1., .3]))[:, None]], 1))
    return torch.from_numpy(np.stack(out).astype(np.float32))


def time_ndc(a, out_path):
    from r2l_amd import render
    H, W, focal, NS, NI = a.height, a.width, 408., 64, 64  # (fern at factor 8: 378 x 504, focal ~ 408)
    torch.manual_seed(3)
    nets = []
    for _ in range(2):
        m = NeRF(D=8, W=256, input_ch=63, output_ch=4, skips=[4], input_ch_views=27, use_viewdirs=True)
        with torch.no_grad():
            m.alpha_linear.bias.add_(0.5)
        for q in m.parameters():
            q.requires_grad = False
        nets.append(m.cuda().eval())
    c2ws = forward_poses(a.poses).cuda()

    def frames(ndc):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        with torch.no_grad():
            render.render_frames(c2ws, H, W, focal, 0., 1., nets[0], nets[1], NS, NI, 1., False, seed=1, ndc=ndc)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.poses

    for ndc in (False, True):
        frames(ndc)  # warm-up: weight packing, allocator, work buffer
    ms = {False: [], True: []}
    for _ in range(a.repeats):
        for ndc in (False, True):
            ms[ndc].append(frames(ndc))
    # the transform alone, on the rays of one frame: many launches between two events
    o, d, _ = render.frame_rays(c2ws[:1], H, W, focal)
    n, reps = o.shape[0], 200
    for _ in range(10):
        render.ndc_rays(H, W, focal, 1., o, d)
    alone = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            render.ndc_rays(H, W, focal, 1., o, d)
        e1.record()
        torch.cuda.synchronize()
        alone.append(e0.elapsed_time(e1) * 1e3 / reps)
    med = lambda v: sorted(v)[len(v) // 2]
    lines = ["render_frames, %d x %d, %d+%d samples, perturb 1, default (fp16x2) teacher kernels, %d frames per call, %s" %
             (H, W, NS, NI, a.poses, torch.cuda.get_device_name(0)),
             "ms/frame (device events), calls alternated: ndc = 0 -> ndc = 1"]
    for ndc in (False, True):
        v = ms[ndc]
        lines.append("  ndc = %d   %s   median %.2f, spread %.2f" % (ndc, "  ".join("%.2f" % x for x in v), med(v), max(v) - min(v)))
    lines.append("  ndc = 1 over ndc = 0: %+.2f %% of a frame (medians)" % (100. * (med(ms[True]) / med(ms[False]) - 1.)))
    lines.append("r2l_ndc_rays alone (render.ndc_rays: two output allocations + one launch), %d rays, %d calls per timing:" % (n, reps))
    lines.append("  us/call  %s   median %.1f = %.0f GB/s of the %d bytes it moves (48 per ray)" %
                 ("  ".join("%.1f" % x for x in alone), med(alone), n * 48 / med(alone) * 1e-3, n * 48))
    text = "\n".join(lines)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ndc", action="store_true", help="time render_frames with ndc = 0 / 1 and r2l_ndc_rays alone instead")
    ap.add_argument("--height", type=int, default=378)
    ap.add_argument("--width", type=int, default=504, help="frame of --ndc (378 x 504: the LLFF scenes at factor 8)")
    ap.add_argument("--poses", type=int, default=24)
    ap.add_argument("--chunk", type=int, default=6, help="--create_data_chunk: poses per flush group")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out_path = os.path.abspath(a.out) if a.out else ""
    if a.ndc:
        return time_ndc(a, out_path)
    tmp = tempfile.mkdtemp(prefix="r2l_tf_")
    os.chdir(tmp)
    torch.manual_seed(3)
    sds = []
    for _ in range(2):
        m = NeRF(D=8, W=256, input_ch=63, output_ch=4, skips=[4], input_ch_views=27, use_viewdirs=True)
        with torch.no_grad():
            m.alpha_linear.bias.add_(0.5)
        sds.append(m.state_dict())
    torch.save({"network_fn_state_dict": sds[0], "network_fine_state_dict": sds[1]}, os.path.join(tmp, "teacher.tar"))
    kd = os.path.join(tmp, "pseudo")
    argv = ["--create_data", "rand", "--config", os.path.join(ROOT, "configs", "lego.txt"), "--datadir", os.path.join(tmp, "no_scene"),
            "--teacher_ckpt", os.path.join(tmp, "teacher.tar"), "--create_data_chunk", str(a.chunk), "--datadir_kd", "x:" + kd,
            "--experiment_name", "cd", "--rm_existing_data", "--r2l_precision", "fp16x2"]
    paths = {"render() per pose": [], "--r2l_fused_frames": ["--r2l_fused_frames"]}

    def run(extra, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        create_data.main(argv + extra + ["--n_pose_kd", str(n)])  # returns after the writer thread has saved the last shard
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    for extra in paths.values():
        run(extra, a.chunk)  # warm-up: imports, weight packing, allocator, work buffer
    ms = {k: [] for k in paths}
    for _ in range(a.repeats):
        for k, extra in paths.items():
            ms[k].append(run(extra, a.poses))
    lines = ["create_data rand, 400x400, 64+128 samples, fp16x2, %d poses per run, flush groups of %d, %s" %
             (a.poses, a.chunk, torch.cuda.get_device_name(0)),
             "ms/pose (wall, shard writing included), runs alternated: " + " -> ".join(paths)]
    for k, v in ms.items():
        lines.append("  %-22s %s   median %.1f, spread %.1f" % (k, "  ".join("%.1f" % x for x in v), sorted(v)[len(v) // 2], max(v) - min(v)))
    text = "\n".join(lines)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
