"""create_data in ms/pose with and without --r2l_fused_frames (teacher frames assembled per pose by render(), or per flush
group inside the library by r2l_teacher_frames_cfg): 400x400, 64+128 samples, the default fp16x2 teacher kernels, seeded D8
W256 teacher pair, shards shuffled and written by the background writer.  Both paths in ONE process on one box, alternated
`--repeats` times after a warm-up run of each; the table goes to stdout and, with --out, to a file.

    python tools/teacher_frames_time.py --poses 24 --repeats 3 --out profiles/teacher_frames.txt
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=24)
    ap.add_argument("--chunk", type=int, default=6, help="--create_data_chunk: poses per flush group")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out_path = os.path.abspath(a.out) if a.out else ""
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
