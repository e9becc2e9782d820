"""Measurements of the device-resident ray store (r2l_amd/raystore.py, r2l_amd/online_kd.py; profiles/raystore.txt):

  loop   the CLI training loop (tools/e2e_train.py) from shard files against --r2l_device_store, alternated `--reps` times in
         one process; the file path's own run-to-run spread is printed beside the difference
  draw   device time of RayStore.next(20) over 240 shards (device events around 200 calls) and the bytes/s it amounts to
         (2 x 20 x 147 456 B per call: every byte is read once and written once)
  files  GB/s of RayStore.append_files for 240 shards
  fill   poses/s of the teacher fill (fill_store_from_teacher) against create_data --r2l_fused_frames for the same poses at
         400 x 400, alternated, and the append's share of a flush group (device events)

python tools/raystore_time.py [loop] [draw] [files] [fill] [--reps 3] [--poses 100] [--chunk 50]"""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import r2l_oracle as O  # noqa: E402
from r2l_amd import create_data, data, options  # noqa: E402
from r2l_amd.online_kd import fill_store_from_teacher, shards_needed  # noqa: E402
from r2l_amd.raystore import RayStore  # noqa: E402
from tools import e2e_train  # noqa: E402


def write_shards(kd, n_files):
    rng = np.random.RandomState(0)
    for k in range(0, n_files, 40):
        data.write_ray_shards(rng.rand(40 * 4096, 9).astype(np.float32), kd, k)
    return [os.path.join(kd, "data_%d.npy" % k) for k in range(n_files)]


def loop(reps):
    ms = {"files": [], "store": []}
    for r in range(reps):
        for tag, extra in (("files", []), ("store", ["--r2l_device_store"])):
            ms[tag].append(e2e_train.main(extra=extra))
    f, s = np.array(ms["files"]), np.array(ms["store"])
    print("loop: files %s ms/iter (mean %.3f, spread max - min %.3f); store %s ms/iter (mean %.3f); store - files %+.3f ms/iter" %
          (np.round(f, 3).tolist(), f.mean(), f.max() - f.min(), np.round(s, 3).tolist(), s.mean(), s.mean() - f.mean()))


def draw(n_shards=240, n_files=20, calls=200):
    store = RayStore(n_shards, "cuda")
    store.append(torch.rand(n_shards * 4096, 9, device="cuda"), key=1)
    for _ in range(20):
        store.next(n_files)
    out = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            store.next(n_files)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / calls * 1e3)
    us = float(np.median(out))
    print("draw: next(%d) over %d shards: %s us per call (median %.2f us) = %.0f GB/s read + written" %
          (n_files, n_shards, np.round(out, 2).tolist(), us, 2 * n_files * 147456 / us / 1e3))


def files(n_shards=240, threads=8):
    kd = tempfile.mkdtemp(prefix="r2l_store_")
    paths = write_shards(kd, n_shards)
    for r in range(3):
        store = RayStore(n_shards, "cuda")
        print("files: " + store.append_files(paths, threads=threads)["message"])
    shutil.rmtree(kd)


def fill(reps, n_pose, chunk):
    tmp = tempfile.mkdtemp(prefix="r2l_fill_")
    os.chdir(tmp)
    csd, fsd = O.make_teacher_state_dicts(5, 2, alpha_bias=0.5)
    ck = os.path.join(tmp, "teacher.tar")
    torch.save({"global_step": 200000, "network_fn_state_dict": csd, "network_fine_state_dict": fsd}, ck)
    cfg = os.path.join(ROOT, "configs", "lego.txt")
    H, W, focal = 400, 400, 555.5555155968841  # what create_data uses without a scene directory
    common = ["--create_data", "rand", "--config", cfg, "--datadir", os.path.join(tmp, "no_scene"), "--teacher_ckpt", ck,
              "--n_pose_kd", str(n_pose), "--create_data_chunk", str(chunk)]
    targs = options.parse_args(common)
    per = {"store": [], "files": []}
    for r in range(reps + 1):  # (the first round warms both up and is not counted)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        store = RayStore(shards_needed(n_pose, chunk, H, W), "cuda")
        state = fill_store_from_teacher(store, targs, H, W, focal, 2., 6., n_pose, chunk, 0, 1, "cuda")
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        share = [e[1].elapsed_time(e[2]) / e[0].elapsed_time(e[2]) for e in state.append_ms]
        del store, state
        torch.cuda.empty_cache()
        kd = os.path.join(tmp, "pseudo")
        t0 = time.perf_counter()
        create_data.main(common + ["--datadir_kd", "x:" + kd, "--rm_existing_data", "--r2l_fused_frames", "--experiment_name", "cd%d" % r])
        torch.cuda.synchronize()
        dt_files = time.perf_counter() - t0
        if r:
            per["store"].append(n_pose / dt)
            per["files"].append(n_pose / dt_files)
            print("fill: round %d: store %.2f poses/s (%.1f ms/pose; append %.3f %% of a flush group), create_data --r2l_fused_frames "
                  "%.2f poses/s (%.1f ms/pose)" % (r, n_pose / dt, dt / n_pose * 1e3, 100 * float(np.mean(share)), n_pose / dt_files,
                                                   dt_files / n_pose * 1e3))
    print("fill: %d poses at %dx%d, groups of %d: store mean %.2f poses/s, files mean %.2f poses/s" %
          (n_pose, H, W, chunk, np.mean(per["store"]), np.mean(per["files"])))
    os.chdir(ROOT)
    shutil.rmtree(tmp)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["draw", "files", "loop", "fill"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--poses", type=int, default=100)
    ap.add_argument("--chunk", type=int, default=50)
    a = ap.parse_args()
    sys.argv = sys.argv[:1]  # (e2e_train passes its own command line through to main.py)
    for what in a.what:
        {"loop": lambda: loop(a.reps), "draw": draw, "files": files, "fill": lambda: fill(a.reps, a.poses, a.chunk)}[what]()
