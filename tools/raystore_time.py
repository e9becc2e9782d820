"""Measurements of the device-resident ray store (r2l_amd/raystore.py, r2l_amd/online_kd.py; profiles/raystore.txt):

  loop   the CLI training loop (tools/e2e_train.py) from shard files against --r2l_device_store, alternated `--reps` times in
         one process; the file path's own run-to-run spread is printed beside the difference
  draw   device time of RayStore.next(20) over 240 shards (device events around 200 calls) and the bytes/s it amounts to
         (2 x 20 x 147 456 B per call: every byte is read once and written once)
  files  GB/s of RayStore.append_files for 240 shards
  fill   poses/s of the teacher fill (fill_store_from_teacher) against create_data --r2l_fused_frames for the same poses at
         400 x 400, alternated, and the append's share of a flush group (device events)

python tools/raystore_time.py [loop] [draw] [files] [fill] [--reps 3] [--poses 100] [--chunk 50]
python tools/raystore_time.py --compact [--reps 3] [--poses 100]   the compact store (CompactRayStore, 16 B/ray) against the plain
         one: next(20) / next(1), a flush group of fill_group, memory after the fill -> profiles/cstore.txt (compact() below)
python tools/raystore_time.py --file [--reps 3] [--poses 100]   the store file: r2l_words_digest against a device copy, save and
         load of a plain and a compact store -> profiles/store_file.txt (store_file() below)
python tools/raystore_time.py --images [--reps 3] [--poses 100]   the real rays of --poses frames at 400 x 400 into a store:
         RayStore.append_images (one launch) against r2l_frame_rays + rgb copy + r2l_store_append, and against the converter's files
         read back by append_files -> profiles/image_store.txt (images() below)"""
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


def _synthetic_group(K, H, W, rng):
    """(rows [K*H*W, 9], c2ws [K, 3, 4], focals [K]): rays of K random poses from r2l_frame_rays, random rgb."""
    import ctypes
    from r2l_amd import _lib
    c2ws = torch.stack([data.get_rand_pose(rng)[:3, :4] for _ in range(K)], 0).float().cuda().contiguous()
    focals = torch.tensor(555.5555155968841 * (1 + rng.rand(K)), dtype=torch.float32, device="cuda")
    rows = torch.empty(K * H * W, 9, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(_lib.load().r2l_frame_rays(p(c2ws), p(focals), 0., K, H, W, None, None, None, p(rows),
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "r2l_frame_rays")
    rows[:, 6:9] = torch.rand(K * H * W, 3, device="cuda")
    return rows, c2ws, focals


def _us_per_call(store, n_files, calls=200):
    for _ in range(20):
        store.next(n_files)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        store.next(n_files)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3


def compact(reps, n_pose, out_path):
    """--compact: the compact store (16 B/ray, CompactRayStore) against the plain one (36 B/ray, RayStore), all in this process,
    `reps` rounds alternating the two; medians, and the spread (max - min) between the runs of the same path.
      next   us per next(20) and per next(1) at H = W = 400 (4 flush groups of 6 poses: 936 shards), device events around 200 calls
      fill   ms per flush group of fill_group (n_pose poses at 400 x 400 in one group), device events of TeacherFill
      bytes  torch.cuda.memory_allocated after the fill against the byte arithmetic"""
    from r2l_amd.online_kd import TeacherFill
    from r2l_amd.raystore import CompactRayStore
    H = W = 400
    lines = ["tools/raystore_time.py --compact --reps %d --poses %d   (%s)" % (reps, n_pose, torch.cuda.get_device_name(0))]
    say = lambda s: (lines.append(s), print(s))
    # ---- next ----
    K, G = 6, 4
    cap = G * (K * H * W // 4096)
    plain, comp = RayStore(cap, "cuda", seed=5), CompactRayStore(cap, G * K, H, W, "cuda", seed=5)
    rng = np.random.RandomState(0)
    for g in range(G):
        rows, c2ws, focals = _synthetic_group(K, H, W, rng)
        plain.append(rows, key=g + 1)
        comp.append_frames(rows[:, 6:9], c2ws, focals, key=g + 1)
        del rows
    assert torch.equal(plain.next(3), comp.next(3))
    for n in (20, 1):
        us = {"plain": [], "compact": []}
        for r in range(reps):
            us["plain"].append(_us_per_call(plain, n))
            us["compact"].append(_us_per_call(comp, n))
        a, b = np.array(us["plain"]), np.array(us["compact"])
        say("next(%d) over %d shards at %dx%d: plain %s us (median %.2f, spread %.2f) | compact %s us (median %.2f, spread %.2f) | "
            "compact - plain %+.2f us; bytes per ray: plain 36 read + 36 written, compact 16 read + 36 written; compact moves "
            "%.0f GB/s" % (n, cap, H, W, np.round(a, 2).tolist(), np.median(a), a.max() - a.min(), np.round(b, 2).tolist(), np.median(b),
                          b.max() - b.min(), np.median(b) - np.median(a), n * 4096 * 52 / np.median(b) / 1e3))
    plain.close()
    comp.close()
    del plain, comp
    torch.cuda.empty_cache()
    # ---- fill ----
    tmp = tempfile.mkdtemp(prefix="r2l_cfill_")
    csd, fsd = O.make_teacher_state_dicts(5, 2, alpha_bias=0.5)
    ck = os.path.join(tmp, "teacher.tar")
    torch.save({"global_step": 200000, "network_fn_state_dict": csd, "network_fine_state_dict": fsd}, ck)
    targs = options.parse_teacher_config(os.path.join(ROOT, "configs", "lego.txt"), teacher_ckpt=ck)
    focal = 555.5555155968841
    shards = shards_needed(n_pose, n_pose, H, W)
    ms, alloc = {"plain": [], "compact": []}, {}
    for r in range(reps + 1):  # (the first round warms both up and is not counted)
        for tag in ("plain", "compact"):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            store = RayStore(shards, "cuda") if tag == "plain" else CompactRayStore(shards, n_pose, H, W, "cuda")
            state = TeacherFill(store, targs, H, W, focal, 2., 6., n_pose, n_pose, 0, 1, "cuda")
            state.fill_group()
            torch.cuda.synchronize()
            e = state.append_ms[0]
            if r:
                ms[tag].append((e[0].elapsed_time(e[2]), e[1].elapsed_time(e[2])))
            del state, e
            torch.cuda.empty_cache()
            alloc[tag] = (torch.cuda.memory_allocated() - base, store.nbytes)
            store.close()
            del store
    for tag in ("plain", "compact"):
        g = np.array([m[0] for m in ms[tag]])
        ap_ = np.array([m[1] for m in ms[tag]])
        say("fill_group, %d poses at %dx%d into the %s store: %s ms per flush group (median %.1f, spread %.1f); of which the append %s ms"
            % (n_pose, H, W, tag, np.round(g, 1).tolist(), np.median(g), g.max() - g.min(), np.round(ap_, 3).tolist()))
    for tag in ("plain", "compact"):
        say("after the fill, %s store: torch.cuda.memory_allocated grew by %d B; byte arithmetic %d B (%d shards of 4096 rays%s)" %
            (tag, alloc[tag][0], alloc[tag][1], shards, "" if tag == "plain" else ", %d poses" % n_pose))
    say("not measured: the 800x800 / 10 000-pose fill (102.4 GB by the arithmetic above)")
    shutil.rmtree(tmp)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


def _ms_per_call(fn, calls=20, warm=3):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def store_file(reps, n_pose, out_path):
    """--file: the store file (RayStore.save / load_store, r2l_words_digest) for a plain and a compact store after one flush group
    of n_pose poses at 400 x 400, all in this process, `reps` rounds alternating the two stores; medians and the spread.
      digest  r2l_words_digest over the rows (one item a shard) in GB/s read, device events around 20 calls, against a torch
              device-to-device copy of the same bytes (which reads and writes them)
      save    RayStore.save to a temporary directory: seconds and GB/s, digests, pinned staging, pwrite and fsync included
      load    load_store of that file: seconds and GB/s, allocation, staging and the digest check included"""
    import ctypes
    from r2l_amd import _lib
    from r2l_amd.online_kd import TeacherFill
    from r2l_amd.raystore import CompactRayStore, load_store
    H = W = 400
    lines = ["tools/raystore_time.py --file --reps %d --poses %d   (%s)" % (reps, n_pose, torch.cuda.get_device_name(0))]
    say = lambda s: (lines.append(s), print(s))
    tmp = tempfile.mkdtemp(prefix="r2l_sfile_")
    csd, fsd = O.make_teacher_state_dicts(5, 2, alpha_bias=0.5)
    ck = os.path.join(tmp, "teacher.tar")
    torch.save({"global_step": 200000, "network_fn_state_dict": csd, "network_fine_state_dict": fsd}, ck)
    targs = options.parse_teacher_config(os.path.join(ROOT, "configs", "lego.txt"), teacher_ckpt=ck)
    shards = shards_needed(n_pose, n_pose, H, W)
    stores, prov = {}, {}
    for tag in ("plain", "compact"):
        store = RayStore(shards, "cuda") if tag == "plain" else CompactRayStore(shards, n_pose, H, W, "cuda")
        state = TeacherFill(store, targs, H, W, 555.5555155968841, 2., 6., n_pose, n_pose, 0, 1, "cuda")
        state.fill_group()
        torch.cuda.synchronize()
        e = state.append_ms[0]
        say("fill_group, %d poses at %dx%d into the %s store: %.1f ms (one flush group; the plain fill is the first of the process)" %
            (n_pose, H, W, tag, e[0].elapsed_time(e[2])))
        stores[tag], prov[tag] = store, state.provenance()
        del state, e
        torch.cuda.empty_cache()
    L, lib = _lib, _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    res = {tag: {"digest": [], "copy": [], "save": [], "load": []} for tag in stores}
    for r in range(reps):
        for tag, store in stores.items():
            rows = store.data[:store.n_shards * store.rows_per_file]
            nbytes = rows.numel() * 4
            out = torch.empty(store.n_shards, dtype=torch.int64, device="cuda")
            st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            wpi = store.rows_per_file * store.ROW_WORDS
            ms = _ms_per_call(lambda: L.check(lib.r2l_words_digest(p(rows), wpi, store.n_shards, 1, p(out), st), "r2l_words_digest"))
            res[tag]["digest"].append(nbytes / ms / 1e6)
            dst = torch.empty_like(rows)
            res[tag]["copy"].append(nbytes / _ms_per_call(lambda: dst.copy_(rows)) / 1e6)
            del dst, out
            path = os.path.join(tmp, tag + ".r2l")
            info = store.save(path, provenance=prov[tag])
            res[tag]["save"].append((info["seconds"], info["GB/s"]))
            loaded = load_store(path, "cuda")
            res[tag]["load"].append((loaded.load_info["seconds"], loaded.load_info["GB/s"]))
            if r == 0:
                assert all(torch.equal(a, b) for (_, a), (_, b) in zip(store._sections(), loaded._sections()))
                res[tag]["bytes"] = info["bytes"]
            loaded.close()
            del loaded
            torch.cuda.empty_cache()
    for tag in stores:
        d, c = np.array(res[tag]["digest"]), np.array(res[tag]["copy"])
        say("%s store, %d shards of 4096 rays, rows %.3f GB: r2l_words_digest %s GB/s read (median %.0f, spread %.0f) | torch copy of "
            "the same bytes %s GB/s copied, i.e. read and written (median %.0f, spread %.0f)" %
            (tag, shards, stores[tag].n_shards * 4096 * stores[tag].ROW_WORDS * 4 / 1e9, np.round(d).tolist(), np.median(d), d.max() - d.min(),
             np.round(c).tolist(), np.median(c), c.max() - c.min()))
        for what in ("save", "load"):
            s, g = np.array([x[0] for x in res[tag][what]]), np.array([x[1] for x in res[tag][what]])
            say("%s store, file of %d B: %s %s s (median %.3f, spread %.3f) = %s GB/s (median %.2f)" %
                (tag, res[tag]["bytes"], what, np.round(s, 3).tolist(), np.median(s), s.max() - s.min(), np.round(g, 2).tolist(), np.median(g)))
    say("the file system is a temporary directory of the machine (%s) and a load reads what the save just wrote (page cache); the "
        "rows are re-read from device memory call after call, partly out of the last-level cache at these sizes, the copy's as the "
        "digest's; not measured: a 10 000-pose store (25.6 / 57.6 GB)" % tempfile.gettempdir())
    shutil.rmtree(tmp)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


def images(reps, n_frames, out_path):
    """--images: the real training rays of n_frames frames at 400 x 400 as store rows, all in this process, `reps` rounds
    alternating the routes; medians and the spread (max - min) between the rounds of the same route.
      one launch     RayStore.append_images (r2l_store_append_images): device events around 10 calls; GB/s against 48 B a ray
                     (12 gathered, 36 written)
      three launches r2l_frame_rays(rows) + the rgb copy into columns 6..8 + r2l_store_append, the [n, 9] intermediate allocated
                     once outside the timing; the same 48 B a ray as the yardstick (it moves 24 + 24 + 72 B more)
      files          data.convert_images_to_ray_shards on the same frames as PNGs (wall time, reading the PNGs included) plus
                     RayStore.append_files of what it wrote: the route of the parent commit"""
    import ctypes
    import json
    from PIL import Image
    from r2l_amd import _lib
    H = W = 400
    K, focal, key = n_frames, 555.5555155968841, 0x1234567
    lines = ["tools/raystore_time.py --images --reps %d --poses %d   (%s)" % (reps, K, torch.cuda.get_device_name(0))]
    say = lambda s: (lines.append(s), print(s))
    rng = np.random.RandomState(0)
    png = (rng.rand(K, H, W, 4) * 255).astype(np.uint8)
    poses = torch.stack([data.get_rand_pose(rng) for _ in range(K)], 0).float()
    rgba = torch.from_numpy(png.astype(np.float32) / 255.)
    imgs = (rgba[..., :3] * rgba[..., -1:] + (1. - rgba[..., -1:])).cuda().contiguous()  # the loader's composite on white
    c2ws = poses[:, :3, :4].cuda().contiguous()
    n, cap = K * H * W, K * H * W // 4096
    L, lib = _lib, _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    new, old = RayStore(cap, "cuda"), RayStore(cap, "cuda")
    rows = torch.empty(n, 9, device="cuda")

    def reset(s):
        s.n_shards, s.files = 0, []

    def one():
        reset(new)
        new.append_images(imgs, c2ws, focal, key)

    def three():
        reset(old)
        L.check(lib.r2l_frame_rays(p(c2ws), None, focal, K, H, W, None, None, None, p(rows), st), "r2l_frame_rays")
        rows[:, 6:9] = imgs.view(-1, 3)
        old.append(rows, key)

    one()
    three()
    assert torch.equal(new.shards(), old.shards())  # the same store bit for bit
    ms = {"one": [], "three": []}
    for r in range(reps):
        ms["one"].append(_ms_per_call(one, calls=10))
        ms["three"].append(_ms_per_call(three, calls=10))
    a, b = np.array(ms["one"]), np.array(ms["three"])
    say("%d frames at %dx%d = %d rays -> %d shards of 4096 (%.3f GB of rows), %d rounds alternating, 10 calls a round, device events" %
        (K, H, W, n, cap, cap * 4096 * 36 / 1e9, reps))
    say("one launch (r2l_store_append_images):                   %s ms (median %.3f, spread %.3f) = %.0f GB/s at 48 B a ray" %
        (np.round(a, 3).tolist(), np.median(a), a.max() - a.min(), n * 48 / np.median(a) / 1e6))
    say("three launches (r2l_frame_rays + rgb copy + r2l_store_append): %s ms (median %.3f, spread %.3f) = %.0f GB/s at 48 B a ray" %
        (np.round(b, 3).tolist(), np.median(b), b.max() - b.min(), n * 48 / np.median(b) / 1e6))
    say("one - three = %+.3f ms (spread of the three-launch route %.3f ms): the one launch is %s" %
        (np.median(a) - np.median(b), b.max() - b.min(),
         "not slower beyond that spread" if np.median(a) - np.median(b) <= b.max() - b.min() else "SLOWER beyond that spread"))
    old.close()
    del rows, old
    torch.cuda.empty_cache()
    # ---- the file route of the parent commit ----
    tmp = tempfile.mkdtemp(prefix="r2l_images_")
    scene = os.path.join(tmp, "scene")
    os.makedirs(os.path.join(scene, "train"))
    t0 = time.perf_counter()
    for i in range(K):
        Image.fromarray(png[i]).save(os.path.join(scene, "train", "r_%d.png" % i), compress_level=1)
    with open(os.path.join(scene, "transforms_train.json"), "w") as f:
        json.dump({"camera_angle_x": 0.6911112070083618,
                   "frames": [{"file_path": "./train/r_%d" % i, "transform_matrix": poses[i].tolist()} for i in range(K)]}, f)
    t_png = time.perf_counter() - t0
    conv, load = [], []
    for r in range(reps):
        t0 = time.perf_counter()
        kd, n_files = data.convert_images_to_ray_shards(scene, full_res=True, white_bkgd=True, rng=np.random.RandomState(r))
        conv.append(time.perf_counter() - t0)
        paths = [os.path.join(kd, "train_%d.npy" % (k + 1)) for k in range(n_files)]
        reset(new)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        new.append_files(paths, threads=8)
        torch.cuda.synchronize()
        load.append(time.perf_counter() - t0)
        shutil.rmtree(kd)
    c, l = np.array(conv), np.array(load)
    say("files (utils/convert_original_data_to_rays_blender.py's work + --r2l_device_store's load), %d files: converter %s s (median "
        "%.2f, spread %.2f; it reads the %d PNGs, written here in %.1f s) + append_files %s s (median %.3f) = %.2f s against %.3f ms" %
        (cap, np.round(c, 2).tolist(), np.median(c), c.max() - c.min(), K, t_png, np.round(l, 3).tolist(), np.median(l),
         np.median(c) + np.median(l), np.median(a)))
    say("the file system is a temporary directory of the machine (%s): the load reads what the converter just wrote (page cache); "
        "every route also decodes the PNGs once (the loader does for the one launch); not measured: 800x800 frames" % tempfile.gettempdir())
    new.close()
    shutil.rmtree(tmp)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["draw", "files", "loop", "fill"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--poses", type=int, default=100)
    ap.add_argument("--chunk", type=int, default=50)
    ap.add_argument("--compact", action="store_true", help="compact store against the plain one -> profiles/cstore.txt")
    ap.add_argument("--file", action="store_true", help="store file: digest, save and load rates -> profiles/store_file.txt")
    ap.add_argument("--images", action="store_true", help="real rays from images: one launch against three and against files -> "
                    "profiles/image_store.txt")
    ap.add_argument("--out", default=None, help="default: profiles/cstore.txt (--compact), profiles/store_file.txt (--file), "
                    "profiles/image_store.txt (--images)")
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "image_store.txt" if a.images else "store_file.txt" if a.file else "cstore.txt")
    if a.images:
        images(a.reps, a.poses, a.out)
        sys.exit(0)
    if a.file:
        store_file(a.reps, a.poses, a.out)
        sys.exit(0)
    if a.compact:
        compact(a.reps, a.poses, a.out)
        sys.exit(0)
    sys.argv = sys.argv[:1]  # (e2e_train passes its own command line through to main.py)
    for what in a.what:
        {"loop": lambda: loop(a.reps), "draw": draw, "files": files, "fill": lambda: fill(a.reps, a.poses, a.chunk)}[what]()
