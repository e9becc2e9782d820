"""ms per teacher training step (r2l_amd/teacher_train.py) at the lego configuration: 1024 rays, 64 + 128 samples, perturb 1,
and the same step as torch fp32 autograd of the oracle's functions on the same GPU.  Prints one JSON line.

  python tools/teacher_train_time.py [--rays 1024] [--steps 20] [--warmup 3]

FLOP model (DESIGN.md §teacher training): forward 1.187 MFLOP, dX chain ~1.12 MFLOP, dW 1.187 MFLOP per point; the fraction
is of the 157.3 TFLOP/s fp32-MFMA peak.  The per-kernel split comes from a separate run of this script under
`rocprofv3 --kernel-trace --stats -- python tools/teacher_train_time.py`.

  python tools/teacher_train_time.py --batching [--steps 20] [--warmup 3] [--out profiles/teacher_batching.txt]

The data path of utils/train_nerf.py per batch, images mode against batching mode (--r2l_batching), on synthetic scenes of the
lego size (100 views of 400 x 400, N_rand 1024) and the fern size (17 views of 378 x 504, NDC, N_rand 1024 and 4096):
  host path      : sample_batch + device_rays + the copies of viewdirs and target, synchronised (what images mode does per step)
  PixelBatcher   : next(N_rand), synchronised per call, and back to back (one synchronisation after all calls)
  whole step     : either of them followed by TeacherTrainer.step (which reads the loss back, so every step is synchronised)
Wall-clock ms (time.perf_counter) around synchronised work; one line per scene to stdout and to --out.

  python tools/teacher_train_time.py --fused [--steps 20] [--warmup 3] [--repeats 3] [--out profiles/teacher_fused_step.txt]

The staged step (TeacherTrainer.step: ~25 library calls and torch ops, the loss read back every step) against the fused step
(TeacherTrainer.fused_step: one library call, nothing read back until the end) in the same process, on a fixed batch, at 1024 rays
(kernel-bound) and at 64 rays (where the host's share should show), 64 + 128 samples, perturb 1.  Wall-clock ms per step over
--steps steps, --repeats times each, alternating: the spread of a path's repeats is what a difference has to exceed.

  python tools/teacher_train_time.py --images [--steps 20] [--warmup 3] [--repeats 3] [--out profiles/teacher_image_sampler.txt]

Images mode's batch from the host (train_nerf._seed + sample_batch + device_rays + two copies, what the loop does without the
switch) against ImageBatcher.next (--r2l_image_sampler), at 400 x 400 (100 views) and 800 x 800 (25 views), N_rand 1024: ms per
batch (whole frame and centre crop; PixelBatcher.next beside it), and ms per whole iteration with the staged and the fused step,
with and without the switch.  One process, --repeats rounds alternating the paths; [median, max - min] per path."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import r2l_oracle as O  # noqa: E402

PEAK = 157.3e12
FLOP_PER_POINT = 1.187e6 + 1.12e6 + 1.187e6


def make(sd):
    from model.nerf_raybased import NeRF
    m = NeRF(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
    m.load_state_dict(sd)
    return m.cuda()


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def wall(fn, steps, warmup, sync_each=True):
    """ms per call of fn, wall clock; synchronised after every call, or once after all of them."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
        if sync_each:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def forward_facing_poses(n, rng):
    """[n,3,4]: rotations <= 0.35 rad about a random axis, centres within +-1 (z within +-0.3): every ray goes down -z."""
    out = []
    for _ in range(n):
        axis = rng.randn(3)
        axis /= np.linalg.norm(axis)
        ang = rng.uniform(-.35, .35)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
        out.append(np.concatenate([R, (rng.uniform(-1, 1, 3) * np.array([1., 1., .3]))[:, None]], 1))
    return np.stack(out).astype(np.float32)


def batching(a):
    from r2l_amd import train_nerf
    from r2l_amd.pixel_batch import PixelBatcher
    from r2l_amd.teacher_train import TeacherTrainer
    dev = torch.device("cuda")
    csd, fsd = O.make_teacher_state_dicts(5, 2, alpha_bias=0.5)
    rng = np.random.RandomState(0)
    scenes = [("lego-like", 100, 400, 400, 555.5555155968841, False, 2., 6., 128, (1024,)),
              ("fern-like", 17, 378, 504, 407.5657, True, 0., 1., 64, (1024, 4096))]
    lines = ["teacher training, data path per batch: images mode (host) against batching mode (r2l_pixel_batch); %s; steps %d, "
             "warmup %d; wall-clock ms" % (torch.cuda.get_device_name(0), a.steps, a.warmup)]
    for name, n, H, W, focal, ndc, near, far, NI, n_rands in scenes:
        images = rng.rand(n, H, W, 3).astype(np.float32)
        poses = (forward_facing_poses(n, rng) if ndc else
                 np.stack([O.pose_spherical(-180. + 360. * k / n, -30., 4.)[:3, :4] for k in range(n)]).astype(np.float32))
        i_train = np.arange(n)
        tr = TeacherTrainer(make(csd), make(fsd), N_samples=64, N_importance=NI, perturb=1., white_bkgd=not ndc, raw_noise_std=0.)
        pb = PixelBatcher(images, poses, H, W, focal, ndc, dev, seed=0)
        for N_rand in n_rands:
            args = argparse.Namespace(N_rand=N_rand, precrop_iters=0, precrop_frac=.5)
            it = [0]

            def host():
                it[0] += 1
                train_nerf._seed(it[0])
                o, d, v, t = train_nerf.sample_batch(it[0], args, images, poses, i_train, H, W, focal)
                o, d = train_nerf.device_rays(o, d, H, W, focal, ndc, dev)
                return o, d, v.to(dev), t.to(dev)

            def step(batch):
                o, d, v, t = batch()
                tr.step(o, d, v, near, far, t, 5e-4)

            r = {"scene": name, "views": n, "H": H, "W": W, "ndc": int(ndc), "N_rand": N_rand, "bank_MB": round(pb.nbytes / 1e6, 1),
                 "host_path_ms": round(wall(host, a.steps, a.warmup), 3),
                 "pixel_batcher_ms": round(wall(lambda: pb.next(N_rand), a.steps, a.warmup), 3),
                 "pixel_batcher_back_to_back_ms": round(wall(lambda: pb.next(N_rand), 10 * a.steps, a.warmup, sync_each=False), 4),
                 "step_images_mode_ms": round(wall(lambda: step(host), a.steps, a.warmup), 3),
                 "step_batching_mode_ms": round(wall(lambda: step(lambda: pb.next(N_rand)), a.steps, a.warmup), 3)}
            lines.append(json.dumps(r))
            print(lines[-1], flush=True)
        del tr, pb
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def fused(a):
    from r2l_amd.teacher_train import TeacherTrainer
    csd, fsd = O.make_teacher_state_dicts(5, 2, alpha_bias=0.5)
    lines = ["teacher training, staged step (TeacherTrainer.step, loss read back per step) against fused step (fused_step, one "
             "r2l_teacher_train_step call, loss read once at the end); 64 + 128 samples, perturb 1; %s; steps %d, warmup %d, "
             "repeats %d; wall-clock ms per step" % (torch.cuda.get_device_name(0), a.steps, a.warmup, a.repeats)]
    for R in (1024, 64):
        g = torch.Generator().manual_seed(0)
        o = (torch.randn(R, 3, generator=g) * .5).cuda()
        d = torch.randn(R, 3, generator=g).cuda()
        vd = d / d.norm(dim=-1, keepdim=True)
        tgt = torch.rand(R, 3, generator=g).cuda()
        tr = TeacherTrainer(make(csd), make(fsd), perturb=1., white_bkgd=True)
        hist = torch.zeros(a.warmup + a.steps, 2, device="cuda")
        it = [0]

        def fused_step():
            k = it[0] % hist.shape[0]
            it[0] += 1
            tr.fused_step(o, d, vd, 2., 6., tgt, 5e-4, step=it[0], seed=0, loss_out=hist[k])

        staged, fus = [], []
        for _ in range(a.repeats):
            staged.append(round(wall(lambda: tr.step(o, d, vd, 2., 6., tgt, 5e-4), a.steps, a.warmup, sync_each=False), 3))
            it[0] = 0
            fus.append(round(wall(fused_step, a.steps, a.warmup, sync_each=False), 3))
            hist.tolist()
        r = {"rays": R, "points": R * 256, "staged_ms": staged, "fused_ms": fus, "staged_median_ms": float(np.median(staged)),
             "fused_median_ms": float(np.median(fus)), "staged_spread_ms": round(max(staged) - min(staged), 3),
             "fused_minus_staged_ms": round(float(np.median(fus) - np.median(staged)), 3)}
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
        del tr
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def images(a):
    from r2l_amd import train_nerf
    from r2l_amd.image_batch import ImageBatcher, crop_window
    from r2l_amd.pixel_batch import PixelBatcher
    from r2l_amd.teacher_train import TeacherTrainer
    dev = torch.device("cuda")
    csd, fsd = O.make_teacher_state_dicts(5, 2, alpha_bias=0.5)
    rng = np.random.RandomState(0)
    N_rand, near, far = 1024, 2., 6.
    lines = ["teacher training in images mode, the batch of an iteration: host path (train_nerf: _seed + sample_batch + device_rays + "
             "the copies of viewdirs and target) against ImageBatcher.next (--r2l_image_sampler, one r2l_image_batch launch); N_rand "
             "%d, 64 + 128 samples, perturb 1; %s; steps %d, warmup %d, %d rounds alternating the paths in one process; wall-clock "
             "ms, [median, max - min] over the rounds" % (N_rand, torch.cuda.get_device_name(0), a.steps, a.warmup, a.repeats)]
    for n, H, W, focal in ((100, 400, 400, 555.5555155968841), (25, 800, 800, 1111.1110311937682)):
        imgs = rng.rand(n, H, W, 3).astype(np.float32)
        poses = np.stack([O.pose_spherical(-180. + 360. * k / n, -30., 4.)[:3, :4] for k in range(n)]).astype(np.float32)
        i_train = np.arange(n)
        tr = TeacherTrainer(make(csd), make(fsd), N_samples=64, N_importance=128, perturb=1., white_bkgd=True, raw_noise_std=0.)
        ib = ImageBatcher(imgs, poses, H, W, focal, False, dev, seed=0)
        pb = PixelBatcher(imgs, poses, H, W, focal, False, dev, seed=0)
        crop = crop_window(H, W, .5)
        hist = torch.zeros(a.warmup + a.steps, 2, device="cuda")
        it = [0]

        def host(precrop_iters=0, seed=True):
            it[0] += 1
            if seed:
                train_nerf._seed(it[0])
            args = argparse.Namespace(N_rand=N_rand, precrop_iters=precrop_iters, precrop_frac=.5)
            o, d, v, t = train_nerf.sample_batch(it[0], args, imgs, poses, i_train, H, W, focal)
            o, d = train_nerf.device_rays(o, d, H, W, focal, False, dev)
            return o, d, v.to(dev), t.to(dev)

        def device(window=None, seed=False):
            it[0] += 1
            if seed:  # (the staged step keeps the per-iteration re-seeding for torch's t_rand / u)
                train_nerf._seed(it[0])
            return ib.next(it[0], N_rand, window)

        def staged(batch):
            o, d, v, t = batch()
            tr.step(o, d, v, near, far, t, 5e-4)  # (reads the loss back: synchronised)

        def fused_(batch):
            o, d, v, t = batch()
            tr.fused_step(o, d, v, near, far, t, 5e-4, step=it[0], seed=0, loss_out=hist[it[0] % hist.shape[0]])

        paths = [
            ("batch_host_ms", lambda: host(), True),
            ("batch_sampler_ms", lambda: device(), True),
            ("batch_host_crop_ms", lambda: host(precrop_iters=1 << 30), True),
            ("batch_sampler_crop_ms", lambda: device(crop), True),
            ("batch_sampler_back_to_back_ms", lambda: device(), False),
            ("batch_pixel_batcher_ms", lambda: pb.next(N_rand), True),
            ("batch_pixel_batcher_back_to_back_ms", lambda: pb.next(N_rand), False),
            ("iter_staged_host_ms", lambda: staged(host), True),
            ("iter_staged_sampler_ms", lambda: staged(lambda: device(seed=True)), True),
            ("iter_fused_host_ms", lambda: fused_(host), False),
            ("iter_fused_sampler_ms", lambda: fused_(device), False),
        ]
        got = {name: [] for name, _, _ in paths}
        for _ in range(a.repeats):
            for name, fn, sync_each in paths:
                it[0] = 0
                got[name].append(wall(fn, a.steps, a.warmup, sync_each=sync_each))
                hist.tolist()
        r = {"views": n, "H": H, "W": W, "N_rand": N_rand, "bank_MB": round(ib.nbytes / 1e6, 1)}
        for name, _, _ in paths:
            r[name] = [round(float(np.median(got[name])), 3), round(max(got[name]) - min(got[name]), 3)]
        for kind in ("staged", "fused"):
            h, s = r["iter_%s_host_ms" % kind], r["iter_%s_sampler_ms" % kind]
            r["iter_%s_sampler_minus_host_ms" % kind] = round(s[0] - h[0], 3)
            r["iter_%s_sampler_not_slower" % kind] = bool(s[0] - h[0] <= max(h[1], s[1]))
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
        del tr, ib, pb, imgs
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no_baseline", action="store_true")
    ap.add_argument("--batching", action="store_true", help="time the data path: images mode's host path against PixelBatcher.next")
    ap.add_argument("--fused", action="store_true", help="time the staged step against the fused step (r2l_teacher_train_step)")
    ap.add_argument("--images", action="store_true", help="time images mode's host path against ImageBatcher.next (--r2l_image_sampler), "
                    "per batch and per whole iteration, staged and fused")
    ap.add_argument("--repeats", type=int, default=3, help="--fused / --images: timed runs per path")
    ap.add_argument("--out", default=None, help="where --batching / --fused / --images write their lines (default: "
                    "profiles/teacher_batching.txt / profiles/teacher_fused_step.txt / profiles/teacher_image_sampler.txt)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "teacher_train_time needs the GPU"
    if a.out is None:
        a.out = os.path.join("profiles", "teacher_image_sampler.txt" if a.images else
                             "teacher_fused_step.txt" if a.fused else "teacher_batching.txt")
    if a.images:
        return images(a)
    if a.fused:
        return fused(a)
    if a.batching:
        return batching(a)
    from r2l_amd.teacher_train import TeacherTrainer
    csd, fsd = O.make_teacher_state_dicts(5, 2, alpha_bias=0.5)
    tr = TeacherTrainer(make(csd), make(fsd), perturb=1., white_bkgd=True)
    R = a.rays
    g = torch.Generator().manual_seed(0)
    o = (torch.randn(R, 3, generator=g) * .5).cuda()
    d = torch.randn(R, 3, generator=g).cuda()
    vd = d / d.norm(dim=-1, keepdim=True)
    tgt = torch.rand(R, 3, generator=g).cuda()
    ms = timed(lambda: (tr.forward_backward(o, d, vd, 2., 6., tgt), tr.adam(5e-4)), a.steps, a.warmup)
    pts = R * (64 + 64 + 128)
    out = {"rays": R, "points": pts, "ms_per_step": round(ms, 3),
           "fraction_of_fp32_mfma_peak": round(FLOP_PER_POINT * pts / (ms * 1e-3) / PEAK, 4),
           "ideal_ms": round(FLOP_PER_POINT * pts / PEAK * 1e3, 3)}
    if not a.no_baseline:
        sds = [{k: v.cuda().requires_grad_(True) for k, v in sd.items()} for sd in (csd, fsd)]
        opt = torch.optim.Adam([p for sd in sds for p in sd.values()], lr=5e-4)
        t = torch.linspace(0., 1., steps=64, device="cuda")

        def step():
            with torch.device("cuda"):  # the oracle builds its constants without a device argument
                z = (2. * (1. - t) + 6. * t).expand(R, 64)
                lo, up = O.stratified_bounds(z)
                z = lo + (up - lo) * torch.rand(R, 64)
                raw0 = O.run_network(sds[0], o[:, None] + d[:, None] * z[..., None], vd)
                rgb0, _, _, w0, _ = O.raw2outputs(raw0, z, d, None, True)
                zs = O.sample_pdf(.5 * (z[..., 1:] + z[..., :-1]), w0[..., 1:-1].detach(), 128, u=torch.rand(R, 128)).detach()
                za = torch.sort(torch.cat([z, zs], -1), -1)[0]
                raw = O.run_network(sds[1], o[:, None] + d[:, None] * za[..., None], vd)
                rgb = O.raw2outputs(raw, za, d, None, True)[0]
                loss = torch.mean((rgb - tgt)**2) + torch.mean((rgb0 - tgt)**2)
                opt.zero_grad()
                loss.backward()
                opt.step()
        out["torch_autograd_ms_per_step"] = round(timed(step, max(3, a.steps // 4), 2), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
