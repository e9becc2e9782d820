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
with and without the switch.  One process, --repeats rounds alternating the paths; [median, max - min] per path.

  python tools/teacher_train_time.py --occ [--steps 20] [--warmup 3] [--repeats 3] [--effect_iters 3000] [--out profiles/teacher_occ_train.txt]

The training step on the live samples of occupancy grids (--r2l_occ_train; TeacherTrainer.set_occupancy) against the plain step of the
same process, on the trained-like pair of tests/teacher_util.py: 1024 rays of scene_rays' camera drawn over its frame, 64 + 128
samples, perturb 1, lr 0 (the weights and with them the live share stay put), grids of 128^3 cells over +-1.6 and +-2.5 and an
all-ones grid (the floor of the capacity-sized launches plus r2l_occ_index); staged and fused, --repeats alternating rounds.  Then
the refresh: OccupancyGrid.rebuild per grid in the exact-fp32 family at 64^3 and 128^3 cells, and the smallest power of two K at
which two rebuilds cost at most 2 % of K plain steps.  Then (--effect_iters > 0) the effect on a result: the analytic scene of
tests/teacher_util.py trained from initial weights with and without grids, and a second seed of the plain run for the spread;
held-out PSNR of each and the newly set cells of every refresh."""
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


def analytic_views(n, H, W, focal, first, n_ref=256):
    """(o, d, viewdirs, rgb) of n views of the analytic scene of tests/teacher_util.py on the r = 4 sphere, each [n*H*W,3] on the GPU:
    the target is the volume render of analytic_targets at n_ref even depths in [2, 6] on white (O.raw2outputs, fp32)."""
    from r2l_amd.render import get_rays
    from tests.teacher_util import analytic_targets
    out = [[], [], [], []]
    t = torch.linspace(0., 1., n_ref, device="cuda")
    for k in range(first, first + n):
        c2w = torch.from_numpy(O.pose_spherical(-180. + 47. * k, -20. - 25. * (k % 3), 4.)[:3, :4])
        ro, rd = [x.reshape(-1, 3).float().cuda() for x in get_rays(H, W, focal, c2w)]
        vd = rd / rd.norm(dim=-1, keepdim=True)
        z = (2. * (1. - t) + 6. * t).expand(ro.shape[0], n_ref)
        pts = ro[:, None] + rd[:, None] * z[..., None]
        with torch.device("cuda"):
            rgb_l, sig = analytic_targets(pts.reshape(-1, 3), vd[:, None].expand(-1, n_ref, 3).reshape(-1, 3))
            raw = torch.cat([rgb_l, sig[:, None]], -1).view(ro.shape[0], n_ref, 4)
            rgb = O.raw2outputs(raw, z, rd, None, True)[0]
        for lst, v in zip(out, (ro, rd, vd, rgb)):
            lst.append(v)
    return [torch.cat(v) for v in out]


class ListLog:
    def __init__(self):
        self.lines = []

    def info(self, *a):
        self.lines.append(" ".join(str(x) for x in a))


def occ(a):
    import re
    from r2l_amd import render
    from r2l_amd.occupancy import OccupancyGrid, TrainOccupancy, pack_bits
    from r2l_amd.teacher_train import TeacherTrainer
    from tests.teacher_util import scene_rays, trained_like_pair
    lines = ["teacher training on the live samples of occupancy grids (TeacherTrainer.set_occupancy; r2l_teacher_mlp_train_live / "
             "r2l_teacher_backward_live / r2l_teacher_train_step_occ) against the plain step of the same process; trained-like pair, "
             "%d rays of scene_rays' camera over its frame, 64 + 128 samples, perturb 1, lr 0; %s; steps %d, warmup %d, %d alternating "
             "rounds; wall-clock ms per step, one synchronisation after the steps of a round"
             % (a.rays, torch.cuda.get_device_name(0), a.steps, a.warmup, a.repeats)]

    def emit(r):
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)

    csd, fsd = trained_like_pair()
    R = a.rays
    rb = scene_rays(181 * 181, 0)[torch.randperm(181 * 181, generator=torch.Generator().manual_seed(0))[:R]].cuda()
    o, d, vd = rb[:, 0:3].contiguous(), rb[:, 3:6].contiguous(), rb[:, 8:11].contiguous()
    tgt = torch.rand(R, 3, generator=torch.Generator().manual_seed(1)).cuda()
    tr = TeacherTrainer(make(csd), make(fsd), perturb=1., white_bkgd=True)
    hist = torch.zeros(a.warmup + a.steps, 2, device="cuda")
    it = [0]

    def fused_step():
        it[0] += 1
        tr.fused_step(o, d, vd, 2., 6., tgt, 0., step=it[0], seed=0, loss_out=hist[it[0] % hist.shape[0]])

    def staged_step():
        tr.step(o, d, vd, 2., 6., tgt, 0.)

    def grids(box, G):
        return tuple(OccupancyGrid([-box] * 3, [box] * 3, G=G, k=2, dilate=1, precision="fp32_mfma").build(net) for net in tr.nets)

    def ones():
        return OccupancyGrid([-1.] * 3, [1.] * 3, G=4, k=1, dilate=0).set_bits(pack_bits(np.ones((4, 4, 4), dtype=bool)), device="cuda")

    pairs = [("plain", None), ("box1.6", grids(1.6, 128)), ("box2.5", grids(2.5, 128)), ("all_ones", (ones(), ones()))]
    got = {(name, kind): [] for name, _ in pairs for kind in ("staged", "fused")}
    share = {}
    for _ in range(a.repeats):
        for name, pair in pairs:
            tr.set_occupancy(pair)
            for kind, fn in (("staged", staged_step), ("fused", fused_step)):
                tr.live_acc.zero_()
                it[0] = 0
                got[(name, kind)].append(round(wall(fn, a.steps, a.warmup, sync_each=False), 3))
                hist.tolist()
                lv, tot = tr.live_acc.tolist()
                share[name] = round(lv / tot, 4) if tot else 1.
    tr.set_occupancy(None)
    med = {k: float(np.median(v)) for k, v in got.items()}
    for name, pair in pairs:
        r = {"grids": name, "rays": R, "points": R * 256, "live_share": share[name]}
        if pair is not None and name != "all_ones":
            r["occupied_share"] = [round(g.occupied_share(), 4) for g in pair]
        for kind in ("staged", "fused"):
            r[kind + "_ms"] = got[(name, kind)]
            r[kind + "_median_ms"] = med[(name, kind)]
            r[kind + "_spread_ms"] = round(max(got[(name, kind)]) - min(got[(name, kind)]), 3)
            r[kind + "_over_plain"] = round(med[(name, kind)] / med[("plain", kind)], 4)
        emit(r)
    # refresh cost
    plain_ms = med[("plain", "fused")]
    for G in (64, 128):
        secs = []
        gs = grids(1.6, G)
        for _ in range(5):
            secs.append([g.rebuild(net).build_seconds for g, net in zip(gs, tr.nets)])
        per_grid = float(np.median([s for row in secs for s in row]))
        K = 1
        while 2. * per_grid * 1e3 > 0.02 * K * plain_ms:
            K *= 2
        emit({"rebuild": "exact fp32, %d^3 cells, 2 probes per cell and axis, dilation 1, box +-1.6" % G, "probes": (2 * G)**3,
              "rebuild_ms_per_grid": round(per_grid * 1e3, 2), "all_ms": [[round(x * 1e3, 2) for x in row] for row in secs],
              "plain_fused_step_ms": plain_ms, "smallest_power_of_two_K_with_two_rebuilds_at_most_2_percent": K,
              "share_of_a_window_at_that_K": round(2. * per_grid * 1e3 / (K * plain_ms), 4)})
    del tr
    if a.effect_iters > 0:
        H = W = 64
        focal = 100.
        train = analytic_views(20, H, W, focal, 0)
        held = analytic_views(4, H, W, focal, 100)
        n_train = train[0].shape[0]
        N_rand, NS, NI = 1024, 32, 64

        def run(seed, every):
            sds = O.make_teacher_state_dicts(seed, 2, alpha_bias=0.5)
            t = TeacherTrainer(make(sds[0]), make(sds[1]), N_samples=NS, N_importance=NI, perturb=1., white_bkgd=True)
            log = ListLog()
            oc = None
            if every:
                args = argparse.Namespace(r2l_occ_every=every, r2l_occ_res=128, r2l_occ_bound=1.6)
                oc = TrainOccupancy(args, t.nets[0], t.nets[1], 2., 6., t, log, start=0)
            g = torch.Generator(device="cuda").manual_seed(seed)
            loss = torch.zeros(2, device="cuda")
            t0 = time.perf_counter()
            for i in range(1, a.effect_iters + 1):
                sel = torch.randint(0, n_train, (N_rand,), generator=g, device="cuda")
                t.fused_step(train[0][sel], train[1][sel], train[2][sel], 2., 6., train[3][sel], 5e-4, step=i, seed=seed, loss_out=loss)
                if oc is not None:
                    oc.after_step(i)
            torch.cuda.synchronize()
            secs = time.perf_counter() - t0
            t.set_occupancy(None)
            ones_ = torch.ones(held[0].shape[0], 1, device="cuda")
            batch = torch.cat([held[0], held[1], 2. * ones_, 6. * ones_, held[2]], -1)
            with torch.no_grad():
                rgb = torch.cat([render.render_rays(batch[k:k + 4096], t.nets[0], None, NS, perturb=0., N_importance=NI, network_fine=t.nets[1],
                                                    white_bkgd=True)["rgb_map"] for k in range(0, batch.shape[0], 4096)])
            psnr = float(-10. * torch.log10(torch.mean((rgb - held[3])**2)))
            r = {"effect_run": "grids every %d" % every if every else "plain", "seed": seed, "iterations": a.effect_iters, "N_rand": N_rand,
                 "samples": "%d + %d" % (NS, NI), "train_loss_last": round(float(loss[0]), 5), "held_out_psnr": round(psnr, 3),
                 "seconds": round(secs, 1)}
            if oc is not None:
                ref = [l for l in log.lines if "refresh after iteration" in l]
                r["newly_set_cells_per_refresh"] = [int(re.search(r"(\d+) cells set now", l).group(1)) for l in ref]
                r["live_share_per_window"] = [float(re.search(r"\(([0-9.]+)%\) in the window", l).group(1)) / 100 for l in ref]
            emit(r)
            return psnr

        p0 = run(0, 0)
        p1 = run(1, 0)
        pk = {K: run(0, K) for K in a.effect_every}
        emit({"effect": "held-out PSNR, grids minus plain (same seed)", "by_K": {str(K): round(v - p0, 3) for K, v in pk.items()},
              "seed_spread_of_the_plain_run": round(abs(p0 - p1), 3)})
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
    ap.add_argument("--occ", action="store_true", help="time the step on the live samples of occupancy grids (--r2l_occ_train) against "
                    "the plain step, the grids' refresh, and the effect on a trained result")
    ap.add_argument("--effect_iters", type=int, default=3000, help="--occ: iterations of each training run of the effect part (0: skip it)")
    ap.add_argument("--effect_every", type=int, nargs="+", default=[64, 1024], help="--occ: the refresh intervals of the runs with grids")
    ap.add_argument("--repeats", type=int, default=3, help="--fused / --images / --occ: timed runs per path")
    ap.add_argument("--out", default=None, help="where --batching / --fused / --images write their lines (default: "
                    "profiles/teacher_batching.txt / profiles/teacher_fused_step.txt / profiles/teacher_image_sampler.txt)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "teacher_train_time needs the GPU"
    if a.out is None:
        a.out = os.path.join("profiles", "teacher_occ_train.txt" if a.occ else "teacher_image_sampler.txt" if a.images else
                             "teacher_fused_step.txt" if a.fused else "teacher_batching.txt")
    if a.occ:
        return occ(a)
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
