"""What an iteration of pose refinement costs (r2l_amd/pose_refine.py, r2l_pose_refine_step), on one GPU, in one process, after
warm-up: W256 D88, the default kernel family and fp32_mfma, (P, n) = (1, 4096), (3, 4096), (24, 4096), 400 x 400 images.

  fused    PoseRefiner.fused_step: one r2l_pose_refine_step call per iteration
  staged   PoseRefiner.step: the same kernels, every library call made from Python
  torch    the route a user has without it, on the same GPU: pose = (matrix_exp([w]x) R0, t0 + v) and its rays in torch,
           model.forward_rays through autograd (R2LRaysFunction: the same forward, dX chain and input-gradient kernels), the
           reductions by autograd, torch.optim.Adam on (w, v); the pixels of an iteration by torch.randint on the device

alternately for `--rounds` rounds (the order rotates from round to round) of `--iters` iterations each, enqueued back to back and synchronised once: ms per iteration by
device events around the round and by the wall clock around it.  Reported: every round, the medians, the spread between the runs
of the same path, and fused against torch.  Then r2l_pose_grad alone against the 60 bytes a ray it moves.

`python tools/pose_refine_time.py --out profiles/pose_refine.txt`"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from r2l_amd import _lib  # noqa: E402
from r2l_amd.engine import _ptr, _stream  # noqa: E402
from r2l_amd.pose_refine import PoseRefiner  # noqa: E402

PATHS = ("fused", "staged", "torch")
H = W = 400
FOCAL = 555.5555155968841


def poses(P, seed):
    g = torch.Generator().manual_seed(seed)
    w = 0.1 * torch.randn(P, 3, generator=g, dtype=torch.float64)
    K = torch.zeros(P, 3, 3, dtype=torch.float64)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    t = torch.tensor([0., 0., 4.], dtype=torch.float64) + 0.2 * torch.randn(P, 3, generator=g, dtype=torch.float64)
    return torch.cat([torch.matrix_exp(K), t[:, :, None]], -1).float()


class TorchRoute:
    """The hand-rolled loop: everything but the student's kernels is torch."""

    def __init__(self, model, ps, images, init, n, lr_rot=2e-3, lr_trans=5e-3):
        self.model, self.ps, self.n, self.P = model, ps, n, init.shape[0]
        self.dev = dev = next(model.parameters()).device
        self.images = images.to(dev).reshape(self.P, H * W, 3)
        self.R0, self.t0 = init[:, :, :3].to(dev).contiguous(), init[:, :, 3].to(dev).contiguous()
        self.w = torch.zeros(self.P, 3, device=dev, requires_grad=True)
        self.v = torch.zeros(self.P, 3, device=dev, requires_grad=True)
        self.opt = torch.optim.Adam([{"params": [self.w], "lr": lr_rot}, {"params": [self.v], "lr": lr_trans}])
        self.dirs = ps.dirs.reshape(-1, 3)
        self.losses = []

    def step(self):
        P, n = self.P, self.n
        pix = torch.randint(0, H * W, (P, n), device=self.dev)
        w = self.w
        zero = torch.zeros_like(w[:, 0])
        K = torch.stack([zero, -w[:, 2], w[:, 1], w[:, 2], zero, -w[:, 0], -w[:, 1], w[:, 0], zero], -1).reshape(P, 3, 3)
        R, t = torch.matmul(torch.matrix_exp(K), self.R0), self.t0 + self.v
        d = torch.matmul(self.dirs[pix], R.transpose(1, 2)).reshape(P * n, 3)
        o = t[:, None, :].expand(P, n, 3).reshape(P * n, 3)
        rgb = self.model.forward_rays(o, d, self.ps, perturb=0.)
        target = torch.gather(self.images, 1, pix[:, :, None].expand(P, n, 3)).reshape(P * n, 3)
        loss = ((rgb - target) ** 2).reshape(P, -1).mean(-1)
        self.opt.zero_grad(set_to_none=True)
        loss.sum().backward()
        self.opt.step()
        self.losses.append(loss.detach())


def time_round(step, n_iter):
    """(ms per iteration by device events, by the wall clock) of n_iter iterations enqueued back to back."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(n_iter):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n_iter, (time.perf_counter() - t0) * 1e3 / n_iter


def time_size(P, n, model, ps, rounds, n_iter, say):
    g = torch.Generator().manual_seed(P)
    images = torch.rand(P, H, W, 3, generator=g)
    init = poses(P, 3 + P)
    fused, staged = PoseRefiner(model, ps, images, init, n), PoseRefiner(model, ps, images, init, n)
    route = TorchRoute(model, ps, images, init, n)
    steps = {"fused": fused.fused_step, "staged": staged.step, "torch": route.step}
    for k in PATHS:  # warm up every path at this size
        time_round(steps[k], 3)
    got = {k: [] for k in PATHS}
    for r in range(rounds):
        for k in PATHS[r % 3:] + PATHS[:r % 3]:  # every path goes first, second and third once in three rounds
            got[k].append(time_round(steps[k], n_iter))
            fused._loss_rows, staged._loss_rows, route.losses = [], [], []
    say("P %2d n %d (N %6d)" % (P, n, P * n))
    med = {}
    for k in PATHS:
        ev, wall = [a for a, _ in got[k]], [b for _, b in got[k]]
        med[k] = (float(np.median(ev)), float(np.median(wall)))
        say("    %-7s events %s ms | median %.4f, spread %.4f | wall %s ms | median %.4f, spread %.4f" % (
            k, " ".join("%8.4f" % x for x in ev), med[k][0], max(ev) - min(ev), " ".join("%8.4f" % x for x in wall), med[k][1],
            max(wall) - min(wall)))
    say("    torch / fused x%.2f by events, x%.2f by the wall clock; staged / fused x%.2f, x%.2f" % (
        med["torch"][0] / med["fused"][0], med["torch"][1] / med["fused"][1], med["staged"][0] / med["fused"][0],
        med["staged"][1] / med["fused"][1]))
    return fused


def time_pose_grad(r, rounds, say):
    """r2l_pose_grad alone on the buffers a refiner's step left, 50 calls per round between two events."""
    lib, (_, w) = r.lib, r._buffers()
    loss = torch.empty(r.P, device="cuda")
    call = lambda: _lib.check(lib.r2l_pose_grad(_ptr(w["rays_d"]), _ptr(w["d_rays_o"]), _ptr(w["d_rays_d"]), _ptr(w["rgb"]),
                                                _ptr(w["target"]), r.P, r.n, _ptr(w["grad"]), _ptr(loss), _ptr(w["pose_grad"]),
                                                _stream()), "r2l_pose_grad")
    time_round(call, 10)
    us = [time_round(call, 50)[0] * 1e3 for _ in range(rounds)]
    m = float(np.median(us))
    say("    r2l_pose_grad alone (%d launches) %s us | median %.2f, spread %.2f | %.1f MB at 60 B a ray: %.0f GB/s" % (
        1 if r.n <= 256 else (2 if r.n <= 16384 else 3), " ".join("%7.2f" % x for x in us), m, max(us) - min(us), r.N * 60 / 1e6,
        r.N * 60 / (m * 1e-6) / 1e9))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sizes", default="1x4096,3x4096,24x4096")
    ap.add_argument("--n_block", type=int, default=43)
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    from model.nerf_raybased import PointSampler
    from oracle import r2l_oracle as O
    from tests.test_forward_gpu import build_model
    say("# tools/pose_refine_time.py on %s, torch %s; one process, %d rounds of %d iterations alternating the paths; ms per iteration" %
        (torch.cuda.get_device_name(0), torch.__version__, a.rounds, a.iters))
    for precision in ("auto", "fp32_mfma"):
        model = build_model(O.make_state_dict(n_block=a.n_block, seed=0), a.n_block)
        for p in model.parameters():
            p.requires_grad_(False)
        model.engine().set_config(precision=precision)
        ps = PointSampler(H, W, FOCAL, 16, 2., 6.)
        say("# W256 D%d, precision %s, %d x %d images" % (2 * a.n_block + 2, precision, H, W))
        for size in a.sizes.split(","):
            P, n = (int(v) for v in size.split("x"))
            time_pose_grad(time_size(P, n, model, ps, a.rounds, a.iters, say), a.rounds, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
