"""What ranking the hard rays in the library buys (--r2l_device_pool; include/r2l_hip.h r2l_pool_select), on one GPU, in one
process, after warm-up; both paths alternately for `--rounds` rounds, so that the spread between two runs of the same path is seen
next to the difference between the paths.

  (a) HardRayPool.update on a full pool (hard_ratio 0.2, hard_mul 20), the default path (a torch sort of all B errors) against
      device_select=True (r2l_pool_select + r2l_pool_store), at B = 4096, 12 288 and 81 920: device events around 200 updates.
  (b) the whole iteration RayStore.next -> augment -> step -> update on W256 D88 at --N_rand 1, 3 and 20, without and with the
      switch (device ranking + Philox jitter): a host clock around 300 iterations that end in a synchronise.

`python tools/pool_select_time.py --out profiles/pool_select.txt`"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from r2l_amd import render  # noqa: E402
from r2l_amd.driver import HardRayPool  # noqa: E402
from r2l_amd.raystore import RayStore  # noqa: E402
from r2l_amd.train_step import R2LTrainer  # noqa: E402


def _rows(n, seed):
    g = torch.Generator().manual_seed(seed)
    o = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1) * 4.
    d = -o / 4. + 0.2 * torch.randn(n, 3, generator=g)
    return torch.cat([o, d, torch.rand(n, 3, generator=g)], 1)


def _full_pool(B, device_select, rows, rgb):
    pool = HardRayPool(0.2, 20., seed=1, device_select=device_select)
    o, d, t = rows[:B, :3], rows[:B, 3:6], rows[:B, 6:9]
    while not pool.full:
        pool.update(rgb[:B], o, d, t, B)
    return pool


def time_updates(B, rounds, n_updates, say):
    rows = _rows(B, B).cuda()
    rgb = torch.rand(B + int(0.2 * B), 3, device="cuda")
    pools = {name: _full_pool(B, sel, rows, rgb) for name, sel in (("default", False), ("device", True))}
    batches = {name: p.augment(rows[:, :3], rows[:, 3:6], rows[:, 6:9]) for name, p in pools.items()}
    got = {name: [] for name in pools}
    for r in range(rounds + 1):  # round 0: warm-up, not reported
        for name, pool in pools.items():
            o, d, t = batches[name]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n_updates):
                pool.update(rgb, o, d, t, B)
            b.record()
            b.synchronize()
            if r:
                got[name].append(a.elapsed_time(b) * 1e3 / n_updates)
    spread = max(got["default"]) - min(got["default"])
    say("update  B %6d  k %5d | default %s us (spread %.2f) | device_select %s us (spread %.2f) | x%.2f" %
        (B, int(0.2 * B), " ".join("%7.2f" % v for v in got["default"]), spread, " ".join("%7.2f" % v for v in got["device"]),
         max(got["device"]) - min(got["device"]), np.median(got["default"]) / np.median(got["device"])))
    ok = np.median(got["device"]) <= np.median(got["default"]) + spread
    say("        condition (device not slower than default by more than the default's spread): %s" % ("met" if ok else "NOT met"))
    return got


def time_iterations(n_rand, rounds, n_iter, trainer, ps, say):
    store = RayStore(40, "cuda", seed=5)
    store.append(_rows(40 * 4096, 7).cuda(), 1)
    B = n_rand * 4096
    got = {"default": [], "switch": []}
    pools = {"default": HardRayPool(0.2, 20., seed=1), "switch": HardRayPool(0.2, 20., seed=1, device_select=True)}
    it = {"default": 0, "switch": 0}

    def run(name, n):
        pool = pools[name]
        for _ in range(n):
            it[name] += 1
            batch = store.next(n_rand)
            o, d, t = pool.augment(batch[:, :3], batch[:, 3:6], batch[:, 6:9])
            t_rand = None
            if name == "switch":
                t_rand = render.draw_uniform(o.shape[0] * 16, 0, 2**61 + it[name] * 4096, "cuda").view(-1, 16)
            rgb, _ = trainer.step(o, d, t, 1e-5, perturb=1., t_rand=t_rand)
            pool.update(rgb, o, d, t, B)
        torch.cuda.synchronize()

    for name in pools:  # fill the pools (100 updates) and warm up
        run(name, 110)
    for _ in range(rounds):
        for name in pools:
            t0 = time.perf_counter()
            run(name, n_iter)
            got[name].append((time.perf_counter() - t0) * 1e3 / n_iter)
    store.close()
    say("iteration  N_rand %2d (%6d + %5d rays) | default %s ms | --r2l_device_pool %s ms | x%.3f" %
        (n_rand, B, int(0.2 * B), " ".join("%7.3f" % v for v in got["default"]), " ".join("%7.3f" % v for v in got["switch"]),
         np.median(got["default"]) / np.median(got["switch"])))
    return got


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("# tools/pool_select_time.py on %s, torch %s; one process, %d rounds alternating the two paths" %
        (torch.cuda.get_device_name(0), torch.__version__, a.rounds))
    say("# (a) HardRayPool.update on a full pool, hard_ratio 0.2, hard_mul 20: us per update, device events around %d updates" % a.updates)
    for B in (4096, 12288, 81920):
        time_updates(B, a.rounds, a.updates, say)
    from model.nerf_raybased import PointSampler
    from oracle import r2l_oracle as O
    from tests.test_forward_gpu import build_model
    say("# (b) RayStore.next -> augment -> step -> update, W256 D88, default arithmetic: ms per iteration, host clock around %d "
        "iterations ending in a synchronise" % a.iters)
    model = build_model(O.make_state_dict(n_block=43, seed=0), 43)
    ps = PointSampler(400, 400, 555.5555155968841, 16, 2., 6.)
    trainer = R2LTrainer(model, ps)
    for n_rand in (1, 3, 20):
        time_iterations(n_rand, a.rounds, a.iters, trainer, ps, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
