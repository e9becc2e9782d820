"""What running the student's iteration as ONE library call buys (--r2l_fused_iter; include/r2l_hip.h r2l_student_train_step), on
one GPU, in one process, after warm-up: the whole iteration on W256 D88 at --N_rand 1, 3 and 20 (hard_ratio 0.2, hard_mul 20, full
pool, perturb 1),

  staged  RayStore.next -> HardRayPool.augment -> draw_uniform -> R2LTrainer.step -> HardRayPool.update  (the --r2l_device_store
          --r2l_device_pool loop: the "switch" path of tools/pool_select_time.py)
  fused   R2LTrainer.fused_step: r2l_student_train_step

alternately for `--rounds` rounds, a host clock around `--iters` iterations that end in a synchronise.  Reported: every round, the
medians, and the spread between the runs of the same path; the condition is "fused not slower than staged by more than the staged
path's spread".  Both paths compute the same bits (tests/test_student_step_gpu.py).

`python tools/student_iter_time.py --out profiles/student_fused_iter.txt`"""
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


def time_iterations(n_rand, rounds, n_iter, trainer, say):
    store = RayStore(40, "cuda", seed=5)
    store.append(_rows(40 * 4096, 7).cuda(), 1)
    B = n_rand * 4096
    paths = ("staged", "fused")
    got = {name: [] for name in paths}
    pools = {name: HardRayPool(0.2, 20., seed=1, device_select=True) for name in paths}
    it = {name: 0 for name in paths}

    def run(name, n):
        pool = pools[name]
        for _ in range(n):
            it[name] += 1
            if name == "fused":
                trainer.fused_step(store, pool, 1e-5, it[name], perturb=1., seed=0, n_files=n_rand)
                continue
            batch = store.next(n_rand)
            o, d, t = pool.augment(batch[:, :3], batch[:, 3:6], batch[:, 6:9])
            t_rand = render.draw_uniform(o.shape[0] * 16, 0, 2**61 + it[name] * 4096, "cuda").view(-1, 16)
            rgb, _ = trainer.step(o, d, t, 1e-5, perturb=1., t_rand=t_rand)
            pool.update(rgb, o, d, t, B)
        torch.cuda.synchronize()

    for name in paths:  # fill the pools (100 updates) and warm up
        run(name, 110)
        assert pools[name].full
    for _ in range(rounds):
        for name in paths:
            t0 = time.perf_counter()
            run(name, n_iter)
            got[name].append((time.perf_counter() - t0) * 1e3 / n_iter)
    store.close()
    med = {name: float(np.median(got[name])) for name in paths}
    spread = {name: max(got[name]) - min(got[name]) for name in paths}
    say("iteration  N_rand %2d (%6d + %5d rays) | staged %s ms (median %.3f, spread %.3f) | fused %s ms (median %.3f, spread %.3f) | "
        "x%.3f, %+.1f us" % (n_rand, B, int(0.2 * B), " ".join("%7.3f" % v for v in got["staged"]), med["staged"], spread["staged"],
                             " ".join("%7.3f" % v for v in got["fused"]), med["fused"], spread["fused"], med["staged"] / med["fused"],
                             (med["fused"] - med["staged"]) * 1e3))
    ok = med["fused"] <= med["staged"] + spread["staged"]
    say("        condition (fused not slower than staged by more than the staged path's spread): %s" % ("met" if ok else "NOT met"))
    return got


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    from model.nerf_raybased import PointSampler
    from oracle import r2l_oracle as O
    from tests.test_forward_gpu import build_model
    say("# tools/student_iter_time.py on %s, torch %s; one process, %d rounds alternating the two paths" %
        (torch.cuda.get_device_name(0), torch.__version__, a.rounds))
    say("# the whole iteration, W256 D88, default arithmetic, hard_ratio 0.2, hard_mul 20 (full pool), perturb 1: ms per iteration, host "
        "clock around %d iterations ending in a synchronise" % a.iters)
    model = build_model(O.make_state_dict(n_block=43, seed=0), 43)
    trainer = R2LTrainer(model, PointSampler(400, 400, 555.5555155968841, 16, 2., 6.))
    for n_rand in (1, 3, 20):
        time_iterations(n_rand, a.rounds, a.iters, trainer, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
