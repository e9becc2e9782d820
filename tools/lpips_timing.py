"""Time of the fused LPIPS kernels per 400x400 pair at one pair per launch and at the launch size the driver picks, and of the same
pairs through the op-by-op torch evaluation (F.conv2d / F.max_pool2d / elementwise) on the same GPU after warm-up.

    python tools/lpips_timing.py [iterations] [--net alex|vgg]

--net alex (default): r2l_lpips against metrics._lpips_torch at 1 and 9 pairs; 8.79 GFLOP per pair.
--net vgg: r2l_lpips_vgg against metrics._lpips_vgg_torch at 1 pair and at driver.lpips_vgg_frames_per_launch(400, 400) pairs;
about 196 GFLOP per pair (the thirteen convolutions of both images, computed from lpips_vgg_sizes).

Device events around `iterations` back-to-back calls; three rounds that alternate the two paths, the median and all three windows
are printed.  The weights are seeded synthetic ones: the time depends on the shapes alone.  The FLOPs are the algorithmic ones
(2 per multiply-add of the convolutions) against the 157.3 TFLOP/s fp32-MFMA peak; the call includes the prologue, pool, slab
reduce, distance and finish kernels."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from r2l_amd import driver, metrics  # noqa: E402
from tools.e2e_render import lpips_vgg_weights, lpips_weights  # noqa: E402

PEAK_TFLOPS = 157.3


def pair_flops(H, W):
    return 2 * sum(2 * ho * wo * co * ci * k * k for (ho, wo), (ci, co, k, _, _) in zip(metrics.lpips_sizes(H, W), metrics.LPIPS_CONVS))


def pair_flops_vgg(H, W):
    sizes = metrics.lpips_vgg_sizes(H, W)
    stage = [sum(l >= p for p in (2, 4, 7, 10)) for l in range(13)]
    return 2 * sum(2 * sizes[s][0] * sizes[s][1] * co * ci * 9 for s, (ci, co) in zip(stage, metrics.LPIPS_VGG_CONVS))


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n  # us per call


def main(n=None, net="alex"):
    dev = torch.device("cuda")
    if net == "vgg":
        params, flops, name = lpips_vgg_weights("random", dev), pair_flops_vgg(400, 400), "r2l_lpips_vgg"
        fused_fn, torch_fn, ks = metrics.lpips_vgg, metrics._lpips_vgg_torch, (1, driver.lpips_vgg_frames_per_launch(400, 400))
        n = n or 20
        from r2l_amd import _lib
        for hw in (400, 800):
            print("work buffer of one %dx%d pair: %.1f MB" % (hw, hw, 4e-6 * _lib.load().r2l_lpips_vgg_work_floats(1, hw, hw)))
    else:
        params, flops, name = lpips_weights("random", dev), pair_flops(400, 400), "r2l_lpips"
        fused_fn, torch_fn, ks = metrics.lpips, metrics._lpips_torch, (1, 9)
        n = n or 200
    print("400x400: %.3f GFLOP per pair" % (flops * 1e-9))
    g = torch.Generator().manual_seed(3)
    for K in ks:
        a = (2 * torch.rand(K, 400, 400, 3, generator=g) - 1).to(dev)
        b = (2 * torch.rand(K, 400, 400, 3, generator=g) - 1).to(dev)
        fused = lambda: fused_fn(a, b, params)
        unfused = lambda: torch_fn(a, b, params)
        paths = (("fused " + name, fused, n), ("op-by-op torch", unfused, max(n // 4, 5)))
        with torch.no_grad():
            want, got = unfused()[0].sum(1), fused()
            print("K = %d: fused against op-by-op torch on the device, max relative difference %.2e" %
                  (K, ((got - want).abs() / want).max().item()))
            for _, fn, _ in paths:
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            us = {tag: [] for tag, _, _ in paths}
            for _ in range(3):  # the rounds alternate the two paths
                for tag, fn, it in paths:
                    us[tag].append(window(fn, it))
            for tag, _, _ in paths:
                w = sorted(us[tag])
                per_pair = w[1] / K
                print("K = %d %-20s: %9.1f us per call (rounds %s), %8.1f us per pair = %.1f TFLOP/s = %.1f %% of the %.1f TFLOP/s "
                      "fp32-MFMA peak" % (K, tag, w[1], " ".join("%.1f" % u for u in us[tag]), per_pair, flops / per_pair * 1e-6,
                                          100 * flops / per_pair * 1e-6 / PEAK_TFLOPS, PEAK_TFLOPS))


if __name__ == "__main__":
    which = "alex"
    if "--net" in sys.argv:
        at = sys.argv.index("--net")
        which = sys.argv[at + 1]
        del sys.argv[at:at + 2]
    assert which in ("alex", "vgg"), which
    main(int(sys.argv[1]) if len(sys.argv) > 1 else None, which)
