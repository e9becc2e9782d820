"""Time of the fused LPIPS kernels (r2l_lpips) per 400x400 pair at 1 and at 9 pairs per launch, and of the same pairs through the
op-by-op torch evaluation (metrics._lpips_torch: F.conv2d / F.max_pool2d / elementwise) on the same GPU after warm-up.

    python tools/lpips_timing.py [iterations]

Device events around `iterations` back-to-back calls, three windows each (the spread is printed).  The weights are seeded
synthetic ones: the time depends on the shapes alone.  8.79 GFLOP per pair (the five convolutions of both images) against the
157.3 TFLOP/s fp32-MFMA peak gives the share of peak; the call includes the pool, distance and finish kernels."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from r2l_amd import metrics  # noqa: E402
from tools.e2e_render import lpips_weights  # noqa: E402

PEAK_TFLOPS = 157.3


def pair_flops(H, W):
    return 2 * sum(2 * ho * wo * co * ci * k * k for (ho, wo), (ci, co, k, _, _) in zip(metrics.lpips_sizes(H, W), metrics.LPIPS_CONVS))


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n  # us per call


def main(n=200):
    dev = torch.device("cuda")
    params = lpips_weights("random", dev)
    flops = pair_flops(400, 400)
    print("400x400: %.3f GFLOP per pair" % (flops * 1e-9))
    g = torch.Generator().manual_seed(3)
    for K in (1, 9):
        a = (2 * torch.rand(K, 400, 400, 3, generator=g) - 1).to(dev)
        b = (2 * torch.rand(K, 400, 400, 3, generator=g) - 1).to(dev)
        fused = lambda: metrics.lpips(a, b, params)
        unfused = lambda: metrics._lpips_torch(a, b, params)
        with torch.no_grad():
            want, got = unfused()[0].sum(1), fused()
            print("K = %d: fused against op-by-op torch on the device, max relative difference %.2e" %
                  (K, ((got - want).abs() / want).max().item()))
            for tag, fn, it in (("fused r2l_lpips", fused, n), ("op-by-op torch", unfused, max(n // 4, 10))):
                for _ in range(5):
                    fn()
                torch.cuda.synchronize()
                us = sorted(window(fn, it) for _ in range(3))
                per_pair = us[1] / K
                print("K = %d %-16s: %9.1f us per call (windows %s), %8.1f us per pair = %.1f TFLOP/s = %.1f %% of the %.1f TFLOP/s "
                      "fp32-MFMA peak" % (K, tag, us[1], " ".join("%.1f" % u for u in us), per_pair, flops / per_pair * 1e-6,
                                          100 * flops / per_pair * 1e-6 / PEAK_TFLOPS, PEAK_TFLOPS))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200)
