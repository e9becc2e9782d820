"""Wall-clock of the test-set evaluation loop (driver.render_path: render + PSNR + SSIM + FLIP + PNG writing of prediction and
ground truth) on 40 synthetic 400x400 views, W256 D88.

    python tools/e2e_render.py [n_frames] [noise] [--lpips_weights PATH|random] [--lpips_vgg_weights PATH|random]

--lpips_weights adds LPIPS to the loop (driver.render_path(lpips_params=)): PATH as --r2l_lpips_weights takes it, or `random`
for seeded synthetic weights (the time depends on the shapes alone; the printed value then means nothing).
--lpips_vgg_weights does the same for the VGG-16 variant (lpips_vgg_params=, --r2l_lpips_vgg_weights)."""
import argparse
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from model.nerf_raybased import NeRF_v3_2, PointSampler  # noqa: E402
from r2l_amd import data, driver  # noqa: E402


class _Log:
    def info(self, *a):
        if "frames in" in str(a[0]):
            print(*a)


def lpips_weights(spec, dev):
    from r2l_amd import metrics
    if spec is None:
        return None
    if spec != "random":
        return metrics.lpips_params(spec).to(dev)
    g = torch.Generator().manual_seed(7)
    convs = [(torch.randn(co, ci, k, k, generator=g) * (2. / (ci * k * k))**0.5, 0.1 * torch.randn(co, generator=g))
             for ci, co, k, _, _ in metrics.LPIPS_CONVS]
    return metrics.lpips_flatten(convs, [torch.randn(c[1], generator=g).abs() / c[1] for c in metrics.LPIPS_CONVS]).to(dev)


def lpips_vgg_weights(spec, dev):
    from r2l_amd import metrics
    if spec is None:
        return None
    if spec != "random":
        return metrics.lpips_vgg_params(spec).to(dev)
    g = torch.Generator().manual_seed(7)
    convs = [(torch.randn(co, ci, 3, 3, generator=g) * (2. / (ci * 9))**0.5, 0.1 * torch.randn(co, generator=g))
             for ci, co in metrics.LPIPS_VGG_CONVS]
    lins = [torch.randn(metrics.LPIPS_VGG_CONVS[t][1], generator=g).abs() / metrics.LPIPS_VGG_CONVS[t][1] * 4.**l
            for l, t in enumerate(metrics.LPIPS_VGG_TAPS)]
    return metrics.lpips_vgg_flatten(convs, lins).to(dev)


def main(n=40, lpips=None, lpips_vgg=None):
    dev = torch.device("cuda")
    lp, lpv = lpips_weights(lpips, dev), lpips_vgg_weights(lpips_vgg, dev)
    trial = argparse.Namespace(ON=True, body_arch="resmlp", inact="relu", outact="none", res_scale=1., n_learnable=2,
                               n_block=-1, near=-1, far=-1)
    args = argparse.Namespace(netdepth=88, netwidth=256, layerwise_netwidths="", act="relu", linear_tail=False,
                              use_residual=True, trial=trial)
    torch.manual_seed(0)
    net = NeRF_v3_2(args, 1008, 3).to(dev)
    ps = PointSampler(400, 400, 555.5555155968841, 16, 2., 6., device=dev)
    poses = torch.stack([data.pose_spherical(-180. + 9. * i, -30., 4.) for i in range(n)]).to(dev)
    # ground-truth frames: smooth images (bilinear upsampling of 25x25 noise; real test frames — an object on a white
    # background — compress at least as well) or, `noise`, incompressible ones: zlib's worst case, 10x the encode time
    if len(sys.argv) > 2 and sys.argv[2] == "noise":
        gts = torch.rand(n, 400, 400, 3)
    else:
        gts = torch.nn.functional.interpolate(torch.rand(n, 3, 25, 25), size=400, mode="bilinear").permute(0, 2, 3, 1).contiguous()
    out = tempfile.mkdtemp(prefix="r2l_frames_")
    for tag, sd in (("metrics only", None), ("metrics + PNGs", out)):
        driver.render_path(poses[:3], net, ps, dev, _Log(), gt_imgs=gts[:3], savedir=None, lpips_params=lp,
                           lpips_vgg_params=lpv)  # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, misc = driver.render_path(poses, net, ps, dev, _Log(), gt_imgs=gts, savedir=sd, lpips_params=lp, lpips_vgg_params=lpv)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print("%-15s: %.1f ms/frame (%d frames, psnr %.3f ssim %.4f flip %.4f%s%s)" %
              (tag, dt * 1e3 / n, n, misc["test_psnr"].item(), misc["test_ssim"].item(), misc["test_flip"].item(),
               " lpips %.4f" % misc["test_lpips"].item() if lp is not None else "",
               " lpips_vgg %.4f" % misc["test_lpips_vgg"].item() if lpv is not None else ""))
    print("files:", len(os.listdir(out)))


if __name__ == "__main__":
    spec = {"--lpips_weights": None, "--lpips_vgg_weights": None}
    for flag in spec:
        if flag in sys.argv:  # (taken out first: the positional arguments keep their places)
            at = sys.argv.index(flag)
            spec[flag] = sys.argv[at + 1]
            del sys.argv[at:at + 2]
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 40, spec["--lpips_weights"], spec["--lpips_vgg_weights"])
