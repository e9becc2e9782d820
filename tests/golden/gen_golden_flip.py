"""Golden vectors for the FLIP metric, produced by the REFERENCE's utils/flip_loss.py on the CPU (dev container only).

    python tests/golden/gen_golden_flip.py       # needs /root/reference; writes tests/golden/flip.npz

Called as main.py:378 does: compute_flip(rec, ref, pixels_per_degree) on [N,3,H,W] tensors.  The reference module moves its
tensors with .cuda() and allocates with device='cuda'; both are neutralised here (Tensor.cuda returns self, the module sees
a `torch` whose zeros() drops the device).  Every case is run twice: in fp32 as the reference runs it (flip32: the yardstick
for fp32 rounding) and under torch.set_default_dtype(float64) (flip64: the value the tests compare against).

Per case NAME the file holds  img_NAME (the key of its input pair: pred_KEY / gt_KEY, [H,W,3] fp32), ppd_NAME, flip32_NAME
[H,W] fp32, flip64_NAME [H,W] fp64, mean32_NAME, mean64_NAME.  `multi_*` is the test-set loop's number (main.py:359-379):
three different frames, each stack rescaled to [-1,1] by its own extrema over all frames, compute_flip, mean."""
import importlib.util
import math
import os

import numpy as np
import torch

REF = "/root/reference/utils/flip_loss.py"
OUT = os.path.dirname(os.path.abspath(__file__))
PPD = 0.7 * (3840 / 0.7) * (math.pi / 180)


class _TorchOnCpu:
    """`torch` as the loaded module sees it: zeros() without its device argument."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def zeros(*a, **k):
        k.pop("device", None)
        return torch.zeros(*a, **k)


def load_reference():
    torch.Tensor.cuda = lambda self, *a, **k: self
    spec = importlib.util.spec_from_file_location("ref_flip_loss", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.torch = _TorchOnCpu()
    return mod


def noisy(H, W, g):
    yy, xx = torch.meshgrid(torch.linspace(0, 3, H), torch.linspace(0, 4, W), indexing="ij")
    gt = torch.stack([0.5 + 0.5 * torch.sin(2.1 * xx + yy), 0.5 + 0.5 * torch.cos(1.3 * yy * xx), (xx / 4. + yy / 3.) / 2.], -1)
    gt = (gt + 0.1 * torch.rand(H, W, 3, generator=g)).clamp(0, 1)
    pred = (gt + 0.08 * torch.randn(H, W, 3, generator=g)).clamp(0, 1)
    return pred, gt


def scene(H, W, g):
    """White background, a textured disc with noise inside only, and a corner patch where pred is a flat 0.97."""
    tex, _ = noisy(H, W, g)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    disc = (((yy - 0.55 * H)**2 + (xx - 0.5 * W)**2) < (0.3 * min(H, W))**2)[..., None]
    gt = torch.where(disc, tex, torch.ones(H, W, 3))
    pred = torch.where(disc, (gt + 0.08 * torch.randn(H, W, 3, generator=g)).clamp(0, 1), gt)
    pred[:12, :14] = 0.97
    return pred.contiguous(), gt.contiguous()


def run(mod, a, b, ppd, dtype):
    """a, b: [N,H,W,3] fp32 -> the reference's [N,H,W] map in `dtype` arithmetic."""
    torch.set_default_dtype(dtype)
    try:
        out = mod.FLIP().compute_flip(a.to(dtype).permute(0, 3, 1, 2), b.to(dtype).permute(0, 3, 1, 2), ppd)
    finally:
        torch.set_default_dtype(torch.float32)
    return out[:, 0]


def stack_rescale(x):
    """The [-1, 1] rescale the test-set loop applies to a whole stack of frames before LPIPS and FLIP (main.py:361-363)."""
    return 2.0 / (x.max() - x.min()) * (x - x.min()) - 1.0


def main():
    mod = load_reference()
    g = torch.Generator().manual_seed(11)
    out, pairs = {}, {}
    for key, (H, W) in (("1x1", (1, 1)), ("7x9", (7, 9)), ("33x16", (33, 16)), ("40x52", (40, 52)), ("70x90", (70, 90))):
        pairs[key] = noisy(H, W, g)
    pairs["scene"] = scene(70, 90, g)
    for key, (p, t) in pairs.items():
        out["pred_" + key], out["gt_" + key] = p.numpy(), t.numpy()
    cases = [(k, k, PPD) for k in ("1x1", "7x9", "33x16", "40x52", "70x90")] + [("33x16_ppd30", "33x16", 30.0), ("70x90_ppd30", "70x90", 30.0),
                                                                                 ("scene", "scene", PPD), ("scene_ppd30", "scene", 30.0)]
    for name, key, ppd in cases:
        p, t = pairs[key]
        f32, f64 = run(mod, p[None], t[None], ppd, torch.float32)[0], run(mod, p[None], t[None], ppd, torch.float64)[0]
        out["img_" + name], out["ppd_" + name] = np.array(key), np.float64(ppd)
        out["flip32_" + name], out["flip64_" + name] = f32.numpy(), f64.numpy()
        out["mean32_" + name], out["mean64_" + name] = np.float32(f32.mean().item()), np.float64(f64.mean().item())
        print("%-12s ppd %.2f mean64 %.6f |mean32-mean64| %.2e max|flip32-flip64| %.2e" %
              (name, ppd, f64.mean().item(), abs(f32.mean().item() - f64.mean().item()), (f32.double() - f64).abs().max().item()))
    out["cases"] = np.array([c[0] for c in cases])
    # the test-set loop's number: three different frames (the second pair with less noise, the third darker), one rescale per stack
    frames = [noisy(28, 36, g) for _ in range(3)]
    rec = torch.stack([frames[0][0], 0.5 * (frames[1][0] + frames[1][1]), 0.1 + 0.6 * frames[2][0]], 0)
    ref = torch.stack([frames[0][1], frames[1][1], 0.05 + 0.6 * frames[2][1]], 0)
    f32 = run(mod, stack_rescale(rec), stack_rescale(ref), PPD, torch.float32)
    f64 = run(mod, stack_rescale(rec.double()), stack_rescale(ref.double()), PPD, torch.float64)
    plain = run(mod, rec, ref, PPD, torch.float64)
    out["multi_rec"], out["multi_ref"] = rec.numpy(), ref.numpy()
    out["multi_flip32"], out["multi_flip64"] = f32.numpy(), f64.numpy()
    out["multi_mean32"], out["multi_mean64"] = np.float32(f32.mean().item()), np.float64(f64.mean().item())
    out["multi_mean64_plain"] = np.float64(plain.mean().item())
    print("multi        mean64 %.6f (plain, no rescale: %.6f) |mean32-mean64| %.2e max|flip32-flip64| %.2e" %
          (f64.mean().item(), plain.mean().item(), abs(f32.mean().item() - f64.mean().item()), (f32.double() - f64).abs().max().item()))
    np.savez_compressed(os.path.join(OUT, "flip.npz"), **out)
    print("wrote flip.npz: %d bytes" % os.path.getsize(os.path.join(OUT, "flip.npz")))


if __name__ == "__main__":
    main()
