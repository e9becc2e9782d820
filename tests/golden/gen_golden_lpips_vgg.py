"""Golden numbers of tests/lpips_vgg_util.py: LPIPS(VGG-16, v0.1, eval mode) in float64, restated here from the definition
without r2l_amd.metrics (plain F.conv2d / F.max_pool2d on NCHW tensors, the network written out stage by stage).

    python tests/golden/gen_golden_lpips_vgg.py        # prints GOLDEN and GOLDEN_STACK to ten digits

Only the inputs are shared with the tests: make_weights(7), pair2(H, W, 5) and the stack case of tests/lpips_vgg_util.py."""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from tests import lpips_vgg_util as U  # noqa: E402

STAGES = ((0, 1), (2, 3), (4, 5, 6), (7, 8, 9), (10, 11, 12))  # the convolutions of conv1_x .. conv5_x


def taps(img, w):
    """img [K,H,W,3] float64 in [-1, 1] -> the five post-ReLU maps [K,C,h,w]"""
    shift = torch.tensor([-0.030, -0.088, -0.188], dtype=torch.float32).double().view(1, 3, 1, 1)  # (fp32 buffers in the package)
    scale = torch.tensor([0.458, 0.448, 0.450], dtype=torch.float32).double().view(1, 3, 1, 1)
    x = (img.permute(0, 3, 1, 2) - shift) / scale
    out = []
    for s, stage in enumerate(STAGES):
        if s > 0:
            x = F.max_pool2d(x, kernel_size=2, stride=2)
        for l in stage:
            x = torch.clamp(F.conv2d(x, w["w%d" % l].double(), w["b%d" % l].double(), stride=1, padding=1), min=0)
        out.append(x)
    return out


def lpips_vgg64(a, b, w):
    """-> [K, 6]: total, v_0 .. v_4"""
    cols = []
    for l, (fa, fb) in enumerate(zip(taps(a, w), taps(b, w))):
        ua = fa / (torch.sqrt((fa * fa).sum(1, keepdim=True)) + 1e-10)
        ub = fb / (torch.sqrt((fb * fb).sum(1, keepdim=True)) + 1e-10)
        d = ((ua - ub)**2 * w["lin%d" % l].double().view(1, -1, 1, 1)).sum(1)
        cols.append(d.mean((1, 2)))
    return torch.stack([sum(cols)] + cols, 1)


def main():
    w = U.make_weights(7)
    print("GOLDEN = {")
    for H, W in U.SIZES:
        a, b = U.pair2(H, W, 5)
        v = lpips_vgg64((2 * a - 1).double()[None], (2 * b - 1).double()[None], w)[0]  # (2 x - 1 in fp32: the tests' inputs)
        print("    (%d, %d): (%s)," % (H, W, ", ".join("%.9e" % x for x in v.tolist())))
    print("}")
    A, B, e = U.stack_case()
    A, B, e = A.double(), B.double(), e.double()
    v = lpips_vgg64(2 / (e[1] - e[0]) * (A - e[0]) - 1, 2 / (e[3] - e[2]) * (B - e[2]) - 1, w)
    print("GOLDEN_STACK = (%s)" % ", ".join("%.9e" % x for x in v[:, 0].tolist()))


if __name__ == "__main__":
    main()
