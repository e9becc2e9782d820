"""Small numeric helpers shared by the drivers (reference: utils/run_nerf_raybased_helpers.py:14-20) and the
test-set SSIM (utils/ssim_torch.py) and FLIP (utils/flip_loss.py)."""
import ctypes
import math

import numpy as np
import torch


def to_tensor(x, device=None):
    device = device or ("cuda" if torch.cuda.is_available() else "cpu")
    return x.to(device) if isinstance(x, torch.Tensor) else torch.Tensor(x).to(device)


def to_array(x):
    return x if isinstance(x, np.ndarray) else x.data.cpu().numpy()


def to8b(x):
    return (255 * np.clip(to_array(x), 0, 1)).astype(np.uint8)


def img2mse(x, y):
    return torch.mean((x - y)**2)


def mse2psnr(x):
    return -10. * torch.log(x) / torch.log(torch.tensor([10.], device=x.device))


_WINDOW = None


def _ssim_window():
    """The reference's 11x11 window, built the way ssim_torch.py:11-25 builds it (fp32 normalise, fp32 outer product)."""
    global _WINDOW
    if _WINDOW is None:
        g = torch.tensor([math.exp(-(x - 5)**2 / float(2 * 1.5**2)) for x in range(11)])
        g = g / g.sum()
        _WINDOW = (g[:, None] @ g[None, :]).contiguous()
    return _WINDOW


def ssim(img, ref):
    """SSIM of two [H, W, C] images in [0,1] (main.py:46 `ssim`, minus the permutes: the kernel reads HWC directly).
    CUDA tensors run the fused HIP kernel (r2l_ssim); CPU tensors (the CPU plumbing config) use torch conv2d."""
    assert img.shape == ref.shape and img.dim() == 3
    win = _ssim_window()
    if img.is_cuda:
        from . import _lib
        L = _lib.load()
        a, b = img.detach().float().contiguous(), ref.detach().to(img.device).float().contiguous()
        H, W, C = a.shape
        partial = torch.empty(L.r2l_ssim_partial_count(H, W, C), device=a.device)
        out = torch.empty(1, device=a.device)
        _lib.check(L.r2l_ssim(a.data_ptr(), b.data_ptr(), H, W, C, win.data_ptr(), partial.data_ptr(), out.data_ptr(),
                              ctypes.c_void_p(torch.cuda.current_stream(a.device).cuda_stream)), "r2l_ssim")
        return out[0]
    import torch.nn.functional as F
    a, b = img.float().permute(2, 0, 1)[None], ref.float().permute(2, 0, 1)[None]
    C = a.shape[1]
    w = win[None, None].expand(C, 1, 11, 11).contiguous()
    mu1, mu2 = F.conv2d(a, w, padding=5, groups=C), F.conv2d(b, w, padding=5, groups=C)
    s1 = F.conv2d(a * a, w, padding=5, groups=C) - mu1 * mu1
    s2 = F.conv2d(b * b, w, padding=5, groups=C) - mu2 * mu2
    s12 = F.conv2d(a * b, w, padding=5, groups=C) - mu1 * mu2
    C1, C2 = 0.01**2, 0.03**2
    return (((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))).mean()


# ---- FLIP (utils/flip_loss.py:70-130 as main.py:371-379 calls it) -------------------------------------------------------
FLIP_PPD = 0.7 * (3840 / 0.7) * (math.pi / 180)  # main.py:373-377: a 0.7 m wide 3840-pixel monitor seen from 0.7 m

# linear RGB -> XYZ under D65 (flip_loss.py:324-333); the white point of YCxCz and L*a*b* is this matrix applied to (1,1,1)
_RGB2XYZ = np.array([[10135552 / 24577794, 8788810 / 24577794, 4435075 / 24577794],
                     [2613072 / 12288897, 8788810 / 12288897, 887015 / 12288897],
                     [1425312 / 73733382, 8788810 / 73733382, 70074185 / 73733382]])


def _flip_windows(ppd):
    """The five 2-D windows in double: CSF a / rg / by (each divided by its own sum) and the edge / point detectors along x
    (positive taps sum to +1, negative ones to -1); the y detectors are their transposes."""
    r = int(math.ceil(3 * math.sqrt(0.04 / (2 * math.pi**2)) * ppd))
    y, x = np.mgrid[-r:r + 1, -r:r + 1]
    z = (x * x + y * y) / float(ppd)**2
    win = {}
    for name, (a1, b1, a2, b2) in (("a", (1, 0.0047, 0, 1e-5)), ("rg", (1, 0.0053, 0, 1e-5)), ("by", (34.1, 0.04, 13.5, 0.025))):
        g = a1 * math.sqrt(math.pi / b1) * np.exp(-math.pi**2 * z / b1) + a2 * math.sqrt(math.pi / b2) * np.exp(-math.pi**2 * z / b2)
        win[name] = g / g.sum()
    sd = 0.5 * 0.082 * ppd
    rf = int(math.ceil(3 * sd))
    y, x = np.mgrid[-rf:rf + 1, -rf:rf + 1]
    g = np.exp(-(x * x + y * y) / (2 * sd * sd))
    for name, w in (("edge", -x * g), ("point", (x * x / (sd * sd) - 1) * g)):
        win[name] = np.where(w < 0, w / -w[w < 0].sum(), w / w[w > 0].sum())
    return win


def _flip_torch(a, b, ppd, padding="replicate"):
    """FLIP map [K,H,W] of two [K,H,W,3] stacks, op by op in their dtype and on their device.  `padding` exists for the tests:
    anything but the reference's 'replicate' is a deliberately wrong evaluation that the bars must be able to see."""
    import torch.nn.functional as F
    t = dict(dtype=a.dtype, device=a.device)
    M = torch.tensor(_RGB2XYZ, **t)
    white = M.sum(1).view(1, 3, 1, 1)
    win = {k: torch.tensor(v, **t)[None, None] for k, v in _flip_windows(ppd).items()}

    def mat(m, x):
        return torch.einsum("ij,kjhw->kihw", m, x)

    def conv(x, w):
        r = w.shape[-1] // 2
        x = F.pad(x, (r, r, r, r), mode=padding) if padding != "zeros" else F.pad(x, (r, r, r, r))
        return F.conv2d(x, w)

    def to_opponent(img):
        c = img.permute(0, 3, 1, 2).clamp(0, 1)
        lin = torch.where(c > 0.04045, ((c + 0.055) / 1.055)**2.4, c / 12.92)
        xyz = mat(M, lin) / white
        return torch.cat([116 * xyz[:, 1:2] - 16, 500 * (xyz[:, 0:1] - xyz[:, 1:2]), 200 * (xyz[:, 1:2] - xyz[:, 2:3])], 1)

    def hunt_lab(lin):
        xyz = mat(M, lin) / white
        f = torch.where(xyz > 0.00885, xyz**(1 / 3), xyz / (3 * (6 / 29)**2) + 4 / 29)
        L = 116 * f[:, 1:2] - 16
        return torch.cat([L, 0.01 * L * 500 * (f[:, 0:1] - f[:, 1:2]), 0.01 * L * 200 * (f[:, 1:2] - f[:, 2:3])], 1)

    def colour(opp):
        flt = torch.cat([conv(opp[:, 0:1], win["a"]), conv(opp[:, 1:2], win["rg"]), conv(opp[:, 2:3], win["by"])], 1)
        yy = (flt[:, 0:1] + 16) / 116
        xyz = torch.cat([yy + flt[:, 1:2] / 500, yy, yy - flt[:, 2:3] / 200], 1) * white
        return hunt_lab(mat(torch.inverse(M), xyz).clamp(0, 1))

    def hyab(p, q):
        d = p - q
        return d[:, 0:1].abs() + torch.norm(d[:, 1:3], dim=1, keepdim=True)

    def features(opp, kind):
        yy = (opp[:, 0:1] + 16) / 116
        # the detectors' taps sum to zero: taking the frame's mean off changes no value and spares fp32 the cancellation residue
        # of that constant, which the square root further down would amplify (a flat frame gives exactly 0).  The float64 branch is
        # the tests' yardstick and follows the reference operation by operation instead: its residue is 1e-17.
        if yy.dtype != torch.float64:
            yy = yy - yy.mean((2, 3), keepdim=True)
        return torch.norm(torch.cat([conv(yy, win[kind]), conv(yy, win[kind].transpose(2, 3))], 1), dim=1, keepdim=True)

    oa, ob = to_opponent(a), to_opponent(b)
    unit = torch.eye(3, **t).view(3, 3, 1, 1)
    cmax = hyab(hunt_lab(unit[1:2]), hunt_lab(unit[2:3])).item()**0.7
    pccmax = 0.4 * cmax
    pw = hyab(colour(oa), colour(ob))**0.7
    dec = torch.where(pw < pccmax, (0.95 / pccmax) * pw, 0.95 + ((pw - pccmax) / (cmax - pccmax)) * 0.05)
    d = torch.max((features(oa, "edge") - features(ob, "edge")).abs(), (features(oa, "point") - features(ob, "point")).abs())
    def_ = ((1 / math.sqrt(2)) * d).pow(0.5).clamp(0, 1)
    return dec.pow(1 - def_)[:, 0]


def flip(img, ref, pixels_per_degree=None, rescale=None, return_map=False):
    """Per-frame mean of the FLIP difference map of [H,W,3] or [K,H,W,3] images (flip_loss.py compute_flip; the function is
    symmetric in its two images).  pixels_per_degree: None = main.py's standard 67.02.  rescale: None (plain FLIP on [0,1]
    images) or a 4-tensor {min_img, max_img, min_ref, max_ref}: each input is first mapped by 2 / (max - min) * (x - min) - 1,
    the [-1,1] rescale main.py:361-363 applies to the whole stack (FLIP then clamps to [0,1]: the number the reference prints).
    CUDA tensors run the fused HIP kernel (r2l_flip); CPU tensors an op-by-op torch evaluation in their own dtype (fp32: the CPU
    plumbing config; float64: the yardstick of the tests).  Returns the means ([K], or 0-d for a single pair), and the map
    ([K,H,W] / [H,W]) as well when return_map."""
    assert img.shape == ref.shape and img.dim() in (3, 4) and img.shape[-1] == 3
    single = img.dim() == 3
    ppd = FLIP_PPD if pixels_per_degree is None else float(pixels_per_degree)
    if img.is_cuda:
        from . import _lib
        L = _lib.load()
        a, b = img.detach().float().contiguous(), ref.detach().to(img.device).float().contiguous()
        K, (H, W) = (1 if single else a.shape[0]), a.shape[-3:-1]
        partial = torch.empty(L.r2l_flip_partial_count(H, W, K), device=a.device)
        out = torch.empty(K, device=a.device)
        fmap = torch.empty((K, H, W), device=a.device) if return_map else None
        ext = rescale.detach().to(a.device).float().contiguous() if rescale is not None else None
        assert ext is None or ext.numel() == 4
        _lib.check(L.r2l_flip(a.data_ptr(), b.data_ptr(), K, H, W, ppd, ext.data_ptr() if ext is not None else None,
                              partial.data_ptr(), fmap.data_ptr() if return_map else None, out.data_ptr(),
                              ctypes.c_void_p(torch.cuda.current_stream(a.device).cuda_stream)), "r2l_flip")
    else:
        a, b = (img[None], ref[None]) if single else (img, ref)
        a, b = (a, b.to(a.dtype)) if a.dtype == torch.float64 else (a.float(), b.float())
        if rescale is not None:
            e = rescale.to(a.dtype)
            assert e.numel() == 4
            a, b = 2 / (e[1] - e[0]) * (a - e[0]) - 1, 2 / (e[3] - e[2]) * (b - e[2]) - 1
        fmap = _flip_torch(a, b, ppd)
        out = fmap.mean((1, 2))
    if single:
        return (out[0], fmap[0]) if return_map else out[0]
    return (out, fmap) if return_map else out
