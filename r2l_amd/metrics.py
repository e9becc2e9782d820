"""Small numeric helpers shared by the drivers (reference: utils/run_nerf_raybased_helpers.py:14-20) and the
test-set SSIM (utils/ssim_torch.py) and FLIP (utils/flip_loss.py)."""
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
                              _lib.stream(a.device)), "r2l_ssim")
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
                              _lib.stream(a.device)), "r2l_flip")
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


# ---- LPIPS (lpips.LPIPS(net='alex', version='0.1') in eval mode, as main.py:359-369 calls it) ---------------------------------
# (in, out, kernel, stride, zero padding) of the five AlexNet convolutions; a 3 / 2 max-pool (floor) sits in front of 1 and 2
LPIPS_CONVS = ((3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1))
LPIPS_SHIFT, LPIPS_SCALE = (-0.030, -0.088, -0.188), (0.458, 0.448, 0.450)
LPIPS_PARAM_FLOATS = sum(ci * co * k * k + 2 * co for ci, co, k, _, _ in LPIPS_CONVS)  # 2 470 848
_LPIPS_FEATURES = (0, 3, 6, 8, 10)  # torchvision's alexnet.features indices of the convolutions


def lpips_sizes(H, W):
    """[(Ho, Wo)] of the five feature maps of an H x W image (400 -> 99, 49, 24, 24, 24; 31 -> 7, 3, 1, 1, 1)."""
    out = []
    for l, (_, _, k, s, p) in enumerate(LPIPS_CONVS):
        if l in (1, 2):
            H, W = (H - 3) // 2 + 1, (W - 3) // 2 + 1
        H, W = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        out.append((H, W))
    return out


def lpips_flatten(convs, lins):
    """[(weight [Co,Ci,k,k], bias [Co])] x 5 and five lin weights -> the flat fp32 vector of r2l_lpips_pack."""
    flat = torch.cat([t.detach().float().reshape(-1) for wb in convs for t in wb] + [t.detach().float().reshape(-1) for t in lins])
    assert flat.numel() == LPIPS_PARAM_FLOATS
    return flat.contiguous()


def lpips_params(path):
    """The flat fp32 parameter vector (for l = 0..4 { conv weight, bias }, then lin_0 .. lin_4) from the user's files: one file,
    or two joined by ':' whose keys are merged.  Two naming schemes are understood: torchvision's AlexNet checkpoint
    (features.{0,3,6,8,10}.{weight,bias}) beside the lpips package's alex.pth (lin{0..4}.model.1.weight), and a saved
    lpips.LPIPS().state_dict() (net.slice{1..5}.{0,3,6,8,10}.{weight,bias} + lin{k}.model.1.weight).  Extra keys are ignored; a
    missing key or a wrong shape is a ValueError that names the key."""
    sd = {}
    for part in str(path).split(":"):
        if not part:
            continue
        obj = torch.load(part, map_location="cpu", weights_only=True)
        if not isinstance(obj, dict):
            raise ValueError("%s: expected a state dict, got %s" % (part, type(obj).__name__))
        sd.update(obj)
    convs, lins = [], []
    for l, (ci, co, k, _, _) in enumerate(LPIPS_CONVS):
        pair = []
        for leaf, shape in (("weight", (co, ci, k, k)), ("bias", (co,))):
            names = ("features.%d.%s" % (_LPIPS_FEATURES[l], leaf), "net.slice%d.%d.%s" % (l + 1, _LPIPS_FEATURES[l], leaf))
            key = next((n for n in names if n in sd), None)
            if key is None:
                raise ValueError("LPIPS weights %s: missing key %s (or %s)" % (path, names[0], names[1]))
            if tuple(sd[key].shape) != shape:
                raise ValueError("LPIPS weights %s: key %s has shape %s, expected %s" % (path, key, tuple(sd[key].shape), shape))
            pair.append(sd[key])
        convs.append(pair)
    for l, (_, co, _, _, _) in enumerate(LPIPS_CONVS):
        key = "lin%d.model.1.weight" % l
        if key not in sd:
            raise ValueError("LPIPS weights %s: missing key %s" % (path, key))
        if tuple(sd[key].shape) != (1, co, 1, 1):
            raise ValueError("LPIPS weights %s: key %s has shape %s, expected %s" % (path, key, tuple(sd[key].shape), (1, co, 1, 1)))
        lins.append(sd[key])
    return lpips_flatten(convs, lins)


def lpips_unflatten(params):
    """The flat vector -> ([(weight, bias)] x 5, [lin] x 5) as views."""
    assert params.numel() == LPIPS_PARAM_FLOATS, "LPIPS parameters: %d floats, expected %d" % (params.numel(), LPIPS_PARAM_FLOATS)
    convs, lins, o = [], [], 0
    for ci, co, k, _, _ in LPIPS_CONVS:
        n = co * ci * k * k
        convs.append((params[o:o + n].view(co, ci, k, k), params[o + n:o + n + co]))
        o += n + co
    for _, co, _, _, _ in LPIPS_CONVS:
        lins.append(params[o:o + co])
        o += co
    return convs, lins


def _lpips_features(x, convs, shift=True, pad_first=False, ceil_mode=False):
    """The five post-ReLU feature maps [K,C,Ho,Wo] of a [K,H,W,3] stack, op by op.  The keywords exist for the tests: anything
    but the defaults is a deliberately wrong evaluation (no shift; zero padding in front of the scaling layer; ceil-mode pools)
    that the bars must be able to see."""
    import torch.nn.functional as F
    t = dict(dtype=x.dtype, device=x.device)
    # the scaling layer's constants are fp32 numbers (the lpips package holds them in fp32 buffers, the kernel as float literals):
    # the float64 yardstick uses those values, not the decimal fractions
    sh = torch.tensor(LPIPS_SHIFT if shift else (0., 0., 0.), dtype=torch.float32).to(**t).view(1, 3, 1, 1)
    sc = torch.tensor(LPIPS_SCALE, dtype=torch.float32).to(**t).view(1, 3, 1, 1)
    x = x.permute(0, 3, 1, 2)
    if pad_first:
        x = F.pad(x, (2, 2, 2, 2))
    x = (x - sh) / sc
    feats = []
    for l, ((w, b), (_, _, _, s, p)) in enumerate(zip(convs, LPIPS_CONVS)):
        if l in (1, 2):
            x = F.max_pool2d(x, 3, 2, ceil_mode=ceil_mode)
        x = F.relu(F.conv2d(x, w.to(**t), b.to(**t), stride=s, padding=0 if (l == 0 and pad_first) else p))
        feats.append(x)
    return feats


def _lpips_torch(a, b, params, **wrong):
    """-> per-layer means [K,5] and the five maps [K,Ho,Wo] of two [K,H,W,3] stacks, in their dtype and on their device."""
    convs, lins = lpips_unflatten(params)
    fa, fb = _lpips_features(a, convs, **wrong), _lpips_features(b, convs, **wrong)
    maps = []
    for l in range(5):
        na = fa[l] / (fa[l].pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        nb = fb[l] / (fb[l].pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        maps.append(((na - nb).pow(2) * lins[l].to(dtype=a.dtype, device=a.device).view(1, -1, 1, 1)).sum(1))
    return torch.stack([m.mean((1, 2)) for m in maps], 1), maps


_LPIPS_PACKED = {}  # (device, data_ptr, version of the params tensor) -> (params, packed stream): a few entries at most


def _lpips_stream(L, params, device):
    key = (str(device), params.data_ptr(), params._version)
    hit = _LPIPS_PACKED.get(key)
    if hit is not None and hit[0] is params:
        return hit[1]
    assert params.numel() == L.r2l_lpips_param_floats(), "LPIPS parameters: %d floats, expected %d" % (
        params.numel(), L.r2l_lpips_param_floats())
    flat = params.detach().to(device).float().contiguous()
    wpack = torch.empty(L.r2l_lpips_pack_floats(), device=device)
    from . import _lib
    _lib.check(L.r2l_lpips_pack(flat.data_ptr(), wpack.data_ptr(), _lib.stream(device)),
               "r2l_lpips_pack")
    while len(_LPIPS_PACKED) >= 4:
        _LPIPS_PACKED.pop(next(iter(_LPIPS_PACKED)))
    _LPIPS_PACKED[key] = (params, wpack)  # (holding params keeps its address from being reused under this key)
    return wpack


def lpips(img, ref, params, rescale=None, normalize=False, return_layers=False, return_maps=False):
    """LPIPS (AlexNet, v0.1) of [H,W,3] or [K,H,W,3] images with values in [-1, 1]; H, W >= 31.  params: the flat vector of
    lpips_params.  normalize: the images are in [0, 1] and are mapped by 2 x - 1 first.  rescale: None or a 4-tensor
    {min_img, max_img, min_ref, max_ref}: each input is first mapped by 2 / (max - min) * (x - min) - 1, the [-1, 1] rescale
    main.py:361-363 applies to the whole stack.  CUDA tensors run the fused HIP kernels (r2l_lpips; the packed weight stream is
    cached per device and params tensor); CPU tensors an op-by-op torch evaluation in their own dtype (fp32: the CPU plumbing
    config; float64: the yardstick of the tests).  Returns the values ([K], or 0-d for a single pair), then, if asked for, the
    per-layer means v_0 .. v_4 ([K,5] / [5]) and the list of the five maps d_l ([K,Ho,Wo] / [Ho,Wo])."""
    assert img.shape == ref.shape and img.dim() in (3, 4) and img.shape[-1] == 3
    single = img.dim() == 3
    H, W = img.shape[-3:-1]
    if H < 31 or W < 31:
        raise ValueError("LPIPS needs images of at least 31 x 31 pixels (got %d x %d): the deepest feature map would be empty" % (H, W))
    if img.is_cuda:
        from . import _lib
        L = _lib.load()
        a, b = img.detach().float().contiguous(), ref.detach().to(img.device).float().contiguous()
        if normalize:
            a, b = 2 * a - 1, 2 * b - 1
        K = 1 if single else a.shape[0]
        wpack = _lpips_stream(L, params, a.device)
        work = torch.empty(L.r2l_lpips_work_floats(K, H, W), device=a.device)
        out = torch.empty(K, device=a.device)
        layers = torch.empty((K, 5), device=a.device) if return_layers else None
        flat = torch.empty((K, L.r2l_lpips_map_floats(H, W)), device=a.device) if return_maps else None
        ext = rescale.detach().to(a.device).float().contiguous() if rescale is not None else None
        assert ext is None or ext.numel() == 4
        _lib.check(L.r2l_lpips(a.data_ptr(), b.data_ptr(), K, H, W, ext.data_ptr() if ext is not None else None, wpack.data_ptr(),
                               work.data_ptr(), layers.data_ptr() if return_layers else None,
                               flat.data_ptr() if return_maps else None, out.data_ptr(),
                               _lib.stream(a.device)), "r2l_lpips")
        maps, o = [], 0
        for ho, wo in (lpips_sizes(H, W) if return_maps else ()):
            maps.append(flat[:, o:o + ho * wo].view(K, ho, wo))
            o += ho * wo
    else:
        a, b = (img[None], ref[None]) if single else (img, ref)
        a, b = (a, b.to(a.dtype)) if a.dtype == torch.float64 else (a.float(), b.float())
        if normalize:
            a, b = 2 * a - 1, 2 * b - 1
        if rescale is not None:
            e = rescale.to(a.dtype)
            assert e.numel() == 4
            a, b = 2 / (e[1] - e[0]) * (a - e[0]) - 1, 2 / (e[3] - e[2]) * (b - e[2]) - 1
        layers, maps = _lpips_torch(a, b, params.detach().to(a.dtype))
        out = layers[:, 0]
        for l in range(1, 5):
            out = out + layers[:, l]
    res = [out[0] if single else out]
    if return_layers:
        res.append(layers[0] if single else layers)
    if return_maps:
        res.append([m[0] for m in maps] if single else maps)
    return res[0] if len(res) == 1 else tuple(res)


# ---- LPIPS, the VGG-16 variant (lpips.LPIPS(net='vgg', version='0.1') in eval mode: the published NeRF / R2L tables) --------------
# (in, out) of the thirteen 3 x 3 / 1 / 1 convolutions; a 2 / 2 max-pool (floor) sits in front of 2, 4, 7 and 10; the taps are the
# post-ReLU outputs of 1, 3, 6, 9 and 12 (conv1_2, conv2_2, conv3_3, conv4_3, conv5_3)
LPIPS_VGG_CONVS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
                   (512, 512), (512, 512), (512, 512))
LPIPS_VGG_TAPS = (1, 3, 6, 9, 12)
_LPIPS_VGG_POOLS = (2, 4, 7, 10)
LPIPS_VGG_PARAM_FLOATS = (sum(9 * ci * co + co for ci, co in LPIPS_VGG_CONVS) +
                          sum(LPIPS_VGG_CONVS[t][1] for t in LPIPS_VGG_TAPS))  # 14 716 160
_LPIPS_VGG_FEATURES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)  # torchvision's vgg16.features indices of the convolutions
_LPIPS_VGG_SLICE = (1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5)              # the lpips package's slice of each


def lpips_vgg_sizes(H, W):
    """[(Ho, Wo)] of the five feature maps of an H x W image (400 -> 400, 200, 100, 50, 25; 16 -> 16, 8, 4, 2, 1)."""
    return [(H >> s, W >> s) for s in range(5)]


def lpips_vgg_flatten(convs, lins):
    """[(weight [Co,Ci,3,3], bias [Co])] x 13 and five lin weights -> the flat fp32 vector of r2l_lpips_vgg_pack."""
    flat = torch.cat([t.detach().float().reshape(-1) for wb in convs for t in wb] + [t.detach().float().reshape(-1) for t in lins])
    assert flat.numel() == LPIPS_VGG_PARAM_FLOATS
    return flat.contiguous()


def lpips_vgg_unflatten(params):
    """The flat vector -> ([(weight, bias)] x 13, [lin] x 5) as views."""
    assert params.numel() == LPIPS_VGG_PARAM_FLOATS, "LPIPS (VGG) parameters: %d floats, expected %d" % (
        params.numel(), LPIPS_VGG_PARAM_FLOATS)
    convs, lins, o = [], [], 0
    for ci, co in LPIPS_VGG_CONVS:
        n = co * ci * 9
        convs.append((params[o:o + n].view(co, ci, 3, 3), params[o + n:o + n + co]))
        o += n + co
    for t in LPIPS_VGG_TAPS:
        co = LPIPS_VGG_CONVS[t][1]
        lins.append(params[o:o + co])
        o += co
    return convs, lins


def lpips_vgg_params(path):
    """The flat fp32 parameter vector (for l = 0..12 { conv weight, bias }, then lin_0 .. lin_4) from the user's files: one file, or
    two joined by ':' whose keys are merged.  Understood: torchvision's VGG-16 checkpoint
    (features.{0,2,5,7,10,12,14,17,19,21,24,26,28}.{weight,bias}) beside the lpips package's vgg.pth (lin{0..4}.model.1.weight,
    shape (1, C, 1, 1)), and a saved lpips.LPIPS(net='vgg').state_dict() (net.slice1.{0,2}, net.slice2.{5,7}, net.slice3.{10,12,14},
    net.slice4.{17,19,21}, net.slice5.{24,26,28} + the same lin keys).  Extra keys (torchvision's classifier.*) are ignored; a
    missing key or a wrong shape is a ValueError that names the key."""
    sd = {}
    for part in str(path).split(":"):
        if not part:
            continue
        obj = torch.load(part, map_location="cpu", weights_only=True)
        if not isinstance(obj, dict):
            raise ValueError("%s: expected a state dict, got %s" % (part, type(obj).__name__))
        sd.update(obj)
    convs, lins = [], []
    for l, (ci, co) in enumerate(LPIPS_VGG_CONVS):
        pair = []
        for leaf, shape in (("weight", (co, ci, 3, 3)), ("bias", (co,))):
            names = ("features.%d.%s" % (_LPIPS_VGG_FEATURES[l], leaf),
                     "net.slice%d.%d.%s" % (_LPIPS_VGG_SLICE[l], _LPIPS_VGG_FEATURES[l], leaf))
            key = next((n for n in names if n in sd), None)
            if key is None:
                raise ValueError("LPIPS (VGG) weights %s: missing key %s (or %s)" % (path, names[0], names[1]))
            if tuple(sd[key].shape) != shape:
                raise ValueError("LPIPS (VGG) weights %s: key %s has shape %s, expected %s" % (path, key, tuple(sd[key].shape), shape))
            pair.append(sd[key])
        convs.append(pair)
    for l, t in enumerate(LPIPS_VGG_TAPS):
        key, co = "lin%d.model.1.weight" % l, LPIPS_VGG_CONVS[t][1]
        if key not in sd:
            raise ValueError("LPIPS (VGG) weights %s: missing key %s" % (path, key))
        if tuple(sd[key].shape) != (1, co, 1, 1):
            raise ValueError("LPIPS (VGG) weights %s: key %s has shape %s, expected %s" % (path, key, tuple(sd[key].shape), (1, co, 1, 1)))
        lins.append(sd[key])
    return lpips_vgg_flatten(convs, lins)


def _lpips_vgg_features(x, convs, shift=True, ceil_mode=False, pre_relu=False):
    """The five feature maps [K,C,Ho,Wo] of a [K,H,W,3] stack, op by op.  The keywords exist for the tests: anything but the
    defaults is a deliberately wrong evaluation (no shift; ceil-mode pools; the tap taken in front of its ReLU) that the bars must
    be able to see."""
    import torch.nn.functional as F
    t = dict(dtype=x.dtype, device=x.device)
    # (the scaling layer's constants are fp32 numbers, as in _lpips_features)
    sh = torch.tensor(LPIPS_SHIFT if shift else (0., 0., 0.), dtype=torch.float32).to(**t).view(1, 3, 1, 1)
    sc = torch.tensor(LPIPS_SCALE, dtype=torch.float32).to(**t).view(1, 3, 1, 1)
    x = (x.permute(0, 3, 1, 2) - sh) / sc
    feats = []
    for l, (w, b) in enumerate(convs):
        if l in _LPIPS_VGG_POOLS:
            x = F.max_pool2d(x, 2, 2, ceil_mode=ceil_mode)
        y = F.conv2d(x, w.to(**t), b.to(**t), padding=1)
        x = F.relu(y)
        if l in LPIPS_VGG_TAPS:
            feats.append(y if pre_relu else x)
    return feats


def _lpips_vgg_torch(a, b, params, **wrong):
    """-> per-layer means [K,5] and the five maps [K,Ho,Wo] of two [K,H,W,3] stacks, in their dtype and on their device."""
    convs, lins = lpips_vgg_unflatten(params)
    fa, fb = _lpips_vgg_features(a, convs, **wrong), _lpips_vgg_features(b, convs, **wrong)
    maps = []
    for l in range(5):
        na = fa[l] / (fa[l].pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        nb = fb[l] / (fb[l].pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        maps.append(((na - nb).pow(2) * lins[l].to(dtype=a.dtype, device=a.device).view(1, -1, 1, 1)).sum(1))
    return torch.stack([m.mean((1, 2)) for m in maps], 1), maps


_LPIPS_VGG_PACKED = {}  # as _LPIPS_PACKED


def _lpips_vgg_stream(L, params, device):
    key = (str(device), params.data_ptr(), params._version)
    hit = _LPIPS_VGG_PACKED.get(key)
    if hit is not None and hit[0] is params:
        return hit[1]
    assert params.numel() == L.r2l_lpips_vgg_param_floats(), "LPIPS (VGG) parameters: %d floats, expected %d" % (
        params.numel(), L.r2l_lpips_vgg_param_floats())
    flat = params.detach().to(device).float().contiguous()
    wpack = torch.empty(L.r2l_lpips_vgg_pack_floats(), device=device)
    from . import _lib
    _lib.check(L.r2l_lpips_vgg_pack(flat.data_ptr(), wpack.data_ptr(), _lib.stream(device)),
               "r2l_lpips_vgg_pack")
    while len(_LPIPS_VGG_PACKED) >= 4:
        _LPIPS_VGG_PACKED.pop(next(iter(_LPIPS_VGG_PACKED)))
    _LPIPS_VGG_PACKED[key] = (params, wpack)
    return wpack


def lpips_vgg(img, ref, params, rescale=None, normalize=False, return_layers=False, return_maps=False):
    """LPIPS (VGG-16, v0.1) of [H,W,3] or [K,H,W,3] images with values in [-1, 1]; H, W >= 16.  params: the flat vector of
    lpips_vgg_params.  normalize, rescale, the CUDA / CPU branches and the return values: as lpips (the kernels are r2l_lpips_vgg;
    the five maps have the sizes of lpips_vgg_sizes)."""
    assert img.shape == ref.shape and img.dim() in (3, 4) and img.shape[-1] == 3
    single = img.dim() == 3
    H, W = img.shape[-3:-1]
    if H < 16 or W < 16:
        raise ValueError("LPIPS (VGG) needs images of at least 16 x 16 pixels (got %d x %d): the deepest feature map would be empty"
                         % (H, W))
    if img.is_cuda:
        from . import _lib
        L = _lib.load()
        a, b = img.detach().float().contiguous(), ref.detach().to(img.device).float().contiguous()
        if normalize:
            a, b = 2 * a - 1, 2 * b - 1
        K = 1 if single else a.shape[0]
        wpack = _lpips_vgg_stream(L, params, a.device)
        nwork = L.r2l_lpips_vgg_work_floats(K, H, W)
        if nwork < 0:
            raise ValueError("LPIPS (VGG): %d pairs of %d x %d exceed one launch" % (K, H, W))
        work = torch.empty(nwork, device=a.device)
        out = torch.empty(K, device=a.device)
        layers = torch.empty((K, 5), device=a.device) if return_layers else None
        flat = torch.empty((K, L.r2l_lpips_vgg_map_floats(H, W)), device=a.device) if return_maps else None
        ext = rescale.detach().to(a.device).float().contiguous() if rescale is not None else None
        assert ext is None or ext.numel() == 4
        _lib.check(L.r2l_lpips_vgg(a.data_ptr(), b.data_ptr(), K, H, W, ext.data_ptr() if ext is not None else None,
                                   wpack.data_ptr(), work.data_ptr(), layers.data_ptr() if return_layers else None,
                                   flat.data_ptr() if return_maps else None, out.data_ptr(),
                                   _lib.stream(a.device)), "r2l_lpips_vgg")
        maps, o = [], 0
        for ho, wo in (lpips_vgg_sizes(H, W) if return_maps else ()):
            maps.append(flat[:, o:o + ho * wo].view(K, ho, wo))
            o += ho * wo
    else:
        a, b = (img[None], ref[None]) if single else (img, ref)
        a, b = (a, b.to(a.dtype)) if a.dtype == torch.float64 else (a.float(), b.float())
        if normalize:
            a, b = 2 * a - 1, 2 * b - 1
        if rescale is not None:
            e = rescale.to(a.dtype)
            assert e.numel() == 4
            a, b = 2 / (e[1] - e[0]) * (a - e[0]) - 1, 2 / (e[3] - e[2]) * (b - e[2]) - 1
        layers, maps = _lpips_vgg_torch(a, b, params.detach().to(a.dtype))
        out = layers[:, 0]
        for l in range(1, 5):
            out = out + layers[:, l]
    res = [out[0] if single else out]
    if return_layers:
        res.append(layers[0] if single else layers)
    if return_maps:
        res.append([m[0] for m in maps] if single else maps)
    return res[0] if len(res) == 1 else tuple(res)
