"""Inputs, golden numbers and yardsticks shared by tests/test_lpips_vgg_cpu.py and tests/test_lpips_vgg_gpu.py.

The golden numbers come from tests/golden/gen_golden_lpips_vgg.py: an fp64 restatement of LPIPS(VGG-16, v0.1) written
independently of r2l_amd.metrics (plain F.conv2d / F.max_pool2d), on make_weights(7), lpips_util.pair2(H, W, 5) and inputs 2 x - 1.
Bars: for every layer value and the total max(4 |CPU fp32 - CPU fp64|, 1e-5 |fp64 value|); for every map position
max(4 max|CPU fp32 map - CPU fp64 map|, 1e-5 max of that fp64 map).

Measured on the CPU at SIZES and the stack case (fp32 branch against fp64 branch of metrics.lpips_vgg, 16 threads): per layer
1.1e-7 .. 1.05e-6 relative (the largest at 16x16 and 17x23, <= 4.2e-7 from 35x47 up), per map position 1.0e-6 .. 3.2e-6 of the
map's maximum.  REL_FLOOR = 1e-5 is 10 to 25 times the first (the AlexNet util chose its own as about 20 times).  One zeroed
weight of conv1_2 (ZERO_CONV1_2) moves the layer where it shows most by 4e-4 .. 6e-3 relative over SIZES and every layer by at
least 1e-5; one of conv5_3 (ZERO_CONV5_3) moves v_4 by 2.7e-5 at 130x131.  The smallest channel norm is 0.17 .. 0.45 of its
layer's median.

lin_l = |randn| / C_l * 4^l: with plain |randn| / C the deep layers' v_l fall to 1e-5, under check_conditions' 1e-4; with the
factor every v_l is at least 3e-3 at these sizes."""
import math

import torch

from tests.lpips_util import pair2  # noqa: F401  (the same image pairs as the AlexNet tests)

CH = [(3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512), (512, 512),
      (512, 512), (512, 512)]
TAPS = (1, 3, 6, 9, 12)


def make_weights(seed):
    """He-scaled convs, biases 0.1 randn, lin_l = |randn| / C_l * 4^l; drawn in the order w0, b0, w1, b1, .., lin0 .. lin4"""
    g = torch.Generator().manual_seed(seed)
    w = {}
    for i, (ci, co) in enumerate(CH):
        w["w%d" % i] = (torch.randn(co, ci, 3, 3, generator=g) * math.sqrt(2. / (ci * 9))).float()
        w["b%d" % i] = (0.1 * torch.randn(co, generator=g)).float()
    for l, t in enumerate(TAPS):
        c = CH[t][1]
        w["lin%d" % l] = (torch.randn(c, generator=g).abs() / c * 4.**l).float()
    return w


# (H, W) -> total, v_0 .. v_4
GOLDEN = {
    (16, 16): (3.730433699e-02, 1.280736334e-02, 7.882888952e-03, 6.656205394e-03, 6.510339765e-03, 3.447539541e-03),
    (17, 23): (4.044655451e-02, 1.241647664e-02, 8.491897848e-03, 7.222342533e-03, 7.205886291e-03, 5.109951196e-03),
    (35, 47): (5.702801050e-02, 1.233298590e-02, 1.042772434e-02, 8.882733044e-03, 8.026324159e-03, 1.735824305e-02),
    (67, 95): (6.307598900e-02, 1.153333374e-02, 1.068819377e-02, 1.088946759e-02, 9.939292645e-03, 2.002570125e-02),
    (130, 131): (6.848458592e-02, 1.112898391e-02, 1.100926300e-02, 1.214430702e-02, 1.215527975e-02, 2.204675224e-02),
    (200, 200): (7.545313509e-02, 1.093875722e-02, 1.094487455e-02, 1.267798229e-02, 1.369875919e-02, 2.719276184e-02),
}
# the stack case: a, b = pair2(67, 95, 5); A = [a, a.flip(0), a.flip(1)], B = [b, 0.8 b, 0.6 b], both rescaled by their own extrema
GOLDEN_STACK = (6.306582755e-02, 7.577634036e-02, 8.603002566e-02)
# one weight (layer, co, ci, kh, kw) of conv1_2 and one of conv5_3 for the tests of what the bars see: centre taps (never on
# padding, whatever the map's size) of channels that are alive at these inputs
ZERO_CONV1_2, ZERO_CONV5_3 = (1, 5, 3, 1, 1), (12, 9, 40, 1, 1)
SIZES = [(16, 16), (17, 23), (35, 47), (67, 95), (130, 131), (200, 200)]
REL_FLOOR = 1e-5


def flat_params(seed=7, zero=None):
    """make_weights(seed) as the flat vector of r2l_lpips_vgg_pack / metrics.lpips_vgg.  zero = (layer, co, ci, kh, kw): that one
    weight is set to 0 first (the tests of what the bars can see)."""
    from r2l_amd import metrics
    w = make_weights(seed)
    if zero is not None:
        assert w["w%d" % zero[0]][zero[1:]].item() != 0.
        w["w%d" % zero[0]][zero[1:]] = 0.
    return metrics.lpips_vgg_flatten([(w["w%d" % i], w["b%d" % i]) for i in range(13)], [w["lin%d" % i] for i in range(5)])


def stack_case():
    """-> A, B [3,67,95,3] fp32 in [0,1] and their extrema {min_A, max_A, min_B, max_B}"""
    a, b = pair2(67, 95, 5)
    A, B = torch.stack([a, a.flip(0), a.flip(1)]), torch.stack([b, 0.8 * b, 0.6 * b])
    return A, B, torch.stack([A.min(), A.max(), B.min(), B.max()])


def check_conditions(x64, params, layers64):
    """What keeps the bars honest, asserted on the fp64 features of a [K,H,W,3] stack: at every position of every layer the
    channel norm is at least 0.05 of that layer's median norm (so x / (n + 1e-10) amplifies no rounding), and every
    v_l >= 1e-4 (no layer hides behind another).  -> the smallest norm / median ratio"""
    from r2l_amd import metrics
    convs, _ = metrics.lpips_vgg_unflatten(params.double())
    worst = float("inf")
    for f in metrics._lpips_vgg_features(x64, convs):
        n = f.pow(2).sum(1).sqrt()
        worst = min(worst, (n.min() / n.median()).item())
    assert worst >= 0.05, worst
    assert layers64.min().item() >= 1e-4, layers64
    return worst


def yardstick(a, b, params, rescale=None):
    """CPU fp64 and fp32 evaluations of [K,H,W,3] fp32 stacks (values in [-1, 1], or any with rescale) -> dict with the fp64
    'total' [K], 'layers' [K,5], 'maps' (five [K,Ho,Wo]), the bars 'bar_total' [K], 'bar_layers' [K,5], 'bar_maps' (five floats)
    and the fp32 branch's own relative differences 'rel_layers' (max per layer value) and 'rel_maps' (max per position, of the
    map's maximum); asserts the conditions above on both stacks."""
    from r2l_amd import metrics
    r64 = rescale.double() if rescale is not None else None
    t64, l64, m64 = metrics.lpips_vgg(a.double(), b.double(), params.double(), rescale=r64, return_layers=True, return_maps=True)
    t32, l32, m32 = metrics.lpips_vgg(a, b, params, rescale=rescale, return_layers=True, return_maps=True)
    assert t32.dtype == torch.float32 and t64.dtype == torch.float64
    xa, xb = a.double(), b.double()
    if r64 is not None:
        xa, xb = 2 / (r64[1] - r64[0]) * (xa - r64[0]) - 1, 2 / (r64[3] - r64[2]) * (xb - r64[2]) - 1
    ratio = min(check_conditions(xa, params, l64), check_conditions(xb, params, l64))
    return {"total": t64, "layers": l64, "maps": m64, "ratio": ratio,
            "rel_layers": ((l32.double() - l64).abs() / l64).max().item(),
            "rel_maps": max(((p.double() - q).abs().max() / q.max()).item() for p, q in zip(m32, m64)),
            "bar_total": torch.maximum(4 * (t32.double() - t64).abs(), REL_FLOOR * t64.abs()),
            "bar_layers": torch.maximum(4 * (l32.double() - l64).abs(), REL_FLOOR * l64.abs()),
            "bar_maps": [max(4 * (p.double() - q).abs().max().item(), REL_FLOOR * q.max().item()) for p, q in zip(m32, m64)]}


_YARD = {}


def yard(size):
    """(a, b [1,H,W,3] in [-1, 1], the yardstick of flat_params()) at one of SIZES, computed once per process and not modified"""
    if size not in _YARD:
        a, b = pair2(size[0], size[1], 5)
        a, b = (2 * a - 1)[None], (2 * b - 1)[None]
        _YARD[size] = (a, b, yardstick(a, b, flat_params()))
    return _YARD[size]


def compare(tag, got, y):
    """got = (total [K], layers [K,5], maps) against the yardstick y: prints the observed errors, then asserts"""
    total, layers, maps = got
    et, el = (total.cpu().double() - y["total"]).abs(), (layers.cpu().double() - y["layers"]).abs()
    em = [(m.cpu().double() - q).abs().max().item() for m, q in zip(maps, y["maps"])]
    print("%s: total %.2e (bar %.2e); layers %s (bars %s); maps %s (bars %s)" % (
        tag, et.max().item(), y["bar_total"].min().item(), " ".join("%.1e" % v for v in el.max(0).values.tolist()),
        " ".join("%.1e" % v for v in y["bar_layers"].min(0).values.tolist()), " ".join("%.1e" % v for v in em),
        " ".join("%.1e" % v for v in y["bar_maps"])))
    assert (et <= y["bar_total"]).all() and (el <= y["bar_layers"]).all()
    assert all(e <= bar for e, bar in zip(em, y["bar_maps"]))


def misses(got, y):
    """-> the largest miss of (layers [K,5], maps) in units of the bars: > 1 means outside"""
    layers, maps = got
    over = ((layers.cpu().double() - y["layers"]).abs() / y["bar_layers"]).max().item()
    for m, q, bar in zip(maps, y["maps"], y["bar_maps"]):
        over = max(over, (m.cpu().double() - q).abs().max().item() / bar)
    return over
