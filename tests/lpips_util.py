"""Inputs, golden numbers and yardsticks shared by tests/test_lpips_cpu.py and tests/test_lpips_gpu.py.

The golden numbers come from an fp64 restatement of LPIPS(AlexNet, v0.1) written independently of r2l_amd.metrics, on
make_weights(7), pair2(H, W, 5) and inputs 2 x - 1.  Bars: for every layer value and the total
max(4 |CPU fp32 - CPU fp64|, 1e-5 |fp64 value|); for every map position max(4 max|CPU fp32 map - CPU fp64 map|,
1e-5 max of that fp64 map).  The 1e-5 floor is about 20 times the fp32-against-fp64 difference of the CPU evaluation at these
inputs (<= 4.5e-7 relative per layer) and well under what one wrong tap does where it reaches a layer (4e-5 .. 7e-4)."""
import math

import torch

CH = [(3,64,11,4,2),(64,192,5,1,2),(192,384,3,1,1),(384,256,3,1,1),(256,256,3,1,1)]
def make_weights(seed):            # He-scaled convs, small biases, non-negative lin weights (as the published ones are)
    g = torch.Generator().manual_seed(seed); w = {}
    for i,(ci,co,k,s,p) in enumerate(CH):
        w['w%d'%i] = (torch.randn(co,ci,k,k,generator=g)*math.sqrt(2./(ci*k*k))).float()
        w['b%d'%i] = (0.1*torch.randn(co,generator=g)).float()
        w['lin%d'%i] = (torch.randn(co,generator=g).abs()/co).float()
    return w
def pair2(H,W,seed):               # two unlike images in [0,1]; callers map them by 2x-1
    g = torch.Generator().manual_seed(seed)
    yy,xx = torch.meshgrid(torch.linspace(0,3,H),torch.linspace(0,4,W),indexing='ij')
    a = torch.stack([0.5+0.5*torch.sin(9.1*xx+5*yy),0.5+0.5*torch.cos(7.3*yy*xx),(xx/4.+yy/3.)/2.],-1)
    a = (a+0.3*torch.rand(H,W,3,generator=g)).clamp(0,1)
    b = torch.stack([0.5+0.5*torch.cos(6.3*xx-4*yy),(xx/4.)*(yy/3.),0.5+0.5*torch.sin(8.7*yy+xx*xx)],-1)
    b = (b+0.3*torch.rand(H,W,3,generator=g)).clamp(0,1)
    return a,b


# (H, W) -> total, v_0 .. v_4
GOLDEN = {
    (31, 31): (1.502155732e-02, 1.337132046e-02, 8.892524162e-04, 3.040711911e-04, 2.394022462e-04, 2.175110128e-04),
    (35, 47): (1.537770735e-02, 1.350923622e-02, 1.049686245e-03, 2.520855017e-04, 2.870428012e-04, 2.796565875e-04),
    (67, 95): (1.609671221e-02, 1.340782717e-02, 1.398915844e-03, 3.446430285e-04, 4.908668997e-04, 4.544592698e-04),
}
# the stack case: a, b = pair2(67, 95, 5); A = [a, a.flip(0), a.flip(1)], B = [b, 0.8 b, 0.6 b], both rescaled by their own extrema
GOLDEN_STACK = (1.611902405e-02, 1.833615236e-02, 2.362145735e-02)
GOLDEN_STACK_MIN = (0.0023290338, 0.0012929393)
SIZES = [(31, 31), (35, 47), (67, 95), (400, 400)]
REL_FLOOR = 1e-5


def flat_params(seed=7):
    """make_weights(seed) as the flat vector of r2l_lpips_pack / metrics.lpips."""
    from r2l_amd import metrics
    w = make_weights(seed)
    return metrics.lpips_flatten([(w["w%d" % i], w["b%d" % i]) for i in range(5)], [w["lin%d" % i] for i in range(5)])


def stack_case():
    """-> A, B [3,67,95,3] fp32 in [0,1] and their extrema {min_A, max_A, min_B, max_B}"""
    a, b = pair2(67, 95, 5)
    A, B = torch.stack([a, a.flip(0), a.flip(1)]), torch.stack([b, 0.8 * b, 0.6 * b])
    return A, B, torch.stack([A.min(), A.max(), B.min(), B.max()])


def check_conditions(x64, params, layers64):
    """What keeps the bars honest, asserted on the fp64 features of a [K,H,W,3] stack: at every position of every layer the
    channel norm is at least 0.05 of that layer's median norm (so x / (n + 1e-10) amplifies no rounding), and every
    v_l >= 1e-4 (no layer hides behind layer 0).  -> the smallest norm / median ratio"""
    from r2l_amd import metrics
    convs, _ = metrics.lpips_unflatten(params.double())
    worst = float("inf")
    for f in metrics._lpips_features(x64, convs):
        n = f.pow(2).sum(1).sqrt()
        worst = min(worst, (n.min() / n.median()).item())
    assert worst >= 0.05, worst
    assert layers64.min().item() >= 1e-4, layers64
    return worst


def yardstick(a, b, params, rescale=None):
    """CPU fp64 and fp32 evaluations of [K,H,W,3] fp32 stacks (values in [-1, 1], or any with rescale) -> dict with the fp64
    'total' [K], 'layers' [K,5], 'maps' (five [K,Ho,Wo]) and the bars 'bar_total' [K], 'bar_layers' [K,5], 'bar_maps' (five
    floats); asserts the conditions above on both stacks."""
    from r2l_amd import metrics
    r64 = rescale.double() if rescale is not None else None
    t64, l64, m64 = metrics.lpips(a.double(), b.double(), params.double(), rescale=r64, return_layers=True, return_maps=True)
    t32, l32, m32 = metrics.lpips(a, b, params, rescale=rescale, return_layers=True, return_maps=True)
    assert t32.dtype == torch.float32 and t64.dtype == torch.float64
    xa, xb = a.double(), b.double()
    if r64 is not None:
        xa, xb = 2 / (r64[1] - r64[0]) * (xa - r64[0]) - 1, 2 / (r64[3] - r64[2]) * (xb - r64[2]) - 1
    ratio = min(check_conditions(xa, params, l64), check_conditions(xb, params, l64))
    return {"total": t64, "layers": l64, "maps": m64, "ratio": ratio,
            "bar_total": torch.maximum(4 * (t32.double() - t64).abs(), REL_FLOOR * t64.abs()),
            "bar_layers": torch.maximum(4 * (l32.double() - l64).abs(), REL_FLOOR * l64.abs()),
            "bar_maps": [max(4 * (p.double() - q).abs().max().item(), REL_FLOOR * q.max().item()) for p, q in zip(m32, m64)]}
