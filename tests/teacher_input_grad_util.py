"""Yardsticks of the teacher's backward to its rays (r2l_teacher_backward_input, r2l_raw2outputs_backward_scaled;
r2l_amd/teacher_input_grad.py), shared by tests/test_teacher_input_grad_{cpu,gpu}.py.

want     : r2l_amd.teacher_input_grad.input_grad_spec in fp64 from given ReLU masks (the device's stash, promoted) at the
           fp32-rounded points o + d z (mul and add rounded separately, as the kernels form them).
mag      : the absolute backprop of tests/teacher_util.teacher_backward_from_stash (|draw|, |W|, the same masks) carried through
           the input-side products (|G| |W|), the encoder's derivative with sin / cos replaced by their bound 1 (so |phi'| <= 2^k),
           and the per-ray sums (|z_s|, |d_len| |d| / |d|, 1 / |d| for the folded view direction).
bar      : |got - want| <= C_IN * mag + floor per entry (floor = 1e-12 max(mag) + 1e-30: underflow only), and per tensor the
           norm-relative NREL_BWD of tests/test_teacher_backward_gpu.py.

C_IN is set the way C_T was (tests/teacher_util.py): input_grad32 below is a PINNED fp32 restatement — every product and sum
rounded to fp32 in a stated order, independent of the kernel: the matrix products by student_util.linear32 (fp32 accumulator,
two products at a time in the order of k), sin / cos correctly rounded, the encoder's derivative term by term in the order of k,
the per-ray sums sample by sample — run on the CPU over SHAPES and both weight kinds (init: seed 5; trained-like: the CPU fit of
teacher_util.forward_weights) against the fp64 spec with the same masks.  C_IN = 4 x the worst |e32| / mag seen; 4 is the margin
C_T keeps between two correct fp32 summation orders.  The table (tests/test_teacher_input_grad_cpu.py prints it; it holds the
pinned restatement within C_IN / 4 in every case):

  worst |e32| / mag per tensor          d_pts      d_rays_o   d_rays_d   d_viewdirs   (the case it was seen at)
  init          over SHAPES            6.7e-14    1.67e-14   1.68e-14   3.61e-8      (1031, 192) / (2049, 1) x 3
  trained-like  over SHAPES            3.26e-11   7.36e-12   7.06e-12   5.48e-8      (1031, 192) / (2049, 1) x 3
  C_IN = 4 x the worst                 1.31e-10   2.95e-11   2.83e-11   2.2e-7
C_IN is one number PER TENSOR: mag is an absolute backprop, and how far it lies above what rounding does depends on the depth of
the path (d_viewdirs is two products deep: 5e-8; d_pts ten: 3e-11, the |W| products of eight layers compound); one constant at
the shallow tensor's value would leave the deep ones without a per-entry bar.  With S samples a ray sum averages its samples'
errors (d_rays_o at (1031, 192): 8.7e-14), so the per-ray constants are set by S = 1, where d_rays_o IS d_pts.
"""
import torch

from r2l_amd import teacher_input_grad as TI
from tests.student_util import linear32
from tests.teacher_util import points32

SHAPES = [(1, 1), (1, 15), (1, 129), (3, 43), (2, 64), (37, 61), (5, 192), (11, 256), (2049, 1), (1031, 192)]
SELF_CHECK_SHAPES = [(3, 43), (37, 61)]
C_IN = {"d_pts": 1.31e-10, "d_rays_o": 2.95e-11, "d_rays_d": 2.83e-11, "d_viewdirs": 2.2e-7}  # the table above
TENSORS = ("d_pts", "d_rays_o", "d_rays_d", "d_viewdirs")


def make_draw(raw, seed):
    """Random dL/draw [R,S,4] (CPU) with the sigma column zeroed where sigma <= 0 (relu' = 0 there in any real seed)."""
    g = torch.Generator().manual_seed(seed)
    draw = torch.randn(*raw.shape, generator=g) * 1e-3
    draw[..., 3][raw[..., 3].cpu() <= 0] = 0.
    return draw


def make_d_len(R, seed):
    return torch.randn(R, generator=torch.Generator().manual_seed(seed + 77)) * 1e-3


def want64(sd, o, d, vd, z, masks, draw, d_len=None, fold=False):
    """The fp64 spec from given masks at the fp32 points: dict of TENSORS, on the device of o."""
    dev = o.device
    f64 = lambda t: t.to(device=dev, dtype=torch.float64)
    R, S = z.shape
    pts = f64(points32(o, d, z)).view(R, S, 3)
    sd64 = {k: f64(v) for k, v in sd.items()}
    out = TI.input_grad_spec(sd64, f64(o), f64(d), f64(vd), f64(z), masks, f64(draw), None if d_len is None else f64(d_len), fold,
                             pts=pts)
    return dict(d_rays_o=out[0], d_rays_d=out[1], d_viewdirs=out[2], d_pts=out[3])


def mags64(sd, o, d, vd, z, masks, draw, d_len=None, fold=False):
    dev = o.device
    f64 = lambda t: t.to(device=dev, dtype=torch.float64)
    R, S = z.shape
    W = {k: f64(v).abs() for k, v in sd.items()}
    body, views = [f64(m) for m in masks[0]], f64(masks[1])
    m_x, m_d = TI.encoding_grads(W, body, views, f64(draw).abs().reshape(R * S, 4))

    def enc(m, L):  # |g_x| + sum_k 2^k (|g_sin_k| + |g_cos_k|)
        out = m[:, 0:3].clone()
        for k in range(L):
            out = out + 2.0**k * (m[:, 3 + 6 * k:6 + 6 * k] + m[:, 6 + 6 * k:9 + 6 * k])
        return out
    m_pts = enc(m_x, TI.L_XYZ).view(R, S, 3)
    m_vd = enc(m_d, TI.L_DIR).view(R, S, 3).sum(1)
    m_dd = (m_pts * f64(z).abs()[:, :, None]).sum(1)
    dn = f64(d).norm(dim=-1, keepdim=True)
    if d_len is not None:
        m_dd = m_dd + f64(d_len).abs()[:, None] * (f64(d).abs() / dn)
    if fold:
        v = f64(vd).abs()
        m_dd = m_dd + (m_vd + (m_vd * v).sum(-1, keepdim=True) * v) / dn
    return dict(d_pts=m_pts, d_rays_o=m_pts.sum(1), d_rays_d=m_dd, d_viewdirs=m_vd)


def input_grad32(sd, o, d, vd, z, masks, draw, d_len=None, fold=False):
    """THE pinned fp32 restatement (see the module's head): dict of TENSORS, fp32, CPU."""
    f = lambda t: t.detach().cpu().float()
    o, d, vd, z, draw = f(o), f(d), f(vd), f(z), f(draw)
    R, S = z.shape
    P = R * S
    W = {k: f(v) for k, v in sd.items()}
    body, views = [f(m) for m in masks[0]], f(masks[1])
    mm = lambda G, w: linear32(G.contiguous(), w.T.contiguous(), torch.zeros(w.shape[1]))  # G @ w, pinned
    dr = draw.reshape(P, 4)
    wr = W["rgb_linear.weight"]
    gv = ((dr[:, 0:1] * wr[0] + dr[:, 1:2] * wr[1]) + dr[:, 2:3] * wr[2]) * views
    Wv = W["views_linears.0.weight"]
    d_pe_d = mm(gv, Wv[:, 256:])
    G = mm(gv, Wv[:, :256])
    G = (mm(G, W["feature_linear.weight"]) + dr[:, 3:4] * W["alpha_linear.weight"]) * body[7]
    d_pe_x = None
    for l in range(7, 0, -1):
        Wl = W["pts_linears.%d.weight" % l]
        nx = 63 if l == 5 else 0
        if nx:
            d_pe_x = mm(G, Wl[:, :nx])
        G = mm(G, Wl[:, nx:]) * body[l - 1]
    d_pe_x = d_pe_x + mm(G, W["pts_linears.0.weight"])

    def enc(x32, g, L):  # sin / cos of the fp32 argument, correctly rounded; the terms in the order of k
        acc = g[:, 0:3].clone()
        for k in range(L):
            fk = 2.0**k
            a = (x32 * fk).double()
            cs, sn = torch.cos(a).float(), torch.sin(a).float()
            acc = acc + fk * (cs * g[:, 3 + 6 * k:6 + 6 * k] - sn * g[:, 6 + 6 * k:9 + 6 * k])
        return acc
    d_pts = enc(points32(o, d, z), d_pe_x, TI.L_XYZ).view(R, S, 3)
    d_dir = enc(vd[:, None, :].expand(R, S, 3).reshape(P, 3), d_pe_d, TI.L_DIR).view(R, S, 3)
    so, sdd, sv = torch.zeros(R, 3), torch.zeros(R, 3), torch.zeros(R, 3)
    for s in range(S):  # sample by sample
        so = so + d_pts[:, s]
        sdd = sdd + z[:, s:s + 1] * d_pts[:, s]
        sv = sv + d_dir[:, s]
    dn = (d[:, 0:1] * d[:, 0:1] + d[:, 1:2] * d[:, 1:2] + d[:, 2:3] * d[:, 2:3]).sqrt()
    if d_len is not None:
        sdd = sdd + f(d_len)[:, None] * (d / dn)
    if fold:
        dot = (sv[:, 0:1] * vd[:, 0:1] + sv[:, 1:2] * vd[:, 1:2]) + sv[:, 2:3] * vd[:, 2:3]
        sdd = sdd + (sv - dot * vd) / dn
    return dict(d_pts=d_pts, d_rays_o=so, d_rays_d=sdd, d_viewdirs=sv)


def floor_of(mag):
    return 1e-12 * mag.max().item() + 1e-30


def ratios(got, want, mags):
    """{tensor: [entries] |got - want| / (mag + floor / C_IN)}: the bar is ratio <= C_IN[tensor] (a NaN reads inf)."""
    out = {}
    for k in got:
        m = mags[k].to(want[k].device)
        e = (got[k].to(want[k].device).double().reshape(want[k].shape) - want[k]).abs()
        out[k] = torch.nan_to_num(e / (m + floor_of(m) / C_IN[k]), nan=float("inf"))
    return out


def violations(got, want, mags, c=None):
    """{tensor: bool mask of the entries beyond |got - want| <= c[tensor] * mag + floor} (c: C_IN)."""
    c = C_IN if c is None else c
    out = {}
    for k in got:
        m = mags[k].to(want[k].device)
        e = (got[k].to(want[k].device).double().reshape(want[k].shape) - want[k]).abs()
        out[k] = ~(e <= c[k] * m + floor_of(m))
    return out


def nrel(a, b):
    return ((a.double() - b.double().to(a.device)).norm() / b.double().norm().clamp_min(1e-300)).item()


# ---- fp64 autograd through render.render_rays' CPU branch ---------------------------------------------------------------------
def nerf_module(sd, dtype=torch.float64):
    from r2l_amd.nerf_raybased import NeRF
    m = NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=4, skips=[4], use_viewdirs=True)
    m.load_state_dict(sd)
    return m.to(dtype)


def render_autograd(nets, o, d, vd, near, far, N_samples, N_importance, white_bkgd, t_rand=None, u=None, raw_noise_std=0.):
    """render.render_rays' CPU branch on leaf tensors: (ret, leaves).  vd None: viewdirs = d / |d| inside the graph."""
    from r2l_amd import render
    o, d = o.detach().clone().requires_grad_(True), d.detach().clone().requires_grad_(True)
    v = None if vd is None else vd.detach().clone().requires_grad_(True)
    vv = d / d.norm(dim=-1, keepdim=True) if v is None else v
    ones = torch.ones_like(o[:, :1])
    batch = torch.cat([o, d, near * ones, far * ones, vv], -1)
    qfn = lambda inputs, vdirs, fn: render.run_network(inputs, vdirs, fn, embed_fn=render.get_embedder(10)[0],
                                                      embeddirs_fn=render.get_embedder(4)[0])
    ret = render.render_rays(batch, nets[0], qfn, N_samples, perturb=0. if t_rand is None else 1., N_importance=N_importance,
                             network_fine=nets[1] if len(nets) > 1 else None, white_bkgd=white_bkgd, raw_noise_std=raw_noise_std,
                             t_rand=t_rand, u=u)
    return ret, (o, d, v)

