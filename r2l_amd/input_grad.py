"""The student's gradient with respect to its input, restated in torch: the specification of csrc/r2l_input_grad.hip
(r2l_backward_input, include/r2l_hip.h) and the meaning of the CPU path, where autograd forms the same quantity op by op.

    d_emb[r][k]     = sum_o gh[r][o] * Wh[o][k]                       gh = dL/d(head pre-activation) [N,256], Wh = head.0.weight
    z[r][s]         = z_lower[s] + z_span[s] * t_rand[r][s]           (t_rand None: z_lower[s]);  ztab = z_lower[16] ++ z_span[16]
    x[r][s][a]      = o[r][a] + d[r][a] * z[r][s]
    d_pts[r][s][a]  = sum_f d_emb[r][(3 s + a) 21 + f] * phi'_f(x)    phi' = 2^f cos(2^f x) | -2^f sin(2^f x) | 1
    d_rays_o[r][a]  = sum_s d_pts[r][s][a]
    d_rays_d[r][a]  = sum_s z[r][s] * d_pts[r][s][a]

The column order is PositionalEmbedder's: per point coordinate ten sines, ten cosines, then the coordinate itself.  The jitter
t_rand and the depth table get no gradient."""
import torch

N_SAMPLE, L_PE = 16, 10


def input_grad_spec(gh, Wh, rays_o=None, rays_d=None, t_rand=None, ztab=None, pts=None, z=None):
    """(d_emb [N,1008], d_rays_o [N,3], d_rays_d [N,3]) in the dtype of gh; the last two are None without rays.
    pts [N,48] / z [N,16]: the sample points and depths to differentiate AT, when they are not to be formed here in gh's dtype
    (a test hands over the fp32-rounded ones a kernel saw)."""
    dt = gh.dtype
    d_emb = gh @ Wh.to(dt)
    if rays_o is None:
        return d_emb, None, None
    n = gh.shape[0]
    if z is None:
        zl, zs = ztab[:N_SAMPLE].to(dt), ztab[N_SAMPLE:].to(dt)
        z = zl + zs * t_rand.to(dt) if t_rand is not None else zl[None, :].expand(n, N_SAMPLE)
    z = z.to(dt)
    if pts is None:
        x = rays_o.to(dt)[:, None, :] + rays_d.to(dt)[:, None, :] * z[:, :, None]
    else:
        x = pts.to(dt).reshape(n, N_SAMPLE, 3)
    w = (2.0 ** torch.arange(L_PE, device=gh.device)).to(dt)
    ang = x[..., None] * w
    phi = torch.cat([w * torch.cos(ang), -w * torch.sin(ang), torch.ones_like(x[..., None])], dim=-1)  # [N,16,3,21]
    d_pts = (d_emb.reshape(n, N_SAMPLE, 3, 2 * L_PE + 1) * phi).sum(-1)
    return d_emb, d_pts.sum(1), (z[:, :, None] * d_pts).sum(1)
