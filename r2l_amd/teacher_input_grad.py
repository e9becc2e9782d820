"""The NeRF teacher's render differentiated in its RAYS (include/r2l_hip.h: r2l_raw2outputs_backward_scaled,
r2l_teacher_backward_input; csrc/r2l_teacher_train.hip).  The weights are frozen: nothing here forms a weight gradient.

With G_l the pre-activation gradient of layer l (as r2l_teacher_backward forms it) and gv that of the views layer:

    d_pe_xyz[P,63] = G_0 W_0 + G_5 W_5[:, 0:63]            d_pe_dir[P,27] = gv W_views[:, 256:283]
    d_x            = g_x + sum_k 2^k (cos(2^k x) g_sin_k - sin(2^k x) g_cos_k)      (L = 10 at x = o + d z, L = 4 at viewdirs)
    d_rays_o = sum_s d_pts     d_rays_d = sum_s z_s d_pts     d_viewdirs = sum_s d_dir
    dL/d|rays_d|   = sum_s dL/dalpha_s relu(sigma'_s) (z_{s+1} - z_s) exp(-relu(sigma'_s) dists_s)       (raw2outputs' interval scaling)
    fold_viewdirs  : d_rays_d += d_len rays_d/|rays_d| + (d_viewdirs - (d_viewdirs . v) v) / |rays_d|   for viewdirs = rays_d/|rays_d|

z is a constant: the coarse depths depend on near / far and the jitter only, the fine samples are detached as the reference
detaches z_samples.

input_grad_spec, raw2outputs_backward_spec and render_loss_grad_spec restate the calls in torch, in the dtype of their inputs:
the meaning of the CPU path and the yardstick of the tests.  TeacherRayGrad is the device path (the library calls one by one,
nothing synchronises) and render_rays_diff wraps it as a torch.autograd.Function for a loss of the caller's own.
"""
import torch

from . import _lib
from . import render
from ._lib import ptr as _ptr, stream as _stream

MAX_SAMPLES = 256  # the raw2outputs backward stages one ray's samples in LDS
L_XYZ, L_DIR = 10, 4
STASH_SLOT = 256  # floats per point of a stash slot (csrc/r2l_teacher_net.h)


# ---- restatements ---------------------------------------------------------------------------------------------------------------
def _sd(net):
    return net if isinstance(net, dict) else {k: v.detach() for k, v in net.state_dict().items()}


def embed(x, L):
    """[x, sin 2^0 x, cos 2^0 x, ...]: the three coordinates together per term (helpers:24-74)."""
    out = [x]
    for k in range(L):
        out += [torch.sin(x * 2.0**k), torch.cos(x * 2.0**k)]
    return torch.cat(out, -1)


def embed_backward(x, g, L):
    """d_x [n,3] from g [n, 3 + 6L] = dL/d embed(x, L)."""
    d = g[:, 0:3].clone()
    for k in range(L):
        f = 2.0**k
        d = d + f * (torch.cos(x * f) * g[:, 3 + 6 * k:6 + 6 * k] - torch.sin(x * f) * g[:, 6 + 6 * k:9 + 6 * k])
    return d


def layer_outputs(sd, pe_x, pe_d):
    """What the training stash holds: relu(h0..h7), the feature, relu(views)."""
    h, outs = pe_x, []
    for i in range(8):
        h = torch.relu(h @ sd["pts_linears.%d.weight" % i].T + sd["pts_linears.%d.bias" % i])
        outs.append(h)
        if i == 4:
            h = torch.cat([pe_x, h], -1)
    feat = h @ sd["feature_linear.weight"].T + sd["feature_linear.bias"]
    v = torch.relu(torch.cat([feat, pe_d], -1) @ sd["views_linears.0.weight"].T + sd["views_linears.0.bias"])
    return outs + [feat, v]


def raw_from_outputs(sd, outs):
    rgb = outs[9] @ sd["rgb_linear.weight"].T + sd["rgb_linear.bias"]
    alpha = outs[7] @ sd["alpha_linear.weight"].T + sd["alpha_linear.bias"]
    return torch.cat([rgb, alpha], -1)


def stash_masks(stash, P):
    """The ReLU masks of a device stash of P points: [layer 0..7 ([P,256] bool)], views ([P,128] bool)."""
    body = [stash[l * P * STASH_SLOT:(l + 1) * P * STASH_SLOT].view(P, STASH_SLOT) > 0 for l in range(8)]
    return body, stash[9 * P * STASH_SLOT:9 * P * STASH_SLOT + P * 128].view(P, 128) > 0


def encoding_grads(W, body, views, dr):
    """(d_pe_xyz [P,63], d_pe_dir [P,27]) from dr [P,4] = dL/draw: the dX chain and the three input-side products.  W: the weights
    (a state dict in dr's dtype), body / views: the ReLU masks in dr's dtype (or bool)."""
    drgb, dsig = dr[:, :3], dr[:, 3:4]
    gv = (drgb @ W["rgb_linear.weight"]) * views
    Wv = W["views_linears.0.weight"]
    d_pe_dir = gv @ Wv[:, 256:]
    G = gv @ Wv[:, :256]
    G = (G @ W["feature_linear.weight"] + dsig * W["alpha_linear.weight"]) * body[7]
    d_pe_x = None
    for l in range(7, 0, -1):
        Wl = W["pts_linears.%d.weight" % l]
        nx = 63 if l == 5 else 0
        if nx:
            d_pe_x = G @ Wl[:, :nx]
        G = (G @ Wl[:, nx:]) * body[l - 1]
    return G @ W["pts_linears.0.weight"] + d_pe_x, d_pe_dir


def input_grad_spec(sd, rays_o, rays_d, viewdirs, z, stash, draw, d_len=None, fold_viewdirs=False, pts=None):
    """r2l_teacher_backward_input restated: (d_rays_o, d_rays_d, d_viewdirs, d_pts) in the dtype of rays_o.  stash: the device's
    (its ReLU masks are used, promoted) or None (the masks of this function's own forward).  pts [R,S,3]: the points to encode
    instead of rays_o + rays_d z (a test passes the fp32-rounded ones in fp64)."""
    dt = rays_o.dtype
    R, S = z.shape
    P = R * S
    W = {k: v.to(dt) for k, v in _sd(sd).items()}
    z = z.to(dt)
    x = (rays_o[:, None, :] + rays_d[:, None, :] * z[:, :, None] if pts is None else pts.to(dt)).reshape(P, 3)
    vd = viewdirs[:, None, :].expand(R, S, 3).reshape(P, 3)
    if stash is None:
        outs = layer_outputs(W, embed(x, L_XYZ), embed(vd, L_DIR))
        body, views = [o > 0 for o in outs[:8]], outs[9] > 0
    elif isinstance(stash, (tuple, list)):  # the masks themselves: ([8 x [P,256]], [P,128])
        body, views = stash
    else:
        body, views = stash_masks(stash, P)
    body, views = [m.to(dt) for m in body], views.to(dt)
    d_pe_x, d_pe_d = encoding_grads(W, body, views, draw.reshape(P, 4).to(dt))
    d_pts = embed_backward(x, d_pe_x, L_XYZ).view(R, S, 3)
    d_vd = embed_backward(vd, d_pe_d, L_DIR).view(R, S, 3).sum(1)
    d_o = d_pts.sum(1)
    d_d = (d_pts * z[:, :, None]).sum(1)
    dn = rays_d.norm(dim=-1, keepdim=True)
    if d_len is not None:
        d_d = d_d + d_len.to(dt)[:, None] * (rays_d / dn)
    if fold_viewdirs:
        d_d = d_d + (d_vd - (d_vd * viewdirs).sum(-1, keepdim=True) * viewdirs) / dn
    return d_o, d_d, d_vd, d_pts


def raw2outputs_backward_spec(raw, z, rays_d, noise, white_bkgd, target=None, g=None, grad_scale=None):
    """r2l_raw2outputs_backward_scaled restated in closed form: (draw [R,S,4], sqerr [R] or None, d_len [R], rgb_map [R,3]).
    g [R,3] given: it is dL/drgb_map; else dL/drgb_map = grad_scale (rgb_map - target), grad_scale = 2 / (3R) by default."""
    dt = raw.dtype
    R, S = z.shape
    dn = rays_d.norm(dim=-1, keepdim=True)
    dz = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], 1e10)], -1)
    dists = dz * dn
    sig = raw[..., 3] if noise is None else raw[..., 3] + noise.to(dt)
    ex = torch.exp(-torch.relu(sig) * dists)
    a = 1. - ex
    t = (1. - a) + 1e-10
    T = torch.cumprod(torch.cat([torch.ones_like(a[:, :1]), t], -1), -1)[:, :-1]
    w = a * T
    sg = torch.sigmoid(raw[..., :3])
    rgb_map = (w[..., None] * sg).sum(1)
    if white_bkgd:
        rgb_map = rgb_map + (1. - w.sum(-1, keepdim=True))
    sqerr = None
    if g is None:
        diff = rgb_map - target.to(dt)
        sqerr = (diff * diff).sum(-1)
        g = (2.0 / (3.0 * R) if grad_scale is None else grad_scale) * diff
    g = g.to(dt)
    e = (sg * g[:, None, :]).sum(-1) - (g.sum(-1, keepdim=True) if white_bkgd else 0.)
    dLda = torch.zeros_like(a)
    U = torch.zeros_like(a[:, 0])
    for k in range(S - 1, -1, -1):  # cumprod's backward by suffix sums: no division by 1 - alpha
        dLda[:, k] = T[:, k] * (e[:, k] - U)
        U = e[:, k] * a[:, k] + t[:, k] * U
    live = (sig > 0).to(dt)
    draw = torch.cat([w[..., None] * g[:, None, :] * (sg * (1. - sg)), (dLda * live * dists * ex)[..., None]], -1)
    d_len = (dLda * live * (sig * dz) * ex).sum(-1)
    return draw, sqerr, d_len, rgb_map


def render_loss_grad_spec(coarse, fine, rays_o, rays_d, viewdirs, near, far, target, N_samples, N_importance, white_bkgd=False,
                          grad_scale=None, t_rand=None, u=None, noise=None, fold_viewdirs=False, g=None):
    """The whole map rays -> loss restated on CPU tensors, in the dtype of rays_o: the objective is
    grad_scale / 2 * (sum (rgb - target)^2 + sum (rgb0 - target)^2) = img2mse(rgb) + img2mse(rgb0) at the default 2 / (3R).
    coarse / fine: modules or state dicts (fine None or N_importance 0: one network).  t_rand given: the stratified jitter
    (perturb 1), else perturb 0; u: the uniforms of the hierarchical sampling (None: linspace).  noise: None or the list of the
    sigma noise per network ([R,S] each, already scaled).  g: None, or the list of dL/drgb_map per network IN PLACE of the loss
    (coarse first; with two networks g[0] seeds rgb0 and g[1] rgb_map).
    Returns dict(loss, d_rays_o, d_rays_d, d_viewdirs, rgb_map, rgb0 (or None), z (list), sqerr (list), parts (per network))."""
    dt = rays_o.dtype
    R = rays_o.shape[0]
    nets = [_sd(coarse)] + ([_sd(fine)] if fine is not None and N_importance > 0 else [])
    nets = [{k: v.to(dt) for k, v in sd.items()} for sd in nets]
    near = torch.as_tensor(near, dtype=dt).expand(R, 1) if not torch.is_tensor(near) or near.dim() < 2 else near.to(dt)
    far = torch.as_tensor(far, dtype=dt).expand(R, 1) if not torch.is_tensor(far) or far.dim() < 2 else far.to(dt)
    perturb = 0. if t_rand is None else 1.
    zs = [render._coarse_z(near, far, N_samples, False, perturb, False, t_rand)]
    noise = noise or [None] * len(nets)

    def forward(sd, z):
        P = R * z.shape[1]
        x = (rays_o[:, None, :] + rays_d[:, None, :] * z[:, :, None]).reshape(P, 3)
        vd = viewdirs[:, None, :].expand(R, z.shape[1], 3).reshape(P, 3)
        return raw_from_outputs(sd, layer_outputs(sd, embed(x, L_XYZ), embed(vd, L_DIR))).view(R, z.shape[1], 4)

    raws = [forward(nets[0], zs[0])]
    if len(nets) > 1:
        weights = render.raw2outputs(raws[0], zs[0], rays_d, white_bkgd=white_bkgd, noise=noise[0])[3]
        uu = None if u is None else u.to(dt)
        if uu is None:
            uu = torch.linspace(0., 1., steps=N_importance).to(dt)
        zs.append(render.sample_pdf_sort(zs[0], weights, N_importance, det=True, u=uu)[1])
        raws.append(forward(nets[1], zs[1]))
    tot = dict(d_rays_o=0., d_rays_d=0., d_viewdirs=0.)
    loss, rgbs, sq, parts = 0., [], [], []
    s = 2.0 / (3.0 * R) if grad_scale is None else grad_scale
    for i, sd in enumerate(nets):
        draw, sqerr, d_len, rgb = raw2outputs_backward_spec(raws[i], zs[i], rays_d, noise[i], white_bkgd, target,
                                                            None if g is None else g[i], s)
        d_o, d_d, d_vd, d_pts = input_grad_spec(sd, rays_o, rays_d, viewdirs, zs[i], None, draw, d_len=d_len,
                                                fold_viewdirs=fold_viewdirs)
        tot["d_rays_o"], tot["d_rays_d"], tot["d_viewdirs"] = tot["d_rays_o"] + d_o, tot["d_rays_d"] + d_d, tot["d_viewdirs"] + d_vd
        if sqerr is not None:
            loss = loss + 0.5 * s * sqerr.sum()
        rgbs.append(rgb)
        sq.append(sqerr)
        parts.append(dict(draw=draw, d_len=d_len, d_rays_o=d_o, d_rays_d=d_d, d_viewdirs=d_vd, d_pts=d_pts, raw=raws[i]))
    return dict(loss=loss, rgb_map=rgbs[-1], rgb0=rgbs[0] if len(nets) > 1 else None, z=zs, sqerr=sq, parts=parts, **tot)


# ---- the device path --------------------------------------------------------------------------------------------------------------
class TeacherRayGrad:
    """Gradients of the frozen teacher's render with respect to rays_o, rays_d and viewdirs.

    loss_and_grad(...) -> (loss_out, d_rays_o, d_rays_d, d_viewdirs) for the objective grad_scale / 2 * (|rgb - target|^2 +
    |rgb0 - target|^2) (img2mse(rgb) + img2mse(rgb0) at the default grad_scale = 2 / (3R)).  On ROCm tensors: stratified z ->
    coarse forward with stash -> r2l_raw2outputs (weights) -> r2l_sample_pdf_sort -> fine forward with stash -> per network
    r2l_raw2outputs_backward_scaled + r2l_teacher_backward_input -> the two gradients summed.  Buffers grow on demand and are
    reused: the returned tensors are views that the next call overwrites.  Nothing synchronises.  loss_out (device [2]) = [the
    objective, psnr of the last network's mse]; last_z = the sample depths (coarse, fine).
    On CPU modules it is render_loss_grad_spec in fp32."""

    def __init__(self, coarse, fine=None, N_samples=64, N_importance=128, white_bkgd=True, raw_noise_std=0.):
        if N_importance > 0 and fine is None:
            raise NotImplementedError("N_importance > 0 without a fine network: the reference re-uses network_fn; not supported")
        self.nets = [coarse] + ([fine] if fine is not None and N_importance > 0 else [])
        self.N_samples, self.N_importance = int(N_samples), int(N_importance) if len(self.nets) > 1 else 0
        self.white_bkgd, self.raw_noise_std = bool(white_bkgd), float(raw_noise_std)
        p0 = next(coarse.parameters())
        self.device, self.on_gpu = p0.device, p0.is_cuda
        self.last_z = []
        self.generation = 0  # counts forward(): a backward on an older state's buffers is refused
        if not self.on_gpu:
            return
        S = self.N_samples + self.N_importance
        if S > MAX_SAMPLES:
            raise ValueError("the teacher's ray gradient takes at most %d samples per ray (N_samples + N_importance), got %d"
                             % (MAX_SAMPLES, S))
        self.lib = _lib.load()
        self.engines = [render.teacher_engine(net) for net in self.nets]
        for eng in self.engines:
            if eng.cfg.precision not in (_lib.PRECISION["auto"], _lib.PRECISION["fp32_mfma"]):
                raise NotImplementedError("the teacher's ray gradient is exact fp32 (precision auto | fp32_mfma), the engine is set "
                                          "to %s" % [k for k, v in _lib.PRECISION.items() if v == eng.cfg.precision][0])
        for net in self.nets:  # frozen
            for p in net.parameters():
                p.requires_grad_(False)
        self._bufs = {}
        self.loss_out = torch.zeros(2, dtype=torch.float32, device=self.device)

    def _buf(self, name, n):
        b = self._bufs.get(name)
        if b is None or b.numel() < n:
            b = torch.empty(n, dtype=torch.float32, device=self.device)
            self._bufs[name] = b
        return b[:n]

    def _noise(self, R, S):
        if self.raw_noise_std <= 0.:
            return None
        return torch.randn(R, S, device=self.device) * self.raw_noise_std

    # ---- stages ---------------------------------------------------------------------------------------------------------------
    def _mlp(self, i, rays_o, rays_d, viewdirs, z):
        eng = self.engines[i]
        eng.ensure_packed()
        R, S = z.shape
        raw = self._buf("raw%d" % i, R * S * 4)
        stash = self._buf("stash%d" % i, self.lib.r2l_teacher_stash_floats(R * S))
        _lib.check(self.lib.r2l_teacher_mlp_train(_ptr(rays_o), _ptr(rays_d), _ptr(viewdirs), _ptr(z), _ptr(eng.wstream),
                                                  _ptr(eng.flat), _ptr(raw), _ptr(stash), R, S, _stream(self.device)),
                   "r2l_teacher_mlp_train")
        return raw.view(R, S, 4), stash

    def forward(self, rays_o, rays_d, viewdirs, near, far, t_rand=None, u=None):
        """Steps 1 - 5: the state the backward needs (rays, z, raw, stash and noise per network)."""
        f32 = dict(dtype=torch.float32, device=self.device)
        rays_o, rays_d, viewdirs = [t.detach().to(**f32).contiguous() for t in (rays_o, rays_d, viewdirs)]
        R = rays_o.shape[0]
        near = torch.as_tensor(near, **f32).expand(R, 1).contiguous()
        far = torch.as_tensor(far, **f32).expand(R, 1).contiguous()
        z = render._coarse_z(near, far, self.N_samples, False, 0. if t_rand is None else 1., False, t_rand)
        self.generation += 1
        st = dict(rays=(rays_o, rays_d, viewdirs), z=[z], noise=[self._noise(R, self.N_samples)], raw=[], stash=[],
                  generation=self.generation)
        raw, stash = self._mlp(0, rays_o, rays_d, viewdirs, z)
        st["raw"].append(raw)
        st["stash"].append(stash)
        if len(self.nets) > 1:
            weights = render.raw2outputs(raw, z, rays_d, noise=st["noise"][0], white_bkgd=self.white_bkgd)[3]
            if u is None:
                u = self._bufs.get("u_det")
                if u is None:
                    u = self._bufs["u_det"] = torch.linspace(0., 1., steps=self.N_importance).to(**f32)
            z_all = render.sample_pdf_sort(z, weights, self.N_importance, det=True, u=u)[1]
            st["z"].append(z_all)
            st["noise"].append(self._noise(R, z_all.shape[1]))
            raw, stash = self._mlp(1, rays_o, rays_d, viewdirs, z_all)
            st["raw"].append(raw)
            st["stash"].append(stash)
        self.last_z = st["z"]
        return st

    def rgb_maps(self, st):
        """rgb_map of every network of a forward state (coarse first), by r2l_raw2outputs."""
        return [render.raw2outputs(st["raw"][i], st["z"][i], st["rays"][1], noise=st["noise"][i], white_bkgd=self.white_bkgd,
                                   need_weights=False)[0] for i in range(len(self.nets))]

    def backward(self, st, target=None, grad_scale=None, g=None, fold_viewdirs=False, with_len=True):
        """Steps 6 - 7 on a forward state: (d_rays_o, d_rays_d, d_viewdirs, [sqerr per network]).  target + grad_scale: the MSE
        seed; g: the list of dL/drgb_map per network (coarse first) in its place.  with_len: the |rays_d| term of raw2outputs'
        intervals goes into d_rays_d."""
        lib, dev = self.lib, self.device
        if st["generation"] != self.generation:
            raise RuntimeError("TeacherRayGrad.backward: this state is of forward %d, the buffers now hold forward %d's raw and stash "
                               "(a later render on the same networks overwrote them); run the backward before rendering again"
                               % (st["generation"], self.generation))
        rays_o, rays_d, viewdirs = st["rays"]
        R = rays_o.shape[0]
        out = [self._buf(k, 2 * R * 3).view(2, R, 3) for k in ("d_rays_o", "d_rays_d", "d_viewdirs")]
        sq = []
        for i in range(len(self.nets)):
            z = st["z"][i]
            S = z.shape[1]
            draw = self._buf("draw", R * S * 4)
            d_len = self._buf("d_len", R) if with_len else None
            sqerr = None
            if g is None:
                sqerr = self._buf("sqerr%d" % i, R)
            _lib.check(lib.r2l_raw2outputs_backward_scaled(_ptr(st["raw"][i]), _ptr(z), _ptr(rays_d), _ptr(st["noise"][i]),
                                                           int(self.white_bkgd), _ptr(target), _ptr(None if g is None else g[i]),
                                                           0. if grad_scale is None else float(grad_scale), _ptr(draw), _ptr(sqerr),
                                                           _ptr(d_len), R, S, _stream(dev)), "r2l_raw2outputs_backward_scaled")
            work = self._buf("work", lib.r2l_teacher_input_grad_work_floats(R * S))
            _lib.check(lib.r2l_teacher_backward_input(_ptr(rays_o), _ptr(rays_d), _ptr(viewdirs), _ptr(z), _ptr(self.engines[i].flat),
                                                      _ptr(st["stash"][i]), _ptr(draw), _ptr(d_len), int(bool(fold_viewdirs)),
                                                      _ptr(out[0][i]), _ptr(out[1][i]), _ptr(out[2][i]), None, _ptr(work), R, S,
                                                      _stream(dev)), "r2l_teacher_backward_input")
            sq.append(sqerr)
        if len(self.nets) > 1:
            for o in out:
                o[0].add_(o[1])
        return out[0][0], out[1][0], out[2][0], sq

    def loss_and_grad(self, rays_o, rays_d, viewdirs, near, far, target, grad_scale=None, t_rand=None, u=None, fold_viewdirs=False):
        R = rays_o.shape[0]
        s = 2.0 / (3.0 * R) if grad_scale is None else float(grad_scale)
        if not self.on_gpu:
            return self._cpu(rays_o, rays_d, viewdirs, near, far, target, s, t_rand, u, fold_viewdirs)
        st = self.forward(rays_o, rays_d, viewdirs, near, far, t_rand, u)
        target = target.detach().to(dtype=torch.float32, device=self.device).contiguous()
        d_o, d_d, d_vd, sq = self.backward(st, target=target, grad_scale=s, fold_viewdirs=fold_viewdirs)
        outs = []
        for i, sqerr in enumerate(sq):
            o = self._buf("mse%d" % i, 2)
            _lib.check(self.lib.r2l_loss_finish(_ptr(sqerr), R, 0.5 * s, _ptr(o), _stream(self.device)), "r2l_loss_finish")
            outs.append(o)
        self.loss_out[0] = sum(o[0] for o in outs)
        self.loss_out[1] = outs[-1][1]
        self.last_sqerr = sq
        self.last_state = st
        return self.loss_out, d_o, d_d, d_vd

    def _cpu(self, rays_o, rays_d, viewdirs, near, far, target, s, t_rand, u, fold_viewdirs):
        R = rays_o.shape[0]
        noise = None
        if self.raw_noise_std > 0.:
            noise = [torch.randn(R, self.N_samples) * self.raw_noise_std] + (
                [torch.randn(R, self.N_samples + self.N_importance) * self.raw_noise_std] if len(self.nets) > 1 else [])
        with torch.no_grad():
            r = render_loss_grad_spec(self.nets[0], self.nets[1] if len(self.nets) > 1 else None, rays_o.float(), rays_d.float(),
                                      viewdirs.float(), near, far, target.float(), self.N_samples, self.N_importance,
                                      self.white_bkgd, s, t_rand, u, noise=noise, fold_viewdirs=fold_viewdirs)
        self.last_z, self.last_sqerr = r["z"], r["sqerr"]
        mse = 0.5 * s * r["sqerr"][-1].sum()
        loss_out = torch.stack([r["loss"], -10. * torch.log10(mse)])
        return loss_out, r["d_rays_o"], r["d_rays_d"], r["d_viewdirs"]


class _RenderRaysDiff(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rays_o, rays_d, viewdirs, rg, near, far, t_rand, u):
        st = rg.forward(rays_o, rays_d, viewdirs, near, far, t_rand, u)
        rgbs = rg.rgb_maps(st)
        ctx.rg, ctx.st = rg, st
        ctx.types = [(t.dtype, t.device) for t in (rays_o, rays_d, viewdirs)]
        return rgbs[-1], (rgbs[0] if len(rgbs) > 1 else torch.zeros_like(rgbs[0]))

    @staticmethod
    def backward(ctx, g_rgb, g_rgb0):
        rg, st = ctx.rg, ctx.st
        f32 = dict(dtype=torch.float32, device=rg.device)
        g = [g_rgb.to(**f32).contiguous()] if len(rg.nets) == 1 else [g_rgb0.to(**f32).contiguous(), g_rgb.to(**f32).contiguous()]
        d_o, d_d, d_vd, _ = rg.backward(st, g=g, fold_viewdirs=False)
        outs = [t.clone().to(dtype=dt, device=dev) for t, (dt, dev) in zip((d_o, d_d, d_vd), ctx.types)]
        return outs[0], outs[1], outs[2], None, None, None, None, None


def render_rays_diff(rays_o, rays_d, viewdirs, near, far, coarse, fine=None, N_samples=64, N_importance=128, white_bkgd=False,
                     raw_noise_std=0., t_rand=None, u=None):
    """(rgb_map, rgb0) of the teacher's render_rays, differentiable in rays_o, rays_d and viewdirs — for a loss of the caller's
    own (rgb0 is zeros without a fine network).  The backward is r2l_raw2outputs_backward_scaled seeded with the upstream
    gradients and r2l_teacher_backward_input per network; viewdirs is an input of its own here, so a caller that normalises
    rays_d into it gets that derivative from autograd.  z is a constant (see the module's head).  The networks' PARAMETERS GET NO
    GRADIENT here: the teacher is frozen (its parameters are set to requires_grad False); train it with TeacherTrainer.  The
    state of a call lives in buffers the next call on the same networks reuses: call backward() before rendering again (a
    backward on an overwritten state raises).  The TeacherRayGrad behind a pair of networks is kept on the coarse module, beside
    its teacher engine, with its stash and work buffers; release_ray_grad(coarse) drops it.
    On CPU modules the same map is torch autograd through the restatement's forward."""
    if not next(coarse.parameters()).is_cuda:
        return _render_rays_diff_cpu(rays_o, rays_d, viewdirs, near, far, coarse, fine, N_samples, N_importance, white_bkgd,
                                     raw_noise_std, t_rand, u)
    key = (id(fine), int(N_samples), int(N_importance), bool(white_bkgd), float(raw_noise_std))
    cache = coarse.__dict__.setdefault("_r2l_ray_grad", {})
    rg = cache.get(key)
    if rg is None:
        rg = cache[key] = TeacherRayGrad(coarse, fine, N_samples, N_importance, white_bkgd, raw_noise_std)
    return _RenderRaysDiff.apply(rays_o, rays_d, viewdirs, rg, near, far, t_rand, u)


def release_ray_grad(coarse):
    """Drop the TeacherRayGrad objects render_rays_diff keeps on `coarse` (their stash and work buffers go with them)."""
    coarse.__dict__.pop("_r2l_ray_grad", None)


def _render_rays_diff_cpu(rays_o, rays_d, viewdirs, near, far, coarse, fine, N_samples, N_importance, white_bkgd, raw_noise_std,
                          t_rand, u):
    dt, R = rays_o.dtype, rays_o.shape[0]
    nets = [{k: v.to(dt) for k, v in _sd(n).items()} for n in ([coarse] + ([fine] if fine is not None and N_importance > 0 else []))]
    near = torch.as_tensor(near, dtype=dt).expand(R, 1)
    far = torch.as_tensor(far, dtype=dt).expand(R, 1)
    z = render._coarse_z(near, far, N_samples, False, 0. if t_rand is None else 1., False, t_rand)

    def rgb_of(sd, z):
        S = z.shape[1]
        x = (rays_o[:, None, :] + rays_d[:, None, :] * z[:, :, None]).reshape(R * S, 3)
        vd = viewdirs[:, None, :].expand(R, S, 3).reshape(R * S, 3)
        raw = raw_from_outputs(sd, layer_outputs(sd, embed(x, L_XYZ), embed(vd, L_DIR))).view(R, S, 4)
        noise = torch.randn(R, S) * raw_noise_std if raw_noise_std > 0. else None
        out = render.raw2outputs(raw, z, rays_d, white_bkgd=white_bkgd, noise=noise)
        return out[0], out[3]

    rgb0, weights = rgb_of(nets[0], z)
    if len(nets) == 1:
        return rgb0, torch.zeros_like(rgb0)
    uu = torch.linspace(0., 1., steps=N_importance).to(dt) if u is None else u.to(dt)
    z_all = render.sample_pdf_sort(z, weights.detach(), N_importance, det=True, u=uu)[1].detach()
    return rgb_of(nets[1], z_all)[0], rgb0
