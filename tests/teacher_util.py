"""Test infrastructure: a NeRF teacher whose weights have LEFT the init distribution.

No trained lego checkpoint can be downloaded here, so the teacher is fitted for a couple of thousand Adam steps (plain torch
autograd on the oracle's functional forward, on whatever device the caller picks) to an analytic scene with the statistics a
trained NeRF shows: sigma pre-activations from about -10^2 in empty space to 10^2 .. 10^3 inside surfaces, a sharp shell and
an opaque blob, view-dependent colour.  The kernels under test never see this code; they get the resulting state dict."""
import torch

from oracle import r2l_oracle as O


def analytic_targets(pts, dirs):
    """(logit-rgb [n,3], sigma pre-activation [n]) of the analytic scene at points / unit view directions."""
    r = pts.norm(dim=-1)
    shell = 600.0 * torch.exp(-((r - 1.0) / 0.06)**2)
    blob = 1000.0 * torch.sigmoid((0.35 - (pts - torch.tensor([0.3, -0.2, 0.4], device=pts.device)).norm(dim=-1)) / 0.02)
    sigma = shell + blob - 80.0 * torch.sigmoid((r - 1.3) / 0.1) - 20.0
    base = torch.stack([torch.sin(3.1 * pts[:, 0] + 0.3), torch.cos(2.3 * pts[:, 1] - 0.5), torch.sin(1.7 * pts[:, 2] + pts[:, 0])], -1)
    spec = (dirs * torch.tensor([0.6, -0.3, 0.5], device=pts.device)).sum(-1, keepdim=True)
    return 2.5 * base + 1.5 * spec, sigma


def fit_teacher(seed, steps=1500, n=8192, device="cpu", lr=5e-4):
    """state dict (CPU tensors) of one NeRF(D=8, W=256, skips=[4], use_viewdirs) fitted to analytic_targets."""
    sd0 = O.make_teacher_state_dicts(seed, 1, alpha_bias=0.5)[0]
    sd = {k: v.clone().to(device).requires_grad_(True) for k, v in sd0.items()}
    opt = torch.optim.Adam(list(sd.values()), lr=lr)
    g = torch.Generator(device="cpu").manual_seed(seed)
    for it in range(steps):
        pts = ((torch.rand(n, 3, generator=g) * 2 - 1) * 1.6).to(device)
        dirs = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1).to(device)
        rgb_t, sig_t = analytic_targets(pts, dirs)
        emb = torch.cat([O.nerf_embed(pts, 10), O.nerf_embed(dirs, 4)], -1)
        out = O.nerf_forward(sd, emb)
        loss = ((out[:, :3] - rgb_t)**2).mean() + ((out[:, 3] - sig_t)**2).mean() * 1e-3
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    return {k: v.detach().cpu().contiguous() for k, v in sd.items()}


def teacher_stats(sd, n=4096, seed=0):
    """(max |hidden activation|, min sigma pre-activation, max sigma pre-activation) on random points of the scene box."""
    g = torch.Generator().manual_seed(seed)
    pts = (torch.rand(n, 3, generator=g) * 2 - 1) * 1.6
    dirs = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    emb = torch.cat([O.nerf_embed(pts, 10), O.nerf_embed(dirs, 4)], -1)
    h, hmax = emb[:, :63], 0.
    for i in range(8):
        h = torch.relu(torch.nn.functional.linear(h, sd["pts_linears.%d.weight" % i], sd["pts_linears.%d.bias" % i]))
        hmax = max(hmax, h.abs().max().item())
        if i == 4:
            h = torch.cat([emb[:, :63], h], -1)
    out = O.nerf_forward(sd, emb)
    return hmax, out[:, 3].min().item(), out[:, 3].max().item()


# ---- the trained-like pair and rays through its scene (shared by the teacher render and teacher training tests) -----------
_TRAINED = {}


def trained_like_pair():
    """(coarse, fine) state dicts fitted on the GPU to analytic_targets; fitted once per process."""
    if not _TRAINED:
        for name, seed in (("coarse", 21), ("fine", 22)):
            _TRAINED[name] = fit_teacher(seed, steps=800, n=4096, device="cuda")
        for name, sd in _TRAINED.items():
            hmax, smin, smax = teacher_stats(sd)
            print("trained-like %s: max |hidden| %.0f, sigma pre-activation %.0f .. %.0f" % (name, hmax, smin, smax))
            assert hmax > 50 and smax > 200 and smin < -20  # the fit really left the init distribution
    return _TRAINED["coarse"], _TRAINED["fine"]


def scene_rays(R, seed, H=181, W=181, focal=250.):
    """R rays of one camera on the r = 4 sphere looking at the analytic scene, as render() packs them (create_data.py:97-176)."""
    from r2l_amd.render import get_rays
    c2w = torch.from_numpy(O.pose_spherical(35., -25., 4.)[:3, :4])
    ro, rd = get_rays(H, W, focal, c2w)
    ro, rd = ro.reshape(-1, 3)[:R], rd.reshape(-1, 3)[:R]
    vd = rd / rd.norm(dim=-1, keepdim=True)
    return torch.cat([ro, rd, 2. * torch.ones_like(rd[:, :1]), 6. * torch.ones_like(rd[:, :1]), vd], -1).float()


# ---- fp64 yardstick of the teacher's network backward (r2l_teacher_backward) ----------------------------------------------
STASH_SLOT = 256  # floats per point of one stash slot (r2l_teacher_net.h: slots 0-7 relu(h0..h7), 8 the feature, 9 relu(views))


def stash_slots(stash, P):
    """The 10 stash slots of P points as views: [P,256] x 9, then [P,128]."""
    return [stash[l * P * STASH_SLOT:l * P * STASH_SLOT + P * (128 if l == 9 else 256)].view(P, 128 if l == 9 else 256)
            for l in range(10)]


def layer_outputs(sd, emb):
    """The stashed quantities restated from a state dict and the [n, 63 + 27] embedding: relu(h0..h7), feature, relu(views)."""
    pts, views = emb[:, :63], emb[:, 63:]
    h, outs = pts, []
    for i in range(8):
        h = torch.relu(h @ sd["pts_linears.%d.weight" % i].T + sd["pts_linears.%d.bias" % i])
        outs.append(h)
        if i == 4:
            h = torch.cat([pts, h], -1)
    feat = h @ sd["feature_linear.weight"].T + sd["feature_linear.bias"]
    v = torch.relu(torch.cat([feat, views], -1) @ sd["views_linears.0.weight"].T + sd["views_linears.0.bias"])
    return outs + [feat, v]


def teacher_backward_from_stash(sd, rays_o, rays_d, viewdirs, z, stash, draw, device="cpu"):
    """fp64 restatement of the teacher's backprop (model/nerf_raybased.py:357-401) from the device's stash.

    sd: the network's state dict; rays_o / rays_d / viewdirs [R,3], z [R,S] and stash (r2l_teacher_stash_floats(R*S) floats) as
    the device saw them (fp32); draw [R,S,4] = dL/draw.  The ReLU masks (stash > 0) and the activations are the device's, promoted
    to fp64; the encodings are recomputed in fp64 from the fp32 points o + d*z (mul and add rounded separately, as the kernels).
    So the only thing left between this and r2l_teacher_backward is the kernel's fp32 rounding.

    Returns (grads, mags): two dicts in state_dict order.  mags is the same backprop run on |draw| and |W| (M_l, the absolute
    pre-activation gradient of layer l): |dW_l| = M_l^T |A_l|, |db_l| = sum_p M_l.  It bounds what rounding can do to each entry,
    including entries whose G cancels (their error is set by the layers above, not by their own size)."""
    f64 = dict(dtype=torch.float64, device=device)
    R, S = z.shape
    P = R * S
    o, d, vd, zz = [t.to(device=device, dtype=torch.float32) for t in (rays_o, rays_d, viewdirs, z)]
    pts = (o[:, None, :] + d[:, None, :] * zz[:, :, None]).reshape(P, 3)  # fp32, mul then add: the kernels' points
    pe_x = O.nerf_embed(pts.to(**f64), 10)
    pe_d = O.nerf_embed(vd.to(**f64)[:, None, :].expand(R, S, 3).reshape(P, 3), 4)
    slots = stash_slots(stash.to(device), P)
    act = lambda l: slots[l].to(**f64)
    W = {k: v.to(**f64) for k, v in sd.items()}
    dr = draw.reshape(P, 4).to(**f64)

    def run(dr, W, absval):
        a = (lambda t: t.abs()) if absval else (lambda t: t)
        g = {}

        def wgrad(name, G, X):
            g[name + ".weight"] = G.T @ a(X)
            g[name + ".bias"] = G.sum(0)
        drgb, dsig = dr[:, :3], dr[:, 3:4]
        v = act(9)
        wgrad("rgb_linear", drgb, v)
        wgrad("alpha_linear", dsig, act(7))
        G = (drgb @ W["rgb_linear.weight"]) * (v > 0)  # views layer, [P,128]
        wgrad("views_linears.0", G, torch.cat([act(8), pe_d], -1))
        G = G @ W["views_linears.0.weight"][:, :256]  # feature (no ReLU)
        wgrad("feature_linear", G, act(7))
        h = act(7)
        G = (G @ W["feature_linear.weight"] + dsig * W["alpha_linear.weight"]) * (h > 0)  # layer 7
        for l in range(7, 0, -1):
            nx = 63 if l == 5 else 0
            x = act(l - 1)
            wgrad("pts_linears.%d" % l, G, torch.cat([pe_x, x], -1) if nx else x)
            G = (G @ W["pts_linears.%d.weight" % l][:, nx:]) * (x > 0)
        wgrad("pts_linears.0", G, pe_x)
        return {k: g[k] for k in sd}

    grads = run(dr, W, False)
    mags = run(dr.abs(), {k: v.abs() for k, v in W.items()}, True)
    return grads, mags
