"""Test infrastructure: a NeRF teacher whose weights have LEFT the init distribution.

No trained lego checkpoint can be downloaded here, so the teacher is fitted for a couple of thousand Adam steps (plain torch
autograd on the oracle's functional forward, on whatever device the caller picks) to an analytic scene with the statistics a
trained NeRF shows: sigma pre-activations from about -10^2 in empty space to 10^2 .. 10^3 inside surfaces, a sharp shell and
an opaque blob, view-dependent colour.  The kernels under test never see this code; they get the resulting state dict."""
import torch

from oracle import r2l_oracle as O
from tests.student_util import EMB_EXACT, linear32, pieces, rms


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


# ---- fp64 yardstick of the teacher's INFERENCE forward (r2l_teacher_mlp_cfg; tests/test_teacher_forward_{cpu,gpu}.py) ------
# Per point, every entry of raw.  unit[p,c] = |W_head| |x_p| + |b_head|, x = relu(views) for the three colour logits and relu(h7)
# for sigma: the size of the sum that rounding acts on in a head.  Bars, in that unit:
#   exact families (fp32 MFMA, bf16x3):  |got - raw64| <= C_T unit + EMB_EXACT jac1 + floor  per entry; per case of >= 1000 points
#       rms((got - raw64) / unit) <= 4 rms(e_ref / unit) + EMB_EXACT rms(jac2 / unit);
#   fp16x2: the same plus 3 e_model per entry and 3 rms(e_model / unit) per case (the student's rule); the scaled stream's
#       per-entry bar also takes 3 x the width of the operand model's family (forward_spread: a stated term from the fp64 model).
# e_ref: the pinned fp32 reference (forward32: every product by student_util.linear32); e_model: the fp16x2 operand model
# (forward16x2).  jac1 / jac2: the l1 / l2 norm of d raw[p,c] / d (the 90 encoding values of point p); EMB_EXACT = 1.5 ulp of a
# value <= 1, r2l_sincos's measured bar for |argument| <= 4096 — which is why every case keeps |coordinate| <= 8 (top xyz
# frequency 2^9), asserted by check_input_condition.  All three families encode with r2l_sincos at the frequency itself.
#
# C_T = 4 x the worst |e_ref| / unit over T_CASES on init-distribution and trained-like weights and over the scaled case,
# measured on the CPU by tests/test_teacher_forward_cpu.py (which holds the reference within C_T / 4 in every case and the worst
# of the table between C_T / 8 and C_T / 4):
#   weights                           worst |e_ref| / unit (case)    rms at (4099, 4)
#   init                              8.99e-7  (5, 192)              1.22e-7
#   trained-like, fitted on the CPU   1.053e-6 (4099, 4)             8.5e-8
#   trained-like, fitted on the GPU   9.40e-7  (4099, 4)             8.9e-8     (printed by the GPU module, not asserted)
#   scaled (|h0| up to 2.5e5)         5.18e-7  (4099, 4)             7.9e-8
# 4 x 1.053e-6 = 4.21e-6, written 4.3e-6.  The pinned reference rounds its accumulator after every second product, in the order
# of k.  torch's sgemm sums in blocks: its fp32 forward lies at 0.036 of the per-entry bar on init weights and at 0.20 on
# trained-like ones, where the pinned reference lies at 0.21 and 0.24 — a C_T taken from torch's sums would be a statement
# about one BLAS, and on init weights it would lie under the pinned fp32 forward itself.
C_T = 4.3e-6
T_FLOOR = 1e-30  # keeps underflow out, nothing else: the smallest unit of any case is ~1e-2
T_TILE, T_WORKGROUP = 32, 128  # points per wave / per workgroup of the three forwards
T_RMS_MIN_POINTS = 1000
T_CASES = [(1, 1), (1, 31), (1, 32), (1, 33), (1, 127), (1, 128), (3, 43), (43, 3), (5, 192), (37, 64), (4099, 4)]
T_SELF_CHECK_CASES = [(43, 3), (37, 64)]
T_INIT_SEED, T_SCALED_SEED = 11, 5
T_XYZ_TOP_COL = 62  # cos(2^9 z): the last column of the xyz encoding
T_DIR_LAST_COL = 26  # cos(2^3 vd_z): the last column of the direction encoding


def scaled_state_dict():
    """The weights of tests/test_teacher_gpu.py::test_teacher_range_control: layer 0 times 1e5, layer 1 times 1e-5."""
    sd = {k: v.clone() for k, v in O.make_teacher_state_dicts(T_SCALED_SEED, 1, alpha_bias=0.5)[0].items()}
    sd["pts_linears.0.weight"] *= 1.0e5
    sd["pts_linears.0.bias"] *= 1.0e5
    sd["pts_linears.1.weight"] *= 1.0e-5
    return sd


_TRAINED_CPU = {}


def forward_weights(kind, device="cuda"):
    """'init': O.make_teacher_state_dicts(11, 2, alpha_bias=0.5)[0]; 'scaled': scaled_state_dict(); 'trained': the trained-like
    coarse net — trained_like_pair()'s on the GPU, a shorter fit of the same kind on the CPU (once per process) without one."""
    if kind == "init":
        return O.make_teacher_state_dicts(T_INIT_SEED, 2, alpha_bias=0.5)[0]
    if kind == "scaled":
        return scaled_state_dict()
    if device != "cpu":
        return trained_like_pair()[0]
    if not _TRAINED_CPU:
        threads = torch.get_num_threads()
        torch.set_num_threads(4)  # (sgemm splits its sums by the thread count: pinned, the fit is the same net on any machine)
        try:
            _TRAINED_CPU["coarse"] = fit_teacher(21, steps=400, n=2048, device="cpu")  # (10 s; sigma reaches 1e3 as on the GPU)
        finally:
            torch.set_num_threads(threads)
        hmax, smin, smax = teacher_stats(_TRAINED_CPU["coarse"])
        assert hmax > 50 and smax > 200 and smin < -20, (hmax, smin, smax)
    return _TRAINED_CPU["coarse"]


def forward_inputs(R, S, kind, seed=0):
    """(o, d, viewdirs, z) of a case on the CPU, fp32, |coordinate of a point| <= 8.  init / scaled: origins 0.3 randn, UNIT
    directions, z in [2, 6) ascending; ray 1 starts where ray 0 does.  trained: rays of scene_rays' camera drawn over its whole
    frame (one origin, every ray its own direction), the same z."""
    g = torch.Generator().manual_seed(seed * 7919 + R * 31 + S)
    if kind == "trained":
        rb = scene_rays(181 * 181, 0)[torch.randperm(181 * 181, generator=g)[:R]]
        o, d, vd = rb[:, 0:3].contiguous(), rb[:, 3:6].contiguous(), rb[:, 8:11].contiguous()
    else:
        o = torch.randn(R, 3, generator=g) * 0.3
        d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
        vd = d / d.norm(dim=-1, keepdim=True)
        if R > 1:
            o[1] = o[0]
    z = torch.sort(torch.rand(R, S, generator=g) * 4 + 2, -1)[0]
    return o, d, vd, z


def points32(o, d, z, fma=False):
    """The kernels' points [R*S,3], fp32: o + d*z with the product and the sum rounded separately (create_data.py:484; the library
    is built with -ffp-contract=off).  fma: mutant (a), one rounding (the exact product and the sum formed in fp64)."""
    o, d, z = [t.to(torch.float32) for t in (o, d, z)]
    if fma:
        return (o.double()[:, None, :] + d.double()[:, None, :] * z.double()[:, :, None]).float().reshape(-1, 3)
    prod = d[:, None, :] * z[:, :, None]
    return (o[:, None, :] + prod).reshape(-1, 3)


def check_input_condition(pts32, vd):
    """r2l_sincos's 1.5 ulp holds for |argument| <= 4096: top frequencies 2^9 (xyz) and 2^3 (direction)."""
    assert pts32.abs().max().item() * 512 <= 4096, pts32.abs().max().item()
    assert vd.abs().max().item() * 8 <= 4096


def encoding64(pts32, vd, S, device="cpu"):
    """[P,90] fp64: the true sin / cos (O.nerf_embed in float64) of the fp32 points and of each point's ray's fp32 direction."""
    P = pts32.shape[0]
    with torch.device(device):  # (the oracle creates its frequency table on the default device)
        pe_x = O.nerf_embed(pts32.to(device).double(), 10)
        pe_d = O.nerf_embed(vd.to(device).double()[:, None, :].expand(P // S, S, 3).reshape(P, 3), 4)
    return torch.cat([pe_x, pe_d], -1)


def net_forward(emb, lin, head):
    """O.nerf_forward's operation sequence with every hidden product by lin(x, name) and the two heads by head(x, name).
    Returns (raw [P,4] = rgb ++ sigma, relu(h7), relu(views))."""
    pts, views = emb[:, :63], emb[:, 63:]
    h = pts
    for i in range(8):
        h = torch.relu(lin(h, "pts_linears.%d" % i))
        if i == 4:
            h = torch.cat([pts, h], -1)
    alpha = head(h, "alpha_linear")
    feat = lin(h, "feature_linear")
    v = torch.relu(lin(torch.cat([feat, views], -1), "views_linears.0"))
    return torch.cat([head(v, "rgb_linear"), alpha], -1), h, v


def forward64(sd64, emb64):
    """(raw64, unit), each [P,4]."""
    lin = lambda x, name: x @ sd64[name + ".weight"].T + sd64[name + ".bias"]
    raw, h7, v = net_forward(emb64, lin, lin)
    mag = lambda x, name: x @ sd64[name + ".weight"].abs().T + sd64[name + ".bias"].abs()
    return raw, torch.cat([mag(v, "rgb_linear"), mag(h7, "alpha_linear")], -1)


def forward32(sd64, emb32):
    """THE fp32 reference: the same net on the fp32-rounded encoding, every product by student_util.linear32 (pinned summation
    order: the same number on any machine), ReLU and concatenation exact.  (linear32 takes products two at a time: an odd K — 63,
    319, 283 — gets one zero column, which adds an exact zero.)"""
    def lin(x, name):
        w, b = sd64[name + ".weight"], sd64[name + ".bias"]
        if x.shape[1] % 2:
            x = torch.nn.functional.pad(x, (0, 1))
            w = torch.nn.functional.pad(w, (0, 1))
        return linear32(x.contiguous(), w, b)
    return net_forward(emb32.float(), lin, lin)[0]


def forward16x2(sd64, emb64, s=1.0, drop_mid=None, undivided_bias=None, jitter=0.0):
    """The operand model of r2l_teacher2.hip (machinery r2l_f2.h), fp64: both operands of every product of the eight body layers,
    feature_linear and the views layer written hi + mid in fp16, the product taken as the three terms the kernel keeps (W_hi x_hi +
    W_mid x_hi + W_hi x_mid), the sum exact, a bias as its two pieces (its stage multiplies them by ones).  The two heads are left
    exact: the kernel forms them as fp32 fmaf chains on the VALU from the fp32 accumulators and the fp32 weights (alpha inside the
    feature layer's gathers, rgb behind the views layer).
    s: the activation scale, a power of two, where t2_pack_elements and the kernel apply it: layer 0 runs on its weights and bias
    as they are and its OUTPUT is multiplied by 1 / s; every other bias and the embedding column blocks of layer 5 and of the
    views layer are divided by s before their split; the heads' dot products are multiplied by s, their biases added unscaled.
    drop_mid = layer name: mutant (b), the W_hi x_mid term lost in that layer.  undivided_bias = layer name: mutant (f).
    jitter = e: a SECOND REALIZATION of the same model — every activation operand times (1 +- e), seeded signs, before its split.
    The kernel splits fp32 accumulators, which differ from this function's fp64 values by about an ulp; on which side of a
    rounding boundary a piece falls follows such differences, so the model is a family and forward_spread measures its width."""
    f16 = torch.float16
    gen = torch.Generator(device=emb64.device).manual_seed(0)

    def lin(x, name, emb_cols=None, bias_div=None):
        w = sd64[name + ".weight"]
        if emb_cols is not None and s != 1.0:
            w = w.clone()
            w[:, emb_cols] = w[:, emb_cols] / s
        b = sd64[name + ".bias"] / ((s if bias_div is None else bias_div) if name != undivided_bias else 1.0)
        if jitter:
            x = x * (1.0 + jitter * (torch.randint(0, 2, x.shape, generator=gen, device=x.device).double() * 2 - 1))
        (xh, xm), (wh, wm) = pieces(x, f16, 2), pieces(w, f16, 2)
        out = xh @ (wh + wm).T + sum(pieces(b, f16, 2))
        return out if name == drop_mid else out + xm @ wh.T

    pts, views = emb64[:, :63], emb64[:, 63:]
    h = torch.relu(lin(pts, "pts_linears.0", bias_div=1.0) / s)
    for i in range(1, 8):
        h = torch.relu(lin(h, "pts_linears.%d" % i, emb_cols=slice(0, 63) if i == 5 else None))
        if i == 4:
            h = torch.cat([pts, h], -1)
    head = lambda x, name: (x @ sd64[name + ".weight"].T) * s + sd64[name + ".bias"]
    alpha = head(h, "alpha_linear")
    feat = lin(h, "feature_linear")
    v = torch.relu(lin(torch.cat([feat, views], -1), "views_linears.0", emb_cols=slice(256, 283)))
    return torch.cat([head(v, "rgb_linear"), alpha], -1)


T_JITTER = 2.0 ** -23  # one ulp of fp32, relative


def forward_spread(sd64, emb64, unit, s):
    """The width of the operand model's family at scale s: the worst |forward16x2(jitter = one fp32 ulp) - forward16x2| / unit over
    the points (a scalar tensor).  At s > 1 the operands x / s have their mid pieces in fp16's SUBNORMAL range, where a piece is
    carried to 2^-25 absolute — s 2^-25 in the net's own units — whichever side it rounds to: the width grows with s (the scaled
    net: 6e-7 unit at s = 8, 2e-6 at 32, 1.5e-5 at 256), while the part of e_model that the kernel SHARES with the model (the
    fp16 pieces of the weights, the same bits on both sides: 1.6e-5 unit rms on the scaled net, whose layer 1 holds 6e-7) does
    not tell the two apart.  r2l_f2.h documents the property ("parts below 2^-14 lose bits but are then below 2^-25
    absolutely"); it enters the per-entry fp16x2 bar of the SCALED stream as 3 x this width x unit, the factor the operand
    model's own distance gets.  At s = 1 the bars hold without it and it is left out."""
    return ((forward16x2(sd64, emb64, s=s, jitter=T_JITTER) - forward16x2(sd64, emb64, s=s)).abs() / unit).max()


def jacobian_rows(sd64, emb64):
    """[d raw[:, c] / d emb for c = 0 .. 3], each [P,90]: four fp64 autograd passes, each on the sum over the points of one output
    (points do not interact: row p of the gradient is point p's Jacobian row)."""
    e = emb64.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        raw = forward64(sd64, e)[0]
        return [torch.autograd.grad(raw[:, c].sum(), e, retain_graph=(c < 3))[0] for c in range(4)]


def forward_yardstick(sd, emb64, model_scale=None, chunk=4096, spread=False):
    """Everything the bars need of one case.  sd: the fp32 state dict; emb64 [P,90] on the device the fp64 work is to run on.
    Returns fp64 tensors [P,4] on that device: raw (fp64 forward), unit, jac1, jac2, e_ref = |forward32 - raw| (never a kernel's),
    and, with model_scale = s, e_model = |forward16x2 at scale s - raw|; with spread, 'spread' = forward_spread at that scale (a
    scalar)."""
    dev = emb64.device
    sd64 = {k: v.detach().to(device=dev, dtype=torch.float64) for k, v in sd.items()}
    keys = ["raw", "unit", "jac1", "jac2", "e_ref"] + (["e_model"] if model_scale is not None else [])
    out = {k: [] for k in keys}
    for lo in range(0, emb64.shape[0], chunk):
        e = emb64[lo:lo + chunk]
        raw, unit = forward64(sd64, e)
        rows = jacobian_rows(sd64, e)
        out["raw"].append(raw)
        out["unit"].append(unit)
        out["jac1"].append(torch.stack([r.abs().sum(1) for r in rows], 1))
        out["jac2"].append(torch.stack([r.norm(dim=1) for r in rows], 1))
        out["e_ref"].append((forward32(sd64, e.float()).double() - raw).abs())
        if model_scale is not None:
            out["e_model"].append((forward16x2(sd64, e, s=model_scale) - raw).abs())
    Y = {k: torch.cat(v) for k, v in out.items()}
    if spread:
        Y["spread"] = forward_spread(sd64, emb64, Y["unit"], model_scale)
    return Y


def forward_bars(Y, fp16x2=False):
    """(per-entry bar [P,4], per-case rms bar in units) of a family group."""
    entry = C_T * Y["unit"] + EMB_EXACT * Y["jac1"] + T_FLOOR
    case = 4.0 * rms(Y["e_ref"] / Y["unit"]) + EMB_EXACT * rms(Y["jac2"] / Y["unit"])
    if fp16x2:
        entry = entry + 3.0 * Y["e_model"] + (3.0 * Y["spread"] * Y["unit"] if "spread" in Y else 0.)
        case = case + 3.0 * rms(Y["e_model"] / Y["unit"])
    return entry, case


def forward_check(got, Y, fp16x2=False):
    """got [P,4] against the yardstick Y: dict(bad: bool [P], points with an entry not within its bar (a NaN is not); ratio [P]:
    largest |got - raw64| / bar of each point (inf for a NaN); worst; rms, rms_bar: the per-case statistic and its bar, in units)."""
    entry, case = forward_bars(Y, fp16x2)
    err = (got.double().to(Y["raw"].device).reshape(-1, 4) - Y["raw"]).abs()
    ratio = torch.nan_to_num(err / entry, nan=float("inf")).max(dim=1).values
    return dict(bad=~(ratio <= 1.0), ratio=ratio, worst=ratio.max().item(), rms=rms(err / Y["unit"]), rms_bar=case)


def tile_first_ray_directions(vd, R, S):
    """Mutant (d): [P,3], every point of a 32-point tile given the view direction of the ray of the tile's FIRST point."""
    p = torch.arange(R * S)
    return vd[(p // T_TILE * T_TILE) // S]


def zero_column(sd, name, col):
    """Mutant (c): sd with column col of one weight matrix zeroed."""
    out = dict(sd)
    out[name] = sd[name].clone()
    out[name][:, col] = 0.
    return out
