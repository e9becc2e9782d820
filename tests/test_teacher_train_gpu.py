"""Teacher training on the GPU (r2l_amd/teacher_train.py, csrc/r2l_teacher_train.hip): forward with stash, raw2outputs
backward, full-step gradients against fp64 autograd of the oracle, Adam against torch.optim.Adam, determinism, and the
utils/train_nerf.py command line end to end."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import r2l_oracle as O
from tests.teacher_util import layer_outputs, scene_rays, stash_slots, trained_like_pair

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_teacher(sd, device="cuda"):
    from model.nerf_raybased import NeRF
    m = NeRF(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
    m.load_state_dict(sd)
    return m.to(device)


def rays(R, seed):
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(R, 3, generator=g) * 0.5
    d = torch.randn(R, 3, generator=g)
    vd = d / d.norm(dim=-1, keepdim=True)
    tgt = torch.rand(R, 3, generator=g)
    return o, d, vd, tgt


def test_forward_with_stash():
    from r2l_amd import _lib
    from r2l_amd.engine import _ptr, _stream
    from r2l_amd.render import teacher_engine
    lib = _lib.load()
    sd, _ = O.make_teacher_state_dicts(11, 2, alpha_bias=0.5)
    eng = teacher_engine(make_teacher(sd))
    eng.set_config(precision="fp32_mfma")
    R, S = 37, 61  # P = 2257: not a multiple of 32
    o, d, vd, _ = rays(R, 0)
    z = torch.sort(torch.rand(R, S, generator=torch.Generator().manual_seed(1)) * 4 + 2, -1)[0]
    og, dg, vdg, zg = o.cuda(), d.cuda(), vd.cuda(), z.cuda()  # (kept alive: the C ABI takes raw pointers)
    ref_raw = eng.mlp(og, dg, vdg, zg)
    P = R * S
    stash = torch.full((lib.r2l_teacher_stash_floats(P),), float("nan"), device="cuda")
    raw = torch.empty(R, S, 4, device="cuda")
    _lib.check(lib.r2l_teacher_mlp_train(_ptr(og), _ptr(dg), _ptr(vdg), _ptr(zg), _ptr(eng.wstream), _ptr(eng.flat), _ptr(raw),
                                         _ptr(stash), R, S, _stream()), "mlp_train")
    assert torch.equal(raw, ref_raw), (raw - ref_raw).abs().max().item()
    pts = (o[:, None, :] + d[:, None, :] * z[:, :, None]).reshape(-1, 3)
    emb = torch.cat([O.nerf_embed(pts, 10), O.nerf_embed(vd[:, None].expand(R, S, 3).reshape(-1, 3), 4)], -1)
    want = layer_outputs(sd, emb)
    st = stash.cpu()
    for l in range(10):
        w = 128 if l == 9 else 256
        got = st[l * P * 256:l * P * 256 + P * w].view(P, w)
        err = (got - want[l]).abs().max().item()
        assert err < 2e-5, (l, err)


def oracle_draw(raw, z, rays_d, noise, white, target):
    raw = raw.double().requires_grad_(True)
    rgb = O.raw2outputs(raw, z.double(), rays_d.double(), None if noise is None else noise.double(), white)[0]
    torch.mean((rgb - target.double())**2).backward()
    return raw.grad, torch.mean((rgb - target.double())**2).item()


def nrel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300)).item()


@pytest.mark.parametrize("S", [64, 192, 37, 256])
@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("with_noise", [False, True])
def test_raw2outputs_backward(S, white, with_noise):
    from r2l_amd import _lib
    from r2l_amd.engine import _ptr, _stream
    lib = _lib.load()
    R = 45
    g = torch.Generator().manual_seed(S)
    raw = torch.randn(R, S, 4, generator=g) * 2
    raw[0, 0, 3] = 1e4  # opaque first sample
    raw[1, -1, 3] = 1e4  # alpha = 1 at the last sample (and everywhere the 1e10 dists meet sigma > 0)
    raw[2, :, 3] = -1.0  # sigma < 0 for a whole ray
    z = torch.sort(torch.rand(R, S, generator=g) * 4 + 2, -1)[0]
    d = torch.randn(R, 3, generator=g)
    tgt = torch.rand(R, 3, generator=g)
    noise = torch.randn(R, S, generator=g) * 0.5 if with_noise else None
    draw = torch.empty(R, S, 4, device="cuda")
    sq = torch.empty(R, device="cuda")
    dev = [None if t is None else t.cuda() for t in (raw, z, d, noise, tgt)]  # (kept alive: the C ABI takes raw pointers)
    _lib.check(lib.r2l_raw2outputs_backward(_ptr(dev[0]), _ptr(dev[1]), _ptr(dev[2]), _ptr(dev[3]), int(white), _ptr(dev[4]),
                                            _ptr(draw), _ptr(sq), R, S, _stream()), "r2l_raw2outputs_backward")
    want, mse = oracle_draw(raw, z, d, noise, white, tgt)
    assert nrel(draw.cpu(), want) <= 1e-5, nrel(draw.cpu(), want)
    assert abs(sq.sum().item() / (3 * R) - mse) <= 1e-6 * max(1., mse)


# ---- full step -----------------------------------------------------------------------------------------------------
def draws(R, NS=64, NI=128, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.rand(R, NS, generator=g), torch.rand(R, NI, generator=g)


def oracle_step_grads(csd, fsd, o, d, vd, tgt, t_rand, u, dtype=torch.float64, NS=64, NI=128, white=True, z_dev=None,
                      noise=None, z_tol=1e-4, info=None):
    """Autograd of img2mse(rgb) + img2mse(rgb0) built from oracle pieces, z_samples detached (main.py:728).
    z_dev: the (coarse, fine) sample depths the device used.  The oracle's own agree with them to an ulp or so, but the
    encoding's 2^9 frequency turns one ulp of z into ~1e-4 of phase, which the layer-0 weight gradient shows; the yardstick
    restates the step at the device's depths instead (checked against the oracle's below, the fine ones to z_tol; None: not
    checked).  noise: the (coarse [R,NS], fine [R,NS+NI]) draws the device added to sigma (raw_noise_std > 0).  info: a dict
    that receives the largest distance of the oracle's fine depths from the device's ("z_fine")."""
    sds = [{k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()} for sd in (csd, fsd)]
    R = o.shape[0]
    t = torch.linspace(0., 1., steps=NS)
    z = (2. * (1. - t) + 6. * t).expand(R, NS)
    lower, upper = O.stratified_bounds(z)
    z = lower + (upper - lower) * t_rand
    if z_dev is not None:
        assert (z - z_dev[0]).abs().max().item() <= 1e-5
        z = z_dev[0]
    def net(sd, zz):
        pts = o[:, None, :] + d[:, None, :] * zz[:, :, None]
        return O.run_network(sd, pts.to(dtype), vd.to(dtype))
    nc, nf = (None, None) if noise is None else noise
    raw0 = net(sds[0], z)
    rgb0, _, _, w0, _ = O.raw2outputs(raw0, z.to(dtype), d.to(dtype), None if nc is None else nc.to(dtype), white)
    with torch.no_grad():  # the samples are placed by the fp32 weights, as on the device
        w32 = O.raw2outputs(raw0.float(), z, d, None if nc is None else nc.float(), white)[3]
        zs = O.sample_pdf(.5 * (z[..., 1:] + z[..., :-1]), w32[..., 1:-1], NI, u=u)
        z_all = torch.sort(torch.cat([z, zs], -1), -1)[0]
        if z_dev is not None:
            dz = (z_all - z_dev[1]).abs().max().item()
            if info is not None:
                info["z_fine"] = dz
            assert z_tol is None or dz <= z_tol, dz
            z_all = z_dev[1]
    raw = net(sds[1], z_all)
    rgb = O.raw2outputs(raw, z_all.to(dtype), d.to(dtype), None if nf is None else nf.to(dtype), white)[0]
    loss = torch.mean((rgb - tgt.to(dtype))**2) + torch.mean((rgb0 - tgt.to(dtype))**2)
    loss.backward()
    return [{k: v.grad for k, v in sd.items()} for sd in sds], loss.item()


# (id, case): R rays, NS + NI samples, background, raw_noise_std, weights.  The ids "64" and "1024" are the original cases.
# R = 37 gives P = 2368 coarse / 7104 fine points (partial chunks, tiles and k-steps), R = 1 a single ray; 64 + 192 = 256 samples
# is the most the raw2outputs backward takes.
FULL_STEP_CASES = [
    ("64", dict(R=64, original=True)), ("1024", dict(R=1024, original=True)), ("37", dict(R=37)), ("1", dict(R=1)),
    ("64-black", dict(R=64, white=False)), ("64-noise", dict(R=64, noise_std=1.)),
    ("64-32+96", dict(R=64, NS=32, NI=96)), ("64-64+192", dict(R=64, NS=64, NI=192)),
    ("64-trained", dict(R=64, trained=True)),
]
C_BWD = 3e-6  # per-entry bar of the network backward against its stash yardstick (tests/test_teacher_backward_gpu.py)
C_R2O = 2e-5  # per-entry bar of the raw2outputs backward, relative to the ray's largest |draw| (same module)


def scene_batch(R, seed):
    """R rays through the dense middle of the trained-like scene (pixels of the central 61 x 61 of the 181 x 181 camera)."""
    rb = scene_rays(181 * 181, 0).view(181, 181, -1)[60:121, 60:121].reshape(-1, 11)
    rb = rb[torch.randperm(rb.shape[0], generator=torch.Generator().manual_seed(seed))[:R]]
    tgt = torch.rand(R, 3, generator=torch.Generator().manual_seed(seed + 1))
    return rb[:, 0:3].contiguous(), rb[:, 3:6].contiguous(), rb[:, 8:11].contiguous(), tgt


def draw_fp64(raw, z, d, noise, white, tgt):
    """fp64 autograd of img2mse(raw2outputs(raw)) with respect to raw (one net's term of the step's loss)."""
    raw = raw.detach().cpu().double().requires_grad_(True)
    rgb = O.raw2outputs(raw, z.cpu().double(), d.double(), None if noise is None else noise.double(), white)[0]
    torch.mean((rgb - tgt.double())**2).backward()
    return raw.grad


@pytest.mark.parametrize("case", [c for _, c in FULL_STEP_CASES], ids=[i for i, _ in FULL_STEP_CASES])
def test_full_step_gradients_vs_fp64(case, monkeypatch):
    """The whole step (forward with stash, sample_pdf, raw2outputs backward, network backward of both nets) against two fp64
    yardsticks.
    (a) The stash yardstick, at each net's own raw and stash as the step made them: with the step's own draw, every entry within
    3e-6 of its magnitude (the per-layer bar); with draw from fp64 autograd of raw2outputs + img2mse, every tensor within 1e-5
    norm-relative, except the alpha head: its weight and bias are sums of dL/dsigma, which cancel within each ray, so they are held
    to what the raw2outputs backward's own bar allows, 2e-5 of each ray's largest |draw| per point.  Measured on one MI355X:
    no entry past the first bar; 6.4e-6 on the second (alpha head: up to 1.5e-3 norm-relative, inside its bound).
    (b) A fresh fp64 forward (oracle_step_grads): the original cases at 5e-4 norm-relative, as before.  The added cases at 5e-4
    plus the share of what comes before the network backward, the distance of (a) with the step's own draw from (b): the fp32
    forward flips ReLU masks of activations within rounding of zero (measured up to 8.6e-4 on layer 0 at 32 + 96 samples, where
    one coarse mask flips; the count is printed) and the raw2outputs backward's rounding of the cancelling dL/dsigma (up to 1.5e-3
    on the alpha head, black background); (a) shows that the network backward adds nothing to them."""
    from r2l_amd.teacher_train import TeacherTrainer
    from tests.teacher_util import teacher_backward_from_stash
    R, NS, NI = case["R"], case.get("NS", 64), case.get("NI", 128)
    white, std, trained = case.get("white", True), case.get("noise_std", 0.), case.get("trained", False)
    csd, fsd = trained_like_pair() if trained else O.make_teacher_state_dicts(5, 2, alpha_bias=0.5)
    noise = None
    if std > 0:  # the step's noise fixed by the test and handed to the yardstick
        g = torch.Generator().manual_seed(77)
        noise = (torch.randn(R, NS, generator=g) * std, torch.randn(R, NS + NI, generator=g) * std)
        fixed = {NS: noise[0].cuda(), NS + NI: noise[1].cuda()}
        monkeypatch.setattr(TeacherTrainer, "_noise", lambda self, R_, S_: fixed[S_])
    tr = TeacherTrainer(make_teacher(csd), make_teacher(fsd), N_samples=NS, N_importance=NI, perturb=1., white_bkgd=white,
                        raw_noise_std=std)
    seen = {}
    backward = tr._backward

    def keep(i, rays_o, rays_d, viewdirs, z, raw, stash, nz, target):  # each net's raw, stash and draw as the step used them
        out = backward(i, rays_o, rays_d, viewdirs, z, raw, stash, nz, target)
        seen[i] = (raw, stash, tr._bufs["draw"][:z.numel() * 4].clone().view(*z.shape, 4))
        return out
    tr._backward = keep
    o, d, vd, tgt = scene_batch(R, 5) if trained else rays(R, 3)
    t_rand, u = draws(R, NS, NI)
    og, dg, vdg = o.cuda(), d.cuda(), vd.cuda()
    out = tr.forward_backward(og, dg, vdg, 2., 6., tgt.cuda(), t_rand=t_rand.cuda(), u=u.cuda())
    z_dev = [z.cpu() for z in tr.last_z]
    info = {}
    # fine depths: 1e-4, as before; where the pdf is flat at 1e-5 an fp32 difference of the weights moves a fine sample far
    # (measured 3.2e-3 with noise, 3.9e-2 on the trained-like pair)
    z_tol = 0.16 if trained else (1.3e-2 if std > 0 else 1e-4)
    kw = dict(NS=NS, NI=NI, white=white, z_dev=z_dev, noise=noise, z_tol=z_tol, info=info)
    want, loss = oracle_step_grads(csd, fsd, o, d, vd, tgt, t_rand, u, **kw)
    assert abs(out[0].item() - loss) < 1e-5 * max(loss, 1.)
    if trained:
        with torch.no_grad():
            sig = max(O.run_network(sd, o[:, None, :] + d[:, None, :] * z[:, :, None], vd)[..., 3].max().item()
                      for sd, z in zip((csd, fsd), z_dev))
        assert sig > 200, sig  # the rays do cross the dense parts
    ref32, _ = oracle_step_grads(csd, fsd, o, d, vd, tgt, t_rand, u, dtype=torch.float32, **kw)
    g = tr.grads.cpu()
    off, rows, fails, flips = 0, [], [], []
    for i, sd in enumerate((csd, fsd)):
        raw, stash, draw_dev = seen[i]
        zi = tr.last_z[i]
        d64 = draw_fp64(raw, zi, d, None if noise is None else noise[i], white, tgt)
        with torch.no_grad():  # ReLU masks of the device's forward that differ from an fp64 forward's
            P = zi.numel()
            pts = (og[:, None, :] + dg[:, None, :] * zi[:, :, None]).reshape(P, 3).double()
            emb = torch.cat([O.nerf_embed(pts, 10), O.nerf_embed(vdg.double()[:, None].expand(*zi.shape, 3).reshape(P, 3), 4)], -1)
            acts = layer_outputs({k: v.double().cuda() for k, v in sd.items()}, emb)
            flips.append(sum(int(((st > 0) != (a > 0)).sum()) for l, (st, a) in enumerate(zip(stash_slots(stash, P), acts))
                             if l != 8))
        ys, _ = teacher_backward_from_stash(sd, og, dg, vdg, zi, stash, d64.cuda(), device="cuda")
        ys_dev, mags = teacher_backward_from_stash(sd, og, dg, vdg, zi, stash, draw_dev, device="cuda")
        raymax = d64.abs().amax(dim=(1, 2), keepdim=True).expand(d64.shape).contiguous()
        _, mr = teacher_backward_from_stash(sd, og, dg, vdg, zi, stash, raymax.cuda(), device="cuda")  # sum_p raymax |A|
        for k, w in want[i].items():
            got = g[off:off + w.numel()].view(w.shape)
            off += w.numel()
            e_ys = nrel(got, ys[k].cpu())
            viol = int(((got.double() - ys_dev[k].cpu()).abs() > C_BWD * mags[k].cpu() + 1e-12 * mags[k].max().item()).sum())
            fwd = nrel(ys_dev[k].cpu(), w)
            e, e32 = nrel(got, w), nrel(ref32[i][k], w)
            cos = torch.nn.functional.cosine_similarity(got.double().reshape(1, -1), w.reshape(1, -1)).item()
            rows.append((k, i, e_ys, viol, fwd, e, e32))
            if cos < 0.99999:
                fails.append(("cosine", i, k, cos))
            if viol:
                fails.append(("stash yardstick, own draw", i, k, viol))
            if k.startswith("alpha_linear"):
                over = (got.double() - ys[k].cpu()).abs() > C_BWD * mags[k].cpu() + C_R2O * mr[k].cpu()
                if over.any() and e_ys > 1e-5:
                    fails.append(("stash yardstick, alpha head", i, k, e_ys))
            elif e_ys > 1e-5:
                fails.append(("stash yardstick", i, k, e_ys))
            bar = 5e-4 if case.get("original") else 5e-4 + fwd
            if e > bar:
                fails.append(("fresh fp64", i, k, e, bar))
    print("full step %s: z_fine %.2g; flipped ReLU masks (coarse, fine) %s; worst: vs stash yardstick %.3g (alpha head %.3g), "
          "upstream share %.3g, vs fresh fp64 %.3g, torch fp32 %.3g"
          % (str(case), info.get("z_fine", 0), flips, max(r[2] for r in rows if not r[0].startswith("alpha")),
             max(r[2] for r in rows if r[0].startswith("alpha")), max(r[4] for r in rows), max(r[5] for r in rows),
             max(r[6] for r in rows)))
    for r in sorted(rows, key=lambda r: -r[5])[:4]:
        print("   %-22s net %d: vs stash %.3g (entries past the bar: %d), upstream share %.3g, vs fresh %.3g, torch fp32 %.3g" % r)
    assert not fails, fails


def test_more_than_256_samples_refused_before_any_work():
    """N_samples + N_importance > 256 (N_samples > 256 without a fine net) is refused when the trainer is built, not by the
    raw2outputs backward after two forward passes and sample_pdf."""
    from r2l_amd.teacher_train import TeacherTrainer
    csd, fsd = O.make_teacher_state_dicts(5, 2, alpha_bias=0.5)
    with pytest.raises(ValueError, match="at most 256 samples"):
        TeacherTrainer(make_teacher(csd), make_teacher(fsd), N_samples=64, N_importance=193)
    with pytest.raises(ValueError, match="at most 256 samples"):
        TeacherTrainer(make_teacher(csd), None, N_samples=257, N_importance=0)
    TeacherTrainer(make_teacher(csd), make_teacher(fsd), N_samples=64, N_importance=192)  # 256, the maximum: accepted


def test_three_adam_steps_vs_torch():
    from r2l_amd.teacher_train import TeacherTrainer
    csd, fsd = O.make_teacher_state_dicts(5, 2, alpha_bias=0.5)
    tr = TeacherTrainer(make_teacher(csd), make_teacher(fsd), perturb=1., white_bkgd=True)
    ref = [{k: v.clone().requires_grad_(True) for k, v in sd.items()} for sd in (csd, fsd)]
    opt = torch.optim.Adam([p for sd in ref for p in sd.values()], lr=5e-4, betas=(0.9, 0.999))
    R = 128
    for step in range(3):
        o, d, vd, tgt = rays(R, 10 + step)
        t_rand, u = draws(R, seed=step)
        tr.step(o.cuda(), d.cuda(), vd.cuda(), 2., 6., tgt.cuda(), 5e-4, t_rand=t_rand.cuda(), u=u.cuda())
        grads, _ = oracle_step_grads({k: v.detach() for k, v in ref[0].items()}, {k: v.detach() for k, v in ref[1].items()},
                                     o, d, vd, tgt, t_rand, u, dtype=torch.float32, z_dev=[z.cpu() for z in tr.last_z])
        for sd, gd in zip(ref, grads):
            for k in sd:
                sd[k].grad = gd[k]
        opt.step()
    flat_ref = torch.cat([p.detach().reshape(-1) for sd in ref for p in sd.values()])
    err = (tr.flat.cpu() - flat_ref).abs().max().item()
    # 1e-4 = 0.2 lr: Adam's first steps move every entry by ~lr * sign(grad) whatever its size, so an entry whose gradient is
    # near zero moves differently on two fp32 computations of the gradient (which differ by ~1e-3 norm-relative here, see
    # test_full_step_gradients_vs_fp64); measured 4.5e-5
    assert err <= 1e-4, err
    # the optimizer state loads into torch.optim.Adam
    sd = tr.optimizer_state_dict(5e-4)
    opt2 = torch.optim.Adam([p for s in ref for p in s.values()], lr=5e-4)
    opt2.load_state_dict(sd)
    assert float(sd["state"][0]["step"]) == 3


@pytest.mark.parametrize("R", [64, 37])
def test_step_is_deterministic(R):
    from r2l_amd.teacher_train import TeacherTrainer
    csd, fsd = O.make_teacher_state_dicts(5, 2, alpha_bias=0.5)
    tr = TeacherTrainer(make_teacher(csd), make_teacher(fsd), perturb=1., white_bkgd=True)
    o, d, vd, tgt = [t.cuda() for t in rays(R, 4)]
    t_rand, u = [t.cuda() for t in draws(R)]
    tr.forward_backward(o, d, vd, 2., 6., tgt, t_rand=t_rand, u=u)
    g1 = tr.grads.clone()
    tr.grads.fill_(float("nan"))
    tr.forward_backward(o, d, vd, 2., 6., tgt, t_rand=t_rand, u=u)
    assert torch.equal(g1.view(torch.int32), tr.grads.view(torch.int32))


def test_coarse_only_step():
    from r2l_amd.teacher_train import TeacherTrainer
    csd, fsd = O.make_teacher_state_dicts(5, 2, alpha_bias=0.5)
    tr = TeacherTrainer(make_teacher(csd), None, N_importance=0, perturb=0., white_bkgd=False)
    R = 50
    o, d, vd, tgt = rays(R, 6)
    tr.forward_backward(o.cuda(), d.cuda(), vd.cuda(), 2., 6., tgt.cuda())
    sd = {k: v.double().requires_grad_(True) for k, v in csd.items()}
    t = torch.linspace(0., 1., steps=64)
    z = (2. * (1. - t) + 6. * t).expand(R, 64)
    raw = O.run_network(sd, (o[:, None, :] + d[:, None, :] * z[:, :, None]).double(), vd.double())
    rgb = O.raw2outputs(raw, z.double(), d.double(), None, False)[0]
    torch.mean((rgb - tgt.double())**2).backward()
    want = torch.cat([v.grad.reshape(-1) for v in sd.values()])
    assert nrel(tr.grads.cpu(), want) <= 1e-4


# ---- command line ----------------------------------------------------------------------------------------------------
def make_learnable_scene(root, csd, fsd, size=64):
    """A Blender-layout scene whose images (half_res: 32x32) are renders of a fixed teacher, so the scene is learnable."""
    from PIL import Image
    from r2l_amd import data
    from r2l_amd.render import render
    c, f = make_teacher(csd), make_teacher(fsd)
    focal = .5 * size / np.tan(.5 * 0.6911112070083618)
    for split, n in (("train", 4), ("val", 1), ("test", 1)):
        os.makedirs(os.path.join(root, split))
        frames = []
        for i in range(n):
            pose = data.pose_spherical(90. * i + (45. if split != "train" else 0.), -30., 4.)
            with torch.no_grad():
                rgb = render(size, size, focal, c2w=torch.as_tensor(pose[:3, :4]).cuda(), ndc=False, near=2., far=6.,
                             use_viewdirs=True, network_fn=c, network_fine=f, network_query_fn=None, N_samples=64,
                             N_importance=128, perturb=0., white_bkgd=True)[0]
            img = np.concatenate([(rgb.clamp(0, 1).cpu().numpy() * 255).round().astype(np.uint8),
                                  np.full((size, size, 1), 255, np.uint8)], -1)
            Image.fromarray(img).save(os.path.join(root, split, "r_%d.png" % i))
            frames.append({"file_path": "./%s/r_%d" % (split, i), "transform_matrix": pose.tolist()})
        with open(os.path.join(root, "transforms_%s.json" % split), "w") as fh:
            json.dump({"camera_angle_x": 0.6911112070083618, "frames": frames}, fh)


def test_cli_end_to_end(tmp_path, monkeypatch):
    from r2l_amd import create_data, driver, train_nerf
    from r2l_amd.checkpoint import load_ckpt
    monkeypatch.chdir(tmp_path)
    scene = str(tmp_path / "scene")
    os.makedirs(scene)
    csd, fsd = O.make_teacher_state_dicts(5, 2, alpha_bias=0.5)
    make_learnable_scene(scene, csd, fsd)
    common = ["--config", os.path.join(ROOT, "configs", "lego.txt"), "--datadir", scene, "--testskip", "1", "--N_rand", "256",
              "--precrop_iters", "50", "--i_print", "50", "--lrate_decay", "500"]
    out = train_nerf.main(common + ["--N_iters", "300", "--i_testset", "300", "--i_weights", "300", "--experiment_name", "T"])
    hist = np.array([h[1] for h in out["history"]])
    gain = hist[-30:].mean() - hist[:30].mean()
    print("training PSNR: first 30 steps %.2f dB, last 30 %.2f dB" % (hist[:30].mean(), hist[-30:].mean()))
    assert gain >= 3.0, gain
    ck = os.path.join(out["logger"].weights_path, "ckpt.tar")
    sd = load_ckpt(ck, map_location="cpu")
    for k in ("global_step", "best_psnr", "best_psnr_step", "network_fn_state_dict", "network_fine_state_dict",
              "optimizer_state_dict", "r2l_config"):
        assert k in sd, k
    assert sd["global_step"] == 300 and os.path.exists(os.path.join(out["logger"].weights_path, "ckpt_best.tar"))
    assert len(sd["optimizer_state_dict"]["state"]) == 2 * 24
    # the checkpoint renders through the driver and feeds pseudo-data generation
    r = driver.main(["--model_name", "nerf", "--config", os.path.join(ROOT, "configs", "lego.txt"), "--datadir", scene,
                     "--testskip", "1", "--render_only", "--render_test", "--pretrained_ckpt", ck, "--experiment_name", "R"])
    assert r["rgbs"].shape == (1, 32, 32, 3)
    kd = str(tmp_path / "kd")
    cd = create_data.main(["--create_data", "rand", "--config", os.path.join(ROOT, "configs", "lego.txt"), "--datadir", scene,
                           "--teacher_ckpt", ck, "--n_pose_kd", "4", "--create_data_chunk", "4", "--datadir_kd",
                           scene + ":" + kd, "--experiment_name", "cd", "--testskip", "1"])
    assert cd["n_rays"] == 4 * 32 * 32 and len(os.listdir(kd)) >= 1
    # 2k steps in one run == k steps + --resume k steps, bit for bit
    k = 12
    a = train_nerf.main(common + ["--N_iters", str(2 * k), "--i_testset", "100000", "--i_weights", str(k),
                                  "--save_intermediate_models", "--experiment_name", "A"])
    mid = os.path.join(a["logger"].weights_path, "ckpt_%d.tar" % k)
    b = train_nerf.main(common + ["--N_iters", str(2 * k), "--i_testset", "100000", "--i_weights", str(k),
                                  "--pretrained_ckpt", mid, "--resume", "--experiment_name", "B"])
    assert len(b["history"]) == k
    assert torch.equal(a["trainer"].flat.view(torch.int32), b["trainer"].flat.view(torch.int32))
    assert torch.equal(a["trainer"].exp_avg_sq.view(torch.int32), b["trainer"].exp_avg_sq.view(torch.int32))
