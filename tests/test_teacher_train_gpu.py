"""Teacher training on the GPU (r2l_amd/teacher_train.py, csrc/r2l_teacher_train.hip): forward with stash, raw2outputs
backward, full-step gradients against fp64 autograd of the oracle, Adam against torch.optim.Adam, determinism, and the
utils/train_nerf.py command line end to end."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import r2l_oracle as O

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


def layer_outputs(sd, emb):
    """The stashed quantities restated from the oracle's weights: relu(h0..h7), feature, relu(views)."""
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


def oracle_step_grads(csd, fsd, o, d, vd, tgt, t_rand, u, dtype=torch.float64, NS=64, NI=128, white=True, z_dev=None):
    """Autograd of img2mse(rgb) + img2mse(rgb0) built from oracle pieces, z_samples detached (main.py:728).
    z_dev: the (coarse, fine) sample depths the device used.  The oracle's own agree with them to an ulp or so, but the
    encoding's 2^9 frequency turns one ulp of z into ~1e-4 of phase, which the layer-0 weight gradient shows; the yardstick
    restates the step at the device's depths instead (checked against the oracle's below)."""
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
    raw0 = net(sds[0], z)
    rgb0, _, _, w0, _ = O.raw2outputs(raw0, z.to(dtype), d.to(dtype), None, white)
    with torch.no_grad():  # the samples are placed by the fp32 weights, as on the device
        w32 = O.raw2outputs(raw0.float(), z, d, None, white)[3]
        zs = O.sample_pdf(.5 * (z[..., 1:] + z[..., :-1]), w32[..., 1:-1], NI, u=u)
        z_all = torch.sort(torch.cat([z, zs], -1), -1)[0]
        if z_dev is not None:
            assert (z_all - z_dev[1]).abs().max().item() <= 1e-4
            z_all = z_dev[1]
    raw = net(sds[1], z_all)
    rgb = O.raw2outputs(raw, z_all.to(dtype), d.to(dtype), None, white)[0]
    loss = torch.mean((rgb - tgt.to(dtype))**2) + torch.mean((rgb0 - tgt.to(dtype))**2)
    loss.backward()
    return [{k: v.grad for k, v in sd.items()} for sd in sds], loss.item()


@pytest.mark.parametrize("R", [64, 1024])
def test_full_step_gradients_vs_fp64(R):
    from r2l_amd.teacher_train import TeacherTrainer
    csd, fsd = O.make_teacher_state_dicts(5, 2, alpha_bias=0.5)
    tr = TeacherTrainer(make_teacher(csd), make_teacher(fsd), perturb=1., white_bkgd=True)
    o, d, vd, tgt = rays(R, 3)
    t_rand, u = draws(R)
    out = tr.forward_backward(o.cuda(), d.cuda(), vd.cuda(), 2., 6., tgt.cuda(), t_rand=t_rand.cuda(), u=u.cuda())
    want, loss = oracle_step_grads(csd, fsd, o, d, vd, tgt, t_rand, u, z_dev=[z.cpu() for z in tr.last_z])
    assert abs(out[0].item() - loss) < 1e-5 * max(loss, 1.)
    g = tr.grads.cpu()
    off = 0
    worst = []
    for net in want:
        for k, w in net.items():
            got = g[off:off + w.numel()].view(w.shape)
            off += w.numel()
            e = nrel(got, w)
            cos = torch.nn.functional.cosine_similarity(got.double().reshape(1, -1), w.reshape(1, -1)).item()
            worst.append((e, cos, k))
            # Bar 5e-4, not 1e-4: the step's fp32 forward already differs from fp64 by ~1e-7 per activation, ReLU masks of
            # activations that close to zero flip, and the 2^9-frequency encoding columns amplify both in the layer-0
            # gradients.  torch's own fp32 autograd of this step (R = 64) lands at 1.6e-3 on pts_linears.0.weight of the fine
            # net (4.6e-4 on layer 1); the device step measured 2.3e-4 there.
            assert e <= 5e-4 and cos >= 0.99999, (k, e, cos)
    print("worst norm-relative error", max(worst))


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
