"""Forward-facing LLFF scenes on the GPU: r2l_ndc_rays against fp64, the fused NDC frames against the stages they are made of
(bit for bit), an NDC frame against the oracle, a teacher-training step on NDC rays, the pipeline through the four CLIs on a
synthetic scene whose frames are neither square nor a divisor of 4096 rays, and the student's non-square frame."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import r2l_oracle as O
from tests.test_llff_cpu import LLFF_CONFIGS, make_llff_scene
from tests.test_teacher_frames_gpu import _p, _same, _st, nets, rays_fp64

pytestmark = pytest.mark.gpu

U = 2.0**-24  # unit roundoff of fp32


def forward_poses(K, seed=0):
    """K forward-facing poses [K,3,4] (CPU, fp32): rotations <= 0.35 rad about a random axis, origins within +-1.2, |z| <= 0.5."""
    rng = np.random.RandomState(100 + seed)
    out = []
    for _ in range(K):
        axis = rng.randn(3)
        axis /= np.linalg.norm(axis)
        ang = rng.uniform(-.35, .35)
        Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        R = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * (Kx @ Kx)
        out.append(np.concatenate([R, (rng.uniform(-1.2, 1.2, 3) * np.array([1., 1., .5 / 1.2]))[:, None]], 1))
    return torch.from_numpy(np.stack(out).astype(np.float32))


# ---- 1. r2l_ndc_rays against fp64 -------------------------------------------------------------------------------------------
def ndc_fp64(o, d, H, W, focal, near):
    """(o' , d', M_o, M_d), each [n,3] fp64: the header's formula evaluated in fp64 from the same fp32 inputs, and the magnitude
    model of every component (m_i = |o_i| + |t d_i|; s the exact shifted origin):
      o'_x: |cw| (m_x/|s_z| + |s_x| m_z / s_z^2 + |s_x|/|s_z|)      d'_x: the same + |cw d_x / d_z|        (y: ch)
      o'_z: 1 + 2 near/|s_z| + 2 near m_z / s_z^2                   d'_z: the last two terms."""
    o, d, f = o.double(), d.double(), float(np.float32(focal))
    c = [-1. / (W / (2. * f)), -1. / (H / (2. * f))]
    t = -(near + o[:, 2]) / d[:, 2]
    s = o + t[:, None] * d
    m = o.abs() + (t[:, None] * d).abs()
    sz = s[:, 2]
    no = torch.stack([c[0] * s[:, 0] / sz, c[1] * s[:, 1] / sz, 1. + 2. * near / sz], -1)
    nd = torch.stack([c[0] * (d[:, 0] / d[:, 2] - s[:, 0] / sz), c[1] * (d[:, 1] / d[:, 2] - s[:, 1] / sz), -2. * near / sz], -1)
    Mo, Md = [], []
    for i in range(2):
        mo = abs(c[i]) * (m[:, i] / sz.abs() + s[:, i].abs() * m[:, 2] / sz**2 + s[:, i].abs() / sz.abs())
        Mo.append(mo)
        Md.append(mo + (c[i] * d[:, i] / d[:, 2]).abs())
    tail = 2. * near / sz.abs() + 2. * near * m[:, 2] / sz**2
    return no, nd, torch.stack(Mo + [1. + tail], -1), torch.stack(Md + [tail], -1)


@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (33, 31)])
def test_ndc_rays_vs_fp64(H, W):
    """Per component |err| <= 8 * 2^-24 * M (torch's fp32 evaluation in the same order reaches 1.82 * 2^-24 * M at worst over
    such poses, measured on the CPU from 1 x 1 to 378 x 504: 8 leaves a factor of four)."""
    from r2l_amd import _lib, render
    lib = _lib.load()
    focal, near, G = .9 * W + 3.25, 1., 8
    poses = forward_poses(-(-4099 // (H * W)), seed=H)
    rays = [render.get_rays(H, W, focal, p) for p in poses]
    o_all = torch.cat([r[0].reshape(-1, 3) for r in rays]).contiguous()
    d_all = torch.cat([r[1].reshape(-1, 3) for r in rays]).contiguous()
    assert bool((d_all[:, 2] < -.5).all())  # forward-facing: every ray goes down -z
    worst = 0.
    for n in (1, 5, 257, 4099):  # a lone thread, a partial block, one block + 1, grid-stride tails
        o, d = o_all[-n:].contiguous(), d_all[-n:].contiguous()
        og, dg = o.cuda(), d.cuda()
        bo, bd = (torch.full((n * 3 + G,), -7., device="cuda") for _ in range(2))
        _lib.check(lib.r2l_ndc_rays(_p(og), _p(dg), n, H, W, focal, near, _p(bo), _p(bd), _st()), "r2l_ndc_rays")
        assert bool((bo[n * 3:] == -7.).all()) and bool((bd[n * 3:] == -7.).all())  # the guard floats are untouched
        assert torch.equal(og.cpu(), o) and torch.equal(dg.cpu(), d)  # and so are the inputs
        no, nd = bo[:n * 3].view(n, 3).cpu(), bd[:n * 3].view(n, 3).cpu()
        wo, wd, Mo, Md = ndc_fp64(o, d, H, W, focal, near)
        ratio = max(((no.double() - wo).abs() / (U * Mo)).max().item(), ((nd.double() - wd).abs() / (U * Md)).max().item())
        worst = max(worst, ratio)
        assert ratio <= 8., (n, ratio)
        # in place equals out of place
        io, idd = torch.cat([og.reshape(-1), bo[n * 3:]]), torch.cat([dg.reshape(-1), bd[n * 3:]])
        _lib.check(lib.r2l_ndc_rays(_p(io), _p(idd), n, H, W, focal, near, _p(io), _p(idd), _st()), "r2l_ndc_rays")
        assert torch.equal(io[:n * 3].view(n, 3).cpu(), no) and torch.equal(idd[:n * 3].view(n, 3).cpu(), nd)
        assert bool((io[n * 3:] == -7.).all()) and bool((idd[n * 3:] == -7.).all())
        # the wrapper equals the raw call; the CPU evaluation is within the same bound of fp64 and of the device
        ro, rd = render.ndc_rays(H, W, focal, near, og, dg)
        assert torch.equal(ro.cpu(), no) and torch.equal(rd.cpu(), nd)
        co, cd = render.ndc_rays(H, W, focal, near, o, d)
        assert bool(((co.double() - no.double()).abs() <= 8 * U * Mo).all()) and bool(((cd.double() - nd.double()).abs() <= 8 * U * Md).all())
        assert bool(((co.double() - wo).abs() <= 8 * U * Mo).all()) and bool(((cd.double() - wd).abs() <= 8 * U * Md).all())
    print("r2l_ndc_rays %d x %d: max |err| / (2^-24 M) = %.3f" % (H, W, worst))


def test_ndc_rays_wrapper_keeps_the_shape():
    from r2l_amd import render
    o, d = render.get_rays(5, 7, 9., forward_poses(1)[0])
    no, nd = render.ndc_rays(5, 7, 9., 1., o.cuda(), d.cuda())  # rays_o is an expanded view here
    assert no.shape == nd.shape == (5, 7, 3) and no.is_cuda
    assert (no[..., 2].cpu() + 1).abs().max().item() < 1e-5  # origins on the near plane


# ---- 2. fused = unfused -----------------------------------------------------------------------------------------------------
KHW = (3, 20, 24)
BASE_FOCAL = 26.
SEED, FID0 = (1 << 35) + 11, 5


def _poses(K, first=0):
    return forward_poses(KHW[0], seed=77)[first:first + K].cuda()


def _focals(K, first=0):
    return torch.tensor([31.5 + 4.25 * (first + k) for k in range(K)], device="cuda")  # per frame, none equal to BASE_FOCAL


def _fused(N_samples, N_importance, perturb, K=KHW[0], first=0, chunk=0, rows=False, **kw):
    from r2l_amd.render import render_frames
    coarse, fine = nets()
    kw.setdefault("ndc", True)
    if kw["ndc"]:
        kw.setdefault("ndc_focal", BASE_FOCAL)
    with torch.no_grad():
        return render_frames(_poses(K, first), KHW[1], KHW[2], _focals(K, first), 0., 1., coarse, fine, N_samples, N_importance, perturb,
                             False, SEED, frame_id0=FID0 + first, chunk=chunk, rows=rows, **kw)


def _unfused(N_samples, N_importance, perturb, ndc=True):
    """frame_rays (per-frame focal) -> ndc_rays (base focal) -> render_rays with the documented Philox streams."""
    from r2l_amd.render import draw_uniform, frame_rays, ndc_rays, render_rays
    K, H, W = KHW
    coarse, fine = nets()
    o, d, v = frame_rays(_poses(K), H, W, _focals(K))
    no, nd = ndc_rays(H, W, BASE_FOCAL, 1., o, d) if ndc else (o, d)
    out = {k: [] for k in ("rgb", "disp", "acc", "depth", "rgb0")}
    with torch.no_grad():
        for k in range(K):
            s = slice(k * H * W, (k + 1) * H * W)
            ones = torch.ones_like(d[s][:, :1])
            t_rand = u = None
            if perturb:
                t_rand = draw_uniform(H * W * N_samples, SEED, 2 * (FID0 + k), "cuda").view(H * W, N_samples)
                u = draw_uniform(H * W * N_importance, SEED, 2 * (FID0 + k) + 1, "cuda").view(H * W, N_importance) if N_importance else None
            r = render_rays(torch.cat([no[s], nd[s], 0. * ones, ones, v[s]], -1), coarse, None, N_samples, perturb=float(perturb),
                            N_importance=N_importance, network_fine=fine, white_bkgd=False, t_rand=t_rand, u=u)
            for name, key in (("rgb", "rgb_map"), ("disp", "disp_map"), ("acc", "acc_map"), ("depth", "depth_map"), ("rgb0", "rgb0")):
                out[name].append(r.get(key))
    return {k: (torch.cat(v, 0) if v[0] is not None else None) for k, v in out.items()}, torch.cat([o, d], -1)


@pytest.mark.parametrize("perturb", [0, 1])
@pytest.mark.parametrize("N_samples,N_importance", [(64, 64), (64, 0)])
def test_fused_ndc_frames_equal_the_stages(N_samples, N_importance, perturb):
    got = _fused(N_samples, N_importance, perturb, rows=True)
    want, world = _unfused(N_samples, N_importance, perturb)
    R = KHW[0] * KHW[1] * KHW[2]
    assert got["rgb"].shape == (R, 3) and bool(torch.isfinite(got["rgb"]).all()) and got["rgb"].std().item() > 1e-3
    for name in ("rgb", "acc", "depth"):
        assert torch.equal(got[name], want[name]), name
    assert _same(got["disp"], want["disp"])
    if N_importance > 0:
        assert torch.equal(got["rgb0"], want["rgb0"]) and not torch.equal(got["rgb0"], got["rgb"])
    else:
        assert got["rgb0"] is None and want["rgb0"] is None
    # the rows keep the WORLD rays of frame_rays (per-frame focal), and the final rgb
    assert torch.equal(got["rows"][:, 0:6], world) and torch.equal(got["rows"][:, 6:9], got["rgb"])
    # the transform is not a no-op, and it takes the base focal, not the frames'
    assert not torch.equal(got["rgb"], _fused(N_samples, N_importance, perturb, ndc=False)["rgb"])
    assert not torch.equal(got["rgb"], _fused(N_samples, N_importance, perturb, ndc_focal=BASE_FOCAL + 1.)["rgb"])


def test_fused_ndc_grouping_and_chunking_do_not_change_the_frames():
    names = ("rgb", "disp", "acc", "depth", "rgb0", "rows")
    whole = _fused(64, 64, 1, rows=True)
    parts = [_fused(64, 64, 1, K=1, first=0, rows=True), _fused(64, 64, 1, K=2, first=1, rows=True)]
    for n in names:
        assert _same(whole[n], torch.cat([f[n] for f in parts], 0)), n
    for chunk in (100, 480):  # 480 = H * W: one pass; 100: five passes, the last of 80 rays
        part = _fused(64, 64, 1, chunk=chunk, rows=True)
        for n in names:
            assert _same(whole[n], part[n]), (n, chunk)


def test_ndc_off_is_the_call_without_the_keyword():
    from r2l_amd.render import render_frames
    coarse, fine = nets()
    with torch.no_grad():
        plain = render_frames(_poses(3), KHW[1], KHW[2], _focals(3), 2., 6., coarse, fine, 64, 64, 1, True, SEED, frame_id0=FID0, rows=True)
        off = render_frames(_poses(3), KHW[1], KHW[2], _focals(3), 2., 6., coarse, fine, 64, 64, 1, True, SEED, frame_id0=FID0, rows=True,
                            ndc=False)
    for n in ("rgb", "disp", "acc", "depth", "rgb0", "rows"):
        assert _same(plain[n], off[n]), n
    with pytest.raises(ValueError, match="ndc_focal"):
        render_frames(_poses(3), KHW[1], KHW[2], _focals(3), 0., 1., coarse, fine, 64, 64, 1, False, SEED, ndc=True)


# ---- 3. against the oracle --------------------------------------------------------------------------------------------------
def test_ndc_frame_vs_oracle():
    """One 20 x 24 NDC frame of render(c2w=, ndc=True) against the oracle's render_rays fed [o', d', 0, 1, viewdirs] built on the
    CPU: every pixel < 1e-4 (the bar of test_cli_teacher_render_test_vs_oracle), under the three arithmetics."""
    from r2l_amd import render
    csd, fsd = O.make_teacher_state_dicts(7, 2, alpha_bias=0.5)  # the pair of nets()
    coarse, fine = nets()
    H, W, focal = 20, 24, 26.
    pose = forward_poses(1, seed=5)[0]
    o, d = render.get_rays(H, W, focal, pose)
    no, nd = render.ndc_rays(H, W, focal, 1., o, d)
    ones = torch.ones(H * W, 1)
    rb = torch.cat([no.reshape(-1, 3), nd.reshape(-1, 3), 0. * ones, ones, (d / torch.norm(d, dim=-1, keepdim=True)).reshape(-1, 3)], -1)
    with torch.no_grad():
        ref = O.render_rays(rb, csd, fsd, 64, 64, perturb=0., white_bkgd=False)["rgb_map"].view(H, W, 3)
    assert ref.std().item() > 1e-3
    engines = [render.teacher_engine(m) for m in (coarse, fine)]
    try:
        for prec in ("auto", "fp32_mfma", "bf16x3"):
            for e in engines:
                e.set_config(precision=prec)
            with torch.no_grad():
                rgb = render.render(H, W, focal, chunk=H * W, c2w=pose.cuda(), ndc=True, near=0., far=1., use_viewdirs=True,
                                    network_fn=coarse, network_fine=fine, network_query_fn=None, N_samples=64, N_importance=64,
                                    perturb=0., white_bkgd=False, raw_noise_std=0.)[0]
            err = (rgb.cpu() - ref).abs().max().item()
            print("NDC frame vs oracle, %s: max |rgb - ref| = %.2e" % (prec, err))
            assert rgb.shape == (H, W, 3) and err < 1e-4, (prec, err)
    finally:
        for e in engines:
            e.set_config(precision="auto")  # the shared pair is left as it was


# ---- 4. teacher training on NDC rays ----------------------------------------------------------------------------------------
def test_teacher_step_on_ndc_rays():
    """One TeacherTrainer step on 37 NDC rays (32 + 64 samples): the driver's ray preparation (train_nerf.device_rays) gives, bit
    for bit, the gradients of a step fed the o', d' that ndc_rays computed beforehand — the wiring adds nothing but the transform."""
    from r2l_amd import render, train_nerf
    from r2l_amd.teacher_train import TeacherTrainer
    from tests.test_teacher_train_gpu import make_teacher
    csd, fsd = O.make_teacher_state_dicts(5, 2, alpha_bias=0.5)
    tr = TeacherTrainer(make_teacher(csd), make_teacher(fsd), N_samples=32, N_importance=64, perturb=1., white_bkgd=False,
                        raw_noise_std=0.)
    H, W, focal, R = 20, 24, 26., 37
    o, d = render.get_rays(H, W, focal, forward_poses(1, seed=9)[0])
    g = torch.Generator().manual_seed(0)
    pick = torch.randperm(H * W, generator=g)[:R]
    o, d = o.reshape(-1, 3)[pick].contiguous(), d.reshape(-1, 3)[pick].contiguous()
    vd = (d / torch.norm(d, dim=-1, keepdim=True)).cuda()
    tgt = torch.rand(R, 3, generator=g).cuda()
    t_rand, u = torch.rand(R, 32, generator=g).cuda(), torch.rand(R, 64, generator=g).cuda()
    no, nd = train_nerf.device_rays(o, d, H, W, focal, True, torch.device("cuda"))
    tr.forward_backward(no, nd, vd, 0., 1., tgt, t_rand=t_rand, u=u)
    g_driver = tr.grads.clone()
    assert bool(torch.isfinite(g_driver).all()) and g_driver.abs().max().item() > 0
    wo, wd = render.ndc_rays(H, W, focal, 1., o.cuda(), d.cuda())
    assert torch.equal(no, wo) and torch.equal(nd, wd)
    tr.grads.fill_(float("nan"))
    tr.forward_backward(wo, wd, vd, 0., 1., tgt, t_rand=t_rand, u=u)
    assert torch.equal(g_driver.view(torch.int32), tr.grads.view(torch.int32))
    po, pd = train_nerf.device_rays(o, d, H, W, focal, False, torch.device("cuda"))  # ndc off: the world rays, untouched
    assert torch.equal(po.cpu(), o) and torch.equal(pd.cpu(), d)
    tr.forward_backward(po, pd, vd, 0., 1., tgt, t_rand=t_rand, u=u)
    assert not torch.equal(g_driver.view(torch.int32), tr.grads.view(torch.int32))


@pytest.fixture(scope="module")
def llff(tmp_path_factory):
    """A synthetic scene of 9 views, images/ 32 x 48 and images_2/ 16 x 24 (384 rays per pose: not a divisor of 4096), and a
    seeded teacher checkpoint."""
    root = tmp_path_factory.mktemp("llff")
    scene = str(root / "scene")
    make_llff_scene(scene, H=32, W=48, factor=2, focal=60.)
    csd, fsd = O.make_teacher_state_dicts(5, 2, alpha_bias=0.5)
    ck = str(root / "teacher.tar")
    torch.save({"global_step": 200000, "network_fn_state_dict": csd, "network_fine_state_dict": fsd}, ck)
    cfg = str(root / "teacher_cfg.txt")  # a fern-like teacher config for the fused / online paths: no sigma noise
    with open(cfg, "w") as f:
        f.write(open(os.path.join(LLFF_CONFIGS, "fern.txt")).read().replace("raw_noise_std=1e0", "raw_noise_std=0"))
    return {"scene": scene, "ck": ck, "teacher_cfg": cfg, "root": root}


def test_cli_teacher_training_on_llff(llff, tmp_path, monkeypatch):
    """utils/train_nerf.py on the synthetic scene: four iterations log finite loss / PSNR (raw_noise_std = 1 from the config), and
    2 + --resume 2 ends at the weights of the uninterrupted run, bit for bit."""
    from r2l_amd import train_nerf
    monkeypatch.chdir(tmp_path)
    common = ["--config", os.path.join(LLFF_CONFIGS, "fern.txt"), "--datadir", llff["scene"], "--factor", "2", "--no_batching", "--r2l_llff",
              "--N_iters", "4", "--N_rand", "64", "--i_print", "1", "--i_testset", "4", "--i_weights", "2", "--save_intermediate_models"]
    a = train_nerf.main(common + ["--experiment_name", "A"])
    assert len(a["history"]) == 4 and all(np.isfinite(v) for h in a["history"] for v in h)
    log = open(os.path.join(a["logger"].log_path, "log.txt")).read()
    assert "Loaded llff" in log and log.count("[TRAIN] Iter") == 4 and "[TEST] Iter 4" in log
    mid = os.path.join(a["logger"].weights_path, "ckpt_2.tar")
    b = train_nerf.main(common + ["--pretrained_ckpt", mid, "--resume", "--experiment_name", "B"])
    assert len(b["history"]) == 2
    assert torch.equal(a["trainer"].flat.view(torch.int32), b["trainer"].flat.view(torch.int32))
    assert torch.equal(a["trainer"].exp_avg_sq.view(torch.int32), b["trainer"].exp_avg_sq.view(torch.int32))


# ---- 5. the pipeline through the CLI ----------------------------------------------------------------------------------------
def test_cli_pipeline_on_llff(llff, tmp_path, monkeypatch):
    from PIL import Image
    from r2l_amd import create_data, data, driver
    monkeypatch.chdir(tmp_path)
    scene, H, W = llff["scene"], 16, 24
    common = ["--create_data", "rand", "--config", os.path.join(LLFF_CONFIGS, "fern.txt"), "--datadir", scene, "--factor", "2", "--r2l_llff",
              "--teacher_ckpt", llff["ck"], "--n_pose_kd", "12", "--raw_noise_std", "0"]
    # 12 poses x 384 rays = 4608: exactly one [4096,9] shard
    kd = str(tmp_path / "pseudo")
    out = create_data.main(common + ["--datadir_kd", scene + ":" + kd, "--experiment_name", "cd"])
    assert out["n_rays"] == 12 * 384 and os.listdir(kd) == ["data_0.npy"]
    rows = np.load(os.path.join(kd, "data_0.npy"))
    assert rows.shape == (4096, 9) and rows.dtype == np.float32 and np.all(np.isfinite(rows))
    assert (rows[:, 5] < 0).all() and np.abs(rows[:, :3]).max() < 3.  # world rays: directions down -z, origins near the cameras
    assert rows[:, 6:].min() >= -1e-4 and rows[:, 6:].max() <= 1. + 1e-4 and rows[:, 6:].std() > 1e-3
    # the fused path and the per-pose path on the same poses (perturb 0: their draws differ otherwise), row by row
    shards = {}
    for tag, extra in (("plain", []), ("fused", ["--r2l_fused_frames"])):
        d_ = str(tmp_path / ("pseudo_" + tag))
        create_data.main(common + ["--perturb", "0", "--datadir_kd", scene + ":" + d_, "--experiment_name", "cd_" + tag] + extra)
        assert os.listdir(d_) == ["data_0.npy"]
        shards[tag] = np.load(os.path.join(d_, "data_0.npy"))
    sc = data.load_llff_data(scene, factor=2)
    focal = float(sc.poses[0, 2, 4])
    rng = np.random.RandomState(0)  # the rank's stream replayed: (pose, focal scale) x 12, then the flush seed
    pf = [(data.get_rand_pose_llff(sc, rng)[:3, :4], focal * (1 + rng.rand())) for _ in range(12)]
    r = np.random.RandomState(int(rng.randint(0, 2**31 - 1)))
    p1, p2 = r.permutation(4608), r.permutation(4608)
    o, d64, bound = rays_fp64(torch.stack([p for p, _ in pf], 0), [f for _, f in pf], H, W)
    s = p1[p2][:4096]
    a, b = shards["plain"], shards["fused"]
    assert np.array_equal(a[:, :3], o[s].numpy()) and np.array_equal(b[:, :3], o[s].numpy())  # same poses, same permutations
    safe = np.maximum(bound[s].numpy(), 1e-300)
    r_fused = (np.abs(b[:, 3:6].astype(np.float64) - d64[s].numpy()) / safe).max()
    r_pair = (np.abs(b[:, 3:6].astype(np.float64) - a[:, 3:6]) / safe).max()
    e_rgb = np.abs(a[:, 6:] - b[:, 6:]).max()
    print("|d_fused - d64| / bound %.3f, |d_fused - d_plain| / bound %.3f, max |rgb_fused - rgb_plain| %.2e" % (r_fused, r_pair, e_rgb))
    assert r_fused <= 1. and r_pair <= 1. and e_rgb < 1e-4
    with pytest.raises(NotImplementedError, match="--raw_noise_std 0"):  # the config's sigma noise is outside the fused path
        create_data.main([a_ for a_ in common if a_ not in ("--raw_noise_std", "0")] + ["--r2l_fused_frames", "--datadir_kd",
                                                                                      scene + ":" + kd + "_x"])
    # the student: six iterations on the shard, a resume, the test views 0 and 8 at 16 x 24
    student = ["--model_name", "R2L", "--config", os.path.join(LLFF_CONFIGS, "fern_noview.txt"), "--datadir", scene, "--factor", "2",
               "--n_sample_per_ray", "16", "--netwidth", "256", "--netdepth", "6", "--use_residual", "--trial.ON", "--trial.body_arch",
               "resmlp", "--N_rand", "1", "--hard_ratio", "0.2", "--hard_mul", "2", "--warmup_lr", "0.0001,200", "--i_print", "2",
               "--i_testset", "4", "--i_weights", "6", "--n_pose_video", "3"]
    files = ["--datadir_kd", kd, "--data_mode", "rays", "--experiment_name", "train"]
    res = driver.main(student + files + ["--N_iters", "6"])
    ck = os.path.join(res["logger"].weights_path, "ckpt.tar")
    assert np.isfinite(res["trainer"].loss_out[0].item()) and os.path.exists(ck)
    res2 = driver.main(student + files + ["--N_iters", "8", "--pretrained_ckpt", ck, "--resume"])
    assert res2["trainer"].step_count == 8
    res3 = driver.main(student + ["--pretrained_ckpt", ck, "--render_only", "--render_test", "--experiment_name", "render"])
    assert res3["rgbs"].shape == (2, H, W, 3)
    for k in ("test_psnr", "test_psnr_v2", "test_ssim", "test_flip"):
        assert np.isfinite(res3["misc"][k].item()), k
    pngs = sorted(f for f in os.listdir(res3["logger"].gen_img_path) if f.endswith(".png"))
    assert pngs == ["000.png", "000_error.png", "000_gt.png", "001.png", "001_error.png", "001_gt.png"]
    assert all(Image.open(os.path.join(res3["logger"].gen_img_path, f)).size == (W, H) for f in pngs)
    # the teacher's test render of the same views, per pose and fused (teacher frames in NDC)
    for extra in ([], ["--r2l_fused_frames"]):
        t = driver.main(["--model_name", "nerf", "--config", llff["teacher_cfg"], "--datadir", scene, "--factor", "2", "--pretrained_ckpt",
                         llff["ck"], "--render_only", "--render_test", "--experiment_name", "teacher" + str(len(extra))] + extra)
        assert t["rgbs"].shape == (2, H, W, 3) and np.isfinite(t["misc"]["test_psnr"].item())
    # no files at all: the teacher fills a device-resident store (12 x 384 rays -> one shard), two iterations
    res4 = driver.main(student + ["--r2l_online_kd", "--r2l_teacher_config", llff["teacher_cfg"], "--teacher_ckpt", llff["ck"],
                                  "--n_pose_kd", "12", "--N_iters", "2", "--i_print", "1", "--experiment_name", "online"])
    log = open(os.path.join(res4["logger"].log_path, "log.txt")).read()
    assert "ray store: 1 / 1 shards of 4096 rays" in log and log.count("[TRAIN] Iter") == 2
    assert np.isfinite(res4["trainer"].loss_out[0].item())


# ---- 6. the student's non-square frame --------------------------------------------------------------------------------------
def test_student_frames_non_square():
    """r2l_forward_poses_cfg at H, W = 16, 24 with near, far = 0, 1 (the LLFF student samples the WORLD ray at depths in [0, 1])
    against the oracle's forward on PointSampler-style points: 1e-4."""
    from r2l_amd.nerf_raybased import PointSampler
    from tests.test_forward_gpu import build_model
    H, W, focal = 16, 24, 30.
    sd = O.make_state_dict(n_block=2, seed=3)
    model = build_model(sd, 2)
    ps = PointSampler(H, W, focal, 16, 0., 1., device="cuda")
    c2ws = forward_poses(3, seed=21)
    with torch.no_grad():
        got = model.render_poses(c2ws.cuda(), ps).view(3, H, W, 3).cpu()
        one = model.render_pose(c2ws[1].cuda(), ps).view(H, W, 3).cpu()
    dirs, z = O.pixel_dirs(H, W, focal), O.z_vals(16, 0., 1.)
    for k in range(3):
        ref = O.r2l_forward(sd, O.positional_embed(O.sample_test(dirs, z, c2ws[k]), 10)).view(H, W, 3)
        err = (got[k] - ref).abs().max().item()
        print("student frame %d (16 x 24): max |rgb - ref| = %.2e" % (k, err))
        assert err < 1e-4, (k, err)
    assert (one - got[1]).abs().max().item() < 1e-4
