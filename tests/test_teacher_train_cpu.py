"""CPU plumbing of teacher training (r2l_amd/teacher_train.py, r2l_amd/train_nerf.py): pixel selection, LR schedule,
optimizer state, checkpoint layout and resume, and the loud refusals."""
import os

import numpy as np
import pytest
import torch

from oracle import r2l_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ref_coords(H, W, i, precrop_iters, precrop_frac):
    """main.py:1270-1284, restated."""
    if i < precrop_iters:
        dH = int(H // 2 * precrop_frac)
        dW = int(W // 2 * precrop_frac)
        return torch.stack(torch.meshgrid(torch.linspace(H // 2 - dH, H // 2 + dH - 1, 2 * dH),
                                          torch.linspace(W // 2 - dW, W // 2 + dW - 1, 2 * dW), indexing="ij"), -1)
    return torch.stack(torch.meshgrid(torch.linspace(0, H - 1, H), torch.linspace(0, W - 1, W), indexing="ij"), -1)


def ref_selected_coords(coords, N_rand):
    """get_selected_coords(..., 'rand_pixel') of helpers:385-392, restated."""
    coords = coords.long()
    H, W = coords.shape[:2]
    rand_ix = np.random.choice(H * W, size=[N_rand], replace=False)
    return coords.view(-1, 2)[rand_ix]


@pytest.mark.parametrize("H,W,frac", [(400, 400, .5), (32, 32, .5), (37, 21, .3)])
def test_precrop_and_rand_pixel(H, W, frac):
    from r2l_amd.train_nerf import full_coords, precrop_coords, select_rand_pixels
    assert torch.equal(precrop_coords(H, W, frac), ref_coords(H, W, 0, 10, frac))
    assert torch.equal(full_coords(H, W), ref_coords(H, W, 10, 10, frac))
    n = min(64, (2 * int(H // 2 * frac)) * (2 * int(W // 2 * frac)))
    np.random.seed(7)
    got = select_rand_pixels(precrop_coords(H, W, frac), n)
    np.random.seed(7)
    want = ref_selected_coords(ref_coords(H, W, 0, 10, frac), n)
    assert torch.equal(got, want)
    assert len({tuple(c) for c in got.tolist()}) == n  # without replacement


def test_lr_schedule_teacher_decay():
    from r2l_amd.train_step import lr_schedule
    for step in (1, 1000, 250000, 500000):
        assert lr_schedule(step, 5e-4, 500) == pytest.approx(5e-4 * 0.1**(step / 500000), rel=1e-12)


def cpu_trainer(N_importance=128, seed=5):
    from model.nerf_raybased import NeRF
    from r2l_amd.teacher_train import TeacherTrainer
    csd, fsd = O.make_teacher_state_dicts(seed, 2, alpha_bias=0.5)
    nets = []
    for sd in (csd, fsd):
        m = NeRF(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
        m.load_state_dict(sd)
        nets.append(m)
    return TeacherTrainer(nets[0], nets[1], N_samples=16, N_importance=N_importance, perturb=1.), nets


def batch(R, seed):
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(R, 3, generator=g) * .5
    d = torch.randn(R, 3, generator=g)
    return o, d, d / d.norm(dim=-1, keepdim=True), torch.rand(R, 3, generator=g)


def test_cpu_step_and_optimizer_state_round_trip():
    tr, nets = cpu_trainer()
    R = 8
    for s in range(2):
        o, d, vd, tgt = batch(R, s)
        loss, psnr = tr.step(o, d, vd, 2., 6., tgt, 5e-4, t_rand=torch.rand(R, 16), u=torch.rand(R, 128))
        assert np.isfinite(loss) and psnr == pytest.approx(-10 * np.log10(loss), abs=10)
    sd = tr.optimizer_state_dict(5e-4)
    params = list(nets[0].parameters()) + list(nets[1].parameters())
    assert len(sd["state"]) == len(params) == 48 and sd["param_groups"][0]["lr"] == 5e-4
    opt = torch.optim.Adam(params, lr=5e-4)
    opt.load_state_dict(sd)  # the torch.optim.Adam layout: one param group, coarse then fine
    for i, p in enumerate(params):
        assert opt.state[p]["exp_avg"].shape == p.shape and float(opt.state[p]["step"]) == 2
    tr2, _ = cpu_trainer()
    tr2.load_optimizer_state_dict(sd)
    assert tr2.step_count == 2
    with pytest.raises(ValueError):
        cpu_trainer(N_importance=0)[0].load_optimizer_state_dict(sd)


def make_scene(root, size=8):
    import json
    from PIL import Image
    from r2l_amd import data
    rng = np.random.RandomState(0)
    for split, n in (("train", 2), ("val", 1), ("test", 1)):
        os.makedirs(os.path.join(root, split))
        frames = []
        for i in range(n):
            Image.fromarray((rng.rand(size, size, 4) * 255).astype(np.uint8)).save(os.path.join(root, split, "r_%d.png" % i))
            frames.append({"file_path": "./%s/r_%d" % (split, i), "transform_matrix": data.pose_spherical(40. * i, -30., 4.).tolist()})
        with open(os.path.join(root, "transforms_%s.json" % split), "w") as f:
            json.dump({"camera_angle_x": 0.6911112070083618, "frames": frames}, f)


def test_cli_checkpoint_layout_and_resume_cpu(tmp_path, monkeypatch):
    from r2l_amd import train_nerf
    from r2l_amd.checkpoint import load_ckpt
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    scene = str(tmp_path / "scene")
    os.makedirs(scene)
    make_scene(scene)
    common = ["--config", os.path.join(ROOT, "configs", "lego.txt"), "--datadir", scene, "--testskip", "1", "--N_rand", "4",
              "--N_samples", "8", "--N_importance", "8", "--precrop_iters", "2", "--i_print", "1", "--i_testset", "1000",
              "--N_iters", "4", "--i_weights", "2", "--save_intermediate_models"]
    a = train_nerf.main(common + ["--experiment_name", "A"])
    ck = load_ckpt(os.path.join(a["logger"].weights_path, "ckpt_4.tar"), map_location="cpu")
    assert set(ck) >= {"global_step", "best_psnr", "best_psnr_step", "network_fn_state_dict", "network_fine_state_dict",
                       "optimizer_state_dict", "r2l_config"}
    assert ck["global_step"] == 4 and len(ck["optimizer_state_dict"]["state"]) == 48
    assert list(ck["network_fn_state_dict"])[0] == "pts_linears.0.weight"
    mid = os.path.join(a["logger"].weights_path, "ckpt_2.tar")
    b = train_nerf.main(common + ["--experiment_name", "B", "--pretrained_ckpt", mid, "--resume"])
    assert len(b["history"]) == 2 and b["trainer"].step_count == 4
    for pa, pb in zip(list(a["coarse"].parameters()) + list(a["fine"].parameters()),
                      list(b["coarse"].parameters()) + list(b["fine"].parameters())):
        assert torch.allclose(pa, pb, atol=1e-6)


@pytest.mark.parametrize("extra,env,match", [
    (["--use_batching_is_default"], {}, None),
    ([], {"WORLD_SIZE": "2"}, "one GPU"),
    (["--r2l_precision", "fp16x2"], {}, "fp32"),
    (["--dataset_type", "llff"], {}, "blender"),
    (["--N_samples", "64", "--N_importance", "193"], {}, "at most 256 samples"),
    (["--N_samples", "257", "--N_importance", "0"], {}, "at most 256 samples"),
])
def test_loud_refusals(extra, env, match, monkeypatch):
    from r2l_amd import train_nerf
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    argv = ["--config", os.path.join(ROOT, "configs", "lego.txt")]
    if extra == ["--use_batching_is_default"]:  # no_batching=False: the reference's use_batching mode
        argv = ["--use_viewdirs", "--N_importance", "128"]
        match = "no_batching"
    else:
        argv += extra
    with pytest.raises(NotImplementedError, match=match):
        train_nerf.main(argv)


def test_main_still_refuses_nerf_training():
    from r2l_amd import driver
    with pytest.raises(NotImplementedError, match="TRAINING"):
        driver.main(["--model_name", "nerf", "--config", os.path.join(ROOT, "configs", "lego.txt")])


@pytest.mark.parametrize("R,S", [(1, 1), (1, 15), (3, 5), (2, 43)])
def test_backward_yardstick_vs_fp64_autograd(R, S):
    """tests/teacher_util.teacher_backward_from_stash, fed the stash of an fp64 forward, is fp64 autograd of run_network
    contracted with draw (1e-12 of each entry's magnitude), and its magnitudes bound the gradients.  This pins the yardstick of
    tests/test_teacher_backward_gpu.py without a GPU."""
    from tests.teacher_util import layer_outputs, teacher_backward_from_stash
    sd = O.make_teacher_state_dicts(7, 1, alpha_bias=0.5)[0]
    g = torch.Generator().manual_seed(R * 100 + S)
    o = torch.randn(R, 3, generator=g) * .5
    d = torch.randn(R, 3, generator=g)
    vd = d / d.norm(dim=-1, keepdim=True)
    z = torch.sort(torch.rand(R, S, generator=g) * 4 + 2, -1)[0]
    draw = torch.randn(R, S, 4, generator=g, dtype=torch.float64)
    pts = (o[:, None, :] + d[:, None, :] * z[:, :, None]).double()  # the fp32 points, as the kernels form them
    sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    raw = O.run_network(sd64, pts, vd.double())
    (raw * draw).sum().backward()
    with torch.no_grad():
        emb = torch.cat([O.nerf_embed(pts.reshape(-1, 3), 10), O.nerf_embed(vd.double()[:, None].expand(R, S, 3).reshape(-1, 3), 4)], -1)
        stash = torch.cat([t.reshape(-1) for t in layer_outputs({k: v.detach() for k, v in sd64.items()}, emb)])
    grads, mags = teacher_backward_from_stash(sd, o, d, vd, z, stash, draw)
    assert list(grads) == list(sd) == list(mags)
    for k, want in ((k, v.grad) for k, v in sd64.items()):
        err = (grads[k] - want).abs()
        assert (err <= 1e-12 * mags[k] + 1e-300).all(), (k, (err / mags[k].clamp_min(1e-300)).max().item())
        assert (want.abs() <= mags[k] * (1 + 1e-12)).all(), k
        assert mags[k].max().item() > 0, k
