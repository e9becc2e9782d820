"""Forward-facing LLFF scenes without a GPU: the loader, the pose generator and ndc_rays against the reference's outputs on a
tiny synthetic scene (tests/golden/llff.npz, written by tests/golden/gen_golden_llff.py), the opt-in switch and its refusals,
the fine-tune conversion, the argument contract of the two ABI additions, and a CPU plumbing run of the student CLI."""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLFF_CONFIGS = os.path.join(ROOT, "configs_llff")


def write_llff_scene(root, poses_bounds, image_sets):
    """poses_bounds.npy + one directory of PNGs per (name, uint8 [N,H,W,3]) pair."""
    from PIL import Image
    os.makedirs(root, exist_ok=True)
    np.save(os.path.join(root, "poses_bounds.npy"), poses_bounds)
    for name, stack in image_sets:
        os.makedirs(os.path.join(root, name), exist_ok=True)
        for i, im in enumerate(stack):
            Image.fromarray(im).save(os.path.join(root, name, "view_%02d.png" % i))


def make_llff_scene(root, H=12, W=16, factor=2, n_views=9, seed=5, focal=20.):
    """A synthetic forward-facing scene: cameras looking down -z, rotations <= 0.35 rad about a random axis, centres within
    +-1 (z within +-0.3), bounds in [1.5, 9]; images/ H x W and images_<factor>/ of random bytes."""
    rng = np.random.RandomState(seed)
    rows = []
    for _ in range(n_views):
        axis = rng.randn(3)
        axis /= np.linalg.norm(axis)
        ang = rng.uniform(-.35, .35)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)  # columns: right, up, back
        pos = rng.uniform(-1, 1, 3) * np.array([1., 1., .3])
        m = np.stack([-R[:, 1], R[:, 0], R[:, 2], pos, np.array([H, W, focal])], 1)  # LLFF stores [down, right, back, pos, hwf]
        near = rng.uniform(1.5, 3.)
        rows.append(np.concatenate([m.reshape(-1), [near, rng.uniform(near + 1., 9.)]]))
    sets = [("images", rng.randint(0, 256, size=(n_views, H, W, 3)).astype(np.uint8)),
            ("images_%d" % factor, rng.randint(0, 256, size=(n_views, H // factor, W // factor, 3)).astype(np.uint8))]
    write_llff_scene(root, np.stack(rows), sets)
    return sets


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "llff.npz")))


@pytest.fixture()
def golden_scene(tmp_path, golden):
    root = str(tmp_path / "scene")
    write_llff_scene(root, golden["poses_bounds"], [("images", golden["imgs"]), ("images_2", golden["imgs2"])])
    return root


def test_loader_equals_the_reference(golden, golden_scene):
    from r2l_amd import data
    sc = data.load_llff_data(golden_scene, factor=2, n_pose_video=int(golden["n_pose_video"]))
    images, poses, bds, render_poses, i_test = sc  # the reference's 5-tuple
    assert images.dtype == poses.dtype == bds.dtype == render_poses.dtype == torch.float32
    assert np.array_equal(images.numpy(), golden["images"]) and images.shape == (9, 6, 8, 3)
    for name, got in (("poses", poses), ("bds", bds), ("render_poses", render_poses)):
        assert got.shape == golden[name].shape, name
        assert np.abs(got.numpy().astype(np.float64) - golden[name]).max() <= 1e-6, name
    assert i_test == int(golden["i_test"]) and i_test != 0
    assert poses[0, :, 4].tolist() == [6., 8., 10.]  # H, W of the loaded images, focal / factor
    # the shim module of the reference's import path
    from dataset.load_llff import load_llff_data
    assert load_llff_data is data.load_llff_data


def test_rand_pose_draws_as_the_reference(golden, golden_scene):
    from r2l_amd import data
    sc = data.load_llff_data(golden_scene, factor=2, n_pose_video=8)
    rng = np.random.RandomState(3)  # np.random.seed(3) in the generator: the same MT19937 stream
    got = np.stack([data.get_rand_pose_llff(sc, rng).numpy() for _ in range(3)])
    assert got.shape == golden["rand_poses"].shape == (3, 3, 5)
    assert np.abs(got.astype(np.float64) - golden["rand_poses"]).max() <= 1e-6
    rng2 = np.random.RandomState(3)
    data.get_rand_pose_llff(sc, rng2)
    ref = np.random.RandomState(3)
    ref.rand(6)
    assert rng2.rand() == ref.rand()  # six draws per pose


def test_ndc_rays_cpu_equals_the_reference_bit_for_bit(golden):
    from r2l_amd import render
    o, d = torch.from_numpy(golden["rays_o"]), torch.from_numpy(golden["rays_d"])
    H, W, focal = 6, 8, float(golden["poses"][0, 2, 4])
    no, nd = render.ndc_rays(H, W, focal, 1., o, d)
    assert no.dtype == torch.float32 and no.shape == (6, 8, 3)
    assert np.array_equal(no.numpy(), golden["ndc_o"]) and np.array_equal(nd.numpy(), golden["ndc_d"])
    # NDC: origins on the near plane z' = -1, the far plane (infinity) at o'_z + d'_z = 1
    assert np.abs(no.numpy()[..., 2] + 1).max() < 1e-5 and np.abs(no.numpy()[..., 2] + nd.numpy()[..., 2] - 1).max() < 1e-5


def test_render_ndc_takes_viewdirs_before_the_transform(golden):
    """render(ndc=True) on CPU tensors (create_data.py:138-152): the batch render_rays sees is [o', d', near, far, d / |d|]."""
    from r2l_amd import render
    o, d = torch.from_numpy(golden["rays_o"]), torch.from_numpy(golden["rays_d"])
    seen = {}

    def fake(rays_flat, chunk, **kw):
        seen["rays"] = rays_flat
        return {k: torch.zeros(rays_flat.shape[0]) for k in ("rgb_map", "disp_map", "acc_map")}

    orig, render.batchify_rays = render.batchify_rays, fake
    try:
        render.render(6, 8, 10., rays=torch.stack([o, d], 0), ndc=True, near=0., far=1., use_viewdirs=True)
    finally:
        render.batchify_rays = orig
    r = seen["rays"]
    assert r.shape == (48, 11)
    assert np.array_equal(r[:, 0:3].numpy(), golden["ndc_o"].reshape(-1, 3)) and np.array_equal(r[:, 3:6].numpy(), golden["ndc_d"].reshape(-1, 3))
    assert torch.equal(r[:, 6], torch.zeros(48)) and torch.equal(r[:, 7], torch.ones(48))
    assert torch.equal(r[:, 8:11], (d / torch.norm(d, dim=-1, keepdim=True)).reshape(-1, 3))


def test_switch_configs_and_refusals(tmp_path, golden_scene):
    from r2l_amd import data
    from r2l_amd.options import FLAGS, IGNORED, parse_args, validate_accelerated
    lego = ["--config", os.path.join(ROOT, "configs", "lego_noview.txt")]
    with pytest.raises(NotImplementedError, match="blender") as e:
        validate_accelerated(parse_args(lego + ["--dataset_type", "llff"]))
    assert "r2l_llff" in str(e.value)
    validate_accelerated(parse_args(lego + ["--dataset_type", "llff", "--r2l_llff"]))
    with pytest.raises(NotImplementedError):  # the switch opens llff only
        validate_accelerated(parse_args(lego + ["--dataset_type", "deepvoxels", "--r2l_llff"]))
    assert parse_args(lego).r2l_llff is False
    assert "factor" in FLAGS and "llffhold" in FLAGS and "factor" not in IGNORED and "spherify" in IGNORED
    for name, viewdirs in (("fern.txt", True), ("fern_noview.txt", False)):
        a = parse_args(["--config", os.path.join(LLFF_CONFIGS, name)])
        assert a.dataset_type == "llff" and a.factor == 8 and a.llffhold == 8 and a.r2l_llff is True
        assert (a.N_samples, a.N_importance, a.raw_noise_std, a.N_rand) == (64, 64, 1., 1024)
        assert a.use_viewdirs is viewdirs and a.datadir.endswith("nerf_llff_data/fern") and not a.white_bkgd
        validate_accelerated(a)
    # the tracked files are the generator's output
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_configs_llff", os.path.join(ROOT, "tools", "gen_configs.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.LLFF_SCENES == ["fern", "flower", "fortress", "horns", "leaves", "orchids", "room", "trex"]
    gen.write_llff_configs(gen.LLFF_SCENES, str(tmp_path / "cfg"))
    assert sorted(os.listdir(LLFF_CONFIGS)) == ["fern.txt", "fern_noview.txt"] and len(os.listdir(str(tmp_path / "cfg"))) == 16
    for name in os.listdir(LLFF_CONFIGS):
        assert open(os.path.join(LLFF_CONFIGS, name)).read() == open(str(tmp_path / "cfg" / name)).read()
    assert parse_args(["--config", str(tmp_path / "cfg" / "trex_noview.txt")]).datadir.endswith("nerf_llff_data/trex")
    # spherify stays refused, by the options and by the loader; a missing images_<factor>/ names the directory
    with pytest.raises(NotImplementedError, match="spherify"):
        validate_accelerated(parse_args(lego + ["--dataset_type", "llff", "--r2l_llff", "--spherify"]))
    with pytest.raises(NotImplementedError, match="spherify"):
        data.load_llff_data(golden_scene, factor=2, spherify=True)
    with pytest.raises(FileNotFoundError, match="images_8"):
        data.load_llff_data(golden_scene, factor=8)
    assert data.load_llff_data(golden_scene, factor=1, n_pose_video=4).images.shape == (9, 12, 16, 3)


def test_load_scene(golden, golden_scene):
    """data.load_scene for LLFF (main.py:890-920, 1010-1011): llffhold split, NDC bounds or the scene's under --no_ndc."""
    from r2l_amd import data
    from r2l_amd.options import parse_args
    base = ["--dataset_type", "llff", "--r2l_llff", "--datadir", golden_scene, "--factor", "2", "--n_pose_video", "8"]
    sc = data.load_scene(parse_args(base))
    assert sc.kind == "llff" and sc.ndc and (sc.near, sc.far) == (0., 1.) and sc.hwf == [6, 8, 10.]
    assert sc.i_test.tolist() == [0, 8] and sc.i_val.tolist() == [0, 8] and sc.i_train.tolist() == [1, 2, 3, 4, 5, 6, 7]
    assert sc.poses.shape == (9, 3, 4) and sc.video_poses is sc.render_poses and sc.render_poses.shape == (8, 3, 5)
    assert torch.equal(sc.rgb_images(True), sc.images) and sc.images.shape == (9, 6, 8, 3)  # no white-background compositing
    assert np.abs(sc.rand_pose(np.random.RandomState(3)).numpy() - golden["rand_poses"][0]).max() <= 1e-6
    sc = data.load_scene(parse_args(base + ["--no_ndc", "--llffhold", "4"]))
    assert not sc.ndc and sc.i_test.tolist() == [0, 4, 8]
    assert sc.near == pytest.approx(float(golden["bds"].min()) * .9) and sc.far == pytest.approx(float(golden["bds"].max()))
    sc = data.load_scene(parse_args(base + ["--llffhold", "0"]))
    assert sc.i_test.tolist() == [int(golden["i_test"])] and len(sc.i_train) == 8


def test_blender_scene_is_what_the_drivers_computed(tmp_path):
    """data.load_scene for Blender: the arrays of load_blender_data, 2 / 6, no NDC, get_rand_pose, get_novel_poses."""
    from r2l_amd import data
    from r2l_amd.options import parse_args
    from tests.test_driver_cpu import make_scene
    root = str(tmp_path / "scene")
    os.makedirs(root)
    make_scene(root)
    args = parse_args(["--config", os.path.join(ROOT, "configs", "lego_noview.txt"), "--datadir", root, "--testskip", "1",
                       "--n_pose_video", "5"])
    sc = data.load_scene(args)
    imgs, poses, render_poses, hwf, i_split = data.load_blender_data(root, True, 1)
    assert torch.equal(sc.images, imgs) and torch.equal(sc.poses, poses) and torch.equal(sc.render_poses, render_poses)
    assert sc.hwf == hwf and (sc.near, sc.far, sc.ndc) == (2., 6., False) and sc.rand_pose is data.get_rand_pose
    assert all(np.array_equal(a, b) for a, b in zip((sc.i_train, sc.i_val, sc.i_test), i_split))
    assert torch.equal(sc.video_poses, data.get_novel_poses(args, n_pose=5))
    assert torch.equal(sc.rgb_images(True), imgs[..., :3] * imgs[..., -1:] + (1. - imgs[..., -1:]))
    assert torch.equal(sc.rgb_images(False), imgs[..., :3])


def test_convert_llff_to_ray_shards(tmp_path, golden, golden_scene):
    """The fine-tune conversion on the 6 x 8 frames with 40-row files: rows are a permutation of world rays + pixels."""
    from r2l_amd import data, render
    savedir, n = data.convert_llff_to_ray_shards(golden_scene, ("train",), "_t", factor=2, llffhold=8, rays_per_file=40,
                                                 rng=np.random.RandomState(0))
    assert savedir == golden_scene + "_real_train_t" and n == (7 * 48) // 40 == 8
    files = sorted(os.listdir(savedir))
    assert files == sorted("train_%d.npy" % k for k in range(1, 9))
    got = np.concatenate([np.load(os.path.join(savedir, "train_%d.npy" % k)) for k in range(1, 9)])
    assert got.dtype == np.float32 and got.shape == (320, 9)
    want = []
    for i in (1, 2, 3, 4, 5, 6, 7):
        o, d = render.get_rays(6, 8, torch.tensor(golden["poses"][i, 2, 4]), torch.from_numpy(golden["poses"][i, :3, :4]))
        want.append(np.concatenate([o.reshape(-1, 3).numpy(), d.reshape(-1, 3).numpy(), golden["images"][i].reshape(-1, 3)], -1))
    want = np.concatenate(want)
    key = lambda a: sorted(map(bytes, np.ascontiguousarray(a.astype(np.float32))))
    have, full = key(got), set(key(want))
    assert len(set(have)) == 320 and set(have) <= full and (want[:, 5] < 0).all()
    # the default file size is the shard format's; the test split takes the held-out views
    savedir, n = data.convert_llff_to_ray_shards(golden_scene, ("test",), "", factor=1, llffhold=8)
    assert n == 0  # 2 x 12 x 16 = 384 rays < 4096: nothing but whole files, as the reference
    savedir, n = data.convert_llff_to_ray_shards(golden_scene, ("train", "test"), "", factor=1, llffhold=8, rays_per_file=64)
    assert n == 27 and np.load(os.path.join(savedir, "traintest_27.npy")).shape == (64, 9)


def _desc(**kw):
    from r2l_amd import _lib
    d = _lib.TeacherFrameDesc(H=20, W=24, focal=30., near=0., far=1., N_samples=64, N_importance=64, perturb=1, white_bkgd=0,
                              raw_noise_std=0., chunk_rays=0, seed=1, frame_id0=0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_descriptor_and_ndc_rays_arguments():
    """The two ABI additions, all device pointers NULL: errors are codes returned before anything is launched."""
    from r2l_amd import _lib
    from tests.test_teacher_frames_cpu import _frames
    lib = _lib.load()
    err = lambda: lib.r2l_last_error().decode()
    assert ctypes.sizeof(_lib.TeacherFrameDesc) == 80 and _lib.TeacherFrameDesc.ndc.offset == 64  # the first reserved word
    for bad in (2, -1):
        d = _desc(ndc=bad)
        assert _frames(lib, d) == 1 and ".ndc" in err(), err()
        assert lib.r2l_teacher_frames_work_floats(ctypes.byref(d)) == -1 and ".ndc" in err()
    word = ctypes.c_float(0.)
    d = _desc(ndc=1, focal=0.)  # ndc takes desc.focal: needed even with a focal_dev
    assert _frames(lib, d, focal_dev=ctypes.addressof(word)) == 1 and "focal" in err() and "ndc" in err()
    assert _frames(lib, _desc(ndc=0, focal=0.), focal_dev=ctypes.addressof(word)) == 1 and "c2w_dev" in err()  # as before
    for kw in ({}, {"chunk_rays": 100}, {"N_importance": 0}, {"perturb": 0}):
        a, b = (lib.r2l_teacher_frames_work_floats(ctypes.byref(_desc(ndc=n, **kw))) for n in (0, 1))
        assert a == b > 0
    d = _desc(ndc=1)
    d.reserved[2] = 1
    assert _frames(lib, d) == 1 and "reserved" in err()
    assert _frames(lib, _desc(ndc=1)) == 1 and "c2w_dev" in err()
    assert _frames(lib, _desc(ndc=1), K=0) == 0
    # r2l_ndc_rays(rays_o, rays_d, n, H, W, focal, near, ndc_o, ndc_d, stream)
    p = ctypes.addressof(word)
    assert lib.r2l_ndc_rays(p, p, -1, 4, 4, 10., 1., p, p, None) == 1 and "n is negative" in err()
    assert lib.r2l_ndc_rays(p, p, 4, 0, 4, 10., 1., p, p, None) == 1 and "H >= 1" in err()
    assert lib.r2l_ndc_rays(p, p, 4, 4, 0, 10., 1., p, p, None) == 1 and "W >= 1" in err()
    assert lib.r2l_ndc_rays(p, p, 4, 4, 4, 0., 1., p, p, None) == 1 and "focal" in err()
    assert lib.r2l_ndc_rays(p, p, 4, 4, 4, -1., 1., p, p, None) == 1 and "focal" in err()
    for k in range(4):
        a = [p, p, p, p]
        a[k] = None
        assert lib.r2l_ndc_rays(a[0], a[1], 4, 4, 4, 10., 1., a[2], a[3], None) == 1 and "NULL" in err()
    assert lib.r2l_ndc_rays(None, None, 0, 4, 4, 10., 1., None, None, None) == 0  # n == 0: a successful no-op


def test_shard_arithmetic_at_a_non_multiple_of_4096():
    """H*W that does not divide 4096 (LLFF: 378 x 504 = 190 512): every flush group keeps floor(rays / 4096) files, the rank's
    index range covers them, write_ray_shards drops the remainder."""
    from r2l_amd import data
    from r2l_amd.create_data import shard_index_base
    from r2l_amd.online_kd import shards_needed
    assert shards_needed(12, 100, 16, 24) == (12 * 384) // 4096 == 1
    assert shards_needed(12, 5, 16, 24) == 0  # 5 x 384 < 4096: such a group keeps nothing
    assert shards_needed(25, 11, 16, 24) == 2 * ((11 * 384) // 4096) + (3 * 384) // 4096 == 2
    assert shards_needed(100, 100, 378, 504) == (100 * 190512) // 4096 == 4651
    assert shards_needed(7, 2, 378, 504, rank=1, world=2) == 2 * ((2 * 190512) // 4096)  # poses 1, 3 | 5, 7
    fpf = (11 * 384) // 4096
    assert [shard_index_base(r, 2, 25, 11, fpf) for r in range(2)] == [0, 2]
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        rows = np.arange(4608 * 9, dtype=np.float32).reshape(4608, 9)
        assert data.write_ray_shards(rows, tmp, 3) == 4 and os.listdir(tmp) == ["data_3.npy"]
        assert np.array_equal(np.load(os.path.join(tmp, "data_3.npy")), rows[:4096])


def test_student_cli_cpu_plumbing(tmp_path, monkeypatch, golden_scene, golden):
    """`main.py --model_name R2L --render_only --render_test` on the LLFF scene, on CPU: the held-out views 0 and 8 at 6 x 8 (a
    non-square frame through the test-set loop, the PNG / video writers, SSIM and FLIP), equal to the oracle's student forward
    on points of the WORLD rays at depths in [0, 1]."""
    from oracle import r2l_oracle as O
    from r2l_amd import driver
    from r2l_amd.checkpoint import save_ckpt
    from r2l_amd.options import parse_args
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    common = ["--model_name", "R2L", "--config", os.path.join(LLFF_CONFIGS, "fern_noview.txt"), "--datadir", golden_scene, "--factor", "2",
              "--n_sample_per_ray", "16", "--netwidth", "256", "--netdepth", "6", "--use_residual", "--trial.ON", "--trial.body_arch",
              "resmlp", "--n_pose_video", "3", "--experiment_name", "llff_cpu"]
    from model.nerf_raybased import NeRF_v3_2
    torch.manual_seed(0)
    net = NeRF_v3_2(parse_args(common), 1008, 3)
    ck = save_ckpt(str(tmp_path / "ckpt.tar"), 7, net, {"state": {}, "param_groups": []}, 0., 0)
    out = driver.main(common + ["--pretrained_ckpt", ck, "--render_only", "--render_test"])
    rgbs, misc = out["rgbs"], out["misc"]
    assert rgbs.shape == (2, 6, 8, 3)
    for k in ("test_psnr", "test_psnr_v2", "test_ssim", "test_flip"):
        assert np.isfinite(misc[k].item()), k
    from PIL import Image
    pngs = sorted(f for f in os.listdir(out["logger"].gen_img_path) if f.endswith(".png"))
    assert pngs == ["000.png", "000_error.png", "000_gt.png", "001.png", "001_error.png", "001_gt.png"]
    assert Image.open(os.path.join(out["logger"].gen_img_path, "001.png")).size == (8, 6)
    gt = np.asarray(Image.open(os.path.join(out["logger"].gen_img_path, "001_gt.png")))
    assert np.array_equal(gt, golden["imgs2"][8])  # view 8 is the second held-out view, written back bit for bit
    for k, view in enumerate((0, 8)):
        pose = torch.from_numpy(golden["poses"][view, :3, :4])
        pts = O.sample_test(O.pixel_dirs(6, 8, float(golden["poses"][0, 2, 4])), O.z_vals(16, 0., 1.), pose)
        ref = O.r2l_forward(net.state_dict(), O.positional_embed(pts, 10)).view(6, 8, 3)
        assert (rgbs[k] - ref).abs().max().item() < 1e-5
    from r2l_amd.video import read_mjpeg_avi
    assert read_mjpeg_avi(out["video_path"])[0].shape == (2, 6, 8, 3)
    # the spiral video poses of the loader
    out = driver.main(common + ["--pretrained_ckpt", ck, "--render_only"])
    assert out["rgbs"].shape == (3, 6, 8, 3)
    # without the switch (a config that lacks it): refused as ever
    with pytest.raises(NotImplementedError, match="blender"):
        driver.main(["--model_name", "R2L", "--dataset_type", "llff", "--datadir", golden_scene, "--render_only"])


def test_teacher_drivers_cpu_plumbing(tmp_path, monkeypatch, golden_scene, golden):
    """The teacher's test render (`--model_name nerf --render_only --render_test`) and two teacher-training iterations on the LLFF
    scene, on CPU: frames equal the oracle's render_rays fed [o', d', 0, 1, viewdirs of the world rays]."""
    from oracle import r2l_oracle as O
    from r2l_amd import driver, render, train_nerf
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    csd, fsd = O.make_teacher_state_dicts(5, 2, alpha_bias=0.5)
    ck = str(tmp_path / "teacher.tar")
    torch.save({"global_step": 1, "network_fn_state_dict": csd, "network_fine_state_dict": fsd}, ck)
    common = ["--config", os.path.join(LLFF_CONFIGS, "fern.txt"), "--datadir", golden_scene, "--factor", "2", "--N_samples", "16",
              "--N_importance", "16"]
    out = driver.main(["--model_name", "nerf"] + common + ["--pretrained_ckpt", ck, "--render_only", "--render_test",
                                                           "--experiment_name", "llff_teacher_cpu"])
    assert out["rgbs"].shape == (2, 6, 8, 3) and np.isfinite(out["misc"]["test_psnr"].item())
    focal = float(golden["poses"][0, 2, 4])
    o, d = render.get_rays(6, 8, focal, torch.from_numpy(golden["poses"][8, :3, :4]))
    no, nd = render.ndc_rays(6, 8, focal, 1., o, d)
    ones = torch.ones(48, 1)
    rb = torch.cat([no.reshape(-1, 3), nd.reshape(-1, 3), 0. * ones, ones, (d / torch.norm(d, dim=-1, keepdim=True)).reshape(-1, 3)], -1)
    with torch.no_grad():
        ref = O.render_rays(rb, csd, fsd, 16, 16, perturb=0., white_bkgd=False)["rgb_map"].view(6, 8, 3)
    assert (out["rgbs"][1] - ref).abs().max().item() < 1e-5
    out = train_nerf.main(common + ["--no_batching", "--N_iters", "2", "--N_rand", "16", "--i_print", "1", "--experiment_name",
                                    "llff_train_cpu"])
    assert len(out["history"]) == 2 and all(np.isfinite(v) for h in out["history"] for v in h)
