"""Image-filled ray store (include/r2l_hip.h r2l_store_append_images; r2l_amd/raystore.py RayStore.append_images /
append_images_spec; r2l_amd/image_store.py; --r2l_image_store), the parts that need no GPU: the numpy restatement against
render.get_rays per pixel, the library's export and argument checks, the switch and its refusals, and the student CLI on a tiny
scene up to the point where it asks for the GPU."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from tests.test_driver_cpu import ROOT, make_scene

INVALID = 1  # hipErrorInvalidValue


def _group(K=3, H=5, W=7, seed=11):
    rng = np.random.RandomState(seed)
    c2w = rng.randn(K, 3, 4).astype(np.float32)
    focal = (6. + 3. * rng.rand(K)).astype(np.float32)
    images = rng.rand(K, H, W, 3).astype(np.float32)
    return images, c2w, focal


def _all_rows(images, c2w, focal):
    """[K*H*W, 9]: o, d of render.get_rays per frame (the host arithmetic the converters use), rgb the image entry."""
    from r2l_amd.render import get_rays
    K, H, W = images.shape[:3]
    od = []
    for k in range(K):
        o, d = get_rays(H, W, float(focal[k]), torch.from_numpy(c2w[k]))
        od.append(np.concatenate([o.reshape(-1, 3).numpy(), d.reshape(-1, 3).numpy()], 1))
    return np.concatenate([np.concatenate(od, 0), images.reshape(-1, 3)], 1)


@pytest.mark.parametrize("rps", [4, 8])
def test_spec_properties(rps):
    """K = 3 frames of 5 x 7 (105 rows): the rows are a permutation-prefix of all pixels' [o, d, rgb], bit for bit."""
    from r2l_amd import raystore as R
    images, c2w, focal = _group()
    rows9 = _all_rows(images, c2w, focal)
    n_rows, m = 105, 105 // rps
    key = 0xC0FFEE1234
    got = R.append_images_spec(images, c2w, focal, rps, key)
    assert got.dtype == np.float32 and got.shape == (m * rps, 9)
    order = R.perm(key, n_rows)[:m * rps]
    assert len(set(order.tolist())) == m * rps  # a prefix of a permutation: no pixel twice
    assert np.array_equal(got, rows9[order])  # o, d as get_rays gives them, rgb exactly the image entry
    assert np.array_equal(got[:, 6:], images.reshape(-1, 3)[order])
    ident = R.append_images_spec(images, c2w, focal, rps, key, shuffle=False)
    assert np.array_equal(ident, rows9[:m * rps])
    other = R.append_images_spec(images, c2w, focal, rps, key + 1)
    assert not np.array_equal(other, got) and not np.array_equal(got, ident)
    assert np.array_equal(other, rows9[R.perm(key + 1, n_rows)[:m * rps]])
    # a per-frame focal is honoured: frame 1 alone changes when its focal does; one number serves all frames
    f2 = focal.copy()
    f2[1] *= 1.5
    diff = np.any(R.append_images_spec(images, c2w, f2, rps, key, shuffle=False) != ident, axis=1)
    frame = np.arange(m * rps) // 35
    assert diff[frame == 1].all() and not diff[frame != 1].any()
    one = R.append_images_spec(images, c2w, 7.5, rps, key)
    assert np.array_equal(one, _all_rows(images, c2w, np.full(3, 7.5, np.float32))[order])
    # fewer rows than a shard: nothing
    assert R.append_images_spec(images[:1, :1, :3], c2w[:1], focal[:1], rps, key).shape == (0, 9)


def test_library_exports_and_checks_its_arguments():
    """The export, and every refusal as hipErrorInvalidValue with the argument's name in r2l_last_error before anything is
    launched (dummy pointers: this runs without a GPU)."""
    from r2l_amd import _lib
    assert "r2l_store_append_images" in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), "r2l_store_append_images")
    lib = _lib.load()
    img, pose, foc, store = (ctypes.c_void_p(v) for v in (1 << 20, 2 << 20, 3 << 20, 4 << 20))  # never dereferenced
    m = ctypes.c_int64(-5)
    mp = ctypes.cast(ctypes.byref(m), ctypes.c_void_p)

    def call(images=img, c2w=pose, fdev=foc, focal=0., K=1, H=2, W=4, st=store, cap=4, first=0, rps=4, n_written=mp):
        return lib.r2l_store_append_images(images, c2w, fdev, focal, K, H, W, st, cap, first, rps, 1, 1, n_written, None)

    # K*H*W = 8 rows at 4 a shard: m = 2
    for kw, word in ((dict(images=None), b"NULL"), (dict(c2w=None), b"NULL"), (dict(st=None), b"NULL"), (dict(n_written=None), b"NULL"),
                     (dict(K=0), b"K"), (dict(K=-2), b"K"), (dict(H=0), b"H"), (dict(W=0), b"W"), (dict(W=-3), b"W"),
                     (dict(fdev=None, focal=0.), b"focal"), (dict(fdev=None, focal=-1.), b"focal"),
                     (dict(rps=0), b"rays_per_shard"), (dict(rps=-4), b"rays_per_shard"), (dict(rps=6), b"rays_per_shard"),
                     (dict(first=3), b"capacity_shards"), (dict(cap=1), b"capacity_shards"), (dict(first=-1), b"first_shard"),
                     (dict(st=ctypes.c_void_p((4 << 20) + 4)), b"aligned"),
                     (dict(images=ctypes.c_void_p((4 << 20) + 64)), b"overlap"),       # inside the store's 4 * 4 * 36 bytes
                     (dict(images=ctypes.c_void_p((4 << 20) - 8)), b"overlap"),        # its 96 bytes run into the store
                     (dict(K=2**20, H=2**20, W=2**20, cap=2**62), b"K * H * W")):
        assert call(**kw) == INVALID, kw
        msg = lib.r2l_last_error()
        assert b"r2l_store_append_images" in msg and word in msg, (kw, msg)
    assert m.value == -5  # nothing was written on a refused call
    # what needs no launch succeeds without a GPU: fewer rows than a shard
    assert call(rps=12) == 0 and m.value == 0
    # images that END where the store begins do not overlap it: accepted up to the launch (m == 0 here too)
    assert call(images=ctypes.c_void_p((4 << 20) - 96), rps=12) == 0


def test_options(tmp_path):
    from r2l_amd import options
    teacher_cfg = os.path.join(ROOT, "configs", "lego.txt")
    online = ["--r2l_online_kd", "--r2l_teacher_config", teacher_cfg, "--teacher_ckpt", "t.tar", "--n_pose_kd", "12"]
    files = ["--data_mode", "rays", "--datadir_kd", "somewhere"]

    def validate(argv):  # main.py's checks, in its order
        a = options.parse_args(argv)
        options.validate_accelerated(a)
        options.validate_image_store(a)
        options.validate_fused_iter(a)
        options.validate_compact_store(a)
        options.validate_store_file(a)
        return a

    assert options.parse_args([]).r2l_image_store is False
    for argv in (["--r2l_image_store"], ["--r2l_image_store"] + online, ["--r2l_image_store", "--r2l_fused_iter", "--r2l_device_pool"],
                 ["--r2l_image_store"] + online + ["--r2l_store_save", "x.store"], ["--r2l_image_store", "--r2l_store_save", "x.store"]):
        assert validate(argv).r2l_image_store
    cfg = tmp_path / "student.txt"
    cfg.write_text("r2l_image_store = True\n")
    assert validate(["--config", str(cfg)]).r2l_image_store
    cfg.write_text("r2l_image_store = False\n")
    assert not options.parse_args(["--config", str(cfg)]).r2l_image_store
    for argv, words in ((["--r2l_image_store", "--r2l_device_store"] + files, ("--r2l_image_store", "--r2l_device_store")),
                        (["--r2l_image_store", "--r2l_store_load", "x.store"], ("--r2l_image_store", "--r2l_store_load")),
                        (["--r2l_image_store", "--r2l_compact_store"] + online, ("--r2l_image_store", "--r2l_compact_store")),
                        (["--r2l_image_store", "--r2l_compact_store"], ("--r2l_image_store", "--r2l_compact_store")),
                        (["--r2l_image_store", "--r2l_kd_every", "2"] + online, ("--r2l_image_store", "--r2l_kd_every"))):
        with pytest.raises(ValueError) as e:
            validate(argv)
        assert all(w in str(e.value) for w in words), (argv, str(e.value))
    # without the switch the refusals around it read as they always did
    with pytest.raises(ValueError, match="--r2l_compact_store needs --r2l_online_kd"):
        validate(["--r2l_compact_store"])
    with pytest.raises(ValueError, match="it needs --r2l_device_store or --r2l_online_kd"):
        validate(["--r2l_fused_iter"])
    with pytest.raises(ValueError, match="it needs --r2l_online_kd"):
        validate(["--r2l_store_save", "x.store"])
    # the sibling entry points share the option table and run validate_accelerated alone: they accept and ignore the flag
    a = options.parse_args(["--config", teacher_cfg, "--r2l_image_store"])
    assert a.r2l_image_store
    options.validate_accelerated(a)


def test_shard_arithmetic_and_key():
    from r2l_amd import image_store as S
    from r2l_amd.raystore import epoch_key
    assert S.image_shards(100, 400, 400) == (3906, 3906)  # README step 4: 100 frames at 400 x 400, 0.58 GB of rows
    assert "%.2f" % (3906 * 4096 * 36 / 1e9) == "0.58"
    parts = [S.image_shards(100, 400, 400, r, 8)[1] for r in range(8)]
    assert sum(parts) == 3906 and parts == [len(range(r, 3906, 8)) for r in range(8)]
    assert S.image_shards(17, 378, 504) == (17 * 378 * 504 // 4096,) * 2  # LLFF: frames need not be square
    assert S.image_shards(2, 6, 6) == (0, 0)
    assert S.image_group_key(5) == epoch_key(5, S.IMAGE_GROUP) and S.image_group_key(5) != S.image_group_key(6)


def test_student_cli_cpu_plumbing(tmp_path, monkeypatch):
    """`main.py --model_name R2L --r2l_image_store --N_iters 2` on a tiny scene, on CPU: the options, the loader's training split
    and the store's arithmetic run, the log names the store and its shard count, and the run ends where every training run
    without a GPU ends.  Two 64 x 64 training frames (half_res of 128 x 128) = 2 shards."""
    from r2l_amd import driver
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    scene = str(tmp_path / "scene")
    os.makedirs(scene)
    make_scene(scene, size=128)
    common = ["--model_name", "R2L", "--config", os.path.join(ROOT, "configs", "lego_noview.txt"), "--datadir", scene,
              "--n_sample_per_ray", "16", "--netwidth", "256", "--netdepth", "6", "--use_residual", "--trial.ON", "--trial.body_arch",
              "resmlp", "--testskip", "1", "--N_iters", "2", "--i_print", "1", "--r2l_image_store"]
    with pytest.raises(RuntimeError, match="needs a ROCm GPU"):
        driver.main(common + ["--N_rand", "2", "--experiment_name", "image_store_cpu"])
    logs = glob.glob(os.path.join(str(tmp_path), "**", "log.txt"), recursive=True)
    assert len(logs) == 1
    line = [l for l in open(logs[0]).read().splitlines() if "image store (--r2l_image_store)" in l]
    assert len(line) == 1 and "2 training frames of --datadir at 64 x 64 = 8192 real rays -> 2 shards of 4096 rays" in line[0], line
    # fewer shards than one step draws: named at start-up, before the GPU is asked for
    with pytest.raises(ValueError) as e:
        driver.main(common + ["--N_rand", "3", "--experiment_name", "image_store_few"])
    assert "--r2l_image_store" in str(e.value) and "2 shards" in str(e.value) and "draws 3" in str(e.value)
    assert glob.glob(os.path.join(str(tmp_path), "**", "*.npy"), recursive=True) == []  # no shard file anywhere
    # the training split the store is filled from: the loader's composite on white at half_res, the two training poses
    from r2l_amd import data, image_store, options
    a = options.parse_args(common)
    sc = data.load_scene(a)
    images, c2ws = image_store.training_frames(sc, a.white_bkgd)
    assert images.shape == (2, 64, 64, 3) and images.dtype == torch.float32 and c2ws.shape == (2, 3, 4)
    assert torch.equal(images, sc.rgb_images(True)[sc.i_train]) and torch.equal(c2ws, sc.poses[sc.i_train][:, :3, :4])
