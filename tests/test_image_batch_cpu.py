"""The pixel sampler of teacher training in images mode, without a GPU (r2l_amd/image_batch.py, --r2l_image_sampler): the
iteration's image and key, the window's ids against permutations, the crop against train_nerf.precrop_coords, the switch, and
train_nerf.main on the CPU across the end of the centre crop."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from tests.test_teacher_train_cpu import make_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = (1 << 40) + 12345


# ---- 1. image_draw ----------------------------------------------------------------------------------------------------------
def test_image_draw_is_pure_and_in_range():
    from r2l_amd.image_batch import DRAW_SALT, image_draw
    from r2l_amd.raystore import epoch_key
    assert DRAW_SALT == int.from_bytes(b"img_mode", "big")
    for n_img in (1, 3, 100):
        got = [image_draw(SEED, i, n_img) for i in range(1, 301)]
        assert got == [image_draw(SEED, i, n_img) for i in range(1, 301)]
        assert all(0 <= img < n_img and 0 <= key < 2**64 for img, key in got)
        assert len({key for _, key in got}) == 300  # a key of its own per iteration
        z = epoch_key(SEED ^ DRAW_SALT, 17)
        assert image_draw(SEED, 17, n_img) == (((z >> 40) * n_img) >> 24, epoch_key(z, 0))
    assert image_draw(SEED + (1 << 64), 5, 7) == image_draw(SEED, 5, 7)  # the seed is taken mod 2^64
    assert [image_draw(SEED, i, 100) for i in range(1, 20)] != [image_draw(SEED + 1, i, 100) for i in range(1, 20)]
    for bad in ((0, 4), (-1, 4), (1, 0)):
        with pytest.raises(ValueError):
            image_draw(SEED, *bad)


def test_image_draw_meets_every_image_about_equally_often():
    """20 000 iterations over 4 images: 5000 each on average, a standard deviation of 61 — 4000 .. 6000 is 16 of them."""
    from r2l_amd.image_batch import image_draw
    for seed in (0, SEED):
        counts = np.bincount([image_draw(seed, i, 4)[0] for i in range(1, 20001)], minlength=4)
        print("image_draw counts, seed %d:" % seed, counts.tolist())
        assert counts.sum() == 20000 and (counts >= 4000).all() and (counts <= 6000).all()


# ---- 2. window_ids, crop_window ---------------------------------------------------------------------------------------------
WINDOWS = [((1, 1), (0, 0, 1, 1)), ((5, 7), (0, 0, 5, 7)), ((5, 7), (1, 2, 3, 4)), ((5, 7), (4, 6, 1, 1)), ((5, 7), (2, 0, 1, 7)),
           ((5, 7), (0, 3, 5, 1)), ((64, 64), (16, 16, 32, 32))]


@pytest.mark.parametrize("hw,window", WINDOWS)
def test_window_ids_meet_every_window_pixel_once_and_none_outside(hw, window):
    from r2l_amd.image_batch import window_ids
    from r2l_amd.raystore import perm
    (H, W), (row0, col0, wh, ww), img = hw, window, 2
    ids = window_ids(H, W, img, window, SEED, wh * ww)
    assert ids.dtype == np.int64 and ids.shape == (wh * ww,)
    rows, cols = np.meshgrid(np.arange(row0, row0 + wh), np.arange(col0, col0 + ww), indexing="ij")
    inside = ((img * H + rows) * W + cols).reshape(-1)
    assert np.array_equal(np.sort(ids), inside)  # each once, none outside
    assert np.array_equal(ids, inside[perm(SEED, wh * ww)])  # position q of the window, row-major
    for n in (0, 1, min(5, wh * ww)):  # fewer draws: a prefix
        assert np.array_equal(window_ids(H, W, img, window, SEED, n), ids[:n])
    if wh * ww > 4:
        assert not np.array_equal(window_ids(H, W, img, window, SEED + 1, wh * ww), ids)


@pytest.mark.parametrize("window,n", [((0, 0, 0, 7), 0), ((0, 0, 5, 0), 0), ((-1, 0, 2, 2), 1), ((0, -1, 2, 2), 1), ((4, 0, 2, 7), 1),
                                      ((0, 6, 5, 2), 1), ((1, 2, 3, 4), 13), ((1, 2, 3, 4), -1)])
def test_window_ids_refuses_bad_windows(window, n):
    from r2l_amd.image_batch import window_ids
    with pytest.raises(ValueError, match="image batch"):
        window_ids(5, 7, 0, window, SEED, n)


@pytest.mark.parametrize("H,W,frac", [(7, 10, .5), (16, 16, .5), (5, 9, .3)])
def test_crop_window_is_the_reference_crop(H, W, frac):
    from r2l_amd import train_nerf
    from r2l_amd.image_batch import crop_window, full_window
    row0, col0, wh, ww = crop_window(H, W, frac)
    coords = train_nerf.precrop_coords(H, W, frac).long()
    assert tuple(coords.shape) == (wh, ww, 2)
    rows, cols = torch.meshgrid(torch.arange(row0, row0 + wh), torch.arange(col0, col0 + ww), indexing="ij")
    assert torch.equal(coords, torch.stack([rows, cols], -1))
    assert full_window(H, W) == (0, 0, H, W)


def test_host_batch_rows_are_get_rays_of_the_drawn_image():
    from r2l_amd.image_batch import host_batch, window_ids
    from r2l_amd.render import get_rays, ndc_rays
    from tests.test_pixel_batch_cpu import scene_arrays
    H, W, focal, img, window = 5, 7, 9.5, 1, (1, 2, 3, 4)
    images, poses = scene_arrays(3, H, W)
    o, d, v, tgt, ids = host_batch(images, poses, H, W, focal, 0, img, window, SEED, 12)
    assert np.array_equal(ids.numpy(), window_ids(H, W, img, window, SEED, 12))
    pix = ids - img * H * W
    fo, fd = get_rays(H, W, focal, poses[img])
    assert torch.equal(o, fo.reshape(-1, 3)[pix]) and torch.equal(d, fd.reshape(-1, 3)[pix])
    assert torch.equal(tgt, images[img].reshape(-1, 3)[pix])
    dd = d.double()
    assert (v.double() - dd / dd.norm(dim=-1, keepdim=True)).abs().max().item() <= 4 * 2.0**-24
    no, nd, nv, ntgt, nids = host_batch(images, poses, H, W, focal, 1, img, window, SEED, 12)
    wo, wd = ndc_rays(H, W, focal, 1., o, d)
    assert torch.equal(no, wo) and torch.equal(nd, wd) and torch.equal(nv, v) and torch.equal(ntgt, tgt) and torch.equal(nids, ids)
    with pytest.raises(ValueError, match="image 3 of 3"):
        host_batch(images, poses, H, W, focal, 0, 3, window, SEED, 1)


def test_batcher_on_cpu_answers_from_host_batch():
    from r2l_amd.image_batch import ImageBatcher, host_batch, image_draw
    from tests.test_pixel_batch_cpu import scene_arrays
    images, poses = scene_arrays(3, 5, 7)
    b = ImageBatcher(images, poses, 5, 7, 9.5, True, "cpu", seed=SEED)
    assert b.n_img == 3 and b.last_ids is None
    for i, n, window in ((4, 12, (1, 2, 3, 4)), (9, 35, None), (4, 12, (1, 2, 3, 4))):  # any order: nothing to seek
        got = b.next(i, n, window)
        img, key = image_draw(SEED, i, 3)
        want = host_batch(images, poses, 5, 7, 9.5, 1, img, window or (0, 0, 5, 7), key, n)
        assert all(torch.equal(a, w) for a, w in zip(got, want[:4])) and torch.equal(b.last_ids, want[4]) and b.last_img == img
    with pytest.raises(ValueError, match="image batch"):
        b.next(1, 13, (1, 2, 3, 4))
    with pytest.raises(ValueError):
        ImageBatcher(images, poses[:2], 5, 7, 9.5, True, "cpu")


# ---- 3. the switch ----------------------------------------------------------------------------------------------------------
def test_switch_parses_from_command_line_and_config_file(tmp_path):
    from r2l_amd.options import parse_args
    assert parse_args([]).r2l_image_sampler is False
    assert parse_args(["--r2l_image_sampler"]).r2l_image_sampler is True
    cfg = tmp_path / "c.txt"
    cfg.write_text("use_viewdirs = True\nno_batching = True\nr2l_image_sampler = True\n")
    a = parse_args(["--config", str(cfg)])
    assert a.r2l_image_sampler is True and a.no_batching is True
    cfg.write_text("r2l_image_sampler = False\n")
    assert parse_args(["--config", str(cfg)]).r2l_image_sampler is False


def test_other_drivers_accept_and_ignore_the_switch():
    from r2l_amd.options import parse_args, validate_accelerated
    a = parse_args(["--config", os.path.join(ROOT, "configs", "lego.txt"), "--r2l_image_sampler"])
    validate_accelerated(a)  # main.py / create_data.py: nothing reads the switch
    import r2l_amd.create_data as cd
    import r2l_amd.driver as dr
    assert "r2l_image_sampler" not in inspect.getsource(cd) and "r2l_image_sampler" not in inspect.getsource(dr)


def test_library_exports_both_symbols():
    from r2l_amd import _lib
    header = open(os.path.join(ROOT, "include", "r2l_hip.h")).read()
    for name in ("r2l_image_batch", "r2l_image_draw"):
        assert name in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), name) and "int %s(" % name in header


# ---- 4. train_nerf.main on the CPU ------------------------------------------------------------------------------------------
def record_batches(monkeypatch):
    """Every ImageBatcher.next() appends (iteration, image, ids) to the first list returned; every train_nerf.sample_batch() its
    iteration to the second."""
    from r2l_amd import image_batch, train_nerf
    seen, host, plain, plain_host = [], [], image_batch.ImageBatcher.next, train_nerf.sample_batch

    def next_(self, i, n, window=None):
        out = plain(self, i, n, window)
        seen.append((i, self.last_img, self.last_ids.cpu().numpy().copy()))
        return out

    def sample_batch(i, *a, **k):
        host.append(i)
        return plain_host(i, *a, **k)

    monkeypatch.setattr(image_batch.ImageBatcher, "next", next_)
    monkeypatch.setattr(train_nerf, "sample_batch", sample_batch)
    return seen, host


@pytest.fixture()
def cpu_scene(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setenv("R2L_SEED", "7")
    scene = str(tmp_path / "scene")
    os.makedirs(scene)
    make_scene(scene, size=16)  # 2 train views, 8 x 8 at lego.txt's half_res; the centre crop at precrop_frac 0.5 is rows and columns 2 .. 5: 16 pixels
    return ["--config", os.path.join(ROOT, "configs", "lego.txt"), "--datadir", scene, "--testskip", "1", "--N_samples", "8",
            "--N_importance", "8", "--i_print", "1", "--i_testset", "1000", "--i_weights", "1000", "--precrop_iters", "3"]


def in_crop(ids, H=8, W=8, lo=2, hi=5):
    row, col = ids % (H * W) // W, ids % W
    return (row >= lo) & (row <= hi) & (col >= lo) & (col <= hi)


def test_cli_images_mode_from_the_sampler_cpu(cpu_scene, monkeypatch):
    from r2l_amd import train_nerf
    from r2l_amd.image_batch import crop_window, image_draw, window_ids
    seen, host = record_batches(monkeypatch)
    a = train_nerf.main(cpu_scene + ["--N_rand", "12", "--N_iters", "6", "--r2l_image_sampler", "--experiment_name", "A"])
    assert host == [] and a["batcher"] is None and a["image_sampler"].n_img == 2 and len(a["history"]) == 6
    assert all(np.isfinite(v) for h in a["history"] for v in h)
    assert [i for i, _, _ in seen] == [1, 2, 3, 4, 5, 6]
    for i, img, ids in seen:
        want_img, key = image_draw(7, i, 2)
        window = crop_window(8, 8, .5) if i < 3 else (0, 0, 8, 8)
        assert img == want_img and np.array_equal(ids, window_ids(8, 8, img, window, key, 12)), i
        assert len(set(ids.tolist())) == 12 and (ids // 64 == img).all()
        assert bool(in_crop(ids).all()) == (i < 3), i  # in the crop exactly while i < precrop_iters
    log = open(os.path.join(a["logger"].log_path, "log.txt")).read()
    assert "--r2l_image_sampler" in log and "Center cropping of size 4 x 4 is enabled until iter 3" in log


def test_cli_images_mode_without_the_switch_is_the_host_path(cpu_scene, monkeypatch):
    from r2l_amd import train_nerf
    seen, host = record_batches(monkeypatch)
    a = train_nerf.main(cpu_scene + ["--N_rand", "12", "--N_iters", "6", "--experiment_name", "A"])
    assert host == [1, 2, 3, 4, 5, 6] and seen == [] and a["image_sampler"] is None and len(a["history"]) == 6
    log = open(os.path.join(a["logger"].log_path, "log.txt")).read()
    assert "r2l_image_sampler" not in log and "Center cropping of size 4 x 4 is enabled until iter 3" in log


def test_switch_changes_nothing_in_batching_mode(cpu_scene, monkeypatch):
    from r2l_amd import train_nerf
    from tests.test_pixel_batch_cpu import write_config
    seen, host = record_batches(monkeypatch)
    argv = ["--config", write_config("teacher.txt")] + cpu_scene[2:] + ["--N_rand", "12", "--N_iters", "2", "--r2l_image_sampler"]
    a = train_nerf.main(argv + ["--experiment_name", "A"])
    assert a["image_sampler"] is None and a["batcher"].M == 512 and seen == [] and host == []
    assert "r2l_image_sampler" not in open(os.path.join(a["logger"].log_path, "log.txt")).read()


def test_an_n_rand_above_the_crop_is_refused_at_start_up(cpu_scene, monkeypatch):
    from r2l_amd import train_nerf
    seen, host = record_batches(monkeypatch)
    with pytest.raises(ValueError, match="precrop_frac") as e:
        train_nerf.main(cpu_scene + ["--N_rand", "17", "--N_iters", "6", "--r2l_image_sampler"])
    assert "N_rand 17" in str(e.value) and "4 x 4 = 16" in str(e.value)
    with pytest.raises(ValueError, match="precrop_frac") as e:  # no crop, but more than a frame holds
        train_nerf.main(cpu_scene + ["--N_rand", "65", "--N_iters", "6", "--r2l_image_sampler", "--precrop_iters", "0"])
    assert "8 x 8 = 64" in str(e.value)
    assert seen == [] and host == []
    # 16 is the whole crop, 64 the whole frame: both run
    train_nerf.main(cpu_scene + ["--N_rand", "16", "--N_iters", "1", "--r2l_image_sampler"])
    train_nerf.main(cpu_scene + ["--N_rand", "64", "--N_iters", "1", "--r2l_image_sampler", "--precrop_iters", "0"])
    assert [len(ids) for _, _, ids in seen] == [16, 64]
