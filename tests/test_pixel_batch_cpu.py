"""The pixel sampler of teacher training in batching mode, without a GPU (r2l_amd/pixel_batch.py, --r2l_batching): the draw
numbers against permutations, host_batch against the reference's bank of rays, the switch, and train_nerf.main on the CPU."""
import os

import numpy as np
import pytest
import torch

from tests.test_teacher_train_cpu import make_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = (1 << 40) + 12345


# ---- 1. pixel_ids -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 16, 17, 105])
def test_pixel_ids_epochs_are_permutations_and_windows_are_slices(M):
    from r2l_amd.pixel_batch import pixel_ids
    from r2l_amd.raystore import epoch_key, perm
    epochs = [pixel_ids(SEED, M, e * M, M) for e in range(4)]
    for e, ids in enumerate(epochs):
        assert ids.dtype == np.int64 and np.array_equal(np.sort(ids), np.arange(M))
        assert np.array_equal(ids, perm(epoch_key(SEED, e), M))
    if M > 1:
        assert any(not np.array_equal(epochs[0], epochs[e]) for e in (1, 2, 3))
        other = [pixel_ids(SEED + 1, M, e * M, M) for e in range(4)]
        assert any(not np.array_equal(a, b) for a, b in zip(epochs, other))
    cat = np.concatenate(epochs)
    windows = [(0, 0), (0, 1), (0, M), (M - 1, 2), (M // 2, M), (1, 3 * M - 1), (0, 4 * M), (2 * M, M), (3 * M - 1, M + 1)]
    for draw0, n in windows:
        assert np.array_equal(pixel_ids(SEED, M, draw0, n), cat[draw0:draw0 + n]), (draw0, n)


def test_pixel_ids_far_draws():
    """Draw numbers past 2^33: the epoch is t // M in full integers, and the window is still a slice of that epoch."""
    from r2l_amd.pixel_batch import pixel_ids
    from r2l_amd.raystore import epoch_key, perm
    M, t0 = 105, (1 << 33) + 5
    e, r = divmod(t0, M)
    want = np.concatenate([perm(epoch_key(SEED, e), M), perm(epoch_key(SEED, e + 1), M)])[r:r + 64]
    assert np.array_equal(pixel_ids(SEED, M, t0, 64), want)


# ---- 2. host_batch against the reference's bank -----------------------------------------------------------------------------
def scene_arrays(n_img, H, W, seed=0):
    """(images [n_img,H,W,3] with pixel g holding g, g + .25, g + .5; forward-facing poses [n_img,3,4])."""
    from tests.test_llff_gpu import forward_poses
    g = torch.arange(n_img * H * W, dtype=torch.float32)
    images = torch.stack([g, g + .25, g + .5], -1).view(n_img, H, W, 3)
    return images, forward_poses(n_img, seed)


def reference_bank(images, poses, H, W, focal):
    """main.py:1141-1154 restated: [n_img*H*W, ro+rd+rgb, 3] fp32 (every image is a training image here)."""
    from r2l_amd.render import get_rays_np
    rays = np.stack([np.stack(get_rays_np(H, W, focal, p), 0) for p in poses[:, :3, :4]], 0)  # [N, ro+rd, H, W, 3]
    rays_rgb = np.concatenate([rays, images[:, None]], 1)  # [N, ro+rd+rgb, H, W, 3]
    rays_rgb = np.transpose(rays_rgb, [0, 2, 3, 1, 4])  # [N, H, W, ro+rd+rgb, 3]
    return np.reshape(rays_rgb, [-1, 3, 3]).astype(np.float32)


@pytest.mark.parametrize("n_img,H,W", [(1, 1, 1), (3, 5, 7), (2, 8, 6)])
def test_host_batch_rows_are_the_reference_banks(n_img, H, W):
    from r2l_amd.pixel_batch import host_batch, pixel_ids
    from r2l_amd.render import ndc_rays
    focal, M = .9 * W + 3.25, n_img * H * W
    images, poses = scene_arrays(n_img, H, W)
    bank = reference_bank(images.numpy(), poses.numpy(), H, W, focal)
    assert bank.shape == (M, 3, 3)
    met = np.zeros(M, dtype=np.int64)
    for draw0 in range(0, M, 13):  # one epoch in batches of 13 (the last one shorter)
        n = min(13, M - draw0)
        o, d, v, tgt, ids = host_batch(images, poses, H, W, focal, 0, SEED, draw0, n)
        ids = ids.numpy()
        assert np.array_equal(ids, pixel_ids(SEED, M, draw0, n))
        assert np.array_equal(o.numpy(), bank[ids, 0]) and np.array_equal(d.numpy(), bank[ids, 1])
        assert np.array_equal(tgt.numpy(), bank[ids, 2])
        dd = d.double()
        assert (v.double() - dd / dd.norm(dim=-1, keepdim=True)).abs().max().item() <= 4 * 2.0**-24
        # ndc: the same selection, the world view directions, ndc_rays of the world rays at near plane 1
        no, nd, nv, ntgt, nids = host_batch(images, poses, H, W, focal, 1, SEED, draw0, n)
        wo, wd = ndc_rays(H, W, focal, 1., o, d)
        assert torch.equal(no, wo) and torch.equal(nd, wd) and torch.equal(nv, v) and torch.equal(ntgt, tgt) and torch.equal(nids, torch.from_numpy(ids))
        met[ids] += 1
    assert (met == 1).all()  # over one epoch every row of the bank is met exactly once
    # a window across the epoch end goes on with the next epoch's first draws
    o, d, v, tgt, ids = host_batch(images, poses, H, W, focal, 0, SEED, M - 1, 3)
    assert np.array_equal(ids.numpy(), pixel_ids(SEED, M, M - 1, 3)) and np.array_equal(d.numpy(), bank[ids.numpy(), 1])


def test_batcher_on_cpu_answers_from_host_batch():
    from r2l_amd.pixel_batch import PixelBatcher, host_batch
    images, poses = scene_arrays(3, 5, 7)
    b = PixelBatcher(images, poses, 5, 7, 9.5, True, "cpu", seed=SEED)
    assert b.M == 105 and b.draw == 0 and b.last_ids is None
    b.seek(90)
    got = b.next(64)
    want = host_batch(images, poses, 5, 7, 9.5, 1, SEED, 90, 64)
    assert all(torch.equal(a, w) for a, w in zip(got, want[:4])) and torch.equal(b.last_ids, want[4])
    assert b.draw == 154 and b.epoch() == 1
    with pytest.raises(ValueError):
        b.seek(-1)
    with pytest.raises(ValueError):
        PixelBatcher(images, poses[:2], 5, 7, 9.5, True, "cpu")
    with pytest.raises(ValueError):
        PixelBatcher(images, poses, 5, 7, 0., True, "cpu")


# ---- 3. the switch ----------------------------------------------------------------------------------------------------------
def test_switch_parses_from_command_line_and_config_file(tmp_path):
    from r2l_amd.options import parse_args
    assert parse_args([]).r2l_batching is False
    assert parse_args(["--r2l_batching"]).r2l_batching is True
    cfg = tmp_path / "c.txt"
    cfg.write_text("use_viewdirs = True\nr2l_batching = True\n")
    a = parse_args(["--config", str(cfg)])
    assert a.r2l_batching is True and a.no_batching is False
    cfg.write_text("r2l_batching = False\n")
    assert parse_args(["--config", str(cfg)]).r2l_batching is False


def test_refusal_without_the_switch_names_it():
    from r2l_amd import train_nerf
    with pytest.raises(NotImplementedError, match="no_batching") as e:
        train_nerf.main(["--use_viewdirs", "--N_importance", "128"])
    assert "r2l_batching" in str(e.value)


def write_config(path):
    """A lego-like teacher config without no_batching (the reference's default mode), for 8 x 8 frames."""
    with open(path, "w") as f:
        f.write("dataset_type=blender\nwhite_bkgd=True\nuse_viewdirs=True\nlrate_decay=500\nprecrop_iters=500\nprecrop_frac=0.5\n"
                "r2l_batching=True\n")
    return str(path)


def record_ids(monkeypatch):
    """Every PixelBatcher.next() appends (draw0, ids) to the returned list."""
    from r2l_amd import pixel_batch
    seen, plain = [], pixel_batch.PixelBatcher.next

    def next_(self, n):
        draw0 = self.draw
        out = plain(self, n)
        seen.append((draw0, self.last_ids.cpu().numpy().copy()))
        return out

    monkeypatch.setattr(pixel_batch.PixelBatcher, "next", next_)
    return seen


@pytest.fixture()
def cpu_scene(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    scene = str(tmp_path / "scene")
    os.makedirs(scene)
    make_scene(scene)  # 2 train views of 8 x 8: M = 128
    return ["--config", write_config(tmp_path / "teacher.txt"), "--datadir", scene, "--testskip", "1", "--N_samples", "8",
            "--N_importance", "8", "--i_print", "1", "--i_testset", "1000", "--i_weights", "2", "--save_intermediate_models"]


def test_both_switches_run_images_mode(cpu_scene, monkeypatch):
    from r2l_amd import train_nerf
    seen = record_ids(monkeypatch)
    common = cpu_scene + ["--N_rand", "4", "--N_iters", "2", "--no_batching"]
    a = train_nerf.main(common + ["--experiment_name", "A"])  # (the config carries r2l_batching = True)
    assert a["batcher"] is None and seen == [] and len(a["history"]) == 2
    log = open(os.path.join(a["logger"].log_path, "log.txt")).read()
    assert "Batching mode" not in log and "Center cropping" in log


def test_cli_batching_mode_and_resume_cpu(cpu_scene, monkeypatch):
    from r2l_amd import train_nerf
    from r2l_amd.pixel_batch import pixel_ids
    monkeypatch.setenv("R2L_SEED", "7")
    seen = record_ids(monkeypatch)
    common = cpu_scene + ["--N_rand", "48", "--N_iters", "4"]
    a = train_nerf.main(common + ["--experiment_name", "A"])
    assert a["batcher"].M == 128 and a["batcher"].draw == 4 * 48 and len(a["history"]) == 4
    assert all(np.isfinite(v) for h in a["history"] for v in h)
    assert [d for d, _ in seen] == [0, 48, 96, 144]
    for i, (_, ids) in enumerate(seen, 1):
        assert np.array_equal(ids, pixel_ids(7, 128, (i - 1) * 48, 48)), i
    assert len(set(seen[2][1][:32])) == 32 and len(set(seen[2][1][32:])) == 16  # iteration 3 straddles the epoch end
    log = open(os.path.join(a["logger"].log_path, "log.txt")).read()
    assert "Batching mode" in log and "epoch 0 begins" in log and "Iter 3: epoch 1 begins" in log and "no centre crop" in log
    del seen[:]
    mid = os.path.join(a["logger"].weights_path, "ckpt_2.tar")
    b = train_nerf.main(common + ["--experiment_name", "B", "--pretrained_ckpt", mid, "--resume"])
    assert len(b["history"]) == 2 and b["trainer"].step_count == 4 and [d for d, _ in seen] == [96, 144]
    for i, (_, ids) in zip((3, 4), seen):
        assert np.array_equal(ids, pixel_ids(7, 128, (i - 1) * 48, 48)), i
    for pa, pb in zip(list(a["coarse"].parameters()) + list(a["fine"].parameters()),
                      list(b["coarse"].parameters()) + list(b["fine"].parameters())):
        assert torch.allclose(pa, pb, atol=1e-6)


def test_other_drivers_accept_and_ignore_the_switch():
    from r2l_amd.options import parse_args, validate_accelerated
    a = parse_args(["--config", os.path.join(ROOT, "configs", "lego.txt"), "--r2l_batching"])
    validate_accelerated(a)  # main.py / create_data.py: nothing reads the switch
    import r2l_amd.create_data as cd
    import r2l_amd.driver as dr
    import inspect
    assert "r2l_batching" not in inspect.getsource(cd) and "r2l_batching" not in inspect.getsource(dr)
