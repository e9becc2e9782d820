"""r2l_pixel_batch and PixelBatcher on the GPU (include/r2l_hip.h "pixel sampler"; r2l_amd/pixel_batch.py; --r2l_batching): every
output against the numpy sampler, against r2l_frame_rays / r2l_ndc_rays gathered at the ids, and against host_batch — all bit for
bit — the argument checks, and train_nerf.main in batching mode with a resume."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.test_llff_cpu import LLFF_CONFIGS, make_llff_scene
from tests.test_llff_gpu import forward_poses
from tests.test_pixel_batch_cpu import record_ids, write_config
from tests.test_teacher_train_cpu import make_scene

pytestmark = pytest.mark.gpu

SEED = (1 << 40) + 12345
G = 8  # guard elements before and after every output
SHAPES = [(1, 1, 1), (1, 4, 4), (1, 1, 17), (3, 5, 7), (4, 64, 64)]
FAR = (1 << 33) + 5
CASES = [(s, w) for s in SHAPES for w in ((0, 5), (0, 257), (FAR, 64))] + [((3, 5, 7), (90, 64)), ((4, 64, 64), (0, 4096 * 256 + 3))]


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def focal_of(W):
    return .9 * W + 3.25


_SCENES = {}


def scene(shape):
    """Per shape, built once and left unchanged: images (pixel g holds g, g + .25, g + .5) and forward-facing poses on both sides,
    and the rays of all frames from r2l_frame_rays, world and through r2l_ndc_rays."""
    if shape not in _SCENES:
        from r2l_amd.render import frame_rays, ndc_rays
        n_img, H, W = shape
        g = torch.arange(n_img * H * W, dtype=torch.float32)
        images = torch.stack([g, g + .25, g + .5], -1).view(n_img, H, W, 3)
        poses = forward_poses(n_img, seed=H)
        s = {"images": images, "poses": poses, "images_dev": images.cuda(), "poses_dev": poses.cuda().contiguous()}
        o, d, v = frame_rays(s["poses_dev"], H, W, focal_of(W))
        assert bool((d[:, 2] != 0).all())
        s["world"] = (o, d, v)
        s["ndc"] = ndc_rays(H, W, focal_of(W), 1., o, d) + (v,)
        _SCENES[shape] = s
    return _SCENES[shape]


def raw_call(s, shape, ndc, draw0, n, seed=SEED, with_ids=True, over=None):
    """One r2l_pixel_batch call into guarded buffers, `over` replacing arguments by name.  Returns (code, {name: whole buffer})."""
    from r2l_amd import _lib
    n_img, H, W = shape
    bufs = {k: torch.full((n * 3 + 2 * G,), -7., device="cuda") for k in ("o", "d", "v", "t")}
    bufs["ids"] = torch.full((n + 2 * G,), -7, dtype=torch.int64, device="cuda")
    a = dict(images=_p(s["images_dev"]), c2w=_p(s["poses_dev"]), n_img=n_img, H=H, W=W, focal=focal_of(W), ndc=ndc, draw0=draw0,
             n_draw=n, seed=seed, ids=_p(bufs["ids"][G:]) if with_ids else None)
    a.update({k: _p(bufs[k][G:]) for k in ("o", "d", "v", "t")})
    a.update(over or {})
    code = _lib.load().r2l_pixel_batch(a["images"], a["c2w"], a["n_img"], a["H"], a["W"], a["focal"], a["ndc"], a["draw0"], a["n_draw"],
                                       a["seed"], a["o"], a["d"], a["v"], a["t"], a["ids"], _st())
    torch.cuda.synchronize()
    return code, bufs


def body(bufs, name, n):
    return bufs[name][G:G + n] if name == "ids" else bufs[name][G:G + n * 3].view(n, 3)


def guards_intact(bufs, n):
    return all(bool((b[:G] == -7).all()) and bool((b[G + n * (1 if k == "ids" else 3):] == -7).all()) for k, b in bufs.items())


@pytest.mark.parametrize("ndc", [0, 1])
@pytest.mark.parametrize("shape,window", CASES)
def test_pixel_batch_bits(shape, window, ndc):
    from r2l_amd.pixel_batch import host_batch, pixel_ids
    n_img, H, W = shape
    M, (draw0, n) = n_img * H * W, window
    s = scene(shape)
    code, bufs = raw_call(s, shape, ndc, draw0, n)
    assert code == 0 and guards_intact(bufs, n)
    # inputs unchanged
    assert torch.equal(s["images_dev"].cpu(), s["images"]) and torch.equal(s["poses_dev"].cpu(), s["poses"])
    ids = body(bufs, "ids", n)
    want_ids = pixel_ids(SEED, M, draw0, n)
    assert np.array_equal(ids.cpu().numpy(), want_ids)
    assert torch.equal(body(bufs, "t", n), s["images_dev"].view(-1, 3)[ids])
    # the rows r2l_frame_rays (and r2l_ndc_rays) write for all frames, gathered at ids
    for name, rows in zip("odv", s["ndc" if ndc else "world"]):
        assert torch.equal(body(bufs, name, n), rows[ids]), name
    # the host specification
    for name, want in zip("odvt", host_batch(s["images"], s["poses"], H, W, focal_of(W), ndc, SEED, draw0, n)[:4]):
        assert torch.equal(body(bufs, name, n), want.cuda()), name
    if ndc and M > 1:
        assert not torch.equal(body(bufs, "d", n), s["world"][1][ids])
    # ids_out = NULL, and the same call again: the same bits
    code2, again = raw_call(s, shape, ndc, draw0, n, with_ids=False)
    assert code2 == 0 and guards_intact(again, n) and bool((again["ids"] == -7).all())
    for name in "odvt":
        assert torch.equal(again[name].view(torch.int32), bufs[name].view(torch.int32)), name


def test_one_epoch_in_batches_of_13_meets_every_pixel_once():
    shape = (3, 5, 7)
    s, met = scene(shape), torch.zeros(105, dtype=torch.int64, device="cuda")
    for draw0 in range(0, 105, 13):
        n = min(13, 105 - draw0)
        code, bufs = raw_call(s, shape, 0, draw0, n)
        assert code == 0
        met += torch.bincount(body(bufs, "ids", n), minlength=105)
    assert bool((met == 1).all())
    code, bufs = raw_call(s, shape, 0, 0, 105, seed=SEED + 1)  # another seed: another order
    other = body(bufs, "ids", 105)
    assert not np.array_equal(other.cpu().numpy(), np.arange(105)) and bool((torch.bincount(other, minlength=105) == 1).all())


def test_no_draws_is_a_successful_no_op():
    code, bufs = raw_call(scene((3, 5, 7)), (3, 5, 7), 1, 17, 0)
    assert code == 0 and all(bool((b == -7).all()) for b in bufs.values())


@pytest.mark.parametrize("over", [
    {"images": None}, {"c2w": None}, {"o": None}, {"d": None}, {"v": None}, {"t": None},
    {"n_img": 0}, {"H": 0}, {"W": -1}, {"focal": 0.}, {"focal": -2.}, {"draw0": -1}, {"n_draw": -1}, {"ndc": 2}, {"ndc": -1},
    {"n_img": 1 << 16, "H": 1 << 8, "W": 1 << 7},  # M = 2^31
    {"n_img": (1 << 31) - 1, "H": (1 << 31) - 1, "W": (1 << 31) - 1},
], ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_invalid_arguments_are_refused_before_any_launch(over):
    from r2l_amd import _lib
    code, bufs = raw_call(scene((3, 5, 7)), (3, 5, 7), 0, 0, 16, over=over)
    assert code == 1  # hipErrorInvalidValue
    msg = _lib.load().r2l_last_error().decode()
    assert "r2l_pixel_batch" in msg and len(msg) > len("r2l_pixel_batch: ")
    assert all(bool((b == -7).all()) for b in bufs.values())  # nothing was launched
    with pytest.raises(RuntimeError, match="r2l_pixel_batch"):
        _lib.check(code, "r2l_pixel_batch")


def test_batcher_hands_out_two_alternating_batches():
    from r2l_amd.pixel_batch import PixelBatcher, host_batch, pixel_ids
    shape = (3, 5, 7)
    s = scene(shape)
    b = PixelBatcher(s["images"], s["poses"], 5, 7, focal_of(7), True, "cuda", seed=SEED)
    assert b.images.is_cuda and b.M == 105 and b.nbytes == 105 * 12 + 3 * 48
    b.seek(90)
    first = b.next(64)
    ids1 = b.last_ids
    second = b.next(64)
    assert b.draw == 90 + 128 and first[0].data_ptr() != second[0].data_ptr()
    for got, ids, draw0 in ((first, ids1, 90), (second, b.last_ids, 154)):  # the first batch outlives the second call
        want = host_batch(s["images"], s["poses"], 5, 7, focal_of(7), 1, SEED, draw0, 64)
        assert all(torch.equal(g, w.cuda()) for g, w in zip(got, want[:4]))
        assert ids.dtype == torch.int64 and np.array_equal(ids.cpu().numpy(), pixel_ids(SEED, 105, draw0, 64))
    third = b.next(64)
    assert third[0].data_ptr() == first[0].data_ptr()  # two sets of buffers, in turn


def test_batcher_refuses_a_bank_that_does_not_fit(monkeypatch):
    from r2l_amd.pixel_batch import PixelBatcher
    s = scene((4, 64, 64))
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (200000, 1 << 30))  # the bank is 196 800 bytes: > 80 %
    before = torch.cuda.memory_allocated()
    with pytest.raises(MemoryError, match="PixelBatcher"):
        PixelBatcher(s["images"], s["poses"], 64, 64, focal_of(64), False, "cuda")
    assert torch.cuda.memory_allocated() == before
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (246001, 1 << 30))  # 80 % is just enough
    assert PixelBatcher(s["images"], s["poses"], 64, 64, focal_of(64), False, "cuda").M == 16384


# ---- train_nerf.main in batching mode -----------------------------------------------------------------------------------------
def run_and_resume(common, seen, M, N_rand, seed):
    """4 iterations, then iterations 3 and 4 again from the checkpoint of iteration 2: the ids of every batch, and the bits at the end."""
    from r2l_amd import train_nerf
    from r2l_amd.pixel_batch import pixel_ids
    a = train_nerf.main(common + ["--experiment_name", "A"])
    assert a["batcher"].M == M and a["batcher"].images.is_cuda and len(a["history"]) == 4
    assert all(np.isfinite(v) for h in a["history"] for v in h)
    assert [d for d, _ in seen] == [(i - 1) * N_rand for i in (1, 2, 3, 4)]
    for draw0, ids in seen:
        assert np.array_equal(ids, pixel_ids(seed, M, draw0, N_rand)), draw0
    log = open(os.path.join(a["logger"].log_path, "log.txt")).read()
    assert "Batching mode" in log and "epoch 0 begins" in log and "Iter 3: epoch 1 begins" in log
    del seen[:]
    mid = os.path.join(a["logger"].weights_path, "ckpt_2.tar")
    b = train_nerf.main(common + ["--experiment_name", "B", "--pretrained_ckpt", mid, "--resume"])
    assert len(b["history"]) == 2 and [d for d, _ in seen] == [2 * N_rand, 3 * N_rand]
    for draw0, ids in seen:
        assert np.array_equal(ids, pixel_ids(seed, M, draw0, N_rand)), draw0
    assert torch.equal(a["trainer"].flat.view(torch.int32), b["trainer"].flat.view(torch.int32))
    assert torch.equal(a["trainer"].exp_avg_sq.view(torch.int32), b["trainer"].exp_avg_sq.view(torch.int32))


def test_cli_batching_mode_and_resume(tmp_path, monkeypatch):
    """2 train views of 8 x 8 (M = 128), N_rand 48: iteration 3 straddles the epoch end."""
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("R2L_SEED", "7")
    root = str(tmp_path / "scene")
    os.makedirs(root)
    make_scene(root)
    common = ["--config", write_config(tmp_path / "teacher.txt"), "--datadir", root, "--testskip", "1", "--N_samples", "8",
              "--N_importance", "8", "--i_print", "1", "--i_testset", "1000", "--i_weights", "2", "--save_intermediate_models",
              "--N_rand", "48", "--N_iters", "4"]
    run_and_resume(common, record_ids(monkeypatch), 128, 48, 7)


def test_cli_batching_mode_on_llff(tmp_path, monkeypatch):
    """NDC rays: 9 views of 16 x 24, 7 of them for training (M = 2688), N_rand 1024: iteration 3 straddles the epoch end."""
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("R2L_SEED", raising=False)
    root = str(tmp_path / "scene")
    make_llff_scene(root, H=32, W=48, factor=2, focal=60.)
    common = ["--config", os.path.join(LLFF_CONFIGS, "fern.txt"), "--datadir", root, "--factor", "2", "--r2l_batching", "--N_iters", "4",
              "--N_rand", "1024", "--i_print", "1", "--i_testset", "1000", "--i_weights", "2", "--save_intermediate_models"]
    seen = record_ids(monkeypatch)
    run_and_resume(common, seen, 2688, 1024, 0)
