"""r2l_image_batch, r2l_image_draw and ImageBatcher on the GPU (include/r2l_hip.h "pixel sampler ... images mode";
r2l_amd/image_batch.py; --r2l_image_sampler): every output against the numpy sampler, against r2l_frame_rays / r2l_ndc_rays
gathered at the ids, and against host_batch — all bit for bit — the argument checks, and train_nerf.main in images mode from the
sampler with a resume."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.test_image_batch_cpu import in_crop, record_batches
from tests.test_llff_cpu import LLFF_CONFIGS, make_llff_scene
from tests.test_pixel_batch_gpu import G, SHAPES, _p, _st, body, focal_of, guards_intact, scene
from tests.test_teacher_train_cpu import make_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = (0xC0FFEE << 32) + 977


def windows_of(H, W):
    """The whole frame, an interior window touching no edge (where the frame has one), a 1 x 1 window, a single row, a single
    column; (row0, col0, win_h, win_w), each once."""
    out = [(0, 0, H, W)]
    if H >= 3 and W >= 3:
        out.append((1, 1, H - 2, W - 2))
    out += [(H - 1, W - 1, 1, 1), (H // 2, 0, 1, W), (0, W // 2, H, 1)]
    return list(dict.fromkeys(out))


def raw_call(s, shape, ndc, img, window, n, key=KEY, with_ids=True, over=None):
    """One r2l_image_batch call into guarded buffers, `over` replacing arguments by name.  Returns (code, {name: whole buffer})."""
    from r2l_amd import _lib
    n_img, H, W = shape
    bufs = {k: torch.full((n * 3 + 2 * G,), -7., device="cuda") for k in ("o", "d", "v", "t")}
    bufs["ids"] = torch.full((n + 2 * G,), -7, dtype=torch.int64, device="cuda")
    a = dict(images=_p(s["images_dev"]), c2w=_p(s["poses_dev"]), n_img=n_img, H=H, W=W, focal=focal_of(W), ndc=ndc, img=img,
             row0=window[0], col0=window[1], win_h=window[2], win_w=window[3], key=key, n_draw=n,
             ids=_p(bufs["ids"][G:]) if with_ids else None)
    a.update({k: _p(bufs[k][G:]) for k in ("o", "d", "v", "t")})
    a.update(over or {})
    code = _lib.load().r2l_image_batch(a["images"], a["c2w"], a["n_img"], a["H"], a["W"], a["focal"], a["ndc"], a["img"], a["row0"],
                                       a["col0"], a["win_h"], a["win_w"], a["key"], a["n_draw"], a["o"], a["d"], a["v"], a["t"],
                                       a["ids"], _st())
    torch.cuda.synchronize()
    return code, bufs


@pytest.mark.parametrize("ndc", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_image_batch_bits(shape, ndc):
    """Per shape: img in {0, n_img - 1} x the five windows x n_draw in {1, 5, the window, 257} (where it fits)."""
    from r2l_amd.image_batch import host_batch, window_ids
    n_img, H, W = shape
    s = scene(shape)
    n_cases = 0
    for img in sorted({0, n_img - 1}):
        for window in windows_of(H, W):
            n_win = window[2] * window[3]
            for n in sorted({m for m in (1, 5, 257, n_win) if m <= n_win}):
                what = (img, window, n)
                code, bufs = raw_call(s, shape, ndc, img, window, n)
                assert code == 0 and guards_intact(bufs, n), what
                ids = body(bufs, "ids", n)
                want_ids = window_ids(H, W, img, window, KEY, n)
                assert np.array_equal(ids.cpu().numpy(), want_ids), what
                assert torch.equal(body(bufs, "t", n), s["images_dev"].view(-1, 3)[ids]), what
                # the rows r2l_frame_rays (and r2l_ndc_rays) write for all frames, gathered at ids
                for name, rows in zip("odv", s["ndc" if ndc else "world"]):
                    assert torch.equal(body(bufs, name, n), rows[ids]), (name, what)
                # the host specification
                for name, want in zip("odvt", host_batch(s["images"], s["poses"], H, W, focal_of(W), ndc, img, window, KEY, n)[:4]):
                    assert torch.equal(body(bufs, name, n), want.cuda()), (name, what)
                if n == n_win:  # the whole window: every pixel of it once, none outside
                    rows, cols = np.meshgrid(np.arange(window[0], window[0] + window[2]),
                                             np.arange(window[1], window[1] + window[3]), indexing="ij")
                    assert np.array_equal(np.sort(ids.cpu().numpy()), ((img * H + rows) * W + cols).reshape(-1)), what
                # ids_out = NULL, and the same call again: the same bits
                code2, again = raw_call(s, shape, ndc, img, window, n, with_ids=False)
                assert code2 == 0 and guards_intact(again, n) and bool((again["ids"] == -7).all()), what
                for name in "odvt":
                    assert torch.equal(again[name].view(torch.int32), bufs[name].view(torch.int32)), (name, what)
                n_cases += 1
    assert n_cases >= (2 if n_img > 1 else 1)
    # inputs unchanged
    assert torch.equal(s["images_dev"].cpu(), s["images"]) and torch.equal(s["poses_dev"].cpu(), s["poses"])


def test_another_key_is_another_order_and_no_draws_is_a_successful_no_op():
    shape, window = (4, 64, 64), (16, 16, 32, 32)
    s = scene(shape)
    a = body(raw_call(s, shape, 0, 3, window, 1024)[1], "ids", 1024)
    b = body(raw_call(s, shape, 0, 3, window, 1024, key=KEY + 1)[1], "ids", 1024)
    assert not torch.equal(a, b) and torch.equal(torch.sort(a)[0], torch.sort(b)[0])
    code, bufs = raw_call(s, shape, 1, 3, window, 0)
    assert code == 0 and all(bool((x == -7).all()) for x in bufs.values())


@pytest.mark.parametrize("over", [
    {"images": None}, {"c2w": None}, {"o": None}, {"d": None}, {"v": None}, {"t": None},
    {"n_img": 0}, {"H": 0}, {"W": -1}, {"focal": 0.}, {"focal": -2.}, {"n_draw": -1}, {"ndc": 2}, {"ndc": -1},
    {"n_img": 1 << 16, "H": 1 << 8, "W": 1 << 7},  # M = 2^31
    {"n_img": (1 << 31) - 1, "H": (1 << 31) - 1, "W": (1 << 31) - 1},
    {"img": -1}, {"img": 3}, {"win_h": 0}, {"win_w": 0}, {"win_h": -1}, {"row0": -1}, {"col0": -1},
    {"row0": 3}, {"col0": 4}, {"win_h": 5}, {"win_w": 6},  # the window (1, 2, 3, 4) of a 5 x 7 frame, pushed over an edge
    {"row0": (1 << 31) - 1, "win_h": (1 << 31) - 1}, {"col0": (1 << 31) - 1, "win_w": (1 << 31) - 1},  # sums past 2^31
    {"n_draw": 13}, {"n_draw": 1 << 40},
], ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_invalid_arguments_are_refused_before_any_launch(over):
    from r2l_amd import _lib
    code, bufs = raw_call(scene((3, 5, 7)), (3, 5, 7), 0, 1, (1, 2, 3, 4), 12, over=over)
    assert code == 1  # hipErrorInvalidValue
    msg = _lib.load().r2l_last_error().decode()
    assert "r2l_image_batch" in msg and len(msg) > len("r2l_image_batch: ")
    assert all(bool((b == -7).all()) for b in bufs.values())  # nothing was launched
    with pytest.raises(RuntimeError, match="r2l_image_batch"):
        _lib.check(code, "r2l_image_batch")


def test_image_draw_of_the_library_is_image_draw():
    from r2l_amd import _lib
    from r2l_amd.image_batch import image_draw
    L = _lib.load()
    img, key = ctypes.c_int(-1), ctypes.c_uint64(0)
    for seed, n_img in ((0, 100), ((1 << 63) + 12345, 7)):
        for i in range(1, 1001):
            assert L.r2l_image_draw(seed, i, n_img, ctypes.byref(img), ctypes.byref(key)) == 0
            assert (img.value, key.value) == image_draw(seed, i, n_img), (seed, i)
    img.value, key.value = -5, 99
    for it, n_img, pi, pk in ((0, 4, img, key), (-1, 4, img, key), (1, 0, img, key), (1, 4, None, key), (1, 4, img, None)):
        code = L.r2l_image_draw(0, it, n_img, ctypes.byref(pi) if pi is not None else None, ctypes.byref(pk) if pk is not None else None)
        assert code == 1 and "r2l_image_draw" in L.r2l_last_error().decode()
    assert (img.value, key.value) == (-5, 99)


def test_batcher_hands_out_two_alternating_batches():
    from r2l_amd.image_batch import ImageBatcher, host_batch, image_draw, window_ids
    shape, window = (3, 5, 7), (1, 2, 3, 4)
    s = scene(shape)
    b = ImageBatcher(s["images"], s["poses"], 5, 7, focal_of(7), True, "cuda", seed=KEY)
    assert b.images.is_cuda and b.n_img == 3 and b.nbytes == 105 * 12 + 3 * 48
    first = b.next(5, 12, window)
    ids1 = b.last_ids
    second = b.next(6, 12)  # the whole frame
    assert first[0].data_ptr() != second[0].data_ptr()
    for got, ids, i, win in ((first, ids1, 5, window), (second, b.last_ids, 6, (0, 0, 5, 7))):  # the first batch outlives the second call
        img, key = image_draw(KEY, i, 3)
        want = host_batch(s["images"], s["poses"], 5, 7, focal_of(7), 1, img, win, key, 12)
        assert all(torch.equal(g, w.cuda()) for g, w in zip(got, want[:4]))
        assert ids.dtype == torch.int64 and np.array_equal(ids.cpu().numpy(), window_ids(5, 7, img, win, key, 12))
    third = b.next(5, 12, window)
    assert third[0].data_ptr() == first[0].data_ptr()  # two sets of buffers, in turn
    assert all(torch.equal(a, c) for a, c in zip(third, first))  # and iteration 5 again: a pure function of (seed, i)
    with pytest.raises(ValueError, match="image batch"):
        b.next(1, 13, window)


# ---- train_nerf.main in images mode from the sampler --------------------------------------------------------------------------
def test_cli_images_mode_fused_and_resume(tmp_path, monkeypatch):
    """2 train views of 8 x 8, N_rand 12, six fused iterations across the end of the centre crop (precrop_iters 3), against three +
    --resume + three: parameters and Adam moments bit for bit, with no sampler state and no host generator in the loop."""
    from r2l_amd import train_nerf
    from r2l_amd.image_batch import crop_window, image_draw, window_ids
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("R2L_SEED", "7")
    root = str(tmp_path / "scene")
    os.makedirs(root)
    make_scene(root, size=16)  # (lego.txt: half_res)
    seeded = []
    monkeypatch.setattr(train_nerf, "_seed", lambda i, plain=train_nerf._seed: (seeded.append(i), plain(i))[1])
    seen, host = record_batches(monkeypatch)
    common = ["--config", os.path.join(ROOT, "configs", "lego.txt"), "--datadir", root, "--testskip", "1", "--N_samples", "8",
              "--N_importance", "8", "--i_print", "2", "--i_testset", "1000", "--i_weights", "3", "--save_intermediate_models",
              "--N_rand", "12", "--N_iters", "6", "--precrop_iters", "3", "--no_batching", "--r2l_image_sampler", "--r2l_fused_step"]
    a = train_nerf.main(common + ["--experiment_name", "A"])
    assert a["image_sampler"].images.is_cuda and a["batcher"] is None and host == [] and seeded == [0]
    assert len(a["history"]) == 6 and all(len(h) == 2 and np.isfinite(h).all() for h in a["history"])
    assert [i for i, _, _ in seen] == [1, 2, 3, 4, 5, 6]
    for i, img, ids in seen:
        want_img, key = image_draw(7, i, 2)
        assert img == want_img and np.array_equal(ids, window_ids(8, 8, img, crop_window(8, 8, .5) if i < 3 else (0, 0, 8, 8), key, 12)), i
        assert bool(in_crop(ids).all()) == (i < 3), i
    log = open(os.path.join(a["logger"].log_path, "log.txt")).read()
    assert "--r2l_image_sampler" in log and "Fused step" in log and "Center cropping of size 4 x 4 is enabled until iter 3" in log
    first = list(seen)
    del seen[:]
    mid = os.path.join(a["logger"].weights_path, "ckpt_3.tar")
    b = train_nerf.main(common + ["--experiment_name", "B", "--pretrained_ckpt", mid, "--resume"])
    assert len(b["history"]) == 3 and [i for i, _, _ in seen] == [4, 5, 6] and host == [] and seeded == [0, 0]
    for (i, img, ids), (j, img2, ids2) in zip(first[3:], seen):
        assert (i, img) == (j, img2) and np.array_equal(ids, ids2)
    for name in ("flat", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(a["trainer"], name).view(torch.int32), getattr(b["trainer"], name).view(torch.int32)), name
    assert a["history"][3:] == b["history"]


def test_cli_images_mode_on_llff(tmp_path, monkeypatch):
    """NDC rays: 9 views of 16 x 24, 7 of them for training, N_rand 256 of one frame's 384 pixels, the staged step."""
    from r2l_amd import image_batch, train_nerf
    from r2l_amd.image_batch import host_batch, image_draw
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("R2L_SEED", raising=False)
    root = str(tmp_path / "scene")
    make_llff_scene(root, H=32, W=48, factor=2, focal=60.)
    batches, plain = [], image_batch.ImageBatcher.next

    def next_(self, i, n, window=None):
        out = plain(self, i, n, window)
        batches.append((i, window, [t.clone() for t in out]))
        return out

    monkeypatch.setattr(image_batch.ImageBatcher, "next", next_)
    seen, host = record_batches(monkeypatch)
    a = train_nerf.main(["--config", os.path.join(LLFF_CONFIGS, "fern.txt"), "--datadir", root, "--factor", "2", "--no_batching",
                         "--r2l_image_sampler", "--N_iters", "3", "--N_rand", "256", "--i_print", "1", "--i_testset", "1000",
                         "--i_weights", "1000"])
    sm = a["image_sampler"]
    assert sm.ndc == 1 and sm.n_img == 7 and (sm.H, sm.W) == (16, 24) and host == [] and len(batches) == 3
    assert len(a["history"]) == 3 and all(np.isfinite(v) for h in a["history"] for v in h)
    for i, window, got in batches:
        assert window == (0, 0, 16, 24)
        img, key = image_draw(0, i, 7)
        want = host_batch(sm.images.cpu(), sm.poses.cpu(), 16, 24, sm.focal, 1, img, window, key, 256)
        assert all(torch.equal(g, w.cuda()) for g, w in zip(got, want[:4])), i
        assert not torch.equal(got[2], got[1] / got[1].norm(dim=-1, keepdim=True))  # rays_d are NDC, viewdirs the world's
    assert "--r2l_image_sampler" in open(os.path.join(a["logger"].log_path, "log.txt")).read()
