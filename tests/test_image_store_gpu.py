"""Image-filled ray store on the GPU (include/r2l_hip.h r2l_store_append_images; RayStore.append_images; r2l_amd/image_store.py;
main.py --r2l_image_store): the one launch against the three it replaces — r2l_frame_rays(rows), the rgb copy into columns 6..8,
r2l_store_append — and against the numpy restatement, its argument contract, the batches drawn from such a store, and the CLI:
README step 5 from images in device memory, alone and behind a teacher fill.  Every comparison is torch.equal / np.array_equal:
there is no tolerance anywhere."""
import ctypes
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_driver_cpu import ROOT
from tests.test_pool_select_gpu import _ckpt_equal
from tests.test_raystore_gpu import G, _log_of, _ray_rows, _student, guarded, guards_ok, tiny  # noqa: F401  (tiny: scene and teacher)

pytestmark = pytest.mark.gpu

INVALID = 1  # hipErrorInvalidValue
SENTINEL = -3.


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from r2l_amd import _lib
    return _lib, _lib.load()


def _group(K, H, W, seed=11):
    """(images [K,H,W,3], c2ws [K,3,4], focals [K]) on the device: random poses, focals in [6, 9), colours in [0, 1)."""
    rng = np.random.RandomState(seed + 100 * K + H)
    c2w = torch.from_numpy(rng.randn(K, 3, 4).astype(np.float32)).cuda()
    focal = torch.from_numpy((6. + 3. * rng.rand(K)).astype(np.float32)).cuda()
    images = torch.from_numpy(rng.rand(K, H, W, 3).astype(np.float32)).cuda()
    return images, c2w, focal


def _old_route(images, c2w, fdev, f, store, cap, first, rps, key, shuffle):
    """r2l_frame_rays(rows) -> rgb into columns 6..8 -> r2l_store_append: the three launches and the [n_rows, 9] intermediate."""
    L, lib = _lib()
    K, H, W = images.shape[:3]
    rows = torch.full((K * H * W, 9), 7., dtype=torch.float32, device="cuda")
    L.check(lib.r2l_frame_rays(_p(c2w), _p(fdev), f, K, H, W, None, None, None, _p(rows), _st()), "r2l_frame_rays")
    rows[:, 6:9] = images.reshape(-1, 3)
    m = ctypes.c_int64(-1)
    L.check(lib.r2l_store_append(_p(rows), K * H * W, _p(store), cap, first, rps, key, shuffle, ctypes.byref(m), _st()), "r2l_store_append")
    return m.value


@pytest.mark.parametrize("first", [0, 2])
@pytest.mark.parametrize("rps", [4, 8, 64])
@pytest.mark.parametrize("H,W", [(5, 7), (8, 8)])
@pytest.mark.parametrize("K", [1, 3])
def test_kernel_equals_the_route_it_replaces(K, H, W, rps, first):
    """n_rows = 35, 64, 105, 192: multiples of the shard and not, powers of four (no cycle walking) and not; fewer rows than a shard
    (35 at 64) write nothing."""
    from r2l_amd.raystore import append_images_spec
    L, lib = _lib()
    images, c2w, focal = _group(K, H, W)
    n_rows, m = K * H * W, K * H * W // rps
    cap = first + m + 2
    key = 0xC0FFEE1234 + n_rows
    for shuffle in (1, 0):
        for fdev, f in ((focal, 0.), (None, 7.25)):
            buf, store = guarded(cap * rps * 9, SENTINEL)
            n_written = ctypes.c_int64(-1)
            L.check(lib.r2l_store_append_images(_p(images), _p(c2w), _p(fdev), f, K, H, W, _p(store), cap, first, rps, key, shuffle,
                                                ctypes.byref(n_written), _st()), "r2l_store_append_images")
            assert n_written.value == m
            wbuf, want = guarded(cap * rps * 9, SENTINEL)
            assert _old_route(images, c2w, fdev, f, want, cap, first, rps, key, shuffle) == m
            what = (shuffle, fdev is None)
            assert torch.equal(store, want), what  # the written shards AND the sentinels before and behind them
            sh = store.view(cap, rps, 9)
            assert bool((sh[:first] == SENTINEL).all()) and bool((sh[first + m:] == SENTINEL).all()), what
            assert guards_ok(buf) and guards_ok(wbuf), what
            spec = append_images_spec(images.cpu().numpy(), c2w.cpu().numpy(), focal.cpu().numpy() if fdev is not None else f, rps, key,
                                      bool(shuffle))
            got = sh[first:first + m].reshape(-1, 9).cpu().numpy()
            assert np.array_equal(got.view(np.uint32), spec.view(np.uint32)), what  # o, d and rgb bit for bit
    if m:
        assert not torch.equal(store, guarded(cap * rps * 9, SENTINEL)[1])  # something was written


def test_argument_contract():
    """Every refusal is hipErrorInvalidValue with the argument's name in r2l_last_error and enqueues nothing: the store keeps its
    sentinel and n_written its value.  m == 0 is a successful no-op."""
    L, lib = _lib()
    K, H, W, rps, cap = 2, 2, 4, 4, 6  # 16 rows: m = 4
    images, c2w, focal = _group(K, H, W)
    buf, store = guarded(cap * rps * 9, SENTINEL)
    inside = store[36:36 + K * H * W * 3]  # "images" that lie in the store
    m = ctypes.c_int64(-5)
    mp = ctypes.cast(ctypes.byref(m), ctypes.c_void_p)

    def call(im=images, pose=c2w, fdev=focal, f=0., K=K, H=H, W=W, st=store, cap=cap, first=0, rps=rps, n_written=mp):
        return lib.r2l_store_append_images(_p(im), _p(pose), _p(fdev), f, K, H, W, _p(st), cap, first, rps, 9, 1, n_written, _st())

    for kw, word in ((dict(im=None), b"NULL"), (dict(pose=None), b"NULL"), (dict(st=None), b"NULL"), (dict(n_written=None), b"NULL"),
                     (dict(K=0), b"K"), (dict(K=-1), b"K"), (dict(H=0), b"H"), (dict(H=-2), b"H"), (dict(W=0), b"W"),
                     (dict(fdev=None, f=0.), b"focal"), (dict(fdev=None, f=-3.), b"focal"), (dict(fdev=None, f=float("nan")), b"focal"),
                     (dict(rps=0), b"rays_per_shard"), (dict(rps=-8), b"rays_per_shard"), (dict(rps=6), b"rays_per_shard"),
                     (dict(first=3), b"capacity_shards"), (dict(cap=3), b"capacity_shards"), (dict(first=-1), b"first_shard"),
                     (dict(cap=-1), b"capacity_shards"), (dict(st=store[1:]), b"aligned"), (dict(im=inside), b"overlap")):
        assert call(**kw) == INVALID, kw
        msg = lib.r2l_last_error()
        assert b"r2l_store_append_images" in msg and word in msg, (kw, msg)
    assert call(rps=32) == 0 and m.value == 0  # 16 rows at 32 a shard: nothing to write, nothing enqueued
    m.value = -5
    torch.cuda.synchronize()
    assert bool((store == SENTINEL).all()) and guards_ok(buf) and m.value == -5
    assert call() == 0 and m.value == 4  # and the arguments the refusals varied are good ones
    torch.cuda.synchronize()
    assert bool((store.view(cap, rps, 9)[:4] != SENTINEL).all()) and bool((store.view(cap, rps, 9)[4:] == SENTINEL).all())


def test_batches_from_an_image_filled_store():
    """RayStore.append_images (device images: the kernel; CPU images: the restatement, uploaded) against RayStore.append of the old
    route's rows, behind a first group: the stores, what next() hands out and what r2l_train_batch hands out are equal."""
    from r2l_amd.raystore import RayStore
    L, lib = _lib()
    K, H, W, rps, key = 3, 8, 8, 8, 0xABCDEF
    images, c2w, focal = _group(K, H, W)
    first_group = torch.from_numpy(_ray_rows(5 * rps + 3, 4)).cuda()
    rows = torch.empty(K * H * W, 9, dtype=torch.float32, device="cuda")
    L.check(lib.r2l_frame_rays(_p(c2w), _p(focal), 0., K, H, W, None, None, None, _p(rows), _st()), "r2l_frame_rays")
    rows[:, 6:9] = images.reshape(-1, 3)
    stores = []
    for how in ("rows", "device images", "cpu images"):
        s = RayStore(5 + 24, "cuda", rays_per_shard=rps, seed=77)
        assert s.append(first_group, 5, shuffle=True) == 5
        if how == "rows":
            assert s.append(rows, key, shuffle=True) == 24
        else:
            im = images if how == "device images" else images.cpu()
            assert s.append_images(im, c2w, focal, key, shuffle=True) == 24
        assert s.n_shards == 29 and len(s.files) == 29
        stores.append(s)
    old = stores[0]
    for s in stores[1:]:
        assert torch.equal(s.shards(), old.shards())
    new = stores[1]
    for n in (3, 29, 4):  # (the second request crosses an epoch boundary)
        a, b = old.next(n), new.next(n)
        assert torch.equal(a, b) and torch.equal(old.last_ids, new.last_ids) and old.draw == new.draw
    outs = []
    for s in (old, new):
        pl = s.plan(6)
        o, d, t = (torch.empty(6 * rps, 3, dtype=torch.float32, device="cuda") for _ in range(3))
        ids = torch.empty(6, dtype=torch.int32, device="cuda")
        L.check(lib.r2l_train_batch(pl["ptr"], pl["n_shards"], pl["rays_per_shard"], pl["draw0"], pl["n_draw"], pl["seed"], None, 0, 0, 0,
                                    _p(o), _p(d), _p(t), _p(ids), None, _st()), "r2l_train_batch")
        outs.append((o, d, t, ids))
    assert all(torch.equal(x, y) for x, y in zip(*outs))
    # one focal for all frames, 4 x 4 poses, and the refusals of the method
    s = RayStore(24, "cuda", rays_per_shard=rps)
    pose4 = torch.cat([c2w, torch.tensor([0., 0., 0., 1.], device="cuda").expand(K, 1, 4)], 1)
    assert s.append_images(images, pose4, 7.5, key, shuffle=False) == 24
    L.check(lib.r2l_frame_rays(_p(c2w), None, 7.5, K, H, W, None, None, None, _p(rows), _st()), "r2l_frame_rays")
    assert torch.equal(s.shards().reshape(-1, 9)[:, :6], rows[:, :6]) and torch.equal(s.shards().reshape(-1, 9)[:, 6:], images.reshape(-1, 3))
    for bad, word in (((images[:2], c2w, focal), "images"), ((images.double(), c2w, focal), "images"), ((images, c2w[0], focal), "c2ws"),
                      ((images, c2w, focal[:2]), "focals"), ((images, c2w, 0.), "focal"), ((images, c2w, focal), "do not fit")):
        with pytest.raises(ValueError, match=word):
            s.append_images(*bad, key)
    assert s.n_shards == 24


def test_ranks_keep_disjoint_shards_of_one_sequence():
    """fill_store_from_images at world size 3: every rank builds the sequence of world size 1 and keeps shards rank, rank + 3, ...
    of it (13 shards: 5 + 4 + 4), behind whatever its store held; CPU images are moved to the device."""
    from r2l_amd.image_store import fill_store_from_images, image_group_key, image_shards
    from r2l_amd.raystore import RayStore, append_images_spec
    K, H, W, rps = 3, 5, 7, 8
    images, c2w, focal = _group(K, H, W)
    whole = RayStore(13, "cuda", rays_per_shard=rps)
    assert fill_store_from_images(whole, images.cpu(), c2w.cpu(), 7.5, seed=5) == 13
    spec = append_images_spec(images.cpu().numpy(), c2w.cpu().numpy(), 7.5, rps, image_group_key(5))
    assert np.array_equal(whole.shards().reshape(-1, 9).cpu().numpy().view(np.uint32), spec.view(np.uint32))
    other = RayStore(13, "cuda", rays_per_shard=rps)
    fill_store_from_images(other, images, c2w, 7.5, seed=6)
    assert not torch.equal(other.shards(), whole.shards())  # the seed is the order
    ahead = torch.from_numpy(_ray_rows(2 * rps, 4)).cuda()
    for rank in range(3):
        assert image_shards(K, H, W, rank, 3, rps) == (13, [5, 4, 4][rank])
        s = RayStore(2 + 5, "cuda", rays_per_shard=rps)
        s.append(ahead, 1, shuffle=False)
        assert fill_store_from_images(s, images, c2w, 7.5, rank=rank, world=3, seed=5) == [5, 4, 4][rank]
        assert torch.equal(s.shards()[:2].reshape(-1, 9), ahead) and torch.equal(s.shards()[2:], whole.shards()[rank::3])
    with pytest.raises(ValueError, match="do not fit"):
        fill_store_from_images(RayStore(4, "cuda", rays_per_shard=rps), images, c2w, 7.5, rank=0, world=3)


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------
def _main(work, argv):
    """driver.main in the directory `work`: (absolute weights path, log text)."""
    from r2l_amd import driver
    cwd = os.getcwd()
    os.chdir(str(work))
    try:
        res = driver.main(argv)
        return os.path.join(str(work), res["logger"].weights_path), _log_of(res)
    finally:
        os.chdir(cwd)


def _equal_ckpts(a, b, names):
    from r2l_amd.checkpoint import load_ckpt
    for name in names:
        x, y = load_ckpt(os.path.join(a, name)), load_ckpt(os.path.join(b, name))
        assert _ckpt_equal(x, y) == (True, True), name
        assert x["global_step"] == y["global_step"]


def _iters(log):
    return [l.split("[TRAIN] Iter ")[1].split()[0] for l in log.splitlines() if "[TRAIN] Iter" in l]


def test_cli_finetune_from_images_in_device_memory(tiny, tmp_path, monkeypatch):  # noqa: F811
    """README step 5 without step 4: three iterations on pseudo shards, then --resume with --r2l_image_store alone — no
    --datadir_kd — for three more, staged and as one library call per iteration; a resume from the middle checkpoint repeats
    the uninterrupted run.  The scene's two 64 x 64 training frames are two shards: every step draws both."""
    from r2l_amd import data
    from r2l_amd.raystore import RayStore
    kd = str(tmp_path / "pseudo")
    os.makedirs(kd)
    data.write_ray_shards(_ray_rows(5 * 4096, 9), kd, 0)
    pool = ["--r2l_device_pool", "--save_intermediate_models"]
    w0, log = _main(tmp_path, _student(tiny, "pseudo") + pool + ["--datadir_kd", kd, "--data_mode", "rays", "--r2l_device_store",
                                                                "--i_weights", "3", "--N_iters", "3"])
    assert _iters(log) == ["1", "2", "3"] and "ray store: read 5 files" in log
    ck3 = os.path.join(w0, "ckpt_3.tar")

    def no_files(self, *a, **kw):
        raise AssertionError("a shard file was asked for")
    monkeypatch.setattr(RayStore, "append_files", no_files)
    monkeypatch.setattr(data, "list_ray_shards", no_files)
    real = ["--r2l_image_store", "--i_weights", "1", "--N_iters", "6", "--pretrained_ckpt", ck3, "--resume"]
    names = ("ckpt_4.tar", "ckpt_5.tar", "ckpt_6.tar")
    wa, log = _main(tmp_path, _student(tiny, "real") + pool + real)
    assert _iters(log) == ["4", "5", "6"] and sorted(os.listdir(wa)) == list(names)
    assert "image store (--r2l_image_store): the 2 training frames of --datadir at 64 x 64 = 8192 real rays -> 2 shards of 4096 rays" in log
    assert "ray store: 2 / 2 shards of 4096 rays" in log and "resuming at draw 6" in log
    assert "no shard file was opened" in log and "ray store: read" not in log and "Loaded data. Now total #train files: 2" in log
    losses = [float(l.split(" loss ")[1].split()[0]) for l in log.splitlines() if "[TRAIN] Iter" in l]
    assert np.all(np.isfinite(losses))
    wb, log = _main(tmp_path, _student(tiny, "real_fused") + pool + real + ["--r2l_fused_iter"])
    assert _iters(log) == ["4", "5", "6"] and "Fused iteration (--r2l_fused_iter)" in log and "ray store: read" not in log
    _equal_ckpts(wa, wb, names)
    wc, log = _main(tmp_path, _student(tiny, "real_resumed") + pool +
                    ["--r2l_image_store", "--i_weights", "1", "--N_iters", "6", "--pretrained_ckpt", os.path.join(wa, "ckpt_5.tar"), "--resume"])
    assert _iters(log) == ["6"] and "resuming at draw 10" in log
    _equal_ckpts(wa, wc, ("ckpt_6.tar",))
    from r2l_amd.checkpoint import load_ckpt
    assert _ckpt_equal(load_ckpt(ck3), load_ckpt(os.path.join(wa, "ckpt_6.tar")))[0] is False  # it did train
    assert glob.glob(os.path.join(str(tmp_path), "Experiments", "**", "*.npy"), recursive=True) == []
    # fewer shards than one step draws: named before anything is allocated
    with pytest.raises(ValueError, match="--r2l_image_store.*2 shards.*draws 3"):
        _main(tmp_path, _student(tiny, "few") + ["--r2l_image_store", "--N_rand", "3"])


def test_cli_real_rows_behind_the_teachers(tiny, tmp_path, monkeypatch):  # noqa: F811
    """--r2l_online_kd --r2l_image_store: three teacher shards (three poses in flush groups of two and one) and the two real
    ones in one store; the saved file, loaded as any plain file, reproduces the run."""
    from r2l_amd import raystore as R
    from r2l_amd.image_store import image_group_key
    run = ["--r2l_device_pool", "--i_weights", "3", "--save_intermediate_models", "--N_iters", "6"]
    online = ["--r2l_online_kd", "--r2l_teacher_config", tiny["teacher_cfg"], "--teacher_ckpt", tiny["ck"], "--n_pose_kd", "3",
              "--create_data_chunk", "2"]
    F = str(tmp_path / "mixed.r2l")
    wa, log = _main(tmp_path, _student(tiny, "mixed") + online + run + ["--r2l_image_store", "--r2l_store_save", F])
    assert "ray store: 3 teacher shards + 2 real shards = 5: real share 0.4000 of every epoch" in log and "--pseudo_ratio is not consulted" in log
    assert "ray store: 5 / 5 shards of 4096 rays" in log and "ray store: saved 5 shards to %s" % F in log
    assert log.index("ray store: saved") < log.index("Begin training") and _iters(log) == [str(i) for i in range(1, 7)]
    h = R.read_store_header(F)
    assert (h["kind"], h["n_shards"], h["rays_per_shard"]) == (0, 5, 4096)
    assert (h["provenance"]["real_frames"], h["provenance"]["real_shards"], h["provenance"]["n_pose"]) == (2, 2, 3)
    # the last two shards are the real group: the rows the method writes for the loader's training split
    from r2l_amd import data, image_store, options
    a = options.parse_args(_student(tiny, "x"))
    sc = data.load_scene(a)
    images, c2ws = image_store.training_frames(sc, a.white_bkgd)
    want = R.append_images_spec(images.numpy(), c2ws.numpy(), float(sc.hwf[2]), 4096, image_group_key())
    store = R.RayStore.load(F, "cuda")
    assert np.array_equal(store.shards()[3:].reshape(-1, 9).cpu().numpy().view(np.uint32), want.view(np.uint32))
    store.close()
    wb, log = _main(tmp_path, _student(tiny, "mixed_loaded") + run + ["--r2l_store_load", F])
    assert "ray store: loaded 5 shards from %s" % F in log and "teacher rendered" not in log and "image store" not in log
    _equal_ckpts(wa, wb, ("ckpt_3.tar", "ckpt_6.tar"))
    # a refusal of the pair at start-up names both flags
    with pytest.raises(ValueError, match="--r2l_image_store.*--r2l_kd_every"):
        _main(tmp_path, _student(tiny, "bad") + online + ["--r2l_image_store", "--r2l_kd_every", "2"])


def test_cli_two_ranks(tiny, tmp_path):  # noqa: F811
    """Two ranks on this one GPU over gloo: each keeps one of the two real shards and draws it every step; the replicas end in
    sync (the run checks them itself)."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("R2L_")}
    env.update(MASTER_ADDR="127.0.0.1", R2L_DIST_BACKEND="gloo", R2L_CHECK_SYNC="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29671", os.path.join(ROOT, "main.py")] + _student(tiny, "dp2") + ["--r2l_image_store", "--i_weights", "2",
                                                                                                "--N_iters", "2"]
    r = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "-> 2 shards of 4096 rays in device memory" in out and "rank 0 of 2 keeps 1" in out
    assert "ray store: 1 / 1 shards of 4096 rays" in out and "no shard file was opened" in out
    assert "replicas in sync after 2 iterations: True (skipped steps: 0)" in out
