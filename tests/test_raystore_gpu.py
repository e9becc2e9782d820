"""Device-resident ray store on the GPU (include/r2l_hip.h r2l_store_append / r2l_store_batch, r2l_amd/raystore.py,
r2l_amd/online_kd.py, the driver's --r2l_device_store / --r2l_online_kd): bit for bit against the numpy restatement
(raystore.perm / shard_ids).  Rows are coded value = 16 * row + col — exact in fp32 at these sizes — so a misplaced float is
visible; every output buffer carries 8 guard floats of -7 at both ends, asserted untouched."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from oracle import r2l_oracle as O
from tests.test_driver_cpu import ROOT, make_scene
from tests.test_forward_gpu import build_model  # noqa: E402
from tests.test_raystore_cpu import SIZES

pytestmark = pytest.mark.gpu

G = 8  # guard floats at both ends
KEYS = [0, 0x9E3779B97F4A7C15, 2**64 - 1, 987654321987]


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from r2l_amd import _lib
    return _lib, _lib.load()


def guarded(n, fill, dtype=torch.float32):
    """(whole buffer, the n inner elements): 8 guards of -7 before and behind; the inner part is 16-byte aligned."""
    buf = torch.full((n + 2 * G,), -7, dtype=dtype, device="cuda")
    inner = buf[G:G + n]
    inner.fill_(fill)
    return buf, inner


def guards_ok(buf):
    return bool((buf[:G] == -7).all()) and bool((buf[-G:] == -7).all())


def coded(n_rows, first=0):
    """[n_rows, 9] fp32, value = 16 * row + col."""
    r = torch.arange(first, first + n_rows, dtype=torch.float32, device="cuda")[:, None] * 16.
    return (r + torch.arange(9, dtype=torch.float32, device="cuda")[None, :]).contiguous()


@pytest.mark.parametrize("n", SIZES)
def test_device_bijection_equals_the_restatement(n):
    from r2l_amd.raystore import perm
    L, lib = _lib()
    for key in KEYS:
        buf, out = guarded(n, -1, torch.int64)
        L.check(lib.r2l_pool_pick(_p(out), n, n, key, _st()), "r2l_pool_pick")
        assert np.array_equal(out.cpu().numpy(), perm(key, n)), (n, key)
        assert guards_ok(buf)


@pytest.mark.parametrize("n_rows,rps", [(4, 4), (5, 4), (7, 8), (4095, 4096), (4096, 4096), (4097, 4096), (3 * 4096 + 5, 4096),
                                        (5 * 4096 + 3, 4096)])
def test_store_append(n_rows, rps):
    from r2l_amd.raystore import perm
    L, lib = _lib()
    rows = coded(n_rows)
    m = n_rows // rps
    key = 0xC0FFEE1234 + n_rows
    want_perm = torch.from_numpy(perm(key, n_rows)[:m * rps]).cuda()
    for first in (0, 3):
        for shuffle in (1, 0):
            cap = first + m + 2
            buf, store = guarded(cap * rps * 9, -3.)
            n_written = ctypes.c_int64(-1)
            L.check(lib.r2l_store_append(_p(rows), n_rows, _p(store), cap, first, rps, key, shuffle, ctypes.byref(n_written), _st()),
                    "r2l_store_append")
            assert n_written.value == m
            sh = store.view(cap, rps, 9)
            want = rows[want_perm] if shuffle else rows[:m * rps]
            assert torch.equal(sh[first:first + m].reshape(-1, 9), want), (first, shuffle)
            assert bool((sh[:first] == -3.).all()) and bool((sh[first + m:] == -3.).all())  # (m == 0: the whole store)
            assert guards_ok(buf)
    if m:  # the shuffle moved something, and it is a different order per key
        assert not torch.equal(rows[want_perm], rows[:m * rps])


@pytest.mark.parametrize("rps", [4, 4096])
@pytest.mark.parametrize("n_shards", [1, 2, 7, 25])
def test_store_batch(n_shards, rps):
    from r2l_amd.raystore import shard_ids
    L, lib = _lib()
    store = coded(n_shards * rps)
    sh = store.view(n_shards, rps, 9)
    seed = 4242 + n_shards
    for n_draw in sorted({1, 2, 20, n_shards + 3}):
        for draw0 in (0, 5 * n_shards - 1):  # (the second one: the request crosses an epoch boundary when n_draw > 1)
            want_ids = shard_ids(seed, n_shards, draw0, n_draw)
            got = []
            for with_ids in (True, False):
                bbuf, batch = guarded(n_draw * rps * 9, -3.)
                ibuf, ids = guarded(n_draw, -1, torch.int32)
                L.check(lib.r2l_store_batch(_p(store), n_shards, rps, draw0, n_draw, seed, _p(batch), _p(ids) if with_ids else None,
                                            _st()), "r2l_store_batch")
                assert guards_ok(bbuf) and guards_ok(ibuf)
                if with_ids:
                    assert np.array_equal(ids.cpu().numpy(), want_ids), (n_draw, draw0)
                else:
                    assert bool((ids == -1).all())
                got.append(batch)
            want = sh[torch.from_numpy(want_ids).cuda()].reshape(-1, 9)
            assert torch.equal(got[0].view(-1, 9), want), (n_draw, draw0)
            assert torch.equal(got[0], got[1])  # ids_out = NULL: the same batch


def test_offsets_are_64_bit():
    """One append and one batch draw on shards whose float offset in the store is above 2^32: a 17.3 GB store of which only the
    touched shards (and the ones a truncated offset would hit) are initialised."""
    from r2l_amd.raystore import perm, shard_ids
    free = torch.cuda.mem_get_info()[0]
    if free < 24e9:
        print("test_offsets_are_64_bit SKIPPED: %.1f GB free, needs 24 GB" % (free / 1e9))
        pytest.skip("needs 24 GB of free device memory")
    L, lib = _lib()
    rps, cap, first = 4096, 117300, 117290
    shard_floats = rps * 9
    assert first * shard_floats > 2**32
    buf = torch.empty(cap * shard_floats + 2 * G, dtype=torch.float32, device="cuda")
    buf[:G] = -7.
    buf[-G:] = -7.
    store = buf[G:G + cap * shard_floats]
    sh = store.view(cap, rps, 9)
    alias = (first * shard_floats) % 2**32 // shard_floats  # where a 32-bit float offset would land
    for s in (first - 1, first + 2, alias - 1, alias, alias + 1, alias + 2, alias + 3):
        sh[s] = -3.
    n_rows, key = 2 * rps + 5, 0xABCDEF0123
    rows = coded(n_rows)
    n_written = ctypes.c_int64(-1)
    L.check(lib.r2l_store_append(_p(rows), n_rows, _p(store), cap, first, rps, key, 1, ctypes.byref(n_written), _st()), "r2l_store_append")
    assert n_written.value == 2
    want = rows[torch.from_numpy(perm(key, n_rows)[:2 * rps]).cuda()]
    assert torch.equal(sh[first:first + 2].reshape(-1, 9), want)
    for s in (first - 1, first + 2, alias - 1, alias, alias + 1, alias + 2, alias + 3):
        assert bool((sh[s] == -3.).all()), s
    # a draw that takes shard `first`: found in the restatement's first epoch
    seed = 99
    ids = shard_ids(seed, cap, 0, cap)
    t = int(np.nonzero(ids == first)[0][0])
    bbuf, batch = guarded(shard_floats, -3.)
    ibuf, got_id = guarded(1, -1, torch.int32)
    L.check(lib.r2l_store_batch(_p(store), cap, rps, t, 1, seed, _p(batch), _p(got_id), _st()), "r2l_store_batch")
    assert int(got_id.item()) == first
    assert torch.equal(batch.view(rps, 9), want[:rps])
    assert guards_ok(bbuf) and guards_ok(ibuf) and bool((buf[:G] == -7.).all()) and bool((buf[-G:] == -7.).all())
    print("test_offsets_are_64_bit RAN: store of %.2f GB, shard %d at float offset %d, draw %d" %
          (cap * shard_floats * 4 / 1e9, first, first * shard_floats, t))


def test_raystore_next_contract():
    from r2l_amd.raystore import RayStore, shard_ids
    n_shards, rps, seed = 7, 4096, 31
    rows = coded(n_shards * rps)
    stores = [RayStore(n_shards, "cuda", rays_per_shard=rps, seed=seed) for _ in range(2)]
    for s in stores:
        assert s.append(rows, key=0, shuffle=False) == n_shards and s.n_shards == n_shards == len(s.files)
        assert s.rows_per_file == rps and torch.equal(s.shards().reshape(-1, 9), rows)
    a, b = stores
    # the tensor of call k is unchanged after call k + 1
    b0 = a.next(3)
    ids0 = a.last_ids.clone()
    keep = b0.clone()
    b1 = a.next(3)
    assert b0.shape == (3 * rps, 9) and b0.data_ptr() != b1.data_ptr() and torch.equal(b0, keep)
    assert np.array_equal(ids0.cpu().numpy(), shard_ids(seed, n_shards, 0, 3))
    assert np.array_equal(a.last_ids.cpu().numpy(), shard_ids(seed, n_shards, 3, 3)) and a.draw == 6
    # 50 calls, each followed by a reduction of the batch on the current stream, no host sync in between
    a.seek(0)
    sums = torch.zeros(50, dtype=torch.float64, device="cuda")
    for k in range(50):
        sums[k] = a.next(3).double().sum()
    shard_sum = rows.view(n_shards, -1).double().sum(1).cpu().numpy()  # exact: integers far below 2^53
    want = np.array([shard_sum[shard_ids(seed, n_shards, 3 * k, 3)].sum() for k in range(50)])
    assert np.array_equal(sums.cpu().numpy(), want)
    # seek: next x 6 on one store, seek(9) + next x 3 on its twin: the last three batches agree
    a.seek(0)
    tail = [a.next(3).clone() for _ in range(6)][3:]
    b.seek(9)
    for k in range(3):
        assert torch.equal(b.next(3), tail[k]), k
    assert a.draw == b.draw == 18
    a.close()
    with pytest.raises(RuntimeError):
        a.next(3)
    # a store that does not fit is refused with both sizes in the message
    free = torch.cuda.mem_get_info()[0]
    too_many = int(free // (rps * 36)) + 1
    with pytest.raises(MemoryError) as e:
        RayStore(too_many, "cuda")
    assert "%.2f GB" % (too_many * rps * 36 / 1e9) in str(e.value) and "free" in str(e.value)


def _ray_rows(n, seed):
    rng = np.random.RandomState(seed)  # origins on the r = 4 sphere, inward directions, colours in [0, 1)
    o = rng.randn(n, 3).astype(np.float32)
    o *= 4. / np.linalg.norm(o, axis=1, keepdims=True)
    d = (-o / 4. + 0.2 * rng.randn(n, 3)).astype(np.float32)
    return np.concatenate([o, d, rng.rand(n, 3).astype(np.float32)], 1)


def test_training_from_the_store_is_training_from_the_files(tmp_path):
    from model.nerf_raybased import PointSampler
    from r2l_amd import data
    from r2l_amd.raystore import RayStore
    from r2l_amd.train_step import R2LTrainer
    kd = str(tmp_path)
    assert data.write_ray_shards(_ray_rows(5 * 4096 + 100, 5), kd, 0) == 5
    files = [os.path.join(kd, "data_%d.npy" % k) for k in (3, 0, 4, 1, 2)]  # list order, not name order
    on_disk = [np.load(f) for f in files]
    store = RayStore(5, "cuda", seed=3)
    info = store.append_files(files, threads=2)
    print(info["message"])
    assert store.n_shards == 5 and store.files == files and info["files"] == 5
    assert np.array_equal(store.shards().cpu().numpy(), np.stack(on_disk))
    sd = O.make_state_dict(n_block=2, seed=3)
    ps = PointSampler(400, 400, 555.5555155968841, 16, 2., 6.)
    flats, ids = [], []
    for source in ("store", "files"):
        tr = R2LTrainer(build_model(sd, 2), ps)
        init = tr.eng.flat.clone()
        for k in range(3):
            if source == "store":
                batch = store.next(2)
                ids.append(store.last_ids.cpu().numpy())
            else:
                batch = torch.from_numpy(np.concatenate([on_disk[i] for i in ids[k]], 0)).cuda()
            tr.step(batch[:, :3], batch[:, 3:6], batch[:, 6:9], 5e-4, perturb=0.)
        assert np.isfinite(tr.loss_out[0].item())
        flats.append(tr.eng.flat.clone())
    assert not torch.equal(flats[0], init)  # it did train
    assert torch.equal(flats[0], flats[1])  # bit-identical parameters


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, *a):
        self.lines.append(" ".join(str(x) for x in a))


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    """The tiny scene and teacher checkpoint of test_cli_fused_frames: half_res 64 x 64 = one shard per pose."""
    root = tmp_path_factory.mktemp("raystore")
    scene = str(root / "scene")
    os.makedirs(scene)
    make_scene(scene, size=128)
    csd, fsd = O.make_teacher_state_dicts(5, 2, alpha_bias=0.5)
    ck = str(root / "teacher.tar")
    torch.save({"global_step": 200000, "network_fn_state_dict": csd, "network_fine_state_dict": fsd}, ck)
    from r2l_amd import data
    focal = float(data.load_blender_data(scene, True, 1)[3][2])
    return {"scene": scene, "ck": ck, "focal": focal, "teacher_cfg": os.path.join(ROOT, "configs", "lego.txt")}


def sorted_rows(rows):
    """Rows in lexicographic order of their bit patterns: int32 [n, 9]."""
    a = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, 9).view(np.int32)
    return a[np.lexsort(a.T[::-1])]


def test_teacher_fill_equals_create_data(tiny, tmp_path, monkeypatch):
    from r2l_amd import create_data, data, options
    from r2l_amd.online_kd import fill_store_from_teacher
    from r2l_amd.raystore import RayStore
    from r2l_amd.render import render_frames
    monkeypatch.chdir(tmp_path)
    common = ["--create_data", "rand", "--config", tiny["teacher_cfg"], "--datadir", tiny["scene"], "--teacher_ckpt", tiny["ck"],
              "--n_pose_kd", "3", "--create_data_chunk", "2", "--perturb", "0"]
    kd = str(tmp_path / "pseudo")
    out = create_data.main(common + ["--datadir_kd", tiny["scene"] + ":" + kd, "--experiment_name", "cd", "--r2l_fused_frames"])
    assert out["n_rays"] == 3 * 4096 and sorted(os.listdir(kd)) == ["data_0.npy", "data_1.npy", "data_2.npy"]
    written = np.concatenate([np.load(os.path.join(kd, f)) for f in sorted(os.listdir(kd))], 0)
    targs = options.parse_args(common)
    log = _Log()
    store = RayStore(3, "cuda")
    # a group at a time: the state is kept between the calls and says what is pending
    state = fill_store_from_teacher(store, targs, 64, 64, tiny["focal"], 2., 6., 3, 2, 0, 1, "cuda", logger=log, groups=1)
    assert (state.pending, state.done, store.n_shards) == (1, False, 2) and state.coarse is not None
    again = fill_store_from_teacher(store, targs, 64, 64, tiny["focal"], 2., 6., 3, 2, 0, 1, "cuda", state=state, groups=1)
    assert again is state and (state.pending, state.done, store.n_shards) == (0, True, 3)
    assert state.coarse is None and state.fine is None and any("released" in l for l in log.lines), log.lines
    got = store.shards().cpu().numpy()
    assert np.array_equal(sorted_rows(got), sorted_rows(written))  # the same rows bit for bit, in another order
    assert not np.array_equal(got.reshape(-1, 9), written)
    # rank 1 of 2, four poses: poses 1 and 3 of that rank's stream, rendered with those frame ids, and nothing else
    store = RayStore(2, "cuda")
    state = fill_store_from_teacher(store, targs, 64, 64, tiny["focal"], 2., 6., 4, 2, 1, 2, "cuda")
    assert state.done and state.mine == [1, 3] and store.n_shards == 2
    rng = np.random.RandomState(1000003)
    coarse, fine = create_data.create_teacher(targs, torch.device("cuda"))
    want = []
    for i in (1, 3):
        pose = data.get_rand_pose(rng)
        f = tiny["focal"] * (1 + rng.rand())
        with torch.no_grad():
            want.append(render_frames(pose[None, :3, :4].cuda(), 64, 64, f, 2., 6., coarse, fine, targs.N_samples, targs.N_importance,
                                      0., targs.white_bkgd, seed=1000003, frame_id0=i, rows=True)["rows"].cpu().numpy())
    assert np.array_equal(sorted_rows(store.shards().cpu().numpy()), sorted_rows(np.concatenate(want, 0)))


def _student(tiny, name):
    return ["--model_name", "R2L", "--config", os.path.join(ROOT, "configs", "lego_noview.txt"), "--datadir", tiny["scene"],
            "--n_sample_per_ray", "16", "--netwidth", "256", "--netdepth", "6", "--use_residual", "--trial.ON", "--trial.body_arch",
            "resmlp", "--testskip", "1", "--N_rand", "2", "--hard_ratio", "0.2", "--hard_mul", "2", "--warmup_lr", "0.0001,200",
            "--i_print", "1", "--experiment_name", name]


def _log_of(res):
    return open(os.path.join(res["logger"].log_path, "log.txt")).read()


def _losses(log):
    return [float(l.split(" loss ")[1].split()[0]) for l in log.splitlines() if "[TRAIN] Iter" in l]


def test_cli_online_kd(tiny, tmp_path, monkeypatch):
    from r2l_amd import driver, options
    from r2l_amd.online_kd import fill_store_from_teacher
    from r2l_amd.raystore import RayStore
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(RayStore, "close", lambda self: None)  # the test reads the store after the run
    online = ["--r2l_online_kd", "--r2l_teacher_config", tiny["teacher_cfg"], "--teacher_ckpt", tiny["ck"], "--n_pose_kd", "3",
              "--N_iters", "4"]
    targs = options.parse_teacher_config(tiny["teacher_cfg"], teacher_ckpt=tiny["ck"])

    def filled_first(chunk):
        s = RayStore(3, "cuda")
        fill_store_from_teacher(s, targs, 64, 64, tiny["focal"], 2., 6., 3, chunk, 0, 1, "cuda")
        return sorted_rows(s.shards().cpu().numpy())

    res = driver.main(_student(tiny, "online") + online + ["--create_data_chunk", "2"])
    log = _log_of(res)
    losses = _losses(log)
    assert len(losses) == 4 and np.all(np.isfinite(losses)) and np.isfinite(res["trainer"].loss_out[0].item())
    assert "ray store: 3 / 3 shards of 4096 rays" in log and "released" in log
    assert res["loader"].n_shards == 3 and res["loader"].draw == 8
    assert np.array_equal(sorted_rows(res["loader"].shards().cpu().numpy()), filled_first(2))
    # data arriving during training: the first flush group before iteration 1, one more every 2 iterations
    res = driver.main(_student(tiny, "every") + online + ["--create_data_chunk", "1", "--r2l_kd_every", "2"])
    log = _log_of(res)
    assert "ray store: 1 / 3 shards of 4096 rays" in log
    grew = [l.split("Iter ")[1] for l in log.splitlines() if "ray store grew to" in l]
    assert [g.split(" (")[0] for g in grew] == ["2 ray store grew to 2 shards", "4 ray store grew to 3 shards"], grew
    losses = _losses(log)
    assert len(losses) == 4 and np.all(np.isfinite(losses))
    assert np.array_equal(sorted_rows(res["loader"].shards().cpu().numpy()), filled_first(1))
    assert glob.glob(os.path.join(str(tmp_path), "**", "*.npy"), recursive=True) == []  # no shard file anywhere
    # what is missing is named before anything is loaded
    with pytest.raises(ValueError, match="--teacher_ckpt"):
        driver.main(_student(tiny, "bad") + ["--r2l_online_kd", "--r2l_teacher_config", tiny["teacher_cfg"]])


def test_cli_device_store_and_resume(tiny, tmp_path, monkeypatch):
    from r2l_amd import data, driver
    monkeypatch.chdir(tmp_path)
    kd = str(tmp_path / "pseudo")
    os.makedirs(kd)
    data.write_ray_shards(_ray_rows(5 * 4096, 9), kd, 0)
    common = _student(tiny, "store") + ["--datadir_kd", kd, "--data_mode", "rays", "--r2l_device_store", "--i_weights", "4"]
    res = driver.main(common + ["--N_iters", "4"])
    log = _log_of(res)
    losses = _losses(log)
    assert len(losses) == 4 and np.all(np.isfinite(losses))
    assert "ray store: read 5 files" in log and "ray store: 5 / 5 shards of 4096 rays" in log and "resuming at draw" not in log
    assert res["loader"].draw == 8
    ck = os.path.join(res["logger"].weights_path, "ckpt.tar")
    res = driver.main(common + ["--N_iters", "6", "--pretrained_ckpt", ck, "--resume", "--experiment_name", "resumed"])
    log = _log_of(res)
    line = [l for l in log.splitlines() if "ray store: resuming at draw" in l]
    assert len(line) == 1 and int(line[0].split("resuming at draw ")[1].split()[0]) == 4 * 2, line  # start iteration x N_rand
    assert [l.split("[TRAIN] Iter ")[1].split()[0] for l in log.splitlines() if "[TRAIN] Iter" in l] == ["5", "6"]
    assert res["loader"].draw == 12
