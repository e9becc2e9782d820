"""Compact ray store on the GPU (include/r2l_hip.h r2l_cstore_append / r2l_cstore_batch; raystore.CompactRayStore;
--r2l_compact_store): the batches it hands out are the plain store's BIT FOR BIT — every comparison here is torch.equal /
np.array_equal, there is no tolerance — and equal the numpy restatement (raystore.cstore_append_spec / cstore_batch_spec)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.test_pool_select_gpu import _ckpt_equal
from tests.test_raystore_gpu import _Log, _log_of, _student, guarded, guards_ok, tiny  # noqa: F401  (tiny: scene and teacher)

pytestmark = pytest.mark.gpu

SEED = 4242


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _pose(rng):
    """A camera on the r = 4 sphere looking at the origin, as a [3, 4] fp32 c2w."""
    eye = rng.randn(3)
    eye *= 4. / np.linalg.norm(eye)
    z = eye / np.linalg.norm(eye)
    x = np.cross([0., 0., 1.], z)
    x /= np.linalg.norm(x)
    return np.concatenate([np.stack([x, np.cross(z, x), z], 1), eye[:, None]], 1).astype(np.float32)


def _group(K, H, W, focal, seed):
    """One flush group as the teacher leaves it: (rows [K*H*W, 9] with o, d from r2l_frame_rays and random rgb, c2ws [K, 3, 4],
    focals).  focal: K values (they go to the device: focal_dev) or one number (NULL focal_dev)."""
    from r2l_amd import _lib
    rng = np.random.RandomState(seed)
    c2ws = torch.from_numpy(np.stack([_pose(rng) for _ in range(K)])).cuda()
    fdev = None if isinstance(focal, float) else torch.tensor(focal, dtype=torch.float32, device="cuda")
    rows = torch.full((K * H * W, 9), -3., dtype=torch.float32, device="cuda")
    _lib.check(_lib.load().r2l_frame_rays(_p(c2ws), _p(fdev), focal if fdev is None else 0., K, H, W, None, None, None, _p(rows),
                                          _st()), "r2l_frame_rays")
    rows[:, 6:9] = torch.from_numpy(rng.rand(K * H * W, 3).astype(np.float32)).cuda()
    return rows, c2ws, (focal if fdev is None else fdev)


class Pair:
    """A RayStore and a CompactRayStore that are appended to and drawn from together, and the numpy picture of the compact one."""

    def __init__(self, cap_shards, cap_poses, H, W, rps, shuffle):
        from r2l_amd.raystore import CompactRayStore, RayStore
        self.H, self.W, self.rps, self.shuffle = H, W, rps, shuffle
        self.plain = RayStore(cap_shards, "cuda", rays_per_shard=rps, seed=SEED)
        self.compact = CompactRayStore(cap_shards, cap_poses, H, W, "cuda", rays_per_shard=rps, seed=SEED)
        self.rgb, self.ids, self.c2w, self.focal, self.pose0 = [], [], [], [], []

    def append(self, group, key):
        from r2l_amd.raystore import cstore_append_spec
        rows, c2ws, focals = group
        K = c2ws.shape[0]
        first_pose = self.compact.n_poses
        m = self.plain.append(rows, key, shuffle=self.shuffle)
        # (the strided [:, 6:9] view of the 36-byte rows: rgb_stride 9)
        assert self.compact.append_frames(rows[:, 6:9], c2ws, focals, key, shuffle=self.shuffle) == m
        assert self.compact.n_shards == self.plain.n_shards == len(self.compact.files) and self.compact.n_poses == first_pose + K
        rgb, ids = cstore_append_spec(rows[:, 6:9].cpu().numpy(), self.rps, key, shuffle=self.shuffle)
        assert ids.shape[0] == m * self.rps
        self.rgb.append(rgb)
        self.ids.append(ids)
        self.c2w.append(c2ws.cpu().numpy())
        self.focal.append(np.full(K, focals, np.float32) if isinstance(focals, float) else focals.cpu().numpy())
        self.pose0 += [first_pose] * m
        # the device store holds what the restatement says: rows { rgb, id }, the pose table, the shards' pose index
        n = self.compact.n_shards * self.rps
        dev = self.compact.data[:n].cpu().numpy()
        assert np.array_equal(dev[:, :3], np.concatenate(self.rgb)) and np.array_equal(dev[:, 3].view(np.uint32), np.concatenate(self.ids))
        assert np.array_equal(self.compact.pose_c2w[:self.compact.n_poses].cpu().numpy(), np.concatenate(self.c2w))
        assert np.array_equal(self.compact.pose_focal[:self.compact.n_poses].cpu().numpy(), np.concatenate(self.focal))
        assert np.array_equal(self.compact.shard_pose0[:self.compact.n_shards].cpu().numpy(), np.array(self.pose0, np.int32))
        return m

    def draw(self, n_calls, n=5):
        """n_calls x next(n) from both stores: equal batches and ids every time, equal to the restatement."""
        from r2l_amd.raystore import cstore_batch_spec
        n_shards, draw0 = self.compact.n_shards, self.compact.draw
        assert self.plain.draw == draw0
        want, want_ids = cstore_batch_spec(np.concatenate(self.rgb), np.concatenate(self.ids), np.concatenate(self.c2w),
                                           np.concatenate(self.focal), np.array(self.pose0, np.int32), self.H, self.W, n_shards, self.rps,
                                           draw0, n_calls * n, SEED)
        B = n * self.rps
        for c in range(n_calls):
            a, b = self.plain.next(n), self.compact.next(n)
            assert b.shape == (B, 9) and torch.equal(a, b), (c, draw0)
            assert torch.equal(self.plain.last_ids, self.compact.last_ids)
            assert np.array_equal(b.cpu().numpy(), want[c * B:(c + 1) * B]), (c, draw0)
            assert np.array_equal(self.compact.last_ids.cpu().numpy(), want_ids[c * n:(c + 1) * n])
        assert self.compact.draw == draw0 + n_calls * n


@pytest.mark.parametrize("shuffle", [True, False])
def test_two_groups_equal_the_plain_store(shuffle):
    """H = 20, W = 24 at 64 rays a shard: K = 3 with three focals on the device (1440 rows: 22 shards, 32 rows dropped), then
    K = 2 with the scalar focal (15 shards, landing at pose 3).  15 x next(5) = 75 draws cross two epoch boundaries of the 37
    shards.  64 rays a shard is a partial tile of the batch kernel (1024 rows a pass)."""
    H, W, rps = 20, 24, 64
    pair = Pair(40, 5, H, W, rps, shuffle)
    assert pair.append(_group(3, H, W, [27.5, 31.25, 40.125], 1), 0xC0FFEE1234) == 22
    assert pair.append(_group(2, H, W, 33.5, 2), 987654321987) == 15
    assert pair.compact.n_poses == 5 and pair.pose0[22] == 3
    pair.draw(15)
    # the two-buffer contract of next: the tensor of call k is unchanged after call k + 1, and replaced by call k + 2
    b0 = pair.compact.next(5)
    keep = b0.clone()
    b1 = pair.compact.next(5)
    assert b0.data_ptr() != b1.data_ptr() and torch.equal(b0, keep)
    # seek: a pure function of the draw number
    pair.compact.seek(10)
    pair.plain.seek(10)
    pair.draw(2)
    with pytest.raises(NotImplementedError):
        pair.compact.plan()
    assert not hasattr(pair.compact, "append_files")
    assert "compact" in pair.compact.describe() and "16 B/ray + 52 B/pose + 4 B/shard" in pair.compact.describe()
    pair.compact.close()
    with pytest.raises(RuntimeError):
        pair.compact.next(5)


def test_one_large_shard():
    """4096 rays a shard at K = 3, H = W = 40: one shard, 704 rows dropped; four full passes of the batch kernel per draw."""
    H = W = 40
    pair = Pair(1, 3, H, W, 4096, True)
    assert pair.append(_group(3, H, W, [55.5, 61., 47.75], 3), 0x9E3779B97F4A7C15) == 1
    pair.draw(2)
    # rays_per_shard that is no multiple of the kernel's pass: 1024 + 512 + 4 rows
    pair = Pair(3, 3, H, W, 1540, True)
    assert pair.append(_group(3, H, W, 50., 4), 77) == 3
    pair.draw(2)


def test_growing_store():
    """The --r2l_kd_every case: draws, then another flush group, then draws with the shard count of the moment."""
    H, W, rps = 20, 24, 64
    pair = Pair(40, 5, H, W, rps, True)
    pair.append(_group(3, H, W, [27.5, 31.25, 40.125], 1), 11)
    pair.draw(3)
    pair.append(_group(2, H, W, 33.5, 2), 12)
    pair.draw(9)  # 15 + 45 draws: past an epoch boundary of the 37 shards


def test_high_ids():
    """ids above 2^31: a hand-written store of 46341 x 46341 frames (H*W = 2^31 + 4633) and one shard of four rows — only those
    four rows are allocated.  The id arithmetic is unsigned.  id 2^31 + 12345 is past H*W - 1, the last pixel of pose 0: it is
    pixel 7712 of pose 1, so the table holds two poses and the quotient id / (H*W) is exercised on a high id too."""
    from r2l_amd import _lib
    from r2l_amd.raystore import cstore_batch_spec
    lib = _lib.load()
    H = W = 46341
    assert H * W > 2**31
    ids = np.array([0, 2**31 + 12345, H * W - 1, 1234567890], dtype=np.uint32)
    rng = np.random.RandomState(5)
    rgb = rng.rand(4, 3).astype(np.float32)
    rows_np = np.concatenate([rgb.view(np.uint32), ids[:, None]], 1)
    rows = torch.from_numpy(rows_np.view(np.int32)).cuda()
    c2w = torch.from_numpy(np.stack([_pose(rng), _pose(rng)])).cuda()
    focal = torch.tensor([51234.5, 60000.25], dtype=torch.float32, device="cuda")
    pose0 = torch.zeros(1, dtype=torch.int32, device="cuda")
    desc = _lib.CompactStoreDesc(rows=rows.data_ptr(), pose_c2w=c2w.data_ptr(), pose_focal=focal.data_ptr(), shard_pose0=pose0.data_ptr(),
                                 capacity_shards=1, capacity_poses=2, rays_per_shard=4, H=H, W=W)
    bbuf, batch = guarded(2 * 4 * 9, -3.)
    ibuf, got_ids = guarded(2, -1, torch.int32)
    _lib.check(lib.r2l_cstore_batch(ctypes.byref(desc), 1, 0, 2, SEED, _p(batch), _p(got_ids), _st()), "r2l_cstore_batch")
    want, want_ids = cstore_batch_spec(rgb, ids, c2w.cpu().numpy(), focal.cpu().numpy(), [0], H, W, 1, 4, 0, 2, SEED)
    assert guards_ok(bbuf) and guards_ok(ibuf)
    got = batch.view(8, 9).cpu().numpy()
    assert np.all(np.isfinite(got)) and np.array_equal(got, want) and np.array_equal(got_ids.cpu().numpy(), want_ids)
    # the rows are those pixels: the last pixel of the frame, and a pixel whose id has the top bit set
    assert np.array_equal(got[2, 3:6], cstore_batch_spec(rgb, [0, 0, H * W - 1, 0], c2w.cpu().numpy(), focal.cpu().numpy(), [0], H, W, 1, 4,
                                                         0, 1, SEED)[0][2, 3:6])
    assert not np.array_equal(got[1, 3:6], got[0, 3:6])
    poses = c2w.cpu().numpy()
    assert np.array_equal(got[1, :3], poses[1, :, 3]) and all(np.array_equal(got[r, :3], poses[0, :, 3]) for r in (0, 2, 3))
    # a row that names a pose outside the table reads nothing: NaN rays, rgb copied
    far = np.array([0, 1, 2, 3], dtype=np.uint32)
    rows_np[:, 3] = far
    rows.copy_(torch.from_numpy(rows_np.view(np.int32)))
    pose0.fill_(7)
    _lib.check(lib.r2l_cstore_batch(ctypes.byref(desc), 1, 0, 1, SEED, _p(batch), None, _st()), "r2l_cstore_batch")
    got = batch.view(8, 9)[:4].cpu().numpy()
    assert np.all(np.isnan(got[:, :6])) and np.array_equal(got[:, 6:], rgb) and guards_ok(bbuf)


def test_teacher_fill(tiny):  # noqa: F811
    """TeacherFill on the tiny teacher with use_rand_focal (a focal per pose): a plain and a compact store filled with the same
    arguments hand out the same epoch of draws.  The compact fill asks render_frames for rgb alone."""
    from r2l_amd import options
    from r2l_amd.online_kd import fill_store_from_teacher
    from r2l_amd.raystore import CompactRayStore, RayStore
    targs = options.parse_teacher_config(tiny["teacher_cfg"], teacher_ckpt=tiny["ck"])
    targs.use_rand_focal = True
    plain, compact = RayStore(3, "cuda", seed=7), CompactRayStore(3, 3, 64, 64, "cuda", seed=7)
    log = _Log()
    for store in (plain, compact):
        state = fill_store_from_teacher(store, targs, 64, 64, tiny["focal"], 2., 6., 3, 2, 0, 1, "cuda", logger=log)
        assert state.done and store.n_shards == 3
    assert compact.n_poses == 3 and compact.shard_pose0.cpu().tolist() == [0, 0, 2]  # groups of two poses and of one
    focals = compact.pose_focal.cpu().numpy()
    assert len(set(focals.tolist())) == 3 and np.all(focals >= np.float32(tiny["focal"]))  # focal x U[1, 2) per pose
    assert any("compact, 3 / 3 shards" in l for l in log.lines), log.lines
    a, b = plain.next(3), compact.next(3)
    assert torch.equal(plain.last_ids, compact.last_ids) and sorted(compact.last_ids.cpu().tolist()) == [0, 1, 2]
    assert torch.equal(a, b)
    assert float(a[:, 6:9].std()) > 0  # the teacher rendered something


@pytest.fixture(scope="module")
def cli_runs(tiny, tmp_path_factory):  # noqa: F811
    """Six iterations of main.py --r2l_online_kd --r2l_kd_every 2 (three flush groups of one pose: the store grows at iterations 2
    and 4), without and with --r2l_compact_store; checkpoints at 3 and 6.  Exact-fp32 kernels: they have no range control, so the
    resumed run below differs from the uninterrupted one in nothing but where its data comes from."""
    from r2l_amd import driver
    cwd, work = os.getcwd(), tmp_path_factory.mktemp("cstore_cli")
    os.chdir(str(work))
    try:
        extra = ["--r2l_online_kd", "--r2l_teacher_config", tiny["teacher_cfg"], "--teacher_ckpt", tiny["ck"], "--n_pose_kd", "3",
                 "--create_data_chunk", "1", "--r2l_kd_every", "2", "--r2l_device_pool", "--r2l_precision", "fp32_mfma", "--i_weights", "3",
                 "--save_intermediate_models", "--N_iters", "6"]
        a = driver.main(_student(tiny, "plain") + extra)
        b = driver.main(_student(tiny, "compact") + extra + ["--r2l_compact_store"])
    finally:
        os.chdir(cwd)
    here = lambda path: os.path.join(str(work), path)  # (the logger's paths are relative to the directory of the run)
    return {"plain": here(a["logger"].weights_path), "compact": here(b["logger"].weights_path), "extra": extra,
            "log": open(here(os.path.join(b["logger"].log_path, "log.txt"))).read()}


def test_cli_compact_store_leaves_the_same_checkpoints(cli_runs):
    from r2l_amd.checkpoint import load_ckpt
    for name in ("ckpt_3.tar", "ckpt_6.tar"):
        a, b = load_ckpt(os.path.join(cli_runs["plain"], name)), load_ckpt(os.path.join(cli_runs["compact"], name))
        assert _ckpt_equal(a, b) == (True, True), name
        assert a["global_step"] == b["global_step"]
    log = cli_runs["log"]
    assert "ray store: compact, 1 / 3 shards of 4096 rays and 1 / 3 poses" in log and "16 B/ray + 52 B/pose + 4 B/shard" in log
    grew = [l.split("Iter ")[1].split(" (")[0] for l in log.splitlines() if "ray store grew to" in l]
    assert grew == ["2 ray store grew to 2 shards", "4 ray store grew to 3 shards"], grew
    assert log.count("[TRAIN] Iter") == 6


def test_cli_compact_store_resumes_bit_for_bit(cli_runs, tiny, tmp_path, monkeypatch):  # noqa: F811
    from r2l_amd import driver
    from r2l_amd.checkpoint import load_ckpt
    monkeypatch.chdir(tmp_path)
    c = driver.main(_student(tiny, "compact_resume") + cli_runs["extra"] +
                    ["--r2l_compact_store", "--pretrained_ckpt", os.path.join(cli_runs["compact"], "ckpt_3.tar"), "--resume"])
    log = _log_of(c)
    # iteration 3 is behind it: two flush groups are re-rendered, the third arrives at iteration 4
    assert "ray store: compact, 2 / 3 shards" in log and "resuming at draw 6" in log
    assert [l.split("[TRAIN] Iter ")[1].split()[0] for l in log.splitlines() if "[TRAIN] Iter" in l] == ["4", "5", "6"]
    assert _ckpt_equal(load_ckpt(os.path.join(cli_runs["compact"], "ckpt_6.tar")),
                       load_ckpt(os.path.join(c["logger"].weights_path, "ckpt_6.tar"))) == (True, True)
