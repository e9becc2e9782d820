"""Compact ray store (include/r2l_hip.h r2l_cstore_append / r2l_cstore_batch; r2l_amd/raystore.py CompactRayStore;
--r2l_compact_store), the parts that need no GPU: the numpy restatement against the plain store's, the argument checks of the two
entry points through the loaded library, the struct's layout, the refusals of the switch and the byte arithmetic."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests.test_driver_cpu import ROOT

INVALID = 1  # hipErrorInvalidValue


def test_spec_equals_the_plain_store_spec():
    """A hand-built flush group, K = 3 poses of 5 x 7 pixels at 8 rays a shard (105 rows: 13 shards, one row dropped).  The plain
    store holds [o, d, rgb] with o, d from pixel_batch's host arithmetic (render.get_rays on CPU tensors), shuffled by perm; the
    compact spec must hand out the same batches, across an epoch boundary."""
    from r2l_amd import raystore as R
    from r2l_amd.render import get_rays
    K, H, W, rps, key, seed = 3, 5, 7, 8, 0xC0FFEE1234, 77
    rng = np.random.RandomState(11)
    c2w = rng.randn(K, 3, 4).astype(np.float32)
    focal = (6. + 3. * rng.rand(K)).astype(np.float32)
    rgb = rng.rand(K * H * W, 3).astype(np.float32)
    od = []
    for k in range(K):
        o, d = get_rays(H, W, float(focal[k]), torch.from_numpy(c2w[k]))
        od.append(np.concatenate([o.reshape(-1, 3).numpy(), d.reshape(-1, 3).numpy()], 1))
    rows9 = np.concatenate([np.concatenate(od, 0), rgb], 1)
    n_rows, m = K * H * W, K * H * W // rps
    assert (n_rows, m, n_rows - m * rps) == (105, 13, 1)
    # pixel_ray_spec is that arithmetic
    ids_all = np.arange(n_rows)
    o, d = R.pixel_ray_spec(c2w[ids_all // (H * W)], focal[ids_all // (H * W)], H, W, ids_all % (H * W) // W, ids_all % W)
    assert o.dtype == d.dtype == np.float32 and np.array_equal(o, rows9[:, :3]) and np.array_equal(d, rows9[:, 3:6])
    for shuffle in (True, False):
        order = R.perm(key, n_rows)[:m * rps] if shuffle else np.arange(m * rps)
        plain = rows9[order]
        rgb_rows, ids = R.cstore_append_spec(rgb, rps, key, shuffle=shuffle)
        assert ids.dtype == np.uint32 and np.array_equal(ids, order) and np.array_equal(rgb_rows, rgb[order])
        assert len(set(order.tolist())) == m * rps  # one row of the group is dropped, none repeated
        shard_pose0 = np.zeros(m, dtype=np.int32)
        for draw0, n_draw in ((0, 5), (11, 4), (2 * m - 1, 3)):  # the last two cross an epoch boundary
            po, pd, pt, pids, _ = R.train_batch_spec(plain, m, rps, draw0, n_draw, seed)
            batch, cids = R.cstore_batch_spec(rgb_rows, ids, c2w, focal, shard_pose0, H, W, m, rps, draw0, n_draw, seed)
            assert batch.dtype == np.float32 and batch.shape == (n_draw * rps, 9) and cids.dtype == np.int32
            assert np.array_equal(cids, pids)
            assert np.array_equal(batch[:, :3], po) and np.array_equal(batch[:, 3:6], pd) and np.array_equal(batch[:, 6:], pt)
    # a second group behind the first: its shards point at pose 3 of the table
    c2w2 = np.concatenate([c2w, rng.randn(2, 3, 4).astype(np.float32)], 0)
    focal2 = np.concatenate([focal, np.full(2, 7.5, np.float32)])
    rgb2 = rng.rand(2 * H * W, 3).astype(np.float32)
    r2, i2 = R.cstore_append_spec(rgb2, rps, key + 1)
    m2 = 2 * H * W // rps
    pose0 = np.concatenate([np.zeros(m, np.int32), np.full(m2, 3, np.int32)])
    batch, cids = R.cstore_batch_spec(np.concatenate([rgb_rows, r2]), np.concatenate([ids, i2]), c2w2, focal2, pose0, H, W, m + m2, rps,
                                      0, m + m2, seed)
    for j, s in enumerate(cids):
        if s >= m:
            g = i2[(s - m) * rps:(s - m + 1) * rps].astype(np.int64)
            o, d = get_rays(H, W, 7.5, torch.from_numpy(c2w2[3 + g[0] // (H * W)]))
            assert np.array_equal(batch[j * rps, :3], o.reshape(-1, 3).numpy()[g[0] % (H * W)])
            assert np.array_equal(batch[j * rps, 3:6], d.reshape(-1, 3).numpy()[g[0] % (H * W)])
            assert np.array_equal(batch[j * rps:(j + 1) * rps, 6:], rgb2[g])


def _desc(**kw):
    from r2l_amd import _lib
    d = dict(rows=64, pose_c2w=64, pose_focal=64, shard_pose0=64, capacity_shards=4, capacity_poses=4, rays_per_shard=4, H=2, W=4)
    d.update(kw)
    res = d.pop("reserved", None)
    s = _lib.CompactStoreDesc(**d)
    if res is not None:
        s.reserved[res[0]] = res[1]
    return s


def test_abi_argument_checks():
    """Every refusal is hipErrorInvalidValue with the argument's name in r2l_last_error, before anything is launched (NULL and
    dummy pointers: this runs without a GPU)."""
    from r2l_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(64)  # any non-NULL, 16-byte aligned value: the checks fail before it is ever dereferenced
    m = ctypes.c_int64(-5)
    mp = ctypes.cast(ctypes.byref(m), ctypes.c_void_p)

    def append(store=None, rgb=one, stride=3, c2w=one, fdev=one, focal=0., K=1, first_shard=0, first_pose=0, n_written=mp):
        s = _desc() if store is None else store
        return lib.r2l_cstore_append(ctypes.byref(s) if s != "null" else None, rgb, stride, c2w, fdev, focal, K, first_shard, first_pose,
                                     1, 1, n_written, None)

    # K = 1, H*W = 8, rays_per_shard 4: m = 2 shards
    for kw, word in ((dict(store="null"), b"NULL"),
                     (dict(store=_desc(rows=0)), b"NULL"),
                     (dict(store=_desc(pose_c2w=0)), b"NULL"),
                     (dict(store=_desc(pose_focal=0)), b"NULL"),
                     (dict(store=_desc(shard_pose0=0)), b"NULL"),
                     (dict(rgb=None), b"NULL"),
                     (dict(c2w=None), b"NULL"),
                     (dict(n_written=None), b"NULL"),
                     (dict(K=0), b"K"),
                     (dict(K=-3), b"K"),
                     (dict(store=_desc(H=0)), b"H"),
                     (dict(store=_desc(W=-1)), b"W"),
                     (dict(first_shard=3), b"capacity_shards"),             # 3 + 2 > 4
                     (dict(store=_desc(capacity_shards=1)), b"capacity_shards"),  # 0 + 2 > 1
                     (dict(first_shard=-1), b"first_shard"),
                     (dict(K=2, first_pose=3), b"capacity_poses"),          # 3 + 2 > 4
                     (dict(K=5, store=_desc(capacity_shards=40)), b"capacity_poses"),
                     (dict(first_pose=-1), b"first_pose"),
                     (dict(store=_desc(rays_per_shard=0)), b"rays_per_shard"),
                     (dict(store=_desc(rays_per_shard=-4)), b"rays_per_shard"),
                     (dict(store=_desc(rays_per_shard=6)), b"rays_per_shard"),
                     (dict(stride=2), b"rgb_stride"),
                     (dict(stride=0), b"rgb_stride"),
                     (dict(fdev=None, focal=0.), b"focal"),
                     (dict(fdev=None, focal=-2.), b"focal"),
                     (dict(store=_desc(reserved=(0, 1))), b"reserved"),
                     (dict(store=_desc(reserved=(1, 7))), b"reserved"),
                     (dict(store=_desc(rows=68)), b"aligned"),
                     (dict(K=2, store=_desc(H=46341, W=46341, capacity_shards=2**30, capacity_poses=2**30)), b"2^32")):
        assert append(**kw) == INVALID, kw
        msg = lib.r2l_last_error()
        assert b"r2l_cstore_append" in msg and word in msg, (kw, msg)
    assert m.value == -5  # nothing was written on a refused call

    def batch(store=None, n_shards=3, draw0=0, n_draw=1, out=one):
        s = _desc() if store is None else store
        return lib.r2l_cstore_batch(ctypes.byref(s) if s != "null" else None, n_shards, draw0, n_draw, 0, out, None, None)

    for kw, word in ((dict(store="null"), b"NULL"),
                     (dict(store=_desc(rows=0)), b"NULL"),
                     (dict(store=_desc(shard_pose0=0)), b"NULL"),
                     (dict(out=None), b"NULL"),
                     (dict(store=_desc(rays_per_shard=0)), b"rays_per_shard"),
                     (dict(store=_desc(rays_per_shard=10)), b"rays_per_shard"),
                     (dict(n_shards=0), b"n_shards"),
                     (dict(n_shards=-2), b"n_shards"),
                     (dict(n_shards=5), b"n_shards"),                       # beyond capacity_shards
                     (dict(n_draw=-1), b"n_draw"),
                     (dict(draw0=-1), b"draw0"),
                     (dict(store=_desc(rows=68)), b"aligned"),
                     (dict(out=ctypes.c_void_p(72)), b"aligned"),
                     (dict(store=_desc(H=0)), b"H"),
                     (dict(store=_desc(reserved=(0, 1))), b"reserved"),
                     (dict(store=_desc(H=2**17, W=2**17)), b"2^32")):
        assert batch(**kw) == INVALID, kw
        msg = lib.r2l_last_error()
        assert b"r2l_cstore_batch" in msg and word in msg, (kw, msg)
    # what needs no launch succeeds without a GPU: fewer rows than a shard write nothing, no draws compute nothing
    assert append(store=_desc(rays_per_shard=12)) == 0 and m.value == 0
    assert batch(n_draw=0) == 0


def test_struct_is_the_headers(tmp_path):
    """72 bytes, no padding; with a C compiler at hand, sizeof and every offset as a C99 translation unit of the header sees them."""
    from r2l_amd import _lib
    S = _lib.CompactStoreDesc
    assert ctypes.sizeof(S) == 72
    offsets = [getattr(S, n).offset for n, _ in S._fields_]
    assert offsets == [0, 8, 16, 24, 32, 40, 48, 56, 60, 64]
    assert sum(ctypes.sizeof(t) for _, t in S._fields_) == 72  # the fields alone fill it
    for name in ("r2l_cstore_append", "r2l_cstore_batch"):
        assert name in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    if shutil.which("gcc") is None:
        return
    src = tmp_path / "size.c"
    fields = ["rows", "pose_c2w", "pose_focal", "shard_pose0", "capacity_shards", "capacity_poses", "rays_per_shard", "H", "W", "reserved"]
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "r2l_hip.h"\nint main(void) {\n    printf("%d", (int)sizeof(r2l_cstore));\n'
                   + "".join('    printf(" %%d", (int)offsetof(r2l_cstore, %s));\n' % f for f in fields) + "    return 0;\n}\n")
    exe = str(tmp_path / "size")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()]
    assert got == [ctypes.sizeof(S)] + offsets, got


def test_options(tmp_path):
    from r2l_amd import options
    teacher_cfg = os.path.join(ROOT, "configs", "lego.txt")
    online = ["--r2l_online_kd", "--r2l_teacher_config", teacher_cfg, "--teacher_ckpt", "t.tar", "--n_pose_kd", "12"]
    assert options.parse_args([]).r2l_compact_store is False
    a = options.parse_args(online + ["--r2l_compact_store", "--r2l_kd_every", "2"])
    assert a.r2l_compact_store and a.r2l_online_kd
    options.validate_accelerated(a)
    options.validate_compact_store(a)
    cfg = tmp_path / "student.txt"
    cfg.write_text("r2l_online_kd = True\nr2l_compact_store = True\nteacher_ckpt = t.tar\nr2l_teacher_config = %s\n" % teacher_cfg)
    a = options.parse_args(["--config", str(cfg)])
    assert a.r2l_compact_store and a.r2l_online_kd
    options.validate_accelerated(a)
    cfg.write_text("r2l_compact_store = False\n")
    assert not options.parse_args(["--config", str(cfg)]).r2l_compact_store
    # the three refusals at start-up, each naming the other flag
    files = ["--data_mode", "rays", "--datadir_kd", "somewhere"]
    for argv, word in ((["--r2l_compact_store"], "--r2l_online_kd"),
                       (["--r2l_compact_store", "--r2l_device_store"] + files, "--r2l_device_store"),
                       (online + ["--r2l_compact_store", "--r2l_device_store"] + files, "--r2l_device_store"),
                       (online + ["--r2l_compact_store", "--r2l_fused_iter"], "--r2l_fused_iter")):
        with pytest.raises(ValueError) as e:
            a = options.parse_args(argv)
            options.validate_accelerated(a)
            options.validate_fused_iter(a)
            options.validate_compact_store(a)  # (main.py's three checks, in its order)
        assert word in str(e.value), (argv, str(e.value))
    # the sibling entry points share the option table and run validate_accelerated alone: they accept and ignore the flag
    a = options.parse_args(["--config", teacher_cfg, "--r2l_compact_store"])
    assert a.r2l_compact_store
    options.validate_accelerated(a)


def test_byte_arithmetic():
    """The size table of the README: 16 B/ray + 52 B/pose + 4 B/shard against 36 B/ray."""
    from r2l_amd.online_kd import shards_needed
    from r2l_amd.raystore import CompactRayStore
    shards = shards_needed(10000, 100, 400, 400)
    assert shards == 100 * (100 * 400 * 400 // 4096) == 390600
    need = CompactRayStore.bytes_needed(shards, 10000)
    assert need == shards * 4096 * 16 + 10000 * 52 + shards * 4
    assert "%.1f" % (need / 1e9) == "25.6" and "%.1f" % (shards * 4096 * 36 / 1e9) == "57.6"
    big = shards_needed(10000, 100, 800, 800)
    assert "%.1f" % (CompactRayStore.bytes_needed(big, 10000) / 1e9) == "102.4" and "%.1f" % (big * 4096 * 36 / 1e9) == "230.4"
    many = shards_needed(40000, 100, 400, 400)
    assert "%.1f" % (CompactRayStore.bytes_needed(many, 40000) / 1e9) == "102.4"
    # the store itself lives in device memory and says so
    with pytest.raises(RuntimeError, match="ROCm device"):
        CompactRayStore(4, 1, 8, 8, "cpu")
