"""Device-resident ray store, the parts that need no GPU: the numpy restatement of the bijection and of the sampler
(r2l_amd/raystore.py perm / shard_ids — the specification of what r2l_store_append / r2l_store_batch compute), the argument
checks of the two entry points through the loaded library, and the new command-line flags."""
import ctypes
import os

import numpy as np
import pytest

from tests.test_driver_cpu import ROOT

SIZES = [1, 2, 3, 4, 5, 16, 17, 4095, 4096, 4097, 65537]
KEYS = [0, 1, 0x9E3779B97F4A7C15, 2**64 - 1, 123456789012345]


def splitmix64(x):
    m = (1 << 64) - 1
    z = (x + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


@pytest.mark.parametrize("n", SIZES)
def test_perm_is_a_bijection(n):
    from r2l_amd.raystore import perm
    seen = set()
    for key in KEYS:
        p = perm(key, n)
        assert p.dtype == np.int64 and p.shape == (n,)
        assert np.array_equal(np.sort(p), np.arange(n)), (key, n)
        seen.add(p.tobytes())
    if n >= 16:
        assert len(seen) == len(KEYS)  # the key matters


@pytest.mark.parametrize("n_shards", [1, 2, 7, 24, 25])
def test_sampler(n_shards):
    from r2l_amd.raystore import epoch_key, perm, shard_ids
    seed = 77
    ids = shard_ids(seed, n_shards, 0, 6 * n_shards)
    for e in range(6):  # every aligned block of n_shards draws is a permutation: the one of its epoch
        block = ids[e * n_shards:(e + 1) * n_shards]
        assert np.array_equal(np.sort(block), np.arange(n_shards)), (n_shards, e)
        assert np.array_equal(block, perm(epoch_key(seed, e), n_shards))
    if n_shards >= 7:
        assert len({ids[e * n_shards:(e + 1) * n_shards].tobytes() for e in range(6)}) > 1  # a fresh order per epoch
        assert not np.array_equal(ids, shard_ids(seed + 1, n_shards, 0, 6 * n_shards))  # and per seed
    # a request that straddles two epochs is the concatenation of their parts
    a, c = max(n_shards - 2, 0), n_shards + 3
    got = shard_ids(seed, n_shards, a, c)
    assert np.array_equal(got, ids[a:a + c])
    assert np.array_equal(got[:n_shards - a], perm(epoch_key(seed, 0), n_shards)[a:])
    assert np.array_equal(got[n_shards - a:2 * n_shards - a], perm(epoch_key(seed, 1), n_shards))
    # pure function of the draw number: shard_ids(seed, n, a + b, c) is the tail of shard_ids(seed, n, a, b + c)
    for a, b, c in ((0, 1, 1), (3, 5, 9), (n_shards, n_shards + 1, 2 * n_shards), (10**9 + 7, 4, 30)):
        assert np.array_equal(shard_ids(seed, n_shards, a + b, c), shard_ids(seed, n_shards, a, b + c)[b:])


def test_shuffle_spreads_poses_over_shards_like_a_true_permutation():
    """8 'poses' of 4096 rows shuffled into 8 shards, 300 fixed keys: the chi-square of the 8 x 8 pose-by-shard table has 49
    degrees of freedom under a uniformly random permutation (mean 49, variance 98 -> standard error of the mean of 300 tables
    0.57).  Bounds: mean within 49 +- 1.7 (three standard errors), maximum below 120 (a single table exceeds that with
    probability < 1e-7); fewer than 1 % of neighbouring output rows were neighbours in the input."""
    from r2l_amd.raystore import perm
    n, rps, poses = 32768, 4096, 8
    chi, neigh = [], []
    for t in range(300):
        p = perm(splitmix64(12345 + t), n)
        table = np.zeros((poses, poses))
        np.add.at(table, (p // rps, np.arange(n) // rps), 1)
        expect = n / poses / poses
        chi.append(((table - expect)**2 / expect).sum())
        neigh.append(np.mean(np.abs(np.diff(p)) == 1))
    print("chi2 of the pose-by-shard table over 300 keys: mean %.2f max %.2f; neighbouring rows kept: %.4f %%" %
          (np.mean(chi), np.max(chi), 100 * np.mean(neigh)))
    assert abs(np.mean(chi) - 49.) <= 1.7
    assert np.max(chi) < 120.
    assert np.max(neigh) < 0.01


def test_abi_argument_checks():
    """Every violation is hipErrorInvalidValue with a message, before anything is launched (so this runs without a GPU)."""
    from r2l_amd import _lib
    lib = _lib.load()
    INVALID = 1
    one = ctypes.c_void_p(64)  # any non-NULL (and 16-byte aligned) value: the checks fail before it is ever dereferenced
    m = ctypes.c_int64(-5)
    mp = ctypes.cast(ctypes.byref(m), ctypes.c_void_p)
    #         rows_in n_rows store cap first rps key shuffle n_written stream
    for args, word in (((None, 8, one, 4, 0, 4, 1, 1, mp, None), b"NULL"),
                       ((one, 8, None, 4, 0, 4, 1, 1, mp, None), b"NULL"),
                       ((one, 8, one, 4, 0, 4, 1, 1, None, None), b"NULL"),
                       ((one, 8, one, 4, 0, 0, 1, 1, mp, None), b"rays_per_shard"),
                       ((one, 8, one, 4, 0, -4, 1, 1, mp, None), b"rays_per_shard"),
                       ((one, 8, one, 4, 0, 6, 1, 1, mp, None), b"rays_per_shard"),
                       ((one, 8, one, 4, 3, 4, 1, 1, mp, None), b"capacity_shards"),   # 3 + 2 > 4
                       ((one, 20, one, 4, 0, 4, 1, 1, mp, None), b"capacity_shards"),  # 0 + 5 > 4
                       ((one, 8, one, 4, -1, 4, 1, 1, mp, None), b"first_shard"),
                       ((one, -8, one, 4, 0, 4, 1, 1, mp, None), b"n_rows")):
        assert lib.r2l_store_append(*args) == INVALID, args
        msg = lib.r2l_last_error()
        assert b"r2l_store_append" in msg and word in msg, (args, msg)
    assert m.value == -5  # nothing was written on a refused call
    #         store n_shards rps draw0 n_draw seed batch ids stream
    for args, word in (((None, 3, 4, 0, 1, 0, one, None, None), b"NULL"),
                       ((one, 3, 4, 0, 1, 0, None, None, None), b"NULL"),
                       ((one, 3, 0, 0, 1, 0, one, None, None), b"rays_per_shard"),
                       ((one, 3, 10, 0, 1, 0, one, None, None), b"rays_per_shard"),
                       ((one, 0, 4, 0, 1, 0, one, None, None), b"n_shards"),
                       ((one, -2, 4, 0, 1, 0, one, None, None), b"n_shards"),
                       ((one, 3, 4, 0, -1, 0, one, None, None), b"n_draw"),
                       ((one, 3, 4, -1, 1, 0, one, None, None), b"draw0"),
                       ((ctypes.c_void_p(68), 3, 4, 0, 1, 0, one, None, None), b"aligned")):
        assert lib.r2l_store_batch(*args) == INVALID, args
        msg = lib.r2l_last_error()
        assert b"r2l_store_batch" in msg and word in msg, (args, msg)
    # what needs no launch succeeds without a GPU: fewer rows than a shard write nothing, no draws copy nothing
    assert lib.r2l_store_append(one, 3, one, 4, 4, 4, 1, 1, mp, None) == 0 and m.value == 0
    assert lib.r2l_store_batch(one, 3, 4, 0, 0, 0, one, None, None) == 0


def test_options(tmp_path):
    from r2l_amd import options
    from r2l_amd.online_kd import check_teacher_args, fill_store_from_teacher, rank_poses, shards_needed
    teacher_cfg = os.path.join(ROOT, "configs", "lego.txt")
    a = options.parse_args([])
    assert (a.r2l_device_store, a.r2l_online_kd, a.r2l_teacher_config, a.r2l_kd_every) == (False, False, "", 0)
    options.validate_accelerated(a)  # without the flags nothing is asked for
    a = options.parse_args(["--r2l_online_kd", "--r2l_teacher_config", teacher_cfg, "--r2l_kd_every", "7", "--teacher_ckpt", "t.tar",
                            "--n_pose_kd", "12"])
    assert a.r2l_online_kd and a.r2l_teacher_config == teacher_cfg and a.r2l_kd_every == 7 and a.n_pose_kd == 12
    options.validate_accelerated(a)
    cfg = tmp_path / "student.txt"
    cfg.write_text("r2l_device_store = True\nr2l_online_kd = False\nr2l_kd_every = 0\ndata_mode = rays\ndatadir_kd = somewhere\n"
                   "r2l_teacher_config = %s\n" % teacher_cfg)
    a = options.parse_args(["--config", str(cfg)])
    assert a.r2l_device_store and not a.r2l_online_kd and a.r2l_teacher_config == teacher_cfg
    options.validate_accelerated(a)
    cfg.write_text("r2l_online_kd = True\nr2l_kd_every = 3\nteacher_ckpt = t.tar\nr2l_teacher_config = %s\n" % teacher_cfg)
    a = options.parse_args(["--config", str(cfg)])
    assert a.r2l_online_kd and a.r2l_kd_every == 3
    options.validate_accelerated(a)
    # what is missing is named
    for argv, word in ((["--r2l_online_kd", "--r2l_teacher_config", teacher_cfg], "--teacher_ckpt"),
                       (["--r2l_online_kd", "--teacher_ckpt", "t.tar"], "--r2l_teacher_config"),
                       (["--r2l_kd_every", "2"], "--r2l_online_kd"),
                       (["--r2l_device_store"], "--datadir_kd"),
                       (["--r2l_device_store", "--datadir_kd", "d"], "--data_mode rays")):
        with pytest.raises(ValueError) as e:
            options.validate_accelerated(options.parse_args(argv))
        assert word in str(e.value), (argv, str(e.value))
    # the teacher's config is a second namespace; what the fused frames path refuses is refused here
    t = options.parse_teacher_config(teacher_cfg, teacher_ckpt="t.tar")
    assert t.use_viewdirs and t.N_samples == 64 and t.N_importance == 128 and t.teacher_ckpt == "t.tar"
    text = open(teacher_cfg).read()
    bad = tmp_path / "lindisp.txt"
    bad.write_text(text + "\nlindisp = True\n")
    with pytest.raises(NotImplementedError):
        options.parse_teacher_config(str(bad))
    bad.write_text(text.replace("use_viewdirs=True", "use_viewdirs=False"))
    with pytest.raises(NotImplementedError):
        options.parse_teacher_config(str(bad))
    bad.write_text(text + "\nraw_noise_std = 1.0\n")
    with pytest.raises(NotImplementedError):
        options.parse_teacher_config(str(bad))
    with pytest.raises(NotImplementedError):
        options.parse_teacher_config(os.path.join(ROOT, "configs", "lego_noview.txt"))  # the student's config is no teacher's
    # the fill itself refuses the same, and a machine without a GPU
    with pytest.raises(NotImplementedError):
        check_teacher_args(options.parse_args(["--use_viewdirs", "--lindisp"]))
    with pytest.raises(NotImplementedError):
        fill_store_from_teacher(None, t, 64, 64, 80., 2., 6., 3, 2, 0, 1, "cpu")
    # pose partition and store size of a rank, as create_data numbers and flushes them
    assert rank_poses(4, 1, 2) == [1, 3] and rank_poses(4, 0, 2) == [2, 4] and rank_poses(3, 0, 1) == [1, 2, 3]
    assert shards_needed(3, 2, 64, 64) == 3 and shards_needed(4, 100, 64, 64, 1, 2) == 2
    assert shards_needed(3, 2, 400, 400) == 78 + 39  # floor(320000 / 4096) + floor(160000 / 4096): a tail per flush group
