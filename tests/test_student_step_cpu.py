"""The fused student iteration (include/r2l_hip.h r2l_train_batch / r2l_student_train_step; main.py --r2l_fused_iter), host side,
without a GPU: the library's exports, the numpy restatement of the batch kernel, the pool's plan / advance bookkeeping against
augment / update, and the refusals of the switch."""
import ctypes
import os

import numpy as np
import pytest
import torch

from r2l_amd import raystore
from r2l_amd.driver import HardRayPool
from r2l_amd.options import parse_args, validate_accelerated, validate_fused_iter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_fused_iteration():
    from r2l_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("r2l_train_batch", "r2l_student_step_work_floats", "r2l_student_train_step", "r2l_last_error"):
        assert hasattr(lib, name), name
    for name in ("r2l_train_batch", "r2l_student_step_work_floats", "r2l_student_train_step"):
        assert name in _lib.SIGNATURES
    # the ctypes struct is the header's: 168 bytes, no padding (4 int, pointer, 13 eight-byte fields, 4 float, int64, 4 int)
    assert ctypes.sizeof(_lib.StudentStepDesc) == 168
    assert _lib.StudentStepDesc.step.offset == 144 and _lib.StudentStepDesc.lw_rgb.offset == 120


def test_work_size_query_checks_the_descriptor_without_a_gpu():
    from r2l_amd import _lib
    lib = _lib.load()
    d = _lib.StudentStepDesc(n_block=2, rays_per_shard=12, n_shards=3, n_draw=3, step=1, n_in=9, n_out=9, pool_capacity_rows=18)
    n = lib.r2l_student_step_work_floats(ctypes.byref(d))
    assert n > 0 and n % 1024 == 0  # every part on a 4 KiB boundary
    d.perturb = 1
    assert lib.r2l_student_step_work_floats(ctypes.byref(d)) == n + 1024  # t_rand [36, 16]
    d.rays_per_shard = 10
    assert lib.r2l_student_step_work_floats(ctypes.byref(d)) == -1 and b"rays_per_shard" in lib.r2l_last_error()


def test_train_batch_spec_is_shard_ids_and_perm_composed():
    """Across an epoch boundary (7 shards, draws 5 .. 9) and with pool rows: rows of shard_ids(...) then pool[perm(key, n)[:n_out]]."""
    rng = np.random.RandomState(3)
    rps, n_shards, seed, key = 4, 7, 0xDEADBEEF12345, 0x1234567890ABCDEF
    store = rng.rand(n_shards * rps, 9).astype(np.float32)
    pool = rng.rand(11, 9).astype(np.float32)
    o, d, t, ids, idx = raystore.train_batch_spec(store, n_shards, rps, 5, 5, seed, pool, 11, 5, key)
    want_ids = raystore.shard_ids(seed, n_shards, 5, 5)
    assert ids.dtype == np.int32 and np.array_equal(ids, want_ids)
    # two epochs: draws 5, 6 close epoch 0, draws 7 .. 9 open epoch 1
    p0, p1 = raystore.perm(raystore.epoch_key(seed, 0), n_shards), raystore.perm(raystore.epoch_key(seed, 1), n_shards)
    assert np.array_equal(want_ids, np.concatenate([p0[5:7], p1[0:3]]))
    want_idx = raystore.perm(key, 11)[:5]
    assert idx.dtype == np.int64 and np.array_equal(idx, want_idx)
    rows = np.concatenate([store[i * rps:(i + 1) * rps] for i in want_ids] + [pool[want_idx]], 0)
    assert o.shape == d.shape == t.shape == (5 * rps + 5, 3)
    assert np.array_equal(o, rows[:, :3]) and np.array_equal(d, rows[:, 3:6]) and np.array_equal(t, rows[:, 6:])
    # no pool rows: the shard rows alone
    o2, _, t2, _, idx2 = raystore.train_batch_spec(store, n_shards, rps, 5, 5, seed)
    assert idx2.shape == (0,) and np.array_equal(o2, o[:5 * rps]) and np.array_equal(t2, t[:5 * rps])


class _KeyedPool(HardRayPool):
    """The pool on CPU tensors with the device path's row choice: _pick counts its draws and derives the key as the CUDA branch
    does, and evaluates the bijection with its numpy restatement (raystore.perm_at) instead of r2l_pool_pick."""

    def _pick(self, n_rows, n_out, device):
        self._draws += 1
        self.keys.append(self._key(self._draws))
        return torch.from_numpy(raystore.perm_at(self.keys[-1], n_rows, np.arange(n_out, dtype=np.uint64)))


def test_pool_plan_and_advance_follow_augment_and_update():
    B = 36
    g = torch.Generator().manual_seed(5)
    a = _KeyedPool(0.25, 0.5, seed=1003)
    a.keys = []
    b = HardRayPool(0.25, 0.5, seed=1003, device_select=True)
    for step in range(6):
        plan = b.plan(B)
        assert (plan["n_in"], plan["n_out"]) == (9, 9) and plan["capacity"] == 18
        rows = torch.rand(B, 9, generator=g)
        was_full, rows_before = a.full, 0 if a.pool is None else a.pool.shape[0]
        o, d, t = a.augment(rows[:, :3], rows[:, 3:6], rows[:, 6:])
        assert o.shape[0] == B + (9 if was_full else 0)
        assert (plan["full"], plan["pool_rows"]) == (was_full, rows_before)
        if was_full:
            assert plan["key"] == a.keys[-1]
        a.update(torch.rand(o.shape[0], 3, generator=g), o, d, t, B)
        b.advance(B)
        assert (b._n, b.full, b._draws) == (a._n, a.full, a._draws), step
    assert a.full and a._draws == 4 and len(a.keys) == 4  # full after two steps, four keyed picks
    sa, sb = a.state_dict(), b.state_dict()
    assert {k: sa[k] for k in ("full", "n", "draws", "hard_ratio", "hard_mul", "batch_size")} == \
           {k: sb[k] for k in ("full", "n", "draws", "hard_ratio", "hard_mul", "batch_size")}
    # a pool that takes nothing in never fills, and its plan says so
    c = HardRayPool(0.01, 1.0, seed=1)
    assert c.plan(B) == {"n_in": 0, "n_out": 0, "pool_rows": 0, "full": False, "capacity": 0, "key": 0}
    c.advance(B)
    assert not c.full and c._draws == 0


def _args(*extra):
    return parse_args(["--model_name", "R2L", "--config", os.path.join(ROOT, "configs", "lego_noview.txt")] + list(extra))


def test_fused_iter_switch_and_its_refusals(tmp_path):
    store = ["--r2l_device_store", "--data_mode", "rays", "--datadir_kd", "somewhere"]
    assert not _args().r2l_fused_iter
    ok = _args("--r2l_fused_iter", "--r2l_device_pool", "--hard_ratio", "0.2", *store)
    assert ok.r2l_fused_iter
    validate_accelerated(ok)
    validate_fused_iter(ok)
    validate_fused_iter(_args("--r2l_fused_iter", *store))  # no pool at all
    cfg = tmp_path / "c.txt"
    cfg.write_text("r2l_fused_iter = True\n")
    assert parse_args(["--config", str(cfg)]).r2l_fused_iter  # the config key
    with pytest.raises(ValueError, match="r2l_device_store or --r2l_online_kd"):
        validate_fused_iter(_args("--r2l_fused_iter", "--data_mode", "rays", "--datadir_kd", "somewhere"))
    with pytest.raises(ValueError, match="r2l_device_pool"):
        validate_fused_iter(_args("--r2l_fused_iter", "--hard_ratio", "0.2", *store))
    with pytest.raises(NotImplementedError, match="on the CPU"):
        validate_fused_iter(ok, 1, "cpu")
    with pytest.raises(NotImplementedError, match="world size 1"):
        validate_fused_iter(ok, 2, "cuda")
    # without the switch nothing is asked
    validate_fused_iter(_args("--hard_ratio", "0.2"), 8, "cpu")


def test_other_drivers_accept_and_ignore_the_switch():
    """utils/create_data.py and utils/train_nerf.py share the parser and its validation: the switch parses and is not looked at."""
    a = parse_args(["--config", os.path.join(ROOT, "configs", "lego.txt"), "--r2l_fused_iter"])
    assert a.r2l_fused_iter
    validate_accelerated(a)  # (no ray store named: only main.py asks for one)
