"""Ranking the hard rays in the library, on the GPU (include/r2l_hip.h r2l_pool_select; r2l_amd/pool_select.py;
HardRayPool(device_select=True); main.py --r2l_device_pool): the kernel bit for bit against the numpy restatement select_spec at
every size where it takes another path, its memory discipline, the pool against a numpy simulation, a training iteration driven
through the C ABI alone, --resume bit for bit through the CLI, and two ranks."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import r2l_oracle as O
from tests.test_driver_cpu import ROOT, make_scene
from tests.test_forward_gpu import build_model

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4096, 12288, 81920, 1000003)
PATTERNS = ("uniform", "ties", "zero", "magnitudes")
PAD = 51  # rows behind the first B: an augmented batch, of which only the first B rows count


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _inputs(B, pattern):
    """rgb: contiguous [B + PAD, 3]; target: the last three columns of a [B + PAD, 9] tensor (row stride 9).  CPU tensors."""
    rng = np.random.RandomState(B % 9973 + 17 * PATTERNS.index(pattern))
    N = B + PAD
    rgb = rng.rand(N, 3).astype(np.float32)
    rows = rng.rand(N, 9).astype(np.float32)
    if pattern == "ties":
        # four distinct errors, period 11 (no power of two): every tie group is spread over all waves, workgroups and chunks,
        # and with k = B / 5 the threshold falls inside the second group
        rows[:, 6:] = 0.25
        rgb[:] = 0.25
        rgb[:, 0] += np.array([0., 0.25, 0.5, 0.75], dtype=np.float32)[(np.arange(N) * 7 % 11) % 4]
    elif pattern == "zero":
        rgb[:] = rows[:, 6:]
    elif pattern == "magnitudes":
        # |d0| from 1e-30 to 1e30, d1 = d2 = 0: errors from 0 through the denormals up to inf, every radix digit varies; ~1 % NaN
        rows[:, 6:] = 0.
        rgb[:] = 0.
        rgb[:, 0] = (10. ** rng.uniform(-30., 30., N)).astype(np.float32) * np.where(rng.rand(N) < 0.5, -1., 1.).astype(np.float32)
        rgb[rng.rand(N) < 0.01, rng.randint(0, 3)] = np.nan
    return torch.from_numpy(rgb), torch.from_numpy(rows)


def _ks(B):
    return sorted({k for k in (1, B // 5, B - 1, B) if k >= 1})


def _bits(err):
    """fp32 errors as comparable bit patterns: which NaN a NaN row carries is not part of the contract, that it is one is."""
    nan = torch.isnan(err)
    return torch.where(nan, torch.full_like(err, 0.), err).view(torch.int32), nan


_SPEC = {}


def _spec(B, pattern, k):
    """select_spec of the case, computed once per (B, pattern): the errors and the full order do not depend on k."""
    from r2l_amd.pool_select import rank_keys, row_errors
    if (B, pattern) not in _SPEC:
        _SPEC.clear()  # (one case at a time: the 10^6-row arrays are not kept around)
        rgb, rows = _inputs(B, pattern)
        err = row_errors(rgb.numpy()[:B], rows.numpy()[:B, 6:])
        order = np.argsort(np.uint32(0xFFFFFFFF) - rank_keys(err), kind="stable")
        _SPEC[(B, pattern)] = (err, order)
    err, order = _SPEC[(B, pattern)]
    return torch.from_numpy(np.sort(order[:k]).astype(np.int64)), torch.from_numpy(err)


def _call(lib, rgb, target, B, k, hard, err, work):
    from r2l_amd import _lib
    _lib.check(lib.r2l_pool_select(_p(rgb), _p(target), rgb.stride(0), target.stride(0), B, k, _p(hard), _p(err), _p(work), _stream()),
               "r2l_pool_select")


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("B", SIZES)
def test_select_equals_spec(B, pattern):
    from r2l_amd import _lib
    from r2l_amd.pool_select import select, select_spec
    lib = _lib.load()
    rgb_c, rows_c = _inputs(B, pattern)
    rgb, rows = rgb_c.cuda(), rows_c.cuda()
    target = rows[:, 6:]
    assert rgb.stride(0) == 3 and target.stride(0) == 9 and rgb.shape[0] == B + PAD
    work = torch.empty(lib.r2l_pool_select_work_bytes(B), dtype=torch.uint8, device="cuda")
    for k in _ks(B):
        want_hard, want_err = _spec(B, pattern, k)
        hard = torch.empty(k, dtype=torch.int64, device="cuda")
        err = torch.empty(B, dtype=torch.float32, device="cuda")
        _call(lib, rgb, target, B, k, hard, err, work)
        assert torch.equal(hard.cpu(), want_hard), (B, pattern, k)
        (got, got_nan), (want, want_nan) = _bits(err.cpu()), _bits(want_err)
        assert torch.equal(got, want) and torch.equal(got_nan, want_nan), (B, pattern, k)
    if B <= 1025:  # the spec as its users call it, and the wrapper with its own scratch
        k = _ks(B)[len(_ks(B)) // 2]
        hard_np, _ = select_spec(rgb_c[:B], rows_c[:B, 6:], k)
        assert torch.equal(torch.from_numpy(hard_np), _spec(B, pattern, k)[0])
        assert torch.equal(select(rgb[:B], target[:B], k).cpu(), _spec(B, pattern, k)[0])


@pytest.mark.parametrize("B", (257, 4096, 12288, 12289, 81920))  # one workgroup (to 12 288 rows) and many
def test_select_memory_discipline(B):
    from r2l_amd import _lib
    lib = _lib.load()
    k, G = B // 5, 64
    rgb_c, rows_c = _inputs(B, "ties" if B % 2 else "uniform")
    rgb, rows = rgb_c.cuda(), rows_c.cuda()
    target = rows[:, 6:]
    want_hard, want_err = _spec(B, "ties" if B % 2 else "uniform", k)
    n_work = lib.r2l_pool_select_work_bytes(B)
    work = torch.zeros(n_work + 2 * G, dtype=torch.uint8, device="cuda")
    hard_buf = torch.full((k + 2 * G,), -7, dtype=torch.int64, device="cuda")
    err_buf = torch.full((B + 2 * G,), -7., dtype=torch.float32, device="cuda")
    hard, err = hard_buf[G:G + k], err_buf[G:G + B]
    outs = []
    for fill in (0x00, 0x00, 0xFF):  # twice alike, then with a work area full of 0xFF bytes: it is written before it is read
        work.fill_(fill)
        hard.fill_(-1)
        err.fill_(-1.)
        _call(lib, rgb, target, B, k, hard, err, work[G:])
        outs.append((hard.cpu().clone(), err.cpu().clone()))
        assert torch.equal(outs[-1][0], want_hard) and torch.equal(outs[-1][1], want_err)
    assert int((work[:G] != 0xFF).sum()) == 0 and int((work[G + n_work:] != 0xFF).sum()) == 0  # nothing outside the stated bytes
    # guard elements in front of and behind both outputs keep their poison
    for buf, n in ((hard_buf, k), (err_buf, B)):
        assert int((buf[:G] != -7).sum()) == 0 and int((buf[G + n:] != -7).sum()) == 0
    # err_out is optional
    hard.fill_(-1)
    _call(lib, rgb, target, B, k, hard, None, work[G:])
    assert torch.equal(hard.cpu(), want_hard)


def test_pool_simulation():
    """HardRayPool(device_select=True) against a numpy pool built from select_spec and raystore.perm_at, after every update."""
    from r2l_amd.driver import HardRayPool
    from r2l_amd.pool_select import select_spec
    from r2l_amd.raystore import perm_at
    B, seed = 128, 3
    pool = HardRayPool(0.25, 0.5, seed=seed, device_select=True)
    sim, n_sim, full, draws = np.zeros((64, 9), np.float32), 0, False, 0
    g = torch.Generator().manual_seed(11)
    for it in range(12):
        o, d, t = (torch.rand(B, 3, generator=g) for _ in range(3))
        o2, d2, t2 = pool.augment(o.cuda(), d.cuda(), t.cuda())
        rows = torch.cat([o, d, t], 1).numpy()
        if full:
            draws += 1
            key = (seed * 0x9E3779B97F4A7C15 + draws * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF
            ix = perm_at(key, 64, np.arange(32, dtype=np.uint64))
            rows = np.concatenate([rows, sim[ix]], 0)
        assert o2.shape[0] == rows.shape[0] == (160 if it >= 2 else 128)
        assert np.array_equal(torch.cat([o2, d2, t2], 1).cpu().numpy(), rows)
        rgb = torch.rand(rows.shape[0], 3, generator=g)
        pool.update(rgb.cuda(), o2, d2, t2, B)
        hard, _ = select_spec(rgb.numpy()[:B], rows[:B, 6:], 32)
        if full:
            sim[ix[:32]] = rows[hard]
        else:
            sim[n_sim:n_sim + 32] = rows[hard]
            n_sim += 32
            full = n_sim >= 64
        assert pool.full == full and np.array_equal(pool.pool.cpu().numpy(), sim[:n_sim]), it
    assert pool._draws == draws == 10


def test_c_abi_only_iterations():
    """Three training iterations made of library calls alone — r2l_store_batch, r2l_pool_pick, r2l_pool_augment, r2l_draw_uniform,
    the packs, forward, backward, r2l_loss_finish, r2l_adam_step, r2l_pool_select, r2l_pool_store; torch only owns the memory and
    zeroes the gradient — against R2LTrainer + HardRayPool(device_select=True) + RayStore on the same seeds: parameters, moments
    and pool bit for bit.  2 shards of 64 rays per step; the pool is full after two updates, so iteration 3 augments."""
    from model.nerf_raybased import PointSampler
    from r2l_amd import _lib, render
    from r2l_amd.driver import HardRayPool
    from r2l_amd.raystore import RayStore
    from r2l_amd.train_step import R2LTrainer
    lib = _lib.load()
    nb, B, RPS, seed, pool_seed, jitter_seed, lr = 2, 128, 64, 5, 1000, 7, 5e-4
    sd = O.make_state_dict(n_block=nb, seed=3)
    rng = np.random.RandomState(2)
    o = rng.randn(6 * RPS, 3).astype(np.float32)
    o *= 4. / np.linalg.norm(o, axis=1, keepdims=True)
    d = (-o / 4. + 0.2 * rng.randn(6 * RPS, 3)).astype(np.float32)
    rows = torch.from_numpy(np.concatenate([o, d, rng.rand(6 * RPS, 3).astype(np.float32)], 1)).cuda()
    ps = PointSampler(400, 400, 555.5555155968841, 16, 2., 6.)

    # ---- the Python classes -------------------------------------------------------------------------------------------------
    store = RayStore(6, "cuda", rays_per_shard=RPS, seed=seed)
    assert store.append(rows, 0, shuffle=False) == 6
    model = build_model(sd, nb)
    tr = R2LTrainer(model, ps)
    tr.eng.set_config(precision="fp32_mfma")
    pool = HardRayPool(0.25, 0.5, seed=pool_seed, device_select=True)
    for it in (1, 2, 3):
        batch = store.next(2)
        ro, rd, tg = pool.augment(batch[:, :3], batch[:, 3:6], batch[:, 6:9])
        n = ro.shape[0]
        t_rand = render.draw_uniform(n * 16, jitter_seed, 2**61 + it * 4096, "cuda").view(n, 16)
        rgb, _ = tr.step(ro, rd, tg, lr, perturb=1., t_rand=t_rand)
        pool.update(rgb, ro, rd, tg, B)
    assert pool.full and pool._draws == 1 and tr.step_count == 3

    # ---- the same through the C ABI -----------------------------------------------------------------------------------------
    cfg = _lib.make_config(precision="fp32_mfma")
    cref = ctypes.byref(cfg)
    f = dict(dtype=torch.float32, device="cuda")
    flat = torch.cat([p.detach().reshape(-1) for p in build_model(sd, nb).parameters()]).float().cuda().contiguous()
    n_param = flat.numel()
    assert n_param == lib.r2l_param_count(nb)
    wf = torch.zeros(lib.r2l_fwd_stream_floats(nb), **f)
    wb = torch.zeros(lib.r2l_bwd_stream_floats(nb), **f)
    grads, m, v = (torch.zeros(n_param, **f) for _ in range(3))
    n_max = B + 32
    slot = int(lib.r2l_stash_slot_floats(n_max))
    save_x, gx = (torch.empty((nb + 1) * slot, **f) for _ in range(2))
    save_t, gt = (torch.empty(nb * slot, **f) for _ in range(2))
    dpre = torch.empty(n_max * 3, **f)
    sqerr = torch.empty(int(lib.r2l_num_tiles(n_max)), **f)
    slab = torch.empty(int(lib.r2l_dw_slab_floats()), **f)
    loss = torch.zeros(2, **f)
    z = ps.z_vals.detach().float().cpu().reshape(-1)
    mids = .5 * (z[1:] + z[:-1])
    lower, upper = torch.cat([z[:1], mids]), torch.cat([mids, z[-1:]])
    ztab = torch.cat([lower, upper - lower]).cuda().contiguous()
    data = store.data  # the filled store: caller-owned memory, read through r2l_store_batch below
    pool_rows = torch.zeros(64, 9, **f)
    work = torch.empty(lib.r2l_pool_select_work_bytes(B), dtype=torch.uint8, device="cuda")
    ix = torch.empty(32, dtype=torch.int64, device="cuda")
    hard = torch.empty(32, dtype=torch.int64, device="cuda")
    draw, n_pool, full, draws = 0, 0, False, 0
    ck = _lib.check
    for it in (1, 2, 3):
        s = _stream()
        batch = torch.empty(B, 9, **f)
        ck(lib.r2l_store_batch(_p(data), 6, RPS, draw, 2, seed, _p(batch), None, s), "r2l_store_batch")
        draw += 2
        n_out = 32 if full else 0
        if full:
            draws += 1
            key = (pool_seed * 0x9E3779B97F4A7C15 + draws * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF
            ck(lib.r2l_pool_pick(_p(ix), 32, 64, key, s), "r2l_pool_pick")
        n = B + n_out
        odt = torch.empty(3, n, 3, **f)  # (with n_out == 0 the augment is the copy of the column slices to contiguous rows)
        ck(lib.r2l_pool_augment(_p(batch[:, :3]), _p(batch[:, 3:6]), _p(batch[:, 6:9]), 9, 9, 9, _p(pool_rows) if full else None,
                                _p(ix) if full else None, B, n_out, _p(odt[0]), _p(odt[1]), _p(odt[2]), s), "r2l_pool_augment")
        t_rand = torch.empty(n * 16, **f)
        ck(lib.r2l_draw_uniform(_p(t_rand), n * 16, jitter_seed, 2**61 + it * 4096, s), "r2l_draw_uniform")
        ck(lib.r2l_pack_forward_layout(_p(flat), nb, _p(wf), lib.r2l_forward_layout_for_cfg(n, 1, cref), s), "pack forward")
        ck(lib.r2l_pack_backward_layout(_p(flat), nb, _p(wb), lib.r2l_backward_layout_for_cfg(n, cref), s), "pack backward")
        rgb = torch.empty(n, 3, **f)
        ck(lib.r2l_forward_rays_cfg(_p(odt[0]), _p(odt[1]), _p(t_rand), _p(ztab), _p(wf), _p(flat), nb, _p(rgb), _p(save_x),
                                    _p(save_t), n, s, cref), "r2l_forward_rays_cfg")
        grads.zero_()
        ck(lib.r2l_backward_part_cfg(_p(odt[0]), _p(odt[1]), _p(t_rand), _p(ztab), None, _p(rgb), _p(odt[2]), None, _p(save_x),
                                     _p(save_t), _p(wb), _p(flat), nb, 2.0 / (3.0 * n), _p(dpre), _p(gx), _p(gt), _p(sqerr),
                                     _p(grads), _p(slab), n, s, _lib.BWD_ALL, 0, 2 * nb, cref), "r2l_backward_part_cfg")
        ck(lib.r2l_loss_finish(_p(sqerr), int(lib.r2l_num_tiles(n)), 1.0 / (3.0 * n), _p(loss), s), "r2l_loss_finish")
        ck(lib.r2l_adam_step(_p(flat), _p(grads), _p(m), _p(v), n_param, lr, 0.9, 0.999, 1e-8, it, 1.0, s), "r2l_adam_step")
        ck(lib.r2l_pool_select(_p(rgb), _p(odt[2]), 3, 3, B, 32, _p(hard), None, _p(work), s), "r2l_pool_select")
        ck(lib.r2l_pool_store(_p(odt[0]), _p(odt[1]), _p(odt[2]), 3, 3, 3, _p(hard), _p(pool_rows), _p(ix) if full else None,
                              0 if full else n_pool, 32, s), "r2l_pool_store")
        if not full:
            n_pool += 32
            full = n_pool >= 64
    torch.cuda.synchronize()
    assert torch.equal(loss, tr.loss_out)
    assert torch.equal(flat, tr.eng.flat) and torch.equal(m, tr.exp_avg) and torch.equal(v, tr.exp_avg_sq)
    assert torch.equal(pool_rows, pool.pool) and draw == store.draw


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------
def _ray_rows(n, seed):
    rng = np.random.RandomState(seed)  # origins on the r = 4 sphere, inward directions, colours in [0, 1)
    o = rng.randn(n, 3).astype(np.float32)
    o *= 4. / np.linalg.norm(o, axis=1, keepdims=True)
    d = (-o / 4. + 0.2 * rng.randn(n, 3)).astype(np.float32)
    return np.concatenate([o, d, rng.rand(n, 3).astype(np.float32)], 1)


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    """A tiny synthetic scene (64 x 64 test views) and ten shard files of 64 rays."""
    from r2l_amd import data
    root = tmp_path_factory.mktemp("pool_select")
    scene, kd = str(root / "scene"), str(root / "pseudo")
    os.makedirs(scene)
    os.makedirs(kd)
    make_scene(scene, size=128)
    assert data.write_ray_shards(_ray_rows(10 * 64, 9), kd, 0, rays_per_file=64) == 10
    return {"scene": scene, "kd": kd}


def _student(tiny, name):
    return ["--model_name", "R2L", "--config", os.path.join(ROOT, "configs", "lego_noview.txt"), "--datadir", tiny["scene"],
            "--n_sample_per_ray", "16", "--netwidth", "256", "--netdepth", "6", "--use_residual", "--trial.ON", "--trial.body_arch",
            "resmlp", "--testskip", "1", "--datadir_kd", tiny["kd"], "--data_mode", "rays", "--r2l_device_store", "--r2l_device_pool",
            "--N_rand", "2", "--hard_ratio", "0.25", "--hard_mul", "0.5", "--warmup_lr", "0.0001,200", "--i_print", "1",
            "--experiment_name", name]


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return torch.equal(a.cpu(), b.cpu())
    return a == b


def _ckpt_equal(a, b):
    """network_fn_state_dict, every Adam moment and the pool of two checkpoints: (weights and moments equal, pool equal)."""
    net = all(torch.equal(a["network_fn_state_dict"][k].cpu(), b["network_fn_state_dict"][k].cpu()) for k in a["network_fn_state_dict"])
    sa, sb = a["optimizer_state_dict"]["state"], b["optimizer_state_dict"]["state"]
    mom = sorted(sa) == sorted(sb) and all(torch.equal(sa[i][q].cpu(), sb[i][q].cpu()) for i in sa for q in ("exp_avg", "exp_avg_sq"))
    pa, pb = a["r2l_hard_pool"], b["r2l_hard_pool"]
    return net and mom, sorted(pa) == sorted(pb) and all(_same(pa[k], pb[k]) for k in pa)


@pytest.mark.parametrize("precision", ("fp32_mfma", "auto"))
def test_cli_resume_bit_for_bit(tiny, tmp_path, monkeypatch, precision):
    from r2l_amd import driver
    from r2l_amd.checkpoint import load_ckpt
    monkeypatch.chdir(tmp_path)
    extra = ["--r2l_precision", precision, "--i_weights", "3", "--save_intermediate_models", "--N_iters", "6"]
    a = driver.main(_student(tiny, "A") + extra)
    wa = a["logger"].weights_path
    assert sorted(os.listdir(wa)) == ["ckpt_3.tar", "ckpt_6.tar"]
    ck3, ck6 = load_ckpt(os.path.join(wa, "ckpt_3.tar")), load_ckpt(os.path.join(wa, "ckpt_6.tar"))
    # the pool is full at iteration 2: the checkpoint of iteration 3 holds a full pool and one keyed pick
    st = ck3["r2l_hard_pool"]
    assert st["full"] and st["n"] == 64 and st["rows"].shape == (64, 9) and st["draws"] == 1 and st["batch_size"] == 128
    assert (st["hard_ratio"], st["hard_mul"]) == (0.25, 0.5) and ck6["r2l_hard_pool"]["draws"] == 4
    b = driver.main(_student(tiny, "B") + extra + ["--pretrained_ckpt", os.path.join(wa, "ckpt_3.tar"), "--resume"])
    log = open(os.path.join(b["logger"].log_path, "log.txt")).read()
    assert "hard-ray pool: resumed with 64 rows (full: True, draw counter 1)" in log and "resuming at draw 6" in log
    assert [l.split("[TRAIN] Iter ")[1].split()[0] for l in log.splitlines() if "[TRAIN] Iter" in l] == ["4", "5", "6"]
    assert _ckpt_equal(ck6, load_ckpt(os.path.join(b["logger"].weights_path, "ckpt_6.tar"))) == (True, True)
    # the state is used: the same resume from a copy of the checkpoint WITHOUT the pool is another run
    bare = dict(ck3)
    del bare["r2l_hard_pool"]
    torch.save(bare, str(tmp_path / "bare_3.tar"))
    c = driver.main(_student(tiny, "C") + extra + ["--pretrained_ckpt", str(tmp_path / "bare_3.tar"), "--resume"])
    assert "hard-ray pool: the checkpoint carries none" in open(os.path.join(c["logger"].log_path, "log.txt")).read()
    assert _ckpt_equal(ck6, load_ckpt(os.path.join(c["logger"].weights_path, "ckpt_6.tar"))) == (False, False)


def test_cli_two_ranks(tiny, tmp_path):
    """Two ranks on this one GPU over gloo, four iterations with the switch: the replicas end in sync (the run checks them itself),
    the pools are not saved, and the two ranks draw their jitter from different streams."""
    from r2l_amd import render
    from r2l_amd.checkpoint import load_ckpt
    env = {k: v for k, v in os.environ.items() if not k.startswith("R2L_")}
    env.update(MASTER_ADDR="127.0.0.1", R2L_DIST_BACKEND="gloo", R2L_CHECK_SYNC="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29653", os.path.join(ROOT, "main.py")] + _student(tiny, "dp2") + ["--i_weights", "4", "--N_iters", "4"]
    r = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "replicas in sync after 4 iterations: True (skipped steps: 0)" in out
    assert "Philox stream 2^61 + 4096 * iteration + 0 of seed 0" in out
    ckpts = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp_path) for f in fs if f == "ckpt.tar"]
    assert len(ckpts) == 1
    ck = load_ckpt(ckpts[0])
    assert ck["global_step"] == 4 and "r2l_hard_pool" not in ck
    t0, t1 = (render.draw_uniform(160 * 16, 0, 2**61 + 3 * 4096 + rank, "cuda") for rank in (0, 1))
    assert not torch.equal(t0, t1) and float((t0 == t1).float().mean()) < 0.01
    assert torch.equal(t0, render.draw_uniform(160 * 16, 0, 2**61 + 3 * 4096, "cuda"))
