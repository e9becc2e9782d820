"""The fused student iteration on the GPU (include/r2l_hip.h r2l_train_batch / r2l_student_train_step; R2LTrainer.fused_step;
main.py --r2l_fused_iter): the batch kernel against the three calls it replaces, the one-call iteration against the staged loop —
RayStore.next -> HardRayPool.augment -> draw_uniform -> R2LTrainer.step -> HardRayPool.update — bit for bit in every kernel family,
its statelessness, the pack rule, a step that leaves fp16's range, the refusals of the descriptor, the CLI, and the C99 host.
All models are W256 with two blocks."""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from oracle import r2l_oracle as O
from tests.test_driver_cpu import ROOT
from tests.test_forward_gpu import build_model
from tests.test_pool_select_gpu import _ckpt_equal, _student, tiny  # noqa: F401  (tiny: the CLI tests' scene and shard files)
from tests.test_train_gpu import FAMILIES

pytestmark = pytest.mark.gpu

NB = 2
SEED, POOL_SEED, JITTER_SEED, LR = 0xC0FFEE123, 1000, 7, 3e-4
SENTINEL = -777.0


@pytest.fixture(autouse=True)
def _auto_family(monkeypatch):
    from tests.conftest import use_family
    use_family(monkeypatch)  # AUTO fields, no R2L_* switch from the environment; the family tests select theirs on top


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(a, b):
    """Same bits (a NaN equals itself)."""
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _ray_rows(n, seed):
    rng = np.random.RandomState(seed)  # origins on the r = 4 sphere, inward directions, colours in [0, 1)
    o = rng.randn(n, 3).astype(np.float32)
    o *= 4. / np.linalg.norm(o, axis=1, keepdims=True)
    d = (-o / 4. + 0.2 * rng.randn(n, 3)).astype(np.float32)
    return np.concatenate([o, d, rng.rand(n, 3).astype(np.float32)], 1)


def _ps():
    from model.nerf_raybased import PointSampler
    return PointSampler(400, 400, 555.5555155968841, 16, 2., 6.)


# ---- 1. r2l_train_batch against r2l_store_batch + r2l_pool_pick + r2l_pool_augment ------------------------------------------------
G = 64  # guard floats on either side of every output (a multiple of 4: the outputs stay 16-byte aligned)


def _guarded(n, dtype=torch.float32):
    big = torch.full((n + 2 * G,), SENTINEL if dtype == torch.float32 else -777, dtype=dtype, device="cuda")
    return big, big[G:G + n]


def _guards_intact(big, n):
    ref = SENTINEL if big.dtype == torch.float32 else -777
    return bool((big[:G] == ref).all()) and bool((big[G + n:] == ref).all())


@pytest.mark.parametrize("rps", (4, 12, 4096))
def test_train_batch_equals_the_three_calls(rps):
    """rays_per_shard x n_shards {1, 3, 7} x n_draw {1, 3} (draw0 = n_shards - 1: the step straddles an epoch) x n_out {0, 1, 5} from
    pools of 1, 6 and 4097 rows: outputs, ids_out and idx_out bit for bit, the numpy restatement too, guard bands untouched."""
    from r2l_amd import _lib, raystore
    lib = _lib.load()
    store_np = _ray_rows(7 * rps, rps)
    store = torch.from_numpy(store_np).cuda()
    pools = {n: torch.from_numpy(_ray_rows(n, 100 + n)).cuda() for n in (1, 6, 4097)}
    seed, key = 0x1234ABCD5678, 0xFEDCBA9876543210
    for n_shards in (1, 3, 7):
        for n_draw in (1, 3):
            draw0, B = n_shards - 1, n_draw * rps
            for n_pool, pool in pools.items():
                for n_out in (k for k in (0, 1, 5) if k <= n_pool):
                    what = (rps, n_shards, n_draw, n_pool, n_out)
                    # the three calls
                    batch = torch.empty(B, 9, dtype=torch.float32, device="cuda")
                    ids = torch.empty(n_draw, dtype=torch.int32, device="cuda")
                    _lib.check(lib.r2l_store_batch(_p(store), n_shards, rps, draw0, n_draw, seed, _p(batch), _p(ids), _stream()), "batch")
                    ix = torch.empty(max(n_out, 1), dtype=torch.int64, device="cuda")
                    _lib.check(lib.r2l_pool_pick(_p(ix), n_out, n_pool, key, _stream()), "pick")
                    want = torch.empty(3, B + n_out, 3, dtype=torch.float32, device="cuda")
                    _lib.check(lib.r2l_pool_augment(_p(batch[:, :3]), _p(batch[:, 3:6]), _p(batch[:, 6:9]), 9, 9, 9, _p(pool), _p(ix), B,
                                                    n_out, _p(want[0]), _p(want[1]), _p(want[2]), _stream()), "augment")
                    # the one call
                    outs = [_guarded((B + n_out) * 3) for _ in range(3)]
                    ids_big, ids2 = _guarded(n_draw, torch.int32)
                    ix_big, ix2 = _guarded(n_out, torch.int64)
                    _lib.check(lib.r2l_train_batch(_p(store), n_shards, rps, draw0, n_draw, seed, _p(pool), n_pool, n_out, key,
                                                   _p(outs[0][1]), _p(outs[1][1]), _p(outs[2][1]), _p(ids2), _p(ix2) if n_out else None,
                                                   _stream()), "r2l_train_batch")
                    for c in range(3):
                        assert _bits(outs[c][1].view(-1, 3), want[c]), (what, c)
                        assert _guards_intact(outs[c][0], (B + n_out) * 3), (what, c)
                    assert torch.equal(ids2, ids) and torch.equal(ix2, ix[:n_out]), what
                    assert _guards_intact(ids_big, n_draw) and _guards_intact(ix_big, n_out), what
                    o, d, t, ids_np, idx_np = raystore.train_batch_spec(store_np, n_shards, rps, draw0, n_draw, seed, pool.cpu().numpy(),
                                                                        n_pool, n_out, key)
                    assert np.array_equal(outs[0][1].view(-1, 3).cpu().numpy(), o) and np.array_equal(outs[2][1].view(-1, 3).cpu().numpy(), t)
                    assert np.array_equal(outs[1][1].view(-1, 3).cpu().numpy(), d)
                    assert np.array_equal(ids2.cpu().numpy(), ids_np) and np.array_equal(ix2.cpu().numpy(), idx_np), what
    # n_out == 0 needs neither a pool nor idx_out; ids_out may be NULL
    out = torch.empty(3, rps, 3, dtype=torch.float32, device="cuda")
    _lib.check(lib.r2l_train_batch(_p(store), 7, rps, 0, 1, seed, None, 0, 0, 0, _p(out[0]), _p(out[1]), _p(out[2]), None, None, _stream()),
               "r2l_train_batch")
    sid = int(raystore.shard_ids(seed, 7, 0, 1)[0])
    assert _bits(out[0], store[sid * rps:(sid + 1) * rps, :3])
    assert lib.r2l_train_batch(_p(store), 7, rps, 0, 1, seed, _p(pools[6]), 6, 2, key, _p(out[0]), _p(out[1]), _p(out[2]), None, None,
                               _stream()) != 0 and b"idx_out" in lib.r2l_last_error()


# ---- 2 - 5. the fused iteration against the staged loop -----------------------------------------------------------------------------
CASES = {
    # rays_per_shard, n_shards, n_draw, (hard_ratio, hard_mul) or None, perturb
    "A": (12, 5, 3, (0.25, 0.5), 1.),    # B = 36 (one 32-ray tile + 4); n_in = 9: full after 2 steps, N = 45 from iteration 3 on
    "B": (4096, 3, 1, (0.2, 2.), 0.),    # n_in = 819, the pool keeps filling
    "C": (4, 7, 17, None, 1.),           # no pool; B = 68 (two tiles + 4), 17 draws per step over 7 shards
}


class Loop:
    """One training loop — model, trainer, store, pool — that runs either form of the iteration."""

    def __init__(self, case, fused, sd=None, calibrate=True, rows=None):
        from r2l_amd.driver import HardRayPool
        from r2l_amd.raystore import RayStore
        from r2l_amd.train_step import R2LTrainer
        rps, n_shards, self.n_draw, hard, self.perturb = CASES[case] if isinstance(case, str) else case
        self.fused, self.ps = fused, _ps()
        self.tr = R2LTrainer(build_model(sd if sd is not None else O.make_state_dict(n_block=NB, seed=9), NB), self.ps)
        self.tr.calibrate = calibrate
        self.store = RayStore(n_shards, "cuda", rays_per_shard=rps, seed=SEED)
        rows = rows if rows is not None else torch.from_numpy(_ray_rows(n_shards * rps, 31)).cuda()
        assert self.store.append(rows, 0, shuffle=False) == n_shards
        self.pool = HardRayPool(hard[0], hard[1], seed=POOL_SEED, device_select=True) if hard else None
        self.rgb = None

    def step(self, it):
        from r2l_amd import render
        tr, pool = self.tr, self.pool
        if self.fused:
            self.rgb, _ = tr.fused_step(self.store, pool, LR, it, perturb=self.perturb, seed=JITTER_SEED, n_files=self.n_draw)
            return
        batch = self.store.next(self.n_draw)
        ro, rd, tg = batch[:, :3], batch[:, 3:6], batch[:, 6:9]
        B = ro.shape[0]
        if pool is not None:
            ro, rd, tg = pool.augment(ro, rd, tg)
        n = ro.shape[0]
        t_rand = render.draw_uniform(n * 16, JITTER_SEED, 2**61 + it * 4096, "cuda").view(n, 16) if self.perturb > 0 else None
        self.rgb, _ = tr.step(ro, rd, tg, LR, perturb=self.perturb, t_rand=t_rand)
        if pool is not None:
            pool.update(self.rgb, ro, rd, tg, B)

    def render(self):
        """A forward-only launch between two iterations (what a test-set render does to the weight streams)."""
        rows = torch.from_numpy(_ray_rows(100, 77)).cuda()
        return self.tr.eng.forward_rays(rows[:, :3], rows[:, 3:6], self.ps.z_vals, 0., None).clone()

    def state(self):
        tr, pool = self.tr, self.pool
        s = {"params": tr.eng.flat, "exp_avg": tr.exp_avg, "exp_avg_sq": tr.exp_avg_sq, "grads": tr.grads, "wstream": tr.eng.wstream,
             "wstream_bwd": tr.wstream_bwd, "loss_out": tr.loss_out, "rgb": self.rgb,
             "pool_rows": pool.pool if pool is not None else None}
        s = {k: (v.clone() if v is not None else None) for k, v in s.items()}
        s["fill"] = (pool._n, pool.full, pool._draws) if pool is not None and pool._store is not None else None
        s["counters"] = (self.store.draw, tr.step_count)
        return s


def _same_state(a, b, what):
    for k in a:
        if k in ("fill", "counters"):
            assert a[k] == b[k], (what, k, a[k], b[k])
        else:
            assert _bits(a[k], b[k]), (what, k)


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("family", list(FAMILIES))
def test_fused_iteration_equals_the_staged_loop(monkeypatch, family, case):
    """Five iterations in each form; after every one: parameters, both moments, gradients, both weight streams (their range-control
    words included), loss_out, rgb, the pool's filled rows and fill state, the store's draw counter — the same bits."""
    from tests.conftest import use_family
    use_family(monkeypatch, **FAMILIES[family])
    staged, fused = Loop(case, False), Loop(case, True)
    for it in range(1, 6):
        staged.step(it)
        fused.step(it)
        _same_state(staged.state(), fused.state(), (family, case, it))
    if case == "A":
        assert staged.rgb.shape[0] == 45 and fused.pool.full and fused.pool._draws == 3 and fused.pool.pool.shape[0] == 18
    if case == "B":
        assert fused.pool.pool.shape[0] == 5 * 819 and not fused.pool.full
    if case == "C":
        assert fused.rgb.shape[0] == 68 and fused.store.draw == 85


def test_fused_iteration_is_stateless():
    """Iteration 4 from FRESH buffers — a new trainer (new work buffer), store and pool — loaded with the state after iteration 3
    equals iteration 4 of the uninterrupted run."""
    run = Loop("A", True)
    for it in (1, 2, 3):
        run.step(it)
    at3, pool3 = run.state(), run.pool.state_dict()
    run.step(4)
    want = run.state()

    fresh = Loop("A", True, calibrate=False)
    tr = fresh.tr
    with torch.no_grad():
        tr.eng.flat.copy_(at3["params"])
    tr.eng.mark_dirty()
    tr.exp_avg.copy_(at3["exp_avg"])
    tr.exp_avg_sq.copy_(at3["exp_avg_sq"])
    tr.eng.wstream.copy_(at3["wstream"])  # (stale weights, but the status words in them carry the range history)
    tr.wstream_bwd.copy_(at3["wstream_bwd"])
    tr.step_count = 3
    fresh.store.seek(at3["counters"][0])
    fresh.pool.load_state_dict(pool3, device="cuda", batch_size=36)
    fresh.step(4)
    _same_state(want, fresh.state(), "fresh buffers")


def test_a_render_between_iterations_changes_nothing():
    """A forward-only render between iterations 2 and 3 re-packs the forward stream from the updated parameters; iteration 3 must
    then pack what the staged trainer's version check packs and no more (the pack flag mirrors that check)."""
    staged, fused = Loop("A", False), Loop("A", True)
    for it in range(1, 6):
        if it == 3:
            assert _bits(staged.render(), fused.render())
        staged.step(it)
        fused.step(it)
        _same_state(staged.state(), fused.state(), ("render", it))


def test_fp16_range_case_agrees():
    """The out-of-range network of tests/test_train_gpu.py::test_fp16_range_control_in_training (head x 3e4, tail x 1e-5), uncalibrated:
    the first step is redone by the bf16x3 kernels inside the forward and backward entry points — the same in both forms, and the
    fallback counters agree."""
    sd = {k: v.clone() for k, v in O.make_state_dict(n_block=NB, seed=4).items()}
    sd["head.0.weight"] *= 3.0e4
    sd["head.0.bias"] *= 3.0e4
    for k in sd:
        if k.startswith("tail."):
            sd[k] = sd[k] * 1.0e-5
    gen = torch.Generator().manual_seed(21)
    n = 600
    rows = torch.cat([torch.randn(n, 3, generator=gen) * 1.5, torch.randn(n, 3, generator=gen), torch.rand(n, 3, generator=gen)], 1).cuda()
    loops = [Loop((600, 1, 1, None, 0.), fused, sd=sd, calibrate=False, rows=rows) for fused in (False, True)]
    for it in (1, 2):
        for lp in loops:
            lp.step(it)
        _same_state(loops[0].state(), loops[1].state(), ("range", it))
        a, b = loops[0].tr.range_info(), loops[1].tr.range_info()
        assert a == b, (it, a, b)
        assert a["trips"] >= 1 and a["bwd_trips"] >= 1 and a["scale"] >= 4, a  # the fallback did run


# ---- 6. the descriptor's refusals -------------------------------------------------------------------------------------------------------
def _valid_call():
    """A valid first step of case A at the C ABI: (descriptor keywords, {name: tensor} of every buffer in call order)."""
    from r2l_amd import _lib
    lib = _lib.load()
    f = dict(dtype=torch.float32, device="cuda")
    n_param = int(lib.r2l_param_count(NB))
    sd = O.make_state_dict(n_block=NB, seed=9)
    params = torch.cat([p.detach().reshape(-1) for p in build_model(sd, NB).parameters()]).float().cuda().contiguous()
    assert params.numel() == n_param
    z = _ps().z_vals.detach().float().cpu().reshape(-1)
    mids = .5 * (z[1:] + z[:-1])
    lower, upper = torch.cat([z[:1], mids]), torch.cat([mids, z[-1:]])
    kw = dict(n_block=NB, perturb=1, pack=1, pool_full=0, rays_per_shard=12, n_shards=5, n_draw=3, draw0=4, store_seed=SEED,
              pool_capacity_rows=18, pool_rows=0, n_in=9, n_out=9, pool_key=0, seed=JITTER_SEED, jitter_stream=2**61 + 4096, lw_rgb=1.0,
              lr=LR, beta1=0.9, beta2=0.999, eps=1e-8, step=1)
    bufs = {"store": torch.from_numpy(_ray_rows(60, 31)).cuda(), "pool": torch.full((18, 9), SENTINEL, **f),
            "ztab": torch.cat([lower, upper - lower]).cuda().contiguous(), "params": params, "grads": torch.full((n_param,), SENTINEL, **f),
            "exp_avg": torch.zeros(n_param, **f), "exp_avg_sq": torch.zeros(n_param, **f),
            "wstream": torch.zeros(lib.r2l_fwd_stream_floats(NB), **f), "wstream_bwd": torch.zeros(lib.r2l_bwd_stream_floats(NB), **f),
            "loss_out": torch.full((2,), SENTINEL, **f), "rgb_out": torch.full((36, 3), SENTINEL, **f)}
    return lib, kw, bufs


BAD_FIELDS = [
    (dict(n_block=-1), "n_block"), (dict(rays_per_shard=0), "rays_per_shard"), (dict(rays_per_shard=10), "rays_per_shard"),
    (dict(rays_per_shard=-4), "rays_per_shard"), (dict(n_shards=0), "n_shards"), (dict(n_draw=0), "n_draw"), (dict(draw0=-1), "draw0"),
    (dict(perturb=2), "perturb"), (dict(perturb=-1), "perturb"), (dict(pack=2), "pack"), (dict(pool_full=2), "pool_full"),
    (dict(n_in=9, n_out=8), "n_in"), (dict(n_in=37, n_out=37, pool_capacity_rows=100), "n_in"), (dict(pool_rows=10), "pool_rows"),
    (dict(pool_full=1, pool_rows=8), "n_out"), (dict(step=0), "step"), (dict(reserved=(0, 0, 1, 0)), "reserved"),
]


def test_invalid_descriptors_fail_before_any_launch():
    from r2l_amd import _lib
    lib, kw, bufs = _valid_call()
    need = int(lib.r2l_student_step_work_floats(ctypes.byref(_lib.StudentStepDesc(**kw))))
    assert need > 0
    GUARD = 4096
    work = torch.full((need + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    before = {k: v.clone() for k, v in bufs.items()}

    def call(desc, ptrs, work_ptr):
        return lib.r2l_student_train_step(ctypes.byref(desc), *[ptrs[k] for k in bufs], work_ptr, _stream())

    def untouched(what):
        for k in bufs:
            assert _bits(bufs[k], before[k]), (what, k)
        assert bool((work == SENTINEL).all()), what

    ptrs = {k: _p(v) for k, v in bufs.items()}
    for change, field in BAD_FIELDS:
        d = _lib.StudentStepDesc(**dict(kw, **change))
        assert lib.r2l_student_step_work_floats(ctypes.byref(d)) == -1 and field.encode() in lib.r2l_last_error(), change
        assert call(d, ptrs, _p(work)) == 1 and field.encode() in lib.r2l_last_error(), change  # hipErrorInvalidValue
        untouched(change)
    d = _lib.StudentStepDesc(**kw)
    for name in bufs:
        if name == "rgb_out":  # optional
            continue
        assert call(d, dict(ptrs, **{name: None}), _p(work)) == 1 and name.encode() in lib.r2l_last_error(), name
        untouched(name)
    assert call(d, ptrs, None) == 1 and b"work" in lib.r2l_last_error()
    assert call(d, ptrs, ctypes.c_void_p(work.data_ptr() + 4)) == 1 and b"16-byte aligned" in lib.r2l_last_error()
    untouched("work")
    bad_cfg = _lib.make_config()
    bad_cfg.dw_mode = 7
    d = _lib.StudentStepDesc(**dict(kw, cfg=ctypes.pointer(bad_cfg)))
    assert call(d, ptrs, _p(work)) == 1 and b"dw_mode" in lib.r2l_last_error()
    untouched("cfg")
    # the valid step: runs, and writes nothing past the queried size
    d = _lib.StudentStepDesc(**kw)
    _lib.check(call(d, ptrs, _p(work)), "r2l_student_train_step")
    torch.cuda.synchronize()
    assert bool((work[need:] == SENTINEL).all())
    loss = bufs["loss_out"].cpu()
    assert torch.isfinite(loss).all() and loss[0] > 0 and not _bits(bufs["params"], before["params"])
    assert bool((bufs["pool"][:9] != SENTINEL).all()) and bool((bufs["pool"][9:] == SENTINEL).all())  # nine hard rays appended
    assert not bool((bufs["rgb_out"] == SENTINEL).any())


# ---- 7. the CLI -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli_runs(tiny, tmp_path_factory):  # noqa: F811
    """Six iterations of the smallest student on the synthetic shards, without and with --r2l_fused_iter; checkpoints at 3 and 6."""
    from r2l_amd import driver
    cwd, work = os.getcwd(), tmp_path_factory.mktemp("fused_cli")
    os.chdir(str(work))
    try:
        extra = ["--i_weights", "3", "--save_intermediate_models", "--N_iters", "6"]
        a = driver.main(_student(tiny, "staged") + extra)
        b = driver.main(_student(tiny, "fused") + extra + ["--r2l_fused_iter"])
    finally:
        os.chdir(cwd)
    here = lambda path: os.path.join(str(work), path)  # (the logger's paths are relative to the directory of the run)
    return {"staged": here(a["logger"].weights_path), "fused": here(b["logger"].weights_path), "extra": extra,
            "logs": here(b["logger"].log_path)}


def test_cli_fused_iter_leaves_the_same_checkpoints(cli_runs):
    from r2l_amd.checkpoint import load_ckpt
    for name in ("ckpt_3.tar", "ckpt_6.tar"):
        a, b = load_ckpt(os.path.join(cli_runs["staged"], name)), load_ckpt(os.path.join(cli_runs["fused"], name))
        assert _ckpt_equal(a, b) == (True, True), name
        assert a["global_step"] == b["global_step"]
    st = load_ckpt(os.path.join(cli_runs["fused"], "ckpt_6.tar"))["r2l_hard_pool"]
    assert st["full"] and st["n"] == 64 and st["draws"] == 4
    log = open(os.path.join(cli_runs["logs"], "log.txt")).read()
    assert "Fused iteration (--r2l_fused_iter)" in log and log.count("[TRAIN] Iter") == 6


def test_cli_fused_iter_resumes_bit_for_bit(cli_runs, tiny, tmp_path, monkeypatch):  # noqa: F811
    from r2l_amd import driver
    from r2l_amd.checkpoint import load_ckpt
    monkeypatch.chdir(tmp_path)
    c = driver.main(_student(tiny, "fused_resume") + cli_runs["extra"] +
                    ["--r2l_fused_iter", "--pretrained_ckpt", os.path.join(cli_runs["fused"], "ckpt_3.tar"), "--resume"])
    log = open(os.path.join(c["logger"].log_path, "log.txt")).read()
    assert "resuming at draw 6" in log and "hard-ray pool: resumed with 64 rows" in log
    assert _ckpt_equal(load_ckpt(os.path.join(cli_runs["staged"], "ckpt_6.tar")),
                       load_ckpt(os.path.join(c["logger"].weights_path, "ckpt_6.tar"))) == (True, True)


# ---- 8. the C99 host ----------------------------------------------------------------------------------------------------------------------
def test_c99_training_host_ends_on_the_trainers_parameters(tmp_path):
    """tests/chost/train_host.c — C99, -pedantic -Werror, built the way tests/test_host_cpu.py builds host.c — runs four iterations
    of case A through r2l_student_train_step; R2LTrainer.fused_step on the same buffers ends on the same parameters and loss."""
    from r2l_amd import _lib
    assert shutil.which("gcc") is not None, "this test builds a C host: it needs gcc"
    lib = _lib.load()
    libdir = os.path.dirname(_lib.LIB_PATH)
    rocm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
    exe = str(tmp_path / "train_host")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "chost", "train_host.c"), "-o", exe, "-L", libdir, "-lr2l_hip", "-L", rocm, "-lamdhip64",
           "-Wl,-rpath," + libdir, "-Wl,-rpath," + rocm]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr

    run = Loop("A", True, calibrate=False)
    rps, n_shards, n_draw, (ratio, mul), perturb = CASES["A"]
    params0 = run.tr.eng.flat.detach().cpu().numpy().copy()
    ztab = run.tr.eng.ztab(run.ps.z_vals, perturb).cpu().numpy()
    store = run.store.data.cpu().numpy()
    assert params0.size == lib.r2l_param_count(NB) and ztab.size == 32 and store.shape == (n_shards * rps, 9)
    B = n_draw * rps
    n_in = int(ratio * B)
    header = [0x5232534c, NB, rps, n_shards, n_draw, SEED, 18, n_in, n_in, int(np.ceil(B * mul)), POOL_SEED, JITTER_SEED, int(perturb), 0, 0, 0]
    with open(str(tmp_path / "in.bin"), "wb") as f:
        f.write(struct.pack("<16q", *header) + struct.pack("<2d", LR, 1.0))
        f.write(params0.astype("<f4").tobytes() + ztab.astype("<f4").tobytes() + store.astype("<f4").tobytes())
    for it in (1, 2, 3, 4):
        run.step(it)
    want = run.tr.eng.flat.detach().cpu().numpy()
    want_loss = run.tr.loss_out.cpu().numpy()

    env = {k: v for k, v in os.environ.items() if not k.startswith("R2L_")}
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "C99 training host ok: 4 iterations" in r.stdout, r.stdout + r.stderr
    got = np.fromfile(str(tmp_path / "out.bin"), dtype="<f4")
    assert got.size == want.size + 2
    assert np.array_equal(got[:-2].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got[-2:].view(np.uint32), want_loss.view(np.uint32))
    assert not np.array_equal(want, params0)
