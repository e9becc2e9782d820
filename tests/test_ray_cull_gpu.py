"""Ray culling on the GPU (--r2l_ray_cull): r2l_occ_rays against its numpy restatement and against any() over r2l_occ_index,
r2l_store_append_live against gather + r2l_store_append, the culled student frames in every kernel family, the dead rays against
the teacher's unskipped frames, and the drivers."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import r2l_oracle as O
from r2l_amd import _lib
from r2l_amd import occupancy as OC
from r2l_amd import ray_cull as RC
from tests import ray_cull_util as RU
from tests.occupancy_util import same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cuda(*arrays):
    return [(a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(DEV).contiguous() for a in arrays]


# ---- 1. r2l_occ_rays --------------------------------------------------------------------------------------------------------------
GUARD = 64


def _occ_rays(grid, o, d, near, far, T, want_live=True):
    """r2l_occ_rays on caller-made buffers with sentinels behind their capacity: (M, idx[:M], live, the buffers)."""
    lib, p = _lib.load(), _lib.ptr
    R = o.shape[0]
    idx = torch.full((R + GUARD,), -3, dtype=torch.int64, device=DEV)
    live = torch.full((R + GUARD,), 9, dtype=torch.uint8, device=DEV)
    count = torch.full((1 + GUARD,), -5, dtype=torch.int64, device=DEV)
    nbytes = lib.r2l_occ_rays_work_bytes(R)
    work = torch.full((nbytes + GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    _lib.check(lib.r2l_occ_rays(ctypes.byref(grid.desc()), p(o), p(d), R, near, far, T, p(idx), p(count), p(live) if want_live else None,
                                p(work), _lib.stream()), "r2l_occ_rays")
    M = int(count[0].item())
    assert bool((idx[R:] == -3).all()) and bool((count[1:] == -5).all()) and bool((work[nbytes:] == 0xAB).all())
    assert bool((live[R:] == 9).all()) and (want_live or bool((live == 9).all()))
    assert bool((idx[M:R] == -3).all())  # entries at and past the count are not written
    return M, idx[:M].cpu().numpy(), live[:R].cpu().numpy()


def _any_over_index(grid, o, d, near, far, T):
    """any() over the EXISTING r2l_occ_index on z[r, j] = t_j built here."""
    R = o.shape[0]
    z = torch.from_numpy(np.broadcast_to(OC.ray_depths(near, far, T)[None], (R, T)).copy()).to(DEV)
    idx, count = grid.index(o, d, z)
    n = idx[:int(count.item())].cpu().numpy()
    live = np.zeros(R, np.uint8)
    live[np.unique(n // T)] = 1
    return live


@pytest.mark.parametrize("G,kind", [(G, kind) for G in (5, 8, 37) for kind in ("empty", "full", "random")])
def test_occ_rays_equals_the_spec_and_any_over_occ_index(G, kind):
    grid = RU.grid_with_bits(G, kind, device=DEV)
    checked = 0
    for R, T in [(1, 1), (63, 15), (64, 16), (65, 17), (257, 64), (2049, 200), (4097, 16), (4097, 1), (257, 15), (65, 200)]:
        on, dn = RU.cull_rays(R, G, seed=T)
        o, d = _cuda(on, dn)
        # (near 0: samples of the axis-parallel rays ON cell and box faces; near == far; near != 0 with dt != 0: the sum is rounded)
        for near, far in ((0., 2.), (.75, .75), (.3, 1.9)):
            M, idx, live = _occ_rays(grid, o, d, near, far, T)
            Ms, idxs, lives = RU.spec(grid, on, dn, near, far, T)
            assert M == Ms and np.array_equal(idx, idxs) and np.array_equal(live, lives), (R, T, near)
            assert np.array_equal(live, _any_over_index(grid, o, d, near, far, T)), (R, T, near)
            M2, idx2, _ = _occ_rays(grid, o, d, near, far, T, want_live=False)  # the flags in work; two calls, the same bits
            assert M2 == M and np.array_equal(idx2, idx)
            checked += 1
        if kind != "random":  # counts 0 and R: rays inside the box
            oi, di = RU.inside_rays(R)
            M, idx, live = _occ_rays(grid, *_cuda(oi, di), 0., 1., T)
            assert M == (R if kind == "full" else 0) and int(live.sum()) == M and np.array_equal(idx, np.arange(M))
    assert checked == 30


def test_occ_rays_r_zero_and_refusals_launch_nothing():
    assert RU.check_refusals() >= 35
    lib, p = _lib.load(), _lib.ptr
    grid = RU.grid_with_bits(5, "full", device=DEV)
    buf = torch.full((256,), 7.5, device=DEV)
    idx = torch.full((64,), -3, dtype=torch.int64, device=DEV)
    st = _lib.stream()
    g = ctypes.byref(grid.desc())
    assert lib.r2l_occ_rays(g, p(buf), p(buf), 4, 2., 6., 0, p(idx), p(idx), None, p(buf), st) == RU.INVALID  # T < 1
    assert lib.r2l_occ_rays(g, p(buf), p(buf), 4, 6., 2., 4, p(idx), p(idx), None, p(buf), st) == RU.INVALID  # far < near
    assert lib.r2l_occ_rays(g, p(buf), p(buf), -1, 2., 6., 4, p(idx), p(idx), None, p(buf), st) == RU.INVALID
    assert lib.r2l_occ_rays(g, p(buf), p(buf), 4, 2., 6., 4, p(idx), p(idx), None, ctypes.c_void_p(buf.data_ptr() + 2), st) == RU.INVALID
    m = ctypes.c_int64(-7)
    assert lib.r2l_store_append_live(p(buf), 4, None, 8, p(buf), 4, 0, 4, 1, 1, ctypes.byref(m), st) == RU.INVALID and m.value == -7
    assert lib.r2l_rgb_scatter_bg(p(buf), p(idx), 9, p(idx), 1., p(buf), 4, st) == RU.INVALID
    torch.cuda.synchronize()
    assert bool((buf == 7.5).all()) and bool((idx == -3).all())
    assert lib.r2l_occ_rays(g, None, None, 0, 2., 6., 4, None, p(idx), None, None, st) == 0  # R == 0: count = 0, nothing else
    assert idx[0].item() == 0 and bool((idx[1:] == -3).all())


# ---- 2. r2l_store_append_live -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rps", [4, 64])
@pytest.mark.parametrize("shuffle", [0, 1])
def test_append_live_equals_gather_then_append(rps, shuffle):
    from r2l_amd import raystore as R
    lib, p = _lib.load(), _lib.ptr
    rs = np.random.RandomState(rps + shuffle)
    n_rows = 1500
    rows = torch.from_numpy(rs.rand(n_rows, 9).astype(F32)).to(DEV)
    cap, first = 20 + 1000 // rps, 2
    for M in (0, 3, 64, 65, 1000):
        idx_np = np.sort(rs.choice(n_rows, M, replace=False)).astype(np.int64)
        if M >= 64:
            idx_np[M // 2] = n_rows + 5  # one index out of range: a NaN row
        idx = torch.from_numpy(idx_np).to(DEV)
        key = 1234567 + M
        got = torch.full((cap * rps, 9), -2., device=DEV)
        want = got.clone()
        m = ctypes.c_int64(-1)
        _lib.check(lib.r2l_store_append_live(p(rows), n_rows, p(idx) if M else None, M, p(got), cap, first, rps, key, shuffle,
                                             ctypes.byref(m), _lib.stream()), "r2l_store_append_live")
        assert m.value == M // rps
        # gather + r2l_store_append (the out-of-range index gathers a NaN row, as the call defines it)
        gathered = torch.full((max(M, 1), 9), float("nan"), device=DEV)
        ok = torch.from_numpy((idx_np >= 0) & (idx_np < n_rows)).to(DEV)
        if M:
            gathered[:M][ok] = rows[idx[ok]]
        m2 = ctypes.c_int64(-1)
        _lib.check(lib.r2l_store_append(p(gathered), M, p(want), cap, first, rps, key, shuffle, ctypes.byref(m2), _lib.stream()),
                   "r2l_store_append")
        assert m2.value == m.value and same_bits(got, want)
        # the restatement, and nothing outside the shards [first, first + m)
        a, b = first * rps, (first + m.value) * rps
        assert same_bits(got[a:b], R.append_live_spec(rows.cpu().numpy(), idx_np, rps, key, bool(shuffle)))
        assert bool((got[:a] == -2.).all()) and bool((got[b:] == -2.).all())
        if M >= 64:
            nan_rows = torch.isnan(got[a:b]).all(1)
            assert int(nan_rows.sum()) <= 1 and int(torch.isnan(got[a:b]).sum()) == 9 * int(nan_rows.sum())
            if not shuffle:
                assert bool(nan_rows[M // 2])  # (M // 2 < m * rps for these M)
    # the class method
    store = R.RayStore(8, DEV, rays_per_shard=rps)
    idx_np = np.sort(rs.choice(n_rows, 5 * rps + 3, replace=False)).astype(np.int64)
    assert store.append_live(rows, torch.from_numpy(idx_np).to(DEV), idx_np.size, 99) == 5 and store.n_shards == 5
    assert same_bits(store.shards().reshape(-1, 9), R.append_live_spec(rows.cpu().numpy(), idx_np, rps, 99))
    store.close()


# ---- 3. culled frames, each family ------------------------------------------------------------------------------------------------
@pytest.fixture(params=["fp32_mfma", "default", "bf16x3"])
def family(request, monkeypatch):
    from tests.conftest import use_family
    use_family(monkeypatch, **({} if request.param == "default" else {"precision": request.param}))
    return request.param


@pytest.fixture(scope="module")
def student():
    from tests.pose_refine_util import make_model
    n_block = 2
    return make_model(n_block=n_block, device=DEV, state=O.make_state_dict(n_block=n_block, seed=3)).eval()


def _sampler(H, W, focal):
    from model.nerf_raybased import PointSampler
    return PointSampler(H, W, focal, 16, 2., 6., device=DEV)


def _pose(k=0):
    return torch.from_numpy(O.pose_spherical(-170. + 47. * k, -15. - 20. * (k % 3), 4.)[:3, :4]).float()[None]


def _cull(G, kind, white, box=8.):
    g = RU.grid_with_bits(G, kind, seed=5, lo=(-box,) * 3, hi=(box,) * 3, device=DEV)
    g.dilate = 1  # (hand-made bits: the tests below hold for ANY bits)
    return RC.RayCull(g, 2., 6., white)


@pytest.mark.parametrize("H,W,kind", [(7, 9, "random"), (32, 32, "random"), (130, 130, "full")])
@pytest.mark.parametrize("white", [True, False])
def test_culled_frames(H, W, kind, white, family, student):
    """Live pixels = r2l_forward_rays_cfg on the compacted rays, bit for bit; dead pixels = the background exactly; a full grid
    agrees with forward_poses within the parity bar."""
    ps = _sampler(H, W, 0.9 * W)
    cull = _cull(16, kind, white)  # 16^3 cells of side 1 over +-8: every segment of the r = 4 camera stays inside
    c2w = _pose(1)
    with torch.no_grad():
        got = cull.render_poses(student, c2w, ps)[0]
    o, d = cull.frame_rays(c2w, H, W, ps.focal, torch.device(DEV))
    T = cull.steps(H, W, ps.focal)
    M, idx, live = RU.spec(cull.grid, o.cpu().numpy(), d.cpu().numpy(), 2., 6., T)
    assert (cull.live_rays, cull.total_rays) == (M, H * W)
    dead = torch.from_numpy(live == 0).to(DEV)
    assert bool((got[dead] == (1. if white else 0.)).all())
    if kind == "full":
        assert M == H * W
        with torch.no_grad():
            ref = student.render_poses(c2w, ps)[0]
        assert float((got - ref).abs().max()) < 1e-4
    else:
        assert 0 < M < H * W
    it = torch.from_numpy(idx).to(DEV)
    with torch.no_grad():
        want = student.engine().forward_rays(o[it], d[it], ps.z_vals, 0.)
    assert same_bits(got[it], want)


@pytest.mark.parametrize("white", [True, False])
def test_an_empty_grid_on_inside_rays_launches_no_forward(white, family, student):
    cull = _cull(4, "empty", white)
    ps = _sampler(32, 32, 30.)
    sentinel = torch.full((32 * 32, 3), -4., device=DEV)
    with torch.no_grad():
        got = cull.render_poses(student, _pose(0), ps, rgb_live=sentinel)
    assert cull.live_rays == 0 and bool((got == (1. if white else 0.)).all()) and bool((sentinel == -4.).all())


def test_without_the_switch_render_path_is_the_parent(student, tmp_path):
    """render_path without ray_cull= is the existing code path, bit for bit; with a full grid it agrees within the parity bar, with
    an empty one it is the background."""
    from r2l_amd import driver

    class Quiet:
        def info(self, *a):
            pass

    ps = _sampler(20, 24, 28.)
    poses = torch.cat([_pose(k) for k in range(3)], 0)
    dev = torch.device(DEV)
    off, _ = driver.render_path(poses, student, ps, dev, Quiet())
    with torch.no_grad():
        parent = student.render_poses(poses, ps).view(3, 20, 24, 3)
    assert same_bits(off, parent)
    full, _ = driver.render_path(poses, student, ps, dev, Quiet(), ray_cull=_cull(8, "full", True))
    assert float((full - off).abs().max()) < 1e-4
    empty, _ = driver.render_path(poses, student, ps, dev, Quiet(), ray_cull=_cull(4, "empty", False))
    assert bool((empty == 0.).all())


# ---- 4. against the teacher's unskipped frames -------------------------------------------------------------------------------------
def test_dead_rays_against_the_teachers_unskipped_frames():
    """The trained-like pair of tests/teacher_util.py, a box that contains every segment whole (tests/ray_cull_util.py T_*): the
    share of dead rays whose unskipped teacher colour is more than 1e-3 from the background is at most MISS_CAP, and at least 30 %
    of the rays are dead."""
    from r2l_amd.nerf_raybased import NeRF
    from r2l_amd.render import render_frames
    from tests.teacher_util import trained_like_pair
    nets = []
    for sd in trained_like_pair():
        m = NeRF(D=8, W=256, input_ch=63, output_ch=4, skips=[4], input_ch_views=27, use_viewdirs=True)
        m.load_state_dict(sd)
        nets.append(m.to(DEV).eval())
    grid = OC.OccupancyGrid([-RU.T_BOX] * 3, [RU.T_BOX] * 3, G=RU.T_G, k=2, dilate=1).build(nets[1])
    H = W = RU.T_HW
    for white in (True, False):
        cull = RC.RayCull(grid, RU.T_NEAR, RU.T_FAR, white)
        T = cull.steps(H, W, RU.T_FOCAL)
        with torch.no_grad():
            out = render_frames(RU.teacher_pose().to(DEV), H, W, RU.T_FOCAL, RU.T_NEAR, RU.T_FAR, nets[0], nets[1], 64, 128, 0, white,
                                seed=1, rows=True)
        rows = out["rows"]
        M, idx, live = cull.live_index(rows[:, 0:3], rows[:, 3:6], T)
        live = live.cpu().numpy()
        Ms, _, lives = RU.spec(grid, rows[:, 0:3].cpu().numpy(), rows[:, 3:6].cpu().numpy(), RU.T_NEAR, RU.T_FAR, T)
        assert M == Ms and np.array_equal(live, lives)
        miss, dead = RU.dead_ray_miss_share(rows[:, 6:9].cpu().numpy(), live, white)
        print("white %s: T = %d, dead rays %.1f %%, dead rays off the background by > 1e-3: %.3f %%" % (white, T, 100 * dead, 100 * miss))
        assert dead >= 0.30, dead
        assert miss <= RU.MISS_CAP, miss


# ---- 5. drivers --------------------------------------------------------------------------------------------------------------------
OCC = ["--r2l_occ_res", "128", "--r2l_occ_bound", "6"]  # (cells of 0.094: the frames' corners are dead)


def _teacher_ckpt(tmp_path):
    from tests.teacher_util import trained_like_pair
    csd, fsd = trained_like_pair()
    ck = str(tmp_path / "teacher.tar")
    torch.save({"global_step": 200000, "network_fn_state_dict": csd, "network_fine_state_dict": fsd}, ck)
    return ck


def _log(res):
    return open(os.path.join(res["logger"].log_path, "log.txt")).read()


def _replayed_plain_fill(ck):
    """The rows of online_kd_run's unculled fill (6 poses, groups of 3, rank 0) by the sequence that filled a store before the
    switch existed: the RandomState stream of online_kd.TeacherFill, render_frames(rows=True, occupancy=pair), perm(flush key)."""
    from r2l_amd import data
    from r2l_amd import raystore as R
    from r2l_amd.nerf_raybased import NeRF
    from r2l_amd.options import parse_teacher_config
    from r2l_amd.render import render_frames
    targs = parse_teacher_config(os.path.join(ROOT, "configs", "lego.txt"))
    sds = torch.load(ck, map_location="cpu", weights_only=False)
    nets = []
    for key in ("network_fn_state_dict", "network_fine_state_dict"):
        m = NeRF(D=8, W=256, input_ch=63, output_ch=4, skips=[4], input_ch_views=27, use_viewdirs=True)
        m.load_state_dict(sds[key])
        nets.append(m.to(DEV).eval())
    pair = tuple(OC.OccupancyGrid([-6.] * 3, [6.] * 3, G=128).build(n) for n in nets)
    focal = .5 * 64 / np.tan(.5 * 0.6911112070083618)
    rng, out = np.random.RandomState(0), []
    for g in range(2):
        group = []
        for _ in range(3):
            pose = data.get_rand_pose(rng)
            group.append((pose[:3, :4], focal * (1 + rng.rand())))
        key = int(rng.randint(0, 2**31 - 1))
        c2ws = torch.stack([torch.as_tensor(p) for p, _ in group], 0).to(DEV)
        focals = torch.tensor([f for _, f in group], dtype=torch.float32, device=DEV)
        with torch.no_grad():
            rows = render_frames(c2ws, 64, 64, focals, 2., 6., nets[0], nets[1], targs.N_samples, targs.N_importance, targs.perturb,
                                 targs.white_bkgd, seed=0, frame_id0=1 + 3 * g, rows=True, ndc=False, ndc_focal=focal,
                                 occupancy=pair)["rows"].cpu().numpy()
        out.append(rows[R.perm_at(key, rows.shape[0], np.arange(rows.shape[0], dtype=np.uint64))])
    return np.concatenate(out)


def test_online_kd_fill_resume_and_render_with_the_switch(tmp_path, monkeypatch):
    from r2l_amd import driver
    from r2l_amd import raystore as R
    from tests import occ_fused_util as FU
    from tests.test_driver_cpu import make_scene
    monkeypatch.chdir(tmp_path)
    ck = _teacher_ckpt(tmp_path)
    fused = ["--r2l_occ_fused", "--n_pose_kd", "6", "--create_data_chunk", "3"] + OCC  # two flush groups of 3 poses
    F_plain = str(tmp_path / "plain.r2l")
    plain, plain_log = FU.online_kd_run(tmp_path, ck, "plain", fused + ["--r2l_store_save", F_plain, "--i_weights", "2"])
    # WITHOUT the switch nothing changes: no line, no launch, no ray_cull entry in the provenance or the checkpoint, and the store is
    # bit for bit what the pre-existing sequence gives — render_frames(rows=True) per flush group with the replayed poses, focals
    # and ids, shuffled by perm(the replayed flush key)
    assert "ray cull" not in plain_log and "ray_cull" not in R.read_store_header(F_plain)["provenance"]
    import glob
    cks = glob.glob(str(tmp_path / "Experiments" / "occkd_plain_*" / "weights" / "ckpt*.tar"))
    assert len(cks) == 1 and RC.KEY not in torch.load(cks[0], map_location="cpu", weights_only=False)
    assert same_bits(plain[0], _replayed_plain_fill(ck))
    culled, log = FU.online_kd_run(tmp_path, ck, "cull", fused + ["--r2l_ray_cull"])
    # the culled store = the unculled fill's rows filtered with rays_spec under the same keys.  The unculled store holds the rows
    # of a group shuffled; the groups' rows are recovered by rendering them again through the same TeacherFill without the switch
    lines = [l for l in log.splitlines() if "ray cull: live rays" in l]
    assert len(lines) == 3 and "of the whole fill" in lines[-1]  # two flush groups and the total
    a, b = [int(x) for x in lines[-1].split("live rays ")[1].split(" (")[0].split(" / ")]
    assert b == 6 * 64 * 64 and 0 < a < b
    assert culled[0].shape[0] < plain[0].shape[0] and culled[0].shape[0] % 4096 == 0
    # every row of the culled store is a row of the unculled one, and a live one
    key = lambda t: {r.tobytes() for r in t.cpu().numpy()}
    assert key(culled[0]) <= key(plain[0])
    scene = str(tmp_path / "scene")
    argv = ["--model_name", "R2L", "--config", os.path.join(ROOT, "configs", "lego_noview.txt"), "--datadir", scene,
            "--n_sample_per_ray", "16", "--netwidth", "256", "--netdepth", "6", "--use_residual", "--trial.ON", "--trial.body_arch",
            "resmlp", "--testskip", "1", "--N_rand", "1", "--warmup_lr", "0.0001,200", "--i_print", "1", "--r2l_online_kd",
            "--r2l_teacher_config", os.path.join(ROOT, "configs", "lego.txt"), "--teacher_ckpt", ck, "--r2l_device_pool", "--hard_ratio", "0.2", "--hard_mul", "2", "--r2l_ray_cull", "--i_weights", "3",
            "--save_intermediate_models"] + fused
    full = driver.main(argv + ["--N_iters", "6", "--experiment_name", "cull_full"])
    w = full["logger"].weights_path
    c6 = torch.load(os.path.join(w, "ckpt_6.tar"), map_location="cpu", weights_only=False)
    assert RC.KEY in c6 and sorted(c6[RC.KEY]) == sorted(RC.STATE_FIELDS) and c6[RC.KEY]["G"] == 128
    # the culled fill holds exactly the shards that filtering the unculled fill's rows with rays_spec and the same keys gives.  A
    # group of 3 poses is 12288 rows = 3 whole shards, so the unculled store holds every row of a group: undo its shuffle with the
    # replayed flush key (online_kd.TeacherFill: per pose two draws for the pose and one for the focal, then the key)
    from r2l_amd import data
    grid = RC.RayCull.from_state(c6[RC.KEY], "cpu").grid
    focal = .5 * 64 / np.tan(.5 * 0.6911112070083618)
    T = OC.cull_steps(grid, 2., 6., OC.frame_d_max(64, 64, focal))
    rng, want = np.random.RandomState(0), []
    for g in range(2):
        for _ in range(3):
            data.get_rand_pose(rng)
            rng.rand()
        key = int(rng.randint(0, 2**31 - 1))
        shuffled = plain[0][g * 12288:(g + 1) * 12288].cpu().numpy()
        rows = np.empty_like(shuffled)
        rows[R.perm_at(key, 12288, np.arange(12288, dtype=np.uint64))] = shuffled
        M, idx, _ = RU.spec(grid, rows[:, 0:3], rows[:, 3:6], 2., 6., T)
        want.append(R.append_live_spec(rows, idx, 4096, key))
    want = np.concatenate(want)
    assert want.shape[0] == culled[0].shape[0] and same_bits(culled[0], want)
    res = driver.main(argv + ["--N_iters", "6", "--experiment_name", "cull_resume", "--pretrained_ckpt", os.path.join(w, "ckpt_3.tar"),
                              "--resume"])
    assert "ray cull: grid from the checkpoint" in _log(res)
    r6 = torch.load(os.path.join(res["logger"].weights_path, "ckpt_6.tar"), map_location="cpu", weights_only=False)
    from tests.test_pool_select_gpu import _ckpt_equal
    assert _ckpt_equal(c6, r6) == (True, True)  # the weights, every Adam moment, the hard-ray pool
    assert sorted(c6) == sorted(r6)
    assert all(c6[k] == r6[k] for k in ("global_step", "best_psnr", "best_psnr_step")) and c6["global_step"] == 6
    assert all(torch.equal(c6[RC.KEY][k], r6[RC.KEY][k]) if k == "bits" else c6[RC.KEY][k] == r6[RC.KEY][k] for k in RC.STATE_FIELDS)
    assert "ray cull: the grid is the store fill's" in _log(full) and _log(full).count("occupancy grid (") == 2  # (built once)
    # --render_only --render_test: the grid comes from the checkpoint, the dead rays are background (configs/lego_noview: white)
    rend = ["--model_name", "R2L", "--config", os.path.join(ROOT, "configs", "lego_noview.txt"), "--datadir", scene, "--testskip", "1",
            "--n_sample_per_ray", "16", "--netwidth", "256", "--netdepth", "6", "--use_residual", "--trial.ON", "--trial.body_arch",
            "resmlp", "--pretrained_ckpt", os.path.join(w, "ckpt_6.tar"), "--render_only", "--render_test"]
    on = driver.main(rend + ["--r2l_ray_cull", "--experiment_name", "cull_render"])
    assert "ray cull: grid from the checkpoint" in _log(on) and "live rays" in _log(on)
    # the dead rays of the test poses, by the restatement on the checkpoint's grid: exactly the background, and only they
    from r2l_amd import data
    cull = RC.RayCull.from_state(c6[RC.KEY], DEV)
    test_poses = torch.stack([torch.as_tensor(np.asarray(data.pose_spherical(40. * i, -30., 4.)), dtype=torch.float32)[:3, :4] for i in range(2)], 0)
    focal = .5 * 64 / np.tan(.5 * 0.6911112070083618)
    o, d = cull.frame_rays(test_poses, 64, 64, focal, torch.device(DEV))
    _, _, live = RU.spec(cull.grid, o.cpu().numpy(), d.cpu().numpy(), 2., 6., cull.steps(64, 64, focal))
    dead = torch.from_numpy(live == 0).view(2, 64, 64)
    print("test poses: %d of %d rays dead" % (int(dead.sum()), dead.numel()))
    assert on["rgbs"].shape == (2, 64, 64, 3) and bool(dead.any()) and not bool(dead.all())
    white = (on["rgbs"].cpu() == 1.).all(-1)
    assert torch.equal(white, dead)  # (a sigmoid of a finite number is below 1: a live pixel is never exactly white)
    off = driver.main(rend + ["--experiment_name", "cull_render_off"])
    assert "WARNING: the checkpoint carries a grid (key r2l_ray_cull)" in _log(off) and "live rays" not in _log(off)
    assert not bool((off["rgbs"].cpu() == 1.).all(-1).any())


def test_create_data_writes_a_culled_store_file_and_main_refuses_it_without_the_switch(tmp_path, monkeypatch):
    from r2l_amd import create_data, driver
    from r2l_amd import raystore as R
    from tests.test_driver_cpu import make_scene
    monkeypatch.chdir(tmp_path)
    ck = _teacher_ckpt(tmp_path)
    scene = str(tmp_path / "scene")
    os.makedirs(scene)
    make_scene(scene, size=128)
    F = str(tmp_path / "cd.r2l")
    out = create_data.main(["--create_data", "rand", "--config", os.path.join(ROOT, "configs", "lego.txt"), "--datadir", scene,
                            "--teacher_ckpt", ck, "--n_pose_kd", "3", "--create_data_chunk", "3", "--experiment_name", "cull_store",
                            "--r2l_store_save", F, "--r2l_occ_fused", "--r2l_ray_cull", "--no_rand_focal"] + OCC)  # (the scene's focal: the corners are dead)
    prov = R.read_store_header(F)["provenance"]
    assert sorted(prov["ray_cull"]) == ["T", "bound", "dilate", "far", "near", "res"]
    assert prov["ray_cull"]["res"] == 128 and prov["ray_cull"]["bound"] == 6. and prov["ray_cull"]["dilate"] == 1
    assert 0 < out["n_rays"] < 3 * 4096 and "ray cull: live rays" in _log(out)
    load = ["--model_name", "R2L", "--config", os.path.join(ROOT, "configs", "lego_noview.txt"), "--datadir", scene,
            "--n_sample_per_ray", "16", "--netwidth", "256", "--netdepth", "6", "--use_residual", "--trial.ON",
            "--trial.body_arch", "resmlp", "--testskip", "1", "--N_rand", "1", "--N_iters", "1", "--r2l_store_load", F]
    with pytest.raises(ValueError, match="r2l_ray_cull"):
        driver.main(load + ["--experiment_name", "cull_load_off"])
    # with the switch the file is used as it is, and the log says whether its rows were culled with the grid this run renders with
    teacher = ["--r2l_ray_cull", "--teacher_ckpt", ck, "--r2l_teacher_config", os.path.join(ROOT, "configs", "lego.txt")]
    same = driver.main(load + teacher + OCC + ["--experiment_name", "cull_load_same"])
    assert "ray cull: the store file was culled with this run's grid" in _log(same)
    other = driver.main(load + teacher + ["--r2l_occ_res", "64", "--r2l_occ_bound", "8", "--experiment_name", "cull_load_other"])
    line = [l for l in _log(other).splitlines() if "this run's grid DIFFER" in l]
    assert len(line) == 1 and "res: file 128, run 64" in line[0] and "bound: file 6.0, run 8.0" in line[0]
