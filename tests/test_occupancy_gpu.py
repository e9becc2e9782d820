"""Occupancy grid of the teacher's render on the GPU (csrc/r2l_occupancy.hip; include/r2l_hip.h "occupancy grid"): the three
kernels against their numpy specs bit for bit, the skipped render against the zero-masked full render bit for bit, its agreement
with the full render where the grid skips positive density, the driver switch and the argument refusals."""
import ctypes
import os

import numpy as np
import pytest
import torch

from r2l_amd import _lib
from r2l_amd import occupancy as OC
from tests import occupancy_util as U
from tests.teacher_util import scene_rays, trained_like_pair

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOX = 1.6  # the fitted box of tests/teacher_util.py::fit_teacher


@pytest.fixture(scope="module")
def nets():
    from r2l_amd.nerf_raybased import NeRF
    out = []
    for sd in trained_like_pair():
        m = NeRF(D=8, W=256, input_ch=63, output_ch=4, skips=[4], input_ch_views=27, use_viewdirs=True)
        m.load_state_dict(sd)
        for p in m.parameters():
            p.requires_grad = False
        out.append(m.to(DEV).eval())
    return out


@pytest.fixture(params=["fp32_mfma", "default"])
def family(request, monkeypatch):
    from tests.conftest import use_family
    use_family(monkeypatch, **({"precision": "fp32_mfma"} if request.param == "fp32_mfma" else {}))
    return request.param


def _frame_rays(R):
    """R rays of scene_rays' camera spread evenly over its 181 x 181 frame (its first rays are the top rows, which miss the scene)."""
    n = 181 * 181
    rays = scene_rays(n, 0)[::n // R][:R].contiguous()
    assert rays.shape[0] == R
    return rays.to(DEV)


def _cuda(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


# ---- 1. compact ---------------------------------------------------------------------------------------------------------------
# R*S: across a wave (64), a round of a workgroup (256), a workgroup's run of samples (2048: 37 * 64 = 2368) and many of them
# (192 005 = 94 workgroups, set by S = 1 rows); 1025 * 2048 + 3: more workgroups than the scan kernel has threads
COMPACT_SIZES = [(1, 1), (63, 7), (64, 64), (65, 5), (255, 5), (256, 64), (257, 1), (37 * 64, 64), (1000 * 192 + 5, 1)]


def test_compact_more_workgroups_than_scan_threads():
    _compact_case(1025 * 2048 + 3, 1, 32, "random")


@pytest.mark.parametrize("kind", ["empty", "full", "random"])
@pytest.mark.parametrize("G", [5, 32])
@pytest.mark.parametrize("n,S", COMPACT_SIZES)
def test_compact_equals_spec(n, S, G, kind):
    _compact_case(n, S, G, kind)


def _compact_case(n, S, G, kind):
    grid = U.grid_with_bits(G, kind, seed=n, device=DEV)
    o, d, v, z = U.edge_rays(n, S, G, seed=1)
    assert z.size == n
    want = OC.compact_spec(grid.words(), grid.lo, grid.inv, G, o, d, v, z)
    if kind == "empty":
        pts = OC.sample_points(o, d, z).reshape(-1, 3)
        inside = ((pts >= -1) & (pts < 1)).all(1)
        assert want[0] == int((~inside).sum())  # all empty: only the samples outside the box (NaN, inf among them) are live
    if kind == "full":
        assert want[0] == n
    if kind == "random" and n >= 2000:
        assert 0 < want[0] < n
    to, td, tv, tz = _cuda(o, d, v, z)
    got = []
    for _ in range(2):
        M, idx, oo, od, ov, oz = grid.compact(to, td, tv, tz)
        got.append((M, idx.clone(), oo.clone(), od.clone(), ov.clone(), oz.clone()))
    M, idx, oo, od, ov, oz = got[0]
    assert M == want[0], (M, want[0])
    assert idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), want[1])
    assert M < 2 or bool((idx[1:] > idx[:-1]).all())  # ascending
    for g_, w_, name in ((oo, want[2], "o"), (od, want[3], "d"), (ov, want[4], "v"), (oz, want[5], "z")):
        assert U.same_bits(g_, w_), name
    assert got[1][0] == M and all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                              b.view(torch.int32) if b.dtype == torch.float32 else b)
                                  for a, b in zip(got[0][1:], got[1][1:]))  # two calls, equal bits


def test_compact_all_empty_inside_gives_zero_and_R0():
    """M = 0 exactly: every sample inside an empty grid; and R == 0 is a successful no-op that sets the count to 0."""
    grid = U.grid_with_bits(5, "empty", device=DEV)
    rs = np.random.RandomState(3)
    o = (rs.rand(300, 3) * 1.8 - 0.9).astype(np.float32)
    d = np.zeros((300, 3), np.float32)
    z = rs.rand(300, 7).astype(np.float32)
    to, td, tz = _cuda(o, d, z)
    M, idx, *_ = grid.compact(to, td, td, tz)
    assert M == 0 and idx.numel() == 0
    raw = grid.scatter(None, idx, 300, 7)  # M = 0: the zero fill alone
    assert raw.shape == (300, 7, 4) and int((raw.view(torch.int32) != 0).sum()) == 0
    grid._buf[("cuda", 0)]["count"].fill_(77)
    M, idx, *_ = grid.compact(to[:0], td[:0], td[:0], tz[:0])
    assert M == 0


# ---- 2. build -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,k", [(5, 1), (5, 2), (16, 1), (16, 2)])
def test_build_equals_spec_on_its_own_sigma(G, k, family, nets):
    """bits == build_spec(sigma_out) for every dilation and threshold, and sigma_out == TeacherEngine.mlp on the probe points."""
    from r2l_amd.render import teacher_engine
    fine = nets[1]
    sig0 = None
    for dilate in (0, 1, 2):
        for thresh in (0., 50.):
            g = OC.OccupancyGrid([-BOX] * 3, [BOX] * 3, G=G, k=k, dilate=dilate, sigma_thresh=thresh).build(fine, keep_sigma=True)
            sig = g.sigma.cpu().numpy()
            assert sig.shape == ((G * k)**3,)
            want = OC.build_spec(sig, G, k, dilate, thresh)
            assert np.array_equal(g.words(), want), (G, k, dilate, thresh)
            if sig0 is None:
                sig0 = sig
                share = g.occupied_share()
                assert G < 16 or 0.02 < share < 0.9, share  # at 16^3 the trained-like scene has both kinds of cells
            assert U.same_bits(sig, sig0)  # the same bits on every call
    pts = OC.probe_points(g.lo, g.step, G, k)
    n = pts.shape[0]
    o, = _cuda(pts)
    zeros = torch.zeros(n, 3, device=DEV)
    view = torch.tensor([0., 0., 1.], device=DEV).expand(n, 3).contiguous()
    raw = teacher_engine(fine).mlp(o, zeros, view, torch.zeros(n, 1, device=DEV))
    assert U.same_bits(raw[:, 0, 3], sig0)
    assert G < 16 or ((sig0 > 50).any() and (sig0 < 0).any())


# ---- 3. scatter ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,S", [(1, 1), (5, 13), (37, 64), (300, 192)])
def test_scatter_equals_spec(R, S):
    rs = np.random.RandomState(R * 1000 + S)
    n = R * S
    for M in sorted({0, 1, n // 3, n}):
        M = min(M, n)
        idx = np.sort(rs.permutation(n)[:M]).astype(np.int64)
        raw_live = rs.randn(M, 4).astype(np.float32)
        if M:
            raw_live[0, 0] = np.nan
        want = OC.scatter_spec(raw_live, idx, R, S)
        t_live, t_idx = _cuda(raw_live, idx)
        got = OC.OccupancyGrid.scatter(t_live if M else None, t_idx, R, S)
        assert U.same_bits(got, want), (R, S, M)


# ---- 4. masked equivalence ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grids64(nets):
    """The test grids: 64^3 x 2 probes x dilation 1 over +-1.6, default family (the builds of the two families agree in the bits
    or not — the tests below hold for ANY bits)."""
    return tuple(OC.OccupancyGrid([-BOX] * 3, [BOX] * 3, G=64, k=2, dilate=1).build(n) for n in nets)


@pytest.mark.parametrize("perturb", [0., 1.])
@pytest.mark.parametrize("Ns,Ni", [(64, 128), (8, 16), (16, 0)])
def test_masked_equivalence(Ns, Ni, perturb, family, nets, grids64):
    """Stage by stage, torch.equal: the live rows' raw is the full launch's raw at idx; the coarse maps and weights are
    raw2outputs of the zero-masked full raw, hence the fine depths are equal; the fine outputs equal the masked full render."""
    from r2l_amd.render import _coarse_z, raw2outputs, render_rays, sample_pdf_sort, teacher_engine
    coarse, fine = nets
    rays = _frame_rays(300)
    R = rays.shape[0]
    g = torch.Generator().manual_seed(Ns * 100 + Ni)
    t_rand = torch.rand(R, Ns, generator=g) if perturb else None
    u = torch.rand(R, max(Ni, 1), generator=g).to(DEV) if perturb else None
    o, d, vd = rays[:, 0:3].contiguous(), rays[:, 3:6].contiguous(), rays[:, 8:11].contiguous()
    engines = [teacher_engine(coarse), teacher_engine(fine)]
    before = [e.range_info() for e in engines]
    got = render_rays(rays, coarse, None, Ns, N_importance=Ni, network_fine=fine, perturb=perturb, t_rand=t_rand, u=u, retraw=True,
                      occupancy=grids64)

    def stage(eng, grid, z):
        full = eng.mlp(o, d, vd, z)
        M, idx, lo_, ld_, lv_, lz_ = grid.compact(o, d, vd, z)
        assert 0 < M < z.numel()
        live = eng.mlp(lo_, ld_, lv_, lz_.reshape(M, 1)).reshape(M, 4)
        assert torch.equal(live.view(torch.int32), full.reshape(-1, 4)[idx].view(torch.int32)), "live rows' raw != full raw at idx"
        masked = torch.zeros_like(full).reshape(-1, 4)
        masked[idx] = full.reshape(-1, 4)[idx]
        masked = masked.reshape(full.shape)
        assert torch.equal(grid.scatter(live, idx.clone(), *z.shape), masked)
        return masked

    z = _coarse_z(rays[:, 6:7].contiguous(), rays[:, 7:8].contiguous(), Ns, False, perturb, False, t_rand)
    m0 = stage(engines[0], grids64[0], z)
    rgb0, disp0, acc0, w0, depth0 = raw2outputs(m0, z, d)
    if Ni == 0:
        want = dict(rgb_map=rgb0, acc_map=acc0, depth_map=depth0, raw=m0)
        disp = disp0
    else:
        assert torch.equal(got["rgb0"], rgb0) and torch.equal(got["acc0"], acc0) and U.same_bits(got["disp0"], disp0)
        zs, z_all, z_std = sample_pdf_sort(z, w0, Ni, det=(perturb == 0.), u=u)
        assert torch.equal(got["z_std"], z_std)  # a function of the fine depths: they are equal
        m1 = stage(engines[1], grids64[1], z_all)
        rgb, disp, acc, _, depth = raw2outputs(m1, z_all, d, need_weights=False)
        want = dict(rgb_map=rgb, acc_map=acc, depth_map=depth, raw=m1)
    for name, w in want.items():
        assert torch.equal(got[name], w), name
    assert U.same_bits(got["disp_map"], disp)  # NaN where acc = 0, on both sides
    after = [e.range_info() for e in engines]
    for b, a in zip(before, after):
        assert (a["trips"], a["rescales"], a["scale"]) == (b["trips"], b["rescales"], b["scale"]), \
            "a launch of the fp16 family tripped or rescaled: the two renders did not run on one stream of weights (%s -> %s)" % (b, a)


# ---- 5. agreement with the unskipped render -------------------------------------------------------------------------------------
MISS_CAP = 0.01  # at most 1 % of the rays may carry a skipped sample with sigma > 0 (a condition, not a measurement)


def _check_miss_report(rep, cap=MISS_CAP):
    """Rays without a miss: rgb, acc, depth bit for bit.  Rays with misses: |d rgb| <= 2 (1 - prod(1 - alpha_missed)) + 1e-5."""
    clean = rep["misses"] == 0
    for name in ("rgb", "acc", "depth"):
        a, b = rep["skip"][name][clean], rep["full"][name][clean]
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    drgb = (rep["skip"]["rgb"].double() - rep["full"]["rgb"].double()).abs().amax(-1)
    bound = 2. * rep["lost"] + 1e-5
    bad = ~(drgb <= bound)
    share = float((~clean).double().mean())
    print("rays with a miss: %d of %d (%.3f %%); largest |d rgb| %.3e, on a ray with bound %.3e" %
          (int((~clean).sum()), clean.numel(), 100 * share, float(drgb.max()), float(bound[drgb.argmax()])))
    assert not bad.any(), (drgb[bad], bound[bad])
    assert share <= cap, share
    return share


def test_agreement_with_the_full_render(family, nets, grids64):
    rays = _frame_rays(2000)
    rep = OC.miss_report(rays, nets[0], nets[1], grids64, 64, 128)
    _check_miss_report(rep)
    assert float(rep["skip"]["acc"].max()) > 0.5  # the rays do hit the scene
    live = sum(g.live_points for g in grids64) / max(sum(g.total_points for g in grids64), 1)
    assert 0.05 < live < 0.95, live


# ---- 6. driver ------------------------------------------------------------------------------------------------------------------
def test_create_data_with_the_switch(tmp_path, monkeypatch):
    """create_data --create_data rand --r2l_occupancy.  Two 16 x 16 poses: the run logs the build and the live share and leaves
    the same shards as without the switch (none: a shard is 4096 rays).  Two 64 x 64 poses (one shard each): the same shard shapes,
    rays bit for bit, and rgb within the bound of test 5 against the run without the switch."""
    from r2l_amd import create_data
    from tests.test_driver_cpu import ROOT, make_scene
    monkeypatch.chdir(tmp_path)
    csd, fsd = trained_like_pair()
    torch.save({"network_fn_state_dict": csd, "network_fine_state_dict": fsd}, str(tmp_path / "teacher.tar"))
    rows = {}
    for size in (32, 128):  # half_res: 16 x 16 and 64 x 64
        scene = str(tmp_path / ("scene%d" % size))
        os.makedirs(scene)
        make_scene(scene, size=size)
        for tag, extra in (("full", []), ("occ", ["--r2l_occupancy", "--r2l_occ_res", "64", "--r2l_occ_bound", str(BOX)])):
            kd = str(tmp_path / ("kd%d%s" % (size, tag)))
            out = create_data.main(["--create_data", "rand", "--config", os.path.join(ROOT, "configs", "lego.txt"), "--datadir", scene,
                                    "--teacher_ckpt", str(tmp_path / "teacher.tar"), "--n_pose_kd", "2", "--create_data_chunk", "2",
                                    "--datadir_kd", scene + ":" + kd, "--experiment_name", "occ%d%s" % (size, tag), "--perturb", "0",
                                    "--no_rand_focal"] + extra)
            files = sorted(os.listdir(kd))
            rows[size, tag] = [np.load(os.path.join(kd, f)) for f in files]
            log = open(os.path.join(out["logger"].log_path, "log.txt")).read()
            if tag == "occ":
                assert log.count("occupancy grid (") == 2 and "built in" in log and "of the cells occupied" in log
                line = [l for l in log.splitlines() if "live points" in l]
                assert len(line) == 1
                a, b = [int(x) for x in line[0].split("live points ")[1].split(" (")[0].split(" / ")]
                assert b == 2 * (size // 2)**2 * (64 + 64 + 128) and 0 < a < b, line
            else:
                assert "occupancy grid" not in log and "live points" not in log  # without the switch no log line changes
        assert [r.shape for r in rows[size, "occ"]] == [r.shape for r in rows[size, "full"]]
    assert rows[32, "full"] == [] and [r.shape for r in rows[128, "full"]] == [(4096, 9)] * 2
    full, occ = np.concatenate(rows[128, "full"]), np.concatenate(rows[128, "occ"])
    assert np.array_equal(full[:, :6].view(np.uint32), occ[:, :6].view(np.uint32))  # the same rays in the same places
    # the bound of test 5 on these very rays (white background, as configs/lego.txt renders them)
    from r2l_amd.nerf_raybased import NeRF
    from r2l_amd.render import teacher_engine
    pair = []
    for sd in (csd, fsd):
        m = NeRF(D=8, W=256, input_ch=63, output_ch=4, skips=[4], input_ch_views=27, use_viewdirs=True)
        m.load_state_dict(sd)
        pair.append(m.to(DEV).eval())
    grids = tuple(OC.OccupancyGrid([-BOX] * 3, [BOX] * 3, G=64).build(n) for n in pair)
    o, d = torch.from_numpy(full[:, 0:3].copy()).to(DEV), torch.from_numpy(full[:, 3:6].copy()).to(DEV)
    one = torch.ones(o.shape[0], 1, device=DEV)
    rays = torch.cat([o, d, 2. * one, 6. * one, d / torch.norm(d, dim=-1, keepdim=True)], -1)  # (viewdirs as render() forms them)
    rep = OC.miss_report(rays, pair[0], pair[1], grids, 64, 128, white_bkgd=True)
    assert np.array_equal(rep["full"]["rgb"].numpy().view(np.uint32), full[:, 6:9].view(np.uint32))  # the report re-renders the rows
    rep["skip"]["rgb"] = torch.from_numpy(occ[:, 6:9].copy())
    clean = rep["misses"] == 0
    assert torch.equal(rep["skip"]["rgb"][clean], rep["full"]["rgb"][clean])
    drgb = (rep["skip"]["rgb"].double() - rep["full"]["rgb"].double()).abs().amax(-1)
    assert bool((drgb <= 2. * rep["lost"] + 1e-5).all())


# ---- 7. argument refusals -------------------------------------------------------------------------------------------------------
def test_argument_refusals_launch_nothing():
    """Every refusal: hipErrorInvalidValue, the argument named, and the device untouched (the dummy pointers of the table would
    fault if a kernel read them; real buffers keep their sentinel)."""
    n = U.check_refusals()
    assert n >= 50
    lib = _lib.load()
    grid = U.grid_with_bits(5, "full", device=DEV)
    buf = torch.full((64,), 7.5, device=DEV)
    cnt = torch.full((1,), -3, dtype=torch.int64, device=DEV)
    p = _lib.ptr
    rc = lib.r2l_occ_compact(ctypes.byref(grid.desc()), p(buf), p(buf), p(buf), p(buf), 4, 0, p(buf), p(buf), p(buf), p(buf), p(cnt),
                             p(cnt), p(buf), _lib.stream())
    assert rc == U.INVALID
    rc = lib.r2l_occ_scatter(p(buf), p(cnt), 9, p(buf), 2, 4, _lib.stream())  # M > R*S
    assert rc == U.INVALID
    torch.cuda.synchronize()
    assert bool((buf == 7.5).all()) and int(cnt[0]) == -3
