"""Empty-space skipping inside the fused teacher-frames call, on the GPU (include/r2l_hip.h "occupancy inside the fused frames
call"): the point network's live form against the plain launch bit for bit in every kernel family, r2l_occ_index against
r2l_occ_compact and its numpy spec, r2l_teacher_frames_occ_cfg against the per-pose occupancy render bit for bit, its agreement
with the unskipped frames, the drivers behind --r2l_occ_fused and the argument refusals."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import r2l_oracle as O
from r2l_amd import _lib
from r2l_amd import occupancy as OC
from tests import occupancy_util as U
from tests import occ_fused_util as FU
from tests.teacher_util import forward_inputs, scaled_state_dict, trained_like_pair

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOX = 1.6  # the fitted box of tests/teacher_util.py::fit_teacher
NEAR, FAR = 2., 6.
MISS_CAP = 0.01  # at most 1 % of the rays may carry a skipped sample with sigma > 0 (a condition, not a measurement)


def _module(sd):
    from r2l_amd.nerf_raybased import NeRF
    m = NeRF(D=8, W=256, input_ch=63, output_ch=4, skips=[4], input_ch_views=27, use_viewdirs=True)
    m.load_state_dict(sd)
    for p in m.parameters():
        p.requires_grad = False
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def nets():
    return [_module(sd) for sd in trained_like_pair()]


@pytest.fixture(scope="module")
def grids64(nets):
    """64^3 cells x 2 probes x dilation 1 over +-1.6, built by the existing build (the tests below hold for ANY bits)."""
    return tuple(OC.OccupancyGrid([-BOX] * 3, [BOX] * 3, G=64, k=2, dilate=1).build(n) for n in nets)


@pytest.fixture(params=["fp32_mfma", "default", "bf16x3"])
def family(request, monkeypatch):
    from tests.conftest import use_family
    use_family(monkeypatch, **({} if request.param == "default" else {"precision": request.param}))
    return request.param


def _cuda(*arrays):
    return [(a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(DEV).contiguous() for a in arrays]


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. the point network on an index list with a device count ---------------------------------------------------------------
GUARD = 64  # sentinel floats behind raw, sentinel entries behind the idx capacity
LIVE_SHAPES = [(1, 1), (129, 1), (300, 7), (37, 64), (50, 192)]  # R*S = 1, 129, 2100, 2368, 9600: 1 .. 75 workgroups of 128


def _live_call(eng, o, d, v, z, idx_buf, count, raw_buf):
    """r2l_teacher_mlp_live_cfg on caller-made buffers (raw_buf and idx_buf carry sentinels behind their capacity)."""
    from r2l_amd import engine
    R, S = z.shape
    eng.ensure_packed()
    p = _lib.ptr
    _lib.check(_lib.load().r2l_teacher_mlp_live_cfg(p(o), p(d), p(v), p(z), p(idx_buf), p(count), p(eng.wstream), p(eng.flat), p(raw_buf),
                                                    R, S, _lib.stream(), ctypes.byref(engine.merged_config(eng.cfg))),
               "r2l_teacher_mlp_live_cfg")
    return raw_buf[:R * S * 4].view(R * S, 4)


def _live_counts(n):
    """The counts of a capacity n: around the half-wave (32) and the workgroup (128), the capacity, and several whole workgroups
    below the capacity (so that workgroups behind the count exist and leave)."""
    c = {0, 1, 31, 32, 33, 127, 128, 129, n}
    if n > 5 * 128:
        c.add(n - 3 * 128 - 5)
    return sorted(x for x in c if x <= n)


@pytest.mark.parametrize("R,S", LIVE_SHAPES)
def test_live_mlp_equals_the_plain_launch_at_idx(R, S, family, nets):
    from r2l_amd.render import teacher_engine
    eng = teacher_engine(nets[1])
    o, d, v, z = _cuda(*forward_inputs(R, S, "trained", seed=3))
    n = R * S
    before = eng.range_info()
    full = eng.mlp(o, d, v, z).reshape(n, 4)
    assert bool(torch.isfinite(full).all()) and int((_bits(full) == 0).sum()) == 0  # (a written entry is never +0: the zero fill shows)
    rs = np.random.RandomState(n)
    perm = rs.permutation(n).astype(np.int64)  # jumps across rays; its tail holds the samples that must NOT be computed
    cases = [(c, perm.copy(), c) for c in _live_counts(n)]
    cases.append((n + 1000, perm.copy(), n))  # a count above the capacity is the capacity
    if n >= 129:
        bad = perm.copy()
        bad[5], bad[70] = n, -1  # two entries out of range: skipped, their samples stay zero
        cases.append((128, bad, 128))
    for count, idx_np, used in cases:
        idx_buf = torch.cat([torch.from_numpy(idx_np), torch.full((GUARD,), 3, dtype=torch.int64)]).to(DEV)
        keep = idx_buf.clone()
        cnt = torch.tensor([count], dtype=torch.int64, device=DEV)
        want = torch.zeros_like(full)
        sel = torch.from_numpy(idx_np[:used][(idx_np[:used] >= 0) & (idx_np[:used] < n)]).to(DEV)
        want[sel] = full[sel]
        got = []
        for _ in range(2):
            raw_buf = torch.full((n * 4 + GUARD,), -7., device=DEV)
            got.append(_live_call(eng, o, d, v, z, idx_buf, cnt, raw_buf).clone())
            assert bool((raw_buf[n * 4:] == -7.).all()), (count, "written behind raw")
        assert torch.equal(_bits(got[0]), _bits(want)), (R, S, count, int((_bits(got[0]) != _bits(want)).any(-1).sum()))
        assert torch.equal(_bits(got[0]), _bits(got[1])), (R, S, count)  # two calls, the same bits
        assert torch.equal(idx_buf, keep) and int(cnt[0]) == count
    # the wrapper
    idx, cnt = torch.from_numpy(perm).to(DEV), torch.tensor([min(33, n)], dtype=torch.int64, device=DEV)
    raw = eng.mlp_live(o, d, v, z, idx, cnt)
    assert raw.shape == (R, S, 4) and torch.equal(_bits(raw.reshape(n, 4)[idx[:min(33, n)]]), _bits(full[idx[:min(33, n)]]))
    assert int((_bits(raw) != 0).any(-1).sum()) == min(33, n)
    after = eng.range_info()
    assert (after["trips"], after["rescales"], after["scale"]) == (before["trips"], before["rescales"], before["scale"]), (before, after)


def test_live_mlp_on_the_index_of_a_grid_equals_compact_mlp_scatter(family, nets, grids64):
    """idx and count straight from r2l_occ_index, nothing read on the host: the parent's compact -> mlp on [M,1] -> scatter."""
    from r2l_amd.render import teacher_engine
    eng, grid = teacher_engine(nets[1]), grids64[1]
    o, d, v, z = _cuda(*forward_inputs(300, 64, "trained", seed=5))
    M, cidx, lo_, ld_, lv_, lz_ = grid.compact(o, d, v, z)
    assert 0 < M < z.numel()
    want = grid.scatter(eng.mlp(lo_, ld_, lv_, lz_.reshape(M, 1)), cidx.clone(), *z.shape)
    idx, cnt = grid.index(o, d, z)
    got = eng.mlp_live(o, d, v, z, idx, cnt)
    assert torch.equal(_bits(got), _bits(want))


def test_live_mlp_through_a_range_trip(monkeypatch):
    """tests/teacher_util.py::scaled_state_dict makes the plain fp16x2 launch trip its range guard (the bf16x3 kernel redoes it,
    the stream is re-packed for a scale).  Two engines of the same weights, one driven by the plain call, one by the live call on
    the same points: the same trips, rescales and scale after every call, and the live raw equals the plain raw at idx — through
    the launch that trips (both kernels of the pair in their live form) and on the re-packed stream behind it."""
    from tests.conftest import use_family
    from r2l_amd.render import teacher_engine
    use_family(monkeypatch)
    sd = scaled_state_dict()
    R, S = 257, 16
    o, d, v, z = forward_inputs(R, S, "init", seed=9)
    n = R * S
    # the subset keeps the point with the largest first-layer activation, so that both engines see the same range
    pts = (o[:, None, :] + d[:, None, :] * z[:, :, None]).reshape(-1, 3)
    h0 = torch.nn.functional.linear(O.nerf_embed(pts, 10), sd["pts_linears.0.weight"], sd["pts_linears.0.bias"]).abs().amax(-1)
    assert h0.max().item() > 4.0e4  # the case really leaves the guarded range
    rs = np.random.RandomState(1)
    sub = rs.permutation(n)[:n // 2].astype(np.int64)
    sub = np.unique(np.concatenate([sub, [int(h0.argmax())]]))
    rs.shuffle(sub)
    full_perm = rs.permutation(n).astype(np.int64)
    o, d, v, z = _cuda(o, d, v, z)
    plain, live = teacher_engine(_module(sd)), teacher_engine(_module(sd))
    tripped = 0
    for step, idx_np in enumerate([full_perm, sub, sub, full_perm, sub]):
        idx = torch.cat([torch.from_numpy(idx_np), torch.zeros(n - idx_np.size, dtype=torch.int64)]).to(DEV)
        cnt = torch.tensor([idx_np.size], dtype=torch.int64, device=DEV)
        a = plain.mlp(o, d, v, z).reshape(n, 4)
        b = live.mlp_live(o, d, v, z, idx, cnt).reshape(n, 4)
        ia, ib = plain.range_info(), live.range_info()
        print("step %d: plain %s | live %s" % (step, {k: ia[k] for k in ("trips", "rescales", "scale")},
                                               {k: ib[k] for k in ("trips", "rescales", "scale")}))
        assert (ia["trips"], ia["rescales"], ia["scale"], ia["flag"]) == (ib["trips"], ib["rescales"], ib["scale"], ib["flag"]), (step, ia, ib)
        tripped = ia["trips"]
        sel = idx[:idx_np.size]
        assert torch.equal(_bits(b[sel]), _bits(a[sel])), step
        assert int((_bits(b) != 0).any(-1).sum()) == idx_np.size
    assert tripped >= 1  # the fixture does trip the guard: the comparison above covered it


# ---- 2. the index alone --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["empty", "full", "random"])
@pytest.mark.parametrize("n,S", [(1, 1), (63, 7), (64, 64), (257, 1), (37 * 64, 64)])
def test_index_equals_compact_and_spec(n, S, kind):
    G = 32
    grid = U.grid_with_bits(G, kind, seed=n, device=DEV)
    o, d, v, z = U.edge_rays(n, S, G, seed=1)
    assert z.size == n
    M, widx, *_ = OC.compact_spec(grid.words(), grid.lo, grid.inv, G, o, d, v, z)
    to, td, tv, tz = _cuda(o, d, v, z)
    cM, cidx, *_ = grid.compact(to, td, tv, tz)
    cidx = cidx.clone()
    assert cM == M and np.array_equal(cidx.cpu().numpy(), widx)
    grid._buf[("cuda", 0)]["idx"].fill_(-9)
    acc = torch.zeros(2, dtype=torch.int64, device=DEV)
    for call in (1, 2):
        idx, cnt = grid.index(to, td, tz, live_acc=acc)
        assert idx.dtype == torch.int64 and cnt.dtype == torch.int64 and idx.numel() == n
        assert int(cnt[0]) == M and torch.equal(idx[:M], cidx)
        assert bool((idx[M:] == -9).all())  # entries at and past the count are not written
        assert acc.tolist() == [call * M, call * n]  # the accumulator adds up over calls
    if kind == "full":
        assert M == n
    if kind == "random" and n >= 2000:
        assert 0 < M < n


# ---- 3. frames -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("perturb", [0, 1])
@pytest.mark.parametrize("Ns,Ni", [(64, 128), (8, 16), (8, 0)])
def test_fused_frames_equal_the_per_pose_occupancy_render(Ns, Ni, perturb, white, nets, grids64):
    acc = torch.zeros(2, dtype=torch.int64, device=DEV)
    got = FU.fused(nets, FU.KHW, Ns, Ni, perturb, white, occupancy=grids64, live_acc=acc, rows=True)
    want, live, total = FU.per_pose(nets, FU.KHW, Ns, Ni, perturb, white, grids64)
    FU.assert_same_frames(got, want, Ni)
    K, H, W = FU.KHW
    assert total == K * H * W * (Ns + (Ns + Ni if Ni else 0)) and acc.tolist() == [live, total]
    assert 0.05 < live / total < 0.95, live / total  # the poses look at the scene: both kinds of samples
    from r2l_amd.render import frame_rays
    o, d, _ = frame_rays(FU.poses(K), H, W, FU.FOCAL)
    assert torch.equal(got["rows"], torch.cat([o, d, got["rgb"]], -1))  # rows = [o, d, rgb]


@pytest.mark.parametrize("perturb", [0, 1])
def test_fused_frames_without_a_fine_net(perturb, nets, grids64):
    """network_fine None: the coarse net and ITS grid serve both passes."""
    pair = (grids64[0], grids64[0])
    acc = torch.zeros(2, dtype=torch.int64, device=DEV)
    got = FU.fused(nets, FU.KHW, 64, 128, perturb, True, occupancy=pair, live_acc=acc, fine=False)
    want, live, total = FU.per_pose(nets, FU.KHW, 64, 128, perturb, True, pair, fine=False)
    FU.assert_same_frames(got, want, 128)
    assert acc.tolist() == [live, total]


def test_one_odd_frame(nets, grids64):
    khw = (1, 33, 31)
    acc = torch.zeros(2, dtype=torch.int64, device=DEV)
    got = FU.fused(nets, khw, 64, 128, 1, False, occupancy=grids64, live_acc=acc)
    want, live, total = FU.per_pose(nets, khw, 64, 128, 1, False, grids64)
    FU.assert_same_frames(got, want, 128)
    assert acc.tolist() == [live, total]


def test_grouping_and_chunking_do_not_change_the_frames(nets, grids64):
    names = ("rgb", "disp", "acc", "depth", "rgb0")
    K = FU.KHW[0]
    acc = torch.zeros(2, dtype=torch.int64, device=DEV)
    whole = FU.fused(nets, FU.KHW, 64, 128, 1, True, occupancy=grids64, live_acc=acc)
    ones = [FU.fused(nets, FU.KHW, 64, 128, 1, True, occupancy=grids64, K=1, first=k, frame_id0=FU.FID0 + k) for k in range(K)]
    for n in names:
        assert FU.same(whole[n], torch.cat([f[n] for f in ones], 0)), n
    for chunk in (100, 480):  # 480 = H * W: one pass; 100: five passes, the last of 80 rays
        acc2 = torch.zeros(2, dtype=torch.int64, device=DEV)
        part = FU.fused(nets, FU.KHW, 64, 128, 1, True, occupancy=grids64, live_acc=acc2, chunk=chunk, rows=True)
        for n in names:
            assert FU.same(whole[n], part[n]), (n, chunk)
        assert acc2.tolist() == acc.tolist()
        assert torch.equal(part["rows"][:, 6:], part["rgb"])


def test_frames_without_occupancy_are_unchanged(nets):
    """render_frames without occupancy= is the same call as before: the stages of the unskipped per-pose render, bit for bit."""
    got = FU.fused(nets, FU.KHW, 64, 128, 1, True)
    want, _, _ = FU.per_pose(nets, FU.KHW, 64, 128, 1, True, None)
    FU.assert_same_frames(got, want, 128)


@pytest.mark.parametrize("white", [False, True])
def test_all_empty_grid_on_inside_rays_gives_the_background(white, nets):
    """Every sample inside an all-empty box: no workgroup of the point network does anything, the frame is the background."""
    big = OC.OccupancyGrid([-16.] * 3, [16.] * 3, G=4, k=1, dilate=0).set_bits(np.zeros(OC.n_words(4), np.uint32), device=DEV)
    acc = torch.zeros(2, dtype=torch.int64, device=DEV)
    got = FU.fused(nets, FU.KHW, 64, 128, 1, white, occupancy=(big, big), live_acc=acc)
    K, H, W = FU.KHW
    assert acc.tolist() == [0, K * H * W * (64 + 192)]
    assert bool((got["rgb"] == (1. if white else 0.)).all()) and bool((got["acc"] == 0).all()) and bool((got["rgb0"] == got["rgb"]).all())


# ---- 4. agreement with the unskipped frames ----------------------------------------------------------------------------------------
def _check_miss_report(rep, cap=MISS_CAP):
    """The bound and the condition of tests/test_occupancy_gpu.py::test_agreement_with_the_full_render."""
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


@pytest.mark.parametrize("white", [False, True])
def test_agreement_with_the_unskipped_frames(white, nets, grids64):
    from r2l_amd.render import frame_rays
    K, H, W = FU.KHW
    o, d, v = frame_rays(FU.poses(K), H, W, FU.FOCAL)
    one = torch.ones_like(o[:, :1])
    rays = torch.cat([o, d, NEAR * one, FAR * one, v], -1)
    rep = OC.miss_report(rays, nets[0], nets[1], grids64, 64, 128, white_bkgd=white)
    _check_miss_report(rep)  # the condition: the parent's per-pose path stays inside the cap on these rays
    full = FU.fused(nets, FU.KHW, 64, 128, 0, white)
    skip = FU.fused(nets, FU.KHW, 64, 128, 0, white, occupancy=grids64)
    for name in ("rgb", "acc", "depth"):
        assert torch.equal(full[name].cpu(), rep["full"][name]), name  # the report's rays ARE the frames' rays
    rep["full"] = {k: full[k].cpu() for k in ("rgb", "acc", "depth")}
    rep["skip"] = {k: skip[k].cpu() for k in ("rgb", "acc", "depth")}
    _check_miss_report(rep)
    assert float(skip["acc"].max()) > 0.5  # the rays do hit the scene


# ---- 5. drivers --------------------------------------------------------------------------------------------------------------------
def _teacher_ckpt(tmp_path):
    csd, fsd = trained_like_pair()
    ck = str(tmp_path / "teacher.tar")
    torch.save({"global_step": 200000, "network_fn_state_dict": csd, "network_fine_state_dict": fsd}, ck)
    return ck, csd, fsd


OCC = ["--r2l_occ_res", "64", "--r2l_occ_bound", str(BOX)]


def _live_line(log):
    line = [l for l in log.splitlines() if "live points" in l]
    assert len(line) == 1, line
    a, b = [int(x) for x in line[0].split("live points ")[1].split(" (")[0].split(" / ")]
    return a, b


def test_create_data_fused_against_the_per_pose_switch(tmp_path, monkeypatch):
    """create_data --r2l_fused_frames --r2l_occ_fused next to create_data --r2l_occupancy and to the full run, two 64 x 64 poses at
    --perturb 0 --no_rand_focal: the same shard shapes, the same rays, rgb within the miss bound against the full run."""
    from r2l_amd import create_data
    from tests.test_driver_cpu import ROOT, make_scene
    monkeypatch.chdir(tmp_path)
    ck, csd, fsd = _teacher_ckpt(tmp_path)
    scene = str(tmp_path / "scene")
    os.makedirs(scene)
    make_scene(scene, size=128)
    rows, logs = {}, {}
    for tag, extra in (("full", ["--r2l_fused_frames"]), ("occ", ["--r2l_occupancy"] + OCC),
                       ("fused", ["--r2l_fused_frames", "--r2l_occ_fused"] + OCC)):
        kd = str(tmp_path / ("kd_" + tag))
        out = create_data.main(["--create_data", "rand", "--config", os.path.join(ROOT, "configs", "lego.txt"), "--datadir", scene,
                                "--teacher_ckpt", ck, "--n_pose_kd", "2", "--create_data_chunk", "2", "--datadir_kd", scene + ":" + kd,
                                "--experiment_name", "occf_" + tag, "--perturb", "0", "--no_rand_focal"] + extra)
        rows[tag] = [np.load(os.path.join(kd, f)) for f in sorted(os.listdir(kd))]
        logs[tag] = open(os.path.join(out["logger"].log_path, "log.txt")).read()
    assert [r.shape for r in rows["fused"]] == [r.shape for r in rows["occ"]] == [r.shape for r in rows["full"]] == [(4096, 9)] * 2
    full, occ, fused = (np.concatenate(rows[t]) for t in ("full", "occ", "fused"))
    assert np.array_equal(full[:, :3].view(np.uint32), fused[:, :3].view(np.uint32))
    assert np.array_equal(full[:, 3:6].view(np.uint32), fused[:, 3:6].view(np.uint32))  # the same rays in the same places
    assert np.array_equal(occ[:, :3], fused[:, :3]) and np.abs(occ[:, 3:6] - fused[:, 3:6]).max() < 1e-6  # (render()'s own rays)
    assert logs["fused"].count("occupancy grid (") == 2 and "occupancy grid" not in logs["full"] and "live points" not in logs["full"]
    a, b = _live_line(logs["fused"])
    assert b == 2 * 64 * 64 * (64 + 64 + 128) and 0 < a < b
    # the miss bound on these very rays (white background, as configs/lego.txt renders them)
    pair = [_module(sd) for sd in (csd, fsd)]
    grids = tuple(OC.OccupancyGrid([-BOX] * 3, [BOX] * 3, G=64).build(n) for n in pair)
    o, d = torch.from_numpy(full[:, 0:3].copy()).to(DEV), torch.from_numpy(full[:, 3:6].copy()).to(DEV)
    one = torch.ones(o.shape[0], 1, device=DEV)
    rays = torch.cat([o, d, 2. * one, 6. * one, d / torch.norm(d, dim=-1, keepdim=True)], -1)
    rep = OC.miss_report(rays, pair[0], pair[1], grids, 64, 128, white_bkgd=True)
    lost = rep["lost"]
    drgb = (torch.from_numpy(fused[:, 6:9].copy()).double() - torch.from_numpy(full[:, 6:9].copy()).double()).abs().amax(-1)
    assert bool((drgb <= 2. * lost + 1e-5).all())
    # (the per-pose switch renders render()'s own rays, which differ from the frames' in the last bits, so the two occupancy runs
    # are not compared bit for bit: tests/test_occupancy_gpu.py holds its rgb to the full per-pose run on its own rays)
    clean = (rep["misses"] == 0).numpy()
    assert np.array_equal(fused[clean, 6:9].view(np.uint32), full[clean, 6:9].view(np.uint32))


@pytest.mark.parametrize("compact", [False, True])
def test_online_kd_fill_with_the_switch(compact, tmp_path, monkeypatch):
    """main.py --r2l_online_kd --r2l_occ_fused: the fill run twice gives torch.equal stores (the grid build is deterministic); the
    log has the two build lines and exactly one 'live points a / b' line with 0 < a < b; a run without the switch has neither."""
    from r2l_amd import raystore as R
    stores, logs = {}, {}
    monkeypatch.chdir(tmp_path)
    ck, _, _ = _teacher_ckpt(tmp_path)
    files = {t: str(tmp_path / (t + ".r2l")) for t in ("a", "plain")}
    for tag, extra in (("a", ["--r2l_occ_fused", "--r2l_store_save", files["a"]] + OCC), ("b", ["--r2l_occ_fused"] + OCC),
                       ("plain", ["--r2l_store_save", files["plain"]])):
        res = FU.online_kd_run(tmp_path, ck, tag, extra + (["--r2l_compact_store"] if compact else []))
        stores[tag], logs[tag] = res
    # the store file says how it was rendered, only under the switch
    assert R.read_store_header(files["a"])["provenance"]["occupancy"] == {"res": 64, "bound": BOX, "k": 2, "dilate": 1}
    assert "occupancy" not in R.read_store_header(files["plain"])["provenance"]
    assert len(stores["a"]) > 0 and all(torch.equal(x, y) for x, y in zip(stores["a"], stores["b"]))
    assert [x.shape for x in stores["a"]] == [x.shape for x in stores["plain"]]  # (another run, the same layout)
    for tag in ("a", "b"):
        assert logs[tag].count("occupancy grid (") == 2
        a, b = _live_line(logs[tag])
        assert 0 < a < b
    assert "occupancy grid" not in logs["plain"] and "live points" not in logs["plain"]


def test_store_save_and_render_only_with_the_switch(tmp_path, monkeypatch):
    """utils/create_data.py --r2l_store_save --r2l_occ_fused (the fill builds the pair and logs its share once) and main.py
    --model_name nerf --render_only --render_test --r2l_fused_frames --r2l_occ_fused (one line at the end of the test render)."""
    from r2l_amd import create_data, driver
    from r2l_amd import raystore as R
    from tests.test_driver_cpu import ROOT, make_scene
    monkeypatch.chdir(tmp_path)
    ck, _, _ = _teacher_ckpt(tmp_path)
    scene = str(tmp_path / "scene")
    os.makedirs(scene)
    make_scene(scene, size=128)
    F = str(tmp_path / "cd.r2l")
    out = create_data.main(["--create_data", "rand", "--config", os.path.join(ROOT, "configs", "lego.txt"), "--datadir", scene,
                            "--teacher_ckpt", ck, "--n_pose_kd", "2", "--create_data_chunk", "2", "--experiment_name", "occf_store",
                            "--r2l_store_save", F, "--r2l_occ_fused"] + OCC)
    log = open(os.path.join(out["logger"].log_path, "log.txt")).read()
    assert out["n_rays"] == 2 * 4096 and log.count("occupancy grid (") == 2
    a, b = _live_line(log)
    assert b == 2 * 4096 * (64 + 64 + 128) and 0 < a < b
    assert R.read_store_header(F)["provenance"]["occupancy"] == {"res": 64, "bound": BOX, "k": 2, "dilate": 1}
    res = driver.main(["--model_name", "nerf", "--config", os.path.join(ROOT, "configs", "lego.txt"), "--datadir", scene,
                       "--pretrained_ckpt", ck, "--testskip", "1", "--render_only", "--render_test", "--r2l_fused_frames",
                       "--r2l_occ_fused", "--experiment_name", "Test__NeRF__occ_fused"] + OCC)
    log = open(os.path.join(res["logger"].log_path, "log.txt")).read()
    n = res["rgbs"].shape[0]
    assert res["rgbs"].shape[1:] == (64, 64, 3) and np.isfinite(res["misc"]["test_psnr"].item())
    assert "teacher frames: fused" in log and log.count("occupancy grid (") == 2
    a, b = _live_line(log)
    assert b == n * 4096 * (64 + 64 + 128) and 0 < a < b


# ---- 6. argument refusals ----------------------------------------------------------------------------------------------------------
def test_argument_refusals_launch_nothing(nets):
    """Every refusal of the new calls: hipErrorInvalidValue, the argument named (the table runs on dummy pointers, which would
    fault if a kernel read them), and real buffers keep their sentinel."""
    assert FU.check_refusals() >= 35
    from r2l_amd import engine
    from r2l_amd.render import teacher_engine
    lib, p = _lib.load(), _lib.ptr
    eng = teacher_engine(nets[0])
    eng.ensure_packed()
    grid = U.grid_with_bits(5, "full", device=DEV)
    buf = torch.full((256,), 7.5, device=DEV)
    idx = torch.full((64,), -3, dtype=torch.int64, device=DEV)
    cfg = ctypes.byref(engine.merged_config(eng.cfg))
    st = _lib.stream()
    assert lib.r2l_teacher_mlp_live_cfg(p(buf), p(buf), p(buf), p(buf), p(idx), p(idx), p(eng.wstream), p(eng.flat), p(buf), 4, 0, st,
                                        cfg) == U.INVALID  # S < 1
    assert lib.r2l_teacher_mlp_live_cfg(p(buf), p(buf), p(buf), p(buf), p(idx), p(idx), p(eng.wstream), p(eng.flat),
                                        ctypes.c_void_p(buf.data_ptr() + 4), 2, 2, st, cfg) == U.INVALID  # misaligned raw
    assert lib.r2l_occ_index(ctypes.byref(grid.desc()), p(buf), p(buf), p(buf), 4, 0, p(idx), p(idx), p(buf), st) == U.INVALID
    assert lib.r2l_occ_live_add(p(idx), -1, p(idx), st) == U.INVALID
    desc = FU.frame_desc(ndc=1)
    assert lib.r2l_teacher_frames_occ_cfg(p(buf), None, 1, ctypes.byref(desc), p(buf), p(buf), p(eng.wstream), p(eng.flat), None, None,
                                          p(buf), p(buf), p(buf), p(buf), p(buf), p(buf), ctypes.byref(grid.desc()), None, p(idx),
                                          p(buf), st, cfg) == U.INVALID
    assert "ndc" in lib.r2l_last_error().decode()
    torch.cuda.synchronize()
    assert bool((buf == 7.5).all()) and bool((idx == -3).all())
