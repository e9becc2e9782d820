"""Ray culling (--r2l_ray_cull; include/r2l_hip.h r2l_occ_rays / r2l_store_append_live; r2l_amd/ray_cull.py), the parts that need
no GPU: the numpy restatements against hand-made cases, cull_steps and the coverage property it exists for, the options table, the
exports and the header text, the checkpoint entry."""
import argparse
import ctypes
import os

import numpy as np
import pytest
import torch

from r2l_amd import _lib
from r2l_amd import occupancy as OC
from tests import ray_cull_util as RU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ---- rays_spec -----------------------------------------------------------------------------------------------------------------------
def _any_over_compact(grid, o, d, near, far, T):
    z = np.broadcast_to(OC.ray_depths(near, far, T)[None], (o.shape[0], T))
    _, n, *_ = OC.compact_spec(grid.words(), grid.lo, grid.inv, grid.G, o, d, o, z)
    live = np.zeros(o.shape[0], np.uint8)
    live[np.unique(n // T)] = 1
    return live


def test_ray_depths_arithmetic():
    t = OC.ray_depths(2., 6., 8)
    assert t.dtype == F32 and np.array_equal(t, np.arange(8, dtype=F32) * F32(.5) + F32(2.25))
    dt = F32(F32(1.7) - F32(0.3)) / F32(7)
    assert np.array_equal(OC.ray_depths(0.3, 1.7, 7), F32(0.3) + (np.arange(7, dtype=F32) + F32(.5)) * dt)
    assert np.array_equal(OC.ray_depths(3., 3., 4), np.full(4, 3., F32))  # near == far
    for bad in ((2., 6., 0), (6., 2., 4), (float("nan"), 1., 4), (0., float("inf"), 4)):
        with pytest.raises(ValueError):
            OC.ray_depths(*bad)


def test_rays_spec_on_a_hand_made_grid():
    """4^3 cells over [-1, 1): only cell (cx, cy, cz) = (3, 0, 0) is set."""
    occ = np.zeros((4, 4, 4), bool)
    occ[0, 0, 3] = True
    g = OC.OccupancyGrid([-1.] * 3, [1.] * 3, G=4, k=1, dilate=0).set_bits(OC.pack_bits(occ))
    o = np.array([[-.9, -.9, -.9],   # along +x through row (y, z) = (0, 0): hits cell 3 at x >= 0.5
                  [-.9, -.4, -.9],   # row y = 1: clear all the way
                  [-.9, -.9, -.9],   # the same start, but so short that it ends before cell 3
                  [-.9, -.9, -.9],   # leaves the box: outside is live
                  [np.nan, 0., 0.],  # not finite: live
                  [.6, -.9, -.9]], F32)  # the step jumps over nothing: starts inside cell 3
    d = np.array([[1.8, 0, 0], [1.8, 0, 0], [1.2, 0, 0], [2.5, 0, 0], [1, 0, 0], [0, 0, 0]], F32)
    M, idx, live = RU.spec(g, o, d, 0., 1., 4)
    assert live.tolist() == [1, 0, 0, 1, 1, 1] and idx.tolist() == [0, 3, 4, 5] and M == 4 and idx.dtype == np.int64
    # T = 1 samples the middle only: ray 0's midpoint (x = 0) is in a clear cell
    assert RU.spec(g, o, d, 0., 1., 1)[2].tolist() == [0, 0, 0, 0, 1, 1]


@pytest.mark.parametrize("G,kind", [(5, "empty"), (5, "full"), (8, "random"), (37, "random")])
def test_rays_spec_is_any_over_compact_spec(G, kind):
    g = RU.grid_with_bits(G, kind)
    o, d = RU.cull_rays(300, G)
    for near, far, T in ((0., 2., G), (0., 2., 2 * G + 1), (.5, .5, 3), (0., 3., 1)):
        M, idx, live = RU.spec(g, o, d, near, far, T)
        want = _any_over_compact(g, o, d, near, far, T)
        assert np.array_equal(live, want) and np.array_equal(idx, np.flatnonzero(want)) and M == int(want.sum())
    if kind == "full":
        assert M == 300
    if kind == "empty":
        oi, di = RU.inside_rays(64)
        assert RU.spec(g, oi, di, 0., 1., 9)[0] == 0


# ---- cull_steps -----------------------------------------------------------------------------------------------------------------------
def test_cull_steps_arithmetic_and_refusals():
    g = OC.OccupancyGrid([-2.5] * 3, [2.5] * 3, G=128, k=2, dilate=1)
    side = 5. / 128
    for d_max in (1., 1.0625, 1.3):
        T = OC.cull_steps(g, 2., 6., d_max)
        assert 4. / T * d_max <= side and (T == 1 or 4. / (T - 1) * d_max > side)
    assert OC.cull_steps(g, 2., 6., 1.) == 103 and OC.cull_steps(g, 2., 2., 1.) == 1
    assert OC.cull_steps(OC.OccupancyGrid([-1.] * 3, [1.] * 3, G=4, dilate=1), 0., 1., 1.) == 2  # (an exact quotient)
    slab = OC.OccupancyGrid([-1., -1., -1.], [1., 3., 1.], G=8, dilate=2)  # the SMALLEST side counts: 0.25
    assert OC.cull_steps(slab, 0., 1., 1.) == 4
    with pytest.raises(ValueError, match="dilate"):
        OC.cull_steps(OC.OccupancyGrid([-1.] * 3, [1.] * 3, G=8, dilate=0), 0., 1., 1.)
    for bad in ((6., 2., 1.), (2., 6., 0.), (2., float("inf"), 1.)):
        with pytest.raises(ValueError):
            OC.cull_steps(g, *bad)
    assert abs(OC.frame_d_max(400, 400, 555.5555) - np.sqrt(1 + 2 * 0.36**2)) < 1e-6
    # the largest |d| of a frame's rays stays below it
    from r2l_amd.raystore import pixel_ray_spec
    c = np.broadcast_to(np.eye(4, dtype=F32)[None, :3], (4, 3, 4))
    _, d = pixel_ray_spec(c, np.full(4, 30., F32), 20, 24, [0, 0, 19, 19], [0, 23, 0, 23])
    assert np.linalg.norm(d, axis=-1).max() <= OC.frame_d_max(20, 24, 30.)


@pytest.mark.parametrize("G", [8, 16])
def test_no_dead_ray_meets_a_cell_that_was_set_before_the_dilation(G):
    """The property cull_steps exists for: random undilated grids, dilated by one; 500 random rays through and past the box with
    T = cull_steps(...); no dead ray has any of 16 T dense points of its segment in a cell set BEFORE the dilation."""
    rs = np.random.RandomState(G)
    n_dead = 0
    for trial in range(4):
        raw = rs.rand(G, G, G) < (0.02, 0.05, 0.1, 0.3)[trial]
        before = OC.OccupancyGrid([-1.] * 3, [1.] * 3, G=G, k=1, dilate=0).set_bits(OC.pack_bits(raw))
        sigma = np.where(raw, 1., -1.).astype(F32)  # one probe a cell
        after = OC.OccupancyGrid([-1.] * 3, [1.] * 3, G=G, k=1, dilate=1).set_bits(OC.build_spec(sigma, G, 1, dilate=1))
        o = (rs.rand(500, 3) * 2.4 - 1.2).astype(F32)
        d = (rs.randn(500, 3) * 0.6).astype(F32)
        near, far = 0.1, 1.3
        T = OC.cull_steps(after, near, far, float(np.linalg.norm(d, axis=-1).max()))
        _, _, live = RU.spec(after, o, d, near, far, T)
        dead = live == 0
        n_dead += int(dead.sum())
        dense = OC.ray_depths(near, far, 16 * T)
        dense = np.concatenate([[F32(near)], dense, [F32(far)]]).astype(F32)
        pts = OC.sample_points(o[dead], d[dead], np.broadcast_to(dense[None], (int(dead.sum()), dense.size))).reshape(-1, 3)
        # "in a cell set before the dilation": inside the box AND that cell's bit (a point outside the box is in no cell)
        f = np.floor((pts - before.lo) * before.inv)
        inside = ((f >= 0) & (f < G)).all(1)
        hit = inside & OC.live_spec(before.words(), before.lo, before.inv, G, pts)
        assert not hit.any(), (trial, int(hit.sum()))
    assert n_dead >= 20  # the property was exercised


# ---- the options table ---------------------------------------------------------------------------------------------------------------
def _args(*extra):
    from r2l_amd.options import parse_args
    return parse_args(["--config", os.path.join(ROOT, "configs", "lego_noview.txt")] + list(extra))


def test_flag_and_config_key(tmp_path):
    from r2l_amd.options import FLAGS, IGNORED
    assert FLAGS["r2l_ray_cull"] == ("flag", False) and "r2l_ray_cull" not in IGNORED
    assert _args().r2l_ray_cull is False and _args("--r2l_ray_cull").r2l_ray_cull is True
    cfg = tmp_path / "c.txt"
    cfg.write_text("r2l_ray_cull = True\n")
    from r2l_amd.options import parse_args
    assert parse_args(["--config", str(cfg)]).r2l_ray_cull is True


def test_options_acceptances_and_refusals():
    from r2l_amd.options import validate_ray_cull
    T = ["--teacher_ckpt", "t.tar", "--r2l_teacher_config", os.path.join(ROOT, "configs", "lego.txt")]
    KD = ["--r2l_online_kd", "--n_pose_kd", "3"] + T
    validate_ray_cull(_args())  # off: nothing is looked at
    validate_ray_cull(_args("--r2l_compact_store", "--dataset_type", "llff"), "cpu")
    # accepted
    validate_ray_cull(_args("--r2l_ray_cull"), "cuda", ckpt_has_grid=True)  # a render from a checkpoint with the grid
    validate_ray_cull(_args("--r2l_ray_cull", "--render_only", "--render_test"), "cuda", ckpt_has_grid=True)
    validate_ray_cull(_args("--r2l_ray_cull", *T), "cuda", ckpt_has_grid=False)  # ... or from the teacher
    validate_ray_cull(_args("--r2l_ray_cull", "--r2l_occ_fused", *KD), "cuda", ckpt_has_grid=False)
    validate_ray_cull(_args("--r2l_ray_cull", "--r2l_occ_fused", "--r2l_fused_iter", "--r2l_kd_every", "5", *KD), "cuda", ckpt_has_grid=False)
    validate_ray_cull(_args("--r2l_ray_cull", "--r2l_store_load", "s.r2l"), "cuda", ckpt_has_grid=True)
    validate_ray_cull(_args("--r2l_ray_cull", "--r2l_occ_fused", "--r2l_store_save", "s.r2l"), "cuda", entry="create_data")
    # refused, the flag named
    for argv, dev, kw, needle in (
            (["--dataset_type", "llff"], None, {}, "llff"),
            (["--r2l_compact_store", "--r2l_occ_fused"] + KD, None, {}, "r2l_compact_store"),
            ([], "cpu", {}, "CPU"),
            (KD, None, {}, "r2l_occ_fused"),
            ([], "cuda", {"ckpt_has_grid": False}, "teacher_ckpt"),
            (["--teacher_ckpt", "t.tar"], "cuda", {"ckpt_has_grid": False}, "r2l_teacher_config"),
            (["--model_name", "nerf"], None, {}, "model_name nerf"),
            (["--r2l_occ_res", "0"], None, {}, "r2l_occ_res"),
            (["--r2l_store_save", "s.r2l"], None, {"entry": "create_data"}, "r2l_occ_fused"),
            (["--r2l_occ_fused"], None, {"entry": "create_data"}, "r2l_store_save")):
        with pytest.raises(ValueError, match="r2l_ray_cull") as e:
            validate_ray_cull(_args("--r2l_ray_cull", *argv), dev, **kw)
        assert needle in str(e.value), (argv, str(e.value))


def test_the_entry_points_refuse_before_anything_is_loaded(tmp_path, monkeypatch):
    from r2l_amd import create_data, driver, train_nerf  # noqa: F401
    monkeypatch.chdir(tmp_path)
    base = ["--config", os.path.join(ROOT, "configs", "lego_noview.txt"), "--datadir", str(tmp_path / "nowhere")]
    kd = ["--r2l_online_kd", "--n_pose_kd", "3", "--teacher_ckpt", "t.tar", "--r2l_teacher_config", os.path.join(ROOT, "configs", "lego.txt")]
    with pytest.raises(ValueError, match="r2l_ray_cull.*r2l_compact_store"):
        driver.main(base + ["--model_name", "R2L", "--r2l_ray_cull", "--r2l_compact_store", "--r2l_occ_fused"] + kd)
    with pytest.raises(ValueError, match="r2l_ray_cull.*llff"):
        driver.main(base + ["--model_name", "R2L", "--r2l_ray_cull", "--dataset_type", "llff", "--r2l_llff"])
    with pytest.raises(ValueError, match="r2l_ray_cull.*r2l_occ_fused"):
        driver.main(base + ["--model_name", "R2L", "--r2l_ray_cull", "--r2l_online_kd", "--n_pose_kd", "3", "--teacher_ckpt", "t.tar",
                            "--r2l_teacher_config", os.path.join(ROOT, "configs", "lego.txt")])
    with pytest.raises(ValueError, match="r2l_ray_cull.*r2l_store_save"):
        create_data.main(base + ["--create_data", "rand", "--r2l_ray_cull"])
    if not torch.cuda.is_available():
        with pytest.raises(ValueError, match="r2l_ray_cull.*CPU"):
            driver.main(base + ["--model_name", "R2L", "--r2l_ray_cull"])


def test_train_nerf_accepts_and_ignores_the_flag(tmp_path, monkeypatch):
    """utils/train_nerf.py with the flag goes exactly as far as without it: here to the scene that is not there."""
    from r2l_amd import train_nerf
    monkeypatch.chdir(tmp_path)
    base = ["--config", os.path.join(ROOT, "configs", "lego.txt"), "--datadir", str(tmp_path / "nowhere"), "--no_batching"]
    ends = []
    for extra in ([], ["--r2l_ray_cull"]):
        with pytest.raises(Exception) as e:
            train_nerf.main(base + ["--experiment_name", "tn%d" % len(extra)] + extra)
        ends.append((type(e.value), str(e.value)))
    assert ends[0] == ends[1] and "r2l_ray_cull" not in ends[1][1] and "nowhere" in ends[1][1]


def test_deferred_grid_and_provenance_mismatch():
    from r2l_amd.ray_cull import RayCull
    g = RU.grid_with_bits(8, "random", lo=(-6., -6., -6.), hi=(6., 6., 6.))
    g.dilate = 1
    late = RayCull.deferred(2., 6.)
    for call in (late.state, lambda: late.steps(64, 64, 80.), lambda: late.provenance(3)):
        with pytest.raises(RuntimeError, match="handed over"):
            call()
    assert late.adopt(g, True) is late and late.grid is g and late.bg == 1.0 and sorted(late.state()) == sorted(RC_FIELDS())
    # every field of the provenance comes from the grid the rows were culled with — the box too
    prov = late.provenance(17)
    assert prov == {"res": 8, "bound": 6., "dilate": 1, "T": 17, "near": 2., "far": 6.}
    assert late.mismatch(prov) == [] and late.mismatch(prov, T=17) == []
    assert late.mismatch(dict(prov, bound=2.5, res=64)) == ["res: file 64, run 8", "bound: file 2.5, run 6.0"]
    assert late.mismatch(prov, T=18) == ["T: file 17, run 18"]


def RC_FIELDS():
    from r2l_amd.ray_cull import STATE_FIELDS
    return STATE_FIELDS


def test_render_path_refuses_the_teacher_branch_and_the_cpu():
    from r2l_amd import driver
    from r2l_amd.ray_cull import RayCull
    cull = RayCull(OC.OccupancyGrid([-1.] * 3, [1.] * 3, G=4, dilate=1).set_bits(np.zeros(2, np.uint32)), 2., 6., True)
    with pytest.raises(ValueError, match="r2l_ray_cull"):
        driver.render_path([], torch.nn.Linear(1, 1), None, torch.device("cpu"), None, ray_cull=cull)


# ---- append_live's restatement ------------------------------------------------------------------------------------------------------
def test_append_live_spec_is_gather_then_append():
    from r2l_amd import raystore as R
    rs = np.random.RandomState(0)
    rows = rs.rand(50, 9).astype(F32)
    idx = np.sort(rs.choice(50, 23, replace=False)).astype(np.int64)
    for rps, shuffle in ((4, True), (4, False), (8, True)):
        got = R.append_live_spec(rows, idx, rps, 77, shuffle)
        g = rows[idx]
        n_out = 23 // rps * rps
        src = R.perm_at(77, 23, np.arange(n_out, dtype=np.uint64)) if shuffle else np.arange(n_out)
        assert got.shape == (n_out, 9) and np.array_equal(got, g[src])
    bad = idx.copy()
    bad[3], bad[9] = 50, -1
    got = R.append_live_spec(rows, bad, 4, 77, False)
    assert np.isnan(got[3]).all() and np.isnan(got[9]).all() and np.array_equal(got[4], rows[idx[4]])
    assert R.append_live_spec(rows, idx[:3], 4, 1).shape == (0, 9)


# ---- exports and header ----------------------------------------------------------------------------------------------------------------
def test_exports_and_header_text():
    lib = _lib.load()
    for name in ("r2l_occ_rays_work_bytes", "r2l_occ_rays", "r2l_store_append_live", "r2l_rays_gather", "r2l_rgb_scatter_bg"):
        assert hasattr(lib, name), name
    text = " ".join(open(os.path.join(ROOT, "include", "r2l_hip.h")).read().replace("\n * ", " ").split())  # (comment lines joined)
    for needle in ("int64_t r2l_occ_rays_work_bytes(int64_t R);",
                   "int r2l_occ_rays(const r2l_occ_grid* grid, const float* rays_o, const float* rays_d, int64_t R, float near, float far, int T,",
                   "t_j = near + ((float)j + 0.5f) * dt", "dt = (far - near) / (float)T", "SPECIFIED BY r2l_occ_index",
                   "within half a cell of a sample", "clear BEFORE the dilation", "d_max = sqrt(1 + (W/(2 f))^2 + (H/(2 f))^2)",
                   "int r2l_store_append_live(const float* rows_in /*[n_rows,9]*/, int64_t n_rows, const int64_t* idx /*[M]*/, int64_t M,",
                   "input row idx[pi(key, M)(i)]", "writes a NaN row and reads nothing", "int r2l_rays_gather(", "int r2l_rgb_scatter_bg("):
        assert needle in text, needle


def test_argument_refusals_on_dummy_pointers():
    assert RU.check_refusals() >= 35
    lib = _lib.load()
    P = ctypes.c_void_p(4096)
    g = _lib.OccGridDesc()
    f3 = lambda *v: (ctypes.c_float * 3)(*v)
    assert lib.r2l_occ_grid_init(ctypes.byref(g), P, 4, 2, f3(-1, -1, -1), f3(1, 1, 1)) == 0
    m = ctypes.c_int64(-1)
    # successful no-ops that touch no memory: m == 0 shards, M == 0 rows
    assert lib.r2l_store_append_live(P, 10, P, 3, P, 4, 0, 4, 5, 1, ctypes.byref(m), None) == 0 and m.value == 0
    assert lib.r2l_store_append_live(P, 10, None, 0, P, 4, 0, 4, 5, 1, ctypes.byref(m), None) == 0 and m.value == 0
    assert lib.r2l_rays_gather(P, P, 5, None, 0, None, None, None) == 0
    assert lib.r2l_rgb_scatter_bg(None, None, 0, None, 1., None, 0, None) == 0


# ---- the checkpoint entry --------------------------------------------------------------------------------------------------------------
def test_checkpoint_key_round_trip(tmp_path):
    from r2l_amd import ray_cull as RC
    from r2l_amd.checkpoint import load_ckpt, save_ckpt
    g = RU.grid_with_bits(37, "random", lo=(-2.5, -2.5, -2.5), hi=(2.5, 2.5, 2.5))
    g.dilate = 1
    cull = RC.RayCull(g, 2., 6., True)
    st = cull.state()
    assert sorted(st) == sorted(RC.STATE_FIELDS) and st["bits"].device.type == "cpu" and st["bits"].dtype == torch.int32
    path = save_ckpt(str(tmp_path / "c.tar"), 3, torch.nn.Linear(2, 2), {}, 0., 0, model_name="other", extra={RC.KEY: st})
    back = RC.RayCull.from_state(load_ckpt(path, map_location="cpu")[RC.KEY])
    assert np.array_equal(back.grid.words(), g.words()) and back.grid.G == 37 and back.grid.k == g.k and back.grid.dilate == 1
    assert np.array_equal(back.grid.lo, g.lo) and np.array_equal(back.grid.inv, g.inv) and np.array_equal(back.grid.hi, g.hi)
    assert (back.near, back.far, back.white_bkgd, back.bg) == (2., 6., True, 1.0)
    assert RC.RayCull(g, 2., 6., False).bg == 0.0
    assert back.steps(400, 400, 555.5555) == OC.cull_steps(g, 2., 6., OC.frame_d_max(400, 400, 555.5555))
    prov = back.provenance(50)
    assert sorted(prov) == ["T", "bound", "dilate", "far", "near", "res"] and prov["res"] == 37 and prov["bound"] == 2.5
    with pytest.raises(ValueError, match="lacks"):
        RC.RayCull.from_state({k: v for k, v in st.items() if k != "near"})
    with pytest.raises(ValueError, match="dilate"):
        RC.RayCull(RU.grid_with_bits(5, "full"), 2., 6., True)  # dilate = 0
