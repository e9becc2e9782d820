"""Early ray termination of the teacher's render (include/r2l_hip.h "early ray termination"; r2l_amd/ert.py), the parts that need
no GPU: the numpy specs against hand-made cases, render_rays(ert=) on CPU tensors against raw2outputs of the masked full raw, the
refusals of the C ABI on dummy pointers, the size queries, the header and the exports."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import r2l_oracle as O
from r2l_amd import _lib
from r2l_amd import ert as E
from r2l_amd import occupancy as OC
from tests import ert_util as EU
from tests import occupancy_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def test_segments_and_check():
    assert E.segments(192, 32) == [(j * 32, j * 32 + 32) for j in range(6)]
    assert E.segments(20, 8) == [(0, 8), (8, 16), (16, 20)] and E.segments(16, 64) == [(0, 16)]
    assert E.check(1e-3, 32) == (1e-3, 32) and E.check(0.1, 8) == (0.1, 8)
    for eps, seg, needle in ((0., 32, "eps"), (-1e-3, 32, "eps"), (0.2, 32, "eps"), (float("nan"), 32, "eps"), (1e-3, 7, "seg")):
        with pytest.raises(ValueError, match=needle):
            E.check(eps, seg)


def test_index_seg_spec_by_hand():
    """3 rays x 5 samples on a 4^3 grid over [-1, 1)^3 with the cell (2, 2, 2) set; rays along +x from x = -1.25."""
    occ = np.zeros((4, 4, 4), dtype=bool)
    occ[2, 2, 2] = True
    g = U.grid_with_bits(4, "empty").set_bits(OC.pack_bits(occ))
    grid = (g.words(), g.lo, g.inv, g.G)
    o = np.array([[-1.25, .25, .25]] * 3, dtype=F32)
    d = np.array([[1., 0., 0.]] * 3, dtype=F32)
    z = np.array([[0., .5, 1., 1.5, 2.5]] * 3, dtype=F32)  # x = -1.25 (outside), -.75, -.25 (empty), .25 (cell 2: set), 1.25 (outside)
    M, idx = E.index_seg_spec(grid, o, d, z, 0, 5)
    assert M == 9 and idx.tolist() == [0, 3, 4, 5, 8, 9, 10, 13, 14] and idx.dtype == np.int64
    M, idx = E.index_seg_spec(grid, o, d, z, 1, 4)  # the segment's samples only
    assert idx.tolist() == [3, 8, 13]
    M, idx = E.index_seg_spec(None, o, d, z, 3, 4)  # no grid, width 1
    assert idx.tolist() == [3, 8, 13]
    # termination: below eps out, exactly eps in, NaN in, 0 out
    eps = F32(1e-3)
    M, idx = E.index_seg_spec(None, o, d, z, 2, 5, trans=np.array([np.nextafter(eps, F32(0)), eps, np.nan], dtype=F32), eps=eps)
    assert idx.tolist() == [7, 8, 9, 12, 13, 14]
    M, idx = E.index_seg_spec(grid, o, d, z, 2, 5, trans=np.array([0., 1., 0.5], dtype=F32), eps=eps)
    assert idx.tolist() == [8, 9, 13, 14]
    M, idx = E.index_seg_spec(grid, o, d, z, 0, 5, trans=np.zeros(3, dtype=F32), eps=eps)
    assert M == 0 and idx.size == 0
    with pytest.raises(ValueError):
        E.index_seg_spec(None, o, d, z, 2, 6)


def test_advance_spec_by_hand():
    """One ray with |d| = 2: the factors by hand, the chain rule of the pinned order, the last interval's 1e10."""
    raw = np.zeros((1, 4, 4), dtype=F32)
    raw[0, :, 3] = [-5., 1., 0.5, 1e-12]
    z = np.array([[1., 1.5, 2.5, 3.]], dtype=F32)
    d = np.array([[0., 2., 0.]], dtype=F32)
    f = E.factors_spec(raw, z, d, np.float64)
    want = [1. + 1e-10, np.exp(-1. * 1. * 2.) + 1e-10, np.exp(-.5 * .5 * 2.) + 1e-10, np.exp(-float(F32(1e-12)) * 1e10 * 2.) + 1e-10]
    assert np.allclose(f[0], want, rtol=1e-15)
    T = E.advance_spec(raw, z, d, 0, 4, dtype=np.float64)
    assert np.isclose(T[0], np.prod(want), rtol=1e-14)
    for dt in (F32, np.float64):
        a = E.advance_spec(raw, z, d, 0, 2, dtype=dt)
        b = E.advance_spec(raw, z, d, 2, 4, trans=a, dtype=dt)
        assert b.dtype == dt and np.array_equal(b, E.advance_spec(raw, z, d, 0, 4, dtype=dt))  # chained = one call, bit for bit
        assert np.array_equal(E.advance_spec(raw, z, d, 0, 2, trans=np.full(1, 7.), dtype=dt), a)  # s0 == 0 ignores trans
    f32 = E.factors_spec(raw, z, d, F32)
    assert f32.dtype == F32 and np.abs(f32.astype(np.float64) - f).max() < 2.**-22
    # a huge sigma: alpha = 1, the factor is the 1e-10 floor
    raw[0, 1, 3] = 1000.
    assert E.advance_spec(raw, z, d, 0, 2)[0] == F32(1e-10)


def test_ert_mask():
    t = [np.array([1., 5e-4, np.nan], dtype=F32), np.array([.5, 0., 1e-3], dtype=F32)]
    m = E.ert_mask(t, 20, 8, 1e-3)
    assert m.shape == (3, 20) and m[:, :8].all()
    assert m[:, 8:16].tolist() == [[True] * 8, [False] * 8, [True] * 8]
    assert m[:, 16:].tolist() == [[True] * 4, [False] * 4, [True] * 4]  # exactly eps stays


def _teacher_pair(lift=0.5):
    """Init-distribution nets with the sigma bias lifted, so that the rays do become opaque along their way."""
    from r2l_amd.nerf_raybased import NeRF
    nets = []
    for sd in O.make_teacher_state_dicts(11, 2, alpha_bias=0.5):
        sd = {k: v.clone() for k, v in sd.items()}
        sd["alpha_linear.bias"] += lift
        m = NeRF(D=8, W=256, input_ch=63, output_ch=4, skips=[4], input_ch_views=27, use_viewdirs=True)
        m.load_state_dict(sd)
        nets.append(m.eval())
    return nets


@pytest.mark.parametrize("NI", [9, 0])
def test_render_rays_cpu_equals_masked_full_raw(NI):
    """render_rays(ert=) on CPU tensors = raw2outputs of the full raw of the last pass, masked by (grid rule) and NOT (the walk's
    own transmittance at the boundary < eps); the coarse outputs are those of the render without ert."""
    from r2l_amd.render import get_embedder, raw2outputs, render_rays, run_network, sample_pdf_sort
    from tests.teacher_util import scene_rays
    torch.manual_seed(0)
    coarse, fine = _teacher_pair()
    e10, e4 = get_embedder(10)[0], get_embedder(4)[0]
    qfn = lambda pts, vd, fn: run_network(pts, vd, fn, embed_fn=e10, embeddirs_fn=e4)
    rays = scene_rays(181 * 181, 0)[::1501][:21].contiguous()
    R, S, seg, eps = rays.shape[0], 12, 8, 0.042  # (the transmittance of these rays at sample 8 / 16 runs from 0.03 to 0.05: a mix)
    T = S + NI
    for with_grid in (False, True):
        occ = None
        if with_grid:
            grids = []
            for net in (coarse, fine):
                g = OC.OccupancyGrid([-1.6] * 3, [1.6] * 3, G=6, k=1, dilate=0, sigma_thresh=0.).build(net, keep_sigma=True)
                g = OC.OccupancyGrid([-1.6] * 3, [1.6] * 3, G=6, k=1, dilate=0, sigma_thresh=float(g.sigma.median())).build(net)
                grids.append(g)
            occ = tuple(grids)
        acc = torch.zeros(2, dtype=torch.int64)
        kw = dict(N_importance=NI, network_fine=fine, perturb=0., retraw=True, occupancy=occ)
        got = render_rays(rays, coarse, qfn, S, ert=(eps, seg), live_acc=acc, **kw)
        plain = render_rays(rays, coarse, qfn, S, **kw)
        o, d, vd = rays[:, 0:3], rays[:, 3:6], rays[:, 8:11]
        t = torch.linspace(0., 1., S)
        z = (rays[:, 6:7] * (1. - t) + rays[:, 7:8] * t).contiguous()
        net, grid = coarse, (occ[0] if occ else None)
        if NI:
            for name in ("rgb0", "acc0", "z_std"):
                assert torch.equal(got[name], plain[name]), name  # the coarse pass is untouched
            pts = o[:, None, :] + d[:, None, :] * z[:, :, None]
            with torch.no_grad():
                raw0 = qfn(pts, vd, coarse)
            if occ:
                live0 = OC.live_spec(occ[0].words(), occ[0].lo, occ[0].inv, occ[0].G, OC.sample_points(o.numpy(), d.numpy(), z.numpy()).reshape(-1, 3))
                raw0 = torch.where(torch.from_numpy(live0).reshape(z.shape)[..., None], raw0, torch.zeros_like(raw0))
            w0 = raw2outputs(raw0, z, d)[3]
            z = sample_pdf_sort(z, w0, NI, det=True)[1]
            net, grid = fine, (occ[1] if occ else None)
        pts = torch.from_numpy(OC.sample_points(o.numpy(), d.numpy(), z.numpy()))
        with torch.no_grad():
            full = qfn(pts, vd, net)
        trans_at = [x.numpy() for x in got["ert_trans"]]
        assert len(trans_at) == len(E.segments(T, seg)) - 1
        tmask, gmask = E.ert_mask(trans_at, T, seg, eps), np.ones((R, T), dtype=bool)
        if grid is not None:
            gmask = OC.live_spec(grid.words(), grid.lo, grid.inv, grid.G, pts.numpy().reshape(-1, 3)).reshape(R, T)
        mask = tmask & gmask
        want_raw = torch.where(torch.from_numpy(mask)[..., None], full, torch.zeros_like(full))
        assert torch.equal(got["raw"], want_raw)
        rgb, disp, acc_map, _, depth = raw2outputs(want_raw, z, d)
        for name, want in (("rgb_map", rgb), ("acc_map", acc_map), ("depth_map", depth)):
            assert torch.equal(got[name], want), name
        assert U.same_bits(got["disp_map"], disp)
        # the transmittances are those of the masked raw itself (a skipped sample never enters a later one), and some ray stops
        for (s0, s1), tr in zip(E.segments(T, seg)[:-1], trans_at):
            assert np.array_equal(tr, E.advance_spec(want_raw.numpy(), z.numpy(), d.numpy(), 0, s1))
        behind = tmask[:, seg:]  # both kinds of samples behind the first boundary: evaluated and skipped
        if not with_grid:  # (these grids cut density away at its median: behind them fewer rays become opaque)
            assert behind.any() and not behind.all(), "nothing (or everything) is skipped: the case shows nothing"
        assert acc.tolist()[1] == R * T and 0 < acc.tolist()[0] <= int(mask.sum()) and (with_grid or acc.tolist()[0] < R * T)
        # the bound: |d rgb| <= T_cut (+ slack of two fp32 sums)
        ref = raw2outputs(torch.where(torch.from_numpy(gmask)[..., None], full, torch.zeros_like(full)), z, d)[0]
        assert torch.equal(ref, plain["rgb_map"])  # (the render without ert on the same grids)
        t_cut = np.zeros(R)
        for tr in reversed(trans_at):
            t_cut = np.where(tr < F32(eps), tr, t_cut)
        assert bool(((got["rgb_map"] - ref).abs().amax(-1).double().numpy() <= t_cut * (1 + 1e-3) + 4 * T * 2.**-24).all())
    with pytest.raises(ValueError, match="raw_noise_std"):
        render_rays(rays, coarse, qfn, S, raw_noise_std=1., ert=(eps, seg))
    with pytest.raises(ValueError, match="viewdirs"):
        render_rays(rays[:, :8], coarse, qfn, S, ert=(eps, seg))
    with pytest.raises(ValueError, match="seg"):
        render_rays(rays, coarse, qfn, S, ert=(eps, 0))
    with pytest.raises(ValueError, match="live_acc"):
        render_rays(rays, coarse, qfn, S, live_acc=torch.zeros(2, dtype=torch.int64))


def test_abi_argument_checks():
    """Every refusal of the four new calls is hipErrorInvalidValue with the argument named, before any launch (dummy pointers)."""
    assert EU.check_refusals() >= 60


def test_header_exports_and_struct():
    names = ["r2l_occ_index_seg_work_bytes", "r2l_occ_index_seg", "r2l_ert_advance", "r2l_teacher_mlp_live_into_cfg",
             "r2l_teacher_frames_ert_work_floats", "r2l_teacher_frames_ert_cfg"]
    header = open(os.path.join(ROOT, "include", "r2l_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert re.search(r"\b%s\(" % n, header) and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert "typedef struct r2l_ert_desc" in header
    S = _lib.ErtDesc
    assert ctypes.sizeof(S) == 16 and [getattr(S, f).offset for f, _ in S._fields_] == [0, 4, 8]


def test_flag_refusals(tmp_path):
    """--r2l_ert EPS / --r2l_ert_seg W: every refusal is a ValueError that names the flag, before anything is loaded."""
    from r2l_amd import options
    cd = ("r2l_fused_frames", "r2l_store_save")
    base = ["--use_viewdirs", "--r2l_ert", "1e-3"]
    a = options.parse_args(["--use_viewdirs"])
    assert a.r2l_ert == 0. and a.r2l_ert_seg == 32 and options.validate_ert(a, cd) is None  # off: nothing is checked
    assert options.validate_ert(options.parse_args(["--r2l_ert_seg", "2", "--r2l_occupancy"]), cd) is None
    assert options.validate_ert(options.parse_args(base + ["--r2l_fused_frames"]), cd) == (1e-3, 32)
    assert options.validate_ert(options.parse_args(base + ["--r2l_store_save", "s.r2l", "--r2l_ert_seg", "64"]), cd) == (1e-3, 64)
    assert options.validate_ert(options.parse_args(base + ["--r2l_fused_frames", "--r2l_occ_fused"]), cd) == (1e-3, 32)  # with the grids
    # forward-facing scenes: without the grids only
    llff = base + ["--r2l_fused_frames", "--dataset_type", "llff", "--r2l_llff"]
    assert options.validate_ert(options.parse_args(llff), cd) == (1e-3, 32)
    options.validate_occ_fused(options.parse_args(llff), cd)
    with pytest.raises(ValueError, match="llff"):
        options.validate_occ_fused(options.parse_args(llff + ["--r2l_occ_fused"]), cd)
    cfg = tmp_path / "c.txt"
    cfg.write_text("use_viewdirs = True\nr2l_fused_frames = True\nr2l_ert = 0.01\nr2l_ert_seg = 16\n")  # config keys too
    assert options.validate_ert(options.parse_args(["--config", str(cfg)]), cd) == (0.01, 16)
    fused = ["--r2l_fused_frames"]
    for extra, needle in (([], "r2l_fused_frames or --r2l_store_save"), (fused + ["--r2l_occupancy"], "r2l_occupancy"),
                          (fused + ["--raw_noise_std", "1"], "raw_noise_std"), (fused + ["--r2l_ert_seg", "7"], "r2l_ert_seg"),
                          (fused + ["--r2l_ert", "0.2"], "r2l_ert"), (fused + ["--r2l_ert", "-0.001"], "r2l_ert")):
        with pytest.raises(ValueError, match=needle) as e:
            options.validate_ert(options.parse_args(base + extra), cd)
        assert "--r2l_ert" in str(e.value)
    with pytest.raises(ValueError, match="use_viewdirs"):
        options.validate_ert(options.parse_args(["--r2l_ert", "1e-3", "--r2l_fused_frames"]), cd)
    with pytest.raises(ValueError, match="use_viewdirs"):
        options.validate_ert(options.parse_args(base + ["--r2l_online_kd"]), ("r2l_online_kd",), use_viewdirs=False)
    options.validate_ert(options.parse_args(base + fused + ["--raw_noise_std", "1"]), cd, raw_noise_std=0.)  # the test render: no noise
    # the drivers raise at start-up
    from r2l_amd import create_data, driver
    with pytest.raises(ValueError, match="r2l_fused_frames"):
        create_data.main(base + ["--create_data", "rand"])
    with pytest.raises(ValueError, match="r2l_ert_seg"):
        create_data.main(base + ["--create_data", "rand", "--r2l_fused_frames", "--r2l_ert_seg", "4"])
    with pytest.raises(ValueError, match="r2l_fused_frames"):
        driver.main(base + ["--model_name", "nerf", "--render_only"])
    with pytest.raises(ValueError, match="r2l_online_kd"):
        driver.main(["--r2l_ert", "1e-3", "--model_name", "R2L"])
