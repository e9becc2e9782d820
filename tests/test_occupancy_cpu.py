"""Occupancy grid of the teacher's render (include/r2l_hip.h "occupancy grid"; r2l_amd/occupancy.py; --r2l_occupancy), the parts
that need no GPU: the three numpy specs against hand-made cases on a 4^3 grid, render_rays(occupancy=...) on CPU tensors against
raw2outputs of the zero-masked full raw, the refusals of the switch and of the C ABI, the header and the exports."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle import r2l_oracle as O
from r2l_amd import occupancy as OC
from tests import occupancy_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _grid4(cells):
    """4^3 grid over [-1, 1)^3 (inv = 2 exactly: cell faces at multiples of 0.5) with the given (cx, cy, cz) cells set."""
    occ = np.zeros((4, 4, 4), dtype=bool)
    for cx, cy, cz in cells:
        occ[cz, cy, cx] = True
    return U.grid_with_bits(4, "empty").set_bits(OC.pack_bits(occ))


def test_fields_and_bit_layout():
    lo, inv, step = OC.grid_fields([-1, -1, -1], [1, 1, 1], 4, 2)
    assert inv.tolist() == [2., 2., 2.] and step.tolist() == [.25, .25, .25] and inv.dtype == F32
    lo, inv, step = OC.grid_fields([-1.6] * 3, [1.6] * 3, 64, 2)  # host fp32: the side is rounded first
    side = F32(1.6) - F32(-1.6)
    assert inv[0] == F32(64) / side and step[0] == side / F32(128)
    g = _grid4([(1, 2, 3)])
    i = (3 * 4 + 2) * 4 + 1
    w = g.words()
    assert w.dtype == np.uint32 and w.size == 2 and w[i >> 5] == np.uint32(1 << (i & 31)) and w[1 - (i >> 5)] == 0
    assert OC.unpack_bits(w, 4)[3, 2, 1] and OC.unpack_bits(w, 4).sum() == 1 and g.occupied_share() == 1 / 64
    for bad in (dict(G=0), dict(G=513), dict(k=0), dict(k=5), dict(dilate=-1)):
        with pytest.raises(ValueError):
            OC.OccupancyGrid([-1] * 3, [1] * 3, **dict(dict(G=4, k=1, dilate=0), **bad))
    with pytest.raises(ValueError):
        OC.OccupancyGrid([-1, 1, -1], [1, 1, 1], G=4)


def test_probe_positions():
    lo, inv, step = OC.grid_fields([-1, 0, 2], [1, 4, 3], 4, 2)
    p = OC.probe_points(lo, step, 4, 2)
    assert p.shape == (512, 3) and p.dtype == F32
    assert p[0].tolist() == [-0.875, 0.25, 2.0625]  # lo + 0.5 step
    assert p[1].tolist() == [-0.625, 0.25, 2.0625]  # x runs fastest
    assert p[8].tolist() == [-0.875, 0.75, 2.0625] and p[64].tolist() == [-0.875, 0.25, 2.1875]
    assert p[511].tolist() == [0.875, 3.75, 2.9375]


def test_live_rule_on_faces_hi_and_nan():
    g = _grid4([(2, 2, 2)])
    live = lambda *pts: OC.live_spec(g.words(), g.lo, g.inv, 4, np.array(pts, dtype=F32)).tolist()
    # a point ON a cell face belongs to the upper cell: (0, 0, 0) is the low corner of cell (2, 2, 2)
    assert live((0, 0, 0), (0.49, 0.49, 0.49), (0.5, 0, 0), (-1e-7, 0, 0)) == [True, True, False, False]
    # exactly at hi: outside, hence live although every cell around is empty; exactly at lo: inside cell 0, empty
    assert live((1, 0, -1), (-1, -1, -1), (0.99, -1, -1)) == [True, False, False]
    # just below lo, far away, NaN and +-inf coordinates: outside, live
    assert live((-1.0001, 0, 0), (0, 50, 0), (np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf)) == [True] * 5
    # -0.0 is inside cell 2 like +0.0
    assert live((-0.0, 0.2, 0.2)) == [True]


def test_compact_and_scatter_spec_by_hand():
    g = _grid4([(2, 2, 2)])
    o = np.array([[-1, .25, .25], [-1, -.75, .25], [3, 3, 3]], dtype=F32)
    d = np.array([[1, 0, 0], [1, 0, 0], [0, 0, 0]], dtype=F32)
    v = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=F32)
    z = np.array([[0.5, 1.0, 1.25, 2.0],      # x = -0.5 (cell 1: empty), 0 (face: cell 2, set), 0.25 (set), 1 (= hi: outside)
                  [1.0, np.nan, 1.5, 3.0],    # cell (2, 0, 2): empty; NaN: live; empty; outside
                  [0.0, 1.0, 2.0, 3.0]], dtype=F32)  # d = 0 at (3, 3, 3): all outside
    M, idx, oo, od, ov, oz = OC.compact_spec(g.words(), g.lo, g.inv, 4, o, d, v, z)
    assert M == 9 and idx.dtype == np.int64 and idx.tolist() == [1, 2, 3, 5, 7, 8, 9, 10, 11]
    assert oo.tolist() == [o[0].tolist()] * 3 + [o[1].tolist()] * 2 + [o[2].tolist()] * 4
    assert ov[3].tolist() == [0, 1, 0] and od[8].tolist() == [0, 0, 0]
    assert U.same_bits(oz, z.reshape(-1)[idx]) and np.isnan(oz[3])
    raw_live = np.arange(36, dtype=F32).reshape(9, 4) + 1
    raw = OC.scatter_spec(raw_live, idx, 3, 4)
    assert raw.shape == (3, 4, 4) and raw.dtype == F32
    assert raw.reshape(12, 4)[idx].tolist() == raw_live.tolist() and (raw.reshape(12, 4)[[0, 4, 6]] == 0).all()
    assert (OC.scatter_spec(np.zeros((0, 4), F32), np.zeros(0, np.int64), 3, 4) == 0).all()  # M = 0: the zero fill alone
    M0 = OC.compact_spec(g.words(), g.lo, g.inv, 4, o[:0], d[:0], v[:0], z[:0])
    assert M0[0] == 0 and M0[1].size == 0


def test_build_spec_threshold_dilation_and_padding():
    G, k = 4, 2
    sig = np.full((G * k,) * 3, -5., dtype=F32)  # [pz, py, px]
    sig[1, 0, 7] = 0.5    # probe (px, py, pz) = (7, 0, 1): cell (3, 0, 0)
    sig[4, 4, 4] = 60.    # cell (2, 2, 2)
    sig[0, 0, 0] = 0.     # not ABOVE the threshold 0
    sig[7, 7, 0] = np.nan  # a NaN is not above anything
    cells = lambda w: sorted(map(tuple, np.argwhere(OC.unpack_bits(w, G))[:, ::-1].tolist()))
    assert cells(OC.build_spec(sig.reshape(-1), G, k, 0, 0.)) == [(2, 2, 2), (3, 0, 0)]
    assert cells(OC.build_spec(sig.reshape(-1), G, k, 0, 50.)) == [(2, 2, 2)]
    # dilation 1 of the corner cell (3, 0, 0) is clipped at three faces: 2 x 2 x 2 cells
    one = np.full((G * k,) * 3, -5., dtype=F32)
    one[1, 0, 7] = 1.
    assert cells(OC.build_spec(one.reshape(-1), G, k, 1, 0.)) == sorted((x, y, z) for x in (2, 3) for y in (0, 1) for z in (0, 1))
    mid = np.full((G * k,) * 3, -5., dtype=F32)
    mid[4, 4, 6] = 1.  # cell (3, 2, 2): clipped at the x face only
    assert cells(OC.build_spec(mid.reshape(-1), G, k, 1, 0.)) == sorted((x, y, z) for x in (2, 3) for y in (1, 2, 3) for z in (1, 2, 3))
    # a box wider than the grid is the whole grid; dilation 2 of (3, 0, 0) reaches x 1..3, y 0..2, z 0..2
    assert len(cells(OC.build_spec(one.reshape(-1), G, k, 2, 0.))) == 27 and len(cells(OC.build_spec(one.reshape(-1), G, k, 9, 0.))) == 64
    # G = 5: 125 bits in 4 words, the 3 padding bits stay zero when every cell is set and dilated
    w = OC.build_spec(np.ones(125, dtype=F32), 5, 1, 2, 0.)
    assert w.dtype == np.uint32 and w.tolist() == [0xFFFFFFFF] * 3 + [(1 << 29) - 1]
    assert OC.pack_bits(np.ones((5, 5, 5), bool)).tolist() == w.tolist()


def _teacher_pair():
    from r2l_amd.nerf_raybased import NeRF
    nets = []
    for sd in O.make_teacher_state_dicts(11, 2, alpha_bias=0.5):
        m = NeRF(D=8, W=256, input_ch=63, output_ch=4, skips=[4], input_ch_views=27, use_viewdirs=True)
        m.load_state_dict(sd)
        nets.append(m.eval())
    return nets


def test_render_rays_cpu_equals_masked_full_raw():
    """render_rays(occupancy=...) on CPU tensors = raw2outputs of the full raw with the entries that are not live zeroed, pass by
    pass, torch.equal (disp: NaN where acc = 0 on both sides).  The grids are built from the nets themselves (CPU build: the
    module's forward on the probes through build_spec) at a threshold that leaves a good part of the box empty."""
    from r2l_amd.render import get_embedder, raw2outputs, render_rays, run_network, sample_pdf_sort
    from tests.teacher_util import scene_rays
    torch.manual_seed(0)
    coarse, fine = _teacher_pair()
    e10, e4 = get_embedder(10)[0], get_embedder(4)[0]
    qfn = lambda pts, vd, fn: run_network(pts, vd, fn, embed_fn=e10, embeddirs_fn=e4)

    rays = scene_rays(181 * 181, 0)[::1501][:21].contiguous()  # 21 rays across the frame
    R, S, NI = rays.shape[0], 12, 9
    grids = []
    for net in (coarse, fine):
        g = OC.OccupancyGrid([-1.6] * 3, [1.6] * 3, G=6, k=1, dilate=0, sigma_thresh=0.).build(net, keep_sigma=True)
        thr = float(g.sigma.median())  # init-distribution nets have no empty space of their own: cut at the median
        g = OC.OccupancyGrid([-1.6] * 3, [1.6] * 3, G=6, k=1, dilate=0, sigma_thresh=thr).build(net)
        assert 0.2 < g.occupied_share() < 0.8
        grids.append(g)
    got = render_rays(rays, coarse, qfn, S, N_importance=NI, network_fine=fine, perturb=0., retraw=True, occupancy=tuple(grids))
    assert 0 < grids[0].live_points < R * S and grids[0].total_points == R * S  # the counters of the two passes
    assert 0 < grids[1].live_points < R * (S + NI) and grids[1].total_points == R * (S + NI)

    # the same by hand: full raw, masked
    o, d, vd = rays[:, 0:3], rays[:, 3:6], rays[:, 8:11]
    t = torch.linspace(0., 1., S)
    z = (rays[:, 6:7] * (1. - t) + rays[:, 7:8] * t).contiguous()

    def masked(net, g, z):
        pts = o[:, None, :] + d[:, None, :] * z[:, :, None]
        live = OC.live_spec(g.words(), g.lo, g.inv, g.G, OC.sample_points(o.numpy(), d.numpy(), z.numpy()).reshape(-1, 3))
        assert U.same_bits(pts, OC.sample_points(o.numpy(), d.numpy(), z.numpy()))
        with torch.no_grad():
            full = run_network(pts, vd, net, embed_fn=e10, embeddirs_fn=e4)
        return torch.where(torch.from_numpy(live).reshape(z.shape)[..., None], full, torch.zeros_like(full)), live

    raw0, live0 = masked(coarse, grids[0], z)
    assert int(live0.sum()) == grids[0].live_points
    rgb0, disp0, acc0, w0, _ = raw2outputs(raw0, z, d)
    zs, z_all, z_std = sample_pdf_sort(z, w0, NI, det=True)
    raw1, live1 = masked(fine, grids[1], z_all)
    assert int(live1.sum()) == grids[1].live_points
    rgb, disp, acc, _, depth = raw2outputs(raw1, z_all, d)
    for name, want in (("rgb0", rgb0), ("acc0", acc0), ("z_std", z_std), ("raw", raw1), ("rgb_map", rgb), ("acc_map", acc),
                       ("depth_map", depth)):
        assert torch.equal(got[name], want), name
    assert U.same_bits(got["disp_map"], disp) and U.same_bits(got["disp0"], disp0)
    # without the switch nothing changed: the unmasked render still is what it was
    plain = render_rays(rays, coarse, qfn, S, N_importance=NI, network_fine=fine, perturb=0.)
    assert not torch.equal(plain["rgb_map"], got["rgb_map"])  # (these grids cut real density away: the threshold is the median)
    with pytest.raises(ValueError, match="raw_noise_std"):
        render_rays(rays, coarse, qfn, S, raw_noise_std=1., occupancy=tuple(grids))


def test_flag_refusals(tmp_path):
    from r2l_amd import options
    base = ["--use_viewdirs", "--r2l_occupancy"]
    a = options.parse_args(base)
    assert a.r2l_occupancy and a.r2l_occ_res == 128 and a.r2l_occ_bound == 0.
    options.validate_occupancy(a)
    assert OC.box_half_side(a, 2., 6.) == 2.5
    a = options.parse_args(base + ["--r2l_occ_res", "64", "--r2l_occ_bound", "1.6"])
    assert a.r2l_occ_res == 64 and OC.box_half_side(a, 2., 6.) == 1.6
    cfg = tmp_path / "c.txt"
    cfg.write_text("use_viewdirs = True\nr2l_occupancy = True\nr2l_occ_res = 32\nr2l_occ_bound = 2\n")  # config keys too
    a = options.parse_args(["--config", str(cfg)])
    assert a.r2l_occupancy and a.r2l_occ_res == 32 and a.r2l_occ_bound == 2.
    options.validate_occupancy(options.parse_args(["--r2l_fused_frames"]))  # without the switch nothing is checked
    teacher_cfg = os.path.join(ROOT, "configs", "lego.txt")
    for extra, needle in ((["--r2l_fused_frames"], "r2l_fused_frames"),
                          (["--r2l_online_kd", "--r2l_teacher_config", teacher_cfg, "--teacher_ckpt", "t.tar"], "r2l_online_kd"),
                          (["--dataset_type", "llff", "--r2l_llff"], "llff"), (["--raw_noise_std", "1"], "raw_noise_std"),
                          (["--r2l_occ_res", "0"], "r2l_occ_res"), (["--r2l_occ_res", "513"], "r2l_occ_res"),
                          (["--r2l_occ_bound", "-1"], "r2l_occ_bound")):
        with pytest.raises(ValueError, match=needle):
            options.validate_occupancy(options.parse_args(base + extra))
    options.validate_occupancy(options.parse_args(base + ["--raw_noise_std", "1"]), raw_noise_std=0.)  # main.py's test render: no noise
    # the drivers raise at start-up, before anything is loaded
    from r2l_amd import create_data, driver
    with pytest.raises(ValueError, match="r2l_fused_frames"):
        create_data.main(base + ["--create_data", "rand", "--r2l_fused_frames"])
    with pytest.raises(ValueError, match="raw_noise_std"):
        create_data.main(base + ["--create_data", "rand", "--raw_noise_std", "1"])
    with pytest.raises(ValueError, match="r2l_store_save"):
        create_data.main(base + ["--create_data", "rand", "--r2l_store_save", str(tmp_path / "s.bin")])
    with pytest.raises(ValueError, match="r2l_fused_frames"):
        driver.main(base + ["--model_name", "nerf", "--render_only", "--r2l_fused_frames"])


def test_abi_argument_checks():
    """Every refusal of include/r2l_hip.h is hipErrorInvalidValue with the argument named, before any launch (dummy pointers)."""
    assert U.check_refusals() >= 50


def test_header_exports_and_struct(tmp_path):
    from r2l_amd import _lib
    names = ["r2l_occ_bits_words", "r2l_occ_grid_init", "r2l_occ_build_work_floats", "r2l_occ_build", "r2l_occ_compact_work_bytes",
             "r2l_occ_compact", "r2l_occ_scatter"]
    header = open(os.path.join(ROOT, "include", "r2l_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert re.search(r"\b%s\(" % n, header) and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert "typedef struct r2l_occ_grid" in header
    S = _lib.OccGridDesc
    assert ctypes.sizeof(S) == 56 and [getattr(S, f).offset for f, _ in S._fields_] == [0, 8, 12, 24, 36, 48]
    assert os.path.exists(os.path.join(ROOT, "r2l_amd", "csrc", "r2l_occupancy.hip"))
    # r2l_occ_grid_init is grid_fields (host fp32), on an awkward box
    d = S()
    lo, hi = (ctypes.c_float * 3)(-1.6, -0.3, 0.1), (ctypes.c_float * 3)(1.6, 2.9, 0.7)
    assert _lib.load().r2l_occ_grid_init(ctypes.byref(d), ctypes.c_void_p(4096), 37, 3, lo, hi) == 0
    f = OC.grid_fields(list(lo), list(hi), 37, 3)
    assert d.G == 37 and d.bits == 4096 and list(d.reserved) == [0, 0]
    assert all(np.array_equal(np.array(getattr(d, n), dtype=F32), f[i]) for i, n in enumerate(("lo", "inv", "step")))
    # the work sizes the header promises
    assert _lib.load().r2l_occ_compact_work_bytes(0) == 16 and _lib.load().r2l_occ_compact_work_bytes(2049) == 16
    assert _lib.load().r2l_occ_compact_work_bytes(2048 * 5 + 1) == 32
    assert _lib.load().r2l_occ_build_work_floats(4, 1) == 14 * 64 + 2 * 4
    if shutil.which("gcc") is None:
        return
    src = tmp_path / "size.c"
    fields = ["bits", "G", "lo", "inv", "step", "reserved"]
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "r2l_hip.h"\nint main(void) {\n    printf("%d", (int)sizeof(r2l_occ_grid));\n'
                   + "".join('    printf(" %%d", (int)offsetof(r2l_occ_grid, %s));\n' % f for f in fields) + "    return 0;\n}\n")
    exe = str(tmp_path / "size")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe],
                   check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["56", "0", "8", "12", "24", "36", "48"]
