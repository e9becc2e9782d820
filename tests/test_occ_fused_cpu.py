"""Empty-space skipping inside the fused teacher-frames call, without a device: the flag table of --r2l_occ_fused, the
declarations (header, ctypes table, library exports), the argument refusals of the new calls on dummy pointers (they return before
any launch) and the work-size formulas include/r2l_hip.h states."""
import ctypes
import os
import re

import pytest

from r2l_amd import _lib
from tests import occ_fused_util as FU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEACHER_CFG = os.path.join(ROOT, "configs", "lego.txt")
NEW = ["r2l_occ_index_work_bytes", "r2l_occ_index", "r2l_occ_live_add", "r2l_teacher_mlp_live_cfg",
       "r2l_teacher_frames_occ_work_floats", "r2l_teacher_frames_occ_cfg"]


def test_flag_table(tmp_path):
    from r2l_amd import options
    cd = ("r2l_fused_frames", "r2l_store_save")  # utils/create_data.py's fused paths
    base = ["--use_viewdirs", "--r2l_occ_fused"]
    a = options.parse_args(base + ["--r2l_fused_frames"])
    assert a.r2l_occ_fused and not a.r2l_occupancy and a.r2l_occ_res == 128 and a.r2l_occ_bound == 0.
    options.validate_occ_fused(a, cd)
    options.validate_occ_fused(options.parse_args(base + ["--r2l_store_save", "s.r2l"]), cd)
    cfg = tmp_path / "c.txt"
    cfg.write_text("use_viewdirs = True\nr2l_occ_fused = True\nr2l_fused_frames = True\nr2l_occ_res = 32\nr2l_occ_bound = 2\n")
    a = options.parse_args(["--config", str(cfg)])  # a config key too; it shares the box of --r2l_occupancy
    assert a.r2l_occ_fused and a.r2l_occ_res == 32 and a.r2l_occ_bound == 2.
    options.validate_occ_fused(a, cd)
    from r2l_amd.occupancy import box_half_side
    assert box_half_side(a, 2., 6.) == 2. and box_half_side(options.parse_args(base), 2., 6.) == 2.5
    options.validate_occ_fused(options.parse_args(["--r2l_occupancy"]), cd)  # without the switch nothing is checked
    fused = ["--r2l_fused_frames"]
    for extra, needle in (([], "r2l_fused_frames or --r2l_store_save"), (fused + ["--r2l_occupancy"], "r2l_occupancy"),
                          (fused + ["--dataset_type", "llff", "--r2l_llff"], "llff"), (fused + ["--raw_noise_std", "1"], "raw_noise_std"),
                          (fused + ["--r2l_occ_res", "0"], "r2l_occ_res"), (fused + ["--r2l_occ_res", "513"], "r2l_occ_res"),
                          (fused + ["--r2l_occ_bound", "-1"], "r2l_occ_bound")):
        with pytest.raises(ValueError, match=needle) as e:
            options.validate_occ_fused(options.parse_args(base + extra), cd)
        assert "--r2l_occ_fused" in str(e.value)
    with pytest.raises(ValueError, match="use_viewdirs"):
        options.validate_occ_fused(options.parse_args(["--r2l_occ_fused", "--r2l_fused_frames"]), cd)
    with pytest.raises(ValueError, match="use_viewdirs"):  # main.py --r2l_online_kd: the teacher's config decides
        options.validate_occ_fused(options.parse_args(base + ["--r2l_online_kd"]), ("r2l_online_kd",), use_viewdirs=False)
    options.validate_occ_fused(options.parse_args(["--r2l_occ_fused", "--r2l_online_kd"]), ("r2l_online_kd",), use_viewdirs=True)
    options.validate_occ_fused(options.parse_args(base + fused + ["--raw_noise_std", "1"]), cd, raw_noise_std=0.)  # the test render
    # --r2l_occupancy keeps its meaning and its refusals
    occ = ["--use_viewdirs", "--r2l_occupancy"]
    for extra, needle in ((["--r2l_fused_frames"], "r2l_fused_frames"),
                          (["--r2l_online_kd", "--r2l_teacher_config", TEACHER_CFG, "--teacher_ckpt", "t.tar"], "r2l_online_kd"),
                          (["--dataset_type", "llff", "--r2l_llff"], "llff"), (["--raw_noise_std", "1"], "raw_noise_std"),
                          (["--r2l_occ_res", "0"], "r2l_occ_res"), (["--r2l_occ_bound", "-1"], "r2l_occ_bound")):
        with pytest.raises(ValueError, match=needle):
            options.validate_occupancy(options.parse_args(occ + extra))
    # the drivers raise at start-up, before anything is loaded
    from r2l_amd import create_data, driver
    with pytest.raises(ValueError, match="r2l_fused_frames or --r2l_store_save"):
        create_data.main(base + ["--create_data", "rand"])
    with pytest.raises(ValueError, match="r2l_occupancy"):
        create_data.main(base + ["--create_data", "rand", "--r2l_fused_frames", "--r2l_occupancy"])
    with pytest.raises(ValueError, match="raw_noise_std"):
        create_data.main(base + ["--create_data", "rand", "--r2l_store_save", str(tmp_path / "s.r2l"), "--raw_noise_std", "1"])
    with pytest.raises(ValueError, match="r2l_store_save"):  # (the per-pose switch still refuses the store fill)
        create_data.main(occ + ["--create_data", "rand", "--r2l_store_save", str(tmp_path / "s.r2l")])
    with pytest.raises(ValueError, match="r2l_fused_frames"):
        driver.main(base + ["--model_name", "nerf", "--render_only"])
    with pytest.raises(ValueError, match="r2l_occupancy"):
        driver.main(base + ["--model_name", "nerf", "--render_only", "--r2l_occupancy", "--r2l_fused_frames"])
    with pytest.raises(ValueError, match="r2l_online_kd"):
        driver.main(["--r2l_occ_fused", "--model_name", "R2L"])
    # the teacher-training entry point shares the option table: it accepts and ignores the switch
    assert options.parse_args(["--config", TEACHER_CFG, "--r2l_occ_fused"]).r2l_occ_fused


def test_header_signatures_and_exports():
    header = open(os.path.join(ROOT, "include", "r2l_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert re.search(r"\b%s\(" % n, header) and n in _lib.SIGNATURES and hasattr(lib, n), n
    # the frames call takes every argument of r2l_teacher_frames_cfg up to rgb0, then the grids, live_acc, work, stream, cfg
    plain, occ = _lib.SIGNATURES["r2l_teacher_frames_cfg"][1], _lib.SIGNATURES["r2l_teacher_frames_occ_cfg"][1]
    assert occ[:16] == plain[:16] and len(occ) == len(plain) + 3 and occ[-3:] == plain[-3:]
    for rule in ("zero-filled first", "product and sum rounded separately", "reads and writes nothing", "No host synchronisation",
                 "template parameter", "before any LDS staging or barrier", "count - 1", "run_if = GO", "has no live variant",
                 "ASCENDING", "No atomics", "grid_coarse serves both passes", "box is in world space", "reserved stays zero"):
        assert rule in header, rule
    # the kernels: the live form is a template parameter of the three forward kernels; the training form has none
    src = {f: open(os.path.join(ROOT, "r2l_amd", "csrc", f)).read() for f in ("r2l_teacher_mlp.hip", "r2l_teacher2.hip", "r2l_teacher3.hip")}
    assert "template <bool STASH, bool LIVE = false>" in src["r2l_teacher_mlp.hip"] and "static_assert(!(STASH && LIVE)" in src["r2l_teacher_mlp.hip"]
    for f in ("r2l_teacher2.hip", "r2l_teacher3.hip"):
        assert "template <bool LIVE>" in src[f]
    for s in src.values():
        assert "t_live_workgroup_idle" in s and "t_live_sample" in s


def test_abi_argument_checks():
    """Every refusal of the new calls is hipErrorInvalidValue with the argument named, before any launch (dummy pointers)."""
    assert FU.check_refusals() >= 35


def test_work_sizes():
    lib = _lib.load()
    for n in (0, 1, 2048, 2049, 300 * 192, 2**31 - 1):
        assert lib.r2l_occ_index_work_bytes(n) == lib.r2l_occ_compact_work_bytes(n) == (max((n + 2047) // 2048, 1) * 4 + 15) // 16 * 16
    r4 = lambda x: (x + 3) // 4 * 4
    for H, W, chunk, Ns, Ni in ((20, 24, 0, 64, 128), (20, 24, 100, 64, 128), (33, 31, 0, 8, 0), (400, 400, 0, 64, 128), (5, 7, 1000, 8, 16)):
        d = FU.frame_desc(H=H, W=W, chunk_rays=chunk, N_samples=Ns, N_importance=Ni)
        plain = lib.r2l_teacher_frames_work_floats(ctypes.byref(d))
        n = (min(chunk, H * W) if chunk else H * W) * (Ns + Ni)  # samples of the larger pass
        want = plain + r4(2 * n) + 4 + r4((lib.r2l_occ_index_work_bytes(n) + 3) // 4)
        assert plain > 0 and lib.r2l_teacher_frames_occ_work_floats(ctypes.byref(d)) == want, (H, W, chunk, Ns, Ni)
        assert want % 4 == 0
