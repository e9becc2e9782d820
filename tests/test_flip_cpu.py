"""FLIP (utils/flip_loss.py) without a GPU: metrics.flip's CPU branch against the reference-made tests/golden/flip.npz
(gen_golden_flip.py), the r2l_flip ABI's argument checks, and test_flip through driver.render_path on one and two ranks.

Bars (from the reference's own rounding, read case by case from the golden file): a pixel within
max(4 * max|flip32 - flip64|, 2e-5) of the reference's fp64 map, a per-frame mean within 1e-5 of its fp64 mean; fp64 input
within 1e-9."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_driver_cpu import ROOT, make_scene

GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "flip.npz"))
CASES = [str(c) for c in GOLDEN["cases"]]
MEAN_BAR = 1e-5


def case(name):
    """-> pred, gt [H,W,3] fp32, ppd, the reference's fp64 map, its fp64 mean, the per-pixel bar of this case"""
    key = str(GOLDEN["img_" + name])
    f32, f64 = torch.tensor(GOLDEN["flip32_" + name]), torch.tensor(GOLDEN["flip64_" + name])
    bar = max(4 * (f32.double() - f64).abs().max().item(), 2e-5)
    return (torch.tensor(GOLDEN["pred_" + key]), torch.tensor(GOLDEN["gt_" + key]), float(GOLDEN["ppd_" + name]), f64,
            float(GOLDEN["mean64_" + name]), bar)


def multi():
    """-> rec, ref [3,H,W,3] fp32, their extrema, the fp64 map of main.py:359-379 on them, its mean, the per-pixel bar"""
    rec, ref = torch.tensor(GOLDEN["multi_rec"]), torch.tensor(GOLDEN["multi_ref"])
    f32, f64 = torch.tensor(GOLDEN["multi_flip32"]), torch.tensor(GOLDEN["multi_flip64"])
    bar = max(4 * (f32.double() - f64).abs().max().item(), 2e-5)
    return rec, ref, torch.stack([rec.min(), rec.max(), ref.min(), ref.max()]), f64, float(GOLDEN["multi_mean64"]), bar


def test_golden_file_covers_the_cases():
    assert CASES == ["1x1", "7x9", "33x16", "40x52", "70x90", "33x16_ppd30", "70x90_ppd30", "scene", "scene_ppd30"]
    for name in CASES:
        pred, gt, ppd, f64, mean64, bar = case(name)
        assert tuple(pred.shape) == tuple(gt.shape) == tuple(f64.shape) + (3,) and f64.dtype == torch.float64
        assert ppd == 30.0 if name.endswith("ppd30") else abs(ppd - 67.0206) < 1e-3
        assert abs(f64.mean().item() - mean64) < 1e-12
    assert GOLDEN["multi_rec"].shape == GOLDEN["multi_ref"].shape == (3, 28, 36, 3)


@pytest.mark.parametrize("name", CASES)
def test_cpu_branch_vs_reference(name):
    from r2l_amd import metrics
    pred, gt, ppd, f64, mean64, bar = case(name)
    m, f = metrics.flip(pred.double(), gt.double(), ppd, return_map=True)
    assert f.dtype == torch.float64 and f.shape == f64.shape and m.dim() == 0
    err64 = (f - f64).abs().max().item()
    m32, f32 = metrics.flip(pred, gt, ppd, return_map=True)
    assert f32.dtype == torch.float32
    err32, merr = (f32.double() - f64).abs().max().item(), abs(m32.item() - mean64)
    print("%s: fp64 branch %.2e; fp32 branch per pixel %.2e (bar %.2e), mean %.2e" % (name, err64, err32, bar, merr))
    assert err64 < 1e-9 and abs(m.item() - mean64) < 1e-9
    assert err32 <= bar and merr <= MEAN_BAR
    assert metrics.flip(pred, gt, ppd).item() == m32.item()  # (without the map: the same number)


def test_multi_frame_stack_rescale_vs_reference():
    """Three different frames in one call with the reference's stack rescale: the number main.py prints as TestFLIP."""
    from r2l_amd import metrics
    rec, ref, ext, f64, mean64, bar = multi()
    m, f = metrics.flip(rec.double(), ref.double(), rescale=ext.double(), return_map=True)
    assert m.shape == (3,) and (f - f64).abs().max().item() < 1e-9 and abs(m.mean().item() - mean64) < 1e-9
    m32, f32 = metrics.flip(rec, ref, rescale=ext, return_map=True)
    assert (f32.double() - f64).abs().max().item() <= bar and abs(m32.double().mean().item() - mean64) <= MEAN_BAR
    for k in range(3):  # frame by frame: the same per-frame means
        assert abs(metrics.flip(rec[k].double(), ref[k].double(), rescale=ext.double()).item() - f64[k].mean().item()) < 1e-9
    # the bar sees a missing rescale
    plain = metrics.flip(rec.double(), ref.double()).mean().item()
    assert abs(plain - float(GOLDEN["multi_mean64_plain"])) < 1e-9 and abs(plain - mean64) > 1e-3


def test_the_bar_sees_zero_padding():
    """Zero instead of replicate padding misses the reference by more than 100 bars at the border of the 40x52 case."""
    from r2l_amd import metrics
    pred, gt, ppd, f64, _, bar = case("40x52")
    wrong = metrics._flip_torch(pred.double()[None], gt.double()[None], ppd, padding="zeros")[0]
    d = (wrong - f64).abs()
    border = torch.cat([d[0], d[-1], d[:, 0], d[:, -1]])
    print("zero padding: border max %.3e = %.0f bars; interior (beyond both radii) max %.3e" %
          (border.max().item(), border.max().item() / bar, d[10:-10, 10:-10].max().item()))
    assert border.max().item() > 100 * bar
    assert d[10:-10, 10:-10].max().item() < 1e-9  # (and only there: the windows reach 10 pixels)


def test_symmetric_in_its_images():
    from r2l_amd import metrics
    for name in ("40x52", "scene_ppd30"):
        pred, gt, ppd, *_ = case(name)
        for dt in (torch.float32, torch.float64):
            a, b = metrics.flip(pred.to(dt), gt.to(dt), ppd, return_map=True), metrics.flip(gt.to(dt), pred.to(dt), ppd, return_map=True)
            assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0])


def test_abi_argument_checks():
    """r2l_flip_partial_count grows with H, W and K; NULL images, K = 0 and a pixels-per-degree whose radii exceed the compiled
    ones are hipErrorInvalidValue with a message, before anything is launched (so this runs without a GPU)."""
    from r2l_amd import _lib
    lib = _lib.load()
    INVALID = 1
    one = ctypes.c_void_p(64)  # any non-NULL value: the checks fail before it is ever dereferenced
    n = lib.r2l_flip_partial_count
    assert n(1, 1, 1) >= 1
    sizes = [1, 7, 16, 33, 70, 400, 401, 800]
    for k in (1, 3, 9):
        for h0, h1 in zip(sizes, sizes[1:]):
            assert n(h0, 400, k) <= n(h1, 400, k) and n(400, h0, k) <= n(400, h1, k) and n(h0, h0, k) <= n(h1, h1, k)
        assert n(1, 1, k) < n(70, 90, k) < n(400, 400, k) < n(800, 800, k)
        assert n(400, 400, k) < n(400, 400, k + 1) and n(400, 400, k) == k * n(400, 400, 1)
    ppd = 67.02
    for args, word in (((None, one, 1, 8, 8, ppd, None, one, None, one, None), b"NULL"),
                       ((one, None, 1, 8, 8, ppd, None, one, None, one, None), b"NULL"),
                       ((one, one, 1, 8, 8, ppd, None, None, None, one, None), b"NULL"),
                       ((one, one, 1, 8, 8, ppd, None, one, None, None, None), b"NULL"),
                       ((one, one, 0, 8, 8, ppd, None, one, None, one, None), b"positive"),
                       ((one, one, 1, 0, 8, ppd, None, one, None, one, None), b"positive"),
                       ((one, one, 1, 8, -3, ppd, None, one, None, one, None), b"positive"),
                       ((one, one, 1, 8, 8, 80.0, None, one, None, one, None), b"pixels_per_degree"),
                       ((one, one, 1, 8, 8, 0.0, None, one, None, one, None), b"pixels_per_degree"),
                       ((one, one, 1, 8, 8, float("nan"), None, one, None, one, None), b"pixels_per_degree")):
        assert lib.r2l_flip(*args) == INVALID, args
        msg = lib.r2l_last_error()
        assert b"r2l_flip" in msg and word in msg, (args, msg)


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, *a):
        self.lines.append(" ".join(str(x) for x in a))


def tiny_student():
    import argparse
    from model.nerf_raybased import NeRF_v3_2, PointSampler
    trial = argparse.Namespace(ON=True, body_arch="resmlp", inact="relu", outact="none", res_scale=1., n_learnable=2, n_block=-1,
                               near=-1, far=-1)
    args = argparse.Namespace(netdepth=6, netwidth=256, layerwise_netwidths="", act="relu", linear_tail=False, use_residual=True,
                              trial=trial)
    torch.manual_seed(0)
    return NeRF_v3_2(args, 1008, 3), PointSampler


def test_render_path_reports_test_flip_cpu():
    """render_path on the CPU, three 9x12 frames: misc['test_flip'] is the fp64 yardstick on the returned frames with the
    reference's rescale over the whole stack (main.py:359-379, 393)."""
    from r2l_amd import data, driver, metrics
    net, PointSampler = tiny_student()
    dev = torch.device("cpu")
    ps = PointSampler(9, 12, 14., 16, 2., 6., device=dev)
    poses = torch.stack([data.pose_spherical(-60. + 50. * i, -30., 4.) for i in range(3)])
    gts = torch.rand(3, 9, 12, 3, generator=torch.Generator().manual_seed(3)) * 0.9 + 0.05
    rgbs, misc = driver.render_path(poses, net, ps, dev, _Log(), gt_imgs=gts)
    assert rgbs.shape == (3, 9, 12, 3) and misc["test_flip"].dim() == 0 and misc["test_ssim"].dim() == 0
    ext = torch.stack([rgbs.min(), rgbs.max(), gts.min(), gts.max()]).double()
    want = metrics.flip(rgbs.double(), gts.double(), rescale=ext).mean().item()
    plain = metrics.flip(rgbs.double(), gts.double()).mean().item()
    print("test_flip %.6f, yardstick %.6f (without the rescale %.6f)" % (misc["test_flip"].item(), want, plain))
    assert abs(misc["test_flip"].item() - want) < 1e-6 and abs(plain - want) > 1e-3
    _, none = driver.render_path(poses, net, ps, dev, _Log())  # no targets: no metric
    assert "test_flip" not in none


def test_cli_two_ranks_log_the_same_test_flip(tmp_path):
    """`main.py --render_only --render_test` as one process and under torchrun with two gloo ranks on the CPU: the extrema of the
    rescale and the sum of the per-frame means are all-reduced, so both log the same TestFLIP, directly behind the unchanged
    `... TestSSIM %.4f` prefix."""
    import unittest.mock as mock
    from r2l_amd import driver
    from r2l_amd.checkpoint import save_ckpt
    from r2l_amd.options import parse_args
    from model.nerf_raybased import NeRF_v3_2
    scene = str(tmp_path / "scene")
    os.makedirs(scene)
    make_scene(scene)
    args = ["--model_name", "R2L", "--config", os.path.join(ROOT, "configs", "lego_noview.txt"), "--datadir", scene,
            "--n_sample_per_ray", "16", "--netwidth", "256", "--netdepth", "6", "--use_residual", "--trial.ON", "--trial.body_arch",
            "resmlp", "--testskip", "1"]
    torch.manual_seed(0)
    save_ckpt(str(tmp_path / "student.tar"), 1, NeRF_v3_2(parse_args(args), 1008, 3), {"state": {}, "param_groups": []}, 0., 0)
    args += ["--pretrained_ckpt", str(tmp_path / "student.tar"), "--render_only", "--render_test"]
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        with mock.patch.object(torch.cuda, "is_available", lambda: False):
            one = driver.main(args + ["--experiment_name", "one_flip"])
    finally:
        os.chdir(cwd)
    env = {k: v for k, v in os.environ.items() if not k.startswith("R2L_")}
    env.update(MASTER_ADDR="127.0.0.1", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", "29633", os.path.join(ROOT, "main.py")] + args +
                       ["--experiment_name", "two_flip"], env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    misc = one["misc"]
    prefix = "[TEST] TestPSNR %.4f TestPSNRv2 %.4f TestSSIM %.4f" % (misc["test_psnr"].item(), misc["test_psnr_v2"].item(),
                                                                    misc["test_ssim"].item())
    want = prefix + " TestFLIP %.4f" % misc["test_flip"].item()
    assert 0. < misc["test_flip"].item() < 1.
    assert want in out, (want, [l for l in out.splitlines() if "[TEST]" in l])
