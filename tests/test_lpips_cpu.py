"""LPIPS (AlexNet, v0.1) without a GPU: metrics.lpips's CPU branch against the golden numbers of tests/lpips_util.py, the
weight-file reader, the r2l_lpips ABI's size queries and argument checks, the option, and test_lpips through driver.render_path
on one and two ranks.  Bars: tests/lpips_util.py."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from tests import lpips_util as U
from tests.test_driver_cpu import ROOT, make_scene
from tests.test_flip_cpu import _Log, tiny_student


@pytest.fixture(scope="module")
def params():
    return U.flat_params()


def state_dicts(scheme):
    """make_weights(7) under the two naming schemes -> (features / slices dict, lin dict)"""
    w = U.make_weights(7)
    feats, lins = {}, {}
    for l, idx in enumerate((0, 3, 6, 8, 10)):
        stem = "features.%d" % idx if scheme == "torchvision" else "net.slice%d.%d" % (l + 1, idx)
        feats[stem + ".weight"], feats[stem + ".bias"] = w["w%d" % l], w["b%d" % l]
        lins["lin%d.model.1.weight" % l] = w["lin%d" % l].view(1, -1, 1, 1)
    return feats, lins


@pytest.mark.parametrize("size", sorted(U.GOLDEN))
def test_fp64_branch_reproduces_the_golden_numbers(params, size):
    from r2l_amd import metrics
    a, b = U.pair2(size[0], size[1], 5)
    total, layers, maps = metrics.lpips((2 * a - 1).double(), (2 * b - 1).double(), params.double(), return_layers=True,
                                        return_maps=True)
    assert total.dtype == torch.float64 and total.dim() == 0 and layers.shape == (5,)
    got, want = [total.item()] + layers.tolist(), U.GOLDEN[size]
    rel = [abs(g / w - 1) for g, w in zip(got, want)]
    print("%dx%d: fp64 branch against the golden numbers, relative: %s" % (size + (" ".join("%.1e" % r for r in rel),)))
    assert max(rel) <= 1e-8
    assert [tuple(m.shape) for m in maps] == metrics.lpips_sizes(*size)
    for l in range(5):  # v_l is the mean of its map, the total their sum in the order 0..4
        assert abs(maps[l].mean().item() - layers[l].item()) <= 1e-15
    assert abs(sum(layers.tolist()) - total.item()) <= 1e-15
    # the conditions that keep the bars honest, and the fp32 plumbing branch within its own floor
    y = U.yardstick((2 * a - 1)[None], (2 * b - 1)[None], params)
    t32 = metrics.lpips(2 * a - 1, 2 * b - 1, params)
    print("  smallest norm / median %.3f; fp32 branch relative %.1e" % (y["ratio"], abs(t32.item() / total.item() - 1)))
    assert t32.dtype == torch.float32 and abs(t32.item() - total.item()) <= U.REL_FLOOR * total.item()


def test_stack_rescale_reproduces_the_golden_numbers(params):
    """Three different frames in one call, both stacks rescaled by their own extrema (main.py:361-363)."""
    from r2l_amd import metrics
    A, B, ext = U.stack_case()
    assert abs(ext[0].item() - U.GOLDEN_STACK_MIN[0]) < 1e-9 and abs(ext[2].item() - U.GOLDEN_STACK_MIN[1]) < 1e-9
    assert ext[1].item() == 1. and ext[3].item() == 1.
    got = metrics.lpips(A.double(), B.double(), params.double(), rescale=ext.double())
    rel = [abs(g / w - 1) for g, w in zip(got.tolist(), U.GOLDEN_STACK)]
    print("stack: relative %s" % " ".join("%.1e" % r for r in rel))
    assert got.shape == (3,) and max(rel) <= 1e-8
    for k in range(3):  # frame by frame: the same numbers
        one = metrics.lpips(A[k].double(), B[k].double(), params.double(), rescale=ext.double())
        assert abs(one.item() - got[k].item()) <= 1e-12
    plain = metrics.lpips(A.double(), B.double(), params.double())  # the bar sees a missing rescale
    assert ((plain - got).abs() > 1e-3 * got).all()


def test_identical_symmetric_normalize(params):
    from r2l_amd import metrics
    a, b = U.pair2(35, 47, 5)
    for dt in (torch.float32, torch.float64):
        x, y, p = 2 * a.to(dt) - 1, 2 * b.to(dt) - 1, params.to(dt)
        t, layers, maps = metrics.lpips(x, x.clone(), p, return_layers=True, return_maps=True)
        assert t.item() == 0. and layers.abs().max().item() == 0. and all(m.abs().max().item() == 0. for m in maps)
        ab, ba = metrics.lpips(x, y, p, return_maps=True), metrics.lpips(y, x, p, return_maps=True)
        assert torch.equal(ab[0], ba[0]) and all(torch.equal(m, n) for m, n in zip(ab[1], ba[1]))
        assert torch.equal(metrics.lpips(a.to(dt), b.to(dt), p, normalize=True), ab[0])
    with pytest.raises(ValueError, match="31"):
        metrics.lpips(torch.zeros(30, 40, 3), torch.zeros(30, 40, 3), params)


def test_output_size_table():
    from r2l_amd import metrics
    assert metrics.lpips_sizes(400, 400) == [(99, 99), (49, 49), (24, 24), (24, 24), (24, 24)]
    assert metrics.lpips_sizes(31, 31) == [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)]
    assert metrics.lpips_sizes(35, 47) == [(8, 11), (3, 5), (1, 2), (1, 2), (1, 2)]
    assert metrics.LPIPS_PARAM_FLOATS == 2470848


def test_the_bars_see_wrong_evaluations(params):
    """Three deliberately wrong fp64 evaluations miss the per-layer bar at 67x95: no shift in the scaling layer, zero padding in
    front of the scaling layer, ceil-mode pools."""
    from r2l_amd import metrics
    a, b = U.pair2(67, 95, 5)
    x, y = (2 * a - 1)[None], (2 * b - 1)[None]
    ref = U.yardstick(x, y, params)
    for wrong in (dict(shift=False), dict(pad_first=True), dict(ceil_mode=True)):
        layers, _ = metrics._lpips_torch(x.double(), y.double(), params.double(), **wrong)
        over = ((layers - ref["layers"]).abs() / ref["bar_layers"])[0]
        print("%s: per-layer miss in bars: %s" % (wrong, " ".join("%.0f" % v for v in over.tolist())))
        assert over.max().item() > 4.
    right, _ = metrics._lpips_torch(x.double(), y.double(), params.double())
    assert torch.equal(right, ref["layers"])


def test_lpips_params_reads_both_naming_schemes(tmp_path, params):
    from r2l_amd import metrics
    tv, lins = state_dicts("torchvision")
    sl, _ = state_dicts("lpips")
    torch.save(tv, str(tmp_path / "alexnet.pth"))
    torch.save(lins, str(tmp_path / "alex.pth"))
    torch.save(dict(sl, **lins, **{"scaling_layer.shift": torch.zeros(1, 3, 1, 1), "classifier.1.weight": torch.zeros(4, 4)}),
               str(tmp_path / "lpips_state.pth"))
    torch.save(dict(tv, **lins), str(tmp_path / "both.pth"))
    two = metrics.lpips_params("%s:%s" % (tmp_path / "alexnet.pth", tmp_path / "alex.pth"))
    assert two.dtype == torch.float32 and two.shape == (2470848,) and torch.equal(two, params)
    assert torch.equal(metrics.lpips_params(str(tmp_path / "lpips_state.pth")), params)
    assert torch.equal(metrics.lpips_params(str(tmp_path / "both.pth")), params)
    with pytest.raises(ValueError, match=r"lin0\.model\.1\.weight"):
        metrics.lpips_params(str(tmp_path / "alexnet.pth"))  # the lin layers are in the other file
    with pytest.raises(ValueError, match=r"features\.0\.weight"):
        metrics.lpips_params(str(tmp_path / "alex.pth"))
    bad = dict(tv, **lins)
    bad["features.6.weight"] = torch.zeros(384, 192, 3, 2)
    torch.save(bad, str(tmp_path / "bad.pth"))
    with pytest.raises(ValueError, match=r"features\.6\.weight.*\(384, 192, 3, 3\)"):
        metrics.lpips_params(str(tmp_path / "bad.pth"))
    bad = dict(tv, **lins)
    del bad["features.10.bias"]
    torch.save(bad, str(tmp_path / "short.pth"))
    with pytest.raises(ValueError, match=r"features\.10\.bias"):
        metrics.lpips_params(str(tmp_path / "short.pth"))
    bad = dict(tv, **lins)
    bad["lin3.model.1.weight"] = torch.zeros(256)
    torch.save(bad, str(tmp_path / "lin.pth"))
    with pytest.raises(ValueError, match=r"lin3\.model\.1\.weight"):
        metrics.lpips_params(str(tmp_path / "lin.pth"))


def test_abi_sizes_and_argument_checks():
    """The size queries, and every refusal of r2l_lpips / r2l_lpips_pack: hipErrorInvalidValue with a message that starts
    r2l_lpips and names the argument, before anything is launched (so this runs without a GPU)."""
    from r2l_amd import _lib, metrics
    lib = _lib.load()
    INVALID = 1
    assert lib.r2l_lpips_param_floats() == 2470848 == metrics.LPIPS_PARAM_FLOATS
    assert lib.r2l_lpips_pack_floats() >= 2470848
    for hw in ((31, 31), (35, 47), (67, 95), (400, 400)):
        assert lib.r2l_lpips_map_floats(*hw) == sum(h * w for h, w in metrics.lpips_sizes(*hw))
    work = lib.r2l_lpips_work_floats
    feats = lambda h, w: 2 * sum(ho * wo * c[1] for (ho, wo), c in zip(metrics.lpips_sizes(h, w), metrics.LPIPS_CONVS))
    for k in (1, 3, 9):
        assert work(k, 400, 400) >= k * feats(400, 400) and work(k, 31, 31) >= k * feats(31, 31)
        assert work(k, 31, 31) < work(k, 67, 95) < work(k, 400, 400) < work(k + 1, 400, 400)
    assert work(9, 400, 400) * 4 < 512 << 20
    for bad in ((0, 400, 400), (-1, 400, 400), (1, 30, 400), (1, 400, 30)):
        assert work(*bad) == -1
    assert lib.r2l_lpips_map_floats(30, 31) == -1 and lib.r2l_lpips_map_floats(31, 30) == -1
    one = ctypes.c_void_p(64)  # any non-NULL aligned value: the checks fail before it is ever dereferenced
    ok = [one, one, 1, 31, 31, None, one, one, None, None, one, None]
    for at, value, word in ((2, 0, b"K"), (2, -2, b"K"), (3, 30, b"H"), (4, 30, b"W"), (0, None, b"img_a"), (1, None, b"img_b"),
                            (6, None, b"wpack"), (7, None, b"work"), (10, None, b"out"), (7, ctypes.c_void_p(68), b"aligned"),
                            (2, 70000, b"K")):
        args = list(ok)
        args[at] = value
        assert lib.r2l_lpips(*args) == INVALID, args
        msg = lib.r2l_last_error()
        assert msg.startswith(b"r2l_lpips") and word in msg, (args, msg)
    for args, word in (((None, one, None), b"params_dev"), ((one, None, None), b"wpack_dev")):
        assert lib.r2l_lpips_pack(*args) == INVALID
        msg = lib.r2l_last_error()
        assert msg.startswith(b"r2l_lpips_pack") and word in msg, msg


def test_option_and_refusals(tmp_path):
    from r2l_amd.options import parse_args, validate_accelerated
    base = ["--model_name", "R2L", "--config", os.path.join(ROOT, "configs", "lego_noview.txt")]
    assert parse_args(base).r2l_lpips_weights == ""
    validate_accelerated(parse_args(base + ["--lpips_net", "vgg"]))  # (without the flag --lpips_net stays an ignored option)
    w = tmp_path / "w.pth"
    torch.save({}, str(w))
    args = parse_args(base + ["--r2l_lpips_weights", str(w)])
    assert args.r2l_lpips_weights == str(w)
    validate_accelerated(args)
    with pytest.raises(NotImplementedError, match="vgg"):
        validate_accelerated(parse_args(base + ["--r2l_lpips_weights", str(w), "--lpips_net", "vgg"]))
    with pytest.raises(FileNotFoundError, match="nowhere"):  # at start-up, not at the first evaluation
        validate_accelerated(parse_args(base + ["--r2l_lpips_weights", "%s:%s" % (w, tmp_path / "nowhere.pth")]))
    cfg = tmp_path / "c.txt"
    cfg.write_text("dataset_type=blender\nr2l_lpips_weights=%s\n" % w)
    assert parse_args(["--config", str(cfg)]).r2l_lpips_weights == str(w)  # (a config key too)


def test_render_path_reports_test_lpips_cpu(params):
    """render_path on the CPU, three 31x40 frames: misc['test_lpips'] is the fp64 yardstick on the returned frames with the
    reference's rescale over the whole stack (main.py:359-369, 392); without params there is no such key and no sixth statistic."""
    from r2l_amd import data, driver, metrics
    net, PointSampler = tiny_student()
    dev = torch.device("cpu")
    ps = PointSampler(31, 40, 40., 16, 2., 6., device=dev)
    poses = torch.stack([data.pose_spherical(-60. + 50. * i, -30., 4.) for i in range(3)])
    gts = torch.stack([U.pair2(31, 40, 3)[1] * s for s in (1., 0.8, 0.6)])
    rgbs, misc = driver.render_path(poses, net, ps, dev, _Log(), gt_imgs=gts, lpips_params=params)
    assert rgbs.shape == (3, 31, 40, 3) and misc["test_lpips"].dim() == 0
    ext = torch.stack([rgbs.min(), rgbs.max(), gts.min(), gts.max()]).double()
    want = metrics.lpips(rgbs.double(), gts.double(), params.double(), rescale=ext).mean().item()
    plain = metrics.lpips(rgbs.double(), gts.double(), params.double()).mean().item()
    print("test_lpips %.8f, yardstick %.8f (without the rescale %.8f)" % (misc["test_lpips"].item(), want, plain))
    assert abs(misc["test_lpips"].item() - want) <= U.REL_FLOOR * want and abs(plain - want) > 1e-3 * want
    _, none = driver.render_path(poses, net, ps, dev, _Log(), gt_imgs=gts)
    assert "test_lpips" not in none and "test_flip" in none
    assert none["test_flip"].item() == misc["test_flip"].item() and none["test_ssim"].item() == misc["test_ssim"].item()
    _, none = driver.render_path(poses, net, ps, dev, _Log(), lpips_params=params)  # no targets: no metric
    assert "test_lpips" not in none


def test_cli_two_ranks_log_the_same_test_lpips(tmp_path):
    """`main.py --render_only --render_test --r2l_lpips_weights` as one process and under torchrun with two gloo ranks on the
    CPU: both log the same TestLPIPS, between TestSSIM and TestFLIP, and it is the fp64 yardstick on the returned frames;
    without the flag the line is what it always was."""
    import unittest.mock as mock
    from r2l_amd import data as D
    from r2l_amd import driver, metrics
    from r2l_amd.checkpoint import save_ckpt
    from r2l_amd.options import parse_args
    from model.nerf_raybased import NeRF_v3_2
    scene = str(tmp_path / "scene")
    os.makedirs(scene)
    make_scene(scene, size=64)  # (half_res: 32x32 frames)
    tv, lins = state_dicts("torchvision")
    torch.save(tv, str(tmp_path / "alexnet.pth"))
    torch.save(lins, str(tmp_path / "alex.pth"))
    weights = "%s:%s" % (tmp_path / "alexnet.pth", tmp_path / "alex.pth")
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
            one = driver.main(args + ["--experiment_name", "one_lpips", "--r2l_lpips_weights", weights])
            off = driver.main(args + ["--experiment_name", "off_lpips"])
            loaded = D.load_scene(parse_args(args))
    finally:
        os.chdir(cwd)
    misc = one["misc"]
    gts = torch.as_tensor(loaded.rgb_images(True)[loaded.i_test]).float()
    rgbs = one["rgbs"]
    assert rgbs.shape == gts.shape == (2, 32, 32, 3)
    ext = torch.stack([rgbs.min(), rgbs.max(), gts.min(), gts.max()]).double()
    want = metrics.lpips(rgbs.double(), gts.double(), U.flat_params().double(), rescale=ext).mean().item()
    print("TestLPIPS %.8f, yardstick %.8f" % (misc["test_lpips"].item(), want))
    assert abs(misc["test_lpips"].item() - want) <= U.REL_FLOOR * want
    assert "test_lpips" not in off["misc"] and off["misc"]["test_flip"].item() == misc["test_flip"].item()
    prefix = "[TEST] TestPSNR %.4f TestPSNRv2 %.4f TestSSIM %.4f" % (misc["test_psnr"].item(), misc["test_psnr_v2"].item(),
                                                                    misc["test_ssim"].item())
    tail = " TestFLIP %.4f" % misc["test_flip"].item()
    want_line = prefix + " TestLPIPS %.4f" % misc["test_lpips"].item() + tail
    logs = {k: open(os.path.join(str(tmp_path), v["logger"].log_path, "log.txt")).read() for k, v in (("one", one), ("off", off))}
    assert want_line in logs["one"] and prefix + tail in logs["off"] and "LPIPS" not in logs["off"]
    env = {k: v for k, v in os.environ.items() if not k.startswith("R2L_")}
    env.update(MASTER_ADDR="127.0.0.1", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", "29647", os.path.join(ROOT, "main.py")] + args +
                       ["--experiment_name", "two_lpips", "--r2l_lpips_weights", weights], env=env, cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert want_line in out, (want_line, [l for l in out.splitlines() if "[TEST]" in l])
