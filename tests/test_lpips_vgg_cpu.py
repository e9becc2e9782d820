"""LPIPS (VGG-16, v0.1) without a GPU: metrics.lpips_vgg's CPU branch against the golden numbers of tests/lpips_vgg_util.py, the
weight-file reader, the r2l_lpips_vgg ABI's size queries and argument checks, the option, test_lpips_vgg through
driver.render_path and the log field.  Bars: tests/lpips_vgg_util.py."""
import ctypes
import os

import pytest
import torch

from tests import lpips_vgg_util as U
from tests.test_driver_cpu import ROOT
from tests.test_flip_cpu import _Log, tiny_student

FEATURES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
SLICE = (1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5)


@pytest.fixture(scope="module")
def params():
    return U.flat_params()


def vgg_state_dicts(scheme):
    """make_weights(7) under the naming schemes -> (features / slices dict, lin dict)"""
    w = U.make_weights(7)
    feats, lins = {}, {}
    for l, idx in enumerate(FEATURES):
        stem = "features.%d" % idx if scheme == "torchvision" else "net.slice%d.%d" % (SLICE[l], idx)
        feats[stem + ".weight"], feats[stem + ".bias"] = w["w%d" % l], w["b%d" % l]
    for l in range(5):
        lins["lin%d.model.1.weight" % l] = w["lin%d" % l].view(1, -1, 1, 1)
    return feats, lins


@pytest.mark.parametrize("size", U.SIZES)
def test_fp64_branch_reproduces_the_golden_numbers(params, size):
    from r2l_amd import metrics
    a, b, y = U.yard(size)
    total, layers, maps = metrics.lpips_vgg(a[0].double(), b[0].double(), params.double(), return_layers=True, return_maps=True)
    assert total.dtype == torch.float64 and total.dim() == 0 and layers.shape == (5,)
    got, want = [total.item()] + layers.tolist(), U.GOLDEN[size]
    rel = [abs(g / w - 1) for g, w in zip(got, want)]
    print("%dx%d: fp64 branch against the golden numbers, relative: %s" % (size + (" ".join("%.1e" % r for r in rel),)))
    assert max(rel) <= 1e-9
    assert [tuple(m.shape) for m in maps] == metrics.lpips_vgg_sizes(*size)
    for l in range(5):  # v_l is the mean of its map, the total their sum in the order 0..4
        assert abs(maps[l].mean().item() - layers[l].item()) <= 1e-15
    assert abs(sum(layers.tolist()) - total.item()) <= 1e-15
    # the fp32 plumbing branch inside the bars (they are built from it: what is asserted is the floor's margin), the conditions
    # that keep the bars honest (asserted by the yardstick), and the measured figures of the util's docstring
    t32, l32, m32 = metrics.lpips_vgg(a, b, params, return_layers=True, return_maps=True)
    print("  smallest norm / median %.3f; fp32 branch: layers %.2e relative, maps %.2e of the map's maximum" % (
        y["ratio"], y["rel_layers"], y["rel_maps"]))
    assert t32.dtype == torch.float32
    U.compare("%dx%d fp32 branch" % size, (t32, l32, m32), y)
    assert y["rel_layers"] <= U.REL_FLOOR and y["rel_maps"] <= U.REL_FLOOR  # (the floor, not the fp32 rounding, sets the bars)


def test_stack_rescale_reproduces_the_golden_numbers(params):
    """Three different frames in one call, both stacks rescaled by their own extrema (main.py:361-363)."""
    from r2l_amd import metrics
    A, B, ext = U.stack_case()
    got = metrics.lpips_vgg(A.double(), B.double(), params.double(), rescale=ext.double())
    rel = [abs(g / w - 1) for g, w in zip(got.tolist(), U.GOLDEN_STACK)]
    print("stack: relative %s" % " ".join("%.1e" % r for r in rel))
    assert got.shape == (3,) and max(rel) <= 1e-9
    one = metrics.lpips_vgg(A[1].double(), B[1].double(), params.double(), rescale=ext.double())  # frame by frame: the same number
    assert abs(one.item() - got[1].item()) <= 1e-12
    plain = metrics.lpips_vgg(A.double(), B.double(), params.double())  # the bar sees a missing rescale
    assert ((plain - got).abs() > 1e-3 * got).all()


def test_identical_symmetric_normalize(params):
    from r2l_amd import metrics
    a, b = U.pair2(17, 23, 5)
    for dt in (torch.float32, torch.float64):
        x, y, p = 2 * a.to(dt) - 1, 2 * b.to(dt) - 1, params.to(dt)
        t, layers, maps = metrics.lpips_vgg(x, x.clone(), p, return_layers=True, return_maps=True)
        assert t.item() == 0. and layers.abs().max().item() == 0. and all(m.abs().max().item() == 0. for m in maps)
        ab, ba = metrics.lpips_vgg(x, y, p, return_maps=True), metrics.lpips_vgg(y, x, p, return_maps=True)
        assert torch.equal(ab[0], ba[0]) and all(torch.equal(m, n) for m, n in zip(ab[1], ba[1]))
        assert torch.equal(metrics.lpips_vgg(a.to(dt), b.to(dt), p, normalize=True), ab[0])
    with pytest.raises(ValueError, match="16"):
        metrics.lpips_vgg(torch.zeros(15, 40, 3), torch.zeros(15, 40, 3), params)


def test_output_size_table():
    from r2l_amd import metrics
    assert metrics.lpips_vgg_sizes(400, 400) == [(400, 400), (200, 200), (100, 100), (50, 50), (25, 25)]
    assert metrics.lpips_vgg_sizes(16, 16) == [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]
    assert metrics.lpips_vgg_sizes(17, 23) == [(17, 23), (8, 11), (4, 5), (2, 2), (1, 1)]
    assert metrics.lpips_vgg_sizes(130, 131) == [(130, 131), (65, 65), (32, 32), (16, 16), (8, 8)]
    assert len(metrics.LPIPS_VGG_CONVS) == 13 and metrics.LPIPS_VGG_PARAM_FLOATS == 14716160


def test_flatten_round_trip_and_parameter_count(params):
    from r2l_amd import _lib, metrics
    assert params.dtype == torch.float32 and params.numel() == _lib.load().r2l_lpips_vgg_param_floats() == metrics.LPIPS_VGG_PARAM_FLOATS
    convs, lins = metrics.lpips_vgg_unflatten(params)
    w = U.make_weights(7)
    assert len(convs) == 13 and [tuple(c[0].shape[:2]) for c in convs] == [(co, ci) for ci, co in metrics.LPIPS_VGG_CONVS]
    assert all(torch.equal(convs[l][0], w["w%d" % l]) and torch.equal(convs[l][1], w["b%d" % l]) for l in range(13))
    assert [t.numel() for t in lins] == [64, 128, 256, 512, 512] and all(torch.equal(lins[l], w["lin%d" % l]) for l in range(5))
    assert torch.equal(metrics.lpips_vgg_flatten(convs, lins), params)
    with pytest.raises(AssertionError, match="14716160"):
        metrics.lpips_vgg_unflatten(params[:-1])


@pytest.mark.parametrize("wrong,size", [(dict(shift=False), (35, 47)), (dict(pre_relu=True), (35, 47)), (dict(ceil_mode=True), (17, 23))])
def test_the_bars_see_wrong_evaluations(params, wrong, size):
    """Deliberately wrong fp64 evaluations leave the per-layer bars by at least 10 x in some layer: no shift in the scaling
    layer, the tap taken in front of its ReLU, ceil-mode pools (17x23: 17 -> 9 instead of 8)."""
    from r2l_amd import metrics
    a, b, y = U.yard(size)
    layers, _ = metrics._lpips_vgg_torch(a.double(), b.double(), params.double(), **wrong)
    over = ((layers - y["layers"]).abs() / y["bar_layers"])[0]
    rel = ((layers - y["layers"]).abs() / y["layers"])[0]
    print("%s: per-layer miss in bars: %s; relative %s" % (wrong, " ".join("%.0f" % v for v in over.tolist()),
                                                          " ".join("%.1e" % v for v in rel.tolist())))
    assert over.max().item() >= 10. and rel.max().item() >= 3e-2
    right, _ = metrics._lpips_vgg_torch(a.double(), b.double(), params.double())
    assert torch.equal(right, y["layers"])


def test_ceil_mode_changes_nothing_at_16x16(params):
    """(why the odd size is among SIZES: at 16 -> 8 -> 4 -> 2 -> 1 a ceil-mode pool is the floor pool)"""
    from r2l_amd import metrics
    a, b, y = U.yard((16, 16))
    layers, _ = metrics._lpips_vgg_torch(a.double(), b.double(), params.double(), ceil_mode=True)
    assert torch.equal(layers, y["layers"])


def test_the_bars_see_one_zeroed_weight_of_conv1_2():
    """The figure of the util's docstring: one weight of conv1_2 set to 0 leaves the bars at every size (fp64 evaluation)."""
    from r2l_amd import metrics
    pz = U.flat_params(zero=U.ZERO_CONV1_2).double()
    for size in U.SIZES[:4]:
        a, b, y = U.yard(size)
        layers, maps = metrics._lpips_vgg_torch(a.double(), b.double(), pz)
        rel = ((layers - y["layers"]).abs() / y["layers"])[0]
        print("%dx%d: relative per layer %s" % (size + (" ".join("%.1e" % v for v in rel.tolist()),)))
        assert rel.max().item() >= 3e-5 and U.misses((layers, maps), y) > 1.


def test_lpips_vgg_params_reads_the_three_naming_schemes(tmp_path, params):
    from r2l_amd import metrics
    tv, lins = vgg_state_dicts("torchvision")
    sl, _ = vgg_state_dicts("lpips")
    torch.save(dict(tv, **{"classifier.0.weight": torch.zeros(4, 4), "classifier.0.bias": torch.zeros(4)}), str(tmp_path / "vgg16.pth"))
    torch.save(lins, str(tmp_path / "vgg.pth"))
    torch.save(dict(sl, **lins, **{"scaling_layer.shift": torch.zeros(1, 3, 1, 1)}), str(tmp_path / "lpips_state.pth"))
    torch.save(dict(tv, **lins), str(tmp_path / "both.pth"))
    two = metrics.lpips_vgg_params("%s:%s" % (tmp_path / "vgg16.pth", tmp_path / "vgg.pth"))  # two files, classifier.* ignored
    assert two.dtype == torch.float32 and two.shape == (14716160,) and torch.equal(two, params)
    assert torch.equal(metrics.lpips_vgg_params(str(tmp_path / "lpips_state.pth")), params)
    assert torch.equal(metrics.lpips_vgg_params(str(tmp_path / "both.pth")), params)
    with pytest.raises(ValueError, match=r"lin0\.model\.1\.weight"):
        metrics.lpips_vgg_params(str(tmp_path / "vgg16.pth"))  # the lin layers are in the other file
    with pytest.raises(ValueError, match=r"features\.0\.weight"):
        metrics.lpips_vgg_params(str(tmp_path / "vgg.pth"))
    bad = dict(tv, **lins)
    bad["features.14.weight"] = torch.zeros(256, 256, 3, 2)
    torch.save(bad, str(tmp_path / "bad.pth"))
    with pytest.raises(ValueError, match=r"features\.14\.weight.*\(256, 256, 3, 3\)"):
        metrics.lpips_vgg_params(str(tmp_path / "bad.pth"))
    bad = dict(tv, **lins)
    del bad["features.28.bias"]
    torch.save(bad, str(tmp_path / "short.pth"))
    with pytest.raises(ValueError, match=r"features\.28\.bias"):
        metrics.lpips_vgg_params(str(tmp_path / "short.pth"))
    bad = dict(tv, **lins)
    bad["lin3.model.1.weight"] = torch.zeros(1, 256, 1, 1)  # (AlexNet's lin3)
    torch.save(bad, str(tmp_path / "lin.pth"))
    with pytest.raises(ValueError, match=r"lin3\.model\.1\.weight.*\(1, 512, 1, 1\)"):
        metrics.lpips_vgg_params(str(tmp_path / "lin.pth"))


def test_abi_sizes_and_argument_checks():
    """The size queries, and every refusal of r2l_lpips_vgg / r2l_lpips_vgg_pack: hipErrorInvalidValue with a message that starts
    with the function's name and names the argument, before anything is launched (so this runs without a GPU)."""
    from r2l_amd import _lib, metrics
    lib = _lib.load()
    INVALID = 1
    assert lib.r2l_lpips_vgg_param_floats() == 14716160
    # layer 0's rows are padded to 16 channels: 9 * 13 * 64 more floats than the flat vector
    assert lib.r2l_lpips_vgg_pack_floats() == 14716160 + 9 * 13 * 64
    for hw in U.SIZES + [(400, 400)]:
        assert lib.r2l_lpips_vgg_map_floats(*hw) == sum(h * w for h, w in metrics.lpips_vgg_sizes(*hw))
    work = lib.r2l_lpips_vgg_work_floats
    for k in (1, 3):
        # at least the largest three maps that are alive together (conv1_1, conv1_2 and nothing smaller than the 16-channel image) ..
        assert work(k, 400, 400) >= k * 2 * 160000 * (64 + 64 + 16)
        # .. and not all thirteen (conv1_1 and conv1_2 alone are 0.47 of them)
        all13 = k * 2 * sum(h * w * metrics.LPIPS_VGG_CONVS[l][1] for l, (h, w) in zip(range(13), [
            metrics.lpips_vgg_sizes(400, 400)[s] for s in (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4)]))
        assert work(k, 400, 400) < all13 * 3 // 4
        assert work(k, 16, 16) < work(k, 17, 23) < work(k, 67, 95) < work(k, 400, 400) < work(k + 1, 400, 400)
    assert work(1, 400, 400) * 4 < 256 << 20 and work(1, 800, 800) * 4 < 1 << 30
    for bad in ((0, 400, 400), (-1, 400, 400), (1, 15, 400), (1, 400, 15), (2, 32768, 16384), (65536, 128, 128)):
        assert work(*bad) == -1, bad
    assert work(1, 32768, 16384) > 0  # (2 K H W = 2^30)
    assert lib.r2l_lpips_vgg_map_floats(15, 16) == -1 and lib.r2l_lpips_vgg_map_floats(16, 15) == -1
    one = ctypes.c_void_p(64)  # any non-NULL aligned value: the checks fail before it is ever dereferenced
    ok = [one, one, 1, 16, 16, None, one, one, None, None, one, None]
    for at, value, word in ((2, 0, b"K"), (2, -2, b"K"), (3, 15, b"H"), (4, 15, b"W"), (3, 20000, b"H"), (0, None, b"img_a"),
                            (1, None, b"img_b"), (6, None, b"wpack"), (7, None, b"work"), (10, None, b"out"),
                            (7, ctypes.c_void_p(68), b"aligned"), (6, ctypes.c_void_p(72), b"aligned"), (2, 70000, b"K")):
        args = list(ok)
        args[at] = value
        assert lib.r2l_lpips_vgg(*args) == INVALID, args
        msg = lib.r2l_last_error()
        assert msg.startswith(b"r2l_lpips_vgg:") and word in msg, (args, msg)
    big = list(ok)
    big[2:5] = [16, 16384, 16384]  # 2 K H W = 2^33
    assert lib.r2l_lpips_vgg(*big) == INVALID and b"K" in lib.r2l_last_error()
    for args, word in (((None, one, None), b"params_dev"), ((one, None, None), b"wpack_dev"),
                       ((one, ctypes.c_void_p(68), None), b"aligned")):
        assert lib.r2l_lpips_vgg_pack(*args) == INVALID
        msg = lib.r2l_last_error()
        assert msg.startswith(b"r2l_lpips_vgg_pack") and word in msg, msg


def test_option_and_refusals(tmp_path):
    from r2l_amd.options import FLAGS, parse_args, validate_accelerated, validate_lpips
    base = ["--model_name", "R2L", "--config", os.path.join(ROOT, "configs", "lego_noview.txt")]
    assert FLAGS["r2l_lpips_vgg_weights"] == (str, "") and parse_args(base).r2l_lpips_vgg_weights == ""
    w, a = tmp_path / "w.pth", tmp_path / "alex.pth"
    torch.save({}, str(w))
    torch.save({}, str(a))
    args = parse_args(base + ["--r2l_lpips_vgg_weights", str(w)])
    assert args.r2l_lpips_vgg_weights == str(w) and args.r2l_lpips_weights == ""
    validate_accelerated(args)
    validate_accelerated(parse_args(base + ["--r2l_lpips_vgg_weights", str(w), "--lpips_net", "vgg"]))  # (--lpips_net plays no part)
    validate_accelerated(parse_args(base + ["--r2l_lpips_vgg_weights", "%s:%s" % (w, a), "--r2l_lpips_weights", str(a)]))  # both
    with pytest.raises(NotImplementedError, match="vgg"):  # the AlexNet switch's refusal stays
        validate_accelerated(parse_args(base + ["--r2l_lpips_weights", str(a), "--r2l_lpips_vgg_weights", str(w), "--lpips_net", "vgg"]))
    with pytest.raises(FileNotFoundError, match="r2l_lpips_vgg_weights.*nowhere"):  # at start-up, not at the first evaluation
        validate_lpips(parse_args(base + ["--r2l_lpips_vgg_weights", "%s:%s" % (w, tmp_path / "nowhere.pth")]))
    with pytest.raises(FileNotFoundError, match="nowhere"):
        validate_accelerated(parse_args(base + ["--r2l_lpips_vgg_weights", str(tmp_path / "nowhere.pth")]))
    cfg = tmp_path / "c.txt"
    cfg.write_text("dataset_type=blender\nr2l_lpips_vgg_weights=%s\n" % w)
    assert parse_args(["--config", str(cfg)]).r2l_lpips_vgg_weights == str(w)  # (a config key too)


def test_render_path_reports_test_lpips_vgg_cpu(params):
    """render_path on the CPU, three 17x23 frames: misc['test_lpips_vgg'] is the fp64 yardstick on the returned frames with the
    reference's rescale over the whole stack; without params there is no such key and every other statistic is what it was."""
    from r2l_amd import data, driver, metrics
    net, PointSampler = tiny_student()
    dev = torch.device("cpu")
    ps = PointSampler(17, 23, 20., 16, 2., 6., device=dev)
    poses = torch.stack([data.pose_spherical(-60. + 50. * i, -30., 4.) for i in range(3)])
    gts = torch.stack([U.pair2(17, 23, 3)[1] * s for s in (1., 0.8, 0.6)])
    rgbs, misc = driver.render_path(poses, net, ps, dev, _Log(), gt_imgs=gts, lpips_vgg_params=params)
    assert rgbs.shape == (3, 17, 23, 3) and misc["test_lpips_vgg"].dim() == 0 and "test_lpips" not in misc
    ext = torch.stack([rgbs.min(), rgbs.max(), gts.min(), gts.max()]).double()
    want = metrics.lpips_vgg(rgbs.double(), gts.double(), params.double(), rescale=ext).mean().item()
    plain = metrics.lpips_vgg(rgbs.double(), gts.double(), params.double()).mean().item()
    print("test_lpips_vgg %.8f, yardstick %.8f (without the rescale %.8f)" % (misc["test_lpips_vgg"].item(), want, plain))
    assert abs(misc["test_lpips_vgg"].item() - want) <= U.REL_FLOOR * want and abs(plain - want) > 1e-3 * want
    _, none = driver.render_path(poses, net, ps, dev, _Log(), gt_imgs=gts)
    assert "test_lpips_vgg" not in none and "test_flip" in none
    assert none["test_flip"].item() == misc["test_flip"].item() and none["test_ssim"].item() == misc["test_ssim"].item()
    _, none = driver.render_path(poses, net, ps, dev, _Log(), lpips_vgg_params=params)  # no targets: no metric
    assert "test_lpips_vgg" not in none


def test_lpips_field_combinations():
    from r2l_amd.driver import lpips_field
    a, v = torch.tensor(0.12345), torch.tensor(0.54321)
    assert lpips_field({}) == ""
    assert lpips_field({"test_lpips": a}) == " TestLPIPS 0.1235"
    assert lpips_field({"test_lpips_vgg": v}) == " TestLPIPSvgg 0.5432"
    assert lpips_field({"test_lpips_vgg": v, "test_lpips": a}) == " TestLPIPS 0.1235 TestLPIPSvgg 0.5432"
