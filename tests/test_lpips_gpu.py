"""The fused LPIPS kernels (csrc/r2l_lpips.hip) on the GPU: against the CPU fp64 yardstick of metrics.lpips at the sizes of
tests/lpips_util.py (total, the five layer values, every map position), their launch invariants (bit-reproducible, K pairs = K
launches, maps and per_layer optional, nothing written outside the buffers) and test_lpips through driver.render_path and the
command line.  Bars: tests/lpips_util.py."""
import ctypes
import os

import pytest
import torch

from tests import lpips_util as U
from tests.test_flip_cpu import _Log

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def params():
    return U.flat_params()


@pytest.fixture(scope="module")
def yard(params):
    """{(H, W): (a, b [1,H,W,3] in [-1, 1], the CPU fp64 yardstick with its bars)}, computed once"""
    out = {}
    for H, W in U.SIZES:
        a, b = U.pair2(H, W, 5)
        a, b = (2 * a - 1)[None], (2 * b - 1)[None]
        out[(H, W)] = (a, b, U.yardstick(a, b, params))
    return out


def compare(tag, got, y):
    """got = (total [K], layers [K,5], maps) of the kernel against the yardstick y: prints the observed errors, then asserts"""
    total, layers, maps = got
    et, el = (total.cpu().double() - y["total"]).abs(), (layers.cpu().double() - y["layers"]).abs()
    em = [(m.cpu().double() - q).abs().max().item() for m, q in zip(maps, y["maps"])]
    print("%s: total %.2e (bar %.2e); layers %s (bars %s); maps %s (bars %s)" % (
        tag, et.max().item(), y["bar_total"].min().item(), " ".join("%.1e" % v for v in el.max(0).values.tolist()),
        " ".join("%.1e" % v for v in y["bar_layers"].min(0).values.tolist()), " ".join("%.1e" % v for v in em),
        " ".join("%.1e" % v for v in y["bar_maps"])))
    assert (et <= y["bar_total"]).all() and (el <= y["bar_layers"]).all()
    assert all(e <= bar for e, bar in zip(em, y["bar_maps"]))


@pytest.mark.parametrize("size", U.SIZES)
def test_kernel_vs_cpu_fp64(yard, params, size):
    from r2l_amd import metrics
    a, b, y = yard[size]
    p = params.cuda()
    got = metrics.lpips(a.cuda(), b.cuda(), p, return_layers=True, return_maps=True)
    assert got[0].is_cuda and got[0].dtype == torch.float32 and got[0].shape == (1,) and got[1].shape == (1, 5)
    assert [tuple(m.shape[1:]) for m in got[2]] == metrics.lpips_sizes(*size)
    compare("%dx%d" % size, got, y)
    if size in U.GOLDEN:  # (and the golden numbers themselves)
        want = torch.tensor(U.GOLDEN[size], dtype=torch.float64)
        have = torch.cat([got[0].cpu().double(), got[1][0].cpu().double()])
        assert ((have - want).abs() <= torch.cat([y["bar_total"], y["bar_layers"][0]]) + 1e-8 * want).all()
    assert torch.equal(metrics.lpips(a.cuda(), b.cuda(), p), got[0])  # maps = per_layer = NULL: the same bits
    again = metrics.lpips(a.cuda(), b.cuda(), p, return_layers=True, return_maps=True)  # a second run: the same bits
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1]) and all(torch.equal(m, n) for m, n in zip(again[2], got[2]))
    single = metrics.lpips(a[0].cuda(), b[0].cuda(), p, return_layers=True, return_maps=True)  # [H,W,3]: 0-d, the same bits
    assert single[0].dim() == 0 and single[0].item() == got[0].item() and torch.equal(single[1], got[1][0])
    ba = metrics.lpips(b.cuda(), a.cuda(), p, return_layers=True, return_maps=True)  # symmetric (within the bars)
    compare("%dx%d swapped" % size, ba, y)


def test_three_pairs_one_launch_with_the_stack_rescale(params):
    """K = 3 different pairs and the reference's rescale (main.py:361-363): the golden numbers; = three K = 1 launches bit for bit;
    without the rescale the values are visibly others."""
    from r2l_amd import metrics
    A, B, ext = U.stack_case()
    y = U.yardstick(A, B, params, rescale=ext)
    a, b, e, p = A.cuda(), B.cuda(), ext.cuda(), params.cuda()
    got = metrics.lpips(a, b, p, rescale=e, return_layers=True, return_maps=True)
    assert got[0].shape == (3,)
    compare("stack", got, y)
    want = torch.tensor(U.GOLDEN_STACK, dtype=torch.float64)
    assert ((got[0].cpu().double() - want).abs() <= y["bar_total"] + 1e-8 * want).all()
    for k in range(3):
        one = metrics.lpips(a[k], b[k], p, rescale=e, return_layers=True, return_maps=True)
        assert one[0].item() == got[0][k].item() and torch.equal(one[1], got[1][k])
        assert all(torch.equal(m, n[k]) for m, n in zip(one[2], got[2]))
    assert torch.equal(metrics.lpips(a, b, p, rescale=e), got[0])
    plain = metrics.lpips(a, b, p).cpu().double()
    assert ((plain - want).abs() > 1e-3 * want).all()


@pytest.mark.parametrize("size", [(35, 47), (400, 400)])
def test_nine_copies_in_one_launch(yard, params, size):
    """Nine copies of one pair in one launch (what render_path hands over): every one the single launch's bits."""
    from r2l_amd import metrics
    a, b, _ = yard[size]
    p = params.cuda()
    one = metrics.lpips(a.cuda(), b.cuda(), p, return_layers=True)
    k9 = metrics.lpips(a.cuda().expand(9, -1, -1, -1).contiguous(), b.cuda().expand(9, -1, -1, -1).contiguous(), p, return_layers=True)
    assert k9[0].shape == (9,) and all(v == one[0].item() for v in k9[0].tolist())
    assert all(torch.equal(k9[1][k], one[1][0]) for k in range(9))


def test_identical_images_give_exactly_zero(yard, params):
    from r2l_amd import metrics
    a, _, _ = yard[(67, 95)]
    total, layers, maps = metrics.lpips(a.cuda(), a.cuda().clone(), params.cuda(), return_layers=True, return_maps=True)
    assert total.item() == 0. and layers.abs().max().item() == 0. and all(m.abs().max().item() == 0. for m in maps)


@pytest.mark.parametrize("shape", [(1, 31, 31), (3, 35, 47), (2, 67, 95)])
def test_nothing_is_written_outside_the_buffers(params, shape):
    """The ABI called directly with work, maps, per_layer and out inside larger allocations: the guard words on both sides stay
    as set, and every word of the three outputs is written."""
    from r2l_amd import _lib, metrics
    L = _lib.load()
    K, H, W = shape
    G, SENT = 256, -12345.0
    g = torch.Generator().manual_seed(5)
    a, b = (2 * torch.rand(K, H, W, 3, generator=g) - 1).cuda(), (2 * torch.rand(K, H, W, 3, generator=g) - 1).cuda()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    flat = params.cuda()
    wpack = torch.empty(L.r2l_lpips_pack_floats(), device="cuda")
    _lib.check(L.r2l_lpips_pack(flat.data_ptr(), wpack.data_ptr(), stream), "r2l_lpips_pack")
    sizes = {"work": L.r2l_lpips_work_floats(K, H, W), "maps": K * L.r2l_lpips_map_floats(H, W), "per_layer": K * 5, "out": K}
    bufs = {k: torch.full((n + 2 * G,), SENT, device="cuda") for k, n in sizes.items()}
    ptr = {k: v.data_ptr() + 4 * G for k, v in bufs.items()}
    _lib.check(L.r2l_lpips(a.data_ptr(), b.data_ptr(), K, H, W, None, wpack.data_ptr(), ptr["work"], ptr["per_layer"], ptr["maps"],
                           ptr["out"], stream), "r2l_lpips")
    torch.cuda.synchronize()
    for k, v in bufs.items():
        assert (v[:G] == SENT).all().item() and (v[G + sizes[k]:] == SENT).all().item(), k
        if k != "work":
            assert (v[G:G + sizes[k]] != SENT).all().item(), k
    total, layers, maps = metrics.lpips(a, b, flat, return_layers=True, return_maps=True)
    assert torch.equal(bufs["out"][G:G + K], total) and torch.equal(bufs["per_layer"][G:G + 5 * K].view(K, 5), layers)
    assert torch.equal(bufs["maps"][G:G + sizes["maps"]].view(K, -1), torch.cat([m.reshape(K, -1) for m in maps], 1))


def test_render_path_reports_test_lpips(params):
    """driver.render_path on the GPU (a 2-block student, three 40x56 frames): misc['test_lpips'] is the CPU fp64 yardstick on the
    returned frames with the reference's stack rescale; without params there is no such key."""
    from model.nerf_raybased import PointSampler
    from oracle import r2l_oracle as O
    from r2l_amd import data, driver, metrics
    from tests.test_forward_gpu import build_model
    dev = torch.device("cuda")
    net = build_model(O.make_state_dict(n_block=2, seed=1), 2)
    ps = PointSampler(40, 56, 60., 16, 2., 6., device=dev)
    poses = torch.stack([data.pose_spherical(-60. + 50. * i, -30., 4.) for i in range(3)]).to(dev)
    gts = U.pair2(40, 56, 9)[1][None].repeat(3, 1, 1, 1) * torch.tensor([1., 0.8, 0.6]).view(3, 1, 1, 1)
    rgbs, misc = driver.render_path(poses, net, ps, dev, _Log(), gt_imgs=gts, lpips_params=params.cuda())
    assert rgbs.shape == (3, 40, 56, 3) and misc["test_lpips"].dim() == 0
    r = rgbs.cpu()
    ext = torch.stack([r.min(), r.max(), gts.min(), gts.max()]).double()
    want = metrics.lpips(r.double(), gts.double(), params.double(), rescale=ext).mean().item()
    plain = metrics.lpips(r.double(), gts.double(), params.double()).mean().item()
    print("render_path test_lpips %.8f, CPU fp64 yardstick %.8f (without the rescale %.8f)" % (misc["test_lpips"].item(), want, plain))
    assert abs(misc["test_lpips"].item() - want) <= 1e-5
    _, none = driver.render_path(poses, net, ps, dev, _Log(), gt_imgs=gts)
    assert "test_lpips" not in none and none["test_flip"].item() == misc["test_flip"].item()


def test_cli_logs_test_lpips(tmp_path, params):
    """`main.py --render_only --render_test --r2l_lpips_weights FILE` logs a TestLPIPS field between TestSSIM and TestFLIP."""
    from oracle import r2l_oracle as O
    from r2l_amd import driver
    from r2l_amd.checkpoint import save_ckpt
    from tests.test_driver_cpu import ROOT, make_scene
    from tests.test_forward_gpu import build_model
    from tests.test_lpips_cpu import state_dicts
    scene = str(tmp_path / "scene")
    os.makedirs(scene)
    make_scene(scene, size=128)
    tv, lins = state_dicts("lpips")
    torch.save(dict(tv, **lins), str(tmp_path / "lpips_state.pth"))
    ckpt = str(tmp_path / "SERVER-20260101-000000_iter7" / "weights" / "ckpt.tar")
    save_ckpt(ckpt, 7, build_model(O.make_state_dict(n_block=2, seed=1), 2).cpu(), {"state": {}, "param_groups": []}, 0., 0)
    args = ["--model_name", "R2L", "--config", os.path.join(ROOT, "configs", "lego_noview.txt"), "--datadir", scene,
            "--n_sample_per_ray", "16", "--netwidth", "256", "--netdepth", "6", "--use_residual", "--trial.ON", "--trial.body_arch",
            "resmlp", "--testskip", "1", "--pretrained_ckpt", ckpt, "--render_only", "--render_test", "--experiment_name", "lp",
            "--r2l_lpips_weights", str(tmp_path / "lpips_state.pth")]
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        res = driver.main(args)
    finally:
        os.chdir(cwd)
    misc = res["misc"]
    assert res["rgbs"].shape == (2, 64, 64, 3) and 0. < misc["test_lpips"].item() < 2.
    log = open(os.path.join(str(tmp_path), res["logger"].log_path, "log.txt")).read()
    want = "TestSSIM %.4f TestLPIPS %.4f TestFLIP %.4f" % (misc["test_ssim"].item(), misc["test_lpips"].item(), misc["test_flip"].item())
    assert want in log, (want, [l for l in log.splitlines() if "[TEST]" in l])
