"""The VGG-16 LPIPS kernels (csrc/r2l_lpips_vgg.hip) on the GPU: against the CPU fp64 yardstick of metrics.lpips_vgg at the sizes
of tests/lpips_vgg_util.py (total, the five layer values, every map position), their launch invariants (bit-reproducible, K pairs
= K launches, maps and per_layer optional, nothing written outside the buffers), that the bars see one zeroed weight, and
test_lpips_vgg through driver.render_path and the command line.  Bars: tests/lpips_vgg_util.py."""
import ctypes
import os

import pytest
import torch

from tests import lpips_vgg_util as U
from tests.test_flip_cpu import _Log

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def params():
    return U.flat_params()


@pytest.mark.parametrize("size", U.SIZES)
def test_kernel_vs_cpu_fp64(params, size):
    from r2l_amd import metrics
    a, b, y = U.yard(size)
    p = params.cuda()
    got = metrics.lpips_vgg(a.cuda(), b.cuda(), p, return_layers=True, return_maps=True)
    assert got[0].is_cuda and got[0].dtype == torch.float32 and got[0].shape == (1,) and got[1].shape == (1, 5)
    assert [tuple(m.shape[1:]) for m in got[2]] == metrics.lpips_vgg_sizes(*size)
    U.compare("%dx%d" % size, got, y)
    want = torch.tensor(U.GOLDEN[size], dtype=torch.float64)  # (and the golden numbers themselves)
    have = torch.cat([got[0].cpu().double(), got[1][0].cpu().double()])
    assert ((have - want).abs() <= torch.cat([y["bar_total"], y["bar_layers"][0]]) + 1e-8 * want).all()
    assert torch.equal(metrics.lpips_vgg(a.cuda(), b.cuda(), p), got[0])  # maps = per_layer = NULL: the same bits
    assert torch.equal(metrics.lpips_vgg(a.cuda(), b.cuda(), p, return_layers=True)[0], got[0])
    assert torch.equal(metrics.lpips_vgg(a.cuda(), b.cuda(), p, return_maps=True)[0], got[0])
    again = metrics.lpips_vgg(a.cuda(), b.cuda(), p, return_layers=True, return_maps=True)  # a second run: the same bits
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1]) and all(torch.equal(m, n) for m, n in zip(again[2], got[2]))
    single = metrics.lpips_vgg(a[0].cuda(), b[0].cuda(), p, return_layers=True)  # [H,W,3]: 0-d, the same bits
    assert single[0].dim() == 0 and single[0].item() == got[0].item() and torch.equal(single[1], got[1][0])


def test_three_pairs_one_launch_with_the_stack_rescale(params):
    """K = 3 different pairs and the reference's rescale (main.py:361-363): the golden numbers; = three K = 1 launches bit for bit;
    a second call gives the same bits; without the rescale the values are visibly others."""
    from r2l_amd import metrics
    A, B, ext = U.stack_case()
    y = U.yardstick(A, B, params, rescale=ext)
    a, b, e, p = A.cuda(), B.cuda(), ext.cuda(), params.cuda()
    got = metrics.lpips_vgg(a, b, p, rescale=e, return_layers=True, return_maps=True)
    assert got[0].shape == (3,)
    U.compare("stack", got, y)
    want = torch.tensor(U.GOLDEN_STACK, dtype=torch.float64)
    assert ((got[0].cpu().double() - want).abs() <= y["bar_total"] + 1e-8 * want).all()
    for k in range(3):
        one = metrics.lpips_vgg(a[k], b[k], p, rescale=e, return_layers=True, return_maps=True)
        assert one[0].item() == got[0][k].item() and torch.equal(one[1], got[1][k])
        assert all(torch.equal(m, n[k]) for m, n in zip(one[2], got[2]))
    again = metrics.lpips_vgg(a, b, p, rescale=e, return_layers=True, return_maps=True)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1]) and all(torch.equal(m, n) for m, n in zip(again[2], got[2]))
    assert torch.equal(metrics.lpips_vgg(a, b, p, rescale=e), got[0])
    plain = metrics.lpips_vgg(a, b, p).cpu().double()
    assert ((plain - want).abs() > 1e-3 * want).all()


def test_identical_images_give_exactly_zero(params):
    from r2l_amd import metrics
    a, _, _ = U.yard((35, 47))
    total, layers, maps = metrics.lpips_vgg(a.cuda(), a.cuda().clone(), params.cuda(), return_layers=True, return_maps=True)
    assert total.item() == 0. and layers.abs().max().item() == 0. and all(m.abs().max().item() == 0. for m in maps)


@pytest.mark.parametrize("shape", [(1, 16, 16), (3, 17, 23), (2, 67, 95)])
def test_nothing_is_written_outside_the_buffers(params, shape):
    """The ABI called directly with work, maps, per_layer and out inside larger allocations: the guard band of 64 floats on both
    sides stays as set, and every word of the three outputs is written."""
    from r2l_amd import _lib, metrics
    L = _lib.load()
    K, H, W = shape
    G, SENT = 64, -12345.0
    g = torch.Generator().manual_seed(5)
    a, b = (2 * torch.rand(K, H, W, 3, generator=g) - 1).cuda(), (2 * torch.rand(K, H, W, 3, generator=g) - 1).cuda()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    flat = params.cuda()
    wpack = torch.empty(L.r2l_lpips_vgg_pack_floats(), device="cuda")
    _lib.check(L.r2l_lpips_vgg_pack(flat.data_ptr(), wpack.data_ptr(), stream), "r2l_lpips_vgg_pack")
    sizes = {"work": L.r2l_lpips_vgg_work_floats(K, H, W), "maps": K * L.r2l_lpips_vgg_map_floats(H, W), "per_layer": K * 5, "out": K}
    bufs = {k: torch.full((n + 2 * G,), SENT, device="cuda") for k, n in sizes.items()}
    ptr = {k: v.data_ptr() + 4 * G for k, v in bufs.items()}
    _lib.check(L.r2l_lpips_vgg(a.data_ptr(), b.data_ptr(), K, H, W, None, wpack.data_ptr(), ptr["work"], ptr["per_layer"], ptr["maps"],
                               ptr["out"], stream), "r2l_lpips_vgg")
    torch.cuda.synchronize()
    for k, v in bufs.items():
        assert (v[:G] == SENT).all().item() and (v[G + sizes[k]:] == SENT).all().item(), k
        if k != "work":
            assert (v[G:G + sizes[k]] != SENT).all().item(), k
    total, layers, maps = metrics.lpips_vgg(a, b, flat, return_layers=True, return_maps=True)
    assert torch.equal(bufs["out"][G:G + K], total) and torch.equal(bufs["per_layer"][G:G + 5 * K].view(K, 5), layers)
    assert torch.equal(bufs["maps"][G:G + sizes["maps"]].view(K, -1), torch.cat([m.reshape(K, -1) for m in maps], 1))


@pytest.mark.parametrize("zero,size", [(U.ZERO_CONV1_2, (35, 47)), (U.ZERO_CONV5_3, (130, 131))])
def test_the_bars_see_one_zeroed_weight(zero, size):
    """A packed stream with one weight of conv1_2 / of conv5_3 set to 0 before packing leaves the bars of the unmodified yardstick
    in at least one layer value."""
    from r2l_amd import metrics
    a, b, y = U.yard(size)
    _, layers, maps = metrics.lpips_vgg(a.cuda(), b.cuda(), U.flat_params(zero=zero).cuda(), return_layers=True, return_maps=True)
    over = ((layers.cpu().double() - y["layers"]).abs() / y["bar_layers"])[0]
    print("zeroed %s at %dx%d: per-layer miss in bars %s; with the maps %.1f" % (
        zero, size[0], size[1], " ".join("%.1f" % v for v in over.tolist()), U.misses((layers, maps), y)))
    assert over.max().item() > 1.


def test_render_path_reports_test_lpips_vgg(params):
    """driver.render_path on the GPU (a 2-block student, three 35x47 frames, world size 1): misc['test_lpips_vgg'] lies within the
    bar of the CPU fp64 evaluation of the returned frames with the reference's stack rescale; without params there is no such key."""
    from model.nerf_raybased import PointSampler
    from oracle import r2l_oracle as O
    from r2l_amd import data, driver, metrics
    from tests.test_forward_gpu import build_model
    dev = torch.device("cuda")
    net = build_model(O.make_state_dict(n_block=2, seed=1), 2)
    ps = PointSampler(35, 47, 50., 16, 2., 6., device=dev)
    poses = torch.stack([data.pose_spherical(-60. + 50. * i, -30., 4.) for i in range(3)]).to(dev)
    gts = U.pair2(35, 47, 9)[1][None].repeat(3, 1, 1, 1) * torch.tensor([1., 0.8, 0.6]).view(3, 1, 1, 1)
    rgbs, misc = driver.render_path(poses, net, ps, dev, _Log(), gt_imgs=gts, lpips_vgg_params=params.cuda())
    assert rgbs.shape == (3, 35, 47, 3) and misc["test_lpips_vgg"].dim() == 0 and "test_lpips" not in misc
    r = rgbs.cpu()
    ext = torch.stack([r.min(), r.max(), gts.min(), gts.max()])
    want = metrics.lpips_vgg(r.double(), gts.double(), params.double(), rescale=ext.double()).mean().item()
    cpu32 = metrics.lpips_vgg(r, gts, params, rescale=ext).mean().item()
    bar = max(4 * abs(cpu32 - want), U.REL_FLOOR * want)  # (the bar of the totals, on the mean over the frames)
    print("render_path test_lpips_vgg %.8f, CPU fp64 yardstick %.8f, bar %.2e" % (misc["test_lpips_vgg"].item(), want, bar))
    assert abs(misc["test_lpips_vgg"].item() - want) <= bar
    _, none = driver.render_path(poses, net, ps, dev, _Log(), gt_imgs=gts)
    assert "test_lpips_vgg" not in none and none["test_flip"].item() == misc["test_flip"].item()


def test_cli_logs_both_lpips_fields(tmp_path):
    """`main.py --render_only --render_test` with both LPIPS flags logs TestLPIPS and TestLPIPSvgg in that order, between TestSSIM
    and TestFLIP."""
    from oracle import r2l_oracle as O
    from r2l_amd import driver
    from r2l_amd.checkpoint import save_ckpt
    from tests.test_driver_cpu import ROOT, make_scene
    from tests.test_forward_gpu import build_model
    from tests.test_lpips_cpu import state_dicts
    from tests.test_lpips_vgg_cpu import vgg_state_dicts
    scene = str(tmp_path / "scene")
    os.makedirs(scene)
    make_scene(scene, size=128)
    tv, lins = state_dicts("lpips")
    torch.save(dict(tv, **lins), str(tmp_path / "lpips_state.pth"))
    tv, lins = vgg_state_dicts("lpips")
    torch.save(dict(tv, **lins), str(tmp_path / "lpips_vgg_state.pth"))
    ckpt = str(tmp_path / "SERVER-20260101-000000_iter7" / "weights" / "ckpt.tar")
    save_ckpt(ckpt, 7, build_model(O.make_state_dict(n_block=2, seed=1), 2).cpu(), {"state": {}, "param_groups": []}, 0., 0)
    args = ["--model_name", "R2L", "--config", os.path.join(ROOT, "configs", "lego_noview.txt"), "--datadir", scene,
            "--n_sample_per_ray", "16", "--netwidth", "256", "--netdepth", "6", "--use_residual", "--trial.ON", "--trial.body_arch",
            "resmlp", "--testskip", "1", "--pretrained_ckpt", ckpt, "--render_only", "--render_test", "--experiment_name", "lpv",
            "--r2l_lpips_weights", str(tmp_path / "lpips_state.pth"), "--r2l_lpips_vgg_weights", str(tmp_path / "lpips_vgg_state.pth")]
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        res = driver.main(args)
    finally:
        os.chdir(cwd)
    misc = res["misc"]
    assert res["rgbs"].shape == (2, 64, 64, 3) and 0. < misc["test_lpips_vgg"].item() < 2. and 0. < misc["test_lpips"].item() < 2.
    log = open(os.path.join(str(tmp_path), res["logger"].log_path, "log.txt")).read()
    want = "TestSSIM %.4f TestLPIPS %.4f TestLPIPSvgg %.4f TestFLIP %.4f" % (
        misc["test_ssim"].item(), misc["test_lpips"].item(), misc["test_lpips_vgg"].item(), misc["test_flip"].item())
    assert want in log, (want, [l for l in log.splitlines() if "[TEST]" in l])
