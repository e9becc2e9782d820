"""The fused FLIP kernel (csrc/r2l_flip.hip) on the GPU: against the reference-made tests/golden/flip.npz, against the CPU
fp64 branch of metrics.flip at frame sizes, its launch invariants (bit-reproducible, K frames = K launches, map optional,
nothing written outside its buffers) and test_flip through driver.render_path.  Bars as in tests/test_flip_cpu.py."""
import ctypes

import pytest
import torch

from tests.test_flip_cpu import CASES, MEAN_BAR, _Log, case, multi

pytestmark = pytest.mark.gpu


def noisy_pair(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 3, H), torch.linspace(0, 4, W), indexing="ij")
    gt = torch.stack([0.5 + 0.5 * torch.sin(2.1 * xx + yy), 0.5 + 0.5 * torch.cos(1.3 * yy * xx), (xx / 4. + yy / 3.) / 2.], -1)
    gt = (gt + 0.1 * torch.rand(H, W, 3, generator=g)).clamp(0, 1)
    return (gt + 0.08 * torch.randn(H, W, 3, generator=g)).clamp(0, 1), gt


@pytest.fixture(scope="module")
def frames():
    """Frame-sized pairs with their CPU maps, computed once: {(H, W): (pred, gt, fp64 map, per-pixel bar)}; the bar is
    max(4 * max|CPU fp32 - CPU fp64|, 2e-5)."""
    from r2l_amd import metrics
    out = {}
    for k, (H, W) in enumerate(((401, 263), (400, 400))):
        pred, gt = noisy_pair(H, W, 21 + k)
        f64 = metrics.flip(pred.double(), gt.double(), return_map=True)[1]
        f32 = metrics.flip(pred, gt, return_map=True)[1]
        out[(H, W)] = (pred, gt, f64, max(4 * (f32.double() - f64).abs().max().item(), 2e-5))
    return out


@pytest.mark.parametrize("name", CASES)
def test_kernel_vs_reference(name):
    from r2l_amd import metrics
    pred, gt, ppd, f64, mean64, bar = case(name)
    m, f = metrics.flip(pred.cuda(), gt.cuda(), ppd, return_map=True)
    assert f.is_cuda and f.dtype == torch.float32 and f.shape == f64.shape and m.dim() == 0
    err, merr = (f.cpu().double() - f64).abs().max().item(), abs(m.item() - mean64)
    print("%s: kernel vs flip64 per pixel %.2e (bar %.2e), mean %.2e (bar %.0e)" % (name, err, bar, merr, MEAN_BAR))
    assert err <= bar and merr <= MEAN_BAR
    assert metrics.flip(pred.cuda(), gt.cuda(), ppd).item() == m.item()  # map = NULL: the same bits
    m2, f2 = metrics.flip(gt.cuda(), pred.cuda(), ppd, return_map=True)  # symmetric
    assert (f2 - f).abs().max().item() <= bar and abs(m2.item() - mean64) <= MEAN_BAR


def test_three_frames_one_launch_with_the_stack_rescale():
    """K = 3 different frames and the reference's rescale (main.py:359-379): the golden number; = three K = 1 launches bit for
    bit; the same bits on a second run and without the map; without the rescale the mean is visibly another."""
    from r2l_amd import metrics
    rec, ref, ext, f64, mean64, bar = multi()
    a, b, e = rec.cuda(), ref.cuda(), ext.cuda()
    m, f = metrics.flip(a, b, rescale=e, return_map=True)
    err, merr = (f.cpu().double() - f64).abs().max().item(), abs(m.double().mean().item() - mean64)
    print("multi: kernel vs flip64 per pixel %.2e (bar %.2e), mean %.2e" % (err, bar, merr))
    assert m.shape == (3,) and err <= bar and merr <= MEAN_BAR
    for k in range(3):
        mk, fk = metrics.flip(a[k], b[k], rescale=e, return_map=True)
        assert torch.equal(fk, f[k]) and mk.item() == m[k].item()
        assert abs(mk.item() - f64[k].mean().item()) <= MEAN_BAR
    m2, f2 = metrics.flip(a, b, rescale=e, return_map=True)
    assert torch.equal(m2, m) and torch.equal(f2, f)
    assert torch.equal(metrics.flip(a, b, rescale=e), m)
    assert abs(metrics.flip(a, b).double().mean().item() - mean64) > 1e-3


@pytest.mark.parametrize("size", [(401, 263), (400, 400)])
def test_frame_sizes_vs_cpu_fp64(frames, size):
    from r2l_amd import metrics
    pred, gt, f64, bar = frames[size]
    m, f = metrics.flip(pred.cuda(), gt.cuda(), return_map=True)
    err, merr = (f.cpu().double() - f64).abs().max().item(), abs(m.item() - f64.mean().item())
    print("%dx%d: kernel vs CPU fp64 per pixel %.2e (bar %.2e), mean %.2e" % (size + (err, bar, merr)))
    assert err <= bar and merr <= MEAN_BAR
    # nine frames in one launch (what render_path hands over): every frame the single launch's bits
    k9 = metrics.flip(pred.cuda()[None].expand(9, -1, -1, -1).contiguous(), gt.cuda()[None].expand(9, -1, -1, -1).contiguous())
    assert k9.shape == (9,) and all(v == m.item() for v in k9.tolist())


def test_identical_and_opposite_images(frames):
    from r2l_amd import metrics
    pred, gt, _, _ = frames[(401, 263)]
    m, f = metrics.flip(pred.cuda(), pred.cuda(), return_map=True)
    assert m.item() == 0. and f.abs().max().item() == 0.
    white, black = torch.ones(70, 90, 3), torch.zeros(70, 90, 3)
    want = metrics.flip(white.double(), black.double()).item()
    got = metrics.flip(white.cuda(), black.cuda()).item()
    print("white against black: kernel %.7f, CPU fp64 %.7f" % (got, want))
    assert abs(got - want) <= 1e-5 and want > 0.5


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 33, 16), (2, 70, 90)])
def test_nothing_is_written_outside_the_buffers(shape):
    """The ABI called directly with map, out and partial inside larger allocations: the guard words on both sides stay as set,
    and every word inside is written."""
    from r2l_amd import _lib
    from r2l_amd.metrics import FLIP_PPD
    L = _lib.load()
    K, H, W = shape
    G, SENT = 256, -12345.0
    g = torch.Generator().manual_seed(5)
    a, b = torch.rand(K, H, W, 3, generator=g).cuda(), torch.rand(K, H, W, 3, generator=g).cuda()
    sizes = {"partial": L.r2l_flip_partial_count(H, W, K), "map": K * H * W, "out": K}
    bufs = {k: torch.full((n + 2 * G,), SENT, device="cuda") for k, n in sizes.items()}
    ptr = {k: v.data_ptr() + 4 * G for k, v in bufs.items()}
    _lib.check(L.r2l_flip(a.data_ptr(), b.data_ptr(), K, H, W, FLIP_PPD, None, ptr["partial"], ptr["map"], ptr["out"],
                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "r2l_flip")
    torch.cuda.synchronize()
    for k, v in bufs.items():
        assert (v[:G] == SENT).all().item() and (v[G + sizes[k]:] == SENT).all().item(), k
        assert (v[G:G + sizes[k]] != SENT).all().item(), k
    from r2l_amd import metrics
    m, f = metrics.flip(a, b, return_map=True)
    assert torch.equal(bufs["out"][G:G + K], m) and torch.equal(bufs["map"][G:G + K * H * W].view(K, H, W), f)


def test_render_path_reports_test_flip():
    """driver.render_path on the GPU (a 2-block student, three 40x56 frames): misc['test_flip'] is the CPU fp64 yardstick on the
    returned frames with the reference's stack rescale."""
    from model.nerf_raybased import PointSampler
    from oracle import r2l_oracle as O
    from r2l_amd import data, driver, metrics
    from tests.test_forward_gpu import build_model
    dev = torch.device("cuda")
    net = build_model(O.make_state_dict(n_block=2, seed=1), 2)
    ps = PointSampler(40, 56, 60., 16, 2., 6., device=dev)
    poses = torch.stack([data.pose_spherical(-60. + 50. * i, -30., 4.) for i in range(3)]).to(dev)
    gts = noisy_pair(40, 56, 9)[1][None].repeat(3, 1, 1, 1) * torch.tensor([1., 0.8, 0.6]).view(3, 1, 1, 1)
    rgbs, misc = driver.render_path(poses, net, ps, dev, _Log(), gt_imgs=gts)
    assert rgbs.shape == (3, 40, 56, 3) and misc["test_flip"].dim() == 0
    r = rgbs.cpu()
    ext = torch.stack([r.min(), r.max(), gts.min(), gts.max()]).double()
    want = metrics.flip(r.double(), gts.double(), rescale=ext).mean().item()
    plain = metrics.flip(r.double(), gts.double()).mean().item()
    print("render_path test_flip %.7f, CPU fp64 yardstick %.7f (without the rescale %.7f)" % (misc["test_flip"].item(), want, plain))
    assert abs(misc["test_flip"].item() - want) <= 1e-5
