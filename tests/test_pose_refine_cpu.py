"""Pose refinement against a trained student, host side (include/r2l_hip.h "pose refinement"; r2l_amd/pose_refine.py;
utils/refine_pose.py): the torch restatements against autograd and torch.optim.Adam in fp64, the pixel choice, the refusals the
library makes before any launch, the convergence of the restatement on the scenario of tests/pose_refine_util.py, and the command
line on the CPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import pose_refine_util as U
from tests.test_driver_cpu import ROOT, make_scene

SEED = 0xC0FFEE


def test_abi_is_declared_bound_and_exported():
    from r2l_amd import _lib
    header = open(os.path.join(ROOT, "include", "r2l_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("r2l_pose_key", "r2l_pose_batch", "r2l_pose_grad", "r2l_pose_update", "r2l_pose_refine_step"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and "int %s(" % name in header
    for name in ("r2l_pose_grad_work_floats", "r2l_pose_refine_work_floats"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and "int64_t %s(" % name in header
    assert "0x706F73655F726566" in header and "%X" % __import__("r2l_amd.pose_refine").pose_refine.POSE_SALT in header
    assert ctypes.sizeof(_lib.PoseRefineDesc) == 96  # no hidden padding but the tail's


def test_pose_key_and_ids():
    from r2l_amd import _lib
    from r2l_amd.keyed_perm import epoch_key
    from r2l_amd.pose_refine import POSE_SALT, pose_ids, pose_key
    lib = _lib.load()
    for it, p in ((1, 0), (17, 3), (2**40, 256)):
        want = epoch_key(epoch_key(SEED ^ POSE_SALT, it), p)
        key = ctypes.c_uint64(0)
        assert pose_key(SEED, it, p) == want
        assert lib.r2l_pose_key(SEED, it, p, ctypes.byref(key)) == 0 and key.value == want
    for bad in ((0, 0, ctypes.byref(key)), (1, -1, ctypes.byref(key)), (1, 0, None)):
        assert lib.r2l_pose_key(SEED, *bad) == 1 and b"r2l_pose_key" in lib.r2l_last_error()
    with pytest.raises(ValueError):
        pose_key(SEED, 0, 0)
    P, H, W = 3, 5, 7
    for n in (1, 9, H * W):
        ids = pose_ids(SEED, 4, P, n, H, W)
        assert np.array_equal(ids, pose_ids(SEED, 4, P, n, H, W))  # a pure function
        for p in range(P):
            seg = ids[p * n:(p + 1) * n]
            assert len(set(seg.tolist())) == n and seg.min() >= p * H * W and seg.max() < (p + 1) * H * W
            assert np.array_equal(seg, pose_ids(SEED, 4, P, H * W, H, W)[p * H * W:p * H * W + n])  # a prefix of the bijection
    full = pose_ids(SEED, 4, P, H * W, H, W).reshape(P, -1)
    assert not np.array_equal(full, pose_ids(SEED, 5, P, H * W, H, W).reshape(P, -1))  # another iteration
    assert not np.array_equal(full, pose_ids(SEED + 1, 4, P, H * W, H, W).reshape(P, -1))  # another seed
    assert not np.array_equal(full[0] % (H * W), full[1] % (H * W))  # another pose
    with pytest.raises(ValueError):
        pose_ids(SEED, 1, 1, H * W + 1, H, W)


def test_refusals_come_before_any_launch():
    """Every entry point names what it refuses and touches no device (there is none here)."""
    from r2l_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(4096)
    err = lambda: lib.r2l_last_error().decode()
    batch = dict(images=one, c2w=one, P=2, H=5, W=7, focal=9.0, seed=1, iteration=1, n=5, o=one, d=one, t=one, ids=None)
    for over, word in ((dict(images=None), "NULL"), (dict(t=None), "NULL"), (dict(P=-1), "P >= 0"), (dict(H=0), "H >= 1"),
                       (dict(focal=0.0), "focal"), (dict(iteration=0), "iteration"), (dict(n=-1), "negative"), (dict(n=36), "exceeds"),
                       (dict(P=2**20, H=2**10, W=2**10), "2^31")):
        a = dict(batch, **over)
        assert lib.r2l_pose_batch(a["images"], a["c2w"], a["P"], a["H"], a["W"], a["focal"], a["seed"], a["iteration"], a["n"], a["o"],
                                  a["d"], a["t"], a["ids"], None) == 1 and "r2l_pose_batch" in err() and word in err(), (over, err())
    assert lib.r2l_pose_batch(None, None, 0, 5, 7, 9.0, 1, 1, 5, None, None, None, None, None) == 0  # P == 0: a no-op
    assert lib.r2l_pose_batch(None, None, 2, 5, 7, 9.0, 1, 1, 0, None, None, None, None, None) == 0  # n == 0: a no-op
    g = lib.r2l_pose_grad_work_floats
    assert g(3, 256) == 0 and g(0, 10**6) == 0 and g(1, 257) == 2048 and g(24, 4096) == 3072 + 1024
    assert g(1, 2**20) == 4096 * 8 + 1024 and g(-1, 5) == -1 and g(2, 2**30) == -1
    for args, word in (((None, one, one, one, one, 1, 5, one, None, None), "NULL"), ((one,) * 5 + (1, 5, None, None, None), "NULL"),
                       ((one,) * 5 + (1, 0, one, None, None), "n >= 1"), ((one,) * 5 + (-1, 5, one, None, None), "negative"),
                       ((one,) * 5 + (2, 2**30, one, None, one), "2^31"), ((one,) * 5 + (1, 257, one, None, None), "work"),
                       ((one,) * 5 + (1, 257, one, None, ctypes.c_void_p(4100)), "work")):
        assert lib.r2l_pose_grad(*args, None) == 1 and "r2l_pose_grad" in err() and word in err(), (args, err())
    assert lib.r2l_pose_grad(None, None, None, None, None, 0, 5, None, None, None, None) == 0  # P == 0
    for args, word in (((None, one, one, one, 1), "NULL"), ((one, one, one, None, 1), "NULL"), ((one, one, one, one, -1), "negative")):
        assert lib.r2l_pose_update(*args, 1e-3, 1e-3, 0.9, 0.999, 1e-8, 1, None) == 1 and word in err(), (args, err())
    assert lib.r2l_pose_update(one, one, one, one, 1, 1e-3, 1e-3, 0.9, 0.999, 1e-8, 0, None) == 1 and "step" in err()
    good = dict(n_block=1, pack=1, P=2, H=5, W=7, focal=9.0, n=5, seed=1, iteration=1, lr_rot=2e-3, lr_trans=5e-3, beta1=0.9,
                beta2=0.999, eps=1e-8)
    ok = _lib.PoseRefineDesc(**good)
    assert lib.r2l_pose_refine_work_floats(ctypes.byref(ok)) > 0
    bad_cfg = _lib.Config(9, 0, 0, 0, 0)
    res = _lib.PoseRefineDesc(**good)
    res.reserved[2] = 1
    cases = [(_lib.PoseRefineDesc(**dict(good, **over)), word) for over, word in (
        (dict(P=0), ".P"), (dict(n=0), ".n"), (dict(n=36), ".n"), (dict(P=2**20, H=2**10, W=2**10), "2^31"),
        (dict(iteration=0), ".iteration"), (dict(focal=0.0), ".focal"), (dict(focal=float("nan")), ".focal"), (dict(n_block=-1), ".n_block"),
        (dict(pack=2), ".pack"), (dict(cfg=ctypes.pointer(bad_cfg)), "r2l_config.precision"))] + [(res, ".reserved")]
    ptrs = [one] * 10
    for d, word in cases:
        assert lib.r2l_pose_refine_work_floats(ctypes.byref(d)) == -1 and word in err(), (word, err())
        assert lib.r2l_pose_refine_step(ctypes.byref(d), *ptrs, None) == 1 and word in err(), (word, err())
    assert lib.r2l_pose_refine_step(None, *ptrs, None) == 1 and "desc is NULL" in err()
    names = ["images", "c2w", "exp_avg", "exp_avg_sq", "ztab", "params", "wstream", "wstream_bwd", "loss_out", "work"]
    for k, name in enumerate(names):
        assert lib.r2l_pose_refine_step(ctypes.byref(ok), *[None if j == k else one for j in range(10)], None) == 1
        assert name in err() and "NULL" in err(), (name, err())
    assert lib.r2l_pose_refine_step(ctypes.byref(ok), *([one] * 9 + [ctypes.c_void_p(4100)]), None) == 1 and "aligned" in err()


def test_pose_grad_spec_is_autograd_of_the_whole_map_in_fp64():
    """d sum_p mse_p / d (w, v) at 0 through R = matrix_exp([w]x) R0, t = t0 + v, the pixel rays and a small CPU student."""
    from r2l_amd.pose_refine import pose_ids, refine_step_spec, student_rgb_spec
    torch.manual_seed(3)
    P, n, H, W, focal, it = 2, 9, 5, 7, 9.0, 3
    dt = torch.float64
    model, ps = U.make_model().to(dt), U.sampler(h=H, w=W, focal=focal)
    g = torch.Generator().manual_seed(5)
    images = torch.rand(P, H, W, 3, generator=g, dtype=dt)
    c2w = torch.cat([U.rotations(P, 7), torch.tensor([[0.1, -0.2, 4.0], [0.3, 0.1, 3.8]], dtype=dt)[:, :, None]], -1)
    zero = torch.zeros(P, 6, dtype=dt)
    *_, loss, parts = refine_step_spec(model, ps, images, c2w, zero, zero, H, W, focal, SEED, it, n, 2e-3, 5e-3, 0.9, 0.999, 1e-8)
    w, v = torch.zeros(P, 3, dtype=dt, requires_grad=True), torch.zeros(P, 3, dtype=dt, requires_grad=True)
    R, t = torch.matrix_exp(U.skew(w)) @ c2w[:, :, :3], c2w[:, :, 3] + v
    ids = torch.from_numpy(pose_ids(SEED, it, P, n, H, W))
    img, pix = ids // (H * W), ids % (H * W)
    row, col = torch.div(pix, W, rounding_mode="floor"), pix % W
    dirs = torch.stack([(col.to(dt) - W * .5) / focal, -((row.to(dt) - H * .5) / focal), -torch.ones(P * n, dtype=dt)], -1)
    rgb = student_rgb_spec(model, ps, t[img], (dirs[:, None, :] * R[img]).sum(-1))
    mse = ((rgb - images.reshape(-1, 3)[ids])**2).reshape(P, -1).mean(-1)
    gw, gv = torch.autograd.grad(mse.sum(), (w, v))
    want = torch.cat([gw, gv], -1)
    rel = ((parts["grad"] - want).abs().max() / want.abs().max()).item()
    print("pose_grad_spec against autograd, fp64: worst entry %.3g of the largest" % rel)
    assert want.abs().min().item() > 0 and rel <= 1e-10
    assert torch.allclose(loss, mse.detach(), rtol=1e-12, atol=0)


@pytest.mark.parametrize("angle", [1e-9, 2e-3, 1.0])
def test_pose_update_spec_is_adam_then_matrix_exp_in_fp64(angle):
    from r2l_amd.pose_refine import pose_update_spec
    dt, P = torch.float64, 4
    lr_rot, lr_trans, b1, b2, eps = angle / 3**0.5, 5e-3, 0.9, 0.999, 1e-8  # step 1 moves every component by its lr: |dw| = angle
    g = torch.Generator().manual_seed(11)
    c2w = torch.cat([U.rotations(P, 13), torch.randn(P, 3, 1, generator=g, dtype=dt)], -1)
    m, v = torch.zeros(P, 6, dtype=dt), torch.zeros(P, 6, dtype=dt)
    pw, pv = torch.zeros(P, 3, dtype=dt, requires_grad=True), torch.zeros(P, 3, dtype=dt, requires_grad=True)
    opt = torch.optim.Adam([{"params": [pw], "lr": lr_rot}, {"params": [pv], "lr": lr_trans}], betas=(b1, b2), eps=eps)
    worst = 0.0
    for step in (1, 2, 3):
        grad = torch.randn(P, 6, generator=g, dtype=dt) * 0.3 + 1.0
        before = torch.cat([pw, pv], -1).detach().clone()
        pw.grad, pv.grad = grad[:, :3].clone(), grad[:, 3:].clone()
        opt.step()
        delta = torch.cat([pw, pv], -1).detach() - before
        if step == 1:
            assert torch.allclose(delta[:, :3].norm(dim=-1), torch.full((P,), angle, dtype=dt), rtol=1e-6)
        want = torch.cat([torch.matrix_exp(U.skew(delta[:, :3])) @ c2w[:, :, :3], (c2w[:, :, 3] + delta[:, 3:])[:, :, None]], -1)
        c2w, m, v = pose_update_spec(c2w, m, v, grad, lr_rot, lr_trans, b1, b2, eps, step)
        st = opt.state[pw]
        assert torch.allclose(m[:, :3], st["exp_avg"], rtol=1e-14, atol=0) and torch.allclose(v[:, :3], st["exp_avg_sq"], rtol=1e-14, atol=0)
        worst = max(worst, (c2w - want).abs().max().item())
        c2w = want  # (both continue from the same pose)
    print("pose_update_spec against Adam + matrix_exp at angle %g: worst entry %.3g" % (angle, worst))
    assert worst <= 1e-12


def test_pose_update_spec_properties_in_fp32():
    from r2l_amd.pose_refine import pose_update_spec
    P = 3
    g = torch.Generator().manual_seed(17)
    c2w = torch.cat([U.rotations(P, 19, torch.float32), torch.randn(P, 3, 1, generator=g)], -1)
    assert c2w.dtype == torch.float32
    zero = torch.zeros(P, 6)
    # a zero gradient (on zero moments): every bit stays
    c1, m1, v1 = pose_update_spec(c2w, zero, zero, zero, 2e-3, 5e-3, 0.9, 0.999, 1e-8, 1)
    assert torch.equal(c1.view(torch.int32), c2w.view(torch.int32)) and torch.equal(m1, zero) and torch.equal(v1, zero)
    # a non-finite gradient: that pose and its moments keep their bits, the others move
    m0, v0 = torch.rand(P, 6, generator=g) - 0.5, torch.rand(P, 6, generator=g)
    grad = torch.randn(P, 6, generator=g)
    for bad in (float("nan"), float("inf")):
        gb = grad.clone()
        gb[1, 4] = bad
        c1, m1, v1 = pose_update_spec(c2w, m0, v0, gb, 2e-3, 5e-3, 0.9, 0.999, 1e-8, 7)
        for new, old in ((c1, c2w), (m1, m0), (v1, v0)):
            assert torch.equal(new[1], old[1]) and bool(torch.isfinite(new).all())
            assert not torch.equal(new[0], old[0]) and not torch.equal(new[2], old[2])
        cg, mg, vg = pose_update_spec(c2w, m0, v0, grad, 2e-3, 5e-3, 0.9, 0.999, 1e-8, 7)
        assert torch.equal(c1[0], cg[0]) and torch.equal(m1[2], mg[2]) and torch.equal(v1[2], vg[2])
    # 1000 updates: R stays orthonormal
    c, m, v = c2w, zero, zero
    for step in range(1, 1001):
        c, m, v = pose_update_spec(c, m, v, torch.randn(P, 6, generator=g), 2e-3, 5e-3, 0.9, 0.999, 1e-8, step)
    R = c[:, :, :3].double()
    off = (R.transpose(1, 2) @ R - torch.eye(3, dtype=torch.float64)).abs().max().item()
    print("R^T R - I after 1000 fp32 updates: %.3g" % off)
    assert off <= 1e-6 and bool((torch.linalg.det(R) > 0).all())


def test_pose_batch_spec_is_the_image_sampler_row_for_row():
    """Rows p n .. of pose_batch_spec are image_batch.host_batch's for img = p, the whole frame and pose_key's key."""
    from r2l_amd.image_batch import full_window, host_batch
    from r2l_amd.pose_refine import pose_batch_spec, pose_key
    P, n, H, W, focal, it = 3, 11, 5, 7, 6.5, 9
    g = torch.Generator().manual_seed(23)
    images = torch.rand(P, H, W, 3, generator=g)
    poses = torch.cat([U.rotations(P, 29, torch.float32), torch.randn(P, 3, 1, generator=g)], -1)
    o, d, t, ids = pose_batch_spec(images, poses, H, W, focal, SEED, it, n)
    for p in range(P):
        ho, hd, _, ht, hid = host_batch(images, poses, H, W, focal, 0, p, full_window(H, W), pose_key(SEED, it, p), n)
        s = slice(p * n, (p + 1) * n)
        assert torch.equal(o[s], ho) and torch.equal(t[s], ht) and np.array_equal(ids[s], np.asarray(hid))
        assert torch.allclose(d[s], hd, rtol=0, atol=2**-22)  # (get_rays sums in torch's order, pixel_ray in the kernel's)


def test_rotation_angle_reads_small_angles():
    from r2l_amd.pose_refine import pose_errors
    for deg in (1e-5, 4e-3, 2.0, 179.0):
        w = torch.tensor([[0.6, 0.0, 0.8]], dtype=torch.float64) * np.deg2rad(deg)
        a = torch.cat([U.rotations(1, 31), torch.zeros(1, 3, 1, dtype=torch.float64)], -1)
        b = torch.cat([torch.matrix_exp(U.skew(w)) @ a[:, :, :3], torch.tensor([[[3e-4], [0.], [4e-4]]], dtype=torch.float64)], -1)
        rot, tr = pose_errors(a, b)
        assert abs(rot.item() - deg) <= 1e-6 * deg + 1e-9 and abs(tr.item() - 5e-4) < 1e-12


def test_refiner_converges_on_the_cpu():
    """The scenario of tests/pose_refine_util.py: 2 degrees and 0.05 away, n = 1024, default rates, 100 iterations."""
    from r2l_amd.pose_refine import PoseRefiner
    model, ps = U.load_student(), U.sampler()
    true, start = U.start_poses(1)
    r = PoseRefiner(model, ps, U.observed(model, ps, true), start, U.N_RAYS)
    rot0, tr0 = r.pose_errors(true)
    assert abs(rot0.item() - U.START_DEG) < 1e-3 and abs(tr0.item() - U.START_DIST) < 1e-5
    r.step()
    r.run(U.ITERS - 1)
    rot1, tr1 = r.pose_errors(true)
    losses = r.losses
    print("CPU restatement, fp32: rotation %.4f -> %.5f degrees, translation %.4f -> %.2e, loss %.3e -> %.3e" % (
        rot0.item(), rot1.item(), tr0.item(), tr1.item(), losses[0, 0].item(), losses[-1, 0].item()))
    assert r.iteration == U.ITERS and losses.shape == (U.ITERS, 1) and r.poses.shape == (1, 3, 4)
    assert rot1.item() <= rot0.item() / 10 and tr1.item() <= tr0.item() / 10
    assert losses[-1, 0].item() < losses[0, 0].item() / 10


def test_refiner_refuses_what_it_cannot_run():
    from r2l_amd.pose_refine import PoseRefiner
    model, ps = U.make_model(), U.sampler(h=5, w=7, focal=9.0)
    images, poses = torch.rand(2, 5, 7, 3), U.true_pose().expand(2, 3, 4)
    PoseRefiner(model, ps, images, torch.eye(4).expand(2, 4, 4), 35)
    for a, kw in (((images, poses[:, :2], 5), "init_poses"), ((images[:1], poses, 5), "images"), ((images, poses, 36), "n_rays"),
                  ((images, poses, 0), "n_rays")):
        with pytest.raises(ValueError, match=kw):
            PoseRefiner(model, ps, *a)


def test_cli_on_the_cpu(tmp_path, monkeypatch):
    """utils/refine_pose.py on a tiny scene: both error lines, the .npy, and the two refusals."""
    from r2l_amd import refine_pose
    from r2l_amd.checkpoint import save_ckpt
    from r2l_amd.options import parse_args
    from model.nerf_raybased import NeRF_v3_2
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    scene = str(tmp_path / "scene")
    os.makedirs(scene)
    make_scene(scene)
    common = ["--model_name", "R2L", "--config", os.path.join(ROOT, "configs", "lego_noview.txt"), "--datadir", scene,
              "--n_sample_per_ray", "16", "--netwidth", "256", "--netdepth", "4", "--use_residual", "--trial.ON", "--trial.body_arch",
              "resmlp", "--testskip", "1", "--experiment_name", "refine"]
    torch.manual_seed(0)
    ck = save_ckpt(str(tmp_path / "student.tar"), 1, NeRF_v3_2(parse_args(common), 1008, 3), {"state": {}, "param_groups": []}, 0., 0)
    run = common + ["--pretrained_ckpt", ck, "--r2l_pose_iters", "3", "--r2l_pose_rays", "20"]
    out = refine_pose.main(run + ["--r2l_pose_out", str(tmp_path / "refined.npy"), "--r2l_pose_noise", "1,0.02"])
    saved = np.load(str(tmp_path / "refined.npy"))
    assert saved.shape == (2, 3, 4) and saved.dtype == np.float32 and np.array_equal(saved, out["poses"].numpy())
    assert out["losses"].shape == (3, 2) and not np.array_equal(saved, out["init"].numpy())
    rot0, tr0, _, _ = out["errors"]
    assert torch.allclose(rot0, torch.full((2,), 1.0, dtype=torch.float64), atol=1e-3) and torch.allclose(
        tr0, torch.full((2,), 0.02, dtype=torch.float64), atol=1e-5)
    log = open(os.path.join(out["logger"].log_path, "log.txt")).read()
    assert "[POSE] rotation error before" in log and "[POSE] translation error before" in log and "[POSE] view 1 (image 4 of the scene):" in log
    # a start from a file, [P,4,4]; the default output path
    init = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
    init[:, :3, :4] = out["true"].numpy()
    np.save(str(tmp_path / "init.npy"), init)
    again = refine_pose.main(run + ["--r2l_pose_init", str(tmp_path / "init.npy")])
    assert os.path.basename(again["out"]) == "refined_poses.npy" and np.load(again["out"]).shape == (2, 3, 4)
    assert float(again["errors"][0].max()) == 0.0
    np.save(str(tmp_path / "bad.npy"), np.zeros((2, 4, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="r2l_pose_init"):
        refine_pose.main(run + ["--r2l_pose_init", str(tmp_path / "bad.npy")])
    with pytest.raises(ValueError, match="r2l_pose_rays"):
        refine_pose.main(common + ["--pretrained_ckpt", ck, "--r2l_pose_iters", "3", "--r2l_pose_rays", "37"])  # 6 x 6 frames


def test_the_other_drivers_accept_the_pose_options():
    from r2l_amd.options import parse_args
    a = parse_args(["--r2l_pose_iters", "7", "--r2l_pose_noise", "3,0.1"])
    assert a.r2l_pose_iters == 7 and a.r2l_pose_rays == 4096 and a.r2l_pose_lr == "2e-3,5e-3" and a.r2l_pose_out == ""
