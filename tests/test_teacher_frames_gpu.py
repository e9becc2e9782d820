"""Teacher frames from poses in one library call, on the GPU (include/r2l_hip.h r2l_draw_uniform / r2l_frame_rays /
r2l_teacher_frames_cfg; r2l_amd/render.py draw_uniform / frame_rays / render_frames; --r2l_fused_frames): the draws against
the Philox restatement, the rays against fp64, the fused frame against the stages it is made of (bit for bit), independence of
grouping and chunking, the row layout, and the two CLI users."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import r2l_oracle as O
from tests.test_driver_cpu import ROOT, make_scene, oracle_teacher_frame
from tests.test_teacher_frames_cpu import draw_uniform_np

pytestmark = pytest.mark.gpu

U = 2.0**-24  # unit roundoff of fp32
NEAR, FAR = 2., 6.


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _poses(K, first=0):
    return torch.stack([torch.from_numpy(O.pose_spherical(-170. + 47. * (first + k), -15. - 20. * ((first + k) % 3), 4.)[:3, :4])
                        for k in range(K)], 0).float().cuda()


_NETS = {}


def nets():
    """(coarse, fine) NeRF modules of the seeded teacher pair, built once per process and left unchanged."""
    if not _NETS:
        from r2l_amd.nerf_raybased import NeRF
        mods = []
        for sd in O.make_teacher_state_dicts(7, 2, alpha_bias=0.5):
            m = NeRF(D=8, W=256, input_ch=63, output_ch=4, skips=[4], input_ch_views=27, use_viewdirs=True)
            m.load_state_dict(sd)
            for q in m.parameters():
                q.requires_grad = False
            mods.append(m.cuda().eval())
        _NETS["pair"] = tuple(mods)
    return _NETS["pair"]


def _same(a, b):
    """Bit for bit, NaN == NaN (disp = 1 / max(1e-10, depth / acc) is NaN where acc == 0)."""
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


# ---- 5. draws -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,stream_id", [(12345, 6), ((1 << 40) + 977, (1 << 33) + 5)])
def test_draw_uniform_is_the_philox_stream(seed, stream_id):
    from r2l_amd.render import draw_uniform
    rows = {}
    for sid in (stream_id, stream_id + 1):
        for n in (1, 3, 4, 5, 4099):
            got = draw_uniform(n, seed, sid, "cuda").cpu().numpy()
            assert got.dtype == np.float32 and got.shape == (n,)
            assert np.array_equal(got, draw_uniform_np(n, seed, sid)), (n, seed, sid)
            assert (got >= 0).all() and (got < 1).all()
        rows[sid] = got
    assert not np.array_equal(rows[stream_id], rows[stream_id + 1])
    assert not np.array_equal(rows[stream_id], draw_uniform(4099, seed + 1, stream_id, "cuda").cpu().numpy())
    assert abs(rows[stream_id].mean() - .5) < .03  # (4099 uniforms: sigma of the mean 0.0045)
    # the bytes behind the last element stay as they were
    buf = torch.full((16,), -7., device="cuda")
    from r2l_amd import _lib
    _lib.check(_lib.load().r2l_draw_uniform(_p(buf), 5, seed, stream_id, _st()), "r2l_draw_uniform")
    assert np.array_equal(buf[:5].cpu().numpy(), draw_uniform_np(5, seed, stream_id)) and bool((buf[5:] == -7.).all())


# ---- 6. rays --------------------------------------------------------------------------------------------------------------
def rays_fp64(c2ws, focals, H, W):
    """(o [K*H*W,3] fp32, d64 [K*H*W,3], bound [K*H*W,3]) of the header's formula in fp64 from the same fp32 inputs;
    bound = 4 * 2^-24 * sum_j |dirs_j R_ij|: every term carries at most two roundings (the division, the product), two adds follow."""
    K = c2ws.shape[0]
    c = c2ws.double().cpu()
    f = torch.as_tensor(focals, dtype=torch.float32).reshape(-1).double().cpu().expand(K)
    row, col = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    d64, bound, o = [], [], []
    for k in range(K):
        dirs = torch.stack([(col - W * .5) / f[k], -(row - H * .5) / f[k], -torch.ones_like(col)], -1).reshape(-1, 1, 3)
        terms = dirs * c[k, :3, :3][None]  # [HW, i, j]
        d64.append(terms.sum(-1))
        bound.append(4 * U * terms.abs().sum(-1))
        o.append(c2ws[k, :3, 3].cpu()[None].expand(H * W, 3))
    return torch.cat(o), torch.cat(d64), torch.cat(bound)


@pytest.mark.parametrize("K,H,W", [(1, 1, 1), (2, 5, 7), (3, 20, 24), (1, 33, 31)])
def test_frame_rays_vs_fp64(K, H, W):
    from r2l_amd import _lib
    from r2l_amd.render import frame_rays
    lib = _lib.load()
    c2ws = _poses(K)
    focals = torch.tensor([27.5 + 3.25 * k for k in range(K)], device="cuda")
    R, G = K * H * W, 8  # G guard floats behind every output
    bufs = {n: torch.full((R * w + G,), -7., device="cuda") for n, w in (("o", 3), ("d", 3), ("v", 3), ("rows", 9))}
    fdev = focals if K > 1 else None
    _lib.check(lib.r2l_frame_rays(_p(c2ws), _p(fdev), float(focals[0]), K, H, W, _p(bufs["o"]), _p(bufs["d"]), _p(bufs["v"]),
                                  _p(bufs["rows"]), _st()), "r2l_frame_rays")
    for n, w in (("o", 3), ("d", 3), ("v", 3), ("rows", 9)):
        assert bool((bufs[n][R * w:] == -7.).all()), n  # nothing written past the end
    o, d, v = (bufs[n][:R * 3].view(R, 3).cpu() for n in "odv")
    rows = bufs["rows"][:R * 9].view(R, 9).cpu()
    want_o, d64, bound = rays_fp64(c2ws, focals if K > 1 else focals[:1], H, W)
    assert torch.equal(o, want_o)
    err = (d.double() - d64).abs()
    print("rays_d: max |d - d64| / bound = %.3f" % (err / bound.clamp_min(1e-300)).max().item())
    assert bool((err <= bound).all())
    v64 = d.double() / d.double().norm(dim=-1, keepdim=True)
    verr = (v.double() - v64).abs().max().item()
    print("viewdirs: max error %.2f x 2^-24" % (verr / U))
    assert verr <= 8 * U
    assert torch.equal(rows[:, :3], o) and torch.equal(rows[:, 3:6], d) and bool((rows[:, 6:] == -7.).all())
    # the Python wrapper, and outputs left out
    wo, wd, wv = frame_rays(c2ws, H, W, focals if K > 1 else float(focals[0]))
    assert torch.equal(wo.cpu(), o) and torch.equal(wd.cpu(), d) and torch.equal(wv.cpu(), v)
    only_d = torch.full((R * 3 + G,), -7., device="cuda")
    _lib.check(lib.r2l_frame_rays(_p(c2ws), _p(fdev), float(focals[0]), K, H, W, None, _p(only_d), None, None, _st()), "r2l_frame_rays")
    assert torch.equal(only_d[:R * 3].view(R, 3).cpu(), d) and bool((only_d[R * 3:] == -7.).all())


# ---- 7. fused = unfused -------------------------------------------------------------------------------------------------
KHW = (3, 20, 24)
FOCAL = 28.
SEED, FID0 = (1 << 35) + 11, 5


def _fused(N_samples, N_importance, perturb, white, fine=True, K=KHW[0], first=0, frame_id0=FID0, chunk=0, rows=False):
    from r2l_amd.render import render_frames
    coarse, fine_net = nets()
    with torch.no_grad():
        return render_frames(_poses(K, first), KHW[1], KHW[2], FOCAL, NEAR, FAR, coarse, fine_net if fine else None, N_samples,
                             N_importance, perturb, white, SEED, frame_id0=frame_id0, chunk=chunk, rows=rows)


def _unfused(N_samples, N_importance, perturb, white, fine=True):
    """The existing path, frame by frame, fed the rays of frame_rays: render() with perturb = 0, render_rays with the draws
    of draw_uniform under the documented stream ids with perturb = 1."""
    from r2l_amd.render import draw_uniform, frame_rays, render, render_rays
    K, H, W = KHW
    coarse, fine_net = nets()
    fine_net = fine_net if fine else None
    o, d, v = frame_rays(_poses(K), H, W, FOCAL)
    out = {k: [] for k in ("rgb", "disp", "acc", "depth", "rgb0")}
    with torch.no_grad():
        for k in range(K):
            s = slice(k * H * W, (k + 1) * H * W)
            if perturb == 0:
                rgb, disp, acc, ex = render(H, W, FOCAL, chunk=H * W, rays=torch.stack([o[s], d[s]], 0), ndc=False, near=NEAR,
                                            far=FAR, use_viewdirs=True, network_fn=coarse, network_query_fn=None,
                                            N_samples=N_samples, N_importance=N_importance, network_fine=fine_net,
                                            white_bkgd=white, perturb=0., raw_noise_std=0.)
                depth, rgb0 = ex["depth_map"], ex.get("rgb0")
            else:
                ones = torch.ones_like(d[s][:, :1])
                t_rand = draw_uniform(H * W * N_samples, SEED, 2 * (FID0 + k), "cuda").view(H * W, N_samples)
                u = draw_uniform(H * W * N_importance, SEED, 2 * (FID0 + k) + 1, "cuda").view(H * W, N_importance) if N_importance else None
                r = render_rays(torch.cat([o[s], d[s], NEAR * ones, FAR * ones, v[s]], -1), coarse, None, N_samples, perturb=1.,
                                N_importance=N_importance, network_fine=fine_net, white_bkgd=white, t_rand=t_rand, u=u)
                rgb, disp, acc, depth, rgb0 = r["rgb_map"], r["disp_map"], r["acc_map"], r["depth_map"], r.get("rgb0")
            for name, val in (("rgb", rgb), ("disp", disp), ("acc", acc), ("depth", depth), ("rgb0", rgb0)):
                out[name].append(val)
    return {k: (torch.cat(v, 0) if v[0] is not None else None) for k, v in out.items()}


@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("perturb", [0, 1])
@pytest.mark.parametrize("N_samples,N_importance", [(64, 128), (16, 16), (8, 0)])
def test_fused_frames_equal_the_stages(N_samples, N_importance, perturb, white):
    got = _fused(N_samples, N_importance, perturb, white)
    want = _unfused(N_samples, N_importance, perturb, white)
    R = KHW[0] * KHW[1] * KHW[2]
    assert got["rgb"].shape == (R, 3) and got["acc"].shape == (R,) and bool(torch.isfinite(got["rgb"]).all())
    for name in ("rgb", "acc", "depth"):
        assert torch.equal(got[name], want[name]), name
    assert _same(got["disp"], want["disp"])
    if N_importance > 0:
        assert torch.equal(got["rgb0"], want["rgb0"]) and not torch.equal(got["rgb0"], got["rgb"])
    else:
        assert got["rgb0"] is None and want["rgb0"] is None
    assert got["rows"] is None


@pytest.mark.parametrize("perturb", [0, 1])
def test_fused_frames_without_a_fine_net(perturb):
    """network_fine = None: the coarse net serves both passes (render_rays' rule)."""
    got = _fused(64, 128, perturb, True, fine=False)
    want = _unfused(64, 128, perturb, True, fine=False)
    for name in ("rgb", "acc", "depth", "rgb0"):
        assert torch.equal(got[name], want[name]), name
    assert _same(got["disp"], want["disp"])
    assert not torch.equal(got["rgb"], _fused(64, 128, perturb, True)["rgb"])  # (the fine net is not a no-op)


# ---- 8. grouping and chunking -------------------------------------------------------------------------------------------
def test_grouping_and_chunking_do_not_change_the_frames():
    names = ("rgb", "disp", "acc", "depth", "rgb0")
    whole = _fused(64, 128, 1, True)
    ones = [_fused(64, 128, 1, True, K=1, first=k, frame_id0=FID0 + k) for k in range(KHW[0])]
    for n in names:
        assert _same(whole[n], torch.cat([f[n] for f in ones], 0)), n
    for chunk in (100, 480):  # 480 = H * W: one pass; 100: five passes, the last of 80 rays
        part = _fused(64, 128, 1, True, chunk=chunk)
        for n in names:
            assert _same(whole[n], part[n]), (n, chunk)
    assert not torch.equal(whole["rgb"], _fused(64, 128, 1, True, frame_id0=FID0 + 1)["rgb"])  # (the draws do matter)


# ---- 9. row layout ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [0, 100])
def test_rows_are_o_d_rgb(chunk):
    from r2l_amd.render import frame_rays
    plain = _fused(64, 128, 1, True, chunk=chunk)
    rows = _fused(64, 128, 1, True, chunk=chunk, rows=True)
    o, d, _ = frame_rays(_poses(KHW[0]), KHW[1], KHW[2], FOCAL)
    assert rows["rows"].shape == (KHW[0] * KHW[1] * KHW[2], 9)
    assert torch.equal(rows["rows"], torch.cat([o, d, rows["rgb"]], -1))
    for n in ("rgb", "disp", "acc", "depth", "rgb0"):
        assert _same(plain[n], rows[n]), n


def test_rows_without_the_other_outputs():
    """rows alone (every other output NULL): the final rgb goes through the work buffer into the rows."""
    from r2l_amd import _lib, engine
    from r2l_amd.render import teacher_engine
    lib = _lib.load()
    K, H, W = KHW
    want = _fused(64, 128, 1, True, rows=True)["rows"]
    coarse, fine = (teacher_engine(m) for m in nets())
    desc = _lib.TeacherFrameDesc(H=H, W=W, focal=FOCAL, near=NEAR, far=FAR, N_samples=64, N_importance=128, perturb=1, white_bkgd=1,
                                 raw_noise_std=0., chunk_rays=100, seed=SEED, frame_id0=FID0)
    n = lib.r2l_teacher_frames_work_floats(ctypes.byref(desc))
    work = torch.full((n + 8,), -7., device="cuda")
    rows = torch.full((K * H * W * 9 + 8,), -7., device="cuda")
    t = torch.linspace(0., 1., steps=64)
    ttab = torch.cat([t, 1. - t]).cuda()
    _lib.check(lib.r2l_teacher_frames_cfg(_p(_poses(K)), None, K, ctypes.byref(desc), _p(ttab), None, _p(coarse.wstream),
                                          _p(coarse.flat), _p(fine.wstream), _p(fine.flat), _p(rows), None, None, None, None, None,
                                          _p(work), _st(), ctypes.byref(engine.merged_config(coarse.cfg))), "r2l_teacher_frames_cfg")
    assert torch.equal(rows[:-8].view(-1, 9), want)
    assert bool((rows[-8:] == -7.).all()) and bool((work[n:] == -7.).all())  # nothing written past either buffer


# ---- 10. CLI ------------------------------------------------------------------------------------------------------------
def test_cli_fused_frames(tmp_path, monkeypatch):
    from r2l_amd import create_data, data, driver
    monkeypatch.chdir(tmp_path)
    scene = str(tmp_path / "scene")
    os.makedirs(scene)
    make_scene(scene, size=128)  # half_res -> 64x64 = 4096 rays per pose = one shard per pose
    csd, fsd = O.make_teacher_state_dicts(5, 2, alpha_bias=0.5)
    ck = str(tmp_path / "teacher.tar")
    torch.save({"global_step": 200000, "network_fn_state_dict": csd, "network_fine_state_dict": fsd}, ck)
    common = ["--create_data", "rand", "--config", os.path.join(ROOT, "configs", "lego.txt"), "--datadir", scene, "--teacher_ckpt", ck,
              "--n_pose_kd", "3", "--create_data_chunk", "2", "--perturb", "0"]
    outs, shards, logs = {}, {}, {}
    for tag, extra in (("plain", []), ("fused", ["--r2l_fused_frames", "--test_teacher", "--testskip", "1"])):
        kd = str(tmp_path / ("pseudo_" + tag))
        outs[tag] = create_data.main(common + ["--datadir_kd", scene + ":" + kd, "--experiment_name", "cd_" + tag] + extra)
        assert outs[tag]["n_rays"] == 3 * 4096
        shards[tag] = {f: np.load(os.path.join(kd, f)) for f in sorted(os.listdir(kd))}
        logs[tag] = open(os.path.join(outs[tag]["logger"].log_path, "log.txt")).read()
    assert list(shards["plain"]) == list(shards["fused"]) == ["data_0.npy", "data_1.npy", "data_2.npy"]
    assert "teacher frames: fused" in logs["fused"] and "teacher frames: render() per pose" in logs["plain"]
    # the rank's stream replayed: pose, focal scale, pose, focal scale, flush seed, pose, focal scale, flush seed
    H = W = 64
    focal = float(data.load_blender_data(scene, True, 1)[3][2])
    rng, groups, want = np.random.RandomState(0), [], {}
    for group in ((1, 2), (3,)):
        pf = [(torch.as_tensor(data.get_rand_pose(rng), dtype=torch.float32)[:3, :4], focal * (1 + rng.rand())) for _ in group]
        groups.append((pf, int(rng.randint(0, 2**31 - 1))))
    first = 0
    for pf, seed in groups:
        o, d64, bound = rays_fp64(torch.stack([p for p, _ in pf], 0), [f for _, f in pf], H, W)
        r = np.random.RandomState(seed)
        p1, p2 = r.permutation(o.shape[0]), r.permutation(o.shape[0])
        perm = p1[p2]
        for j in range(len(pf)):
            s = perm[j * 4096:(j + 1) * 4096]
            want["data_%d.npy" % (first + j)] = (o[s].numpy(), d64[s].numpy(), bound[s].numpy())
        first += len(pf)
    for f in shards["fused"]:
        a, b = shards["plain"][f], shards["fused"][f]
        o, d64, bound = want[f]
        assert a.shape == b.shape == (4096, 9) and b.dtype == np.float32
        assert np.array_equal(b[:, :3], o) and np.array_equal(a[:, :3], o)  # same poses, same permutations: row by row
        safe = np.maximum(bound, 1e-300)  # (a bound of 0: all three terms are 0 and so are both results)
        r_fused = (np.abs(b[:, 3:6].astype(np.float64) - d64) / safe).max()
        r_pair = (np.abs(b[:, 3:6].astype(np.float64) - a[:, 3:6]) / safe).max()
        e_rgb = np.abs(a[:, 6:] - b[:, 6:]).max()
        print("%s: |d_fused - d64| / bound %.3f, |d_fused - d_plain| / bound %.3f, max |rgb_fused - rgb_plain| %.2e" %
              (f, r_fused, r_pair, e_rgb))
        assert r_fused <= 1. and r_pair <= 1.
        assert e_rgb < 1e-4
    # --test_teacher through the fused frames: Loss / PSNR of the oracle's frames
    line = [l for l in logs["fused"].splitlines() if "Teacher test: Loss" in l]
    assert len(line) == 1
    imgs, poses, _, hwf, i_split = data.load_blender_data(scene, True, 1)
    imgs = torch.as_tensor(imgs)
    gts = imgs[..., :3] * imgs[..., -1:] + (1. - imgs[..., -1:])
    mse = np.mean([O.img2mse(oracle_teacher_frame(csd, fsd, poses[i], 64, 64, float(hwf[2])), gts[i]).item() for i in i_split[2]])
    got = [float(v) for v in line[0].split("Teacher test: Loss ")[1].replace("PSNR", "").split()]
    assert abs(got[0] - mse) < 2e-4 and abs(got[1] + 10. * np.log10(mse)) < 2e-3, (line[0], mse)
    # main.py --model_name nerf --render_only --render_test --r2l_fused_frames
    res = driver.main(["--model_name", "nerf", "--config", os.path.join(ROOT, "configs", "lego.txt"), "--datadir", scene,
                       "--pretrained_ckpt", ck, "--testskip", "1", "--render_only", "--render_test", "--r2l_fused_frames",
                       "--experiment_name", "Test__NeRF__fused"])
    assert res["rgbs"].shape == (2, 64, 64, 3) and np.isfinite(res["misc"]["test_psnr"].item())
    assert "teacher frames: fused" in open(os.path.join(res["logger"].log_path, "log.txt")).read()
    assert abs(res["misc"]["test_loss"].item() - mse) < 2e-4
