"""Shared by tests/test_occ_fused_cpu.py and tests/test_occ_fused_gpu.py: the fused frames next to the per-pose occupancy render
they must equal, the online-KD run of the driver tests, and the table of argument refusals of the new calls (include/r2l_hip.h
"occupancy inside the fused frames call").  The refusals happen before any launch, so the table runs on dummy pointers too."""
import ctypes
import os

import torch

from oracle import r2l_oracle as O
from r2l_amd import _lib

INVALID = 1  # hipErrorInvalidValue
KHW = (3, 20, 24)
FOCAL = 28.
NEAR, FAR = 2., 6.
SEED, FID0 = (1 << 35) + 11, 5


def poses(K, first=0):
    """K poses on the r = 4 sphere that look at the origin, where the fitted scene of tests/teacher_util.py sits."""
    return torch.stack([torch.from_numpy(O.pose_spherical(-170. + 47. * (first + k), -15. - 20. * ((first + k) % 3), 4.)[:3, :4])
                        for k in range(K)], 0).float().cuda()


def same(a, b):
    """Bit for bit (disp = 1 / max(1e-10, depth / acc) is NaN where acc == 0: compared by bits)."""
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def fused(nets, khw, Ns, Ni, perturb, white, occupancy=None, live_acc=None, fine=True, K=None, first=0, frame_id0=FID0, chunk=0,
          rows=False):
    from r2l_amd.render import render_frames
    coarse, fine_net = nets
    K = khw[0] if K is None else K
    with torch.no_grad():
        return render_frames(poses(K, first), khw[1], khw[2], FOCAL, NEAR, FAR, coarse, fine_net if fine else None, Ns, Ni, perturb,
                             white, SEED, frame_id0=frame_id0, chunk=chunk, rows=rows, occupancy=occupancy, live_acc=live_acc)


def per_pose(nets, khw, Ns, Ni, perturb, white, occupancy, fine=True):
    """The per-pose path, frame by frame: render(..., occupancy=pair, t_rand=, u=) fed the rays of frame_rays and the draws of
    draw_uniform under the documented stream ids.  Returns (outputs, live points, total points) — the counts of the pair's grids."""
    from r2l_amd.render import draw_uniform, frame_rays, render
    K, H, W = khw
    coarse, fine_net = nets
    fine_net = fine_net if fine else None
    o, d, _ = frame_rays(poses(K), H, W, FOCAL)
    grids = list({id(g): g for g in (occupancy or ())}.values())
    for g in grids:
        g.reset_counters()
    out = {k: [] for k in ("rgb", "disp", "acc", "depth", "rgb0")}
    with torch.no_grad():
        for k in range(K):
            s = slice(k * H * W, (k + 1) * H * W)
            t_rand = u = None
            if perturb:
                t_rand = draw_uniform(H * W * Ns, SEED, 2 * (FID0 + k), "cuda").view(H * W, Ns)
                u = draw_uniform(H * W * Ni, SEED, 2 * (FID0 + k) + 1, "cuda").view(H * W, Ni) if Ni else None
            rgb, disp, acc, ex = render(H, W, FOCAL, chunk=H * W, rays=torch.stack([o[s], d[s]], 0), ndc=False, near=NEAR, far=FAR,
                                        use_viewdirs=True, network_fn=coarse, network_query_fn=None, N_samples=Ns, N_importance=Ni,
                                        network_fine=fine_net, white_bkgd=white, perturb=float(perturb), raw_noise_std=0.,
                                        t_rand=t_rand, u=u, occupancy=occupancy)
            for name, val in (("rgb", rgb), ("disp", disp), ("acc", acc), ("depth", ex["depth_map"]), ("rgb0", ex.get("rgb0"))):
                out[name].append(val)
    out = {k: (torch.cat(v, 0) if v[0] is not None else None) for k, v in out.items()}
    return out, sum(g.live_points for g in grids), sum(g.total_points for g in grids)


def assert_same_frames(got, want, Ni):
    for name in ("rgb", "disp", "acc", "depth"):
        assert same(got[name], want[name]), name
    if Ni > 0:
        assert same(got["rgb0"], want["rgb0"]) and not torch.equal(got["rgb0"], got["rgb"])
    else:
        assert got["rgb0"] is None and want["rgb0"] is None


def frame_desc(**over):
    kw = dict(H=4, W=4, focal=10., near=2., far=6., N_samples=8, N_importance=0, perturb=0, white_bkgd=0, raw_noise_std=0.,
              chunk_rays=0, seed=1, frame_id0=0)
    kw.update(over)
    return _lib.TeacherFrameDesc(**kw)


def online_kd_run(work, ck, tag, extra):
    """main.py --r2l_online_kd for two iterations on a tiny scene under `work`: (the store's shards as a list of tensors, the log)."""
    from r2l_amd import driver
    from r2l_amd.raystore import CompactRayStore, RayStore
    from tests.test_driver_cpu import ROOT, make_scene
    scene = str(work / "scene")
    if not os.path.exists(scene):
        os.makedirs(scene)
        make_scene(scene, size=128)
    keep = []
    closes = {c: c.close for c in (RayStore, CompactRayStore)}
    try:
        for c in closes:  # the test reads the store after the run
            c.close = lambda self: None
        argv = ["--model_name", "R2L", "--config", os.path.join(ROOT, "configs", "lego_noview.txt"), "--datadir", scene,
                "--n_sample_per_ray", "16", "--netwidth", "256", "--netdepth", "6", "--use_residual", "--trial.ON", "--trial.body_arch",
                "resmlp", "--testskip", "1", "--N_rand", "2", "--hard_ratio", "0.2", "--hard_mul", "2", "--warmup_lr", "0.0001,200",
                "--i_print", "1", "--experiment_name", "occkd_" + tag, "--r2l_online_kd", "--r2l_teacher_config", os.path.join(ROOT, "configs", "lego.txt"), "--teacher_ckpt", ck,
                "--n_pose_kd", "3", "--create_data_chunk", "2", "--N_iters", "2"] + list(extra)
        res = driver.main(argv)
        loader = res["loader"]
        n = loader.n_shards * loader.rows_per_file
        keep = [loader.data[:n].clone()]  # plain: [o, d, rgb] rows; compact: { rgb, ray id } rows
        if hasattr(loader, "append_frames"):
            keep += [loader.pose_c2w.clone(), loader.pose_focal.clone()]
    finally:
        for c, f in closes.items():
            c.close = f
    res["loader"].close()
    return keep, open(os.path.join(res["logger"].log_path, "log.txt")).read()


def refusals():
    """[(what, call() -> return code, the text r2l_last_error must contain)]: every refusal include/r2l_hip.h lists for the new
    calls.  The pointers are dummies (never dereferenced: the check comes before any launch)."""
    lib = _lib.load()
    P = ctypes.c_void_p(4096)  # a non-NULL, 16-byte aligned address nobody reads
    NULL = None
    f3 = lambda *v: (ctypes.c_float * 3)(*v)

    def good(**over):
        g = _lib.OccGridDesc()
        assert lib.r2l_occ_grid_init(ctypes.byref(g), P, 4, 2, f3(-1, -1, -1), f3(1, 1, 1)) == 0
        for k, v in over.items():
            setattr(g, k, v)
        return g

    bad_cfg = _lib.Config(precision=99)
    cases = []

    def live(R=3, S=2, cfg=None, **over):
        names = ["rays_o", "rays_d", "viewdirs", "z", "idx", "count_dev", "wstream", "tparams", "raw"]
        a = {n: P for n in names}
        a.update(over)
        return lib.r2l_teacher_mlp_live_cfg(*[a[n] for n in names], R, S, None, cfg)

    cases += [("live: NULL %s" % n, (lambda n=n: live(**{n: NULL})), n)
              for n in ["rays_o", "rays_d", "viewdirs", "z", "idx", "count_dev", "wstream", "tparams", "raw"]]
    cases += [
        ("live: R < 0", lambda: live(R=-1), "R is negative"),
        ("live: S < 1", lambda: live(S=0), "S:"),
        ("live: R*S = 2^31", lambda: live(R=2**23, S=256), "R*S"),
        ("live: R = 2^40", lambda: live(R=2**40, S=1), "R*S"),
        ("live: misaligned raw", lambda: live(raw=ctypes.c_void_p(4104)), "raw"),
        ("live: bad cfg", lambda: live(cfg=ctypes.byref(bad_cfg)), "precision"),
    ]

    def index(g, R=3, S=2, **over):
        names = ["rays_o", "rays_d", "z", "idx_out", "count_out", "work"]
        a = {n: P for n in names}
        a.update(over)
        return lib.r2l_occ_index(g, a["rays_o"], a["rays_d"], a["z"], R, S, a["idx_out"], a["count_out"], a["work"], None)

    cases += [("index: NULL %s" % n, (lambda n=n: index(ctypes.byref(good()), **{n: NULL})), n)
              for n in ["rays_o", "rays_d", "z", "idx_out", "count_out", "work"]]
    cases += [
        ("index: NULL grid", lambda: index(NULL), "grid"),
        ("index: reserved", lambda: index(ctypes.byref(good(reserved=(ctypes.c_int * 2)(7, 0)))), "reserved"),
        ("index: G > 512", lambda: index(ctypes.byref(good(G=600))), "G:"),
        ("index: NULL bits", lambda: index(ctypes.byref(good(bits=None))), "bits"),
        ("index: R < 0", lambda: index(ctypes.byref(good()), R=-1), "R is negative"),
        ("index: S < 1", lambda: index(ctypes.byref(good()), S=0), "S:"),
        ("index: R*S = 2^31", lambda: index(ctypes.byref(good()), R=2**23, S=256), "R*S"),
        ("index: misaligned work", lambda: index(ctypes.byref(good()), work=ctypes.c_void_p(4098)), "work"),
        ("live_add: NULL count", lambda: lib.r2l_occ_live_add(NULL, 5, P, None), "count"),
        ("live_add: NULL live_acc", lambda: lib.r2l_occ_live_add(P, 5, NULL, None), "live_acc"),
        ("live_add: total < 0", lambda: lib.r2l_occ_live_add(P, -1, P, None), "total"),
    ]

    def frames(gc, gf=NULL, desc=None, K=1, cfg=None, work=P):
        d = desc if desc is not None else frame_desc()
        return lib.r2l_teacher_frames_occ_cfg(P, NULL, K, ctypes.byref(d), P, P, P, P, NULL, NULL, P, P, P, P, P, P, gc, gf, NULL, work,
                                              None, cfg)

    cases += [
        ("frames: NULL grid_coarse", lambda: frames(NULL), "grid_coarse"),
        ("frames: coarse grid reserved", lambda: frames(ctypes.byref(good(reserved=(ctypes.c_int * 2)(0, 3)))), "reserved"),
        ("frames: coarse grid NULL bits", lambda: frames(ctypes.byref(good(bits=None))), "bits"),
        ("frames: fine grid G < 1", lambda: frames(ctypes.byref(good()), ctypes.byref(good(G=0))), "G:"),
        ("frames: fine grid inv", lambda: frames(ctypes.byref(good()), ctypes.byref(good(inv=f3(2, 0, 2)))), "inv"),
        ("frames: ndc", lambda: frames(ctypes.byref(good()), desc=frame_desc(ndc=1)), "ndc"),
        ("frames: descriptor reserved", lambda: frames(ctypes.byref(good()), desc=frame_desc(reserved=(ctypes.c_int * 3)(0, 1, 0))),
         "reserved"),
        ("frames: K < 0", lambda: frames(ctypes.byref(good()), K=-1), "K is negative"),
        ("frames: NULL work", lambda: frames(ctypes.byref(good()), work=NULL), "work"),
        ("frames: misaligned work", lambda: frames(ctypes.byref(good()), work=ctypes.c_void_p(4100)), "work"),
        ("frames: bad cfg", lambda: frames(ctypes.byref(good()), cfg=ctypes.byref(bad_cfg)), "precision"),
    ]
    return cases


def check_refusals():
    """Run the table: every case returns hipErrorInvalidValue and r2l_last_error names the argument.  Also the size queries and
    the successful no-ops that need no device."""
    lib = _lib.load()
    for what, call, needle in refusals():
        rc = call()
        msg = (lib.r2l_last_error() or b"").decode()
        assert rc == INVALID, (what, rc, msg)
        assert needle in msg, (what, msg)
    assert lib.r2l_occ_index_work_bytes(-1) == -1 and lib.r2l_occ_index_work_bytes(2**31) == -1
    assert lib.r2l_teacher_frames_occ_work_floats(ctypes.byref(frame_desc(ndc=2))) == -1
    P = ctypes.c_void_p(4096)
    assert lib.r2l_teacher_mlp_live_cfg(P, P, P, P, P, P, P, P, P, 0, 3, None, None) == 0  # R == 0: a successful no-op
    return len(refusals())
