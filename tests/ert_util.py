"""Shared by tests/test_ert_cpu.py and tests/test_ert_gpu.py: the rays through the centre of the fitted scene, the masked
full render that early termination must equal, and the table of argument refusals of the four new calls (include/r2l_hip.h "early
ray termination").  The refusals happen before any launch, so the table runs on dummy pointers too."""
import ctypes

import numpy as np
import torch

from r2l_amd import _lib
from r2l_amd import ert as E
from tests.occ_fused_util import frame_desc

F32 = np.float32
INVALID = 1  # hipErrorInvalidValue


def centre_rays():
    """Every 17th pixel of the 181 x 181, focal-250 frame of teacher_util.scene_rays' camera: 1928 rays through the whole frame
    (scene_rays(R) itself returns the top rows, which all miss the scene)."""
    from tests.teacher_util import scene_rays
    rays = scene_rays(181 * 181, 0)[::17].contiguous()
    assert rays.shape == (1928, 11)
    return rays


def boundary_trans64(raw, z, rays_d, seg):
    """fp64 transmittance [R] at every segment boundary before the last segment, restated from a FULL raw."""
    S = z.shape[1]
    f = E.factors_spec(raw, z, rays_d, np.float64)
    T = np.cumprod(f, -1)
    return [T[:, s1 - 1] for s0, s1 in E.segments(S, seg)[:-1]]


def refusals():
    """[(what, call() -> return code, the text r2l_last_error must contain)] for r2l_occ_index_seg, r2l_ert_advance,
    r2l_teacher_mlp_live_into_cfg and r2l_teacher_frames_ert_cfg.  The pointers are dummies (never dereferenced)."""
    lib = _lib.load()
    P = ctypes.c_void_p(4096)
    NULL = None
    f3 = lambda *v: (ctypes.c_float * 3)(*v)
    i2 = lambda *v: (ctypes.c_int * 2)(*v)

    def good(**over):
        g = _lib.OccGridDesc()
        assert lib.r2l_occ_grid_init(ctypes.byref(g), P, 4, 2, f3(-1, -1, -1), f3(1, 1, 1)) == 0
        for k, v in over.items():
            setattr(g, k, v)
        return g

    bad_cfg = _lib.Config(precision=99)
    cases = []

    def iseg(g=NULL, R=3, S=8, s0=0, s1=4, trans=P, eps=1e-3, **over):
        a = {n: P for n in ["rays_o", "rays_d", "z", "idx_out", "count_out", "work"]}
        a.update(over)
        return lib.r2l_occ_index_seg(g, a["rays_o"], a["rays_d"], a["z"], R, S, s0, s1, trans, eps, a["idx_out"], a["count_out"],
                                     a["work"], None)

    cases += [("index_seg: NULL %s" % n, (lambda n=n: iseg(**{n: NULL})), n) for n in ["rays_o", "rays_d", "z", "idx_out", "count_out", "work"]]
    cases += [
        ("index_seg: s0 < 0", lambda: iseg(s0=-1), "s0"),
        ("index_seg: s0 == s1", lambda: iseg(s0=4, s1=4), "s0"),
        ("index_seg: s0 > s1", lambda: iseg(s0=5, s1=4), "s0"),
        ("index_seg: s1 > S", lambda: iseg(s1=9), "s1"),
        ("index_seg: R < 0", lambda: iseg(R=-1), "R is negative"),
        ("index_seg: S < 1", lambda: iseg(S=0, s0=0, s1=1), "S:"),
        ("index_seg: R*S = 2^31", lambda: iseg(R=2**23, S=256), "R*S"),
        ("index_seg: R = 2^40", lambda: iseg(R=2**40, S=8), "R*S"),
        ("index_seg: eps = 0", lambda: iseg(eps=0.), "eps"),
        ("index_seg: eps < 0", lambda: iseg(eps=-1e-3), "eps"),
        ("index_seg: eps NaN", lambda: iseg(eps=float("nan")), "eps"),
        ("index_seg: eps inf", lambda: iseg(eps=float("inf")), "eps"),
        ("index_seg: misaligned work", lambda: iseg(work=ctypes.c_void_p(4098)), "work"),
        ("index_seg: grid reserved", lambda: iseg(ctypes.byref(good(reserved=i2(7, 0)))), "reserved"),
        ("index_seg: grid G > 512", lambda: iseg(ctypes.byref(good(G=600))), "G:"),
        ("index_seg: grid NULL bits", lambda: iseg(ctypes.byref(good(bits=None))), "bits"),
        ("index_seg: grid inv", lambda: iseg(ctypes.byref(good(inv=f3(2, 0, 2)))), "inv"),
    ]

    def adv(R=3, S=8, s0=0, s1=4, **over):
        a = {n: P for n in ["raw", "z", "rays_d", "trans"]}
        a.update(over)
        return lib.r2l_ert_advance(a["raw"], a["z"], a["rays_d"], R, S, s0, s1, a["trans"], None)

    cases += [("advance: NULL %s" % n, (lambda n=n: adv(**{n: NULL})), n) for n in ["raw", "z", "rays_d", "trans"]]
    cases += [
        ("advance: s0 < 0", lambda: adv(s0=-1), "s0"),
        ("advance: s0 == s1", lambda: adv(s0=2, s1=2), "s0"),
        ("advance: s1 > S", lambda: adv(s1=9), "s1"),
        ("advance: S > 256", lambda: adv(S=257), "S:"),
        ("advance: S < 1", lambda: adv(S=0, s1=1), "S:"),
        ("advance: R < 0", lambda: adv(R=-1), "R is negative"),
        ("advance: R*S = 2^31", lambda: adv(R=2**23, S=256), "R*S"),
    ]

    def into(R=3, S=2, capacity=4, cfg=None, **over):
        names = ["rays_o", "rays_d", "viewdirs", "z", "idx", "count_dev", "wstream", "tparams", "raw"]
        a = {n: P for n in names}
        a.update(over)
        return lib.r2l_teacher_mlp_live_into_cfg(a["rays_o"], a["rays_d"], a["viewdirs"], a["z"], a["idx"], a["count_dev"], capacity,
                                                 a["wstream"], a["tparams"], a["raw"], R, S, None, cfg)

    cases += [("into: NULL %s" % n, (lambda n=n: into(**{n: NULL})), n)
              for n in ["rays_o", "rays_d", "viewdirs", "z", "idx", "count_dev", "wstream", "tparams", "raw"]]
    cases += [
        ("into: R < 0", lambda: into(R=-1), "R is negative"),
        ("into: S < 1", lambda: into(S=0), "S:"),
        ("into: R*S = 2^31", lambda: into(R=2**23, S=256), "R*S"),
        ("into: capacity < 0", lambda: into(capacity=-1), "capacity"),
        ("into: capacity > R*S", lambda: into(capacity=7), "capacity"),
        ("into: misaligned raw", lambda: into(raw=ctypes.c_void_p(4104)), "raw"),
        ("into: bad cfg", lambda: into(cfg=ctypes.byref(bad_cfg)), "precision"),
    ]

    def frames(gc=NULL, gf=NULL, desc=None, ert=None, K=1, cfg=None, work=P, null_ert=False):
        d = desc if desc is not None else frame_desc()
        e = ert if ert is not None else _lib.ErtDesc(eps=1e-3, seg=32)
        return lib.r2l_teacher_frames_ert_cfg(P, NULL, K, ctypes.byref(d), P, P, P, P, NULL, NULL, P, P, P, P, P, P, gc, gf, NULL,
                                              NULL if null_ert else ctypes.byref(e), work, None, cfg)

    cases += [
        ("frames: NULL ert", lambda: frames(null_ert=True), "ert"),
        ("frames: eps = 0", lambda: frames(ert=_lib.ErtDesc(eps=0., seg=32)), "eps"),
        ("frames: eps < 0", lambda: frames(ert=_lib.ErtDesc(eps=-1., seg=32)), "eps"),
        ("frames: eps > 0.1", lambda: frames(ert=_lib.ErtDesc(eps=0.2, seg=32)), "eps"),
        ("frames: eps NaN", lambda: frames(ert=_lib.ErtDesc(eps=float("nan"), seg=32)), "eps"),
        ("frames: seg < 8", lambda: frames(ert=_lib.ErtDesc(eps=1e-3, seg=7)), "seg"),
        ("frames: ert reserved", lambda: frames(ert=_lib.ErtDesc(eps=1e-3, seg=32, reserved=i2(0, 1))), "reserved"),
        ("frames: ndc with a grid", lambda: frames(ctypes.byref(good()), desc=frame_desc(ndc=1)), "ndc"),
        ("frames: grid_fine alone", lambda: frames(NULL, ctypes.byref(good())), "grid_fine"),
        ("frames: coarse grid reserved", lambda: frames(ctypes.byref(good(reserved=i2(0, 3)))), "reserved"),
        ("frames: fine grid G < 1", lambda: frames(ctypes.byref(good()), ctypes.byref(good(G=0))), "G:"),
        ("frames: raw_noise_std", lambda: frames(desc=frame_desc(raw_noise_std=1.)), "raw_noise_std"),
        ("frames: descriptor reserved", lambda: frames(desc=frame_desc(reserved=(ctypes.c_int * 3)(0, 1, 0))), "reserved"),
        ("frames: K < 0", lambda: frames(K=-1), "K is negative"),
        ("frames: NULL work", lambda: frames(work=NULL), "work"),
        ("frames: misaligned work", lambda: frames(work=ctypes.c_void_p(4100)), "work"),
        ("frames: bad cfg", lambda: frames(cfg=ctypes.byref(bad_cfg)), "precision"),
    ]
    return cases


def check_refusals():
    """Run the table; then the size queries and the successful no-ops that need no device."""
    lib = _lib.load()
    for what, call, needle in refusals():
        rc = call()
        msg = (lib.r2l_last_error() or b"").decode()
        assert rc == INVALID, (what, rc, msg)
        assert needle in msg, (what, msg)
    P = ctypes.c_void_p(4096)
    assert lib.r2l_occ_index_seg_work_bytes(-1) == -1 and lib.r2l_occ_index_seg_work_bytes(2**31) == -1
    assert lib.r2l_occ_index_seg_work_bytes(0) == 16 and lib.r2l_occ_index_seg_work_bytes(2049) == 16
    assert lib.r2l_occ_index_seg_work_bytes(2048 * 5 + 1) == 32
    d = frame_desc(H=5, W=7, N_samples=8, N_importance=16, chunk_rays=10)
    e = _lib.ErtDesc(eps=1e-3, seg=8)
    assert lib.r2l_teacher_frames_ert_work_floats(ctypes.byref(d), ctypes.byref(e)) == lib.r2l_teacher_frames_occ_work_floats(ctypes.byref(d)) + 12
    assert lib.r2l_teacher_frames_ert_work_floats(ctypes.byref(d), ctypes.byref(_lib.ErtDesc(eps=1e-3, seg=4))) == -1
    assert lib.r2l_teacher_frames_ert_work_floats(ctypes.byref(frame_desc(ndc=2)), ctypes.byref(e)) == -1
    assert lib.r2l_teacher_frames_ert_work_floats(ctypes.byref(d), None) == -1
    # ndc without grids passes the descriptor checks (K == 0: a successful no-op, nothing is launched)
    assert lib.r2l_teacher_frames_ert_cfg(P, None, 0, ctypes.byref(frame_desc(ndc=1)), P, P, P, P, None, None, P, P, P, P, P, P, None, None,
                                          None, ctypes.byref(e), P, None, None) == 0
    assert lib.r2l_ert_advance(P, P, P, 0, 8, 0, 4, P, None) == 0  # R == 0
    assert lib.r2l_teacher_mlp_live_into_cfg(P, P, P, P, P, P, 0, P, P, P, 0, 3, None, None) == 0  # R == 0
    return len(refusals())
