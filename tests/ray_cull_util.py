"""Shared by tests/test_ray_cull_cpu.py and tests/test_ray_cull_gpu.py: rays whose samples sit on the edges of the ray rule, the
refusal table of the new calls (include/r2l_hip.h r2l_occ_rays, r2l_store_append_live) — it runs on dummy pointers: the checks come
before any launch —, and the set-up of the comparison with the teacher's unskipped frames."""
import ctypes

import numpy as np
import torch

from oracle import r2l_oracle as O
from r2l_amd import _lib
from r2l_amd import occupancy as OC
from tests.occupancy_util import grid_with_bits  # noqa: F401

F32 = np.float32
INVALID = 1  # hipErrorInvalidValue
MISS_CAP = 0.01  # the cap the grid tests use (tests/test_occ_fused_gpu.py)

# the comparison with the teacher's frames: camera at radius 4, 48 x 48, near 2, far 6.  A point outside the box is live, so the
# box must contain every segment whole: along the view axis a segment runs from radius 2 to radius 2 behind the origin, and at
# t = 6 it is at most 6 * 24/40 * sqrt(2) = 5.1 off the axis (largest coordinate of this pose's segments: 4.8).  +-6 at 128^3 has the
# cell side (0.094) of 64^3 over +-3.  A narrower frame (focal 60) is mostly scene and has too few dead rays for the 30 % the test
# asks for
T_BOX, T_G, T_HW, T_FOCAL, T_NEAR, T_FAR = 6., 128, 48, 40., 2., 6.


def cull_rays(R, G, seed=0, lo=-1., hi=1.):
    """(o, d) float32 [R,3] through and past the box [lo, hi)^3 of a G^3 grid, made like occupancy_util.edge_rays: random rays; every
    7th axis-parallel with o on the lower face, so that with near = 0, far = hi - lo and T = G / 2 or G its samples fall ON cell
    faces; every 5th starts far outside and points away (all samples outside: live); o of every 11th has a NaN, d of every 13th an
    inf.  Ray 0 stays a plain random ray."""
    rs = np.random.RandomState(seed * 7919 + R + 31 * G)
    o = (rs.rand(R, 3) * 1.6 - 0.8).astype(F32) * F32(hi)
    d = (rs.randn(R, 3) * 0.4).astype(F32)
    o[7::7, 0] = lo
    o[7::7, 1:] = (rs.randint(0, G, size=(len(range(7, R, 7)), 2)).astype(F32) * F32((hi - lo) / G) + F32(lo)).astype(F32)  # on faces
    d[7::7] = (1., 0., 0.)
    o[5::5] = (3. * hi, 0., 0.)
    d[5::5] = (1., 0., 0.)
    o[11::11, 1] = np.nan
    d[13::13, 2] = np.inf
    return o, d


def inside_rays(R, seed=0):
    """Rays whose segment [0, 1] stays inside [-1, 1)^3: with an empty grid every one is dead."""
    rs = np.random.RandomState(seed + R)
    return (rs.rand(R, 3) * 0.8 - 0.4).astype(F32), (rs.rand(R, 3) * 0.8 - 0.4).astype(F32)


def spec(grid, o, d, near, far, T):
    return OC.rays_spec(grid.words(), grid.lo, grid.inv, grid.G, o, d, near, far, T)


def refusals():
    """[(what, call() -> return code, the text r2l_last_error must contain)] of r2l_occ_rays, r2l_rays_gather, r2l_rgb_scatter_bg
    and r2l_store_append_live.  The pointers are dummies (never dereferenced: the check comes before any launch)."""
    lib = _lib.load()
    P = ctypes.c_void_p(4096)
    NULL = None
    f3 = lambda *v: (ctypes.c_float * 3)(*v)

    def good(**over):
        g = _lib.OccGridDesc()
        assert lib.r2l_occ_grid_init(ctypes.byref(g), P, 4, 2, f3(-1, -1, -1), f3(1, 1, 1)) == 0
        for k, v in over.items():
            setattr(g, k, v)
        return g

    def rays(g, R=3, near=2., far=6., T=8, live=P, **over):
        a = {n: P for n in ("rays_o", "rays_d", "idx_out", "count_out", "work")}
        a.update(over)
        return lib.r2l_occ_rays(g, a["rays_o"], a["rays_d"], R, near, far, T, a["idx_out"], a["count_out"], live, a["work"], None)

    ok = lambda: ctypes.byref(good())
    cases = [("rays: NULL %s" % n, (lambda n=n: rays(ok(), **{n: NULL})), n) for n in ("rays_o", "rays_d", "idx_out", "count_out", "work")]
    cases += [
        ("rays: NULL grid", lambda: rays(NULL), "grid"),
        ("rays: NULL bits", lambda: rays(ctypes.byref(good(bits=None))), "bits"),
        ("rays: G > 512", lambda: rays(ctypes.byref(good(G=600))), "G:"),
        ("rays: inv", lambda: rays(ctypes.byref(good(inv=f3(2, 0, 2)))), "inv"),
        ("rays: reserved", lambda: rays(ctypes.byref(good(reserved=(ctypes.c_int * 2)(0, 3)))), "reserved"),
        ("rays: R < 0", lambda: rays(ok(), R=-1), "R is negative"),
        ("rays: R = 2^31", lambda: rays(ok(), R=2**31), "R:"),
        ("rays: T < 1", lambda: rays(ok(), T=0), "T:"),
        ("rays: NaN near", lambda: rays(ok(), near=float("nan")), "near"),
        ("rays: inf far", lambda: rays(ok(), far=float("inf")), "far"),
        ("rays: far < near", lambda: rays(ok(), near=6., far=2.), "near <= far"),
        ("rays: far - near overflows", lambda: rays(ok(), near=-3e38, far=3e38), "fp32 range"),
        ("rays: misaligned work", lambda: rays(ok(), work=ctypes.c_void_p(4098)), "work"),
    ]
    gather = lambda o=P, d=P, R=4, idx=P, M=2, oo=P, od=P: lib.r2l_rays_gather(o, d, R, idx, M, oo, od, None)
    cases += [
        ("gather: R < 0", lambda: gather(R=-1), "R:"),
        ("gather: M < 0", lambda: gather(M=-1), "M:"),
        ("gather: NULL idx", lambda: gather(idx=NULL), "idx"),
        ("gather: NULL rays_o", lambda: gather(o=NULL), "rays_o"),
        ("gather: NULL rays_d", lambda: gather(d=NULL), "rays_d"),
        ("gather: NULL out_o", lambda: gather(oo=NULL), "out_o"),
        ("gather: NULL out_d", lambda: gather(od=NULL), "out_d"),
    ]
    scat = lambda rgb=P, idx=P, M=2, live=P, bg=1., out=P, R=4: lib.r2l_rgb_scatter_bg(rgb, idx, M, live, bg, out, R, None)
    cases += [
        ("scatter_bg: R < 0", lambda: scat(R=-1), "R:"),
        ("scatter_bg: M > R", lambda: scat(M=5), "M:"),
        ("scatter_bg: M < 0", lambda: scat(M=-1), "M:"),
        ("scatter_bg: NaN bg", lambda: scat(bg=float("nan")), "bg"),
        ("scatter_bg: NULL live", lambda: scat(live=NULL), "live"),
        ("scatter_bg: NULL rgb_out", lambda: scat(out=NULL), "rgb_out"),
        ("scatter_bg: NULL rgb_live", lambda: scat(rgb=NULL), "rgb_live"),
        ("scatter_bg: NULL idx", lambda: scat(idx=NULL), "idx"),
    ]
    m = ctypes.c_int64(-7)

    def app(rows=P, n_rows=100, idx=P, M=8, store=P, cap=4, first=0, rps=4, out=ctypes.byref(m)):
        return lib.r2l_store_append_live(rows, n_rows, idx, M, store, cap, first, rps, 5, 1, out, None)

    cases += [
        ("append_live: NULL rows_in", lambda: app(rows=NULL), "pointer"),
        ("append_live: NULL store", lambda: app(store=NULL), "pointer"),
        ("append_live: NULL n_written_out", lambda: app(out=NULL), "pointer"),
        ("append_live: rays_per_shard 6", lambda: app(rps=6), "rays_per_shard"),
        ("append_live: rays_per_shard 0", lambda: app(rps=0), "rays_per_shard"),
        ("append_live: n_rows < 0", lambda: app(n_rows=-1), "n_rows"),
        ("append_live: M < 0", lambda: app(M=-1), "M is negative"),
        ("append_live: NULL idx", lambda: app(idx=NULL), "idx"),
        ("append_live: first_shard < 0", lambda: app(first=-1), "first_shard"),
        ("append_live: over capacity", lambda: app(M=20), "capacity_shards"),
        ("append_live: first + m over capacity", lambda: app(first=3), "capacity_shards"),
    ]
    return cases, m


def check_refusals():
    lib = _lib.load()
    cases, m = refusals()
    for what, call, needle in cases:
        rc = call()
        msg = (lib.r2l_last_error() or b"").decode()
        assert rc == INVALID, (what, rc, msg)
        assert needle in msg and "r2l_" in msg, (what, msg)
    assert m.value == -7  # no refused append wrote its count
    assert lib.r2l_occ_rays_work_bytes(-1) == -1 and lib.r2l_occ_rays_work_bytes(2**31) == -1
    assert lib.r2l_occ_rays_work_bytes(0) == 16 and lib.r2l_occ_rays_work_bytes(2049) == 16 + 2064
    return len(cases)


# ---- the comparison with the teacher's unskipped frames --------------------------------------------------------------------------------
def teacher_pose():
    return torch.from_numpy(O.pose_spherical(35., -25., 4.)[:3, :4]).float()[None]


def teacher_frame_rays():
    """(o, d) float32 numpy [48*48, 3]: the rays of r2l_frame_rays for teacher_pose(), in its arithmetic (raystore.pixel_ray_spec)."""
    from r2l_amd.raystore import pixel_ray_spec
    H = W = T_HW
    row, col = np.divmod(np.arange(H * W), W)
    c = np.broadcast_to(teacher_pose().numpy(), (H * W, 3, 4))
    return pixel_ray_spec(c, np.full(H * W, T_FOCAL, F32), H, W, row, col)


def dead_ray_miss_share(rgb_full, live, white):
    """(share of the dead rays whose unskipped colour is more than 1e-3 from the background, share of dead rays)."""
    dead = np.asarray(live) == 0
    off = np.abs(np.asarray(rgb_full, dtype=np.float64) - (1. if white else 0.)).max(-1) > 1e-3
    return float((off & dead).sum()) / max(int(dead.sum()), 1), float(dead.mean())
