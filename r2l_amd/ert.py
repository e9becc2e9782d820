"""Early ray termination of the teacher's render: stop a ray once it is opaque (include/r2l_hip.h "early ray termination",
csrc/r2l_occupancy.hip, csrc/r2l_teacher_frame.hip).

An occupancy grid removes the samples in empty space.  What it cannot remove are the samples BEHIND the first opaque surface:
their cells are occupied, the ray just never gets there.  The last pass of a render (the fine pass with N_importance > 0, else the
only pass) is walked front to back in segments of `seg` consecutive sample numbers:

    zero-filled raw;  per segment [s0, s1):  index (r2l_occ_index_seg: the segment's samples that are live by the grid rule, of the
    rays whose transmittance is not below eps) -> the point network on that list, written into raw in place
    (r2l_teacher_mlp_live_into_cfg, the count read on the device) -> the transmittance through the segment (r2l_ert_advance)

and the unchanged raw2outputs follows.  A skipped sample keeps raw = 0, which raw2outputs turns into alpha = 0 exactly — the grids'
mechanism —, so a ray terminated with transmittance T_cut < eps moves its pixel by at most T_cut.  The coarse pass, its weights and
so the fine depths are untouched.

index_seg_spec / advance_spec restate the two new kernels in numpy; ert_mask is the meaning of the feature (which samples a
terminated render evaluates); ert_query is the staged form render_rays(ert=) uses, call by call.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from . import occupancy as OC
from ._lib import ptr as _ptr, stream as _stream

F32 = np.float32
EPS_MAX, SEG_MIN = 0.1, 8


def check(eps, seg):
    """(eps, seg) as the library takes them, or ValueError: 0 < eps <= 0.1, seg >= 8 (r2l_ert_desc)."""
    eps, seg = float(eps), int(seg)
    if not 0. < eps <= EPS_MAX:
        raise ValueError("early termination: eps must be in (0, %g], got %g" % (EPS_MAX, eps))
    if seg < SEG_MIN:
        raise ValueError("early termination: seg must be >= %d, got %d" % (SEG_MIN, seg))
    return eps, seg


def check_staged(eps, seg):
    """(eps, seg) as the staged calls take them, or ValueError: eps positive and finite (r2l_occ_index_seg), seg >= 1.  The tighter
    range of check() belongs to the fused call and the switches."""
    eps, seg = float(eps), int(seg)
    if not (0. < eps < float("inf")):
        raise ValueError("early termination: eps must be positive and finite, got %g" % eps)
    if seg < 1:
        raise ValueError("early termination: seg must be >= 1, got %d" % seg)
    return eps, seg


def segments(S, seg):
    """[(s0, s1)]: [j*seg, min((j+1)*seg, S))."""
    return [(s0, min(s0 + int(seg), int(S))) for s0 in range(0, int(S), int(seg))]


# ---------------------------------------------------------------------------------------------------------------
# the two kernels in numpy
# ---------------------------------------------------------------------------------------------------------------
def index_seg_spec(grid, rays_o, rays_d, z, s0, s1, trans=None, eps=0.):
    """What r2l_occ_index_seg writes: (M, idx int64[M] ascending).  grid: None or (bits, lo, inv, G) as OC.live_spec takes them.
    Sample n = r*S + s, s0 <= s < s1, is live iff its point is live by the grid rule and NOT (trans[r] < eps) — a NaN keeps its
    ray."""
    z = np.asarray(z, dtype=F32)
    R, S = z.shape
    if not 0 <= s0 < s1 <= S:
        raise ValueError("index_seg_spec: need 0 <= s0 < s1 <= S")
    live = np.ones((R, s1 - s0), dtype=bool)
    if grid is not None and R:
        bits, lo, inv, G = grid
        pts = OC.sample_points(rays_o, rays_d, z[:, s0:s1])
        live &= OC.live_spec(bits, lo, inv, G, pts.reshape(-1, 3)).reshape(R, s1 - s0)
    if trans is not None:
        with np.errstate(invalid="ignore"):
            live &= ~(np.asarray(trans, dtype=F32).reshape(R, 1) < F32(eps))
    r, sl = np.nonzero(live)  # row-major: ascending in n
    idx = (r.astype(np.int64) * S + s0 + sl).astype(np.int64)
    return int(idx.size), idx


def factors_spec(raw, z, rays_d, dtype=F32):
    """f[R,S] = (1 - alpha_s) + 1e-10 with alpha_s by raw2outputs' per-sample expressions without noise, every operation rounded to
    `dtype` (np.float32: the kernel's order with numpy's exp in place of __expf; np.float64: the reference of the tests, from the
    same fp32 inputs)."""
    raw, z, d = (np.asarray(t, dtype=F32).astype(dtype) for t in (raw, z, rays_d))
    one = dtype(1.)
    with np.errstate(over="ignore", invalid="ignore"):
        dn = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        dist = np.concatenate([z[:, 1:] - z[:, :-1], np.full_like(z[:, :1], dtype(1e10))], -1) * dn[:, None]
        alpha = one - np.exp(-np.maximum(raw[..., 3], dtype(0.)) * dist)
        return ((one - alpha) + dtype(1e-10)).astype(dtype)


def advance_spec(raw, z, rays_d, s0, s1, trans=None, dtype=F32):
    """What r2l_ert_advance leaves in trans [R]: T = 1 (s0 == 0) or trans[r], times f_s for s = s0 .. s1-1 in ascending order, one
    rounding per product."""
    f = factors_spec(raw, z, rays_d, dtype)
    R, S = f.shape
    if not 0 <= s0 < s1 <= S:
        raise ValueError("advance_spec: need 0 <= s0 < s1 <= S")
    T = np.ones(R, dtype=dtype) if s0 == 0 else np.asarray(trans).astype(dtype).copy()
    for s in range(s0, s1):
        T = (T * f[:, s]).astype(dtype)
    return T


def ert_mask(trans_at, S, seg, eps):
    """bool[R,S]: the samples early termination leaves in, given trans_at = [T at the boundary behind segment 0, 1, ...] ([R] each,
    as ert_query returns them): segment 0 whole, segment j >= 1 on the rays with NOT (trans_at[j-1] < eps)."""
    segs = segments(S, seg)
    R = len(trans_at[0]) if trans_at else None
    cols = []
    for j, (s0, s1) in enumerate(segs):
        if j == 0:
            cols.append(None)
            continue
        with np.errstate(invalid="ignore"):
            cols.append(~(np.asarray(trans_at[j - 1], dtype=F32) < F32(eps)))
    if R is None:
        return None  # one segment: everything is evaluated (the caller knows R)
    mask = np.ones((R, S), dtype=bool)
    for (s0, s1), c in zip(segs, cols):
        if c is not None:
            mask[:, s0:s1] = c[:, None]
    return mask


# ---------------------------------------------------------------------------------------------------------------
# the staged query of render_rays(ert=)
# ---------------------------------------------------------------------------------------------------------------
def index_seg(grid, rays_o, rays_d, z, s0, s1, trans, eps, idx, count, work):
    """r2l_occ_index_seg on caller-made buffers (GPU)."""
    R, S = z.shape
    _lib.check(_lib.load().r2l_occ_index_seg(None if grid is None else ctypes.byref(grid.desc()), _ptr(rays_o), _ptr(rays_d), _ptr(z),
                                             R, S, int(s0), int(s1), _ptr(trans), float(eps), _ptr(idx), _ptr(count), _ptr(work),
                                             _stream()), "r2l_occ_index_seg")


def advance(raw, z, rays_d, s0, s1, trans):
    """r2l_ert_advance in place on trans (GPU)."""
    R, S = z.shape
    _lib.check(_lib.load().r2l_ert_advance(_ptr(raw), _ptr(z), _ptr(rays_d), R, S, int(s0), int(s1), _ptr(trans), _stream()),
               "r2l_ert_advance")


def mlp_live_into(eng, rays_o, rays_d, viewdirs, z, idx, count, capacity, raw):
    """r2l_teacher_mlp_live_into_cfg: the point network at the samples idx[0 .. min(count, capacity)), written into raw in place."""
    from . import engine as _engine
    R, S = z.shape
    eng.ensure_packed()
    _lib.check(_lib.load().r2l_teacher_mlp_live_into_cfg(_ptr(rays_o), _ptr(rays_d), _ptr(viewdirs), _ptr(z), _ptr(idx), _ptr(count),
                                                         int(capacity), _ptr(eng.wstream), _ptr(eng.flat), _ptr(raw), R, S, _stream(),
                                                         ctypes.byref(_engine.merged_config(eng.cfg))),
               "r2l_teacher_mlp_live_into_cfg")


def ert_query(net, rays_o, rays_d, viewdirs, z, eps, seg, grid=None, live_acc=None, network_query_fn=None):
    """(raw[R,S,4], trans_at): the point network on the samples o + d*z walked front to back in segments of `seg`, a ray dropping
    out at the first segment boundary where its transmittance is below eps; samples that are skipped (terminated, or not live in
    `grid`, a built OccupancyGrid or None) keep raw = 0.  trans_at: the transmittance [R] the walk held at each segment boundary
    (len = number of segments - 1) — what decided the mask, for the tests.
    GPU tensors: r2l_occ_index_seg -> [r2l_occ_live_add into live_acc, an int64[2] device tensor] -> r2l_teacher_mlp_live_into_cfg
    -> r2l_ert_advance, nothing read on the host.  CPU tensors: the full raw of network_query_fn, the transmittances of advance_spec
    (fp32) on it, and the mask — a skipped sample's raw never enters a later transmittance, because its ray is gone or its own
    factor is that of raw = 0."""
    eps, seg = check_staged(eps, seg)
    R, S = z.shape
    segs = segments(S, seg)
    if z.is_cuda:
        from .render import teacher_engine
        if grid is not None:
            grid._need_built()
            if grid.bits.device != z.device:
                raise ValueError("early termination: the grid was built on %s, the rays are on %s" % (grid.bits.device, z.device))
        eng = teacher_engine(net)
        dev = z.device
        rays_o, rays_d, viewdirs, z = (t.contiguous() for t in (rays_o, rays_d, viewdirs, z))
        cap = max(R * min(seg, S), 1)
        lib = _lib.load()
        idx = torch.empty(cap, dtype=torch.int64, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        work = torch.empty(max(lib.r2l_occ_index_seg_work_bytes(cap), 16), dtype=torch.uint8, device=dev)
        trans = torch.empty(max(R, 1), dtype=torch.float32, device=dev)
        raw = torch.zeros(R, S, 4, dtype=torch.float32, device=dev)
        trans_at = []
        with torch.cuda.device(dev):
            for j, (s0, s1) in enumerate(segs):
                index_seg(grid, rays_o, rays_d, z, s0, s1, None if j == 0 else trans, eps, idx, count, work)
                if live_acc is not None:
                    _lib.check(lib.r2l_occ_live_add(_ptr(count), R * (s1 - s0), _ptr(live_acc), _stream()), "r2l_occ_live_add")
                mlp_live_into(eng, rays_o, rays_d, viewdirs, z, idx, count, R * (s1 - s0), raw)
                if s1 < S:
                    advance(raw, z, rays_d, s0, s1, trans)
                    trans_at.append(trans[:R].clone())
        return raw, trans_at
    pts = torch.from_numpy(OC.sample_points(rays_o.numpy(), rays_d.numpy(), z.numpy()))
    with torch.no_grad():
        full = network_query_fn(pts, viewdirs, net)[..., :4].float().numpy()
    keep = np.ones((R, S), dtype=bool)
    if grid is not None:
        keep = OC.live_spec(grid.words(), grid.lo, grid.inv, grid.G, pts.numpy().reshape(-1, 3)).reshape(R, S)
    raw = np.where(keep[..., None], full, F32(0.)).astype(F32)
    trans, trans_at, alive = None, [], np.ones(R, dtype=bool)
    for s0, s1 in segs:
        raw[~alive, s0:s1] = 0.
        if s1 < S:
            trans = advance_spec(raw, z.numpy(), rays_d.numpy(), s0, s1, trans)
            trans_at.append(torch.from_numpy(trans.copy()))
            with np.errstate(invalid="ignore"):
                alive = ~(trans < F32(eps))
    if live_acc is not None:
        live_acc += torch.tensor([int((raw != 0).any(-1).sum()), R * S])
    return torch.from_numpy(raw), trans_at
