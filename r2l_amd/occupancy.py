"""Occupancy grid of the teacher's render: skip the sample points that lie in empty space (include/r2l_hip.h "occupancy grid",
csrc/r2l_occupancy.hip).

A trained NeRF of a bounded scene has a negative sigma pre-activation in most of the box; raw2outputs turns such a sample into
alpha = 0 exactly, so it contributes exactly nothing.  OccupancyGrid keeps one bit per cell of a box — set where any of the
cell's k^3 probes has sigma > sigma_thresh, then dilated — and render_rays(..., occupancy=(grid_coarse, grid_fine)) sends only
the live samples (cell bit set, or outside the box) through the point network:

    compact (r2l_occ_compact) -> read M (8 bytes, the one synchronisation) -> TeacherEngine.mlp on [M] rows with S = 1
    -> scatter (r2l_occ_scatter) into a zero-filled raw[R,S,4] -> the unchanged raw2outputs / sample_pdf_sort.

Inside the fused frames call (render_frames(occupancy=pair), --r2l_occ_fused) the count never leaves the device:

    index (r2l_occ_index: compact's idx and count, no row copies) -> TeacherEngine.mlp_live on the index list (the kernels' live
    form reads the count itself and writes raw in place) -> the unchanged raw2outputs / sample_pdf_sort.

While the teacher trains (TeacherTrainer(occupancy=pair), --r2l_occ_train) the same index list serves the forward with stash and
the backward (r2l_teacher_mlp_train_live, r2l_teacher_backward_live); TrainOccupancy below holds the driver's refresh rule, and
OccupancyGrid.rebuild refills a grid in place.

build_spec / compact_spec / scatter_spec restate the three library calls in numpy: they are what CPU tensors run, and what
the tests hold the kernels to bit for bit.
"""
import ctypes
import time

import numpy as np
import torch

from . import _lib
from ._lib import ptr as _ptr, stream as _stream

F32 = np.float32
G_MAX, K_MAX = 512, 4


# ---------------------------------------------------------------------------------------------------------------
# the arithmetic pinned in include/r2l_hip.h, in numpy (every operation rounded to fp32 on its own)
# ---------------------------------------------------------------------------------------------------------------
def grid_fields(lo, hi, G, k):
    """(lo, inv, step), float32[3] each: inv = (float)G / (hi - lo), step = (hi - lo) / (float)(G*k) (r2l_occ_grid_init)."""
    lo, hi = np.asarray(lo, dtype=F32).reshape(3), np.asarray(hi, dtype=F32).reshape(3)
    G, k = int(G), int(k)
    if not 1 <= G <= G_MAX:
        raise ValueError("occupancy grid: G must be in 1 .. %d, got %d" % (G_MAX, G))
    if not 1 <= k <= K_MAX:
        raise ValueError("occupancy grid: k must be in 1 .. %d, got %d" % (K_MAX, k))
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo < hi).all()):
        raise ValueError("occupancy grid: need finite lo[a] < hi[a] on every axis, got lo %s hi %s" % (lo, hi))
    side = (hi - lo).astype(F32)
    return lo, (F32(G) / side).astype(F32), (side / F32(G * k)).astype(F32)


def n_words(G):
    return (int(G)**3 + 31) // 32


def probe_axis(lo_a, step_a, G, k):
    """float32[G*k]: probe p = c*k + j of one axis sits at lo + ((float)p + 0.5f) * step."""
    p = np.arange(int(G) * int(k)).astype(F32)
    return (F32(lo_a) + ((p + F32(.5)).astype(F32) * F32(step_a)).astype(F32)).astype(F32)


def probe_points(lo, step, G, k):
    """float32[(G k)^3, 3] in probe order: probe (px, py, pz) has the place (pz*G*k + py)*G*k + px."""
    ax = [probe_axis(lo[a], step[a], G, k) for a in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x, y, z], -1).reshape(-1, 3)


def pack_bits(occ):
    """bool[G,G,G] indexed [cz,cy,cx] -> uint32[ceil(G^3/32)]: cell i = (cz*G + cy)*G + cx is bit i & 31 of word i >> 5."""
    occ = np.asarray(occ, dtype=bool)
    flat = occ.reshape(-1)
    pad = np.zeros(n_words(occ.shape[0]) * 32, dtype=np.uint64)
    pad[:flat.size] = flat
    return (pad.reshape(-1, 32) << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32)


def unpack_bits(bits, G):
    """uint32 words -> bool[G,G,G] indexed [cz,cy,cx]."""
    w = np.asarray(bits).astype(np.uint32).reshape(-1)
    flat = ((w[:, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(-1)
    return flat[:int(G)**3].reshape(G, G, G)


def build_spec(sigma, G, k, dilate=0, sigma_thresh=0.):
    """What r2l_occ_build writes to bits, given the probe sigma [(G k)^3] in probe order: a cell is occupied iff any of its k^3
    probes has sigma > sigma_thresh (a NaN is not above anything), then the box maximum over (2 dilate + 1)^3 cells clipped at the
    grid's faces.  Returns uint32[ceil(G^3/32)], padding bits zero."""
    G, k, dilate = int(G), int(k), int(dilate)
    if dilate < 0:
        raise ValueError("occupancy grid: dilate must be >= 0")
    s = np.asarray(sigma, dtype=F32).reshape(G, k, G, k, G, k)  # [cz, jz, cy, jy, cx, jx]
    occ = (s > F32(sigma_thresh)).any(axis=(1, 3, 5))
    d = min(dilate, G - 1)
    for axis in range(3):
        if d == 0:
            break
        out = occ.copy()
        for off in range(1, d + 1):
            a = [slice(None)] * 3
            b = [slice(None)] * 3
            a[axis], b[axis] = slice(off, None), slice(None, G - off)
            out[tuple(b)] |= occ[tuple(a)]  # cell c sees c + off
            out[tuple(a)] |= occ[tuple(b)]  # cell c sees c - off
        occ = out
    return pack_bits(occ)


def live_spec(bits, lo, inv, G, pts):
    """bool[n]: live = outside the box, or the cell's bit.  c = floorf((p - lo) * inv), difference and product rounded
    separately; inside iff 0 <= c < G on all axes (NaN / inf: outside)."""
    pts = np.asarray(pts, dtype=F32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor(((pts - np.asarray(lo, dtype=F32)).astype(F32) * np.asarray(inv, dtype=F32)).astype(F32))
        inside = ((f >= 0) & (f < F32(G))).all(1)
    c = np.where(inside[:, None], f, 0).astype(np.int64)
    i = (c[:, 2] * G + c[:, 1]) * G + c[:, 0]
    w = np.asarray(bits).astype(np.uint32).reshape(-1)
    bit = ((w[i >> 5] >> (i & 31).astype(np.uint32)) & 1).astype(bool)
    return ~inside | bit


def sample_points(rays_o, rays_d, z):
    """float32[R,S,3]: rays_o + rays_d * z, product and sum rounded separately (as r2l_teacher_mlp_cfg forms its points)."""
    o, d, z = (np.asarray(t, dtype=F32) for t in (rays_o, rays_d, z))
    with np.errstate(invalid="ignore", over="ignore"):
        return (o[:, None, :] + (d[:, None, :] * z[:, :, None]).astype(F32)).astype(F32)


def compact_spec(bits, lo, inv, G, rays_o, rays_d, viewdirs, z):
    """What r2l_occ_compact writes: (M, idx int64[M] ascending, out_o, out_d, out_v float32[M,3], out_z float32[M])."""
    o, d, v, z = (np.asarray(t, dtype=F32) for t in (rays_o, rays_d, viewdirs, z))
    R, S = z.shape
    live = live_spec(bits, lo, inv, G, sample_points(o, d, z).reshape(-1, 3)) if R else np.zeros(0, dtype=bool)
    idx = np.flatnonzero(live).astype(np.int64)
    r = idx // max(S, 1)
    return int(idx.size), idx, o[r], d[r], v[r], z.reshape(-1)[idx]


def ray_depths(near, far, T):
    """float32[T]: t_j = near + ((float)j + 0.5f) * dt, dt = (far - near) / (float)T, every operation rounded separately — the
    depths r2l_occ_rays steps along a ray."""
    near, far, T = F32(near), F32(far), int(T)
    if T < 1 or not (np.isfinite(near) and np.isfinite(far)) or far < near:
        raise ValueError("ray_depths: need T >= 1 and finite near <= far, got T = %d, near %r, far %r" % (T, near, far))
    dt = F32(F32(far - near) / F32(T))
    return (near + ((np.arange(T).astype(F32) + F32(.5)).astype(F32) * dt).astype(F32)).astype(F32)


def rays_spec(bits, lo, inv, G, rays_o, rays_d, near, far, T):
    """What r2l_occ_rays writes: (M, idx int64[M] ascending, live uint8[R]).  Stated on compact_spec, as include/r2l_hip.h states
    the call on r2l_occ_index: with z[r, j] = ray_depths(near, far, T)[j] for all rays, ray r is live iff compact_spec lists any
    sample n in [r*T, (r+1)*T)."""
    o, d = (np.asarray(t, dtype=F32).reshape(-1, 3) for t in (rays_o, rays_d))
    R, T = o.shape[0], int(T)
    z = np.broadcast_to(ray_depths(near, far, T)[None, :], (R, T))
    live = np.zeros(R, dtype=np.uint8)
    for a in range(0, R, 65536):  # (slabs of rays: z[R,T] points are the spec's memory, not the kernel's)
        b = min(a + 65536, R)
        _, n, *_ = compact_spec(bits, lo, inv, G, o[a:b], d[a:b], o[a:b], z[a:b])
        live[a + np.unique(n // T)] = 1
    idx = np.flatnonzero(live).astype(np.int64)
    return int(idx.size), idx, live


def frame_d_max(H, W, focal):
    """The largest |rays_d| of an H x W pinhole frame (r2l_frame_rays: d = R (x, y, -1), R a rotation), a little above it:
    sqrt(1 + (W/(2 f))^2 + (H/(2 f))^2).  focal: the SMALLEST focal in use (under use_rand_focal the scene's: the draws scale it
    up)."""
    f = float(focal)
    if not f > 0:
        raise ValueError("frame_d_max: need focal > 0, got %r" % (focal,))
    return float(np.sqrt(1. + (W / (2. * f))**2 + (H / (2. * f))**2))


def cull_steps(grid, near, far, d_max):
    """The smallest T with (far - near) / T * d_max <= the smallest cell side of `grid` (an OccupancyGrid), at least 1: with it
    and a grid dilated by at least one cell, every point of a dead ray's segment [near, far] lies within half a cell of a sample
    that is inside the box and in a clear cell — so the point's own cell was clear BEFORE the dilation, or the point is at most half
    a cell outside the box (include/r2l_hip.h r2l_occ_rays).  Refuses a grid built with dilate < 1: the argument needs the ring."""
    if grid.dilate < 1:
        raise ValueError("cull_steps: the ray rule needs a grid dilated by at least one cell (dilate >= 1), this one has dilate = %d"
                         % grid.dilate)
    near, far, d_max = float(near), float(far), float(d_max)
    if not (np.isfinite(near) and np.isfinite(far) and far >= near and np.isfinite(d_max) and d_max > 0):
        raise ValueError("cull_steps: need finite near <= far and d_max > 0, got near %r, far %r, d_max %r" % (near, far, d_max))
    side = float(((grid.hi.astype(np.float64) - grid.lo.astype(np.float64)) / grid.G).min())
    span = (far - near) * d_max
    T = max(int(np.ceil(span / side)), 1)
    while T > 1 and span / (T - 1) <= side:  # (the quotient's rounding: settle on the definition)
        T -= 1
    while span / T > side:
        T += 1
    if T >= 2**31:
        raise ValueError("cull_steps: %d steps (cells far smaller than the segment)" % T)
    return T


def scatter_spec(raw_live, idx, R, S):
    """What r2l_occ_scatter writes: float32[R,S,4], zero but for raw_out[idx[i]] = raw_live[i]."""
    out = np.zeros((int(R) * int(S), 4), dtype=F32)
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    if idx.size:
        out[idx] = np.asarray(raw_live, dtype=F32).reshape(-1, 4)
    return out.reshape(int(R), int(S), 4)


# ---------------------------------------------------------------------------------------------------------------
# the grid object
# ---------------------------------------------------------------------------------------------------------------
class OccupancyGrid:
    """One bit per cell of the box [lo, hi): G^3 cells, k probes per cell and axis, `dilate` cells of dilation.
    build(net) fills it from a NeRF module (through teacher_engine(net) on the GPU: the engine's precision); render_rays takes a
    pair of built grids as occupancy=(grid_for_network_fn, grid_for_network_fine).  live_points / total_points count what the
    renders since reset_counters() sent to the network and what they would have sent without the grid."""

    def __init__(self, lo, hi, G=128, k=2, dilate=1, sigma_thresh=0.0, precision=None):
        self.G, self.k, self.dilate, self.sigma_thresh = int(G), int(k), int(dilate), float(sigma_thresh)
        self.precision = precision  # None: the engine's kernel family; else that of _lib.PRECISION (the training grids: fp32_mfma)
        if self.dilate < 0:
            raise ValueError("occupancy grid: dilate must be >= 0")
        self.lo, self.inv, self.step = grid_fields(lo, hi, G, k)
        self.hi = np.asarray(hi, dtype=F32).reshape(3)
        self.bits = None  # int32 tensor [n_words(G)] (the uint32 words) on the device of the net it was built from
        self.sigma = None  # build(keep_sigma=True): the probe sigma the bits were made from, probe order
        self.build_seconds = None
        self._desc = None
        self._buf = {}
        self.reset_counters()

    def reset_counters(self):
        self.live_points, self.total_points = 0, 0

    # -- bits -------------------------------------------------------------------------------------------------
    def set_bits(self, words, device="cpu"):
        """Take uint32 words (numpy) as the grid's bits (tests, tools)."""
        w = np.ascontiguousarray(np.asarray(words).astype(np.uint32).reshape(-1))
        if w.size != n_words(self.G):
            raise ValueError("occupancy grid: %d words given, G = %d has %d" % (w.size, self.G, n_words(self.G)))
        self.bits = torch.from_numpy(w.view(np.int32).copy()).to(device)
        self._desc = None
        return self

    def words(self):
        """The bits as uint32 numpy words."""
        self._need_built()
        return self.bits.cpu().numpy().view(np.uint32)

    def occupied_share(self):
        """Share of the G^3 cells whose bit is set."""
        return float(unpack_bits(self.words(), self.G).mean())

    def _need_built(self):
        if self.bits is None:
            raise RuntimeError("occupancy grid: build() it first")

    def desc(self):
        """The r2l_occ_grid of this grid's device bits (r2l_occ_grid_init; its fields must be grid_fields')."""
        self._need_built()
        if self._desc is None:
            d = _lib.OccGridDesc()
            lo, hi = (ctypes.c_float * 3)(*self.lo.tolist()), (ctypes.c_float * 3)(*self.hi.tolist())
            _lib.check(_lib.load().r2l_occ_grid_init(ctypes.byref(d), _ptr(self.bits), self.G, self.k, lo, hi), "r2l_occ_grid_init")
            got = (np.array(d.lo, dtype=F32), np.array(d.inv, dtype=F32), np.array(d.step, dtype=F32))
            if not all(np.array_equal(a, b) for a, b in zip(got, (self.lo, self.inv, self.step))):
                raise RuntimeError("occupancy grid: r2l_occ_grid_init and grid_fields disagree: %s vs %s" % (got, (self.lo, self.inv, self.step)))
            self._desc = d
        return self._desc

    def _cfg(self, eng):
        """The r2l_config of this grid's r2l_occ_build: the engine's, or the grid's own precision."""
        from . import engine as _engine
        return _lib.make_config(precision=self.precision) if self.precision else _engine.merged_config(eng.cfg)

    # -- build ------------------------------------------------------------------------------------------------
    def build(self, net, keep_sigma=False):
        """Fill the bits from `net` (a NeRF module).  GPU parameters: r2l_occ_build through teacher_engine(net) — its packed
        weights and its r2l_config.  CPU parameters: the module's own forward on the probes, then build_spec."""
        from . import engine as _engine
        from .render import Embedder, teacher_engine
        dev = next(net.parameters()).device
        t0 = time.time()
        n_probe = (self.G * self.k)**3
        if dev.type == "cuda":
            eng = teacher_engine(net)
            lib = _lib.load()
            with torch.cuda.device(dev):
                eng.ensure_packed()
                self.bits = torch.zeros(n_words(self.G), dtype=torch.int32, device=dev)
                self._desc = None
                work = torch.empty(lib.r2l_occ_build_work_floats(self.G, self.k), dtype=torch.float32, device=dev)
                sig = torch.empty(n_probe, dtype=torch.float32, device=dev) if keep_sigma else None
                _lib.check(lib.r2l_occ_build(ctypes.byref(self.desc()), self.k, self.dilate, self.sigma_thresh, _ptr(eng.wstream),
                                             _ptr(eng.flat), ctypes.byref(self._cfg(eng)), _ptr(work), _ptr(sig),
                                             _stream()), "r2l_occ_build")
                torch.cuda.synchronize(dev)  # (work is released here; the build is timed)
            self.sigma = sig
        else:
            pts = torch.from_numpy(probe_points(self.lo, self.step, self.G, self.k))
            e_x, e_d = Embedder(10).embed, Embedder(4).embed
            view = e_d(torch.tensor([[0., 0., 1.]]))
            with torch.no_grad():
                sig = torch.cat([net(torch.cat([e_x(p), view.expand(p.shape[0], -1)], -1))[:, 3] for p in pts.split(65536)])
            self.set_bits(build_spec(sig.numpy(), self.G, self.k, self.dilate, self.sigma_thresh))
            self.sigma = sig if keep_sigma else None
        self.build_seconds = time.time() - t0
        return self

    def rebuild(self, net):
        """Refill the bits IN PLACE from `net` (the refresh of a grid while its teacher trains): the grid keeps its bits tensor,
        its descriptor and — on the GPU — the work buffer of its first rebuild, so whoever holds the descriptor (a trainer) sees the
        new bits with nothing to re-wire.  Synchronises (the rebuild is timed; it is off the per-step path).  A grid that was
        never built is built."""
        if self.bits is None:
            return self.build(net)
        from . import engine as _engine
        from .render import teacher_engine
        dev = next(net.parameters()).device
        if dev != self.bits.device:
            raise ValueError("occupancy grid: built on %s, the net is on %s" % (self.bits.device, dev))
        t0 = time.time()
        if dev.type == "cuda":
            eng = teacher_engine(net)
            lib = _lib.load()
            with torch.cuda.device(dev):
                eng.ensure_packed()
                work = self._buf.get("build_work")
                if work is None:
                    work = self._buf["build_work"] = torch.empty(lib.r2l_occ_build_work_floats(self.G, self.k), dtype=torch.float32,
                                                                 device=dev)
                _lib.check(lib.r2l_occ_build(ctypes.byref(self.desc()), self.k, self.dilate, self.sigma_thresh, _ptr(eng.wstream),
                                             _ptr(eng.flat), ctypes.byref(self._cfg(eng)), _ptr(work), None, _stream()),
                           "r2l_occ_build")
                torch.cuda.synchronize(dev)
        else:
            bits, desc = self.bits, self._desc
            self.build(net)  # (makes a new tensor) ...
            bits.copy_(self.bits)  # ... whose words go into the old one
            self.bits, self._desc = bits, desc
        self.sigma = None
        self.build_seconds = time.time() - t0
        return self

    # -- the masked point-network query of render_rays ------------------------------------------------------------
    def _buffers(self, n, dev):
        key = (dev.type, dev.index)
        b = self._buf.get(key)
        if b is None or b["n"] < n:
            f = dict(dtype=torch.float32, device=dev)
            b = self._buf[key] = dict(n=n, o=torch.empty(n, 3, **f), d=torch.empty(n, 3, **f), v=torch.empty(n, 3, **f),
                                      z=torch.empty(n, **f), idx=torch.empty(n, dtype=torch.int64, device=dev),
                                      count=torch.empty(1, dtype=torch.int64, device=dev),
                                      work=torch.empty(max(_lib.load().r2l_occ_compact_work_bytes(n), 16), dtype=torch.uint8, device=dev))
        return b

    def compact(self, rays_o, rays_d, viewdirs, z):
        """(M, idx[M], o[M,3], d[M,3], v[M,3], z[M]) of the live samples, GPU tensors (r2l_occ_compact; reads M: synchronises).
        The returned tensors are views of buffers the grid re-uses on the next call."""
        R, S = z.shape
        b = self._buffers(max(R * S, 1), z.device)
        with torch.cuda.device(z.device):
            _lib.check(_lib.load().r2l_occ_compact(ctypes.byref(self.desc()), _ptr(rays_o.contiguous()), _ptr(rays_d.contiguous()),
                                                   _ptr(viewdirs.contiguous()), _ptr(z.contiguous()), R, S, _ptr(b["o"]), _ptr(b["d"]),
                                                   _ptr(b["v"]), _ptr(b["z"]), _ptr(b["idx"]), _ptr(b["count"]), _ptr(b["work"]),
                                                   _stream()), "r2l_occ_compact")
        M = int(b["count"].item())  # the 8-byte device-to-host copy: the one synchronisation of the masked query
        return M, b["idx"][:M], b["o"][:M], b["d"][:M], b["v"][:M], b["z"][:M]

    def index(self, rays_o, rays_d, z, live_acc=None):
        """(idx, count): the live samples' numbers, ascending, in an int64 tensor of capacity R*S (entries at and past the count are
        not written) and their count as an int64[1] device tensor — r2l_occ_compact's idx and count without its row copies
        (r2l_occ_index), and WITHOUT a read on the host: what TeacherEngine.mlp_live takes.  live_acc: None or an int64[2] device
        tensor that receives += (count, R*S) in stream order (r2l_occ_live_add).  The returned tensors are views of buffers the
        grid re-uses on the next call."""
        R, S = z.shape
        b = self._buffers(max(R * S, 1), z.device)
        lib = _lib.load()
        with torch.cuda.device(z.device):
            _lib.check(lib.r2l_occ_index(ctypes.byref(self.desc()), _ptr(rays_o.contiguous()), _ptr(rays_d.contiguous()),
                                         _ptr(z.contiguous()), R, S, _ptr(b["idx"]), _ptr(b["count"]), _ptr(b["work"]), _stream()),
                       "r2l_occ_index")
            if live_acc is not None:
                _lib.check(lib.r2l_occ_live_add(_ptr(b["count"]), R * S, _ptr(live_acc), _stream()), "r2l_occ_live_add")
        return b["idx"][:max(R * S, 1)], b["count"]

    def rays(self, rays_o, rays_d, near, far, T):
        """(idx, count, live): the numbers of the rays that meet an occupied cell at any of their T depths (r2l_occ_rays), ascending,
        in an int64 tensor of capacity R (entries at and past the count are not written), their count as an int64[1] device tensor —
        nothing is read on the host — and a uint8[R] flag per ray.  The returned tensors are views of buffers the grid re-uses on
        the next call."""
        self._need_built()
        R, dev = int(rays_o.shape[0]), rays_o.device
        if self.bits.device != dev:
            raise ValueError("occupancy grid: built on %s, the rays are on %s" % (self.bits.device, dev))
        key = ("rays", dev.type, dev.index)
        b = self._buf.get(key)
        lib = _lib.load()
        if b is None or b["n"] < R:
            n = max(R, 1)
            b = self._buf[key] = dict(n=n, idx=torch.empty(n, dtype=torch.int64, device=dev),
                                      count=torch.empty(1, dtype=torch.int64, device=dev),
                                      live=torch.empty(n, dtype=torch.uint8, device=dev),
                                      work=torch.empty(max(lib.r2l_occ_rays_work_bytes(n), 16), dtype=torch.uint8, device=dev))
        rays_o, rays_d = rays_o.contiguous(), rays_d.contiguous()  # (named: a copy must live until the launch is enqueued)
        with torch.cuda.device(dev):
            _lib.check(lib.r2l_occ_rays(ctypes.byref(self.desc()), _ptr(rays_o), _ptr(rays_d), R, float(near),
                                        float(far), int(T), _ptr(b["idx"]), _ptr(b["count"]), _ptr(b["live"]), _ptr(b["work"]),
                                        _stream()), "r2l_occ_rays")
        return b["idx"][:max(R, 1)], b["count"], b["live"][:R]

    @staticmethod
    def scatter(raw_live, idx, R, S):
        """raw[R,S,4] on the GPU: zeros, raw[idx[i]] = raw_live[i] (r2l_occ_scatter)."""
        dev = idx.device
        raw = torch.empty(R, S, 4, dtype=torch.float32, device=dev)
        M = int(idx.shape[0])
        with torch.cuda.device(dev):
            _lib.check(_lib.load().r2l_occ_scatter(_ptr(raw_live.contiguous()) if M else None, _ptr(idx) if M else None, M, _ptr(raw),
                                                   R, S, _stream()), "r2l_occ_scatter")
        return raw

    def query(self, net, rays_o, rays_d, viewdirs, z, network_query_fn=None):
        """raw[R,S,4] of the samples o + d*z with the samples that are not live left at zero.  GPU tensors: compact ->
        teacher_engine(net).mlp on the M live rows (S = 1; nothing is launched for M == 0) -> scatter.  CPU tensors: compact_spec,
        the live rows of network_query_fn(pts, viewdirs, net), scatter_spec."""
        from .render import teacher_engine
        self._need_built()
        R, S = z.shape
        if z.is_cuda:
            if self.bits.device != z.device:
                raise ValueError("occupancy grid: built on %s, the rays are on %s" % (self.bits.device, z.device))
            M, idx, o, d, v, zl = self.compact(rays_o, rays_d, viewdirs, z)
            raw_live = teacher_engine(net).mlp(o, d, v, zl.reshape(M, 1)) if M > 0 else None
            raw = self.scatter(raw_live, idx, R, S)
        else:
            M, idx, o, d, v, zl = compact_spec(self.words(), self.lo, self.inv, self.G, rays_o.numpy(), rays_d.numpy(),
                                               viewdirs.numpy(), z.numpy())
            raw_live = np.zeros((0, 4), dtype=F32)
            if M > 0:
                # A CPU BLAS gives a row other bits in another batch, the HIP kernels do not (a point is a column of its tile):
                # here the network runs on every sample and the live rows are taken from that, which is what the GPU path
                # computes; the CPU path is plumbing, nothing is saved on it
                pts = torch.from_numpy(sample_points(rays_o.numpy(), rays_d.numpy(), z.numpy()))
                with torch.no_grad():
                    raw_live = network_query_fn(pts, viewdirs, net).reshape(R * S, -1)[:, :4].numpy()[idx]
            raw = torch.from_numpy(scatter_spec(raw_live, idx, R, S))
        self.live_points += M
        self.total_points += R * S
        return raw


def miss_report(ray_batch, network_fn, network_fine, occupancy, N_samples, N_importance, white_bkgd=False):
    """What a pair of grids costs on given rays (GPU, perturb = 0): the full render next to the skipped one, and per ray the
    samples of the FULL render that the grids skip although their sigma is positive ("misses").  ray_batch [R,11] as render()
    packs it.  Returns a dict of CPU tensors:
      full / skip     {'rgb', 'acc', 'depth'} of render_rays without / with occupancy=
      misses [R]      skipped samples with sigma > 0, both passes (fine pass: at the full render's depths)
      lost [R] fp64   1 - prod over the ray's misses of (1 - alpha_s), alpha_s = 1 - exp(-sigma_s dist_s |d|) in fp64 from the
                      full render's raw: the weight the misses can carry, and as much transmittance is freed behind them —
                      |rgb_skip - rgb_full| <= 2 lost while the fine depths agree (a miss of the coarse pass also moves the fine
                      depths: then the fine misses counted here are those of the full render's depths)
    A ray without a miss renders bit for bit as without the grids."""
    from .render import _coarse_z, raw2outputs, render_rays, sample_pdf_sort, teacher_engine
    o, d, vd = ray_batch[:, 0:3].contiguous(), ray_batch[:, 3:6].contiguous(), ray_batch[:, 8:11].contiguous()
    near, far = ray_batch[:, 6:7].contiguous(), ray_batch[:, 7:8].contiguous()
    fine_net = network_fn if network_fine is None else network_fine
    kw = dict(network_fn=network_fn, network_query_fn=None, N_samples=N_samples, N_importance=N_importance, network_fine=network_fine,
              white_bkgd=white_bkgd, perturb=0.)
    out = {}
    with torch.no_grad():
        for name, occ in (("full", None), ("skip", occupancy)):
            r = render_rays(ray_batch, occupancy=occ, **kw)
            out[name] = {"rgb": r["rgb_map"].cpu(), "acc": r["acc_map"].cpu(), "depth": r["depth_map"].cpu()}
        z = _coarse_z(near, far, N_samples, False, 0., False)
        passes = [(occupancy[0], network_fn, z)]
        if N_importance > 0:
            raw0 = teacher_engine(network_fn).mlp(o, d, vd, z)
            w0 = raw2outputs(raw0, z, d, 0, white_bkgd)[3]
            passes.append((occupancy[1], fine_net, sample_pdf_sort(z, w0, N_importance, det=True)[1]))
        R = z.shape[0]
        misses, keep = torch.zeros(R, dtype=torch.int64), torch.ones(R, dtype=torch.float64)
        norm = d.double().norm(dim=-1, keepdim=True).cpu()
        for grid, net, zz in passes:
            sigma = teacher_engine(net).mlp(o, d, vd, zz)[..., 3].double().cpu()
            zc = zz.cpu()
            live = live_spec(grid.words(), grid.lo, grid.inv, grid.G, sample_points(o.cpu().numpy(), d.cpu().numpy(), zc.numpy()).reshape(-1, 3))
            miss = ~torch.from_numpy(live).reshape(zc.shape) & (sigma > 0)
            dist = torch.cat([zc[:, 1:] - zc[:, :-1], torch.full_like(zc[:, :1], 1e10)], -1).double() * norm
            alpha = 1. - torch.exp(-torch.relu(sigma) * dist)
            misses += miss.sum(-1)
            keep *= torch.where(miss, 1. - alpha, torch.ones_like(alpha)).prod(-1)
    out.update(misses=misses, lost=1. - keep)
    return out


# ---------------------------------------------------------------------------------------------------------------
# drivers (--r2l_occupancy, --r2l_occ_fused)
# ---------------------------------------------------------------------------------------------------------------
def box_half_side(args, near, far):
    """--r2l_occ_bound, or 0.625 (far - near): 2.5 for the Blender scenes (near 2, far 6), whose objects sit inside [-1.5, 1.5]^3."""
    return float(args.r2l_occ_bound) if args.r2l_occ_bound > 0 else 0.625 * (float(far) - float(near))


def build_pair(args, coarse, fine, near, far, logger):
    """The (coarse, fine) grids of a driver run, built once after the teacher is loaded; logs the build time and the occupied
    share.  fine None (N_importance == 0 in main.py's teacher): the coarse net serves both passes, and so does its grid."""
    b = box_half_side(args, near, far)
    grids = []
    for name, net in (("coarse", coarse), ("fine", fine)):
        if net is None:
            grids.append(grids[0])
            continue
        g = OccupancyGrid([-b] * 3, [b] * 3, G=args.r2l_occ_res).build(net)
        logger.info("occupancy grid (%s net): %d^3 cells over +-%.3g, %d probes per cell and axis, dilation %d: built in %.2fs, "
                    "%.1f%% of the cells occupied" % (name, g.G, b, g.k, g.dilate, g.build_seconds, 100. * g.occupied_share()))
        grids.append(g)
    return tuple(grids)


def fused_skipping(args):
    """Whether a run skips samples inside the fused frames call: --r2l_occ_fused (grids), --r2l_ert (early termination), or both."""
    return bool(args.r2l_occ_fused) or args.r2l_ert > 0


class FusedOccupancy:
    """What a run skips inside the fused frames call: the grids of --r2l_occ_fused (the pair build_pair makes), the early
    termination of --r2l_ert EPS / --r2l_ert_seg W (r2l_amd/ert.py), or both, and the device counters the frames calls add their live
    and total samples to (render_frames(occupancy=, ert=, live_acc=)).  Nothing is read per frame: log() reads the two counters
    once, when the run's frames are done."""

    def __init__(self, args, coarse, fine, near, far, logger):
        self.pair = build_pair(args, coarse, fine, near, far, logger) if args.r2l_occ_fused else None
        self.bound = box_half_side(args, near, far)
        self.ert = (float(args.r2l_ert), int(args.r2l_ert_seg)) if args.r2l_ert > 0 else None
        self.live_acc = torch.zeros(2, dtype=torch.int64, device=next(coarse.parameters()).device)

    def kwargs(self):
        return {"live_acc": self.live_acc, **({"occupancy": self.pair} if self.pair is not None else {}),
                **({"ert": self.ert} if self.ert is not None else {})}

    def provenance(self):
        """The entries a store file's provenance gains: 'occupancy' with the grids, 'ert' with early termination."""
        out = {}
        if self.pair is not None:
            g = self.pair[0]
            out["occupancy"] = {"res": g.G, "bound": self.bound, "k": g.k, "dilate": g.dilate}
        if self.ert is not None:
            out["ert"] = {"eps": self.ert[0], "seg": self.ert[1]}
        return out

    def log(self, logger):
        a, b = (int(x) for x in self.live_acc.tolist())  # the one read of the run
        if self.ert is not None:  # (the one line of such a run; without grids b counts the last pass alone)
            logger.info("early termination: eps %g, seg %d, live points %d / %d (%.1f%%)" % (self.ert[0], self.ert[1], a, b, 100. * a / max(b, 1)))
        else:
            logger.info("occupancy grid: live points %d / %d (%.1f%%)" % (a, b, 100. * a / max(b, 1)))
        return a, b


def log_live(pair, logger):
    """'live points a / b' of the renders of a run (both grids)."""
    seen = {id(g): g for g in pair}.values()
    a, b = sum(g.live_points for g in seen), sum(g.total_points for g in seen)
    logger.info("occupancy grid: live points %d / %d (%.1f%%)" % (a, b, 100. * a / max(b, 1)))
    return a, b


def popcount_words(w):
    """Number of set bits of an int32 word tensor (plain torch ops; the arithmetic shift's sign copies fall to the & 1)."""
    return int(sum(((w >> s) & 1).sum() for s in range(32)))


class TrainOccupancy:
    """The grids of a teacher-training run with --r2l_occ_train (utils/train_nerf.py): one per net, built with sigma threshold 0 and
    one cell of dilation by the exact-fp32 kernels — the trainer's family —, handed to TeacherTrainer.set_occupancy and refreshed IN
    PLACE every --r2l_occ_every iterations.  The grids in force in iteration i are built from the weights as they stand after
    iteration options.occ_refresh_base(i, K); a checkpoint of iteration i carries the grids in force in iteration i + 1 (state(),
    under KEY), so that --resume repeats the uninterrupted run.  The trainer's device counters are read at each refresh only."""
    KEY = "r2l_occ_train"

    def __init__(self, args, coarse, fine, near, far, trainer, logger, start=0, state=None):
        from .options import occ_refresh_base
        self.K, self.bound, self.trainer, self.logger = int(args.r2l_occ_every), box_half_side(args, near, far), trainer, logger
        self.nets = [coarse] + ([fine] if fine is not None and len(trainer.nets) > 1 else [])
        b = self.bound
        self.grids = [OccupancyGrid([-b] * 3, [b] * 3, G=args.r2l_occ_res, k=2, dilate=1, sigma_thresh=0., precision="fp32_mfma")
                      for _ in self.nets]
        self.base = occ_refresh_base(start + 1, self.K)
        dev = next(coarse.parameters()).device
        why = self._mismatch(state)
        if why is None:
            for g, w in zip(self.grids, state["words"]):
                g.set_bits(w.cpu().numpy().view(np.uint32), device=dev)
            logger.info("occupancy grids of the training step: restored from the checkpoint (built from the weights after iteration "
                        "%d; %d^3 cells over +-%.3g, refreshed every %d iterations)" % (self.base, self.grids[0].G, b, self.K))
        else:
            if start > 0:
                logger.info("occupancy grids of the training step: %s — rebuilt at once from the checkpoint's weights (iteration %d), "
                            "where the uninterrupted run's were built after iteration %d" % (why, start, self.base))
                self.base = start
            for name, g, net in zip(("coarse", "fine"), self.grids, self.nets):
                g.build(net)
                logger.info("occupancy grid of the training step (%s net): %d^3 cells over +-%.3g, %d probes per cell and axis, "
                            "dilation %d, exact fp32: built in %.3fs, %.1f%% of the cells occupied; refreshed every %d iterations"
                            % (name, g.G, b, g.k, g.dilate, g.build_seconds, 100. * g.occupied_share(), self.K))
        trainer.set_occupancy(self.pair())
        if trainer.live_acc is not None:
            trainer.live_acc.zero_()

    def pair(self):
        return (self.grids[0], self.grids[-1])

    def _mismatch(self, state):
        """Why a checkpoint's grids cannot serve this run, or None."""
        if state is None:
            return "the checkpoint has no key %r" % self.KEY
        g = self.grids[0]
        want = {"res": g.G, "bound": self.bound, "k": g.k, "dilate": g.dilate, "every": self.K, "base": self.base, "n": len(self.grids)}
        for k, v in want.items():
            if state.get(k) != v:
                return "the checkpoint's grids have %s = %r, this run %r" % (k, state.get(k), v)
        return None

    def state(self):
        """The checkpoint entry: the fields the grids were made with, the iteration whose weights they were built from, the words."""
        g = self.grids[0]
        return {"res": g.G, "bound": self.bound, "k": g.k, "dilate": g.dilate, "every": self.K, "base": self.base, "n": len(self.grids),
                "words": [x.bits.detach().cpu().clone() for x in self.grids]}

    def after_step(self, i):
        """Called when iteration i is done: refresh when the next iteration begins a window."""
        if i % self.K == 0:
            self.refresh(i)

    def refresh(self, i):
        a, b = (int(x) for x in self.trainer.live_acc.tolist())  # the one read of the window's counters
        self.trainer.live_acc.zero_()
        secs, share, new = [], [], 0
        for g, net in zip(self.grids, self.nets):
            old = g.bits.clone()
            g.rebuild(net)
            new += popcount_words(g.bits & ~old)
            secs.append(g.build_seconds)
            share.append(100. * g.occupied_share())
        self.base = i
        self.logger.info("occupancy grid refresh after iteration %d: built in %s s, %s %% of the cells occupied, live points %d / %d "
                         "(%.1f%%) in the window, %d cells set now that were clear in the outgoing grids"
                         % (i, " + ".join("%.3f" % s for s in secs), " / ".join("%.1f" % s for s in share), a, b,
                            100. * a / max(b, 1), new))
        return a, b, new
