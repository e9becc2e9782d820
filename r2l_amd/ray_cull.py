"""Whole rays that see only empty space are left out (--r2l_ray_cull; include/r2l_hip.h r2l_occ_rays).

A light-field student cannot skip samples: it pays its whole network for a ray whose colour is the background exactly.  The
occupancy grid of the teacher that made the final colour knows those rays — a ray none of whose T points o + d t_j falls into an
occupied cell or outside the box is DEAD (occupancy.rays_spec, occupancy.cull_steps for T and why that T is enough) — and two
consumers use the answer:

  the student's render (RayCull.render_poses, driver.render_path), per launch group of frames:
      r2l_frame_rays -> r2l_occ_rays -> read M (8 bytes, the one synchronisation) -> r2l_rays_gather -> r2l_forward_rays_cfg
      (t_rand = NULL) on the M live rays in the engine's family -> r2l_rgb_scatter_bg: dead pixels get the background colour
      exactly (1.0 with white_bkgd, else 0.0), live pixels their row.  M == 0 launches no forward.  The chain kernels and
      r2l_forward_poses_cfg are not touched;
  the fill of the ray store (online_kd.TeacherFill.fill_group), per flush group:
      render_frames -> r2l_occ_rays on the WORLD o, d of the rows -> read M -> RayStore.append_live (r2l_store_append_live).

The grid travels in every checkpoint of a run with the switch (KEY): a later render needs no teacher.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import ptr as _ptr, stream as _stream
from .occupancy import OccupancyGrid, cull_steps, frame_d_max

KEY = "r2l_ray_cull"
STATE_FIELDS = ("bits", "G", "lo", "hi", "k", "dilate", "near", "far", "white_bkgd")


class RayCull:
    """One built, dilated OccupancyGrid, the segment [near, far] of the scene's rays and the background colour."""

    def __init__(self, grid, near, far, white_bkgd):
        self.grid, self.near, self.far, self.white_bkgd = None, float(near), float(far), bool(white_bkgd)
        self.live_rays, self.total_rays = 0, 0  # what the renders / the fill have seen (host counts: M is read anyway)
        self._steps = {}
        if grid is not None:
            self.adopt(grid, white_bkgd)

    @classmethod
    def deferred(cls, near, far):
        """A RayCull whose grid the store fill will hand over (online_kd.TeacherFill builds the teacher's grids anyway: adopt())."""
        return cls(None, near, far, False)

    def adopt(self, grid, white_bkgd):
        if grid.dilate < 1:
            raise ValueError("ray cull: the grid must be dilated by at least one cell (occupancy.cull_steps), got dilate = %d" % grid.dilate)
        grid._need_built()
        self.grid, self.white_bkgd, self._steps = grid, bool(white_bkgd), {}
        return self

    def _need_grid(self):
        if self.grid is None:
            raise RuntimeError("ray cull: the grid has not been handed over yet (it comes with the first group of the store fill)")

    @property
    def bg(self):
        return 1.0 if self.white_bkgd else 0.0

    def steps(self, H, W, focal):
        """T of the rays of H x W frames whose smallest focal is `focal` (occupancy.cull_steps)."""
        self._need_grid()
        key = (int(H), int(W), float(focal))
        if key not in self._steps:
            self._steps[key] = cull_steps(self.grid, self.near, self.far, frame_d_max(H, W, focal))
        return self._steps[key]

    # -- checkpoint entry ------------------------------------------------------------------------------------------------
    def state(self):
        """The checkpoint entry (KEY): the grid's words and what they mean.  CPU tensors and plain numbers only."""
        self._need_grid()
        g = self.grid
        return {"bits": g.bits.detach().cpu().clone(), "G": g.G, "lo": [float(x) for x in g.lo], "hi": [float(x) for x in g.hi],
                "k": g.k, "dilate": g.dilate, "near": self.near, "far": self.far, "white_bkgd": self.white_bkgd}

    @classmethod
    def from_state(cls, state, device="cpu"):
        missing = [f for f in STATE_FIELDS if f not in state]
        if missing:
            raise ValueError("ray cull: the checkpoint entry %r lacks %s" % (KEY, ", ".join(missing)))
        g = OccupancyGrid(state["lo"], state["hi"], G=state["G"], k=state["k"], dilate=state["dilate"])
        g.set_bits(torch.as_tensor(state["bits"]).cpu().numpy().view(np.uint32), device=device)
        return cls(g, state["near"], state["far"], state["white_bkgd"])

    def provenance(self, T):
        """The `ray_cull` entry of a store file's provenance: every field from the grid the rows were culled with."""
        self._need_grid()
        g = self.grid
        return {"res": g.G, "bound": float(g.hi[0]), "dilate": g.dilate, "T": int(T), "near": self.near, "far": self.far}

    def mismatch(self, prov, T=None):
        """What a store file's `ray_cull` provenance says otherwise than this grid: a list of 'field: file x, run y' (empty: none).
        T is compared when given (the T of this run's frames)."""
        mine = self.provenance(0 if T is None else T)
        return ["%s: file %r, run %r" % (k, prov.get(k), v) for k, v in mine.items() if (k != "T" or T is not None) and prov.get(k) != v]

    # -- the rule ----------------------------------------------------------------------------------------------------------
    def live_index(self, rays_o, rays_d, T):
        """(M, idx, live): r2l_occ_rays on device rays, then the ONE 8-byte read of the count.  idx has capacity R, its first M
        entries are the live rays, ascending; live is uint8[R].  Views of buffers the grid re-uses."""
        self._need_grid()
        idx, count, live = self.grid.rays(rays_o, rays_d, self.near, self.far, T)
        M = int(count.item())
        self.live_rays += M
        self.total_rays += int(rays_o.shape[0])
        return M, idx, live

    # -- the student's render ------------------------------------------------------------------------------------------------
    def render_rays(self, eng, rays_o, rays_d, z_vals, T, rgb_live=None):
        """rgb[R,3] of explicit device rays through the engine `eng` (R2LEngine): the live rays through r2l_forward_rays_cfg, the dead
        ones the background.  rgb_live: None, or a float32 buffer of at least [M,3] the forward writes into (tests).  Returns
        (rgb, M, idx, live)."""
        lib, dev = _lib.load(), rays_o.device
        rays_o, rays_d = rays_o.contiguous(), rays_d.contiguous()
        R = int(rays_o.shape[0])
        M, idx, live = self.live_index(rays_o, rays_d, T)
        rgb = torch.empty(R, 3, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            if M > 0:
                o = torch.empty(M, 3, dtype=torch.float32, device=dev)
                d = torch.empty(M, 3, dtype=torch.float32, device=dev)
                _lib.check(lib.r2l_rays_gather(_ptr(rays_o), _ptr(rays_d), R, _ptr(idx), M, _ptr(o), _ptr(d), _stream()),
                           "r2l_rays_gather")
                eng.ensure_packed(M, with_stash=False)
                if rgb_live is None:
                    rgb_live = torch.empty(M, 3, dtype=torch.float32, device=dev)
                elif rgb_live.numel() < 3 * M or rgb_live.dtype != torch.float32 or rgb_live.device != dev or not rgb_live.is_contiguous():
                    raise ValueError("ray cull: rgb_live must be a contiguous fp32 buffer of at least [%d, 3] on %s" % (M, dev))
                _lib.check(lib.r2l_forward_rays_cfg(_ptr(o), _ptr(d), None, _ptr(eng.ztab(z_vals, 0.)), _ptr(eng.wstream),
                                                    _ptr(eng.flat), eng.n_block, _ptr(rgb_live), None, None, M, _stream(), eng._cfg()),
                           "r2l_forward_rays")
            _lib.check(lib.r2l_rgb_scatter_bg(_ptr(rgb_live) if M > 0 else None, _ptr(idx) if M > 0 else None, M, _ptr(live), self.bg,
                                              _ptr(rgb), R, _stream()), "r2l_rgb_scatter_bg")
        return rgb, M, idx, live

    def frame_rays(self, c2ws, H, W, focal, device):
        """(o, d) [K*H*W, 3] of K whole frames (r2l_frame_rays)."""
        c = torch.as_tensor(c2ws, dtype=torch.float32)[:, :3, :4].to(device).contiguous()
        K = int(c.shape[0])
        o = torch.empty(K * H * W, 3, dtype=torch.float32, device=device)
        d = torch.empty(K * H * W, 3, dtype=torch.float32, device=device)
        if K:
            with torch.cuda.device(device):
                _lib.check(_lib.load().r2l_frame_rays(_ptr(c), None, float(focal), K, int(H), int(W), _ptr(o), _ptr(d), None, None,
                                                      _stream()), "r2l_frame_rays")
        return o, d

    def render_poses(self, model, c2ws, point_sampler, rgb_live=None):
        """rgb[K, H*W, 3] for the K frames seen from c2ws: NeRF_v3_2.render_poses with the dead rays left out."""
        ps = point_sampler
        eng = model.engine()
        eng.ensure_packed(1, with_stash=False)  # (flattens: the engine's device is known)
        dev = eng.device
        if self.grid.bits.device != dev:
            raise ValueError("ray cull: the grid is on %s, the student on %s" % (self.grid.bits.device, dev))
        K = int(torch.as_tensor(c2ws).shape[0])
        if K == 0:
            return torch.empty(0, ps.H * ps.W, 3, dtype=torch.float32, device=dev)
        o, d = self.frame_rays(c2ws, ps.H, ps.W, ps.focal, dev)
        rgb = self.render_rays(eng, o, d, ps.z_vals, self.steps(ps.H, ps.W, ps.focal), rgb_live=rgb_live)[0]
        return rgb.view(K, ps.H * ps.W, 3)

    def log(self, logger, what="ray cull"):
        logger.info("%s: live rays %d / %d (%.1f%%)" % (what, self.live_rays, self.total_rays, 100. * self.live_rays / max(self.total_rays, 1)))
        return self.live_rays, self.total_rays


def build_from_teacher(args, near, far, device, logger):
    """The grid of a run whose checkpoint carries none: the teacher named by --teacher_ckpt + --r2l_teacher_config, behind the
    run's arithmetic switch, through occupancy.build_pair — the grid of the net that makes the final colour (fine, or coarse when
    there is no fine net).  The teacher is dropped again."""
    from .create_data import create_teacher
    from .driver import apply_arithmetic
    from .occupancy import build_pair
    from .options import parse_teacher_config
    targs = parse_teacher_config(args.r2l_teacher_config, teacher_ckpt=args.teacher_ckpt)
    targs.r2l_precision = args.r2l_precision
    coarse, fine = create_teacher(targs, device)
    apply_arithmetic(targs, device, logger, teachers=(coarse, fine))
    pair = build_pair(args, coarse, fine, near, far, logger)
    cull = RayCull(pair[1], near, far, targs.white_bkgd)
    for net in (coarse, fine):
        if net is not None:
            net.__dict__.pop("_r2l_teacher_engine", None)
    return cull


def for_run(args, ckpt, near, far, device, logger, fill_builds=False):
    """The RayCull of a main.py run with --r2l_ray_cull: from the checkpoint's entry, else built from the teacher.  fill_builds: the
    run's first student render comes after its store fill (--r2l_online_kd), which builds the teacher's grids anyway: without a
    checkpoint entry the RayCull is then deferred and adopts the fill's grid, so that nothing is loaded or built twice."""
    from .options import validate_ray_cull
    has = ckpt is not None and ckpt.get(KEY) is not None
    validate_ray_cull(args, device.type, ckpt_has_grid=has)
    if has:
        cull = RayCull.from_state(ckpt[KEY], device)
        g = cull.grid
        logger.info("ray cull: grid from the checkpoint (%d^3 cells over [%g, %g], dilation %d, %.1f%% occupied; near %g, far %g, %s "
                    "background)" % (g.G, g.lo[0], g.hi[0], g.dilate, 100. * g.occupied_share(), cull.near, cull.far,
                                     "white" if cull.white_bkgd else "black"))
        return cull
    if fill_builds:
        logger.info("ray cull: the grid is the store fill's (the teacher's fine grid, or the coarse one without a fine net)")
        return RayCull.deferred(near, far)
    cull = build_from_teacher(args, near, far, device, logger)
    logger.info("ray cull: grid built from the teacher %s (%d^3 cells, dilation %d; near %g, far %g, %s background)" %
                (args.teacher_ckpt, cull.grid.G, cull.grid.dilate, cull.near, cull.far, "white" if cull.white_bkgd else "black"))
    return cull
