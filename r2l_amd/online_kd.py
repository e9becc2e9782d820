"""Teacher pseudo data rendered straight into a device-resident RayStore (r2l_amd/raystore.py) — create_data without the files.

fill_store_from_teacher replays create_data.main's fused branch (--r2l_fused_frames) for one rank: the same RandomState stream
(pose, focal scale per pose; the flush seed per group of --create_data_chunk poses), the same render_frames calls (seed =
1000003 * rank, frame_id0 = the pose number, rows=True) per run of consecutive pose numbers — and then appends the group's rows
to the store with key = the flush seed instead of copying them to the host, shuffling and saving them.  The store therefore
holds the rows create_data --r2l_fused_frames would have written for the same arguments, in another order (the device shuffle
is the bijection of csrc/r2l_perm.h, not numpy's permutation).  The frames are a pure function of seed and pose number, so a
re-run (driver --resume) reproduces the store bit for bit."""
import numpy as np
import torch

from . import data as D

RAYS_PER_SHARD = 4096


def check_teacher_args(targs, device=None):
    """The refusals of the fused frames path (create_data.main, driver.render_path)."""
    if targs.lindisp or targs.raw_noise_std or not targs.use_viewdirs:
        raise NotImplementedError("teacher fill of the ray store renders through the fused frames path: lindisp, raw_noise_std > 0 "
                                  "and use_viewdirs=False are outside it (pass --raw_noise_std 0)")
    if device is not None and torch.device(device).type != "cuda":
        raise NotImplementedError("teacher fill of the ray store renders through libr2l_hip.so: it needs a GPU")


def rank_poses(n_pose, rank, world):
    """Pose numbers of a rank, as create_data.main: i % world == rank of 1 .. n_pose."""
    return [i for i in range(1, n_pose + 1) if i % world == rank]


def shards_needed(n_pose, chunk_poses, H, W, rank=0, world=1, rays_per_shard=RAYS_PER_SHARD):
    """Shards the rank's fill writes: every flush group keeps floor(poses * H * W / rays_per_shard) of them."""
    n, chunk = len(rank_poses(n_pose, rank, world)), max(int(chunk_poses), 1)
    return sum((min(chunk, n - a) * H * W) // rays_per_shard for a in range(0, n, chunk))


class _Quiet:
    def info(self, *a):
        pass


class TeacherFill:
    """State of an incremental fill: the rank's pose list, its RandomState, the teacher pair and what is still pending."""

    def __init__(self, store, targs, H, W, focal, near, far, n_pose, chunk_poses, rank, world, device, logger=None,
                 rand_pose=None, ndc=False, occ_args=None, ray_cull=None):
        from .create_data import create_teacher
        from .driver import apply_arithmetic
        check_teacher_args(targs, device)
        self.store, self.targs, self.logger = store, targs, logger
        self.H, self.W, self.focal, self.near, self.far = int(H), int(W), float(focal), float(near), float(far)
        self.rank, self.world, self.device = rank, world, torch.device(device)
        # the scene's pose generator and ray convention (data.load_scene): blender's by default
        self.rand_pose, self.ndc = rand_pose or D.get_rand_pose, bool(ndc)
        self.chunk = max(int(chunk_poses), 1)
        self.mine = rank_poses(int(n_pose), rank, world)
        self.rng = np.random.RandomState(1000003 * rank)  # per-rank pose / focal / shuffle stream, as create_data.main
        self.at = 0  # poses of self.mine rendered so far
        self.groups = 0
        self.append_ms = []  # (event pair) per group: the append's share of a flush group, read by tools/raystore_time.py
        self.n_pose = int(n_pose)
        self.coarse, self.fine = create_teacher(targs, self.device)
        self.r2l_config = None  # the record apply_arithmetic returns (precision of the teacher kernels): provenance()
        if logger is not None:
            self.r2l_config = apply_arithmetic(targs, self.device, logger, teachers=(self.coarse, self.fine))
        # --r2l_occ_fused / --r2l_ert (occ_args: the namespace that carries r2l_occ_res / r2l_occ_bound / r2l_ert / r2l_ert_seg):
        # both grids once, behind the arithmetic switch; the build and the render are deterministic, so a re-run renders the same store
        self.occ = self.occ_prov = None
        if occ_args is not None:
            from .occupancy import FusedOccupancy
            if self.ndc and occ_args.r2l_occ_fused:
                raise ValueError("--r2l_occ_fused puts its box about the origin of a bounded scene: not with an NDC (llff) scene")
            self.occ = FusedOccupancy(occ_args, self.coarse, self.fine, self.near, self.far, _Quiet() if logger is None else logger)
            self.occ_prov = self.occ.provenance()  # (kept: the grids go with the teacher in release())
        # --r2l_ray_cull (ray_cull: a ray_cull.RayCull, or True for one on this fill's own grid — the grid of the net that makes the
        # final colour): the rays of a group that meet no occupied cell are not appended.  T from the SCENE's focal: the smallest in
        # use (use_rand_focal scales it up)
        self.cull = self.cull_T = None
        if ray_cull:
            from .ray_cull import RayCull
            if self.occ is None or self.occ.pair is None:
                raise ValueError("--r2l_ray_cull culls the fill with the grids of --r2l_occ_fused: give that switch too")
            if hasattr(store, "append_frames"):
                raise ValueError("--r2l_ray_cull: not with --r2l_compact_store, whose rows keep a ray's number in its flush group")
            if isinstance(ray_cull, RayCull):  # the run's own (a checkpoint's grid), or deferred: it adopts this fill's grid
                self.cull = ray_cull if ray_cull.grid is not None else ray_cull.adopt(self.occ.pair[1], targs.white_bkgd)
            else:
                self.cull = RayCull(self.occ.pair[1], self.near, self.far, targs.white_bkgd)
            self.cull_T = self.cull.steps(self.H, self.W, self.focal)
            self.cull_live, self.cull_total = 0, 0
            self.occ_prov = {**self.occ_prov, "ray_cull": self.cull.provenance(self.cull_T)}

    @property
    def pending(self):
        return len(self.mine) - self.at

    @property
    def done(self):
        return self.pending == 0

    def _info(self, msg):
        if self.logger is not None:
            self.logger.info(msg)

    def provenance(self):
        """What a store file says about its fill (raystore.RayStore.save): for the log of the run that loads it, nothing is
        derived from it.  No time stamp: equal fills give equal files."""
        import os
        a = self.targs
        return {"teacher_ckpt": a.teacher_ckpt, "N_samples": a.N_samples, "N_importance": a.N_importance, "perturb": a.perturb,
                "white_bkgd": bool(a.white_bkgd), "use_rand_focal": bool(a.use_rand_focal), "n_pose": self.n_pose,
                "create_data_chunk": self.chunk, "near": self.near, "far": self.far, "ndc": self.ndc, "focal": self.focal,
                "precision": (self.r2l_config or {}).get("precision", a.r2l_precision), "R2L_SEED": os.environ.get("R2L_SEED", "0"),
                **(self.occ_prov or {})}

    def fill_group(self):
        """Render the next flush group into the store; returns the number of shards it added."""
        from .driver import _runs
        from .render import render_frames
        if self.done:
            return 0
        a = self.targs
        group = []
        for i in self.mine[self.at:self.at + self.chunk]:
            pose = self.rand_pose(self.rng)
            focal_ = self.focal * (1 + self.rng.rand()) if a.use_rand_focal else self.focal  # focal x U[1,2) (create_data.py:816)
            group.append((i, pose[:3, :4], focal_))
        ids = [g[0] for g in group]
        c2ws = torch.stack([g[1] for g in group], 0).to(self.device)
        focals = torch.tensor([g[2] for g in group], dtype=torch.float32, device=self.device)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        # a compact store (raystore.CompactRayStore) takes rgb and the poses: the 24 bytes of o, d per ray are never written
        compact = hasattr(self.store, "append_frames")
        occ_kw = self.occ.kwargs() if self.occ is not None else {}
        with torch.no_grad():
            parts = [render_frames(c2ws[s:s + n], self.H, self.W, focals[s:s + n], self.near, self.far, self.coarse, self.fine,
                                   a.N_samples, a.N_importance, a.perturb, a.white_bkgd, seed=1000003 * self.rank,
                                   frame_id0=ids[s], rows=not compact, ndc=self.ndc, ndc_focal=self.focal,
                                   **occ_kw)["rgb" if compact else "rows"] for s, n in _runs(ids)]
        rows = parts[0] if len(parts) == 1 else torch.cat(parts, 0)
        key = int(self.rng.randint(0, 2**31 - 1))  # the flush seed: drawn where create_data.main's flush() draws it
        e[1].record()
        if self.cull is not None:
            # r2l_occ_rays on the group's WORLD o, d; ONE 8-byte read of the count per flush group; r2l_store_append_live
            M, idx, _ = self.cull.live_index(rows[:, 0:3], rows[:, 3:6], self.cull_T)
            self.cull_live += M
            self.cull_total += int(rows.shape[0])
            self._info("ray cull: live rays %d / %d (%.1f%%) of the flush group" % (M, rows.shape[0], 100. * M / max(rows.shape[0], 1)))
            m = self.store.append_live(rows, idx, M, key, shuffle=True)
        else:
            m = self.store.append_frames(rows, c2ws, focals, key, shuffle=True) if compact else self.store.append(rows, key, shuffle=True)
        e[2].record()
        self.append_ms.append(e)
        self.at += len(group)
        self.groups += 1
        self._info("[%d/%d poses on rank %d] teacher rendered into the ray store: %s" %
                   (self.at, len(self.mine), self.rank, self.store.describe()))
        if self.done:
            self.release()
        return m

    def release(self):
        """Drop the teacher: its engines (flat parameters, packed streams), the frames' work buffer and the modules."""
        if self.coarse is None:
            return
        if self.occ is not None:  # the live share of the whole fill: the one read of the counters
            if self.logger is not None:
                self.occ.log(self.logger)
            self.occ = None
        if self.cull is not None:
            self._info("ray cull: live rays %d / %d (%.1f%%) of the whole fill" %
                       (self.cull_live, self.cull_total, 100. * self.cull_live / max(self.cull_total, 1)))
        freed = 0
        for net in (self.coarse, self.fine):
            eng = net.__dict__.pop("_r2l_teacher_engine", None)
            if eng is not None:
                for t in (getattr(eng, "_frames_work", None), getattr(eng, "wstream", None), eng.flat):
                    freed += t.numel() * 4 if t is not None else 0
        self.coarse = self.fine = None
        torch.cuda.empty_cache()
        self._info("ray store complete (%s): teacher engines and work buffers released (%.1f MB)" %
                   (self.store.describe(), freed / 1e6))


def fill_store_from_teacher(store, targs, H, W, focal, near, far, n_pose, chunk_poses, rank, world, device, logger=None,
                            state=None, groups=None):
    """Render this rank's poses (i % world == rank of 1 .. n_pose) into `store`, a flush group of `chunk_poses` poses at a time.
    targs: the TEACHER's namespace (options.parse_args of its config: N_samples, N_importance, perturb, white_bkgd,
    use_rand_focal, teacher_ckpt, ...).  groups=None renders everything that is pending, groups=g at most g flush groups; pass
    the returned TeacherFill back as `state` to continue (state.pending = poses still to render).  When the last group is in, the
    teacher's engines and work buffers are released."""
    if state is None:
        state = TeacherFill(store, targs, H, W, focal, near, far, n_pose, chunk_poses, rank, world, device, logger)
    n = 0
    while not state.done and (groups is None or n < groups):
        state.fill_group()
        n += 1
    if state.done:
        state.release()  # (a rank without poses never entered fill_group)
    return state
