"""R2L driver: the `python main.py --model_name R2L ...` surface (render_only / render_test / --benchmark / distillation
training with hard-ray mining / checkpoints), mirroring the control flow of the reference's main.py:888-1542 for the
accelerated path only.  One process per GPU; under torchrun the ray shards, test frames and log output are
rank-partitioned and the only collective is the flat-gradient all-reduce inside R2LTrainer.
"""
import ctypes
import json
import math
import os
import time

import numpy as np
import torch
import torch.distributed as dist

from . import data as D
from .checkpoint import load_ckpt, load_weights_v2, parse_expid_iter, save_ckpt
from .logger import Logger
from .metrics import flip, img2mse, lpips, lpips_vgg, mse2psnr, ssim, to8b
from .nerf_raybased import NeRF_v3_2, PointSampler, PositionalEmbedder
from .options import (parse_args, validate_accelerated, validate_compact_store, validate_fused_iter, validate_image_store,
                      validate_ert, validate_occ_fused, validate_occupancy, validate_ray_cull, validate_store_file)
from .dist_utils import split_shards
from .train_step import N_SAMPLE, R2LTrainer, lr_schedule


# ---------------------------------------------------------------------------------------------------------------
def init_distributed():
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if torch.cuda.is_available():
        torch.cuda.set_device(local % torch.cuda.device_count())
        device = torch.device("cuda", local % torch.cuda.device_count())
    else:
        device = torch.device("cpu")
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        # (R2L_DIST_BACKEND=gloo: two ranks on ONE GPU in tests — RCCL refuses a device twice, gloo moves CUDA tensors through the host)
        dist.init_process_group(os.environ.get("R2L_DIST_BACKEND") or ("nccl" if device.type == "cuda" else "gloo"))
    return rank, world, device


def sync(device):
    if device.type == "cuda":
        torch.cuda.synchronize()


class HardRayPool:
    """Hard-example pool of main.py:1164-1165, 1325-1347, 1410-1425: after each step the hard_ratio*B rays with the
    largest per-ray MSE enter the pool (appended until it holds >= B*hard_mul rows, then replacing random rows), and
    n_hard_out random pool rows are appended to every batch once the pool is full.

    The pool ([rows, 9] = o,d,rgb; 59 MB at the README sizes) lives on the device of the rays it is fed, is allocated
    once at its final size, and on a GPU the random row choice is a device randperm: the reference's host-side
    np.random.permutation(1.6 M) per step costs as much as a whole MI355X training step.

    device_select=True (GPU only, --r2l_device_pool): update() ranks the rays inside the library — r2l_pool_select, a radix
    select, then r2l_pool_store: two launches — instead of a torch sort of all B errors.  The hard rays then enter the pool in
    index order (the default path stores them in error order), so a run with the switch is another run than one without.
    state_dict() / load_state_dict(): what a checkpoint needs to continue the pool bit for bit."""

    def __init__(self, hard_ratio, hard_mul, rng=None, seed=0, device_select=False):
        self.ratio, self.mul = hard_ratio, hard_mul
        self.device_select = bool(device_select)
        self._batch_size = None  # the batch size the store was sized for (first update)
        self.pool = None      # rows filled so far (a view of _store once allocated)
        self._store = None
        self.full = False
        self.rng = rng or np.random
        self.seed = seed
        self._draws = 0
        self._ix_out = None

    def sizes(self, batch_size):
        if isinstance(self.ratio, list):
            n_in, n_out = int(self.ratio[0] * batch_size), int(self.ratio[1] * batch_size)
        else:
            n_in = n_out = int(self.ratio * batch_size)
        return min(n_in, n_out), n_out

    def _pick(self, n_rows, n_out, device):
        if device.type == "cuda":
            # n_out distinct rows, every row equally likely: a keyed bijection of [0, n_rows) evaluated at 0 .. n_out-1
            # (include/r2l_hip.h r2l_pool_pick) instead of a 1.6 M-key randperm per step; key = f(seed, draw counter)
            from . import _lib
            lib = _lib.load()
            ix = torch.empty(n_out, dtype=torch.int64, device=device)
            self._draws += 1
            key = self._key(self._draws)
            _lib.check(lib.r2l_pool_pick(_lib.ptr(ix), n_out, n_rows, key, _lib.stream()), "r2l_pool_pick")
            return ix
        return torch.as_tensor(self.rng.permutation(n_rows)[:n_out], device=device)

    def _key(self, draws):
        """Key of the keyed row choice number `draws` (counted from 1) of this pool."""
        return (self.seed * 0x9E3779B97F4A7C15 + draws * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF

    # ---- a step that moves the rows itself (r2l_student_train_step: R2LTrainer.fused_step) ------------------------------------
    def plan(self, batch_size, device="cpu"):
        """What the next step on a batch of `batch_size` rays does with the pool, as augment() + update() would: n_in hard rays
        enter (appended at row pool_rows while the pool is not full, else replacing picked rows), n_out rows picked with `key`
        are appended to the batch once it is full.  Allocates the store (on `device`) if this is the first step.  Changes
        nothing else: advance() does."""
        n_in, n_out = self.sizes(batch_size)
        if n_in > 0 and self._store is None:
            self._allocate(batch_size, n_in, torch.device(device))
        rows = self._n if self._store is not None else 0
        return {"n_in": max(n_in, 0), "n_out": n_out if n_in > 0 else 0, "pool_rows": rows, "full": bool(self.full),
                "capacity": self._store.shape[0] if self._store is not None else 0,
                "key": self._key(self._draws + 1) if self.full else 0}

    def advance(self, batch_size):
        """The bookkeeping of augment() + update() for a step whose rows were moved by the library (plan() said how): the draw
        counter, the fill count and the fill state."""
        n_in, _ = self.sizes(batch_size)
        if self.full:
            self._draws += 1
            self._ix_out = None  # (the rows that step picked stayed in its work buffer: nothing of an earlier augment() is valid)
            return
        if n_in <= 0:
            return
        self._n += n_in
        self.pool = self._store[:self._n]
        if self._n >= batch_size * self.mul:
            self.full = True

    @staticmethod
    def _rows(x):
        """(tensor, row stride in floats) of a [N,3] fp32 tensor whose rows are contiguous (column slices of a shard batch)."""
        if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != 3 or x.stride(1) != 1:
            x = x.float().contiguous()
        return x, x.stride(0)

    def extra_rays(self, batch_size, updates_done):
        """Rays augment() appends to a batch of `batch_size` after `updates_done` update() calls on batches of that size — a
        pure function of the two, so every rank of a data-parallel run can tell every other rank's step size without a
        collective (driver.train: global ray count of a step when --N_rand does not divide by the world size)."""
        n_in, n_out = self.sizes(batch_size)
        if n_in <= 0:
            return 0
        steps_to_full = max(1, -(-int(np.ceil(batch_size * self.mul)) // n_in))
        return n_out if updates_done >= steps_to_full else 0

    def augment(self, rays_o, rays_d, target):
        if not self.full:
            return rays_o, rays_d, target
        _, n_out = self.sizes(rays_o.shape[0])
        self._ix_out = self._pick(self.pool.shape[0], n_out, self.pool.device)
        if self.pool.is_cuda:  # one kernel: batch rows (possibly column slices of the [B,9] shard batch) + picked pool rows
            from . import _lib
            lib, B = _lib.load(), rays_o.shape[0]
            (o, so), (d, sd), (t, st) = self._rows(rays_o), self._rows(rays_d), self._rows(target)
            out = torch.empty(3, B + n_out, 3, dtype=torch.float32, device=self.pool.device)
            p = _lib.ptr
            _lib.check(lib.r2l_pool_augment(p(o), p(d), p(t), so, sd, st, p(self.pool), p(self._ix_out), B, n_out, p(out[0]),
                                            p(out[1]), p(out[2]), _lib.stream()), "r2l_pool_augment")
            return out[0], out[1], out[2]
        picked = self.pool[self._ix_out]
        return (torch.cat([rays_o, picked[:, :3]], 0), torch.cat([rays_d, picked[:, 3:6]], 0),
                torch.cat([target, picked[:, 6:]], 0))

    def _allocate(self, batch_size, n_in, device):
        steps = max(1, -(-int(np.ceil(batch_size * self.mul)) // n_in))
        self._store = torch.empty(steps * n_in, 9, dtype=torch.float32, device=device)
        self._n = 0
        self._batch_size = int(batch_size)

    def state_dict(self):
        """The pool as a checkpoint carries it: the filled rows on the host, the fill state, the draw counter of the keyed row
        choice and the three numbers the store's size follows from."""
        rows = self.pool.detach().cpu().clone() if self.pool is not None else torch.empty(0, 9, dtype=torch.float32)
        return {"rows": rows, "full": bool(self.full), "n": int(rows.shape[0]), "draws": int(self._draws),
                "hard_ratio": self.ratio, "hard_mul": self.mul, "batch_size": self._batch_size}

    def load_state_dict(self, state, device=None, batch_size=None):
        """Continue from state_dict().  device: where the pool lives (default: where the saved rows are); batch_size: the batch
        size of the run that continues, when it is known.  ValueError naming the field if the pool was built for other numbers."""
        for field, mine in (("hard_ratio", self.ratio), ("hard_mul", self.mul)):
            if state[field] != mine:
                raise ValueError("HardRayPool.load_state_dict: %s is %r in the saved pool, %r here" % (field, state[field], mine))
        if batch_size is not None and state["batch_size"] is not None and int(batch_size) != state["batch_size"]:
            raise ValueError("HardRayPool.load_state_dict: batch_size is %d in the saved pool, %d here" %
                             (state["batch_size"], int(batch_size)))
        rows = state["rows"]
        if rows.shape[0] != state["n"] or (state["batch_size"] is None and state["n"]):
            raise ValueError("HardRayPool.load_state_dict: n is %d in the saved pool, which holds %d rows" %
                             (state["n"], rows.shape[0]))
        self._draws, self.full, self._ix_out = int(state["draws"]), False, None
        self.pool = self._store = self._batch_size = None
        if state["batch_size"] is None:
            return
        n_in, _ = self.sizes(state["batch_size"])
        self._allocate(state["batch_size"], n_in, torch.device(device) if device is not None else rows.device)
        if state["n"] > self._store.shape[0]:
            raise ValueError("HardRayPool.load_state_dict: n is %d in the saved pool, the store holds %d rows" %
                             (state["n"], self._store.shape[0]))
        self._n = int(state["n"])
        self._store[:self._n].copy_(rows)
        self.pool = self._store[:self._n]
        self.full = bool(state["full"])

    def update(self, rgb, rays_o, rays_d, target, batch_size):
        n_in, _ = self.sizes(batch_size)
        if n_in <= 0:
            return
        if self.device_select:
            if not (rgb.is_cuda and rays_o.is_cuda):
                raise NotImplementedError("HardRayPool(device_select=True) ranks the rays on the GPU only (r2l_pool_select of "
                                          "libr2l_hip.so); these rays are on %s" % rays_o.device)
            from .pool_select import select
            hard = select(rgb[:batch_size], target[:batch_size], n_in)  # ascending index order, ties to the lower index
        else:
            err = torch.mean((rgb[:batch_size] - target[:batch_size])**2, dim=1)
            _, order = torch.sort(err)
            hard = order[-n_in:]
        if self._store is None:  # final size: the first multiple of n_in that reaches batch_size * hard_mul
            self._allocate(batch_size, n_in, rays_o.device)
        if rays_o.is_cuda:  # one kernel: gather the hard rows [o, d, rgb] and put them where they go (replace / append)
            from . import _lib
            lib = _lib.load()
            (o, so), (d, sd), (t, st) = self._rows(rays_o), self._rows(rays_d), self._rows(target)
            hard = hard.contiguous()
            dst = self._ix_out[:n_in].contiguous() if self.full else None
            p = _lib.ptr
            _lib.check(lib.r2l_pool_store(p(o), p(d), p(t), so, sd, st, p(hard), p(self._store), p(dst), 0 if self.full else self._n,
                                          n_in, _lib.stream()), "r2l_pool_store")
            if self.full:
                return
        else:
            rows = torch.cat([rays_o[hard], rays_d[hard], target[hard]], dim=-1)
            if self.full:
                self.pool[self._ix_out[:n_in]] = rows
                return
            self._store[self._n:self._n + n_in] = rows
        self._n += n_in
        self.pool = self._store[:self._n]
        if self._n >= batch_size * self.mul:
            self.full = True


# ---------------------------------------------------------------------------------------------------------------
def create_r2l(args, device, logger):
    """Model + (optional) checkpoint, following main.py:455-509: a checkpoint that carries the pickled `network_fn`
    REPLACES the freshly constructed module before its state dict is loaded."""
    embedder = PositionalEmbedder(L=args.multires, device=device)
    input_dim = args.n_sample_per_ray * 3 * embedder.embed_dim
    model = NeRF_v3_2(args, input_dim, 3).to(device)
    history = {"start": 0, "best_psnr": 0, "best_psnr_step": 0}
    ckpt = None
    if args.pretrained_ckpt:
        ckpt = load_ckpt(args.pretrained_ckpt, map_location=device)
        if "network_fn" in ckpt:
            model = ckpt["network_fn"].to(device)
            logger.info('Use model arch saved in checkpoint "%s"' % args.pretrained_ckpt)
        load_weights_v2(model, ckpt, "network_fn_state_dict")
        logger.info('Load pretrained ckpt successfully: "%s".' % args.pretrained_ckpt)
        if args.resume:
            history.update(start=ckpt["global_step"], best_psnr=ckpt.get("best_psnr", 0),
                           best_psnr_step=ckpt.get("best_psnr_step", 0))
    n_params = sum(p.numel() for p in model.parameters())
    macs = sum(m.in_features * m.out_features for m in model.modules() if isinstance(m, torch.nn.Linear))
    logger.info("Model complexity per pixel: FLOPs %.10fM, Params %.10fM" % (macs / 1e6, n_params / 1e6))
    return model, embedder, history, ckpt


def create_nerf_teacher(args, device, logger, near, far, ndc=False):
    """The `model_name in ['nerf']` branch of create_nerf (main.py:407-453, 481-509, 511-541) for rendering: coarse NeRF (+ the
    fine one when N_importance > 0) built from --netdepth/--netwidth(/_fine), weights from --pretrained_ckpt through
    load_weights_v2 ('network_fn_state_dict' / 'network_fine_state_dict'; a checkpoint that carries pickled modules replaces the
    constructed ones), and render_kwargs_test: perturb = --perturb_test, raw_noise_std = 0, near / far / ndc of the scene.
    Teacher TRAINING is out of scope: no optimizer, parameters frozen."""
    from .nerf_raybased import NeRF
    from .render import get_embedder, run_network
    embed_fn, input_ch = get_embedder(args.multires, args.i_embed)
    embeddirs_fn, input_ch_views = (get_embedder(args.multires_views, args.i_embed) if args.use_viewdirs else (None, 0))
    output_ch = 5 if args.N_importance > 0 else 4
    model = NeRF(D=args.netdepth, W=args.netwidth, input_ch=input_ch, output_ch=output_ch, skips=[4],
                 input_ch_views=input_ch_views, use_viewdirs=args.use_viewdirs).to(device)
    model_fine = None
    if args.N_importance > 0:
        model_fine = NeRF(D=args.netdepth_fine, W=args.netwidth_fine, input_ch=input_ch, output_ch=output_ch, skips=[4],
                          input_ch_views=input_ch_views, use_viewdirs=args.use_viewdirs).to(device)
    if args.pretrained_ckpt:
        ckpt = load_ckpt(args.pretrained_ckpt, map_location=device)
        if "network_fn" in ckpt:
            model = ckpt["network_fn"].to(device)
            if model_fine is not None:
                assert "network_fine" in ckpt
                model_fine = ckpt["network_fine"].to(device)
            logger.info('Use model arch saved in checkpoint "%s"' % args.pretrained_ckpt)
        load_weights_v2(model, ckpt, "network_fn_state_dict")
        if model_fine is not None:
            load_weights_v2(model_fine, ckpt, "network_fine_state_dict")
        logger.info('Load pretrained ckpt successfully: "%s".' % args.pretrained_ckpt)
    for net in (model, model_fine):
        if net is not None:
            for p in net.parameters():
                p.requires_grad = False
    qfn = lambda inputs, viewdirs, fn: run_network(inputs, viewdirs, fn, embed_fn=embed_fn, embeddirs_fn=embeddirs_fn,
                                                   netchunk=args.netchunk)
    n_params = sum(p.numel() for p in model.parameters())
    macs = sum(m.in_features * m.out_features for m in model.modules() if isinstance(m, torch.nn.Linear))
    macs *= args.N_samples + args.N_samples + args.N_importance  # as main.py:547-549
    logger.info("Model complexity per pixel: FLOPs %.10fM, Params %.10fM" % (macs / 1e6, n_params / 1e6))
    # render_kwargs_test (main.py:511-541) + bds_dict (main.py:977-982)
    return dict(network_query_fn=qfn, perturb=args.perturb_test, N_importance=args.N_importance, network_fine=model_fine,
                N_samples=args.N_samples, network_fn=model, use_viewdirs=args.use_viewdirs, white_bkgd=args.white_bkgd,
                raw_noise_std=0., ndc=ndc, lindisp=args.lindisp, near=near, far=far)


def apply_arithmetic(args, device, logger, student=None, teachers=()):
    """--r2l_precision / --r2l_dw_mode (options.py; include/r2l_hip.h r2l_config) -> the engines of this run, through
    R2LEngine.set_config / TeacherEngine.set_config — arguments of the *_cfg entry points, not environment switches.  Returns the
    record {'precision', 'dw_mode', 'requested': {...}} that is logged here and stored in every checkpoint the run writes (key
    'r2l_config': the reference's loaders never look at it, main.py:481-509).  CPU (config 0, plumbing): torch fp32 ops."""
    req = {"precision": args.r2l_precision, "dw_mode": args.r2l_dw_mode}
    if device.type != "cuda":
        rec = {"precision": "torch fp32 (CPU plumbing)", "dw_mode": "autograd fp32", "requested": req}
    else:
        from . import engine as _engine
        cfg = _lib_config(req)
        if student is not None:
            student.engine().set_config(precision=req["precision"], dw_mode=req["dw_mode"])
        for net in teachers:
            if net is not None:
                from .render import teacher_engine
                teacher_engine(net).set_config(precision=req["precision"])
        rec = dict(_engine.arithmetic(cfg), requested=req)
    logger.info("r2l_config: precision %s, dw_mode %s (requested: --r2l_precision %s --r2l_dw_mode %s)" %
                (rec["precision"], rec["dw_mode"], req["precision"], req["dw_mode"]))
    return rec


def _lib_config(req):
    from . import _lib
    return _lib.make_config(precision=req["precision"], dw_mode=req["dw_mode"])


POSES_PER_LAUNCH = 9


def render_frame(model, point_sampler, c2w):
    """One frame [H,W,3] (main.py:300-324 R2L branch): fused sample -> encode -> network."""
    with torch.no_grad():
        rgb = model.render_pose(c2w[:3, :4], point_sampler)
    return rgb.view(point_sampler.H, point_sampler.W, 3)


class _FrameWriter:
    """PNG writing off the render loop (replaces the inline imageio.imwrite of main.py:337-344): the frame is quantised to 8
    bit on the device (same rounding as to8b), copied non-blocking into a pinned buffer, and handed — with the event behind
    the copy — to the library's encoder threads (include/r2l_hip.h r2l_png_writer_*: native threads, zlib level 1, no GIL).
    Rounds 1 - 3 encoded with PIL in Python threads: ~15 ms per 400x400 PNG with the GIL held around zlib, which made the
    test-set loop encoder-bound (6.5 ms/frame against 4.5 without images, profiles/r03_e2e_render.txt)."""

    # With 9 frames per launch 27 images arrive at once (frame, target, error): the pinned staging slots must cover two groups, or
    # save() blocks on the encoders before the next group's render is launched.
    def __init__(self, device, workers=None, slots=6 * POSES_PER_LAUNCH + 4, level=1):
        from . import _lib
        self._lib, self.lib = _lib, _lib.load()
        self.device, self.slots = device, slots
        n = workers or max(4, min(32, os.cpu_count() or 8))
        self._h = ctypes.c_void_p()
        _lib.check(self.lib.r2l_png_writer_open(n, level, ctypes.byref(self._h)), "r2l_png_writer_open")
        self.inflight = []  # (job id, what must stay alive until it is done, recyclable pinned buffer or None)
        self.free = {}

    def _submit(self, path, ptr, shape, event):
        H, W = int(shape[0]), int(shape[1])
        C = int(shape[2]) if len(shape) == 3 else 1
        job = ctypes.c_int64()
        self._lib.check(self.lib.r2l_png_writer_submit(self._h, os.fsencode(path), ctypes.c_void_p(ptr), H, W, C,
                                                       ctypes.c_void_p(event) if event else None, ctypes.byref(job)),
                        "r2l_png_writer_submit")
        return job.value

    def _retire(self, n_keep):
        while len(self.inflight) > n_keep:
            job, _, host = self.inflight.pop(0)
            try:
                self._lib.check(self.lib.r2l_png_writer_wait(self._h, job), "r2l_png_writer_wait")
            finally:  # (a failed write still returns its pinned staging slot: the writer stays usable)
                if host is not None:
                    self.free.setdefault(tuple(host.shape), []).append(host)

    def save(self, img, path):
        """img: float [H,W,3] in [0,1] (device or host tensor / array)."""
        if isinstance(img, torch.Tensor) and img.is_cuda:
            q = (255 * torch.clamp(img, 0, 1)).to(torch.uint8).contiguous()  # float -> uint8 truncates, as numpy's astype does
            key = tuple(q.shape)
            free = self.free.get(key)
            if free is None:  # ONE pinned allocation for all staging slots of this frame size (44 separate ones cost ~100 ms)
                slab = torch.empty((self.slots,) + key, dtype=torch.uint8, pin_memory=True)
                free = self.free[key] = [slab[i] for i in range(self.slots)]
            if not free:
                self._retire(self.slots - 1)
            if not free:  # (every slot of this size still in flight behind jobs of another size: wait for all)
                self._retire(0)
            host = free.pop()
            host.copy_(q, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self.inflight.append((self._submit(path, host.data_ptr(), key, ev.cuda_event), (ev, q), host))
        else:
            arr = np.ascontiguousarray(to8b(img))
            self.inflight.append((self._submit(path, arr.ctypes.data, arr.shape, None), arr, None))

    def flush(self):
        """Every frame handed over so far is on disk (the writer stays usable: its threads and pinned slots are kept)."""
        self._retire(0)

    def close(self):
        if not self._h:
            return
        self._retire(0)
        self._lib.check(self.lib.r2l_png_writer_close(self._h), "r2l_png_writer_close")
        self._h = ctypes.c_void_p()

    _shared = {}

    @classmethod
    def shared(cls, device, workers=None):
        """One writer per device and process, kept across render_path calls (the test set is evaluated every i_testset
        iterations: thread start-up and the pinned allocation are paid once)."""
        key = (str(device), workers)
        w = cls._shared.get(key)
        if w is None:
            import atexit
            w = cls._shared[key] = cls(device, workers=workers)
            atexit.register(w.close)
        return w


def save_video(rgbs, logger, expid, iter_, tag, rank=0, world=1, device=None):
    """`video_<expid>_iter<k>_<tag>` of main.py:1096-1097 / 1483-1484 from the frames render_path returned (this rank's
    poses[rank::world]; with world > 1 the ranks' frames are gathered to rank 0 and re-interleaved).  Container: Motion-JPEG
    AVI instead of the reference's mp4 (video.py says why).  Returns the path on rank 0, None elsewhere."""
    from .video import write_mjpeg_avi
    frames = to8b(rgbs) if rgbs.numel() else np.zeros((0, 0, 0, 3), np.uint8)
    if world > 1:
        parts = [None] * world if rank == 0 else None
        dist.gather_object(frames, parts, dst=0)  # only rank 0 needs (and holds) the other ranks' frames
        if rank != 0:
            return None
        total = sum(p.shape[0] for p in parts)
        hw = next((p.shape[1:] for p in parts if p.shape[0]), (0, 0, 3))
        allf = np.zeros((total,) + tuple(hw), np.uint8)
        for r, p in enumerate(parts):
            if p.shape[0]:  # (a rank beyond the number of poses rendered nothing)
                allf[r::world] = p
        frames_np = allf
    else:
        frames_np = frames
    path = os.path.join(logger.gen_img_path, "video_%s_iter%s_%s.avi" % (expid, iter_, tag))
    os.makedirs(logger.gen_img_path, exist_ok=True)
    write_mjpeg_avi(path, frames_np, fps=30, quality=8)
    return path


FLIP_FRAMES_PER_LAUNCH = 64  # frame pairs per r2l_flip launch (its map is not kept: scratch is one float per 32x8 tile)


LPIPS_WORK_BYTES = 256 << 20  # the work buffer of one r2l_lpips launch may take this much (26 MB per 400x400 pair: 9 pairs)


def lpips_frames_per_launch(H, W):
    """LPIPS_FRAMES_PER_LAUNCH: frame pairs per r2l_lpips launch, from the size of its work buffer (at least 1, at most 64)."""
    from . import _lib
    per_pair = 4 * _lib.load().r2l_lpips_work_floats(1, H, W)
    return max(1, min(64, LPIPS_WORK_BYTES // max(per_pair, 1)))


LPIPS_VGG_WORK_BYTES = 1 << 30  # the same for r2l_lpips_vgg, whose maps are full resolution (236 MB per 400x400 pair: 4 pairs)


def lpips_vgg_frames_per_launch(H, W):
    """Frame pairs per r2l_lpips_vgg launch, from the size of its work buffer (at least 1, at most 64)."""
    from . import _lib
    per_pair = 4 * _lib.load().r2l_lpips_vgg_work_floats(1, H, W)
    return max(1, min(64, LPIPS_VGG_WORK_BYTES // max(per_pair, 1)))


def _stack_extrema(rgbs, gts, device, world):
    """-> the target stack and {min, max} of the rendered and of the target stack over ALL frames of the test set (main.py:361-363
    rescales both to [-1, 1] by them before LPIPS and FLIP).  The extrema stay on the device (one all_reduce(MAX) makes them
    global) and go to the kernels as a pointer: no host sync here."""
    if gts:
        gts = torch.stack(gts, 0)
        ext = torch.stack([rgbs.max(), -rgbs.min(), gts.max(), -gts.min()]).float()
    else:  # a rank beyond the number of poses still takes part in the collective
        ext = torch.full((4,), -torch.finfo(torch.float32).max, device=device)
    if world > 1:
        dist.all_reduce(ext, op=dist.ReduceOp.MAX)
    return gts, torch.stack([-ext[1], ext[0], -ext[3], ext[2]])


def _flip_sum(rgbs, gts, extrema, device):
    """Sum over this rank's frames of the per-frame FLIP means (fp64, 0-d, on the device), evaluated as main.py:359-379 does:
    rendered and target stacks (gts, extrema: _stack_extrema) are each rescaled to [-1, 1], then compute_flip."""
    total = torch.zeros((), dtype=torch.float64, device=device)
    for g0 in range(0, len(gts), FLIP_FRAMES_PER_LAUNCH):
        total += flip(rgbs[g0:g0 + FLIP_FRAMES_PER_LAUNCH], gts[g0:g0 + FLIP_FRAMES_PER_LAUNCH], rescale=extrema).double().sum()
    return total


def _lpips_sum(rgbs, gts, extrema, params, device, vgg=False):
    """Sum over this rank's frames of LPIPS(AlexNet; vgg: VGG-16) on the same rescaled stacks (main.py:359-369), in launch groups
    sized by the kernels' work buffer."""
    total = torch.zeros((), dtype=torch.float64, device=device)
    if len(gts):
        fn, per_launch = (lpips_vgg, lpips_vgg_frames_per_launch) if vgg else (lpips, lpips_frames_per_launch)
        n = per_launch(*rgbs.shape[1:3]) if device.type == "cuda" else 8  # (the reference's batches of 8)
        for g0 in range(0, len(gts), n):
            total += fn(rgbs[g0:g0 + n], gts[g0:g0 + n], params, rescale=extrema).double().sum()
    return total


def _runs(idx):
    """(start, length) of the runs of consecutive integers in idx: [3, 4, 5, 9] -> (0, 3), (3, 1)."""
    out, k = [], 0
    for j in range(1, len(idx) + 1):
        if j == len(idx) or idx[j] != idx[j - 1] + 1:
            out.append((k, j - k))
            k = j
    return out


def render_path(poses, model, point_sampler, device, logger, gt_imgs=None, savedir=None, rank=0, world=1, teacher=None,
                lpips_params=None, lpips_vgg_params=None, ray_cull=None):
    """Render poses[rank::world]; returns (rgbs [n,H,W,3], misc with test_loss/test_psnr/test_psnr_v2 over ALL frames)
    and test_ssim / test_flip — main.py:189-398.  No host
    sync inside the loop: metrics stay on the device, frames are written by _FrameWriter, per-frame times come from device
    events and are logged after the loop.  FLIP runs once behind the loop (_flip_sum): the reference rescales both stacks by
    their extrema over ALL frames first (main.py:361-363), so it cannot be accumulated frame by frame.
    lpips_params = the flat AlexNet + lin weights of metrics.lpips_params (--r2l_lpips_weights: the user's files, none are
    shipped): misc gains test_lpips (main.py:359-369, 392), evaluated behind the loop on the same rescaled stacks (_lpips_sum);
    None: no LPIPS work at all and no such key.
    lpips_vgg_params = the flat VGG-16 + lin weights of metrics.lpips_vgg_params (--r2l_lpips_vgg_weights): misc gains
    test_lpips_vgg in the same way (the number the published tables call LPIPS); None: no VGG work and no such key.
    teacher = None: the R2L branch (main.py:284-324), `model` = the student.
    teacher = dict(hwf=(H, W, focal), chunk=, render_kwargs=): the `model_name in ['nerf']` branch (main.py:275-282): every
    frame is render(H, W, focal, chunk, c2w=pose[:3,:4], **render_kwargs) of r2l_amd/render.py (coarse + fine NeRF on the
    teacher kernels); `model` = render_kwargs['network_fn'], `point_sampler` unused.  With fused=True in that dict
    (--r2l_fused_frames; GPU only) the frames come from render_frames in groups of POSES_PER_LAUNCH instead.
    ray_cull = a ray_cull.RayCull (--r2l_ray_cull; student branch, GPU): the rays of a launch group that meet no occupied cell are
    left out of the forward and get the background colour exactly; None: nothing changes."""
    model.eval()
    if ray_cull is not None and (teacher is not None or device.type != "cuda"):
        raise ValueError("--r2l_ray_cull culls the student's renders on a GPU (not the teacher branch, not a CPU run)")
    mine = list(range(rank, len(poses), world))
    rgbs, gts, sq_err, psnrs, ssims, events, errors = [], [], [], [], [], [], []
    if savedir is not None:
        os.makedirs(savedir, exist_ok=True)  # every rank writes its own frames: none may rely on rank 0's mkdir
    writer = _FrameWriter.shared(device, workers=int(os.environ.get("R2L_PNG_WORKERS", "0")) or None) if savedir is not None else None
    on_gpu = device.type == "cuda"
    t_loop = time.time()
    def account(i, rgb):
        rgbs.append(rgb)
        if gt_imgs is not None:
            gt = gt_imgs[i].to(rgb.device, non_blocking=True)
            if gt.shape[:2] != rgb.shape[:2]:  # --render_factor (teacher branch): the reference CROPS the target, main.py:329-333
                gt = gt[:rgb.shape[0], :rgb.shape[1]].contiguous()
            gts.append(gt)
            errors.append((rgb - gt).abs())  # misc['errors'] (main.py:330, 386): this rank's frames; main() writes their video
            mse = img2mse(rgb, gt)
            sq_err.append(mse)
            psnrs.append(mse2psnr(mse))
            ssims.append(ssim(rgb, gt))
        if writer is not None:
            writer.save(rgb, os.path.join(savedir, "%03d.png" % i))
            if gt_imgs is not None:
                writer.save(gt_imgs[i], os.path.join(savedir, "%03d_gt.png" % i))
                # |rgb - gt| as an image, as the reference saves it beside every test frame (main.py:330, 342-344)
                writer.save(errors[-1], os.path.join(savedir, "%03d_error.png" % i))

    if teacher is not None:
        from .render import render
        H, W, focal = teacher["hwf"]
        rf = teacher.get("render_factor", 0)
        if rf != 0:  # "Render downsampled for speed" (main.py:197-201); the R2L branch's sampler is built for the full frame
            H, W, focal = int(H / rf), int(W / rf), focal / rf
        # a whole frame per launch on the GPU (as create_data.main: --chunk is a memory work-around of the op-by-op path)
        chunk = max(int(teacher["chunk"]), H * W) if on_gpu else int(teacher["chunk"])
        fused = bool(teacher.get("fused"))
        if fused and not on_gpu:
            raise NotImplementedError("--r2l_fused_frames renders through libr2l_hip.so: it needs a GPU")
        logger.info("teacher frames: " + ("fused, one library call per %d poses (render_frames)" % POSES_PER_LAUNCH if fused
                                          else "render() per pose"))
        if fused:  # groups of poses through r2l_teacher_frames_cfg, as the student branch below groups its frames
            from .render import render_frames
            kw = teacher["render_kwargs"]
            if kw.get("lindisp") or kw.get("raw_noise_std", 0.) or not kw.get("use_viewdirs", True):
                raise NotImplementedError("--r2l_fused_frames: lindisp, raw_noise_std > 0 and use_viewdirs=False are outside the fused path")
            for g0 in range(0, len(mine), POSES_PER_LAUNCH):
                idx = mine[g0:g0 + POSES_PER_LAUNCH]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                c2ws = torch.stack([torch.as_tensor(poses[i], dtype=torch.float32)[:3, :4] for i in idx], 0).to(device)
                with torch.no_grad():  # (draws of --perturb_test > 0: stream pair of frame i = its pose number, whatever the ranks)
                    outs = [render_frames(c2ws[k:k + n], H, W, focal, kw["near"], kw["far"], kw["network_fn"], kw.get("network_fine"),
                                          kw["N_samples"], kw.get("N_importance", 0), kw.get("perturb", 0.), kw.get("white_bkgd", False),
                                          seed=int(teacher.get("seed", 0)), frame_id0=idx[k], ndc=bool(kw.get("ndc")),
                                          **(teacher["occ_fused"].kwargs() if teacher.get("occ_fused") is not None else {}))["rgb"]
                            for k, n in _runs(idx)]
                frames = (outs[0] if len(outs) == 1 else torch.cat(outs, 0)).view(len(idx), H, W, 3)
                e1.record()
                events.append((idx, e0, e1))
                for k, i in enumerate(idx):
                    account(i, frames[k])
        for i in ([] if fused else mine):
            t0 = time.time()
            if on_gpu:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            c2w = torch.as_tensor(poses[i], dtype=torch.float32)[:3, :4].to(device)
            with torch.no_grad():
                rgb, _disp, _acc, _extras = render(H, W, focal, chunk=chunk, c2w=c2w, **teacher["render_kwargs"])
            if on_gpu:
                e1.record()
                events.append(([i], e0, e1))
            else:
                logger.info("[#%d] frame, rendering done, time for this frame: %.4fs" % (i, time.time() - t0))
            account(i, rgb)
    elif on_gpu:
        # POSES_PER_LAUNCH frames per launch (engine.forward_poses: no launch gap and no partly filled last round of
        # workgroups per frame; 9 x 1250 workgroups = 43.95 rounds of the 256 CUs at 400x400)
        for g0 in range(0, len(mine), POSES_PER_LAUNCH):
            idx = mine[g0:g0 + POSES_PER_LAUNCH]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            c2ws = torch.stack([torch.as_tensor(poses[i], dtype=torch.float32)[:3, :4] for i in idx], 0)
            with torch.no_grad():
                frames = (model.render_poses(c2ws, point_sampler) if ray_cull is None else
                          ray_cull.render_poses(model, c2ws, point_sampler)).view(len(idx), point_sampler.H, point_sampler.W, 3)
            e1.record()
            events.append((idx, e0, e1))
            for k, i in enumerate(idx):
                account(i, frames[k])
    else:
        for i in mine:
            t0 = time.time()
            rgb = render_frame(model, point_sampler, poses[i])
            logger.info("[#%d] frame, rendering done, time for this frame: %.4fs" % (i, time.time() - t0))
            account(i, rgb)
    rgbs = torch.stack(rgbs, 0) if rgbs else torch.empty(0)
    flip_sum = lpips_sum = lpips_vgg_sum = None
    if gt_imgs is not None:  # (enqueued before the host waits below)
        gts, extrema = _stack_extrema(rgbs, gts, device, world)
        flip_sum = _flip_sum(rgbs, gts, extrema, device)
        if lpips_params is not None:
            lpips_sum = _lpips_sum(rgbs, gts, extrema, lpips_params, device)
        if lpips_vgg_params is not None:
            lpips_vgg_sum = _lpips_sum(rgbs, gts, extrema, lpips_vgg_params, device, vgg=True)
    if writer is not None:
        writer.flush()  # (shared writer: threads and pinned slots stay for the next evaluation)
    if on_gpu:
        sync(device)
        if ray_cull is not None:
            ray_cull.log(logger, "ray cull (student renders so far)")
        for idx, e0, e1 in events:
            for i in idx:  # (one launch per group of frames: its time divided evenly)
                logger.info("[#%d] frame, rendering done, time for this frame: %.4fs" % (i, e0.elapsed_time(e1) * 1e-3 / len(idx)))
        if mine:
            logger.info("%d frames in %.3fs wall (%.1f ms/frame incl. metrics and image writing)" %
                        (len(mine), time.time() - t_loop, (time.time() - t_loop) * 1e3 / len(mine)))
    misc = {}
    if gt_imgs is not None:
        sums = [torch.stack(v).double().sum() if v else torch.zeros((), dtype=torch.float64, device=device)
                for v in (sq_err, psnrs, ssims)]
        stats = torch.stack([sums[0].reshape(()), sums[1].reshape(()),
                             torch.tensor(float(len(mine)), dtype=torch.float64, device=device),
                             sums[2].reshape(()), flip_sum.reshape(())] +
                            ([lpips_sum.reshape(())] if lpips_sum is not None else []) +
                            ([lpips_vgg_sum.reshape(())] if lpips_vgg_sum is not None else [])).to(device)
        if world > 1:
            dist.all_reduce(stats)  # host-side metric gather (5 scalars, one more per LPIPS variant), not on the data path
        stats = stats.tolist()
        misc["test_loss"] = torch.tensor(stats[0] / max(stats[2], 1))
        misc["test_psnr"] = mse2psnr(misc["test_loss"].float()).squeeze()
        misc["test_psnr_v2"] = torch.tensor(stats[1] / max(stats[2], 1))
        misc["test_ssim"] = torch.tensor(stats[3] / max(stats[2], 1))
        misc["test_flip"] = torch.tensor(stats[4] / max(stats[2], 1))  # (frames of one size: the mean of per-frame means, main.py:393)
        if lpips_sum is not None:
            misc["test_lpips"] = torch.tensor(stats[5] / max(stats[2], 1))
        if lpips_vgg_sum is not None:  # (the last entry)
            misc["test_lpips_vgg"] = torch.tensor(stats[-1] / max(stats[2], 1))
        misc["errors"] = torch.stack(errors, 0) if errors else torch.empty(0)
    model.train()
    return rgbs, misc


def load_lpips_weights(args, device, logger):
    """--r2l_lpips_weights -> the flat parameter vector on the device (metrics.lpips_params), or None without the flag."""
    from .metrics import lpips_params
    from .options import validate_lpips
    validate_lpips(args)
    if not args.r2l_lpips_weights:
        return None
    params = lpips_params(args.r2l_lpips_weights).to(device)
    logger.info("LPIPS (AlexNet, v0.1) in the test-set loop: %d parameters from %s" % (params.numel(), args.r2l_lpips_weights))
    return params


def load_lpips_vgg_weights(args, device, logger):
    """--r2l_lpips_vgg_weights -> the flat parameter vector on the device (metrics.lpips_vgg_params), or None without the flag."""
    from .metrics import lpips_vgg_params
    from .options import validate_lpips
    validate_lpips(args)
    if not args.r2l_lpips_vgg_weights:
        return None
    params = lpips_vgg_params(args.r2l_lpips_vgg_weights).to(device)
    logger.info("LPIPS (VGG-16, v0.1) in the test-set loop: %d parameters from %s" % (params.numel(), args.r2l_lpips_vgg_weights))
    return params


def lpips_field(misc):
    """' TestLPIPS %.4f' for the test-set log lines (main.py:1080, 1468: between TestSSIM and TestFLIP), then ' TestLPIPSvgg %.4f';
    each only with its flag."""
    return ((" TestLPIPS %.4f" % misc["test_lpips"].item() if "test_lpips" in misc else "") +
            (" TestLPIPSvgg %.4f" % misc["test_lpips_vgg"].item() if "test_lpips_vgg" in misc else ""))


# ---------------------------------------------------------------------------------------------------------------
def open_training_source(args, scene, H, W, focal, near, far, shards, start, rank, world, device, logger, ray_cull=None):
    """The source of this rank's training batches, as the options say: a store the teacher fills (--r2l_online_kd, plain or
    --r2l_compact_store), a store of the scene's real training rays (--r2l_image_store, alone or behind the teacher's), a store
    file (--r2l_store_load), a store the shard files are read into once (--r2l_device_store), or the reader of the shard files.  shards: shard files per step of every rank; start: the iteration a resumed run starts
    behind.  Returns (loader, files, filler): files — the names the run counts as its training files; filler — the
    online_kd.TeacherFill while poses are still pending, else None."""
    filler = None  # --r2l_online_kd: the teacher fill of the store (online_kd.TeacherFill), while poses are pending
    if args.r2l_online_kd:
        # no shard files: the teacher renders this rank's poses into a device-resident store (r2l_amd/online_kd.py), all of
        # them before iteration 1 or — --r2l_kd_every K — the first flush group now and one more every K iterations (the
        # reference's data arriving during training, --i_update_data, main.py:1218-1259, without the files).  The sampler
        # draws with the shard count of the moment.
        from .online_kd import TeacherFill, shards_needed
        from .options import parse_teacher_config
        from .raystore import RayStore
        targs = parse_teacher_config(args.r2l_teacher_config, teacher_ckpt=args.teacher_ckpt)
        targs.r2l_precision = args.r2l_precision  # one arithmetic switch per run: the teacher kernels follow the command line
        n_pose = args.n_pose_kd if isinstance(args.n_pose_kd, int) else int(args.n_pose_kd[0])
        cap = shards_needed(n_pose, args.create_data_chunk, H, W, rank, world)
        if cap < 1:
            raise ValueError("--r2l_online_kd: rank %d of %d gets no shard from --n_pose_kd %d" % (rank, world, n_pose))
        real = None  # --r2l_image_store: the real training rays go behind the teacher's groups, into the same store
        if args.r2l_image_store:
            from .image_store import fill_store_from_images, image_shards, training_frames
            real = training_frames(scene, args.white_bkgd)
            cap += image_shards(real[0].shape[0], H, W, rank, world)[1]
        if args.r2l_compact_store:
            # 16 bytes a ray: rgb and the ray's number in its flush group; o, d are recomputed per draw from the group's poses
            # (one pose-table slot per pose of this rank) and the batches are the plain store's bit for bit
            from .online_kd import rank_poses
            from .raystore import CompactRayStore
            loader = CompactRayStore(cap, len(rank_poses(n_pose, rank, world)), H, W, device, seed=9973 * rank, logger=logger)
        else:
            loader = RayStore(cap, device, seed=9973 * rank, logger=logger)
        filler = TeacherFill(loader, targs, H, W, focal, near, far, n_pose, args.create_data_chunk, rank, world, device, logger,
                             rand_pose=scene.rand_pose, ndc=scene.ndc, occ_args=args if (args.r2l_occ_fused or args.r2l_ert > 0) else None,
                             ray_cull=ray_cull)
        # a resumed run rebuilds what the store held at its start iteration: the frames are a pure function of seed and pose
        # number, so these are the same rows bit for bit
        n_groups = None if args.r2l_kd_every <= 0 else 1 + start // args.r2l_kd_every
        while not filler.done and (n_groups is None or filler.groups < n_groups):
            filler.fill_group()
        provenance = filler.provenance()
        if real is not None:  # (--r2l_kd_every 0, checked at start-up: the teacher's fill is complete)
            n_teacher = loader.n_shards
            n_real = fill_store_from_images(loader, real[0], real[1], focal, rank, world, logger=logger)
            # the sampler draws shards uniformly: the real share of the training set is a shard count, not a schedule
            logger.info("ray store: %d teacher shards + %d real shards = %d: real share %.4f of every epoch (the sampler draws shards "
                        "uniformly; --pseudo_ratio is not consulted)" %
                        (n_teacher, n_real, loader.n_shards, n_real / max(loader.n_shards, 1)))
            provenance.update({"real_frames": int(real[0].shape[0]), "real_shards": n_real})
            real = None
        files = loader.files
        if args.r2l_store_save:  # (--r2l_kd_every 0, checked at start-up: the fill is complete) render once, train many times
            from .raystore import store_rank_path
            loader.save(store_rank_path(args.r2l_store_save, rank, world), provenance=provenance, rank=rank, world=world)
        if filler.done:
            filler = None
    elif args.r2l_image_store:
        # no shard files and no teacher: the training images and poses the loader holds become the store's rows in one launch
        # (r2l_amd/image_store.py) — README step 5 without step 4.  A pure function of the scene and R2L_SEED: a resumed run
        # rebuilds the same rows bit for bit
        from .image_store import fill_store_from_images, image_shards, training_frames
        from .raystore import RayStore
        real = training_frames(scene, args.white_bkgd)
        loader = RayStore(max(image_shards(real[0].shape[0], H, W, rank, world)[1], 1), device, seed=9973 * rank, logger=logger)
        n_real = fill_store_from_images(loader, real[0], real[1], focal, rank, world, logger=logger)
        real = None
        files = loader.files
        if args.r2l_store_save:
            from .raystore import store_rank_path
            loader.save(store_rank_path(args.r2l_store_save, rank, world),
                        provenance={"image_store": args.datadir, "real_frames": len(scene.i_train), "real_shards": n_real, "H": H, "W": W,
                                    "focal": focal, "white_bkgd": bool(args.white_bkgd), "R2L_SEED": os.environ.get("R2L_SEED", "0")},
                        rank=rank, world=world)
    elif args.r2l_store_load:
        # the store a run with --r2l_store_save (or utils/create_data.py) wrote: plain or compact as the file says, its digests
        # recomputed on the device before a row of it is trained on
        from .raystore import load_store, read_store_header, store_rank_path
        path = store_rank_path(args.r2l_store_load, rank, world)
        hdr = read_store_header(path)
        if (hdr["rank"], hdr["world"]) != (rank, world):
            raise ValueError("--r2l_store_load %s: written by rank %d of %d, this is rank %d of %d" %
                             (path, hdr["rank"], hdr["world"], rank, world))
        if hdr["kind"] == 1 and (hdr["H"], hdr["W"]) != (H, W):
            raise ValueError("--r2l_store_load %s: a compact store of %d x %d frames, the scene is %d x %d" %
                             (path, hdr["H"], hdr["W"], H, W))
        if hdr["n_shards"] < shards[rank]:
            raise ValueError("--r2l_store_load %s: %d shards, one step of this rank draws %d (--N_rand %d over %d ranks)" %
                             (path, hdr["n_shards"], shards[rank], args.N_rand, world))
        if hdr["kind"] == 1 and args.r2l_fused_iter:
            raise ValueError("--r2l_store_load %s: a compact store hands out batches through its own kernel: not with "
                             "--r2l_fused_iter, which reads the 36-byte rows of the plain store" % path)
        logger.info("ray store file %s: provenance %s" % (path, json.dumps(hdr["provenance"], sort_keys=True)))
        if ray_cull is not None:  # the file is used as it is; the log says whether its rows were culled with this run's grid
            theirs = hdr["provenance"].get("ray_cull") if isinstance(hdr["provenance"], dict) else None
            diff = ["the file's provenance has no ray_cull entry (its rows were not culled)"] if not theirs else ray_cull.mismatch(theirs)
            logger.info("ray cull: the store file %s" % ("was culled with this run's grid" if not diff else
                                                         "and this run's grid DIFFER — " + "; ".join(diff)))
        if isinstance(hdr["provenance"], dict) and hdr["provenance"].get("ray_cull") and not args.r2l_ray_cull:
            raise ValueError("--r2l_store_load %s: its provenance says ray_cull (the store holds no ray that sees only empty space): "
                             "train on it with --r2l_ray_cull, so that every render of the run is culled too" % path)
        loader = load_store(path, device, seed=9973 * rank, logger=logger)
        files = loader.files
    elif args.r2l_device_store:
        # the shard files are read ONCE into device memory; no reader threads, no per-step host-to-device copy
        from .raystore import RayStore
        datadir_kd = args.datadir_kd.split(":")[1] if ":" in args.datadir_kd else args.datadir_kd
        files = D.list_ray_shards(datadir_kd, args.pseudo_ratio, args.pseudo_data_hold_ratio)
        mine = D.shard_for_rank(files, rank, world)
        if not mine:
            raise ValueError("rank %d got no ray shards (have %d files, world %d)" % (rank, len(files), world))
        rows, cols = ctypes.c_int64(), ctypes.c_int64()
        from . import _lib
        _lib.check(_lib.load().r2l_npy_shape(mine[0].encode(), ctypes.byref(rows), ctypes.byref(cols)), "r2l_npy_shape")
        loader = RayStore(len(mine), device, rays_per_shard=rows.value, seed=9973 * rank, logger=logger)
        loader.append_files(mine, threads=max(1, min(args.num_workers, 16)))
    else:
        datadir_kd = args.datadir_kd.split(":")[1] if ":" in args.datadir_kd else args.datadir_kd
        files = D.list_ray_shards(datadir_kd, args.pseudo_ratio, args.pseudo_data_hold_ratio)
        loader = D.RayShardLoader(files, shards[rank], rank=rank, world=world, device=device,
                                  threads=max(1, min(args.num_workers, 16)))
    if args.r2l_online_kd or args.r2l_device_store or args.r2l_store_load or args.r2l_image_store:
        loader.n_files = shards[rank]
        logger.info("ray store: %s" % loader.describe())
        if start > 0:  # --resume: the sampler is a pure function of (seed, shard count, draw): only the counter is restored
            loader.seek(start * shards[rank])
            logger.info("ray store: resuming at draw %d (start iteration %d x %d shards per step)" % (loader.draw, start, shards[rank]))
    return loader, files, filler


def main(argv=None):
    args = parse_args(argv)
    validate_accelerated(args)
    validate_image_store(args)
    validate_fused_iter(args)
    validate_compact_store(args)
    validate_store_file(args)
    validate_ray_cull(args)
    is_teacher = args.model_name == "nerf"
    if is_teacher and (not args.render_only or args.benchmark):
        # (--benchmark times render_func = the R2L student's forward, main.py:401-404,1124-1133)
        raise NotImplementedError("--model_name nerf: the accelerated path renders a pretrained teacher (--render_only, with or "
                                  "without --render_test / --test_pretrained) and uses it in utils/create_data.py; TRAINING "
                                  "the teacher runs through utils/train_nerf.py")
    if is_teacher:
        validate_occupancy(args, raw_noise_std=0.)  # (the teacher's test render runs without noise; student runs ignore the switch)
        validate_occ_fused(args, ("r2l_fused_frames",), raw_noise_std=0.)
        validate_ert(args, ("r2l_fused_frames",), raw_noise_std=0.)
    elif args.r2l_occ_fused or args.r2l_ert != 0:  # the teacher of the online fill: its config says whether it has view directions (its raw_noise_std
        targs_ = None         # is 0, or parse_teacher_config refuses it)
        if args.r2l_online_kd and args.r2l_teacher_config:
            from .options import parse_teacher_config
            targs_ = parse_teacher_config(args.r2l_teacher_config)
        validate_occ_fused(args, ("r2l_online_kd",), raw_noise_std=0., use_viewdirs=targs_.use_viewdirs if targs_ is not None else True)
        validate_ert(args, ("r2l_online_kd",), raw_noise_std=0., use_viewdirs=targs_.use_viewdirs if targs_ is not None else True)
    rank, world, device = init_distributed()
    validate_ray_cull(args, device.type)
    if args.r2l_device_pool and not (args.render_only or args.benchmark) and device.type != "cuda":
        raise NotImplementedError("--r2l_device_pool ranks the hard rays and draws the jitter on the GPU (r2l_pool_select, "
                                  "r2l_draw_uniform of libr2l_hip.so); this run is on the CPU")
    if not (args.render_only or args.benchmark):
        validate_fused_iter(args, world, device.type)
    np.random.seed(0)
    # every rank must build the same student: torch's default generator is seeded per process otherwise (the reference had
    # ONE module that nn.DataParallel re-broadcast every step, main.py:472-479); R2LTrainer additionally broadcasts rank 0's
    # flat parameter buffer once, so a checkpoint-less start is identical on all ranks by construction
    torch.manual_seed(int(os.environ.get("R2L_SEED", "0")))
    logger = Logger(args, rank)
    lpips_w = load_lpips_weights(args, device, logger)  # (read once; None without --r2l_lpips_weights)
    lpips_vgg_w = load_lpips_vgg_weights(args, device, logger)  # (None without --r2l_lpips_vgg_weights)

    scene = D.load_scene(args)
    images, poses, hwf = scene.images, scene.poses, scene.hwf
    logger.info("Loaded %s" % scene.kind, tuple(images.shape), tuple(poses.shape), hwf, args.datadir)
    i_train, i_val, i_test = scene.i_train, scene.i_val, scene.i_test
    near, far = scene.near, scene.far
    if hasattr(args, "trial") and args.trial.near > 0:
        assert args.trial.far > args.trial.near
        near, far = args.trial.near, args.trial.far
    images = scene.rgb_images(args.white_bkgd)
    H, W, focal = int(hwf[0]), int(hwf[1]), float(hwf[2])
    if args.focal_scale > 0:
        focal *= args.focal_scale

    teacher = ray_cull = None
    if is_teacher:
        kwargs_test = create_nerf_teacher(args, device, logger, near, far, ndc=scene.ndc)
        model, point_sampler = kwargs_test["network_fn"], None
        teacher = dict(hwf=(H, W, focal), chunk=args.chunk, render_kwargs=kwargs_test, render_factor=args.render_factor,
                       fused=args.r2l_fused_frames)
        history = {"start": 0, "best_psnr": 0, "best_psnr_step": 0}
        r2l_config = apply_arithmetic(args, device, logger, teachers=(model, kwargs_test["network_fine"]))
        if args.r2l_occupancy:  # both grids once, behind --r2l_precision
            from .occupancy import build_pair
            kwargs_test["occupancy"] = build_pair(args, model, kwargs_test["network_fine"], near, far, logger)
        if args.r2l_occ_fused or args.r2l_ert > 0:  # the same grids / early termination inside the fused frames calls of render_path
            from .occupancy import FusedOccupancy
            teacher["occ_fused"] = FusedOccupancy(args, model, kwargs_test["network_fine"], near, far, logger)
    else:
        model, embedder, history, ckpt = create_r2l(args, device, logger)
        point_sampler = PointSampler(H, W, focal, args.n_sample_per_ray, near, far, device=device)
        r2l_config = apply_arithmetic(args, device, logger, student=model)
        if ckpt is not None and ckpt.get("r2l_config"):
            was = ckpt["r2l_config"]
            logger.info("checkpoint was trained with r2l_config: precision %s, dw_mode %s" % (was.get("precision"), was.get("dw_mode")))
        if args.r2l_ray_cull:  # the grid of every student render of this run, of the store fill, and of the checkpoints it writes
            from . import ray_cull as _rc
            # (a training run renders its first student frame after the store fill: the fill's grid serves, nothing is built twice)
            ray_cull = _rc.for_run(args, ckpt, near, far, device, logger,
                                   fill_builds=bool(args.r2l_online_kd) and not (args.test_pretrained or args.render_only or args.benchmark))
        elif ckpt is not None and ckpt.get("r2l_ray_cull") is not None:
            logger.info("WARNING: the checkpoint carries a grid (key r2l_ray_cull): it was trained on a culled ray store and has never "
                        "seen a background ray; this run is without --r2l_ray_cull and renders every ray through it")
    test_poses, test_images = poses[i_test], images[i_test]
    video_poses = scene.video_poses
    start, best_psnr, best_psnr_step = history["start"], history["best_psnr"], history["best_psnr_step"]

    if args.test_pretrained:
        _, misc = render_path(test_poses, model, point_sampler, device, logger, gt_imgs=test_images, rank=rank,
                              world=world, teacher=teacher, lpips_params=lpips_w, lpips_vgg_params=lpips_vgg_w, ray_cull=ray_cull)
        logger.info("Pretrained test: TestLoss %.4f TestPSNR %.4f TestPSNRv2 %.4f TestSSIM %.4f%s TestFLIP %.4f" %
                    (misc["test_loss"].item(), misc["test_psnr"].item(), misc["test_psnr_v2"].item(),
                     misc["test_ssim"].item(), lpips_field(misc), misc["test_flip"].item()))

    if args.render_only:
        logger.info("RENDER ONLY")
        expid, iter_ = parse_expid_iter(args.pretrained_ckpt)
        t_ = time.time()
        if args.render_test:
            rgbs, misc = render_path(test_poses, model, point_sampler, device, logger, gt_imgs=test_images,
                                     savedir=logger.gen_img_path if rank == 0 or world > 1 else None, rank=rank,
                                     world=world, teacher=teacher, lpips_params=lpips_w, lpips_vgg_params=lpips_vgg_w, ray_cull=ray_cull)
            logger.info("[TEST] TestPSNR %.4f TestPSNRv2 %.4f TestSSIM %.4f%s TestFLIP %.4f" %
                        (misc["test_psnr"].item(), misc["test_psnr_v2"].item(), misc["test_ssim"].item(), lpips_field(misc),
                         misc["test_flip"].item()))
        else:
            rgbs, misc = render_path(video_poses, model, point_sampler, device, logger, savedir=logger.gen_img_path,
                                     rank=rank, world=world, teacher=teacher, ray_cull=ray_cull)
        n_rays = rgbs.numel() // 3 if rgbs.numel() else 0  # (frames x rendered pixels: --render_factor shrinks the teacher's frames)
        dt = time.time() - t_
        logger.info("Rendered %d frames (%d rays) in %.2fs on rank %d = %.0f rays/s incl. I/O; frames in %s" %
                    (rgbs.shape[0], n_rays, dt, rank, n_rays / max(dt, 1e-9), logger.gen_img_path))
        if teacher is not None and "occupancy" in teacher["render_kwargs"]:
            from .occupancy import log_live
            log_live(teacher["render_kwargs"]["occupancy"], logger)
        if teacher is not None and teacher.get("occ_fused") is not None:
            teacher["occ_fused"].log(logger)
        # (the reference writes the video of whichever frames it rendered — test views too, main.py:1096-1097)
        video_path = save_video(rgbs, logger, expid, iter_, args.video_tag, rank, world, device)
        if "errors" in misc:  # (main.py:1098-1102: the |rgb - gt| frames as a second video)
            save_video(misc["errors"], logger, expid, iter_, args.video_tag + "_error", rank, world, device)
        return {"misc": misc, "rgbs": rgbs, "logger": logger, "video_path": video_path, "r2l_config": r2l_config}

    if args.benchmark:
        # torch.utils.benchmark.Timer('render_func(model, pose)').timeit(100) in the reference (main.py:1124-1133)
        pose = video_poses[0]
        for _ in range(3):
            render_frame(model, point_sampler, pose)
        sync(device)
        t0 = time.time()
        n = 100 if device.type == "cuda" else 2
        for _ in range(n):
            render_frame(model, point_sampler, pose)
        sync(device)
        per = (time.time() - t0) / n
        logger.info("render_func(model, pose): %.3f ms per %dx%d frame = %.3f M rays/s" % (per * 1e3, H, W,
                                                                                           H * W / per / 1e6))
        return {"ms_per_frame": per * 1e3, "logger": logger}

    # ---------------- distillation training (data_mode rays) ----------------
    if not (args.r2l_online_kd or args.r2l_store_load or args.r2l_image_store) and (args.data_mode != "rays" or not args.datadir_kd):
        raise NotImplementedError("training on the accelerated path needs --data_mode rays --datadir_kd <dir of "
                                  "[4096,9] .npy ray shards> (README step 3/5), or --r2l_online_kd (the teacher renders into a "
                                  "device-resident ray store)")
    if args.r2l_image_store:
        # what the real group will hold is arithmetic on the loaded split: named, and checked against one step's draw, before
        # anything is allocated (and before a run without a GPU is turned away below)
        from .image_store import plan_image_store
        plan_image_store(args, len(i_train), H, W, rank, world, logger)
    if device.type != "cuda":
        raise RuntimeError("R2L training runs on the HIP path and needs a ROCm GPU")
    # --N_rand is the GLOBAL batch in shard files per step, as in the reference (its DataLoader builds one batch that
    # nn.DataParallel then splits over the GPUs, main.py:794-806,1374): each rank loads N_rand / world shards, so the
    # README command keeps its optimisation schedule (lrate, N_iters, hard-ray pool size) at any GPU count
    # (not divisible by the rank count — the README's --N_rand 20 on 8 GPUs —: the first N_rand % world ranks take one shard
    # more and every rank's gradient is weighted by its share of the step's rays, below; nn.DataParallel scattered uneven
    # batches the same way, main.py:1374)
    try:
        shards = split_shards(args.N_rand, world)
    except ValueError as e:
        raise SystemExit(str(e))
    loader, files, filler = open_training_source(args, scene, H, W, float(hwf[2]), near, far, shards, start, rank, world, device, logger,
                                                 ray_cull=ray_cull)
    uneven = len(set(shards)) > 1
    if uneven:
        logger.info("--N_rand %d over %d ranks: %s shard files per rank and step; gradients weighted by ray share" %
                    (args.N_rand, world, shards))
    logger.info("Loaded data. Now total #train files: %d (this rank: %d)" % (len(files), len(loader.files)))
    trainer = R2LTrainer(model, point_sampler, lw_rgb=args.lw_rgb)
    if ckpt is not None and args.resume:
        trainer.load_optimizer_state_dict(ckpt["optimizer_state_dict"])
        logger.info("Resume optimizer successfully.")
    pool = None
    if args.hard_ratio:
        pool = HardRayPool(args.hard_ratio, args.hard_mul, seed=1000 + rank, device_select=args.r2l_device_pool)
    # --r2l_device_pool: the pool ranks on the device, the jitter comes from the library's Philox streams (include/r2l_hip.h:
    # stream 2^61 + 4096 * iteration + rank of R2L_SEED), and at world size 1 the pool travels in every checkpoint: with the ray
    # store's seek a resumed run repeats the uninterrupted one bit for bit
    jitter_seed = int(os.environ.get("R2L_SEED", "0"))
    save_pool = bool(args.r2l_device_pool and pool is not None and world == 1)
    if args.r2l_device_pool:
        from .render import draw_uniform
        logger.info("[Config] Device pool (--r2l_device_pool): hard rays ranked by r2l_pool_select, jitter from Philox stream "
                    "2^61 + 4096 * iteration + %d of seed %d" % (rank, jitter_seed))
        if pool is not None and ckpt is not None and args.resume:
            if world > 1:
                logger.info("hard-ray pool: every rank has its own and rank 0 writes the checkpoint, so the pools of a multi-rank "
                            "run are not saved: they start empty after --resume")
            elif ckpt.get("r2l_hard_pool") is not None:
                pool.load_state_dict(ckpt["r2l_hard_pool"], device=device, batch_size=shards[rank] * loader.rows_per_file)
                logger.info("hard-ray pool: resumed with %d rows (full: %s, draw counter %d)" %
                            (0 if pool.pool is None else pool.pool.shape[0], pool.full, pool._draws))
            else:
                logger.info("hard-ray pool: the checkpoint carries none (written without --r2l_device_pool?): it starts empty")
    pool_extra = lambda: ({**({"r2l_hard_pool": pool.state_dict()} if save_pool else {}),
                           **({"r2l_ray_cull": ray_cull.state()} if ray_cull is not None else {})} or None)
    if args.r2l_fused_iter:
        # the whole iteration below — batch, pool rows, jitter, step, pool update — is one call of r2l_student_train_step
        logger.info("[Config] Fused iteration (--r2l_fused_iter): one library call per iteration, jitter from Philox stream "
                    "2^61 + 4096 * iteration + %d of seed %d" % (rank, jitter_seed))
    hist_psnr, t_data, t_batch = 0., 0., 0.
    logger.info("Begin training")
    for i in range(start + 1, args.N_iters + 1):
        t0 = time.time()
        lr = lr_schedule(i, args.lrate, args.lrate_decay, args.warmup_lr)
        if filler is not None and i % args.r2l_kd_every == 0:  # --r2l_kd_every: one more flush group of teacher frames
            filler.fill_group()
            logger.info("Iter %d ray store grew to %d shards (%d poses pending)" % (i, loader.n_shards, filler.pending))
            if filler.done:
                filler = None
        if args.r2l_fused_iter:  # one library call; the store's shard count of the moment goes into its descriptor
            _, loss_out = trainer.fused_step(loader, pool, lr, i, perturb=args.perturb, seed=jitter_seed, rank=rank)
        else:
            batch = loader.next()  # device tensor (shard reader: its H2D copy ran on the loader's stream during the last step)
            rays_o, rays_d, target = batch[:, :3], batch[:, 3:6], batch[:, 6:9]
            batch_size = rays_o.shape[0]
            if pool is not None:
                rays_o, rays_d, target = pool.augment(rays_o, rays_d, target)
            t_data = time.time() - t0
            n_global = None
            if uneven:  # this step's rays over all ranks: shard rows + what each rank's hard-ray pool appends (deterministic)
                rows = [q * loader.rows_per_file for q in shards]
                n_global = [r + (pool.extra_rays(r, i - start - 1) if pool is not None else 0) for r in rows]
                # the ray count PREDICTED for this rank is the weight its gradient gets: it must be the batch it really holds (a
                # shard with another row count, a pool that fills differently: silently wrong weights, and ranks that disagree
                # on the collective sequence — ADVICE r3)
                if rays_o.shape[0] != n_global[rank]:
                    raise RuntimeError("uneven --N_rand: rank %d holds %d rays in iteration %d, the share computed on every rank "
                                       "says %d (shards with differing row counts?)" % (rank, rays_o.shape[0], i, n_global[rank]))
            t_rand = None
            if args.r2l_device_pool and args.perturb > 0:  # (perturb 0: nothing is drawn)
                n = rays_o.shape[0]
                t_rand = draw_uniform(n * N_SAMPLE, jitter_seed, 2**61 + i * 4096 + rank, device).view(n, N_SAMPLE)
            rgb, loss_out = trainer.step(rays_o, rays_d, target, lr, perturb=args.perturb, t_rand=t_rand, n_global=n_global)
            if pool is not None:
                pool.update(rgb, rays_o, rays_d, target, batch_size)
        t_batch = time.time() - t0
        if i % args.i_print == 0:
            loss, psnr = loss_out.tolist()  # the only host sync of the loop, every i_print iterations
            hist_psnr = psnr if hist_psnr == 0. else hist_psnr * 0.95 + psnr * 0.05
            logger.info("[TRAIN] Iter %d data_time %.4f batch_time %.4f loss %.6f psnr %.4f hist_psnr %.4f LR %.10f" %
                        (i, t_data, t_batch, loss, psnr, hist_psnr, lr))
            # where the fp16 kernels stand with this model (include/r2l_hip.h range control): largest |activation| / |chain
            # gradient| of the last step, the power-of-two scales the streams run on, head-room to the guard, fallbacks so far
            ri = trainer.range_info()
            logger.info("[RANGE] Iter %d act_amax %.4g act_scale %g headroom x%.3g | grad_amax %.4g grad_scale %g headroom x%.3g | "
                        "fallbacks fwd %d bwd %d" % (i, ri["amax"], ri["scale"], ri["headroom"], ri.get("grad_amax", 0.),
                                                     ri.get("grad_scale", 1.), ri.get("grad_headroom", float("inf")),
                                                     ri["trips"], ri.get("bwd_trips", 0)))
        if i % args.i_testset == 0:
            savedir = os.path.join(logger.gen_img_path, "testset_%s_iter%d" % (logger.ExpID, i))
            os.makedirs(savedir, exist_ok=True)
            t_ = time.time()
            _, misc = render_path(test_poses, model, point_sampler, device, logger, gt_imgs=test_images,
                                  savedir=savedir, rank=rank, world=world, lpips_params=lpips_w, lpips_vgg_params=lpips_vgg_w,
                                  ray_cull=ray_cull)
            if misc["test_psnr_v2"] > best_psnr:
                best_psnr, best_psnr_step = misc["test_psnr_v2"].item(), i
                if rank == 0:
                    save_ckpt(os.path.join(logger.weights_path, "ckpt_best.tar"), i, model,
                              trainer.optimizer_state_dict(lr), best_psnr, best_psnr_step, r2l_config=r2l_config,
                              extra=pool_extra())
            logger.info("[TEST] Iter %d TestPSNR %.4f TestPSNRv2 %.4f TestSSIM %.4f%s TestFLIP %.4f BestPSNRv2 %.4f (Iter %d) "
                        "TrainHistPSNR %.4f LR %.8f Time %.1fs" %
                        (i, misc["test_psnr"].item(), misc["test_psnr_v2"].item(), misc["test_ssim"].item(), lpips_field(misc),
                         misc["test_flip"].item(), best_psnr, best_psnr_step, hist_psnr, lr, time.time() - t_))
        if i % args.i_video == 0:
            # test: using novel poses (main.py:1473-1484)
            logger.info("Iter %d Rendering video... (n_pose: %d)" % (i, len(video_poses)))
            t_ = time.time()
            rgbs, _ = render_path(video_poses, model, point_sampler, device, logger, rank=rank, world=world, ray_cull=ray_cull)
            path = save_video(rgbs, logger, logger.ExpID, i, args.video_tag, rank, world, device)
            if rank == 0:
                logger.info('Iter %d Save video: "%s" (time: %.2fs)' % (i, path, time.time() - t_))
        if i % args.i_weights == 0 and rank == 0:
            name = "ckpt_%d.tar" % i if args.save_intermediate_models else "ckpt.tar"
            path = save_ckpt(os.path.join(logger.weights_path, name), i, model, trainer.optimizer_state_dict(lr),
                             best_psnr, best_psnr_step, r2l_config=r2l_config, extra=pool_extra())
            logger.info('Iter %d Save checkpoint: "%s".' % (i, path))
    loader.close()
    if world > 1 and os.environ.get("R2L_CHECK_SYNC"):  # tests: the replicas must have stayed bit-identical
        from .dist_utils import parameters_in_sync
        ok = parameters_in_sync(trainer.eng.flat)
        logger.info("replicas in sync after %d iterations: %s (skipped steps: %d)" % (args.N_iters, ok, trainer.drain()))
        if not ok:
            raise RuntimeError("data-parallel replicas diverged")
    return {"trainer": trainer, "logger": logger, "model": model, "r2l_config": r2l_config, "loader": loader}
