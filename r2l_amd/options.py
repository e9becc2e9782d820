"""Command-line / config-file surface of the R2L drivers (main.py, utils/create_data.py).

Keeps the flag names, defaults and file syntax of the reference's option.py + smilelogging argparser
(/root/reference/option.py:6-358, smilelogging/__init__.py:8-42) for every flag that parameterises the hot path
(SURVEY.md appendix A): `--config file` with `key = value` lines (# comments, True/False for switches), command
line overrides the file, argparse prefix abbreviations work (README spells --num_worker), dotted `--trial.*`
flags fold into `args.trial` iff `--trial.ON` (slutils.py:176-188).  configargparse is not installed on the
target image, so this is a small table-driven parser of our own.
"""
import argparse
import glob
import os
import sys

from utils import EmptyClass

# name: (type | "flag", default)            -- "flag" = store_true switch
FLAGS = {
    # experiment bookkeeping (smilelogging argparser)
    "experiment_name": (str, ""), "experiments_dir": (str, "Experiments"), "debug": ("flag", False),
    "resume_TimeID": (str, ""),
    # data
    "expname": (str, None), "basedir": (str, "./logs/"), "datadir": (str, "./data/nerf_synthetic/lego"),
    "dataset_type": (str, "blender"), "testskip": (int, 8), "factor": (int, 8), "llffhold": (int, 8), "white_bkgd": ("flag", False), "half_res": ("flag", False),
    "datadir_kd": (str, ""), "data_mode": (str, "images"), "num_workers": (int, 8), "pseudo_ratio": (float, -1.),
    "pseudo_data_hold_ratio": (float, 0.), "i_update_data": (int, 1000000000), "focal_scale": (float, 1.),
    # networks
    "model_name": (str, "R2L"), "netdepth": (int, 8), "netwidth": (int, 256), "netdepth_fine": (int, 8),
    "netwidth_fine": (int, 256), "n_sample_per_ray": (int, 192), "multires": (int, 10), "multires_views": (int, 4),
    "i_embed": (int, 0), "use_viewdirs": ("flag", False), "use_residual": ("flag", False),
    "linear_tail": ("flag", False), "layerwise_netwidths": (str, ""), "act": (str, "relu"),
    "freeze_pretrained": ("flag", False),
    # rendering / sampling
    "N_samples": (int, 64), "N_importance": (int, 0), "perturb": (float, 1.), "perturb_test": (float, 0.),
    "raw_noise_std": (float, 0.), "chunk": (int, 1024 * 32), "netchunk": (int, 1024 * 64), "lindisp": ("flag", False),
    "no_ndc": ("flag", False), "render_only": ("flag", False), "render_test": ("flag", False),
    "render_factor": (float, 0), "n_pose_video": (str, "40"), "video_tag": (str, ""), "benchmark": ("flag", False),
    # optimisation
    "N_rand": (int, 32 * 32 * 4), "N_iters": (int, 200000), "lrate": (float, 5e-4), "lrate_decay": (int, 250),
    "warmup_lr": (str, ""), "lw_rgb": (float, 1.), "hard_ratio": (str, ""), "hard_mul": (float, 1.),
    "no_batching": ("flag", False), "precrop_iters": (int, 0), "precrop_frac": (float, .5),
    # checkpoints / logging cadence
    "pretrained_ckpt": (str, ""), "resume": ("flag", False), "test_pretrained": ("flag", False),
    "save_intermediate_models": ("flag", False), "i_print": (int, 100), "i_img": (int, 500), "i_weights": (int, 10000),
    "i_testset": (int, 2000), "i_video": (int, 10000), "no_reload": ("flag", False), "ft_path": (str, None),
    # teacher / pseudo-data generation (utils/create_data.py)
    "teacher_ckpt": (str, None), "test_teacher": ("flag", False), "create_data": (str, "spiral_evenly_spaced"),
    "n_pose_kd": (str, "100"), "create_data_chunk": (int, 100), "rm_existing_data": ("flag", False),
    "max_save": (int, 40000),
    # arithmetic of the HIP kernels (this build's own keys; include/r2l_hip.h r2l_config.precision / .dw_mode): which kernel
    # family every launch of the run uses.  auto = the library default (fp16x2 products, fp16 weight-gradient operands);
    # fp32_mfma = the reference's arithmetic (exact fp32 products and accumulation) — the graded numbers of bench.py
    "r2l_precision": (str, "auto"), "r2l_dw_mode": (str, "auto"),
    # teacher frames (create_data, the teacher's test render) through ONE library call per group of poses
    # (r2l_teacher_frames_cfg: rays, draws and all stages behind the C ABI) instead of render()'s per-pose assembly; opt-in
    "r2l_fused_frames": ("flag", False),
    # occupancy grid of the teacher's per-pose render (r2l_amd/occupancy.py; r2l_occ_build / r2l_occ_compact / r2l_occ_scatter):
    # the sample points in cells where the trained sigma is not positive skip the point network; opt-in.  r2l_occ_res: cells per
    # axis; r2l_occ_bound: half side of the cube about the origin, 0 = 0.625 (far - near), 2.5 for the Blender scenes.  Honoured by
    # utils/create_data.py --create_data rand, --test_teacher and main.py --model_name nerf --render_only; not with
    # --r2l_fused_frames / --r2l_online_kd (the frames call has no host read of the live count), --dataset_type llff (NDC space
    # needs its own box) or raw_noise_std > 0.  utils/train_nerf.py (but for r2l_occ_train below, which shares r2l_occ_res and
    # r2l_occ_bound) and student training ignore the three
    "r2l_occupancy": ("flag", False), "r2l_occ_res": (int, 128), "r2l_occ_bound": (float, 0.),
    # the same grids inside the FUSED frames call (r2l_teacher_frames_occ_cfg: the live count stays on the device, nothing is
    # read on the host): utils/create_data.py --create_data rand with --r2l_fused_frames or --r2l_store_save, --test_teacher and
    # main.py --model_name nerf --render_only with --r2l_fused_frames, main.py --r2l_online_kd.  Shares r2l_occ_res / r2l_occ_bound;
    # not together with --r2l_occupancy (the per-pose path), nor with llff or raw_noise_std > 0.  utils/train_nerf.py ignores it
    "r2l_occ_fused": ("flag", False),
    # whole rays that see only empty space are left out (r2l_occ_rays; r2l_amd/ray_cull.py): main.py culls EVERY student render of
    # the run (dead pixels get the background colour exactly) and, with r2l_online_kd and r2l_occ_fused, the rays of the store fill;
    # utils/create_data.py --r2l_store_save with r2l_occ_fused writes a culled store file.  The grid travels in every checkpoint
    # (key r2l_ray_cull); a later run takes it from --pretrained_ckpt, else builds it from --teacher_ckpt + --r2l_teacher_config.
    # GPU only; not with llff or r2l_compact_store.  A run with the switch is another run than one without.  utils/train_nerf.py
    # ignores it
    "r2l_ray_cull": ("flag", False),
    # early ray termination in the last pass of the FUSED frames call (r2l_teacher_frames_ert_cfg; r2l_amd/ert.py): the pass is walked
    # front to back in segments of r2l_ert_seg samples and a ray whose transmittance is below r2l_ert (0 = off, at most 0.1) at a
    # segment boundary leaves the segments behind it; a pixel moves by less than r2l_ert.  The paths of r2l_occ_fused, with it or
    # without; with --dataset_type llff only without it (no box is needed: the first way to skip samples in NDC space).  Not with
    # --r2l_occupancy, raw_noise_std > 0 or a teacher without view directions.  utils/train_nerf.py ignores both
    "r2l_ert": (float, 0.), "r2l_ert_seg": (int, 32),
    # the grids while the teacher TRAINS (utils/train_nerf.py only; r2l_teacher_mlp_train_live / r2l_teacher_backward_live /
    # r2l_teacher_train_step_occ): forward and backward of every step run on the live samples, the live counts stay on the device.
    # Shares r2l_occ_res / r2l_occ_bound; r2l_occ_every: a refresh of both grids from the current weights every so many iterations
    # (sigma threshold 0, one cell of dilation, the exact-fp32 kernels; 512: the smallest power of two at which two rebuilds of 128^3
    # cells cost at most 2 % of as many lego-size steps, profiles/teacher_occ_train.txt).  GPU only; not with llff or raw_noise_std > 0;
    # opt-in.
    # main.py / create_data.py ignore both
    "r2l_occ_train": ("flag", False), "r2l_occ_every": (int, 512),
    # device-resident ray store (r2l_amd/raystore.py): training draws its shards from HBM with one launch per step.
    # r2l_device_store: the shard files of --datadir_kd are read once into the store.  r2l_online_kd: no files at all, the
    # teacher (--teacher_ckpt, described by the config file --r2l_teacher_config) renders --n_pose_kd poses into the store, all
    # before iteration 1 (r2l_kd_every 0) or one flush group of --create_data_chunk poses every r2l_kd_every iterations
    "r2l_device_store": ("flag", False), "r2l_online_kd": ("flag", False), "r2l_teacher_config": (str, ""),
    "r2l_kd_every": (int, 0),
    # r2l_compact_store (with r2l_online_kd): the store keeps 16 bytes a ray — rgb and the ray's number in its flush group — and
    # recomputes o, d per draw from the group's poses (raystore.CompactRayStore, r2l_cstore_append / r2l_cstore_batch): the same
    # batches bit for bit in 4/9 of the memory.  Not with r2l_device_store (rows from files carry arbitrary rays) or
    # r2l_fused_iter (the one-call iteration reads 36-byte rows).  utils/create_data.py / utils/train_nerf.py ignore it
    "r2l_compact_store": ("flag", False),
    # a filled store as one checksummed file per rank (raystore.RayStore.save / load_store; INTEGRATION.md "store file"): render
    # once, train many times.  r2l_store_save (main.py with r2l_online_kd and r2l_kd_every 0: written once the fill is complete;
    # utils/create_data.py --create_data rand: the poses go into a store instead of shard files, compact with r2l_compact_store).
    # r2l_store_load: a third source of main.py's training beside r2l_online_kd and r2l_device_store; the kind comes from the
    # file.  The name is the path at world size 1, <path>.rank<r>of<w> otherwise.  utils/train_nerf.py ignores both
    "r2l_store_save": (str, ""), "r2l_store_load": (str, ""),
    # r2l_image_store: the store holds the REAL training rays of --datadir — the images and poses the loader already has, turned
    # into shuffled [o, d, rgb] rows on the device (r2l_amd/image_store.py, r2l_store_append_images): the fine-tuning stage
    # (README step 5) without the converter's files and without --datadir_kd.  With r2l_online_kd (r2l_kd_every 0) the real
    # group goes behind the teacher's groups: one store of real and pseudo rows.  Not with r2l_device_store / r2l_store_load
    # (one more source of rays), r2l_compact_store or r2l_kd_every > 0.  utils/create_data.py / utils/train_nerf.py ignore it
    "r2l_image_store": ("flag", False),
    # forward-facing LLFF scenes (--dataset_type llff: --factor, --llffhold, --no_ndc; NDC rays through r2l_ndc_rays); opt-in —
    # without the switch --dataset_type llff is refused as it always was.  configs/fern.txt and its kin carry it
    "r2l_llff": ("flag", False),
    # teacher training in the reference's batching mode (no --no_batching: every batch is N_rand pixels drawn without replacement
    # from all training images) through a pixel sampler on the device (r2l_amd/pixel_batch.py, r2l_pixel_batch); opt-in — without
    # the switch utils/train_nerf.py refuses a run without --no_batching as it always did.  main.py / create_data.py ignore it
    "r2l_batching": ("flag", False),
    # teacher training in images mode (--no_batching: one training image per iteration, N_rand distinct pixels of it, of its centre
    # crop for precrop_iters) through a pixel sampler on the device (r2l_amd/image_batch.py, r2l_image_batch) instead of
    # train_nerf.sample_batch on the host: the image and pixel choices are a keyed bijection's, not numpy's; opt-in — without the
    # switch, and without --no_batching, nothing changes.  main.py / create_data.py ignore it
    "r2l_image_sampler": ("flag", False),
    # teacher training with one library call per iteration (r2l_teacher_train_step): t_rand, u and the sigma noise are drawn on the
    # device from Philox streams of (R2L_SEED, iteration) instead of torch's generator, and the loop reads the loss only where it
    # prints, tests or ends; opt-in, GPU only.  main.py / create_data.py ignore it
    "r2l_fused_step": ("flag", False),
    # student training with the hard-ray pool's ranking inside the library (r2l_pool_select instead of a torch sort), the jitter
    # t_rand from Philox streams of (R2L_SEED, iteration, rank) instead of torch's generator, and — at world size 1 — the pool in
    # every checkpoint, so that --resume on a ray store repeats the uninterrupted run bit for bit; opt-in, GPU only.
    # utils/create_data.py / utils/train_nerf.py ignore it
    "r2l_device_pool": ("flag", False),
    # student training with one library call per iteration (r2l_student_train_step: batch from the ray store, pool rows, jitter,
    # forward, backward, Adam and the pool update behind the C ABI), bit for bit the --r2l_device_store --r2l_device_pool loop;
    # opt-in, one GPU, needs a ray store and, with --hard_ratio, --r2l_device_pool.  utils/create_data.py / utils/train_nerf.py
    # ignore it
    "r2l_fused_iter": ("flag", False),
    # LPIPS(AlexNet, v0.1) in the test-set loop (r2l_lpips): the user's weight file(s), one path or two joined by ':' (torchvision's
    # AlexNet checkpoint and the lpips package's alex.pth, or a saved lpips.LPIPS().state_dict(): metrics.lpips_params).  None are
    # shipped; '' = no LPIPS, every log line as it always was
    "r2l_lpips_weights": (str, ""),
    # LPIPS(VGG-16, v0.1) in the test-set loop (r2l_lpips_vgg), a switch of its own beside the one above (both may be given; --lpips_net
    # plays no part in it): one path or two joined by ':' (torchvision's VGG-16 checkpoint and the lpips package's vgg.pth, or a
    # saved lpips.LPIPS(net='vgg').state_dict(): metrics.lpips_vgg_params).  None are shipped; '' = no VGG work at all
    "r2l_lpips_vgg_weights": (str, ""),
    # pose refinement against a trained student (utils/refine_pose.py; r2l_amd/pose_refine.py, r2l_pose_refine_step): iterations,
    # pixels per view and iteration, the start — a file of poses [P,3,4] / [P,4,4], one per test view, or the true poses turned by
    # DEG degrees about a random axis and shifted by DIST in a random direction (seeded) —, Adam's two learning rates ROT,TRANS
    # and the .npy the refined poses go to ('' = refined_poses.npy in the experiment's log folder).  main.py,
    # utils/create_data.py and utils/train_nerf.py ignore them
    "r2l_pose_iters": (int, 200), "r2l_pose_rays": (int, 4096), "r2l_pose_init": (str, ""), "r2l_pose_noise": (str, "2,0.05"),
    "r2l_pose_lr": (str, "2e-3,5e-3"), "r2l_pose_out": (str, ""),
    # new-architecture switches (dotted group)
    "trial.ON": ("flag", False), "trial.body_arch": (str, "mlp"), "trial.res_scale": (float, 1.),
    "trial.n_learnable": (int, 2), "trial.inact": (str, "relu"), "trial.outact": (str, "none"),
    "trial.n_block": (int, -1), "trial.near": (float, -1.), "trial.far": (float, -1.),
}
CHOICES = {"r2l_precision": ["auto", "fp16x2", "bf16x3", "fp32_mfma"], "r2l_dw_mode": ["auto", "fp16", "exact"],
           "model_name": ["nerf", "nerf_v3.2", "R2L"], "data_mode": ["images", "rays"], "act": ["relu", "lrelu"],
           "trial.body_arch": ["mlp", "resmlp"], "trial.inact": ["none", "relu", "lrelu"],
           "trial.outact": ["none", "relu", "lrelu"]}
# flags of reference variants outside the accelerated path: accepted so old command lines / configs still parse
IGNORED = {"plucker": ("flag", False), "learn_depth": (str, ""), "shuffle_input": ("flag", False),
           "given_render_path_rays": (str, ""), "convert_to_onnx": ("flag", False), "lpips_net": (str, "alex"),
           "trans_origin": (str, ""), "select_pixel_mode": (str, "rand_pixel"),
           "spherify": ("flag", False), "shape": (str, "greek"), "lw_depth": (float, 0.1),
           "no_cache": ("flag", False), "no_scp": ("flag", False), "cache_code": (str, ""), "skips": (str, "4")}


def _build_parser():
    p = argparse.ArgumentParser(description="R2L on MI355X", allow_abbrev=True)
    p.add_argument("--config", type=str, default=None, help="config file: key = value per line")
    for table in (FLAGS, IGNORED):
        for name, (typ, default) in table.items():
            if typ == "flag":
                p.add_argument("--" + name, action="store_true", default=default)
            else:
                p.add_argument("--" + name, type=typ, default=default, choices=CHOICES.get(name))
    p.add_argument("--no_rand_focal", dest="use_rand_focal", action="store_false", default=True)
    return p


def read_config_file(path):
    """`key = value` lines -> argv-style list ('#' starts a comment; True/False toggle store_true switches)."""
    argv = []
    with open(path) as f:
        for line in f:
            line = line.split("#", 1)[0].strip()
            if not line or (line.startswith("[") and line.endswith("]")):  # blank / [section] headers are cosmetic
                continue
            if "=" in line:
                key, val = [s.strip() for s in line.split("=", 1)]
            else:
                key, val = line, "True"
            typ = (FLAGS.get(key) or IGNORED.get(key) or (str,))[0]
            if typ == "flag" or key == "no_rand_focal":
                if val.lower() in ("true", "1", "yes"):
                    argv.append("--" + key)
                elif val.lower() not in ("false", "0", "no"):
                    raise ValueError("%s: switch %s needs True/False, got %r" % (path, key, val))
            else:
                argv += ["--" + key, val]
    return argv


def check_path(pattern):
    """Expand a glob to exactly one existing path (smilelogging/utils.py:424-432 behaviour); '' stays ''."""
    if not pattern:
        return pattern
    hits = sorted(glob.glob(pattern))
    if len(hits) != 1:
        raise FileNotFoundError("%r matched %d paths (need exactly 1): %s" % (pattern, len(hits), hits[:5]))
    return hits[0]


def _n_pose(v):
    if v.lower() == "none":
        return None
    return int(v) if v.isdigit() else v.split(",")


def parse_args(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    p = _build_parser()
    pre, _ = p.parse_known_args(argv)
    if pre.config:
        argv = read_config_file(pre.config) + argv  # later (command-line) occurrences win
    args = p.parse_args(argv)
    # post-processing, as option.py:362-386
    if args.video_tag == "":
        args.video_tag = "pose%s" % args.n_pose_video
    args.n_pose_kd = _n_pose(args.n_pose_kd)
    args.n_pose_video = _n_pose(args.n_pose_video)
    args.pretrained_ckpt = check_path(args.pretrained_ckpt)
    if args.hard_ratio != "":
        hr = [float(x) for x in args.hard_ratio.split(",")]
        args.hard_ratio = hr[0] if len(hr) == 1 else hr
    # fold dotted groups: args.'trial.x' -> args.trial.x when trial.ON
    for key in [k for k in vars(args) if "." in k]:
        group, name = key.split(".")
        if getattr(args, group + ".ON"):
            if not hasattr(args, group):
                setattr(args, group, EmptyClass())
            setattr(getattr(args, group), name, getattr(args, key))
    for key in [k for k in vars(args) if "." in k]:
        delattr(args, key)
    return args


def validate_lpips(args):
    """--r2l_lpips_weights is the AlexNet variant only, --r2l_lpips_vgg_weights the VGG-16 one whatever --lpips_net says; the files
    must be there at start-up, not at the first evaluation hours into a run."""
    for part in (args.r2l_lpips_vgg_weights.split(":") if args.r2l_lpips_vgg_weights else ()):
        if not os.path.isfile(part):
            raise FileNotFoundError("--r2l_lpips_vgg_weights: no such file: %r" % part)
    if not args.r2l_lpips_weights:
        return
    if args.lpips_net != "alex":
        raise NotImplementedError("--r2l_lpips_weights evaluates LPIPS with the AlexNet features only (--lpips_net alex), got "
                                  "--lpips_net %s; the VGG-16 variant has its own switch, --r2l_lpips_vgg_weights" % args.lpips_net)
    for part in args.r2l_lpips_weights.split(":"):
        if not os.path.isfile(part):
            raise FileNotFoundError("--r2l_lpips_weights: no such file: %r" % part)


def validate_accelerated(args):
    """Fail loudly for reference variants this build does not accelerate (out of scope)."""
    validate_lpips(args)
    for name in ("plucker", "learn_depth", "shuffle_input", "given_render_path_rays", "convert_to_onnx"):
        if getattr(args, name):
            raise NotImplementedError("--%s is a reference variant outside the accelerated R2L path" % name)
    if args.dataset_type == "llff" and args.r2l_llff:
        if args.spherify:
            raise NotImplementedError("--spherify (360-degree LLFF captures) is outside the accelerated path")
        if args.lindisp:
            raise NotImplementedError("--lindisp is outside the accelerated path")
    elif args.dataset_type != "blender":
        raise NotImplementedError("only --dataset_type blender is on the accelerated path (got %s); --dataset_type llff needs "
                                  "the switch --r2l_llff (config key r2l_llff = True)" % args.dataset_type)
    validate_ray_store(args)


def validate_ray_store(args):
    """The ray-store flags name what they need: fail before anything is loaded."""
    if args.r2l_kd_every < 0:
        raise ValueError("--r2l_kd_every must be >= 0")
    if args.r2l_online_kd:
        for name in ("teacher_ckpt", "n_pose_kd", "r2l_teacher_config"):
            if not getattr(args, name):
                raise ValueError("--r2l_online_kd needs --%s" % name)
        if args.r2l_device_store:
            raise ValueError("--r2l_online_kd fills the store from the teacher, --r2l_device_store from files: give one of them")
    elif args.r2l_kd_every:
        raise ValueError("--r2l_kd_every needs --r2l_online_kd")
    if args.r2l_device_store and (args.data_mode != "rays" or not args.datadir_kd):
        raise ValueError("--r2l_device_store needs --data_mode rays and --datadir_kd")


def validate_occupancy(args, raw_noise_std=None):
    """--r2l_occupancy as the per-pose teacher renders take it (utils/create_data.py, main.py --model_name nerf --render_only;
    training entry points accept and ignore it).  raw_noise_std: the value the renders will run with (default: --raw_noise_std;
    the test renders pass 0).  Names the other flag, before anything is loaded."""
    if not args.r2l_occupancy:
        return
    for other in ("r2l_fused_frames", "r2l_online_kd"):
        if getattr(args, other):
            raise ValueError("--r2l_occupancy skips samples after a host read of the live count: not with --%s, whose frames call "
                             "enqueues every stage without one (--r2l_occ_fused skips inside that call, with the count left on the device)" % other)
    if args.dataset_type == "llff":
        raise ValueError("--r2l_occupancy puts its box about the origin of a bounded scene: not with --dataset_type llff (NDC "
                         "space needs a box of its own)")
    if (args.raw_noise_std if raw_noise_std is None else raw_noise_std) > 0:
        raise ValueError("--r2l_occupancy with raw_noise_std > 0: noise can lift a skipped sample above zero (pass "
                         "--raw_noise_std 0)")
    if not 1 <= args.r2l_occ_res <= 512:
        raise ValueError("--r2l_occ_res must be in 1 .. 512, got %d" % args.r2l_occ_res)
    if args.r2l_occ_bound < 0:
        raise ValueError("--r2l_occ_bound must be >= 0 (0: 0.625 (far - near)), got %g" % args.r2l_occ_bound)
    if not args.use_viewdirs:
        raise ValueError("--r2l_occupancy needs --use_viewdirs (the teacher kernels' network)")


OCC_EVERY_MAX = 1 << 30


def validate_occ_train(args, device_type=None):
    """--r2l_occ_train (utils/train_nerf.py only; the sibling entry points accept and ignore it): the occupancy grids inside the
    teacher's training step.  Names what is wrong before anything is loaded; device_type: where the run is, once known (the switch
    has no CPU form: a CPU run with it is refused, not trained without it)."""
    if not args.r2l_occ_train:
        return
    if args.raw_noise_std > 0:
        raise ValueError("--r2l_occ_train with raw_noise_std > 0: noise can lift a skipped sample above zero, and its gradient "
                         "with it (pass --raw_noise_std 0)")
    if args.dataset_type == "llff":
        raise ValueError("--r2l_occ_train puts its box about the origin of a bounded scene: not with --dataset_type llff (NDC "
                         "space needs a box of its own)")
    if not args.use_viewdirs:
        raise ValueError("--r2l_occ_train needs a teacher with --use_viewdirs (the teacher kernels' network)")
    if not 1 <= args.r2l_occ_res <= 512:
        raise ValueError("--r2l_occ_train: --r2l_occ_res must be in 1 .. 512, got %d" % args.r2l_occ_res)
    if args.r2l_occ_bound < 0:
        raise ValueError("--r2l_occ_train: --r2l_occ_bound must be >= 0 (0: 0.625 (far - near)), got %g" % args.r2l_occ_bound)
    if not 1 <= args.r2l_occ_every <= OCC_EVERY_MAX:
        raise ValueError("--r2l_occ_train: --r2l_occ_every must be in 1 .. 2^30 iterations, got %d" % args.r2l_occ_every)
    if device_type is not None and device_type != "cuda":
        raise ValueError("--r2l_occ_train runs the live kernels of libr2l_hip.so on a GPU; this run is on the CPU")


def occ_refresh_base(i, K):
    """The iteration whose weights the grids in force in iteration i >= 1 are built from: K * floor((i - 1) / K) — 0 stands for
    the weights a run starts from (the initial ones, or the checkpoint's for a run that starts there).  Pure: a resumed run and an
    uninterrupted one ask the same question."""
    if i < 1 or K < 1:
        raise ValueError("occ_refresh_base: need i >= 1 and K >= 1, got i = %d, K = %d" % (i, K))
    return K * ((i - 1) // K)


def validate_occ_fused(args, paths, raw_noise_std=None, use_viewdirs=None):
    """--r2l_occ_fused: the occupancy grids inside the fused frames call.  paths: the switches of this entry point that render
    through that call (one of them must be given).  raw_noise_std / use_viewdirs: the values of the TEACHER the frames come from
    (default: this namespace's; main.py --r2l_online_kd passes its teacher config's).  Names the other flag, before anything is
    loaded."""
    if not args.r2l_occ_fused:
        return
    if args.r2l_occupancy:
        raise ValueError("--r2l_occ_fused skips samples inside the fused frames call, --r2l_occupancy in the per-pose render: give "
                         "one of the two (not --r2l_occ_fused with --r2l_occupancy)")
    if not any(getattr(args, p) for p in paths):
        raise ValueError("--r2l_occ_fused acts inside the fused frames call: it needs %s (the per-pose renders take "
                         "--r2l_occupancy)" % " or ".join("--" + p for p in paths))
    if args.dataset_type == "llff":
        raise ValueError("--r2l_occ_fused puts its box about the origin of a bounded scene: not with --dataset_type llff (NDC "
                         "space needs a box of its own)")
    if (args.raw_noise_std if raw_noise_std is None else raw_noise_std) > 0:
        raise ValueError("--r2l_occ_fused with raw_noise_std > 0: noise can lift a skipped sample above zero (pass "
                         "--raw_noise_std 0)")
    if not 1 <= args.r2l_occ_res <= 512:
        raise ValueError("--r2l_occ_fused: --r2l_occ_res must be in 1 .. 512, got %d" % args.r2l_occ_res)
    if args.r2l_occ_bound < 0:
        raise ValueError("--r2l_occ_fused: --r2l_occ_bound must be >= 0 (0: 0.625 (far - near)), got %g" % args.r2l_occ_bound)
    if not (args.use_viewdirs if use_viewdirs is None else use_viewdirs):
        raise ValueError("--r2l_occ_fused needs a teacher with --use_viewdirs (the teacher kernels' network)")


def validate_ray_cull(args, device_type=None, entry="main", ckpt_has_grid=None):
    """--r2l_ray_cull as main.py (entry 'main') and utils/create_data.py (entry 'create_data') take it; utils/train_nerf.py accepts
    and ignores it.  Names the flag, before anything is loaded.  device_type: where the run is, once known (a CPU run is refused, not
    rendered without culling).  ckpt_has_grid: once --pretrained_ckpt is read (main.py), whether it carries the key r2l_ray_cull —
    without it the grid is built from the teacher, which then must be named."""
    if not args.r2l_ray_cull:
        return
    if args.dataset_type == "llff":
        raise ValueError("--r2l_ray_cull asks a grid whose box sits about the origin of a bounded scene: not with --dataset_type llff "
                         "(NDC space needs a box of its own)")
    if args.r2l_compact_store:
        raise ValueError("--r2l_ray_cull: not with --r2l_compact_store, whose rows keep a ray's number in its flush group (a culled "
                         "compact store would need an id variant of its own)")
    if device_type is not None and device_type != "cuda":
        raise ValueError("--r2l_ray_cull runs r2l_occ_rays of libr2l_hip.so on a GPU; this run is on the CPU")
    if not 1 <= args.r2l_occ_res <= 512:
        raise ValueError("--r2l_ray_cull: --r2l_occ_res must be in 1 .. 512, got %d" % args.r2l_occ_res)
    if args.r2l_occ_bound < 0:
        raise ValueError("--r2l_ray_cull: --r2l_occ_bound must be >= 0 (0: 0.625 (far - near)), got %g" % args.r2l_occ_bound)
    if entry == "create_data":
        if not (args.r2l_store_save and args.r2l_occ_fused):
            raise ValueError("--r2l_ray_cull in utils/create_data.py culls the store fill: it needs --r2l_store_save and "
                             "--r2l_occ_fused (the grids are built there)")
        return
    if args.model_name == "nerf":
        raise ValueError("--r2l_ray_cull culls the STUDENT's renders and its store: not with --model_name nerf (with grids the "
                         "teacher's dead rays already cost only the floor)")
    if args.r2l_online_kd and not args.r2l_occ_fused:
        raise ValueError("--r2l_ray_cull culls the fill of --r2l_online_kd with the grids of --r2l_occ_fused: give that switch too")
    if ckpt_has_grid is False and not (args.teacher_ckpt and args.r2l_teacher_config):
        raise ValueError("--r2l_ray_cull needs a grid: either --pretrained_ckpt names a checkpoint of a run with the switch (it "
                         "carries the key r2l_ray_cull), or --teacher_ckpt and --r2l_teacher_config name the teacher to build it from")


def validate_ert(args, paths, raw_noise_std=None, use_viewdirs=None):
    """--r2l_ert EPS / --r2l_ert_seg W: early ray termination in the last pass of the fused frames call.  Arguments as
    validate_occ_fused's; returns (eps, seg), or None with the switch off.  Names the flag, before anything is loaded."""
    if args.r2l_ert == 0:
        return None
    if not 0. < args.r2l_ert <= 0.1:
        raise ValueError("--r2l_ert must be in (0, 0.1] (0: off), got %g" % args.r2l_ert)
    if args.r2l_ert_seg < 8:
        raise ValueError("--r2l_ert_seg must be >= 8, got %d" % args.r2l_ert_seg)
    if args.r2l_occupancy:
        raise ValueError("--r2l_ert acts inside the fused frames call, --r2l_occupancy in the per-pose render: not --r2l_ert with "
                         "--r2l_occupancy (--r2l_occ_fused is the grids' switch of that call)")
    if not any(getattr(args, p) for p in paths):
        raise ValueError("--r2l_ert acts inside the fused frames call: it needs %s" % " or ".join("--" + p for p in paths))
    if (args.raw_noise_std if raw_noise_std is None else raw_noise_std) > 0:
        raise ValueError("--r2l_ert with raw_noise_std > 0: the transmittance of the walk is that of the noiseless sigma (pass "
                         "--raw_noise_std 0)")
    if not (args.use_viewdirs if use_viewdirs is None else use_viewdirs):
        raise ValueError("--r2l_ert needs a teacher with --use_viewdirs (the teacher kernels' network)")
    return float(args.r2l_ert), int(args.r2l_ert_seg)


def validate_compact_store(args):
    """--r2l_compact_store (main.py only; the sibling entry points accept and ignore it): the 16-bytes-a-ray store recomputes the
    rays of teacher frames, so it needs the teacher fill and excludes what reads other rows.  Names the other flag."""
    if not args.r2l_compact_store:
        return
    if args.r2l_device_store:
        raise ValueError("--r2l_compact_store recomputes the rays of teacher frames: not with --r2l_device_store, whose rows "
                         "come from files and carry arbitrary rays")
    if args.r2l_fused_iter:
        raise ValueError("--r2l_compact_store hands out batches through its own kernel: not with --r2l_fused_iter, which reads "
                         "the 36-byte rows of the plain store")
    if not args.r2l_online_kd:
        raise ValueError("--r2l_compact_store needs --r2l_online_kd (the teacher fills the store)")


def validate_image_store(args):
    """--r2l_image_store (main.py only; the sibling entry points accept and ignore it): the real training rays as a flush group
    of a plain store, alone or behind the teacher's groups.  Names the other flag, before anything is loaded."""
    if not args.r2l_image_store:
        return
    for other in ("r2l_device_store", "r2l_store_load"):
        if getattr(args, other):
            raise ValueError("--r2l_image_store fills the store from the training images of --datadir: not with --%s (--r2l_online_kd "
                             "may fill the same store; a third source of rays may not: give one)" % other)
    if args.r2l_compact_store:
        raise ValueError("--r2l_image_store writes plain 36-byte rows: not with --r2l_compact_store, whose rows carry the rays of "
                         "teacher frames")
    if args.r2l_kd_every > 0:
        raise ValueError("--r2l_image_store appends the real rays behind a COMPLETE teacher fill: not with --r2l_kd_every %d (give "
                         "--r2l_kd_every 0)" % args.r2l_kd_every)


def validate_store_file(args):
    """--r2l_store_save / --r2l_store_load as main.py takes them (utils/create_data.py has its own use of --r2l_store_save,
    utils/train_nerf.py ignores both).  Names the other flag, before anything is loaded."""
    if args.r2l_store_load:
        for other in ("r2l_online_kd", "r2l_device_store", "r2l_kd_every", "r2l_store_save"):
            if getattr(args, other):
                raise ValueError("--r2l_store_load takes the store from a file: not with --%s (one source of rays per run, and a "
                                 "loaded store is not saved again)" % other)
    if args.r2l_store_save:
        if not (args.r2l_online_kd or args.r2l_image_store):
            raise ValueError("--r2l_store_save writes the store the teacher fills: it needs --r2l_online_kd (or "
                             "utils/create_data.py --create_data rand, which renders into a store and writes the file)")
        if args.r2l_kd_every > 0:
            raise ValueError("--r2l_store_save writes the complete store before iteration 1: not with --r2l_kd_every %d, a store "
                             "that grows during training has no single content" % args.r2l_kd_every)


def validate_fused_iter(args, world=1, device_type="cuda"):
    """--r2l_fused_iter (main.py only): the student's iteration as one library call draws its batch from a ray store and moves
    the pool's rows itself, on one GPU.  Names what is missing before anything is loaded."""
    if not args.r2l_fused_iter:
        return
    if not (args.r2l_device_store or args.r2l_online_kd or args.r2l_store_load or args.r2l_image_store):
        raise ValueError("--r2l_fused_iter draws its batches from a ray store: it needs --r2l_device_store or --r2l_online_kd")
    if args.hard_ratio and not args.r2l_device_pool:
        raise ValueError("--r2l_fused_iter with --hard_ratio needs --r2l_device_pool (the hard rays are ranked inside the call)")
    if device_type != "cuda":
        raise NotImplementedError("--r2l_fused_iter runs r2l_student_train_step of libr2l_hip.so on a GPU; this run is on the CPU")
    if world != 1:
        raise NotImplementedError("--r2l_fused_iter runs at world size 1 (the gradient all-reduce of a data-parallel step sits "
                                  "inside the call's sequence); this run has %d ranks" % world)


def parse_teacher_config(path, teacher_ckpt=None):
    """--r2l_teacher_config: the teacher's own config file (e.g. configs/lego.txt) as a second namespace — the student's config
    does not describe the teacher (use_viewdirs, N_samples, N_importance, perturb, white_bkgd).  The refusals of the fused
    frames path apply: lindisp, raw_noise_std > 0 and a teacher without view directions raise NotImplementedError."""
    targs = parse_args(["--config", path])
    if targs.lindisp or targs.raw_noise_std or not targs.use_viewdirs:
        raise NotImplementedError("%s: the ray store is filled through the fused frames path: lindisp, raw_noise_std > 0 and "
                                  "use_viewdirs=False are outside it (a config with raw_noise_std > 0, such as the LLFF ones: "
                                  "copy it with raw_noise_std = 0)" % path)
    if teacher_ckpt is not None:
        targs.teacher_ckpt = teacher_ckpt
    return targs
