"""Refine camera poses against a trained R2L student (utils/refine_pose.py; r2l_amd/pose_refine.py, r2l_pose_refine_step):

  python utils/refine_pose.py --config configs/lego_noview.txt --pretrained_ckpt <student.tar> \\
      --r2l_pose_iters 200 --r2l_pose_rays 4096 [--r2l_pose_init poses.npy | --r2l_pose_noise DEG,DIST] \\
      [--r2l_pose_lr ROT,TRANS] [--r2l_pose_out refined.npy] [--r2l_precision ...]

The held-out test views of the scene are the queries, as many per launch as keep P * rays at most 98 304.  They start from
--r2l_pose_init ([P,3,4] or [P,4,4], one pose per test view) or from the true poses turned by DEG degrees about a random axis and
shifted by DIST in a random direction (seeded; default 2,0.05), are refined for --r2l_pose_iters iterations of --r2l_pose_rays
pixels each, and are written as one .npy [P,3,4].  Where the true poses are known — always, for a scene's test views — the
rotation and translation error of every view is logged before and after, with medians.  LLFF scenes work as they are: the student
takes world rays, frames need not be square, and no NDC is involved."""
import os

import numpy as np
import torch

from . import data as D
from .driver import apply_arithmetic, create_r2l, init_distributed
from .logger import Logger
from .nerf_raybased import PointSampler
from .options import parse_args, validate_accelerated
from .pose_refine import R2L_SEED, PoseRefiner, perturb_poses, pose_errors

MAX_RAYS_PER_LAUNCH = 98304  # where a step's kernels are at their most efficient


def _pair(text, what):
    try:
        a, b = (float(x) for x in str(text).split(","))
    except ValueError:
        raise ValueError("%s takes two numbers joined by a comma, got %r" % (what, text))
    return a, b


def load_init(path, n_views):
    """--r2l_pose_init: [P,3,4] or [P,4,4] with one pose per query view -> [P,3,4] fp32."""
    poses = np.load(path)
    if poses.ndim != 3 or tuple(poses.shape[1:]) not in ((3, 4), (4, 4)):
        raise ValueError("--r2l_pose_init %s: need poses [P,3,4] or [P,4,4], got shape %s" % (path, tuple(poses.shape)))
    if poses.shape[0] != n_views:
        raise ValueError("--r2l_pose_init %s: %d poses for %d query views" % (path, poses.shape[0], n_views))
    return torch.from_numpy(np.ascontiguousarray(poses[:, :3, :4], dtype=np.float32))


def main(argv=None):
    args = parse_args(argv)
    validate_accelerated(args)
    if args.r2l_pose_iters < 1:
        raise ValueError("--r2l_pose_iters must be >= 1")
    lr_rot, lr_trans = _pair(args.r2l_pose_lr, "--r2l_pose_lr")
    deg, dist = _pair(args.r2l_pose_noise, "--r2l_pose_noise")
    _, _, device = init_distributed()
    seed = int(os.environ.get("R2L_SEED", str(R2L_SEED)))
    torch.manual_seed(0)
    logger = Logger(args, 0)
    scene = D.load_scene(args)
    hwf = scene.hwf
    H, W, focal = int(hwf[0]), int(hwf[1]), float(hwf[2])
    if args.focal_scale > 0:
        focal *= args.focal_scale
    near, far = scene.near, scene.far
    if hasattr(args, "trial") and args.trial.near > 0:
        near, far = args.trial.near, args.trial.far
    n = int(args.r2l_pose_rays)
    if not 1 <= n <= H * W:
        raise ValueError("--r2l_pose_rays %d is outside 1 .. H*W = %d x %d = %d: an iteration takes DISTINCT pixels of a view" %
                         (n, H, W, H * W))
    i_test = np.asarray(scene.i_test)
    images = torch.as_tensor(np.asarray(scene.rgb_images(args.white_bkgd)[i_test]), dtype=torch.float32)
    true = torch.as_tensor(np.asarray(scene.poses[i_test]), dtype=torch.float32)[:, :3, :4]
    if args.r2l_pose_init:
        init = load_init(args.r2l_pose_init, len(i_test))
    else:
        init = perturb_poses(true, deg, dist, seed=seed)
    logger.info("Loaded %s: %d query views %d x %d, focal %.3f; start: %s" % (
        scene.kind, len(i_test), H, W, focal,
        args.r2l_pose_init or "true poses turned by %g degrees and shifted by %g (seed %d)" % (deg, dist, seed)))

    model, _, _, _ = create_r2l(args, device, logger)
    for p in model.parameters():
        p.requires_grad_(False)
    ps = PointSampler(H, W, focal, args.n_sample_per_ray, near, far, device=device)
    apply_arithmetic(args, device, logger, student=model)

    per = max(1, MAX_RAYS_PER_LAUNCH // n)
    refined, losses = [], []
    for a in range(0, len(i_test), per):
        r = PoseRefiner(model, ps, images[a:a + per], init[a:a + per], n, lr_rot=lr_rot, lr_trans=lr_trans, seed=seed)
        refined.append(r.run(args.r2l_pose_iters, fused=True).detach().cpu())
        losses.append(r.losses.detach().cpu())
        logger.info("[POSE] views %d .. %d: %d iterations of %d rays each; mean loss %.3e -> %.3e" % (
            a, min(a + per, len(i_test)) - 1, args.r2l_pose_iters, n, losses[-1][0].mean().item(), losses[-1][-1].mean().item()))
    refined = torch.cat(refined, 0)
    rot0, tr0 = pose_errors(init, true)
    rot1, tr1 = pose_errors(refined, true)
    for k in range(len(i_test)):
        logger.info("[POSE] view %d (image %d of the scene): rotation %.4f -> %.4f degrees, translation %.5f -> %.5f" % (
            k, int(i_test[k]), rot0[k].item(), rot1[k].item(), tr0[k].item(), tr1[k].item()))
    logger.info("[POSE] rotation error before %.4f after %.4f degrees (medians over %d views)" % (
        rot0.median().item(), rot1.median().item(), len(i_test)))
    logger.info("[POSE] translation error before %.5f after %.5f (medians over %d views)" % (
        tr0.median().item(), tr1.median().item(), len(i_test)))
    out = args.r2l_pose_out or os.path.join(logger.log_path, "refined_poses.npy")
    np.save(out, refined.numpy())
    logger.info('[POSE] wrote %d refined poses [P,3,4] to "%s"' % (refined.shape[0], out))
    return {"poses": refined, "init": init, "true": true, "losses": torch.cat(losses, 1), "errors": (rot0, tr0, rot1, tr1),
            "out": out, "logger": logger}


if __name__ == "__main__":
    main()
