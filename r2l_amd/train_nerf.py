"""Step 1 of the pipeline: train the NeRF teacher, the `python main.py --model_name nerf --config configs/lego.txt` command of
the reference (main.py:1199-1513, images mode with no_batching), here `python utils/train_nerf.py --config configs/lego.txt`.

Each iteration draws one training image (np.random.choice(i_train)), centre-crops it for precrop_iters, takes N_rand of its
pixels without replacement (rand_pixel, helpers:385-392) and runs one TeacherTrainer step (r2l_amd/teacher_train.py) at the
learning rate of lr_schedule.  The numpy and torch generators are re-seeded from (R2L_SEED, iteration) at every iteration, so a
run is reproducible and a --resume from a checkpoint of iteration k continues exactly as the uninterrupted run would.
With --r2l_batching and no --no_batching the run is the reference's batching mode (main.py:1137-1162, 1199-1210) instead:
iteration i takes draws (i-1)*N_rand .. i*N_rand - 1 of the pixel sampler of r2l_amd/pixel_batch.py, seeded with R2L_SEED — N_rand
pixels of all training images, without replacement inside an epoch, no centre crop.  Two differences from the reference: every
batch has N_rand rays (one that reaches the end of an epoch goes on with the first draws of the next; the reference hands out one
short batch, then reshuffles), and the permutation is the keyed bijection of csrc/r2l_perm.h, not numpy's.  The sampler has no
state, so --resume seeks to start*N_rand and continues bit for bit.
With --r2l_fused_step (GPU only) an iteration is ONE library call, TeacherTrainer.fused_step: the same kernels in the same order, but
t_rand, u and the sigma noise of raw_noise_std come from the Philox streams 2^62 + 4*i + k of R2L_SEED (include/r2l_hip.h) instead of
torch's generator, and the loss stays on the device: the host reads it where it prints, tests and ends, never per iteration.  The
step has no state, so --resume continues bit for bit; batching mode then skips the per-iteration re-seeding (nothing there draws
from the host generators), images mode keeps it for its numpy pixel choice.
With --r2l_image_sampler and --no_batching the batch of images mode comes from the device too (r2l_amd/image_batch.py): iteration i
takes image image_draw(R2L_SEED, i, n_train) and N_rand distinct pixels of its centre crop (i < precrop_iters) or of the whole frame,
one r2l_image_batch launch in place of sample_batch, device_rays and four copies.  The image and pixel choices are the keyed
bijection's, not numpy's; the distribution is the reference's.  An N_rand above the crop's (or the frame's) pixel count is refused
at start-up, where the reference would fail inside numpy at the first iteration.  With --r2l_fused_step no host generator is left
in the loop, the re-seeding is skipped, and --resume is exact with no sampler state; the staged step keeps it for torch's draws.
With --r2l_occ_train (GPU only, raw_noise_std 0) forward and backward of every step run on the samples that are live in an occupancy grid
per net (r2l_amd/occupancy.py TrainOccupancy; TeacherTrainer.set_occupancy): the grids in force in iteration i are built from the
weights after iteration K * floor((i - 1) / K), K = --r2l_occ_every, and every checkpoint carries them under a key of its own
('r2l_occ_train', which the reference's loaders never read), so that --resume repeats the uninterrupted run — bit for bit under
--r2l_fused_step --r2l_image_sampler.
Checkpoints are the reference's layout (checkpoint.save_ckpt, model_name='nerf'): utils/create_data.py --teacher_ckpt and
main.py --model_name nerf --render_only read them unchanged.
"""
import os
import time

import numpy as np
import torch

from . import data as D
from .checkpoint import load_ckpt, save_ckpt
from .driver import lpips_field, apply_arithmetic, create_nerf_teacher, init_distributed, load_lpips_vgg_weights, load_lpips_weights, render_path
from .image_batch import ImageBatcher, crop_window, full_window
from .logger import Logger
from .occupancy import TrainOccupancy
from .options import parse_args, validate_accelerated, validate_occ_train
from .pixel_batch import PixelBatcher
from .render import get_rays, ndc_rays
from .teacher_train import MAX_SAMPLES, TeacherTrainer
from .train_step import lr_schedule


def validate_teacher_training(args):
    """Loud refusals for what this path does not implement."""
    validate_accelerated(args)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise NotImplementedError("teacher training runs on one GPU (WORLD_SIZE > 1 is not supported)")
    if not args.no_batching and not args.r2l_batching:
        raise NotImplementedError("teacher training implements images mode with --no_batching; use_batching, the reference's "
                                  "default, needs the switch --r2l_batching (config key r2l_batching = True)")
    if args.r2l_precision not in ("auto", "fp32_mfma"):
        raise NotImplementedError("teacher training is exact fp32 (--r2l_precision auto | fp32_mfma), got %s" % args.r2l_precision)
    if not args.use_viewdirs or args.N_importance < 0:
        raise NotImplementedError("teacher training implements NeRF(D=8, W=256, 63+27, skips=[4], use_viewdirs)")
    S = args.N_samples + max(args.N_importance, 0)
    if S > MAX_SAMPLES:
        raise NotImplementedError("teacher training takes at most %d samples per ray (N_samples + N_importance), got %d"
                                  % (MAX_SAMPLES, S))


def precrop_coords(H, W, frac):
    """[2dH, 2dW, 2] pixel coordinates of the centre crop (main.py:1273-1284)."""
    dH, dW = int(H // 2 * frac), int(W // 2 * frac)
    return torch.stack(torch.meshgrid(torch.linspace(H // 2 - dH, H // 2 + dH - 1, 2 * dH),
                                      torch.linspace(W // 2 - dW, W // 2 + dW - 1, 2 * dW), indexing="ij"), -1)


def full_coords(H, W):
    return torch.stack(torch.meshgrid(torch.linspace(0, H - 1, H), torch.linspace(0, W - 1, W), indexing="ij"), -1)


def select_rand_pixels(coords, N_rand):
    """get_selected_coords(coords, N_rand, 'rand_pixel') (helpers:385-392): N_rand distinct pixels."""
    coords = coords.long()
    H, W = coords.shape[:2]
    rand_ix = np.random.choice(H * W, size=[N_rand], replace=False)
    return coords.view(-1, 2)[rand_ix]


def sample_batch(i, args, images, poses, i_train, H, W, focal):
    """(rays_o, rays_d, viewdirs, target) of iteration i (main.py:1260-1302)."""
    img_i = np.random.choice(i_train)
    target = images[img_i]
    pose = poses[img_i, :3, :4]
    rays_o, rays_d = get_rays(H, W, focal, torch.as_tensor(pose, dtype=torch.float32))
    coords = precrop_coords(H, W, args.precrop_frac) if i < args.precrop_iters else full_coords(H, W)
    sel = select_rand_pixels(coords, args.N_rand)
    rays_o, rays_d = rays_o[sel[:, 0], sel[:, 1]], rays_d[sel[:, 0], sel[:, 1]]
    target = torch.as_tensor(target)[sel[:, 0], sel[:, 1]]
    viewdirs = rays_d / torch.norm(rays_d, dim=-1, keepdim=True)
    return rays_o, rays_d, viewdirs, target


def device_rays(rays_o, rays_d, H, W, focal, ndc, device):
    """The selected rays on `device` as the step takes them: NDC scenes (main.py:1303-1306 -> render(ndc=True)) put them through
    ndc_rays at near plane 1 there; the view directions stay those of the world rays."""
    rays_o, rays_d = rays_o.to(device), rays_d.to(device)
    if ndc:
        rays_o, rays_d = ndc_rays(H, W, focal, 1., rays_o, rays_d)
    return rays_o, rays_d


def _seed(i):
    s = (int(os.environ.get("R2L_SEED", "0")) * 1000003 + i) % (2**32)
    np.random.seed(s)
    torch.manual_seed(s)


def main(argv=None):
    args = parse_args(argv)
    args.model_name = "nerf"
    validate_occ_train(args, None)  # (the switch's own refusals first: they name it; the device is checked below)
    validate_teacher_training(args)
    rank, world, device = init_distributed()
    validate_occ_train(args, device.type)
    if args.r2l_fused_step and device.type != "cuda":
        raise NotImplementedError("--r2l_fused_step runs on the GPU only (r2l_teacher_train_step of libr2l_hip.so); this run is on "
                                  "device '%s'" % device)
    _seed(0)
    logger = Logger(args, rank)
    lpips_w = load_lpips_weights(args, device, logger)  # (read once; None without --r2l_lpips_weights)
    lpips_vgg_w = load_lpips_vgg_weights(args, device, logger)  # (None without --r2l_lpips_vgg_weights)
    scene = D.load_scene(args)
    images, poses, hwf = scene.images, scene.poses, scene.hwf
    logger.info("Loaded %s" % scene.kind, tuple(images.shape), tuple(poses.shape), hwf, args.datadir)
    i_train, i_test = scene.i_train, scene.i_test
    near, far = scene.near, scene.far
    images = scene.rgb_images(args.white_bkgd)
    H, W, focal = int(hwf[0]), int(hwf[1]), float(hwf[2])

    kwargs_test = create_nerf_teacher(args, device, logger, near, far, ndc=scene.ndc)
    coarse, fine = kwargs_test["network_fn"], kwargs_test["network_fine"]
    for net in (coarse, fine):
        if net is not None:
            net.train()
            for p in net.parameters():
                p.requires_grad = device.type != "cuda"  # the device path computes its gradients by hand
    r2l_config = apply_arithmetic(args, device, logger, teachers=(coarse, fine))
    trainer = TeacherTrainer(coarse, fine, N_samples=args.N_samples, N_importance=args.N_importance, perturb=args.perturb,
                             white_bkgd=args.white_bkgd, raw_noise_std=args.raw_noise_std)
    start, best_psnr, best_psnr_step = 0, 0., 0
    occ_state = None
    if args.pretrained_ckpt and args.resume:
        ckpt = load_ckpt(args.pretrained_ckpt, map_location=device)
        start = int(ckpt["global_step"])
        best_psnr, best_psnr_step = float(ckpt.get("best_psnr", 0.)), int(ckpt.get("best_psnr_step", 0))
        trainer.load_optimizer_state_dict(ckpt["optimizer_state_dict"])
        occ_state = ckpt.get(TrainOccupancy.KEY)
        logger.info("Resume from %s at iteration %d" % (args.pretrained_ckpt, start))
    teacher = dict(hwf=(H, W, focal), chunk=args.chunk, render_kwargs=kwargs_test, render_factor=0)
    test_poses, test_images = poses[i_test], images[i_test]

    occ = None
    if args.r2l_occ_train:
        occ = TrainOccupancy(args, coarse, fine, near, far, trainer, logger, start=start, state=occ_state)

    def save(path, i, lr):
        return save_ckpt(path, i, coarse, trainer.optimizer_state_dict(lr), best_psnr, best_psnr_step, model_name="nerf",
                         model_fine=fine, r2l_config=r2l_config, extra={TrainOccupancy.KEY: occ.state()} if occ is not None else None)

    batcher = None
    if not args.no_batching:  # (validate_teacher_training: only with --r2l_batching)
        batcher = PixelBatcher(torch.as_tensor(images[i_train]), poses[i_train], H, W, focal, scene.ndc, device,
                               seed=int(os.environ.get("R2L_SEED", "0")))
        batcher.seek(start * args.N_rand)
        logger.info("[Config] Batching mode (--r2l_batching): N_rand %d of M = %s; draw %d, in epoch %d" %
                    (args.N_rand, batcher.describe(), batcher.draw, batcher.epoch()))
        if args.precrop_iters > 0:
            logger.info("[Config] precrop_iters = %d is ignored: batching mode has no centre crop" % args.precrop_iters)

    sampler = None
    if args.no_batching and args.r2l_image_sampler:  # (in batching mode the switch changes nothing)
        crop, frame = crop_window(H, W, args.precrop_frac), full_window(H, W)
        if start + 1 < args.precrop_iters and args.N_rand > crop[2] * crop[3]:
            raise ValueError("--r2l_image_sampler: N_rand %d exceeds the %d x %d = %d pixels of the centre crop (precrop_frac %g of "
                             "%d x %d, until iteration %d): a batch is N_rand DISTINCT pixels of one image; lower N_rand or raise "
                             "precrop_frac" % (args.N_rand, crop[2], crop[3], crop[2] * crop[3], args.precrop_frac, H, W,
                                               args.precrop_iters))
        if args.N_rand > H * W:
            raise ValueError("--r2l_image_sampler: N_rand %d exceeds the %d x %d = %d pixels of a frame: a batch is N_rand DISTINCT "
                             "pixels of one image (precrop_frac plays no part here); lower N_rand" % (args.N_rand, H, W, H * W))
        sampler = ImageBatcher(torch.as_tensor(images[i_train]), poses[i_train], H, W, focal, scene.ndc, device,
                               seed=int(os.environ.get("R2L_SEED", "0")))
        logger.info("[Config] Images mode through the device pixel sampler (--r2l_image_sampler): per iteration one r2l_image_batch "
                    "launch, N_rand %d distinct pixels of one of %s; image and pixels are a pure function of (seed %d, iteration), "
                    "not numpy's choices" % (args.N_rand, sampler.describe(), sampler.seed))

    fused = bool(args.r2l_fused_step)
    if fused:
        seed = int(os.environ.get("R2L_SEED", "0"))
        n_left = max(args.N_iters - start, 0)
        loss_hist = torch.zeros(n_left, 2, dtype=torch.float32, device=device)  # [loss, psnr] per iteration; read where printed
        logger.info("[Config] Fused step (--r2l_fused_step): one r2l_teacher_train_step call per iteration; t_rand, u and the sigma "
                    "noise are the Philox streams 2^62 + 4*iter + k of seed %d (r2l_draw_uniform / r2l_draw_normal), not torch's "
                    "generator; the loss is read at i_print, i_testset and the end" % seed)
    else:
        logger.info("[Config] Staged step: TeacherTrainer.step, the draws are torch's generator, re-seeded per iteration")

    history, lr, t0 = [], args.lrate, time.time()
    for i in range(start + 1, args.N_iters + 1):
        if not (fused and (batcher is not None or sampler is not None)):
            _seed(i)
        lr = lr_schedule(i, args.lrate, args.lrate_decay, args.warmup_lr)
        if batcher is not None:
            a = batcher.draw
            rays_o, rays_d, viewdirs, target = batcher.next(args.N_rand)
            for e in range(-(-a // batcher.M), (batcher.draw - 1) // batcher.M + 1):  # the epochs whose first draw is in this batch
                logger.info("[TRAIN] Iter %d: epoch %d begins (draw %d)" % (i, e, e * batcher.M))
        elif sampler is not None:
            rays_o, rays_d, viewdirs, target = sampler.next(i, args.N_rand, crop if i < args.precrop_iters else frame)
            if i == start + 1 and i < args.precrop_iters:
                logger.info("[Config] Center cropping of size %d x %d is enabled until iter %d" % (crop[2], crop[3], args.precrop_iters))
        else:
            rays_o, rays_d, viewdirs, target = sample_batch(i, args, images, poses, i_train, H, W, focal)
            if i == start + 1 and i < args.precrop_iters:
                dH, dW = int(H // 2 * args.precrop_frac), int(W // 2 * args.precrop_frac)
                logger.info("[Config] Center cropping of size %d x %d is enabled until iter %d" % (2 * dH, 2 * dW, args.precrop_iters))
            rays_o, rays_d = device_rays(rays_o, rays_d, H, W, focal, scene.ndc, device)
            viewdirs, target = viewdirs.to(device), target.to(device)
        if fused:
            trainer.fused_step(rays_o, rays_d, viewdirs, near, far, target, lr, step=i, seed=seed, loss_out=loss_hist[i - start - 1])
            if i % args.i_print == 0 or (i % args.i_testset == 0 and len(i_test)):
                loss, psnr = loss_hist[i - start - 1].tolist()
        else:
            loss, psnr = trainer.step(rays_o, rays_d, viewdirs, near, far, target, lr)
            history.append((loss, psnr))
        if occ is not None:
            occ.after_step(i)  # (before any checkpoint of iteration i: it carries the grids of iteration i + 1)
        if i % args.i_print == 0:
            logger.info("[TRAIN] Iter %d Loss %.4f PSNR %.4f LR %.8f Time %.1fs" % (i, loss, psnr, lr, time.time() - t0))
        if i % args.i_testset == 0 and len(i_test):
            savedir = os.path.join(logger.gen_img_path, "testset_%s_iter%d" % (logger.ExpID, i))
            _, misc = render_path(test_poses, coarse, None, device, logger, gt_imgs=test_images, savedir=savedir,
                                  teacher=teacher, lpips_params=lpips_w, lpips_vgg_params=lpips_vgg_w)
            for net in (coarse, fine):
                if net is not None:
                    net.train()
            if misc["test_psnr_v2"].item() > best_psnr:
                best_psnr, best_psnr_step = misc["test_psnr_v2"].item(), i
                save(os.path.join(logger.weights_path, "ckpt_best.tar"), i, lr)
            logger.info("[TEST] Iter %d TestPSNR %.4f TestPSNRv2 %.4f%s BestPSNRv2 %.4f (Iter %d)" %
                        (i, misc["test_psnr"].item(), misc["test_psnr_v2"].item(), lpips_field(misc), best_psnr, best_psnr_step))
        if i % args.i_weights == 0:
            name = "ckpt_%d.tar" % i if args.save_intermediate_models else "ckpt.tar"
            path = save(os.path.join(logger.weights_path, name), i, lr)
            logger.info('Iter %d Save checkpoint: "%s".' % (i, path))
    if fused:
        history = [tuple(row) for row in loss_hist.tolist()]
    return {"trainer": trainer, "logger": logger, "history": history, "coarse": coarse, "fine": fine,
            "r2l_config": r2l_config, "batcher": batcher, "image_sampler": sampler, "occupancy": occ}
