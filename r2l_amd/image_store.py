"""The scene's REAL training rays in a device-resident RayStore (r2l_amd/raystore.py) — the fine-tuning stage (README steps 4 and
5) without utils/convert_original_data_to_rays_*.py and its `train_<k>.npy` files.

The converters compute get_rays of every training frame on the host, shuffle all pixels and write [4096,9] shards; those rows are
a pure function of the images and poses data.load_scene already holds.  fill_store_from_images appends them as ONE flush group
(RayStore.append_images -> r2l_store_append_images: one launch, rays in r2l_frame_rays' arithmetic), so the shuffle is global over
all training pixels as the converter's is — another order (the keyed bijection of csrc/r2l_perm.h, not numpy's permutation), the
same distribution: every training pixel at most once per epoch, fewer than one shard of them dropped.

The group's key is epoch_key(R2L_SEED, IMAGE_GROUP): a pure function of the seed, the same on every rank.  At world size > 1
every rank builds the same permuted sequence and keeps shards rank, rank + world, ... of it: disjoint, a pure function of
(seed, rank, world)."""
import os

import torch

from .keyed_perm import epoch_key

RAYS_PER_SHARD = 4096
IMAGE_GROUP = 0x696D616765  # "image": the epoch number the real group's key is derived with (no sampler epoch gets near it)


def image_group_key(seed=None):
    """Key of the real rays' flush group: epoch_key(R2L_SEED, IMAGE_GROUP)."""
    return epoch_key(int(os.environ.get("R2L_SEED", "0")) if seed is None else int(seed), IMAGE_GROUP)


def training_frames(scene, white_bkgd):
    """(images [K, H, W, 3] fp32, c2ws [K, 3, 4] fp32) of the scene's training split, as data.load_scene loaded it: blender frames
    composited on white with --white_bkgd, at --half_res if asked for; LLFF frames at --factor, held-out views excluded."""
    idx = torch.as_tensor(scene.i_train, dtype=torch.long)
    images = torch.as_tensor(scene.rgb_images(white_bkgd), dtype=torch.float32)[idx].contiguous()
    c2ws = torch.as_tensor(scene.poses, dtype=torch.float32)[idx][:, :3, :4].contiguous()
    return images, c2ws


def image_shards(n_frames, H, W, rank=0, world=1, rays_per_shard=RAYS_PER_SHARD):
    """(shards the whole group gives, shards rank `rank` of `world` keeps: rank, rank + world, ... of them)."""
    m = int(n_frames) * int(H) * int(W) // int(rays_per_shard)
    return m, len(range(rank, m, world))


def plan_image_store(args, n_frames, H, W, rank, world, logger=None):
    """What --r2l_image_store will put into this rank's store, from the options and the training split's size alone: logs it
    and raises ValueError when the store would hold fewer shards than one step of this rank draws.  Returns {'real': this
    rank's real shards, 'teacher': its teacher shards (--r2l_online_kd, else 0), 'all_real': the whole group's}."""
    from .dist_utils import split_shards
    from .online_kd import shards_needed
    m_all, m_mine = image_shards(n_frames, H, W, rank, world)
    teacher = 0
    if args.r2l_online_kd:
        n_pose = args.n_pose_kd if isinstance(args.n_pose_kd, int) else int(args.n_pose_kd[0])
        teacher = shards_needed(n_pose, args.create_data_chunk, H, W, rank, world)
    try:
        need = split_shards(args.N_rand, world)[rank]
    except ValueError:
        need = 0  # (an --N_rand the rank count cannot split: the driver turns it away itself)
    if m_mine + teacher < need:
        raise ValueError("--r2l_image_store: %d training frames of %d x %d give %d shards of %d real rays (%d on rank %d of %d)%s, one "
                         "step of this rank draws %d (--N_rand %d over %d ranks)" %
                         (n_frames, H, W, m_all, RAYS_PER_SHARD, m_mine, rank, world,
                          " behind %d teacher shards of --r2l_online_kd" % teacher if args.r2l_online_kd else "", need, args.N_rand, world))
    if logger is not None:
        logger.info("image store (--r2l_image_store): the %d training frames of --datadir at %d x %d = %d real rays -> %d shards of "
                    "%d rays in device memory (%.3f GB at 36 B a ray)%s" %
                    (n_frames, H, W, n_frames * H * W, m_all, RAYS_PER_SHARD, m_all * RAYS_PER_SHARD * 36 / 1e9,
                     "" if world == 1 else "; rank %d of %d keeps %d" % (rank, world, m_mine)))
    return {"real": m_mine, "teacher": teacher, "all_real": m_all}


def fill_store_from_images(store, images, c2ws, focal, rank=0, world=1, seed=None, logger=None):
    """Append the real rays of `images` [K, H, W, 3] under `c2ws` [K, 3|4, 4] and `focal` (a number, or [K]) to `store` as one
    flush group shuffled by image_group_key(seed); at world > 1 the rank's shards rank::world of the permuted sequence.  Images on
    the CPU are moved to the store's device first.  Returns the number of shards appended."""
    K, H, W = images.shape[:3]
    m_all, m_mine = image_shards(K, H, W, rank, world, store.rows_per_file)
    if store.n_shards + m_mine > store.capacity:
        raise ValueError("fill_store_from_images: %d shards do not fit behind %d in a store of %d" % (m_mine, store.n_shards, store.capacity))
    key = image_group_key(seed)
    images = images.to(store.device)
    if torch.is_tensor(focal):
        focal = focal.to(store.device)
    if world == 1:
        m = store.append_images(images, c2ws, focal, key, shuffle=True)
    else:
        from .raystore import RayStore
        m = 0
        if m_mine:
            whole = RayStore(m_all, store.device, rays_per_shard=store.rows_per_file)  # the sequence every rank builds
            whole.append_images(images, c2ws, focal, key, shuffle=True)
            m = store.append(whole.shards()[rank::world].reshape(-1, 9), 0, shuffle=False)
            whole.close()  # (freed behind the copy: the allocator is stream-ordered)
    if logger is not None:
        logger.info("image store: %d training frames of %d x %d = %d real rays as one flush group, %d shards of %d rays%s (%d "
                    "rays of the shuffled sequence dropped); no shard file was opened" %
                    (K, H, W, K * H * W, m_all, store.rows_per_file,
                     "" if world == 1 else ", rank %d of %d keeps %d of them" % (rank, world, m), K * H * W - m_all * store.rows_per_file))
    return m
