"""Generate tests/golden/llff.npz by running the REFERENCE's LLFF data layer on a tiny synthetic scene (dev container only).

    python tests/golden/gen_golden_llff.py       # needs /root/reference; writes tests/golden/llff.npz

As gen_golden.py: the reference never travels to the GPU box, only this small data file does (the scene's inputs + the
reference's outputs).  dataset/load_llff.py imports imageio (absent here: a stub backed by PIL's reader) and visualize_3d
(matplotlib PDFs, a side effect: stubbed); it runs in a temporary working directory.
"""
import io
import os
import sys
import tempfile
import types

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
N_VIEWS, H, W, FACTOR = 9, 12, 16, 2


def synthetic_scene(seed=1):
    """(poses_bounds [9,17], images [9,12,16,3] uint8, images_2 [9,6,8,3] uint8): cameras looking down -z, rotations <= 0.35 rad
    about a random axis, centres within +-1 (z within +-0.3), bounds in [1.5, 9]."""
    rng = np.random.RandomState(seed)
    rows = []
    for _ in range(N_VIEWS):
        axis = rng.randn(3)
        axis /= np.linalg.norm(axis)
        ang = rng.uniform(-.35, .35)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)  # columns: right, up, back
        pos = rng.uniform(-1, 1, 3) * np.array([1., 1., .3])
        # LLFF's stored column order is [down, right, back, position, (H, W, focal)]
        m = np.stack([-R[:, 1], R[:, 0], R[:, 2], pos, np.array([H, W, 20.])], 1)
        near = rng.uniform(1.5, 3.)
        rows.append(np.concatenate([m.reshape(-1), [near, rng.uniform(near + 1., 9.)]]))
    imgs = rng.randint(0, 256, size=(N_VIEWS, H, W, 3)).astype(np.uint8)
    imgs2 = rng.randint(0, 256, size=(N_VIEWS, H // FACTOR, W // FACTOR, 3)).astype(np.uint8)
    return np.stack(rows).astype(np.float64), imgs, imgs2


def write_scene(basedir, poses_bounds, imgs, imgs2):
    from PIL import Image
    np.save(os.path.join(basedir, "poses_bounds.npy"), poses_bounds)
    for name, stack in (("images", imgs), ("images_%d" % FACTOR, imgs2)):
        os.makedirs(os.path.join(basedir, name), exist_ok=True)
        for i, im in enumerate(stack):
            Image.fromarray(im).save(os.path.join(basedir, name, "view_%02d.png" % i))


def import_reference_llff():
    assert os.path.isdir(REF), "reference not mounted"
    sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") != os.path.abspath(os.path.join(OUT, "..", ".."))]
    sys.path.insert(0, REF)
    from PIL import Image
    m = types.ModuleType("imageio")
    m.imread = lambda f, **kw: np.asarray(Image.open(f))
    sys.modules["imageio"] = m
    import utils.run_nerf_raybased_helpers as rh
    assert rh.__file__.startswith(REF)
    torch.autograd.set_detect_anomaly(False)
    rh.visualize_3d = lambda *a, **k: None
    import dataset.load_llff as ll
    assert ll.__file__.startswith(REF)
    return rh, ll


def main():
    rh, ll = import_reference_llff()
    poses_bounds, imgs, imgs2 = synthetic_scene()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            scene = os.path.join(tmp, "scene")
            os.makedirs(scene)
            write_scene(scene, poses_bounds, imgs, imgs2)
            images, poses, bds, render_poses, i_test = ll.load_llff_data(scene, factor=FACTOR, recenter=True, bd_factor=.75,
                                                                        spherify=False, n_pose_video=8)
            np.random.seed(3)
            rand_poses = np.stack([ll.get_rand_pose_v2().cpu().numpy() for _ in range(3)])
        finally:
            os.chdir(cwd)
    images, poses, bds, render_poses = (t.cpu().numpy() for t in (images, poses, bds, render_poses))
    # ndc_rays on the frame of view 0, fp32 on the CPU, focal as an fp32 tensor (as hwf is in the reference's LLFF drivers)
    h, w, focal = int(poses[0, 0, 4]), int(poses[0, 1, 4]), torch.tensor(poses[0, 2, 4])
    ro, rd = rh.get_rays(h, w, focal, torch.from_numpy(poses[0, :3, :4]).to(rh.device))
    no, nd = rh.ndc_rays(h, w, focal, 1., ro, rd)
    buf = io.BytesIO()
    np.savez_compressed(buf, poses_bounds=poses_bounds, imgs=imgs, imgs2=imgs2, factor=FACTOR, n_pose_video=8, images=images,
                        poses=poses, bds=bds, render_poses=render_poses, i_test=int(i_test), rand_poses=rand_poses,
                        rays_o=ro.cpu().numpy(), rays_d=rd.cpu().numpy(), ndc_o=no.cpu().numpy(), ndc_d=nd.cpu().numpy())
    with open(os.path.join(OUT, "llff.npz"), "wb") as f:
        f.write(buf.getvalue())
    print("tests/golden/llff.npz: %d B; poses %s render_poses %s i_test %d" % (len(buf.getvalue()), poses.shape, render_poses.shape,
                                                                              int(i_test)))


if __name__ == "__main__":
    main()
