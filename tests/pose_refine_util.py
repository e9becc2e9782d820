"""Shared by tests/test_pose_refine_cpu.py and tests/test_pose_refine_gpu.py: the localisation scenario and small helpers.

The scenario.  A smooth analytic light field — the colour of a ray is a product of low-frequency sines of its intersection with the
plane z = 0 — fitted by a W256 student with one ResMLP block (600 Adam steps of 4096 rays, origins around (0, 0, 4), near 2,
far 6).  The fitted weights are the fixture tests/golden/pose_refine_student.npz (fp16: 0.75 MB; the student IS the rounded
weights), written by `python -m tests.pose_refine_util` (17 s on 16 CPU threads).  The observed image is 64 x 64 at focal 80,
rendered by the student itself at the true pose, and the refinement starts 2 degrees and 0.05 away."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "pose_refine_student.npz")
H = W = 64
FOCAL = 80.0
NEAR, FAR, N_SAMPLE = 2.0, 6.0, 16
N_RAYS, ITERS = 1024, 100
START_DEG, START_DIST = 2.0, 0.05
FIT_STEPS, FIT_RAYS, FIT_SEED = 600, 4096, 11


def field(o, d):
    """Colour [N,3] in (0, 1) of the rays (o, d): sines of the point where the ray meets z = 0."""
    s = -o[:, 2] / d[:, 2]
    x, y = o[:, 0] + s * d[:, 0], o[:, 1] + s * d[:, 1]
    return torch.stack([0.5 + 0.4 * torch.sin(1.7 * x + 0.3) * torch.sin(1.3 * y - 0.2),
                        0.5 + 0.4 * torch.sin(1.1 * x - 0.7) * torch.sin(2.1 * y + 0.5),
                        0.5 + 0.4 * torch.sin(2.3 * x + 1.1) * torch.sin(0.9 * y + 0.9)], -1)


def true_pose():
    """A camera at (0, 0, 4) looking down -z: [1,3,4]."""
    return torch.tensor([[[1., 0., 0., 0.], [0., 1., 0., 0.], [0., 0., 1., 4.]]])


def fit_rays(n, g):
    """Training rays: origins around (0, 0, 4), directions of a camera turned a few degrees, over a little more than the frame."""
    o = torch.tensor([0., 0., 4.]) + 0.15 * torch.randn(n, 3, generator=g)
    d = torch.cat([(torch.rand(n, 2, generator=g) - 0.5) * 1.1, -torch.ones(n, 1)], -1)
    w = 0.06 * torch.randn(n, 3, generator=g)  # a small rotation of each direction
    return o, d + torch.cross(w, d, dim=-1)


def make_model(n_block=1, device="cpu", state=None):
    import argparse
    from model.nerf_raybased import NeRF_v3_2
    trial = argparse.Namespace(ON=True, body_arch="resmlp", inact="relu", outact="none", res_scale=1., n_learnable=2,
                               n_block=-1, near=-1, far=-1)
    args = argparse.Namespace(netdepth=2 * n_block + 2, netwidth=256, layerwise_netwidths="", act="relu", linear_tail=False,
                              use_residual=True, trial=trial)
    m = NeRF_v3_2(args, 1008, 3)
    if state is not None:
        m.load_state_dict(state)
    return m.to(device)


def sampler(device="cpu", h=H, w=W, focal=FOCAL):
    from model.nerf_raybased import PointSampler
    return PointSampler(h, w, focal, N_SAMPLE, NEAR, FAR, device=device)


def fit_student(steps=FIT_STEPS, log=None):
    """The fit of the scenario on the CPU: the state dict, rounded to fp16."""
    torch.manual_seed(FIT_SEED)
    g = torch.Generator().manual_seed(FIT_SEED)
    m, ps = make_model(), sampler()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.1**(1.0 / steps))
    for i in range(steps):
        o, d = fit_rays(FIT_RAYS, g)
        loss = ((m.forward_rays(o, d, ps) - field(o, d))**2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        sched.step()
        if log is not None and (i % 100 == 0 or i == steps - 1):
            log("fit step %d: mse %.3e" % (i, loss.item()))
    return {k: v.detach().half() for k, v in m.state_dict().items()}


def load_student(device="cpu", dtype=torch.float32):
    """The fitted student of the fixture, frozen."""
    z = np.load(FIXTURE)
    m = make_model(state={k: torch.from_numpy(z[k].astype(np.float32)) for k in z.files}, device=device).to(dtype)
    for p in m.parameters():
        p.requires_grad_(False)
    return m


def observed(model, ps, poses):
    """images [P,H,W,3]: the student's own renders at `poses`, fp32 on the model's device."""
    with torch.no_grad():
        return torch.stack([model.render_pose(c, ps).float().reshape(ps.H, ps.W, 3) for c in poses], 0)


def start_poses(P=1):
    """The true pose P times, and ONE start START_DEG / START_DIST away from it, P times (the poses of a batch still draw different
    pixels).  The start is the second of perturb_poses(.., seed=5) for four poses.  A plane seen almost head-on leaves a valley — a
    turn about an axis in the plane against a shift along the other — along which Adam at the default rates needs more than the
    100 iterations of the scenario: the first, third and fourth start of that seed stand at 0.07 / 0.06 / 0.9 degrees and 0.006 /
    0.005 / 0.07 after 100 iterations, at 3e-4 / 3e-4 / 0.55 degrees after 200 and at 2e-6 / 2e-6 / 0.02 degrees after 300
    (measured on the CPU restatement); the second, with little of that component, is at 0.006 degrees and 4e-4 after 100."""
    from r2l_amd.pose_refine import perturb_poses
    true = true_pose().expand(P, 3, 4).contiguous()
    one = perturb_poses(true_pose().expand(4, 3, 4), START_DEG, START_DIST, seed=5)[1:2]
    return true, one.expand(P, 3, 4).contiguous()


def rotations(P, seed, dtype=torch.float64):
    """P random rotations, orthonormal to the precision of `dtype`."""
    g = torch.Generator().manual_seed(seed)
    q, r = torch.linalg.qr(torch.randn(P, 3, 3, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r, dim1=-2, dim2=-1))[:, None, :]
    q[:, :, 2] *= torch.linalg.det(q)[:, None]
    return q.to(dtype)


def skew(w):
    K = torch.zeros(w.shape[0], 3, 3, dtype=w.dtype)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    return K


if __name__ == "__main__":
    sd = fit_student(log=print)
    np.savez(FIXTURE, **{k: v.numpy() for k, v in sd.items()})
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")
