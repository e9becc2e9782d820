"""Camera-pose refinement against a trained R2L student (include/r2l_hip.h "pose refinement"; csrc/r2l_pose.hip).

P observed images, P pose estimates.  Iteration i >= 1 takes n pixels of every image — pose p the positions
perm(pose_key(seed, i, p), H*W)[0 .. n) of its frame, the keyed bijection of csrc/r2l_perm.h, so they are distinct —, forms their
world rays under the current estimates, renders them with the frozen student, and moves every pose down the gradient of ITS mean
squared error:

    grad[p][0:3] = sum_j rays_d x d_rays_d        the derivative with respect to w at 0 of  R <- exp([w]x) R  (about the camera centre)
    grad[p][3:6] = sum_j d_rays_o                 the derivative with respect to v at 0 of  t <- t + v
    delta        = Adam's update of a zero 6-vector (lr_rot for w, lr_trans for v),  R <- exp([dw]x) R,  one Gram-Schmidt pass,  t += dv

pose_ids, pose_batch_spec, pose_grad_spec, pose_update_spec and refine_step_spec restate the stages in torch, in the dtype of their
inputs; they are the specification the tests hold the kernels to and the meaning of the CPU path, where the student is the plain
module and autograd gives the ray gradients.  On a ROCm device PoseRefiner.step() makes the library calls one by one and
fused_step() is r2l_pose_refine_step, the same kernels in one call; the two agree bit for bit.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import ptr as _ptr, stream as _stream
from .keyed_perm import M64, epoch_key, perm_at

POSE_SALT = 0x706F73655F726566  # "pose_ref"
R2L_SEED = 0x52324C  # "R2L": the default seed of the pixel choice
SERIES_THETA2 = 1e-4  # Rodrigues' coefficients by their series below this squared angle


def pose_key(seed, iteration, p):
    """What r2l_pose_key writes: the key of pose p's pixel bijection at iteration >= 1."""
    iteration, p = int(iteration), int(p)
    if iteration < 1 or p < 0:
        raise ValueError("pose_key: need iteration >= 1 and p >= 0, got %d and %d" % (iteration, p))
    return epoch_key(epoch_key((int(seed) & M64) ^ POSE_SALT, iteration), p)


def pose_ids(seed, iteration, P, n, H, W):
    """Pixel ids of an iteration (what r2l_pose_batch writes to ids_out): int64[P*n], (p*H + row)*W + col."""
    P, n, H, W = int(P), int(n), int(H), int(W)
    if not 0 <= n <= H * W:
        raise ValueError("pose_ids: %d rays from a frame of %d x %d pixels" % (n, H, W))
    out = np.empty(P * n, dtype=np.int64)
    for p in range(P):
        out[p * n:(p + 1) * n] = p * H * W + perm_at(pose_key(seed, iteration, p), H * W, np.arange(n, dtype=np.uint64))
    return out


def pose_batch_spec(images, poses, H, W, focal, seed, iteration, n):
    """(rays_o, rays_d, target, ids) of an iteration on CPU tensors, rays and target [P*n,3] fp32: pixel_ray of
    csrc/r2l_pixel_ray.h at pose_ids, every operation separately rounded (raystore.pixel_ray_spec)."""
    from .raystore import pixel_ray_spec
    images = torch.as_tensor(images, dtype=torch.float32).cpu()
    poses = np.asarray(torch.as_tensor(poses, dtype=torch.float32).cpu()[:, :3, :4].contiguous().numpy(), dtype=np.float32)
    P = poses.shape[0]
    ids = pose_ids(seed, iteration, P, n, H, W)
    img, pix = ids // (H * W), ids % (H * W)
    o, d = pixel_ray_spec(poses[img], np.full(ids.shape[0], focal, dtype=np.float32), H, W, pix // W, pix % W)
    return (torch.from_numpy(np.ascontiguousarray(o, dtype=np.float32)), torch.from_numpy(np.ascontiguousarray(d, dtype=np.float32)),
            images.reshape(-1, 3)[torch.from_numpy(ids)], ids)


def pose_grad_spec(rays_d, d_rays_o, d_rays_d, rgb, target, P, n):
    """(grad [P,6], loss [P]) in the dtype of rays_d (r2l_pose_grad up to the order of its sums)."""
    dt = rays_d.dtype
    seg = lambda x: x.to(dt).reshape(P, n, 3)
    rot = torch.cross(seg(rays_d), seg(d_rays_d), dim=-1).sum(1)
    loss = ((seg(rgb) - seg(target))**2).sum((1, 2)) / torch.tensor(3.0 * n, dtype=torch.float32).to(dt)
    return torch.cat([rot, seg(d_rays_o).sum(1)], -1), loss


def _cross_rows(w, r):
    """w [P,3] x every column of r [P,3,3] -> [P,3,3]."""
    return torch.cross(w[:, :, None].expand_as(r), r, dim=1)


def pose_update_spec(c2w, exp_avg, exp_avg_sq, grad, lr_rot, lr_trans, beta1, beta2, eps, step):
    """(c2w', exp_avg', exp_avg_sq') of r2l_pose_update in the dtype of c2w; the inputs are left alone.  The scalars enter with
    the values given (a test that compares with the fp32 kernel passes fp32-representable ones)."""
    dt = c2w.dtype
    g, m, v = grad.to(dt), exp_avg.to(dt), exp_avg_sq.to(dt)
    ok = torch.isfinite(g).all(-1)
    g0 = torch.where(ok[:, None], g, torch.zeros_like(g))
    m1 = m + (g0 - m) * (1 - beta1)
    v1 = v * beta2 + (g0 * g0) * (1 - beta2)
    bc1, bc2 = 1 - beta1**step, 1 - beta2**step
    lr = torch.tensor([lr_rot] * 3 + [lr_trans] * 3, dtype=dt, device=c2w.device)
    delta = -((lr / bc1) * (m1 / (v1.sqrt() / bc2**0.5 + eps)))
    w, dv = delta[:, :3], delta[:, 3:]
    R, t = c2w[:, :3, :3], c2w[:, :3, 3]
    th2 = (w * w).sum(-1)
    th = th2.sqrt()
    small = th2 < SERIES_THETA2
    ths = torch.where(small, torch.ones_like(th), th)  # (no 0 / 0 on the branch not taken)
    sh, ch = torch.sin(0.5 * ths), torch.cos(0.5 * ths)
    A = torch.where(small, 1 - th2 * (1 / 6 - th2 * (1 / 120)), 2 * sh * ch / ths)
    B = torch.where(small, 0.5 - th2 * (1 / 24 - th2 * (1 / 720)), 2 * sh * sh / (ths * ths))
    k1 = _cross_rows(w, R)
    k2 = _cross_rows(w, k1)
    Rn = R + A[:, None, None] * k1 + B[:, None, None] * k2
    cols = []
    for c in range(3):  # modified Gram-Schmidt over the columns 0, 1, 2
        x = Rn[:, :, c]
        for q in cols:
            x = x - (q * x).sum(-1, keepdim=True) * q
        cols.append(x / x.norm(dim=-1, keepdim=True))
    Rn = torch.stack(cols, -1)
    moved = ok & (w != 0).any(-1)  # dw == 0: R keeps its bits (the Gram-Schmidt pass belongs to the rotation)
    Rn = torch.where(moved[:, None, None], Rn, R)
    tn = torch.where(ok[:, None], t + dv, t)
    keep = lambda new, old: torch.where(ok[:, None], new, old)
    return torch.cat([Rn, tn[:, :, None]], -1), keep(m1, m), keep(v1, v)


def student_rgb_spec(model, point_sampler, rays_o, rays_d):
    """The plain module on explicit rays at the test-time depths (perturb 0), in the dtype of the rays."""
    from .nerf_raybased import PositionalEmbedder
    from .engine import L_PE
    z = point_sampler.z_vals.to(rays_o.dtype).to(rays_o.device)
    pts = (rays_o[:, None, :] + rays_d[:, None, :] * z[None, :, None]).reshape(rays_o.shape[0], -1)
    return model._forward_torch(PositionalEmbedder(L_PE, device=rays_o.device)(pts))


def refine_step_spec(model, point_sampler, images, c2w, exp_avg, exp_avg_sq, H, W, focal, seed, iteration, n, lr_rot, lr_trans,
                     beta1, beta2, eps):
    """One whole iteration on CPU tensors in the dtype of c2w (the model's parameters must have it): (c2w', exp_avg', exp_avg_sq',
    loss [P], parts) — parts holds the rays, rgb, the ray gradients and grad, for tests."""
    dt, P = c2w.dtype, c2w.shape[0]
    if dt == torch.float32:
        o, d, target, ids = pose_batch_spec(images, c2w, H, W, focal, seed, iteration, n)
    else:  # the same pixels, the rays in the wider type
        ids = pose_ids(seed, iteration, P, n, H, W)
        gi = torch.from_numpy(ids)
        img, pix = gi // (H * W), gi % (H * W)
        row, col = torch.div(pix, W, rounding_mode="floor"), pix % W
        dirs = torch.stack([(col.to(dt) - W * .5) / focal, -((row.to(dt) - H * .5) / focal), -torch.ones(gi.shape[0], dtype=dt)], -1)
        o, d = c2w[img, :3, 3], (dirs[:, None, :] * c2w[img, :3, :3]).sum(-1)
        target = torch.as_tensor(images).to(dt).reshape(-1, 3)[gi]
    o, d = o.detach().clone().requires_grad_(True), d.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        rgb = student_rgb_spec(model, point_sampler, o, d)
        total = (((rgb - target.to(dt))**2).reshape(P, n * 3).sum(-1) / (3.0 * n)).sum()
        d_o, d_d = torch.autograd.grad(total, (o, d))
    grad, loss = pose_grad_spec(d.detach(), d_o, d_d, rgb.detach(), target, P, n)
    c2w1, m1, v1 = pose_update_spec(c2w, exp_avg, exp_avg_sq, grad, lr_rot, lr_trans, beta1, beta2, eps, iteration)
    parts = dict(rays_o=o.detach(), rays_d=d.detach(), target=target, rgb=rgb.detach(), d_rays_o=d_o, d_rays_d=d_d, grad=grad, ids=ids)
    return c2w1, m1, v1, loss, parts


def rotation_angle_deg(Ra, Rb):
    """Angle in degrees between rotations [P,3,3], in fp64 from the Frobenius norm |Ra - Rb|_F = 2 sqrt(2) sin(angle / 2) (acos of
    an fp32 trace reads 0 below 0.02 degrees)."""
    diff = (torch.as_tensor(Ra).double().cpu() - torch.as_tensor(Rb).double().cpu()).reshape(-1, 9).norm(dim=-1)
    return torch.rad2deg(2 * torch.asin(torch.clamp(diff / (2 * 2**0.5), max=1.0)))


def pose_errors(poses, true_poses):
    """(degrees [P], distance [P]) between two sets of poses [P,3|4,4], fp64 on the CPU."""
    a, b = torch.as_tensor(poses).double().cpu()[:, :3, :4], torch.as_tensor(true_poses).double().cpu()[:, :3, :4]
    return rotation_angle_deg(a[:, :, :3], b[:, :, :3]), (a[:, :, 3] - b[:, :, 3]).norm(dim=-1)


def perturb_poses(poses, degrees, distance, seed=0):
    """poses [P,3|4,4] turned by `degrees` about a random axis (about the camera centre) and shifted by `distance` in a random
    direction, seeded: [P,3,4] fp32."""
    c = torch.as_tensor(poses).double().cpu()[:, :3, :4].clone()
    g = torch.Generator().manual_seed(int(seed))
    unit = lambda x: x / x.norm(dim=-1, keepdim=True)
    axis = unit(torch.randn(c.shape[0], 3, generator=g, dtype=torch.float64)) * np.deg2rad(float(degrees))
    shift = unit(torch.randn(c.shape[0], 3, generator=g, dtype=torch.float64)) * float(distance)
    K = torch.zeros(c.shape[0], 3, 3, dtype=torch.float64)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = (-axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0],
                                                                            -axis[:, 1], axis[:, 0])
    c[:, :, :3] = torch.matrix_exp(K) @ c[:, :, :3]
    c[:, :, 3] += shift
    return c.float()


class PoseRefiner:
    """Refines init_poses [P,3|4,4] so that the frozen student `model` reproduces images [P,H,W,3] (values in [0, 1], as
    Scene.rgb_images gives them): n_rays pixels per image and iteration.  The device is the model's.

    step()       one iteration, staged: every call of r2l_pose_refine_step's list made from Python
    fused_step() the same iteration as ONE library call (bit for bit the same result)
    run(iters)   enqueues iterations and synchronises once;  poses [P,3,4];  losses [iterations so far, P]
    Both step methods are refine_step_spec on the CPU.  The engine's r2l_config applies (model.engine().set_config), so every
    kernel family is reachable.  Nothing here synchronises but run(), losses and pose_errors()."""

    def __init__(self, model, point_sampler, images, init_poses, n_rays, lr_rot=2e-3, lr_trans=5e-3, betas=(0.9, 0.999), eps=1e-8,
                 seed=R2L_SEED):
        self.model, self.ps = model, point_sampler
        self.device = next(model.parameters()).device
        images = torch.as_tensor(images, dtype=torch.float32)
        poses = torch.as_tensor(init_poses, dtype=torch.float32)
        if poses.dim() != 3 or tuple(poses.shape[1:]) not in ((3, 4), (4, 4)):
            raise ValueError("PoseRefiner: init_poses must be [P,3,4] or [P,4,4], got %s" % (tuple(poses.shape),))
        self.P, self.H, self.W = int(poses.shape[0]), int(point_sampler.H), int(point_sampler.W)
        if images.dim() != 4 or tuple(images.shape) != (self.P, self.H, self.W, 3):
            raise ValueError("PoseRefiner: need images [%d,%d,%d,3], got %s" % (self.P, self.H, self.W, tuple(images.shape)))
        self.n = int(n_rays)
        if not 1 <= self.n <= self.H * self.W:
            raise ValueError("PoseRefiner: n_rays %d is outside 1 .. H*W = %d" % (self.n, self.H * self.W))
        if self.P < 1 or self.P * self.n >= 2**31 or self.P * self.H * self.W >= 2**31:
            raise ValueError("PoseRefiner: need 1 <= P and P*n_rays, P*H*W < 2^31")
        self.N = self.P * self.n
        self.focal = float(point_sampler.focal)
        self.lr_rot, self.lr_trans, self.betas, self.eps = float(lr_rot), float(lr_trans), (float(betas[0]), float(betas[1])), float(eps)
        self.seed = int(seed) & M64
        self.iteration = 0
        f = dict(dtype=torch.float32, device=self.device)
        self.images = images.to(self.device).contiguous()
        self.c2w = poses[:, :3, :4].to(self.device).contiguous().clone()
        self.exp_avg, self.exp_avg_sq = torch.zeros(self.P, 6, **f), torch.zeros(self.P, 6, **f)
        self._loss_rows = []
        self._loss_buf, self._loss_used = None, 0
        self.last = {}
        self.gpu = self.device.type == "cuda"
        if self.gpu:
            for p in model.parameters():  # frozen: the streams are packed once
                p.requires_grad_(False)
            self.eng = model.engine()
            self.lib = self.eng.lib
            self.eng.ensure_packed(self.N, with_stash=True)  # (flattens; the forward stream is packed again by the first step)
            self.wstream_bwd = torch.zeros(self.lib.r2l_bwd_stream_floats(self.eng.n_block), **f)
            self._packed = False
            self._work = None

    # ---- state ------------------------------------------------------------------------------------------------------------------
    @property
    def poses(self):
        return self.c2w

    @property
    def losses(self):
        """[iterations so far, P] on the refiner's device (reading it on the host synchronises)."""
        if not self._loss_rows:
            return torch.zeros(0, self.P, dtype=torch.float32, device=self.device)
        return torch.stack(self._loss_rows, 0)

    def pose_errors(self, true_poses):
        return pose_errors(self.c2w, true_poses)

    def state_dict(self):
        return {"poses": self.c2w.clone(), "exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone(),
                "iteration": self.iteration}

    def load_state_dict(self, state):
        self.c2w.copy_(state["poses"])
        self.exp_avg.copy_(state["exp_avg"])
        self.exp_avg_sq.copy_(state["exp_avg_sq"])
        self.iteration = int(state["iteration"])

    def _loss_row(self):
        """A fresh device row [P] for this iteration's losses (rows are handed out of blocks of 256: no allocation per step)."""
        if self._loss_buf is None or self._loss_used == self._loss_buf.shape[0]:
            self._loss_buf = torch.zeros(256, self.P, dtype=torch.float32, device=self.device)
            self._loss_used = 0
        row = self._loss_buf[self._loss_used]
        self._loss_used += 1
        self._loss_rows.append(row)
        return row

    # ---- the CPU path -----------------------------------------------------------------------------------------------------------
    def _spec_step(self):
        it = self.iteration + 1
        c2w, m, v, loss, parts = refine_step_spec(self.model, self.ps, self.images, self.c2w, self.exp_avg, self.exp_avg_sq, self.H,
                                                  self.W, self.focal, self.seed, it, self.n, self.lr_rot, self.lr_trans,
                                                  self.betas[0], self.betas[1], self.eps)
        self.c2w, self.exp_avg, self.exp_avg_sq = c2w.detach(), m.detach(), v.detach()
        self._loss_row().copy_(loss.detach())
        self.last = parts
        self.iteration = it
        return loss

    # ---- the device paths -------------------------------------------------------------------------------------------------------
    def _desc(self, it, pack):
        self._cfg_keep = self.eng.effective_config()  # (kept alive: the descriptor points at it)
        return _lib.PoseRefineDesc(n_block=self.eng.n_block, pack=pack, cfg=ctypes.pointer(self._cfg_keep), P=self.P, H=self.H, W=self.W,
                                   focal=self.focal, n=self.n, seed=self.seed, iteration=it, lr_rot=self.lr_rot, lr_trans=self.lr_trans,
                                   beta1=self.betas[0], beta2=self.betas[1], eps=self.eps)

    def work_layout(self):
        """{part: (offset, floats)} of the work buffer of r2l_pose_refine_step (include/r2l_hip.h), and the total."""
        lib, nb, N = self.lib, self.eng.n_block, self.N
        slot = int(lib.r2l_stash_slot_floats(N))
        sizes = [("rays_o", N * 3), ("rays_d", N * 3), ("target", N * 3), ("rgb", N * 3), ("save_x", (nb + 1) * slot),
                 ("save_t", max(nb, 1) * slot), ("gx", (nb + 1) * slot), ("gt", max(nb, 1) * slot), ("dpre", N * 3),
                 ("sqerr", int(lib.r2l_num_tiles(N))), ("d_rays_o", N * 3), ("d_rays_d", N * 3), ("grad", self.P * 6),
                 ("pose_grad", int(lib.r2l_pose_grad_work_floats(self.P, self.n)))]
        out, at = {}, 0
        for k, s in sizes:
            out[k] = (at, s)
            at += (s + 1023) & ~1023
        return out, at

    def _buffers(self):
        """The one work buffer, sized by the library; the staged path uses its parts, the fused call the whole."""
        if self._work is None:
            need = int(self.lib.r2l_pose_refine_work_floats(ctypes.byref(self._desc(1, 0))))
            if need < 0:
                _lib.check(1, "r2l_pose_refine_work_floats")
            layout, total = self.work_layout()
            assert total == need, (total, need)
            self._work = torch.empty(need, dtype=torch.float32, device=self.device)
            self._parts = {k: self._work[a:a + s] for k, (a, s) in layout.items()}
        return self._work, self._parts

    def _views(self, w):
        N = self.N
        self.last = {k: w[k].view(N, 3) for k in ("rays_o", "rays_d", "target", "rgb", "d_rays_o", "d_rays_d")}
        self.last["grad"] = w["grad"].view(self.P, 6)

    def stage_batch(self, it):
        """Stage 1 of an iteration: the rays and colours of iteration `it` under the current poses, into the work buffer."""
        _, w = self._buffers()
        _lib.check(self.lib.r2l_pose_batch(_ptr(self.images), _ptr(self.c2w), self.P, self.H, self.W, self.focal, self.seed, it, self.n,
                                           _ptr(w["rays_o"]), _ptr(w["rays_d"]), _ptr(w["target"]), None, _stream(self.device)),
                   "r2l_pose_batch")

    def stage_gradient(self, loss):
        """Stages 2 - 6 on the rays_o / rays_d / target of the work buffer (stage_batch's, or a test's own): [pack,] forward with
        the stash, the dX chain in MSE mode, the input gradient, the pose gradient -> grad [P,6] (a view of the work buffer) and
        loss [P]."""
        lib, eng, nb, N, st = self.lib, self.eng, self.eng.n_block, self.N, _stream(self.device)
        _, w = self._buffers()
        cfg = eng._cfg()
        ztab = eng.ztab(self.ps.z_vals, 0.)
        if not self._packed:
            _lib.check(lib.r2l_pack_forward_layout(_ptr(eng.flat), nb, _ptr(eng.wstream), lib.r2l_forward_layout_for_cfg(N, 1, cfg), st),
                       "r2l_pack_forward_layout")
            _lib.check(lib.r2l_pack_backward_layout(_ptr(eng.flat), nb, _ptr(self.wstream_bwd), lib.r2l_backward_layout_for_cfg(N, cfg),
                                                    st), "r2l_pack_backward_layout")
            self._packed = True
        _lib.check(lib.r2l_forward_rays_cfg(_ptr(w["rays_o"]), _ptr(w["rays_d"]), None, _ptr(ztab), _ptr(eng.wstream), _ptr(eng.flat), nb,
                                            _ptr(w["rgb"]), _ptr(w["save_x"]), _ptr(w["save_t"]), N, st, cfg), "r2l_forward_rays")
        grad_scale = 2.0 / (3.0 * self.n)
        _lib.check(lib.r2l_backward_part_cfg(_ptr(w["rays_o"]), _ptr(w["rays_d"]), None, _ptr(ztab), None, _ptr(w["rgb"]), _ptr(w["target"]),
                                             None, _ptr(w["save_x"]), _ptr(w["save_t"]), _ptr(self.wstream_bwd), _ptr(eng.flat), nb,
                                             grad_scale, _ptr(w["dpre"]), _ptr(w["gx"]), _ptr(w["gt"]), _ptr(w["sqerr"]), _ptr(w["dpre"]),
                                             None, N, st, _lib.BWD_CHAIN, 0, 2 * nb, cfg), "r2l_backward (chain)")
        _lib.check(lib.r2l_backward_input(_ptr(w["gx"]), _ptr(eng.flat), nb, _ptr(w["rays_o"]), _ptr(w["rays_d"]), None, _ptr(ztab), None,
                                          _ptr(w["d_rays_o"]), _ptr(w["d_rays_d"]), N, st), "r2l_backward_input")
        _lib.check(lib.r2l_pose_grad(_ptr(w["rays_d"]), _ptr(w["d_rays_o"]), _ptr(w["d_rays_d"]), _ptr(w["rgb"]), _ptr(w["target"]),
                                     self.P, self.n, _ptr(w["grad"]), _ptr(loss), _ptr(w["pose_grad"]), st), "r2l_pose_grad")
        self._views(w)
        return self.last["grad"]

    def stage_update(self, it):
        """Stage 7: Adam on the 6-vectors and the retraction, step = it."""
        _, w = self._buffers()
        _lib.check(self.lib.r2l_pose_update(_ptr(self.c2w), _ptr(self.exp_avg), _ptr(self.exp_avg_sq), _ptr(w["grad"]), self.P,
                                            self.lr_rot, self.lr_trans, self.betas[0], self.betas[1], self.eps, it,
                                            _stream(self.device)), "r2l_pose_update")

    def step(self):
        """One iteration, staged: every call of r2l_pose_refine_step's list made from Python.  Returns this iteration's losses [P]
        (device, no sync)."""
        if not self.gpu:
            return self._spec_step()
        it = self.iteration + 1
        loss = self._loss_row()
        self.stage_batch(it)
        self.stage_gradient(loss)
        self.stage_update(it)
        self.iteration = it
        return loss

    def fused_step(self):
        """One iteration as one library call.  Returns this iteration's losses [P] (device, no sync)."""
        if not self.gpu:
            return self._spec_step()
        eng = self.eng
        work, w = self._buffers()
        it = self.iteration + 1
        d = self._desc(it, 0 if self._packed else 1)
        loss = self._loss_row()
        _lib.check(self.lib.r2l_pose_refine_step(ctypes.byref(d), _ptr(self.images), _ptr(self.c2w), _ptr(self.exp_avg),
                                                 _ptr(self.exp_avg_sq), _ptr(eng.ztab(self.ps.z_vals, 0.)), _ptr(eng.flat),
                                                 _ptr(eng.wstream), _ptr(self.wstream_bwd), _ptr(loss), _ptr(work), _stream(self.device)),
                   "r2l_pose_refine_step")
        self._packed = True
        self._views(w)
        self.iteration = it
        return loss

    def run(self, iters, fused=True):
        """Enqueue `iters` iterations and synchronise once.  Returns the poses."""
        for _ in range(int(iters)):
            (self.fused_step if fused else self.step)()
        if self.gpu:
            torch.cuda.synchronize(self.device)
        return self.c2w
