"""torch.autograd bridge for the HIP student path: keeps `rgb = model(embedded); loss.backward(); optimizer.step()`
(the reference's module-boundary training idiom, main.py:1374-1406) working with any loss and any torch optimizer.
Forward = r2l_forward_emb with the activation stash, backward = r2l_backward in generic mode (dL/drgb supplied by
autograd).  The build's own training loop does not go through autograd (r2l_amd/train_step.py).
Both functions also differentiate with respect to their INPUT (the embedding; rays_o / rays_d), as the reference's plain torch
module does: r2l_backward_input behind the dX chain (csrc/r2l_input_grad.hip, restated in r2l_amd/input_grad.py)."""
import torch

from . import _lib
from ._lib import ptr as _ptr, stream as _stream
from .engine import get_engine


class R2LEmbFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, module, emb, *params):
        eng = get_engine(module)
        eng.ensure_packed()
        emb2 = emb.reshape(-1, emb.shape[-1]).contiguous().float()
        n, nb = emb2.shape[0], eng.n_block
        f = dict(dtype=torch.float32, device=emb2.device)
        slot = int(eng.lib.r2l_stash_slot_floats(n))  # include/r2l_hip.h: (n_block + 1) / n_block slots of this many floats
        save_x = torch.empty((nb + 1) * slot, **f)
        save_t = torch.empty(max(nb, 1) * slot, **f)
        rgb = eng.forward_emb(emb2, save=(save_x, save_t))
        ctx.module, ctx.n = module, n
        ctx.lead = emb.shape[:-1]
        ctx.save_for_backward(emb2, rgb, save_x, save_t)
        return rgb.reshape(*emb.shape[:-1], 3)

    @staticmethod
    def backward(ctx, grad_rgb):
        emb2, rgb, save_x, save_t = ctx.saved_tensors
        eng = get_engine(ctx.module)
        eng.ensure_packed()
        lib, n, nb = eng.lib, ctx.n, eng.n_block
        f = dict(dtype=torch.float32, device=emb2.device)
        want_emb, want_params = ctx.needs_input_grad[1], any(ctx.needs_input_grad[2:])
        wbwd = torch.empty(lib.r2l_bwd_stream_floats(nb), **f)
        _lib.check(lib.r2l_pack_backward(_ptr(eng.flat), nb, _ptr(wbwd), _stream()), "r2l_pack_backward")
        slot = int(lib.r2l_stash_slot_floats(n))
        gx = torch.empty((nb + 1) * slot, **f)
        gt = torch.empty(max(nb, 1) * slot, **f)
        dpre = torch.empty(n * 3, **f)
        drgb = grad_rgb.reshape(-1, 3).contiguous().float()
        # A frozen student (only the input asks for a gradient): the dX chain alone — no weight-gradient stage, no 204 MB slab,
        # no flat gradient (the chain never touches `grads`; the entry point wants a pointer)
        grads = torch.zeros(eng.n_param, **f) if want_params else dpre
        slab = torch.empty(int(lib.r2l_dw_slab_floats()), **f) if want_params else None
        parts = _lib.BWD_ALL if want_params else _lib.BWD_CHAIN
        # The pre-embedded path always runs on the exact-fp32 MFMA kernels with a row-major stash (r2l_forward_emb has one
        # kernel); of the engine's r2l_config only `tiling` applies — which fp32 chain walks the backward — and `reserve_cus`;
        # precision / dw_mode concern the fused (ray-input) path only
        _lib.check(
            lib.r2l_backward_part_cfg(None, None, None, None, _ptr(emb2), _ptr(rgb), None, _ptr(drgb), _ptr(save_x),
                                      _ptr(save_t), _ptr(wbwd), _ptr(eng.flat), nb, 0.0, _ptr(dpre), _ptr(gx), _ptr(gt), None,
                                      _ptr(grads), _ptr(slab), n, _stream(), parts, 0, 2 * nb, eng._cfg()),
            "r2l_backward")
        d_emb = None
        if want_emb:  # dL/d(emb) = gh . W_head on the fp32 MFMA (csrc/r2l_input_grad.hip), in the input's leading dimensions
            d_emb = eng.backward_input(gx, n, want_emb=True)[0].reshape(*ctx.lead, emb2.shape[-1])
        return (None, d_emb) + _split_grads(eng, grads if want_params else None, ctx.needs_input_grad[2:])


def _split_grads(eng, grads, needs):
    """The flat gradient as views shaped like the parameters (None where autograd asks for none)."""
    out, off = [], 0
    for p, need in zip(eng.params, needs):
        k = p.numel()
        out.append(grads[off:off + k].view(p.shape) if (grads is not None and need) else None)
        off += k
    return tuple(out)


class R2LRaysFunction(torch.autograd.Function):
    """rgb = student(embed(sample_train(rays_o, rays_d))) with the sampler and the encoder fused in the kernels, differentiable
    with respect to rays_o, rays_d and the parameters: forward = r2l_forward_rays_cfg with the stash, backward =
    r2l_backward_part_cfg in generic mode under the engine's config (the dX chain alone when no parameter asks for a gradient),
    then r2l_backward_input.  The jitter t_rand gets no gradient.  Pose -> rays stays in torch (rays_d = dirs @ R^T is
    differentiable there)."""

    @staticmethod
    def forward(ctx, module, rays_o, rays_d, t_rand, z_vals, perturb, *params):
        eng = get_engine(module)
        o, d = rays_o.contiguous().float(), rays_d.contiguous().float()
        n, nb = o.shape[0], eng.n_block
        eng.ensure_packed(n, with_stash=True)
        f = dict(dtype=torch.float32, device=o.device)
        if perturb > 0 and t_rand is None:
            t_rand = torch.rand(n, 16, **f)
        u = t_rand.contiguous().float() if perturb > 0 else None
        slot = int(eng.lib.r2l_stash_slot_floats(n))
        save_x = torch.empty((nb + 1) * slot, **f)
        save_t = torch.empty(max(nb, 1) * slot, **f)
        rgb = eng.forward_rays(o, d, z_vals, perturb, u, save=(save_x, save_t))
        ctx.module, ctx.n, ctx.ztab, ctx.u = module, n, eng.ztab(z_vals, perturb), u
        ctx.save_for_backward(o, d, rgb, save_x, save_t)
        return rgb

    @staticmethod
    def backward(ctx, grad_rgb):
        o, d, rgb, save_x, save_t = ctx.saved_tensors
        eng = get_engine(ctx.module)
        lib, n, nb, u, ztab = eng.lib, ctx.n, eng.n_block, ctx.u, ctx.ztab
        f = dict(dtype=torch.float32, device=o.device)
        want_rays, want_params = ctx.needs_input_grad[1] or ctx.needs_input_grad[2], any(ctx.needs_input_grad[6:])
        # (zero-filled: the status words behind the streams carry the fp16 chain's scale history, include/r2l_hip.h)
        wbwd = torch.zeros(lib.r2l_bwd_stream_floats(nb), **f)
        _lib.check(lib.r2l_pack_backward(_ptr(eng.flat), nb, _ptr(wbwd), _stream()), "r2l_pack_backward")
        slot = int(lib.r2l_stash_slot_floats(n))
        gx = torch.empty((nb + 1) * slot, **f)
        gt = torch.empty(max(nb, 1) * slot, **f)
        dpre = torch.empty(n * 3, **f)
        drgb = grad_rgb.reshape(-1, 3).contiguous().float()
        grads = torch.zeros(eng.n_param, **f) if want_params else dpre
        slab = torch.empty(int(lib.r2l_dw_slab_floats()), **f) if want_params else None
        parts = _lib.BWD_ALL if want_params else _lib.BWD_CHAIN
        _lib.check(
            lib.r2l_backward_part_cfg(_ptr(o), _ptr(d), _ptr(u), _ptr(ztab), None, _ptr(rgb), None, _ptr(drgb), _ptr(save_x),
                                      _ptr(save_t), _ptr(wbwd), _ptr(eng.flat), nb, 0.0, _ptr(dpre), _ptr(gx), _ptr(gt), None,
                                      _ptr(grads), _ptr(slab), n, _stream(), parts, 0, 2 * nb, eng._cfg()),
            "r2l_backward")
        d_o = d_d = None
        if want_rays:
            _, d_o, d_d = eng.backward_input(gx, n, rays=(o, d, u, ztab), want_rays=True)
        return (None, d_o if ctx.needs_input_grad[1] else None, d_d if ctx.needs_input_grad[2] else None, None, None,
                None) + _split_grads(eng, grads if want_params else None, ctx.needs_input_grad[6:])
