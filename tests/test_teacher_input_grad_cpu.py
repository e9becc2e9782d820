"""The restatements of r2l_amd/teacher_input_grad.py on the CPU: in fp64 they equal torch autograd through
render.render_rays' CPU branch (the op-by-op teacher), and the pinned fp32 restatement that sets C_IN of the GPU tests lies
within C_IN / 4 of the fp64 spec over the GPU tests' whole shape list (tests/teacher_input_grad_util.py)."""
import itertools

import pytest
import torch

from oracle import r2l_oracle as O
from r2l_amd import render
from r2l_amd import teacher_input_grad as TI
from tests import teacher_input_grad_util as U
from tests.teacher_util import forward_weights

REL = 1e-10  # of the largest entry; measured 1e-15
R, NS, NI = 5, 6, 8


def _close(got, want, what):
    scale = want.abs().max().item()
    err = (got - want).abs().max().item()
    assert scale > 0, what
    assert err <= REL * scale, (what, err / scale)
    return err / scale


def _rays(seed, n=R):
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(n, 3, generator=g, dtype=torch.float64) * 0.4
    d = torch.randn(n, 3, generator=g, dtype=torch.float64) * (0.6 + torch.rand(n, 1, generator=g, dtype=torch.float64))
    vd = torch.nn.functional.normalize(torch.randn(n, 3, generator=g, dtype=torch.float64), dim=-1)
    tgt = torch.rand(n, 3, generator=g, dtype=torch.float64)
    return o, d, vd, tgt


def _pair():
    return [{k: v.double() for k, v in sd.items()} for sd in O.make_teacher_state_dicts(5, 2, alpha_bias=0.5)]


CONFIGS = list(itertools.product([1, 2], [0, 1], [False, True], [False, True], [False, True]))


@pytest.mark.parametrize("n_nets,perturb,white,noisy,fold", CONFIGS)
def test_spec_equals_autograd_through_render_rays(n_nets, perturb, white, noisy, fold):
    """d_rays_o, d_rays_d (and d_viewdirs where viewdirs is an input of its own) of render_loss_grad_spec in fp64 against fp64
    autograd of grad_scale / 2 (|rgb - t|^2 + |rgb0 - t|^2) through render.render_rays: relative 1e-10 of the largest entry."""
    sds = _pair()[:n_nets]
    nets = [U.nerf_module(sd) for sd in sds]
    o, d, vd, tgt = _rays(3 + n_nets)
    g = torch.Generator().manual_seed(11)
    t_rand = torch.rand(R, NS, generator=g, dtype=torch.float64) if perturb else None
    u = torch.rand(R, NI, generator=g, dtype=torch.float64) if perturb else torch.linspace(0., 1., NI).double()
    ni = NI if n_nets > 1 else 0
    std = 0.3 if noisy else 0.
    s = 0.37
    torch.manual_seed(5)
    ret, (lo, ld, lv) = U.render_autograd(nets, o, d, None if fold else vd, 2., 6., NS, ni, white, t_rand, u, raw_noise_std=std)
    loss = 0.5 * s * ((ret["rgb_map"] - tgt)**2).sum()
    if n_nets > 1:
        loss = loss + 0.5 * s * ((ret["rgb0"] - tgt)**2).sum()
    grads = torch.autograd.grad(loss, [lo, ld] + ([] if fold else [lv]))
    torch.manual_seed(5)  # the draws of render.raw2outputs, in its order
    noise = ([torch.randn(R, NS) * std] + ([torch.randn(R, NS + NI) * std] if n_nets > 1 else [])) if noisy else None
    vd_in = d / d.norm(dim=-1, keepdim=True) if fold else vd
    r = TI.render_loss_grad_spec(sds[0], sds[1] if n_nets > 1 else None, o, d, vd_in, 2., 6., tgt, NS, ni, white, s, t_rand, u,
                                 noise=noise, fold_viewdirs=fold)
    _close(r["loss"], loss.detach(), "loss")
    _close(r["rgb_map"], ret["rgb_map"].detach(), "rgb_map")
    worst = max(_close(r["d_rays_o"], grads[0], "d_rays_o"), _close(r["d_rays_d"], grads[1], "d_rays_d"))
    if not fold:
        worst = max(worst, _close(r["d_viewdirs"], grads[2], "d_viewdirs"))
    print("spec vs autograd (nets %d, perturb %d, white %d, noise %d, fold %d): %.2g" % (n_nets, perturb, white, noisy, fold, worst))


@pytest.mark.parametrize("white,noisy,seeded", [(False, False, False), (True, True, False), (True, False, True), (False, True, True)])
def test_raw2outputs_backward_spec_equals_autograd(white, noisy, seeded):
    """draw and d_len of the closed form against fp64 autograd of render.raw2outputs with |rays_d| a leaf of its own, under the MSE
    seed at an arbitrary grad_scale and under an arbitrary dL/drgb_map."""
    g = torch.Generator().manual_seed(2)
    n, S = 7, 9
    raw = (torch.randn(n, S, 4, generator=g, dtype=torch.float64) * 2).requires_grad_(True)
    z = torch.sort(torch.rand(n, S, generator=g, dtype=torch.float64) * 4 + 2, -1)[0]
    unit = torch.nn.functional.normalize(torch.randn(n, 3, generator=g, dtype=torch.float64), dim=-1)
    length = (0.5 + torch.rand(n, 1, generator=g, dtype=torch.float64)).requires_grad_(True)
    noise = (torch.randn(n, S, generator=g) * 0.5) if noisy else None  # (fp32 values: render.raw2outputs keeps noise in fp32)
    tgt = torch.rand(n, 3, generator=g, dtype=torch.float64)
    gs = torch.randn(n, 3, generator=g, dtype=torch.float64)
    rgb = render.raw2outputs(raw, z, unit * length, white_bkgd=white, noise=noise)[0]
    s = 0.81
    loss = (rgb * gs).sum() if seeded else 0.5 * s * ((rgb - tgt)**2).sum()
    want_draw, want_len = torch.autograd.grad(loss, [raw, length])
    draw, sqerr, d_len, rgb_s = TI.raw2outputs_backward_spec(raw.detach(), z, (unit * length).detach(),
                                                             None if noise is None else noise.double(), white,
                                                             None if seeded else tgt, gs if seeded else None, s)
    _close(rgb_s, rgb.detach(), "rgb_map")
    _close(draw, want_draw, "draw")
    _close(d_len, want_len[:, 0], "d_len")
    if not seeded:
        _close(sqerr, ((rgb - tgt)**2).sum(-1).detach(), "sqerr")


def test_render_rays_diff_under_an_upstream_gradient():
    """render_rays_diff on CPU modules, the g form of render_loss_grad_spec and autograd through render.render_rays agree under
    an arbitrary upstream gradient on (rgb_map, rgb0)."""
    sds = _pair()
    nets = [U.nerf_module(sd) for sd in sds]
    o, d, vd, _ = _rays(9)
    g = torch.Generator().manual_seed(4)
    G1, G0 = torch.randn(R, 3, generator=g, dtype=torch.float64), torch.randn(R, 3, generator=g, dtype=torch.float64)
    u = torch.linspace(0., 1., NI).double()
    ret, leaves = U.render_autograd(nets, o, d, vd, 2., 6., NS, NI, True, None, u)
    want = torch.autograd.grad((ret["rgb_map"] * G1).sum() + (ret["rgb0"] * G0).sum(), leaves)
    r = TI.render_loss_grad_spec(sds[0], sds[1], o, d, vd, 2., 6., None, NS, NI, True, g=[G0, G1])
    lo, ld, lv = [t.clone().requires_grad_(True) for t in (o, d, vd)]
    rgb, rgb0 = TI.render_rays_diff(lo, ld, lv, 2., 6., nets[0], nets[1], NS, NI, True)
    ((rgb * G1).sum() + (rgb0 * G0).sum()).backward()
    for k, w, got in zip(("d_rays_o", "d_rays_d", "d_viewdirs"), want, (lo.grad, ld.grad, lv.grad)):
        _close(r[k], w, k + " (spec)")
        _close(got, w, k + " (render_rays_diff)")
    assert all(p.grad is None for n in nets for p in n.parameters())


def test_teacher_ray_grad_on_cpu_modules_is_the_spec():
    sds = O.make_teacher_state_dicts(5, 2, alpha_bias=0.5)
    nets = [U.nerf_module(sd, torch.float32) for sd in sds]
    o, d, vd, tgt = [t.float() for t in _rays(1)]
    rg = TI.TeacherRayGrad(nets[0], nets[1], NS, NI, True)
    loss_out, d_o, d_d, d_vd = rg.loss_and_grad(o, d, vd, 2., 6., tgt, fold_viewdirs=True)
    r = TI.render_loss_grad_spec(sds[0], sds[1], o, d, vd, 2., 6., tgt, NS, NI, True, fold_viewdirs=True)
    assert torch.equal(d_o, r["d_rays_o"]) and torch.equal(d_d, r["d_rays_d"]) and torch.equal(d_vd, r["d_viewdirs"])
    assert torch.equal(loss_out[0], r["loss"]) and len(rg.last_z) == 2 and rg.last_z[1].shape == (R, NS + NI)
    with pytest.raises(NotImplementedError):
        TI.TeacherRayGrad(nets[0], None, NS, NI, True)


# ---- the pinned fp32 restatement: what C_IN is read from ------------------------------------------------------------------------
def pinned_case(sd, Rr, S, kind, seed=0):
    """One row of the table: the worst |input_grad32 - fp64 spec| / (mag + floor) per tensor, with d_len and the folding on."""
    from tests.teacher_util import forward_inputs
    o, d, vd, z = forward_inputs(Rr, S, "trained" if kind == "trained" else "init", seed)
    if kind == "init":
        d = d * (0.5 + torch.rand(Rr, 1, generator=torch.Generator().manual_seed(S)))  # |d| != 1
    sd64 = {k: v.double() for k, v in sd.items()}
    pts = U.points32(o, d, z).double()
    outs = TI.layer_outputs(sd64, TI.embed(pts, 10), TI.embed(vd.double()[:, None, :].expand(Rr, S, 3).reshape(-1, 3), 4))
    masks = ([x > 0 for x in outs[:8]], outs[9] > 0)
    raw = TI.raw_from_outputs(sd64, outs).view(Rr, S, 4)
    draw = U.make_draw(raw, Rr * 1000 + S)
    d_len = U.make_d_len(Rr, S)
    want = U.want64(sd, o, d, vd, z, masks, draw, d_len, True)
    mags = U.mags64(sd, o, d, vd, z, masks, draw, d_len, True)
    got = U.input_grad32(sd, o, d, vd, z, masks, draw, d_len, True)
    out = {}
    for k in U.TENSORS:
        m = mags[k]
        out[k] = ((got[k].double() - want[k]).abs() / (m + 1e-12 * m.max() + 1e-300)).max().item()
    return out


@pytest.mark.parametrize("kind", ["init", "trained"])
def test_pinned_fp32_restatement_sets_c_in(kind):
    """The pinned fp32 restatement against the fp64 spec over the GPU tests' shapes: every entry within C_IN / 4 of its magnitude.
    (The last shape, 198 000 points and five minutes on the CPU, is part of the table in teacher_input_grad_util's head; it is run
    here at an eighth of its rays, (129, 192): the same tiles, tails and sample count.)"""
    sd = forward_weights(kind, device="cpu") if kind == "trained" else O.make_teacher_state_dicts(5, 1, alpha_bias=0.5)[0]
    worst = {k: 0. for k in U.TENSORS}
    for Rr, S in U.SHAPES[:-1] + [(129, 192)]:
        row = pinned_case(sd, Rr, S, kind)
        print("pinned fp32 (%d, %d) %s: %s" % (Rr, S, kind, "  ".join("%s %.3g" % kv for kv in row.items())))
        worst = {k: max(worst[k], row[k]) for k in row}
    for k in U.TENSORS:
        assert worst[k] <= U.C_IN[k] / 4, (k, worst[k], U.C_IN[k])


# ---- the C ABI ------------------------------------------------------------------------------------
def test_abi_is_declared_bound_and_exported():
    import ctypes
    import os
    from r2l_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "r2l_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("r2l_raw2outputs_backward_scaled", "r2l_teacher_backward_input"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and "int %s(" % name in header
    assert "r2l_teacher_input_grad_work_floats" in _lib.SIGNATURES and hasattr(lib, "r2l_teacher_input_grad_work_floats")
    assert "int64_t r2l_teacher_input_grad_work_floats(" in header
    assert len(_lib.SIGNATURES["r2l_teacher_backward_input"][1]) == 17 and len(_lib.SIGNATURES["r2l_raw2outputs_backward_scaled"][1]) == 14


if __name__ == "__main__":  # python -m tests.test_teacher_input_grad_cpu: the whole table of teacher_input_grad_util's head
    # (both weight kinds over every shape, the 198 000-point one included: about six minutes)
    for _kind in ("init", "trained"):
        _sd0 = forward_weights(_kind, device="cpu") if _kind == "trained" else O.make_teacher_state_dicts(5, 1, alpha_bias=0.5)[0]
        _worst = {k: 0. for k in U.TENSORS}
        for _R, _S in U.SHAPES:
            _row = pinned_case(_sd0, _R, _S, _kind)
            print("pinned fp32 (%d, %d) %s: %s" % (_R, _S, _kind, "  ".join("%s %.3g" % kv for kv in _row.items())), flush=True)
            _worst = {k: max(_worst[k], _row[k]) for k in _row}
        print("%s: worst %s; 4 x = %s" % (_kind, _worst, {k: 4 * v for k, v in _worst.items()}))
