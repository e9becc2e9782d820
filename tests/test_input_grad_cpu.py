"""The student's input gradient without a GPU: the library's export and argument checks (host code, in front of the first
launch), the torch restatement r2l_amd/input_grad.py against fp64 autograd through the oracle's own sampler and encoder, and the
CPU module — plain torch ops, differentiable in its input — against the restatement fed the fp64 head gradient.  The CPU path is
the meaning the GPU path (tests/test_input_grad_gpu.py) has to reproduce."""
import argparse
import ctypes
import os

import pytest
import torch

from oracle import r2l_oracle as O
from r2l_amd.input_grad import input_grad_spec
from tests import input_grad_util as U
from tests import student_util as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_backward_input():
    from r2l_amd import _lib
    header = open(os.path.join(ROOT, "include", "r2l_hip.h")).read()
    name = "r2l_backward_input"
    assert name in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), name) and "int %s(" % name in header
    assert len(_lib.SIGNATURES[name][1]) == 12


def test_argument_errors_are_named_before_any_launch():
    """Every refusal of include/r2l_hip.h returns non-zero with its message; none of them reaches the device (no GPU here)."""
    from r2l_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)  # never dereferenced: the checks come first
    call = lambda gx=p, par=p, nb=1, o=p, d=p, u=None, zt=p, e=p, do=p, dd=p, n=5: lib.r2l_backward_input(gx, par, nb, o, d, u, zt, e,
                                                                                                           do, dd, n, None)
    cases = [(dict(e=None, do=None, dd=None), "no output"), (dict(o=None), "ray form"), (dict(d=None), "ray form"),
             (dict(zt=None), "ray form"), (dict(do=None), "go together"), (dict(dd=None), "go together"), (dict(n=0), "N < 1"),
             (dict(n=-3), "N < 1"), (dict(nb=-1), "n_block"), (dict(gx=None), "NULL"), (dict(par=ctypes.c_void_p(4100)), "aligned")]
    for kw, word in cases:
        assert call(**kw) != 0, kw
        assert word in lib.r2l_last_error().decode(), (kw, lib.r2l_last_error())


@pytest.mark.parametrize("perturb", [0., 1.])
@pytest.mark.parametrize("n", [1, 33])
def test_spec_equals_autograd_through_the_oracle(n, perturb):
    """d_rays_o, d_rays_d of the restatement against torch autograd through O.sample_train + O.positional_embed, contracted with
    a random d_emb = gh Wh, in fp64: 1e-12 relative."""
    g = torch.Generator().manual_seed(100 * n + int(perturb))
    o, d, _, u = S.candidate_rays(n, 7 + n)
    gh = torch.randn(n, 256, generator=g, dtype=torch.float64)
    Wh = torch.randn(256, 1008, generator=g, dtype=torch.float64) / 16.
    z = O.z_vals(S.N_SAMPLE, S.NEAR, S.FAR).double()
    lower, upper = O.stratified_bounds(z)  # (the table in fp64 too: the span as the oracle forms it from the promoted depths)
    ztab = torch.cat([lower, upper - lower]) if perturb > 0 else torch.cat([z, torch.zeros_like(z)])
    d_emb, d_o, d_d = input_grad_spec(gh, Wh, o.double(), d.double(), u.double() if perturb > 0 else None, ztab)
    assert torch.equal(d_emb, gh @ Wh)
    o64, d64 = o.double().requires_grad_(True), d.double().requires_grad_(True)
    emb = O.positional_embed(O.sample_train(o64, d64, z, perturb, u.double() if perturb > 0 else None), 10)
    want_o, want_d = torch.autograd.grad((emb * d_emb).sum(), (o64, d64))
    for got, want in ((d_o, want_o), (d_d, want_d)):
        assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()
    assert input_grad_spec(gh, Wh)[1:] == (None, None)


def cpu_model(sd, nb):
    from model.nerf_raybased import NeRF_v3_2
    trial = argparse.Namespace(ON=True, body_arch="resmlp", inact="relu", outact="none", res_scale=1., n_learnable=2, n_block=-1,
                               near=-1, far=-1)
    args = argparse.Namespace(netdepth=2 * nb + 2, netwidth=256, layerwise_netwidths="", act="relu", linear_tail=False,
                              use_residual=True, trial=trial)
    m = NeRF_v3_2(args, 1008, 3)
    m.load_state_dict(sd)
    return m.double()


@pytest.mark.parametrize("frozen", [False, True])
def test_cpu_module_agrees_with_the_spec(frozen):
    """forward(emb) and forward_rays(o, d) on the CPU, inputs requiring grad, parameters frozen or not: the input's gradient is the
    restatement's, fed the fp64 gradient at the head's pre-activation."""
    from model.nerf_raybased import PointSampler
    nb, n, perturb = 1, 33, 1.
    sd = O.make_state_dict(n_block=nb, seed=S.NET_SEED)
    sd64 = S.f64(sd)
    m = cpu_model(sd, nb)
    for p in m.parameters():
        p.requires_grad_(not frozen)
    o, d, _, u = S.candidate_rays(n, 11)
    drgb = torch.randn(n, 3, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    ps = PointSampler(8, 8, 10., S.N_SAMPLE, S.NEAR, S.FAR, device="cpu")
    ztab = U.ztab_of(perturb).double()
    # the embedded form
    emb = O.positional_embed(O.sample_train(o, d, O.z_vals(S.N_SAMPLE, S.NEAR, S.FAR), perturb, u).double(), 10)
    e = emb.clone().requires_grad_(True)
    rgb = m(e)
    assert rgb.requires_grad
    (rgb * drgb).sum().backward()
    gh, _ = U.head_gradient64(sd64, emb, drgb)
    want = input_grad_spec(gh, sd64["head.0.weight"])[0]
    assert (e.grad - want).abs().max().item() <= 1e-10 * want.abs().max().item()
    # the ray form
    o64, d64 = o.double().requires_grad_(True), d.double().requires_grad_(True)
    rgb = m.forward_rays(o64, d64, ps, perturb=perturb, t_rand=u.double())
    (rgb * drgb).sum().backward()
    with torch.no_grad():
        emb_r = O.positional_embed(ps.sample_train(o.double(), d.double(), perturb, u.double()), 10)
    gh, _ = U.head_gradient64(sd64, emb_r, drgb)
    _, want_o, want_d = input_grad_spec(gh, sd64["head.0.weight"], o.double(), d.double(), u.double(), ztab)
    assert (o64.grad - want_o).abs().max().item() <= 1e-10 * want_o.abs().max().item()
    assert (d64.grad - want_d).abs().max().item() <= 1e-10 * want_d.abs().max().item()
