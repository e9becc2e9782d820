"""Pose refinement against a trained student on the GPU (include/r2l_hip.h "pose refinement"; csrc/r2l_pose.hip;
r2l_amd/pose_refine.py): r2l_pose_batch against r2l_image_batch bit for bit; r2l_pose_grad and r2l_pose_update per entry against
their fp64 restatements; the staged iteration against the one-call iteration bit for bit in every kernel family; the pose
gradient of a whole staged iteration against fp64 autograd on mask-stable rays; convergence on the scenario of
tests/pose_refine_util.py; the command line.

Bars.  r2l_pose_grad: |got - want| <= 2^-18 sum |terms| — one product rounding and up to 60 fp32 additions on a term's path (the
header states at most 33); the terms of a rotation entry are its 2 n products, of a translation entry its n addends, of a loss its
3 n squares over 3 n.  r2l_pose_update: R within 32 * 2^-24 per entry (2-ulp sincos, the products, one Gram-Schmidt pass), t within
4 * 2^-24 (|t| + |delta|), the moments within 4 ulp.  Measured worst values: DESIGN.md "Pose refinement"."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import r2l_oracle as O
from tests import input_grad_util as IU
from tests import pose_refine_util as U
from tests import student_util as S
from tests.conftest import use_family
from tests.test_driver_cpu import ROOT, make_scene
from tests.test_forward_gpu import build_model
from tests.test_student_backward_gpu import FAMILIES
from tests.test_teacher_backward_gpu import guarded, guards_intact, untouched

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE
u24 = 2.0 ** -24
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _leave_no_garbage():
    yield
    _CACHE.clear()
    import gc
    gc.collect()


def lib():
    from r2l_amd import _lib
    return _lib.load()


def ptr(t):
    from r2l_amd.engine import _ptr
    return _ptr(t)


def stream():
    from r2l_amd.engine import _stream
    return _stream()


def bits(t):
    return t.contiguous().view(torch.int32)


def poses_near_the_scene(P, seed):
    """P poses a few degrees off the head-on view from around (0, 0, 4): [P,3,4] fp32, rotations orthonormal to fp32."""
    g = torch.Generator().manual_seed(seed)
    w = 0.1 * torch.randn(P, 3, generator=g, dtype=torch.float64)
    t = torch.tensor([0., 0., 4.], dtype=torch.float64) + 0.2 * torch.randn(P, 3, generator=g, dtype=torch.float64)
    return torch.cat([torch.matrix_exp(U.skew(w)), t[:, :, None]], -1).float()


# ---- r2l_pose_batch -----------------------------------------------------------------------------------------------------------
def guarded_ids(n):
    whole, inner = guarded(2 * n)
    return whole, inner.view(torch.int64)


@pytest.mark.parametrize("P,n,H,W", [(1, 1, 5, 7), (3, 65, 9, 13), (2, 35, 5, 7), (2, 1000, 40, 50)])
def test_pose_batch_rows_are_the_image_samplers(P, n, H, W):
    from r2l_amd.pose_refine import pose_batch_spec, pose_key
    L, focal, it = lib(), 0.9 * W, 12
    g = torch.Generator().manual_seed(100 + n)
    images = torch.rand(P, H, W, 3, generator=g).cuda()
    c2w = poses_near_the_scene(P, 7 + n).cuda()
    N = P * n
    out = {k: guarded(N * 3) for k in ("o", "d", "t")}
    ids_whole, ids = guarded_ids(N)
    rc = L.r2l_pose_batch(ptr(images), ptr(c2w), P, H, W, focal, SEED, it, n, ptr(out["o"][1]), ptr(out["d"][1]), ptr(out["t"][1]),
                          ptr(ids), stream())
    assert rc == 0, L.r2l_last_error()
    torch.cuda.synchronize()
    for k, (whole, _) in out.items():
        assert guards_intact(whole, N * 3), "write outside " + k
    assert guards_intact(ids_whole, 2 * N)
    f = dict(dtype=torch.float32, device="cuda")
    for p in range(P):
        ro, rd, rv, rt = (torch.empty(n, 3, **f) for _ in range(4))
        rid = torch.empty(n, dtype=torch.int64, device="cuda")
        key = ctypes.c_uint64(0)
        assert L.r2l_pose_key(SEED, it, p, ctypes.byref(key)) == 0 and key.value == pose_key(SEED, it, p)
        rc = L.r2l_image_batch(ptr(images), ptr(c2w), P, H, W, focal, 0, p, 0, 0, H, W, key.value, n, ptr(ro), ptr(rd), ptr(rv), ptr(rt),
                               ptr(rid), stream())
        assert rc == 0, L.r2l_last_error()
        s = slice(p * n, (p + 1) * n)
        for name, ref in (("o", ro), ("d", rd), ("t", rt)):
            assert torch.equal(bits(out[name][1].view(N, 3)[s]), bits(ref)), (name, p)
        assert torch.equal(ids[s], rid) and len(set(rid.tolist())) == n
    so, sd_, st, sid = pose_batch_spec(images.cpu(), c2w.cpu(), H, W, focal, SEED, it, n)  # ... and the restatement's, bit for bit
    assert torch.equal(bits(out["o"][1].view(N, 3).cpu()), bits(so)) and torch.equal(bits(out["d"][1].view(N, 3).cpu()), bits(sd_))
    assert torch.equal(bits(out["t"][1].view(N, 3).cpu()), bits(st)) and np.array_equal(ids.cpu().numpy(), sid)
    # without ids_out, and a refusal: nothing is written
    again = guarded(N * 3)
    assert L.r2l_pose_batch(ptr(images), ptr(c2w), P, H, W, focal, SEED, it, n, ptr(again[1]), ptr(out["d"][1]), ptr(out["t"][1]), None,
                            stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(bits(again[1]), bits(out["o"][1]))
    fresh = guarded(N * 3)
    for over in (dict(n=H * W + 1), dict(it=0), dict(focal=0.0)):
        a = dict(dict(n=n, it=it, focal=focal), **over)
        assert L.r2l_pose_batch(ptr(images), ptr(c2w), P, H, W, a["focal"], SEED, a["it"], a["n"], ptr(fresh[1]), ptr(fresh[1]),
                                ptr(fresh[1]), None, stream()) == 1 and b"r2l_pose_batch" in L.r2l_last_error()
    torch.cuda.synchronize()
    assert untouched(fresh[0])


# ---- r2l_pose_grad ------------------------------------------------------------------------------------------------------------
GRAD_SHAPES = [(P, n) for n in (1, 63, 64, 65, 257, 1000, 4097) for P in (1, 3)] + [(257, 5)]
NAMES = ("rays_d", "d_rays_o", "d_rays_d", "rgb", "target")


def grad_inputs(P, n):
    """Five [P n, 3] CPU tensors with |entries| in [0.5, 1] and random signs: every ray carries a comparable share.  The last ray of
    the middle pose is fixed, so that each of its seven terms is far from zero (the self-check leaves that ray out)."""
    g = torch.Generator().manual_seed(31 * P + n)
    x = {k: (0.5 + 0.5 * torch.rand(P * n, 3, generator=g)) * (1 - 2 * (torch.rand(P * n, 3, generator=g) < 0.5).float()) for k in NAMES}
    if P >= 3:
        j = (P // 2) * n + n - 1
        for k, val in (("rays_d", (1., -0.5, 0.75)), ("d_rays_d", (0.5, 1., -1.)), ("d_rays_o", (0.5, -1., 0.75)), ("rgb", (0.9, 0.9, 0.9)),
                       ("target", (-0.6, -0.6, -0.6))):
            x[k][j] = torch.tensor(val)
    return x


def grad_yardstick(x64, P, n):
    """(want [P,7], sum |terms| [P,7]) in fp64: grad ++ loss."""
    from r2l_amd.pose_refine import pose_grad_spec
    grad, loss = pose_grad_spec(*[x64[k] for k in NAMES], P, n)
    seg = lambda t: t.reshape(P, n, 3)
    d, dd = seg(x64["rays_d"]).abs(), seg(x64["d_rays_d"]).abs()
    rot = torch.stack([d[..., 1] * dd[..., 2] + d[..., 2] * dd[..., 1], d[..., 2] * dd[..., 0] + d[..., 0] * dd[..., 2],
                       d[..., 0] * dd[..., 1] + d[..., 1] * dd[..., 0]], -1).sum(1)
    mags = torch.cat([rot, seg(x64["d_rays_o"]).abs().sum(1), loss[:, None]], -1)  # (a loss's terms are positive)
    return torch.cat([grad, loss[:, None]], -1), mags


def without_ray(x64, j):
    """The inputs with ray j contributing nothing."""
    x = {k: v.clone() for k, v in x64.items()}
    x["d_rays_o"][j] = 0.
    x["d_rays_d"][j] = 0.
    x["rgb"][j] = x["target"][j]
    return x


def grad_case(P, n):
    """grad_inputs on the device, each inside NaN guards; the fp64 restatement and sum |terms|."""
    if (P, n) not in _CACHE:
        x, whole = {}, {}
        for k, v in grad_inputs(P, n).items():
            whole[k], buf = guarded(P * n * 3)
            buf.copy_(v.reshape(-1))
            x[k] = buf.view(P * n, 3)
        x64 = {k: v.double() for k, v in x.items()}
        want, mags = grad_yardstick(x64, P, n)
        _CACHE[(P, n)] = dict(x=x, whole=whole, x64=x64, want=want, mags=mags)
    return _CACHE[(P, n)]


def call_grad(c, P, n, x=None, with_loss=True):
    L = lib()
    x = c["x"] if x is None else x
    gw, grad = guarded(P * 6)
    lw, loss = guarded(P)
    need = int(L.r2l_pose_grad_work_floats(P, n))
    ww, work = guarded(max(need, 1))
    rc = L.r2l_pose_grad(*[ptr(x[k]) for k in NAMES], P, n, ptr(grad), ptr(loss) if with_loss else None, ptr(work) if need else None,
                         stream())
    assert rc == 0, L.r2l_last_error()
    torch.cuda.synchronize()
    assert guards_intact(gw, P * 6) and guards_intact(ww, max(need, 1)) and (guards_intact(lw, P) if with_loss else untouched(lw))
    return torch.cat([grad.view(P, 6), loss.view(P, 1)], -1)


@pytest.mark.parametrize("P,n", GRAD_SHAPES)
def test_pose_grad_vs_fp64_spec(P, n):
    c = grad_case(P, n)
    got = call_grad(c, P, n)
    assert bool(torch.isfinite(got).all()), "an output is not finite (the inputs sit between NaN guards, the scratch starts as NaN)"
    ratio = ((got.double() - c["want"]).abs() / c["mags"]).max().item() / 2.0 ** -18
    print("r2l_pose_grad P %d n %d: worst |got - want| / sum|terms| = %.3f of the 2^-18 bar" % (P, n, ratio))
    assert ratio <= 1.0
    assert torch.equal(bits(got), bits(call_grad(c, P, n)))  # two calls, the same bits
    assert torch.equal(bits(got[:, :6]), bits(call_grad(c, P, n, with_loss=False)[:, :6]))  # loss == NULL changes nothing else
    for k in c["whole"]:
        assert guards_intact(c["whole"][k], P * n * 3), "an input was written: " + k


def test_pose_grad_bar_sees_one_missing_ray():
    """Self-check: the same comparison with the last ray of the middle segment left out of `want` fails at n = 4097 (the deficit is
    1/4097 of sum |terms| against the bar's 3.8e-6) — in every entry of that pose, in no entry of the others."""
    P, n = 3, 4097
    c = grad_case(P, n)
    got = call_grad(c, P, n)
    want, _ = grad_yardstick(without_ray(c["x64"], 1 * n + n - 1), P, n)
    bad = (got.double() - want).abs() > 2.0 ** -18 * c["mags"]
    assert bool(bad[1].all()) and not bool(bad[0].any()) and not bool(bad[2].any()), bad


def test_pose_grad_unaligned_inputs_take_the_scalar_path():
    """n % 4 == 0 but an input off a 16-byte boundary: other loads, another order, the same sums within the bar."""
    P, n = 3, 1000
    c = grad_case(P, n)
    x = dict(c["x"])
    shifted = torch.full((P * n * 3 + 1,), float("nan"), device="cuda")
    shifted[1:] = x["rgb"].reshape(-1)
    x["rgb"] = shifted[1:].view(P * n, 3)
    assert x["rgb"].data_ptr() % 16 == 4
    got = call_grad(c, P, n, x=x)
    assert ((got.double() - c["want"]).abs() <= 2.0 ** -18 * c["mags"]).all()


# ---- r2l_pose_update ------------------------------------------------------------------------------------------------------------
def ulp32(x):
    x = x.float().abs()
    return (torch.nextafter(x, torch.full_like(x, float("inf"))) - x).double()


def update_case(angle, step, seed):
    P = 3
    g = torch.Generator().manual_seed(seed)
    c2w = torch.cat([U.rotations(P, seed + 1, torch.float32), torch.randn(P, 3, 1, generator=g) + torch.tensor([[0.], [0.], [4.]])], -1)
    grad = (0.5 + torch.rand(P, 6, generator=g)) * (1 - 2 * (torch.rand(P, 6, generator=g) < 0.5).float())
    if step == 1:
        m, v = torch.zeros(P, 6), torch.zeros(P, 6)
    else:  # moments of a run that has seen gradients like this one
        m, v = grad * (0.8 + 0.4 * torch.rand(P, 6, generator=g)), grad * grad * (0.5 + torch.rand(P, 6, generator=g))
    f32 = lambda x: float(np.float32(x))
    return dict(c2w=c2w, grad=grad, m=m, v=v, lr_rot=f32(angle / 3 ** 0.5), lr_trans=f32(5e-3), b1=f32(0.9), b2=f32(0.999), eps=f32(1e-8),
                step=step, P=P)


def call_update(c, grad=None):
    L, P = lib(), c["P"]
    cw, c2w = guarded(P * 12)
    mw, m = guarded(P * 6)
    vw, v = guarded(P * 6)
    c2w.copy_(c["c2w"].reshape(-1)); m.copy_(c["m"].reshape(-1)); v.copy_(c["v"].reshape(-1))
    gr = (c["grad"] if grad is None else grad).cuda().contiguous()
    rc = L.r2l_pose_update(ptr(c2w), ptr(m), ptr(v), ptr(gr), P, c["lr_rot"], c["lr_trans"], c["b1"], c["b2"], c["eps"], c["step"], stream())
    assert rc == 0, L.r2l_last_error()
    torch.cuda.synchronize()
    assert guards_intact(cw, P * 12) and guards_intact(mw, P * 6) and guards_intact(vw, P * 6)
    return c2w.view(P, 3, 4).cpu(), m.view(P, 6).cpu(), v.view(P, 6).cpu()


@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("angle", [1e-9, 2e-3, 1.0])
def test_pose_update_vs_fp64_spec(angle, step):
    from r2l_amd.pose_refine import pose_update_spec
    c = update_case(angle, step, 41 + step)
    got_c, got_m, got_v = call_update(c)
    w_c, w_m, w_v = pose_update_spec(c["c2w"].double(), c["m"].double(), c["v"].double(), c["grad"].double(), c["lr_rot"], c["lr_trans"],
                                     c["b1"], c["b2"], c["eps"], step)
    # the step the fp64 side took, for the bars and the log
    dR = w_c[:, :, :3] @ c["c2w"][:, :, :3].double().transpose(1, 2)
    theta = torch.acos(torch.clamp((dR.diagonal(dim1=1, dim2=2).sum(-1) - 1) / 2, -1, 1)) if angle > 1e-4 else torch.full((3,), angle)
    delta_t = (w_c[:, :, 3] - c["c2w"][:, :, 3].double()).abs()
    eR = ((got_c[:, :, :3].double() - w_c[:, :, :3]).abs().max() / u24).item()
    et = ((got_c[:, :, 3].double() - w_c[:, :, 3]).abs() / (u24 * (w_c[:, :, 3].abs() + delta_t))).max().item()
    em = ((got_m.double() - w_m).abs() / ulp32(w_m)).max().item()
    ev = ((got_v.double() - w_v).abs() / ulp32(w_v)).max().item()
    print("r2l_pose_update angle %g (fp64 step %.3g rad) step %d: R %.2f u (bar 32), t %.2f u (|t| + |delta|) (bar 4), m %.2f ulp, v %.2f ulp "
          "(bar 4)" % (angle, theta.max().item(), step, eR, et, em, ev))
    assert not torch.equal(got_c, c["c2w"])
    assert eR <= 32 and et <= 4 and em <= 4 and ev <= 4
    R = got_c[:, :, :3].double()
    assert (R.transpose(1, 2) @ R - torch.eye(3, dtype=torch.float64)).abs().max().item() <= 1e-6


def test_pose_update_leaves_what_it_must():
    c = update_case(2e-3, 1, 77)
    # a zero gradient on zero moments: every bit stays
    got_c, got_m, got_v = call_update(c, grad=torch.zeros(3, 6))
    assert torch.equal(bits(got_c), bits(c["c2w"])) and not bool(got_m.any()) and not bool(got_v.any())
    # a non-finite gradient in one of three poses: that pose and its moments keep their bits, the others are updated as without it
    c = update_case(2e-3, 1000, 78)
    clean = call_update(c)
    for bad, at in ((float("nan"), 0), (float("inf"), 5), (-float("inf"), 2)):
        grad = c["grad"].clone()
        grad[1, at] = bad
        got = call_update(c, grad=grad)
        for new, old, ref in zip(got, (c["c2w"], c["m"], c["v"]), clean):
            assert torch.equal(bits(new[1]), bits(old[1])), "the pose with the non-finite gradient moved"
            assert torch.equal(bits(new[0]), bits(ref[0])) and torch.equal(bits(new[2]), bits(ref[2])) and bool(torch.isfinite(new).all())
            assert not torch.equal(new[0], old[0])


# ---- staged equals fused --------------------------------------------------------------------------------------------------------
STATE = ("c2w", "exp_avg", "exp_avg_sq")
PARTS = ("rays_o", "rays_d", "target", "rgb", "d_rays_o", "d_rays_d", "grad")


def refiner(sd, nb, P, n, H=40, W=40, seed=5):
    from model.nerf_raybased import PointSampler
    from r2l_amd.pose_refine import PoseRefiner
    g = torch.Generator().manual_seed(seed)
    images = torch.rand(P, H, W, 3, generator=g)
    ps = PointSampler(H, W, 50., S.N_SAMPLE, S.NEAR, S.FAR, device="cuda")
    return PoseRefiner(build_model(sd, nb), ps, images, poses_near_the_scene(P, seed + 1), n, seed=SEED)


def same_bits(a, b, what):
    for k in STATE:
        assert torch.equal(bits(getattr(a, k)), bits(getattr(b, k))), (what, k)
    for k in PARTS:
        assert torch.equal(bits(a.last[k]), bits(b.last[k])), (what, k)
    assert torch.equal(bits(a.losses), bits(b.losses)), (what, "losses")


def staged_against_fused(nb, P, n):
    sd = O.make_state_dict(n_block=nb, seed=S.NET_SEED)
    a, b = refiner(sd, nb, P, n), refiner(sd, nb, P, n)
    start = a.c2w.clone()
    for it in (1, 2, 3):
        a.step()
        b.fused_step()
        torch.cuda.synchronize()
        same_bits(a, b, "iteration %d" % it)
        assert bool(torch.isfinite(a.c2w).all()) and bool(torch.isfinite(a.losses).all())
    assert not torch.equal(a.c2w, start) and a.losses.shape == (3, P) and bool((a.last["grad"] != 0).all())
    state = b.state_dict()
    c = refiner(sd, nb, P, n)  # a fresh refiner loaded with the state after the third iteration
    c.load_state_dict(state)
    b.fused_step()
    c.fused_step()
    a.step()
    torch.cuda.synchronize()
    for k in STATE + ("iteration",):
        assert torch.equal(torch.as_tensor(getattr(b, k)).cpu(), torch.as_tensor(getattr(c, k)).cpu()), ("resumed", k)
    assert torch.equal(bits(b.losses[3]), bits(c.losses[0])) and torch.equal(bits(b.last["grad"]), bits(c.last["grad"]))
    same_bits(a, b, "iteration 4")


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("P,n", [(1, 33), (3, 65), (2, 1000)])
def test_staged_equals_fused_bit_for_bit(P, n, family, monkeypatch):
    use_family(monkeypatch, **FAMILIES[family])
    staged_against_fused(1, P, n)


def test_staged_equals_fused_with_two_blocks(monkeypatch):
    use_family(monkeypatch)
    staged_against_fused(2, 3, 65)


# ---- the pose gradient of a whole staged iteration against fp64 autograd -------------------------------------------------------------
def e2e_case(nb, P, n):
    """P n mask-stable rays (student_util.select_case, the selection of test_student_backward_gpu.case), ray p n + j taken for ray j
    of pose p, and fp64 autograd of the whole map (w, v) -> sum_p mse_p at 0: d <- exp([w_p]x) d, o <- o + v_p, evaluated AT the
    fp32 sample points the device sees."""
    key = ("e2e", nb, P, n)
    if key not in _CACHE:
        N = P * n
        sd = O.make_state_dict(n_block=nb, seed=S.NET_SEED)
        c = S.select_case(sd, N, 0., S.case_seed(nb, N, 0.), device="cuda")
        assert c["rejected"] <= S.REJECT_CAP[nb], c["rejected"]
        sd64 = S.f64(sd, "cuda")
        o, d, tgt = c["o"].cuda(), c["d"].cuda(), c["tgt"].cuda()
        w = torch.zeros(P, 3, dtype=torch.float64, device="cuda", requires_grad=True)
        v = torch.zeros(P, 3, dtype=torch.float64, device="cuda", requires_grad=True)
        pose = torch.arange(N, device="cuda") // n
        K = torch.zeros(P, 3, 3, dtype=torch.float64, device="cuda")
        K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
        d64 = (torch.matrix_exp(K)[pose] @ d.double()[:, :, None])[:, :, 0]
        o64 = o.double() + v[pose]
        pts32, _ = IU.points32(o, d, None, 0.)
        with torch.device("cuda"):
            pts = O.sample_train(o64, d64, O.z_vals(S.N_SAMPLE, S.NEAR, S.FAR).double(), 0., None)
            pts = pts + (pts32.double() - pts).detach()
            rgb = O.r2l_forward(sd64, O.positional_embed(pts, 10))
        mse = ((rgb - tgt.double()) ** 2).reshape(P, -1).mean(-1)
        gw, gv = torch.autograd.grad(mse.sum(), (w, v))
        _CACHE[key] = dict(sd=sd, o=o, d=d, tgt=tgt, want=torch.cat([gw, gv], -1), loss=mse.detach())
    return _CACHE[key]


@pytest.mark.parametrize("family", list(FAMILIES))
def test_pose_gradient_of_a_staged_iteration_vs_fp64_autograd(family, monkeypatch):
    nb, P, n = 1, 3, 65
    E = e2e_case(nb, P, n)
    use_family(monkeypatch, **FAMILIES[family])
    r = refiner(E["sd"], nb, P, n, H=16, W=16)
    _, w = r._buffers()
    for k, src in (("rays_o", E["o"]), ("rays_d", E["d"]), ("target", E["tgt"])):
        w[k][:P * n * 3].copy_(src.reshape(-1))
    loss = torch.empty(P, device="cuda")
    grad = r.stage_gradient(loss)
    torch.cuda.synchronize()
    rel = [S.nrel(grad[p], E["want"][p]) for p in range(P)]
    print("pose gradient of a staged iteration, %s: norm-relative per pose %s (bar %.3g); loss %s" % (
        family, ", ".join("%.3g" % x for x in rel), S.NREL_BWD, ", ".join("%.3g" % x for x in ((loss.double() - E["loss"]).abs() / E["loss"]).tolist())))
    assert all(E["want"][p].norm().item() > 0 for p in range(P)) and max(rel) <= S.NREL_BWD


# ---- convergence ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["auto", "fp32_mfma"])
def test_refiner_converges_on_the_gpu(precision, monkeypatch):
    """The CPU scenario (tests/pose_refine_util.py) through run(100, fused=True): both errors fall at least tenfold."""
    from r2l_amd.pose_refine import PoseRefiner
    use_family(monkeypatch, **({} if precision == "auto" else dict(precision=precision)))
    P = 2
    true, start = U.start_poses(P)
    if "cpu" not in _CACHE:  # the restatement's result, once
        m, ps = U.load_student(), U.sampler()
        r = PoseRefiner(m, ps, U.observed(m, ps, true[:1]), start[:1], U.N_RAYS)
        r.run(U.ITERS)
        _CACHE["cpu"] = r.pose_errors(true[:1])
    model, ps = U.load_student("cuda"), U.sampler("cuda")
    r = PoseRefiner(model, ps, U.observed(model, ps, true.cuda()), start, U.N_RAYS)
    rot0, tr0 = r.pose_errors(true)
    r.run(U.ITERS, fused=True)
    rot1, tr1 = r.pose_errors(true)
    losses = r.losses.cpu()
    print("GPU %s: rotation %s -> %s degrees, translation %s -> %s; loss %.3e -> %.3e; the CPU restatement ends at %.5f degrees, %.2e" % (
        precision, rot0.tolist(), ["%.5f" % x for x in rot1.tolist()], tr0.tolist(), ["%.2e" % x for x in tr1.tolist()],
        losses[0].mean().item(), losses[-1].mean().item(), _CACHE["cpu"][0].item(), _CACHE["cpu"][1].item()))
    assert losses.shape == (U.ITERS, P) and bool(torch.isfinite(losses).all())
    assert bool((rot1 <= rot0 / 10).all()) and bool((tr1 <= tr0 / 10).all())


# ---- the command line -----------------------------------------------------------------------------------------------------------------
def test_cli_on_the_gpu(tmp_path, monkeypatch):
    from r2l_amd import refine_pose
    from r2l_amd.checkpoint import save_ckpt
    from r2l_amd.options import parse_args
    from model.nerf_raybased import NeRF_v3_2
    use_family(monkeypatch)
    monkeypatch.chdir(tmp_path)
    scene = str(tmp_path / "scene")
    os.makedirs(scene)
    make_scene(scene, size=16)  # (lego_noview.txt: half_res, 8 x 8 frames)
    common = ["--model_name", "R2L", "--config", os.path.join(ROOT, "configs", "lego_noview.txt"), "--datadir", scene,
              "--n_sample_per_ray", "16", "--netwidth", "256", "--netdepth", "4", "--use_residual", "--trial.ON", "--trial.body_arch",
              "resmlp", "--testskip", "1", "--experiment_name", "refine_gpu"]
    torch.manual_seed(0)
    ck = save_ckpt(str(tmp_path / "student.tar"), 1, NeRF_v3_2(parse_args(common), 1008, 3), {"state": {}, "param_groups": []}, 0., 0)
    out = refine_pose.main(common + ["--pretrained_ckpt", ck, "--r2l_pose_iters", "5", "--r2l_pose_rays", "40", "--r2l_pose_out",
                                     str(tmp_path / "refined.npy")])
    saved = np.load(str(tmp_path / "refined.npy"))
    assert saved.shape == (2, 3, 4) and np.isfinite(saved).all() and not np.array_equal(saved, out["init"].numpy())
    assert out["losses"].shape == (5, 2) and bool(torch.isfinite(out["losses"]).all())
    R = torch.from_numpy(saved[:, :, :3]).double()
    assert (R.transpose(1, 2) @ R - torch.eye(3, dtype=torch.float64)).abs().max().item() < 1e-6
    log = open(os.path.join(out["logger"].log_path, "log.txt")).read()
    assert "[POSE] rotation error before 2.0000" in log and "[POSE] translation error before 0.05000" in log
