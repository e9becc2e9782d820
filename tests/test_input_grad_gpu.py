"""The student's gradient with respect to its input on the GPU (csrc/r2l_input_grad.hip, r2l_backward_input): (a) the kernel
alone, fed a head gradient of the test's making, per entry against the fp64 restatement r2l_amd/input_grad.py; (b) end to end
against fp64 autograd through the oracle on mask-stable rays, the pre-embedded path in its two tilings and the ray path in every
kernel family of tests/test_student_backward_gpu.py; (c) the autograd surface of NeRF_v3_2.forward / forward_rays.

Bars.  d_emb is an fp32 MFMA sum over K = 256: per entry |got - want| <= C_BWD * mag + floor (tests/student_util.py), mag the
absolute sum |gh| |Wh|.  The ray-form sums continue it through encoder and sampler AT the fp32-rounded sample points (half an ulp
of a point moves phi' at the top frequency by 1e-4 of its bound), with phi' replaced by its bound 2^f in the yardstick
(tests/input_grad_util.py ray_mags).  End to end the bars are those test_student_backward_gpu.bar_failures applies to an exact
family — per entry C_BWD with the absolute backprop carried one layer further, per tensor NREL_BWD — for every family: the kernel
reads the chain's fp32 gh, not the fp16-rounded operand of the default trio's weight gradient."""
import pytest
import torch

from oracle import r2l_oracle as O
from tests import input_grad_util as U
from tests import student_util as S
from tests.conftest import use_family
from tests.test_forward_gpu import build_model
from tests.test_student_backward_gpu import FAMILIES, bar_failures, case, sampler
from tests.test_teacher_backward_gpu import guarded, guards_intact

pytestmark = pytest.mark.gpu

N_KERNEL = (1, 31, 32, 33, 65, 129, 1000)  # the 32-ray tile edge, the 128-ray workgroup edge, several workgroups
E2E_SHAPES = [(1, 33), (3, 65), (3, 1000)]  # of S.SHAPES
RAY_BAR = S.C_BWD  # the ray-form sums of (a) fit under the bar of the product itself (measured worst ratios: DESIGN.md §6)
EXACT_FAMILY = "main-f32mfma"  # the group whose bars bar_failures is asked for
_KCASES, _E2E = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _leave_no_garbage():
    """A module and its engine refer to each other, and an autograd graph holds the module: what these tests build is freed by
    the cycle collector only.  Collect when the file is done, so that no later test sees device memory released under its feet."""
    yield
    import gc
    gc.collect()


def lib_and_params():
    from r2l_amd import _lib
    if "lib" not in _KCASES:
        sd = O.make_state_dict(n_block=1, seed=S.NET_SEED)
        _KCASES["lib"] = (_lib.load(), O.flatten_state_dict(sd).float().cuda().contiguous(), sd["head.0.weight"].double().cuda())
    return _KCASES["lib"]


def kernel_case(n, perturb):
    """gh: random normal rows, half the entries zeroed like a ReLU mask; rays of the suites' distribution; the fp64 restatement
    at the fp32-rounded points and its magnitudes.  Computed once."""
    if (n, perturb) not in _KCASES:
        _, _, Wh64 = lib_and_params()
        g = torch.Generator().manual_seed(4242 + 2 * n + int(perturb > 0))
        gh = (torch.randn(n, 256, generator=g) * (torch.rand(n, 256, generator=g) < 0.5)).cuda()
        o, d, _, u = [t.cuda() for t in S.candidate_rays(n, 77 + n)]
        want, z = U.spec_at_fp32_points(gh.double(), Wh64, o, d, u, perturb)
        mags = {"d_emb": gh.double().abs() @ Wh64.abs()}
        mags.update(U.ray_mags(want["d_emb"].abs(), z))
        _KCASES[(n, perturb)] = dict(gh=gh, o=o.contiguous(), d=d.contiguous(), u=u.contiguous() if perturb > 0 else None,
                                     ztab=U.ztab_of(perturb, "cuda").contiguous(), want=want, mags=mags)
    return _KCASES[(n, perturb)]


def call_kernel(c, n, emb=True, rays=True, nb=1):
    """r2l_backward_input on a gx whose slot 0 holds gh and whose every other word — the padding rows included — is NaN, into
    guarded outputs.  Returns ({name: tensor}, {name: (whole buffer, floats)})."""
    from r2l_amd.engine import _ptr, _stream
    lib, flat, _ = lib_and_params()
    gx = torch.full(((nb + 1) * int(lib.r2l_stash_slot_floats(n)),), float("nan"), device="cuda")
    gx[:n * 256] = c["gh"].reshape(-1)
    bufs = {}
    if emb:
        bufs["d_emb"] = guarded(n * 1008) + (n * 1008,)
    if rays:
        bufs["d_rays_o"], bufs["d_rays_d"] = guarded(n * 3) + (n * 3,), guarded(n * 3) + (n * 3,)
    p = lambda k: _ptr(bufs[k][1]) if k in bufs else None
    rc = lib.r2l_backward_input(_ptr(gx), _ptr(flat), nb, _ptr(c["o"]), _ptr(c["d"]), _ptr(c["u"]), _ptr(c["ztab"]), p("d_emb"),
                                p("d_rays_o"), p("d_rays_d"), n, _stream())
    assert rc == 0, lib.r2l_last_error()
    torch.cuda.synchronize()
    shape = {"d_emb": (n, 1008), "d_rays_o": (n, 3), "d_rays_d": (n, 3)}
    return {k: v[1].view(shape[k]) for k, v in bufs.items()}, bufs


# ---- (a) the kernel alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("perturb", [0., 1.])
@pytest.mark.parametrize("n", N_KERNEL)
def test_kernel_vs_fp64_spec(n, perturb):
    c = kernel_case(n, perturb)
    got, bufs = call_kernel(c, n)
    for k, (whole, _, floats) in bufs.items():
        assert guards_intact(whole, floats), "write outside " + k
    assert all(bool(torch.isfinite(v).all().item()) for v in got.values()), "an entry is not finite (padding rows are NaN)"
    for k in got:
        print("kernel N %d perturb %g %s: worst |got - want| / mag %.3g" % (
            n, perturb, k, S.worst_ratio({k: got[k]}, {k: c["want"][k]}, c["mags"])[0]))
    viol = S.entry_violations({"d_emb": got["d_emb"]}, {"d_emb": c["want"]["d_emb"]}, c["mags"])
    rays = {k: c["want"][k] for k in ("d_rays_o", "d_rays_d")}
    viol.update(S.entry_violations({k: got[k] for k in rays}, rays, c["mags"], c=RAY_BAR))
    assert not any(viol.values()), viol


@pytest.mark.parametrize("n", [33, 129, 1000])
def test_kernel_is_deterministic_and_its_output_combinations_agree(n):
    c = kernel_case(n, 1.)
    both, _ = call_kernel(c, n)
    again, _ = call_kernel(c, n)
    emb_only, be = call_kernel(c, n, rays=False)
    rays_only, br = call_kernel(c, n, emb=False)
    for k in both:
        assert torch.equal(both[k], again[k]), k + ": two calls differ"
    assert torch.equal(both["d_emb"], emb_only["d_emb"])
    assert torch.equal(both["d_rays_o"], rays_only["d_rays_o"]) and torch.equal(both["d_rays_d"], rays_only["d_rays_d"])
    for bufs in (be, br):
        for k, (whole, _, floats) in bufs.items():
            assert guards_intact(whole, floats), k


def test_kernel_stores_rows_to_an_unaligned_d_emb():
    """d_emb 4 bytes off a 16-byte boundary (the scalar stores): the same bits, nothing written around them."""
    from r2l_amd.engine import _ptr, _stream
    n = 33
    c = kernel_case(n, 0.)
    lib, flat, _ = lib_and_params()
    want, _ = call_kernel(c, n, rays=False)
    gx = torch.full((2 * int(lib.r2l_stash_slot_floats(n)),), float("nan"), device="cuda")
    gx[:n * 256] = c["gh"].reshape(-1)
    whole, inner = guarded(n * 1008 + 1)
    assert lib.r2l_backward_input(_ptr(gx), _ptr(flat), 1, None, None, None, None, _ptr(inner[1:]), None, None, n, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(inner[1:].view(n, 1008), want["d_emb"])
    assert guards_intact(whole, n * 1008 + 1) and inner[:1].view(torch.int32).item() == whole.view(torch.int32)[0].item()


def test_kernel_argument_errors():
    from r2l_amd.engine import _ptr, _stream
    n = 33
    c = kernel_case(n, 1.)
    lib, flat, _ = lib_and_params()
    gx = torch.zeros(2 * int(lib.r2l_stash_slot_floats(n)), device="cuda")
    e, do, dd = torch.empty(n, 1008, device="cuda"), torch.empty(n, 3, device="cuda"), torch.empty(n, 3, device="cuda")
    base = dict(gx=gx, par=flat, nb=1, o=c["o"], d=c["d"], u=c["u"], zt=c["ztab"], e=e, do=do, dd=dd, n=n)
    cases = [(dict(e=None, do=None, dd=None), "no output"), (dict(o=None), "ray form"), (dict(d=None), "ray form"),
             (dict(zt=None), "ray form"), (dict(do=None), "go together"), (dict(dd=None), "go together"), (dict(n=0), "N < 1"),
             (dict(n=-1), "N < 1"), (dict(nb=-1), "n_block")]
    for kw, word in cases:
        a = dict(base, **kw)
        rc = lib.r2l_backward_input(_ptr(a["gx"]), _ptr(a["par"]), a["nb"], _ptr(a["o"]), _ptr(a["d"]), _ptr(a["u"]), _ptr(a["zt"]),
                                    _ptr(a["e"]), _ptr(a["do"]), _ptr(a["dd"]), a["n"], _stream())
        assert rc != 0 and word in lib.r2l_last_error().decode(), (kw, rc, lib.r2l_last_error())
    torch.cuda.synchronize()


# ---- (b) end to end against fp64 autograd on mask-stable rays -------------------------------------------------------------------
def e2e_case(nb, n, perturb, path):
    """test_student_backward_gpu.case (selected rays, generic-mode dL/drgb) plus the input gradient's yardstick and magnitudes."""
    key = (nb, n, perturb, path)
    if key not in _E2E:
        c = case(nb, n, perturb, path=path, mode="generic")
        assert c["rejected"] <= S.REJECT_CAP[nb], c["rejected"]
        sd64, drgb = c["sd64"], c["kw"]["drgb64"]
        Wh64 = sd64["head.0.weight"]
        if path == "emb":
            _, gh_abs = U.head_gradient64(sd64, c["emb64"], drgb)
            want, mags = {"d_emb": U.autograd_emb64(sd64, c["emb64"], drgb)}, U.input_mags(gh_abs, Wh64)
        else:
            emb64 = S.reference_encoding(c["o"], c["d"], c["u"], perturb, "cuda")
            _, gh_abs = U.head_gradient64(sd64, emb64, drgb)
            _, z = U.points32(c["o"].cuda(), c["d"].cuda(), c["u"].cuda(), perturb)
            do, dd = U.autograd_rays64(sd64, c["o"], c["d"], c["u"], perturb, drgb)
            want, mags = {"d_rays_o": do, "d_rays_d": dd}, U.input_mags(gh_abs, Wh64, z)
            del mags["d_emb"]
        _E2E[key] = dict(c=c, want=want, mags=mags)
    return _E2E[key]


def frozen_model(sd, nb):
    m = build_model(sd, nb)
    for p in m.parameters():
        p.requires_grad_(False)
    return m


def run_emb_calls(c, nb, n):
    """The library calls of a frozen student's step on the pre-embedded path: forward with stash, the dX chain alone,
    r2l_backward_input."""
    from r2l_amd import _lib
    from r2l_amd.engine import _ptr, _stream, get_engine
    eng = get_engine(build_model(c["sd"], nb))
    eng.ensure_packed()
    lib = eng.lib
    f = dict(dtype=torch.float32, device="cuda")
    emb = c["emb64"].float().contiguous()
    slot = int(lib.r2l_stash_slot_floats(n))
    save_x, save_t = torch.empty((nb + 1) * slot, **f), torch.empty(max(nb, 1) * slot, **f)
    rgb = eng.forward_emb(emb, save=(save_x, save_t))
    wbwd = torch.zeros(lib.r2l_bwd_stream_floats(nb), **f)
    _lib.check(lib.r2l_pack_backward(_ptr(eng.flat), nb, _ptr(wbwd), _stream()), "r2l_pack_backward")
    gx, gt = torch.full(((nb + 1) * slot,), float("nan"), **f), torch.empty(max(nb, 1) * slot, **f)
    dpre = torch.empty(n * 3, **f)
    drgb = c["kw"]["drgb64"].float().contiguous()
    _lib.check(lib.r2l_backward_part_cfg(None, None, None, None, _ptr(emb), _ptr(rgb), None, _ptr(drgb), _ptr(save_x),
                                         _ptr(save_t), _ptr(wbwd), _ptr(eng.flat), nb, 0.0, _ptr(dpre), _ptr(gx), _ptr(gt), None,
                                         _ptr(dpre), None, n, _stream(), _lib.BWD_CHAIN, 0, 2 * nb, eng._cfg()), "r2l_backward (chain)")
    return eng.backward_input(gx, n, want_emb=True)[0]


def run_rays_autograd(c, nb, n, perturb, trainable=False):
    """forward_rays with rays that require grad, loss = sum(rgb * drgb): (d_rays_o, d_rays_d)."""
    m = build_model(c["sd"], nb) if trainable else frozen_model(c["sd"], nb)
    o, d = c["o"].cuda().requires_grad_(True), c["d"].cuda().requires_grad_(True)
    rgb = m.forward_rays(o, d, sampler(), perturb=perturb, t_rand=c["u"].cuda() if perturb > 0 else None)
    assert rgb.requires_grad
    (rgb * c["kw"]["drgb64"].float()).sum().backward()
    torch.cuda.synchronize()
    return {"d_rays_o": o.grad, "d_rays_d": d.grad}, m


def check_e2e(tag, E, got):
    want, mags = E["want"], E["mags"]
    assert all(bool(torch.isfinite(v).all().item()) for v in got.values())
    for k in want:
        print("%s %s: norm-relative %.3g, worst |got - want| / mag %.3g" % (
            tag, k, S.nrel(got[k], want[k]), S.worst_ratio({k: got[k]}, {k: want[k]}, mags)[0]))
    bad = bar_failures(EXACT_FAMILY, got, want, mags, None)
    assert not bad, bad


@pytest.mark.parametrize("tiling", ["main", "coop16"])
@pytest.mark.parametrize("perturb", [0., 1.])
@pytest.mark.parametrize("nb,n", E2E_SHAPES)
def test_emb_path_vs_fp64_autograd(nb, n, perturb, tiling, monkeypatch):
    E = e2e_case(nb, n, perturb, "emb")
    use_family(monkeypatch, tiling=tiling)
    check_e2e("emb n_block %d N %d perturb %g %s" % (nb, n, perturb, tiling), E, {"d_emb": run_emb_calls(E["c"], nb, n)})


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("perturb", [0., 1.])
@pytest.mark.parametrize("nb,n", E2E_SHAPES)
def test_ray_path_vs_fp64_autograd(nb, n, perturb, family, monkeypatch):
    E = e2e_case(nb, n, perturb, "rays")
    use_family(monkeypatch, **FAMILIES[family])
    got, _ = run_rays_autograd(E["c"], nb, n, perturb)
    check_e2e("rays n_block %d N %d perturb %g %s" % (nb, n, perturb, family), E, got)


@pytest.mark.parametrize("family", ["main-f32mfma", "coopf"])
def test_bars_see_one_ray_without_its_head_gradient(family, monkeypatch):
    """Self-check of the bars: the yardstick of the same step with ONE ray's row of gh zeroed (the rays do not interact: that
    ray's rows of the input gradient vanish, every other row stays) must fail the bar on every tensor, with the device's unchanged
    output as `got` — for the probe rays of student_util.  The device is never asked to misbehave."""
    nb, n, perturb = 3, 65, 1.
    use_family(monkeypatch, **FAMILIES[family])
    Er, Ee = e2e_case(nb, n, perturb, "rays"), e2e_case(nb, n, perturb, "emb")
    got, _ = run_rays_autograd(Er["c"], nb, n, perturb)
    pairs = [(Er, got)]
    if family == "main-f32mfma":
        pairs.append((Ee, {"d_emb": run_emb_calls(Ee["c"], nb, n)}))
    for E, g in pairs:
        assert not bar_failures(EXACT_FAMILY, g, E["want"], E["mags"], None)
        for p in S.probe_rays(n):
            want_p = {k: v.clone() for k, v in E["want"].items()}
            mags_p = {k: v.clone() for k, v in E["mags"].items()}
            for k in want_p:
                assert want_p[k][p].abs().max().item() > 0, (p, k, "probe ray without a gradient")
                want_p[k][p] = 0.
                mags_p[k][p] = 0.
            bad = bar_failures(EXACT_FAMILY, g, want_p, mags_p, None)
            assert set(bad) == set(want_p), (p, bad, "the bar does not see ray %d's head gradient missing" % p)


# ---- (c) the autograd surface -----------------------------------------------------------------------------------------------
def test_frozen_student_gives_the_embedding_its_gradient(monkeypatch):
    nb, n, perturb = 3, 65, 1.
    E = e2e_case(nb, n, perturb, "emb")
    use_family(monkeypatch, tiling="main")
    c = E["c"]
    want = run_emb_calls(c, nb, n)
    m = frozen_model(c["sd"], nb)
    emb = c["emb64"].float().reshape(5, 13, 1008).clone().requires_grad_(True)  # (leading dimensions are kept)
    rgb = m(emb)
    assert rgb.shape == (5, 13, 3) and rgb.requires_grad
    (rgb * c["kw"]["drgb64"].float().reshape(5, 13, 3)).sum().backward()
    assert emb.grad is not None and emb.grad.shape == emb.shape
    assert torch.equal(emb.grad.reshape(n, 1008), want)
    assert all(p.grad is None for p in m.parameters())


def test_parameter_gradients_do_not_change_with_an_input_that_requires_grad(monkeypatch):
    nb, n, perturb = 3, 65, 1.
    E = e2e_case(nb, n, perturb, "emb")
    use_family(monkeypatch, tiling="main")
    c = E["c"]
    drgb = c["kw"]["drgb64"].float()
    grads = []
    for need in (False, True):
        m = build_model(c["sd"], nb)
        emb = c["emb64"].float().clone().requires_grad_(need)
        (m(emb) * drgb).sum().backward()
        grads.append([p.grad.clone() for p in m.parameters()])
        if need:
            assert torch.equal(emb.grad, run_emb_calls(c, nb, n))
    assert all(torch.equal(a, b) for a, b in zip(*grads))
    got = dict(zip(c["sd"].keys(), grads[1]))
    assert not bar_failures(EXACT_FAMILY, got, c["want"], c["mags"], c["e_model"])


@pytest.mark.parametrize("family", ["main-f32mfma", "coopf", "coop16"])
def test_trainable_student_gets_ray_and_parameter_gradients(family, monkeypatch):
    """forward_rays, rays that require grad, parameters trainable: the rays' gradients are the frozen student's bit for bit, and
    the parameters' pass the bars of their family in tests/test_student_backward_gpu.py (generic mode)."""
    nb, n, perturb = 3, 65, 1.
    E = e2e_case(nb, n, perturb, "rays")
    c = E["c"]
    use_family(monkeypatch, **FAMILIES[family])
    frozen, _ = run_rays_autograd(c, nb, n, perturb)
    got, m = run_rays_autograd(c, nb, n, perturb, trainable=True)
    assert torch.equal(got["d_rays_o"], frozen["d_rays_o"]) and torch.equal(got["d_rays_d"], frozen["d_rays_d"])
    grads = {k: p.grad for k, p in zip(c["sd"].keys(), m.parameters())}
    assert all(g is not None for g in grads.values())
    bad = bar_failures(family, grads, c["want"], c["mags"], c["e_model"], c, None)
    assert not bad, dict(list(bad.items())[:6])


def test_pose_gradient_through_forward_rays(monkeypatch):
    """Pose refinement's set-up: a frozen student, rays from a pose through torch (rays_d = dirs R^T), d loss / d pose against
    fp64 autograd through the oracle on mask-stable pixels; per entry of the 3 x 4 within NREL_BWD of the matrix's norm.  The fp64
    side takes the fp32 values of rays and points the device saw and the exact Jacobians of the operations that made them."""
    from model.nerf_raybased import PointSampler
    use_family(monkeypatch)  # the library's own choice of family
    nb, n = 3, 200
    sd = O.make_state_dict(n_block=nb, seed=S.NET_SEED)
    sd64 = S.f64(sd, "cuda")
    ps = PointSampler(64, 64, 80., S.N_SAMPLE, S.NEAR, S.FAR, device="cuda")
    pose0 = torch.as_tensor(O.pose_spherical(30., -30., 4.), dtype=torch.float32)[:3, :4].cuda()
    dirs = ps.dirs.reshape(-1, 3)
    rays_of = lambda pose, dr: (pose[:3, 3].expand(dr.shape[0], 3), (dr[:, None, :] * pose[:3, :3]).sum(-1))
    with torch.no_grad():  # the mask-stable pixels of the frame, decided by the fp64 forward alone
        o_all, d_all = rays_of(pose0, dirs)
        pts_all, _ = U.points32(o_all, d_all, None, 0.)
        idx = torch.nonzero(S.stable_rays(sd64, S.encode64(pts_all, "cuda"), S.DELTA[nb])).flatten()
        assert idx.numel() >= n and 1.0 - idx.numel() / dirs.shape[0] <= S.REJECT_CAP[nb]
        idx = idx[:n]
    dr = dirs[idx].contiguous()
    drgb = (torch.randn(n, 3, generator=torch.Generator().manual_seed(9)) * 1e-3).cuda()
    m = frozen_model(sd, nb)
    pose = pose0.clone().requires_grad_(True)
    o, d = rays_of(pose, dr)
    rgb = m.forward_rays(o, d, ps, perturb=0.)
    (rgb * drgb).sum().backward()
    torch.cuda.synchronize()
    # fp64
    pose64 = pose0.double().requires_grad_(True)
    o64, d64 = rays_of(pose64, dr.double())
    o64 = o64 + (o.detach().double() - o64).detach()
    d64 = d64 + (d.detach().double() - d64).detach()
    pts32, _ = U.points32(o.detach(), d.detach(), None, 0.)
    with torch.device("cuda"):
        pts = O.sample_train(o64, d64, O.z_vals(S.N_SAMPLE, S.NEAR, S.FAR).double(), 0., None)
        pts = pts + (pts32.double() - pts).detach()
        want = torch.autograd.grad((O.r2l_forward(sd64, O.positional_embed(pts, 10)) * drgb.double()).sum(), pose64)[0]
    err = (pose.grad.double() - want).abs().max().item()
    print("pose gradient: worst entry %.3g of the norm (bar %.3g)" % (err / want.norm().item(), S.NREL_BWD))
    assert want.norm().item() > 0 and err <= S.NREL_BWD * want.norm().item()


def test_forward_rays_with_plain_tensors_is_unchanged(monkeypatch):
    """No ray requires grad: the forward-only launch, its bits, and no graph — parameters trainable or not."""
    use_family(monkeypatch)  # the library's own choice of family
    nb, n, perturb = 3, 65, 1.
    E = e2e_case(nb, n, perturb, "rays")
    c = E["c"]
    m = build_model(c["sd"], nb)
    ps = sampler()
    o, d, u = c["o"].cuda(), c["d"].cuda(), c["u"].cuda()
    rgb = m.forward_rays(o, d, ps, perturb=perturb, t_rand=u)
    assert not rgb.requires_grad and rgb.grad_fn is None
    assert torch.equal(rgb, m.engine().forward_rays(o, d, ps.z_vals, perturb, u))
    with torch.no_grad():  # grad mode off: rays that require grad build no graph either
        rgb2 = m.forward_rays(o.clone().requires_grad_(True), d, ps, perturb=perturb, t_rand=u)
    assert rgb2.grad_fn is None and torch.equal(rgb2, rgb)
