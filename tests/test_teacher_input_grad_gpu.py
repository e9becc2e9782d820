"""r2l_teacher_backward_input and r2l_raw2outputs_backward_scaled through the C ABI, and TeacherRayGrad / render_rays_diff on
top of them, against the fp64 restatements of r2l_amd/teacher_input_grad.py (bars: tests/teacher_input_grad_util.py)."""
import pytest
import torch

from r2l_amd import teacher_input_grad as TI
from tests import teacher_input_grad_util as U
from tests.test_teacher_backward_gpu import (C_R2O, C_R2O_LOGITS, NREL_BWD, Net, guarded, guards_intact, inputs, r2o_inputs,
                                             raw2outputs64, untouched, weights)

pytestmark = pytest.mark.gpu


def _L():
    from r2l_amd import _lib as L
    return L


def _p(t):
    return _L().ptr(t)


def _s():
    return _L().stream()


_CASES = {}


def case(R, S, kind):
    """Forward with stash, a draw and a d_len of one shape, the fp64 want and the magnitudes with and without the d_len / fold
    terms: computed once per process and left unchanged."""
    key = (R, S, kind)
    if key not in _CASES:
        sd = weights(kind)
        net = Net(sd)
        o, d, vd, z = [t.cuda() for t in inputs(R, S, kind)]
        raw, _, stash, _ = net.forward_stash(o, d, vd, z)
        draw = U.make_draw(raw, R * 1000 + S).cuda()
        d_len = U.make_d_len(R, S).cuda()
        masks = TI.stash_masks(stash, R * S)
        c = dict(sd=sd, net=net, o=o, d=d, vd=vd, z=z, stash=stash, draw=draw, d_len=d_len, masks=masks)
        c["want"] = {f: U.want64(sd, o, d, vd, z, masks, draw, d_len if f else None, f) for f in (False, True)}
        c["mags"] = {f: U.mags64(sd, o, d, vd, z, masks, draw, d_len if f else None, f) for f in (False, True)}
        _CASES.clear()  # (one case at a time: the largest holds 2 GB of fp64)
        _CASES[key] = c
    return _CASES[key]


def call(c, full=True, want=("d_rays_o", "d_rays_d", "d_viewdirs", "d_pts"), with_len=None, fold=None):
    """One call with every output and the work buffer between sentinel guards; the work buffer is of exactly
    r2l_teacher_input_grad_work_floats(P) floats and holds NaN.  Returns (rc, {name: (whole, interior)}, (work_whole, n_work))."""
    lib = _L().load()
    R, S = c["z"].shape
    sizes = dict(d_rays_o=R * 3, d_rays_d=R * 3, d_viewdirs=R * 3, d_pts=R * S * 3)
    bufs = {k: guarded(n) for k, n in sizes.items()}
    n_work = lib.r2l_teacher_input_grad_work_floats(R * S)
    w_whole, work = guarded(n_work)
    work.fill_(float("nan"))
    arg = lambda k: _p(bufs[k][1]) if k in want else None
    with_len, fold = full if with_len is None else with_len, full if fold is None else fold
    rc = lib.r2l_teacher_backward_input(_p(c["o"]), _p(c["d"]), _p(c["vd"]), _p(c["z"]), _p(c["net"].flat), _p(c["stash"]),
                                        _p(c["draw"]), _p(c["d_len"]) if with_len else None, int(fold), arg("d_rays_o"), arg("d_rays_d"),
                                        arg("d_viewdirs"), arg("d_pts"), _p(work), R, S, _s())
    torch.cuda.synchronize()
    return rc, bufs, (w_whole, n_work)


def shaped(bufs, R, S):
    return {k: v[1].view(R, S, 3) if k == "d_pts" else v[1].view(R, 3) for k, v in bufs.items()}


@pytest.mark.parametrize("kind", ["init", "trained"])
@pytest.mark.parametrize("R,S", U.SHAPES)
def test_backward_input_vs_fp64(R, S, kind):
    """Every entry of d_pts, d_rays_o, d_rays_d and d_viewdirs against the fp64 spec run from the device's own stash at the
    fp32-rounded points, with and without d_len / fold_viewdirs: |got - want| <= C_IN mag + floor per entry and norm-relative
    NREL_BWD per tensor; guards intact; a second call gives the same bits."""
    c = case(R, S, kind)
    for full in (True, False):
        rc, bufs, (w_whole, n_work) = call(c, full)
        assert rc == 0
        for k, (whole, inner) in bufs.items():
            assert guards_intact(whole, inner.numel()), "write outside " + k
            assert bool(torch.isfinite(inner).all().item()), "an entry of %s was not written" % k
        assert guards_intact(w_whole, n_work), "write outside work"
        got, want, mags = shaped(bufs, R, S), c["want"][full], c["mags"][full]
        ratio = {k: v.max().item() for k, v in U.ratios(got, want, mags).items()}
        rel = {k: U.nrel(got[k], want[k]) for k in got}
        print("backward_input (%d, %d) %s full %d: |got - want| / mag %s   norm-relative %s" % (
            R, S, kind, full, " ".join("%s %.3g" % kv for kv in ratio.items()), " ".join("%s %.3g" % kv for kv in rel.items())))
        bad = {k: int(v.sum().item()) for k, v in U.violations(got, want, mags).items() if v.any()}
        assert not bad, bad
        assert max(rel.values()) <= NREL_BWD, rel
        if full:
            _, again, _ = call(c, full)
            assert all(torch.equal(again[k][1].view(torch.int32), bufs[k][1].view(torch.int32)) for k in bufs), "not reproducible"


@pytest.mark.parametrize("kind", ["init", "trained"])
@pytest.mark.parametrize("with_len,fold", [(True, False), (False, True)])
def test_d_len_and_fold_each_alone(with_len, fold, kind):
    """d_len given with fold_viewdirs = 0, and fold_viewdirs = 1 without d_len, at (37, 61): d_rays_d under the bars of the test
    above, the other outputs the bits of the call with both."""
    c = case(37, 61, kind)
    R, S = 37, 61
    _, both, _ = call(c, True)
    rc, bufs, (w_whole, n_work) = call(c, True, with_len=with_len, fold=fold)
    assert rc == 0 and guards_intact(w_whole, n_work)
    o, d, vd, z = c["o"], c["d"], c["vd"], c["z"]
    want = U.want64(c["sd"], o, d, vd, z, c["masks"], c["draw"], c["d_len"] if with_len else None, fold)
    mags = U.mags64(c["sd"], o, d, vd, z, c["masks"], c["draw"], c["d_len"] if with_len else None, fold)
    got = shaped(bufs, R, S)
    assert (want["d_rays_d"] - c["want"][True]["d_rays_d"]).abs().max().item() > 0  # the variant is another number
    bad = {k: int(v.sum().item()) for k, v in U.violations(got, want, mags).items() if v.any()}
    assert not bad, bad
    assert U.nrel(got["d_rays_d"], want["d_rays_d"]) <= NREL_BWD
    for k in ("d_rays_o", "d_viewdirs", "d_pts"):
        assert torch.equal(bufs[k][1].view(torch.int32), both[k][1].view(torch.int32)), k


@pytest.mark.parametrize("kind", ["init", "trained"])
@pytest.mark.parametrize("R,S", U.SELF_CHECK_SHAPES)
def test_bar_sees_one_missing_sample(R, S, kind):
    """Self-check of the bar: a want with ONE sample of one ray left out of the sums (its draw zeroed: points do not interact)
    must fail it, and in that ray's entries only.  The sample is the one of the middle ray with the largest |d_pts|."""
    c = case(R, S, kind)
    rc, bufs, _ = call(c, True)
    got, want, mags = shaped(bufs, R, S), c["want"][True], c["mags"][True]
    assert rc == 0 and not any(v.any() for v in U.violations(got, want, mags).values())
    r = R // 2
    s = int(want["d_pts"][r].abs().amax(-1).argmax().item())
    draw_p = c["draw"].clone()
    draw_p[r, s] = 0.
    want_p = U.want64(c["sd"], c["o"], c["d"], c["vd"], c["z"], c["masks"], draw_p, c["d_len"], True)
    viol = U.violations(got, want_p, mags)
    for k in ("d_rays_o", "d_rays_d", "d_viewdirs"):
        assert bool(viol[k][r].any().item()), (k, "the bar does not see sample %d of ray %d missing" % (s, r))
    assert bool(viol["d_pts"][r, s].any().item())
    for k, v in viol.items():
        v = v.clone()
        if k == "d_pts":
            v[r, s] = False
        else:
            v[r] = False
        assert not bool(v.any().item()), (k, "an entry of another ray fails")


def test_optional_outputs_absent_in_turn():
    """Each optional output absent in turn: its buffer is untouched, the others hold the bits of the full call (d_rays_d with
    fold_viewdirs too, whether or not d_viewdirs is returned)."""
    c = case(3, 43, "init")
    _, full, _ = call(c, True)
    for want in (("d_rays_o", "d_rays_d", "d_viewdirs"), ("d_rays_o", "d_rays_d", "d_pts"), ("d_viewdirs", "d_pts"), ("d_pts",),
                 ("d_viewdirs",), ("d_rays_o", "d_rays_d")):
        rc, bufs, (w_whole, n_work) = call(c, True, want)
        assert rc == 0 and guards_intact(w_whole, n_work)
        for k, (whole, inner) in bufs.items():
            if k in want:
                assert torch.equal(inner.view(torch.int32), full[k][1].view(torch.int32)), (want, k)
                assert guards_intact(whole, inner.numel())
            else:
                assert untouched(whole), (want, k)


def test_no_rays_and_refusals():
    """R = 0 succeeds and writes nothing; every refusal returns non-zero with a message and writes nothing."""
    lib = _L().load()
    c = case(3, 43, "init")
    R, S = 3, 43
    outs = [guarded(R * S * 3) for _ in range(4)]
    w_whole, work = guarded(lib.r2l_teacher_input_grad_work_floats(R * S))
    base = [_p(c["o"]), _p(c["d"]), _p(c["vd"]), _p(c["z"]), _p(c["net"].flat), _p(c["stash"]), _p(c["draw"]), _p(c["d_len"]), 1]
    po = [_p(b[1]) for b in outs]

    def run(args, outp, Rr, Ss, wk=True):
        rc = lib.r2l_teacher_backward_input(*args, *outp, _p(work) if wk else None, Rr, Ss, _s())
        torch.cuda.synchronize()
        assert untouched(w_whole) and all(untouched(b[0]) for b in outs)
        return rc, lib.r2l_last_error().decode()
    assert run(base, po, 0, S)[0] == 0
    assert lib.r2l_teacher_input_grad_work_floats(-1) == -1 and lib.r2l_teacher_input_grad_work_floats(0) == 0
    rc, msg = run(base, [None] * 4, R, S)
    assert rc != 0 and "no output" in msg
    for outp in ([po[0], None, None, None], [None, po[1], po[2], po[3]]):
        rc, msg = run(base, outp, R, S)
        assert rc != 0 and "together" in msg
    for Ss in (0, 257):
        rc, msg = run(base, po, R, Ss)
        assert rc != 0 and "1 <= S <= 256" in msg
    rc, msg = run(base, po, -1, S)
    assert rc != 0 and "R >= 0" in msg
    for i in range(7):  # rays_o, rays_d, viewdirs, z, tparams, stash, draw
        rc, msg = run(base[:i] + [None] + base[i + 1:], po, R, S)
        assert rc != 0 and "NULL" in msg, i
    rc, msg = run(base, po, R, S, wk=False)
    assert rc != 0 and "NULL" in msg


# ---- the scaled raw2outputs backward ----------------------------------------------------------------------------------------------
def _r2o(R, S):
    white, with_noise = (R + S) % 2 == 0, S % 3 != 0
    raw, z, d, noise, tgt = r2o_inputs(R, S, with_noise)
    if R >= 3 and S > 1:
        raw[0, :, 3] = -raw[0, :, 3].abs() - (0. if noise is None else noise[0].abs())  # no density at all: d_len = 0
        raw[2, 0, 3] = 1e4  # an opaque first sample: alpha = 1 exactly (exp(-1e4 * 0.25 |d|) underflows in fp32, |d| >= 0.05) ..
        z[2, 0] = z[2, 1] - 0.25  # .. whatever the draw of z; a nearly opaque one would test fp32's 1 - alpha, not d_len
        if noise is not None:
            noise[2, 0] = 0.
    return white, raw, z, d, noise, tgt


def _scaled(dev, white, g, scale, R, S, want_len=True):
    lib = _L().load()
    dr_whole, draw = guarded(R * S * 4)
    sq_whole, sq = guarded(R)
    dl_whole, dl = guarded(R)
    rc = lib.r2l_raw2outputs_backward_scaled(_p(dev[0]), _p(dev[1]), _p(dev[2]), _p(dev[3]), int(white), _p(dev[4]), _p(g), scale,
                                             _p(draw), _p(sq), _p(dl) if want_len else None, R, S, _s())
    torch.cuda.synchronize()
    assert rc == 0, lib.r2l_last_error()
    assert guards_intact(dr_whole, R * S * 4) and guards_intact(sq_whole, R) and guards_intact(dl_whole, R)
    return draw, sq, dl, (sq_whole, dl_whole)


@pytest.mark.parametrize("R", [1, 3, 4, 5, 45])
@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 128, 255, 256])
def test_raw2outputs_backward_keeps_its_bits(S, R):
    """r2l_raw2outputs_backward is the scaled form at g = NULL, d_len = NULL, grad_scale = (float)(2.0 / (3.0 R)): draw and sqerr
    bit for bit (with and without d_len asked for)."""
    lib = _L().load()
    white, raw, z, d, noise, tgt = _r2o(R, S)
    dev = [None if t is None else t.cuda() for t in (raw, z, d, noise, tgt)]
    draw0, sq0 = torch.empty(R * S * 4, device="cuda"), torch.empty(R, device="cuda")
    _L().check(lib.r2l_raw2outputs_backward(_p(dev[0]), _p(dev[1]), _p(dev[2]), _p(dev[3]), int(white), _p(dev[4]), _p(draw0),
                                            _p(sq0), R, S, _s()), "r2l_raw2outputs_backward")
    scale = torch.tensor(2.0 / (3.0 * R), dtype=torch.float64).float().item()
    for want_len in (False, True):
        draw, sq, _, _ = _scaled(dev, white, None, scale, R, S, want_len)
        assert torch.equal(draw.view(torch.int32), draw0.view(torch.int32)) and torch.equal(sq.view(torch.int32), sq0.view(torch.int32))


@pytest.mark.parametrize("seeded", [False, True])
@pytest.mark.parametrize("R", [1, 3, 4, 5, 45])
@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 128, 255, 256])
def test_raw2outputs_backward_scaled_vs_fp64(S, R, seeded):
    """draw under an arbitrary grad_scale and under a g seed against fp64 autograd of the oracle (the bars of
    test_raw2outputs_backward_edges: 2e-5 of the ray's largest |draw|, 1e-3 on the rays with colour logits of +-10), and d_len
    per ray against fp64 within the same factors of sum_s |draw3| relu(sigma') / |d|.  A ray without density has d_len = 0.
    d_len is held to fp64 on the rays with trained-like magnitudes too (sigma up to 10^3, nearly opaque samples in mid-ray): the
    kernel forms it from a transmittance of its own, exp(-x) + 1e-10, not from fp32's 1 - alpha."""
    white, raw, z, d, noise, tgt = _r2o(R, S)
    dev = [None if t is None else t.cuda() for t in (raw, z, d, noise, tgt)]
    scale = 0.4375
    g = (torch.randn(R, 3, generator=torch.Generator().manual_seed(S)) * 0.5) if seeded else None
    gd = None if g is None else g.cuda()
    draw, sq, dl, (sq_whole, _) = _scaled(dev, white, gd, scale, R, S)
    if seeded:
        assert untouched(sq_whole), "sqerr written under a g seed"
    raw64 = raw.double().requires_grad_(True)
    unit = torch.nn.functional.normalize(d.double(), dim=-1)
    length = d.double().norm(dim=-1, keepdim=True).requires_grad_(True)
    n64 = None if noise is None else noise.double()
    rgb = raw2outputs64(raw64, z.double(), unit * length, n64, white)
    loss = (rgb * g.double()).sum() if seeded else 0.5 * scale * ((rgb - tgt.double())**2).sum()
    want, want_len = torch.autograd.grad(loss, [raw64, length])
    got = draw.view(R, S, 4).cpu().double()
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(dl).all())
    logits = torch.tensor([(r + S) % 6 == 4 for r in range(R)])
    c = torch.where(logits, C_R2O_LOGITS, C_R2O).double()
    ray_max = want.abs().amax(dim=(1, 2))
    err = (got - want).abs().amax(dim=(1, 2))
    sig = raw64.detach()[..., 3] + (0. if n64 is None else n64)
    len_unit = (want[..., 3].abs() * torch.relu(sig)).sum(-1) / length.detach()[:, 0]
    len_err = (dl.cpu().double() - want_len[:, 0]).abs()
    print("scaled raw2outputs backward (%d, %d) seeded %d: draw / ray max %.3g, d_len / unit %.3g" % (
        R, S, seeded, (err / ray_max.clamp_min(1e-300) / c * C_R2O).max().item(),
        (len_err / len_unit.clamp_min(1e-300) / c * C_R2O)[len_unit > 0].max().item() if (len_unit > 0).any() else 0.))
    assert bool((err <= c * ray_max + 1e-30).all())
    assert bool((len_err <= c * len_unit + 1e-30).all()), (len_err, len_unit)
    if R >= 3 and S > 1:
        assert dl[0].item() == 0.
    if not seeded:
        diff = rgb.detach() - tgt.double()
        sq_err = (sq.cpu().double() - (diff**2).sum(-1)).abs()
        assert bool((sq_err <= 1e-6 * ((diff**2).sum(-1) + diff.abs().sum(-1))).all())


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def _e2e_want(rg, st, sds, tgt, s, g, fold):
    """The fp64 restatement from both device stashes, the device's raw and last_z: (want, mags) summed over the networks."""
    o, d, vd = st["rays"]
    R = o.shape[0]
    tot, mag = {}, {}
    for i, sd in enumerate(sds):
        z = st["z"][i]
        draw, _, d_len, _ = TI.raw2outputs_backward_spec(st["raw"][i].double(), z.double(), d.double(), st["noise"][i], rg.white_bkgd,
                                                         None if tgt is None else tgt.double(), None if g is None else g[i].double(), s)
        masks = TI.stash_masks(st["stash"][i], R * z.shape[1])
        w = U.want64(sd, o, d, vd, z, masks, draw, d_len, fold)
        m = U.mags64(sd, o, d, vd, z, masks, draw, d_len, fold)
        for k in ("d_rays_o", "d_rays_d", "d_viewdirs"):
            tot[k] = tot.get(k, 0.) + w[k]
            mag[k] = mag.get(k, 0.) + m[k]
    return tot, mag


@pytest.mark.parametrize("R,NS,NI", [(65, 16, 32), (3, 64, 128)])
def test_teacher_ray_grad_end_to_end(R, NS, NI):
    """TeacherRayGrad.loss_and_grad on the trained-like pair against the fp64 spec run from both device stashes and the device's
    last_z, under the kernel tests' bars; render_rays_diff(...).backward() fills .grad of the three ray tensors with the values
    its own fp64 restatement gives."""
    from tests.teacher_util import scene_rays, trained_like_pair
    sds = trained_like_pair()
    nets = [U.nerf_module(sd, torch.float32).cuda() for sd in sds]
    rb = scene_rays(181 * 181, 0)[torch.randperm(181 * 181, generator=torch.Generator().manual_seed(R))[:R]].cuda()
    o, d, vd = rb[:, 0:3].contiguous(), rb[:, 3:6].contiguous(), rb[:, 8:11].contiguous()
    tgt = torch.rand(R, 3, generator=torch.Generator().manual_seed(1)).cuda()
    rg = TI.TeacherRayGrad(nets[0], nets[1], NS, NI, True)
    s = 2.0 / (3.0 * R)
    loss_out, d_o, d_d, d_vd = rg.loss_and_grad(o, d, vd, 2., 6., tgt, fold_viewdirs=True)
    got = dict(d_rays_o=d_o.clone(), d_rays_d=d_d.clone(), d_viewdirs=d_vd.clone())
    assert len(rg.last_z) == 2 and rg.last_z[1].shape == (R, NS + NI)
    want, mags = _e2e_want(rg, rg.last_state, sds, tgt, s, None, True)
    bad = {k: int(v.sum().item()) for k, v in U.violations(got, want, mags).items() if v.any()}
    rel = {k: U.nrel(got[k], want[k]) for k in got}
    print("loss_and_grad (%d, %d, %d): |got - want| / mag %s  norm-relative %s" % (
        R, NS, NI, {k: "%.3g" % v.max().item() for k, v in U.ratios(got, want, mags).items()}, rel))
    assert not bad, bad
    assert max(rel.values()) <= NREL_BWD, rel
    sq = sum(x.double().sum() for x in rg.last_sqerr)
    assert abs(loss_out[0].item() - 0.5 * s * sq.item()) <= 1e-5 * 0.5 * s * sq.item()
    # the autograd function, under a loss of the caller's own
    lo, ld, lv = [t.clone().requires_grad_(True) for t in (o, d, vd)]
    rgb, rgb0 = TI.render_rays_diff(lo, ld, lv, 2., 6., nets[0], nets[1], NS, NI, True)
    gen = torch.Generator().manual_seed(2)
    G1, G0 = torch.randn(R, 3, generator=gen).cuda(), torch.randn(R, 3, generator=gen).cuda()
    ((rgb * G1).sum() + (rgb0 * G0).sum()).backward()
    rg2 = nets[0].__dict__["_r2l_ray_grad"][(id(nets[1]), NS, NI, True, 0.)]
    st = rg2.forward(o, d, vd, 2., 6.)
    want, mags = _e2e_want(rg2, st, sds, None, 0., [G0, G1], False)
    got = dict(d_rays_o=lo.grad, d_rays_d=ld.grad, d_viewdirs=lv.grad)
    bad = {k: int(v.sum().item()) for k, v in U.violations(got, want, mags).items() if v.any()}
    assert not bad, bad
    assert max(U.nrel(got[k], want[k]) for k in got) <= NREL_BWD
    # two renders, then the backward of the first: its raw and stash are gone, and that is an error, not a wrong gradient
    first = TI.render_rays_diff(lo, ld, lv, 2., 6., nets[0], nets[1], NS, NI, True)[0]
    TI.render_rays_diff(lo, ld, lv, 2., 6., nets[0], nets[1], NS, NI, True)
    with pytest.raises(RuntimeError, match="before rendering again"):
        first.sum().backward()
    TI.release_ray_grad(nets[0])
    assert "_r2l_ray_grad" not in nets[0].__dict__
