"""The teacher-training kernels through the C ABI at every tile and chunk edge, against fp64 (csrc/r2l_teacher_train.hip,
csrc/r2l_teacher_mlp.hip):
  r2l_teacher_backward      per element against tests/teacher_util.teacher_backward_from_stash (fp64 backprop from the device's
                            own stash), with a self-check that the bar sees one missing point, and buffer bounds;
  r2l_teacher_mlp_train     raw bit-equal to the inference kernel, every stash slot against an fp64 forward, buffer bounds;
  r2l_raw2outputs_backward  draw and sqerr per ray against fp64 autograd of the oracle, the degenerate rows, the refusals.
The shapes are chosen from the points a backward can be cut at, not from how today's kernels cut it: P < 16, one 2048-point chunk
and one point more, a 128-row tile and one row more, tails in all of them at once, and a step of the size the trainer runs."""
import ctypes

import pytest
import torch

from oracle import r2l_oracle as O
from tests.teacher_util import (layer_outputs, scene_rays, stash_slots, teacher_backward_from_stash, trained_like_pair)

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF  # a quiet-NaN bit pattern: what an unwritten entry still holds after the call
GUARD = 4096  # floats of sentinel on each side of a buffer

# (R, S): P = R S points.  The edges: P < 16; one 128-row tile + 1; exactly one 2048-point chunk; one chunk + 1; tails of the
# chunk, the 128-row tile and the 16-deep step at once; several chunks + tail at the fine sample count; 96 chunks + 1344 points.
SHAPES = [(1, 1), (1, 15), (3, 43), (32, 64), (2049, 1), (37, 61), (45, 192), (1031, 192)]
# Per-element bar of the network backward: |got - want| <= C_BWD * magnitude + floor (magnitude: the absolute backprop).
C_BWD = 3e-6
NREL_BWD = 1e-5


def _lib():
    from r2l_amd import _lib as L
    return L


def _p(t):
    from r2l_amd.engine import _ptr
    return _ptr(t)


def _s():
    from r2l_amd.engine import _stream
    return _stream()


def guarded(n):
    """(whole, interior): n floats between two GUARD-float guards, all holding the SENTINEL bit pattern."""
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    return whole, whole[GUARD:GUARD + n]


def guards_intact(whole, n):
    bits = whole.view(torch.int32)
    return bool((bits[:GUARD] == SENTINEL).all().item()) and bool((bits[GUARD + n:] == SENTINEL).all().item())


def untouched(whole):
    return bool((whole.view(torch.int32) == SENTINEL).all().item())


def weights(kind):
    if kind == "init":
        return O.make_teacher_state_dicts(5, 1, alpha_bias=0.5)[0]
    return trained_like_pair()[0]


def inputs(R, S, kind, seed=0):
    """(o, d, viewdirs, z) on the CPU, fp32: random rays for the init weights, rays through the scene for the trained-like."""
    g = torch.Generator().manual_seed(seed * 7919 + R * 31 + S)
    if kind == "init":
        o = torch.randn(R, 3, generator=g) * 0.5
        d = torch.randn(R, 3, generator=g)
        vd = d / d.norm(dim=-1, keepdim=True)
    else:
        rb = scene_rays(181 * 181, 0)
        rb = rb[torch.randint(0, 181 * 181, (R,), generator=g)]
        o, d, vd = rb[:, 0:3].contiguous(), rb[:, 3:6].contiguous(), rb[:, 8:11].contiguous()
    z = torch.sort(torch.rand(R, S, generator=g) * 4 + 2, -1)[0]
    return o, d, vd, z


class Net:
    """One teacher's flat parameters (state_dict order) and packed stream on the device."""

    def __init__(self, sd):
        lib = _lib().load()
        self.sd = sd
        self.flat = torch.cat([v.reshape(-1) for v in sd.values()]).float().cuda()
        assert self.flat.numel() == lib.r2l_teacher_param_count()
        self.wstream = torch.zeros(lib.r2l_teacher_stream_floats(), dtype=torch.float32, device="cuda")
        _lib().check(lib.r2l_pack_teacher(_p(self.flat), _p(self.wstream), _s()), "r2l_pack_teacher")

    def forward_stash(self, o, d, vd, z):
        """(raw, stash_whole, stash, raw_whole) of r2l_teacher_mlp_train, both outputs between sentinel guards."""
        lib = _lib().load()
        R, S = z.shape
        n_st = lib.r2l_teacher_stash_floats(R * S)
        st_whole, st = guarded(n_st)
        raw_whole, raw = guarded(R * S * 4)
        _lib().check(lib.r2l_teacher_mlp_train(_p(o), _p(d), _p(vd), _p(z), _p(self.wstream), _p(self.flat), _p(raw), _p(st),
                                               R, S, _s()), "r2l_teacher_mlp_train")
        return raw.view(R, S, 4), st_whole, st, raw_whole

    def forward_infer(self, o, d, vd, z):
        lib = _lib().load()
        R, S = z.shape
        raw = torch.empty(R, S, 4, device="cuda")
        cfg = _lib().make_config(precision="fp32_mfma")
        _lib().check(lib.r2l_teacher_mlp_cfg(_p(o), _p(d), _p(vd), _p(z), _p(self.wstream), _p(self.flat), _p(raw), R, S, _s(),
                                             ctypes.byref(cfg)), "r2l_teacher_mlp_cfg")
        return raw

    def backward(self, o, d, vd, z, stash, draw):
        """(grads, grads_whole, work_whole, n_work): r2l_teacher_backward into an interior slice of a sentinel buffer, with a
        work buffer of exactly r2l_teacher_train_work_floats(P) floats between guards."""
        lib = _lib().load()
        R, S = z.shape
        n = self.flat.numel()
        g_whole, grads = guarded(n)
        n_work = lib.r2l_teacher_train_work_floats(R * S)
        w_whole, work = guarded(n_work)
        _lib().check(lib.r2l_teacher_backward(_p(o), _p(d), _p(vd), _p(z), _p(self.flat), _p(stash), _p(draw), _p(grads),
                                              _p(work), R, S, _s()), "r2l_teacher_backward")
        return grads, g_whole, w_whole, n_work


def split(flat, sd):
    out, off = {}, 0
    for k, v in sd.items():
        out[k] = flat[off:off + v.numel()].view(v.shape)
        off += v.numel()
    return out


def nrel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300)).item()


def bar_violations(got, want, mags):
    """{tensor: number of entries with |got - want| > C_BWD * mag + floor}; the floor only keeps underflow out."""
    out = {}
    for k in want:
        floor = 1e-12 * mags[k].max().item() + 1e-30
        out[k] = int(((got[k].double() - want[k]).abs() > C_BWD * mags[k] + floor).sum().item())
    return out


def worst_ratio(got, want, mags):
    r = 0.
    for k in want:
        m = mags[k]
        e = (got[k].double() - want[k]).abs()
        ok = m > 1e-12 * m.max()
        if ok.any():
            r = max(r, (e[ok] / m[ok]).max().item())
    return r


def probe_points(P):
    """The points a missing tail would lose first: the first, the last of chunk 0, the first of chunk 1, the last of the last
    full 128-row tile and the last point."""
    return sorted({0, 2047, 2048, (P // 128) * 128 - 1, P - 1})


def make_draw(R, S, seed, keep_rays=()):
    """Random dL/draw with a few whole rays zeroed (never one of keep_rays)."""
    g = torch.Generator().manual_seed(seed)
    draw = torch.randn(R, S, 4, generator=g) * 1e-3
    for r in (1, R // 2 + 1):
        if 0 < r < R - 1 and r not in keep_rays:
            draw[r] = 0.
    return draw


def run_backward_case(R, S, kind, real_draw=True):
    """Forward with stash, a draw, the device backward and the fp64 yardstick of one shape.  The draw is random with a few rays
    zeroed, except at (45, 192) with real_draw: there it is the raw2outputs backward of the forward's own raw."""
    lib = _lib().load()
    sd = weights(kind)
    net = Net(sd)
    o, d, vd, z = [t.cuda() for t in inputs(R, S, kind)]
    raw, _, stash, _ = net.forward_stash(o, d, vd, z)
    P = R * S
    if real_draw and (R, S) == (45, 192):  # a real seed: img2mse + raw2outputs backward of the forward's own raw
        tgt = torch.rand(R, 3, generator=torch.Generator().manual_seed(9)).cuda()
        draw = torch.empty(R, S, 4, device="cuda")
        sq = torch.empty(R, device="cuda")
        _lib().check(lib.r2l_raw2outputs_backward(_p(raw), _p(z), _p(d), None, 1, _p(tgt), _p(draw), _p(sq), R, S, _s()),
                     "r2l_raw2outputs_backward")
    else:
        draw = make_draw(R, S, R * 1000 + S, keep_rays={p // S for p in probe_points(P)}).cuda()
    grads, g_whole, w_whole, n_work = net.backward(o, d, vd, z, stash, draw)
    want, mags = teacher_backward_from_stash(sd, o, d, vd, z, stash, draw, device="cuda")
    return dict(net=net, sd=sd, o=o, d=d, vd=vd, z=z, stash=stash, draw=draw, grads=grads, g_whole=g_whole, w_whole=w_whole,
                n_work=n_work, want=want, mags=mags, got=split(grads, sd))


@pytest.mark.parametrize("kind", ["init", "trained"])
@pytest.mark.parametrize("R,S", SHAPES)
def test_teacher_backward_vs_fp64(R, S, kind):
    """r2l_teacher_backward per element against the fp64 yardstick (same masks and activations: only fp32 rounding is left).
    Bars per tensor: |got - want| <= 3e-6 * magnitude per entry, and norm-relative <= 1e-5 for every tensor of more than one
    entry (alpha_linear.bias is one sum that cancels to 2 % of its magnitude under the real draw at (45, 192): 3.6e-5 relative
    there, held by its per-entry bar).  Measured on one MI355X over the whole table, both weight sets: worst |got - want| /
    magnitude 6.9e-7, norm-relative 1.6e-6 (tensors of more than one entry)."""
    c = run_backward_case(R, S, kind)
    got, want, mags = c["got"], c["want"], c["mags"]
    n = c["net"].flat.numel()
    # bounds: every gradient entry written (the buffer held NaN), nothing written outside grads or work
    assert bool(torch.isfinite(c["grads"]).all().item()), "an entry of grads was not written"
    assert guards_intact(c["g_whole"], n), "write outside grads"
    assert guards_intact(c["w_whole"], c["n_work"]), "write outside work"
    worst_n = max((nrel(got[k], want[k]), k) for k in want if want[k].numel() > 1)
    worst_r = worst_ratio(got, want, mags)
    print("teacher backward (%d, %d) %s: worst norm-relative %.3g (%s), worst |got - want| / magnitude %.3g"
          % (R, S, kind, worst_n[0], worst_n[1], worst_r))
    bad = {k: v for k, v in bar_violations(got, want, mags).items() if v}
    assert not bad, bad
    assert worst_n[0] <= NREL_BWD, worst_n


@pytest.mark.parametrize("kind", ["init", "trained"])
@pytest.mark.parametrize("R,S", [(37, 61), (45, 192)])
def test_teacher_backward_bar_sees_one_missing_point(R, S, kind):
    """Self-check of the bar above: the yardstick of the same step WITHOUT one point p (its draw zeroed: points are independent,
    so this removes G_l[p]^T A_l[p] from every layer) must fail it, for p at the first point, either side of the first chunk
    edge, the end of the last full 128-row tile and the last point.  The probe points have live ReLUs: p's contribution to every
    hidden layer's weight gradient is non-zero, and the perturbed yardstick fails the bar on each of those eight tensors.  (The
    draw is random here: behind an opaque surface a real one leaves the last points of a ray without a gradient.)
    Which half of the bar sees it: the per-entry one in the heads and layers 6-7 (one point is 1e-5 .. 1e-2 of the absolute
    backprop there); in layers 0-5 the absolute backprop grows far past the gradient (one point: 1e-12 .. 1e-5 of it), and the
    norm-relative one does (one point moves those tensors by 2e-3 .. 4e-2)."""
    c = run_backward_case(R, S, kind, real_draw=False)
    got, want, mags = c["got"], c["want"], c["mags"]
    assert not any(bar_violations(got, want, mags).values())
    for p in probe_points(R * S):
        draw_p = c["draw"].clone().view(-1, 4)
        draw_p[p] = 0.
        want_p, _ = teacher_backward_from_stash(c["sd"], c["o"], c["d"], c["vd"], c["z"], c["stash"], draw_p.view(R, S, 4),
                                                device="cuda")
        viol = bar_violations(got, want_p, mags)
        for l in range(8):
            k = "pts_linears.%d.weight" % l
            assert (want[k] - want_p[k]).abs().max().item() > 0, (p, k, "probe point without a live path")
            assert viol[k] > 0 or nrel(got[k], want_p[k]) > NREL_BWD, (p, k, "the bar does not see point %d missing" % p)


@pytest.mark.parametrize("R,S", [(0, 61), (37, 0)])
def test_teacher_backward_no_points(R, S):
    """P = 0: grads are zeroed, nothing else is touched."""
    lib = _lib().load()
    net = Net(weights("init"))
    n = net.flat.numel()
    g_whole, grads = guarded(n)
    bufs = [guarded(64)[0] for _ in range(6)]  # o, d, viewdirs, z, stash, draw, each a small sentinel buffer
    w_whole, work = guarded(64)
    rc = lib.r2l_teacher_backward(*[_p(b[GUARD:]) for b in bufs[:4]], _p(net.flat), _p(bufs[4][GUARD:]), _p(bufs[5][GUARD:]),
                                  _p(grads), _p(work), R, S, _s())
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((grads == 0).all().item()) and guards_intact(g_whole, n)
    assert untouched(w_whole) and all(untouched(b) for b in bufs)


# ---- forward with stash -------------------------------------------------------------------------------------------------
C_FWD = 5e-6  # per entry of every stash slot: |got - fp64| <= C_FWD * (|W_l| |x_l| + |b_l|), x_l the fp64 input of that layer


def forward_magnitudes(sd, emb, outs):
    """|W_l| |x_l| + |b_l| of every stashed layer: the size of the sum fp32 rounds, per entry."""
    a = {k: v.abs() for k, v in sd.items()}
    pts, views = emb[:, :63].abs(), emb[:, 63:].abs()
    mags = []
    for i in range(8):
        x = pts if i == 0 else (torch.cat([pts, outs[4]], -1) if i == 5 else outs[i - 1])
        mags.append(x @ a["pts_linears.%d.weight" % i].T + a["pts_linears.%d.bias" % i])
    mags.append(outs[7] @ a["feature_linear.weight"].T + a["feature_linear.bias"])
    mags.append(torch.cat([outs[8].abs(), views], -1) @ a["views_linears.0.weight"].T + a["views_linears.0.bias"])
    return mags


@pytest.mark.parametrize("kind", ["init", "trained"])
@pytest.mark.parametrize("R,S", [(1, 1), (1, 31), (1, 33), (3, 43), (1031, 192)])
def test_forward_with_stash_tails(R, S, kind):
    """r2l_teacher_mlp_train at partial 32-point tiles and workgroups: raw bit-equal to r2l_teacher_mlp_cfg(fp32_mfma), every
    stash slot per entry within 5e-6 of its magnitude of an fp64 forward (measured on one MI355X: 1.1e-6), and nothing written
    past r2l_teacher_stash_floats(P) or past raw."""
    sd = weights(kind)
    net = Net(sd)
    o, d, vd, z = [t.cuda() for t in inputs(R, S, kind, seed=1)]
    raw, st_whole, stash, raw_whole = net.forward_stash(o, d, vd, z)
    P = R * S
    assert guards_intact(st_whole, stash.numel()), "write outside the stash"
    assert guards_intact(raw_whole, P * 4), "write outside raw"
    assert torch.equal(raw, net.forward_infer(o, d, vd, z)), "raw of the forward with stash is not the inference kernel's"
    f64 = dict(dtype=torch.float64, device="cuda")
    pts = (o[:, None, :] + d[:, None, :] * z[:, :, None]).reshape(P, 3)
    emb = torch.cat([O.nerf_embed(pts.to(**f64), 10), O.nerf_embed(vd.to(**f64)[:, None].expand(R, S, 3).reshape(P, 3), 4)], -1)
    sd64 = {k: v.to(**f64) for k, v in sd.items()}
    want = layer_outputs(sd64, emb)
    mags = forward_magnitudes(sd64, emb, want)
    worst = 0.
    for l, got in enumerate(stash_slots(stash, P)):
        err = (got.double() - want[l]).abs()
        ok = err <= C_FWD * mags[l] + 1e-30
        worst = max(worst, (err / mags[l].clamp_min(1e-30)).max().item())
        assert bool(ok.all().item()), (l, int((~ok).sum().item()))  # (an unwritten entry is NaN: it fails here too)
    print("forward with stash (%d, %d) %s: worst |got - fp64| / magnitude %.3g" % (R, S, kind, worst))


# ---- raw2outputs backward -----------------------------------------------------------------------------------------------
# draw per entry, relative to the ray's largest |draw|: C_R2O on every ray but those with colour logits of +-10 (kind 4 of
# r2o_inputs), where fp32's 1 - sigmoid cancels and C_R2O_LOGITS holds.  Measured on one MI355X: 4.2e-6 and 2.1e-4.
C_R2O = 2e-5
C_R2O_LOGITS = 1e-3


def raw2outputs64(raw, z, rays_d, noise, white):
    """rgb_map of O.raw2outputs in fp64, except that S = 1 keeps its one interval of 1e10: the reference expands 1e10 over the
    empty slice of dists there (no sample at all, tests/test_teacher_gpu.py), the kernels give the one sample the last
    interval, as for every other S."""
    if raw.shape[1] > 1:
        return O.raw2outputs(raw, z, rays_d, noise, white)[0]
    dist = torch.full_like(z, 1e10) * torch.norm(rays_d[..., None, :], dim=-1)
    sigma = raw[..., 3] if noise is None else raw[..., 3] + noise
    alpha = 1. - torch.exp(-torch.relu(sigma) * dist)
    rgb_map = torch.sum(alpha[..., None] * torch.sigmoid(raw[..., :3]), -2)
    return rgb_map + (1. - alpha.sum(-1, keepdim=True)) if white else rgb_map


def r2o_inputs(R, S, with_noise):
    """raw [R,S,4], z [R,S], rays_d [R,3] (|d| != 1), noise [R,S] or None, target [R,3]; ray r is of kind (r + S) % 6:
    0 plain, 1 sigma = 0 exactly on every other sample, 2 duplicated depths, 3 alpha = 1 in mid-ray, 4 trained-like magnitudes
    (sigma up to 10^3, colour logits +-10), 5 sigma near zero with noise that flips its sign."""
    g = torch.Generator().manual_seed(R * 1000 + S)
    raw = torch.randn(R, S, 4, generator=g) * 2
    z = torch.sort(torch.rand(R, S, generator=g) * 4 + 2, -1)[0]
    d = torch.randn(R, 3, generator=g) * (0.5 + torch.rand(R, 1, generator=g))
    noise = torch.randn(R, S, generator=g) * 0.5 if with_noise else None
    tgt = torch.rand(R, 3, generator=g)
    for r in range(R):
        kind = (r + S) % 6
        if kind == 1:
            raw[r, ::2, 3] = 0.
            if noise is not None:
                noise[r] = 0.
        elif kind == 2:
            z[r, 1::3] = z[r, 0:S - 1:3][:z[r, 1::3].numel()]
        elif kind == 3:
            raw[r, S // 2, 3] = 1e4
        elif kind == 4:
            raw[r, :, 3] = torch.rand(S, generator=g) * 1100 - 100
            raw[r, :, :3] = torch.rand(S, 3, generator=g) * 20 - 10
        elif kind == 5:
            raw[r, :, 3] = torch.randn(S, generator=g) * 0.1
            if noise is not None:
                noise[r] = -2 * raw[r, :, 3] + torch.randn(S, generator=g) * 0.01
    return raw, z, d, noise, tgt


@pytest.mark.parametrize("R", [1, 3, 4, 5, 45])
@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 128, 255, 256])
def test_raw2outputs_backward_edges(S, R):
    """draw per entry within 2e-5 (1e-3 on rays with colour logits of +-10) of the ray's largest |draw| of fp64 autograd of the oracle's raw2outputs + img2mse, and the
    per-ray squared error within 1e-6 relative (to the value plus the sum of |rgb - target|, its sensitivity to a relative
    error of rgb), over ray counts below and across one workgroup of 4 rays and the degenerate rows of r2o_inputs.
    Measured on one MI355X: draw 4.2e-6 (2.1e-4), sqerr 6.6e-7."""
    lib = _lib().load()
    white, with_noise = (R + S) % 2 == 0, S % 3 != 0
    raw, z, d, noise, tgt = r2o_inputs(R, S, with_noise)
    dev = [None if t is None else t.cuda() for t in (raw, z, d, noise, tgt)]  # (kept alive: the C ABI takes raw pointers)
    dr_whole, draw = guarded(R * S * 4)
    sq_whole, sq = guarded(R)
    _lib().check(lib.r2l_raw2outputs_backward(_p(dev[0]), _p(dev[1]), _p(dev[2]), _p(dev[3]), int(white), _p(dev[4]), _p(draw),
                                              _p(sq), R, S, _s()), "r2l_raw2outputs_backward")
    assert guards_intact(dr_whole, R * S * 4) and guards_intact(sq_whole, R)
    raw64 = raw.double().requires_grad_(True)
    rgb = raw2outputs64(raw64, z.double(), d.double(), None if noise is None else noise.double(), white)
    diff = rgb - tgt.double()
    torch.mean(diff**2).backward()
    want = raw64.grad
    got = draw.view(R, S, 4).cpu().double()
    scale = want.abs().amax(dim=(1, 2), keepdim=True)
    err = (got - want).abs()
    assert bool(torch.isfinite(got).all())
    logits = torch.tensor([(r + S) % 6 == 4 for r in range(R)])
    c = torch.where(logits, C_R2O_LOGITS, C_R2O).double()[:, None, None]
    ratio = (err / scale.clamp_min(1e-300)).amax(dim=(1, 2))
    worst = ratio[~logits].max().item() if (~logits).any() else 0.
    worst_l = ratio[logits].max().item() if logits.any() else 0.
    sq_want = (diff**2).sum(-1).detach()
    sq_err = (sq.cpu().double() - sq_want).abs()
    sq_scale = sq_want + diff.abs().sum(-1).detach()
    print("raw2outputs backward (%d, %d): worst draw / ray max %.3g (logits +-10: %.3g), worst sqerr %.3g" % (
        R, S, worst, worst_l, (sq_err / sq_scale).max().item()))
    assert bool((err <= c * scale + 1e-30).all()), (worst, worst_l)
    assert bool((sq_err <= 1e-6 * sq_scale).all()), (sq_err / sq_scale).max().item()


@pytest.mark.parametrize("R,S,ok", [(3, 0, False), (3, 257, False), (0, 64, True)])
def test_raw2outputs_backward_refusals(R, S, ok):
    """S = 0 and S = 257 are refused with a message and write nothing; R = 0 returns 0 and writes nothing."""
    lib = _lib().load()
    n = max(R, 1) * max(S, 1) * 4
    ins = [guarded(n)[0] for _ in range(3)] + [guarded(16)[0]]  # raw, z, rays_d, target
    dr_whole, draw = guarded(n)
    sq_whole, sq = guarded(max(R, 1))
    rc = lib.r2l_raw2outputs_backward(_p(ins[0][GUARD:]), _p(ins[1][GUARD:]), _p(ins[2][GUARD:]), None, 1, _p(ins[3][GUARD:]),
                                      _p(draw), _p(sq), R, S, _s())
    torch.cuda.synchronize()
    if ok:
        assert rc == 0
    else:
        assert rc != 0
        assert "1 <= S <= 256" in lib.r2l_last_error().decode()
    assert untouched(dr_whole) and untouched(sq_whole)
