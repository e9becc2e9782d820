"""The fp64 yardstick of the teacher's inference forward and its bars (tests/teacher_util.py: forward_yardstick, forward_bars)
checked on the CPU, without a kernel: the points' arithmetic against the restatement the backward's yardstick uses, the yardstick
against the oracle in fp64, the Jacobian against finite differences, the pinned fp32 reference held inside C_T / 4 on every case
of the table, the fp16x2 operand model's own distance and its scale invariance, the condition on the inputs — and the mutants
(a) .. (f), which the older 2e-5 bar lets through and these bars must see.  tests/test_teacher_forward_gpu.py applies the same
bars to the three kernel families.

Measured (the trained-like net: 400 Adam steps on four threads, the same net wherever the test runs); unit = |W_head| |x| + |b_head|,
median 0.31 on init weights and 15 .. 27 on trained-like ones:
  the pinned fp32 reference's distance from fp64: worst 8.99e-7 unit on init weights ((5, 192); rms 1.2e-7), 1.053e-6 on trained-like
      ones ((4099, 4); rms 8.5e-8), 5.2e-7 on the scaled net; C_T = 4.3e-6.  torch's own fp32: 0.03 of the per-entry bar on init
      weights, 0.20 on trained-like ones.  The encoder's allowance is at most 1.8e-7 unit (init) and 4.9e-6 (trained-like).
  the fp16x2 operand model: worst 3.5e-7 / 2.2e-6 unit, rms 7.4e-8 / 8.6e-8 (init / trained-like): at most 0.31 of the exact
      per-entry bar.  On the scaled net 1.27e-4 worst, 1.65e-5 rms at s = 32 (layer 1's weights of 6e-7 are fp16 subnormals); the
      width of its family 6.1e-7 / 2.0e-6 / 1.5e-5 unit at s = 8 / 32 / 256.
Mutants, as a multiple of the per-entry bar (exact group; the fp16x2 group within 10 % of it), trained-like / init weights:
  (a) fused points: worst 7.4 / 0.67 at (37, 64) and (4099, 4); 2.5 .. 2.7 % of the differing points beyond the bar / none.  On init
      weights it is NOT seen and not required (DAMPED below): the issue's "8 bars" was taken against torch's blocked fp32 sums;
  (b) W_hi x_mid lost in layer 0 / layer 3 / the views layer: median point at 6.8 / 4.3 / 5.7, 90 .. 99 % of the points beyond
      the fp16x2 bar; on init weights 0.10 / 0.11 (not required: DAMPED) / 6.4 (99.7 %);
  (c) the top xyz column of layer 5 zeroed: median 52 / 359; the last direction column of the views layer: 38 / 9.5e3;
  (d) the tile's first ray's direction: every affected point, median 4e3 / 4.8e4; no other point;
  (e) the last point left at the sentinel: that point and no other; swapped with its neighbour: both, 4e2 .. 1.8e5;
  (f) scaled, one bias undivided by s = 32 / 256: every point, median 185 .. 2.6e5.
"""
import functools

import pytest
import torch

from oracle import r2l_oracle as O
from tests import teacher_util as T

SCALED_CASE, SCALED_S = (4099, 4), 32.0  # (the device settles at 2^5 on this net, after one launch at the blind jump's 2^8)
SENTINEL = 0x7FA5C3E1  # the NaN pattern tests/test_teacher_gpu.py fills raw with


@functools.lru_cache(maxsize=None)
def case(kind, R, S):
    """Inputs, points, encoding and yardstick of one case, once per process."""
    sd = T.forward_weights(kind, "cpu")
    o, d, vd, z = T.forward_inputs(R, S, kind)
    pts = T.points32(o, d, z)
    emb = T.encoding64(pts, vd, S)
    Y = T.forward_yardstick(sd, emb, model_scale=SCALED_S if kind == "scaled" else 1.0, spread=(kind == "scaled"))
    return dict(sd=sd, sd64={k: v.double() for k, v in sd.items()}, o=o, d=d, vd=vd, z=z, pts=pts, emb=emb, Y=Y)


def table():
    return [(kind, R, S) for kind in ("init", "trained") for R, S in T.T_CASES] + [("scaled",) + SCALED_CASE]


@pytest.mark.parametrize("kind", ["init", "trained"])
@pytest.mark.parametrize("R,S", [(3, 43), (4099, 4)])
def test_points_equal_the_backward_yardsticks_bit_for_bit(R, S, kind):
    """points32 against the expression of teacher_backward_from_stash (one torch fp32 expression: product, then sum) and against
    numpy fp32, to the bit; the fused form differs from it on a sizeable share of the points, by the
    product's rounding."""
    o, d, vd, z = T.forward_inputs(R, S, kind)
    pts = T.points32(o, d, z)
    assert pts.dtype == torch.float32 and pts.shape == (R * S, 3)
    assert torch.equal(pts, (o[:, None, :] + d[:, None, :] * z[:, :, None]).reshape(R * S, 3))
    on, dn, zn = o.numpy(), d.numpy(), z.numpy()
    assert (pts.numpy() == (on[:, None, :] + dn[:, None, :] * zn[:, :, None]).reshape(-1, 3)).all()
    fma = T.points32(o, d, z, fma=True)
    share = (fma != pts).any(1).double().mean().item()
    print("(%d, %d) %s: the fused points differ at %.1f %% of the points" % (R, S, kind, 100 * share))
    assert 0.05 < share < 0.95
    size = (o.double().abs()[:, None, :] + (d.double()[:, None, :] * z.double()[:, :, None]).abs()).reshape(-1, 3)
    assert ((fma.double() - pts.double()).abs() <= 2.0 ** -23 * size).all()  # (the product's rounding, seen at the sum's size)


@pytest.mark.parametrize("kind,R,S", table())
def test_inputs_meet_the_encoders_condition(kind, R, S):
    """max |p| * 2^9 <= 4096 in every case (r2l_sincos's 1.5 ulp is measured there); unit directions; and, where a tile can hold
    two rays, two rays with one origin and different view directions inside one 32-point tile."""
    o, d, vd, z = T.forward_inputs(R, S, kind)
    T.check_input_condition(T.points32(o, d, z), vd)
    assert (vd.norm(dim=-1) - 1).abs().max().item() < 1e-6 and z.min().item() >= 2 and z.max().item() < 6
    if R > 1 and S < T.T_TILE:
        assert torch.equal(o[0], o[1]) and not torch.equal(vd[0], vd[1])


@pytest.mark.parametrize("kind", ["init", "trained"])
def test_yardstick_equals_the_oracle_in_fp64(kind):
    """forward64 = O.nerf_forward / O.run_network on fp64 tensors to 1e-12 of the unit; the unit is what its definition says and
    bounds |raw|; chunking changes nothing."""
    c = case(kind, 3, 43)
    raw, unit = T.forward64(c["sd64"], c["emb"])
    want = O.nerf_forward(c["sd64"], c["emb"])
    assert (raw - want).abs().max().item() <= 1e-12 * unit.max().item()
    net = O.run_network(c["sd64"], c["pts"].double().view(3, 43, 3), c["vd"].double()).reshape(-1, 4)
    assert (raw - net).abs().max().item() <= 1e-12 * unit.max().item()
    assert bool((unit >= raw.abs()).all()) and bool((unit > 0).all())
    Y, Yc = c["Y"], T.forward_yardstick(c["sd"], c["emb"], model_scale=1.0, chunk=50)
    for k in Y:  # (e_ref: its fp32 steps round fp64 sums, whose last bit may follow the batch's shape)
        assert Y[k].shape == (129, 4) and (k == "e_ref" or (Y[k] - Yc[k]).abs().max().item() <= 1e-12 * Y["unit"].max().item()), k
    assert bool((Y["jac1"] >= Y["jac2"]).all()) and bool((Y["jac2"] > 0).all())


def test_jacobian_equals_finite_differences():
    """d raw[p,c] / d emb[p,j] from autograd against a central difference of the fp64 forward, on columns of every kind."""
    c = case("init", 3, 43)
    rows = T.jacobian_rows(c["sd64"], c["emb"])
    f = lambda e: T.forward64(c["sd64"], e)[0]
    h = 1e-6
    for p, j in ((0, 0), (5, 3), (31, T.T_XYZ_TOP_COL), (32, 40), (77, 63), (128, 63 + T.T_DIR_LAST_COL), (128, 2)):
        ep, em = c["emb"].clone(), c["emb"].clone()
        ep[p, j] += h
        em[p, j] -= h
        diff = f(ep) - f(em)
        assert diff[torch.arange(129) != p].abs().max().item() == 0.  # the points do not interact
        for ch in range(4):
            assert abs(diff[p, ch].item() / (2 * h) - rows[ch][p, j].item()) <= 1e-6 * rows[ch][p].abs().max().item(), (p, j, ch)
    assert rows[3][:, 63:].abs().max().item() == 0.  # sigma does not see the view direction


def test_forward32_is_the_oracle_in_fp32():
    c = case("init", 3, 43)
    got = T.forward32(c["sd64"], c["emb"].float())
    assert got.dtype == torch.float32
    assert (got - O.nerf_forward(c["sd"], c["emb"].float())).abs().max().item() < 2e-6


@pytest.mark.parametrize("kind,R,S", table())
def test_fp32_reference_inside_a_quarter_of_c_t(kind, R, S):
    """The pinned fp32 reference's worst entry stays under C_T / 4 in every case; torch's own fp32 forward on the fp32-rounded
    encoding (summed however this CPU's sgemm sums) passes both bars of the exact families as a subject."""
    c = case(kind, R, S)
    Y = c["Y"]
    r = Y["e_ref"] / Y["unit"]
    m = Y["e_model"] / Y["unit"]
    t = T.forward_check(O.nerf_forward(c["sd"], c["emb"].float()), Y)
    print("REF %s (%d, %d): fp32 reference worst %.4g rms %.4g unit (abs %.3g); fp16x2 model%s worst %.4g rms %.4g unit, %.3g of the exact "
          "per-entry bar; torch's fp32 at %.3g of the per-entry bar, rms %.3g of its bar; unit median %.3g; encoder's allowance <= %.3g unit"
          % (kind, R, S, r.max().item(), T.rms(r), Y["e_ref"].max().item(), " (s = %g)" % SCALED_S if kind == "scaled" else "",
             m.max().item(), T.rms(m), (Y["e_model"] / T.forward_bars(Y)[0]).max().item(), t["worst"], t["rms"] / t["rms_bar"],
             Y["unit"].median().item(), (T.EMB_EXACT * Y["jac1"] / Y["unit"]).max().item()))
    assert r.max().item() <= T.C_T / 4, r.max().item()
    assert not bool(t["bad"].any()) and (R * S < T.T_RMS_MIN_POINTS or t["rms"] <= t["rms_bar"])


def test_c_t_bracket():
    """C_T is 4 times the reference's worst distance over the whole table: that worst lies between C_T / 8 and C_T / 4."""
    worst = max((case(*k)["Y"]["e_ref"] / case(*k)["Y"]["unit"]).max().item() for k in table())
    print("fp32 reference, worst over the table: %.4g unit; C_T %.3g" % (worst, T.C_T))
    assert T.C_T / 8 <= worst <= T.C_T / 4, worst


def test_operand_model_distance():
    """The fp16x2 operand model against fp64.  One product carries at most 2^-21 of its size (the dropped mid * mid term and the
    two mid roundings); the roundings of different products and layers are independent, so over a case the rms stays below one
    product's 2^-21 unit, and the worst entry below the linear sum over the eleven layers, 11 * 2^-21 unit — and it is not fp64
    either (rms above 2^-27).  On the scaled net, whose layer 0 holds 1e5, the model needs its scale: at s = 1 fp16 overflows."""
    for kind in ("init", "trained"):
        for R, S in T.T_CASES:
            Y = case(kind, R, S)["Y"]
            m = Y["e_model"] / Y["unit"]
            assert 2.0 ** -27 < T.rms(m) < 2.0 ** -21 and m.max().item() < 11 * 2.0 ** -21, (kind, R, S, T.rms(m), m.max().item())
    c = case("scaled", *SCALED_CASE)
    h0 = torch.relu(c["emb"][:, :63] @ c["sd64"]["pts_linears.0.weight"].T + c["sd64"]["pts_linears.0.bias"])
    assert h0.max().item() > 65504  # the case leaves the guarded range (R2L_F2_RANGE = 32768) and fp16 altogether
    assert not bool(torch.isfinite(T.forward16x2(c["sd64"], c["emb"], s=1.0)).all())
    assert bool(torch.isfinite(T.forward16x2(c["sd64"], c["emb"], s=SCALED_S)).all())


# Init-distribution weights DAMP what happens in front of the last layers.  A layer has 256 weights of variance 1 / (3 * 256) and
# about half of its units live: a perturbation of its input leaves it sqrt(1 / 6) = 0.41 times as large, per layer.  The W_hi x_mid
# term of layer 0 or 3 is 2^-12 of that layer's products to begin with and reaches raw at 0.07 .. 0.11 of the fp16x2 bar; the fused
# points, half an ulp of d * z, at 0.53 .. 0.66 of either bar.  Both lie UNDER the distance of the pinned fp32 reference from fp64
# (worst 9e-7 unit, which C_T is four times), and no bar derived from that reference can see them: on these weights the two are
# printed and not required.  On the trained-like weights, whose layers do not damp, they are required like every other mutant;
# and on both kinds everything that acts from layer 5's skip block onwards is.
DAMPED = {"init": ("pts_linears.0", "pts_linears.3")}


def _report(tag, r, affected):
    a = torch.as_tensor(affected)
    share = r["bad"][a].double().mean().item() if a.any() else 0.
    print("MUTANT %s: %d of %d affected points beyond the bar (%.1f %%), worst ratio %.3g, median over the affected %.3g; unaffected "
          "points at most %.3g" % (tag, int(r["bad"][a].sum()), int(a.sum()), 100 * share, r["ratio"][a].max().item() if a.any() else 0.,
                                   r["ratio"][a].median().item() if a.any() else 0., r["ratio"][~a].max().item() if (~a).any() else 0.))
    return share


@pytest.mark.parametrize("kind", ["init", "trained"])
@pytest.mark.parametrize("R,S", [(37, 64), (4099, 4)])
def test_bars_see_fused_points(R, S, kind):
    """(a): the fp64 forward of the points formed with ONE rounding, rounded to fp32, against the bars of both groups: beyond the
    per-entry bar on some of the points whose coordinates differ, within it on every other point.  (The effect of one point is
    0.5 ulp of d * z, times up to 2^9 in the encoding's argument, through that point's Jacobian: a heavy-tailed quantity — which
    is why this mutant is looked for in cases of some thousand points.)
    Required on the trained-like weights.  On init-distribution weights it is printed and NOT required: see DAMPED below."""
    c = case(kind, R, S)
    fma = T.points32(c["o"], c["d"], c["z"], fma=True)
    differ = (fma != c["pts"]).any(1)
    got = T.forward64(c["sd64"], T.encoding64(fma, c["vd"], S))[0].float()
    seen = {}
    for name, fp16 in (("exact", False), ("fp16x2", True)):
        r = T.forward_check(got, c["Y"], fp16)
        _report("%s (%d, %d) (a) fused points, %s" % (kind, R, S, name), r, differ)
        assert not bool(r["bad"][~differ].any())
        seen[name] = bool(r["bad"][differ].any())
    assert kind in DAMPED or (seen["exact"] and seen["fp16x2"]), seen


@pytest.mark.parametrize("kind", ["init", "trained"])
@pytest.mark.parametrize("R,S", T.T_SELF_CHECK_CASES + [(3, 43)])
def test_bars_see_the_mutants(R, S, kind):
    """got = the mutant's fp64 forward rounded to fp32 (for (b): the mutated operand model), held to the bars of both groups.
    Every figure is printed before the first assertion."""
    c = case(kind, R, S)
    sd, sd64, Y, emb, P = c["sd"], c["sd64"], c["Y"], c["emb"], R * S
    tag = "%s (%d, %d) " % (kind, R, S)
    fwd = lambda s, e: T.forward64(s, e)[0].float()
    groups = (("exact", False), ("fp16x2", True))
    for name, fp16 in groups:  # the unmutated forward and the unmutated model pass
        assert not bool(T.forward_check(fwd(sd64, emb), Y, fp16)["bad"].any())
    assert not bool(T.forward_check(T.forward16x2(sd64, emb).float(), Y, True)["bad"].any())
    every = torch.ones(P, dtype=torch.bool)
    missed = []

    for layer in ("pts_linears.0", "pts_linears.3", "views_linears.0"):  # (b), fp16x2 only
        r = T.forward_check(T.forward16x2(sd64, emb, drop_mid=layer).float(), Y, True)
        if _report(tag + "(b) W_hi x_mid lost in %s, fp16x2" % layer, r, every) <= 0.5 and layer not in DAMPED.get(kind, ()):
            missed.append(("b", layer))

    for wname, col in (("pts_linears.5.weight", T.T_XYZ_TOP_COL), ("views_linears.0.weight", 256 + T.T_DIR_LAST_COL)):  # (c)
        got = fwd({k: v.double() for k, v in T.zero_column(sd, wname, col).items()}, emb)
        for name, fp16 in groups:
            r = T.forward_check(got, Y, fp16)
            if _report(tag + "(c) column %d of %s zeroed, %s" % (col, wname, name), r, every) <= 0.5:
                missed.append(("c", wname, name))

    if S < T.T_TILE or S % T.T_TILE:  # (d): a tile holds points of two rays
        vd_t = T.tile_first_ray_directions(c["vd"], R, S)
        e = emb.clone()
        e[:, 63:] = O.nerf_embed(vd_t.double(), 4)
        moved = (vd_t != c["vd"][torch.arange(P) // S]).any(1)
        assert moved.any()
        got = fwd(sd64, e)
        for name, fp16 in groups:
            r = T.forward_check(got, Y, fp16)
            if _report(tag + "(d) the tile's first ray's direction, %s" % name, r, moved) <= 0.5 or bool(r["bad"][~moved].any()):
                missed.append(("d", name))

    pair = (torch.arange(P) == P - 1) | (torch.arange(P) == P - 2)  # (e)
    got = fwd(sd64, emb)
    got[P - 1] = torch.tensor([SENTINEL] * 4, dtype=torch.int32).view(torch.float32)
    for name, fp16 in groups:
        r = T.forward_check(got, Y, fp16)
        if not (bool(r["bad"][P - 1]) and int(r["bad"].sum()) == 1):
            missed.append(("e, sentinel", name))
    got = fwd(sd64, emb)
    got[[P - 1, P - 2]] = got[[P - 2, P - 1]]
    for name, fp16 in groups:
        r = T.forward_check(got, Y, fp16)
        _report(tag + "(e) the last two points swapped, %s" % name, r, pair)
        if not (bool(r["bad"][P - 1]) and bool(r["bad"][P - 2]) and int(r["bad"].sum()) == 2):
            missed.append(("e, swap", name))
    assert not missed, missed


def test_scaled_bars_see_an_undivided_bias():
    """(f), the scaled stream at s = 2^5 and 2^8: the operand model with one layer's bias left undivided by s fails the fp16x2 bars
    (with the family's width in them) at every point; the model at the scale itself, and its second realization, pass them."""
    c = case("scaled", *SCALED_CASE)
    sd64, emb = c["sd64"], c["emb"]
    every = torch.ones(emb.shape[0], dtype=torch.bool)
    for s in (SCALED_S, 256.0):
        Y = dict(c["Y"], e_model=(T.forward16x2(sd64, emb, s=s) - c["Y"]["raw"]).abs(), spread=T.forward_spread(sd64, emb, c["Y"]["unit"], s))
        for jitter in (0., T.T_JITTER):
            assert not bool(T.forward_check(T.forward16x2(sd64, emb, s=s, jitter=jitter).float(), Y, True)["bad"].any())
        for layer in ("pts_linears.2", "feature_linear", "views_linears.0"):
            r = T.forward_check(T.forward16x2(sd64, emb, s=s, undivided_bias=layer).float(), Y, True)
            share = _report("scaled (f) bias of %s undivided by s = %g, fp16x2" % (layer, s), r, every)
            assert share > 0.99


def test_operand_models_family_widens_with_the_scale():
    """forward_spread, the term the scaled stream's per-entry bar takes: on the scaled net it grows with s (mid pieces of x / s
    under fp16's normal range are carried to s 2^-25 in the net's units) and stays below the model's own distance; the second
    realization lies as far from fp64 as the first (same rms to 20 %): neither is THE model."""
    c = case("scaled", *SCALED_CASE)
    sd64, emb, unit, raw = c["sd64"], c["emb"], c["Y"]["unit"], c["Y"]["raw"]
    w = {s: T.forward_spread(sd64, emb, unit, s).item() for s in (8.0, 32.0, 256.0)}
    print("scaled net: width of the operand model's family %s unit" % ", ".join("%.3g at s = %g" % (v, s) for s, v in w.items()))
    assert w[8.0] < w[32.0] < w[256.0] and w[256.0] > 4 * w[32.0]
    for s in (32.0, 256.0):
        a, b = T.forward16x2(sd64, emb, s=s), T.forward16x2(sd64, emb, s=s, jitter=T.T_JITTER)
        ea, eb = T.rms((a - raw) / unit), T.rms((b - raw) / unit)
        assert w[s] < ((a - raw).abs() / unit).max().item() and abs(ea - eb) < 0.2 * ea, (s, w[s], ea, eb)
