"""The fp64 yardstick of the student's FORWARD and its bars (tests/student_util.py: forward_yardstick, forward_bars) checked on
the CPU, without a kernel: the yardstick against the oracle in fp64, the Jacobian behind the encoder's allowance against finite
differences, the fp32 references inside the exact families' bars with C_FWD held in its bracket, the pose kernels' point
arithmetic restated and held against the oracle's — and five mutants that the 1e-4 parity bar lets through, which these bars
must see.  tests/test_student_forward_gpu.py applies the same bars to every kernel family.

The fp32 reference is student_util.forward32 (pinned summation order; the figures do not depend on the CPU).  Measured, candidate
pools of 4096 rays, unit = rgb (1 - rgb) mz:
  the fp32 reference's distance from fp64, in units    n_block 1          3                  8                  43
      worst per entry, perturb 0 / 1                    2.40e-8 / 2.68e-8  1.97e-8 / 2.09e-8  1.96e-8 / 1.72e-8  3.06e-8 / 2.94e-8
      rms, perturb 0 / 1                                4.54e-9 / 4.54e-9  4.20e-9 / 4.15e-9  4.16e-9 / 4.19e-9  6.73e-9 / 6.73e-9
  C_FWD = 1.25e-7: 4 x 3.057e-8 = 1.223e-7.  The worst lies at 0.98 of C_FWD / 4, at 1.96 of C_FWD / 8.
  (absolute: 2.3e-7 .. 5.8e-7; the units of these nets run from 1.6 to ~40, median 13 .. 16.)
  torch's own fp32 on the CPU these figures were taken on: worst 2.0e-8 .. 3.4e-8, rms 4.0e-9 .. 7.5e-9: at most 0.21 of the
  per-entry bar and 0.27 of the rms bar (on a second CPU: rms 2.8e-9 .. 5.2e-9, 0.14 and 0.19 of the bars).  The encoder's
  allowance is at most 4.1e-8 unit (exact) and 3.6e-7 (fp16x2).
Mutants (got = the mutant's fp64 forward rounded to fp32; N = 1000, perturb 1), n_block 3 / 43.  Reference rms 4.2e-9 / 6.6e-9,
fp16x2 operand model rms 7.6e-9 / 1.4e-8 unit; rms bars 1.75e-8 / 2.73e-8 (exact), 4.65e-8 / 7.81e-8 (fp16x2):
  (a) one-product layer: max |rgb| error 1.3e-5 / 2.3e-5; 87 % / 96 % of the rays beyond the exact per-entry bar, the median ray at
      1.9 / 2.9 of it; rms 2.2e-7 / 3.4e-7 = 12.6 / 12.6 x the exact and 4.7 / 4.4 x the fp16x2 rms bar;
  (b) encoding off by 1e-5: max |rgb| error 4.1e-6 / 7.5e-6; rms 8.6e-8 / 1.1e-7 = 4.9 / 4.0 x the exact rms bar; against the fp16x2
      bars it is marginal: rms 1.8 / 1.4 x, per entry 0.94 / 1.14 of the bar at the worst (not required);
  (c) one feature of ray 31 zeroed: that ray at 6.0e3 / 8.2e3 (exact), 2.8e3 / 2.8e3 (fp16x2) of its bar, every other ray <= 0.02;
  (d) one bias entry (0.043 / 0.038) dropped: max |rgb| error 3.4e-4 / 5.3e-4; the LEAST affected ray at 137 / 120 (exact) and
      59 / 44 (fp16x2) of its bar;
  (e) ray 31 from ray 32's encoding: 8.0e4 / 7.2e4 (exact), 3.4e4 / 2.5e4 (fp16x2) of its bar;
  recorded only: a bf16x3 chain whose operands keep two of their three pieces: max |rgb| error 1.5e-6 / 5.9e-6, rms 2.7e-8 /
      7.1e-8 unit = 6.4 / 10.8 x the reference's own, 1.5 / 2.6 x the exact rms bar, per entry 0.70 / 1.74 of the bar.
  (Column 1007, which mutant (c) zeroes, is the last sample's z coordinate itself, the identity feature behind its 20 sines and
  cosines; its top-frequency cosine is column 1006.)
"""
import functools

import numpy as np
import pytest
import torch

from oracle import r2l_oracle as O
from tests import student_util as S


@functools.lru_cache(maxsize=None)
def net(nb):
    return O.make_state_dict(n_block=nb, seed=S.NET_SEED)


@functools.lru_cache(maxsize=None)
def pool(nb, perturb):
    """The whole candidate pool of a depth: (emb64, yardstick)."""
    _, _, _, emb = S.forward_inputs(S.POOL_MIN, perturb, S.case_seed(nb, S.POOL_MIN, perturb))
    return emb, S.forward_yardstick(net(nb), emb, jacobian=True)


@pytest.mark.parametrize("nb,n,perturb", [(1, 33, 1.), (3, 200, 0.), (43, 65, 1.)])
def test_forward64_equals_the_oracle_in_fp64(nb, n, perturb):
    """forward64 = O.r2l_forward on fp64 tensors to 1e-14; chunking changes nothing; the unit is what its definition says."""
    sd64 = S.f64(net(nb))
    _, _, _, emb = S.forward_inputs(n, perturb, S.case_seed(nb, n, perturb))
    f = S.forward64(sd64, emb)
    assert (f["rgb"] - O.r2l_forward(sd64, emb)).abs().max().item() < 1e-14
    Y, Yc = S.forward_yardstick(net(nb), emb, model=True), S.forward_yardstick(net(nb), emb, model=True, chunk=(n + 1) // 2)
    for k in Y:  # (e_ref: its fp32 steps round fp64 sums, whose last bit may follow the batch's shape)
        assert Y[k].shape == (n, 3) and (k == "e_ref" or (Y[k] - Yc[k]).abs().max().item() <= 1e-12 * Y["unit"].max().item()), k
    mz = f["ym"] @ sd64["tail.0.weight"].abs().T + sd64["tail.0.bias"].abs()
    z = f["y"] @ sd64["tail.0.weight"].T + sd64["tail.0.bias"]
    assert bool((mz >= z.abs()).all()) and torch.allclose(Y["unit"], f["rgb"] * (1 - f["rgb"]) * mz, rtol=1e-12, atol=0)
    assert bool((Y["jac1"] >= Y["jac2"]).all()) and bool((Y["jac2"] > 0).all())


@pytest.mark.parametrize("nb", [3, 43])
def test_jacobian_equals_finite_differences(nb):
    """dz_c / d emb[p][j] from autograd against a central difference of the fp64 forward, a few entries of every kind of column
    (low and top frequency, sine and cosine, identity; first and last sample): to 1e-6 of the row's largest entry."""
    n = 40
    sd64 = S.f64(net(nb))
    _, _, _, emb = S.forward_inputs(n, 1., S.case_seed(nb, n, 1.))
    rows = S.tail_jacobian_rows(sd64, emb)
    z = lambda e: torch.logit(S.forward64(sd64, e)["rgb"])
    h = 1e-6
    for p, j in ((0, 0), (3, 9), (17, 19), (31, 20), (31, S.MUTANT_COL), (39, 1006), (20, 500)):
        ep, em = emb.clone(), emb.clone()
        ep[p, j] += h
        em[p, j] -= h
        fd = (z(ep) - z(em))[p] / (2 * h)
        for c in range(3):
            assert abs(fd[c].item() - rows[c][p, j].item()) <= 1e-6 * rows[c][p].abs().max().item(), (p, j, c)
            assert (z(ep) - z(em))[torch.arange(n) != p].abs().max().item() == 0.  # the rays do not interact


def test_forward32_is_the_oracle_in_fp32():
    """The pinned fp32 reference against torch's own fp32 forward: the same function to fp32 rounding (a few 1e-7 absolute), and
    with one product per rounding step and in one step the accumulator's definition holds to the bit on small integers."""
    sd = net(3)
    _, _, _, emb = S.forward_inputs(200, 1., 7)
    assert (S.forward32(S.f64(sd), emb.float()) - O.r2l_forward(sd, emb.float())).abs().max().item() < 2e-6
    g = torch.Generator().manual_seed(0)
    x, w, b = [torch.randint(-8, 9, sh, generator=g).float() for sh in ((5, 16), (7, 16), (7,))]
    for kstep in (1, 2, 16):
        assert torch.equal(S.linear32(x, w.double(), b.double(), kstep), torch.nn.functional.linear(x, w, b))
    z = torch.linspace(-12, 12, 1001)
    assert (S.sigmoid32(z).double() - torch.sigmoid(z.double())).abs().max().item() <= 1.5 * 2.0 ** -24


@pytest.mark.parametrize("perturb", [0., 1.])
@pytest.mark.parametrize("nb", S.FWD_DEPTHS)
def test_fp32_references_inside_the_exact_bars(nb, perturb):
    """Whole pool, every depth: the pinned fp32 reference's worst entry stays under C_FWD / 4; and torch's own fp32 forward
    (O.r2l_forward on the fp32-rounded encoding, summed however this CPU's sgemm sums) passes both bars of the exact families."""
    emb, Y = pool(nb, perturb)
    r = S.forward_check(O.r2l_forward(net(nb), emb.float()), Y, S.EMB_EXACT)
    worst = (Y["e_ref"] / Y["unit"]).max().item()
    print("n_block %d perturb %g: fp32 reference worst %.4g rms %.4g unit (abs %.3g); torch's fp32 at %.3g of the per-entry bar, rms "
          "%.4g = %.3g of its bar; encoder's allowance at most %.3g (exact) / %.3g (fp16x2) unit"
          % (nb, perturb, worst, S.rms(Y["e_ref"] / Y["unit"]), Y["e_ref"].max().item(), r["worst"], r["rms"], r["rms"] / r["rms_bar"],
             (S.EMB_EXACT * Y["jac1"] / Y["unit"]).max().item(), (S.EMB_ERR * Y["jac1"] / Y["unit"]).max().item()))
    assert not bool(r["bad"].any()) and r["rms"] <= r["rms_bar"], r
    assert worst <= S.C_FWD / 4, worst


def test_c_fwd_bracket():
    """C_FWD is 4 times the fp32 reference's worst distance over the pools of every depth and both jitter modes: that worst lies
    between C_FWD / 8 and C_FWD / 4, so the constant can drift neither loose nor under the reference."""
    worst = max((pool(nb, perturb)[1]["e_ref"] / pool(nb, perturb)[1]["unit"]).max().item() for nb in S.FWD_DEPTHS for perturb in (0., 1.))
    print("fp32 reference, worst over every pool: %.4g unit; C_FWD %.3g" % (worst, S.C_FWD))
    assert S.C_FWD / 8 <= worst <= S.C_FWD / 4, worst


def bf16_pieces(x, n):
    return sum(S.pieces(x, torch.bfloat16, n))



@pytest.mark.parametrize("nb", [3, 43])
def test_bars_see_the_mutants(nb):
    """Each mutant's fp64 forward, rounded to fp32, as `got`:
    (a) body.(nb//2).body.0.weight rounded to fp16 (a one-product layer): the exact per-entry bar fails on at least half of the rays
        and the rms exceeds the exact AND the fp16x2 rms bar;
    (b) the encoding off by 1e-5 with random signs (a fast-math sine): the rms exceeds the exact rms bar (the fp16x2 bar is recorded);
    (c) ray 31's last feature zeroed: the per-entry bars fail at that ray by ~1e4 and at no other;
    (d) one entry of the last block's second bias dropped: every ray fails;
    (e) ray 31 computed from ray 32's encoding: that ray fails.
    Recorded, not required: a bf16x3 chain without its third piece (both operands of every head and body product cut to two bf16
    pieces), as a multiple of the fp32 reference's own rms."""
    n, perturb = 1000, 1.
    sd = net(nb)
    sd64 = S.f64(sd)
    _, _, _, emb = S.forward_inputs(n, perturb, S.case_seed(nb, n, perturb))
    Y = S.forward_yardstick(sd, emb, model=True)
    fwd = lambda s, e: S.forward64(s, e)["rgb"].float()
    exact = lambda got: S.forward_check(got, Y, S.EMB_EXACT)
    half = lambda got: S.forward_check(got, Y, S.EMB_ERR, True)
    for bars in (exact, half):  # the unmutated forward passes
        r = bars(fwd(sd64, emb))
        assert not bool(r["bad"].any()) and r["rms"] <= r["rms_bar"]
    tag = "n_block %d: " % nb
    ref_rms = S.rms(Y["e_ref"] / Y["unit"])
    print(tag + "fp32 reference rms %.3g, fp16x2 model rms %.3g unit (worst entry %.3g); rms bars %.3g (exact), %.3g (fp16x2)"
          % (ref_rms, S.rms(Y["e_model"] / Y["unit"]), (Y["e_model"] / Y["unit"]).max().item(), exact(Y["rgb"])["rms_bar"],
             half(Y["rgb"])["rms_bar"]))

    k = "body.%d.body.0.weight" % (nb // 2)  # (a)
    got = fwd({**sd64, k: sd64[k].half().double()}, emb)
    a, ah = exact(got), half(got)
    print(tag + "(a) max |rgb| error %.3g; exact per-entry bar fails on %.1f %% of the rays, median ray at %.2f of it; rms %.3g = %.1f x "
          "the exact, %.1f x the fp16x2 rms bar" % ((got.double() - Y["rgb"]).abs().max().item(), 100 * a["bad"].double().mean().item(),
                                                   a["ratio"].median().item(), a["rms"], a["rms"] / a["rms_bar"], ah["rms"] / ah["rms_bar"]))
    assert a["bad"].double().mean().item() >= 0.5 and a["rms"] > a["rms_bar"] and ah["rms"] > ah["rms_bar"]

    gen = torch.Generator().manual_seed(nb)  # (b)
    got = fwd(sd64, emb + 1e-5 * (torch.randint(0, 2, emb.shape, generator=gen).double() * 2 - 1))
    b, bh = exact(got), half(got)
    print(tag + "(b) max |rgb| error %.3g; rms %.3g = %.2f x the exact rms bar, %.2f x the fp16x2 one (not required); per entry %.2f / "
          "%.2f of the bars at the worst" % ((got.double() - Y["rgb"]).abs().max().item(), b["rms"], b["rms"] / b["rms_bar"],
                                             bh["rms"] / bh["rms_bar"], b["worst"], bh["worst"]))
    assert b["rms"] > b["rms_bar"]

    p = S.MUTANT_RAY  # (c), and the yardstick of (c) against the unmutated forward, as the GPU self-check takes it
    e = emb.clone()
    e[p, S.MUTANT_COL] = 0.
    got = fwd(sd64, e)
    others = torch.arange(n) != p
    for name, r in (("exact", exact(got)), ("fp16x2", half(got))):
        print(tag + "(c) %s: ray %d at %.3g of its bar, every other ray at most %.3g" % (name, p, r["ratio"][p].item(), r["ratio"][others].max().item()))
        assert bool(r["bad"][p]) and not bool(r["bad"][others].any())
    Yc = S.mutant_c(Y, sd, emb[p:p + 1], model=True)
    for emb_err, fp16 in ((S.EMB_EXACT, False), (S.EMB_ERR, True)):
        r = S.forward_check(fwd(sd64, emb), Yc, emb_err, fp16)
        assert bool(r["bad"][p]) and not bool(r["bad"][others].any()) and r["ratio"][p].item() > 100.

    k = "body.%d.body.2.bias" % (nb - 1)  # (d)
    bias = sd64[k].clone()
    bias[0] = 0.
    got = fwd({**sd64, k: bias}, emb)
    d, dh = exact(got), half(got)
    print(tag + "(d) bias entry %.3g dropped: max |rgb| error %.3g; the least affected ray at %.3g (exact) / %.3g (fp16x2) of its bar"
          % (sd64[k][0].item(), (got.double() - Y["rgb"]).abs().max().item(), d["ratio"].min().item(), dh["ratio"].min().item()))
    assert bool(d["bad"].all()) and bool(dh["bad"].all())

    got = fwd(sd64, emb)  # (e)
    got[p] = got[p + 1]
    ee, eh = exact(got), half(got)
    print(tag + "(e) ray %d at %.3g (exact) / %.3g (fp16x2) of its bar" % (p, ee["ratio"][p].item(), eh["ratio"][p].item()))
    assert bool(ee["bad"][p]) and bool(eh["bad"][p]) and int(ee["bad"].sum()) == 1 and int(eh["bad"].sum()) == 1

    cut = {kk: (bf16_pieces(v, 2) if not kk.startswith("tail.") else v) for kk, v in sd64.items()}  # recorded only
    lin = lambda x, name: bf16_pieces(x, 2) @ cut[name + ".weight"].T + cut[name + ".bias"]
    x0 = torch.relu(lin(emb, "head.0"))
    x = x0
    for blk in range(nb):
        x = lin(torch.relu(lin(x, "body.%d.body.0" % blk)), "body.%d.body.2" % blk) + x
    got = torch.sigmoid((x + x0) @ sd64["tail.0.weight"].T + sd64["tail.0.bias"]).float()
    c = exact(got)
    print(tag + "bf16 chain without its third piece: max |rgb| error %.3g, rms %.3g unit = %.2f x the fp32 reference's own; %.2f of the "
          "exact rms bar, per entry %.2f of the bar (not required to be seen)"
          % ((got.double() - Y["rgb"]).abs().max().item(), c["rms"], c["rms"] / ref_rms, c["rms"] / c["rms_bar"], c["worst"]))


POSE_FRAMES = [(7, 9, 10.), (33, 31, 40.), (37, 41, 50.)]


@pytest.mark.parametrize("H,W,focal", POSE_FRAMES)
def test_pose_points_restatement_against_the_oracle(H, W, focal):
    """student_util.pose_points32 — the pose kernels' point arithmetic restated in numpy fp32 — against O.sample_test: within 1 ulp
    per coordinate.  (Here they agree to the bit: torch sums the three products of a direction in the kernels' order.  The GPU
    test feeds the restatement to the yardstick either way.)"""
    z = O.z_vals(S.N_SAMPLE, S.NEAR, S.FAR)
    worst, differing = 0., 0
    for k in range(3):
        c2w = torch.from_numpy(O.pose_spherical(30. * k, -20. - 3 * k, 4.)[:3, :4])
        want = O.sample_test(O.pixel_dirs(H, W, focal), z, c2w).numpy()
        got = S.pose_points32(c2w.numpy(), H, W, focal, z.numpy())
        assert got.shape == want.shape == (H * W, 48) and got.dtype == np.float32
        ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
        worst, differing = max(worst, float(ulps.max())), differing + int((got != want).sum())
    print("%d x %d: %d coordinates differ from O.sample_test, by at most %.3g ulp" % (H, W, differing, worst))
    assert worst <= 1.0
