"""What tests/test_render_stages_gpu.py rests on, checked without a GPU (tests/render_util.py): the fp64 yardstick of compositing
is the oracle's op sequence, the input tables meet their conditions, the reference's own fp32 arithmetic (torch on the CPU) and the
torch-op branches of r2l_amd/render.py pass every bar and judgement, and the self-check's probes have live rays."""
import pytest
import torch

from oracle import r2l_oracle as O
from tests import render_util as U


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


# ---- compositing ------------------------------------------------------------------------------------------------------------
def test_r2o_yardstick_is_the_oracle_in_fp64():
    """raw2outputs64 is oracle raw2outputs on fp64 copies of the inputs, bit for bit, for S >= 2; for S = 1 its rgb is the contract
    the backward's test pins (tests/test_teacher_backward_gpu.py::raw2outputs64)."""
    from tests.test_teacher_backward_gpu import raw2outputs64 as backward_rgb64
    for S in U.R2O_S:
        raw, z, d, noise, white = U.r2o_inputs(45, S)
        want = U.r2o_want(45, S)
        n64 = None if noise is None else noise.double()
        if S >= 2:
            ref = O.raw2outputs(raw.double(), z.double(), d.double(), n64, white)
            for a, b in zip(want, ref):
                assert b.dtype == torch.float64 and torch.equal(bits(a), bits(b)), S
        assert torch.equal(bits(want[0]), bits(backward_rgb64(raw.double(), z.double(), d.double(), n64, white))), S


def test_r2o_table_conditions():
    """Every ray has acc64 == 0 exactly or acc64 >= 1e-3; the two empty kinds are exactly empty; alpha is exactly 1 where the table
    says so, in fp64 and in fp32, and four of them in a row leave fp32's normal range; every kind occurs at R = 45."""
    for S in U.R2O_S:
        for R in U.R2O_R:
            raw, z, d, noise, white = U.r2o_inputs(R, S)
            rgb, disp, acc, w, depth = U.r2o_want(R, S)
            assert bool(((acc == 0) | (acc >= U.ACC_LIVE)).all()), (R, S, acc)
            assert bool((z[:, 1:] >= z[:, :-1]).all())
            dn = d.norm(dim=-1)
            assert bool(((dn == 0) | ((dn > 0.19) & (dn < 3.01))).all())
            for r in range(R):
                kind = U.r2o_kind(r, S)
                if kind in (7, 8):
                    assert acc[r] == 0 and bool((w[r] == 0).all()), (R, S, r)
                if kind in (3, 4):
                    p, n = S // 2, min(1 if kind == 3 else 4, S - S // 2)
                    for dt in (torch.float64, torch.float32):
                        dist = torch.cat([z[r, 1:] - z[r, :-1], torch.full((1,), 1e10)]).to(dt) * d[r].to(dt).norm()
                        sigma = raw[r, :, 3].to(dt) if noise is None else raw[r, :, 3].to(dt) + noise[r].to(dt)
                        alpha = 1. - torch.exp(-torch.relu(sigma) * dist)
                        assert bool((alpha[p:p + n] == 1).all()), (R, S, r, dt)
                    if n == 4 and p + n < S:  # the transmittance behind them: (1e-10)^4, below fp32's smallest normal number
                        assert 0 < w[r, p + n:].sum() < 1.1754944e-38, (R, S, r)
        assert {U.r2o_kind(r, S) for r in range(45)} == set(range(len(U.R2O_KINDS)))


def test_r2o_reference_distance_sets_the_bars():
    """The bars are 4 x the distance of the reference's own fp32 arithmetic from the yardstick over the whole table: measure it,
    print it, and fail if it is above bar / 4 on any output (the table moved: re-derive the bars) or if a bar is beyond the
    existing rtol 3e-5 / atol 3e-6.  The torch-op branch of r2l_amd.render.raw2outputs (S >= 2) passes the same bars, and both
    have disp = NaN exactly on the rays with acc64 == 0 and every other output finite."""
    from r2l_amd.render import raw2outputs
    worst = {k: 0. for k in U.R2O_BARS}
    for S in U.R2O_S:
        for R in U.R2O_R:
            raw, z, d, noise, white = U.r2o_inputs(R, S)
            want = U.r2o_want(R, S)
            sides = [U.raw2outputs32(raw, z, d, noise, white)]
            if S >= 2:
                sides.append(raw2outputs(raw, z, d, 0. if noise is None else 1., white, noise=noise))
            for n, got in enumerate(sides):
                assert torch.equal(torch.isnan(got[1]), want[2] == 0), (R, S)
                assert all(bool(torch.isfinite(got[i]).all()) for i in (0, 2, 3, 4)), (R, S)
                err = U.r2o_errors(got, want, z)
                assert not any(bool(f.any()) for f in U.r2o_failures(err).values()), (R, S, U.r2o_worst(err))
                if n == 0:
                    worst = {k: max(worst[k], v) for k, v in U.r2o_worst(err).items()}
    print("reference fp32 vs fp64 over the table:", {k: "%.3g" % v for k, v in worst.items()})
    for k in U.R2O_BARS:
        assert worst[k] <= U.R2O_REF[k], (k, worst[k])
        assert U.R2O_BARS[k] == 4 * U.R2O_REF[k] and U.R2O_BARS[k] <= U.R2O_BAR_CEILING[k] * (1 + 1e-12), k


@pytest.mark.parametrize("S", U.R2O_PROBE_S)
def test_r2o_self_check_probes_have_live_rays(S):
    """Every probe sample has rays whose w64[p] is above 10 x the weights bar, and with the reference's fp32 outputs as `got` the
    yardstick without that sample fails the weights bar and a map bar on every one of them."""
    R = U.R2O_PROBE_R
    got = U.raw2outputs32(*U.r2o_inputs(R, S))
    res = U.r2o_self_check(got, R, S)
    assert sorted(res) == U.r2o_probes(S) and S - 1 in res and 0 in res
    for p, (live, unseen) in res.items():
        assert live >= 1, (S, p, "no live ray for this probe")
        assert unseen == 0, (S, p, unseen)


def test_r2o_instances_cover_the_dispatch():
    assert {U.r2o_instance(S) for S in U.R2O_S} == {"<1,4>", "<2,4>", "<3,2>", "<4,2>", "16<ROWS=4>", "16<ROWS=8>", "16<ROWS=12>",
                                                   "16<ROWS=16>"}
    assert U.r2o_instance(160) == "<3,2>" and U.r2o_instance(129) == "<3,2>" and U.r2o_instance(191) == "<3,2>"


# ---- coarse depths ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,R", U.STRAT_SHAPES + [U.STRAT_BIG])
def test_strat_spec_is_the_torch_branch_of_coarse_z(S, R):
    """strat_spec == r2l_amd.render._coarse_z on CPU tensors bit for bit, without and with t_rand, for per-ray and shared near /
    far; ttab is linspace ++ (1 - linspace); t_rand holds exact 0 and 1 - 2^-24; near and far differ between rays."""
    from r2l_amd.render import _coarse_z
    near, far, rows, t_rand = U.strat_inputs(R, S)
    assert torch.equal(rows[:, 6:7], near) and torch.equal(rows[:, 7:8], far)
    assert bool((near >= 1.7).all() and (near <= 2.3).all() and (far >= 5.5).all() and (far <= 6.5).all())
    if R > 1:
        assert near.unique().numel() > 1 and far.unique().numel() > 1
    assert bool((t_rand == 0).any()) and (R * S == 1 or bool((t_rand == 1 - 2.**-24).any())) and bool((t_rand < 1).all())
    tt = U.strat_ttab(S)
    t = torch.linspace(0., 1., steps=S)
    assert tt.shape == (2 * S,) and torch.equal(tt[:S], t) and torch.equal(tt[S:], 1. - t)
    for tr in (None, t_rand):
        ref = _coarse_z(near, far, S, False, 0. if tr is None else 1., False, tr)
        got = U.strat_spec(near, far, R, S, tr)
        assert got.shape == (R, S) and torch.equal(bits(got), bits(ref))
        assert bool((got[:, 1:] >= got[:, :-1]).all())
        # one shared pair: what every ray gets is what a one-ray call with that pair gets
        shared = U.strat_spec(near[:1], far[:1], R, S, tr)
        for r in sorted({0, R // 2, R - 1}):
            one = _coarse_z(near[:1], far[:1], S, False, 0. if tr is None else 1., False, None if tr is None else tr[r:r + 1])
            assert torch.equal(bits(shared[r:r + 1]), bits(one))


# ---- importance sampling ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,NI,R", U.PDF_SHAPES)
def test_pdf_tables_and_fp32_reference(S, NI, R):
    """The table's conditions (ascending depths, u[:, 0] = 0, the degenerate rows are what they say, every kind present from
    R = 6), the cap on excused samples, and the fp32 oracle and the torch-op branch of r2l_amd.render.sample_pdf_sort under the
    judgement and the exact facts the kernels are held to."""
    from r2l_amd.render import sample_pdf_sort
    z, w, u = U.pdf_inputs(S, NI, R)
    assert bool((z[:, 1:] >= z[:, :-1]).all()) and bool((u[:, 0] == 0).all()) and bool(((u >= 0) & (u < 1)).all())
    inner = w[:, 1:-1]
    for r in range(R):
        kind = r % len(U.PDF_KINDS)
        if kind == 1:
            assert bool((inner[r] == 0).all())
        elif kind == 2:
            assert int((inner[r] != 0).sum()) == 1 and inner[r].max() == 1
        elif kind == 3:
            nz = (inner[r] != 0).nonzero().flatten()
            assert 1 <= nz.numel() <= 3 and int(nz[-1] - nz[0]) == nz.numel() - 1 and abs(float(inner[r].sum()) - 1) < 1e-6
        elif kind == 4:
            assert 0 < inner[r].max() <= 1e-6
        elif kind == 5 and S >= 3:
            assert bool((z[r, 1:] == z[r, :-1]).any())
    knife, edge = U.pdf_excused_share(S, NI, R)
    print("sample_pdf (%d, %d, %d): knife %.2f %%, edge %.2f %%" % (S, NI, R, 100 * knife, 100 * edge))
    if NI >= 64:
        c = U.pdf_want(S, NI, R)
        assert float((c["knife"] | c["edge"]).double().mean()) <= U.PDF_CAP
    ref32 = O.sample_pdf(U.pdf_bins32(z), inner, NI, det=False, u=u)
    assert ref32.dtype == torch.float32
    ok = U.pdf_judge(ref32, S, NI, R)
    assert bool(ok.all()), (~ok).nonzero()[:10]
    zs, z_all, z_std = sample_pdf_sort(z, w, NI, u=u)
    ok = U.pdf_judge(zs, S, NI, R)
    assert bool(ok.all()), (~ok).nonzero()[:10]
    assert not U.pdf_exact_facts(zs, z_all, z_std, S, NI, R)
    # the judgement is not vacuous: samples moved by a tenth of their ray's depth range fail it
    moved = U.pdf_judge(ref32 + 0.1 * (z[:, -1:] - z[:, :1]), S, NI, R)
    assert float((~moved).double().mean()) > 0.5


def test_pdf_shapes_reach_the_argument_checks_extremes():
    assert {(3, 1), (3, 192), (64, 1), (64, 192)} <= {(S, NI) for S, NI, _ in U.PDF_SHAPES}
    assert all(3 <= S <= 64 and 1 <= NI <= 192 and S + NI <= 256 for S, NI, _ in U.PDF_SHAPES)
    assert [R for S, NI, R in U.PDF_SHAPES if (S, NI) == (64, 128)] == list(U.PDF_QUARTER_R)
