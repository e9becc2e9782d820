"""fp64 yardsticks, input tables and judgements of the teacher's three render stages (csrc/r2l_render.hip), shared by
tests/test_render_stages_cpu.py (which checks them without a GPU) and tests/test_render_stages_gpu.py (which holds the
kernels to them).  Nothing here touches a device.

  r2l_raw2outputs      raw2outputs64: the op sequence of oracle/r2l_oracle.py::raw2outputs in fp64 on the fp32 inputs (bit-equal
                       to it for S >= 2: asserted on the CPU); S = 1 gives the one sample the interval 1e10 |d|.
  r2l_stratified_z     strat_spec: the reference's fp32 expressions, op by op, on CPU tensors — the kernel owes the same bits.
  r2l_sample_pdf_sort  pdf_judge: oracle sample_pdf in fp64 and the bar / excuses of
                       tests/test_teacher_gpu.py::test_sample_pdf_sort_shapes_vs_oracle around it.
"""
import functools

import torch
import torch.nn.functional as F

from oracle import r2l_oracle as O

# ---------------------------------------------------------------------------------------------------------------
# compositing
# ---------------------------------------------------------------------------------------------------------------
# sample counts: the four wave-per-ray instances r2l_raw2outputs_kernel<CH, RPW> with partial last lanes, and the quarter-wave
# kernel's ROWS = 4, 8, 12, 16
R2O_S_WAVE = (1, 2, 63, 65, 127, 129, 160, 191, 193, 255)
R2O_S_QUARTER = (64, 128, 192, 256)
R2O_S = R2O_S_WAVE + R2O_S_QUARTER
# ray counts: below, at and across a wave's rays (RPW = 2 or 4; four per quarter-wave wave) and a workgroup's (8 or 16)
R2O_R = (1, 3, 5, 8, 9, 17, 45)
R2O_KINDS = ("plain", "sigma 0 on every other sample", "duplicated depths", "alpha 1 once in mid-ray",
             "alpha 1 on four consecutive samples", "trained-like magnitudes", "sigma near 0, noise flips its sign",
             "empty: sigma + noise <= 0", "empty: rays_d = 0")
ACC_LIVE = 1e-3  # every ray of the table has acc64 == 0 exactly or acc64 >= ACC_LIVE (asserted on the CPU)

# Bars: 4 x the distance of the reference's OWN fp32 arithmetic (torch on the CPU: raw2outputs32 below) from raw2outputs64 over the
# whole table R2O_S x R2O_R, measured by tests/test_render_stages_cpu.py::test_r2o_reference_distance_sets_the_bars, which
# fails if that distance moves above bar / 4.  The kernels add one ulp per v_exp_f32 / v_rcp_f32 and another association of
# the product and the sums to correctly rounded fp32.  rgb, weights, acc: absolute; depth: absolute of depth / max|z| of the
# ray; disp: relative, on rays with acc64 >= ACC_LIVE.  (reference's own distance -> bar)
# Measured: rgb 4.62e-7, weights 4.80e-7, acc 7.44e-7, depth 5.02e-7, disp 1.43e-6; rounded up to two digits here.
R2O_REF = {"rgb": 4.7e-7, "weights": 4.9e-7, "acc": 7.5e-7, "depth": 5.1e-7, "disp": 1.5e-6}
R2O_BARS = {k: 4 * v for k, v in R2O_REF.items()}
R2O_MAPS = ("rgb", "acc", "depth", "disp")
# no bar may go beyond the existing shapes test's rtol 3e-5 / atol 3e-6 (outputs are O(1))
R2O_BAR_CEILING = {"rgb": 3e-6, "weights": 3e-6, "acc": 3e-6, "depth": 3e-6, "disp": 3e-5}
# self-check: the yardstick without sample p of every ray must fail the bars on every ray with w64[p] > 10 x the weights bar
R2O_PROBE_S = (64, 65, 160, 256)
R2O_PROBE_R = 45


def r2o_probes(S):
    return sorted({p for p in (0, 15, 16, 63, 64, S - 1) if p < S})


def r2o_instance(S):
    """The kernel instance r2l_raw2outputs dispatches S to."""
    if S % 64 == 0:
        return "16<ROWS=%d>" % (S // 16)
    ch = (S + 63) // 64
    return "<%d,%d>" % (ch, 4 if ch <= 2 else 2)


def r2o_kind(r, S):
    return (r + S) % len(R2O_KINDS)


@functools.lru_cache(maxsize=None)
def r2o_inputs(R, S):
    """(raw [R,S,4], z [R,S], rays_d [R,3], noise [R,S] or None, white): ray r is of kind R2O_KINDS[(r + S) % 9].  Noise is given
    for S % 3 != 0, the white background by the parity of R + S, |d| is 0.2 .. 3.  The tensors are shared: do not write to them."""
    g = torch.Generator().manual_seed(R * 1000 + S)
    raw = torch.randn(R, S, 4, generator=g) * 2
    z = torch.sort(torch.rand(R, S, generator=g) * 4 + 2, -1)[0]
    d = torch.randn(R, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True) * (0.2 + 2.8 * torch.rand(R, 1, generator=g))
    noise = torch.randn(R, S, generator=g) * 0.5 if S % 3 != 0 else None
    for r in range(R):
        kind = r2o_kind(r, S)
        if kind == 1:
            raw[r, ::2, 3] = 0.
            if noise is not None:
                noise[r] = 0.
        elif kind == 2:
            z[r, 1::3] = z[r, 0:S - 1:3][:z[r, 1::3].numel()]
        elif kind in (3, 4):
            # depths at least 2 / S apart, so that sigma = 1e5 times the interval times |d| >= 0.2 is at least 156: exp(-156)
            # underflows in fp32 and vanishes beside 1 in fp64 — alpha is exactly 1 on both sides, and the transmittance behind
            # it is 1e-10 (once) or 1e-40 (four times: an fp32 subnormal)
            z[r] = 2 + 4 * (torch.arange(S) + 0.5 * torch.rand(S, generator=g)) / S
            raw[r, S // 2:S // 2 + (1 if kind == 3 else 4), 3] = 1e5
        elif kind == 5:
            raw[r, :, 3] = torch.rand(S, generator=g) * 1100 - 100
            raw[r, :, :3] = torch.rand(S, 3, generator=g) * 20 - 10
        elif kind == 6:
            raw[r, :, 3] = torch.randn(S, generator=g) * 0.1
            if noise is not None:
                noise[r] = -2 * raw[r, :, 3] + torch.randn(S, generator=g) * 0.01
        elif kind == 7:
            raw[r, :, 3] = -raw[r, :, 3].abs() - 0.01
            raw[r, ::3, 3] = 0.
            if noise is not None:
                noise[r] = -noise[r].abs()
                noise[r, ::3] = 0.
        elif kind == 8:
            d[r] = 0.
    return raw, z, d, noise, (R + S) % 2 == 0


def _r2o_ops(raw, z, rays_d, noise, white, drop=None):
    """oracle/r2l_oracle.py::raw2outputs, op by op, in the dtype of its arguments — except that the last interval is built by
    full_like: for S = 1 the one sample gets 1e10 |d| (the oracle expands 1e10 over an empty slice there).  drop = p: alpha of
    sample p of every ray is zeroed (the self-check's missing sample)."""
    dists = torch.cat([z[..., 1:] - z[..., :-1], torch.full_like(z[..., :1], 1e10)], -1)
    dists = dists * torch.norm(rays_d[..., None, :], dim=-1)
    rgb = torch.sigmoid(raw[..., :3])
    sigma = raw[..., 3] if noise is None else raw[..., 3] + noise
    alpha = 1. - torch.exp(-F.relu(sigma) * dists)
    if drop is not None:
        alpha = alpha.clone()
        alpha[:, drop] = 0.
    weights = alpha * torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1. - alpha + 1e-10], -1), -1)[:, :-1]
    rgb_map = torch.sum(weights[..., None] * rgb, -2)
    depth_map = torch.sum(weights * z, -1)
    disp_map = 1. / torch.max(1e-10 * torch.ones_like(depth_map), depth_map / torch.sum(weights, -1))
    acc_map = torch.sum(weights, -1)
    if white:
        rgb_map = rgb_map + (1. - acc_map[..., None])
    return rgb_map, disp_map, acc_map, weights, depth_map


def raw2outputs64(raw, z, rays_d, noise, white, drop=None):
    """(rgb_map, disp_map, acc_map, weights, depth_map) in fp64 from the fp32 inputs: the yardstick."""
    return _r2o_ops(raw.double(), z.double(), rays_d.double(), None if noise is None else noise.double(), white, drop)


def raw2outputs32(raw, z, rays_d, noise, white):
    """The reference's own arithmetic: the same ops in fp32 (torch on the CPU)."""
    return _r2o_ops(raw.float(), z.float(), rays_d.float(), None if noise is None else noise.float(), white)


@functools.lru_cache(maxsize=None)
def r2o_want(R, S, drop=None):
    return raw2outputs64(*r2o_inputs(R, S), drop=drop)


def r2o_errors(got, want, z):
    """Per-ray distances {rgb, weights, acc, depth, disp} [R] of five outputs `got` from the fp64 `want`: the largest absolute one
    over the ray's channels / entries; depth over max|z| of the ray; disp relative, and only on rays with acc64 >= ACC_LIVE (0
    elsewhere).  An entry of `got` that is NaN gives NaN, which no bar admits."""
    g = [t.detach().cpu().double() for t in got]
    zmax = z.double().abs().amax(-1)
    live = want[2] >= ACC_LIVE
    disp = torch.where(live, (g[1] - want[1]).abs() / want[1].abs(), torch.zeros_like(want[1]))
    return {"rgb": _nanmax((g[0] - want[0]).abs()), "weights": _nanmax((g[3] - want[3]).abs()), "acc": (g[2] - want[2]).abs(),
            "depth": (g[4] - want[4]).abs() / zmax, "disp": disp}


def _nanmax(e):
    return torch.where(torch.isnan(e).any(-1), torch.full_like(e[:, 0], float("nan")), e.amax(-1))


def r2o_failures(err, bars=None):
    """{output: [R] bool, True where the ray misses the bar} (NaN misses)."""
    bars = R2O_BARS if bars is None else bars
    return {k: ~(err[k] <= bars[k]) for k in bars}


def r2o_worst(err):
    return {k: float(torch.nan_to_num(v, nan=float("inf")).max()) for k, v in err.items()}


def r2o_self_check(got, R, S, bars=None):
    """The self-check of the bars for one case: for every probe p, the rays with w64[p] > 10 x the weights bar ("live" for p) must
    miss the weights bar AND at least one map bar when `got` is judged against the yardstick without sample p.  Returns
    {p: (number of live rays, number of those the bars do not see)}."""
    bars = R2O_BARS if bars is None else bars
    z = r2o_inputs(R, S)[1]
    w64 = r2o_want(R, S)[3]
    out = {}
    for p in r2o_probes(S):
        live = w64[:, p] > 10 * bars["weights"]
        fail = r2o_failures(r2o_errors(got, r2o_want(R, S, drop=p), z), bars)
        a_map = fail["rgb"] | fail["acc"] | fail["depth"] | fail["disp"]
        out[p] = (int(live.sum()), int((live & ~(fail["weights"] & a_map)).sum()))
    return out


# ---------------------------------------------------------------------------------------------------------------
# coarse depths
# ---------------------------------------------------------------------------------------------------------------
STRAT_SHAPES = [(S, R) for S in (1, 2, 3, 16, 64, 65) for R in (1, 5, 257)]
STRAT_BIG = (65, 16385)  # R S > 4096 x 256: the grid-stride loop takes a second trip
STRAT_LAYOUTS = ("nf_stride 1", "nf_stride 11", "nf_stride 0")


def strat_ttab(S):
    """ttab of r2l_stratified_z, built exactly as r2l_amd/render.py builds it."""
    t = torch.linspace(0., 1., steps=S)
    return torch.cat([t, 1. - t])


@functools.lru_cache(maxsize=None)
def strat_inputs(R, S):
    """(near [R,1], far [R,1], rows [R,11] holding them in columns 6 and 7, t_rand [R,S] with exact 0 and 1 - 2^-24 among its
    entries): near 1.7 .. 2.3 and far 5.5 .. 6.5 differ between rays."""
    g = torch.Generator().manual_seed(R * 1000 + S + 7)
    near = 1.7 + 0.6 * torch.rand(R, 1, generator=g)
    far = 5.5 + torch.rand(R, 1, generator=g)
    rows = torch.randn(R, 11, generator=g)
    rows[:, 6:7], rows[:, 7:8] = near, far
    t_rand = torch.rand(R, S, generator=g)
    flat = t_rand.view(-1)
    flat[::97] = 0.
    flat[5::101] = 1. - 2.**-24
    flat[-1] = 1. - 2.**-24 if flat.numel() > 1 else 0.
    return near, far, rows, t_rand


def strat_spec(near, far, R, S, t_rand=None):
    """z_vals [R,S] by the reference's expressions in fp32, each op rounded on its own (near, far: [R,1], or [1,1] for one shared
    pair) — the torch-op branch of r2l_amd/render.py::_coarse_z (equality asserted on the CPU)."""
    t = torch.linspace(0., 1., steps=S)
    z = near * (1. - t) + far * t
    if t_rand is not None:
        mids = .5 * (z[..., 1:] + z[..., :-1])
        upper = torch.cat([mids, z[..., -1:]], -1)
        lower = torch.cat([z[..., :1], mids], -1)
        z = lower + (upper - lower) * t_rand
    return z.expand(R, S).contiguous()


# ---------------------------------------------------------------------------------------------------------------
# importance sampling
# ---------------------------------------------------------------------------------------------------------------
PDF_QUARTER_R = (1, 3, 5, 16, 17)  # (64, 128, R): the quarter-wave kernel
PDF_SHAPES = [(3, 1, 7), (3, 192, 5), (4, 5, 9), (64, 1, 17), (64, 192, 17), (63, 128, 21)] + [(64, 128, R) for R in PDF_QUARTER_R]
PDF_KINDS = ("random w**3", "all zero", "one-hot", "two or three adjacent bins", "w * 1e-6", "duplicated coarse depths")
PDF_CAP = 0.03  # knife + edge samples of a case with NI >= 64


@functools.lru_cache(maxsize=None)
def pdf_inputs(S, NI, R):
    """(z [R,S] ascending, weights [R,S], u [R,NI] with u[:, 0] = 0); ray r is of kind PDF_KINDS[r % 6].  The degenerate kinds are
    the pdfs of opaque rays: their inner weights sum to 1.  weights[:, 0] and [:, -1], which sample_pdf never sees, stay random."""
    g = torch.Generator().manual_seed(S * 100000 + NI * 100 + R)
    z = torch.sort(torch.rand(R, S, generator=g) * 4 + 2, -1)[0]
    w = torch.rand(R, S, generator=g) ** 3
    u = torch.rand(R, NI, generator=g)
    u[:, 0] = 0.
    nw = S - 2
    for r in range(R):
        kind = r % len(PDF_KINDS)
        if kind == 1:
            w[r, 1:-1] = 0.
        elif kind == 2:
            w[r, 1:-1] = 0.
            w[r, 1 + int(torch.randint(0, nw, (1,), generator=g))] = 1.
        elif kind == 3:
            n = min(2 + r // len(PDF_KINDS) % 2, nw)
            k = 1 + int(torch.randint(0, nw - n + 1, (1,), generator=g))
            part = 0.1 + torch.rand(n, generator=g)
            w[r, 1:-1] = 0.
            w[r, k:k + n] = part / part.sum()
        elif kind == 4:
            w[r] = w[r] * 1e-6
        elif kind == 5:
            z[r, 1::3] = z[r, 0:S - 1:3][:z[r, 1::3].numel()]
    return z, w, u


def pdf_bins32(z):
    """The fp32 bin edges every implementation computes: .5 * (z[1:] + z[:-1])."""
    return .5 * (z[..., 1:] + z[..., :-1])


@functools.lru_cache(maxsize=None)
def pdf_want(S, NI, R):
    """The fp64 side of the judgement for one case: the oracle's sample_pdf on the fp32 inputs and what its bar needs."""
    z, w, u = [t.double() for t in pdf_inputs(S, NI, R)]
    mids = .5 * (z[:, 1:] + z[:, :-1])
    want = O.sample_pdf(mids, w[:, 1:-1], NI, det=False, u=u)
    pdf = (w[:, 1:-1] + 1e-5) / torch.sum(w[:, 1:-1] + 1e-5, -1, keepdim=True)
    cdf = torch.cat([torch.zeros(R, 1, dtype=torch.float64), torch.cumsum(pdf, -1)], -1)
    nb = cdf.shape[-1]
    inds = torch.searchsorted(cdf, u.contiguous(), right=True)
    below, above = (inds - 1).clamp(min=0), inds.clamp(max=nb - 1)
    step = torch.gather(cdf, 1, above) - torch.gather(cdf, 1, below)
    lo_edge, hi_edge = torch.gather(mids, 1, below), torch.gather(mids, 1, above)
    allowed = 1e-5 + 1e-5 * want.abs() + (hi_edge - lo_edge) * 4e-7 / step.clamp_min(1e-5)
    # knife: the cdf step within 3e-7 of the reference's own `denom < 1e-5` discontinuity
    knife = (step - 1e-5).abs() < 3e-7
    # edge: u within 4e-7 of an interior cdf entry — which bin it falls into depends on the rounding of the cdf
    if nb > 2:
        edge = ((u[:, :, None] - cdf[:, None, 1:-1]).abs().amin(-1) < 4e-7)
    else:
        edge = torch.zeros_like(knife)
    # the outer edges of the bins that the neighbouring indices admit
    lo_out = torch.gather(mids, 1, (below - 1).clamp(min=0))
    hi_out = torch.gather(mids, 1, (above + 1).clamp(max=nb - 1))
    return dict(want=want, allowed=allowed, knife=knife, edge=edge, lo_out=lo_out, hi_out=hi_out, cdf=cdf)


def pdf_judge(got, S, NI, R):
    """[R,NI] bool, True where a sample of `got` passes: |got - want| <= 1e-5 + 1e-5 |want| + (hi_edge - lo_edge) * 4e-7 /
    max(step, 1e-5); knife and edge samples only have to lie within lo_out - 1e-5 .. hi_out + 1e-5.  (NaN fails.)"""
    c = pdf_want(S, NI, R)
    g = got.detach().cpu().double()
    close = (g - c["want"]).abs() <= c["allowed"]
    inside = (g >= c["lo_out"] - 1e-5) & (g <= c["hi_out"] + 1e-5)
    return torch.where(c["knife"] | c["edge"], inside, close)


def pdf_excused_share(S, NI, R):
    c = pdf_want(S, NI, R)
    return float(c["knife"].double().mean()), float(c["edge"].double().mean())


def pdf_exact_facts(zs, z_all, z_std, S, NI, R):
    """The facts that hold bit for bit (or, z_std, as tests/test_teacher_gpu.py holds them) for any implementation's outputs on
    the CPU: returns a list of the ones violated."""
    z, w, u = pdf_inputs(S, NI, R)
    zs, z_all, z_std = zs.detach().cpu(), z_all.detach().cpu(), z_std.detach().cpu()
    bad = []
    first = pdf_want(S, NI, R)["cdf"][:, 1] > 0  # (always: every pdf entry is at least 1e-5 / total)
    if not torch.equal(zs[first, 0].view(torch.int32), pdf_bins32(z)[first, 0].view(torch.int32)):
        bad.append("u = 0 does not give bins[:, 0] bit for bit")
    if not torch.equal(z_all.view(torch.int32), torch.sort(torch.cat([z, zs], -1), -1)[0].view(torch.int32)):
        bad.append("z_all is not torch.sort(cat[z, z_samples])")
    if not torch.allclose(z_std, torch.std(zs, dim=-1, unbiased=False), rtol=1e-4, atol=1e-6):
        bad.append("z_std")
    return bad
