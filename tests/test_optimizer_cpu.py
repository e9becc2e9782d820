"""The optimizer stage's yardstick (tests/optim_util.py) checked without a GPU: the bars hold for a numpy fp32 restatement of the
kernel's sequence in both contraction forms and reject seven mutations of it; adam64 is torch.optim.Adam; the distance to
torch's fp32 Adam is the documented one; loss64 and the restated fp16x2 stream layouts are what they claim to be.
Every test prints the figures it asserts (pytest -s): profiles/optimizer_yardstick.txt quotes them."""
import math

import numpy as np
import pytest
import torch

from oracle import r2l_oracle as O
from tests import optim_util as OU

T = torch.from_numpy
N = 400000


@pytest.fixture(scope="module")
def base():
    return OU.adam_inputs(N, 0)


@pytest.fixture(scope="module")
def cases(base):
    """setting name -> ((p, g, m, v) numpy fp32, adam64 of them): computed once, shared, never written to."""
    out = {}
    for st in OU.SETTINGS:
        name, step, s, b1, b2, eps, lr = st
        arrs = OU.for_setting(base, st)
        out[name] = (arrs, OU.adam64(*[T(a) for a in arrs], lr, b1, b2, eps, step, s))
    return out


def test_inputs_cover_what_the_bars_are_about(cases):
    """Every setting's inputs hold exact-zero gradients, fresh (m = v = 0) entries, the N_CANCEL cancelling entries (|M| tiny
    against |m| + |gi|), gradients across 1e-12 .. 1e3, sqrt(V) on both sides of eps, and no V in (0, 2^-100)."""
    for st in OU.SETTINGS:
        name, step, s, b1, b2, eps, lr = st
        (p, g, m, v), ref = cases[name]
        assert (g == 0).sum() > 0.03 * N and ((m == 0) & (v == 0)).sum() > 0.03 * N
        c = slice(OU.CANCEL_AT, OU.CANCEL_AT + OU.N_CANCEL)
        live = T(m[c]) != 0
        ratio = (ref.M[c].abs() / (ref.Em[c] / OU.U))[live]
        assert live.sum() > 900 and ratio.max().item() < 1e-6, (name, ratio.max().item())
        nz = np.abs(g[g != 0]) * OU.f32(s)
        assert nz.min() < 1e-11 * OU.f32(s) * 10 and nz.max() > 1e2 * OU.f32(s)
        V = ref.V
        assert not ((V > 0) & (V < OU.V_MIN)).any()
        assert (V.sqrt() < 0.1 * eps).sum() > 100 and (V.sqrt() > 10 * eps).sum() > 100, name
        assert torch.isfinite(ref.P).all() and torch.isfinite(ref.Ep).all()


@pytest.mark.parametrize("fma", [False, True], ids=["plain", "fma"])
@pytest.mark.parametrize("setting", OU.SETTINGS, ids=OU.SETTING_IDS)
def test_restatement_within_bars(cases, setting, fma):
    name, step, s, b1, b2, eps, lr = setting
    arrs, ref = cases[name]
    p1, m1, v1 = OU.adam32(*arrs, lr, b1, b2, eps, step, s, fma=fma)
    fr = OU.fractions(T(p1), T(m1), T(v1), ref)
    print("YARDSTICK cpu restatement %s %s: m %.3f Em  v %.3f Ev  p %.3f Ep" % (name, "fma" if fma else "plain", fr["m"], fr["v"], fr["p"]))
    for k in fr:
        assert fr[k] <= OU.BARS[k], (k, fr)


# by how many times its bar each mutant misses it, in its best setting: measured (400 000 entries; the plain form), asserted at the
# power of ten below — never under 100
MUTANT_FACTOR = {"no_root_bc2": 1e5, "step_minus_1": 1e5, "b2_as_b1": 1e8, "g2_unscaled": 1e13, "eps_in_root": 1e5,
                 "eps_before_div": 1e5, "old_m": 1e5}
# where a mutant computes the same numbers as the kernel (nothing to see): bias corrections that are 1, grad_scale = 1
MUTANT_BLIND = {"no_root_bc2": ("step200000", "stepmax"), "step_minus_1": ("step200000", "stepmax"),
                "eps_before_div": ("step200000", "stepmax"), "g2_unscaled": ("step1", "step200000", "stepmax")}


@pytest.mark.parametrize("mutant", OU.MUTANTS)
def test_mutant_misses_a_bar(cases, mutant):
    factors = {}
    for setting in OU.SETTINGS:
        name, step, s, b1, b2, eps, lr = setting
        arrs, ref = cases[name]
        p1, m1, v1 = OU.adam32(*arrs, lr, b1, b2, eps, step, s, mutant=mutant)
        fr = OU.fractions(T(p1), T(m1), T(v1), ref)
        factors[name] = max(fr[k] / OU.BARS[k] for k in fr)
    finite = {k: f for k, f in factors.items() if math.isfinite(f)}
    best = max(finite, key=finite.get)
    print("YARDSTICK cpu mutant %s: misses a bar by %.3g x (%s); per setting %s"
          % (mutant, finite[best], best, {k: "%.3g" % f for k, f in factors.items()}))
    assert MUTANT_FACTOR[mutant] >= 100
    assert finite[best] >= MUTANT_FACTOR[mutant], factors
    for name in MUTANT_BLIND.get(mutant, ()):
        assert factors[name] <= 1.0, (name, factors[name])  # the same numbers as the kernel there: within the bars
    caught = [k for k, f in factors.items() if f >= 100]
    assert len(caught) >= len(OU.SETTINGS) - len(MUTANT_BLIND.get(mutant, ())), factors


def _scaled_err(a, b, scale):
    ok = scale > 0
    return ((a - b).abs()[ok] / scale[ok]).max().item()


@pytest.mark.parametrize("step,b1,b2,eps,lr", [(1, 0.9, 0.999, 1e-8, 5e-4), (7, 0.9, 0.999, 1e-8, 1e-4), (1000, 0.5, 0.9, 1e-3, 3e-4),
                                               (200000, 0.9, 0.999, 1e-8, 5e-5)])
def test_adam64_is_the_oracle_and_torch_in_fp64(step, b1, b2, eps, lr):
    """With the decimal betas as doubles, adam64 agrees with oracle.adam_step and with torch.optim.Adam on float64 tensors to 1e-14,
    relative to the size of the terms of each sum (|m| + |g|, V, |p| + |P|) and, for the update itself, to |P - p|."""
    n = 20000
    p, g, m, v = [T(a).double() for a in OU.adam_inputs(n, 3)]
    ref = OU.adam64(p, g, m, v, lr, b1, b2, eps, step, 1.0, exact_scalars=True)
    po, mo, vo = O.adam_step(p, g, m, v, step, lr, b1, b2, eps)
    par = torch.nn.Parameter(p.clone())
    opt = torch.optim.Adam([par], lr=lr, betas=(b1, b2), eps=eps)
    group = opt.state_dict()["param_groups"][0]
    opt.load_state_dict({"state": {0: {"step": torch.tensor(float(step - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}},
                         "param_groups": [group]})
    par.grad = g.clone()
    opt.step()
    st = opt.state[par]
    assert float(st["step"]) == step and par.dtype == torch.float64 and st["exp_avg"].dtype == torch.float64
    worst = 0.0
    for what, (p2, m2, v2) in (("oracle", (po, mo, vo)), ("torch", (par.detach(), st["exp_avg"], st["exp_avg_sq"]))):
        errs = (_scaled_err(m2, ref.M, m.abs() + g.abs()), _scaled_err(v2, ref.V, ref.V),
                _scaled_err(p2, ref.P, p.abs() + ref.P.abs()), _scaled_err(p2 - p, ref.P - p, (ref.P - p).abs()))
        worst = max(worst, *errs[:3])
        assert max(errs[:3]) <= 1e-14, (what, errs)
        # the update S M / D inherits M's cancellation (|M| against |m| + |g|: down to 1e-4 in these inputs) and the
        # rounding of p - update back into p's grid, so it is held at 1e-9 of itself
        assert errs[3] <= 1e-9, (what, errs)
    print("YARDSTICK cpu adam64 vs oracle / torch fp64, step %d: worst relative distance %.2e" % (step, worst))


def test_distance_to_torch_fp32_adam():
    """torch.optim.Adam on CPU fp32 tensors, ten steps from a fresh state with a new wide-range gradient at every step.  After each
    step torch's (p, m, v) lie within torch_allowance (tests/optim_util.py: the two weight constants and the bias corrections
    torch forms differently, on top of the fp32 bars) of adam64 applied to torch's own previous state — per step, so nothing
    accumulates.  Measured relative distances (the contract documented beside r2l_adam_one, in include/r2l_hip.h and DESIGN.md):
    v up to 1.30e-5 of V (entries whose V is all increment), m up to 7.2e-8 of |m| + |g|, the update up to 7.8e-6 of itself at
    steps 1 .. 10 (half of v's distance and half of the bias correction's 1.29e-5, which mostly cancel; p's own grid adds ~1e-6)."""
    n, lr, b1, b2, eps = 50000, 5e-4, 0.9, 0.999, 1e-8
    p0 = T(OU.adam_inputs(n, 5)[0])
    par = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([par], lr=lr, betas=(b1, b2), eps=eps, foreach=False)
    m = torch.zeros(n)
    v = torch.zeros(n)
    worst = {"m": 0.0, "v": 0.0, "p": 0.0}
    rel = {"m": 0.0, "v": 0.0, "upd": 0.0}
    free = [p0.double(), m.double(), v.double()]  # adam64 left to itself for the ten steps: the accumulated distance, reported
    for step in range(1, 11):
        g = OU.for_setting([p0.numpy()] + OU.adam_inputs(n, 100 + step)[1:], ("torch", step, 1.0, b1, b2, eps, lr))[1]
        if step > 1:  # (for_setting looked at a v that is not this run's: redo its rule on the real state)
            gi = g.astype(np.float64)
            V = v.double().numpy() * OU.f32(b2) + gi * gi * (1 - OU.f32(b2))
            g[(V > 0) & (V < OU.V_MIN)] = 0.0
        g = T(g)
        prev = [par.detach().clone(), m.clone(), v.clone()]
        par.grad = g.clone()
        opt.step()
        st = opt.state[par]
        m, v = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
        assert par.dtype == m.dtype == v.dtype == torch.float32
        ref = OU.adam64(prev[0], g, prev[1], prev[2], lr, b1, b2, eps, step, 1.0)
        allow = OU.torch_allowance(ref, g, prev[1], lr, b1, b2, eps, step)
        fr = OU.fractions(par.detach(), m, v, ref, extra=allow)
        for k in fr:
            worst[k] = max(worst[k], fr[k])
            assert fr[k] <= 1.0, (step, k, fr)
        rel["m"] = max(rel["m"], _scaled_err(m.double(), ref.M, prev[1].double().abs() + g.double().abs()))
        rel["v"] = max(rel["v"], _scaled_err(v.double(), ref.V, ref.V))
        upd = prev[0].double() - ref.P
        # (entries whose update is at least a tenth of p: below that p's own grid hides the update's relative error)
        big = upd.abs() > 0.1 * prev[0].double().abs()
        rel["upd"] = max(rel["upd"], _scaled_err((prev[0].double() - par.detach().double())[big], upd[big], upd[big].abs()))
        f = OU.adam64(free[0], g, free[1], free[2], lr, b1, b2, eps, step, 1.0)
        free = [f.P, f.M, f.V]
    drift = ((par.detach().double() - free[0]).abs().max().item() / lr)
    print("YARDSTICK cpu torch fp32 Adam vs adam64, steps 1..10: fraction of the allowance m %.3f v %.3f p %.3f; relative distance "
          "m %.2e (of |m|+|g|) v %.2e (of V) update %.2e (of itself); free-running distance after 10 steps %.2e lr"
          % (worst["m"], worst["v"], worst["p"], rel["m"], rel["v"], rel["upd"], drift))
    # the documented numbers: the constants' differences show, and nothing beyond them
    assert 1.0e-5 <= rel["v"] <= 1.4e-5 and rel["m"] <= 4e-7 and rel["upd"] <= 1.5e-5, rel
    # without the constants' terms the distance is NOT covered by the fp32 bars alone: the caveat is real
    ref = OU.adam64(prev[0], g, prev[1], prev[2], lr, b1, b2, eps, 10, 1.0)
    assert OU.fractions(par.detach(), m, v, ref)["v"] > 10 * OU.BARS["v"]


def test_weight_constants():
    """The numbers the documents quote: 1.0f - 0.999f = 0.00099998713 against 0.001f (1.29e-5 apart), 1.0f - 0.9f against 0.1f
    (2.2e-7), and beta + (1 - beta) = 1 exactly only for the library's pair."""
    F = np.float32
    for b, lo, hi in ((0.999, 1.28e-5, 1.30e-5), (0.9, 2.1e-7, 2.4e-7)):
        ours, theirs = F(1) - F(b), F(1.0 - b)
        assert lo < abs(float(theirs) - float(ours)) / float(ours) < hi
        assert float(F(b)) + float(ours) == 1.0 and float(F(b)) + float(theirs) != 1.0
    assert abs(float(F(1) - F(0.999)) - 0.00099998713) < 1e-11


# ---- loss64 -----------------------------------------------------------------------------------------------------------------------
def _finish32(partials, inv_denom):
    """r2l_loss_finish_kernel in numpy: fp64 strided sums of 256 threads, a binary tree, one rounding to fp32, logf / logf."""
    x = np.asarray(partials, dtype=np.float32).astype(np.float64)
    red = np.array([x[t::256].sum() for t in range(256)])
    k = 128
    while k > 0:
        red[:k] += red[k:2 * k]
        k >>= 1
    F = np.float32
    with np.errstate(divide="ignore", invalid="ignore"):
        mse = F(red[0] * float(F(inv_denom)))
        psnr = F(-10.0) * np.log(mse) / np.log(F(10.0))
    assert psnr.dtype == np.float32
    return float(mse), float(psnr)


@pytest.mark.parametrize("inv_denom", [1.0 / 3, 1.0 / (3 * 4096)])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 100003])
def test_loss64_bars_hold_for_the_restatement(n, inv_denom):
    rng = np.random.default_rng(n)
    x = (10.0 ** rng.uniform(-8, 2, n)).astype(np.float32)
    mse, psnr, bm, bp = OU.loss64(x, inv_denom)
    m32, p32 = _finish32(x, inv_denom)
    assert abs(mse - float(np.sum(x.astype(np.float64))) * OU.f32(inv_denom)) <= 1e-12 * mse
    assert abs(psnr + 10 * math.log10(mse)) <= 1e-12
    print("YARDSTICK cpu loss restatement n=%d: mse %.3f of its bar, psnr %.3f of its bar" % (n, abs(m32 - mse) / bm, abs(p32 - psnr) / bp))
    assert abs(m32 - mse) <= bm and abs(p32 - psnr) <= bp
    # the bars see a wrong constant: log2 for ln, a dropped factor
    assert abs(p32 * math.log(2.0) - psnr) > 100 * bp or abs(psnr) < 1e-3
    assert abs(m32 * (1 + 1e-5) - mse) > 10 * bm


def test_loss64_edges():
    assert OU.loss64(np.zeros(7, np.float32), 1 / 3)[:2] == (0.0, float("inf"))
    assert OU.loss64(np.zeros(0, np.float32), 1 / 3)[:2] == (0.0, float("inf"))
    assert _finish32(np.zeros(7, np.float32), 1 / 3) == (0.0, float("inf"))
    x = np.ones(300, np.float32)
    x[123] = np.nan
    assert all(math.isnan(q) for q in OU.loss64(x, 1 / 3)[:2]) and all(math.isnan(q) for q in _finish32(x, 1 / 3))


# ---- the restated fp16x2 stream layouts ------------------------------------------------------------------------------------------------
def test_split16():
    """(hi, mid) bit patterns of the planted values, and hi + mid = w to 2^-22 relative over fp16's normal range."""
    hi, mid = OU.split16(np.array([0.0, -0.0, 65504.0, 7e4, 1e-8, 1.0, -2.5, 1e-3], dtype=np.float32))
    assert list(hi[:5]) == [0x0000, 0x8000, 0x7BFF, 0x7C00, 0x0000]
    assert list(mid[:5]) == [0x0000, 0x0000, 0x0000, 0xFC00, 0x0000]
    assert (hi[5], mid[5]) == (0x3C00, 0) and (hi[6], mid[6]) == (0xC100, 0)
    assert 0 < (mid[7] & 0x7FFF) < 0x0400  # 1e-3: the mid half is an fp16 subnormal
    rng = np.random.default_rng(0)
    w = (rng.uniform(-1, 1, 100000) * 10.0 ** rng.uniform(-3, 4.5, 100000)).astype(np.float32)
    w = w[np.abs(w) < 60000]
    hi, mid = OU.split16(w)
    back = hi.view(np.float16).astype(np.float64) + mid.view(np.float16).astype(np.float64)
    assert (np.abs(back - w) <= 2.0 ** -22 * np.abs(w) + 2.0 ** -25).all()


@pytest.mark.parametrize("n_block", [0, 1, 3])
def test_stream_gathers_are_permutations(n_block):
    """Every head weight, every body weight and every head / body bias appears exactly once in the forward stream's gather, every
    body weight exactly once in the backward stream's; the tail never (the kernels read it from the flat parameters); the two
    streams hold the same body weights, the backward one transposed."""
    idx, kind = OU.fwd_gather(n_block)
    assert idx.shape[0] == OU.fwd_stages(n_block) + OU.PAD_STAGES and (kind[OU.fwd_stages(n_block):] == 3).all()
    s, h, o = OU._within()
    keep = np.ones(4096, bool)
    got = []
    for g in range(idx.shape[0]):
        if kind[g] == 0:
            got.append(idx[g])
        elif kind[g] in (1, 2):
            got.append(idx[g][(h == 0) & (s == 0)])
    got = np.sort(np.concatenate(got))
    assert np.array_equal(got, np.arange(OU.off_tail_w(n_block)))
    assert OU.param_count(n_block) == OU.off_tail_w(n_block) + 771
    bidx = OU.bwd_gather(n_block)
    assert bidx.shape[0] == OU.bwd_stages(n_block) + OU.PAD_STAGES
    body = np.sort(bidx[bidx >= 0])
    want = np.concatenate([np.arange(OU.off_body_w(l), OU.off_body_b(l)) for l in range(2 * n_block)]) if n_block else np.zeros(0, np.int64)
    assert np.array_equal(body, want)
    if n_block:
        # stage kb of layer l, forward: (o, in) = W[o][in]; backward (blocks reversed, second layer first): W[in][o]
        flat = np.arange(OU.param_count(n_block), dtype=np.int64)
        l, kb = 1, 5
        fw = idx[64 + 17 * l + 1 + kb] - OU.off_body_w(l)
        bw = bidx[34 * (n_block - 1) + 1 + kb] - OU.off_body_w(l)
        assert np.array_equal(fw // 256, o) and np.array_equal(bw % 256, o) and np.array_equal(fw % 256, bw // 256)
        assert np.array_equal(np.unique(fw % 256), np.arange(16 * kb, 16 * kb + 16))
    # the head: lane half h holds samples 8 h .. 8 h + 7 (columns 504 h .. 504 h + 503), frequencies paired (sin f, cos f)
    col = OU.head_column(np.arange(63)[:, None], np.arange(8)[None, :], 1)
    assert col.min() == 504 and col.max() == 1007 and np.unique(col).size == 504
    assert OU.head_column(0, 0, 0) == 0 and OU.head_column(0, 1, 0) == 10 and OU.head_column(60, 0, 0) == 20
