"""Test infrastructure: an fp64 yardstick of the optimizer stage (csrc/r2l_train.hip), per entry, with derived bars.

adam64 — the update of r2l_adam_step / _guarded / _packed in fp64
---------------------------------------------------------------
The tensors are the kernel's fp32 inputs promoted to fp64; the scalars lr, b1, b2, eps, s (grad_scale) are the fp32 values the
C ABI receives, promoted exactly (f32() below) — in particular 1 - b is formed from the fp32 b, as the kernel does.  u = 2^-24.

    gi = g s          M = m + (gi - m)(1 - b1)        V = v b2 + gi^2 (1 - b2)
    S  = lr / (1 - b1^step)     D = sqrt(V) / sqrt(1 - b2^step) + eps      P = p - S M / D
    Em = u (|m| + |gi|)         Ev = u V        Ep = u (|p| + |P|) + S Em / D + u |S M / D|

Bars per entry:  |m' - M| <= 4 Em,   |v' - V| <= 6 Ev,   |p' - P| <= 8 Ep.  They are rounding counts of r2l_adam_one's fp32
sequence (every fp32 operation is off by at most u relative to its own result; fused multiply-adds only remove roundings):

  m'  gi = fl(g s): u |gi|.  d = fl(gi - m): u |d| <= u (|gi| + |m|).  t = fl(d (1 - b1)): u |t| <= u |d| ((1 - b1) is exact: b1
      lies in [1/2, 1]).  m' = fl(m + t): u |m'|, and m' is a convex combination of m and gi.  The errors of gi and d reach m'
      scaled by (1 - b1) <= 1/2.  Sum: at most u (|m| + |gi|) (1/2 + 1/2 + 1/2 + 1) < 4 Em.
  v'  every term is non-negative, so relative errors carry through the sum: gi (1), its square (doubles it: 2, plus the
      product's own: 3), times (1 - b2) (4; the factor itself is one fp32 subtraction of exact operands and is the SAME
      number in the reference), the final sum (5); the other branch v b2 has 1 + 1.  5 roundings at most: 6 Ev leaves one
      for second-order terms.  (Subnormal flushing is not part of this contract: inputs keep V >= 2^-100 or V == 0 exactly.)
  p'  on the update S M / D: S = fl(lr / fl(bc1)) 2, sqrt 1 (+ v' relative error 5/2), the division by fl(sqrt(bc2)) 2, + eps 1,
      M / D 1, times S 1: about 11 relative roundings on |S M / D|, which is at most |p| + |P|; the absolute error of m'
      (4 Em) reaches p' through S / D; the final subtraction rounds once more on |p'|.  So
      |p' - P| <= 4 S Em / D + 11 u |S M / D| + u |P| <= 8 (u (|p| + |P|) + S Em / D + u |S M / D|) = 8 Ep with room to spare.

adam32 restates the kernel's sequence in numpy fp32 (with or without the contractions hipcc may make) and, by name, seven
mutations of it; tests/test_optimizer_cpu.py holds the restatement to the bars and every mutant out of them by >= 100 x.

Distance to torch.optim.Adam in fp32 (torch_allowance)
------------------------------------------------------
The library forms 1 - b from the fp32 b it receives: 1.0f - 0.999f = 0.00099998713, so that b + (1 - b) = 1 holds in the
arithmetic that is run.  torch passes the fp32 roundings of the two DOUBLES b and 1 - b: 0.999f beside 0.001f.  The pairs differ by
dl2 = |0.001f - (1.0f - 0.999f)| / (1.0f - 0.999f) = 1.29e-5 in the weight of g^2 and by dl1 = 2.2e-7 in the weight of g - m.
torch's bias corrections come from the double b, the library's from the promoted fp32 b: 1 - b^step differs by up to
1.29e-5 relative for b2 (small steps), 1.5e-7 for b1.  First order, for one step from a common fp32 state:

    Am = 4 Em + dl1 |gi - m| (1 - b1)              Av = 6 Ev + dl2 gi^2 (1 - b2)
    Ap = 8 Ep + 1.01 [ (S / D) dl1 |gi - m| (1 - b1) + |S M / D| (dS + dD) ],
         dS = |bc1_t - bc1| / bc1_t,  dD = (dl2 gi^2 (1 - b2) / V + |bc2_t - bc2| / bc2_t) / 2   (the root halves both)

(1.01: the second-order terms.)  The constants are computed from the number formats, not measured.

loss64 — r2l_loss_finish
------------------------
fp64 sum of the partials times the fp32 inv_denom, and -10 log10 of it.  Bars: mse 2 u relative (the kernel sums and scales in
fp64 and rounds once); psnr (10 / ln 10) (4 u |ln mse| + 4 u) + u |psnr|: two logf calls at 2 ulp each act on |ln mse| (the
quotient ln mse / ln 10 carries both relative errors), the fp32 mse itself is off by u (an absolute u in its logarithm), and
the product with -10 and the quotient round once each.

fp16x2 streams
--------------
fwd_stream_bits / bwd_stream_bits restate the layout-2 weight streams as numpy gathers over the flat parameters
(csrc/r2l_f2.h f2_pack_fwd_element; the layout comment above r2l_adam_pack_kernel and csrc/r2l_bwd2.hip r2l_pack_bwd2_kernel) and
give the (hi, mid) fp16 bit patterns: hi = fp16(w), mid = fp16(w - hi).
"""
import collections
import math

import numpy as np
import torch

U = 2.0 ** -24
V_MIN = 2.0 ** -100
INT_MAX = 2 ** 31 - 1


def f32(x):
    """The fp32 value a C float argument receives, as a Python float (exact)."""
    return float(np.float32(x))


# (name, step, grad_scale, beta1, beta2, eps, lr): the settings every per-entry test of the update runs
SETTINGS = [
    ("step1", 1, 1.0, 0.9, 0.999, 1e-8, 1.02e-4),
    ("step2_s8", 2, 1.0 / 8, 0.9, 0.999, 1e-8, 1.04e-4),
    ("step7_s3", 7, 1.0 / 3, 0.9, 0.999, 1e-8, 1.14e-4),
    ("step1000_s4096", 1000, 2.0 ** -12, 0.9, 0.999, 1e-8, 4.9e-4),
    ("step200000", 200000, 1.0, 0.9, 0.999, 1e-8, 2.0e-4),
    ("step7_beta", 7, 1.0 / 3, 0.5, 0.9, 1e-3, 5e-4),
    ("stepmax", INT_MAX, 1.0, 0.9, 0.999, 1e-8, 5e-5),
]
SETTING_IDS = [s[0] for s in SETTINGS]

Adam64 = collections.namedtuple("Adam64", "P M V Ep Em Ev")


def adam64(p, g, m, v, lr, b1, b2, eps, step, s, exact_scalars=False):
    """One Adam step in fp64 (module docstring).  p, g, m, v: torch tensors of any float dtype and device (promoted);
    returns Adam64(P, M, V, Ep, Em, Ev) in fp64 on the same device.  Non-finite inputs propagate as IEEE says.
    exact_scalars: take the scalars as the doubles they are (comparisons with other fp64 statements of Adam) instead of the fp32
    values the C ABI would receive."""
    p, g, m, v = [t.detach().to(torch.float64) for t in (p, g, m, v)]
    if not exact_scalars:
        lr, b1, b2, eps, s = f32(lr), f32(b1), f32(b2), f32(eps), f32(s)
    step = int(step)
    gi = g * s
    M = m + (gi - m) * (1.0 - b1)
    V = v * b2 + gi * gi * (1.0 - b2)
    S = lr / (1.0 - b1 ** step)
    D = V.sqrt() / math.sqrt(1.0 - b2 ** step) + eps
    upd = S * M / D
    P = p - upd
    Em = U * (m.abs() + gi.abs())
    Ev = U * V
    Ep = U * (p.abs() + P.abs()) + S * Em / D + U * upd.abs()
    return Adam64(P, M, V, Ep, Em, Ev)


BARS = {"m": 4.0, "v": 6.0, "p": 8.0}


def fractions(p1, m1, v1, ref, extra=None):
    """Largest |out - ref| in units of (Em, Ev, Ep) over the entries whose reference is finite -> {'m', 'v', 'p'} (floats; to be
    held against BARS).  An entry whose unit is 0 must match exactly (else inf).  extra: {'m' | 'v' | 'p': tensor}, an absolute
    allowance added to BARS[k] * unit — then the result is in units of that whole allowance and is to be held against 1."""
    out = {}
    for k, got, want, unit in (("m", m1, ref.M, ref.Em), ("v", v1, ref.V, ref.Ev), ("p", p1, ref.P, ref.Ep)):
        if extra is not None:
            unit = BARS[k] * unit + extra[k]
        ok = torch.isfinite(want) & torch.isfinite(unit)
        diff = (got.to(torch.float64) - want).abs()[ok]
        unit = unit[ok]
        frac = torch.where(diff == 0, torch.zeros_like(diff), diff / unit)  # (0 / 0 -> 0, x / 0 -> inf, NaN stays)
        frac = torch.nan_to_num(frac, nan=float("inf"))
        out[k] = frac.max().item() if frac.numel() else 0.0
    return out


def nonfinite_agree(p1, m1, v1, ref):
    """Are p', m', v' non-finite in exactly the entries where the reference is?"""
    return all(torch.equal(torch.isfinite(got), torch.isfinite(want))
               for got, want in ((p1, ref.P), (m1, ref.M), (v1, ref.V)))


# ---- inputs ----------------------------------------------------------------------------------------------------------------
N_CANCEL, CANCEL_AT = 1000, 300  # entries [300, 1300): gi (1 - b1) cancels m b1


def _logu(rng, n, lo, hi):
    return (10.0 ** rng.uniform(lo, hi, n)) * rng.choice([-1.0, 1.0], n)


def adam_inputs(n, seed=0):
    """(p, g, m, v) numpy fp32 [n]: |g| log-uniform over 1e-12 .. 1e3 with 5 % exact zeros; m half of the time near g's size,
    else independent over the same range; v = (|g| 10^U(-1,1))^2, or the size of m^2 where g is 0; 5 % of the entries in
    the state of a first step (m = v = 0); |p| over 1e-3 .. 4."""
    rng = np.random.default_rng(seed)
    g = _logu(rng, n, -12, 3)
    m = np.where(rng.random(n) < 0.5, g * rng.uniform(0.3, 3.0, n) * rng.choice([-1.0, 1.0], n), _logu(rng, n, -12, 3))
    g[rng.random(n) < 0.05] = 0.0
    v = (np.where(g != 0, np.abs(g), np.abs(m)) * 10.0 ** rng.uniform(-1, 1, n)) ** 2
    fresh = rng.random(n) < 0.05
    m[fresh] = 0.0
    v[fresh] = 0.0
    p = _logu(rng, n, -3, 0.6)
    return [a.astype(np.float32) for a in (p, g, m, v)]


def for_setting(base, setting):
    """Copies of (p, g, m, v) fitted to a setting: the N_CANCEL entries from CANCEL_AT on get the gradient whose share cancels
    the old moment's (M is within rounding of 0), and entries with 0 < V < 2^-100 are zeroed (g = v = 0: V == 0 exactly)."""
    _, step, s, b1, b2, eps, lr = setting
    p, g, m, v = [a.copy() for a in base]
    b1f, sf = np.float32(b1), np.float32(s)
    hi = min(g.shape[0], CANCEL_AT + N_CANCEL)
    if hi > CANCEL_AT:
        with np.errstate(over="ignore"):
            g[CANCEL_AT:hi] = -m[CANCEL_AT:hi] * b1f / (np.float32(1) - b1f) / sf
    gi = g.astype(np.float64) * float(sf)
    V = v.astype(np.float64) * f32(b2) + gi * gi * (1.0 - f32(b2))
    small = (V > 0) & (V < V_MIN)
    g[small] = 0.0
    v[small] = 0.0
    return p, g, m, v


# ---- the kernel's sequence in numpy fp32, and its mutants ------------------------------------------------------------------------
MUTANTS = ("no_root_bc2", "step_minus_1", "b2_as_b1", "g2_unscaled", "eps_in_root", "eps_before_div", "old_m")


def _fma(a, b, c):
    # fp32 operands: the product is exact in fp64; the sum rounds to fp64 and then to fp32 (a double rounding that differs from
    # a true fused multiply-add in ~2^-29 of the cases by one ulp: immaterial for a model of the contraction)
    return (a.astype(np.float64) * np.float64(b) + np.asarray(c, dtype=np.float64)).astype(np.float32)


def adam32(p, g, m, v, lr, b1, b2, eps, step, s, fma=False, mutant=None):
    """r2l_adam_one and its host-side constants (csrc/r2l_train.hip) on numpy fp32 arrays -> (p', m', v').  fma: with the
    contractions a compiler may make (m + d c, v b + q, p - S q as fused multiply-adds).  mutant: one of MUTANTS."""
    assert mutant is None or mutant in MUTANTS
    F = np.float32
    one = F(1)
    lrf, b1f, b2f, epsf, sf = F(lr), F(b1), F(b2), F(eps), F(s)
    if mutant == "b2_as_b1":
        b2f = b1f
    k = int(step) - 1 if mutant == "step_minus_1" else int(step)
    bc1 = 1.0 - float(b1f) ** k
    bc2 = 1.0 - float(b2f) ** k
    with np.errstate(all="ignore"):
        step_size = lrf / F(bc1)
        sqrt_bc2 = F(math.sqrt(bc2))
        omb1, omb2 = one - b1f, one - b2f
        gi = g * sf
        d = gi - m
        mi = _fma(d, omb1, m) if fma else m + d * omb1
        gg = g * g if mutant == "g2_unscaled" else gi * gi
        vi = _fma(v, b2f, gg * omb2) if fma else v * b2f + gg * omb2
        if mutant == "no_root_bc2":
            denom = np.sqrt(vi) / F(bc2) + epsf
        elif mutant == "eps_in_root":
            denom = np.sqrt(vi / F(bc2) + epsf)
        elif mutant == "eps_before_div":
            denom = (np.sqrt(vi) + epsf) / sqrt_bc2
        else:
            denom = np.sqrt(vi) / sqrt_bc2 + epsf
        q = (m if mutant == "old_m" else mi) / denom
        p1 = _fma(q, -step_size, p) if fma else p - step_size * q
    for a in (p1, mi, vi):
        assert a.dtype == np.float32
    return p1, mi, vi


# ---- torch.optim.Adam in fp32 ---------------------------------------------------------------------------------------------------
def torch_allowance(ref, g, m, lr, b1, b2, eps, step, s=1.0):
    """{'m', 'v', 'p'}: what torch.optim.Adam(betas=(b1, b2)) — b1, b2 the Python doubles torch is given — may differ by, per
    entry and beyond BARS x (Em, Ev, Ep), from adam64 of the same fp32 state after ONE step (module docstring).  ref: that
    adam64 result (step = the step being taken); g, m: its inputs."""
    F = np.float32
    b1f, b2f = F(b1), F(b2)
    omb1, omb2 = float(F(1) - b1f), float(F(1) - b2f)       # the library's weights
    dl1 = abs(float(F(1.0 - b1)) - omb1) / omb1            # torch's: the fp32 rounding of the double 1 - b
    dl2 = abs(float(F(1.0 - b2)) - omb2) / omb2
    bc1_t, bc2_t = 1.0 - b1 ** step, 1.0 - b2 ** step
    bc1, bc2 = 1.0 - float(b1f) ** step, 1.0 - float(b2f) ** step
    dS = abs(bc1_t - bc1) / bc1_t
    g, m = g.detach().to(torch.float64), m.detach().to(torch.float64)
    gi = g * f32(s)
    dM = dl1 * (gi - m).abs() * omb1
    dV = dl2 * gi * gi * omb2
    S = f32(lr) / bc1
    D = ref.V.sqrt() / math.sqrt(bc2) + f32(eps)
    rel_v = torch.where(ref.V > 0, dV / ref.V, torch.zeros_like(dV))
    dD = 0.5 * (rel_v + abs(bc2_t - bc2) / bc2_t)
    dP = 1.01 * (S / D * dM + (S * ref.M / D).abs() * (dS + dD))
    return {"m": dM, "v": dV, "p": dP}


# ---- r2l_loss_finish ------------------------------------------------------------------------------------------------------------
def loss64(partials, inv_denom):
    """(mse, psnr, mse_bar, psnr_bar) as Python floats: fp64 sum of the fp32 partials (math.fsum: exact) times the fp32 inv_denom,
    -10 log10 of it, and the bars of the module docstring."""
    x = np.asarray(partials, dtype=np.float64).reshape(-1)
    if not np.isfinite(x).all():
        return float("nan"), float("nan"), float("nan"), float("nan")
    mse = math.fsum(x.tolist()) * f32(inv_denom)
    if mse == 0.0:
        return 0.0, float("inf"), 0.0, 0.0
    psnr = -10.0 * math.log10(mse)
    return mse, psnr, 2 * U * mse, (10.0 / math.log(10.0)) * (4 * U * abs(math.log(mse)) + 4 * U) + U * abs(psnr)


# ---- the fp16x2 weight streams (layout 2) -----------------------------------------------------------------------------------------
R_IN, R_W = 1008, 256
PAD_STAGES = 8
STAGE_HALVES = 8192  # 16 KiB: [split (hi, mid)][tile 8][lane 64][slot 8] fp16


def off_head_b():
    return R_IN * R_W


def off_body_w(layer):
    return R_IN * R_W + R_W + layer * (R_W * R_W + R_W)


def off_body_b(layer):
    return off_body_w(layer) + R_W * R_W


def off_tail_w(n_block):
    return off_body_w(2 * n_block)


def param_count(n_block):
    return off_tail_w(n_block) + 3 * R_W + 3


def fwd_stages(n_block):
    return 64 + 34 * n_block


def bwd_stages(n_block):
    return 34 * n_block


def split16(w):
    """numpy fp32 -> (hi, mid) fp16 bit patterns (uint16): hi = fp16(w) (round to nearest even, overflow to inf, gradual
    underflow), mid = fp16(w - hi) with the subtraction in fp32."""
    w = np.asarray(w, dtype=np.float32)
    with np.errstate(all="ignore"):
        hi = w.astype(np.float16)
        mid = (w - hi.astype(np.float32)).astype(np.float16)
    return hi.view(np.uint16), mid.view(np.uint16)


def _within():
    within = np.arange(4096)
    s, lane, tile = within & 7, (within >> 3) & 63, within >> 9
    i, h = lane & 31, lane >> 5
    return s, h, 32 * tile + i


def body_input_index(kb, s, h):
    """The input feature a stage piece's slot holds: 16 features per stage kb, lanes' halves interleaved in groups of four."""
    T, r = kb >> 1, kb & 1
    return 32 * T + 8 * (2 * r + (s >> 2)) + 4 * h + (s & 3)


def head_column(kb, s, h):
    """Column of head.weight in slot s of head stage 1 + kb (kb 0 .. 62), lane half h: value v = 8 kb + s of the half's 504 —
    the (sin, cos) pairs of 24 coordinates (8 samples x 3) frequency by frequency, then the 24 raw coordinates; a coordinate's
    21 columns are [sin 0..9 | cos 0..9 | x] in the kernels' own order of the embedding (the pack un-does it: flat columns)."""
    v = 8 * kb + s
    ci, w20 = v // 20, v % 20
    f = w20 >> 1
    trig = 21 * (3 * (8 * h + ci // 3) + ci % 3) + np.where(w20 & 1, 10 + f, f)
    e = v - 480
    raw = 21 * (3 * (8 * h + e // 3) + e % 3) + 20
    return np.where(v < 480, trig, raw)


def fwd_gather(n_block):
    """(index [stages, 4096] into the flat parameters or -1, kind [stages]): kind 0 = weight stage (hi and mid planes), 1 = head
    bias stage, 2 = body bias stage (times inv_s), 3 = zero stage.  Bias stages keep (hi, mid) in slots 0, 1 of lane half 0 of the hi
    plane only."""
    s, h, o = _within()
    n = fwd_stages(n_block)
    idx = np.full((n + PAD_STAGES, 4096), -1, dtype=np.int64)
    kind = np.full(n + PAD_STAGES, 3, dtype=np.int64)
    idx[0], kind[0] = off_head_b() + o, 1
    for g in range(1, 64):
        idx[g], kind[g] = o * R_IN + head_column(g - 1, s, h), 0
    for g in range(64, n):
        layer, r17 = (g - 64) // 17, (g - 64) % 17
        if r17 == 0:
            idx[g], kind[g] = off_body_b(layer) + o, 2
        else:
            idx[g], kind[g] = off_body_w(layer) + o * R_W + body_input_index(r17 - 1, s, h), 0
    return idx, kind


def fwd_stream_bits(flat, n_block, inv_s=1.0):
    """uint16 [stages + pad, 2, 4096]: the fp16x2 forward stream of the flat fp32 parameters (numpy) at activation scale 1 / inv_s."""
    flat = np.asarray(flat, dtype=np.float32)
    idx, kind = fwd_gather(n_block)
    s, h, _ = _within()
    out = np.zeros((idx.shape[0], 2, 4096), dtype=np.uint16)
    for g in range(idx.shape[0]):
        if kind[g] == 3:
            continue
        w = flat[idx[g]]
        if kind[g] == 2:
            w = w * np.float32(inv_s)
        hi, mid = split16(w)
        if kind[g] == 0:
            out[g, 0], out[g, 1] = hi, mid
        else:
            out[g, 0] = np.where((h == 0) & (s == 0), hi, np.where((h == 0) & (s == 1), mid, 0))
    return out


def bwd_gather(n_block):
    """index [stages + pad, 4096] or -1: the transposed stream of the dX chain.  Blocks from the last to the first, 34 stages each:
    [zero | W2^T 16 stages | zero | W1^T 16 stages]; element (output o of the TRANSPOSED product = input column of W, feature `in` =
    output row of W) = W[in][o]."""
    s, h, o = _within()
    n = bwd_stages(n_block)
    idx = np.full((n + PAD_STAGES, 4096), -1, dtype=np.int64)
    for g in range(n):
        slot, r = g // 34, g % 34
        b = n_block - 1 - slot
        if r == 0 or r == 17:
            continue
        layer, kb = (2 * b + 1, r - 1) if r < 17 else (2 * b, r - 18)
        idx[g] = off_body_w(layer) + body_input_index(kb, s, h) * R_W + o
    return idx


def bwd_stream_bits(flat, n_block):
    flat = np.asarray(flat, dtype=np.float32)
    idx = bwd_gather(n_block)
    out = np.zeros((idx.shape[0], 2, 4096), dtype=np.uint16)
    live = idx[:, 0] >= 0
    hi, mid = split16(flat[idx[live]])
    out[live, 0], out[live, 1] = hi, mid
    return out
