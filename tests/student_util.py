"""Test infrastructure: an fp64 yardstick of the student's training step that needs no knowledge of any stash layout.

The student (88-layer ResMLP) has a ReLU in front of every second layer.  A pre-activation within rounding of zero takes
either side of its ReLU depending on the fp32 summation order, and each such flip moves gradient entries by a whole ray's share:
against an arbitrary batch no reference can be sharper than that (tests/test_train_gpu.py holds 2e-3 of a tensor's max).  The
route taken here is INPUT SELECTION, decided by the fp64 forward alone and before any kernel runs: stable_rays keeps the rays
whose every ReLU input t satisfies |t| >= delta * m, m = |x| |W|^T + |b| being the size of the sum that rounding acts on.  On
those rays no mask can flip (the fp32 oracle's own pre-activation error is at most 4.7e-7 of m at every depth, delta is 10 to
20 times that), the kernels are given exactly the selected rays, and every entry of every gradient tensor is compared.

Plain torch on whatever device the tensors live on; no library call.  tests/test_student_yardstick_cpu.py checks this file
against fp64 autograd and checks the conditions the GPU tests rely on (rejected shares, margins, visibility of one ray).

The second half is the FORWARD's yardstick (forward_yardstick, forward_bars; tests/test_student_forward_gpu.py): every ray, every
entry of rgb, bars in the unit that rounding in the tail's sum acts on.  tests/test_student_forward_cpu.py checks it."""
import math

import numpy as np
import torch

from oracle import r2l_oracle as O

N_SAMPLE, NEAR, FAR = 16, 2., 6.
EMB_ERR = 8e-7  # r2l_sincos_double (csrc/r2l_common.h): absolute error of the fp16x2 forwards' encoding
PROD_ERR = 2.0 ** -21  # relative error of one fp16x2 / three-fp16-product product
POOL_MIN = 4096  # candidates examined at least, so that the rejected share is a statistic and not three coin tosses

# delta and the cap on the rejected share, by depth (shallow test nets and the real 43 blocks).  The margin check of
# tests/test_student_yardstick_cpu.py (encoding off by 8e-7, every product by 2^-21) flips no mask of a selected ray at these.
DELTA = {1: 1e-5, 3: 1e-5, 8: 1e-5, 43: 5e-6}
REJECT_CAP = {1: 0.15, 3: 0.15, 8: 0.25, 43: 0.50}


def f64(sd, device=None):
    return {k: v.detach().to(device=device if device is not None else v.device, dtype=torch.float64) for k, v in sd.items()}


def forward64(sd, emb64):
    """The student's forward (O.r2l_forward) in the dtype of its arguments, with everything the backward and the selection need:
    rgb [N,3]; ts: the ReLU inputs (head, then body.b.body.0 of every block), each [N,256]; ms: |x| |W|^T + |b| of the same
    units; xs: the block inputs x_0 .. x_nb and xms: the absolute-product magnitude of the one sum that produced each
    (x_0: m of the live units; x_b: |x_{b-1}| + |relu t| |W2|^T + |b2|); y = x_nb + x_0, the tail's input, and ym likewise."""
    nb = O.n_block_of(sd)
    lin = lambda x, name: x @ sd[name + ".weight"].T + sd[name + ".bias"]
    mag = lambda x, name: x.abs() @ sd[name + ".weight"].abs().T + sd[name + ".bias"].abs()
    ts, ms = [lin(emb64, "head.0")], [mag(emb64, "head.0")]
    x = torch.relu(ts[0])
    xs, xms = [x], [ms[0] * (ts[0] > 0)]
    for b in range(nb):
        ts.append(lin(x, "body.%d.body.0" % b))
        ms.append(mag(x, "body.%d.body.0" % b))
        xms.append(x.abs() + mag(torch.relu(ts[-1]), "body.%d.body.2" % b))
        x = lin(torch.relu(ts[-1]), "body.%d.body.2" % b) + x
        xs.append(x)
    y = x + xs[0]
    return dict(rgb=torch.sigmoid(lin(y, "tail.0")), ts=ts, ms=ms, xs=xs, xms=xms, y=y, ym=xms[-1] + xms[0])


def stable_rays(sd, emb64, delta, chunk=4096):
    """Boolean mask [N]: |t| >= delta * m at every ReLU input of the net."""
    out = []
    for lo in range(0, emb64.shape[0], chunk):
        f = forward64(sd, emb64[lo:lo + chunk])
        ok = torch.ones(f["rgb"].shape[0], dtype=torch.bool, device=emb64.device)
        for t, m in zip(f["ts"], f["ms"]):
            ok &= (t.abs() >= delta * m).all(dim=1)
        out.append(ok)
    return torch.cat(out) if out else torch.zeros(0, dtype=torch.bool, device=emb64.device)


def half_hi(x):
    """The default trio's weight-gradient operand: x scaled by a power of two (largest entry into [128, 256), well inside fp16),
    rounded to fp16 — the hi piece of the stash — and scaled back.  fp64 in, fp64 out."""
    amax = x.abs().max().item()
    if amax == 0. or not math.isfinite(amax):
        return x
    s = 2.0 ** (7 - math.floor(math.log2(amax)))
    return (x * s).half().double() / s


def backward64(sd, emb64, target64=None, drgb64=None, drop=None, round_op=None):
    """Manual backprop of loss = mean((rgb - target)^2) (or of a caller's dL/drgb) through the student: (rgb, loss, grads, mags).

    grads: every tensor of sd, weights and biases, in its order.  mags: beside each, the absolute backprop |G|^T |A| (biases:
    sum |G|), where |G| and |A| are the ABSOLUTE-PRODUCT magnitudes of the layer's output gradient and of its input: |g| |W| of
    the one sum that produced G, and forward64's m / xms for A — because that, not the cancelled value, is the size of what
    rounding acts on.  (With the cancelled values the fp32 autograd of the reference itself is off by 3e-2 of "mag": a stream entry
    x_b near zero, or a gradient that cancels, of a unit that is live for a few rays.  Absolute values through the WHOLE chain,
    as the 10-layer teacher's yardstick takes them, grow ~32x per block here and bound nothing at 43 blocks.)  The per-entry bars
    refer to it.
    drop = p: ray p's dL/dz is zeroed, the 1/N of the whole step is kept: the step with ray p left out.
    round_op: the default trio's weight-gradient operands (csrc/r2l_dw16.hip, r2l_dw_head16.hip).  Head and body take
    dW = round_op(G)^T round_op(A) and, summed from the same fragments, db = sum round_op(G); product and sum stay fp64, the
    chain that produces G is exact, and the tail (csrc/r2l_bwd2.hip: fp32 operands) is left alone.  Pass half_hi."""
    nb = O.n_block_of(sd)
    f = forward64(sd, emb64)
    rgb, ts, ms, xs, xms, y = f["rgb"], f["ts"], f["ms"], f["xs"], f["xms"], f["y"]
    n = emb64.shape[0]
    if drgb64 is None:
        drgb64 = (2.0 / (3.0 * n)) * (rgb - target64)
        drgb_abs = (2.0 / (3.0 * n)) * (rgb + target64.abs())  # rgb - target cancels where the net is right
        loss = ((rgb - target64)**2).mean()
    else:
        drgb_abs, loss = drgb64.abs(), None
    dz, dz_abs = drgb64 * rgb * (1.0 - rgb), drgb_abs * rgb * (1.0 - rgb)
    if drop is not None:
        dz, dz_abs = dz.clone(), dz_abs.clone()
        dz[drop] = 0.
        dz_abs[drop] = 0.
    g, mg = {}, {}
    rnd = round_op if round_op is not None else (lambda t: t)

    def wgrad(name, G, Gabs, A, Aabs, rounded=True):
        Gr, Ar = (rnd(G), rnd(A)) if rounded else (G, A)
        g[name + ".weight"], g[name + ".bias"] = Gr.T @ Ar, Gr.sum(0)
        mg[name + ".weight"], mg[name + ".bias"] = Gabs.T @ Aabs, Gabs.sum(0)

    wgrad("tail.0", dz, dz_abs, y, f["ym"], rounded=False)
    dy = dz @ sd["tail.0.weight"]
    dy_abs = dz_abs @ sd["tail.0.weight"].abs()
    gx, gx_abs = dy, dy_abs
    for b in range(nb - 1, -1, -1):
        t = ts[b + 1]
        w2, w0 = sd["body.%d.body.2.weight" % b], sd["body.%d.body.0.weight" % b]
        wgrad("body.%d.body.2" % b, gx, gx_abs, torch.relu(t), ms[b + 1] * (t > 0))
        gt, gt_abs = (gx @ w2) * (t > 0), (gx.abs() @ w2.abs()) * (t > 0)
        wgrad("body.%d.body.0" % b, gt, gt_abs, xs[b], xms[b])
        gx, gx_abs = gx + gt @ w0, gx.abs() + gt.abs() @ w0.abs()
    wgrad("head.0", (gx + dy) * (ts[0] > 0), (gx_abs + dy_abs) * (ts[0] > 0), emb64, emb64.abs())
    return rgb, loss, {k: g[k] for k in sd}, {k: mg[k] for k in sd}


# ---- inputs: rays, the reference encoding and the selection ---------------------------------------------------------------
def candidate_rays(n, seed):
    """n candidate rays on the CPU (fp32), the distribution of tests/test_train_gpu.py's bit-reproducibility test: origins around
    (0, 0, 4), unit directions and stratified-jitter uniforms.  The targets are uniform over [0, 0.4) and [0.6, 1): a default-init
    net renders mid-grey, and a ray whose target happens to be its rendering carries no gradient — no gradient test can see such
    a ray go missing, whatever its bar.  Every ray of these batches has an error of at least ~0.1 in every channel."""
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(n, 3, generator=g) * 0.3 + torch.tensor([0., 0., 4.])
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    r = torch.rand(n, 3, generator=g)
    tgt = 0.8 * r + 0.2 * (r >= 0.5)
    u = torch.rand(n, N_SAMPLE, generator=g)
    return o, d, tgt, u


def reference_encoding(o, d, u, perturb, device="cpu", through_fp32=False):
    """The rays path's reference encoding: the points from O.sample_train in fp32 (the library reproduces that arithmetic bit
    for bit), then the TRUE sin / cos of those fp32 arguments, O.positional_embed in fp64.  through_fp32: that encoding rounded to
    fp32 and promoted again — what a caller of the pre-embedded path hands over, identical to the bit on both sides."""
    pts = O.sample_train(o, d, O.z_vals(N_SAMPLE, NEAR, FAR), perturb, u if perturb > 0 else None)
    with torch.device(device):  # (the oracle creates its frequency table on the default device)
        emb = O.positional_embed(pts.to(device).double(), 10)
    return emb.float().double() if through_fp32 else emb


def select_case(sd, n, perturb, seed, device="cpu", through_fp32=False, delta=None):
    """N mask-stable rays of a seeded candidate pool, in pool order.  Returns dict(o, d, tgt, u: the N rays on the CPU, fp32;
    emb64 [N,1008] on `device`; rejected: share of the whole pool that was rejected; examined: candidates gone through until N
    were found).  The pool holds max(POOL_MIN, 3 N) candidates, all of which are classified, so the share asserted against the
    cap is the same statistic at N = 1 as at N = 16385."""
    nb = O.n_block_of(sd)
    delta = DELTA[nb] if delta is None else delta
    pool = max(POOL_MIN, 3 * n)
    o, d, tgt, u = candidate_rays(pool, seed)
    sd64 = f64(sd, device)
    ok = []
    for lo in range(0, pool, 8192):
        s = slice(lo, lo + 8192)
        ok.append(stable_rays(sd64, reference_encoding(o[s], d[s], u[s], perturb, device, through_fp32), delta))
    ok = torch.cat(ok).cpu()
    idx = torch.nonzero(ok).flatten()
    assert idx.numel() >= n, "pool of %d candidates holds only %d stable rays, %d wanted" % (pool, idx.numel(), n)
    idx = idx[:n]
    o, d, tgt, u = o[idx].contiguous(), d[idx].contiguous(), tgt[idx].contiguous(), u[idx].contiguous()
    return dict(o=o, d=d, tgt=tgt, u=u, emb64=reference_encoding(o, d, u, perturb, device, through_fp32),
                rejected=1.0 - ok.double().mean().item(), examined=int(idx[-1].item()) + 1, delta=delta)


# ---- bars -------------------------------------------------------------------------------------------------------------------
C_BWD = 3e-6  # per entry: |got - want| <= C_BWD * mag + floor   (tests/test_teacher_backward_gpu.py: same arithmetic, same kind of yardstick)
NREL_BWD = 1e-5  # per tensor, norm-relative


def nrel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300)).item()


def entry_violations(got, want, mags, c=C_BWD):
    """{tensor: number of entries with |got - want| > c * mag + floor}; the floor only keeps underflow out."""
    out = {}
    for k in want:
        floor = 1e-12 * mags[k].max().item() + 1e-30
        out[k] = int(((got[k].double() - want[k]).abs() > c * mags[k] + floor).sum().item())
    return out


def worst_ratio(got, want, mags):
    """largest |got - want| / mag over the entries whose mag is not negligible, and its tensor."""
    r = (0., None)
    for k in want:
        m = mags[k]
        ok = m > 1e-12 * m.max()
        if ok.any():
            r = max(r, (((got[k].double() - want[k]).abs()[ok] / m[ok]).max().item(), k))
    return r


def split_flat(flat, sd):
    out, off = {}, 0
    for k, v in sd.items():
        out[k] = flat[off:off + v.numel()].view(v.shape)
        off += v.numel()
    return out


# ---- the table of shapes (shared by the CPU conditions and the GPU tests) -------------------------------------------------
# Where a step can be cut, gone through source by source (ray counts; every unit gets an N on both sides of it, or of a multiple):
#   2      r2l_dw_head.hip head weight gradient: a k-step pairs rays 2s, 2s + 1; rays per slice rounded up to even
#   16     coop16 tiles (r2l_coop16.hip C16_RAYS); k-step of r2l_dw16.hip and r2l_dw_head16.hip
#   32     R2L_TILE_RAYS: one wave's tile in every other chain, the cooperative fp16 chains' tile, the stash's padding unit
#   64     DW_CHUNK, the body weight gradients' work unit (r2l_dw.h); two 32-ray tiles of one cooperative workgroup (coopf2)
#   128    four one-wave tiles of a workgroup (r2l_fwd2 / r2l_bwd2 / r2l_forward, main tiling)
#   256    rays per slice of the head weight gradient below 64 slices (one slice up to 256 rays, two from 257)
#   512    workgroups of the tail gradient, one ray each up to 512 rays, two from 513 (r2l_dw_tail_kernel, DW_TAIL_SLAB)
#   6144   the fp16 trio's body weight gradient: two workgroups per layer up to here, the 11/16 grid above
#   16384  DW_MAX_WGS = 256 workgroups x 64 rays: more work units per layer than workgroups; 64 head slices x 256 rays
#          (257 -> 258 per slice above); R2L_COOPF_MAX_RAYS, where the AUTO tiling leaves the cooperative chains
N_AT_3 = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 257, 511, 513, 1000, 4097, 6145, 16385)
SHAPES = [(3, n) for n in N_AT_3] + [(1, 33), (1, 1000), (8, 33), (8, 1000), (43, 65), (43, 1000), (43, 4097)]
SELF_CHECK_SHAPES = [(3, 65), (3, 1000), (3, 4097), (43, 1000)]
NET_SEED = 3


def case_seed(nb, n, perturb):
    return nb * 1000003 + n * 16 + int(perturb > 0)


def probe_rays(n):
    """The rays a cut step would lose first: 0, either side of the first 32-ray tile edge, the last ray of the last full 64-ray
    work unit, the last ray."""
    return sorted({p for p in (0, 31, 32, (n // 64) * 64 - 1, n - 1) if 0 <= p < n})


# ---- the forward: yardstick, unit and bars (tests/test_student_forward_cpu.py, tests/test_student_forward_gpu.py) ----------
# ReLU is continuous: the forward needs no mask-stable rays.  Every candidate ray is used, every entry of rgb compared.
#
# unit[p,c] = rgb64 (1 - rgb64) mz, mz = ym |W_tail|^T + |b_tail|: the size of the sum that rounding acts on in the tail's
# pre-activation z, carried through the sigmoid to first order.  Every bar is in this unit, plus 2^-24 absolute for the final
# rounding of an rgb below 1.
#
# C_FWD: the fp32 reference's own distance (forward32 below: O.r2l_forward's operations in fp32 with a pinned summation order, on
# the fp32-rounded reference encoding) from the fp64 forward in that unit, times 4 — the margin tests/test_render_stages_gpu.py
# gives a kernel over torch's fp32 for a different summation order.  Worst |ref32 - rgb64| / unit over whole candidate pools
# (POOL_MIN = 4096 rays, perturb 0 and 1), measured by tests/test_student_forward_cpu.py, which holds the worst between C_FWD / 8
# and C_FWD / 4:
#   n_block   worst (perturb 0 / 1)      rms (perturb 0 / 1)        torch's own fp32 on one CPU: worst, rms
#   1         2.402e-8 / 2.677e-8        4.54e-9 / 4.54e-9          2.89e-8 / 2.96e-8, 4.73e-9 / 4.74e-9
#   3         1.970e-8 / 2.088e-8        4.20e-9 / 4.15e-9          2.15e-8 / 1.99e-8, 3.97e-9 / 3.98e-9
#   8         1.964e-8 / 1.715e-8        4.16e-9 / 4.19e-9          2.19e-8 / 1.96e-8, 4.17e-9 / 4.13e-9
#   43        3.057e-8 / 2.944e-8        6.73e-9 / 6.73e-9          3.36e-8 / 3.22e-8, 7.42e-9 / 7.49e-9
# 4 x 3.057e-8 = 1.223e-7, written 1.25e-7 (a rounding that falls the other way in one fp64 sum moves an entry by ~3e-10):
C_FWD = 1.25e-7
RGB_FLOOR = 2.0 ** -24
EMB_EXACT = 1.5 * 2.0 ** -24  # r2l_sincos: 1.5 ulp of values <= 1 (tests/test_sincos_gpu.py ULP_BAR); EMB_ERR after one angle doubling
FWD_CHUNK = 4096  # forward64 keeps four [N,256] fp64 tensors per block
FWD_DEPTHS = (1, 3, 8, 43)


def pieces(x, dtype, n):
    """x = p_1 + ... + p_n + (dropped): p_1 = dtype(x), p_2 = dtype(x - p_1), ..., each promoted again."""
    out, r = [], x
    for _ in range(n):
        out.append(r.to(dtype).to(x.dtype))
        r = r - out[-1]
    return out


def forward16x2(sd, emb64):
    """The operand model of the fp16x2 chains (r2l_f2.h; r2l_fwd2.hip, r2l_coopf_fwd.hip): the forward in fp64 with both operands
    of every head and body product written hi + mid in fp16 and the product taken as the terms the kernels keep, hi*hi + hi*mid +
    mid*hi.  A bias is the sum of its two pieces (its stage multiplies them by ones).  Accumulation, residual adds and ReLU stay
    fp64.  The tail is left alone: the kernels form it on the VALU from the fp32 tail weights and the fp32 accumulators of
    y = x_n + x_0.  Returns rgb [N,3]."""
    def lin(x, name):
        (xh, xm), (wh, wm) = pieces(x, torch.float16, 2), pieces(sd[name + ".weight"], torch.float16, 2)
        return xh @ (wh + wm).T + xm @ wh.T + sum(pieces(sd[name + ".bias"], torch.float16, 2))
    x0 = torch.relu(lin(emb64, "head.0"))
    x = x0
    for b in range(O.n_block_of(sd)):
        x = lin(torch.relu(lin(x, "body.%d.body.0" % b)), "body.%d.body.2" % b) + x
    return torch.sigmoid((x + x0) @ sd["tail.0.weight"].T + sd["tail.0.bias"])


def tail_jacobian_rows(sd, emb64):
    """[dz_c / d emb for c = 0, 1, 2], each [N,1008]: z the tail's pre-activation.  Three fp64 autograd passes, each on the sum
    over the rays of one channel of z (the rays do not interact: row p of the gradient is ray p's Jacobian row)."""
    e = emb64.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        h0 = torch.relu(e @ sd["head.0.weight"].T + sd["head.0.bias"])
        x = h0
        for b in range(O.n_block_of(sd)):
            t = torch.relu(x @ sd["body.%d.body.0.weight" % b].T + sd["body.%d.body.0.bias" % b])
            x = t @ sd["body.%d.body.2.weight" % b].T + sd["body.%d.body.2.bias" % b] + x
        z = (x + h0) @ sd["tail.0.weight"].T + sd["tail.0.bias"]
        return [torch.autograd.grad(z[:, c].sum(), e, retain_graph=(c < 2))[0] for c in range(3)]


def tail_jacobian_norms(sd, emb64):
    """(||dz_c / d emb_p||_1, ||.||_2), each [N,3]."""
    rows = tail_jacobian_rows(sd, emb64)
    return torch.stack([r.abs().sum(1) for r in rows], 1), torch.stack([r.norm(dim=1) for r in rows], 1)


REF_KSTEP = 2


def linear32(x32, w, b, kstep=REF_KSTEP, slab=32):
    """F.linear in fp32 with a PINNED summation order: an fp32 accumulator that starts at the bias and takes the products `kstep`
    at a time in the order of k, acc = fp32(acc + sum of kstep products), the inner sum formed in fp64.  The same on any device."""
    n, k = x32.shape
    assert k % kstep == 0 and x32.dtype == torch.float32
    xs = x32.double().view(n, k // kstep, kstep).transpose(0, 1)  # [steps, n, kstep]
    ws = w.double().view(-1, k // kstep, kstep).permute(1, 2, 0)  # [steps, kstep, out]
    acc = b.float().expand(n, -1).contiguous()
    tmp = torch.empty(n, acc.shape[1], dtype=torch.float64, device=acc.device)
    for lo in range(0, k // kstep, slab):
        for part in torch.bmm(xs[lo:lo + slab], ws[lo:lo + slab]):
            torch.add(acc, part, out=tmp)  # (fp32 + fp64 -> fp64)
            acc.copy_(tmp)
    return acc


def sigmoid32(z32):
    """1 / (1 + exp(-z)) in fp32, three operations, each correctly rounded (formed in fp64, rounded to fp32)."""
    e = torch.exp(-z32.double()).float()
    d = (1.0 + e.double()).float()
    return (1.0 / d.double()).float()


def forward32(sd, emb32, chunk=4096):
    """THE fp32 reference of the forward tests: O.r2l_forward's operations in fp32, each rounded on its own, every dot product by
    linear32 and the sigmoid by sigmoid32 — pinned, so that the reference's distance from fp64, which sets the bars, does not
    depend on the machine the test runs on.  torch's own fp32 (O.r2l_forward on fp32 tensors) does: its sgemm sums in blocks whose
    size follows the CPU, and at 43 blocks its rms distance was 7.5e-9 unit on one machine and 5.1e-9 on another, on the same rays
    — which moved one and the same kernel output from 0.74 to 1.05 of a bar of 4 times that rms.  REF_KSTEP = 2 (two products per
    rounding of the accumulator) reproduces the first machine, where the figures that shaped these bars were taken: rms 4.47 /
    4.05 / 4.15 / 6.75e-9 unit at 1 / 3 / 8 / 43 blocks against torch's 4.69 / 3.84 / 4.14 / 7.50e-9 there (1024 rays), under it
    where it matters.  (REF_KSTEP = 4 gives 5.1e-9 at 43 blocks.)  tests/test_student_forward_cpu.py holds torch's fp32, whatever
    the CPU, to the bars as a subject."""
    out = []
    for lo in range(0, emb32.shape[0], chunk):
        lin = lambda x, name: linear32(x, sd[name + ".weight"], sd[name + ".bias"])
        h0 = torch.relu(lin(emb32[lo:lo + chunk].float(), "head.0"))
        x = h0
        for b in range(O.n_block_of(sd)):
            x = lin(torch.relu(lin(x, "body.%d.body.0" % b)), "body.%d.body.2" % b) + x
        out.append(sigmoid32(lin(x + h0, "tail.0")))
    return torch.cat(out) if out else torch.zeros(0, 3)


def forward_yardstick(sd, emb64, model=False, jacobian=True, chunk=FWD_CHUNK):
    """Everything the forward bars need of one case, in chunks of `chunk` rays.  sd: the fp32 state dict; emb64 [N,1008] fp64 on the
    device the fp64 work is to run on.  Returns fp64 tensors on that device, each [N,3]:
      rgb     the fp64 forward (forward64);
      unit    rgb (1 - rgb) mz;
      jac1, jac2   rgb (1 - rgb) ||dz_c / d emb_p|| in L1 and L2: times the encoder's error EMB, the encoder's allowance as a
              first-order bound, and its size under independent errors;
      e_ref   |ref32 - rgb|, ref32 = forward32 on the encoding rounded to fp32: the fp32 reference's own distance.  Never a kernel's;
      e_model (model=True) |forward16x2 - rgb|: what the fp16x2 operands cost."""
    dev = emb64.device
    sd64 = f64(sd, dev)
    keys = ["rgb", "unit", "jac1", "jac2", "e_ref"] + (["e_model"] if model else [])
    out = {k: [] for k in keys}
    for lo in range(0, emb64.shape[0], chunk):
        e = emb64[lo:lo + chunk]
        f = forward64(sd64, e)
        rgb = f["rgb"]
        s = rgb * (1.0 - rgb)
        out["rgb"].append(rgb)
        out["unit"].append(s * (f["ym"] @ sd64["tail.0.weight"].abs().T + sd64["tail.0.bias"].abs()))
        del f
        j1, j2 = tail_jacobian_norms(sd64, e) if jacobian else (torch.zeros_like(s), torch.zeros_like(s))
        out["jac1"].append(s * j1)
        out["jac2"].append(s * j2)
        out["e_ref"].append((forward32(sd64, e.float()).double() - rgb).abs())
        if model:
            out["e_model"].append((forward16x2(sd64, e) - rgb).abs())
    return {k: torch.cat(v) if v else torch.zeros(0, 3, dtype=torch.float64, device=dev) for k, v in out.items()}


def rms(t):
    return t.double().pow(2).mean().sqrt().item()


def forward_bars(Y, emb_err, fp16x2=False):
    """(per-entry bar [N,3], per-case rms bar in units) of a family group.
    exact families:  |got - rgb64| <= C_FWD unit + EMB jac1 + 2^-24;  rms((got - rgb64) / unit) <= 4 rms(e_ref / unit) + EMB
    rms(jac2 / unit);  fp16x2 families: the same plus 3 e_model per entry and 3 rms(e_model / unit) per case — the factor the
    backward test gives its fp16 operand model, which leaves out the dropped mid*mid terms and the fp32 accumulation."""
    entry = C_FWD * Y["unit"] + emb_err * Y["jac1"] + RGB_FLOOR
    case = 4.0 * rms(Y["e_ref"] / Y["unit"]) + emb_err * rms(Y["jac2"] / Y["unit"])
    if fp16x2:
        entry = entry + 3.0 * Y["e_model"]
        case = case + 3.0 * rms(Y["e_model"] / Y["unit"])
    return entry, case


RMS_MIN_RAYS = 1000  # the per-case statistic is asserted from here on


def forward_check(got, Y, emb_err, fp16x2=False):
    """got [N,3] against the yardstick Y under the bars of a family group: dict(bad: bool [N], rays with an entry beyond its bar;
    ratio: [N] largest |got - rgb64| / bar of each ray; worst: the largest of all; rms, rms_bar: the per-case statistic and its
    bar, in units)."""
    entry, case = forward_bars(Y, emb_err, fp16x2)
    err = (got.double().to(Y["rgb"].device) - Y["rgb"]).abs()
    ratio = err / entry
    return dict(bad=(ratio > 1.0).any(dim=1), worst=ratio.max().item() if ratio.numel() else 0., ratio=ratio.max(dim=1).values,
                rms=rms(err / Y["unit"]), rms_bar=case)


def pose_points32(c2w, H, W, focal, z):
    """The sample points of a frame as the pose kernels form them (the POSE branch of r2l_fwd2.hip, r2l_fwd3.hip, r2l_forward.hip,
    r2l_coopf_fwd.hip and r2l_coop16.hip, one text in five files, built with -ffp-contract=off), restated in numpy fp32, every
    operation rounded on its own:  pixel pix -> row pj = pix / W, column pi = pix % W;  dx = (pi - W * 0.5) / focal,
    dy = -((pj - H * 0.5) / focal);  d_k = (dx c[k][0] + dy c[k][1]) + (-1) c[k][2],  o_k = c[k][3];  point = o_k + d_k z_s.
    c2w [3,4], z [S]; returns fp32 [H*W, 3*S], sample-major like O.sample_test."""
    f = np.float32
    c = np.asarray(c2w, dtype=f)[:3, :4]
    z = np.asarray(z, dtype=f)
    pix = np.arange(H * W)
    dx = ((pix % W).astype(f) - f(W) * f(0.5)) / f(focal)
    dy = -(((pix // W).astype(f) - f(H) * f(0.5)) / f(focal))
    d = np.stack([(dx * c[k, 0] + dy * c[k, 1]) + f(-1.0) * c[k, 2] for k in range(3)], 1)  # [N,3]
    pts = c[None, None, :, 3] + d[:, None, :] * z[None, :, None]
    assert pts.dtype == f
    return pts.reshape(H * W, -1)


def encode64(pts32, device="cpu", through_fp32=False):
    """The true sin / cos (fp64) of fp32 points [N,48] (a torch tensor)."""
    with torch.device(device):
        emb = O.positional_embed(pts32.to(device).double(), 10)
    return emb.float().double() if through_fp32 else emb


FWD_N_AT_3 = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1000, 4097, 16385)
FWD_SHAPES = [(3, n) for n in FWD_N_AT_3] + [(1, 33), (1, 1000), (43, 65), (43, 1000), (43, 4097)]
FWD_SELF_CHECK_SHAPES = [(3, 65), (43, 1000)]
MUTANT_RAY, MUTANT_COL = 31, 1007  # mutant (c): one feature of one ray zeroed — the last column, the last sample's z coordinate itself


def splice_ray(Y, p, Y_p):
    """Y with ray p's rows replaced by the one-ray yardstick Y_p (the rays do not interact)."""
    out = {k: v.clone() for k, v in Y.items()}
    for k in out:
        out[k][p] = Y_p[k][0]
    return out


def mutant_c(Y, sd, emb_row, model=False):
    """The yardstick of mutant (c): ray MUTANT_RAY's feature MUTANT_COL zeroed, every other ray as it was.  emb_row [1,1008]: that
    ray's encoding."""
    e = emb_row.clone()
    e[0, MUTANT_COL] = 0.
    return splice_ray(Y, MUTANT_RAY, forward_yardstick(sd, e, model=model))


def forward_inputs(n, perturb, seed, device="cpu", through_fp32=False):
    """The first n candidate rays of a seeded pool, all of them: (o, d, u on the CPU, fp32; emb64 [n,1008] on device)."""
    o, d, _, u = candidate_rays(n, seed)
    return o, d, u, reference_encoding(o, d, u, perturb, device, through_fp32)
