"""The optimizer stage on the GPU, per entry against fp64 (tests/optim_util.py): r2l_adam_step / _guarded / _packed, the fp16x2
re-pack, r2l_loss_finish, and the trainers' adam() with the state dict they hand to torch.optim.Adam.  Everything goes through the C
ABI on torch-owned buffers.  Bars are the derived ones of tests/optim_util.py; every test prints the fraction of each bar it
measured (pytest -s; profiles/optimizer_yardstick.txt quotes them)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import r2l_oracle as O
from tests import optim_util as OU

pytestmark = pytest.mark.gpu

GRID = 2048 * 256  # threads of r2l_adam_kernel's launch: one grid-stride turn
SIZES = [1, 255, 257, GRID - 1, GRID + 1, 3 * GRID + 77]
SENTINEL = 12345.678


@pytest.fixture(scope="module")
def lib():
    from r2l_amd import _lib
    return _lib.load()


def ptr(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + 4 * off)


def stream():
    from r2l_amd.engine import _stream
    return _stream()


def check(code, what):
    from r2l_amd import _lib
    _lib.check(code, what)


_CACHE = {}


def device_inputs(setting):
    """(p, g, m, v) fp32 on the device for a setting, SIZES[-1] entries (the last setting asked for is kept: tests slice it)."""
    if _CACHE.get("name") != setting[0]:
        if "base" not in _CACHE:
            _CACHE["base"] = OU.adam_inputs(SIZES[-1], 0)
        _CACHE["name"] = setting[0]
        _CACHE["dev"] = [torch.from_numpy(a).cuda() for a in OU.for_setting(_CACHE["base"], setting)]
    return _CACHE["dev"]


def fenced(t):
    """A copy of t with one sentinel float in front and one behind; the kernels get the address of element 1."""
    buf = torch.full((t.numel() + 2,), SENTINEL, dtype=torch.float32, device=t.device)
    buf[1:-1] = t
    return buf


def bits(t):
    return t.view(torch.int32)


def run_adam(lib, arrs, setting, guard=None, guarded=False):
    """r2l_adam_step (or _guarded) on fenced copies -> the four buffers (fences included)."""
    _, step, s, b1, b2, eps, lr = setting
    bufs = [fenced(a) for a in arrs]
    n = arrs[0].numel()
    args = [ptr(b, 1) for b in bufs] + [n, lr, b1, b2, eps, step, s]
    if guarded:
        check(lib.r2l_adam_step_guarded(*args, ptr(guard) if guard is not None else None, stream()), "r2l_adam_step_guarded")
    else:
        check(lib.r2l_adam_step(*args, stream()), "r2l_adam_step")
    return bufs


def fences_intact(bufs):
    want = torch.tensor(SENTINEL, dtype=torch.float32).view(torch.int32).item()
    return all(bits(b)[0].item() == want and bits(b)[-1].item() == want for b in bufs)


def assert_bars(fr, what):
    print("YARDSTICK gpu %s: m %.3f Em  v %.3f Ev  p %.3f Ep" % (what, fr["m"], fr["v"], fr["p"]))
    for k in fr:
        assert fr[k] <= OU.BARS[k], (what, k, fr)


# ---- r2l_adam_step per entry ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("setting", OU.SETTINGS, ids=OU.SETTING_IDS)
def test_adam_step_per_entry(lib, setting, n):
    """Seven settings (steps 1 .. 2^31 - 1, grad_scale 1, 1/8, 1/3, 2^-12, betas (0.5, 0.9) with eps 1e-3) x sizes around the
    grid-stride turn and a ragged tail: p', m', v' of every entry within 8 Ep, 4 Em, 6 Ev of adam64; the gradient and the float
    on either side of every buffer untouched (the buffers start 4 bytes off torch's alignment)."""
    _, step, s, b1, b2, eps, lr = setting
    arrs = [a[:n] for a in device_inputs(setting)]
    bufs = run_adam(lib, arrs, setting)
    ref = OU.adam64(*arrs, lr, b1, b2, eps, step, s)
    p1, g1, m1, v1 = [b[1:-1] for b in bufs]
    assert fences_intact(bufs) and torch.equal(bits(g1), bits(arrs[1]))
    assert torch.isfinite(ref.P).all()
    assert_bars(OU.fractions(p1, m1, v1, ref), "adam_step %s n=%d" % (setting[0], n))


def test_adam_step_nonfinite_gradients(lib):
    """+-inf / NaN gradients make p, m, v non-finite in exactly the entries where adam64's are; the neighbours stay within the bars."""
    setting = OU.SETTINGS[2]
    _, step, s, b1, b2, eps, lr = setting
    n = 4096
    arrs = [a[:n].clone() for a in device_inputs(setting)]
    bad = {0: math.inf, 10: math.inf, 11: -math.inf, 12: math.nan, 255: -math.inf, 256: math.nan, 1000: math.inf, n - 1: math.nan}
    for i, x in bad.items():
        arrs[1][i] = x
    bufs = run_adam(lib, arrs, setting)
    ref = OU.adam64(*arrs, lr, b1, b2, eps, step, s)
    p1, _, m1, v1 = [b[1:-1] for b in bufs]
    assert fences_intact(bufs)
    assert OU.nonfinite_agree(p1, m1, v1, ref)
    idx = torch.tensor(sorted(bad), device="cuda")
    assert not torch.isfinite(p1[idx]).any() and not torch.isfinite(m1[idx]).any() and not torch.isfinite(v1[idx]).any()
    assert torch.isfinite(p1).sum().item() == n - len(bad)
    for got, want in ((p1, ref.P), (m1, ref.M), (v1, ref.V)):
        assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert_bars(OU.fractions(p1, m1, v1, ref), "adam_step non-finite gradients, the other entries")


def test_adam_step_eps_zero(lib):
    """eps = 0: an entry with g = v = 0 divides by zero — NaN (m = 0) or +-inf (m != 0) exactly where the reference says."""
    setting = ("eps0", 7, 1.0, 0.9, 0.999, 0.0, 5e-4)
    _, step, s, b1, b2, eps, lr = setting
    n = 1024
    arrs = [a[:n].clone() for a in device_inputs(OU.SETTINGS[0])]
    dead = torch.arange(0, n, 7, device="cuda")
    arrs[1][dead] = 0.0
    arrs[3][dead] = 0.0
    arrs[2][dead[::2]] = 0.0
    arrs[2][dead[1::2]] = torch.where(arrs[2][dead[1::2]] == 0, torch.ones_like(arrs[2][dead[1::2]]), arrs[2][dead[1::2]])
    bufs = run_adam(lib, arrs, setting)
    ref = OU.adam64(*arrs, lr, b1, b2, eps, step, s)
    p1, _, m1, v1 = [b[1:-1] for b in bufs]
    assert torch.isnan(ref.P[dead[::2]]).all() and torch.isinf(ref.P[dead[1::2]]).all()
    assert OU.nonfinite_agree(p1, m1, v1, ref)
    assert torch.equal(torch.isnan(p1), torch.isnan(ref.P))
    inf = torch.isinf(ref.P)
    assert torch.equal(p1[inf].double(), ref.P[inf])  # the sign of the infinity
    assert_bars(OU.fractions(p1, m1, v1, ref), "adam_step eps = 0, the finite entries")


# ---- write-back and step-dependent constants -------------------------------------------------------------------------------------------
def test_adam_200_consecutive_steps(lib):
    """200 calls in place, steps 1 .. 200, warm-up learning rates, a gradient that changes with the step: after every call the state
    is within the bars of adam64 applied to the kernel's own previous state (a moment that is not written back, or a bias
    correction that goes wrong after step 3, shows at the next call).  Then one call each at steps 1e5 and 2^31 - 1."""
    from r2l_amd.train_step import lr_schedule
    n, b1, b2, eps = 4096, 0.9, 0.999, 1e-8
    gen = torch.Generator(device="cuda").manual_seed(11)
    p = (torch.rand(n, device="cuda", generator=gen) * 2 - 1) * 0.5
    m = torch.zeros(n, device="cuda")
    v = torch.zeros(n, device="cuda")
    amp = 10.0 ** (torch.rand(n, device="cuda", generator=gen) * 8 - 6)
    phase = torch.rand(n, device="cuda", generator=gen) * 6.2831853
    freq = 0.02 + 0.2 * torch.rand(n, device="cuda", generator=gen)
    worst = {"m": 0.0, "v": 0.0, "p": 0.0}
    steps = list(range(1, 201)) + [100000, OU.INT_MAX]
    for step in steps:
        g = amp * (torch.sin(freq * min(step, 1000) + phase) + 0.3 * torch.randn(n, device="cuda", generator=gen))
        lr = lr_schedule(min(step, 100000), 5e-4, 500, "0.0001,200")
        prev = (p.clone(), m.clone(), v.clone())
        check(lib.r2l_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), n, lr, b1, b2, eps, step, 1.0, stream()), "r2l_adam_step")
        ref = OU.adam64(prev[0], g, prev[1], prev[2], lr, b1, b2, eps, step, 1.0)
        fr = OU.fractions(p, m, v, ref)
        for k in fr:
            worst[k] = max(worst[k], fr[k])
            assert fr[k] <= OU.BARS[k], (step, k, fr)
        assert not torch.equal(m, prev[1]) and not torch.equal(v, prev[2]) and not torch.equal(p, prev[0])
    assert (v > 0).all() and torch.isfinite(p).all()
    assert_bars(worst, "adam_step 200 consecutive steps + 1e5 + 2^31-1")


# ---- r2l_adam_step_guarded ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [257, GRID + 1])
def test_adam_guarded(lib, n):
    setting = OU.SETTINGS[3]
    arrs = [a[:n] for a in device_inputs(setting)]
    plain = run_adam(lib, arrs, setting)
    for word, moves in ((None, True), (0, True), (1, False), (-2 ** 31, False)):
        guard = None if word is None else torch.tensor([word], dtype=torch.int32, device="cuda")
        out = run_adam(lib, arrs, setting, guard=guard, guarded=True)
        assert fences_intact(out)
        for k, (a, b, c) in enumerate(zip(out, plain, arrs)):
            want = b[1:-1] if moves else c
            assert torch.equal(bits(a[1:-1]), bits(want)), (word, k)
        if guard is not None:
            assert guard.item() == word
    assert not torch.equal(plain[0][1:-1], arrs[0])


# ---- r2l_adam_step_packed ------------------------------------------------------------------------------------------------------------------
PLANTED = [0.0, -0.0, 65504.0, 7e4, 1e-8]
PACK_SETTING = ("packed", 1000, 1.0 / 8, 0.9, 0.999, 1e-8, 4.9e-4)


def stream_region(lib, buf, n_block, fwd):
    """(int16 view of the fp16x2 stages of a stream buffer, offset of its 16 status words in floats)."""
    fn = lib.r2l_forward_status_words if fwd else lib.r2l_backward_status_words
    addr = ctypes.cast(fn(ptr(buf), n_block), ctypes.c_void_p).value
    status = (addr - buf.data_ptr()) // 4
    stages = (OU.fwd_stages(n_block) if fwd else OU.bwd_stages(n_block)) + OU.PAD_STAGES
    assert status + 16 == buf.numel() and status - stages * 4096 >= 0
    return buf[status - stages * 4096:status].view(torch.int16), status


def region_bits(lib, buf, n_block, fwd):
    r, _ = stream_region(lib, buf, n_block, fwd)
    return r.cpu().numpy().view(np.uint16).reshape(-1, 2, 4096)


def packed_state(lib, n_block, seed):
    """Parameters |w| <= 4 with the planted body weights, wide-range gradients, non-zero moments, both streams packed once.
    The planted entries get g = m = 0 (v > 0): the update leaves them as they are, bit for bit."""
    n = OU.param_count(n_block)
    assert n == lib.r2l_param_count(n_block)
    rng = np.random.default_rng(seed)
    base = [np.resize(a, n) for a in OU.adam_inputs(min(n, SIZES[-1]), seed)]
    base[0] = rng.uniform(-4, 4, n).astype(np.float32)
    p, g, m, v = OU.for_setting(base, PACK_SETTING)
    planted = []
    for layer in range(2 * n_block):
        for j, w in enumerate(PLANTED):
            # spread over tiles, rows and both 16-column halves of a stage
            at = OU.off_body_w(layer) + (37 * j + 3 * layer) % 256 * 256 + (53 * j + 11 * layer + 16 * (j & 1)) % 256
            p[at], g[at], m[at], v[at] = w, 0.0, 0.0, 1.0
            planted.append(at)
    t = [torch.from_numpy(a).cuda() for a in (p, g, m, v)]
    fwd = torch.zeros(lib.r2l_fwd_stream_floats(n_block), dtype=torch.float32, device="cuda")
    bwd = torch.zeros(lib.r2l_bwd_stream_floats(n_block), dtype=torch.float32, device="cuda")
    pack_both(lib, t[0], n_block, fwd, bwd)
    return t, fwd, bwd, planted


def pack_both(lib, p, n_block, fwd, bwd):
    check(lib.r2l_pack_forward_layout(ptr(p), n_block, ptr(fwd), 2, stream()), "r2l_pack_forward_layout")
    check(lib.r2l_pack_backward_layout(ptr(p), n_block, ptr(bwd), 2, stream()), "r2l_pack_backward_layout")


def packed_call(lib, t, n_block, fwd, bwd, guard):
    _, step, s, b1, b2, eps, lr = PACK_SETTING
    check(lib.r2l_adam_step_packed(ptr(t[0]), ptr(t[1]), ptr(t[2]), ptr(t[3]), n_block, lr, b1, b2, eps, step, s, ptr(guard), ptr(fwd),
                                   ptr(bwd), stream()), "r2l_adam_step_packed")


@pytest.mark.parametrize("n_block", [0, 1, 43])
def test_adam_packed(lib, n_block):
    """r2l_adam_step_packed against r2l_adam_step_guarded + the two layout-2 packs on clones of one state: parameters and moments
    bit-equal and within the bars of adam64, both whole stream buffers bit-equal as int32 (status words included); with guard
    word 1 nothing moves.  n_block 0 (no tile workgroups), 1 and 43 move the head / bias / tail offsets of the "rest" loop."""
    _, step, s, b1, b2, eps, lr = PACK_SETTING
    t0, fwd0, bwd0, planted = packed_state(lib, n_block, 20 + n_block)
    zero = torch.zeros(1, dtype=torch.int32, device="cuda")
    one = torch.ones(1, dtype=torch.int32, device="cuda")
    # guard word 1: nothing moves
    t, fwd, bwd = [a.clone() for a in t0], fwd0.clone(), bwd0.clone()
    packed_call(lib, t, n_block, fwd, bwd, one)
    for a, b in zip(t + [fwd, bwd], t0 + [fwd0, bwd0]):
        assert torch.equal(bits(a), bits(b))
    # the packed call
    ta, fa, ba = [a.clone() for a in t0], fwd0.clone(), bwd0.clone()
    packed_call(lib, ta, n_block, fa, ba, zero)
    # the separate launches
    tb, fb, bb = [a.clone() for a in t0], fwd0.clone(), bwd0.clone()
    check(lib.r2l_adam_step_guarded(ptr(tb[0]), ptr(tb[1]), ptr(tb[2]), ptr(tb[3]), tb[0].numel(), lr, b1, b2, eps, step, s, ptr(zero),
                                    stream()), "r2l_adam_step_guarded")
    pack_both(lib, tb[0], n_block, fb, bb)
    for k, name in enumerate(("params", "grads", "exp_avg", "exp_avg_sq")):
        assert torch.equal(bits(ta[k]), bits(tb[k])), name
    assert torch.equal(bits(ta[1]), bits(t0[1]))
    assert torch.equal(bits(fa), bits(fb)), "forward stream"
    assert torch.equal(bits(ba), bits(bb)), "backward stream"
    assert not torch.equal(bits(ta[0]), bits(t0[0]))
    if planted:
        at = torch.tensor(planted, device="cuda")
        assert torch.equal(bits(ta[0][at]), bits(t0[0][at]))  # the planted weights went through the update unchanged
        assert not torch.equal(bits(fa), bits(fwd0)) and not torch.equal(bits(ba), bits(bwd0))
    ref = OU.adam64(*t0, lr, b1, b2, eps, step, s)
    assert_bars(OU.fractions(ta[0], ta[2], ta[3], ref), "adam_step_packed n_block=%d" % n_block)


# ---- the fp16x2 streams against an independent statement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_block", [1, 3])
def test_fp16x2_streams_vs_restatement(lib, n_block):
    """Both layout-2 streams bit for bit against tests/optim_util.py's numpy gathers (head bias stage, 63 head stages, body bias
    stages, body weight stages, zero stages), as left by the separate packers and by the packed optimizer call, at scale 1."""
    t, fwd, bwd, planted = packed_state(lib, n_block, 40 + n_block)
    flat = t[0].cpu().numpy()
    stages = OU.fwd_stages(n_block)
    for who in ("packers", "adam_step_packed"):
        if who == "adam_step_packed":
            packed_call(lib, t, n_block, fwd, bwd, torch.zeros(1, dtype=torch.int32, device="cuda"))
            new = t[0].cpu().numpy()
            assert not np.array_equal(new, flat)
            flat = new
        got_f, want_f = region_bits(lib, fwd, n_block, True), OU.fwd_stream_bits(flat, n_block)
        got_b, want_b = region_bits(lib, bwd, n_block, False), OU.bwd_stream_bits(flat, n_block)
        assert got_f.shape == want_f.shape and got_b.shape == want_b.shape
        bad = np.nonzero((got_f != want_f).reshape(got_f.shape[0], -1).any(axis=1))[0]
        assert bad.size == 0, (who, "forward stages", bad[:10])
        bad = np.nonzero((got_b != want_b).reshape(got_b.shape[0], -1).any(axis=1))[0]
        assert bad.size == 0, (who, "backward stages", bad[:10])
        _, status = stream_region(lib, fwd, n_block, True)
        words = fwd[status:status + 16].view(torch.int32).cpu()
        assert int(words[4]) == 0x52324c34 and float(words.view(torch.float32)[2]) == 1.0  # committed, scale 1
    # the planted values are where the restatement says, as the bit patterns tests/test_optimizer_cpu.py::test_split16 lists
    hi, mid = OU.split16(flat[planted[:len(PLANTED)]])
    assert list(hi) == [0x0000, 0x8000, 0x7BFF, 0x7C00, 0x0000] and list(mid) == [0, 0, 0, 0xFC00, 0]
    idx, kind = OU.fwd_gather(n_block)
    for at, h16 in zip(planted[:len(PLANTED)], hi):
        g, w = np.nonzero(idx[:stages] == at)
        assert g.size == 1 and kind[g[0]] == 0 and got_f[g[0], 0, w[0]] == h16


# ---- r2l_loss_finish ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inv_denom", [1.0 / 3, 1.0 / (3 * 4096)])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 100003])
def test_loss_finish(lib, n, inv_denom):
    rng = np.random.default_rng(n)
    x = (10.0 ** rng.uniform(-8, 2, n)).astype(np.float32)
    mse, psnr, bm, bp = OU.loss64(x, inv_denom)
    part = fenced(torch.from_numpy(x).cuda())
    out = torch.full((4,), SENTINEL, dtype=torch.float32, device="cuda")
    check(lib.r2l_loss_finish(ptr(part, 1), n, inv_denom, ptr(out, 1), stream()), "r2l_loss_finish")
    got = out.cpu().double()
    assert got[0].item() == np.float32(SENTINEL) and got[3].item() == np.float32(SENTINEL)
    assert torch.equal(part[1:-1].cpu(), torch.from_numpy(x))
    em, ep = abs(got[1].item() - mse), abs(got[2].item() - psnr)
    print("YARDSTICK gpu loss_finish n=%d inv_denom=%.3g: mse %.3f of its bar, psnr %.3f of its bar" % (n, inv_denom, em / bm, ep / bp))
    assert em <= bm and ep <= bp, (em / bm, ep / bp)


def test_loss_finish_edges(lib):
    out = torch.full((2,), SENTINEL, dtype=torch.float32, device="cuda")
    part = torch.zeros(1000, device="cuda")
    for n in (1000, 0):
        out.fill_(SENTINEL)
        check(lib.r2l_loss_finish(ptr(part), n, 1.0 / 3, ptr(out), stream()), "r2l_loss_finish")
        assert out[0].item() == 0.0 and out[1].item() == math.inf, (n, out)
    part[123] = math.nan
    part[:100] = 1.0
    check(lib.r2l_loss_finish(ptr(part), 1000, 1.0 / 3, ptr(out), stream()), "r2l_loss_finish")
    assert torch.isnan(out).all()


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------------------
def _student():
    from model.nerf_raybased import PointSampler
    from r2l_amd.train_step import R2LTrainer
    from tests.test_forward_gpu import build_model
    tr = R2LTrainer(build_model(O.make_state_dict(n_block=1, seed=6), 1), PointSampler(400, 400, 555.5555155968841, 16, 2., 6.))
    return tr, tr.eng.flat, list(tr.eng.params)


def _teacher():
    from r2l_amd.teacher_train import TeacherTrainer
    from tests.test_teacher_train_gpu import make_teacher
    csd, fsd = O.make_teacher_state_dicts(5, 2, alpha_bias=0.5)
    tr = TeacherTrainer(make_teacher(csd), make_teacher(fsd), perturb=1., white_bkgd=True)
    return tr, tr.flat, list(tr.params)


@pytest.mark.parametrize("make", [_student, _teacher], ids=["student", "teacher"])
def test_trainer_adam_and_state_dict(make):
    """tr.adam(lr) on synthetic gradients and preset moments at step_count 999: within the bars of adam64 with the trainer's betas
    and eps.  Then optimizer_state_dict goes into torch.optim.Adam on CPU copies and both step once more on the same gradients:
    the kernel within the bars, torch within torch_allowance (tests/optim_util.py) of adam64 of the same state."""
    tr, flat, params = make()
    n = flat.numel()
    assert n == sum(q.numel() for q in params)
    lr, (b1, b2), eps = 3.3e-4, tr.betas, tr.eps
    base = [np.resize(a, n) for a in OU.adam_inputs(min(n, SIZES[-1]), 7)]
    base[0] = flat.detach().cpu().numpy().copy()
    _, g, m, v = OU.for_setting(base, ("trainer", 1000, 1.0, b1, b2, eps, lr))
    g, m, v = [torch.from_numpy(a).cuda() for a in (g, m, v)]
    tr.grads.copy_(g)
    tr.exp_avg.copy_(m)
    tr.exp_avg_sq.copy_(v)
    tr.step_count = 999
    p0 = flat.detach().clone()
    tr.adam(lr)
    assert tr.step_count == 1000
    ref = OU.adam64(p0, g, m, v, lr, b1, b2, eps, 1000, 1.0)
    assert torch.equal(tr.grads, g)
    assert_bars(OU.fractions(flat.detach(), tr.exp_avg, tr.exp_avg_sq, ref), "trainer.adam %s" % make.__name__)
    # the state dict, stepped by torch
    sd = tr.optimizer_state_dict(lr)
    p1, m1, v1 = flat.detach().clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone()
    cpu, off = [], 0
    for q in params:
        cpu.append(torch.nn.Parameter(p1[off:off + q.numel()].view(q.shape).cpu().clone()))
        off += q.numel()
    opt = torch.optim.Adam(cpu, lr=lr, betas=(b1, b2), eps=eps)
    opt.load_state_dict(sd)
    off = 0
    for q in cpu:
        q.grad = g[off:off + q.numel()].view(q.shape).cpu().clone()
        off += q.numel()
    opt.step()
    tr.adam(lr)
    assert tr.step_count == 1001 and float(opt.state[cpu[0]]["step"]) == 1001
    ref = OU.adam64(p1, g, m1, v1, lr, b1, b2, eps, 1001, 1.0)
    assert_bars(OU.fractions(flat.detach(), tr.exp_avg, tr.exp_avg_sq, ref), "trainer.adam %s, second step" % make.__name__)
    allow = OU.torch_allowance(ref, g, m1, lr, b1, b2, eps, 1001)
    tp = torch.cat([q.detach().reshape(-1) for q in cpu]).cuda()
    tm = torch.cat([opt.state[q]["exp_avg"].reshape(-1) for q in cpu]).cuda()
    tv = torch.cat([opt.state[q]["exp_avg_sq"].reshape(-1) for q in cpu]).cuda()
    fr = OU.fractions(tp, tm, tv, ref, extra=allow)
    print("YARDSTICK gpu torch.optim.Adam on %s's state dict vs adam64: fraction of the allowance m %.3f v %.3f p %.3f"
          % (make.__name__, fr["m"], fr["v"], fr["p"]))
    for k in fr:
        assert fr[k] <= 1.0, (k, fr)
    # and the kernel's state is not torch's bit for bit: the documented distance is there (v's increment weight)
    assert not torch.equal(tv, tr.exp_avg_sq)
