"""Every gradient of the student's training step, per entry, against fp64 on mask-stable rays — under every kernel family.

The yardstick (tests/student_util.py) is the fp64 backprop of the reference's own loss; it knows no stash layout.  The rays of
every case are SELECTED by the fp64 forward alone, before a kernel runs: those whose every ReLU input lies at least delta of its
absolute-product magnitude away from zero, so that no summation order can flip a mask.  The kernels get exactly those N rays and
every entry of every gradient tensor is compared; nothing is left out afterwards.  tests/test_student_yardstick_cpu.py checks
the conditions this relies on without a GPU.

Paths:  (a) rays path, all eight families of tests/test_train_gpu.FAMILIES: R2LTrainer.forward_backward (MSE mode: sampler,
encoder and the head's re-encoding inside the kernels), and generic mode (r2l_backward_part_cfg with a caller's dL/drgb);
(b) pre-embedded path (r2l_forward_emb_cfg with stash + r2l_backward_part_cfg with emb, as r2l_amd/autograd.py), tilings main
and coop16.  If (a) fails for an exact family where (b) passes, the sampler or encoder is at fault, not the GEMMs.

Bars, every tensor (biases included) of every case:
  exact families (main-exact, coopf-exact, main-bf16x3-trio, main-f32mfma, coop16) and the pre-embedded path:
      per entry |got - want| <= 3e-6 * mag + floor, per tensor norm-relative <= 1e-5 (C_BWD, NREL_BWD of the teacher's test);
  default trio (main, coopf, coopf2): head and body tensors norm-relative <= 3 * e_model + 1e-5, e_model the error of the fp16-hi
      operand model (student_util.half_hi) computed in fp64 on the same inputs; tail.0.* (fp32 operands) at the exact bars;
  rgb within 1e-4, loss within 1e-6.
Measured on one MI355X over the whole table (610 tests of this file and tests/test_sincos_gpu.py: 33 s), worst case per group:
  group                                        norm-relative (bar)              |got - want| / mag (bar 3e-6)
  rays, bf16x3 trio / fp32 MFMA / coop16       2.3e-6 (1e-5)                    1.1e-6  head.0.weight, n_block 43 N 65
  rays, main-exact / coopf-exact               2.3e-6 (1e-5)                    1.1e-6; head.0.weight 1e-3 at N = 16, 2.1e-5 at
                                                                                N = 31: its bar is derived below (EXACT_FP16)
  rays, default trio: tail.0.*                 1.4e-6 (1e-5)                    3.1e-7
  rays, default trio: head and body            0.332 of 3 * e_model + 1e-5 at the most (3.91e-4 measured, model 3.89e-4, generic
                                               mode N = 65; 2.0e-5 at N = 16385): the fp16-hi model IS the error, to 1 %
  pre-embedded path, main / coop16             3.8e-6 (1e-5)                    1.05e-6
  rgb 2.4e-6 (1e-4), loss 4.8e-8 (1e-6); rejected shares 5.3 - 10.7 % / 16.9 - 19.0 % / 37.9 - 39.5 % at n_block <= 3 / 8 / 43.
The fp32 figures are WITHIN 3x of their bars at n_block 43, N = 65 (per entry 1.1e-6 of 3e-6; norm-relative 3.8e-6 of 1e-5,
pre-embedded path).  One missing ray: every weight tensor of the dropped yardstick is off by >= 3.4e-2 norm-relative at
N = 65, 2.4e-3 at N = 1000 and 1.36e-3 at N = 4097, against bars of 1e-5 and 3 * e_model + 1e-5 = 7.5e-4 / 2.5e-4 / 1.4e-4.
"""
import pytest
import torch

from oracle import r2l_oracle as O
from tests import student_util as S
from tests.conftest import use_family
from tests.test_forward_gpu import build_model
from tests.test_teacher_backward_gpu import guarded, guards_intact
from tests.test_train_gpu import FAMILIES

pytestmark = pytest.mark.gpu

EXACT = ("main-exact", "coopf-exact", "main-bf16x3-trio", "main-f32mfma", "coop16")
# dw_mode = exact of the fp16 trio: every weight-gradient operand is an fp16 pair hi + mid (csrc/r2l_dw_head16.hip, r2l_dw16.hip).
# That is 2^-22 relative per operand (2^-21 per product, not fp32's 2^-24), and an ABSOLUTE floor of 2^-25 — half of fp16's
# subnormal spacing — on each: on the encoding value, and on the gradient times the chain's power-of-two scale.  Both show in
# head.0.weight entries of FEW rays whose unit is live for one ray and whose encoding column is ~1e-5 there (a sine next to a
# zero): 1e-3 of `mag` at N = 16, 2.1e-5 at N = 31, at 1.2e-6 norm-relative of the tensor.  So for these two families, and
# head.0.weight only: C_BWD x 8 (= 2^-21 / 2^-24, the widest the fp32 bar may be stretched for them) plus the floor derived from
# the 2^-25:  |dW[i][j]| error <= 2^-25 * (sum_p |G[p][i]| + sum_p |PE[p][j]| / gscale).  Every other tensor, and the
# norm-relative bar of this one, stay at the fp32 values.
EXACT_FP16 = ("main-exact", "coopf-exact")
HALF_FLOOR = 2.0 ** -25
TRIO = ("main", "coopf", "coopf2")
assert set(EXACT) | set(TRIO) == set(FAMILIES)

_CASES = {}


def case(nb, n, perturb, path="rays", mode="mse"):
    """Inputs and yardstick of one case, computed once (fp64 on the GPU through torch) and shared by the families."""
    key = (nb, n, perturb, path, mode)
    if key not in _CASES:
        sd = O.make_state_dict(n_block=nb, seed=S.NET_SEED)
        c = S.select_case(sd, n, perturb, S.case_seed(nb, n, perturb), device="cuda", through_fp32=(path == "emb"))
        assert c["rejected"] <= S.REJECT_CAP[nb], c["rejected"]
        sd64 = S.f64(sd, "cuda")
        kw = dict(target64=c["tgt"].double().cuda())
        if mode == "generic":  # a caller's dL/drgb that is no MSE gradient
            kw = dict(drgb64=(torch.randn(n, 3, generator=torch.Generator().manual_seed(n)) * 1e-3).double().cuda())
        rgb, loss, want, mags = S.backward64(sd64, c["emb64"], **kw)
        _, _, model, _ = S.backward64(sd64, c["emb64"], round_op=S.half_hi, **kw)
        c.update(sd=sd, sd64=sd64, kw=kw, rgb=rgb, loss=loss, want=want, mags=mags, pe_colsum=c["emb64"].abs().sum(0),
                 e_model={k: S.nrel(model[k], want[k]) for k in sd})
        if path != "emb":
            del c["emb64"]  # (kept for the self-check only where it is asked for again: recomputed there)
        _CASES[key] = c
    return _CASES[key]


def sampler():
    from model.nerf_raybased import PointSampler
    return PointSampler(400, 400, 555.5555155968841, S.N_SAMPLE, S.NEAR, S.FAR)


def run_rays(c, nb, n, perturb, generic=False):
    """The step on the device: (rgb, loss or None, grads dict, whole guarded buffer, n_param)."""
    from r2l_amd import _lib
    from r2l_amd.engine import _ptr, _stream
    from r2l_amd.train_step import R2LTrainer
    ps = sampler()
    tr = R2LTrainer(build_model(c["sd"], nb), ps)
    n_param = tr.grads.numel()
    whole, tr.grads = guarded(n_param)
    o, d, tgt, u = [c[k].cuda() for k in ("o", "d", "tgt", "u")]
    rgb = tr.forward_backward(o, d, tgt, perturb=perturb, t_rand=u if perturb > 0 else None)
    loss = tr.loss_out[0].item()
    if generic:
        eng = tr.eng
        t_rand = u.contiguous() if perturb > 0 else None
        rgb = eng.forward_rays(o, d, ps.z_vals, perturb, t_rand, save=(tr.save_x, tr.save_t))
        drgb = c["kw"]["drgb64"].float().contiguous()
        whole, tr.grads = guarded(n_param)
        tr.grads.zero_()
        _lib.check(tr.lib.r2l_backward_part_cfg(_ptr(o), _ptr(d), _ptr(t_rand), _ptr(eng.ztab(ps.z_vals, perturb)), None, _ptr(rgb),
                                                None, _ptr(drgb), _ptr(tr.save_x), _ptr(tr.save_t), _ptr(tr.wstream_bwd),
                                                _ptr(eng.flat), eng.n_block, 0.0, _ptr(tr.dpre), _ptr(tr.gx), _ptr(tr.gt), None,
                                                _ptr(tr.grads), _ptr(tr.dw_slab), n, _stream(), _lib.BWD_ALL, 0, 2 * eng.n_block,
                                                eng._cfg()), "r2l_backward (generic)")
        loss = None
    torch.cuda.synchronize()
    gscale = None
    if tr.eng.layout_for(n, True) == 2:  # an fp16 family: the family under test ran, not the bf16x3 kernels behind it
        info = tr.range_info()
        assert info["trips"] == 0 and info["bwd_trips"] == 0 and info["grad_scale"] > 0, info
        gscale = info["grad_scale"]
    return rgb, loss, S.split_flat(tr.grads, c["sd"]), whole, n_param, gscale


def run_emb(c, nb, n):
    """r2l_forward_emb_cfg with stash, then r2l_backward_part_cfg with emb in generic mode: the calls of r2l_amd/autograd.py."""
    from r2l_amd import _lib
    from r2l_amd.engine import _ptr, _stream, get_engine
    eng = get_engine(build_model(c["sd"], nb))
    eng.ensure_packed()
    lib = eng.lib
    f = dict(dtype=torch.float32, device="cuda")
    emb = c["emb64"].float().contiguous()
    assert torch.equal(emb.double(), c["emb64"])  # identical to the reference's input to the bit
    slot = int(lib.r2l_stash_slot_floats(n))
    save_x, save_t = torch.empty((nb + 1) * slot, **f), torch.empty(max(nb, 1) * slot, **f)
    rgb = eng.forward_emb(emb, save=(save_x, save_t))
    wbwd = torch.empty(lib.r2l_bwd_stream_floats(nb), **f)
    _lib.check(lib.r2l_pack_backward(_ptr(eng.flat), nb, _ptr(wbwd), _stream()), "r2l_pack_backward")
    whole, grads = guarded(eng.n_param)
    grads.zero_()
    gx, gt = torch.empty((nb + 1) * slot, **f), torch.empty(max(nb, 1) * slot, **f)
    dpre, slab = torch.empty(n * 3, **f), torch.empty(int(lib.r2l_dw_slab_floats()), **f)
    drgb = c["kw"]["drgb64"].float().contiguous()
    _lib.check(lib.r2l_backward_part_cfg(None, None, None, None, _ptr(emb), _ptr(rgb), None, _ptr(drgb), _ptr(save_x),
                                         _ptr(save_t), _ptr(wbwd), _ptr(eng.flat), nb, 0.0, _ptr(dpre), _ptr(gx), _ptr(gt), None,
                                         _ptr(grads), _ptr(slab), n, _stream(), _lib.BWD_ALL, 0, 2 * nb, eng._cfg()),
               "r2l_backward (emb)")
    torch.cuda.synchronize()
    return rgb, None, S.split_flat(grads, c["sd"]), whole, eng.n_param, None


def bar_failures(family, got, want, mags, e_model, c=None, gscale=None):
    """{tensor: (what, measured, bar)} of the tensors that miss the bar of their family group."""
    exact = family in EXACT
    viol = S.entry_violations(got, want, mags)
    if family in EXACT_FP16:
        k = "head.0.weight"
        floor = HALF_FLOOR * (mags["head.0.bias"][:, None] + c["pe_colsum"][None, :] / gscale)
        viol[k] = int(((got[k].double() - want[k]).abs() > 8 * S.C_BWD * mags[k] + floor).sum().item())
    bad = {}
    for k in want:
        e = S.nrel(got[k], want[k])
        if exact or k.startswith("tail."):
            if viol[k]:
                bad[k] = ("entries beyond 3e-6 * mag", viol[k], 0)
            elif e > S.NREL_BWD:
                bad[k] = ("norm-relative", e, S.NREL_BWD)
        elif e > 3 * e_model[k] + S.NREL_BWD:
            bad[k] = ("norm-relative", e, 3 * e_model[k] + S.NREL_BWD)
    return bad


def check(tag, family, c, out):
    rgb, loss, got, whole, n_param, gscale = out
    want, mags, e_model = c["want"], c["mags"], c["e_model"]
    assert guards_intact(whole, n_param), "write outside grads"
    assert all(bool(torch.isfinite(v).all().item()) for v in got.values()), "a gradient entry is not finite"
    rgb_err = (rgb.double() - c["rgb"]).abs().max().item()
    loss_err = abs(loss - c["loss"].item()) if loss is not None else 0.
    exact = family in EXACT
    strict = [k for k in want if exact or k.startswith("tail.")]
    worst_n = max((S.nrel(got[k], want[k]), k) for k in strict)
    worst_r = S.worst_ratio({k: got[k] for k in strict}, {k: want[k] for k in strict}, mags)
    line = "%s %s: rgb %.3g, loss %.3g; exact-bar tensors: norm-relative %.3g (%s), |got - want| / mag %.3g (%s)" % (
        tag, family, rgb_err, loss_err, worst_n[0], worst_n[1], worst_r[0], worst_r[1])
    if not exact:
        over = max((S.nrel(got[k], want[k]) / (3 * e_model[k] + S.NREL_BWD), k) for k in want if k not in strict)
        line += "; fp16 tensors: norm-relative %.3g of the bar (%s: %.3g, model %.3g)" % (
            over[0], over[1], S.nrel(got[over[1]], want[over[1]]), e_model[over[1]])
    print(line)
    assert rgb_err < 1e-4 and loss_err < 1e-6, (rgb_err, loss_err)
    bad = bar_failures(family, got, want, mags, e_model, c, gscale)
    assert not bad, dict(list(bad.items())[:6])


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("perturb", [0., 1.])
@pytest.mark.parametrize("nb,n", S.SHAPES)
def test_rays_path_vs_fp64(nb, n, perturb, family, monkeypatch):
    """MSE mode through R2LTrainer.forward_backward, every shape of student_util.SHAPES, with and without stratified jitter."""
    c = case(nb, n, perturb)
    use_family(monkeypatch, **FAMILIES[family])
    check("rays n_block %d N %d perturb %g" % (nb, n, perturb), family, c, run_rays(c, nb, n, perturb))


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("n,perturb", [(65, 1.), (1000, 0.)])
def test_rays_path_generic_mode_vs_fp64(n, perturb, family, monkeypatch):
    """Generic mode: forward with stash, then r2l_backward_part_cfg with a caller's dL/drgb that is no MSE gradient (the fp16
    trio chooses its power-of-two chain scale on the device from max |drgb|)."""
    c = case(3, n, perturb, mode="generic")
    use_family(monkeypatch, **FAMILIES[family])
    check("generic n_block 3 N %d perturb %g" % (n, perturb), family, c, run_rays(c, 3, n, perturb, generic=True))


@pytest.mark.parametrize("tiling", ["main", "coop16"])
@pytest.mark.parametrize("perturb", [0., 1.])
@pytest.mark.parametrize("nb,n", S.SHAPES)
def test_emb_path_vs_fp64(nb, n, perturb, tiling, monkeypatch):
    """The pre-embedded path: exact-fp32 MFMA, row-major stash, input identical to the reference's to the bit — the exact bars."""
    c = case(nb, n, perturb, path="emb", mode="generic")
    use_family(monkeypatch, tiling=tiling)
    check("emb n_block %d N %d perturb %g" % (nb, n, perturb), "main-f32mfma" if tiling == "main" else "coop16", c,
          run_emb(c, nb, n))


@pytest.mark.parametrize("family", ["main-f32mfma", "coopf-exact", "coopf"])
@pytest.mark.parametrize("nb,n", S.SELF_CHECK_SHAPES)
def test_bars_see_one_missing_ray(nb, n, family, monkeypatch):
    """Self-check of the bars, for an fp32-exact family, an exact-dW fp16 family (whose head.0.weight bar is the widened one)
    and the default trio: the yardstick of the same step WITHOUT ray p
    (drop = p: its dL/dz zeroed, the 1/N of the whole step kept) must fail the bar on EVERY weight tensor, with the device's
    unchanged output as `got` — for p = 0, 31, 32, the last ray of the last full 64-ray work unit and N - 1.  The device is never
    asked to misbehave."""
    perturb = 1.
    c = case(nb, n, perturb)
    use_family(monkeypatch, **FAMILIES[family])
    out = run_rays(c, nb, n, perturb)
    got, gscale = out[2], out[5]
    assert not bar_failures(family, got, c["want"], c["mags"], c["e_model"], c, gscale)
    emb64 = S.reference_encoding(c["o"], c["d"], c["u"], perturb, "cuda")
    weights = [k for k in c["sd"] if k.endswith(".weight")]
    for p in S.probe_rays(n):
        _, _, want_p, mags_p = S.backward64(c["sd64"], emb64, drop=p, **c["kw"])
        bad = bar_failures(family, got, want_p, mags_p, c["e_model"], c, gscale)
        margin = min(S.nrel(got[k], want_p[k]) for k in weights)
        print("n_block %d N %d %s: without ray %d every weight tensor is off by >= %.3g norm-relative" % (nb, n, family, p, margin))
        for k in weights:
            assert (c["want"][k] - want_p[k]).abs().max().item() > 0, (p, k, "probe ray without a live path")
            assert k in bad, (p, k, "the bar does not see ray %d missing" % p)
