"""The teacher's three render stages (csrc/r2l_render.hip) through the C ABI, at every kernel instance and on the rows real scenes
produce, against the yardsticks of tests/render_util.py (checked without a GPU by tests/test_render_stages_cpu.py).

r2l_raw2outputs: all five outputs per ray against the oracle's op sequence in fp64, S x R = {1, 2, 63, 65, 127, 129, 160, 191, 193,
255; 64, 128, 192, 256} x {1, 3, 5, 8, 9, 17, 45}, rays cycling through nine kinds (plain, exact zeros, duplicated depths, alpha = 1
once and four times in a row, trained-like magnitudes, sign-flipping noise, two empty kinds), with and without the weights output.
Bars = 4 x the distance of the reference's OWN fp32 arithmetic (torch on the CPU) from the same yardstick over the same table:

  output             reference fp32 (measured / used)   bar       ceiling (the older shapes test's atol / rtol)
  rgb                4.62e-7 / 4.7e-7                    1.88e-6   3e-6
  weights            4.80e-7 / 4.9e-7                    1.96e-6   3e-6
  acc                7.44e-7 / 7.5e-7                    3.00e-6   3e-6
  depth / max|z|     5.02e-7 / 5.1e-7                    2.04e-6   3e-6
  disp (relative)    1.43e-6 / 1.5e-6                    6.00e-6   3e-5

The kernels' worst values per instance, measured on one MI355X over the whole table (133 tests of this file: 3.1 s):

  instance (S)                      rgb       weights   acc       depth     disp
  <1,4>       (1, 2, 63)            1.73e-7   2.40e-7   2.48e-7   1.95e-7   2.88e-7
  <2,4>       (65, 127)             3.89e-7   5.79e-7   5.30e-7   3.87e-7   9.27e-7
  <3,2>       (129, 160, 191)       5.09e-7   6.58e-7   5.23e-7   4.61e-7   4.38e-7
  <4,2>       (193, 255)            6.18e-7   8.80e-7   7.23e-7   4.83e-7   2.42e-6
  16<ROWS=4>  (64)                  2.55e-7   1.39e-7   1.61e-7   1.73e-7   5.25e-7
  16<ROWS=8>  (128)                 2.67e-7   5.70e-7   4.10e-7   3.31e-7   9.22e-7
  16<ROWS=12> (192)                 5.25e-7   7.19e-7   1.03e-6   7.28e-7   4.23e-7
  16<ROWS=16> (256)                 6.63e-7   1.41e-6   1.07e-6   7.53e-7   1.17e-6
  worst / bar                       0.35      0.72      0.36      0.37      0.40

Nothing exceeds a bar; weights at ROWS = 16 is the one figure within 3 x of its bar's edge.  Self-check: every probe sample
(0, 15, 16, 63, 64, S - 1 at S = 64, 65, 160, 256) has 8 - 15 live rays of 45, and the bars see the missing sample on all of them.

r2l_stratified_z: equal bits with the reference's fp32 expressions (render_util.strat_spec), three near / far layouts, without and
with jitter, S = 1 and the grid-stride loop included.  r2l_sample_pdf_sort: the oracle's sample_pdf in fp64 under the bar and the
excuses of test_teacher_gpu.py::test_sample_pdf_sort_shapes_vs_oracle, at the extremes of the argument check and on degenerate pdfs;
u = 0 and the merged depths bit for bit; the generic and the quarter-wave kernel agree bit for bit.  Measured on one MI355X: every
bit-equality holds; outside the excused samples the worst |got - want| / allowed is 0.22 at (64, 192, 17), 0.13 at (63, 128, 21) and
(64, 128, 3), below 0.07 elsewhere.
Every output buffer of every call sits between guard zones that must come back intact."""
import ctypes

import pytest
import torch

from tests import render_util as U
from tests.test_teacher_backward_gpu import guarded, guards_intact, untouched

pytestmark = pytest.mark.gpu


def _lib():
    from r2l_amd import _lib as L
    return L


def _p(t):
    from r2l_amd.engine import _ptr
    return _ptr(t)


def _s():
    from r2l_amd.engine import _stream
    return _stream()


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- compositing ------------------------------------------------------------------------------------------------------------
def r2o_launch(R, S, want_weights):
    """r2l_raw2outputs on the table's case into guarded buffers: ((rgb, disp, acc, weights or None, depth) on the CPU, all guards
    intact)."""
    lib = _lib().load()
    raw, z, d, noise, white = U.r2o_inputs(R, S)
    dev = [None if t is None else t.cuda().contiguous() for t in (raw, z, d, noise)]  # (kept alive: the C ABI takes raw pointers)
    sizes = {"rgb": 3 * R, "disp": R, "acc": R, "weights": R * S, "depth": R}
    if not want_weights:
        del sizes["weights"]
    buf = {k: guarded(n) for k, n in sizes.items()}
    ptr = {k: _p(v[1]) for k, v in buf.items()}
    _lib().check(lib.r2l_raw2outputs(_p(dev[0]), _p(dev[1]), _p(dev[2]), _p(dev[3]), int(white), ptr["rgb"], ptr["disp"], ptr["acc"],
                                     ptr.get("weights", ctypes.c_void_p(0)), ptr["depth"], R, S, _s()), "r2l_raw2outputs")
    torch.cuda.synchronize()
    intact = all(guards_intact(buf[k][0], n) for k, n in sizes.items())
    out = {k: v[1].cpu() for k, v in buf.items()}
    return (out["rgb"].view(R, 3), out["disp"], out["acc"], out["weights"].view(R, S) if want_weights else None, out["depth"]), intact


@pytest.mark.parametrize("R", U.R2O_R)
@pytest.mark.parametrize("S", U.R2O_S)
def test_raw2outputs_vs_fp64(S, R):
    """Every output of every ray within its bar of the fp64 yardstick (the bars and their origin: the module docstring); finite
    except disp, which is NaN exactly on the rays whose fp64 opacity is 0; nothing written outside the five buffers; and the call
    without weights returns the other four bit for bit."""
    got, intact = r2o_launch(R, S, True)
    assert intact, "write outside an output buffer"
    want = U.r2o_want(R, S)
    assert all(bool(torch.isfinite(got[i]).all()) for i in (0, 2, 3, 4)), "an entry was not written, or is not finite"
    assert torch.equal(torch.isnan(got[1]), want[2] == 0), "disp is NaN on other rays than the empty ones"
    err = U.r2o_errors(got, want, U.r2o_inputs(R, S)[1])
    worst = U.r2o_worst(err)
    print("raw2outputs S %d R %d instance %s: rgb %.3g weights %.3g acc %.3g depth %.3g disp %.3g" % (
        S, R, U.r2o_instance(S), worst["rgb"], worst["weights"], worst["acc"], worst["depth"], worst["disp"]))
    bad = {k: [int(r) for r in f.nonzero().flatten()] for k, f in U.r2o_failures(err).items() if bool(f.any())}
    assert not bad, (bad, worst, [U.R2O_KINDS[U.r2o_kind(r, S)] for rs in bad.values() for r in rs][:8])
    lean, intact = r2o_launch(R, S, False)
    assert intact, "write outside an output buffer (call without weights)"
    for i in (0, 1, 2, 4):  # (disp is NaN on an empty ray: compare the bits)
        assert torch.equal(bits(lean[i]), bits(got[i])), "the call without weights returns other maps"


@pytest.mark.parametrize("S", U.R2O_PROBE_S)
def test_raw2outputs_bars_see_one_missing_sample(S):
    """Self-check of the bars: the kernel's unchanged output against the yardstick WITHOUT sample p of every ray (alpha_p = 0), for
    p at the first sample, either side of the first lane-row / chunk edges (15 | 16, 63 | 64) and the last sample.  Every ray
    whose w64[p] is above 10 x the weights bar must fail the weights bar and at least one map bar.  The device is never asked to
    misbehave."""
    R = U.R2O_PROBE_R
    got, _ = r2o_launch(R, S, True)
    err = U.r2o_errors(got, U.r2o_want(R, S), U.r2o_inputs(R, S)[1])
    assert not any(bool(f.any()) for f in U.r2o_failures(err).values())
    for p, (live, unseen) in U.r2o_self_check(got, R, S).items():
        print("raw2outputs S %d: without sample %d, %d live rays, %d not seen by the bars" % (S, p, live, unseen))
        assert live >= 1 and unseen == 0, (S, p, live, unseen)


# ---- coarse depths ----------------------------------------------------------------------------------------------------------
def strat_launch(near_ptr, far_ptr, nf_stride, ttab, t_rand, R, S):
    lib = _lib().load()
    whole, z = guarded(R * S)
    rc = lib.r2l_stratified_z(near_ptr, far_ptr, nf_stride, _p(ttab), _p(t_rand), _p(z), R, S, _s())
    torch.cuda.synchronize()
    return rc, whole, z


@pytest.mark.parametrize("S,R", U.STRAT_SHAPES + [U.STRAT_BIG])
def test_stratified_z_bit_for_bit(S, R):
    """z_out has the bits of the reference's fp32 expressions (render_util.strat_spec == the torch-op branch of
    r2l_amd.render._coarse_z), without and with jitter (t_rand holds exact 0 and 1 - 2^-24), for per-ray near / far as two arrays
    (nf_stride 1), as columns 6 and 7 of [R,11] ray rows (nf_stride 11) and for one shared pair (nf_stride 0); nothing is written
    outside z_out.  (65, 16385) is more than 4096 x 256 elements: the grid-stride loop's second trip."""
    near, far, rows, t_rand = U.strat_inputs(R, S)
    near_d, far_d, rows_d = near.cuda().contiguous(), far.cuda().contiguous(), rows.cuda().contiguous()
    ttab, tr_d = U.strat_ttab(S).cuda(), t_rand.cuda().contiguous()
    col = lambda k: ctypes.c_void_p(rows_d.data_ptr() + 4 * k)
    layouts = {"nf_stride 1": (_p(near_d), _p(far_d), 1, near, far), "nf_stride 11": (col(6), col(7), 11, near, far),
               "nf_stride 0": (_p(near_d), _p(far_d), 0, near[:1], far[:1])}
    assert tuple(layouts) == U.STRAT_LAYOUTS
    for name, (np_, fp_, stride, n_cpu, f_cpu) in layouts.items():
        for tr_cpu, tr in ((None, None), (t_rand, tr_d)):
            rc, whole, z = strat_launch(np_, fp_, stride, ttab, tr, R, S)
            assert rc == 0
            assert guards_intact(whole, R * S), (name, "write outside z_out")
            want = U.strat_spec(n_cpu, f_cpu, R, S, tr_cpu)
            diff = bits(z.cpu().view(R, S)) != bits(want)
            assert not bool(diff.any()), (name, "jitter" if tr is not None else "no jitter", int(diff.sum()), diff.nonzero()[:5])


def test_stratified_z_no_rays():
    """R = 0 returns 0 and writes nothing."""
    S = 16
    near, far, _, _ = U.strat_inputs(5, S)
    near_d, far_d, ttab = near.cuda(), far.cuda(), U.strat_ttab(S).cuda()
    whole, z = guarded(64)
    rc = _lib().load().r2l_stratified_z(_p(near_d), _p(far_d), 1, _p(ttab), None, _p(z), 0, S, _s())
    torch.cuda.synchronize()
    assert rc == 0
    assert untouched(whole)


# ---- importance sampling ----------------------------------------------------------------------------------------------------
def pdf_launch(S, NI, R, odd_stride=False):
    """r2l_sample_pdf_sort on the table's case into guarded buffers: (z_samples, z_all, z_std on the CPU, guards intact, all
    pointers 16-byte aligned).  odd_stride: u rows of NI + 1 floats, which the quarter-wave kernel cannot take."""
    lib = _lib().load()
    z, w, u = U.pdf_inputs(S, NI, R)
    stride = NI
    if odd_stride:
        stride = NI + 1
        u = torch.cat([u, torch.zeros(R, 1)], -1)
    z_d, w_d, u_d = z.cuda().contiguous(), w.cuda().contiguous(), u.cuda().contiguous()
    sizes = (R * NI, R * (S + NI), R)
    buf = [guarded(n) for n in sizes]
    _lib().check(lib.r2l_sample_pdf_sort(_p(z_d), _p(w_d), _p(u_d), stride, _p(buf[0][1]), _p(buf[1][1]), _p(buf[2][1]), R, S, NI,
                                         _s()), "r2l_sample_pdf_sort")
    torch.cuda.synchronize()
    intact = all(guards_intact(b[0], n) for b, n in zip(buf, sizes))
    aligned = all(t.data_ptr() % 16 == 0 for t in (z_d, w_d, u_d, buf[0][1], buf[1][1]))
    return buf[0][1].cpu().view(R, NI), buf[1][1].cpu().view(R, S + NI), buf[2][1].cpu(), intact, aligned


@pytest.mark.parametrize("S,NI,R", U.PDF_SHAPES)
def test_sample_pdf_sort_vs_fp64(S, NI, R):
    """z_samples under the judgement of render_util.pdf_judge against the oracle's sample_pdf in fp64 (the older shapes test's bar
    and knife excuse, plus the edge excuse; the excused share is capped on the CPU), on rays cycling through random, all-zero,
    one-hot, two-or-three-bin, 1e-6 and duplicated-depth rows; u = 0 gives bins[:, 0] and z_all is torch.sort of the kernel's own
    samples, both bit for bit; z_std; guards.  (64, 128, R) takes the quarter-wave kernel (its alignment precondition is
    asserted) and must agree bit for bit with the generic kernel, reached through an odd u stride."""
    zs, z_all, z_std, intact, aligned = pdf_launch(S, NI, R)
    assert intact, "write outside an output buffer"
    assert bool(torch.isfinite(zs).all() and torch.isfinite(z_all).all() and torch.isfinite(z_std).all()), "an entry was not written"
    ok = U.pdf_judge(zs, S, NI, R)
    c = U.pdf_want(S, NI, R)
    e = ((zs.double() - c["want"]).abs() / c["allowed"])[~(c["knife"] | c["edge"])]
    print("sample_pdf_sort (%d, %d, %d): worst |got - want| / allowed %.3g outside the excused samples" % (
        S, NI, R, float(e.max()) if e.numel() else 0.))
    assert bool(ok.all()), [(int(r), int(i), U.PDF_KINDS[int(r) % len(U.PDF_KINDS)]) for r, i in (~ok).nonzero()[:10]]
    assert not U.pdf_exact_facts(zs, z_all, z_std, S, NI, R)
    if (S, NI) == (64, 128):
        assert aligned, "the quarter-wave kernel needs 16-byte aligned rows: this case did not take it"
        gs, ga, gd, intact, _ = pdf_launch(S, NI, R, odd_stride=True)
        assert intact, "write outside an output buffer (generic kernel)"
        assert torch.equal(bits(zs), bits(gs)) and torch.equal(bits(z_all), bits(ga)) and torch.equal(bits(z_std), bits(gd))
