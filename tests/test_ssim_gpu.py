"""The SSIM kernel (csrc/r2l_ssim.hip) on the GPU, per 16 x 16 tile: every partial and out[0] of every case of tests/ssim_util.py
through the C ABI against the fp64 yardstick, under the bars derived there (and checked without a GPU by tests/test_ssim_cpu.py);
the window the library builds itself; launch invariants (same bits twice, every partial written and none accumulated into,
nothing written outside the buffers); a non-contiguous input through metrics.ssim; the refusals.

Every test prints the figures it asserts (pytest -s, lines starting with YARDSTICK ssim): profiles/ssim_yardstick.txt quotes
them."""
import ctypes

import pytest
import torch

from tests import ssim_util as S

pytestmark = pytest.mark.gpu

G, SENT = 64, -12345.0  # guard words on both sides of every buffer, and what they hold


def _guarded(t):
    """A device copy of the flat fp32 tensor t between G guard words on either side -> (whole buffer, pointer to the payload)."""
    buf = torch.full((t.numel() + 2 * G,), SENT, device="cuda")
    buf[G:G + t.numel()] = t.reshape(-1).cuda()
    return buf, buf.data_ptr() + 4 * G


def run_abi(c, window, fill=SENT):
    """r2l_ssim on the case's images with both images, partial and out between guard words -> partial, out (CPU), after checking
    that the guards and the images are as they were.  window: a [11, 11] fp32 tensor or None (window_host = NULL)."""
    from r2l_amd import _lib
    L = _lib.load()
    H, W, C = c.shape
    n = L.r2l_ssim_partial_count(H, W, C)
    assert n == c.t64.numel()
    a, pa = _guarded(c.pred)
    b, pb = _guarded(c.gt)
    part, pp = _guarded(torch.full((n,), fill))
    out, po = _guarded(torch.full((1,), fill))
    win = window.contiguous() if window is not None else None
    torch.cuda.synchronize()
    _lib.check(L.r2l_ssim(pa, pb, H, W, C, win.data_ptr() if win is not None else None, pp, po,
                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "r2l_ssim")
    torch.cuda.synchronize()
    for name, buf, k in (("img1", a, c.pred.numel()), ("img2", b, c.gt.numel()), ("partial", part, n), ("out", out, 1)):
        assert (buf[:G] == SENT).all().item() and (buf[G + k:] == SENT).all().item(), (c.name, name)
    assert torch.equal(a[G:G + c.pred.numel()].cpu(), c.pred.reshape(-1)) and torch.equal(b[G:G + c.gt.numel()].cpu(), c.gt.reshape(-1))
    return part[G:G + n].cpu(), out[G:G + 1].cpu()


def hold_to_bars(c, partial, out, tag):
    """Assert the bars of the case and report the worst ratios -> them."""
    assert torch.isfinite(partial).all() and torch.isfinite(out).all(), (c.name, tag)
    r_tile, k = S.worst_ratio(partial, c.t64, c.bar_tile)
    r_mean = abs(out.item() - c.mean64) / c.bar_mean
    line = "%s %s: tile %.3f of its bar (entry %d: %.2e from fp64), out[0] %.3f of its bar (%.2e from fp64)" % (
        c.name, tag, r_tile, k, abs(partial[k].item() - c.t64[k].item()), r_mean, abs(out.item() - c.mean64))
    r_seq = None
    if c.seq_t is not None:
        r_seq, _ = S.worst_ratio(partial, c.seq_t, c.seq_bar)
        line += "; against the restatement %.3f of that bar" % r_seq
    # not asserted: does the device equal the restatement summed in the kernel's own order, bit for bit?
    seq = S.ssim_map32_seq(c.pred, c.gt, c.window)
    want = S.tiles32_butterfly(seq)
    same = int((want == partial).sum())
    line += "; partials bit-equal to the restatement in butterfly order: %d of %d, out[0] %s" % (
        same, partial.numel(), "equal" if S.finish32(want, c.pred.numel()) == out.item() else "differs")
    S.report(line)
    assert r_tile <= 1 and r_mean <= 1, (c.name, tag, r_tile, r_mean)
    assert r_seq is None or r_seq <= 1, (c.name, tag, r_seq)
    return r_tile, r_mean, r_seq


@pytest.mark.parametrize("name", S.CASES)
def test_tiles_and_mean_vs_fp64(name):
    c = S.case(name)
    partial, out = run_abi(c, c.window)
    hold_to_bars(c, partial, out, "window passed")
    # the same bits on a second call, and from a partial buffer that held NaN: every partial is written, none accumulated into
    p2, o2 = run_abi(c, c.window, fill=float("nan"))
    assert torch.equal(p2, partial) and torch.equal(o2, out)
    p3, o3 = run_abi(c, c.window, fill=0.0)
    assert torch.equal(p3, partial) and torch.equal(o3, out)


@pytest.mark.parametrize("name", [n for n in S.CASES if not n.endswith("-asym")])
def test_window_computed_by_the_library(name):
    """window_host = NULL under the same bars (the yardstick on the restated library window, which test_ssim_cpu.py holds to the
    reference's bits), and its distance from the call with the window passed."""
    c, lib = S.case(name), S.case(name, "lib")
    partial, out = run_abi(lib, None)
    hold_to_bars(lib, partial, out, "window_host = NULL")
    passed, out_passed = run_abi(c, c.window)
    d = (partial.double() - passed.double()).abs().max().item()
    S.report("%s: NULL window against the passed window: largest tile difference %.2e, out[0] %.2e" % (
        name, d, abs(out.item() - out_passed.item())))
    r, _ = S.worst_ratio(partial, c.t64, c.bar_tile)  # and under the passed window's own bars
    assert r <= 1 and abs(out.item() - c.mean64) <= c.bar_mean


def test_non_contiguous_input_through_metrics():
    """metrics.ssim on [H, W, C] views of CHW tensors equals the contiguous call bit for bit, and both the ABI's out[0]."""
    from r2l_amd import metrics
    c = S.case("47x21x3-wide")
    a, b = c.pred.permute(2, 0, 1).contiguous().cuda().permute(1, 2, 0), c.gt.permute(2, 0, 1).contiguous().cuda().permute(1, 2, 0)
    assert not a.is_contiguous() and not b.is_contiguous() and torch.equal(a.cpu(), c.pred)
    got = metrics.ssim(a, b)
    want = metrics.ssim(c.pred.cuda(), c.gt.cuda())
    assert got.is_cuda and got.dim() == 0 and got.item() == want.item()
    assert want.item() == run_abi(c, c.window)[1].item()
    assert metrics.ssim(a, c.gt.cuda()).item() == want.item() and metrics.ssim(c.pred.cuda(), b).item() == want.item()


def test_refusals_write_nothing():
    """H, W or C of 0, C = 65536 (the grid's z limit is 65535) and a NULL out: non-zero, a message, nothing launched."""
    from r2l_amd import _lib
    L = _lib.load()
    c = S.case("5x6x2-wide")
    H, W, C = c.shape
    a, pa = _guarded(c.pred)
    b, pb = _guarded(c.gt)
    part, pp = _guarded(torch.full((64,), SENT))
    out, po = _guarded(torch.full((1,), SENT))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for args in ((pa, pb, 0, W, C, None, pp, po), (pa, pb, H, 0, C, None, pp, po), (pa, pb, H, W, 0, None, pp, po),
                 (pa, pb, H, W, 65536, None, pp, po), (pa, pb, H, W, C, None, pp, None), (pa, pb, -1, W, C, None, pp, po)):
        assert L.r2l_ssim(*args, stream) != 0, args
        msg = L.r2l_last_error()
        assert msg and b"r2l_ssim" in msg, (args, msg)
        torch.cuda.synchronize()
        assert (part == SENT).all().item() and (out == SENT).all().item(), args
    assert torch.equal(a[G:G + c.pred.numel()].cpu(), c.pred.reshape(-1))
    # and the same buffers still serve a good call
    _lib.check(L.r2l_ssim(pa, pb, H, W, C, None, pp, po, stream), "r2l_ssim")
    torch.cuda.synchronize()
    assert abs(out[G].item() - S.case("5x6x2-wide", "lib").mean64) <= S.case("5x6x2-wide", "lib").bar_mean
