"""The SSIM yardstick of tests/ssim_util.py without a GPU: it reproduces the reference's own outputs (tests/golden/ssim.npz) and
the oracle, the numpy restatement of the kernel's sequence computes the reference's arithmetic and stays inside the bars the
device kernel is held to (tests/test_ssim_gpu.py), nine wrong evaluations each miss those bars on a named case, and the distance
of the reference's fp32 SSIM from fp64 on a flat bright background is pinned.

Every test prints the figures it asserts (pytest -s, lines starting with YARDSTICK ssim): profiles/ssim_yardstick.txt quotes
them."""
import os

import numpy as np
import pytest
import torch

from oracle import r2l_oracle as O
from tests import ssim_util as S
from tests.conftest import GOLDEN


def test_table_covers_the_shapes_kinds_and_windows():
    from r2l_amd import _lib
    n = _lib.load().r2l_ssim_partial_count
    kinds = {s: set() for s in S.SHAPES}
    for name in S.CASES:
        c = S.case(name)
        assert tuple(c.pred.shape) == tuple(c.gt.shape) == c.shape and c.pred.dtype == torch.float32
        assert c.t64.numel() == n(*c.shape) == c.bar_tile.numel() and (c.bar_tile > 0).all()
        kinds[c.shape].add(c.kind)
    assert all(len(k) >= 2 for k in kinds.values()), kinds
    assert set().union(*kinds.values()) == set(S.KINDS)
    assert max(h * w for h, w, _ in S.SHAPES) == 160 * 144
    # the only case in which the finish kernel's stride loop of 256 turns, with a ragged last turn
    assert n(160, 144, 3) == 270 and [s for s in S.SHAPES if n(*s) > 256] == [(160, 144, 3)]
    asym = [S.case(k) for k in S.CASES if k.endswith("-asym")]
    assert len(asym) == 2 and all(c.shape[0] != c.shape[1] for c in asym)


def test_windows():
    """The window the Python layer passes is the reference's own (golden file) bit for bit, and so is the one r2l_ssim builds for
    window_host = NULL, as restated; with the eleven values summed in fp32 in index order it is not (117 taps an ulp off).  The
    asymmetric window sums to 1 and differs from its transpose and from both flips."""
    gold = torch.from_numpy(np.load(os.path.join(GOLDEN, "ssim.npz"))["window"])
    assert torch.equal(S.window_ref(), gold) and torch.equal(O.ssim_window(), gold)
    assert torch.equal(S.window_lib(), gold)
    old = S._window_lib(True)
    S.report("window: NULL path restated with an in-order fp32 sum: %d taps differ from the reference's, sum %.9f against %.9f" % (
        (old != gold).sum().item(), old.double().sum().item(), gold.double().sum().item()))
    assert (old != gold).sum().item() > 100
    w = S.window_asym()
    assert w.dtype == torch.float32 and abs(w.double().sum().item() - 1) < 1e-6 and (w > 0).all()
    rel = lambda v: ((v - w).abs() / w).max().item()
    assert min(rel(w.t()), rel(w.flip(0)), rel(w.flip(1))) > 0.1
    ratio = w / S.window_ref()
    assert 0.45 < ratio.min().item() and ratio.max().item() < 1.6


def test_yardstick_reproduces_the_reference_outputs():
    """tiles64(ssim_map64) summed and divided by H W C against the reference's fp32 results at its three sizes."""
    g = np.load(os.path.join(GOLDEN, "ssim.npz"))
    win = torch.from_numpy(g["window"])
    for tag in "abc":  # 40x52, 7x9, 33x16
        pred, gt = torch.from_numpy(g["pred_" + tag]), torch.from_numpy(g["gt_" + tag])
        got = S.tiles64(S.ssim_map64(pred, gt, win)).sum().item() / pred.numel()
        S.report("golden %s %s: yardstick %.9f, reference %.9f, distance %.2e (bar 2e-6)" % (
            tag, tuple(pred.shape), got, float(g["ssim_" + tag]), abs(got - float(g["ssim_" + tag]))))
        assert abs(got - float(g["ssim_" + tag])) < 2e-6
        same = S.tiles64(S.ssim_map64(gt, gt, win)).sum().item() / gt.numel()
        assert abs(same - 1) < 1e-12 and abs(float(g["ssim_same_" + tag]) - 1) < 2e-6


@pytest.mark.parametrize("name", S.CASES)
def test_ref32_is_the_oracle_and_sets_the_bars(name):
    """ssim_map32_ref's mean against oracle.ssim (on the reference's window: the oracle takes no other), and the distances of the
    reference's own fp32 arithmetic from fp64 that the bars are made of."""
    c = S.case(name)
    mean = S.ssim_map32_ref(c.pred, c.gt, S.window_ref()).mean().item()
    want = O.ssim(c.pred, c.gt).item()
    S.report("%s: reference fp32 from fp64 worst tile %.2e, mean %.2e; bars tile %.2e .. %.2e, mean %.2e; ref32 - oracle %.1e" % (
        name, c.ref_tile, c.ref_mean, c.bar_tile.min().item(), c.bar_tile.max().item(), c.bar_mean, abs(mean - want)))
    assert abs(mean - want) <= 1e-6
    assert abs(c.t64.sum().item() / c.pred.numel() - c.map64.mean().item()) < 1e-12  # the tile table loses no pixel


@pytest.mark.parametrize("name", S.CASES)
def test_restatement_of_the_kernel(name):
    """ssim_map32_seq: on the flat and scene kinds at most 1e-6 per pixel from the reference's fp32 map (this is what lets it stand
    in for the reference's arithmetic on the device); on every case, summed in the kernel's own order, inside the bars the device
    kernel is held to."""
    c = S.case(name)
    seq = S.ssim_map32_seq(c.pred, c.gt, c.window)
    px = (seq - S.ssim_map32_ref(c.pred, c.gt, c.window)).abs().max().item()
    tiles = S.tiles32_butterfly(seq)
    r_tile, _ = S.worst_ratio(tiles, c.t64, c.bar_tile)
    r_mean = abs(S.finish32(tiles, c.pred.numel()) - c.mean64) / c.bar_mean
    line = "%s: restatement - reference fp32 per pixel %.2e; in the kernel's order: tile %.3f of its bar, mean %.3f" % (
        name, px, r_tile, r_mean)
    if c.kind in S.SEQ_KINDS:
        r_seq, _ = S.worst_ratio(tiles, c.seq_t, c.seq_bar)
        line += ", tile against the restatement's fp64 sum %.3f of that bar" % r_seq
        assert px <= 1e-6 and r_seq <= 1
    S.report(line)
    assert r_tile <= 1 and r_mean <= 1


# mutant -> (cases that must catch it, cases that cannot see it)
MUTANT_CASES = {
    "replicate_padding": (["160x144x3-tex", "5x6x2-wide"], []),
    "window_transposed": (["33x16x4-tex-asym", "47x21x3-wide-asym"], ["33x16x4-wide", "47x21x3-wide"]),
    # exchanging x and y in the partial INDEX alone changes nothing on a grid of one row or one column; (16, 33, 4) is 1 x 3 tiles
    # and sees the exchange in the tile origin, a grid with both sides > 1 sees the index
    "grid_origin_transposed": (["16x33x4-tex", "33x16x4-wide"], []),
    "grid_index_transposed": (["47x21x3-wide", "160x144x3-tex"], ["16x33x4-tex"]),
    "last_ragged_row_masked": (["17x15x3-wide", "17x15x3-flat", "17x15x3-scene97"], ["16x33x4-tex"]),
    "tap_row_10_dropped": (["15x17x3-tex", "160x144x3-tex", "17x15x3-wide"], ["1x1x1-tex", "5x6x2-wide"]),  # (H <= 5: row 10 is padding)
    "c1_c2_exchanged": (["31x32x5-dark", "11x11x1-dark", "16x16x1-dark", "1x1x1-dark"], []),
    "next_channel": (["5x6x2-wide", "31x32x5-tex", "16x33x4-tex"], ["16x16x1-dark"]),
    # the factor cancels between numerator and denominator except through C2: the mutant moves a pixel by about
    # (1/120) C2 (sig1 + sig2 - 2 sig12) / (sig1 + sig2 + C2)^2, which is largest where the variances are of C2's size (dark).  On
    # the small tex and wide cases it stays at 0.35 .. 1.9 bars: there the bars do not decide it, and those cases are not named
    "sample_variance": (["31x32x5-dark", "16x16x1-dark", "11x11x1-dark", "160x144x3-tex"], []),
}


def mutant_factor(c, mutant):
    """By how many times the worst tile of the mutated yardstick misses the case's bar, and that tile's entry."""
    if mutant in S.MAP_MUTANTS:
        t = S.tiles64(S.ssim_map64(c.pred, c.gt, c.window, mutant=mutant))
    else:
        t = S.tiles64(c.map64, mutant=mutant)
    return S.worst_ratio(t, c.t64, c.bar_tile)


@pytest.mark.parametrize("mutant", sorted(MUTANT_CASES))
def test_the_bars_see_the_mutant(mutant):
    seen, blind = MUTANT_CASES[mutant]
    for name in seen:
        f, k = mutant_factor(S.case(name), mutant)
        S.report("mutant %s on %s: worst tile (entry %d) misses its bar %.3g times" % (mutant, name, k, f))
        assert f > 1, (mutant, name, f)
    for name in blind:
        f, _ = mutant_factor(S.case(name), mutant)
        S.report("mutant %s on %s: invisible there (%.3g of the bar)" % (mutant, name, f))
        assert f == 0, (mutant, name, f)


def test_flat_frames_need_the_restatement_bar():
    """On a flat frame four times the reference's own distance from fp64 is 0.6 a tile: a dropped tap row stays under it.  The bar
    against the restatement, which the flat and scene kinds are held to as well, sees it."""
    c = S.case("160x144x3-flat")
    f64, _ = mutant_factor(c, "tap_row_10_dropped")
    w = c.window.clone()
    w[S.WIN - 1] = 0
    f_seq, _ = S.worst_ratio(S.tiles32_butterfly(S.ssim_map32_seq(c.pred, c.gt, w)), c.seq_t, c.seq_bar)
    S.report("mutant tap_row_10_dropped on 160x144x3-flat: %.3g of the fp64 bar, misses the restatement's bar %.3g times" % (f64, f_seq))
    assert f64 < 1 < f_seq


def test_replicate_padding_shows_in_border_tiles_only():
    c = S.case("160x144x3-tex")
    t = S.tiles64(S.ssim_map64(c.pred, c.gt, c.window, mutant="replicate_padding"))
    r = ((t - c.t64).abs() / c.bar_tile).view(3, 10, 9)
    assert r[:, 1:-1, 1:-1].max().item() == 0  # the window reaches 5 pixels, a tile has 16
    border = torch.cat([r[:, 0].reshape(-1), r[:, -1].reshape(-1), r[:, :, 0].reshape(-1), r[:, :, -1].reshape(-1)])
    S.report("mutant replicate_padding on 160x144x3-tex: border tiles miss their bars %.3g .. %.3g times, interior tiles 0" % (
        border.min().item(), border.max().item()))
    assert border.min().item() > 1


def test_the_frame_bar_sees_a_mean_over_hw():
    for name in ("15x17x3-tex", "5x6x2-wide", "160x144x3-flat"):
        c = S.case(name)
        H, W, C = c.shape
        wrong = c.t64.sum().item() / (H * W)
        f = abs(wrong - c.mean64) / c.bar_mean
        S.report("mutant mean_over_hw on %s: misses the frame bar %.3g times" % (name, f))
        assert f > 1


def test_white_background_finding():
    """The documentation's claim, not the kernel: on a white ground truth with a textured centre against a prediction whose
    background is flat at 0.97, 100 x 90 x 3, the reference's fp32 SSIM lies 1e-4 .. 1e-3 ABOVE its fp64 value (the fourth decimal
    of the TestSSIM the logs print); on the texture alone, seeded as tests/test_metrics_gpu.py seeds it (H + W), it is below 5e-7.
    (That figure moves with the seed: 6e-8 .. 6.5e-7 over eight seeds tried, always three orders below the scene's.)"""
    w = S.window_ref()
    c = S.build_case("scene", (100, 90, 3), "scene97", w, 97)
    d = S.ssim_map32_ref(c.pred, c.gt, w).double().mean().item() - c.mean64
    px = (S.ssim_map32_ref(c.pred, c.gt, w).double() - c.map64).abs().max().item()
    t = S.build_case("tex", (100, 90, 3), "tex", w, 100 + 90)
    S.report("finding 100x90x3: scene97 fp32 mean - fp64 mean %+.3e (fp64 %.6f), worst pixel %.2e, worst tile %.2e; tex %.2e" % (
        d, c.mean64, px, c.ref_tile, t.ref_mean))
    for kind, shape in (("scene97", (40, 52, 3)), ("scene995", (100, 90, 3)), ("flat", (100, 90, 3))):
        o = S.build_case(kind, shape, kind, w, 99)
        S.report("finding %s %s: fp32 mean from fp64 mean %.3e, worst tile %.2e" % (kind, shape, o.ref_mean, o.ref_tile))
    assert 1e-4 <= d <= 1e-3
    assert t.ref_mean < 5e-7
