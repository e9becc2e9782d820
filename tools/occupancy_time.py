"""The teacher's per-pose render in ms per 400x400 frame with and without the occupancy grid (render(..., occupancy=pair)), in
ONE process: 64 + 128 samples, chunk 32 768, perturb 0, the tests' trained-like pair (tests/teacher_util.py: no lego teacher is at
hand), boxes +-1.6 (the fitted box) and +-2.5 (the drivers' default for the Blender scenes).  After a warm-up of each path, three
alternating rounds, device events around work that ends in a synchronise.  Also: the live share, the build time of the pair, the
kernel times of compact and scatter on one chunk, max |d RGB| and PSNR between the two frames, and the share of rays that carry
a skipped sample with sigma > 0 on the 2000 rays of tests/test_occupancy_gpu.py (test 5).

    python tools/occupancy_time.py --out profiles/occupancy.txt

--fused: the grids inside the fused frames call (render_frames(occupancy=pair), r2l_teacher_frames_occ_cfg) instead.  Same frame,
pair, grid and boxes; ms per frame of (a) render_frames without grids, (b) render_frames with the grids, (c) the per-pose path
above (render(..., occupancy=pair), chunk 32 768) and (d) render_frames with an ALL-EMPTY grid whose box holds every sample (the
floor: the capacity-sized grid of workgroups that leave at once, the index launches, the stages around the point network), three
rounds alternated a -> b -> c -> d; the live share of (b) from its device counters and the spread between rounds.

    python tools/occupancy_time.py --fused --out profiles/occupancy_fused.txt

--ert: early ray termination in the last pass of the fused frames call (render_frames(ert=(eps, seg)), r2l_teacher_frames_ert_cfg).
Same frame, pair and boxes, chunk 32 768; ms per frame of (a) the grids alone (r2l_teacher_frames_occ_cfg: the baseline), (b) grids +
termination at eps 1e-3 with seg 16, 32, 64, (c) termination without grids, seg 32, next to the frame without either, (d) grids +
termination with seg 256: one segment, nothing terminated — the cost of the mechanism; three rounds alternated over all paths.  The
live shares from the device counters, PSNR and max |d RGB| of (b) against (a), and r2l_ert_advance / r2l_occ_index_seg alone on one
chunk's fine pass (32 768 rays x 192 samples, one segment of 32).

    python tools/occupancy_time.py --ert --out profiles/ert.txt
"""
import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import r2l_oracle as O  # noqa: E402
from r2l_amd import engine, occupancy as OC, render  # noqa: E402
from r2l_amd.nerf_raybased import NeRF  # noqa: E402
from tests.teacher_util import scene_rays, trained_like_pair  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def fused_report(a, nets, H, W, focal, c2w, dev):
    """The lines of --fused (see the module docstring)."""
    import numpy as np
    med = lambda v: sorted(v)[len(v) // 2]
    kw = dict(chunk=32768, c2w=c2w, ndc=False, near=2., far=6., use_viewdirs=True, network_fn=nets[0], network_fine=nets[1],
              network_query_fn=None, N_samples=64, N_importance=128, perturb=0., white_bkgd=True)
    per_pose = lambda occ: render.render(H, W, focal, occupancy=occ, **kw)[0]
    frames = lambda occ, acc=None: render.render_frames(c2w[None], H, W, focal, 2., 6., nets[0], nets[1], 64, 128, 0., True, seed=0,
                                                        occupancy=occ, live_acc=acc)["rgb"]
    lines = ["teacher frames, %d x %d, 64+128 samples, perturb 0, precision %s (%s), trained-like pair of tests/teacher_util.py, %s"
             % (H, W, a.precision, engine.arithmetic(render.teacher_engine(nets[0]).cfg)["precision"], torch.cuda.get_device_name(0)),
             "grid %d^3 cells x 2 probes per cell and axis x dilation 1; ms/frame by device events, one process, rounds alternated a -> b -> c -> d" % a.res,
             "(a) render_frames, no grids   (b) render_frames(occupancy=pair): a whole frame per pass, no host read",
             "(c) render(occupancy=pair) per pose, chunk 32768: a host read of the live count per pass   (d) render_frames, all-empty grid "
             "over +-16: every sample inside and skipped"]
    with torch.no_grad():
        empty = OC.OccupancyGrid([-16.] * 3, [16.] * 3, G=a.res, k=1, dilate=0).set_bits(np.zeros(OC.n_words(a.res), np.uint32), device=dev)
        for box in (1.6, 2.5):
            pair = tuple(OC.OccupancyGrid([-box] * 3, [box] * 3, G=a.res).build(n) for n in nets)
            acc, acc_d = (torch.zeros(2, dtype=torch.int64, device=dev) for _ in range(2))
            paths = {"a": lambda: frames(None), "b": lambda: frames(pair, acc), "c": lambda: per_pose(pair),
                     "d": lambda: frames((empty, empty), acc_d)}
            for fn in paths.values():
                fn()  # warm-up: weight packing, allocator, work buffers
            acc.zero_()
            acc_d.zero_()
            ms, out = {k: [] for k in paths}, {}
            for _ in range(a.rounds):
                for k, fn in paths.items():
                    t, out[k] = timed(fn)
                    ms[k].append(t)
            live, total = (int(x) for x in acc.tolist())
            share = live / max(total, 1)
            lines.append("box +-%.1f: occupied cells %.1f %% (coarse net) / %.1f %% (fine net)" %
                         (box, 100 * pair[0].occupied_share(), 100 * pair[1].occupied_share()))
            for k, v in ms.items():
                lines.append("  (%s) %s   median %.2f, spread %.2f" % (k, "  ".join("%.2f" % x for x in v), med(v), max(v) - min(v)))
            spread = max(max(v) - min(v) for v in ms.values())
            lines.append("  live points of (b) %.1f %% (%d / %d over %d frames); (d) live %d" %
                         (100 * share, live, total, a.rounds, int(acc_d[0])))
            lines.append("  (b) / (a) %.3f; (b) - (c) %+.2f ms (largest spread of a path %.2f ms); live share x (a) + (d) = %.2f ms against (b) %.2f ms"
                         % (med(ms["b"]) / med(ms["a"]), med(ms["b"]) - med(ms["c"]), spread, share * med(ms["a"]) + med(ms["d"]), med(ms["b"])))
            lines.append("  max |rgb(b) - rgb(c)| %.3e (the per-pose path forms its own rays), max |rgb(b) - rgb(a)| %.3e; (d) is the "
                         "background: %s" % (float((out["b"].reshape(-1, 3) - out["c"].reshape(-1, 3)).abs().max()),
                                             float((out["b"] - out["a"]).abs().max()), bool((out["d"] == 1.).all())))
    return lines


def ert_report(a, nets, H, W, focal, c2w, dev):
    """The lines of --ert (see the module docstring)."""
    from r2l_amd import _lib, ert as E
    med = lambda v: sorted(v)[len(v) // 2]
    EPS = 1e-3

    def frames(occ, ert, acc):
        return render.render_frames(c2w[None], H, W, focal, 2., 6., nets[0], nets[1], 64, 128, 0., True, seed=0, chunk=32768,
                                    occupancy=occ, live_acc=acc, ert=ert)["rgb"]

    lines = ["teacher frames, %d x %d, 64+128 samples, chunk 32768, perturb 0, precision %s (%s), trained-like pair of tests/teacher_util.py, %s"
             % (H, W, a.precision, engine.arithmetic(render.teacher_engine(nets[0]).cfg)["precision"], torch.cuda.get_device_name(0)),
             "grid %d^3 cells x 2 probes per cell and axis x dilation 1; eps %g; ms/frame by device events, one process, rounds alternated "
             "over all paths" % (a.res, EPS),
             "(a) grids only (the baseline)   (b16/b32/b64) grids + early termination, seg 16 / 32 / 64   (c) early termination without "
             "grids, seg 32   (n) neither   (d) grids + early termination, seg 256: one segment, nothing terminated",
             "The scene is analytic: an opaque shell at r = 1 stops every ray that meets it, so the gain below is NOT that of a published scene."]
    with torch.no_grad():
        for box in (1.6, 2.5):
            pair = tuple(OC.OccupancyGrid([-box] * 3, [box] * 3, G=a.res).build(n) for n in nets)
            accs = {k: torch.zeros(2, dtype=torch.int64, device=dev) for k in ("a", "b16", "b32", "b64", "c", "d")}
            paths = {"a": lambda: frames(pair, None, accs["a"]), "b16": lambda: frames(pair, (EPS, 16), accs["b16"]),
                     "b32": lambda: frames(pair, (EPS, 32), accs["b32"]), "b64": lambda: frames(pair, (EPS, 64), accs["b64"]),
                     "c": lambda: frames(None, (EPS, 32), accs["c"]), "n": lambda: frames(None, None, None),
                     "d": lambda: frames(pair, (EPS, 256), accs["d"])}
            for fn in paths.values():
                fn()  # warm-up
            for t in accs.values():
                t.zero_()
            ms, out = {k: [] for k in paths}, {}
            for _ in range(a.rounds):
                for k, fn in paths.items():
                    t, out[k] = timed(fn)
                    ms[k].append(t)
            lines.append("box +-%.1f: occupied cells %.1f %% (coarse net) / %.1f %% (fine net)" %
                         (box, 100 * pair[0].occupied_share(), 100 * pair[1].occupied_share()))
            for k, v in ms.items():
                share = ""
                if k in accs:
                    live, total = (int(x) for x in accs[k].tolist())
                    share = "; live points %.1f %% (%d / %d)" % (100. * live / max(total, 1), live, total)
                lines.append("  (%-3s) %s   median %.2f, spread %.2f%s" % (k, "  ".join("%.2f" % x for x in v), med(v), max(v) - min(v), share))
            for k in ("b16", "b32", "b64"):
                diff = (out[k] - out["a"]).abs()
                mse = float((diff.double()**2).mean())
                lines.append("  (%s) / (a) %.3f; max |d RGB| against (a) %.3e, PSNR %s dB" %
                             (k, med(ms[k]) / med(ms["a"]), float(diff.max()), "inf" if mse == 0 else "%.2f" % (-10. * math.log10(mse))))
            lines.append("  (c) / (n) %.3f; (d) - (a) %+.2f ms (the extra launches with nothing terminated); (d) equals (a) bit for bit: %s" %
                         (med(ms["c"]) / med(ms["n"]), med(ms["d"]) - med(ms["a"]), bool(torch.equal(out["d"], out["a"]))))
        # the two new kernels alone, on the fine pass of one chunk
        rays = scene_rays(H * W, 0, H=H, W=W, focal=focal)[::max(H * W // 32768, 1)][:32768].to(dev)
        o, d, vd = rays[:, 0:3].contiguous(), rays[:, 3:6].contiguous(), rays[:, 8:11].contiguous()
        n = rays.shape[0]
        z = torch.linspace(2., 6., 192, device=dev).expand(n, 192).contiguous()
        raw = render.teacher_engine(nets[1]).mlp(o, d, vd, z)
        trans = torch.empty(n, device=dev)
        idx = torch.empty(n * 32, dtype=torch.int64, device=dev)
        cnt = torch.empty(1, dtype=torch.int64, device=dev)
        work = torch.empty(max(_lib.load().r2l_occ_index_seg_work_bytes(n * 32), 16), dtype=torch.uint8, device=dev)
        E.advance(raw, z, d, 0, 64, trans)
        ta = [timed(lambda: E.advance(raw, z, d, 64, 96, trans))[0] for _ in range(5)]
        ti = [timed(lambda: E.index_seg(pair[1], o, d, z, 96, 128, trans, EPS, idx, cnt, work))[0] for _ in range(5)]
        tn = [timed(lambda: E.index_seg(None, o, d, z, 96, 128, trans, EPS, idx, cnt, work))[0] for _ in range(5)]
        lines.append("one chunk's fine pass (%d rays x 192 samples), one segment of 32: r2l_ert_advance %.3f ms, r2l_occ_index_seg %.3f ms with "
                     "the grid, %.3f ms without (3 launches; %d of %d live; medians of 5)" % (n, med(ta), med(ti), med(tn), int(cnt[0]), n * 32))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=400)
    ap.add_argument("--res", type=int, default=128, help="cells per axis")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--precision", default="auto", choices=["auto", "fp16x2", "bf16x3", "fp32_mfma"])
    ap.add_argument("--out", default="")
    ap.add_argument("--fused", action="store_true", help="time the grids inside the fused frames call (profiles/occupancy_fused.txt)")
    ap.add_argument("--ert", action="store_true", help="time early ray termination in the fused frames call (profiles/ert.txt)")
    a = ap.parse_args()
    dev = "cuda:0"
    nets = []
    for sd in trained_like_pair():
        m = NeRF(D=8, W=256, input_ch=63, output_ch=4, skips=[4], input_ch_views=27, use_viewdirs=True)
        m.load_state_dict(sd)
        for p in m.parameters():
            p.requires_grad = False
        m = m.to(dev).eval()
        render.teacher_engine(m).set_config(precision=a.precision)
        nets.append(m)
    H = W = a.size
    focal = 555.5555155968841 * a.size / 400.
    c2w = torch.from_numpy(O.pose_spherical(35., -25., 4.)[:3, :4]).to(dev)
    if a.fused or a.ert:
        text = "\n".join((ert_report if a.ert else fused_report)(a, nets, H, W, focal, c2w, dev))
        print(text)
        if a.out:
            with open(os.path.abspath(a.out), "w") as f:
                f.write(text + "\n")
        return
    kw = dict(chunk=32768, c2w=c2w, ndc=False, near=2., far=6., use_viewdirs=True, network_fn=nets[0], network_fine=nets[1],
              network_query_fn=None, N_samples=64, N_importance=128, perturb=0., white_bkgd=True)
    frame = lambda occ: render.render(H, W, focal, occupancy=occ, **kw)[0]
    med = lambda v: sorted(v)[len(v) // 2]
    lines = ["teacher render(), %d x %d, 64+128 samples, chunk 32768, perturb 0, precision %s (%s), trained-like pair of tests/teacher_util.py, %s"
             % (H, W, a.precision, engine.arithmetic(render.teacher_engine(nets[0]).cfg)["precision"], torch.cuda.get_device_name(0)),
             "grid %d^3 cells x 2 probes per cell and axis x dilation 1; ms/frame by device events, rounds alternated full -> skipped" % a.res]
    with torch.no_grad():
        for box in (1.6, 2.5):
            pair = tuple(OC.OccupancyGrid([-box] * 3, [box] * 3, G=a.res).build(n) for n in nets)
            build_ms = [g.build_seconds * 1e3 for g in pair]
            for occ in (None, pair):
                frame(occ)  # warm-up: weight packing, allocator, the grids' buffers
            for g in pair:
                g.reset_counters()
            ms = {"full": [], "skipped": []}
            for _ in range(a.rounds):
                t, full = timed(lambda: frame(None))
                ms["full"].append(t)
                t, skip = timed(lambda: frame(pair))
                ms["skipped"].append(t)
            live = sum(g.live_points for g in pair) / sum(g.total_points for g in pair)
            diff = (full - skip).abs()
            mse = float((diff.double()**2).mean())
            # compact and scatter alone, on the fine pass of one chunk (32 768 rays x 192 samples)
            rays = scene_rays(H * W, 0, H=H, W=W, focal=focal)[::max(H * W // 32768, 1)][:32768].to(dev)  # spread over the frame
            o, d, vd = rays[:, 0:3].contiguous(), rays[:, 3:6].contiguous(), rays[:, 8:11].contiguous()
            n = rays.shape[0]
            z = torch.linspace(2., 6., 192, device=dev).expand(n, 192).contiguous()
            pair[1].compact(o, d, vd, z)
            tc = [timed(lambda: pair[1].compact(o, d, vd, z)) for _ in range(5)]
            M, idx = tc[-1][1][0], tc[-1][1][1]
            raw_live = torch.randn(M, 4, device=dev)
            ts = [timed(lambda: OC.OccupancyGrid.scatter(raw_live, idx, n, 192))[0] for _ in range(5)]
            lines.append("box +-%.1f: occupied cells %.1f %% (coarse net) / %.1f %% (fine net); build %.0f + %.0f ms (wall, %d probes each)"
                         % (box, 100 * pair[0].occupied_share(), 100 * pair[1].occupied_share(), build_ms[0], build_ms[1], (2 * a.res)**3))
            for k, v in ms.items():
                lines.append("  %-8s %s   median %.2f, spread %.2f" % (k, "  ".join("%.2f" % x for x in v), med(v), max(v) - min(v)))
            lines.append("  skipped / full %.3f (medians); live points %.1f %% of %d per frame" %
                         (med(ms["skipped"]) / med(ms["full"]), 100 * live, H * W * 256))
            lines.append("  max |d RGB| %.3e, PSNR between the frames %s dB" %
                         (float(diff.max()), "inf" if mse == 0 else "%.2f" % (-10. * math.log10(mse))))
            lines.append("  one chunk's fine pass (%d x 192 samples, %d live): compact (3 launches + the 8-byte read) %.3f ms, scatter "
                         "(memset + 1 launch) %.3f ms (medians of 5)" % (n, M, med([t for t, _ in tc]), med(ts)))
            if box == 1.6 and a.res >= 64:
                g64 = pair if a.res == 64 else tuple(OC.OccupancyGrid([-box] * 3, [box] * 3, G=64).build(n) for n in nets)
                spread = scene_rays(181 * 181, 0)[::181 * 181 // 2000][:2000].contiguous().to(dev)  # test 5's rays
                rep = OC.miss_report(spread, nets[0], nets[1], g64, 64, 128)
                n_miss = int((rep["misses"] > 0).sum())
                drgb = (rep["skip"]["rgb"].double() - rep["full"]["rgb"].double()).abs().amax(-1)
                lines.append("  tests/test_occupancy_gpu.py test 5 (2000 rays, grid 64^3 x 2 x dilation 1): %d rays (%.2f %%) carry a skipped "
                             "sample with sigma > 0; largest |d RGB| among them %.3e" % (n_miss, n_miss / 20., float(drgb.max())))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(os.path.abspath(a.out), "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
