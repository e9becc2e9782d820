"""ms per teacher training step (r2l_amd/teacher_train.py) at the lego configuration: 1024 rays, 64 + 128 samples, perturb 1,
and the same step as torch fp32 autograd of the oracle's functions on the same GPU.  Prints one JSON line.

  python tools/teacher_train_time.py [--rays 1024] [--steps 20] [--warmup 3]

FLOP model (DESIGN.md §teacher training): forward 1.187 MFLOP, dX chain ~1.12 MFLOP, dW 1.187 MFLOP per point; the fraction
is of the 157.3 TFLOP/s fp32-MFMA peak.  The per-kernel split comes from a separate run of this script under
`rocprofv3 --kernel-trace --stats -- python tools/teacher_train_time.py`."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import r2l_oracle as O  # noqa: E402

PEAK = 157.3e12
FLOP_PER_POINT = 1.187e6 + 1.12e6 + 1.187e6


def make(sd):
    from model.nerf_raybased import NeRF
    m = NeRF(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
    m.load_state_dict(sd)
    return m.cuda()


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no_baseline", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "teacher_train_time needs the GPU"
    from r2l_amd.teacher_train import TeacherTrainer
    csd, fsd = O.make_teacher_state_dicts(5, 2, alpha_bias=0.5)
    tr = TeacherTrainer(make(csd), make(fsd), perturb=1., white_bkgd=True)
    R = a.rays
    g = torch.Generator().manual_seed(0)
    o = (torch.randn(R, 3, generator=g) * .5).cuda()
    d = torch.randn(R, 3, generator=g).cuda()
    vd = d / d.norm(dim=-1, keepdim=True)
    tgt = torch.rand(R, 3, generator=g).cuda()
    ms = timed(lambda: (tr.forward_backward(o, d, vd, 2., 6., tgt), tr.adam(5e-4)), a.steps, a.warmup)
    pts = R * (64 + 64 + 128)
    out = {"rays": R, "points": pts, "ms_per_step": round(ms, 3),
           "fraction_of_fp32_mfma_peak": round(FLOP_PER_POINT * pts / (ms * 1e-3) / PEAK, 4),
           "ideal_ms": round(FLOP_PER_POINT * pts / PEAK * 1e3, 3)}
    if not a.no_baseline:
        sds = [{k: v.cuda().requires_grad_(True) for k, v in sd.items()} for sd in (csd, fsd)]
        opt = torch.optim.Adam([p for sd in sds for p in sd.values()], lr=5e-4)
        t = torch.linspace(0., 1., steps=64, device="cuda")

        def step():
            with torch.device("cuda"):  # the oracle builds its constants without a device argument
                z = (2. * (1. - t) + 6. * t).expand(R, 64)
                lo, up = O.stratified_bounds(z)
                z = lo + (up - lo) * torch.rand(R, 64)
                raw0 = O.run_network(sds[0], o[:, None] + d[:, None] * z[..., None], vd)
                rgb0, _, _, w0, _ = O.raw2outputs(raw0, z, d, None, True)
                zs = O.sample_pdf(.5 * (z[..., 1:] + z[..., :-1]), w0[..., 1:-1].detach(), 128, u=torch.rand(R, 128)).detach()
                za = torch.sort(torch.cat([z, zs], -1), -1)[0]
                raw = O.run_network(sds[1], o[:, None] + d[:, None] * za[..., None], vd)
                rgb = O.raw2outputs(raw, za, d, None, True)[0]
                loss = torch.mean((rgb - tgt)**2) + torch.mean((rgb0 - tgt)**2)
                opt.zero_grad()
                loss.backward()
                opt.step()
        out["torch_autograd_ms_per_step"] = round(timed(step, max(3, a.steps // 4), 2), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
