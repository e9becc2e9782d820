"""What the student's input gradient costs (r2l_backward_input, csrc/r2l_input_grad.hip), on one GPU, in one process, after
warm-up: W256 D88, 4096 / 12 288 / 98 304 rays, perturb 1.

  call-rays   r2l_backward_input alone, ray form (d_rays_o, d_rays_d; the [N,1008] product stays in the workgroup)
  call-emb    r2l_backward_input alone, d_emb only
  torch       the op-by-op route on the same GPU, the yardstick: gh @ Wh by torch.matmul in fp32, then torch autograd through
              PointSampler.sample_train and PositionalEmbedder (their forward included: autograd needs it)
  bwd         the whole R2LRaysFunction backward, parameters trainable, rays plain: dX chain + weight gradients
  bwd+input   the same with rays that require grad: + r2l_backward_input

alternately for `--rounds` rounds; device events around every timed piece (the forward of a backward is not timed), summed over
the iterations of a round.  Reported: every round, the medians, the spread between the runs of the same path, and the FLOP model
of the GEMM (2 * 256 * 1008 per ray) against the fp32 matrix peak of 157.3 TF.

`python tools/input_grad_time.py --out profiles/input_grad.txt`"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from r2l_amd import _lib  # noqa: E402
from r2l_amd.autograd import R2LRaysFunction  # noqa: E402
from r2l_amd.engine import _ptr, _stream  # noqa: E402

PEAK_F32 = 157.3e12
PATHS = ("call-rays", "call-emb", "torch", "bwd", "bwd+input")


def timed(fn, n_iter, setup=None):
    """ms per call of fn by device events; setup() runs untimed in front of every call."""
    total = 0.
    for _ in range(n_iter):
        arg = setup() if setup is not None else None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(arg)
        e1.record()
        e1.synchronize()
        total += e0.elapsed_time(e1)
    return total / n_iter


def time_size(n, model, ps, rounds, say):
    from model.nerf_raybased import PositionalEmbedder
    eng = model.engine()
    eng.ensure_packed()  # (the engine has a device, and its depth table lands there, only from here on)
    g = torch.Generator().manual_seed(n)
    o = (torch.randn(n, 3, generator=g) * 0.3 + torch.tensor([0., 0., 4.])).cuda()
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1).cuda()
    u = torch.rand(n, 16, generator=g).cuda()
    drgb = (torch.randn(n, 3, generator=g) * 1e-3).cuda()
    params = list(model.parameters())
    pe = PositionalEmbedder(10, device="cuda")
    ztab = eng.ztab(ps.z_vals, 1.)

    # a gx as a step leaves it: one backward through the function, its gx kept by a hook on the engine's call
    kept = {}
    inner = eng.backward_input
    eng.backward_input = lambda gx, *a, **k: (kept.__setitem__("gx", gx), inner(gx, *a, **k))[1]
    graph = lambda grad_rays: R2LRaysFunction.apply(model, o.clone().requires_grad_(grad_rays), d.clone().requires_grad_(grad_rays),
                                                    u, ps.z_vals, 1., *params)
    (graph(True) * drgb).sum().backward()
    eng.backward_input = inner
    gx = kept["gx"]
    gh = gx[:n * 256].view(n, 256)
    Wh = model.head[0].weight.detach()
    lib = eng.lib
    d_emb, d_o, d_d = torch.empty(n, 1008, device="cuda"), torch.empty(n, 3, device="cuda"), torch.empty(n, 3, device="cuda")

    def call(emb, rays):
        _lib.check(lib.r2l_backward_input(_ptr(gx), _ptr(eng.flat), eng.n_block, _ptr(o), _ptr(d), _ptr(u), _ptr(ztab),
                                          _ptr(d_emb) if emb else None, _ptr(d_o) if rays else None, _ptr(d_d) if rays else None, n,
                                          _stream()), "r2l_backward_input")

    def torch_route(_):
        o_, d_ = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
        emb = pe(ps.sample_train(o_, d_, 1., u))
        emb.backward(torch.matmul(gh, Wh))

    def backward(rgb):
        (rgb * drgb).sum().backward()
        for p in params:
            p.grad = None

    runs = {"call-rays": (lambda _: call(False, True), None, 50), "call-emb": (lambda _: call(True, False), None, 50),
            "torch": (torch_route, None, 20), "bwd": (backward, lambda: graph(False), 8), "bwd+input": (backward, lambda: graph(True), 8)}
    got = {k: [] for k in PATHS}
    for k in PATHS:  # warm up every path at this size
        timed(runs[k][0], 3, runs[k][1])
    print("N %d: warm-up done" % n, flush=True)
    for _ in range(rounds):
        for k in PATHS:
            fn, setup, n_iter = runs[k]
            got[k].append(timed(fn, n_iter, setup))
    med = {k: float(np.median(v)) for k, v in got.items()}
    model_ms = 2. * 256 * 1008 * n / PEAK_F32 * 1e3
    say("N %6d | FLOP model of the GEMM %.4f ms" % (n, model_ms))
    for k in PATHS:
        say("    %-10s %s ms | median %.4f, spread %.4f" % (k, " ".join("%8.4f" % v for v in got[k]), med[k], max(got[k]) - min(got[k])))
    say("    call-rays is %.1f %% of the fp32 matrix peak by the GEMM's FLOP model; torch / call-rays x%.2f; input gradient in the "
        "backward %+.4f ms (%+.2f %%)" % (100. * model_ms / med["call-rays"], med["torch"] / med["call-rays"],
                                          med["bwd+input"] - med["bwd"], 100. * (med["bwd+input"] / med["bwd"] - 1.)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", default="4096,12288,98304")
    ap.add_argument("--n_block", type=int, default=43)
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    from model.nerf_raybased import PointSampler
    from oracle import r2l_oracle as O
    from tests.test_forward_gpu import build_model
    say("# tools/input_grad_time.py on %s, torch %s; one process, %d rounds alternating the paths; device events, ms per call" %
        (torch.cuda.get_device_name(0), torch.__version__, a.rounds))
    say("# W256 D%d, default arithmetic, perturb 1" % (2 * a.n_block + 2))
    model = build_model(O.make_state_dict(n_block=a.n_block, seed=0), a.n_block)
    ps = PointSampler(400, 400, 555.5555155968841, 16, 2., 6.)
    for n in [int(v) for v in a.sizes.split(",")]:
        time_size(n, model, ps, a.rounds, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
