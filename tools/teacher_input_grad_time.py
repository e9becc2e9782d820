"""Times of the teacher's backward to its rays on one GPU -> profiles/teacher_input_grad.txt.

    timeout -k 10 600 python tools/teacher_input_grad_time.py --samples 64 --out profiles/teacher_input_grad.txt && \\
    timeout -k 10 600 python tools/teacher_input_grad_time.py --samples 192 --append --out profiles/teacher_input_grad.txt

Each invocation is one process: its paths alternate within a round, three rounds, ms by device events, median and spread
(max - min) of the three.  --samples S (1024 rays): r2l_teacher_backward_input alone; r2l_teacher_backward (with its weight
gradients) on the same inputs; the forward with stash + r2l_teacher_backward_input; the torch route — fp32 autograd through the
op-by-op teacher from the same draw to the rays, forward included (autograd needs its own); and the whole
TeacherRayGrad.loss_and_grad at N_samples + N_importance = S (64: 64 + 0; 192: 64 + 128).  Init-distribution weights: the times do not depend on them."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from oracle import r2l_oracle as O  # noqa: E402
from r2l_amd import _lib, render  # noqa: E402
from r2l_amd import teacher_input_grad as TI  # noqa: E402
from r2l_amd._lib import ptr as _p, stream as _s  # noqa: E402
from r2l_amd.nerf_raybased import NeRF  # noqa: E402

R, ROUNDS, ITERS = 1024, 3, 10


def timed(fn, iters=ITERS):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def rounds(paths):
    """{name: [ms per round]}: the paths alternate within each round."""
    out = {k: [] for k in paths}
    for _ in range(ROUNDS):
        for k, fn in paths.items():
            out[k].append(timed(fn))
    return out


def line(name, v):
    return "    %-34s %s ms | median %.4f, spread %.4f" % (name, " ".join("%9.4f" % x for x in v), statistics.median(v), max(v) - min(v))


def module(sd):
    m = NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=4, skips=[4], use_viewdirs=True)
    m.load_state_dict(sd)
    return m.cuda()


def kernel_times(S):
    lib = _lib.load()
    sds = O.make_teacher_state_dicts(5, 2, alpha_bias=0.5)
    nets = [module(sd) for sd in sds]
    g = torch.Generator().manual_seed(S)
    o = (torch.randn(R, 3, generator=g) * 0.5).cuda()
    d = torch.randn(R, 3, generator=g).cuda()
    vd = d / d.norm(dim=-1, keepdim=True)
    z = torch.sort(torch.rand(R, S, generator=g) * 4 + 2, -1)[0].cuda()
    draw = (torch.randn(R, S, 4, generator=g) * 1e-3).cuda()
    tgt = torch.rand(R, 3, generator=g).cuda()
    ns, ni = (64, 0) if S == 64 else (64, S - 64)
    rg = TI.TeacherRayGrad(nets[0], nets[1] if ni else None, ns, ni, True)
    eng = rg.engines[0]
    eng.ensure_packed()
    P = R * S
    raw = torch.empty(P * 4, device="cuda")
    stash = torch.empty(lib.r2l_teacher_stash_floats(P), device="cuda")
    work = torch.empty(lib.r2l_teacher_input_grad_work_floats(P), device="cuda")
    work_t = torch.empty(lib.r2l_teacher_train_work_floats(P), device="cuda")
    grads = torch.empty(lib.r2l_teacher_param_count(), device="cuda")
    outs = [torch.empty(R, 3, device="cuda") for _ in range(3)]

    def fwd():
        _lib.check(lib.r2l_teacher_mlp_train(_p(o), _p(d), _p(vd), _p(z), _p(eng.wstream), _p(eng.flat), _p(raw), _p(stash), R, S, _s()),
                   "r2l_teacher_mlp_train")

    def bwd_in():
        _lib.check(lib.r2l_teacher_backward_input(_p(o), _p(d), _p(vd), _p(z), _p(eng.flat), _p(stash), _p(draw), None, 0, _p(outs[0]),
                                                  _p(outs[1]), _p(outs[2]), None, _p(work), R, S, _s()), "r2l_teacher_backward_input")

    def bwd_w():
        _lib.check(lib.r2l_teacher_backward(_p(o), _p(d), _p(vd), _p(z), _p(eng.flat), _p(stash), _p(draw), _p(grads), _p(work_t), R, S,
                                            _s()), "r2l_teacher_backward")

    embed, embeddirs = render.get_embedder(10)[0], render.get_embedder(4)[0]

    def torch_route():
        lo, ld, lv = [t.detach().clone().requires_grad_(True) for t in (o, d, vd)]
        pts = lo[:, None, :] + ld[:, None, :] * z[:, :, None]
        emb = torch.cat([embed(pts.reshape(-1, 3)), embeddirs(lv[:, None, :].expand(R, S, 3).reshape(-1, 3))], -1)
        nets[0](emb).backward(draw.view(-1, 4))

    fwd()
    t = rounds({"r2l_teacher_backward_input": bwd_in, "r2l_teacher_backward (with dW)": bwd_w,
                "forward with stash + backward_input": lambda: (fwd(), bwd_in()), "torch autograd, forward + backward": torch_route,
                "TeacherRayGrad.loss_and_grad %d+%d" % (ns, ni): lambda: rg.loss_and_grad(o, d, vd, 2., 6., tgt, fold_viewdirs=True)})
    lines = ["R %d, S %d (P = %d points)" % (R, S, P)] + [line(k, v) for k, v in t.items()]
    med = {k: statistics.median(v) for k, v in t.items()}
    lines.append("    r2l_teacher_backward / r2l_teacher_backward_input x%.2f; torch / (forward with stash + backward_input) x%.2f" % (
        med["r2l_teacher_backward (with dW)"] / med["r2l_teacher_backward_input"],
        med["torch autograd, forward + backward"] / med["forward with stash + backward_input"]))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=0)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default="profiles/teacher_input_grad.txt")
    a = ap.parse_args()
    lines = []
    if not a.append:
        lines.append("# tools/teacher_input_grad_time.py on %s, torch %s; one process per block, %d rounds of %d iterations alternating "
                     "the paths; ms per call by device events" % (torch.cuda.get_device_name(0), torch.__version__, ROUNDS, ITERS))
    if a.samples:
        lines += kernel_times(a.samples)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
