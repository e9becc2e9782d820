"""Hashes of what the library computes, one line per launch shape, for comparing two builds of the library bit for bit:
    R2L_LIB_PATH=<a>/libr2l_hip.so python tools/grad_hash.py ; python tools/grad_hash.py   (GPU box)
Rows: one training step (rgb, loss, flat gradient) per (precision, dw_mode, ray count); then what the host-side dispatch queries
cannot see — forward-only rays, one-frame / two-frame pose launches, the pre-embedded forward (bf16x3) and training step, a staged
step (r2l_backward_part in buckets, reserve_cus = 8), the teacher's point network per precision, and two steps driven by the
process environment (R2L_NO_DW2=1, R2L_FORCE_VARIANT=coop16), each in a fresh child process."""
import hashlib
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from r2l_amd.train_step import R2LTrainer  # noqa: E402

dev = torch.device("cuda", 0)
ENV_ROWS = {"no_dw2": {"R2L_NO_DW2": "1"}, "coop16": {"R2L_FORCE_VARIANT": "coop16"}}


def digest(*tensors):
    h = hashlib.sha1()
    for t in tensors:
        h.update(t.detach().float().cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def batch(n):
    g = torch.Generator().manual_seed(n)
    o = (torch.randn(n, 3, generator=g) * 0.3 + torch.tensor([0., 0., 4.])).to(dev)
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1).to(dev)
    tgt = torch.rand(n, 3, generator=g).to(dev)
    u = torch.rand(n, 16, generator=g).to(dev)
    return o, d, tgt, u


def step(label, n, staged=False, **cfg):
    net, ps, _ = bench.make_model(dev)
    o, d, tgt, u = batch(n)
    tr = R2LTrainer(net, ps)
    tr.eng.set_config(**cfg)
    tr.force_staged = staged
    rgb = tr.forward_backward(o, d, tgt, perturb=1., t_rand=u)
    torch.cuda.synchronize()
    print("%-28s %6d rays  %s" % (label, n, digest(rgb, tr.loss_out, tr.grads)), flush=True)


def forward_rows():
    net, ps, _ = bench.make_model(dev)
    from r2l_amd.engine import get_engine
    eng = get_engine(net)
    for n in (4096, 160000):
        o, d, _, u = batch(n)
        print("%-28s %6d rays  %s" % ("forward rays", n, digest(eng.forward_rays(o, d, ps.z_vals, 1., u))), flush=True)
    c2w = torch.tensor([[[1., 0., 0., 0.1], [0., 1., 0., -0.2], [0., 0., 1., 4.0]],
                        [[0.8, 0., 0.6, 0.5], [0., 1., 0., 0.3], [-0.6, 0., 0.8, 3.5]]])
    print("%-28s %6d rays  %s" % ("forward pose (1 frame)", 200 * 200, digest(eng.forward_pose(c2w[0], 200, 200, 277.7, ps.z_vals))), flush=True)
    print("%-28s %6d rays  %s" % ("forward poses (2 frames)", 2 * 200 * 200, digest(eng.forward_poses(c2w, 200, 200, 277.7, ps.z_vals))), flush=True)
    # module-boundary path: the encoding given by the caller
    from r2l_amd.autograd import R2LEmbFunction
    n = 4096
    g = torch.Generator().manual_seed(7)
    emb = (torch.rand(n, 1008, generator=g) * 2 - 1).to(dev)
    tgt = torch.rand(n, 3, generator=g).to(dev)
    eng.set_config(precision="bf16x3")
    print("%-28s %6d rays  %s" % ("forward emb bf16x3", n, digest(eng.forward_emb(emb))), flush=True)
    for prec in ("auto", "fp32_mfma"):
        eng.set_config(precision=prec)
        params = list(eng.params)
        for p in params:
            p.grad = None
        rgb = R2LEmbFunction.apply(net, emb, *params)
        ((rgb - tgt) ** 2).mean().backward()
        torch.cuda.synchronize()
        print("%-28s %6d rays  %s" % ("emb step %s" % prec, n, digest(rgb, *[p.grad for p in params])), flush=True)


def teacher_rows():
    from model.nerf_raybased import NeRF
    from r2l_amd.render import teacher_engine
    torch.manual_seed(0)
    m = NeRF(D=8, W=256, input_ch=63, output_ch=4, skips=[4], input_ch_views=27, use_viewdirs=True).to(dev)
    R, S = 2048, 64
    o, d, _, _ = batch(R)
    g = torch.Generator().manual_seed(3)
    z = (2. + 4. * torch.rand(R, S, generator=g).sort(-1).values).to(dev)
    for prec in ("auto", "fp16x2", "bf16x3", "fp32_mfma"):
        te = teacher_engine(m)
        te.set_config(precision=prec)
        print("%-28s %6d pts   %s" % ("teacher mlp %s" % prec, R * S, digest(te.mlp(o, d, d, z))), flush=True)


if len(sys.argv) == 3 and sys.argv[1] == "--env-row":  # child: the switches are process environment
    for n in (4096, 40000):
        step("env " + " ".join("%s=%s" % kv for kv in ENV_ROWS[sys.argv[2]].items()), n)
    sys.exit(0)

for prec, dw in (("fp32_mfma", "auto"), ("fp16x2", "fp16"), ("fp16x2", "exact"), ("bf16x3", "auto")):
    for n in (4096, 12288 - 5, 40000, 98304):
        step("%-10s dw %-5s" % (prec, dw), n, precision=prec, dw_mode=dw)
forward_rows()
step("staged, reserve_cus 8", 4096, staged=True, reserve_cus=8)
step("staged, reserve_cus 8", 40000, staged=True, reserve_cus=8)
teacher_rows()
for name, switches in ENV_ROWS.items():
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--env-row", name], env=dict(os.environ, **switches),
                       stdout=subprocess.PIPE, text=True, timeout=600)
    sys.stdout.write(r.stdout)
    sys.stdout.flush()
    if r.returncode != 0:
        sys.exit("environment row %s failed with status %d" % (name, r.returncode))
