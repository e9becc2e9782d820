"""Data-parallel training step with TWO ranks.  On a box with >= 2 GPUs: one GPU per rank and the nccl (= RCCL) backend — the
production path, which the 1-GPU leases of the build could never run (fires the first time a node appears).  On
the one GPU a test box usually has: both ranks on it (RCCL refuses two ranks on one device, so the process group is gloo,
which all-reduces CUDA tensors through the host).  Either way the real R2LTrainer path of world_size > 1 —
replica sync from rank 0, staged backward (r2l_backward_part), bucketed gradient all-reduce submitted as the buckets finish,
Adam with grad_scale 1/world — against the single-process oracle on the FULL batch (reference: nn.DataParallel splitting
one batch over the GPUs, /root/reference/main.py:472-479, 1374-1406)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r"""
import os, sys, torch
sys.path.insert(0, %(root)r)
import torch.distributed as dist
from oracle import r2l_oracle as O
from tests.test_forward_gpu import build_model
from model.nerf_raybased import PointSampler
from r2l_amd.train_step import R2LTrainer, lr_schedule
from r2l_amd.dist_utils import bucket_plan, parameters_in_sync
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
multi = torch.cuda.device_count() >= world             # one GPU per rank: RCCL over xGMI; else both ranks share GPU 0 (gloo)
torch.cuda.set_device(rank if multi else 0)
if multi:
    dist.init_process_group("nccl", device_id=torch.device("cuda", rank))
else:
    dist.init_process_group("gloo")
variant = os.environ["R2L_FORCE_VARIANT"]
segments = int(os.environ.get("R2L_TEST_SEGMENTS", "1"))
nb = 3
sd0 = O.make_state_dict(n_block=nb, seed=40)           # what rank 0 builds
sd = O.make_state_dict(n_block=nb, seed=40 + rank)     # every rank builds ITS OWN weights ...
m = build_model(sd, nb)
ps = PointSampler(400, 400, 555.5555155968841, 16, 2., 6.)
tr = R2LTrainer(m, ps, chain_segments=segments)        # ... and continues with rank 0's
assert tr.world() == 2 and tr.n_buckets == 4 and tr.eng.cfg.reserve_cus == 8 and "R2L_RESERVE_CUS" not in os.environ
assert parameters_in_sync(tr.eng.flat)
assert torch.equal(m.state_dict()["body.1.body.0.weight"].cpu(), sd0["body.1.body.0.weight"])
g = torch.Generator().manual_seed(3)
n = 2 * (5000 if variant == "main" else 4096 if variant == "coopf" else 1024)
o = torch.randn(n, 3, generator=g) * 0.3 + torch.tensor([0., 0., 4.])
d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
tgt = torch.rand(n, 3, generator=g)
uneven = os.environ.get("R2L_TEST_UNEVEN") == "1"   # ranks take 5/8 and 3/8 of the batch (--N_rand not divisible by world)
cut = [0, n * 5 // 8, n] if uneven else [0, n // 2, n]
sl = slice(cut[rank], cut[rank + 1])
emb = O.positional_embed(O.sample_train(o, d, O.z_vals(16, 2., 6.), 0.), 10)
ref = {k: v.clone() for k, v in sd0.items()}
mo = {k: torch.zeros_like(v) for k, v in ref.items()}
vo = {k: torch.zeros_like(v) for k, v in ref.items()}
for step in (1, 2, 3):
    lr = lr_schedule(step, 5e-4, 500, "0.0001,200")
    loss, _, gr = O.r2l_loss_and_grads(ref, emb, tgt)   # ONE process, the full batch
    for k in ref:
        ref[k], mo[k], vo[k] = O.adam_step(ref[k], gr[k], mo[k], vo[k], step, lr)
    tr.forward_backward(o[sl].cuda(), d[sl].cuda(), tgt[sl].cuda(),
                        n_global=[cut[1] - cut[0], cut[2] - cut[1]] if uneven else None)  # every rank's ray count
    if segments > 1:
        # opt-in for small steps of the default trio: the dX chain in 3 segments, each segment's weight gradients and
        # all-reduce on a second stream beside the next segment; + the head bucket + the step-validity word (MAX)
        assert tr.chain_segments == 3 and tr._guard is not None and tr.reducer.pending() == 3 + 1 + 1
    else:
        assert tr.chain_segments == 1 and tr._guard is None  # the default at every world size (ADVICE r3)
        assert tr.reducer.pending() == len(bucket_plan(nb, tr.n_buckets)) == 4   # 3 body buckets (one per block) + the head, in flight until Adam needs them
    tr.allreduce_grads()
    assert tr.reducer.pending() == 0
    tr.adam(lr)
    # ray-share-weighted mean of the two ranks' losses == the full-batch loss
    lo = tr.loss_out[:1].clone() * (cut[rank + 1] - cut[rank]) / n
    dist.all_reduce(lo)
    assert abs(lo.item() - loss.item()) < 2e-6, (step, lo.item(), loss.item())
    assert parameters_in_sync(tr.eng.flat), step
assert tr.drain() == 0 and not tr.segments_disabled
new = m.state_dict()
worst, cos = 0., 1.
for k in ref:
    worst = max(worst, (new[k].cpu() - ref[k]).abs().max().item())
    a, b = (new[k].cpu() - sd0[k]).flatten().double(), (ref[k] - sd0[k]).flatten().double()
    cos = min(cos, (torch.dot(a, b) / (a.norm() * b.norm())).item())
if variant in ("main", "coopf"):   # fp16-rounded weight-gradient operands: tests/test_train_gpu.py::test_three_adam_steps_vs_oracle
    assert cos > 0.9998 and worst < 2e-3, (cos, worst)
else:
    assert worst < 2e-5, worst
dist.barrier()
dist.destroy_process_group()
print("rank", rank, variant, "nccl" if multi else "gloo", "ok: max |param - single-process oracle| = %%.2e, min update cosine %%.6f" %% (worst, cos))
"""


@pytest.mark.parametrize("variant,uneven,segments", [("coop16", False, 1), ("main", False, 1), ("coopf", False, 1),
                                                     ("coopf", True, 1), ("coopf", False, 3), ("coopf", True, 3)])
def test_two_ranks_train_like_one_process(tmp_path, variant, uneven, segments):
    """coopf = the default dispatch of small steps (configs[3]: 4096 rays per GPU -> one-tile cooperative fp16 chains);
    uneven = the ranks hold 5/8 and 3/8 of the batch and weight their gradients by ray share (n_global); segments = 3: the
    opt-in segmented dX chain (R2LTrainer(chain_segments=3))."""
    script = tmp_path / "worker.py"
    script.write_text(WORKER % {"root": ROOT})
    env = {k: v for k, v in os.environ.items() if not k.startswith("R2L_")}
    env.update(MASTER_ADDR="127.0.0.1", R2L_FORCE_VARIANT=variant, R2L_TEST_UNEVEN="1" if uneven else "0",
               R2L_TEST_SEGMENTS=str(segments))
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29613", str(script)], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("ok: max |param") == 2  # (the two ranks' lines may interleave)
    print(r.stdout[-400:])


def test_bench_two_ranks_walk(tmp_path):
    """bench.py's N > 1 code (process group, barrier-bracketed timing with MAX over ranks, frames sharded over ranks,
    weak / strong / 4096-ray training legs through the bucketed all-reduce, pose-sharded teacher leg, rank-0-only line) run
    as TWO ranks on this one GPU over gloo (R2L_BENCH_SHARED_GPU_TEST=1): the line must carry n_gpus 2, the measured rank
    count 2, the legs of a distributed run and the label that it is not a measurement."""
    import json
    env = {k: v for k, v in os.environ.items() if not k.startswith("R2L_")}
    env.update(MASTER_ADDR="127.0.0.1", R2L_BENCH_SHARED_GPU_TEST="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29617", os.path.join(ROOT, "bench.py"),
                        "--gpus", "2", "--steps", "2", "--warmup", "1", "--full"], env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["rccl_ranks"] == 2 and "shared_gpu_test" in out
    assert out["value"] > 0 and out["config"]["parallelism"].startswith("frames sharded across 2")
    # top level = the graded exact-fp32 families (value / dtype / roofline / train / teacher); the library's default fp16 trio is
    # the fast mode and reports under "fast_mode" (bench.py docstring)
    assert out["dtype"].startswith("f32 (v_mfma_f32_32x32x2_f32") and out["roofline"]["peak"] == 157.3
    assert out["train"]["roofline"]["peak"] == 157.3 and out["teacher"]["precision"] == "fp32_mfma"
    fast = out["fast_mode"]
    assert fast["path"] == "fp16x2" and abs(fast["roofline"]["peak"] - 2500.0 / 3) < 1e-6 and "range" in fast
    for leg in ("train", "train_strong", "train_4096", "train_12288", "teacher"):
        assert leg in fast, leg
    assert fast["train_strong"]["scaling"] == "strong" and fast["train_strong"]["global_rays_per_step"] == 98304
    for r in (out["train"]["roofline"], fast["train"]["roofline"]):
        assert r["grad_allreduce_alone_ms"] > 0 and r["grad_allreduce_bytes"] == 5917187 * 4 and r["allreduce_buckets"] == 4
    assert "2 tile(s) per workgroup" in fast["train_strong"]["roofline"]["matrix_path"]  # 49 152 rays per rank
    assert "raw2outputs" in out and out["raw2outputs"]["S64"]["bytes_per_ray"] == 1572 and out["raw2outputs"]["S192"]["bytes_per_ray"] == 3876
    assert list(out)[-1] == "summary" and out["summary"]["fast_train_4096"][0] > 0
    assert "cpu_baseline" not in out  # rank 0 at N = 1 only
