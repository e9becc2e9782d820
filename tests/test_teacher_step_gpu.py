"""One teacher training step in one library call on the GPU (include/r2l_hip.h r2l_draw_normal / r2l_teacher_train_step;
TeacherTrainer.fused_step; utils/train_nerf.py --r2l_fused_step): the device's normals against the fp64 restatement, the fused
step against the staged step bit for bit, its statelessness, and the command line with a resume."""
import os

import numpy as np
import pytest
import torch

from oracle import r2l_oracle as O
from tests.test_pixel_batch_cpu import write_config
from tests.test_teacher_step_cpu import STREAMS, draw_normal_np
from tests.test_teacher_train_cpu import make_scene
from tests.test_teacher_train_gpu import make_teacher, rays

pytestmark = pytest.mark.gpu
BASE = 1 << 62  # stream ids of a step: BASE + 4 * step + k


# ---- r2l_draw_normal ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,stream_id", STREAMS)
def test_draw_normal_against_fp64(seed, stream_id):
    """Every element within 6 * 2^-24 * r + 1e-12 of the fp64 restatement, r = sqrt(-2 ln u1).  Where the bar comes from: a 1-ulp
    logf moves r by 2^-24 r, the correctly rounded sqrtf by another 2^-24 r, a 2-ulp sincospif at the exact argument 2 u2 by
    2 * 2^-24 r, the product's rounding by 2^-24 r: 5 * 2^-24 r (correctly rounded functions measure 3.2; an angle formed as
    fp32(2 pi) * u2 measures 7.0 and fails).  n = 4099 ends inside a Philox block; shorter draws end at every position of a block,
    and the slices [i0:] are compared with the restatement started at i0.  Measured on one MI355X: 2.43 and 2.39."""
    from r2l_amd.render import draw_normal
    n = 4099
    want, r = draw_normal_np(n, seed, stream_id, with_r=True)
    got = draw_normal(n, seed, stream_id, "cuda")
    assert got.dtype == torch.float32 and got.shape == (n,)
    g = got.cpu().numpy().astype(np.float64)
    ratio = np.abs(g - want) / (2.0**-24 * r + 1e-12 / 6)
    print("r2l_draw_normal(%d, %d): worst |error| / (2^-24 r) = %.2f over %d elements; max |n_i| %.2f" %
          (seed, stream_id, ratio.max(), n, np.abs(g).max()))
    assert np.all(np.abs(g - want) <= 6 * 2.0**-24 * r + 1e-12), ratio.max()
    # a pure function of the element index: shorter draws are prefixes, whatever part of the last block they end in
    for m in (1, 2, 3, 4, 5, 1023, 1024, 1025, 4096, 4097, 4098):
        assert torch.equal(draw_normal(m, seed, stream_id, "cuda"), got[:m]), m
    for i0 in (1, 2, 3, 4094):
        w0, r0 = draw_normal_np(n - i0, seed, stream_id, i0=i0, with_r=True)
        assert np.all(np.abs(g[i0:] - w0) <= 6 * 2.0**-24 * r0 + 1e-12), i0
    # scale: one fp32 rounding of scale * n_i
    half = draw_normal(n, seed, stream_id, "cuda", scale=0.5)
    assert torch.equal(half, got * 0.5)
    third = draw_normal(n, seed, stream_id, "cuda", scale=1. / 3.)
    assert torch.equal(third, got * torch.tensor(1. / 3., dtype=torch.float32, device="cuda"))
    assert np.abs(g).max() <= 5.77


def test_draw_normal_writes_nothing_past_n():
    from r2l_amd import _lib
    from r2l_amd.engine import _ptr, _stream
    buf = torch.full((16,), 7., device="cuda")
    for n in (0, 1, 5, 8):
        buf.fill_(7.)
        _lib.check(_lib.load().r2l_draw_normal(_ptr(buf), n, 3, 4, 1., _stream()), "r2l_draw_normal")
        assert torch.all(buf[n:] == 7.) and torch.all(buf[:n] != 7.), n


# ---- fused = staged ----------------------------------------------------------------------------------------------------------
# R rays, NS + NI samples, background, perturb, raw_noise_std: the smallest shapes that cross partial tiles and chunks (R = 37),
# the general and the quarter-wave kernels of raw2outputs / sample_pdf_sort (32 + 96 against 64 + 128 / 192), the shared row of
# uniforms (perturb 0), both noise buffers, and the coarse net alone (one ray, no fine stream)
STEP_CASES = [
    ("37-64+128-white", dict(R=37, NS=64, NI=128, white=True, perturb=1., std=0.)),
    ("64-32+96-black-noise", dict(R=64, NS=32, NI=96, white=False, perturb=1., std=1.)),
    ("64-64+192-white-det-noise", dict(R=64, NS=64, NI=192, white=True, perturb=0., std=.5)),
    ("1-64+0-white", dict(R=1, NS=64, NI=0, white=True, perturb=1., std=0.)),
]
LR, SEED = 5e-4, (1 << 40) + 99


def trainer(case, sds=None):
    from r2l_amd.teacher_train import TeacherTrainer
    csd, fsd = sds if sds is not None else O.make_teacher_state_dicts(5, 2, alpha_bias=0.5)
    fine = make_teacher(fsd) if case["NI"] > 0 else None
    return TeacherTrainer(make_teacher(csd), fine, N_samples=case["NS"], N_importance=case["NI"], perturb=case["perturb"],
                          white_bkgd=case["white"], raw_noise_std=case["std"])


def staged_step(tr, case, batch, step, monkeypatch):
    """TeacherTrainer.step fed the draws the fused step makes for itself."""
    from r2l_amd.render import draw_normal, draw_uniform
    from r2l_amd.teacher_train import TeacherTrainer
    R, NS, NI = case["R"], case["NS"], case["NI"]
    sid = BASE + 4 * step
    t_rand = draw_uniform(R * NS, SEED, sid, "cuda").view(R, NS) if case["perturb"] > 0 else None
    u = draw_uniform(R * NI, SEED, sid + 1, "cuda").view(R, NI) if case["perturb"] > 0 and NI > 0 else None
    stream_of = {NS: sid + 2, NS + NI: sid + 3} if NI > 0 else {NS: sid + 2}
    noise = lambda self, R_, S_: (draw_normal(R_ * S_, SEED, stream_of[S_], "cuda", scale=case["std"]).view(R_, S_)
                                  if case["std"] > 0 else None)
    monkeypatch.setattr(TeacherTrainer, "_noise", noise)
    out = tr.step(*batch[:3], 2., 6., batch[3], LR, t_rand=t_rand, u=u)
    for eng in tr.engines:
        eng.ensure_packed()  # the staged path packs at the next launch; the fused call has packed already
    return out


def state_of(tr):
    return [tr.flat, tr.exp_avg, tr.exp_avg_sq] + [eng.wstream for eng in tr.engines]


def assert_same_state(a, b, what):
    for name, x, y in zip(("params", "exp_avg", "exp_avg_sq", "wstream_coarse", "wstream_fine"), state_of(a), state_of(b)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (what, name, (x - y).abs().max().item())


@pytest.mark.parametrize("case", [c for _, c in STEP_CASES], ids=[i for i, _ in STEP_CASES])
def test_fused_step_equals_staged_step(case, monkeypatch):
    """Three consecutive steps: after each, parameters, both moments, both weight streams, loss and psnr are the same bits.  Then
    statelessness: step 3 from a fresh trainer loaded with the state after step 2 equals the uninterrupted step 3."""
    staged, fused = trainer(case), trainer(case)
    assert_same_state(staged, fused, "start")
    saved = None
    for step in (1, 2, 3):
        batch = [t.cuda() for t in rays(case["R"], 20 + step)]
        loss, psnr = staged_step(staged, case, batch, step, monkeypatch)
        before = fused.flat.clone()
        out = fused.fused_step(*batch[:3], 2., 6., batch[3], LR, step=step, seed=SEED)
        assert out is fused.loss_out and fused.step_count == step == staged.step_count
        assert not torch.equal(before, fused.flat)  # it did train
        assert_same_state(staged, fused, "step %d" % step)
        got = out.tolist()
        assert np.isfinite(got).all()
        assert np.float32(got[0]).tobytes() == np.float32(loss).tobytes() and np.float32(got[1]).tobytes() == np.float32(psnr).tobytes(), \
            (step, got, loss, psnr)
        if step == 2:
            saved = ([{k: v.detach().clone() for k, v in net.state_dict().items()} for net in fused.nets],
                     fused.optimizer_state_dict(LR))
    # the weights the modules hold are the flat buffer: a render that follows sees the updated, packed weights
    fresh = trainer(case, sds=(saved[0][0], saved[0][-1]))
    fresh.load_optimizer_state_dict(saved[1])
    loss_hist = torch.zeros(4, 2, device="cuda")
    out = fresh.fused_step(*batch[:3], 2., 6., batch[3], LR, step=3, seed=SEED, loss_out=loss_hist[2])
    assert out.data_ptr() == loss_hist[2].data_ptr() and torch.all(loss_hist[:2] == 0) and torch.all(loss_hist[3] == 0)
    assert_same_state(fused, fresh, "step 3 from a fresh trainer")
    assert torch.equal(loss_hist[2].view(torch.int32), fused.loss_out.view(torch.int32))


def test_fused_step_depends_on_seed_and_step():
    """Other seeds or iterations draw other numbers; the same ones, the same bits (two trainers, no shared state)."""
    case = STEP_CASES[1][1]
    batch = [t.cuda() for t in rays(case["R"], 5)]
    outs = []
    for step, seed in ((1, SEED), (1, SEED), (2, SEED), (1, SEED + 1)):
        tr = trainer(case)
        tr.fused_step(*batch[:3], 2., 6., batch[3], LR, step=step, seed=seed)
        outs.append(tr.exp_avg.clone())  # (1 - beta1) * grad: the step's gradient, whatever Adam's step count
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    assert not torch.equal(outs[0], outs[2]) and not torch.equal(outs[0], outs[3])


# ---- command line ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["images", "batching", "batching-noise"])
def test_cli_fused_step_and_resume(mode, tmp_path, monkeypatch):
    """2 train views of 8 x 8, N_rand 32: four iterations in one run against two + --resume + two, every parameter bit for bit."""
    from r2l_amd import train_nerf
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("R2L_SEED", "7")
    root = str(tmp_path / "scene")
    os.makedirs(root)
    make_scene(root)
    common = ["--config", write_config(tmp_path / "teacher.txt"), "--datadir", root, "--testskip", "1", "--N_samples", "8",
              "--N_importance", "8", "--i_print", "2", "--i_testset", "1000", "--i_weights", "2", "--save_intermediate_models",
              "--N_rand", "32", "--N_iters", "4", "--r2l_fused_step"]
    common += ["--no_batching", "--precrop_iters", "0"] if mode == "images" else []
    common += ["--raw_noise_std", "1.0"] if mode.endswith("noise") else []
    a = train_nerf.main(common + ["--experiment_name", "A"])
    assert (a["batcher"] is None) == (mode == "images") and a["trainer"].raw_noise_std == (1. if mode.endswith("noise") else 0.)
    assert len(a["history"]) == 4 and all(len(h) == 2 and np.isfinite(h).all() for h in a["history"])
    log = open(os.path.join(a["logger"].log_path, "log.txt")).read()
    assert "Fused step" in log and "Philox" in log and "[TRAIN] Iter 4 Loss" in log and "[TRAIN] Iter 3 Loss" not in log
    mid = os.path.join(a["logger"].weights_path, "ckpt_2.tar")
    b = train_nerf.main(common + ["--experiment_name", "B", "--pretrained_ckpt", mid, "--resume"])
    assert len(b["history"]) == 2 and b["history"] == a["history"][2:]
    for name in ("flat", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(a["trainer"], name).view(torch.int32), getattr(b["trainer"], name).view(torch.int32)), name
    for pa, pb in zip(a["trainer"].params, b["trainer"].params):
        assert torch.equal(pa.data, pb.data)
    assert b["trainer"].step_count == 4
    # without the switch the same command trains by the staged path, on torch's draws: other numbers
    if mode == "batching":
        c = train_nerf.main([x for x in common if x != "--r2l_fused_step"] + ["--experiment_name", "C"])
        assert "Fused step" not in open(os.path.join(c["logger"].log_path, "log.txt")).read()
        assert len(c["history"]) == 4 and not torch.equal(c["trainer"].flat, a["trainer"].flat)
