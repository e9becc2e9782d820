"""The teacher's training step on the live samples of an occupancy grid, on the GPU (include/r2l_hip.h "occupancy while the teacher
trains": r2l_teacher_mlp_train_live, r2l_teacher_backward_live, r2l_teacher_train_step_occ; TeacherTrainer(occupancy=);
utils/train_nerf.py --r2l_occ_train): the live forward against the plain one at the index list, the live backward against the plain
backward of the compacted problem, the whole step under all-ones grids against the plain step — all bit for bit —, the step under
real grids against the masked render and fp64, fused against staged across a rebuild, the command line with a resume, and the
argument refusals.  Exact-fp32 kernels throughout."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.teacher_util import forward_weights, scene_rays, stash_slots, teacher_backward_from_stash, trained_like_pair
from tests.test_teacher_backward_gpu import (C_BWD, NREL_BWD, SENTINEL, Net, bar_violations, guarded, guards_intact, inputs, make_draw,
                                             nrel, split)
from tests.test_teacher_step_gpu import LR, SEED, assert_same_state, staged_step
from tests.test_teacher_train_cpu import ROOT, make_scene
from tests.test_teacher_train_gpu import make_teacher, rays

pytestmark = pytest.mark.gpu

R0, S0 = 37, 61
P0 = R0 * S0  # 2257: no multiple of the 128-lane workgroup or of the 2048-point chunk
COUNTS = [0, 1, 127, 128, 129, 2047, 2048, 2049, P0]
INVALID = 1  # hipErrorInvalidValue


def _L():
    from r2l_amd import _lib
    return _lib


def _p(t):
    return _L().ptr(t)


def _s():
    return _L().stream()


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def subset(M, seed=3):
    """An ascending random subset of M of the P0 samples (int64, capacity P0: the entries past M are never read)."""
    perm = torch.randperm(P0, generator=torch.Generator().manual_seed(seed))
    idx = torch.full((P0,), -(1 << 40), dtype=torch.int64)  # past the count: numbers nobody may use as an address
    idx[:M] = torch.sort(perm[:M])[0]
    return idx.cuda()


_PLAIN = {}


def plain(kind):
    """Net, inputs, and the plain training forward's raw and stash slots of one kind of weights: computed once, never written."""
    if kind not in _PLAIN:
        net = Net(forward_weights(kind))
        o, d, vd, z = [t.cuda() for t in inputs(R0, S0, kind)]
        raw, st_whole, st, _ = net.forward_stash(o, d, vd, z)
        _PLAIN[kind] = dict(net=net, o=o, d=d, vd=vd, z=z, raw=raw.reshape(P0, 4), slots=stash_slots(st, P0), stash=st)
    return _PLAIN[kind]


def live_forward(ref, idx, count):
    """r2l_teacher_mlp_train_live into sentinel buffers: (raw [P0,4], stash, raw_whole, stash_whole)."""
    lib = _L().load()
    n_st = lib.r2l_teacher_stash_floats(P0)
    st_whole, st = guarded(n_st)
    raw_whole, raw = guarded(P0 * 4)
    cnt = torch.tensor([count], dtype=torch.int64, device="cuda")
    net = ref["net"]
    _L().check(lib.r2l_teacher_mlp_train_live(_p(ref["o"]), _p(ref["d"]), _p(ref["vd"]), _p(ref["z"]), _p(idx), _p(cnt), _p(net.wstream),
                                              _p(net.flat), _p(raw), _p(st), R0, S0, _s()), "r2l_teacher_mlp_train_live")
    assert guards_intact(raw_whole, P0 * 4) and guards_intact(st_whole, n_st)
    return raw.view(P0, 4), st, cnt


def check_forward(ref, raw, st, good):
    """good = (samples, their tile lanes).  raw: the plain bits at the samples, +0 elsewhere.  Stash: the row of each lane is the
    plain row of its sample; every other row keeps the sentinel."""
    idx_good, rows_good = good
    want = torch.zeros_like(ref["raw"])
    want[idx_good] = ref["raw"][idx_good]
    assert same(raw, want)
    keep = torch.ones(P0, dtype=torch.bool, device="cuda")
    keep[rows_good] = False
    for l, (got, full) in enumerate(zip(stash_slots(st, P0), ref["slots"])):
        assert same(got[rows_good], full[idx_good]), l
        assert bool((bits(got)[keep] == SENTINEL).all().item()), l


@pytest.mark.parametrize("kind", ["init", "trained"])
@pytest.mark.parametrize("M", COUNTS)
def test_forward_live(M, kind):
    ref = plain(kind)
    idx = subset(M)
    raw, st, _ = live_forward(ref, idx, M)
    rows = torch.arange(M, device="cuda")
    check_forward(ref, raw, st, (idx[:M], rows))
    if M == P0:  # a count above the capacity counts as the capacity
        raw2, st2, _ = live_forward(ref, idx, P0 + 5)
        assert same(raw2, raw) and same(st2, st) and same(raw, ref["raw"]) and same(st, ref["stash"])


def test_forward_live_entries_out_of_range():
    """One entry -1 and one entry P: nothing is read or written for those lanes (their raw stays zero, their stash rows unwritten)."""
    ref = plain("trained")
    M = 300
    idx = subset(M)
    lost = idx[[7, 200]].clone()
    idx[7], idx[200] = -1, P0
    raw, st, _ = live_forward(ref, idx, M)
    rows = torch.tensor([i for i in range(M) if i not in (7, 200)], device="cuda")
    check_forward(ref, raw, st, (idx[rows], rows))
    assert bool((raw[lost] == 0).all().item())


def live_backward(ref, idx, cnt, st, draw):
    lib = _L().load()
    net = ref["net"]
    n = net.flat.numel()
    g_whole, grads = guarded(n)
    n_work = lib.r2l_teacher_train_live_work_floats(P0)
    assert n_work == lib.r2l_teacher_train_work_floats(P0) + 4 * P0
    w_whole, work = guarded(n_work)
    _L().check(lib.r2l_teacher_backward_live(_p(ref["o"]), _p(ref["d"]), _p(ref["vd"]), _p(ref["z"]), _p(idx), _p(cnt), _p(net.flat), _p(st),
                                             _p(draw), _p(grads), _p(work), R0, S0, _s()), "r2l_teacher_backward_live")
    assert guards_intact(g_whole, n) and guards_intact(w_whole, n_work)
    return grads


@pytest.mark.parametrize("kind", ["init", "trained"])
@pytest.mark.parametrize("M", COUNTS)
def test_backward_live_equals_compacted_backward(M, kind):
    """grads of the live backward (on the live forward's compact stash) = r2l_teacher_backward on rows o[idx/S], d[idx/S], v[idx/S],
    z.flat[idx] as [M,1] with the PLAIN stash's rows idx gathered to the layout of M points and draw.flat[idx]: bit for bit."""
    lib = _L().load()
    ref = plain(kind)
    net = ref["net"]
    idx = subset(M)
    draw = make_draw(R0, S0, R0 * 1000 + S0).cuda()
    _, st, cnt = live_forward(ref, idx, M)
    got = live_backward(ref, idx, cnt, st, draw)
    assert same(live_backward(ref, idx, cnt, st, draw), got)  # two calls, the same bits
    ii = idx[:M]
    r = ii // S0
    if M > 0:
        o, d, vd = ref["o"][r].contiguous(), ref["d"][r].contiguous(), ref["vd"][r].contiguous()
        z = ref["z"].reshape(-1)[ii].reshape(M, 1).contiguous()
        stash = torch.cat([s[ii].reshape(-1) for s in ref["slots"]])
        dr = draw.reshape(P0, 4)[ii].reshape(M, 1, 4).contiguous()
        want = net.backward(o, d, vd, z, stash, dr)[0]
    else:
        want = torch.full((net.flat.numel(),), 7., device="cuda")
        _L().check(lib.r2l_teacher_backward(None, None, None, None, None, None, None, _p(want), None, 0, 1, _s()), "r2l_teacher_backward")
        assert bool((bits(got) == 0).all().item())
    assert same(got, want), (M, kind, (got - want).abs().max().item())
    if M == P0:  # every sample live, in order: the plain backward itself
        assert same(got, net.backward(ref["o"], ref["d"], ref["vd"], ref["z"], ref["stash"], draw)[0])


# ---- whole steps -------------------------------------------------------------------------------------------------------------------
CASE = dict(R=45, NS=16, NI=16, white=True, perturb=1., std=0.)


def pair_trainer(kind, case=CASE, occupancy=None):
    from r2l_amd.render import teacher_engine
    from r2l_amd.teacher_train import TeacherTrainer
    from oracle import r2l_oracle as O
    csd, fsd = trained_like_pair() if kind == "trained" else O.make_teacher_state_dicts(5, 2, alpha_bias=0.5)
    tr = TeacherTrainer(make_teacher(csd), make_teacher(fsd), N_samples=case["NS"], N_importance=case["NI"], perturb=case["perturb"],
                        white_bkgd=case["white"], raw_noise_std=case["std"], occupancy=occupancy)
    for net in tr.nets:
        teacher_engine(net).set_config(precision="fp32_mfma")  # (renders and grid builds of these nets: the trainer's family)
    return tr


def ones_grid():
    from r2l_amd.occupancy import OccupancyGrid, pack_bits
    return OccupancyGrid([-1.] * 3, [1.] * 3, G=5, k=1, dilate=0).set_bits(pack_bits(np.ones((5, 5, 5), dtype=bool)), device="cuda")


@pytest.mark.parametrize("kind", ["init", "trained"])
def test_step_with_all_ones_grids_is_the_plain_step(kind, monkeypatch):
    """Every sample live: the staged live step and r2l_teacher_train_step_occ each equal their plain counterpart bit for bit —
    loss, gradients, parameters after Adam, both moments, both weight streams; the counters saw every sample of both passes."""
    batch = [t.cuda() for t in (rays(CASE["R"], 21) if kind == "init" else batch_rays(CASE["R"], 21))]
    g = ones_grid()
    for fused in (False, True):
        a, b = pair_trainer(kind), pair_trainer(kind, occupancy=(g, ones_grid()))
        outs = []
        for tr in (a, b):
            if fused:
                outs.append(tr.fused_step(*batch[:3], 2., 6., batch[3], LR, step=1, seed=SEED).clone())
            else:
                staged_step(tr, CASE, batch, 1, monkeypatch)
                outs.append(tr.loss_out.clone())
        assert same(outs[0], outs[1]) and same(a.grads, b.grads) and float(a.grads.abs().max()) > 0, fused
        assert_same_state(a, b, "fused" if fused else "staged")
        total = CASE["R"] * (2 * CASE["NS"] + CASE["NI"])
        assert b.live_acc.tolist() == [total, total] and a.live_acc.tolist() == [0, 0]


def batch_rays(R, seed):
    """R rays of scene_rays' camera drawn over its whole frame, and targets: (o, d, viewdirs, target)."""
    rb = scene_rays(181 * 181, 0)[torch.randperm(181 * 181, generator=torch.Generator().manual_seed(seed))[:R]]
    tgt = torch.rand(R, 3, generator=torch.Generator().manual_seed(seed + 1))
    return rb[:, 0:3].contiguous(), rb[:, 3:6].contiguous(), rb[:, 8:11].contiguous(), tgt


REAL = dict(R=256, NS=16, NI=16, white=True, perturb=0., std=0.)
REAL_BOX, REAL_G = 1.6, 32


def real_grids(tr):
    from r2l_amd.occupancy import OccupancyGrid
    return tuple(OccupancyGrid([-REAL_BOX] * 3, [REAL_BOX] * 3, G=REAL_G, k=2, dilate=1, precision="fp32_mfma").build(net)
                 for net in tr.nets)


def test_step_with_real_grids():
    """The trained-like pair under grids of 32^3 cells over +-1.6 (2 probes per cell and axis, one cell of dilation), 256 rays of
    scene_rays' camera drawn over its whole frame (the first 256 are one image row that misses the scene), 16 + 16 samples, perturb 0.

    Against the masked full render: per ray and net, sqerr has the plain step's bits on the rays where occupancy.miss_report counts
    no miss, and the loss recomputed from those rays' sqerr is the same number.
    Against fp64: the bars of tests/test_teacher_backward_gpu.py — every entry within 3e-6 of its magnitude and every tensor within
    1e-5 norm-relative of the fp64 backprop (teacher_util.teacher_backward_from_stash, which tests/test_teacher_train_cpu.py pins to
    fp64 autograd) of the ZERO-MASKED problem: all R*S samples at the step's last_z, draw zeroed where live_spec says not live, the
    activations of the live samples the device's own (the compact stash spread to the full layout, zero rows elsewhere).
    Condition, asserted and not skipped: at most 1 % of the rays carry a miss, the grids skip at least 20 % of the samples."""
    from r2l_amd.occupancy import live_spec, miss_report, sample_points
    o, d, vd, tgt = [t.cuda() for t in batch_rays(REAL["R"], 4)]
    a = pair_trainer("trained", REAL)
    b = pair_trainer("trained", REAL)
    grids = real_grids(b)
    b.set_occupancy(grids)
    seen = {}
    backward = b._backward

    def keep(i, rays_o, rays_d, viewdirs, z, raw, stash, nz, target):
        out = backward(i, rays_o, rays_d, viewdirs, z, raw, stash, nz, target)
        idx, cnt = b._live[i]
        seen[i] = (stash.clone(), b._bufs["draw"][:z.numel() * 4].clone().view(*z.shape, 4), idx.clone(), int(cnt.item()))
        return out
    b._backward = keep
    la = a.forward_backward(o, d, vd, 2., 6., tgt).clone()
    lb = b.forward_backward(o, d, vd, 2., 6., tgt).clone()
    R = REAL["R"]
    ones = torch.ones(R, 1, device="cuda")
    rep = miss_report(torch.cat([o, d, 2. * ones, 6. * ones, vd], -1), a.nets[0], a.nets[1], grids, REAL["NS"], REAL["NI"], white_bkgd=True)
    ok = (rep["misses"] == 0).cuda()
    live_n, total = b.live_acc.tolist()
    print("real grids: %d of %d rays carry a miss; live samples %d / %d (%.1f%% skipped); loss plain %.6g, live %.6g"
          % (int((~ok).sum()), R, live_n, total, 100. * (1 - live_n / total), la[0].item(), lb[0].item()))
    assert int((~ok).sum()) <= R // 100 and live_n <= 0.8 * total and total == R * (2 * REAL["NS"] + REAL["NI"])
    for i in (0, 1):
        sa, sb = a._bufs["sqerr%d" % i][:R], b._bufs["sqerr%d" % i][:R]
        assert same(sa[ok], sb[ok]), i
        assert float(sa[ok].sum()) == float(sb[ok].sum())
    if bool(ok.all()):
        assert same(la, lb)
    # fp64, per net
    off = 0
    g = b.grads
    for i, sd in enumerate(trained_like_pair()):
        stash_c, draw, idx, cnt = seen[i]
        z = b.last_z[i]
        P = z.numel()
        live = live_spec(grids[i].words(), grids[i].lo, grids[i].inv, grids[i].G,
                         sample_points(o.cpu().numpy(), d.cpu().numpy(), z.cpu().numpy()).reshape(-1, 3))
        want_idx = torch.from_numpy(np.flatnonzero(live)).cuda()
        assert cnt == want_idx.numel() and torch.equal(idx[:cnt], want_idx)
        full = torch.zeros(stash_c.numel(), device="cuda")
        for fs, cs in zip(stash_slots(full, P), stash_slots(stash_c, P)):
            fs[want_idx] = cs[:cnt]
        masked = draw * torch.from_numpy(live).cuda().view(*z.shape, 1)
        assert same(masked + 0., draw + 0.)  # a sample that is not live has raw = 0, hence an exactly zero row of draw
        want, mags = teacher_backward_from_stash(sd, o, d, vd, z, full, masked, device="cuda")
        got = split(g[off:off + b.n_net], sd)
        off += b.n_net
        viol = bar_violations(got, want, mags)
        worst = max(nrel(got[k], want[k]) for k in want)
        print("real grids, net %d: entries past %.0e of their magnitude: %d; worst norm-relative error %.3g" % (i, C_BWD, sum(viol.values()), worst))
        assert not any(viol.values()), viol
        for k in want:
            assert nrel(got[k], want[k]) <= NREL_BWD, (i, k, nrel(got[k], want[k]))


def test_fused_equals_staged_across_a_rebuild(monkeypatch):
    """Three consecutive steps on real grids, the grids rebuilt in place between the second and the third: the fused step equals the
    staged one bit for bit, and live_acc is the sum of the counts the staged path's index lists had."""
    staged, fused = pair_trainer("trained"), pair_trainer("trained")
    gs, gf = real_grids(staged), real_grids(fused)
    staged.set_occupancy(gs)
    fused.set_occupancy(gf)
    counted = 0
    for step in (1, 2, 3):
        batch = [t.cuda() for t in batch_rays(CASE["R"], 30 + step)]
        loss, psnr = staged_step(staged, CASE, batch, step, monkeypatch)
        counted += sum(int(c.item()) for _, c in staged._live.values())
        out = fused.fused_step(*batch[:3], 2., 6., batch[3], LR, step=step, seed=SEED)
        assert_same_state(staged, fused, "step %d" % step)
        assert same(staged.grads, fused.grads)
        got = out.tolist()
        assert np.float32(got[0]).tobytes() == np.float32(loss).tobytes() and np.float32(got[1]).tobytes() == np.float32(psnr).tobytes()
        if step == 2:
            for grids, tr in ((gs, staged), (gf, fused)):
                for g, net in zip(grids, tr.nets):
                    held = g.bits
                    assert g.rebuild(net).bits is held  # (in place: the trainer's descriptor still points at the bits)
            assert all(np.array_equal(x.words(), y.words()) for x, y in zip(gs, gf))
    total = 3 * CASE["R"] * (2 * CASE["NS"] + CASE["NI"])
    assert staged.live_acc.tolist() == [counted, total] == fused.live_acc.tolist() and 0 < counted < total


# ---- command line ------------------------------------------------------------------------------------------------------------------
def test_cli_occ_train_and_resume(tmp_path, monkeypatch):
    """2 train views of 8 x 8 (16 x 16 at half_res), six fused iterations from the device pixel sampler with a refresh every 2 and
    a checkpoint at 4, against a resume from 4: parameters, moments and grid words at 6 bit for bit; three refresh lines in the
    uninterrupted run's log; the checkpoint loads through the plain loader, which ignores the key."""
    from r2l_amd import train_nerf
    from r2l_amd.checkpoint import load_ckpt
    from r2l_amd.driver import create_nerf_teacher
    from r2l_amd.options import parse_args
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("R2L_SEED", "7")
    root = str(tmp_path / "scene")
    os.makedirs(root)
    make_scene(root, size=16)
    base = ["--config", os.path.join(ROOT, "configs", "lego.txt"), "--datadir", root, "--testskip", "1", "--N_samples", "8",
            "--N_importance", "8", "--i_print", "2", "--i_testset", "1000", "--i_weights", "2", "--save_intermediate_models",
            "--N_rand", "12", "--N_iters", "6", "--precrop_iters", "0", "--no_batching", "--r2l_image_sampler", "--r2l_fused_step"]
    common = base + ["--r2l_occ_train", "--r2l_occ_every", "2", "--r2l_occ_res", "16"]
    a = train_nerf.main(common + ["--experiment_name", "A"])
    log = open(os.path.join(a["logger"].log_path, "log.txt")).read()
    assert log.count("occupancy grid refresh after iteration") == 3 and log.count("live points") == 3
    assert all("refresh after iteration %d:" % i in log for i in (2, 4, 6)) and log.count("occupancy grid of the training step (") == 2
    assert a["occupancy"].base == 6 and a["trainer"].occupancy == a["occupancy"].pair()
    mid = os.path.join(a["logger"].weights_path, "ckpt_4.tar")
    ck = load_ckpt(mid, map_location="cpu")
    st = ck["r2l_occ_train"]
    assert st["base"] == 4 and st["every"] == 2 and st["res"] == 16 and len(st["words"]) == 2 and st["words"][0].numel() == 128
    b = train_nerf.main(common + ["--experiment_name", "B", "--pretrained_ckpt", mid, "--resume"])
    logb = open(os.path.join(b["logger"].log_path, "log.txt")).read()
    assert "restored from the checkpoint" in logb and logb.count("occupancy grid refresh after iteration") == 1
    assert "occupancy grid of the training step (" not in logb
    assert len(b["history"]) == 2 and b["history"] == a["history"][4:]
    for name in ("flat", "exp_avg", "exp_avg_sq"):
        assert same(getattr(a["trainer"], name), getattr(b["trainer"], name)), name
    for ga, gb in zip(a["occupancy"].grids, b["occupancy"].grids):
        assert torch.equal(ga.bits, gb.bits)
    # the plain loader: the teacher of a render or of create_data, with no occupancy switch, reads the checkpoint as ever
    args = parse_args(base + ["--pretrained_ckpt", mid])
    args.model_name = "nerf"
    kw = create_nerf_teacher(args, torch.device("cuda"), a["logger"], 2., 6., ndc=False)
    for k, v in kw["network_fn"].state_dict().items():
        assert torch.equal(v.cpu(), ck["network_fn_state_dict"][k].cpu()), k
    # a checkpoint without the key: rebuilt at once, and said
    ck.pop("r2l_occ_train")
    bare = str(tmp_path / "bare.tar")
    torch.save(ck, bare)
    c = train_nerf.main(common + ["--experiment_name", "C", "--pretrained_ckpt", bare, "--resume"])
    assert "rebuilt at once" in open(os.path.join(c["logger"].log_path, "log.txt")).read()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def refusals():
    """[(what, call() -> code, what r2l_last_error must name)]; dummy pointers, never dereferenced: the checks come before any launch."""
    lib = _L().load()
    P = ctypes.c_void_p(4096)
    f3 = lambda *v: (ctypes.c_float * 3)(*v)

    def grid(**over):
        g = _L().OccGridDesc()
        assert lib.r2l_occ_grid_init(ctypes.byref(g), P, 4, 2, f3(-1, -1, -1), f3(1, 1, 1)) == 0
        for k, v in over.items():
            setattr(g, k, v)
        return g

    def fwd(R=3, S=2, **over):
        names = ["rays_o", "rays_d", "viewdirs", "z", "idx", "count_dev", "wstream", "tparams", "raw", "stash"]
        a = {n: P for n in names}
        a.update(over)
        return lib.r2l_teacher_mlp_train_live(*[a[n] for n in names], R, S, None)

    def bwd(R=3, S=2, **over):
        names = ["rays_o", "rays_d", "viewdirs", "z", "idx", "count_dev", "tparams", "stash", "draw", "grads", "work"]
        a = {n: P for n in names}
        a.update(over)
        return lib.r2l_teacher_backward_live(*[a[n] for n in names], R, S, None)

    def desc(**over):
        kw = dict(N_rand=4, N_samples=8, N_importance=8, perturb=1, white_bkgd=1, raw_noise_std=0., near=2., far=6., lr=5e-4, beta1=.9,
                  beta2=.999, eps=1e-8, step=1, seed=1)
        kw.update(over)
        return _L().TeacherStepDesc(**kw)

    def step(gc, gf=None, d=None, work=P, **over):
        d = d if d is not None else desc()
        names = ["rays_o", "rays_d", "viewdirs", "target", "ttab", "u_det", "params", "grads", "exp_avg", "exp_avg_sq", "wstream_coarse",
                 "wstream_fine", "loss_out"]
        a = {n: P for n in names}
        a.update(over)
        return lib.r2l_teacher_train_step_occ(ctypes.byref(d), *[a[n] for n in names], gc, gf, None, work, None)

    cases = [("forward: NULL %s" % n, (lambda n=n: fwd(**{n: None})), "tparams" if n == "tparams" else n)
             for n in ["rays_o", "rays_d", "viewdirs", "z", "idx", "count_dev", "wstream", "tparams", "raw", "stash"]]
    cases += [("forward: R < 0", lambda: fwd(R=-1), "R is negative"), ("forward: S < 1", lambda: fwd(S=0), "S:"),
              ("forward: R*S = 2^31", lambda: fwd(R=2**23, S=256), "R*S"),
              ("forward: misaligned raw", lambda: fwd(raw=ctypes.c_void_p(4104)), "raw"),
              ("forward: misaligned stash", lambda: fwd(stash=ctypes.c_void_p(4100)), "stash")]
    cases += [("backward: NULL %s" % n, (lambda n=n: bwd(**{n: None})), n)
              for n in ["rays_o", "rays_d", "viewdirs", "z", "idx", "count_dev", "tparams", "stash", "draw", "grads", "work"]]
    cases += [("backward: R < 0", lambda: bwd(R=-1), "R is negative"), ("backward: S < 1", lambda: bwd(S=0), "S:"),
              ("backward: too many points", lambda: bwd(R=65535, S=128), "R*S")]
    cases += [
        ("step: NULL grid_coarse", lambda: step(None), "grid_coarse"),
        ("step: coarse grid reserved", lambda: step(ctypes.byref(grid(reserved=(ctypes.c_int * 2)(0, 3)))), "reserved"),
        ("step: coarse grid NULL bits", lambda: step(ctypes.byref(grid(bits=None))), "bits"),
        ("step: fine grid G > 512", lambda: step(ctypes.byref(grid()), ctypes.byref(grid(G=600))), "G:"),
        ("step: fine grid inv", lambda: step(ctypes.byref(grid()), ctypes.byref(grid(inv=f3(2, 0, 2)))), "inv"),
        ("step: raw_noise_std > 0", lambda: step(ctypes.byref(grid()), d=desc(raw_noise_std=.5)), "raw_noise_std"),
        ("step: too many samples", lambda: step(ctypes.byref(grid()), d=desc(N_rand=2**20, N_samples=64, N_importance=64)), "N_rand"),
        ("step: the plain step's refusals hold (N_rand)", lambda: step(ctypes.byref(grid()), d=desc(N_rand=0)), "N_rand"),
        ("step: the plain step's refusals hold (target)", lambda: step(ctypes.byref(grid()), target=None), "target"),
        ("step: NULL work", lambda: step(ctypes.byref(grid()), work=None), "work"),
        ("step: misaligned work", lambda: step(ctypes.byref(grid()), work=ctypes.c_void_p(4100)), "work"),
    ]
    return cases, desc


def test_refusals():
    """Every refusal of the three new calls returns hipErrorInvalidValue, names its argument in r2l_last_error and launches nothing
    (the pointers are dummies: a launch would fault; buffers a call could reach are checked for their sentinel)."""
    lib = _L().load()
    canary = torch.full((1024,), 7., device="cuda")
    cases, desc = refusals()
    for what, call, needle in cases:
        rc = call()
        msg = (lib.r2l_last_error() or b"").decode()
        assert rc == INVALID, (what, rc, msg)
        assert needle in msg, (what, msg)
    torch.cuda.synchronize()
    assert bool((canary == 7.).all().item())
    assert lib.r2l_teacher_train_live_work_floats(-1) == -1 and lib.r2l_teacher_train_live_work_floats(0) == 0
    assert lib.r2l_teacher_step_occ_work_floats(ctypes.byref(desc(raw_noise_std=1.))) == -1
    assert lib.r2l_teacher_step_occ_work_floats(ctypes.byref(desc(N_rand=0))) == -1
    d = desc()
    assert lib.r2l_teacher_step_occ_work_floats(ctypes.byref(d)) > lib.r2l_teacher_step_work_floats(ctypes.byref(d)) > 0
    P = ctypes.c_void_p(4096)
    assert lib.r2l_teacher_mlp_train_live(P, P, P, P, P, P, P, P, P, P, 0, 3, None) == 0  # R == 0: a successful no-op
