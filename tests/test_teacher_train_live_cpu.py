"""CPU plumbing of the occupancy grids inside teacher training (--r2l_occ_train; r2l_amd/options.py validate_occ_train /
occ_refresh_base, r2l_amd/occupancy.py TrainOccupancy / OccupancyGrid.rebuild, TeacherTrainer(occupancy=)): the option refusals,
the sibling entry points that ignore the flags, the checkpoint key, the refresh schedule, and the CPU step under a pair of grids
against autograd of the masked render."""
import os

import numpy as np
import pytest
import torch

from tests.test_teacher_train_cpu import ROOT, batch, cpu_trainer, make_scene

LEGO = os.path.join(ROOT, "configs", "lego.txt")


@pytest.mark.parametrize("extra,match", [
    (["--raw_noise_std", "1.0"], "raw_noise_std"),
    (["--dataset_type", "llff"], "llff"),
    (["--use_viewdirs_off"], "use_viewdirs"),
    (["--r2l_occ_res", "0"], "r2l_occ_res"),
    (["--r2l_occ_res", "513"], "r2l_occ_res"),
    (["--r2l_occ_bound", "-1"], "r2l_occ_bound"),
    (["--r2l_occ_every", "0"], "r2l_occ_every"),
    (["--r2l_occ_every", str(2**30 + 1)], "r2l_occ_every"),
])
def test_option_refusals(extra, match):
    """ValueError at start-up, naming the flag, before anything is loaded (no --datadir exists here)."""
    from r2l_amd import train_nerf
    argv = ["--config", LEGO, "--r2l_occ_train"] + extra
    if extra == ["--use_viewdirs_off"]:  # a teacher without view directions: no config file (lego.txt switches them on)
        argv = ["--no_batching", "--N_importance", "128", "--r2l_occ_train"]
    with pytest.raises(ValueError, match=match):
        train_nerf.main(argv)


def test_cpu_run_is_refused(tmp_path, monkeypatch):
    from r2l_amd import train_nerf
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(ValueError, match="CPU"):
        train_nerf.main(["--config", LEGO, "--r2l_occ_train", "--datadir", str(tmp_path / "nowhere")])


def test_defaults_and_siblings_ignore_the_flags():
    """The switch is off by default; main.py's and create_data's parsers take the three flags, and their validators of the other
    occupancy switches do not look at them."""
    from r2l_amd.options import parse_args, validate_occ_fused, validate_occ_train, validate_occupancy
    plain = parse_args(["--config", LEGO])
    assert plain.r2l_occ_train is False and plain.r2l_occ_every >= 1 and (plain.r2l_occ_every & (plain.r2l_occ_every - 1)) == 0
    validate_occ_train(plain, "cpu")  # off: nothing to refuse, on any device
    args = parse_args(["--config", LEGO, "--r2l_occ_train", "--r2l_occ_every", "7", "--r2l_occ_res", "600", "--raw_noise_std", "1"])
    assert args.r2l_occ_train is True and args.r2l_occ_every == 7
    validate_occupancy(args)  # (--r2l_occupancy is off: the res of 600 and the noise are not theirs to judge)
    validate_occ_fused(args, ("r2l_fused_frames",))
    import main as main_py  # noqa: F401  (the entry points import with the option table as it stands)
    from r2l_amd import create_data, driver
    for mod in (driver, create_data):
        src = open(mod.__file__).read()
        assert "r2l_occ_train" not in src and "r2l_occ_every" not in src, mod.__name__


@pytest.mark.parametrize("K", [1, 2, 7])
def test_refresh_schedule_is_pure(K):
    """occ_refresh_base(i, K) = K floor((i - 1) / K): the grids of iteration i come from the weights after that iteration, whether
    the run started at 0 or resumed anywhere — and TrainOccupancy refreshes exactly when the next iteration's base changes."""
    from r2l_amd.options import occ_refresh_base
    N = 30
    base = [occ_refresh_base(i, K) for i in range(1, N + 1)]
    assert base[0] == 0 and all(b % K == 0 and i - K <= b < i for i, b in zip(range(1, N + 1), base))
    for resume in (0, 1, K, K + 1, 2 * K + 3):  # a run that starts after iteration `resume` asks the same question
        assert [occ_refresh_base(i, K) for i in range(resume + 1, N + 1)] == base[resume:]
    refreshed_after = [i for i in range(1, N) if i % K == 0]  # TrainOccupancy.after_step
    assert refreshed_after == [i for i in range(1, N) if occ_refresh_base(i + 1, K) != occ_refresh_base(i, K)]
    with pytest.raises(ValueError):
        occ_refresh_base(0, K)


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, *a):
        self.lines.append(" ".join(str(x) for x in a))


def _grid_args(**over):
    from r2l_amd.options import parse_args
    argv = ["--config", LEGO, "--r2l_occ_train", "--r2l_occ_res", "4", "--r2l_occ_bound", "1.5", "--r2l_occ_every", "2"]
    for k, v in over.items():
        argv += ["--" + k, str(v)]
    return parse_args(argv)


def test_checkpoint_key_round_trips(tmp_path):
    """TrainOccupancy.state() through save_ckpt / load_ckpt under its own key: a second run takes the words back without a build;
    another refresh interval, or a checkpoint without the key, rebuilds and says so.  The reference's keys are untouched."""
    from r2l_amd.checkpoint import load_ckpt, save_ckpt
    from r2l_amd.occupancy import TrainOccupancy
    tr, nets = cpu_trainer(N_importance=8)
    log = _Log()
    occ = TrainOccupancy(_grid_args(), nets[0], nets[1], 2., 6., tr, log, start=0)
    assert tr.occupancy == occ.pair() and len(occ.grids) == 2 and sum("built in" in l for l in log.lines) == 2
    occ.grids[0].set_bits(np.arange(2, dtype=np.uint32) * 77 + 5)  # words no build of this net gives
    path = save_ckpt(str(tmp_path / "c.tar"), 2, nets[0], tr.optimizer_state_dict(5e-4), 0., 0, model_name="nerf", model_fine=nets[1],
                     extra={TrainOccupancy.KEY: occ.state()})
    ck = load_ckpt(path, map_location="cpu")
    assert TrainOccupancy.KEY == "r2l_occ_train" and set(ck) >= {"global_step", "network_fn_state_dict", "network_fine_state_dict",
                                                                  "optimizer_state_dict", TrainOccupancy.KEY}
    st = ck[TrainOccupancy.KEY]
    assert st["res"] == 4 and st["every"] == 2 and st["base"] == 0 and st["k"] == 2 and st["dilate"] == 1 and st["bound"] == 1.5
    tr2, nets2 = cpu_trainer(N_importance=8)
    log2 = _Log()
    back = TrainOccupancy(_grid_args(), nets2[0], nets2[1], 2., 6., tr2, log2, start=2, state=dict(st, base=2))
    assert np.array_equal(back.grids[0].words(), occ.grids[0].words()) and np.array_equal(back.grids[1].words(), occ.grids[1].words())
    assert any("restored from the checkpoint" in l for l in log2.lines) and not any("built in" in l for l in log2.lines)
    for state, needle in ((None, "no key"), (dict(st, base=2, every=4), "every")):
        log3 = _Log()
        again = TrainOccupancy(_grid_args(), nets2[0], nets2[1], 2., 6., tr2, log3, start=2, state=state)
        assert any("rebuilt at once" in l and needle in l for l in log3.lines), log3.lines
        assert not np.array_equal(again.grids[0].words(), occ.grids[0].words())


def test_rebuild_is_in_place():
    from r2l_amd.occupancy import OccupancyGrid
    _, nets = cpu_trainer(N_importance=8)
    g = OccupancyGrid([-1.5] * 3, [1.5] * 3, G=4, k=2, dilate=1).build(nets[0])
    want = g.words().copy()
    bits = g.bits
    g.bits.zero_()
    assert g.rebuild(nets[0]).bits is bits and np.array_equal(g.words(), want) and g.build_seconds >= 0


def test_cpu_step_with_pair_is_autograd_of_the_masked_render():
    """TeacherTrainer._cpu_step under a pair of grids: loss and gradients are those of torch autograd over a render whose raw is
    zero where the pass's grid has no live cell (OccupancyGrid.query's rule: live_spec of the fp32 points), and the grids count."""
    from r2l_amd import render
    from r2l_amd.metrics import img2mse
    from r2l_amd.occupancy import OccupancyGrid, live_spec, pack_bits
    R, Ns, Ni = 6, 16, 8  # (cpu_trainer: N_samples 16)
    tr, nets = cpu_trainer(N_importance=Ni)
    rng = np.random.RandomState(3)
    grids = [OccupancyGrid([-3.] * 3, [3.] * 3, G=6, k=1, dilate=0).set_bits(pack_bits(rng.rand(6, 6, 6) < .5)) for _ in range(2)]
    o, d, vd, tgt = batch(R, 1)
    t_rand, u = torch.rand(R, Ns), torch.rand(R, Ni)

    def masked_loss():
        def qfn(pts, v, fn):
            g = grids[0 if fn is nets[0] else 1]
            live = live_spec(g.words(), g.lo, g.inv, g.G, pts.detach().numpy().reshape(-1, 3)).reshape(pts.shape[:-1])
            raw = render.run_network(pts, v, fn, embed_fn=render.get_embedder(10)[0], embeddirs_fn=render.get_embedder(4)[0])
            return torch.where(torch.from_numpy(live)[..., None], raw, torch.zeros_like(raw))
        ones = torch.ones(R, 1)
        ret = render.render_rays(torch.cat([o, d, 2. * ones, 6. * ones, vd], -1).float(), nets[0], qfn, Ns, perturb=1., N_importance=Ni,
                                 network_fine=nets[1], white_bkgd=True, t_rand=t_rand, u=u)
        return img2mse(ret["rgb_map"], tgt) + img2mse(ret["rgb0"], tgt)

    for p in tr.params:
        p.grad = None
    want_loss = masked_loss()
    want = torch.autograd.grad(want_loss, tr.params, allow_unused=True)
    full_loss = tr.step(o, d, vd, 2., 6., tgt, 0., t_rand=t_rand, u=u)[0]  # lr 0: the weights stay, the gradients are left in .grad
    tr.set_occupancy(grids)
    loss = tr.step(o, d, vd, 2., 6., tgt, 0., t_rand=t_rand, u=u)[0]
    assert loss == want_loss.item() and loss != full_loss
    for p, w in zip(tr.params, want):
        assert torch.equal(p.grad, torch.zeros_like(p) if w is None else w)
    assert grids[0].total_points == R * Ns and grids[1].total_points == R * (Ns + Ni)
    assert 0 < grids[0].live_points < R * Ns and 0 < grids[1].live_points < R * (Ns + Ni)
    tr.set_occupancy(None)
    assert tr.step(o, d, vd, 2., 6., tgt, 0., t_rand=t_rand, u=u)[0] == full_loss
    with pytest.raises(ValueError, match="raw_noise_std"):
        from r2l_amd.teacher_train import TeacherTrainer
        TeacherTrainer(nets[0], nets[1], N_samples=Ns, N_importance=Ni, raw_noise_std=1., occupancy=grids)
