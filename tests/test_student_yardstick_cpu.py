"""The fp64 yardstick of the student's training step (tests/student_util.py) checked on the CPU: against fp64 autograd of the
oracle, and for the conditions that tests/test_student_backward_gpu.py relies on — the rejected shares, the reference's own fp32
autograd inside the exact-family bar on selected rays, the margin of the selection against the encoder's and the fp16x2
products' documented errors, and that one missing ray is ten times the bar that applies."""
import pytest
import torch

from oracle import r2l_oracle as O
from tests import student_util as S

CPU_SHAPES = [(nb, n) for nb, n in S.SHAPES if n <= 4097]


def case(nb, n, perturb, **kw):
    sd = O.make_state_dict(n_block=nb, seed=S.NET_SEED)
    return sd, S.f64(sd), S.select_case(sd, n, perturb, S.case_seed(nb, n, perturb), **kw)


@pytest.mark.parametrize("nb,n,perturb", [(1, 33, 1.), (3, 200, 0.), (8, 65, 1.), (43, 65, 0.)])
def test_backward64_equals_fp64_autograd(nb, n, perturb):
    """Manual backprop = autograd of O.r2l_forward in fp64 to 1e-12 norm-relative, every tensor, MSE and generic mode; drop = p
    is the autograd of the loss without ray p's term (the 1/N kept)."""
    sd, sd64, c = case(nb, n, perturb)
    emb, tgt = c["emb64"], c["tgt"].double()
    drgb = torch.randn(n, 3, generator=torch.Generator().manual_seed(1)).double() * 1e-3
    p_drop = n // 2
    keep = torch.ones(n, 1, dtype=torch.float64)
    keep[p_drop] = 0.
    for mode in ("mse", "generic", "drop"):
        p = {k: v.clone().requires_grad_(True) for k, v in sd64.items()}
        rgb = O.r2l_forward(p, emb)
        if mode == "mse":
            O.img2mse(rgb, tgt).backward()
            rgb64, loss, g, _ = S.backward64(sd64, emb, tgt)
            assert abs(loss.item() - O.img2mse(rgb, tgt).item()) < 1e-15 and (rgb64 - rgb).abs().max().item() < 1e-15
        elif mode == "generic":
            (rgb * drgb).sum().backward()
            _, _, g, _ = S.backward64(sd64, emb, drgb64=drgb)
        else:
            (((rgb - tgt)**2) * keep).sum().div(3 * n).backward()
            _, _, g, _ = S.backward64(sd64, emb, tgt, drop=p_drop)
        for k in sd:
            assert S.nrel(g[k], p[k].grad) < 1e-12, (mode, k)


@pytest.mark.parametrize("perturb", [0., 1.])
@pytest.mark.parametrize("nb,n", CPU_SHAPES)
def test_conditions_on_selected_rays(nb, n, perturb):
    """Per shape of the GPU table with N <= 4097, both jitter modes:
    - the rejected share of the candidate pool stays under its cap (measured: 5.3 - 5.9 % at n_block 1, 8.3 - 10.7 % at 3,
      16.9 - 19.0 % at 8, 37.9 - 39.5 % at 43);
    - the reference's fp32 autograd, which knows nothing of this file, stays inside the exact families' bars against the yardstick:
      every entry within 3e-6 of its magnitude, every tensor within 1e-5 norm-relative (measured: 3e-7 and 5e-7 at the worst);
    - one missing ray (each probe position) moves every weight tensor by at least 1e-3 norm-relative up to N = 1000 — 100 times
      the exact bar — and, head and body, by at least 10 times the fp16-hi model's own error (measured: 18.6 times at the least).
      At N = 4097 the floor is 1e-4, 10 times the exact bar: in a tensor to which the rays contribute coherently (the tail's,
      the last blocks') one ray is 1 / N = 2.4e-4 of the whole, whatever the ray; measured there 2.4e-4 .. 1.4e-3.
      (N = 1: the one ray IS the step; nothing to drop.)"""
    sd, sd64, c = case(nb, n, perturb)
    assert c["rejected"] <= S.REJECT_CAP[nb], c["rejected"]
    emb, tgt = c["emb64"], c["tgt"].double()
    _, _, want, mags = S.backward64(sd64, emb, tgt)
    _, _, g32 = O.r2l_loss_and_grads(sd, emb.float(), c["tgt"])
    worst_n = max((S.nrel(g32[k], want[k]), k) for k in sd)
    worst_r = S.worst_ratio(g32, want, mags)
    _, _, model, _ = S.backward64(sd64, emb, tgt, round_op=S.half_hi)
    e_model = {k: S.nrel(model[k], want[k]) for k in sd}
    assert e_model["tail.0.weight"] == 0. and e_model["tail.0.bias"] == 0.
    weights = [k for k in sd if k.endswith(".weight")]
    moved, over_model = float("inf"), float("inf")
    if n > 1:
        for p in S.probe_rays(n):
            _, _, gp, _ = S.backward64(sd64, emb, tgt, drop=p)
            for k in weights:
                moved = min(moved, S.nrel(want[k], gp[k]))
                if not k.startswith("tail"):
                    over_model = min(over_model, S.nrel(want[k], gp[k]) / e_model[k])
    print("n_block %d N %d perturb %g: rejected %.3f (first %d candidates for %d rays); fp32 autograd norm-relative %.3g (%s), "
          "per entry %.3g (%s); fp16-hi model %.3g; one ray moves a weight tensor by >= %.3g, >= %.1f x the model's error"
          % (nb, n, perturb, c["rejected"], c["examined"], n, worst_n[0], worst_n[1], worst_r[0], worst_r[1],
             max(e_model.values()), moved, over_model))
    bad = {k: v for k, v in S.entry_violations(g32, want, mags).items() if v}
    assert not bad, bad
    assert worst_n[0] <= S.NREL_BWD, worst_n
    assert moved >= (1e-3 if n <= 1000 else 10 * S.NREL_BWD) and over_model >= 10., (moved, over_model)


@pytest.mark.parametrize("perturb", [0., 1.])
@pytest.mark.parametrize("nb", [3, 8, 43])
def test_selection_margin_against_encoder_and_product_errors(nb, perturb):
    """The rays path's kernels do not see the reference encoding: r2l_sincos is within 1.5 ulp of it and the fp16x2 forwards'
    angle doubling within 8e-7 absolute, and their products carry a relative 2^-21.  Stand-in: the fp64 forward with the
    encoding off by +-8e-7 and every weight by a relative +-2^-21 (random signs; so every product is off by that much, with the
    sign shared by the rays) must flip no mask of a selected ray, and move no pre-activation by more than half of delta.
    Measured: at most 9e-7 of m against delta = 1e-5 (n_block <= 8) and 5e-6 (43)."""
    n = 2048
    sd, sd64, c = case(nb, n, perturb)
    emb = c["emb64"]
    gen = torch.Generator().manual_seed(nb)
    sign = lambda t: torch.randint(0, 2, t.shape, generator=gen).double() * 2 - 1
    off = S.forward64({k: v * (1 + S.PROD_ERR * sign(v)) for k, v in sd64.items()}, emb + S.EMB_ERR * sign(emb))
    ref = S.forward64(sd64, emb)
    flips = sum(int(((a > 0) != (b > 0)).sum().item()) for a, b in zip(off["ts"], ref["ts"]))
    moved = max(((a - b).abs() / m).max().item() for a, b, m in zip(off["ts"], ref["ts"], ref["ms"]))
    print("n_block %d perturb %g: %d masks flipped, pre-activations moved by at most %.3g of m (delta %.1e)"
          % (nb, perturb, flips, moved, c["delta"]))
    assert flips == 0
    assert moved <= 0.5 * c["delta"], moved
