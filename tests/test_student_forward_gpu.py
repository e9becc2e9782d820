"""The student's forward, per ray and per entry of rgb, against fp64 — under every kernel family and through every entry point.

The yardstick and the bars are those of tests/student_util.py (forward_yardstick, forward_bars), checked without a GPU by
tests/test_student_forward_cpu.py: unit = rgb64 (1 - rgb64) mz;
  exact families (main-f32mfma, main-bf16x3, coop16) and the pre-embedded path:
      per entry  |got - rgb64| <= C_FWD unit + EMB rgb64 (1 - rgb64) ||dz / d emb||_1 + 2^-24,
      per case (N >= 1000)  rms((got - rgb64) / unit) <= 4 x the fp32 reference's rms on the same rays + EMB x the L2 term's rms;
  fp16x2 families (main, coopf, coopf2): the same plus 3 e_model per entry and 3 rms(e_model / unit) per case, e_model the error
      of the fp16x2 operand model (student_util.forward16x2) on the same rays.
EMB = 1.5 * 2^-24 (r2l_sincos) for the exact families, 8e-7 (one angle doubling) for the fp16x2 ones, 0 on the pre-embedded
path.  Every candidate ray is used and every entry compared; rgb is written between guard zones; for an fp16x2 family the range
guard is asserted not to have handed the launch to the bf16x3 kernel.

Entry points: forward_rays forward-only (the render kernels) and with a stash (the training forward kernels), perturb 0 and 1;
forward_emb at the precisions of tests/test_forward_gpu.py::test_emb_path_matches_oracle, and with a stash under main / coop16;
forward_pose and forward_poses on K = 3 frames of 7 x 9 and 33 x 31 pixels (tiles straddle frames).  The pose kernels form
their points with the arithmetic of O.sample_test, one operation at a time (-ffp-contract=off): student_util.pose_points32
restates it in numpy fp32, the CPU test finds the two equal to the bit, and the restatement feeds the yardstick.

The fp32 reference behind C_FWD and the rms bars is student_util.forward32, O.r2l_forward's fp32 operations with a pinned
summation order: torch's own fp32 sums as the CPU under it likes, and its rms distance from fp64 differed by a factor 1.45
between two machines on the same rays, which carried the bf16x3 chain from 0.74 to 1.05 of one and the same bar.

Measured on one MI355X (678 tests, 27 s; none above 0.4 s after the first), worst case per group as a fraction of its bar:
  group                                     per entry             per case rms (unit)               max |rgb - rgb64|
  rays, fp32 MFMA / coop16 / bf16x3         0.63  (43, N 4097)    0.80  2.23e-8  (43, N 1000)       2.1e-6
      at n_block 1 / 3 / head x 4           0.15 / 0.17 / 0.15    0.25 / 0.29 / 0.29  <= 5.0e-9     <= 9.3e-7
  rays, fp16x2 (main, coopf, coopf2)        0.24  (43, N 4097)    0.28  2.19e-8  (43, N 1000)       2.1e-6
      at n_block 1 / 3 / head x 4           0.09 / 0.10 / 0.07    0.18 / 0.18 / 0.13  <= 9.0e-9     <= 7.5e-7
  pre-embedded, AUTO / fp32_mfma / stash    0.66  (43, N 4097)    0.73  1.96e-8  (43, N 4097)       1.6e-6
  pre-embedded, bf16x3 (= fp16x2)           0.71  (43, N 4097)    0.81  2.18e-8  (43, N 4097)       1.8e-6
  pose paths, exact / fp16x2                0.40 / 0.17 (43)      0.32 / 0.18  (3 blocks, 3 x 33 x 31)   1.1e-6
With and without a stash every family gives the same figures.  The nearest miss is the bf16x3 chain's rms at 43 blocks: 0.80
of its bar on the rays path, 0.81 on the pre-embedded one (2.2e-8 unit; the fp32-MFMA chains 1.9e-8, the reference 6.7e-9).
At 1 and 3 blocks every exact chain lies within 1.2 of the reference's own rms; at 43 blocks at 2.9 times it.  That is the
order of summation and no defect: the chains add W2 relu(t) + b2 onto the residual stream x INSIDE the matrix unit's
accumulator, one or two products per rounding, so every step rounds at the size of x, where the reference rounds the finished
dot product once against x.  The same order in fp64-formed fp32 steps on the CPU, round to nearest, gives 1.99e-8 (one product
per step) and 1.66e-8 (two), against the kernels' 1.90 - 1.96e-8.
Self-check: against the yardstick of mutant (c) ray 31 lies at 2.9e3 - 2.9e4 of its bar, every other ray at 0.48 at the most.
"""
import ctypes

import pytest
import torch

from oracle import r2l_oracle as O
from tests import student_util as S
from tests.conftest import use_family
from tests.test_forward_gpu import FAMILIES, build_model
from tests.test_teacher_backward_gpu import guarded, guards_intact

pytestmark = pytest.mark.gpu

EXACT = ("main-f32mfma", "main-bf16x3", "coop16")
FP16X2 = ("main", "coopf", "coopf2")
assert set(EXACT) | set(FP16X2) == set(FAMILIES)
POSE_FRAMES = {(7, 9): 10., (33, 31): 40.}  # H, W -> focal; H * W no multiple of 32
K_FRAMES = 3

_CASES = {}


def net(name):
    """(state dict, n_block): 'gain4' is the 2-block net of tests/test_forward_gpu.py::test_small_depth_and_gain (head weight x 4:
    stress on the encoding), a number n the seeded n-block net of the gradient tests."""
    if name == "gain4":
        sd = O.make_state_dict(n_block=2, seed=5)
        sd["head.0.weight"] = sd["head.0.weight"] * 4
        return sd, 2
    return O.make_state_dict(n_block=name, seed=S.NET_SEED), name


def poses():
    return torch.stack([torch.from_numpy(O.pose_spherical(30. * k, -20. - 3 * k, 4.)[:3, :4]) for k in range(K_FRAMES)], 0).float()


def case(name, n, perturb, path="rays"):
    """Inputs and yardstick of one case, computed once (fp64 on the GPU through torch; the fp32 reference on the CPU) and shared by
    the families.  path: 'rays', 'emb' (the encoding rounded through fp32) or ('pose', H, W): the K frames, n = K * H * W."""
    key = (name, n, perturb, path)
    if key not in _CASES:
        sd, nb = net(name)
        c = dict(sd=sd, nb=nb)
        if path in ("rays", "emb"):
            c["o"], c["d"], c["u"], emb64 = S.forward_inputs(n, perturb, S.case_seed(nb, n, perturb), "cuda", through_fp32=(path == "emb"))
            if path == "emb":
                c["emb32"] = emb64.float().contiguous()
                assert torch.equal(c["emb32"].double(), emb64)  # identical to the reference's input to the bit
        else:
            _, H, W = path
            z = O.z_vals(S.N_SAMPLE, S.NEAR, S.FAR)
            pts = [torch.from_numpy(S.pose_points32(p.numpy(), H, W, POSE_FRAMES[(H, W)], z.numpy())) for p in poses()]
            emb64 = S.encode64(torch.cat(pts, 0), "cuda")
            assert emb64.shape[0] == n
        c["Y"] = S.forward_yardstick(sd, emb64, model=True)
        if n > S.MUTANT_RAY and path == "rays":
            c["emb_row"] = emb64[S.MUTANT_RAY:S.MUTANT_RAY + 1].clone()
        _CASES[key] = c
    return _CASES[key]


def engine_of(c):
    from r2l_amd.engine import get_engine
    return get_engine(build_model(c["sd"], c["nb"]))


def stash_of(eng, n):
    slot = int(eng.lib.r2l_stash_slot_floats(n))
    f = dict(dtype=torch.float32, device="cuda")
    return torch.empty((eng.n_block + 1) * slot, **f), torch.empty(max(eng.n_block, 1) * slot, **f)


def finish(eng, family, n, with_stash, whole, rgb):
    """Guards, and for an fp16x2 family: the family under test ran, not the bf16x3 kernel behind its range guard."""
    torch.cuda.synchronize()
    assert guards_intact(whole, rgb.numel()), "write outside rgb"
    if family in FP16X2:
        assert eng.layout_for(n, with_stash) == 2, (family, n, with_stash)
        info = eng.range_info()
        assert info["trips"] == 0 and info["flag"] == 0 and info["scale"] == 1.0, info
    return rgb.view(-1, 3)


def run_rays(c, family, n, perturb, with_stash):
    """R2LEngine.forward_rays's call (r2l_forward_rays_cfg), with rgb between guard zones."""
    from r2l_amd import _lib
    from r2l_amd.engine import _ptr, _stream
    eng = engine_of(c)
    o, d = c["o"].cuda().contiguous(), c["d"].cuda().contiguous()
    t_rand = c["u"].cuda().contiguous() if perturb > 0 else None
    eng.ensure_packed(n, with_stash=with_stash)
    sx, st = stash_of(eng, n) if with_stash else (None, None)
    whole, rgb = guarded(n * 3)
    ztab = eng.ztab(O.z_vals(S.N_SAMPLE, S.NEAR, S.FAR), perturb)
    _lib.check(eng.lib.r2l_forward_rays_cfg(_ptr(o), _ptr(d), _ptr(t_rand), _ptr(ztab), _ptr(eng.wstream), _ptr(eng.flat), eng.n_block,
                                            _ptr(rgb), _ptr(sx), _ptr(st), n, _stream(), eng._cfg()), "r2l_forward_rays")
    return finish(eng, family, n, with_stash, whole, rgb)


def run_emb(c, n, with_stash):
    """R2LEngine.forward_emb's call (r2l_forward_emb_cfg)."""
    from r2l_amd import _lib
    from r2l_amd.engine import W, _ptr, _stream
    eng = engine_of(c)
    eng.ensure_packed()
    sx, st = stash_of(eng, n) if with_stash else (None, None)
    x0 = None
    if not with_stash and eng.effective_config().precision in (_lib.PRECISION["bf16x3"], _lib.PRECISION["fp16x2"]):
        x0 = torch.empty(int(eng.lib.r2l_padded_rows(n)) * W, dtype=torch.float32, device="cuda")
    whole, rgb = guarded(n * 3)
    _lib.check(eng.lib.r2l_forward_emb_cfg(_ptr(c["emb32"]), _ptr(eng.wstream), _ptr(eng.flat), eng.n_block, _ptr(rgb), _ptr(sx), _ptr(st),
                                           n, _ptr(x0), _stream(), eng._cfg()), "r2l_forward_emb")
    torch.cuda.synchronize()
    assert guards_intact(whole, n * 3), "write outside rgb"
    return rgb.view(-1, 3)


def run_pose(c, family, H, W, frames):
    """R2LEngine.forward_pose (frames: one frame index) or forward_poses (None: all K frames, one launch where the host layer makes
    one — pinned cooperative tilings go frame by frame there, and here)."""
    from r2l_amd import _lib
    from r2l_amd.engine import _ptr, _stream
    eng = engine_of(c)
    focal, hw = POSE_FRAMES[(H, W)], H * W
    ztab = None
    c2ws = poses()

    def one(k, out):
        host = (ctypes.c_float * 12)(*c2ws[k].reshape(-1).tolist())
        _lib.check(eng.lib.r2l_forward_pose_cfg(ctypes.cast(host, ctypes.c_void_p), H, W, float(focal), _ptr(ztab), _ptr(eng.wstream),
                                                _ptr(eng.flat), eng.n_block, _ptr(out), _stream(), eng._cfg()), "r2l_forward_pose")
    if frames is not None:
        n = hw
        eng.ensure_packed(n, with_stash=False)
        ztab = eng.ztab(O.z_vals(S.N_SAMPLE, S.NEAR, S.FAR), 0.)
        whole, rgb = guarded(n * 3)
        one(frames, rgb)
    else:
        n = K_FRAMES * hw
        eng.ensure_packed(n, with_stash=False)
        ztab = eng.ztab(O.z_vals(S.N_SAMPLE, S.NEAR, S.FAR), 0.)
        whole, rgb = guarded(n * 3)
        if eng.lib.r2l_variant_for_cfg(n, eng._cfg()) != 0 or eng.lib.r2l_coop_tiles_for_cfg(n, eng.n_block, eng._cfg()):
            n = hw  # (the launches the range guard is asked about)
            eng.ensure_packed(n, with_stash=False)
            for k in range(K_FRAMES):
                one(k, rgb[k * hw * 3:(k + 1) * hw * 3])
        else:
            cd = c2ws.cuda().contiguous()
            _lib.check(eng.lib.r2l_forward_poses_cfg(_ptr(cd), K_FRAMES, H, W, float(focal), _ptr(ztab), _ptr(eng.wstream), _ptr(eng.flat),
                                                     eng.n_block, _ptr(rgb), _stream(), eng._cfg()), "r2l_forward_poses")
    return finish(eng, family, n, False, whole, rgb)


def check(tag, family, got, Y, emb_err, fp16x2):
    assert got.shape == Y["rgb"].shape and bool(torch.isfinite(got).all().item())
    r = S.forward_check(got, Y, emb_err, fp16x2)
    n = got.shape[0]
    p = int(r["ratio"].argmax().item())
    print("FWD %s | %s | %s | per entry %.3f of the bar (ray %d) | rms %.3g unit = %.3f of its bar%s | max abs %.3g"
          % ("fp16x2" if fp16x2 else "exact", family, tag, r["worst"], p, r["rms"], r["rms"] / r["rms_bar"],
             "" if n >= S.RMS_MIN_RAYS else " (not asserted)", (got.double() - Y["rgb"]).abs().max().item()))
    bad = torch.nonzero(r["bad"]).flatten().tolist()
    assert not bad, ("%d rays beyond the per-entry bar" % len(bad), bad[:8], r["ratio"][bad[:8]].tolist())
    if n >= S.RMS_MIN_RAYS:
        assert r["rms"] <= r["rms_bar"], (r["rms"], r["rms_bar"])


def emb_err_of(family):
    return S.EMB_ERR if family in FP16X2 else S.EMB_EXACT


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("with_stash", [False, True], ids=["render", "stash"])
@pytest.mark.parametrize("perturb", [0., 1.])
@pytest.mark.parametrize("nb,n", S.FWD_SHAPES)
def test_rays_path_vs_fp64(nb, n, perturb, with_stash, family, monkeypatch):
    """forward_rays, forward-only (the default of every render launch) and with a stash (the training forward kernels), every
    shape of student_util.FWD_SHAPES, with and without stratified jitter."""
    c = case(nb, n, perturb)
    use_family(monkeypatch, **FAMILIES[family])
    got = run_rays(c, family, n, perturb, with_stash)
    check("rays%s n_block %d N %d perturb %g" % (" + stash" if with_stash else "", nb, n, perturb), family, got, c["Y"],
          emb_err_of(family), family in FP16X2)


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("perturb", [0., 1.])
@pytest.mark.parametrize("n", [33, 1000])
def test_rays_path_head_gain_4_vs_fp64(n, perturb, family, monkeypatch):
    """The 2-block net with the head weight times 4: the encoder's share of the error is four times as large."""
    c = case("gain4", n, perturb)
    use_family(monkeypatch, **FAMILIES[family])
    got = run_rays(c, family, n, perturb, False)
    check("rays, head x 4, N %d perturb %g" % (n, perturb), family, got, c["Y"], emb_err_of(family), family in FP16X2)


@pytest.mark.parametrize("precision", ["auto", "fp32_mfma", "bf16x3", "fp16x2"])
@pytest.mark.parametrize("nb,n", S.FWD_SHAPES)
def test_emb_path_vs_fp64(nb, n, precision, monkeypatch):
    """forward_emb forward-only at every precision of the engine (AUTO / fp32_mfma: the exact-fp32 kernel; bf16x3, and fp16x2
    alike: head on the fp32 MFMA, body and tail on the bf16x3 chain): the input is the reference's to the bit, EMB = 0, exact bars."""
    c = case(nb, n, 1., path="emb")
    use_family(monkeypatch, precision=precision)
    check("emb n_block %d N %d" % (nb, n), "emb-" + precision, run_emb(c, n, False), c["Y"], 0., False)


@pytest.mark.parametrize("tiling", ["main", "coop16"])
@pytest.mark.parametrize("nb,n", S.FWD_SHAPES)
def test_emb_path_with_stash_vs_fp64(nb, n, tiling, monkeypatch):
    """forward_emb with a stash (the call of r2l_amd/autograd.py): the exact-fp32 kernels, row-major stash."""
    c = case(nb, n, 1., path="emb")
    use_family(monkeypatch, tiling=tiling)
    check("emb + stash n_block %d N %d" % (nb, n), "emb-" + tiling, run_emb(c, n, True), c["Y"], 0., False)


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("nb,H,W", [(3, 7, 9), (3, 33, 31), (43, 7, 9)])
def test_pose_paths_vs_fp64(nb, H, W, family, monkeypatch):
    """forward_poses on K = 3 frames whose H * W is no multiple of 32 (tiles straddle frames), then forward_pose on the last frame:
    the same bars as the rays path against the yardstick on the kernels' own fp32 points."""
    hw = H * W
    c = case(nb, K_FRAMES * hw, 0., path=("pose", H, W))
    use_family(monkeypatch, **FAMILIES[family])
    many = run_pose(c, family, H, W, None)
    check("poses n_block %d %d x %d x %d" % (nb, K_FRAMES, H, W), family, many, c["Y"], emb_err_of(family), family in FP16X2)
    k = K_FRAMES - 1
    one = run_pose(c, family, H, W, k)
    Yk = {key: v[k * hw:(k + 1) * hw] for key, v in c["Y"].items()}
    check("pose n_block %d frame %d of %d x %d" % (nb, k, H, W), family, one, Yk, emb_err_of(family), family in FP16X2)


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("H,W", list(POSE_FRAMES))
def test_pose_mode_equals_rays_mode_on_frame_rays(H, W, family, monkeypatch):
    """The pose mode of every forward chain forms the ray of a pixel with the pixel_ray of csrc/r2l_pixel_ray.h, the one that
    r2l_frame_rays writes (csrc/r2l_student_net.h): so a pose-mode launch and a rays-mode launch on the rows render.frame_rays
    gives for the same poses are the same arithmetic on the same bits, and their rgb is equal bit for bit — no tolerance.
    7 x 9: two tiles, the second ragged; 33 x 31: more than one workgroup in every family; K frames by the pose table where the
    family takes one (tiles straddle frames), then the last frame by value."""
    from r2l_amd import render
    sd, nb = net(3)
    hw = H * W
    use_family(monkeypatch, **FAMILIES[family])
    o, d, _ = render.frame_rays(poses().cuda(), H, W, POSE_FRAMES[(H, W)])
    for frames, rows in ((None, slice(0, K_FRAMES * hw)), (K_FRAMES - 1, slice((K_FRAMES - 1) * hw, K_FRAMES * hw))):
        by_pose = run_pose(dict(sd=sd, nb=nb), family, H, W, frames).clone()
        c = dict(sd=sd, nb=nb, o=o[rows], d=d[rows], u=None)
        by_rays = run_rays(c, family, by_pose.shape[0], 0., False)
        differ = int((by_pose.view(torch.int32) != by_rays.view(torch.int32)).any(1).sum().item())
        print("POSE == RAYS | %s | %d x %d, %s | %d of %d rays differ" % (family, H, W, "K frames" if frames is None else "one frame",
                                                                        differ, by_pose.shape[0]))
        assert differ == 0, (family, H, W, frames, differ)


@pytest.mark.parametrize("family", ["main-f32mfma", "coop16", "main"])
@pytest.mark.parametrize("nb,n", S.FWD_SELF_CHECK_SHAPES)
def test_bars_see_one_feature_of_one_ray(nb, n, family, monkeypatch):
    """Self-check of the bars on the device, two exact families and one fp16x2 family: against the yardstick of mutant (c) — ray
    31's last encoding feature zeroed — the kernel's unchanged output must fail the per-entry bar at that ray and pass at every
    other.  The device is never asked to misbehave."""
    perturb = 1.
    c = case(nb, n, perturb)
    use_family(monkeypatch, **FAMILIES[family])
    got = run_rays(c, family, n, perturb, False)
    fp16 = family in FP16X2
    assert not bool(S.forward_check(got, c["Y"], emb_err_of(family), fp16)["bad"].any())
    r = S.forward_check(got, S.mutant_c(c["Y"], c["sd"], c["emb_row"], model=True), emb_err_of(family), fp16)
    p = S.MUTANT_RAY
    others = torch.arange(n, device=r["bad"].device) != p
    print("n_block %d N %d %s: against mutant (c) ray %d is at %.3g of its bar, every other ray at most %.3g"
          % (nb, n, family, p, r["ratio"][p].item(), r["ratio"][others].max().item()))
    assert bool(r["bad"][p]) and not bool(r["bad"][others].any())
