"""Early ray termination of the teacher's render, on the GPU (include/r2l_hip.h "early ray termination"): r2l_occ_index_seg
against its numpy spec, r2l_ert_advance against fp64, r2l_teacher_mlp_live_into_cfg against the zero-filling call in every kernel
family, the staged render against the masked full render bit for bit, the bound on the whole frame, the fused frames call
against the staged render bit for bit, and the argument refusals."""
import ctypes

import numpy as np
import pytest
import torch

from r2l_amd import _lib
from r2l_amd import ert as E
from r2l_amd import occupancy as OC
from tests import ert_util as EU
from tests import occ_fused_util as FU
from tests import occupancy_util as U
from tests.teacher_util import forward_inputs, trained_like_pair

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOX = 1.6
NEAR, FAR = 2., 6.
F32 = np.float32
EPS = 1e-3


def _module(sd):
    from r2l_amd.nerf_raybased import NeRF
    m = NeRF(D=8, W=256, input_ch=63, output_ch=4, skips=[4], input_ch_views=27, use_viewdirs=True)
    m.load_state_dict(sd)
    for p in m.parameters():
        p.requires_grad = False
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def nets():
    return [_module(sd) for sd in trained_like_pair()]


@pytest.fixture(scope="module")
def grids64(nets):
    return tuple(OC.OccupancyGrid([-BOX] * 3, [BOX] * 3, G=64, k=2, dilate=1).build(n) for n in nets)


@pytest.fixture(params=["fp32_mfma", "default", "bf16x3"])
def family(request, monkeypatch):
    from tests.conftest import use_family
    use_family(monkeypatch, **({} if request.param == "default" else {"precision": request.param}))
    return request.param


def _cuda(*arrays):
    return [(a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(DEV).contiguous() for a in arrays]


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. the index of a segment ---------------------------------------------------------------------------------------------
# (R, S, s0, s1): R*(s1-s0) = 1, 2047, 2048, 2049 (the 2048 samples of a workgroup) and 2 099 200 (1025 workgroups: the scan's
# threads own more than one count); width 1, s0 > 0, s1 == S and s1 < S
SEG_CASES = [(1, 1, 0, 1), (2047, 3, 1, 2), (1024, 5, 3, 5), (683, 7, 2, 5), (16400, 130, 1, 129)]


def _trans_mix(R, eps, seed):
    rs = np.random.RandomState(seed)
    eps = F32(eps)
    pool = np.array([np.nextafter(eps, F32(0)), eps, np.nextafter(eps, F32(1)), 0., np.nan, 1., 0.5 * eps, 2 * eps], dtype=F32)
    t = pool[rs.randint(0, pool.size, size=R)]
    t[:min(R, pool.size)] = pool[:min(R, pool.size)]
    return t


@pytest.mark.parametrize("kind", [None, "random", "empty"])
@pytest.mark.parametrize("R,S,s0,s1", SEG_CASES)
def test_index_seg_equals_the_spec(R, S, s0, s1, kind):
    G = 32
    grid = None if kind is None else U.grid_with_bits(G, kind, seed=R, device=DEV)
    o, d, _, z = U.edge_rays(R * S, S, G, seed=2)
    assert z.shape == (R, S)
    spec_grid = None if grid is None else (grid.words(), grid.lo, grid.inv, G)
    to, td, tz = _cuda(o, d, z)
    W = s1 - s0
    lib = _lib.load()
    idx = torch.empty(R * W + 8, dtype=torch.int64, device=DEV)
    cnt = torch.empty(1, dtype=torch.int64, device=DEV)
    work = torch.empty(max(lib.r2l_occ_index_seg_work_bytes(R * W), 16), dtype=torch.uint8, device=DEV)
    for name, trans in (("none", None), ("mix", _trans_mix(R, EPS, R)), ("all terminated", np.zeros(R, dtype=F32))):
        M, want = E.index_seg_spec(spec_grid, o, d, z, s0, s1, trans=trans, eps=EPS)
        tt = None if trans is None else _cuda(trans)[0]
        for call in range(2):
            idx.fill_(-9)
            cnt.fill_(-1)
            E.index_seg(grid, to, td, tz, s0, s1, tt, EPS, idx, cnt, work)
            assert int(cnt[0]) == M, (name, int(cnt[0]), M)
            assert np.array_equal(idx[:M].cpu().numpy(), want), name
            assert bool((idx[M:] == -9).all())  # entries at and past the count are not written
        if name == "all terminated":
            assert M == 0
        if name == "mix" and kind != "empty" and R >= 8:
            assert 0 < M < R * W
        if name == "none" and kind is None:
            assert M == R * W


# ---- 2. the transmittance through a segment ------------------------------------------------------------------------------------
def _advance_inputs(R, S, seed):
    """sigma from -100 to 1000: most samples thin (so that the product stays away from 0 for a while), some empty, some opaque."""
    rs = np.random.RandomState(seed)
    sig = np.where(rs.rand(R, S) < 0.6, rs.rand(R, S) * 2., np.where(rs.rand(R, S) < 0.5, -100. * rs.rand(R, S), 1000. * rs.rand(R, S)**4))
    sig[0, 0], sig[min(1, R - 1), S - 1] = -100., 1000.
    raw = rs.randn(R, S, 4).astype(F32)
    raw[..., 3] = sig.astype(F32)
    z = np.sort(rs.rand(R, S) * 4. + 2., -1).astype(F32)
    d = (rs.randn(R, 3) * 0.7).astype(F32)
    return raw, z, d


@pytest.mark.parametrize("S", [2, 64, 192, 256])
def test_advance_against_fp64(S):
    R = 77  # three workgroups of 32 rays, the last one partly filled
    raw, z, d = _advance_inputs(R, S, S)
    traw, tz, td = _cuda(raw, z, d)
    cuts = sorted({1, S // 3, S // 2, S - 1, S} - {0})
    worst = 0.
    for s1 in cuts:
        trans = torch.full((R + 8,), 7., device=DEV)  # s0 == 0 ignores what trans held; nothing behind R is written
        E.advance(traw, tz, td, 0, s1, trans)
        got = trans[:R].cpu().numpy()
        assert bool((trans[R:] == 7.).all())
        want = E.advance_spec(raw, z, d, 0, s1, dtype=np.float64)
        err = np.abs(got.astype(np.float64) - want).max()
        worst = max(worst, err / (s1 * 2.**-22))
        print("S %d, s1 %d: max |T - T64| = %.3e, the bar s1 * 2^-22 = %.3e; T64 from %.3e to %.3e" % (S, s1, err, s1 * 2.**-22, want.min(), want.max()))
        assert err <= s1 * 2.**-22, (S, s1, err)
        if s1 > 1:  # two chained calls equal the one call bit for bit
            for a in sorted({1, s1 // 2, s1 - 1}):
                t2 = torch.full((R,), -3., device=DEV)
                E.advance(traw, tz, td, 0, a, t2)
                E.advance(traw, tz, td, a, s1, t2)
                assert torch.equal(_bits(t2), _bits(trans[:R])), (S, a, s1)
    print("S %d: worst error / bar = %.3f" % (S, worst))


# ---- 3. the point network written into raw in place -------------------------------------------------------------------------------
def _into_call(eng, o, d, v, z, idx, cnt, capacity, raw_buf):
    E.mlp_live_into(eng, o, d, v, z, idx, cnt, capacity, raw_buf)


def test_live_into_equals_the_zero_filling_call(family, nets):
    from r2l_amd.render import teacher_engine
    eng = teacher_engine(nets[1])
    R, S = 37, 64
    n = R * S
    o, d, v, z = _cuda(*forward_inputs(R, S, "trained", seed=4))
    perm = torch.from_numpy(np.random.RandomState(n).permutation(n).astype(np.int64)).to(DEV)
    full = eng.mlp(o, d, v, z).reshape(n, 4)
    assert int((_bits(full) == 0).sum()) == 0
    for count in (n, 1000, 129, 1):
        cnt = torch.tensor([count], dtype=torch.int64, device=DEV)
        want = eng.mlp_live(o, d, v, z, perm, cnt)
        # (a) on a pre-zeroed raw with capacity R*S: the zero-filling call, bit for bit
        raw = torch.zeros(n * 4 + 64, device=DEV)
        raw[n * 4:] = -7.
        _into_call(eng, o, d, v, z, perm, cnt, n, raw)
        assert torch.equal(_bits(raw[:n * 4]), _bits(want.reshape(-1))) and bool((raw[n * 4:] == -7.).all()), count
        # (b) on a sentinel-filled raw: every entry not in the list keeps the sentinel
        raw = torch.full((n * 4 + 64,), -7., device=DEV)
        _into_call(eng, o, d, v, z, perm, cnt, n, raw)
        r = raw[:n * 4].view(n, 4)
        listed = torch.zeros(n, dtype=torch.bool, device=DEV)
        listed[perm[:count]] = True
        assert torch.equal(_bits(r[listed]), _bits(full[listed])) and bool((r[~listed] == -7.).all()) and bool((raw[n * 4:] == -7.).all())
    # (c) a capacity below the count truncates: the launch is sized for the capacity, entries past it are not read
    cnt = torch.tensor([1000], dtype=torch.int64, device=DEV)
    for capacity in (500, 128, 1, 0):
        idx = torch.cat([perm[:capacity], torch.full((300,), n + 5, dtype=torch.int64, device=DEV)])  # (a read past it would show)
        raw = torch.full((n * 4,), -7., device=DEV)
        _into_call(eng, o, d, v, z, idx, cnt, capacity, raw)
        r = raw.view(n, 4)
        listed = torch.zeros(n, dtype=torch.bool, device=DEV)
        listed[perm[:capacity]] = True
        assert torch.equal(_bits(r[listed]), _bits(full[listed])) and bool((r[~listed] == -7.).all()), capacity
    # (d) count 0 writes nothing; an entry outside [0, R*S) writes nothing at that number
    raw = torch.full((n * 4,), -7., device=DEV)
    _into_call(eng, o, d, v, z, perm, torch.zeros(1, dtype=torch.int64, device=DEV), n, raw)
    assert bool((raw == -7.).all())
    bad = perm[:200].clone()
    bad[5], bad[70] = n, -1
    _into_call(eng, o, d, v, z, bad, torch.tensor([200], dtype=torch.int64, device=DEV), 200, raw)
    assert int((raw.view(n, 4) != -7.).any(-1).sum()) == 198


# ---- 4. the staged render equals the masked full render ---------------------------------------------------------------------------
def _rays():
    return EU.centre_rays().to(DEV)


def _draws(R, Ns, Ni, perturb):
    if not perturb:
        return None, None
    from r2l_amd.render import draw_uniform
    return draw_uniform(R * Ns, 77, 0, DEV).view(R, Ns), (draw_uniform(R * Ni, 77, 1, DEV).view(R, Ni) if Ni else None)


def _render(nets, rays, Ns, Ni, perturb, white=False, occupancy=None, ert=None, live_acc=None):
    from r2l_amd.render import render_rays
    t_rand, u = _draws(rays.shape[0], Ns, Ni, perturb)
    with torch.no_grad():
        return render_rays(rays, nets[0], None, Ns, N_importance=Ni, network_fine=nets[1], perturb=float(perturb), white_bkgd=white,
                           retraw=True, t_rand=t_rand, u=u, occupancy=occupancy, ert=ert, live_acc=live_acc)


def _last_z(nets, rays, Ns, Ni, perturb, white, occupancy):
    """The depths of the last pass, by the stages of render_rays."""
    from r2l_amd.render import _coarse_z, raw2outputs, sample_pdf_sort, teacher_engine
    o, d, v = rays[:, 0:3].contiguous(), rays[:, 3:6].contiguous(), rays[:, 8:11].contiguous()
    t_rand, u = _draws(rays.shape[0], Ns, Ni, perturb)
    z = _coarse_z(rays[:, 6:7].contiguous(), rays[:, 7:8].contiguous(), Ns, False, float(perturb), False, t_rand)
    if Ni:
        raw0 = occupancy[0].query(nets[0], o, d, v, z) if occupancy else teacher_engine(nets[0]).mlp(o, d, v, z)
        w0 = raw2outputs(raw0, z, d, 0, white)[3]
        z = sample_pdf_sort(z, w0, Ni, det=(perturb == 0), u=u)[1]
    return z


OUTS = ("rgb_map", "disp_map", "acc_map", "depth_map")


@pytest.mark.parametrize("with_grids", [True, False])
@pytest.mark.parametrize("perturb", [0, 1])
@pytest.mark.parametrize("Ns,Ni", [(64, 128), (16, 0)])
def test_staged_render_equals_the_masked_full_render(Ns, Ni, perturb, with_grids, family, nets, grids64):
    from r2l_amd.render import raw2outputs
    rays = _rays()
    R, T = rays.shape[0], Ns + Ni
    occ = grids64 if with_grids else None
    plain = _render(nets, rays, Ns, Ni, perturb, occupancy=occ)  # raw: the FULL raw of the last pass, zero where the grid skips
    z = _last_z(nets, rays, Ns, Ni, perturb, False, occ)
    d = rays[:, 3:6].contiguous()
    for seg in (32, 7, T):
        got = _render(nets, rays, Ns, Ni, perturb, occupancy=occ, ert=(EPS, seg))
        trans_at = [t.cpu().numpy() for t in got["ert_trans"]]
        assert len(trans_at) == len(E.segments(T, seg)) - 1
        if seg >= T:  # one segment, no termination: the grids-only render, bit for bit
            assert torch.equal(_bits(got["raw"]), _bits(plain["raw"]))
            for name in OUTS:
                assert FU.same(got[name], plain[name]), (name, seg)
            continue
        # the mask is restated from the transmittances the library itself held: no rounding decides a mask bit
        tmask = torch.from_numpy(E.ert_mask(trans_at, T, seg, EPS)).to(DEV)
        want_raw = torch.where(tmask[..., None], plain["raw"], torch.zeros_like(plain["raw"]))
        assert torch.equal(_bits(got["raw"]), _bits(want_raw)), seg
        rgb, disp, acc, _, depth = raw2outputs(want_raw, z, d, 0, False)
        for name, want in zip(OUTS, (rgb, disp, acc, depth)):
            assert FU.same(got[name], want), (name, seg)
        if Ni:
            for name in ("rgb0", "disp0", "acc0", "z_std"):
                assert FU.same(got[name], plain[name]), (name, seg)  # the coarse pass and the fine depths are untouched
        # and each transmittance is r2l_ert_advance of the raw the render left (a skipped sample enters as raw = 0)
        for (s0, s1), tr in zip(E.segments(T, seg)[:-1], got["ert_trans"]):
            t2 = torch.empty(R, device=DEV)
            E.advance(got["raw"], z, d, 0, s1, t2)
            assert torch.equal(_bits(t2), _bits(tr)), (seg, s1)
        if seg == 32 and Ni:
            assert 0 < int((~tmask).any(-1).sum()) < R  # some rays stop, some do not


# ---- 5. the bound on the whole frame ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("white", [False, True])
def test_the_bound_holds_on_every_ray(white, nets, grids64):
    Ns, Ni, seg, perturb = 64, 128, 32, 1
    T = Ns + Ni
    rays = _rays()
    R = rays.shape[0]
    acc_occ = torch.zeros(2, dtype=torch.int64, device=DEV)
    acc_ert = torch.zeros(2, dtype=torch.int64, device=DEV)
    plain = _render(nets, rays, Ns, Ni, perturb, white, occupancy=grids64, ert=(EPS, T), live_acc=acc_occ)  # one segment: grids only
    ref = _render(nets, rays, Ns, Ni, perturb, white, occupancy=grids64)
    for name in OUTS:
        assert FU.same(plain[name], ref[name]), name
    got = _render(nets, rays, Ns, Ni, perturb, white, occupancy=grids64, ert=(EPS, seg), live_acc=acc_ert)
    # non-vacuity, from the render WITHOUT early termination: the share of rays whose fp64 transmittance is below eps at a boundary
    z = _last_z(nets, rays, Ns, Ni, perturb, white, grids64)
    t64 = EU.boundary_trans64(plain["raw"].cpu().numpy(), z.cpu().numpy(), rays[:, 3:6].cpu().numpy(), seg)
    share = float(np.any([t < EPS for t in t64], axis=0).mean())
    print("rays below eps = %g at a segment boundary before the last segment: %.1f %% of %d" % (EPS, 100 * share, R))
    assert share >= 0.25, share
    # T_cut: the library's transmittance at the boundary where the ray was terminated (0: never)
    t_cut = np.zeros(R)
    for tr in reversed([t.cpu().numpy() for t in got["ert_trans"]]):
        t_cut = np.where(tr < F32(EPS), tr.astype(np.float64), t_cut)
    bound = t_cut * (1 + 1e-3) + 4 * T * 2.**-24
    drgb = (got["rgb_map"].double() - plain["rgb_map"].double()).abs().amax(-1).cpu().numpy()
    dacc = (got["acc_map"].double() - plain["acc_map"].double()).abs().cpu().numpy()
    ddep = (got["depth_map"].double() - plain["depth_map"].double()).abs().cpu().numpy()
    print("white %d: max |d rgb| %.3e, |d acc| %.3e, |d depth| %.3e; largest T_cut %.3e; terminated rays %d of %d" %
          (white, drgb.max(), dacc.max(), ddep.max(), t_cut.max(), int((t_cut > 0).sum()), R))
    assert (drgb <= bound).all(), float((drgb - bound).max())
    assert (dacc <= bound).all(), float((dacc - bound).max())
    assert (ddep <= FAR * bound).all(), float((ddep - FAR * bound).max())
    assert float(t_cut.max()) < EPS
    a, b = acc_ert.tolist(), acc_occ.tolist()
    print("live points: early termination %d / %d, grids only %d / %d" % (a[0], a[1], b[0], b[1]))
    assert a[1] == b[1] == R * (Ns + T) and a[0] < b[0]


# ---- 6. the fused call equals the staged render --------------------------------------------------------------------------------------
KHW = (2, 37, 29)
CHUNK = 500  # does not divide a frame of 1073 rays


def _fused(nets, Ns, Ni, perturb, occupancy=None, ert=None, live_acc=None, chunk=CHUNK):
    from r2l_amd.render import render_frames
    with torch.no_grad():
        return render_frames(FU.poses(KHW[0]), KHW[1], KHW[2], FU.FOCAL, NEAR, FAR, nets[0], nets[1], Ns, Ni, perturb, True, FU.SEED,
                             frame_id0=FU.FID0, chunk=chunk, occupancy=occupancy, live_acc=live_acc, ert=ert)


def _per_frame(nets, Ns, Ni, perturb, occupancy, ert, live_acc, rays_of_frame, near, far, white):
    from r2l_amd.render import draw_uniform, render_rays
    K, H, W = KHW
    out = {k: [] for k in ("rgb", "disp", "acc", "depth", "rgb0")}
    with torch.no_grad():
        for k in range(K):
            o, d, v = rays_of_frame(k)
            one = torch.ones_like(o[:, :1])
            t_rand = u = None
            if perturb:
                t_rand = draw_uniform(H * W * Ns, FU.SEED, 2 * (FU.FID0 + k), "cuda").view(H * W, Ns)
                u = draw_uniform(H * W * Ni, FU.SEED, 2 * (FU.FID0 + k) + 1, "cuda").view(H * W, Ni) if Ni else None
            r = render_rays(torch.cat([o, d, near * one, far * one, v], -1), nets[0], None, Ns, perturb=float(perturb), N_importance=Ni,
                            network_fine=nets[1], white_bkgd=white, t_rand=t_rand, u=u, occupancy=occupancy, ert=ert, live_acc=live_acc)
            for name, key in (("rgb", "rgb_map"), ("disp", "disp_map"), ("acc", "acc_map"), ("depth", "depth_map"), ("rgb0", "rgb0")):
                out[name].append(r.get(key))
    return {k: (torch.cat(v, 0) if v[0] is not None else None) for k, v in out.items()}


@pytest.mark.parametrize("with_grids", [True, False])
@pytest.mark.parametrize("perturb", [0, 1])
@pytest.mark.parametrize("Ns,Ni", [(64, 128), (16, 0)])
def test_fused_frames_equal_the_staged_render(Ns, Ni, perturb, with_grids, nets, grids64):
    from r2l_amd.render import frame_rays
    K, H, W = KHW
    occ = grids64 if with_grids else None
    T = Ns + Ni
    o, d, v = frame_rays(FU.poses(K), H, W, FU.FOCAL)
    of = lambda k: tuple(t[k * H * W:(k + 1) * H * W].contiguous() for t in (o, d, v))
    for seg in (32, 8, 256):
        acc_f = torch.zeros(2, dtype=torch.int64, device=DEV)
        acc_s = torch.zeros(2, dtype=torch.int64, device=DEV)
        got = _fused(nets, Ns, Ni, perturb, occupancy=occ, ert=(EPS, seg), live_acc=acc_f)
        want = _per_frame(nets, Ns, Ni, perturb, occ, (EPS, seg), acc_s, of, NEAR, FAR, True)
        FU.assert_same_frames(got, want, Ni)
        assert acc_f.tolist() == acc_s.tolist() and acc_f.tolist()[1] == K * H * W * (T + (Ns if with_grids and Ni else 0))
        if seg >= T:  # one segment: the entry point without early termination, bit for bit
            base = _fused(nets, Ns, Ni, perturb, occupancy=occ)
            FU.assert_same_frames(got, base, Ni)
        elif Ni:
            assert acc_f.tolist()[0] < acc_f.tolist()[1]
    whole = _fused(nets, Ns, Ni, perturb, occupancy=occ, ert=(EPS, 32), chunk=0)  # chunking does not change a frame
    part = _fused(nets, Ns, Ni, perturb, occupancy=occ, ert=(EPS, 32))
    FU.assert_same_frames(whole, part, Ni)


@pytest.mark.parametrize("perturb", [0, 1])
def test_fused_ndc_frames_equal_the_staged_render(perturb):
    """Forward-facing rays in NDC, where the grids are refused: early termination alone, on the set-up of tests/test_llff_gpu.py.
    The seeded pair's density is thin — no ray falls below eps here (the printed share is 100 %) — so this holds the NDC entry
    point to the staged render bit for bit and its counters, not a gain."""
    from r2l_amd.render import frame_rays, ndc_rays, render_frames
    from tests.test_llff_gpu import BASE_FOCAL, forward_poses
    from tests.test_teacher_frames_gpu import nets as init_nets
    pair = init_nets()
    K, H, W = KHW
    poses = forward_poses(K, seed=77).cuda()
    Ns, Ni, ert = 64, 64, (0.1, 16)
    o, d, v = frame_rays(poses, H, W, BASE_FOCAL)
    no, nd = ndc_rays(H, W, BASE_FOCAL, 1., o, d)
    of = lambda k: tuple(t[k * H * W:(k + 1) * H * W].contiguous() for t in (no, nd, v))
    acc_f = torch.zeros(2, dtype=torch.int64, device=DEV)
    acc_s = torch.zeros(2, dtype=torch.int64, device=DEV)
    with torch.no_grad():
        got = render_frames(poses, H, W, BASE_FOCAL, 0., 1., pair[0], pair[1], Ns, Ni, perturb, False, FU.SEED, frame_id0=FU.FID0,
                            chunk=CHUNK, ndc=True, ert=ert, live_acc=acc_f)
    want = _per_frame(pair, Ns, Ni, perturb, None, ert, acc_s, of, 0., 1., False)
    FU.assert_same_frames(got, want, Ni)
    assert acc_f.tolist() == acc_s.tolist() and acc_f.tolist()[1] == K * H * W * (Ns + Ni)
    print("NDC frames: live points %d / %d" % tuple(acc_f.tolist()))
    with pytest.raises(ValueError, match="ndc"):
        g = U.grid_with_bits(4, "full", device=DEV)
        render_frames(poses, H, W, BASE_FOCAL, 0., 1., pair[0], pair[1], Ns, Ni, perturb, False, FU.SEED, ndc=True, ert=ert, occupancy=(g, g))


# ---- 7. argument refusals -----------------------------------------------------------------------------------------------------------------
def test_argument_refusals_launch_nothing(nets):
    assert EU.check_refusals() >= 60
    from r2l_amd import engine
    from r2l_amd.render import render_frames, teacher_engine
    lib, p = _lib.load(), _lib.ptr
    eng = teacher_engine(nets[0])
    eng.ensure_packed()
    grid = U.grid_with_bits(5, "full", device=DEV)
    buf = torch.full((256,), 7.5, device=DEV)
    idx = torch.full((64,), -3, dtype=torch.int64, device=DEV)
    cfg = ctypes.byref(engine.merged_config(eng.cfg))
    st = _lib.stream()
    assert lib.r2l_occ_index_seg(ctypes.byref(grid.desc()), p(buf), p(buf), p(buf), 4, 4, 2, 2, None, 0., p(idx), p(idx), p(buf), st) == U.INVALID
    assert lib.r2l_occ_index_seg(None, p(buf), p(buf), p(buf), 4, 4, 0, 2, p(buf), 0., p(idx), p(idx), p(buf), st) == U.INVALID
    assert "eps" in lib.r2l_last_error().decode()
    assert lib.r2l_ert_advance(p(buf), p(buf), p(buf), 4, 4, 0, 5, p(buf), st) == U.INVALID
    assert lib.r2l_teacher_mlp_live_into_cfg(p(buf), p(buf), p(buf), p(buf), p(idx), p(idx), 17, p(eng.wstream), p(eng.flat), p(buf), 4, 4,
                                             st, cfg) == U.INVALID
    assert "capacity" in lib.r2l_last_error().decode()
    for desc, e, g, needle in ((FU.frame_desc(ndc=1), _lib.ErtDesc(eps=1e-3, seg=32), grid, "ndc"),
                               (FU.frame_desc(), _lib.ErtDesc(eps=0.5, seg=32), None, "eps"),
                               (FU.frame_desc(), _lib.ErtDesc(eps=1e-3, seg=4), None, "seg"),
                               (FU.frame_desc(), _lib.ErtDesc(eps=1e-3, seg=32, reserved=(ctypes.c_int * 2)(1, 0)), None, "reserved")):
        rc = lib.r2l_teacher_frames_ert_cfg(p(buf), None, 1, ctypes.byref(desc), p(buf), p(buf), p(eng.wstream), p(eng.flat), None, None,
                                            p(buf), p(buf), p(buf), p(buf), p(buf), p(buf), None if g is None else ctypes.byref(g.desc()),
                                            None, p(idx), ctypes.byref(e), p(buf), st, cfg)
        assert rc == U.INVALID and needle in lib.r2l_last_error().decode(), needle
    torch.cuda.synchronize()
    assert bool((buf == 7.5).all()) and bool((idx == -3).all())
    for bad, needle in (((0.5, 32), "eps"), ((1e-3, 4), "seg")):
        with pytest.raises(ValueError, match=needle):
            render_frames(FU.poses(1), 4, 4, FU.FOCAL, NEAR, FAR, nets[0], nets[1], 8, 0, 0, False, 1, ert=bad)


# ---- 8. drivers ---------------------------------------------------------------------------------------------------------------------------
def _sorted_rows(rows):
    a = np.ascontiguousarray(rows, dtype=F32).view(np.uint32)
    return a[np.lexsort(a.T[::-1])]


def test_create_data_store_with_the_switch(tmp_path, monkeypatch, nets, grids64):
    """utils/create_data.py --create_data rand --r2l_store_save --r2l_occ_fused --r2l_ert 1e-3 on the trained-like pair: the one log
    line, the 'ert' entry of the file's provenance, rows that are the library-level frames (the store shuffles a flush group: the
    rows are compared as a set), and a second run that writes the same bytes."""
    import hashlib
    import os
    from r2l_amd import create_data, options
    from r2l_amd import data as D
    from r2l_amd import raystore as RS
    from r2l_amd.render import render_frames
    from tests.test_driver_cpu import ROOT, make_scene
    monkeypatch.chdir(tmp_path)
    csd, fsd = trained_like_pair()
    ck = str(tmp_path / "teacher.tar")
    torch.save({"global_step": 200000, "network_fn_state_dict": csd, "network_fine_state_dict": fsd}, ck)
    scene_dir = str(tmp_path / "scene")
    os.makedirs(scene_dir)
    make_scene(scene_dir, size=128)
    base = ["--create_data", "rand", "--config", os.path.join(ROOT, "configs", "lego.txt"), "--datadir", scene_dir, "--teacher_ckpt", ck,
            "--n_pose_kd", "2", "--create_data_chunk", "2", "--no_rand_focal", "--r2l_occ_fused", "--r2l_occ_res", "64", "--r2l_occ_bound",
            str(BOX)]
    digests, logs = [], []
    for tag in ("a", "b"):
        F = str(tmp_path / (tag + ".r2l"))
        argv = base + ["--experiment_name", "ert_" + tag, "--r2l_store_save", F, "--r2l_ert", "1e-3"]
        out = create_data.main(argv)
        logs.append(open(os.path.join(out["logger"].log_path, "log.txt")).read())
        digests.append(hashlib.sha256(open(F, "rb").read()).hexdigest())
    assert digests[0] == digests[1]
    log = logs[0]
    line = [l for l in log.splitlines() if "live points" in l]
    assert len(line) == 1 and "early termination: eps 0.001, seg 32, live points " in line[0], line
    a, b = [int(x) for x in line[0].split("live points ")[1].split(" (")[0].split(" / ")]
    assert b == 2 * 4096 * (64 + 64 + 128) and 0 < a < b
    prov = RS.read_store_header(F)["provenance"]
    assert prov["ert"] == {"eps": 1e-3, "seg": 32} and prov["occupancy"] == {"res": 64, "bound": BOX, "k": 2, "dilate": 1}
    # the library-level render of the same poses
    args = options.parse_args(argv)
    scene = D.load_scene(args)
    H, W, focal = int(scene.hwf[0]), int(scene.hwf[1]), float(scene.hwf[2])
    assert (H, W) == (64, 64)
    rng = np.random.RandomState(0)
    c2ws = torch.stack([scene.rand_pose(rng)[:3, :4] for _ in range(2)], 0).to(DEV)
    acc = torch.zeros(2, dtype=torch.int64, device=DEV)
    with torch.no_grad():
        want = render_frames(c2ws, H, W, torch.full((2,), focal, device=DEV), scene.near, scene.far, nets[0], nets[1], args.N_samples,
                             args.N_importance, args.perturb, args.white_bkgd, seed=0, frame_id0=1, rows=True, occupancy=grids64,
                             ert=(1e-3, 32), live_acc=acc)["rows"]
    store = RS.RayStore.load(F, DEV)
    got = store.data[:store.n_shards * store.rows_per_file].cpu().numpy()
    store.close()
    assert got.shape == (2 * 4096, 9) and np.array_equal(_sorted_rows(got), _sorted_rows(want.cpu().numpy()))
    assert acc.tolist() == [a, b]
    # without the switch: no such line, no such entry
    F = str(tmp_path / "plain.r2l")
    out = create_data.main(base + ["--experiment_name", "ert_plain", "--r2l_store_save", F])
    plain_log = open(os.path.join(out["logger"].log_path, "log.txt")).read()
    assert "early termination" not in plain_log and "ert" not in RS.read_store_header(F)["provenance"]
    assert "occupancy grid: live points" in plain_log
