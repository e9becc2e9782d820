"""One teacher training step in one library call (include/r2l_hip.h r2l_draw_normal / r2l_teacher_train_step; --r2l_fused_step):
what can be checked without a GPU — the numpy restatement of r2l_draw_normal that the GPU tests compare the device's draws with,
the argument contract (errors are codes returned before anything is launched), the work-buffer size, and the switch."""
import ctypes

import numpy as np
import pytest

from tests.test_teacher_frames_cpu import _MASK, philox4x32_10

STREAMS = [(1, 2), ((1 << 40) + 7, (1 << 62) + 5)]  # (seed, stream_id): small words, and words above 2^32 in both


# ---- numpy restatement of r2l_draw_normal, in fp64 ---------------------------------------------------------------------------
def draw_normal_np(n, seed, stream_id, i0=0, with_r=False):
    """Elements i0 .. i0 + n - 1 of r2l_draw_normal(seed, stream_id, scale = 1) in float64 (with_r: and each element's
    r = sqrt(-2 ln u1))."""
    i = np.arange(i0, i0 + n, dtype=np.uint64)
    b = i >> np.uint64(2)
    ctr = np.stack([b & _MASK, b >> np.uint64(32), np.full_like(b, stream_id & 0xFFFFFFFF), np.full_like(b, stream_id >> 32)], 1)
    w = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).astype(np.int64)
    e = (i & np.uint64(3)).astype(np.int64)
    pair, row = (e >> 1) * 2, np.arange(n)
    u1 = ((w[row, pair] >> 8) + 1).astype(np.float64) * 2.0**-24
    u2 = (w[row, pair + 1] >> 8).astype(np.float64) * 2.0**-24
    r = np.sqrt(-2. * np.log(u1))
    out = r * np.where(e & 1, np.sin(2. * np.pi * u2), np.cos(2. * np.pi * u2))
    return (out, r) if with_r else out


def test_draw_normal_restatement_is_a_function_of_the_element_index():
    for i0 in (1, 2, 3, 5):
        assert np.array_equal(draw_normal_np(9, 7, 3, i0=i0), draw_normal_np(9 + i0, 7, 3)[i0:])
    a = draw_normal_np(8, 7, 3)
    assert not np.array_equal(a, draw_normal_np(8, 8, 3)) and not np.array_equal(a, draw_normal_np(8, 7, 4))
    # the two elements of a pair share r: their squares sum to -2 ln u1
    n, r = draw_normal_np(8, 7, 3, with_r=True)
    assert np.allclose(n[0::2]**2 + n[1::2]**2, r[0::2]**2, rtol=1e-12) and np.array_equal(r[0::2], r[1::2])


@pytest.mark.parametrize("seed,stream_id", STREAMS)
def test_draw_normal_restatement_moments(seed, stream_id):
    """2^20 elements: |mean| sqrt(n) <= 4, |var - 1| / sqrt(2 / n) <= 4 (four standard errors of either moment), and the range
    |n_i| <= sqrt(48 ln 2) = 5.77 that u1 >= 2^-24 gives."""
    n = 1 << 20
    x = draw_normal_np(n, seed, stream_id)
    m, v, top = abs(x.mean()) * np.sqrt(n), abs(x.var() - 1.) / np.sqrt(2. / n), np.abs(x).max()
    print("draw_normal_np(%d, %d): |mean| sqrt(n) %.2f, |var - 1| / sqrt(2/n) %.2f, max |n_i| %.2f" % (seed, stream_id, m, v, top))
    assert m <= 4. and v <= 4. and top <= 5.77, (m, v, top)


# ---- argument contract -------------------------------------------------------------------------------------------------------
def _desc(**kw):
    from r2l_amd import _lib
    d = _lib.TeacherStepDesc(N_rand=32, N_samples=64, N_importance=128, perturb=1, white_bkgd=1, raw_noise_std=0., near=2., far=6.,
                             lr=5e-4, beta1=.9, beta2=.999, eps=1e-8, step=1, seed=1)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


NAMES = ["rays_o", "rays_d", "viewdirs", "target", "ttab", "u_det", "params", "grads", "exp_avg", "exp_avg_sq", "wstream_coarse",
         "wstream_fine", "loss_out", "work"]


def _step(lib, d, **ptrs):
    """r2l_teacher_train_step with NULL device pointers except those named in ptrs."""
    return lib.r2l_teacher_train_step(ctypes.byref(d) if d is not None else None, *[ptrs.get(n) for n in NAMES], None)


def test_invalid_descriptors_are_rejected():
    """Every invalid field makes r2l_teacher_step_work_floats return -1 and r2l_teacher_train_step return hipErrorInvalidValue (1)
    before anything is launched — all device pointers are NULL here — with the field named in r2l_last_error."""
    from r2l_amd import _lib
    lib = _lib.load()
    err = lambda: lib.r2l_last_error().decode()
    res = _desc()
    res.reserved[3] = 1
    for field, d in (("N_rand", _desc(N_rand=0)), ("N_rand", _desc(N_rand=-4)), ("N_samples", _desc(N_samples=0)),
                     ("N_samples", _desc(N_samples=2, N_importance=4)), ("N_importance", _desc(N_samples=64, N_importance=193)),
                     ("N_samples", _desc(N_samples=65, N_importance=128)), ("N_samples", _desc(N_samples=257, N_importance=0)),
                     ("N_importance", _desc(N_importance=-1)), ("perturb", _desc(perturb=2)), ("perturb", _desc(perturb=-1)),
                     ("white_bkgd", _desc(white_bkgd=2)), ("raw_noise_std", _desc(raw_noise_std=-.5)),
                     ("raw_noise_std", _desc(raw_noise_std=float("nan"))), ("near", _desc(near=6., far=6.)),
                     ("far", _desc(near=7., far=6.)), ("step", _desc(step=0)), ("step", _desc(step=-3)),
                     ("step", _desc(step=1 << 60)), ("reserved", res)):
        assert lib.r2l_teacher_step_work_floats(ctypes.byref(d)) == -1 and field in err(), (field, err())
        assert _step(lib, d) == 1 and field in err(), (field, err())
    assert lib.r2l_teacher_step_work_floats(None) == -1 and "desc" in err()
    assert _step(lib, None) == 1 and "desc" in err()
    assert lib.r2l_teacher_step_work_floats(ctypes.byref(_desc(step=(1 << 60) - 1))) > 0


def test_missing_pointers_are_named():
    """The address of a host word stands in for the pointers that are given: the call returns before any use."""
    from r2l_amd import _lib
    lib = _lib.load()
    err = lambda: lib.r2l_last_error().decode()
    word = (ctypes.c_float * 8)()
    at = (ctypes.addressof(word) + 15) & ~15
    given = {n: at for n in NAMES}
    for d, skip in ((_desc(), ()), (_desc(N_importance=0), ("wstream_fine",)), (_desc(perturb=0), ())):
        need = [n for n in NAMES if n not in skip and not (n == "u_det" and d.perturb == 1)]
        for missing in need:
            ptrs = {n: p for n, p in given.items() if n != missing and n not in skip}
            assert _step(lib, d, **ptrs) == 1 and missing in err(), (missing, err())
    # the fine stream goes with N_importance: NULL with a fine pass, or given without one, is refused
    assert _step(lib, _desc(), **{n: p for n, p in given.items() if n != "wstream_fine"}) == 1 and "wstream_fine" in err()
    assert _step(lib, _desc(N_importance=0), **given) == 1 and "wstream_fine" in err() and "N_importance == 0" in err()
    # the shared row of uniforms is needed exactly when nothing is drawn and there is a fine pass
    no_u = {n: p for n, p in given.items() if n != "u_det"}
    assert _step(lib, _desc(perturb=0), **no_u) == 1 and "u_det" in err()
    for d in (_desc(perturb=1), _desc(perturb=0, N_importance=0)):
        ptrs = {n: p for n, p in no_u.items() if n != "work" and not (n == "wstream_fine" and d.N_importance == 0)}
        assert _step(lib, d, **ptrs) == 1 and "u_det" not in err() and "work is NULL" in err(), err()
    assert _step(lib, _desc(), **dict(given, work=at + 4)) == 1 and "16-byte aligned" in err()


def test_draw_normal_arguments():
    from r2l_amd import _lib
    lib = _lib.load()
    err = lambda: lib.r2l_last_error().decode()
    assert lib.r2l_draw_normal(None, 4, 1, 2, 1., None) == 1 and "r2l_draw_normal" in err() and "out" in err()
    assert lib.r2l_draw_normal(None, -1, 1, 2, 1., None) == 1 and "n is negative" in err()
    assert lib.r2l_draw_normal(None, 0, 1, 2, 1., None) == 0


def test_work_size():
    """Non-decreasing in N_rand, no larger without noise than with it, and it holds at least both nets' stashes."""
    from r2l_amd import _lib
    lib = _lib.load()
    size = lambda **kw: lib.r2l_teacher_step_work_floats(ctypes.byref(_desc(**kw)))
    sizes = [size(N_rand=r) for r in (1, 2, 3, 4, 5, 31, 32, 33, 37, 64, 1024, 4096)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]
    for kw in (dict(), dict(N_importance=0), dict(perturb=0), dict(N_rand=37, N_samples=32, N_importance=96)):
        quiet, noisy = size(raw_noise_std=0., **kw), size(raw_noise_std=1., **kw)
        assert 0 < quiet <= noisy, kw
        R, S, T = kw.get("N_rand", 32), kw.get("N_samples", 64), kw.get("N_samples", 64) + kw.get("N_importance", 128)
        assert noisy - quiet >= R * S + (R * T if T > S else 0)
        assert quiet >= lib.r2l_teacher_stash_floats(R * S) + (lib.r2l_teacher_stash_floats(R * T) if T > S else 0) \
            + lib.r2l_teacher_train_work_floats(R * T)
    assert size(N_importance=0) < size() and size(perturb=0) < size()
    assert ctypes.sizeof(_lib.TeacherStepDesc) == 80  # 12 words, two 64-bit fields, 4 reserved words


# ---- the switch --------------------------------------------------------------------------------------------------------------
def test_flag_parsing(tmp_path):
    """--r2l_fused_step: a switch, default off; from the command line and from a config file."""
    from r2l_amd.options import parse_args
    assert parse_args([]).r2l_fused_step is False
    assert parse_args(["--r2l_fused_step"]).r2l_fused_step is True
    cfg = tmp_path / "c.txt"
    cfg.write_text("N_samples = 32\nr2l_fused_step = True\n")
    a = parse_args(["--config", str(cfg)])
    assert a.r2l_fused_step is True and a.N_samples == 32 and a.r2l_batching is False
    cfg.write_text("r2l_fused_step = False\n")
    assert parse_args(["--config", str(cfg)]).r2l_fused_step is False


def test_fused_step_needs_a_gpu(monkeypatch):
    """On a CPU device the switch is refused by name, the wrappers raise instead of computing something else."""
    import torch
    from r2l_amd import render, train_nerf
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for mode in (["--no_batching"], ["--r2l_batching"]):
        with pytest.raises(NotImplementedError, match="GPU") as e:
            train_nerf.main(["--use_viewdirs", "--N_importance", "128", "--r2l_fused_step"] + mode)
        assert "r2l_fused_step" in str(e.value)
    with pytest.raises(NotImplementedError):
        render.draw_normal(4, 1, 2, "cpu")


def test_other_drivers_accept_and_ignore_the_switch():
    import inspect
    import os
    from r2l_amd.options import parse_args, validate_accelerated
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    a = parse_args(["--config", os.path.join(root, "configs", "lego.txt"), "--r2l_fused_step"])
    validate_accelerated(a)  # main.py / create_data.py: nothing reads the switch
    import r2l_amd.create_data as cd
    import r2l_amd.driver as dr
    assert "r2l_fused_step" not in inspect.getsource(cd) and "r2l_fused_step" not in inspect.getsource(dr)
