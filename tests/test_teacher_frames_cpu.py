"""Teacher frames from poses in one library call (include/r2l_hip.h r2l_draw_uniform / r2l_frame_rays /
r2l_teacher_frames_cfg): what can be checked without a GPU — the argument contract (errors are codes returned before anything
is launched), the work-buffer size, the CLI switch, and the Philox4x32-10 restatement the GPU tests compare the device's
draws with."""
import ctypes

import numpy as np

# ---- numpy restatement of Philox4x32-10 (Salmon et al., SC'11) and of r2l_draw_uniform -------------------------------------
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: uint32 [n,4], key: two uint32 -> uint32 [n,4]."""
    c = [np.asarray(counter, dtype=np.uint64)[:, i] for i in range(4)]
    k0, k1 = int(key[0]), int(key[1])
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & _MASK, p1 >> np.uint64(32), p1 & _MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack(c, 1).astype(np.uint32)


def draw_uniform_np(n, seed, stream_id, i0=0):
    """Elements i0 .. i0 + n - 1 of the stream (seed, stream_id) of r2l_draw_uniform, float32."""
    i = np.arange(i0, i0 + n, dtype=np.uint64)
    b = i >> np.uint64(2)
    ctr = np.stack([b & _MASK, b >> np.uint64(32), np.full_like(b, stream_id & 0xFFFFFFFF), np.full_like(b, stream_id >> 32)], 1)
    w = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))
    word = w[np.arange(n), (i & np.uint64(3)).astype(np.int64)]
    return ((word >> np.uint32(8)).astype(np.float32) * np.float32(2.0**-24)).astype(np.float32)


def test_philox_known_answers():
    """The known-answer vectors of Philox4x32-10 (Random123's kat_vectors: zero, all ones, digits of pi)."""
    for ctr, key, want in (
        ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
        ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
        ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
    ):
        got = philox4x32_10(np.array([ctr], dtype=np.uint32), key)[0]
        assert [int(x) for x in got] == list(want), ([hex(int(x)) for x in got], [hex(x) for x in want])
    u = draw_uniform_np(9, 0, 0)
    assert u.dtype == np.float32 and u[0] == np.float32((0x6627e8d5 >> 8) * 2.0**-24) and (u >= 0).all() and (u < 1).all()
    assert np.array_equal(draw_uniform_np(5, 7, 3, i0=3), draw_uniform_np(8, 7, 3)[3:])  # a pure function of the element index


# ---- argument contract --------------------------------------------------------------------------------------------------
def _desc(**kw):
    from r2l_amd import _lib
    d = _lib.TeacherFrameDesc(H=20, W=24, focal=30., near=2., far=6., N_samples=64, N_importance=128, perturb=1, white_bkgd=1,
                              raw_noise_std=0., chunk_rays=0, seed=1, frame_id0=0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _frames(lib, d, K=1, cfg=None, **ptrs):
    """r2l_teacher_frames_cfg with NULL device pointers except those named in ptrs."""
    names = ["c2w_dev", "focal_dev", "ttab", "u_det", "wstream_coarse", "tparams_coarse", "wstream_fine", "tparams_fine", "rows",
             "rgb", "disp", "acc", "depth", "rgb0", "work", "stream"]
    a = {n: ptrs.get(n) for n in names}
    return lib.r2l_teacher_frames_cfg(a["c2w_dev"], a["focal_dev"], K, ctypes.byref(d) if d is not None else None, a["ttab"],
                                      a["u_det"], a["wstream_coarse"], a["tparams_coarse"], a["wstream_fine"], a["tparams_fine"],
                                      a["rows"], a["rgb"], a["disp"], a["acc"], a["depth"], a["rgb0"], a["work"], a["stream"],
                                      ctypes.byref(cfg) if cfg is not None else None)


def test_invalid_arguments_are_rejected():
    """Every invalid case of the header's contract returns hipErrorInvalidValue (1) before anything is launched — all device
    pointers are NULL here, so this runs without a GPU — and r2l_last_error names the field."""
    from r2l_amd import _lib
    lib = _lib.load()
    err = lambda: lib.r2l_last_error().decode()
    res = _desc()
    res.reserved[2] = 5
    for field, d in ((".H", _desc(H=0)), (".W", _desc(W=0)), ("N_samples", _desc(N_samples=0)),
                     ("N_samples", _desc(N_samples=2, N_importance=4)), ("N_importance", _desc(N_samples=64, N_importance=193)),
                     ("N_samples", _desc(N_samples=257, N_importance=0)),
                     ("N_importance", _desc(N_importance=-1)), ("perturb", _desc(perturb=2)), ("perturb", _desc(perturb=-1)),
                     ("raw_noise_std", _desc(raw_noise_std=.5)), ("near", _desc(near=6., far=6.)), ("far", _desc(near=7., far=6.)),
                     ("chunk_rays", _desc(chunk_rays=-1)), ("reserved", res)):
        assert _frames(lib, d) == 1 and field in err(), (field, err())
        assert lib.r2l_teacher_frames_work_floats(ctypes.byref(d)) == -1 and field in err(), (field, err())
    assert _frames(lib, None) == 1 and "desc" in err()
    assert _frames(lib, _desc(), K=-1) == 1 and "K is negative" in err()
    bad_cfg = _lib.make_config()
    bad_cfg.precision = 9
    assert _frames(lib, _desc(), cfg=bad_cfg) == 1 and "precision" in err()
    bad_cfg = _lib.make_config()
    bad_cfg.reserved[0] = 1
    assert _frames(lib, _desc(), cfg=bad_cfg) == 1 and "reserved" in err()
    # a fine pair that is half NULL (the address of a host word stands in for the other half: the call returns before any use)
    word = ctypes.c_float(0.)
    for half in ("wstream_fine", "tparams_fine"):
        assert _frames(lib, _desc(), **{half: ctypes.addressof(word)}) == 1 and "tparams_fine" in err() and "wstream_fine" in err()
    # the shared row of uniforms is needed exactly when nothing is drawn and there is a fine pass
    assert _frames(lib, _desc(perturb=0)) == 1 and "u_det" in err()
    assert _frames(lib, _desc(perturb=0, N_importance=0)) == 1 and "u_det" not in err() and "c2w_dev" in err()
    assert _frames(lib, _desc()) == 1 and "c2w_dev" in err() and "required pointer" in err()
    assert _frames(lib, _desc(focal=0.)) == 1 and "focal" in err()
    # K == 0 is a successful no-op, whatever the pointers
    assert _frames(lib, _desc(), K=0) == 0
    # the two small entry points
    assert lib.r2l_draw_uniform(None, 4, 1, 2, None) == 1 and "out" in err()
    assert lib.r2l_draw_uniform(None, -1, 1, 2, None) == 1 and "n is negative" in err()
    assert lib.r2l_draw_uniform(None, 0, 1, 2, None) == 0
    assert lib.r2l_frame_rays(None, None, 30., 1, 4, 4, None, None, None, None, None) == 1 and "c2w_dev" in err()
    assert lib.r2l_frame_rays(None, None, 30., 1, 0, 4, None, None, None, None, None) == 1 and "H >= 1" in err()
    assert lib.r2l_frame_rays(None, None, 30., -1, 4, 4, None, None, None, None, None) == 1 and "K is negative" in err()
    assert lib.r2l_frame_rays(None, None, 30., 0, 4, 4, None, None, None, None, None) == 0


def test_work_size():
    """r2l_teacher_frames_work_floats: positive, grows with chunk_rays, chunk_rays = 0 means a whole frame (and no more than
    one: a larger chunk_rays changes nothing); it holds at least the raw[R, S + NI, 4] of one pass."""
    from r2l_amd import _lib
    lib = _lib.load()
    size = lambda **kw: lib.r2l_teacher_frames_work_floats(ctypes.byref(_desc(**kw)))
    hw = 20 * 24
    whole = size(chunk_rays=0)
    assert whole > 0 and whole == size(chunk_rays=hw) == size(chunk_rays=10 * hw)
    assert 0 < size(chunk_rays=1) < size(chunk_rays=100) < size(chunk_rays=hw - 1) < whole
    assert whole >= hw * 192 * 4 and size(N_importance=0) >= hw * 64 * 4
    assert size(N_importance=0) < whole and size(perturb=0) < whole
    assert lib.r2l_teacher_frames_work_floats(None) == -1


def test_flag_parsing(tmp_path):
    """--r2l_fused_frames: a switch, default off; from the command line and from a config file."""
    from r2l_amd.options import parse_args
    assert parse_args([]).r2l_fused_frames is False
    assert parse_args(["--r2l_fused_frames"]).r2l_fused_frames is True
    cfg = tmp_path / "c.txt"
    cfg.write_text("N_samples = 32\nr2l_fused_frames = True\n")
    a = parse_args(["--config", str(cfg)])
    assert a.r2l_fused_frames is True and a.N_samples == 32
    cfg.write_text("r2l_fused_frames = False\n")
    assert parse_args(["--config", str(cfg)]).r2l_fused_frames is False


def test_fused_frames_need_a_gpu():
    """render_frames / frame_rays / draw_uniform are GPU only: on CPU tensors they raise instead of computing something else."""
    import pytest
    import torch
    from r2l_amd import render
    with pytest.raises(NotImplementedError):
        render.frame_rays(torch.eye(4)[None, :3], 4, 4, 10.)
    with pytest.raises(NotImplementedError):
        render.draw_uniform(4, 1, 2, "cpu")
