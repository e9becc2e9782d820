"""Shared by tests/test_occupancy_cpu.py and tests/test_occupancy_gpu.py: hand-made grids, rays whose samples sit on the edges
of the cell rule, and the table of argument refusals of the occupancy calls (include/r2l_hip.h "occupancy grid").  Nothing here
needs a device: the refusals happen before any launch, so the table runs on dummy pointers too."""
import ctypes

import numpy as np
import torch

from r2l_amd import _lib
from r2l_amd import occupancy as OC

F32 = np.float32
INVALID = 1  # hipErrorInvalidValue


def grid_with_bits(G, kind, seed=0, lo=(-1., -1., -1.), hi=(1., 1., 1.), device="cpu"):
    """An OccupancyGrid over [lo, hi) whose bits are 'empty', 'full' or 'random' (half of the cells, seeded)."""
    g = OC.OccupancyGrid(lo, hi, G=G, k=1, dilate=0)
    if kind == "empty":
        occ = np.zeros((G, G, G), dtype=bool)
    elif kind == "full":
        occ = np.ones((G, G, G), dtype=bool)
    else:
        occ = np.random.RandomState(seed + G).rand(G, G, G) < 0.5
    return g.set_bits(OC.pack_bits(occ), device=device)


def edge_rays(n, S, G, seed=0, lo=-1., hi=1.):
    """(o, d, v [R,3], z [R,S]) float32 numpy with R = ceil(n / S) rays through the box [lo, hi)^3 of a G^3 grid.  Most samples are
    random points inside and around the box; every 7th ray is axis-parallel with d = (1, 0, 0), o_x = lo and z on multiples of the
    cell size, so that its samples fall ON cell faces, on the box's faces (z = 0 and z = hi - lo) and outside it; sample 0 of
    every 11th ray has z = NaN, of every 13th z = +inf."""
    R = (n + S - 1) // S
    rs = np.random.RandomState(seed * 7919 + n + 31 * S + G)
    o = (rs.rand(R, 3) * 2.6 - 1.3).astype(F32)
    d = (rs.randn(R, 3) * 0.5).astype(F32)
    z = np.sort(rs.rand(R, S) * 3., -1).astype(F32)
    cell = F32((hi - lo) / G)
    n7 = len(range(0, R, 7))
    o[::7, 0] = lo
    d[::7] = (1., 0., 0.)
    z[::7] = (rs.randint(-1, G + 2, size=(n7, S)).astype(F32) * cell).astype(F32)  # faces of cells, lo (0), hi (G), and beyond both
    o[::14, 1], o[::14, 2] = lo, hi  # y on the lower face (inside), z on the upper face (outside)
    z[::11, 0] = np.nan
    z[::13, 0] = np.inf
    v = (d / np.maximum(np.linalg.norm(d, axis=-1, keepdims=True), 1e-9)).astype(F32)
    return o, d, v, z


def same_bits(a, b):
    """Two float arrays / tensors are the same bit patterns (NaN == NaN, -0 != +0)."""
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a, dtype=F32).view(np.uint32),
                                                 np.ascontiguousarray(b, dtype=F32).view(np.uint32))


def refusals():
    """[(what, call() -> return code, the text r2l_last_error must contain)]: every refusal include/r2l_hip.h lists for the four
    occupancy calls.  The pointers are dummies (never dereferenced: the check comes before any launch)."""
    lib = _lib.load()
    P = ctypes.c_void_p(4096)  # a non-NULL, 16-byte aligned address nobody reads
    NULL = None
    f3 = lambda *v: (ctypes.c_float * 3)(*v)
    lo, hi = f3(-1, -1, -1), f3(1, 1, 1)

    def good(**over):
        g = _lib.OccGridDesc()
        assert lib.r2l_occ_grid_init(ctypes.byref(g), P, 4, 2, lo, hi) == 0
        for k, v in over.items():
            setattr(g, k, v)
        return g

    cases = []
    init = lambda g, bits, G, k, a, b: lib.r2l_occ_grid_init(g, bits, G, k, a, b)
    G0 = _lib.OccGridDesc()
    cases += [
        ("init: NULL grid", lambda: init(NULL, P, 4, 2, lo, hi), "grid"),
        ("init: NULL bits", lambda: init(ctypes.byref(G0), NULL, 4, 2, lo, hi), "bits"),
        ("init: NULL lo", lambda: init(ctypes.byref(G0), P, 4, 2, NULL, hi), "lo"),
        ("init: NULL hi", lambda: init(ctypes.byref(G0), P, 4, 2, lo, NULL), "hi"),
        ("init: G < 1", lambda: init(ctypes.byref(G0), P, 0, 2, lo, hi), "G:"),
        ("init: G > 512", lambda: init(ctypes.byref(G0), P, 513, 2, lo, hi), "G:"),
        ("init: k < 1", lambda: init(ctypes.byref(G0), P, 4, 0, lo, hi), "k:"),
        ("init: k > 4", lambda: init(ctypes.byref(G0), P, 4, 5, lo, hi), "k:"),
        ("init: lo == hi", lambda: init(ctypes.byref(G0), P, 4, 2, lo, f3(1, -1, 1)), "lo"),
        ("init: lo > hi", lambda: init(ctypes.byref(G0), P, 4, 2, f3(-1, 2, -1), hi), "lo"),
        ("init: NaN hi", lambda: init(ctypes.byref(G0), P, 4, 2, lo, f3(1, 1, float("nan"))), "hi"),
    ]
    build = lambda g, k=2, dilate=1, thr=0., w=P, t=P, work=P: lib.r2l_occ_build(g, k, dilate, thr, w, t, None, work, None, None)
    bad_cfg = _lib.Config(precision=99)
    cases += [
        ("build: NULL grid", lambda: build(NULL), "grid"),
        ("build: NULL bits", lambda: build(ctypes.byref(good(bits=None))), "bits"),
        ("build: G < 1", lambda: build(ctypes.byref(good(G=0))), "G:"),
        ("build: G > 512", lambda: build(ctypes.byref(good(G=513))), "G:"),
        ("build: k < 1", lambda: build(ctypes.byref(good()), k=0), "k:"),
        ("build: k > 4", lambda: build(ctypes.byref(good()), k=5), "k:"),
        ("build: dilate < 0", lambda: build(ctypes.byref(good()), dilate=-1), "dilate"),
        ("build: NaN sigma_thresh", lambda: build(ctypes.byref(good()), thr=float("nan")), "sigma_thresh"),
        ("build: lo >= hi (inv)", lambda: build(ctypes.byref(good(inv=f3(2, 0, 2)))), "inv"),
        ("build: lo >= hi (step)", lambda: build(ctypes.byref(good(step=f3(-.25, .25, .25)))), "step"),
        ("build: reserved", lambda: build(ctypes.byref(good(reserved=(ctypes.c_int * 2)(0, 1)))), "reserved"),
        ("build: NULL wstream", lambda: build(ctypes.byref(good()), w=NULL), "wstream"),
        ("build: NULL tparams", lambda: build(ctypes.byref(good()), t=NULL), "tparams"),
        ("build: NULL work", lambda: build(ctypes.byref(good()), work=NULL), "work"),
        ("build: misaligned work", lambda: build(ctypes.byref(good()), work=ctypes.c_void_p(4100)), "work"),
        ("build: bad cfg", lambda: lib.r2l_occ_build(ctypes.byref(good()), 2, 1, 0., P, P, ctypes.byref(bad_cfg), P, None, None),
         "precision"),
    ]

    def compact(g, R=3, S=2, **null):
        names = ["rays_o", "rays_d", "viewdirs", "z", "out_o", "out_d", "out_v", "out_z", "idx_out", "count_out", "work"]
        a = {n: (NULL if null.get(n) else P) for n in names}
        return lib.r2l_occ_compact(g, a["rays_o"], a["rays_d"], a["viewdirs"], a["z"], R, S, a["out_o"], a["out_d"], a["out_v"],
                                   a["out_z"], a["idx_out"], a["count_out"], a["work"], None)

    cases += [("compact: NULL %s" % n, (lambda n=n: compact(ctypes.byref(good()), **{n: True})), n)
              for n in ["rays_o", "rays_d", "viewdirs", "z", "out_o", "out_d", "out_v", "out_z", "idx_out", "count_out", "work"]]
    cases += [
        ("compact: NULL grid", lambda: compact(NULL), "grid"),
        ("compact: reserved", lambda: compact(ctypes.byref(good(reserved=(ctypes.c_int * 2)(7, 0)))), "reserved"),
        ("compact: G > 512", lambda: compact(ctypes.byref(good(G=600))), "G:"),
        ("compact: R < 0", lambda: compact(ctypes.byref(good()), R=-1), "R is negative"),
        ("compact: S < 1", lambda: compact(ctypes.byref(good()), S=0), "S:"),
        ("compact: R*S = 2^31", lambda: compact(ctypes.byref(good()), R=2**23, S=256), "R*S"),
        ("compact: R = 2^40", lambda: compact(ctypes.byref(good()), R=2**40, S=1), "R*S"),
    ]
    scatter = lambda raw_live=P, idx=P, M=2, raw_out=P, R=3, S=2: lib.r2l_occ_scatter(raw_live, idx, M, raw_out, R, S, None)
    cases += [
        ("scatter: R < 0", lambda: scatter(R=-1), "R is negative"),
        ("scatter: S < 1", lambda: scatter(S=0), "S:"),
        ("scatter: R*S = 2^31", lambda: scatter(R=2**23, S=256), "R*S"),
        ("scatter: M < 0", lambda: scatter(M=-1), "M:"),
        ("scatter: M > R*S", lambda: scatter(M=7), "M:"),
        ("scatter: NULL raw_out", lambda: scatter(raw_out=NULL), "raw_out"),
        ("scatter: misaligned raw_out", lambda: scatter(raw_out=ctypes.c_void_p(4104)), "raw_out"),
        ("scatter: NULL raw_live", lambda: scatter(raw_live=NULL), "raw_live"),
        ("scatter: misaligned raw_live", lambda: scatter(raw_live=ctypes.c_void_p(4100)), "raw_live"),
        ("scatter: NULL idx", lambda: scatter(idx=NULL), "idx"),
    ]
    return cases


def check_refusals():
    """Run the table: every case returns hipErrorInvalidValue and r2l_last_error names the argument.  Also the size queries."""
    lib = _lib.load()
    for what, call, needle in refusals():
        rc = call()
        msg = (lib.r2l_last_error() or b"").decode()
        assert rc == INVALID, (what, rc, msg)
        assert needle in msg and "r2l_occ" in msg or needle in msg and "r2l_config" in msg, (what, msg)
    assert lib.r2l_occ_build_work_floats(0, 1) == -1 and lib.r2l_occ_build_work_floats(4, 5) == -1
    assert lib.r2l_occ_build_work_floats(513, 1) == -1 and lib.r2l_occ_bits_words(0) == -1 and lib.r2l_occ_bits_words(513) == -1
    assert lib.r2l_occ_compact_work_bytes(-1) == -1 and lib.r2l_occ_compact_work_bytes(2**31) == -1
    assert lib.r2l_occ_bits_words(5) == 4 and lib.r2l_occ_bits_words(512) == 2**22
    return len(refusals())
