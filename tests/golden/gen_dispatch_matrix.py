"""Dispatch matrix of libr2l_hip.so: what the host-side queries answer over every combination of the dispatch switches.

The fixture dispatch_matrix.npz pins the answers of the library as it was BEFORE the launch plan (csrc/r2l_dispatch.h) replaced
the scattered predicates; tests/test_host_cpu.py::test_dispatch_matrix_matches_recorded walks the same matrix on the library
under test and compares every point.  Record it from a build of the commit whose dispatch is the reference, never from the code
under test (no GPU needed: the queries do no device work):

    git worktree add /tmp/parent <commit> && (cd /tmp/parent && R2L_LIB_DIR=/tmp/parent_lib python -m r2l_amd.build)
    R2L_LIB_PATH=/tmp/parent_lib/libr2l_hip.so python tests/golden/gen_dispatch_matrix.py

Axes (4 341 760 points, ~40 s): R2L_FORCE_VARIANT x R2L_NO_FWD3 x R2L_NO_FWD2 x R2L_NO_BWD2 x R2L_NO_DW2 x R2L_COOPF_TILES
(process environment) x r2l_config.precision x .tiling x .coop_tiles x n_block x N.  Per point, as int8: r2l_variant_for_cfg,
r2l_coop_tiles_for_cfg, r2l_forward_layout_for_cfg(stash 0), (stash 1), r2l_backward_layout_for_cfg, r2l_chain_segments_ok_cfg.
"""
import ctypes
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "dispatch_matrix.npz")

FORCE_VARIANT = (None, "main", "coop16", "coopf", "coop")
ON_OFF = (None, "1")
COOPF_TILES = (None, "1", "2", "3")
ENV_AXES = (("R2L_FORCE_VARIANT", FORCE_VARIANT), ("R2L_NO_FWD3", ON_OFF), ("R2L_NO_FWD2", ON_OFF), ("R2L_NO_BWD2", ON_OFF),
            ("R2L_NO_DW2", ON_OFF), ("R2L_COOPF_TILES", COOPF_TILES))
PRECISION = (0, 1, 2, 3)
TILING = (0, 1, 3, 4)
COOP_TILES = (0, 1, 2, 3)
N_BLOCK = (43, 0)
RAYS = tuple(sorted({1, 31, 32, 33, 6144, 6145, 16352, 16353, 160000, 1 << 21} |
                    {4096 * k + d for k in range(1, 33) for d in (-1, 0, 1)}))
# every other switch the queries could see is cleared while the matrix is walked
OTHER_ENV = ("R2L_DW_EXACT", "R2L_RESERVE_CUS", "R2L_DW_WGS", "R2L_MIXED_MAP")
SHAPE = tuple(len(v) for _, v in ENV_AXES) + (len(PRECISION), len(TILING), len(COOP_TILES), len(N_BLOCK), len(RAYS), 6)


def record(lib, config_type):
    """The whole matrix from `lib` (r2l_amd._lib.load()) as an int8 array of SHAPE.  The process environment is restored."""
    names = [n for n, _ in ENV_AXES] + list(OTHER_ENV)
    saved = {n: os.environ.get(n) for n in names}
    out = np.empty(SHAPE, dtype=np.int8)
    variant, tiles = lib.r2l_variant_for_cfg, lib.r2l_coop_tiles_for_cfg
    fwd, bwd, seg = lib.r2l_forward_layout_for_cfg, lib.r2l_backward_layout_for_cfg, lib.r2l_chain_segments_ok_cfg
    try:
        for n in names:
            os.environ.pop(n, None)
        for env_idx in itertools.product(*(range(len(v)) for _, v in ENV_AXES)):
            for (name, values), i in zip(ENV_AXES, env_idx):
                if values[i] is None:
                    os.environ.pop(name, None)
                else:
                    os.environ[name] = values[i]
            for ip, prec in enumerate(PRECISION):
                for it, tiling in enumerate(TILING):
                    for ic, coop in enumerate(COOP_TILES):
                        cfg = config_type()
                        cfg.precision, cfg.tiling, cfg.coop_tiles = prec, tiling, coop
                        c = ctypes.byref(cfg)
                        rows = [(variant(n, c), tiles(n, nb, c), fwd(n, 0, c), fwd(n, 1, c), bwd(n, c), seg(n, nb, c))
                                for nb in N_BLOCK for n in RAYS]
                        out[env_idx + (ip, it, ic)] = np.asarray(rows, dtype=np.int8).reshape(len(N_BLOCK), len(RAYS), 6)
    finally:
        for n, v in saved.items():
            if v is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = v
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from r2l_amd import _lib
    m = record(_lib.load(), _lib.Config)
    np.savez_compressed(FIXTURE, matrix=m, rays=np.asarray(RAYS, dtype=np.int64))
    print("%s: %d points, %d distinct answer rows, %d bytes (library: %s)" %
          (FIXTURE, m.size // 6, len(np.unique(m.reshape(-1, 6), axis=0)), os.path.getsize(FIXTURE), _lib.LIB_PATH))
