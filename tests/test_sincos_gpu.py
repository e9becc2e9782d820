"""The encoder's sin / cos in isolation (csrc/r2l_common.h r2l_sincos, r2l_sincos_double) against fp64, at the bars its comments
state: 1.5 ulp of the true value over |x| <= 4096, and 8e-7 absolute after one angle doubling.  A probe kernel of a few lines
(tests/kernels/sincos_probe.hip) is built with the library's compiler flags — -ffp-contract=off matters — passed through the
ISA audit of r2l_amd/build.py, and loaded with ctypes."""
import ctypes
import glob
import math
import os
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP_BAR = 1.5
DOUBLE_BAR = 8e-7


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    from r2l_amd import build as B
    out = tmp_path_factory.mktemp("sincos_probe")
    so = str(out / "libsincos_probe.so")
    cmd = [B.HIPCC] + B.FLAGS + ["-save-temps=obj", "-shared", "-I", os.path.join(ROOT, "include"), "-I", B.CSRC,
                                 os.path.join(ROOT, "tests", "kernels", "sincos_probe.hip"), "-o", so]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(out))
    assert r.returncode == 0, r.stdout + r.stderr
    asm = [t for t in glob.glob(str(out / "*.s")) if "-hip-amdgcn" in t]
    assert asm, "no device assembly to audit"
    for t in asm:
        with open(t) as f:
            text = f.read()
        B.audit_isa(text, "sincos_probe.hip")
        assert "v_fma_f32" in text or "v_fmac_f32" in text  # the requested FMAs are there ...
    lib = ctypes.CDLL(so)
    lib.sincos_probe.restype = ctypes.c_int
    lib.sincos_probe.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]

    def run(x):
        """x: fp32 numpy array -> [n,4] fp32 numpy: sin, cos, doubled sin, doubled cos."""
        xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
        res = torch.full((xd.numel(), 4), float("nan"), dtype=torch.float32, device="cuda")
        rc = lib.sincos_probe(xd.data_ptr(), res.data_ptr(), xd.numel(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0, rc
        return res.cpu().numpy()
    return run


def ulp_of(v):
    """fp32 ulp at the magnitude of the fp64 value v (subnormals: the smallest normal's)."""
    _, e = np.frexp(np.abs(v))
    return np.ldexp(1.0, np.maximum(e, -125) - 24)


def errors(run, x):
    """(worst ulp error of sin / cos with its argument, worst absolute error of the doubled pair) against fp64 sin / cos of the
    same fp32 arguments."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    got = run(x).astype(np.float64)
    assert np.isfinite(got).all()
    xd = x.astype(np.float64)
    s, c = np.sin(xd), np.cos(xd)
    e = np.maximum(np.abs(got[:, 0] - s) / ulp_of(s), np.abs(got[:, 1] - c) / ulp_of(c))
    i = int(np.argmax(e))
    dbl = max(np.abs(got[:, 2] - np.sin(2 * xd)).max(), np.abs(got[:, 3] - np.cos(2 * xd)).max())
    return float(e[i]), float(x[i]), float(dbl)


def test_sincos_on_the_encoders_arguments(probe):
    """2^k x for k <= 9 with x drawn as the coordinates of sample points o + d z (origins around (0, 0, 4) and wide ones, z in
    [2, 6]), |x| < 8: r2l_sincos within 1.5 ulp of the true value, one doubling within 8e-7 absolute.  Measured on one MI355X:
    1.482 ulp (x = -625.302) and 2.11e-7; the ulp bar is tight."""
    g = torch.Generator().manual_seed(0)
    n = 400000
    o = torch.randn(n, 3, generator=g) * torch.tensor([0.3, 1.5])[torch.randint(0, 2, (n, 1), generator=g)].reshape(n, 1)
    o = o + torch.tensor([0., 0., 4.]) * (torch.rand(n, 1, generator=g) < 0.5)
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    pts = (o + d * (2. + 4. * torch.rand(n, 1, generator=g))).reshape(-1)
    pts = pts[pts.abs() < 8].numpy()
    worst_u, worst_d = 0., 0.
    for k in range(10):
        u, at, dbl = errors(probe, pts * np.float32(2 ** k))
        print("k = %d, %d arguments: %.3f ulp (x = %r), doubling %.3g" % (k, pts.size, u, at, dbl))
        worst_u, worst_d = max(worst_u, u), max(worst_d, dbl)
    assert worst_u <= ULP_BAR, worst_u
    assert worst_d <= DOUBLE_BAR, worst_d


def test_sincos_sweep_to_4096(probe):
    """A dense sweep of |x| <= 4096 (8M points), a denser one of |x| <= 8, the four fp32 neighbours on either side of every
    multiple of pi/2 in range (where the reduced argument cancels), +-0, the smallest normals and +-4096.  Measured on one
    MI355X: dense 1.472 ulp (x = -2843.016), next to k pi/2 1.088 ulp, doubling 2.06e-7."""
    dense = np.linspace(-4096., 4096., 8000001).astype(np.float32)
    small = np.linspace(-8., 8., 2000001).astype(np.float32)
    near = [(np.arange(-2607, 2608) * (math.pi / 2)).astype(np.float32)]
    for direction in (np.inf, -np.inf):
        v = near[0]
        for _ in range(4):
            v = np.nextafter(v, np.float32(direction))
            near.append(v)
    tiny = np.float32(np.finfo(np.float32).tiny)
    edge = np.array([0., -0., tiny, -tiny, 1e-20, 4096., -4096., np.nextafter(np.float32(4096.), np.float32(0.))], dtype=np.float32)
    for name, x in (("dense", dense), ("|x| <= 8", small), ("next to k pi/2", np.concatenate(near)), ("edges", edge)):
        assert np.abs(x).max() <= 4096.
        u, at, dbl = errors(probe, x)
        print("%s, %d arguments: %.3f ulp (x = %r), doubling %.3g" % (name, x.size, u, at, dbl))
        assert u <= ULP_BAR, (name, u, at)
        assert dbl <= DOUBLE_BAR, (name, dbl)
    got = probe(np.array([0., -0.], dtype=np.float32))
    assert got[0, 0] == 0. and got[1, 0] == 0. and got[0, 1] == 1. and got[1, 1] == 1.
