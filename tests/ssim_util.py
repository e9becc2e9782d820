"""Test infrastructure: an fp64 yardstick of the SSIM kernel (csrc/r2l_ssim.hip) per 16 x 16 tile, with derived bars.

The contract (include/r2l_hip.h): partial[(c * tilesY + ty) * tilesX + tx] is the sum of the SSIM map over the pixels of tile
(ty, tx) of channel c that lie inside the image; out[0] is the fixed-order sum of the partials times 1 / (H W C).

Yardsticks
----------
ssim_map64      the oracle's op sequence (oracle/r2l_oracle.py ssim) in fp64 on the fp32 images and the fp32 window values, without
                the final mean -> [H, W, C].  tiles64 sums a map per tile and channel in fp64, in the layout above.
ssim_map32_ref  the same ops in torch fp32 on the CPU: the reference's own arithmetic.  Its distance from ssim_map64 sets the bars.
ssim_map32_seq  a numpy fp32 restatement of the KERNEL's sequence: zero-padded halo, the 121 taps in i, j order, five fused
                multiply-add chains (p p, q q and p q rounded first), the kernel's final expression with C1 = 0.01f * 0.01f and
                C2 = 0.03f * 0.03f.  The fused multiply-add is the fp64 product-sum rounded to fp32: the product of two fp32 numbers
                is exact in fp64, the sum is rounded once to fp64 and once more to fp32.  That double rounding can move a result by
                one fp32 ulp on rare elements (when the fp64 sum lands exactly on an fp32 rounding boundary that the exact sum
                misses).
tiles32_butterfly  the kernel's own summation order of a fp32 map: per wave of four tile rows the xor butterfly 32, 16, 8, 4, 2, 1,
                then (w0 + w1) + (w2 + w3).  finish32 restates r2l_ssim_finish_kernel the same way.  Used for a report only.

Bars (u = 2^-24)
----------------
Per case, for every tile and channel:   |got - tiles64| <= 4 R + TILE_ADDS u sum_tile |map64|
  R = max over the case's tiles of |tiles(ssim_map32_ref) - tiles64|: the reference's own fp32 noise on that case, times the 4 the
  project uses everywhere.  TILE_ADDS = 8: a pixel's value passes through six shuffle additions (offsets 32 ... 1 of the xor
  butterfly) and two additions of the four wave sums out of LDS, (red[0] + red[1]) + (red[2] + red[3]); each rounds by at most u of
  a partial sum, and every partial sum is at most sum_tile |map|.
out[0]:   |got - mean64| <= 4 |mean32_ref - mean64| + (2 TILE_ADDS + turns - 1) u mean|map64| + 2 u |mean64|
  the tile sums' allowance again; the finish kernel's additions on top: a partial passes through turns - 1 = ceil(n / 256) - 1
  additions of its thread's stride loop (the first lands on an exact 0), six shuffle additions and two out of LDS; 1 / (H W C) is
  one rounded division of an exactly representable count (H W C < 2^24 in every case) and the product with it rounds once more.
On the flat and scene kinds R is large (the cancellation in s - mu^2 on a flat bright background: DESIGN.md section 6), fp64 is too
far away to judge a tile, and every tile sum is ALSO held to tiles(ssim_map32_seq):
  |got - tiles(seq)| <= TILE_ADDS u sum_tile |seq| + 2 u (pixels of the tile inside the image)
(2 u: one fp32 ulp of a map value below 2, for the documented double rounding).  The restatement is the specification of the
kernel's order there, as optim_util's fp32 restatement is for Adam.

Mutants: MUTANTS names nine wrong evaluations of the yardstick or of the tile table; tests/test_ssim_cpu.py holds every one out of
the bars on a named case.
"""
import collections
import math
import os

import numpy as np
import torch

U = 2.0**-24
T = 16          # SS_T: the tile
WIN, R = 11, 5  # SS_WIN, SS_R
TILE_ADDS = 8   # 6 shuffle levels + 2 additions of the four wave sums (r2l_ssim_kernel)
FINISH_ADDS = 8  # the same tree in r2l_ssim_finish_kernel, behind its stride loop of 256

SHAPES = [(1, 1, 1), (5, 6, 2), (11, 11, 1), (15, 17, 3), (17, 15, 3), (16, 16, 1), (16, 33, 4), (33, 16, 4), (31, 32, 5),
          (47, 21, 3), (160, 144, 3)]
KINDS = ["tex", "scene97", "scene995", "flat", "dark", "wide"]
SEQ_KINDS = ("scene97", "scene995", "flat")  # held to the restatement as well

# (shape, kind, window): the kinds cycle over the shapes, every shape gets at least two, both orientations of a non-square shape
# get different ones; the asymmetric window (the only one that sees a transposed tap index) on two non-square shapes
_TABLE = [((1, 1, 1), "tex"), ((1, 1, 1), "flat"), ((1, 1, 1), "dark"),
          ((5, 6, 2), "scene97"), ((5, 6, 2), "wide"),
          ((11, 11, 1), "scene995"), ((11, 11, 1), "dark"),
          ((15, 17, 3), "tex"), ((15, 17, 3), "flat"),
          ((17, 15, 3), "scene97"), ((17, 15, 3), "wide"), ((17, 15, 3), "flat"),
          ((16, 16, 1), "dark"), ((16, 16, 1), "scene995"),
          ((16, 33, 4), "tex"), ((16, 33, 4), "scene97"),
          ((33, 16, 4), "flat"), ((33, 16, 4), "wide"),
          ((31, 32, 5), "scene995"), ((31, 32, 5), "dark"), ((31, 32, 5), "tex"),
          ((47, 21, 3), "scene97"), ((47, 21, 3), "wide"),
          ((160, 144, 3), "tex"), ((160, 144, 3), "flat"), ((160, 144, 3), "scene97")]
_ASYM = [((33, 16, 4), "tex"), ((47, 21, 3), "wide")]


def case_name(shape, kind, window="ref"):
    return "%dx%dx%d-%s" % (shape + (kind,)) + ("" if window == "ref" else "-" + window)


CASES = [case_name(s, k) for s, k in _TABLE] + [case_name(s, k, "asym") for s, k in _ASYM]
_SPEC = {case_name(s, k): (s, k, "ref") for s, k in _TABLE}
_SPEC.update({case_name(s, k, "asym"): (s, k, "asym") for s, k in _ASYM})


def report(line):
    """Print a figure (pytest -s; profiles/ssim_yardstick.txt quotes these lines) and, when R2L_YARDSTICK_OUT names a file,
    append it there."""
    line = "YARDSTICK ssim " + line
    print(line)
    path = os.environ.get("R2L_YARDSTICK_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


# ---- windows ------------------------------------------------------------------------------------------------------------------
def window_ref():
    """The window metrics.ssim passes (ssim_torch.py:11-25)."""
    from r2l_amd import metrics
    return metrics._ssim_window().clone()


def window_lib():
    """What r2l_ssim builds for window_host = NULL, restated: the Gaussian from the double exp rounded to fp32, its sum formed in
    double and rounded once, the division in fp32, the outer product in fp32."""
    return _window_lib(False)


def _window_lib(in_order):
    """in_order: the sum in fp32 in index order instead, as the library formed it before: one ulp below, 117 taps off by an ulp."""
    g = np.array([math.exp(-float((x - R) * (x - R)) / (2.0 * 1.5 * 1.5)) for x in range(WIN)]).astype(np.float32)
    s = np.float32(0)
    for v in g:
        s = np.float32(s + v)
    if not in_order:
        s = np.float32(g.astype(np.float64).sum())
    g = (g / s).astype(np.float32)
    return torch.from_numpy((g[:, None] * g[None, :]).astype(np.float32))


def window_asym(seed=7):
    """The reference's values times a seeded factor in [0.5, 1.5] per tap, renormalised to sum 1 in fp32: neither symmetric under
    transposition nor under a flip of either axis."""
    f = 0.5 + torch.rand(WIN, WIN, generator=torch.Generator().manual_seed(seed))
    w = window_ref() * f
    return (w / w.sum()).contiguous()


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def _texture(H, W, C, g):
    """The seeded sine texture of tests/test_metrics_gpu.py::test_ssim_vs_oracle_fullsize."""
    yy, xx = torch.meshgrid(torch.linspace(0, 9, H), torch.linspace(0, 7, W), indexing="ij")
    gt = 0.5 + 0.4 * torch.sin(xx * 1.7 + yy)[..., None] * torch.ones(C) + 0.1 * torch.rand(H, W, C, generator=g)
    return gt.clamp(0, 1)


def make_pair(shape, kind, seed):
    """-> pred, gt [H, W, C] fp32."""
    H, W, C = shape
    g = torch.Generator().manual_seed(seed)
    if kind == "tex":
        gt = _texture(H, W, C, g)
        pred = (gt + 0.05 * torch.randn(H, W, C, generator=g)).clamp(0, 1)
    elif kind in ("scene97", "scene995"):  # white ground truth, textured centre third; the prediction's background is flat
        tex = _texture(H, W, C, g)
        ys, xs = slice(H // 3, max(H - H // 3, H // 3 + 1)), slice(W // 3, max(W - W // 3, W // 3 + 1))
        gt = torch.ones(H, W, C)
        gt[ys, xs] = tex[ys, xs]
        pred = torch.full((H, W, C), 0.97 if kind == "scene97" else 0.995)
        pred[ys, xs] = (tex[ys, xs] + 0.05 * torch.randn(H, W, C, generator=g)[ys, xs]).clamp(0, 1)
    elif kind == "flat":
        gt, pred = torch.ones(H, W, C), torch.full((H, W, C), 0.97)
    elif kind == "dark":  # C1 decides the luminance term
        gt, pred = torch.zeros(H, W, C), 0.02 * torch.rand(H, W, C, generator=g)
    elif kind == "wide":  # the ABI does not restrict the range
        gt = -0.5 + 2.5 * torch.rand(H, W, C, generator=g)
        pred = (gt + 0.2 * torch.randn(H, W, C, generator=g)).clamp(-0.5, 2)
    else:
        raise KeyError(kind)
    return pred.contiguous(), gt.contiguous()


# ---- yardsticks ---------------------------------------------------------------------------------------------------------------
def _oracle_ops(a, b, window, C1, C2, padding="zeros", var_factor=1.0):
    """oracle/r2l_oracle.py ssim, op by op in the dtype of a, without the mean -> [H, W, C]."""
    import torch.nn.functional as F
    a, b = a.permute(2, 0, 1)[None], b.permute(2, 0, 1)[None]
    C = a.shape[1]
    w = window.to(a)[None, None].expand(C, 1, WIN, WIN).contiguous()
    if padding == "zeros":
        conv = lambda t: F.conv2d(t, w, padding=R, groups=C)
    else:
        conv = lambda t: F.conv2d(F.pad(t, (R, R, R, R), mode=padding), w, groups=C)
    mu1, mu2 = conv(a), conv(b)
    mu1_sq, mu2_sq, mu12 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1, s2, s12 = conv(a * a) - mu1_sq, conv(b * b) - mu2_sq, conv(a * b) - mu12
    if var_factor != 1.0:
        s1, s2, s12 = s1 * var_factor, s2 * var_factor, s12 * var_factor
    m = ((2 * mu12 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    return m[0].permute(1, 2, 0).contiguous()


def ssim_map64(a, b, window, mutant=None):
    """The yardstick.  mutant: None or a name of MAP_MUTANTS, a deliberately wrong evaluation that the bars must be able to see."""
    assert a.dtype == b.dtype == window.dtype == torch.float32
    a, b, w = a.double(), b.double(), window.double()
    C1, C2, kw = 0.01**2, 0.03**2, {}
    if mutant == "replicate_padding":
        kw["padding"] = "replicate"
    elif mutant == "window_transposed":
        w = w.t().contiguous()
    elif mutant == "tap_row_10_dropped":
        w = w.clone()
        w[WIN - 1] = 0
    elif mutant == "c1_c2_exchanged":
        C1, C2 = C2, C1
    elif mutant == "next_channel":
        a, b = a.roll(-1, 2), b.roll(-1, 2)  # channel c reads channel (c + 1) % C
    elif mutant == "sample_variance":
        kw["var_factor"] = 121.0 / 120.0
    elif mutant is not None:
        raise KeyError(mutant)
    return _oracle_ops(a, b, w, C1, C2, **kw)


def ssim_map32_ref(a, b, window):
    assert a.dtype == b.dtype == window.dtype == torch.float32
    return _oracle_ops(a, b, window, 0.01**2, 0.03**2)


def _fma(x, y, z):
    return (x.astype(np.float64) * y.astype(np.float64) + z.astype(np.float64)).astype(np.float32)


def ssim_map32_seq(a, b, window):
    """The kernel's sequence in numpy fp32 (module docstring) -> [H, W, C] fp32 tensor."""
    assert a.dtype == b.dtype == window.dtype == torch.float32
    H, W, C = a.shape
    pa, pb = np.zeros((H + 2 * R, W + 2 * R, C), np.float32), np.zeros((H + 2 * R, W + 2 * R, C), np.float32)
    pa[R:R + H, R:R + W], pb[R:R + H, R:R + W] = a.numpy(), b.numpy()
    win = window.numpy()
    m1, m2, s11, s22, s12 = (np.zeros((H, W, C), np.float32) for _ in range(5))
    for i in range(WIN):
        for j in range(WIN):
            w = np.full((1, 1, 1), win[i, j], np.float32)
            p, q = pa[i:i + H, j:j + W], pb[i:i + H, j:j + W]
            m1, m2 = _fma(w, p, m1), _fma(w, q, m2)
            s11, s22, s12 = _fma(w, p * p, s11), _fma(w, q * q, s22), _fma(w, p * q, s12)
    f = np.float32
    mu1_sq, mu2_sq, mu12 = m1 * m1, m2 * m2, m1 * m2
    sig1, sig2, sig12 = s11 - mu1_sq, s22 - mu2_sq, s12 - mu12
    C1, C2 = f(0.01) * f(0.01), f(0.03) * f(0.03)
    v = ((f(2) * mu12 + C1) * (f(2) * sig12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sig1 + sig2 + C2))
    assert v.dtype == np.float32
    return torch.from_numpy(v)


# ---- tile tables --------------------------------------------------------------------------------------------------------------
def tile_grid(H, W):
    return (H + T - 1) // T, (W + T - 1) // T  # tilesY, tilesX


def _padded(m):
    H, W, C = m.shape
    tY, tX = tile_grid(H, W)
    p = torch.zeros(tY * T, tX * T, C, dtype=m.dtype)
    p[:H, :W] = m
    return p.view(tY, T, tX, T, C)


def tiles64(m, mutant=None):
    """Per-tile, per-channel sums of a [H, W, C] map in fp64 -> flat [C * tilesY * tilesX], entry (c * tilesY + ty) * tilesX + tx.
    mutant: None or a name of TABLE_MUTANTS."""
    H, W, C = m.shape
    m = m.double()
    tY, tX = tile_grid(H, W)
    if mutant == "last_ragged_row_masked":  # the row mask of a ragged last tile one row too early
        if H % T:
            m = m.clone()
            m[H - 1] = 0
    elif mutant == "grid_origin_transposed":  # x and y exchanged between the grid and the tile origin:
        out = torch.zeros(C, tY, tX, dtype=torch.float64)  # entry (ty, tx) sums the tile at rows 16 tx, columns 16 ty
        for ty in range(tY):
            for tx in range(tX):
                out[:, ty, tx] = m[T * tx:T * tx + T, T * ty:T * ty + T].sum((0, 1))
        return out.reshape(-1)
    t = _padded(m).sum((1, 3)).permute(2, 0, 1)  # [C, tY, tX]
    if mutant == "grid_index_transposed":  # tilesX and tilesY exchanged in the partial index: (c * tilesX + tx) * tilesY + ty
        t = t.permute(0, 2, 1)
    elif mutant not in (None, "last_ragged_row_masked"):
        raise KeyError(mutant)
    return t.reshape(-1).contiguous()


def tile_pixels(H, W, C):
    return tiles64(torch.ones(H, W, C))


def tiles32_butterfly(m):
    """The kernel's own order on a fp32 map: thread = 16 ty + tx, four waves of 64, xor butterfly, (w0 + w1) + (w2 + w3)."""
    assert m.dtype == torch.float32
    tY, tX, C = tile_grid(*m.shape[:2]) + (m.shape[2],)
    x = _padded(m).permute(4, 0, 2, 1, 3).reshape(C * tY * tX, 4, 64).numpy().copy()  # [tile, wave, lane]
    for o in (32, 16, 8, 4, 2, 1):
        x = x[..., :o] + x[..., o:2 * o]
    x = x[..., 0]
    assert x.dtype == np.float32
    return torch.from_numpy((x[:, 0] + x[:, 1]) + (x[:, 2] + x[:, 3]))


def finish32(partial, count):
    """r2l_ssim_finish_kernel on a fp32 partial vector: stride loop of 256 per thread, the same tree, times 1.f / count."""
    p = partial.numpy().astype(np.float32)
    n = len(p)
    turns = (n + 255) // 256
    buf = np.zeros(turns * 256, np.float32)
    buf[:n] = p
    v = np.zeros(256, np.float32)
    for k in range(turns):
        v = v + buf[256 * k:256 * k + 256]  # (adding the padding's 0.f changes nothing)
    x = v.reshape(4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        x = x[..., :o] + x[..., o:2 * o]
    x = x[..., 0]
    return float(((x[0] + x[1]) + (x[2] + x[3])) * (np.float32(1) / np.float32(count)))


MAP_MUTANTS = ("replicate_padding", "window_transposed", "tap_row_10_dropped", "c1_c2_exchanged", "next_channel", "sample_variance")
TABLE_MUTANTS = ("grid_origin_transposed", "grid_index_transposed", "last_ragged_row_masked")
MUTANTS = MAP_MUTANTS + TABLE_MUTANTS + ("mean_over_hw",)

# ---- cases ----------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name shape kind pred gt window map64 t64 mean64 ref_tile ref_mean bar_tile bar_mean "
                                      "seq_t seq_bar")
_CACHE = {}


def build_case(name, shape, kind, window, seed):
    H, W, C = shape
    pred, gt = make_pair(shape, kind, seed)
    m64 = ssim_map64(pred, gt, window)
    t64, abs64 = tiles64(m64), tiles64(m64.abs())
    m32 = ssim_map32_ref(pred, gt, window)
    n = H * W * C
    mean64 = t64.sum().item() / n
    ref_tile = (tiles64(m32) - t64).abs().max().item()
    ref_mean = abs(m32.double().sum().item() / n - mean64)
    bar_tile = 4 * ref_tile + TILE_ADDS * U * abs64
    turns = (t64.numel() + 255) // 256
    bar_mean = 4 * ref_mean + (TILE_ADDS + FINISH_ADDS + turns - 1) * U * abs64.sum().item() / n + 2 * U * abs(mean64)
    seq_t = seq_bar = None
    if kind in SEQ_KINDS:
        seq = ssim_map32_seq(pred, gt, window)
        seq_t = tiles64(seq)
        seq_bar = TILE_ADDS * U * tiles64(seq.abs()) + 2 * U * tile_pixels(H, W, C)
    return Case(name, shape, kind, pred, gt, window, m64, t64, mean64, ref_tile, ref_mean, bar_tile, bar_mean, seq_t, seq_bar)


def case(name, window=None):
    """The table case `name`, computed once and left unchanged.  window: None = the case's own (the reference's, or the asymmetric
    one); "lib" = the window r2l_ssim builds for window_host = NULL."""
    key = (name, window)
    if key not in _CACHE:
        shape, kind, wname = _SPEC[name]
        w = window_lib() if window == "lib" else (window_asym() if wname == "asym" else window_ref())
        _CACHE[key] = build_case(name, shape, kind, w, 1000 + CASES.index(name))
    return _CACHE[key]


def worst_ratio(got, want, bar):
    """max over entries of |got - want| / bar (0 / 0 = 0) and its index."""
    d = (got.double() - want).abs()
    r = torch.where(d > 0, d / bar.clamp_min(1e-300), torch.zeros_like(d))
    k = int(r.argmax())
    return r[k].item(), k
