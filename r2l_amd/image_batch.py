"""Pixel sampler of teacher training in images mode (include/r2l_hip.h r2l_image_batch / r2l_image_draw; --r2l_image_sampler).

The reference's no_batching mode (main.py:1260-1302) draws one training image per iteration, centre-crops it for precrop_iters
and takes N_rand of its pixels without replacement — get_rays of the whole frame, a meshgrid of its coordinates and a
permutation of all of them, on the host, to pick N_rand pixels.  Here iteration i takes

    z = epoch_key(seed ^ 0x696D675F6D6F6465, i),   img = ((z >> 40) * n_img) >> 24,   key = epoch_key(z, 0)

and draw j takes position  q = perm(key, win_h*win_w)[j]  of the window (row0, col0, win_h, win_w), row-major: the keyed
bijection of csrc/r2l_perm.h again, so the N_rand pixels are distinct, and the ray of each is computed when it is drawn
(the per-pixel body of r2l_pixel_batch).  The choices are ours, not numpy's; the distribution is the reference's: a uniform
image, a uniform sample without replacement within the window.  A pure function of (seed, i): there is no sampler state and
nothing to seek on a resume.

window_ids() and host_batch() restate in numpy / torch what the kernel computes; they are the specification the tests hold it to,
and the CPU path of the training loop.
"""
import numpy as np

from . import _lib
from .keyed_perm import M64, epoch_key, perm_at
from .pixel_batch import PixelSource, _check, host_rows

DRAW_SALT = 0x696D675F6D6F6465  # "img_mode"


def image_draw(seed, i, n_img):
    """(img, key) of iteration i >= 1 (what r2l_image_draw writes): the image among n_img, and the key of its window's bijection."""
    i, n_img = int(i), int(n_img)
    if i < 1 or n_img < 1:
        raise ValueError("image_draw: need iteration >= 1 and n_img >= 1, got %d and %d" % (i, n_img))
    z = epoch_key((int(seed) & M64) ^ DRAW_SALT, i)
    return ((z >> 40) * n_img) >> 24, epoch_key(z, 0)


def crop_window(H, W, frac):
    """(row0, col0, win_h, win_w) of the centre crop of train_nerf.precrop_coords (main.py:1273-1284): rows H//2 - dH .. H//2 + dH - 1
    with dH = int(H//2 * frac), columns likewise."""
    dH, dW = int(H // 2 * frac), int(W // 2 * frac)
    return H // 2 - dH, W // 2 - dW, 2 * dH, 2 * dW


def full_window(H, W):
    return 0, 0, int(H), int(W)


def _check_window(H, W, window, n_draw):
    row0, col0, win_h, win_w = (int(x) for x in window)
    if win_h < 1 or win_w < 1 or row0 < 0 or col0 < 0 or row0 + win_h > H or col0 + win_w > W:
        raise ValueError("image batch: window (row0 %d, col0 %d, %d x %d) is empty or leaves the %d x %d frame" %
                         (row0, col0, win_h, win_w, H, W))
    if not 0 <= n_draw <= win_h * win_w:
        raise ValueError("image batch: %d draws from a window of %d x %d pixels" % (n_draw, win_h, win_w))
    return row0, col0, win_h, win_w


def window_ids(H, W, img, window, key, n_draw):
    """Pixel ids of the draws 0 .. n_draw - 1 (what r2l_image_batch writes to ids_out): int64[n_draw], (img*H + row)*W + col."""
    n_draw = int(n_draw)
    row0, col0, win_h, win_w = _check_window(H, W, window, n_draw)
    q = perm_at(int(key) & M64, win_h * win_w, np.arange(n_draw, dtype=np.uint64))
    return (int(img) * H + row0 + q // win_w) * W + col0 + q % win_w


def host_batch(images, poses, H, W, focal, ndc, img, window, key, n_draw):
    """(rays_o, rays_d, viewdirs, target, ids) of the draws 0 .. n_draw - 1 on CPU tensors: pixel_batch.host_rows at window_ids."""
    images, poses, H, W, focal = _check(images, poses, H, W, focal)
    if not 0 <= int(img) < images.shape[0]:
        raise ValueError("image batch: image %d of %d" % (img, images.shape[0]))
    return host_rows(images, poses, H, W, focal, ndc, window_ids(H, W, img, window, key, n_draw))


class ImageBatcher(PixelSource):
    """The training images and poses, and next(i, n, window): the (rays_o, rays_d, viewdirs, target) of iteration i, each [n, 3] —
    n distinct pixels of the window (row0, col0, win_h, win_w; None = the whole frame) of image image_draw(seed, i, n_img).

    On a ROCm device the images [n_img,H,W,3] (fp32, after Scene.rgb_images) and poses are uploaded once and a batch is one
    r2l_image_batch launch on the CURRENT stream into one of two alternating sets of output buffers: the tensors handed out stay
    valid until the second-next call, and nothing synchronises (PixelBatcher's contract).  On the CPU next() answers from
    host_rows at window_ids.  next() is a pure function of (seed, i): there is no draw counter.  last_ids holds the pixel ids of
    the last batch (int64), last_img its image."""

    last_img = None

    def describe(self):
        return "%d images %d x %d, %.3f GB on %s" % (self.n_img, self.H, self.W, self.nbytes / 1e9, self.device)

    def _draw(self, i, n, window=None):
        n = int(n)
        window = _check_window(self.H, self.W, full_window(self.H, self.W) if window is None else window, n)
        return n, image_draw(self.seed, i, self.n_img) + (window,)

    def _ids(self, n, which):
        img, key, window = which
        return window_ids(self.H, self.W, img, window, key, n)

    def _launch(self, n, which, out, st):
        img, key, window = which
        _lib.check(self._L.r2l_image_batch(*self._frames, img, *window, key, n, *out, st), "r2l_image_batch")

    def _drawn(self, n, which):
        self.last_img = which[0]
