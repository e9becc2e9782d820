"""Device-resident ray store: the [o, d, rgb] rows of distillation live in HBM between the teacher's rendering and the
student's steps, instead of going through [4096,9] `.npy` shards (include/r2l_hip.h r2l_store_append / r2l_store_batch).

Sampler: draw t takes shard  perm(epoch_key(seed, t // n_shards), n_shards)[t % n_shards]  — a fresh permutation of the shards
per epoch, without replacement inside an epoch, a pure function of (seed, n_shards, t): shard_ids(), the draw_ids of
r2l_amd/keyed_perm.py (where perm and epoch_key, the keyed bijection of csrc/r2l_perm.h, are restated in numpy).  A store that
grows while it is trained from (driver --r2l_kd_every) is sampled with the shard count of the moment.

CompactRayStore (driver --r2l_compact_store) is the 16-bytes-a-ray form of a store the teacher fills: a row keeps rgb and the
ray's number in its flush group, o and d are recomputed per draw (r2l_cstore_append / r2l_cstore_batch); cstore_append_spec,
cstore_batch_spec and pixel_ray_spec restate it, and its batches are RayStore's bit for bit.

Store file (driver --r2l_store_save / --r2l_store_load): save() / load() of both classes go through r2l_amd/store_file.py,
whose names are importable from here too.
"""
import ctypes
import time

import numpy as np
import torch

from . import _lib
from ._lib import ptr as _p, stream as _stream
from .device_source import DeviceSource, DrawCounter
from .keyed_perm import M64, draw_ids, epoch_key, perm, perm_at  # noqa: F401  (tests and tools import them from here)
from .store_file import (STORE_SALT, STORE_SECTIONS, _load_store, _save_store, load_store, pack_store_header,  # noqa: F401
                         parse_store_header, read_store_header, store_layout, store_rank_path, words_digest_spec, words_digest_terms)


def shard_ids(seed, n_shards, draw0, n_draw):
    """Shard ids of the draws draw0 .. draw0 + n_draw - 1 (what r2l_store_batch copies and writes to ids_out): int64[n_draw]."""
    return draw_ids(seed, n_shards, draw0, n_draw)


def train_batch_spec(store, n_shards, rays_per_shard, draw0, n_draw, seed, pool=None, n_pool_rows=0, n_out=0, pool_key=0):
    """What r2l_train_batch writes, in numpy: (out_o, out_d, out_t, ids, idx).  store: the store's rows [>= n_shards *
    rays_per_shard, 9]; pool: [>= n_pool_rows, 9].  out_*: float32[n_draw * rays_per_shard + n_out, 3] — the rows of the shards
    shard_ids(seed, n_shards, draw0, n_draw), then the pool rows perm(pool_key, n_pool_rows)[:n_out]; ids int32[n_draw], idx
    int64[n_out]."""
    store = np.asarray(store, dtype=np.float32).reshape(-1, 9)
    rps = int(rays_per_shard)
    ids = shard_ids(seed, n_shards, draw0, n_draw)
    rows = [store[i * rps:(i + 1) * rps] for i in ids]
    idx = np.empty(0, dtype=np.int64)
    if n_out > 0:
        idx = perm_at(pool_key, n_pool_rows, np.arange(n_out, dtype=np.uint64))
        rows.append(np.asarray(pool, dtype=np.float32).reshape(-1, 9)[idx])
    rows = np.concatenate(rows, 0) if rows else np.empty((0, 9), dtype=np.float32)
    o, d, t = (np.ascontiguousarray(rows[:, c:c + 3]) for c in (0, 3, 6))
    return o, d, t, ids.astype(np.int32), idx


def pixel_ray_spec(c2w, focal, H, W, row, col):
    """pixel_ray of csrc/r2l_pixel_ray.h on n pixels, every operation separately rounded in np.float32: c2w [n, 3, 4], focal [n],
    row / col integer arrays [n] -> (o [n, 3], d [n, 3]).  The arithmetic include/r2l_hip.h pins under r2l_frame_rays."""
    f32 = np.float32
    c = np.asarray(c2w, dtype=f32).reshape(-1, 3, 4)
    f = np.asarray(focal, dtype=f32).reshape(-1)
    dx = (np.asarray(col).astype(f32) - f32(W) * f32(.5)) / f
    dy = -((np.asarray(row).astype(f32) - f32(H) * f32(.5)) / f)
    d = np.empty((c.shape[0], 3), dtype=f32)
    for i in range(3):
        d[:, i] = (dx * c[:, i, 0] + dy * c[:, i, 1]) + f32(-1.) * c[:, i, 2]
    return np.ascontiguousarray(c[:, :, 3]), d


def cstore_append_spec(rgb, rays_per_shard, key, shuffle=True):
    """What r2l_cstore_append writes into its new shards, in numpy: rgb [n_rows, 3] (n_rows = K*H*W of a flush group) ->
    (rgb_rows float32[m * rays_per_shard, 3], ids uint32[m * rays_per_shard]) with m = n_rows // rays_per_shard: row i holds
    rgb[perm(key, n_rows)[i]] and that index; the tail of the permuted sequence is dropped.  shuffle=False: the identity."""
    rgb = np.asarray(rgb, dtype=np.float32).reshape(-1, 3)
    n_rows = rgb.shape[0]
    if n_rows > 2**32 - 1:
        raise ValueError("cstore_append_spec: %d rows, a row's id is 32 bits" % n_rows)
    n_out = n_rows // int(rays_per_shard) * int(rays_per_shard)
    src = perm_at(key, n_rows, np.arange(n_out, dtype=np.uint64)) if shuffle else np.arange(n_out, dtype=np.int64)
    return np.ascontiguousarray(rgb[src]), src.astype(np.uint32)


def append_images_spec(images, c2ws, focals, rays_per_shard, key, shuffle=True):
    """What r2l_store_append_images writes into its new shards, in numpy: images [K, H, W, 3], c2ws [K, 3, 4], focals [K] or one
    number -> float32[m * rays_per_shard, 9] with m = K*H*W // rays_per_shard: row i is [o, d, rgb] of ray r = perm(key, K*H*W)[i],
    (o, d) = pixel_ray_spec of pose r // (H*W) at pixel ((r % (H*W)) // W, r % W), rgb = images.reshape(-1, 3)[r]; the tail of
    the permuted sequence is dropped.  shuffle=False: the identity."""
    images = np.asarray(images, dtype=np.float32)
    K, H, W = images.shape[:3]
    c2ws = np.asarray(c2ws, dtype=np.float32).reshape(K, 3, 4)
    focals = np.broadcast_to(np.asarray(focals, dtype=np.float32).reshape(-1), (K,))
    n_rows, hw = K * H * W, H * W
    n_out = n_rows // int(rays_per_shard) * int(rays_per_shard)
    src = perm_at(key, n_rows, np.arange(n_out, dtype=np.uint64)) if shuffle else np.arange(n_out, dtype=np.int64)
    k, pix = src // hw, src % hw
    o, d = pixel_ray_spec(c2ws[k], focals[k], H, W, pix // W, pix % W)
    return np.concatenate([o, d, images.reshape(-1, 3)[src]], 1)


def append_live_spec(rows, idx, rays_per_shard, key, shuffle=True):
    """What r2l_store_append_live writes into its new shards, in numpy: rows [n_rows, 9], idx int64[M] -> float32[m *
    rays_per_shard, 9] with m = M // rays_per_shard: row i is rows[idx[perm(key, M)[i]]] — a gather of the M rows followed by
    r2l_store_append's shuffle over M; an index outside [0, n_rows) gives a NaN row; the tail of the permuted sequence is dropped.
    shuffle=False: the identity."""
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 9)
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    M = idx.size
    n_out = M // int(rays_per_shard) * int(rays_per_shard)
    src = idx[perm_at(key, M, np.arange(n_out, dtype=np.uint64)) if shuffle else np.arange(n_out, dtype=np.int64)]
    ok = (src >= 0) & (src < rows.shape[0])
    out = np.full((n_out, 9), np.nan, dtype=np.float32)
    out[ok] = rows[src[ok]]
    return out


def cstore_batch_spec(rgb_rows, ids, pose_c2w, pose_focal, shard_pose0, H, W, n_shards, rays_per_shard, draw0, n_draw, seed):
    """What r2l_cstore_batch writes, in numpy: (batch float32[n_draw * rays_per_shard, 9], shard ids int32[n_draw]).  rgb_rows
    [>= n_shards * rays_per_shard, 3] and ids (uint32, same length) are the store's rows, pose_c2w [n_pose, 3, 4] / pose_focal
    [n_pose] its pose table, shard_pose0 [>= n_shards] the pose-table index of each shard's flush group.  Row = [o, d, rgb] with
    (o, d) = pixel_ray_spec of pose shard_pose0[shard] + id // (H*W) at pixel ((id % (H*W)) // W, id % W)."""
    rps, hw = int(rays_per_shard), int(H) * int(W)
    rgb_rows = np.asarray(rgb_rows, dtype=np.float32).reshape(-1, 3)
    ids = np.asarray(ids).astype(np.uint64).reshape(-1)
    sh = shard_ids(seed, n_shards, draw0, n_draw)
    at = (sh[:, None] * rps + np.arange(rps, dtype=np.int64)[None, :]).reshape(-1)
    rid = ids[at]
    p = np.repeat(np.asarray(shard_pose0, dtype=np.int64)[sh], rps) + (rid // np.uint64(hw)).astype(np.int64)
    pix = rid % np.uint64(hw)
    row, col = (pix // np.uint64(W)).astype(np.int64), (pix % np.uint64(W)).astype(np.int64)
    o, d = pixel_ray_spec(np.asarray(pose_c2w, dtype=np.float32).reshape(-1, 3, 4)[p],
                          np.asarray(pose_focal, dtype=np.float32).reshape(-1)[p], H, W, row, col)
    return np.concatenate([o, d, rgb_rows[at]], 1), sh.astype(np.int32)


class _Store(DrawCounter, DeviceSource):
    """What the two stores share: capacity_shards x rays_per_shard rows in device memory, n_shards of them filled, and next():
    the [o, d, rgb] rows of the next draws.  A class supplies its rows and how they are appended, _batch() (its launch),
    describe(), plan(), and what its store file is made from: KIND, ROW_WORDS, FILE_NAME, _sections(), _header_fields() and
    _from_header()."""

    def __init__(self, capacity_shards, device, rays_per_shard, seed, logger):
        if torch.device(device).type != "cuda":
            raise RuntimeError("%s lives in GPU memory: it needs a ROCm device (got %s)" % (type(self).__name__, torch.device(device)))
        self.capacity, self.rows_per_file, self.seed = int(capacity_shards), int(rays_per_shard), int(seed) & M64
        self.n_shards = 0
        self.files = []  # one name per filled shard (source file, or FILE_NAME % k for appended rows)
        self.n_files = None  # default of next()
        self.logger = logger

    def _new_slot(self, n):
        return (torch.empty(n * self.rows_per_file, 9, dtype=torch.float32, device=self.device),
                torch.empty(n, dtype=torch.int32, device=self.device))

    def _filled(self, what):
        if self.data is None:
            raise RuntimeError("%s is closed" % type(self).__name__)
        if self.n_shards < 1:
            raise RuntimeError("%s.%s: the store is empty" % (type(self).__name__, what))

    def _appended(self, m):
        self.files += [self.FILE_NAME % k for k in range(self.n_shards, self.n_shards + m)]
        self.n_shards += m
        return m

    def next(self, n_files=None):
        """[n_files * rays_per_shard, 9] device tensor [o, d, rgb] of the next n_files draws; valid until the second-next call."""
        n = int(self.n_files if n_files is None else n_files)
        self._filled("next")
        (buf, ids), (pbuf, pids) = self._take(n)
        self._batch(n, pbuf, pids, _stream(self.device))
        self.draw += n
        self.last_ids = ids
        return buf

    __next__ = next

    def __iter__(self):
        return self

    def save(self, path, provenance=None, rank=0, world=1, salt=None):
        """Write the filled sections (a plain store: its shards; a compact one: rows, the filled pose table and the shards' pose
        indices) and their device-computed digests to `path` (through path + ".tmp" and a rename); provenance: a dict for the log
        of whoever loads the file.  Returns {'path', 'bytes', 'seconds', 'GB/s', 'message'}."""
        return _save_store(self, path, provenance, rank, world, STORE_SALT if salt is None else salt)

    @classmethod
    def load(cls, path, device, seed=0, capacity_shards=None, logger=None):
        """A store holding what save() wrote (a compact one takes H, W and the pose count from the file): the header is checked
        before anything is allocated, the digests are recomputed on the device and compared before the store is handed out.
        Every refusal is a ValueError naming the path."""
        return _load_store(cls, path, device, seed, capacity_shards, logger)

    def close(self):
        self.data = None
        DeviceSource.close(self)


class RayStore(_Store):
    """capacity_shards x rays_per_shard rows [o, d, rgb] in device memory, filled by append() (device rows, e.g. the teacher's
    frames) or append_files() (existing shard files, read once) and drawn from by next(): one launch per batch, no host work.

    next(n_files) has RayShardLoader.next's contract — the returned [n_files * rays_per_shard, 9] tensor stays valid until the
    second-next call (two buffers) — and everything is ordered on the CURRENT stream: the copy into a buffer is enqueued behind
    whatever read it two calls ago on that stream, so there is no host sync and no side stream.  `rows_per_file`, `files`
    (one name per filled shard) and close() make it a drop-in for the driver's loader.

    save(path) writes the filled shards as one checksummed file, RayStore.load(path, device) is a store filled from it
    (r2l_amd/store_file.py): next / plan / seek / describe / close behave as after a fill."""

    KIND, ROW_WORDS, FILE_NAME = 0, 9, "store:%d"  # the file's kind, 32-bit words a row, the name of a shard in `files`

    def _sections(self):
        """(name, filled part) of what a store file holds besides the digests."""
        return [("rows", self.data[:self.n_shards * self.rows_per_file])]

    def _header_fields(self):
        return {"n_poses": 0, "H": 0, "W": 0}

    @classmethod
    def _from_header(cls, h, capacity, device, seed, logger):
        return cls(capacity, device, rays_per_shard=h["rays_per_shard"], seed=seed, logger=logger)

    def __init__(self, capacity_shards, device, rays_per_shard=4096, seed=0, logger=None):
        _Store.__init__(self, capacity_shards, device, rays_per_shard, seed, logger)
        if self.capacity < 1 or self.rows_per_file < 1 or self.rows_per_file % 4:
            raise ValueError("RayStore: capacity_shards >= 1 and rays_per_shard a positive multiple of 4 (got %d, %d)" %
                             (self.capacity, self.rows_per_file))
        self._open(device, self.capacity * self.rows_per_file * 36, "RayStore: %d shards of %d rays" % (self.capacity, self.rows_per_file))
        self.data = torch.empty(self.capacity * self.rows_per_file, 9, dtype=torch.float32, device=self.device)

    def append(self, rows, key, shuffle=True):
        """Append a device [n, 9] fp32 tensor as floor(n / rays_per_shard) shards, rows shuffled by perm(key, n) (the tail of
        the shuffled sequence is dropped, as create_data drops it).  Returns the number of shards written."""
        if rows.device != self.device or rows.dtype != torch.float32 or rows.dim() != 2 or rows.shape[1] != 9:
            raise ValueError("RayStore.append: need a [n, 9] fp32 tensor on %s" % self.device)
        rows = rows.contiguous()
        m = ctypes.c_int64()
        _lib.check(self._L.r2l_store_append(_p(rows), rows.shape[0], _p(self.data), self.capacity, self.n_shards,
                                            self.rows_per_file, int(key) & M64, int(bool(shuffle)), ctypes.byref(m),
                                            _stream(self.device)), "r2l_store_append")
        return self._appended(m.value)

    def append_live(self, rows, idx, M, key, shuffle=True):
        """Append the M rows rows[idx[:M]] (idx: a device int64 tensor, e.g. the live rays of OccupancyGrid.rays; M: its count, read
        by the caller) as floor(M / rays_per_shard) shards, shuffled by perm(key, M): what append(rows[idx[:M]], key) writes, bit for
        bit, in one launch and without the gathered rows (r2l_store_append_live).  Returns the number of shards written."""
        if rows.device != self.device or rows.dtype != torch.float32 or rows.dim() != 2 or rows.shape[1] != 9:
            raise ValueError("RayStore.append_live: need a [n, 9] fp32 tensor on %s" % self.device)
        M = int(M)
        if idx.device != self.device or idx.dtype != torch.int64 or idx.dim() != 1 or not 0 <= M <= idx.shape[0]:
            raise ValueError("RayStore.append_live: need an int64 index tensor on %s with at least M = %d entries" % (self.device, M))
        rows, idx = rows.contiguous(), idx.contiguous()
        m = ctypes.c_int64()
        _lib.check(self._L.r2l_store_append_live(_p(rows), rows.shape[0], _p(idx), M, _p(self.data), self.capacity, self.n_shards,
                                                 self.rows_per_file, int(key) & M64, int(bool(shuffle)), ctypes.byref(m),
                                                 _stream(self.device)), "r2l_store_append_live")
        return self._appended(m.value)

    def append_images(self, images, c2ws, focals, key, shuffle=True):
        """Append the real rays of K whole frames as ONE flush group (r2l_store_append_images): images [K, H, W, 3] fp32, c2ws
        [K, 3|4, 4], focals [K] fp32 tensor or one number for all K.  floor(K*H*W / rays_per_shard) shards of rows [o, d, rgb],
        o, d the pixels' rays in r2l_frame_rays' arithmetic, shuffled by perm(key, K*H*W) as append() shuffles.  Images on the
        store's device go through the kernel; images on the CPU go through append_images_spec and the rows are uploaded.  Returns
        the number of shards written."""
        if self.data is None:
            raise RuntimeError("RayStore is closed")
        c2ws = torch.as_tensor(c2ws, dtype=torch.float32)
        if c2ws.dim() != 3 or c2ws.shape[0] < 1 or c2ws.shape[1] not in (3, 4) or c2ws.shape[2] != 4:
            raise ValueError("RayStore.append_images: need c2ws [K, 3|4, 4], K >= 1")
        K = c2ws.shape[0]
        if (not torch.is_tensor(images) or images.dtype != torch.float32 or images.dim() != 4 or images.shape[0] != K
                or images.shape[3] != 3 or images.shape[1] < 1 or images.shape[2] < 1):
            raise ValueError("RayStore.append_images: need images [K, H, W, 3] = [%d, H, W, 3] fp32" % K)
        on_host = images.device.type == "cpu"
        if not on_host and images.device != self.device:
            raise ValueError("RayStore.append_images: images are on %s, the store on %s (CPU images go through the numpy "
                             "restatement)" % (images.device, self.device))
        H, W = int(images.shape[1]), int(images.shape[2])
        fdev, f = None, 0.
        if torch.is_tensor(focals):
            if focals.dtype != torch.float32 or tuple(focals.shape) != (K,):
                raise ValueError("RayStore.append_images: need focals [K] fp32, or one number")
            fdev = focals
        else:
            f = float(focals)
            if not f > 0.:
                raise ValueError("RayStore.append_images: need focal > 0 (got %r)" % (focals,))
        rps = self.rows_per_file
        m = K * H * W // rps
        if self.n_shards + m > self.capacity:
            raise ValueError("RayStore.append_images: %d shards of %d x %d x %d pixels do not fit behind %d shards in a store of %d" %
                             (m, K, H, W, self.n_shards, self.capacity))
        if on_host:
            rows = append_images_spec(images.numpy(), c2ws[:, :3, :4].cpu().numpy(), fdev.cpu().numpy() if fdev is not None else f,
                                      rps, int(key) & M64, shuffle)
            self.data[self.n_shards * rps:(self.n_shards + m) * rps].copy_(torch.from_numpy(rows))
            return self._appended(m)
        images = images.contiguous()
        c2ws = c2ws.to(self.device)[:, :3, :4].contiguous()
        if fdev is not None:
            fdev = fdev.to(self.device).contiguous()
        n = ctypes.c_int64()
        _lib.check(self._L.r2l_store_append_images(_p(images), _p(c2ws), _p(fdev), f, K, H, W, _p(self.data), self.capacity,
                                                   self.n_shards, rps, int(key) & M64, int(bool(shuffle)), ctypes.byref(n),
                                                   _stream(self.device)), "r2l_store_append_images")
        return self._appended(n.value)

    def append_files(self, files, threads=4):
        """Read every listed [rays_per_shard, 9] .npy shard ONCE, in list order, through two pinned group buffers into the
        store (no shuffle: the files are shuffled already).  Host threads fill one group while the other one is copied."""
        from concurrent.futures import ThreadPoolExecutor
        files = list(files)
        if self.n_shards + len(files) > self.capacity:
            raise ValueError("RayStore.append_files: %d files do not fit behind %d shards in a store of %d" %
                             (len(files), self.n_shards, self.capacity))
        threads = max(1, int(threads))
        group = max(1, min(len(files), 4 * threads))
        rps = self.rows_per_file
        pinned = [torch.empty(group, rps, 9, dtype=torch.float32).pin_memory() for _ in range(2)]
        views = [p.numpy() for p in pinned]
        done = [None, None]
        want = (rps, 9)

        def read(path, dst):
            with open(path, "rb") as f:
                major, _minor = np.lib.format.read_magic(f)
                shape, fortran, dtype = (np.lib.format.read_array_header_1_0 if major == 1 else np.lib.format.read_array_header_2_0)(f)
                if tuple(shape) != want or fortran or dtype != np.dtype("<f4"):
                    raise ValueError("%s: need a C-order float32 %s array, got %s %s" % (path, want, dtype, tuple(shape)))
                buf = memoryview(dst).cast("B")
                got = f.readinto(buf)
                if got != len(buf):
                    raise ValueError("%s: short read (%d of %d bytes)" % (path, got, len(buf)))

        t0 = time.perf_counter()
        view = self.data.view(self.capacity, rps, 9)
        with ThreadPoolExecutor(max_workers=threads) as ex:
            for g, a in enumerate(range(0, len(files), group)):
                part, k = files[a:a + group], g & 1
                if done[k] is not None:
                    done[k].synchronize()  # the copy that last read this pinned buffer
                list(ex.map(read, part, [views[k][i] for i in range(len(part))]))
                view[self.n_shards:self.n_shards + len(part)].copy_(pinned[k][:len(part)], non_blocking=True)
                done[k] = torch.cuda.Event()
                done[k].record()
                self.n_shards += len(part)
        for ev in done:
            if ev is not None:
                ev.synchronize()
        self.files += files
        dt = time.perf_counter() - t0
        gb = len(files) * rps * 36 / 1e9
        msg = "ray store: read %d files, %.3f GB in %.2fs = %.2f GB/s (%d threads)" % (len(files), gb, dt, gb / max(dt, 1e-9), threads)
        if self.logger is not None:
            self.logger.info(msg)
        return {"files": len(files), "GB": gb, "GB/s": gb / max(dt, 1e-9), "message": msg}

    def _batch(self, n, pbuf, pids, st):
        _lib.check(self._L.r2l_store_batch(_p(self.data), self.n_shards, self.rows_per_file, self.draw, n, self.seed, pbuf, pids, st),
                   "r2l_store_batch")

    def plan(self, n_files=None):
        """What a caller that draws the next batch itself (r2l_train_batch, r2l_student_train_step) needs: the store's base
        pointer, the shards filled at this moment, rays per shard, the sampler's seed, and the draws next() would take.
        advance() afterwards moves the counter as next() does."""
        self._filled("plan")
        return {"ptr": _p(self.data), "n_shards": self.n_shards, "rays_per_shard": self.rows_per_file, "seed": self.seed,
                "draw0": self.draw, "n_draw": int(self.n_files if n_files is None else n_files)}

    def advance(self, n_files=None):
        self.draw += int(self.n_files if n_files is None else n_files)

    def shards(self):
        """The filled part of the store as a [n_shards, rays_per_shard, 9] view."""
        return self.data[:self.n_shards * self.rows_per_file].view(self.n_shards, self.rows_per_file, 9)

    def describe(self):
        return "%d / %d shards of %d rays, %.3f GB of %.3f GB allocated in device memory" % (
            self.n_shards, self.capacity, self.rows_per_file, self.n_shards * self.rows_per_file * 36 / 1e9, self.nbytes / 1e9)


class CompactRayStore(_Store):
    """A ray store the TEACHER fills, at 16 bytes a ray instead of 36 (include/r2l_hip.h r2l_cstore_append / r2l_cstore_batch): a
    row keeps { rgb, id } — id = the ray's number inside its flush group — and next() recomputes o, d from the group's pose table
    with the arithmetic r2l_frame_rays computed them with, so the batches equal the plain store's bit for bit.  capacity_shards x
    rays_per_shard rows, capacity_poses pose-table slots (13 floats each) and one int per shard, for frames of one size H x W.

    RayStore's surface: append_frames() instead of append(), then next / seek / files / n_files / rows_per_file / describe /
    close with the same contracts (two buffers, everything ordered on the CURRENT stream).  There is no append_files — rows from
    files carry arbitrary rays — and plan() refuses: the fused iteration reads the 36-byte layout."""

    ROW_BYTES, POSE_BYTES, SHARD_BYTES = 16, 52, 4
    KIND, ROW_WORDS, FILE_NAME = 1, 4, "cstore:%d"  # the file's kind, 32-bit words a row, the name of a shard in `files`

    def _sections(self):
        """(name, filled part) of what a store file holds besides the digests, in the file's order."""
        return [("rows", self.data[:self.n_shards * self.rows_per_file]), ("pose_c2w", self.pose_c2w[:self.n_poses]),
                ("pose_focal", self.pose_focal[:self.n_poses]), ("shard_pose0", self.shard_pose0[:self.n_shards])]

    def _header_fields(self):
        return {"n_poses": self.n_poses, "H": self.H, "W": self.W}

    @classmethod
    def _from_header(cls, h, capacity, device, seed, logger):
        store = cls(capacity, h["n_poses"], h["H"], h["W"], device, rays_per_shard=h["rays_per_shard"], seed=seed, logger=logger)
        store.n_poses = h["n_poses"]
        return store

    @staticmethod
    def bytes_needed(capacity_shards, capacity_poses, rays_per_shard=4096):
        """16 B per ray + 52 B per pose + 4 B per shard."""
        return (int(capacity_shards) * int(rays_per_shard) * CompactRayStore.ROW_BYTES + int(capacity_poses) * CompactRayStore.POSE_BYTES
                + int(capacity_shards) * CompactRayStore.SHARD_BYTES)

    def __init__(self, capacity_shards, capacity_poses, H, W, device, rays_per_shard=4096, seed=0, logger=None):
        _Store.__init__(self, capacity_shards, device, rays_per_shard, seed, logger)
        self.capacity_poses, self.H, self.W = int(capacity_poses), int(H), int(W)
        if self.capacity < 1 or self.capacity_poses < 1 or self.rows_per_file < 1 or self.rows_per_file % 4:
            raise ValueError("CompactRayStore: capacity_shards >= 1, capacity_poses >= 1 and rays_per_shard a positive multiple of 4 "
                             "(got %d, %d, %d)" % (self.capacity, self.capacity_poses, self.rows_per_file))
        if self.H < 1 or self.W < 1 or self.H * self.W > 2**32 - 1:
            raise ValueError("CompactRayStore: need H >= 1, W >= 1 and H * W <= 2^32 - 1 (got %d x %d)" % (self.H, self.W))
        self._open(device, self.bytes_needed(self.capacity, self.capacity_poses, self.rows_per_file),
                   "CompactRayStore: %d shards of %d rays and %d poses" % (self.capacity, self.rows_per_file, self.capacity_poses))
        self.data = torch.empty(self.capacity * self.rows_per_file, 4, dtype=torch.float32, device=self.device)  # { rgb, id }
        self.pose_c2w = torch.empty(self.capacity_poses, 3, 4, dtype=torch.float32, device=self.device)
        self.pose_focal = torch.empty(self.capacity_poses, dtype=torch.float32, device=self.device)
        self.shard_pose0 = torch.empty(self.capacity, dtype=torch.int32, device=self.device)
        self.desc = _lib.CompactStoreDesc(rows=self.data.data_ptr(), pose_c2w=self.pose_c2w.data_ptr(),
                                          pose_focal=self.pose_focal.data_ptr(), shard_pose0=self.shard_pose0.data_ptr(),
                                          capacity_shards=self.capacity, capacity_poses=self.capacity_poses,
                                          rays_per_shard=self.rows_per_file, H=self.H, W=self.W)
        self.n_poses = 0

    def append_frames(self, rgb, c2ws, focals, key, shuffle=True):
        """Append one flush group of K whole frames: rgb [K*H*W, 3] fp32 on the device (rows may be strided: the [:, 6:9] of
        [o, d, rgb] rows), c2ws [K, 3, 4], focals [K] device tensor or one number for all K.  floor(K*H*W / rays_per_shard)
        shards, rows shuffled by perm(key, K*H*W) as RayStore.append shuffles them.  Returns the number of shards written."""
        if self.data is None:
            raise RuntimeError("CompactRayStore is closed")
        c2ws = torch.as_tensor(c2ws, dtype=torch.float32)  # (as render_frames takes its poses: [K, 3|4, 4], converted to fp32)
        if c2ws.dim() != 3 or c2ws.shape[0] < 1 or c2ws.shape[1] not in (3, 4) or c2ws.shape[2] != 4:
            raise ValueError("CompactRayStore.append_frames: need c2ws [K, 3|4, 4], K >= 1")
        K = c2ws.shape[0]
        c2ws = c2ws.to(self.device)[:, :3, :4].contiguous()
        if (rgb.device != self.device or rgb.dtype != torch.float32 or rgb.dim() != 2 or tuple(rgb.shape) != (K * self.H * self.W, 3)):
            raise ValueError("CompactRayStore.append_frames: need rgb [K*H*W, 3] = [%d, 3] fp32 on %s" % (K * self.H * self.W, self.device))
        if rgb.stride(1) != 1 or rgb.stride(0) < 3:
            rgb = rgb.contiguous()
        fdev, f = None, 0.
        if torch.is_tensor(focals):
            if focals.device != self.device or focals.dtype != torch.float32 or tuple(focals.shape) != (K,):
                raise ValueError("CompactRayStore.append_frames: need focals [K] fp32 on %s, or one number" % self.device)
            fdev = focals.contiguous()
        else:
            f = float(focals)
        m = ctypes.c_int64()
        _lib.check(self._L.r2l_cstore_append(ctypes.byref(self.desc), _p(rgb), rgb.stride(0), _p(c2ws), _p(fdev), f, K,
                                             self.n_shards, self.n_poses, int(key) & M64, int(bool(shuffle)), ctypes.byref(m),
                                             _stream(self.device)), "r2l_cstore_append")
        self.n_poses += K
        return self._appended(m.value)

    def _batch(self, n, pbuf, pids, st):
        _lib.check(self._L.r2l_cstore_batch(ctypes.byref(self.desc), self.n_shards, self.draw, n, self.seed, pbuf, pids, st),
                   "r2l_cstore_batch")

    def plan(self, n_files=None):
        raise NotImplementedError("CompactRayStore.plan: r2l_train_batch / r2l_student_train_step read the 36-byte rows of a RayStore; "
                                  "a compact store hands out batches through next() only")

    def describe(self):
        return "compact, %d / %d shards of %d rays and %d / %d poses, %.3f GB of %.3f GB allocated in device memory " \
               "(16 B/ray + 52 B/pose + 4 B/shard)" % (
                   self.n_shards, self.capacity, self.rows_per_file, self.n_poses, self.capacity_poses,
                   self.bytes_needed(self.n_shards, self.n_poses, self.rows_per_file) / 1e9, self.nbytes / 1e9)

    def close(self):
        self.pose_c2w = self.pose_focal = self.shard_pose0 = self.desc = None
        _Store.close(self)
