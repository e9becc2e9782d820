"""Device-resident ray store: the [o, d, rgb] rows of distillation live in HBM between the teacher's rendering and the
student's steps, instead of going through [4096,9] `.npy` shards (include/r2l_hip.h r2l_store_append / r2l_store_batch).

perm() and shard_ids() restate in numpy what the device computes — the keyed bijection of csrc/r2l_perm.h (the one the hard-ray
pool's row choice uses) and the sampler built on it; they are the specification the tests hold the kernels to.

Sampler: draw t takes shard  perm(epoch_key(seed, t // n_shards), n_shards)[t % n_shards]  — a fresh permutation of the shards
per epoch, without replacement inside an epoch (the InfiniteSampler of main.py:759-767), a pure function of (seed, n_shards, t).
A store that grows while it is trained from (driver --r2l_kd_every) is sampled with the shard count of the moment.

CompactRayStore (driver --r2l_compact_store) is the 16-bytes-a-ray form of a store the teacher fills: a row keeps rgb and the
ray's number in its flush group, o and d are recomputed per draw (r2l_cstore_append / r2l_cstore_batch); cstore_append_spec,
cstore_batch_spec and pixel_ray_spec restate it, and its batches are RayStore's bit for bit.

Store file (driver --r2l_store_save / --r2l_store_load; the last section of this module): a filled store of either kind as one
checksummed file per rank — save() / load() of both classes, load_store, read_store_header — with a digest per shard computed
on the device (r2l_words_digest); words_digest_spec restates the digest.
"""
import ctypes
import time

import numpy as np

M64 = (1 << 64) - 1


def _mix(x):
    """murmur3 finalizer on uint32 arrays (wrapping arithmetic)."""
    x = x.astype(np.uint32, copy=True)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x85ebca6b)
    x ^= x >> np.uint32(13)
    x *= np.uint32(0xc2b2ae35)
    x ^= x >> np.uint32(16)
    return x


def _mix1(x):
    return int(_mix(np.array([x & 0xffffffff], dtype=np.uint32))[0])


def round_keys(key):
    key = int(key) & M64
    lo, hi = key & 0xffffffff, key >> 32
    return [_mix1(lo), _mix1(hi ^ 0x9e3779b9), _mix1(lo ^ 0x7f4a7c15), _mix1((hi + 0x6a09e667) & 0xffffffff)]


def half_bits(n):
    bits = 2
    while (1 << bits) < n:
        bits += 2
    return bits // 2


def _feistel(x, hb, k):
    mask = np.uint32((1 << hb) - 1)
    l = (x >> np.uint64(hb)).astype(np.uint32) & mask
    r = x.astype(np.uint32) & mask
    for i in range(4):
        f = _mix(r ^ np.uint32(k[i])) & mask
        l, r = r, l ^ f
    return (l.astype(np.uint64) << np.uint64(hb)) | r.astype(np.uint64)


def perm_at(key, n, idx):
    """pi(key, n) evaluated at the indices idx (each < n): int64 array."""
    hb, k = half_bits(n), round_keys(key)
    x = _feistel(np.asarray(idx, dtype=np.uint64), hb, k)
    while True:
        out = np.nonzero(x >= np.uint64(n))[0]
        if out.size == 0:
            return x.astype(np.int64)
        x[out] = _feistel(x[out], hb, k)  # cycle walking


def perm(key, n):
    """The bijection of [0, n) that r2l_pool_pick(n, n, key) writes and r2l_store_append shuffles by: int64[n]."""
    return perm_at(key, n, np.arange(n, dtype=np.uint64))


def epoch_key(seed, epoch):
    """splitmix64 finalizer of seed + (epoch + 1) * 0x9E3779B97F4A7C15 (mod 2^64)."""
    z = (int(seed) + (int(epoch) + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def shard_ids(seed, n_shards, draw0, n_draw):
    """Shard ids of the draws draw0 .. draw0 + n_draw - 1 (what r2l_store_batch copies and writes to ids_out): int64[n_draw]."""
    out = np.empty(n_draw, dtype=np.int64)
    t, j = int(draw0), 0
    while j < n_draw:
        e, r = divmod(t, n_shards)
        n = min(n_shards - r, n_draw - j)
        out[j:j + n] = perm_at(epoch_key(seed, e), n_shards, np.arange(r, r + n, dtype=np.uint64))
        t, j = t + n, j + n
    return out


def words_digest_terms(words, words_per_item, n_items, salt=0):
    """The summands of r2l_words_digest: uint64[n_items, words_per_item], entry [k, i] = epoch_key((i << 32) | word[k, i], salt + k)."""
    n, wpi = int(n_items), int(words_per_item)
    w = np.ascontiguousarray(words).reshape(-1).view(np.uint32)
    if wpi < 1 or wpi >= 2**32 or n < 0 or w.size != n * wpi:
        raise ValueError("words_digest_spec: need 1 <= words_per_item < 2^32 and n_items * words_per_item = %d words (got %d x %d)"
                         % (w.size, n, wpi))
    x = w.reshape(n, wpi).astype(np.uint64) | (np.arange(wpi, dtype=np.uint64) << np.uint64(32))[None, :]
    c = np.array([((int(salt) + k + 1) * 0x9E3779B97F4A7C15) & M64 for k in range(n)], dtype=np.uint64)
    z = x + c[:, None]  # (uint64 arrays wrap: arithmetic mod 2^64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def words_digest_spec(words, words_per_item, n_items, salt=0):
    """What r2l_words_digest writes, in numpy: uint64[n_items], out[k] = the sum mod 2^64 of words_digest_terms(...)[k] — an integer
    sum, so the order of the accumulation plays no part.  words: n_items * words_per_item 32-bit words (any 4-byte dtype)."""
    return words_digest_terms(words, words_per_item, n_items, salt).sum(axis=1, dtype=np.uint64)


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


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class RayStore:
    """capacity_shards x rays_per_shard rows [o, d, rgb] in device memory, filled by append() (device rows, e.g. the teacher's
    frames) or append_files() (existing shard files, read once) and drawn from by next(): one launch per batch, no host work.

    next(n_files) has RayShardLoader.next's contract — the returned [n_files * rays_per_shard, 9] tensor stays valid until the
    second-next call (two buffers) — and everything is ordered on the CURRENT stream: the copy into a buffer is enqueued behind
    whatever read it two calls ago on that stream, so there is no host sync and no side stream.  `rows_per_file`, `files`
    (one name per filled shard) and close() make it a drop-in for the driver's loader.

    save(path) writes the filled shards as one checksummed file, RayStore.load(path, device) is a store filled from it (the
    "store file" section at the end of this module): next / plan / seek / describe / close behave as after a fill."""

    KIND, ROW_WORDS, FILE_NAME = 0, 9, "store:%d"  # the file's kind, 32-bit words a row, the name of a shard in `files`

    def _sections(self):
        """(name, filled part) of what a store file holds besides the digests."""
        return [("rows", self.data[:self.n_shards * self.rows_per_file])]

    def save(self, path, provenance=None, rank=0, world=1, salt=None):
        """Write the filled shards and their device-computed digests to `path` (through path + ".tmp" and a rename); provenance:
        a dict for the log of whoever loads the file.  Returns {'path', 'bytes', 'seconds', 'GB/s', 'message'}."""
        return _save_store(self, path, provenance, rank, world, STORE_SALT if salt is None else salt)

    @classmethod
    def load(cls, path, device, seed=0, capacity_shards=None, logger=None):
        """A store holding what save() wrote: the header is checked before anything is allocated, the digests are recomputed
        on the device and compared before the store is handed out.  Every refusal is a ValueError naming the path."""
        return _load_store(cls, path, device, seed, capacity_shards, logger)

    def __init__(self, capacity_shards, device, rays_per_shard=4096, seed=0, logger=None):
        import torch
        from . import _lib
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("RayStore lives in GPU memory: it needs a ROCm device (got %s)" % self.device)
        if self.device.index is None:  # "cuda" -> the current device, so that tensors' devices compare equal to it
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.capacity, self.rows_per_file, self.seed = int(capacity_shards), int(rays_per_shard), int(seed) & M64
        if self.capacity < 1 or self.rows_per_file < 1 or self.rows_per_file % 4:
            raise ValueError("RayStore: capacity_shards >= 1 and rays_per_shard a positive multiple of 4 (got %d, %d)" %
                             (self.capacity, self.rows_per_file))
        need = self.capacity * self.rows_per_file * 36
        free, _total = torch.cuda.mem_get_info(self.device)
        if need > 0.8 * free:
            raise MemoryError("RayStore: %d shards of %d rays need %.2f GB, more than 80 %% of the %.2f GB free on %s" %
                              (self.capacity, self.rows_per_file, need / 1e9, free / 1e9, self.device))
        self._lib, self._L = _lib, _lib.load()
        self.data = torch.empty(self.capacity * self.rows_per_file, 9, dtype=torch.float32, device=self.device)
        self.nbytes = need
        self.n_shards = 0
        self.files = []  # one name per filled shard (source file, or "store:<k>" for appended rows)
        self.n_files = None  # default of next()
        self.draw = 0
        self.last_ids = None
        self._buf, self._ids, self._k = [None, None], [None, None], 0
        self.logger = logger

    def _stream(self):
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def append(self, rows, key, shuffle=True):
        """Append a device [n, 9] fp32 tensor as floor(n / rays_per_shard) shards, rows shuffled by perm(key, n) (the tail of
        the shuffled sequence is dropped, as create_data drops it).  Returns the number of shards written."""
        import torch
        if rows.device != self.device or rows.dtype != torch.float32 or rows.dim() != 2 or rows.shape[1] != 9:
            raise ValueError("RayStore.append: need a [n, 9] fp32 tensor on %s" % self.device)
        rows = rows.contiguous()
        m = ctypes.c_int64()
        self._lib.check(self._L.r2l_store_append(_p(rows), rows.shape[0], _p(self.data), self.capacity, self.n_shards,
                                                 self.rows_per_file, int(key) & M64, int(bool(shuffle)), ctypes.byref(m),
                                                 self._stream()), "r2l_store_append")
        self.files += ["store:%d" % k for k in range(self.n_shards, self.n_shards + m.value)]
        self.n_shards += m.value
        return m.value

    def append_files(self, files, threads=4):
        """Read every listed [rays_per_shard, 9] .npy shard ONCE, in list order, through two pinned group buffers into the
        store (no shuffle: the files are shuffled already).  Host threads fill one group while the other one is copied."""
        import torch
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

    def next(self, n_files=None):
        """[n_files * rays_per_shard, 9] device tensor of the next n_files draws; valid until the second-next call."""
        import torch
        n = int(self.n_files if n_files is None else n_files)
        if self.data is None:
            raise RuntimeError("RayStore is closed")
        if self.n_shards < 1:
            raise RuntimeError("RayStore.next: the store is empty")
        k = self._k
        if self._buf[k] is None or self._buf[k].shape[0] != n * self.rows_per_file:
            # (a new tensor: the one handed out two calls ago stays the caller's; the allocator is stream-ordered)
            self._buf[k] = torch.empty(n * self.rows_per_file, 9, dtype=torch.float32, device=self.device)
            self._ids[k] = torch.empty(n, dtype=torch.int32, device=self.device)
        self._lib.check(self._L.r2l_store_batch(_p(self.data), self.n_shards, self.rows_per_file, self.draw, n, self.seed,
                                                _p(self._buf[k]), _p(self._ids[k]), self._stream()), "r2l_store_batch")
        self.draw += n
        self.last_ids = self._ids[k]
        self._k ^= 1
        return self._buf[k]

    __next__ = next

    def plan(self, n_files=None):
        """What a caller that draws the next batch itself (r2l_train_batch, r2l_student_train_step) needs: the store's base
        pointer, the shards filled at this moment, rays per shard, the sampler's seed, and the draws next() would take.
        advance() afterwards moves the counter as next() does."""
        if self.data is None:
            raise RuntimeError("RayStore is closed")
        if self.n_shards < 1:
            raise RuntimeError("RayStore.plan: the store is empty")
        return {"ptr": _p(self.data), "n_shards": self.n_shards, "rays_per_shard": self.rows_per_file, "seed": self.seed,
                "draw0": self.draw, "n_draw": int(self.n_files if n_files is None else n_files)}

    def advance(self, n_files=None):
        self.draw += int(self.n_files if n_files is None else n_files)

    def __iter__(self):
        return self

    def seek(self, draw):
        if draw < 0:
            raise ValueError("RayStore.seek: negative draw")
        self.draw = int(draw)

    def shards(self):
        """The filled part of the store as a [n_shards, rays_per_shard, 9] view."""
        return self.data[:self.n_shards * self.rows_per_file].view(self.n_shards, self.rows_per_file, 9)

    def describe(self):
        return "%d / %d shards of %d rays, %.3f GB of %.3f GB allocated in device memory" % (
            self.n_shards, self.capacity, self.rows_per_file, self.n_shards * self.rows_per_file * 36 / 1e9, self.nbytes / 1e9)

    def close(self):
        self.data = None
        self._buf, self._ids, self.last_ids = [None, None], [None, None], None


class CompactRayStore:
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

    def save(self, path, provenance=None, rank=0, world=1, salt=None):
        """RayStore.save for the compact layout: rows, the filled pose table and the shards' pose indices, each digested."""
        return _save_store(self, path, provenance, rank, world, STORE_SALT if salt is None else salt)

    @classmethod
    def load(cls, path, device, seed=0, capacity_shards=None, logger=None):
        """RayStore.load for the compact layout; H, W and the pose count come from the file."""
        return _load_store(cls, path, device, seed, capacity_shards, logger)

    @staticmethod
    def bytes_needed(capacity_shards, capacity_poses, rays_per_shard=4096):
        """16 B per ray + 52 B per pose + 4 B per shard."""
        return (int(capacity_shards) * int(rays_per_shard) * CompactRayStore.ROW_BYTES + int(capacity_poses) * CompactRayStore.POSE_BYTES
                + int(capacity_shards) * CompactRayStore.SHARD_BYTES)

    def __init__(self, capacity_shards, capacity_poses, H, W, device, rays_per_shard=4096, seed=0, logger=None):
        import torch
        from . import _lib
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("CompactRayStore lives in GPU memory: it needs a ROCm device (got %s)" % self.device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.capacity, self.capacity_poses = int(capacity_shards), int(capacity_poses)
        self.H, self.W = int(H), int(W)
        self.rows_per_file, self.seed = int(rays_per_shard), int(seed) & M64
        if self.capacity < 1 or self.capacity_poses < 1 or self.rows_per_file < 1 or self.rows_per_file % 4:
            raise ValueError("CompactRayStore: capacity_shards >= 1, capacity_poses >= 1 and rays_per_shard a positive multiple of 4 "
                             "(got %d, %d, %d)" % (self.capacity, self.capacity_poses, self.rows_per_file))
        if self.H < 1 or self.W < 1 or self.H * self.W > 2**32 - 1:
            raise ValueError("CompactRayStore: need H >= 1, W >= 1 and H * W <= 2^32 - 1 (got %d x %d)" % (self.H, self.W))
        need = self.bytes_needed(self.capacity, self.capacity_poses, self.rows_per_file)
        free, _total = torch.cuda.mem_get_info(self.device)
        if need > 0.8 * free:
            raise MemoryError("CompactRayStore: %d shards of %d rays and %d poses need %.2f GB, more than 80 %% of the %.2f GB free on %s"
                              % (self.capacity, self.rows_per_file, self.capacity_poses, need / 1e9, free / 1e9, self.device))
        self._lib, self._L = _lib, _lib.load()
        self.data = torch.empty(self.capacity * self.rows_per_file, 4, dtype=torch.float32, device=self.device)  # { rgb, id }
        self.pose_c2w = torch.empty(self.capacity_poses, 3, 4, dtype=torch.float32, device=self.device)
        self.pose_focal = torch.empty(self.capacity_poses, dtype=torch.float32, device=self.device)
        self.shard_pose0 = torch.empty(self.capacity, dtype=torch.int32, device=self.device)
        self.desc = _lib.CompactStoreDesc(rows=self.data.data_ptr(), pose_c2w=self.pose_c2w.data_ptr(),
                                          pose_focal=self.pose_focal.data_ptr(), shard_pose0=self.shard_pose0.data_ptr(),
                                          capacity_shards=self.capacity, capacity_poses=self.capacity_poses,
                                          rays_per_shard=self.rows_per_file, H=self.H, W=self.W)
        self.nbytes = need
        self.n_shards = 0
        self.n_poses = 0
        self.files = []  # one name per filled shard ("cstore:<k>")
        self.n_files = None  # default of next()
        self.draw = 0
        self.last_ids = None
        self._buf, self._ids, self._k = [None, None], [None, None], 0
        self.logger = logger

    def _stream(self):
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def append_frames(self, rgb, c2ws, focals, key, shuffle=True):
        """Append one flush group of K whole frames: rgb [K*H*W, 3] fp32 on the device (rows may be strided: the [:, 6:9] of
        [o, d, rgb] rows), c2ws [K, 3, 4], focals [K] device tensor or one number for all K.  floor(K*H*W / rays_per_shard)
        shards, rows shuffled by perm(key, K*H*W) as RayStore.append shuffles them.  Returns the number of shards written."""
        import torch
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
        self._lib.check(self._L.r2l_cstore_append(ctypes.byref(self.desc), _p(rgb), rgb.stride(0), _p(c2ws), _p(fdev), f, K,
                                                  self.n_shards, self.n_poses, int(key) & M64, int(bool(shuffle)), ctypes.byref(m),
                                                  self._stream()), "r2l_cstore_append")
        self.files += ["cstore:%d" % k for k in range(self.n_shards, self.n_shards + m.value)]
        self.n_shards += m.value
        self.n_poses += K
        return m.value

    def next(self, n_files=None):
        """[n_files * rays_per_shard, 9] device tensor [o, d, rgb] of the next n_files draws; valid until the second-next call."""
        import torch
        n = int(self.n_files if n_files is None else n_files)
        if self.data is None:
            raise RuntimeError("CompactRayStore is closed")
        if self.n_shards < 1:
            raise RuntimeError("CompactRayStore.next: the store is empty")
        k = self._k
        if self._buf[k] is None or self._buf[k].shape[0] != n * self.rows_per_file:
            # (a new tensor: the one handed out two calls ago stays the caller's; the allocator is stream-ordered)
            self._buf[k] = torch.empty(n * self.rows_per_file, 9, dtype=torch.float32, device=self.device)
            self._ids[k] = torch.empty(n, dtype=torch.int32, device=self.device)
        self._lib.check(self._L.r2l_cstore_batch(ctypes.byref(self.desc), self.n_shards, self.draw, n, self.seed, _p(self._buf[k]),
                                                 _p(self._ids[k]), self._stream()), "r2l_cstore_batch")
        self.draw += n
        self.last_ids = self._ids[k]
        self._k ^= 1
        return self._buf[k]

    __next__ = next

    def __iter__(self):
        return self

    def plan(self, n_files=None):
        raise NotImplementedError("CompactRayStore.plan: r2l_train_batch / r2l_student_train_step read the 36-byte rows of a RayStore; "
                                  "a compact store hands out batches through next() only")

    def seek(self, draw):
        if draw < 0:
            raise ValueError("CompactRayStore.seek: negative draw")
        self.draw = int(draw)

    def describe(self):
        return "compact, %d / %d shards of %d rays and %d / %d poses, %.3f GB of %.3f GB allocated in device memory " \
               "(16 B/ray + 52 B/pose + 4 B/shard)" % (
                   self.n_shards, self.capacity, self.rows_per_file, self.n_poses, self.capacity_poses,
                   self.bytes_needed(self.n_shards, self.n_poses, self.rows_per_file) / 1e9, self.nbytes / 1e9)

    def close(self):
        self.data = self.pose_c2w = self.pose_focal = self.shard_pose0 = self.desc = None
        self._buf, self._ids, self.last_ids = [None, None], [None, None], None


# ---- store file: a filled store as it sits in device memory, one checksummed file per rank (INTEGRATION.md "store file") ----
# Little-endian.  A 4096-byte header, then sections that each start on a 4096-byte boundary: rows (the filled shards), for a
# compact store pose_c2w / pose_focal / shard_pose0 (the filled parts), and digests: uint64[n_shards] of r2l_words_digest over the
# rows with one item per shard and salt `salt`, then — compact — one digest per pose-table section, each section a single item
# with salt `salt + n_shards + j` (j = 0, 1, 2 in the order above): entry x of the digest section was computed with salt + x.
# The provenance (a JSON object inside the header) is for the log: nothing is derived from it, and it carries no time stamp.
STORE_MAGIC, STORE_VERSION, STORE_ALIGN = b"R2LSTORE", 1, 4096
STORE_SALT = 0x52324C53544F5245  # default salt of the digests ("R2LSTORE" as a number)
STORE_SECTIONS = ("rows", "pose_c2w", "pose_focal", "shard_pose0", "digests")
STORE_CHUNK = 64 << 20  # bytes per pinned staging buffer; two of them
_HEAD = "<8sIIQQQIIIIQ10QI"  # magic, version, kind, rays_per_shard, n_shards, n_poses, H, W, rank, world, salt, 5 x (offset, length), len(json)
_HEAD_BYTES, _PROV_AT = 148, 256  # bytes [148, 256) and whatever follows the provenance up to 4096 are reserved: zero
_ROW_BYTES = {0: 36, 1: 16}


def store_rank_path(path, rank=0, world=1):
    """File of a rank: `path` at world size 1, `path.rank<r>of<w>` otherwise (--r2l_store_save / --r2l_store_load)."""
    return path if world == 1 else "%s.rank%dof%d" % (path, rank, world)


def _align(n):
    return (int(n) + STORE_ALIGN - 1) // STORE_ALIGN * STORE_ALIGN


def store_layout(kind, rays_per_shard, n_shards, n_poses):
    """{section: (offset, length)} of a store file: the sections in STORE_SECTIONS order, each on a 4096-byte boundary; a plain
    store's pose-table sections are (0, 0)."""
    n, rps, npose = int(n_shards), int(rays_per_shard), int(n_poses)
    lengths = {"rows": n * rps * _ROW_BYTES[kind], "pose_c2w": npose * 48 if kind else 0, "pose_focal": npose * 4 if kind else 0,
               "shard_pose0": n * 4 if kind else 0, "digests": (n + (3 if kind else 0)) * 8}
    out, at = {}, STORE_ALIGN
    for name in STORE_SECTIONS:
        out[name] = (at, lengths[name]) if lengths[name] else (0, 0)
        at = _align(at + lengths[name])
    return out


def pack_store_header(kind, rays_per_shard, n_shards, n_poses=0, H=0, W=0, rank=0, world=1, salt=STORE_SALT, provenance=None,
                      sections=None):
    """The 4096 header bytes.  sections: {name: (offset, length)}, by default store_layout's."""
    import json
    import struct
    sections = store_layout(kind, rays_per_shard, n_shards, n_poses) if sections is None else sections
    prov = json.dumps(provenance or {}, sort_keys=True).encode("utf-8")
    if len(prov) > STORE_ALIGN - _PROV_AT:
        raise ValueError("store file: the provenance is %d bytes of JSON, the header has room for %d" % (len(prov), STORE_ALIGN - _PROV_AT))
    flat = [v for name in STORE_SECTIONS for v in sections[name]]
    head = struct.pack(_HEAD, STORE_MAGIC, STORE_VERSION, int(kind), int(rays_per_shard), int(n_shards), int(n_poses), int(H), int(W),
                       int(rank), int(world), int(salt) & M64, *flat, len(prov))
    assert len(head) == _HEAD_BYTES
    return head + bytes(_PROV_AT - _HEAD_BYTES) + prov + bytes(STORE_ALIGN - _PROV_AT - len(prov))


def parse_store_header(raw, path="<bytes>", file_size=None):
    """Header bytes -> dict (kind, rays_per_shard, n_shards, n_poses, H, W, rank, world, salt, sections, provenance, path).  Every
    refusal is a ValueError that names the path and the fact; file_size (when given) is what the sections must fit into."""
    import json
    import struct

    def bad(what):
        return ValueError("%s: not a usable ray-store file: %s" % (path, what))

    if len(raw) < STORE_ALIGN:
        raise bad("truncated: %d bytes, the header alone is %d" % (len(raw), STORE_ALIGN))
    f = struct.unpack(_HEAD, raw[:_HEAD_BYTES])
    if f[0] != STORE_MAGIC:
        raise bad("wrong magic %r (want %r)" % (f[0], STORE_MAGIC))
    if f[1] != STORE_VERSION:
        raise bad("version %d, this build reads version %d" % (f[1], STORE_VERSION))
    kind = f[2]
    if kind not in _ROW_BYTES:
        raise bad("unknown kind %d (0 = 36-byte rows, 1 = compact)" % kind)
    plen = f[-1]
    if plen > STORE_ALIGN - _PROV_AT:
        raise bad("provenance length %d exceeds the header" % plen)
    if any(raw[_HEAD_BYTES:_PROV_AT]) or any(raw[_PROV_AT + plen:STORE_ALIGN]):
        raise bad("non-zero reserved bytes in the header")
    h = dict(zip(("rays_per_shard", "n_shards", "n_poses", "H", "W", "rank", "world", "salt"), f[3:11]), kind=kind, path=path)
    if h["rays_per_shard"] < 1 or h["rays_per_shard"] % 4 or h["n_shards"] < 1 or h["n_shards"] >= 2**31 or h["n_poses"] >= 2**31:
        raise bad("rays_per_shard %d / n_shards %d / n_poses %d out of range" % (h["rays_per_shard"], h["n_shards"], h["n_poses"]))
    if kind == 1 and (h["n_poses"] < 1 or h["H"] < 1 or h["W"] < 1):
        raise bad("a compact store needs n_poses, H, W >= 1 (got %d, %d, %d)" % (h["n_poses"], h["H"], h["W"]))
    if h["world"] < 1 or h["rank"] >= h["world"]:
        raise bad("rank %d of world %d" % (h["rank"], h["world"]))
    h["sections"] = {name: (f[11 + 2 * i], f[12 + 2 * i]) for i, name in enumerate(STORE_SECTIONS)}
    want = store_layout(kind, h["rays_per_shard"], h["n_shards"], h["n_poses"])
    for name in STORE_SECTIONS:
        off, length = h["sections"][name]
        if length != want[name][1] or off % STORE_ALIGN or (length and off < STORE_ALIGN) or (not length and off):
            raise bad("section %s at %d, %d bytes: want %d bytes on a %d-byte boundary" % (name, off, length, want[name][1], STORE_ALIGN))
    try:
        h["provenance"] = json.loads(raw[_PROV_AT:_PROV_AT + plen].decode("utf-8")) if plen else {}
    except ValueError as e:
        raise bad("the provenance is not UTF-8 JSON (%s)" % e)
    if file_size is not None:
        for name in STORE_SECTIONS:
            off, length = h["sections"][name]
            if off + length > file_size:
                raise bad("truncated: section %s reaches byte %d, the file has %d" % (name, off + length, file_size))
    return h


def read_store_header(path):
    """Header of a store file as a dict (parse_store_header), checked against the file's size.  Touches no GPU."""
    import os
    with open(path, "rb") as f:
        raw = f.read(STORE_ALIGN)
        size = os.fstat(f.fileno()).st_size
    return parse_store_header(raw, path, size)


def _as_bytes(t):
    import torch
    return t.reshape(-1).view(torch.uint8)


def _pinned_pair(largest):
    import torch
    n = max(1, min(STORE_CHUNK, int(largest)))  # (no more than the largest section: small stores pin little)
    return [torch.empty(n, dtype=torch.uint8).pin_memory() for _ in range(2)]


def _pieces(sections, layout, chunk):
    """(device byte tensor, file offset) of every chunk of every section, in file order."""
    out = []
    for name, t in sections:
        b, off = _as_bytes(t), layout[name][0]
        assert b.numel() == layout[name][1], name
        out += [(b[a:a + chunk], off + a) for a in range(0, b.numel(), chunk)]
    return out


def _store_digests(store, salt):
    """Digests of a store's filled sections on the device (current stream): int64 tensor holding the uint64 [n_shards (+ 3)]."""
    import torch
    secs = store._sections()
    n = store.n_shards
    dig = torch.empty(n + len(secs) - 1, dtype=torch.int64, device=store.device)
    st, L = store._stream(), store._L
    store._lib.check(L.r2l_words_digest(_p(secs[0][1]), store.rows_per_file * store.ROW_WORDS, n, int(salt) & M64, _p(dig), st),
                     "r2l_words_digest")
    for j, (name, t) in enumerate(secs[1:]):
        if t.numel() >= 2**32:
            raise ValueError("store file: section %s has %d words, one digest covers fewer than 2^32" % (name, t.numel()))
        store._lib.check(L.r2l_words_digest(_p(t), t.numel(), 1, (int(salt) + n + j) & M64,
                                            ctypes.c_void_p(dig.data_ptr() + 8 * (n + j)), st), "r2l_words_digest")
    return dig


def _save_store(store, path, provenance=None, rank=0, world=1, salt=STORE_SALT):
    import os
    import torch
    if store.data is None:
        raise RuntimeError("%s is closed" % type(store).__name__)
    if store.n_shards < 1:
        raise ValueError("%s.save: the store is empty" % type(store).__name__)
    t0 = time.perf_counter()
    kind, n_poses = store.KIND, getattr(store, "n_poses", 0)
    layout = store_layout(kind, store.rows_per_file, store.n_shards, n_poses)
    head = pack_store_header(kind, store.rows_per_file, store.n_shards, n_poses, getattr(store, "H", 0), getattr(store, "W", 0), rank,
                             world, salt, provenance, layout)
    with torch.cuda.device(store.device):
        dig = _store_digests(store, salt)
        secs = store._sections() + [("digests", dig)]
        pieces = _pieces(secs, layout, STORE_CHUNK)
        pinned = _pinned_pair(max(p[0].numel() for p in pieces))
        views = [p.numpy() for p in pinned]
        tmp = path + ".tmp"
        fd = os.open(tmp, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        try:
            _pwrite(fd, head, 0)
            done = [None, None]

            def write(i):  # chunk i has landed in its pinned buffer: to the file
                done[i & 1].synchronize()
                _pwrite(fd, memoryview(views[i & 1])[:pieces[i][0].numel()], pieces[i][1])

            for i, (src, _off) in enumerate(pieces):  # the copy of chunk i runs while chunk i - 1 is written
                pinned[i & 1][:src.numel()].copy_(src, non_blocking=True)
                done[i & 1] = torch.cuda.Event()
                done[i & 1].record()
                if i:
                    write(i - 1)
            write(len(pieces) - 1)
            os.fsync(fd)
        finally:
            os.close(fd)
    os.replace(tmp, path)  # a killed run leaves no half file under the final name
    dt = time.perf_counter() - t0
    nbytes = max(off + length for off, length in layout.values())
    msg = "ray store: saved %d shards to %s, %.3f GB in %.2fs = %.2f GB/s (digests on the device, salt %#x)" % (
        store.n_shards, path, nbytes / 1e9, dt, nbytes / 1e9 / max(dt, 1e-9), salt)
    if store.logger is not None:
        store.logger.info(msg)
    return {"path": path, "bytes": nbytes, "seconds": dt, "GB/s": nbytes / 1e9 / max(dt, 1e-9), "message": msg}


def _pwrite(fd, buf, offset):
    import os
    buf = memoryview(buf).cast("B")
    while len(buf):
        n = os.pwrite(fd, buf, offset)
        buf, offset = buf[n:], offset + n


def _pread(fd, buf, offset, path):
    import os
    buf = memoryview(buf).cast("B")
    while len(buf):
        n = os.preadv(fd, [buf], offset)
        if n <= 0:
            raise ValueError("%s: not a usable ray-store file: truncated: short read at byte %d" % (path, offset))
        buf, offset = buf[n:], offset + n


def _load_store(cls, path, device, seed=0, capacity_shards=None, logger=None):
    import os
    import torch
    t0 = time.perf_counter()
    h = read_store_header(path)  # (every refusal of the header comes before any device allocation)
    if h["kind"] != cls.KIND:
        raise ValueError("%s: kind %d (%s), %s.load reads kind %d; load_store picks the class from the file" % (
            path, h["kind"], "compact" if h["kind"] else "36-byte rows", cls.__name__, cls.KIND))
    n = h["n_shards"]
    cap = n if capacity_shards is None else int(capacity_shards)
    if cap < n:
        raise ValueError("%s: the file holds %d shards, capacity_shards is %d" % (path, n, cap))
    if cls.KIND:
        store = cls(cap, h["n_poses"], h["H"], h["W"], device, rays_per_shard=h["rays_per_shard"], seed=seed, logger=logger)
        store.n_poses = h["n_poses"]
    else:
        store = cls(cap, device, rays_per_shard=h["rays_per_shard"], seed=seed, logger=logger)
    store.n_shards = n
    store.files = [cls.FILE_NAME % k for k in range(n)]
    try:
        with torch.cuda.device(store.device):
            secs = store._sections()
            pieces = _pieces(secs, h["sections"], STORE_CHUNK)
            pinned = _pinned_pair(max(p[0].numel() for p in pieces))
            views = [p.numpy() for p in pinned]
            want = np.empty(n + len(secs) - 1, dtype="<u8")
            fd = os.open(path, os.O_RDONLY)
            try:
                _pread(fd, want, h["sections"]["digests"][0], path)
                done = [None, None]
                for i, (dst, off) in enumerate(pieces):  # chunk i is read while the copy of chunk i - 1 runs
                    if done[i & 1] is not None:
                        done[i & 1].synchronize()  # the copy that last read this pinned buffer
                    _pread(fd, memoryview(views[i & 1])[:dst.numel()], off, path)
                    dst.copy_(pinned[i & 1][:dst.numel()], non_blocking=True)
                    done[i & 1] = torch.cuda.Event()
                    done[i & 1].record()
            finally:
                os.close(fd)
            got = _store_digests(store, h["salt"]).cpu().numpy().view(np.uint64)  # (synchronises: the copies are behind it)
        bad = np.nonzero(got != want.astype(np.uint64))[0]
        if bad.size:
            x = int(bad[0])
            where = "shard %d" % x if x < n else "section %s" % secs[1 + x - n][0]
            raise ValueError("%s: digest mismatch in %s (file %#018x, device %#018x): the file is corrupt and is not loaded" % (
                path, where, int(want[x]), int(got[x])))
    except Exception:
        store.close()
        raise
    dt = time.perf_counter() - t0
    nbytes = max(off + length for off, length in h["sections"].values())
    msg = "ray store: loaded %d shards from %s, %.3f GB in %.2fs = %.2f GB/s, %d digests verified" % (
        n, path, nbytes / 1e9, dt, nbytes / 1e9 / max(dt, 1e-9), got.size)
    if logger is not None:
        logger.info(msg)
    store.load_info = {"path": path, "bytes": nbytes, "seconds": dt, "GB/s": nbytes / 1e9 / max(dt, 1e-9), "message": msg, "header": h}
    return store


def load_store(path, device, seed=0, capacity_shards=None, logger=None):
    """The store a file holds, of the class its `kind` names: RayStore (0) or CompactRayStore (1)."""
    cls = CompactRayStore if read_store_header(path)["kind"] else RayStore
    return cls.load(path, device, seed=seed, capacity_shards=capacity_shards, logger=logger)
