"""Store file (driver --r2l_store_save / --r2l_store_load; INTEGRATION.md "store file"): a filled ray store of either kind
(r2l_amd/raystore.py) as it sits in device memory, one checksummed file per rank — what save() / load() of both store classes go
through, load_store, read_store_header — with a digest per shard computed on the device (r2l_words_digest); words_digest_spec
restates the digest in numpy.

Little-endian.  A 4096-byte header, then sections that each start on a 4096-byte boundary: rows (the filled shards), for a
compact store pose_c2w / pose_focal / shard_pose0 (the filled parts), and digests: uint64[n_shards] of r2l_words_digest over the
rows with one item per shard and salt `salt`, then — compact — one digest per pose-table section, each section a single item
with salt `salt + n_shards + j` (j = 0, 1, 2 in the order above): entry x of the digest section was computed with salt + x.
The provenance (a JSON object inside the header) is for the log: nothing is derived from it, and it carries no time stamp.

A store class says what its file is made from: KIND, ROW_WORDS, FILE_NAME, _sections(), _header_fields() and _from_header().
"""
import ctypes
import json
import os
import struct
import time

import numpy as np
import torch

from . import _lib
from .keyed_perm import M64

STORE_MAGIC, STORE_VERSION, STORE_ALIGN = b"R2LSTORE", 1, 4096
STORE_SALT = 0x52324C53544F5245  # default salt of the digests ("R2LSTORE" as a number)
STORE_SECTIONS = ("rows", "pose_c2w", "pose_focal", "shard_pose0", "digests")
STORE_CHUNK = 64 << 20  # bytes per pinned staging buffer; two of them
_HEAD = "<8sIIQQQIIIIQ10QI"  # magic, version, kind, rays_per_shard, n_shards, n_poses, H, W, rank, world, salt, 5 x (offset, length), len(json)
_HEAD_BYTES, _PROV_AT = 148, 256  # bytes [148, 256) and whatever follows the provenance up to 4096 are reserved: zero
_ROW_BYTES = {0: 36, 1: 16}


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
    with open(path, "rb") as f:
        raw = f.read(STORE_ALIGN)
        size = os.fstat(f.fileno()).st_size
    return parse_store_header(raw, path, size)


def _as_bytes(t):
    return t.reshape(-1).view(torch.uint8)


def _pinned_pair(largest):
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
    secs = store._sections()
    n = store.n_shards
    dig = torch.empty(n + len(secs) - 1, dtype=torch.int64, device=store.device)
    st, L = _lib.stream(store.device), store._L
    _lib.check(L.r2l_words_digest(_lib.ptr(secs[0][1]), store.rows_per_file * store.ROW_WORDS, n, int(salt) & M64, _lib.ptr(dig), st),
               "r2l_words_digest")
    for j, (name, t) in enumerate(secs[1:]):
        if t.numel() >= 2**32:
            raise ValueError("store file: section %s has %d words, one digest covers fewer than 2^32" % (name, t.numel()))
        _lib.check(L.r2l_words_digest(_lib.ptr(t), t.numel(), 1, (int(salt) + n + j) & M64,
                                      ctypes.c_void_p(dig.data_ptr() + 8 * (n + j)), st), "r2l_words_digest")
    return dig


def _save_store(store, path, provenance=None, rank=0, world=1, salt=STORE_SALT):
    if store.data is None:
        raise RuntimeError("%s is closed" % type(store).__name__)
    if store.n_shards < 1:
        raise ValueError("%s.save: the store is empty" % type(store).__name__)
    t0 = time.perf_counter()
    fields = store._header_fields()
    layout = store_layout(store.KIND, store.rows_per_file, store.n_shards, fields["n_poses"])
    head = pack_store_header(store.KIND, store.rows_per_file, store.n_shards, rank=rank, world=world, salt=salt, provenance=provenance,
                             sections=layout, **fields)
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
    buf = memoryview(buf).cast("B")
    while len(buf):
        n = os.pwrite(fd, buf, offset)
        buf, offset = buf[n:], offset + n


def _pread(fd, buf, offset, path):
    buf = memoryview(buf).cast("B")
    while len(buf):
        n = os.preadv(fd, [buf], offset)
        if n <= 0:
            raise ValueError("%s: not a usable ray-store file: truncated: short read at byte %d" % (path, offset))
        buf, offset = buf[n:], offset + n


def _load_store(cls, path, device, seed=0, capacity_shards=None, logger=None):
    t0 = time.perf_counter()
    h = read_store_header(path)  # (every refusal of the header comes before any device allocation)
    if h["kind"] != cls.KIND:
        raise ValueError("%s: kind %d (%s), %s.load reads kind %d; load_store picks the class from the file" % (
            path, h["kind"], "compact" if h["kind"] else "36-byte rows", cls.__name__, cls.KIND))
    n = h["n_shards"]
    cap = n if capacity_shards is None else int(capacity_shards)
    if cap < n:
        raise ValueError("%s: the file holds %d shards, capacity_shards is %d" % (path, n, cap))
    store = cls._from_header(h, cap, device, seed, logger)
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
    from .raystore import CompactRayStore, RayStore
    cls = CompactRayStore if read_store_header(path)["kind"] else RayStore
    return cls.load(path, device, seed=seed, capacity_shards=capacity_shards, logger=logger)
