"""Store file (r2l_amd/raystore.py save / load / read_store_header, include/r2l_hip.h r2l_words_digest, --r2l_store_save /
--r2l_store_load), the parts that need no GPU: the digest's numpy restatement, the argument checks of the entry point through the
loaded library, the header's pack / parse round trip and every refusal of a hand-written file, and the refusals of the two flags."""
import ctypes
import os

import numpy as np
import pytest

from tests.test_driver_cpu import ROOT

INVALID = 1  # hipErrorInvalidValue
M64 = (1 << 64) - 1


def test_digest_spec_properties():
    from r2l_amd import raystore as R
    rng = np.random.RandomState(3)
    wpi, n, salt = 37, 5, 0xFEDCBA9876543210
    words = rng.randint(0, 2**32, size=n * wpi, dtype=np.uint64).astype(np.uint32)
    want = R.words_digest_spec(words, wpi, n, salt)
    assert want.dtype == np.uint64 and want.shape == (n,) and len(set(want.tolist())) == n
    # the definition, word by word in python integers
    for k in (0, n - 1):
        assert int(want[k]) == sum(R.epoch_key((i << 32) | int(words[k * wpi + i]), salt + k) for i in range(wpi)) & M64
    # any order of the accumulation gives the same bits
    terms = R.words_digest_terms(words, wpi, n, salt)
    for trial in range(3):
        order = rng.permutation(wpi)
        for k in range(n):
            acc = 0
            for i in order:
                acc = (acc + int(terms[k, i])) & M64
            assert acc == int(want[k])
    assert np.array_equal(terms[:, ::-1].sum(axis=1, dtype=np.uint64), want)
    # one flipped bit of one word
    for at, bit in ((0, 0), (wpi + 5, 31), (n * wpi - 1, 13)):
        w = words.copy()
        w[at] ^= np.uint32(1 << bit)
        got = R.words_digest_spec(w, wpi, n, salt)
        assert got[at // wpi] != want[at // wpi] and np.array_equal(np.delete(got, at // wpi), np.delete(want, at // wpi))
    # two different words of an item swap places
    w = words.copy()
    assert w[2 * wpi + 1] != w[2 * wpi + 30]
    w[[2 * wpi + 1, 2 * wpi + 30]] = w[[2 * wpi + 30, 2 * wpi + 1]]
    got = R.words_digest_spec(w, wpi, n, salt)
    assert got[2] != want[2] and np.array_equal(np.delete(got, 2), np.delete(want, 2))
    # two different items swap places
    w = words.reshape(n, wpi).copy()
    w[[1, 3]] = w[[3, 1]]
    got = R.words_digest_spec(w, wpi, n, salt)
    assert got[1] != want[1] and got[3] != want[3] and got[1] != want[3] and got[3] != want[1]
    assert np.array_equal(got[[0, 2, 4]], want[[0, 2, 4]])
    # the salt: item k under salt s is item 0 under salt s + k
    assert R.words_digest_spec(words[wpi:2 * wpi], wpi, 1, salt + 1)[0] == want[1]
    assert R.words_digest_spec(words, wpi, n, 0)[0] != want[0]
    # any 4-byte dtype is taken as its bits
    f = rng.rand(8).astype(np.float32)
    assert np.array_equal(R.words_digest_spec(f, 4, 2), R.words_digest_spec(f.view(np.uint32), 4, 2))
    with pytest.raises(ValueError):
        R.words_digest_spec(words, 0, n)
    with pytest.raises(ValueError):
        R.words_digest_spec(words, wpi, n + 1)


def test_abi_argument_checks():
    """Every refusal is hipErrorInvalidValue with the argument's name in r2l_last_error, before anything is launched (NULL and
    dummy pointers: this runs without a GPU)."""
    from r2l_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(64)  # any non-NULL, 16-byte aligned value: the checks fail before it is ever dereferenced

    def digest(words=one, wpi=4, n=1, out=one):
        return lib.r2l_words_digest(words, wpi, n, 7, out, None)

    for kw, word in ((dict(words=None), b"NULL"),
                     (dict(out=None), b"NULL"),
                     (dict(wpi=0), b"words_per_item"),
                     (dict(wpi=-4), b"words_per_item"),
                     (dict(wpi=2**32), b"words_per_item"),
                     (dict(n=-1), b"n_items"),
                     (dict(words=ctypes.c_void_p(66)), b"words must be 4-byte aligned"),
                     (dict(words=ctypes.c_void_p(65)), b"words must be 4-byte aligned"),
                     (dict(out=ctypes.c_void_p(68)), b"out must be 8-byte aligned")):
        assert digest(**kw) == INVALID, kw
        msg = lib.r2l_last_error()
        assert b"r2l_words_digest" in msg and word in msg, (kw, msg)
    # no items: nothing is enqueued, whatever the pointers are; this succeeds without a GPU
    assert digest(n=0) == 0 and digest(words=None, out=None, n=0) == 0
    assert "r2l_words_digest" in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), "r2l_words_digest")
    assert "r2l_words_digest" in open(os.path.join(ROOT, "include", "r2l_hip.h")).read()


def _file(tmp_path, name, header, size=None):
    """A file of `size` bytes (default: what the header's sections need) that starts with `header`."""
    from r2l_amd import raystore as R
    path = str(tmp_path / name)
    if size is None:
        size = max(o + n for o, n in R.parse_store_header(header)["sections"].values())
    with open(path, "wb") as f:
        f.write(header)
        f.truncate(size)
    return path


def test_header_round_trip(tmp_path):
    from r2l_amd import raystore as R
    prov = {"teacher_ckpt": "logs/téacher.tar", "N_samples": 64, "perturb": 1.0, "white_bkgd": True, "R2L_SEED": "0"}
    raw = R.pack_store_header(1, 4096, 390600, 10000, 400, 400, rank=3, world=8, salt=2**64 - 5, provenance=prov)
    assert len(raw) == 4096 and raw[:8] == b"R2LSTORE"
    h = R.parse_store_header(raw)
    assert (h["kind"], h["rays_per_shard"], h["n_shards"], h["n_poses"], h["H"], h["W"], h["rank"], h["world"], h["salt"]) == \
        (1, 4096, 390600, 10000, 400, 400, 3, 8, 2**64 - 5)
    assert h["provenance"] == prov
    s = h["sections"]
    assert list(s) == list(R.STORE_SECTIONS) and s == R.store_layout(1, 4096, 390600, 10000)
    assert s["rows"] == (4096, 390600 * 4096 * 16) and s["pose_c2w"][1] == 480000 and s["pose_focal"][1] == 40000
    assert s["shard_pose0"][1] == 390600 * 4 and s["digests"][1] == (390600 + 3) * 8
    ends = 4096
    for name in R.STORE_SECTIONS:  # in file order, each on a 4096-byte boundary, none overlapping
        assert s[name][0] % 4096 == 0 and s[name][0] >= ends and s[name][0] - ends < 4096
        ends = s[name][0] + s[name][1]
    # the same arguments give the same bytes: no time stamp
    assert raw == R.pack_store_header(1, 4096, 390600, 10000, 400, 400, rank=3, world=8, salt=2**64 - 5, provenance=dict(reversed(list(prov.items()))))
    # a plain store: no pose tables, H = W = 0
    raw0 = R.pack_store_header(0, 4, 3)
    h0 = R.parse_store_header(raw0)
    assert (h0["kind"], h0["H"], h0["W"], h0["n_poses"], h0["salt"], h0["provenance"]) == (0, 0, 0, 0, R.STORE_SALT, {})
    assert h0["sections"] == {"rows": (4096, 3 * 4 * 36), "pose_c2w": (0, 0), "pose_focal": (0, 0), "shard_pose0": (0, 0), "digests": (8192, 24)}
    # through a file
    path = _file(tmp_path, "ok.r2l", raw0)
    assert os.path.getsize(path) == 8192 + 24
    got = R.read_store_header(path)
    assert got["path"] == path and {k: v for k, v in got.items() if k != "path"} == {k: v for k, v in h0.items() if k != "path"}
    assert R.store_rank_path("a/b.r2l") == "a/b.r2l" and R.store_rank_path("a/b.r2l", 2, 4) == "a/b.r2l.rank2of4"
    with pytest.raises(ValueError, match="provenance"):
        R.pack_store_header(0, 4, 3, provenance={"x": "y" * 4000})


def test_header_refusals(tmp_path):
    """Hand-written files: every refusal is a ValueError naming the path and the fact."""
    from r2l_amd import raystore as R
    good = R.pack_store_header(1, 4, 6, 2, 5, 7, provenance={"a": 1})
    size = max(o + n for o, n in R.parse_store_header(good)["sections"].values())

    def patched(at, value):
        b = bytearray(good)
        b[at:at + len(value)] = value
        return bytes(b)

    moved = dict(R.store_layout(1, 4, 6, 2))
    moved["pose_focal"] = (moved["pose_focal"][0] + 8, moved["pose_focal"][1])
    short = dict(R.store_layout(1, 4, 6, 2))
    short["rows"] = (short["rows"][0], short["rows"][1] - 16)
    cases = [("magic", patched(0, b"R2LSTORF"), size, "magic"),
             ("version", patched(8, (2).to_bytes(4, "little")), size, "version 2"),
             ("kind", patched(12, (2).to_bytes(4, "little")), size, "unknown kind 2"),
             ("reserved_a", patched(148, b"\x01"), size, "reserved"),
             ("reserved_b", patched(255, b"\x80"), size, "reserved"),
             ("reserved_c", patched(4095, b"\x01"), size, "reserved"),
             ("reserved_d", patched(256 + len(b'{"a": 1}'), b"x"), size, "reserved"),
             ("cut_by_one", good, size - 1, "truncated"),
             ("cut_in_rows", good, 4096 + 100, "truncated"),
             ("header_only", good, 4096, "truncated"),
             ("half_header", good[:2000], 2000, "truncated"),
             ("empty", b"", 0, "truncated"),
             ("unaligned", R.pack_store_header(1, 4, 6, 2, 5, 7, sections=moved), size + 8, "section pose_focal"),
             ("wrong_length", R.pack_store_header(1, 4, 6, 2, 5, 7, sections=short), size, "section rows"),
             ("rps", R.pack_store_header(1, 6, 6, 2, 5, 7), size * 2, "rays_per_shard"),
             ("no_shards", R.pack_store_header(0, 4, 0), size, "n_shards"),
             ("no_hw", R.pack_store_header(1, 4, 6, 2, 0, 7), size, "H, W"),
             ("rank", R.pack_store_header(0, 4, 6, rank=2, world=2), size * 2, "rank 2 of world 2"),
             ("json", patched(256, b"{'a': 1}"), size, "JSON")]
    for name, header, n, word in cases:
        path = _file(tmp_path, name, header, n)
        with pytest.raises(ValueError) as e:
            R.read_store_header(path)
        assert path in str(e.value) and word in str(e.value), (name, str(e.value))
    assert R.read_store_header(_file(tmp_path, "good", good, size))["n_shards"] == 6
    assert R.read_store_header(_file(tmp_path, "longer", good, size + 1))["n_shards"] == 6  # (only the sections must fit)
    # the refusals of load that need no device: they come before any allocation (this machine may have no GPU at all)
    plain = _file(tmp_path, "plain", R.pack_store_header(0, 4, 6))
    compact = _file(tmp_path, "compact", good, size)
    for cls, path, kw, word in ((R.CompactRayStore, plain, {}, "kind 0"), (R.RayStore, compact, {}, "kind 1"),
                                (R.RayStore, plain, dict(capacity_shards=5), "capacity_shards is 5"),
                                (R.CompactRayStore, compact, dict(capacity_shards=1), "capacity_shards is 1"),
                                (R.RayStore, _file(tmp_path, "cut", good, size - 1), {}, "truncated")):
        with pytest.raises(ValueError) as e:
            cls.load(path, "cuda", **kw)
        assert path in str(e.value) and word in str(e.value), str(e.value)
    with pytest.raises(ValueError, match="truncated"):
        R.load_store(_file(tmp_path, "cut2", good, size - 1), "cuda")
    with pytest.raises(FileNotFoundError):
        R.read_store_header(str(tmp_path / "nothing"))


def test_options(tmp_path):
    from r2l_amd import options
    teacher_cfg = os.path.join(ROOT, "configs", "lego.txt")
    online = ["--r2l_online_kd", "--r2l_teacher_config", teacher_cfg, "--teacher_ckpt", "t.tar", "--n_pose_kd", "12"]
    files = ["--data_mode", "rays", "--datadir_kd", "somewhere"]

    def checked(argv):  # main.py's four checks, in its order
        a = options.parse_args(argv)
        options.validate_accelerated(a)
        options.validate_fused_iter(a)
        options.validate_compact_store(a)
        options.validate_store_file(a)
        return a

    a = options.parse_args([])
    assert a.r2l_store_save == "" and a.r2l_store_load == ""
    checked([])
    assert checked(online + ["--r2l_store_save", "s.r2l"]).r2l_store_save == "s.r2l"
    assert checked(online + ["--r2l_store_save", "s.r2l", "--r2l_compact_store"]).r2l_compact_store
    assert checked(["--r2l_store_load", "s.r2l"]).r2l_store_load == "s.r2l"
    cfg = tmp_path / "student.txt"
    cfg.write_text("r2l_store_load = some/where.r2l\n")
    assert checked(["--config", str(cfg)]).r2l_store_load == "some/where.r2l"
    cfg.write_text("r2l_online_kd = True\nr2l_store_save = out.r2l\nteacher_ckpt = t.tar\nr2l_teacher_config = %s\n" % teacher_cfg)
    assert checked(["--config", str(cfg)]).r2l_store_save == "out.r2l"
    # the start-up refusals, each naming the other flag
    for argv, words in ((["--r2l_store_save", "s"], ("--r2l_store_save", "--r2l_online_kd")),
                        (["--r2l_store_save", "s", "--r2l_device_store"] + files, ("--r2l_store_save", "--r2l_online_kd")),
                        (online + ["--r2l_store_save", "s", "--r2l_kd_every", "2"], ("--r2l_store_save", "--r2l_kd_every")),
                        (online + ["--r2l_store_load", "s"], ("--r2l_store_load", "--r2l_online_kd")),
                        (["--r2l_store_load", "s", "--r2l_device_store"] + files, ("--r2l_store_load", "--r2l_device_store")),
                        (["--r2l_store_load", "s", "--r2l_kd_every", "2"], ("--r2l_kd_every",)),
                        (["--r2l_store_load", "s", "--r2l_store_save", "t"], ("--r2l_store_load", "--r2l_store_save")),
                        # --r2l_compact_store is neither needed nor consulted by a load; its own refusal stays
                        (["--r2l_store_load", "s", "--r2l_compact_store"], ("--r2l_compact_store", "--r2l_online_kd"))):
        with pytest.raises(ValueError) as e:
            checked(argv)
        assert all(w in str(e.value) for w in words), (argv, str(e.value))
    # --r2l_fused_iter: a store file is a ray store; without any of the three sources the refusal is what it was
    a = checked(["--r2l_store_load", "s", "--r2l_fused_iter", "--r2l_device_pool"])
    assert a.r2l_fused_iter and a.r2l_store_load == "s"
    options.validate_fused_iter(a, 1, "cuda")
    with pytest.raises(ValueError) as e:
        checked(["--r2l_fused_iter"])
    assert str(e.value) == "--r2l_fused_iter draws its batches from a ray store: it needs --r2l_device_store or --r2l_online_kd"
    with pytest.raises(ValueError, match="--r2l_device_pool"):
        checked(["--r2l_store_load", "s", "--r2l_fused_iter", "--hard_ratio", "0.2"])
    with pytest.raises(NotImplementedError, match="world size 1"):
        options.validate_fused_iter(a, 2, "cuda")
    # the sibling entry points share the option table and run validate_accelerated alone: utils/create_data.py takes
    # --r2l_store_save without --r2l_online_kd (and needs no --datadir_kd with it), utils/train_nerf.py ignores both
    a = options.parse_args(["--config", teacher_cfg, "--create_data", "rand", "--r2l_store_save", "g.r2l", "--r2l_compact_store"])
    assert a.r2l_store_save == "g.r2l" and a.datadir_kd == ""
    options.validate_accelerated(a)
    from r2l_amd.train_nerf import validate_teacher_training
    a = options.parse_args(["--config", teacher_cfg, "--no_batching", "--r2l_store_save", "g.r2l", "--r2l_store_load", "h.r2l"])
    validate_teacher_training(a)


def test_create_data_store_mode_keeps_the_fused_path_refusals(tmp_path, monkeypatch):
    """utils/create_data.py --r2l_store_save renders through the fused frames path: lindisp, raw_noise_std > 0, a teacher without
    view directions and a run without a GPU are refused before anything is loaded."""
    import torch
    from r2l_amd import create_data
    monkeypatch.chdir(tmp_path)
    teacher_cfg = os.path.join(ROOT, "configs", "lego.txt")
    common = ["--create_data", "rand", "--config", teacher_cfg, "--r2l_store_save", str(tmp_path / "g.r2l"), "--n_pose_kd", "2"]
    for extra in (["--lindisp"], ["--raw_noise_std", "1.0"]):
        with pytest.raises(NotImplementedError, match="fused frames path"):
            create_data.main(common + extra)
    if not torch.cuda.is_available():
        with pytest.raises(NotImplementedError, match="needs a GPU"):
            create_data.main(common)
    assert not os.path.exists(str(tmp_path / "g.r2l"))
