"""Store file on the GPU (include/r2l_hip.h r2l_words_digest; raystore.RayStore.save / .load, CompactRayStore.save / .load,
load_store; --r2l_store_save / --r2l_store_load): the digest kernel against its numpy restatement, save -> load round trips of
both kinds, refused corrupt files, and runs that load a file against the runs whose teacher filled the store.  Every comparison
is torch.equal / np.array_equal / bytes ==: there is no tolerance anywhere."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.test_cstore_gpu import SEED, Pair, _group
from tests.test_pool_select_gpu import _ckpt_equal
from tests.test_raystore_gpu import G, _log_of, _student, guarded, guards_ok, tiny  # noqa: F401  (tiny: scene and teacher)

pytestmark = pytest.mark.gpu

PASS, SLICE = 1024, 16384  # words a workgroup takes per pass / per work unit (csrc/r2l_store_digest.hip)
POISON = 0x5A5A5A5A5A5A5A5A


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _digest(words, wpi, n, salt):
    """r2l_words_digest into a poisoned, guarded out: the digests as uint64, after the guards were checked."""
    from r2l_amd import _lib
    buf, out = guarded(n, POISON, torch.int64)
    _lib.check(_lib.load().r2l_words_digest(_p(words), wpi, n, salt, _p(out), _st()), "r2l_words_digest")
    assert guards_ok(buf)
    return out.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("wpi,n", [(1, 1), (3, 1), (13, 3), (4, 1), (36, 5), (16, 3), (PASS, 1), (PASS + 1, 2), (SLICE, 1), (SLICE + 1, 2),
                                   (4096 * 9, 7)])
def test_kernel_equals_the_restatement(wpi, n):
    """(3, 1), (13, 3), PASS + 1, SLICE + 1: tails, and items that do not start on a 16-byte boundary; (36, 5) / (16, 3): the smallest
    plain / compact shards; PASS, SLICE: one pass and one work unit exactly; (4096 * 9, 7): a shard of the real size, three work
    units an item.  Every shape also from a base address 4, 8 and 12 bytes past a 16-byte boundary (heads of 3, 2 and 1 words)."""
    from r2l_amd.raystore import words_digest_spec
    rng = np.random.RandomState(wpi + n)
    fills = {"random": rng.randint(0, 2**32, size=n * wpi, dtype=np.uint64).astype(np.uint32),
             "zeros": np.zeros(n * wpi, np.uint32), "ones": np.full(n * wpi, 0xFFFFFFFF, np.uint32)}
    for name, host in fills.items():
        for salt in (0, 0xFEDCBA9876543210):
            want = words_digest_spec(host, wpi, n, salt)
            for shift in ((0, 1, 2, 3) if name == "random" else (0,)):
                buf = torch.full((G + n * wpi + 4 + G,), -7, dtype=torch.int32, device="cuda")  # (G = 8 words: 32 bytes)
                words = buf[G + shift:G + shift + n * wpi]
                assert words.data_ptr() % 16 == 4 * shift
                words.copy_(torch.from_numpy(host.view(np.int32)))
                keep = buf.clone()
                got = _digest(words, wpi, n, salt)
                assert np.array_equal(got, want), (name, salt, shift, [hex(int(x)) for x in got[:3]], [hex(int(x)) for x in want[:3]])
                assert torch.equal(buf, keep)  # the words are read only
    if n > 1:  # the item's number enters: equal items get different digests
        assert len(set(words_digest_spec(fills["zeros"], wpi, n, 0).tolist())) == n


def test_kernel_no_items_and_many_small_items():
    """n_items == 0 enqueues nothing and writes nothing; 40 000 items of 4 words run through the kernel's stride loop (the grid is
    capped at 32 768 workgroups)."""
    from r2l_amd import _lib
    from r2l_amd.raystore import words_digest_spec
    buf, out = guarded(4, POISON, torch.int64)
    words = torch.zeros(16, dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().r2l_words_digest(_p(words), 4, 0, 0, _p(out), _st()), "r2l_words_digest")
    assert guards_ok(buf) and bool((out == POISON).all())
    n = 40000
    host = np.random.RandomState(1).randint(0, 2**32, size=n * 4, dtype=np.uint64).astype(np.uint32)
    got = _digest(torch.from_numpy(host.view(np.int32)).cuda(), 4, n, 9)
    assert np.array_equal(got, words_digest_spec(host, 4, n, 9))


# ---- save -> load ------------------------------------------------------------------------------------------------------------
def _pair(H=5, W=7, rps=4, groups=((3, [6.5, 7.25, 9.125], 1, 0xC0FFEE1234), (3, [8.5, 6.75, 7.0], 2, 987654321987))):
    """The pair of tests/test_cstore_gpu.py, filled: by default 5 x 7 frames, two groups of 3 poses with a focal per pose at 4
    rays a shard (105 rows a group: 26 shards, one row dropped)."""
    n_sh = sum(K * H * W // rps for K, _, _, _ in groups)
    pair = Pair(n_sh, sum(g[0] for g in groups), H, W, rps, True)
    for K, focals, seed, key in groups:
        pair.append(_group(K, H, W, focals, seed), key)
    assert pair.plain.n_shards == pair.compact.n_shards == n_sh
    return pair


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """The default pair, saved once: {'pair', 'plain': path, 'compact': path, 'info': what the two saves returned}."""
    root = tmp_path_factory.mktemp("store_file")
    pair = _pair()
    out = {"pair": pair, "plain": str(root / "plain.r2l"), "compact": str(root / "compact.r2l"), "root": root}
    out["info"] = [pair.plain.save(out["plain"], provenance={"who": "plain"}), pair.compact.save(out["compact"], provenance={"who": "compact"})]
    return out


def _same_store(a, b):
    assert type(a) is type(b) and (a.n_shards, a.rows_per_file, a.files) == (b.n_shards, b.rows_per_file, b.files)
    n = a.n_shards * a.rows_per_file
    assert torch.equal(a.data[:n], b.data[:n])
    if a.KIND:
        assert (a.n_poses, a.H, a.W) == (b.n_poses, b.H, b.W)
        assert torch.equal(a.pose_c2w[:a.n_poses], b.pose_c2w[:a.n_poses]) and torch.equal(a.pose_focal[:a.n_poses], b.pose_focal[:a.n_poses])
        assert torch.equal(a.shard_pose0[:a.n_shards], b.shard_pose0[:a.n_shards])


def _same_draws(stores, n, calls, seeks=()):
    """next(n) x calls from every store, from draw 0 and from every draw of `seeks`: equal batches and ids."""
    for at in (0,) + tuple(seeks):
        for s in stores:
            s.seek(at)
        for c in range(calls):
            got = [(s.next(n), s.last_ids) for s in stores]
            for b, ids in got[1:]:
                assert torch.equal(b, got[0][0]) and torch.equal(ids, got[0][1]), (at, c)
        assert len({s.draw for s in stores}) == 1 and stores[0].draw == at + n * calls


def test_round_trip_both_kinds(small):
    from r2l_amd import raystore as R
    pair = small["pair"]
    for info, path in zip(small["info"], (small["plain"], small["compact"])):
        assert info["path"] == path and info["bytes"] == os.path.getsize(path) and info["seconds"] > 0 and info["GB/s"] > 0
        assert not os.path.exists(path + ".tmp")
        print(info["message"])
    hp, hc = R.read_store_header(small["plain"]), R.read_store_header(small["compact"])
    assert (hp["kind"], hp["n_shards"], hp["rays_per_shard"], hp["n_poses"], hp["H"], hp["W"], hp["provenance"]) == (0, 52, 4, 0, 0, 0, {"who": "plain"})
    assert (hc["kind"], hc["n_shards"], hc["rays_per_shard"], hc["n_poses"], hc["H"], hc["W"], hc["provenance"]) == (1, 52, 4, 6, 5, 7, {"who": "compact"})
    plain, compact = R.RayStore.load(small["plain"], "cuda", seed=SEED), R.CompactRayStore.load(small["compact"], "cuda", seed=SEED)
    _same_store(pair.plain, plain)
    _same_store(pair.compact, compact)
    assert plain.capacity == 52 and (compact.capacity, compact.capacity_poses) == (52, 6)
    assert plain.describe() == pair.plain.describe() and compact.describe() == pair.compact.describe()
    print(plain.load_info["message"])
    # the dispatcher picks the class from the file; a larger capacity leaves room behind the file's shards
    big, cbig = R.load_store(small["plain"], "cuda", seed=SEED, capacity_shards=60), R.load_store(small["compact"], "cuda", seed=SEED)
    assert type(big) is R.RayStore and big.capacity == 60 and type(cbig) is R.CompactRayStore
    _same_store(pair.plain, big)
    # 52 shards: 12 x next(5) crosses an epoch boundary; then from draw 47 (another crossing) and from draw 210
    _same_draws([pair.plain, plain, compact, big, cbig, pair.compact], 5, 12, seeks=(47, 210))
    # plan(): what r2l_train_batch / r2l_student_train_step are handed
    plain.seek(3)
    pair.plain.seek(3)
    a, b = pair.plain.plan(2), plain.plan(2)
    assert b["ptr"].value == plain.data.data_ptr() and {k: v for k, v in a.items() if k != "ptr"} == {k: v for k, v in b.items() if k != "ptr"}
    with pytest.raises(NotImplementedError):
        compact.plan()
    # a loaded store can be appended to, as a filled one can
    rows = _group(1, 5, 7, 6., 9)[0]
    assert big.append(rows, 5) == 8 and big.n_shards == 60 == len(big.files)
    for s in (plain, compact, big, cbig):
        s.close()
    with pytest.raises(RuntimeError):
        plain.next(5)
    with pytest.raises(RuntimeError):
        compact.next(5)
    # the refusals that name the class and the capacity
    with pytest.raises(ValueError, match="kind 1"):
        R.RayStore.load(small["compact"], "cuda")
    with pytest.raises(ValueError, match="kind 0"):
        R.CompactRayStore.load(small["plain"], "cuda")
    with pytest.raises(ValueError, match="capacity_shards is 51"):
        R.load_store(small["plain"], "cuda", capacity_shards=51)


def test_file_holds_the_store_and_the_restatements_digests(small):
    """Section by section: the bytes of the file are the device's, and the digest section is words_digest_spec of them — one item a
    shard with the header's salt, then one item per pose-table section with salt + n_shards + 0, 1, 2."""
    from r2l_amd import raystore as R
    pair = small["pair"]
    for path, store in ((small["plain"], pair.plain), (small["compact"], pair.compact)):
        h = R.read_store_header(path)
        raw = open(path, "rb").read()
        assert h["salt"] == R.STORE_SALT and len(raw) == h["sections"]["digests"][0] + h["sections"]["digests"][1]
        sec = {name: raw[o:o + n] for name, (o, n) in h["sections"].items()}
        n = store.n_shards
        assert sec["rows"] == store.data[:n * store.rows_per_file].cpu().numpy().tobytes()
        want = [R.words_digest_spec(np.frombuffer(sec["rows"], np.uint32), store.rows_per_file * store.ROW_WORDS, n, h["salt"])]
        if store.KIND:
            assert sec["pose_c2w"] == store.pose_c2w[:store.n_poses].cpu().numpy().tobytes() and len(sec["pose_c2w"]) == 6 * 48
            assert sec["pose_focal"] == store.pose_focal[:store.n_poses].cpu().numpy().tobytes()
            assert sec["shard_pose0"] == store.shard_pose0[:n].cpu().numpy().tobytes()
            for j, name in enumerate(("pose_c2w", "pose_focal", "shard_pose0")):
                w = np.frombuffer(sec[name], np.uint32)
                want.append(R.words_digest_spec(w, w.size, 1, h["salt"] + n + j))
        assert np.array_equal(np.frombuffer(sec["digests"], "<u8"), np.concatenate(want))
        # between the sections: zeros
        at = 4096
        for name in R.STORE_SECTIONS:
            o, ln = h["sections"][name]
            if ln:
                assert not any(raw[at:o])
                at = o + ln


def test_two_saves_are_byte_identical(small, tmp_path):
    pair = small["pair"]
    for store, first in ((pair.plain, small["plain"]), (pair.compact, small["compact"])):
        again = str(tmp_path / "again.r2l")
        store.save(again, provenance={"who": "compact" if store.KIND else "plain"})
        assert open(again, "rb").read() == open(first, "rb").read()
        store.save(again, provenance={"who": "else"}, salt=77)  # (over an existing file; another salt: other digests)
        a, b = open(again, "rb").read(), open(first, "rb").read()
        assert len(a) == len(b) and a != b
        type(store).load(again, "cuda").close()


def test_one_shard_of_4096_rays(tmp_path):
    """rays_per_shard = 4096 with one 64 x 64 group: one shard of the real size (three work units of the digest kernel)."""
    from r2l_amd import raystore as R
    pair = _pair(64, 64, 4096, groups=((1, [70.5], 3, 0x9E3779B97F4A7C15),))
    assert pair.plain.n_shards == 1
    paths = [str(tmp_path / "plain.r2l"), str(tmp_path / "compact.r2l")]
    pair.plain.save(paths[0])
    pair.compact.save(paths[1])
    assert os.path.getsize(paths[0]) == 4096 + 4096 * 36 + 8 and R.read_store_header(paths[1])["sections"]["rows"] == (4096, 65536)
    plain, compact = R.load_store(paths[0], "cuda", seed=SEED), R.load_store(paths[1], "cuda", seed=SEED)
    _same_store(pair.plain, plain)
    _same_store(pair.compact, compact)
    _same_draws([pair.plain, plain, compact], 2, 2)


def _flipped(src, dst, at):
    raw = bytearray(open(src, "rb").read())
    raw[at] ^= 0x10
    with open(dst, "wb") as f:
        f.write(raw)
    return dst


def test_corrupt_files_are_refused(small, tmp_path, monkeypatch):
    from r2l_amd import raystore as R
    for kind, cls in (("plain", R.RayStore), ("compact", R.CompactRayStore)):
        h = R.read_store_header(small[kind])
        row_bytes = 36 if kind == "plain" else 16
        # one byte inside the rows of shard 1 (and of the last shard)
        for shard in (1, 51):
            bad = _flipped(small[kind], str(tmp_path / "bad.r2l"), h["sections"]["rows"][0] + shard * 4 * row_bytes + 5)
            with pytest.raises(ValueError) as e:
                cls.load(bad, "cuda")
            assert bad in str(e.value) and "digest mismatch in shard %d " % shard in str(e.value), str(e.value)
        # a digest itself
        bad = _flipped(small[kind], str(tmp_path / "bad.r2l"), h["sections"]["digests"][0] + 8 * 7)
        with pytest.raises(ValueError, match="digest mismatch in shard 7 "):
            R.load_store(bad, "cuda")
    h = R.read_store_header(small["compact"])
    for name in ("pose_c2w", "pose_focal", "shard_pose0"):
        bad = _flipped(small["compact"], str(tmp_path / "bad.r2l"), h["sections"][name][0] + 6)
        with pytest.raises(ValueError) as e:
            R.CompactRayStore.load(bad, "cuda")
        assert bad in str(e.value) and "digest mismatch in section %s " % name in str(e.value), str(e.value)
    # a file cut one byte short is refused before anything is allocated on the device
    def no_store(self, *a, **kw):
        raise AssertionError("a store was allocated for a truncated file")
    monkeypatch.setattr(R.RayStore, "__init__", no_store)
    monkeypatch.setattr(R.CompactRayStore, "__init__", no_store)
    for kind, cls in (("plain", R.RayStore), ("compact", R.CompactRayStore)):
        raw = open(small[kind], "rb").read()
        cut = str(tmp_path / "cut.r2l")
        with open(cut, "wb") as f:
            f.write(raw[:-1])
        before = torch.cuda.memory_allocated()
        for load in (cls.load, R.load_store):
            with pytest.raises(ValueError) as e:
                load(cut, "cuda")
            assert cut in str(e.value) and "truncated" in str(e.value)
        assert torch.cuda.memory_allocated() <= before  # (less: tensors of the refused loads above may be collected meanwhile)
    # an empty store has nothing to save
    monkeypatch.undo()
    with pytest.raises(ValueError, match="empty"):
        R.RayStore(2, "cuda", rays_per_shard=4).save(str(tmp_path / "empty.r2l"))
    assert not os.path.exists(str(tmp_path / "empty.r2l"))


# ---- command line --------------------------------------------------------------------------------------------------------------
RUN = ["--r2l_device_pool", "--r2l_precision", "fp32_mfma", "--i_weights", "3", "--save_intermediate_models", "--N_iters", "6"]


def _main(work, argv):
    """driver.main in the directory `work`: (absolute weights path, log text)."""
    from r2l_amd import driver
    cwd = os.getcwd()
    os.chdir(str(work))
    try:
        res = driver.main(argv)
        return os.path.join(str(work), res["logger"].weights_path), _log_of(res)
    finally:
        os.chdir(cwd)


@pytest.fixture(scope="module")
def saved(tiny, tmp_path_factory):  # noqa: F811
    """(a) and the saving half of (d): six iterations of main.py --r2l_online_kd --r2l_store_save, three poses in flush groups of two
    and one, checkpoints at 3 and 6, without and with --r2l_compact_store.  Exact-fp32 kernels, as tests/test_cstore_gpu.py runs them."""
    work = tmp_path_factory.mktemp("store_cli")
    online = ["--r2l_online_kd", "--r2l_teacher_config", tiny["teacher_cfg"], "--teacher_ckpt", tiny["ck"], "--n_pose_kd", "3",
              "--create_data_chunk", "2"]
    out = {"work": work, "F": str(work / "F.r2l"), "Fc": str(work / "Fc.r2l")}
    out["plain"], out["plain_log"] = _main(work, _student(tiny, "save_plain") + online + RUN + ["--r2l_store_save", out["F"]])
    out["compact"], out["compact_log"] = _main(work, _student(tiny, "save_compact") + online + RUN +
                                               ["--r2l_compact_store", "--r2l_store_save", out["Fc"]])
    return out


def _equal_ckpts(a, b, names=("ckpt_3.tar", "ckpt_6.tar")):
    from r2l_amd.checkpoint import load_ckpt
    for name in names:
        x, y = load_ckpt(os.path.join(a, name)), load_ckpt(os.path.join(b, name))
        assert _ckpt_equal(x, y) == (True, True), name
        assert x["global_step"] == y["global_step"]


@pytest.mark.parametrize("kind", ["plain", "compact"])
def test_cli_load_is_the_run_that_filled(saved, tiny, kind):  # noqa: F811
    """(b), (c), (d): a run that loads the file leaves the checkpoints of the run whose teacher filled the store, and resumed from
    its ckpt_3.tar it ends on ckpt_6.tar's bits.  The kind comes from the file: --r2l_compact_store is not given."""
    from r2l_amd import raystore as R
    path = saved["F" if kind == "plain" else "Fc"]
    h = R.read_store_header(path)
    assert (h["kind"], h["n_shards"], h["rays_per_shard"], h["rank"], h["world"]) == (int(kind == "compact"), 3, 4096, 0, 1)
    assert (h["H"], h["W"], h["n_poses"]) == ((64, 64, 3) if kind == "compact" else (0, 0, 0))
    p = h["provenance"]
    assert p["teacher_ckpt"] == tiny["ck"] and (p["n_pose"], p["create_data_chunk"], p["near"], p["far"], p["ndc"]) == (3, 2, 2., 6., False)
    assert p["precision"] and p["R2L_SEED"] == "0" and {"N_samples", "N_importance", "perturb", "white_bkgd", "use_rand_focal", "focal"} <= set(p)
    assert "ray store: saved 3 shards to %s" % path in saved[kind + "_log"]
    assert saved[kind + "_log"].index("ray store: saved") < saved[kind + "_log"].index("Begin training")
    _equal_ckpts(saved["plain"], saved["compact"])  # (the compact store's batches are the plain store's)
    w, log = _main(saved["work"], _student(tiny, "load_" + kind) + RUN + ["--r2l_store_load", path])
    assert "ray store file %s: provenance {" % path in log and "ray store: loaded 3 shards from %s" % path in log
    assert ("%d digests verified" % (6 if kind == "compact" else 3)) in log and "teacher rendered" not in log
    assert ("ray store: compact, 3 / 3 shards" if kind == "compact" else "ray store: 3 / 3 shards of 4096 rays") in log
    assert log.count("[TRAIN] Iter") == 6
    _equal_ckpts(saved[kind], w)
    w2, log = _main(saved["work"], _student(tiny, "resume_" + kind) + RUN +
                    ["--r2l_store_load", path, "--pretrained_ckpt", os.path.join(w, "ckpt_3.tar"), "--resume"])
    assert "resuming at draw 6" in log
    assert [l.split("[TRAIN] Iter ")[1].split()[0] for l in log.splitlines() if "[TRAIN] Iter" in l] == ["4", "5", "6"]
    _equal_ckpts(saved[kind], w2, names=("ckpt_6.tar",))


@pytest.mark.parametrize("kind", ["plain", "compact"])
def test_cli_create_data_writes_the_same_store(saved, tiny, kind):  # noqa: F811
    """(e): utils/create_data.py --r2l_store_save renders the very rows main.py --r2l_online_kd renders: behind the header (whose
    provenance may differ) the file is F's byte for byte — every section and every digest.  No shard files, no --datadir_kd."""
    import glob
    from r2l_amd import create_data
    from r2l_amd import raystore as R
    G_ = str(saved["work"] / ("G_%s.r2l" % kind))
    cwd = os.getcwd()
    os.chdir(str(saved["work"]))
    try:
        out = create_data.main(["--create_data", "rand", "--config", tiny["teacher_cfg"], "--datadir", tiny["scene"], "--teacher_ckpt", tiny["ck"],
                                "--n_pose_kd", "3", "--create_data_chunk", "2", "--r2l_precision", "fp32_mfma", "--experiment_name", "cd_" + kind,
                                "--r2l_store_save", G_] + (["--r2l_compact_store"] if kind == "compact" else []))
    finally:
        os.chdir(cwd)
    assert out["store_file"] == G_ and out["n_rays"] == 3 * 4096
    a, b = open(saved["F" if kind == "plain" else "Fc"], "rb").read(), open(G_, "rb").read()
    assert len(a) == len(b) and a[4096:] == b[4096:]
    ha, hb = R.read_store_header(saved["F" if kind == "plain" else "Fc"]), R.read_store_header(G_)
    drop = ("path", "provenance")
    assert {k: v for k, v in ha.items() if k not in drop} == {k: v for k, v in hb.items() if k not in drop}
    assert hb["provenance"]["teacher_ckpt"] == tiny["ck"] and hb["provenance"]["n_pose"] == 3
    assert glob.glob(os.path.join(str(saved["work"]), "**", "*.npy"), recursive=True) == []


def test_cli_fused_iter_from_a_plain_file(saved, tiny):  # noqa: F811
    """(f): a plain file satisfies --r2l_fused_iter's need for a store, and the one-call iteration leaves the staged run's bits."""
    w, log = _main(saved["work"], _student(tiny, "fused") + RUN + ["--r2l_store_load", saved["F"], "--r2l_fused_iter"])
    assert "Fused iteration (--r2l_fused_iter)" in log and "ray store: loaded 3 shards" in log
    _equal_ckpts(saved["plain"], w)


def test_cli_refusals_after_the_header_is_read(saved, tiny, tmp_path):  # noqa: F811
    from r2l_amd import raystore as R

    def written(name, header):
        path = str(tmp_path / name)
        with open(path, "wb") as f:
            f.write(header)
            f.truncate(max(o + n for o, n in R.parse_store_header(header)["sections"].values()))
        return path

    cases = [(written("rank.r2l", R.pack_store_header(0, 4096, 3, rank=1, world=2)), [], "written by rank 1 of 2"),
             (written("hw.r2l", R.pack_store_header(1, 4096, 3, 3, 32, 64)), [], "32 x 64 frames, the scene is 64 x 64"),
             (written("few.r2l", R.pack_store_header(0, 4096, 1)), [], "1 shards, one step of this rank draws 2"),
             (saved["Fc"], ["--r2l_fused_iter"], "--r2l_fused_iter")]
    for path, extra, word in cases:
        with pytest.raises(ValueError) as e:
            _main(saved["work"], _student(tiny, "refused") + RUN + ["--r2l_store_load", path] + extra)
        assert path in str(e.value) and word in str(e.value), str(e.value)
    with pytest.raises(FileNotFoundError):
        _main(saved["work"], _student(tiny, "refused") + RUN + ["--r2l_store_load", str(tmp_path / "nothing.r2l")])
