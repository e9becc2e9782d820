"""The numpy restatements of the device samplers and of the store file's header and digest, held to values recorded before
they were gathered into r2l_amd/keyed_perm.py and r2l_amd/store_file.py (tests/golden/sampler_restatements.npz, written by
tests/golden/gen_sampler_restatements.py from restatement_values() below): exact arrays and bytes, no tolerance."""
import os

import numpy as np
import pytest

NS = (1, 2, 5, 17, 4097)
SEEDS = (0, 2**64 - 1)


def _draws(n):
    """(draw0, n_draw): a whole first epoch, from mid-epoch across two epoch boundaries or more, from the last draw of an epoch
    across two, and a few draws far into the run."""
    return (0, n), (n // 2 + 3 * n, 2 * n + 3), (5 * n + n - 1, n + 2), (2**40 + 1, 3)


def restatement_values():
    """{name: array} of every restatement at a handful of small arguments, through the names tests and tools import."""
    from r2l_amd import image_batch, pixel_batch, raystore
    out = {}
    for s, seed in enumerate(SEEDS):
        for n in NS:
            out["perm_s%d_n%d" % (s, n)] = raystore.perm(seed, n)
            for c, (draw0, n_draw) in enumerate(_draws(n)):
                out["shard_ids_s%d_n%d_c%d" % (s, n, c)] = raystore.shard_ids(seed, n, draw0, n_draw)
                out["pixel_ids_s%d_n%d_c%d" % (s, n, c)] = pixel_batch.pixel_ids(seed, n, draw0, n_draw)
        for i, n_img in ((1, 1), (2, 5), (17, 17), (4097, 100), (2**40 + 3, 2**20)):
            out["image_draw_s%d_i%d_n%d" % (s, i, n_img)] = np.array(image_batch.image_draw(seed, i, n_img), dtype=np.uint64)
        # windows: the whole frame, one smaller than the frame, a single pixel, a single row
        for w, (H, W, img, window, n_draw) in enumerate(((5, 17, 0, (0, 0, 5, 17), 85), (17, 5, 3, (2, 1, 11, 3), 20),
                                                         (2, 2, 4096, (1, 1, 1, 1), 1), (70, 64, 1, (69, 3, 1, 59), 59))):
            out["window_ids_s%d_w%d" % (s, w)] = image_batch.window_ids(H, W, img, window, seed ^ 0x5bd1e995, n_draw)
    rng = np.random.RandomState(7)
    for wpi, n_items, salt in ((1, 1, 0), (5, 2, 2**64 - 1), (17, 5, raystore.STORE_SALT), (4097, 2, 3)):
        words = rng.randint(0, 2**32, size=wpi * n_items, dtype=np.uint64).astype(np.uint32)
        out["digest_w%d_n%d" % (wpi, n_items)] = raystore.words_digest_spec(words, wpi, n_items, salt)
    out["header_plain"] = np.frombuffer(raystore.pack_store_header(0, 4096, 17, rank=1, world=2, provenance={"scene": "lego", "n": 5}),
                                        dtype=np.uint8)
    out["header_compact"] = np.frombuffer(raystore.pack_store_header(1, 64, 5, n_poses=2, H=17, W=40, salt=2**64 - 1), dtype=np.uint8)
    return out


@pytest.fixture(scope="module")
def recorded(golden_dir):
    return np.load(os.path.join(golden_dir, "sampler_restatements.npz"))


def test_restatements_equal_the_recorded_values(recorded):
    got = restatement_values()
    assert sorted(got) == sorted(recorded.files)
    for name, a in got.items():
        want = recorded[name]
        assert a.dtype == want.dtype and a.shape == want.shape and np.array_equal(a, want), name


def test_recorded_headers_parse(recorded):
    from r2l_amd import raystore
    h = raystore.parse_store_header(recorded["header_plain"].tobytes())
    assert (h["kind"], h["n_shards"], h["rank"], h["world"], h["provenance"]) == (0, 17, 1, 2, {"scene": "lego", "n": 5})
    h = raystore.parse_store_header(recorded["header_compact"].tobytes())
    assert (h["kind"], h["n_poses"], h["H"], h["W"], h["salt"]) == (1, 2, 17, 40, 2**64 - 1)
    assert h["sections"] == raystore.store_layout(1, 64, 5, 2)


def test_draw_ids_is_both_samplers():
    from r2l_amd import keyed_perm, pixel_batch, raystore
    for seed in SEEDS:
        for n in NS:
            for draw0, n_draw in _draws(n):
                want = keyed_perm.draw_ids(seed, n, draw0, n_draw)
                assert np.array_equal(raystore.shard_ids(seed, n, draw0, n_draw), want)
                assert np.array_equal(pixel_batch.pixel_ids(seed, n, draw0, n_draw), want)
    assert raystore.perm is keyed_perm.perm and raystore.perm_at is keyed_perm.perm_at
    assert raystore.epoch_key is keyed_perm.epoch_key and raystore.M64 == keyed_perm.M64
