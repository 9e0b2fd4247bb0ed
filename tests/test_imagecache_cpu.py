"""The uint8 image cache without a GPU (xmc_gan_amd/imagecache.py, xmc_gan/image_cache.py): what the build tool writes, what loading
refuses, the sampling rule of the loader, the host-side bounds check of `ops.crop_flip_normalize` and its look-up table."""
import os
import shutil
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]

import datafeed_ref as R  # noqa: E402
from xmc_gan_amd import imagecache as IC  # noqa: E402

S = 8                                   # train: Resize(9)
# (width, height) of the JPEGs: landscape, portrait, shorter side already 9 (Resize hands the image back untouched), square, a wide one whose
# resized width makes 3 * w odd
SIZES = [(40, 30), (30, 47), (13, 9), (21, 21), (50, 18)]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("coco")
    data_dir, keys = R.mini_tree(root / "data", SIZES)
    out = str(root / "cache")
    import xmc_gan.image_cache as CLI
    for split in ("train", "test"):
        CLI.main(["build", "--data_dir", data_dir, "--imsize", str(S), "--split", split, "--out", out, "--threads", "3"])
    return data_dir, keys, out


@pytest.mark.parametrize("split", ["train", "test"])
def test_the_tool_writes_resize_applied_by_hand(tree, split):
    data_dir, keys, out = tree
    cache = IC.ImageCache.load(out, split, S, keys)
    assert cache.keys == keys and len(cache) == len(SIZES)
    raw = np.fromfile(cache.u8_path, dtype=np.uint8)
    assert raw.size == cache.nbytes and raw.size % 16 == 0
    end = 0
    for i, k in enumerate(keys):
        want = R.resized_by_hand(os.path.join(data_dir, "images", f"{k}.jpg"), split, S)
        h, w, o = int(cache.heights[i]), int(cache.widths[i]), int(cache.offsets[i])
        assert (h, w) == want.shape[:2] and o % 16 == 0 and o >= end
        assert not raw[end:o].any()                                        # alignment padding is zero
        assert np.array_equal(raw[o:o + h * w * 3].reshape(h, w, 3), want)
        assert np.array_equal(cache.image(i), want)
        end = o + h * w * 3
    assert raw.size - end >= 16 and not raw[end:].any()                    # the tail an aligned load of the last pixel may touch
    hw = list(zip(cache.heights.tolist(), cache.widths.tolist()))
    if split == "train":
        # shorter side 9, aspect kept; the 13 x 9 image is the JPEG's own bytes
        assert hw == [(9, 12), (14, 9), (9, 13), (9, 9), (9, 25)]
        from PIL import Image
        assert np.array_equal(cache.image(2), np.array(Image.open(os.path.join(data_dir, "images", "k002.jpg")).convert("RGB")))
    else:
        assert hw == [(S, S)] * len(SIZES)                                 # every test image ends up exactly S x S
    assert cache.offsets.dtype == np.int64 and cache.heights.dtype == np.int32 and cache.widths.dtype == np.int32


def _copy(out, dst, split="train", size=S, new_size=None):
    os.makedirs(dst, exist_ok=True)
    for a, b in zip(IC.cache_paths(out, split, size), IC.cache_paths(dst, split, new_size or size)):
        shutil.copy(a, b)
    return dst


def _rewrite_index(cache_dir, **changes):
    idx = IC.cache_paths(cache_dir, "train", S)[1]
    with np.load(idx) as z:
        d = {k: z[k] for k in z.files}
    d.update(changes)
    with open(idx, "wb") as f:
        np.savez(f, **d)


def test_loading_refuses_what_does_not_match(tree, tmp_path):
    data_dir, keys, out = tree
    with pytest.raises(ValueError, match="image_cache.py build"):           # no cache of that size at all
        IC.ImageCache.load(out, "train", 16, keys)
    d = _copy(out, str(tmp_path / "size"), new_size=16)                     # a cache built for another size under this size's name
    with pytest.raises(ValueError, match="size 8.*image_cache.py build"):
        IC.ImageCache.load(d, "train", 16, keys)
    with pytest.raises(ValueError, match="keys.*image_cache.py build"):     # other keys
        IC.ImageCache.load(out, "train", S, keys[:-1] + ["other"])
    with pytest.raises(ValueError, match="keys"):                           # the same keys in another order
        IC.ImageCache.load(out, "train", S, keys[::-1])
    d = _copy(out, str(tmp_path / "trunc"))                                 # a truncated .u8
    u8 = IC.cache_paths(d, "train", S)[0]
    with open(u8, "r+b") as f:
        f.truncate(os.path.getsize(u8) - 32)
    with pytest.raises(ValueError, match="bytes.*image_cache.py build"):
        IC.ImageCache.load(d, "train", S, keys)
    d = _copy(out, str(tmp_path / "misaligned"))                            # a misaligned offset
    off = IC.ImageCache.load(out, "train", S, keys).offsets.copy()
    off[2] += 4
    _rewrite_index(d, offsets=off)
    with pytest.raises(ValueError, match="16-byte aligned"):
        IC.ImageCache.load(d, "train", S, keys)
    d = _copy(out, str(tmp_path / "overlap"))                               # aligned, but image 1 starts inside image 0
    off = IC.ImageCache.load(out, "train", S, keys).offsets.copy()
    off[1] = 16
    _rewrite_index(d, offsets=off)
    with pytest.raises(ValueError, match="increasing"):
        IC.ImageCache.load(d, "train", S, keys)
    d = _copy(out, str(tmp_path / "version"))
    _rewrite_index(d, version=IC.FORMAT_VERSION + 1)
    with pytest.raises(ValueError, match="version"):
        IC.ImageCache.load(d, "train", S, keys)
    d = _copy(out, str(tmp_path / "split"))                                 # the test split's files under the train split's names
    for a, b in zip(IC.cache_paths(out, "test", S), IC.cache_paths(d, "train", S)):
        shutil.copy(a, b)
    with pytest.raises(ValueError, match="split 'test'"):
        IC.ImageCache.load(d, "train", S, keys)


@pytest.mark.parametrize("world", [1, 2])
def test_sampling_partitions_a_permutation(world):
    n, bs, seed = 23, 4, 5
    hw = np.stack([np.arange(n) % 5 + 9, np.arange(n) % 7 + 9], 1).astype(np.int32)
    per_epoch = []
    for epoch in (1, 2, 3):
        ranks = [IC.epoch_indices(n, bs, seed, epoch, r, world) for r in range(world)]
        perm = np.random.default_rng([seed, epoch]).permutation(n)
        n_local = n // world
        for r, idx in enumerate(ranks):
            assert idx.shape == (n_local // bs, bs) and idx.dtype == np.int64             # drop_last: whole batches only
            assert np.array_equal(idx.ravel(), perm[r::world][:n_local][:n_local // bs * bs])
            assert np.array_equal(idx, IC.epoch_indices(n, bs, seed, epoch, r, world))    # same seed, same draws
            p = IC.epoch_params(idx, hw, S, seed, epoch, r)
            assert p.shape == idx.shape + (4,) and p.dtype == np.int32
            assert np.array_equal(p, IC.epoch_params(idx, hw, S, seed, epoch, r))
            assert np.array_equal(p[..., 0], idx)
            h, w = hw[idx, 0], hw[idx, 1]
            assert (p[..., 1] >= 0).all() and (p[..., 1] <= h - S).all() and (p[..., 2] >= 0).all() and (p[..., 2] <= w - S).all()
            assert set(np.unique(p[..., 3])) <= {0, 1}
            from xmc_gan_amd import ops
            for b in range(len(p)):
                ops.validate_crop_params(p[b], hw, S)
        flat = np.concatenate([i.ravel() for i in ranks])
        assert len(set(flat.tolist())) == len(flat)                                       # no image twice in an epoch, over all ranks
        assert set(flat.tolist()) <= set(perm[:n_local * world].tolist())                 # all from the permutation's prefix
        per_epoch.append(flat)
    assert not np.array_equal(per_epoch[0], per_epoch[1]) and not np.array_equal(per_epoch[1], per_epoch[2])
    assert not np.array_equal(IC.epoch_indices(n, bs, seed + 1, 1), IC.epoch_indices(n, bs, seed, 1))
    if world == 2:                                                                        # the ranks draw different crops
        i0 = IC.epoch_indices(400, 100, seed, 1, 0, 2)
        big = np.full((400, 2), 40, np.int32)
        assert not np.array_equal(IC.epoch_params(i0, big, S, seed, 1, 0)[..., 1:], IC.epoch_params(i0, big, S, seed, 1, 1)[..., 1:])


def test_sampling_is_uniform_over_the_offsets_and_flips():
    """4 000 draws over 3 x 5 possible offsets: every offset and both flips occur, each within 5 sigma of its share"""
    idx = np.zeros((40, 100), np.int64)
    hw = np.array([[S + 2, S + 4]], np.int32)
    p = IC.epoch_params(idx, hw, S, 0, 1).reshape(-1, 4)
    n = len(p)
    for col, k in ((1, 3), (2, 5), (3, 2)):
        counts = np.bincount(p[:, col], minlength=k)
        assert len(counts) == k
        sigma = np.sqrt(n * (1 / k) * (1 - 1 / k))
        assert (np.abs(counts - n / k) <= 5 * sigma).all(), (col, counts)


def test_evaluation_order_and_drop_last():
    idx, p = IC.ordered_params(11, 4)
    assert np.array_equal(idx, np.arange(8).reshape(2, 4)) and np.array_equal(p[..., 0], idx) and not p[..., 1:].any()
    assert IC.epoch_indices(3, 4, 0, 1).shape == (0, 4)                                   # fewer images than a batch: no batch


def test_the_params_validator_rejects_each_kind_of_row():
    from xmc_gan_amd import ops
    hw = np.array([[9, 12], [14, 9]], np.int32)
    good = np.array([[0, 1, 4, 0], [1, 6, 1, 1], [1, 0, 0, 0]], np.int32)
    ops.validate_crop_params(good, hw, S)
    for row, what in (([-1, 0, 0, 0], "index below 0"), ([2, 0, 0, 0], "index == N"), ([0, -1, 0, 0], "top below 0"),
                      ([0, 2, 0, 0], "top > h - S"), ([0, 0, -1, 0], "left below 0"), ([0, 0, 5, 0], "left > w - S"),
                      ([1, 0, 2, 0], "left > w - S of the second image"), ([0, 0, 0, 2], "flip 2"), ([0, 0, 0, -1], "flip -1")):
        bad = good.copy()
        bad[1] = row
        with pytest.raises(ValueError, match="row 1"):
            ops.validate_crop_params(bad, hw, S)
    with pytest.raises(ValueError):
        ops.validate_crop_params(good.astype(np.int64), hw, S)                            # the kernel reads int32
    with pytest.raises(ValueError):
        ops.validate_crop_params(good[:, :3], hw, S)
    with pytest.raises(ValueError):
        ops.validate_crop_params(good[:0], hw, S)
    with pytest.raises(ValueError, match="row 0"):
        ops.validate_crop_params(good, hw, 16)                                            # a crop larger than the images


def test_the_table_is_to_normalized_tensor_of_every_byte():
    from xmc_gan.dataset import to_normalized_tensor
    from xmc_gan_amd import ops
    table = ops.normalize_table()
    assert table.dtype == torch.float32 and tuple(table.shape) == (256,)
    rgb = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)             # a 1 x 256 RGB image, pixel v = (v, v, v)
    want = to_normalized_tensor(rgb)
    for c in range(3):
        assert torch.equal(table, want[c, 0])
    assert float(table[0]) == -1.0 and float(table[255]) == 1.0 and (table[1:] > table[:-1]).all()


def test_build_uses_at_most_16_threads_and_no_cpu_count(tree, monkeypatch):
    import concurrent.futures
    data_dir, keys, out = tree
    seen = []

    class Pool(concurrent.futures.ThreadPoolExecutor):
        def __init__(self, n):
            seen.append(n)
            super().__init__(n)
    monkeypatch.setattr(IC, "ThreadPoolExecutor", Pool)
    monkeypatch.setattr(os, "cpu_count", lambda: (_ for _ in ()).throw(AssertionError("sized from os.cpu_count()")))
    IC.build_cache(data_dir, S, "test", out, threads=64)
    IC.build_cache(data_dir, S, "test", out)
    assert seen[0] == 16 and 1 <= seen[1] <= 16


def test_text_only_dataset_never_opens_an_image(tree):
    """the loader's text dataset is the existing class with transform=None; gathering its captions touches no image file"""
    from xmc_gan.dataset import WordTextDataset
    data_dir, keys, out = tree
    cfg = types.SimpleNamespace(IMG=types.SimpleNamespace(SIZE=S), TEXT=types.SimpleNamespace(CAPTIONS_PER_IMAGE=5, MAX_LENGTH=6))
    ds = WordTextDataset(data_dir=data_dir, mode="train", transform=None, cfg=cfg)
    assert [str(k) for k in ds.filenames] == keys
    cap, n = ds.get_caption(0 * 5 + 1)
    assert cap.shape == (6,) and 1 <= n <= 6


# ------------------------------------------------------------------------------------------ the C ABI, without a GPU
def test_header_makefile_and_binding_declare_the_entry_point():
    import re
    import xmc_gan_amd.lib as L
    hdr = open(os.path.join(ROOT, "include", "xmc_gan_hip.h")).read()
    assert "xmc_crop_flip_normalize" in set(re.findall(r"\b(xmc_[a-z0-9_]+)\s*\(", hdr))
    note = hdr[hdr.index("Added without a new version"):hdr.index("#define XMC_ABI_VERSION")]
    assert "xmc_crop_flip_normalize" in note and "datafeed.hip" in note
    mk = open(os.path.join(ROOT, "xmc-gan_amd", "csrc", "Makefile")).read()
    assert "datafeed.hip" in mk[mk.index("SRCS"):mk.index("OBJS")]
    assert "xmc_crop_flip_normalize" in L.EXPORTS
    src = open(os.path.join(ROOT, "xmc-gan_amd", "csrc", "datafeed.hip")).read()
    assert "atomic" not in src.replace("No atomics", "") and "asm" not in src


@pytest.mark.parametrize("variant", ["bf16", "f16"])
def test_both_builds_refuse_bad_arguments_before_any_launch(variant):
    """NULL pointer, N < 1, a pool that is no multiple of 16 bytes -> XMC_EINVAL; B < 1, S < 8, S % 8 != 0, S > 1024 -> XMC_ESHAPE; a misaligned
    pool, out or offsets -> XMC_EALIGN.  None of these calls launches, so this runs without a GPU."""
    import ctypes
    import xmc_gan_amd.lib as L
    f = L.load(variant).xmc_crop_flip_normalize
    EINVAL, EALIGN, ESHAPE = -1, -2, -3
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 4)
    good = [p, 4096, p, p, 1, p, p, p, 1, 8, None]               # pool, bytes, offsets, hw, N, params, table, out, B, S, stream

    def call(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return f(*a)
    for i in (0, 2, 3, 5, 6, 7):
        assert call(**{f"a{i}": None}) == EINVAL
    assert call(a4=0) == EINVAL and call(a1=8) == EINVAL and call(a1=4100) == EINVAL and call(a1=0) == EINVAL
    assert call(a8=0) == ESHAPE and call(a9=0) == ESHAPE and call(a9=4) == ESHAPE and call(a9=12) == ESHAPE and call(a9=1032) == ESHAPE
    assert call(a9=-8) == ESHAPE
    assert call(a0=odd) == EALIGN and call(a7=odd) == EALIGN and call(a2=odd) == EALIGN
