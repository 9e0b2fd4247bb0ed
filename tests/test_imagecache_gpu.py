"""The uint8 image cache on the GPU: `ops.crop_flip_normalize` (csrc/datafeed.hip) bit for bit against the PIL operations it replaces
(tests/datafeed_ref.py), the host-side refusal of bad params, `DeviceImageLoader` against its own `last_params` and against the DataLoader
it stands in for, and ``train_gan.py --image_cache`` end to end on a miniature COCO-layout tree.  No worker process is started anywhere."""
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]

import datafeed_ref as R  # noqa: E402
from golden_util import CFG_DIR  # noqa: E402


# ------------------------------------------------------------------------------------------------------------------------ the kernel
def _pool(S, seed):
    """A hand-laid pool in the cache's format: (h, w) chosen so that 3 * w is odd (77, 101: rows start at every byte phase), an image of
    exactly S x S in the middle, a first and a last image with room to crop at their far corners.  Returns (images, bytes, offsets, hw)."""
    rng = np.random.RandomState(seed)
    dims = [(S + 3, 77 if S < 77 else S + 13), (S, S), (S + 2, 101 if S < 101 else S + 37), (S + 1, S + 16), (S + 5, S + 19)]
    images = [rng.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in dims]
    buf, offsets = bytearray(), []
    for im in images:
        buf += b"\0" * ((-len(buf)) % 16)
        offsets.append(len(buf))
        buf += im.tobytes()
    buf += b"\0" * ((-len(buf)) % 16 + 16)
    return images, np.frombuffer(bytes(buf), dtype=np.uint8), np.array(offsets, np.int64), np.array(dims, np.int32)


def _cases(S, offsets, hw):
    """the rows the issue lists; returns int32 [B,4]"""
    rows = []
    n = len(hw)
    for i in range(n):                                                  # every corner of every image, both flips
        h, w = int(hw[i, 0]), int(hw[i, 1])
        for top in sorted({0, h - S}):
            for left in sorted({0, w - S}):
                rows += [(i, top, left, 0), (i, top, left, 1)]
    i = 3                                                               # left = 0..15 at w = S + 16: 3 * left runs over every residue mod 16
    for left in range(16):
        rows.append((i, 1, left, left & 1))
    for i in (0, 2):                                                    # odd 3 * w: a different phase in every source row
        for left in (1, 2, 3, 5):
            rows.append((i, 1, left, 0))
    rows += [rows[3], rows[3]]                                          # the same crop of the same image twice more in one batch
    p = np.array(rows, np.int32)
    first = offsets[p[:, 0]] + (p[:, 1].astype(np.int64) * hw[p[:, 0], 1] + p[:, 2]) * 3
    assert set((first % 16).tolist()) == set(range(16))                 # the first source byte's address covers every residue mod 16
    assert (1, 0, 0, 0) in rows and (1, 0, 0, 1) in rows                # the S x S image
    last = n - 1
    assert (last, int(hw[last, 0]) - S, int(hw[last, 1]) - S, 0) in rows and (0, 0, 0, 1) in rows
    return p


@pytest.fixture(scope="module", params=[8, 64])
def pool_case(request):
    from xmc_gan_amd import ops
    S = request.param
    images, raw, offsets, hw = _pool(S, seed=S)
    params = _cases(S, offsets, hw)
    dev = torch.device("cuda", 0)
    return dict(S=S, images=images, params=params, ref=R.batch_ref(images, params, S), pool=torch.from_numpy(raw.copy()).to(dev),
                offsets=torch.from_numpy(offsets).to(dev), hw=ops.HostMirror(hw, dev))


def test_kernel_equals_the_pil_path_bit_for_bit(pool_case):
    from xmc_gan_amd import ops
    c = pool_case
    out = ops.crop_flip_normalize(c["pool"], c["offsets"], c["hw"], c["params"], c["S"])
    assert out.dtype == torch.float32 and tuple(out.shape) == (len(c["params"]), 3, c["S"], c["S"]) and out.is_contiguous()
    got = out.cpu()
    for b in range(len(got)):
        assert torch.equal(got[b], c["ref"][b]), (b, c["params"][b].tolist())
    assert float(got.min()) >= -1.0 and float(got.max()) <= 1.0 and float(got.std()) > 0.3


@pytest.mark.parametrize("B", [1, 5])
def test_kernel_small_batches_and_the_callers_out(pool_case, B):
    from xmc_gan_amd import ops
    c = pool_case
    pick = np.arange(len(c["params"]))[-B - 7:][:B]                     # mixed images, flips and phases
    params = np.ascontiguousarray(c["params"][pick])
    out = torch.full((B, 3, c["S"], c["S"]), 7.0, device=c["pool"].device)
    ret = ops.crop_flip_normalize(c["pool"], c["offsets"], c["hw"], ops.HostMirror(params, c["pool"].device), c["S"], out=out)
    assert ret is out
    assert torch.equal(out.cpu(), c["ref"][torch.from_numpy(pick)])


def test_bad_params_raise_before_any_launch(pool_case, monkeypatch):
    from xmc_gan_amd import ops
    import xmc_gan_amd.lib as L
    c = pool_case
    S, hw = c["S"], c["hw"].host
    calls = []
    monkeypatch.setattr(L, "call", lambda name, *a: calls.append(name))
    good = c["params"][:3].copy()
    n = len(hw)
    for row in ([-1, 0, 0, 0], [n, 0, 0, 0], [0, -1, 0, 0], [0, int(hw[0, 0]) - S + 1, 0, 0], [0, 0, -1, 0], [0, 0, int(hw[0, 1]) - S + 1, 0],
                [1, 1, 0, 0], [1, 0, 1, 0], [0, 0, 0, 2]):
        bad = good.copy()
        bad[2] = row
        with pytest.raises(ValueError, match="row 2"):
            ops.crop_flip_normalize(c["pool"], c["offsets"], c["hw"], bad, S)
        with pytest.raises(ValueError, match="row 2"):
            ops.crop_flip_normalize(c["pool"], c["offsets"], c["hw"], ops.HostMirror(bad, c["pool"].device), S)
    with pytest.raises(TypeError):                                      # device-only params cannot be checked without a read-back
        ops.crop_flip_normalize(c["pool"], c["offsets"], c["hw"], torch.from_numpy(good).to(c["pool"].device), S)
    with pytest.raises(TypeError):
        ops.crop_flip_normalize(c["pool"], c["offsets"], c["hw"].dev, good, S)
    assert calls == []                                                  # nothing reached the library


def test_a_size_that_is_no_multiple_of_8_is_the_librarys_shape_error(pool_case):
    from xmc_gan_amd import ops
    import xmc_gan_amd.lib as L
    c = pool_case
    S = c["S"] - 4                                                      # fits every image, 4 mod 8
    with pytest.raises(L.XmcHipError, match="XMC_ESHAPE"):
        ops.crop_flip_normalize(c["pool"], c["offsets"], c["hw"], np.array([[0, 0, 0, 0]], np.int32), S)


# ------------------------------------------------------------------------------------------------------------------------ the loader
S_LOADER = 8
SIZES = [(40, 30), (30, 47), (13, 9), (21, 21), (50, 18), (33, 20), (19, 31), (64, 48), (25, 25), (31, 17), (12, 44)]     # (width, height)


def _cfg(size, max_length=6):
    return types.SimpleNamespace(IMG=types.SimpleNamespace(SIZE=size), TEXT=types.SimpleNamespace(CAPTIONS_PER_IMAGE=5, MAX_LENGTH=max_length))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from xmc_gan_amd import imagecache as IC
    root = tmp_path_factory.mktemp("coco")
    data_dir, keys = R.mini_tree(root / "data", SIZES, sent=True)
    out = str(root / "cache")
    for split in ("train", "test"):
        IC.build_cache(data_dir, S_LOADER, split, out, threads=2)
    return data_dir, keys, out


def _same_layout(a, b):
    """two loader batches: same container lengths, leaf types, dtypes and shapes"""
    (ia, ta, ka), (ib, tb, kb) = a, b
    assert torch.is_tensor(ia) and torch.is_tensor(ib) and ia.dtype == ib.dtype == torch.float32 and ia.shape == ib.shape
    assert len(ta) == len(tb) == 1 and len(ta[0]) == len(tb[0]) == 2
    (ca, la), (cb, lb) = ta[0], tb[0]
    assert torch.is_tensor(la) and torch.is_tensor(lb) and la.dtype == lb.dtype == torch.int64 and la.shape == lb.shape
    if torch.is_tensor(cb):
        assert torch.is_tensor(ca) and ca.dtype == cb.dtype == torch.int64 and ca.shape == cb.shape and not ca.is_cuda and not cb.is_cuda
    else:   # (a batch of str: a list here; default_collate hands it back as a list or a tuple, depending on the torch version)
        assert isinstance(ca, list) and isinstance(cb, (list, tuple)) and len(ca) == len(cb) and all(isinstance(s, str) for s in list(ca) + list(cb))
    assert isinstance(ka, list) and isinstance(kb, (list, tuple)) and len(ka) == len(kb) and all(isinstance(k, str) for k in list(ka) + list(kb))


@pytest.mark.parametrize("text", ["WORD", "SENT"])
def test_loader_epoch_equals_the_reference_and_the_dataloaders_layout(tree, text):
    from xmc_gan import dataset as D
    from xmc_gan_amd import imagecache as IC
    data_dir, keys, out = tree
    arch = D.WordTextDataset if text == "WORD" else D.SentTextDataset
    dev = torch.device("cuda", 0)
    ds = arch(data_dir=data_dir, mode="train", transform=None, cfg=_cfg(S_LOADER))
    cache = IC.ImageCache.load(out, "train", S_LOADER, ds.filenames)
    images = [cache.image(i) for i in range(len(cache))]
    loader = IC.DeviceImageLoader(cache, ds, 4, dev, train=True, seed=3)
    assert len(loader) == len(SIZES) // 4 and loader.dataset is ds and loader.drop_last
    pil = torch.utils.data.DataLoader(arch(data_dir=data_dir, mode="train", transform=D.train_transform(S_LOADER), cfg=_cfg(S_LOADER)),
                                      batch_size=4, drop_last=True, shuffle=True, num_workers=0)
    assert len(pil) == len(loader)
    seen = []
    for epoch in (1, 2):
        batches = list(loader)
        assert len(batches) == len(loader) and loader.epoch == epoch
        for got, want in zip(batches, pil):
            _same_layout(got, want)
            assert got[0].is_cuda
        # the images: every batch against the reference with the params the loader reports, checked as it is yielded
        loader.epoch = epoch - 1                                        # (the same epoch again)
        for imgs, texts, ks in loader:
            idx, params = loader.last_params
            assert params.dtype == np.int32 and params.shape == (4, 4) and np.array_equal(params[:, 0], idx)
            assert torch.equal(imgs.cpu(), R.batch_ref(images, params, S_LOADER))
            assert ks == [keys[i] for i in idx]
            caps, lens = texts[0]
            for j, i in enumerate(idx):                                 # the caption TextDataset.__getitem__ hands out (sent_ix = 1)
                c, n = ds.get_caption(int(i) * 5 + 1)
                assert int(lens[j]) == n and (caps[j] == c if text == "SENT" else np.array_equal(caps[j].numpy(), c))
            seen.append(idx.copy())
    assert len(set(np.concatenate(seen[:2]).tolist())) == 8             # no image twice in an epoch
    assert not np.array_equal(np.concatenate(seen[:2]), np.concatenate(seen[2:]))      # another permutation in the next epoch
    again = IC.DeviceImageLoader(cache, ds, 4, dev, train=True, seed=3, start_epoch=1)  # a resumed run continues with epoch 2's draws
    next(iter(again))
    assert np.array_equal(again.last_params[0], seen[2])


def test_loader_in_evaluation_order_equals_the_test_transform(tree):
    from xmc_gan import dataset as D
    from xmc_gan_amd import imagecache as IC
    data_dir, keys, out = tree
    dev = torch.device("cuda", 0)
    ds = D.WordTextDataset(data_dir=data_dir, mode="test", transform=None, cfg=_cfg(S_LOADER))
    loader = IC.DeviceImageLoader(IC.ImageCache.load(out, "test", S_LOADER, ds.filenames), ds, 4, dev, train=False)
    pil = torch.utils.data.DataLoader(D.WordTextDataset(data_dir=data_dir, mode="test", transform=D.test_transform(S_LOADER), cfg=_cfg(S_LOADER)),
                                      batch_size=4, drop_last=True, shuffle=False, num_workers=0)
    for _ in range(2):                                                  # every pass is the same pass
        n = 0
        for got, want in zip(loader, pil):
            _same_layout(got, want)
            assert torch.equal(got[0].cpu(), want[0]) and got[2] == list(want[2])
            assert torch.equal(got[1][0][0], want[1][0][0]) and torch.equal(got[1][0][1], want[1][0][1])
            n += 1
        assert n == len(loader) == len(pil) == 2


def test_loader_refuses_a_pool_that_does_not_fit(tree):
    from xmc_gan import dataset as D
    from xmc_gan_amd import imagecache as IC
    data_dir, keys, out = tree
    ds = D.WordTextDataset(data_dir=data_dir, mode="test", transform=None, cfg=_cfg(S_LOADER))
    cache = IC.ImageCache.load(out, "test", S_LOADER, ds.filenames)
    with pytest.raises(RuntimeError, match=f"{cache.nbytes} bytes.*reserve"):
        IC.DeviceImageLoader(cache, ds, 4, torch.device("cuda", 0), train=False, reserve=1 << 50)


# ------------------------------------------------------------------------------------------------------------------------ the entry point
def _mini_yml(tmp_path, **subst):
    """df_gan_damsm.yml shrunk for a test run (thin network, tiny vocabulary, no pretrained encoder file)"""
    txt = open(os.path.join(CFG_DIR, "df_gan_damsm.yml")).read()
    rep = {"NCH: 32": "NCH: 8", "VOCA_SIZE: 27297": "VOCA_SIZE: 40", "BATCH_SIZE: 88": "BATCH_SIZE: 4", "LOG_INTERVAL: 200": "LOG_INTERVAL: 2",
           "NUM_WORKERS: 8": "NUM_WORKERS: 0", "ENCODER_DIR: data/DAMSMencoders/coco/text_encoder100.pth": "ENCODER_DIR: ''",
           "MAX_LENGTH: 20": "MAX_LENGTH: 8", "MAGP: true": "MAGP: false"}
    rep.update(subst)
    for a, b in rep.items():
        assert a in txt, a
        txt = txt.replace(a, b)
    path = tmp_path / "mini.yml"
    path.write_text(txt)
    return str(path)


def test_entry_point_trains_and_evaluates_from_the_cache(tmp_path):
    """``--image_cache`` with a DAMSM preset at 64 px, batches of 4 over 8 generated images.  The entry point writes checkpoints from epoch 51
    on (reference train_gan.py:328-334) and evaluates then, so the run is 51 epochs of two iterations: finite losses, the first batch's
    real-image grid and captions, the per-epoch sample grids, the checkpoint, and eval()'s PNGs of the generated and the cached real images."""
    import xmc_gan.train_gan as tg
    from xmc_gan_amd import imagecache as IC
    data_dir, keys = R.mini_tree(tmp_path / "coco", [(100, 90)] * 5 + [(80, 120), (76, 76), (150, 76)])
    cache_dir, run = str(tmp_path / "cache"), str(tmp_path / "run")
    for split in ("train", "test"):
        IC.build_cache(data_dir, 64, split, cache_dir, threads=2)
    last = tg.main(["--cfg", _mini_yml(tmp_path), "--data_dir", data_dir, "--image_cache", cache_dir, "--bs", "4", "--imsize", "64",
                    "--max_epoch", "51", "--output_dir", run, "--seed", "3"])
    assert {"errD", "errG"} <= set(last)
    for k, v in last.items():
        if torch.is_tensor(v) and v.numel() == 1:
            assert math.isfinite(float(v)), k
    assert last.get("hipgraph") is True                                 # the captured iteration takes the device batches as it takes any other
    assert sorted(os.listdir(os.path.join(run, "model"))) == ["netD_051.pth", "netG_051.pth", "optimizerD.pth", "optimizerG.pth"]
    img = os.path.join(run, "img")
    files = set(os.listdir(img))
    assert {"sents.txt", "imgs.png", "fake_samples_epoch_001.png", "fake_samples_epoch_051.png", "test", "org"} <= files, files
    assert len(open(os.path.join(img, "sents.txt")).read().splitlines()) == 4
    assert sorted(os.listdir(os.path.join(img, "test"))) == sorted(os.listdir(os.path.join(img, "org"))) == sorted(f"{k}.png" for k in keys)
    from PIL import Image
    # eval() was handed the cached test image: its PNG is trunc((x + 1) * 127.5) of the normalised bytes
    from xmc_gan.dataset import to_normalized_tensor
    from xmc_gan.utils.visual import to_uint8_hwc
    want = to_uint8_hwc(to_normalized_tensor(IC.ImageCache.load(cache_dir, "test", 64, keys).image(5)))
    assert np.array_equal(np.array(Image.open(os.path.join(img, "org", f"{keys[5]}.png"))), want)


def test_entry_point_names_the_build_command_when_the_cache_is_missing(tmp_path, capsys):
    import xmc_gan.train_gan as tg
    data_dir, keys = R.mini_tree(tmp_path / "coco", [(100, 90)] * 4)
    with pytest.raises(SystemExit) as e:
        tg.main(["--cfg", _mini_yml(tmp_path), "--data_dir", data_dir, "--image_cache", str(tmp_path / "nothing"), "--bs", "4", "--imsize", "64",
                 "--max_epoch", "1", "--output_dir", str(tmp_path / "run")])
    msg = str(e.value)
    assert "python xmc_gan/image_cache.py build" in msg and f"--data_dir {data_dir}" in msg and "--imsize 64" in msg and "--split train" in msg
    # a cache of another size is refused the same way
    from xmc_gan_amd import imagecache as IC
    IC.build_cache(data_dir, 32, "train", str(tmp_path / "c32"), threads=1)
    with pytest.raises(SystemExit, match="image_cache.py build"):
        tg.main(["--cfg", _mini_yml(tmp_path), "--data_dir", data_dir, "--image_cache", str(tmp_path / "c32"), "--bs", "4", "--imsize", "64",
                 "--max_epoch", "1", "--output_dir", str(tmp_path / "run")])
