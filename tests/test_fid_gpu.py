"""The FID evaluation on the GPU (xmc_gan_amd/fid.py, csrc/fid.hip) against the plain-torch f64 restatement in tests/fid_ref.py.

The error figure is the project's: max |got - want| over the rms of `want`.  Every bar is 1.5 x the figure measured on the MI355X, which
is written beside it; in f32 anything above 1e-3 would be a bug, not rounding.  The shapes are the smallest that still reach what can go
wrong: odd maps, M = N * OH * OW that is no multiple of a tile (N = 3), each tile the dispatcher can pick for f32 operands, two tap ranges."""
import copy
import logging
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fid_ref
from xmc_gan_amd import fid as FID
from xmc_gan_amd import lib as L
from xmc_gan_amd import ops

DEV = torch.device("cuda", 0)


def _err(got, want):
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double()
    assert got.shape == want.shape, (got.shape, want.shape)
    return float((got - want).abs().max() / want.pow(2).mean().sqrt())


def _nhwc(x_nchw, pad_to=None):
    """f64 NCHW (host) -> f32 NHWC on the device, channels zero-padded to `pad_to`"""
    x = x_nchw.permute(0, 2, 3, 1).float()
    if pad_to is not None and x.shape[-1] < pad_to:
        x = F.pad(x, (0, pad_to - x.shape[-1]))
    return x.contiguous().to(DEV)


def _nchw(y_nhwc, c=None):
    y = y_nhwc.cpu().permute(0, 3, 1, 2)
    return y if c is None else y[:, :c]


@pytest.fixture(scope="module")
def net(tmp_path_factory):
    """(the restatement, the native extractor without a resize, the random weights file) from one random state dict"""
    sd = fid_ref.random_state_dict(7)
    path = str(tmp_path_factory.mktemp("fid") / "inception_random.pth")
    torch.save(sd, path)
    return fid_ref.Reference(sd), FID.InceptionFID(path, DEV, resize_to=None), path


# ------------------------------------------------------------------------------------------ front end
@pytest.mark.parametrize("h,w,measured", [(64, 64, 7.194e-07), (256, 256, 7.019e-07), (300, 400, 7.508e-07)])
def test_resize_u8(h, w, measured):
    u8 = torch.randint(0, 256, (3, h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(h))
    got = ops.fid_resize_u8(u8.to(DEV), (299, 299))
    assert tuple(got.shape) == (3, 299, 299, 8) and got.dtype == torch.float32
    assert not got[..., 3:].any()
    e = _err(_nchw(got, 3), fid_ref.Reference.front_end(u8, 299))
    print(f"resize {h}x{w} -> 299: {e:.3e}")
    assert e <= 1.5 * measured


def test_resize_u8_same_size_is_exact():
    u8 = torch.arange(256, dtype=torch.uint8).repeat(3 * 299 * 299 * 3 // 256 + 1)[:3 * 299 * 299 * 3].reshape(3, 299, 299, 3)
    got = ops.fid_resize_u8(u8.to(DEV), (299, 299)).cpu()
    assert torch.equal(got[..., :3], 2.0 * (u8.float() / 255.0) - 1.0) and not got[..., 3:].any()
    odd = torch.randint(0, 256, (2, 5, 7, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    assert torch.equal(ops.fid_resize_u8(odd.to(DEV)).cpu()[..., :3], 2.0 * (odd.float() / 255.0) - 1.0)
    with pytest.raises(ValueError):
        ops.fid_resize_u8(torch.zeros((1, 4, 4, 4), dtype=torch.uint8, device=DEV))


# ------------------------------------------------------------------------------------------ pools
# measured, by (stride, map, channels); 1x1 maps: one pixel divided by 1, exact
POOL_AVG_MEASURED = {(1, 7, 7, 8): 4.229e-07, (1, 7, 7, 288): 4.944e-07, (1, 6, 6, 8): 2.462e-07, (1, 6, 6, 288): 4.376e-07,
                     (1, 3, 5, 8): 2.572e-07, (1, 3, 5, 288): 4.218e-07, (1, 1, 1, 8): 0.0, (1, 1, 1, 288): 0.0,
                     (2, 7, 7, 8): 3.459e-07, (2, 7, 7, 288): 4.275e-07, (2, 6, 6, 8): 1.540e-07, (2, 6, 6, 288): 3.723e-07,
                     (2, 3, 5, 8): 1.860e-07, (2, 3, 5, 288): 3.817e-07}


@pytest.mark.parametrize("c", [8, 288])
@pytest.mark.parametrize("h,w", [(7, 7), (6, 6), (3, 5), (1, 1)])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("mode", ["max", "avg"])
def test_pool3x3(mode, stride, h, w, c):
    x = torch.randn(3, c, h, w, generator=torch.Generator().manual_seed(h * 10 + w)).double()
    xd = _nhwc(x)
    if stride == 2 and (h < 3 or w < 3):                    # no whole window: torch refuses it too
        with pytest.raises(ValueError):
            ops.pool3x3(xd, mode, stride)
        return
    pad = 1 if stride == 1 else 0
    want = F.max_pool2d(x, 3, stride, pad) if mode == "max" else F.avg_pool2d(x, 3, stride, pad, count_include_pad=False)
    got = _nchw(ops.pool3x3(xd, mode, stride))
    if mode == "max":
        assert torch.equal(got, want.float())
    else:
        e = _err(got, want)
        print(f"pool avg s{stride} {h}x{w} C{c}: {e:.3e}")
        assert e <= 1.5 * POOL_AVG_MEASURED[(stride, h, w, c)]
        # corners divide by 4 (stride 1), edges by 6: a map of ones stays a map of ones
        ones = ops.pool3x3(torch.ones_like(xd), "avg", stride)
        assert torch.equal(ones, torch.ones_like(ones))


def test_pool3x3_refuses_bad_arguments():
    x = torch.zeros((1, 5, 5, 8), dtype=torch.float32, device=DEV)
    for bad in (lambda: ops.pool3x3(x, "sum", 1), lambda: ops.pool3x3(x, "max", 3), lambda: ops.pool3x3(x[..., :6].contiguous(), "max", 1),
                lambda: ops.pool3x3(x.bfloat16(), "max", 1)):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------ single convolutions
# (cin, cout, kernel, stride, padding, map, N, measured figure): the four rectangular kernels; the stem's stride-2 layer on its 8-channel
# source; a 25-tap kernel (two tap ranges); an 80-channel source (20 sixteen-byte units per tap: no power of two).  Those have
# M = N * OH * OW <= 1024 and run on the 128x32 tile; the last two have M > 1024 and reach the 128x128 and 128x64 tiles.
CONVS = [(128, 128, (1, 7), 1, (0, 3), (9, 9), 3, 5.323e-06), (160, 192, (7, 1), 1, (3, 0), (9, 9), 3, 8.109e-06),
         (384, 384, (1, 3), 1, (0, 1), (5, 5), 3, 9.818e-06), (384, 384, (3, 1), 1, (1, 0), (5, 5), 3, 8.058e-06),
         (3, 32, 3, 2, 0, (15, 15), 3, 9.663e-07), (48, 64, 5, 1, 2, (9, 9), 3, 4.141e-06), (80, 192, 3, 1, 0, (11, 11), 3, 5.306e-06),
         (128, 128, (1, 7), 1, (0, 3), (17, 17), 4, 7.180e-06), (32, 64, 3, 1, 1, (21, 19), 3, 3.717e-06)]


@pytest.mark.parametrize("cin,cout,k,s,p,hw,n,measured", CONVS)
def test_single_convolution(cin, cout, k, s, p, hw, n, measured):
    g = torch.Generator().manual_seed(cin + cout)
    kh, kw = fid_ref._pair(k)
    x = torch.randn(n, cin, *hw, generator=g).double()
    w = (torch.randn(cout, cin, kh, kw, generator=g) * (2.0 / (cin * kh * kw)) ** 0.5)
    b = 0.1 * torch.randn(cout, generator=g)
    want = F.relu(F.conv2d(x, w.double(), b.double(), stride=s, padding=fid_ref._pair(p)))
    geom = ops.ConvGeom(cin, cout, k, s, p)
    got = FID.conv_bias_relu(_nhwc(x, 8), w.to(DEV), b.to(DEV), geom)
    assert tuple(got.shape[1:3]) == tuple(want.shape[2:]) == geom.out_hw(*hw)
    e = _err(_nchw(got), want)
    print(f"conv {cin}->{cout} k{k} s{s} p{p} on {hw} N{n}: {e:.3e} [{L.load().xmc_last_kernel().decode()}]")
    assert e <= 1.5 * measured


def test_square_geometry_is_unchanged():
    """the generalised ConvGeom describes every square layer as before"""
    g = ops.ConvGeom(64, 32, 4, 2, 1)
    assert (g.k, g.s, g.p, g.kh, g.kw, g.ph, g.pw, g.ntaps) == (4, 2, 1, 4, 4, 1, 1, 16) and g.out_hw(16, 16) == (8, 8)
    assert g.taps() == [(i - 1, j - 1, i * 4 + j) for i in range(4) for j in range(4)]
    r = ops.ConvGeom(8, 8, (1, 7), 1, (0, 3))
    assert r.k is None and r.p is None and r.out_hw(9, 11) == (9, 11) and r.taps()[0] == (0, -3, 0) and r.taps()[6] == (0, 3, 6)


# ------------------------------------------------------------------------------------------ moments
@pytest.mark.parametrize("d", [64, 2048])
def test_moments(d):
    """Mean 50, spread 0.5: sum x x^T is 13 * 2500 per entry, the covariance 0.25 -- an f32 accumulator (2^-24 * 3e4 = 2e-3 per entry) loses
    it entirely.  In f64 the sums carry 13 roundings of 1.1e-16 * 3.3e4 = 3.6e-12 each, and the subtraction passes them on divided by 12:
    below 1e-11 absolute, against np.cov's own 1e-16.  The bar is 1e-9."""
    g = torch.Generator().manual_seed(d)
    x = (50.0 + 0.5 * torch.randn(13, d, generator=g)).float()
    runs = []
    for _ in range(2):
        st = FID.FeatureStats(d, DEV)
        for lo, hi in ((0, 5), (5, 6), (6, 13)):
            st.update(x[lo:hi].to(DEV))
        assert st.n == 13
        runs.append((st.total.clone(), st.outer.clone(), st.finalize()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    mu, sigma = runs[0][2]
    xn = x.double().numpy()
    emu, esig = np.abs(mu - xn.mean(0)).max(), np.abs(sigma - np.cov(xn, rowvar=False)).max()
    print(f"moments D={d}: mean off by {emu:.3e}, covariance by {esig:.3e}")
    assert emu <= 1e-12 and esig <= 1e-9
    with pytest.raises(ValueError):
        ops.fid_moments(x.to(DEV), st.total.float(), st.outer)


# ------------------------------------------------------------------------------------------ blocks and the whole network
@pytest.mark.parametrize("name,hw,measured", [("Mixed_5b", 5, 3.211e-06), ("Mixed_6a", 9, 7.680e-06), ("Mixed_6b", 5, 6.090e-06),
                                              ("Mixed_7a", 9, 4.002e-06), ("Mixed_7b", 5, 6.736e-06), ("Mixed_7c", 5, 1.081e-05)])
def test_block(net, name, hw, measured):
    ref, ex, _ = net
    x = torch.randn(2, FID.BLOCK_IN[name], hw, hw, generator=torch.Generator().manual_seed(hw)).abs().double()
    want = ref.block(name, x)
    got = ex.block(name, _nhwc(x))
    e = _err(_nchw(got), want)
    print(f"{name} on {hw}x{hw}: {e:.3e}")
    assert e <= 1.5 * measured


def test_network_without_resize(net):
    ref, ex, _ = net
    u8 = torch.randint(0, 256, (5, 75, 75, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(75))
    want = ref.features(u8, None)
    got = ex(u8)
    assert tuple(got.shape) == (5, 2048) and got.dtype == torch.float32
    e = _err(got, want)
    print(f"network 75x75 N5: {e:.3e} (feature rms {float(want.pow(2).mean().sqrt()):.3f})")
    assert e <= 1.5 * 9.290e-06                 # measured: 9.290e-06
    with pytest.raises(ValueError):
        ex(u8[:, :70])


def test_network_with_resize(net):
    ref, ex, _ = net
    ex299 = copy.copy(ex)
    ex299.resize_to = 299
    u8 = torch.randint(0, 256, (2, 64, 64, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(64))
    e = _err(ex299(u8), ref.features(u8, 299))
    print(f"network 64x64 -> 299 N2: {e:.3e}")
    assert e <= 1.5 * 2.791e-06                 # measured: 2.791e-06


def test_network_ignores_the_precision_mode(net):
    _, ex, _ = net
    u8 = torch.randint(0, 256, (2, 75, 75, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    try:
        a = ex(u8)
        ops.set_precision("f16")
        b = ex(u8)
        ops.set_precision("fp32")
        c = ex(u8)
    finally:
        ops.set_precision("bf16")
    assert torch.equal(a, b) and torch.equal(a, c)


def test_fid_end_to_end(net):
    ref, ex, _ = net
    g = torch.Generator().manual_seed(16)
    a = torch.randint(0, 256, (16, 75, 75, 3), dtype=torch.uint8, generator=g)
    b = (torch.rand(16, 75, 75, 3, generator=g) ** 2 * 200 + 20).to(torch.uint8)          # darker, narrower
    got = FID.fid_from_images(a, b, ex, batch=7)                                          # batches of 7 + 7 + 2
    stats = []
    for im in (a, b):
        f = ref.features(im, None).numpy()
        stats.append((f.mean(0), np.cov(f, rowvar=False)))
    want = FID.frechet_distance(*stats[0], *stats[1])
    rel = abs(got - want) / want
    print(f"FID of 16 + 16 images: {got:.6f} vs {want:.6f}, relative error {rel:.3e}")
    assert want > 0 and rel <= 1.5 * 2.342e-07          # measured: 2.342e-07 (1.936603 against 1.936602)


def test_stats_of_dir_mixed_sizes(net, tmp_path):
    from PIL import Image
    _, ex, _ = net
    g = torch.Generator().manual_seed(5)
    ims = [torch.randint(0, 256, (75 + 4 * (i % 2), 75, 3), dtype=torch.uint8, generator=g) for i in range(5)]
    for i, im in enumerate(ims):
        Image.fromarray(im.numpy()).save(str(tmp_path / f"{i}.png"))
    (tmp_path / "notes.txt").write_text("not an image")
    st = FID.stats_of_dir(str(tmp_path), ex, batch=4)
    assert st.n == 5
    feats = torch.cat([ex(im[None]) for im in ims]).double().cpu().numpy()
    mu, sigma = st.finalize()
    assert np.abs(mu - feats.mean(0)).max() <= 1e-12 * max(1.0, np.abs(feats).max())
    assert np.abs(sigma - np.cov(feats, rowvar=False)).max() <= 1e-9 * max(1.0, np.abs(feats).max() ** 2)
    os.makedirs(str(tmp_path / "empty"))
    with pytest.raises(ValueError):
        FID.stats_of_dir(str(tmp_path / "empty"), ex)


# ------------------------------------------------------------------------------------------ the trainer's evaluation
def test_eval_scores_with_the_native_path(net, tmp_path):
    import xmc_gan.train_gan as tg
    from test_sample_gpu import _use_cfg, _yml
    from xmc_gan.config import gan
    _, _, weights = net
    try:
        cfg = _use_cfg(_yml(tmp_path))
        torch.manual_seed(2)
        netG, _, _, _ = tg.build_models(DEV)
        enc = tg.SyntheticTextEncoder(cfg.TEXT.EMBEDDING_DIM, cfg.TEXT.MAX_LENGTH, 1, DEV)
        loader = tg.SyntheticCOCO(2, 4, cfg.IMG.SIZE, cfg.TEXT.MAX_LENGTH, 1, cfg.TEXT.VOCA_SIZE)
        lines = []
        logger = logging.getLogger("fid-eval-test")
        logger.setLevel(logging.INFO)
        handler = logging.Handler()
        handler.emit = lambda rec: lines.append(rec.getMessage())
        logger.addHandler(handler)
        rows = []
        writer = type("W", (), {"add_scalar": lambda self, tag, v, step: rows.append((tag, v, step))})()
        img = tmp_path / "img"
        kw = dict(loader=loader, state_epoch=7, text_encoder=enc, netG=netG, logger=logger, num_samples=8, save_dir=str(img / "test"),
                  org_dir=str(img / "org"), writer=writer, fid_inception=weights)
        _, fid = tg.eval(**kw)
        assert fid is not None and np.isfinite(fid) and fid > 0
        assert lines[-1] == f" epoch 7, FID : {fid}" and rows == [("FID", fid, 7)]
        cache = img / "org_stats.npz"
        assert cache.is_file() and FID.load_stats(str(cache), with_count=True)[2] == 8
        assert len(os.listdir(img / "org")) == 8 and len(os.listdir(img / "test")) == 8
        # the real images' statistics are what the PNGs in org/ give
        mu, sigma = FID.load_stats(str(cache))
        from xmc_gan.utils.visual import fid_between, fid_extractor
        mu_d, sigma_d = FID.stats_of_dir(str(img / "org"), fid_extractor(weights, DEV)).finalize()
        assert np.abs(mu - mu_d).max() <= 1e-5 * np.abs(mu_d).max()
        # and the two directories score the same through `fid_between` with the weights given
        between = fid_between(str(img / "org"), str(img / "test"), DEV, weights=weights)
        assert abs(between - fid) <= 1e-4 * fid
        # a second call reuses the cache: the file is not written again
        before = os.stat(cache).st_mtime_ns
        called = []
        real_update = FID.FeatureStats.update
        try:
            FID.FeatureStats.update = lambda self, f: (called.append(1), real_update(self, f))[1]
            _, fid2 = tg.eval(**kw)
        finally:
            FID.FeatureStats.update = real_update
        assert os.stat(cache).st_mtime_ns == before and len(called) == 2          # (the two generated batches only)
        assert np.isfinite(fid2) and lines[-1] == f" epoch 7, FID : {fid2}"
    finally:
        gan.reset_cfg()
        ops.set_precision("bf16")


def test_sample_scores_what_it_sampled(net, tmp_path):
    import xmc_gan.sample as sample
    import xmc_gan.train_gan as tg
    from test_sample_gpu import _use_cfg, _yml
    from xmc_gan.config import gan
    from xmc_gan.utils.visual import fid_between
    _, _, weights = net
    try:
        yml = _yml(tmp_path)
        _use_cfg(yml)
        torch.manual_seed(4)
        torch.save(tg.build_models(DEV)[0].state_dict(), tmp_path / "netG.pth")
        gan.reset_cfg()
        against = tmp_path / "against.npz"
        g = np.random.default_rng(0)
        feats = np.abs(g.standard_normal((12, 2048)))
        FID.save_stats(str(against), feats.mean(0), np.cov(feats, rowvar=False))
        base = ["--cfg", yml, "--checkpoint", str(tmp_path / "netG.pth"), "--out", str(tmp_path / "out"), "--synthetic", "5", "--grid_max", "0"]
        with pytest.raises(SystemExit, match="fid_inception"):
            sample.main(base + ["--fid_against", str(against), "--fid_inception", str(tmp_path / "nope.pth")])
        with pytest.raises(SystemExit, match="fid_against"):
            sample.main(base + ["--fid_against", str(tmp_path / "nowhere"), "--fid_inception", weights])
        man = sample.main(base + ["--fid_against", str(against), "--fid_inception", weights])
        assert np.isfinite(man["fid"]) and man["fid"] > 0
        # the same number from the PNGs it wrote (batches of 4 + 1 there, one of 5 here: equal up to the f32 tiles' row grouping)
        again = fid_between(str(against), str(tmp_path / "out"), DEV, weights=weights)
        assert abs(again - man["fid"]) <= 1e-4 * man["fid"]
        assert sample.main(base[:-4] + ["--synthetic", "2", "--grid_max", "0"])["fid"] is None
    finally:
        gan.reset_cfg()
        ops.set_precision("bf16")
