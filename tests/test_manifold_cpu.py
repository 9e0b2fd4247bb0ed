"""Precision / recall / density / coverage without a GPU: the f64 reference on a hand-worked example, the host arithmetic of
xmc_gan_amd/manifold.py, the feature files, the argument checks of the three entry points (they happen before any launch) and the
refusals of the command lines."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import manifold_ref as REF
from xmc_gan_amd import manifold as MF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_on_a_hand_worked_line():
    """1-D points (D = 4, the other columns zero), k = 2, with a duplicate and ties.
    R = 0, 0, 1, 3, 6:  distances^2 from each point to the others, sorted:
        0 -> 0 (the duplicate, kept: excluded by index only), 1, 9, 36      rad2 = 1
        0 -> 0, 1, 9, 36                                                    rad2 = 1
        1 -> 1, 1, 4, 25                                                    rad2 = 1   (a tie at the radius)
        3 -> 4, 9, 9, 9                                                     rad2 = 9
        6 -> 9, 25, 36, 36                                                  rad2 = 25
    G = 1, 2, 10:  1 -> 1, 81: rad2 = 81;  2 -> 1, 64: rad2 = 64;  10 -> 64, 81: rad2 = 81
    cnt_G: G=1 lies in the balls of 0, 0 (1 <= 1), 1 (0), 3 (4 <= 9), 6 (25 <= 25: on the boundary)  -> 5
           G=2: 0: 4 > 1, 0: no, 1: 1 <= 1 yes, 3: 1 <= 9 yes, 6: 16 <= 25 yes                        -> 3
           G=10: 100, 100, 81, 49, 16 <= 25 yes                                                       -> 1
    cnt_R: every real point is within 81 of G=1 and 64 of G=2; of G=10 (rad2 81): 6 (16), 3 (49), 1 (81: boundary)
           0 -> 2, 0 -> 2, 1 -> 3, 3 -> 3, 6 -> 3
    near2_R: 0 -> 1, 0 -> 1, 1 -> 0, 3 -> 1, 6 -> 16;  coverage: 1<=1, 1<=1, 0<=1, 1<=9, 16<=25: all five."""
    def line(v):
        x = np.zeros((len(v), 4), np.float32)
        x[:, 1] = v
        return x
    R, G = line([0, 0, 1, 3, 6]), line([1, 2, 10])
    assert REF.knn_radius2(R, 2).tolist() == [1, 1, 1, 9, 25]
    assert REF.knn_radius2(G, 2).tolist() == [81, 64, 81]
    o = REF.reference(R, G, 2)
    assert o["cnt_g"].tolist() == [5, 3, 1] and o["cnt_r"].tolist() == [2, 2, 3, 3, 3]
    assert o["near2_r"].tolist() == [1, 1, 0, 1, 16] and o["cov"].all()
    assert (o["precision"], o["recall"], o["coverage"]) == (1.0, 1.0, 1.0) and o["density"] == 9 / (2 * 3)
    # decisions exactly on a boundary are what the band marks: G=1 against the ball of 6, real 1 against the ball of G=10
    assert o["cnt_g_lo"].tolist() == [2, 2, 1] and o["cnt_g_hi"].tolist() == [5, 3, 1]
    assert o["ambiguous_g"].tolist() == [True, True, False]
    # k = 1 sees the duplicate as the nearest neighbour: radius 0
    assert REF.knn_radius2(R, 1).tolist() == [0, 0, 1, 4, 9]
    with pytest.raises(AssertionError):
        REF.knn_radius2(G, 3)


def test_prdc_from_counts():
    r = MF.prdc_from_counts([5, 3, 1, 0], [2, 0, 3, 3, 3], [1, 1, 0, 1, 26], [1, 1, 1, 9, 25], 2)
    assert r == dict(precision=0.75, recall=0.8, density=9 / 8, coverage=0.8, k=2, n_real=5, n_fake=4)
    R, G = REF.gaussian(40, 30, 8, 3)
    o = REF.reference(R, G, 3)
    r = MF.prdc_from_counts(o["cnt_g"], o["cnt_r"], o["near2_r"], o["rad2_r"], 3)
    for name in ("precision", "recall", "density", "coverage", "k", "n_real", "n_fake"):
        assert r[name] == o[name], name
    with pytest.raises(ValueError):
        MF.prdc_from_counts([1], [1, 2], [0.0], [1.0], 1)
    with pytest.raises(ValueError):
        MF.prdc_from_counts([1], [1], [0.0], [1.0], 0)


def test_feature_bank_files(tmp_path):
    g = np.random.default_rng(1)
    bank = MF.FeatureBank(8, "cpu")
    assert tuple(bank.rows().shape) == (0, 8)
    parts = [g.standard_normal((n, 8)).astype(np.float32) for n in (3, 300, 1, 700)]        # grows past 256 and past a doubling
    for p in parts:
        bank.update(torch.from_numpy(p))
    want = np.concatenate(parts)
    assert bank.n == 1004 and np.array_equal(bank.rows().numpy(), want)
    path = str(tmp_path / "feats.npz")
    bank.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == ["features", "n"] and int(z["n"]) == 1004 and z["features"].dtype == np.float32
    again = MF.FeatureBank.load(path, "cpu")
    assert again.n == 1004 and again.dims == 8 and np.array_equal(again.rows().numpy(), want)
    with pytest.raises(ValueError, match="rows"):
        bank.update(torch.zeros(2, 9))
    # a statistics file of FID holds only moments
    from xmc_gan_amd import fid as FID
    stats = str(tmp_path / "stats.npz")
    FID.save_stats(stats, want.mean(0), np.cov(want, rowvar=False), 1004)
    with pytest.raises(ValueError, match="only moments"):
        MF.FeatureBank.load(stats, "cpu")
    other = str(tmp_path / "other.npz")
    np.savez(other, x=np.zeros(3))
    with pytest.raises(ValueError, match="features"):
        MF.load_features(other)
    # the kernels are GPU only
    with pytest.raises(RuntimeError, match="GPU only"):
        MF.prdc(bank, again, 3)


def test_entry_points_check_their_arguments():
    """all refusals come before any launch, so they need no GPU; the pointers are host memory that is never read"""
    from xmc_gan_amd import lib as L
    lib = L.load()
    EINVAL, EALIGN, ESHAPE = -1, -2, -3
    buf = ctypes.create_string_buffer(4096 + 64)
    base = (ctypes.addressof(buf) + 63) & ~63
    p, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)
    # slices: clamped to the 128-row chunks of the candidates and to 64; 0 chooses
    assert lib.xmc_manifold_slices(300, 257, 1) == 1 and lib.xmc_manifold_slices(300, 257, 2) == 2
    assert lib.xmc_manifold_slices(300, 257, 5) == 3 and lib.xmc_manifold_slices(300, 257, 0) == 3
    assert lib.xmc_manifold_slices(6000, 6000, 0) == 10 and lib.xmc_manifold_slices(30000, 30000, 0) == 2          # 512 // 47, 512 // 235
    assert lib.xmc_manifold_slices(100000, 100000, 0) == 1
    assert lib.xmc_manifold_slices(100000, 100000, 1000) == 64 and lib.xmc_manifold_slices(0, 5, 0) == 0
    # row_sqnorm
    assert lib.xmc_row_sqnorm(None, p, 4, 8, None) == EINVAL and lib.xmc_row_sqnorm(p, None, 4, 8, None) == EINVAL
    assert lib.xmc_row_sqnorm(p, p, 0, 8, None) == EINVAL
    for d in (0, 2, 6, 4100):
        assert lib.xmc_row_sqnorm(p, p, 4, d, None) == ESHAPE, d
    assert lib.xmc_row_sqnorm(odd, p, 4, 8, None) == EALIGN and lib.xmc_row_sqnorm(p, odd, 4, 8, None) == EALIGN
    # knn_radius2(x, n2, r2, ws, ws_bytes, N, D, k, slices, stream)
    ok = dict(x=p, n2=p, r2=p, ws=None, ws_bytes=0, N=300, D=8, k=3, slices=1)

    def knn(**kw):
        a = dict(ok, **kw)
        return lib.xmc_knn_radius2(a["x"], a["n2"], a["r2"], a["ws"], a["ws_bytes"], a["N"], a["D"], a["k"], a["slices"], None)
    for name in ("x", "n2", "r2"):
        assert knn(**{name: None}) == EINVAL, name
        assert knn(**{name: odd}) == EALIGN, name
    assert knn(k=0) == EINVAL and knn(k=17) == EINVAL and knn(slices=-1) == EINVAL and knn(N=0) == EINVAL
    assert knn(N=3) == ESHAPE and knn(N=16, k=16) == ESHAPE          # N >= k + 1
    assert knn(D=6) == ESHAPE and knn(D=4100) == ESHAPE and knn(D=0) == ESHAPE
    assert knn(slices=2) == EINVAL                                    # two slices need scratch
    assert knn(slices=2, ws=p, ws_bytes=2 * 300 * 3 * 4 - 1) == EINVAL
    assert knn(slices=2, ws=odd, ws_bytes=1 << 20) == EALIGN
    # manifold_count(a, na2, b, nb2, rb2, count, near2, ws, ws_bytes, Na, Nb, D, slices, stream)
    okc = dict(a=p, na2=p, b=p, nb2=p, rb2=p, count=p, near2=p, ws=None, ws_bytes=0, Na=300, Nb=257, D=8, slices=1)

    def cnt(**kw):
        a = dict(okc, **kw)
        return lib.xmc_manifold_count(a["a"], a["na2"], a["b"], a["nb2"], a["rb2"], a["count"], a["near2"], a["ws"], a["ws_bytes"], a["Na"],
                                      a["Nb"], a["D"], a["slices"], None)
    for name in ("a", "na2", "b", "nb2"):
        assert cnt(**{name: None}) == EINVAL, name
        assert cnt(**{name: odd}) == EALIGN, name
    assert cnt(rb2=None, near2=None) == EINVAL                        # nothing to write
    assert cnt(count=None) == EINVAL                                  # radii without a place for the counts
    assert cnt(rb2=odd) == EALIGN and cnt(near2=odd) == EALIGN and cnt(count=ctypes.c_void_p(base + 2)) == EALIGN
    assert cnt(Na=0) == EINVAL and cnt(Nb=0) == EINVAL and cnt(slices=-1) == EINVAL
    assert cnt(D=6) == ESHAPE and cnt(D=4100) == ESHAPE
    assert cnt(slices=2) == EINVAL and cnt(slices=2, ws=p, ws_bytes=2 * 300 * 8 - 1) == EINVAL
    # the wrappers refuse host tensors
    from xmc_gan_amd import ops
    x = torch.zeros(8, 8)
    for call in (lambda: ops.row_sqnorm(x), lambda: ops.knn_radius2(x, 3), lambda: ops.manifold_count(x, x, None)):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()


def test_command_lines_refuse(tmp_path, monkeypatch):
    import xmc_gan.prdc as cli
    import xmc_gan.sample as sample
    import xmc_gan.train_gan as tg
    from PIL import Image
    from test_sample_cpu import _yml
    from xmc_gan.config import gan
    from xmc_gan_amd import fid as FID
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.delenv("XMC_FID_INCEPTION", raising=False)
    # defaults: everything off
    a = sample.parse_args(["--cfg", "c.yml", "--checkpoint", "g.pth", "--out", "o"])
    assert (a.prdc_against, a.prdc_k) == ("", 5)
    assert tg.parse_args(["--cfg", "c.yml"]).prdc == 0
    c = cli.parse_args(["a", "b"])
    assert (c.k, c.batch, c.inception, c.save_features) == (5, 100, "", "")
    few, full = tmp_path / "few", tmp_path / "full"
    few.mkdir(), full.mkdir()
    for i in range(7):
        Image.fromarray(np.full((8, 8, 3), 30 * i, np.uint8)).save(str(full / f"{i}.png"))
        if i < 3:
            Image.fromarray(np.full((8, 8, 3), 30 * i, np.uint8)).save(str(few / f"{i}.png"))
    g = np.random.default_rng(0)
    feats = str(tmp_path / "feats.npz")
    MF.save_features(feats, g.standard_normal((9, 2048)))
    small = str(tmp_path / "small.npz")
    MF.save_features(small, g.standard_normal((4, 2048)))
    stats = str(tmp_path / "stats.npz")
    FID.save_stats(stats, np.zeros(8), np.eye(8))
    weights = tmp_path / "w.pth"
    weights.write_bytes(b"")
    for argv, word in (([str(few), str(full), "--inception", str(weights)], "fewer than k + 1"),
                       ([small, feats], "fewer than k + 1"),
                       ([str(full), str(tmp_path / "missing"), "--inception", str(weights)], "neither"),
                       ([str(full), feats], "--inception"),
                       ([str(full), feats, "--inception", str(tmp_path / "nope.pth")], "not a file"),
                       ([feats, stats], "only moments"),
                       ([feats, feats, "--k", "0"], "--k"),
                       ([feats, feats, "--k", "17"], "--k"),
                       ([feats, feats, "--batch", "0"], "--batch")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code not in (0, None) and word in str(e.value.code) and "\n" not in str(e.value.code), (argv, e.value.code)
    with pytest.raises(RuntimeError, match="MI355X"):
        cli.main([feats, feats])
    ckpt = tmp_path / "netG.pth"
    ckpt.write_bytes(b"")
    base = ["--checkpoint", str(ckpt), "--out", str(tmp_path / "out"), "--synthetic", "2"]
    try:
        yml = _yml(tmp_path)
        with pytest.raises(SystemExit, match="fid_inception"):
            sample.main(["--cfg", yml, "--prdc_against", feats] + base)
        with pytest.raises(SystemExit, match="fid_inception"):
            sample.main(["--cfg", yml, "--prdc_against", feats, "--fid_inception", str(tmp_path / "nope.pth")] + base)
        with pytest.raises(SystemExit, match="prdc_against"):
            sample.main(["--cfg", yml, "--prdc_against", str(tmp_path / "nowhere"), "--fid_inception", str(weights)] + base)
        with pytest.raises(SystemExit, match="prdc_k"):
            sample.main(["--cfg", yml, "--prdc_against", feats, "--fid_inception", str(weights), "--prdc_k", "17"] + base)
        gan.reset_cfg()
        with pytest.raises(SystemExit, match="--prdc"):
            tg.main(["--cfg", yml, "--synthetic", "1", "--prdc", "17"])
        gan.reset_cfg()
        with pytest.raises(SystemExit, match="--prdc"):
            tg.main(["--cfg", yml, "--synthetic", "1", "--prdc", "-1"])
    finally:
        gan.reset_cfg()
