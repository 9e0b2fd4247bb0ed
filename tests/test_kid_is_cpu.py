"""KID and the Inception Score without a device: the subset draw, the split boundaries, the f64 reference of tests/kid_ref.py against
loops and closed forms, `MetricSuite` on the host with a stand-in extractor, and what the command lines refuse before a device is touched."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kid_ref as REF
from xmc_gan_amd import evaluate as EV
from xmc_gan_amd import fid as FID
from xmc_gan_amd import manifold as MF


# ------------------------------------------------------------------------------------------ the subset draw
def test_kid_subsets():
    ir, jf = MF.kid_subsets(50, 40, 7, 16, seed=3)
    assert ir.shape == jf.shape == (7, 16) and ir.dtype == jf.dtype == np.int32
    for tab, n in ((ir, 50), (jf, 40)):
        assert tab.min() >= 0 and tab.max() < n and all(len(set(row)) == 16 for row in tab.tolist())
    again = MF.kid_subsets(50, 40, 7, 16, seed=3)
    assert np.array_equal(again[0], ir) and np.array_equal(again[1], jf)
    other = MF.kid_subsets(50, 40, 7, 16, seed=4)
    assert not np.array_equal(other[0], ir)
    # the rule, restated: one generator, per subset the real indices first
    rng = np.random.default_rng([3, 0x4B4944])
    for s in range(7):
        assert np.array_equal(ir[s], rng.choice(50, 16, replace=False)) and np.array_equal(jf[s], rng.choice(40, 16, replace=False))
    want = REF.subsets(50, 40, 7, 16, 3)
    assert np.array_equal(want[0], ir) and np.array_equal(want[1], jf)
    # m = min(size, n_real, n_fake)
    assert MF.kid_subsets(50, 9, 2, 16)[0].shape == (2, 9) and MF.kid_subsets(5, 40, 2, 16)[1].shape == (2, 5)
    assert MF.kid_subsets(6000, 6000)[0].shape == (100, 1000)
    assert sorted(MF.kid_subsets(4, 9, 1, 1000)[0][0].tolist()) == [0, 1, 2, 3]
    for args in ((1, 40, 3, 16), (50, 1, 3, 16), (50, 40, 3, 1), (0, 0, 3, 16)):
        with pytest.raises(ValueError, match="two rows"):
            MF.kid_subsets(*args)
    with pytest.raises(ValueError, match="subsets"):
        MF.kid_subsets(50, 40, 0, 16)


def test_is_split_bounds():
    b = FID.is_split_bounds(23, 10)
    assert b == [(0, 2), (2, 4), (4, 6), (6, 9), (9, 11), (11, 13), (13, 16), (16, 18), (18, 20), (20, 23)]
    assert b == [(s * 23 // 10, (s + 1) * 23 // 10) for s in range(10)] == REF.split_bounds(23, 10)
    assert FID.is_split_bounds(10, 10) == [(i, i + 1) for i in range(10)]
    assert FID.is_split_bounds(7, 1) == [(0, 7)]
    for n, s in ((9, 10), (0, 1), (5, 0)):
        with pytest.raises(ValueError):
            FID.is_split_bounds(n, s)


# ------------------------------------------------------------------------------------------ the reference checks itself
def test_reference_inception_score():
    assert abs(REF.inception_score(np.zeros((40, 1008)), 10)[0] - 1.0) <= 1e-12
    for c, n in ((7, 70), (10, 100)):
        logits = np.zeros((n, c))
        logits[np.arange(n), np.arange(n) % c] = 80.0
        mean, std, parts = REF.inception_score(logits, 2)
        assert abs(mean - c) <= 1e-9 and std <= 1e-9 and np.abs(parts - c).max() <= 1e-9
    g = np.random.default_rng(1)
    z = 3.0 * g.standard_normal((23, 9))
    z[3, 2], z[5, 1] = 80.0, -80.0
    mean, std, parts = REF.inception_score(z, 10)
    loop = REF.inception_score_loop(z, 10)
    assert np.abs(parts / loop - 1.0).max() <= 1e-12 and abs(mean - loop.mean()) <= 1e-12 and abs(std - loop.std()) <= 1e-12
    # the host half of the library, fed by sums formed here: the same numbers
    zz = z - z.max(1, keepdims=True)
    p = np.exp(zz) / np.exp(zz).sum(1, keepdims=True)
    H = np.array([(p[lo:hi] * np.log(p[lo:hi])).sum() for lo, hi in REF.split_bounds(23, 10)])
    P = np.array([p[lo:hi].sum(0) for lo, hi in REF.split_bounds(23, 10)])
    got = FID.is_from_sums(H, P, 23, 10)
    assert np.abs(got[2] / parts - 1.0).max() <= 1e-12 and abs(got[0] - mean) <= 1e-12 and abs(got[1] - std) <= 1e-12


def test_reference_kid():
    g = np.random.default_rng(2)
    real, fake = g.standard_normal((9, 8)), g.standard_normal((7, 8)) + 0.5
    ir, jf = REF.subsets(9, 7, 4, 5, seed=1)
    ir[0, 1] = ir[0, 3]                                  # one bank row at two positions: they are a pair
    sums, loop = REF.poly_mmd_sums(real, fake, ir, jf), REF.poly_mmd_sums_loop(real, fake, ir, jf)
    assert np.abs(sums / loop - 1.0).max() <= 1e-12
    assert np.abs(REF.mmd2(sums, 5) - ((loop[:, 0] + loop[:, 1]) / 20.0 - 2.0 * loop[:, 2] / 25.0)).max() <= 1e-12
    mean, std = MF.kid_from_sums(sums, 5)
    assert (mean, std) == REF.kid(real, fake, ir, jf)
    # a set against itself with identical tables: XX = YY, XY = XX + the diagonal
    m = 6
    tab = REF.subsets(9, 9, 3, m, seed=2)[0]
    own = REF.poly_mmd_sums_loop(real, real, tab, tab)
    for s in range(3):
        diag = np.array([(real[i] @ real[i] / 8.0 + 1.0) ** 3 for i in tab[s]])
        want = -2.0 * diag.mean() / m + own[s, 0] * (2.0 / (m * (m - 1)) - 2.0 / (m * m))
        assert abs(REF.mmd2(REF.poly_mmd_sums(real, real, tab, tab), m)[s] - want) <= 1e-12 * max(1.0, abs(want))


# ------------------------------------------------------------------------------------------ MetricSuite on the host
class _Extractor:
    """stands in for InceptionFID on the host: uint8 [B,H,W,3] -> f32 [B,2048], a function of the pixels; the classifier comes from the file"""
    device = torch.device("cpu")

    def __init__(self, weights):
        self.calls, self.weights = 0, weights

    def __call__(self, u8):
        self.calls += 1
        g = torch.Generator().manual_seed(int(u8.sum()))
        return torch.rand(u8.shape[0], 2048, generator=g)

    def fc(self):
        return FID.load_inception_fc(self.weights)

    def logits(self, feats):
        return (feats @ self.fc().T).contiguous()


def _host_update(self, feats):
    f = feats.double()
    self.total += f.sum(0)
    self.outer += f.T @ f
    self.n += int(f.shape[0])


def _images(n, seed):
    return torch.randint(0, 256, (n, 4, 4, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


@pytest.fixture
def host(tmp_path, monkeypatch):
    """(a factory of suites on the host, the stand-in extractor, what was saved, what the kernels' stand-ins saw)"""
    weights = str(tmp_path / "inception.pth")
    torch.save({"fc.weight": torch.randn((1008, 2048), generator=torch.Generator().manual_seed(0)) / 45.0}, weights)
    ex = _Extractor(weights)
    saved, seen = [], {}
    real_save = MF.save_features
    monkeypatch.setattr(FID, "InceptionFID", lambda path, device: ex)
    monkeypatch.setattr(EV, "_models", {})
    monkeypatch.setattr(FID.FeatureStats, "update", _host_update)
    monkeypatch.setattr(MF, "save_features", lambda path, feats: (saved.append(os.path.basename(path)), real_save(path, feats))[1])
    monkeypatch.setattr(MF, "prdc", lambda r, f, k: (seen.update(prdc=(r, f)), dict(precision=1.0, recall=1.0, density=1.0, coverage=1.0, k=k,
                                                                                   n_real=r.n, n_fake=f.n))[1])

    def host_kid(r, f, subsets, size, seed):
        seen.update(kid=(r, f))
        ir, jf = MF.kid_subsets(r.n, f.n, subsets, size, seed)
        mean, std = REF.kid(r.rows().numpy(), f.rows().numpy(), ir, jf)
        return dict(kid=mean, std=std, subsets=subsets, subset_size=ir.shape[1], n_real=r.n, n_fake=f.n)
    monkeypatch.setattr(MF, "kid", host_kid)
    return (lambda **kw: EV.MetricSuite("cpu", weights, **kw)), ex, saved, seen


def _feed(suite, d=None):
    if d:
        suite.open_cache(d)
    for s in (1, 2):
        suite.update_fake(_images(3, s))
        suite.update_real(_images(3, 10 + s))
    suite.real_from_cache(6, lambda: pytest.fail("the real images were asked for again"))
    return list(suite.results())


def test_kid_and_prdc_share_one_bank_and_one_file(host, tmp_path):
    make, ex, saved, seen = host
    suite = make(prdc_k=2, kid=True, kid_subsets=3, kid_subset_size=4)
    assert suite.fake[EV.KID] is suite.fake[EV.PRDC]
    res = _feed(suite, str(tmp_path))
    assert ex.calls == 4                                  # one extractor pass per batch and side
    assert [m for m, _, _ in res] == [EV.FID, EV.PRDC, EV.KID] and all(w is None for _, _, w in res)
    assert saved == ["org_features.npz"]                  # (FID's statistics file goes through save_stats)
    assert seen["kid"][0] is seen["prdc"][0] and seen["kid"][1] is seen["prdc"][1] and seen["kid"][1].n == 6
    kid = res[2][1]
    assert (kid["subsets"], kid["subset_size"], kid["n_real"], kid["n_fake"]) == (3, 4, 6, 6)
    # a second suite finds the file: nothing is gathered, nothing is written
    del saved[:]
    suite = make(prdc_k=2, kid=True, kid_subsets=3, kid_subset_size=4)
    suite.open_cache(str(tmp_path))
    assert not suite.wants_real
    for s in (1, 2):
        suite.update_fake(_images(3, s))
    suite.real_from_cache(6, lambda: pytest.fail("asked again"))
    assert list(suite.results())[2][1] == kid and saved == []
    # KID alone keeps the same file
    suite = make(kid=True, fid=False, kid_subsets=3, kid_subset_size=4)
    assert list(suite.fake) == [EV.KID] and suite.wants_real == [EV.KID]
    suite.open_cache(str(tmp_path))
    assert not suite.wants_real
    for s in (1, 2):
        suite.update_fake(_images(3, s))
    suite.real_from_cache(6, lambda: pytest.fail("asked again"))
    assert [(m, v) for m, v, _ in suite.results()] == [(EV.KID, kid)] and saved == []


def test_flags_off_results_are_what_they_were(host, tmp_path):
    make, ex, saved, seen = host
    res = _feed(make(prdc_k=2), str(tmp_path))
    assert [m for m, _, _ in res] == [EV.FID, EV.PRDC] and "kid" not in seen
    plain = EV.MetricSuite("cpu")
    assert plain.fake == {} and plain.why == {} and list(plain.results()) == []
    # asked for without the Inception weights: one reason each, after the existing ones
    res = list(EV.MetricSuite("cpu", "", prdc_k=2, kid=True, inception_score=10).results())
    assert [m for m, _, _ in res] == [EV.PRDC, EV.KID, EV.IS] and all(v is None and "fid_inception" in w for _, v, w in res)


def test_inception_score_through_the_suite(host, monkeypatch):
    make, ex, saved, seen = host
    from xmc_gan_amd import ops

    def host_sums(logits, splits, classes=None):
        z = logits.double().numpy()
        z = z - z.max(1, keepdims=True)
        p = np.exp(z) / np.exp(z).sum(1, keepdims=True)
        b = REF.split_bounds(z.shape[0], splits)
        return (torch.tensor([(p[lo:hi] * np.log(p[lo:hi])).sum() for lo, hi in b]), torch.from_numpy(np.stack([p[lo:hi].sum(0) for lo, hi in b])))
    monkeypatch.setattr(ops, "inception_score_sums", host_sums)
    suite = make(fid=False, inception_score=2)
    assert list(suite.fake) == [EV.IS] and not suite.wants_real
    for s in (1, 2):
        suite.update_fake(_images(3, s))
    (metric, values, why), = suite.results()
    want = REF.inception_score(torch.cat([ex.logits(_Extractor(None)(_images(3, s))) for s in (1, 2)]).numpy(), 2)
    assert metric == EV.IS and why is None and (values["splits"], values["n"]) == (2, 6)
    assert abs(values["inception_score"] - want[0]) <= 1e-12 and abs(values["std"] - want[1]) <= 1e-12
    # fewer images than splits: the reason, not an error
    suite = make(fid=False, inception_score=10)
    suite.update_fake(_images(3, 1))
    (metric, values, why), = suite.results()
    assert values is None and "10 splits" in why


def test_weights_without_the_classifier_give_the_reason(host, tmp_path):
    make, ex, _, _ = host
    for sd, what in (({"other": torch.zeros(1)}, "hold no 'fc.weight'"), ({"fc.weight": torch.zeros(1000, 2048)}, r"\[1008, 2048\]")):
        torch.save(sd, ex.weights)
        suite = make(inception_score=10)
        assert EV.IS not in suite.fake and EV.FID in suite.fake
        res = _feed(suite)
        assert [m for m, _, _ in res] == [EV.FID, EV.IS] and res[1][1] is None
        import re
        assert re.search(what, res[1][2])
    with pytest.raises(ValueError, match="fc.weight"):
        FID.load_inception_fc(ex.weights)
    with pytest.raises(ImportError):
        FID.load_inception_fc(str(tmp_path / "nowhere.pth"))


# ------------------------------------------------------------------------------------------ the command lines
def test_command_lines_refuse_before_a_device_is_touched(tmp_path, monkeypatch):
    import xmc_gan.inception_score as is_cli
    import xmc_gan.kid as kid_cli
    from PIL import Image
    monkeypatch.delenv("XMC_FID_INCEPTION", raising=False)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("a device was asked for"))
    g = np.random.default_rng(0)
    feats, one, stats = str(tmp_path / "f.npz"), str(tmp_path / "one.npz"), str(tmp_path / "s.npz")
    MF.save_features(feats, g.standard_normal((5, 2048)))
    MF.save_features(one, g.standard_normal((1, 2048)))
    FID.save_stats(stats, np.zeros(4), np.eye(4), n=9)
    imgs, single, weights = tmp_path / "imgs", tmp_path / "single", str(tmp_path / "w.pth")
    for d, n in ((imgs, 3), (single, 1)):
        d.mkdir()
        for i in range(n):
            Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(str(d / f"{i}.png"))
    open(weights, "wb").close()
    for argv, what in (([str(tmp_path / "nowhere"), feats], "neither an image directory"), ([feats, str(tmp_path / "x.txt")], "neither an image directory"),
                       ([stats, feats], "statistics file"), ([feats, stats], "statistics file"), ([feats, feats, "--subsets", "0"], "--subsets"),
                       ([feats, feats, "--subset_size", "1"], "--subset_size"), ([feats, one], "two rows"), ([str(single), feats], "fewer than two images"),
                       ([str(imgs), feats], "needs the FID Inception weights"), ([str(imgs), feats, "--inception", str(tmp_path / "no.pth")], "is not a file"),
                       ([feats, feats, "--batch", "0"], "--batch")):
        with pytest.raises(SystemExit, match=what):
            kid_cli.main(argv)
    for argv, what in (([str(tmp_path / "nowhere")], "not an image directory"), ([feats], "not an image directory"),
                       ([str(imgs), "--splits", "0"], "--splits"), ([str(imgs), "--splits", "4", "--inception", weights], "fewer than --splits"),
                       ([str(imgs), "--splits", "2"], "needs the FID Inception weights"),
                       ([str(imgs), "--splits", "2", "--inception", str(tmp_path / "no.pth")], "is not a file")):
        with pytest.raises(SystemExit, match=what):
            is_cli.main(argv)


def test_trainer_flags(monkeypatch):
    import xmc_gan.train_gan as tg
    a = tg.parse_args([])
    assert (a.kid, a.kid_subsets, a.kid_subset_size, a.inception_score) == (False, 100, 1000, 0)
    assert tg.parse_args(["--inception_score"]).inception_score == 10 and tg.parse_args(["--inception_score", "5"]).inception_score == 5
    assert tg.EvalOptions() == ("", 0, "", False, 100, 1000, 0) and tg.EvalOptions("w", 3, "d")[:3] == ("w", 3, "d")
    assert tg._new_metric_args(tg.EvalOptions(), None, None, None, None) == {}
    assert tg._new_metric_args(tg.EvalOptions(kid=True, inception_score=4), None, 7, None, None) == dict(kid=True, kid_subsets=7, kid_subset_size=1000,
                                                                                                         inception_score=4)
    line, tags, without = tg._EVAL_REPORT["KID"]
    assert line.format(epoch=7, kid=0.5, std=0.1, subsets=3, subset_size=8, n_real=8, n_fake=8) == " epoch 7, KID : 0.5 +- 0.1 (subsets=3, size=8, n=8/8)"
    line, tags, without = tg._EVAL_REPORT["IS"]
    assert line.format(epoch=7, inception_score=2.5, std=0.1, splits=2, n=8) == " epoch 7, IS : 2.5 +- 0.1 (splits=2, n=8)"
    assert without.format(epoch=7, cnt=8, why="x") == " epoch 7, IS not computed: x"
