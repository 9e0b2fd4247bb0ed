"""The evaluation pipeline's host code (xmc_gan_amd/evaluate.py), without a device: where a metric's weights come from and what the refusals
say, the real side's cache rule, the loaded-model cache, and that a run which asks for no metric imports none of the metric modules."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from xmc_gan_amd import evaluate as EV
from xmc_gan_amd import fid as FID
from xmc_gan_amd import manifold as MF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F_ENV, D_ENV = "XMC_FID_INCEPTION", "XMC_DAMSM_IMAGE_ENCODER"


# ------------------------------------------------------------------------------------------ paths
def test_resolve_weights(tmp_path, monkeypatch):
    good, other, nope = str(tmp_path / "w.pth"), str(tmp_path / "env.pth"), str(tmp_path / "nope.pth")
    for p in (good, other):
        open(p, "wb").close()
    monkeypatch.delenv(F_ENV, raising=False)
    monkeypatch.delenv(D_ENV, raising=False)
    # the trainer: the flag, else the variable, else nothing ('' : the metric is off); a path that is no file is refused
    assert EV.resolve_weights(good, F_ENV, "--fid_inception", must_exist=False) == good
    assert EV.resolve_weights("", F_ENV, "--fid_inception", must_exist=False) == ""
    with pytest.raises(SystemExit) as e:
        EV.resolve_weights(nope, F_ENV, "--fid_inception", must_exist=False)
    assert str(e.value) == f"--fid_inception: {nope} is not a file"
    with pytest.raises(SystemExit) as e:
        EV.resolve_weights(nope, D_ENV, "--damsm_image_encoder", must_exist=False)
    assert str(e.value) == f"--damsm_image_encoder: {nope} is not a file"
    # xmc_gan/fid.py and xmc_gan/prdc.py: a directory cannot be scored without them
    with pytest.raises(SystemExit) as e:
        EV.resolve_weights("", F_ENV, "--inception")
    assert str(e.value) == "scoring a directory needs the FID Inception weights: --inception PATH or XMC_FID_INCEPTION"
    with pytest.raises(SystemExit) as e:
        EV.resolve_weights(nope, F_ENV, "--inception")
    assert str(e.value) == f"--inception: {nope} is not a file"
    # sample.py and xmc_gan/rprecision.py: one message for both, with what was got
    for given in ("", nope):
        with pytest.raises(SystemExit) as e:
            EV.resolve_weights(given, F_ENV, "--fid_inception", refusal="--fid_against needs the FID Inception weights")
        assert str(e.value) == f"--fid_against needs the FID Inception weights: --fid_inception PATH or XMC_FID_INCEPTION (got {given!r})"
        with pytest.raises(SystemExit, match="prdc_against") as e:
            EV.resolve_weights(given, F_ENV, "--fid_inception", refusal="--prdc_against needs the FID Inception weights")
        assert "fid_inception" in str(e.value) and F_ENV in str(e.value)
        with pytest.raises(SystemExit) as e:
            EV.resolve_weights(given, D_ENV, "--damsm_image_encoder", refusal="--rprecision needs the DAMSM image encoder weights")
        assert str(e.value) == (f"--rprecision needs the DAMSM image encoder weights: --damsm_image_encoder PATH or XMC_DAMSM_IMAGE_ENCODER "
                                f"(got {given!r})")
        with pytest.raises(SystemExit) as e:
            EV.resolve_weights(given, D_ENV, "--image_encoder", refusal="the DAMSM image encoder weights are needed")
        assert str(e.value) == f"the DAMSM image encoder weights are needed: --image_encoder PATH or XMC_DAMSM_IMAGE_ENCODER (got {given!r})"
    assert EV.resolve_weights(good, D_ENV, "--image_encoder", refusal="the DAMSM image encoder weights are needed") == good
    # the variable stands in for an empty flag, and only for an empty flag
    monkeypatch.setenv(F_ENV, other)
    assert EV.resolve_weights("", F_ENV, "--fid_inception", must_exist=False) == other
    assert EV.resolve_weights("", F_ENV, "--inception") == other
    assert EV.resolve_weights("", F_ENV, "--fid_inception", refusal="--fid_against needs the FID Inception weights") == other
    assert EV.resolve_weights(good, F_ENV, "--inception") == good
    monkeypatch.setenv(F_ENV, nope)
    with pytest.raises(SystemExit) as e:
        EV.resolve_weights("", F_ENV, "--fid_inception", must_exist=False)
    assert str(e.value) == f"--fid_inception: {nope} is not a file"


def test_image_set_kind(tmp_path):
    npz, txt = tmp_path / "a.npz", tmp_path / "a.txt"
    for p in (npz, txt):
        p.write_bytes(b"")
    assert EV.image_set_kind(str(tmp_path)) == "dir" and EV.image_set_kind(str(npz)) == "npz"
    assert EV.image_set_kind(str(txt)) is None and EV.image_set_kind(str(tmp_path / "nowhere")) is None
    assert EV.image_set_kind(str(tmp_path / "nowhere.npz")) is None
    os.makedirs(str(tmp_path / "d.npz"))
    assert EV.image_set_kind(str(tmp_path / "d.npz")) == "dir"


# ------------------------------------------------------------------------------------------ the cache rule
class _Extractor:
    """stands in for InceptionFID on the host: uint8 [B,H,W,3] -> f32 [B,2048], a function of the pixels"""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = 0

    def __call__(self, u8):
        self.calls += 1
        g = torch.Generator().manual_seed(int(u8.sum()))
        return torch.rand(u8.shape[0], 2048, generator=g)


def _host_update(self, feats):
    """`FeatureStats.update` without the moments kernel"""
    f = feats.double()
    self.total += f.sum(0)
    self.outer += f.T @ f
    self.n += int(f.shape[0])


@pytest.fixture
def host_suite(tmp_path, monkeypatch):
    """(a factory of FID + PRDC suites on the host, the stand-in extractor, the weights path)"""
    ex = _Extractor()
    weights = str(tmp_path / "inception.pth")
    open(weights, "wb").close()
    monkeypatch.setattr(FID, "InceptionFID", lambda path, device: ex)
    monkeypatch.setattr(EV, "_models", {})
    monkeypatch.setattr(FID.FeatureStats, "update", _host_update)
    return (lambda: EV.MetricSuite("cpu", weights, prdc_k=2)), ex


def _images(n, seed):
    return torch.randint(0, 256, (n, 4, 4, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def _write_caches(d, n=8):
    g = np.random.default_rng(3)
    feats = g.standard_normal((n, 2048)).astype(np.float32)
    FID.save_stats(os.path.join(d, "org_stats.npz"), feats.mean(0), np.cov(feats, rowvar=False), n=n)
    MF.save_features(os.path.join(d, "org_features.npz"), feats)
    return feats


def _mtimes(d):
    return [os.stat(os.path.join(d, f)).st_mtime_ns for f in ("org_stats.npz", "org_features.npz")]


def _never():
    raise AssertionError("the real images were asked for again")


def test_cache_of_the_same_count_is_reused(host_suite, tmp_path):
    make, ex = host_suite
    d = str(tmp_path)
    feats = _write_caches(d, 8)
    before = _mtimes(d)
    suite = make()
    suite.open_cache(d)
    assert not suite.wants_real                          # both files read: no real image goes through the extractor
    suite.update_fake(_images(8, 1))
    suite.update_real(_images(8, 2))
    assert ex.calls == 1
    suite.real_from_cache(8, _never)
    mu, sigma = suite.real[EV.FID]()
    assert np.array_equal(mu, feats.mean(0).astype(np.float64)) and np.array_equal(sigma, np.cov(feats, rowvar=False))       # the file's own
    bank = suite.real[EV.PRDC]()
    assert bank.n == 8 and np.array_equal(bank.rows().numpy(), feats)
    assert _mtimes(d) == before                          # nothing was computed again: nothing is written


def test_cache_of_another_count_is_computed_again_in_one_pass(host_suite, tmp_path):
    make, ex = host_suite
    d = str(tmp_path)
    _write_caches(d, 8)
    before = _mtimes(d)
    suite = make()
    suite.open_cache(d)
    assert not suite.wants_real                          # (the count is known only after the last batch)
    fake, real = [_images(3, 1), _images(3, 2)], [_images(3, 3), _images(3, 4), _images(3, 5)]
    for u8 in fake:
        suite.update_fake(u8)
    passes = []
    suite.real_from_cache(6, lambda: (passes.append(1), iter(real))[1])
    assert passes == [1] and ex.calls == 2 + 2           # one more pass for both metrics, stopped at 6 rows
    want = torch.cat([_Extractor()(u8) for u8 in real[:2]])
    assert np.array_equal(suite.real[EV.PRDC]().rows().numpy(), want.numpy())
    mu, sigma, n = FID.load_stats(os.path.join(d, "org_stats.npz"), with_count=True)
    assert n == 6 and np.allclose(mu, want.double().mean(0).numpy(), rtol=0, atol=1e-12)
    assert MF.load_features(os.path.join(d, "org_features.npz")).shape == (6, 2048)
    assert all(a > b for a, b in zip(_mtimes(d), before))
    assert np.array_equal(suite.real[EV.FID]()[0], mu)


def test_without_a_cache_the_gathered_rows_are_the_real_side_and_are_written(host_suite, tmp_path):
    make, ex = host_suite
    d = str(tmp_path)
    suite = make()
    suite.open_cache(d)
    assert suite.wants_real
    for s in (1, 2):
        suite.update_fake(_images(3, s))
        suite.update_real(_images(3, 10 + s))
    assert ex.calls == 4
    suite.real_from_cache(6, _never)
    assert FID.load_stats(os.path.join(d, "org_stats.npz"), with_count=True)[2] == 6
    assert MF.load_features(os.path.join(d, "org_features.npz")).shape == (6, 2048)
    # and with no directory nothing is written anywhere
    suite = make()
    assert suite.wants_real
    suite.update_fake(_images(3, 1))
    suite.update_real(_images(3, 2))
    suite.real_from_cache(3, _never)
    assert not suite.wants_real and suite.real[EV.PRDC]().n == 3


def test_foreign_and_unreadable_cache_files(host_suite, tmp_path):
    make, ex = host_suite
    d = str(tmp_path)
    feats = _write_caches(d, 8)
    # a feature file that holds something else is no cache: the rows are gathered and the file is written over
    FID.save_stats(os.path.join(d, "org_features.npz"), feats.mean(0), np.cov(feats, rowvar=False), n=8)
    suite = make()
    suite.open_cache(d)
    assert suite.wants_real                              # (for the feature rows; the statistics file still reads)
    suite.update_fake(_images(8, 1))
    suite.update_real(_images(8, 2))
    suite.real_from_cache(8, _never)
    assert MF.load_features(os.path.join(d, "org_features.npz")).shape == (8, 2048)
    # a statistics file without a count (pytorch_fid's) is a file for another count
    FID.save_stats(os.path.join(d, "org_stats.npz"), feats.mean(0), np.cov(feats, rowvar=False))
    suite = make()
    suite.open_cache(d)
    suite.update_fake(_images(8, 1))
    passes = []
    suite.real_from_cache(8, lambda: (passes.append(1), iter([_images(8, 2)]))[1])
    assert passes == [1] and FID.load_stats(os.path.join(d, "org_stats.npz"), with_count=True)[2] == 8
    # a statistics file that holds something else is an error, as it always was
    MF.save_features(os.path.join(d, "org_stats.npz"), feats)
    with pytest.raises(ValueError, match="mu"):
        make().open_cache(d)


# ------------------------------------------------------------------------------------------ the loaded models
def test_model_cache_holds_one_model_per_kind_and_follows_the_file(tmp_path, monkeypatch):
    loads = []
    from xmc_gan_amd import rprecision as RP
    monkeypatch.setattr(FID, "InceptionFID", lambda path, device: (loads.append(("inception", path)), object())[1])
    monkeypatch.setattr(RP, "load_image_encoder", lambda path, nef, device: (loads.append(("damsm", path)), object())[1])
    monkeypatch.setattr(EV, "_models", {})
    a, b = str(tmp_path / "a.pth"), str(tmp_path / "b.pth")
    for p in (a, b):
        open(p, "wb").close()
    m1 = EV.load_model("inception", a, "cpu")
    assert EV.load_model("inception", a, torch.device("cpu")) is m1 and len(loads) == 1
    assert EV.load_model("inception", os.path.join(str(tmp_path), ".", "a.pth"), "cpu") is m1          # (the same file by another spelling)
    d1 = EV.load_model("damsm", b, "cpu")                # another kind: a model of its own, beside the first
    assert d1 is not m1 and EV.load_model("inception", a, "cpu") is m1 and len(loads) == 2
    st = os.stat(a)
    os.utime(a, ns=(st.st_atime_ns, st.st_mtime_ns + 10 ** 9))          # the file was rewritten
    m2 = EV.load_model("inception", a, "cpu")
    assert m2 is not m1 and len(loads) == 3 and EV.load_model("inception", a, "cpu") is m2
    m3 = EV.load_model("inception", b, "cpu")            # another file takes its place
    assert m3 is not m2 and len(EV._models) == 2 and EV.load_model("damsm", b, "cpu") is d1
    assert EV.load_model("inception", a, "cpu") is not m2 and len(loads) == 5
    from xmc_gan.utils.visual import fid_extractor
    assert fid_extractor(a, "cpu") is EV.load_model("inception", a, "cpu")


# ------------------------------------------------------------------------------------------ lazy imports
def test_a_run_without_metrics_imports_no_metric_module():
    code = ("import sys\n"
            "import xmc_gan.train_gan as tg\n"
            "tg.parse_args([])\n"
            "import xmc_gan.sample\n"
            "print([m for m in ('xmc_gan_amd.fid', 'xmc_gan_amd.manifold', 'xmc_gan_amd.rprecision') if m in sys.modules])\n")
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == "[]"
