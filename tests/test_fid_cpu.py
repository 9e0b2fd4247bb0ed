"""Host side of the FID evaluation (xmc_gan_amd/fid.py, xmc_gan/fid.py): the Fréchet distance against the textbook formula, the
statistics file, BatchNorm folding, the weight loader's refusals, the command line's refusals, and `fid_between`'s unchanged default."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fid_ref
from xmc_gan_amd import fid as FID


def _stats(n, d, seed):
    """mean / covariance (np.cov) of n ReLU'd correlated random feature rows"""
    g = np.random.default_rng(seed)
    x = np.maximum(g.standard_normal((n, d)) @ g.standard_normal((d, d)) / np.sqrt(d) + 0.3, 0.0)
    return x.mean(0), np.cov(x, rowvar=False)


CASES = [(400, 128), (2000, 256), (64, 128), (37, 96)]          # the last two: fewer samples than dimensions, singular covariances


@pytest.mark.parametrize("n,d", CASES)
def test_frechet_distance_against_sqrtm(n, d):
    """|mu1 - mu2|^2 + tr(s1 + s2 - 2 sqrtm(s1 s2)) with scipy's sqrtm.  Measured relative differences: 2e-15, 1e-14 (full rank), 2.8e-8,
    3.0e-8 (singular: sqrtm's own error on a singular product); the bar is 1e-6, far below the two decimals an FID is quoted to."""
    from scipy.linalg import sqrtm
    (m1, s1), (m2, s2) = _stats(n, d, 1), _stats(n, d, 2)
    ref = ((m1 - m2) ** 2).sum() + np.trace(s1) + np.trace(s2) - 2.0 * np.trace(sqrtm(s1 @ s2).real)
    got = FID.frechet_distance(m1, s1, m2, s2)
    rel = abs(got - ref) / abs(ref)
    print(f"frechet_distance n={n} d={d}: {got} vs {ref}, relative difference {rel:.2e}")
    assert rel <= 1e-6


@pytest.mark.parametrize("n,d", CASES)
def test_frechet_distance_identical_and_symmetric(n, d):
    (m1, s1), (m2, s2) = _stats(n, d, 3), _stats(n, d, 4)
    same = FID.frechet_distance(m1, s1, m1, s1)
    print(f"identical statistics n={n} d={d}: {same:.3e} (tr sigma {np.trace(s1):.3e})")
    assert abs(same) <= 1e-9 * np.trace(s1)
    ab, ba = FID.frechet_distance(m1, s1, m2, s2), FID.frechet_distance(m2, s2, m1, s1)
    # both orders are the singular values of a matrix and of its transpose: equal up to the rounding of two f64 products
    assert abs(ab - ba) <= 1e-12 * (np.trace(s1) + np.trace(s2))
    assert ab > 0


def test_frechet_distance_refuses_mismatched_shapes():
    m, s = _stats(20, 8, 0)
    with pytest.raises(ValueError):
        FID.frechet_distance(m, s, m[:4], s[:4, :4])


def test_stats_npz_round_trip(tmp_path):
    m, s = _stats(50, 16, 5)
    p = str(tmp_path / "a.npz")
    FID.save_stats(p, m, s, 50)
    assert sorted(os.listdir(tmp_path)) == ["a.npz"]
    m2, s2, n = FID.load_stats(p, with_count=True)
    assert n == 50 and m2.dtype == np.float64 and np.array_equal(m, m2) and np.array_equal(s, s2)
    with np.load(p) as z:                                   # what pytorch_fid reads
        assert np.array_equal(z["mu"], m) and np.array_equal(z["sigma"], s)
    q = str(tmp_path / "b.npz")                             # a file pytorch_fid wrote: no count
    np.savez(q, mu=m, sigma=s)
    assert FID.load_stats(q, with_count=True)[2] is None and np.array_equal(FID.load_stats(q)[1], s)
    np.savez(str(tmp_path / "c.npz"), mu=m)
    with pytest.raises(ValueError):
        FID.load_stats(str(tmp_path / "c.npz"))


def test_fold_bn_against_batch_norm():
    g = torch.Generator().manual_seed(0)
    w = torch.randn(24, 16, 1, 7, generator=g) * 0.1
    gamma, beta = 1 + 0.1 * torch.randn(24, generator=g), 0.1 * torch.randn(24, generator=g)
    mean, var = 0.1 * torch.randn(24, generator=g), 0.5 + torch.rand(24, generator=g)
    x = torch.randn(2, 16, 5, 9, generator=g).double()
    F = torch.nn.functional
    ref = F.batch_norm(F.conv2d(x, w.double(), padding=(0, 3)), mean.double(), var.double(), gamma.double(), beta.double(), training=False, eps=1e-3)
    wf, bf = FID.fold_bn(w, gamma, beta, mean, var)
    assert wf.dtype == torch.float32 and bf.dtype == torch.float32 and wf.shape == w.shape
    got = F.conv2d(x, wf.double(), bf.double(), padding=(0, 3))
    # the folded weights are f64 results rounded once to f32: 2^-24 relative each, over a sum of 16 * 7 terms of order 0.1
    assert (got - ref).abs().max() <= 1e-6 * ref.abs().max()
    # eps is 1e-3, not BatchNorm2d's default 1e-5
    assert not torch.allclose(FID.fold_bn(w, gamma, beta, mean, var, eps=1e-5)[0], wf, rtol=1e-5, atol=0)


def test_layer_table_matches_the_restatement():
    mine = FID.inception_layers()
    theirs = fid_ref.layer_table()
    assert len(mine) == len(theirs) == 94 and list(mine) == [t[0] for t in theirs]
    for name, cin, cout, k, s, p in theirs:
        assert mine[name] == (cin, cout, fid_ref._pair(k), s, fid_ref._pair(p)), name


def test_loader_error_paths(tmp_path, monkeypatch):
    monkeypatch.delenv("XMC_FID_INCEPTION", raising=False)
    with pytest.raises(ImportError, match="XMC_FID_INCEPTION"):
        FID.load_inception_weights(None)
    with pytest.raises(ImportError, match="does not exist"):
        FID.load_inception_weights(str(tmp_path / "nope.pth"))
    sd = fid_ref.random_state_dict(0)
    good = str(tmp_path / "good.pth")
    torch.save(sd, good)
    w = FID.load_inception_weights(good)
    assert len(w) == 94 and tuple(w["Mixed_6b.branch7x7_2"][0].shape) == (128, 128, 1, 7)
    monkeypatch.setenv("XMC_FID_INCEPTION", good)
    assert len(FID.load_inception_weights(None)) == 94
    lack = dict(sd)
    del lack["Mixed_7c.branch_pool.bn.running_var"]
    torch.save(lack, str(tmp_path / "lack.pth"))
    with pytest.raises(ImportError, match="Mixed_7c.branch_pool.bn.running_var"):
        FID.load_inception_weights(str(tmp_path / "lack.pth"))
    bad = dict(sd)
    bad["Mixed_6b.branch7x7_2.conv.weight"] = bad["Mixed_6b.branch7x7_2.conv.weight"].permute(0, 1, 3, 2).contiguous()      # 7x1 for 1x7
    torch.save(bad, str(tmp_path / "bad.pth"))
    with pytest.raises(ValueError, match="Mixed_6b.branch7x7_2.conv.weight"):
        FID.load_inception_weights(str(tmp_path / "bad.pth"))


def test_cli_argument_errors(tmp_path, monkeypatch, capsys):
    from PIL import Image
    from xmc_gan import fid as cli
    monkeypatch.delenv("XMC_FID_INCEPTION", raising=False)
    empty, full = tmp_path / "empty", tmp_path / "full"
    empty.mkdir(), full.mkdir()
    for i in range(3):
        Image.fromarray(np.full((8, 8, 3), 40 * i, np.uint8)).save(str(full / f"{i}.png"))
    m, s = _stats(30, 8, 6)
    FID.save_stats(str(tmp_path / "a.npz"), m, s)
    FID.save_stats(str(tmp_path / "b.npz"), *_stats(30, 8, 7))
    weights = tmp_path / "w.pth"
    weights.write_bytes(b"")
    for argv, word in (([str(empty), str(full), "--inception", str(weights)], "fewer than two images"),
                       ([str(full), str(tmp_path / "missing"), "--inception", str(weights)], "neither"),
                       ([str(full), str(tmp_path / "a.npz")], "--inception"),
                       ([str(full), str(tmp_path / "a.npz"), "--inception", str(tmp_path / "nope.pth")], "not a file"),
                       ([str(tmp_path / "a.npz"), str(tmp_path / "b.npz"), "--batch", "0"], "--batch")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code not in (0, None) and word in str(e.value.code) and "\n" not in str(e.value.code), (argv, e.value.code)
    # two statistics files need neither weights nor a device
    out = str(tmp_path / "copy.npz")
    value = cli.main([str(tmp_path / "a.npz"), str(tmp_path / "b.npz"), "--save_stats", out])
    assert capsys.readouterr().out.strip() == f"FID: {value}" and value > 0
    assert np.array_equal(FID.load_stats(out)[1], s)


def test_fid_between_without_weights_is_unchanged(monkeypatch):
    from xmc_gan.utils.visual import fid_between
    monkeypatch.setitem(sys.modules, "pytorch_fid", None)               # (not importable, whether or not it is installed)
    monkeypatch.setitem(sys.modules, "pytorch_fid.fid_score", None)
    monkeypatch.delenv("XMC_FID_INCEPTION", raising=False)
    assert fid_between("/nonexistent/a", "/nonexistent/b", "cpu") is None
