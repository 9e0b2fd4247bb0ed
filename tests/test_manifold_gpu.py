"""Precision / recall / density / coverage on the GPU (xmc_gan_amd/manifold.py, csrc/manifold.hip) against the f64 restatement in
tests/manifold_ref.py.

Integer lattices make every product and sum exact in f32: there the radii, counts and minima must EQUAL the reference, ties at the k-th
radius included.  On real-valued rows a decision within the band TAU * (|a|^2 + |b|^2) of its threshold may fall either way (the band is
derived in manifold_ref.py from the f32 MFMA chain's error, not measured here): such a row is "ambiguous", the reference alone must show
that at most 2 % of the rows are, every other row's count must equal the reference and an ambiguous one must lie in [lo, hi].  The radii
and nearest distances are continuous: the error figure is the project's, max |got - want| over the rms of `want`, and every bar is 1.5 x
the figure measured on the MI355X, written beside it; above 1e-4 would be a bug, not rounding.  The sizes straddle the 32 / 64 / 128-row
tiles, the 32-column stage of D (D = 8, 12, 72) and more than one workgroup and slice."""
import functools
import logging
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fid_ref
import manifold_ref as REF
from xmc_gan_amd import fid as FID
from xmc_gan_amd import manifold as MF
from xmc_gan_amd import ops

DEV = torch.device("cuda", 0)

SETS = {"gauss8": (REF.gaussian, (130, 67, 8, 1), 3), "gauss72": (REF.gaussian, (257, 300, 72, 2), 5), "gauss64": (REF.gaussian, (300, 257, 64, 3), 5),
        "lowrank3": (REF.lowrank, (513, 129, 2048, 4), 3), "lowrank5": (REF.lowrank, (300, 257, 2048, 5), 5)}
# measured on the MI355X: (rad2 of the real rows, rad2 of the generated rows, near2 of the real rows, near2 of the generated rows)
MEASURED = {"gauss8": (4.769e-07, 4.843e-07, 5.356e-07, 5.267e-07), "gauss72": (2.097e-07, 2.305e-07, 2.765e-07, 2.706e-07),
            "gauss64": (3.186e-07, 4.270e-07, 4.470e-07, 2.885e-07), "lowrank3": (2.754e-06, 2.232e-06, 2.868e-06, 5.448e-06),
            "lowrank5": (2.613e-06, 1.721e-06, 3.492e-06, 4.351e-06)}
# (the low-rank rows lie close together: d2 is a few percent of |a|^2 + |b|^2, and the rounding of the norms and the dot, ~1e-7 of THAT sum,
# is ten times larger relative to d2)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(real, fake, k, the reference) of a named set: built once, shared by the tests, never modified"""
    make, args, k = SETS[name]
    real, fake = make(*args)
    return real, fake, k, REF.reference(real, fake, k)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _err(got, want):
    got, want = got.double().cpu().numpy(), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max() / np.sqrt((want ** 2).mean()))


def _run(real, fake, k, slices=0):
    """the four launches of `prdc`, every per-row result kept"""
    r, f = _dev(real), _dev(fake)
    rad_r, rad_g = ops.knn_radius2(r, k, slices), ops.knn_radius2(f, k, slices)
    cnt_g, near_g = ops.manifold_count(f, r, rad_r, slices)
    cnt_r, near_r = ops.manifold_count(r, f, rad_g, slices)
    return dict(rad2_r=rad_r, rad2_g=rad_g, cnt_g=cnt_g, near2_g=near_g, cnt_r=cnt_r, near2_r=near_r)


# ------------------------------------------------------------------------------------------ exact
def _assert_equal(got, want):
    for name in ("rad2_r", "rad2_g", "near2_r", "near2_g"):
        assert got[name].dtype == torch.float32 and np.array_equal(got[name].double().cpu().numpy(), want[name]), name
    for name in ("cnt_g", "cnt_r"):
        assert got[name].dtype == torch.int32 and np.array_equal(got[name].cpu().numpy(), want[name]), name


@pytest.mark.parametrize("k", [3, 1, 16])
def test_lattice_equals_the_reference(k):
    real, fake = REF.lattice()                        # 130 x 12 and 67 x 12, entries 0..3
    want = REF.reference(real, fake, k)
    if k == 3:                                         # what makes the case worth having, from the reference alone
        d = REF.sqdist(real, real)
        np.fill_diagonal(d, np.inf)
        d.sort(axis=1)
        assert int((d[:, 2] == d[:, 3]).sum()) == 41   # rows with a tie exactly at the k-th radius
        assert int(want["ambiguous_g"].sum()) > 0      # decisions exactly on a radius
    _assert_equal(_run(real, fake, k), want)


@pytest.mark.parametrize("nr,ng,d,k", [(4, 4, 12, 3), (2, 2, 4, 1), (130, 67, 4, 3), (17, 17, 12, 16), (129, 128, 36, 2)])
def test_small_lattices_equal_the_reference(nr, ng, d, k):
    """D = 4, N = k + 1 (the smallest legal set), and a D just past one 32-column stage"""
    real, fake = REF.lattice(nr, ng, d, seed=nr + d)
    _assert_equal(_run(real, fake, k), REF.reference(real, fake, k))


def test_single_query_row_and_optional_outputs():
    real, fake = REF.lattice()
    want = REF.reference(real, fake, 3)
    r, rad = _dev(real), _dev(want["rad2_r"].astype(np.float32))
    for j in (0, 66):
        cnt, near = ops.manifold_count(_dev(fake[j:j + 1]), r, rad)
        assert int(cnt[0]) == want["cnt_g"][j] and float(near[0]) == want["near2_g"][j]
    cnt, near = ops.manifold_count(_dev(fake), r, None)          # no radii: only the nearest distance
    assert cnt is None and np.array_equal(near.double().cpu().numpy(), want["near2_g"])
    # the C entry point without a place for the nearest distance: only the counts (one slice and two)
    from xmc_gan_amd import lib as L
    f = _dev(fake)
    nf, nr = ops.row_sqnorm(f), ops.row_sqnorm(r)
    for slices in (1, 2):
        cnt = torch.full((67,), -1, dtype=torch.int32, device=DEV)
        ws = torch.empty((2 * 67 * 2,), dtype=torch.float32, device=DEV)
        L.call("xmc_manifold_count", ops._p(f), ops._p(nf), ops._p(r), ops._p(nr), ops._p(rad), ops._p(cnt), None, ops._p(ws), ws.numel() * 4, 67, 130,
               12, slices, ops._st())
        assert np.array_equal(cnt.cpu().numpy(), want["cnt_g"]), slices
    # a duplicate of a query among the candidates is a neighbour at distance 0; only the row itself is left out
    twice = np.concatenate([real[:5], real[:5], real[5:40]])
    rad2 = ops.knn_radius2(_dev(twice), 1).cpu().numpy()
    assert (rad2[:10] == 0).all() and np.array_equal(rad2.astype(np.float64), REF.knn_radius2(twice, 1))


def test_row_sqnorm():
    real, _ = REF.lattice()
    assert np.array_equal(ops.row_sqnorm(_dev(real)).double().cpu().numpy(), (real.astype(np.float64) ** 2).sum(1))
    for name, measured in (("gauss72", 1.163e-7), ("lowrank3", 2.287e-7)):
        x = _case(name)[0]
        e = _err(ops.row_sqnorm(_dev(x)), (x.astype(np.float64) ** 2).sum(1))
        print(f"row_sqnorm {name} {x.shape}: {e:.3e}")
        assert e <= 1.5 * measured


# ------------------------------------------------------------------------------------------ rounding band
@pytest.mark.parametrize("name", list(SETS))
def test_rounding_band(name):
    real, fake, k, want = _case(name)
    amb_g, amb_r = want["ambiguous_g"], want["ambiguous_r"]
    print(f"{name}: ambiguous rows {int(amb_g.sum())} of {amb_g.size} generated, {int(amb_r.sum())} of {amb_r.size} real")
    assert amb_g.sum() <= 0.02 * amb_g.size and amb_r.sum() <= 0.02 * amb_r.size           # a condition on the test's data, not a measurement
    got = _run(real, fake, k)
    figures = tuple(_err(got[n], want[n]) for n in ("rad2_r", "rad2_g", "near2_r", "near2_g"))
    print(f"{name}: rad2_r {figures[0]:.3e} rad2_g {figures[1]:.3e} near2_r {figures[2]:.3e} near2_g {figures[3]:.3e}")
    cnt_g, cnt_r = got["cnt_g"].cpu().numpy(), got["cnt_r"].cpu().numpy()
    assert np.array_equal(cnt_g[~amb_g], want["cnt_g"][~amb_g]) and np.array_equal(cnt_r[~amb_r], want["cnt_r"][~amb_r])
    assert ((want["cnt_g_lo"] <= cnt_g) & (cnt_g <= want["cnt_g_hi"])).all() and ((want["cnt_r_lo"] <= cnt_r) & (cnt_r <= want["cnt_r_hi"])).all()
    cov = (got["near2_r"] <= got["rad2_r"]).cpu().numpy()
    assert np.array_equal(cov[~amb_r], want["cov"][~amb_r]) and (want["cov_lo"] <= cov).all() and (cov <= want["cov_hi"]).all()
    for f, m in zip(figures, MEASURED[name]):
        assert f <= 1.5 * m, (figures, MEASURED[name])


def test_every_slice_count_gives_the_same_bytes():
    real, fake, k, _ = _case("gauss64")              # 300 / 257 rows: three 128-row chunks, so 5 and 0 are clamped to 3
    runs = {s: _run(real, fake, k, s) for s in (1, 2, 5, 0)}
    for s in (2, 5, 0):
        for name, t in runs[s].items():
            assert torch.equal(t, runs[1][name]), (s, name)
    again = _run(real, fake, k, 2)
    assert all(torch.equal(t, runs[2][n]) for n, t in again.items())


@pytest.mark.parametrize("name", ["gauss64", "lowrank5"])
def test_prdc(name):
    real, fake, k, want = _case(name)
    got = MF.prdc(_dev(real), _dev(fake), k)
    assert (got["k"], got["n_real"], got["n_fake"]) == (k, real.shape[0], fake.shape[0])
    ag, ar = int(want["ambiguous_g"].sum()), int(want["ambiguous_r"].sum())
    print(name, {m: (got[m], want[m]) for m in ("precision", "recall", "density", "coverage")}, "ambiguous", ag, ar)
    tiny = 1e-12
    assert abs(got["precision"] - want["precision"]) <= ag / fake.shape[0] + tiny
    assert abs(got["recall"] - want["recall"]) <= ar / real.shape[0] + tiny
    assert abs(got["coverage"] - want["coverage"]) <= ar / real.shape[0] + tiny
    assert abs(got["density"] - want["density"]) <= float((want["cnt_g_hi"] - want["cnt_g_lo"]).sum()) / (k * fake.shape[0]) + tiny
    bank_r, bank_g = MF.FeatureBank(real.shape[1], DEV), MF.FeatureBank(fake.shape[1], DEV)
    for i in range(0, real.shape[0], 100):
        bank_r.update(_dev(real[i:i + 100]))
    bank_g.update(_dev(fake))
    assert MF.prdc(bank_r, bank_g, k) == got
    with pytest.raises(ValueError, match="rows"):
        MF.prdc(_dev(real[:k]), _dev(fake), k)


# ------------------------------------------------------------------------------------------ the entry points
@pytest.fixture(scope="module")
def weights(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("prdc") / "inception_random.pth")
    torch.save(fid_ref.random_state_dict(7), path)
    return path


def test_eval_reports_prdc_beside_fid(weights, tmp_path):
    import xmc_gan.train_gan as tg
    from test_sample_gpu import _use_cfg, _yml
    from xmc_gan.config import gan
    try:
        cfg = _use_cfg(_yml(tmp_path))
        torch.manual_seed(2)
        netG, _, _, _ = tg.build_models(DEV)
        enc = tg.SyntheticTextEncoder(cfg.TEXT.EMBEDDING_DIM, cfg.TEXT.MAX_LENGTH, 1, DEV)
        loader = tg.SyntheticCOCO(2, 4, cfg.IMG.SIZE, cfg.TEXT.MAX_LENGTH, 1, cfg.TEXT.VOCA_SIZE)
        lines = []
        logger = logging.getLogger("prdc-eval-test")
        logger.setLevel(logging.INFO)
        handler = logging.Handler()
        handler.emit = lambda rec: lines.append(rec.getMessage())
        logger.addHandler(handler)
        rows = []
        writer = type("W", (), {"add_scalar": lambda self, tag, v, step: rows.append((tag, v, step))})()

        def run(sub, **extra):
            img = tmp_path / sub
            del lines[:], rows[:]
            torch.manual_seed(11)
            return img, tg.eval(loader=loader, state_epoch=7, text_encoder=enc, netG=netG, logger=logger, num_samples=8, save_dir=str(img / "test"),
                                org_dir=str(img / "org"), writer=writer, fid_inception=weights, **extra)[1]
        off, fid_off = run("off")
        assert lines == [f" epoch 7, FID : {fid_off}"] and rows == [("FID", fid_off, 7)] and not (off / "org_features.npz").exists()
        metrics, seen, real_prdc = {}, {}, MF.prdc
        try:                                           # the rows eval() scored
            MF.prdc = lambda r, f, k: (seen.update(real=r.rows().clone(), fake=f.rows().clone()), real_prdc(r, f, k))[1]
            on, fid_on = run("on", prdc=3, metrics=metrics)
        finally:
            MF.prdc = real_prdc
        assert fid_on == fid_off and lines[0] == f" epoch 7, FID : {fid_on}" and rows[0] == ("FID", fid_on, 7)
        m = metrics
        assert lines[1] == (f" epoch 7, precision : {m['precision']} recall : {m['recall']} density : {m['density']} coverage : {m['coverage']} "
                            f"(k=3, n=8/8)") and len(lines) == 2
        assert [r[0] for r in rows[1:]] == ["precision", "recall", "density", "coverage"] and all(r[2] == 7 for r in rows)
        assert (m["prdc_k"], m["n_real"], m["n_fake"]) == (3, 8, 8)
        assert all(0.0 <= m[n] <= 1.0 for n in ("precision", "recall", "coverage")) and m["density"] >= 0.0
        # the numbers are the reference's on the rows eval() scored, up to the rows the band leaves open
        want = REF.reference(seen["real"].cpu().numpy(), seen["fake"].cpu().numpy(), 3)
        ag, ar = int(want["ambiguous_g"].sum()), int(want["ambiguous_r"].sum())
        print({n: (m[n], want[n]) for n in ("precision", "recall", "density", "coverage")}, "ambiguous", ag, ar)
        assert abs(m["precision"] - want["precision"]) <= ag / 8 + 1e-12 and abs(m["recall"] - want["recall"]) <= ar / 8 + 1e-12
        assert abs(m["coverage"] - want["coverage"]) <= ar / 8 + 1e-12
        assert abs(m["density"] - want["density"]) <= float((want["cnt_g_hi"] - want["cnt_g_lo"]).sum()) / (3 * 8) + 1e-12
        # the cached real rows are those rows, and what the PNGs in org/ give
        cache = on / "org_features.npz"
        real = MF.FeatureBank.load(str(cache), DEV)
        assert real.n == 8 and real.dims == 2048 and torch.equal(real.rows(), seen["real"])
        from xmc_gan.utils.visual import fid_extractor
        again = MF.bank_of_dir(str(on / "org"), fid_extractor(weights, DEV))
        assert float((again.rows() - real.rows()).abs().max()) <= 1e-4 * float(real.rows().abs().max())
        # a second call reuses the rows: the file is not written again
        before = os.stat(cache).st_mtime_ns
        metrics2 = {}
        torch.manual_seed(11)
        tg.eval(loader=loader, state_epoch=7, text_encoder=enc, netG=netG, logger=logger, num_samples=8, save_dir=str(on / "test"),
                org_dir=str(on / "org"), writer=writer, fid_inception=weights, prdc=3, metrics=metrics2)
        assert os.stat(cache).st_mtime_ns == before and metrics2 == metrics
        # without the Inception weights: one line says why
        del lines[:]
        os.environ.pop("XMC_FID_INCEPTION", None)
        tg.eval(loader=loader, state_epoch=7, text_encoder=enc, netG=netG, logger=logger, num_samples=8, prdc=3)
        assert sum("precision / recall / density / coverage not computed" in ln for ln in lines) == 1
    finally:
        gan.reset_cfg()
        ops.set_precision("bf16")


def test_sample_writes_prdc_into_the_manifest(weights, tmp_path):
    import xmc_gan.sample as sample
    import xmc_gan.train_gan as tg
    from test_sample_gpu import _use_cfg, _yml
    from xmc_gan.config import gan
    try:
        yml = _yml(tmp_path)
        _use_cfg(yml)
        torch.manual_seed(4)
        torch.save(tg.build_models(DEV)[0].state_dict(), tmp_path / "netG.pth")
        gan.reset_cfg()
        g = np.random.default_rng(0)
        against = str(tmp_path / "against.npz")
        MF.save_features(against, np.abs(g.standard_normal((12, 2048))))
        base = ["--cfg", yml, "--checkpoint", str(tmp_path / "netG.pth"), "--out", str(tmp_path / "out"), "--synthetic", "5", "--grid_max", "0"]
        man = sample.main(base + ["--prdc_against", against, "--prdc_k", "2", "--fid_inception", weights])
        assert sorted(man["prdc"]) == ["coverage", "density", "k", "n_fake", "n_real", "precision", "recall"]
        assert (man["prdc"]["k"], man["prdc"]["n_real"], man["prdc"]["n_fake"]) == (2, 12, 5) and man["fid"] is None
        assert "prdc" not in sample.main(base)
        with pytest.raises(SystemExit, match="prdc_against"):       # five sampled images have no 6th neighbour
            sample.main(base + ["--prdc_against", against, "--prdc_k", "5", "--fid_inception", weights])
    finally:
        gan.reset_cfg()
        ops.set_precision("bf16")
