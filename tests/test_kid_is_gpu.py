"""KID and the Inception Score on the GPU (csrc/kid.hip, xmc_gan_amd/manifold.py `kid`, xmc_gan_amd/fid.py `InceptionScore`) against the f64
restatement in tests/kid_ref.py.

On lattices whose kernel values are float32 numbers (kid_ref.assert_exact_in_f32 shows that from the data) every product and sum of the
kernel is exact, so the three sums must EQUAL the reference bit for bit.  On real-valued rows the error figure of a sum is |got - want| /
want (every element is >= 1, so the sums are positive); every bar is 1.5 x the figure measured on the MI355X, written beside it, under the
hard ceiling (D + 8) * 2^-24 of an f32 fma chain over D.  The Inception Score kernel is f64 throughout: each part's score agrees to 1e-10.
The shapes straddle the 32 / 128-row tiles and the 32-column stage of D."""
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
import kid_ref as REF
import manifold_ref
from xmc_gan_amd import fid as FID
from xmc_gan_amd import manifold as MF
from xmc_gan_amd import ops

DEV = torch.device("cuda", 0)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _tables(nr, nf, m, s, seed):
    """unsorted index tables that share rows across subsets"""
    g = np.random.default_rng(seed)
    return (np.stack([g.permutation(nr)[:m] for _ in range(s)]).astype(np.int32),
            np.stack([g.permutation(nf)[:m] for _ in range(s)]).astype(np.int32))


def _sums(real, fake, ir, jf):
    out = ops.poly_mmd_sums(_dev(real), _dev(fake), torch.from_numpy(ir), torch.from_numpy(jf))
    assert out.dtype == torch.float64 and tuple(out.shape) == (ir.shape[0], 3)
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------ exact lattices
LATTICES = [(4, 4, 2, 1, 4, 4), (4, 4, 2, 1, 8, 4), (40, 35, 33, 3, 16, 4), (40, 35, 33, 3, 32, 4), (300, 257, 130, 3, 8, 4),
            (300, 257, 130, 3, 32, 4), (300, 257, 129, 7, 64, 2), (300, 257, 130, 3, 128, 2)]


@pytest.mark.parametrize("nr,nf,m,s,d,levels", LATTICES)
def test_lattice_sums_equal_the_reference(nr, nf, m, s, d, levels):
    g = np.random.default_rng(nr + m + d)
    real, fake = g.integers(0, levels, (nr, d)).astype(np.float32), g.integers(0, levels, (nf, d)).astype(np.float32)
    REF.assert_exact_in_f32(real, fake)
    ir, jf = _tables(nr, nf, m, s, d)
    assert s == 1 or len(np.intersect1d(ir[0], ir[1])) > 0                       # subsets share rows
    want = REF.poly_mmd_sums(real, fake, ir, jf)
    got = _sums(real, fake, ir, jf)
    assert np.array_equal(got, want), (got, want)


def test_identical_rows_in_a_subset_are_a_pair():
    """exclusion is by position: two positions that hold the same values (and two that name the same bank row) count"""
    g = np.random.default_rng(5)
    real, fake = g.integers(0, 4, (40, 16)).astype(np.float32), g.integers(0, 4, (35, 16)).astype(np.float32)
    real[7] = real[3]                                                            # two identical bank rows ...
    REF.assert_exact_in_f32(real, fake)
    ir, jf = _tables(40, 35, 33, 2, 1)
    ir[0, 5], ir[0, 20] = 3, 7                                                   # ... in the same subset
    ir[0] = np.where((np.arange(33) != 5) & (np.arange(33) != 20) & np.isin(ir[0], (3, 7)), 11, ir[0])
    ir[1, 2] = ir[1, 30]                                                         # and one bank row at two positions
    want = REF.poly_mmd_sums(real, fake, ir, jf)
    assert np.array_equal(want, REF.poly_mmd_sums_loop(real, fake, ir, jf))
    k37 = float(REF.kernel(real[3:4], real[7:8])[0, 0])
    dedup = REF.poly_mmd_sums(real, fake, np.delete(ir[:1], 20, axis=1), np.delete(jf[:1], 20, axis=1))
    assert want[0, 0] > dedup[0, 0] + 2 * k37 - 1e-9                             # the pair (5, 20) is in the sum, both ways
    assert np.array_equal(_sums(real, fake, ir, jf), want)


# ------------------------------------------------------------------------------------------ real-valued rows
REAL_SETS = {"gauss72": (manifold_ref.gaussian, (300, 257, 72, 2)), "lowrank2048": (manifold_ref.lowrank, (300, 257, 2048, 5))}
# measured on the MI355X: |got - want| / want of (XX, YY, XY), the largest over the three subsets
MEASURED = {"gauss72": (1.060e-09, 1.106e-09, 1.209e-09), "lowrank2048": (3.674e-09, 9.851e-10, 3.369e-09)}
# (a sum of 16 900 elements whose rounding errors, ~1e-7 each, have both signs: the sum is far more accurate than an element)


@functools.lru_cache(maxsize=None)
def _real_case(name):
    """(real, fake, index tables, the reference sums): built once, shared, never modified"""
    make, args = REAL_SETS[name]
    real, fake = (np.abs(x) for x in make(*args))
    ir, jf = _tables(real.shape[0], fake.shape[0], 130, 3, 17)
    x = np.concatenate([real, fake]).astype(np.float64)
    assert (REF.kernel(x, x) >= 1.0).all()                                       # non-negative rows: every element is >= 1
    return real, fake, ir, jf, REF.poly_mmd_sums(real, fake, ir, jf)


def _bar(name):
    d = REAL_SETS[name][1][2]
    ceiling = (d + 8) * 2.0 ** -24
    return [ceiling if m is None else min(1.5 * m, ceiling) for m in MEASURED[name]], ceiling


@pytest.mark.parametrize("name", list(REAL_SETS))
def test_real_valued_sums(name):
    real, fake, ir, jf, want = _real_case(name)
    got = _sums(real, fake, ir, jf)
    figures = (np.abs(got - want) / want).max(axis=0)
    print(f"{name}: XX {figures[0]:.3e} YY {figures[1]:.3e} XY {figures[2]:.3e}")
    bars, ceiling = _bar(name)
    assert (got > 0).all() and all(f <= b for f, b in zip(figures, bars)), (figures, bars, ceiling)
    assert np.array_equal(_sums(real, fake, ir, jf), got)                       # two runs, equal bytes


@pytest.mark.parametrize("name", list(REAL_SETS))
def test_kid_value_and_determinism(name):
    real, fake, _, _, _ = _real_case(name)
    got = MF.kid(_dev(real), _dev(fake), subsets=3, subset_size=130, seed=4)
    assert (got["subsets"], got["subset_size"], got["n_real"], got["n_fake"]) == (3, 130, 300, 257)
    ir, jf = REF.subsets(300, 257, 3, 130, 4)
    assert np.array_equal(ir, MF.kid_subsets(300, 257, 3, 130, 4)[0]) and np.array_equal(jf, MF.kid_subsets(300, 257, 3, 130, 4)[1])
    sums = REF.poly_mmd_sums(real, fake, ir, jf)
    want, spread = REF.kid(real, fake, ir, jf)
    m = 130
    scale = (sums[:, 0].mean() + sums[:, 1].mean()) / (m * (m - 1.0)) + 2 * sums[:, 2].mean() / (m * m)     # mean XX + mean YY + 2 mean XY
    bar = max(_bar(name)[0])
    print(f"{name}: kid {got['kid']:.9e} want {want:.9e} (+- {spread:.3e}); |diff| / scale = {abs(got['kid'] - want) / scale:.3e}, bar {bar:.3e}")
    assert abs(got["kid"] - want) <= bar * scale and abs(got["std"] - spread) <= 2 * bar * scale
    bank_r, bank_g = MF.FeatureBank(real.shape[1], DEV), MF.FeatureBank(fake.shape[1], DEV)
    for i in range(0, 300, 100):
        bank_r.update(_dev(real[i:i + 100]))
        bank_g.update(_dev(fake[i:i + 100]))
    assert MF.kid(bank_r, bank_g, subsets=3, subset_size=130, seed=4) == got
    small = MF.kid(_dev(real[:5]), _dev(fake), subsets=2, subset_size=130)
    assert small["subset_size"] == 5
    with pytest.raises(ValueError, match="two rows"):
        MF.kid(_dev(real[:1]), _dev(fake))


def test_bad_index_is_refused_on_the_host():
    real, fake = _dev(np.ones((6, 8), np.float32)), _dev(np.ones((5, 8), np.float32))
    ok = torch.zeros((2, 3), dtype=torch.int32)
    from xmc_gan_amd import lib as L
    launched = []
    real_call = L.call
    try:
        L.call = lambda name, *a: (launched.append(name), real_call(name, *a))[1]
        for bad, side in ((6, 0), (-1, 0), (5, 1), (-1, 1)):
            tab = ok.clone()
            tab[1, 2] = bad
            with pytest.raises(ValueError, match="indices span"):
                ops.poly_mmd_sums(real, fake, *((tab, ok) if side == 0 else (ok, tab)))
        with pytest.raises(ValueError):
            ops.poly_mmd_sums(real, fake, ok[:, :1], ok[:, :1])                  # m < 2
        assert launched == []
        ops.poly_mmd_sums(real, fake, ok, ok)
        assert launched == ["xmc_poly_mmd_sums"]
    finally:
        L.call = real_call


# ------------------------------------------------------------------------------------------ inception score
def _scores(logits, splits, classes=None):
    n = logits.shape[0]
    H, P = ops.inception_score_sums(logits, splits, classes)
    assert H.dtype == torch.float64 and tuple(P.shape) == (splits, classes or logits.shape[1])
    return FID.is_from_sums(H.cpu().numpy(), P.cpu().numpy(), n, splits)


@pytest.mark.parametrize("n,c,splits", [(1, 5, 1), (10, 1008, 10), (23, 1008, 10), (130, 65, 3), (257, 1008, 10)])
def test_inception_score_kernel(n, c, splits):
    g = np.random.default_rng(n + c)
    logits = (3.0 * g.standard_normal((n, c))).astype(np.float32)
    if n == 130:                                                                  # the overflow guard
        logits[::7, 3], logits[::5, 11], logits[4, :] = 80.0, -80.0, 80.0
    want_mean, want_std, want = REF.inception_score(logits, splits)
    mean, std, got = _scores(_dev(logits), splits)
    err = float(np.abs(got / want - 1.0).max())
    print(f"IS kernel {n}x{c}/{splits}: {mean:.12f} +- {std:.3e}, max relative error of a part {err:.3e}")
    assert err <= 1e-10 and abs(mean / want_mean - 1.0) <= 1e-10 and abs(std - want_std) <= 1e-10 * want_mean
    assert np.array_equal(_scores(_dev(logits), splits)[2], got)
    if n == 257:                                                                  # a row stride of 1024 with garbage in the padding
        padded = np.full((n, 1024), 1e30, np.float32)
        padded[:, 16:] = np.nan
        padded[:, :c] = logits
        assert np.array_equal(_scores(_dev(padded), splits, classes=c)[2], got)
        assert np.array_equal(_scores(_dev(padded)[:, :c], splits)[2], got)     # a view with the stride of the padded rows


def test_inception_score_closed_forms():
    mean, std, _ = _scores(torch.zeros((40, 1008), device=DEV), 4)
    assert abs(mean - 1.0) <= 1e-12 and std <= 1e-12
    c, n = 7, 70
    logits = np.zeros((n, c), np.float32)
    logits[np.arange(n), np.arange(n) % c] = 80.0
    mean, _, parts = _scores(_dev(logits), 2)
    assert abs(mean - c) <= 1e-9 * c and np.abs(parts - c).max() <= 1e-9 * c
    with pytest.raises(ValueError):
        ops.inception_score_sums(torch.zeros((3, 8), device=DEV), 4)             # fewer rows than splits


# ------------------------------------------------------------------------------------------ the logits
@pytest.fixture(scope="module")
def weights(tmp_path_factory):
    """(a weights file with the all-zero fc.weight of fid_ref.random_state_dict, one with a seeded random fc.weight, that weight)"""
    d = tmp_path_factory.mktemp("kid_is")
    sd = fid_ref.random_state_dict(7)
    torch.save(sd, str(d / "zero_fc.pth"))
    fc = (torch.randn((1008, 2048), generator=torch.Generator().manual_seed(3)) / 45.0).float()
    torch.save(dict(sd, **{"fc.weight": fc}), str(d / "random_fc.pth"))
    return str(d / "zero_fc.pth"), str(d / "random_fc.pth"), fc


LOGITS_MEASURED = 7.555e-06        # measured on the MI355X: max |got - want| over the rms of want


def test_logits_against_f64_matmul(weights):
    zero, rand, fc = weights
    g = np.random.default_rng(2)
    feats = np.abs(g.standard_normal((37, 2048))).astype(np.float32)
    net = FID.InceptionFID(rand, DEV)
    got = net.logits(_dev(feats))
    assert got.dtype == torch.float32 and tuple(got.shape) == (37, 1008)
    want = feats.astype(np.float64) @ fc.double().numpy().T
    err = float(np.abs(got.double().cpu().numpy() - want).max() / np.sqrt((want ** 2).mean()))
    print(f"InceptionFID.logits 37 x 2048 -> 1008: {err:.3e}")
    assert err <= (1e-4 if LOGITS_MEASURED is None else min(1.5 * LOGITS_MEASURED, 1e-4))
    acc = FID.InceptionScore(net, splits=3)
    for i in range(0, 37, 10):
        acc.update(_dev(feats[i:i + 10]))
    out = acc.finalize()
    want_mean, want_std, _ = REF.inception_score(got.cpu().numpy(), 3)
    assert (out["splits"], out["n"]) == (3, 37) and abs(out["inception_score"] / want_mean - 1) <= 1e-10 and abs(out["std"] - want_std) <= 1e-10
    flat = FID.InceptionScore(FID.InceptionFID(zero, DEV), splits=2)
    flat.update(_dev(feats))
    assert abs(flat.finalize()["inception_score"] - 1.0) <= 1e-12
    with pytest.raises(ValueError, match="splits"):
        FID.InceptionScore(net, splits=50).finalize()


# ------------------------------------------------------------------------------------------ the entry points
def _eval_harness(tmp_path, name):
    import xmc_gan.train_gan as tg
    from test_sample_gpu import _use_cfg, _yml
    cfg = _use_cfg(_yml(tmp_path))
    torch.manual_seed(2)
    netG, _, _, _ = tg.build_models(DEV)
    enc = tg.SyntheticTextEncoder(cfg.TEXT.EMBEDDING_DIM, cfg.TEXT.MAX_LENGTH, 1, DEV)
    loader = tg.SyntheticCOCO(2, 4, cfg.IMG.SIZE, cfg.TEXT.MAX_LENGTH, 1, cfg.TEXT.VOCA_SIZE)
    lines, rows = [], []
    logger = logging.getLogger(name)
    logger.setLevel(logging.INFO)
    handler = logging.Handler()
    handler.emit = lambda rec: lines.append(rec.getMessage())
    logger.addHandler(handler)
    writer = type("W", (), {"add_scalar": lambda self, tag, v, step: rows.append((tag, v, step))})()

    def run(sub, **extra):
        img = tmp_path / sub
        del lines[:], rows[:]
        torch.manual_seed(11)
        dirs = dict(save_dir=str(img / "test"), org_dir=str(img / "org")) if sub else {}
        return img, tg.eval(loader=loader, state_epoch=7, text_encoder=enc, netG=netG, logger=logger, num_samples=8, writer=writer, **dirs, **extra)[1]
    return run, lines, rows


# measured on the MI355X: |kid - want| / (mean XX + mean YY + 2 mean XY) on the 8 + 8 rows eval() scores here (100 subsets of m = 8: 56 + 56 + 64
# elements per subset, so far fewer rounding errors average out than in the 130-row cases above)
EVAL_KID_MEASURED = 6.947e-08


def test_eval_reports_kid_and_is(weights, tmp_path):
    from xmc_gan.config import gan
    zero, rand, fc = weights
    try:
        run, lines, rows = _eval_harness(tmp_path, "kid-is-eval-test")
        off, fid_off = run("off", fid_inception=rand)
        off_lines, off_rows = list(lines), list(rows)
        assert off_lines == [f" epoch 7, FID : {fid_off}"] and not (off / "org_features.npz").exists()
        metrics, seen, real_kid = {}, {}, MF.kid
        try:                                           # the rows eval() scored
            MF.kid = lambda r, f, *a: (seen.update(real=r.rows().clone(), fake=f.rows().clone()), real_kid(r, f, *a))[1]
            on, fid_on = run("on", fid_inception=rand, kid=True, inception_score=2, metrics=metrics)
        finally:
            MF.kid = real_kid
        m = metrics
        assert fid_on == fid_off and lines[:1] == off_lines and rows[:1] == off_rows and len(lines) == 3
        assert lines[1] == f" epoch 7, KID : {m['kid']} +- {m['kid_std']} (subsets=100, size=8, n=8/8)"
        assert lines[2] == f" epoch 7, IS : {m['inception_score']} +- {m['inception_score_std']} (splits=2, n=8)"
        assert rows[1:] == [("KID", m["kid"], 7), ("IS", m["inception_score"], 7)]
        assert (m["kid_subsets"], m["kid_subset_size"], m["kid_n_real"], m["kid_n_fake"], m["inception_score_splits"], m["inception_score_n"]) == (100, 8, 8, 8, 2, 8)
        # the values are the reference's on the rows eval() scored
        real, fake = seen["real"].cpu().numpy(), seen["fake"].cpu().numpy()
        ir, jf = REF.subsets(8, 8, 100, 1000, 0)
        sums = REF.poly_mmd_sums(real, fake, ir, jf)
        want, spread = REF.kid(real, fake, ir, jf)
        scale = (sums[:, 0].mean() + sums[:, 1].mean()) / 56.0 + 2 * sums[:, 2].mean() / 64.0
        bar = min(1.5 * EVAL_KID_MEASURED, (2048 + 8) * 2.0 ** -24)
        print(f"eval KID {m['kid']:.9e} want {want:.9e}: |diff| / scale {abs(m['kid'] - want) / scale:.3e}, bar {bar:.3e}")
        assert abs(m["kid"] - want) <= bar * scale and abs(m["kid_std"] - spread) <= 2 * bar * scale
        logits = seen["fake"].double().cpu().numpy() @ fc.double().numpy().T
        want_is = REF.inception_score(logits, 2)
        print(f"eval IS {m['inception_score']:.9f} want {want_is[0]:.9f}")
        assert abs(m["inception_score"] / want_is[0] - 1.0) <= 1e-4               # (the logits' f32 GEMM, bar 1e-4 of their rms, is what differs)
        # the real rows are cached once, beside org/, and a second call does not write them again
        cache = on / "org_features.npz"
        assert MF.FeatureBank.load(str(cache), DEV).n == 8 and torch.equal(MF.FeatureBank.load(str(cache), DEV).rows(), seen["real"])
        before = os.stat(cache).st_mtime_ns
        metrics2 = {}
        _, fid2 = run("on", fid_inception=rand, kid=True, inception_score=2, metrics=metrics2)
        assert os.stat(cache).st_mtime_ns == before and metrics2 == metrics and fid2 == fid_on
    finally:
        gan.reset_cfg()
        ops.set_precision("bf16")


def test_eval_kid_beside_prdc_and_without_weights(weights, tmp_path):
    from xmc_gan.config import gan
    zero, rand, fc = weights
    try:
        run, lines, rows = _eval_harness(tmp_path, "kid-prdc-eval-test")
        # KID beside PRDC: one file, both lines
        both, _ = run("both", fid_inception=rand, kid=True, prdc=3, kid_subsets=5)
        assert len(lines) == 3 and lines[1].startswith(" epoch 7, precision : ") and lines[2].startswith(" epoch 7, KID : ")
        assert "(subsets=5, size=8, n=8/8)" in lines[2] and sorted(f for f in os.listdir(both) if f.endswith(".npz")) == ["org_features.npz", "org_stats.npz"]
        # without Inception weights: one reason line each
        os.environ.pop("XMC_FID_INCEPTION", None)
        run("", kid=True, inception_score=2)
        assert sum(ln.startswith(" epoch 7, KID not computed: ") for ln in lines) == 1
        assert sum(ln.startswith(" epoch 7, IS not computed: ") for ln in lines) == 1
    finally:
        gan.reset_cfg()
        ops.set_precision("bf16")


def test_sample_and_the_command_lines(weights, tmp_path, capsys):
    import xmc_gan.inception_score as is_cli
    import xmc_gan.kid as kid_cli
    import xmc_gan.sample as sample
    import xmc_gan.train_gan as tg
    from test_sample_gpu import _use_cfg, _yml
    from xmc_gan.config import gan
    zero, rand, fc = weights
    try:
        yml = _yml(tmp_path)
        _use_cfg(yml)
        torch.manual_seed(4)
        torch.save(tg.build_models(DEV)[0].state_dict(), tmp_path / "netG.pth")
        gan.reset_cfg()
        g = np.random.default_rng(0)
        against = str(tmp_path / "against.npz")
        MF.save_features(against, np.abs(g.standard_normal((12, 2048))))
        out = str(tmp_path / "out")
        # (--bs 8: the five images are one batch, as they are when the directory is read back below)
        base = ["--cfg", yml, "--checkpoint", str(tmp_path / "netG.pth"), "--out", out, "--synthetic", "5", "--grid_max", "0", "--bs", "8"]
        seen, real_kid = {}, MF.kid
        try:                                           # the rows and the arguments sample.py scored with
            MF.kid = lambda r, f, *a: (seen.update(fake=f.rows().clone(), args=a), real_kid(r, f, *a))[1]
            man = sample.main(base + ["--kid_against", against, "--kid_subsets", "4", "--inception_score", "--is_splits", "2", "--fid_inception", rand])
        finally:
            MF.kid = real_kid
        assert seen["args"] == (4, 1000, 100)          # --kid_subsets, the default size, and sample.py's --seed (default 100) for the draw
        assert sorted(man["kid"]) == ["kid", "n_fake", "n_real", "std", "subset_size", "subsets"]
        assert (man["kid"]["subsets"], man["kid"]["subset_size"], man["kid"]["n_real"], man["kid"]["n_fake"]) == (4, 5, 12, 5)
        assert sorted(man["inception_score"]) == ["inception_score", "n", "splits", "std"] and man["inception_score"]["n"] == 5 and man["fid"] is None
        plain = sample.main(base)
        assert "kid" not in plain and "inception_score" not in plain
        # the command lines on the PNGs sample.py wrote: the library's values on the same rows
        extractor = FID.InceptionFID(rand, DEV)
        bank = MF.bank_of_dir(out, extractor)
        real = MF.FeatureBank.load(against, DEV)
        assert bank.n == 5 and torch.equal(bank.rows(), seen["fake"])            # the PNGs hold the bytes that were scored on the device
        # the manifest's values are the library's on those rows, with sample.py's seed for the draw
        assert man["kid"] == MF.kid(real, bank, 4, 1000, 100)
        acc = FID.InceptionScore(extractor, 2)
        acc.update(bank.rows())
        assert man["inception_score"] == acc.finalize()
        # the command lines: the same values again (xmc_gan/kid.py draws with seed 0 unless told otherwise)
        feats = str(tmp_path / "real_again.npz")
        got = kid_cli.main([against, out, "--inception", rand, "--subsets", "4", "--seed", "100", "--save_features", feats])
        assert got == man["kid"] and "KID: " in capsys.readouterr().out
        assert np.array_equal(MF.load_features(feats), MF.load_features(against))
        assert kid_cli.main([against, out, "--inception", rand, "--subsets", "4"]) == MF.kid(real, bank, 4, 1000, 0)
        got = is_cli.main([out, "--inception", rand, "--splits", "2"])
        assert got == man["inception_score"] and "IS: " in capsys.readouterr().out
        with pytest.raises(SystemExit, match="fc.weight"):
            noclass = str(tmp_path / "noclass.pth")
            torch.save({k: v for k, v in fid_ref.random_state_dict(7).items() if not k.startswith("fc.")}, noclass)
            is_cli.main([out, "--inception", noclass, "--splits", "2"])
        with pytest.raises(SystemExit, match="inception_score"):
            sample.main(base + ["--inception_score", "--fid_inception", noclass])
        with pytest.raises(SystemExit, match="kid_against"):
            sample.main(base + ["--kid_against", str(tmp_path / "nowhere"), "--fid_inception", rand])
        with pytest.raises(SystemExit, match="fewer than --splits"):
            is_cli.main([out, "--inception", rand, "--splits", "9"])
    finally:
        gan.reset_cfg()
        ops.set_precision("bf16")
