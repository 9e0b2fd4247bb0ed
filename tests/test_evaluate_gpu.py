"""The evaluation pipeline on the GPU (xmc_gan_amd/evaluate.py under xmc_gan/train_gan.py eval()): FID, precision / recall / density / coverage
and R-precision out of one pass give the numbers each gives alone, every batch is converted, Inception-encoded and DAMSM-encoded once, a
second evaluation reuses the cached real side, and a training run leaves nothing behind that a later eval() would pick up."""
import logging
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import damsm_ref
import fid_ref
from xmc_gan.model.encoder import CNN_ENCODER, RNN_ENCODER
from xmc_gan_amd import fid as FID
from xmc_gan_amd import ops

DEV = torch.device("cuda", 0)
PRDC_KEYS = ("precision", "recall", "density", "coverage", "prdc_k", "n_real", "n_fake")
RP_KEYS = ("r_precision", "std", "n", "k", "splits", "per_split")


@pytest.fixture(scope="module")
def weights(tmp_path_factory):
    """(random FID Inception weights, random weights of a 256-wide DAMSM image encoder), as files"""
    d = tmp_path_factory.mktemp("evaluate")
    inception, damsm = str(d / "inception_random.pth"), str(d / "image_encoder_random.pth")
    torch.save(fid_ref.random_state_dict(7), inception)
    torch.save(damsm_ref.random_state_dict(11, 256), damsm)
    return inception, damsm


@pytest.fixture
def no_env(monkeypatch):
    monkeypatch.delenv("XMC_FID_INCEPTION", raising=False)
    monkeypatch.delenv("XMC_DAMSM_IMAGE_ENCODER", raising=False)


@pytest.fixture
def counts(monkeypatch):
    """how often a batch was converted to uint8, went through the Inception extractor, went through the DAMSM image encoder"""
    n = dict(u8=0, inception=0, damsm=0)

    def counted(fn, key):
        def wrapper(*a, **k):
            n[key] += 1
            return fn(*a, **k)
        return wrapper
    monkeypatch.setattr(FID, "nchw_to_u8", counted(FID.nchw_to_u8, "u8"))
    monkeypatch.setattr(FID.InceptionFID, "__call__", counted(FID.InceptionFID.__call__, "inception"))
    monkeypatch.setattr(CNN_ENCODER, "encode_u8", counted(CNN_ENCODER.encode_u8, "damsm"))
    return n


class _Run:
    """eval() on 13 distinct synthetic batches of 8 (k = 100 needs 99 captions of other images), its lines and scalar rows kept"""

    def __init__(self, tmp_path, weights):
        import xmc_gan.train_gan as tg
        from test_sample_gpu import _use_cfg, _yml
        from xmc_gan_amd.evaluate import load_model
        self.tg, cfg = tg, _use_cfg(_yml(tmp_path))
        for kind, path in zip(("inception", "damsm"), weights):       # loaded before any run is seeded: constructing CNN_ENCODER draws its
            load_model(kind, path, DEV)                               # initial weights from torch's generator, which the noise comes from
        torch.manual_seed(2)
        self.netG = tg.build_models(DEV)[0]
        self.text = RNN_ENCODER(cfg).to(DEV).eval()
        self.loader = tg.SyntheticCOCO(13, 8, cfg.IMG.SIZE, cfg.TEXT.MAX_LENGTH, 1, cfg.TEXT.VOCA_SIZE, distinct=13)
        self.lines, self.rows = [], []
        self.logger = logging.getLogger("evaluate-test")
        self.logger.setLevel(logging.INFO)
        handler = logging.Handler()
        handler.emit = lambda rec: self.lines.append(rec.getMessage())
        self.logger.handlers[:] = [handler]
        self.writer = type("W", (), {"add_scalar": lambda _, tag, v, step: self.rows.append((tag, v, step))})()

    def __call__(self, **kw):
        del self.lines[:], self.rows[:]
        metrics = {}
        torch.manual_seed(11)
        fid = self.tg.eval(loader=self.loader, state_epoch=7, text_encoder=self.text, netG=self.netG, logger=self.logger, num_samples=104,
                           writer=self.writer, metrics=metrics, **kw)[1]
        return fid, metrics


def test_all_metrics_in_one_pass(weights, no_env, counts, tmp_path):
    from xmc_gan.config import gan
    inception, damsm = weights
    try:
        run = _Run(tmp_path, weights)
        fid, m = run(fid_inception=inception, prdc=3, damsm_image_encoder=damsm)
        # one conversion and one Inception pass per generated and per real batch, one DAMSM pass per generated batch: nothing twice
        assert counts == dict(u8=26, inception=26, damsm=13)
        lines, rows = list(run.lines), list(run.rows)
        assert len(lines) == 3 and lines[0] == f" epoch 7, FID : {fid}"
        assert lines[1] == (f" epoch 7, precision : {m['precision']} recall : {m['recall']} density : {m['density']} coverage : {m['coverage']} "
                            f"(k=3, n=104/104)")
        assert lines[2] == f" epoch 7, R-precision : {m['r_precision']} +- {m['std']} (k=100, n=104)"
        assert [r[0] for r in rows] == ["FID", "precision", "recall", "density", "coverage", "R_precision"] and all(r[2] == 7 for r in rows)
        assert [r[1] for r in rows] == [fid, m["precision"], m["recall"], m["density"], m["coverage"], m["r_precision"]]
        assert set(m) == set(PRDC_KEYS + RP_KEYS) and (m["prdc_k"], m["n_real"], m["n_fake"], m["n"], m["k"]) == (3, 104, 104, 104, 100)
        # the numbers are those of FID and PRDC alone, and of R-precision alone
        fid_a, m_a = run(fid_inception=inception, prdc=3)
        assert fid_a == fid and m_a == {k: m[k] for k in PRDC_KEYS} and run.lines == lines[:2] and run.rows == rows[:5]
        fid_b, m_b = run(damsm_image_encoder=damsm)
        assert fid_b is None and m_b == {k: m[k] for k in RP_KEYS} and run.lines[-1] == lines[2] and run.rows == rows[5:]
    finally:
        gan.reset_cfg()
        ops.set_precision("bf16")


def test_a_second_evaluation_reuses_the_real_side(weights, no_env, counts, tmp_path):
    from xmc_gan.config import gan
    inception, damsm = weights
    try:
        run = _Run(tmp_path, weights)
        org = tmp_path / "img" / "org"
        kw = dict(fid_inception=inception, prdc=3, damsm_image_encoder=damsm, org_dir=str(org))
        fid, m = run(**kw)
        assert counts == dict(u8=26, inception=26, damsm=13) and len(os.listdir(org)) == 104
        caches = [tmp_path / "img" / "org_stats.npz", tmp_path / "img" / "org_features.npz"]
        before = [os.stat(c).st_mtime_ns for c in caches]
        counts.update(u8=0, inception=0, damsm=0)
        fid2, m2 = run(**kw)
        assert counts == dict(u8=13, inception=13, damsm=13)          # the generated batches only: no real image is extracted again
        assert [os.stat(c).st_mtime_ns for c in caches] == before
        assert fid2 == fid and m2 == m
    finally:
        gan.reset_cfg()
        ops.set_precision("bf16")


def test_a_training_run_leaves_no_evaluation_settings_behind(weights, no_env, tmp_path):
    """main(--prdc 3 --fid_inception W) followed by a plain eval(fid_inception=W): FID alone.  (With the settings kept in module-level
    lists, as they were, the eval() also logged precision / recall / density / coverage and wrote org_features.npz.)"""
    import xmc_gan.train_gan as tg
    from test_sample_gpu import _yml
    from xmc_gan.config import gan
    inception, _ = weights
    try:
        tg.main(["--cfg", _yml(tmp_path), "--synthetic", "2", "--max_epoch", "1", "--graph", "0", "--prdc", "3", "--fid_inception", inception,
                 "--imsize", "64", "--bs", "4", "--output_dir", str(tmp_path / "run")])
        cfg = gan.cfg
        netG = tg.main.last_models[0]
        enc = tg.SyntheticTextEncoder(cfg.TEXT.EMBEDDING_DIM, cfg.TEXT.MAX_LENGTH, 1, DEV)
        loader = tg.SyntheticCOCO(2, 4, cfg.IMG.SIZE, cfg.TEXT.MAX_LENGTH, 1, cfg.TEXT.VOCA_SIZE)
        lines = []
        logger = logging.getLogger("evaluate-state-test")
        logger.setLevel(logging.INFO)
        handler = logging.Handler()
        handler.emit = lambda rec: lines.append(rec.getMessage())
        logger.handlers[:] = [handler]
        logger.propagate = False
        img = tmp_path / "img"
        _, fid = tg.eval(loader=loader, state_epoch=7, text_encoder=enc, netG=netG, logger=logger, num_samples=8, save_dir=str(img / "test"),
                         org_dir=str(img / "org"), fid_inception=inception)
        assert lines == [f" epoch 7, FID : {fid}"]
        assert (img / "org_stats.npz").is_file() and not (img / "org_features.npz").exists()
    finally:
        gan.reset_cfg()
        ops.set_precision("bf16")
