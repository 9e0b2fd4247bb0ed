"""The caption-embedding cache on the GPU: `ops.caption_gather` (csrc/captionfeed.hip) bit for bit against its numpy restatement
(tests/caption_ref.py), `CachedTextEncoder.forward_keys` bit for bit against the live encoders over two epochs of a `DeviceImageLoader`, a
cache built at another batch size against the f64 restatement of the sentence encoder, and ``train_gan.py --caption_cache`` end to end on a
miniature COCO-layout tree.  Nothing outside the repository is read; no worker process is started."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]

import caption_ref as R  # noqa: E402
import datafeed_ref as DR  # noqa: E402
import sbert_ref as SR  # noqa: E402
from golden_util import CFG_DIR  # noqa: E402

DEV = torch.device("cuda", 0)
N = 7


@pytest.fixture(autouse=True)
def _restore():
    yield
    from xmc_gan.config import gan
    from xmc_gan_amd import ops
    ops.set_precision("bf16")
    gan.reset_cfg()


# ------------------------------------------------------------------------------------------------------------------------ the kernel
_tables = {}


def _case(E, T):
    """the device tables of (E, T) and the host arrays they were made from, built once"""
    if (E, T) not in _tables:
        lens = R.kernel_lens(T)
        sent, tok, off = R.tables(lens, E, seed=E + T)
        _tables[(E, T)] = dict(host=(sent, tok, off, lens), dev=tuple(torch.from_numpy(x).to(DEV) for x in (sent, tok, off, lens)))
    return _tables[(E, T)]


def _prefilled(B, E, T):
    return (torch.full((B, E, T), float("nan"), device=DEV), torch.full((B, E), float("nan"), device=DEV), torch.ones((B, T), dtype=torch.bool, device=DEV))


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("T", [5, 20, 64])
@pytest.mark.parametrize("E", [8, 72, 128])
def test_kernel_equals_the_restatement_bit_for_bit(E, T, B):
    """E = 8: narrower than a 64-channel chunk; 72: a chunk and a partial one; 128: two chunks.  T = 5: T % 4 != 0; 64: the limit.  Lengths
    (1, T, 3, T-1, 2, T, 1); the outputs are pre-filled with NaN / True, so an element the kernel does not write shows."""
    from xmc_gan_amd import ops
    c = _case(E, T)
    for rows in ([[N - 1], [0]] if B == 1 else [[0, N - 1, 3, 3, 1]]):               # rows 0 and N-1, and a row twice in one batch
        rows = np.array(rows, np.int32)
        want = [torch.from_numpy(x) for x in R.gather_ref(*c["host"], rows, T)]
        out = _prefilled(B, E, T)
        ret = ops.caption_gather(*c["dev"], ops.HostMirror(rows, DEV), T, out=out)
        assert all(r is o for r, o in zip(ret, out))                                # the caller's tensors are the ones written
        for name, g, w in zip(("words_embs", "sent_embs", "mask"), out, want):
            assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g.cpu(), w), (name, rows.tolist())
        fresh = ops.caption_gather(*c["dev"], rows, T)                              # a host array: uploaded by the op; new tensors
        assert fresh[0].dtype == torch.float32 and fresh[2].dtype == torch.bool and fresh[0].is_contiguous()
        for g, o in zip(fresh, out):
            assert g.data_ptr() != o.data_ptr() and g.device == DEV and torch.equal(g, o)        # two calls, the same bytes


def test_shapes_outside_the_kernels_limits_are_the_librarys_shape_error():
    from xmc_gan_amd import ops
    lens = R.kernel_lens(5)
    rows = np.array([0], np.int32)
    sent, tok, off = R.tables(lens, 6)
    with pytest.raises(ValueError, match="XMC_ESHAPE"):                              # E = 6: not a multiple of 4
        ops.caption_gather(*(torch.from_numpy(x).to(DEV) for x in (sent, tok, off, lens)), rows, 5)
    c = _case(8, 5)
    with pytest.raises(ValueError, match="XMC_ESHAPE"):                              # T = 65
        ops.caption_gather(*c["dev"], rows, 65)


def test_bad_rows_raise_before_any_launch(monkeypatch):
    from xmc_gan_amd import ops
    import xmc_gan_amd.lib as L
    c = _case(8, 5)
    calls = []
    monkeypatch.setattr(L, "load", lambda *a: calls.append("load"))
    for bad in ([0, -1], [N, 0]):
        with pytest.raises(ValueError, match="out of range"):
            ops.caption_gather(*c["dev"], ops.HostMirror(np.array(bad, np.int32), DEV), 5)
    with pytest.raises(ValueError, match="host copy"):
        ops.caption_gather(*c["dev"], torch.zeros(2, dtype=torch.int32, device=DEV), 5)
    assert calls == []


# ------------------------------------------------------------------------------------------------------------------------ against the live encoders
SIZES = [(40, 30), (30, 47), (13, 9), (21, 21), (50, 18), (33, 20), (19, 31), (64, 48), (25, 25), (31, 17), (12, 44)]     # 11 images (width, height)
S_IMG, ML, BS = 8, 8, 4


def _cfg(preset, **text):
    from xmc_gan.config import gan
    gan.reset_cfg()
    gan.cfg_from_file(os.path.join(CFG_DIR, preset))
    gan.cfg.IMG.SIZE = S_IMG
    gan.cfg.TRAIN.BATCH_SIZE = BS
    for k, v in text.items():
        gan.cfg.TEXT[k] = v
    return gan.cfg


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from xmc_gan_amd import imagecache as IC
    root = tmp_path_factory.mktemp("coco")
    data_dir, keys = DR.mini_tree(root / "data", SIZES, sent=True)
    images = str(root / "image_cache")
    IC.build_cache(data_dir, S_IMG, "train", images, threads=2)
    return dict(root=root, data_dir=data_dir, keys=keys, images=images)


def _same(got, want, what):
    for name, g, w in zip(("words_embs", "sent_embs", "mask"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.device == w.device, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        assert torch.equal(g, w), (what, name, float((g.float() - w.float()).abs().max()))


def _two_epochs_equal_the_live_encoder(tree, cfg, live, cache_dir):
    """build at --bs 4 (11 captions: the last batch is a filled one), load, and compare every batch of two epochs with the live encoder"""
    from xmc_gan import dataset as D
    from xmc_gan_amd import captioncache as CC, imagecache as IC, ops
    CC.build_cache(cfg, tree["data_dir"], "train", live, cache_dir, BS, "the test's encoder")
    arch = D.WordTextDataset if cfg.TEXT.TYPE == "WORD" else D.SentTextDataset
    ds = arch(data_dir=tree["data_dir"], mode="train", transform=None, cfg=cfg)
    cache = CC.CaptionCache.load(cache_dir, "train", cfg, ds, ops.precision())
    assert len(cache) == len(SIZES) and cache.meta["batch_size"] == BS and cache.meta["encoder_source"] == "the test's encoder"
    cached = CC.CachedTextEncoder(cache, DEV, reserve=0)
    assert not list(cached.parameters()) and cached.encoder_name == cfg.TEXT.ENCODER_NAME and cached.emb_dim == cfg.TEXT.EMBEDDING_DIM
    loader = IC.DeviceImageLoader(IC.ImageCache.load(tree["images"], "train", S_IMG, ds.filenames), ds, BS, DEV, train=True, seed=5)
    seen = []
    for epoch in (1, 2):
        for imgs, texts, keys in loader:
            caps, cap_lens = texts[0]
            with torch.no_grad():
                want = live(caps, cap_lens)
            got = cached.forward_keys(keys)
            _same(got, want, (epoch, keys))
            assert tuple(got[0].shape) == (BS, cfg.TEXT.EMBEDDING_DIM, ML) and got[1].data_ptr() != cached.sent_tab.data_ptr()
            seen.append(tuple(keys))
    assert len(seen) == 4 and set(seen[:2]) != set(seen[2:])                        # another permutation in the second epoch
    # rows: the same through a HostMirror and a host array; a bad row and an unknown key are refused
    rows = np.array([10, 0, 10, 3], np.int32)
    _same(cached.forward_rows(ops.HostMirror(rows, DEV)), cached.forward_rows(rows.astype(np.int64)), "rows")
    _same(cached.forward_rows(rows), cached.forward_keys([tree["keys"][i] for i in rows]), "keys")
    for i in (0, 10):
        w, s, m = cache.entry(i)
        got = cached.forward_rows([i])
        assert np.array_equal(got[0][0].cpu().numpy(), w) and np.array_equal(got[1][0].cpu().numpy(), s) and np.array_equal(got[2][0].cpu().numpy(), m)
    with pytest.raises(ValueError, match="out of range"):
        cached.forward_rows([0, 11])
    with pytest.raises(ValueError, match="out of range"):
        cached.forward_rows(np.array([2 ** 32], np.int64))
    with pytest.raises(KeyError, match="nokey"):
        cached.forward_keys(["k000", "nokey"])
    with pytest.raises(TypeError, match="forward_keys"):
        cached(["a"], torch.tensor([1]))
    return cache, cached, ds


@pytest.mark.parametrize("rnn_type", ["LSTM", "GRU"])
def test_cached_rnn_encoder_equals_the_live_one_bit_for_bit(tree, tmp_path, rnn_type):
    """WORD captions and a randomly initialised RNN_ENCODER.  EMBEDDING_DIM is 256, the one width the recurrence kernels are built for
    (`xmc_lstm_bidir` / `xmc_gru_bidir` return XMC_EINVAL for any other: a live encoder at 32 cannot run, so there is nothing to compare a
    narrower cache with); four 64-channel chunks per caption."""
    from xmc_gan.model.encoder import RNN_ENCODER
    cfg = _cfg("df_gan_damsm.yml", EMBEDDING_DIM=256, MAX_LENGTH=ML, VOCA_SIZE=40, RNN_TYPE=rnn_type, ENCODER_DIR="")
    torch.manual_seed(11)
    live = RNN_ENCODER(cfg).to(DEV).eval().requires_grad_(False)
    cache, cached, ds = _two_epochs_equal_the_live_encoder(tree, cfg, live, str(tmp_path / "cache"))
    assert cached.rnn_type == rnn_type and cache.encoder == "RNN"
    assert np.array_equal(cache.lens, [min(len(ds.captions[i * 5 + 1]), ML) for i in range(len(SIZES))])      # the count of non-zero ids
    assert cache.matches_encoder(live)
    with torch.no_grad():
        live.rnn.weight_hh_l0_reverse[3, 2] += 1e-3
    assert not cache.matches_encoder(live)
    with pytest.raises(RuntimeError, match=f"{cache.nbytes} bytes.*reserve"):
        from xmc_gan_amd import captioncache as CC
        CC.CachedTextEncoder(cache, DEV, reserve=1 << 50)


# the bars tests/test_sbert_gpu.py holds the small encoder (hidden 128, 2 layers) to in the bf16 mode (its SMALL_BAR["bf16"]): largest absolute
# error over the output's rms against the f64 restatement, (words_embs, sent_embs)
SBERT_BF16_BAR = (1.5 * 9.691e-03, 1.5 * 5.496e-03)


def _err(got, want):
    want = want.double()
    return float((got.double() - want).abs().max() / want.pow(2).mean().sqrt())


def test_cached_sbert_encoder_equals_the_live_one_bit_for_bit(tree, tmp_path):
    """SENT captions, a generated 2-layer, 128-wide RoBERTa and a byte-level BPE trained on the tree's sentences.  The --bs 4 cache equals
    the live encoder bit for bit; a --bs 3 cache is held to the f64 restatement at the bar of the bf16 mode, and its distance from the
    --bs 4 cache is printed (DESIGN.md section 7m records it)."""
    try:
        import tokenizers
    except ImportError:
        pytest.skip("the `tokenizers` package is not importable on this machine: SBERT_ENCODER.forward cannot tokenize sentences")
    import pickle
    from xmc_gan.model.encoder import SBERT_ENCODER
    from xmc_gan_amd import captioncache as CC, ops
    with open(os.path.join(tree["data_dir"], "bert_captions.pickle"), "rb") as f:
        sents = pickle.load(f)[0]
    tok = tokenizers.ByteLevelBPETokenizer()
    tok.train_from_iterator(sents, vocab_size=280, min_frequency=1, special_tokens=["<s>", "<pad>", "</s>", "<unk>", "<mask>"], show_progress=False)
    model = tmp_path / "model"
    hf, w = SR.write_model_dir(model, 21, SR.hf_config(hidden=128, layers=2, vocab=tok.get_vocab_size(), max_pos=40))
    tok.save(str(model / "tokenizer.json"))
    cfg = _cfg("df_gan_sbert_seperate.yml", EMBEDDING_DIM=128, MAX_LENGTH=ML)
    ops.set_precision("bf16")
    live = SBERT_ENCODER(cfg, model_dir=str(model)).to(DEV)
    cache, cached, ds = _two_epochs_equal_the_live_encoder(tree, cfg, live, str(tmp_path / "cache4"))
    assert cache.encoder == "SBERT" and cache.rnn_type == "" and cache.meta["precision"] == "bf16" and cache.meta["encoder_source"]
    handed = [ds.get_caption(i * 5 + 1)[0] for i in range(len(SIZES))]
    ids, lens = live.tokenize(handed)
    assert np.array_equal(cache.lens, lens.numpy())                                 # the token count with <s> and </s>
    assert cache.matches_encoder(live)
    kept = live._w["1.wo"].data[5, 7].clone()
    live._w["1.wo"].data[5, 7] += 1e-3
    assert not cache.matches_encoder(live)
    live._w["1.wo"].data[5, 7] = kept
    assert cache.matches_encoder(live)
    # another batch size: not promised bit-equal, held to the f64 restatement
    CC.build_cache(cfg, tree["data_dir"], "train", live, str(tmp_path / "cache3"), 3)
    cache3 = CC.CaptionCache.load(str(tmp_path / "cache3"), "train", cfg, ds, "bf16")
    assert cache3.meta["batch_size"] == 3 and np.array_equal(cache3.lens, cache.lens)
    want = SR.encode(w, hf, ids, lens, ML, bool(cfg.TEXT.BERT_NORM))
    e3 = [torch.from_numpy(np.stack(x)) for x in zip(*(cache3.entry(i) for i in range(len(SIZES))))]
    e4 = [torch.from_numpy(np.stack(x)) for x in zip(*(cache.entry(i) for i in range(len(SIZES))))]
    ew, es = _err(e3[0], want[0]), _err(e3[1], want[1])
    print(f"caption cache built at --bs 3 against the f64 restatement: words {ew:.3e} sent {es:.3e}; the --bs 4 cache: words "
          f"{_err(e4[0], want[0]):.3e} sent {_err(e4[1], want[1]):.3e}; |bs 3 - bs 4|: words {float((e3[0] - e4[0]).abs().max()):.3e} sent "
          f"{float((e3[1] - e4[1]).abs().max()):.3e}")
    assert torch.equal(e3[2], want[2])
    assert ew <= SBERT_BF16_BAR[0] and es <= SBERT_BF16_BAR[1]


# ------------------------------------------------------------------------------------------------------------------------ the entry point
def _build_caches(yml, data_dir, out):
    import xmc_gan.caption_cache as cli
    for split in ("train", "test"):
        cli.main(["build", "--cfg", yml, "--data_dir", data_dir, "--split", split, "--out", out, "--bs", "4"])
    from xmc_gan.config import gan
    gan.reset_cfg()


def _no_encoder(monkeypatch):
    from xmc_gan.model.encoder import RNN_ENCODER

    def forward(self, *a, **k):
        raise AssertionError("the text encoder ran in a --caption_cache run")
    monkeypatch.setattr(RNN_ENCODER, "forward", forward)


def test_entry_point_trains_and_evaluates_from_both_caches(tmp_path, monkeypatch, caplog):
    """``--image_cache`` and ``--caption_cache`` with the shrunken DAMSM preset at 64 px, batches of 4 over 8 generated images, 51 epochs of two
    iterations (checkpoints and eval() start at epoch 51); RNN_ENCODER.forward raises, so no encoder runs."""
    import logging
    import xmc_gan.train_gan as tg
    from xmc_gan_amd import imagecache as IC
    caplog.set_level(logging.INFO)
    data_dir, keys = DR.mini_tree(tmp_path / "coco", [(100, 90)] * 5 + [(80, 120), (76, 76), (150, 76)])
    images, captions, run = str(tmp_path / "images"), str(tmp_path / "captions"), str(tmp_path / "run")
    for split in ("train", "test"):
        IC.build_cache(data_dir, 64, split, images, threads=2)
    yml = R.mini_yml(tmp_path)
    _build_caches(yml, data_dir, captions)
    _no_encoder(monkeypatch)
    last = tg.main(["--cfg", yml, "--data_dir", data_dir, "--image_cache", images, "--caption_cache", captions, "--bs", "4", "--imsize", "64",
                    "--max_epoch", "51", "--output_dir", run, "--seed", "3"])
    assert {"errD", "errG"} <= set(last)
    for k, v in last.items():
        if torch.is_tensor(v) and v.numel() == 1:
            assert math.isfinite(float(v)), k
    assert last.get("hipgraph") is True
    assert sorted(os.listdir(os.path.join(run, "model"))) == ["netD_051.pth", "netG_051.pth", "optimizerD.pth", "optimizerG.pth"]
    img = os.path.join(run, "img")
    files = set(os.listdir(img))
    assert {"sents.txt", "imgs.png", "fake_samples_epoch_001.png", "fake_samples_epoch_051.png", "test", "org"} <= files, files
    assert len(open(os.path.join(img, "sents.txt")).read().splitlines()) == 4
    assert sorted(os.listdir(os.path.join(img, "test"))) == sorted(os.listdir(os.path.join(img, "org"))) == sorted(f"{k}.png" for k in keys)
    lines = [r.getMessage() for r in caplog.records if r.getMessage().startswith("caption cache ")]      # one line per split
    assert len(lines) == 2 and "train.cap.f32: 8 captions" in lines[0] and "test.cap.f32: 8 captions" in lines[1], lines
    assert all("bytes on the device" in l and "RNN encoder" in l for l in lines)


def test_entry_point_names_the_build_command_for_a_missing_or_a_foreign_cache(tmp_path, monkeypatch):
    import xmc_gan.train_gan as tg
    data_dir, keys = DR.mini_tree(tmp_path / "coco", [(100, 90)] * 4)
    yml = R.mini_yml(tmp_path)
    common = ["--data_dir", data_dir, "--bs", "4", "--imsize", "64", "--max_epoch", "1", "--output_dir", str(tmp_path / "run")]
    with pytest.raises(SystemExit) as e:
        tg.main(["--cfg", yml, "--caption_cache", str(tmp_path / "nothing")] + common)
    msg = str(e.value)
    assert msg.startswith("--caption_cache: ") and "python xmc_gan/caption_cache.py build" in msg and f"--cfg {yml}" in msg
    assert f"--data_dir {data_dir}" in msg and "--split train" in msg and f"--out {tmp_path / 'nothing'}" in msg
    from xmc_gan.config import gan
    gan.reset_cfg()
    captions = str(tmp_path / "captions")
    _build_caches(yml, data_dir, captions)                                           # MAX_LENGTH 8
    _no_encoder(monkeypatch)
    other = R.mini_yml(tmp_path, name="len6.yml", **{"MAX_LENGTH: 20": "MAX_LENGTH: 6"})
    with pytest.raises(SystemExit, match="max_length 8.*python xmc_gan/caption_cache.py build"):
        tg.main(["--cfg", other, "--caption_cache", captions] + common)


def test_entry_point_with_the_pil_loader_and_the_caption_cache(tmp_path, monkeypatch):
    """no --image_cache: the DataLoader's batches carry the same keys; one epoch of two iterations"""
    import xmc_gan.train_gan as tg
    data_dir, keys = DR.mini_tree(tmp_path / "coco", [(100, 90)] * 5 + [(80, 120), (76, 76), (150, 76)])
    yml = R.mini_yml(tmp_path)
    captions = str(tmp_path / "captions")
    _build_caches(yml, data_dir, captions)
    _no_encoder(monkeypatch)
    last = tg.main(["--cfg", yml, "--data_dir", data_dir, "--caption_cache", captions, "--bs", "4", "--imsize", "64", "--max_epoch", "1",
                    "--output_dir", str(tmp_path / "run"), "--seed", "3"])
    assert {"errD", "errG"} <= set(last)
    for k, v in last.items():
        if torch.is_tensor(v) and v.numel() == 1:
            assert math.isfinite(float(v)), k
    assert len(open(os.path.join(tmp_path / "run", "img", "sents.txt")).read().splitlines()) == 4
