"""The sentence encoder on the GPU: each kernel of csrc/transformer.hip alone, `SBERT_ENCODER.forward_ids` whole (small, and at
RoBERTa-base's width), determinism, independence from padding, and the entry points -- against tests/sbert_ref.py computed on the CPU in
f64 inside the test.  Nothing outside the repository is read: weights and model directories are generated from seeds.

Error figure everywhere: the largest absolute error over the output's rms against the f64 restatement.  Bars are 1.5 x the figure measured on
the MI355X (the project's ratchet rule), written beside each constant; in fp32 mode anything above 1e-3 would be a bug, not a bar.
For the 16-bit modes the same restatement with its GEMM operands rounded to the format on the CPU is reported as well (`format`): the bar
reflects the number format, not the kernels."""
import math
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sbert_ref as R
from golden_util import CFG_DIR
import xmc_gan_amd.lib as L
from xmc_gan_amd import ops

DEV = torch.device("cuda", 0)
FMT = {"bf16": torch.bfloat16, "f16": torch.float16, "fp32": None}


@pytest.fixture(autouse=True)
def _restore():
    yield
    ops.set_precision("bf16")
    from xmc_gan.config import gan
    gan.reset_cfg()


def _err(got, want):
    want = want.double()
    return float((got.detach().double().cpu() - want).abs().max() / want.pow(2).mean().sqrt())


def _cfg(**text):
    from xmc_gan.config import gan
    gan.reset_cfg()
    gan.cfg_from_file(os.path.join(CFG_DIR, "df_gan_sbert_seperate.yml"))
    for k, v in text.items():
        gan.cfg.TEXT[k] = v
    return gan.cfg


def _i32(lengths):
    return torch.tensor(lengths, dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------ kernels alone
LN_BAR = {64: 1.5 * 2.733e-07, 128: 1.5 * 3.279e-07, 768: 1.5 * 5.211e-07, 1024: 1.5 * 4.420e-07}          # 1.5 x measured


@pytest.mark.parametrize("width", [64, 128, 768, 1024])
def test_add_layernorm_rows(width):
    """LN(x + bias + residual) on 21 rows (not a multiple of the 4 rows a workgroup takes), a mean far from zero (two-pass statistics),
    and the 16-bit copy = the f32 result rounded"""
    g = torch.Generator().manual_seed(width)
    x, res = torch.randn(21, width, generator=g) * 2 + 3, torch.randn(21, width, generator=g)
    bias, gamma, beta = torch.randn(width, generator=g), 1 + 0.1 * torch.randn(width, generator=g), torch.randn(width, generator=g)
    want = R.layer_norm((x + bias + res).double(), gamma.double(), beta.double(), 1e-5)
    ops.set_precision("bf16")
    got, got16 = ops.add_layernorm(x.to(DEV), res.to(DEV), gamma.to(DEV), beta.to(DEV), 1e-5, bias=bias.to(DEV), out16=torch.bfloat16)
    e = _err(got, want)
    print(f"add_layernorm width {width}: {e:.3e}")
    assert got.dtype == torch.float32 and got16.dtype == torch.bfloat16 and torch.equal(got16, got.to(torch.bfloat16))
    assert e <= LN_BAR[width]
    got2, none = ops.add_layernorm((x + bias).to(DEV), res.to(DEV), gamma.to(DEV), beta.to(DEV), 1e-5)
    assert none is None and _err(got2, want) <= LN_BAR[width]
    with pytest.raises(L.XmcHipError):                     # a width that is not built is refused, not computed wrong
        ops.add_layernorm(torch.zeros(4, 96, device=DEV), None, torch.ones(96, device=DEV), torch.zeros(96, device=DEV), 1e-5)
    with pytest.raises(RuntimeError):
        ops.add_layernorm(x, res, gamma, beta, 1e-5)


EMBED_BAR = 1.5 * 5.027e-07          # 1.5 x measured


def test_roberta_embed_ln_positions_from_lengths():
    hf = R.hf_config(hidden=128, layers=0, vocab=60, max_pos=40)
    w = R.random_weights(hf, 7)
    ids, lens = R.random_batch(hf, [7, 4, 2], 7, seed=2)
    want = R.hidden_states(w, hf, ids, lens)                    # no layers: the embedding block alone
    e = "embeddings."
    d = lambda k: w[e + k].to(DEV).contiguous()
    ops.set_precision("f16")
    got, got16 = ops.roberta_embed_ln(ids.to(DEV), _i32([7, 4, 2]), d("word_embeddings.weight"), d("position_embeddings.weight"),
                                      d("token_type_embeddings.weight")[0].contiguous(), d("LayerNorm.weight"), d("LayerNorm.bias"), 1e-5, 1,
                                      out16=torch.float16)
    err = _err(got.view(3, 7, 128), want)
    print(f"roberta_embed_ln: {err:.3e}")
    assert err <= EMBED_BAR and torch.equal(got16, got.to(torch.float16))
    # padded positions read the padding position (HF: cumsum(mask) * mask + padding_idx), not t + 2
    pad_row = R.layer_norm((w[e + "word_embeddings.weight"][1] + w[e + "token_type_embeddings.weight"][0] + w[e + "position_embeddings.weight"][1]).double(),
                           w[e + "LayerNorm.weight"].double(), w[e + "LayerNorm.bias"].double(), 1e-5)
    assert _err(got.view(3, 7, 128)[2, 5], pad_row) <= EMBED_BAR


ATT_BAR = {7: 1.5 * 8.469e-07, 64: 1.5 * 4.137e-06}          # 1.5 x measured


@pytest.mark.parametrize("T,lengths", [(7, [7, 4, 2]), (64, [64, 33, 2])])
def test_attention_short_ragged(T, lengths):
    """B = 3, 2 heads of dimension 64; length 2 is a sentence of <s></s> alone.  Compared on the rows of valid queries; the rows of padded
    queries are finite (zeros).  Scores of a few units: the softmax is far from uniform."""
    g = torch.Generator().manual_seed(T)
    B, heads, H = 3, 2, 128
    qkv = torch.randn(B * T, 3 * H, generator=g)
    qkv[:, :2 * H] *= 1.5
    q, k, v = (qkv[:, i * H:(i + 1) * H].double().view(B, T, H) for i in range(3))
    want = R.attention(q, k, v, lengths, heads)
    ops.set_precision("fp32")
    got = ops.attention_short(qkv.to(DEV), _i32(lengths), B, T, heads).view(B, T, H)
    valid = torch.arange(T)[None, :] < torch.tensor(lengths)[:, None]
    e = _err(got.cpu()[valid], want[valid])
    print(f"attention_short T {T}: {e:.3e}")
    assert e <= ATT_BAR[T]
    assert torch.isfinite(got).all() and (got.cpu()[~valid] == 0).all()
    ops.set_precision("bf16")                                   # the 16-bit destination: the same values rounded
    got16 = ops.attention_short(qkv.to(DEV), _i32(lengths), B, T, heads, out_dtype=torch.bfloat16).view(B, T, H)
    assert torch.equal(got16, got.to(torch.bfloat16))


def test_attention_short_refuses_other_shapes():
    lens = _i32([3])
    with pytest.raises(AssertionError):                        # T > 64
        ops.attention_short(torch.zeros(65, 3 * 64, device=DEV), lens, 1, 65, 1)
    with pytest.raises(AssertionError):                        # head dimension 32
        ops.attention_short(torch.zeros(4, 3 * 64, device=DEV), lens, 1, 4, 2)
    lib = L.load()
    p = torch.zeros(65 * 192, device=DEV)
    assert lib.xmc_attention_short(p.data_ptr(), lens.data_ptr(), p.data_ptr(), 1, 65, 1, 64, L.F32, None) == -3      # XMC_ESHAPE
    assert lib.xmc_attention_short(p.data_ptr(), lens.data_ptr(), p.data_ptr(), 1, 4, 2, 32, L.F32, None) == -3


GELU_BAR = 1.5 * 2.739e-07          # 1.5 x measured


def test_bias_gelu_is_the_erf_form():
    g = torch.Generator().manual_seed(3)
    x, bias = torch.randn(21, 256, generator=g) * 2, torch.randn(256, generator=g) * 0.5
    x[0, :8] = torch.tensor([-30.0, -12.0, -6.0, -5.0, 5.0, 6.0, 12.0, 30.0])
    x[20, -4:] = torch.tensor([-100.0, 100.0, -1e4, 1e4])
    a = (x + bias).double()
    want = R.gelu_erf(a)
    ops.set_precision("fp32")
    got = ops.bias_gelu(x.to(DEV), bias.to(DEV)).cpu()
    small = a.abs() < 50                                        # the rms of the few huge outputs must not carry the figure
    e = _err(got[small], want[small])
    print(f"bias_gelu: {e:.3e}")
    assert e <= GELU_BAR
    tanh_form = 0.5 * a * (1 + torch.tanh(math.sqrt(2 / math.pi) * (a + 0.044715 * a ** 3)))
    assert _err(tanh_form[small], want[small]) > 100 * GELU_BAR      # the bar tells the two forms apart
    assert torch.isfinite(got).all()
    assert (got[a < -12].abs() <= 1e-30).all() and torch.equal(got[a > 12], (x + bias)[a > 12])
    ops.set_precision("bf16")
    assert torch.equal(ops.bias_gelu(x.to(DEV), bias.to(DEV), out_dtype=torch.bfloat16).cpu(), got.to(torch.bfloat16))


POOL_BAR = {True: 1.5 * 2.927e-07, False: 1.5 * 1.661e-07}          # 1.5 x measured


@pytest.mark.parametrize("bert_norm", [True, False])
def test_pool_mask_transpose_tail(bert_norm):
    """T = 7 into MAX_LENGTH = 20: words_embs is a masked copy (exact), zero at padding and beyond T (exactly), the mask is exact"""
    g = torch.Generator().manual_seed(11)
    B, T, H, ML, lengths = 3, 7, 128, 20, [7, 4, 2]
    hidden = torch.randn(B, T, H, generator=g) + 0.5
    words_w, sent_w, mask_w = R.pool_tail(hidden.double(), lengths, ML, bert_norm)
    words, sent, mask = ops.sbert_pool(hidden.to(DEV), _i32(lengths), ML, bert_norm)
    assert words.shape == (B, H, ML) and sent.shape == (B, H) and mask.shape == (B, ML) and mask.dtype == torch.bool
    assert torch.equal(mask.cpu(), mask_w)
    assert torch.equal(words.cpu(), words_w.float())
    for b, n in enumerate(lengths):
        assert (words[b, :, n:] == 0).all() and bool(mask[b, n:].all()) and not bool(mask[b, :n].any())
    e = _err(sent, sent_w)
    print(f"sbert_pool sent_embs (BERT_NORM {bert_norm}): {e:.3e}")
    assert e <= POOL_BAR[bert_norm]
    if bert_norm:
        assert torch.allclose(sent.norm(dim=1).cpu(), torch.ones(B), atol=1e-6)


# ------------------------------------------------------------------------------------------ the whole encoder
@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """2 layers, hidden 128, 2 heads, FFN 256, vocab 60; B = 3 with ragged lengths; the f64 restatement, computed once"""
    d = tmp_path_factory.mktemp("sbert_small")
    hf, w = R.write_model_dir(d, 21)
    ids, lens = R.random_batch(hf, [9, 5, 2], 9, seed=4)
    want = {fmt: R.encode(w, hf, ids, lens, 12, False, gemm_fmt=FMT[fmt]) for fmt in FMT}
    return dict(dir=str(d), hf=hf, w=w, ids=ids, lens=lens, want=want)


def _encoder(model_dir, **text):
    from xmc_gan.model.encoder import SBERT_ENCODER
    return SBERT_ENCODER(_cfg(**text), model_dir=model_dir).to(DEV)


def _report(tag, got, want, want_fmt=None):
    """(words_embs, sent_embs) error figures against the f64 restatement; in a 16-bit mode also the format's own error (restatement with
    rounded GEMM operands against the exact one) and the kernels' distance from that rounded restatement"""
    ew, es = _err(got[0], want[0]), _err(got[1], want[1])
    line = f"{tag}: words {ew:.3e} sent {es:.3e}"
    if want_fmt is not None:
        line += (f" | format: words {_err(want_fmt[0], want[0]):.3e} sent {_err(want_fmt[1], want[1]):.3e}"
                 f" | against the rounded restatement: words {_err(got[0], want_fmt[0]):.3e} sent {_err(got[1], want_fmt[1]):.3e}")
    print(line)
    return ew, es


# mode: (words_embs bar, sent_embs bar)
# 1.5 x measured.  The 16-bit figures are the format's: the restatement with its GEMM operands rounded on the CPU is 9.691e-03 / 5.496e-03 (bf16)
# and 1.069e-03 / 7.681e-04 (f16) from the exact one, and the kernels are 1.169e-06 / 4.940e-07 (bf16) and 6.536e-05 / 9.120e-06 (f16: operands
# that round to the other neighbour in f32 than in f64) from the rounded restatement
SMALL_BAR = {"fp32": (1.5 * 1.210e-06, 1.5 * 6.010e-07), "bf16": (1.5 * 9.691e-03, 1.5 * 5.496e-03), "f16": (1.5 * 1.069e-03, 1.5 * 7.725e-04)}


@pytest.mark.parametrize("mode", ["fp32", "bf16", "f16"])
def test_whole_encoder_small(small, mode):
    ops.set_precision(mode)
    enc = _encoder(small["dir"], EMBEDDING_DIM=128, MAX_LENGTH=12)
    words, sent, mask = enc.forward_ids(small["ids"], small["lens"])
    want = small["want"]["fp32"]
    assert words.shape == (3, 128, 12) and words.dtype == torch.float32 and sent.shape == (3, 128) and torch.equal(mask.cpu(), want[2])
    for b, n in enumerate(small["lens"].tolist()):
        assert (words[b, :, n:] == 0).all()
    ew, es = _report(f"small encoder [{mode}]", (words, sent), want, None if mode == "fp32" else small["want"][mode])
    assert ew <= SMALL_BAR[mode][0] and es <= SMALL_BAR[mode][1]
    if mode == "fp32":
        assert max(SMALL_BAR[mode]) <= 1e-3


WIDE_BAR = (1.5 * 8.032e-06, 1.5 * 1.906e-06)          # 1.5 x measured


def test_whole_encoder_at_roberta_base_width(tmp_path):
    """1 layer, hidden 768, 12 heads, FFN 3072 (RoBERTa-base's layer), B = 2, T = MAX_LENGTH = 20, lengths {20, 9}, fp32 mode, BERT_NORM on"""
    hf = R.hf_config(hidden=768, layers=1, heads=12, ffn=3072, vocab=60, max_pos=40)
    _, w = R.write_model_dir(tmp_path, 33, hf)
    ids, lens = R.random_batch(hf, [20, 9], 20, seed=5)
    want = R.encode(w, hf, ids, lens, 20, True)
    ops.set_precision("fp32")
    enc = _encoder(str(tmp_path), BERT_NORM=True)
    words, sent, mask = enc.forward_ids(ids, lens)
    assert words.shape == (2, 768, 20) and torch.equal(mask.cpu(), want[2])
    ew, es = _report("768-wide layer [fp32]", (words, sent), want)
    assert ew <= WIDE_BAR[0] and es <= WIDE_BAR[1] and max(WIDE_BAR) <= 1e-3


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_same_input_twice_gives_identical_bytes(small, mode):
    ops.set_precision(mode)
    enc = _encoder(small["dir"], EMBEDDING_DIM=128, MAX_LENGTH=12)
    a = [t.clone() for t in enc.forward_ids(small["ids"], small["lens"])]
    b = enc.forward_ids(small["ids"].to(DEV), small["lens"].to(DEV))          # device inputs: the same path after the copy
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_result_does_not_depend_on_the_padding(small):
    """[B, T] and the same sentences padded to a longer T: identical bytes in the valid columns of words_embs (the others are zero either
    way) and identical sent_embs, fp32 mode"""
    ops.set_precision("fp32")
    enc = _encoder(small["dir"], EMBEDDING_DIM=128, MAX_LENGTH=12)
    ids, lens = small["ids"], small["lens"]
    wide = torch.full((3, 12), small["hf"]["pad_token_id"], dtype=torch.int64)
    wide[:, :9] = ids
    w1, s1, m1 = enc.forward_ids(ids, lens)
    w2, s2, m2 = enc.forward_ids(wide, lens)
    assert torch.equal(w1, w2) and torch.equal(s1, s2) and torch.equal(m1, m2)


# ------------------------------------------------------------------------------------------ entry points
def _mini_sent_coco(root, n_img=8):
    from PIL import Image
    rng = np.random.RandomState(1)
    (root / "images").mkdir(parents=True)
    keys = [f"k{i:03d}" for i in range(n_img)]
    for k in keys:
        Image.fromarray(rng.randint(0, 256, (90, 100, 3), dtype=np.uint8)).save(root / "images" / f"{k}.jpg")
    for mode in ("train", "test"):
        (root / mode).mkdir()
        with open(root / mode / "filenames.pickle", "wb") as f:
            pickle.dump(keys, f)
    words = "a the man dog cat rides sits on in green wooden bench wave grass large small plate of food and".split()
    sents = [" ".join(rng.choice(words, size=rng.randint(1, 26))) for _ in range(n_img * 5)]      # some longer than MAX_LENGTH tokens
    with open(root / "bert_captions.pickle", "wb") as f:
        pickle.dump([sents, sents[::-1]], f)
    return str(root), sents


def test_sbert_preset_from_the_entry_points(tmp_path):
    """`train_gan.main` on an SBERT preset with --sbert_dir: sentences from a miniature SentTextDataset tree, tokenized on the host, encoded
    by a generated 1-layer, 768-wide model directory, two iterations at 64 px with finite losses; then `sample.py --captions` with the same
    directory writes images."""
    try:
        import tokenizers
    except ImportError:
        pytest.skip("the `tokenizers` package is not importable on this machine: SBERT_ENCODER.forward cannot tokenize sentences")
    import xmc_gan.sample as sample
    import xmc_gan.train_gan as tg
    data, sents = _mini_sent_coco(tmp_path / "coco")
    tok = tokenizers.ByteLevelBPETokenizer()
    tok.train_from_iterator(sents, vocab_size=280, min_frequency=1, special_tokens=["<s>", "<pad>", "</s>", "<unk>", "<mask>"], show_progress=False)
    model = tmp_path / "model"
    R.write_model_dir(model, 8, R.hf_config(hidden=768, layers=1, heads=12, ffn=3072, vocab=tok.get_vocab_size(), max_pos=40))
    tok.save(str(model / "tokenizer.json"))
    txt = open(os.path.join(CFG_DIR, "df_gan_sbert_seperate.yml")).read()
    for a, b in {"NCH: 32": "NCH: 8", "BATCH_SIZE: 88": "BATCH_SIZE: 4", "LOG_INTERVAL: 200": "LOG_INTERVAL: 2", "NUM_WORKERS: 8": "NUM_WORKERS: 0"}.items():
        assert a in txt, a
        txt = txt.replace(a, b)
    assert "SIZE: 64" in txt and "ENCODER_NAME: SBERT" in txt
    yml = tmp_path / "mini_sbert.yml"
    yml.write_text(txt)
    last = tg.main(["--cfg", str(yml), "--data_dir", data, "--max_epoch", "1", "--precision", "bf16", "--sbert_dir", str(model),
                    "--output_dir", str(tmp_path / "run")])
    assert {"errD", "errG"} <= set(last)
    for k, v in last.items():
        if torch.is_tensor(v) and v.numel() == 1:
            assert math.isfinite(float(v)), k
    logged = [l.strip() for l in open(tmp_path / "run" / "img" / "sents.txt").read().splitlines()]
    assert len(logged) == 4 and all(l in sents for l in logged)                 # the first batch's sentences reached the encoder as strings
    netG = tg.main.last_models[0]
    torch.save(netG.state_dict(), tmp_path / "netG.pth")
    caps = tmp_path / "caps.txt"
    caps.write_text("a man rides a wave\nthe cat sits on a wooden bench\n")
    man = sample.main(["--cfg", str(yml), "--checkpoint", str(tmp_path / "netG.pth"), "--out", str(tmp_path / "out"), "--captions", str(caps),
                       "--sbert_dir", str(model)])
    assert sorted(os.listdir(tmp_path / "out")) == ["00000_0.png", "00001_0.png", "captions.txt", "grid.png", "manifest.json"]
    assert man["captions"] == 2
