"""CPU-only checks of the sentence encoder (`xmc_gan.model.encoder.SBERT_ENCODER`): the tests' f64 restatement (tests/sbert_ref.py)
against `transformers.RobertaModel`, the host-side tokenization against the `tokenizers` package, the model-directory loader, and
construction from every SBERT preset.  The device path is tests/test_sbert_gpu.py."""
import glob
import json
import os

import pytest
import torch

import sbert_ref as R
from golden_util import CFG_DIR

SBERT_PRESETS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CFG_DIR, "*.yml")) if "ENCODER_NAME: SBERT" in open(p).read())


@pytest.fixture(autouse=True)
def _clean(monkeypatch):
    monkeypatch.delenv("XMC_SBERT_DIR", raising=False)
    yield
    from xmc_gan.config import gan
    gan.reset_cfg()


def _cfg(preset="df_gan_sbert_seperate.yml", **text):
    from xmc_gan.config import gan
    gan.reset_cfg()
    gan.cfg_from_file(os.path.join(CFG_DIR, preset))
    for k, v in text.items():
        gan.cfg.TEXT[k] = v
    return gan.cfg


def test_restatement_equals_transformers_roberta_model():
    """The tie to the real architecture: `sbert_ref.hidden_states` against a randomly initialised `transformers.RobertaModel` in f64 on a
    ragged batch, at the valid positions (a padded position's hidden state is dropped by the pooling tail).  Both are f64 evaluations of
    the same formulas in a different operation order: observed 1.74e-15 of the output's rms (outputs of order 1), bound = 10 x that."""
    tr = pytest.importorskip("transformers")
    hf = R.hf_config(hidden=128, layers=2, heads=2, ffn=256, vocab=60, max_pos=40)
    torch.manual_seed(0)
    conf = tr.RobertaConfig(**{k: v for k, v in hf.items() if k not in ("model_type", "architectures")})
    model = tr.RobertaModel(conf, add_pooling_layer=False).double().eval()
    with torch.no_grad():              # the default initialisation has unit LayerNorms and zero biases: move them
        for n, p in model.named_parameters():
            if "LayerNorm" in n or n.endswith(".bias"):
                p.add_(torch.randn_like(p) * 0.1)
            elif "dense" in n or "self." in n:
                p.mul_(2.5)            # N(0, 0.02) -> N(0, 0.05): attention scores of order 1
    w = {k: v.detach().clone() for k, v in model.state_dict().items()}
    lengths = [13, 6, 2]
    ids, lens = R.random_batch(hf, lengths, 13, seed=1)
    attn = (torch.arange(13)[None, :] < lens[:, None]).long()
    with torch.no_grad():
        want = model(input_ids=ids, attention_mask=attn).last_hidden_state
    got = R.hidden_states(w, hf, ids, lens)
    assert got.dtype == torch.float64 and got.shape == want.shape == (3, 13, 128)
    valid = attn.bool()
    err = float((got - want)[valid].abs().max() / want[valid].pow(2).mean().sqrt())
    print(f"restatement vs transformers: max abs error / rms = {err:.2e}")
    assert err <= 1.74e-14


def _train_bpe(tmp_path):
    tk = pytest.importorskip("tokenizers")
    corpus = ["a man riding a wave on top of a surfboard", "two dogs play in the green grass", "a plate of food with broccoli and rice",
              "people standing near a large clock tower", "the cat sits on a wooden bench"]
    tok = tk.ByteLevelBPETokenizer()
    tok.train_from_iterator(corpus, vocab_size=300, min_frequency=1, special_tokens=["<s>", "<pad>", "</s>", "<unk>", "<mask>"], show_progress=False)
    return tk, tok, corpus


@pytest.mark.parametrize("files", ["tokenizer.json", "vocab+merges"])
def test_tokenization_adds_specials_truncates_and_pads(tmp_path, files):
    """<s> ... </s> around the stripped sentence, truncation to MAX_LENGTH tokens INCLUDING both specials, right padding with the pad id,
    lengths = tokens with the specials -- against `tokenizers`' own encode of the same sentences"""
    from xmc_gan.model.encoder import SBERT_ENCODER
    tk, tok, corpus = _train_bpe(tmp_path)
    hf = R.hf_config(hidden=128, layers=1, heads=2, ffn=256, vocab=tok.get_vocab_size(), max_pos=40)
    R.write_model_dir(tmp_path / "m", 3, hf)
    if files == "tokenizer.json":
        tok.save(str(tmp_path / "m" / "tokenizer.json"))
    else:
        tok.save_model(str(tmp_path / "m"))
        assert os.path.isfile(tmp_path / "m" / "vocab.json") and os.path.isfile(tmp_path / "m" / "merges.txt")
    L = 8
    enc = SBERT_ENCODER(_cfg(EMBEDDING_DIM=128, MAX_LENGTH=L), model_dir=str(tmp_path / "m"))
    sents = ["  " + corpus[0] + " \n", "a cat", corpus[2], "grass"]
    ids, lens = enc.tokenize(sents)
    assert ids.dtype == torch.int64 and ids.shape == (4, L) and lens.dtype == torch.int64 and lens.shape == (4,)
    bos, pad, eos = tok.token_to_id("<s>"), tok.token_to_id("<pad>"), tok.token_to_id("</s>")
    assert (bos, pad, eos) == (0, 1, 2)
    long_seen = False
    for row, n, s in zip(ids.tolist(), lens.tolist(), sents):
        own = tok.encode(s.strip(), add_special_tokens=False).ids
        long_seen |= len(own) > L - 2
        assert n == min(len(own), L - 2) + 2 <= L
        assert row[0] == bos and row[n - 1] == eos and row[1:n - 1] == own[:L - 2]
        assert row[n:] == [pad] * (L - n)
        assert all(t not in (bos, pad, eos) for t in row[1:n - 1])
    assert long_seen and int(lens.min()) < L               # one sentence was truncated, one left padding
    assert lens.tolist()[0] == L and ids[0, L - 1] == eos  # truncation keeps </s> as the last of the MAX_LENGTH tokens


def test_forward_without_tokenizer_files_names_them(tmp_path):
    pytest.importorskip("tokenizers")
    from xmc_gan.model.encoder import SBERT_ENCODER
    R.write_model_dir(tmp_path / "m", 3)
    enc = SBERT_ENCODER(_cfg(EMBEDDING_DIM=128), model_dir=str(tmp_path / "m"))
    with pytest.raises(ImportError, match="tokenizer.json"):
        enc(["a cat"], torch.tensor([2]))


def _loaded(enc):
    """the encoder's tensors back under their Hugging Face keys"""
    out = {}
    H = enc.hidden
    w = enc._w
    e = "embeddings."
    out[e + "word_embeddings.weight"], out[e + "position_embeddings.weight"] = w["word"], w["pos"]
    out[e + "token_type_embeddings.weight"] = w["type0"][None]
    out[e + "LayerNorm.weight"], out[e + "LayerNorm.bias"] = w["emb_g"], w["emb_b"]
    for i in range(enc.nlayers):
        l = f"encoder.layer.{i}."
        for j, n in enumerate(("query", "key", "value")):
            out[l + f"attention.self.{n}.weight"] = w[f"{i}.wqkv"][j * H:(j + 1) * H]
            out[l + f"attention.self.{n}.bias"] = w[f"{i}.bqkv"][j * H:(j + 1) * H]
        for mine, key in (("o", "attention.output.dense"), ("1", "intermediate.dense"), ("2", "output.dense")):
            out[l + key + ".weight"], out[l + key + ".bias"] = w[f"{i}.w{mine}"], w[f"{i}.b{mine}"]
        for mine, key in (("ln1", "attention.output.LayerNorm"), ("ln2", "output.LayerNorm")):
            out[l + key + ".weight"], out[l + key + ".bias"] = w[f"{i}.{mine}g"], w[f"{i}.{mine}b"]
    return out


@pytest.mark.parametrize("subdir,prefix,pooler,safetensors", [("", "", False, False), ("0_Transformer", "", False, False),
                                                             ("", "roberta.", True, False), ("0_Transformer", "roberta.", True, True)])
def test_loader_layouts_prefix_and_ignored_keys(tmp_path, subdir, prefix, pooler, safetensors):
    """the directory itself and its 0_Transformer/ subfolder, keys with and without 'roberta.', pooler / LM head / position_ids keys
    ignored, pytorch_model.bin and model.safetensors: every tensor arrives unchanged; nothing is a parameter, a buffer or in state_dict()"""
    if safetensors:
        pytest.importorskip("safetensors")
    from xmc_gan.model.encoder import SBERT_ENCODER
    hf, w = R.write_model_dir(tmp_path / "m", 5, subdir=subdir, prefix=prefix, pooler=pooler, safetensors=safetensors)
    enc = SBERT_ENCODER(_cfg(EMBEDDING_DIM=128), model_dir=str(tmp_path / "m"))
    got = _loaded(enc)
    want = {k: v for k, v in w.items() if not k.startswith(("pooler.", "lm_head.")) and k != "embeddings.position_ids"}
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == torch.float32 and torch.equal(got[k], want[k]), k
    assert len(enc.state_dict()) == 0 and not list(enc.parameters()) and not list(enc.buffers())
    assert not enc.training and all(not t.requires_grad for t in enc._w.values())
    assert (enc.hidden, enc.heads, enc.ffn, enc.nlayers, enc.pad_id, enc.eps) == (128, 2, 256, 2, 1, 1e-5)
    enc2 = enc.to(torch.float64)               # `.to()` reaches the frozen tensors (they stay f32: the kernels' format)
    assert enc2 is enc and all(t.dtype == torch.float32 for t in enc._w.values())
    with pytest.raises(RuntimeError):          # no CPU fallback
        enc.forward_ids(*R.random_batch(hf, [5, 3], 5, seed=0))


def test_loader_rejects_what_is_not_built(tmp_path, monkeypatch):
    from xmc_gan.model.encoder import SBERT_ENCODER
    cfg = _cfg(EMBEDDING_DIM=128)
    with pytest.raises(ImportError, match="XMC_SBERT_DIR"):                  # no directory at all
        SBERT_ENCODER(cfg)
    with pytest.raises(ImportError, match="does not exist"):
        SBERT_ENCODER(cfg, model_dir=str(tmp_path / "nowhere"))
    (tmp_path / "empty").mkdir()
    with pytest.raises(ImportError, match="config.json"):
        SBERT_ENCODER(cfg, model_dir=str(tmp_path / "empty"))
    monkeypatch.setenv("XMC_SBERT_DIR", str(tmp_path / "empty"))             # the environment variable is read
    with pytest.raises(ImportError, match="config.json"):
        SBERT_ENCODER(cfg)
    monkeypatch.delenv("XMC_SBERT_DIR")
    (tmp_path / "noweights").mkdir()
    (tmp_path / "noweights" / "config.json").write_text(json.dumps(R.hf_config()))
    with pytest.raises(ImportError, match="pytorch_model.bin"):
        SBERT_ENCODER(cfg, model_dir=str(tmp_path / "noweights"))
    for i, over in enumerate((dict(hidden_act="gelu_new"), dict(hidden_act="gelu_pytorch_tanh"), dict(model_type="bert"),
                              dict(position_embedding_type="relative_key"))):
        R.write_model_dir(tmp_path / f"bad{i}", 1, R.hf_config(**over))
        with pytest.raises(NotImplementedError, match=list(over)[0]):
            SBERT_ENCODER(cfg, model_dir=str(tmp_path / f"bad{i}"))
    R.write_model_dir(tmp_path / "ok", 1)
    with pytest.raises(ValueError, match="EMBEDDING_DIM"):                   # hidden 128 against the preset's 768
        SBERT_ENCODER(_cfg(), model_dir=str(tmp_path / "ok"))
    hf, w = R.write_model_dir(tmp_path / "short", 1)
    w.pop("encoder.layer.1.output.dense.bias")
    torch.save(w, tmp_path / "short" / "pytorch_model.bin")
    with pytest.raises(ImportError, match="encoder.layer.1.output.dense.bias"):
        SBERT_ENCODER(_cfg(EMBEDDING_DIM=128), model_dir=str(tmp_path / "short"))
    monkeypatch.setenv("XMC_SBERT_DIR", str(tmp_path / "ok"))
    assert SBERT_ENCODER(_cfg(EMBEDDING_DIM=128)).model_dir == str(tmp_path / "ok")


@pytest.fixture(scope="module")
def dir768(tmp_path_factory):
    d = tmp_path_factory.mktemp("sbert768")
    R.write_model_dir(d, 2, R.hf_config(hidden=768, layers=1, heads=12, ffn=3072, vocab=60, max_pos=40))
    return str(d)


@pytest.mark.parametrize("preset", SBERT_PRESETS)
def test_construction_from_every_sbert_preset(preset, dir768):
    from xmc_gan.model.encoder import SBERT_ENCODER
    assert len(SBERT_PRESETS) == 7
    cfg = _cfg(preset)
    assert cfg.TEXT.ENCODER_NAME == "SBERT" and cfg.TEXT.ENCODER_DIR == ""
    enc = SBERT_ENCODER(cfg, model_dir=dir768)
    assert len(enc.state_dict()) == 0 and not enc.training
    assert enc.max_seq_length == cfg.TEXT.MAX_LENGTH and enc.bert_norm == bool(cfg.TEXT.BERT_NORM) and enc.hidden == cfg.TEXT.EMBEDDING_DIM


def test_entry_points_take_sbert_dir():
    import xmc_gan.sample as sample
    import xmc_gan.train_gan as tg
    assert tg.parse_args([]).sbert_dir == "" and tg.parse_args(["--sbert_dir", "/x"]).sbert_dir == "/x"
    a = sample.parse_args(["--cfg", "c", "--checkpoint", "k", "--out", "o", "--captions", "f", "--sbert_dir", "/x"])
    assert a.sbert_dir == "/x"
