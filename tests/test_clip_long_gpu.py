"""`CLIPScorer(..., max_tokens=N)` on the GPU: one layer per tower at ViT-B/16's and ViT-L/14's geometry (197 / 257 image tokens, the text
tower at CLIP's own 77 positions) against tests/clip_ref.py in f64 on the CPU; the rule of one attention kernel per tower; that a default
scorer never reaches `ops.attention_long`; and CLIPScore end to end through `MetricSuite` at a context of 77.

Error figure: e = max |got - want| / rms(want).  Bars are computed here, not measured: 4 x e_f32, the same figure of the same restatement
(`vision_embed` / `encoder_layers` and the pooled row's LayerNorm and projection) evaluated by torch on the CPU with f32 weights on the same
inputs.  The figures each test prints are in DESIGN.md 7q."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_ref as R
from xmc_gan_amd import ops
from xmc_gan_amd.clip import CLIPScorer

DEV = torch.device("cuda", 0)
FACTOR = 4.0
WORDS = ("a man riding wave on top of surfboard two dogs play in the green grass plate food with broccoli and rice people standing near "
         "large clock tower cat sits wooden bench").split()


def _err(got, want):
    want = torch.as_tensor(want).double()
    return float((got.detach().double().cpu() - want).abs().max() / want.pow(2).mean().sqrt())


def _image_features32(w, hf, pixels):
    """`clip_ref.image_features` on f32 weights: its `vision_embed` with the patch convolution in f32, then its own layers"""
    c = hf["vision_config"]
    x = torch.nn.functional.conv2d(pixels.float(), w["vision_model.embeddings.patch_embedding.weight"], stride=c["patch_size"])
    x = x.flatten(2).transpose(1, 2)
    x = torch.cat([w["vision_model.embeddings.class_embedding"].expand(x.shape[0], 1, -1), x], 1) + w["vision_model.embeddings.position_embedding.weight"]
    x = R.layer_norm(x, w["vision_model.pre_layrnorm.weight"], w["vision_model.pre_layrnorm.bias"], c["layer_norm_eps"])
    x = R.encoder_layers(w, "vision_model.", c, x, causal=False)
    pooled = R.layer_norm(x[:, 0], w["vision_model.post_layernorm.weight"], w["vision_model.post_layernorm.bias"], c["layer_norm_eps"])
    return pooled @ w["visual_projection.weight"].t()


def _text_features32(w, hf, ids, lens):
    c = hf["text_config"]
    x = R.encoder_layers(w, "text_model.", c, R.text_embed(w, ids), causal=True)
    x = R.layer_norm(x, w["text_model.final_layer_norm.weight"], w["text_model.final_layer_norm.bias"], c["layer_norm_eps"])
    return x[torch.arange(ids.shape[0]), lens - 1] @ w["text_projection.weight"].t()


def _images(hf, n, hw, seed=3):
    img = R.sample_images(n, hw[0], hw[1], seed=seed)
    size = hf["vision_config"]["image_size"]
    return img, torch.from_numpy(R.preprocess(img, size, size))


def _towers(model, which, n_img, hw, lengths, T, max_tokens):
    """both towers against the f64 restatement, each within 4 x the f32 restatement's own error"""
    d, hf, w = model
    sc = CLIPScorer(d, DEV, max_tokens)
    img, px = _images(hf, n_img, hw)
    want = R.image_features(w, hf, px)
    bar = FACTOR * _err(_image_features32(w, hf, px), want)
    got = sc.encode_images(torch.from_numpy(img).to(DEV))
    e = _err(got, want)
    print(f"{which} image tower ({sc.tokens} tokens): e {e:.3e}, e_f32 {bar / FACTOR:.3e}, bar {bar:.3e}")
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape) and bool(torch.isfinite(got).all()) and e <= bar
    ids, lens = R.random_ids(hf, lengths, T, seed=4)
    want = R.text_features(w, hf, ids, lens)
    bar = FACTOR * _err(_text_features32(w, hf, ids, lens), want)
    got = sc.encode_text_ids(ids, lens)
    e = _err(got, want)
    print(f"{which} text tower (T {T}): e {e:.3e}, e_f32 {bar / FACTOR:.3e}, bar {bar:.3e}")
    assert tuple(got.shape) == tuple(want.shape) and bool(torch.isfinite(got).all()) and e <= bar
    return sc


def test_one_layer_at_vit_b16_geometry(tmp_path):
    """vision 768 wide, 12 heads, FFN 3072, 224 / 16 (197 tokens); text 512 wide, 8 heads, 77 positions; captions of 77, 20 and 2 tokens"""
    hf = R.hf_config(width=768, layers=1, heads=12, ffn=3072, image=224, patch=16, vocab=1000, max_pos=77, dim=512,
                     text=dict(width=512, heads=8, ffn=2048))
    hf, w = R.write_model_dir(tmp_path / "clip-b16-1layer", 7, hf)
    sc = _towers((str(tmp_path / "clip-b16-1layer"), hf, w), "b16", 2, (256, 256), [77, 20, 2], 77, 197)
    assert (sc.tokens, sc.context, sc.vision.long, sc.text.long) == (197, 77, True, True)


def test_one_layer_at_vit_l14_geometry(tmp_path):
    """vision 1024 wide, 16 heads, FFN 4096, 224 / 14 (257 tokens; the patch embedding's K is 588, a multiple of 4 and not of 8); text 768
    wide, 12 heads"""
    hf = R.hf_config(width=1024, layers=1, heads=16, ffn=4096, image=224, patch=14, vocab=1000, max_pos=77, dim=768,
                     text=dict(width=768, heads=12, ffn=3072))
    hf, w = R.write_model_dir(tmp_path / "clip-l14-1layer", 8, hf)
    sc = _towers((str(tmp_path / "clip-l14-1layer"), hf, w), "l14", 2, (256, 256), [77, 20, 2], 77, 257)
    assert (sc.tokens, sc.context, sc.g_patch.cin) == (257, 77, 588)


@pytest.fixture(scope="module")
def tiny77(tmp_path_factory):
    """the tiny model (width 128, 2 heads, 2 layers, 17 image tokens, 60 ids) with CLIP's 77 positions, and a word tokenizer"""
    d = tmp_path_factory.mktemp("clip") / "clip-tiny-77"
    hf, w = R.write_model_dir(d, 5, R.hf_config(max_pos=77), tokenizer=R.word_tokenizer(sorted(set(WORDS))))
    return str(d), hf, w


def _count(monkeypatch):
    calls = {"attention_long": 0, "attention_short": 0, "attention_causal": 0}
    for name in calls:
        def wrapped(*a, _f=getattr(ops, name), _n=name, **k):
            calls[_n] += 1
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, wrapped)
    return calls


def test_one_kernel_per_tower_and_bytes_do_not_depend_on_the_batch(tiny77, monkeypatch):
    d, hf, w = tiny77
    calls = _count(monkeypatch)
    sc = _towers(tiny77, "tiny at 77", 3, (40, 60), [77, 9, 2], 77, 77)
    assert (sc.vision.long, sc.text.long, sc.tokens, sc.context) == (False, True, 17, 77)
    assert calls == {"attention_long": 2, "attention_short": 2, "attention_causal": 0}          # 2 layers: vision short, text long
    # a caption's feature: the same bytes in a batch padded to 9 and to 77 tokens, random tokens after the EOS
    lengths = [9, 5, 2, 7]
    short, lens = R.random_ids(hf, lengths, 9, seed=4)
    long_, _ = R.random_ids(hf, lengths, 77, seed=4, fill="noise")
    a, b = sc.encode_text_ids(short, lens), sc.encode_text_ids(long_, lens)
    assert torch.equal(a, b) and torch.equal(a, sc.encode_text_ids(short, lens))
    assert calls == {"attention_long": 8, "attention_short": 2, "attention_causal": 0}          # T = 9 as well: the tower's kernel, not the batch's


def test_a_default_scorer_never_calls_attention_long(tiny77, monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("ops.attention_long was called by a scorer without max_tokens")
    monkeypatch.setattr(ops, "attention_long", refuse)
    d, hf, w = tiny77
    sc = CLIPScorer(d, DEV)
    assert (sc.context, sc.max_tokens, sc.vision.long, sc.text.long) == (64, 64, False, False)
    ids, lens = R.random_ids(hf, [64, 9, 2], 64, seed=4)
    got = sc.encode_text_ids(ids, lens)
    img, _ = _images(hf, 2, (40, 60))
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(sc.encode_images(torch.from_numpy(img).to(DEV))).all())
    with pytest.raises(ValueError, match="T <= 64"):
        sc.encode_text_ids(torch.zeros(1, 65, dtype=torch.int64), torch.tensor([65]))


def _row_err(got, want):
    """the largest relative L2 error of a feature row"""
    return float(((got.double() - want).norm(dim=1) / want.norm(dim=1)).max())


def test_metric_suite_at_context_77(tiny77):
    """a caption of 70 words: whole at a context of 77, cut at 64.  A cosine moves by at most the sum of the relative L2 errors of its two
    rows (first order), so 100 x the mean cosine, clip_score and its std are within 100 x (image bar + text bar), the bars being 4 x the
    relative row error of the f32 restatement on these inputs"""
    import tokenizers
    from xmc_gan_amd.evaluate import CLIP, MetricSuite
    d, hf, w = tiny77
    seventy = " ".join(WORDS[(7 * i) % len(WORDS)] for i in range(70))
    caps = ["a man riding a wave", seventy, "the cat sits on a wooden bench"]
    img, px = _images(hf, 6, (40, 40), seed=1)
    pairing = torch.tensor([0, 0, 1, 1, 2, 2])
    suite = MetricSuite(DEV, clip_dir=d, clip_max_tokens=77)
    suite.update_fake(torch.from_numpy(img).to(DEV), None, pairing, captions=caps)
    (metric, values, why), = list(suite.results())
    assert metric == CLIP and why is None and values["n"] == 6 and values["n_truncated"] == 0
    # the restatement at context 77
    tok, tc = tokenizers.Tokenizer.from_file(os.path.join(d, "tokenizer.json")), hf["text_config"]
    rows = [[tc["bos_token_id"]] + tok.encode(c, add_special_tokens=False).ids + [tc["eos_token_id"]] for c in caps]
    T = max(map(len, rows))
    assert T == 72
    ids, lens = torch.tensor([r + [0] * (T - len(r)) for r in rows]), torch.tensor([len(r) for r in rows])
    wi, wt = R.image_features(w, hf, px), R.text_features(w, hf, ids, lens)
    want = R.clip_score(R.cosine(wi, wt[pairing]))
    bar = 100 * FACTOR * (_row_err(_image_features32(w, hf, px), wi) + _row_err(_text_features32(w, hf, ids, lens), wt))
    e = max(abs(values["clip_score"] - want[0]), abs(values["std"] - want[1]), 100 * abs(values["cosine"] - want[2]))
    print(f"MetricSuite at context 77: clip_score {values['clip_score']:.6f} against {want[0]:.6f}; it, std and 100 x cosine within {e:.3e}, bar {bar:.3e}")
    assert e <= bar
    # the same inputs through a scorer at the default context of 64: the long caption is cut, and the score is another
    cut = MetricSuite(DEV, clip_dir=d)
    cut.update_fake(torch.from_numpy(img).to(DEV), None, pairing, captions=caps)
    (_, v64, _), = list(cut.results())
    assert v64["n_truncated"] == 1 and v64["clip_score"] != values["clip_score"] and v64["cosine"] != values["cosine"]
